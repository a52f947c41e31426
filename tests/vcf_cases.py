"""The VCF export stated by brute force: plain Python string formatting of DESIGN 4.25's line format, one cell at a time,
and the whole file from a result's fields.  Shares no code with tagdigger_amd; tests/test_vcf.py checks writeVCF's host
backend against it, tests/test_vcf_gpu.py the kernels of csrc/vcf.hip."""
import functools
import random
from fractions import Fraction

import dosage_cases as dc
import genocall_cases as gc

U32 = (1 << 32) - 1
COST_MAX = 1 << 23
CELL_MAX = 64
DEFAULT_RANGE = 256 << 20


def tables(err_ppm):
    """(CA, CB) of ploidy 2 by the dosage tests' own statement of the cost tables."""
    CA, CB, _ = dc.ref_tables(2, err_ppm)
    return list(CA), list(CB)


def gt(code, P):
    return "/".join(["."] * P if code > P else ["0"] * (P - code) + ["1"] * code)


def scaled(a, b):
    n = a + b
    return (127 * a // n, 127 * b // n) if n > 127 else (a, b)


def pl_of(a, b, CA, CB):
    x, y = scaled(a, b)
    c = [y * CA[g] + x * CB[g] for g in range(3)]
    assert max(c) - min(c) < 1 << 30
    return [min(255, ((v - min(c)) * 30103 + 327680000) // 655360000) for v in c]


def cell(a, b, code, P, lik=False, CA=None, CB=None):
    text = "%s:%d,%d:%d" % (gt(code, P), a, b, a + b)
    if lik:
        assert P == 2
        if code > 2:
            text += ":.:."
        else:
            pl = pl_of(a, b, CA, CB)
            text += ":%d:%d,%d,%d" % (min([99] + [pl[g] for g in range(3) if g != code]), pl[0], pl[1], pl[2])
    assert len(text) + 1 <= CELL_MAX
    return text


def lines(counts, i0, i1, calls, sel, prefixes, P, lik=False, CA=None, CB=None):
    """The body lines as a list of bytes, one per entry of sel."""
    out = []
    for k, m in enumerate(sel):
        cells = [cell(row[i0[m]], row[i1[m]], crow[m], P, lik, CA, CB) for row, crow in zip(counts, calls)]
        out.append(prefixes[k] + "".join("\t" + c for c in cells).encode("ascii") + b"\n")
    return out


def offsets(body):
    off = [0]
    for line in body:
        off.append(off[-1] + len(line))
    return off


def plan(lengths, budget):
    """The ranges as (first, last) pairs: consecutive lines of at most `budget` bytes together, at least one line."""
    out, k = [], 0
    while k < len(lengths):
        e, total = k + 1, lengths[k]
        while e < len(lengths) and total + lengths[e] <= budget:
            total += lengths[e]
            e += 1
        out.append((k, e))
        k = e
    return out


def prefix_bytes(k, length):
    """A prefix of exactly `length` bytes that names its line."""
    text = ("L%d|" % k).encode("ascii") * (length // 3 + 1)
    return text[:length]


def random_calls(rng, S, M, P):
    codes = list(range(P + 1)) + [P + 1, 3, 255]
    return [[rng.choice(codes) for _ in range(M)] for _ in range(S)]


def mixed(i0, i1):
    """test_mixed_layout's changes to an adjacent layout: an allele pair swapped, a shared column, two first columns exchanged."""
    i0, i1 = list(i0), list(i1)
    i0[5], i1[5] = i1[5], i0[5]
    i1[22] = i1[40]
    i0[49], i0[50] = i0[50], i0[49]
    return i0, i1


MODES = {"p2": (2, False), "p2lik": (2, True), "p4": (4, False), "p8": (8, False)}
LAYOUTS = ("adjacent", "scattered", "mixed")


@functools.lru_cache(maxsize=None)
def grid_case(S, M, layout, mode):
    """(counts, i0, i1, T, calls, prefixes, reference lines for sel = 0 .. M - 1) of the equality tests."""
    P, lik = MODES[mode]
    counts, i0, i1, T = gc.grid_case(S, M, 2 if layout == "scattered" else 0)
    if layout == "mixed":
        i0, i1 = mixed(i0, i1)
    rng = random.Random(77 + S + 1000 * P)
    calls = random_calls(rng, S, M, P)
    prefixes = [prefix_bytes(k, (7 * k) % 33) for k in range(M)]
    CA, CB = tables(10000) if lik else (None, None)
    return counts, list(i0), list(i1), T, calls, prefixes, lines(counts, i0, i1, calls, range(M), prefixes, P, lik, CA, CB)


def exact_pl(x, y, err_ppm):
    """-10 log10(L_g / L_max) of x reads of allele 0 and y of allele 1 as floats from exact rationals (60-digit decimal)."""
    import decimal
    e = Fraction(err_ppm, 1000000)
    p1 = [e, Fraction(1, 2), 1 - e]                       # a read shows allele 1 from genotype g
    like = [p ** y * (1 - p) ** x for p in p1]
    best = max(like)
    out = []
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        for v in like:
            r = v / best
            out.append(float(-10 * (decimal.Decimal(r.numerator) / decimal.Decimal(r.denominator)).log10()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the whole file from a result's fields
def snp(t0, t1):
    if len(t0) != len(t1):
        return None
    sites = [k for k in range(len(t0)) if t0[k].upper() != t1[k].upper()]
    return (t0[sites[0]].upper(), t1[sites[0]].upper()) if len(sites) == 1 else None


def place(name, k, positions):
    if positions is None:
        return "0", k + 1
    if positions == "names":
        chrom, pos, _ = name.rsplit("-", 2)
        return chrom, int(pos)
    return str(positions[name][0]), int(positions[name][1])


def file_text(markers, samples, counts, i0, i1, calls, stats, mask, P, tagseqs=None, positions=None, passing_only=True, lik=False,
              err_ppm=10000):
    """The whole VCF file as bytes.  stats: dict of lists called, alt, depth0, depth1."""
    fmt = "GT:AD:DP:GQ:PL" if lik else "GT:AD:DP"
    keep = [m for m in range(len(markers)) if mask[m] or not passing_only]
    at = {m: place(markers[m], m, positions) for m in keep}
    chroms = []
    if positions is not None:
        for m in keep:
            if at[m][0] not in chroms:
                chroms.append(at[m][0])
        keep.sort(key=lambda m: (chroms.index(at[m][0]), at[m][1], m))
    prefixes, symbolic = [], False
    for m in keep:
        bases = snp(tagseqs[i0[m]], tagseqs[i1[m]]) if tagseqs is not None else None
        symbolic = symbolic or bases is None
        ref, alt = bases or ("N", "<ALLELE1>")
        info = "NS=%d;DP=%d;AC=%d;AN=%d" % (stats["called"][m], stats["depth0"][m] + stats["depth1"][m], stats["alt"][m],
                                            P * stats["called"][m])
        prefixes.append(("%s\t%d\t%s\t%s\t%s\t.\t%s\t%s\t%s" % (at[m][0], at[m][1], markers[m], ref, alt,
                                                                  "PASS" if mask[m] else "filtered", info, fmt)).encode("ascii"))
    head = ["##fileformat=VCFv4.2", "##source=tagdigger_amd"] + ["##contig=<ID=%s>" % c for c in chroms]
    head += ['##INFO=<ID=NS,Number=1,Type=Integer,Description="Samples with a call">',
             '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads of both alleles over all samples">',
             '##INFO=<ID=AC,Number=A,Type=Integer,Description="Copies of allele 1 among the calls">',
             '##INFO=<ID=AN,Number=1,Type=Integer,Description="Allele copies among the calls">']
    if any(not mask[m] for m in keep):
        head.append('##FILTER=<ID=filtered,Description="Outside the call rate, allele frequency or heterozygosity filters">')
    head += ['##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
             '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads of allele 0 and of allele 1">',
             '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Reads of both alleles">']
    if lik:
        head += ['##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: the smallest PL of another genotype, at most 99">',
                 '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods, at most 255">']
    if symbolic:
        head.append('##ALT=<ID=ALLELE1,Description="The second tag of a marker whose tags are not one base apart">')
    head.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + list(samples)))
    CA, CB = tables(err_ppm) if lik else (None, None)
    return ("\n".join(head) + "\n").encode("ascii") + b"".join(lines(counts, i0, i1, calls, keep, prefixes, P, lik, CA, CB))


def tag_sequences(T, i0, i1, rng=None):
    """One sequence per column: the markers alternate between two tags one base apart (a SNP marker), two tags two bases
    apart and two tags of different lengths."""
    rng = rng or random.Random(5)
    seqs = [None] * T
    for m in range(len(i0)):
        base = "TGCAG" + "".join(rng.choice("ACGT") for _ in range(30))
        other = list(base)
        other[10] = {"A": "C", "C": "G", "G": "T", "T": "A"}[base[10]]
        if m % 3 == 1:
            other[20] = {"A": "C", "C": "G", "G": "T", "T": "A"}[base[20]]
        seqs[i0[m]], seqs[i1[m]] = base, "".join(other) + ("A" if m % 3 == 2 else "")
    return [s or "TGCAGNNNN" for s in seqs]


def assert_populated(calls, mask, P, tagseqs, i0, i1, missing):
    """Every GT class, a missing cell, a filtered marker, a SNP marker and a non-SNP marker occur."""
    seen = {c for row in calls for c in row}
    assert seen >= set(range(P + 1)) | {missing}, seen
    assert not all(mask) and any(mask)
    kinds = {snp(tagseqs[i0[m]], tagseqs[i1[m]]) is not None for m in range(len(i0))}
    assert kinds == {True, False}
