"""Shared by tests/test_census.py and tests/test_census_gpu.py: the census rule restated over a dict, with the
oracle's tree for the barcode + cut site lookup and its line splitting; inputs for the tests."""
import random

from oracle import tagdigger_oracle as orc

ACGT = "ACGT"


def ref_census(data, barcodes, cutsite="TGCAG", taglen=64, maxreads=5e9):
    """(census dict, statistics) of FASTQ bytes by the per-read rule: lines as text mode splits them, line k a read
    when k % 4 == 1, strip + upper, sequence_index_lookup in the tree of find_tags_fastq (:209-219), the window from
    the cut site's first base."""
    barcut, barnum, _, _ = orc.prepare_lists(barcodes, ["A"], cutsite)
    tree = orc.build_sequence_tree(barcut, barnum)
    bound = max(1, maxreads)
    census = {}
    st = dict(reads=0, barcut=0, short=0, ambiguous=0)
    for k, raw in enumerate(orc.iter_lines(data)):
        if k % 4 != 1:
            continue
        st["reads"] += 1
        line1 = orc.clean_read(raw)
        b = orc.sequence_index_lookup(line1, tree)
        if b != -1:
            st["barcut"] += 1
            w = line1[len(barcodes[b]):len(barcodes[b]) + taglen]
            if len(w) < taglen:
                st["short"] += 1
            elif not set(w) <= set(ACGT):
                st["ambiguous"] += 1
            else:
                census[w] = census.get(w, 0) + 1
        if st["reads"] >= bound:
            break
    st["counted"] = st["barcut"] - st["short"] - st["ambiguous"]
    st["distinct"] = len(census)
    return census, st


def ordered(census, min_count=1, top=None):
    """[seqs, counts]: count descending, then sequence ascending."""
    ent = sorted(((s, c) for s, c in census.items() if c >= min_count), key=lambda e: (-e[1], e[0]))
    if top is not None:
        ent = ent[:top]
    return [[e[0] for e in ent], [e[1] for e in ent]]


def ref_names(seqs, known, cutsite):
    """The known-tag annotation, the slow and obvious way."""
    names, tags = known[0], [t.upper() for t in known[1]]
    cutlen = len(cutsite)
    with_site = {t[:cutlen] for t in tags} <= set(orc.enumerate_cut_sites(cutsite.upper()))
    out = []
    for w in seqs:
        s = w if with_site else w[cutlen:]
        out.append(";".join(n for n, t in zip(names, tags) if s.startswith(t) or t.startswith(s)))
    return out


def rand_seq(rnd, n):
    return "".join(rnd.choice(ACGT) for _ in range(n))


def fastq(reads, nl="\n", quality=True):
    """FASTQ text of the given sequence lines."""
    out = []
    for i, r in enumerate(reads):
        out.append("@r%d%s%s%s+%s%s%s" % (i, nl, r, nl, nl, "I" * len(r) if quality else "I", nl))
    return "".join(out).encode("latin-1")


BARCODES_MIXED = ["ACGT", "TGACA", "GATTAC", "CCTAGGA", "TTGGCCAA", "AGAGTCTCA"]       # lengths 4..9, prefix-free


def library(rnd, nreads, barcodes=BARCODES_MIXED, sites=("TGCAG",), pool=None, lo=30, hi=160, dirt=True):
    """Sequence lines of lengths lo..hi: barcode + site + a tail from `pool` (or random), some without a barcode,
    some with an N, some too short for a window."""
    reads = []
    for _ in range(nreads):
        n = rnd.randint(lo, hi)
        roll = rnd.random() if dirt else 1.0
        if roll < 0.08:
            reads.append(rand_seq(rnd, n))
            continue
        head = rnd.choice(barcodes) + rnd.choice(sites)
        tail = rnd.choice(pool) if pool else rand_seq(rnd, 160)
        r = (head + tail)[:n]
        if roll < 0.14:
            k = rnd.randrange(len(r))
            r = r[:k] + "N" + r[k + 1:]
        elif roll < 0.18:
            r = r.lower()
        reads.append(r)
    return reads
