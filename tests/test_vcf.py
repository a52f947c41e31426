"""VCF export on the host: writeVCF(backend="host") against the brute force of tests/vcf_cases.py, a pinned tiny file,
positions, the PL rule against exact rationals, the library's exports and the host-checkable parts of csrc/vcf.hip
under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import dosage_cases as dc
import genocall_cases as gc
import vcf_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tagdigger_amd", "csrc")


def stats_lists(result):
    return {k: [int(v) for v in result.stats[k]] for k in ("called", "alt", "depth0", "depth1")}


def host_file(tmp_path, result, counts, **kw):
    from tagdigger_amd import tagdigger_fun as tf
    path = str(tmp_path / "host.vcf")
    info = tf.writeVCF(path, result, counts, backend="host", **kw)
    with open(path, "rb") as fh:
        data = fh.read()
    body_at = data.index(b"\n", data.index(b"#CHROM")) + 1
    assert info["backend"] == "host" and info["bytes"] == len(data) - body_at and info["lines"] == data[body_at:].count(b"\n")
    return data


def geno_populated():
    """(result, counts as lists, array, tag sequences) of the genotype tests' populated case, called on the host."""
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T, ref = gc.populated_case()
    arr = gc.as_array(counts, T)
    result = tf.call_genotypes(arr, ["s%d" % k for k in range(len(counts))], gc.tag_names(65, i0, i1, T), backend="host", **gc.PARAMS[1])
    gc.check_result(ref, result.calls, result.stats, result.mask, result.stats["passed"])
    i0, i1 = (list(c) for c in result.columns)
    seqs = vc.tag_sequences(T, i0, i1)
    vc.assert_populated(result.calls.tolist(), list(result.mask), 2, seqs, i0, i1, 3)
    return result, counts, arr, seqs


@pytest.mark.parametrize("passing_only", [True, False])
@pytest.mark.parametrize("lik", [False, True])
def test_host_equals_brute_force_diploid(tmp_path, lik, passing_only):
    result, counts, arr, seqs = geno_populated()
    i0, i1 = (list(c) for c in result.columns)
    got = host_file(tmp_path, result, arr, tagseqs=seqs, passing_only=passing_only, likelihoods=lik, err=0.002)
    want = vc.file_text(result.markers, result.samples, counts, i0, i1, result.calls.tolist(), stats_lists(result), list(result.mask), 2,
                        tagseqs=seqs, passing_only=passing_only, lik=lik, err_ppm=2000)
    assert got == want
    assert (b"\tfiltered\t" in got) == (not passing_only) and b"\t./.:" in got and b"<ALLELE1>" in got


@pytest.mark.parametrize("P", [4, 6])
def test_host_equals_brute_force_polyploid(tmp_path, P):
    import random
    from tagdigger_amd import tagdigger_fun as tf
    S, M = 33, 40
    counts = dc.binomial_counts(random.Random(90 + P), S, M, P)
    i0, i1, T = gc.adjacent(M)
    arr = gc.as_array(counts, T)
    result = tf.call_dosage(arr, ["s%d" % k for k in range(S)], gc.tag_names(M, i0, i1, T), ploidy=P, backend="host", min_call_rate=0.4,
                            min_maf=0.05)
    seqs = vc.tag_sequences(T, i0, i1)
    vc.assert_populated(result.calls.tolist(), list(result.mask), P, seqs, i0, i1, 255)
    for passing_only in (True, False):
        got = host_file(tmp_path, result, arr, tagseqs=seqs, passing_only=passing_only)
        want = vc.file_text(result.markers, result.samples, counts, i0, i1, result.calls.tolist(), stats_lists(result), list(result.mask),
                            P, tagseqs=seqs, passing_only=passing_only)
        assert got == want
    assert ("\t" + "/".join(["."] * P) + ":").encode() in got and ("\t" + "/".join(["0"] * (P - 1) + ["1"]) + ":").encode() in got
    with pytest.raises(ValueError):
        tf.writeVCF(str(tmp_path / "no.vcf"), result, arr, likelihoods=True, backend="host")


TINY = (
    '##fileformat=VCFv4.2\n'
    '##source=tagdigger_amd\n'
    '##INFO=<ID=NS,Number=1,Type=Integer,Description="Samples with a call">\n'
    '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads of both alleles over all samples">\n'
    '##INFO=<ID=AC,Number=A,Type=Integer,Description="Copies of allele 1 among the calls">\n'
    '##INFO=<ID=AN,Number=1,Type=Integer,Description="Allele copies among the calls">\n'
    '##FILTER=<ID=filtered,Description="Outside the call rate, allele frequency or heterozygosity filters">\n'
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads of allele 0 and of allele 1">\n'
    '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Reads of both alleles">\n'
    '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: the smallest PL of another genotype, at most 99">\n'
    '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods, at most 255">\n'
    '##ALT=<ID=ALLELE1,Description="The second tag of a marker whose tags are not one base apart">\n'
    '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\ts3\n'
    '0\t1\tA\tA\tC\t.\tPASS\tNS=3;DP=21;AC=3;AN=6\tGT:AD:DP:GQ:PL\t0/0:10,0:10:30:0,30,200\t1/1:0,7:7:21:140,21,0\t0/1:2,2:4:28:28,0,28\n'
    '0\t2\tB\tN\t<ALLELE1>\t.\tPASS\tNS=3;DP=26;AC=4;AN=6\tGT:AD:DP:GQ:PL\t0/1:3,4:7:39:59,0,39\t0/1:5,5:10:70:70,0,70\t1/1:0,9:9:27:180,27,0\n'
    '0\t3\tC\tC\tG\t.\tfiltered\tNS=1;DP=1;AC=0;AN=2\tGT:AD:DP:GQ:PL\t./.:0,0:0:.:.\t0/0:1,0:1:3:0,3,20\t./.:0,0:0:.:.\n'
    '0\t4\tD\tG\tA\t.\tPASS\tNS=3;DP=8000000501;AC=3;AN=6\tGT:AD:DP:GQ:PL\t0/0:200,1:201:99:0,255,255\t1/1:0,300:300:99:255,255,0\t'
    '0/1:4000000000,4000000000:8000000000:99:255,0,255\n')
TINY_COUNTS = [[10, 0, 3, 4, 0, 0, 200, 1], [0, 7, 5, 5, 1, 0, 0, 300], [2, 2, 0, 9, 0, 0, 4000000000, 4000000000]]
TINY_NAMES = ["A_0", "A_1", "B_0", "B_1", "C_0", "C_1", "D_0", "D_1"]
TINY_SEQS = ["TGCAGAAAA", "TGCAGACAA", "TGCAGTTTT", "TGCAGTTTTG", "TGCAGCCCC", "TGCAGCGCC", "TGCAGGGGG", "TGCAGGGGA"]


def tiny_result():
    from tagdigger_amd import tagdigger_fun as tf
    arr = np.array(TINY_COUNTS, dtype=np.uint32)
    return tf.call_genotypes(arr, ["s1", "s2", "s3"], TINY_NAMES, backend="host", min_call_rate=0.5), arr


def test_tiny_file_is_pinned(tmp_path):
    result, arr = tiny_result()
    got = host_file(tmp_path, result, arr, tagseqs=TINY_SEQS, passing_only=False, likelihoods=True)
    assert got.decode("ascii") == TINY
    plain = host_file(tmp_path, result, arr, passing_only=True).decode("ascii").split("\n")
    assert [ln for ln in plain if ln.startswith("##")] == [ln for ln in TINY.split("\n") if ln.startswith("##") and "FILTER" not in ln
                                                           and "ID=GQ" not in ln and "ID=PL" not in ln]
    assert plain[-4:] == ["0\t1\tA\tN\t<ALLELE1>\t.\tPASS\tNS=3;DP=21;AC=3;AN=6\tGT:AD:DP\t0/0:10,0:10\t1/1:0,7:7\t0/1:2,2:4",
                          "0\t2\tB\tN\t<ALLELE1>\t.\tPASS\tNS=3;DP=26;AC=4;AN=6\tGT:AD:DP\t0/1:3,4:7\t0/1:5,5:10\t1/1:0,9:9",
                          "0\t4\tD\tN\t<ALLELE1>\t.\tPASS\tNS=3;DP=8000000501;AC=3;AN=6\tGT:AD:DP\t0/0:200,1:201\t1/1:0,300:300\t"
                          "0/1:4000000000,4000000000:8000000000", ""]


def body_columns(data):
    return [ln.split("\t")[:3] for ln in data.decode("ascii").split("\n") if ln and not ln.startswith("#")]


def contigs(data):
    return [ln[len("##contig=<ID="):-1] for ln in data.decode("ascii").split("\n") if ln.startswith("##contig")]


def test_positions(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    counts = np.array([[5, 0] * 6, [0, 5] * 6], dtype=np.uint32)
    markers = ["chr2-0300-top", "chr1-20-top", "chr2-100-bot", "chr1-20-bot", "scaf-7-1-5-top", "chr2-100-top"]
    names = [m + "_" + a for m in markers for a in "01"]
    result = tf.call_genotypes(counts, ["x", "y"], names, backend="host")
    got = host_file(tmp_path, result, counts, positions="names")
    # chromosomes in first-seen order, then the position, ties by marker index; a name is split from the right
    assert contigs(got) == ["chr2", "chr1", "scaf-7-1"]
    assert body_columns(got) == [["chr2", "100", "chr2-100-bot"], ["chr2", "100", "chr2-100-top"], ["chr2", "300", "chr2-0300-top"],
                                 ["chr1", "20", "chr1-20-top"], ["chr1", "20", "chr1-20-bot"], ["scaf-7-1", "5", "scaf-7-1-5-top"]]
    where = {"chr2-0300-top": ("B", 9), "chr1-20-top": ("A", 9), "chr2-100-bot": ("B", 2), "chr1-20-bot": ("B", 9), "scaf-7-1-5-top": ("A", 1),
             "chr2-100-top": ("A", 9)}
    got = host_file(tmp_path, result, counts, positions=where)
    assert contigs(got) == ["B", "A"]
    assert body_columns(got) == [["B", "2", "chr2-100-bot"], ["B", "9", "chr2-0300-top"], ["B", "9", "chr1-20-bot"], ["A", "1", "scaf-7-1-5-top"],
                                 ["A", "9", "chr1-20-top"], ["A", "9", "chr2-100-top"]]
    assert got == vc.file_text(result.markers, result.samples, counts.tolist(), *(list(c) for c in result.columns), result.calls.tolist(),
                               stats_lists(result), list(result.mask), 2, positions=where)
    got = host_file(tmp_path, result, counts)
    assert contigs(got) == [] and body_columns(got) == [["0", str(k + 1), m] for k, m in enumerate(markers)]
    bad = tf.call_genotypes(counts[:, :4], ["x", "y"], ["chr1-20-top_0", "chr1-20-top_1", "Mk7_0", "Mk7_1"], backend="host")
    with pytest.raises(Exception, match="Marker Mk7: its name does not read as chrom-pos-strand"):
        tf.writeVCF(str(tmp_path / "bad.vcf"), bad, counts[:, :4], positions="names", backend="host")
    with pytest.raises(Exception, match="Marker Mk7: no position given"):
        tf.writeVCF(str(tmp_path / "bad.vcf"), bad, counts[:, :4], positions={"chr1-20-top": ("1", 20)}, backend="host")
    worse = tf.call_genotypes(counts[:, :2], ["x", "y"], ["chr1-x20-top_0", "chr1-x20-top_1"], backend="host")
    with pytest.raises(Exception, match="Marker chr1-x20-top"):
        tf.writeVCF(str(tmp_path / "bad.vcf"), worse, counts[:, :2], positions="names", backend="host")


@pytest.mark.parametrize("err_ppm", [1000, 10000, 200000])
def test_pl_rule_against_exact_rationals(err_ppm):
    """Over all 8 256 cells with x + y <= 127: the uncapped integer PL lies within 1 of -10 log10(L_g / L_max), and the
    genotype the likelihood rule calls has PL 0."""
    from tagdigger_amd import tagdigger_fun as tf
    CA, CB, _ = tf.dosage_tables(2, err_ppm / 1e6)
    assert (CA, CB) == vc.tables(err_ppm)
    het_min = tf.het_threshold_table(err_ppm / 1e6)
    worst, widest, cells = 0.0, 0, 0
    for n in range(128):
        for y in range(n + 1):
            x = n - y
            c = [y * CA[g] + x * CB[g] for g in range(3)]
            widest = max(widest, max(c) - min(c))
            pl = [((v - min(c)) * 30103 + 327680000) // 655360000 for v in c]
            worst = max([worst] + [abs(p - e) for p, e in zip(pl, vc.exact_pl(x, y, err_ppm))])
            called = 1 if min(x, y) >= het_min[n] else 0 if x >= y else 2
            assert n == 0 or pl[called] == 0, (x, y, pl, called)
            assert [min(255, p) for p in pl] == vc.pl_of(x, y, CA, CB)
            cells += 1
    assert cells == 8256 and worst < 1 and widest < 1 << 30, (worst, widest)


def test_arguments(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    result, arr = tiny_result()
    with pytest.raises(ValueError):
        tf.writeVCF(str(tmp_path / "a.vcf"), result, arr, backend="cpu")
    with pytest.raises(ValueError):
        tf.writeVCF(str(tmp_path / "a.vcf"), result, tf.DeviceCounts(0, arr.shape), backend="host")
    with pytest.raises(ValueError):
        tf.writeVCF(str(tmp_path / "a.vcf"), result, arr[:2], backend="host")


def test_library_exports_the_vcf_symbols():
    from tagdigger_amd import _binding
    out = subprocess.run(["nm", "-D", "--defined-only", _binding.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"td_vcf_format", "td_vcf_file"} <= defined and {"td_vcf_format", "td_vcf_file"} <= set(_binding.EXPORTS)
    assert not [s for s in defined if "plan_ranges" in s]


def test_range_planner_and_cell_formatter_under_sanitizers():
    """san/vcf_san: a stand-alone program over vcf_ranges.hpp and vcf_cell.hpp (the code the kernels compile), built with
    ASan and UBSan.  It loads nothing into python and needs no preloaded runtime."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "san-vcf"])
    r = subprocess.run([os.path.join(CSRC, "san", "vcf_san")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-500:], r.stderr[-3000:])
