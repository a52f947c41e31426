"""het_threshold_table, call_genotypes(backend="host"), the writers and the tag_calls command line without a GPU,
against the rule stated by brute force in tests/genocall_cases.py."""
import csv
import math

import numpy as np
import pytest

import genocall_cases as gc


def host(counts, T, names, samples=None, **kw):
    from tagdigger_amd import tagdigger_fun as tf
    samples = ["s%d" % k for k in range(len(counts))] if samples is None else samples
    return tf.call_genotypes(gc.as_array(counts, T), samples, names, backend="host", **kw)


def test_table_values_at_one_percent():
    from tagdigger_amd import tagdigger_fun as tf
    table = tf.het_threshold_table(0.01)
    assert len(table) == 128 and table[0] == 1
    assert table[1] == 2                                   # one read is never heterozygous
    assert table[2:7] == [1] * 5
    assert table[7] == 2 and table[8] == 2                 # 0.99^6 * 0.01 = 0.00941 > 2^-7 = 0.00781
    assert table == list(gc.ref_table(10000))
    for err_ppm in (1, 2000, 250000, 499999):
        assert tf.het_threshold_table(err_ppm / 1e6) == list(gc.ref_table(err_ppm))


@pytest.mark.parametrize("err_ppm", [10000, 2000, 1, 499999])
def test_table_against_float_logs(err_ppm):
    """An independent evaluation in floating-point logarithms decides every (n, k) whose two sides differ by more than
    1 part in 10^9; the table must agree with it there."""
    from tagdigger_amd import tagdigger_fun as tf
    table = tf.het_threshold_table(err_ppm / 1e6)
    e = err_ppm / 1e6
    decided = 0
    for n in range(1, 128):
        for k in range(n // 2 + 1):
            lhs = n * math.log(0.5)
            rhs = (n - k) * math.log1p(-e) + k * math.log(e)
            if abs(lhs - rhs) <= 1e-9 * max(1.0, abs(lhs)):
                continue
            decided += 1
            assert (lhs > rhs) == (k >= table[n]), (n, k)         # the inequality is monotone in k for e < 1/2
    assert decided > 4000


@pytest.mark.parametrize("pset", [0, 1])
@pytest.mark.parametrize("rule", gc.RULES)
@pytest.mark.parametrize("M", [1, 64, 65])
@pytest.mark.parametrize("S", [1, 3, 65])
def test_host_equals_brute_force(S, M, rule, pset):
    counts, i0, i1, T = gc.grid_case(S, M)
    got = host(counts, T, gc.tag_names(M, i0, i1, T), rule=rule, **gc.PARAMS[pset])
    gc.check_result(gc.grid_ref(S, M, 0, rule, pset), got.calls, got.stats, got.mask, got.stats["passed"])
    assert got.markers == gc.marker_names(M) and got.stats["backend"] == "host"
    assert got.calls.dtype == np.uint8 and got.calls.shape == (S, M)


def test_populated_and_permuted_columns():
    gc.populated_case()                                    # (asserts that every class of the rule occurs)
    counts, i0, i1, T = gc.grid_case(65, 65, 1)
    order = gc.first_seen(i0, i1)
    got = host(counts, T, gc.tag_names(65, i0, i1, T), rule="likelihood", **gc.PARAMS[1])
    gc.check_result(gc.reordered(gc.grid_ref(65, 65, 1, "likelihood", 1), order), got.calls, got.stats, got.mask)
    assert got.markers == [gc.marker_names(65)[m] for m in order]


def test_presence_rule_writes_writeDiploidGeno_bytes(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T = gc.grid_case(65, 64)
    names = gc.tag_names(64, i0, i1, T)
    samples = ["plant %d" % k for k in range(65)]
    arr = gc.as_array(counts, T)
    old, new = str(tmp_path / "old.csv"), str(tmp_path / "new.csv")
    tf.writeDiploidGeno(old, arr, samples, names)
    tf.writeGenoCalls(new, tf.call_genotypes(arr, samples, names, rule="presence", min_depth=1, min_maf=0.3,
                                             backend="host"), passing_only=False)
    data = open(old, "rb").read()
    assert data == open(new, "rb").read() and data.count(b"\r\n") == 66
    # the same from lists of ints, as the reference's callers hold the matrix
    tf.writeDiploidGeno(old, counts, samples, names)
    assert open(old, "rb").read() == data


@pytest.mark.parametrize("counts,params,passes", gc.filter_boundary_cases())
def test_filter_boundaries(counts, params, passes):
    ref = gc.ref_calls(counts, [0], [1], rule="presence", **params)
    assert ref["mask"] == [passes]
    got = host(counts, 2, ["m_0", "m_1"], rule="presence", **params)
    gc.check_result(ref, got.calls, got.stats, got.mask, got.stats["passed"])


def test_scaling_boundary_and_extreme_counts():
    counts, i0, i1, T = gc.extreme_case()
    for rule in gc.RULES:
        for min_depth in (1, 128, 1 << 33):
            ref = gc.ref_calls(counts, i0, i1, rule=rule, min_depth=min_depth)
            got = host(counts, T, ["m_0", "m_1"], rule=rule, min_depth=min_depth)
            gc.check_result(ref, got.calls, got.stats, got.mask)
    ref = gc.ref_calls(counts, i0, i1)
    cells = dict(zip(gc.EXTREME_CELLS, (row[0] for row in ref["calls"])))
    # n = 127 is looked up as it is, n = 128 is scaled to 127 a // 128; the table at 1 % asks for 12 reads of 127
    assert cells[(120, 7)] == 0 and cells[(121, 7)] == 0 and cells[(64, 64)] == 1 and cells[(64, 63)] == 1
    assert cells[(gc.U32, gc.U32)] == 1 and cells[(gc.U32, 0)] == 0 and cells[(gc.U32, 1)] == 0 and cells[(1, gc.U32)] == 2
    assert ref["stats"]["depth0"][0] == sum(a for a, _ in gc.EXTREME_CELLS) > 1 << 34


def small_result(tf, **kw):
    #          m1_0 m1_1 m2_1 m2_0 m3_0 m3_1
    counts = [[9,   0,   4,   5,   0,   0],
              [0,   7,   0,   8,   1,   0],
              [6,   6,   0,   0,   0,   2]]
    names = ["m1_0", "m1_1", "m2_1", "m2_0", "m3_0", "m3_1"]
    return tf.call_genotypes(np.array(counts, dtype=np.uint32), ["a", "b,c", "d"], names, backend="host", **kw), names


def test_writers_byte_for_byte(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    res, names = small_result(tf, min_depth=2, min_call_rate=0.5)
    assert res.calls.tolist() == [[0, 1, 3], [2, 0, 3], [1, 3, 2]] and res.mask.tolist() == [True, True, False]
    path = str(tmp_path / "out")
    tf.writeMarkerStats(path, res)
    assert open(path, "rb").read() == (b"Marker name,called,n0,n1,n2,alt,depth0,depth1,pass\r\n"
                                       b"m1,3,1,1,1,3,15,13,1\r\n"
                                       b"m2,2,1,1,0,1,13,4,1\r\n"
                                       b"m3,1,0,0,1,2,1,2,0\r\n")
    tf.writeGenoCalls(path, res)
    assert open(path, "rb").read() == b',m1,m2\r\na,0,1\r\n"b,c",2,0\r\nd,1,\r\n'
    tf.writeGenoCalls(path, res, passing_only=False)
    assert open(path, "rb").read() == b',m1,m2,m3\r\na,0,1,\r\n"b,c",2,0,\r\nd,1,,2\r\n'
    seqs = ["TGCAGAAC", "TGCAGATC", "TGCAGGGT", "TGCAGGGG", "TGCAGCCC", "TGCATCCC"]
    tf.writeHapMap(path, res, seqs, passing_only=False)
    head = "rs#\talleles\tchrom\tpos\tstrand\tassembly#\tcenter\tprotLSID\tassayLSID\tpanelLSID\tQCcode\ta\tb,c\td\n"
    assert open(path, "rb").read() == (head +
                                       "m1\tA/T\t0\t1\t+\tNA\tNA\tNA\tNA\tNA\tNA\tA\tT\tW\n"
                                       "m2\tG/T\t0\t2\t+\tNA\tNA\tNA\tNA\tNA\tNA\tK\tG\tN\n"
                                       "m3\tG/T\t0\t3\t+\tNA\tNA\tNA\tNA\tNA\tNA\tN\tN\tT\n").encode()
    tf.writeHapMap(path, res, seqs)
    assert open(path, "rb").read().count(b"\n") == 3 and b"m3" not in open(path, "rb").read()


def test_errors(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    counts = np.ones((2, 3), dtype=np.uint32)
    with pytest.raises(Exception, match="All allele names must be '0' or '1'."):
        tf.call_genotypes(counts, ["a", "b"], ["m_0", "m_1", "m_2"], backend="host")          # three alleles
    with pytest.raises(Exception, match="All allele names must be '0' or '1'."):
        tf.call_genotypes(counts[:, :2], ["a", "b"], ["m_0", "m_2"], backend="host")          # an allele named '2'
    with pytest.raises(Exception, match="All allele names must be '0' or '1'."):
        tf.call_genotypes(counts[:, :1], ["a", "b"], ["m_0"], backend="host")                 # one allele only
    with pytest.raises(Exception, match="All allele names must be '0' or '1'."):
        tf.call_genotypes(counts[:, :2], ["a", "b"], ["m_0_0", "m_1_0"], backend="host")      # allele '0' twice
    res, names = small_result(tf)
    for seqs in (["ACGT", "ACGA", "ACGT", "AGGA", "AC", "AG"],          # m2's tags differ at two bases
                 ["ACGT", "ACGA", "ACGT", "ACG", "AC", "AG"]):           # ... or in length
        with pytest.raises(Exception, match="Marker m2"):
            tf.writeHapMap(str(tmp_path / "h"), res, seqs, passing_only=False)
    good = dict(rule="likelihood", err=0.01, min_depth=1, min_call_rate=0.0, min_maf=0.0, max_het=1.0)
    for bad in (dict(rule="bayes"), dict(err=0.0), dict(err=0.5), dict(min_depth=0), dict(min_depth=1.5),
                dict(min_call_rate=1.1), dict(min_call_rate=-0.1), dict(min_maf=0.51), dict(max_het=1.5),
                dict(backend="cpu")):
        with pytest.raises(ValueError):
            tf.call_genotypes(counts[:, :2], ["a", "b"], ["m_0", "m_1"], **dict(dict(good, backend="host"), **bad))
    with pytest.raises(OverflowError, match="2\\^32"):
        tf.call_genotypes(np.array([[1 << 32, 1]], dtype=np.int64), ["a"], ["m_0", "m_1"], backend="host")
    with pytest.raises(OverflowError):
        tf.call_genotypes(np.array([[-1, 1]], dtype=np.int64), ["a"], ["m_0", "m_1"], backend="host")
    with pytest.raises(TypeError):
        tf.call_genotypes(np.array([[1.0, 1.0]]), ["a"], ["m_0", "m_1"], backend="host")
    # a wider type whose values fit is taken
    got = tf.call_genotypes(np.array([[gc.U32, 1]], dtype=np.int64), ["a"], ["m_0", "m_1"], backend="host")
    assert got.calls.tolist() == [[0]]
    with pytest.raises(ValueError, match="DeviceCounts"):
        tf.call_genotypes(tf.DeviceCounts(4096, (1, 2)), ["a"], ["m_0", "m_1"], backend="host")
    empty = tf.call_genotypes(np.zeros((0, 2), dtype=np.uint32), [], ["m_0", "m_1"], backend="host")
    assert empty.calls.shape == (0, 1) and empty.mask.tolist() == [False]


def test_cli_counts_file_host_backend(tmp_path, capsys):
    from tagdigger_amd import tag_calls
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T, ref = gc.populated_case()
    names = ["%s_%s_%d" % (n[:7], "AC"[int(n[-1])], int(n[-1])) for n in gc.tag_names(65, i0, i1, T)]   # Mk00000_A_0, Mk00000_C_1
    samples = ["s%02d" % k for k in range(65)]
    cfile, out, stats = str(tmp_path / "counts.csv"), str(tmp_path / "calls.csv"), str(tmp_path / "stats.csv")
    tf.writeCounts(cfile, counts, samples, names)
    p = gc.PARAMS[1]
    argv = ["-i", cfile, "-o", out, "--stats", stats, "--td-backend", "host", "--err", str(p["err"]),
            "--min-depth", str(p["min_depth"]), "--min-call-rate", str(p["min_call_rate"]), "--min-maf", str(p["min_maf"]),
            "--max-het", str(p["max_het"])]
    assert tag_calls.main(argv) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    flat = [c for row in ref["calls"] for c in row]
    assert line == "Samples: 65 Markers: 65 Passed: %d Calls: %d Missing: %d" % (
        ref["passed"], len(flat) - flat.count(3), flat.count(3))
    keep = [m for m in range(65) if ref["mask"][m]]
    with open(out, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == [""] + [gc.marker_names(65)[m] for m in keep]
    assert [r[0] for r in rows[1:]] == samples
    assert [r[1:] for r in rows[1:]] == [[("0", "1", "2", "")[row[m]] for m in keep] for row in ref["calls"]]
    with open(stats, newline="") as fh:
        srows = list(csv.reader(fh))
    assert srows[1:] == [[gc.marker_names(65)[m]] + [str(ref["stats"][k][m]) for k in gc.STATS] + [str(int(ref["mask"][m]))]
                         for m in range(65)]
    # the presence rule through the command line
    assert tag_calls.main(["-i", cfile, "-o", out, "--rule", "presence", "--td-backend", "host"]) == 0
    pres = gc.ref_calls(counts, i0, i1, rule="presence")
    flat = [c for row in pres["calls"] for c in row]
    assert capsys.readouterr().out.strip().splitlines()[-1] == "Samples: 65 Markers: 65 Passed: 65 Calls: %d Missing: %d" % (
        len(flat) - flat.count(3), flat.count(3))
    with pytest.raises(Exception):
        tag_calls.main(["-o", out])                        # neither a counts file nor a library
