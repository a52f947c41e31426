"""Genotype calling on the device (csrc/genocall.hip) against the rule stated by brute force in tests/genocall_cases.py."""
import csv
import random

import numpy as np
import pytest

import genocall_cases as gc
import tagnet_cases as tc

pytestmark = pytest.mark.gpu

TD_E_ARG = -2
LIB_BARCODES = ["ACGT", "TGACA", "CATG", "GGTAC", "TTCGA"]
LIB_SAMPLES = ["s0", "s1", "s2", "s1", "s3"]               # two barcodes of one sample: their rows are summed


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def raw(eng, counts, i0, i1, T, rule="likelihood", err=0.01, min_depth=1, min_call_rate=0.0, min_maf=0.0, max_het=1.0, **kw):
    """The raw Engine call with the test's own table."""
    return eng.geno_call(gc.as_array(counts, T), i0, i1, list(gc.ref_table(gc.ppm(err))), rule=gc.RULES.index(rule),
                         err_ppm=gc.ppm(err), min_depth=min_depth, min_call_ppm=gc.ppm(min_call_rate),
                         min_maf_ppm=gc.ppm(min_maf), max_het_ppm=gc.ppm(max_het), **kw)


def chunk_sizes():
    from tagdigger_amd.engine import GENO_CHUNK
    return [1, 3, GENO_CHUNK + 1, 2 * GENO_CHUNK + 2]      # 1, 3, 65, 130: one chunk, two, and three with a short last one


@pytest.mark.parametrize("scatter", [0, 2])
@pytest.mark.parametrize("rule", gc.RULES)
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 260])
def test_device_equals_brute_force(eng, M, rule, scatter):
    assert chunk_sizes() == [1, 3, 65, 130]
    for S in chunk_sizes():
        counts, i0, i1, T = gc.grid_case(S, M, scatter)
        for pset in (0, 1):
            got = raw(eng, counts, i0, i1, T, rule=rule, **gc.PARAMS[pset])
            gc.check_result(gc.grid_ref(S, M, scatter, rule, pset), got.calls, got.stats, got.mask, got.passed)
            assert got.calls.dtype == np.uint8 and got.calls.shape == (S, M) and got.ms > 0


def test_mixed_layout(eng):
    """Adjacent columns with a few markers' alleles swapped or moved: lanes that take the 8-byte load next to lanes that
    cannot, in one wave."""
    counts, i0, i1, T = gc.grid_case(65, 64)
    i0, i1 = list(i0), list(i1)
    i0[5], i1[5] = i1[5], i0[5]                            # allele 1 in front of allele 0
    i1[22] = i1[40]                                        # two markers share a column (the C-ABI takes any indices)
    i0[49], i0[50] = i0[50], i0[49]
    ref = gc.ref_calls(counts, i0, i1, **gc.PARAMS[1])
    got = raw(eng, counts, i0, i1, T, **gc.PARAMS[1])
    gc.check_result(ref, got.calls, got.stats, got.mask, got.passed)


def test_populated_case_through_python(eng):
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T, ref = gc.populated_case()           # (asserts that every class of the rule occurs)
    got = tf.call_genotypes(gc.as_array(counts, T), ["s%d" % k for k in range(len(counts))], gc.tag_names(65, i0, i1, T),
                            rule="likelihood", backend="gpu", **gc.PARAMS[1])
    gc.check_result(ref, got.calls, got.stats, got.mask, got.stats["passed"])
    assert got.stats["backend"] == "gpu" and got.markers == gc.marker_names(65)


def test_extreme_counts(eng):
    counts, i0, i1, T = gc.extreme_case()
    for rule in gc.RULES:
        for min_depth in (1, 128, 1 << 33):
            got = raw(eng, counts, i0, i1, T, rule=rule, min_depth=min_depth)
            gc.check_result(gc.ref_calls(counts, i0, i1, rule=rule, min_depth=min_depth), got.calls, got.stats, got.mask, got.passed)


@pytest.mark.parametrize("counts,params,passes", gc.filter_boundary_cases())
def test_filter_boundaries(eng, counts, params, passes):
    ref = gc.ref_calls(counts, [0], [1], rule="presence", **params)
    assert ref["mask"] == [passes]
    got = raw(eng, counts, [0], [1], 2, rule="presence", **params)
    gc.check_result(ref, got.calls, got.stats, got.mask, got.passed)


def test_all_samples_missing(eng):
    counts, i0, i1, T = gc.grid_case(65, 64)
    for min_call_rate, passed in ((0.0, 64), (0.01, 0)):
        got = raw(eng, counts, i0, i1, T, min_depth=1 << 34, min_call_rate=min_call_rate)
        ref = gc.ref_calls(counts, i0, i1, min_depth=1 << 34, min_call_rate=min_call_rate)
        assert ref["passed"] == passed and ref["stats"]["called"] == [0] * 64
        gc.check_result(ref, got.calls, got.stats, got.mask, got.passed)
    zeros = [[0] * T for _ in range(3)]
    got = raw(eng, zeros, i0, i1, T)
    gc.check_result(gc.ref_calls(zeros, i0, i1), got.calls, got.stats, got.mask, got.passed)
    assert (got.calls == 3).all()


def test_empty_inputs(eng):
    table = list(gc.ref_table(10000))
    got = eng.geno_call(np.zeros((5, 4), dtype=np.uint32), [], [], table)
    assert got.calls.shape == (5, 0) and got.mask.shape == (0,) and got.passed == 0 and got.ms == 0
    assert all(len(got.stats[k]) == 0 for k in gc.STATS)
    got = eng.geno_call(np.zeros((0, 4), dtype=np.uint32), [0, 2], [1, 3], table)
    assert got.calls.shape == (0, 2) and got.mask.tolist() == [False, False] and got.passed == 0 and got.ms == 0
    assert all(got.stats[k].tolist() == [0, 0] for k in gc.STATS)
    got = eng.geno_call(np.zeros((3, 0), dtype=np.uint32), [], [], table)
    assert got.calls.shape == (3, 0) and got.passed == 0


def test_error_paths(eng):
    from tagdigger_amd import TagdigError
    counts, i0, i1, T = gc.grid_case(3, 64)
    ref = gc.grid_ref(3, 64, 0, "likelihood", 0)

    def then_a_valid_call():
        got = raw(eng, counts, i0, i1, T)
        gc.check_result(ref, got.calls, got.stats, got.mask, got.passed)

    past = list(i1)
    past[17] = T
    with pytest.raises(TagdigError) as ei:
        raw(eng, counts, i0, past, T)
    assert ei.value.code == TD_E_ARG and ei.value.bad_index == 17
    then_a_valid_call()
    same = list(i1)
    same[40] = i0[40]
    with pytest.raises(TagdigError) as ei:
        raw(eng, counts, i0, same, T)
    assert ei.value.code == TD_E_ARG and ei.value.bad_index == 40
    then_a_valid_call()
    table = list(gc.ref_table(10000))
    arr = gc.as_array(counts, T)
    for bad in (dict(rule=2), dict(err_ppm=0), dict(err_ppm=500000), dict(min_depth=0), dict(min_call_ppm=1000001),
                dict(min_maf_ppm=500001), dict(max_het_ppm=1000001)):
        with pytest.raises(TagdigError) as ei:
            eng.geno_call(arr, i0, i1, table, **bad)
        assert ei.value.code == TD_E_ARG and ei.value.bad_index is None
    broken = list(table)
    broken[5] = 7
    with pytest.raises(TagdigError) as ei:
        eng.geno_call(arr, i0, i1, broken)
    assert ei.value.code == TD_E_ARG
    then_a_valid_call()


def test_calls_left_on_the_device(eng):
    counts, i0, i1, T = gc.grid_case(65, 65)
    full = raw(eng, counts, i0, i1, T, **gc.PARAMS[1])
    kept = raw(eng, counts, i0, i1, T, fetch_calls=False, keep_device=True, **gc.PARAMS[1])
    try:
        assert kept.calls is None and kept.d_calls
        assert eng.d2h(kept.d_calls, 65 * 65) == full.calls.tobytes()
    finally:
        eng.dev_free(kept.d_calls)
    only = raw(eng, counts, i0, i1, T, fetch_calls=False, **gc.PARAMS[1])
    assert only.calls is None and only.d_calls is None
    for got in (kept, only):
        assert got.passed == full.passed and got.mask.tolist() == full.mask.tolist()
        assert all(got.stats[k].tolist() == full.stats[k].tolist() for k in gc.STATS)


@pytest.fixture(scope="module")
def counted_library(tmp_path_factory):
    """A small library (tagnet_cases.library_fastq, barcode by barcode so that the samples differ in their alleles;
    two of the five barcodes are one sample), the markers census_markers finds in it, and the samples x tags matrix a
    read-by-read count gives."""
    from tagdigger_amd import tagdigger_fun as tf
    rng = random.Random(2026)
    seqs, counts = tc.library(rng, 35, 24, 2)
    data = b""
    for b in LIB_BARCODES:                                 # every barcode carries its own third of the tags' reads, or none
        share = [c // 3 if rng.random() < 0.6 else 0 for c in counts]
        data += tc.library_fastq(rng, seqs, share, barcodes=[b])
    d = tmp_path_factory.mktemp("genolib")
    fq, key, markers = str(d / "lib.fq"), str(d / "key.csv"), str(d / "markers.csv")
    with open(fq, "wb") as fh:
        fh.write(data)
    with open(key, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["File", "Barcode", "Sample"])
        for b, s in zip(LIB_BARCODES, LIB_SAMPLES):
            w.writerow([fq, b, s])
    census = {}
    reads = data.decode("ascii").split("\n")[1::4]
    for r in reads:
        for b in LIB_BARCODES:
            if r.startswith(b + "TGCAG") and len(r) >= len(b) + 40:
                census[r[len(b):len(b) + 40]] = census.get(r[len(b):len(b) + 40], 0) + 1
    cseqs, ccounts = tc.census_order({s: c for s, c in census.items() if c >= 2})
    found = tf.census_markers(cseqs, ccounts, backend="host")
    with open(markers, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Marker name", "Tag sequence", "Count 0", "Count 1"])
        for name, merged, (c0, c1) in zip(*found):
            w.writerow([name, merged, c0, c1])
    names, sequences = tf.readTags_Merged(markers)
    assert len(names) >= 16 and len(names) == 2 * len(found[0])
    samples = ["s0", "s1", "s2", "s3"]
    matrix = [[0] * len(sequences) for _ in samples]
    for r in reads:
        for b, s in zip(LIB_BARCODES, LIB_SAMPLES):
            if r.startswith(b + "TGCAG"):
                for t, tag in enumerate(sequences):
                    if r.startswith(tag, len(b)):
                        matrix[samples.index(s)][t] += 1
    return dict(fq=fq, key=key, markers=markers, names=names, sequences=sequences, samples=samples, matrix=matrix)


def test_calls_from_the_matrix_the_counter_filled(eng, counted_library):
    from tagdigger_amd import tagdigger_fun as tf
    lib = counted_library
    keys = tf.readBarcodeKeyfile(lib["key"])
    order, rows = tf.sample_rows(keys)
    assert order == lib["samples"]
    eng.set_index(LIB_BARCODES, lib["sequences"], "TGCAG")
    eng.count_file(lib["fq"])
    S, T = len(order), len(lib["sequences"])
    d_total = eng.dev_alloc(S * T * 4)
    try:
        eng.h2d(d_total, bytes(S * T * 4))
        eng.fold_rows(rows[lib["fq"]], d_total, S)
        _, folded = tf.combineReadCounts({lib["fq"]: eng.counts_numpy()}, keys)
        assert folded.tolist() == lib["matrix"]
        par = dict(min_depth=2, min_call_rate=0.75, min_maf=0.1)
        want = tf.call_genotypes(folded, order, lib["names"], backend="host", **par)
        i0, i1 = want.columns
        got = eng.geno_call(d_total, i0, i1, tf.het_threshold_table(0.01), shape=(S, T), min_depth=2, min_call_ppm=750000,
                            min_maf_ppm=100000)
        through = tf.call_genotypes(tf.DeviceCounts(d_total, (S, T)), order, lib["names"], backend="gpu", **par)
    finally:
        eng.dev_free(d_total)
    ref = gc.ref_calls(lib["matrix"], i0, i1, **par)
    assert {c for row in ref["calls"] for c in row} >= {0, 1, 2} and 0 < ref["passed"]
    gc.check_result(ref, want.calls, want.stats, want.mask, want.stats["passed"])
    gc.check_result(ref, got.calls, got.stats, got.mask, got.passed)
    gc.check_result(ref, through.calls, through.stats, through.mask, through.stats["passed"])
    assert through.markers == want.markers


def test_cli_counting_mode_end_to_end(counted_library, tmp_path, capsys):
    from tagdigger_amd import tag_calls
    from tagdigger_amd import tagdigger_fun as tf
    lib = counted_library
    files = {k: (str(tmp_path / ("dev_" + k)), str(tmp_path / ("host_" + k))) for k in ("calls", "stats", "hapmap")}
    counts_csv = str(tmp_path / "counts.csv")
    filters = ["--min-depth", "2", "--min-call-rate", "0.75", "--min-maf", "0.1"]

    def outputs(k):
        return ["-o", files["calls"][k], "--stats", files["stats"][k], "--hapmap", files["hapmap"][k]]

    assert tag_calls.main(["-b", lib["key"], "--MergedTags", lib["markers"], "-e", "PstI", "--counts-out", counts_csv] +
                          outputs(0) + filters) == 0
    dev_line = capsys.readouterr().out.strip().splitlines()[-1]
    assert tag_calls.main(["-i", counts_csv, "--MergedTags", lib["markers"], "--td-backend", "host"] + outputs(1) + filters) == 0
    host_line = capsys.readouterr().out.strip().splitlines()[-1]
    i0, i1 = [lib["names"].index(n) for n in lib["names"][0::2]], [lib["names"].index(n) for n in lib["names"][1::2]]
    ref = gc.ref_calls(lib["matrix"], i0, i1, min_depth=2, min_call_rate=0.75, min_maf=0.1)
    flat = [c for row in ref["calls"] for c in row]
    assert dev_line == host_line == "Samples: 4 Markers: %d Passed: %d Calls: %d Missing: %d" % (
        len(i0), ref["passed"], len(flat) - flat.count(3), flat.count(3))
    for dev, host in files.values():
        with open(dev, "rb") as a, open(host, "rb") as b:
            data = a.read()
            assert data == b.read() and len(data) > 0
    expected = str(tmp_path / "expected_counts.csv")
    tf.writeCounts(expected, lib["matrix"], lib["samples"], lib["names"])
    with open(counts_csv, "rb") as a, open(expected, "rb") as b:
        assert a.read() == b.read()
    with open(files["calls"][0], newline="") as fh:
        rows = list(csv.reader(fh))
    keep = [m for m in range(len(i0)) if ref["mask"][m]]
    assert [r[1:] for r in rows[1:]] == [[("0", "1", "2", "")[row[m]] for m in keep] for row in ref["calls"]]
