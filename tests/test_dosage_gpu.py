"""Polyploid dosage calling on the device (csrc/dosage.hip) against the rule stated by brute force in
tests/dosage_cases.py."""
import csv

import numpy as np
import pytest

import dosage_cases as dc
import genocall_cases as gc
from test_genocall_gpu import LIB_BARCODES, counted_library  # noqa: F401  (the small library: two barcodes of one sample)

pytestmark = pytest.mark.gpu

TD_E_ARG = -2


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def raw_call(eng, counts, i0, i1, T, P, prior, err_ppm=10000, tables=None, **kw):
    """The raw Engine call with the test's own tables."""
    CA, CB, CP = tables or dc.ref_tables(P, err_ppm)
    return eng.dose_call(gc.as_array(counts, T), i0, i1, list(CA), list(CB), [list(r) for r in CP] if prior == "hwe" else None,
                         ploidy=P, prior=dc.PRIORS.index(prior), err_ppm=err_ppm, **kw)


@pytest.fixture(scope="module")
def raw(eng):
    def run(counts, i0, i1, T, P, prior, **kw):
        got = raw_call(eng, counts, i0, i1, T, P, prior, diploid=True, **kw)
        assert got.calls.dtype == np.uint8 and got.diploid.dtype == np.uint8 and (got.ms > 0) == (len(i0) > 0 and len(counts) > 0)
        return got.calls, got.diploid, got.stats, got.mask, got.passed
    return run


def test_chunk_sizes():
    from tagdigger_amd.engine import DOSE_CHUNK
    assert dc.GRID_S == (1, 3, DOSE_CHUNK + 1, 2 * DOSE_CHUNK + 2)


@pytest.mark.parametrize("scatter", [0, 2])
@pytest.mark.parametrize("prior", dc.PRIORS)
@pytest.mark.parametrize("P", dc.PLOIDIES)
@pytest.mark.parametrize("M", dc.GRID_M)
def test_device_equals_brute_force(raw, M, P, prior, scatter):
    dc.check_grid(raw, M, P, prior, scatter)


def test_knife_edges(raw):
    dc.check_knife_edges(raw)


def test_tie_of_the_issue(raw):
    """P = 3, a = b = 5, flat prior: dosage 1 at margin 0, missing at margin 1."""
    assert raw([[5, 5]], [0], [1], 2, 3, "flat", min_margin=0)[0].tolist() == [[1]]
    assert raw([[5, 5]], [0], [1], 2, 3, "flat", min_margin=1)[0].tolist() == [[dc.MISSING]]


def test_extremes_and_mixed_layout(raw):
    dc.check_extremes(raw)


def test_orientation(raw):
    dc.check_orientation(raw)


def test_populated_case_through_python(eng):
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T, ref = dc.populated_case()            # (asserts that every class of the rule occurs)
    par = dc.PARAMS[1]
    got = tf.call_dosage(gc.as_array(counts, T), ["s%d" % k for k in range(len(counts))], gc.tag_names(65, i0, i1, T), ploidy=6,
                         prior="hwe", err=par["err_ppm"] / 1e6, min_depth=par["min_depth"], min_margin=par["min_margin"],
                         min_call_rate=par["min_call_ppm"] / 1e6, min_maf=par["min_maf_ppm"] / 1e6, backend="gpu")
    dc.check_result(ref, got.calls, got.diploid, got.stats, got.mask, got.stats["passed"])
    assert got.backend == "gpu" and got.markers == gc.marker_names(65) and got.d_diploid is None


def test_without_the_diploidised_buffer_and_on_the_device(eng):
    counts, i0, i1, T = dc.grid_case(65, 65)
    ref = dc.grid_ref(65, 65, 0, 4, "hwe", 1)
    plain = raw_call(eng, counts, i0, i1, T, 4, "hwe", **{k: v for k, v in dc.PARAMS[1].items() if k != "err_ppm"}, err_ppm=2000)
    assert plain.diploid is None and plain.d_calls is None and plain.d_diploid is None
    dc.check_result(ref, plain.calls, None, plain.stats, plain.mask, plain.passed)
    kept = raw_call(eng, counts, i0, i1, T, 4, "hwe", fetch_calls=False, keep_device=True, keep_diploid=True,
                    **{k: v for k, v in dc.PARAMS[1].items() if k != "err_ppm"}, err_ppm=2000)
    try:
        assert kept.calls is None and kept.diploid is None and kept.d_calls and kept.d_diploid
        assert eng.d2h(kept.d_calls, 65 * 65) == plain.calls.tobytes()
        assert np.frombuffer(eng.d2h(kept.d_diploid, 65 * 65), dtype=np.uint8).reshape(65, 65).tolist() == ref["diploid"]
    finally:
        eng.dev_free(kept.d_calls)
        eng.dev_free(kept.d_diploid)
    assert kept.passed == plain.passed and all(kept.stats[k].tolist() == plain.stats[k].tolist() for k in dc.STATS)


def test_empty_inputs(eng):
    CA, CB, CP = (list(map(list, t)) if isinstance(t[0], tuple) else list(t) for t in dc.ref_tables(4, 10000))
    got = eng.dose_call(np.zeros((5, 4), dtype=np.uint32), [], [], CA, CB, CP, diploid=True)
    assert got.calls.shape == (5, 0) and got.mask.shape == (0,) and got.passed == 0 and got.ms == 0
    assert all(len(got.stats[k]) == 0 for k in dc.STATS)
    got = eng.dose_call(np.zeros((0, 4), dtype=np.uint32), [0, 2], [1, 3], CA, CB, CP)
    assert got.calls.shape == (0, 2) and got.mask.tolist() == [False, False] and got.passed == 0 and got.ms == 0
    assert all(got.stats[k].tolist() == [0, 0] for k in dc.STATS)


def test_error_paths(eng):
    from tagdigger_amd import TagdigError
    counts, i0, i1, T = dc.grid_case(3, 64)
    CA, CB, CP = dc.ref_tables(4, 10000)
    CA, CB, CP = list(CA), list(CB), [list(r) for r in CP]
    arr = gc.as_array(counts, T)

    def then_a_valid_call():
        got = eng.dose_call(arr, i0, i1, CA, CB, CP, diploid=True, **{k: v for k, v in dc.PARAMS[0].items()})
        dc.check_result(dc.grid_ref(3, 64, 0, 4, "hwe", 0), got.calls, got.diploid, got.stats, got.mask, got.passed)

    past = list(i1)
    past[17] = T
    with pytest.raises(TagdigError) as ei:
        eng.dose_call(arr, i0, past, CA, CB, CP)
    assert ei.value.code == TD_E_ARG and ei.value.bad_index == 17
    then_a_valid_call()
    same = list(i1)
    same[40] = i0[40]
    with pytest.raises(TagdigError) as ei:
        eng.dose_call(arr, i0, same, CA, CB, CP)
    assert ei.value.code == TD_E_ARG and ei.value.bad_index == 40
    for bad in (dict(ploidy=1), dict(ploidy=9), dict(err_ppm=0), dict(err_ppm=500000), dict(min_depth=0), dict(prior=2),
                dict(min_call_ppm=1000001), dict(min_maf_ppm=500001)):
        with pytest.raises(TagdigError) as ei:
            if "ploidy" in bad:                            # (tables of the length that ploidy asks for; the library refuses first)
                eng.dose_call(arr, i0, i1, [0] * 10, [0] * 10, None, prior=0, **bad)
            else:
                eng.dose_call(arr, i0, i1, CA, CB, CP, **bad)
        assert ei.value.code == TD_E_ARG and ei.value.bad_index is None
    for where in ("ca", "cb", "cp"):
        tabs = dict(ca=list(CA), cb=list(CB), cp=[list(r) for r in CP])
        if where == "cp":
            tabs["cp"][63][4] = (1 << 23) + 1
        else:
            tabs[where][2] = (1 << 23) + 1
        with pytest.raises(TagdigError) as ei:
            eng.dose_call(arr, i0, i1, tabs["ca"], tabs["cb"], tabs["cp"])
        assert ei.value.code == TD_E_ARG and ei.value.bad_index is None
    at_max = [list(r) for r in CP]
    at_max[63][4] = 1 << 23                                # the bound itself is taken
    eng.dose_call(arr, i0, i1, CA, CB, at_max)
    with pytest.raises(TagdigError) as ei:
        eng.dose_call(arr, i0, i1, CA, CB, None, prior=1)  # the HWE prior without its table
    assert ei.value.code == TD_E_ARG
    then_a_valid_call()


def test_chain_on_the_device(eng):
    """counts -> call_dosage(keep_device=True) -> sample_relations and marker_ld on the diploidised DeviceCalls: equal to
    the host route over the same diploidised matrix; for P = 2 that matrix is the dosage matrix with 255 -> 3."""
    from tagdigger_amd import tagdigger_fun as tf
    S, M = 65, 65
    counts = dc.binomial_counts(__import__("random").Random(99), S, M, 4)
    i0, i1, T = gc.adjacent(M)
    samples, names = ["s%d" % k for k in range(S)], gc.tag_names(M, i0, i1, T)
    d = eng.dev_alloc(S * T * 4)
    try:
        eng.h2d(d, gc.as_array(counts, T).tobytes())
        res = tf.call_dosage(tf.DeviceCounts(d, (S, T)), samples, names, ploidy=4, min_depth=2, min_call_rate=0.5, keep_device=True)
        try:
            ref = dc.ref_dosage(counts, i0, i1, 4, "hwe", min_depth=2, min_margin=dc.ref_margin(10), min_call_ppm=500000)
            dc.check_result(ref, res.calls, res.diploid, res.stats, res.mask, res.stats["passed"])
            assert 0 < ref["passed"] and res.d_diploid.shape == (S, M) and res.d_diploid.ptr
            rel_dev = tf.sample_relations(res.d_diploid, samples, mask=res.mask, min_shared=5, backend="gpu")
            ld_dev = tf.marker_ld(res.d_diploid, res.markers, mask=res.mask, min_shared=5, min_r2=0.2, backend="gpu")
        finally:
            eng.dev_free(res.d_diploid.ptr)
        two = tf.call_dosage(tf.DeviceCounts(d, (S, T)), samples, names, ploidy=2, prior="flat")
    finally:
        eng.dev_free(d)
    rel_host = tf.sample_relations(np.array(ref["diploid"], dtype=np.uint8), samples, mask=res.mask, min_shared=5, backend="host")
    ld_host = tf.marker_ld(np.array(ref["diploid"], dtype=np.uint8), res.markers, mask=res.mask, min_shared=5, min_r2=0.2, backend="host")
    assert rel_dev.joint.tolist() == rel_host.joint.tolist() and rel_dev.duplicates == rel_host.duplicates
    assert ld_dev.edges.tolist() == ld_host.edges.tolist() and len(ld_host.edges) > 0
    assert two.diploid.tolist() == np.where(two.calls == dc.MISSING, 3, two.calls).tolist()
    assert {0, 1, 2, 3} == set(two.diploid.reshape(-1).tolist())


def test_cli_gpu_backend_and_counting_mode(counted_library, tmp_path, capsys):  # noqa: F811
    from tagdigger_amd import tag_dosage
    from tagdigger_amd import tagdigger_fun as tf
    lib = counted_library
    names = lib["names"]
    i0, i1 = [names.index(n) for n in names[0::2]], [names.index(n) for n in names[1::2]]
    ref = dc.ref_dosage(lib["matrix"], i0, i1, 4, "hwe", min_depth=2, min_margin=dc.ref_margin(10), min_call_ppm=500000)
    flat = [c for row in ref["calls"] for c in row]
    assert len(set(flat) - {dc.MISSING}) >= 2 and 0 < ref["passed"]
    want_line = "Samples: 4 Markers: %d Ploidy: 4 Passed: %d Calls: %d Missing: %d" % (
        len(i0), ref["passed"], len(flat) - flat.count(dc.MISSING), flat.count(dc.MISSING))
    counts_csv = str(tmp_path / "counts.csv")
    files = {k: [str(tmp_path / (mode + "_" + k)) for mode in ("lib", "gpu", "host")] for k in ("dosage", "stats", "diploid")}
    filters = ["--ploidy", "4", "--min-depth", "2", "--min-call-rate", "0.5"]

    def outputs(k):
        return ["-o", files["dosage"][k], "--stats", files["stats"][k], "--diploid", files["diploid"][k]]

    assert tag_dosage.main(["-b", lib["key"], "--MergedTags", lib["markers"], "-e", "PstI", "--counts-out", counts_csv] +
                           outputs(0) + filters) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1] == want_line
    assert tag_dosage.main(["-i", counts_csv] + outputs(1) + filters) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1] == want_line
    assert tag_dosage.main(["-i", counts_csv, "--td-backend", "host"] + outputs(2) + filters) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1] == want_line
    for lib_file, gpu_file, host_file in files.values():
        with open(lib_file, "rb") as a, open(gpu_file, "rb") as b, open(host_file, "rb") as c:
            data = a.read()
            assert data == b.read() == c.read() and len(data) > 0
    expected = str(tmp_path / "expected_counts.csv")
    tf.writeCounts(expected, lib["matrix"], lib["samples"], names)
    with open(counts_csv, "rb") as a, open(expected, "rb") as b:
        assert a.read() == b.read()
    keep = [m for m in range(len(i0)) if ref["mask"][m]]
    with open(files["dosage"][0], newline="") as fh:
        rows = list(csv.reader(fh))
    assert [r[1:] for r in rows[1:]] == [["" if row[m] == dc.MISSING else str(row[m]) for m in keep] for row in ref["calls"]]
