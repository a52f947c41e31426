"""LD-kNN imputation on the device (csrc/impute.hip) against tests/impute_cases.py, matrix and statistics exactly: every
S around the wave and the transpose step, every L around the halves of the 64-bit planes, k below and above the eligible
donors, the order of the voters, the tie, the zero total, the overlap and the confidence at their knife edges, the
division behind the weight for every overlap, no chaining between markers, the degenerate markers, the sample limit, the
arguments, and the chain from the count matrix to the filled calls without the calls leaving the device."""
import numpy as np
import pytest

import genocall_cases as gc
import impute_cases as ic

pytestmark = pytest.mark.gpu

TD_E_ARG = -2


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def run(eng, calls, nbr, k, min_overlap, ppm):
    calls, nbr = np.asarray(calls, dtype=np.uint8), np.asarray(nbr, dtype=np.int32)
    got = eng.impute_knn(calls, nbr, k=k, min_overlap=min_overlap, min_conf_ppm=ppm)
    ic.check(ic.impute_ref(calls.tolist(), nbr.tolist(), k, min_overlap, ppm), got.calls, got.stats)
    return got


def test_constants_match_the_header():
    import os
    import re
    from conftest import ROOT
    from tagdigger_amd import engine
    from tagdigger_amd import tagdigger_fun as tf
    hdr = open(os.path.join(ROOT, "include", "tagdig.h")).read()
    assert int(re.search(r"TD_IMPUTE_MAX_SAMPLES = (\d+)", hdr).group(1)) == engine.IMPUTE_MAX_SAMPLES == tf.IMPUTE_MAX_SAMPLES == ic.MAX_SAMPLES
    assert int(re.search(r"TD_IMPUTE_MAX_NBR = (\d+)", hdr).group(1)) == engine.IMPUTE_MAX_NBR == tf.IMPUTE_MAX_NBR == ic.MAX_NBR
    assert int(re.search(r"TD_IMPUTE_MAX_K = (\d+)", hdr).group(1)) == engine.IMPUTE_MAX_K == tf.IMPUTE_MAX_K == ic.MAX_K
    assert int(re.search(r"TD_IMPUTE_STATS = (\d+)", hdr).group(1)) == len(engine.IMPUTE_STATS) == len(tf.IMPUTE_STATS) == len(ic.STATS)
    assert engine.IMPUTE_STATS == tf.IMPUTE_STATS == ic.STATS


@pytest.mark.parametrize("L", ic.GRID_L)
@pytest.mark.parametrize("S", ic.GRID_S)
def test_grid(eng, S, L):
    """structured_calls with wild missing bytes at M = L + 3, the table with -1 holes at the front, in the middle and at
    the end of its rows, at every k; an unimputed cell keeps its exact byte (the reference copies the input)."""
    calls, nbr = ic.grid_calls(S, L), ic.grid_nbr(L)
    for k in ic.GRID_K:
        got = eng.impute_knn(calls, nbr, k=k, min_overlap=ic.grid_overlap(L), min_conf_ppm=ic.GRID_PPM)
        ref = ic.grid_ref(S, L, k)
        try:
            ic.check(ref, got.calls, got.stats)
        except AssertionError:
            raise AssertionError((S, L, k, got.stats.sum(axis=0).tolist(), np.array(ref[1]).sum(axis=0).tolist()))
        left = (got.calls > 2)
        assert np.array_equal(got.calls[left], calls[left]) and np.array_equal(got.calls[calls <= 2], calls[calls <= 2])


def test_grid_counts_something_in_every_column():
    """What test_grid compares against has cells imputed, left without a donor and left undecided: a kernel that does
    nothing cannot pass there.  (The donors are ranked once per shape and shared with test_grid.)"""
    totals = np.zeros(4, dtype=np.int64)
    for S in ic.GRID_S:
        for L in ic.GRID_L:
            for k in ic.GRID_K:
                totals += np.array(ic.grid_ref(S, L, k)[1]).sum(axis=0)
    ic.assert_grid_populated(totals.tolist())
    assert totals[0] == totals[1:].sum()


def test_equal_weights_the_smaller_donor_wins(eng):
    nbr = [[1], [-1]]
    for a, b in ((0, 2), (2, 0), (1, 0)):
        calls = [[3, 1], [a, 1], [b, 1]]
        assert [f[0] for f in ic.weights_ref(calls, nbr, 0, 0)] == [65536, 65536]
        got = run(eng, calls, nbr, 1, 1, 0)
        assert got.calls[0, 0] == a and got.stats[0].tolist() == [1, 1, 0, 0]


def test_two_classes_with_equal_votes_leave_the_cell(eng):
    got = run(eng, [[77, 1], [0, 1], [2, 1]], [[1], [-1]], 2, 1, 0)
    assert got.calls[0, 0] == 77 and got.stats[0].tolist() == [1, 0, 0, 1]
    got = run(eng, [[77, 1], [0, 1], [2, 1], [0, 1]], [[1], [-1]], 3, 1, 0)        # and a third voter decides
    assert got.calls[0, 0] == 0


def test_zero_total_leaves_the_cell(eng):
    calls = [[200, 0, 0], [1, 2, 2], [1, 2, 2]]                                        # every donor at dist = 2 ovl
    assert [f[0] for f in ic.weights_ref(calls, [[1, 2], [-1, -1], [-1, -1]], 0, 0)] == [0, 0]
    got = run(eng, calls, [[1, 2], [-1, -1], [-1, -1]], 2, 1, 0)
    assert got.calls[0, 0] == 200 and got.stats[0].tolist() == [1, 0, 0, 1]


def test_overlap_at_its_threshold(eng):
    nbr = [[1, 2, 3, 4]] + [[-1] * 4] * 4
    calls = [[3, 0, 1, 2, 9], [1, 0, 1, 2, 0]]                                         # the target is called at three neighbours
    assert ic.weights_ref(calls, nbr, 0, 0)[0][2] == 3
    got = run(eng, calls, nbr, 1, 3, 0)
    assert got.calls[0, 0] == 1 and got.stats[0].tolist() == [1, 1, 0, 0]
    got = run(eng, calls, nbr, 1, 4, 0)
    assert got.calls[0, 0] == 3 and got.stats[0].tolist() == [1, 0, 1, 0]


def test_confidence_at_its_threshold(eng):
    calls = [[3, 1], [0, 1], [0, 1], [1, 1], [0, 1]]                                   # V = (3 w, w, 0): 750 000 ppm exactly
    got = run(eng, calls, [[1], [-1]], 4, 1, 750000)
    assert got.calls[0, 0] == 0 and got.stats[0].tolist() == [1, 1, 0, 0]
    got = run(eng, calls, [[1], [-1]], 4, 1, 750001)
    assert got.calls[0, 0] == 3 and got.stats[0].tolist() == [1, 0, 0, 1]
    got = run(eng, calls, [[1], [-1]], 4, 1, 1000000)
    assert got.calls[0, 0] == 3
    got = run(eng, [[3, 1], [2, 1]], [[1], [-1]], 4, 1, 1000000)                       # unanimous: 10^6 ppm is reached
    assert got.calls[0, 0] == 2


def test_the_division_behind_the_weight(eng):
    """For every ovl in 1 .. 64 two voters of weights 32768 (2 ovl - 1) // ovl and 32768 (2 ovl - 2) // ovl: the confidence
    is put at floor(10^6 V[0] / total) and one above, where a weight that is off by one flips the cell."""
    calls, nbr = ic.division_case()
    cl, nl = calls.tolist(), nbr.tolist()
    ranked = ic.ranked_ref(cl, nl, 1)
    inexact = 0
    for ovl in range(1, 65):
        m = 63 + ovl
        (w1, d1, o1, x1), (w2, d2, o2, x2) = ic.weights_ref(cl, nl, m, 0)
        assert (d1, o1, x1, d2, o2, x2) == (1, ovl, 1, 2, ovl, 2) and w1 == 32768 * (2 * ovl - 1) // ovl
        inexact += 32768 * (2 * ovl - 1) % ovl != 0
        ppm0 = w1 * 10 ** 6 // (w1 + w2)
        for ppm in (ppm0, min(ppm0 + 1, 10 ** 6)):
            got = eng.impute_knn(calls, nbr, k=2, min_overlap=1, min_conf_ppm=ppm)
            ic.check(ic.vote_ref(cl, 128, ranked, 2, ppm), got.calls, got.stats)
        assert got.calls[0, m] == (0 if min(ppm0 + 1, 10 ** 6) * (w1 + w2) <= w1 * 10 ** 6 else 3)
    assert inexact == 64 - 7                       # every ovl but the powers of two


def test_no_chaining(eng):
    """Marker 0's cell of sample 0 is imputed.  Were that value read as sample 0's call at marker 0, sample 0 would share
    two neighbours with sample 1 at marker 1 and vote there; from the input it shares one and does not."""
    calls = [[3, 1, 0, 0], [2, 3, 0, 0]]
    nbr = [[2, 3], [0, 2], [-1, -1], [-1, -1]]
    got = run(eng, calls, nbr, 1, 2, 0)
    assert got.calls.tolist() == [[2, 1, 0, 0], [2, 3, 0, 0]]
    assert got.stats.tolist() == [[1, 1, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    chained = ic.impute_ref(got.calls.tolist(), nbr, 1, 2, 0)                          # what reading the output would give
    assert chained[0][1][1] == 1


def test_degenerate_markers_and_kept_bytes(eng):
    S, M = 70, 6
    calls = np.array(ic.lc.structured_calls(S, M))
    calls[:, 1] = np.arange(S) % 200 + 3                   # nobody is called at marker 1: targets without donors
    calls[5, [0, 2, 3, 4, 5]] = (250, 99, 3, 4, 5)         # sample 5 is missing at marker 0 and at all of its neighbours
    nbr = np.array([[2, 3, 4, 5], [0, 2, 3, -1], [-1, -1, -1, -1], [0, -1, 1, 4], [5, 3, 0, 1], [4, -1, -1, 0]], dtype=np.int32)
    got = run(eng, calls, nbr, 3, 1, 500000)
    assert got.stats[1].tolist() == [S, 0, S, 0] and np.array_equal(got.calls[:, 1], calls[:, 1])
    assert got.calls[5, 0] == 250 and got.stats[0, 2] >= 1
    miss2 = int((calls[:, 2] > 2).sum())
    assert miss2 > 0 and got.stats[2].tolist() == [miss2, 0, miss2, 0] and np.array_equal(got.calls[:, 2], calls[:, 2])
    assert got.stats[:, 1].sum() > 0
    left = got.calls > 2
    assert left.any() and np.array_equal(got.calls[left], calls[left]) and (calls[left] > 3).any()


def test_sample_limit(eng):
    calls, nbr = ic.big_case()
    got = eng.impute_knn(calls, nbr, k=10, min_overlap=4, min_conf_ppm=600000)
    ref = ic.impute_ref(calls.tolist(), nbr.tolist(), 10, 4, 600000)
    ic.check(ref, got.calls, got.stats)
    assert got.stats[:, 1].sum() > 100 and got.calls[ic.MAX_SAMPLES - 1, 0] <= 2
    from tagdigger_amd import TagdigError
    with pytest.raises(TagdigError) as ei:
        eng.impute_knn(None, np.full((6, 64), -1, dtype=np.int32), shape=(ic.MAX_SAMPLES + 1, 6))
    assert ei.value.code == TD_E_ARG


def test_arguments_and_degenerate_shapes(eng):
    from tagdigger_amd import TagdigError
    S, L = 65, 4
    calls, nbr = ic.grid_calls(S, L), ic.grid_nbr(L)
    M = L + 3
    for bad, where in ((3, 3), (M, 2), (M + 100, 0), (-2, 5), (-2147483648, 6)):        # itself, >= M, < -1
        table = np.array(nbr)
        table[where, 1] = bad
        with pytest.raises(TagdigError) as ei:
            eng.impute_knn(calls, table)
        assert ei.value.code == TD_E_ARG and ei.value.bad_index == where, (bad, where)
    table = np.array(nbr)
    row = int(np.nonzero((table >= 0).sum(axis=1) >= 2)[0][-1])
    have = table[row][table[row] >= 0]
    table[row, np.nonzero(table[row] == have[1])[0][0]] = have[0]                       # a marker twice
    with pytest.raises(TagdigError) as ei:
        eng.impute_knn(calls, table)
    assert ei.value.code == TD_E_ARG and ei.value.bad_index == row
    for kw in (dict(k=0), dict(k=ic.MAX_K + 1), dict(min_overlap=0), dict(min_conf_ppm=1000001)):
        with pytest.raises(TagdigError) as ei:
            eng.impute_knn(calls, nbr, **kw)
        assert ei.value.code == TD_E_ARG, kw
    for width in (0, ic.MAX_NBR + 1):
        with pytest.raises(TagdigError) as ei:
            eng.impute_knn(calls, np.full((M, width), -1, dtype=np.int32))
        assert ei.value.code == TD_E_ARG, width
    # neither shape lets a missing check reach memory
    for shape in ((ic.MAX_SAMPLES + 1, 0), (0, 1 << 31), (2, 3)):
        with pytest.raises(TagdigError) as ei:
            eng.impute_knn(None, np.full((shape[1] if shape[1] < 100 else 1, 2), -1, dtype=np.int32), shape=shape)
        assert ei.value.code == TD_E_ARG, shape
    for shape in ((0, 5), (3, 0), (0, 0)):
        got = eng.impute_knn(np.zeros(shape, dtype=np.uint8), np.full((shape[1], 3), -1, dtype=np.int32), keep_device=True)
        assert got.calls.shape == shape and got.stats.shape == (shape[1], 4) and not got.stats.any() and got.ms == 0 and not got.d_calls
    got = eng.impute_knn(calls, nbr, k=3, min_overlap=ic.grid_overlap(L), min_conf_ppm=ic.GRID_PPM)     # and a valid call after them
    ic.check(ic.grid_ref(S, L, 3), got.calls, got.stats)


def test_outputs_agree_and_repeat(eng):
    S, L = 129, 33
    calls, nbr = ic.grid_calls(S, L), ic.grid_nbr(L)
    kw = dict(k=3, min_overlap=4, min_conf_ppm=ic.GRID_PPM)
    runs = [eng.impute_knn(calls, nbr, keep_device=True, **kw) for _ in range(2)]
    try:
        on_device = [np.frombuffer(eng.d2h(r.d_calls, calls.size), dtype=np.uint8).reshape(calls.shape) for r in runs]
    finally:
        for r in runs:
            eng.dev_free(r.d_calls)
    assert runs[0].calls.tobytes() == runs[1].calls.tobytes() == on_device[0].tobytes() == on_device[1].tobytes()
    assert runs[0].stats.tobytes() == runs[1].stats.tobytes() and runs[0].stats[:, 1].sum() > 0
    assert runs[0].ms > 0 and runs[0].times["transpose_ms"] > 0 and runs[0].times["vote_ms"] > 0
    only = eng.impute_knn(calls, nbr, fetch=False, **kw)                               # statistics alone
    assert only.calls is None and only.d_calls is None and only.stats.tobytes() == runs[0].stats.tobytes()


def test_from_counts_to_imputed_calls():
    """counts -> td_geno_call with the calls kept on the device -> marker_ld on the DeviceCalls -> impute_calls on them
    equals the same through host arrays, and the loop."""
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T = gc.grid_case(65, 260)
    samples = ["w%03d" % k for k in range(65)]
    geno = tf.call_genotypes(gc.as_array(counts, T), samples, gc.tag_names(260, i0, i1, T), backend="gpu", keep_device=True,
                             **gc.PARAMS[1])
    kw = dict(l=8, k=5, min_overlap=2, min_conf=0.5)
    filled = None
    try:
        ld = tf.marker_ld(geno.d_calls, geno.markers, mask=geno.mask, min_r2=0.05, min_shared=10)
        got = tf.impute_calls(geno.d_calls, geno.markers, ld=ld, mask=geno.mask, **kw)
        filled = got.calls
        assert isinstance(filled, tf.DeviceCalls) and filled.shape == (65, 260) and filled.ptr and filled.ptr != geno.d_calls.ptr
        on_device = np.frombuffer(tf.default_engine(0).d2h(filled.ptr, 65 * 260), dtype=np.uint8).reshape(65, 260)
        own = tf.impute_calls(geno.d_calls, geno.markers, mask=geno.mask, min_r2=0.05, ld_min_shared=10, **kw)     # its own marker_ld
        own_calls = np.frombuffer(tf.default_engine(0).d2h(own.calls.ptr, 65 * 260), dtype=np.uint8).reshape(65, 260)
        tf.default_engine(0).dev_free(own.calls.ptr)
    finally:
        tf.default_engine(0).dev_free(geno.d_calls.ptr)
        if filled is not None:
            tf.default_engine(0).dev_free(filled.ptr)
    host = tf.impute_calls(geno.calls, geno.markers, mask=geno.mask, min_r2=0.05, ld_min_shared=10, backend="host", **kw)
    through = tf.impute_calls(geno.calls, geno.markers, mask=geno.mask, min_r2=0.05, ld_min_shared=10, **kw)    # host arrays, gpu backend
    assert got.imputed > 0 and got.imputed == host.imputed == through.imputed == own.imputed
    assert np.array_equal(got.neighbours, host.neighbours) and (got.neighbours[~geno.mask] == -1).all()
    for other in (host.calls, through.calls, own_calls):
        assert on_device.tobytes() == other.tobytes()
    assert np.array_equal(got.stats, host.stats) and np.array_equal(got.stats, through.stats) and got.ms > 0
    assert np.array_equal(on_device[:, ~geno.mask], geno.calls[:, ~geno.mask])
    ic.check(ic.impute_ref(geno.calls.tolist(), got.neighbours.tolist(), 5, 2, 500000), on_device, got.stats)


def test_cli_impute_from_tag_calls(tmp_path, capsys):
    """tag_calls -i ... --impute on the device (the calls stay there, the filter mask selects the markers) writes the bytes
    the host backend writes, and what tag_impute writes from tag_calls' own -o file."""
    from tagdigger_amd import tag_calls, tag_impute
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T = gc.grid_case(65, 260)
    samples = ["w%03d" % k for k in range(65)]
    f = {k: str(tmp_path / k) for k in ("counts.csv", "calls1.csv", "imp1.csv", "st1.csv", "calls2.csv", "imp2.csv", "st2.csv", "imp3.csv")}
    tf.writeCounts(f["counts.csv"], counts, samples, gc.tag_names(260, i0, i1, T))
    opts = ["--err", "0.002", "--min-depth", "3", "--min-call-rate", "0.6", "--min-maf", "0.05", "--max-het", "0.75",
            "--impute-neighbours", "8", "--impute-voters", "5", "--impute-min-r2", "0.05", "--min-overlap", "2", "--min-conf", "0.5",
            "--ld-min-shared", "10"]
    assert tag_calls.main(["-i", f["counts.csv"], "-o", f["calls1.csv"], "--impute", f["imp1.csv"], "--impute-stats", f["st1.csv"]] + opts) == 0
    out1 = capsys.readouterr().out
    assert tag_calls.main(["-i", f["counts.csv"], "-o", f["calls2.csv"], "--impute", f["imp2.csv"], "--impute-stats", f["st2.csv"],
                           "--td-backend", "host"] + opts) == 0
    assert capsys.readouterr().out == out1 and int(out1.split("Imputed: ")[1].split()[0]) > 0
    assert tag_impute.main(["-i", f["calls1.csv"], "-o", f["imp3.csv"], "-l", "8", "-k", "5", "--min-r2", "0.05", "--min-overlap", "2",
                            "--min-conf", "0.5", "--ld-min-shared", "10"]) == 0
    for names in (("calls1.csv", "calls2.csv"), ("imp1.csv", "imp2.csv", "imp3.csv"), ("st1.csv", "st2.csv")):
        data = [open(f[k], "rb").read() for k in names]
        assert all(d == data[0] for d in data) and data[0].count(b"\n") > 2, names
    assert open(f["imp1.csv"], "rb").read() != open(f["calls1.csv"], "rb").read()


def test_shared_transpose_counts_the_called_samples(eng):
    """k_calls_transpose (csrc/calls_transpose.hpp) is one kernel with two instantiations: td_ld_pairs gathers the
    participating columns through the mask's index list, td_impute_knn takes every column.  Both count the samples called
    per marker in the same pass; the three ways to ask for that number agree with numpy at the tile and step tails of
    both axes.  (A table of -1 makes k_impute leave at once after its statistics: the pre-pass alone is exercised.)"""
    rng = np.random.default_rng(20261019)
    codes = np.array([0, 1, 2, 3, 9, 255], dtype=np.uint8)
    for S in (1, 63, 64, 65):
        for M in (2, 63, 64, 65, 130):
            calls = codes[rng.integers(0, len(codes), size=(S, M))]
            want = (calls <= 2).sum(axis=0)
            keep = np.arange(M) % 3 != 2                           # drops every third marker; at least two stay
            assert np.array_equal(eng.ld_pairs(calls, count_only=True).called, want), (S, M)
            masked = eng.ld_pairs(calls, use=keep, count_only=True).called
            assert np.array_equal(masked[keep], want[keep]) and not masked[~keep].any(), (S, M)
            stats = eng.impute_knn(calls, np.full((M, 1), -1, dtype=np.int32)).stats
            assert np.array_equal(S - stats[:, 0].astype(np.int64), want), (S, M)
