"""The LD edges of marker pairs on the device (csrc/ld.hip, int8 MFMA) against tests/ld_cases.py: every tile and tail, the
orientation of the result, the compaction of the mask, the 128-bit comparison at its knife edge, the capacity of the
edge buffer, more tile pairs than a grid dimension of 65 535, the limits, and the chain from the count matrix to the
edges without the calls leaving the device."""
import numpy as np
import pytest

import genocall_cases as gc
import ld_cases as lc

pytestmark = pytest.mark.gpu

TD_E_ARG, TD_E_LIMIT = -2, -7


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def tile():
    from tagdigger_amd.engine import LD_TILE
    assert LD_TILE <= 128                                  # (the shapes below stay small)
    return LD_TILE


def check(ref, got):
    lc.check_arrays(ref, got.edges, got.n, got.degree, got.called)


def test_constants_match_the_header():
    import os
    import re
    from conftest import ROOT
    from tagdigger_amd import engine
    from tagdigger_amd import tagdigger_fun as tf
    hdr = open(os.path.join(ROOT, "include", "tagdig.h")).read()
    assert int(re.search(r"TD_LD_MAX_SAMPLES = (\d+)", hdr).group(1)) == engine.LD_MAX_SAMPLES == tf.LD_MAX_SAMPLES == lc.MAX_SAMPLES
    assert 1 << int(re.search(r"TD_LD_MAX_MARKERS = 1 << (\d+)", hdr).group(1)) == engine.LD_MAX_MARKERS == tf.LD_MAX_MARKERS == lc.MAX_MARKERS
    assert int(re.search(r"TD_LD_TILE = (\d+)", hdr).group(1)) == engine.LD_TILE
    assert np.dtype(engine.LD_EDGE) == np.dtype(lc.EDGE) == np.dtype(tf.LD_EDGE) and np.dtype(lc.EDGE).itemsize == 24


@pytest.mark.parametrize("which", range(6))
def test_tiles_and_tails(eng, which):
    """Every M around the tile edge (the last with a tile pair two off the diagonal) at every S around the 16-byte load,
    the 64-sample step and beyond, without and with a mask, with every pair let in and at a real threshold; odd M puts
    the rows at odd addresses.  Codes from 0 .. 2 and 3 .. 255."""
    TILE = tile()
    M = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 2)[which]
    edges = 0
    for S in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129):
        calls = lc.structured_calls(S, M)
        for masked in (False, True):
            for min_shared, ppm in ((0, 0), (10, 800000)):
                got = eng.ld_pairs(calls, use=lc.random_mask(M) if masked else None, min_r2_ppm=ppm, min_shared=min_shared)
                ref = lc.grid_ref(S, M, masked, min_shared, ppm)
                try:
                    check(ref, got)
                except AssertionError:
                    raise AssertionError((S, M, masked, min_shared, ppm, got.n, len(ref["edges"])))
                edges += ppm > 0 and got.n
    assert edges > 0 or M == 1


def test_orientation_and_sign(eng):
    """A pair (i in tile 0, j in tile 1) with different variances and a negative cov: a transposed C/D or swapped planes,
    which symmetric data would pass, puts marker j's variance into var_i."""
    TILE = tile()
    S, M = 40, 2 * TILE + 2
    i, j = 3, TILE + 5
    calls = np.array(lc.structured_calls(S, M))
    calls[:, i] = [0, 2] * 20                              # dosages 0 / 2 against 1 / 0: var_i = 4 var_j, cov < 0
    calls[:, j] = [1, 0] * 20
    calls[7, i], calls[12, j] = 200, 3                     # and a missing call in either
    got = eng.ld_pairs(calls, min_r2_ppm=900000, min_shared=10)
    ref = lc.ld_ref(calls.tolist(), None, 10, 900000)
    check(ref, got)
    e = got.edges[(got.edges["i"] == i) & (got.edges["j"] == j)]
    assert len(e) == 1 and e["shared"][0] == 38 and e["cov"][0] < 0
    assert e["var_i"][0] == 4 * e["var_j"][0] == 38 * (19 * 4) - (19 * 2) ** 2
    # the same pair the other way round in the numbering: i in tile 1, j beyond it
    calls[:, [i, 2 * TILE + 1]] = calls[:, [2 * TILE + 1, i]]
    got = eng.ld_pairs(calls, min_r2_ppm=900000, min_shared=10)
    check(lc.ld_ref(calls.tolist(), None, 10, 900000), got)
    e = got.edges[(got.edges["i"] == j) & (got.edges["j"] == 2 * TILE + 1)]
    assert len(e) == 1 and e["cov"][0] < 0 and 4 * e["var_i"][0] == e["var_j"][0]


def test_mask_compaction(eng):
    """A mask that blanks whole tiles and leaves the participating set straddling a tile edge: the indices come back in
    the original numbering, blanked markers have degree 0 and are not counted."""
    TILE = tile()
    S, M = 33, 4 * TILE + 10
    calls = lc.structured_calls(S, M)
    use = np.zeros(M, dtype=np.uint8)
    use[TILE + 6:2 * TILE] = 1                             # TILE - 6 markers of the second tile ...
    use[3 * TILE:] = 7                                     # ... and TILE + 10 from the fourth on: compacted tiles of 64, 64, 4
    for min_shared, ppm in ((0, 0), (10, 800000)):
        got = eng.ld_pairs(calls, use=use, min_r2_ppm=ppm, min_shared=min_shared)
        ref = lc.ld_ref(calls.tolist(), use.tolist(), min_shared, ppm)
        assert len(ref["edges"]) > 0
        check(ref, got)
        assert not got.degree[use == 0].any() and not got.called[use == 0].any() and got.called[use != 0].all()
        assert use[got.edges["i"]].all() and use[got.edges["j"]].all()
        assert ((got.edges["i"] < 2 * TILE) & (got.edges["j"] >= 3 * TILE)).any()


@pytest.mark.parametrize("S", [4096, 16384])
def test_threshold_knife_edge(eng, S):
    """ppm0 = floor(10^6 cov^2 / (var_i var_j)) lets the pair in and ppm0 + 1 does not (unless the quotient is exact), at
    sizes where both sides of the comparison pass 2^64: a 64-bit product that wraps or a float decides wrongly here."""
    M = 32
    calls = lc.structured_calls(S, M)
    sums = lc.sums_numpy(calls)
    called = (calls <= 2).sum(axis=0).tolist()
    r2 = {}
    for pair, s in sums.items():
        n, cov, var_i, var_j = lc.moments(s)
        assert var_i > 0 and var_j > 0
        r2[pair] = (10 ** 6 * cov * cov // (var_i * var_j), cov, var_i, var_j)
    by = sorted(r2, key=lambda p: r2[p][0])
    tested = [by[-1], by[-2], by[-3], by[len(by) // 2], by[len(by) // 2 + 1], by[3]]
    assert r2[by[-1]][0] == 10 ** 6                        # the marker that was made twice: an exact quotient
    wide = 0
    for pair in tested:
        ppm0, cov, var_i, var_j = r2[pair]
        exact = ppm0 * var_i * var_j == 10 ** 6 * cov * cov
        wide += cov * cov * 10 ** 6 > 1 << 64 and ppm0 * var_i * var_j > 1 << 64
        got = eng.ld_pairs(calls, min_r2_ppm=ppm0, min_shared=0)
        check(lc.from_sums(sums, M, called, 0, ppm0), got)
        assert pair in set(zip(got.edges["i"].tolist(), got.edges["j"].tolist()))
        if ppm0 < 10 ** 6:
            got = eng.ld_pairs(calls, min_r2_ppm=ppm0 + 1, min_shared=0)
            check(lc.from_sums(sums, M, called, 0, ppm0 + 1), got)
            assert (pair in set(zip(got.edges["i"].tolist(), got.edges["j"].tolist()))) == exact
    assert wide >= 1


def test_capacity(eng):
    from tagdigger_amd import TagdigError
    S, M = 65, 130
    calls = lc.structured_calls(S, M)
    ref = lc.grid_ref(S, M, False, 10, 800000)
    total = len(ref["edges"])
    assert total > 20
    kw = dict(min_r2_ppm=800000, min_shared=10)
    for capacity in (0, 1, total - 1):
        with pytest.raises(TagdigError) as ei:
            eng.ld_pairs(calls, capacity=capacity, retry=False, **kw)
        err = ei.value
        assert err.code == TD_E_LIMIT and err.n == total
        assert err.degree.tolist() == ref["degree"] and err.called.tolist() == ref["called"]
    got = eng.ld_pairs(calls, capacity=total, retry=False, **kw)                       # exactly enough
    check(ref, got)
    got = eng.ld_pairs(calls, count_only=True, **kw)                                   # no buffer: counted only
    assert got.n == total and len(got.edges) == 0
    assert got.degree.tolist() == ref["degree"] and got.called.tolist() == ref["called"]
    for capacity in (0, 3, total + 100):                                               # the retry with the exact size
        check(ref, eng.ld_pairs(calls, capacity=capacity, **kw))
    # no record past the capacity is written: a buffer larger than the capacity it is announced with keeps its filling
    import ctypes as C
    from tagdigger_amd import _binding as B
    L = B.load()
    d = eng.dev_alloc(calls.nbytes)
    try:
        eng.h2d(d, calls.tobytes())
        for capacity, rc_want in ((0, TD_E_LIMIT), (5, TD_E_LIMIT), (total - 1, TD_E_LIMIT), (total, 0)):
            buf = np.full(total + 8, 0xa5, dtype=np.uint8).repeat(24).view(lc.EDGE)
            n = C.c_uint64(0)
            rc = L.td_ld_pairs(eng._h, C.c_void_p(d), S, M, None, 800000, 10, buf.ctypes.data_as(C.c_void_p), capacity,
                               C.byref(n), None, None, None)
            assert rc == rc_want and n.value == total
            written = total if rc == 0 else 0              # with TD_E_LIMIT nothing comes back at all
            assert (buf[written:].view(np.uint8) == 0xa5).all(), capacity
            if rc == 0:
                assert buf[:total].tolist() == [tuple(e) for e in ref["edges"]]
    finally:
        eng.dev_free(d)


def test_more_tile_pairs_than_a_grid_dimension(eng):
    """363 tiles are 66 066 tile pairs.  Every marker is constant (no variance, no edge) but for planted pairs at the
    corners of the triangle, across the first tile edge and in the middle; markers 0 and M - 2 are called at different
    samples, so that they meet marker M - 1 and not each other."""
    TILE = tile()
    S, M = 8, 362 * TILE + 1
    calls = np.empty((S, M), dtype=np.uint8)
    calls[:] = np.arange(M) % 5                            # constants 0 .. 4 (3 and 4: never called)
    last = [0, 1, 2, 1, 2, 0, 1, 2]
    planted = {0: [0, 1, 2, 1, 3, 3, 3, 3], M - 1: last, M - 2: [9, 9, 9, 9, 0, 2, 1, 0],         # (0, M - 1) +, (M - 2, M - 1) -
               TILE - 1: [0, 0, 1, 1, 2, 2, 0, 0], TILE: [0, 0, 1, 1, 2, 2, 0, 0],                 # (TILE - 1, TILE) +
               181 * TILE + 7: [2, 0, 0, 1, 0, 2, 1, 1], 250 * TILE + 63: [0, 2, 2, 1, 2, 0, 1, 1]}    # mid-matrix, -
    for m, col in planted.items():
        calls[:, m] = col
    got = eng.ld_pairs(calls, min_r2_ppm=1000000, min_shared=1)
    want = [(0, M - 1, 1), (TILE - 1, TILE, 1), (181 * TILE + 7, 250 * TILE + 63, -1), (M - 2, M - 1, -1)]
    assert [(int(e["i"]), int(e["j"]), int(np.sign(e["cov"]))) for e in got.edges] == want and got.n == 4
    assert [int(e["shared"]) for e in got.edges] == [4, 8, 8, 4]
    degree = np.zeros(M, dtype=np.uint32)
    for i, j, _ in want:
        degree[i] += 1
        degree[j] += 1
    assert np.array_equal(got.degree, degree)
    assert np.array_equal(got.called, (calls <= 2).sum(axis=0))
    # and the small restatement agrees on the planted columns alone
    cols = sorted(planted)
    ref = lc.ld_ref(calls[:, cols].tolist(), None, 1, 1000000)
    assert [(cols[e[0]], cols[e[1]]) + tuple(e[2:]) for e in ref["edges"]] == got.edges.tolist()


def test_arguments_and_degenerate_shapes(eng):
    from tagdigger_amd import TagdigError
    TILE = tile()
    S, M = 33, TILE + 1
    calls = lc.structured_calls(S, M)
    # neither shape lets a missing check reach memory
    for shape, kw in (((lc.MAX_SAMPLES + 1, 0), {}), ((0, 1 << 31), {}), ((2, 3), {}), ((0, 0), dict(min_r2_ppm=1000001)),
                      ((lc.MAX_SAMPLES + 1, 1 << 31), dict(min_r2_ppm=1000001))):
        with pytest.raises(TagdigError) as ei:
            eng.ld_pairs(None, shape=shape, **kw)
        assert ei.value.code == TD_E_ARG, shape
    with pytest.raises(TagdigError) as ei:
        eng.ld_pairs(calls, min_r2_ppm=1000001)
    assert ei.value.code == TD_E_ARG
    many = np.zeros((2, lc.MAX_MARKERS + 1), dtype=np.uint8)
    planted = {0: [0, 1], 12345: [0, 2], 70000: [2, 0], 600001: [1, 2], lc.MAX_MARKERS - 1: [2, 1], lc.MAX_MARKERS: [0, 2]}
    for m, col in planted.items():
        many[:, m] = col
    with pytest.raises(TagdigError) as ei:
        eng.ld_pairs(many, min_shared=0)
    assert ei.value.code == TD_E_LIMIT and str(lc.MAX_MARKERS + 1) in ei.value.detail and str(lc.MAX_MARKERS) in ei.value.detail
    use = np.ones(lc.MAX_MARKERS + 1, dtype=np.uint8)
    use[12345] = 0                                         # exactly the limit takes part: the largest grid there is, 1.3 * 10^8 tile pairs
    got = eng.ld_pairs(many, use=use, min_r2_ppm=1000000, min_shared=2, capacity=16)
    cols = sorted(planted)
    ref = lc.ld_ref(many[:, cols].tolist(), [m != 12345 for m in cols], 2, 1000000)    # two samples: any two varying markers have r^2 = 1
    assert len(ref["edges"]) == 10 and {e[3] > 0 for e in ref["edges"]} == {True, False}
    assert [(cols[e[0]], cols[e[1]]) + tuple(e[2:]) for e in ref["edges"]] == got.edges.tolist() and got.n == 10
    assert got.degree.sum() == 20 and all(got.degree[m] == 4 for m in cols if m != 12345) and got.degree[12345] == 0
    assert np.array_equal(got.called, 2 * use)
    # degenerate shapes: no edges, no degrees
    for c, kw in ((np.zeros((0, 5), dtype=np.uint8), {}), (np.zeros((3, 0), dtype=np.uint8), {}),
                  (calls, dict(use=np.zeros(M, dtype=np.uint8))),
                  (np.full((S, M), 3, dtype=np.uint8), {}), (np.full((S, M), 200, dtype=np.uint8), dict(use=np.ones(M, dtype=np.uint8)))):
        got = eng.ld_pairs(c, min_r2_ppm=0, min_shared=0, **kw)
        assert got.n == 0 and len(got.edges) == 0 and got.edges.dtype == np.dtype(lc.EDGE)
        assert got.degree.shape == (c.shape[1],) and not got.degree.any() and not got.called.any()
    one = np.zeros(M, dtype=np.uint8)
    one[TILE - 2] = 1                                      # one participating marker: counted, without a pair
    got = eng.ld_pairs(calls, use=one, min_r2_ppm=0, min_shared=0)
    assert got.n == 0 and not got.degree.any() and got.ms == 0
    assert got.called.tolist() == lc.called_ref(calls.tolist(), one.tolist()) and got.called[TILE - 2] > 0
    check(lc.grid_ref(S, M, False, 10, 800000), eng.ld_pairs(calls, min_r2_ppm=800000, min_shared=10))     # and a valid call after them


def test_determinism(eng):
    S, M = 129, 2 * tile() + 2
    calls = lc.structured_calls(S, M)
    runs = [eng.ld_pairs(calls, min_r2_ppm=0, min_shared=0) for _ in range(2)]
    assert runs[0].n > 5000 and runs[0].edges.tobytes() == runs[1].edges.tobytes()
    assert runs[0].degree.tobytes() == runs[1].degree.tobytes() and runs[0].called.tobytes() == runs[1].called.tobytes()
    assert runs[0].ms > 0 and runs[0].times["pairs_ms"] > 0 and runs[0].times["transpose_ms"] > 0


def test_from_call_genotypes_to_marker_ld():
    """counts -> td_geno_call with the calls kept on the device -> marker_ld on the DeviceCalls under the pass mask equals
    the host route on the fetched calls."""
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T = gc.grid_case(65, 260)
    samples = ["w%03d" % k for k in range(65)]
    geno = tf.call_genotypes(gc.as_array(counts, T), samples, gc.tag_names(260, i0, i1, T), backend="gpu", keep_device=True,
                             **gc.PARAMS[1])
    try:
        assert isinstance(geno.d_calls, tf.DeviceCalls) and geno.d_calls.shape == (65, 260) and geno.d_calls.ptr
        got = tf.marker_ld(geno.d_calls, geno.markers, mask=geno.mask, min_r2=0.05, min_shared=10)
    finally:
        tf.default_engine(0).dev_free(geno.d_calls.ptr)
    host = tf.marker_ld(geno.calls, geno.markers, mask=geno.mask, min_r2=0.05, min_shared=10, backend="host")
    assert 0 < geno.mask.sum() < 260 and len(host.edges) > 0
    assert got.edges.tobytes() == host.edges.tobytes() and got.r2.tolist() == host.r2.tolist() and got.phase.tolist() == host.phase.tolist()
    assert np.array_equal(got.degree, host.degree) and np.array_equal(got.called, host.called)
    assert got.stats["backend"] == "gpu" and got.stats["ms"] > 0 and got.stats["used"] == int(geno.mask.sum())
    passing = [m for m in range(260) if geno.mask[m]]
    ref = lc.ld_ref(geno.calls[:, passing].tolist(), None, 10, 50000)                  # and both equal the loop
    assert [(passing[e[0]], passing[e[1]]) + tuple(e[2:]) for e in ref["edges"]] == got.edges.tolist()
    assert tf.ld_groups(got).tolist() == tf.ld_groups(host).tolist() and tf.ld_prune(got).tolist() == tf.ld_prune(host).tolist()


def test_cli_ld_from_tag_calls(tmp_path, capsys):
    """tag_calls -i ... --ld (the calls stay on the device, the filter mask selects the markers) writes the bytes tag_ld
    writes from tag_calls' own -o file, on either backend."""
    from tagdigger_amd import tag_calls, tag_ld
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T = gc.grid_case(65, 260)
    samples = ["w%03d" % k for k in range(65)]
    f = {k: str(tmp_path / k) for k in ("counts.csv", "calls.csv", "ld1.csv", "g1.csv", "k1.txt", "rel1.csv", "ld2.csv", "g2.csv",
                                        "k2.txt", "calls3.csv", "ld3.csv", "g3.csv", "k3.txt", "rel3.csv")}
    tf.writeCounts(f["counts.csv"], counts, samples, gc.tag_names(260, i0, i1, T))
    filters = ["--err", "0.002", "--min-depth", "3", "--min-call-rate", "0.6", "--min-maf", "0.05", "--max-het", "0.75"]
    ld = ["--min-r2", "0.05", "--ld-min-shared", "10", "--max-dist", "0.3", "--min-shared", "20", "--relations-ld-pruned"]
    assert tag_calls.main(["-i", f["counts.csv"], "-o", f["calls.csv"], "--ld", f["ld1.csv"], "--ld-groups", f["g1.csv"], "--ld-keep",
                           f["k1.txt"], "--relations", f["rel1.csv"]] + filters + ld) == 0
    assert tag_ld.main(["-i", f["calls.csv"], "-o", f["ld2.csv"], "--groups", f["g2.csv"], "--keep", f["k2.txt"], "--min-r2", "0.05",
                        "--min-shared", "10"]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1].startswith("Markers: ")
    assert tag_calls.main(["-i", f["counts.csv"], "-o", f["calls3.csv"], "--ld", f["ld3.csv"], "--ld-groups", f["g3.csv"], "--ld-keep",
                           f["k3.txt"], "--relations", f["rel3.csv"], "--td-backend", "host"] + filters + ld) == 0
    for names in (("ld1.csv", "ld2.csv", "ld3.csv"), ("g1.csv", "g2.csv", "g3.csv"), ("k1.txt", "k2.txt", "k3.txt"),
                  ("rel1.csv", "rel3.csv"), ("calls.csv", "calls3.csv")):
        data = [open(f[k], "rb").read() for k in names]
        assert all(d == data[0] for d in data) and data[0].count(b"\n") > 2, names
