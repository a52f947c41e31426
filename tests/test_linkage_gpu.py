"""The linkage kernels on the device (csrc/link.hip, int8 MFMA) against tests/link_cases.py: the class counts at every
alignment, every tile and tail of the pair kernel, the sign and orientation of the result, the row subset, the three
thresholds at their knife edges, the capacity of the edge buffer, more tile pairs than a row of the grid, the limits, and
the chain from the count matrix to the map without the calls leaving the device."""
import ctypes as C

import numpy as np
import pytest

import link_cases as kc

pytestmark = pytest.mark.gpu

TD_E_ARG, TD_E_LIMIT = -2, -7
GRID_MP = (1, 2, 63, 64, 65, 130)
GRID_R = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def tile():
    from tagdigger_amd.engine import LINK_TILE
    assert LINK_TILE <= 128                                # (the shapes below stay small)
    return LINK_TILE


def tab(R):
    return np.array(kc.table(R), dtype=np.int64)


def check(ref, got):
    kc.check_arrays(ref, got.edges, got.n, got.degree, got.informative)


def run(eng, calls, cls, rows=None, **th):
    R = len(calls) if rows is None else len(rows)
    return eng.link_pairs(calls, cls, tab(R), rows=rows, **th)


def test_constants_match_the_header():
    import os
    import re
    from conftest import ROOT
    from tagdigger_amd import engine
    from tagdigger_amd import tagdigger_fun as tf
    hdr = open(os.path.join(ROOT, "include", "tagdig.h")).read()
    assert int(re.search(r"TD_LINK_MAX_SAMPLES = (\d+)", hdr).group(1)) == engine.LINK_MAX_SAMPLES == tf.LINK_MAX_SAMPLES == kc.MAX_SAMPLES
    assert 1 << int(re.search(r"TD_LINK_MAX_MARKERS = 1 << (\d+)", hdr).group(1)) == engine.LINK_MAX_MARKERS == tf.LINK_MAX_MARKERS == kc.MAX_MARKERS
    assert int(re.search(r"TD_LINK_TILE = (\d+)", hdr).group(1)) == engine.LINK_TILE
    assert np.dtype(engine.LINK_EDGE) == np.dtype(kc.EDGE) == np.dtype(tf.LINK_EDGE) and np.dtype(kc.EDGE).itemsize == 24
    assert engine.LINK_NO_PART == tf.LINK_NO_PART == kc.NO_PART and engine.LINK_LOD_MIN == tf.LINK_LOD_MIN == kc.LOD_MIN
    assert tf.LINK_CLASSES == kc.CLASSES and tf.LINK_REASONS == kc.REASONS


@pytest.mark.parametrize("M", [1, 2, 15, 16, 17, 63, 64, 65, 129])
def test_counts(eng, M):
    """Every M around the 16-byte load (odd M puts the rows at odd addresses) at every R around the rows of a workgroup,
    over all rows, a permuted subset and a subset that skips the first and last row.  Codes 0 .. 255."""
    for R in (1, 2, 63, 64, 65):
        for kind in ("all", "permuted", "inner"):
            S, rows = kc.rows_around(R, kind)
            calls = kc.structured_calls(S, M)
            counts, ms = eng.link_counts(calls, rows=rows)
            assert counts.dtype == np.uint32 and counts.shape == (M, 4) and ms > 0
            assert counts.tolist() == kc.counts_ref(calls.tolist(), list(range(S)) if rows is None else rows), (R, kind)


def test_counts_of_every_byte_and_many_row_chunks(eng):
    S, M = 300, 1040                                       # two workgroups along the columns, ten along the rows
    calls = (np.arange(S * M, dtype=np.uint32).reshape(S, M) * 7 % 256).astype(np.uint8)
    assert len(np.unique(calls)) == 256
    counts, _ = eng.link_counts(calls)
    want = np.stack([(calls == 0).sum(axis=0), (calls == 1).sum(axis=0), (calls == 2).sum(axis=0), (calls > 2).sum(axis=0)], axis=1)
    assert np.array_equal(counts, want)


@pytest.mark.parametrize("Mp", GRID_MP)
def test_tiles_and_tails(eng, Mp):
    """Every count of participating markers around the tile edge (the last with a tile pair two off the diagonal) at
    every R around the 16-byte load, the 64-offspring step and beyond; all three class pairs mixed, without and with
    markers that take no part; every pair let in and real thresholds."""
    edges = 0
    for R in GRID_R:
        for holes in (0, 1):
            calls, cls = kc.structured_calls(R, kc.grid_markers(Mp, holes)), kc.mixed_cls(Mp, holes)
            for th in (kc.OFF, kc.REAL):
                got = run(eng, calls, cls, **th)
                try:
                    check(kc.grid_ref(R, Mp, holes, th), got)
                except AssertionError:
                    raise AssertionError((R, Mp, holes, th, got.n))
                edges += th is kc.REAL and got.n
    assert edges > 0 or Mp <= 2


@pytest.mark.parametrize("kind", ["permuted", "inner"])
def test_row_subset(eng, kind):
    S, Mp = 65, 65
    rows = list(kc.row_subset(S, kind))
    calls, cls = kc.structured_calls(S, Mp), kc.mixed_cls(Mp, 0)
    for th in (kc.OFF, kc.REAL):
        check(kc.grid_ref(S, Mp, 0, th, kind), run(eng, calls, cls, rows=rows, **th))


def test_sign_and_orientation(eng):
    """Pairs across the first tile edge: fully discordant (D = -R), fully concordant, D = 0 (coupling by the tie rule)
    and D = -2 with N even (repulsion).  Different informative counts at i and j show a transposed result."""
    TILE = tile()
    R, M = 40, 2 * TILE + 2
    i, j, j2, j3, j4 = 3, TILE + 5, TILE + 9, TILE + 11, 2 * TILE + 1
    calls = np.array(kc.structured_calls(R, M))
    cls = np.array(kc.mixed_cls(M, 0))
    cls[[i, j, j2, j3, j4]] = 2
    calls[:, i] = [0, 2] * 20
    calls[:, j] = 2 - calls[:, i]                          # D = -40
    calls[:, j2] = calls[:, i]                             # D = +40
    calls[:, j3] = calls[:, i]
    calls[:20, j3] = 2 - calls[:20, j3]                    # 20 concordant, 20 discordant: D = 0
    calls[:, j4] = calls[:, j3]
    calls[38, j4], calls[39, j4] = 200, 3                  # two concordant offspring missing: 18 against 20, N = 38, D = -2
    got = run(eng, calls, cls, **kc.OFF)
    check(kc.pairs_ref(calls.tolist(), range(R), cls.tolist(), **kc.OFF), got)
    by = {(int(e["i"]), int(e["j"])): (int(e["n"]), int(e["rec_phase"]) & 0x7fffffff, int(e["rec_phase"]) >> 31, int(e["lod16"])) for e in got.edges}
    assert by[i, j] == (40, 0, 1, 65536 * 40) and by[i, j2] == (40, 0, 0, 65536 * 40)
    assert by[i, j3][:3] == (40, 20, 0) and abs(by[i, j3][3]) <= 2           # (the LOD of r = 1 / 2: 0 but for the table's rounding)
    n, rec, phase, _ = by[i, j4]
    assert (n, rec, phase) == (38, 18, 1)
    assert got.informative[i] == 40 and got.informative[j4] == 38


def test_the_signed_accumulator_at_its_limit(eng):
    """R = 16384 fully discordant across the tile edge: D reaches -16384 and N 16384."""
    TILE = tile()
    R, M = kc.MAX_SAMPLES, TILE + 2
    rng = np.random.default_rng(12)
    calls = rng.integers(0, 4, size=(R, M), dtype=np.uint8)
    calls[:, 0] = np.arange(R) % 2 * 2
    calls[:, M - 1] = 2 - calls[:, 0]
    cls = np.array(kc.mixed_cls(M, 0))
    cls[[0, M - 1]] = 2
    th = dict(max_rf_ppm=100000, min_lod16=kc.min_lod16("3"), min_shared=50)
    got = run(eng, calls, cls, **th)
    sums = kc.sums_numpy(calls, range(R), cls.tolist())
    informative = [int(np.isin(calls[:, m], kc.CLASSES[int(k)]).sum()) for m, k in enumerate(cls)]
    check(kc.from_sums(sums, M, informative, R, **th), got)
    e = got.edges[(got.edges["i"] == 0) & (got.edges["j"] == M - 1)]
    assert len(e) == 1 and e["n"][0] == R and e["rec_phase"][0] == 1 << 31 and e["lod16"][0] == 65536 * R
    assert sums[0, M - 1] == (R, -R)


def test_parents_are_excluded(eng):
    """Changing the bytes of rows that `rows` omits changes no output."""
    S, Mp = 67, 65
    calls = np.array(kc.structured_calls(S, Mp))
    cls = kc.mixed_cls(Mp, 0)
    rows = list(range(2, S))
    a = run(eng, calls, cls, rows=rows, **kc.REAL)
    ca, _ = eng.link_counts(calls, rows=rows)
    calls[:2] = (calls[:2] + 1) % 3
    b = run(eng, calls, cls, rows=rows, **kc.REAL)
    cb, _ = eng.link_counts(calls, rows=rows)
    assert a.n > 0 and a.edges.tobytes() == b.edges.tobytes() and np.array_equal(ca, cb)
    assert np.array_equal(a.degree, b.degree) and np.array_equal(a.informative, b.informative)
    c = run(eng, calls, cls, rows=[0] + rows, **kc.REAL)                                # ... and they do count when listed
    assert not np.array_equal(c.informative, a.informative)


def test_threshold_knife_edges(eng):
    cls = np.array([2, 2], dtype=np.uint8)
    f = kc.table(120)

    def edge(calls, **th):
        got = run(eng, calls, cls, **th)
        check(kc.pairs_ref(calls.tolist(), range(len(calls)), cls.tolist(), **th), got)
        return got.n == 1

    for repulsion in (False, True):
        calls = kc.two_markers(100, 20, repulsion, extra=7)                             # N = 100, rec = 20
        lod16 = 65536 * 100 + f[20] + f[80] - f[100]
        assert lod16 > 0
        # rec 10^6 == max_rf_ppm N, and one off
        assert edge(calls, max_rf_ppm=200000, min_lod16=kc.LOD_MIN, min_shared=0)
        assert not edge(calls, max_rf_ppm=199999, min_lod16=kc.LOD_MIN, min_shared=0)
        # lod16 == min_lod16, and one off
        assert edge(calls, max_rf_ppm=500000, min_lod16=lod16, min_shared=0)
        assert not edge(calls, max_rf_ppm=500000, min_lod16=lod16 + 1, min_shared=0)
        # N == min_shared, and one off
        assert edge(calls, max_rf_ppm=500000, min_lod16=kc.LOD_MIN, min_shared=100)
        assert not edge(calls, max_rf_ppm=500000, min_lod16=kc.LOD_MIN, min_shared=101)
        got = run(eng, calls, cls, **kc.OFF)
        assert got.edges.tolist() == [(0, 1, 100, 20 | int(repulsion) << 31, lod16)]
    # a pair whose lod16 is negative: an edge below 0 only
    neg = [(n, rec) for n in range(2, 121) for rec in range(n // 2 + 1) if 65536 * n + f[rec] + f[n - rec] - f[n] < 0]
    assert neg
    n, rec = neg[0]
    lod16 = 65536 * n + f[rec] + f[n - rec] - f[n]
    calls = kc.two_markers(n, rec)
    assert lod16 in (-1, -2)
    assert not edge(calls, max_rf_ppm=500000, min_lod16=0, min_shared=0)
    assert edge(calls, max_rf_ppm=500000, min_lod16=lod16, min_shared=0)
    assert not edge(calls, max_rf_ppm=500000, min_lod16=lod16 + 1, min_shared=0)
    assert edge(calls, max_rf_ppm=500000, min_lod16=kc.LOD_MIN, min_shared=0)


def test_capacity(eng):
    from tagdigger_amd import TagdigError
    from tagdigger_amd import _binding as B
    S, Mp = 65, 130
    calls, cls = kc.structured_calls(S, Mp), kc.mixed_cls(Mp, 0)
    ref = kc.grid_ref(S, Mp, 0, kc.REAL)
    total = len(ref["edges"])
    assert total > 20
    for capacity in (0, 1, total - 1):
        with pytest.raises(TagdigError) as ei:
            run(eng, calls, cls, capacity=capacity, retry=False, **kc.REAL)
        err = ei.value
        assert err.code == TD_E_LIMIT and err.n == total
        assert err.degree.tolist() == ref["degree"] and err.informative.tolist() == ref["informative"]
    check(ref, run(eng, calls, cls, capacity=total, retry=False, **kc.REAL))             # exactly enough
    got = run(eng, calls, cls, count_only=True, **kc.REAL)                               # no buffer: counted only
    assert got.n == total and len(got.edges) == 0
    assert got.degree.tolist() == ref["degree"] and got.informative.tolist() == ref["informative"]
    for capacity in (0, 3, total + 100):                                                 # the retry with the exact size
        check(ref, run(eng, calls, cls, capacity=capacity, **kc.REAL))
    # no record past the capacity is written: a buffer larger than the capacity it is announced with keeps its filling
    L = B.load()
    lodtab = tab(S)
    d = eng.dev_alloc(calls.nbytes)
    try:
        eng.h2d(d, calls.tobytes())
        for capacity, rc_want in ((0, TD_E_LIMIT), (5, TD_E_LIMIT), (total - 1, TD_E_LIMIT), (total, 0)):
            buf = np.full(total + 8, 0xa5, dtype=np.uint8).repeat(24).view(kc.EDGE)
            n = C.c_uint64(0)
            rc = L.td_link_pairs(eng._h, C.c_void_p(d), S, Mp, None, S, cls.ctypes.data_as(C.c_void_p), lodtab.ctypes.data_as(C.c_void_p),
                                 kc.REAL["max_rf_ppm"], kc.REAL["min_lod16"], kc.REAL["min_shared"], buf.ctypes.data_as(C.c_void_p), capacity,
                                 C.byref(n), None, None, None)
            assert rc == rc_want and n.value == total
            written = total if rc == 0 else 0              # with TD_E_LIMIT nothing comes back at all
            assert (buf[written:].view(np.uint8) == 0xa5).all(), capacity
            if rc == 0:
                assert buf[:total].tolist() == [tuple(e) for e in ref["edges"]]
    finally:
        eng.dev_free(d)


def test_more_tile_pairs_than_a_row_of_the_grid(eng):
    """256 tiles are 32 896 tile pairs, more than the 32 768 of a row of the grid, at R = 1.  Every marker is
    uninformative (its one cell is a heterozygote under the class pair 0 / 2) but for planted ones at the corners of the
    triangle, across the first tile edge and in the middle: every pair of those is an edge with N = 1."""
    TILE = tile()
    M = 255 * TILE + 1
    calls = np.ones((1, M), dtype=np.uint8)
    planted = {0: 0, TILE - 1: 2, TILE: 2, 100 * TILE + 7: 0, 181 * TILE + 63: 2, M - 2: 0, M - 1: 2}
    for m, c in planted.items():
        calls[0, m] = c
    cls = np.full(M, 2, dtype=np.uint8)
    th = dict(max_rf_ppm=0, min_lod16=1, min_shared=1)
    got = run(eng, calls, cls, **th)
    cols = sorted(planted)
    ref = kc.pairs_ref(calls[:, cols].tolist(), [0], [2] * len(cols), **th)
    assert len(ref["edges"]) == 21 and {e[3] >> 31 for e in ref["edges"]} == {0, 1}
    assert [(cols[e[0]], cols[e[1]]) + tuple(e[2:]) for e in ref["edges"]] == got.edges.tolist() and got.n == 21
    want = np.zeros(M, dtype=np.uint32)
    want[cols] = 6
    assert np.array_equal(got.degree, want) and np.array_equal(got.informative, want // 6)


def test_limits_and_argument_errors(eng):
    """Every error the header lists; a NULL matrix shows that the check came before anything was read."""
    from tagdigger_amd import TagdigError
    from tagdigger_amd import _binding as B
    S, M = 10, 20
    calls = kc.structured_calls(S, M)
    cls = np.array(kc.mixed_cls(M, 0))
    lod = tab(S)

    def arg(code, call):
        with pytest.raises(TagdigError) as ei:
            call()
        assert ei.value.code == code
        return ei.value.detail

    for fn in (lambda **kw: eng.link_counts(None, **kw), lambda **kw: eng.link_pairs(None, cls, lod, **kw)):
        assert "rows[2]" in arg(TD_E_ARG, lambda: fn(shape=(S, M), rows=[1, 2, S, 3]))                   # a row index >= S
        assert "twice" in arg(TD_E_ARG, lambda: fn(shape=(S, M), rows=[1, 2, 3, 2]))                     # a row listed twice
        assert "NULL call matrix" in arg(TD_E_ARG, lambda: fn(shape=(S, M)))                             # no matrix with R M > 0
        assert "NULL call matrix" in arg(TD_E_ARG, lambda: fn(shape=(S, M), rows=[4, 1]))
    arg(TD_E_ARG, lambda: eng.link_counts(None, shape=(kc.MAX_SAMPLES + 1, 0)))                          # R above the limit
    arg(TD_E_ARG, lambda: eng.link_counts(None, shape=(0, 1 << 31)))                                     # M >= 2^31
    arg(TD_E_ARG, lambda: eng.link_pairs(None, None, tab(0), shape=(kc.MAX_SAMPLES + 1, 0)))
    arg(TD_E_ARG, lambda: eng.link_pairs(None, None, tab(0), shape=(0, 1 << 31)))
    for bad in (3, 4, 128, 254):                                                                         # a cls byte outside {0, 1, 2, 255}
        wrong = cls.copy()
        wrong[7] = bad
        assert "cls[7]" in arg(TD_E_ARG, lambda: eng.link_pairs(None, wrong, lod, shape=(S, M)))
    assert "max_rf_ppm" in arg(TD_E_ARG, lambda: eng.link_pairs(None, cls, lod, shape=(S, M), max_rf_ppm=500001))
    assert "lodtab" in arg(TD_E_ARG, lambda: eng.link_pairs(None, cls, None, shape=(S, M)))
    assert "cls" in arg(TD_E_ARG, lambda: eng.link_pairs(None, None, lod, shape=(S, M)))
    # rows == NULL with R != S, and a NULL counts_out: through the library itself
    L = B.load()
    out = np.zeros((M, 4), dtype=np.uint32)
    assert L.td_link_counts(eng._h, None, S, M, None, S - 1, out.ctypes.data_as(C.c_void_p), None) == TD_E_ARG
    assert L.td_link_counts(eng._h, None, 0, M, None, 0, None, None) == TD_E_ARG
    assert L.td_link_counts(None, None, 0, 0, None, 0, None, None) == TD_E_ARG
    n = C.c_uint64(7)
    assert L.td_link_pairs(eng._h, None, S, M, None, S - 1, cls.ctypes.data_as(C.c_void_p), lod.ctypes.data_as(C.c_void_p), 0, 0, 0, None, 0,
                           C.byref(n), None, None, None) == TD_E_ARG and n.value == 0
    # more participating markers than the limit
    detail = arg(TD_E_LIMIT, lambda: eng.link_pairs(None, np.zeros(kc.MAX_MARKERS + 1, dtype=np.uint8), tab(2), shape=(2, kc.MAX_MARKERS + 1)))
    assert str(kc.MAX_MARKERS + 1) in detail and str(kc.MAX_MARKERS) in detail
    # degenerate shapes: no edges, nothing informative
    for c, k in ((np.zeros((0, 5), dtype=np.uint8), np.zeros(5, dtype=np.uint8)), (np.zeros((3, 0), dtype=np.uint8), np.zeros(0, dtype=np.uint8)),
                 (np.array(calls), np.full(M, kc.NO_PART, dtype=np.uint8)), (np.full((S, M), 200, dtype=np.uint8), cls)):
        got = run(eng, c, k, **kc.REAL)
        assert got.n == 0 and len(got.edges) == 0 and got.edges.dtype == np.dtype(kc.EDGE) and got.degree.shape == (c.shape[1],)
        assert not got.informative.any() and not got.degree.any()
        counts, _ = eng.link_counts(c)
        assert counts.shape == (c.shape[1], 4) and counts.sum() == c.size
    one = np.full(M, kc.NO_PART, dtype=np.uint8)
    one[11] = 1                                            # one participating marker: informative, without a pair
    got = run(eng, calls, one, **kc.OFF)
    assert got.n == 0 and not got.degree.any()
    assert got.informative.tolist() == kc.informative_ref(calls.tolist(), range(S), one.tolist()) and got.informative[11] > 0
    check(kc.pairs_ref(calls.tolist(), range(S), cls.tolist(), **kc.OFF), run(eng, calls, cls, **kc.OFF))     # and a valid call after them


def sim_counts(calls):
    """A count matrix whose calls are `calls`: 20 reads of the allele(s) of every called cell."""
    S, M = calls.shape
    counts = np.zeros((S, 2 * M), dtype=np.uint32)
    counts[:, 0::2] = np.select([calls == 0, calls == 1, calls == 2], [20, 10, 0], 0)
    counts[:, 1::2] = np.select([calls == 0, calls == 1, calls == 2], [0, 10, 20], 0)
    return counts


def same_result(a, b):
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.verdict, b.verdict) and np.array_equal(a.cls, b.cls)
    assert a.warnings == b.warnings and len(a.maps) == len(b.maps)
    for x, y in zip(a.maps, b.maps):
        assert x.edges.tobytes() == y.edges.tobytes() and np.array_equal(x.groups, y.groups)
        assert np.array_equal(x.degree, y.degree) and np.array_equal(x.informative, y.informative)
        assert x.order == y.order and x.positions == y.positions and x.phases == y.phases


def test_from_call_genotypes_to_the_map():
    """counts -> td_geno_call with the calls kept on the device -> linkage_map on the DeviceCalls equals the host route on
    the fetched calls and the loops, on the simulated cross (with missing cells, distorted and het x het markers)."""
    import genocall_cases as gc
    from tagdigger_amd import tagdigger_fun as tf
    sim = kc.simulated_cross("cp", offspring=200, ngroups=3, per_group=40, missing=0.03, distorted=4, hethet=4, seed=14)
    calls = sim["calls"]
    S, M = calls.shape
    samples = kc.sample_names(S)
    geno = tf.call_genotypes(sim_counts(calls), samples, gc.tag_names(M, list(range(0, 2 * M, 2)), list(range(1, 2 * M, 2)), 2 * M),
                             backend="gpu", keep_device=True)
    try:
        assert isinstance(geno.d_calls, tf.DeviceCalls) and geno.d_calls.shape == (S, M) and geno.calls.tolist() == calls.tolist()
        got = tf.linkage_map(geno.d_calls, samples, geno.markers, "cp", parents=[0, 1])
    finally:
        tf.default_engine(0).dev_free(geno.d_calls.ptr)
    host = tf.linkage_map(geno.calls, samples, geno.markers, "cp", parents=[0, 1], backend="host")
    same_result(got, host)
    same_result(tf.linkage_map(geno.calls, samples, geno.markers, "cp", parents=[0, 1]), host)       # a host matrix on the gpu backend
    kc.check_result(kc.map_ref(calls, "cp", parents=(0, 1)), got)
    assert got.stats["backend"] == "gpu" and got.stats["ms"] > 0 and sum(len(lm.order) for lm in got.maps) == 3
    assert all(got.verdict[m] != 0 for m in sim["bad"])


def test_repeatability(eng):
    S, Mp = 129, 130
    calls, cls = kc.structured_calls(S, Mp), kc.mixed_cls(Mp, 0)
    runs = [run(eng, calls, cls, **kc.OFF) for _ in range(2)]
    assert runs[0].n == Mp * (Mp - 1) // 2 and runs[0].edges.tobytes() == runs[1].edges.tobytes()
    assert runs[0].degree.tobytes() == runs[1].degree.tobytes() and runs[0].informative.tobytes() == runs[1].informative.tobytes()
    assert runs[0].ms > 0 and runs[0].times["pairs_ms"] > 0 and runs[0].times["gather_ms"] > 0
