"""The joint table of sample pairs on the device (csrc/relate.hip, int8 MFMA) against tests/relate_cases.py: every tile
and tail, the seam between marker chunks, the orientation of the result, the degenerate shapes and the chain from the
count matrix to the relations without the calls leaving the device."""
import numpy as np
import pytest

import genocall_cases as gc
import relate_cases as rc

pytestmark = pytest.mark.gpu

TD_E_ARG = -2


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def structure():
    from tagdigger_amd.engine import RELATE_KCHUNK, RELATE_TILE
    assert RELATE_TILE <= 128 and RELATE_KCHUNK <= 65536       # (the shapes below stay small)
    return RELATE_TILE, RELATE_KCHUNK


def test_constants_match_the_header():
    import os
    import re
    from conftest import ROOT
    from tagdigger_amd import engine
    hdr = open(os.path.join(ROOT, "include", "tagdig.h")).read()
    for name in ("MAX_SAMPLES", "TILE", "KCHUNK"):
        assert int(re.search(r"TD_RELATE_%s = (\d+)" % name, hdr).group(1)) == getattr(engine, "RELATE_" + name)
    assert engine.RELATE_MAX_SAMPLES == rc.MAX_SAMPLES


@pytest.mark.parametrize("M", [1, 15, 16, 17, 63, 64, 65, 127, 129, 257])
def test_tiles_and_tails(eng, M):
    """Every S around the tile edge (the last with a tile pair two off the diagonal) at every M around the 16-byte load,
    the 64-marker step and beyond; odd M with S > 1 puts the rows at odd addresses.  Codes from 0 .. 3 and 4 .. 255."""
    TILE, _ = structure()
    for S in (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 2):
        calls = rc.random_calls(S, M)
        for masked in (False, True):
            got = eng.relate_joint(calls, use=rc.random_mask(M) if masked else None)
            assert got.joint.dtype == np.uint32 and got.joint.shape == (S, S, 3, 3) and got.d_joint is None and got.ms > 0
            assert np.array_equal(got.joint, rc.grid_ref(S, M, masked)), (S, M, masked)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_chunk_seam(eng, which):
    TILE, KCHUNK = structure()
    M = (KCHUNK - 1, KCHUNK, KCHUNK + 1, 2 * KCHUNK + 3)[which]
    S = TILE + 1
    calls = rc.random_calls(S, M)
    around = np.zeros(M, dtype=np.uint8)
    around[max(0, KCHUNK - 2):KCHUNK + 2] = 1              # only the markers on either side of the seam
    blank = np.ones(M, dtype=np.uint8)
    blank[KCHUNK:2 * KCHUNK] = 0                           # the whole second chunk blanked
    assert np.array_equal(eng.relate_joint(calls).joint, rc.grid_ref(S, M, False))
    for use in (around, blank):
        ref = rc.joint_ref(calls, use)
        assert ref.sum() > 0
        assert np.array_equal(eng.relate_joint(calls, use=use).joint, ref)


def test_orientation(eng):
    """Constant rows, in one tile and TILE + 1 apart: a transposed result or a swapped plane order, which symmetric data
    would pass, puts M into the wrong cell."""
    TILE, _ = structure()
    M, S = 100, TILE + 6
    calls = np.array(rc.random_calls(S, M))
    const = {0: 0, 1: 2, 2: 1, 3: 255, TILE + 1: 2, TILE + 2: 0, TILE + 3: 1, TILE + 4: 3}
    for row, code in const.items():
        calls[row] = code
    J = eng.relate_joint(calls).joint.astype(np.int64)

    def only(i, j, a, b):
        want = np.zeros((3, 3), dtype=np.int64)
        want[a, b] = M
        assert np.array_equal(J[i, j], want), (i, j, J[i, j])
        assert np.array_equal(J[j, i], want.T), (j, i, J[j, i])

    only(0, 1, 0, 2)                                       # joint[0][1][0][2] == M, joint[0][1][2][0] == 0, joint[1][0][2][0] == M
    only(0, 2, 0, 1)
    only(2, 1, 1, 2)
    only(0, TILE + 1, 0, 2)                                # the same across two tiles, and from the other side
    only(TILE + 2, 1, 0, 2)
    only(2, TILE + 1, 1, 2)
    only(TILE + 3, 0, 1, 0)
    only(TILE + 3, TILE + 1, 1, 2)
    for row in (3, TILE + 4):
        assert not J[row].any() and not J[:, row].any()    # a missing row meets nothing
    assert np.array_equal(J, rc.joint_ref(calls))


def test_degenerate(eng):
    from tagdigger_amd import TagdigError
    TILE, _ = structure()
    S, M = TILE + 1, 129
    calls = rc.random_calls(S, M)
    assert not eng.relate_joint(calls, use=np.zeros(M, dtype=np.uint8)).joint.any()                 # all masked
    assert not eng.relate_joint(np.full((S, M), 3, dtype=np.uint8)).joint.any()                     # all missing
    assert not eng.relate_joint(np.full((S, M), 200, dtype=np.uint8), use=np.ones(M, dtype=np.uint8)).joint.any()
    got = eng.relate_joint(np.zeros((0, 5), dtype=np.uint8))
    assert got.joint.shape == (0, 0, 3, 3) and got.ms == 0
    got = eng.relate_joint(np.zeros((3, 0), dtype=np.uint8))
    assert got.joint.shape == (3, 3, 3, 3) and not got.joint.any() and got.ms == 0
    # neither shape lets a missing check reach memory
    for shape in ((rc.MAX_SAMPLES + 1, 0), (0, 1 << 31), (2, 3)):
        with pytest.raises(TagdigError) as ei:
            eng.relate_joint(None, shape=shape)
        assert ei.value.code == TD_E_ARG, shape
    assert np.array_equal(eng.relate_joint(calls).joint, rc.grid_ref(S, M, False))                  # and a valid call after them


def test_from_the_calls_the_call_kernel_left(eng):
    counts, i0, i1, T = gc.grid_case(65, 260)
    par = gc.PARAMS[1]
    res = eng.geno_call(gc.as_array(counts, T), i0, i1, list(gc.ref_table(gc.ppm(par["err"]))), err_ppm=gc.ppm(par["err"]),
                        min_depth=par["min_depth"], min_call_ppm=gc.ppm(par["min_call_rate"]),
                        min_maf_ppm=gc.ppm(par["min_maf"]), max_het_ppm=gc.ppm(par["max_het"]), keep_device=True)
    try:
        assert res.d_calls and 0 < res.mask.sum() < 260
        ref = rc.joint_ref(res.calls, res.mask)
        assert ref.sum() > 0
        got = eng.relate_joint(res.d_calls, shape=(65, 260), use=res.mask)
        assert np.array_equal(got.joint, ref)
        kept = eng.relate_joint(res.d_calls, shape=(65, 260), use=res.mask, fetch=False, keep_device=True)
        try:
            assert kept.joint is None and kept.d_joint
            assert eng.d2h(kept.d_joint, ref.nbytes) == ref.tobytes()
        finally:
            eng.dev_free(kept.d_joint)
    finally:
        eng.dev_free(res.d_calls)


def test_from_call_genotypes_to_sample_relations():
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T = gc.grid_case(65, 260)
    samples = rc.sample_names(65)
    geno = tf.call_genotypes(gc.as_array(counts, T), samples, gc.tag_names(260, i0, i1, T), backend="gpu", keep_device=True,
                             **gc.PARAMS[1])
    try:
        assert isinstance(geno.d_calls, tf.DeviceCalls) and geno.d_calls.shape == (65, 260) and geno.d_calls.ptr
        got = tf.sample_relations(geno.d_calls, samples, mask=geno.mask, max_dist=0.3, min_shared=20)
    finally:
        tf.default_engine(0).dev_free(geno.d_calls.ptr)
    rc.check_result(rc.expected(geno.calls, geno.mask, max_dist=0.3, min_shared=20), got)
    assert got.stats["backend"] == "gpu" and got.stats["ms"] > 0 and got.stats["used"] == int(geno.mask.sum())
    plain = tf.call_genotypes(gc.as_array(counts, T), samples, gc.tag_names(260, i0, i1, T), backend="gpu", **gc.PARAMS[1])
    assert plain.d_calls is None and np.array_equal(plain.calls, geno.calls)


def test_populated_case_through_python():
    from tagdigger_amd import tagdigger_fun as tf
    calls, samples, mask, exp = rc.populated_case()
    got = tf.sample_relations(calls, samples, mask=mask, backend="gpu")
    rc.check_result(exp, got)
    host = tf.sample_relations(calls, samples, mask=mask, backend="host")
    assert np.array_equal(host.joint, got.joint) and host.duplicates == got.duplicates


def test_cli_relations_from_tag_calls(tmp_path, capsys):
    """tag_calls -i ... --relations (the calls stay on the device, the filter mask selects the markers) writes the bytes
    tag_relate writes from tag_calls' own -o file."""
    from tagdigger_amd import tag_calls, tag_relate
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T = gc.grid_case(65, 260)
    samples = rc.sample_names(65)
    files = {k: str(tmp_path / k) for k in ("counts.csv", "calls.csv", "pairs1.csv", "dist1.csv", "pairs2.csv", "dist2.csv",
                                            "calls_host.csv", "pairs3.csv")}
    tf.writeCounts(files["counts.csv"], counts, samples, gc.tag_names(260, i0, i1, T))
    filters = ["--err", "0.002", "--min-depth", "3", "--min-call-rate", "0.6", "--min-maf", "0.05", "--max-het", "0.75"]
    relate = ["--max-dist", "0.3", "--min-shared", "20"]
    assert tag_calls.main(["-i", files["counts.csv"], "-o", files["calls.csv"], "--relations", files["pairs1.csv"],
                           "--relations-matrix", files["dist1.csv"]] + filters + relate) == 0
    assert tag_relate.main(["-i", files["calls.csv"], "-o", files["pairs2.csv"], "--matrix", files["dist2.csv"]] + relate) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert tag_calls.main(["-i", files["counts.csv"], "-o", files["calls_host.csv"], "--relations", files["pairs3.csv"],
                           "--td-backend", "host"] + filters + relate) == 0
    ref = gc.grid_ref(65, 260, 0, "likelihood", 1)
    exp = rc.expected(np.array(ref["calls"], dtype=np.uint8), ref["mask"], max_dist=0.3, min_shared=20)
    assert line == "Samples: 65 Markers: %d Pairs: 2080 Duplicates: %d" % (ref["passed"], len(exp["duplicates"]))
    want = rc.pairs_csv(samples, exp)
    for name in ("pairs1.csv", "pairs2.csv", "pairs3.csv"):
        with open(files[name], "rb") as fh:
            assert fh.read() == want, name
    for name in ("dist1.csv", "dist2.csv"):
        with open(files[name], "rb") as fh:
            assert fh.read() == rc.matrix_csv(samples, exp), name
