"""sample_relations(backend="host"), the writers and the tag_relate command line without a GPU, against the joint table
stated by brute force in tests/relate_cases.py."""
import numpy as np
import pytest

import relate_cases as rc


@pytest.mark.parametrize("S,M", [(1, 1), (3, 65), (17, 129)])
def test_reference_equals_brute_force(S, M):
    """The numpy reference every other test leans on, against plain ints: with bytes above 3, without and with a mask."""
    calls = rc.random_calls(S, M)
    assert M < 16 or (calls > 3).any()
    for use in (None, rc.random_mask(M)):
        assert rc.joint_ref(calls, use).tolist() == rc.joint_brute(calls.tolist(), None if use is None else use.tolist())


@pytest.mark.parametrize("S,M", [(1, 1), (3, 65), (17, 129), (65, 260)])
def test_host_backend_equals_reference(S, M):
    from tagdigger_amd import tagdigger_fun as tf
    calls = rc.random_calls(S, M, wild=False)
    for masked in (False, True):
        got = tf.sample_relations(calls, rc.sample_names(S), mask=rc.random_mask(M) if masked else None, backend="host")
        assert got.joint.dtype == np.uint32 and np.array_equal(got.joint, rc.grid_ref(S, M, masked, wild=False))
        assert got.stats["backend"] == "host" and got.stats["markers"] == M
    assert np.array_equal(tf._relations_host(rc.random_calls(S, M), rc.random_mask(M)), rc.grid_ref(S, M, True))    # bytes above 3


def test_populated_case_on_the_host():
    from tagdigger_amd import tagdigger_fun as tf
    calls, samples, mask, exp = rc.populated_case()
    got = tf.sample_relations(calls.tolist(), samples, mask=mask, backend="host")       # (lists are taken too)
    rc.check_result(exp, got)
    assert got.samples == samples and np.isnan(got.distance[4, 5]) and np.isnan(got.kinship[0, 7])
    assert got.stats["max_dist_ppm"] == 20000 and got.stats["min_shared"] == 50 and got.stats["used"] == 360


def test_identities():
    J = rc.grid_ref(17, 129, True).astype(np.int64)
    calls, use = rc.random_calls(17, 129), rc.random_mask(129)
    assert np.array_equal(J.transpose(1, 0, 3, 2), J)                                   # joint[j][i][b][a] == joint[i][j][a][b]
    for i in range(17):
        assert J[i, i][~np.eye(3, dtype=bool)].sum() == 0                               # a sample never disagrees with itself
        assert np.trace(J[i, i]) == int(((calls[i] <= 2) & (use != 0)).sum())           # the trace is its called count
    assert J.sum() > 0


def boundary_calls(shared, dist):
    """Two samples with `shared` markers called in both, `dist` of them one allele copy apart, and 7 called in one only."""
    a = [0] * shared + [0] * 7
    b = [1] * dist + [0] * (shared - dist) + [3] * 7
    return [a, b]


@pytest.mark.parametrize("shared,dist,max_dist,min_shared,flagged", [
    (50, 2, 0.02, 50, True),            # both at equality: 2 * 10^6 == 20 000 * 2 * 50, and 50 >= 50
    (50, 3, 0.02, 50, False),           # one unit too far
    (50, 1, 0.02, 50, True),            # one unit inside
    (49, 1, 0.02, 50, False),           # one marker too few (1 * 10^6 <= 20 000 * 98 holds)
    (51, 2, 0.02, 50, True),
    (50, 2, 0.02, 51, False),
    (400, 1, 0.00125, 400, True),       # 1 * 10^6 == 1250 * 2 * 400
    (400, 1, 0.001249, 400, False),     # one part per million below
    (400, 0, 0.0, 0, True),             # identical calls pass a zero distance
    (400, 1, 0.0, 0, False),
])
def test_duplicate_rule_at_its_boundaries(shared, dist, max_dist, min_shared, flagged):
    from tagdigger_amd import tagdigger_fun as tf
    calls = boundary_calls(shared, dist)
    d = rc.derived(rc.joint_brute(calls)[0][1])
    assert d["shared"] == shared and d["dist"] == dist
    assert rc.is_duplicate(d, rc.ppm(max_dist), min_shared) == flagged
    got = tf.sample_relations(calls, ["a", "b"], max_dist=max_dist, min_shared=min_shared, backend="host")
    assert got.duplicates == ([(0, 1)] if flagged else [])


def test_writers_byte_for_byte(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    calls, samples, mask, exp = rc.populated_case()
    got = tf.sample_relations(calls, samples, mask=mask, backend="host")
    pairs, matrix = str(tmp_path / "pairs.csv"), str(tmp_path / "dist.csv")
    tf.writeRelations(pairs, got)
    tf.writeDistanceMatrix(matrix, got)
    want = rc.pairs_csv(samples, exp)
    assert b",NA," in want and b",1\r\n" in want and b",0\r\n" in want and b"-0." in want    # NA, both flags, a negative kinship
    with open(pairs, "rb") as fh:
        assert fh.read() == want
    with open(matrix, "rb") as fh:
        assert fh.read() == rc.matrix_csv(samples, exp)


def test_empty_inputs_on_the_host(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    got = tf.sample_relations(np.zeros((3, 0), dtype=np.uint8), ["a", "b", "c"], backend="host")
    assert got.joint.shape == (3, 3, 3, 3) and not got.joint.any() and got.duplicates == [] and np.isnan(got.distance).all()
    got = tf.sample_relations([], [], backend="host")
    assert got.joint.shape == (0, 0, 3, 3) and got.duplicates == []
    tf.writeRelations(str(tmp_path / "p.csv"), got)
    with open(str(tmp_path / "p.csv"), "rb") as fh:
        assert fh.read() == rc.pairs_csv([], dict(pairs={}, duplicates=[]))


def test_round_trip_through_the_command_line(tmp_path, capsys):
    """writeGenoCalls -> tag_relate -i --td-backend host: a blank cell is missing."""
    from tagdigger_amd import tag_relate
    from tagdigger_amd import tagdigger_fun as tf
    calls, samples, mask, _ = rc.populated_case()
    M = calls.shape[1]
    geno = tf.GenoResult(["Mk%05d" % m for m in range(M)], samples, np.array(calls), {}, np.array(mask), None)
    calls_csv, pairs, matrix = str(tmp_path / "calls.csv"), str(tmp_path / "pairs.csv"), str(tmp_path / "dist.csv")
    tf.writeGenoCalls(calls_csv, geno, passing_only=True)
    assert tag_relate.main(["-i", calls_csv, "-o", pairs, "--matrix", matrix, "--td-backend", "host"]) == 0
    exp = rc.expected(calls, mask)
    assert capsys.readouterr().out.strip().splitlines()[-1] == "Samples: 8 Markers: 360 Pairs: 28 Duplicates: %d" % len(exp["duplicates"])
    with open(pairs, "rb") as fh:
        assert fh.read() == rc.pairs_csv(samples, exp)
    with open(matrix, "rb") as fh:
        assert fh.read() == rc.matrix_csv(samples, exp)
    assert tag_relate.main(["-i", calls_csv, "-o", pairs, "--max-dist", "0.5", "--min-shared", "1", "--td-backend", "host"]) == 0
    exp = rc.expected(calls, mask, max_dist=0.5, min_shared=1)
    assert len(exp["duplicates"]) > 3
    with open(pairs, "rb") as fh:
        assert fh.read() == rc.pairs_csv(samples, exp)
    broken = str(tmp_path / "broken.csv")
    with open(calls_csv) as fh, open(broken, "w") as out:
        out.write(fh.read().replace(",2,", ",5,", 1))
    with pytest.raises(Exception, match="0, 1, 2 or blank"):
        tag_relate.main(["-i", broken, "-o", pairs, "--td-backend", "host"])


def test_value_errors():
    from tagdigger_amd import tagdigger_fun as tf
    calls = np.array(rc.populated_case()[0])
    names = rc.sample_names(8)
    bad = calls.copy()
    bad[2, 5] = 4
    for args, kw in (((bad, names), {}),                                   # a code above 3 in a host array
                     ((calls.astype(np.int64) - 1, names), {}),            # a negative code
                     ((calls.astype(np.float64), names), {}),              # not integers
                     ((calls[0], names[:1]), {}),                          # not a matrix
                     ((calls, names[:7]), {}),                             # a name too few
                     ((calls, names), dict(mask=[1] * 399)),               # a mask entry too few
                     ((calls, names), dict(max_dist=-0.000001)),
                     ((calls, names), dict(max_dist=1.000001)),
                     ((calls, names), dict(min_shared=-1)),
                     ((calls, names), dict(min_shared=2.5)),
                     ((calls, names), dict(backend="cpu")),
                     ((tf.DeviceCalls(0, (8, 400)), names), dict(backend="host"))):
        with pytest.raises(ValueError):
            tf.sample_relations(*args, **dict(dict(backend="host"), **kw))
    got = tf.sample_relations(calls, names, max_dist=1.0, min_shared=0, backend="host")     # the ends of the ranges are taken
    assert len(got.duplicates) == 28                       # (0 * 10^6 <= 10^6 * 2 * 0 holds for a pair without a shared marker too)


def test_keep_device_is_off_by_default():
    """call_genotypes without keep_device, and on the host with it, carries no device buffer."""
    import genocall_cases as gc
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T = gc.grid_case(3, 64)
    for kw in ({}, dict(keep_device=True)):
        got = tf.call_genotypes(gc.as_array(counts, T), ["a", "b", "c"], gc.tag_names(64, i0, i1, T), backend="host", **kw)
        assert got.d_calls is None
        gc.check_result(gc.grid_ref(3, 64, 0, "likelihood", 0), got.calls, got.stats, got.mask, got.stats["passed"])
