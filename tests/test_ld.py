"""marker_ld(backend="host"), the groups, the pruning, the writers and the tag_ld / tag_calls command lines without a GPU,
against the LD rule stated by a plain loop in tests/ld_cases.py."""
import random

import numpy as np
import pytest

import genocall_cases as gc
import ld_cases as lc

SHAPES = [(33, 70), (65, 130), (129, 67)]


@pytest.mark.parametrize("S,M", SHAPES)
def test_cases_are_not_trivial(S, M):
    """The generator leaves edges at every threshold, and not all pairs except at (0, 0) -- where a pair drops out only
    for a marker that does not vary among the shared samples."""
    from tagdigger_amd import tagdigger_fun as tf
    pairs = M * (M - 1) // 2
    for min_shared, ppm in lc.THRESHOLDS:
        ref = lc.grid_ref(S, M, False, min_shared, ppm)
        assert len(ref["edges"]) > 0, (min_shared, ppm)
        got = tf.marker_ld(lc.structured_calls(S, M, wild=False), lc.marker_names(M), min_r2=ppm / 1e6, min_shared=min_shared,
                           backend="host")
        assert got.stats["edges"] == len(lc.grid_ref(S, M, False, min_shared, ppm, wild=False)["edges"]) > 0
        if ppm:
            assert len(ref["edges"]) < pairs // 2
    assert len(lc.grid_ref(S, M, False, 0, 0)["edges"]) > pairs * 9 // 10
    assert (lc.structured_calls(S, M) > 3).any()
    phases = {e[3] > 0 for e in lc.flipped_ref(S, M, False, 10, 800000)["edges"]}
    assert phases == {True, False}                         # with exchanged alleles both phases occur


@pytest.mark.parametrize("S,M", SHAPES + [(1, 5), (2, 3), (4, 1)])
def test_host_equals_the_loop(S, M):
    from tagdigger_amd import tagdigger_fun as tf
    calls = lc.structured_calls(S, M)
    for masked in (False, True):
        use = lc.random_mask(M) if masked else None
        for min_shared, ppm in lc.THRESHOLDS:
            edges, degree, called = tf._ld_host(calls, use, ppm, min_shared)
            lc.check_arrays(lc.grid_ref(S, M, masked, min_shared, ppm), edges, len(edges), degree, called)


def test_host_where_the_comparison_passes_64_bits():
    """sums_numpy is the reference where the loop does not reach; it equals the loop where it does.  At 4 096 samples
    both sides of the comparison pass 2^64, and _ld_host's two-word comparison stands on the knife edge: ppm0 lets the
    pair in, ppm0 + 1 does not."""
    from tagdigger_amd import tagdigger_fun as tf
    calls = lc.structured_calls(65, 130)
    for use in (None, lc.random_mask(130)):
        assert lc.sums_numpy(calls, use) == lc.pair_sums(calls.tolist(), None if use is None else use.tolist())
    S, M = 4096, 32
    calls = lc.structured_calls(S, M)
    sums = lc.sums_numpy(calls)
    called = (calls <= 2).sum(axis=0).tolist()
    wide = 0
    for pair in sorted(sums, key=lambda p: -lc.moments(sums[p])[1] ** 2)[1:5]:
        n, cov, var_i, var_j = lc.moments(sums[pair])
        ppm0 = 10 ** 6 * cov * cov // (var_i * var_j)
        assert 0 < ppm0 < 10 ** 6 and ppm0 * var_i * var_j != 10 ** 6 * cov * cov
        wide += cov * cov * 10 ** 6 > 1 << 64 and ppm0 * var_i * var_j > 1 << 64
        for ppm, inside in ((ppm0, True), (ppm0 + 1, False)):
            edges, degree, called_got = tf._ld_host(calls, None, ppm, 0)
            lc.check_arrays(lc.from_sums(sums, M, called, 0, ppm), edges, len(edges), degree, called_got)
            assert (pair in set(zip(edges["i"].tolist(), edges["j"].tolist()))) == inside
    assert wide >= 1


def test_host_blocks_of_markers(monkeypatch):
    """More markers than one block of _ld_host holds: the seams between blocks lose and double nothing."""
    from tagdigger_amd import tagdigger_fun as tf
    S, M = 65, 130
    monkeypatch.setattr(tf, "_LD_HOST_CELLS", 1000)        # blocks of 7 markers
    for min_shared, ppm in lc.THRESHOLDS:
        edges, degree, called = tf._ld_host(lc.structured_calls(S, M), None, ppm, min_shared)
        lc.check_arrays(lc.grid_ref(S, M, False, min_shared, ppm), edges, len(edges), degree, called)


def test_result_fields():
    from tagdigger_amd import tagdigger_fun as tf
    S, M = 65, 130
    calls, mask = lc.flipped_calls(S, M), lc.random_mask(M)
    got = tf.marker_ld(calls.tolist(), lc.marker_names(M), mask=mask.tolist(), min_r2=0.8, min_shared=10, backend="host")
    ref = lc.flipped_ref(S, M, True, 10, 800000)
    lc.check_arrays(ref, got.edges, len(got.edges), got.degree, got.called)
    assert got.markers == lc.marker_names(M) and got.mask.tolist() == (mask != 0).tolist()
    assert got.r2.dtype == np.float64 and got.r2.tolist() == [e[3] * e[3] / (e[4] * e[5]) for e in ref["edges"]]
    assert got.phase.tolist() == [1 if e[3] > 0 else -1 for e in ref["edges"]] and -1 in got.phase and 1 in got.phase
    assert (got.r2 >= 0.8).all() and (got.r2 <= 1.0).all()
    st = got.stats
    assert (st["backend"], st["markers"], st["used"], st["edges"], st["min_r2_ppm"], st["min_shared"]) == \
        ("host", M, int((mask != 0).sum()), len(ref["edges"]), 800000, 10)


class FakeResult:
    def __init__(self, M, mask, edges, called):
        self.markers = lc.marker_names(M)
        self.mask = np.array(mask, dtype=bool)
        self.edges = np.array([(i, j, 0, 0, 0, 0) for i, j in edges], dtype=lc.EDGE)
        self.called = np.array(called, dtype=np.uint32)
        self.degree = np.zeros(M, dtype=np.uint32)
        for i, j in edges:
            self.degree[i] += 1
            self.degree[j] += 1


def check_graph(M, mask, edges, called):
    from tagdigger_amd import tagdigger_fun as tf
    res = FakeResult(M, mask, edges, called)
    groups, keep = tf.ld_groups(res), tf.ld_prune(res)
    assert groups.tolist() == lc.groups_ref(M, mask, edges)
    assert keep.tolist() == lc.prune_ref(M, mask, edges, called)
    assert keep.dtype == bool and not keep[~res.mask].any() and not groups[~res.mask].any()
    kept = set(np.nonzero(keep)[0].tolist())
    assert not any(i in kept and j in kept for i, j in edges)                          # no two kept markers share an edge
    nbrs = {m: set() for m in range(M)}
    for i, j in edges:
        nbrs[i].add(j)
        nbrs[j].add(i)
    assert all(nbrs[m] & kept for m in range(M) if mask[m] and m not in kept)          # a dropped marker has a kept neighbour
    return groups.tolist(), keep.tolist()


def test_groups_and_pruning_by_hand():
    # a chain 0 - 1 - 2 - 3 - 4, equal called: the walk by index keeps 0, 2, 4
    g, k = check_graph(5, [1] * 5, [(0, 1), (1, 2), (2, 3), (3, 4)], [9] * 5)
    assert g == [1] * 5 and k == [True, False, True, False, True]
    # the same chain with the best-called marker in the middle of one end
    g, k = check_graph(5, [1] * 5, [(0, 1), (1, 2), (2, 3), (3, 4)], [9, 12, 9, 9, 9])
    assert k == [False, True, False, True, False]
    # a star around 3: by called the centre goes first and stands alone; with poorer calls the leaves stay
    star = [(0, 3), (1, 3), (2, 3), (3, 4), (3, 5)]
    g, k = check_graph(6, [1] * 6, star, [5, 5, 5, 8, 5, 5])
    assert g == [1] * 6 and k == [False, False, False, True, False, False]
    g, k = check_graph(6, [1] * 6, star, [5, 5, 5, 4, 5, 5])
    assert k == [True, True, True, False, True, True]
    # two components, a singleton, two markers that do not take part; groups by their smallest marker
    g, k = check_graph(9, [1, 1, 0, 1, 1, 1, 0, 1, 1], [(1, 7), (0, 4), (4, 8), (5, 7)], [3, 3, 0, 3, 3, 3, 0, 3, 3])
    assert g == [1, 2, 0, 3, 1, 2, 0, 2, 1]
    assert k == [True, True, False, True, False, True, False, False, True]
    # ties in called are broken by the index
    g, k = check_graph(4, [1] * 4, [(0, 1), (2, 3)], [7, 7, 6, 7])
    assert k == [True, False, False, True]
    # no edges, and nothing at all
    g, k = check_graph(3, [1, 0, 1], [], [1, 0, 1])
    assert g == [1, 0, 2] and k == [True, False, True]
    check_graph(0, [], [], [])


@pytest.mark.parametrize("seed", range(6))
def test_groups_and_pruning_on_random_graphs(seed):
    rng = random.Random(880 + seed)
    M = rng.choice((30, 200, 1000))
    mask = [rng.random() < 0.8 for _ in range(M)]
    part = [m for m in range(M) if mask[m]]
    edges = set()
    for _ in range(int(len(part) * rng.choice((0.3, 0.8, 2.5)))):
        i, j = rng.sample(part, 2)
        edges.add((min(i, j), max(i, j)))
    # long paths as well: the labels must travel the whole way
    path = rng.sample(part, len(part) // 3)
    edges.update((min(a, b), max(a, b)) for a, b in zip(path, path[1:]))
    called = [rng.randint(0, 5) if mask[m] else 0 for m in range(M)]
    check_graph(M, mask, sorted(edges), called)


def test_writers_byte_for_byte(tmp_path):
    from tagdigger_amd import tag_ld
    from tagdigger_amd import tagdigger_fun as tf
    S, M = 65, 130
    calls, mask = lc.flipped_calls(S, M), lc.random_mask(M)
    names = lc.marker_names(M)
    got = tf.marker_ld(calls, names, mask=mask, min_r2=0.5, min_shared=1, backend="host")
    ref = lc.flipped_ref(S, M, True, 1, 500000)
    pairs, groups, keep = (str(tmp_path / k) for k in ("pairs.csv", "groups.csv", "keep.txt"))
    tf.writeLDPairs(pairs, got)
    tf.writeLDGroups(groups, got)
    tag_ld.write_keep(keep, got)
    want = lc.pairs_csv(names, ref["edges"])
    assert b",+\r\n" in want and b",-\r\n" in want and b",1.000000," in want and b",0." in want
    with open(pairs, "rb") as fh:
        assert fh.read() == want
    want = lc.groups_csv(names, mask != 0, ref)
    assert b",1\r\n" in want and b",0\r\n" in want and want.count(b"\r\n") == 1 + int((mask != 0).sum())
    with open(groups, "rb") as fh:
        assert fh.read() == want
    with open(keep, "rb") as fh:
        assert fh.read() == lc.keep_txt(names, mask != 0, ref)
    assert tf.readMarkerNames(keep) == [n for n, k in zip(names, tf.ld_prune(got)) if k]      # what -k/--tokeep reads


def test_empty_inputs_on_the_host(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    for calls, names in ((np.zeros((0, 3), dtype=np.uint8), ["a", "b", "c"]), (np.zeros((4, 0), dtype=np.uint8), []), ([], []),
                         (np.full((4, 3), 3, dtype=np.uint8), ["a", "b", "c"])):
        got = tf.marker_ld(calls, names, min_r2=0.0, min_shared=0, backend="host")
        assert len(got.edges) == 0 and got.edges.dtype == np.dtype(lc.EDGE) and not got.degree.any() and not got.called.any()
        assert tf.ld_groups(got).tolist() == list(range(1, len(names) + 1)) and tf.ld_prune(got).tolist() == [True] * len(names)
        tf.writeLDPairs(str(tmp_path / "p.csv"), got)
        with open(str(tmp_path / "p.csv"), "rb") as fh:
            assert fh.read() == lc.pairs_csv(names, [])
    one = tf.marker_ld([[0, 1], [1, 3], [2, 3]], ["a", "b"], mask=[1, 0], min_r2=0.0, min_shared=0, backend="host")
    assert len(one.edges) == 0 and one.called.tolist() == [3, 0] and one.degree.tolist() == [0, 0]


def write_calls(path, calls, names, samples):
    from tagdigger_amd import tagdigger_fun as tf
    geno = tf.GenoResult(names, samples, np.array(calls), {}, np.ones(len(names), dtype=bool), None)
    tf.writeGenoCalls(path, geno, passing_only=True)


def test_tag_ld_command_line(tmp_path, capsys):
    from tagdigger_amd import tag_ld
    S, M = 65, 130
    calls, names = lc.structured_calls(S, M, wild=False), lc.marker_names(M)
    files = {k: str(tmp_path / k) for k in ("calls.csv", "pairs.csv", "groups.csv", "keep.txt")}
    write_calls(files["calls.csv"], calls, names, ["w%03d" % s for s in range(S)])
    assert tag_ld.main(["-i", files["calls.csv"], "-o", files["pairs.csv"], "--groups", files["groups.csv"], "--keep",
                        files["keep.txt"], "--min-shared", "10", "--td-backend", "host"]) == 0
    ref = lc.grid_ref(S, M, False, 10, 800000, wild=False)
    mask = [True] * M
    group, keep = lc.groups_ref(M, mask, ref["edges"]), lc.prune_ref(M, mask, ref["edges"], ref["called"])
    assert capsys.readouterr().out.strip().splitlines()[-1] == "Markers: %d Participating: %d Edges: %d Groups: %d Kept: %d" % (
        M, M, len(ref["edges"]), max(group), sum(keep))
    assert 1 < max(group) < M and 0 < sum(keep) < M
    for name, want in (("pairs.csv", lc.pairs_csv(names, ref["edges"])), ("groups.csv", lc.groups_csv(names, mask, ref)),
                       ("keep.txt", lc.keep_txt(names, mask, ref))):
        with open(files[name], "rb") as fh:
            assert fh.read() == want, name
    assert tag_ld.main(["-i", files["calls.csv"], "-o", files["pairs.csv"], "--min-r2", "1.0", "--min-shared", "5",
                        "--td-backend", "host"]) == 0
    ref = lc.grid_ref(S, M, False, 5, 1000000, wild=False)
    assert len(ref["edges"]) > 0
    with open(files["pairs.csv"], "rb") as fh:
        assert fh.read() == lc.pairs_csv(names, ref["edges"])


FILTERS = ["--err", "0.002", "--min-depth", "3", "--min-call-rate", "0.6", "--min-maf", "0.05", "--max-het", "0.75"]


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_tag_calls_ld_flags_on_the_host(tmp_path):
    """tag_calls --ld ... writes what tag_ld writes from tag_calls' own -o file; --relations-ld-pruned what tag_relate
    writes from the calls of the kept markers; and without the new flags every file is what it was."""
    from tagdigger_amd import tag_calls, tag_ld, tag_relate
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T = gc.grid_case(65, 260)
    samples = ["w%03d" % k for k in range(65)]
    f = {k: str(tmp_path / k) for k in ("counts.csv", "calls.csv", "stats.csv", "rel.csv", "calls2.csv", "stats2.csv", "rel2.csv",
                                        "ld.csv", "groups.csv", "keep.txt", "relp.csv", "ld3.csv", "groups3.csv", "keep3.txt",
                                        "calls4.csv", "rel4.csv")}
    tf.writeCounts(f["counts.csv"], counts, samples, gc.tag_names(260, i0, i1, T))
    ld = ["--min-r2", "0.05", "--ld-min-shared", "10"]
    rel = ["--max-dist", "0.3", "--min-shared", "20"]
    base = ["-i", f["counts.csv"], "--td-backend", "host"] + FILTERS + rel
    assert tag_calls.main(base + ["-o", f["calls.csv"], "--stats", f["stats.csv"], "--relations", f["rel.csv"]]) == 0
    assert tag_calls.main(base + ld + ["-o", f["calls2.csv"], "--stats", f["stats2.csv"], "--relations", f["rel2.csv"], "--ld", f["ld.csv"],
                                       "--ld-groups", f["groups.csv"], "--ld-keep", f["keep.txt"]]) == 0
    # without the new flags: what the rule says, as before; with them the old files do not change
    ref = gc.grid_ref(65, 260, 0, "likelihood", 1)
    direct = tf.call_genotypes(gc.as_array(counts, T), samples, gc.tag_names(260, i0, i1, T), backend="host", **gc.PARAMS[1])
    assert direct.calls.tolist() == ref["calls"]
    tf.writeGenoCalls(str(tmp_path / "direct.csv"), direct, passing_only=True)
    assert read(f["calls.csv"]) == read(str(tmp_path / "direct.csv"))
    for a, b in (("calls.csv", "calls2.csv"), ("stats.csv", "stats2.csv"), ("rel.csv", "rel2.csv")):
        assert read(f[a]) == read(f[b]), a
    # tag_ld on the written calls gives the same three files
    assert tag_ld.main(["-i", f["calls.csv"], "-o", f["ld3.csv"], "--groups", f["groups3.csv"], "--keep", f["keep3.txt"],
                        "--min-r2", "0.05", "--min-shared", "10", "--td-backend", "host"]) == 0
    for a, b in (("ld.csv", "ld3.csv"), ("groups.csv", "groups3.csv"), ("keep.txt", "keep3.txt")):
        assert read(f[a]) == read(f[b]), a
    passing = [m for m in range(260) if ref["mask"][m]]
    calls = np.array(ref["calls"], dtype=np.uint8)[:, passing]
    names = [direct.markers[m] for m in passing]
    want = lc.ld_ref(calls.tolist(), None, 10, 50000)
    assert 0 < len(want["edges"]) < len(passing) * (len(passing) - 1) // 2
    assert read(f["ld.csv"]) == lc.pairs_csv(names, want["edges"])
    kept = tf.readMarkerNames(f["keep.txt"])
    assert 0 < len(kept) < len(passing) and read(f["keep.txt"]) == lc.keep_txt(names, [True] * len(names), want)
    # the relations over the pruned markers: tag_calls -k keep.txt gives exactly those markers
    assert tag_calls.main(base + ld + ["-o", f["calls2.csv"], "--relations", f["relp.csv"], "--relations-ld-pruned"]) == 0
    assert read(f["calls2.csv"]) == read(f["calls.csv"])
    write_calls(f["calls4.csv"], calls[:, [names.index(k) for k in kept]], kept, samples)
    assert tag_relate.main(["-i", f["calls4.csv"], "-o", f["rel4.csv"], "--td-backend", "host"] + rel) == 0
    assert read(f["relp.csv"]) == read(f["rel4.csv"]) and read(f["relp.csv"]) != read(f["rel.csv"])
    with pytest.raises(Exception, match="--relations-ld-pruned goes with"):
        tag_calls.main(base + ["-o", f["calls2.csv"], "--relations-ld-pruned"])


def test_value_errors():
    from tagdigger_amd import tagdigger_fun as tf
    calls = np.array(lc.structured_calls(8, 20, wild=False))
    names = lc.marker_names(20)
    bad = calls.copy()
    bad[2, 5] = 4
    for args, kw in (((bad, names), {}),                                   # a code above 3 in a host array
                     ((calls.astype(np.int64) - 1, names), {}),            # a negative code
                     ((calls.astype(np.float64), names), {}),              # not integers
                     ((calls[0], names[:1]), {}),                          # not a matrix
                     ((calls, names[:19]), {}),                            # a name too few
                     ((calls, names), dict(mask=[1] * 19)),                # a mask entry too few
                     ((calls, names), dict(min_r2=-0.000001)),
                     ((calls, names), dict(min_r2=1.000001)),
                     ((calls, names), dict(min_shared=-1)),
                     ((calls, names), dict(min_shared=2.5)),
                     ((calls, names), dict(min_shared=True)),
                     ((calls, names), dict(backend="cpu")),
                     ((np.zeros((lc.MAX_SAMPLES + 1, 1), dtype=np.uint8), names[:1]), {}),
                     ((np.zeros((1, lc.MAX_MARKERS + 1), dtype=np.uint8), [""] * (lc.MAX_MARKERS + 1)), {}),
                     ((tf.DeviceCalls(0, (8, 20)), names), dict(backend="host"))):
        with pytest.raises(ValueError):
            tf.marker_ld(*args, **dict(dict(backend="host"), **kw))
    got = tf.marker_ld(calls, names, min_r2=0.0, min_shared=0, backend="host")         # the ends of the ranges are taken
    assert len(got.edges) == len(lc.ld_ref(calls.tolist())["edges"]) > 150
    assert len(tf.marker_ld(calls, names, min_r2=1.0, min_shared=8, backend="host").edges) == \
        len(lc.ld_ref(calls.tolist(), None, 8, 1000000)["edges"])
    assert tf.LD_MAX_SAMPLES == lc.MAX_SAMPLES and tf.LD_MAX_MARKERS == lc.MAX_MARKERS
