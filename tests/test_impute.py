"""The host side of LD-kNN imputation (tagdigger_fun: _impute_host, ld_neighbours, impute_calls, impute_check,
writeImputeStats; the tag_impute command line and tag_calls --impute with the host backend) against tests/impute_cases.py.
No GPU."""
import numpy as np
import pytest

import genocall_cases as gc
import impute_cases as ic
import ld_cases as lc
from tagdigger_amd import tagdigger_fun as tf


def host(calls, nbr, k, min_overlap, ppm):
    calls, nbr = np.asarray(calls, dtype=np.uint8), np.asarray(nbr, dtype=np.int32)
    got = tf._impute_host(calls, nbr, k, min_overlap, ppm)
    ic.check(ic.impute_ref(calls.tolist(), nbr.tolist(), k, min_overlap, ppm), *got)
    return got


@pytest.mark.parametrize("L", ic.GRID_L)
@pytest.mark.parametrize("S", ic.GRID_S)
def test_host_equals_the_loop_on_the_grid(S, L, monkeypatch):
    calls, nbr = ic.grid_calls(S, L), ic.grid_nbr(L)
    if S == 129:
        monkeypatch.setattr(tf, "_IMPUTE_HOST_CELLS", 3 * S * S)        # several blocks of markers, the last one short
    for k in ic.GRID_K:
        got = tf._impute_host(calls, nbr, k, ic.grid_overlap(L), ic.GRID_PPM)
        ic.check(ic.grid_ref(S, L, k), *got)
        left = got[0] > 2
        assert np.array_equal(got[0][left], calls[left])


def test_the_grid_counts_something_in_every_column():
    totals = np.zeros(4, dtype=np.int64)
    for S in ic.GRID_S:
        for L in ic.GRID_L:
            for k in ic.GRID_K:
                totals += np.array(ic.grid_ref(S, L, k)[1]).sum(axis=0)
    ic.assert_grid_populated(totals.tolist())


def test_planted_cells_on_the_host():
    assert host([[3, 1], [2, 1], [0, 1]], [[1], [-1]], 1, 1, 0)[0][0, 0] == 2          # equal weights: the smaller donor
    assert host([[77, 1], [0, 1], [2, 1]], [[1], [-1]], 2, 1, 0)[0][0, 0] == 77        # two classes tie
    assert host([[200, 0, 0], [1, 2, 2], [1, 2, 2]], [[1, 2], [-1, -1], [-1, -1]], 2, 1, 0)[1][0].tolist() == [1, 0, 0, 1]
    conf = [[3, 1], [0, 1], [0, 1], [1, 1], [0, 1]]
    assert host(conf, [[1], [-1]], 4, 1, 750000)[0][0, 0] == 0 and host(conf, [[1], [-1]], 4, 1, 750001)[0][0, 0] == 3
    nbr = [[1, 2, 3, 4]] + [[-1] * 4] * 4
    calls = [[3, 0, 1, 2, 9], [1, 0, 1, 2, 0]]
    assert host(calls, nbr, 1, 3, 0)[1][0].tolist() == [1, 1, 0, 0] and host(calls, nbr, 1, 4, 0)[1][0].tolist() == [1, 0, 1, 0]
    got = host([[3, 1, 0, 0], [2, 3, 0, 0]], [[2, 3], [0, 2], [-1, -1], [-1, -1]], 1, 2, 0)     # no chaining
    assert got[0].tolist() == [[2, 1, 0, 0], [2, 3, 0, 0]]
    calls, nbr = ic.division_case()
    for ppm in (0, 500000, 510000, 666666, 1000000):
        host(calls, nbr, 2, 1, ppm)
    for shape in ((0, 4), (3, 0), (0, 0)):
        got = tf._impute_host(np.zeros(shape, dtype=np.uint8), np.full((shape[1], 2), -1, dtype=np.int32), 3, 1, 0)
        assert got[0].shape == shape and got[1].shape == (shape[1], 4) and not got[1].any()


def test_ld_neighbours_equals_the_exact_order():
    S, M = 65, 40
    calls = np.where(lc.structured_calls(S, M) > 2, 3, lc.structured_calls(S, M)).astype(np.uint8)
    ld = tf.marker_ld(calls, lc.marker_names(M), min_r2=0.05, min_shared=10, backend="host")
    edges = ld.edges.tolist()
    assert len(edges) > M
    degree = np.bincount(np.concatenate([ld.edges["i"], ld.edges["j"]]), minlength=M)
    assert degree.max() > 3 and degree.min() < 20
    for l in (1, 3, 20, 64):
        table = tf.ld_neighbours(ld, l)
        assert table.dtype == np.int32 and table.shape == (M, l) and table.tolist() == ic.neighbours_ref(edges, M, l)
    # the last marker is the first one over again: whoever is joined to both has them at one r^2, the smaller index first
    full = tf.ld_neighbours(ld, 64)
    tied = [m for m in range(1, M - 1) if 0 in full[m] and M - 1 in full[m]]
    assert tied and all(list(full[m]).index(0) + 1 == list(full[m]).index(M - 1) for m in tied)
    assert (full[:, -1] == -1).all() and (full >= 0).sum() == 2 * len(edges)           # fewer than l edges: padded
    # a masked marker has no edges and an empty row; no marker at all gives an empty table
    mask = np.arange(M) % 3 != 0
    part = tf.marker_ld(calls, lc.marker_names(M), mask=mask, min_r2=0.05, min_shared=10, backend="host")
    table = tf.ld_neighbours(part, 5)
    assert table.tolist() == ic.neighbours_ref(part.edges.tolist(), M, 5) and (table[~mask] == -1).all() and mask[table[table >= 0]].all()
    none = tf.marker_ld(np.zeros((4, 0), dtype=np.uint8), [], backend="host")
    assert tf.ld_neighbours(none, 2).shape == (0, 2)
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError):
            tf.ld_neighbours(ld, bad)


def test_impute_calls_on_the_host_and_its_arguments():
    S, M = 65, 40
    calls = np.where(lc.structured_calls(S, M) > 2, 3, lc.structured_calls(S, M)).astype(np.uint8)
    names = lc.marker_names(M)
    mask = np.arange(M) % 5 != 0
    kw = dict(l=6, k=4, min_overlap=2, min_conf=0.55, min_r2=0.05, ld_min_shared=10, backend="host")
    got = tf.impute_calls(calls, names, mask=mask, **kw)
    ld = tf.marker_ld(calls, names, mask=mask, min_r2=0.05, min_shared=10, backend="host")
    assert np.array_equal(got.neighbours, tf.ld_neighbours(ld, 6))
    ic.check(ic.impute_ref(calls.tolist(), got.neighbours.tolist(), 4, 2, 550000), got.calls, got.stats)
    assert got.imputed == int(got.stats[:, 1].sum()) > 0 and got.ms == 0 and got.params["min_conf_ppm"] == 550000
    assert np.array_equal(got.calls[:, ~mask], calls[:, ~mask]) and not got.stats[~mask, 1].any()
    # an LD result made without the mask: the mask still keeps everybody else out
    wide = tf.marker_ld(calls, names, min_r2=0.05, min_shared=10, backend="host")
    cut = tf.impute_calls(calls, names, ld=wide, mask=mask, **kw)
    assert (cut.neighbours[~mask] == -1).all() and mask[cut.neighbours[cut.neighbours >= 0]].all()
    ic.check(ic.impute_ref(calls.tolist(), cut.neighbours.tolist(), 4, 2, 550000), cut.calls, cut.stats)
    as_lists = tf.impute_calls(calls.tolist(), names, mask=mask.tolist(), **kw)
    assert as_lists.calls.tobytes() == got.calls.tobytes()
    for bad in (dict(l=0), dict(l=65), dict(k=0), dict(k=33), dict(min_overlap=0), dict(min_conf=1.5), dict(backend="cpu")):
        with pytest.raises(ValueError):
            tf.impute_calls(calls, names, **dict(kw, **bad))
    with pytest.raises(ValueError):
        tf.impute_calls(np.zeros((ic.MAX_SAMPLES + 1, 2), dtype=np.uint8), ["a", "b"], **kw)
    with pytest.raises(ValueError):
        tf.impute_calls(np.full((2, 2), 4, dtype=np.uint8), ["a", "b"], **kw)
    with pytest.raises(ValueError):
        tf.impute_calls(tf.DeviceCalls(0, (2, 2)), ["a", "b"], **kw)
    empty = tf.impute_calls([], [], **kw)
    assert empty.calls.shape == (0, 0) and empty.imputed == 0


def test_impute_check_hides_the_seeded_cells_and_recounts():
    S, M = 65, 40
    calls = np.where(lc.structured_calls(S, M) > 2, 3, lc.structured_calls(S, M)).astype(np.uint8)
    names = lc.marker_names(M)
    kw = dict(l=6, k=4, min_overlap=2, min_conf=0.55, min_r2=0.05, ld_min_shared=10, backend="host")
    ncalled = int((calls <= 2).sum())
    hidden = tf.impute_hidden_cells(calls, 50000, 3)
    assert len(hidden) == ncalled * 50000 // 10 ** 6 > 50 and len(set(hidden.tolist())) == len(hidden)
    assert (calls.reshape(-1)[hidden] <= 2).all() and (np.diff(hidden) > 0).all()
    flat = np.flatnonzero(calls <= 2)
    assert np.array_equal(hidden, np.sort(np.random.default_rng(3).choice(flat, size=len(hidden), replace=False)))
    assert not np.array_equal(hidden, tf.impute_hidden_cells(calls, 50000, 4)) and len(tf.impute_hidden_cells(calls, 0, 3)) == 0
    table = tf.impute_check(calls, names, hide_ppm=50000, seed=3, **kw)
    # the recount: hide the same cells, take the neighbours from the holed matrix, impute with the loop
    holed = calls.copy()
    holed.reshape(-1)[hidden] = 3
    ld = tf.marker_ld(holed, names, min_r2=0.05, min_shared=10, backend="host")
    ref = np.array(ic.impute_ref(holed.tolist(), tf.ld_neighbours(ld, 6).tolist(), 4, 2, 550000)[0], dtype=np.uint8)
    want = np.zeros((3, 4), dtype=np.int64)
    for cell in hidden.tolist():
        want[calls.reshape(-1)[cell], min(int(ref.reshape(-1)[cell]), 3)] += 1
    assert table.dtype == np.int64 and table.tolist() == want.tolist() and table.sum() == len(hidden)
    assert table[:, :3].sum() > 0 and table[:, 3].sum() > 0
    mask = np.arange(M) % 2 == 0                   # under a mask only cells of the markers that take part are hidden
    part = tf.impute_hidden_cells(calls, 100000, 0, mask)
    assert len(part) == int((calls[:, mask] <= 2).sum()) // 10 and mask[part % M].all()
    assert tf.impute_check(calls, names, hide_ppm=100000, seed=0, mask=mask, **kw).sum() == len(part)


def test_forced_case_comes_back_as_the_truth():
    truth, hidden, nbr = ic.forced_case()
    S, M = truth.shape
    holed = truth.copy()
    holed.reshape(-1)[hidden] = 3
    cl, nl = holed.tolist(), nbr.tolist()
    for cell in hidden.tolist():                   # by construction: a donor at dist 0 over all the neighbours
        t, m = divmod(cell, M)
        ranked = ic.weights_ref(cl, nl, m, t)
        assert any((w, ovl, dist) == (65536, nbr.shape[1], 0) for w, d, ovl, dist in ranked)
        assert all(truth[d, m] == truth[t, m] for w, d, ovl, dist in ranked if w == 65536)      # whoever is first of them, it tells the truth
    got, stats = tf._impute_host(holed, nbr, 1, 1, 1000000)
    assert np.array_equal(got, truth) and stats[:, 1].sum() == len(hidden) == stats[:, 0].sum() and not stats[:, 2:].any()
    ic.check(ic.impute_ref(cl, nl, 1, 1, 1000000), got, stats)


def stats_csv(markers, stats, nbr):
    lines = ["marker,missing,imputed,no_donor,undecided,neighbours"]
    for m, name in enumerate(markers):
        lines.append(",".join([name] + [str(int(x)) for x in stats[m]] + [str(sum(1 for q in nbr[m] if q >= 0))]))
    return ("\r\n".join(lines) + "\r\n").encode("ascii")


def test_cli_round_trip_on_the_host(tmp_path, capsys):
    from tagdigger_amd import tag_impute
    from tagdigger_amd.tag_relate import read_calls
    S, M = 65, 40
    calls = np.where(lc.structured_calls(S, M) > 2, 3, lc.structured_calls(S, M)).astype(np.uint8)
    names, samples = lc.marker_names(M), ["s%02d" % s for s in range(S)]
    f = {k: str(tmp_path / k) for k in ("calls.csv", "imputed.csv", "stats.csv")}
    tag_impute.write_calls(f["calls.csv"], samples, names, calls)
    assert read_calls(f["calls.csv"])[2].tobytes() == calls.tobytes()
    opts = ["-l", "6", "-k", "4", "--min-overlap", "2", "--min-conf", "0.55", "--min-r2", "0.05", "--ld-min-shared", "10", "--td-backend", "host"]
    assert tag_impute.main(["-i", f["calls.csv"], "-o", f["imputed.csv"], "--stats", f["stats.csv"], "--check", "0.05", "--seed", "3"] + opts) == 0
    want = tf.impute_calls(calls, names, l=6, k=4, min_overlap=2, min_conf=0.55, min_r2=0.05, ld_min_shared=10, backend="host")
    ref = ic.impute_ref(calls.tolist(), want.neighbours.tolist(), 4, 2, 550000)
    back = read_calls(f["imputed.csv"])
    assert back[0] == samples and back[1] == names and np.minimum(back[2], 3).tolist() == np.minimum(np.array(ref[0]), 3).tolist()
    assert open(f["stats.csv"], "rb").read() == stats_csv(names, ref[1], want.neighbours.tolist())
    out = capsys.readouterr().out.strip().splitlines()
    total = np.array(ref[1]).sum(axis=0)
    assert out[0] == "Markers: {} Missing: {} Imputed: {} No donor: {} Undecided: {}".format(M, *total) and total[1] > 0
    table = tf.impute_check(calls, names, hide_ppm=50000, seed=3, l=6, k=4, min_overlap=2, min_conf=0.55, min_r2=0.05, ld_min_shared=10,
                            backend="host")
    assert out[1:] == ["truth,as_0,as_1,as_2,left_missing"] + ["{},{},{},{},{}".format(g, *table[g]) for g in range(3)]


def test_tag_calls_impute_on_the_host_and_unchanged_without_it(tmp_path, capsys):
    """tag_calls --impute writes what tag_impute writes from tag_calls' own -o file; without --impute tag_calls writes and
    prints what it did."""
    from tagdigger_amd import tag_calls, tag_impute
    counts, i0, i1, T = gc.grid_case(65, 260)
    samples = ["w%03d" % k for k in range(65)]
    tagnames = gc.tag_names(260, i0, i1, T)
    f = {k: str(tmp_path / k) for k in ("counts.csv", "plain.csv", "plain_stats.csv", "calls.csv", "imp1.csv", "st1.csv", "imp2.csv", "st2.csv",
                                        "direct.csv", "direct_stats.csv")}
    tf.writeCounts(f["counts.csv"], counts, samples, tagnames)
    filters = ["--err", "0.002", "--min-depth", "3", "--min-call-rate", "0.6", "--min-maf", "0.05", "--max-het", "0.75", "--td-backend", "host"]
    assert tag_calls.main(["-i", f["counts.csv"], "-o", f["plain.csv"], "--stats", f["plain_stats.csv"]] + filters) == 0
    plain_out = capsys.readouterr().out
    geno = tf.call_genotypes(gc.as_array(counts, T), samples, tagnames, backend="host", **gc.PARAMS[1])
    tf.writeGenoCalls(f["direct.csv"], geno)
    tf.writeMarkerStats(f["direct_stats.csv"], geno)
    assert open(f["plain.csv"], "rb").read() == open(f["direct.csv"], "rb").read()
    assert open(f["plain_stats.csv"], "rb").read() == open(f["direct_stats.csv"], "rb").read()
    assert plain_out == tag_calls.stats_line(geno) + "\n"
    tune = ["--min-overlap", "2", "--min-conf", "0.5", "--ld-min-shared", "10"]
    assert tag_calls.main(["-i", f["counts.csv"], "-o", f["calls.csv"], "--impute", f["imp1.csv"], "--impute-stats", f["st1.csv"],
                           "--impute-neighbours", "8", "--impute-voters", "5", "--impute-min-r2", "0.05"] + tune + filters) == 0
    out1 = capsys.readouterr().out.strip().splitlines()
    assert open(f["calls.csv"], "rb").read() == open(f["plain.csv"], "rb").read() and out1[0] + "\n" == plain_out
    assert tag_impute.main(["-i", f["calls.csv"], "-o", f["imp2.csv"], "--stats", f["st2.csv"], "-l", "8", "-k", "5", "--min-r2", "0.05",
                            "--td-backend", "host"] + tune) == 0
    out2 = capsys.readouterr().out.strip().splitlines()
    assert open(f["imp1.csv"], "rb").read() == open(f["imp2.csv"], "rb").read() != open(f["calls.csv"], "rb").read()
    passing = [r for r in open(f["st1.csv"], newline="").read().split("\r\n")[1:] if r and geno.mask[geno.markers.index(r.split(",")[0])]]
    assert passing == [r for r in open(f["st2.csv"], newline="").read().split("\r\n")[1:] if r]
    assert out1[1].split(" Missing: ")[0] == "Markers: 260" and out2[0].split(" Missing: ")[0] == "Markers: {}".format(int(geno.mask.sum()))
    assert int(out2[0].split("Imputed: ")[1].split()[0]) > 0
    with pytest.raises(Exception):
        tag_calls.main(["-i", f["counts.csv"], "-o", f["calls.csv"], "--impute-stats", f["st1.csv"]] + filters)
