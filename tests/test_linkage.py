"""The linkage rule of DESIGN 4.24 without a GPU: the table, the numpy backend against the plain loops of
tests/link_cases.py on every shape the device tests use, the class selection, the segregation filter at its edges, the
groups, the greedy chain, a simulated cross whose order and phases must come back, the command line and the way in from
tag_dosage's diploidised calls."""
import decimal

import numpy as np
import pytest

import link_cases as kc

GRID_MP = (1, 2, 63, 64, 65, 130)
GRID_R = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)


def tf():
    from tagdigger_amd import tagdigger_fun
    return tagdigger_fun


# ---- the table
def test_table_powers_of_two_and_monotone():
    f = tf().linkage_tables(16384)
    assert len(f) == 16385 and f[0] == 0 and f[1] == 0 and all(isinstance(x, int) for x in f[:5])
    for e in range(15):
        assert f[1 << e] == 65536 * (1 << e) * e
    assert all(a < b for a, b in zip(f[1:], f[2:]))
    assert tf().linkage_tables(10) == f[:11]


def test_table_agrees_at_double_precision():
    f = tf().linkage_tables(16384)
    for k in range(16385):
        assert f[k] == kc.table_entry(k, prec=100), k
    assert list(kc.table(300)) == f[:301]


def test_min_lod16_from_the_decimal_text():
    t = tf()
    assert t.linkage_min_lod16(0) == 0 and t.linkage_min_lod16("3") == kc.min_lod16("3") == 653118
    assert t.linkage_min_lod16(3) == t.linkage_min_lod16(3.0) == 653118
    for text in ("0.1", "2.5", "10", "-1"):
        v = t.linkage_min_lod16(text)
        assert v == kc.min_lod16(text)
        with decimal.localcontext() as ctx:
            ctx.prec = 80
            unit = 65536 * decimal.Decimal(10).ln() / decimal.Decimal(2).ln()
            assert v - 1 < decimal.Decimal(text) * unit <= v


def test_lod_can_be_slightly_negative():
    f = kc.table(64)
    lods = {(n, rec): 65536 * n + f[rec] + f[n - rec] - f[n] for n in range(1, 65) for rec in range(n // 2 + 1)}
    assert min(lods.values()) in (-1, -2) and lods[10, 0] == 655360


# ---- the host backend against the loops
@pytest.mark.parametrize("Mp", GRID_MP)
def test_host_pairs_on_the_grid(Mp):
    t = tf()
    edges = 0
    for R in GRID_R:
        for holes in (0, 1):
            calls, cls = kc.structured_calls(R, kc.grid_markers(Mp, holes)), kc.mixed_cls(Mp, holes)
            for th in (kc.OFF, kc.REAL):
                got = t._link_pairs_host(calls, np.arange(R), cls, np.array(kc.table(R), dtype=np.int64), **th)
                kc.check_arrays(kc.grid_ref(R, Mp, holes, th), got[0], len(got[0]), got[1], got[2])
                edges += th is kc.REAL and len(got[0])
    assert edges > 0 or Mp <= 2


@pytest.mark.parametrize("kind", ["permuted", "inner"])
def test_host_pairs_on_a_row_subset(kind):
    t = tf()
    S, Mp = 65, 65
    rows = kc.row_subset(S, kind)
    calls, cls = kc.structured_calls(S, Mp), kc.mixed_cls(Mp, 0)
    for th in (kc.OFF, kc.REAL):
        got = t._link_pairs_host(calls, np.array(rows), cls, np.array(kc.table(len(rows)), dtype=np.int64), **th)
        kc.check_arrays(kc.grid_ref(S, Mp, 0, th, kind), got[0], len(got[0]), got[1], got[2])


def test_the_numpy_sums_of_the_cases_equal_the_loop():
    calls, cls = kc.structured_calls(33, kc.grid_markers(20, 1)), kc.mixed_cls(20, 1).tolist()
    rows = list(kc.row_subset(33, "permuted"))
    assert kc.sums_numpy(calls, rows, cls) == kc.pair_sums(calls.tolist(), rows, cls)


@pytest.mark.parametrize("M", [1, 2, 15, 16, 17, 63, 64, 65, 129])
def test_host_counts(M):
    t = tf()
    for R in (1, 2, 63, 64, 65):
        calls = kc.structured_calls(R, M)
        for kind in ("all", "permuted", "inner"):
            rows = kc.row_subset(R, kind)
            rows = list(range(R)) if rows is None else list(rows)
            assert t._link_counts_host(calls, np.array(rows)).tolist() == kc.counts_ref(calls.tolist(), rows)


# ---- class selection
def test_bc_classes_and_the_tie():
    counts = [[5, 9, 5, 0], [6, 9, 5, 1], [5, 9, 6, 1], [0, 0, 0, 20], [0, 3, 7, 0]]
    map_of, cls = tf().linkage_classes("bc", np.array(counts))
    assert map_of.tolist() == [1] * 5 and cls.tolist() == [0, 0, 1, 0, 1]
    assert (map_of.tolist(), cls.tolist()) == kc.classes_ref("bc", counts)
    map_of, cls = tf().linkage_classes("dh", np.array(counts))
    assert map_of.tolist() == [1] * 5 and cls.tolist() == [2] * 5 and (map_of.tolist(), cls.tolist()) == kc.classes_ref("dh", counts)


def test_cp_classes_for_every_pair_of_parent_calls():
    codes = [0, 1, 2, 3, 4, 7, 128, 254, 255]
    p1 = [a for a in codes for b in codes]
    p2 = [b for a in codes for b in codes]
    map_of, cls = tf().linkage_classes("cp", np.zeros((81, 4), dtype=np.uint32), (np.array(p1, dtype=np.uint8), np.array(p2, dtype=np.uint8)))
    assert (map_of.tolist(), cls.tolist()) == kc.classes_ref("cp", [[0] * 4] * 81, p1, p2)
    want = {(1, 0): (1, 0), (1, 2): (1, 1), (0, 1): (2, 0), (2, 1): (2, 1)}
    for a, b, k, c in zip(p1, p2, map_of.tolist(), cls.tolist()):
        assert (k, c) == want.get((a, b), (0, kc.NO_PART)), (a, b)


# ---- the segregation filter at equality and one off
def test_segregation_filter_edges():
    t = tf()
    # cls 0: a = c0, b = c1, o = c2.  min_shared 50; chi2 (a - b)^2 1000 <= 4000 (a + b); other o 10^6 <= 50000 (a + b + o)
    cases = [([25, 25, 0, 0], 0), ([25, 24, 0, 1], 3),                 # a + b = 50 and 49
             ([60, 40, 0, 0], 0), ([61, 40, 0, 0], 4), ([40, 60, 0, 0], 0), ([40, 61, 0, 0], 4),      # 400 * 1000 == 4000 * 100; 441000 > 404000
             ([50, 45, 5, 0], 0), ([50, 44, 5, 1], 5),                 # 5 * 10^6 == 50000 * 100; 5 * 10^6 > 50000 * 99
             ([10, 10, 30, 0], 3), ([70, 30, 50, 0], 4)]               # the first failing test names the reason
    counts = np.array([c for c, _ in cases], dtype=np.uint32)
    cls = np.zeros(len(cases), dtype=np.uint8)
    a, b, o, verdict = t.linkage_segregation(counts, cls, 50, 4000, 50000)
    assert verdict.tolist() == [v for _, v in cases]
    assert list(zip(a.tolist(), b.tolist(), o.tolist(), verdict.tolist())) == kc.segregation_ref(counts.tolist(), cls.tolist(), 50, 4000, 50000)
    # the other two class pairs read their own columns, and a marker without one is named so
    counts = np.array([[3, 30, 31, 0], [30, 2, 31, 0], [9, 9, 9, 9]], dtype=np.uint32)
    cls = np.array([1, 2, kc.NO_PART], dtype=np.uint8)
    a, b, o, verdict = t.linkage_segregation(counts, cls, 50, 6635, 50000)
    assert (a.tolist(), b.tolist(), o.tolist(), verdict.tolist()) == ([31, 30, 0], [30, 31, 0], [3, 2, 0], [0, 0, 1])
    assert list(zip(a.tolist(), b.tolist(), o.tolist(), verdict.tolist())) == kc.segregation_ref(counts.tolist(), cls.tolist(), 50, 6635, 50000)


# ---- groups
def edge_array(pairs):
    e = np.zeros(len(pairs), dtype=kc.EDGE)
    for k, p in enumerate(pairs):
        e[k] = tuple(p) + (0,) * (5 - len(p))
    return e


def test_groups_and_min_group_at_its_edge():
    t = tf()
    M = 12
    part = np.array([m != 5 for m in range(M)])
    pairs = [(7, 9), (0, 3), (3, 8), (1, 2), (2, 4), (4, 10), (1, 10)]         # {0, 3, 8}, {1, 2, 4, 10}, {7, 9}, singletons 6, 11
    for min_group, want in ((1, [1, 2, 2, 1, 2, 0, 3, 4, 1, 4, 2, 5]), (2, [1, 2, 2, 1, 2, 0, 0, 3, 1, 3, 2, 0]),
                            (3, [1, 2, 2, 1, 2, 0, 0, 0, 1, 0, 2, 0]), (4, [0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0]), (5, [0] * M)):
        got = t.linkage_groups(M, part, edge_array(pairs), min_group).tolist()
        assert got == want == kc.groups_ref(M, part.tolist(), pairs, min_group), min_group


# ---- the chain
def order_both(members, pairs, min_shared):
    edges = edge_array([(i, j, n, rec | ph << 31) for (i, j), (n, rec, ph) in sorted(pairs.items())])
    got = tf().linkage_order(np.array(sorted(members)), edges, min_shared)
    assert got == kc.order_ref(members, pairs, min_shared)
    return got


def test_order_ties_resolve_by_index():
    # four markers, every pair at rf 0.1: the chain starts with (2, 5), takes 7 and then 9 at the left end (the smaller
    # flag) -- 9 7 2 5 -- and is turned round, since 5 < 9
    pairs = {(i, j): (100, 10, 0) for i in (2, 5, 7, 9) for j in (2, 5, 7, 9) if i < j}
    order, positions, phases = order_both([2, 5, 7, 9], pairs, 10)
    assert order == [5, 2, 7, 9] and phases == [0, 0, 0, 0]
    # the same with one closer pair in the middle of the numbering: it starts the chain
    pairs[5, 7] = (100, 3, 1)
    order, positions, phases = order_both([2, 5, 7, 9], pairs, 10)
    assert order[0] < order[-1] and abs(order.index(5) - order.index(7)) == 1
    assert phases[order.index(5)] != phases[order.index(7)]
    # a pair below min_shared counts as unlinked (500000), a pair that is absent too
    pairs = {(0, 1): (100, 5, 0), (1, 2): (9, 0, 0), (0, 2): (100, 30, 1)}
    order, positions, phases = order_both([0, 1, 2], pairs, 10)
    assert order == [1, 0, 2] and phases == [0, 0, 1]
    order, positions, phases = order_both([0, 1, 2], {(0, 1): (100, 5, 0)}, 10)
    assert order == [1, 0, 2] and positions[2] - positions[1] == pytest.approx(25.0 * np.log(1.998 / 0.002), rel=1e-9)


def test_order_orientation_and_positions():
    # the chain 8 - 3 - 6 - 1 is built from the middle; the end holding the smaller marker is written first
    pairs = {(3, 6): (200, 2, 0), (3, 8): (200, 10, 1), (1, 6): (200, 20, 1), (1, 3): (200, 40, 0), (6, 8): (200, 30, 0), (1, 8): (200, 60, 1)}
    order, positions, phases = order_both([1, 3, 6, 8], pairs, 50)
    assert order == [1, 6, 3, 8] and phases == [0, 1, 1, 0]
    want = [0.0]
    for r in (0.1, 0.01, 0.05):
        want.append(want[-1] + 25.0 * np.log((1 + 2 * r) / (1 - 2 * r)))
    assert np.allclose(positions, want, rtol=1e-12, atol=0)
    assert order_both([4], {}, 1) == ([4], [0.0], [0])
    order, positions, _ = order_both([4, 9], {(4, 9): (10, 5, 0)}, 1)          # r = 1 / 2 is capped at 0.499
    assert order == [4, 9] and positions[1] == pytest.approx(25.0 * np.log(1.998 / 0.002), rel=1e-9)


def test_a_group_above_max_order_is_written_unordered(tmp_path):
    t = tf()
    sim = kc.simulated_cross("dh", offspring=120, ngroups=2, per_group=12, seed=5)
    kw = dict(min_shared=50, min_group=3)
    got = t.linkage_map(sim["calls"], kc.sample_names(120), kc.marker_names(24), "dh", max_order=11, backend="host", **kw)
    ref = kc.map_ref(sim["calls"], "dh", max_order=11, **kw)
    kc.check_result(ref, got)
    assert len(got.warnings) == 2 and "more than --max-order 11" in got.warnings[0] and got.maps[0].positions[1] is None
    assert got.maps[0].order[1] == sorted(got.maps[0].order[1])
    t.writeLinkageMap(str(tmp_path / "map.csv"), got)
    assert open(str(tmp_path / "map.csv"), "rb").read() == kc.map_csv(kc.marker_names(24), ref)
    got = t.linkage_map(sim["calls"], kc.sample_names(120), kc.marker_names(24), "dh", max_order=12, backend="host", **kw)
    kc.check_result(kc.map_ref(sim["calls"], "dh", max_order=12, **kw), got)
    assert not got.warnings and got.maps[0].positions[1] is not None


# ---- a simulated cross comes back
SIM = dict(cross="cp", offspring=200, ngroups=3, per_group=40, seed=14)      # a seed at which no marker is distorted by chance and the greedy chain of the loops recovers every order (checked below)


def check_truth(sim, maps):
    """maps: [(number, groups, order, phases)].  Every true group is one group of its map, in the true order or its
    reverse, with the founder phases up to a flip of the whole group."""
    for number, cols, founder in sim["truth"]:
        groups, order, phases = next((g, o, p) for k, g, o, p in maps if k == number)
        g = groups[cols[0]]
        assert g > 0 and all(groups[m] == g for m in cols) and sum(1 for x in groups if x == g) == len(cols)
        assert order[g] in (cols, cols[::-1])
        by = dict(zip(order[g], phases[g]))
        assert len({by[m] ^ ph for m, ph in zip(cols, founder)}) == 1


def test_simulated_cross_order_and_phases():
    sim = kc.simulated_cross(**SIM)
    ref = kc.map_ref(sim["calls"], "cp", parents=sim["parents"])
    check_truth(sim, [(mp["number"], mp["groups"], mp["order"], mp["phases"]) for mp in ref["maps"]])      # the restatement itself recovers it
    got = tf().linkage_map(sim["calls"], kc.sample_names(202), kc.marker_names(120), "cp", parents=["pl0000", "pl0001"], backend="host")
    kc.check_result(ref, got)
    check_truth(sim, [(lm.number, lm.groups.tolist(), lm.order, lm.phases) for lm in got.maps])
    assert {lm.number: len(lm.order) for lm in got.maps} == {1: 2, 2: 1}


@pytest.mark.parametrize("cross", ["cp", "bc", "dh"])
def test_host_map_with_missing_distorted_and_hethet_markers(cross):
    sim = kc.simulated_cross(cross, offspring=90, ngroups=2, per_group=10, step=0.05, missing=0.06, distorted=3, hethet=3, seed=11)
    S, M = sim["calls"].shape
    mask = np.ones(M, dtype=bool)
    mask[sim["truth"][0][1][4]] = False
    offspring = list(range(S - 1, (1 if cross == "cp" else -1) + 3, -1))       # not every row, and not in order
    kw = dict(min_shared=40, min_group=2)
    got = tf().linkage_map(sim["calls"], kc.sample_names(S), kc.marker_names(M), cross, parents=sim["parents"], offspring=offspring,
                           mask=mask, backend="host", **kw)
    ref = kc.map_ref(sim["calls"], cross, parents=sim["parents"], offspring=offspring, mask=mask.tolist(), **kw)
    kc.check_result(ref, got)
    reasons = {kc.REASONS[v] for v in got.verdict.tolist()}
    assert {"", "masked", "distorted"} <= reasons and (cross == "dh" or "other" in reasons or "parents" in reasons)
    assert all(got.verdict[m] != 0 for m in sim["bad"]) and sum(len(lm.edges) for lm in got.maps) > 10


# ---- the command line
def test_cli_round_trip(tmp_path, capsys):
    from tagdigger_amd import tag_linkage
    sim = kc.simulated_cross("cp", offspring=80, ngroups=3, per_group=8, step=0.05, missing=0.05, distorted=2, hethet=2, seed=7)
    S, M = sim["calls"].shape
    samples, markers = kc.sample_names(S), kc.marker_names(M)
    f = {k: str(tmp_path / k) for k in ("calls.csv", "map.csv", "pairs.csv", "stats.csv", "kids.txt")}
    open(f["calls.csv"], "wb").write(kc.calls_csv(samples, markers, sim["calls"]))
    kids = list(range(3, S))
    open(f["kids.txt"], "w").write("".join(samples[s] + "\n" for s in kids))
    assert tag_linkage.main(["-i", f["calls.csv"], "-o", f["map.csv"], "--cross", "cp", "--parents", "pl0000,pl0001", "--offspring",
                             f["kids.txt"], "--pairs", f["pairs.csv"], "--stats", f["stats.csv"], "--min-lod", "2.5", "--max-rf", "0.3",
                             "--min-shared", "30", "--max-chi2", "7.5", "--max-other", "0.04", "--min-group", "2", "--max-order", "100",
                             "--td-backend", "host"]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1].startswith("Markers: %d Offspring: %d Map1: " % (M, len(kids)))
    ref = kc.map_ref(sim["calls"], "cp", parents=(0, 1), offspring=kids, min_lod="2.5", max_rf_ppm=300000, min_shared=30,
                     max_chi2_milli=7500, max_other_ppm=40000, min_group=2, max_order=100)
    assert sum(len(mp["order"]) for mp in ref["maps"]) >= 3
    assert open(f["map.csv"], "rb").read() == kc.map_csv(markers, ref)
    assert open(f["pairs.csv"], "rb").read() == kc.pairs_csv(markers, ref)
    assert open(f["stats.csv"], "rb").read() == kc.stats_csv(markers, ref)


# ---- the way in from tag_dosage --diploid
def test_tetraploid_simplex_markers_through_call_dosage():
    """Simplex x nulliplex markers of a tetraploid (dosage 0 / 1, or 4 / 3) segregate 1 : 1 in the diploidised calls and
    map as a backcross; a duplex marker's 5 : 1 is thrown out by the segregation filter."""
    import genocall_cases as gc
    t = tf()
    sim = kc.simulated_cross("bc", offspring=100, ngroups=2, per_group=10, step=0.05, seed=13)
    calls = np.array(sim["calls"])
    S, M = calls.shape
    rng = np.random.default_rng(77)
    duplex = M                                      # one more marker: duplex x nulliplex, dosages 0 / 1 / 2 at 1 : 4 : 1
    dose = np.where(calls == 2, 4, np.where(calls == 1, np.where((calls == 2).any(axis=0)[None, :], 3, 1), 0))
    dose = np.concatenate([dose, rng.choice([0, 1, 1, 1, 1, 2], size=(S, 1))], axis=1)
    counts = np.zeros((S, 2 * (M + 1)), dtype=np.uint32)
    counts[:, 0::2], counts[:, 1::2] = 80 - 20 * dose, 20 * dose
    i0, i1 = list(range(0, 2 * (M + 1), 2)), list(range(1, 2 * (M + 1), 2))
    res = t.call_dosage(counts, kc.sample_names(S), gc.tag_names(M + 1, i0, i1, 2 * (M + 1)), ploidy=4, backend="host")
    assert res.calls[:, :M].tolist() == dose[:, :M].tolist() and res.diploid[:, :M].tolist() == calls.tolist()
    got = t.linkage_map(res.diploid, res.samples, res.markers, "bc", backend="host")
    ref = kc.map_ref(res.diploid, "bc")
    kc.check_result(ref, got)
    check_truth(sim, [(1, got.maps[0].groups.tolist(), got.maps[0].order, got.maps[0].phases)])
    assert kc.REASONS[got.verdict[duplex]] in ("distorted", "other") and got.maps[0].groups[duplex] == 0
