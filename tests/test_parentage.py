"""The host side of parentage without a GPU: the reference of tests/parentage_cases.py against the bit-plane
expression, tagdigger_fun._parentage_host against it on the word, slot and ranking grids at reduced sizes, the choice of
the candidates and the status rule at their knife edges, the writers' bytes, the command line on the host backend, the
names, and the margins of the simulated pedigree."""
import numpy as np
import pytest

import parentage_cases as pc
from tagdigger_amd import tag_parentage
from tagdigger_amd import tagdigger_fun as tf


def host(calls, use, offspring, cand, selfing, K, min_shared):
    return tf._parentage_host(np.asarray(calls, dtype=np.uint8), use, offspring, np.asarray(cand, dtype=np.int32), selfing, K, min_shared)


def test_reference_equals_the_plane_expression():
    pc.check_plane_expression()


def test_reference_counts_by_hand():
    """o = 1 between parents 0 and 2 fits everywhere; o = 0 between parents 1 and 2 fits nowhere; a missing parent shares
    nothing."""
    calls, offspring, cand, M = pc.orientation_case()
    t = pc.table_ref(calls.tolist(), None, offspring, cand.tolist(), True)
    pairs = pc.slot_pairs(3, True)
    assert t[0][pairs.index((0, 1))] == (M, 0) and t[0][pairs.index((0, 0))] == (M, M) and t[0][pairs.index((1, 1))] == (M, M)
    assert t[1][pairs.index((0, 1))] == (M, M) and t[1][pairs.index((0, 0))] == (M, 0) and t[1][pairs.index((1, 1))] == (M, M)
    assert all(t[i][pairs.index((a, 2))] == (0, 0) for i in (0, 1) for a in (0, 1, 2))
    best, table = host(calls, None, offspring, cand, True, 2, 1)
    pc.check(t, cand.tolist(), True, 2, 1, best, table)


@pytest.mark.parametrize("M,kind", [c for c in pc.EDGE_CASES if c[0] in (1, 63, 64, 65, 129, 64 * pc.WCHUNK + 1)])
def test_host_word_edges(M, kind):
    calls, use, offspring, cand, ref = pc.edge_case(M, kind)
    best, table = host(calls, use, offspring, cand, True, 2, 1)
    pc.check(ref, cand.tolist(), True, 2, 1, best, table)


@pytest.mark.parametrize("selfing", (True, False))
@pytest.mark.parametrize("C", (1, 2, 3, 4, 5, pc.BLOCK + 1))
def test_host_slot_edges(C, selfing):
    calls, offspring, cand, ref = pc.slot_case(C, selfing)
    assert len(ref[0]) == (C * (C + 1) // 2 if selfing else C * (C - 1) // 2)
    best, table = host(calls, None, offspring, cand, selfing, 3, 1)
    pc.check(ref, cand.tolist(), selfing, 3, 1, best, table)


def test_host_ranking():
    calls, offspring, cand, diagonal = pc.rank_case()
    ref = pc.table_ref(calls.tolist(), None, offspring, cand.tolist(), True)
    assert [ref[0][t] for t in diagonal] == list(pc.RANK_TRIOS)
    assert sum(1 for n, _ in ref[0] if n > 0) == len(pc.RANK_TRIOS)            # trios of two candidates share nothing
    assert [t for _, _, t in pc.rank_ref(ref[0], pc.RANK_MIN_SHARED)] == [diagonal[a] for a in pc.RANK_ORDER]
    assert pc.rank_ref(ref[1], pc.RANK_MIN_SHARED) == []
    for K in range(1, pc.MAX_TOP + 1):
        best, table = host(calls, None, offspring, cand, True, K, pc.RANK_MIN_SHARED)
        want = pc.check(ref, cand.tolist(), True, K, pc.RANK_MIN_SHARED, best, table)
        assert want[0]["p"].tolist() == (list(pc.RANK_ORDER) + [pc.NONE] * pc.MAX_TOP)[:K]
        assert (want[1]["p"] == pc.NONE).all() and not want[1]["n"].any()


def test_candidates_at_their_knife_edges():
    """e2 10^6 == ppm n2 is in, one more error is out; n2 == min_shared is in, one less is out; the order is e2 / n2 by
    cross-multiplication, then n2 descending, then the index; the cut keeps the lower index of a tie."""
    n2 = np.array([100, 100, 50, 49, 200, 100, 100, 300], dtype=np.int64)
    e2 = np.array([3, 4, 0, 0, 6, 3, 0, 9], dtype=np.int64)
    allowed = np.ones(8, dtype=bool)
    allowed[6] = False
    got = tf._parent_candidates(n2, e2, allowed, 50, 30000, 32)
    assert got.tolist() == [2, 7, 4, 0, 5]         # 0 errors; then 3 %: n2 = 300, 200, 100 (index 0 before 5)
    pairs = [[(int(n), int(e)) for n, e in zip(n2, e2)]]
    assert pc.candidates_ref(pairs, 0, [1, 2, 3, 4, 5, 7], 50, 30000, 32) == [2, 7, 4, 5]      # (o = 0 itself is left out there)
    assert tf._parent_candidates(n2, e2, allowed, 50, 30000, 4).tolist() == [2, 7, 4, 0]       # the tie at the cut
    assert tf._parent_candidates(n2, e2, allowed, 51, 30000, 32).tolist() == [7, 4, 0, 5]
    assert tf._parent_candidates(n2, e2, allowed, 50, 29999, 32).tolist() == [2]


def test_candidate_order_is_exact_where_floats_tie():
    """1 / 3 against 715827883 / 2147483647: equal as float64 quotients' neighbours, different as fractions."""
    n2 = np.array([2147483647, 3, 2147483646], dtype=np.int64)
    e2 = np.array([715827883, 1, 715827882], dtype=np.int64)
    got = tf._parent_candidates(n2, e2, np.ones(3, dtype=bool), 1, 1000000, 32).tolist()
    pairs = [[(int(n), int(e)) for n, e in zip(n2, e2)]]
    assert got == pc.candidates_ref(pairs, -1, [0, 1, 2], 1, 1000000, 32) == [2, 1, 0]


def test_status_rule():
    assert pc.decide([(100, 3, 0)], 30000, 1) == "trio" and pc.decide([(100, 4, 0)], 30000, 1) == "single"
    assert pc.decide([(100, 0, 0), (100, 3, 1)], 30000, 2) == "ambiguous" and pc.decide([(100, 0, 0), (100, 4, 1)], 30000, 2) == "trio"
    assert pc.decide([], 30000, 0) == "none" and pc.decide([], 30000, 2) == "single"
    # the product at the same edges: one candidate that is a perfect selfing parent at exactly 3 % and just above
    M = 100
    for errors, status in ((3, "trio"), (4, "single")):
        parent = np.ones(M, dtype=np.uint8)
        child = np.ones(M, dtype=np.uint8)
        parent[:errors] = 0                        # (0, 0) -> {0}: a heterozygous child is an error there
        res = tf.parentage(np.array([child, parent]), ["kid", "par"], offspring=["kid"], min_shared=M, backend="host")
        assert res.status == [status] and res.candidates == [1]
        assert res.trios == [[(1, 1, M, errors)]] and res.passes == [[errors == 3]]
        assert res.single == [None if errors == 3 else (1, M, 0)]
        pc.check_result(pc.parentage_ref([child.tolist(), parent.tolist()], ["kid", "par"], offspring=["kid"], min_shared=M), res)
    res = tf.parentage(np.array([child, parent]), ["kid", "par"], offspring=["kid"], min_shared=M + 1, backend="host")
    assert res.status == ["none"] and res.candidates == [0] and res.trios == [[]]


def test_pedigree_margins():
    worst_true, best_false = pc.pedigree_margins()
    limit = pc.ppm(pc.DEFAULTS["max_trio_err"])
    assert 2 * worst_true[0] * 10 ** 6 <= limit * worst_true[1], worst_true        # at most half the threshold
    assert best_false[0] * 10 ** 6 >= 2 * limit * best_false[1], best_false        # at least twice it
    _, _, truth = pc.pedigree()
    assert len(truth) == pc.PED_OFFSPRING and sum(1 for p, q in truth.values() if p == q) == 2


def test_pedigree_on_the_host_backend():
    calls, names, truth = pc.pedigree()
    ref = pc.pedigree_ref(True)
    assert all(r["status"] == "trio" and tuple(sorted(r["trios"][0][:2])) == truth[r["o"]] for r in ref)
    res = tf.parentage(calls, names, offspring=names[pc.PED_FOUNDERS:], parents=names[:pc.PED_FOUNDERS], backend="host")
    pc.check_result(ref, res)
    assert res.stats["backend"] == "host" and res.stats["used"] == res.stats["markers"] == pc.PED_MARKERS
    everyone = tf.parentage(calls, names, backend="host")
    pc.check_result(pc.pedigree_ref(False), everyone)
    masked = tf.parentage(calls, names, mask=np.arange(pc.PED_MARKERS) % 3 != 0, top=3, selfing=False, max_candidates=5, backend="host")
    pc.check_result(pc.parentage_ref(calls.tolist(), names, use=(np.arange(pc.PED_MARKERS) % 3 != 0).tolist(), top=3, selfing=False,
                                     max_candidates=5), masked)
    assert masked.stats["used"] == 400


def test_writers_and_cli_on_the_host(tmp_path, capsys):
    calls, names, _ = pc.pedigree()
    markers = ["m%03d" % m for m in range(pc.PED_MARKERS)]
    f = {k: str(tmp_path / k) for k in ("calls.csv", "p.csv", "t.csv", "p2.csv", "t2.csv", "off.txt", "par.txt")}
    open(f["calls.csv"], "wb").write(pc.calls_csv(names, markers, calls))
    ref = pc.pedigree_ref(False)
    res = tf.parentage(calls, names, backend="host")
    tf.writeParentage(f["p.csv"], res)
    tf.writeTrios(f["t.csv"], res)
    assert open(f["p.csv"], "rb").read() == pc.parentage_csv(names, ref)
    assert open(f["t.csv"], "rb").read() == pc.trios_csv(names, ref)
    assert len({r["status"] for r in ref}) >= 3    # the file shows filled and empty cells of both kinds
    assert tag_parentage.main(["-i", f["calls.csv"], "-o", f["p2.csv"], "--trios", f["t2.csv"], "--td-backend", "host"]) == 0
    assert capsys.readouterr().out == pc.summary_ref(ref) + "\n"
    assert open(f["p2.csv"], "rb").read() == pc.parentage_csv(names, ref) and open(f["t2.csv"], "rb").read() == pc.trios_csv(names, ref)
    open(f["off.txt"], "w").write("\n".join(names[pc.PED_FOUNDERS:]) + "\n")
    open(f["par.txt"], "w").write("\n".join(names[:pc.PED_FOUNDERS]) + "\n\n")
    assert tag_parentage.main(["-i", f["calls.csv"], "-o", f["p2.csv"], "--offspring", f["off.txt"], "--parents", f["par.txt"],
                               "--td-backend", "host"]) == 0
    assert capsys.readouterr().out == "Offspring: 20 Trio: 20 Ambiguous: 0 Single: 0 None: 0\n"
    assert open(f["p2.csv"], "rb").read() == pc.parentage_csv(names, pc.pedigree_ref(True))
    lists = pc.parentage_ref(calls.tolist(), names, max_pair_err=0.05, max_trio_err=0.01, min_shared=400, max_candidates=3, top=1, selfing=False)
    assert tag_parentage.main(["-i", f["calls.csv"], "-o", f["p2.csv"], "--trios", f["t2.csv"], "--max-pair-err", "0.05", "--max-trio-err", "0.01",
                               "--min-shared", "400", "--max-candidates", "3", "--top", "1", "--no-selfing", "--td-backend", "host"]) == 0
    assert capsys.readouterr().out == pc.summary_ref(lists) + "\n"
    assert open(f["p2.csv"], "rb").read() == pc.parentage_csv(names, lists) and open(f["t2.csv"], "rb").read() == pc.trios_csv(names, lists)


def test_tag_calls_parentage_on_the_host(tmp_path, capsys):
    """tag_calls --parentage from the pedigree's read depths, over the markers that pass, writes what tag_parentage writes
    from tag_calls' own -o file."""
    from tagdigger_amd import tag_calls
    _, names, _ = pc.pedigree()
    counts, tags = pc.pedigree_counts()
    f = {k: str(tmp_path / k) for k in ("counts.csv", "calls.csv", "p1.csv", "t1.csv", "p2.csv", "t2.csv", "off.txt", "par.txt")}
    tf.writeCounts(f["counts.csv"], counts, names, tags)
    open(f["off.txt"], "w").write("\n".join(names[pc.PED_FOUNDERS:]) + "\n")
    open(f["par.txt"], "w").write("\n".join(names[:pc.PED_FOUNDERS]) + "\n")
    assert tag_calls.main(["-i", f["counts.csv"], "-o", f["calls.csv"], "--min-call-rate", "0.9", "--parentage", f["p1.csv"], "--parentage-trios",
                           f["t1.csv"], "--parentage-offspring", f["off.txt"], "--parentage-parents", f["par.txt"], "--td-backend", "host"]) == 0
    line = capsys.readouterr().out.splitlines()[-1]
    assert tag_parentage.main(["-i", f["calls.csv"], "-o", f["p2.csv"], "--trios", f["t2.csv"], "--offspring", f["off.txt"], "--parents",
                               f["par.txt"], "--td-backend", "host"]) == 0
    assert capsys.readouterr().out == line + "\n" == "Offspring: 20 Trio: 20 Ambiguous: 0 Single: 0 None: 0\n"
    assert 100 < open(f["calls.csv"], "rb").read().split(b"\r\n")[0].count(b",") < pc.PED_MARKERS
    assert open(f["p1.csv"], "rb").read() == open(f["p2.csv"], "rb").read() and open(f["t1.csv"], "rb").read() == open(f["t2.csv"], "rb").read()
    with pytest.raises(Exception, match="go with --parentage"):
        tag_calls.main(["-i", f["counts.csv"], "-o", f["calls.csv"], "--parentage-trios", f["t1.csv"], "--td-backend", "host"])


def test_names_and_arguments():
    calls, names, _ = pc.pedigree()
    with pytest.raises(ValueError, match="offspring 'nobody'"):
        tf.parentage(calls, names, offspring=["K00", "nobody"], backend="host")
    with pytest.raises(ValueError, match="parent 'F99'"):
        tf.parentage(calls, names, parents=["F99"], backend="host")
    for kw in (dict(min_shared=0), dict(max_candidates=0), dict(max_candidates=pc.MAX_CAND + 1), dict(top=0), dict(top=pc.MAX_TOP + 1),
               dict(max_trio_err=1.5), dict(max_pair_err=-0.1), dict(backend="cpu"), dict(mask=[1, 0])):
        with pytest.raises(ValueError):
            tf.parentage(calls, names, **dict(dict(backend="host"), **kw))
    with pytest.raises(ValueError):
        tf.parentage(calls, names[:-1], backend="host")
    with pytest.raises(ValueError):
        tf.parentage(tf.DeviceCalls(0, (0, 0)), [], backend="host")
    empty = tf.parentage(np.zeros((0, 0), dtype=np.uint8), [], backend="host")
    assert empty.offspring == [] and empty.status == [] and empty.counts() == [0, 0, 0, 0]
    nothing = tf.parentage(np.zeros((3, 0), dtype=np.uint8), ["a", "b", "c"], backend="host")
    assert nothing.status == ["none"] * 3 and nothing.candidates == [0] * 3
