"""Shared by tests/test_parentage.py and tests/test_parentage_gpu.py: the Mendelian trio counts, their ranking, the choice
of the candidates and the decision of DESIGN 4.18 stated by plain loops in Python's integers, the bytes of the two CSV
files, and the inputs of the tests.  It imports nothing from the product.

For an offspring o and two parents p, q, over the participating markers at which all three are called (codes 0 / 1 / 2;
any byte above 2 is missing; marker m takes part iff there is no mask or use[m] != 0): n = their number, e = those at
which the offspring's call is not in ALLOWED[parents' calls]."""
import functools
import random

import numpy as np

import relate_cases as rc

MAX_SAMPLES, MAX_CAND, MAX_TOP, BLOCK, WCHUNK = 16384, 128, 8, 64, 16
NONE = 0xFFFFFFFF
TRIO = [("p", "<u4"), ("q", "<u4"), ("n", "<u4"), ("e", "<u4")]
DEFAULTS = dict(max_pair_err=0.03, max_trio_err=0.03, min_shared=50, max_candidates=32, top=2, selfing=True)

# what two parents can produce, by their calls (the smaller first)
ALLOWED = {(0, 0): {0}, (0, 1): {0, 1}, (0, 2): {1}, (1, 1): {0, 1, 2}, (1, 2): {1, 2}, (2, 2): {2}}


def is_error(o, p, q):
    return o not in ALLOWED[(min(p, q), max(p, q))]


def plane_error(o, p, q):
    """The expression of include/tagdig.h on one marker's bits."""
    o0, o1, o2 = int(o == 0), int(o == 1), int(o == 2)
    p0, p2, q0, q2 = int(p == 0), int(p == 2), int(q == 0), int(q == 2)
    return (o2 & (p0 | q0)) | (o0 & (p2 | q2)) | (o1 & ((p0 & q0) | (p2 & q2)))


def check_plane_expression():
    """All 27 combinations: the bit expression is the table."""
    seen = 0
    for o in range(3):
        for p in range(3):
            for q in range(3):
                assert plane_error(o, p, q) == int(is_error(o, p, q)), (o, p, q)
                assert is_error(o, p, q) == is_error(o, q, p)
                seen += 1
    assert seen == 27 and sum(is_error(o, p, q) for o in range(3) for p in range(3) for q in range(3)) == 12


def slot_pairs(C, selfing):
    """The trios of C candidate slots in their numbering: a ascending, then b ascending."""
    return [(a, b) for a in range(C) for b in range(a if selfing else a + 1, C)]


def trio_count(rows, used, o, p, q):
    """(n, e) of one trio: the loop over the markers.  rows: lists of ints; used: the participating markers."""
    ro, rp, rq = rows[o], rows[p], rows[q]
    n = e = 0
    for m in used:
        a, b, c = ro[m], rp[m], rq[m]
        if a <= 2 and b <= 2 and c <= 2:
            n += 1
            if a not in ALLOWED[(b, c) if b <= c else (c, b)]:
                e += 1
    return n, e


def table_ref(calls, use, offspring, cand, selfing):
    """[O][T] of (n, e), every trio by trio_count (a pair of samples is counted once per offspring and shared by the
    slots that name it); a pair with an empty slot has n = e = 0."""
    rows = [[int(c) for c in row] for row in calls]
    M = len(rows[0]) if rows else 0
    used = [m for m in range(M) if use is None or use[m]]
    out = []
    for i, o in enumerate(offspring):
        memo, line = {}, []
        for a, b in slot_pairs(len(cand[i]), selfing):
            p, q = int(cand[i][a]), int(cand[i][b])
            if p < 0 or q < 0:
                line.append((0, 0))
                continue
            key = (min(p, q), max(p, q))
            if key not in memo:
                memo[key] = trio_count(rows, used, int(o), p, q)
            line.append(memo[key])
        out.append(line)
    return out


def before(x, y):
    """Trio x = (n, e, t) comes before trio y: the tuple rule in Python's integers."""
    if x[1] * y[0] != y[1] * x[0]:
        return x[1] * y[0] < y[1] * x[0]
    if x[0] != y[0]:
        return x[0] > y[0]
    return x[2] < y[2]


def rank_ref(line, min_shared):
    """The ranked trios of one row, best first: [(n, e, t)]."""
    live = [(n, e, t) for t, (n, e) in enumerate(line) if n >= min_shared]
    return sorted(live, key=functools.cmp_to_key(lambda x, y: -1 if before(x, y) else 1))


def best_ref(table, cand, selfing, K, min_shared):
    """The records td_parent_trios must return: structured [O, K]."""
    O = len(table)
    best = np.zeros((O, K), dtype=TRIO)
    best["p"] = best["q"] = NONE
    for i in range(O):
        pairs = slot_pairs(len(cand[i]), selfing)
        for k, (n, e, t) in enumerate(rank_ref(table[i], min_shared)[:K]):
            a, b = pairs[t]
            best[i, k] = (int(cand[i][a]), int(cand[i][b]), n, e)
    return best


def table_array(table):
    O = len(table)
    T = len(table[0]) if O else 0
    return np.array(table, dtype=np.uint32).reshape(O, T, 2)


def check(ref_table, cand, selfing, K, min_shared, got_best, got_table):
    """Both outputs of the product against the reference, as np.array_equal."""
    want_table, want_best = table_array(ref_table), best_ref(ref_table, cand, selfing, K, min_shared)
    assert got_table.dtype == np.uint32 and got_table.shape == want_table.shape, (got_table.shape, want_table.shape)
    assert np.array_equal(got_table, want_table), np.argwhere(got_table != want_table)[:5].tolist()
    assert got_best.shape == want_best.shape
    for k in ("p", "q", "n", "e"):
        assert np.array_equal(got_best[k], want_best[k]), (k, got_best[k].tolist()[:3], want_best[k].tolist()[:3])
    return want_best


# ------------------------------------------------------------------ candidates, decision, files
def ppm(x):
    return int(round(x * 1e6))


def candidates_ref(pairs, o, allowed, min_shared, pair_ppm, max_candidates):
    """pairs[o][p] = (n2, e2).  The candidate parents of o, in order."""
    ok = [p for p in allowed if p != o and pairs[o][p][0] >= min_shared and pairs[o][p][1] * 10 ** 6 <= pair_ppm * pairs[o][p][0]]

    def cmp(x, y):
        (nx, ex), (ny, ey) = pairs[o][x], pairs[o][y]
        return -1 if (ex * ny, -nx, x) < (ey * nx, -ny, y) else 1

    return sorted(ok, key=functools.cmp_to_key(cmp))[:max_candidates]


def pair_numbers(calls, use):
    """pairs[o][p] = (n2, e2) for all samples: markers called in both, opposing homozygotes, by plain loops."""
    rows = [[int(c) for c in row] for row in calls]
    S = len(rows)
    used = [m for m in range(len(rows[0]) if S else 0) if use is None or use[m]]
    out = [[(0, 0)] * S for _ in range(S)]
    for o in range(S):
        for p in range(o, S):
            n = e = 0
            for m in used:
                a, b = rows[o][m], rows[p][m]
                if a <= 2 and b <= 2:
                    n += 1
                    e += a + b == 2 and a != 1
            out[o][p] = out[p][o] = (n, e)
    return out


def decide(ranked, trio_ppm, ncand):
    """The status from the ranked trios [(n, e, t)] of one offspring."""
    ok = [e * 10 ** 6 <= trio_ppm * n for n, e, _ in ranked[:2]]
    if ok[:1] == [True]:
        return "ambiguous" if ok[1:2] == [True] else "trio"
    return "single" if ncand else "none"


def parentage_ref(calls, names, offspring=None, parents=None, use=None, max_pair_err=0.03, max_trio_err=0.03, min_shared=50,
                  max_candidates=32, top=2, selfing=True):
    """The whole decision by the loops above: a list with one dict per offspring (o, status, trios [(p, q, n, e, pass)]
    up to top, single (p, n2, e2) or None, candidates)."""
    where = {n: k for k, n in reversed(list(enumerate(names)))}
    off = list(range(len(names))) if offspring is None else [where[n] for n in offspring]
    allowed = sorted(set(range(len(names)) if parents is None else (where[n] for n in parents)))
    pairs = pair_numbers(calls, use)
    out = []
    for o in off:
        cand = candidates_ref(pairs, o, allowed, min_shared, ppm(max_pair_err), max_candidates)
        line = table_ref(calls, use, [o], [cand], selfing)[0] if cand else []
        ranked = rank_ref(line, min_shared)
        sp = slot_pairs(len(cand), selfing)
        status = decide(ranked, ppm(max_trio_err), len(cand))
        trios = [(cand[sp[t][0]], cand[sp[t][1]], n, e, e * 10 ** 6 <= ppm(max_trio_err) * n) for n, e, t in ranked[:top]]
        single = (cand[0],) + pairs[o][cand[0]] if status == "single" else None
        out.append(dict(o=o, status=status, trios=trios, single=single, candidates=len(cand)))
    return out


def rate_text(e, n):
    return "NA" if n == 0 else format(e / n, ".6f")


def parentage_csv(names, ref):
    """The bytes writeParentage must write."""
    lines = ["offspring,status,parent1,parent2,shared,errors,error_rate,single_parent,pair_shared,pair_errors,pair_error_rate,candidates"]
    for r in ref:
        trio, one = [""] * 5, [""] * 4
        if r["status"] in ("trio", "ambiguous"):
            p, q, n, e, _ = r["trios"][0]
            trio = [names[p], names[q], str(n), str(e), rate_text(e, n)]
        if r["single"] is not None:
            p, n, e = r["single"]
            one = [names[p], str(n), str(e), rate_text(e, n)]
        lines.append(",".join([names[r["o"]], r["status"]] + trio + one + [str(r["candidates"])]))
    return ("\r\n".join(lines) + "\r\n").encode("ascii")


def trios_csv(names, ref):
    """The bytes writeTrios must write."""
    lines = ["offspring,rank,parent1,parent2,shared,errors,error_rate,pass"]
    for r in ref:
        for k, (p, q, n, e, ok) in enumerate(r["trios"]):
            lines.append(",".join([names[r["o"]], str(k + 1), names[p], names[q], str(n), str(e), rate_text(e, n), "1" if ok else "0"]))
    return ("\r\n".join(lines) + "\r\n").encode("ascii")


def summary_ref(ref):
    count = [sum(1 for r in ref if r["status"] == k) for k in ("trio", "ambiguous", "single", "none")]
    return "Offspring: {} Trio: {} Ambiguous: {} Single: {} None: {}".format(len(ref), *count)


def check_result(ref, result):
    """A ParentageResult of the product against parentage_ref, item by item."""
    assert list(result.offspring) == [r["o"] for r in ref]
    assert list(result.status) == [r["status"] for r in ref]
    assert [list(map(tuple, t)) for t in result.trios] == [[x[:4] for x in r["trios"]] for r in ref]
    assert [list(p) for p in result.passes] == [[x[4] for x in r["trios"]] for r in ref]
    assert list(result.single) == [r["single"] for r in ref]
    assert list(result.candidates) == [r["candidates"] for r in ref]


# ------------------------------------------------------------------ inputs
def shuffled_candidates(S, offspring, C, seed, holes=()):
    """One row of C slots per offspring: distinct samples other than the offspring in a shuffled, non-ascending order,
    -1 at the slots named in holes (of the first row only; the rows differ)."""
    rng = random.Random(seed)
    rows = []
    for i, o in enumerate(offspring):
        others = [s for s in range(S) if s != o]
        while True:
            rng.shuffle(others)
            row = others[:C]
            if len(row) < 2 or any(x > y for x, y in zip(row, row[1:])):
                break
        if i == 0:
            for h in holes:
                row[h] = -1
        rows.append(row)
    return np.array(rows, dtype=np.int32).reshape(len(offspring), C)


EDGE_M = (1, 63, 64, 65, 127, 129, 64 * WCHUNK - 1, 64 * WCHUNK, 64 * WCHUNK + 1, 2 * 64 * WCHUNK + 3)
EDGE_S, EDGE_C = 9, 5
EDGE_OFFSPRING = (4, 0, 8)
EDGE_MASKS = ("none", "random", "seam", "no_second_chunk")


def edge_mask(M, kind):
    """The masks of the word and chunk edges: none, random bytes, only the two markers either side of the chunk seam, and
    everything but the second chunk.  None where the kind does not apply at this M."""
    seam = 64 * WCHUNK
    if kind == "none":
        return None
    if kind == "random":
        return rc.random_mask(M)
    if M <= seam:
        return None
    use = np.zeros(M, dtype=np.uint8)
    if kind == "seam":
        use[seam - 1:seam + 1] = (1, 200)
    else:
        use[:] = 1
        use[seam:2 * seam] = 0
    return use


# every M with no mask and a random one; the two seam masks where there is a second chunk
EDGE_CASES = tuple((M, kind) for M in EDGE_M for kind in EDGE_MASKS if kind in ("none", "random") or M > 64 * WCHUNK)


@functools.lru_cache(maxsize=None)
def edge_case(M, kind):
    """(calls, use, offspring, cand, reference table) or None.  Calls of codes 0 .. 2 with a tenth missing (3 and wild
    bytes), so that n and e are large and differ from trio to trio."""
    use = edge_mask(M, kind)
    if kind != "none" and use is None:
        return None
    rng = np.random.default_rng(5100 + M)
    calls = rng.integers(0, 3, size=(EDGE_S, M), dtype=np.uint8)
    gone = rng.random((EDGE_S, M)) < 0.1
    calls[gone] = rng.choice(np.array([3, 3, 4, 77, 255], dtype=np.uint8), size=int(gone.sum()))
    cand = shuffled_candidates(EDGE_S, EDGE_OFFSPRING, EDGE_C, 77 + M, holes=(2,))
    return calls, use, list(EDGE_OFFSPRING), cand, table_ref(calls.tolist(), use, EDGE_OFFSPRING, cand.tolist(), True)


SLOT_C = (1, 2, 3, 4, 5, BLOCK // 2 - 1, BLOCK // 2, BLOCK // 2 + 1, BLOCK - 1, BLOCK, BLOCK + 1, 128)     # (up to BLOCK candidates the blocks are half as wide)
SLOT_M = 130


@functools.lru_cache(maxsize=None)
def slot_case(C, selfing):
    """S = C + 2 samples, M = 130, two offspring rows (the last two samples) with different shuffled candidate lists; the
    first row has holes at the first, a middle and the last slot where C >= 4, at the first where C is 2 or 3."""
    S = C + 2
    calls = rc.random_calls(S, SLOT_M)
    offspring = [S - 1, S - 2]
    holes = (0, C // 2, C - 1) if C >= 4 else (0,) if C >= 2 else ()
    cand = shuffled_candidates(S, offspring, C, 900 + C, holes=holes)
    return calls, offspring, cand, table_ref(calls.tolist(), None, offspring, cand.tolist(), selfing)


def orientation_case():
    """Constant rows: 0 = all 0, 1 = all 1, 2 = all 2, 3 = all missing, 4 = all 0 again; M = 70.  The same samples serve
    as offspring in one row and as parents in the other."""
    M = 70
    calls = np.array([[0] * M, [1] * M, [2] * M, [9] * M, [0] * M], dtype=np.uint8)
    offspring = [1, 0]
    cand = np.array([[0, 2, 3], [1, 2, 3]], dtype=np.int32)
    return calls, offspring, cand, M


RANK_MIN_SHARED = 20
RANK_TRIOS = ((100, 10), (60, 3), (50, 5), (60, 3), (RANK_MIN_SHARED, 0), (RANK_MIN_SHARED - 1, 0), (40, 40))
# by the rule: (20, 0) t = 4; then e / n = 1 / 20 twice, t = 1 before t = 3; then 1 / 10 with n = 100 (t = 0) before n = 50
# (t = 2); then (40, 40); (19, 0) is not ranked
RANK_ORDER = (4, 1, 3, 0, 2, 6)


def rank_case():
    """A hand-built table: the offspring is heterozygous everywhere; candidate a is called on a stretch of markers of its
    own, e_a times 0 and n_a - e_a times 1, so that the trio (a, a) has (n_a, e_a) and every trio of two different
    candidates shares no marker.  Row 0 has all candidates, row 1 only the one below min_shared and holes: none ranked.
    Returns (calls, offspring, cand, the diagonal trio numbers of row 0 in candidate order)."""
    M = sum(n for n, _ in RANK_TRIOS)
    C = len(RANK_TRIOS)
    calls = np.full((C + 1, M), 3, dtype=np.uint8)
    calls[C] = 1
    lo = 0
    for a, (n, e) in enumerate(RANK_TRIOS):
        calls[a, lo:lo + e] = 0
        calls[a, lo + e:lo + n] = 1
        lo += n
    cand = np.array([list(range(C)), [-1, 5] + [-1] * (C - 2)], dtype=np.int32)
    diagonal = [slot_pairs(C, True).index((a, a)) for a in range(C)]
    return calls, [C, C], cand, diagonal


# ------------------------------------------------------------------ the pedigree
PED_FOUNDERS, PED_OFFSPRING, PED_MARKERS, PED_SEED = 12, 20, 600, 3


@functools.lru_cache(maxsize=None)
def pedigree(seed=PED_SEED):
    """(calls uint8 [32, 600] read-only, names, truth {offspring index: (p, q)}): 12 founders drawn at allele frequencies
    in 0.1 .. 0.9; 20 offspring of two founders each, the first two selfed; 10 % of the calls missing; 1 % of the
    heterozygotes under-called to one of the homozygotes."""
    rng = random.Random(seed)
    F, N, M = PED_FOUNDERS, PED_OFFSPRING, PED_MARKERS
    freq = [rng.uniform(0.1, 0.9) for _ in range(M)]
    haps = [[[int(rng.random() < freq[m]) for m in range(M)] for _ in range(2)] for _ in range(F)]
    truth = {}
    for k in range(N):
        p = rng.randrange(F)
        q = p if k < 2 else rng.choice([x for x in range(F) if x != p])
        truth[F + k] = (min(p, q), max(p, q))
        haps.append([[haps[x][rng.randrange(2)][m] for m in range(M)] for x in (p, q)])
    rows = []
    for h in haps:
        row = []
        for m in range(M):
            g = h[0][m] + h[1][m]
            if g == 1 and rng.random() < 0.01:
                g = rng.choice((0, 2))
            row.append(3 if rng.random() < 0.10 else g)
        rows.append(row)
    calls = np.array(rows, dtype=np.uint8)
    calls.setflags(write=False)
    names = ["F%02d" % k for k in range(F)] + ["K%02d" % k for k in range(N)]
    return calls, names, truth


def pedigree_margins(seed=PED_SEED):
    """(largest e / n of a true trio, smallest e / n of a false trio among the founders), as (e, n) pairs, over all
    offspring; a trio of founders is false unless it is the true pair."""
    calls, _, truth = pedigree(seed)
    rows, used = calls.tolist(), list(range(PED_MARKERS))
    worst_true, best_false = (0, 1), (1, 1)
    for o, (p, q) in truth.items():
        for a in range(PED_FOUNDERS):
            for b in range(a, PED_FOUNDERS):
                n, e = trio_count(rows, used, o, a, b)
                if (a, b) == (p, q):
                    if e * worst_true[1] > worst_true[0] * n:
                        worst_true = (e, n)
                elif e * best_false[1] < best_false[0] * n:
                    best_false = (e, n)
    return worst_true, best_false


@functools.lru_cache(maxsize=None)
def pedigree_ref(lists):
    """parentage_ref of the pedigree under the defaults: lists=True with parents = the founders and offspring = the rest,
    False with both None."""
    calls, names, _ = pedigree()
    if lists:
        return parentage_ref(calls.tolist(), names, offspring=names[PED_FOUNDERS:], parents=names[:PED_FOUNDERS])
    return parentage_ref(calls.tolist(), names)


def pedigree_counts():
    """(counts uint32 [32, 1200], tag names): read depths from which tag_calls' default rule calls the pedigree's matrix
    again -- 12 reads of the one tag, 6 of each, or none; marker m at columns 2 m and 2 m + 1."""
    calls, _, _ = pedigree()
    depth = np.array([[12, 0], [6, 6], [0, 12], [0, 0]], dtype=np.uint32)
    counts = depth[np.minimum(calls, 3)].reshape(calls.shape[0], 2 * PED_MARKERS)
    return counts, [name for m in range(PED_MARKERS) for name in ("Mk%05d_0" % m, "Mk%05d_1" % m)]


def calls_csv(names, markers, calls):
    """writeGenoCalls' layout: the bytes tag_parentage reads."""
    lines = [",".join([""] + list(markers))]
    for name, row in zip(names, calls.tolist()):
        lines.append(",".join([name] + ["" if c > 2 else str(c) for c in row]))
    return ("\r\n".join(lines) + "\r\n").encode("ascii")
