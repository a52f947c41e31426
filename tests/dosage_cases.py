"""Shared by tests/test_dosage.py and tests/test_dosage_gpu.py: the dosage-calling rule stated by brute
force in Python's integers, the inputs of the tests, and the checks that both backends go through.

ref_dosage walks sample by sample and marker by marker with plain ints and builds its own cost tables (fractions for the
probabilities, decimal at 80 digits through log10 for the logarithm): it imports nothing from the product."""
import decimal
import functools
import random
from fractions import Fraction
from math import comb

import genocall_cases as gc

STATS = ("called",) + tuple("n%d" % d for d in range(9)) + ("alt", "depth0", "depth1", "bin")
U32 = (1 << 32) - 1
NB = 64
MISSING = 255
COST_MAX = 1 << 23
PLOIDIES = (2, 3, 4, 6, 8)
PRIORS = ("flat", "hwe")
GRID_S = (1, 3, 65, 130)                                   # one chunk of 64 rows, two, and three with a short last one
GRID_M = (1, 63, 64, 65, 257, 260)


@functools.lru_cache(maxsize=None)
def ref_cost(x):
    """round_half_even(-65536 log2 x) of a Fraction 0 < x."""
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        bits = -(decimal.Decimal(x.numerator) / decimal.Decimal(x.denominator)).log10() / decimal.Decimal(2).log10()
        return int((bits * 65536).to_integral_value(rounding=decimal.ROUND_HALF_EVEN))


@functools.lru_cache(maxsize=None)
def ref_tables(P, err_ppm):
    """(CA, CB, CP): CA[d] the cost of an allele-1 read, CB[d] of an allele-0 read at dosage d, CP[k][d] of the prior."""
    e = Fraction(err_ppm, 10 ** 6)
    p = [(d * (1 - e) + (P - d) * e) / P for d in range(P + 1)]
    CA = tuple(ref_cost(x) for x in p)
    CB = tuple(ref_cost(1 - x) for x in p)
    CP = []
    for k in range(NB):
        q = Fraction(2 * k + 1, 2 * NB)
        CP.append(tuple(ref_cost(comb(P, d) * q ** d * (1 - q) ** (P - d)) for d in range(P + 1)))
    return CA, CB, tuple(CP)


def ref_margin(odds):
    return ref_cost(1 / Fraction(odds))


def ppm(x):
    return int(round(x * 1e6))


# two parameter sets: the defaults, and the depth threshold, another error rate and margin and both filters switched on
PARAMS = (dict(err_ppm=10000, min_depth=1, min_margin=ref_margin(10), min_call_ppm=0, min_maf_ppm=0),
          dict(err_ppm=2000, min_depth=3, min_margin=ref_margin(3), min_call_ppm=600000, min_maf_ppm=50000))


def ref_bin(depth0, depth1):
    tot = depth0 + depth1
    return 0 if tot == 0 else min(NB - 1, NB * depth1 // tot)


def ref_costs(a, b, CA, CB, prior):
    return [b * CA[d] + a * CB[d] + prior[d] for d in range(len(CA))]


def ref_cell(a, b, CA, CB, prior, min_depth, min_margin):
    """(code, margin) of one cell; margin is None below min_depth."""
    if a + b < min_depth:
        return MISSING, None
    c = ref_costs(a, b, CA, CB, prior)
    low = min(c)
    best = c.index(low)                                    # the smallest d of minimal cost
    margin = min(c[:best] + c[best + 1:]) - low
    return (best if margin >= min_margin else MISSING), margin


def ref_dosage(counts, i0, i1, P, prior, err_ppm=10000, min_depth=1, min_margin=0, min_call_ppm=0, min_maf_ppm=0, tables=None):
    """dict(calls [S][M], diploid [S][M], stats {name: [M]}, mask [M], passed) of the rule; counts: rows of ints."""
    CA, CB, CP = tables or ref_tables(P, err_ppm)
    S, M = len(counts), len(i0)
    calls = [[0] * M for _ in range(S)]
    stats = {k: [0] * M for k in STATS}
    mask = []
    for m in range(M):
        col = [(row[i0[m]], row[i1[m]]) for row in counts]
        depth0, depth1 = sum(a for a, _ in col), sum(b for _, b in col)
        k = ref_bin(depth0, depth1)
        row_prior = CP[k] if prior == "hwe" else (0,) * (P + 1)
        n = [0] * 9
        for s, (a, b) in enumerate(col):
            code = calls[s][m] = ref_cell(a, b, CA, CB, row_prior, min_depth, min_margin)[0]
            if code != MISSING:
                n[code] += 1
        called, alt = sum(n), sum(d * n[d] for d in range(9))
        for key, v in zip(STATS, [called] + n + [alt, depth0, depth1, k]):
            stats[key][m] = v
        mask.append(S > 0 and called * 10 ** 6 >= min_call_ppm * S and
                    min(alt, P * called - alt) * 10 ** 6 >= min_maf_ppm * P * called)
    diploid = [[3 if c == MISSING else 0 if c == 0 else 2 if c == P else 1 for c in row] for row in calls]
    return dict(calls=calls, diploid=diploid, stats=stats, mask=mask, passed=sum(mask))


def check_result(ref, calls, diploid, stats, mask, passed=None):
    """calls / diploid / stats / mask of the product (numpy) against the brute force, item by item."""
    assert calls.tolist() == ref["calls"]
    if diploid is not None:
        assert diploid.tolist() == ref["diploid"]
    for k in STATS:
        assert [int(v) for v in stats[k]] == ref["stats"][k], k
    assert [bool(v) for v in mask] == ref["mask"]
    if passed is not None:
        assert int(passed) == ref["passed"]


grid_case = gc.grid_case                                   # (counts, i0, i1, T), shared with the genotype tests


@functools.lru_cache(maxsize=None)
def grid_ref(S, M, scatter, P, prior, pset):
    counts, i0, i1, _ = grid_case(S, M, scatter)
    return ref_dosage(counts, i0, i1, P, prior, **PARAMS[pset])


def check_grid(run, M, P, prior, scatter):
    """run(counts, i0, i1, T, P, prior, **PARAMS[pset]) -> (calls, diploid, stats, mask, passed) over every S and both sets."""
    for S in GRID_S:
        counts, i0, i1, T = grid_case(S, M, scatter)
        for pset in (0, 1):
            got = run(counts, i0, i1, T, P, prior, **PARAMS[pset])
            check_result(grid_ref(S, M, scatter, P, prior, pset), *got)
            assert got[0].shape == (S, M) and got[1].shape == (S, M)


def binomial_counts(rng, S, M, P):
    """Adjacent columns; per marker an allele frequency, per cell a dosage drawn from it, a depth (a tenth empty, most
    between 1 and 40 reads, a few deep ones) and its reads drawn with 1 % error."""
    counts = [[0] * (2 * M) for _ in range(S)]
    for m in range(M):
        q = rng.random()
        for s in range(S):
            d = sum(rng.random() < q for _ in range(P))
            u = rng.random()
            n = 0 if u < 0.1 else rng.randint(1, 40) if u < 0.9 else rng.randint(100, 3000)
            p = (d * 0.99 + (P - d) * 0.01) / P
            b = sum(rng.random() < p for _ in range(n)) if n <= 40 else int(round(n * p))
            counts[s][2 * m], counts[s][2 * m + 1] = n - b, b
    return counts


@functools.lru_cache(maxsize=None)
def populated_case(P=6, prior="hwe"):
    """One case under the second parameter set on which every class 0 .. P occurs, a cell is missing by depth and a cell
    with enough reads is missing by margin, and some markers pass and some fail (all asserted here)."""
    S, M = 65, 65
    counts = binomial_counts(random.Random(2323), S, M, P)
    i0, i1, T = gc.adjacent(M)
    par = PARAMS[1]
    ref = ref_dosage(counts, i0, i1, P, prior, **par)
    codes = {c for row in ref["calls"] for c in row}
    assert codes == set(range(P + 1)) | {MISSING}, codes
    by_depth = by_margin = 0
    for s in range(S):
        for m in range(M):
            if ref["calls"][s][m] == MISSING:
                shallow = counts[s][i0[m]] + counts[s][i1[m]] < par["min_depth"]
                by_depth += shallow
                by_margin += not shallow
    assert by_depth > 0 and by_margin > 0, (by_depth, by_margin)
    assert 0 < ref["passed"] < M, ref["passed"]
    return counts, i0, i1, T, ref


def margin_edge_cases():
    """(P, a, b, delta): cells under the flat prior whose margin delta is positive, from the tables."""
    out = []
    for P, a, b in ((4, 7, 5), (2, 9, 2), (8, 13, 30), (3, 1, 0)):
        CA, CB, _ = ref_tables(P, 10000)
        code, delta = ref_cell(a, b, CA, CB, (0,) * (P + 1), 1, 0)
        assert code != MISSING and delta > 0
        out.append((P, a, b, delta))
    return out


def bin_edge_cases():
    """(counts, expected bin) with one marker at columns 0, 1: 64 depth1 == k tot exactly and one allele-1 read less, every
    read of allele 1 (clamped to the last bin), and no read at all."""
    cases = []
    for k in (1, 17, 63):
        cases.append(([[128 - 2 * k, 0], [0, 2 * k]], k))                 # tot 128, depth1 2 k
        cases.append(([[129 - 2 * k, 0], [0, 2 * k - 1]], k - 1))         # tot 128, depth1 2 k - 1
    cases.append(([[0, 5], [0, U32]], NB - 1))
    cases.append(([[0, 0], [0, 0], [0, 0]], 0))
    for counts, k in cases:
        assert ref_bin(sum(r[0] for r in counts), sum(r[1] for r in counts)) == k
    return cases


@functools.lru_cache(maxsize=None)
def bin_flip_case(P=4, err_ppm=10000):
    """Two markers (columns 0, 1 and 2, 3) whose first sample holds the same cell (a, b), called differently because a
    second sample's reads put the markers into the neighbouring bins k and k + 1.  Searched for, and asserted found."""
    CA, CB, CP = ref_tables(P, err_ppm)
    for k in range(1, NB - 2):
        for a in range(0, 12):
            for b in range(0, 12):
                if a + b == 0:
                    continue
                lo = ref_cell(a, b, CA, CB, CP[k], 1, 0)[0]
                hi = ref_cell(a, b, CA, CB, CP[k + 1], 1, 0)[0]
                if lo != hi:
                    def filler(kk):                        # tot 6400, depth1 100 kk + 50: the middle of bin kk
                        return [6400 - (100 * kk + 50) - a, 100 * kk + 50 - b]
                    counts = [[a, b, a, b], filler(k) + filler(k + 1)]
                    ref = ref_dosage(counts, [0, 2], [1, 3], P, "hwe", err_ppm=err_ppm)
                    assert ref["stats"]["bin"] == [k, k + 1] and ref["calls"][0] == [lo, hi] and lo != hi
                    return counts, [0, 2], [1, 3], 4, ref
    raise AssertionError("no cell changes its call between two neighbouring bins")


def filter_boundary_cases():
    """(counts, params, passes) for P = 4, flat prior, margin 0, one marker over 8 samples, placed so that the left side of
    one inequality equals its right side (passes) or lies one unit below it (fails).  The rows spell the dosages:
    (40, 0) -> 0, (30, 10) -> 1, (20, 20) -> 2, (10, 30) -> 3, (0, 40) -> 4, (0, 0) -> missing (asserted in the tests
    through the statistics of the brute force)."""
    cell = {0: [40, 0], 1: [30, 10], 2: [20, 20], 3: [10, 30], 4: [0, 40], None: [0, 0]}

    def rows(*doses):
        return [cell[d] for d in doses]
    N = None
    cases = []
    # call rate: called / 8 against 0.75 -> 6 called is equality (6 * 10^6 = 750 000 * 8), 5 called is below
    cases.append((rows(0, 1, 2, 3, 4, 0, N, N), dict(min_call_ppm=750000), True, (6, 10)))
    cases.append((rows(0, 1, 2, 3, 4, N, N, N), dict(min_call_ppm=750000), False, (5, 10)))
    # minor allele frequency: minor / (4 called) against 0.125 -> called 8, 32 copies, minor 4 is equality, 3 is below
    cases.append((rows(0, 0, 0, 0, 0, 0, 1, 3), dict(min_maf_ppm=125000), True, (8, 4)))
    cases.append((rows(0, 0, 0, 0, 0, 0, 1, 2), dict(min_maf_ppm=125000), False, (8, 3)))
    # ... and with allele 1 the commoner one: minor = 4 called - alt
    cases.append((rows(4, 4, 4, 4, 4, 4, 3, 1), dict(min_maf_ppm=125000), True, (8, 28)))
    cases.append((rows(4, 4, 4, 4, 4, 4, 3, 2), dict(min_maf_ppm=125000), False, (8, 29)))
    # nobody called: passes only with min_call_ppm = 0
    cases.append((rows(N, N, N, N, N, N, N, N), dict(), True, (0, 0)))
    cases.append((rows(N, N, N, N, N, N, N, N), dict(min_call_ppm=1), False, (0, 0)))
    return cases


# the largest counts: costs beyond 2^52 with the err = 1 ppm, P = 8 tables; the depth sums pass 2^32
EXTREME_CELLS = ((U32, U32), (U32, 0), (0, U32), (U32, U32 - 1), (U32 - 1, U32), (U32, 1), (1, U32), (1 << 31, 1 << 24),
                 (U32, U32 // 7), (U32 // 8 * 3, U32 // 8 * 5), (0, 0), (1, 1))


def extreme_case():
    """One marker, one sample per cell of EXTREME_CELLS."""
    return [[a, b] for a, b in EXTREME_CELLS], [0], [1], 2


def mixed_layout_case():
    """Adjacent columns with a few markers' alleles swapped or moved: lanes that take the 8-byte load next to lanes that
    cannot, in one wave."""
    counts, i0, i1, T = grid_case(65, 64)
    i0, i1 = list(i0), list(i1)
    i0[5], i1[5] = i1[5], i0[5]                            # allele 1 in front of allele 0
    i1[22] = i1[40]                                        # two markers share a column (the C-ABI takes any indices)
    i0[49], i0[50] = i0[50], i0[49]
    return counts, i0, i1, T


def check_knife_edges(run):
    """The edges both backends must hold; run as in check_grid (keyword parameters default as in ref_dosage)."""
    for P, a, b, delta in margin_edge_cases():
        for margin, called in ((delta, True), (delta + 1, False)):
            ref = ref_dosage([[a, b]], [0], [1], P, "flat", min_margin=margin)
            assert (ref["calls"][0][0] != MISSING) == called
            check_result(ref, *run([[a, b]], [0], [1], 2, P, "flat", min_margin=margin))
    # an exact tie: odd ploidy, a == b, flat prior -> the lower of the two middle dosages at margin 0, missing at margin 1
    for P in (3, 5, 7):
        for margin, want in ((0, (P - 1) // 2), (1, MISSING)):
            ref = ref_dosage([[5, 5]], [0], [1], P, "flat", min_margin=margin)
            assert ref["calls"] == [[want]]
            check_result(ref, *run([[5, 5]], [0], [1], 2, P, "flat", min_margin=margin))
    for counts, k in bin_edge_cases():
        for prior in PRIORS:                               # the bin is reported under both priors
            ref = ref_dosage(counts, [0], [1], 4, prior)
            assert ref["stats"]["bin"] == [k]
            check_result(ref, *run(counts, [0], [1], 2, 4, prior))
    counts, i0, i1, T, ref = bin_flip_case()
    check_result(ref, *run(counts, i0, i1, T, 4, "hwe"))
    for counts, params, passes, (called, alt) in filter_boundary_cases():
        ref = ref_dosage(counts, [0], [1], 4, "flat", **params)
        assert ref["mask"] == [passes] and ref["stats"]["called"] == [called] and ref["stats"]["alt"] == [alt]
        check_result(ref, *run(counts, [0], [1], 2, 4, "flat", **params))


def check_extremes(run):
    counts, i0, i1, T = extreme_case()
    tables = ref_tables(8, 1)
    assert max(tables[0]) == 1306235 and max(max(r) for r in tables[2]) < COST_MAX
    assert max(ref_costs(U32, U32, tables[0], tables[1], tables[2][0])) > 1 << 52     # far beyond what a double holds exactly
    for prior in PRIORS:
        for min_depth, min_margin in ((1, 0), (1, ref_margin(10)), (1 << 33, 0)):
            ref = ref_dosage(counts, i0, i1, 8, prior, err_ppm=1, min_depth=min_depth, min_margin=min_margin)
            assert ref["stats"]["depth0"][0] > 1 << 32 and ref["stats"]["depth1"][0] > 1 << 32
            if min_depth > 1:
                assert ref["stats"]["called"] == [0]       # 2^33 - 2 reads at the most
            check_result(ref, *run(counts, i0, i1, T, 8, prior, err_ppm=1, min_depth=min_depth, min_margin=min_margin))
    # all samples missing, by depth and because nothing was read
    counts, i0, i1, T = grid_case(65, 64)
    for min_call_ppm, passed in ((0, 64), (10000, 0)):
        ref = ref_dosage(counts, i0, i1, 4, "hwe", min_depth=1 << 34, min_call_ppm=min_call_ppm)
        assert ref["passed"] == passed and ref["stats"]["called"] == [0] * 64
        check_result(ref, *run(counts, i0, i1, T, 4, "hwe", min_depth=1 << 34, min_call_ppm=min_call_ppm))
    zeros = [[0] * T for _ in range(3)]
    ref = ref_dosage(zeros, i0, i1, 4, "hwe")
    assert ref["stats"]["bin"] == [0] * 64 and ref["stats"]["called"] == [0] * 64
    check_result(ref, *run(zeros, i0, i1, T, 4, "hwe"))
    counts, i0, i1, T = mixed_layout_case()
    for P, prior in ((4, "hwe"), (3, "flat")):
        check_result(ref_dosage(counts, i0, i1, P, prior, **PARAMS[1]), *run(counts, i0, i1, T, P, prior, **PARAMS[1]))


def check_orientation(run):
    """The code counts the copies of allele 1 -- the tag of column i1: reads of allele 0 alone are dosage 0, of allele 1
    alone dosage P, and for P = 2 the clear cells are call_genotypes' codes."""
    for P in PLOIDIES:
        counts = [[30, 0], [0, 30], [15, 15]] if P % 2 == 0 else [[30, 0], [0, 30]]
        want = [[0], [P], [P // 2]][:len(counts)]
        ref = ref_dosage(counts, [0], [1], P, "flat")
        assert ref["calls"] == want
        check_result(ref, *run(counts, [0], [1], 2, P, "flat"))
    clear = [[20, 0], [0, 20], [10, 10], [200, 2], [3, 300]]
    assert ref_dosage(clear, [0], [1], 2, "flat")["calls"] == gc.ref_calls(clear, [0], [1])["calls"] == [[0], [2], [1], [0], [2]]
