"""Shared by tests/test_genocall.py and tests/test_genocall_gpu.py: the genotype-calling rule stated by
brute force in Python's integers, and the inputs of the tests.

ref_calls walks sample by sample and marker by marker with plain ints and builds its own threshold table with
fractions.Fraction: it imports nothing from the product."""
import functools
import random
from fractions import Fraction

STATS = ("called", "n0", "n1", "n2", "alt", "depth0", "depth1")
U32 = (1 << 32) - 1
# two parameter sets: the defaults, and every filter and the depth threshold switched on
PARAMS = (dict(err=0.01, min_depth=1, min_call_rate=0.0, min_maf=0.0, max_het=1.0),
          dict(err=0.002, min_depth=3, min_call_rate=0.6, min_maf=0.05, max_het=0.75))
RULES = ("likelihood", "presence")


def ppm(x):
    return int(round(x * 1e6))


@functools.lru_cache(maxsize=None)
def ref_table(err_ppm):
    """het_min[0 .. 127]: the smallest k in 0 .. n // 2 with (1/2)^n > (1 - e)^(n - k) e^k, n + 1 when there is none."""
    e = Fraction(err_ppm, 10 ** 6)
    table = [1]
    for n in range(1, 128):
        found = n + 1
        for k in range(n // 2 + 1):
            if Fraction(1, 2 ** n) > (1 - e) ** (n - k) * e ** k:
                found = k
                break
        table.append(found)
    return tuple(table)


def ref_code(a, b, rule, table, min_depth):
    n = a + b
    if n < min_depth:
        return 3
    if rule == "presence":
        return 1 if a > 0 and b > 0 else 0 if a > 0 else 2
    if n > 127:
        a, b = 127 * a // n, 127 * b // n
    if min(a, b) >= table[a + b]:
        return 1
    return 0 if a >= b else 2


def ref_calls(counts, i0, i1, rule="likelihood", err=0.01, min_depth=1, min_call_rate=0.0, min_maf=0.0, max_het=1.0):
    """dict(calls [S][M], stats {name: [M]}, mask [M], passed) of the rule; counts is a list of rows of ints."""
    table = ref_table(ppm(err))
    S, M = len(counts), len(i0)
    calls = [[ref_code(row[i0[m]], row[i1[m]], rule, table, min_depth) for m in range(M)] for row in counts]
    stats = {k: [0] * M for k in STATS}
    mask = []
    for m in range(M):
        col = [calls[s][m] for s in range(S)]
        n0, n1, n2 = col.count(0), col.count(1), col.count(2)
        called, alt = n0 + n1 + n2, n1 + 2 * n2
        for k, v in zip(STATS, (called, n0, n1, n2, alt, sum(row[i0[m]] for row in counts), sum(row[i1[m]] for row in counts))):
            stats[k][m] = v
        mask.append(S > 0 and called * 10 ** 6 >= ppm(min_call_rate) * S and
                    min(alt, 2 * called - alt) * 10 ** 6 >= ppm(min_maf) * 2 * called and
                    n1 * 10 ** 6 <= ppm(max_het) * called)
    return dict(calls=calls, stats=stats, mask=mask, passed=sum(mask))


def assert_populated(ref, counts, i0, i1):
    """Every class of the rule is there: codes 0, 1, 2 and 3, markers that pass and markers that fail, and a cell with
    more than 127 reads.  An expectation without one of them must not pass by accident."""
    codes = {c for row in ref["calls"] for c in row}
    assert codes == {0, 1, 2, 3}, codes
    assert 0 < ref["passed"] < len(ref["mask"]), ref["passed"]
    assert any(row[i0[m]] + row[i1[m]] > 127 for row in counts for m in range(len(i0)))


def marker_names(M):
    return ["Mk%05d" % m for m in range(M)]


def tag_names(M, i0, i1, T):
    """Tag names for the T = 2 M columns: marker m's alleles at columns i0[m] and i1[m]."""
    names = [None] * T
    for m in range(M):
        names[i0[m]] = "Mk%05d_0" % m
        names[i1[m]] = "Mk%05d_1" % m
    assert None not in names
    return names


def first_seen(i0, i1):
    """The markers in the order extractMarkers meets them: by their first column."""
    return sorted(range(len(i0)), key=lambda m: min(i0[m], i1[m]))


def reordered(ref, order):
    """The brute force's answer with its markers in another order."""
    return dict(calls=[[row[m] for m in order] for row in ref["calls"]],
                stats={k: [v[m] for m in order] for k, v in ref["stats"].items()},
                mask=[ref["mask"][m] for m in order], passed=ref["passed"])


def adjacent(M):
    """Columns as census_markers lays them out: marker m at columns 2 m and 2 m + 1."""
    return [2 * m for m in range(M)], [2 * m + 1 for m in range(M)], 2 * M


def scattered(rng, M, spare):
    """Columns under a random permutation, with `spare` unused columns in between."""
    T = 2 * M + spare
    cols = rng.sample(range(T), 2 * M)
    return cols[:M], cols[M:], T


def random_counts(rng, S, T):
    """Counts of every kind in every matrix: zeros, singletons, balanced and skewed cells, cells above 127 reads and a
    few near 2^32.  Columns differ in how often they are empty (one in six is never seen, one in six rarely), so that
    markers differ in call rate and allele frequency and the filters have something to drop."""
    def cell(p_zero):
        u = rng.random()
        if u < p_zero:
            return 0
        u = rng.random()
        if u < 0.35:
            return rng.randint(1, 3)
        if u < 0.80:
            return rng.randint(4, 60)
        if u < 0.96:
            return rng.randint(100, 5000)
        return rng.randint(U32 - 5, U32)
    p_zero = [rng.choice((1.0, 0.9, 0.3, 0.3, 0.3, 0.1)) for _ in range(T)]
    return [[cell(p_zero[c]) for c in range(T)] for _ in range(S)]


@functools.lru_cache(maxsize=None)
def grid_case(S, M, scatter=0):
    """(counts, i0, i1, T) of the grid tests, the same for every test of both files.  scatter 0: adjacent columns;
    1: the columns permuted; 2: permuted with 7 unused columns in between."""
    rng = random.Random(4100 + 1000 * S + M + 500 * scatter)
    i0, i1, T = scattered(rng, M, 7 if scatter == 2 else 0) if scatter else adjacent(M)
    return random_counts(rng, S, T), i0, i1, T


@functools.lru_cache(maxsize=None)
def grid_ref(S, M, scatter, rule, pset):
    counts, i0, i1, _ = grid_case(S, M, scatter)
    return ref_calls(counts, i0, i1, rule=rule, **PARAMS[pset])


@functools.lru_cache(maxsize=None)
def populated_case():
    """One case on which assert_populated holds under the second parameter set, likelihood rule (asserted here)."""
    counts, i0, i1, T = grid_case(65, 65)
    ref = ref_calls(counts, i0, i1, rule="likelihood", **PARAMS[1])
    assert_populated(ref, counts, i0, i1)
    return counts, i0, i1, T, ref


# cells at the edges of the scaling step: n = 127 is looked up as it is, n = 128 is scaled; the largest counts
EXTREME_CELLS = ((127, 0), (126, 1), (120, 7), (64, 63), (128, 0), (127, 1), (121, 7), (64, 64), (0, 128), (1, 127),
                 (U32, U32), (U32, 0), (U32, 1), (0, U32), (1, U32), (U32, U32 - 1), (1 << 31, 1 << 24))


def extreme_case():
    """One marker, one sample per cell of EXTREME_CELLS."""
    return [[a, b] for a, b in EXTREME_CELLS], [0], [1], 2


def filter_boundary_cases():
    """(counts, params, passes) with one marker over 8 samples under the presence rule, placed so that the left side of
    one inequality equals its right side (passes) or lies one unit below it (fails).  n0, n1, n2 are what the rows spell:
    (5, 0) -> 0, (5, 5) -> 1, (0, 5) -> 2, (0, 0) -> missing."""
    def rows(n0, n1, n2, missing):
        return [[5, 0]] * n0 + [[5, 5]] * n1 + [[0, 5]] * n2 + [[0, 0]] * missing
    cases = []
    # call rate: called / 8 against 0.75 -> 6 called is equality (6 * 10^6 = 750 000 * 8), 5 called is below
    cases.append((rows(3, 1, 2, 2), dict(min_call_rate=0.75), True))
    cases.append((rows(3, 1, 1, 3), dict(min_call_rate=0.75), False))
    # minor allele frequency: minor / (2 called) against 0.125 -> called 8, minor 2 is equality, minor 1 is below
    cases.append((rows(6, 2, 0, 0), dict(min_maf=0.125), True))
    cases.append((rows(7, 1, 0, 0), dict(min_maf=0.125), False))
    # ... and with allele 1 the commoner one: minor = 2 called - alt
    cases.append((rows(0, 2, 6, 0), dict(min_maf=0.125), True))
    cases.append((rows(0, 1, 7, 0), dict(min_maf=0.125), False))
    # heterozygosity: n1 / called against 0.5 -> 4 of 8 is equality, 5 of 8 is above
    cases.append((rows(2, 4, 2, 0), dict(max_het=0.5), True))
    cases.append((rows(2, 5, 1, 0), dict(max_het=0.5), False))
    cases.append((rows(3, 3, 2, 0), dict(max_het=0.5), True))
    # nobody called: passes only with min_call_rate = 0
    cases.append((rows(0, 0, 0, 8), dict(), True))
    cases.append((rows(0, 0, 0, 8), dict(min_call_rate=0.000001), False))
    return cases


def as_array(counts, T):
    import numpy as np
    return np.array(counts, dtype=np.uint32).reshape(len(counts), T)


def check_result(ref, calls, stats, mask, passed=None):
    """calls / stats / mask of the product (numpy) against the brute force, item by item."""
    assert calls.tolist() == ref["calls"]
    for k in STATS:
        assert [int(v) for v in stats[k]] == ref["stats"][k], k
    assert [bool(v) for v in mask] == ref["mask"]
    if passed is not None:
        assert int(passed) == ref["passed"]
