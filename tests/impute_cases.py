"""Shared by tests/test_impute.py and tests/test_impute_gpu.py: the imputation rule of DESIGN 4.17 stated by plain loops
in Python's integers, the choice of the neighbours restated with exact fractions, and the inputs of the tests.  It imports
nothing from the product.

calls is S x M, codes 0 / 1 / 2, any byte above 2 missing.  nbr[m] lists the markers that stand in for marker m (-1: no
entry).  For a target t missing at m and a donor d called at m, over the neighbours q at which both are called: ovl = how
many, dist = the sum of |calls[t][q] - calls[d][q]|; eligible iff ovl >= min_overlap; w = 32768 (2 ovl - dist) // ovl.
The first k eligible donors by (w descending, d ascending) vote with calls[d][m]; the cell becomes g iff V[g] is the only
maximum, the total is positive and V[g] * 10^6 >= ppm * total.  Only the input is ever read."""
import functools
import operator
from fractions import Fraction

import numpy as np

import ld_cases as lc

MAX_SAMPLES = 4096
MAX_NBR = 64
MAX_K = 32
STATS = ("missing", "imputed", "no_donor", "undecided")

# (ovl, dist) that a pair of codes adds, as ovl + 256 dist, by 4 a + b with the codes cut to 0 .. 3 (3 = missing)
_PAIR = [(1 + 256 * abs(a - b)) if a <= 2 and b <= 2 else 0 for a in range(4) for b in range(4)]


def ranked_ref(calls, nbr, min_overlap):
    """{(t, m): [(-w, d)] ascending} for every missing cell: its eligible donors in voting order.  The loop over the
    neighbours is a sum over a table of the 16 pairs of codes, so that the large shapes stay within seconds: nothing else
    differs from the sentence above.  It does not depend on k or the confidence, so the tests share it among them."""
    calls = [[int(c) for c in row] for row in calls]
    S, M = len(calls), len(nbr)
    assert min_overlap >= 1 and all(len(row) == M for row in calls)
    cells = {}
    for m in range(M):
        N = [int(q) for q in nbr[m] if q >= 0]
        assert all(int(q) >= -1 for q in nbr[m]) and all(0 <= q < M and q != m for q in N) and len(set(N)) == len(N)
        over = [[min(calls[s][q], 3) for q in N] for s in range(S)]           # the sample's codes at the neighbours
        donors = [d for d in range(S) if calls[d][m] <= 2]
        for t in range(S):
            if calls[t][m] <= 2:
                continue
            mine = [4 * c for c in over[t]]
            ranked = []
            for d in donors:
                acc = sum(map(_PAIR.__getitem__, map(operator.add, mine, over[d])))
                ovl, dist = acc & 255, acc >> 8
                if ovl >= min_overlap:
                    ranked.append((-(32768 * (2 * ovl - dist) // ovl), d))
            ranked.sort()
            cells[t, m] = ranked
    return cells


def vote_ref(calls, M, cells, k, ppm):
    """(filled matrix as lists, stats as M rows of [missing, imputed, no_donor, undecided]) from ranked_ref's cells."""
    assert k >= 1 and 0 <= ppm <= 10 ** 6
    out = [[int(c) for c in row] for row in calls]
    stats = [[0, 0, 0, 0] for _ in range(M)]
    for (t, m), ranked in cells.items():
        stats[m][0] += 1
        V = [0, 0, 0]
        for nw, d in ranked[:k]:
            V[int(calls[d][m])] -= nw
        total, top = sum(V), max(V)
        if not ranked:
            stats[m][2] += 1
        elif total > 0 and V.count(top) == 1 and top * 10 ** 6 >= ppm * total:
            out[t][m] = V.index(top)
            stats[m][1] += 1
        else:
            stats[m][3] += 1
    return out, stats


def impute_ref(calls, nbr, k, min_overlap, ppm):
    """The rule: (filled matrix as lists, stats as M rows of [missing, imputed, no_donor, undecided])."""
    calls = [[int(c) for c in row] for row in calls]
    return vote_ref(calls, len(nbr), ranked_ref(calls, nbr, min_overlap), k, ppm)


def weights_ref(calls, nbr, m, t):
    """[(w, d, ovl, dist)] of every donor of the cell (t, m) with ovl > 0, by (w descending, d ascending): for the
    tests that plant a value."""
    N = [q for q in nbr[m] if q >= 0]
    found = []
    for d in range(len(calls)):
        if d != t and calls[d][m] <= 2:
            both = [q for q in N if calls[t][q] <= 2 and calls[d][q] <= 2]
            ovl, dist = len(both), sum(abs(int(calls[t][q]) - int(calls[d][q])) for q in both)
            if ovl:
                found.append((32768 * (2 * ovl - dist) // ovl, d, ovl, dist))
    return sorted(found, key=lambda f: (-f[0], f[1]))


def check(ref, calls, stats):
    """The product's filled matrix and statistics (numpy) against impute_ref's pair."""
    assert calls.dtype == np.uint8 and calls.tolist() == ref[0]
    assert np.asarray(stats).tolist() == ref[1]


def neighbours_ref(edges, M, l):
    """The neighbour table from edges (i, j, shared, cov, var_i, var_j): row m = the markers joined to m by (r^2
    descending, other marker ascending) with r^2 an exact fraction, the first l, then -1.  Asserts that the order by the
    correctly rounded float64 quotient is the same: no two of a marker's edges are closer than a double tells apart."""
    joined = [[] for _ in range(M)]
    for e in edges:
        i, j, cov, var_i, var_j = int(e[0]), int(e[1]), int(e[3]), int(e[4]), int(e[5])
        r2 = Fraction(cov * cov, var_i * var_j)
        joined[i].append((-r2, j))
        joined[j].append((-r2, i))
    table = []
    for m in range(M):
        exact = sorted(joined[m])
        assert [o for _, o in exact] == [o for _, o in sorted(joined[m], key=lambda x: (float(x[0]), x[1]))], m
        row = [o for _, o in exact[:l]]
        table.append(row + [-1] * (l - len(row)))
    return table


# ---- inputs
GRID_S = (1, 2, 63, 64, 65, 129, 300)
GRID_L = (1, 31, 32, 33, 63, 64)
GRID_K = (1, 3, 32)
GRID_PPM = 600000


def grid_overlap(L):
    return 1 if L == 1 else 4


def grid_calls(S, L):
    return lc.structured_calls(S, L + 3)           # M = L + 3: odd or even, rows at odd addresses for every other L


@functools.lru_cache(maxsize=None)
def grid_nbr(L, seed=0):
    """int32 [L + 3, L]: row m is a random choice of L of the L + 2 other markers (below and above m), with -1 holes at
    the front (m % 4 == 0), in the middle (1) and at the end (2); every fourth row is full."""
    M = L + 3
    rng = np.random.default_rng(7700 + 17 * L + 100003 * seed)
    nbr = np.empty((M, L), dtype=np.int32)
    for m in range(M):
        others = np.array([q for q in range(M) if q != m])
        row = rng.permutation(others)[:L]
        holes = max(1, L // 5)
        if m % 4 == 0:
            row[:holes] = -1
        elif m % 4 == 1:
            row[L // 2:L // 2 + holes] = -1
        elif m % 4 == 2:
            row[L - holes:] = -1
        nbr[m] = row
    assert (nbr[:, 0] == -1).any() and (nbr[:, -1] == -1).any()
    if L > 1:
        both = [bool(((nbr[m] >= 0) & (nbr[m] < m)).any() and (nbr[m] > m).any()) for m in range(M)]
        assert sum(both) >= M // 2                 # most rows point below and above their own marker
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=None)
def grid_ranked(S, L):
    return ranked_ref(grid_calls(S, L).tolist(), grid_nbr(L).tolist(), grid_overlap(L))


def grid_ref(S, L, k):
    """impute_ref of the grid's case: the donors are ranked once per (S, L), the vote taken per k."""
    return vote_ref(grid_calls(S, L).tolist(), L + 3, grid_ranked(S, L), k, GRID_PPM)


def assert_grid_populated(totals):
    """Over the whole grid every column of the statistics counted something: a kernel that does nothing cannot pass."""
    assert all(t > 0 for t in totals), totals


@functools.lru_cache(maxsize=None)
def big_case():
    """(calls uint8 [4096, 6], nbr int32 [6, 64]) at the sample limit: two founder columns, 5 % of the cells redrawn,
    1 % missing with wild bytes; the last sample is missing at marker 0 and called everywhere else, so that the largest
    donor index and the largest target index both occur.  Rows of the table hold the five other markers among 59 holes."""
    S, M, L = MAX_SAMPLES, 6, MAX_NBR
    rng = np.random.default_rng(4096)
    founders = rng.integers(0, 3, size=(S, 2), dtype=np.uint8)
    C = founders[:, rng.integers(0, 2, size=M)].copy()
    noise = rng.random((S, M)) < 0.05
    C[noise] = rng.integers(0, 3, size=int(noise.sum()), dtype=np.uint8)
    gone = rng.random((S, M)) < 0.01
    C[gone] = rng.integers(3, 256, size=int(gone.sum()), dtype=np.uint8)
    C[S - 1] = founders[S - 1, 0]
    C[S - 1, 0] = 255
    nbr = np.full((M, L), -1, dtype=np.int32)
    for m in range(M):
        nbr[m, rng.permutation(L)[:M - 1]] = [q for q in range(M) if q != m]
    C.setflags(write=False)
    nbr.setflags(write=False)
    return C, nbr


def division_case():
    """(calls [3, 128], nbr [128, 64]): markers 0 .. 63 are a pool at which everybody is called; marker 64 + (ovl - 1) has
    the first ovl pool markers as neighbours.  Sample 0 is missing at every marker past the pool, sample 1 (class 0 there)
    differs from it by 1 at pool marker 0 and sample 2 (class 1) by 2: weights 32768 (2 ovl - 1) // ovl and
    32768 (2 ovl - 2) // ovl, the first not an integer quotient for every ovl that is no power of two."""
    calls = np.zeros((3, 128), dtype=np.uint8)
    calls[1, 0], calls[2, 0] = 1, 2
    calls[0, 64:], calls[1, 64:], calls[2, 64:] = 3, 0, 1
    nbr = np.full((128, 64), -1, dtype=np.int32)
    for ovl in range(1, 65):
        nbr[63 + ovl, :ovl] = np.arange(ovl)
    return calls, nbr


def forced_case(seed=0):
    """(truth uint8 [64, 24], hidden flat indices, nbr): every marker is a copy of one of two founder columns over 64
    samples, no noise, nothing missing; a marker's neighbours are its exact copies.  The founders are built so that every
    sample has a twin with the same two founder values: whatever cell is hidden, a donor with dist = 0 and full overlap
    exists (asserted by the test from the data)."""
    S, M = 64, 24
    rng = np.random.default_rng(640 + seed)
    half = rng.integers(0, 3, size=(S // 2, 2), dtype=np.uint8)
    founders = np.concatenate([half, half])        # sample s and s + 32 are twins
    which = np.arange(M) % 2
    truth = founders[:, which].copy()
    nbr = np.full((M, M // 2 - 1), -1, dtype=np.int32)
    for m in range(M):
        nbr[m] = [q for q in range(M) if q != m and which[q] == which[m]]
    # hide one cell per sample pair at most, so that a hidden cell's twin is still called at the marker and its copies
    hidden = np.sort(np.array([s * M + int(rng.integers(0, M)) for s in range(S // 2)]))
    return truth, hidden, nbr
