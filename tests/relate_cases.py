"""Shared by tests/test_relate.py and tests/test_relate_gpu.py: the joint table of sample pairs stated by
brute force, the quantities derived from it and the duplicate rule in Python's integers, and the inputs of the tests.
It imports nothing from the product.

joint[i][j][a][b] = the participating markers m with calls[i][m] == a and calls[j][m] == b, a and b in 0 .. 2; any byte
above 2 is missing; marker m takes part iff there is no mask or use[m] != 0."""
import functools
import random

import numpy as np

COLUMNS = ("shared", "ibs0", "ibs1", "ibs2", "hethet", "het_i", "het_j")
MAX_SAMPLES = 16384


def joint_brute(calls, use=None):
    """Plain ints, marker by marker: nested lists [S][S][3][3].  calls is a list of rows (or a small array)."""
    rows = [[int(c) for c in row] for row in calls]
    S = len(rows)
    M = len(rows[0]) if S else 0
    J = [[[[0] * 3 for _ in range(3)] for _ in range(S)] for _ in range(S)]
    for m in range(M):
        if use is not None and not use[m]:
            continue
        for i in range(S):
            a = rows[i][m]
            if a > 2:
                continue
            for j in range(S):
                b = rows[j][m]
                if b <= 2:
                    J[i][j][a][b] += 1
    return J


def joint_ref(calls, use=None):
    """numpy: (C == a) as float64 times (C == b) transposed, exact below 2^53.  uint32 [S, S, 3, 3]."""
    C = np.asarray(calls, dtype=np.uint8)
    S = C.shape[0]
    if use is not None:
        C = C[:, np.asarray(use) != 0]
    J = np.zeros((S, S, 3, 3), dtype=np.uint32)
    planes = [(C == a).astype(np.float64) for a in range(3)]
    for a in range(3):
        for b in range(3):
            J[:, :, a, b] = planes[a] @ planes[b].T
    return J


def derived(J):
    """dict of plain ints from one pair's 3 x 3 table."""
    J = [[int(x) for x in row] for row in J]
    shared = sum(sum(row) for row in J)
    ibs0 = J[0][2] + J[2][0]
    ibs2 = J[0][0] + J[1][1] + J[2][2]
    ibs1 = shared - ibs0 - ibs2
    return dict(shared=shared, ibs0=ibs0, ibs1=ibs1, ibs2=ibs2, hethet=J[1][1], het_i=J[1][0] + J[1][1] + J[1][2],
                het_j=J[0][1] + J[1][1] + J[2][1], dist=ibs1 + 2 * ibs0)


def ppm(x):
    return int(round(x * 1e6))


def is_duplicate(d, max_dist_ppm, min_shared):
    """The duplicate rule, integer products only."""
    return d["shared"] >= min_shared and d["dist"] * 10 ** 6 <= max_dist_ppm * 2 * d["shared"]


def distance_text(d):
    return "NA" if d["shared"] == 0 else format(d["dist"] / (2 * d["shared"]), ".6f")


def kinship_text(d):
    het = d["het_i"] + d["het_j"]
    return "NA" if het == 0 else format((d["hethet"] - 2 * d["ibs0"]) / het, ".6f")


def expected(calls, use=None, max_dist=0.02, min_shared=50):
    """dict(joint, pairs {(i, j): derived}, duplicates [(i, j), i < j]) from joint_ref."""
    J = joint_ref(calls, use)
    S = J.shape[0]
    pairs = {(i, j): derived(J[i, j].tolist()) for i in range(S) for j in range(S)}
    dups = [(i, j) for i in range(S) for j in range(i + 1, S) if is_duplicate(pairs[i, j], ppm(max_dist), min_shared)]
    return dict(joint=J, pairs=pairs, duplicates=dups)


def check_result(exp, result):
    """A RelationResult of the product against `expected`, item by item."""
    assert result.joint.dtype == np.uint32 and np.array_equal(result.joint, exp["joint"])
    S = exp["joint"].shape[0]
    for k in COLUMNS + ("dist",):
        got = getattr(result, k)
        assert got.shape == (S, S)
        assert got.tolist() == [[exp["pairs"][i, j][k] for j in range(S)] for i in range(S)], k
    for (i, j), d in exp["pairs"].items():
        x, k = float(result.distance[i, j]), float(result.kinship[i, j])
        assert ("NA" if x != x else format(x, ".6f")) == distance_text(d)
        assert ("NA" if k != k else format(k, ".6f")) == kinship_text(d)
    assert [tuple(p) for p in result.duplicates] == exp["duplicates"]


def pairs_csv(samples, exp):
    """The bytes writeRelations must write."""
    lines = ["sample_i,sample_j,shared,ibs0,ibs1,ibs2,hethet,het_i,het_j,distance,kinship,duplicate"]
    S = len(samples)
    for i in range(S):
        for j in range(i + 1, S):
            d = exp["pairs"][i, j]
            lines.append(",".join([samples[i], samples[j]] + [str(d[k]) for k in COLUMNS] +
                                  [distance_text(d), kinship_text(d), "1" if (i, j) in exp["duplicates"] else "0"]))
    return ("\r\n".join(lines) + "\r\n").encode("ascii")


def matrix_csv(samples, exp):
    """The bytes writeDistanceMatrix must write."""
    S = len(samples)
    lines = [",".join([""] + list(samples))]
    for i in range(S):
        lines.append(",".join([samples[i]] + [distance_text(exp["pairs"][i, j]) for j in range(S)]))
    return ("\r\n".join(lines) + "\r\n").encode("ascii")


def sample_names(S):
    return ["w%03d" % k for k in range(S)]


@functools.lru_cache(maxsize=None)
def random_calls(S, M, wild=True, seed=0):
    """A read-only uint8 [S, M] matrix of codes 0 .. 3, every sample with its own share of missing cells; wild: about one
    byte in 16 is drawn from 4 .. 255 instead (missing as well)."""
    rng = np.random.default_rng(7700 + 131 * S + M + 100003 * seed)
    p_missing = rng.choice([0.05, 0.2, 0.6], size=(S, 1))
    C = rng.integers(0, 3, size=(S, M), dtype=np.uint8)
    C[rng.random((S, M)) < p_missing] = 3
    if wild:
        w = rng.random((S, M)) < 1 / 16
        C[w] = rng.integers(4, 256, size=int(w.sum()), dtype=np.uint8)
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def random_mask(M, seed=0):
    rng = np.random.default_rng(9100 + M + 100003 * seed)
    use = (rng.random(M) < 0.6).astype(np.uint8) * rng.integers(1, 256, size=M, dtype=np.uint8)    # any nonzero byte passes
    use.setflags(write=False)
    return use


@functools.lru_cache(maxsize=None)
def grid_ref(S, M, masked, wild=True):
    """joint_ref of random_calls(S, M, wild) without or with random_mask(M): computed once, shared, read-only."""
    J = joint_ref(random_calls(S, M, wild), random_mask(M) if masked else None)
    J.setflags(write=False)
    return J


@functools.lru_cache(maxsize=None)
def populated_case():
    """(calls [8][400] as a read-only array, sample names, mask, expectation under the defaults 0.02 / 50) in which a
    flagged and an unflagged pair, a pair with shared == 0, a pair with ibs0 > 0 and a pair below min_shared that is
    close enough otherwise all occur (asserted here)."""
    rng = random.Random(415)
    M = 400
    base = [rng.choice((0, 0, 1, 2)) for _ in range(M)]
    other = [rng.choice((0, 1, 2, 2)) for _ in range(M)]
    rows = []
    rows.append(list(base))                                                    # 0: a plant
    rows.append([3 if rng.random() < 0.1 else c for c in base])                # 1: the same plant in another well
    noisy = list(base)
    for m in rng.sample(range(M), 3):                                          # 2: the same plant with 3 calls of 400 off by one
        noisy[m] = 1 if noisy[m] != 1 else 0
    rows.append(noisy)
    rows.append(list(other))                                                   # 3: another plant
    rows.append([c if m < 200 else 3 for m, c in enumerate(base)])             # 4: called in the first half only
    rows.append([c if m >= 200 else 3 for m, c in enumerate(other)])           # 5: called in the second half only
    rows.append([c if m < 30 else 3 for m, c in enumerate(base)])              # 6: the plant again, 30 markers only
    rows.append([3] * M)                                                       # 7: an empty well
    mask = [m % 10 != 9 for m in range(M)]
    calls = np.array(rows, dtype=np.uint8)
    calls.setflags(write=False)
    exp = expected(calls, mask)
    P, D = exp["pairs"], exp["duplicates"]
    assert (0, 1) in D and (0, 2) in D and (0, 3) not in D                     # flagged and unflagged
    assert P[4, 5]["shared"] == 0 and P[0, 7]["shared"] == 0                   # no marker in common
    assert P[0, 3]["ibs0"] > 0
    assert 0 < P[0, 6]["shared"] < 50 and P[0, 6]["dist"] == 0 and (0, 6) not in D     # identical, but on too few markers
    assert P[0, 2]["dist"] > 0
    return calls, sample_names(len(rows)), mask, exp
