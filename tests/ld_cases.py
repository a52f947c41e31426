"""Shared by tests/test_ld.py and tests/test_ld_gpu.py: the LD rule of DESIGN 4.16 stated by a plain triple loop in
Python's integers, the groups and the pruning restated plainly, the bytes the writers must write, and the inputs of the
tests.  It imports nothing from the product.

For two participating markers i < j, over the samples s at which both are called (a byte above 2 is missing), with
x = calls[s][i] and y = calls[s][j]: n, sx, sy, sxx, syy, sxy; cov = n sxy - sx sy, var_i = n sxx - sx^2,
var_j = n syy - sy^2.  The pair is an edge iff n >= min_shared, var_i > 0, var_j > 0 and
cov^2 * 10^6 >= min_r2_ppm * var_i * var_j.  Marker m takes part iff there is no mask or use[m] != 0."""
import functools

import numpy as np

MAX_SAMPLES = 16384
MAX_MARKERS = 1 << 20
EDGE = [("i", "<u4"), ("j", "<u4"), ("shared", "<u4"), ("cov", "<i4"), ("var_i", "<u4"), ("var_j", "<u4")]
# (min_shared, min_r2_ppm): everything, the defaults' neighbourhood, r^2 = 1 only
THRESHOLDS = ((0, 0), (1, 500000), (10, 800000), (5, 1000000))


def pair_sums(calls, use=None):
    """{(i, j): (n, sx, sy, sxx, syy, sxy)} for every pair of participating markers i < j, sample by sample in plain
    ints.  calls is a list of rows (or a small array)."""
    cols = [[int(c) for c in col] for col in zip(*calls)] if len(calls) else []
    part = [m for m in range(len(cols)) if use is None or use[m]]
    out = {}
    for a, i in enumerate(part):
        ci = cols[i]
        for j in part[a + 1:]:
            n = sx = sy = sxx = syy = sxy = 0
            for x, y in zip(ci, cols[j]):
                if x <= 2 and y <= 2:
                    n += 1
                    sx += x
                    sy += y
                    sxx += x * x
                    syy += y * y
                    sxy += x * y
            out[i, j] = (n, sx, sy, sxx, syy, sxy)
    return out


def moments(sums):
    """(n, cov, var_i, var_j) of one pair's sums."""
    n, sx, sy, sxx, syy, sxy = sums
    return n, n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy


def is_edge(sums, min_shared, ppm):
    """The edge test, Python's integers only."""
    n, cov, var_i, var_j = moments(sums)
    return n >= min_shared and var_i > 0 and var_j > 0 and cov * cov * 10 ** 6 >= ppm * var_i * var_j


def called_ref(calls, use=None):
    M = len(calls[0]) if len(calls) else (0 if use is None else len(use))
    return [sum(1 for row in calls if int(row[m]) <= 2) if use is None or use[m] else 0 for m in range(M)]


def from_sums(sums, M, called, min_shared, ppm):
    """dict(edges = [(i, j, n, cov, var_i, var_j)] ascending, degree [M], called [M]) from pair_sums' table."""
    edges, degree = [], [0] * M
    for (i, j) in sorted(sums):
        if is_edge(sums[i, j], min_shared, ppm):
            edges.append((i, j) + moments(sums[i, j]))
            degree[i] += 1
            degree[j] += 1
    return dict(edges=edges, degree=degree, called=list(called))


def ld_ref(calls, use=None, min_shared=0, ppm=0):
    calls = [[int(c) for c in row] for row in calls]
    M = len(calls[0]) if calls else (0 if use is None else len(use))
    return from_sums(pair_sums(calls, use), M, called_ref(calls, use), min_shared, ppm)


def sums_numpy(calls, use=None):
    """pair_sums for shapes the loop cannot reach: int64 products of the planes (exact), the same dictionary.
    tests/test_ld.py checks it against the loop."""
    C = np.asarray(calls, dtype=np.uint8)
    part = [m for m in range(C.shape[1]) if use is None or use[m]]
    ok = (C[:, part] <= 2).astype(np.int64)
    X = np.where(ok == 1, C[:, part], 0).astype(np.int64)
    Q = X * X
    n, sx, sy, sxx, syy, sxy = ok.T @ ok, X.T @ ok, ok.T @ X, Q.T @ ok, ok.T @ Q, X.T @ X
    return {(i, j): tuple(int(t[a, b]) for t in (n, sx, sy, sxx, syy, sxy))
            for a, i in enumerate(part) for b, j in enumerate(part) if a < b}


def as_records(edges):
    return np.array([tuple(e) for e in edges], dtype=EDGE)


def check_arrays(ref, edges, n, degree, called):
    """The product's edge array, count, degrees and called counts against from_sums' dictionary."""
    assert edges.dtype == np.dtype(EDGE) and n == len(ref["edges"])
    assert edges.tolist() == [tuple(e) for e in ref["edges"]]
    assert [int(x) for x in degree] == ref["degree"]
    assert [int(x) for x in called] == ref["called"]


# ---- groups and pruning, restated plainly
def groups_ref(M, mask, edges):
    """Connected components by repeated search: [M] group numbers from 1 in the order of the smallest marker, 0 for a
    marker that does not take part."""
    nbrs = {m: set() for m in range(M)}
    for e in edges:
        nbrs[e[0]].add(e[1])
        nbrs[e[1]].add(e[0])
    group, g = [0] * M, 0
    for m in range(M):
        if mask[m] and not group[m]:
            g += 1
            todo = [m]
            while todo:
                k = todo.pop()
                if not group[k]:
                    group[k] = g
                    todo.extend(nbrs[k])
    return group


def prune_ref(M, mask, edges, called):
    nbrs = {m: set() for m in range(M)}
    for e in edges:
        nbrs[e[0]].add(e[1])
        nbrs[e[1]].add(e[0])
    keep = [False] * M
    for m in sorted((m for m in range(M) if mask[m]), key=lambda m: (-called[m], m)):
        keep[m] = not any(keep[k] for k in nbrs[m])
    return keep


# ---- the writers' bytes
def r2_text(e):
    return format(e[3] * e[3] / (e[4] * e[5]), ".6f")


def pairs_csv(markers, edges):
    lines = ["marker_i,marker_j,shared,r2,phase"]
    for e in edges:
        lines.append(",".join([markers[e[0]], markers[e[1]], str(e[2]), r2_text(e), "+" if e[3] > 0 else "-" if e[3] < 0 else "0"]))
    return ("\r\n".join(lines) + "\r\n").encode("ascii")


def groups_csv(markers, mask, ref):
    M = len(markers)
    group = groups_ref(M, mask, ref["edges"])
    keep = prune_ref(M, mask, ref["edges"], ref["called"])
    lines = ["marker,group,group_size,degree,called,kept"]
    for m in range(M):
        if mask[m]:
            lines.append(",".join([markers[m], str(group[m]), str(group.count(group[m])), str(ref["degree"][m]),
                                   str(ref["called"][m]), "1" if keep[m] else "0"]))
    return ("\r\n".join(lines) + "\r\n").encode("ascii")


def keep_txt(markers, mask, ref):
    keep = prune_ref(len(markers), mask, ref["edges"], ref["called"])
    return "".join(name + "\n" for name, k in zip(markers, keep) if k).encode("ascii")


def marker_names(M):
    return ["Mk%05d" % m for m in range(M)]


# ---- inputs
@functools.lru_cache(maxsize=None)
def structured_calls(S, M, wild=True, seed=0):
    """A read-only uint8 [S, M] matrix with LD in it: 8 founder columns of random 0 / 1 / 2, every marker a copy of a
    random founder, 10 % of the cells redrawn from 0 .. 2 and 10 % missing -- wild: random bytes 3 .. 255, else 3.  The
    last marker is then made the first one over again, byte for byte (a tag that was made twice: r^2 = 1)."""
    rng = np.random.default_rng(6100 + 131 * S + M + 100003 * seed)
    founders = rng.integers(0, 3, size=(S, 8), dtype=np.uint8)
    C = founders[:, rng.integers(0, 8, size=M)].copy()
    noise = rng.random((S, M)) < 0.1
    C[noise] = rng.integers(0, 3, size=int(noise.sum()), dtype=np.uint8)
    gone = rng.random((S, M)) < 0.1
    C[gone] = rng.integers(3, 256, size=int(gone.sum()), dtype=np.uint8) if wild else 3
    C[:, M - 1] = C[:, 0]
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def flipped_calls(S, M):
    """structured_calls(S, M, wild=False) with the alleles of every third marker exchanged (2 - x): both phases occur."""
    C = np.array(structured_calls(S, M, wild=False))
    C[:, ::3] = np.where(C[:, ::3] <= 2, 2 - C[:, ::3], 3)
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def flipped_sums(S, M, masked):
    calls = flipped_calls(S, M).tolist()
    use = random_mask(M).tolist() if masked else None
    return pair_sums(calls, use), tuple(called_ref(calls, use))


def flipped_ref(S, M, masked, min_shared, ppm):
    sums, called = flipped_sums(S, M, masked)
    return from_sums(sums, M, called, min_shared, ppm)


@functools.lru_cache(maxsize=None)
def random_mask(M, seed=0):
    rng = np.random.default_rng(9300 + M + 100003 * seed)
    use = (rng.random(M) < 0.6).astype(np.uint8) * rng.integers(1, 256, size=M, dtype=np.uint8)    # any nonzero byte passes
    use.setflags(write=False)
    return use


@functools.lru_cache(maxsize=None)
def grid_sums(S, M, masked, wild=True):
    """(pair_sums, called) of structured_calls(S, M, wild) without or with random_mask(M): looped once, shared."""
    calls = structured_calls(S, M, wild).tolist()
    use = random_mask(M).tolist() if masked else None
    return pair_sums(calls, use), tuple(called_ref(calls, use))


def grid_ref(S, M, masked, min_shared, ppm, wild=True):
    sums, called = grid_sums(S, M, masked, wild)
    return from_sums(sums, M, called, min_shared, ppm)
