"""Shared by tests/test_linkage.py and tests/test_linkage_gpu.py: the linkage rule of DESIGN 4.24 stated by plain loops
over Python's integers (the table by decimal), the groups, the greedy chain and the writers' bytes restated plainly, and
the inputs of the tests.  It imports nothing from the product.

Only the offspring rows enter a count.  A participating marker has classes (A, B) by its cls code 0 = (0, 1), 1 = (2, 1),
2 = (0, 2); a cell is x = +1 for A, -1 for B, 0 otherwise.  For markers i < j: N = sum x_i^2 x_j^2, D = sum x_i x_j,
rec = (N - |D|) / 2, phase = (D < 0), lod16 = 65536 N + f[rec] + f[N - rec] - f[N], f[k] = round(65536 k log2 k).  An
edge iff N >= min_shared, rec 10^6 <= max_rf_ppm N and lod16 >= min_lod16."""
import decimal
import functools
import math

import numpy as np

MAX_SAMPLES = 16384
MAX_MARKERS = 1 << 20
EDGE = [("i", "<u4"), ("j", "<u4"), ("n", "<u4"), ("rec_phase", "<u4"), ("lod16", "<i8")]
NO_PART = 255
LOD_MIN = -(1 << 63)
CLASSES = ((0, 1), (2, 1), (0, 2))
REASONS = ("", "parents", "masked", "few", "distorted", "other")
OFF = dict(max_rf_ppm=500000, min_lod16=LOD_MIN, min_shared=0)         # every pair is an edge
REAL = dict(max_rf_ppm=250000, min_lod16=3 * 217706, min_shared=8)


# ---- the table
def table_entry(k, prec=50):
    """round(65536 k log2 k) at `prec` digits."""
    if k == 0:
        return 0
    with decimal.localcontext() as ctx:
        ctx.prec = prec
        v = decimal.Decimal(65536) * k * decimal.Decimal(k).ln() / decimal.Decimal(2).ln()
        return int(v.quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_EVEN))


@functools.lru_cache(maxsize=None)
def table(n):
    return tuple(table_entry(k) for k in range(n + 1))


def min_lod16(text):
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        v = decimal.Decimal(text) * 65536 * decimal.Decimal(10).ln() / decimal.Decimal(2).ln()
        return int(v.to_integral_value(rounding=decimal.ROUND_CEILING))


# ---- steps 1 and 2 by loops
def counts_ref(calls, rows):
    """[M][4]: c0, c1, c2, cmiss over the offspring rows."""
    M = len(calls[0]) if len(calls) else 0
    out = [[0, 0, 0, 0] for _ in range(M)]
    for r in rows:
        for m in range(M):
            out[m][min(int(calls[r][m]), 3)] += 1
    return out


def classes_ref(cross, counts, p1=None, p2=None):
    """([map_of], [cls]) per marker."""
    map_of, cls = [], []
    for m, c in enumerate(counts):
        if cross == "dh":
            map_of.append(1), cls.append(2)
        elif cross == "bc":
            map_of.append(1), cls.append(0 if c[0] >= c[2] else 1)
        else:
            a, b = int(p1[m]), int(p2[m])
            if a == 1 and b in (0, 2):
                map_of.append(1), cls.append(0 if b == 0 else 1)
            elif b == 1 and a in (0, 2):
                map_of.append(2), cls.append(0 if a == 0 else 1)
            else:
                map_of.append(0), cls.append(NO_PART)
    return map_of, cls


def segregation_ref(counts, cls, min_shared, max_chi2_milli, max_other_ppm):
    """[(a, b, o, verdict)] per marker: verdict an index into REASONS."""
    out = []
    for c, k in zip(counts, cls):
        if k == NO_PART:
            out.append((0, 0, 0, 1))
            continue
        a, b = c[CLASSES[k][0]], c[CLASSES[k][1]]
        o = c[0] + c[1] + c[2] - a - b
        if a + b < min_shared:
            v = 3
        elif (a - b) ** 2 * 1000 > max_chi2_milli * (a + b):
            v = 4
        elif o * 10 ** 6 > max_other_ppm * (a + b + o):
            v = 5
        else:
            v = 0
        out.append((a, b, o, v))
    return out


def x_columns(calls, rows, cls):
    """{marker: [x over the offspring]} of the participating markers."""
    out = {}
    for m, k in enumerate(cls):
        if k != NO_PART:
            a, b = CLASSES[k]
            out[m] = [1 if int(calls[r][m]) == a else -1 if int(calls[r][m]) == b else 0 for r in rows]
    return out


def pair_sums(calls, rows, cls):
    """{(i, j): (N, D)} for every pair of participating markers i < j, offspring by offspring in plain ints."""
    xs = x_columns(calls, rows, cls)
    part = sorted(xs)
    out = {}
    for a, i in enumerate(part):
        for j in part[a + 1:]:
            n = d = 0
            for x, y in zip(xs[i], xs[j]):
                n += x * x * y * y
                d += x * y
            out[i, j] = (n, d)
    return out


def decide(n, d, f, max_rf_ppm, min_lod16, min_shared):
    """(is an edge, rec, phase, lod16) of one pair."""
    assert (n - d) % 2 == 0
    c, r = (n + d) // 2, (n - d) // 2
    rec = min(c, r)
    lod16 = 65536 * n + f[rec] + f[n - rec] - f[n]
    return n >= min_shared and rec * 10 ** 6 <= max_rf_ppm * n and lod16 >= min_lod16, rec, 0 if d >= 0 else 1, lod16


def from_sums(sums, M, informative, R, max_rf_ppm, min_lod16, min_shared):
    """dict(edges = [(i, j, n, rec | phase << 31, lod16)] ascending, degree [M], informative [M])."""
    f = table(R)
    edges, degree = [], [0] * M
    for (i, j) in sorted(sums):
        n, d = sums[i, j]
        e, rec, phase, lod16 = decide(n, d, f, max_rf_ppm, min_lod16, min_shared)
        if e:
            edges.append((i, j, n, rec | phase << 31, lod16))
            degree[i] += 1
            degree[j] += 1
    return dict(edges=edges, degree=degree, informative=list(informative))


def informative_ref(calls, rows, cls):
    xs = x_columns(calls, rows, cls)
    return [sum(abs(x) for x in xs[m]) if m in xs else 0 for m in range(len(cls))]


def pairs_ref(calls, rows, cls, max_rf_ppm=500000, min_lod16=LOD_MIN, min_shared=0):
    calls = [[int(c) for c in row] for row in calls]
    rows, cls = [int(r) for r in rows], [int(k) for k in cls]
    return from_sums(pair_sums(calls, rows, cls), len(cls), informative_ref(calls, rows, cls), len(rows), max_rf_ppm, min_lod16,
                     min_shared)


def check_arrays(ref, edges, n, degree, informative):
    assert edges.dtype == np.dtype(EDGE) and n == len(ref["edges"])
    assert edges.tolist() == [tuple(e) for e in ref["edges"]]
    assert [int(x) for x in degree] == ref["degree"]
    assert [int(x) for x in informative] == ref["informative"]


# ---- step 3, restated plainly
def groups_ref(M, part, edges, min_group):
    nbrs = {m: set() for m in range(M)}
    for e in edges:
        nbrs[e[0]].add(e[1])
        nbrs[e[1]].add(e[0])
    comp, seen = [], set()
    for m in range(M):
        if part[m] and m not in seen:
            todo, mine = [m], set()
            while todo:
                k = todo.pop()
                if k not in mine:
                    mine.add(k)
                    todo.extend(nbrs[k])
            seen |= mine
            comp.append(sorted(mine))
    group, g = [0] * M, 0
    for mine in comp:                              # in the order of their smallest marker
        if len(mine) >= min_group:
            g += 1
            for k in mine:
                group[k] = g
    return group


def order_ref(members, pairs, min_shared):
    """The greedy chain.  pairs: {(i, j): (n, rec, phase)} of the members' pairs with n >= 1.  Returns (order, positions,
    phases)."""
    def get(u, v):
        return pairs.get((min(u, v), max(u, v)), (0, 0, 0))

    def rf(u, v):
        n, rec, _ = get(u, v)
        return rec * 10 ** 6 // n if n >= max(1, min_shared) else 500000

    members = sorted(members)
    if len(members) == 1:
        chain = list(members)
    else:
        _, i, j = min((rf(i, j), i, j) for a, i in enumerate(members) for j in members[a + 1:])
        chain, free = [i, j], [m for m in members if m not in (i, j)]
        while free:
            _, u, right = min((rf(e, u), u, right) for u in free for right, e in ((0, chain[0]), (1, chain[-1])))
            if right:
                chain.append(u)
            else:
                chain.insert(0, u)
            free.remove(u)
        if chain[0] > chain[-1]:
            chain.reverse()
    positions, phases = [0.0], [0]
    for u, v in zip(chain, chain[1:]):
        n, rec, ph = get(u, v)
        r = min(rec / n, 0.499) if n else 0.499
        positions.append(positions[-1] + 25.0 * math.log((1.0 + 2.0 * r) / (1.0 - 2.0 * r)))
        phases.append(phases[-1] ^ ph)
    return chain, positions, phases


def map_ref(calls, cross, parents=None, offspring=None, mask=None, min_lod="3", max_rf_ppm=250000, min_shared=50, max_chi2_milli=6635,
            max_other_ppm=50000, min_group=3, max_order=4096):
    """The whole of linkage_map by the loops above: dict(counts, map_of, cls, seg, maps = [dict(number, cls, ref, groups,
    order, positions, phases)], warnings)."""
    calls = [[int(c) for c in row] for row in calls]
    S, M = len(calls), len(calls[0]) if calls else 0
    rows = [s for s in range(S) if not parents or s not in parents] if offspring is None else list(offspring)
    counts = counts_ref(calls, rows)
    map_of, cls = classes_ref(cross, counts, *([calls[p] for p in parents] if cross == "cp" else []))
    seg = segregation_ref(counts, cls, min_shared, max_chi2_milli, max_other_ppm)
    seg = [(a, b, o, 2 if v != 1 and mask is not None and not mask[m] else v) for m, (a, b, o, v) in enumerate(seg)]
    lod16 = min_lod16(min_lod)
    maps, warnings = [], []
    for number in ((1, 2) if cross == "cp" else (1,)):
        taking = [map_of[m] == number and seg[m][3] == 0 for m in range(M)]
        map_cls = [cls[m] if taking[m] else NO_PART for m in range(M)]
        sums = pair_sums(calls, rows, map_cls)
        ref = from_sums(sums, M, informative_ref(calls, rows, map_cls), len(rows), max_rf_ppm, lod16, min_shared)
        groups = groups_ref(M, taking, ref["edges"], min_group)
        order, positions, phases = {}, {}, {}
        for g in range(1, max(groups) + 1 if groups else 1):
            members = [m for m in range(M) if groups[m] == g]
            if len(members) > max_order:
                warnings.append("map {} group {}: {} markers, more than --max-order {}: written unordered".format(
                    number, g, len(members), max_order))
                order[g], positions[g], phases[g] = members, None, None
                continue
            f = table(len(rows))
            pairs = {}
            for a, i in enumerate(members):
                for j in members[a + 1:]:
                    n, d = sums[i, j]
                    if n >= 1:
                        _, rec, ph, _ = decide(n, d, f, 500000, LOD_MIN, 1)
                        pairs[i, j] = (n, rec, ph)
            order[g], positions[g], phases[g] = order_ref(members, pairs, min_shared)
        maps.append(dict(number=number, cls=map_cls, ref=ref, groups=groups, order=order, positions=positions, phases=phases))
    return dict(counts=counts, map_of=map_of, cls=cls, seg=seg, maps=maps, warnings=warnings, rows=rows)


def check_result(ref, got):
    """A LinkageResult against map_ref's dictionary."""
    assert got.counts.tolist() == ref["counts"] and got.offspring == ref["rows"]
    assert got.map_of.tolist() == ref["map_of"] and got.cls.tolist() == ref["cls"]
    assert list(zip(got.a.tolist(), got.b.tolist(), got.o.tolist(), got.verdict.tolist())) == ref["seg"]
    assert got.warnings == ref["warnings"] and len(got.maps) == len(ref["maps"])
    for lm, want in zip(got.maps, ref["maps"]):
        assert lm.number == want["number"] and lm.cls.tolist() == want["cls"]
        check_arrays(want["ref"], lm.edges, len(lm.edges), lm.degree, lm.informative)
        assert lm.groups.tolist() == want["groups"]
        assert lm.order == want["order"] and lm.positions == want["positions"] and lm.phases == want["phases"]


# ---- the writers' bytes
def _csv(lines):
    return ("\r\n".join(lines) + "\r\n").encode("ascii")


def pairs_csv(markers, ref):
    lines = ["map,marker_i,marker_j,n,rec,rf,phase,lod16,lod"]
    for mp in ref["maps"]:
        for i, j, n, rp, lod16 in mp["ref"]["edges"]:
            rec = rp & 0x7fffffff
            lines.append(",".join([str(mp["number"]), markers[i], markers[j], str(n), str(rec), format(rec / n if n else 0.0, ".6f"),
                                   "R" if rp >> 31 else "C", str(lod16), format(lod16 / (65536 * math.log2(10)), ".3f")]))
    return _csv(lines)


def map_csv(markers, ref):
    lines = ["map,group,order,marker,position_cM,phase"]
    for mp in ref["maps"]:
        for g in sorted(mp["order"]):
            for k, m in enumerate(mp["order"][g]):
                if mp["positions"][g] is None:
                    lines.append(",".join([str(mp["number"]), str(g), "", markers[m], "", ""]))
                else:
                    lines.append(",".join([str(mp["number"]), str(g), str(k + 1), markers[m], format(mp["positions"][g][k], ".3f"),
                                           str(mp["phases"][g][k])]))
    return _csv(lines)


def stats_csv(markers, ref):
    lines = ["marker,c0,c1,c2,missing,map,class_a,class_b,a,b,other,informative,degree,group,dropped"]
    by_map = {mp["number"]: mp for mp in ref["maps"]}
    for m, name in enumerate(markers):
        a, b, o, v = ref["seg"][m]
        row = [name] + [str(x) for x in ref["counts"][m]] + [str(ref["map_of"][m])]
        row += [str(x) for x in CLASSES[ref["cls"][m]] + (a, b, o)] if v != 1 else [""] * 5
        if v == 0:
            mp = by_map[ref["map_of"][m]]
            row += [str(mp["ref"]["informative"][m]), str(mp["ref"]["degree"][m]), str(mp["groups"][m])]
        else:
            row += [""] * 3
        lines.append(",".join(row + [REASONS[v]]))
    return _csv(lines)


def calls_csv(samples, markers, calls):
    """The bytes of writeGenoCalls' layout: an empty first header cell, the markers; a row per sample, blank = missing."""
    lines = [",".join([""] + list(markers))]
    for name, row in zip(samples, calls):
        lines.append(",".join([name] + [str(int(c)) if int(c) <= 2 else "" for c in row]))
    return _csv(lines)


def marker_names(M):
    return ["Lk%05d" % m for m in range(M)]


def sample_names(S):
    return ["pl%04d" % s for s in range(S)]


# ---- inputs
@functools.lru_cache(maxsize=None)
def structured_calls(S, M, wild=True, seed=0):
    """A read-only uint8 [S, M] matrix with linkage in it: 6 founder columns of random 0 / 1 / 2, every marker a copy of a
    random founder or its mirror image (2 - x: repulsion), 8 % of the cells redrawn and 8 % missing -- wild: random
    bytes 3 .. 255, else 3."""
    rng = np.random.default_rng(7700 + 131 * S + M + 100003 * seed)
    founders = rng.integers(0, 3, size=(S, 6), dtype=np.uint8)
    C = founders[:, rng.integers(0, 6, size=M)].copy()
    flip = rng.random(M) < 0.4
    C[:, flip] = 2 - C[:, flip]
    noise = rng.random((S, M)) < 0.08
    C[noise] = rng.integers(0, 3, size=int(noise.sum()), dtype=np.uint8)
    gone = rng.random((S, M)) < 0.08
    C[gone] = rng.integers(3, 256, size=int(gone.sum()), dtype=np.uint8) if wild else 3
    C.setflags(write=False)
    return C


def grid_markers(Mp, holes):
    """The markers of a grid case with Mp participating ones: with holes, half as many again take no part."""
    return Mp + (Mp // 2 + 1 if holes else 0)


@functools.lru_cache(maxsize=None)
def mixed_cls(Mp, holes, seed=0):
    """cls of grid_markers(Mp, holes) markers: all three codes mixed over exactly Mp of them, NO_PART for the rest."""
    rng = np.random.default_rng(5100 + Mp + 100003 * seed + holes)
    M = grid_markers(Mp, holes)
    cls = np.full(M, NO_PART, dtype=np.uint8)
    cls[np.sort(rng.choice(M, size=Mp, replace=False))] = rng.integers(0, 3, size=Mp, dtype=np.uint8)
    cls.setflags(write=False)
    return cls


@functools.lru_cache(maxsize=None)
def row_subset(S, kind):
    """None, a permuted subset, or a subset in order that skips the first and last row."""
    if kind == "all":
        return None
    rng = np.random.default_rng(3300 + S)
    if kind == "permuted":
        return tuple(int(r) for r in rng.permutation(S)[:max(1, (2 * S + 2) // 3)])
    return tuple(range(1, S - 1)) if S > 2 else (0,)


def rows_around(R, kind):
    """(S, rows) with exactly R offspring rows: "all" -- None, every row; "permuted" -- R of R + 3 rows in a random order;
    "inner" -- rows 1 .. R of R + 2, skipping the first and the last."""
    if kind == "all":
        return R, None
    if kind == "inner":
        return R + 2, list(range(1, R + 1))
    return R + 3, [int(r) for r in np.random.default_rng(3400 + R).permutation(R + 3)[:R]]


def sums_numpy(calls, rows, cls):
    """pair_sums for shapes the loop cannot reach: int64 products of the planes (exact), the same dictionary.
    tests/test_linkage.py checks it against the loop."""
    C = np.asarray(calls, dtype=np.uint8)[np.asarray(rows, dtype=np.int64)]
    part = [m for m in range(C.shape[1]) if cls[m] != NO_PART]
    ab = np.array([CLASSES[cls[m]] for m in part], dtype=np.uint8).reshape(len(part), 2)
    X = (C[:, part] == ab[None, :, 0]).astype(np.int64) - (C[:, part] == ab[None, :, 1]).astype(np.int64)
    V = X * X
    n, d = V.T @ V, X.T @ X
    return {(i, j): (int(n[a, b]), int(d[a, b])) for a, i in enumerate(part) for b, j in enumerate(part) if a < b}


def two_markers(n, rec, repulsion=False, extra=0):
    """A read-only uint8 [n + extra, 2] matrix of 0 / 2 calls (cls 2) with N = n informative offspring at both markers and
    rec recombinants among them, in coupling or repulsion; the extra rows are missing at the second marker."""
    C = np.zeros((n + extra, 2), dtype=np.uint8)
    C[::2, 0] = 2
    C[:, 1] = C[:, 0]
    C[:rec, 1] = 2 - C[:rec, 1]
    if repulsion:
        C[:, 1] = 2 - C[:, 1]
    C[n:, 1] = 3
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def grid_sums(S, Mp, holes, kind="all"):
    """(pair_sums, informative, R) of structured_calls(S, grid_markers(Mp, holes)) under mixed_cls(Mp, holes) over
    row_subset(S, kind): looped once, shared."""
    calls = structured_calls(S, grid_markers(Mp, holes)).tolist()
    cls = mixed_cls(Mp, holes).tolist()
    rows = row_subset(S, kind)
    rows = list(range(S)) if rows is None else list(rows)
    return pair_sums(calls, rows, cls), tuple(informative_ref(calls, rows, cls)), len(rows)


def grid_ref(S, Mp, holes, thresholds, kind="all"):
    sums, informative, R = grid_sums(S, Mp, holes, kind)
    return from_sums(sums, grid_markers(Mp, holes), informative, R, **thresholds)


@functools.lru_cache(maxsize=None)
def simulated_cross(cross="cp", offspring=200, ngroups=3, per_group=40, step=0.04, missing=0.0, distorted=0, hethet=0, seed=3):
    """A simulated cross.  Returns dict(calls uint8 [S, M] read-only, parents (row indices or None), truth = [(map, [the
    markers of a group in their true order], [their founder phases])], bad = the distorted and het x het markers).

    cp: rows 0 and 1 are the parents.  Every marker is heterozygous in one parent (alternating by group, so both maps get
    groups) with a random founder phase, homozygous 0 or 2 in the other.  A gamete of the heterozygous parent walks
    along the group and switches strand with probability `step` between neighbours; the offspring is heterozygous where
    the strand carries the allele the other parent lacks.  dh: 0 / 2 by the strand and the phase; bc: 0 / 1 (or 2 / 1).
    The true order is scattered over the columns by a fixed permutation; distorted markers lose most of one class,
    het x het markers segregate 1 : 2 : 1."""
    rng = np.random.default_rng(9100 + seed)
    M = ngroups * per_group + distorted + hethet
    first = 2 if cross == "cp" else 0
    S = offspring + first
    calls = np.zeros((S, M), dtype=np.uint8)
    where = rng.permutation(M)
    truth, col = [], 0
    for g in range(ngroups):
        strand = rng.integers(0, 2, size=offspring)
        cols, phases = [], []
        number = 1 + g % 2 if cross == "cp" else 1
        for k in range(per_group):
            if k:
                strand = strand ^ (rng.random(offspring) < step)
            m, ph = int(where[col]), int(rng.integers(0, 2))
            col += 1
            allele = strand ^ ph                   # 1: the offspring got the allele that makes it the B class
            if cross == "dh":
                calls[:, m] = np.where(allele, 2, 0)
            else:
                hom = int(rng.integers(0, 2)) * 2  # the homozygous side: class A
                calls[first:, m] = np.where(allele, 1, hom)
                if cross == "cp":
                    calls[number - 1, m], calls[2 - number, m] = 1, hom
            cols.append(m)
            phases.append(ph)
        truth.append((number, cols, phases))
    bad = []
    for k in range(distorted):
        m = int(where[col])
        col += 1
        calls[first:, m] = np.where(rng.random(offspring) < 0.2, 1, 0) if cross != "dh" else np.where(rng.random(offspring) < 0.2, 2, 0)
        if cross == "cp":
            calls[0, m], calls[1, m] = 1, 0
        bad.append(m)
    for k in range(hethet):
        m = int(where[col])
        col += 1
        calls[first:, m] = rng.integers(0, 2, size=offspring) + rng.integers(0, 2, size=offspring)
        if cross == "cp":
            calls[0, m] = calls[1, m] = 1
        bad.append(m)
    if missing:
        gone = rng.random((S, M)) < missing
        gone[:first] = False
        calls[gone] = 3
    calls.setflags(write=False)
    return dict(calls=calls, parents=(0, 1) if cross == "cp" else None, truth=truth, bad=bad)
