"""Device side of Tag Manager: the glue between tagdigger_fun's Tag Manager functions and the kernels of csrc/tagset.hip
(include/tagdig.h: td_tagset_load, td_tagset_lookup, td_tagset_varsites).

  SortedTags   a tag set sorted on the device (K1 pack, K2 radix sort) in the order of sorted(zip(seqs, names)),
               kept resident for lookups (K3);
  walk_host    the host restatement of one lookupMarkerByTag walk, as the same four indices K3 returns;
  add_walk     the markers of one walk, added to a set in the reference's order (the set's iteration order is part
               of the output, so the order of insertion matters);
  varsites     compareTags' columns for many groups of tags at once (K4).

The device takes ACGT tags of at most 256 bases; `device_takes` says whether a call's tags qualify.  When they do not,
the caller runs its host restatement for the whole call.
"""
import numpy as np

MAX_LEN = 256
stage_ms = {}          # device ms of the last calls, by kernel (K1 .. K4), for tools/tag_manager_bench.py


def _note(name, ms):
    stage_ms[name] = stage_ms.get(name, 0.0) + ms


def device_takes(*seqlists):
    """True when every tag is ASCII ACGT and at most 256 bases long."""
    for seqs in seqlists:
        if any(len(s) > MAX_LEN for s in seqs):
            return False
        try:
            raw = "".join(seqs).encode("ascii")
        except UnicodeEncodeError:
            return False
        if raw.translate(None, b"ACGT"):
            return False
    return True


def pack(seqs):
    """(ASCII bytes of the tags end to end, uint64 offsets n + 1)."""
    lens = np.fromiter(map(len, seqs), dtype=np.uint64, count=len(seqs))
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    return "".join(seqs).encode("ascii"), offs


def name_order(names):
    """The tags sorted by name in code-point order (Python's str order), as indices."""
    if names and not any("\x00" in x for x in names):
        arr = np.array(names, dtype=str)           # numpy compares UCS4 code points; NUL-free names compare as str
        return np.argsort(arr, kind="stable").astype(np.uint32)
    return np.array(sorted(range(len(names)), key=names.__getitem__), dtype=np.uint32)


def marker_of(tagname):
    return tagname[:tagname.find('_')]


class SortedTags:
    """[names, seqs] sorted as sorted(zip(seqs, names)) by K2, and the sorted set resident for K3.  by_name=False
    keeps the given order among equal sequences (for a list that is sorted already)."""

    def __init__(self, eng, names, seqs, by_name=True):
        raw, offs = pack(seqs)
        self.set, perm, self.passes, ms = eng.tagset_load(raw, offs, name_order(names) if by_name else None)
        _note("K1", ms[0])
        _note("K2", ms[1])
        self.eng = eng
        p = perm.tolist()
        self.names = tuple(names[i] for i in p)
        self.seqs = tuple(seqs[i] for i in p)
        self.markers = [marker_of(x) for x in self.names]

    def walks(self, queries, allow_diff_lengths):
        """int32 [len(queries), 4]: f, a, b, c of every query's walk."""
        raw, offs = pack(queries)
        out, ms = self.eng.tagset_lookup(self.set, raw, offs, allow_diff_lengths)
        _note("K3", ms)
        return out

    def close(self):
        self.set.close()


def walk_host(S, q, allow_diff_lengths):
    """One query's walk through the sorted list S (lookupMarkerByTag, tagdigger_fun.py:1674-1706), step by step:
    (f, a, b, c) as K3 returns them."""
    import bisect
    n = len(S)
    i = bisect.bisect_left(S, q)
    f = -1
    if i < n and S[i] == q:
        f = i
    elif allow_diff_lengths:
        if i > 0 and q.startswith(S[i - 1]):
            f = i - 1
            i -= 1
            while i > 0 and S[i] == S[i - 1]:
                i -= 1
        if i < n and S[i].startswith(q):
            several = i + 1 < n and S[i] != S[i + 1] and S[i + 1].startswith(q)
            if not several:
                f = i
    if f < 0:
        return (-1, -1, -1, -1)
    a = i
    while i + 1 < n and (S[i] == S[i + 1] or (allow_diff_lengths and S[i + 1].startswith(q))):
        i += 1
    b = i
    while allow_diff_lengths and i > 0 and q.startswith(S[i - 1]):
        i -= 1
    return (f, a, b, i)


def add_walk(out, markers, walk):
    """Add the markers of one walk to the set `out` in the reference's order: f, a + 1 .. b, b - 1 down to c."""
    f, a, b, c = (int(x) for x in walk)
    if f < 0:
        return
    out.add(markers[f])
    for j in range(a + 1, b + 1):
        out.add(markers[j])
    for j in range(b - 1, c - 1, -1):
        out.add(markers[j])


def mask_columns(row):
    """The columns set in one group's 4 x 64-bit mask, ascending."""
    cols = []
    for w, word in enumerate(row):
        while word:
            low = word & -word
            cols.append(64 * w + low.bit_length() - 1)
            word ^= low
    return cols


def varsites(eng, groups, trim):
    """compareTags' columns for each group (a list of tag sequences), and per group whether a tag holds a byte
    outside ACGT (K4)."""
    flat = [s for g in groups for s in g]
    raw, offs = pack(flat)
    goff = np.zeros(len(groups) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, groups), dtype=np.uint64, count=len(groups)), out=goff[1:])
    idx = np.arange(len(flat), dtype=np.uint32)
    masks, bad, ms = eng.tagset_varsites(raw, offs, idx, goff, trim)
    _note("K4", ms)
    return [mask_columns(r) for r in masks.tolist()], bad.tolist()
