"""The case builders of tests/index_edges_cases.py without a GPU: they are deterministic and prefix-free, their reads are
what they claim to be, the shapes they promise follow from td_set_index's rules, and on every case three references
that share no code agree exactly -- the C oracle's trie, the Python oracle's trie and the rule by str.startswith."""
import pytest

import index_edges_cases as ic

KEYS = ic.case_keys()


def three_references(case):
    for weighted in (False, True):
        brute = ic.brute_counts(case, weighted)
        assert ic.c_reference(case, weighted) == brute, (case.name, weighted)
        if weighted and len(case.tags) > 1000:      # (the Python trie of a large index is slow to build: once is enough)
            continue
        m, st = ic.py_reference(case, weighted)
        assert (m, st) == brute, (case.name, weighted)
    return ic.brute_counts(case)


@pytest.mark.parametrize("key", KEYS, ids=lambda k: "%s%r" % k)
def test_case_reads_and_references(key):
    case = ic.get_case(key)
    stored = ic.stored_tags(case)
    assert ic.is_prefix_free(stored) and len(set(stored)) == len(stored)
    assert ic.is_prefix_free([b + ic.CUT for b in case.barcodes])
    probe = ic.Brute(case)
    kinds = {}
    for kind, seq in case.reads:
        bar, tag = probe.lookup(seq)
        kinds[kind] = kinds.get(kind, 0) + 1
        if kind == "hit":
            assert bar >= 0 and tag >= 0, seq
        elif kind in ic.MISS_KINDS:
            assert bar >= 0 and tag < 0, (kind, seq)           # every near miss really is a miss
        elif kind == "nobar":
            assert bar < 0
    assert kinds["hit"] >= min(len(stored), 300) and kinds["random"] >= 100
    full = set(stored)          # (where all four last bases are tags -- the families of four at L = 33 -- no change of it misses)
    if not all(t[:-1] + c in full for t in stored for c in "ACGT"):
        assert kinds["last"] >= kinds["hit"] // 2 and kinds["short"] >= kinds["hit"] // 2
    if max(len(t) for t in stored) > 33:            # (at 33 a stem's four next bases are all taken: no foreign tail)
        assert kinds["stem"] >= min(len(stored), 300) // 4
    m, st = three_references(case)
    assert st["reads"] == len(case.reads) and st["reads"] > st["barcut"] > st["tag"] >= kinds["hit"]
    assert case.data.count(b"\n") == 4 * len(case.reads)


def test_builders_are_deterministic():
    for fn, args in ((ic.family_case, (65,)), (ic.family_case, ("w1",)), (ic.ring_case, (10, 1)), (ic.dense_random_case, (3,)),
                     (ic.short_case, (17,)), (ic.nq_case, (2, 8)), (ic.wide_offset_case, (64,))):
        assert fn.__wrapped__(*args) == fn(*args)


def test_width_and_staging_rule():
    """32 W bases hold the tag; 16 (2 W + 3) staged bytes hold a read that starts at byte 15 of a chunk, an offset of 32
    and a tag of 32 W -- with one byte to spare (79 of 80 at W = 1, 367 of 368 at W = 10), and not one base more."""
    assert [ic.width_of(L) for L in ic.FAMILY_L] == [1, 2, 2, 3, 3, 4, 4, 6, 6, 10, 10]
    for W in ic.WIDTHS:
        assert 15 + 32 + 32 * W == 16 * (2 * W + 3) - 1
        assert ic.width_of(32 * W, 32) == W
        if W < 10:
            assert ic.width_of(32 * W, 34) == ic.WIDTHS[ic.WIDTHS.index(W) + 1]
    assert (15 + 32 + 32, 15 + 32 + 320) == (79, 367)
    with pytest.raises(StopIteration):
        ic.width_of(321)
    with pytest.raises(StopIteration):
        ic.width_of(320, 40)


def test_promised_regimes():
    """What the GPU module asserts from td_index_info follows from the rules restated here."""
    for L in ic.FAMILY_L:
        case = ic.family_case(L)
        n, spb = ic.family_size(L), ic.SPB[ic.width_of(L)]
        assert case.expect["W"] == ic.width_of(L) and case.expect["min_longest"] == -(-n // spb) - 1
        by_stem = {}
        for t in ic.stored_tags(case):
            assert len(t) == L
            by_stem[t[:32]] = by_stem.get(t[:32], 0) + 1
        assert set(by_stem.values()) == {n} and sum(by_stem.values()) >= 45
    assert ic.family_size(33) == 4 and ic.family_size(32) == 1 and all(ic.family_size(L) == 45 for L in ic.FAMILY_L[2:])
    for W in ic.WIDTHS[1:]:
        stored = ic.stored_tags(ic.family_case(("mixed", W)))
        assert len({t[:32] for t in stored}) == 1 and len({len(t) for t in stored}) > 5 and max(len(t) for t in stored) == 32 * W
    w1 = ic.family_case("w1")
    assert w1.expect["m_bases"] == 20 and w1.expect["W"] == 1 and w1.expect["min_longest"] == 8
    assert len({t[:20] for t in ic.stored_tags(w1) if len(t) == 32}) == 1
    for W in ic.WIDTHS:
        assert [ic.ring_family_size(w) for w in ic.WIDTHS] == [76, 45, 30, 45, 30, 15]
        for k in range(ic.RING_STEMS):
            case = ic.ring_case(W, k)
            shape = ic.expected_shape(ic.stored_tags(case))
            nlong = len(case.tags) - shape["nshort"]
            assert case.load == 95 and 8 * ic.SPB[W] * 0.95 < nlong <= 16 * ic.SPB[W] * 0.95 - (1 if W == 1 else 0)
            assert case.expect["W"] == W and case.expect["min_longest"] >= 14
        assert len({ic.stored_tags(ic.ring_case(W, k))[-1][:20] for k in range(ic.RING_STEMS)}) == ic.RING_STEMS
        dense = ic.dense_random_case(W)
        nb = ic.DENSE_BUCKETS[W]
        assert nb // 2 * ic.SPB[W] * 0.95 < len(dense.tags) < nb * ic.SPB[W] * 0.95 and 1400 < len(dense.tags) < 2500
    for L in (64, 96):
        case = ic.allelic_case(L)
        by_stem = {}
        for t in ic.stored_tags(case):
            assert len(t) == L
            by_stem[t[:32]] = by_stem.get(t[:32], 0) + 1
        assert len(by_stem) == 3000 and set(by_stem.values()) == {4, 5, 6}
    shapes = {n: ic.short_case(n).expect for n in ic.SHORT_COUNTS}
    assert (shapes[15]["m_bases"], shapes[15]["nshort"]) == (32, 15) and (shapes[16]["m_bases"], shapes[16]["nshort"]) == (32, 16)
    for n in (17, 40, "all"):
        assert shapes[n]["m_bases"] < 32 and shapes[n]["nshort"] == 16
        m = shapes[n]["m_bases"]
        rests = {len(seq) - len(b) - len(ic.CUT) for kind, seq in ic.short_case(n).reads if kind == "edge"
                 for b in ic.short_case(n).barcodes if seq.startswith(b + ic.CUT)}
        assert {m - 1, m, m + 1} <= rests
    assert sorted((W, ic.nq_case(W, nq).expect["nch2"]) for W in (1, 2, 3) for nq in ic.NQ[W]) == \
        sorted((W, nq) for W in (1, 2, 3) for nq in ic.NQ[W])
    for n in ic.WIDE_OFFSET_LENS:
        assert ic.wide_offset_case(n).expect["W"] == ic.WIDTHS[ic.WIDTHS.index(n // 32) + 1]


@pytest.mark.parametrize("W", ic.WIDTHS)
def test_staging_buffers(W):
    """Offset 32 and tags of exactly 32 W bases: the sequence lines start at every alignment, end at the tag's last base
    (then \\n, \\r\\n or the end of the buffer) and slide across the 96 KiB boundary; the references agree on every
    buffer, and every read but the planted miss counts."""
    barcodes, tags, miss = ic.staging_index(W)
    assert all(len(b) + len(ic.CUT) == 32 for b in barcodes) and all(len(t) == len(ic.CUT) + 32 * W for t in tags) and len(tags) == 6
    assert ic.is_prefix_free(tags + [ic.CUT + miss])

    def seq_starts(data):
        at, out = 0, []
        for i, line in enumerate(data.splitlines(keepends=True)):
            if i & 3 == 1:
                out.append((at, line.rstrip(b"\r\n")))
            at += len(line)
        return out
    for nl in ("\n", "\r\n"):
        data = ic.staging_aligned(W, nl)
        starts = seq_starts(data)
        assert len(starts) == 16 * 7 and {at & 15 for at, _ in starts} == set(range(16))
        assert all(len(seq) == 32 + 32 * W for _, seq in starts)
        m, st = three_references(ic.staging_case(W, data))
        assert st == {"reads": 112, "barcut": 112, "tag": 96}
    for a in range(16):
        data = ic.staging_tail(W, a)
        at, seq = seq_starts(data)[-1]
        assert at & 15 == a and data.endswith(seq) and len(seq) == 32 + 32 * W
        assert three_references(ic.staging_case(W, data))[1] == {"reads": 2, "barcut": 2, "tag": 2}
    offsets = ic.staging_slide_offsets(W)
    n = 32 + 32 * W
    assert {d & 15 for d in offsets} == set(range(16)) and {-n - 2, -n - 1, -n, -n + 1, -1, 0, 1} <= set(offsets)
    for d in offsets:
        data = ic.staging_slide(W, d)
        assert [at for at, _ in seq_starts(data) if at >= ic.SEAM - 400][0] == ic.SEAM + d
        assert len(data) > ic.SEAM + 32 * 1024
        assert max(len(x) for x in data.splitlines()) <= 4096
        if d in (offsets[0], -n, 0):
            st = three_references(ic.staging_case(W, data))[1]
        else:
            st = ic.c_reference(ic.staging_case(W, data))[1]
        assert st["tag"] == 2 and st["barcut"] == 3
