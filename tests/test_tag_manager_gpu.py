"""Tag Manager on an MI355X: K2's order against sorted(zip(seqs, names)) (10^6 random tags included), K3's walks
against the host walk on the adversarial lookup sets, K4's masks against compareTags in both modes, every golden
transcript and function call through the device backend, and large runs (compareTagSets on 2 x 10^5 markers,
consolidateTagSets on 5 x 10^4) compared with the host backend.

The independent checks are Python's own sorted() and the reference-shaped compareTags / walk_host restatements."""
import random

import numpy as np
import pytest

from tag_manager_cases import (LOOKUPS, TRANSCRIPTS, check_functions, lookup_results, lookup_set, run_transcript,
                               sorted_names)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd.engine import default_engine
    return default_engine(0)


# ------------------------------------------------------------------ K2
def test_k2_order_1e6_random(eng):
    """10^6 tags of 1-150 bases with shared stems, A tails and duplicates under other names."""
    from tagdigger_amd.tagset import SortedTags
    rng = np.random.default_rng(11)
    n = 1_000_000
    lens = rng.integers(1, 151, n)
    codes = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(lens.sum()))].tobytes().decode()
    offs = np.concatenate([[0], np.cumsum(lens)])
    seqs = [codes[offs[i]:offs[i + 1]] for i in range(n)]
    for i in range(0, n, 97):                      # duplicates and A-extended prefixes
        seqs[i] = seqs[i + 1] if i % 2 else seqs[i + 1][:40] + "A" * (i % 5)
    names = ["m%07d_%d" % (int(x), i % 3) for i, x in enumerate(rng.permutation(n))]
    st = SortedTags(eng, names, seqs)
    st.close()
    want = sorted(zip(seqs, names))
    assert list(st.seqs) == [w[0] for w in want]
    assert list(st.names) == [w[1] for w in want]


@pytest.mark.parametrize("name", sorted({x["set"] for x in LOOKUPS}))
def test_k2_golden_sets(eng, name):
    from tagdigger_amd import tagdigger_fun as tf
    names, seqs = lookup_set(name)
    srt = tf.sortTagsBySeq([names, seqs], backend="gpu")
    assert list(srt[0]) == sorted_names(name)


# ------------------------------------------------------------------ K3
def _queries(seqs, golden):
    qs = set(golden)
    for s in seqs[:400]:
        qs.update({s, s[:len(s) // 2], s[:-1], s + "A", s + "C"})
    return sorted(q for q in qs if q)


@pytest.mark.parametrize("name", sorted({x["set"] for x in LOOKUPS}))
def test_k3_walks_match_host(eng, name):
    from tagdigger_amd.tagset import SortedTags, walk_host
    names, seqs = lookup_set(name)
    golden = [q for x in LOOKUPS if x["set"] == name for q in x["queries"]]
    st = SortedTags(eng, names, seqs)
    try:
        qs = _queries(list(st.seqs), golden)
        for adl in (False, True):
            got = st.walks(qs, adl).tolist()
            want = [list(walk_host(st.seqs, q, adl)) for q in qs]
            bad = [(q, g, w) for q, g, w in zip(qs, got, want) if g != w]
            assert not bad, bad[:5]
    finally:
        st.close()


@pytest.mark.parametrize("name", sorted({x["set"] for x in LOOKUPS}))
def test_k3_golden_lookups(eng, name):
    from tagdigger_amd import tagdigger_fun as tf
    names, seqs = lookup_set(name)
    srt = tf.sortTagsBySeq([names, seqs], backend="host")
    for rec in (x for x in LOOKUPS if x["set"] == name):
        each, every = lookup_results(rec)
        adl = rec["allowDiffLengths"]
        for q, want in zip(rec["queries"], each):
            assert sorted(tf.lookupMarkerByTag(srt[0], srt[1], [q], allowDiffLengths=adl)) == want, q
        assert sorted(tf.lookupMarkerByTag(srt[0], srt[1], rec["queries"], allowDiffLengths=adl)) == every


# ------------------------------------------------------------------ K4
def test_k4_masks_match_compare_tags(eng):
    from tagdigger_amd.tagdigger_fun import compareTags
    from tagdigger_amd.tagset import varsites
    rng = random.Random(5)
    groups = []
    for _ in range(3000):
        L = rng.choice([1, 31, 63, 64, 65, 127, 128, 129, 191, 192, 200, 255, 256])
        base = "".join(rng.choices("ACGT", k=L))
        g = []
        for _ in range(rng.randint(1, 20)):
            t = list(base[:rng.randint(max(1, L - 70), L)])
            for _ in range(rng.randint(0, 3)):
                p = rng.randrange(len(t))
                t[p] = rng.choice("ACGT")
            g.append("".join(t))
        groups.append(g)
    for trim in (True, False):
        cols, bad = varsites(eng, groups, trim)
        assert not any(bad)
        for g, c in zip(groups, cols):
            assert c == [x[0] for x in compareTags(g, trim=trim)]


def test_k4_flags_non_acgt(eng):
    from tagdigger_amd.tagset import varsites
    cols, bad = varsites(eng, [["ACGT", "ACTT"], ["ACNT", "ACGT"], ["A" * 200 + "x"]], True)
    assert bad == [0, 1, 1] and cols[0] == [2]


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("case", TRANSCRIPTS, ids=[c["name"] for c in TRANSCRIPTS])
def test_transcript_device(case, tmp_path):
    run_transcript(case, "gpu", tmp_path)


def test_functions_device():
    check_functions("gpu")


def _study(n_markers, seed):
    rng = random.Random(seed)
    old = [[], []]
    new = [[], []]
    for i in range(n_markers):
        a = "TGCAG" + "".join(rng.choices("ACGT", k=59))
        p = rng.randrange(5, 60)
        b = a[:p] + rng.choice([x for x in "ACGT" if x != a[p]]) + a[p + 1:]
        old[0] += ["M%06d_0" % i, "M%06d_1" % i]
        old[1] += [a, b]
        r = rng.random()
        if r < 0.3:
            na, nb = a[:50], b[:50]
        elif r < 0.6:
            na, nb = a, b
        else:
            na = "TGCAG" + "".join(rng.choices("ACGT", k=59))
            nb = na[:30] + rng.choice([x for x in "ACGT" if x != na[30]]) + na[31:]
        if na == nb:
            nb = na + "A"
        new[0] += ["N%06d_0" % i, "N%06d_1" % i]
        new[1] += [na, nb]
    return old, new


def test_large_run_equals_host(capsys):
    """compareTagSets on 2 x 10^5 markers (4 x 10^5 tags per set) and consolidateTagSets on 5 x 10^4: device backend
    == host backend.  (consolidateTagSets's host restatement takes about 30 s at 2 x 10^5 markers, more than this
    file's share of the suite's time.)"""
    from tagdigger_amd import tagdigger_fun as tf
    from tagdigger_amd import tagset
    old, new = _study(200_000, 3)
    tagset.stage_ms.clear()
    for adl in (True, False):
        got = tf.compareTagSets(old, new, perfectMatch=not adl, allowDiffLengths=adl, backend="gpu")
        want = tf.compareTagSets(old, new, perfectMatch=not adl, allowDiffLengths=adl, backend="host")
        assert list(got.items()) == list(want.items())
    old, new = _study(50_000, 4)
    got = tf.consolidateTagSets(old, new, allowDiffLengths=True, backend="gpu")
    out_gpu = capsys.readouterr().out
    want = tf.consolidateTagSets(old, new, allowDiffLengths=True, backend="host")
    assert capsys.readouterr().out == out_gpu
    assert got[0] == want[0]
    assert list(got[1].items()) == list(want[1].items())
    assert {"K1", "K2", "K3", "K4"} <= set(tagset.stage_ms)
