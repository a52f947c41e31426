"""The tag index probe (match_stream / match_finish, csrc/kernels.hpp) and the table td_set_index builds, at their
structural edges, on the device: chains of displaced keys at every width, the ring wrap, W = 10, the hashed prefix below
32 bases and the short list, the staging budget used to its last byte, every piece count of k_fast2 / k_fast4, the
limits.  The cases are tests/index_edges_cases.py's, which tests/test_index_edges.py holds against three references on
the CPU.  Expected values: the C oracle on identical bytes -- the count matrix and reads / barcut / tag, exact, in every
kernel mode and once weighted (k_count<4, W, true>).  td_index_info only shows that a case reached the regime it is
named after; no count is taken from it."""
import functools

import numpy as np
import pytest

import index_edges_cases as ic
from helpers import DEFAULT_MODE, KERNEL_MODES, apply_mode, mode_id

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _reference(barcodes, tags, extra_off, data, weighted):
    case = ic.Case("", list(barcodes), list(tags), ic.CUT, None, data, 25, extra_off, None)
    st = {}
    m = ic.COracle(case).count_bytes(data, tassel_tagcount=weighted, stats=st)
    return m, (st["reads"], st["barcut"], st["tag"])


def reference(case, weighted=False):
    """(matrix, (reads, barcut, tag)) from the C oracle; computed once and left unchanged."""
    return _reference(tuple(case.barcodes), tuple(case.tags), case.extra_off, case.data, weighted)


def load_index(eng, case):
    if case.extra_off:          # the tag search starts behind the barcode entry: the C-ABI's lists
        barcut = [b + case.cutsite for b in case.barcodes]
        eng._set_index_lists(barcut, len(barcut), [len(x) + case.extra_off for x in barcut], ic.stored_tags(case))
    else:
        eng.set_index(case.barcodes, case.tags, case.cutsite)


def assert_regime(info, expect, name):
    for key, want in expect.items():
        if key.startswith("min_"):
            assert info[key[4:]] >= want, (name, key, info)
        else:
            assert info[key] == want, (name, key, info)


def count_and_compare(eng, case, weighted, what):
    want, wst = reference(case, weighted)
    eng.reset()
    eng.count_bytes(case.data, tassel_tagcount=weighted)
    got = eng.counts_numpy(signed=weighted)
    st = eng.stats()
    assert (got == (want.astype(np.int64) if weighted else want)).all(), (case.name, what)
    assert (st["reads"], st["barcut"], st["tag"]) == wst, (case.name, what)


def check(eng, case, modes=KERNEL_MODES):
    """The case in every kernel mode and once weighted; returns td_index_info's report."""
    try:
        eng.set_option("table_load_pct", case.load)
        load_index(eng, case)
        info = eng.index_info()
        if case.expect:
            assert_regime(info, case.expect, case.name)
        for mode in modes:
            apply_mode(eng, mode)
            count_and_compare(eng, case, False, mode_id(mode))
        apply_mode(eng, DEFAULT_MODE)
        count_and_compare(eng, case, True, "weighted")
        eng.reset()
    finally:
        eng.set_option("table_load_pct", 25)
        apply_mode(eng, DEFAULT_MODE)
    return info


# ------------------------------------------------------------------------------------------------ chains
@pytest.mark.parametrize("L", ic.FAMILY_KEYS, ids=str)
def test_families_at_every_width(eng, L):
    """45 tags behind one 32-base stem share a home bucket: a chain of at least ceil(45 / spb) - 1 hops, at the first and
    the last length of every width; hits along the whole chain, and misses that walk it to its end."""
    case = ic.family_case(L)
    info = check(eng, case)
    assert info["W"] == case.expect["W"] and info["longest"] >= case.expect["min_longest"]
    if L != 32:
        assert info["displaced"] > 0


@pytest.mark.parametrize("W", ic.WIDTHS)
def test_dense_ring_wraps(eng, W):
    """16 buckets at 95 % load and one family that fills them: the chain covers nearly the whole ring, and for at least
    one of the stems it goes on from the last bucket to bucket 0."""
    wrapped = []
    for k in range(ic.RING_STEMS):
        info = check(eng, ic.ring_case(W, k))
        assert info["buckets"] == 16 and info["W"] == W
        wrapped.append(info["wrapped"])
    assert any(wrapped), wrapped


@pytest.mark.parametrize("W", ic.WIDTHS)
def test_random_tags_at_95_percent_load(eng, W):
    """Many interleaved chains: full buckets carry the filter bits of foreign keys, and most misses stop at a clear one."""
    case = ic.dense_random_case(W)
    info = check(eng, case)
    assert info["buckets"] == ic.DENSE_BUCKETS[W] and info["displaced"] >= len(case.tags) // 10 and info["longest"] >= 3


@pytest.mark.parametrize("L", [64, 96])
def test_multi_allelic_markers_at_default_load(eng, L):
    """4-6 alleles that differ behind base 32 and a bucket of 3 (64 bases) or 2 (96) slots: every marker is displaced."""
    check(eng, ic.allelic_case(L))


# ------------------------------------------------------------------------------------------------ m_bases, short list
@pytest.mark.parametrize("nshort", ic.SHORT_COUNTS, ids=str)
def test_short_list_and_hashed_prefix(eng, nshort):
    """15 and 16 tags below 32 bases leave m = 32; the 17th pulls m down to its length and the short list stays at 16."""
    info = check(eng, ic.short_case(nshort))
    assert (info["m_bases"] < 32) == (nshort in (17, 40, "all")) and info["nshort"] == (15 if nshort == 15 else 16)


# ------------------------------------------------------------------------------------------------ piece counts
@pytest.mark.parametrize("W,nq", [(W, nq) for W in (1, 2, 3) for nq in ic.NQ[W]])
def test_every_piece_count(eng, W, nq):
    """k_fast2<.., W, NQ> and k_fast4<W, NQ> for each of the three NQ of a width (and the other kernels on the same input)."""
    info = check(eng, ic.nq_case(W, nq))
    assert (info["W"], info["nch2"]) == (W, nq)


@pytest.mark.parametrize("maxlen", ic.WIDE_OFFSET_LENS)
def test_offset_behind_the_barcode_takes_the_next_width(eng, maxlen):
    """Kept regression (found by this module's piece-count cases): a tag offset of 40 with tags that fill their width."""
    case = ic.wide_offset_case(maxlen)
    info = check(eng, case)
    assert info["W"] == case.expect["W"] > ic.width_of(maxlen) and 15 + 40 + maxlen <= 16 * info["nch"]


# ------------------------------------------------------------------------------------------------ staging edge
def staging_buffers(W):
    out = [("aligned %r" % nl, ic.staging_aligned(W, nl)) for nl in ("\n", "\r\n")]
    out += [("buffer ends at alignment %d" % a, ic.staging_tail(W, a)) for a in range(16)]
    out += [("line starts at the tile boundary %+d" % d, ic.staging_slide(W, d)) for d in ic.staging_slide_offsets(W)]
    return out


@pytest.mark.parametrize("mode", KERNEL_MODES + ["weighted"], ids=lambda m: m if isinstance(m, str) else mode_id(m))
def test_exact_lengths_at_the_staging_edge(eng, mode):
    """Barcode + site of exactly 32 bases and tags of exactly 32 W, for every W: the read ends at the tag's last base --
    then \\n, \\r\\n, or the buffer --, its line starts at every alignment 0..15 (at 15 all but one staged byte is
    used), and it slides across a boundary of every tile size (96 KiB in: a boundary of 16, 24 and 32 KiB tiles; asserted below for the mode's own)."""
    weighted = mode == "weighted"
    try:
        for W in ic.WIDTHS:
            barcodes, tags, _ = ic.staging_index(W)
            eng.set_index(barcodes, tags, ic.CUT)
            info = eng.index_info()
            assert info["W"] == W and info["nch"] == 2 * W + 3 and info["m_bases"] == 32
            if not weighted:
                apply_mode(eng, mode)
            # the tile of this mode, as tests/test_gpu_parity.py::test_tile_boundary_sweep takes it (wide tags run k_fast /
            # k_count at tile_kb, the weighted kernel at 16 KiB): SEAM must be a boundary between two of its tiles
            tile_kb = 16 if weighted else mode.get("tile_kb", 32) if W > 3 or mode.get("kernel", 1) == 1 else 24 if mode["kernel"] == 4 else mode["tile_kb2"]
            assert ic.SEAM % (tile_kb * 1024) == 0 and ic.SEAM >= 2 * tile_kb * 1024
            for what, data in staging_buffers(W):
                count_and_compare(eng, ic.staging_case(W, data), weighted, (W, what))
            eng.reset()
    finally:
        apply_mode(eng, DEFAULT_MODE)


# ------------------------------------------------------------------------------------------------ limits
def test_limits(eng):
    import tagdigger_amd
    case = ic.limit_case(320)
    assert max(len(t) for t in ic.stored_tags(case)) == 320
    check(eng, case)
    rnd_tag = ic.stored_tags(case)[0]
    with pytest.raises(tagdigger_amd.TagdigError) as ei:
        eng.set_index(case.barcodes, case.tags + [ic.CUT + "A" + rnd_tag], ic.CUT)            # 321 bases behind the site
    assert ei.value.code == -7
    with pytest.raises(tagdigger_amd.TagdigError):
        eng.index_info()                                                                      # (no index after a failed build)
    check(eng, ic.family_case(64), modes=KERNEL_MODES[-1:])                                  # ... and the engine counts on
    with pytest.raises(tagdigger_amd.TagdigError) as ei:
        eng.set_index(["ACGT" * 7], case.tags, ic.CUT)                                        # barcode + site of 33 bases
    assert ei.value.code == -7
    with pytest.raises(tagdigger_amd.TagdigError) as ei:                                      # offset 40 and 320 bases: no width stages it
        eng._set_index_lists(["ACGT" * 6 + "ACG" + ic.CUT], 1, [40], ic.stored_tags(case))
    assert ei.value.code == -7
    check(eng, ic.family_case(64), modes=KERNEL_MODES[-1:])


# ------------------------------------------------------------------------------------------------ the drop-in function
@pytest.mark.parametrize("which", ["family of 320 bases", "multi-allelic markers"])
def test_find_tags_fastq_from_a_file(tmp_path, which):
    from oracle import tagdigger_oracle as orc
    from tagdigger_amd import tagdigger_fun as tf
    case = ic.family_case(320) if which.startswith("family") else ic.allelic_case(64)
    path = tmp_path / "edges.fq"
    path.write_bytes(case.data)
    want = orc.find_tags_fastq(str(path), case.barcodes, case.tags, ic.CUT)
    assert tf.find_tags_fastq(str(path), case.barcodes, case.tags, ic.CUT, progress=False) == want
    assert sum(map(sum, want)) >= 45
