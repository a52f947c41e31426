"""td_count_and_split_device on every route (tests/fused_cases.py; tests/test_fused.py shows without a GPU that every
input can catch a wrong line index).

The call enqueues a count pass and the splitter's line prefix and decisions behind it.  Where the splitter's kernel is
k_split2 (24 KiB tiles) and the count pass just enqueued was a free-running one with 24 KiB tiles over as many tiles, the
prefix takes every tile's terminator count from the record the count kernel left (k_info_counts; prefix source 2);
every other pairing counts the terminators from the bytes again (k_count_lines; source 1).  Engine.split_prefix_source
says which one ran, and every route below asserts the one it expects -- a test that meant to run the fused source and
ran a fallback fails.

Every run: the call through the binding into a buffer of sentinels; every slot of a sequence line holds the oracle's
decision, every slot behind them the sentinel; the terminator count is the bytes'; matrix and counters are the C
oracle's.  All exact.  Then the two separate calls (reset, count_device, split_device) on the same resident bytes must
give the same answers.

Geometry, from the kernels' text: k_fast4 and k_split2 take tiles of 24 576 bytes, k_fast2 tiles of tile_kb2 (16, 24,
32 KiB), k_fast and the exact kernel tiles of tile_kb (16, 32 KiB), k_split tiles of 16 384 bytes."""
import ctypes as C

import numpy as np
import pytest

import fused_cases as fc
import ring_cases as rc
import splitter_edge_cases as ec
from test_splitter_edges_gpu import first_sequence_line, set_splitter

pytestmark = pytest.mark.gpu

SENTINEL, SLACK = fc.SENTINEL, fc.SLACK
TD_E_ARG, TD_E_STATE = -2, -9
RESTORE = dict(fastpath=1, kernel=4, tile_kb2=0, tile_kb=32, prescan=0, split_kernel=2, progress=0, max_grid=0, run=8, f4_nprod=0,
               fast_max_matrix_bytes=0)

# (id, options, prefix source where the splitter set is compact -- where it is not, k_split decides and the source is 1)
DEFAULT = ("default", dict(kernel=4, split_kernel=2), 2)
DEEP = [("ring-run%d-nprod%d" % (run, nprod), dict(kernel=4, max_grid=1, run=run, f4_nprod=nprod), 2)
        for run in (1, 3, 4096) for nprod in (0, 7, 13)]
OTHER = [("fast2-24-grid0", dict(kernel=2, tile_kb2=24, max_grid=0), 2),
         ("fast2-24-grid1", dict(kernel=2, tile_kb2=24, max_grid=1), 2),
         ("fast2-16", dict(kernel=2, tile_kb2=16), 1),
         ("fast2-32", dict(kernel=2, tile_kb2=32), 1),
         ("fast-16", dict(kernel=1, tile_kb=16), 1),
         ("fast-32", dict(kernel=1, tile_kb=32), 1),
         ("exact", dict(fastpath=0), 1),
         ("prescan", dict(prescan=1), 1),
         ("k_split-under-24", dict(kernel=4, split_kernel=1), 1),     # (the d_state reallocation: test_k_split_under_a_24k_count_pass_grows_d_state)
         ("progress", dict(progress=1, kernel=4), 2),
         ("matrix-fallback", dict(fast_max_matrix_bytes=-1), 1)]       # (-1: a limit below the case's matrix, set per case)


@pytest.fixture(scope="module")
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    yield e
    e.close()


def apply(eng, options, case=None):
    for k, v in RESTORE.items():
        eng.set_option(k, v)
    for k, v in options.items():
        if k == "fast_max_matrix_bytes" and v == -1:
            v = len(case.set.barcodes) * eng.ntags * 4          # (the free-running path needs the matrix to be smaller than this)
        eng.set_option(k, v)


class Resident:
    """A case's index and splitter set, its bytes in device memory, and a result buffer that is filled with sentinels
    before every call."""

    def __init__(self, eng, case, data=None):
        self.eng, self.case = eng, case
        self.data = case.data if data is None else data
        self.d = self.d_out = 0

    def __enter__(self):
        self.eng.set_index(list(self.case.set.barcodes), list(self.case.tags), self.case.set.cutsite)
        set_splitter(self.eng, self.case.set)
        self.d = self.eng.dev_alloc(max(16, len(self.data)))
        self.eng.h2d(self.d, self.data)
        self.cap = (fc.n_terminators(self.data) + 1) // 4 + 2
        self.fill = np.full((self.cap + SLACK) * 2, SENTINEL, dtype=np.uint32).tobytes()
        self.d_out = self.eng.dev_alloc(len(self.fill))
        return self

    def __exit__(self, *exc):
        self.eng.dev_free(self.d)
        self.eng.dev_free(self.d_out)

    def call(self, fused, nbytes=None, first_line=0, maxreads=5e9, d=None):
        """td_count_and_split_device (or td_split_device) through the binding; (int32 [cap + SLACK, 2], terminators)."""
        from tagdigger_amd import _binding as B
        from tagdigger_amd.engine import effective_maxreads
        eng = self.eng
        nbytes = len(self.data) if nbytes is None else nbytes
        d = self.d if d is None else d
        eng.h2d(self.d_out, self.fill)
        terms = C.c_uint64(0)
        if fused:
            B.check(eng._L.td_count_and_split_device(eng._h, C.c_void_p(d), nbytes, first_line, effective_maxreads(maxreads),
                                                     C.c_void_p(self.d_out), self.cap, None, C.byref(terms)))
        else:
            B.check(eng._L.td_split_device(eng._h, C.c_void_p(d), nbytes, first_line, C.c_void_p(self.d_out), self.cap, None, C.byref(terms)))
        raw = eng.d2h(self.d_out, len(self.fill))
        # which source that call's prefix took -- read before td_count_lines_device, a line prefix of its own (16 KiB tiles), runs.
        # It runs behind the call, never in front of it: in front it would size d_state for the 16 KiB tiles before the count pass
        self.source = eng.split_prefix_source()
        assert eng.count_lines_device(d, nbytes) == fc.n_terminators(self.data[:nbytes])
        return np.frombuffer(raw, dtype=np.int32).reshape(-1, 2), terms.value

    def check_decisions(self, res, terms, want, note, nbytes=None):
        nseq = len(want)
        got = res[:nseq]
        if not np.array_equal(got, want):
            bad = np.flatnonzero((got != want).any(axis=1))
            labels = self.case.labels
            raise AssertionError("%r: %d of %d decisions differ; slot, label, got, want: %r" % (
                note, len(bad), nseq, [(int(k), labels[k] if labels else None, got[k].tolist(), want[k].tolist()) for k in bad[:8]]))
        rest = res[nseq:].view(np.uint32)
        assert (rest == SENTINEL).all(), "%r: slots at or behind %d were written: %r" % (note, nseq, (np.argwhere(rest != SENTINEL)[:8] + [nseq, 0]).tolist())
        assert terms == fc.n_terminators(self.data if nbytes is None else self.data[:nbytes]), note

    def check_counts(self, want_m, want_st, note, bound=False, lines=None):
        """Matrix and counters against the C oracle's.  TD_STAT_LINES is the line terminators seen; the oracle's "lines" also
        counts a last line without a terminator, so that counter is held against the bytes' own terminators (`lines`: of
        several buffers).  With a bound it is left out: the oracle stops reading there, the device counts the buffer's."""
        got, st = self.eng.counts_numpy(), self.eng.stats()
        assert (got == want_m).all(), (note, "cells that differ", int((got != want_m).sum()), "sum", int(got.sum()), int(want_m.sum()))
        nterm = fc.n_terminators(self.data) if lines is None else lines
        want_st = dict(want_st, lines=nterm)
        if bound:
            st, want_st = dict(st, lines=0), dict(want_st, lines=0)
        assert st == want_st, (note, st, want_st)

    def check(self, want, want_m, want_st, source, note, first_line=0, maxreads=None):
        """One fused call against the oracles, from a reset engine."""
        kw = {} if maxreads is None else dict(maxreads=maxreads)
        self.eng.reset()
        res, terms = self.call(True, first_line=first_line, **kw)
        got_source = self.source
        assert got_source == source, (note, "prefix source", got_source, "expected", source)
        self.check_decisions(res, terms, want, note)
        self.check_counts(want_m, want_st, note, bound=maxreads is not None)
        return res

    def check_separate(self, want, want_m, want_st, note, first_line=0):
        """reset, count_device, split_device on the same bytes."""
        self.eng.reset()
        self.eng.count_device(self.d, len(self.data), first_line=first_line)
        res, terms = self.call(False, first_line=first_line)
        assert self.source == 1, note
        self.check_decisions(res, terms, want, note)
        self.check_counts(want_m, want_st, note)


def source_of(case, eng, nominal):
    """The route's source where k_split2 decides; k_split's 16 KiB tiles never match the count pass's."""
    used = eng.split_kernel_in_use()
    if nominal == 2:
        assert used == (2 if case.set.compact else 1), case.name
    return nominal if used == 2 else 1


def run_routes(eng, name, routes, variants):
    """variants: the whole bytes at first_line 0 and 4, and the bytes cut to begin at their first sequence line (first_line 1)."""
    case = fc.cases()[name]
    want = fc.expected_decisions(case)
    cut = first_sequence_line(case.data) if variants else None
    seen = set()
    try:
        with Resident(eng, case) as r:
            for rid, options, nominal in routes:
                apply(eng, options, case)
                source = source_of(case, eng, nominal)
                seen.add((rid.split("-")[0], source))
                for first_line in (0, 4) if variants else (0,):
                    m, st = fc.expected_counts(case, first_line=first_line)
                    r.check(want, m, st, source, (name, rid, "first_line", first_line), first_line=first_line)
                r.check_separate(want, *fc.expected_counts(case, first_line=0), (name, rid, "separate calls"))
            if cut is not None:
                tail = case.data[cut:]
                assert len(fc.expected_decisions(case._replace(name=name + " cut"), tail, 1)) == len(want)
                with Resident(eng, case, tail) as r2:
                    for rid, options, nominal in routes:
                        apply(eng, options, case)
                        m, st = fc.expected_counts(case, tail, first_line=1)
                        r2.check(want, m, st, source_of(case, eng, nominal), (name, rid, "first_line", 1), first_line=1)
    finally:
        apply(eng, {})
    print(" [%s: route, prefix source: %s] " % (name, ", ".join("%s %d" % x for x in sorted(seen))), end="")
    return seen


ALL = list(fc.cases())


@pytest.mark.parametrize("name", ALL)
def test_fused_default_and_deep_ring(eng, name):
    """The default route and one workgroup that takes every tile through its ring, at runs of 1, 3 and 4096 tiles and the
    estimated, 7 and 13 producer waves; first_line 0, 4 and 1."""
    seen = run_routes(eng, name, [DEFAULT] + DEEP, True)
    assert seen == ({("default", 2), ("ring", 2)} if fc.cases()[name].set.compact else {("default", 1), ("ring", 1)})


@pytest.mark.parametrize("name", ALL)
def test_fused_other_routes(eng, name):
    """k_fast2 at the splitter's tile and at the others, k_fast, the exact kernel (asked for, with the prescan, and for a
    matrix the free-running path does not address), k_split under a 24 KiB count pass (on this engine d_state has long
    grown past what either needs: the reallocation has a test of its own below), and the recording instantiation of k_fast4."""
    seen = run_routes(eng, name, OTHER, False)
    if fc.cases()[name].set.compact:
        assert {s for _, s in seen} == {1, 2}          # both sources, for every generator


# ---------------------------------------------------------------------------------------------------- d_state grows behind the count pass
def test_k_split_under_a_24k_count_pass_grows_d_state():
    """k_fast4 counts in 24 KiB tiles, k_split decides in 16 KiB tiles: launch_count sizes d_state for n / 24 KiB tiles and
    enqueues the count pass, which keeps its block sums there; line_prefix then asks for n / 16 KiB tiles, and DevBuf::ensure,
    which only grows, frees the array and allocates a larger one while the count pass is still enqueued.  That happens only
    where nothing has sized d_state before: a fresh Engine whose FIRST launch is the fused call (no td_count_lines_device in
    front of it), then, on the same engine, a buffer with more tiles than any before it, twice.  Matrix, counters and
    decisions are the oracles'; the growth itself cannot be seen from outside -- it follows from the sizes: 15, 43 and 188
    tiles of 24 KiB are 23, 64 and 282 of 16 KiB, each more than anything asked for before."""
    import tagdigger_amd
    names = ["edge:geometry-24576", "ring:qual", "ring:short"]
    tiles = [(-(-len(fc.cases()[n].data) // fc.TILE2), -(-len(fc.cases()[n].data) // fc.TILE1)) for n in names]
    assert all(t16 > t24 for t24, t16 in tiles) and all(tiles[k + 1][0] > tiles[k][1] for k in range(len(tiles) - 1))
    e = tagdigger_amd.Engine(0)
    try:
        for name in names:
            case = fc.cases()[name]
            with Resident(e, case) as r:
                apply(e, dict(kernel=4, split_kernel=1))
                assert e.split_kernel_in_use() == 1
                r.check(fc.expected_decisions(case), *fc.expected_counts(case), 1, (name, "k_split under k_fast4, d_state grows"))
                # and once more with the array as large as it needs to be
                r.check(fc.expected_decisions(case), *fc.expected_counts(case), 1, (name, "k_split under k_fast4"))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- bounds
BOUNDED = ["ring:qual", "ring:short", "edge:geometry-24576", "edge:geometry-16384", "extra:short-records"]


@pytest.mark.parametrize("name", BOUNDED)
def test_fused_with_a_bound(eng, name):
    """maxreads at three quarters of the reads, and 3, on the default route and all nine deep-ring ones.  The splitter has no bound: the decisions cover the whole buffer; the
    matrix is the oracle's at that maxreads.  The count pass stays free-running -- and the prefix takes its records --
    where the bound's line lies nbytes / 16 lines and more behind the first (fused_cases.bound_is_far, launch_count's rule
    restated): with lines of 18 bytes and more that is behind the buffer's end, so of these inputs only the short
    records have a bound that is far and stops the count; for the others both bounds are near ones (tests/test_fused.py)."""
    case = fc.cases()[name]
    want = fc.expected_decisions(case)
    reads = fc.expected_counts(case)[1]["reads"]
    far_seen = set()
    try:
        with Resident(eng, case) as r:
            for rid, options, nominal in [DEFAULT] + DEEP:
                apply(eng, options, case)
                for bound in (reads * 3 // 4, 3):
                    far = fc.bound_is_far(len(case.data), bound)
                    source = source_of(case, eng, nominal) if far else 1
                    m, st = fc.expected_counts(case, maxreads=bound)
                    assert st["reads"] == bound and 0 < m.sum() < fc.expected_counts(case)[0].sum()
                    r.check(want, m, st, source, (name, rid, "maxreads", bound), maxreads=bound)
                    far_seen.add((bound == 3, source))
    finally:
        apply(eng, {})
    print(" [%s: (near bound, prefix source) %r] " % (name, sorted(far_seen)), end="")
    assert far_seen == ({(False, 2), (True, 1)} if name == "extra:short-records" else {(False, 1), (True, 1)})


# ---------------------------------------------------------------------------------------------------- width
def test_fused_with_wide_tags(eng):
    """Tags of 100 bases: four words, which only k_fast counts (32 KiB tiles): the prefix is counted from the bytes.  The same
    bytes with tags of up to 64 bases take the count pass's records."""
    wide, base = fc.wide_case(), fc.cases()["edge:hall-A"]
    try:
        for case, source in ((wide, 1), (base, 2)):
            with Resident(eng, case) as r:
                apply(eng, {})
                r.check(fc.expected_decisions(case), *fc.expected_counts(case), source, (case.name, "default"))
                apply(eng, dict(max_grid=1))
                r.check(fc.expected_decisions(case), *fc.expected_counts(case), source, (case.name, "max_grid 1"))
    finally:
        apply(eng, {})


# ---------------------------------------------------------------------------------------------------- state between calls
def test_no_state_leaks_between_calls(eng):
    """Two buffers of as many 24 KiB tiles with other terminator counts in them (geometry-24576, and the same with its
    first record moved to the end)."""
    A, B = fc.cases()["edge:geometry-24576"], fc.rotated_case()
    assert len(A.data) == len(B.data) and A.tags == B.tags
    wa, wb = fc.expected_decisions(A), fc.expected_decisions(B)
    (ma, sa), (mb, sb) = fc.expected_counts(A), fc.expected_counts(B)
    both = {k: sa[k] + sb[k] for k in sa}
    both["lines"] = fc.n_terminators(A.data) + fc.n_terminators(B.data)
    try:
        with Resident(eng, A) as ra, Resident(eng, B) as rb:
            for options in ({}, dict(max_grid=1)):
                apply(eng, options)
                # a fused call on A, then plain td_split_device on B: A's tile records must not serve
                ra.check(wa, ma, sa, 2, "A fused")
                res, terms = rb.call(False)
                assert rb.source == 1
                rb.check_decisions(res, terms, wb, "B split behind A fused")
                # count_device on A, then a fused call on B: B's decisions, the matrix of both
                eng.reset()
                eng.count_device(ra.d, len(A.data))
                res, terms = rb.call(True)
                assert rb.source == 2
                rb.check_decisions(res, terms, wb, "B fused behind A counted")
                rb.check_counts(ma + mb, both, "A counted, B fused", lines=both["lines"])
                # two fused calls without a reset
                eng.reset()
                res, terms = ra.call(True)
                ra.check_decisions(res, terms, wa, "A fused, first of two")
                res, terms = rb.call(True)
                assert rb.source == 2
                rb.check_decisions(res, terms, wb, "B fused, second of two")
                rb.check_counts(ma + mb, both, "A fused, B fused", lines=both["lines"])
    finally:
        apply(eng, {})


# ---------------------------------------------------------------------------------------------------- bytes >= 0x80 in a read
def nonascii_inputs():
    for which, off in (("first", rc.HI_SPAN[0]), ("last", rc.HI_SPAN[1])):
        c = rc.hi_case(True, off)
        good = rc.Case("hi frame seq", *rc.sweep_index(), rc.CUT, rc._hi_frame(True)[0])
        yield "ring-%s" % which, fc.Case("nonascii ring " + which, fc.ring_set(tuple(c.barcodes), c.cutsite), tuple(c.tags), c.data, None, "ring"), good.data
    for n, c in ec.cases().items():
        if c.error == "nonascii":
            good = ec.cases()["geometry-%s" % n.split("-")[1]].data
            yield n, fc.adhoc("nonascii " + n, c.data, tags=fc.cases()["edge:geometry-24576"].tags), good


@pytest.mark.parametrize("which", [n for n, _, _ in nonascii_inputs()])
def test_fused_byte_above_ascii_in_a_sequence_line(eng, which):
    """NonAsciiSequence on the default and on the exact route; after reset a valid fused call on the same engine is right."""
    from tagdigger_amd import _binding as B
    case, good = next((c, g) for n, c, g in nonascii_inputs() if n == which)
    assert not fc.sequence_lines_are_ascii(case.data) and fc.sequence_lines_are_ascii(good)
    ok = case._replace(name=case.name + " good", data=good)
    try:
        for options in ({}, dict(max_grid=1), dict(fastpath=0)):
            with Resident(eng, case) as r:
                apply(eng, options)
                eng.reset()
                with pytest.raises(B.NonAsciiSequence):
                    r.call(True)
            with Resident(eng, ok) as r:
                r.check(fc.expected_decisions(ok), *fc.expected_counts(ok), 1 if "fastpath" in options else 2, (which, options, "after the error"))
    finally:
        apply(eng, {})
        eng.reset()


# ---------------------------------------------------------------------------------------------------- degenerate buffers
def degenerate_inputs():
    geo = ec.cases()["geometry-24576"].data
    out = [("one-terminator", b"\n"), ("one-base", b"A"), ("lf-only", b"\n" * 1003), ("crlf-only", b"\r\n" * (fc.TILE2 // 2 + 7)),
           ("cr-only", b"\r" * 777), ("tile2-less-1", geo[:fc.TILE2 - 1]), ("tile1-less-1", geo[:fc.TILE1 - 1])]
    out += [("small-%d" % n, ec.SMALL[:n]) for n in range(1, len(ec.SMALL) + 1)]
    return out


def test_fused_degenerate_buffers(eng):
    tags = fc.cases()["edge:geometry-24576"].tags
    try:
        for label, data in degenerate_inputs():
            case = fc.adhoc("degenerate " + label, data, tags=tags)
            want, (m, st) = fc.expected_decisions(case), fc.expected_counts(case)
            with Resident(eng, case) as r:
                for options, source in (({}, 2), (dict(max_grid=1), 2), (dict(fastpath=0), 1), (dict(split_kernel=1), 1)):
                    apply(eng, options)
                    r.check(want, m, st, source, (label, options))
                r.check_separate(want, m, st, (label, "separate calls"))
                # no bytes at all: nothing is written, nothing is counted
                eng.reset()
                res, terms = r.call(True, nbytes=0)
                assert terms == 0 and (res.view(np.uint32) == SENTINEL).all() and eng.counts_numpy().sum() == 0
                assert eng.stats() == dict(reads=0, barcut=0, tag=0, lines=0)
    finally:
        apply(eng, {})


def test_fused_argument_errors():
    """A pointer that is not 16-byte aligned: TD_E_ARG; no splitter: TD_E_STATE; neither counts anything."""
    import tagdigger_amd
    case = fc.cases()["edge:length-tile-16384"]
    e = tagdigger_amd.Engine(0)
    try:
        e.set_index(list(case.set.barcodes), list(case.tags), case.set.cutsite)
        d = e.dev_alloc(len(case.data) + 16)
        try:
            e.h2d(d, case.data)
            with pytest.raises(tagdigger_amd.TagdigError) as ei:
                e.count_and_split_device(d, len(case.data))
            assert ei.value.code == TD_E_STATE
            set_splitter(e, case.set)
            d_out = e.dev_alloc(8 * 1024)
            try:
                from tagdigger_amd import _binding as B
                terms = C.c_uint64(0)
                with pytest.raises(tagdigger_amd.TagdigError) as ei:
                    B.check(e._L.td_count_and_split_device(e._h, C.c_void_p(d + 1), len(case.data) - 1, 0, 10 ** 9, C.c_void_p(d_out), 1024, None, C.byref(terms)))
                assert ei.value.code == TD_E_ARG
            finally:
                e.dev_free(d_out)
            assert e.counts_numpy().sum() == 0
            res, terms = e.count_and_split_device(d, len(case.data))
            assert e.split_prefix_source() == 2 and terms == fc.n_terminators(case.data)
            assert np.array_equal(res[:len(fc.expected_decisions(case))], fc.expected_decisions(case))
        finally:
            e.dev_free(d)
    finally:
        e.close()
