"""Both splitter kernels at their structural edges (tests/splitter_edge_cases.py), against the oracle, which
tests/test_splitter_edges.py holds against the real reference on every edge read.

Every case runs under split_kernel 2 and 1, max_grid 0, 1 and 2, first_line 0 and 4, and once more as the same bytes
cut to begin at their first sequence line (first_line 1); all with exact equality.  td_split_device is called through
the binding with an output buffer filled with a sentinel: every slot of a sequence line holds the expected decision,
every slot behind them still holds the sentinel, and the terminator count is right.  td_split_kernel_in_use says which
kernel decided: 2 where the case is built to fit k_split2's compact form, 1 where it is built not to.

The geometry the cases are built for, from the kernels' text (kernel_splitter2.hpp, kernel_splitter.hpp, launch_split):
    k_split2<6>: tile 24 576 bytes (6 chunks of 16 bytes for each of 256 threads), halo 512 bytes, wave quarter 6 144
                 bytes, thread span 96 bytes, 384 line starts per wave list
    k_split<4>:  tile 16 384 bytes, thread span 64 bytes
"""
import ctypes as C

import numpy as np
import pytest

import splitter_edge_cases as ec

pytestmark = pytest.mark.gpu

TILE2, HALO2, QUARTER2, SPAN2, LIST2 = 24576, 512, 6144, 96, 384
TILE1, SPAN1 = 16384, 64
SENTINEL = 0x5A5A5A5A
SLACK = 8                 # result slots beyond what the call asks for: they must stay untouched too


def test_the_cases_are_built_for_this_geometry():
    assert set(ec.GEOM) == {TILE2, TILE1} and ec.HALO == HALO2
    assert ec.GEOM[TILE2] == {"quarter": QUARTER2, "span": SPAN2, "list": LIST2} and ec.GEOM[TILE1]["span"] == SPAN1
    assert QUARTER2 * 4 == TILE2 and SPAN2 * 256 == TILE2 and SPAN1 * 256 == TILE1 and LIST2 == QUARTER2 // 16


@pytest.fixture(scope="module")
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    yield e
    e.close()


def n_terminators(data):
    return len(ec.lines_of(data)) - (0 if data[-1:] in (b"\n", b"\r") else 1)


def split_with_sentinel(eng, d_buf, nbytes, first_line):
    """td_split_device into a buffer of sentinels; returns (int32 [cap + SLACK, 2], terminators)."""
    from tagdigger_amd import _binding as B
    cap = (eng.count_lines_device(d_buf, nbytes) + 1) // 4 + 2
    fill = np.full((cap + SLACK) * 2, SENTINEL, dtype=np.uint32).tobytes()
    d_out = eng.dev_alloc(len(fill))
    try:
        eng.h2d(d_out, fill)
        terms = C.c_uint64(0)
        B.check(eng._L.td_split_device(eng._h, C.c_void_p(d_buf), nbytes, first_line, C.c_void_p(d_out), cap, None, C.byref(terms)))
        raw = eng.d2h(d_out, len(fill))
    finally:
        eng.dev_free(d_out)
    return np.frombuffer(raw, dtype=np.int32).reshape(-1, 2), terms.value


def check_run(eng, d_buf, data, first_line, want, labels, note):
    res, terms = split_with_sentinel(eng, d_buf, len(data), first_line)
    nseq = ec.seq_line_count(data, first_line)
    assert nseq == len(want), note
    got = [(int(a), int(b)) for a, b in res[:nseq]]
    if got != want:
        bad = [(k, labels[k] if labels else None, got[k], want[k]) for k in range(nseq) if got[k] != want[k]]
        raise AssertionError("%s: %d of %d decisions differ; slot, label, got, want: %r" % (note, len(bad), nseq, bad[:8]))
    rest = res[nseq:].view(np.uint32)
    assert (rest == SENTINEL).all(), "%s: slots at or behind %d were written: %r" % (note, nseq, np.argwhere(rest != SENTINEL)[:8].tolist())
    assert terms == n_terminators(data), note


def set_splitter(eng, st):
    import contextlib
    import io
    from tagdigger_amd import tagdigger_fun as tf
    with contextlib.redirect_stdout(io.StringIO()):
        ends = tf._adapter_ends(st.adapter, st.barcodes)
    s0, s1 = ec.sites_of(st)
    eng.set_splitter(st.barcodes, st.cutsite, s0, s1, ends)


def first_sequence_line(data):
    """Offset of the buffer's second line (its first sequence line), or None where it has none."""
    first = ec.lines_of(data)[0]
    cut = len(first) + (2 if data[len(first):len(first) + 2] == b"\r\n" else 1)
    return cut if cut < len(data) else None


@pytest.mark.parametrize("name", [n for n, c in ec.cases().items() if c.error is None])
def test_gpu_splitter_edges(eng, name):
    c = ec.cases()[name]
    st = ec.SETS[c.set]
    want = ec.expected(c.set, ec.ascii_twin(c.data))      # (bytes >= 0x80 lie in header lines only: the builders checked)
    cut = first_sequence_line(c.data)
    set_splitter(eng, st)
    d = eng.dev_alloc(len(c.data))
    d2 = eng.dev_alloc(len(c.data)) if cut is not None else None
    seen = {}
    try:
        eng.h2d(d, c.data)
        if cut is not None:
            eng.h2d(d2, c.data[cut:])
        for kern in (2, 1):
            eng.set_option("split_kernel", kern)
            used = eng.split_kernel_in_use()
            assert used == (2 if kern == 2 and st.compact else 1), (name, kern)
            seen[kern] = used
            for grid in (0, 1, 2):
                eng.set_option("max_grid", grid)
                for first_line in (0, 4):
                    check_run(eng, d, c.data, first_line, want, c.labels, (name, "kernel", used, "max_grid", grid, "first_line", first_line))
                if cut is not None:
                    check_run(eng, d2, c.data[cut:], 1, want, c.labels, (name, "kernel", used, "max_grid", grid, "first_line", 1))
    finally:
        eng.set_option("max_grid", 0)
        eng.set_option("split_kernel", 2)
        eng.dev_free(d)
        if d2 is not None:
            eng.dev_free(d2)
    print(" [%s, set %s: kernel in use %d under split_kernel 2, %d under 1] " % (name, c.set, seen[2], seen[1]), end="")


@pytest.mark.parametrize("name", [n for n, c in ec.cases().items() if c.error == "nonascii"])
def test_gpu_splitter_byte_above_ascii_in_a_sequence_line(name):
    """A byte >= 0x80 in a sequence line ends the call in TD_E_NONASCII, whichever kernel meets it."""
    import tagdigger_amd
    from tagdigger_amd import _binding as B
    c = ec.cases()[name]
    for kern in (2, 1):
        for grid in (0, 1):
            e = tagdigger_amd.Engine(0)
            try:
                set_splitter(e, ec.SETS[c.set])
                e.set_option("split_kernel", kern)
                e.set_option("max_grid", grid)
                assert e.split_kernel_in_use() == kern
                d = e.dev_alloc(len(c.data))
                try:
                    e.h2d(d, c.data)
                    with pytest.raises(B.NonAsciiSequence):
                        split_with_sentinel(e, d, len(c.data), 0)
                finally:
                    e.dev_free(d)
            finally:
                e.close()


def test_gpu_split_kernel_query_needs_a_splitter():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    try:
        with pytest.raises(tagdigger_amd.TagdigError) as ei:
            e.split_kernel_in_use()
        assert ei.value.code == -9          # TD_E_STATE
        e.set_option("split_kernel", 1)
        with pytest.raises(tagdigger_amd.TagdigError):
            e.split_kernel_in_use()
    finally:
        e.close()
