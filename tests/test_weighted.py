"""The references of the weighted count agree with each other before the kernel is judged by them: on every case
of tests/weighted_cases.py the C oracle gives what the literal Python rule gives -- the matrix as signed integers,
reads / barcut / tag, and the exception type.  No GPU."""
import random

import pytest

import weighted_cases as wc
from helpers import small_index


def agree(case):
    py, c = wc.py_reference(case), wc.c_reference(case)
    assert py[0] == c[0], case.name
    if py[0] == "raises":
        assert py[1] is c[1], case.name
        return py
    assert c[1] == py[1], case.name
    assert {k: c[2][k] for k in ("reads", "barcut", "tag")} == py[2], case.name
    if case.maxreads >= 5e9:
        assert c[2]["lines"] >= wc.line_count(case.data), case.name
    return py


@pytest.mark.parametrize("header,ok", wc.HEADERS, ids=lambda v: repr(v)[:24])
def test_header_grammar(header, ok):
    """The reference's own expression, the Python oracle and the C oracle on one record."""
    case = wc.Case("header", wc.G_BAR, wc.G_TAG, "TGCAG", (header + wc.G_BODY).encode("latin-1"))
    if ok:
        assert agree(case)[1] == [[wc.literal_rule(header)]]
    else:
        with pytest.raises(ValueError):
            wc.literal_rule(header)
        assert agree(case) == ("raises", ValueError)


def test_small_cases():
    seen = set()
    for case in wc.small_cases():
        seen.add(agree(case)[0])
    assert seen == {"ok", "raises"}
    assert wc.py_reference(wc.maxreads_header_cases()[0])[0] == "ok"
    assert wc.py_reference(wc.maxreads_header_cases()[1]) == ("raises", ValueError)
    assert wc.py_reference(wc.wide_cases()[0])[1] == [[2 ** 32 - 1 + 5 + 2 ** 33 + 2 ** 40]]
    assert wc.py_reference(wc.wide_cases()[1])[1] == [[-7 - 2 ** 35]]


def test_tile_sweep_cases():
    for pad in wc.SWEEP_PADS:
        case = wc.tile_sweep_case(pad)
        assert len(case.data) > 3 * wc.TILE and case.data.index(b"@h") == wc.TILE + pad
        py = agree(case)
        assert sorted(v for row in py[1] for v in row) == [1000, 1007, 1028, 1035, 14345, 15345], pad


@pytest.mark.parametrize("cutsite,nl", wc.FUZZ_SHAPES)
@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_cases(cutsite, nl, seed):
    case = wc.fuzz_case(cutsite, nl, seed)
    py = agree(case)
    assert py[0] == "ok" and 0 < py[2]["tag"] < py[2]["barcut"] < py[2]["reads"]
    assert any(v < 0 for row in py[1] for v in row) and any(v > 2 ** 32 for row in py[1] for v in row)


def test_generator_is_dirty():
    """What the generator promises is in its output: every terminator, blanks, N, lower case, long lines, weights in
    all their forms, headers without count=."""
    rnd = random.Random(5)
    barcodes, tags, cutsites = small_index(rnd, "TGCAG")
    data = wc.weighted_fastq(rnd, barcodes, tags, cutsites, nrec=1500, nl_choices=("\n", "\r\n", "\r"), long_lines=True,
                             permanent_shifts=True)
    lines = data.splitlines()
    assert b"\r\n" in data and b"\r@" in data and b"\n@" in data
    assert any(len(l) > 600 for l in lines) and b"" in lines
    for needle in (b"count=0", b"count=-", b"count=+", b"count=00", b"_", b"count= ", b"N", b"acg"):
        assert needle in data, needle
    assert any(l.startswith(b"@r") and b"count=" not in l for l in lines)
    assert len(lines) > 4 * 1500                                       # (the lines between records)


@pytest.mark.parametrize("maxlen", wc.WIDTH_MAXLENS)
def test_width_cases(maxlen):
    py = agree(wc.width_case(maxlen))
    assert py[0] == "ok" and py[2]["tag"] > 50


@pytest.mark.parametrize("nl", ["\n", "\r\n"])
def test_piece_seam_cases(nl):
    """All 2 R alignments against the C oracle and the matrix their construction implies; the Python rule on the
    first, the last and one in the middle (a file has ~1 600 reads)."""
    for lead in wc.SEAM_LEADS:
        case = wc.seam_case(lead, nl)
        want, st = wc.seam_expected(case)
        c = wc.c_reference(case)
        assert c[1] == want and c[2] == st, lead
        assert len(case.data) > 3 * wc.SEAM_PIECE
        rec0 = case.data.index(b"@s0000")
        assert rec0 % wc.SEAM_R == lead and len(case.data) - rec0 == wc.SEAM_NREC * wc.SEAM_R
        if lead in (0, 61, wc.SEAM_R - 1):
            agree(case)
