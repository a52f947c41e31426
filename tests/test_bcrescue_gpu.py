"""Barcode rescue on the GPU (csrc/bcrescue.hip) against the brute-force restatement of tests/bcrescue_cases.py, through
td_bcrescue_device (a resident buffer) and td_bcrescue_file (the file readers): the matrix, the classes, the per-row
counters and the position histogram, for equality."""
import gzip
import random

import pytest

import bcrescue_cases as bc
from conftest import load_golden
from helpers import bgzf_bytes
from oracle import tagdigger_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    yield e
    e.close()


def fetched(eng):
    st = eng.bcrescue_stats()
    matrix, rows, pos = eng.bcrescue_fetch()
    st["row_rescued"] = rows.tolist()
    st["positions"] = [int(x) for x in pos]
    return matrix.tolist(), st


def run_pieces(eng, pieces, maxreads=5e9):
    for part, fl in pieces:
        if not part:
            continue
        d = eng.dev_alloc(len(part))
        try:
            eng.h2d(d, part)
            eng.bcrescue_device(d, len(part), fl, maxreads)
            eng.sync()
        finally:
            eng.dev_free(d)


def begin(eng, case, K):
    eng._bcrescue_begin_lists(case.barcut, case.barnum, case.tagoff, case.stored, K)


def device_rescue(eng, case, K=1, maxreads=5e9, pieces=None):
    """Through td_bcrescue_device: `pieces` = [(bytes, first_line), ...] of one begin, else the whole buffer."""
    begin(eng, case, K)
    try:
        run_pieces(eng, pieces or [(case.data, 0)], maxreads)
        return fetched(eng)
    finally:
        eng.bcrescue_end()


def file_rescue(eng, path, case, K=1, maxreads=5e9):
    begin(eng, case, K)
    try:
        eng.bcrescue_file(path, maxreads)
        return fetched(eng)
    finally:
        eng.bcrescue_end()


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def both_routes(eng, tmp_path, case, K, want=None):
    want = want or bc.ref_case(case, K)
    bc.check(device_rescue(eng, case, K), want)
    bc.check(file_rescue(eng, write(tmp_path, "r.fq", case.data), case, K), want)
    return want


# ---------------------------------------------------------------------------------------------------- golden payloads
@pytest.mark.parametrize("K", [1, 2])
def test_golden_payloads(eng, tmp_path, K):
    from tagdigger_amd import tagdigger_fun as tf
    cases = load_golden("hotpath_cases.json") + load_golden("hotpath_random.json")

    def run(path, args, maxreads):
        got = tf.rescue_barcodes_fastq(path, *args, maxreads=maxreads, max_mismatch=K)          # td_bcrescue_file on the default engine
        case = bc.Case(orc.read_fastq_bytes(path), *bc.lists(*args))
        assert device_rescue(eng, case, K, maxreads) == got
        return got
    ran, skips = bc.golden_payloads(tmp_path, cases, K, run)
    assert skips == bc.GOLDEN_SKIPS[K]                         # the host rule's, tests/test_bcrescue.py
    assert ran * 4 >= 3 * len(cases)


# -------------------------------------------------------------------- entry geometry, read length, ties, dirt, tag lengths
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", sorted(bc.NAMED))
def test_named_cases(eng, tmp_path, name, K):
    case = bc.NAMED[name](K)
    want = both_routes(eng, tmp_path, case, K)
    assert want[1]["rescued1"] >= 1
    # CRLF with a last line without terminator, bare CR
    text = case.data.decode("latin-1")
    for nl, cut in (("\r\n", 2), ("\r", 0)):
        data = text.replace("\n", nl).encode("latin-1")
        both_routes(eng, tmp_path, case._replace(data=data[:len(data) - cut]), K, want)


def test_line_as_the_buffers_last_bytes(eng, tmp_path):
    """the read line is the buffer's end: one base short of the entry, exactly the entry, a tag cut one base short"""
    case = bc.read_length_case()
    for raw in list(orc.iter_lines(case.data))[1::4]:
        one = case._replace(data=b"@a\n" + raw)
        both_routes(eng, tmp_path, one, 1)


# ---------------------------------------------------------------------------------------------------- tile composition
@pytest.mark.parametrize("kind", ["exact", "nohit", 63, 64, 65])
def test_tile_composition(eng, tmp_path, kind):
    case = bc.tile_case(kind)
    want = both_routes(eng, tmp_path, case, 2)
    assert want[1]["exact"] == (want[1]["reads"] if kind == "exact" else 0 if kind == "nohit" else 150 - kind)


def test_tile_seam_at_every_offset_of_the_head(eng):
    rnd = random.Random(71)
    bodies, tags = bc.some_tags(rnd, 3, 40)
    reads = ["ACGTTGCAG"[:4] + "AGCAG" + bodies[0] + "ACGT", "ACGTTGCAN" + bodies[1], "NCGTTGCAG" + bodies[2] + "A"]
    begin_lists = bc.lists(["ACGT"], tags)
    eng._bcrescue_begin_lists(*begin_lists, 1)
    try:
        for offset in range(0, 34):                                   # the line starts `offset` bytes before the tile's end
            read = reads[offset % 3]
            data = bc.seam_buffer(rnd, offset, read)
            before = fetched(eng)
            run_pieces(eng, [(data, 0)])
            after = fetched(eng)
            want = bc.ref_lists(data, *begin_lists, 1)
            assert want[1]["rescued1"] >= 1 and want[1]["tagged"] >= 1
            assert {k: after[1][k] - before[1][k] for k in bc.CLASSES + ("tagged",)} == {k: want[1][k] for k in bc.CLASSES + ("tagged",)}, offset
            assert [[a - b for a, b in zip(ra, rb)] for ra, rb in zip(after[0], before[0])] == want[0], offset
            assert [a - b for a, b in zip(after[1]["positions"], before[1]["positions"])] == want[3], offset
            assert [[a - b for a, b in zip(ra, rb)] for ra, rb in zip(after[1]["row_rescued"], before[1]["row_rescued"])] == want[2], offset
    finally:
        eng.bcrescue_end()


# ------------------------------------------------------------------------------------------------------- index shapes
def test_384_rows_of_two_variants(eng, tmp_path):
    case = bc.wide_index_case()
    for K in (1, 2):
        want = both_routes(eng, tmp_path, case, K)
        assert want[1]["ambiguous"] > 5 and want[1]["rescued1"] > 50


def test_the_largest_index_and_one_more(eng, tmp_path):
    from tagdigger_amd import TagdigError, tagdigger_fun as tf
    case = bc.full_index_case(0)
    assert bc.lds_bytes(case.barnum) <= bc.LDS_INDEX < bc.lds_bytes(case.barnum + 1)
    want = bc.ref_case(case, 2, min_distance=False)
    got = device_rescue(eng, case, 2)
    assert got[1].pop("min_entry_distance") == tf._bcrescue_min_distance(tf._bcrescue_entries(case.barcut, case.barnum))
    bc.check(got, want)
    assert want[1]["rescued1"] >= 5 and want[1]["rescued2"] >= 5
    with pytest.raises(TagdigError) as ei:
        begin(eng, bc.full_index_case(1), 2)
    assert ei.value.code == -7 and "LDS" in ei.value.detail
    with pytest.raises(TagdigError) as ei:
        eng.bcrescue_end()
    assert ei.value.code == -9


# ----------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def big():
    return bc.big_case()


_BIG_WANT = {}


def big_want(big, K=1, maxreads=5e9):
    """the restatement over the big library, computed once per (K, maxreads)"""
    if (K, maxreads) not in _BIG_WANT:
        _BIG_WANT[K, maxreads] = bc.ref_case(big, K, maxreads)
    return _BIG_WANT[K, maxreads]


@pytest.mark.parametrize("K", [1, 2])
def test_grid_caps_and_two_runs_identical(eng, big, K):
    want = big_want(big, K)
    assert want[1]["rescued1"] > 100 and want[1]["none"] > 50 and want[1]["tagged"] > 100
    try:
        got = []
        for cap in (0, 1, 2, 0):
            eng.set_option("max_grid", cap)
            got.append(device_rescue(eng, big, K))
            bc.check(got[-1], want)
        assert got[0] == got[3]
    finally:
        eng.set_option("max_grid", 0)


def test_pieces_that_begin_inside_a_record(eng, big):
    want = big_want(big, 2)
    lines = big.data.split(b"\r\n")
    for cut in (4 * 130 + 1, 4 * 301 + 2, 4 * 77 + 3):
        head = b"\r\n".join(lines[:cut]) + b"\r\n"
        bc.check(device_rescue(eng, big, 2, pieces=[(head, 0), (big.data[len(head):], cut)]), want)


def test_maxreads_and_the_three_file_formats(eng, big, tmp_path):
    plain = write(tmp_path, "m.fq", big.data)
    gz = write(tmp_path, "m2.fq.gz", gzip.compress(big.data))
    bg = write(tmp_path, "m.fq.gz", bgzf_bytes(big.data, block=1024))     # ~100 members: two GPU batches of 64
    eng.set_option("zb_members", 64)
    eng.set_option("stage_kb", 64)                                        # pieces of 64 KiB: maxreads falls inside one
    try:
        for maxreads in (1, 130, 391, 699, 5e9):
            want = big_want(big, 1, maxreads)
            assert want[1]["reads"] == min(maxreads, 700)
            bc.check(device_rescue(eng, big, 1, maxreads), want)
            for path in (plain, gz, bg):
                bc.check(file_rescue(eng, path, big, 1, maxreads), want)
    finally:
        eng.set_option("zb_members", 1 << 30)
        eng.set_option("stage_kb", 0)


def test_hot_cell(eng, tmp_path):
    """70 000 rescued reads on one cell, one row counter and one position"""
    rnd = random.Random(72)
    bodies, tags = bc.some_tags(rnd, 8, 50)
    one = bc.sub("ACGTTGCAG", 6) + bodies[3]
    two = bc.sub("ACGTTGCAG", 2) + bodies[5]
    begin_lists = bc.lists(["ACGT", "TGACA"], tags)

    def scaled(reads, n):
        """the restatement of one round of `reads`, n times over: the rule is per read"""
        m, st, rows, pos = bc.ref_lists(bc.fastq(reads, quality=False), *begin_lists, 1)
        return ([[n * x for x in r] for r in m], {k: v if k == "min_entry_distance" else n * v for k, v in st.items()},
                [[n * x for x in r] for r in rows], [n * x for x in pos])
    case = bc.Case(bc.fastq([one] * 70000, quality=False), *begin_lists)
    want = scaled([one], 70000)
    assert want[0][0][3] == 70000 and want[3][6] == 70000 and want[2][0] == [70000, 0]
    bc.check(device_rescue(eng, case), want)
    case = bc.Case(bc.fastq([one, two] * 35000, quality=False), *begin_lists)     # neighbouring lanes of every wave, two cells
    want = scaled([one, two], 35000)
    assert want[0][0][3] == want[0][0][5] == 35000
    bc.check(device_rescue(eng, case), want)
    bc.check(file_rescue(eng, write(tmp_path, "hot.fq", case.data), case), want)


def test_lifetime(eng, big):
    import numpy as np
    import tagdigger_amd
    from tagdigger_amd import TagdigError
    want = big_want(big)
    with pytest.raises(TagdigError) as ei:
        eng.bcrescue_end()                                                # end without begin
    assert ei.value.code == -9
    for call in (eng.bcrescue_stats, eng.bcrescue_fetch, eng.bcrescue_matrix, lambda: eng.bcrescue_device(0, 16)):
        with pytest.raises(TagdigError) as ei:
            call()
        assert ei.value.code == -9
    begin(eng, big, 1)
    run_pieces(eng, [(big.data, 0)])
    begin(eng, big, 1)                                                    # begin twice: the first is dropped, everything starts at zero
    got = fetched(eng)
    assert {k: got[1][k] for k in bc.CLASSES + ("tagged",)} == dict.fromkeys(bc.CLASSES + ("tagged",), 0) and not any(map(any, got[0]))
    run_pieces(eng, [(big.data, 0)])
    bc.check(fetched(eng), want)
    # the matrix where it lies
    raw = eng.d2h(eng.bcrescue_matrix(), 4 * big.barnum * len(big.stored))
    assert np.frombuffer(raw, dtype=np.uint32).reshape(big.barnum, len(big.stored)).tolist() == want[0]
    eng.bcrescue_end()
    # td_destroy with the state open
    other = tagdigger_amd.Engine(0)
    begin(other, big, 2)
    d = other.dev_alloc(len(big.data))
    other.h2d(d, big.data)
    other.bcrescue_device(d, len(big.data))
    other.sync()
    other.dev_free(d)
    other.close()


def test_census_qc_and_tag_rescue_on_the_same_handle(eng, big):
    """a census, a QC and a tag rescue interleaved with the barcode rescue: every one of them unchanged"""
    import rescue_cases as rc
    from census_cases import ordered, ref_census
    from qc_cases import STATS as QC_STATS, TABLES as QC_TABLES, ref_qc, same
    bars = bc.BARCODES_MIXED
    tags = ["TGCAG" + t for t in big.stored]
    want = big_want(big, 2)
    cwant = ref_census(big.data, bars, "TGCAG", 40)
    qwant = ref_qc(big.data, bars, "TGCAG", 160)
    rwant = rc.ref_rescue(big.data, bars, tags, K=1)
    eng.census_begin(bars, "TGCAG", 40, 4096)
    eng.qc_begin(bars, "TGCAG", 160)
    eng.rescue_begin(bars, tags, "TGCAG", 1)
    begin(eng, big, 2)
    try:
        d = eng.dev_alloc(len(big.data))
        try:
            eng.h2d(d, big.data)
            eng.census_device(d, len(big.data))
            eng.bcrescue_device(d, len(big.data))
            eng.qc_device(d, len(big.data))
            eng.rescue_device(d, len(big.data))
            eng.sync()
        finally:
            eng.dev_free(d)
        bc.check(fetched(eng), want)
        assert list(eng.census_fetch()) == ordered(cwant[0])
        qst = eng.qc_stats()
        same(dict(zip(QC_TABLES, eng.qc_fetch()), stats={k: qst[k] for k in QC_STATS}), qwant)
        rst = eng.rescue_stats()
        rm, rpos = eng.rescue_fetch()
        assert (rm.tolist(), {k: rst[k] for k in rc.CLASSES}, [int(x) for x in rpos]) == rwant[:3]
        bc.check(fetched(eng), want)
    finally:
        eng.census_end()
        eng.qc_end()
        eng.rescue_end()
        eng.bcrescue_end()


def test_find_tags_fastq_untouched(big, tmp_path):
    import rescue_cases as rc
    from tagdigger_amd import tagdigger_fun as tf
    tags = ["TGCAG" + t for t in big.stored]
    path = write(tmp_path, "u.fq", big.data)
    before = tf.find_tags_fastq(path, bc.BARCODES_MIXED, tags, progress=False)
    matrix, st = tf.rescue_barcodes_fastq(path, bc.BARCODES_MIXED, tags, max_mismatch=2)
    after = tf.find_tags_fastq(path, bc.BARCODES_MIXED, tags, progress=False)
    bc.check((matrix, st), big_want(big, 2))
    assert before == after == rc.ref_rescue(big.data, bc.BARCODES_MIXED, tags, K=1)[3]        # the exact reads are the counter's
    arr = tf.rescue_barcodes_fastq(path, bc.BARCODES_MIXED, tags, max_mismatch=2, as_array=True)[0]
    assert arr.dtype.name == "uint32" and arr.tolist() == matrix


def test_begin_errors_as_the_host_rule_names_them(eng, tmp_path):
    from tagdigger_amd import TagdigError, tagdigger_fun as tf
    for tags, bad in ((["AAAC", "GGGG", "AAAC"], 2), (["AAACT", "GGGG", "AAAC"], 2), (["CC", "AAACT", "GG", "AAACTT", "AAAC"], 3)):
        with pytest.raises(AssertionError) as ei:
            eng.bcrescue_begin(["ACGT"], ["TGCAG" + t for t in tags])
        assert str(ei.value) == "Problematic sequence: {}.  Likely due to overlapping tags.".format(bad)
    with pytest.raises(IndexError):
        eng.bcrescue_begin(["ACGT"], [])
    with pytest.raises(IndexError):
        eng.bcrescue_begin(["ACGT"], ["TGCAGAAAA", "TGCAG"])
    with pytest.raises(TagdigError) as ei:
        eng.bcrescue_begin(["ACGT"], ["TGCAG" + "A" * 129])
    assert ei.value.code == -7 and not ei.value.detail.startswith("barcode rescue: entry")
    with pytest.raises(TagdigError) as ei:
        eng._bcrescue_begin_lists(["ACGTTGCAG"], 1, [9], ["acgtacgt"], 1)
    assert ei.value.code == -6
    with pytest.raises(AssertionError) as ei:                                 # td_set_index's errors
        eng.bcrescue_begin(["ACGTTGCAGA", "ACGT"], ["TGCAGAAAA"])
    assert str(ei.value) == "Problematic sequence: 1.  Likely due to overlapping tags."
    for K in (0, 3):
        with pytest.raises(TagdigError) as ei:
            eng.bcrescue_begin(["ACGT"], ["TGCAGAAAA"], max_mismatch=K)
        assert ei.value.code == -2
    # every surviving entry longer than 2 K bases: TD_E_LIMIT, a ValueError through the Python function
    path = write(tmp_path, "e.fq", bc.fastq(["ACGTTGCAGACGTACGT"]))
    for K, barcodes, cutsite, ok in ((1, ["AC"], "", False), (1, ["ACG"], "", True), (2, ["AC"], "GT", False), (2, ["ACG"], "GT", True),
                                     (2, ["ACGTA", "T"], "GCA", False)):
        if ok:
            assert tf.rescue_barcodes_fastq(path, barcodes, ["AAAA"], cutsite=cutsite, max_mismatch=K)[1]["reads"] == 1
            continue
        with pytest.raises(TagdigError) as ei:
            eng.bcrescue_begin(barcodes, ["AAAA"], cutsite, K)
        assert ei.value.code == -7 and ei.value.detail.startswith("barcode rescue: entry")
        with pytest.raises(ValueError, match="^barcode rescue: entry"):
            tf.rescue_barcodes_fastq(path, barcodes, ["AAAA"], cutsite=cutsite, max_mismatch=K)
    with pytest.raises(TagdigError) as ei:
        eng.bcrescue_end()                                                # none of them left a state behind
    assert ei.value.code == -9


def test_nonascii_kills_the_pass_until_begin(eng):
    from tagdigger_amd import NonAsciiSequence
    tags = ["TGCAG" + "ACGTTGCATTGACCAGTTAC"]
    begin_lists = bc.lists(["ACGT"], tags)
    bad = bc.fastq(["ACGTAGCAGACGTTGCATTGACCAGTTAC"]) + b"@x\nACGTTGCAGAC\xe9TTGC\n+\nI\n"
    good = bc.fastq(["ACGTAGCAGACGTTGCATTGACCAGTTAC", "ACGTTGCAGACGTTGCATTGACCAGTTAC"])
    eng._bcrescue_begin_lists(*begin_lists, 1)
    try:
        run_pieces(eng, [(bad, 0)])
        for _ in range(2):
            with pytest.raises(NonAsciiSequence):
                eng.bcrescue_stats()
        with pytest.raises(NonAsciiSequence):
            run_pieces(eng, [(good, 0)])
        eng._bcrescue_begin_lists(*begin_lists, 1)
        run_pieces(eng, [(good, 0)])
        want = bc.ref_lists(good, *begin_lists, 1)
        assert want[1]["rescued1"] == 1 and want[1]["tagged"] == 1 and want[1]["exact"] == 1
        bc.check(fetched(eng), want)
    finally:
        eng.bcrescue_end()
