"""The tag census on the GPU (csrc/census.hip) against the census rule restated in tests/census_cases.py, through
td_census_device (a resident buffer) and td_census_file (the file readers)."""
import ctypes as C
import gzip
import os
import random

import pytest

from conftest import load_golden, write_case_file
from census_cases import BARCODES_MIXED, fastq, library, ordered, rand_seq, ref_census, ref_names
from helpers import bgzf_bytes
from oracle import tagdigger_oracle as orc

pytestmark = pytest.mark.gpu

CASES = [c for c in load_golden("hotpath_cases.json") + load_golden("hotpath_random.json") if not c.get("filename_override")]
STATS = ("reads", "barcut", "short", "ambiguous", "counted", "distinct")


@pytest.fixture(scope="module")
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    yield e
    e.close()


def device_census(eng, data, barcodes, cutsite, taglen, maxreads=5e9, slots=1024, pieces=None, first_line=0, min_count=1, top=None):
    """Through td_census_device: `pieces` = [(bytes, first_line), ...] of one begin, else the whole buffer."""
    eng.census_begin(barcodes, cutsite, taglen, slots)
    try:
        for part, fl in (pieces or [(data, first_line)]):
            if not part:
                continue
            d = eng.dev_alloc(len(part))
            try:
                eng.h2d(d, part)
                eng.census_device(d, len(part), fl, maxreads)
                eng.sync()
            finally:
                eng.dev_free(d)
        st = eng.census_stats()
        return list(eng.census_fetch(min_count, top)), st
    finally:
        eng.census_end()


def file_census(eng, path, barcodes, cutsite, taglen, maxreads=5e9, slots=1024):
    eng.census_begin(barcodes, cutsite, taglen, slots)
    try:
        eng.census_file(path, maxreads)
        st = eng.census_stats()
        return list(eng.census_fetch()), st
    finally:
        eng.census_end()


def check(got, want):
    (lists, st), (census, wst) = got, want
    assert lists == ordered(census)
    assert {k: st[k] for k in STATS} == {k: wst[k] for k in STATS}


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


# 1 ---------------------------------------------------------------------------------------------------------------
def test_golden_payloads(eng, tmp_path):
    from tagdigger_amd import NonAsciiSequence
    ran = 0
    for k, case in enumerate(CASES):
        kw = case["kwargs"]
        barcodes, cutsite, maxreads = case["barcodes"], kw.get("cutsite", "TGCAG"), kw.get("maxreads", 5e9)
        d = tmp_path / ("c%d" % k)
        d.mkdir()
        path = write_case_file(case, d)
        data = orc.read_fastq_bytes(path)
        for taglen in (8, 20):
            try:
                want = ref_census(data, barcodes, cutsite, taglen, maxreads)
            except (AssertionError, IndexError) as exc:
                with pytest.raises(type(exc)) as ei:
                    eng.census_begin(barcodes, cutsite, taglen, 1024)
                if isinstance(exc, AssertionError):
                    assert str(ei.value) == str(exc), case["name"]
                continue
            except orc.NonAsciiSequence:
                with pytest.raises(NonAsciiSequence):
                    device_census(eng, data, barcodes, cutsite, taglen, maxreads)
                with pytest.raises(NonAsciiSequence):
                    file_census(eng, path, barcodes, cutsite, taglen, maxreads)
                continue
            check(device_census(eng, data, barcodes, cutsite, taglen, maxreads), want)
            check(file_census(eng, path, barcodes, cutsite, taglen, maxreads), want)
            ran += 1
    assert ran > 150


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam_lib():
    rnd = random.Random(5)
    pool = [rand_seq(rnd, 160) for _ in range(40)]
    # tails that differ in the window's last bases only, for every seam
    pool += [pool[0][:k] + ("A" if pool[0][k] != "A" else "C") + pool[0][k + 1:] for k in (0, 25, 26, 27, 28, 57, 58, 59)]
    return fastq(library(rnd, 600, sites=("CAGC", "CTGC"), pool=pool, lo=60, hi=160))


@pytest.mark.parametrize("taglen", [1, 31, 32, 33, 63, 64])
def test_packing_seams_mixed_barcodes_degenerate_site(eng, seam_lib, taglen, tmp_path):
    want = ref_census(seam_lib, BARCODES_MIXED, "CWGC", taglen)
    assert want[1]["counted"] > 300 and (taglen < 4 or len({s[:4] for s in want[0]}) == 2)
    check(device_census(eng, seam_lib, BARCODES_MIXED, "CWGC", taglen), want)
    check(file_census(eng, write(tmp_path, "s.fq", seam_lib), BARCODES_MIXED, "CWGC", taglen), want)


# 3, 4, 10, 12 -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_lib():
    rnd = random.Random(7)
    pool = [rand_seq(rnd, 160) for _ in range(300)]
    data = fastq(library(rnd, 520, pool=pool), nl="\r\n")
    assert len(data) > 3 * 16384 + 100                           # more than three of the kernel's 16 KiB tiles
    return data


def test_several_tiles_and_two_runs_identical(eng, big_lib, tmp_path):
    want = ref_census(big_lib, BARCODES_MIXED, "TGCAG", 40)
    a = device_census(eng, big_lib, BARCODES_MIXED, "TGCAG", 40)
    b = device_census(eng, big_lib, BARCODES_MIXED, "TGCAG", 40)
    check(a, want)
    assert a == b
    path = write(tmp_path, "b.fq", big_lib)
    f = file_census(eng, path, BARCODES_MIXED, "TGCAG", 40)
    check(f, want)
    assert f == file_census(eng, path, BARCODES_MIXED, "TGCAG", 40)
    gz = write(tmp_path, "b.fq.gz", gzip.compress(big_lib))
    check(file_census(eng, gz, BARCODES_MIXED, "TGCAG", 40), want)


def test_two_calls_with_odd_first_line(eng, big_lib):
    want = ref_census(big_lib, BARCODES_MIXED, "TGCAG", 40)
    lines = big_lib.split(b"\r\n")
    for cut in (4 * 130 + 1, 4 * 201 + 2, 4 * 77 + 3):             # the second call starts inside a record
        head = b"\r\n".join(lines[:cut]) + b"\r\n"
        tail = big_lib[len(head):]
        check(device_census(eng, None, BARCODES_MIXED, "TGCAG", 40, pieces=[(head, 0), (tail, cut)]), want)


def test_maxreads_inside_buffer_and_inside_staged_piece(eng, big_lib, tmp_path):
    bg = write(tmp_path, "m.fq.gz", bgzf_bytes(big_lib, block=1024))     # ~100 members: two GPU batches of 64
    plain = write(tmp_path, "m.fq", big_lib)
    eng.set_option("zb_members", 64)
    try:
        for maxreads in (1, 130, 391, 519):
            want = ref_census(big_lib, BARCODES_MIXED, "TGCAG", 24, maxreads)
            assert want[1]["reads"] == maxreads
            check(device_census(eng, big_lib, BARCODES_MIXED, "TGCAG", 24, maxreads), want)
            check(file_census(eng, bg, BARCODES_MIXED, "TGCAG", 24, maxreads), want)
            check(file_census(eng, plain, BARCODES_MIXED, "TGCAG", 24, maxreads), want)
    finally:
        eng.set_option("zb_members", 1 << 30)


# 5, 6, 7 ---------------------------------------------------------------------------------------------------------
def both_routes(eng, data, taglen, tmp_path, slots, barcodes=("ACGT",)):
    want = ref_census(data, list(barcodes), "TGCAG", taglen)
    check(device_census(eng, data, list(barcodes), "TGCAG", taglen, slots=slots), want)
    check(file_census(eng, write(tmp_path, "r.fq", data), list(barcodes), "TGCAG", taglen, slots=slots), want)
    return want


def test_hot_slots_wave_combining(eng, tmp_path):
    rnd = random.Random(3)
    hot = [rand_seq(rnd, 70) for _ in range(3)]
    reads = ["ACGTTGCAG" + hot[0 if rnd.random() < 0.8 else rnd.randrange(3)] for _ in range(20000)]
    want = both_routes(eng, fastq(reads, quality=False), 64, tmp_path, 1024)
    assert want[1]["distinct"] == 3 and want[1]["counted"] == 20000


def test_all_distinct_racing_claims(eng, tmp_path):
    rnd = random.Random(4)
    reads = ["ACGTTGCAG%s" % rand_seq(rnd, 40) for _ in range(20000)]
    want = both_routes(eng, fastq(reads, quality=False), 45, tmp_path, 32768)          # load 0.61: long probe runs
    assert want[1]["distinct"] == 20000


def test_keys_differing_in_one_word_or_one_base(eng, tmp_path):
    rnd = random.Random(6)
    base = "TGCAG" + rand_seq(rnd, 59)
    flip = lambda s, k: s[:k] + ("A" if s[k] != "A" else "C") + s[k + 1:]
    variants = [base, flip(base, 63), flip(base, 5), flip(base, 31), flip(base, 32), flip(flip(base, 10), 20)]
    reads = ["ACGT" + variants[i % len(variants)] for i in range(6000)]               # interleaved read by read
    want = both_routes(eng, fastq(reads, quality=False), 64, tmp_path, 1024)
    assert want[1]["distinct"] == 6 and set(want[0].values()) == {1000}


# 8 ---------------------------------------------------------------------------------------------------------------
def test_exact_maximum_load_then_limit(eng):
    from tagdigger_amd import _binding as B
    from tagdigger_amd.engine import census_index, _c_strings
    L = B.load()
    rnd = random.Random(8)
    windows = set()
    while len(windows) < 769:
        windows.add(rand_seq(rnd, 20))
    windows = sorted(windows)
    full = fastq(["ACGTTGCAG" + w for w in windows[:768]] * 2, quality=False)
    got = device_census(eng, full, ["ACGT"], "TGCAG", 25, slots=1024)                 # 1024 slots take 768 keys: exactly full
    assert got[1]["max_keys"] == 768 and got[1]["distinct"] == 768
    check(got, ref_census(full, ["ACGT"], "TGCAG", 25))
    # one key more, through the C-ABI itself
    barcut, barnum, baroff = census_index(["ACGT"], "TGCAG")
    more = fastq(["ACGTTGCAG" + windows[768]], quality=False)

    def begin():
        assert L.td_census_begin(eng._h, _c_strings(barcut), len(barcut), barnum, (C.c_uint32 * 1)(*baroff), 25, 1024) == 0
    begin()
    try:
        for part in (full, more):
            d = eng.dev_alloc(len(part))
            try:
                eng.h2d(d, part)
                assert L.td_census_device(eng._h, C.c_void_p(d), len(part), 0, 2 ** 62, None) == 0
                eng.sync()
            finally:
                eng.dev_free(d)
        st = (C.c_uint64 * 8)()
        assert L.td_census_stats(eng._h, st) == -7
        msg = L.td_last_error().decode()
        assert "1024 slots" in msg and "768" in msg
        n = C.c_uint64(5)
        assert L.td_census_fetch(eng._h, 1, None, None, 0, C.byref(n)) == -7 and n.value == 0
        d = eng.dev_alloc(len(more))
        try:
            eng.h2d(d, more)
            assert L.td_census_device(eng._h, C.c_void_p(d), len(more), 0, 2 ** 62, None) == -7
        finally:
            eng.dev_free(d)
        begin()                                                                       # begun again: usable
        assert L.td_census_stats(eng._h, st) == 0 and st[5] == 0
    finally:
        assert L.td_census_end(eng._h) == 0


def test_exact_maximum_load_then_limit_through_the_file_route(eng, tmp_path):
    from tagdigger_amd import _binding as B
    from tagdigger_amd.engine import census_index, _c_strings
    L = B.load()
    rnd = random.Random(18)
    windows = set()
    while len(windows) < 769:
        windows.add(rand_seq(rnd, 20))
    windows = sorted(windows)
    full = fastq(["ACGTTGCAG" + w for w in windows[:768]] * 2, quality=False)
    got = file_census(eng, write(tmp_path, "full.fq", full), ["ACGT"], "TGCAG", 25, slots=1024)
    assert got[1]["distinct"] == got[1]["max_keys"] == 768
    check(got, ref_census(full, ["ACGT"], "TGCAG", 25))
    over = write(tmp_path, "over.fq", full + fastq(["ACGTTGCAG" + windows[768]], quality=False))
    barcut, barnum, baroff = census_index(["ACGT"], "TGCAG")
    assert L.td_census_begin(eng._h, _c_strings(barcut), len(barcut), barnum, (C.c_uint32 * 1)(*baroff), 25, 1024) == 0
    try:
        assert L.td_census_file(eng._h, over.encode(), 2 ** 62) == -7
        msg = L.td_last_error().decode()
        assert msg.startswith("census table full") and "1024 slots" in msg and "768" in msg
        n = C.c_uint64(5)
        assert L.td_census_fetch(eng._h, 1, None, None, 0, C.byref(n)) == -7 and n.value == 0
        st = (C.c_uint64 * 8)()
        assert L.td_census_stats(eng._h, st) == -7
        assert L.td_census_file(eng._h, over.encode(), 2 ** 62) == -7
        assert L.td_census_begin(eng._h, _c_strings(barcut), len(barcut), barnum, (C.c_uint32 * 1)(*baroff), 25, 4096) == 0
        assert L.td_census_file(eng._h, over.encode(), 2 ** 62) == 0
        assert L.td_census_stats(eng._h, st) == 0 and st[5] == 769
    finally:
        assert L.td_census_end(eng._h) == 0


def test_nonascii_through_the_file_route_latches_until_begin(eng, tmp_path):
    from tagdigger_amd import _binding as B
    from tagdigger_amd.engine import census_index, _c_strings
    L = B.load()
    good = fastq(["ACGTTGCAG" + "ACGTTGCATTGACCAGTTAC"])
    bad = write(tmp_path, "bad.fq", good + b"@x\nACGTTGCAGAC\xe9TTGCATTGACCAGTTAC\n+\nI\n")
    barcut, barnum, baroff = census_index(["ACGT"], "TGCAG")

    def begin():
        assert L.td_census_begin(eng._h, _c_strings(barcut), len(barcut), barnum, (C.c_uint32 * 1)(*baroff), 20, 1024) == 0
    begin()
    try:
        assert L.td_census_file(eng._h, bad.encode(), 2 ** 62) == -8                  # TD_E_NONASCII
        msg = L.td_last_error()
        st = (C.c_uint64 * 8)()
        for _ in range(2):
            assert L.td_census_stats(eng._h, st) == -8 and L.td_last_error() == msg
        n = C.c_uint64(5)
        assert L.td_census_fetch(eng._h, 1, None, None, 0, C.byref(n)) == -8 and n.value == 0 and L.td_last_error() == msg
        assert L.td_census_file(eng._h, write(tmp_path, "good.fq", good).encode(), 2 ** 62) == -8 and L.td_last_error() == msg
        begin()                                                                       # begun again: usable
        assert L.td_census_file(eng._h, write(tmp_path, "good.fq", good).encode(), 2 ** 62) == 0
        assert L.td_census_stats(eng._h, st) == 0 and list(st[:6]) == [1, 1, 0, 0, 1, 1]
    finally:
        assert L.td_census_end(eng._h) == 0


def test_fetch_without_a_census_is_a_state_error(eng):
    from tagdigger_amd import TagdigError
    with pytest.raises(TagdigError) as ei:
        eng.census_fetch()
    assert ei.value.code == -9


# 5, 6 once more with every window going to the table by itself: lanes of one wave race for the same empty slot
def test_uncombined_hot_and_distinct(eng, tmp_path, monkeypatch):
    monkeypatch.setenv("TAGDIG_CENSUS_COMBINE", "0")           # (read at td_census_begin)
    rnd = random.Random(13)
    hot = [rand_seq(rnd, 70) for _ in range(3)]
    reads = ["ACGTTGCAG" + hot[0 if rnd.random() < 0.8 else rnd.randrange(3)] for _ in range(20000)]
    want = both_routes(eng, fastq(reads, quality=False), 64, tmp_path, 1024)
    assert want[1]["distinct"] == 3 and want[1]["counted"] == 20000
    reads = ["ACGTTGCAG%s" % rand_seq(rnd, 40) for _ in range(10000)]
    reads = [r for pair in zip(reads, reads) for r in pair]         # every window twice, side by side: the same wave claims and adds
    want = both_routes(eng, fastq(reads, quality=False), 45, tmp_path, 16384)
    assert want[1]["distinct"] == 10000 and set(want[0].values()) == {2}


# 9 ---------------------------------------------------------------------------------------------------------------
def test_tag_census_grows_from_the_smallest_table(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    rnd = random.Random(9)
    reads = ["ACGTTGCAG" + rand_seq(rnd, 30) for _ in range(5000)]
    data = fastq(reads + reads[:100], quality=False)
    path = write(tmp_path, "g.fq", data)
    want, st = ref_census(data, ["ACGT"], "TGCAG", 30)
    assert st["distinct"] == 5000
    got = tf.tag_census(path, ["ACGT"], taglen=30, slots=tf.CENSUS_MIN_SLOTS)
    assert list(got) == ordered(want) and got.stats == {k: st[k] for k in STATS}
    with pytest.raises(Exception) as ei:                        # the stated memory bound holds
        tf.tag_census(path, ["ACGT"], taglen=30, slots=tf.CENSUS_MIN_SLOTS, max_table_bytes=4096 * 16)
    assert "census table full" in str(ei.value)
    assert list(tf.tag_census(path, ["ACGT"], taglen=30, min_count=2, top=50)) == ordered(want, 2, 50)


# 11 --------------------------------------------------------------------------------------------------------------
def test_cross_check_with_the_counter(eng, tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    rnd = random.Random(10)
    tags = [rand_seq(rnd, rnd.randint(20, 50)) for _ in range(30)]
    names = ["M%d_%d" % (i // 2, i % 2) for i in range(30)]
    names, tags = tf.sanitizeTags([names, ["TGCAG" + t for t in tags]])
    pool = [t[5:] + rand_seq(rnd, 120) for t in tags] + [rand_seq(rnd, 170) for _ in range(30)]
    reads = library(rnd, 3000, pool=pool, lo=120, hi=160, dirt=False)
    path = write(tmp_path, "x.fq", fastq(reads))
    eng.set_index(BARCODES_MIXED, tags, "TGCAG")
    eng.count_file(path)
    cst = eng.stats()
    got = tf.tag_census(path, BARCODES_MIXED, taglen=64, known=[names, tags])
    assert max(len(t) for t in tags) <= 64
    assert got.stats["barcut"] == cst["barcut"] and got.stats["short"] == 0 and got.stats["ambiguous"] == 0
    assert sum(c for c, n in zip(got[1], got[2]) if n) == cst["tag"] > 0
    assert got[2] == ref_names(got[0], [names, tags], "TGCAG")
