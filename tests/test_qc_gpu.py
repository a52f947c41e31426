"""The library QC on the GPU (csrc/qc.hip) against the QC rule restated in tests/qc_cases.py, through td_qc_device (a
resident buffer) and td_qc_file (the file readers): exact equality of every table and every total."""
import ctypes as C
import gzip
import random

import numpy as np
import pytest

from conftest import load_golden, write_case_file
from qc_cases import (BARCODES, STATS, TABLES, check_invariants, library, named_inputs, plus, rand_qual, rand_seq, records, ref_cached,
                      ref_qc, same, times)
from helpers import bgzf_bytes
from oracle import tagdigger_oracle as orc

pytestmark = pytest.mark.gpu

CASES = [c for c in load_golden("hotpath_cases.json") + load_golden("hotpath_random.json") if not c.get("filename_override")]


@pytest.fixture(scope="module")
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    yield e
    e.close()


def fetch(eng):
    st = eng.qc_stats()
    out = dict(zip(TABLES, eng.qc_fetch()))
    out["stats"] = {k: st[k] for k in STATS}
    return out


def device_qc(eng, data, barcodes, cutsite="TGCAG", cycles=160, maxreads=5e9, pieces=None):
    """Through td_qc_device: `pieces` = [(bytes, first_line), ...] of one begin, else the whole buffer."""
    eng.qc_begin(barcodes, cutsite, cycles)
    try:
        for part, fl in (pieces or [(data, 0)]):
            if not part:
                continue
            d = eng.dev_alloc(len(part))
            try:
                eng.h2d(d, part)
                eng.qc_device(d, len(part), fl, maxreads)
                eng.sync()
            finally:
                eng.dev_free(d)
        return fetch(eng)
    finally:
        eng.qc_end()


def file_qc(eng, path, barcodes, cutsite="TGCAG", cycles=160, maxreads=5e9):
    eng.qc_begin(barcodes, cutsite, cycles)
    try:
        eng.qc_file(path, maxreads)
        return fetch(eng)
    finally:
        eng.qc_end()


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
        for cycles in (8, 200):
            try:
                want = ref_qc(data, barcodes, cutsite, cycles, maxreads)
            except (AssertionError, IndexError) as exc:
                with pytest.raises(type(exc)) as ei:
                    eng.qc_begin(barcodes, cutsite, cycles)
                if isinstance(exc, AssertionError):
                    assert str(ei.value) == str(exc), case["name"]
                continue
            except orc.NonAsciiSequence:
                with pytest.raises(NonAsciiSequence):
                    device_qc(eng, data, barcodes, cutsite, cycles, maxreads)
                with pytest.raises(NonAsciiSequence):
                    file_qc(eng, path, barcodes, cutsite, cycles, maxreads)
                continue
            same(device_qc(eng, data, barcodes, cutsite, cycles, maxreads), want)
            same(file_qc(eng, path, barcodes, cutsite, cycles, maxreads), want)
            ran += 1
    assert ran > 150


# 2, 3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(named_inputs()))
def test_edge_inputs(eng, name, tmp_path):
    """Line lengths around every chunk, step and row boundary and one of 40 000 bytes; every byte value in quality
    lines; every strip byte at both ends; lines that start on, before and behind a tile seam with each terminator;
    files whose last record is incomplete."""
    data, cycles = named_inputs()[name]
    want = ref_cached(name, data, BARCODES, "TGCAG", cycles)
    got = device_qc(eng, data, BARCODES, cycles=cycles)
    same(got, want)
    check_invariants(got)
    same(file_qc(eng, write(tmp_path, "e.fq", data), BARCODES, cycles=cycles), want)


@pytest.fixture(scope="module")
def big_lib():
    rnd = random.Random(51)
    data = records(library(rnd, 520), nl=b"\r\n")
    assert len(data) > 3 * 16384 + 100
    return data, ref_qc(data, BARCODES, "TGCAG", 160)


def test_two_runs_identical_and_gz(eng, big_lib, tmp_path):
    data, want = big_lib
    a = device_qc(eng, data, BARCODES)
    b = device_qc(eng, data, BARCODES)
    same(a, want)
    same(b, a)
    same(file_qc(eng, write(tmp_path, "b.fq.gz", gzip.compress(data)), BARCODES), want)


# 4 ---------------------------------------------------------------------------------------------------------------
def test_pieces_that_start_inside_a_record(eng, big_lib):
    data, want = big_lib
    lines = data.split(b"\r\n")
    for cut in (4 * 130 + 1, 4 * 201 + 2, 4 * 77 + 3):
        head = b"\r\n".join(lines[:cut]) + b"\r\n"
        same(device_qc(eng, None, BARCODES, pieces=[(head, 0), (data[len(head):], cut)]), want)
    # a cut between the sequence and the quality line of record R - 1, with max_reads = R
    R = 300
    want_r = ref_qc(data, BARCODES, "TGCAG", 160, R)
    assert want_r["stats"]["reads"] == want_r["stats"]["qual_lines"] == R
    for cut in (4 * (R - 1) + 2, 4 * (R - 1) + 3):
        head = b"\r\n".join(lines[:cut]) + b"\r\n"
        got = device_qc(eng, None, BARCODES, maxreads=R, pieces=[(head, 0), (data[len(head):], cut)])
        assert got["stats"]["qual_lines"] == R
        same(got, want_r)


# 5 ---------------------------------------------------------------------------------------------------------------
def test_maxreads_inside_buffer_and_files(eng, big_lib, tmp_path):
    data, _ = big_lib
    bg = write(tmp_path, "m.fq.gz", bgzf_bytes(data, block=1024))          # ~100 members: two GPU batches of 64
    plain = write(tmp_path, "m.fq", data)
    gz = write(tmp_path, "g.fq.gz", gzip.compress(data))
    eng.set_option("zb_members", 64)
    try:
        for maxreads in (1, 130, 391, 519, 520):
            want = ref_qc(data, BARCODES, "TGCAG", 160, maxreads)
            assert want["stats"]["reads"] == want["stats"]["qual_lines"] == maxreads
            same(device_qc(eng, data, BARCODES, maxreads=maxreads), want)
            for path in (bg, plain, gz):
                same(file_qc(eng, path, BARCODES, maxreads=maxreads), want)
    finally:
        eng.set_option("zb_members", 1 << 30)


def test_bound_sweeps_across_the_record_in_which_the_first_piece_ends(eng, tmp_path):
    rnd = random.Random(52)
    pairs = [((rnd.choice(BARCODES) + "TGCAG" + rand_seq(rnd, 200))[:100].encode(), rand_qual(rnd, 100).encode()) for _ in range(700)]
    data = b"".join(b"@r%05d\n" % i + s + b"\n+\n" + q + b"\n" for i, (s, q) in enumerate(pairs))        # 211 bytes a record
    assert len(data) > 2 * 65536
    path = write(tmp_path, "s.fq", data)
    at = 65536 // 211                                                       # the record in which the first 64 KiB piece ends
    eng.set_option("stage_kb", 64)
    try:
        for R in range(at - 2, at + 4):
            want = ref_qc(data, BARCODES, "TGCAG", 160, R)
            assert want["stats"]["qual_lines"] == R
            same(file_qc(eng, path, BARCODES, maxreads=R), want)
    finally:
        eng.set_option("stage_kb", 0)


# 6 ---------------------------------------------------------------------------------------------------------------
def test_merge_settings_give_the_same_result(eng, big_lib):
    data, want = big_lib
    for opts in ({"qc_flush_tiles": 1}, {"max_grid": 1}, {"qc_flush_tiles": 1, "max_grid": 1}, {"qc_flush_tiles": 2, "max_grid": 2}):
        for k, v in opts.items():
            eng.set_option(k, v)
        try:
            same(device_qc(eng, data, BARCODES), want)
        finally:
            for k in opts:
                eng.set_option(k, 0)


def test_70000_identical_reads_in_one_workgroup(eng):
    """Every read adds to the same cells, and one workgroup takes them all: a cell passes 65 535 between two merges."""
    rec = records([(b"ACGTTGCAGACGTNACGT", b"IIIIIIIIIIIIIIIII#")])
    want = times(ref_qc(rec, BARCODES, "TGCAG", 12), 70000)
    assert int(want["qual_cycle"][0, 40]) == 70000 and int(want["base_cycle"][12].sum()) == 6 * 70000
    eng.set_option("max_grid", 1)
    try:
        same(device_qc(eng, rec * 70000, BARCODES, cycles=12), want)
    finally:
        eng.set_option("max_grid", 0)
    same(device_qc(eng, rec * 70000, BARCODES, cycles=12), want)


def test_reads_all_longer_than_the_lds_window(eng, tmp_path):
    rnd = random.Random(53)
    pairs = [((rnd.choice(BARCODES) + "TGCAG" + rand_seq(rnd, 400))[:rnd.randint(200, 330)].encode(), rand_qual(rnd, rnd.randint(200, 330)).encode())
             for _ in range(300)]
    data = records(pairs)
    for cycles in (1024, 300, 153):
        want = ref_qc(data, BARCODES, "TGCAG", cycles)
        same(device_qc(eng, data, BARCODES, cycles=cycles), want)
    same(file_qc(eng, write(tmp_path, "l.fq", data), BARCODES, cycles=1024), ref_qc(data, BARCODES, "TGCAG", 1024))


def test_more_barcodes_than_the_lds_rows(eng):
    rnd = random.Random(54)
    barcodes = []
    while len(barcodes) < 600:                                   # 600 barcodes of one length: prefix-free
        b = rand_seq(rnd, 8)
        if b not in barcodes:
            barcodes.append(b)
    pairs = [((rnd.choice(barcodes) + "TGCAG" + rand_seq(rnd, 60)).encode(), rand_qual(rnd, 73).encode()) for _ in range(1500)]
    data = records(pairs)
    same(device_qc(eng, data, barcodes), ref_qc(data, barcodes, "TGCAG", 160))
    same(device_qc(eng, data, barcodes[:384]), ref_qc(data, barcodes[:384], "TGCAG", 160))      # rows in LDS, a narrower window


# 7 ---------------------------------------------------------------------------------------------------------------
def test_accumulation_and_begin_again(eng, big_lib, tmp_path):
    data, want = big_lib
    other = records(library(random.Random(55), 100))
    a, b = write(tmp_path, "a.fq", data), write(tmp_path, "b.fq.gz", gzip.compress(other))
    eng.qc_begin(BARCODES, "TGCAG", 160)
    try:
        eng.qc_file(a)
        eng.qc_file(b)
        same(fetch(eng), plus(want, ref_qc(other, BARCODES, "TGCAG", 160)))
        eng.qc_begin(BARCODES, "TGCAG", 160)                                    # begun again: zeroed
        got = fetch(eng)
        assert not any(got["stats"].values()) and not any(int(got[t].sum()) for t in TABLES)
        eng.qc_file(a)
        same(fetch(eng), want)
    finally:
        eng.qc_end()


def test_state_errors_through_the_c_abi(eng, tmp_path):
    from tagdigger_amd import _binding as B
    from tagdigger_amd.engine import census_index, _c_strings
    L = B.load()
    st = (C.c_uint64 * 8)()
    assert L.td_qc_stats(eng._h, st) == -9                                      # no begin
    assert L.td_qc_fetch(eng._h, None, None, None, None, None) == -9
    assert L.td_qc_file(eng._h, b"x.fq", 5) == -9
    assert L.td_qc_device(eng._h, None, 0, 0, 5, None) == -9
    barcut, barnum, baroff = census_index(["ACGT"], "TGCAG")
    begin = lambda cyc=50: L.td_qc_begin(eng._h, _c_strings(barcut), len(barcut), barnum, (C.c_uint32 * 1)(*baroff), cyc)
    assert begin(0) == -2 and begin(1025) == -2
    assert begin() == 0
    try:
        bad = records([(b"ACGTTGCAGAC", b"IIIII"), (b"ACGTTG\xe9AGAC", b"IIIII")])
        good = records([(b"ACGTTGCAGAC", b"II\xe9II")])                          # a byte >= 0x80 in a quality line is no error
        d = eng.dev_alloc(len(bad))
        try:
            eng.h2d(d, good)
            assert L.td_qc_device(eng._h, C.c_void_p(d), len(good), 0, 2 ** 62, None) == 0
            assert L.td_qc_stats(eng._h, st) == 0 and st[0] == 1 and st[5] == 1
            eng.h2d(d, bad)
            assert L.td_qc_device(eng._h, C.c_void_p(d), len(bad), 0, 2 ** 62, None) == 0
            assert L.td_qc_stats(eng._h, st) == -8
            assert L.td_qc_fetch(eng._h, None, None, None, None, None) == -8
            assert L.td_qc_device(eng._h, C.c_void_p(d), len(bad), 0, 2 ** 62, None) == -8
            assert L.td_qc_file(eng._h, write(tmp_path, "g.fq", good).encode(), 2 ** 62) == -8
        finally:
            eng.dev_free(d)
        assert begin() == 0                                                     # begun again: usable
        assert L.td_qc_stats(eng._h, st) == 0 and st[0] == 0 and st[7] == 50
        # a file that fails part-way: the tables are never handed out
        assert L.td_qc_file(eng._h, write(tmp_path, "bad.fq", good * 3 + bad).encode(), 2 ** 62) == -8
        assert L.td_qc_stats(eng._h, st) == -8
    finally:
        assert L.td_qc_end(eng._h) == 0
    assert L.td_qc_stats(eng._h, st) == -9


# 8 ---------------------------------------------------------------------------------------------------------------
def test_cross_check_with_the_counter_and_library_qc(eng, big_lib, tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    data, want = big_lib
    path = write(tmp_path, "x.fq", data)
    eng.set_index(BARCODES, ["TGCAGAAAA"], "TGCAG")
    eng.count_file(path)
    cst = eng.stats()
    got = tf.library_qc(path, BARCODES)
    same(got, want)
    assert got.stats["reads"] == cst["reads"]
    assert got.stats["barcut"] == cst["barcut"] == int(got.barcodes[:-1, 0].sum())
    same(tf.library_qc(path, BARCODES, backend="host"), want)
