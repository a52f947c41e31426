"""library_qc without a GPU (backend="host"), its writers and command line against the QC rule restated in
tests/qc_cases.py: exact equality of every table and every total."""
import csv
import gzip
import io
import random

import numpy as np
import pytest

from conftest import load_golden, write_case_file
from qc_cases import BARCODES, check_invariants, library, named_inputs, records, ref_cached, ref_qc, same
from oracle import tagdigger_oracle as orc

CASES = [c for c in load_golden("hotpath_cases.json") + load_golden("hotpath_random.json") if not c.get("filename_override")]


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


@pytest.mark.parametrize("C", [8, 200])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_golden_payloads_host(case, C, tmp_path):
    from tagdigger_amd import NonAsciiSequence, tagdigger_fun as tf
    path = write_case_file(case, tmp_path)
    kw = case["kwargs"]
    barcodes, cutsite, maxreads = case["barcodes"], kw.get("cutsite", "TGCAG"), kw.get("maxreads", 5e9)
    run = lambda: tf.library_qc(path, barcodes, cutsite, C, maxreads, backend="host")
    try:
        want = ref_qc(orc.read_fastq_bytes(path), barcodes, cutsite, C, maxreads)
    except (AssertionError, IndexError) as exc:
        with pytest.raises(type(exc)) as ei:
            run()
        if isinstance(exc, AssertionError):
            assert str(ei.value) == str(exc)
        return
    except orc.NonAsciiSequence:
        with pytest.raises(NonAsciiSequence):
            run()
        return
    got = run()
    same(got, want)
    check_invariants(got)


@pytest.mark.parametrize("name", sorted(named_inputs()))
def test_edge_inputs_host(name, tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    data, C = named_inputs()[name]
    want = ref_cached(name, data, BARCODES, "TGCAG", C)
    check_invariants(want)
    got = tf.library_qc(write(tmp_path, "e.fq", data), BARCODES, max_cycles=C, backend="host")
    same(got, want)
    check_invariants(got)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    rnd = random.Random(41)
    data = records(library(rnd, 300), nl=b"\r\n")
    d = tmp_path_factory.mktemp("qc")
    plain, gz = str(d / "lib.fq"), str(d / "lib.fq.gz")
    with open(plain, "wb") as fh:
        fh.write(data)
    with gzip.open(gz, "wb") as fh:
        fh.write(data)
    return data, plain, gz


def test_maxreads_inside_file_and_gz(lib):
    from tagdigger_amd import tagdigger_fun as tf
    data, plain, gz = lib
    for maxreads in (1, 57, 57.5, 299, 300, 5e9):
        want = ref_qc(data, BARCODES, "TGCAG", 100, maxreads)
        assert want["stats"]["qual_lines"] == want["stats"]["reads"] == min(300, -int(-maxreads // 1))
        for path in (plain, gz):
            same(tf.library_qc(path, BARCODES, max_cycles=100, maxreads=maxreads, backend="host"), want)


def quantile_table(rows):
    from tagdigger_amd import tagdigger_fun as tf
    qual = np.zeros((len(rows), 95), dtype=np.uint64)
    for i, row in enumerate(rows):
        for v, c in row.items():
            qual[i, v] = c
    return tf.QCResult({}, None, None, qual, None, None, len(rows) - 1)


def test_quantile_rule_at_its_knife_edges():
    res = quantile_table([{}, {7: 1}, {10: 1, 20: 1, 30: 1, 40: 1}, {5: 3, 6: 1}, {0: 1, 93: 99}, {94: 5}, {2: 10}])
    # empty; n = 1; p * n reached exactly; ties; the two ends of the scale; invalid bytes only; one value
    assert res.cycle_quantiles(50) == [None, 7, 20, 5, 93, None, 2]
    assert res.cycle_quantiles(25) == [None, 7, 10, 5, 93, None, 2]
    assert res.cycle_quantiles(26) == [None, 7, 20, 5, 93, None, 2]
    assert res.cycle_quantiles(75) == [None, 7, 30, 5, 93, None, 2]
    assert res.cycle_quantiles(76) == [None, 7, 40, 6, 93, None, 2]
    assert res.cycle_quantiles(1) == [None, 7, 10, 5, 0, None, 2]
    assert res.cycle_quantiles(2) == [None, 7, 10, 5, 93, None, 2]
    assert res.cycle_quantiles(100) == [None, 7, 40, 6, 93, None, 2]
    assert res.cycle_means_x100() == [None, 700, 2500, 525, 9207, None, 200]


SMALL = records([(b"ACGTTGCAGAC", b"IIIIIIIII5#"), (b"TGACATGCAGNA", b"I5I5"), (b"GGGGGG", b"\x01\x80"), (b"acgttgcagt", b"")])

WANT_SAMPLES = (
    "Library,Barcode,Sample,Reads,Reads ppm of library,Bases,Reads with non-ACGT\r\n"
    "L,ACGT,s0,2,500000,21,0\r\n"
    "L,TGACA,s1,1,250000,12,1\r\n"
    "L,(none),(none),1,250000,6,0\r\n")
WANT_CYCLES = (
    "Library,Cycle,A,C,G,T,N,Other,Quality values,Invalid quality bytes,Mean quality,Q10,Q25,Q50,Q75,Q90\r\n"
    "L,1,2,0,1,1,0,0,2,1,40.00,40,40,40,40,40\r\n"
    "L,2,0,2,2,0,0,0,2,1,30.00,20,20,20,40,40\r\n"
    "L,3,1,0,3,0,0,0,2,0,40.00,40,40,40,40,40\r\n"
    "L,>3,6,5,9,6,1,0,9,0,31.33,2,20,40,40,40\r\n")
WANT_LENGTHS = "Library,Length,Reads\r\nL,0,0\r\nL,1,0\r\nL,2,0\r\nL,>=3,4\r\n"


def test_writers_pinned(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    path = write(tmp_path, "small.fq", SMALL)
    res = tf.library_qc(path, ["ACGT", "TGACA"], max_cycles=3, backend="host")
    same(res, ref_qc(SMALL, ["ACGT", "TGACA"], "TGCAG", 3))
    assert res.stats == dict(reads=4, barcut=3, qual_lines=4, bases=39, qual_bases=15, qual_invalid=2, empty_qual=2)
    out = [str(tmp_path / n) for n in ("s.csv", "c.csv", "l.csv", "q.csv")]
    tf.writeQCSamples(out[0], ["L"], [res], [["ACGT", "TGACA"]], [["s0", "s1"]])
    tf.writeQCCycles(out[1], ["L"], [res])
    tf.writeQCLengths(out[2], ["L"], [res])
    tf.writeQCQualityMatrix(out[3], ["L"], [res])
    read = lambda p: open(p, "rb").read().decode()
    assert read(out[0]) == WANT_SAMPLES
    assert read(out[1]) == WANT_CYCLES
    assert read(out[2]) == WANT_LENGTHS
    rows = list(csv.reader(io.StringIO(read(out[3]), newline="")))
    assert rows[0] == ["Library", "Cycle"] + ["Q%d" % v for v in range(94)] + ["Invalid"] and len(rows) == 5
    assert [r[:2] for r in rows[1:]] == [["L", "1"], ["L", "2"], ["L", "3"], ["L", ">3"]]
    assert [[int(x) for x in r[2:]] for r in rows[1:]] == res.qual_cycle.tolist()


def test_cli_two_libraries(lib, tmp_path, capsys):
    from tagdigger_amd import tag_qc, tagdigger_fun as tf
    data, plain, gz = lib
    other = records(library(random.Random(42), 50, barcodes=BARCODES[:2]))
    second = write(tmp_path, "second.fq", other)
    key = str(tmp_path / "key.csv")
    with open(key, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["File", "Barcode", "Sample"])
        for i, b in enumerate(BARCODES):
            w.writerow([gz, b, "s%d" % i])
        for i, b in enumerate(BARCODES[:2]):
            w.writerow([second, b, "t%d" % i])
    prefix = str(tmp_path / "out")
    assert tag_qc.main(["-f", gz, "-f", second, "-b", key, "-e", "PstI", "-o", prefix, "--max-cycles", "40", "--quality-matrix",
                        "--td-backend", "host"]) == 0
    wants = [ref_qc(data, BARCODES, "TGCAG", 40), ref_qc(other, BARCODES[:2], "TGCAG", 40)]
    rows = list(csv.reader(open(prefix + "_samples.csv", newline="")))
    assert len(rows) == 1 + 7 + 3
    assert [r[:3] for r in rows[1:8]] == [[gz, b, "s%d" % i] for i, b in enumerate(BARCODES)] + [[gz, "(none)", "(none)"]]
    assert [[int(r[3]), int(r[5]), int(r[6])] for r in rows[1:8]] == wants[0]["barcodes"].tolist()
    assert [[int(r[3]), int(r[5]), int(r[6])] for r in rows[8:]] == wants[1]["barcodes"].tolist()
    assert [int(r[4]) for r in rows[8:]] == [int(x) * 1000000 // 50 for x in wants[1]["barcodes"][:, 0]]
    cyc = list(csv.reader(open(prefix + "_cycles.csv", newline="")))
    assert len(cyc) == 1 + 2 * 41 and cyc[41][1] == ">40" and cyc[42][:2] == [second, "1"]
    assert [[int(x) for x in r[2:8]] for r in cyc[1:42]] == wants[0]["base_cycle"].tolist()
    mat = list(csv.reader(open(prefix + "_quality.csv", newline="")))
    assert [[int(x) for x in r[2:]] for r in mat[42:]] == wants[1]["qual_cycle"].tolist()
    lens = list(csv.reader(open(prefix + "_lengths.csv", newline="")))
    assert [int(r[2]) for r in lens[1:42]] == wants[0]["lengths"].tolist() and lens[41][1] == ">=40"
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2
    for line, f, want in zip(lines, (gz, second), wants):
        st = want["stats"]
        assert line.startswith("%s: Reads: %d With barcode and cut site: %d Bases: %d Quality lines: %d Mean quality: " % (
            f, st["reads"], st["barcut"], st["bases"], st["qual_lines"]))
        assert line.endswith(" Invalid quality bytes: %d" % st["qual_invalid"])
    # without --quality-matrix the fourth file is not written
    assert tag_qc.main(["-f", second, "-b", key, "-c", "TGCAG", "-o", prefix + "2", "--td-backend", "host"]) == 0
    import os
    assert os.path.exists(prefix + "2_cycles.csv") and not os.path.exists(prefix + "2_quality.csv")
    assert tf.QC_MAX_CYCLES == 1024


def test_argument_errors(lib):
    from tagdigger_amd import tag_qc, tagdigger_fun as tf
    _, plain, _ = lib
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError):
            tf.library_qc(plain, BARCODES, max_cycles=bad, backend="host")
    with pytest.raises(AssertionError) as ei:
        tf.library_qc(plain, ["ACGN"], backend="host")
    assert str(ei.value) == "Non-ACGT barcode."
    with pytest.raises(AssertionError) as ei:
        tf.library_qc(plain, ["ACGT"], cutsite="TGCAX", backend="host")
    assert str(ei.value) == "Invalid cut site."
    with pytest.raises(AssertionError) as ei:
        tf.library_qc(plain, ["ACGTT", "ACGT"], cutsite="", backend="host")         # (a later member ends inside an earlier one)
    assert str(ei.value) == "Problematic sequence: 1.  Likely due to overlapping tags."
    with pytest.raises(ValueError):
        tf.library_qc(plain, ["ACGT"], backend="cpu")
    with pytest.raises(SystemExit):
        tag_qc.main(["-b", "k.csv", "-e", "PstI", "-o", "x"])             # no library


def test_truncated_gz_raises_before_the_bound_only(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    rnd = random.Random(43)
    data = records(library(rnd, 3000, lo=100, hi=150))
    whole = gzip.compress(data)
    path = write(tmp_path, "cut.fq.gz", whole[:len(whole) // 2])
    with pytest.raises(EOFError):
        tf.library_qc(path, BARCODES, backend="host")
    with pytest.raises(EOFError):
        tf.library_qc(path, BARCODES, maxreads=2900, backend="host")
    got = tf.library_qc(path, BARCODES, maxreads=20, backend="host")       # the loop ends long before the damage
    same(got, ref_qc(data, BARCODES, "TGCAG", 160, 20))
