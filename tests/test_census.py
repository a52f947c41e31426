"""tag_census without a GPU (backend="host") against the census rule restated in tests/census_cases.py."""
import csv
import gzip
import io
import random

import pytest

from conftest import load_golden, write_case_file
from census_cases import BARCODES_MIXED, fastq, library, ordered, rand_seq, ref_census, ref_names
from oracle import tagdigger_oracle as orc

CASES = [c for c in load_golden("hotpath_cases.json") + load_golden("hotpath_random.json") if not c.get("filename_override")]
STATS = ("reads", "barcut", "short", "ambiguous", "counted", "distinct")


def case_args(case):
    kw = case["kwargs"]
    return case["barcodes"], kw.get("cutsite", "TGCAG"), kw.get("maxreads", 5e9)


def expect_or_raise(fn_ref, fn_got):
    """Both give the same result, or raise the same class (an AssertionError also with the same message)."""
    try:
        want = fn_ref()
    except (AssertionError, IndexError) as exc:
        with pytest.raises(type(exc)) as ei:
            fn_got()
        if isinstance(exc, AssertionError):
            assert str(ei.value) == str(exc)
        return None
    except orc.NonAsciiSequence:
        from tagdigger_amd import NonAsciiSequence
        with pytest.raises(NonAsciiSequence):
            fn_got()
        return None
    return want


@pytest.mark.parametrize("taglen", [8, 20])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_golden_payloads_host(case, taglen, tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    path = write_case_file(case, tmp_path)
    barcodes, cutsite, maxreads = case_args(case)
    want = expect_or_raise(lambda: ref_census(orc.read_fastq_bytes(path), barcodes, cutsite, taglen, maxreads),
                           lambda: tf.tag_census(path, barcodes, cutsite, taglen, maxreads, backend="host"))
    if want is None:
        return
    got = tf.tag_census(path, barcodes, cutsite, taglen, maxreads, backend="host")
    assert list(got) == ordered(want[0])
    assert got.stats == {k: want[1][k] for k in STATS}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    rnd = random.Random(11)
    pool = [rand_seq(rnd, 160) for _ in range(12)]
    data = fastq(library(rnd, 400, pool=pool), nl="\r\n")
    d = tmp_path_factory.mktemp("census")
    plain, gz = str(d / "lib.fq"), str(d / "lib.fq.gz")
    with open(plain, "wb") as fh:
        fh.write(data)
    with gzip.open(gz, "wb") as fh:
        fh.write(data)
    return data, plain, gz


def test_maxreads_inside_file_and_gz(lib):
    from tagdigger_amd import tagdigger_fun as tf
    data, plain, gz = lib
    for maxreads in (1, 57, 57.5, 399, 400, 5e9):
        want, st = ref_census(data, BARCODES_MIXED, "TGCAG", 20, maxreads)
        for path in (plain, gz):
            got = tf.tag_census(path, BARCODES_MIXED, taglen=20, maxreads=maxreads, backend="host")
            assert list(got) == ordered(want)
            assert got.stats == {k: st[k] for k in STATS}
    assert ref_census(data, BARCODES_MIXED, "TGCAG", 20, 57)[1]["reads"] == 57


def test_min_count_top_and_ties(lib, tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    data, plain, _ = lib
    want, st = ref_census(data, BARCODES_MIXED, "TGCAG", 12)
    counts = sorted(want.values())
    assert len(set(counts)) < len(counts), "the input must hold ties"
    mid = counts[len(counts) // 2]
    got = tf.tag_census(plain, BARCODES_MIXED, taglen=12, min_count=mid, backend="host")
    assert list(got) == ordered(want, min_count=mid) and got[0]
    assert got.stats["distinct"] == len(want)                    # before min_count is applied
    for top in (0, 1, 5, 10 ** 6):
        assert list(tf.tag_census(plain, BARCODES_MIXED, taglen=12, top=top, backend="host")) == ordered(want, top=top)
    # ties alone: every window once, so the order is the sequences'
    reads = ["ACGTTGCAG" + t for t in ("TTTT", "GGGG", "AAAA", "CCCC", "ACGT", "AGCT")]
    path = str(tmp_path / "ties.fq")
    with open(path, "wb") as fh:
        fh.write(fastq(reads))
    got = tf.tag_census(path, ["ACGT"], taglen=9, backend="host")
    assert got[0] == sorted("TGCAG" + t for t in ("TTTT", "GGGG", "AAAA", "CCCC", "ACGT", "AGCT")) and got[1] == [1] * 6


@pytest.mark.parametrize("with_site", [True, False])
def test_known_annotation(with_site, tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    L = 16
    bodies = ["AAAACCCCGGGTTTTACGT", "AAAACCCCGGGTTTAACGT", "CCCCCCCCCCCCCCCCCCC", "GTGTGTGTGTGTGTGTGTG"]
    reads = ["ACGTTGCAG" + b for b in bodies for _ in range(2)]
    path = str(tmp_path / "k.fq")
    with open(path, "wb") as fh:
        fh.write(fastq(reads))
    site = "TGCAG" if with_site else ""
    # a tag longer than the window, one shorter, two that name the same window, one that matches nothing
    known = [["long_0", "short_0", "same_0", "same_1", "none_0"],
             [site + "AAAACCCCGGGTTTTACGT", site + "CCCC", site + "AAAACCCCGGG", (site + "AAAACCCCGGGTTTT")[:L] if with_site else "AAAACCCCGGG",
              site + "TTTTTTTT"]]
    got = tf.tag_census(path, ["ACGT"], taglen=L, known=known, backend="host")
    assert len(got) == 3 and got[2] == ref_names(got[0], known, "TGCAG")
    assert any(";" in n for n in got[2]) and "" in got[2] and any(n.startswith("long_0") for n in got[2])
    assert "short_0" in got[2]


def test_argument_errors(lib):
    from tagdigger_amd import tagdigger_fun as tf
    _, plain, _ = lib
    for bad in (0, 65):
        with pytest.raises(ValueError):
            tf.tag_census(plain, BARCODES_MIXED, taglen=bad, backend="host")
    with pytest.raises(AssertionError) as ei:
        tf.tag_census(plain, ["ACGN"], backend="host")
    assert str(ei.value) == "Non-ACGT barcode."
    with pytest.raises(AssertionError) as ei:
        tf.tag_census(plain, ["ACGT"], cutsite="TGCAX", backend="host")
    assert str(ei.value) == "Invalid cut site."
    with pytest.raises(ValueError):
        tf.tag_census(plain, ["ACGT"], backend="cpu")


def test_cli_writes_the_csv(lib, tmp_path, capsys):
    from tagdigger_amd import tag_census
    data, _, gz = lib
    key = str(tmp_path / "key.csv")
    with open(key, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["File", "Barcode", "Sample"])
        for i, b in enumerate(BARCODES_MIXED):
            w.writerow([gz, b, "s%d" % i])
    want, st = ref_census(data, BARCODES_MIXED, "TGCAG", 24)
    seqs, counts = ordered(want, min_count=2, top=7)
    tags = str(tmp_path / "tags.csv")
    with open(tags, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Marker name", "Tag sequence"])
        w.writerow(["M1", seqs[0][:10] + "[" + seqs[0][10] + "/" + ("A" if seqs[0][10] != "A" else "C") + "]" + seqs[0][11:]])
    from tagdigger_amd import tagdigger_fun as tf
    known = tf.readTags_Merged(tags)
    out = str(tmp_path / "census.csv")
    assert tag_census.main(["-f", gz, "-b", key, "-e", "PstI", "-o", out, "--taglen", "24", "--min-count", "2", "--top", "7",
                            "--known-merged", tags, "--td-backend", "host"]) == 0
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(["Tag sequence", "Count", "Known tags"])
    for s, c, n in zip(seqs, counts, ref_names(seqs, known, "TGCAG")):
        w.writerow([s, c, n])
    with open(out, "rb") as fh:
        assert fh.read() == buf.getvalue().encode()
    assert ref_names(seqs, known, "TGCAG")[0] != ""
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line == ("Reads: {reads} With barcode and cut site: {barcut} Short: {short} Ambiguous: {ambiguous} "
                    "Counted: {counted} Distinct: {distinct}").format(**st)
