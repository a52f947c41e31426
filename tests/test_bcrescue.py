"""The barcode-rescue rule on the host (tagdigger_fun._bcrescue_host) against the brute-force restatement of
tests/bcrescue_cases.py, its begin errors, the statistics file and the command line on the host backend.  No GPU."""
import csv
import random

import pytest

import bcrescue_cases as bc
from conftest import load_golden
from tagdigger_amd import tagdigger_fun as tf


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def host(tmp_path, case, K, maxreads=5e9):
    return tf._bcrescue_host_lists(write(tmp_path, "h.fq", case.data), case.barcut, case.barnum, case.tagoff, case.stored, maxreads, K)


check = bc.check


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", sorted(bc.NAMED))
def test_host_rule_on_the_named_cases(tmp_path, name, K):
    case = bc.NAMED[name](K)
    check(host(tmp_path, case, K), bc.ref_case(case, K))


@pytest.mark.parametrize("kind", ["exact", "nohit", 63, 64, 65])
def test_host_rule_on_the_tile_cases(tmp_path, kind):
    case = bc.tile_case(kind)
    check(host(tmp_path, case, 2), bc.ref_case(case, 2))


def test_host_rule_on_the_index_shapes(tmp_path):
    for case, all_pairs in ((bc.wide_index_case(), True), (bc.full_index_case(0), False), (bc.big_case(), True)):
        for K in (1, 2):
            check(host(tmp_path, case, K), bc.ref_case(case, K, min_distance=all_pairs))
    big = bc.big_case()
    for maxreads in (1, 130, 699):
        want = bc.ref_case(big, 1, maxreads)
        assert want[1]["reads"] == maxreads
        check(host(tmp_path, big, 1, maxreads), want)


def test_named_cases_hold_their_classes():
    def st(case, K):
        return bc.ref_case(case, K)
    m, s, rows, pos = st(bc.geometry_case(1), 1)
    assert s["rescued1"] == 150 and s["exact"] == 0 and pos[0] >= 12 and pos[13] >= 2          # every position of every entry, the last of the longest
    m, s, rows, pos = st(bc.geometry_case(2), 2)
    assert s["rescued2"] == 24 and s["none"] == 6                                                # four pairs and K + 1 = 3 per entry
    m, s, rows, pos = st(bc.long_entries_case(2), 2)
    assert pos[30] >= 2 and pos[31] >= 2 and s["rescued2"] == 4
    m, s, rows, pos = st(bc.near_and_far_case(), 1)
    assert rows[0][0] == 2 and rows[1][0] == 2 and s["ambiguous"] == 0
    m, s, rows, pos = st(bc.read_length_case(), 1)
    assert s["none"] == 3 and s["rescued1"] == 6 and s["tagged"] == 3
    m, s, rows, pos = st(bc.two_rows_tie_case(), 1)
    assert s["ambiguous"] == 2 and s["min_entry_distance"] == 2
    m, s, rows, pos = st(bc.variants_tie_case(), 1)
    assert s["rescued1"] == 3 and pos[4] == 2 and pos[5] == 1 and s["ambiguous"] == 0           # the earlier entry's position, not the directory's first
    m, s, rows, pos = st(bc.length_trap_case(), 1)
    assert s["ambiguous"] == 1 and s["rescued1"] == 1 and s["exact"] == 1
    m, s, rows, pos = st(bc.shadow_case(), 1)
    assert s["rescued1"] == 3 and s["ambiguous"] == 0 and rows[2] == rows[3] == [0, 0]
    m, s, rows, pos = st(bc.degenerate_site_case(1), 1)
    assert s["rescued1"] == 30 and s["ambiguous"] == 0
    m, s, rows, pos = st(bc.tag_lengths_case(True), 1)
    assert all(sum(r[t] for r in m) >= 6 for t in range(len(m[0])))                              # every tag length is counted


def test_min_entry_distance_on_hand_made_sets():
    def dist(barcut, barnum):
        entries = tf._bcrescue_entries(barcut, barnum)
        assert entries == bc.entries_of(barcut, barnum)
        assert tf._bcrescue_min_distance(entries) == bc.min_entry_distance(entries)
        return tf._bcrescue_min_distance(entries)
    assert dist(["ACGTTGCAG"], 1) == bc.NO_PAIR
    assert dist(["ACGTTGCAG", "ACGTTGCAT"], 1) == bc.NO_PAIR                   # two entries, one row
    assert dist(["ACGTTGCAG", "ACGTTGCAT"], 2) == 1
    assert dist(["AAAAATGCAG", "AACCCTGCAG", "GGTGTTGCAG"], 3) == 3
    # variable lengths: over the shorter entry's length, the longer one truncated
    assert dist(["ACGTTTAA", "ACGTTTTAA"], 2) == 1                             # ACGTTTAA / ACGTTTTA
    assert dist(["ACGTACGT", "ACGTACGAAAAA"], 2) == 1
    assert dist(["ACGTACGTTTTT", "ACGAACGT"], 2) == 1
    assert dist(["ACGT", "TGCATTTT", "TGCAAAAAAA"], 3) == 4
    # the variants of one row do not count, those of two rows do: rows 0 1 0 1
    assert dist(["AAAACAGC", "CCCCCAGC", "AAAACTGC", "CCCCCTGC"], 2) == 4
    assert dist(["AAAACAGC", "AAAACTGC"], 2) == 1
    # a shadowed duplicate is no entry
    assert dist(["ACGTTGCAG", "GGATCTGCAG", "ACGTTGCAG", "ACGTTGCAGAC"], 4) == 8


def test_begin_errors(tmp_path):
    from tagdigger_amd import TagdigError
    path = write(tmp_path, "e.fq", bc.fastq(["ACGTTGCAGACGTACGT"]))

    def run(tags, K=1, barcodes=("ACGT",), cutsite="TGCAG", backend="host"):
        return tf.rescue_barcodes_fastq(path, list(barcodes), tags, cutsite=cutsite, max_mismatch=K, backend=backend)
    for K in (0, 3):
        with pytest.raises(ValueError):
            run(["TGCAGAAAA"], K)
    with pytest.raises(ValueError):
        run(["TGCAGAAAA"], backend="cpu")
    with pytest.raises(AssertionError, match="Non-ACGT tag"):
        run(["TGCAGAANA"])
    with pytest.raises(AssertionError, match="Non-ACGT barcode"):
        run(["TGCAGAAAA"], barcodes=["ACNT"])
    with pytest.raises(IndexError):
        run([])
    with pytest.raises(IndexError):
        run(["TGCAGAAAA", "TGCAG"])                       # stripped of the site: empty
    with pytest.raises(TagdigError) as ei:
        run(["TGCAG" + "A" * 129])
    assert ei.value.code == -7
    assert run(["TGCAG" + "A" * 128])[1]["exact"] == 1
    for tags, bad in ((["AAAC", "GGGG", "AAAC"], 2), (["AAACT", "GGGG", "AAAC"], 2), (["CC", "AAACT", "GG", "AAACTT", "AAAC"], 3)):
        with pytest.raises(AssertionError) as ei:
            run(["TGCAG" + t for t in tags])
        assert str(ei.value) == "Problematic sequence: {}.  Likely due to overlapping tags.".format(bad)
    # the index build's errors are td_set_index's: a later barcode + site that begins an earlier one
    with pytest.raises(AssertionError) as ei:
        run(["TGCAGAAAA"], barcodes=["ACGTTGCAGA", "ACGT"])
    assert str(ei.value) == "Problematic sequence: 1.  Likely due to overlapping tags."
    # every surviving entry must be longer than 2 K bases
    for K, barcodes, cutsite, ok in ((1, ["AC"], "", False), (1, ["ACG"], "", True), (2, ["AC"], "GT", False), (2, ["ACG"], "GT", True),
                                     (2, ["ACGTA", "T"], "GCA", False)):
        if ok:
            assert run(["AAAA"], K, barcodes, cutsite)[1]["reads"] == 1
            continue
        with pytest.raises(ValueError, match="^barcode rescue: entry"):
            run(["AAAA"], K, barcodes, cutsite)
        with pytest.raises(bc.Limit):
            bc.check_begin(*bc.lists(barcodes, ["AAAA"], cutsite)[:2], ["AAAA"], K)


def test_golden_payloads_and_the_skip_bound(tmp_path):
    """The recorded hot-path payloads through the host rule.  What may be skipped is counted by reason: these counts are
    the ones tests/test_bcrescue_gpu.py must reach too, and three quarters of the payloads run."""
    cases = load_golden("hotpath_cases.json") + load_golden("hotpath_random.json")
    assert len(cases) == 132
    for K in (1, 2):
        ran, skips = bc.golden_payloads(tmp_path, cases, K, lambda path, args, maxreads: tf.rescue_barcodes_fastq(
            path, *args, maxreads=maxreads, max_mismatch=K, backend="host"))
        assert skips == bc.GOLDEN_SKIPS[K]
        assert ran * 4 >= 3 * len(cases)


def test_stats_file(tmp_path):
    results = [dict(zip(bc.STATS, (100, 70, 12, 3, 5, 10, 11, 3)), row_rescued=[], positions=[]),
               dict(zip(bc.STATS, (7, 7, 0, 0, 0, 0, 0, 64)), row_rescued=[], positions=[]),
               dict(zip(bc.STATS, (9, 0, 0, 0, 2, 7, 0, 1)), row_rescued=[], positions=[])]
    path = str(tmp_path / "s.csv")
    tf.writeBarcodeRescueStats(path, ["a.fq", "b,\"x\".fq", "c.fq"], results)
    with open(path, "rb") as fh:
        raw = fh.read()
    assert raw.count(b"\r\n") == 4 and b'"b,""x"".fq"' in raw                   # csv.writer rows
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["Library"] + list(bc.STATS) + ["rescued_share"]
    assert rows[1] == ["a.fq", "100", "70", "12", "3", "5", "10", "11", "3", "0.500000"]
    assert rows[2] == ["b,\"x\".fq", "7", "7", "0", "0", "0", "0", "0", "64", "NA"]
    assert rows[3][-1] == "0.000000"


def merged_table(path, markers):
    with open(path, "w", newline="") as fh:
        out = csv.writer(fh)
        out.writerow(["Marker name", "Tag sequence"])
        for name, left, a, b, right in markers:
            out.writerow([name, "%s[%s/%s]%s" % (left, a, b, right)])


def read_csv(path):
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    return rows[0][1:], [r[0] for r in rows[1:]], [[int(x) for x in r[1:]] for r in rows[1:]]


def test_barcode_rescue_command_line_on_the_host(tmp_path, capsys, monkeypatch):
    import rescue_cases as rc
    from tagdigger_amd import barcode_rescue
    rnd = random.Random(61)
    markers = []
    for k in range(6):
        left, right = "TGCAG" + bc.rand_seq(rnd, 20), bc.rand_seq(rnd, 30)
        a = rnd.choice("ACGT")
        markers.append(("Mk%d" % k, left, a, bc.other(a), right))
    tags = [left + x + right for _, left, a, b, right in markers for x in (a, b)]
    table = str(tmp_path / "markers.csv")
    merged_table(table, markers)
    # lib_b's barcodes lie one substitution apart: its line of warning
    libs = {"lib_a.fq": (["ACGT", "TGACA"], ["s1", "s2"]), "lib_b.fq": (["GATTAC", "GATTAG", "ACGT"], ["s2", "s3", "s3"])}
    monkeypatch.chdir(tmp_path)
    with open("key.csv", "w", newline="") as fh:
        out = csv.writer(fh)
        out.writerow(["File", "Barcode", "Sample"])
        for f, (bars, sams) in libs.items():
            for b, s in zip(bars, sams):
                out.writerow([f, b, s])
    want, want_exact = {}, {}
    for f, (bars, sams) in libs.items():
        reads = bc.library(rnd, [b + "TGCAG" for b in bars], [t[5:] for t in tags], 300)
        data = bc.fastq(reads)
        with open(f, "wb") as fh:
            fh.write(data)
        want[f] = bc.ref_lists(data, *bc.lists(bars, tags), 2)
        want_exact[f] = rc.ref_rescue(data, bars, tags, K=1)[3]
        assert want[f][1]["rescued1"] > 30 and want[f][1]["rescued2"] > 5 and want[f][1]["exact"] > 100 and want[f][1]["tagged"] > 30
    assert barcode_rescue.main(["-e", "PstI", "--MergedTags", table, "-b", "key.csv", "-o", "sum.csv", "--max-mismatch", "2", "--rescued-out",
                                "rescued.csv", "--rows-out", "rows.csv", "--stats", "stats.csv", "--td-backend", "host"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("lib_")]
    assert len(lines) == 3 and "WARNING" in lines[2] and lines[2].startswith("lib_b.fq") and "WARNING" not in lines[0] + lines[1]
    assert all("%d rescued at 1, %d rescued at 2" % (want[f][1]["rescued1"], want[f][1]["rescued2"]) in l for f, l in zip(sorted(libs), lines))
    names, samples, total = read_csv("sum.csv")
    _, s_r, rescued = read_csv("rescued.csv")
    assert samples == s_r == ["s1", "s2", "s3"] and len(names) == 12
    keys = {f: [bars, sams] for f, (bars, sams) in libs.items()}
    exact = tf.combineReadCounts({f: [list(r) for r in want_exact[f]] for f in libs}, keys)[1]
    assert rescued == tf.combineReadCounts({f: [list(r) for r in want[f][0]] for f in libs}, keys)[1]
    # the counts are the counter's plus the rescued
    assert total == [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(exact, rescued)]
    assert sum(map(sum, rescued)) == sum(w[1]["tagged"] for w in want.values()) > 0
    with open("stats.csv", newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["Library"] + list(bc.STATS) + ["rescued_share"]
    for row, f in zip(rows[1:], sorted(libs)):
        st = want[f][1]
        assert row[:-1] == [f] + [str(st[k]) for k in bc.STATS]
        assert row[-1] == format((st["rescued1"] + st["rescued2"]) / (st["reads"] - st["exact"]), ".6f")
    with open("rows.csv", newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["Library", "Barcode", "Sample", "rescued1", "rescued2"]
    assert rows[1:] == [[f, b, s, str(r[0]), str(r[1])] for f in sorted(libs) for b, s, r in zip(*libs[f], want[f][2])]
    # the sum file is a counts file: tag_calls reads it
    from tagdigger_amd import tag_calls
    assert tag_calls.main(["-i", "sum.csv", "-o", "calls.csv", "--td-backend", "host"]) == 0
    assert "Samples: 3 Markers: 6" in capsys.readouterr().out
