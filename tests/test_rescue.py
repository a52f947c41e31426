"""Tag rescue on the host: tagdigger_fun._rescue_host against the brute-force restatement of tests/rescue_cases.py, the
begin errors, and the tag_rescue command line end to end with --td-backend host.  No GPU."""
import csv
import random

import pytest

import rescue_cases as rc
from conftest import load_golden

from tagdigger_amd import tagdigger_fun as tf
from tagdigger_amd import tag_rescue


def host(tmp_path, data, barcodes, tags, cutsite="TGCAG", K=1, maxreads=5e9, name="h.fq"):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    res = tf.rescue_tags_fastq(path, barcodes, tags, cutsite=cutsite, maxreads=maxreads, max_mismatch=K, backend="host")
    assert res.backend == "host"
    return res


def check(res, want):
    rescued, st, positions, _ = want
    assert res.rescued == rescued
    assert {k: res.stats[k] for k in rc.CLASSES} == st
    assert res.positions == positions
    assert st["rescued1"] + 2 * st["rescued2"] == sum(positions)


CASES = {
    "tie_equal": lambda K: rc.tie_case_equal(),
    "tie_lengths": lambda K: rc.tie_case_lengths(),
    "two_parts_65": lambda K: rc.two_parts_case(K, 65),
    "two_parts_64": lambda K: rc.two_parts_case(K, 64),
    "second_part_tie": lambda K: rc.second_part_tie_case(),
    "last_part": lambda K: rc.last_part_case(K),
    "n_and_dirt": lambda K: rc.n_case(K),
    "line_ends": lambda K: rc.line_end_case(),
    "shadow": lambda K: rc.shadow_case(),
    "run_65": lambda K: rc.run_case(65, K),
    "mixed": lambda K: rc.mixed_case(K),
}


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_rule_on_the_named_cases(tmp_path, name, K):
    reads, tags = CASES[name](K)
    barcodes = rc.BARCODES_MIXED if name == "mixed" else ["ACGT"]
    for nl, last_nl in (("\n", True), ("\r\n", False)):
        data = rc.fastq(reads, nl=nl, last_nl=last_nl)
        check(host(tmp_path, data, barcodes, tags, K=K), rc.ref_rescue(data, barcodes, tags, K=K))


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 127, 128])
def test_host_rule_on_every_tag_length(tmp_path, n, K):
    reads, tags = rc.length_case(n, K)
    data = rc.fastq(reads)
    want = rc.ref_rescue(data, ["ACGT"], tags, K=K)
    if n >= 31:
        assert want[1]["rescued1"] >= 4 and (K == 1 or want[1]["rescued2"] >= 2)
    check(host(tmp_path, data, ["ACGT"], tags, K=K), want)


def test_named_cases_hold_their_classes():
    """what the builders are named for, in the restatement's own classes"""
    def st(case, K=1):
        reads, tags = case
        return rc.ref_rescue(rc.fastq(reads), ["ACGT"], tags, K=K)[1]
    assert st(rc.tie_case_equal())["ambiguous"] == 1 and st(rc.tie_case_equal())["rescued1"] == 1
    s = st(rc.tie_case_lengths())                          # (the second read is too short for the longer tag: no tie there)
    assert s["ambiguous"] == 1 and s["rescued1"] == 1
    assert st(rc.second_part_tie_case())["ambiguous"] == 2
    assert st(rc.two_parts_case(1, 65))["rescued1"] == 3 and st(rc.two_parts_case(2, 64), 2)["rescued1"] == 3
    assert st(rc.last_part_case(1))["rescued1"] == 2 and st(rc.last_part_case(2), 2)["rescued2"] == 2
    s = st(rc.shadow_case())
    assert s["exact"] == 2 and s["rescued1"] == 1 and s["ambiguous"] == 0
    s = st(rc.n_case(1))
    assert s["rescued1"] >= 5 and s["exact"] == 1
    s = st(rc.line_end_case())
    assert s["reads"] == 8 and s["barcut"] == 7 and s["rescued1"] == 3


def test_golden_payloads_and_the_skip_bound(tmp_path):
    from oracle import tagdigger_oracle as orc
    from tagdigger_amd import NonAsciiSequence
    cases = load_golden("hotpath_cases.json") + load_golden("hotpath_random.json")
    assert len(cases) == 132
    ran = skipped = 0
    for k, case in enumerate(cases):
        kw = case["kwargs"]
        d = tmp_path / ("g%d" % k)
        d.mkdir()
        what, value, path = rc.golden_plan(case, d)
        args = (case["barcodes"], case["tags"], kw.get("cutsite", "TGCAG"))
        if what == "skip":
            skipped += 1
            continue
        for K in (1, 2):
            run = lambda: tf.rescue_tags_fastq(path, *args, maxreads=kw.get("maxreads", 5e9), max_mismatch=K, backend="host")
            if what == "raises":
                with pytest.raises(type(value)):
                    run()
                continue
            try:
                want = rc.ref_rescue(value, *args, K, kw.get("maxreads", 5e9))
            except orc.NonAsciiSequence:
                with pytest.raises(NonAsciiSequence):
                    run()
                continue
            # class 0 is the counter's: what the real reference recorded for this payload
            assert want[1]["exact"] == sum(sum(r) for r in case["counts"]) == sum(sum(r) for r in want[3]), case["name"]
            check(run(), want)
            ran += 1
    assert skipped * 4 <= len(cases) and ran > 200


def test_begin_errors(tmp_path):
    from tagdigger_amd import TagdigError
    data = rc.fastq(["ACGTTGCAGACGTACGT"])
    path = str(tmp_path / "e.fq")
    with open(path, "wb") as fh:
        fh.write(data)

    def run(tags, K=1, cutsite="TGCAG"):
        return tf.rescue_tags_fastq(path, ["ACGT"], tags, cutsite=cutsite, max_mismatch=K, backend="host")
    for K in (0, 3):
        with pytest.raises(ValueError):
            run(["TGCAGAAAA"], K)
    with pytest.raises(ValueError):
        tf.rescue_tags_fastq(path, ["ACGT"], ["TGCAGAAAA"], backend="cpu")
    with pytest.raises(AssertionError, match="Non-ACGT tag"):
        run(["TGCAGAANA"])
    with pytest.raises(IndexError):
        run([])
    with pytest.raises(IndexError):
        run(["TGCAGAAAA", "TGCAG"])                       # stripped of the site: empty
    with pytest.raises(TagdigError) as ei:
        run(["TGCAG" + "A" * 129])
    assert ei.value.code == -7
    assert run(["TGCAG" + "A" * 128]).stats["barcut"] == 1
    for tags, bad in ((["AAAC", "GGGG", "AAAC"], 2), (["AAACT", "GGGG", "AAAC"], 2), (["AAAC", "GGGG", "AAACT"], 2),
                      (["AAACT", "AAAC", "AAACTT", "AAAC"], 1), (["CC", "AAACT", "GG", "AAACTT", "AAAC"], 3)):
        with pytest.raises(AssertionError) as ei:
            run(["TGCAG" + t for t in tags])
        assert str(ei.value) == "Problematic sequence: {}.  Likely due to overlapping tags.".format(bad)
        with pytest.raises(AssertionError) as ej:
            rc.check_tags(tags)
        assert str(ej.value) == str(ei.value)
    # the host rule needs no parts: the shortest tag may be shorter than max_mismatch + 1
    res = run(["TGCAGA", "TGCAGCC"], 2)
    assert res.stats["longest_run"] == 2 and res.stats["barcut"] == 1


def test_longest_run_of_the_host_statistics(tmp_path):
    reads, tags = rc.run_case(64)
    res = host(tmp_path, rc.fastq(reads), ["ACGT"], tags)
    assert res.stats["longest_run"] == 64 == rc.longest_run([t[5:] for t in tags], 1)


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


def test_tag_rescue_command_line_on_the_host(tmp_path, capsys, monkeypatch):
    rnd = random.Random(21)
    markers = []
    for k in range(6):
        left, right = "TGCAG" + rc.rand_seq(rnd, 20), rc.rand_seq(rnd, 30)
        a = rnd.choice("ACGT")
        markers.append(("Mk%d" % k, left, a, rc.other(a), right))
    tags = [left + x + right for _, left, a, b, right in markers for x in (a, b)]
    table = str(tmp_path / "markers.csv")
    merged_table(table, markers)
    libs = {"lib_a.fq": (["ACGT", "TGACA"], ["s1", "s2"]), "lib_b.fq": (["GATTAC", "ACGT"], ["s2", "s3"])}
    monkeypatch.chdir(tmp_path)
    with open("key.csv", "w", newline="") as fh:
        out = csv.writer(fh)
        out.writerow(["File", "Barcode", "Sample"])
        for f, (bars, sams) in libs.items():
            for b, s in zip(bars, sams):
                out.writerow([f, b, s])
    want_exact, want_resc, want_stats = {}, {}, {}
    for f, (bars, sams) in libs.items():
        reads = []
        for _ in range(300):
            t = rnd.choice(tags)[5:]
            roll = rnd.random()
            w = t if roll < 0.5 else rc.sub(t, rnd.randrange(len(t))) if roll < 0.8 else rc.sub(t, 3, 40) if roll < 0.9 else rc.rand_seq(rnd, 60)
            reads.append(rnd.choice(bars) + "TGCAG" + w + rc.rand_seq(rnd, 10))
        data = rc.fastq(reads)
        with open(f, "wb") as fh:
            fh.write(data)
        want_resc[f], want_stats[f], _, want_exact[f] = rc.ref_rescue(data, bars, tags, K=1)
        assert want_stats[f]["rescued1"] > 30 and want_stats[f]["exact"] > 100
    assert tag_rescue.main(["-e", "PstI", "--MergedTags", table, "-b", "key.csv", "-o", "sum.csv", "--exact-out", "exact.csv",
                            "--rescued-out", "rescued.csv", "--stats", "stats.csv", "--td-backend", "host"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("lib_")]
    assert len(lines) == 2 and all("%d rescued at 1" % want_stats[f]["rescued1"] in l for f, l in zip(sorted(libs), lines))
    names, samples, total = read_csv("sum.csv")
    _, s_e, exact = read_csv("exact.csv")
    _, s_r, rescued = read_csv("rescued.csv")
    assert samples == s_e == s_r == ["s1", "s2", "s3"] and len(names) == 12
    keys = {f: [bars, sams] for f, (bars, sams) in libs.items()}
    assert exact == tf.combineReadCounts({f: [list(r) for r in want_exact[f]] for f in libs}, keys)[1]
    assert rescued == tf.combineReadCounts({f: [list(r) for r in want_resc[f]] for f in libs}, keys)[1]
    assert total == [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(exact, rescued)]
    assert sum(map(sum, rescued)) == sum(st["rescued1"] for st in want_stats.values()) > 0
    with open("stats.csv", newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["Library"] + list(rc.CLASSES) + ["rescued_share"]
    for row, f in zip(rows[1:], sorted(libs)):
        st = want_stats[f]
        assert row[:-1] == [f] + [str(st[k]) for k in rc.CLASSES]
        assert row[-1] == format((st["rescued1"] + st["rescued2"]) / st["barcut"], ".6f")
    # the sum file is a counts file: tag_calls reads it
    from tagdigger_amd import tag_calls
    assert tag_calls.main(["-i", "sum.csv", "-o", "calls.csv", "--td-backend", "host"]) == 0
    assert "Samples: 3 Markers: 6" in capsys.readouterr().out
