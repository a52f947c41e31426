"""Tag rescue on the GPU (csrc/rescue.hip) against the brute-force restatement of tests/rescue_cases.py, through
td_rescue_device (a resident buffer) and td_rescue_file (the file readers): the matrix, the seven classes and the
position histogram, for equality."""
import gzip
import random

import pytest

import rescue_cases as rc
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
    st = eng.rescue_stats()
    matrix, pos = eng.rescue_fetch()
    return matrix.tolist(), {k: st[k] for k in rc.CLASSES}, [int(x) for x in pos], st["longest_run"]


def run_pieces(eng, pieces, maxreads=5e9):
    for part, fl in pieces:
        if not part:
            continue
        d = eng.dev_alloc(len(part))
        try:
            eng.h2d(d, part)
            eng.rescue_device(d, len(part), fl, maxreads)
            eng.sync()
        finally:
            eng.dev_free(d)


def device_rescue(eng, data, barcodes, tags, cutsite="TGCAG", K=1, maxreads=5e9, pieces=None):
    """Through td_rescue_device: `pieces` = [(bytes, first_line), ...] of one begin, else the whole buffer."""
    eng.rescue_begin(barcodes, tags, cutsite, K)
    try:
        run_pieces(eng, pieces or [(data, 0)], maxreads)
        return fetched(eng)
    finally:
        eng.rescue_end()


def file_rescue(eng, path, barcodes, tags, cutsite="TGCAG", K=1, maxreads=5e9):
    eng.rescue_begin(barcodes, tags, cutsite, K)
    try:
        eng.rescue_file(path, maxreads)
        return fetched(eng)
    finally:
        eng.rescue_end()


def check(got, want):
    rescued, st, positions, _ = want
    assert got[1] == st
    assert got[0] == rescued
    assert got[2] == positions


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def both_routes(eng, tmp_path, reads, barcodes, tags, cutsite="TGCAG", K=1, nl="\n", last_nl=True):
    data = rc.fastq(reads, nl=nl, last_nl=last_nl)
    want = rc.ref_rescue(data, barcodes, tags, cutsite, K)
    check(device_rescue(eng, data, barcodes, tags, cutsite, K), want)
    check(file_rescue(eng, write(tmp_path, "r.fq", data), barcodes, tags, cutsite, K), want)
    return want


# ---------------------------------------------------------------------------------------------------- golden payloads
def test_golden_payloads(eng, tmp_path):
    from tagdigger_amd import NonAsciiSequence, TagdigError, tagdigger_fun as tf
    cases = load_golden("hotpath_cases.json") + load_golden("hotpath_random.json")
    ran = skipped = 0
    for k, case in enumerate(cases):
        kw = case["kwargs"]
        d = tmp_path / ("g%d" % k)
        d.mkdir()
        what, value, path = rc.golden_plan(case, d)
        args = (case["barcodes"], case["tags"], kw.get("cutsite", "TGCAG"))
        maxreads = kw.get("maxreads", 5e9)
        if what == "skip":
            skipped += 1
            continue
        for K in (1, 2):
            if what == "raises":
                with pytest.raises(type(value)):
                    file_rescue(eng, path, *args, K, maxreads)
                continue
            # tags too short for K + 1 parts: the device refuses, the Python function answers through the host rule
            no_parts = rc.part_bases(orc.prepare_lists(*args)[2], K) < 1
            through_python = lambda: tf.rescue_tags_fastq(path, *args, maxreads=maxreads, max_mismatch=K)
            try:
                want = rc.ref_rescue(value, *args, K, maxreads)
            except orc.NonAsciiSequence:
                with pytest.raises(NonAsciiSequence):
                    through_python() if no_parts else device_rescue(eng, value, *args, K, maxreads)
                with pytest.raises(NonAsciiSequence):
                    through_python() if no_parts else file_rescue(eng, path, *args, K, maxreads)
                continue
            if no_parts:
                with pytest.raises(TagdigError) as ei:
                    eng.rescue_begin(*args, K)
                assert ei.value.code == -7 and ei.value.detail.startswith("tag rescue: run")
                res = through_python()
                assert res.backend == "host" and (res.rescued, {k: res.stats[k] for k in rc.CLASSES}, res.positions) == want[:3]
                ran += 1
                continue
            # class 0 is the counter's: what the real reference recorded for this payload
            assert want[1]["exact"] == sum(sum(r) for r in case["counts"]), case["name"]
            check(device_rescue(eng, value, *args, K, maxreads), want)
            check(file_rescue(eng, path, *args, K, maxreads), want)
            ran += 1
    assert skipped * 4 <= len(cases) and ran > 200


# -------------------------------------------------------------------------------------------------------- tag lengths
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 127, 128])
def test_every_tag_length(eng, tmp_path, n, K):
    from tagdigger_amd import TagdigError, tagdigger_fun as tf
    reads, tags = rc.length_case(n, K)
    P = n // (K + 1)
    if P < 1:
        # no part: the device refuses, the Python function answers through the host rule
        with pytest.raises(TagdigError) as ei:
            eng.rescue_begin(["ACGT"], tags, "TGCAG", K)
        assert ei.value.code == -7 and ei.value.detail.startswith("tag rescue: run")
        data = rc.fastq(reads)
        res = tf.rescue_tags_fastq(write(tmp_path, "p.fq", data), ["ACGT"], tags, max_mismatch=K)
        want = rc.ref_rescue(data, ["ACGT"], tags, K=K)
        assert res.backend == "host" and (res.rescued, {k: res.stats[k] for k in rc.CLASSES}, res.positions) == want[:3]
        return
    want = both_routes(eng, tmp_path, reads, ["ACGT"], tags, K=K)
    if n >= 31:
        assert want[1]["rescued1"] >= 4 and (K == 1 or want[1]["rescued2"] >= 2)


@pytest.mark.parametrize("K", [1, 2])
def test_mixed_lengths_in_one_index(eng, tmp_path, K):
    reads, tags = rc.mixed_case(K)
    want = both_routes(eng, tmp_path, reads, rc.BARCODES_MIXED, tags, K=K)
    assert want[1]["rescued1"] > 30 and want[1]["exact"] >= 18


# ------------------------------------------------------------------------- N, dirt, line ends, ties, duplicates, shadows
NAMED = {
    "tie_equal": lambda K: rc.tie_case_equal(),
    "tie_lengths": lambda K: rc.tie_case_lengths(),
    "two_parts_65": lambda K: rc.two_parts_case(K, 65),
    "two_parts_64": lambda K: rc.two_parts_case(K, 64),
    "second_part_tie": lambda K: rc.second_part_tie_case(),
    "last_part": lambda K: rc.last_part_case(K),
    "n_and_dirt": lambda K: rc.n_case(K),
    "line_ends": lambda K: rc.line_end_case(),
    "shadow": lambda K: rc.shadow_case(),
}


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_cases(eng, tmp_path, name, K):
    reads, tags = NAMED[name](K)
    both_routes(eng, tmp_path, reads, ["ACGT"], tags, K=K)
    both_routes(eng, tmp_path, reads, ["ACGT"], tags, K=K, nl="\r\n", last_nl=False)     # CRLF, a last line without terminator
    both_routes(eng, tmp_path, reads, ["ACGT"], tags, K=K, nl="\r")


def test_line_as_the_buffers_last_bytes(eng, tmp_path):
    """the read line is the buffer's end: at the tag's end, one base short of it, inside the barcode, with avail = 0"""
    reads, tags = rc.line_end_case()
    for r in reads:
        data = ("@a\n" + r).encode()
        want = rc.ref_rescue(data, ["ACGT"], tags)
        check(device_rescue(eng, data, ["ACGT"], tags), want)
        check(file_rescue(eng, write(tmp_path, "e.fq", data), ["ACGT"], tags), want)


# --------------------------------------------------------------------------------------------------------------- runs
@pytest.mark.parametrize("nrun", [1, 63, 64, 65, 1000])
def test_runs_and_the_run_cap(eng, tmp_path, nrun):
    from tagdigger_amd import TagdigError, tagdigger_fun as tf
    reads, tags = rc.run_case(nrun)
    data = rc.fastq(reads)
    want = rc.ref_rescue(data, ["ACGT"], tags)
    assert want[1]["rescued1"] >= 1
    got = device_rescue(eng, data, ["ACGT"], tags)
    check(got, want)
    assert got[3] == nrun
    path = write(tmp_path, "run.fq", data)
    try:
        eng.set_option("rescue_max_run", nrun)                  # just enough
        check(file_rescue(eng, path, ["ACGT"], tags), want)
        if nrun > 1:
            eng.set_option("rescue_max_run", nrun - 1)          # just below
            with pytest.raises(TagdigError) as ei:
                eng.rescue_begin(["ACGT"], tags)
            assert ei.value.code == -7 and ei.value.detail.startswith("tag rescue: run of %d tags" % nrun)
            # ... which the Python function answers through the host rule (it counts on the default engine)
            from tagdigger_amd.engine import default_engine
            default_engine(0).set_option("rescue_max_run", nrun - 1)
            try:
                res = tf.rescue_tags_fastq(path, ["ACGT"], tags)
                assert res.backend == "host"
                assert (res.rescued, {k: res.stats[k] for k in rc.CLASSES}, res.positions) == want[:3]
                assert res.stats["longest_run"] == nrun
                default_engine(0).set_option("rescue_max_run", nrun)
                res = tf.rescue_tags_fastq(path, ["ACGT"], tags)
                assert res.backend == "gpu"
                assert (res.rescued, {k: res.stats[k] for k in rc.CLASSES}, res.positions) == want[:3]
            finally:
                default_engine(0).set_option("rescue_max_run", 0)
    finally:
        eng.set_option("rescue_max_run", 0)


# ------------------------------------------------------------------------------------------------------- index shapes
def shape_library(rnd, stored, heads, n=400):
    """reads: a head (barcode + whatever precedes the compared window) + a stored tag with 0..3 substitutions"""
    reads = []
    for _ in range(n):
        t = rnd.choice(stored)
        k = rnd.choice((0, 1, 1, 2, 3))
        w = rc.sub(t, *rnd.sample(range(len(t)), k))
        if rnd.random() < 0.1:
            w = rc.sub(w, rnd.randrange(len(w)), to="N")
        reads.append(rnd.choice(heads) + w + rc.rand_seq(rnd, rnd.randrange(0, 12)))
    return reads


def test_index_shapes(eng, tmp_path):
    rnd = random.Random(31)
    bars = rc.BARCODES_MIXED
    bodies = rc.free_tags(rnd, [rnd.randint(24, 70) for _ in range(30)])
    # a degenerate cut site, the tags keep it: compared from the site's first base
    tags = [rnd.choice(("CAGC", "CTGC")) + b for b in bodies]
    want = both_routes(eng, tmp_path, shape_library(rnd, tags, bars), bars, tags, "CWGC", 1)
    assert want[1]["rescued1"] > 50 and want[1]["exact"] > 30
    both_routes(eng, tmp_path, shape_library(rnd, tags, bars), bars, tags, "CWGC", 2)
    # tags without the site: compared behind it
    want = both_routes(eng, tmp_path, shape_library(rnd, bodies, [b + s for b in bars for s in ("CAGC", "CTGC")]), bars, bodies, "CWGC", 2)
    assert want[1]["rescued2"] > 30
    # one cut site, the tags carry it and are stripped
    tags = ["TGCAG" + b for b in bodies]
    want = both_routes(eng, tmp_path, shape_library(rnd, bodies, [b + "TGCAG" for b in bars]), bars, tags, "TGCAG", 2)
    assert want[1]["rescued1"] > 50 and sum(map(sum, want[0])) == want[1]["rescued1"] + want[1]["rescued2"]
    # no cut site at all
    both_routes(eng, tmp_path, shape_library(rnd, bodies, bars), bars, bodies, "", 1)


def test_offset_behind_the_barcode_entry(eng):
    """the C-ABI takes a tag offset behind the barcode + cut site entry: the window may start behind the line's end"""
    rnd = random.Random(32)
    stored = rc.free_tags(rnd, [30] * 5)
    reads = ["ACGTTGCAG" + "GATTACA" + rc.sub(stored[0], 7) + "AC", "ACGTTGCAG" + "GAT", "ACGTTGCAG", "ACGTTGCAGGATTACA",
             "ACGTTGCAGGATTACA" + stored[1], "ACGTTGCAGGATTACA" + rc.sub(stored[1], 3, 9)[:29] + "N", "ACGTTGCAGGA  "]
    data = rc.fastq(reads)
    want = rc.ref_rescue_lists(data, ["ACGTTGCAG"], 1, [16], stored, 1)
    assert want[1]["barcut"] == 7 and want[1]["rescued1"] == 1 and want[1]["exact"] == 1 and want[1]["none"] == 5
    eng._rescue_begin_lists(["ACGTTGCAG"], 1, [16], stored, 1)
    try:
        run_pieces(eng, [(data, 0)])
        check(fetched(eng), want)
    finally:
        eng.rescue_end()


# ----------------------------------------------------------------------------------------------------------- geometry
@pytest.fixture(scope="module")
def big():
    rnd = random.Random(33)
    bodies = rc.free_tags(rnd, [rnd.randint(30, 110) for _ in range(40)])
    reads = shape_library(rnd, bodies, [b + "TGCAG" for b in rc.BARCODES_MIXED] + ["TTTTTTTTT"], 700)
    data = rc.fastq(reads, nl="\r\n")
    assert len(data) > 6 * rc.TILE
    return data, ["TGCAG" + b for b in bodies]


_BIG_WANT = {}


def big_want(big, K=1, maxreads=5e9):
    """the restatement over the big library, computed once per (K, maxreads)"""
    if (K, maxreads) not in _BIG_WANT:
        _BIG_WANT[K, maxreads] = rc.ref_rescue(big[0], rc.BARCODES_MIXED, big[1], K=K, maxreads=maxreads)
    return _BIG_WANT[K, maxreads]


def test_tile_seam_at_every_window_offset(eng):
    rnd = random.Random(34)
    stored = rc.free_tags(rnd, [128] * 3 + [40])
    tags = ["TGCAG" + t for t in stored]
    read = "ACGTTGCAG" + rc.sub(stored[0], 0, 127) + "ACGT"
    eng.rescue_begin(["ACGT"], tags, "TGCAG", 2)
    try:
        total = [0] * 7
        for window_at in range(rc.TILE - 135, rc.TILE + 12):       # the line's start and the window's 128 bases cross the seam
            data = rc.straddle_buffer(rnd, window_at, read)
            before = fetched(eng)
            run_pieces(eng, [(data, 0)])
            after = fetched(eng)
            want = rc.ref_rescue(data, ["ACGT"], tags, K=2)
            assert want[1]["rescued2"] >= 1
            assert {k: after[1][k] - before[1][k] for k in rc.CLASSES} == want[1], window_at
            assert [[a - b for a, b in zip(ra, rb)] for ra, rb in zip(after[0], before[0])] == want[0], window_at
            assert [a - b for a, b in zip(after[2], before[2])] == want[2], window_at
    finally:
        eng.rescue_end()


@pytest.mark.parametrize("K", [1, 2])
def test_grid_caps_and_two_runs_identical(eng, big, K):
    data, tags = big
    want = big_want(big, K)
    assert want[1]["rescued1"] > 100 and want[1]["none"] > 50
    try:
        got = []
        for cap in (0, 1, 2, 0):
            eng.set_option("max_grid", cap)
            got.append(device_rescue(eng, data, rc.BARCODES_MIXED, tags, K=K))
            check(got[-1], want)
        assert got[0] == got[3]
    finally:
        eng.set_option("max_grid", 0)


def test_pieces_that_begin_inside_a_record(eng, big):
    data, tags = big
    want = big_want(big, 2)
    lines = data.split(b"\r\n")
    for cut in (4 * 130 + 1, 4 * 301 + 2, 4 * 77 + 3):
        head = b"\r\n".join(lines[:cut]) + b"\r\n"
        check(device_rescue(eng, None, rc.BARCODES_MIXED, tags, K=2, pieces=[(head, 0), (data[len(head):], cut)]), want)


def test_maxreads_and_the_three_file_formats(eng, big, tmp_path):
    data, tags = big
    plain = write(tmp_path, "m.fq", data)
    gz = write(tmp_path, "m2.fq.gz", gzip.compress(data))
    bg = write(tmp_path, "m.fq.gz", bgzf_bytes(data, block=1024))        # ~100 members: two GPU batches of 64
    eng.set_option("zb_members", 64)
    eng.set_option("stage_kb", 64)                                        # pieces of 64 KiB: maxreads falls inside one
    try:
        for maxreads in (1, 130, 391, 699, 5e9):
            want = big_want(big, 1, maxreads)
            assert want[1]["reads"] == min(maxreads, 700)
            check(device_rescue(eng, data, rc.BARCODES_MIXED, tags, maxreads=maxreads), want)
            for path in (plain, gz, bg):
                check(file_rescue(eng, path, rc.BARCODES_MIXED, tags, maxreads=maxreads), want)
    finally:
        eng.set_option("zb_members", 1 << 30)
        eng.set_option("stage_kb", 0)


# ----------------------------------------------------------------------------------------------------------- hot cell
def test_hot_cell(eng, tmp_path):
    rnd = random.Random(35)
    stored = rc.free_tags(rnd, [50] * 8)
    tags = ["TGCAG" + t for t in stored]
    one = "ACGTTGCAG" + rc.sub(stored[3], 17)
    two = "ACGTTGCAG" + rc.sub(stored[5], 44)
    def scaled(reads, n):
        """the restatement of one round of `reads`, n times over: the rule is per read"""
        rescued, st, positions, _ = rc.ref_rescue(rc.fastq(reads, quality=False), ["ACGT"], tags)
        return [[n * x for x in row] for row in rescued], {k: n * v for k, v in st.items()}, [n * x for x in positions], None
    data = rc.fastq([one] * 70000, quality=False)
    want = scaled([one], 70000)
    assert want[0][0][3] == 70000 and want[2][17] == 70000
    check(device_rescue(eng, data, ["ACGT"], tags), want)
    data = rc.fastq([one, two] * 35000, quality=False)                    # neighbouring lanes of every wave, two cells
    want = scaled([one, two], 35000)
    assert want[0][0][3] == want[0][0][5] == 35000
    check(device_rescue(eng, data, ["ACGT"], tags), want)
    check(file_rescue(eng, write(tmp_path, "hot.fq", data), ["ACGT"], tags), want)


# ----------------------------------------------------------------------------------------------------------- lifetime
def test_lifetime(eng, big):
    import tagdigger_amd
    from tagdigger_amd import TagdigError
    data, tags = big
    want = big_want(big)
    with pytest.raises(TagdigError) as ei:
        eng.rescue_end()                                                  # end without begin
    assert ei.value.code == -9
    for call in (eng.rescue_stats, eng.rescue_fetch, eng.rescue_matrix):
        with pytest.raises(TagdigError) as ei:
            call()
        assert ei.value.code == -9
    eng.rescue_begin(rc.BARCODES_MIXED, tags)
    run_pieces(eng, [(data, 0)])
    eng.rescue_begin(rc.BARCODES_MIXED, tags)                             # begin twice: the first is dropped, the matrix starts at zero
    assert fetched(eng)[1] == dict.fromkeys(rc.CLASSES, 0)
    run_pieces(eng, [(data, 0)])
    got = fetched(eng)
    check(got, want)
    # the matrix where it lies
    import numpy as np
    raw = eng.d2h(eng.rescue_matrix(), 4 * len(rc.BARCODES_MIXED) * len(tags))
    assert np.frombuffer(raw, dtype=np.uint32).reshape(len(rc.BARCODES_MIXED), len(tags)).tolist() == want[0]
    eng.rescue_end()
    # td_destroy with a rescue open
    other = tagdigger_amd.Engine(0)
    other.rescue_begin(rc.BARCODES_MIXED, tags, max_mismatch=2)
    d = other.dev_alloc(len(data))
    other.h2d(d, data)
    other.rescue_device(d, len(data))
    other.sync()
    other.dev_free(d)
    other.close()


def test_census_and_rescue_on_one_handle(eng, big):
    from census_cases import ordered, ref_census
    data, tags = big
    want = big_want(big, 2)
    cwant = ref_census(data, rc.BARCODES_MIXED, "TGCAG", 40)
    eng.census_begin(rc.BARCODES_MIXED, "TGCAG", 40, 4096)
    eng.rescue_begin(rc.BARCODES_MIXED, tags, max_mismatch=2)
    try:
        d = eng.dev_alloc(len(data))
        try:
            eng.h2d(d, data)
            eng.census_device(d, len(data))
            eng.rescue_device(d, len(data))
            eng.sync()
        finally:
            eng.dev_free(d)
        check(fetched(eng), want)
        assert list(eng.census_fetch()) == ordered(cwant[0])
        check(fetched(eng), want)
    finally:
        eng.census_end()
        eng.rescue_end()


def test_find_tags_fastq_untouched(big, tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    data, tags = big
    path = write(tmp_path, "u.fq", data)
    before = tf.find_tags_fastq(path, rc.BARCODES_MIXED, tags, progress=False)
    res = tf.rescue_tags_fastq(path, rc.BARCODES_MIXED, tags, max_mismatch=2)
    after = tf.find_tags_fastq(path, rc.BARCODES_MIXED, tags, progress=False)
    want = big_want(big, 2)
    assert res.backend == "gpu" and res.rescued == want[0] and res.positions == want[2]
    assert {k: res.stats[k] for k in rc.CLASSES} == want[1]
    assert before == after == want[3]                                     # the exact reads are the counter's
    arr = tf.rescue_tags_fastq(path, rc.BARCODES_MIXED, tags, max_mismatch=2, as_array=True).rescued
    assert arr.dtype.name == "uint32" and arr.tolist() == want[0]


def test_begin_errors_as_the_host_rule_names_them(eng):
    from tagdigger_amd import TagdigError
    for tags, bad in ((["AAAC", "GGGG", "AAAC"], 2), (["AAACT", "GGGG", "AAAC"], 2), (["AAAC", "GGGG", "AAACT"], 2),
                      (["AAACT", "AAAC", "AAACTT", "AAAC"], 1), (["CC", "AAACT", "GG", "AAACTT", "AAAC"], 3)):
        with pytest.raises(AssertionError) as ei:
            eng.rescue_begin(["ACGT"], ["TGCAG" + t for t in tags])
        assert str(ei.value) == "Problematic sequence: {}.  Likely due to overlapping tags.".format(bad)
    with pytest.raises(IndexError):
        eng.rescue_begin(["ACGT"], [])
    with pytest.raises(IndexError):
        eng.rescue_begin(["ACGT"], ["TGCAGAAAA", "TGCAG"])
    with pytest.raises(TagdigError) as ei:
        eng.rescue_begin(["ACGT"], ["TGCAG" + "A" * 129])
    assert ei.value.code == -7 and not ei.value.detail.startswith("tag rescue: run")
    with pytest.raises(TagdigError) as ei:
        eng._rescue_begin_lists(["ACGTTGCAG"], 1, [9], ["acgtacgt"], 1)
    assert ei.value.code == -6
    for K in (0, 3):
        with pytest.raises(TagdigError) as ei:
            eng.rescue_begin(["ACGT"], ["TGCAGAAAA"], max_mismatch=K)
        assert ei.value.code == -2
    with pytest.raises(TagdigError) as ei:
        eng.rescue_end()                                                  # none of them left a rescue behind
    assert ei.value.code == -9


def test_nonascii_kills_the_rescue_until_begin(eng):
    from tagdigger_amd import NonAsciiSequence
    tags = ["TGCAG" + "ACGTTGCATTGACCAGTTAC"]
    bad = rc.fastq(["ACGTTGCAGACGTTGCATTGACCAGTTAC"]) + b"@x\nACGTTGCAGAC\xe9TTGC\n+\nI\n"
    good = rc.fastq(["ACGTTGCAGACGTTGCATTGACCAGTTAA"])
    eng.rescue_begin(["ACGT"], tags)
    try:
        run_pieces(eng, [(bad, 0)])
        for _ in range(2):
            with pytest.raises(NonAsciiSequence):
                eng.rescue_stats()
        with pytest.raises(NonAsciiSequence):
            run_pieces(eng, [(good, 0)])
        eng.rescue_begin(["ACGT"], tags)
        run_pieces(eng, [(good, 0)])
        check(fetched(eng), rc.ref_rescue(good, ["ACGT"], tags))
    finally:
        eng.rescue_end()
