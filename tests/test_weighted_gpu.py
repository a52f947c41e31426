"""The weighted count on the device (tassel_tagcount=True: k_count<..., TASSEL=true>, its header parser and its
64-bit matrix) against the references of tests/weighted_cases.py, which tests/test_weighted.py has held against each
other.  Exact: the matrix as signed integers and reads / barcut / tag / lines, through count_bytes and count_file."""
import gzip

import pytest

import weighted_cases as wc
from helpers import bgzf_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    yield e
    e.close()


def run(eng, case, how, tmp_path):
    eng.set_index(case.barcodes, case.tags, case.cutsite)
    eng.reset()
    if how == "bytes":
        return eng.count_bytes(case.data, first_line=case.first_line, maxreads=case.maxreads, tassel_tagcount=True)
    assert case.first_line == 0
    path = tmp_path / ("w.fq.gz" if how.endswith("gz") else "w.fq")
    path.write_bytes(case.data if how == "file" else how_blob(how, case.data))
    eng.count_file(str(path), maxreads=case.maxreads, tassel_tagcount=True)
    return None


def how_blob(how, data):
    if how == "bgzf.gz":
        return bgzf_bytes(data, block=1024)              # with option zb_members 64: batches of 64 KiB
    if how == "members.gz":
        return b"".join(gzip.compress(data[i:i + 65536], compresslevel=1) for i in range(0, len(data), 65536))
    return gzip.compress(data, compresslevel=1)


def result(eng):
    st = eng.stats()
    return eng.counts_numpy(signed=True).tolist(), st


def check(eng, case, tmp_path, ref=None, hows=("bytes", "file")):
    """The case through each route against the reference (default: the literal Python rule)."""
    ref = ref or wc.py_reference(case)
    for how in hows:
        if how != "bytes" and case.first_line:
            continue
        lines = run(eng, case, how, tmp_path)
        if ref[0] == "raises":
            with pytest.raises(ref[1]):
                eng.counts()
            continue
        got, st = result(eng)
        assert got == ref[1], (case.name, how)
        assert {k: st[k] for k in ("reads", "barcut", "tag")} == {k: ref[2][k] for k in ("reads", "barcut", "tag")}, (case.name, how)
        assert st["lines"] == wc.line_count(case.data), (case.name, how)
        if lines is not None:
            assert lines == st["lines"]
    eng.reset()


# ------------------------------------------------------------------------------------------------ header grammar
@pytest.mark.parametrize("header,ok", wc.HEADERS, ids=lambda v: repr(v)[:24])
def test_header_grammar(eng, tmp_path, header, ok):
    """One record in one tile: the reference's expression, the C oracle, the kernel; errors are ValueError through
    find_tags_fastq."""
    from tagdigger_amd import tagdigger_fun as tf
    case = wc.Case("header", wc.G_BAR, wc.G_TAG, "TGCAG", (header + wc.G_BODY).encode("latin-1"))
    path = tmp_path / "h.fq"
    path.write_bytes(case.data)
    if ok:
        want = ("ok", [[wc.literal_rule(header)]], {"reads": 1, "barcut": 1, "tag": 1})
        assert wc.c_reference(case)[1] == want[1]
        check(eng, case, tmp_path, want)
        assert tf.find_tags_fastq(str(path), wc.G_BAR, wc.G_TAG, tassel_tagcount=True, progress=False) == want[1]
    else:
        with pytest.raises(ValueError):
            wc.literal_rule(header)
        assert wc.c_reference(case) == ("raises", ValueError)
        check(eng, case, tmp_path, ("raises", ValueError))
        with pytest.raises(ValueError):
            tf.find_tags_fastq(str(path), wc.G_BAR, wc.G_TAG, tassel_tagcount=True, progress=False)


def test_bad_header_behind_and_on_maxreads(eng, tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    behind, on = wc.maxreads_header_cases()
    assert wc.py_reference(behind)[0] == "ok" and wc.py_reference(on) == ("raises", ValueError)
    check(eng, behind, tmp_path)
    check(eng, on, tmp_path)
    path = tmp_path / "m.fq"
    path.write_bytes(on.data)
    assert tf.find_tags_fastq(str(path), wc.G_BAR, wc.G_TAG, maxreads=1, tassel_tagcount=True, progress=False) == [[3]]
    with pytest.raises(ValueError):
        tf.find_tags_fastq(str(path), wc.G_BAR, wc.G_TAG, maxreads=2, tassel_tagcount=True, progress=False)


# ------------------------------------------------------------------------------------------------ tile seams
def test_tile_seam_sweep(eng, tmp_path):
    """The boundary between the second and the third 16 KiB tile at every byte from a header's '@' -- through count=,
    its digits, between the \\r and the \\n -- to the first bases of the sequence line."""
    for pad in wc.SWEEP_PADS:
        check(eng, wc.tile_sweep_case(pad), tmp_path, hows=("bytes",) if pad % 8 else ("bytes", "file"))


# ------------------------------------------------------------------------------------------------ fuzz
@pytest.mark.parametrize("cutsite,nl", wc.FUZZ_SHAPES)
@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_vs_oracle(eng, tmp_path, cutsite, nl, seed):
    case = wc.fuzz_case(cutsite, nl, seed)
    check(eng, case, tmp_path, wc.c_reference(case))


@pytest.mark.parametrize("maxlen", wc.WIDTH_MAXLENS)
def test_all_tag_widths(eng, tmp_path, maxlen):
    case = wc.width_case(maxlen)
    check(eng, case, tmp_path, wc.c_reference(case))


# ------------------------------------------------------------------------------------------------ ends of the buffer
@pytest.mark.parametrize("case", wc.buffer_end_cases(), ids=lambda c: c.name)
def test_buffer_ends(eng, tmp_path, case):
    check(eng, case, tmp_path)


# ------------------------------------------------------------------------------------------------ maxreads, first_line
@pytest.mark.parametrize("case", wc.maxreads_cases(), ids=lambda c: c.name)
def test_maxreads(eng, tmp_path, case):
    ref = wc.py_reference(case)
    assert ref[2]["reads"] == min(case.maxreads, wc.py_reference(wc.limits_base())[2]["reads"])
    check(eng, case, tmp_path, ref)


@pytest.mark.parametrize("case", wc.first_line_cases(), ids=lambda c: c.name)
def test_first_line(eng, tmp_path, case):
    ref = wc.c_reference(case)
    assert ref[0] == "ok" and ref[1] == wc.py_reference(case)[1]
    check(eng, case, tmp_path, ref)


# ------------------------------------------------------------------------------------------------ the 64-bit matrix
def test_wide_and_negative_cells(eng, tmp_path):
    wide, neg = wc.wide_cases()
    check(eng, wide, tmp_path)
    check(eng, neg, tmp_path)
    run(eng, neg, "bytes", tmp_path)
    assert eng.counts(signed=True) == [[-7 - 2 ** 35]] and eng.counts() == [[2 ** 64 - 7 - 2 ** 35]]


def test_accumulate_reset_and_mixing(eng, tmp_path):
    case = wc.fuzz_case("TGCAG", ("\n",), 1)
    weighted = wc.c_reference(case)[1]
    from oracle import c_oracle
    plain = c_oracle.COracle(case.barcodes, case.tags, case.cutsite).count_bytes(case.data).astype("int64").tolist()
    assert plain != weighted
    twice = [[2 * v for v in row] for row in weighted]
    zero = [[0] * len(case.tags) for _ in case.barcodes]
    run(eng, case, "bytes", tmp_path)
    eng.count_bytes(case.data, tassel_tagcount=True)                    # two calls accumulate
    assert eng.counts(signed=True) == twice
    assert eng.stats()["reads"] == 2 * wc.c_reference(case)[2]["reads"]
    eng.reset()
    assert eng.counts(signed=True) == zero
    eng.count_bytes(case.data)                                          # weighted, reset, unweighted: the unweighted matrix
    assert eng.counts(signed=True) == plain
    eng.count_bytes(case.data, tassel_tagcount=True)                    # no reset in between: both are in the matrix
    assert eng.counts(signed=True) == [[a + b for a, b in zip(r, s)] for r, s in zip(plain, weighted)]
    eng.count_bytes(case.data)
    assert eng.counts(signed=True) == [[2 * a + b for a, b in zip(r, s)] for r, s in zip(plain, weighted)]
    # a new index starts from zero
    other = wc.width_case(20)
    eng.set_index(other.barcodes, other.tags, other.cutsite)
    assert eng.counts(signed=True) == [[0] * len(other.tags) for _ in other.barcodes]
    eng.count_bytes(other.data, tassel_tagcount=True)
    assert eng.counts(signed=True) == wc.c_reference(other)[1]
    eng.reset()


# ------------------------------------------------------------------------------------------------ piece seams
# route -> (how the bytes reach the library, records, the options that bring seams into a small input, their defaults,
# environment).  count_file's routes: csrc/tagdig.hip count_file_impl.
SEAM_ROUTES = {
    "host buffer": ("bytes", wc.SEAM_NREC, {"stage_kb": 64}, {"stage_kb": 0}, {}),                          # pump()
    "plain file": ("file", wc.SEAM_NREC, {"stage_kb": 64}, {"stage_kb": 0}, {}),                            # pump()
    "BGZF inflated on the device": ("bgzf.gz", wc.SEAM_NREC, {"zb_members": 64}, {"zb_members": 1 << 30}, {}),    # count_bgzf_gpu: batches of 64 KiB
    "BGZF inflated on the host": ("bgzf.gz", wc.SEAM_NREC, {"gpu_inflate": 0, "stage_kb": 64}, {"gpu_inflate": 1, "stage_kb": 0}, {}),   # pump()
    # count_gzip_dev: the chunk-parallel host decoder (also below 8 MiB); a batch closes at every member's end, 64 KiB of text
    "gzip decoded on the host, resolved on the device": (
        "members.gz", wc.SEAM_NREC, {}, {}, {"TAGDIG_PAR_INFLATE": "1", "TAGDIG_INFLATE_CHUNK": "3000", "TAGDIG_INFLATE_THREADS": "4"}),
    # count_gzip_gpu: 384 KiB of text in segments of 64 KiB of compressed bytes, which end where a DEFLATE block ends
    "gzip decoded on the device": (
        "one.gz", 3072, {"gz_gpu_min": 0, "gz_gpu_terr_kb": 16, "gz_gpu_seg_kb": 64, "gz_gpu_margin_kb": 64},
        {"gz_gpu_min": 8 << 20, "gz_gpu_terr_kb": 128, "gz_gpu_seg_kb": 1 << 20, "gz_gpu_margin_kb": 16384}, {"TAGDIG_PAR_INFLATE": "0"}),
}


@pytest.mark.parametrize("nl", ["\n", "\r\n"], ids=["lf", "crlf"])
@pytest.mark.parametrize("route", sorted(SEAM_ROUTES))
def test_piece_seams(eng, tmp_path, monkeypatch, route, nl):
    """Pieces of 64 KiB or less over a file of a little more than three 64 KiB pieces: the lead-in record moves the first
    boundary across every byte of a record, behind its header and between the header's \\r and \\n too.  Every record
    has a cell and a weight of its own."""
    how, nrec, options, defaults, env = SEAM_ROUTES[route]
    for k in ("TAGDIG_PAR_INFLATE", "TAGDIG_ZLIB", "TAGDIG_INFLATE_CHUNK", "TAGDIG_INFLATE_THREADS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for k, v in options.items():
        eng.set_option(k, v)
    bad = []
    try:
        for lead in wc.SEAM_LEADS:
            case = wc.seam_case(lead, nl, nrec)
            want = wc.seam_expected(case)
            run(eng, case, how, tmp_path)
            got = result(eng)
            if got != want:
                bad.append((lead, want[1]["reads"] - got[1]["reads"]))
            if route == "gzip decoded on the device":
                assert eng.last_gz_route() == 1
    finally:
        for k, v in defaults.items():
            eng.set_option(k, v)
    print("%s, %r: %d of %d alignments differ (lead-in, reads lost): %s" % (route, nl, len(bad), len(wc.SEAM_LEADS), bad[:12]))
    assert bad == []
