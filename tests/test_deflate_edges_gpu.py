"""The catalogue of tests/deflate_cases.py on the device: the wave decoder for ordinary gzip (csrc/gz_gpu.hpp: k_gz_find,
k_gz_tokens with its scalar path, k_gz_lz's five forms of copy, the windows chained in segments of 32 chunks, k_gz_resolve and
the CRC-32) and the lane decoder for BGZF members (csrc/gpu_inflate.hpp as the device builds it, its tables interleaved in
LDS).  Neither had seen a stream that zlib's encoder does not write.  tests/test_deflate_edges.py holds the same catalogue
against zlib and takes it through the host decoders.

The `device` rule (gz_gpu.hpp's header, GzGpuStream): the wave decoder may leave a valid file to the host only when it is under
64 bytes, has an incomplete literal/length code, has a chunk with more tokens than 4 * span + 4096, is made of small members,
or finds no room on the card.  Every other valid case must come back as bytes from td_gunzip_file_gpu, and td_count_file must
say that the device decoded it."""
import gzip
import zlib

import pytest

import deflate_cases as dc
from oracle import c_oracle

pytestmark = pytest.mark.gpu

CASES = dc.catalogue()
VALID, REFUSED = dc.valid_names(), dc.refused_names()
SMALL_VALID = [n for n in VALID if len(CASES[n].want) <= 65536 and len(CASES[n].raw) <= 65536 - 26]
SMALL_REFUSED = [n for n in REFUSED if len(CASES[n].trailer_text) <= 65536 and len(CASES[n].raw) <= 65536 - 26]
DEFAULTS = (("gz_gpu_terr_kb", 128), ("gz_gpu_verify", 0), ("gz_gpu_seg_kb", 1 << 20), ("gz_gpu_margin_kb", 16384))


@pytest.fixture(scope="module")
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    e.set_option("gz_gpu_min", 0)
    cfg = dc.synth_config()
    e.set_index(cfg.barcodes, cfg.tags, cfg.cutsite)
    yield e
    e.close()


_ORACLE = {}


def oracle(text, maxreads=None):
    """the counts and statistics of the plain text (computed once per text and bound)"""
    key = (zlib.crc32(text), len(text), maxreads)
    if key not in _ORACLE:
        cfg = dc.synth_config()
        st = {}
        kw = {} if maxreads is None else {"maxreads": maxreads}
        _ORACLE[key] = (c_oracle.COracle(cfg.barcodes, cfg.tags, cfg.cutsite).count_bytes(text, stats=st, **kw), st)
    return _ORACLE[key]


def check_counts(eng, text, what, maxreads=None):
    want, ost = oracle(text, maxreads)
    st = eng.stats()
    assert (eng.counts_numpy() == want).all(), what
    assert (st["reads"], st["barcut"], st["tag"]) == (ost["reads"], ost["barcut"], ost["tag"]), what


def write(tmp_path, blob, name="lib.fq.gz"):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(blob)
    return path


def restore(eng):
    for k, v in DEFAULTS:
        eng.set_option(k, v)


def text_and_counts(eng, path, c, what, maxreads=None):
    got = eng.gunzip_file_gpu(path, len(c.want) + 64)
    if c.device:
        assert got is not None, ("the device decoder left the file to the host", what)
        assert len(got) == len(c.want) and got == c.want, what
    else:
        assert got is None, (c.why, what)
    eng.reset()
    if maxreads is None:
        eng.count_file(path)
    else:
        eng.count_file(path, maxreads=maxreads)
    check_counts(eng, c.want, what, maxreads)
    assert eng.last_gz_route() == (1 if c.device else 0), what


@pytest.mark.parametrize("terr_kb", [16, 128])
@pytest.mark.parametrize("name", VALID)
def test_valid_streams(eng, tmp_path, monkeypatch, capfd, name, terr_kb):
    c = CASES[name]
    path = write(tmp_path, c.member())
    monkeypatch.setenv("TAGDIG_INFLATE_STATS", "1")
    try:
        eng.set_option("gz_gpu_terr_kb", terr_kb)
        capfd.readouterr()
        text_and_counts(eng, path, c, (name, terr_kb))
        if not c.device:
            assert c.why in capfd.readouterr().err                 # (the reason the decoder gives for leaving the file)
    finally:
        restore(eng)


def test_counts_are_not_all_zero():
    """(the literals are reads of the synthetic library: the comparison with the oracle is about something)"""
    for name in ("long-codes-max-tokens", "many-chunks", "decoy-in-stored", "dependent-copies", "stored-65535-then-copies"):
        want, ost = oracle(CASES[name].want)
        assert want.sum() > 0 and ost["reads"] > 0, name


@pytest.mark.parametrize("seg_kb,margin_kb", [(1 << 20, 16384), (128, 64), (64, 64)])
@pytest.mark.parametrize("verify", [0, 1])
@pytest.mark.parametrize("name", ["many-chunks", "decoy-in-stored"])
def test_many_chunks_and_decoys(eng, tmp_path, monkeypatch, capfd, name, verify, seg_kb, margin_kb):
    """Territories of 16 KiB: more than 40 chunks, so the windows go through k_gz_seg_windows as well as the walk of 32 chunks;
    segments of 128 and 64 KiB of compressed bytes, so the crafted blocks cross the seams between segments; maxreads inside the
    file.  The decoys are real false starts: without `verify` the block search takes them, the chunk in front runs past them and
    the stretch is decoded again -- the decoder says so under TAGDIG_INFLATE_STATS."""
    c = CASES[name]
    path = write(tmp_path, c.member())
    monkeypatch.setenv("TAGDIG_INFLATE_STATS", "1")
    try:
        eng.set_option("gz_gpu_terr_kb", 16)
        eng.set_option("gz_gpu_verify", verify)
        eng.set_option("gz_gpu_seg_kb", seg_kb)
        eng.set_option("gz_gpu_margin_kb", margin_kb)
        capfd.readouterr()
        got = eng.gunzip_file_gpu(path, len(c.want) + 64)
        err = capfd.readouterr().err
        assert got is not None and got == c.want, err[-2000:]
        if name == "decoy-in-stored" and verify == 0 and seg_kb == 1 << 20:
            assert "false block starts" in err, err[-2000:]
        if name == "many-chunks" and seg_kb == 1 << 20:
            import re
            assert int(re.search(r"(\d+) chunks", err).group(1)) > 40, err[-2000:]
        reads = c.want.count(b"\n") // 4
        for maxreads in (None, reads // 2 + 17):
            eng.reset()
            eng.count_file(path, **({} if maxreads is None else {"maxreads": maxreads}))
            check_counts(eng, c.want, (name, verify, seg_kb, maxreads), maxreads)
            assert eng.last_gz_route() == 1
    finally:
        restore(eng)


@pytest.mark.parametrize("name", REFUSED)
def test_refused_streams(eng, tmp_path, name):
    """What zlib refuses: never bytes from the device decoder; td_count_file ends as gzip.open ends, with nothing counted; and
    the next good file is the device decoder's again.  (The member's CRC-32 and length are those of the text a decoder
    without the check in question would give: they are not what refuses the stream.)"""
    from tagdigger_amd._binding import TagdigError
    c = CASES[name]
    path = write(tmp_path, c.member(), "bad.fq.gz")
    try:
        gzip.open(path).read()
        expected = None
    except (EOFError, OSError, zlib.error) as exc:
        expected = exc
    assert expected is not None
    try:
        for terr_kb in (16, 128):
            eng.set_option("gz_gpu_terr_kb", terr_kb)
            try:
                got = eng.gunzip_file_gpu(path, len(c.trailer_text) + 4096)
            except TagdigError:
                got = None
            assert got is None, name
        eng.reset()
        with pytest.raises(type(expected)) as ei:
            eng.count_file(path)
        assert type(ei.value) is type(expected), name
        st = eng.stats()
        assert eng.counts_numpy().sum() == 0 and (st["reads"], st["barcut"], st["tag"]) == (0, 0, 0)
        good = CASES["dependent-copies"]
        text_and_counts(eng, write(tmp_path, good.member()), good, ("after", name))
    finally:
        restore(eng)


# ---------------------------------------------------------------------------------------------- the lane decoder on the device
def lane_file(extra=None):
    """every valid case that fits a BGZF member, over and over until there are more than 64: the lanes of a wave each in a
    stream of another structure.  extra: a case to put in the middle (a refused one)."""
    names = SMALL_VALID * (64 // len(SMALL_VALID) + 1)
    if extra:
        names = names[:37] + [extra] + names[37:]
    assert len(names) > 64
    return dc.bgzf_file([dc.bgzf_member(CASES[n].raw, CASES[n].trailer_text) for n in names]), b"".join(CASES[n].trailer_text for n in names)


def test_lane_decoder_takes_every_structure_at_once(eng, tmp_path):
    blob, text = lane_file()
    assert set(SMALL_VALID) >= {"long-codes-small", "258-as-284-31", "dist-32768-exact", "one-distance-code", "no-distance-code",
                                "repeat-across-lit-dist", "empty-blocks-alignments", "overlapping-copies", "dependent-copies",
                                "empty-text-64", "only-end-code"}
    assert gzip.decompress(blob) == text
    path = write(tmp_path, blob)
    d = eng.dev_alloc(len(text) + 64)
    try:
        n = eng.bgzf_inflate_range(path, 0, len(blob), d, len(text))
        assert n == len(text)
        assert eng.d2h(d, n) == text
    finally:
        eng.dev_free(d)
    eng.reset()
    eng.count_file(path)
    check_counts(eng, text, "the BGZF file of every structure")


@pytest.mark.parametrize("name", SMALL_REFUSED)
def test_lane_decoder_refuses(eng, tmp_path, name):
    from tagdigger_amd._binding import TagdigError
    blob, text = lane_file(name)
    path = write(tmp_path, blob)
    try:
        gzip.open(path).read()
        expected = None
    except (EOFError, OSError, zlib.error) as exc:
        expected = exc
    assert expected is not None
    d = eng.dev_alloc(len(text) + 64)
    try:
        with pytest.raises(TagdigError):
            eng.bgzf_inflate_range(path, 0, len(blob), d, len(text))
    finally:
        eng.dev_free(d)
    eng.reset()
    with pytest.raises(type(expected)):
        eng.count_file(path)
