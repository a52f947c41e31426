"""MD5 on an MI355X (csrc/md5.hip): td_md5_device and td_md5_files against hashlib.md5, all 16 bytes equal, and
writeMD5sums through the device against the reference's recorded output (tests/golden/md5sums.json)."""
import hashlib
import random

import numpy as np
import pytest

import interactive_cases as ic

pytestmark = pytest.mark.gpu
MD5 = ic.load("md5sums.json")["cases"]
LENGTHS = [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128]


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd.engine import default_engine
    return default_engine(0)


def device_md5(eng, messages, lead=0):
    """td_md5_device over the messages laid end to end `lead` bytes into a device buffer."""
    data = b"\xa5" * lead + b"".join(messages)
    offs = np.zeros(len(messages) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in messages], out=offs[1:])
    offs += np.uint64(lead)
    d = eng.dev_alloc(len(data) + 64)
    try:
        if data:
            eng.h2d(d, data)
        got, _ = eng.md5_device(d, offs)
    finally:
        eng.dev_free(d)
    return got


def check(eng, messages, lead=0):
    got = device_md5(eng, messages, lead)
    want = [hashlib.md5(m).digest() for m in messages]
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (bad[:10], [len(messages[i]) for i in bad[:10]])


def test_device_rfc1321_and_seam_lengths(eng):
    rng = random.Random(1)
    check(eng, list(ic.RFC1321))
    check(eng, [rng.randbytes(n) for n in LENGTHS])
    for n in LENGTHS:                                    # each alone: n = 1
        check(eng, [rng.randbytes(n)])


@pytest.mark.parametrize("lead", [0, 1, 2, 3, 16])
def test_device_any_alignment(eng, lead):
    """Messages of every length 0 .. 200 end to end: every start alignment, with and without 16-byte aligned starts."""
    rng = random.Random(lead)
    check(eng, [rng.randbytes(n) for n in range(201)], lead)
    check(eng, [rng.randbytes(64 * k) for k in (1, 2, 3, 4)], lead)      # whole blocks only (aligned when lead % 16 == 0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 384, 1000])
def test_device_message_counts(eng, n):
    rng = random.Random(n)
    check(eng, [rng.randbytes(rng.randrange(0, 3000)) for _ in range(n)])


def test_device_random_lengths_some_empty(eng):
    rng = random.Random(300000)
    check(eng, [b"" if rng.randrange(5) == 0 else rng.randbytes(rng.randrange(0, 300001)) for _ in range(200)])


def test_device_one_long_among_short(eng):
    rng = random.Random(9)
    msgs = [rng.randbytes(rng.randrange(0, 500)) for _ in range(130)]
    msgs[70] = rng.randbytes(20_000_003)
    check(eng, msgs)


def test_device_no_messages(eng):
    got, _ = eng.md5_device(None, np.zeros(1, dtype=np.uint64))
    assert got == []


# ------------------------------------------------------------------ td_md5_files
def files_md5(eng, tmp_path, messages, piece):
    paths = []
    for k, m in enumerate(messages):
        p = tmp_path / ("m%04d.bin" % k)
        p.write_bytes(m)
        paths.append(str(p))
    eng.set_option("md5_piece", piece)
    try:
        got, ms = eng.md5_files(paths)
    finally:
        eng.set_option("md5_piece", 0)
    want = [hashlib.md5(m).digest() for m in messages]
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (piece, bad[:10], [len(messages[i]) for i in bad[:10]])
    return ms


@pytest.mark.parametrize("piece", [64, 128, 4096])
def test_files_piece_seams(eng, tmp_path, piece):
    """A small piece size, so that messages cross seams at P - 1, P, P + 1, a message's padding is split over two
    pieces (P - 8 .. P - 1: the 0x80 in one, the length in the next) and a message ends exactly on a seam, its last piece
    padding only (P, 2 P, 3 P); with the seam lengths of the blocks themselves."""
    rng = random.Random(piece)
    lens = set(LENGTHS)
    for k in (1, 2, 3):
        lens |= {k * piece + d for d in range(-10, 3)} | {k * piece - 56, k * piece - 55, k * piece - 64, k * piece + 55,
                                                          k * piece + 56}
    lens |= {5 * piece + 17, 0}
    files_md5(eng, tmp_path, [rng.randbytes(n) for n in sorted(x for x in lens if x >= 0)], piece)


def test_files_default_piece(eng, tmp_path):
    """The built-in piece (1 MiB): files below, at, just over and several times that size, and empty ones; 70 files."""
    rng = random.Random(5)
    sizes = [0, 1, (1 << 20) - 9, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 3 * (1 << 20) + 77, 0] + \
            [rng.randrange(0, 200000) for _ in range(62)]
    block = rng.randbytes(1 << 16)
    msgs = [(block * (n // len(block) + 1))[:n] for n in sizes]
    ms = files_md5(eng, tmp_path, msgs, 0)
    assert len(ms) == 3 and all(x >= 0 for x in ms) and ms[2] > 0


@pytest.mark.parametrize("n", [1, 65, 384])
def test_files_counts(eng, tmp_path, n):
    rng = random.Random(n)
    files_md5(eng, tmp_path, [rng.randbytes(rng.randrange(0, 5000)) for _ in range(n)], 1024)


def test_files_missing_file(eng, tmp_path):
    from tagdigger_amd import TagdigError
    paths = []
    for k in range(6):
        p = tmp_path / ("f%d.bin" % k)
        if k not in (2, 4):
            p.write_bytes(b"x" * (100 * k))
        paths.append(str(p))
    with pytest.raises(TagdigError) as e:
        eng.md5_files(paths)
    assert e.value.code == -11 and e.value.bad_index == 2 and "f2.bin" in str(e.value)
    got, _ = eng.md5_files(paths[:2])                       # the engine is usable afterwards
    assert got == [hashlib.md5(b"").digest(), hashlib.md5(b"x" * 100).digest()]


# ------------------------------------------------------------------ writeMD5sums through the device
@pytest.mark.parametrize("golden", MD5, ids=lambda c: c["name"])
def test_write_md5sums_device(golden, tmp_path, monkeypatch):
    """The device route (the threshold forced to 1) answers to the reference's recorded CSV, stdout and exception."""
    ic.check_md5_case(golden, golden, tmp_path, "gpu", monkeypatch, threshold=1)


def test_write_md5sums_device_is_used(tmp_path, monkeypatch):
    """With the threshold at 1, writeMD5sums goes through Engine.md5_files."""
    from tagdigger_amd import engine, tagdigger_fun as tf
    calls = []
    real = engine.Engine.md5_files
    monkeypatch.setattr(engine.Engine, "md5_files", lambda self, paths: calls.append(len(paths)) or real(self, paths))
    monkeypatch.setattr(tf, "_MD5_DEVICE_MIN_FILES", 1)
    p = tmp_path / "a.bin"
    p.write_bytes(b"abc")
    tf.writeMD5sums([str(p)], str(tmp_path / "o.csv"))
    assert calls == [1]
    assert (tmp_path / "o.csv").read_bytes().endswith(b",900150983cd24fb0d6963f7d28e17f72\r\n")


def test_write_md5sums_default_threshold(tmp_path, monkeypatch):
    """As shipped: a list as long as the measured threshold goes to the device, a list one shorter to the host pool."""
    from tagdigger_amd import engine, tagdigger_fun as tf
    calls = []
    real = engine.Engine.md5_files
    monkeypatch.setattr(engine.Engine, "md5_files", lambda self, paths: calls.append(len(paths)) or real(self, paths))
    n = tf._MD5_DEVICE_MIN_FILES
    assert n == 384
    rng = random.Random(384)
    names = []
    for k in range(n):
        p = tmp_path / ("s%03d.fq" % k)
        p.write_bytes(rng.randbytes(rng.randrange(0, 3000)))
        names.append(str(p))
    want = b"".join(("%s,%s\r\n" % (f, hashlib.md5(open(f, "rb").read()).hexdigest())).encode() for f in names)
    tf.writeMD5sums(names, str(tmp_path / "long.csv"))
    assert calls == [n]
    assert (tmp_path / "long.csv").read_bytes() == b"File name,MD5 sum\r\n" + want
    tf.writeMD5sums(names[:-1], str(tmp_path / "short.csv"))
    assert calls == [n]
    assert (tmp_path / "short.csv").read_bytes() == b"File name,MD5 sum\r\n" + want[:want.rindex(names[-1].encode())]
