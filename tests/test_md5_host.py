"""writeMD5sums on the host route and remove_monomorphic_loci against what the reference did (tests/golden/md5sums.json,
tests/golden/interactive.json; recorded by tests/golden/make_interactive_golden.py).  No GPU."""
import hashlib

import pytest

import interactive_cases as ic

MD5 = ic.load("md5sums.json")["cases"]
MONO = ic.load("interactive.json")["remove_monomorphic_loci"]


def test_golden_covers_the_cases_defined():
    assert [c["name"] for c in MD5] == [c["name"] for c in ic.md5_cases()]
    for g, c in zip(MD5, ic.md5_cases()):
        assert g["filelist"] == c["filelist"]
        assert {k: ic.unpack(v) for k, v in g["files"].items()} == c["files"]
    lens = next(c for c in ic.md5_cases() if c["name"] == "block_seam_lengths")
    assert sorted(len(v) for v in lens["files"].values()) == [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128]


def test_rfc1321_vectors_recorded():
    """The recorded sums of the seven test vectors are the ones RFC 1321 prints (appendix A.5)."""
    want = ["d41d8cd98f00b204e9800998ecf8427e", "0cc175b9c0f1b6a831c399e269772661", "900150983cd24fb0d6963f7d28e17f72",
            "f96b697d7cb7938d525a2f31aaf161d0", "c3fcd3d76192e4007dfb496cca67e13b", "d174ab98d277d9f5a5611c2c9f419d9f",
            "57edf4a22be3c955ac49da2e2107b67a"]
    g = next(c for c in MD5 if c["name"] == "rfc1321_vectors")
    assert [line.split()[-1] for line in g["stdout"].splitlines()] == want
    assert [hashlib.md5(v).hexdigest() for v in ic.RFC1321] == want


@pytest.mark.parametrize("golden", MD5, ids=lambda c: c["name"])
def test_write_md5sums_host(golden, tmp_path):
    ic.check_md5_case(golden, golden, tmp_path, "host")


def test_write_md5sums_short_list_stays_on_the_host(tmp_path):
    """backend="gpu" with a list shorter than the device threshold hashes on the host: no GPU is needed."""
    from tagdigger_amd import tagdigger_fun as tf
    golden = next(c for c in MD5 if c["name"] == "rfc1321_vectors")
    assert tf._MD5_DEVICE_MIN_FILES is None or len(golden["filelist"]) < tf._MD5_DEVICE_MIN_FILES
    ic.check_md5_case(golden, golden, tmp_path, "gpu")


def test_write_md5sums_rejects_unknown_backend(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    with pytest.raises(ValueError):
        tf.writeMD5sums(["x"], str(tmp_path / "o.csv"), backend="cuda")
    assert not (tmp_path / "o.csv").exists()


def test_write_md5sums_many_files_in_list_order(tmp_path):
    """More files than pool threads, of sizes around the host route's read size: rows stay in list order."""
    from tagdigger_amd import tagdigger_fun as tf
    names = []
    for k in range(40):
        p = tmp_path / ("f%02d.bin" % (39 - k))
        p.write_bytes(bytes([k]) * (k * 1000))
        names.append(str(p))
    out = tmp_path / "sums.csv"
    tf.writeMD5sums(names, str(out), backend="host")
    rows = out.read_bytes().split(b"\r\n")
    assert rows[0] == b"File name,MD5 sum" and rows[-1] == b""
    assert rows[1:-1] == [("%s,%s" % (n, hashlib.md5(open(n, "rb").read()).hexdigest())).encode() for n in names]


@pytest.mark.parametrize("k", range(len(MONO)))
def test_remove_monomorphic_loci(k):
    from tagdigger_amd import tagdigger_fun as tf
    assert MONO[k]["args"] == ic.MONO_CASES[k]
    names, seqs, verbose = MONO[k]["args"]
    got = ic.call_recorded(tf.remove_monomorphic_loci, [names, seqs], {"verbose": verbose})
    want = {key: MONO[k][key] for key in ("result", "raises", "message", "stdout") if key in MONO[k]}
    assert got == want
