"""exp_frag_size on an MI355X: every golden case through the device path, K1 (genome framing) against Python's own
text-mode reading on texts built to stress tile seams, K2 / K3 (search, gather) against str slicing and str.find on
random windows, and one 256 MB / 100 k-tag run compared byte for byte with the host backend.

The independent check here is the test-local restatement (io.TextIOWrapper with universal newlines, str.strip,
str.upper, str.find): nothing of the product's search code is imported for it."""
import io
import os
import random

import numpy as np
import pytest

from fragsize_cases import CASES, run_case, unpack

pytestmark = pytest.mark.gpu

TILE = 32768          # K1's bytes per workgroup (csrc/fragsize.hip); seams every 16 and 128 bytes inside it


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_device(case, tmp_path, monkeypatch, capsys):
    run_case(case, tmp_path, monkeypatch, capsys, [])


def test_golden_took_the_device_path(tmp_path, monkeypatch, capsys):
    """An ASCII genome with non-empty cut sites is framed and searched on the device, not by the host restatement."""
    from tagdigger_amd import exp_frag_size
    case = next(c for c in CASES if c["name"] == "many_tags")
    for name, b64 in case["files"].items():
        (tmp_path / name).write_bytes(unpack(b64))
    monkeypatch.chdir(tmp_path)
    stages, stage_ms = exp_frag_size.run(exp_frag_size.build_parser().parse_args(case["args"]))
    assert any(name == "genome (gpu)" for name, _ in stages)
    assert {"K1", "K2", "K3"} <= set(stage_ms)


# ------------------------------------------------------------------ K1
def restate_frame(data):
    """What the reference's loop keeps of a genome file: Python's text-mode lines, headers, strip().upper()."""
    seq, recs, n = [], [], 0
    for line in io.TextIOWrapper(io.BytesIO(data), encoding="ascii", newline=None):
        if line[0] == ">":
            recs.append((line[1:].strip(), n))
        else:
            s = line.strip().upper()
            seq.append(s)
            n += len(s)
    return "".join(seq).encode(), recs


def seam_text(rng, size):
    """Random FASTA-like text with terminators, whitespace runs and headers planted on 16-, 128- and tile seams, lines
    longer than a tile, and \\r\\n pairs split by seams."""
    words = [b"ACGT", b"acgtn", b"NNNN", b"RYKM", b" ", b"\t", b"\x0b\x0c\x1c\x1d\x1e\x1f", b"  \t ", b"\n", b"\r\n", b"\r",
             b"\n\n", b">chr%d desc\n", b">  s%d \t\r\n", b">\n", b"\r\r\n\n", b"x=y;"]
    out = bytearray()
    while len(out) < size:
        r = rng.random()
        if r < 0.05:
            out += bytes(rng.choice(b"ACGTacgtN") for _ in range(rng.randrange(TILE, 2 * TILE + 100)))   # a long line
        else:
            w = rng.choice(words)
            out += (w % rng.randrange(1000)) if b"%d" in w else w
            if rng.random() < 0.5:
                out += bytes(rng.choice(b"ACGTacgtN") for _ in range(rng.randrange(1, 200)))
    out = out[:size]
    for seam in range(16, len(out) - 2, 16):
        if seam % 128 and rng.random() < 0.9:
            continue
        k = rng.randrange(8)
        if k == 0:
            out[seam - 1:seam + 1] = b"\r\n"          # the pair split by the seam
        elif k == 1:
            out[seam - 1] = ord("\r")
        elif k == 2:
            out[seam] = ord("\n")
        elif k == 3:
            out[seam - 1:seam + 1] = b"\n>"           # a header starting on the seam
        elif k == 4:
            out[seam - 2:seam + 2] = b"  \t "         # whitespace across the seam
        elif k == 5:
            out[seam - 1:seam + 1] = b"\r>"
    return bytes(out)


def frame_on_device(eng, data, out_shift=3):
    n = len(data)
    d_in = eng.dev_alloc(n + 16)
    d_out = eng.dev_alloc(n + 32)
    try:
        eng.h2d(d_in, data)
        nout, rows, nonascii, _ = eng.fasta_frame_device(d_in, n, d_out + out_shift, 4)
        got = eng.d2h(d_out + out_shift, nout)
    finally:
        eng.dev_free(d_in)
        eng.dev_free(d_out)
    return got, rows, nonascii


@pytest.mark.parametrize("seed", range(24))
def test_k1_seams_against_text_mode(eng, seed):
    rng = random.Random(seed)
    size = rng.choice([1, 15, 16, 17, 127, 129, TILE - 1, TILE, TILE + 1, 3 * TILE + rng.randrange(TILE), 200000])
    data = seam_text(rng, size)
    want_seq, want_recs = restate_frame(data)
    got, rows, nonascii = frame_on_device(eng, data, out_shift=seed % 16)
    assert not nonascii
    assert got == want_seq
    got_recs = [(data[lo:hi].decode(), off) for lo, hi, off in rows.tolist()]
    assert got_recs == want_recs


def test_k1_unwrapped_and_edge_cases(eng):
    rng = random.Random(99)
    chrom = bytes(rng.choice(b"ACGTacgt") for _ in range(5 * TILE + 77))
    for data in [b"", b">", b"\r", b"\r\n", b"\n>a\n", b" a ", b">x\r\n  acg t \r\n\r>y", b">h\n" + chrom,
                 b"pre\n>h \t\n" + chrom + b"\r\n>t\n" + chrom[:100], b"\x1c\x1dA\x1e\x1f", b"A" * (TILE * 2) + b"\r",
                 b"\r" * TILE + b"\n" * TILE, b" " * (3 * TILE) + b"C" + b" " * TILE]:
        want_seq, want_recs = restate_frame(data)
        got, rows, nonascii = frame_on_device(eng, data)
        assert not nonascii
        assert got == want_seq
        assert [(data[lo:hi].decode(), off) for lo, hi, off in rows.tolist()] == want_recs


def test_k1_flags_non_ascii(eng):
    data = b">a\nACGT\n" * 5000 + "é".encode() + b"\nACGT\n"
    _, _, nonascii = frame_on_device(eng, data)
    assert nonascii


# ------------------------------------------------------------------ K2 / K3
def restate_search(seq, lo, hi, rev, tagsize, sites):
    sub = seq[lo:hi]
    if rev:
        sub = sub.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    best = None
    for cs in sites:
        k = sub.find(cs, tagsize - len(cs))
        if k != -1 and (best is None or k + len(cs) < best):
            best = k + len(cs)
    if best is None:
        return -1, 0, 0, ""
    frag = sub[:best]
    return best, frag.count("G") + frag.count("C"), frag.count("N"), frag


@pytest.mark.parametrize("seed", range(4))
def test_k2_k3_against_find(eng, seed):
    from tagdigger_amd.engine import frag_job_dtype
    rng = random.Random(1000 + seed)
    seq = "".join(rng.choice("ACGTACGTACGTNRY") for _ in range(200000))
    for cs in ("CCGCCG", "CCGG", "CTGCAG"):
        for p in rng.sample(range(len(seq) - 10), 300):
            seq = seq[:p] + cs + seq[p + len(cs):]
    pool = ["CCGCCG", "CCGG", "CTGCAG", "GCGC", "AAAA", "CGCG", "ATAT", "C", "GG", "ACGTACGTACGTACGTACGTACGTACGTACGTA"]
    sites = rng.sample(pool, rng.randrange(1, len(pool) + 1))
    while len(sites) < 16 and seed == 3:
        sites.append("".join(rng.choice("ACGT") for _ in range(rng.randrange(1, 64))))
    njobs = 5000
    jobs = np.zeros(njobs, dtype=frag_job_dtype())
    want = []
    for j in range(njobs):
        lo = rng.randrange(len(seq))
        hi = min(len(seq), lo + rng.choice([0, 1, 5, 64, 500, 3000, 3001, rng.randrange(3002)]))
        rev = rng.random() < 0.5
        ts = rng.choice([0, 1, 3, 6, 64, 100, 2995, 3001, 3100, rng.randrange(200)])
        jobs[j] = (lo, hi, ts, int(rev), 0)
        want.append(restate_search(seq, lo, hi, rev, ts, sites))
    d = eng.dev_alloc(len(seq) + 16)
    try:
        eng.h2d(d, seq.encode())
        out, _ = eng.frag_search_device(d, len(seq), jobs, sites)
        assert [tuple(r[:3]) for r in out.tolist()] == [w[:3] for w in want]
        found = np.flatnonzero(out[:, 0] >= 0)
        blob, _ = eng.frag_gather_device(d, len(seq), jobs[found], out[found, 0])
    finally:
        eng.dev_free(d)
    assert blob.decode() == "".join(want[j][3] for j in found.tolist())


# ------------------------------------------------------------------ scale
def test_scale_256mb_100k_tags_device_equals_host(tmp_path, monkeypatch, capsys):
    from tagdigger_amd import exp_frag_size
    rng = np.random.default_rng(7)
    nchrom, clen = 8, 32 << 20
    with open(tmp_path / "genome.fa", "wb") as fh:
        for c in range(nchrom):
            s = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, clen, dtype=np.uint8) % 9]
            fh.write(b">chr%d scaffold\n" % c if c == 5 else b">chr%d\n" % c)
            if c == 3:
                fh.write(s.tobytes() + b"\n")                      # one unwrapped chromosome
            else:
                rows = s[:clen - clen % 60].reshape(-1, 60)
                fh.write(np.hstack([rows, np.full((rows.shape[0], 1), 10, np.uint8)]).tobytes())
                fh.write(s[clen - clen % 60:].tobytes() + b"\r\n")
    ntags = 100000
    chrom = rng.integers(0, nchrom + 1, ntags)
    pos = rng.integers(-5, clen + 5, ntags)
    flag = rng.choice([0, 16, 4, 20], ntags)
    with open(tmp_path / "tags.sam", "w") as fh:
        fh.write("@HD\tVN:1.0\n")
        for i in range(ntags):
            fh.write("tag%d\t%d\tchr%d\t%d\t40\t%s\t*\t0\t0\t%s\t*\n" % (
                i, flag[i], chrom[i], pos[i], "3S61M" if i % 7 == 0 else "64M", "ACGT" * 16))
    monkeypatch.chdir(tmp_path)
    parser = exp_frag_size.build_parser()
    outs = {}
    for backend in ("gpu", "host"):
        capsys.readouterr()
        stages, _ = exp_frag_size.run(parser.parse_args(["-s", "tags.sam", "-g", "genome.fa", "-o", backend + ".csv",
                                                         "--td-backend", backend]))
        assert any(name == "genome (%s)" % backend for name, _ in stages)
        outs[backend] = (capsys.readouterr().out, (tmp_path / (backend + ".csv")).read_bytes())
    assert outs["gpu"][0] == outs["host"][0] and outs["gpu"][0].count("\n") >= 50
    assert outs["gpu"][1] == outs["host"][1]
    assert outs["gpu"][1].count(b"\r\n") == ntags + 1
    os.remove(tmp_path / "genome.fa")
