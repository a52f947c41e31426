"""VCF body lines formatted on the device (csrc/vcf.hip) against the brute force of tests/vcf_cases.py."""
import csv
import random

import numpy as np
import pytest

import dosage_cases as dc
import genocall_cases as gc
import vcf_cases as vc

pytestmark = pytest.mark.gpu

TD_E_ARG, TD_E_LIMIT, TD_E_IO = -2, -7, -11
U32 = vc.U32


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def sizes():
    """(sample counts, line counts) from the engine's constants: one chunk short, full, one over, three chunks; the tiles
    of the emit and of the measure kernel one short, full, one over, and two with three over."""
    from tagdigger_amd.engine import VCF_CHUNK, VCF_MTILE, VCF_TILE
    S = [1, VCF_CHUNK - 1, VCF_CHUNK, VCF_CHUNK + 1, 2 * VCF_CHUNK + 2]
    K = sorted({1, 63, 64, 65} | {k for t in (VCF_TILE, VCF_MTILE) for k in (t - 1, t, t + 1, 2 * t + 3)})
    return S, K


def as_calls(calls, M):
    return np.array(calls, dtype=np.uint8).reshape(len(calls), M)


def run(eng, counts, T, i0, i1, calls, sel, prefixes, P, lik=False, CA=None, CB=None, **kw):
    if lik and CA is None:
        CA, CB = vc.tables(10000)
    return eng.vcf_format(gc.as_array(counts, T), as_calls(calls, len(i0)), i0, i1, sel, prefixes, ploidy=P, likelihoods=lik, ca=CA, cb=CB, **kw)


def check(got, ref):
    """The text and the line offsets of a VcfText against the reference lines."""
    text = b"".join(ref)
    assert got.nbytes == len(text)
    assert got.line_off.tolist() == vc.offsets(ref)
    assert got.text == text


@pytest.mark.parametrize("layout", vc.LAYOUTS)
@pytest.mark.parametrize("mode", sorted(vc.MODES))
def test_device_equals_brute_force(eng, mode, layout):
    Ss, Ks = sizes()
    assert Ss == [1, 63, 64, 65, 130] and Ks == [1, 63, 64, 65, 131, 255, 256, 257, 515]
    P, lik = vc.MODES[mode]
    M = max(Ks)
    for S in Ss:
        counts, i0, i1, T, calls, prefixes, ref = vc.grid_case(S, M, layout, mode)
        for K in Ks:
            got = run(eng, counts, T, i0, i1, calls, list(range(K)), prefixes[:K], P, lik)
            check(got, ref[:K])
            assert got.ms["measure"] > 0 and got.ms["emit"] > 0


DIGITS = [0, 9] + [v for e in range(1, 9) for v in (10 ** e, 10 ** (e + 1) - 1)] + [10 ** 9, U32]


@pytest.mark.parametrize("mode", sorted(vc.MODES))
def test_digit_widths(eng, mode):
    """Both alleles at every digit width, in every pairing: sample s has a = DIGITS[s], marker m has b = DIGITS[m]."""
    assert DIGITS[:6] == [0, 9, 10, 99, 100, 999] and DIGITS[-3:] == [10 ** 9 - 1, 10 ** 9, U32] and len(DIGITS) == 20
    P, lik = vc.MODES[mode]
    n = len(DIGITS)
    counts = [[DIGITS[s] if c % 2 == 0 else DIGITS[c // 2] for c in range(2 * n)] for s in range(n)]
    i0, i1, T = gc.adjacent(n)
    calls = vc.random_calls(random.Random(3), n, n, P)
    prefixes = [vc.prefix_bytes(k, 5) for k in range(n)]
    CA, CB = vc.tables(10000) if lik else (None, None)
    ref = vc.lines(counts, i0, i1, calls, range(n), prefixes, P, lik, CA, CB)
    assert (":%d,%d:%d" % (U32, U32, 2 ** 33 - 2)).encode() in ref[-1]
    check(run(eng, counts, T, i0, i1, calls, list(range(n)), prefixes, P, lik), ref)


@pytest.mark.parametrize("width", ["min", "max", "max_lik"])
def test_alignment(eng, width):
    """Prefix lengths 0 .. 32, the empty prefix included, with every cell at its minimum or at its maximum width: the
    lines, and with them every chunk's LDS segment, start at every residue mod 16."""
    P, lik, value, code = {"min": (2, False, 0, 0), "max": (8, False, U32, 4), "max_lik": (2, True, U32, 1)}[width]
    S, M = 70, 3
    counts = [[value] * (2 * M) for _ in range(S)]
    i0, i1, T = gc.adjacent(M)
    calls = [[code] * M for _ in range(S)]
    sel = [k % M for k in range(99)]
    prefixes = [vc.prefix_bytes(k, k % 33) for k in range(99)]
    CA, CB = vc.tables(10000) if lik else (None, None)
    ref = vc.lines(counts, i0, i1, calls, sel, prefixes, P, lik, CA, CB)
    cell = len(ref[0]) - 1
    assert cell == S * {"min": 10, "max": 49, "max_lik": 50}[width]
    assert {o % 16 for o in vc.offsets(ref)} == set(range(16))
    assert {(o + len(p) + 64 * cell // S) % 16 for o, p in zip(vc.offsets(ref), prefixes)} == set(range(16))      # the second chunk's start
    check(run(eng, counts, T, i0, i1, calls, sel, prefixes, P, lik), ref)


@pytest.mark.parametrize("mode", sorted(vc.MODES))
def test_codes(eng, mode):
    P, lik = vc.MODES[mode]
    codes = list(range(P + 1)) + [P + 1, 3, 255]
    counts = [[7 + s, 2 * s] for s in range(len(codes))]
    ref = vc.lines(counts, [0], [1], [[c] for c in codes], [0], [b"x"], P, lik, *(vc.tables(10000) if lik else (None, None)))
    if P == 2:
        assert b"\t0/0:" in ref[0] and b"\t0/1:" in ref[0] and b"\t1/1:" in ref[0] and ref[0].count(b"\t./.:") == 3
    else:
        assert ref[0].count(("\t" + "/".join(["."] * P) + ":").encode()) == 2 and ("\t" + "/".join(["0"] * (P - 3) + ["1"] * 3) + ":").encode() in ref[0]
    check(run(eng, counts, 2, [0], [1], [[c] for c in codes], [0], [b"x"], P, lik), ref)


def test_sel_orders(eng):
    counts, i0, i1, T, calls, prefixes, ref = vc.grid_case(65, 515, "adjacent", "p2lik")
    M = 130
    for sel in (list(reversed(range(M))), [3, 3, 3, 7, 0, 7, 129, 129], list(range(1, M, 3))):
        pre = [vc.prefix_bytes(k, (5 * k) % 23) for k in range(len(sel))]
        want = [pre[k] + ref[m][len(prefixes[m]):] for k, m in enumerate(sel)]
        check(run(eng, counts, T, i0, i1, calls, sel, pre, 2, True), want)


def pl_edge(d):
    return (d * 30103 + 327680000) // 655360000


def test_pl_edges(eng):
    """Tables handed in as data.  CB = [0, d, d], CA = 0 and one read of allele 0: PL = [0, r(d), r(d)] with the rounding
    step between d = 10885 and 10886, and the step 254 -> 255; the caps; GQ = 0; the scaling above 127 reads."""
    assert pl_edge(10885) == 0 and pl_edge(10886) == 1
    d255 = -(-(255 * 655360000 - 327680000) // 30103)
    assert pl_edge(d255 - 1) == 254 and pl_edge(d255) == 255 and d255 <= vc.COST_MAX
    for d, text in ((10885, b"0/0:1,0:1:0:0,0,0"), (10886, b"0/0:1,0:1:1:0,1,1"), (d255 - 1, b"0/0:1,0:1:99:0,254,254"),
                    (d255, b"0/0:1,0:1:99:0,255,255"), (vc.COST_MAX, b"0/0:1,0:1:99:0,255,255")):
        CA, CB = [0, 0, 0], [0, d, d]
        # (1, 0) called 0; (1, 0) called 2: not the cheapest genotype, GQ = 0; (127, 0): capped; (1000, 24): scaled to (124, 2)
        counts = [[1, 0], [1, 0], [127, 0], [1000, 24], [0, 5]]
        calls = [[0], [2], [0], [0], [3]]
        ref = vc.lines(counts, [0], [1], calls, [0], [b""], 2, True, CA, CB)
        cells = ref[0][1:-1].split(b"\t")
        assert cells[0] == text and cells[1].split(b":")[3] == b"0" and cells[4] == b"./.:0,5:5:.:."
        assert vc.scaled(1000, 24) == (124, 2) and cells[3] == ("0/0:1000,24:1024:%d:0,%d,%d" % (min(99, min(255, pl_edge(124 * d))),
                                                                                             min(255, pl_edge(124 * d)), min(255, pl_edge(124 * d)))).encode()
        check(run(eng, counts, 2, [0], [1], calls, [0], [b""], 2, True, CA, CB), ref)
    # GQ between the caps: PL = [0, 40, 119] called 0 -> GQ 40; called 1 -> GQ 0
    dq = next(d for d in range(1, vc.COST_MAX) if pl_edge(d) == 40)
    CA, CB = [0, 0, 0], [0, dq, 3 * dq]
    ref = vc.lines([[1, 0], [1, 0]], [0], [1], [[0], [1]], [0], [b"p"], 2, True, CA, CB)
    assert pl_edge(3 * dq) == 119 and ref[0] == b"p\t0/0:1,0:1:40:0,40,119\t0/1:1,0:1:0:0,40,119\n"
    check(run(eng, [[1, 0], [1, 0]], 2, [0], [1], [[0], [1]], [0], [b"p"], 2, True, CA, CB), ref)


@pytest.fixture(scope="module")
def range_case():
    counts, i0, i1, T, calls, prefixes, ref = vc.grid_case(65, 515, "scattered", "p2")
    K = 40
    prefixes, ref = list(prefixes[:K]), list(ref[:K])
    long_one = vc.prefix_bytes(7, 3000)                    # one line far longer than the others
    ref[7] = long_one + ref[7][len(prefixes[7]):]
    prefixes[7] = long_one
    return counts, i0, i1, T, calls, list(range(K)), prefixes, ref


def test_ranges(eng, range_case, tmp_path):
    from tagdigger_amd import TagdigError
    counts, i0, i1, T, calls, sel, prefixes, ref = range_case
    lengths = [len(x) for x in ref]
    text = b"".join(ref)
    check(run(eng, counts, T, i0, i1, calls, sel, prefixes, 2), ref)
    arr, cal = gc.as_array(counts, T), as_calls(calls, len(i0))
    path = str(tmp_path / "body.vcf")
    three = sum(lengths[:3])
    assert lengths[3] > 1 and lengths[7] > 3000 and max(lengths[:7] + lengths[8:]) < 1250
    budgets = {"one line each": 1, "hit exactly": three, "missed by one byte": three - 1, "one line longer": 2500, "default": 0}
    for name, budget in budgets.items():
        plan = vc.plan(lengths, budget or vc.DEFAULT_RANGE)
        if name == "one line each":
            assert len(plan) == len(ref)
        if name == "hit exactly":
            assert plan[0] == (0, 3)
        if name == "missed by one byte":
            assert plan[0] == (0, 2)
        if name == "one line longer":
            assert any(e - b == 1 and lengths[b] > budget for b, e in plan) and any(e - b > 1 for b, e in plan)
        if name == "default":
            assert plan == [(0, len(ref))]
        with open(path, "wb") as fh:
            fh.write(b"old contents that are longer than nothing\n" * 3)
        got = eng.vcf_file(path, arr, cal, i0, i1, sel, prefixes, ploidy=2, range_bytes=budget, append=False)
        assert (got.ranges, got.nbytes) == (len(plan), len(text)), name
        with open(path, "rb") as fh:
            assert fh.read() == text, name
        with open(path, "wb") as fh:
            fh.write(b"#header\n")
        got = eng.vcf_file(path, arr, cal, i0, i1, sel, prefixes, ploidy=2, range_bytes=budget, append=True)
        with open(path, "rb") as fh:
            assert fh.read() == b"#header\n" + text, name
        # the same ranges through the memory route
        check(eng.vcf_format(arr, cal, i0, i1, sel, prefixes, ploidy=2, range_bytes=budget), ref)
    with pytest.raises(TagdigError) as ei:
        eng.vcf_file(str(tmp_path / "no_such_directory" / "body.vcf"), arr, cal, i0, i1, sel, prefixes, ploidy=2)
    assert ei.value.code == TD_E_IO
    got = eng.vcf_file(path, arr, cal, i0, i1, sel, prefixes, ploidy=2)
    with open(path, "rb") as fh:
        assert fh.read() == text and got.ranges == 1


def test_offsets_beyond_32_bits(eng):
    """Measure only: 2^20 lines over 512 samples with wide cells, drawn from five markers.  The total passes 2^32."""
    S, M, K = 512, 5, 1 << 20
    values = [U32, 10 ** 9, 12345, 7, 0]
    counts = [[v for m in range(M) for v in (values[m], values[(m + s) % M])] for s in range(S)]
    i0, i1, T = gc.adjacent(M)
    calls = [[(s + m) % 10 for m in range(M)] for s in range(S)]
    rng = np.random.RandomState(11)
    sel = rng.randint(0, M, size=K).astype(np.uint32)
    plen = (np.arange(K) % 3).astype(np.uint64)
    poff = np.concatenate([[0], np.cumsum(plen)]).astype(np.uint64)
    blob = b"ab" * K
    width = [len(x) for x in vc.lines(counts, i0, i1, calls, range(M), [b""] * M, 8)]
    assert len(set(width)) == M
    per_line = np.array(width, dtype=np.uint64)[sel] + plen
    mult = np.bincount(sel, minlength=M)
    total = sum(int(mult[m]) * width[m] for m in range(M)) + int(plen.sum())
    assert total > 1 << 32 and total == int(per_line.sum())
    got = eng.vcf_format(gc.as_array(counts, T), as_calls(calls, M), i0, i1, sel, (blob[:int(poff[-1])], poff), ploidy=8, measure_only=True)
    assert got.text is None and got.nbytes == total and int(got.line_off[K]) == total
    assert np.array_equal(got.line_off, np.concatenate([[0], np.cumsum(per_line)]).astype(np.uint64))


def test_no_launch_cases(eng):
    counts, i0, i1, T, calls, prefixes, ref = vc.grid_case(1, 515, "adjacent", "p2")
    got = run(eng, counts, T, i0, i1, calls, [], [], 2)
    assert got.nbytes == 0 and got.text == b"" and got.line_off.tolist() == [0] and got.ms["emit"] == 0
    empty = np.zeros((0, T), dtype=np.uint32)
    sel = [4, 0, 4]
    got = eng.vcf_format(empty, np.zeros((0, 515), dtype=np.uint8), i0, i1, sel, [b"abc", b"", b"defg"], ploidy=4)
    assert got.text == b"abc\n\ndefg\n" and got.line_off.tolist() == [0, 4, 5, 10] and got.ms["measure"] == 0


def test_capacity_one_byte_short(eng, range_case):
    from tagdigger_amd import TagdigError
    counts, i0, i1, T, calls, sel, prefixes, ref = range_case
    need = sum(len(x) for x in ref)
    with pytest.raises(TagdigError) as ei:
        run(eng, counts, T, i0, i1, calls, sel, prefixes, 2, capacity=need - 1)
    assert ei.value.code == TD_E_LIMIT and ei.value.needed == need
    check(run(eng, counts, T, i0, i1, calls, sel, prefixes, 2, capacity=need), ref)


def test_argument_errors(eng, range_case):
    from tagdigger_amd import TagdigError
    counts, i0, i1, T, calls, sel, prefixes, ref = range_case
    arr, cal = gc.as_array(counts, T), as_calls(calls, len(i0))
    CA, CB = vc.tables(10000)

    def refused(bad_index, *args, **kw):
        with pytest.raises(TagdigError) as ei:
            eng.vcf_format(*args, **kw)
        assert ei.value.code == TD_E_ARG and ei.value.bad_index == bad_index, ei.value
        check(eng.vcf_format(arr, cal, i0, i1, sel, prefixes, ploidy=2), ref)          # nothing is left latched

    for P in (0, 1, 9):
        refused(None, arr, cal, i0, i1, sel, prefixes, ploidy=P)
    refused(None, arr, cal, i0, i1, sel, prefixes, ploidy=4, likelihoods=True, ca=CA, cb=CB)
    refused(None, arr, cal, i0, i1, sel, prefixes, ploidy=2, likelihoods=True, ca=[0, vc.COST_MAX + 1, 0], cb=CB)
    refused(None, arr, cal, i0, i1, sel, prefixes, ploidy=2, likelihoods=True, ca=CA, cb=[0, 0, vc.COST_MAX + 1])
    past = list(sel)
    past[17] = len(i0)
    refused(17, arr, cal, i0, i1, past, prefixes, ploidy=2)
    wide = list(i1)
    wide[400] = T
    refused(400, arr, cal, i0, wide, sel, prefixes, ploidy=2)
    same = list(i1)
    same[9] = i0[9]
    refused(9, arr, cal, i0, same, sel, prefixes, ploidy=2)
    poff = vc.offsets(prefixes)
    poff[6] = poff[5] - 1
    refused(5, arr, cal, i0, i1, sel, (b"".join(prefixes), poff), ploidy=2)
    d = eng.dev_alloc(arr.nbytes + 8)
    try:
        eng.h2d(d + 4, arr.tobytes())
        check(eng.vcf_format(d + 4, cal, i0, i1, sel, prefixes, shape=arr.shape, ploidy=2), ref)         # 4-byte aligned: taken
        refused(None, d + 2, cal, i0, i1, sel, prefixes, shape=arr.shape, ploidy=2)
        refused(None, d + 4, 0, i0, i1, sel, prefixes, shape=arr.shape, ploidy=2)                     # no call matrix
    finally:
        eng.dev_free(d)


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_writevcf_gpu_equals_host(eng, tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T, ref = gc.populated_case()
    arr = gc.as_array(counts, T)
    samples, names = ["s%d" % k for k in range(len(counts))], gc.tag_names(65, i0, i1, T)
    host = tf.call_genotypes(arr, samples, names, backend="host", **gc.PARAMS[1])
    seqs = vc.tag_sequences(T, *(list(c) for c in host.columns))
    vc.assert_populated(host.calls.tolist(), list(host.mask), 2, seqs, *(list(c) for c in host.columns), 3)
    paths = {k: str(tmp_path / (k + ".vcf")) for k in ("host", "numpy", "device")}
    d = eng.dev_alloc(arr.nbytes)
    try:
        eng.h2d(d, arr.tobytes())
        kept = tf.call_genotypes(tf.DeviceCounts(d, arr.shape), samples, names, backend="gpu", keep_device=True, **gc.PARAMS[1])
        try:
            assert kept.d_calls.ptr
            for lik, passing_only, rb in ((False, True, None), (True, False, 3000)):
                kw = dict(tagseqs=seqs, passing_only=passing_only, likelihoods=lik, err=0.002)
                tf.writeVCF(paths["host"], host, arr, backend="host", **kw)
                plain = tf.call_genotypes(arr, samples, names, backend="gpu", **gc.PARAMS[1])
                info = tf.writeVCF(paths["numpy"], plain, arr, backend="gpu", range_bytes=rb, **kw)
                assert info["backend"] == "gpu" and info["ranges"] >= (2 if rb else 1) and info["lines"] > 0
                tf.writeVCF(paths["device"], kept, tf.DeviceCounts(d, arr.shape), backend="gpu", range_bytes=rb, **kw)
                want = read(paths["host"])
                assert want.count(b"\n") > 10 and read(paths["numpy"]) == want and read(paths["device"]) == want
        finally:
            eng.dev_free(kept.d_calls.ptr)
    finally:
        eng.dev_free(d)
    # a polyploid result: its dosages are uploaded
    P = 4
    pc = dc.binomial_counts(random.Random(94), 33, 40, P)
    j0, j1, PT = gc.adjacent(40)
    parr = gc.as_array(pc, PT)
    dose = tf.call_dosage(parr, samples[:33], gc.tag_names(40, j0, j1, PT), ploidy=P, backend="gpu", min_call_rate=0.4)
    tf.writeVCF(paths["host"], dose, parr, backend="host", passing_only=False)
    tf.writeVCF(paths["numpy"], dose, parr, backend="gpu", passing_only=False)
    assert read(paths["numpy"]) == read(paths["host"]) and b"0/0/1/1" in read(paths["host"])


def write_counts_csv(path, samples, names, counts):
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow([""] + names)
        for s, row in zip(samples, counts):
            w.writerow([s] + list(row))


def test_cli_writes_what_writevcf_writes(tmp_path, capsys):
    from tagdigger_amd import tag_calls, tag_dosage
    from tagdigger_amd import tagdigger_fun as tf
    counts, i0, i1, T, ref = gc.populated_case()
    arr = gc.as_array(counts, T)
    samples = ["s%d" % k for k in range(len(counts))]
    markers = ["chr%d-%04d-top" % (m % 3, 7 * (65 - m)) for m in range(65)]
    names = [None] * T
    for m in range(65):
        names[i0[m]], names[i1[m]] = markers[m] + "_0", markers[m] + "_1"
    csv_path, pos_path = str(tmp_path / "counts.csv"), str(tmp_path / "positions.csv")
    write_counts_csv(csv_path, samples, names, counts)
    with open(pos_path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Marker name", "Chromosome", "Position"])
        for m in range(65):
            w.writerow([markers[m], "LG%d" % (m % 2), 1000 - m])
    got, want = str(tmp_path / "cli.vcf"), str(tmp_path / "fun.vcf")
    filters = ["--min-depth", "3", "--min-call-rate", "0.6", "--min-maf", "0.05", "--err", "0.002"]
    host = tf.call_genotypes(arr, samples, names, backend="host", **gc.PARAMS[1])
    assert gc.PARAMS[1] == dict(err=0.002, min_depth=3, min_call_rate=0.6, min_maf=0.05, max_het=gc.PARAMS[1]["max_het"])
    filters += ["--max-het", str(gc.PARAMS[1]["max_het"])]
    assert tag_calls.main(["-i", csv_path, "-o", str(tmp_path / "calls.csv"), "--vcf", got, "--vcf-likelihoods", "--vcf-positions", "names"] + filters) == 0
    tf.writeVCF(want, host, arr, positions="names", likelihoods=True, err=0.002, backend="host")
    assert read(got) == read(want) and read(got).count(b"\n") > 20 and b"##contig=<ID=chr0>" in read(got)
    assert tag_calls.main(["-i", csv_path, "-o", str(tmp_path / "calls.csv"), "--vcf", got, "--vcf-positions", pos_path] + filters) == 0
    tf.writeVCF(want, host, arr, positions={markers[m]: ("LG%d" % (m % 2), 1000 - m) for m in range(65)}, backend="host")
    assert read(got) == read(want) and b"##contig=<ID=LG0>" in read(got)
    dose = tf.call_dosage(arr, samples, names, ploidy=4, backend="host", min_call_rate=0.3)
    assert tag_dosage.main(["-i", csv_path, "-o", str(tmp_path / "dose.csv"), "--ploidy", "4", "--min-call-rate", "0.3", "--vcf", got]) == 0
    tf.writeVCF(want, dose, arr, backend="host")
    assert read(got) == read(want) and read(got).count(b"\n") > 20
    capsys.readouterr()
