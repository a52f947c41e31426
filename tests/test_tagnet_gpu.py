"""The tag network on the device (csrc/tagnet.hip) against the rule stated by brute force in tests/tagnet_cases.py."""
import csv
import random

import numpy as np
import pytest

import tagnet_cases as tc
from census_cases import ordered, ref_census
from tagnet_cases import BARCODES, check_against, expected_file, expected_line, library_fastq

pytestmark = pytest.mark.gpu

TD_E_ARG, TD_E_OVERLAP, TD_E_ALPHABET, TD_E_LIMIT = -2, -3, -6, -7


@pytest.fixture(scope="module")
def eng():
    from tagdigger_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def build(eng, seqs, counts, ppm=tc.PPM, taglen=None):
    L = len(seqs[0]) if taglen is None else taglen
    return eng.tagnet_build("".join(seqs).encode("ascii"), counts, L, ppm)


def check_raw(eng, seqs, counts, ref, ppm=tc.PPM):
    """The C-ABI's answers, one by one, against the reference."""
    net = build(eng, seqs, counts, ppm)
    try:
        assert {k: net.stats[k] for k in tc.STATS} == ref["stats"]
        pairs, npairs = eng.tagnet_pairs(net)
        kept, nkept = eng.tagnet_edges(net, kept_only=True)
        every, nevery = eng.tagnet_edges(net, kept_only=False)
        assert [tuple(map(int, e)) for e in pairs] == ref["pairs"] and npairs == len(ref["pairs"])
        assert [tuple(map(int, e)) for e in kept] == ref["edges"] and nkept == len(ref["edges"])
        assert [tuple(map(int, e)) for e in every] == ref["all_edges"] and nevery == len(ref["all_edges"])
        assert eng.tagnet_degrees(net).tolist() == ref["degree"]
        return net.stats
    finally:
        net.close()


@pytest.mark.parametrize("min_ratio", tc.GRID_RATIO)
@pytest.mark.parametrize("L", tc.GRID_L)
def test_gpu_equals_brute_force(eng, L, min_ratio):
    from tagdigger_amd import tagdigger_fun as tf
    seqs, counts = tc.grid_case(L)
    ref = tc.grid_ref(L, round(min_ratio * 1e6))
    at_default = tc.grid_ref(L, tc.PPM)["stats"]          # (asserts that every class is populated from L = 5 on)
    assert at_default["edges"] > at_default["kept"] > 0
    got = tf.tag_network(list(seqs), list(counts), min_ratio=min_ratio, backend="gpu")
    check_against(ref, got)
    assert got.stats["backend"] == "gpu"


def test_raw_tiny_inputs(eng):
    net = build(eng, [], [], taglen=7)
    assert net.stats == dict(tags=0, edges=0, kept=0, deg0=0, deg1=0, hubs=0, pairs=0, compares=0)
    assert eng.tagnet_pairs(net)[1] == 0 and eng.tagnet_edges(net, False)[1] == 0 and len(eng.tagnet_degrees(net)) == 0
    net.close()
    net = build(eng, ["ACGTACG"], [5])
    assert net.stats == dict(tags=1, edges=0, kept=0, deg0=1, deg1=0, hubs=0, pairs=0, compares=0)
    assert eng.tagnet_pairs(net)[1] == 0 and eng.tagnet_degrees(net).tolist() == [0]
    net.close()
    # the four tags of one base: a 4-clique
    seqs, counts = ["A", "C", "G", "T"], [7, 7, 6, 5]
    ref = tc.ref_network(seqs, counts, tc.PPM)
    assert ref["stats"]["edges"] == 6 and ref["stats"]["hubs"] == 4 and ref["pairs"] == []
    st = check_raw(eng, seqs, counts, ref)
    assert st["compares"] == 6


@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("L", [64, 20])
def test_one_long_run(eng, L, swapped):
    seqs, counts, ref = tc.long_run_case(L, swapped)      # (asserts on the reference: > 1 024 tags, every class there)
    st = check_raw(eng, seqs, counts, ref)
    n = len(seqs)
    assert st["compares"] >= n * (n - 1) // 2             # the whole input is one run of one of the two orders


def test_runs_around_the_tile_edge(eng):
    from tagdigger_amd.engine import TAGNET_TILE
    seqs, counts = tc.many_runs(random.Random(5), TAGNET_TILE)
    ref = tc.ref_network(seqs, counts, tc.PPM)
    tc.assert_populated(ref)
    check_raw(eng, seqs, counts, ref)


@pytest.mark.parametrize("seqs,counts,kept", tc.boundary_cases())
def test_ratio_boundary(eng, seqs, counts, kept):
    ref = tc.ref_network(seqs, counts, tc.PPM)
    assert ref["edges"] == ([(0, 1)] if kept else []) and ref["stats"]["edges"] == 1
    check_raw(eng, seqs, counts, ref)


def test_error_paths(eng):
    from tagdigger_amd import TagdigError
    from tagdigger_amd import tagdigger_fun as tf
    good, gcounts = list(tc.grid_case(33)[0]), list(tc.grid_case(33)[1])
    gref = tc.grid_ref(33, tc.PPM)

    def then_a_valid_build():
        check_raw(eng, good, gcounts, gref)

    bad = list(good)
    bad[17] = bad[17][:5] + "N" + bad[17][6:]
    with pytest.raises(TagdigError) as ei:
        build(eng, bad, gcounts)
    assert ei.value.code == TD_E_ALPHABET and ei.value.bad_index == 17
    then_a_valid_build()
    dup = list(good)
    dup[40] = dup[3]
    with pytest.raises(TagdigError) as ei:
        build(eng, dup, gcounts)
    assert ei.value.code == TD_E_OVERLAP and ei.value.bad_index == 40
    then_a_valid_build()
    for taglen in (0, 65):
        with pytest.raises(TagdigError) as ei:
            eng.tagnet_build(b"A" * (2 * taglen), [1, 1], taglen, tc.PPM)
        assert ei.value.code == TD_E_ARG
    with pytest.raises(TagdigError) as ei:
        build(eng, good, gcounts, ppm=1000001)
    assert ei.value.code == TD_E_ARG
    then_a_valid_build()
    # the compare cap
    seqs, counts, ref = tc.long_run_case(64, False)
    eng.set_option("tagnet_max_compares", 1000)
    try:
        with pytest.raises(TagdigError) as ei:
            build(eng, seqs, counts)
        assert ei.value.code == TD_E_LIMIT
        compares = ei.value.stats["compares"]
        assert compares >= len(seqs) * (len(seqs) - 1) // 2
        assert str(compares) in ei.value.detail and "1000" in ei.value.detail.replace(str(compares), "")
        # through Python the same input is answered by the host restatement
        from tagdigger_amd.engine import default_engine
        deng = default_engine(0)
        deng.set_option("tagnet_max_compares", 1000)
        try:
            got = tf.tag_network(seqs, counts, backend="gpu")
        finally:
            deng.set_option("tagnet_max_compares", 0)
        check_against(ref, got)
        assert got.stats["backend"] == "host"
    finally:
        eng.set_option("tagnet_max_compares", 0)
    then_a_valid_build()
    assert tf.tag_network(seqs, counts, backend="gpu").stats["backend"] == "gpu"


def test_capacity_smaller_than_the_result(eng):
    seqs, counts = tc.grid_case(63)
    ref = tc.grid_ref(63, tc.PPM)
    net = build(eng, list(seqs), list(counts))
    try:
        for fetch, want in ((lambda cap: eng.tagnet_pairs(net, cap), ref["pairs"]),
                            (lambda cap: eng.tagnet_edges(net, True, cap), ref["edges"]),
                            (lambda cap: eng.tagnet_edges(net, False, cap), ref["all_edges"])):
            assert len(want) > 5
            head, total = fetch(5)
            assert total == len(want) and [tuple(map(int, e)) for e in head] == want[:5]
            none, total = fetch(0)
            assert total == len(want) and len(none) == 0
            full, total = fetch(len(want))
            assert total == len(want) and [tuple(map(int, e)) for e in full] == want
    finally:
        net.close()


def test_degrees(eng):
    seqs, counts = tc.grid_case(33)
    ref = tc.grid_ref(33, tc.PPM)
    net = build(eng, list(seqs), list(counts))
    try:
        deg = eng.tagnet_degrees(net)
        assert deg.dtype == np.uint32 and deg.tolist() == ref["degree"]
    finally:
        net.close()


def test_cli_end_to_end(tmp_path, capsys):
    from tagdigger_amd import tag_pairs
    rng = random.Random(2025)
    seqs, counts = tc.library(rng, 35, 12, 3)
    data = library_fastq(rng, seqs, counts)
    fq, key, out = str(tmp_path / "lib.fq"), str(tmp_path / "key.csv"), str(tmp_path / "markers.csv")
    with open(fq, "wb") as fh:
        fh.write(data)
    with open(key, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["File", "Barcode", "Sample"])
        for i, b in enumerate(BARCODES):
            w.writerow([fq, b, "s%d" % i])
    assert tag_pairs.main(["-f", fq, "-b", key, "-e", "PstI", "--taglen", "40", "-o", out]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    want, _ = ref_census(data, BARCODES, "TGCAG", 40)
    rseqs, rcounts = ordered(want, min_count=2)
    ref = tc.ref_network(rseqs, rcounts, tc.PPM)
    tc.assert_populated(ref)
    with open(out, "rb") as fh:
        assert fh.read() == expected_file(rseqs, rcounts, ref)
    assert line == expected_line(ref)
