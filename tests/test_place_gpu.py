"""Tag placement on the device (csrc/place.hip) against the rule stated by brute force in tests/place_cases.py."""
import csv
import os
import subprocess
import sys

import pytest

import place_cases as pc
from test_place import write

pytestmark = pytest.mark.gpu

TD_E_ARG, TD_E_ALPHABET, TD_E_LIMIT = -2, -6, -7
SITE_IDS = [c[0] for c in pc.site_cases()]
CASES = {"grid": pc.join_case, "mult": pc.multiplicity_case, "run": pc.long_run_case}


def gpu_sites(tmp_path, text, cutsite, L, name="genome.fa"):
    from tagdigger_amd import tagdigger_fun as tf
    return tf.genome_cut_sites(write(tmp_path / name, text), cutsite, L, backend="gpu")


@pytest.mark.parametrize("case_id", SITE_IDS)
def test_site_scan_equals_brute_force(tmp_path, case_id):
    _, text, cutsite, L = next(c for c in pc.site_cases() if c[0] == case_id)
    got = gpu_sites(tmp_path, text, cutsite, L)
    try:
        pc.check_sites(pc.site_ref(case_id), got)
        assert got.stats["backend"] == "gpu"
    finally:
        got.close()


def place_gpu(tmp_path, kind, *args):
    from tagdigger_amd import tagdigger_fun as tf
    text, site, L, k, tags = CASES[kind](*args)
    sites = gpu_sites(tmp_path, text, site, L)
    try:
        pc.check_sites(pc.join_ref(kind, *args)["sites"] | dict(names=sites.names, rec_start=sites.rec_start), sites)
        return tf.place_tags(list(tags), sites, max_mismatch=k, backend="gpu")
    finally:
        sites.close()


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("L", ("k+1",) + pc.GRID_L)
def test_join_equals_brute_force(tmp_path, L, k):
    L = k + 1 if L == "k+1" else L
    got = place_gpu(tmp_path, "grid", L, k)
    pc.check_placed(pc.join_ref("grid", L, k), got)
    assert got.stats["backend"] == "gpu"


def test_multiplicity_and_both_strands(tmp_path):
    ref = pc.join_ref("mult")
    assert [ref["n_at"][i][0] for i in range(4)] == [1, 2, 300, 2] and ref["locus"][2] == 0
    got = place_gpu(tmp_path, "mult")
    pc.check_placed(ref, got)
    assert got.stats["backend"] == "gpu"


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("m", pc.LONG_RUNS)
def test_long_run(tmp_path, m, k):
    ref = pc.join_ref("run", m, k)
    assert ref["compares"] >= m * (len(ref["dist"]) - 1)
    got = place_gpu(tmp_path, "run", m, k)
    pc.check_placed(ref, got)
    assert got.stats["backend"] == "gpu"


def test_zero_tags_zero_loci_and_a_bad_byte(tmp_path):
    from tagdigger_amd import TagdigError
    from tagdigger_amd import tagdigger_fun as tf
    text, site, L, k, tags = pc.join_case(16, 1)
    sites = gpu_sites(tmp_path, text, site, L)
    try:
        eng, place = sites._place._eng, sites._place
        none = tf.place_tags([], sites, max_mismatch=1)
        assert none.status == [] and none.stats["backend"] == "gpu"
        n_at, dist, locus, stats, _ = eng.place_tags(place, b"", 0, 1)
        assert len(dist) == 0 and stats["tags"] == 0
        bad = list(tags[:12])
        bad[7] = bad[7][:9] + "N" + bad[7][10:]
        with pytest.raises(TagdigError) as ei:
            eng.place_tags(place, "".join(bad).encode(), len(bad), 1)
        assert ei.value.code == TD_E_ALPHABET and ei.value.bad_index == 7
        for k_bad in (4, 17):
            with pytest.raises(TagdigError) as ei:
                eng.place_tags(place, "".join(tags[:2]).encode(), 2, k_bad)
            assert ei.value.code == TD_E_ARG
        pc.check_placed(pc.join_ref("grid", 16, 1), tf.place_tags(list(tags), sites, max_mismatch=1))      # and a valid call after them
    finally:
        sites.close()
    empty = gpu_sites(tmp_path, ">c\nAACCAACCAACCAACCAACCAACC\n", "TGCAG", 16, name="nosite.fa")
    try:
        assert empty.stats["loci"] == 0
        got = tf.place_tags(["TGCAGAACCAACCAAC"] * 3, empty, max_mismatch=2)
        assert got.status == ["none"] * 3 and got.dist == [pc.NONE] * 3 and got.locus == [pc.NO_LOCUS] * 3
        with pytest.raises(TagdigError) as ei:
            empty._place._eng.place_tags(empty._place, b"TGCAGAACCAACCAAC" + b"TGCAGAACCAACCAAX", 2, 1)
        assert ei.value.code == TD_E_ALPHABET and ei.value.bad_index == 1
    finally:
        empty.close()


def test_the_cap(tmp_path):
    from tagdigger_amd import TagdigError
    from tagdigger_amd import tagdigger_fun as tf
    text, site, L, k, tags = pc.long_run_case(600, 2)
    ref = pc.join_ref("run", 600, 2)
    sites = gpu_sites(tmp_path, text, site, L)
    eng = sites._place._eng
    eng.set_option("place_max_compares", ref["compares"] - 1)
    try:
        with pytest.raises(TagdigError) as ei:
            eng.place_tags(sites._place, "".join(tags).encode(), len(tags), k)
        assert ei.value.code == TD_E_LIMIT and ei.value.stats["compares"] == ref["compares"]
        assert str(ref["compares"]) in ei.value.detail and str(ref["compares"] - 1) in ei.value.detail
        got = tf.place_tags(list(tags), sites, max_mismatch=k, backend="gpu")
        pc.check_placed(ref, got)
        assert got.stats["backend"] == "host"
        eng.set_option("place_max_compares", ref["compares"])
        assert tf.place_tags(list(tags), sites, max_mismatch=k, backend="gpu").stats["backend"] == "gpu"
    finally:
        eng.set_option("place_max_compares", 0)
        sites.close()


def test_a_place_left_open_goes_with_the_handle(tmp_path):
    from tagdigger_amd import Engine
    _, text, cutsite, L = next(c for c in pc.site_cases() if c[0] == "cwgc")
    G, names, rec_start = pc.parse_fasta(text)
    eng = Engine(0)
    d = eng.dev_alloc(len(G) + 16)
    try:
        eng.h2d(d, G.encode())
        a = eng.place_sites(d, len(G), rec_start, pc.remnants_of(cutsite), L)
        b = eng.place_sites(d, len(G), rec_start, pc.remnants_of(cutsite), L)
        assert a.stats["loci"] == b.stats["loci"] == pc.site_ref("cwgc")["stats"]["loci"]
        x, rec, strand, wins = eng.place_loci(b, windows=True)
        assert wins == pc.site_ref("cwgc")["windows"]
        b.close()                                       # one freed by hand, the other left to td_destroy
        a.ptr = None
    finally:
        eng.dev_free(d)
        eng.close()


def test_raw_calls_on_an_unaligned_genome():
    """The C-ABI by itself: a genome that does not start on a 16-byte boundary (the scan's byte-wise staging), and the
    statistics td_place_tags counts."""
    from tagdigger_amd import Engine
    text, site, L, k, tags = pc.multiplicity_case()
    ref = pc.join_ref("mult")
    G, names, rec_start = pc.parse_fasta(text)
    _, etext, esite, eL = next(c for c in pc.site_cases() if c[0] == "edge+3")
    EG, _, erec = pc.parse_fasta(etext)
    eng = Engine(0)
    d = eng.dev_alloc(max(len(G), len(EG)) + 32)
    try:
        eng.h2d(d + 1, EG.encode())
        edge = eng.place_sites(d + 1, len(EG), erec, [esite], eL)
        x, rec, strand, wins = eng.place_loci(edge, windows=True)
        eref = pc.site_ref("edge+3")
        assert x.tolist() == eref["x"] and strand.tolist() == eref["strand"] and wins == eref["windows"]
        assert {s: edge.stats[s] for s in eref["stats"]} == eref["stats"]
        edge.close()
        eng.h2d(d + 1, G.encode())
        place = eng.place_sites(d + 1, len(G), rec_start, [site], L)
        assert eng.place_loci(place, windows=True)[3] == ref["sites"]["windows"]
        n_at, dist, locus, stats, ms = eng.place_tags(place, "".join(tags).encode(), len(tags), k)
        assert n_at.tolist() == ref["n_at"] and dist.tolist() == ref["dist"] and locus.tolist() == ref["locus"]
        assert stats == dict(tags=len(tags), unique=ref["status"].count("unique"), multi=ref["status"].count("multi"),
                             none=ref["status"].count("none"), compares=ref["compares"])
        assert ref["status"].count("unique") and ref["status"].count("multi")
        assert set(ms) == {"pack", "parts", "runs", "join"} and ms["parts"] > 0
        assert eng.place_tags(place, "".join(tags).encode(), len(tags), k)[4]["parts"] == 0      # the tables are kept
        other = Engine(0)
        try:
            from tagdigger_amd import TagdigError
            with pytest.raises(TagdigError) as ei:
                other.place_tags(place, "".join(tags).encode(), len(tags), k)
            assert ei.value.code == TD_E_ARG
        finally:
            other.close()
        place.close()
    finally:
        eng.dev_free(d)
        eng.close()


def test_the_chain(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    text, L, planted, frag, counts, fq = pc.chain_case()
    fa = write(tmp_path / "genome.fa", text)
    lib = str(tmp_path / "lib.fq")
    with open(lib, "wb") as fh:
        fh.write(fq)
    census = tf.tag_census(lib, pc.BARCODES, cutsite="TGCAG", taglen=L, backend="gpu")
    assert sorted(census[0]) == sorted(t for tags in planted.values() for t in tags)
    sites = tf.genome_cut_sites(fa, "TGCAG", L, backend="gpu")
    try:
        res = tf.place_tags(census[0], sites, max_mismatch=1, backend="gpu")
    finally:
        sites.close()
    assert res.status == ["unique"] * len(census[0]) and res.stats["backend"] == "gpu"
    sam = str(tmp_path / "placed.sam")
    tf.writePlacementSAM(sam, res)
    names, seqs = tf.readTags_TASSELSAM(sam, binaryOnly=True)
    by_marker = {}
    for nm, s in zip(names, seqs):
        by_marker.setdefault(nm.split("_")[0], []).append(s)
    assert {k: sorted(v) for k, v in by_marker.items()} == {"%s-%04d-%s" % key: tags for key, tags in planted.items()}
    got = tf.find_tags_fastq(lib, pc.BARCODES, seqs, cutsite="TGCAG", progress=False)
    assert got == [[counts[(b, s)] for s in seqs] for b in pc.BARCODES]
    # census -> place -> expected fragment sizes: PstI's site alone closes the fragments (MspI's CCGG, the other default,
    # arises by chance where a window ending in CC meets CC on the other strand)
    out = str(tmp_path / "frag.csv")
    subprocess.run([sys.executable, "-m", "tagdigger_amd.exp_frag_size", "-s", sam, "-g", fa, "-o", out, "-c", "CTGCAG"],
                   check=True, timeout=120, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rows = list(csv.DictReader(open(out, newline="")))
    assert len(rows) == len(census[0])
    assert {r["Marker name"][len("tagSeq="):]: r["Fragment size"] for r in rows} == {t: str(n) for t, n in frag.items()}
    where = {(r["Sequence name"], int(r["Position"]), "top" if r["Strand"] == "forward" else "bot") for r in rows}
    assert where == set(planted)
