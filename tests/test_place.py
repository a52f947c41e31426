"""Tag placement on the host (tagdigger_fun genome_cut_sites / place_tags with backend="host", the writers and the command
line) against the rule stated by brute force in tests/place_cases.py.  No GPU."""
import csv
import gzip

import pytest

import place_cases as pc

SITE_IDS = [c[0] for c in pc.site_cases()]


def write(path, text, mode="w"):
    with (gzip.open(path, mode + "t") if str(path).endswith(".gz") else open(path, mode)) as fh:
        fh.write(text)
    return str(path)


def host_sites(tmp_path, text, cutsite, L, name="genome.fa"):
    from tagdigger_amd import tagdigger_fun as tf
    return tf.genome_cut_sites(write(tmp_path / name, text), cutsite, L, backend="host")


@pytest.mark.parametrize("case_id", SITE_IDS)
def test_host_sites_equal_brute_force(tmp_path, case_id):
    _, text, cutsite, L = next(c for c in pc.site_cases() if c[0] == case_id)
    got = host_sites(tmp_path, text, cutsite, L)
    pc.check_sites(pc.site_ref(case_id), got)
    assert got.stats["backend"] == "host"


def test_the_cases_hold_what_they_are_for():
    st = pc.site_ref("bounds")["stats"]
    assert st["dropped_bounds"] >= 7 and st["forward"] == 2 and st["reverse"] == 2
    assert pc.site_ref("alphabet")["stats"]["dropped_alphabet"] == 28
    pal = pc.site_ref("palindrome")
    assert any(pal["x"][i] == pal["x"][i + 1] and pal["strand"][i:i + 2] == [0, 1] for i in range(len(pal["x"]) - 1))
    assert pc.site_ref("overlap")["stats"]["forward"] == 3
    assert pc.site_ref("site_of_64")["stats"] == dict(loci=2, forward=1, reverse=1, distinct=1, dropped_bounds=0,
                                                      dropped_alphabet=0, records=1)
    assert len(pc.remnants_of("CWGC")) == 2
    for off in range(-5, 6):                              # the planted sites are there, whatever else the random genome holds
        ref = pc.site_ref("edge%+d" % off)
        assert (pc.SCAN_TILE - pc.SCAN_HALO + off, 0) in zip(ref["x"], ref["strand"])
        assert (2 * pc.SCAN_TILE - pc.SCAN_HALO + 300 + off, 1) in zip(ref["x"], ref["strand"])


def test_gz_and_several_files(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    _, text, cutsite, L = next(c for c in pc.site_cases() if c[0] == "cwgc")
    cut = text.index(">two")
    paths = [write(tmp_path / "a.fa.gz", text[:cut]), write(tmp_path / "b.fa", text[cut:])]
    pc.check_sites(pc.site_ref("cwgc"), tf.genome_cut_sites(paths, cutsite, L, backend="host"))


def place_host(tmp_path, kind, *args):
    from tagdigger_amd import tagdigger_fun as tf
    text, site, L, k, tags = {"grid": pc.join_case, "mult": pc.multiplicity_case, "run": pc.long_run_case}[kind](*args)
    sites = host_sites(tmp_path, text, site, L)
    return tf.place_tags(list(tags), sites, max_mismatch=k, backend="host")


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("L", ("k+1",) + pc.GRID_L)
def test_host_join_equals_brute_force(tmp_path, L, k):
    L = k + 1 if L == "k+1" else L
    ref = pc.join_ref("grid", L, k)
    got = place_host(tmp_path, "grid", L, k)
    pc.check_placed(ref, got)
    assert got.stats["backend"] == "host"
    if L >= 16:                                           # every class of tag is there
        assert {"unique", "none"} <= set(ref["status"]) and set(ref["dist"]) >= set(range(k + 1)) | {pc.NONE}


def test_host_multiplicity(tmp_path):
    ref = pc.join_ref("mult")
    assert [ref["n_at"][i][0] for i in range(4)] == [1, 2, 300, 2] and ref["status"][:4] == ["unique", "multi", "multi", "multi"]
    assert ref["locus"][2] == 0                           # the first of 300 copies
    pc.check_placed(ref, place_host(tmp_path, "mult"))


@pytest.mark.parametrize("m", [257, 600])
def test_host_long_run(tmp_path, m):
    pc.check_placed(pc.join_ref("run", m, 2), place_host(tmp_path, "run", m, 2))


def test_value_errors(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    fa = write(tmp_path / "g.fa", ">c\nAATGCAGACGTACGTACGTAACC\n")
    with pytest.raises(ValueError):
        tf.genome_cut_sites(fa, tf.enzymes["None"], 8, backend="host")
    dup = write(tmp_path / "dup.fa", ">c one\nAATGCAGACGT\n>d\nACGT\n>c two\nACGTTGCAGAAAA\n")
    with pytest.raises(ValueError, match="twice"):
        tf.genome_cut_sites(dup, "TGCAG", 8, backend="host")
    with pytest.raises(ValueError, match="empty name"):
        tf.genome_cut_sites(write(tmp_path / "anon.fa", ">\nAATGCAGACGT\n"), "TGCAG", 8, backend="host")
    with pytest.raises(ValueError):
        tf.genome_cut_sites(write(tmp_path / "head.fa", "AATGCAGACGT\n>c\nACGT\n"), "TGCAG", 8, backend="host")
    with pytest.raises(ValueError):
        tf.genome_cut_sites(fa, "TGCAG", 4, backend="host")          # a cut site longer than the tags
    with pytest.raises(ValueError):
        tf.genome_cut_sites(fa, "TGCAG", 65, backend="host")
    sites3 = tf.genome_cut_sites(fa, "TGC", 3, backend="host")
    with pytest.raises(ValueError):
        tf.place_tags(["TGC"], sites3, max_mismatch=3, backend="host")       # L < k + 1
    assert tf.place_tags(["TGC"], sites3, max_mismatch=2, backend="host").status == ["multi"]      # TGC and, reversed, GCA
    sites = tf.genome_cut_sites(fa, "TGCAG", 8, backend="host")
    with pytest.raises(ValueError):
        tf.place_tags(["TGCAGACG"], sites, max_mismatch=4, backend="host")
    with pytest.raises(ValueError):
        tf.place_tags(["TGCAGAC"], sites, backend="host")
    with pytest.raises(ValueError):
        tf.place_tags(["TGCAGACN"], sites, backend="host")
    empty = tf.place_tags([], sites, backend="host")
    assert empty.status == [] and empty.stats["tags"] == 0


# ------------------------------------------------------------------ the writers
GENOME = ">chr_1 first\nAACCATGCAGAACCAACCAA\n>chr2\nCCAAGTTGGTTCTGCAAACA\nAACATGCAGAACCAACCAAA\nTGCAGAACCAACCAAC\n"
#   chr_1: TGCAGAACCAAC forward at x = 5 (pos 6).  chr2 (56 bases): GTTGGTTCTGCA is the reverse window TGCAGAACCAAC, pos 5,
#   cut position 16; TGCAGAACCAAC forward at pos 25 and at pos 41.
TAGS = ["TGCAGAACCAAC", "TGCAGAACCAAT", "TGCAGAACCTTG", "TGCAGGGGGGGG"]


def small_result(tmp_path, k=1):
    from tagdigger_amd import tagdigger_fun as tf
    sites = host_sites(tmp_path, GENOME, "TGCAG", 12, name="small.fa")
    return sites, tf.place_tags(TAGS, sites, max_mismatch=k, backend="host")


def test_writers_byte_for_byte(tmp_path):
    from tagdigger_amd import tagdigger_fun as tf
    sites, res = small_result(tmp_path)
    assert sites.windows() == ["TGCAGAACCAAC"] * 4 and sites.strand.tolist() == [0, 1, 0, 0]
    tf.writeCutSites(str(tmp_path / "sites.csv"), sites)
    assert open(tmp_path / "sites.csv", newline="").read() == (
        "Chromosome,Cut position,Strand,Window\r\n"
        "chr_1,6,top,TGCAGAACCAAC\r\n"
        "chr2,16,bot,TGCAGAACCAAC\r\n"
        "chr2,25,top,TGCAGAACCAAC\r\n"
        "chr2,41,top,TGCAGAACCAAC\r\n")
    tf.writePlacements(str(tmp_path / "placed.csv"), res, counts=[9, 5, 4, 3])
    assert open(tmp_path / "placed.csv", newline="").read() == (
        "Tag sequence,Count,Status,Chromosome,Position,Strand,Mismatches,Best loci,Loci within k\r\n"
        "TGCAGAACCAAC,9,multi,chr_1,6,top,0,4,4\r\n"
        "TGCAGAACCAAT,5,multi,chr_1,6,top,1,4,4\r\n"
        "TGCAGAACCTTG,4,none,,,,,0,0\r\n"
        "TGCAGGGGGGGG,3,none,,,,,0,0\r\n")
    head = "@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr_1\tLN:20\n@SQ\tSN:chr2\tLN:56\n@PG\tID:tag_place\tPN:tagdigger_amd.tag_place\n"
    tf.writePlacementSAM(str(tmp_path / "drop.sam"), res)
    assert open(tmp_path / "drop.sam").read() == head + (
        "tagSeq=TGCAGAACCAAC\t4\t*\t0\t0\t*\t*\t0\t0\tTGCAGAACCAAC\t*\tNM:i:0\tX0:i:4\tX1:i:0\n"
        "tagSeq=TGCAGAACCAAT\t4\t*\t0\t0\t*\t*\t0\t0\tTGCAGAACCAAT\t*\tNM:i:1\tX0:i:4\tX1:i:0\n"
        "tagSeq=TGCAGAACCTTG\t4\t*\t0\t0\t*\t*\t0\t0\tTGCAGAACCTTG\t*\tX0:i:0\tX1:i:0\n"
        "tagSeq=TGCAGGGGGGGG\t4\t*\t0\t0\t*\t*\t0\t0\tTGCAGGGGGGGG\t*\tX0:i:0\tX1:i:0\n")
    tf.writePlacementSAM(str(tmp_path / "first.sam"), res, names=["a", "b", "c", "d"], multi="first")
    assert open(tmp_path / "first.sam").read().splitlines()[4:6] == [
        "a\t0\tchr_1\t6\t0\t12M\t*\t0\t0\tTGCAGAACCAAC\t*\tNM:i:0\tX0:i:4\tX1:i:0",
        "b\t0\tchr_1\t6\t0\t12M\t*\t0\t0\tTGCAGAACCAAT\t*\tNM:i:1\tX0:i:4\tX1:i:0"]
    with pytest.raises(ValueError):
        tf.writePlacementSAM(str(tmp_path / "x.sam"), res, multi="all")


def planted_genome():
    """Two markers of two alleles each, one per strand, and a tag that lies twice."""
    f0, f1 = "TGCAGAACCAACCAAA", "TGCAGAACCATCCAAA"
    b0, b1 = "TGCAGCCAACACACCA", "TGCAGCCAACACACAA"
    twice = "TGCAGACACACACACA"
    chr1 = "CCAA" * 5 + f0 + "CCAA" * 6 + pc.rc(b0) + "CCAA" * 4 + twice + "CCAA" * 3      # f0 at pos 21, b0 at pos 61, cut 76
    chr2 = "CCAA" * 3 + twice + "CCAA" * 2
    return pc.fasta([("chr1", chr1), ("chr2", chr2)]), (f0, f1, b0, b1, twice)


def test_sam_is_read_by_the_existing_readers(tmp_path):
    from tagdigger_amd import exp_frag_size as efs
    from tagdigger_amd import tagdigger_fun as tf
    text, (f0, f1, b0, b1, twice) = planted_genome()
    sites = host_sites(tmp_path, text, "TGCAG", 16)
    tags = [f1, b0, twice, f0, b1, "TGCAGTTTTTTTTTTT"]
    res = tf.place_tags(tags, sites, max_mismatch=1, backend="host")
    assert res.status == ["unique", "unique", "multi", "unique", "unique", "none"]
    sam = str(tmp_path / "placed.sam")
    tf.writePlacementSAM(sam, res)
    names, seqs = tf.readTags_TASSELSAM(sam, binaryOnly=True)
    assert dict(zip(names, seqs)) == {"chr1-021-top_A_0": f0, "chr1-021-top_T_1": f1,
                                     "chr1-076-bot_A_0": b1, "chr1-076-bot_C_1": b0}
    got = efs.read_sam(sam)
    assert got.names == ["tagSeq=" + t for t in tags]
    assert got.seqnames == ["chr1", "chr1", "*", "chr1", "chr1", "*"]
    assert got.positions == [21, 76, 0, 21, 76, 0]
    assert got.forward == [True, False, True, True, False, True]
    assert got.aligned == [True, True, False, True, True, False]
    assert got.tagsizes == [16] * 6


def test_cli_host(tmp_path, capsys):
    from tagdigger_amd import tag_place
    from tagdigger_amd import tagdigger_fun as tf
    text, (f0, f1, b0, b1, twice) = planted_genome()
    fa = write(tmp_path / "genome.fa.gz", text)
    census = str(tmp_path / "census.csv")
    with open(census, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Tag sequence", "Count", "Known tags"])
        w.writerows([[f0, 40, ""], [b0, 30, ""], [f1, 12, ""], [twice, 11, ""], [b1, 9, ""], ["TGCAGTTTTTTTTTTT", 1, ""]])
    sam, table, digest = (str(tmp_path / n) for n in ("placed.sam", "placed.csv", "sites.csv"))
    assert tag_place.main(["-i", census, "-g", fa, "-e", "PstI", "-o", sam, "--table", table, "--sites", digest,
                           "--td-backend", "host"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line == "Loci: 4 Distinct windows: 3 Dropped: 0 Tags: 5 Unique: 4 Multi: 1 None: 0"
    names, seqs = tf.readTags_TASSELSAM(sam, binaryOnly=True)
    assert sorted(seqs) == sorted([f0, f1, b0, b1])
    rows = list(csv.reader(open(table, newline="")))
    assert rows[1] == [f0, "40", "unique", "chr1", "21", "top", "0", "1", "1"]
    assert rows[4] == [twice, "11", "multi", "chr1", "93", "top", "0", "2", "2"]
    assert len(list(csv.reader(open(digest, newline="")))) == 5
    with pytest.raises(Exception):
        tag_place.main(["-i", census, "-g", fa, "-e", "None", "-o", sam, "--td-backend", "host"])
