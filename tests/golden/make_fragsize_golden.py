#!/usr/bin/env python3
"""Generate tests/golden/fragsize.json from the REAL reference exp_frag_size.py (build container only; data only, never
reference code): each case is a set of small input files (SAM, FASTA, plain / .gz / damaged), the command line, and what
the reference did with them -- stdout and the CSV's bytes, or the exception (class and message, the last line of its
traceback).  Payloads are stored as base64 of a zlib stream.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_fragsize_golden.py REFERENCE_DIR
"""
import base64
import gzip
import json
import os
import random
import subprocess
import sys
import tempfile
import zlib

REF = sys.argv[1] if len(sys.argv) > 1 else None
HERE = os.path.dirname(os.path.abspath(__file__))


def pack(data):
    """bytes -> base64 of their zlib stream (tests unpack with base64 + zlib)"""
    return base64.b64encode(zlib.compress(data, 9)).decode()


def sam_line(name, flag, seq, pos, cigar="64M", tag="A" * 64):
    return "%s\t%d\t%s\t%d\t30\t%s\t*\t0\t0\t%s\t*\n" % (name, flag, seq, pos, cigar, tag)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def wrap(seq, width, eol="\n"):
    return "".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def with_sites(rng, n, sites=("CTGCAG", "CCGG"), every=400):
    s = list(rand_seq(rng, n))
    for p in range(rng.randrange(50, every), n - 10, every):
        site = rng.choice(sites)
        s[p:p + len(site)] = site
    return "".join(s[:n])


def cases():
    rng = random.Random(20261016)
    out = []

    def case(name, files, args, note=""):
        out.append({"name": name, "files": {k: pack(v if isinstance(v, bytes) else v.encode()) for k, v in files.items()},
                    "args": args, "note": note})

    # 1: three chromosomes, > 1 000 searches (progress lines), both strands, clips, indels, unaligned, unknown names;
    #    the last chromosome is never searched
    chroms = [("chr1", with_sites(rng, 3000, every=90)), ("chr2", with_sites(rng, 2500, every=90)),
              ("chr3", with_sites(rng, 1500, every=90))]
    fa = "".join(">%s\n%s" % (c, wrap(s, 60)) for c, s in chroms)
    sam = "@HD\tVN:1.0\n@SQ\tSN:chr1\tLN:3000\n"
    for i in range(2300):
        c = rng.choice(["chr1", "chr1", "chr2", "chr2", "chr3", "chrX"])
        sam += sam_line("t%d" % i, rng.choice([0, 16, 4, 20, 256]), c, rng.randint(1, 3000),
                        rng.choice(["16M", "2S14M", "12M4S", "7M2I7M", "7M3D9M", "3S10M3S"]), "ACGTTGCA" * 2)
    case("many_tags", {"g.fa": fa, "t.sam": sam}, ["-s", "t.sam", "-g", "g.fa", "-o", "out.csv"])

    # 2: line ends, case, IUPAC, whitespace, ragged and unwrapped lines, empty record, text before the first header,
    #    duplicate names, a header with a description
    s1, s2, s3 = with_sites(rng, 5000), with_sites(rng, 4000), with_sites(rng, 3000)
    lower = "".join(c.lower() if rng.random() < 0.3 else c for c in s1)
    iupac = "".join(rng.choice("NRYKMSWBDHV") if rng.random() < 0.05 else c for c in s2)
    fa = ("ACGTCCGGAT\r\n" +                                     # before the first header: record ""
          ">chrA\r\n" + wrap(lower, 70, "\r\n") +
          ">chrB\r" + wrap(iupac[:2000], 33, "\r") + wrap(iupac[2000:], 51, "\n") +
          ">empty\n\n  \n" +
          ">chrC desc\n" + s3 + "\n" +                           # unwrapped; 'chrC desc' does not match chrC
          ">chrD\n" + "".join(" \t" + s3[i:i + 40] + " \x0b\x0c\x1c\n" if i % 80 else s3[i:i + 40] + "  AC  GT\n"
                              for i in range(0, len(s3), 40)) +
          ">chrA\n" + wrap(s2, 80) +                             # chrA again: searched twice
          ">chrLast\n" + wrap(s1[:500], 60))
    sam = ""
    for i in range(300):
        c = rng.choice(["chrA", "chrB", "chrC", "chrD", "chrC desc", "empty", "", "chrLast"])
        sam += sam_line("m%d" % i, rng.choice([0, 16]), c, rng.randint(1, 5200), rng.choice(["64M", "5S59M"]))
    case("line_ends_and_whitespace", {"g.fa": fa, "t.sam": sam}, ["-s", "t.sam", "-g", "g.fa"])

    # 3: edges of a record: clips at position 1 (a negative start wraps), windows cut short at both ends, tags shorter
    #    than the cut site, a later search that finds nothing after one that did
    a = "CCGG" + with_sites(rng, 1200) + "CTGCAG"
    b = rand_seq(rng, 900, "AT") + "CCGG" + rand_seq(rng, 50, "AT")
    fa = ">r1\n%s>r2\n%s>r1\n%s>end\nACGT\n" % (wrap(a, 60), wrap(b, 60), wrap(rand_seq(rng, 700, "AT"), 60))
    sam = "".join([
        sam_line("clip1", 0, "r1", 1, "5S59M"), sam_line("clip2", 16, "r1", 1, "10S54M"), sam_line("start", 0, "r1", 1),
        sam_line("nearend", 0, "r1", 1190), sam_line("revstart", 16, "r1", 1), sam_line("revend", 16, "r1", 1200),
        sam_line("short2", 0, "r1", 3, "2M", "AC"), sam_line("short0", 0, "r1", 3, "0M", ""),
        sam_line("short1r", 16, "r1", 600, "1M", "G"), sam_line("past", 0, "r1", 5000), sam_line("pastrev", 16, "r1", 5000),
        sam_line("neg", 0, "r1", -20), sam_line("b1", 0, "r2", 100), sam_line("b2", 16, "r2", 950),
        sam_line("zero", 0, "r1", 0)])
    case("record_edges", {"g.fa": fa, "t.sam": sam}, ["-s", "t.sam", "-g", "g.fa", "-o", "edges.csv"])

    # 4: an empty cut site (trailing comma), and the ZeroDivisionError it can cause
    fa = ">r1\n%s>r2\nNNNNNNNNNNNNCCGG\n>z\nA\n" % wrap(with_sites(rng, 800), 60)
    sam = sam_line("t1", 0, "r1", 10) + sam_line("t2", 16, "r1", 500) + sam_line("t3", 0, "r1", 790)
    case("empty_cut_site", {"g.fa": fa, "t.sam": sam}, ["-s", "t.sam", "-g", "g.fa", "-c", "CCGG,"])
    case("empty_cut_site_zero_division", {"g.fa": fa, "t.sam": sam + sam_line("t0", 0, "r1", 5, "0M", "")},
         ["-s", "t.sam", "-g", "g.fa", "-c", "CCGG,"])
    case("all_n_zero_division", {"g.fa": fa, "t.sam": sam_line("n3", 0, "r2", 1, "3M", "NNN")},
         ["-s", "t.sam", "-g", "g.fa", "-c", ",CCGG"])

    # 5: -d: renaming by the file's name, and the IndexError of the renaming rule
    fa = ">scaffold_7\n%s>other\nACGT\n" % wrap(with_sites(rng, 3000), 60)
    sam = "".join(sam_line("d%d" % i, rng.choice([0, 16]), "chrQ", rng.randint(1, 3000)) for i in range(40))
    case("dir_rename", {"gdir/chrQ.fa": fa, "t.sam": sam}, ["-s", "t.sam", "-d", "gdir"])
    case("dir_rename_indexerror", {"gdir/zzz.fa.gz": gzip.compress(fa.encode(), mtime=0), "t.sam": sam},
         ["-s", "t.sam", "-d", "gdir"])
    case("dir_no_rename", {"gdir/chrQ.v1.fasta": ">chrQ\n" + wrap(with_sites(rng, 3000), 60) + ">x\nA\n", "t.sam": sam},
         ["-s", "t.sam", "-d", "gdir", "-o", "d.csv"])

    # 6: gzip by name: .gz, .GZ (read as text), a damaged .gz
    fa = ">g1\n%s>g2\n%s>g3\nACGT\n" % (wrap(with_sites(rng, 4000), 60), wrap(with_sites(rng, 2000), 61))
    sam = "".join(sam_line("z%d" % i, rng.choice([0, 16]), rng.choice(["g1", "g2"]), rng.randint(1, 4000)) for i in range(60))
    blob = gzip.compress(fa.encode(), mtime=0)
    case("gz_genome", {"g.fa.gz": blob, "t.sam": sam}, ["-s", "t.sam", "-g", "g.fa.gz"])
    case("GZ_upper_is_text", {"g.fa.GZ": blob, "t.sam": sam}, ["-s", "t.sam", "-g", "g.fa.GZ"])
    case("gz_truncated", {"g.fa.gz": blob[:len(blob) // 2], "t.sam": sam}, ["-s", "t.sam", "-g", "g.fa.gz"])
    bad = bytearray(blob)
    bad[-8] ^= 0xFF                                                # CRC-32 of the member
    case("gz_bad_crc", {"g.fa.gz": bytes(bad), "t.sam": sam}, ["-s", "t.sam", "-g", "g.fa.gz"])
    case("genome_missing", {"t.sam": sam}, ["-s", "t.sam", "-g", "nothere.fa"])

    # 7: the -e / -c paths
    fa = ">e1\n%s>e2\nA\n" % wrap(with_sites(rng, 3000, ("CTGCAG", "CCGG", "ATGCAT")), 60)
    sam = "".join(sam_line("e%d" % i, rng.choice([0, 16]), "e1", rng.randint(1, 3000)) for i in range(50))
    files = {"g.fa": fa, "t.sam": sam}
    base = ["-s", "t.sam", "-g", "g.fa"]
    case("enzyme_clark", files, base + ["-e", "PstI-MspI-Clark"])
    case("enzyme_prefix_nsi", files, base + ["-e", "NsiI"])
    case("enzyme_with_matching_sites", files, base + ["-e", "NsiI-MspI", "-c", " ccgg ,ATGCAT"])
    case("enzyme_sites_mismatch", files, base + ["-e", "PstI", "-c", "CCGG"])
    case("enzyme_not_found", files, base + ["-e", "EcoRI"])
    case("cutsite_non_acgt", files, base + ["-c", "CCGN"])
    case("cutsites_lower_and_spaces", files, base + ["-c", " ccgg , ctgcag,GCCGGC"])
    case("overlapping_sites", files, base + ["-c", "CCGCCG,CGCC,GG"])
    case("both_g_and_d", files, base + ["-d", "."])
    case("neither_g_nor_d", files, ["-s", "t.sam"])
    case("working_dir", {"w/g.fa": fa, "w/t.sam": sam}, ["-s", "t.sam", "-g", "g.fa", "-w", "w", "-o", "o.csv"])

    # 8: UNEAK query / hit pairs, and the SAM reader's failures
    u = with_sites(rng, 3000)
    fa = ">u1\n%s>u2\nA\n" % wrap(u, 60)
    sam = "".join([
        sam_line("TP1_query_64", 0, "u1", 100), sam_line("TP1_hit_64", 0, "u1", 100),
        sam_line("TP2_query_64", 16, "u1", 900), sam_line("TP2_hit_64", 16, "u1", 900),
        sam_line("TP3_query_64", 0, "u1", 500), sam_line("TP3_hit_64", 0, "u1", 501),
        sam_line("TP4_query_64", 4, "u1", 700), sam_line("TP4_hit_64", 4, "u1", 700),
        sam_line("plain", 0, "u1", 1500)])
    case("uneak_pairs", {"g.fa": fa, "t.sam": sam}, ["-s", "t.sam", "-g", "g.fa"])
    case("uneak_names_differ", {"g.fa": fa, "t.sam": sam_line("TP1_query_64", 0, "u1", 1) + sam_line("TP9_hit_64", 0, "u1", 1)},
         ["-s", "t.sam", "-g", "g.fa"])
    case("uneak_hit_first", {"g.fa": fa, "t.sam": sam_line("TP1_hit_64", 0, "u1", 1)}, ["-s", "t.sam", "-g", "g.fa"])
    case("sam_blank_line", {"g.fa": fa, "t.sam": sam_line("a", 0, "u1", 5) + "\n"}, ["-s", "t.sam", "-g", "g.fa"])
    case("sam_bad_position", {"g.fa": fa, "t.sam": sam_line("a", 0, "u1", 5).replace("\t5\t", "\tx5\t")},
         ["-s", "t.sam", "-g", "g.fa"])

    # 9: a genome byte >= 0x80 (the locale's codec decides; the host path reproduces it)
    fa = ">n1 café\n%s>n2\n%s>n3\nA\n" % (wrap(with_sites(rng, 2000), 60), wrap(with_sites(rng, 900), 60))
    sam = "".join(sam_line("x%d" % i, rng.choice([0, 16]), rng.choice(["n1 café", "n2"]), rng.randint(1, 1900))
                  for i in range(20))
    case("non_ascii_genome", {"g.fa": fa, "t.sam": sam}, ["-s", "t.sam", "-g", "g.fa"])
    return out


def run_case(c):
    with tempfile.TemporaryDirectory() as d:
        for name, b64 in c["files"].items():
            p = os.path.join(d, name)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as fh:
                fh.write(zlib.decompress(base64.b64decode(b64)))
        env = dict(os.environ, PYTHONPATH=REF, PYTHONDONTWRITEBYTECODE="1", LC_ALL="C.UTF-8")
        r = subprocess.run([sys.executable, os.path.join(REF, "exp_frag_size.py")] + c["args"], cwd=d, env=env,
                           capture_output=True)
        c["stdout"] = r.stdout.decode()
        if r.returncode:
            last = r.stderr.decode().strip().splitlines()[-1]
            cls, _, msg = last.partition(": ")
            c["exception"] = {"class": cls.split(":")[0], "message": msg}
            c["csv_b64"] = None
        else:
            c["exception"] = None
            args = c["args"]
            wd = args[args.index("-w") + 1] if "-w" in args else "."
            out = args[args.index("-o") + 1] if "-o" in args else "out.csv"
            with open(os.path.join(d, wd, out), "rb") as fh:
                c["csv_b64"] = pack(fh.read())
    return c


if __name__ == "__main__":
    if REF is None:
        sys.exit(__doc__)
    got = [run_case(c) for c in cases()]
    with open(os.path.join(HERE, "fragsize.json"), "w") as fh:
        json.dump(got, fh, indent=0, sort_keys=True)
        fh.write("\n")
    for c in got:
        print("%-32s %s" % (c["name"], c["exception"]["class"] if c["exception"] else "ok, %d progress lines" %
                            len(c["stdout"].splitlines())))
