#!/usr/bin/env python3
"""Generate tests/golden/tag_manager.json from the REAL reference tag_manager.py and tagdigger_fun.py (build container
only; data only, never reference code).

Two kinds of case:
  transcripts  tag_manager.py run with PYTHONHASHSEED=0 in a scratch directory holding the case's files, its answers
               piped on stdin: stdout (the scratch directory's path replaced by {CWD}), every file written or
               changed, and the exception's last traceback line (or null);
  functions    Tag Manager functions of the reference module called directly: result (sets as sorted lists),
               stdout, files written, or the exception.
Payloads are base64 of a zlib stream.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_tag_manager_golden.py REFERENCE_DIR
"""
import base64
import contextlib
import io
import json
import os
import random
import subprocess
import sys
import tempfile
import zlib

REF = sys.argv[1] if len(sys.argv) > 1 else None
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

if REF and os.environ.get("PYTHONHASHSEED") != "0":      # set order is part of the results: fix the hash seed
    env = dict(os.environ, PYTHONHASHSEED="0", PYTHONDONTWRITEBYTECODE="1")
    sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))


def pack(data):
    return base64.b64encode(zlib.compress(data if isinstance(data, bytes) else data.encode(), 9)).decode()


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def snp(rng, s, pos=None):
    pos = rng.randrange(5, len(s) - 5) if pos is None else pos
    alt = rng.choice([b for b in "ACGT" if b != s[pos]])
    return s[:pos] + alt + s[pos + 1:], pos


def merged(a, b):
    """[x/y] form of two equal-length tags differing at some sites."""
    d = [i for i in range(len(a)) if a[i] != b[i]]
    lo, hi = d[0], d[-1]
    return a[:lo] + "[" + a[lo:hi + 1] + "/" + b[lo:hi + 1] + "]" + a[hi + 1:]


# ------------------------------------------------------------------ fixtures
def study(seed):
    """An old database and a new study that overlaps it: exact matches, shorter / longer versions, a third allele,
    markers sharing one tag, and new markers."""
    rng = random.Random(seed)
    old = []                                  # (marker, [tags])
    for i in range(1, 25):
        a = "TGCAG" + rand_seq(rng, 59)
        b, _ = snp(rng, a, rng.randrange(5, 45))
        old.append(("Mrkr%03d" % i, [a, b]))
    a = old[3][1][0]                          # a marker sharing a tag with marker 4 (consolidated in option 2)
    c, _ = snp(rng, a, 40)
    old.append(("Mrkr030", [a, c]))
    new = []
    for k, (m, tags) in enumerate(old[:10]):
        if k % 3 == 0:
            new.append(("TP%d" % (100 + k), list(tags)))                     # same tags
        elif k % 3 == 1:
            new.append(("TP%d" % (100 + k), [t[:50] for t in tags]))         # shorter versions
        else:
            third, _ = snp(rng, tags[0], 20)
            new.append(("TP%d" % (100 + k), [tags[0], third]))               # one tag shared, one new
    for k in range(6):
        a = "TGCAG" + rand_seq(rng, 59)
        b, _ = snp(rng, a)
        new.append(("TP%d" % (200 + k), [a, b]))
    return old, new


def db_csv(markers, extra=None):
    extra = extra or {}
    heads = ["Chrom", "Position"]
    out = "Marker name,Tag sequence," + ",".join(heads) + "\n"
    for i, (m, tags) in enumerate(markers):
        row = extra.get(m, ["Chr%02d" % (i % 3 + 1), str(1000 * (i + 1))])
        out += "%s,%s,%s\n" % (m, merged(tags[0], tags[1]), ",".join(row))
    return out


def rows_csv(markers):
    out = "Marker name,Allele name,Tag sequence\n"
    for m, tags in markers:
        for k, t in enumerate(tags):
            out += "%s,%d,%s\n" % (m, k, t)
    return out


def merged_csv(markers):
    out = "Marker name,Tag sequence\n"
    for m, tags in markers:
        out += "%s,%s\n" % (m, merged(tags[0], tags[1]))
    return out


UNEAK = (">TP276_query_64\nTGCAGAAAAACACGTATCTTTGCTTCTACCAGATGCACAAAGAGAGGGGAAATAGGCAAGAGCAA\n"
         ">TP276_hit_64\nTGCAGAAAAACACGTCTCTTTGCTTCTACCAGATGCACAAAGAGAGGGGAAATAGGCAAGAGCAA\n"
         ">TP539_query_30\nTGCAGAAAACACAGAAACAGAACCATGCACAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA\n"
         ">TP539_hit_64\nTGCAGAAAACACAGAAACAGAACTATGCACGAGTCACCAGCGGCTGAAAAACATGAATGATAGAG\n"
         ">TP777_query_64\nTGCAGTTTTACACAGAAACAGAACCATGCACGAGTCACCAGCGGCTGAAAAACATGAATGATAGAG\n"
         ">TP777_hit_64\nTGCAGTTTTACACAGAAACAGAACCATGCACGAGTCACCAGCGGCTGAAAAACATGTATGATAGAG\n")
COLUMNS = ("Marker name,Tag sequence 0,Tag sequence 1\nTP276,TGCAGAAAAACACGTATCTTTG,TGCAGAAAAACACGTCTCTTTG\n"
           "M2,ACGTACGTAAGGT,ACCTACGTTAGGT\nM3,TTGCAGCATCATCAG,TTGCAGCTTCATCAG\n")
ROWS3 = ("Marker name,Allele name,Tag sequence\nTP276,0,TGCAGAAAAACACGTATCT\nTP276,1,TGCAGAAAAACACGTCTCT\n"
         "Mrker4050,0,TGCAGAGAG\nMrker4050,1,TGCAGAGTG\nMrker4050,2,tgcagagcg\nMx,a,TGCAGTTTTT\nMx,b,TGCAGTTTTTAC\n")
STACKS = {"cat.tags.tsv": "# comment\n" + "".join("0\t1\t%s\t\t0\t+\tconsensus\t0\t\t%s\t0\t0\t0\n" % r for r in
                                                  [("1", "TGCAGAAAACCCCGGGGTTTT"), ("2", "TGCAGTTTTGGGGCCCCAAAA"),
                                                   ("4", "tgcagcccccaaaaa")]),
          "cat.snps.tsv": "# c\n" + "".join("0\t1\t%s\t%d\tE\t0\tA\tC\n" % r for r in [("1", 7), ("1", 12), ("2", 9)]),
          "cat.alleles.tsv": "# c\n" + "".join("0\t1\t%s\t%s\t50.0\t10\n" % r for r in
                                               [("1", "AC"), ("1", "GT"), ("1", "AT"), ("2", "C"), ("2", "A"), ("4", "")])}
STACKS2 = {"t.tsv": "# c\n1\t7\t\t\t\tTGCAGAAAACCCC\n1\t8\t\t\t\tTGCAGTTTTGGGG\n",
           "s.tsv": "1\t7\t6\tE\n1\t8\t5\tE\n", "a.tsv": "1\t7\tA\n1\t7\tG\n1\t8\tC\n1\t8\tA\n"}
TASSEL = ("@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:Chr01\tLN:43270923\n@SQ\tSN:scaffold_12\tLN:9000\n@PG\tID:bowtie2\n"
          "tagSeq=A\t0\tChr01\t1000\t42\t20M\t*\t0\t0\tTGCAGAAAACCCCGGGGTTT\tIIII\n"
          "tagSeq=B\t0\tChr01\t1000\t42\t20M\t*\t0\t0\tTGCAGAAAACCCCGGTGTTT\tIIII\n"
          "tagSeq=C\t16\tChr01\t2000\t42\t10M2D8M\t*\t0\t0\tAAACCCGGGTTTACTGCA\tIIII\n"
          "tagSeq=D\t16\tChr01\t2000\t42\t10M2D8M\t*\t0\t0\tAAACCCGGGTTAACTGCA\tIIII\n"
          "tagSeq=E\t4\t*\t0\t0\t*\t*\t0\t0\tTGCAGGGGGGGGGG\tIIII\n"
          "tagSeq=F\t0\tscaffold_12\t77\t42\t12M\t*\t0\t0\tTGCAGTTTTTTT\tIIII\n"
          "tagSeq=H\t0\tscaffold_12\t77\t42\t12M\t*\t0\t0\tTGCAGTTATTTT\tIIII\n")
PYRAD = (">s1_0    TGCAGAAAACCCCGGGG--\n>s1_1    TGCAGAAAACCCCGGGG--\n>s2_0    TGCAGAAAATCCCGGGGTT\n>s2_1    TGCAGAAAACCCCGGGG\n"
         "//                   *              |0|\n"
         ">s1_0    TGCAGCA\n>s1_1    TGCAGCC\n>s2_0    TGCAGCG\n"
         "//      * |13|\n")


def transcripts():
    old, new = study(20261016)
    db = db_csv(old)
    extra = "Marker name,Chrom,Notes\n" + "".join("%s,ChrN%d,note %d\n" % (m, i, i) for i, (m, _) in enumerate(new))
    extra_new = "Marker name,Source,Notes\n" + "".join("%s,study2,n%d\n" % (m, i) for i, (m, _) in enumerate(new[::2]))
    # a SAM of the database's markers: unmapped, reverse strand, secondary flags
    sam = "@HD\tVN:1.0\n@SQ\tSN:Chr01\tLN:100000\n"
    for i, (m, tags) in enumerate(old):
        flag = [0, 16, 4, 0, 16, 20, 256, 272][i % 8]
        sam += "%s\t%d\tChr%02d\t%d\t%d\t64M\t*\t0\t0\t%s\tIIII\n" % (m, flag, i % 3 + 1, 500 * i + 7, 30 + i % 12, tags[0])
    keep = "TP276\n\nTP777,\n  TP539  \n"
    keep_many = "".join("M%d\n" % i for i in range(12)) + "TP276\n"
    C = []

    def case(name, files, answers, note=""):
        C.append({"name": name, "files": files, "stdin": "".join(a + "\n" for a in answers), "note": note})

    d = ["n"]                                      # keep the directory
    # option 4, one case per tag format
    case("new_merged_all_extras", {"tags.csv": merged_csv(new), "extra.csv": extra},
         ["x", "n", "9", "4", "maybe", "N", "", "2", "tags.csv", "", "Abc", "0", "3", "y", "", "new.fa",
          "q", "y", "", "Original", "y", "missing.csv", "extra.csv", "", "db_new.csv", ""])
    case("new_uneak_keep", {"u.fa": UNEAK, "keep.txt": keep},
         d + ["4", "y", "nokeep.txt", "keep.txt", "1", "u.fa", "Mk", "4", "n", "n", "n", "out.csv", ""])
    case("new_uneak_keep_many", {"u.fa": UNEAK, "keep.txt": keep_many},
         d + ["4", "Y", "keep.txt", "1", "u.fa", "Mk", "2", "y", "u.fasta", "y", "orig", "n", "out.csv", ""])
    case("new_columns", {"c.csv": COLUMNS}, d + ["4", "n", "3", "c.csv", "P", "1", "y", "c.fa", "n", "n", "o.csv", ""])
    case("new_rows_three_alleles", {"r.csv": ROWS3},
         d + ["4", "n", "4", "r.csv", "Q", "5", "y", "r.fa", "y", "Orig", "n", "o.csv", ""])
    case("new_stacks_v1", STACKS, d + ["4", "n", "5", "cat.tags.tsv", "cat.snps.tsv", "cat.alleles.tsv", "3", "1", "x", "n",
                                       "S", "2", "y", "s.fa", "y", "Stacks", "n", "o.csv", ""])
    case("new_rows_ok", {"r.csv": ROWS3.split("Mx,")[0]},
         d + ["4", "n", "4", "r.csv", "Q", "5", "y", "r.fa", "y", "Orig", "n", "o.csv", ""])
    case("new_stacks_v1_binary", STACKS, d + ["4", "n", "5", "cat.tags.tsv", "cat.snps.tsv", "cat.alleles.tsv", "1", "y",
                                              "S", "2", "y", "s.fa", "n", "n", "o.csv", ""])
    case("new_stacks_v2_binary", STACKS2, d + ["4", "n", "5", "t.tsv", "s.tsv", "a.tsv", "2", "y", "S", "3", "n", "n", "n",
                                               "o.csv", ""])
    case("new_tassel_key", {"t.sam": TASSEL}, d + ["4", "n", "6", "t.sam", "n", "n", "y", "key.csv", "T", "4", "y", "t.fa",
                                                  "y", "TASSEL", "n", "o.csv", ""])
    case("new_tassel_binary", {"t.sam": TASSEL}, d + ["4", "n", "6", "t.sam", "y", "n", "T", "4", "n", "n", "n", "o.csv", ""])
    case("new_pyrad", {"p.alleles": PYRAD}, d + ["4", "n", "7", "p.alleles", "n", "R", "2", "y", "p.fa", "n", "n", "o.csv", ""])
    case("new_retry_single_tag",
         {"bad.csv": "Marker name,Allele name,Tag sequence\nA1,0,ACGTACGT\nA2,0,ACGTTCGT\nA2,1,ACGTACGA\n",
          "good.csv": rows_csv(new[:4])},
         d + ["4", "n", "4", "missing.csv", "4", "bad.csv", "n", "4", "good.csv", "G", "1", "n", "n", "n", "o.csv", ""])
    case("new_identical_tags", {"r.csv": "Marker name,Allele name,Tag sequence\nA1,0,ACGTACGT\nA1,1,acgtacgt\n"},
         d + ["4", "n", "4", "r.csv"], "readTags_Rows rejects the duplicate; the program then reads stdin to its end")
    # option 1
    case("lookup_subset_adl_select", {"db.csv": db, "new.csv": rows_csv(new)},
         d + ["1", "n", "4", "new.csv", "nodb.csv", "db.csv", "z", "y", "y", "q", "s", "y", "n", "lookup.csv", ""])
    case("lookup_perfect_all", {"db.csv": db, "new.csv": rows_csv(new)},
         d + ["1", "n", "4", "new.csv", "db.csv", "n", "n", "a", "lookup.csv", ""])
    case("lookup_subset_exact_none", {"db.csv": db, "new.csv": merged_csv(new)},
         d + ["1", "n", "2", "new.csv", "db.csv", "y", "n", "n", "", "lookup.csv", ""])
    case("lookup_perfect_adl", {"db.csv": db, "new.csv": rows_csv(new)},
         d + ["1", "n", "4", "new.csv", "db.csv", "n", "y", "a", "lookup.csv", ""])
    # option 2
    case("add_perfect_orig_fasta_extra_old", {"db.csv": db, "new.csv": rows_csv(new), "extra.csv": extra},
         d + ["2", "n", "4", "new.csv", "db.csv", "n", "y", "", "Study2", "", "Mk", "x", "", "", "y", "new.fa",
              "y", "extra.csv", "x", "o", "", "merged.csv", ""])
    case("add_perfect_extra_new_renumber", {"db.csv": db, "new.csv": rows_csv(new), "extra.csv": extra},
         d + ["2", "n", "4", "new.csv", "db.csv", "n", "n", "", "5", "2", "24", "40", "n", "y", "extra.csv", "n",
              "merged.csv", ""])
    case("add_perfect_no_overlap_cols", {"db.csv": db, "new.csv": rows_csv(new), "extra.csv": extra_new},
         d + ["2", "n", "4", "new.csv", "db.csv", "n", "n", "", "", "", "n", "y", "extra.csv", "merged.csv", ""])
    case("add_consolidate_adl", {"db.csv": db, "new.csv": rows_csv(new), "extra.csv": extra},
         d + ["2", "n", "4", "new.csv", "db.csv", "y", "y", "y", "Orig", "", "", "", "y", "new.fa", "y", "extra.csv",
              "n", "merged.csv", ""])
    case("add_consolidate_exact", {"db.csv": db, "new.csv": rows_csv(new)},
         d + ["2", "n", "4", "new.csv", "db.csv", "y", "n", "n", "Zz", "", "", "y", "new.fa", "n", "merged.csv", ""])
    case("add_last_name_without_digits", {"db.csv": db + "Zeta,TGCAGAA[A/C]TT,Chr01,5\n", "new.csv": rows_csv(new)},
         d + ["2", "n", "4", "new.csv", "db.csv", "y", "y", "n"])
    # option 3
    case("align_fasta_varsites", {"db.csv": db, "a.sam": sam},
         d + ["3", "db.csv", "y", "all.fa", "y", "nosam.sam", "a.sam", "", "Chrom", "Pos", "Qual", "SNP", "aligned.csv", ""])
    case("align_plain", {"db.csv": db, "a.sam": sam},
         d + ["3", "db.csv", "n", "n", "a.sam", "Chr", "Pos", "MapQ", "aligned.csv", ""])
    case("align_bad_sam", {"db.csv": db, "a.sam": "@HD\nMrkr001\n", "b.sam": sam},
         d + ["3", "db.csv", "n", "n", "a.sam", "b.sam", "C", "P", "Q", "aligned.csv", ""])
    # the working directory prompt
    case("change_directory", {"sub/db.csv": db, "sub/new.csv": rows_csv(new)},
         ["y", "nosuchdir", "sub", "1", "n", "4", "new.csv", "db.csv", "y", "y", "n", "out.csv", ""])
    return C


FIXTURES = {}                                          # input files and arguments shared by several cases


def fixture(data, key=None):
    """Store data once; cases refer to it by key (default: a digest of the data)."""
    import hashlib
    raw = data if isinstance(data, bytes) else data.encode()
    key = key or hashlib.sha1(raw).hexdigest()[:12]
    FIXTURES[key] = pack(raw)
    return key


def run_transcript(c):
    with tempfile.TemporaryDirectory() as d:
        d = os.path.realpath(d)
        for name, text in c["files"].items():
            p = os.path.join(d, name)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as fh:
                fh.write(text.encode() if isinstance(text, str) else text)
        before = {}
        for root, _, files in os.walk(d):
            for f in files:
                p = os.path.join(root, f)
                before[os.path.relpath(p, d)] = open(p, "rb").read()
        env = dict(os.environ, PYTHONHASHSEED="0", PYTHONDONTWRITEBYTECODE="1")
        r = subprocess.run([sys.executable, os.path.join(REF, "tag_manager.py")], cwd=d, input=c["stdin"].encode(),
                           capture_output=True, env=env, timeout=300)
        outputs = {}
        for root, _, files in os.walk(d):
            for f in files:
                p = os.path.join(root, f)
                rel = os.path.relpath(p, d)
                data = open(p, "rb").read()
                if before.get(rel) != data:
                    outputs[rel] = pack(data)
        err = r.stderr.decode().strip().splitlines()
        return {"name": c["name"], "note": c["note"], "files": {k: fixture(v) for k, v in c["files"].items()},
                "stdin": c["stdin"], "stdout_b64": pack(r.stdout.decode().replace(d, "{CWD}")), "returncode": r.returncode,
                "exception": err[-1] if r.returncode else None, "outputs": outputs}


# ------------------------------------------------------------------ function-level cases
def lookup_sets():
    rng = random.Random(7)
    sets = []
    # the issue's example and its variant without the second extension
    sets.append(("quirk", ["AC", "AC", "ACGTA", "ACGTC"], ["p1_0", "p2_0", "e1_0", "e2_0"], ["ACGT", "AC", "ACG", "ACGTA", "A"]))
    sets.append(("quirk_one_ext", ["AC", "AC", "ACGTA"], ["p1_0", "p2_0", "e1_0"], ["ACGT", "AC", "ACGTAA"]))
    # 10 000 duplicates under different names, with prefixes and extensions around them
    dup = "TGCAGACGTACGTTT"
    seqs = [dup] * 10000 + ["TGCAG", "TGCAGACG", dup + "A", dup + "C", "TGCAGT"]
    names = ["D%02d_%05d_0" % (i % 40, i) for i in range(10000)] + ["P1_a", "P2_a", "E1_a", "E2_a", "O_a"]
    sets.append(("dups_10k", seqs, names, [dup, dup + "AG", "TGCAGACGT", "TGCAGACGTACG", "TGCAG", dup + "A"]))
    # nested prefixes A, AC, ACG, ... with other strings between them
    base = "ACGTTGCAAGCTTACG"
    seqs, names = [], []
    for k in range(1, len(base) + 1):
        seqs.append(base[:k])
        names.append("N%02d_0" % k)
        seqs.append(base[:k - 1] + ("T" if base[k - 1] != "T" else "G") + "AAA")
        names.append("B%02d_0" % k)
    seqs += [base[:6]] * 3
    names += ["R1_0", "R2_0", "R3_0"]
    sets.append(("nested_prefixes", seqs, names, [base, base + "AC", base[:9], base[:5] + "T", "AC", "ACGTTGCAAGCTTACGT"]))
    # several distinct extensions of one query
    q = rand_seq(rng, 40)
    seqs = [q + rand_seq(rng, 5) for _ in range(6)] + [q[:20], q[:20], q[:30]]
    names = ["X%d_0" % i for i in range(len(seqs))]
    sets.append(("extensions", seqs, names, [q, q[:25], q[:20], q[:35], q + "A"]))
    # tags of 31, 32, 33, 64 and 65 bases (word seams) with A-tail prefixes
    t = rand_seq(rng, 70)
    seqs, names = [], []
    for L in (31, 32, 33, 64, 65):
        seqs += [t[:L], t[:L] + "A", t[:L] + "AA", t[:L - 1] + "A"]
        names += ["L%dz_0" % L, "L%da_0" % L, "L%db_0" % L, "L%dc_0" % L]
    seqs += [t[:32] + "A" * 33, t[:31] + "A"]
    names += ["T1_0", "T2_0"]
    sets.append(("word_seams", seqs, names, [t[:31], t[:32], t[:33], t[:64], t[:65], t[:32] + "A", t[:32] + "AAAA",
                                             t[:70], t[:31] + "AA", t[:20], t[:64] + "AAA"]))
    # random sets with shared prefixes
    for r in range(2):
        stem = [rand_seq(rng, 10) for _ in range(4)]
        seqs = []
        for _ in range(300):
            s = rng.choice(stem) + rand_seq(rng, rng.randrange(0, 12))
            seqs.append(s[:rng.randrange(1, len(s) + 1)])
        names = ["R%d%03d_%d" % (r, i % 97, i) for i in range(len(seqs))]
        queries = [x for x in rng.sample(seqs, 40)] + [rng.choice(stem)[:rng.randrange(1, 11)] for _ in range(20)] + \
                  [rand_seq(rng, rng.randrange(1, 25)) for _ in range(20)]
        sets.append(("random_%d" % r, seqs, names, queries))
    return sets


def functions(ref, sets, lookups):
    out = []

    def call(func, args, kwargs=None, files=None, note=""):
        kwargs = kwargs or {}
        files = files or {}
        with tempfile.TemporaryDirectory() as d:
            old = os.getcwd()
            os.chdir(d)
            try:
                for name, text in files.items():
                    with open(name, "w", newline="") as fh:
                        fh.write(text)
                before = set(os.listdir("."))
                buf = io.StringIO()
                text = json.dumps(args).replace(json.dumps(otags), '"@old"').replace(json.dumps(ntags), '"@new"')
                rec = {"func": func, "args_b64": pack(text), "kwargs": kwargs, "files": files, "note": note}
                try:
                    with contextlib.redirect_stdout(buf):
                        res = getattr(ref, func)(*args, **kwargs)
                    rec["result_b64"] = pack(json.dumps(jsonable(res)))
                except Exception as e:
                    rec["raises"] = type(e).__name__
                    rec["message"] = str(e)
                rec["stdout"] = buf.getvalue()
                rec["written"] = {n: pack(open(n, "rb").read()) for n in sorted(set(os.listdir(".")) - before)}
            finally:
                os.chdir(old)
        out.append(rec)

    for name, seqs, names, queries in lookup_sets():
        srt = ref.sortTagsBySeq([names, seqs])
        where = {x: i for i, x in enumerate(names)}
        perm = [where[x] for x in srt[0]]                  # names are unique: the sorted order as input indices, deltas
        sets[name] = {"names": pack("\n".join(names)), "seqs": pack("\n".join(seqs)),
                      "sorted_deltas": pack(json.dumps([perm[0]] + [b - a for a, b in zip(perm, perm[1:])]))}
        for adl in (False, True):
            each = [sorted(ref.lookupMarkerByTag(srt[0], srt[1], [q], allowDiffLengths=adl)) for q in queries]
            every = sorted(ref.lookupMarkerByTag(srt[0], srt[1], queries, allowDiffLengths=adl))
            lookups.append({"set": name, "queries": queries, "allowDiffLengths": adl,
                            "each_b64": pack(json.dumps(each)), "all_b64": pack(json.dumps(every))})
    old, new = study(99)
    global otags, ntags
    otags = [[], []]
    for m, tags in old:
        for k, t in enumerate(tags):
            otags[0].append("%s_%d_%d" % (m, k, k))
            otags[1].append(t)
    ntags = [[], []]
    for m, tags in new:
        for k, t in enumerate(tags):
            ntags[0].append("%s_%d" % (m, k))
            ntags[1].append(t)
    fixture(json.dumps(otags), "@old")
    fixture(json.dumps(ntags), "@new")
    for pm in (False, True):
        for adl in (False, True):
            call("compareTagSets", [otags, ntags], {"perfectMatch": pm, "allowDiffLengths": adl})
    for adl in (False, True):
        call("consolidateTagSets", [otags, ntags], {"allowDiffLengths": adl, "prefix": "Q", "numdig": 4, "startnumnew": 7})
        call("consolidateTagSets", [ntags], {"allowDiffLengths": adl})
    call("consolidateTagSets", [[[], []], ntags])
    call("compareTagSets", [[[], []], ntags])
    call("compareTagSets", [otags, [ntags[0] + ntags[0][:1], ntags[1] + ["ACGT"]]])
    call("mergedTagList", [otags])
    call("mergedTagList", [ntags])
    call("mergedTagList", [[["A_0", "A_1", "B_0"], ["ACGT", "ACTT", "ACGG"]]])
    call("mergedTagList", [[["A_0", "A_1"], ["ACGT", "ACGT"]]])
    call("mergedTagList", [[["A_0", "A_1"], ["ACGT", "ACNT"]]])
    call("mergedTagList", [[["A_1", "A_0", "A_2"], ["ACGTAAC", "ACTT", "ACGTTTTTG"]]])
    call("mergeTags", [["ACGTA", "ACGTAAG", "TCGTA"]])
    call("mergeTags", [[]])
    call("varSitesByMarker", [otags[0], otags[1]])
    call("varSitesByMarker", [["A_0", "A_1", "A_2", "B_0"], ["ACGTAAAA", "ACGTT", "TCGTAAAC", "GG"]])
    call("exportFasta", ["e.fa", otags[0][:20], otags[1][:20]])
    call("exportFasta", ["e.fa", ["A_0", "A_1", "A_2", "B_0"], ["ACGTAAAA", "ACGTT", "TCGTAAAC", "GG"]])
    call("exportFasta", ["e.fa", ["A B_0", "A B_1"], ["ACGT", "ACTT"]])
    call("exportFasta2", ["e2.fa", ["M1", "M2"], ["AC[A/G]T", "A[CC/GT]T"]])
    call("exportFasta2", ["e2.fa", ["M1", "M2"], ["AC[A/G]T", "A[CC/G]T"]])
    call("consolidateExtraCols", [[[["a", "b"], {"m1": ["1", "2"], "m2": ["3", "4"]}],
                                   [["b", "c"], {"m1": ["5", "6"], "m3": ["7", "8"]}],
                                   [["a"], {"m4": ["9"]}]]])
    call("readSAM", ["x.sam"], {"varDict": {"M1": [3, 10], "M2": []}},
         files={"x.sam": "@HD\nM1\t16\tc1\t100\t30\t8M\t*\t0\t0\tACGTACGTAC\nM2\t4\t*\t0\t0\nM2\t0\tc2\t5\t9\n"})
    call("readSAM", ["x.sam"], files={"x.sam": "M1\t0\tc1\n"})
    return out


def main():
    sys.path.insert(0, REF)
    import tagdigger_fun as ref
    sets, lookups = {}, []
    data = {"transcripts": [run_transcript(c) for c in transcripts()], "functions": functions(ref, sets, lookups),
            "lookup_sets": sets, "lookups": lookups, "fixtures": FIXTURES}
    out = os.path.join(HERE, "tag_manager.json")
    with open(out, "w") as fh:                         # one record per line
        fh.write("{\n")
        for k, key in enumerate(sorted(data)):
            items = data[key]
            if isinstance(items, dict):
                body = ",\n".join(json.dumps(n) + ": " + json.dumps(v, sort_keys=True) for n, v in sorted(items.items()))
                fh.write('"%s": {\n%s\n}' % (key, body))
            else:
                fh.write('"%s": [\n%s\n]' % (key, ",\n".join(json.dumps(v, sort_keys=True) for v in items)))
            fh.write(",\n" if k + 1 < len(data) else "\n}\n")
    print("wrote %s: %d transcripts, %d function calls, %d bytes" % (out, len(data["transcripts"]), len(data["functions"]),
                                                                     os.path.getsize(out)))
    for t in data["transcripts"]:
        print("  %-36s rc=%d %s" % (t["name"], t["returncode"], t["exception"] or ""))


def jsonable(x):
    if isinstance(x, set):
        return {"__set__": sorted(x)}
    if isinstance(x, dict):
        return {"__dict__": [[jsonable(k), jsonable(v)] for k, v in x.items()]}
    if isinstance(x, (list, tuple)):
        return [jsonable(v) for v in x]
    return x


if __name__ == "__main__":
    if not REF:
        sys.exit(__doc__)
    main()
