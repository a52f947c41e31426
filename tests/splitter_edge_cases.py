"""Inputs that reach the structural edges of the barcode splitter's two kernels: k_split2 (csrc/kernel_splitter2.hpp:
a 24 KiB tile staged in LDS, one lane per read, sites found 128 positions at a time, adapter entries in groups of eight
addressed by a read's last three characters) and k_split (csrc/kernel_splitter.hpp: lines walked in global memory),
which every input that does not fit k_split2's compact form falls back to.

Plain Python; the product is not imported here.  Three layers:

  * edge READS per adapter/barcode set (SETS), written as compact specs ("TTGACCTGCAG|AT*137|CCGG|AT": pieces joined,
    `unit*n` = the unit repeated and cut to n characters).  tests/golden/make_splitter_edges_golden.py evaluates the
    real reference on every one of them and writes tests/golden/splitter_edges.json; tests/test_splitter_edges.py holds
    the oracle's restatement against those answers.
  * the grouping rule of td_set_splitter restated (compact_form): which sets k_split2 can take.
  * CASES: FASTQ buffers built from those reads (and, for the tile geometry, filler records that only place bytes), each
    with its expected decisions from the oracle and self-checks that the buffer has the property it is named for.
    tests/test_splitter_edges_gpu.py runs them.

Geometry, stated here and in the GPU module, imported from nowhere:
    k_split2<6>: tile 24 576 bytes, halo 512, wave quarter 6 144, thread span 96, 384 line starts per wave list;
                 the site search takes windows of 128 text positions at a stride of 112, the first at 16 * (start >> 4)
    k_split<4>:  tile 16 384 bytes, thread span 64
"""
import collections
import functools
import random

from conftest import load_golden
from oracle import tagdigger_oracle as po

HALO = 512
GEOM = {24576: {"quarter": 6144, "span": 96, "list": 384}, 16384: {"quarter": 4096, "span": 64, "list": None}}
WINDOW, STRIDE = 128, 112
REGS = 80               # an entry's characters behind which only the overflow loop of the entry compare looks

HALL = [tuple(x) for x in load_golden("splitter.json")["adapters"]["PstI-MspI-Hall"]]


def _rnd_tail(seed, n, forbid=("CCGG", "CTGCAG")):
    """n random bases without a full site in them, nor with the remains in front."""
    rng = random.Random(seed)
    s = ""
    while len(s) < n:
        c = rng.choice("ACGT")
        if not any(f in ("CCG" + s + c)[-8:] for f in forbid):
            s += c
    return s


# name -> (adapter, barcodes, cut site).  `compact`: the kernel the query must report under split_kernel 2.
Set = collections.namedtuple("Set", "adapter barcodes cutsite compact")
SETS = collections.OrderedDict()
SETS["hall"] = Set(HALL, ["AACG", "TTGACC", "CGT", "GATTACAGGATC", "CCAC"], "TGCAG", True)
# one full site is the beginning of the other: both are found at the same position (the rs0 < rs1 tie)
SETS["prefix"] = Set([("CCG^G", "AGATCGGTT"), ("CCGGA^T", "[barcode]AGAT")], ["AACG", "TTGACC"], "TGCAG", True)
# a site of eight bases (the limit) that begins with the cut site's last letter, and a site of one base
SETS["lens"] = Set([("GATCCGG^C", "AGAT"), ("G^", "[barcode]TT")], ["AACT", "TTCACC"], "TGCAG", True)
# an empty site: str.find finds it at `start` itself
SETS["empty"] = Set([("^", "ACCA"), ("CTGCA^G", "[barcode]AGA")], ["AACG", "TTGACC"], "TGCAG", True)
# entries of one and two characters (nothing remains of the common cutter's site)
SETS["tiny"] = Set([("^CCGG", "GATC"), ("C^TGCAG", "[barcode]AGA")], ["AACG", "TTGACC"], "TGCAG", True)
# entries of 4 .. 128 characters: the compact form's longest, and the overflow loop of the compare
SETS["long"] = Set([("CCG^G", _rnd_tail(7, 125)), ("CTGCA^G", "[barcode]AGAT")], ["AACG", "TTGACC"], "TGCAG", True)
# one more character: not compact
SETS["len129"] = Set([("CCG^G", _rnd_tail(7, 126)), ("CTGCA^G", "[barcode]AGAT")], ["AACG", "TTGACC"], "TGCAG", False)
# the adapter returns to ...ACG eight times, each time behind other characters: a group of exactly eight entries
_SPACERS = ["TT", "AGT", "CAT", "GGA", "TCTA", "CTGA", "AATA", "GTCA", "TGTA"]
SETS["eight"] = Set([("CCG^G", "".join(s + "ACG" for s in _SPACERS[:7]) + "TT"), ("CTGCA^G", "[barcode]TTAT")],
                    ["AACG", "TTGACC"], "TGCAG", True)
SETS["nine"] = Set([("CCG^G", "".join(s + "ACG" for s in _SPACERS[:8]) + "TT"), ("CTGCA^G", "[barcode]TTAT")],
                   ["AACG", "TTGACC"], "TGCAG", False)
# a site with a letter outside ACGT (behind the cut, so that the entries stay ACGT): matched letter by letter
SETS["nsite"] = Set([("CCG^N", "CTCAGGCAT"), ("CTGCA^G", "[barcode]AGAT")], ["AACG", "TTGACC"], "TGCAG", False)
# the adapter repeats ACGTT behind other characters: two entries of one group share their last four characters
SETS["echo"] = Set([("CCG^G", "ATACGTTGGACGTTCA"), ("CTGCA^G", "[barcode]AGAT")], ["AACG", "TTGACC"], "TGCAG", True)


def sites_of(st):
    return st.adapter[0][0].replace("^", ""), st.adapter[1][0].replace("^", "")


def fulls_of(st, bc):
    """The two strings whose beginnings a read may end with."""
    a0, a1 = st.adapter
    return (a0[0][:a0[0].find("^")] + a0[1],
            a1[0][:a1[0].find("^")] + a1[1].replace("[barcode]", po.reverse_complement(bc)))


# ---------------------------------------------------------------------------------------------------- read specs
def expand(spec):
    out = []
    for tok in spec.split("|"):
        if "*" in tok:
            unit, n = tok.split("*")
            n = int(n)
            out.append((unit * (n // len(unit) + 1))[:n])
        else:
            out.append(tok)
    return "".join(out)


def at(n):
    return "AT*%d" % n


def join(*parts):
    return "|".join(p for p in parts if p not in ("", "AT*0"))


def recase(s, how):
    """0 as it is, 1 lower case, 2 every other character lower."""
    if how % 3 == 0:
        return s
    if how % 3 == 1:
        return s.lower()
    return "".join(c.lower() if i & 1 else c for i, c in enumerate(s))


def entries_from_oracle(st):
    """Per barcode [(entry, slice)], read off the oracle's trie over the reversed beginnings."""
    out = []
    for tree, slices in po.build_adapter_tree(st.adapter, st.barcodes):
        found = []

        def walk(node, path):
            if node[0] == "leaf":
                found.append((path[::-1], slices[node[1]]))
                return
            for code, child in enumerate(node[1]):
                if child is not None:
                    walk(child, path + "ACGT"[code])
        walk(tree, "")
        out.append(sorted(found))
    return out


def code(ch):
    return (ord(ch) >> 1) & 3


def group_sizes(entries):
    """td_set_splitter's grouping restated for one barcode: 64 groups by the codes (byte >> 1) & 3 of an entry's last
    three characters; an entry shorter than that sits in every group of the characters it has."""
    sizes = [0] * 64
    for g in range(64):
        for seq, _ in entries:
            if not seq:
                continue
            if code(seq[-1]) == g >> 4 and (len(seq) < 2 or code(seq[-2]) == (g >> 2) & 3) and (len(seq) < 3 or code(seq[-3]) == g & 3):
                sizes[g] += 1
    return sizes


def compact_form(st, entries):
    """What td_split_kernel_in_use must say under split_kernel 2 (five barcodes: the index fits beside the tile)."""
    ok = all(set(s) <= set("ACGT") for s in sites_of(st))
    for per in entries:
        ok = ok and max(group_sizes(per)) <= 8 and all(len(s) <= 128 and -128 <= sl <= 127 for s, sl in per)
    return ok


# ---------------------------------------------------------------------------------------------------- A: site search
def site_sweep(st, bc, which, ds, tail="AT"):
    """One read per end position: the site `which` behind d characters over {A, T}; case by d."""
    site = sites_of(st)[which]
    return [("A-sweep%d-%s" % (which, bc), join(recase(bc + st.cutsite, d // 3), at(d), recase(site, d), tail)) for d in ds]


def reads_A_hall():
    st = SETS["hall"]
    s0, s1 = sites_of(st)
    out = []
    for which in (0, 1):
        out += site_sweep(st, "TTGACC", which, range(0, 301))                    # start 11: windows at 0, 112, 224
        L = len(sites_of(st)[which])
        near = [d for d in range(0, 301) if (d + L) % STRIDE in (0, 1, 15, 16, 17, STRIDE - 1) or d < 3]   # (its last character at 16 + d + L)
        out += site_sweep(st, "GATTACAGGATC", which, near)                        # start 17: windows at 16, 128, 240
        for how in (0, 1, 2):                                                      # every case at the seams
            for e in (111, 112, 113, 126, 127, 128, 129, 223, 224, 239, 240, 241):
                d = e - 11 - L + 1
                out.append(("A-case%d" % which, join("TTGACCTGCAG", at(d), recase(sites_of(st)[which], how), "TA")))
    # both sites in one read: every ordered pair of end positions, near and far from the windows' seams
    ends = (40, 111, 114, 121, 127, 128, 133, 225, 241)
    for e0 in ends:
        for e1 in ends:
            a, b = e0 - len(s0) + 1, e1 - len(s1) + 1               # where they start
            if a == b or (a < b and a + len(s0) > b) or (b < a and b + len(s1) > a):
                continue
            first, second = ((a, s0), (b, s1)) if a < b else ((b, s1), (a, s0))
            out.append(("A-pair", join("TTGACCTGCAG", at(first[0] - 11), first[1], at(second[0] - first[0] - len(first[1])), second[1], "TT")))
    # near-misses that must not clip
    out.append(("A-miss-barcode-C", join("CCACTGCAG", at(30))))                   # ...C TGCAG spells CTGCAG across the cut
    out.append(("A-miss-barcode-C", join("CCACTGCAG", at(30), "CTGCAG", "AT")))   # (and a real one behind it)
    for site in (s0, s1):
        out.append(("A-miss-short", join("AACGTGCAG", at(20), site[:-1])))        # its last character missing at the read's end
        out.append(("A-miss-short", join("AACGTGCAG", at(120), site[:-1])))
        for k in range(1, len(site)):
            out.append(("A-miss-N", join("AACGTGCAG", at(20), site[:k] + "N" + site[k:], "AT")))
            out.append(("A-miss-N", join("AACGTGCAG", at(20), site[:k] + "N" + site[k + 1:], "AT")))
    # read lengths: around `start`, and 16 k - 1, 16 k, 16 k + 1 around 128 and 240
    for bc in ("AACG", "GATTACAGGATC"):
        head = bc + "TGCAG"
        start = len(head)
        out.append(("A-len", head[:-1]))
        out.append(("A-len", head))
        for site in (s0, s1):
            out.append(("A-len", head + site[:-1]))
            out.append(("A-len", head + site))
        base = 16 * (start >> 4)
        for n in (base + x for x in (127, 128, 129, 239, 240, 241)):
            out.append(("A-len", join(head, at(n - start))))
            for site in (s0, s1):
                out.append(("A-len", join(head, at(n - start - len(site)), site)))
                out.append(("A-len", join(head, at(n - start - len(site) + 1), site[:-1])))
    return out


def reads_A_prefix():
    out = []
    for d in (0, 1, 50, 100, 108, 111, 117, 122, 123, 124, 200):
        out.append(("A-tie", join("AACGTGCAG", at(d), "CCGGAT", "AT")))           # both sites at one position
        out.append(("A-tie", join("AACGTGCAG", at(d), "CCGGAA", "AT")))           # only the shorter one
        out.append(("A-tie", join("AACGTGCAG", at(d), "CCGGA")))                  # the longer one cut by the read's end
        out.append(("A-tie", join("AACGTGCAG", at(d), "ccggat")))
        out.append(("A-overlap", join("AACGTGCAG", at(d), "CCGGATCCGGAT", "A")))
        out.append(("A-overlap", join("AACGTGCAG", at(d), "CCCGGCCGGAT", "A")))
    return out


def reads_A_lens():
    st = SETS["lens"]
    s0, s1 = sites_of(st)
    assert len(s0) == 8 and len(s1) == 1 and s0[0] == st.cutsite[-1]
    out = []
    for bc in st.barcodes:
        head = bc + st.cutsite
        out.append(("A-before-start", join(head[:-1], s0, at(20))))               # the site starts one character before `start`
        out.append(("A-before-start", join(head[:-1], s0, at(20), s0, "A")))
        out.append(("A-len", head))
        out.append(("A-len", head + "G"))
        out.append(("A-len", head + s0[:-1].replace("G", "A")))
        for d in list(range(0, 20)) + list(range(96, 136)) + [215, 216, 217, 230, 231, 232, 233]:
            out.append(("A-eight", join(head, at(d), s0.replace("G", "g") if d & 1 else s0, "AT")))   # (its own G is the other site)
            out.append(("A-eight-alone", join(head, at(d), "CATCCTTC", "GATCC", "AT")))
            out.append(("A-one", join(head, at(d), recase("G", d), "AT")))
            out.append(("A-none", join(head, at(d))))
    return out


def reads_A_empty():
    out = []
    for bc in SETS["empty"].barcodes:
        head = bc + "TGCAG"
        out += [("A-empty", head[:-1]), ("A-empty", head), ("A-empty", head + "A"), ("A-empty", join(head, at(30))),
                ("A-empty", join(head, "CTGCAG", at(10))), ("A-empty", join(head, at(130), "CTGCAG", "A")), ("A-empty", join(head, at(7), "ACC"))]
    return out


# ---------------------------------------------------------------------------------------------------- B: adapter run-off
def prefix_sweep(st, bodies=(20, 0)):
    """Every beginning of both adapters, for every barcode, behind a body and directly behind the cut site."""
    out = []
    for bc in st.barcodes:
        for which, full in enumerate(fulls_of(st, bc)):
            for n in range(1, len(full) + 1):
                for body in bodies:
                    out.append(("B-prefix%d" % which, join(bc + st.cutsite, at(body), recase(full[:n], n + body))))
    return out


def reads_B_tiny():
    st = SETS["tiny"]
    out = prefix_sweep(st)
    for bc in st.barcodes:
        head = bc + st.cutsite
        f0, f1 = fulls_of(st, bc)
        for ent in (f0[:1], f0[:2], f1[:2]):
            out.append(("B-N", join(head, at(9), "N" + ent)))                     # no base right in front of a short entry
            out.append(("B-N", join(head, at(9), "NA" + ent)))
            out.append(("B-N", join(head, at(9), "N" + ent[:-1] + "n")))
            out.append(("B-N", join(head, at(9), "NT" + ent.lower())))
        for tail in ("NG", "NAG", "GN", "ANG", "NNG", "GNA", "NGA", "AN", "N"):
            out.append(("B-N", join(head, at(9), tail)))
            out.append(("B-N", head + tail))
    return out


PLANT_LENGTHS = (85, 88, 89, 92, 93, 100, 128)


def reads_B_long():
    st = SETS["long"]
    out = prefix_sweep(st, bodies=(20,))
    f0 = fulls_of(st, "AACG")[0]
    assert len(f0) == 128
    head = "AACGTGCAG"
    for E in PLANT_LENGTHS:
        for i in sorted(planted(E)):                                              # one mismatch at the entry's character i
            wrong = "ACGT"[("ACGT".index(f0[i]) + 1 + (i & 1)) & 3]
            out.append(("B-plant-%d" % E, join(head, at(11), f0[:i] + wrong + f0[i + 1:E])))
    # the read as long as the longest entry whose last characters it carries, and one character shorter
    for E in (100, 128):
        out.append(("B-tail", head + f0[len(head):E]))
        out.append(("B-tail", head + f0[len(head) + 1:E]))
        out.append(("B-tail", head + f0[:E]))
    return out


def planted(E):
    """The entry characters that carry a planted mismatch in reads_B_long, for entry length E."""
    return set(range(E)) if E in (85, 128) else set(range(0, E - 84)) | set(range(72, E))


def reads_B_echo():
    st = SETS["echo"]
    out = prefix_sweep(st)
    f0 = fulls_of(st, "AACG")[0]                                                  # CCGATACGTTGGACGTTCA
    long_, short_ = f0[:17], f0[:10]                                              # both end with ACGTT
    assert long_.endswith("ACGTT") and short_.endswith("ACGTT") and long_[-6] != short_[-6]
    for head in ("AACGTGCAG", "TTGACCTGCAG"):
        out.append(("B-echo-first", join(head, at(20), long_)))
        out.append(("B-echo-second", join(head, at(20), short_)))                 # the longer candidate fails, the shorter one matches
        out.append(("B-echo-second", join(head, at(21), "GG" + short_)))
        out.append(("B-echo-none", join(head, at(20), "GATACGTT")))               # both fail
        out.append(("B-echo-none", join(head, at(20), "CCGTTACGTT")))
        out.append(("B-echo-none", join(head, at(20), "ACGATACGTTGAACGTT")))
        out.append(("B-echo-second", join(head, at(20), f0[:9])))                 # ...ACGT: the same with four characters
        out.append(("B-echo-first", join(head, at(20), f0[:16])))
    return out


def reads_B_hall_extra():
    """A read that is exactly an entry's length past the cut site is in the sweep (body 0); one that is a character
    shorter than an entry whose end it carries:"""
    st = SETS["hall"]
    out = []
    for bc in st.barcodes:
        head = bc + st.cutsite
        for full in fulls_of(st, bc):
            for n in (len(head), len(head) + 1, len(head) + 2, 30):
                if n <= len(full):
                    out.append(("B-shorter", head + full[len(head):n]))           # as long as the entry full[:n]
                    out.append(("B-shorter", head + full[len(head) + 1:n]))       # one shorter
    return out


def reads_sites_and_ends(st):
    """For the sets that are not compact: the adapter sweep and a few sites."""
    s0, s1 = sites_of(st)
    out = prefix_sweep(st, bodies=(20,))
    for bc in st.barcodes:
        head = bc + st.cutsite
        for d in (0, 5, 110, 125):
            for site in (s0, s1, s0.lower(), s0.replace("N", "G"), s0.replace("N", "A")):
                out.append(("NC-site", join(head, at(d), site, "AT")))
    return out


# geometry reads (group C): a read of exactly n characters that ends with the beginning of the common adapter, so that a
# line end found one byte off changes the decision
def geo_read(n, bc="AACG"):
    head, tail = bc + "TGCAG", "CCGCTCAG"
    assert n >= len(head) + len(tail)
    return join(head, at(n - len(head) - len(tail)), tail)


GEO_LENGTHS = sorted(set([20, 24, 30, 33, 40, 60, 100] + list(range(440, 531)) + [24576 + 1000, 16384 + 1000]))


@functools.lru_cache(maxsize=None)
def edge_reads():
    """set -> [(group, spec)], duplicates removed (first mention kept)."""
    raw = collections.OrderedDict()
    raw["hall"] = (reads_A_hall() + prefix_sweep(SETS["hall"]) + reads_B_hall_extra()
                   + [("C-geometry", geo_read(n)) for n in GEO_LENGTHS] + [("C-geometry", geo_read(n, "CGT")) for n in (20, 33)]
                   + [("C-filler", s) for s in FILLER_READS])
    raw["prefix"] = reads_A_prefix() + prefix_sweep(SETS["prefix"])
    raw["lens"] = reads_A_lens() + prefix_sweep(SETS["lens"])
    raw["empty"] = reads_A_empty()
    raw["tiny"] = reads_B_tiny()
    raw["long"] = reads_B_long()
    raw["eight"] = prefix_sweep(SETS["eight"], bodies=(20,))
    raw["echo"] = reads_B_echo()
    for name in ("len129", "nine", "nsite"):
        raw[name] = reads_sites_and_ends(SETS[name])
    out = collections.OrderedDict()
    for name, reads in raw.items():
        seen, keep = set(), []
        for grp, spec in reads:
            if spec not in seen:
                seen.add(spec)
                keep.append((grp, spec))
        out[name] = keep
    return out


# reads of the filler records: five different decisions in a cycle that four does not divide, so that a decision
# written to a neighbouring slot shows
FILLER_READS = ["AACGTGCAG|AT*20", "TTGACCTGCAG|AT*8|CCGG|AT*4", "GGGG|AT*10", "CGTTGCAG|AT*12|CCGCTC", "CCACTGCAG|AT*6|CTGCAG|A"]


def oracle_decisions(st, seqs):
    """[(barcode index, findAdapterSeq value or None)] for stripped sequence texts, by the oracle's restatement."""
    barcut = po.combine_barcode_and_cutsite(st.barcodes, st.cutsite)
    tree = po.build_sequence_tree(barcut, len(barcut))
    trees = po.build_adapter_tree(st.adapter, st.barcodes)
    s0, s1 = sites_of(st)
    out = []
    for s in seqs:
        s = s.upper()
        bar = po.sequence_index_lookup(s, tree)
        out.append((bar, po.find_adapter_seq(s, trees[bar], s0, s1, len(st.barcodes[bar]) + len(st.cutsite)) if bar > -1 else None))
    return out


# ---------------------------------------------------------------------------------------------------- buffers
Case = collections.namedtuple("Case", "name set data labels error")     # error: None, or "nonascii" (the call must end in it)


MIN_RECORD = 88         # bytes: at most 4 * 6144 / 88 = 279 terminators in a wave quarter, so that no list overflows


def fastq_of(reads, newline=b"\n"):
    """One record per read, its header padded so that terminators stay sparse enough for k_split2's wave lists (a tile
    whose list overflows is walked in global memory: the reads would never meet the code they are built for)."""
    out = []
    for r in reads:
        pad = max(0, MIN_RECORD - len(r) - 3 - 4 * len(newline))
        out.append(b"@" + b"h" * pad + newline + r.encode("ascii") + newline + b"+" + newline + b"I" + newline)
    return b"".join(out)


def cold_tiles(data, T=24576):
    """The tiles of a buffer that k_split2 walks in global memory, by its rule restated: the first tile, a tile whose
    window of tile + halo does not lie inside the buffer, one with a byte >= 0x80 in that window, one with more
    terminators in a wave quarter than its list holds ("\r\n" is one terminator)."""
    Q = T // 4
    n = len(data)
    is_term = bytearray(n)
    for i, c in enumerate(data):
        if c == 0x0A or (c == 0x0D and data[i + 1:i + 2] != b"\n"):
            is_term[i] = 1
    cold = set()
    for t in range((n + T - 1) // T):
        lo = t * T
        if t == 0 or lo + T + HALO > n or any(c >= 0x80 for c in data[lo:lo + T + HALO]):
            cold.add(t)
        elif any(sum(is_term[lo + q * Q:lo + (q + 1) * Q]) > GEOM[T]["list"] for q in range(4)):
            cold.add(t)
    return cold


LEAD, TRAIL = 24576, 2 * 24576 + HALO      # header lines this long put the reads between them into k_split2's regular tiles


def read_case(name, setname, groups=None, newline=b"\n"):
    """The set's reads (of the groups named), one record each, between two records with very long header lines: k_split2
    walks the buffer's first tile and its last ones in global memory, and the reads are to meet its own code."""
    reads = [(g, expand(s)) for g, s in edge_reads()[setname] if groups is None or g.split("-")[0] in groups]
    assert reads, name
    filler = expand(FILLER_READS[0]).encode("ascii")
    lead = b"@" + b"h" * LEAD + newline + filler + newline + b"+" + newline + b"I" + newline
    trail = b"@" + b"h" * TRAIL + newline + filler + newline + b"+" + newline + b"I" + newline
    data = lead + fastq_of([r for _, r in reads], newline) + trail
    assert not cold_tiles(data) & set(range((len(lead) - 1) // 24576, (len(data) - len(trail)) // 24576 + 1)), name
    return Case(name, setname, data, ["lead"] + [g for g, _ in reads] + ["trail"], None)


def lines_of(data):
    return list(po.iter_lines(data))


def seq_line_count(data, first_line):
    """Sequence lines of a buffer whose first line has global index first_line; an unterminated last line counts."""
    return sum(1 for k in range(len(lines_of(data))) if (first_line + k) & 3 == 1)


def completed(data):
    """The buffer with its last record completed (so that the oracle's loop reaches the record's fourth line)."""
    out = data
    if out and out[-1:] not in (b"\n", b"\r"):
        out += b"\n"
    n = len(lines_of(out))
    while n & 3:
        out += b"+\n"
        n += 1
    return out


def ascii_twin(data):
    """The same text with every byte >= 0x80 replaced by a letter (for bytes in header lines, which decide nothing:
    the oracle rejects such lines itself)."""
    return bytes(c if c < 0x80 else 0x78 for c in data)


def expected(setname, data):
    """The oracle's decisions for every sequence line of the buffer, as the kernels report them."""
    return expected_for(SETS[setname], data)


def expected_for(st, data):
    """The same for any Set (tests/fused_cases.py: the ring inputs' barcodes with the Hall adapter)."""
    want = []
    po.barcode_splitter_bytes(completed(data), st.barcodes, st.cutsite, st.adapter, decisions=want)
    n = seq_line_count(data, 0)             # (a last record that ends within its header line was completed too)
    assert n <= len(want) <= n + 1
    return [(b, 999 if b < 0 else c) for b, c in want[:n]]


class Layout:
    """FASTQ bytes grown record by record, with filler records that bring a chosen byte to a chosen offset."""
    MINREC = len(b"@\n\n+\nI\n")

    def __init__(self):
        self.buf = bytearray()
        self.labels = []
        self.marks = {}          # label -> (offset of the sequence line, its raw length)
        self._nfill = 0

    def _filler(self, size):
        seq = expand(FILLER_READS[self._nfill % len(FILLER_READS)]).encode()
        self._nfill += 1
        pad = size - self.MINREC - len(seq)
        if pad < 0:                                              # no room for a read: an empty one
            seq, pad = b"", size - self.MINREC
        assert pad >= 0
        self.buf += b"@" + b"f" * pad + b"\n" + seq + b"\n+\nI\n"
        self.labels.append("filler")

    def fill_to(self, target):
        need = target - len(self.buf)
        assert need == 0 or need >= self.MINREC, (target, need)
        std = 120
        while need:
            size = std if need >= std + self.MINREC else need
            self._filler(size)
            need -= size
        assert len(self.buf) == target

    def record(self, label, seq, seq_start=None, seq_term=None, hdr_end=b"\n", seq_end=b"\n", header=b""):
        """A record whose sequence line (raw bytes `seq`, blanks included) starts at seq_start, or whose sequence line's
        terminator starts at seq_term; None: right here."""
        seq = seq if isinstance(seq, bytes) else seq.encode("ascii")
        if seq_term is not None:
            seq_start = seq_term - len(seq)
        if seq_start is None:
            seq_start = len(self.buf) + 1 + len(header) + len(hdr_end)
        gap = seq_start - len(hdr_end) - 1 - len(header) - len(self.buf)
        assert gap >= 0, (label, gap)
        pad = 0
        if gap < self.MINREC:
            pad = gap
        else:
            self.fill_to(len(self.buf) + gap)
        self.buf += b"@" + b"h" * pad + header + hdr_end
        assert len(self.buf) == seq_start
        self.marks[label] = (seq_start, len(seq))
        self.buf += seq + seq_end + b"+\nI\n"
        self.labels.append(label)

    def raw_lines(self, label, blob, nseq):
        """Bytes that are whole records already (nseq sequence lines)."""
        self.marks[label] = (len(self.buf), len(blob))
        self.buf += blob
        self.labels += [label] * nseq


def geo(n, bc="AACG"):
    return expand(geo_read(n, bc))


ENDS = ((b"\r\n", b"\n"), (b"\r", b"\n"), (b"\n", b"\r\n"), (b"\n", b"\r"))     # (header's terminator, sequence line's)
BLANKS = b" \t\x0b\x0c\x1c\x1d\x1e\x1f"
NTILES = 15
COLD = (0, 3, 5, 7, 8, 14)      # what k_split2 walks in global memory: first and last tile, flagged tiles


@functools.lru_cache(maxsize=None)
def geometry_case(T):
    """One buffer of 15 tiles of T bytes for the set "hall": every event of the tile geometry at a seam of its own, cold
    tiles between regular ones.  Seam k = offset k T, the end of tile k - 1, whose halo is [k T, k T + HALO).
    Events "crlf-<seam>-<w><sh>": terminator w of ENDS (0, 1: the header's "\r\n" / "\r"; 2, 3: the sequence line's)
    with its first byte at the seam - 1 (sh 0: a "\r\n" is split by it) or at the seam (sh 1)."""
    Q, S, H = GEOM[T]["quarter"], GEOM[T]["span"], HALO
    lay = Layout()
    events = []          # (offset it is laid at, function)

    def small(seam_name, seam, w, sh):
        hdr_end, seq_end = ENDS[w]
        label = "crlf-%s-%d%d" % (seam_name, w, sh)
        if w < 2:
            events.append((seam, lambda: lay.record(label, geo(24), seq_start=seam - 1 + sh + len(hdr_end), hdr_end=hdr_end)))
        else:
            events.append((seam, lambda: lay.record(label, geo(24), seq_term=seam - 1 + sh, seq_end=seq_end)))

    # tile 1 (regular): a 16-byte chunk's end that is no thread span's, then a thread span's end
    pos = T + 256
    for name, want in (("16", lambda x: x % S == 16), ("span", lambda x: x % S == 0 and x % Q != 0)):
        for w in range(4):
            for sh in (0, 1):
                pos += 130
                while not want(pos):
                    pos += 1
                small(name, pos, w, sh)
    # wave quarters' ends in regular tiles
    qseams = [T + Q, T + 2 * Q, T + 3 * Q, 2 * T + Q, 2 * T + 2 * Q, 2 * T + 3 * Q, 4 * T + Q, 4 * T + 2 * Q]
    for (w, sh), seam in zip([(w, sh) for w in range(4) for sh in (0, 1)], qseams):
        small("quarter", seam, w, sh)

    def seam_event(k, label, n, start=None, term=None, **kw):
        events.append((k * T - 1, lambda: lay.record(label, geo(n), seq_start=None if start is None else k * T + start,
                                                     seq_term=None if term is None else k * T + term, **kw)))

    seam_event(1, "term-crlf-split-T", 60, term=-1, seq_end=b"\r\n")
    seam_event(2, "start-T-1,term-H-2", H - 1, start=-1)
    seam_event(3, "start-T,term-H-1", H - 1, start=0)
    # 400 empty lines in the second quarter of tile 3: more terminators than a wave's list holds
    events.append((3 * T + Q + 160, lambda: (lay.fill_to(3 * T + Q + 160), lay.raw_lines("empty-lines", b"\n" * 400, 100))))
    seam_event(4, "term-cr-T-1", 60, term=-1, seq_end=b"\r")
    seam_event(5, "hdr-crlf-split,term-H", H - 1, start=1, hdr_end=b"\r\n")
    events.append((5 * T + 2 * Q + 333, lambda: lay.record("high-byte-in-tile", geo(30), seq_start=5 * T + 2 * Q + 333, header=b"\xe9t\xe9")))
    seam_event(6, "term-cr-T", 60, term=0, seq_end=b"\r")
    seam_event(7, "hdr-cr-T-1,term-H+1", H + 1, start=0, hdr_end=b"\r")
    events.append((8 * T - 1, lambda: lay.record("trailing-blanks-over-T", geo(33).encode() + BLANKS * 2, seq_term=8 * T + 7)))
    events.append((8 * T + 200, lambda: lay.record("high-byte-in-halo", geo(30), seq_start=8 * T + 200, header=b"caf\xc3\xa9")))
    seam_event(9, "start-T-1-short", 20, start=-1)

    def blanks_and_ends():     # every byte str.strip() takes off, at both ends of a line; empty and all-blank lines
        for i, c in enumerate(BLANKS):
            c = bytes([c])
            lay.record("blank-%02x-front" % c[0], c + geo(20 + i).encode())
            lay.record("blank-%02x-back" % c[0], geo(20 + i).encode() + c)
            lay.record("blank-%02x-both" % c[0], c + c + geo(20 + i).encode() + c)
        lay.record("empty-line", b"")
        lay.record("blank-line", b" ")
        lay.record("blank-line-all", BLANKS)
        lay.record("mixed-ends-a", geo(24), hdr_end=b"\r", seq_end=b"\r\n")        # CRLF, CR and LF in one buffer
        lay.record("mixed-ends-b", geo(24), hdr_end=b"\r\n", seq_end=b"\r")
    events.append((9 * T + 1000, blanks_and_ends))
    seam_event(10, "hdr-cr-T,term-crlf-split-H", H - 2, start=1, hdr_end=b"\r", seq_end=b"\r\n")
    events.append((11 * T - 1, lambda: lay.record("blanks-over-T", BLANKS[:5] + geo(40).encode() + BLANKS[5:], seq_start=11 * T - 3)))
    seam_event(11, "term-cr-H-1", 100, term=H - 1, seq_end=b"\r")
    seam_event(12, "long-read", T + 1000, start=-300)                              # tile 12 holds no line start
    seam_event(14, "term-cr-H", 100, term=H, seq_end=b"\r")
    events.sort(key=lambda e: e[0])
    for _, fn in events:
        fn()
    lay.fill_to(NTILES * T - 31)
    lay.record("last", geo(24, "CGT"))
    lay.buf[-1:] = b"\r"                                                           # "\r" as the buffer's last byte
    return lay, bytes(lay.buf)


def is_blank(c):
    return c in BLANKS


def geometry_checks(T):
    """The properties geometry_case(T) is named for, read from its bytes."""
    lay, data = geometry_case(T)
    H, Q, S = HALO, GEOM[T]["quarter"], GEOM[T]["span"]
    m = lay.marks
    assert len(data) == NTILES * T and NTILES >= 9 and data[-1] == 0x0D
    s, n = m["term-crlf-split-T"]
    assert data[T - 1] == 0x0D and data[T] == 0x0A and s + n == T - 1
    s, n = m["start-T-1,term-H-2"]
    assert s == 2 * T - 1 and data[s - 1] == 0x0A and s + n == 2 * T + H - 2 and data[s + n] == 0x0A
    s, n = m["start-T,term-H-1"]
    assert s == 3 * T and data[s - 1] == 0x0A and s + n == 3 * T + H - 1 and data[s + n] == 0x0A
    s, n = m["term-cr-T-1"]
    assert s + n == 4 * T - 1 and data[s + n] == 0x0D and data[s + n + 1] != 0x0A
    s, n = m["hdr-crlf-split,term-H"]
    assert data[5 * T - 1] == 0x0D and data[5 * T] == 0x0A and s == 5 * T + 1 and s + n == 5 * T + H and data[s + n] == 0x0A
    s, n = m["term-cr-T"]
    assert s + n == 6 * T and data[s + n] == 0x0D and data[s + n + 1] != 0x0A
    s, n = m["hdr-cr-T-1,term-H+1"]
    assert data[7 * T - 1] == 0x0D and s == 7 * T and s + n == 7 * T + H + 1 and data[s + n] == 0x0A
    s, n = m["trailing-blanks-over-T"]
    assert s + n == 8 * T + 7 and all(is_blank(c) for c in data[8 * T - 9:8 * T + 7]) and not is_blank(data[8 * T - 10])
    s, n = m["start-T-1-short"]
    assert s == 9 * T - 1 and data[s - 1] == 0x0A
    s, n = m["hdr-cr-T,term-crlf-split-H"]
    assert data[10 * T] == 0x0D and s == 10 * T + 1 and s + n == 10 * T + H - 1 and data[s + n:s + n + 2] == b"\r\n"
    s, n = m["blanks-over-T"]
    assert s == 11 * T - 3 and all(is_blank(c) for c in data[s:s + 5]) and not is_blank(data[s + 5])
    s, n = m["term-cr-H-1"]
    assert s >= 11 * T and s + n == 11 * T + H - 1 and data[s + n] == 0x0D and data[s + n + 1] != 0x0A
    s, n = m["long-read"]
    assert s < 12 * T and s + n > 13 * T and not any(c in b"\r\n" for c in data[12 * T - 1:13 * T])    # tile 12 holds no line start
    s, n = m["term-cr-H"]
    assert s >= 14 * T and s + n == 14 * T + H and data[s + n] == 0x0D and data[s + n + 1] != 0x0A
    # a wave quarter with more terminators than its list holds (384)
    lo = 3 * T + Q
    assert sum(1 for c in data[lo:lo + Q] if c in b"\r\n") >= 385
    # bytes >= 0x80: in tile 5 behind tile 4's halo, and in tile 7's halo (so in tile 8); all of them in header lines
    high = [i for i, c in enumerate(data) if c >= 0x80]
    assert high and all(5 * T + H <= i < 6 * T or 8 * T <= i < 8 * T + H for i in high)
    assert any(i < 6 * T for i in high) and any(i >= 8 * T for i in high)
    for idx, line in enumerate(po.iter_lines(data)):
        assert idx & 3 == 0 or not any(c >= 0x80 for c in line)
    # no other tile has a quarter with more than 384 terminators
    for t in range(NTILES):
        for q in range(4):
            if (t, q) != (3, 1):
                assert sum(1 for c in data[t * T + q * Q:t * T + (q + 1) * Q] if c in b"\r\n") <= 384
    # one workgroup that takes every tile meets cold after regular and regular after cold; every t & 3 among the regular
    regular = [t for t in range(NTILES) if t not in COLD]
    assert {t & 3 for t in regular} == {0, 1, 2, 3}
    assert any(t - 1 in COLD for t in regular) and any(t + 1 in COLD for t in regular)
    # the events of the halo lie behind regular tiles
    for k in (2, 3, 5, 7, 10, 11, 12, 14):
        assert k - 1 in regular
    # CRLF at the small seams: every event where it was meant to be
    for name, (s, n) in m.items():
        if not name.startswith("crlf-"):
            continue
        _, which, ws = name.split("-")
        step = {"16": 16, "span": S, "quarter": Q}[which]
        w, sh = int(ws[0]), int(ws[1])
        term = ENDS[w][0] if w < 2 else ENDS[w][1]
        tb = s - len(term) if w < 2 else s + n                   # first byte of the terminator in question
        assert (tb + 1 - sh) % step == 0 and (which != "16" or (tb + 1 - sh) % S != 0), name
        assert data[tb:tb + len(term)] == term and (len(term) == 2 or data[tb + 1] != 0x0A), name
        assert (tb // T) in regular, name
    assert {n for n in m if n.startswith("crlf-")} == {"crlf-%s-%d%d" % (a, w, sh) for a in ("16", "span", "quarter")
                                                      for w in range(4) for sh in (0, 1)}
    # every blank at both ends of a line
    for c in BLANKS:
        s, n = m["blank-%02x-front" % c]
        assert data[s] == c and not is_blank(data[s + 1])
        s, n = m["blank-%02x-back" % c]
        assert data[s + n - 1] == c and data[s + n] == 0x0A
    return True


def nonascii_case(T):
    """Three tiles with one byte >= 0x80 in a SEQUENCE line of the middle tile: the call must end in TD_E_NONASCII."""
    lay = Layout()
    seq = bytearray(geo(40).encode())
    seq[17] = 0xE9
    lay.record("high-byte-in-sequence", bytes(seq), seq_start=T + 5000)
    lay.fill_to(3 * T)
    return Case("nonascii-%d" % T, "hall", bytes(lay.buf), list(lay.labels), "nonascii")


SMALL = b"@\nAACGTGCAGATATCCGC\n+\nI\n"       # cut after 1, 15, 16 and 17 bytes: inside its sequence line


@functools.lru_cache(maxsize=None)
def cases():
    """Every buffer the GPU module runs, by name."""
    out = collections.OrderedDict()

    def add(c):
        assert c.name not in out
        out[c.name] = c
    add(read_case("hall-A", "hall", groups=("A",)))
    add(read_case("hall-B", "hall", groups=("B",)))
    add(read_case("hall-B-crlf", "hall", groups=("B",), newline=b"\r\n"))
    for name in SETS:
        if name != "hall":
            add(read_case(name, name))
    for T in GEOM:
        lay, data = geometry_case(T)
        add(Case("geometry-%d" % T, "hall", data, list(lay.labels), None))
        for what, n in (("tile", T), ("tile+halo-1", T + HALO - 1), ("tile+halo", T + HALO), ("two-tiles-less-1", 2 * T - 1), ("two-tiles", 2 * T)):
            add(Case("length-%s-%d" % (what, T), "hall", data[:n], None, None))
        add(nonascii_case(T))
    for n in (1, 15, 16, 17):
        add(Case("length-%d" % n, "hall", SMALL[:n], None, None))
    # a buffer that ends inside a 32-bit word, behind a last line of a few bytes that has no terminator: every
    # residue of the length, in a buffer of one tile and in the second tile of two
    for T in GEOM:
        for base, tails in ((1000, (b"A", b"AA", b"AAC", b"AACGTGCAGATCCGC")), (T + 1000, (b"A",))):
            for k in range(4):
                for tail in tails:
                    lay = Layout()
                    lay.fill_to(base + k)
                    lay.buf += b"@\n" + tail
                    lay.labels.append("tail")
                    add(Case("tail-%d-%d-%d" % (base + k, len(tail), T), "hall", bytes(lay.buf), list(lay.labels), None))
    return out


def self_checks():
    """Every read case has the property it is named for."""
    reads = edge_reads()
    ents = {name: entries_from_oracle(st) for name, st in SETS.items()}
    for name, st in SETS.items():
        assert compact_form(st, ents[name]) == st.compact, name
    # A: one read per end position of each site over three search windows and both seams, for start 11 (windows from 0)
    st = SETS["hall"]
    for which, site in enumerate(sites_of(st)):
        ends = set()
        for g, spec in reads["hall"]:
            if g == "A-sweep%d-TTGACC" % which:
                text = expand(spec).upper()
                assert set(text[11:].replace(site, "", 1)) <= set("AT") and text[11:].count(site) == 1
                ends.add(text.find(site, 11) + len(site) - 1)
        start = 11
        assert ends == set(range(start + len(site) - 1, start + len(site) + 300)), which
        base = 16 * (start >> 4)
        for k in (0, 1):                                        # the window's last position, and the first one it does not see
            assert base + STRIDE * k + WINDOW - 1 in ends and base + STRIDE * k + WINDOW in ends
        # a site that straddles the stride: starts before 112 k, ends at or behind it
        assert all(any(e - len(site) + 1 < base + STRIDE * k <= e for e in ends) for k in (1, 2))
        ends17 = {expand(s).upper().find(site, 17) + len(site) - 1 for g, s in reads["hall"] if g == "A-sweep%d-GATTACAGGATC" % which}
        assert {16 + WINDOW - 1, 16 + WINDOW, 16 + STRIDE + WINDOW - 1, 16 + STRIDE + WINDOW} <= ends17
    cased = [expand(s) for g, s in reads["hall"] if g.startswith("A-case")]
    assert any("ccgg" in r for r in cased) and any("CcGg" in r for r in cased) and any("CCGG" in r for r in cased)
    # near-misses: the text spells a site that begins before `start`
    assert "CTGCAG" in "CCAC" + "TGCAG" and "CCAC" in st.barcodes
    s0 = sites_of(SETS["lens"])[0]
    assert any(expand(s).find(s0) == len(bc) + 4 for g, s in reads["lens"] if g == "A-before-start" for bc in SETS["lens"].barcodes[:1])
    a, b = sites_of(SETS["prefix"])
    assert b.startswith(a) and a != b
    assert sites_of(SETS["empty"])[0] == ""
    # B: the compact form at its limits, and just beyond them
    lens = lambda name: {len(s) for per in ents[name] for s, _ in per}
    assert max(lens("long")) == 128 and set(range(85, 129)) <= lens("long")
    assert max(lens("len129")) == 129
    assert max(max(group_sizes(per)) for per in ents["eight"]) == 8
    assert max(max(group_sizes(per)) for per in ents["nine"]) == 9
    assert not set(sites_of(SETS["nsite"])[0]) <= set("ACGT")
    assert {1, 2} <= lens("tiny")
    # the planted mismatches: every character of an entry that only the overflow loop compares (REGS .. E - 5), its
    # 8-byte steps and its last partial word among them; and every character 84 places and more from the read's end
    for E in PLANT_LENGTHS:
        got = planted(E)
        assert set(range(REGS, E - 4)) <= got and set(range(0, E - 84)) <= got, E
        assert {REGS, REGS + 7, REGS + 8} & set(range(REGS, E - 4)) <= got
    assert any((E - 4 - REGS) % 8 for E in PLANT_LENGTHS) and any(E - 4 - REGS > 8 for E in PLANT_LENGTHS)
    f0 = fulls_of(SETS["long"], "AACG")[0]
    for g, spec in reads["long"]:
        if g.startswith("B-plant-"):
            E = int(g.split("-")[2])
            tail = expand(spec)[-E:]
            assert sum(1 for x, y in zip(tail, f0[:E]) if x != y) == 1
    # two entries of one group that share their last four characters
    per = ents["echo"][0]
    assert any(x != y and x[-4:] == y[-4:] for x, _ in per for y, _ in per if len(x) > 4 and len(y) > 4)
    # C
    # (read_case asserts that the read cases' reads lie in tiles that k_split2 takes as regular ones)
    assert cold_tiles(geometry_case(24576)[1]) == set(COLD)
    tails = [c for n, c in cases().items() if n.startswith("tail-")]
    assert {(len(c.data) & 3, len(lines_of(c.data)[-1])) for c in tails} >= {(r, n) for r in range(4) for n in (1, 2, 3)}
    assert all(c.data[-1:] not in (b"\n", b"\r") and len(lines_of(c.data)) & 3 == 2 for c in tails)
    for T in GEOM:
        geometry_checks(T)
        c = nonascii_case(T)
        bad = [i for i, ch in enumerate(c.data) if ch >= 0x80]
        assert len(bad) == 1 and T <= bad[0] < 2 * T
        assert [k & 3 for k, line in enumerate(po.iter_lines(c.data)) if any(ch >= 0x80 for ch in line)] == [1]
    return True
