"""Host-side mirror of the reference's tagdigger_fun module for the counting path.

`find_tags_fastq` has the reference's signature, defaults, return type and
exceptions (tagdigger_fun.py:192-277) but its record loop runs on an MI355X.
Of the primitives under it, `enumerate_cut_sites` and `combine_barcode_and_cutsite`
(reference :136-190, :60-69) are exported under their reference names.  The
reference's nested-list trees (`build_sequence_tree` / `sequence_index_lookup`,
:71-134) have no counterpart here: their rules live in the flat device index that
`Engine.set_index` builds (csrc/tagdig.hip, td_set_index) and in the matching
kernels; a restatement of the two functions exists only as test infrastructure
(the CPU checker beside the tests).
"""
from .engine import (Engine, default_engine, enumerate_cut_sites,  # noqa: F401
                     combine_barcode_and_cutsite, effective_maxreads, census_index)

# restriction enzyme cut sites as they appear after the barcode (reference tagdigger_fun.py:19-20)
enzymes = {'ApeKI': 'CWGC', 'EcoT22I': 'TGCAT', 'NcoI': 'CATGG',
           'NsiI': 'TGCAT', 'PstI': 'TGCAG', 'SbfI': 'TGCAGG', 'None': ''}


def find_tags_fastq(fqfile, barcodes, tags, cutsite="TGCAG", maxreads=5e9, tassel_tagcount=False,
                    device=0, as_array=False, progress=True):
    """Count barcode x tag combinations in one FASTQ file (plain or .gz by name).

    Returns list[list[int]] shaped [len(barcodes)][len(tags)], rows and columns
    in the order given -- exactly what the reference returns (tagdigger_fun.py
    :237,:277) -- and prints the reference's progress lines (:268-271: the three
    counters after every 50 000 reads, the file name after every 1 000 000; the
    numbers are kept on the device per window of reads and printed once the file
    is through; `progress=False` leaves them out).  Differences, all documented
    in DESIGN.md: a sequence line holding a byte >= 0x80 raises NonAsciiSequence; an index
    whose first sequence is empty raises IndexError at build time (the
    reference raises at its first lookup).
    """
    eng = default_engine(device)
    eng.set_index(barcodes, tags, cutsite)          # asserts + index, before the file is opened (:198-233)
    eng.set_option("progress", 1 if progress else 0)
    eng.count_file(fqfile, maxreads, tassel_tagcount)
    if progress:
        for line in eng.progress_lines(fqfile):
            print(line)
    if as_array:                                    # (this build only: the matrix as a numpy array, no Python lists)
        return eng.counts_numpy(signed=bool(tassel_tagcount))
    return eng.counts(signed=bool(tassel_tagcount))


def find_tags_fastq_many(files, barcodes, tags, cutsite="TGCAG", maxreads=5e9, tassel_tagcount=False,
                         devices=(0,)):
    """`find_tags_fastq` over several files, the files dealt out to the GPUs in `devices` and counted
    concurrently (one host thread and one engine per GPU; the library calls release the GIL).

    `barcodes` is either one list used for every file or a list of lists, one per file -- the way
    the reference's callers loop `find_tags_fastq(f, bckeys[f][0], tags[1], cutsite=...)` over the
    files of a key file (tagdigger_script.py:124-126).  Returns the matrices in the order of `files`;
    each equals the single-file call's.  An exception in any file is raised after the others finish.
    (Several processes instead of threads, with an all-reduce into sample rows: tagdigger_amd.multi.)
    """
    import threading
    files = list(files)
    per_file = bool(barcodes) and isinstance(barcodes[0], (list, tuple))
    if per_file and len(barcodes) != len(files):
        raise ValueError("one barcode list per file expected")
    devs = list(dict.fromkeys(int(d) for d in devices))
    if not devs:
        raise ValueError("no device given")
    results, errors = [None] * len(files), [None] * len(files)
    todo = list(range(len(files)))
    lock = threading.Lock()

    def work(dev):
        while True:
            with lock:
                if not todo:
                    return
                k = todo.pop(0)
            try:
                results[k] = find_tags_fastq(files[k], barcodes[k] if per_file else barcodes, tags, cutsite=cutsite,
                                             maxreads=maxreads, tassel_tagcount=tassel_tagcount, device=dev,
                                             progress=False)        # (several files at once: no interleaved prints)
            except BaseException as exc:      # noqa: BLE001 -- reported to the caller below
                errors[k] = exc
    threads = [threading.Thread(target=work, args=(d,)) for d in devs[1:]]
    for t in threads:
        t.start()
    work(devs[0])
    for t in threads:
        t.join()
    for exc in errors:
        if exc is not None:
            raise exc
    return results


class CensusResult(list):
    """What tag_census returns: [seqs, counts] (or [seqs, counts, names]) with the statistics in `.stats`."""
    stats = None


CENSUS_MIN_SLOTS = 1024
CENSUS_DEFAULT_SLOTS = 1 << 22
CENSUS_MAX_TABLE_BYTES = 16 << 30


def _census_host_index(barcodes, cutsite):
    """The barcode + cut site index of find_tags_fastq (reference tagdigger_fun.py:209-219) as a dict of the
    sequences its tree keeps -> barcode row, with the tree's failures (what td_set_index reports)."""
    barcut, barnum, _ = census_index(barcodes, cutsite)
    if not barcut:
        raise IndexError("list index out of range")
    if barnum == 1 and barcut == [""]:                 # (:109-110: a lone empty sequence matches every base)
        return {b: 0 for b in "ACGT"}
    if barcut[0] == "":
        raise IndexError("string index out of range")
    try:
        kept = _trie_survivors(barcut)
    except AssertionError as exc:
        pos = int(str(exc).split(":")[1].split(".")[0])
        raise AssertionError("Problematic sequence: {}.  Likely due to overlapping tags.".format(pos % barnum)) from None
    return {seq: pos % barnum for seq, pos in kept}


def _census_host(fqfile, barcodes, cutsite, taglen, maxreads):
    """The census rule read by read over a dict: (window -> count, statistics)."""
    from ._binding import NonAsciiSequence
    index = _census_host_index(barcodes, cutsite)
    lengths = sorted({len(s) for s in index})
    bound = effective_maxreads(maxreads)
    census = {}
    st = dict.fromkeys(("reads", "barcut", "short", "ambiguous"), 0)
    opener = _gzip.open if fqfile[-2:].lower() == 'gz' else open
    with opener(fqfile, 'rt', encoding='latin-1') as fh:
        for k, line in enumerate(fh):
            if k % 4 != 1:
                continue
            st["reads"] += 1
            if any(ch >= '\x80' for ch in line):
                raise NonAsciiSequence("non-ASCII byte in a sequence line")
            line1 = line.strip().upper()
            b = -1
            for n in lengths:
                if line1[:n] in index and len(line1) >= n:
                    b = index[line1[:n]]
                    break
            if b != -1:
                st["barcut"] += 1
                w = line1[len(barcodes[b]):len(barcodes[b]) + taglen]
                if len(w) < taglen:
                    st["short"] += 1
                elif not set(w) <= _ACGT:
                    st["ambiguous"] += 1
                else:
                    census[w] = census.get(w, 0) + 1
            if st["reads"] >= bound:
                break
    st["counted"] = st["barcut"] - st["short"] - st["ambiguous"]
    st["distinct"] = len(census)
    return census, st


def _census_known_names(seqs, known, cutsite):
    """Names of the known tags each window belongs to, joined by ';' ('' when unknown).  The strip decision is
    find_tags_fastq's (reference :222-231): tags that all begin with a cut-site variant are compared with the window,
    others with the window behind the cut site; a tag matches when it is a prefix of that string or that string a
    prefix of it.  On the host over the fetched entries: a bisect for the tags a window begins, one dict lookup per
    distinct tag length for the tags that begin a window."""
    names, tags = known[0], [t.upper() for t in known[1]]
    cutsite = cutsite.upper()
    cutlen = len(cutsite)
    skip = 0 if set(t[:cutlen] for t in tags).issubset(set(enumerate_cut_sites(cutsite))) else cutlen
    order = sorted(range(len(tags)), key=lambda i: tags[i])
    sorted_tags = [tags[i] for i in order]
    by_seq = {}
    for i, t in enumerate(tags):
        by_seq.setdefault(t, []).append(i)
    lengths = sorted({len(t) for t in tags})
    out = []
    for w in seqs:
        s = w[skip:]
        lo = _bisect.bisect_left(sorted_tags, s)
        hi = _bisect.bisect_left(sorted_tags, s + '\x7f')
        hits = [order[k] for k in range(lo, hi)]                   # tags that begin with s (s itself among them)
        for n in lengths:
            if n >= len(s):
                break
            hits.extend(by_seq.get(s[:n], ()))                     # tags that s begins with
        out.append(";".join(names[i] for i in sorted(hits)))
    return out


def tag_census(fqfile, barcodes, cutsite="TGCAG", taglen=64, maxreads=5e9, min_count=1, top=None, known=None,
               device=0, backend="gpu", slots=0, max_table_bytes=CENSUS_MAX_TABLE_BYTES):
    """The distinct sequences that follow the barcodes of one library (plain or .gz by name), and how often each occurs.

    For every read with a barcode + cut site -- find_tags_fastq's rule up to there -- the window of `taglen` bases
    (1..64) that starts on the cut site's first base is counted; a read too short for it counts as `short`, a window
    with anything but ACGT as `ambiguous`.  Returns [seqs, counts] of the windows seen at least `min_count` times,
    by count descending, then sequence ascending; `top=N` keeps the first N.  With `known=[names, seqs]` (what the
    readTags_* functions return) a third list holds, per window, the names of the known tags it belongs to joined
    by ';' ('' for an unknown one).  The statistics (reads, barcut, short, ambiguous, counted, distinct) are the
    result's `.stats`.

    backend="gpu": the table is filled on the device (csrc/census.hip).  A table that fills up is begun again with
    four times the slots (from `slots`, default 2^22) and the file recounted, as long as the table stays within
    `max_table_bytes` (default 16 GiB); beyond that the TD_E_LIMIT is raised.  backend="host": a dict over the same
    rule.  Not done here: tassel_tagcount weights, per-sample rows, several GPUs.  Grouping the tags into
    markers: tag_network and census_markers."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    taglen = int(taglen)
    if not 1 <= taglen <= 64:
        raise ValueError("taglen must be 1..64")
    min_count = max(1, int(min_count))
    if backend == "host":
        census, stats = _census_host(fqfile, barcodes, cutsite, taglen, maxreads)
        entries = sorted(((s, c) for s, c in census.items() if c >= min_count), key=lambda e: (-e[1], e[0]))
        if top is not None:
            entries = entries[:max(0, int(top))]
        seqs, counts = [e[0] for e in entries], [e[1] for e in entries]
    else:
        from ._binding import TagdigError
        eng = default_engine(device)
        slots = int(slots) or CENSUS_DEFAULT_SLOTS
        try:
            while True:
                eng.census_begin(barcodes, cutsite, taglen, slots)
                try:
                    eng.census_file(fqfile, maxreads)
                    break
                except TagdigError as exc:
                    if exc.code != -7 or not exc.detail.startswith("census table full"):
                        raise
                    slots *= 4
                    if slots * (32 if taglen > 32 else 16) > max_table_bytes:
                        raise
            stats = eng.census_stats()
            seqs, counts = eng.census_fetch(min_count, top)
        except BaseException:
            try:
                eng.census_end()
            except Exception:      # noqa: BLE001 -- the error that brought us here is the one to report
                pass
            raise
        eng.census_end()
    out = CensusResult([seqs, counts])
    if known is not None:
        out.append(_census_known_names(seqs, known, cutsite))
    out.stats = {k: stats[k] for k in ("reads", "barcut", "short", "ambiguous", "counted", "distinct")}
    return out


class NetworkResult:
    """What tag_network returns: `.pairs` and `.edges` (the kept edges) as lists of (i, j), i < j, ascending; `.degree`,
    the kept edges at every tag; `.stats`: tags, edges, kept, deg0, deg1, hubs, pairs, compares, backend."""

    def __init__(self, pairs, edges, degree, stats):
        self.pairs, self.edges, self.degree, self.stats = pairs, edges, degree, stats


def _ratio_ppm(min_ratio):
    if not 0 <= min_ratio <= 1:
        raise ValueError("min_ratio must lie in [0, 1]")
    return int(round(min_ratio * 1e6))


def _network_input(seqs, counts):
    """The tags upper-cased and checked against the rule's input: one length (1..64), ACGT, pairwise distinct."""
    seqs = [s.upper() for s in seqs]
    counts = [int(c) for c in counts]
    if len(seqs) != len(counts):
        raise ValueError("seqs and counts differ in length")
    L = len(seqs[0]) if seqs else 0
    if any(len(s) != L for s in seqs):
        raise ValueError("tags of unequal length")
    if seqs and not 1 <= L <= 64:
        raise ValueError("tags must have 1..64 bases")
    if not set("".join(seqs)) <= _ACGT:
        raise ValueError("non-ACGT character in tag {}".format(next(i for i, s in enumerate(seqs) if not set(s) <= _ACGT)))
    seen = {}
    for i, s in enumerate(seqs):
        if seen.setdefault(s, i) != i:
            raise ValueError("tag {} equals tag {}".format(i, seen[s]))
    return seqs, counts, L


def _network_host(seqs, counts, L, ppm):
    """The rule of DESIGN 4.13 over a dict: for every tag, every position and each of the three other bases, one
    lookup -- 3 L n of them, no comparing of tag with tag."""
    where = {s: i for i, s in enumerate(seqs)}
    edges, kept = 0, []
    others = {b: "ACGT".replace(b, "") for b in "ACGT"}
    for i, s in enumerate(seqs):
        for k in range(L):
            head, tail = s[:k], s[k + 1:]
            for base in others[s[k]]:
                j = where.get(head + base + tail)
                if j is None or j < i:
                    continue
                edges += 1
                minor, major = min(counts[i], counts[j]), max(counts[i], counts[j])
                if minor * 1000000 >= ppm * major:
                    kept.append((i, j))
    kept.sort()
    degree = [0] * len(seqs)
    for i, j in kept:
        degree[i] += 1
        degree[j] += 1
    pairs = [(i, j) for i, j in kept if degree[i] == 1 and degree[j] == 1]
    stats = dict(tags=len(seqs), edges=edges, kept=len(kept), deg0=degree.count(0), deg1=degree.count(1),
                 hubs=sum(1 for d in degree if d >= 2), pairs=len(pairs), compares=0, backend="host")
    return NetworkResult(pairs, kept, degree, stats)


def tag_network(seqs, counts, min_ratio=0.03, device=0, backend="gpu"):
    """The one-mismatch network of a census and its reciprocal pairs (the UNEAK network filter).

    seqs: n distinct ACGT tags of one length (1..64; lower case is upper-cased), counts their counts.  An edge joins two
    tags that differ at exactly one position; it is kept when minor * 1 000 000 >= round(min_ratio * 1e6) * major, in
    integers (min_ratio in [0, 1]; the default is UNEAK's error tolerance rate); a pair is a kept edge whose two ends
    have no other kept edge.  Returns a NetworkResult.

    backend="gpu": the self-join runs on the device (csrc/tagnet.hip).  Its comparing is quadratic in the longest run of
    tags that share a half; an input whose `compares` exceed the device's cap is answered by the host restatement
    instead, and `.stats["backend"]` says which of the two it was.  backend="host": the dict restatement.
    ValueError: unequal lengths, a character outside ACGT, a duplicate, min_ratio outside [0, 1].
    Not done here: indels, distance 2, tags of more than 64 bases, several GPUs, per-sample filters."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    ppm = _ratio_ppm(min_ratio)
    seqs, counts, L = _network_input(seqs, counts)
    if backend == "host" or not seqs:
        res = _network_host(seqs, counts, L, ppm)
        if backend == "gpu":
            res.stats["backend"] = "gpu"          # (nothing to send to the device)
        return res
    from ._binding import TagdigError
    eng = default_engine(device)
    try:
        net = eng.tagnet_build("".join(seqs).encode("ascii"), counts, L, ppm)
    except TagdigError as exc:
        if exc.code != -7 or not exc.detail.startswith("tag network: compares"):
            raise
        return _network_host(seqs, counts, L, ppm)
    try:
        pairs = [(int(i), int(j)) for i, j in eng.tagnet_pairs(net)[0]]
        edges = [(int(i), int(j)) for i, j in eng.tagnet_edges(net, kept_only=True)[0]]
        degree = [int(d) for d in eng.tagnet_degrees(net)]
        stats = dict(net.stats, backend="gpu")
    finally:
        net.close()
    return NetworkResult(pairs, edges, degree, stats)


def census_markers(seqs, counts, min_ratio=0.03, prefix="Mrkr", numdig=7, start=1, device=0, backend="gpu"):
    """[marker names, merged strings, pair counts] of the reciprocal pairs of a census (tag_network's `.pairs`, in
    their order).  Marker k is named prefix + zero-padded (start + k), as consolidateTagSets names new markers; its
    merged string is mergeTags([major, minor]) with the major allele the tag of the lower index -- in a census the
    commoner one, the alphabetically first on a tie -- and paircounts[k] = (count of the major, count of the minor).
    The first two lists are what mergedTagList returns: they go straight into writeMarkerDatabase and exportFasta2.
    `.stats` holds tag_network's statistics."""
    if '_' in prefix:
        raise ValueError("marker names cannot contain underscores: prefix {!r}".format(prefix))
    net = tag_network(seqs, counts, min_ratio=min_ratio, device=device, backend=backend)
    seqs = [s.upper() for s in seqs]
    names, merged, paircounts = [], [], []
    for k, (i, j) in enumerate(net.pairs):
        names.append("{}{:0{width}}".format(prefix, start + k, width=numdig))
        merged.append(mergeTags([seqs[i], seqs[j]]))
        paircounts.append((int(counts[i]), int(counts[j])))
    out = CensusResult([names, merged, paircounts])
    out.stats = net.stats
    return out


# ------------------------------------------------------------------ tag placement (csrc/place.hip)
PLACE_NONE = 255                      # dist of a tag without a locus within k
PLACE_NO_LOCUS = 0xFFFFFFFFFFFFFFFF   # its locus


class CutSites:
    """What genome_cut_sites returns: the in-silico digest of a genome.  `.names` and `.rec_start` (R + 1 offsets into
    the framed genome) describe the records; `.x`, `.rec`, `.strand` (0 forward, 1 reverse) the loci in id order;
    `.pos1` their SAM positions and `.cutpos` their cut positions; `.windows()` their windows; `.stats`: loci, forward,
    reverse, distinct, dropped_bounds, dropped_alphabet, records, backend.  With backend "gpu" the digest stays on the
    device until close(), so that several tag sets can be placed against it."""

    def __init__(self, names, rec_start, remnants, taglen, x, rec, strand, stats, place=None, windows=None):
        import numpy as np
        self.names, self.rec_start, self.remnants, self.taglen = list(names), [int(v) for v in rec_start], list(remnants), taglen
        self.x = np.asarray(x, dtype=np.int64)
        self.rec = np.asarray(rec, dtype=np.int64)
        self.strand = np.asarray(strand, dtype=np.int64)
        self.stats, self._place, self._windows, self._distinct = stats, place, windows, None
        starts = np.asarray(self.rec_start, dtype=np.int64)
        self.pos1 = self.x - starts[self.rec] + 1 if len(self.x) else self.x
        self.cutpos = self.pos1 + (taglen - 1) * self.strand

    @property
    def records(self):
        """[(name, length)] in genome order"""
        return [(nm, self.rec_start[r + 1] - self.rec_start[r]) for r, nm in enumerate(self.names)]

    def windows(self):
        if self._windows is None:
            self._windows = self._place._eng.place_loci(self._place, windows=True)[3] if len(self.x) else []
        return self._windows

    def distinct(self):
        """{window: [loci that have it, the smallest of their ids]}"""
        if self._distinct is None:
            d = {}
            for i, w in enumerate(self.windows()):
                e = d.get(w)
                if e is None:
                    d[w] = [1, i]
                else:
                    e[0] += 1
            self._distinct = d
        return self._distinct

    def close(self):
        if self._place is not None:
            self._place.close()
            self._place = None


def _place_remnants(cutsite, taglen):
    taglen = int(taglen)
    if not 1 <= taglen <= 64:
        raise ValueError("taglen must be 1..64")
    cutsite = cutsite.upper()
    if cutsite == "":
        raise ValueError("tags cannot be placed without a cut site: the loci are the genome's cut sites")
    if not set(cutsite) <= set('ACGTNRYKMSWBDHV'):
        raise ValueError("invalid cut site {!r}".format(cutsite))
    remnants = enumerate_cut_sites(cutsite)
    if len(remnants) > 16:
        raise ValueError("the cut site {} stands for {} sequences; at most 16 are taken".format(cutsite, len(remnants)))
    if len(cutsite) > taglen:
        raise ValueError("the cut site is longer than the tags")
    return remnants, taglen


def _place_records(genome, nbytes):
    """SAM names and record bounds from the headers a genome reader recorded (exp_frag_size's HostGenome / DeviceGenome)."""
    events = []
    for evs, exc in genome.files:
        events.extend(evs)
        if exc is not None:
            raise exc
    if nbytes and (not events or events[0][1] > 0):
        raise ValueError("the genome holds sequence before its first header line: a record without a name")
    names = [(nm.split() or [""])[0] for nm, _ in events]
    seen = set()
    for nm in names:
        if nm == "":
            raise ValueError("a genome record has an empty name")
        if nm in seen:
            raise ValueError("the record name {} occurs twice in the genome".format(nm))
        seen.add(nm)
    return names, [off for _, off in events] + [nbytes]


def _find_all(text, pat):
    k = text.find(pat)
    while k != -1:
        yield k
        k = text.find(pat, k + 1)


def _sites_host(text, rec_start, remnants, L):
    """The digest rule of DESIGN 4.20 on a str: (x, rec, strand, windows, stats) in locus order."""
    cand = set()
    for c in remnants:
        cand.update((x, 0) for x in _find_all(text, c))
        cand.update((y + len(c) - L, 1) for y in _find_all(text, reverseComplement(c)))
    xs, recs, strands, wins = [], [], [], []
    stats = dict(loci=0, forward=0, reverse=0, distinct=0, dropped_bounds=0, dropped_alphabet=0, records=len(rec_start) - 1)
    for x, strand in sorted(cand):
        if x < 0:
            stats["dropped_bounds"] += 1
            continue
        r = _bisect.bisect_right(rec_start, x + L - 1 if strand else x) - 1
        if x < rec_start[r] or x + L > rec_start[r + 1]:
            stats["dropped_bounds"] += 1
            continue
        w = text[x:x + L]
        if not set(w) <= _ACGT:
            stats["dropped_alphabet"] += 1
            continue
        xs.append(x)
        recs.append(r)
        strands.append(strand)
        wins.append(reverseComplement(w) if strand else w)
        stats["reverse" if strand else "forward"] += 1
    stats["loci"] = len(xs)
    stats["distinct"] = len(set(wins))
    return xs, recs, strands, wins, stats


def genome_cut_sites(genomefiles, cutsite, taglen, device=0, backend="gpu"):
    """The in-silico digest of a genome: every place a tag of `taglen` bases could come from.

    genomefiles: one FASTA file or a list of them, plain or .gz, read as exp_frag_size reads them (headers, and
    line.strip().upper() of every other line).  A record's name is its header up to the first whitespace.  A locus is a
    position where a record holds, on either strand, one of the cut site's remnants followed by ACGT only, `taglen`
    bases in all, inside the record.  Returns a CutSites.

    backend="gpu": the genome is framed into one device buffer and scanned there (csrc/place.hip); a genome file
    holding a byte >= 0x80 goes to the host, like exp_frag_size's.  backend="host": str.find over the same rule.
    ValueError: an empty cut site, more than 16 remnants, a cut site longer than taglen, a record with an empty name,
    two records of one name."""
    from . import exp_frag_size as efs
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    remnants, L = _place_remnants(cutsite, taglen)
    paths = [genomefiles] if isinstance(genomefiles, (str, bytes)) else list(genomefiles)
    if backend == "gpu":
        eng = default_engine(device)
        genome = None
        try:
            genome = efs.DeviceGenome(eng, paths)
            names, rec_start = _place_records(genome, genome.nbytes)
            place = eng.place_sites(genome.d_seq, genome.nbytes, rec_start, remnants, L)
        except efs._NeedHost:
            backend = "host"
        finally:
            if genome is not None:
                genome.close()
        if backend == "gpu":
            x, rec, strand, _ = eng.place_loci(place)
            return CutSites(names, rec_start, remnants, L, x, rec, strand, dict(place.stats, backend="gpu"), place=place)
    genome = efs.HostGenome(paths)
    names, rec_start = _place_records(genome, len(genome.text))
    x, rec, strand, wins, stats = _sites_host(genome.text, rec_start, remnants, L)
    return CutSites(names, rec_start, remnants, L, x, rec, strand, dict(stats, backend="host"), windows=wins)


def _place_parts(L, k):
    return [(p * L // (k + 1), (p + 1) * L // (k + 1)) for p in range(k + 1)]


def _place_host(seqs, distinct, L, k):
    """The placement rule of DESIGN 4.20 over dicts: per part, the distinct windows by their bases of that part; a tag is
    compared with the windows that share one of its parts, and a pair counts in the lowest part it agrees on.
    distinct: {window: (multiplicity, first locus id)}.  -> (n_at, dist, locus, compares)."""
    parts = _place_parts(L, k)
    tables = []
    for lo, hi in parts:
        tab = {}
        for w in distinct:
            tab.setdefault(w[lo:hi], []).append(w)
        tables.append(tab)
    n_at, dist, locus, compares = [], [], [], 0
    for s in seqs:
        row = [0, 0, 0, 0]
        first = [PLACE_NO_LOCUS] * 4
        for p, (lo, hi) in enumerate(parts):
            run = tables[p].get(s[lo:hi], ())
            compares += len(run)
            for w in run:
                if any(s[a:b] == w[a:b] for a, b in parts[:p]):
                    continue
                d = sum(1 for u, v in zip(s, w) if u != v)
                if d <= k:
                    mult, fid = distinct[w]
                    row[d] += mult
                    first[d] = min(first[d], fid)
        best = next((d for d in range(k + 1) if row[d]), None)
        n_at.append(row)
        dist.append(PLACE_NONE if best is None else best)
        locus.append(PLACE_NO_LOCUS if best is None else first[best])
    return n_at, dist, locus, compares


class PlacementResult:
    """What place_tags returns, per tag: `.seqs`, `.n_at` (loci at distance 0..3), `.dist` (255: none), `.locus` (id, or
    2^64 - 1), `.status` ('unique', 'multi', 'none'), `.nbest`, `.nwithin`, and for placed tags `.chrom`, `.pos` (SAM
    position), `.cutpos`, `.strand` ('top' / 'bot'; None where there is no locus).  `.stats`: tags, unique, multi,
    none, compares, backend.  `.records`: the genome's (name, length) list; `.taglen`, `.max_mismatch`."""

    def __init__(self, seqs, n_at, dist, locus, sites, k, stats):
        self.seqs, self.taglen, self.max_mismatch, self.records = seqs, sites.taglen, k, sites.records
        self.n_at = [[int(v) for v in row] for row in n_at]
        self.dist = [int(d) for d in dist]
        self.locus = [int(v) for v in locus]
        self.nbest = [row[d] if d != PLACE_NONE else 0 for row, d in zip(self.n_at, self.dist)]
        self.nwithin = [sum(row) for row in self.n_at]
        self.status = ["none" if d == PLACE_NONE else "unique" if b == 1 else "multi" for d, b in zip(self.dist, self.nbest)]
        self.chrom, self.pos, self.cutpos, self.strand = [], [], [], []
        for d, i in zip(self.dist, self.locus):
            placed = d != PLACE_NONE
            self.chrom.append(sites.names[int(sites.rec[i])] if placed else None)
            self.pos.append(int(sites.pos1[i]) if placed else None)
            self.cutpos.append(int(sites.cutpos[i]) if placed else None)
            self.strand.append(("bot" if sites.strand[i] else "top") if placed else None)
        self.stats = dict(stats, tags=len(seqs), unique=self.status.count("unique"), multi=self.status.count("multi"),
                          none=self.status.count("none"))


def place_tags(seqs, sites, max_mismatch=1, backend="gpu"):
    """Where the tags of a census lie on a genome.

    seqs: n ACGT tags of sites.taglen bases (lower case is upper-cased; equal tags are allowed); sites: what
    genome_cut_sites returned.  For every tag the loci whose window differs from it at d = 0 .. max_mismatch positions are
    counted (plain Hamming distance, remnant included, no indels); the tag's distance is the smallest d that has one, its
    locus the first of those, and it is 'unique' when that d has exactly one locus, 'multi' when more, 'none' when no
    locus lies within max_mismatch.  Returns a PlacementResult.

    backend="gpu": the join runs on the device against the digest resident there (csrc/place.hip).  An input whose
    `compares` exceed the device's cap is answered by the host restatement, as is a digest that was built on the host;
    `.stats["backend"]` says which of the two it was.  backend="host": dicts over the same rule.
    ValueError: max_mismatch outside 0..3, tags shorter than max_mismatch + 1, a length other than sites.taglen, a
    character outside ACGT."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    k, L = int(max_mismatch), sites.taglen
    if not 0 <= k <= 3:
        raise ValueError("max_mismatch must be 0..3")
    if L < k + 1:
        raise ValueError("tags of {} bases cannot be placed with {} mismatches: max_mismatch + 1 bases are needed".format(L, k))
    seqs = [s.upper() for s in seqs]
    for i, s in enumerate(seqs):
        if len(s) != L:
            raise ValueError("tag {} has {} bases, the cut sites were taken for {}".format(i, len(s), L))
        if not set(s) <= _ACGT:
            raise ValueError("non-ACGT character in tag {}".format(i))
    answered_by = "host"
    if backend == "gpu" and sites._place is not None:
        if seqs and len(sites.x):
            from ._binding import TagdigError
            eng = sites._place._eng
            try:
                n_at, dist, locus, stats, ms = eng.place_tags(sites._place, "".join(seqs).encode("ascii"), len(seqs), k)
                res = PlacementResult(seqs, n_at, dist, locus, sites, k, dict(compares=stats["compares"], backend="gpu"))
                res.ms = ms
                return res
            except TagdigError as exc:
                if exc.code != -7 or not exc.detail.startswith("tag placement: compares"):
                    raise
        else:
            answered_by = "gpu"           # (nothing to send to the device)
    distinct = sites.distinct() if seqs and len(sites.x) else {}
    n_at, dist, locus, compares = _place_host(seqs, distinct, L, k)
    return PlacementResult(seqs, n_at, dist, locus, sites, k, dict(compares=compares, backend=answered_by))


def writePlacementSAM(filename, result, names=None, multi="drop"):
    """A PlacementResult as a SAM file that readTags_TASSELSAM and exp_frag_size read: @HD, one @SQ per genome record,
    @PG, one line per tag.  QNAME names[t] or tagSeq=<sequence>; FLAG 0 forward, 16 reverse, 4 unplaced ('none', and
    'multi' unless multi="first", which places a multi tag at its first locus); MAPQ 60 for a unique tag with no other
    locus within k, 30 for another unique one, 0 otherwise; CIGAR <L>M; SEQ the tag, reverse-complemented for flag 16;
    NM:i: the mismatches, X0:i: the loci at that distance, X1:i: the other loci within k."""
    if multi not in ("drop", "first"):
        raise ValueError("multi must be 'drop' or 'first'")
    if names is not None and len(names) != len(result.seqs):
        raise ValueError("names and tags differ in number")
    L = result.taglen
    with open(filename, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:unknown\n")
        for nm, ln in result.records:
            fh.write("@SQ\tSN:{}\tLN:{}\n".format(nm, ln))
        fh.write("@PG\tID:tag_place\tPN:tagdigger_amd.tag_place\n")
        for t, s in enumerate(result.seqs):
            qname = names[t] if names is not None else "tagSeq=" + s
            status = result.status[t]
            opt = "X0:i:{}\tX1:i:{}".format(result.nbest[t], result.nwithin[t] - result.nbest[t])
            if status != "none":
                opt = "NM:i:{}\t".format(result.dist[t]) + opt
            if status == "unique" or (status == "multi" and multi == "first"):
                rev = result.strand[t] == "bot"
                mapq = 0 if status == "multi" else 60 if result.nwithin[t] == 1 else 30
                fields = [qname, 16 if rev else 0, result.chrom[t], result.pos[t], mapq, "{}M".format(L), "*", 0, 0,
                          reverseComplement(s) if rev else s, "*", opt]
            else:
                fields = [qname, 4, "*", 0, 0, "*", "*", 0, 0, s, "*", opt]
            fh.write("\t".join(str(f) for f in fields) + "\n")


def writePlacements(filename, result, counts=None):
    """A PlacementResult as CSV: Tag sequence, Count (counts[t], or empty), Status, Chromosome, Position (the cut
    position), Strand (top / bot), Mismatches, Best loci, Loci within k.  A multi tag shows its first locus."""
    with open(filename, "w", newline="") as fh:
        out = _csv.writer(fh)
        out.writerow(["Tag sequence", "Count", "Status", "Chromosome", "Position", "Strand", "Mismatches", "Best loci", "Loci within k"])
        for t, s in enumerate(result.seqs):
            placed = result.status[t] != "none"
            out.writerow([s, "" if counts is None else counts[t], result.status[t],
                          result.chrom[t] if placed else "", result.cutpos[t] if placed else "", result.strand[t] if placed else "",
                          result.dist[t] if placed else "", result.nbest[t], result.nwithin[t]])


def writeCutSites(filename, sites):
    """The in-silico digest as CSV: Chromosome, Cut position, Strand (top / bot), Window, in locus order."""
    with open(filename, "w", newline="") as fh:
        out = _csv.writer(fh)
        out.writerow(["Chromosome", "Cut position", "Strand", "Window"])
        for r, c, st, w in zip(sites.rec.tolist(), sites.cutpos.tolist(), sites.strand.tolist(), sites.windows()):
            out.writerow([sites.names[r], c, "bot" if st else "top", w])


# =============================================================================
# Periphery of the counting path: plain host
# Python, no acceleration -- kept so that the reference's command line stays a
# drop-in.  Same return values, same printed messages, same files written.
# =============================================================================
import bisect as _bisect
import csv as _csv
import gzip as _gzip
import re as _re


def isFastq(filename):
    """1 for a plain FASTQ file, 2 for a gzipped one (chosen by name), 0 otherwise or if it
    cannot be opened -- judged from the first three lines only (reference tagdigger_fun.py:279-307)."""
    gz = filename[-2:].lower() == 'gz'
    try:
        con = _gzip.open(filename, 'rt') if gz else open(filename, 'r')
    except IOError:
        return 0
    verdict = 2 if gz else 1
    try:
        header = con.readline()
        if header[0] != '@':
            verdict = 0
        if not set(con.readline().strip()) <= set('ACGTNacgtn'):
            verdict = 0
        if con.readline()[0] != '+':
            verdict = 0
    finally:
        con.close()
    return verdict


def readBarcodeKeyfile(filename, forSplitter=False):
    """Key file (CSV with File/Barcode/Sample columns, any order) -> {file: [[barcodes], [samples]]},
    or None after printing what is wrong (reference tagdigger_fun.py:309-374)."""
    cols = ("Input File", "Barcode", "Output File") if forSplitter else ("File", "Barcode", "Sample")
    try:
        result = {}
        with open(filename, 'r', newline='') as con:
            where = None
            rownum = 1                                         # the reference's row numbers skip blank lines
            for row in _csv.reader(con):
                if where is None:
                    where = [row.index(c) for c in cols]      # ValueError if a column is missing
                    continue
                f, b, s = row[where[0]].strip(), row[where[1]].strip().upper(), row[where[2]].strip()
                if f == "" and b == "" and s == "":
                    continue
                rownum += 1
                if f == "":
                    raise Exception("Blank cell found where file name should be in row {}.".format(rownum))
                if s == "":
                    raise Exception("Blank cell found where sample name should be in row {}.".format(rownum))
                if not set(b) <= set('ACGT'):
                    raise Exception("{0} in row {1} is not a valid barcode.".format(b, rownum))
                entry = result.setdefault(f, [[], []])
                if b in entry[0]:
                    raise Exception("Each barcode can only be present once for each file.")
                entry[0].append(b)
                entry[1].append(s)
        if forSplitter:
            outs = [s for v in result.values() for s in v[1]]
            if len(set(outs)) < len(outs):
                raise Exception("All output files must have unique names for barcode splitter.")
    except IOError:
        print("Could not read file {}.".format(filename))
        return None
    except ValueError:
        print("File header needed containing '{}', '{}', and '{}'.".format(*cols))
        return None
    except Exception as err:
        print(err.args[0])
        return None
    return result


def readMarkerNames(filename):
    """List of marker names to keep: commas and surrounding whitespace dropped, empty lines
    skipped (reference tagdigger_fun.py:921-934)."""
    try:
        with open(filename, mode='r') as con:
            lines = con.readlines()
    except IOError:
        print("File {} not readable.".format(filename))
        return None
    cleaned = [ln.replace(",", "").strip() for ln in lines]
    return [x for x in cleaned if x != ""]


def compareTags(taglist, trim=True):
    """Variable sites among tags of one locus: [(position, [base per tag]), ...]
    (reference tagdigger_fun.py:376-393)."""
    assert type(taglist) is list, "taglist must be list."
    assert all([set(t) <= set('ATCG') for t in taglist]), "taglist must be a list of ACGT strings."
    lengths = set(len(t) for t in taglist)
    if len(lengths) > 1:
        if trim:
            taglist = [t[:min(lengths)] for t in taglist]
        else:
            taglist = [t.ljust(max(lengths), 'N') for t in taglist]
    out = []
    for i in range(len(taglist[0])):
        col = [t[i] for t in taglist]
        if len(set(c for c in col if c != 'N')) > 1:
            out.append((i, col))
    return out


class _SeqList(list):
    """The list of tag sequences a reader builds, with a set beside it: the reference's uniqueness
    checks are `x in seqlist` on a plain list (quadratic; hours at 500 k tags).  Same answers."""
    def __init__(self):
        super().__init__()
        self._seen = set()

    def __contains__(self, x):
        return x in self._seen

    def append(self, x):
        self._seen.add(x)
        super().append(x)

    def extend(self, xs):
        xs = list(xs)
        self._seen.update(xs)
        super().extend(xs)


def _keep_set(toKeep):
    """Marker names to keep as a set (the reference tests `name in toKeep` on the list)."""
    return None if toKeep is None else set(toKeep)


def _read_tag_table(filename, needed, header_msg, handle_row):
    """Shared skeleton of the CSV tag readers: header check, per-row callback, error printing."""
    names, seqs = [], _SeqList()
    try:
        with open(filename, mode='r') as con:
            where = None
            for rownum, row in enumerate(_csv.reader(con), start=1):
                if where is None:
                    if not set(needed) <= set(row):
                        raise Exception(header_msg)
                    where = [row.index(c) for c in needed]
                else:
                    handle_row(row, where, rownum, names, seqs)
    except IOError:
        print("File {} not readable.".format(filename))
        return None
    except Exception as err:
        print(err.args[0])
        return None
    return [names, list(seqs)]


def readTags_Merged(filename, toKeep=None, allowDuplicates=False):
    """Merged format: marker name + tag with the variable region as [A/C] (reference
    tagdigger_fun.py:563-618).  Names come out as marker_allele_index."""
    toKeep = _keep_set(toKeep)

    def row_fn(row, where, rownum, names, seqs):
        cell = row[where[1]]
        if not set('[/]') < set(cell):
            raise Exception("Characters '[/]' not found in row {}.".format(rownum))
        marker = row[where[0]].strip()
        if '_' in marker:
            raise Exception("Marker {}: marker names cannot contain underscores.".format(row[where[0]]))
        if toKeep != None and marker not in toKeep:
            return
        left, right = cell.find('['), cell.find(']')
        alleles = [a.strip().upper() for a in cell[left + 1:right].split('/')]
        tags = [(cell[:left] + a + cell[right + 1:]).upper().strip().replace('-', '') for a in alleles]
        if not allowDuplicates and any([t in seqs for t in tags]):
            print("Non-unique sequence found: line {0}.".format(rownum))
            print("Marker {} skipped.".format(marker))
            return
        seqs.extend(tags)
        if not all([set(t) <= set('ACGT') for t in tags]):
            raise Exception("Tag sequence not formatted correctly in row {}.".format(rownum))
        names.extend(["{}_{}_{}".format(marker, alleles[i], i) for i in range(len(tags))])
    return _read_tag_table(filename, ("Marker name", "Tag sequence"),
                           "Need 'Marker name' and 'Tag sequence' in header row.", row_fn)


def readTags_Rows(filename, toKeep=None):
    """One row per allele: marker name, allele name, tag (reference tagdigger_fun.py:475-514)."""
    toKeep = _keep_set(toKeep)

    def row_fn(row, where, rownum, names, seqs):
        marker = row[where[0]].strip()
        if '_' in marker:
            raise Exception("Marker {}: marker names cannot contain underscores.".format(marker))
        if toKeep != None and marker not in toKeep:
            return
        allele = row[where[1]].strip()
        tag = row[where[2]].upper().strip()
        if not set(tag) <= set('ACGT'):
            raise Exception("Tag sequence not formatted as ACGT in row {}.".format(rownum))
        if tag in seqs:
            raise Exception("Non-unique sequence found: line {0}.".format(rownum))
        names.append(marker + '_' + allele)
        seqs.append(tag)
    return _read_tag_table(filename, ("Marker name", "Allele name", "Tag sequence"),
                           "Need 'Marker name', 'Allele name', and 'Tag sequence' in header row.", row_fn)


def readTags_Columns(filename, toKeep=None):
    """One row per marker with two tags (reference tagdigger_fun.py:516-561)."""
    toKeep = _keep_set(toKeep)

    def row_fn(row, where, rownum, names, seqs):
        marker = row[where[0]].strip()
        if '_' in marker:
            raise Exception("Marker {}: marker names cannot contain underscores.".format(marker))
        if toKeep != None and marker not in toKeep:
            return
        tag0, tag1 = row[where[1]].upper().strip(), row[where[2]].upper().strip()
        if not set(tag0 + tag1) <= set('ACGT'):
            raise Exception("Tag sequence not formatted as ACGT in row {}.".format(rownum))
        if tag0 in seqs or tag1 in seqs:
            raise Exception("Non-unique sequence found: line {0}.".format(rownum))
        seqs.extend([tag0, tag1])
        diff = compareTags([tag0, tag1])
        names.append(marker + '_' + ''.join(d[1][0] for d in diff) + '_0')
        names.append(marker + '_' + ''.join(d[1][1] for d in diff) + '_1')
    return _read_tag_table(filename, ("Marker name", "Tag sequence 0", "Tag sequence 1"),
                           "Need 'Marker name', 'Tag sequence 0', and 'Tag sequence 1' in header row.", row_fn)


def readTags_UNEAK_FASTA(filename, toKeep=None):
    """Tag pairs from a TASSEL-UNEAK FASTA: four lines per pair, '>TPn_query_len' / sequence /
    '>TPn_hit_len' / sequence (reference tagdigger_fun.py:395-473)."""
    names, seqs = [], _SeqList()
    toKeep = _keep_set(toKeep)
    try:
        with open(filename, mode='r') as con:
            name1 = name2 = seq1 = seq2 = None
            len1 = len2 = 0
            for n, line in enumerate(con):
                part = n % 4
                if part in (0, 2):
                    if line[:3] != ">TP":
                        raise Exception("Line {0} of {1} does not start with '>TP'.".format(n + 1, filename))
                    cut = line.rfind("_")
                    if part == 0:
                        name1 = line[1:cut]
                        len1 = int(line[cut + 1:].strip())     # real tag length (some are padded with A's)
                    else:
                        name2 = line[1:cut]
                        if name1[:name1.find("_")] != name2[:name2.find("_")]:
                            raise Exception("Tag name in line {0} does not match tag name in line {1}.".format(n + 1, n - 1))
                        len2 = int(line[cut + 1:].strip())
                    continue
                seq = line.strip().upper()
                seq = seq[:len1] if part == 1 else seq[:len2]
                if not set(seq) <= set('ACGT'):
                    raise Exception("Line {0} is not ACGT sequence.".format(n + 1))
                if seq in seqs:
                    raise Exception("Non-unique sequence found: line {0}.".format(n + 1))
                if part == 1:
                    seq1 = seq
                    continue
                seq2 = seq
                marker = name1[:name1.find("_")]
                if toKeep != None and marker not in toKeep:
                    continue
                shortest = min(len1, len2)
                if len1 != len2 and seq1[:shortest] == seq2[:shortest]:
                    print("{} skipped because tags cannot be distinguished.".format(marker))
                    continue
                diff = compareTags([seq1, seq2])
                base1, base2 = diff[0][1][0], diff[0][1][1]
                first_is_0 = base1 < base2                       # alphabetical, to match hapMap2numeric
                names.extend([name1 + "_" + base1 + ("_0" if first_is_0 else "_1"),
                              name2 + "_" + base2 + ("_1" if first_is_0 else "_0")])
                seqs.extend([seq1[:shortest], seq2[:shortest]])
    except IOError:
        print("File {} not readable.".format(filename))
        return None
    except Exception as err:
        print(err.args[0])
        return None
    return [names, list(seqs)]


def reverseComplement(sequence):
    """Reverse complement; characters other than A, C, G, T pass through unchanged (reference
    tagdigger_fun.py:1203-1206)."""
    return sequence.translate({65: 'T', 67: 'G', 71: 'C', 84: 'A'})[::-1]


def _open_maybe_gz(path):
    """Text-mode handle; gzip when the name ends in '.gz' (as the Stacks reader decides, :630)."""
    return _gzip.open(path, mode='rt') if path.endswith('.gz') else open(path, mode='r')


def _stacks_rows(path):
    """Rows of a Stacks catalog table (tab separated), comment rows ('#...') left out."""
    with _open_maybe_gz(path) as con:
        for row in _csv.reader(con, delimiter='\t'):
            if not row[0].startswith("#"):
                yield row


def readTags_Stacks(tagsfile, snpsfile, allelesfile, toKeep=None, binaryOnly=False, version=1):
    """Tags from a Stacks catalog: consensus sequences (tags.tsv), SNP columns (snps.tsv) and
    haplotypes (alleles.tsv) -> one tag per haplotype, named locus_haplotype (reference
    tagdigger_fun.py:620-719).  The column layout depends on the Stacks version."""
    if version == 1:
        col_locus, col_seq, col_hap, col_pos = 2, 9, 3, 3
    else:
        col_locus, col_seq, col_hap, col_pos = 1, 5, 2, 2
    wanted = lambda locus: toKeep == None or locus in toKeep
    try:
        consensus = {}
        for row in _stacks_rows(tagsfile):
            if wanted(row[col_locus]):
                consensus[row[col_locus]] = row[col_seq]
        haplotypes = []
        for row in _stacks_rows(allelesfile):
            if wanted(row[col_locus]):
                haplotypes.append((row[col_locus], row[col_hap]))
        snp_columns = {}
        for row in _stacks_rows(snpsfile):
            if wanted(row[col_locus]):
                snp_columns.setdefault(row[col_locus], []).append(int(row[col_pos]))

        names, seqs = [], []
        for locus, hap in haplotypes:
            seq = consensus[locus]
            if len(hap) > 0:
                # the haplotype's k-th character replaces the consensus base at the k-th SNP column
                cols = snp_columns[locus]
                pieces = [seq[:cols[0]]]
                for k, base in enumerate(hap):
                    pieces.append(base)
                    pieces.append(seq[cols[k] + 1:] if k + 1 == len(hap) else seq[cols[k] + 1:cols[k + 1]])
                seq = "".join(pieces)
            seq = seq.upper()
            if set(seq) <= set('ACGT'):
                names.append(locus + '_' + hap)
                seqs.append(seq)
            else:
                print("{}_{} skipped for having non-ACGT nucleotides.".format(locus, hap))
        if binaryOnly:
            # loci with exactly two haplotypes; 0 / 1 by alphabetical order of the haplotypes
            kept_names, kept_seqs = [], []
            for alleles, where in extractMarkers(names)[1]:
                if len(alleles) != 2:
                    continue
                first_is_0 = alleles[0] < alleles[1]
                kept_names.append(names[where[0]] + ('_0' if first_is_0 else '_1'))
                kept_names.append(names[where[1]] + ('_1' if first_is_0 else '_0'))
                kept_seqs.extend([seqs[where[0]], seqs[where[1]]])
            names, seqs = kept_names, kept_seqs
        return [names, seqs]
    except IOError:
        print("Files not readable.")
    except (IndexError, ValueError):
        print("Files in wrong format.")
    except KeyError:
        print("Locus names not matching properly.")
    except Exception as err:
        print(err.args[0])
    return None


_SAM_UNALIGNED = {4 + f for f in (0, 1, 2, 8, 16, 32, 64, 128)}     # the forms of flag 4 the reference tests for (:750)
_SAM_REVERSE = {16 + f for f in (0, 1, 2, 8, 32, 64, 128)}          # and of flag 16 (:761)


def readTags_TASSELSAM(filename, toKeep=None, binaryOnly=False, noMonomorphic=False,
                       writeMarkerKey=False, keyfilename=None):
    """Tags from a SAM file of aligned TASSEL-GBSv2 tags; alignments that start at the same
    position and strand are the tags of one marker, named chromosome-position-strand (reference
    tagdigger_fun.py:721-854).  toKeep holds TASSEL SNP names (e.g. S03_350622)."""
    assert (not writeMarkerKey) or keyfilename != None, "keyfilename needed."
    names, seqs, snp_key = [], [], []
    by_marker = {}
    width = 0            # digits of the longest chromosome length seen so far (@SQ LN:)
    try:
        with open(filename, mode='r') as con:
            for line in con:
                if line[0:3] == '@SQ':
                    width = max(width, len(line.split()[2][3:]))
                    continue
                if line[0] == '@':
                    continue
                f = line.split()
                flags = int(f[1])
                if flags in _SAM_UNALIGNED:
                    continue
                chrom = f[2].replace('_', '*')            # '_' separates marker from allele in tag names
                pos = int(f[3])
                seq = f[9]
                strand = "top"
                if flags in _SAM_REVERSE:
                    strand = "bot"
                    seq = reverseComplement(seq)
                    # the tag starts at the cut site, i.e. at the alignment's last reference base
                    cigar = f[5]
                    deleted = sum(int(x[:-1]) for x in _re.findall(r'\d+D', cigar))
                    inserted = sum(int(x[:-1]) for x in _re.findall(r'\d+I', cigar))
                    pos = pos + len(seq) - inserted + deleted - 1
                marker = "{}-{:0>{width}}-{}".format(chrom, pos, strand, width=width)
                if marker not in by_marker:
                    by_marker[marker] = [seq]
                    continue
                # of two tags one of which is a prefix of the other, the shorter stays (:776-785)
                kept = [t for t in by_marker[marker] if not t.startswith(seq)]
                by_marker[marker] = kept
                if not any(seq.startswith(t) for t in kept):
                    kept.append(seq)

        for marker in sorted(by_marker):
            tags = by_marker[marker]
            if (binaryOnly and len(tags) != 2) or (noMonomorphic and len(tags) == 1):
                continue
            diff = compareTags(tags, trim=False)
            if toKeep != None or writeMarkerKey:
                chrom, postext, strand = marker.split('-')[:3]
                chrom = chrom.upper()
                if chrom.startswith("CHROMOSOME"):
                    chrom = chrom[10:]
                if chrom.startswith("CHR"):
                    chrom = chrom[3:]
                step = 1 if strand == 'top' else -1
                tassel_names = ['S{}_{}'.format(chrom, int(postext) + step * d[0]) for d in diff]
                if toKeep != None and all(n not in toKeep for n in tassel_names):
                    continue
                if writeMarkerKey:
                    snp_key.extend((n, marker) for n in tassel_names)
            alleles = [''.join(d[1][i] for d in diff) for i in range(len(tags))]
            tagnames = [marker + '_' + a for a in alleles]
            if binaryOnly and alleles[0] != alleles[1]:
                low = 0 if alleles[0] < alleles[1] else 1
                tagnames[low] += '_0'
                tagnames[1 - low] += '_1'
            names.extend(tagnames)
            seqs.extend(tags)
        if len(names) == 0:
            raise Exception("No markers output; is list of markers to keep in right format (e.g. S03_350622)?")
    except IOError:
        print("Could not read file {}.".format(filename))
        return None
    except Exception as err:
        print(err.args[0])
        return None
    if writeMarkerKey:
        try:
            with open(keyfilename, mode='w', newline='') as out:
                w = _csv.writer(out)
                w.writerow(["TASSEL-GBSv2 marker name", "TagDigger marker name"])
                for pair in snp_key:
                    w.writerow(pair)
        except IOError:
            print("Could not write file {}.".format(keyfilename))
            return None
    return [names, seqs]


def _pyrad_locus(seqset, marker, binaryOnly):
    """Names and sequences for the alleles of one pyRAD locus (reference tagdigger_fun.py:865-889):
    trim to the shortest, drop trailing gap columns, drop alleles with N, sort, name by the
    variable columns."""
    n = min(len(x) for x in seqset)
    aligned = [x[:n] for x in seqset]
    while any(x[-1] == '-' for x in aligned):
        aligned = [x[:-1] for x in aligned]
        n -= 1
    aligned = sorted(set(x for x in aligned if 'N' not in x))
    if not ((len(aligned) != 0 and not binaryOnly) or len(aligned) == 2):
        return [], []
    variable = [i for i in range(n) if len(set(x[i] for x in aligned)) > 1]
    names = ['{}_{}_{}'.format(marker, ''.join(x[i] for i in variable), k) for k, x in enumerate(aligned)]
    return names, [x.replace('-', '') for x in aligned]


def readTags_pyRAD(filename, toKeep=None, binaryOnly=False):
    """Tags from a pyRAD .alleles file: '>sample  sequence' lines, each locus closed by a '//' line
    that carries its number (reference tagdigger_fun.py:856-919)."""
    names, seqs = [], []
    current = set()
    linenum = 0
    try:
        with open(filename, mode='r') as con:
            for line in con:
                if line[0] == '>':
                    seq = line.split()[1]
                    if not set(seq) <= set('ACGT-N'):
                        raise Exception("Character other than ACGTN- detected in sequence.")
                    current.add(seq)
                elif line[0] == '/':
                    marker = line.split()[-1][1:-1]
                    for ch in "|*-":
                        marker = marker.replace(ch, "")
                    if toKeep == None or marker in toKeep:
                        n, q = _pyrad_locus(current, marker, binaryOnly)
                        names.extend(n)
                        seqs.extend(q)
                    current = set()
                else:
                    raise Exception("File not in pyRAD format.")
                linenum += 1
    except IOError:
        print("File {} not readable.".format(filename))
        return None
    except Exception as err:
        print("Line {}:".format(linenum))
        print(err.args[0])
        return None
    return [names, seqs]


# adapter sets for the barcode splitter: (restriction site with ^ where genomic sequence ends,
# top-strand adapter after the overhang; [barcode] = reverse complement of the barcode)
# (reference tagdigger_fun.py:27-47)
_P5_BARCODED = '[barcode]AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGTAGATCTCGGTGGTCGCCGTATCATT'
_HALL_COMMON = 'CTCAGGCATCACTCGATTCCTCCGTCGTATGCCGTCTTCTGCTTG'
_CLARK_COMMON = 'CTCAGGCATCACTCGATTCCTATCTCGTATGCCGTCTTCTGCTTG'
adapters = {'PstI-MspI-Hall': [('CCG^G', _HALL_COMMON), ('CTGCA^G', _P5_BARCODED)],
            'NsiI-MspI-Hall': [('CCG^G', _HALL_COMMON), ('ATGCA^T', _P5_BARCODED)],
            'PstI-MspI-Clark': [('CCG^G', _CLARK_COMMON), ('CTGCA^G', _P5_BARCODED)],
            'NsiI-MspI-Clark': [('CCG^G', _CLARK_COMMON), ('ATGCA^T', _P5_BARCODED)],
            'PstI-MspI-Poland': [('CCG^G', 'AGATCGGAAGAGCGGTTCAGCAGGAATGCCGAGACCGATCTCGTATGCCGTCTTCTGCTTG'),
                                 ('CTGCA^G', _P5_BARCODED)]}


def _trie_survivors(sequences):
    """Which of `sequences` (ACGT strings) a prefix trie built in this order would hold, as
    (sequence, position) pairs -- the rules of tree_one_level (reference tagdigger_fun.py:71-86):
    among sequences sharing a path, if the FIRST one ends there it is kept and the others
    (duplicates, extensions) are dropped silently; if a LATER one ends inside the first, that is an
    AssertionError naming its position.  Children are visited in A, C, G, T order."""
    kept = []

    def walk(group, depth):
        first = group[0]
        if len(first[0]) == depth:
            kept.append(first)
            return
        branches = ([], [], [], [])
        for item in group:
            assert len(item[0]) > depth, \
                "Problematic sequence: {}.  Likely due to overlapping tags.".format(item[1])
            branches["ACGT".find(item[0][depth])].append(item)
        for branch in branches:
            if branch:
                walk(branch, depth + 1)

    if sequences:
        walk([(s, k) for k, s in enumerate(sequences)], 0)
    return kept


def _adapter_ends(adapter, barcodes):
    """For every barcode, the adapter beginnings the splitter looks for at the END of a read, each
    with the (negative) index the read is then sliced with: what build_adapter_tree (reference
    tagdigger_fun.py:1208-1249) builds as a reversed-sequence trie, resolved to a flat list.
    Every beginning keeps at least one base beyond the remains of the restriction site."""
    def beginnings(site, tail):
        remains = site.find('^')
        full = site[:remains] + tail
        # longest first, down to one base past the site's remains; reversed, as the trie stores them
        rev = full[::-1]
        cut = [rev[i:] for i in range(len(rev) - remains)]
        return remains, cut, [remains - len(c) for c in cut]

    remains0, common, common_idx = beginnings(adapter[0][0], adapter[0][1])
    out = []
    for bc in barcodes:
        remains1, rare, rare_idx = beginnings(adapter[1][0], adapter[1][1].replace('[barcode]', reverseComplement(bc)))
        everything, indices = common + rare, common_idx + rare_idx
        try:
            kept = _trie_survivors(everything)
        except AssertionError:
            # some beginning is the end of another: keep the shorter of each such (sorted-adjacent) pair
            print("Some overlap of adapter sequence for barcode {}.".format(bc))
            everything = sorted(everything)
            drop = set()
            for k in range(len(everything) - 1):
                if everything[k + 1].startswith(everything[k]):
                    drop.add(k + 1)
                    print("Won't search for {0} at end of sequence since {1} is already being searched for.".format(
                        everything[k + 1][::-1], everything[k][::-1]))
            everything = [x for k, x in enumerate(everything) if k not in drop]
            indices = [remains1 - len(x) for x in everything]          # (the rare cutter's offset for all, as :1246)
            kept = _trie_survivors(everything)
        out.append([(seq[::-1], indices[pos]) for seq, pos in kept])
    return out


def barcodeSplitter(inputFile, barcodes, outputFiles, cutsite='TGCAG', adapter=adapters["PstI-MspI-Hall"],
                    maxreads=500000000, device=0):
    """Split one FASTQ file into one file per barcode, removing the barcode and, on the 3' end,
    anything from the first full restriction site or from an adapter that runs off the read
    (reference tagdigger_fun.py:1286-1368).  The per-read decisions are made on the GPU.
    The progress lines of the reference's loop (:1357-1360) are printed once the file is through."""
    assert set(cutsite) <= set('ACGT'), "Only ACGT cut sites allowed."
    assert all([set(bc) <= set('ACGT') for bc in barcodes]), "Found non-ACGT barcodes."
    assert len(adapter) == 2
    assert all([set(a[0]) <= set('ACGT^') for a in adapter])
    assert set(adapter[0][1]) <= set('ACGT')
    assert set(adapter[1][1]) <= set('[barcode]ACGT')

    print("Building indices for rapid searching...")
    entries = _adapter_ends(adapter, barcodes)
    eng = default_engine(device)
    eng.set_splitter(barcodes, cutsite, adapter[0][0].replace('^', ''), adapter[1][0].replace('^', ''), entries)
    print("Done with indexing setup.")
    print(inputFile)

    # the same failures as the reference's open() calls, in its order (:1318-1327)
    if inputFile[-2:].lower() == 'gz':
        with open(inputFile, 'rb') as fh:
            head = fh.read(2)
        if head and head != b'\x1f\x8b':
            raise _gzip.BadGzipFile("Not a gzipped file (%r)" % head)
    else:
        open(inputFile, 'r').close()
    for name in outputFiles:
        open(name, mode='w').close()
    reads, _, _ = eng.split_file(inputFile, outputFiles, maxreads)
    for line in eng.split_progress_lines(inputFile, reads):
        print(line)
    return None


def sanitizeTags(taglist):
    """Drop every marker one of whose tags is a prefix of (or equal to) another tag, so that the
    tag set handed to find_tags_fastq is prefix-free (reference tagdigger_fun.py:1030-1058).
    Mutates and returns taglist.  Marker membership is a NAME-PREFIX test, as in the reference:
    removing 'TP27' also removes 'TP276...'."""
    assert len(taglist) == 2, "'taglist' should have two elements."
    assert len(taglist[0]) == len(taglist[1]), \
        "List of tag names should be the same as list of tag sequences."
    print("\nSanitizing tags...")
    names, seqs = taglist
    ordered = sorted(seqs)
    for k in range(len(ordered) - 1):
        short = ordered[k]
        if not ordered[k + 1].startswith(short) or short not in seqs:
            continue
        owner = names[seqs.index(short)]
        marker = owner[:owner.find("_")]
        print("Removing " + marker + " for overlap with another marker.")
        for j in sorted((j for j in range(len(seqs)) if names[j].startswith(marker)), reverse=True):
            print(names.pop(j))
            print(seqs.pop(j))
    return taglist


def _is_array(x):
    return type(x).__module__ == "numpy"


def sample_rows(bckeys):
    """Global sample order exactly as combineReadCounts builds it, and per file the row of each barcode."""
    order, slot, rows = [], {}, {}
    for f in sorted(bckeys.keys()):
        rows[f] = []
        for sample in bckeys[f][1]:
            if sample not in slot:
                slot[sample] = len(order)
                order.append(sample)
            rows[f].append(slot[sample])
    return order, rows


def combineReadCounts(countsdict, bckeys):
    """Per-barcode rows of every library -> per-sample rows: files in sorted order, samples in
    order of first appearance, equal names summed (reference tagdigger_fun.py:1061-1098).
    This is also what a multi-GPU run must equal after its all-reduce.
    Matrices given as numpy arrays (Engine.counts_numpy, what the command line uses) are summed with
    numpy and the totals come back as one int64 array; lists give lists, as in the reference."""
    files = sorted(bckeys.keys())
    if files and all(_is_array(countsdict[f]) for f in files):
        import numpy as np
        order, rows = sample_rows(bckeys)
        totals = np.zeros((len(order), countsdict[files[0]].shape[1]), dtype=np.int64)
        for f in files:
            np.add.at(totals, rows[f], countsdict[f].astype(np.int64, copy=False))
        return [order, totals]
    order, totals = [], []
    slot = {}
    for f in files:
        for row, sample in enumerate(bckeys[f][1]):
            if sample in slot:
                k = slot[sample]
                totals[k] = [a + b for a, b in zip(countsdict[f][row], totals[k])]
            else:
                slot[sample] = len(order)
                order.append(sample)
                totals.append(countsdict[f][row])
    return [order, totals]


def _csv_cell(text):
    """One field exactly as csv.writer (default dialect, minimal quoting) writes it as the FIRST of several fields
    (a row of one empty field is written as '""', an empty first field of a longer row as nothing)."""
    import io
    buf = io.StringIO()
    _csv.writer(buf).writerow([text, "x"])
    return buf.getvalue()[:-4]                      # (without ',x' and the row's \r\n)


def writeCounts(filename, counts, samnames, tagnames):
    """Samples x tags CSV, csv.writer defaults (CRLF rows) (reference tagdigger_fun.py:1100-1111).
    A numpy matrix is written row by row with ndarray.tofile (decimal integers, the same bytes)."""
    assert len(samnames) == len(counts), "Length of samnames should be the same as length of counts."
    assert len(tagnames) == len(counts[0]), "Length of tagnames should be length of second dimension of counts."
    if _is_array(counts):
        import io
        import locale
        import numpy as np
        enc = locale.getpreferredencoding(False)            # (what open(..., 'w') would encode with)
        head = io.StringIO()
        _csv.writer(head).writerow([""] + tagnames)
        rows = np.ascontiguousarray(counts, dtype=np.int64)
        import ctypes
        from . import _binding
        fmt = _binding.load().td_format_csv_row                # (integer rows formatted by the library: 200 M cells/s)
        buf = ctypes.create_string_buffer(24 * max(1, rows.shape[1]))
        with open(filename, mode='wb') as fb:
            fb.write(head.getvalue().encode(enc))
            for name, row in zip(samnames, rows):
                n = fmt(row.ctypes.data, rows.shape[1], buf, len(buf))
                if n < 0:
                    raise RuntimeError("td_format_csv_row: buffer too small")
                fb.write((_csv_cell(name) + ",").encode(enc))
                fb.write(memoryview(buf)[:n])
                fb.write(b"\r\n")
        return
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow([""] + tagnames)
        for name, row in zip(samnames, counts):
            out.writerow([name] + row)


def extractMarkers(tagnames):
    """[marker names in first-seen order, per marker [[allele names], [tag indices]]]
    (reference tagdigger_fun.py:1113-1142)."""
    if len(tagnames) != len(set(tagnames)):
        raise Exception("Non-unique tag names found.")
    markers, alleles, where = [], [], {}
    for k, t in enumerate(tagnames):
        m = t[:t.find('_')]
        if m not in where:
            where[m] = len(markers)
            markers.append(m)
            alleles.append([[], []])
        alleles[where[m]][0].append(t[t.rfind('_') + 1:])
        alleles[where[m]][1].append(k)
    return [markers, alleles]


def writeDiploidGeno(filename, counts, samnames, tagnames):
    """0 / 1 / 2 / blank genotype calls from the allele-0 and allele-1 counts of every marker
    (reference tagdigger_fun.py:1144-1180)."""
    assert len(samnames) == len(counts), "Length of samnames should be the same as length of counts."
    assert len(tagnames) == len(counts[0]), "Length of tagnames should be length of second dimension of counts."
    markers, alleles = extractMarkers(tagnames)
    try:
        if not all(set(a[0]) <= {'0', '1'} for a in alleles):
            raise Exception("All allele names must be '0' or '1'.")
        if _is_array(counts):
            import numpy as np
            i0 = np.array([a[1][a[0].index('0')] for a in alleles], dtype=np.int64)
            i1 = np.array([a[1][a[0].index('1')] for a in alleles], dtype=np.int64)
            has0, has1 = counts[:, i0] > 0, counts[:, i1] > 0
            table = np.array(['', '0', '2', '1'])                  # neither, allele 0 only, allele 1 only, both
            rows = table[has0 + 2 * has1].tolist()
        else:
            rows = []
            for s in range(len(samnames)):
                calls = []
                for a in alleles:
                    c0 = counts[s][a[1][a[0].index('0')]]
                    c1 = counts[s][a[1][a[0].index('1')]]
                    calls.append('1' if c0 > 0 and c1 > 0 else '0' if c0 > 0 else '2' if c1 > 0 else '')
                rows.append(calls)
        with open(filename, mode='w', newline='') as fh:
            out = _csv.writer(fh)
            out.writerow([""] + markers)
            for name, calls in zip(samnames, rows):
                out.writerow([name] + calls)
    except IOError:
        print("Could not write file {}.".format(filename))
    except Exception as err:
        print(err.args[0])
    return None


# ---------------------------------------------------------------------------------------------------------------------
# Genotype calls and marker filters from the count matrix: the step behind census -> pairs -> counts.
# The rule is stated in integers; call_genotypes(backend="host") restates it in numpy, csrc/genocall.hip runs it where
# the matrix lies.  Both read the same threshold table, which only this module builds.
GENO_STATS = ("called", "n0", "n1", "n2", "alt", "depth0", "depth1")
GENO_RULES = ("likelihood", "presence")
GENO_MISSING = 3
_HET_TABLE = {}


def _ppm(value, lo, hi, what):
    """A rate as parts per million, an integer in lo .. hi."""
    ppm = int(round(float(value) * 1e6))
    if not lo <= ppm <= hi:
        raise ValueError("{} must lie in [{}, {}]".format(what, lo / 1e6, hi / 1e6))
    return ppm


def het_threshold_table(err):
    """het_min[0 .. 127] for the sequencing error rate e = round(err * 10^6) / 10^6 (1 ppm .. 499 999 ppm), as exact
    rationals: het_min[n] is the smallest k in 0 .. n // 2 for which a heterozygote explains k reads of the rarer allele
    among n better than an error does -- (1/2)^n > (1 - e)^(n - k) e^k -- or n + 1 when no k does; het_min[0] = 1.
    A cell with min(a, b) >= het_min[a + b] is called heterozygous."""
    from fractions import Fraction
    ppm = _ppm(err, 1, 499999, "err")
    if ppm not in _HET_TABLE:
        e = Fraction(ppm, 1000000)
        table = [1]
        for n in range(1, 128):
            half = Fraction(1, 2) ** n
            table.append(next((k for k in range(n // 2 + 1) if half > (1 - e) ** (n - k) * e ** k), n + 1))
        _HET_TABLE[ppm] = tuple(table)
    return list(_HET_TABLE[ppm])


class DeviceCounts:
    """A samples x tags uint32 count matrix in device memory (what the counter and Engine.fold_rows fill), for
    call_genotypes(backend="gpu"): `ptr` a device pointer, `shape` = (samples, tags)."""

    def __init__(self, ptr, shape):
        self.ptr, self.shape = int(ptr), (int(shape[0]), int(shape[1]))

    def __len__(self):
        return self.shape[0]


class GenoResult:
    """What call_genotypes returns: `.markers` (names in first-seen order), `.samples`, `.calls` (uint8 [samples,
    markers]: copies of allele 1, 3 = missing), `.stats` (called, n0, n1, n2, alt, depth0, depth1 as arrays over the
    markers; passed, backend, ms and the parameters), `.mask` (bool per marker: it passes the filters), `.columns`
    (the count matrix' columns of allele 0 and allele 1 per marker), `.d_calls` (call_genotypes(keep_device=True) on the
    gpu backend: a DeviceCalls, the calls where the kernel wrote them, which the caller frees; else None)."""

    def __init__(self, markers, samples, calls, stats, mask, columns, d_calls=None):
        self.markers, self.samples, self.calls, self.stats, self.mask, self.columns = markers, samples, calls, stats, mask, columns
        self.d_calls = d_calls


def _geno_markers(tagnames):
    """(marker names, columns of allele '0', columns of allele '1') by extractMarkers."""
    markers, alleles = extractMarkers(tagnames)
    if not all(sorted(a[0]) == ['0', '1'] for a in alleles):
        raise Exception("All allele names must be '0' or '1'.")
    return markers, [a[1][a[0].index('0')] for a in alleles], [a[1][a[0].index('1')] for a in alleles]


def _geno_host(counts, i0, i1, table, rule, min_depth, min_call_ppm, min_maf_ppm, max_het_ppm):
    """The rule of DESIGN 4.14 in numpy's uint64, which holds every intermediate exactly: n < 2^33, 127 a < 2^39, the
    filters' products < 2^54."""
    import numpy as np
    S, M = counts.shape[0], len(i0)
    a = counts[:, i0].astype(np.uint64)
    b = counts[:, i1].astype(np.uint64)
    n = a + b
    if rule == "presence":
        code = np.where((a > 0) & (b > 0), 1, np.where(a > 0, 0, 2))
    else:
        deep = n > 127
        div = np.where(deep, n, 1)
        x = np.where(deep, 127 * a // div, a)
        y = np.where(deep, 127 * b // div, b)
        het = np.minimum(x, y) >= np.asarray(table, dtype=np.uint64)[x + y]
        code = np.where(het, 1, np.where(x >= y, 0, 2))
    calls = np.where(n < np.uint64(min_depth), GENO_MISSING, code).astype(np.uint8)
    n0, n1, n2 = ((calls == c).sum(axis=0, dtype=np.uint64) for c in (0, 1, 2))
    called, alt = n0 + n1 + n2, n1 + 2 * n2
    million = np.uint64(1000000)
    mask = ((called * million >= np.uint64(min_call_ppm * S)) &
            (np.minimum(alt, 2 * called - alt) * million >= np.uint64(min_maf_ppm) * 2 * called) &
            (n1 * million <= np.uint64(max_het_ppm) * called))
    if S == 0:
        mask[:] = False                               # no sample: no marker passes on no evidence
    stats = dict(zip(GENO_STATS, (called, n0, n1, n2, alt, a.sum(axis=0, dtype=np.uint64), b.sum(axis=0, dtype=np.uint64))))
    return calls, stats, mask


def call_genotypes(counts, samnames, tagnames, rule="likelihood", err=0.01, min_depth=1, min_call_rate=0.0, min_maf=0.0,
                   max_het=1.0, device=0, backend="gpu", keep_device=False):
    """Genotype calls from a samples x tags count matrix, and which markers pass the filters.

    Markers and alleles come from the tag names as extractMarkers reads them; every marker needs exactly one allele
    '0' and one allele '1'.  For a sample's counts a and b of the two alleles, n = a + b:
      missing (3)          n < min_depth
      rule="presence"      1 when both were seen, else 0 or 2 -- writeDiploidGeno's table when min_depth is 1
      rule="likelihood"    n above 127 is scaled to 127 first (a' = 127 a // n, b' = 127 b // n); heterozygous (1) when
                           min(a', b') >= het_threshold_table(err)[a' + b'], else 0 when a' >= b', else 2
    A marker passes when called / samples >= min_call_rate, its minor allele frequency among the called >= min_maf and
    the share of heterozygous calls <= max_het -- all three compared as integers in parts per million.
    counts: a numpy matrix or lists (uint32 values), or a DeviceCounts (backend="gpu" only).  backend="gpu" runs
    csrc/genocall.hip on the matrix where it lies; backend="host" is the numpy restatement.  keep_device=True with the
    gpu backend leaves the calls on the device as well: `.d_calls` is a DeviceCalls for sample_relations, and the
    caller's to free (default_engine(device).dev_free(result.d_calls.ptr) when ptr is not 0).  Returns a GenoResult."""
    import numpy as np
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    if rule not in GENO_RULES:
        raise ValueError("rule must be 'likelihood' or 'presence'")
    err_ppm = _ppm(err, 1, 499999, "err")
    if int(min_depth) != min_depth or min_depth < 1:
        raise ValueError("min_depth must be an integer of at least 1")
    min_depth = int(min_depth)
    min_call_ppm = _ppm(min_call_rate, 0, 1000000, "min_call_rate")
    min_maf_ppm = _ppm(min_maf, 0, 500000, "min_maf")
    max_het_ppm = _ppm(max_het, 0, 1000000, "max_het")
    on_device = isinstance(counts, DeviceCounts)
    if on_device and backend != "gpu":
        raise ValueError("a DeviceCounts matrix needs backend='gpu'")
    if not on_device:
        from .engine import counts_as_uint32
        counts = counts_as_uint32(counts if len(counts) else np.zeros((0, len(tagnames)), dtype=np.uint32))
    assert len(samnames) == counts.shape[0], "Length of samnames should be the same as length of counts."
    assert len(tagnames) == counts.shape[1], "Length of tagnames should be length of second dimension of counts."
    markers, i0, i1 = _geno_markers(tagnames)
    table = het_threshold_table(err_ppm / 1e6)
    d_calls = None
    if backend == "host":
        calls, stats, mask = _geno_host(counts, i0, i1, table, rule, min_depth, min_call_ppm, min_maf_ppm, max_het_ppm)
        ms = 0.0
    else:
        res = default_engine(device).geno_call(counts.ptr if on_device else counts, i0, i1, table,
                                               shape=counts.shape if on_device else None, rule=GENO_RULES.index(rule),
                                               err_ppm=err_ppm, min_depth=min_depth, min_call_ppm=min_call_ppm,
                                               min_maf_ppm=min_maf_ppm, max_het_ppm=max_het_ppm,
                                               keep_device=bool(keep_device))
        calls, stats, mask, ms = res.calls, res.stats, res.mask, res.ms
        if keep_device:
            d_calls = DeviceCalls(res.d_calls or 0, calls.shape)
    stats = dict(stats, passed=int(mask.sum()), backend=backend, ms=ms, rule=rule, err_ppm=err_ppm, min_depth=min_depth,
                 min_call_ppm=min_call_ppm, min_maf_ppm=min_maf_ppm, max_het_ppm=max_het_ppm)
    return GenoResult(markers, list(samnames), calls, stats, mask, (i0, i1), d_calls)


def _geno_selected(result, passing_only):
    return [m for m in range(len(result.markers)) if result.mask[m] or not passing_only]


def writeGenoCalls(filename, result, passing_only=True):
    """The calls in writeDiploidGeno's layout (samples in rows, markers in columns, csv.writer's CRLF rows): 0 / 1 / 2,
    blank for missing.  passing_only: the markers that pass the filters; False: all of them."""
    import numpy as np
    keep = _geno_selected(result, passing_only)
    rows = np.array(['0', '1', '2', ''])[result.calls[:, keep]].tolist()
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow([""] + [result.markers[m] for m in keep])
        for name, calls in zip(result.samples, rows):
            out.writerow([name] + calls)


def writeMarkerStats(filename, result):
    """One row per marker: name, called, n0, n1, n2, alt, depth0, depth1, pass (1 / 0); CSV with a header row."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(["Marker name"] + list(GENO_STATS) + ["pass"])
        for m, name in enumerate(result.markers):
            out.writerow([name] + [int(result.stats[k][m]) for k in GENO_STATS] + [1 if result.mask[m] else 0])


HAPMAP_HEADER = ("rs#", "alleles", "chrom", "pos", "strand", "assembly#", "center", "protLSID", "assayLSID", "panelLSID",
                 "QCcode")


def writeHapMap(filename, result, tagseqs, passing_only=True):
    """The calls as a HapMap table (tab-separated, LF): rs# the marker name, alleles X/Y from the one base at which the
    marker's two tags differ, chrom 0, pos the marker's 1-based ordinal among the result's markers, strand +, the other
    leading columns NA; then per sample X (code 0), Y (code 2), the IUPAC code of the two (code 1) or N (missing).
    tagseqs: the tag sequences, one per column of the count matrix.  A marker whose tags differ in length or at another
    number of bases than one cannot be written this way: an Exception names it."""
    i0, i1 = result.columns
    lines = ["\t".join(HAPMAP_HEADER + tuple(result.samples))]
    for m in _geno_selected(result, passing_only):
        t0, t1 = tagseqs[i0[m]].upper(), tagseqs[i1[m]].upper()
        sites = [k for k in range(min(len(t0), len(t1))) if t0[k] != t1[k]]
        if len(t0) != len(t1) or len(sites) != 1:
            raise Exception("Marker {}: HapMap output needs two tags of one length that differ at exactly one base."
                            .format(result.markers[m]))
        x, y = t0[sites[0]], t1[sites[0]]
        letters = (x, IUPAC_codes[frozenset(x + y)], y, "N")
        lines.append("\t".join([result.markers[m], x + "/" + y, "0", str(m + 1), "+"] + ["NA"] * 6 +
                               [letters[c] for c in result.calls[:, m].tolist()]))
    with open(filename, mode='w', newline='') as fh:
        fh.write("\n".join(lines) + "\n")


# ---------------------------------------------------------------------------------------------------------------------
# Polyploid allele dosage calls from the count matrix: call_genotypes' sibling for one ploidy P = 2 .. 8.
# Every probability of the model becomes an integer cost, round(-65536 log2 x), in tables that only this module builds
# (fractions for the probabilities, decimal for the logarithm); the rule then adds and compares 64-bit integers.
# call_dosage(backend="host") restates it in numpy, csrc/dosage.hip runs it where the matrix lies.
DOSE_STATS = ("called",) + tuple("n%d" % d for d in range(9)) + ("alt", "depth0", "depth1", "bin")
DOSE_PRIORS = ("flat", "hwe")
DOSE_MAX_PLOIDY = 8
DOSE_BINS = 64
DOSE_COST_MAX = 1 << 23
DOSE_MISSING = 255
_DOSE_TABLES = {}


def _dose_cost(x, digits=60):
    """round_half_even(-65536 log2 x) of a fractions.Fraction 0 < x <= 1, with decimal at `digits` digits."""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = max(50, int(digits))
        bits = -(decimal.Decimal(x.numerator) / decimal.Decimal(x.denominator)).ln() / decimal.Decimal(2).ln()
        return int((bits * 65536).quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_EVEN))


def dosage_tables(ploidy, err, nbins=DOSE_BINS):
    """(CA, CB, CP) for ploidy P and the sequencing error rate e = round(err * 10^6) / 10^6 as an exact rational, all as
    lists of ints, cost(x) = round_half_even(-65536 log2 x):
      CA[d] = cost(p_d), CB[d] = cost(1 - p_d)   p_d = (d (1 - e) + (P - d) e) / P: a read of a cell with d copies of
                                                 allele 1 shows allele 1 (CA) or allele 0 (CB); CA[d] == CB[P - d]
      CP[k][d] = cost(C(P, d) q^d (1 - q)^(P - d))   q = (2 k + 1) / (2 nbins), the centre of bin k of the marker's
                                                 allele-1 read share: Hardy-Weinberg proportions at that frequency
    Pure Python (fractions, decimal at 60 digits): the same on every machine."""
    from fractions import Fraction
    from math import comb
    P = int(ploidy)
    if P != ploidy or not 2 <= P <= DOSE_MAX_PLOIDY:
        raise ValueError("ploidy must be an integer in 2 .. {}".format(DOSE_MAX_PLOIDY))
    if int(nbins) != nbins or nbins < 1:
        raise ValueError("nbins must be a positive integer")
    key = (P, _ppm(err, 1, 499999, "err"), int(nbins))
    if key not in _DOSE_TABLES:
        e = Fraction(key[1], 1000000)
        p = [(d * (1 - e) + (P - d) * e) / P for d in range(P + 1)]
        CA = tuple(_dose_cost(x) for x in p)
        CB = tuple(_dose_cost(1 - x) for x in p)
        assert all(CA[d] == CB[P - d] for d in range(P + 1))
        CP = []
        for k in range(key[2]):
            q = Fraction(2 * k + 1, 2 * key[2])
            CP.append(tuple(_dose_cost(comb(P, d) * q ** d * (1 - q) ** (P - d)) for d in range(P + 1)))
        _DOSE_TABLES[key] = (CA, CB, tuple(CP))
    CA, CB, CP = _DOSE_TABLES[key]
    return list(CA), list(CB), [list(row) for row in CP]


def dosage_margin(min_odds):
    """round(65536 log2 min_odds): the least cost margin (units of 2^-16 bit) between the best and the second-best
    dosage at which the best is min_odds times as probable.  min_odds >= 1."""
    from fractions import Fraction
    odds = Fraction(min_odds)
    if odds < 1:
        raise ValueError("min_odds must be at least 1")
    margin = _dose_cost(1 / odds)
    if margin > 0xffffffff:
        raise ValueError("min_odds is too large: the margin must fit 32 bits")
    return margin


class DosageResult:
    """What call_dosage returns: `.markers`, `.samples`, `.ploidy`, `.calls` (uint8 [samples, markers]: copies of allele
    1, 0 .. ploidy, 255 = missing), `.diploid` (uint8: 0 for dosage 0, 2 for dosage ploidy, 1 between, 3 = missing -- what
    sample_relations, marker_ld, impute_calls and parentage read), `.stats` (called, n0 .. n8, alt, depth0, depth1, bin as
    arrays over the markers; passed, backend, ms and the parameters), `.mask` (bool per marker: it passes the filters),
    `.columns`, `.backend`, `.d_diploid` (call_dosage(keep_device=True) on the gpu backend: a DeviceCalls of the
    diploidised matrix where the kernel wrote it, which the caller frees; else None)."""

    def __init__(self, markers, samples, ploidy, calls, diploid, stats, mask, columns, backend, d_diploid=None):
        self.markers, self.samples, self.ploidy, self.calls, self.diploid = markers, samples, ploidy, calls, diploid
        self.stats, self.mask, self.columns, self.backend, self.d_diploid = stats, mask, columns, backend, d_diploid


def _dosage_host(counts, i0, i1, ploidy, CA, CB, CP, min_depth, min_margin, min_call_ppm, min_maf_ppm):
    """The rule of DESIGN 4.23 in numpy's uint64, which holds every intermediate exactly: a cost stays below 2^57,
    64 depth1 below 2^63 for at most 2^24 samples.  CP None: the flat prior.  Returns (calls, diploid, stats, mask)."""
    import numpy as np
    S, M, P = counts.shape[0], len(i0), int(ploidy)
    if S > 1 << 24:
        raise ValueError("more than 2^24 samples")
    a = counts[:, i0].astype(np.uint64)
    b = counts[:, i1].astype(np.uint64)
    depth0, depth1 = a.sum(axis=0, dtype=np.uint64), b.sum(axis=0, dtype=np.uint64)
    tot = depth0 + depth1
    bins = np.where(tot == 0, 0, np.minimum(np.uint64(DOSE_BINS - 1), np.uint64(DOSE_BINS) * depth1 // np.where(tot == 0, 1, tot))).astype(np.int64)
    prior = np.zeros((P + 1, M), dtype=np.uint64) if CP is None else np.asarray(CP, dtype=np.uint64)[bins].T.copy()

    def cost(d):
        return b * np.uint64(CA[d]) + a * np.uint64(CB[d]) + prior[d][None, :]
    best, second = cost(0), np.full((S, M), ~np.uint64(0), dtype=np.uint64)
    code = np.zeros((S, M), dtype=np.uint8)
    for d in range(1, P + 1):
        c = cost(d)
        lead = c < best                               # strict: among equal costs the smallest d stays best
        second = np.minimum(second, np.where(lead, best, c))
        best = np.where(lead, c, best)
        code[lead] = d
    missing = (a + b < np.uint64(min_depth)) | (second - best < np.uint64(min_margin))
    calls = np.where(missing, DOSE_MISSING, code).astype(np.uint8)
    diploid = np.where(missing, GENO_MISSING, np.where(code == 0, 0, np.where(code == P, 2, 1))).astype(np.uint8)
    n = [(calls == d).sum(axis=0, dtype=np.uint64) for d in range(9)]
    called = sum(n[1:], n[0])
    alt = sum((np.uint64(d) * n[d] for d in range(1, 9)), np.zeros(M, dtype=np.uint64))
    million = np.uint64(1000000)
    mask = ((called * million >= np.uint64(min_call_ppm * S)) &
            (np.minimum(alt, np.uint64(P) * called - alt) * million >= np.uint64(min_maf_ppm * P) * called))
    if S == 0:
        mask[:] = False                               # no sample: no marker passes on no evidence
    stats = dict(zip(DOSE_STATS, [called] + n + [alt, depth0, depth1, bins.astype(np.uint64)]))
    return calls, diploid, stats, mask


def call_dosage(counts, samnames, tagnames, ploidy=4, prior="hwe", err=0.01, min_depth=1, min_odds=10, min_call_rate=0.0,
                min_maf=0.0, device=0, backend="gpu", keep_device=False, min_margin=None):
    """Allele dosage calls of polyploid samples from a samples x tags count matrix, and which markers pass the filters
    (DESIGN 4.23).  Every sample carries `ploidy` copies (2 .. 8) of each marker; a call is the number of copies of
    allele 1, 0 .. ploidy.

    Markers and alleles come from the tag names as call_genotypes reads them.  For a sample's counts a and b of the two
    alleles the cost of dosage d is b CA[d] + a CB[d] + CP[bin][d] in the integer tables of dosage_tables(ploidy, err):
    minus log2 of the binomial likelihood of the reads with error rate err, and of the prior.  prior="hwe": Hardy-Weinberg
    proportions at the marker's allele-1 read share over all samples, in 64 bins; prior="flat": none.  The call is the
    cheapest dosage (the lower one of equals) when the second cheapest costs at least dosage_margin(min_odds) more -- it is
    min_odds times as probable --, else missing (255); a cell with a + b < min_depth is missing too.  min_margin, when
    given, replaces dosage_margin(min_odds).  A marker passes when called / samples >= min_call_rate and its minor allele
    frequency among the called copies >= min_maf, compared as integers in parts per million.
    counts: a numpy matrix or lists (uint32 values), or a DeviceCounts (backend="gpu" only).  backend="gpu" runs
    csrc/dosage.hip on the matrix where it lies; backend="host" is the numpy restatement.  keep_device=True with the gpu
    backend leaves the diploidised calls on the device as well: `.d_diploid` is a DeviceCalls for sample_relations,
    marker_ld, impute_calls and parentage, and the caller's to free.  Returns a DosageResult."""
    import numpy as np
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    if prior not in DOSE_PRIORS:
        raise ValueError("prior must be 'flat' or 'hwe'")
    err_ppm = _ppm(err, 1, 499999, "err")
    CA, CB, CP = dosage_tables(ploidy, err_ppm / 1e6)
    ploidy = int(ploidy)
    if int(min_depth) != min_depth or min_depth < 1:
        raise ValueError("min_depth must be an integer of at least 1")
    min_depth = int(min_depth)
    if min_margin is None:
        min_margin = dosage_margin(min_odds)
    if int(min_margin) != min_margin or not 0 <= min_margin <= 0xffffffff:
        raise ValueError("min_margin must be an integer in 0 .. 2^32 - 1")
    min_margin = int(min_margin)
    min_call_ppm = _ppm(min_call_rate, 0, 1000000, "min_call_rate")
    min_maf_ppm = _ppm(min_maf, 0, 500000, "min_maf")
    on_device = isinstance(counts, DeviceCounts)
    if on_device and backend != "gpu":
        raise ValueError("a DeviceCounts matrix needs backend='gpu'")
    if not on_device:
        from .engine import counts_as_uint32
        counts = counts_as_uint32(counts if len(counts) else np.zeros((0, len(tagnames)), dtype=np.uint32))
    assert len(samnames) == counts.shape[0], "Length of samnames should be the same as length of counts."
    assert len(tagnames) == counts.shape[1], "Length of tagnames should be length of second dimension of counts."
    markers, i0, i1 = _geno_markers(tagnames)
    d_diploid = None
    if backend == "host":
        calls, diploid, stats, mask = _dosage_host(counts, i0, i1, ploidy, CA, CB, CP if prior == "hwe" else None, min_depth,
                                                   min_margin, min_call_ppm, min_maf_ppm)
        ms = 0.0
    else:
        res = default_engine(device).dose_call(counts.ptr if on_device else counts, i0, i1, CA, CB, CP if prior == "hwe" else None,
                                               shape=counts.shape if on_device else None, ploidy=ploidy,
                                               prior=DOSE_PRIORS.index(prior), err_ppm=err_ppm, min_depth=min_depth,
                                               min_margin=min_margin, min_call_ppm=min_call_ppm, min_maf_ppm=min_maf_ppm,
                                               diploid=True, keep_diploid=bool(keep_device))
        calls, diploid, stats, mask, ms = res.calls, res.diploid, res.stats, res.mask, res.ms
        if keep_device:
            d_diploid = DeviceCalls(res.d_diploid or 0, calls.shape)
    stats = dict(stats, passed=int(mask.sum()), backend=backend, ms=ms, ploidy=ploidy, prior=prior, err_ppm=err_ppm,
                 min_depth=min_depth, min_margin=min_margin, min_call_ppm=min_call_ppm, min_maf_ppm=min_maf_ppm)
    return DosageResult(markers, list(samnames), ploidy, calls, diploid, stats, mask, (i0, i1), backend, d_diploid)


def writeDosage(filename, result, passing_only=True):
    """The dosages in writeGenoCalls' layout (samples in rows, markers in columns, csv.writer's CRLF rows): 0 .. ploidy,
    blank for missing.  passing_only: the markers that pass the filters; False: all of them."""
    import numpy as np
    keep = _geno_selected(result, passing_only)
    text = np.array([str(d) for d in range(DOSE_MISSING)] + [''])
    rows = text[result.calls[:, keep]].tolist()
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow([""] + [result.markers[m] for m in keep])
        for name, calls in zip(result.samples, rows):
            out.writerow([name] + calls)


def writeDosageStats(filename, result):
    """One row per marker: name, called, n0 .. n<ploidy>, alt, depth0, depth1, bin, pass (1 / 0); CSV with a header row."""
    cols = [k for k in DOSE_STATS if not (k[0] == "n" and int(k[1:]) > result.ploidy)]
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(["Marker name"] + cols + ["pass"])
        for m, name in enumerate(result.markers):
            out.writerow([name] + [int(result.stats[k][m]) for k in cols] + [1 if result.mask[m] else 0])


# ---------------------------------------------------------------------------------------------------------------------
# VCF export: the calls with both read depths of every cell, GT:AD:DP and optionally GQ:PL, in the one
# format every downstream tool reads.  Python writes the header and builds every line's first nine columns; the cells
# -- a transpose of the sample-major matrices into variable-width text -- are formatted by csrc/vcf.hip from the count
# matrix and the calls where they lie, or by numpy here (backend="host"), byte for byte the same.
VCF_FIXED = ("#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT")
VCF_HOST_BLOCK = 2048        # lines the host backend formats at a time


def _vcf_position(name, positions):
    """(chrom, pos) of a marker: from its name chrom-pos-strand (positions="names") or from the dict."""
    if positions == "names":
        parts = name.rsplit("-", 2)
        if len(parts) != 3 or not parts[0] or not parts[1].isdigit():
            raise Exception("Marker {}: its name does not read as chrom-pos-strand.".format(name))
        return parts[0], int(parts[1])
    if name not in positions:
        raise Exception("Marker {}: no position given.".format(name))
    chrom, pos = positions[name]
    return str(chrom), int(pos)


def _vcf_lines(result, tagseqs, positions, passing_only, ploidy, fmt):
    """(marker index per line, prefix bytes per line, chromosomes in first-seen order or None): the lines in writing order
    with their eight fixed columns and FORMAT."""
    keep = _geno_selected(result, passing_only)
    i0, i1 = result.columns
    chroms = None
    if positions is None:
        where = {m: ("0", m + 1) for m in keep}
    else:
        where = {m: _vcf_position(result.markers[m], positions) for m in keep}
        chroms = []
        for m in keep:
            if where[m][0] not in chroms:
                chroms.append(where[m][0])
        rank = {c: k for k, c in enumerate(chroms)}
        keep = sorted(keep, key=lambda m: (rank[where[m][0]], where[m][1], m))
    stats = result.stats
    prefixes = []
    for m in keep:
        ref, alt = "N", "<ALLELE1>"
        if tagseqs is not None:
            t0, t1 = tagseqs[i0[m]].upper(), tagseqs[i1[m]].upper()
            sites = [k for k in range(min(len(t0), len(t1))) if t0[k] != t1[k]]
            if len(t0) == len(t1) and len(sites) == 1:
                ref, alt = t0[sites[0]], t1[sites[0]]
        called = int(stats["called"][m])
        info = "NS={};DP={};AC={};AN={}".format(called, int(stats["depth0"][m]) + int(stats["depth1"][m]), int(stats["alt"][m]),
                                                ploidy * called)
        prefixes.append("\t".join([where[m][0], str(where[m][1]), result.markers[m], ref, alt, ".",
                                   "PASS" if result.mask[m] else "filtered", info, fmt]).encode("utf-8"))
    return keep, prefixes, chroms


def _vcf_header(result, chroms, likelihoods, any_symbolic, any_filtered):
    lines = ["##fileformat=VCFv4.2", "##source=tagdigger_amd"]
    lines += ["##contig=<ID={}>".format(c) for c in chroms or []]
    lines += ['##INFO=<ID=NS,Number=1,Type=Integer,Description="Samples with a call">',
              '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads of both alleles over all samples">',
              '##INFO=<ID=AC,Number=A,Type=Integer,Description="Copies of allele 1 among the calls">',
              '##INFO=<ID=AN,Number=1,Type=Integer,Description="Allele copies among the calls">']
    if any_filtered:
        lines.append('##FILTER=<ID=filtered,Description="Outside the call rate, allele frequency or heterozygosity filters">')
    lines += ['##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
              '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads of allele 0 and of allele 1">',
              '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Reads of both alleles">']
    if likelihoods:
        lines += ['##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: the smallest PL of another genotype, at most 99">',
                  '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods, at most 255">']
    if any_symbolic:
        lines.append('##ALT=<ID=ALLELE1,Description="The second tag of a marker whose tags are not one base apart">')
    lines.append("\t".join(VCF_FIXED + tuple(result.samples)))
    return ("\n".join(lines) + "\n").encode("utf-8")


def _vcf_cells_host(a, b, code, ploidy, likelihoods, CA, CB):
    """The cells of DESIGN 4.25 as a numpy array of strings, shaped like a, b (uint64) and code."""
    import numpy as np
    P = ploidy
    gts = np.array(["/".join(["0"] * (P - c) + ["1"] * c) for c in range(P + 1)] + ["/".join(["."] * P)])
    add = np.char.add
    n = a + b
    text = add(add(add(add(add(gts[np.minimum(code, P + 1)], ":"), a.astype(str)), ","), add(b.astype(str), ":")), n.astype(str))
    if likelihoods:
        deep = n > 127
        div = np.where(deep, n, 1)
        x = np.where(deep, 127 * a // div, a)
        y = np.where(deep, 127 * b // div, b)
        cost = [y * np.uint64(CA[g]) + x * np.uint64(CB[g]) for g in range(3)]
        cmin = np.minimum(np.minimum(cost[0], cost[1]), cost[2])
        pl = [np.minimum(((c - cmin) * np.uint64(30103) + np.uint64(327680000)) // np.uint64(655360000), 255) for c in cost]
        gq = np.full(a.shape, 99, dtype=np.uint64)
        for g in range(3):
            gq = np.where(code != g, np.minimum(gq, pl[g]), gq)
        lik = add(add(add(add(gq.astype(str), ":"), add(pl[0].astype(str), ",")), add(pl[1].astype(str), ",")), pl[2].astype(str))
        text = add(add(text, ":"), np.where(code > 2, ".:.", lik))
    return text


def writeVCF(filename, result, counts, tagseqs=None, positions=None, passing_only=True, likelihoods=False, err=0.01,
             range_bytes=None, device=0, backend="gpu"):
    """The calls as a VCF 4.2 file with both read depths of every cell.

    result: a GenoResult (ploidy 2) or a DosageResult; counts: the matrix it was called from, a numpy matrix or a
    DeviceCounts (backend="gpu" only).  One line per marker that passes (passing_only=False: every marker, FILTER
    `filtered` for those outside the mask), cells GT:AD:DP: GT the dosage as P alleles (0/0/1/1; ./. for missing), AD the
    reads of allele 0 and allele 1, DP their sum.  likelihoods=True (ploidy 2) adds GQ:PL from the integer costs of
    dosage_tables(2, err): PL[g] = round(3.0103 (cost[g] - min cost) / 65536), at most 255, over the depths scaled to 127 as
    the likelihood rule scales them; GQ the smallest PL of another genotype than the call, at most 99.
    CHROM and POS: positions=None gives writeHapMap's chrom 0 and the marker's 1-based ordinal; positions="names" reads
    marker names chrom-pos-strand (readTags_TASSELSAM, tag_place); a dict maps marker name -> (chrom, pos).  With
    positions the lines are sorted by (chromosome in first-seen order, pos, marker index).  REF / ALT are the two bases
    where tagseqs (one sequence per column of counts) shows two tags of one length that differ at exactly one base, else N
    and <ALLELE1>.  INFO holds NS, DP, AC and AN from the result's statistics.
    backend="gpu": the header is written here, the body by csrc/vcf.hip from the matrix and the calls on the device
    (`result.d_calls` where call_genotypes kept them), in ranges of about range_bytes (default 256 MiB) that are written
    while the next one is formatted.  backend="host": the same bytes from numpy.  Returns a dict: lines, bytes (of the
    body), ranges and ms (gpu)."""
    import numpy as np
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    ploidy = int(getattr(result, "ploidy", 2))
    if likelihoods and ploidy != 2:
        raise ValueError("likelihoods (GQ:PL) are written for ploidy 2 only")
    on_device = isinstance(counts, DeviceCounts)
    if on_device and backend != "gpu":
        raise ValueError("a DeviceCounts matrix needs backend='gpu'")
    if not on_device:
        from .engine import counts_as_uint32
        counts = counts_as_uint32(counts if len(counts) else np.zeros((0, 0), dtype=np.uint32))
    S, M = len(result.samples), len(result.markers)
    if counts.shape[0] != S:
        raise ValueError("counts has {} rows, the result {} samples".format(counts.shape[0], S))
    CA = CB = None
    if likelihoods:
        CA, CB, _ = dosage_tables(2, _ppm(err, 1, 499999, "err") / 1e6)
    fmt = "GT:AD:DP:GQ:PL" if likelihoods else "GT:AD:DP"
    keep, prefixes, chroms = _vcf_lines(result, tagseqs, positions, passing_only, ploidy, fmt)
    header = _vcf_header(result, chroms, likelihoods, any(b"\t<ALLELE1>\t" in p for p in prefixes),
                         any(not result.mask[m] for m in keep))
    i0, i1 = (np.asarray(c, dtype=np.int64) for c in result.columns)
    with open(filename, "wb") as fh:
        fh.write(header)
        if backend == "host":
            nbytes = 0
            for lo in range(0, len(keep), VCF_HOST_BLOCK):
                sel = np.asarray(keep[lo:lo + VCF_HOST_BLOCK], dtype=np.int64)
                cells = _vcf_cells_host(counts[:, i0[sel]].astype(np.uint64), counts[:, i1[sel]].astype(np.uint64),
                                        np.asarray(result.calls)[:, sel], ploidy, likelihoods, CA, CB)
                block = b"".join(prefixes[lo + j] + b"".join(b"\t" + c.encode("ascii") for c in cells[:, j].tolist()) + b"\n"
                                 for j in range(len(sel)))
                fh.write(block)
                nbytes += len(block)
            return dict(lines=len(keep), bytes=nbytes, ranges=None, ms=None, backend="host")
    d_calls = getattr(result, "d_calls", None)
    calls = d_calls.ptr if d_calls is not None and d_calls.ptr else np.ascontiguousarray(result.calls, dtype=np.uint8)
    res = default_engine(device).vcf_file(filename, counts.ptr if on_device else counts, calls, i0, i1, keep, prefixes,
                                          shape=counts.shape if on_device else None, ploidy=ploidy, likelihoods=likelihoods,
                                          ca=CA, cb=CB, range_bytes=range_bytes or 0, append=True)
    return dict(lines=len(keep), bytes=res.nbytes, ranges=res.ranges, ms=res.ms, backend="gpu")


# ---------------------------------------------------------------------------------------------------------------------
# Pairwise sample relations from the calls: the step behind the calls.  Everything is a function of one
# table, joint[i][j][a][b] = the participating markers at which sample i is called a and sample j is called b; it is
# exact in integers.  csrc/relate.hip computes it on the matrix cores from the calls where they lie, _relations_host
# restates it in numpy.  Floats appear only in .distance and .kinship.
RELATE_MAX_SAMPLES = 16384


class DeviceCalls:
    """A samples x markers uint8 call matrix in device memory (what call_genotypes(keep_device=True) leaves there), for
    sample_relations(backend="gpu"): `ptr` a device pointer (0: no buffer, an empty matrix), `shape` = (samples,
    markers)."""

    def __init__(self, ptr, shape):
        self.ptr, self.shape = int(ptr), (int(shape[0]), int(shape[1]))

    def __len__(self):
        return self.shape[0]


class RelationResult:
    """What sample_relations returns: `.samples`, `.joint` (uint32 [S, S, 3, 3]) and, as int64 [S, S] arrays over the
    ordered pairs, `.shared` (markers called in both), `.ibs0`, `.ibs1`, `.ibs2`, `.hethet`, `.het_i`, `.het_j`, `.dist`
    (= ibs1 + 2 ibs0); `.distance` = dist / (2 shared) and `.kinship` = (hethet - 2 ibs0) / (het_i + het_j) as float64
    with nan where the denominator is 0; `.duplicates` (list of (i, j), i < j); `.stats` (backend, ms, markers, used,
    max_dist_ppm, min_shared)."""

    def __init__(self, samples, joint, max_dist_ppm, min_shared, stats):
        import numpy as np
        J = joint.astype(np.int64)
        self.samples, self.joint = samples, joint
        self.shared = J.sum(axis=(2, 3))
        self.ibs0 = J[:, :, 0, 2] + J[:, :, 2, 0]
        self.ibs2 = J[:, :, 0, 0] + J[:, :, 1, 1] + J[:, :, 2, 2]
        self.ibs1 = self.shared - self.ibs0 - self.ibs2
        self.hethet = J[:, :, 1, 1].copy()
        self.het_i = J[:, :, 1, :].sum(axis=2)
        self.het_j = J[:, :, :, 1].sum(axis=2)
        self.dist = self.ibs1 + 2 * self.ibs0
        with np.errstate(divide="ignore", invalid="ignore"):
            self.distance = np.where(self.shared > 0, self.dist / (2.0 * self.shared), np.nan)
            het = self.het_i + self.het_j
            self.kinship = np.where(het > 0, (self.hethet - 2 * self.ibs0) / het.astype(np.float64), np.nan)
        # the duplicate rule in integers: dist <= 2^32 and 10^6 < 2^20, so every product stays below 2^53
        flagged = (self.shared >= min_shared) & (self.dist * 1000000 <= max_dist_ppm * 2 * self.shared)
        self.duplicates = [(int(i), int(j)) for i, j in zip(*np.nonzero(np.triu(flagged, 1)))]
        self.stats = dict(stats, max_dist_ppm=max_dist_ppm, min_shared=min_shared)


def _relations_host(calls, use=None):
    """joint[i][j][a][b] of DESIGN 4.15 in numpy: the Gram product of the one-hot planes, in float32 over blocks of
    markers short enough to be exact there (< 2^24), summed in int64."""
    import numpy as np
    calls = np.asarray(calls, dtype=np.uint8)
    S, M = calls.shape
    total = np.zeros((3 * S, 3 * S), dtype=np.int64)
    cols = np.arange(M) if use is None else np.nonzero(np.asarray(use) != 0)[0]
    block = max(1, min((1 << 24) - 1, (1 << 26) // max(1, 3 * S)))
    for lo in range(0, len(cols), block):
        part = calls[:, cols[lo:lo + block]]
        X = np.stack([part == a for a in (0, 1, 2)], axis=1).reshape(3 * S, -1).astype(np.float32)
        total += np.rint(X @ X.T).astype(np.int64)
    return total.reshape(S, 3, S, 3).transpose(0, 2, 1, 3).astype(np.uint32)


def sample_relations(calls, samnames, mask=None, max_dist=0.02, min_shared=50, device=0, backend="gpu"):
    """Pairwise relations of the samples from their genotype calls: are two wells the same plant, was a
    sample swapped, which samples are relatives.

    calls: a samples x markers matrix of codes 0, 1, 2 (copies of allele 1) and 3 (missing) -- numpy or lists -- or a
    DeviceCalls (backend="gpu" only; there any byte above 2 is missing).  mask: one entry per marker, a marker takes
    part iff its entry is true (None: all) -- call_genotypes' `.mask` restricts the relations to the markers that pass.
    For every pair the 3 x 3 table of how often call a in one sample meets call b in the other is counted; the IBS
    counts, the IBS distance dist / (2 shared) and the KING-robust kinship (hethet - 2 ibs0) / (het_i + het_j) follow
    from it.  A pair i < j is a duplicate iff shared >= min_shared and dist * 10^6 <= max_dist_ppm * 2 * shared, in
    integers (max_dist is taken in parts per million).  backend="gpu" runs csrc/relate.hip on the calls where they lie;
    backend="host" is the numpy restatement.  Returns a RelationResult."""
    import numpy as np
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    max_dist_ppm = _ppm(max_dist, 0, 1000000, "max_dist")
    if isinstance(min_shared, bool) or int(min_shared) != min_shared or min_shared < 0:
        raise ValueError("min_shared must be an integer of at least 0")
    min_shared = int(min_shared)
    on_device = isinstance(calls, DeviceCalls)
    if on_device and backend != "gpu":
        raise ValueError("a DeviceCalls matrix needs backend='gpu'")
    samnames = list(samnames)
    if not on_device:
        calls = np.asarray(calls if len(calls) else np.zeros((0, 0 if mask is None else len(mask)), dtype=np.uint8))
        if calls.ndim != 2:
            raise ValueError("the call matrix must have two dimensions (samples x markers)")
        if calls.dtype.kind not in "iub":
            raise ValueError("the call matrix must hold the integer codes 0 .. 3, not {}".format(calls.dtype))
        if calls.size and (int(calls.min()) < 0 or int(calls.max()) > 3):
            raise ValueError("the call matrix must hold 0, 1, 2 or 3 (missing) only")
        calls = np.ascontiguousarray(calls, dtype=np.uint8)
    S, M = calls.shape
    if len(samnames) != S:
        raise ValueError("samnames must name every row of the call matrix")
    if S > RELATE_MAX_SAMPLES:
        raise ValueError("at most {} samples".format(RELATE_MAX_SAMPLES))
    if M >= 1 << 31:
        raise ValueError("markers must number below 2^31")
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (M,):
            raise ValueError("mask must have one entry per marker")
        mask = mask != 0
    if backend == "host":
        joint, ms = _relations_host(calls, mask), 0.0
    else:
        res = default_engine(device).relate_joint(calls.ptr or None if on_device else calls,
                                                  shape=(S, M) if on_device else None, use=mask)
        joint, ms = res.joint, res.ms
    used = M if mask is None else int(mask.sum())
    return RelationResult(samnames, joint, max_dist_ppm, min_shared, dict(backend=backend, ms=ms, markers=M, used=used))


RELATION_COLUMNS = ("sample_i", "sample_j", "shared", "ibs0", "ibs1", "ibs2", "hethet", "het_i", "het_j", "distance",
                    "kinship", "duplicate")


def _na(x):
    return "NA" if x != x else format(x, ".6f")


def writeRelations(filename, result):
    """One row per pair of samples i < j: the names, shared, ibs0, ibs1, ibs2, hethet, het_i, het_j, distance and
    kinship (six decimals, NA where undefined) and duplicate (1 / 0); CSV with a header row, csv.writer's CRLF rows."""
    dups = set(result.duplicates)
    S = len(result.samples)
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(RELATION_COLUMNS)
        for i in range(S):
            for j in range(i + 1, S):
                out.writerow([result.samples[i], result.samples[j]] +
                             [int(getattr(result, k)[i, j]) for k in RELATION_COLUMNS[2:9]] +
                             [_na(float(result.distance[i, j])), _na(float(result.kinship[i, j])), 1 if (i, j) in dups else 0])


def writeDistanceMatrix(filename, result):
    """The samples x samples IBS distances (six decimals, NA where two samples share no called marker): the sample
    names in the header row and the first column; CSV, csv.writer's CRLF rows."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow([""] + list(result.samples))
        for i, name in enumerate(result.samples):
            out.writerow([name] + [_na(float(x)) for x in result.distance[i]])


# ---------------------------------------------------------------------------------------------------------------------
# Pairwise marker LD from the calls: the check of the markers against each other.  For two participating
# markers i < j, over the samples called at both: n, sx, sy, sxx, syy, sxy; cov = n sxy - sx sy, var_i = n sxx - sx^2,
# var_j = n syy - sy^2.  The pair is an edge iff n >= min_shared, var_i > 0, var_j > 0 and cov^2 10^6 >= min_r2_ppm var_i
# var_j -- integers only, the two sides as 128-bit values.  csrc/ld.hip decides it on the matrix cores from the calls
# where they lie, _ld_host restates it in numpy.  Floats appear only in .r2.
LD_MAX_SAMPLES = 16384
LD_MAX_MARKERS = 1 << 20
LD_EDGE = [("i", "<u4"), ("j", "<u4"), ("shared", "<u4"), ("cov", "<i4"), ("var_i", "<u4"), ("var_j", "<u4")]
_LD_HOST_CELLS = 1 << 21    # pairs of one block of _ld_host: a dozen int64 arrays of this size at a time


class LDResult:
    """What marker_ld returns: `.markers` (all M names), `.mask` (bool [M]: the marker takes part), `.edges` (structured
    array i, j, shared, cov, var_i, var_j; i < j in the numbering of `.markers`, ascending by (i, j)), `.r2` (float64 per
    edge, cov^2 / (var_i var_j)), `.phase` (int8 per edge, +1 / -1: the sign of cov; 0 only where min_r2 = 0 lets a pair
    with cov = 0 in), `.degree` and `.called` (uint32 [M]; 0 for markers that do not take part), `.stats` (backend, ms,
    markers, used, edges, min_r2_ppm, min_shared)."""

    def __init__(self, markers, mask, edges, degree, called, stats):
        import numpy as np
        self.markers, self.mask, self.edges, self.degree, self.called = markers, mask, edges, degree, called
        # cov^2 and var_i var_j pass 2^53: the quotient of Python's integers is the correctly rounded one
        self.r2 = np.array([c * c / (a * b) for c, a, b in zip(edges["cov"].tolist(), edges["var_i"].tolist(),
                                                                 edges["var_j"].tolist())], dtype=np.float64)
        self.phase = np.sign(edges["cov"]).astype(np.int8)
        self.stats = dict(stats, edges=len(edges))


def _ld_wide(a, k):
    """a * k as two uint64 words (high, low 32 bits) for a < 2^57 and k <= 2^20: nothing wraps."""
    import numpy as np
    t = (a & np.uint64(0xffffffff)) * np.uint64(k)
    return (a >> np.uint64(32)) * np.uint64(k) + (t >> np.uint64(32)), t & np.uint64(0xffffffff)


def _ld_host(calls, use, min_r2_ppm, min_shared):
    """The rule of DESIGN 4.16 in numpy, over blocks of markers: the six sums as float32 products (at most 4 * 16384,
    exact there), everything after them in 64-bit integers, the comparison on two words.  Returns (edges ascending by
    (i, j), degree, called)."""
    import numpy as np
    calls = np.asarray(calls, dtype=np.uint8)
    S, M = calls.shape
    cols = np.arange(M) if use is None else np.nonzero(np.asarray(use) != 0)[0]
    part = calls[:, cols]
    ok = part <= 2
    C = ok.astype(np.float32)
    X = np.where(ok, part, 0).astype(np.float32)
    Q = X * X
    called = np.zeros(M, dtype=np.uint32)
    called[cols] = ok.sum(axis=0)
    degree = np.zeros(M, dtype=np.uint32)
    Mp = len(cols)
    found = []
    block = max(1, _LD_HOST_CELLS // max(1, Mp))
    for lo in range(0, Mp if S else 0, block):
        hi = min(Mp, lo + block)
        Cb, Xb, Qb = C[:, lo:hi].T, X[:, lo:hi].T, Q[:, lo:hi].T

        def gram(a, b):
            return np.rint(a @ b[:, lo:]).astype(np.int64)

        n, sx, sy, sxy, sxx, syy = gram(Cb, C), gram(Xb, C), gram(Cb, X), gram(Xb, X), gram(Qb, C), gram(Cb, Q)
        cov, var_i, var_j = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
        lhs_hi, lhs_lo = _ld_wide((cov * cov).astype(np.uint64), 1000000)
        rhs_hi, rhs_lo = _ld_wide((var_i * var_j).astype(np.uint64), min_r2_ppm)
        edge = (n >= min_shared) & (var_i > 0) & (var_j > 0) & ((lhs_hi > rhs_hi) | ((lhs_hi == rhs_hi) & (lhs_lo >= rhs_lo)))
        edge &= np.arange(lo, Mp)[None, :] > np.arange(lo, hi)[:, None]                # i < j
        bi, bj = np.nonzero(edge)                                                      # row-major: ascending (i, j)
        rec = np.zeros(len(bi), dtype=LD_EDGE)
        rec["i"], rec["j"] = cols[bi + lo], cols[bj + lo]
        for name, a in (("shared", n), ("cov", cov), ("var_i", var_i), ("var_j", var_j)):
            rec[name] = a[bi, bj]
        found.append(rec)
    edges = np.concatenate(found) if found else np.zeros(0, dtype=LD_EDGE)
    if len(edges):
        degree += np.bincount(edges["i"], minlength=M).astype(np.uint32) + np.bincount(edges["j"], minlength=M).astype(np.uint32)
    return edges, degree, called


def marker_ld(calls, marknames, mask=None, min_r2=0.8, min_shared=50, device=0, backend="gpu"):
    """Pairwise LD of the markers from the genotype calls: which markers are redundant, which co-segregate,
    which were made twice.

    calls: a samples x markers matrix of codes 0, 1, 2 (copies of allele 1) and 3 (missing) -- numpy or lists -- or a
    DeviceCalls (backend="gpu" only; there any byte above 2 is missing).  mask: one entry per marker, a marker takes
    part iff its entry is true (None: all).  A pair of participating markers i < j is an edge iff at least min_shared
    samples are called at both, both vary among those samples and r^2 = cov^2 / (var_i var_j) >= min_r2, compared in
    integers (min_r2 is taken in parts per million).  backend="gpu" runs csrc/ld.hip on the calls where they lie;
    backend="host" is the numpy restatement: the same edges in the same order.  Returns an LDResult."""
    import numpy as np
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    min_r2_ppm = _ppm(min_r2, 0, 1000000, "min_r2")
    if isinstance(min_shared, bool) or int(min_shared) != min_shared or not 0 <= min_shared < 1 << 32:
        raise ValueError("min_shared must be an integer of at least 0")
    min_shared = int(min_shared)
    on_device = isinstance(calls, DeviceCalls)
    if on_device and backend != "gpu":
        raise ValueError("a DeviceCalls matrix needs backend='gpu'")
    marknames = list(marknames)
    if not on_device:
        calls = np.asarray(calls if len(calls) else np.zeros((0, len(marknames)), dtype=np.uint8))
        if calls.ndim != 2:
            raise ValueError("the call matrix must have two dimensions (samples x markers)")
        if calls.dtype.kind not in "iub":
            raise ValueError("the call matrix must hold the integer codes 0 .. 3, not {}".format(calls.dtype))
        if calls.size and (int(calls.min()) < 0 or int(calls.max()) > 3):
            raise ValueError("the call matrix must hold 0, 1, 2 or 3 (missing) only")
        calls = np.ascontiguousarray(calls, dtype=np.uint8)
    S, M = calls.shape
    if len(marknames) != M:
        raise ValueError("marknames must name every column of the call matrix")
    if S > LD_MAX_SAMPLES:
        raise ValueError("at most {} samples".format(LD_MAX_SAMPLES))
    if M >= 1 << 31:
        raise ValueError("markers must number below 2^31")
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (M,):
            raise ValueError("mask must have one entry per marker")
        mask = mask != 0
    used = M if mask is None else int(mask.sum())
    if used > LD_MAX_MARKERS:
        raise ValueError("{} participating markers, at most {}".format(used, LD_MAX_MARKERS))
    if backend == "host":
        (edges, degree, called), ms = _ld_host(calls, mask, min_r2_ppm, min_shared), 0.0
    else:
        res = default_engine(device).ld_pairs(calls.ptr or None if on_device else calls, shape=(S, M) if on_device else None,
                                              use=mask, min_r2_ppm=min_r2_ppm, min_shared=min_shared)
        edges, degree, called, ms = res.edges, res.degree, res.called, res.ms
    return LDResult(marknames, np.ones(M, dtype=bool) if mask is None else mask, edges, degree, called,
                    dict(backend=backend, ms=ms, markers=M, used=used, min_r2_ppm=min_r2_ppm, min_shared=min_shared))


def _edge_components(M, edges):
    """int64 [M]: for every marker the smallest marker of its connected component under the edges (fields i and j)."""
    import numpy as np
    label = np.arange(M, dtype=np.int64)
    ei, ej = edges["i"].astype(np.int64), edges["j"].astype(np.int64)
    while len(ei):                                 # every marker takes the smallest label around it, then its label's label
        new = label.copy()
        np.minimum.at(new, ei, label[ej])
        np.minimum.at(new, ej, label[ei])
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    return label


def ld_groups(result):
    """The connected components of the participating markers under the edges (linkage groups, bins of co-segregating
    markers): int64 [M], groups numbered from 1 in the order of their smallest marker, singletons included, 0 for a
    marker that does not take part."""
    import numpy as np
    M = len(result.markers)
    label = _edge_components(M, result.edges)
    groups = np.zeros(M, dtype=np.int64)
    part = np.nonzero(result.mask)[0]
    roots = np.unique(label[part])                 # ascending: a component's label is its smallest marker
    groups[part] = np.searchsorted(roots, label[part]) + 1
    return groups


def ld_prune(result):
    """A keep mask over all M markers: the participating markers are walked by (`called` descending, index ascending)
    and a marker is kept iff none of its neighbours is kept already.  No two kept markers are joined by an edge, every
    dropped participating marker has a kept neighbour, and a marker that does not take part is False."""
    import numpy as np
    M = len(result.markers)
    ei, ej = result.edges["i"].astype(np.int64), result.edges["j"].astype(np.int64)
    src, dst = np.concatenate([ei, ej]), np.concatenate([ej, ei])
    order = np.argsort(src, kind="stable")
    dst = dst[order]
    start = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=M))])
    part = np.nonzero(result.mask)[0]
    keep = np.zeros(M, dtype=bool)
    for m in part[np.lexsort((part, -result.called[part].astype(np.int64)))]:
        if not keep[dst[start[m]:start[m + 1]]].any():
            keep[m] = True
    return keep


LD_PAIR_COLUMNS = ("marker_i", "marker_j", "shared", "r2", "phase")
LD_GROUP_COLUMNS = ("marker", "group", "group_size", "degree", "called", "kept")


def writeLDPairs(filename, result):
    """One row per edge: the two marker names, shared, r2 (six decimals) and phase (+ / -, by the sign of cov; 0 when
    cov is 0); CSV with a header row, csv.writer's CRLF rows."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(LD_PAIR_COLUMNS)
        for e, r2 in zip(result.edges, result.r2):
            cov = int(e["cov"])
            out.writerow([result.markers[int(e["i"])], result.markers[int(e["j"])], int(e["shared"]), format(float(r2), ".6f"),
                          "+" if cov > 0 else "-" if cov < 0 else "0"])


def writeLDGroups(filename, result, groups=None, keep=None):
    """One row per participating marker: marker, group (ld_groups), group_size, degree, called, kept (ld_prune: 1 / 0);
    CSV with a header row, csv.writer's CRLF rows.  groups, keep: what ld_groups and ld_prune gave for this result, where
    the caller has them already."""
    import numpy as np
    groups = ld_groups(result) if groups is None else groups
    keep = ld_prune(result) if keep is None else keep
    sizes = np.bincount(groups)
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(LD_GROUP_COLUMNS)
        for m in np.nonzero(result.mask)[0]:
            out.writerow([result.markers[m], int(groups[m]), int(sizes[groups[m]]), int(result.degree[m]), int(result.called[m]),
                          1 if keep[m] else 0])


# ---------------------------------------------------------------------------------------------------------------------
# LD-kNN imputation of the missing calls: the step that fills the holes.  For a missing cell (t, m): the
# markers most in LD with m (a row of the neighbour table, from marker_ld's edges), the samples most alike over those
# markers, and their vote.  Over B = the neighbours q at which target t and donor d are both called: ovl = |B|, dist =
# the sum of |calls[t][q] - calls[d][q]|; a donor called at m with ovl >= min_overlap weighs
# w = 32768 (2 ovl - dist) // ovl; the first k by (w descending, d ascending) vote with their call at m; the cell becomes
# g iff V[g] is the only maximum, the total is positive and V[g] 10^6 >= min_conf_ppm total.  Integers only; only the
# input's calls are read, so no cell depends on another's result.  csrc/impute.hip decides it from the calls where they
# lie, _impute_host restates it in numpy.  No float takes part anywhere but in the order of the neighbours (LDResult.r2).
IMPUTE_MAX_SAMPLES = 4096
IMPUTE_MAX_NBR = 64
IMPUTE_MAX_K = 32
IMPUTE_STATS = ("missing", "imputed", "no_donor", "undecided")
_IMPUTE_HOST_CELLS = 1 << 20    # target-donor pairs of one block of _impute_host at most: three float32 planes of L times this size at a time


class ImputeResult:
    """What impute_calls returns: `.markers`, `.calls` (uint8 [S, M], the filled matrix: imputed cells hold 0 / 1 / 2,
    every other cell its input byte -- or a DeviceCalls, the caller's to free, when the input was one), `.stats` (uint32
    [M, 4] by IMPUTE_STATS: missing, imputed, no_donor, undecided), `.neighbours` (int32 [M, l], -1 where there is none),
    `.ms` (device time), `.imputed` (the cells filled in all), `.params` (backend, l, k, min_overlap, min_conf_ppm)."""

    def __init__(self, markers, calls, stats, neighbours, ms, params):
        self.markers, self.calls, self.stats, self.neighbours, self.ms, self.params = markers, calls, stats, neighbours, ms, params
        self.imputed = int(stats[:, 1].sum(dtype="uint64")) if len(stats) else 0


def ld_neighbours(result, l=20):
    """The neighbour table of impute_calls from an LDResult: int32 [M, l]; row m holds the markers joined to m by an edge,
    ordered by (r2 descending, other marker ascending), the first l of them, then -1."""
    import numpy as np
    if isinstance(l, bool) or int(l) != l or not 1 <= l <= IMPUTE_MAX_NBR:
        raise ValueError("l must be an integer in 1 .. {}".format(IMPUTE_MAX_NBR))
    l, M = int(l), len(result.markers)
    table = np.full((M, l), -1, dtype=np.int32)
    ei, ej = result.edges["i"].astype(np.int64), result.edges["j"].astype(np.int64)
    src, dst, r2 = np.concatenate([ei, ej]), np.concatenate([ej, ei]), np.concatenate([result.r2, result.r2])
    order = np.lexsort((dst, -r2, src))            # by marker, then r2 descending, then the other marker
    src, dst = src[order], dst[order]
    start = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=M))])
    rank = np.arange(len(src)) - start[src]        # the place within the marker's run
    take = rank < l
    table[src[take], rank[take]] = dst[take]
    return table


def _impute_host(calls, nbr, k, min_overlap, min_conf_ppm):
    """The rule of DESIGN 4.17 in numpy, over blocks of markers: ovl and dist of every target against every sample as
    float32 products of the planes over the neighbours (at most 128, exact there), everything after them in int64.  Returns (the filled
    matrix, stats uint32 [M, 4])."""
    import numpy as np
    calls = np.asarray(calls, dtype=np.uint8)
    S, M = calls.shape
    nbr = np.asarray(nbr, dtype=np.int64)
    nbr = nbr.reshape(M, nbr.size // M if M else 1)
    out = calls.copy()
    stats = np.zeros((M, len(IMPUTE_STATS)), dtype=np.uint32)
    own = np.ascontiguousarray(np.minimum(calls, 3).T)             # [M, S], codes 0 .. 3
    gone = own == 3
    stats[:, 0] = gone.sum(axis=1)
    has = (nbr >= 0).any(axis=1)
    stats[~has, 2] = stats[~has, 0]                # an empty row: no target has a donor
    active = np.nonzero(has & (stats[:, 0] > 0))[0]
    sample = np.arange(S, dtype=np.int64)
    block = max(1, _IMPUTE_HOST_CELLS // max(1, S * S))
    for lo in range(0, len(active), block):
        ms = active[lo:lo + block]
        nb = nbr[ms]
        A = own[np.maximum(nb, 0)]                 # [b, L, S]
        C = ((A <= 2) & (nb >= 0)[:, :, None]).astype(np.float32)
        bt, tt = np.nonzero(gone[ms])              # the targets: (marker of the block, sample)
        Cd, ct = C[bt], C[bt, :, tt][:, None, :]   # [n, L, S] over the donors; the target's own plane [n, 1, L]
        o = np.rint((ct @ Cd)[:, 0, :]).astype(np.int64)           # [n, S]
        ds = np.zeros_like(o)
        for level in (1, 2):                       # the thermometer planes: |x - y| = [x >= 1 != y >= 1] + [x >= 2 != y >= 2]
            X = C * (A >= level)
            Xd, xt = X[bt], X[bt, :, tt][:, None, :]
            ds += np.rint((xt @ Cd + ct @ Xd - 2 * (xt @ Xd))[:, 0, :]).astype(np.int64)
        w = 32768 * (2 * o - ds) // np.maximum(o, 1)
        key = np.where((o >= min_overlap) & ~gone[ms][bt], (w << 12) | (4095 - sample), -1)
        top = -np.sort(-key, axis=1)[:, :k]        # the k largest keys, largest first
        voter = top >= 0
        tw = np.where(voter, top >> 12, 0)
        cls = own[ms][bt[:, None], np.where(voter, 4095 - (top & 4095), 0)]
        V = np.stack([(tw * (cls == g)).sum(axis=1) for g in (0, 1, 2)], axis=1)
        total, best = V.sum(axis=1), V.max(axis=1)
        sure = voter[:, 0] & (total > 0) & ((V == best[:, None]).sum(axis=1) == 1) & (best * 1000000 >= min_conf_ppm * total)
        out[tt[sure], ms[bt[sure]]] = V.argmax(axis=1)[sure]
        for col, sel in ((1, sure), (2, ~voter[:, 0]), (3, voter[:, 0] & ~sure)):
            stats[ms, col] = np.bincount(bt[sel], minlength=len(ms))
    return out, stats


def _impute_params(l, k, min_overlap, min_conf):
    for name, v, hi in (("l", l, IMPUTE_MAX_NBR), ("k", k, IMPUTE_MAX_K), ("min_overlap", min_overlap, (1 << 32) - 1)):
        if isinstance(v, bool) or int(v) != v or not 1 <= v <= hi:
            raise ValueError("{} must be an integer in 1 .. {}".format(name, hi))
    return int(l), int(k), int(min_overlap), _ppm(min_conf, 0, 1000000, "min_conf")


def impute_calls(calls, marknames, ld=None, mask=None, l=20, k=10, min_overlap=4, min_conf=0.6, min_r2=0.5, ld_min_shared=50,
                 device=0, backend="gpu"):
    """LD-kNN imputation of the missing genotype calls.

    calls, marknames and mask are marker_ld's: a samples x markers matrix of codes 0, 1, 2 and 3 (missing) -- numpy or
    lists -- or a DeviceCalls (backend="gpu" only; there any byte above 2 is missing); a marker takes part iff its entry of
    mask is true (None: all).  ld: the LDResult whose edges choose the neighbours; None runs marker_ld(calls, marknames,
    mask, min_r2, ld_min_shared) first.  For a missing cell the l markers most in LD with its marker are taken
    (ld_neighbours); the samples called at the marker are ranked by how alike they are to the cell's sample over those
    neighbours, among those that share at least min_overlap of them; the k most alike vote with their own call, weighted by
    likeness, and the cell is filled iff one class wins with at least min_conf of the weight (taken in parts per million).
    A cell that is not filled keeps its input; a marker that does not take part, or is in LD with nothing, is left as it is.
    backend="gpu" runs csrc/impute.hip on the calls where they lie; backend="host" is the numpy restatement: the same bytes.
    At most IMPUTE_MAX_SAMPLES samples.  Returns an ImputeResult; with a DeviceCalls its `.calls` is a DeviceCalls too, and
    the caller's to free."""
    import numpy as np
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    l, k, min_overlap, min_conf_ppm = _impute_params(l, k, min_overlap, min_conf)
    on_device = isinstance(calls, DeviceCalls)
    if on_device and backend != "gpu":
        raise ValueError("a DeviceCalls matrix needs backend='gpu'")
    marknames = list(marknames)
    if ld is None:
        ld = marker_ld(calls, marknames, mask=mask, min_r2=min_r2, min_shared=ld_min_shared, device=device, backend=backend)
    if not on_device:
        calls = np.asarray(calls if len(calls) else np.zeros((0, len(marknames)), dtype=np.uint8))
        if calls.ndim != 2:
            raise ValueError("the call matrix must have two dimensions (samples x markers)")
        if calls.dtype.kind not in "iub":
            raise ValueError("the call matrix must hold the integer codes 0 .. 3, not {}".format(calls.dtype))
        if calls.size and (int(calls.min()) < 0 or int(calls.max()) > 3):
            raise ValueError("the call matrix must hold 0, 1, 2 or 3 (missing) only")
        calls = np.ascontiguousarray(calls, dtype=np.uint8)
    S, M = calls.shape
    if len(marknames) != M or len(ld.markers) != M:
        raise ValueError("marknames and the LD result must name every column of the call matrix")
    if S > IMPUTE_MAX_SAMPLES:
        raise ValueError("at most {} samples".format(IMPUTE_MAX_SAMPLES))
    neighbours = ld_neighbours(ld, l)
    if mask is not None:                           # (an LD result made under another mask: nobody outside this one takes part)
        mask = np.asarray(mask)
        if mask.shape != (M,):
            raise ValueError("mask must have one entry per marker")
        mask = mask != 0
        neighbours[~mask] = -1
        neighbours[(neighbours >= 0) & ~mask[np.maximum(neighbours, 0)]] = -1
    if backend == "host":
        (filled, stats), ms = _impute_host(calls, neighbours, k, min_overlap, min_conf_ppm), 0.0
    else:
        res = default_engine(device).impute_knn(calls.ptr or None if on_device else calls, neighbours,
                                                shape=(S, M) if on_device else None, k=k, min_overlap=min_overlap,
                                                min_conf_ppm=min_conf_ppm, fetch=not on_device, keep_device=on_device)
        filled, stats, ms = DeviceCalls(res.d_calls or 0, (S, M)) if on_device else res.calls, res.stats, res.ms
    return ImputeResult(marknames, filled, stats, neighbours, ms,
                        dict(backend=backend, l=l, k=k, min_overlap=min_overlap, min_conf_ppm=min_conf_ppm))


def impute_hidden_cells(calls, hide_ppm=50000, seed=0, mask=None):
    """The cells impute_check hides: floor(n hide_ppm / 10^6) of the n called cells (of the markers that take part),
    drawn without replacement by numpy's default_rng(seed); flat indices into the matrix, ascending."""
    import numpy as np
    calls = np.asarray(calls)
    if isinstance(hide_ppm, bool) or int(hide_ppm) != hide_ppm or not 0 <= hide_ppm <= 1000000:
        raise ValueError("hide_ppm must be an integer in 0 .. 1000000")
    called = calls <= 2
    if mask is not None:
        called = called & (np.asarray(mask) != 0)[None, :]
    flat = np.flatnonzero(called)
    n = len(flat) * int(hide_ppm) // 1000000
    return np.sort(np.random.default_rng(seed).choice(flat, size=n, replace=False)) if n else flat[:0]


def impute_check(calls, marknames, hide_ppm=50000, seed=0, **kw):
    """How well would impute_calls(calls, marknames, **kw) do here?  Hides impute_hidden_cells(calls, hide_ppm, seed, mask)
    (sets them missing), imputes the rest's way, and returns the int64 [3, 4] table of the hidden cells: true class (rows)
    against outcome 0, 1, 2 or left missing (columns).  With ld=None the LD is taken from the matrix with the cells hidden,
    as it would be in use.  The way to choose l, k, min_overlap and min_conf for one's own data: nothing is promised."""
    import numpy as np
    if isinstance(calls, DeviceCalls):
        raise ValueError("impute_check hides cells of a host matrix")
    truth = np.ascontiguousarray(np.asarray(calls if len(calls) else np.zeros((0, len(marknames)))), dtype=np.uint8)
    hidden = impute_hidden_cells(truth, hide_ppm, seed, kw.get("mask"))
    holed = truth.copy()
    holed.reshape(-1)[hidden] = GENO_MISSING
    got = impute_calls(holed, marknames, **kw).calls.reshape(-1)[hidden]
    table = np.zeros((3, 4), dtype=np.int64)
    np.add.at(table, (truth.reshape(-1)[hidden], np.minimum(got, 3)), 1)
    return table


IMPUTE_STAT_COLUMNS = ("marker",) + IMPUTE_STATS + ("neighbours",)


def writeImputeStats(filename, result):
    """One row per marker: marker, missing, imputed, no_donor, undecided and neighbours (the entries of its row of the
    table); CSV with a header row, csv.writer's CRLF rows."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(IMPUTE_STAT_COLUMNS)
        for m, name in enumerate(result.markers):
            out.writerow([name] + [int(x) for x in result.stats[m]] + [int((result.neighbours[m] >= 0).sum())])


# ---------------------------------------------------------------------------------------------------------------------
# Parent pairs by Mendelian exclusion: which two samples are the parents of this one.  For an offspring o and
# two candidate parents p, q, over the participating markers at which all three are called: n = their number, e = those at
# which o's call is none that (p, q) can produce.  Candidates come from the pair table of sample_relations (n2 = markers
# called in both, e2 = opposing homozygotes), the decision from the trios ranked by e / n.  Integers only; csrc/parent.hip
# counts the trios with bit planes and popcounts from the calls where they lie, _parentage_host restates it in numpy.
PARENT_MAX_SAMPLES = 16384
PARENT_MAX_CAND = 128
PARENT_MAX_TOP = 8
PARENT_NONE = 0xFFFFFFFF
PARENT_TRIO = [("p", "<u4"), ("q", "<u4"), ("n", "<u4"), ("e", "<u4")]
PARENT_STATUS = ("trio", "ambiguous", "single", "none")
_PARENT_HOST_BLOCK = 1 << 16    # markers of one block of _parentage_host: float32 planes of C times this size at a time


class ParentageResult:
    """What parentage returns: `.samples` (all names), `.offspring` (the sample indices asked about, in order) and, per
    offspring, `.status` ("trio", "ambiguous", "single" or "none"), `.trios` (the first `top` ranked trios as tuples
    (p, q, n, e) of sample indices and counts, best first), `.passes` (whether each of them passes max_trio_err),
    `.single` ((p, n2, e2) of the first candidate when the status is "single", else None) and `.candidates` (how many
    candidate parents the pair test left); `.stats` (backend, ms, markers, used and the thresholds)."""

    def __init__(self, samples, offspring, status, trios, passes, single, candidates, stats):
        self.samples, self.offspring, self.status, self.trios = samples, offspring, status, trios
        self.passes, self.single, self.candidates, self.stats = passes, single, candidates, stats

    def counts(self):
        """How many offspring have each status, in the order of PARENT_STATUS."""
        return [sum(1 for s in self.status if s == k) for k in PARENT_STATUS]


def _parent_pairs(C, selfing):
    """The slot pairs (a, b) of C slots in trio order: a ascending, then b ascending; a <= b with selfing, else a < b."""
    import numpy as np
    return np.triu_indices(C, 0 if selfing else 1)


def _parent_first(n, e, live):
    """The index of the first trio among `live` by (e / n ascending by cross-multiplication, n descending, index
    ascending); n, e int64 below 2^31, n > 0 where live.  -1 when none is live."""
    import numpy as np
    idx = np.flatnonzero(live)
    if not len(idx):
        return -1
    b = int(idx[np.argmin(e[idx] / n[idx])])
    while True:                                    # the float minimum is a start; the exact rule decides
        l, r = e[idx] * n[b], e[b] * n[idx]
        better = (l < r) | ((l == r) & ((n[idx] > n[b]) | ((n[idx] == n[b]) & (idx < b))))
        if not better.any():
            return b
        sub = idx[better]
        b = int(sub[np.argmin(e[sub] / n[sub])])


def _parent_rank(table, cand, selfing, K, min_shared):
    """The first K trios of every row of a table [O, T, 2] by the ranking of DESIGN 4.18, as td_parent_trio records [O, K]."""
    import numpy as np
    O, C = cand.shape
    ia, ib = _parent_pairs(C, selfing)
    best = np.zeros((O, K), dtype=PARENT_TRIO)
    best["p"] = best["q"] = PARENT_NONE
    for i in range(O):
        n, e = table[i, :, 0].astype(np.int64), table[i, :, 1].astype(np.int64)
        live = n >= min_shared
        for k in range(K):
            t = _parent_first(n, e, live)
            if t < 0:
                break
            best[i, k] = (cand[i, ia[t]], cand[i, ib[t]], n[t], e[t])
            live[t] = False
    return best


def _parentage_host(calls, use, offspring, cand, selfing, K, min_shared):
    """The trio counts and their ranking of DESIGN 4.18 in numpy.  n and e of every slot pair are sums of Gram products of
    0 / 1 planes over the markers -- with A = called in offspring and parent, n = A A'; where the offspring is 0 the errors
    are the trios with a parent called 2, i.e. all minus those with neither; likewise at 2; where it is 1 they are the
    trios with both parents 0 or both 2 -- taken in float32 over blocks of markers short enough to be exact (< 2^24) and
    summed in int64.  Returns (best [O, K] records, table uint32 [O, T, 2])."""
    import numpy as np
    calls = np.asarray(calls, dtype=np.uint8)
    S, M = calls.shape
    offspring, cand = np.asarray(offspring, dtype=np.int64), np.asarray(cand, dtype=np.int64)
    O, C = cand.shape
    ia, ib = _parent_pairs(C, selfing)
    cols = np.arange(M) if use is None else np.nonzero(np.asarray(use) != 0)[0]
    N, E = np.zeros((O, C, C), dtype=np.int64), np.zeros((O, C, C), dtype=np.int64)
    for lo in range(0, len(cols), _PARENT_HOST_BLOCK):
        part = calls[:, cols[lo:lo + _PARENT_HOST_BLOCK]]
        for i in range(O):
            own = part[offspring[i]]
            P = part[np.maximum(cand[i], 0)]
            P = np.where((cand[i] >= 0)[:, None], P, 3)            # an empty slot is called nowhere
            both = (P <= 2) & (own <= 2)[None, :]

            def gram(X):
                X = X.astype(np.float32)
                return np.rint(X @ X.T).astype(np.int64)

            o0, o1, o2 = both & (own == 0), both & (own == 1), both & (own == 2)
            N[i] += gram(both)
            E[i] += gram(o0) - gram(o0 & (P != 2)) + gram(o2) - gram(o2 & (P != 0)) + gram(o1 & (P == 0)) + gram(o1 & (P == 2))
    table = np.stack([N[:, ia, ib], E[:, ia, ib]], axis=2).astype(np.uint32).reshape(O, len(ia), 2)
    return _parent_rank(table, cand, selfing, K, min_shared), table


def _parent_candidates(n2, e2, allowed, min_shared, max_pair_err_ppm, max_candidates):
    """The candidate parents of one offspring from its row of the pair table (n2, e2 int64 [S]; allowed bool [S]): those
    with n2 >= min_shared and e2 10^6 <= max_pair_err_ppm n2, ordered by e2 / n2 ascending (cross-multiplied), n2
    descending, index ascending; the first max_candidates."""
    import functools
    import numpy as np
    idx = np.flatnonzero(allowed & (n2 >= min_shared) & (e2 * 1000000 <= max_pair_err_ppm * n2))
    if len(idx) > 1:
        n, e = n2[idx], e2[idx]
        order = np.lexsort((idx, -n, e / n))       # a float key first; the neighbours are then checked exactly
        idx, n, e = idx[order], n[order], e[order]
        l, r = e[:-1] * n[1:], e[1:] * n[:-1]
        in_order = (l < r) | ((l == r) & ((n[:-1] > n[1:]) | ((n[:-1] == n[1:]) & (idx[:-1] < idx[1:]))))
        if not in_order.all():

            def cmp(x, y):
                l, r = int(e2[x]) * int(n2[y]), int(e2[y]) * int(n2[x])
                return -1 if (l, -int(n2[x]), x) < (r, -int(n2[y]), y) else 1

            idx = np.array(sorted(idx.tolist(), key=functools.cmp_to_key(cmp)), dtype=np.int64)
    return idx[:max_candidates]


def _name_indices(names, where, what):
    out = []
    for name in names:
        if name not in where:
            raise ValueError("{} {!r} is not a sample of the call matrix".format(what, name))
        out.append(where[name])
    return out


def parentage(calls, samnames, offspring=None, parents=None, mask=None, max_pair_err=0.03, max_trio_err=0.03, min_shared=50,
              max_candidates=32, top=2, selfing=True, device=0, backend="gpu"):
    """Parent pairs of the samples by Mendelian exclusion.

    calls, samnames and mask are sample_relations': a samples x markers matrix of codes 0, 1, 2 and 3 (missing) -- numpy
    or lists -- or a DeviceCalls (backend="gpu" only; there any byte above 2 is missing); a marker takes part iff its
    entry of mask is true (None: all).  offspring, parents: lists of sample names, the samples asked about and the samples
    that may be parents (None: all samples).  Sample p is a candidate parent of o iff it is in parents, is not o, shares
    n2 >= min_shared called markers with o and is an opposing homozygote at e2 of them with e2 10^6 <= max_pair_err_ppm
    n2; the first max_candidates by (e2 / n2 ascending, n2 descending, index ascending) are kept.  For every pair of an
    offspring's candidates (one twice included, with selfing) the trio is counted: n markers called in all three, e of
    them at which the offspring's call is none the pair can produce.  Trios with n >= min_shared are ranked by (e / n
    ascending, n descending, slot pair ascending); one passes iff e 10^6 <= max_trio_err_ppm n.  Status: "trio" -- the
    best passes and the second does not; "ambiguous" -- two pass; "single" -- none passes but there is a candidate (the
    first is reported); "none".  The rates are taken in parts per million.  Nothing is promised about accuracy: the
    thresholds are the user's to set for the error rate of their calls.  backend="gpu" runs csrc/relate.hip and
    csrc/parent.hip on the calls where they lie; backend="host" is the numpy restatement: the same result.  Returns a
    ParentageResult."""
    import numpy as np
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    pair_ppm = _ppm(max_pair_err, 0, 1000000, "max_pair_err")
    trio_ppm = _ppm(max_trio_err, 0, 1000000, "max_trio_err")
    for name, v, lo, hi in (("min_shared", min_shared, 1, (1 << 31) - 1), ("max_candidates", max_candidates, 1, PARENT_MAX_CAND),
                            ("top", top, 1, PARENT_MAX_TOP)):
        if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError("{} must be an integer in {} .. {}".format(name, lo, hi))
    min_shared, max_candidates, top, selfing = int(min_shared), int(max_candidates), int(top), bool(selfing)
    on_device = isinstance(calls, DeviceCalls)
    if on_device and backend != "gpu":
        raise ValueError("a DeviceCalls matrix needs backend='gpu'")
    samnames = list(samnames)
    if not on_device:
        calls = np.asarray(calls if len(calls) else np.zeros((0, 0 if mask is None else len(mask)), dtype=np.uint8))
        if calls.ndim != 2:
            raise ValueError("the call matrix must have two dimensions (samples x markers)")
        if calls.dtype.kind not in "iub":
            raise ValueError("the call matrix must hold the integer codes 0 .. 3, not {}".format(calls.dtype))
        if calls.size and (int(calls.min()) < 0 or int(calls.max()) > 3):
            raise ValueError("the call matrix must hold 0, 1, 2 or 3 (missing) only")
        calls = np.ascontiguousarray(calls, dtype=np.uint8)
    S, M = calls.shape
    if len(samnames) != S:
        raise ValueError("samnames must name every row of the call matrix")
    if S > PARENT_MAX_SAMPLES:
        raise ValueError("at most {} samples".format(PARENT_MAX_SAMPLES))
    if M >= 1 << 31:
        raise ValueError("markers must number below 2^31")
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (M,):
            raise ValueError("mask must have one entry per marker")
        mask = mask != 0
    where = {}
    for k, name in enumerate(samnames):
        where.setdefault(name, k)
    off = list(range(S)) if offspring is None else _name_indices(offspring, where, "offspring")
    allowed = np.ones(S, dtype=bool)
    if parents is not None:
        allowed[:] = False
        allowed[_name_indices(parents, where, "parent")] = True
    K, O = max(2, top), len(off)
    eng = d_own = None
    ms = 0.0
    try:
        if backend == "host":
            joint = _relations_host(calls, mask)
        else:
            eng = default_engine(device)
            if on_device:
                ptr = calls.ptr or None
            else:                                  # one upload serves both kernels
                ptr = d_own = eng.dev_alloc(calls.nbytes) if calls.size else None
                if d_own:
                    eng.h2d(d_own, calls.tobytes())
            rel = eng.relate_joint(ptr, shape=(S, M), use=mask)
            joint, ms = rel.joint, rel.ms
        J = joint[off].astype(np.int64) if O else np.zeros((0, S, 3, 3), dtype=np.int64)
        n2, e2 = J.sum(axis=(2, 3)), J[:, :, 0, 2] + J[:, :, 2, 0]
        lists = []
        for i, o in enumerate(off):
            ok = allowed.copy()
            ok[o] = False
            lists.append(_parent_candidates(n2[i], e2[i], ok, min_shared, pair_ppm, max_candidates))
        Cn = max([1] + [len(x) for x in lists])
        cand = np.full((O, Cn), -1, dtype=np.int32)
        for i, x in enumerate(lists):
            cand[i, :len(x)] = x
        if backend == "host":
            best = _parentage_host(calls, mask, off, cand, selfing, K, min_shared)[0] if O else np.zeros((0, K), dtype=PARENT_TRIO)
        else:
            res = eng.parent_trios(ptr, off, cand, shape=(S, M), use=mask, selfing=selfing, top=K, min_shared=min_shared)
            best, ms = res.best, ms + res.ms
    finally:
        if d_own:
            eng.dev_free(d_own)
    status, trios, passes, single = [], [], [], []
    for i in range(O):
        ranked = [(int(r["p"]), int(r["q"]), int(r["n"]), int(r["e"])) for r in best[i] if r["p"] != PARENT_NONE]
        ok = [e * 1000000 <= trio_ppm * n for _, _, n, e in ranked]
        if ok[:1] == [True]:
            status.append("ambiguous" if ok[1:2] == [True] else "trio")
        else:
            status.append("single" if len(lists[i]) else "none")
        first = int(lists[i][0]) if status[-1] == "single" else None
        single.append(None if first is None else (first, int(n2[i, first]), int(e2[i, first])))
        trios.append(ranked[:top])
        passes.append(ok[:top])
    used = M if mask is None else int(mask.sum())
    stats = dict(backend=backend, ms=ms, markers=M, used=used, max_pair_err_ppm=pair_ppm, max_trio_err_ppm=trio_ppm, min_shared=min_shared,
                 max_candidates=max_candidates, top=top, selfing=selfing)
    return ParentageResult(samnames, off, status, trios, passes, single, [len(x) for x in lists], stats)


def _rate_text(e, n):
    return "NA" if n == 0 else format(e / n, ".6f")


PARENTAGE_COLUMNS = ("offspring", "status", "parent1", "parent2", "shared", "errors", "error_rate", "single_parent", "pair_shared",
                     "pair_errors", "pair_error_rate", "candidates")
PARENT_TRIO_COLUMNS = ("offspring", "rank", "parent1", "parent2", "shared", "errors", "error_rate", "pass")


def writeParentage(filename, result):
    """One row per offspring: its name, the status, for "trio" and "ambiguous" the best trio (the parents' names, the
    markers called in all three, the Mendelian errors among them and their share, six decimals), for "single" the first
    candidate (name, markers called in both, opposing homozygotes and their share), and the number of candidates; cells
    that do not apply are empty.  CSV with a header row, csv.writer's CRLF rows."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(PARENTAGE_COLUMNS)
        for i, o in enumerate(result.offspring):
            trio, one = [""] * 5, [""] * 4
            if result.status[i] in ("trio", "ambiguous"):
                p, q, n, e = result.trios[i][0]
                trio = [result.samples[p], result.samples[q], n, e, _rate_text(e, n)]
            if result.single[i] is not None:
                p, n, e = result.single[i]
                one = [result.samples[p], n, e, _rate_text(e, n)]
            out.writerow([result.samples[o], result.status[i]] + trio + one + [result.candidates[i]])


def writeTrios(filename, result):
    """One row per ranked trio that parentage kept (the first `top` of every offspring): offspring, rank from 1, the
    parents' names, shared, errors, their share (six decimals) and pass (1 / 0); CSV with a header row, CRLF rows."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(PARENT_TRIO_COLUMNS)
        for i, o in enumerate(result.offspring):
            for k, (p, q, n, e) in enumerate(result.trios[i]):
                out.writerow([result.samples[o], k + 1, result.samples[p], result.samples[q], n, e, _rate_text(e, n),
                              1 if result.passes[i][k] else 0])


# ---------------------------------------------------------------------------------------------------------------------
# Linkage of the markers of a cross: which markers are linked, in which phase, in what order.  Only the
# offspring rows enter a count.  A marker that takes part has two classes A and B (by the cross type, from its class
# counts or the parents' calls); a cell is x = +1 for A, -1 for B, 0 otherwise.  For two markers of one map:
# N = sum x_i^2 x_j^2, D = sum x_i x_j, rec = (N - |D|) / 2, phase = (D < 0), lod16 = 65536 N + f[rec] + f[N - rec] - f[N]
# with f[k] = round(65536 k log2 k); an edge iff N >= min_shared, rec 10^6 <= max_rf_ppm N and lod16 >= min_lod16 --
# integers only.  csrc/link.hip decides it on the matrix cores from the calls where they lie, _link_pairs_host restates
# it in numpy; groups, order and positions are host code that both backends share.  Floats appear only in the positions.
LINK_MAX_SAMPLES = 16384
LINK_MAX_MARKERS = 1 << 20
LINK_EDGE = [("i", "<u4"), ("j", "<u4"), ("n", "<u4"), ("rec_phase", "<u4"), ("lod16", "<i8")]
LINK_NO_PART = 255
LINK_LOD_MIN = -(1 << 63)
LINK_CROSSES = ("dh", "bc", "cp")
LINK_CLASSES = ((0, 1), (2, 1), (0, 2))            # the cls code of a marker -> its classes (A, B)
LINK_REASONS = ("", "parents", "masked", "few", "distorted", "other")
_LINK_HOST_CELLS = 1 << 21  # pairs of one block of _link_pairs_host
_LINK_TABLE = [0, 0]        # f[0 .. ]: grown by linkage_tables, never shrunk


def _link_entry(k, prec):
    """round_half_even(65536 k log2 k) for k >= 1 with decimal at `prec` digits, or None where that precision cannot
    tell on which side of a half the value lies."""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = prec
        v = decimal.Decimal(65536 * k) * decimal.Decimal(k).ln() / decimal.Decimal(2).ln()
        lo = v.to_integral_value(rounding=decimal.ROUND_FLOOR)
        slack = decimal.Decimal(10) ** (v.adjusted() + 5 - prec)       # far above the error of two ln and two operations
        if abs(v - lo - decimal.Decimal("0.5")) <= slack and (k & (k - 1)):
            return None
        return int(v.quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_EVEN))


def linkage_tables(n, prec=50):
    """f[k] = round(65536 k log2 k) for k = 0 .. n (f[0] = 0) as a list of ints: the table behind the LOD of
    linkage_map, lod16 = 65536 N + f[rec] + f[N - rec] - f[N] = 65536 log2 of the likelihood ratio of r = rec / N against
    r = 1 / 2.  Pure Python (decimal, at a precision raised until every entry is unambiguous): the same on every machine."""
    n = int(n)
    if n < 0:
        raise ValueError("n must be at least 0")
    while len(_LINK_TABLE) <= n:
        k, p, e = len(_LINK_TABLE), int(prec), None
        while e is None:
            e = _link_entry(k, p)
            p *= 2
        _LINK_TABLE.append(e)
    return _LINK_TABLE[:n + 1]


def linkage_min_lod16(min_lod):
    """ceil(min_lod * 65536 * log2 10), from the decimal text of min_lod: the threshold lod16 is compared with."""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        v = decimal.Decimal(str(min_lod)) * 65536 * decimal.Decimal(10).ln() / decimal.Decimal(2).ln()
        return int(v.to_integral_value(rounding=decimal.ROUND_CEILING))


def _link_scaled(value, scale, lo, hi, what):
    """A decimal option as an integer in units of 1 / scale, from its decimal text (rounded half even), in lo .. hi."""
    import decimal
    v = int((decimal.Decimal(str(value)) * scale).quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_EVEN))
    if not lo <= v <= hi:
        raise ValueError("{} must lie in {} .. {}".format(what, lo / scale, hi / scale))
    return v


def linkage_classes(cross, counts, parent_calls=None):
    """(map_of, cls) of every marker, int8 and uint8 [M]: the map a marker belongs to (1 or 2; 0: none) and its class
    pair as an index into LINK_CLASSES (LINK_NO_PART where map_of is 0).  dh: A = 0, B = 2.  bc: (0, 1) if c0 >= c2 else
    (2, 1), from counts [M, 4].  cp: parent_calls = (calls of parent 1, calls of parent 2) over the markers; map 1 iff
    parent 1 is 1 and parent 2 is 0 or 2, then A = parent 2's call and B = 1; map 2 with the roles swapped."""
    import numpy as np
    if cross not in LINK_CROSSES:
        raise ValueError("cross must be one of {}".format(", ".join(LINK_CROSSES)))
    counts = np.asarray(counts).reshape(-1, 4)
    M = len(counts)
    map_of, cls = np.ones(M, dtype=np.int8), np.full(M, 2, dtype=np.uint8)
    if cross == "bc":
        cls[:] = np.where(counts[:, 0] >= counts[:, 2], 0, 1)
    elif cross == "cp":
        if parent_calls is None:
            raise ValueError("cross 'cp' needs the calls of its two parents")
        p1, p2 = (np.asarray(p, dtype=np.uint8).reshape(M) for p in parent_calls)
        hom1, hom2 = (p1 == 0) | (p1 == 2), (p2 == 0) | (p2 == 2)
        in1, in2 = (p1 == 1) & hom2, (p2 == 1) & hom1
        map_of[:] = np.where(in1, 1, np.where(in2, 2, 0))
        hom = np.where(in1, p2, p1)                # the homozygous parent's call: class A
        cls[:] = np.where(map_of == 0, LINK_NO_PART, np.where(hom == 0, 0, 1))
    return map_of, cls


def linkage_segregation(counts, cls, min_shared, max_chi2_milli, max_other_ppm):
    """(a, b, o, verdict) per marker from counts [M, 4] and the class pairs: a = count(A), b = count(B), o = the called
    cells that are neither (int64 [M]; 0 where cls is LINK_NO_PART), verdict (uint8 [M], an index into LINK_REASONS): 0
    iff the marker segregates -- a + b >= min_shared, (a - b)^2 1000 <= max_chi2_milli (a + b) and
    o 10^6 <= max_other_ppm (a + b + o) -- else the first test that fails; 1 where it has no class pair."""
    import numpy as np
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    cls = np.asarray(cls, dtype=np.uint8)
    part = cls != LINK_NO_PART
    k = np.where(part, cls, 0)
    ab = np.array(LINK_CLASSES, dtype=np.int64)
    rows = np.arange(len(counts))
    a = np.where(part, counts[rows, ab[k, 0]], 0)
    b = np.where(part, counts[rows, ab[k, 1]], 0)
    o = np.where(part, counts[:, :3].sum(axis=1) - a - b, 0)
    verdict = np.zeros(len(counts), dtype=np.uint8)
    # (a - b)^2 1000 < 2^38 and o 10^6 < 2^34: int64 holds every product
    verdict[o * 1000000 > max_other_ppm * (a + b + o)] = 5
    verdict[(a - b) ** 2 * 1000 > max_chi2_milli * (a + b)] = 4
    verdict[a + b < min_shared] = 3
    verdict[~part] = 1
    return a, b, o, verdict


def _link_counts_host(calls, rows):
    import numpy as np
    part = calls[rows]
    return np.stack([(part == 0).sum(axis=0), (part == 1).sum(axis=0), (part == 2).sum(axis=0), (part > 2).sum(axis=0)],
                    axis=1).astype(np.uint32).reshape(calls.shape[1], 4)


def _link_pairs_host(calls, rows, cls, lodtab, max_rf_ppm, min_lod16, min_shared):
    """Step 2 of DESIGN 4.24 in numpy, over blocks of markers: D and N as float32 products (at most 16384, exact
    there), everything after them in 64-bit integers.  Returns (edges ascending by (i, j), degree, informative)."""
    import numpy as np
    M = calls.shape[1]
    cols = np.nonzero(cls != LINK_NO_PART)[0]
    part = calls[np.asarray(rows, dtype=np.int64)][:, cols]
    ab = np.array(LINK_CLASSES, dtype=np.uint8)[cls[cols]]
    X = (part == ab[None, :, 0]).astype(np.float32) - (part == ab[None, :, 1]).astype(np.float32)
    V = np.abs(X)
    informative, degree = np.zeros(M, dtype=np.uint32), np.zeros(M, dtype=np.uint32)
    informative[cols] = V.sum(axis=0).astype(np.uint32)
    tab = np.asarray(lodtab, dtype=np.int64)
    Mp, found = len(cols), []
    block = max(1, _LINK_HOST_CELLS // max(1, Mp))
    for lo in range(0, Mp if len(rows) else 0, block):
        hi = min(Mp, lo + block)
        d = np.rint(X[:, lo:hi].T @ X[:, lo:]).astype(np.int64)
        n = np.rint(V[:, lo:hi].T @ V[:, lo:]).astype(np.int64)
        rec = (n - np.abs(d)) // 2
        lod = 65536 * n + tab[rec] + tab[n - rec] - tab[n]
        edge = (n >= min_shared) & (rec * 1000000 <= max_rf_ppm * n) & (lod >= min_lod16)
        edge &= np.arange(lo, Mp)[None, :] > np.arange(lo, hi)[:, None]                # i < j
        bi, bj = np.nonzero(edge)                                                      # row-major: ascending (i, j)
        e = np.zeros(len(bi), dtype=LINK_EDGE)
        e["i"], e["j"], e["n"], e["lod16"] = cols[bi + lo], cols[bj + lo], n[bi, bj], lod[bi, bj]
        e["rec_phase"] = rec[bi, bj] | ((d[bi, bj] < 0).astype(np.int64) << 31)
        found.append(e)
    edges = np.concatenate(found) if found else np.zeros(0, dtype=LINK_EDGE)
    if len(edges):
        degree += np.bincount(edges["i"], minlength=M).astype(np.uint32) + np.bincount(edges["j"], minlength=M).astype(np.uint32)
    return edges, degree, informative


def linkage_groups(M, part, edges, min_group):
    """The connected components of the participating markers (part: bool [M]) under the edges: int64 [M], the components
    of at least min_group markers numbered from 1 in the order of their smallest marker, 0 for every other marker."""
    import numpy as np
    label = _edge_components(M, edges)
    groups = np.zeros(M, dtype=np.int64)
    members = np.nonzero(part)[0]
    roots, sizes = np.unique(label[members], return_counts=True)      # ascending: a component's label is its smallest marker
    roots = roots[sizes >= min_group]
    kept = np.isin(label[members], roots)
    groups[members[kept]] = np.searchsorted(roots, label[members[kept]]) + 1
    return groups


def linkage_order(members, edges, min_shared):
    """The greedy chain of one group.  members: its markers, ascending; edges: every pair of them with n >= 1 (the pair
    call with the thresholds off).  rf_ppm(u, v) = rec 10^6 // n where n >= min_shared, else 500000.  The chain starts
    with the pair of smallest (rf_ppm, i, j); then the unplaced marker u and end e of smallest (rf_ppm(e, u), u, e is the
    right end) is appended at e, until none remains; the end holding the smaller marker comes first.  Returns (order,
    positions, phases): the markers along the chain, cumulative Kosambi centimorgans of the adjacent pairs
    (25 ln((1 + 2 r) / (1 - 2 r)), r = rec / n capped at 0.499; 0.499 where n = 0) and the phase of every marker relative
    to the first (its left neighbour's XOR the pair's)."""
    import math
    import numpy as np
    members = np.asarray(members, dtype=np.int64)
    g = len(members)
    if g == 0:
        return [], [], []
    li, lj = np.searchsorted(members, edges["i"]), np.searchsorted(members, edges["j"])
    n = np.zeros((g, g), dtype=np.int64)
    rec, ph = np.zeros((g, g), dtype=np.int64), np.zeros((g, g), dtype=np.int64)
    n[li, lj] = n[lj, li] = edges["n"]
    rec[li, lj] = rec[lj, li] = edges["rec_phase"] & 0x7fffffff
    ph[li, lj] = ph[lj, li] = edges["rec_phase"] >> 31
    rf = np.where(n >= max(1, min_shared), rec * 1000000 // np.maximum(n, 1), 500000)
    if g == 1:
        chain = [0]
    else:
        iu, ju = np.triu_indices(g, 1)                                 # ascending (i, j): the first minimum is the smallest
        first = int(np.argmin(rf[iu, ju]))
        chain = [int(iu[first]), int(ju[first])]
        free = np.ones(g, dtype=bool)
        free[chain] = False
        local = np.arange(g, dtype=np.int64)
        while free.any():
            left, right = chain[0], chain[-1]
            key = np.concatenate([(rf[left] << 32) | (local << 1), (rf[right] << 32) | (local << 1) | 1])
            key[np.concatenate([~free, ~free])] = np.iinfo(np.int64).max
            at = int(np.argmin(key))
            u = at % g
            if at >= g:
                chain.append(u)
            else:
                chain.insert(0, u)
            free[u] = False
        if chain[0] > chain[-1]:
            chain.reverse()
    positions, phases = [0.0], [0]
    for u, v in zip(chain, chain[1:]):
        r = min(int(rec[u, v]) / int(n[u, v]), 0.499) if n[u, v] else 0.499
        positions.append(positions[-1] + 25.0 * math.log((1.0 + 2.0 * r) / (1.0 - 2.0 * r)))
        phases.append(phases[-1] ^ int(ph[u, v]))
    return [int(members[k]) for k in chain], positions, phases


class LinkageMap:
    """One map of a LinkageResult: `.number` (1 or 2), `.cls` (uint8 [M]: the class pair of the markers that take part,
    LINK_NO_PART elsewhere), `.edges` (structured array i, j, n, rec_phase, lod16; ascending by (i, j)), `.rec` and
    `.phase` (per edge), `.degree` and `.informative` (uint32 [M]), `.groups` (int64 [M], from 1; 0: in no group),
    `.order` (dict group -> the markers along the chain, or ascending where the group is too large to order),
    `.positions` and `.phases` (dict group -> list of cM / 0-1 per marker of `.order`, None where unordered)."""

    def __init__(self, number, cls, edges, degree, informative):
        self.number, self.cls, self.edges, self.degree, self.informative = number, cls, edges, degree, informative
        self.rec = (edges["rec_phase"] & 0x7fffffff).astype("int64")
        self.phase = (edges["rec_phase"] >> 31).astype("int8")
        self.groups, self.order, self.positions, self.phases = None, {}, {}, {}


class LinkageResult:
    """What linkage_map returns: `.samples`, `.markers`, `.cross`, `.parents` (row indices or None), `.offspring` (row
    indices), `.counts` (uint32 [M, 4]: c0, c1, c2, cmiss over the offspring), `.map_of` (int8 [M]: 1, 2 or 0), `.cls`
    (uint8 [M]), `.a`, `.b`, `.o` (int64 [M]), `.verdict` (uint8 [M], an index into LINK_REASONS; 0: takes part),
    `.maps` (list of LinkageMap), `.warnings` (list of lines), `.stats` (backend, ms, the integer thresholds)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _link_rows(names, samnames, what):
    """Row indices from a list of names or indices."""
    out = []
    for x in names:
        if isinstance(x, str):
            if x not in samnames:
                raise ValueError("{} {!r} is not among the samples".format(what, x))
            out.append(samnames.index(x))
        else:
            if not 0 <= int(x) < len(samnames):
                raise ValueError("{} {} is no row of the call matrix".format(what, x))
            out.append(int(x))
    if len(set(out)) != len(out):
        raise ValueError("a {} is listed twice".format(what))
    return out


def linkage_map(calls, samnames, marknames, cross, parents=None, offspring=None, mask=None, min_lod=3, max_rf=0.25, min_shared=50,
                max_chi2=6.635, max_other=0.05, min_group=3, max_order=4096, device=0, backend="gpu"):
    """The linkage map of a cross from its genotype calls.

    calls: a samples x markers matrix of codes 0, 1, 2 and 3 (missing) -- numpy or lists -- or a DeviceCalls
    (backend="gpu" only; there any byte above 2 is missing).  cross: "dh" (doubled haploids), "bc" (backcross) or "cp"
    (pseudo-testcross of an outcrossing F1: two maps, one per parent).  parents: the two parent rows (names or indices;
    needed for "cp", optional otherwise); offspring: the rows that enter the counts (names or indices; None: every row
    that is no parent).  mask: one entry per marker, a marker can take part iff its entry is true.  Markers that
    segregate as their class pair demands (linkage_segregation) are compared pairwise; the pairs with at least
    min_shared informative offspring, a recombination fraction of at most max_rf and a LOD of at least min_lod are the
    edges, their connected components of at least min_group markers the linkage groups, and every group of at most
    max_order markers is ordered by the greedy chain of linkage_order.  backend="gpu" runs csrc/link.hip on the calls
    where they lie; backend="host" is the numpy restatement: the same result.  Returns a LinkageResult."""
    import numpy as np
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    if cross not in LINK_CROSSES:
        raise ValueError("cross must be one of {}".format(", ".join(LINK_CROSSES)))
    max_rf_ppm = _link_scaled(max_rf, 1000000, 0, 500000, "max_rf")
    max_chi2_milli = _link_scaled(max_chi2, 1000, 0, 1 << 40, "max_chi2")
    max_other_ppm = _link_scaled(max_other, 1000000, 0, 1000000, "max_other")
    min_lod16 = linkage_min_lod16(min_lod)
    for name, v in (("min_shared", min_shared), ("min_group", min_group), ("max_order", max_order)):
        if isinstance(v, bool) or int(v) != v or not 0 <= v < 1 << 32:
            raise ValueError("{} must be an integer of at least 0".format(name))
    min_shared, min_group, max_order = int(min_shared), int(min_group), int(max_order)
    on_device = isinstance(calls, DeviceCalls)
    if on_device and backend != "gpu":
        raise ValueError("a DeviceCalls matrix needs backend='gpu'")
    samnames, marknames = list(samnames), list(marknames)
    if not on_device:
        calls = np.asarray(calls if len(calls) else np.zeros((0, len(marknames)), dtype=np.uint8))
        if calls.ndim != 2:
            raise ValueError("the call matrix must have two dimensions (samples x markers)")
        if calls.dtype.kind not in "iub":
            raise ValueError("the call matrix must hold the integer codes 0 .. 3, not {}".format(calls.dtype))
        if calls.size and (int(calls.min()) < 0 or int(calls.max()) > 3):
            raise ValueError("the call matrix must hold 0, 1, 2 or 3 (missing) only")
        calls = np.ascontiguousarray(calls, dtype=np.uint8)
    S, M = calls.shape
    if len(samnames) != S:
        raise ValueError("samnames must name every row of the call matrix")
    if len(marknames) != M:
        raise ValueError("marknames must name every column of the call matrix")
    if M >= 1 << 31:
        raise ValueError("markers must number below 2^31")
    parents = None if parents is None else _link_rows(parents, samnames, "parent")
    if cross == "cp" and (parents is None or len(parents) != 2):
        raise ValueError("cross 'cp' needs its two parents")
    if offspring is None:
        offspring = [s for s in range(S) if parents is None or s not in parents]
    else:
        offspring = _link_rows(offspring, samnames, "offspring")
        if parents is not None and set(offspring) & set(parents):
            raise ValueError("a parent is listed among the offspring")
    if len(offspring) > LINK_MAX_SAMPLES:
        raise ValueError("at most {} offspring".format(LINK_MAX_SAMPLES))
    rows = np.array(offspring, dtype=np.uint32)
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (M,):
            raise ValueError("mask must have one entry per marker")
        mask = mask != 0
    eng = default_engine(device) if backend == "gpu" else None
    matrix, shape = (calls.ptr or None, (S, M)) if on_device else (calls, None)
    d_own = None
    if eng is not None and not on_device and calls.size:               # one upload serves every call below
        d_own = eng.dev_alloc(calls.nbytes)
        eng.h2d(d_own, calls.tobytes())
        matrix, shape = d_own, (S, M)
    try:
        total_ms = 0.0
        if eng is None:
            counts = _link_counts_host(calls, rows)
        else:
            counts, ms = eng.link_counts(matrix, shape=shape, rows=rows)
            total_ms += ms
        parent_calls = None
        if cross == "cp":
            if on_device:
                parent_calls = [np.frombuffer(eng.d2h(calls.ptr + p * M, M), dtype=np.uint8) if M else np.zeros(0, np.uint8) for p in parents]
            else:
                parent_calls = [calls[p] for p in parents]
        map_of, cls = linkage_classes(cross, counts, parent_calls)
        a, b, o, verdict = linkage_segregation(counts, cls, min_shared, max_chi2_milli, max_other_ppm)
        if mask is not None:
            verdict[(verdict != 1) & ~mask] = 2
        lodtab = np.array(linkage_tables(len(rows)), dtype=np.int64)

        def pair_call(use_cls, rf_ppm, lod16, shared, capacity=None):
            if eng is None:
                return _link_pairs_host(calls, rows, use_cls, lodtab, rf_ppm, lod16, shared) + (0.0,)
            res = eng.link_pairs(matrix, use_cls, lodtab, shape=shape, rows=rows, max_rf_ppm=rf_ppm, min_lod16=lod16, min_shared=shared,
                                 capacity=capacity)
            return res.edges, res.degree, res.informative, res.ms

        maps, warnings = [], []
        for number in ((1, 2) if cross == "cp" else (1,)):
            taking = (map_of == number) & (verdict == 0)
            if int(taking.sum()) > LINK_MAX_MARKERS:
                raise ValueError("{} participating markers, at most {}".format(int(taking.sum()), LINK_MAX_MARKERS))
            map_cls = np.where(taking, cls, LINK_NO_PART).astype(np.uint8)
            edges, degree, informative, ms = pair_call(map_cls, max_rf_ppm, min_lod16, min_shared)
            total_ms += ms
            lm = LinkageMap(number, map_cls, edges, degree, informative)
            lm.groups = linkage_groups(M, taking, edges, min_group)
            for g in range(1, int(lm.groups.max()) + 1 if M else 1):
                members = np.nonzero(lm.groups == g)[0]
                if len(members) > max_order:
                    warnings.append("map {} group {}: {} markers, more than --max-order {}: written unordered".format(
                        number, g, len(members), max_order))
                    lm.order[g], lm.positions[g], lm.phases[g] = [int(m) for m in members], None, None
                    continue
                group_cls = np.full(M, LINK_NO_PART, dtype=np.uint8)
                group_cls[members] = map_cls[members]
                within, _, _, ms = pair_call(group_cls, 500000, LINK_LOD_MIN, 1, capacity=max(1, len(members) * (len(members) - 1) // 2))
                total_ms += ms
                lm.order[g], lm.positions[g], lm.phases[g] = linkage_order(members, within, min_shared)
            maps.append(lm)
    finally:
        if d_own:
            eng.dev_free(d_own)
    return LinkageResult(samples=samnames, markers=marknames, cross=cross, parents=parents, offspring=offspring, counts=counts,
                         map_of=map_of, cls=cls, a=a, b=b, o=o, verdict=verdict, maps=maps, warnings=warnings,
                         stats=dict(backend=backend, ms=total_ms, markers=M, offspring=len(offspring), max_rf_ppm=max_rf_ppm,
                                    min_lod16=min_lod16, min_shared=min_shared, max_chi2_milli=max_chi2_milli,
                                    max_other_ppm=max_other_ppm, min_group=min_group, max_order=max_order))


LINK_PAIR_COLUMNS = ("map", "marker_i", "marker_j", "n", "rec", "rf", "phase", "lod16", "lod")
LINK_MAP_COLUMNS = ("map", "group", "order", "marker", "position_cM", "phase")
LINK_STAT_COLUMNS = ("marker", "c0", "c1", "c2", "missing", "map", "class_a", "class_b", "a", "b", "other", "informative", "degree",
                     "group", "dropped")
_LINK_LOD_UNIT = 217705.98518566475               # 65536 log2 10: lod16 per unit of LOD


def writeLinkagePairs(filename, result):
    """One row per edge of every map: map, the two marker names, n, rec, rf = rec / n (six decimals), phase (C coupling /
    R repulsion), lod16 and the LOD (three decimals); CSV with a header row, csv.writer's CRLF rows."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(LINK_PAIR_COLUMNS)
        for lm in result.maps:
            for e, rec, ph in zip(lm.edges.tolist(), lm.rec.tolist(), lm.phase.tolist()):
                out.writerow([lm.number, result.markers[e[0]], result.markers[e[1]], e[2], rec, format(rec / e[2] if e[2] else 0.0, ".6f"),
                              "R" if ph else "C", e[4], format(e[4] / _LINK_LOD_UNIT, ".3f")])


def writeLinkageMap(filename, result):
    """One row per placed marker: map, group, order (from 1 along the chain), marker, position in centimorgans (three
    decimals) and phase (0 / 1 relative to the group's first marker); a group too large to order has blank order,
    position and phase.  CSV with a header row, csv.writer's CRLF rows."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(LINK_MAP_COLUMNS)
        for lm in result.maps:
            for g in sorted(lm.order):
                ordered = lm.positions[g] is not None
                for k, m in enumerate(lm.order[g]):
                    out.writerow([lm.number, g, k + 1 if ordered else "", result.markers[m],
                                  format(lm.positions[g][k], ".3f") if ordered else "", lm.phases[g][k] if ordered else ""])


def writeLinkageStats(filename, result):
    """One row per marker: its counts over the offspring, map, class pair, a, b, other, informative, degree and group
    (blank where it takes no part) and why it was dropped (blank: it takes part); CSV with a header row, CRLF rows."""
    by_map = {lm.number: lm for lm in result.maps}
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(LINK_STAT_COLUMNS)
        for m, name in enumerate(result.markers):
            k, v = int(result.map_of[m]), int(result.verdict[m])
            row = [name] + [int(x) for x in result.counts[m]] + [k]
            row += list(LINK_CLASSES[int(result.cls[m])]) + [int(result.a[m]), int(result.b[m]), int(result.o[m])] if v != 1 else [""] * 5
            lm = by_map.get(k)
            row += [int(lm.informative[m]), int(lm.degree[m]), int(lm.groups[m])] if v == 0 else [""] * 3
            out.writerow(row + [LINK_REASONS[v]])


# ---------------------------------------------------------------------------------------------------------------------
# Library QC: what one asks of a freshly sequenced library before anything else is worth running.
# Every statistic is an integer; backend="gpu" (csrc/qc.hip) and backend="host" give the same tables.
QC_STRIP = " \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"            # the counter's strip set (str.strip() of an ASCII line)
QC_BASE_CLASSES = ("A", "C", "G", "T", "N", "Other")
QC_STAT_NAMES = ("reads", "barcut", "qual_lines", "bases", "qual_bases", "qual_invalid", "empty_qual")
QC_PERCENTILES = (10, 25, 50, 75, 90)
QC_MAX_CYCLES = 1024


class QCResult:
    """What library_qc returns.  `.stats`: reads, barcut, qual_lines, bases, qual_bases, qual_invalid, empty_qual;
    numpy uint64 arrays `.barcodes` (B + 1 rows of reads, bases, reads with a non-ACGT character; the last row is "no
    barcode"), `.base_cycle` (C + 1 rows of A, C, G, T, N, other), `.qual_cycle` (C + 1 rows of Phred 0..93 and, in
    column 94, invalid bytes), `.lengths` (C + 1) and `.meanq` (94); row C of a per-cycle table holds positions >= C."""

    def __init__(self, stats, barcodes, base_cycle, qual_cycle, lengths, meanq, max_cycles):
        self.stats, self.barcodes, self.base_cycle, self.qual_cycle = stats, barcodes, base_cycle, qual_cycle
        self.lengths, self.meanq, self.max_cycles = lengths, meanq, max_cycles

    def cycle_quantiles(self, p):
        """Per row of qual_cycle: the smallest Phred value v with 100 * #(values <= v) >= p * n over the row's n valid
        values, in integers; None for a row without one."""
        out = []
        for row in self.qual_cycle:
            counts = [int(x) for x in row[:94]]
            n = sum(counts)
            if n == 0:
                out.append(None)
                continue
            seen = 0
            for v, c in enumerate(counts):
                seen += c
                if 100 * seen >= p * n:
                    out.append(v)
                    break
            else:                                      # (p > 100: no value reaches it)
                out.append(None)
        return out

    def cycle_means_x100(self):
        """Per row of qual_cycle: 100 * sum of the valid values // their number; None for a row without one."""
        out = []
        for row in self.qual_cycle:
            n = sum(int(x) for x in row[:94])
            out.append(None if n == 0 else 100 * sum(v * int(x) for v, x in enumerate(row[:94])) // n)
        return out


def _qc_host(fqfile, barcodes, cutsite, C, maxreads):
    """The QC rule line by line.  The file is read as the reference reads it with one record more than the bound, so
    that the last record's quality line is seen: through line 4 R + 1, or to the file's end."""
    import numpy as np
    from ._binding import NonAsciiSequence
    index = _census_host_index(barcodes, cutsite)
    keylens = sorted({len(s) for s in index})
    R = effective_maxreads(maxreads)
    B = len(barcodes)
    bar = [[0, 0, 0] for _ in range(B + 1)]
    base = [[0] * 6 for _ in range(C + 1)]
    qual = [[0] * 95 for _ in range(C + 1)]
    lengths = [0] * (C + 1)
    meanq = [0] * 94
    st = dict.fromkeys(QC_STAT_NAMES, 0)
    # (bytes.translate to class and bin numbers, then plain list cells: a numpy scalar add per byte is ten times slower)
    to_class = bytes(dict(zip(b"ACGTN", range(5))).get(v, 5) for v in range(256))
    to_bin = bytes(v - 33 if 33 <= v <= 126 else 94 for v in range(256))
    opener = _gzip.open if fqfile[-2:].lower() == 'gz' else open
    with opener(fqfile, 'rt', encoding='latin-1') as fh:
        for k, line in enumerate(fh):
            if k & 1 and (k >> 2) < R:
                if k & 3 == 1:
                    if any(ch >= '\x80' for ch in line):
                        raise NonAsciiSequence("non-ASCII byte in a sequence line")
                    line1 = line.strip(QC_STRIP).upper()
                    n = len(line1)
                    b = B
                    for m in keylens:
                        if n >= m and line1[:m] in index:
                            b = index[line1[:m]]
                            break
                    codes = line1.encode('latin-1').translate(to_class)
                    st["reads"] += 1
                    st["bases"] += n
                    st["barcut"] += b < B
                    row = bar[b]
                    row[0] += 1
                    row[1] += n
                    row[2] += codes.count(4) + codes.count(5) > 0
                    lengths[min(n, C)] += 1
                    for i, c in enumerate(codes[:C]):
                        base[i][c] += 1
                    if n > C:
                        tail, row = codes[C:], base[C]
                        for c in range(6):
                            row[c] += tail.count(c)
                else:
                    bins = line.strip(QC_STRIP).encode('latin-1').translate(to_bin)
                    invalid = bins.count(94)
                    nvalid = len(bins) - invalid
                    for i, v in enumerate(bins[:C]):
                        qual[i][v] += 1
                    if len(bins) > C:
                        tail, row = bins[C:], qual[C]
                        for v in set(tail):
                            row[v] += tail.count(v)
                    st["qual_lines"] += 1
                    st["qual_bases"] += nvalid
                    st["qual_invalid"] += invalid
                    if nvalid == 0:
                        st["empty_qual"] += 1
                    else:
                        meanq[(sum(bins) - 94 * invalid) // nvalid] += 1
            if k >= 4 * R + 1:
                break
    u = lambda x: np.array(x, dtype=np.uint64)
    bar, base, qual, lengths, meanq = u(bar), u(base), u(qual), u(lengths), u(meanq)
    return QCResult(st, bar, base, qual, lengths, meanq, C)


def library_qc(fqfile, barcodes, cutsite="TGCAG", max_cycles=160, maxreads=5e9, device=0, backend="gpu"):
    """Per-barcode and per-cycle statistics of one library (plain or .gz by name) in one pass -> QCResult.

    Lines are the counter's; record r is lines 4r .. 4r + 3 and the first `maxreads` records are looked at.  A sequence
    line is stripped and upper-cased (a byte >= 0x80 raises NonAsciiSequence); its barcode row comes from
    find_tags_fastq's barcode + cut site lookup, the last row taking the reads without one.  A quality line is stripped
    and its bytes 33..126 count as Phred 0..93, any other byte as invalid.  Positions >= max_cycles (1..1024) go to the
    tables' last row.  Every line is decided on its own: there is no per-barcode quality and no length comparison of a
    record's two lines.  backend="gpu": csrc/qc.hip; backend="host": the same rule in Python."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    C = int(max_cycles)
    if not 1 <= C <= QC_MAX_CYCLES:
        raise ValueError("max_cycles must be 1..1024")
    if backend == "host":
        return _qc_host(fqfile, barcodes, cutsite, C, maxreads)
    eng = default_engine(device)
    eng.qc_begin(barcodes, cutsite, C)
    try:
        eng.qc_file(fqfile, maxreads)
        stats = eng.qc_stats()
        tables = eng.qc_fetch()
    finally:
        try:
            eng.qc_end()
        except Exception:          # noqa: BLE001 -- the error that brought us here is the one to report
            pass
    return QCResult({k: stats[k] for k in QC_STAT_NAMES}, *tables, C)


def _qc_cycle_label(i, C):
    return str(i + 1) if i < C else ">{}".format(C)


def writeQCSamples(filename, libraries, results, barcodes, samples):
    """One row per barcode of every library and a last row `(none)` for its reads without barcode + cut site: Library,
    Barcode, Sample, Reads, Reads ppm of library (floor), Bases, Reads with non-ACGT.  `libraries`, `results`,
    `barcodes` and `samples` are lists with one entry per library.  CSV with a header row, csv.writer's CRLF rows."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(["Library", "Barcode", "Sample", "Reads", "Reads ppm of library", "Bases", "Reads with non-ACGT"])
        for lib, res, bars, sams in zip(libraries, results, barcodes, samples):
            total = res.stats["reads"]
            for k, row in enumerate(res.barcodes):
                r, n, a = (int(x) for x in row)
                last = k == len(bars)
                out.writerow([lib, "(none)" if last else bars[k], "(none)" if last else sams[k], r,
                              r * 1000000 // total if total else 0, n, a])


def writeQCCycles(filename, libraries, results):
    """One row per cycle of every library (the last, `>C`, for the positions beyond max_cycles): the six base counts,
    the valid and invalid quality bytes, their mean (100 * sum // n, two decimals) and the 10th, 25th, 50th, 75th and
    90th percentile; the quality cells of a cycle without a valid byte are empty."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(["Library", "Cycle"] + list(QC_BASE_CLASSES) + ["Quality values", "Invalid quality bytes", "Mean quality"] +
                     ["Q{}".format(p) for p in QC_PERCENTILES])
        for lib, res in zip(libraries, results):
            means = res.cycle_means_x100()
            quants = [res.cycle_quantiles(p) for p in QC_PERCENTILES]
            for i in range(res.max_cycles + 1):
                valid = sum(int(x) for x in res.qual_cycle[i][:94])
                mean = "" if means[i] is None else "{}.{:02d}".format(means[i] // 100, means[i] % 100)
                out.writerow([lib, _qc_cycle_label(i, res.max_cycles)] + [int(x) for x in res.base_cycle[i]] +
                             [valid, int(res.qual_cycle[i][94]), mean] + ["" if q[i] is None else q[i] for q in quants])


def writeQCLengths(filename, libraries, results):
    """Library, Length, Reads: the reads of every length 0 .. max_cycles - 1 and, as `>=C`, of the longer ones."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(["Library", "Length", "Reads"])
        for lib, res in zip(libraries, results):
            for n, c in enumerate(res.lengths):
                out.writerow([lib, n if n < res.max_cycles else ">={}".format(res.max_cycles), int(c)])


def writeQCQualityMatrix(filename, libraries, results):
    """The full cycle x Phred table: Library, Cycle, Q0 .. Q93, Invalid."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(["Library", "Cycle"] + ["Q{}".format(v) for v in range(94)] + ["Invalid"])
        for lib, res in zip(libraries, results):
            for i, row in enumerate(res.qual_cycle):
                out.writerow([lib, _qc_cycle_label(i, res.max_cycles)] + [int(x) for x in row])


# ---------------------------------------------------------------------------------------------------------------------
# Tag rescue: reads one or two substitutions from a known tag.
RESCUE_MAX_TAGLEN = 128
RESCUE_CLASSES = ("reads", "barcut", "exact", "rescued1", "rescued2", "ambiguous", "none")
RESCUE_STAT_NAMES = RESCUE_CLASSES + ("longest_run",)


class RescueResult:
    """What rescue_tags_fastq returns: rescued ([len(barcodes)][len(tags)], lists or a numpy uint32 array), stats (dict:
    reads, barcut, exact, rescued1, rescued2, ambiguous, none, longest_run), positions (128 ints: mismatches of the
    rescued reads by position in the tag), backend ("gpu" or "host": which of the two answered)."""

    def __init__(self, rescued, stats, positions, backend):
        self.rescued, self.stats, self.positions, self.backend = rescued, stats, positions, backend


def _rescue_check_tags(stored):
    """td_rescue_begin's checks of the stored tags, with the exceptions its error codes are raised as."""
    from ._binding import TagdigError
    if not stored:
        raise IndexError("list index out of range")
    for t in stored:
        if not t:
            raise IndexError("list index out of range")
        if len(t) > RESCUE_MAX_TAGLEN:
            raise TagdigError(-7, "tag longer than 128 bases")
    # sorted, the tags that begin the current one form a chain; of all pairs the one whose later tag comes first
    chain, bad = [], None
    for k in sorted(range(len(stored)), key=lambda i: (stored[i], i)):
        while chain and not stored[k].startswith(stored[chain[-1][0]]):
            chain.pop()
        low = k
        if chain:
            cand = max(k, chain[-1][1])
            bad = cand if bad is None else min(bad, cand)
            low = min(low, chain[-1][1])
        chain.append((k, low))
    if bad is not None:
        raise AssertionError("Problematic sequence: {}.  Likely due to overlapping tags.".format(bad))


def _rescue_longest_run(stored, K):
    """The longest run of tags that share one of the K + 1 parts of the device's index (len(stored) when the shortest
    tag leaves no part)."""
    P = min(32, min(len(t) for t in stored) // (K + 1))
    if P < 1:
        return len(stored)
    longest = 0
    for p in range(K + 1):
        runs = {}
        for t in stored:
            key = t[p * P:(p + 1) * P]
            runs[key] = runs.get(key, 0) + 1
        longest = max(longest, max(runs.values()))
    return longest


def _rescue_host(fqfile, barcodes, tags, cutsite, maxreads, K):
    """The rescue rule read by read: (rescued matrix as lists, statistics, positions, the matrix of the exact reads --
    with tags none of which begins another, what find_tags_fastq counts).  Every tag of a length is held against the
    window in one numpy comparison; a window seen before is answered from a dict."""
    import numpy as np
    from ._binding import NonAsciiSequence
    from .engine import rescue_index
    barcut, barnum, tagoff, stored = rescue_index(barcodes, tags, cutsite)
    index = _census_host_index(barcodes, cutsite)
    _rescue_check_tags(stored)
    lengths = sorted({len(s) for s in index})
    by_len = {}
    for t, s in enumerate(stored):
        by_len.setdefault(len(s), []).append(t)
    groups = [(n, np.array(ids), np.frombuffer("".join(stored[t] for t in ids).encode("ascii"), dtype=np.uint8).reshape(len(ids), n))
              for n, ids in sorted(by_len.items())]
    maxlen = groups[-1][0]
    bound = effective_maxreads(maxreads)
    rescued = [[0] * len(stored) for _ in range(barnum)]
    exact = [[0] * len(stored) for _ in range(barnum)]
    positions = [0] * RESCUE_MAX_TAGLEN
    st = dict.fromkeys(RESCUE_CLASSES, 0)
    memo = {}

    def classify(w):
        """(class, tag, mismatching positions) of a window"""
        best, who, several = K + 1, -1, False
        for n, ids, mat in groups:
            if n > len(w):
                break
            d = (mat != np.frombuffer(w[:n].encode("latin-1"), dtype=np.uint8)).sum(axis=1)
            m = int(d.min())
            if m == 0:
                return "exact", int(ids[int(d.argmin())]), ()
            if m <= best and m <= K:
                hits = np.flatnonzero(d == m)
                if m < best:
                    best, who, several = m, int(ids[hits[0]]), len(hits) > 1
                else:
                    several = True
        if who < 0:
            return "none", -1, ()
        if several:
            return "ambiguous", -1, ()
        t = stored[who]
        return "rescued{}".format(best), who, tuple(i for i in range(len(t)) if w[i] != t[i])

    opener = _gzip.open if fqfile[-2:].lower() == 'gz' else open
    with opener(fqfile, 'rt', encoding='latin-1') as fh:
        for k, line in enumerate(fh):
            if k % 4 != 1:
                continue
            st["reads"] += 1
            if any(ch >= '\x80' for ch in line):
                raise NonAsciiSequence("non-ASCII byte in a sequence line")
            line1 = line.strip().upper()
            b = -1
            for n in lengths:
                if line1[:n] in index and len(line1) >= n:
                    b = index[line1[:n]]
                    break
            if b != -1:
                st["barcut"] += 1
                w = line1[tagoff[b]:tagoff[b] + maxlen]
                if w not in memo:
                    memo[w] = classify(w)
                kind, t, where = memo[w]
                st[kind] += 1
                if kind == "exact":
                    exact[b][t] += 1
                elif t >= 0:
                    rescued[b][t] += 1
                    for i in where:
                        positions[i] += 1
            if st["reads"] >= bound:
                break
    st["longest_run"] = _rescue_longest_run(stored, K)
    return rescued, st, positions, exact


def rescue_tags_fastq(fqfile, barcodes, tags, cutsite="TGCAG", maxreads=5e9, max_mismatch=1, device=0, backend="gpu",
                      as_array=False):
    """Count the reads of one FASTQ file (plain or .gz by name) that find_tags_fastq drops because they lie 1 ..
    max_mismatch (1 or 2) substitutions from a known tag -> RescueResult.

    The set-up is find_tags_fastq's (asserts, every cut-site variant, the strip decision).  Per read with a barcode +
    cut site: w = the stripped, upper-cased line from where the tags are compared, a tag of n bases is a candidate iff
    n <= len(w), and its distance is the number of positions i < n with w[i] != tag[i] (a character outside ACGT
    mismatches every base; no indels, no qualities).  A candidate at distance 0: the read is `exact` -- the counter's,
    nothing is written.  Otherwise the smallest distance m decides: m <= max_mismatch and one tag attains it -> that
    cell of `.rescued`, `rescued<m>` and `.positions[i]` for every mismatching i; several tags attain it ->
    `ambiguous`; else `none`.  barcut == exact + rescued1 + rescued2 + ambiguous + none.

    The tags as compared must be 1..128 bases and none may equal or begin another (AssertionError naming the later tag).
    backend="gpu": csrc/rescue.hip.  An index in which more tags share one part than the device takes ("rescue_max_run")
    is answered by the host rule, as is a tag list too short for max_mismatch + 1 parts; `.backend` says which of the
    two it was.  backend="host": the same rule in Python."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    K = int(max_mismatch)
    if K not in (1, 2):
        raise ValueError("max_mismatch must be 1 or 2")
    answered_by = "host"
    if backend == "gpu":
        from ._binding import TagdigError
        eng = default_engine(device)
        try:
            eng.rescue_begin(barcodes, tags, cutsite, K)
            answered_by = "gpu"
        except TagdigError as exc:
            if exc.code != -7 or not exc.detail.startswith("tag rescue: run"):
                raise
    if answered_by == "gpu":
        try:
            eng.rescue_file(fqfile, maxreads)
            stats = eng.rescue_stats()
            matrix, pos = eng.rescue_fetch()
        finally:
            try:
                eng.rescue_end()
            except Exception:          # noqa: BLE001 -- the error that brought us here is the one to report
                pass
        rescued = matrix if as_array else matrix.tolist()
        positions = [int(x) for x in pos]
    else:
        rescued, stats, positions, _ = _rescue_host(fqfile, barcodes, tags, cutsite, maxreads, K)
        if as_array:
            import numpy as np
            rescued = np.array(rescued, dtype=np.uint32).reshape(len(barcodes), len(tags))
    return RescueResult(rescued, {k: stats[k] for k in RESCUE_STAT_NAMES}, positions, answered_by)


def writeRescueStats(filename, libraries, results):
    """One row per library: Library, the seven classes, and the rescued reads' share of the reads with barcode + cut
    site (six decimals; NA without any).  CSV with a header row, csv.writer's CRLF rows."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(["Library"] + list(RESCUE_CLASSES) + ["rescued_share"])
        for lib, res in zip(libraries, results):
            st = res.stats
            out.writerow([lib] + [st[k] for k in RESCUE_CLASSES] + [_rate_text(st["rescued1"] + st["rescued2"], st["barcut"])])


# ---------------------------------------------------------------------------------------------------------------------
# Barcode rescue (csrc/bcrescue.hip): the reads every other pass drops because their first bases are no
# barcode + cut site entry, brought back when they lie one or two substitutions from the entries of exactly one barcode.
BCRESCUE_CLASSES = ("reads", "exact", "rescued1", "rescued2", "ambiguous", "none")
BCRESCUE_STAT_NAMES = BCRESCUE_CLASSES + ("tagged", "min_entry_distance")
BCRESCUE_POSITIONS = 32
BCRESCUE_NO_PAIR = 64          # min_entry_distance of an index whose entries all belong to one row


def _bcrescue_entries(barcut, barnum):
    """The entries the index build leaves, in list order, as (sequence, row) -- of duplicates the first, an entry that
    extends an earlier one shadowed -- with the build's failures (what td_set_index reports)."""
    if not barcut:
        raise IndexError("list index out of range")
    if barnum == 1 and barcut == [""]:                 # (a lone empty sequence matches every base)
        return [(b, 0) for b in "ACGT"]
    if barcut[0] == "":
        raise IndexError("string index out of range")
    try:
        kept = _trie_survivors(barcut)
    except AssertionError as exc:
        pos = int(str(exc).split(":")[1].split(".")[0])
        raise AssertionError("Problematic sequence: {}.  Likely due to overlapping tags.".format(pos % barnum)) from None
    return [(seq, pos % barnum) for seq, pos in sorted(kept, key=lambda sp: sp[1])]


def _bcrescue_min_distance(entries):
    """The smallest Hamming distance between two entries of different rows, over the shorter one's length."""
    import numpy as np
    n = len(entries)
    width = max(len(s) for s, _ in entries)
    bases = np.zeros((n, width), dtype=np.uint8)
    for k, (s, _) in enumerate(entries):
        bases[k, :len(s)] = np.frombuffer(s.encode("ascii"), dtype=np.uint8)
    lens = np.array([len(s) for s, _ in entries])
    rows = np.array([r for _, r in entries])
    col = np.arange(width)
    best = BCRESCUE_NO_PAIR
    for i in range(n - 1):
        other = rows[i + 1:] != rows[i]
        if not other.any():
            continue
        shorter = np.minimum(lens[i], lens[i + 1:])
        d = ((bases[i + 1:] != bases[i]) & (col[None, :] < shorter[:, None])).sum(axis=1)
        best = min(best, int(d[other].min()))
    return best


def _bcrescue_host(fqfile, barcodes, tags, cutsite, maxreads, K):
    """The barcode-rescue rule read by read -> (matrix as lists, statistics).  The entries of one length are held
    against the read's first bases in one numpy comparison; a head seen before is answered from a dict."""
    from .engine import rescue_index
    barcut, barnum, tagoff, stored = rescue_index(barcodes, tags, cutsite)
    return _bcrescue_host_lists(fqfile, barcut, barnum, tagoff, stored, maxreads, K)


def _bcrescue_host_lists(fqfile, barcut, barnum, tagoff, stored, maxreads, K):
    """_bcrescue_host from the lists td_bcrescue_begin takes."""
    import numpy as np
    from ._binding import NonAsciiSequence
    entries = _bcrescue_entries(barcut, barnum)
    _rescue_check_tags(stored)
    for seq, row in entries:
        if len(seq) <= 2 * K:
            raise ValueError("barcode rescue: entry of {} bases leaves no room for {} mismatches (every entry must be longer than {})".format(
                len(seq), K, 2 * K))
    exact_index = {seq: row for seq, row in entries}
    lengths = sorted({len(s) for s in exact_index})
    by_len = {}
    for k, (seq, _) in enumerate(entries):
        by_len.setdefault(len(seq), []).append(k)
    groups = [(n, np.array(ids), np.frombuffer("".join(entries[k][0] for k in ids).encode("ascii"), dtype=np.uint8).reshape(len(ids), n))
              for n, ids in sorted(by_len.items())]
    entry_rows = np.array([r for _, r in entries])
    widest = groups[-1][0]
    tag_index = {t: k for k, t in enumerate(stored)}
    tag_lengths = sorted({len(t) for t in stored})
    bound = effective_maxreads(maxreads)
    matrix = [[0] * len(stored) for _ in range(barnum)]
    row_rescued = [[0, 0] for _ in range(barnum)]
    positions = [0] * BCRESCUE_POSITIONS
    st = dict.fromkeys(BCRESCUE_CLASSES + ("tagged",), 0)
    memo = {}

    def classify(head, length):
        """(class, entry, mismatching positions) of a read without an exact entry: head = its first bases, length = len(read)"""
        best, who = K + 1, []
        for n, ids, mat in groups:
            if n > length:
                break
            d = (mat != np.frombuffer(head[:n].encode("latin-1"), dtype=np.uint8)).sum(axis=1)
            m = int(d.min())
            if m <= K and m <= best:
                hits = [int(k) for k in ids[np.flatnonzero(d == m)]]
                who = hits if m < best else who + hits
                best = m
        if not who:
            return "none", -1, ()
        if len({int(entry_rows[k]) for k in who}) > 1:
            return "ambiguous", -1, ()
        k = min(who)                                    # of one row's variants that tie, the earliest in the list
        seq = entries[k][0]
        return "rescued{}".format(best), k, tuple(i for i in range(len(seq)) if head[i] != seq[i])

    opener = _gzip.open if fqfile[-2:].lower() == 'gz' else open
    with opener(fqfile, 'rt', encoding='latin-1') as fh:
        for k, line in enumerate(fh):
            if k % 4 != 1:
                continue
            st["reads"] += 1
            if any(ch >= '\x80' for ch in line):
                raise NonAsciiSequence("non-ASCII byte in a sequence line")
            line1 = line.strip().upper()
            if any(line1[:n] in exact_index and len(line1) >= n for n in lengths):
                st["exact"] += 1
            else:
                key = (line1[:widest], min(len(line1), widest))
                if key not in memo:
                    memo[key] = classify(*key)
                kind, e, where = memo[key]
                st[kind] += 1
                if e >= 0:
                    b = entries[e][1]
                    row_rescued[b][len(where) - 1] += 1
                    for i in where:
                        positions[i] += 1
                    w = line1[tagoff[b]:]
                    for n in tag_lengths:
                        if n <= len(w) and w[:n] in tag_index:
                            matrix[b][tag_index[w[:n]]] += 1
                            st["tagged"] += 1
                            break
            if st["reads"] >= bound:
                break
    st["min_entry_distance"] = _bcrescue_min_distance(entries)
    st["row_rescued"] = row_rescued
    st["positions"] = positions
    return matrix, st


def rescue_barcodes_fastq(fqfile, barcodes, tags, cutsite="TGCAG", maxreads=5e9, max_mismatch=1, device=0, backend="gpu",
                          as_array=False):
    """Count the reads of one FASTQ file (plain or .gz by name) that find_tags_fastq drops because their first bases are
    no barcode + cut site entry but lie 1 .. max_mismatch (1 or 2) substitutions from the entries of exactly one barcode
    -> (matrix [len(barcodes)][len(tags)], statistics).

    The set-up is find_tags_fastq's (asserts, every cut-site variant, the strip decision).  The entries are the barcode +
    cut site strings the index build leaves; entry k belongs to barcode k % len(barcodes).  Per read (stripped,
    upper-cased): an entry that is an exact prefix -> `exact`, the counter's read, nothing else.  Otherwise every entry
    no longer than the read is a candidate at the number of its positions that differ from the read (a character outside
    ACGT differs from every base; no indels, no qualities), and the smallest distance m decides: m > max_mismatch or no
    candidate -> `none`; entries of several barcodes at m -> `ambiguous` (cut-site variants of one barcode that tie are no
    tie: the earliest in the list counts); else the read is rescued into that barcode: `rescued<m>`, `row_rescued[b][m -
    1]`, `positions[i]` for every mismatching i, and the counter's tag step from where the tags are compared: the stored
    tag that begins the rest of the read gets the matrix cell and `tagged`.
    reads == exact + rescued1 + rescued2 + ambiguous + none.

    The statistics: those classes, `tagged`, `min_entry_distance` (the smallest distance between entries of two
    barcodes over the shorter one's length, 64 with one barcode: at or below max_mismatch, exact reads of one sample lie
    one error from rescue into another), `row_rescued` ([len(barcodes)][2]) and `positions` (32 ints).
    The tags follow rescue_tags_fastq's conditions.  Every entry must be longer than 2 * max_mismatch bases (ValueError).
    backend="gpu": csrc/bcrescue.hip; backend="host": the same rule in Python."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    K = int(max_mismatch)
    if K not in (1, 2):
        raise ValueError("max_mismatch must be 1 or 2")
    if backend == "host":
        matrix, stats = _bcrescue_host(fqfile, barcodes, tags, cutsite, maxreads, K)
        if as_array:
            import numpy as np
            matrix = np.array(matrix, dtype=np.uint32).reshape(len(barcodes), len(tags))
        return matrix, stats
    from ._binding import TagdigError
    eng = default_engine(device)
    try:
        eng.bcrescue_begin(barcodes, tags, cutsite, K)
    except TagdigError as exc:
        if exc.code == -7 and exc.detail.startswith("barcode rescue: entry"):
            raise ValueError(exc.detail) from None
        raise
    try:
        eng.bcrescue_file(fqfile, maxreads)
        stats = eng.bcrescue_stats()
        m, rows, pos = eng.bcrescue_fetch()
    finally:
        try:
            eng.bcrescue_end()
        except Exception:          # noqa: BLE001 -- the error that brought us here is the one to report
            pass
    stats["row_rescued"] = [[int(x) for x in r] for r in rows]
    stats["positions"] = [int(x) for x in pos]
    return (m if as_array else m.tolist()), stats


def writeBarcodeRescueStats(filename, libraries, results):
    """One row per library (results: the statistics dicts of rescue_barcodes_fastq): Library, the six classes, tagged,
    min_entry_distance, and the rescued reads' share of the reads without an exact entry (six decimals; NA without
    any).  CSV with a header row, csv.writer's CRLF rows."""
    with open(filename, mode='w', newline='') as fh:
        out = _csv.writer(fh)
        out.writerow(["Library"] + list(BCRESCUE_STAT_NAMES) + ["rescued_share"])
        for lib, st in zip(libraries, results):
            out.writerow([lib] + [st[k] for k in BCRESCUE_STAT_NAMES] + [_rate_text(st["rescued1"] + st["rescued2"], st["reads"] - st["exact"])])


# ---------------------------------------------------------------------------------------------------------------------
# Tag Manager (reference tagdigger_fun.py:1389-1905 and the prompts of :936-1028, :1182-1200).
#
# Every function keeps the reference's signature, return values, printed lines, files and exceptions.  Those with a
# data-parallel core take `device` and `backend` after them: backend="gpu" sorts (K2), looks up (K3) and compares tags
# (K4) on the device through tagdigger_amd.tagset; backend="host" is the plain restatement.  The device takes ACGT tags
# of at most 256 bases; a call with any other tag runs on the host as a whole.
import os as _os

from . import tagset as _ts

# codes for ambiguous nucleotides (reference :50-57)
IUPAC_codes = {frozenset('AG'): 'R', frozenset('CT'): 'Y',
               frozenset('GT'): 'K', frozenset('AC'): 'M',
               frozenset('CG'): 'S', frozenset('AT'): 'W',
               frozenset('CGT'): 'B', frozenset('AGT'): 'D',
               frozenset('ACT'): 'H', frozenset('ACG'): 'V',
               frozenset('ACGT'): 'N',
               frozenset('A'): 'A', frozenset('C'): 'C',
               frozenset('G'): 'G', frozenset('T'): 'T'}


def _use_device(backend, *seqlists):
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    return backend == "gpu" and _ts.device_takes(*seqlists)


_ACGT = frozenset('ACGT')


def _compare_positions(taglist, trim):
    """[p for p, _ in compareTags(taglist, trim)], same assertions, one zip over the columns."""
    assert type(taglist) is list, "taglist must be list."
    assert set("".join(taglist)) <= _ACGT, "taglist must be a list of ACGT strings."
    lengths = set(len(t) for t in taglist)
    if len(lengths) > 1 and not trim:
        width = max(lengths)
        return [i for i, col in enumerate(zip(*[t.ljust(width, 'N') for t in taglist])) if len(set(col) - {'N'}) > 1]
    taglist[0]
    return [i for i, col in enumerate(zip(*taglist)) if len(set(col)) > 1]


def _columns(groups, trim, device, on_device):
    """compareTags' column positions for every group, in order.  On the device (K4) a group with a byte outside ACGT
    is handed to compareTags itself, which raises the reference's AssertionError."""
    if not on_device:
        return [_compare_positions(g, trim) for g in groups]
    cols, bad = _ts.varsites(default_engine(device), groups, trim)
    for g, flag in enumerate(bad):
        if flag:
            compareTags(groups[g], trim=trim)
            raise AssertionError("taglist must be a list of ACGT strings.")
    return cols


def exportFasta(filename, namelist, seqlist, device=0, backend="gpu"):
    """FASTA of one record per marker, with IUPAC codes at the sites where its tags differ (reference :1389-1433)."""
    assert len(namelist) == len(seqlist), "List of marker names and list of tag sequences should be same length."
    assert all([set(t) <= set('ACGT') for t in seqlist]), "Tag sequences need to be ACGT."
    markers, alleles = extractMarkers(namelist)
    groups = [[seqlist[i] for i in a[1]] for a in alleles]
    multi = [g for g in groups if len(g) > 1]
    multicols = iter(_columns(multi, False, device, _use_device(backend, seqlist)))
    try:
        with open(filename, mode='w') as fh:
            for name, mtags in zip(markers, groups):
                if ' ' in name:
                    raise Exception("{}: Marker names cannot contain spaces.".format(name))
                fh.write('>' + name + '\n')
                if len(mtags) == 1:
                    fh.write(mtags[0] + '\n')
                    continue
                cols = next(multicols)
                first = mtags[0]
                fh.write(first[:cols[0]])
                for k, c in enumerate(cols):
                    letters = {t[c] for t in mtags if c < len(t)}
                    fh.write(IUPAC_codes[frozenset(letters)])
                    fh.write(first[c + 1:] if k == len(cols) - 1 else first[c + 1:cols[k + 1]])
                fh.write('\n')
    except IOError:
        print("Could not write file {}.".format(filename))
    except Exception as err:
        print(err.args[0])
        _os.remove(filename)
    return None


def varSitesByMarker(namelist, seqlist, device=0, backend="gpu"):
    """{marker: positions of its variable sites}, tags trimmed to the shortest (reference :1435-1448)."""
    markers, alleles = extractMarkers(namelist)
    groups = [[seqlist[i] for i in a[1]] for a in alleles]
    cols = _columns(groups, True, device, _use_device(backend, seqlist))
    return dict(zip(markers, cols))


def readSAM(filename, varDict=None):
    """{marker: (reference name, position, quality[, variable site positions])} from a SAM file of aligned markers;
    unaligned records are skipped (reference :1450-1488)."""
    result = dict()
    try:
        with open(filename, mode='r') as fh:
            for line in fh:
                if line[0] == '@':
                    continue
                cols = line.split()
                flag = int(cols[1])
                if flag in _SAM_UNALIGNED:
                    continue
                if varDict != None:
                    if flag in _SAM_REVERSE:
                        taglen = len(cols[9])
                        sites = [int(cols[3]) + taglen - 1 - i for i in varDict[cols[0]]]
                    else:
                        sites = [int(cols[3]) + i for i in varDict[cols[0]]]
                    result[cols[0]] = (cols[2], cols[3], cols[4], sites)
                else:
                    result[cols[0]] = (cols[2], cols[3], cols[4])
        return result
    except IOError:
        print("Could not read file {}.".format(filename))
        return None
    except IndexError:
        print("File {} in wrong format.".format(filename))
        return None


def _longest(tags):
    """The first of the longest tags (an empty list: IndexError, as in the reference)."""
    lengths = [len(t) for t in tags]
    return [t for t, n in zip(tags, lengths) if n == max(lengths)][0]


def _merged_from_columns(tags, positions):
    """The merged string of mergeTags from the tags and the variable columns compareTags(trim=False) found."""
    lengths = [len(t) for t in tags]
    longest = max(lengths)
    template = _longest(tags)
    assert len(positions) > 0, "All tags in set are identical."
    lo = min(positions)
    hi = max(positions) if len(set(lengths)) == 1 else longest - 1
    return template[:lo] + '[' + '/'.join(t[lo:hi + 1] for t in tags) + ']' + template[hi + 1:]


def mergeTags(tags):
    """One merged string, variable region in square brackets, variants separated by '/' (reference :1490-1507)."""
    _longest(tags)
    return _merged_from_columns(tags, [c[0] for c in compareTags(tags, trim=False)])


def mergedTagList(tags, device=0, backend="gpu"):
    """[marker names, merged strings], alleles of each marker in allele-name order; None after printing the reason
    when a marker has one tag or cannot be merged (reference :1509-1527)."""
    markers, alleles = extractMarkers(tags[0])
    try:
        if not all([len(a[1]) > 1 for a in alleles]):
            raise Exception("Each marker needs multiple tags.")
        groups = [[tags[1][ti] for _, ti in sorted(zip(a[0], a[1]))] for a in alleles]
        if not _use_device(backend, tags[1]):
            return [markers, [mergeTags(g) for g in groups]]
        cols, bad = _ts.varsites(default_engine(device), groups, False)
        merged = []
        for g, c, flag in zip(groups, cols, bad):
            if flag:
                compareTags(g, trim=False)
            merged.append(_merged_from_columns(g, c))
        return [markers, merged]
    except Exception as err:
        print(err.args[0])
        return None


def exportFasta2(filename, markernames, mergedstrings):
    """FASTA from merged strings of exactly two variants of equal length (reference :1529-1565, deprecated there)."""
    assert len(markernames) == len(mergedstrings), \
        "Must have same number of marker names and merged strings."
    try:
        with open(filename, mode='w') as fh:
            for name, merged in zip(markernames, mergedstrings):
                if ' ' in name:
                    raise Exception("{}: Marker names cannot contain spaces.".format(name))
                if not set(merged) <= set('[/]ACGT'):
                    raise Exception("{}: Unexpected character in merged string.".format(name))
                if not set('[/]') < set(merged):
                    raise Exception("{}: Square brackets and slash not found.".format(name))
                fh.write('>' + name + '\n')
                p1, p2, p3 = merged.find('['), merged.find('/'), merged.find(']')
                if p1 > p2 or p2 > p3:
                    raise Exception("{}: Square brackets and slash in wrong order.".format(name))
                fh.write(merged[:p1])
                v1, v2 = merged[p1 + 1:p2], merged[p2 + 1:p3]
                if len(v1) != len(v2):
                    raise Exception("{}: Variable regions are of different lengths.".format(name))
                for x, y in zip(v1, v2):
                    fh.write(IUPAC_codes[frozenset({x, y})])
                fh.write(merged[p3 + 1:] + '\n')
    except IOError:
        print("Could not write file {}.".format(filename))
    except Exception as err:
        print(err.args[0])
        _os.remove(filename)
    return None


def readTabularData(filename, markerDict=None, ignoreSeq=False):
    """[headers, {marker: row}] from a CSV with a 'Marker name' column; rows of one marker are merged, later
    non-blank cells winning (reference :1567-1606)."""
    try:
        with open(filename, 'r', newline='') as fh:
            data = dict()
            first = True
            for row in _csv.reader(fh):
                if first:
                    first = False
                    if "Marker name" not in row:
                        raise Exception("Need a 'Marker name' column header.")
                    mi = row.index("Marker name")
                    headers = row
                    headers.pop(mi)
                    if ignoreSeq:
                        si = row.index("Tag sequence")
                        headers.pop(si)
                    continue
                marker = row.pop(mi)
                if markerDict != None and marker in markerDict.keys():
                    marker = markerDict[marker]
                if ignoreSeq:
                    row.pop(si)
                if marker in data:
                    old = data[marker]
                    data[marker] = [row[i] if row[i].strip() != "" else old[i] for i in range(len(row))]
                else:
                    data[marker] = row
        return [headers, data]
    except IOError:
        print("Could not read file {}.".format(filename))
        return None
    except Exception as err:
        print(err.args[0])
        return None


def writeMarkerDatabase(filename, markernames, mergedseq, extracollist):
    """CSV: marker name, merged sequence, then the columns of each [headers, {marker: values}] in extracollist
    (reference :1608-1640)."""
    assert isinstance(extracollist, list), "extracollist must be a list (empty if not needed)."
    assert all([len(x) == 2 for x in extracollist]), "Each item in extracollist needs two components."
    assert all([isinstance(x[1], dict) for x in extracollist]), "extracollist needs dictionaries."
    try:
        with open(filename, 'w', newline='') as fh:
            out = _csv.writer(fh)
            header = ['Marker name', 'Tag sequence']
            for x in extracollist:
                header.extend(x[0])
            out.writerow(header)
            widths = [len(x[0]) for x in extracollist]
            for i in range(len(markernames)):
                m = markernames[i]
                row = [m, mergedseq[i]]
                for (_, d), width in zip(extracollist, widths):
                    row.extend(d[m] if m in d.keys() else ["" for _ in range(width)])
                out.writerow(row)
    except IOError:
        print("Could not write file {}.".format(filename))
    return None


def readMarkerDatabase(filename):
    """[tags as readTags_Merged gives them, [headers, {marker: row}]] of a database written by writeMarkerDatabase;
    None when it cannot be read (reference :1642-1660)."""
    print("Reading data...")
    try:
        tags = readTags_Merged(filename, allowDuplicates=True)
        if tags == None:
            raise IOError
        extra = readTabularData(filename, ignoreSeq=True)
        if extra == None:
            raise IOError
        return [tags, extra]
    except IOError:
        return None
    except Exception as err:
        print(err.args[0])
        return None


def _is_sorted(seqs):
    return all(seqs[i] <= seqs[i + 1] for i in range(len(seqs) - 1))


def lookupMarkerByTag(tagNamesSort, tagSeqSort, queryTags, allowDiffLengths=False, device=0, backend="gpu"):
    """The set of markers whose tags match the query tags of one marker, in the sorted tag list (reference
    :1662-1708; the set is filled in the reference's order, see tagset.add_walk)."""
    assert len(tagSeqSort) == len(tagNamesSort), "tagNamesSort and tagSeqSort not same length"
    out = set()
    if not queryTags:
        return out
    markers = [_ts.marker_of(x) for x in tagNamesSort]
    if (len(tagSeqSort) and _use_device(backend, tagSeqSort, queryTags) and _is_sorted(tagSeqSort)):
        st = _ts.SortedTags(default_engine(device), list(tagNamesSort), list(tagSeqSort), by_name=False)
        try:
            walks = st.walks(list(queryTags), allowDiffLengths)
        finally:
            st.close()
        for w in walks:
            _ts.add_walk(out, markers, w)
        return out
    for q in queryTags:
        _ts.add_walk(out, markers, _ts.walk_host(tagSeqSort, q, allowDiffLengths))
    return out


def sortTagsBySeq(tags, device=0, backend="gpu"):
    """[names, sequences] as tuples, in the order of sorted(zip(sequences, names)) (reference :1710-1714)."""
    if len(tags[1]) and len(tags[0]) == len(tags[1]) and _use_device(backend, tags[1]):
        st = _ts.SortedTags(default_engine(device), list(tags[0]), list(tags[1]))
        st.close()
        return [st.names, st.seqs]
    seqs, names = zip(*sorted(zip(tags[1], tags[0])))
    return [names, seqs]


class _Lookup:
    """Lookups of many query markers against one sorted tag set: all walks in one K3 launch on the device, or one
    by one on the host."""

    def __init__(self, names_sorted, seqs_sorted, queries, adl, st=None):
        self.markers = [_ts.marker_of(x) for x in names_sorted]
        self.seqs, self.adl = seqs_sorted, adl
        self.walks = None
        if st is not None:
            flat = [q for qs in queries for q in qs]
            self.walks = st.walks(flat, adl).tolist() if flat else []
            self.start = [0]
            for qs in queries:
                self.start.append(self.start[-1] + len(qs))

    def __call__(self, k, queries):
        out = set()
        if self.walks is None:
            for q in queries:
                _ts.add_walk(out, self.markers, _ts.walk_host(self.seqs, q, self.adl))
        else:
            for w in self.walks[self.start[k]:self.start[k + 1]]:
                _ts.add_walk(out, self.markers, w)
        return out


def _sorted_set(tags, device, on_device):
    """(sortTagsBySeq's [names, seqs], the device set or None)."""
    if on_device:
        st = _ts.SortedTags(default_engine(device), list(tags[0]), list(tags[1]))
        return [st.names, st.seqs], st
    return sortTagsBySeq(tags, backend="host"), None


def compareTagSets(oldtags, newtags, perfectMatch=False, allowDiffLengths=True, device=0, backend="gpu"):
    """{new marker: [old markers it matches]} (reference :1716-1751)."""
    on_device = len(oldtags[1]) > 0 and _use_device(backend, oldtags[1], newtags[1])
    old_sort, st = _sorted_set(oldtags, device, on_device)
    try:
        oldmarkers = extractMarkers(old_sort[0])
        newmarkers = extractMarkers(newtags[0])
        result = dict.fromkeys(set(newmarkers[0]))
        by_name = dict(zip(oldmarkers[0], range(len(oldmarkers[0]))))
        queries = [[newtags[1][i] for i in a[1]] for a in newmarkers[1]]
        lookup = _Lookup(old_sort[0], old_sort[1], queries, allowDiffLengths, st)
    finally:
        if st is not None:
            st.close()
    for k, name in enumerate(newmarkers[0]):
        result[name] = []
        theseseq = queries[k]
        found = lookup(k, theseseq)
        if perfectMatch and len(found) == 1:
            oldmarker = found.pop()
            oldseq = [old_sort[1][i] for i in oldmarkers[1][by_name[oldmarker]][1]]
            if allowDiffLengths:
                shortest = min([len(s) for s in theseseq + oldseq])
                oldseq = [s[:shortest] for s in oldseq]
                theseseq = [s[:shortest] for s in theseseq]
            if set(oldseq) == set(theseseq):
                result[name].append(oldmarker)
        elif not perfectMatch:
            result[name].extend(found)
    return result


def _absorb(theseseq, seqtoadd, allowDiffLengths):
    """Fold another marker's tags into theseseq (reference :1787-1797, :1822-1832): with allowDiffLengths a tag that
    is a shorter version of one already there is dropped and a longer version replaces the shorter one.  The list is
    changed while it is walked, exactly as the reference does."""
    if allowDiffLengths:
        for sNew in seqtoadd:
            for k in range(len(theseseq)):
                sOld = theseseq[k]
                if sOld.startswith(sNew):
                    if sNew in seqtoadd:
                        seqtoadd.remove(sNew)
                if sNew.startswith(sOld):
                    theseseq[k] = sNew
                    seqtoadd.remove(sNew)
    theseseq.extend(seqtoadd)


def _named_tags(markers, groups, device, on_device):
    """Tag names marker_alleles_index, alleles being the bases at compareTags' variable sites."""
    cols = _columns(groups, True, device, on_device)
    names = []
    for m, g, c in zip(markers, groups, cols):
        names.extend("{}_{}_{}".format(m, "".join(t[i] for i in c), k) for k, t in enumerate(g))
    return names


def consolidateTagSets(oldtags, newtags=None, allowDiffLengths=True, prefix="Mrkr", numdig=7, startnumnew=1,
                       device=0, backend="gpu"):
    """[consolidated tags, {marker: markers merged into it}]: markers that share tags are merged, first within
    oldtags, then (when given) newtags's consolidated markers into the old ones; unmatched new markers get new names
    (reference :1753-1860)."""
    on_device = len(oldtags[1]) > 0 and _use_device(backend, oldtags[1], *([newtags[1]] if newtags is not None else []))
    old_sort, st = _sorted_set(oldtags, device, on_device)
    try:
        oldmarkers = extractMarkers(oldtags[0])
        by_name = dict(zip(oldmarkers[0], range(len(oldmarkers[0]))))
        queries = [[oldtags[1][i] for i in a[1]] for a in oldmarkers[1]]
        lookup = _Lookup(old_sort[0], old_sort[1], queries, allowDiffLengths, st)
    finally:
        if st is not None:
            st.close()

    kept, groups, names_host = [], [], []
    merged_into = dict()
    absorbed = set()
    for k, name in enumerate(oldmarkers[0]):
        if name in absorbed:
            continue
        theseseq = list(queries[k])
        found = lookup(k, theseseq)
        assert name in found, "Marker {} not found in lookup".format(name)
        found.remove(name)
        for other in found:
            absorbed.add(other)
            di = by_name.get(other)
            assert di is not None and oldmarkers[0][di] == other, \
                "Duplicate marker mismatch at {} {}".format(name, other)
            extra = [oldtags[1][i] for i in oldmarkers[1][di][1] if oldtags[1][i] not in theseseq]
            _absorb(theseseq, extra, allowDiffLengths)
        kept.append(name)
        groups.append(theseseq)
        if not on_device:
            names_host.extend(_named_tags([name], [theseseq], device, False))
        merged_into[name] = sorted(found)
    old_cons = [_named_tags(kept, groups, device, True) if on_device else names_host, [s for g in groups for s in g]]
    print("{} markers consolidated into {} markers".format(len(oldmarkers[0]), len(merged_into)))
    if newtags == None:
        return [old_cons, merged_into]

    newtemp = consolidateTagSets(newtags, newtags=None, allowDiffLengths=allowDiffLengths, device=device,
                                 backend=backend)
    new_cons = newtemp[0]
    new_sort, st = _sorted_set(new_cons, device, on_device and len(new_cons[1]) > 0)
    try:
        newmarkers = extractMarkers(new_cons[0])
        new_by_name = dict(zip(newmarkers[0], range(len(newmarkers[0]))))
        oldmarkers = extractMarkers(old_cons[0])
        queries = [[old_cons[1][i] for i in a[1]] for a in oldmarkers[1]]
        lookup = _Lookup(new_sort[0], new_sort[1], queries, allowDiffLengths, st)
    finally:
        if st is not None:
            st.close()
    matched = set()
    names_out, groups, names_host = [], [], []
    for k, name in enumerate(oldmarkers[0]):
        theseseq = list(queries[k])
        for other in lookup(k, theseseq):
            matched.add(other)
            di = new_by_name[other]
            extra = [new_cons[1][i] for i in newmarkers[1][di][1] if new_cons[1][i] not in theseseq]
            _absorb(theseseq, extra, allowDiffLengths)
            merged_into[name].append(other)
            merged_into[name].extend(newtemp[1][other])
        names_out.append(name)
        groups.append(theseseq)
        if not on_device:
            names_host.extend(_named_tags([name], [theseseq], device, False))
    tagsOut = [_named_tags(names_out, groups, device, True) if on_device else names_host, [s for g in groups for s in g]]
    for k, name in enumerate(newmarkers[0]):
        if name in matched:
            continue
        newname = "{}{:0{width}}".format(prefix, startnumnew, width=numdig)
        startnumnew += 1
        tagsOut[0].extend(new_cons[0][i].replace(name, newname) for i in newmarkers[1][k][1])
        tagsOut[1].extend(new_cons[1][i] for i in newmarkers[1][k][1])
        merged_into[newname] = [name]
        merged_into[newname].extend(newtemp[1][name])
    print("{} markers consolidated into {} markers".format(len(oldmarkers[0]) + len(newmarkers[0]),
                                                           len(merged_into)))
    return [tagsOut, merged_into]


def allColumns(extracollist):
    """Every column header of an extracollist, in order (reference :1862-1867)."""
    out = []
    for x in extracollist:
        out.extend(x[0])
    return out


def consolidateExtraCols(extracollist):
    """Merge columns that share a header; later tables overwrite earlier ones (reference :1869-1905)."""
    ac = allColumns(extracollist)
    while len(set(ac)) < len(ac):
        ntab = len(extracollist)
        for j in range(0, ntab - 1):
            for k in range(j + 1, ntab):
                hj, hk = extracollist[j][0], extracollist[k][0]
                if len(set(hj) & set(hk)) == 0:
                    continue
                onlyJ = [e for e in hj if e not in hk]
                onlyK = [e for e in hk if e not in hj]
                shared = [e for e in hj if e in hk]
                newJ, newK, both = [onlyJ, dict()], [onlyK, dict()], [shared, dict()]
                for src, dst, hdr in ((extracollist[j], newJ, hj), (extracollist[k], newK, hk)):
                    own = [hdr.index(e) for e in dst[0]]
                    common = [hdr.index(e) for e in shared]
                    for m in src[1].keys():
                        dst[1][m] = [src[1][m][i] for i in own]
                        both[1][m] = [src[1][m][i] for i in common]
                extracollist[j] = newJ
                extracollist[k] = newK
                extracollist.append(both)
        extracollist = [x for x in extracollist if len(x[0]) > 0]
        ac = allColumns(extracollist)
    return extracollist


# ------------------------------------------------------------------ prompts (reference :936-1028, :1182-1200)
_TAG_FORMATS = '''
Available tag file formats are:
  1: UNEAK FASTA
  2: Merged tags
  3: Tags in columns
  4: Tags in rows
  5: Stacks catalog
  6: SAM file for TASSEL-GBSv2 pipeline
  7: pyRAD .alleles output
'''


def _ask(prompt, allowed, upper=True):
    answer = None
    while answer not in allowed:
        answer = input(prompt).strip()
        if upper:
            answer = answer.upper()
    return answer


def readTags_interactive():
    """Ask for an optional list of marker names, a tag file format and its file(s); read the tags."""
    toKeep = None
    print('''
Do you wish to supply a list of marker names?  If provided, this list
will be used to subset the list of markers in the tag file.''')
    choice = ""
    while choice.upper() not in {'Y', 'N'}:
        choice = input("Y/N: ").strip()
    print("")
    if choice.upper() == 'Y':
        while toKeep == None:
            toKeep = readMarkerNames(input("File name: ").strip())
        print('''
File contains {} marker names.'''.format(len(toKeep)))
        for name in toKeep[:10]:
            print(name)
        if len(toKeep) > 10:
            print('...')
    print(_TAG_FORMATS)
    simple = {'1': readTags_UNEAK_FASTA, '2': readTags_Merged, '3': readTags_Columns, '4': readTags_Rows}
    tags = None
    while tags == None:
        fmt = '0'
        while fmt not in {'1', '2', '3', '4', '5', '6', '7'}:
            fmt = input("Enter the number of the format of your tag file: ").strip()
        if fmt == '5':
            tagsfile = input("Enter the name of the *.catalog.tags.tsv file: ").strip()
            snpsfile = input("Enter the name of the *.catalog.snps.tsv file: ").strip()
            allelesfile = input("Enter the name of the *.catalog.alleles.tsv file: ").strip()
            version = ""
            while version not in {"1", "2"}:
                version = input("Enter Stacks version (1 or 2): ").strip()[0]
            binary = _ask("Only retain binary markers? y/n: ", {'Y', 'N'})
            tags = readTags_Stacks(tagsfile, snpsfile, allelesfile, toKeep=toKeep,
                                   binaryOnly=binary == 'Y', version=int(version))
        elif fmt == '6':
            tagfile = input("Enter the file name: ").strip()
            binary = _ask("Only retain binary markers? y/n: ", {'Y', 'N'})
            mono = 'Y' if binary == 'Y' else _ask("Eliminate monomorphic markers? y/n: ", {'Y', 'N'})
            keychoice = _ask("Output a key file matching TASSEL-GBSv2 SNP names to TagDigger marker names? y/n: ",
                             {'Y', 'N'})
            keyfile = input("File name for CSV file with key: ").strip() if keychoice == 'Y' else None
            print("Reading {}...".format(tagfile))
            tags = readTags_TASSELSAM(tagfile, toKeep=toKeep, binaryOnly=binary == 'Y', noMonomorphic=mono == 'Y',
                                      writeMarkerKey=keychoice == 'Y', keyfilename=keyfile)
        elif fmt == '7':
            tagfile = input("Enter the file name: ").strip()
            binary = _ask("Only retain binary markers? y/n: ", {'Y', 'N'})
            print("Reading {}...".format(tagfile))
            tags = readTags_pyRAD(tagfile, toKeep=toKeep, binaryOnly=binary == 'Y')
        else:
            tagfile = input("Enter the file name: ").strip()
            tags = simple[fmt](tagfile, toKeep=toKeep)
        print('')
    print("{} tag sequences read.\n".format(len(tags[1])))
    return tags


def set_directory_interactive():
    """Offer to change the working directory, then list its contents."""
    print("\nCurrent directory is:")
    print(_os.getcwd())
    choice = ""
    while choice.upper() not in {'Y', 'N'}:
        choice = input("Use different directory for reading and writing files? (y/n) ").strip()
    if choice.upper() == 'Y':
        target = ""
        while not _os.path.isdir(target):
            target = input("New directory: ")
        _os.chdir(target)
    print("\nContents of current directory:")
    for entry in _os.listdir('.'):
        print(entry)
    return None


# ------------------------------------------------------------------ MD5 sums of the split files (reference :1370-1386)
# Shortest file list that backend="gpu" hashes on the device (one file per lane, csrc/md5.hip); None: no list is.
# Measured (profiles/md5/bench_mi355x.txt) at 1, 8, 64, 96 and 384 files of 16.6 MB: 384 is the shortest list at which
# the device route beat the host's 16 threads by more than the spread between rounds (0.30 against 0.43 s, spread 6 %);
# at 96 files it lost (0.21 against 0.11 s): a lane hashes 0.1 GB/s, so the lanes must outnumber the cores' lead.
_MD5_DEVICE_MIN_FILES = 384
_MD5_HOST_THREADS = 16


def _md5_file_host(path):
    import hashlib
    m = hashlib.md5()
    with open(path, 'rb') as con:
        while True:
            chunk = con.read(8 * 1048576)
            if chunk == b'':
                break
            m.update(chunk)
    return m.hexdigest()


def _md5_on_device(backend, nfiles):
    return backend == "gpu" and _MD5_DEVICE_MIN_FILES is not None and nfiles >= _MD5_DEVICE_MIN_FILES


def _md5_hex(filelist, device, on_device):
    """(hexdigest of every file in front of the first one that cannot be read, that file's index or None)."""
    if not filelist:
        return [], None
    if on_device:
        from ._binding import TagdigError
        try:
            digests, _ = default_engine(device).md5_files(filelist)
        except TagdigError as err:
            if err.code != -11:
                raise
            bad = err.bad_index
            done, earlier = _md5_hex(filelist[:bad], device, True)
            return done, bad if earlier is None else earlier
        return [d.hex() for d in digests], None
    from concurrent.futures import ThreadPoolExecutor     # (hashlib releases the GIL while it hashes)

    def job(path):
        try:
            return _md5_file_host(path)
        except OSError as err:
            return err
    with ThreadPoolExecutor(max_workers=min(_MD5_HOST_THREADS, len(filelist))) as pool:
        results = list(pool.map(job, filelist))
    for k, r in enumerate(results):
        if not isinstance(r, str):
            return results[:k], k
    return results, None


def writeMD5sums(filelist, outfile, device=0, backend="gpu"):
    """CSV of file names and MD5 checksums, and one right-aligned line per file on stdout (reference :1370-1386).
    backend="gpu" hashes a list of _MD5_DEVICE_MIN_FILES files or more on the device, one file per lane
    (td_md5_files); a shorter list, and backend="host", on a pool of host threads.  A file that cannot be opened raises
    what the reference's open() raises, after the rows and lines of the files in front of it."""
    if backend not in ("gpu", "host"):
        raise ValueError("backend must be 'gpu' or 'host'")
    maxfilelen = max([len(f) for f in filelist])
    with open(outfile, mode='w', newline='') as csvcon:
        cw = _csv.writer(csvcon)
        cw.writerow(["File name", "MD5 sum"])
        sums, failed = _md5_hex(list(filelist), device, _md5_on_device(backend, len(filelist)))
        for f, digest in zip(filelist, sums):
            cw.writerow([f, digest])
            print("{:>{width}} {}".format(f, digest, width=maxfilelen))
        if failed is not None:
            open(filelist[failed], 'rb').close()
            raise OSError("cannot read {}".format(filelist[failed]))
    return None


def remove_monomorphic_loci(namelist, seqlist, verbose=False):
    """[names, sequences] of the tags whose marker has more than one tag, marker by marker (reference :1907-1924)."""
    assert len(namelist) == len(seqlist)
    keep = [i for _, indices in extractMarkers(namelist)[1] if len(indices) > 1 for i in indices]
    if verbose:
        print("{} tags removed belonging to monomorphic loci".format(len(seqlist) - len(keep)))
    return [[namelist[i] for i in keep], [seqlist[i] for i in keep]]
