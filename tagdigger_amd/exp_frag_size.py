#!/usr/bin/env python3
"""Expected fragment sizes from a genome, with the flags of the reference's exp_frag_size.py (:25-33): for every tag of a
SAM file, the distance from the tag's position to the nearest restriction site in the genome, the fragment's GC content
and its sequence, as CSV.

    python -m tagdigger_amd.exp_frag_size -s tags.sam -g genome.fa[.gz] -o out.csv [-c CTGCAG,CCGG] [-e PstI-MspI]
    python -m tagdigger_amd.exp_frag_size -s tags.sam -d genome_dir/ ...

The work is split in three:
  plan    (host)   the SAM reader (:75-135), the genome files and how each is read, the record bookkeeping of the
                   reference's header loop (:153-175: renaming, which records are searched, the jobs in its order) and
                   every job's window by Python's slice rules;
  search           the device -- K1 frames each genome file in HBM (td_fasta_frame_device), K2 searches every window
                   (td_frag_search_device), K3 gathers the fragments kept (td_frag_gather_device) -- or the host
                   restatement (str slicing and str.find), used for a genome file holding a byte >= 0x80 (which the
                   reference decodes with the locale's codec), an empty cut site, more than 16 cut sites, and
                   --td-backend host;
  write            the jobs applied in order with the reference's overwrite rule (:186-197), its progress lines
                   (:198-200) and the CSV (:206-212).
Flags that exist only in this build carry a --td- prefix and never change the results.
"""
import argparse
import bisect
import csv
import gzip
import mmap
import os
import re
import sys
import time

from .tagdigger_fun import adapters

DEFCS = 'CTGCAG,CCGG'
DEFENZ = 'PstI-MspI'
MAXFRAG = 3000
_COMP = str.maketrans("ACGT", "TGCA")


class _NeedHost(Exception):
    """A genome file the device does not frame (a byte >= 0x80): the whole run goes to the host restatement."""


def build_parser():
    ap = argparse.ArgumentParser(description="TagDigger script for estimating DNA fragment sizes (MI355X build)")
    ap.add_argument('-s', '--samfile', help='SAM file of tags to evaluate', required=True)
    ap.add_argument('-g', '--genomefile', help='FASTA file of reference genome')
    ap.add_argument('-d', '--genome_dir', help='Directory with multiple FASTA files of reference genome')
    ap.add_argument('-o', '--outfile', help='CSV output file', default='out.csv')
    ap.add_argument('-c', '--cutsites', help='Comma-delimited list of restriction sites', default=DEFCS)
    ap.add_argument('-e', '--enzymes', help='Name of enzyme pair', default=DEFENZ)
    ap.add_argument('-w', '--working_dir', help='Directory for reading and writing files')
    ap.add_argument('--td-device', type=int, default=0, help="GPU to run on (this build only)")
    ap.add_argument('--td-backend', choices=["gpu", "host"], default="gpu",
                    help="host: the host restatement of the search, no GPU (this build only; same output)")
    ap.add_argument('--td-timing', action='store_true', help="print where the wall time went, per stage (this build only)")
    return ap


# ------------------------------------------------------------------ plan: arguments, SAM, genome files
def genome_files(args):
    """(paths, short names) as at :44-54."""
    if (args.genomefile is None) == (args.genome_dir is None):
        raise Exception("Must provide either one file for reference genome (-g) or directory with multiple files (-d).")
    if args.genomefile is not None:
        return [args.genomefile], []
    names = os.listdir(args.genome_dir)
    return [os.path.join(args.genome_dir, x) for x in names], [x.split('.')[0] for x in names]


def cut_sites(args):
    """The cut sites of :57-70 and their exceptions."""
    if args.enzymes == DEFENZ:
        sites = [x.strip().upper() for x in args.cutsites.split(',')]
        if not set("".join(sites)) <= set('ACGT'):
            raise Exception("Non-ACGT cutsites listed.")
        return sites
    names = [k for k in adapters.keys() if k.startswith(args.enzymes)]
    if not names:
        raise Exception("Enzymes {} not found.  See 'adapters' in tagdigger_fun.py.".format(args.enzymes))
    sites = [a[0].replace("^", "") for a in adapters[names[0]]]
    if args.cutsites != DEFCS and sorted(sites) != sorted(x.strip().upper() for x in args.cutsites.split(',')):
        raise Exception("Cutsites and enzymes don't match.  Only one of these arguments is needed")
    return sites


def _cigar_sum(cigar, op):
    return sum(int(x) for x in re.findall(r"(\d+)" + op, cigar)) if op in cigar else 0


class Tags:
    """The columns the reference keeps per marker (:74-80)."""

    def __init__(self):
        self.names, self.seqnames, self.positions, self.forward, self.aligned, self.tagsizes = [], [], [], [], [], []

    def add(self, name, seqname, pos, forward, aligned, tagsize):
        self.names.append(name)
        self.seqnames.append(seqname)
        self.positions.append(pos)
        self.forward.append(forward)
        self.aligned.append(aligned)
        self.tagsizes.append(tagsize)


def read_sam(path):
    """The SAM reader of :83-135, field for field in the same order (so that a malformed line raises what the
    reference raises), UNEAK query / hit pairs included."""
    tags = Tags()
    q = None                                   # the last UNEAK query line: (marker, sequence, position, aligned, forward)
    with open(path, 'r') as fh:
        for line in fh:
            if line[0] == '@':
                continue
            f = line.split("\t")
            is_q = f[0][-8:-3] == "query"
            is_h = f[0][-6:-3] == "hit"
            name, seqname, pos = f[0], f[2], int(f[3])
            bits = bin(int(f[1]))[2:]
            aligned = len(bits) < 3 or bits[-3] == '0'
            forward = len(bits) < 5 or bits[-5] == '0'
            cigar = f[5]
            tagsize = len(f[9])
            dels, ins, clip = _cigar_sum(cigar, "D"), _cigar_sum(cigar, "I"), _cigar_sum(cigar, "S")
            pos = pos - clip if forward else pos + tagsize - 1 - ins + dels - clip
            if is_q:
                q = (name.split("_")[0], seqname, pos, aligned, forward)
            if is_h:
                marker = name.split("_")[0]
                if q is None:
                    raise NameError("name 'Qmrkr' is not defined")
                assert marker == q[0], "UNEAK marker names don't match."
                if aligned and seqname == q[1] and pos == q[2] and forward == q[4]:
                    tags.add(marker, seqname, pos, forward, aligned, tagsize)
                else:
                    tags.add(marker, "*", 0, True, False, tagsize)
            if not is_q and not is_h:
                tags.add(name, seqname, pos, forward, aligned, tagsize)
    return tags


# ------------------------------------------------------------------ genome reading
def _is_gz(path):
    return path.endswith(".gz")               # :159, case-sensitive


def read_host(path):
    """One genome file the way the reference reads it (:158-189): text mode, headers and line.strip().upper().
    -> (text, [(name, offset in text)], the exception that ended the reading or None)."""
    try:
        fh = gzip.open(path, 'rt') if _is_gz(path) else open(path, 'r')
    except Exception as e:                     # noqa: BLE001 -- re-raised where the reference raises it
        return "", [], e
    parts, events, n, exc = [], [], 0, None
    try:
        for line in fh:
            if line[0] == ">":
                events.append((line[1:].strip(), n))
            else:
                s = line.strip().upper()
                parts.append(s)
                n += len(s)
    except Exception as e:                     # noqa: BLE001
        exc = e
    finally:
        fh.close()
    return "".join(parts), events, exc


class HostGenome:
    """The host restatement: the genome as one str."""
    kind = "host"

    def __init__(self, paths):
        self.files = []                        # (events with global offsets, exception)
        parts, base = [], 0
        for p in paths:
            text, events, exc = read_host(p)
            parts.append(text)
            self.files.append(([(nm, base + o) for nm, o in events], exc))
            base += len(text)
            if exc is not None:
                break
        self.text = "".join(parts)

    def close(self):
        pass


def _gunzip(eng, path):
    """A .gz genome file's text through the project's decoders, or raises what gzip.open would."""
    from . import _binding as B
    size = os.path.getsize(path)
    if size >= 8 << 20:
        cap = 8 * size + (1 << 20)
        while True:
            try:
                got = eng.gunzip_file_gpu(path, cap)
                break
            except B.TagdigError as e:
                if e.code != -7:
                    raise
                cap *= 2
        if got is not None:
            return got
    import ctypes as C
    cap = max(4 * size, 1 << 16)
    with open(path, 'rb') as fh:
        if size >= 4:
            fh.seek(-4, 2)
            cap = max(cap, int.from_bytes(fh.read(4), "little") + 16)
    L = B.load()
    while True:
        buf = (C.c_uint8 * cap)()
        n = C.c_uint64(0)
        rc = L.td_gunzip_file(path.encode(), buf, cap, 0, C.byref(n))
        if rc == -7:
            cap *= 2
            continue
        B.check(rc)
        return bytes(memoryview(buf)[:n.value])


class DeviceGenome:
    """Every genome file framed by K1 into ONE device buffer (the reference's `sequence` carries over from file to
    file, so a record may span files); stays resident for the searches."""
    kind = "gpu"

    def __init__(self, eng, paths, timing=None):
        self.eng, self.files, self.d_seq, self.nbytes = eng, [], None, 0
        self.k1_ms = 0.0
        sources = []                           # per file: ("plain", size) | ("bytes", data) | ("host", text, events, exc)
        for p in paths:
            if _is_gz(p):
                try:
                    open(p, 'rb').close()
                    src = ("bytes", _gunzip(eng, p))
                except Exception:              # noqa: BLE001 -- the reference's own reading says how this file ends
                    text, events, exc = read_host(p)
                    src = ("host", text, events, exc)
            else:
                try:
                    open(p, 'rb').close()
                    src = ("plain", os.path.getsize(p))
                except Exception:              # noqa: BLE001
                    src = ("host",) + read_host(p)
            sources.append(src)
            if src[0] == "host":
                if not src[1].isascii():
                    raise _NeedHost(p)
                if src[3] is not None:
                    break
        sizes = [s[1] if s[0] == "plain" else len(s[1]) for s in sources]
        cap = sum(sizes) + 16
        try:
            self.d_seq = eng.dev_alloc(cap)
        except Exception as e:                 # noqa: BLE001
            raise MemoryError("the normalised genome needs up to %d bytes of device memory, which could not be "
                              "allocated (%s)" % (cap, e)) from None
        d_in, in_cap = None, 0
        try:
            base = 0
            for p, src in zip(paths, sources):
                if src[0] == "host":
                    eng.h2d(self.d_seq + base, src[1].encode("ascii"))
                    self.files.append(([(nm, base + o) for nm, o in src[2]], src[3]))
                    base += len(src[1])
                    continue
                n = src[1] if src[0] == "plain" else len(src[1])
                if n + 16 > in_cap:
                    if d_in:
                        eng.dev_free(d_in)
                        d_in = None
                    in_cap = n + 16
                    d_in = eng.dev_alloc(in_cap)
                if src[0] == "plain":
                    if n:
                        eng.load_file_range(p, 0, n, d_in)
                    host = None
                else:
                    eng.h2d(d_in, src[1])
                    host = src[1]
                nout, rows, nonascii, ms = eng.fasta_frame_device(d_in, n, self.d_seq + base, 4096)
                self.k1_ms += ms
                if nonascii:
                    raise _NeedHost(p)
                events = []
                if len(rows):
                    if host is None:
                        with open(p, 'rb') as fh:
                            host = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
                    events = [(host[int(lo):int(hi)].decode("ascii"), base + int(off)) for lo, hi, off in rows.tolist()]
                    if isinstance(host, mmap.mmap):
                        host.close()
                self.files.append((events, None))
                base += nout
            self.nbytes = base
        except BaseException:
            self.close()
            raise
        finally:
            if d_in:
                eng.dev_free(d_in)

    def close(self):
        if self.d_seq:
            self.eng.dev_free(self.d_seq)
            self.d_seq = None


# ------------------------------------------------------------------ plan: the header loop
def plan_jobs(tags, genome, gfshort):
    """The reference's header loop (:160-189) over the recorded headers: -> (numpy arrays of the jobs in the
    reference's order -- tag index, window [lo, hi) in the genome, reverse flag --, the exception to raise after them)."""
    import numpy as np
    nm = len(tags.names)
    seqsort = sorted(tags.seqnames)
    by_name = {}
    for i, s in enumerate(tags.seqnames):
        by_name.setdefault(s, []).append(i)
    job_tag, job_rlo, job_rhi = [], [], []
    cur = new = ""
    start = 0
    exc = None
    for i, (events, file_exc) in enumerate(genome.files):
        for name, pos in events:
            cur, new = new, name
            b = bisect.bisect_left(seqsort, new)
            try:
                if (b >= nm or seqsort[b] != new) and len(gfshort) > 0 and \
                        seqsort[bisect.bisect_left(seqsort, gfshort[i])] == gfshort[i]:
                    new = gfshort[i]
            except IndexError as e:
                exc = e
                break
            if pos == start:
                continue
            for t in by_name.get(cur, ()):
                job_tag.append(t)
                job_rlo.append(start)
                job_rhi.append(pos)
            start = pos
        if exc is None:
            exc = file_exc
        if exc is not None:
            break
    tag = np.array(job_tag, dtype=np.int64)
    rlo = np.array(job_rlo, dtype=np.int64)
    rhi = np.array(job_rhi, dtype=np.int64)
    pos = np.array(tags.positions, dtype=np.int64)[tag] if nm else np.zeros(0, np.int64)
    fwd = np.array(tags.forward, dtype=bool)[tag] if nm else np.zeros(0, bool)
    length = rhi - rlo
    a = np.where(fwd, pos - 1, np.maximum(0, pos - MAXFRAG))
    b = np.where(fwd, pos + MAXFRAG, pos)
    a, b = _slice_bound(a, length), _slice_bound(b, length)
    lo = rlo + a
    hi = rlo + np.maximum(a, b)
    return tag, lo, hi, ~fwd, exc


def _slice_bound(x, length):
    """slice(x, ...).indices(length) for one bound (step 1): negative counts from the end, then clamped to [0, length]."""
    import numpy as np
    x = np.where(x < 0, x + length, x)
    return np.clip(x, 0, length)


# ------------------------------------------------------------------ search
def search_host(genome, tags, sites, tag, lo, hi, rev):
    """The search of :183-195 as the reference writes it, per job: (sizes, G + C, N, fragments by job)."""
    import numpy as np
    text = genome.text
    size = np.full(len(tag), -1, dtype=np.int64)
    gc = np.zeros(len(tag), dtype=np.int64)
    nn = np.zeros(len(tag), dtype=np.int64)
    frags = {}
    for j in range(len(tag)):
        sub = text[lo[j]:hi[j]]
        if rev[j]:
            sub = sub.translate(_COMP)[::-1]
        ts = tags.tagsizes[tag[j]]
        best = None
        for cs in sites:
            k = sub.find(cs, ts - len(cs))
            if k != -1 and (best is None or k + len(cs) < best):
                best = k + len(cs)
        if best is not None:
            frag = sub[:best]
            size[j] = best
            gc[j] = frag.count('G') + frag.count('C')
            nn[j] = frag.count('N')
            frags[j] = frag
    return size, gc, nn, lambda idx: [frags[j] for j in idx]


def search_device(genome, tags, sites, tag, lo, hi, rev, stage_ms):
    import numpy as np
    from .engine import frag_job_dtype
    jobs = np.zeros(len(tag), dtype=frag_job_dtype())
    jobs["lo"], jobs["hi"], jobs["reverse"] = lo, hi, rev
    if len(tag):
        jobs["tagsize"] = np.minimum(np.array(tags.tagsizes, dtype=np.int64)[tag], 1 << 20)
    out, ms = genome.eng.frag_search_device(genome.d_seq, genome.nbytes, jobs, sites)
    stage_ms["K2"] = ms

    def fragments(idx):
        idx = np.asarray(idx, dtype=np.int64)
        sizes = out[idx, 0]
        blob, ms3 = genome.eng.frag_gather_device(genome.d_seq, genome.nbytes, jobs[idx], sizes)
        stage_ms["K3"] = ms3
        text = blob.decode("ascii")
        ends = np.cumsum(np.maximum(sizes, 0))
        starts = ends - np.maximum(sizes, 0)
        return [text[s:e] for s, e in zip(starts.tolist(), ends.tolist())]
    return out[:, 0].astype(np.int64), out[:, 1].astype(np.int64), out[:, 2].astype(np.int64), fragments


# ------------------------------------------------------------------ write
def write_results(outfile, tags, tag, size, gc, nn, fragments, exc, out=None):
    """Apply the jobs in order (:186-200): a later search always sets the size, and the GC content and sequence only
    when it found a site; print the progress counter every 1 000 searches; write the CSV (:203-212) unless something
    raised."""
    import numpy as np
    out = out or sys.stdout
    found = size >= 0
    zero = np.flatnonzero(found & (size - nn == 0))
    done = int(zero[0]) if len(zero) else len(tag)
    for c in range(1000, done + 1, 1000):
        print(c, file=out)
    if len(zero):
        j = int(zero[0])
        int(gc[j]) / int(size[j] - nn[j])               # raises ZeroDivisionError, as :193-195 does
    if exc is not None:
        raise exc
    nm = len(tags.names)
    last = np.full(nm, -1, dtype=np.int64)
    last[tag] = np.arange(len(tag))                     # numpy keeps the last of repeated indices
    last_found = np.full(nm, -1, dtype=np.int64)
    fj = np.flatnonzero(found)
    last_found[tag[fj]] = fj
    keep = np.flatnonzero(last_found >= 0)
    seqs = fragments(last_found[keep].tolist()) if len(keep) else []
    frag_seq = [""] * nm
    gc_val = ["NA"] * nm
    for t, j, s in zip(keep.tolist(), last_found[keep].tolist(), seqs):
        frag_seq[t] = s
        gc_val[t] = int(gc[j]) / int(size[j] - nn[j])
    with open(outfile, 'w', newline='') as fh:
        w = csv.writer(fh)
        w.writerow(["Marker name", "Sequence name", "Position", "Strand", "Fragment size",
                    "Fragment GC content", "Fragment sequence"])
        sizes = size.tolist()
        for i in range(nm):
            j = int(last[i])
            fs = sizes[j] if j >= 0 and sizes[j] >= 0 else "NA"
            w.writerow([tags.names[i], tags.seqnames[i], tags.positions[i],
                        "forward" if tags.forward[i] else "reverse", fs, gc_val[i], frag_seq[i]])


# ------------------------------------------------------------------ driver
def run(args, out=None):
    t0 = time.perf_counter()
    stages = []
    mark = [t0]

    def stage(name):
        now = time.perf_counter()
        stages.append((name, now - mark[0]))
        mark[0] = now

    if args.working_dir is not None:
        os.chdir(args.working_dir)
    paths, gfshort = genome_files(args)
    sites = cut_sites(args)
    tags = read_sam(args.samfile)
    stage("SAM (%d tags)" % len(tags.names))
    backend = args.td_backend
    if backend == "gpu" and (any(s == "" for s in sites) or len(sites) > 16 or any(len(s) > 64 for s in sites)):
        backend = "host"
    stage_ms = {}
    genome = None
    eng = None
    try:
        if backend == "gpu":
            from .engine import Engine
            eng = Engine(args.td_device)
            try:
                genome = DeviceGenome(eng, paths)
                stage_ms["K1"] = genome.k1_ms
            except _NeedHost:
                backend = "host"
        if backend == "host":
            genome = HostGenome(paths)
        stage("genome (%s)" % backend)
        tag, lo, hi, rev, exc = plan_jobs(tags, genome, gfshort)
        stage("plan (%d searches)" % len(tag))
        if backend == "gpu":
            size, gc, nn, fragments = search_device(genome, tags, sites, tag, lo, hi, rev, stage_ms)
        else:
            size, gc, nn, fragments = search_host(genome, tags, sites, tag, lo, hi, rev)
        stage("search")
        write_results(args.outfile, tags, tag, size, gc, nn, fragments, exc, out=out)
        stage("write")
    finally:
        if genome is not None:
            genome.close()
        if eng is not None:
            eng.close()
    if args.td_timing:
        for name, sec in stages:
            print("td-timing: %-28s %8.3f s" % (name, sec), file=sys.stderr)
        for k, v in stage_ms.items():
            print("td-timing: %-28s %8.3f ms device" % (k, v), file=sys.stderr)
        print("td-timing: %-28s %8.3f s" % ("total", time.perf_counter() - t0), file=sys.stderr)
    return stages, stage_ms


def main(argv=None):
    args = build_parser().parse_args(argv)
    run(args)


if __name__ == "__main__":
    main()
