"""Host-side driver of the MI355X tag counter: one Engine = one GPU handle.

Mirrors the set-up half of the reference's find_tags_fastq
(tagdigger_fun.py:197-233) in Python -- asserts, cut-site enumeration,
barcode+cutsite list, strip-or-shift decision -- and hands the two string
lists to libtagdig (td_set_index), which builds the flat device index.  The
record loop (:239-277) runs on the GPU.
"""
import collections
import contextlib
import ctypes as C
import os
import math

from . import _binding as B

# IUPAC codes in the order the reference expands them (tagdigger_fun.py:140-189)
_IUPAC = (("R", "AG"), ("Y", "CT"), ("K", "GT"), ("M", "AC"), ("S", "CG"), ("W", "AT"),
          ("B", "CGT"), ("D", "AGT"), ("H", "ACT"), ("V", "ACG"), ("N", "ACGT"))


def enumerate_cut_sites(cutsite):
    """All concrete cut sites of an IUPAC cut site, in the reference's order
    (tagdigger_fun.py:136-190): codes are expanded one kind at a time, leftmost
    occurrence first, the new lists concatenated per replacement base."""
    out = [cutsite]
    for code, bases in _IUPAC:
        while out[0].find(code) > -1:
            nxt = []
            for b in bases:
                nxt.extend(x.replace(code, b, 1) for x in out)
            out = nxt
    return out


def combine_barcode_and_cutsite(barcodes, cutsite):
    """(barcode + cutsite).upper() per barcode (tagdigger_fun.py:60-69)."""
    assert all([set(barcode.upper()) <= set('ACGT') for barcode in barcodes]), "Non-ACGT barcode."
    assert set(cutsite.upper()) <= set('ACGT'), "Invalid cut site."
    return [(barcode + cutsite).upper() for barcode in barcodes]


def census_index(barcodes, cutsite):
    """What a tag census hands to td_census_begin: the barcode + cut site list of find_tags_fastq
    (tagdigger_fun.py:198-219: its asserts, every cut-site variant), the number of barcodes, and where
    the window starts in a read -- behind the barcode, on the cut site's first base."""
    assert all([set(barcode.upper()) <= set('ACGT') for barcode in barcodes]), "Non-ACGT barcode."
    cutsite = cutsite.upper()
    assert set(cutsite) <= set('ACGTNRYKMSWBDHV'), "Invalid cut site."
    barcut = []
    for cut in enumerate_cut_sites(cutsite):
        barcut += combine_barcode_and_cutsite(barcodes, cut)
    return barcut, len(barcodes), [len(x) for x in barcodes]


def rescue_index(barcodes, tags, cutsite):
    """What a tag rescue hands to td_rescue_begin: Engine.set_index's set-up (find_tags_fastq, tagdigger_fun.py:197-233)
    with its asserts and its strip decision -- the barcode + cut site list over every cut-site variant, the number of
    barcodes, where the tag comparison starts in a read of each barcode, and the tags as they are compared."""
    assert all([set(barcode.upper()) <= set('ACGT') for barcode in barcodes]), "Non-ACGT barcode."
    cutsite = cutsite.upper()
    assert set(cutsite) <= set('ACGTNRYKMSWBDHV'), "Invalid cut site."
    tags = [tag.upper() for tag in tags]
    assert all([set(tag) <= set('ACGT') for tag in tags]), "Non-ACGT tag."
    cutlen = len(cutsite)
    tagoff = [len(x) + cutlen for x in barcodes]
    cutsites = enumerate_cut_sites(cutsite)
    barcut = []
    for cut in cutsites:
        barcut += combine_barcode_and_cutsite(barcodes, cut)
    if set(x[:cutlen] for x in tags).issubset(set(cutsites)):
        if len(cutsites) == 1:
            tags = [x[cutlen:] for x in tags]          # site already checked with the barcode
        else:
            tagoff = [x - cutlen for x in tagoff]      # tags keep the (variable) site
    return barcut, len(barcodes), tagoff, tags


INDEX_INFO = ("W", "m_bases", "buckets", "spb", "nshort", "displaced", "longest", "wrapped", "nch", "nch2")     # TD_INDEX_* slots

CENSUS_STATS = ("reads", "barcut", "short", "ambiguous", "counted", "distinct", "slots", "max_keys")
RESCUE_STATS = ("reads", "barcut", "exact", "rescued1", "rescued2", "ambiguous", "none", "longest_run")     # TD_RESCUE_* slots
RESCUE_MAX_TAGLEN = 128     # TD_RESCUE_MAX_TAGLEN
BCRESCUE_STATS = ("reads", "exact", "rescued1", "rescued2", "ambiguous", "none", "tagged", "min_entry_distance")     # TD_BCRESCUE_* slots
BCRESCUE_POSITIONS = 32     # TD_BCRESCUE_POSITIONS
QC_STATS = ("reads", "barcut", "qual_lines", "bases", "qual_bases", "qual_invalid", "empty_qual", "max_cycles")     # TD_QC_* slots


def effective_maxreads(maxreads):
    """The reference tests `readscount >= maxreads` after each read
    (tagdigger_fun.py:272-273): one read is always processed and a fractional
    bound rounds up."""
    if maxreads >= 2 ** 62:
        return 2 ** 62
    return max(1, int(math.ceil(maxreads)))


def frag_job_dtype():
    """numpy layout of td_frag_job (include/tagdig.h)."""
    import numpy as np
    return np.dtype([("lo", "<u8"), ("hi", "<u8"), ("tagsize", "<i4"), ("reverse", "<i4"), ("reserved", "<u8")])


def _c_strings(strings):
    arr = (C.c_char_p * max(1, len(strings)))()
    for i, s in enumerate(strings):
        arr[i] = s.encode("ascii")
    return arr


class TagSet:
    """A sorted tag set resident on the device (td_tagset_load); freed by close() or when collected."""

    def __init__(self, eng, ptr, n):
        self._eng, self.ptr, self.n = eng, ptr, n

    def close(self):
        if self.ptr and self.ptr.value and getattr(self._eng, "_h", None):
            self._eng._L.td_tagset_free(self._eng._h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TagNet:
    """A tag network built on the device (td_tagnet_build); freed by close() or when collected."""

    def __init__(self, eng, ptr, n, stats, ms):
        self._eng, self.ptr, self.n, self.stats, self.ms = eng, ptr, n, stats, ms

    def close(self):
        if self.ptr and self.ptr.value and getattr(self._eng, "_h", None):
            self._eng._L.td_tagnet_free(self._eng._h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Place:
    """A genome's cut sites resident on the device (td_place_sites); freed by close(), when collected, or with the
    engine.  `.stats`: loci, forward, reverse, distinct, dropped_bounds, dropped_alphabet, records; `.ms`: device time."""

    def __init__(self, eng, ptr, taglen, stats, ms):
        self._eng, self.ptr, self.taglen, self.stats, self.ms = eng, ptr, taglen, stats, ms
        self.n = stats["loci"]

    def close(self):
        if self.ptr and self.ptr.value and getattr(self._eng, "_h", None):
            self._eng._L.td_place_free(self._eng._h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PLACE_STATS = ("loci", "forward", "reverse", "distinct", "dropped_bounds", "dropped_alphabet", "records")   # TD_PLACE_* slots
PLACE_MS = ("count", "scan", "emit", "dedupe")
PLACED_STATS = ("tags", "unique", "multi", "none", "compares")      # TD_PLACED_* slots
PLACED_MS = ("pack", "parts", "runs", "join")


TAGNET_STATS = ("tags", "edges", "kept", "deg0", "deg1", "hubs", "pairs", "compares")
TAGNET_MS = ("pack", "sort", "runs", "compare", "select", "host_order")
TAGNET_TILE = 256           # TD_TAGNET_TILE: rows and columns of a compare tile of csrc/tagnet.hip


GENO_STATS = ("called", "n0", "n1", "n2", "alt", "depth0", "depth1")     # TD_GENO_* slots of a marker's statistics row
GENO_RULES = {"likelihood": 0, "presence": 1}
GENO_TABLE = 128            # TD_GENO_TABLE: entries of het_min
GENO_CHUNK = 64             # TD_GENO_CHUNK: sample rows per workgroup of csrc/genocall.hip's call kernel


class GenoCalls(collections.namedtuple("GenoCalls", "calls stats mask ms passed d_calls")):
    """What Engine.geno_call returns: calls (uint8 [S, M]; None when they were not fetched), stats (dict of uint64 [M]
    arrays by GENO_STATS), mask (bool [M]), ms (device time), passed (how many pass), d_calls (the device buffer of the
    calls when it was asked for -- the caller's, to be freed with dev_free -- else None)."""
    __slots__ = ()


DOSE_STATS = ("called",) + tuple("n%d" % d for d in range(9)) + ("alt", "depth0", "depth1", "bin")     # TD_DOSE_* slots
DOSE_PRIORS = {"flat": 0, "hwe": 1}
DOSE_MAX_PLOIDY = 8         # TD_DOSE_MAX_PLOIDY
DOSE_BINS = 64              # TD_DOSE_BINS: rows of the prior table
DOSE_COST_MAX = 1 << 23     # TD_DOSE_COST_MAX: the largest table entry the library takes
DOSE_MISSING = 255          # TD_DOSE_MISSING
DOSE_CHUNK = 64             # TD_DOSE_CHUNK: sample rows per workgroup of csrc/dosage.hip's kernels


class DoseCalls(collections.namedtuple("DoseCalls", "calls diploid stats mask ms passed d_calls d_diploid")):
    """What Engine.dose_call returns: calls (uint8 [S, M], dosage 0 .. P or 255; None when not fetched), diploid (the
    diploidised matrix, 0 / 1 / 2 / 3; None when not asked for or not fetched), stats (dict of uint64 [M] arrays by
    DOSE_STATS), mask (bool [M]), ms (device time), passed, d_calls and d_diploid (the device buffers when they were asked
    for -- the caller's, to be freed with dev_free -- else None)."""
    __slots__ = ()


VCF_CHUNK = 64              # TD_VCF_CHUNK: samples per workgroup of csrc/vcf.hip's measure and emit kernels
VCF_TILE = 64               # TD_VCF_TILE: lines per workgroup of its emit kernel
VCF_MTILE = 256             # TD_VCF_MTILE: lines per workgroup of its measure kernel
VCF_CELL_MAX = 64           # TD_VCF_CELL_MAX: bytes of a cell with its tab, at most
VCF_RANGE_BYTES = 256 << 20  # TD_VCF_RANGE_BYTES: the default budget of a range (a choice that has not been measured)
VCF_MS = ("measure", "scan", "emit")


class VcfText(collections.namedtuple("VcfText", "text nbytes line_off ms ranges")):
    """What Engine.vcf_format and Engine.vcf_file return: text (the body lines as bytes; None for a measuring call and
    for a file), nbytes (their total), line_off (uint64 [K + 1], the byte offset of every line; None for a file), ms (dict
    of device ms: measure, scan, emit; for a file also write, the wall ms spent in write()), ranges (a file: the ranges it
    was emitted in; else None)."""
    __slots__ = ()


RELATE_MAX_SAMPLES = 16384  # TD_RELATE_MAX_SAMPLES: the joint table is 9 S^2 uint32
RELATE_TILE = 64            # TD_RELATE_TILE: samples along a workgroup's tile edge of csrc/relate.hip
RELATE_KCHUNK = 32768       # TD_RELATE_KCHUNK: markers per workgroup of csrc/relate.hip


class RelateJoint(collections.namedtuple("RelateJoint", "joint ms d_joint")):
    """What Engine.relate_joint returns: joint (uint32 [S, S, 3, 3]; None when it was not fetched), ms (device time),
    d_joint (the device buffer of the table when it was asked for -- the caller's, to be freed with dev_free -- else
    None)."""
    __slots__ = ()


PARENT_MAX_SAMPLES = 16384  # TD_PARENT_MAX_SAMPLES
PARENT_MAX_CAND = 128       # TD_PARENT_MAX_CAND: candidate slots of an offspring row
PARENT_MAX_TOP = 8          # TD_PARENT_MAX_TOP: ranked trios returned per offspring row
PARENT_BLOCK = 64           # TD_PARENT_BLOCK: candidate slots along a workgroup's block edge of csrc/parent.hip
PARENT_WCHUNK = 16          # TD_PARENT_WCHUNK: 64-marker words staged in LDS at a time by csrc/parent.hip
PARENT_SELFING = 1          # TD_PARENT_SELFING: flags bit 0
PARENT_TRIO = [("p", "<u4"), ("q", "<u4"), ("n", "<u4"), ("e", "<u4")]    # td_parent_trio
PARENT_NONE = 0xFFFFFFFF    # p and q of a record where fewer than `top` trios rank


class ParentTrios(collections.namedtuple("ParentTrios", "best table ms times")):
    """What Engine.parent_trios returns: best (structured array [O, top] with the fields of td_parent_trio; p = q =
    PARENT_NONE where fewer trios rank), table (uint32 [O, T, 2] of (n, e) per trio; None when it was not fetched), ms
    (device time of the three kernels), times (dict: pack_ms, trio_ms, rank_ms)."""
    __slots__ = ()


LD_MAX_SAMPLES = 16384      # TD_LD_MAX_SAMPLES: cov and var of a pair of markers fit 32 bits
LD_MAX_MARKERS = 1 << 20    # TD_LD_MAX_MARKERS: participating markers of one call
LD_TILE = 64                # TD_LD_TILE: markers along a workgroup's tile edge of csrc/ld.hip
LD_EDGE = [("i", "<u4"), ("j", "<u4"), ("shared", "<u4"), ("cov", "<i4"), ("var_i", "<u4"), ("var_j", "<u4")]    # td_ld_edge


class LDPairs(collections.namedtuple("LDPairs", "edges n degree called ms times")):
    """What Engine.ld_pairs returns: edges (structured array with the fields of td_ld_edge, ascending by (i, j)), n (how
    many there are), degree and called (uint32 [M]), ms (device time of the two kernels), times (dict: transpose_ms and
    pairs_ms on the device, sort_ms on the host, of the call that returned the edges)."""
    __slots__ = ()


LINK_MAX_SAMPLES = 16384    # TD_LINK_MAX_SAMPLES: offspring rows of one call
LINK_MAX_MARKERS = 1 << 20  # TD_LINK_MAX_MARKERS: participating markers of one call
LINK_TILE = 64              # TD_LINK_TILE: markers along a workgroup's tile edge of csrc/link.hip
LINK_EDGE = [("i", "<u4"), ("j", "<u4"), ("n", "<u4"), ("rec_phase", "<u4"), ("lod16", "<i8")]    # td_link_edge
LINK_NO_PART = 255          # the cls byte of a marker that takes no part
LINK_LOD_MIN = -(1 << 63)   # min_lod16 with the LOD test off


class LinkPairs(collections.namedtuple("LinkPairs", "edges n degree informative ms times")):
    """What Engine.link_pairs returns: edges (structured array with the fields of td_link_edge, ascending by (i, j)), n
    (how many there are), degree and informative (uint32 [M]), ms (device time of the two kernels), times (dict:
    gather_ms and pairs_ms on the device, sort_ms on the host, of the call that returned the edges)."""
    __slots__ = ()


IMPUTE_MAX_SAMPLES = 4096   # TD_IMPUTE_MAX_SAMPLES: the samples' planes lie in one workgroup's LDS
IMPUTE_MAX_NBR = 64         # TD_IMPUTE_MAX_NBR: a plane is one 64-bit word per sample
IMPUTE_MAX_K = 32           # TD_IMPUTE_MAX_K: voters of a cell
IMPUTE_STATS = ("missing", "imputed", "no_donor", "undecided")     # the columns of a marker's statistics row


class ImputeKnn(collections.namedtuple("ImputeKnn", "calls stats ms times d_calls")):
    """What Engine.impute_knn returns: calls (uint8 [S, M], the filled matrix; None when it was not fetched), stats
    (uint32 [M, 4] by IMPUTE_STATS), ms (device time of the two kernels), times (dict: transpose_ms, vote_ms), d_calls (the
    device buffer of the filled matrix when it was asked for -- the caller's, to be freed with dev_free -- else None)."""
    __slots__ = ()


def counts_as_uint32(counts):
    """A count matrix as a C-contiguous uint32 array.  uint32 is what the device reads; another integer type is taken
    when every value fits, and refused otherwise."""
    import numpy as np
    a = np.asarray(counts)
    if a.ndim != 2:
        raise ValueError("the count matrix must have two dimensions (samples x tags)")
    if a.dtype != np.uint32:
        if a.dtype.kind not in "iu":
            raise TypeError("the count matrix must hold integers (uint32), not {}".format(a.dtype))
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xffffffff):
            raise OverflowError("the count matrix holds values outside 0 .. 2^32 - 1 (min {}, max {}): genotype calling "
                                "reads uint32 counts".format(int(a.min()), int(a.max())))
        a = a.astype(np.uint32)
    return np.ascontiguousarray(a)


class Engine:
    """Owns a td_handle on one GPU."""

    def __init__(self, device=0):
        self._L = B.load()
        h = C.c_void_p()
        B.check(self._L.td_create(C.byref(h), int(device)))
        self._h = h
        self.device = device
        self.barnum = 0
        self.ntags = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.td_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ index
    def set_index(self, barcodes, tags, cutsite="TGCAG"):
        """Set-up of find_tags_fastq, tagdigger_fun.py:197-233.  The index on the device is kept when the
        same barcodes, tags and cut site come again (the libraries of one run usually share a barcode set):
        only the counts are zeroed then, as a fresh index would have them."""
        key = (tuple(barcodes), tuple(tags), cutsite)
        if key == getattr(self, "_index_key", None):
            self.reset()
            return
        self._index_key = None
        assert all([set(barcode.upper()) <= set('ACGT') for barcode in barcodes]), "Non-ACGT barcode."
        cutsite = cutsite.upper()
        assert set(cutsite) <= set('ACGTNRYKMSWBDHV'), "Invalid cut site."
        tags = [tag.upper() for tag in tags]
        assert all([set(tag) <= set('ACGT') for tag in tags]), "Non-ACGT tag."
        cutlen = len(cutsite)
        barcutlen = [len(x) + cutlen for x in barcodes]
        barnum = len(barcodes)
        cutsites = enumerate_cut_sites(cutsite)
        barcut = []
        for cut in cutsites:
            barcut += combine_barcode_and_cutsite(barcodes, cut)
        if set(x[:cutlen] for x in tags).issubset(set(cutsites)):
            if len(cutsites) == 1:
                tags = [x[cutlen:] for x in tags]          # site already checked with the barcode
            else:
                barcutlen = [x - cutlen for x in barcutlen]  # tags keep the (variable) site
        self._set_index_lists(barcut, barnum, barcutlen, tags)
        self._index_key = key

    def _set_index_lists(self, barcut, barnum, tagoff, tags):
        """td_set_index as include/tagdig.h states it: the barcode + cut site strings (entry k belongs to barcode
        k % barnum), where the tag search starts in a read of each barcode (up to 63 bases in: it may lie behind the
        barcode entry), and the tags as the table stores them.  set_index derives these from find_tags_fastq's
        arguments; called directly only by tests that need an offset find_tags_fastq never asks for."""
        self._index_key = None
        off = (C.c_uint32 * max(1, barnum))(*tagoff)
        B.check(self._L.td_set_index(self._h, _c_strings(barcut), len(barcut), barnum, off,
                                     _c_strings(tags), len(tags)))
        self.barnum, self.ntags = barnum, len(tags)

    def index_info(self):
        """td_index_info: the shape of the tag hash table the last set_index built, by INDEX_INFO's names (W, m_bases,
        buckets, spb, nshort, displaced, longest, wrapped, nch, nch2).  Host-side bookkeeping of the build: for tests
        and diagnostics, never part of a count."""
        out = (C.c_uint64 * len(INDEX_INFO))()
        B.check(self._L.td_index_info(self._h, out))
        return dict(zip(INDEX_INFO, (int(x) for x in out)))

    # ------------------------------------------------------------------ counting
    def reset(self):
        B.check(self._L.td_reset(self._h))

    def set_option(self, name, value):
        B.check(self._L.td_set_option(self._h, name.encode(), int(value)))

    def bind_counts(self, device_ptr):
        B.check(self._L.td_bind_counts(self._h, C.c_void_p(device_ptr) if device_ptr else None))

    def count_device(self, d_ptr, nbytes, first_line=0, maxreads=5e9, tassel_tagcount=False, stream=0):
        """Enqueue one pass over a FASTQ buffer already in HBM (asynchronous)."""
        B.check(self._L.td_count_device(self._h, C.c_void_p(d_ptr), nbytes, first_line,
                                        effective_maxreads(maxreads), 1 if tassel_tagcount else 0,
                                        C.c_void_p(stream) if stream else None))

    def count_bytes(self, data, first_line=0, maxreads=5e9, tassel_tagcount=False):
        """Count a host buffer of whole lines; returns the number of line terminators consumed."""
        n = len(data)
        lines = C.c_uint64(0)
        if n:
            # no copy: bytes objects and ctypes arrays are passed by address, numpy arrays by .ctypes.data
            if isinstance(data, (bytes, C.Array)):
                ptr = data
            elif hasattr(data, "ctypes"):
                ptr = C.c_void_p(data.ctypes.data)
            else:
                ptr = (C.c_char * n).from_buffer_copy(data)
            B.check(self._L.td_count_host(self._h, ptr, n, first_line, effective_maxreads(maxreads),
                                          1 if tassel_tagcount else 0, C.byref(lines)))
        return lines.value

    def count_file(self, path, maxreads=5e9, tassel_tagcount=False):
        """Record loop of find_tags_fastq (tagdigger_fun.py:239-277) over a file."""
        # same failure modes as the reference's open() / gzip.open(): the OSError of a file that cannot be opened here;
        # what a .gz that is damaged, padded or no gzip at all ends in comes from the library (td_count_file, csrc/gz_pyrules.hpp:
        # EOFError / gzip.BadGzipFile / zlib.error with gzip.open's messages, raised by _binding.check)
        open(path, 'rb').close()
        B.check(self._L.td_count_file(self._h, path.encode(), effective_maxreads(maxreads),
                                      1 if tassel_tagcount else 0))

    def gunzip_file_gpu(self, path, capacity):
        """An ordinary .gz file inflated by the device decoder (csrc/gz_gpu.hpp): its text as bytes, or None where that
        decoder leaves the file to the host decoders (see td_gunzip_file_gpu in include/tagdig.h)."""
        buf = (C.c_uint8 * max(1, capacity))()
        n, on_gpu = C.c_uint64(0), C.c_int(0)
        B.check(self._L.td_gunzip_file_gpu(self._h, path.encode(), buf, capacity, C.byref(n), C.byref(on_gpu)))
        return bytes(memoryview(buf)[:n.value]) if on_gpu.value else None

    # one ordinary gzip file over several ranks (multi.count_file_sharded): include/tagdig.h td_gz_shard_*
    def gz_shard_open(self, path, byte_lo, byte_hi, first):
        """-> (first block start in the range as a bit position of the file, or None; the file's size)"""
        start, size = C.c_uint64(0), C.c_uint64(0)
        B.check(self._L.td_gz_shard_open(self._h, path.encode(), int(byte_lo), int(byte_hi), 1 if first else 0, C.byref(start), C.byref(size)))
        return (None if start.value == 2 ** 64 - 1 else start.value), size.value

    def gz_shard_decode(self, stop_bit):
        """-> (end bit, bytes of text, ended the member, map: numpy uint16[32768])"""
        import numpy as np
        end, n, fin = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        m = np.zeros(32768, dtype=np.uint16)
        B.check(self._L.td_gz_shard_decode(self._h, 2 ** 64 - 1 if stop_bit is None else int(stop_bit), C.byref(end), C.byref(n), C.byref(fin),
                                           m.ctypes.data_as(C.c_void_p)))
        return end.value, n.value, bool(fin.value), m

    def gz_shard_resolve(self, window_in, member_out_before):
        """-> (device pointer of the stretch's text, its CRC-32)"""
        import numpy as np
        w = np.ascontiguousarray(window_in, dtype=np.uint8)
        assert w.size == 32768
        ptr, crc = C.c_void_p(0), C.c_uint32(0)
        B.check(self._L.td_gz_shard_resolve(self._h, w.ctypes.data_as(C.c_void_p), int(member_out_before), C.byref(ptr), C.byref(crc)))
        return int(ptr.value or 0), crc.value

    def crc32_join(self, crc_a, crc_b, len_b):
        return int(self._L.td_crc32_join(int(crc_a), int(crc_b), int(len_b)))

    def last_gz_route(self):
        """1: the .gz file counted last was inflated on the device; 0: by a host decoder."""
        return int(self._L.td_last_gz_route(self._h))

    # ------------------------------------------------------------------ barcode splitter
    def set_splitter(self, barcodes, cutsite, fullsite0, fullsite1, entries):
        """entries[b] = [(adapter beginning to look for at the end of a read, slice index), ...] for
        barcode b (what build_adapter_tree, tagdigger_fun.py:1208-1249, resolves to)."""
        begin = [0]
        seqs, slices = [], []
        for per_barcode in entries:
            for seq, sl in per_barcode:
                seqs.append(seq)
                slices.append(sl)
            begin.append(len(seqs))
        B.check(self._L.td_set_splitter(self._h, _c_strings(barcodes), len(barcodes), cutsite.encode("ascii"),
                                        fullsite0.encode("ascii"), fullsite1.encode("ascii"),
                                        (C.c_uint32 * len(begin))(*begin), _c_strings(seqs),
                                        (C.c_int32 * max(1, len(slices)))(*slices), len(seqs)))

    def split_kernel_in_use(self):
        """td_split_kernel_in_use: 2 (k_split2) or 1 (k_split), the kernel that decides for the splitter set last and
        the option split_kernel as it stands."""
        k = C.c_int(0)
        B.check(self._L.td_split_kernel_in_use(self._h, C.byref(k)))
        return k.value

    def split_prefix_source(self):
        """td_debug_counters [20]: where the last line prefix took its per-tile terminator counts from -- 1 counted from the
        bytes, 2 the tile records of the count pass that count_and_split_device had just enqueued; 0 before any."""
        return self.debug_counters()[20]

    def split_device(self, d_ptr, nbytes, first_line=0, stream=0):
        """[(barcode index or -1, findAdapterSeq value), ...] for the sequence lines of a device buffer."""
        import numpy as np
        cap = (self.count_lines_device(d_ptr, nbytes, stream) + 1) // 4 + 2
        d_out = self.dev_alloc(cap * 8)
        try:
            terms = C.c_uint64(0)
            B.check(self._L.td_split_device(self._h, C.c_void_p(d_ptr), nbytes, first_line, C.c_void_p(d_out), cap,
                                            C.c_void_p(stream) if stream else None, C.byref(terms)))
            raw = self.d2h(d_out, cap * 8)
        finally:
            self.dev_free(d_out)
        # lines of the buffer: one per terminator, plus an unterminated last line (the caller knows)
        return np.frombuffer(raw, dtype=np.int32).reshape(-1, 2), terms.value

    def count_and_split_device(self, d_ptr, nbytes, first_line=0, maxreads=5e9, stream=0):
        """Counting and the splitter's per-read decisions over ONE buffer in HBM (BASELINE config 5); the counts land
        in the engine's matrix, the decisions come back as split_device's."""
        import numpy as np
        cap = (self.count_lines_device(d_ptr, nbytes, stream) + 1) // 4 + 2
        d_out = self.dev_alloc(cap * 8)
        try:
            terms = C.c_uint64(0)
            B.check(self._L.td_count_and_split_device(self._h, C.c_void_p(d_ptr), nbytes, first_line, effective_maxreads(maxreads),
                                                      C.c_void_p(d_out), cap, C.c_void_p(stream) if stream else None, C.byref(terms)))
            raw = self.d2h(d_out, cap * 8)
        finally:
            self.dev_free(d_out)
        return np.frombuffer(raw, dtype=np.int32).reshape(-1, 2), terms.value

    def split_file(self, in_path, out_paths, maxreads=500000000):
        """The record loop of barcodeSplitter (tagdigger_fun.py:1318-1368); returns (reads, with
        barcode and cut site, clipped on the 3' end)."""
        st = (C.c_uint64 * 3)()
        B.check(self._L.td_split_file(self._h, in_path.encode(), _c_strings(out_paths),
                                      effective_maxreads(maxreads), st))
        return st[0], st[1], st[2]

    def split_progress_lines(self, in_path, reads):
        """The lines barcodeSplitter's loop prints while it reads (tagdigger_fun.py:1357-1360), for the last split_file."""
        n = C.c_uint64(0)
        B.check(self._L.td_split_progress(self._h, None, 0, C.byref(n)))
        out = (C.c_uint64 * max(1, 2 * n.value))()
        B.check(self._L.td_split_progress(self._h, out, n.value, C.byref(n)))
        lines, bar, clip = [], 0, 0
        for k in range(n.value):
            done = 50000 * (k + 1)
            if done > reads:
                break
            bar, clip = bar + out[2 * k], clip + out[2 * k + 1]
            if done % 1000000 == 0:
                lines.append(in_path)
            lines.append("Reads: {0} With barcode and cut site: {1} Clipped on 3' end: {2}".format(done, bar, clip))
        return lines

    def count_lines_device(self, d_ptr, nbytes, stream=0):
        out = C.c_uint64(0)
        B.check(self._L.td_count_lines_device(self._h, C.c_void_p(d_ptr), nbytes,
                                              C.c_void_p(stream) if stream else None, C.byref(out)))
        return out.value

    def load_file_range(self, path, offset, length, d_dst):
        """bytes [offset, offset + length) of a file -> device memory at d_dst, through the library's pinned staging pieces"""
        B.check(self._L.td_load_file_range(self._h, os.fsencode(path), int(offset), int(length), C.c_void_p(d_dst)))

    def bgzf_inflate_range(self, path, off_begin, off_end, d_dst, capacity):
        """the BGZF members starting in [off_begin, off_end) of a file, inflated on the GPU into d_dst; returns the bytes written"""
        n = C.c_uint64(0)
        B.check(self._L.td_bgzf_inflate_range(self._h, os.fsencode(path), int(off_begin), int(off_end), C.c_void_p(d_dst), int(capacity), C.byref(n)))
        return n.value

    def fold_rows(self, rows, d_dst, n_dst_rows, stream=0):
        """K3: add this library's barcode rows into sample rows on the device (d_dst: n_dst_rows x ntags uint32 in
        device memory; rows[b] = the sample row of barcode b) -- combineReadCounts (tagdigger_fun.py:1061-1098)
        without host lists."""
        arr = (C.c_uint32 * max(1, self.barnum))(*rows)
        B.check(self._L.td_fold_rows(self._h, arr, n_dst_rows, C.c_void_p(d_dst), C.c_void_p(stream) if stream else None))

    # ------------------------------------------------------------------ tag census (td_census_*)
    def census_begin(self, barcodes, cutsite="TGCAG", taglen=64, slots=0):
        """A fresh census of the windows of `taglen` bases behind these barcodes (a power of two of slots; 0: 2^22)."""
        barcut, barnum, baroff = census_index(barcodes, cutsite)
        B.check(self._L.td_census_begin(self._h, _c_strings(barcut), len(barcut), barnum,
                                        (C.c_uint32 * max(1, barnum))(*baroff), int(taglen), int(slots)))
        self._census_taglen = int(taglen)

    def census_device(self, d_ptr, nbytes, first_line=0, maxreads=5e9, stream=0):
        """Enqueue one census pass over a FASTQ buffer already in HBM (asynchronous, accumulates)."""
        B.check(self._L.td_census_device(self._h, C.c_void_p(d_ptr), nbytes, first_line, effective_maxreads(maxreads),
                                         C.c_void_p(stream) if stream else None))

    def census_file(self, path, maxreads=5e9):
        """The census over a file, plain or gzip by name, through count_file's readers (accumulates)."""
        open(path, 'rb').close()
        B.check(self._L.td_census_file(self._h, os.fsencode(path), effective_maxreads(maxreads)))

    def census_stats(self):
        """{reads, barcut, short, ambiguous, counted, distinct, slots, max_keys}, cumulative since census_begin."""
        st = (C.c_uint64 * 8)()
        B.check(self._L.td_census_stats(self._h, st))
        return dict(zip(CENSUS_STATS, (int(x) for x in st)))

    def census_fetch(self, min_count=1, top=None):
        """(windows, counts) with count >= min_count, by count descending, then sequence; `top`: the first N of them."""
        L = getattr(self, "_census_taglen", 0)
        n = C.c_uint64(0)
        if top is None or not L:              # (how many there are; without a census: the library's TD_E_STATE)
            B.check(self._L.td_census_fetch(self._h, int(min_count), None, None, 0, C.byref(n)))
            want = n.value
        else:
            want = max(0, int(top))
        if want == 0:
            return [], []
        seqs = C.create_string_buffer(want * L)
        counts = (C.c_uint64 * want)()
        B.check(self._L.td_census_fetch(self._h, int(min_count), seqs, counts, want, C.byref(n)))
        want = min(want, n.value)
        text = seqs.raw.decode("ascii")
        return [text[k * L:(k + 1) * L] for k in range(want)], [int(x) for x in counts[:want]]

    def census_end(self):
        B.check(self._L.td_census_end(self._h))
        self._census_taglen = 0

    # ------------------------------------------------------------------ library QC (td_qc_*; csrc/qc.hip)
    def qc_begin(self, barcodes, cutsite="TGCAG", max_cycles=160):
        """Fresh QC tables for these barcodes: per-cycle rows 0 .. max_cycles - 1 and one overflow row."""
        barcut, barnum, baroff = census_index(barcodes, cutsite)
        B.check(self._L.td_qc_begin(self._h, _c_strings(barcut), len(barcut), barnum,
                                    (C.c_uint32 * max(1, barnum))(*baroff), int(max_cycles)))
        self._qc_shape = (barnum, int(max_cycles))

    def qc_device(self, d_ptr, nbytes, first_line=0, maxreads=5e9, stream=0):
        """Enqueue one QC pass over a FASTQ buffer already in HBM (asynchronous, accumulates)."""
        B.check(self._L.td_qc_device(self._h, C.c_void_p(d_ptr), nbytes, first_line, effective_maxreads(maxreads),
                                     C.c_void_p(stream) if stream else None))

    def qc_file(self, path, maxreads=5e9):
        """The QC over a file, plain or gzip by name, through count_file's readers (accumulates)."""
        open(path, 'rb').close()
        B.check(self._L.td_qc_file(self._h, os.fsencode(path), effective_maxreads(maxreads)))

    def qc_stats(self):
        """{reads, barcut, qual_lines, bases, qual_bases, qual_invalid, empty_qual, max_cycles}, cumulative since qc_begin."""
        st = (C.c_uint64 * 8)()
        B.check(self._L.td_qc_stats(self._h, st))
        return dict(zip(QC_STATS, (int(x) for x in st)))

    def qc_fetch(self):
        """(barcodes (B+1, 3), base_cycle (C+1, 6), qual_cycle (C+1, 95), lengths (C+1), meanq (94)) as numpy uint64."""
        import numpy as np
        barnum, cyc = getattr(self, "_qc_shape", (0, 0))
        out = [np.zeros(shape, dtype=np.uint64) for shape in ((barnum + 1, 3), (cyc + 1, 6), (cyc + 1, 95), (cyc + 1,), (94,))]
        B.check(self._L.td_qc_fetch(self._h, *[C.c_void_p(a.ctypes.data) for a in out]))
        return tuple(out)

    def qc_end(self):
        B.check(self._L.td_qc_end(self._h))
        self._qc_shape = (0, 0)

    # ------------------------------------------------------------------ tag rescue (td_rescue_*; csrc/rescue.hip)
    def rescue_begin(self, barcodes, tags, cutsite="TGCAG", max_mismatch=1):
        """A fresh rescue matrix for these barcodes and tags (set_index's set-up), at 1 or 2 mismatches."""
        barcut, barnum, tagoff, stored = rescue_index(barcodes, tags, cutsite)
        self._rescue_begin_lists(barcut, barnum, tagoff, stored, max_mismatch)

    def _rescue_begin_lists(self, barcut, barnum, tagoff, tags, max_mismatch=1):
        """td_rescue_begin as include/tagdig.h states it; called directly only by tests that need an offset or a tag list
        rescue_begin never derives."""
        self._rescue_shape = (0, 0)
        B.check(self._L.td_rescue_begin(self._h, _c_strings(barcut), len(barcut), barnum, (C.c_uint32 * max(1, barnum))(*tagoff),
                                        _c_strings(tags), len(tags), int(max_mismatch)))
        self._rescue_shape = (barnum, len(tags))

    def rescue_device(self, d_ptr, nbytes, first_line=0, maxreads=5e9, stream=0):
        """Enqueue one rescue pass over a FASTQ buffer already in HBM (asynchronous, accumulates)."""
        B.check(self._L.td_rescue_device(self._h, C.c_void_p(d_ptr), nbytes, first_line, effective_maxreads(maxreads),
                                         C.c_void_p(stream) if stream else None))

    def rescue_file(self, path, maxreads=5e9):
        """The rescue over a file, plain or gzip by name, through count_file's readers (accumulates)."""
        open(path, 'rb').close()
        B.check(self._L.td_rescue_file(self._h, os.fsencode(path), effective_maxreads(maxreads)))

    def rescue_stats(self):
        """{reads, barcut, exact, rescued1, rescued2, ambiguous, none, longest_run}, cumulative since rescue_begin."""
        st = (C.c_uint64 * 8)()
        B.check(self._L.td_rescue_stats(self._h, st))
        return dict(zip(RESCUE_STATS, (int(x) for x in st)))

    def rescue_work(self):
        """{probes, verified, part_bases, max_probe}: directory probes and verified tags of the passes so far, and the
        shape of the index."""
        st = (C.c_uint64 * 4)()
        B.check(self._L.td_rescue_work(self._h, st))
        return dict(zip(("probes", "verified", "part_bases", "max_probe"), (int(x) for x in st)))

    def rescue_fetch(self):
        """(rescued uint32 [barnum, ntags], positions uint64 [128]) as numpy arrays."""
        import numpy as np
        barnum, ntags = getattr(self, "_rescue_shape", (0, 0))
        rescued = np.zeros((barnum, ntags), dtype=np.uint32)
        positions = np.zeros(RESCUE_MAX_TAGLEN, dtype=np.uint64)
        B.check(self._L.td_rescue_fetch(self._h, C.c_void_p(rescued.ctypes.data) if rescued.size else None,
                                        C.c_void_p(positions.ctypes.data)))
        return rescued, positions

    def rescue_matrix(self):
        """The device address of the rescue matrix (uint32 [barnum, ntags]); good until rescue_end or the next begin."""
        p = C.c_void_p()
        B.check(self._L.td_rescue_matrix(self._h, C.byref(p)))
        return p.value

    def rescue_end(self):
        B.check(self._L.td_rescue_end(self._h))
        self._rescue_shape = (0, 0)

    # ------------------------------------------------------------------ barcode rescue (td_bcrescue_*; csrc/bcrescue.hip)
    def bcrescue_begin(self, barcodes, tags, cutsite="TGCAG", max_mismatch=1):
        """Fresh barcode-rescue results for these barcodes and tags (set_index's set-up), at 1 or 2 mismatches."""
        barcut, barnum, tagoff, stored = rescue_index(barcodes, tags, cutsite)
        self._bcrescue_begin_lists(barcut, barnum, tagoff, stored, max_mismatch)

    def _bcrescue_begin_lists(self, barcut, barnum, tagoff, tags, max_mismatch=1):
        """td_bcrescue_begin as include/tagdig.h states it; called directly only by tests that need an entry list, an
        offset or a tag list bcrescue_begin never derives."""
        self._bcrescue_shape = (0, 0)
        B.check(self._L.td_bcrescue_begin(self._h, _c_strings(barcut), len(barcut), barnum, (C.c_uint32 * max(1, barnum))(*tagoff),
                                          _c_strings(tags), len(tags), int(max_mismatch)))
        self._bcrescue_shape = (barnum, len(tags))

    def bcrescue_device(self, d_ptr, nbytes, first_line=0, maxreads=5e9, stream=0):
        """Enqueue one barcode-rescue pass over a FASTQ buffer already in HBM (asynchronous, accumulates)."""
        B.check(self._L.td_bcrescue_device(self._h, C.c_void_p(d_ptr), nbytes, first_line, effective_maxreads(maxreads),
                                           C.c_void_p(stream) if stream else None))

    def bcrescue_file(self, path, maxreads=5e9):
        """The barcode rescue over a file, plain or gzip by name, through count_file's readers (accumulates)."""
        open(path, 'rb').close()
        B.check(self._L.td_bcrescue_file(self._h, os.fsencode(path), effective_maxreads(maxreads)))

    def bcrescue_stats(self):
        """{reads, exact, rescued1, rescued2, ambiguous, none, tagged, min_entry_distance}, cumulative since bcrescue_begin."""
        st = (C.c_uint64 * 8)()
        B.check(self._L.td_bcrescue_stats(self._h, st))
        return dict(zip(BCRESCUE_STATS, (int(x) for x in st)))

    def bcrescue_fetch(self):
        """(matrix uint32 [barnum, ntags], row_rescued uint64 [barnum, 2], positions uint64 [32]) as numpy arrays."""
        import numpy as np
        barnum, ntags = getattr(self, "_bcrescue_shape", (0, 0))
        matrix = np.zeros((barnum, ntags), dtype=np.uint32)
        rows = np.zeros((barnum, 2), dtype=np.uint64)
        positions = np.zeros(BCRESCUE_POSITIONS, dtype=np.uint64)
        B.check(self._L.td_bcrescue_fetch(self._h, C.c_void_p(matrix.ctypes.data) if matrix.size else None,
                                          C.c_void_p(rows.ctypes.data) if rows.size else None, C.c_void_p(positions.ctypes.data)))
        return matrix, rows, positions

    def bcrescue_matrix(self):
        """The device address of the matrix (uint32 [barnum, ntags]); good until bcrescue_end or the next begin."""
        p = C.c_void_p()
        B.check(self._L.td_bcrescue_matrix(self._h, C.byref(p)))
        return p.value

    def bcrescue_end(self):
        B.check(self._L.td_bcrescue_end(self._h))
        self._bcrescue_shape = (0, 0)

    # ------------------------------------------------------------------ tag network (td_tagnet_*; csrc/tagnet.hip)
    def tagnet_build(self, seqs, counts, taglen, ratio_ppm):
        """td_tagnet_build: seqs is the n * taglen ASCII bytes of n distinct ACGT tags, counts their counts.  Returns a
        TagNet (`.stats`: tags, edges, kept, deg0, deg1, hubs, pairs, compares; `.ms`: device time per kernel).  A
        failure raises TagdigError; `.bad_index` holds the tag for TD_E_ALPHABET and TD_E_OVERLAP, `.stats` what is
        known at a TD_E_LIMIT."""
        import numpy as np
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        n = len(counts)
        if len(seqs) != n * int(taglen) and 1 <= int(taglen) <= 64:
            raise ValueError("seqs must hold n * taglen bytes")
        buf = np.frombuffer(bytes(seqs), dtype=np.uint8) if len(seqs) else np.zeros(1, dtype=np.uint8)
        cnt = counts if n else np.zeros(1, dtype=np.uint64)
        out, st, ms = C.c_void_p(), (C.c_uint64 * 8)(), (C.c_double * 6)()
        rc = self._L.td_tagnet_build(self._h, buf.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), n, int(taglen),
                                     int(ratio_ppm), C.byref(out), st, ms)
        if rc:
            err = self._error(rc)
            err.bad_index = self._L.td_last_bad_index() if rc in (-3, -6) else None
            err.stats = dict(zip(TAGNET_STATS, (int(x) for x in st)))
            raise err
        return TagNet(self, out, n, dict(zip(TAGNET_STATS, (int(x) for x in st))), dict(zip(TAGNET_MS, ms)))

    def _tagnet_fetch(self, call, capacity):
        import numpy as np
        n = C.c_uint64(0)
        if capacity is None:
            B.check(call(None, 0, C.byref(n)))
            capacity = n.value
        out = np.zeros((max(1, int(capacity)), 2), dtype=np.uint32)
        B.check(call(out.ctypes.data_as(C.c_void_p), int(capacity), C.byref(n)))
        return out[:min(int(capacity), n.value)], n.value

    def tagnet_edges(self, net, kept_only=True, capacity=None):
        """td_tagnet_edges: (uint32 [k, 2] edges i < j ascending, how many there are); capacity None: all of them."""
        return self._tagnet_fetch(lambda p, c, n: self._L.td_tagnet_edges(self._h, net.ptr, 1 if kept_only else 0, p, c, n),
                                  capacity)

    def tagnet_pairs(self, net, capacity=None):
        """td_tagnet_pairs: (uint32 [k, 2] pairs i < j ascending, how many there are)."""
        return self._tagnet_fetch(lambda p, c, n: self._L.td_tagnet_pairs(self._h, net.ptr, p, c, n), capacity)

    def tagnet_degrees(self, net):
        """td_tagnet_degrees: uint32 [n], kept edges at every tag."""
        import numpy as np
        deg = np.zeros(max(1, net.n), dtype=np.uint32)
        B.check(self._L.td_tagnet_degrees(self._h, net.ptr, deg.ctypes.data_as(C.c_void_p)))
        return deg[:net.n]

    def tagnet_free(self, net):
        net.close()

    # ------------------------------------------------------------------ tag placement (td_place_*; csrc/place.hip)
    def place_sites(self, d_seq, nbytes, rec_start, remnants, taglen):
        """td_place_sites over a framed genome in device memory: rec_start holds the R + 1 record bounds.  Returns a
        Place.  A failure raises TagdigError with `.stats` holding what is known."""
        import numpy as np
        rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
        out, st, ms = C.c_void_p(), (C.c_uint64 * 8)(), (C.c_double * 4)()
        rc = self._L.td_place_sites(self._h, C.c_void_p(d_seq) if d_seq else None, int(nbytes), rs.ctypes.data_as(C.c_void_p),
                                    len(rs) - 1, _c_strings(remnants), len(remnants), int(taglen), C.byref(out), st, ms)
        stats = dict(zip(PLACE_STATS, (int(x) for x in st)))
        if rc:
            err = self._error(rc)
            err.stats = stats
            raise err
        return Place(self, out, int(taglen), stats, dict(zip(PLACE_MS, ms)))

    def place_loci(self, place, windows=False):
        """td_place_loci: (x uint64 [n], record uint32 [n], strand uint8 [n], windows as a list of str or None)."""
        import numpy as np
        n, L = place.n, place.taglen
        x, rec, strand = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint32), np.zeros(max(1, n), np.uint8)
        win = C.create_string_buffer(max(1, n * L)) if windows else None
        B.check(self._L.td_place_loci(self._h, place.ptr, x.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p),
                                      strand.ctypes.data_as(C.c_void_p), win))
        text = win.raw[:n * L].decode("ascii") if windows else None
        return x[:n], rec[:n], strand[:n], [text[i * L:(i + 1) * L] for i in range(n)] if windows else None

    def place_tags(self, place, seqs, n, max_mismatch):
        """td_place_tags: seqs is the n * taglen ASCII bytes of n ACGT tags.  Returns (n_at uint32 [n, 4], dist uint8 [n],
        locus uint64 [n], stats, ms).  A failure raises TagdigError; `.bad_index` holds the tag for TD_E_ALPHABET,
        `.stats` what is known at a TD_E_LIMIT."""
        import numpy as np
        n = int(n)
        if len(seqs) != n * place.taglen:
            raise ValueError("seqs must hold n * taglen bytes")
        buf = np.frombuffer(bytes(seqs), dtype=np.uint8) if len(seqs) else np.zeros(1, dtype=np.uint8)
        n_at, dist, locus = np.zeros((max(1, n), 4), np.uint32), np.zeros(max(1, n), np.uint8), np.zeros(max(1, n), np.uint64)
        st, ms = (C.c_uint64 * 8)(), (C.c_double * 4)()
        rc = self._L.td_place_tags(self._h, place.ptr, buf.ctypes.data_as(C.c_void_p), n, int(max_mismatch),
                                   n_at.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p),
                                   locus.ctypes.data_as(C.c_void_p), st, ms)
        stats = dict(zip(PLACED_STATS, (int(x) for x in st)))
        if rc:
            err = self._error(rc)
            err.bad_index = self._L.td_last_bad_index() if rc == -6 else None
            err.stats = stats
            raise err
        return n_at[:n], dist[:n], locus[:n], stats, dict(zip(PLACED_MS, ms))

    # ------------------------------------------------------------------ what the matrix calls below share
    @contextlib.contextmanager
    def _device_matrix(self, matrix, shape, dtype, columns, none_ok=True):
        """(device pointer, rows, columns) of an input matrix: a device pointer (None or 0 where none_ok: a null
        pointer) with shape=(rows, columns), taken where it lies, or a host matrix of `dtype` (uint8, or uint32 by
        counts_as_uint32), uploaded and freed on exit.  `columns` names the second axis in the messages."""
        import numpy as np
        if isinstance(matrix, int) or (none_ok and matrix is None):
            if shape is None:
                raise ValueError("a device pointer needs shape=(samples, {})".format(columns))
            rows, cols = (int(x) for x in shape)
            yield matrix or 0, rows, cols
            return
        if dtype == np.uint32:
            host = counts_as_uint32(matrix)
        else:
            host = np.ascontiguousarray(matrix)
            if host.ndim != 2 or host.dtype != np.uint8:
                raise ValueError("the call matrix must be a uint8 matrix (samples x {})".format(columns))
        d = self.dev_alloc(host.nbytes) if host.size else 0
        try:
            if host.size:
                B.check(self._L.td_memcpy_h2d(self._h, C.c_void_p(d), host.ctypes.data_as(C.c_void_p), host.nbytes))
            yield (d,) + host.shape
        finally:
            if d:
                self.dev_free(d)

    @staticmethod
    def _marker_mask(use, M):
        """The marker mask as M bytes 0 / 1 (a marker takes part iff its entry is not zero); None for none or M == 0."""
        import numpy as np
        if use is None:
            return None
        use = np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8)
        if use.shape != (M,):
            raise ValueError("use must have one entry per marker")
        return use if M else None

    def _error(self, rc):
        """The TagdigError of a call that answered rc, from the library's error slot; the caller adds its attributes."""
        return B.TagdigError(rc, (self._L.td_last_error() or b"").decode("utf-8", "replace"))

    # ------------------------------------------------------------------ genotype calls (td_geno_call; csrc/genocall.hip)
    def geno_call(self, counts, i0, i1, het_min, shape=None, rule=0, err_ppm=10000, min_depth=1, min_call_ppm=0,
                  min_maf_ppm=0, max_het_ppm=1000000, fetch_calls=True, keep_device=False):
        """td_geno_call: genotype calls, per-marker statistics and the filter mask of the markers (i0[m], i1[m]) --
        pairs of columns -- of a samples x tags count matrix.  counts is a numpy matrix (uploaded; see counts_as_uint32)
        or a device pointer with shape=(S, T): a matrix the counter or fold_rows filled is called where it lies.
        het_min: the 128 thresholds of tagdigger_fun.het_threshold_table.  fetch_calls=False leaves the calls on the
        device (statistics and mask only); keep_device=True hands their device buffer out as `.d_calls`.  Returns a
        GenoCalls.  A failure raises TagdigError; `.bad_index` holds the marker for a bad pair of columns."""
        import numpy as np
        i0 = np.ascontiguousarray(i0, dtype=np.uint32)
        i1 = np.ascontiguousarray(i1, dtype=np.uint32)
        het = np.ascontiguousarray(het_min, dtype=np.uint16)
        if i0.ndim != 1 or i0.shape != i1.shape:
            raise ValueError("i0 and i1 must be two index lists of one length")
        if het.shape != (GENO_TABLE,):
            raise ValueError("het_min must have {} entries".format(GENO_TABLE))
        M = len(i0)
        with self._device_matrix(counts, shape, np.uint32, "tags", none_ok=False) as (d_counts, S, T):
            par = B.GenoParams(int(rule), int(err_ppm), int(min_depth), int(min_call_ppm), int(min_maf_ppm), int(max_het_ppm), 0)
            calls = np.zeros((S, M), dtype=np.uint8) if fetch_calls else None
            stats = np.zeros((max(1, M), len(GENO_STATS)), dtype=np.uint64)
            mask = np.zeros(max(1, M), dtype=np.uint8)
            passed, ms, d_calls = C.c_uint64(0), C.c_double(0), C.c_void_p()
            idx0, idx1 = (a if M else np.zeros(1, dtype=np.uint32) for a in (i0, i1))
            rc = self._L.td_geno_call(self._h, C.c_void_p(d_counts) if d_counts else None, S, T, M,
                                      idx0.ctypes.data_as(C.c_void_p), idx1.ctypes.data_as(C.c_void_p),
                                      het.ctypes.data_as(C.c_void_p), C.byref(par),
                                      calls.ctypes.data_as(C.c_void_p) if fetch_calls and calls.size else None,
                                      C.byref(d_calls) if keep_device else None, stats.ctypes.data_as(C.c_void_p),
                                      mask.ctypes.data_as(C.c_void_p), C.byref(passed), C.byref(ms))
        if rc:
            err = self._error(rc)
            err.bad_index = self._L.td_last_bad_index() if rc == -2 and err.detail.startswith("marker ") else None
            raise err
        return GenoCalls(calls, {k: stats[:M, j].copy() for j, k in enumerate(GENO_STATS)}, mask[:M].astype(bool),
                         ms.value, passed.value, d_calls.value if keep_device else None)

    # ------------------------------------------------------------------ dosage calls (td_dose_call; csrc/dosage.hip)
    def dose_call(self, counts, i0, i1, ca, cb, cp=None, shape=None, ploidy=4, prior=1, err_ppm=10000, min_depth=1,
                  min_margin=0, min_call_ppm=0, min_maf_ppm=0, fetch_calls=True, diploid=False, keep_device=False,
                  keep_diploid=False):
        """td_dose_call: allele dosage calls 0 .. ploidy (255 missing), per-marker statistics and the filter mask of the
        markers (i0[m], i1[m]) of a samples x tags count matrix; counts and shape as for geno_call.  ca, cb: ploidy + 1
        costs each; cp: DOSE_BINS x (ploidy + 1) costs, None with prior 0 (flat) -- tagdigger_fun.dosage_tables builds
        all three.  diploid=True computes the diploidised matrix (0, 1, 2, 3 missing) as well.  fetch_calls=False
        leaves both matrices on the device; keep_device=True hands the device buffer of the dosages out as `.d_calls`,
        keep_diploid=True that of the diploidised matrix as `.d_diploid` (computed for it if need be): the caller's to
        dev_free.  Returns a DoseCalls.  A failure raises TagdigError;
        `.bad_index` holds the marker for a bad pair of columns."""
        import numpy as np
        i0 = np.ascontiguousarray(i0, dtype=np.uint32)
        i1 = np.ascontiguousarray(i1, dtype=np.uint32)
        if i0.ndim != 1 or i0.shape != i1.shape:
            raise ValueError("i0 and i1 must be two index lists of one length")
        P = int(ploidy)
        ca = np.ascontiguousarray(ca, dtype=np.uint32)
        cb = np.ascontiguousarray(cb, dtype=np.uint32)
        if 2 <= P <= DOSE_MAX_PLOIDY and (ca.shape != (P + 1,) or cb.shape != (P + 1,)):      # (the library refuses another ploidy)
            raise ValueError("ca and cb must have ploidy + 1 entries")
        if cp is not None:
            cp = np.ascontiguousarray(cp, dtype=np.uint32)
            if 2 <= P <= DOSE_MAX_PLOIDY and cp.shape != (DOSE_BINS, P + 1):
                raise ValueError("cp must have {} rows of ploidy + 1 entries".format(DOSE_BINS))
        M = len(i0)
        with self._device_matrix(counts, shape, np.uint32, "tags", none_ok=False) as (d_counts, S, T):
            par = B.DoseParams(P, int(prior), int(err_ppm), int(min_margin), int(min_depth), int(min_call_ppm), int(min_maf_ppm))
            calls = np.zeros((S, M), dtype=np.uint8) if fetch_calls else None
            dip = np.zeros((S, M), dtype=np.uint8) if fetch_calls and diploid else None
            stats = np.zeros((max(1, M), len(DOSE_STATS)), dtype=np.uint64)
            mask = np.zeros(max(1, M), dtype=np.uint8)
            passed, ms, d_calls, d_dip = C.c_uint64(0), C.c_double(0), C.c_void_p(), C.c_void_p()
            idx0, idx1 = (a if M else np.zeros(1, dtype=np.uint32) for a in (i0, i1))
            rc = self._L.td_dose_call(self._h, C.c_void_p(d_counts) if d_counts else None, S, T, M,
                                      idx0.ctypes.data_as(C.c_void_p), idx1.ctypes.data_as(C.c_void_p),
                                      ca.ctypes.data_as(C.c_void_p), cb.ctypes.data_as(C.c_void_p),
                                      cp.ctypes.data_as(C.c_void_p) if cp is not None else None, C.byref(par),
                                      calls.ctypes.data_as(C.c_void_p) if calls is not None and calls.size else None,
                                      C.byref(d_calls) if keep_device else None,
                                      dip.ctypes.data_as(C.c_void_p) if dip is not None and dip.size else None,
                                      C.byref(d_dip) if keep_diploid else None, stats.ctypes.data_as(C.c_void_p),
                                      mask.ctypes.data_as(C.c_void_p), C.byref(passed), C.byref(ms))
        if rc:
            err = self._error(rc)
            err.bad_index = self._L.td_last_bad_index() if rc == -2 and err.detail.startswith("marker ") else None
            raise err
        return DoseCalls(calls, dip, {k: stats[:M, j].copy() for j, k in enumerate(DOSE_STATS)}, mask[:M].astype(bool), ms.value,
                         passed.value, d_calls.value if keep_device else None, d_dip.value if keep_diploid else None)

    # ------------------------------------------------------------------ VCF export (td_vcf_format, td_vcf_file; csrc/vcf.hip)
    @contextlib.contextmanager
    def _vcf_inputs(self, counts, calls, i0, i1, sel, prefixes, shape, ploidy, likelihoods, ca, cb, range_bytes):
        """The arguments both VCF entry points share, as ctypes values: (argument tuple, K).  counts as for geno_call
        (shape=(S, T) with a device pointer); calls a uint8 matrix [S, M] (uploaded) or a device pointer; prefixes: K
        bytes objects, or the pair (all bytes, K + 1 offsets)."""
        import numpy as np
        i0 = np.ascontiguousarray(i0, dtype=np.uint32)
        i1 = np.ascontiguousarray(i1, dtype=np.uint32)
        if i0.ndim != 1 or i0.shape != i1.shape:
            raise ValueError("i0 and i1 must be two index lists of one length")
        M = len(i0)
        sel = np.ascontiguousarray(sel, dtype=np.uint32)
        if sel.ndim != 1:
            raise ValueError("sel must be a list of marker indices")
        K = len(sel)
        if isinstance(prefixes, tuple):
            blob, poff = bytes(prefixes[0]), np.ascontiguousarray(prefixes[1], dtype=np.uint64)
        else:
            blob = b"".join(prefixes)
            poff = np.zeros(len(prefixes) + 1, dtype=np.uint64)
            if len(prefixes):
                poff[1:] = np.cumsum([len(p) for p in prefixes], dtype=np.uint64)
        if poff.shape != (K + 1,):
            raise ValueError("one prefix per entry of sel (K + 1 offsets)")
        par = B.VcfParams(int(ploidy), 1 if likelihoods else 0, int(range_bytes or 0))
        if ca is not None or cb is not None:
            ca, cb = [int(x) for x in ca], [int(x) for x in cb]
            if len(ca) != 3 or len(cb) != 3:
                raise ValueError("ca and cb must have three entries")
            par.ca[:], par.cb[:] = ca, cb
        with self._device_matrix(counts, shape, np.uint32, "tags", none_ok=False) as (d_counts, S, T):
            with self._device_matrix(calls, (S, M) if isinstance(calls, int) else None, np.uint8, "markers", none_ok=False) as (d_calls, S2, M2):
                if (S2, M2) != (S, M):
                    raise ValueError("the call matrix must be samples x markers ({} x {}), not {} x {}".format(S, M, S2, M2))
                idx0, idx1, selx = (a if len(a) else np.zeros(1, dtype=np.uint32) for a in (i0, i1, sel))
                keep = (idx0, idx1, selx, poff, blob, par)           # alive until the call has returned
                yield (self._h, C.c_void_p(d_counts) if d_counts else None, S, T, M, idx0.ctypes.data_as(C.c_void_p),
                       idx1.ctypes.data_as(C.c_void_p), C.c_void_p(d_calls) if d_calls else None, C.byref(par),
                       selx.ctypes.data_as(C.c_void_p), K, C.cast(C.c_char_p(blob), C.c_void_p), poff.ctypes.data_as(C.c_void_p)), K
                del keep

    def _vcf_error(self, rc):
        err = self._error(rc)
        err.bad_index = self._L.td_last_bad_index() if rc == -2 and err.detail.startswith(("marker ", "sel[", "prefix_off[")) else None
        return err

    def vcf_format(self, counts, calls, i0, i1, sel, prefixes, shape=None, ploidy=2, likelihoods=False, ca=None, cb=None,
                   range_bytes=0, measure_only=False, capacity=None):
        """td_vcf_format: the VCF body lines of the markers sel[k] -- prefixes[k], a tab and GT:AD:DP(:GQ:PL) per sample,
        a newline -- formatted on the device from the count matrix and the calls (see include/tagdig.h).  counts and
        shape as for geno_call; calls: a uint8 matrix [S, M] or the device pointer geno_call / dose_call kept.  ca, cb:
        the three costs each of tagdigger_fun.dosage_tables(2, err), read with likelihoods.  measure_only=True emits
        nothing.  capacity: the bytes of the output buffer (default: what a measuring call reports).  Returns a VcfText.
        A failure raises TagdigError; `.bad_index` holds the index at fault, `.needed` the bytes for TD_E_LIMIT."""
        import numpy as np
        with self._vcf_inputs(counts, calls, i0, i1, sel, prefixes, shape, ploidy, likelihoods, ca, cb, range_bytes) as (args, K):
            line_off = np.zeros(K + 1, dtype=np.uint64)
            n_out, ms = C.c_uint64(0), (C.c_double * 3)()
            rc = self._L.td_vcf_format(*args, line_off.ctypes.data_as(C.c_void_p), None, 0, C.byref(n_out), ms)
            out = None
            if not rc and not measure_only:
                cap = n_out.value if capacity is None else int(capacity)
                out = np.zeros(max(1, cap), dtype=np.uint8)
                rc = self._L.td_vcf_format(*args, line_off.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cap,
                                           C.byref(n_out), ms)
        if rc:
            err = self._vcf_error(rc)
            err.needed = n_out.value
            raise err
        return VcfText(None if out is None else out[:n_out.value].tobytes(), n_out.value, line_off, dict(zip(VCF_MS, ms)), None)

    def vcf_file(self, path, counts, calls, i0, i1, sel, prefixes, shape=None, ploidy=2, likelihoods=False, ca=None, cb=None,
                 range_bytes=0, append=False):
        """td_vcf_file: the text of vcf_format written to `path` (append=False truncates), range by range while the next
        range is formatted.  Returns a VcfText without text or line offsets; `.ranges` is how many ranges it took."""
        with self._vcf_inputs(counts, calls, i0, i1, sel, prefixes, shape, ploidy, likelihoods, ca, cb, range_bytes) as (args, K):
            n_out, ranges, ms = C.c_uint64(0), C.c_uint64(0), (C.c_double * 4)()
            rc = self._L.td_vcf_file(*args, os.fsencode(path), 1 if append else 0, C.byref(n_out), C.byref(ranges), ms)
        if rc:
            raise self._vcf_error(rc)
        return VcfText(None, n_out.value, None, dict(zip(VCF_MS + ("write",), ms)), ranges.value)

    # ------------------------------------------------------------------ sample relations (td_relate_joint; csrc/relate.hip)
    def relate_joint(self, calls, shape=None, use=None, fetch=True, keep_device=False):
        """td_relate_joint: joint[i][j][a][b] = the markers at which sample i is called a and sample j is called b
        (a, b in 0 .. 2; any byte above 2 is missing), for every ordered pair of samples.  calls is a numpy uint8 matrix
        [S, M] (uploaded) or a device pointer with shape=(S, M): the calls Engine.geno_call(keep_device=True) left on
        the device are read where they lie.  use: M bytes, a marker takes part iff its byte is not zero (None: all).
        fetch=False leaves the table on the device; keep_device=True hands its device buffer out as `.d_joint`.
        Returns a RelateJoint.  A failure raises TagdigError."""
        import numpy as np
        with self._device_matrix(calls, shape, np.uint8, "markers") as (d_calls, S, M):
            use = self._marker_mask(use, M)
            in_range = S <= RELATE_MAX_SAMPLES and M < 1 << 31     # (the library answers TD_E_ARG otherwise)
            joint = np.zeros((S, S, 3, 3), dtype=np.uint32) if fetch and in_range else None
            ms, d_joint = C.c_double(0), C.c_void_p()
            rc = self._L.td_relate_joint(self._h, C.c_void_p(d_calls) if d_calls else None, S, M,
                                         use.ctypes.data_as(C.c_void_p) if use is not None else None,
                                         joint.ctypes.data_as(C.c_void_p) if joint is not None and joint.size else None,
                                         C.byref(d_joint) if keep_device else None, C.byref(ms))
        B.check(rc)
        return RelateJoint(joint, ms.value, d_joint.value if keep_device else None)

    # ------------------------------------------------------------------ marker LD (td_ld_pairs; csrc/ld.hip)
    def ld_pairs(self, calls, shape=None, use=None, min_r2_ppm=800000, min_shared=50, capacity=None, retry=True,
                 count_only=False):
        """td_ld_pairs: the pairs of participating markers i < j with n >= min_shared, var_i > 0, var_j > 0 and
        cov^2 * 10^6 >= min_r2_ppm * var_i * var_j over the samples called at both (include/tagdig.h has the rule).
        calls is a numpy uint8 matrix [S, M] (uploaded) or a device pointer with shape=(S, M).  use: M bytes, a marker
        takes part iff its byte is not zero (None: all).  capacity: records of the first buffer (None: 8 per marker, at
        least 2^16 and at most 2^20, 24 MB); when there are more edges the call is made once more with the exact size -- unless
        retry=False, with which the TagdigError of TD_E_LIMIT is raised and carries what is complete all the same as `.n`,
        `.degree` and `.called`.  count_only=True passes no buffer: no edges, but n, degree and called.  Returns an
        LDPairs.  A failure raises TagdigError."""
        import numpy as np
        with self._device_matrix(calls, shape, np.uint8, "markers") as (d_calls, S, M):
            use = self._marker_mask(use, M)
            in_range = M < 1 << 31                               # (the library answers TD_E_ARG otherwise)
            degree = np.zeros(max(1, M if in_range else 1), dtype=np.uint32)
            called = np.zeros(max(1, M if in_range else 1), dtype=np.uint32)
            capacity = max(1 << 16, min(8 * M, 1 << 20) if in_range else 0) if capacity is None else max(0, int(capacity))
            n, ms, total_ms = C.c_uint64(0), C.c_double(0), 0.0
            for attempt in range(2):
                edges = np.zeros(0 if count_only else max(1, capacity), dtype=LD_EDGE)
                rc = self._L.td_ld_pairs(self._h, C.c_void_p(d_calls) if d_calls else None, S, M,
                                         use.ctypes.data_as(C.c_void_p) if use is not None else None, int(min_r2_ppm),
                                         int(min_shared), None if count_only else edges.ctypes.data_as(C.c_void_p), capacity, C.byref(n),
                                         degree.ctypes.data_as(C.c_void_p), called.ctypes.data_as(C.c_void_p), C.byref(ms))
                total_ms += ms.value
                if rc == B.TD_E_LIMIT and n.value > capacity and attempt == 0 and retry:     # once more with the exact size
                    capacity = n.value
                    continue
                break
        if rc:
            err = self._error(rc)
            err.n, err.degree, err.called = n.value, degree[:M], called[:M]
            raise err
        t = (C.c_double * 3)()
        B.check(self._L.td_ld_last_times(self._h, t))
        return LDPairs(edges[:0 if count_only else n.value].copy(), n.value, degree[:M], called[:M], total_ms,
                       dict(transpose_ms=t[0], pairs_ms=t[1], sort_ms=t[2]))

    # ------------------------------------------------------------------ linkage of a cross (td_link_counts, td_link_pairs; csrc/link.hip)
    @staticmethod
    def _offspring_rows(rows):
        """The offspring rows as a uint32 array, or None for all rows (the library checks the indices)."""
        import numpy as np
        if rows is None:
            return None
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        if rows.ndim != 1:
            raise ValueError("rows must be a list of row indices")
        return rows

    def link_counts(self, calls, shape=None, rows=None):
        """td_link_counts: (c0, c1, c2, cmiss) of every marker over the offspring rows (any byte above 2 is missing).
        calls is a numpy uint8 matrix [S, M] (uploaded) or a device pointer with shape=(S, M).  rows: the offspring row
        indices (None: every row).  Returns (counts uint32 [M, 4], ms).  A failure raises TagdigError."""
        import numpy as np
        rows = self._offspring_rows(rows)
        with self._device_matrix(calls, shape, np.uint8, "markers") as (d_calls, S, M):
            R = S if rows is None else len(rows)
            counts = np.zeros((max(1, M if M < 1 << 31 else 1), 4), dtype=np.uint32)
            ms = C.c_double(0)
            rc = self._L.td_link_counts(self._h, C.c_void_p(d_calls) if d_calls else None, S, M,
                                        rows.ctypes.data_as(C.c_void_p) if rows is not None else None, R,
                                        counts.ctypes.data_as(C.c_void_p), C.byref(ms))
        B.check(rc)
        return counts[:M], ms.value

    def link_pairs(self, calls, cls, lodtab, shape=None, rows=None, max_rf_ppm=500000, min_lod16=LINK_LOD_MIN, min_shared=0,
                   capacity=None, retry=True, count_only=False):
        """td_link_pairs: the pairs of participating markers i < j with N >= min_shared, rec * 10^6 <= max_rf_ppm * N and
        lod16 >= min_lod16 over the offspring rows (include/tagdig.h has the rule).  calls is a numpy uint8 matrix [S, M]
        (uploaded) or a device pointer with shape=(S, M).  cls: M bytes, a marker's class pair 0 = (A 0, B 1), 1 = (A 2,
        B 1), 2 = (A 0, B 2) or LINK_NO_PART.  lodtab: int64, at least R + 1 entries (tagdigger_fun.linkage_tables).
        rows: the offspring row indices (None: every row).  capacity, retry, count_only: as Engine.ld_pairs; the
        TagdigError of TD_E_LIMIT carries `.n`, `.degree` and `.informative`.  Returns a LinkPairs."""
        import numpy as np
        rows = self._offspring_rows(rows)
        if cls is not None:
            cls = np.ascontiguousarray(cls, dtype=np.uint8)
        if lodtab is not None:
            lodtab = np.ascontiguousarray(lodtab, dtype=np.int64)
        with self._device_matrix(calls, shape, np.uint8, "markers") as (d_calls, S, M):
            R = S if rows is None else len(rows)
            in_range = M < 1 << 31                               # (the library answers TD_E_ARG otherwise)
            if cls is not None and in_range and cls.shape != (M,):
                raise ValueError("cls must have one byte per marker")
            if lodtab is not None and R <= LINK_MAX_SAMPLES and (lodtab.ndim != 1 or len(lodtab) < R + 1):
                raise ValueError("lodtab must have at least R + 1 = {} entries".format(R + 1))
            degree = np.zeros(max(1, M if in_range else 1), dtype=np.uint32)
            informative = np.zeros(max(1, M if in_range else 1), dtype=np.uint32)
            capacity = max(1 << 16, min(8 * M, 1 << 20) if in_range else 0) if capacity is None else max(0, int(capacity))
            n, ms, total_ms = C.c_uint64(0), C.c_double(0), 0.0
            for attempt in range(2):
                edges = np.zeros(0 if count_only else max(1, capacity), dtype=LINK_EDGE)
                rc = self._L.td_link_pairs(self._h, C.c_void_p(d_calls) if d_calls else None, S, M,
                                           rows.ctypes.data_as(C.c_void_p) if rows is not None else None, R,
                                           cls.ctypes.data_as(C.c_void_p) if cls is not None and cls.size else None,
                                           lodtab.ctypes.data_as(C.c_void_p) if lodtab is not None else None, int(max_rf_ppm),
                                           int(min_lod16), int(min_shared), None if count_only else edges.ctypes.data_as(C.c_void_p),
                                           capacity, C.byref(n), degree.ctypes.data_as(C.c_void_p),
                                           informative.ctypes.data_as(C.c_void_p), C.byref(ms))
                total_ms += ms.value
                if rc == B.TD_E_LIMIT and n.value > capacity and attempt == 0 and retry:     # once more with the exact size
                    capacity = n.value
                    continue
                break
        if rc:
            err = self._error(rc)
            err.n, err.degree, err.informative = n.value, degree[:M], informative[:M]
            raise err
        t = (C.c_double * 4)()
        B.check(self._L.td_link_last_times(self._h, t))
        return LinkPairs(edges[:0 if count_only else n.value].copy(), n.value, degree[:M], informative[:M], total_ms,
                         dict(gather_ms=t[1], pairs_ms=t[2], sort_ms=t[3]))

    # ------------------------------------------------------------------ LD-kNN imputation (td_impute_knn; csrc/impute.hip)
    def impute_knn(self, calls, nbr, shape=None, k=10, min_overlap=4, min_conf_ppm=600000, fetch=True, keep_device=False):
        """td_impute_knn: every missing cell (a byte above 2) of the call matrix is filled by the vote of the k samples
        most alike over the marker's neighbours, or keeps its byte (include/tagdig.h has the rule).  calls is a numpy
        uint8 matrix [S, M] (uploaded) or a device pointer with shape=(S, M).  nbr: int32 [M, L], row m the markers that
        stand in for marker m, -1 where there is none (tagdigger_fun.ld_neighbours).  fetch=False leaves the filled matrix
        on the device; keep_device=True hands its device buffer out as `.d_calls`.  Returns an ImputeKnn.  A failure
        raises TagdigError; `.bad_index` holds the marker for a bad row of the table."""
        import numpy as np
        nbr = np.ascontiguousarray(nbr, dtype=np.int32)
        if nbr.ndim != 2:
            raise ValueError("the neighbour table must have two dimensions (markers x neighbours)")
        with self._device_matrix(calls, shape, np.uint8, "markers") as (d_calls, S, M):
            in_range = S <= IMPUTE_MAX_SAMPLES and M < 1 << 31     # (the library answers TD_E_ARG otherwise)
            if in_range and nbr.shape[0] != M:
                raise ValueError("the neighbour table must have one row per marker")
            par = B.ImputeParams(nbr.shape[1], int(k), int(min_overlap), int(min_conf_ppm))
            out = np.zeros((S, M), dtype=np.uint8) if fetch and in_range else None
            stats = np.zeros((max(1, M if in_range else 1), len(IMPUTE_STATS)), dtype=np.uint32)
            ms, d_out = C.c_double(0), C.c_void_p()
            rc = self._L.td_impute_knn(self._h, C.c_void_p(d_calls) if d_calls else None, S, M,
                                       nbr.ctypes.data_as(C.c_void_p) if nbr.size else None, C.byref(par),
                                       out.ctypes.data_as(C.c_void_p) if out is not None and out.size else None,
                                       C.byref(d_out) if keep_device else None, stats.ctypes.data_as(C.c_void_p), C.byref(ms))
        if rc:
            err = self._error(rc)
            err.bad_index = self._L.td_last_bad_index() if rc == -2 and err.detail.startswith("neighbours of marker ") else None
            raise err
        t = (C.c_double * 2)()
        B.check(self._L.td_impute_last_times(self._h, t))
        return ImputeKnn(out, stats[:M], ms.value, dict(transpose_ms=t[0], vote_ms=t[1]), d_out.value if keep_device else None)

    # ------------------------------------------------------------------ parent pairs (td_parent_trios; csrc/parent.hip)
    def parent_trios(self, calls, offspring, cand, shape=None, use=None, selfing=True, top=2, min_shared=50, fetch_table=False):
        """td_parent_trios: for every offspring row and every pair of its candidate slots, n = the participating markers
        at which offspring and both candidates are called and e = those at which the offspring's call is none the two can
        produce; the first `top` trios with n >= min_shared by (e / n ascending, n descending, trio number ascending)
        (include/tagdig.h has the rule).  calls is a numpy uint8 matrix [S, M] (uploaded) or a device pointer with
        shape=(S, M).  offspring: O sample indices.  cand: int32 [O, C], row i the candidate parents of offspring[i], -1
        for an empty slot.  use: M bytes, a marker takes part iff its byte is not zero (None: all).  selfing: the pairs
        (a, a) are trios too.  fetch_table=True brings the whole table to the host as well.  Returns a ParentTrios.  A
        failure raises TagdigError; `.bad_index` holds the row for a bad offspring or candidate entry."""
        import numpy as np
        offspring = np.ascontiguousarray(offspring, dtype=np.uint32)
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        if offspring.ndim != 1 or cand.ndim != 2 or cand.shape[0] != len(offspring):
            raise ValueError("cand must have one row of candidate slots per offspring")
        O, Cn, K = len(offspring), cand.shape[1], int(top)
        with self._device_matrix(calls, shape, np.uint8, "markers") as (d_calls, S, M):
            use = self._marker_mask(use, M)
            in_range = 1 <= Cn <= PARENT_MAX_CAND and 1 <= K <= PARENT_MAX_TOP     # (the library answers TD_E_ARG otherwise)
            T = (Cn * (Cn + 1) // 2 if selfing else Cn * (Cn - 1) // 2) if in_range else 0
            best = np.zeros((O, K if in_range else 1), dtype=PARENT_TRIO)
            table = np.zeros((O, T, 2), dtype=np.uint32) if fetch_table else None
            ms = C.c_double(0)
            rc = self._L.td_parent_trios(self._h, C.c_void_p(d_calls) if d_calls else None, S, M,
                                         use.ctypes.data_as(C.c_void_p) if use is not None else None,
                                         offspring.ctypes.data_as(C.c_void_p) if O else None, O,
                                         cand.ctypes.data_as(C.c_void_p) if cand.size else None, Cn,
                                         PARENT_SELFING if selfing else 0, max(0, K), int(min_shared),
                                         best.ctypes.data_as(C.c_void_p) if best.size else None,
                                         table.ctypes.data_as(C.c_void_p) if fetch_table and table.size else None, C.byref(ms))
        if rc:
            err = self._error(rc)
            err.bad_index = self._L.td_last_bad_index() if rc == -2 and err.detail.startswith(("offspring row ", "candidates of row ")) else None
            raise err
        t = (C.c_double * 3)()
        B.check(self._L.td_parent_last_times(self._h, t))
        return ParentTrios(best, table, ms.value, dict(pack_ms=t[0], trio_ms=t[1], rank_ms=t[2]))

    # ------------------------------------------------------------------ expected fragment sizes (exp_frag_size)
    def fasta_frame_device(self, d_text, nbytes, d_out, rec_cap):
        """K1 over one genome file in device memory (td_fasta_frame_device): the reference's line.strip().upper()
        of every sequence line, concatenated, lands at d_out.  Returns (bytes written, numpy uint64 [headers, 3]
        rows: name offsets [lo, hi) in the input and the sequence bytes before the header, holds a byte >= 0x80,
        device ms)."""
        import numpy as np
        n_out, n_rec, nonascii, ms = C.c_uint64(0), C.c_uint64(0), C.c_int(0), C.c_double(0)
        for _ in range(2):        # a second time with the table the file needs (the first call reports its headers)
            rec = np.zeros((max(1, rec_cap), 3), dtype=np.uint64)
            rc = self._L.td_fasta_frame_device(self._h, C.c_void_p(d_text), int(nbytes), C.c_void_p(d_out), C.byref(n_out),
                                               rec.ctypes.data_as(C.c_void_p), int(rec_cap), C.byref(n_rec),
                                               C.byref(nonascii), C.byref(ms))
            if rc == -7 and n_rec.value > rec_cap:
                rec_cap = n_rec.value
                continue
            B.check(rc)
            break
        if nonascii.value:
            return 0, rec[:0], True, ms.value
        return n_out.value, rec[:n_rec.value], False, ms.value

    def frag_search_device(self, d_seq, seq_bytes, jobs, sites):
        """K2 (td_frag_search_device): jobs is a numpy frag_job_dtype() array; returns (int32 [njobs, 4] = size or -1,
        G + C, N, 0; device ms)."""
        import numpy as np
        jobs = np.ascontiguousarray(jobs, dtype=frag_job_dtype())
        out = np.zeros((max(1, len(jobs)), 4), dtype=np.int32)
        arr = (C.c_char_p * max(1, len(sites)))(*[x.encode("ascii") for x in sites])
        ms = C.c_double(0)
        B.check(self._L.td_frag_search_device(self._h, C.c_void_p(d_seq), int(seq_bytes), jobs.ctypes.data_as(C.c_void_p),
                                              len(jobs), arr, len(sites), out.ctypes.data_as(C.c_void_p), C.byref(ms)))
        return out[:len(jobs)], ms.value

    def frag_gather_device(self, d_seq, seq_bytes, jobs, sizes):
        """K3 (td_frag_gather_device): the fragments subseq[:size] of the jobs, packed in job order; returns
        (bytes, device ms)."""
        import numpy as np
        jobs = np.ascontiguousarray(jobs, dtype=frag_job_dtype())
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        cap = int(np.clip(sizes, 0, None).sum())
        buf = np.zeros(max(1, cap), dtype=np.uint8)
        n, ms = C.c_uint64(0), C.c_double(0)
        B.check(self._L.td_frag_gather_device(self._h, C.c_void_p(d_seq), int(seq_bytes), jobs.ctypes.data_as(C.c_void_p),
                                              sizes.ctypes.data_as(C.c_void_p), len(jobs), buf.ctypes.data_as(C.c_void_p),
                                              cap, C.byref(n), C.byref(ms)))
        return buf[:n.value].tobytes(), ms.value

    # ------------------------------------------------------------------ Tag Manager (tag sets)
    def tagset_load(self, seqs, offs, order=None):
        """K1 + K2 (td_tagset_load): seqs is the tags' ASCII bytes, offs their uint64 offsets (n + 1), order the tags
        sorted by name (None: as given).  Returns (TagSet resident on the device, uint32 sorted position -> input
        index, radix passes run, (K1 ms, K2 ms))."""
        import numpy as np
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        buf = np.frombuffer(seqs, dtype=np.uint8) if len(seqs) else np.zeros(1, dtype=np.uint8)
        ordp = None
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            ordp = order.ctypes.data_as(C.c_void_p)
        perm = np.zeros(max(1, n), dtype=np.uint32)
        out, passes, ms = C.c_void_p(), C.c_uint32(0), (C.c_double * 2)()
        B.check(self._L.td_tagset_load(self._h, buf.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), n, ordp,
                                       C.byref(out), perm.ctypes.data_as(C.c_void_p), C.byref(passes), ms))
        return TagSet(self, out, n), perm[:n], passes.value, (ms[0], ms[1])

    def tagset_lookup(self, tagset, seqs, offs, allow_diff_lengths):
        """K3 (td_tagset_lookup): int32 [nq, 4] = f, a, b, c per query (sorted positions, -1: nothing found), device ms."""
        import numpy as np
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nq = len(offs) - 1
        buf = np.frombuffer(seqs, dtype=np.uint8) if len(seqs) else np.zeros(1, dtype=np.uint8)
        out = np.zeros((max(1, nq), 4), dtype=np.int32)
        ms = C.c_double(0)
        B.check(self._L.td_tagset_lookup(self._h, tagset.ptr, buf.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                         nq, 1 if allow_diff_lengths else 0, out.ctypes.data_as(C.c_void_p), C.byref(ms)))
        return out[:nq], ms.value

    def tagset_varsites(self, seqs, offs, idx, goff, trim):
        """K4 (td_tagset_varsites): uint64 [groups, 4] column masks, uint8 [groups] non-ACGT flags, device ms."""
        import numpy as np
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        goff = np.ascontiguousarray(goff, dtype=np.uint64)
        ng = len(goff) - 1
        buf = np.frombuffer(seqs, dtype=np.uint8) if len(seqs) else np.zeros(1, dtype=np.uint8)
        idxb = idx if len(idx) else np.zeros(1, dtype=np.uint32)
        mask = np.zeros((max(1, ng), 4), dtype=np.uint64)
        bad = np.zeros(max(1, ng), dtype=np.uint8)
        ms = C.c_double(0)
        B.check(self._L.td_tagset_varsites(self._h, buf.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                           len(offs) - 1, idxb.ctypes.data_as(C.c_void_p), goff.ctypes.data_as(C.c_void_p),
                                           ng, 1 if trim else 0, mask.ctypes.data_as(C.c_void_p),
                                           bad.ctypes.data_as(C.c_void_p), C.byref(ms)))
        return mask[:ng], bad[:ng], ms.value

    # ------------------------------------------------------------------ MD5 sums (csrc/md5.hip)
    def md5_device(self, d_ptr, offs):
        """td_md5_device: MD5 of the messages d_ptr[offs[i] .. offs[i + 1]) in device memory, one per lane.
        Returns (list of 16-byte digests, device ms)."""
        import numpy as np
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        out = np.zeros((max(1, n), 16), dtype=np.uint8)
        ms = C.c_double(0)
        B.check(self._L.td_md5_device(self._h, d_ptr, offs.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p),
                                      C.byref(ms)))
        return [out[i].tobytes() for i in range(n)], ms.value

    def md5_files(self, paths):
        """td_md5_files: MD5 of every file, streamed through the device, one file per lane.  Returns (list of 16-byte
        digests, (ms reading, ms waiting for the GPU, ms in the kernel)); a file that cannot be opened or read raises
        TagdigError (TD_E_IO) with the file's position in `bad_index`."""
        import numpy as np
        n = len(paths)
        arr = (C.c_char_p * max(1, n))(*[os.fsencode(p) for p in paths])
        out = np.zeros((max(1, n), 16), dtype=np.uint8)
        bad, ms = C.c_uint32(0), (C.c_double * 3)()
        rc = self._L.td_md5_files(self._h, arr, n, out.ctypes.data_as(C.c_void_p), C.byref(bad), ms)
        if rc == -11:
            err = self._error(rc)
            err.bad_index = bad.value
            raise err
        B.check(rc)
        return [out[i].tobytes() for i in range(n)], (ms[0], ms[1], ms[2])

    # ------------------------------------------------------------------ results
    def stats(self):
        st = (C.c_uint64 * B.TD_STAT_NSTATS)()
        B.check(self._L.td_get_stats(self._h, st))
        return {"reads": st[0], "barcut": st[1], "tag": st[2], "lines": st[3]}

    def progress_windows(self, nwindows=None):
        """[(reads with barcode + cut site, reads with tag)] per window of 50 000 reads, in read order (option
        "progress" must have been on while counting); the last window may be partly filled.  nwindows: that many
        windows from read 0 on (a shard of a byte-sharded file holds reads of high ordinals only); default: the
        windows of the reads this engine counted."""
        n = C.c_uint64(0)
        B.check(self._L.td_get_progress(self._h, None, 0, C.byref(n)))
        want = n.value if nwindows is None else int(nwindows)
        out = (C.c_uint64 * max(1, 2 * want))()
        B.check(self._L.td_get_progress(self._h, out, want, C.byref(n)))
        return [(out[2 * i], out[2 * i + 1]) for i in range(want)]

    def progress_lines(self, fqfile):
        """The lines the reference's loop prints while it reads (tagdigger_fun.py:268-271): the file name after
        every 1 000 000 reads, the three counters after every 50 000."""
        reads = self.stats()["reads"]
        lines, bar, tag = [], 0, 0
        for k, (b, t) in enumerate(self.progress_windows()):
            done = 50000 * (k + 1)
            if done > reads:
                break
            bar, tag = bar + b, tag + t
            if done % 1000000 == 0:
                lines.append(fqfile)
            lines.append("Reads: {0} With barcode and cut site: {1} With tag: {2}".format(done, bar, tag))
        return lines

    def counts_flat(self):
        out = (C.c_uint64 * max(1, self.barnum * self.ntags))()
        B.check(self._L.td_get_counts(self._h, out))
        return out

    def counts(self, signed=False):
        """list[list[int]] shaped [barcodes][tags], like the reference's mycounts (:237)."""
        # (numpy's tolist() builds the Python ints in C: 38 M cells in a second instead of half a minute)
        return self.counts_numpy(signed=signed).tolist()

    def counts_numpy(self, signed=False):
        """The same matrix as a numpy array (uint64; int64 when `signed`: tassel weights may be negative)."""
        import numpy as np
        flat = self.counts_flat()
        a = np.frombuffer(flat, dtype=np.int64 if signed else np.uint64, count=self.barnum * self.ntags)
        return a.reshape(self.barnum, self.ntags).copy()

    def debug_counters(self):
        out = (C.c_uint64 * 24)()
        B.check(self._L.td_debug_counters(self._h, out))
        return list(out)

    def kernel_time_ms(self):
        ms = C.c_double(0)
        n = C.c_uint32(0)
        B.check(self._L.td_kernel_time_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_times_ms(self, capacity=4096):
        """Device time of every launch since the last call, in launch order (needs option "timing")."""
        out = (C.c_double * capacity)()
        n = C.c_uint32(0)
        B.check(self._L.td_kernel_times_ms(self._h, out, capacity, C.byref(n)))
        return list(out[:n.value])

    # ------------------------------------------------------------------ device memory helpers
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        B.check(self._L.td_dev_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, ptr):
        B.check(self._L.td_dev_free(self._h, C.c_void_p(ptr)))

    def h2d(self, d_ptr, data):
        n = len(data)
        if n:
            buf = (C.c_char * n).from_buffer_copy(data)
            B.check(self._L.td_memcpy_h2d(self._h, C.c_void_p(d_ptr), buf, n))

    def d2h(self, d_ptr, nbytes):
        buf = (C.c_char * max(1, nbytes))()
        if nbytes:
            B.check(self._L.td_memcpy_d2h(self._h, buf, C.c_void_p(d_ptr), nbytes))
        return bytes(buf[:nbytes])

    def sync(self):
        B.check(self._L.td_device_sync(self._h))


_default = {}


def default_engine(device=0):
    eng = _default.get(device)
    if eng is None:
        eng = _default[device] = Engine(device)
    return eng
