/* libtagdig -- C-ABI of the MI355X tag-counting engine.
 *
 * Drop-in boundary for ONE path of lvclark/tagdigger: the per-read
 * barcode-demux + known-tag count loop, tagdigger_fun.find_tags_fastq
 * (reference tagdigger_fun.py:192-277) and the index primitives under it
 * (:60-190).  The reference has no FFI of its own (it is pure Python); these
 * are the entry points a ctypes binding of that function needs, and
 * tagdigger_amd/_binding.py is that binding (INTEGRATION.md shows the stub a
 * reference maintainer would add).
 *
 * Conventions: plain pointers and sizes only; every buffer is caller-owned
 * unless said otherwise; functions return 0 on success or a negative TD_E_*
 * code with a message available from td_last_error(); nothing here calls
 * exit()/abort().  One handle drives one GPU; a handle is not thread-safe.
 * There is NO CPU fallback: without a usable HIP device td_create fails.
 */
#ifndef TAGDIG_H
#define TAGDIG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct td_handle td_handle;

enum {
    TD_OK = 0,
    TD_E_HIP = -1,        /* a HIP runtime call failed                                   */
    TD_E_ARG = -2,        /* bad argument (NULL, misaligned device pointer, ...)          */
    TD_E_OVERLAP = -3,    /* index build: reference's AssertionError "Problematic
                             sequence: {idx}" (tagdigger_fun.py:82); idx via td_last_bad_index */
    TD_E_EMPTY = -4,      /* index build: empty barcode or tag list (IndexError, :76)     */
    TD_E_ROOTLEAF = -5,   /* index build: first sequence empty, not the :109 special case;
                             the reference dies at its first lookup       */
    TD_E_ALPHABET = -6,   /* non-ACGT character in an index sequence (:198-204 asserts)   */
    TD_E_LIMIT = -7,      /* beyond an implementation limit (barcode+site > 32 bases,
                             tag > 320 bases, > 32767 barcode entries, ...)               */
    TD_E_NONASCII = -8,   /* a counted sequence line holds a byte >= 0x80                 */
    TD_E_STATE = -9,      /* call order (no index set, ...)                               */
    TD_E_INTERNAL = -10,  /* look-back timeout or other should-not-happen condition       */
    TD_E_IO = -11,        /* file could not be opened / read / inflated                   */
    TD_E_TASSEL = -12,    /* tassel_tagcount: header without a parsable count= value      */
    /* a .gz input ends the way gzip.open(fqfile, 'rt') ends it in the reference's loop
     * (tagdigger_fun.py:240-243, :250; csrc/gz_pyrules.hpp): the binding raises the same class
     * with the same message (td_last_error)                                               */
    TD_E_GZ_EOF = -13,    /* the compressed stream stops before its end-of-stream marker: EOFError */
    TD_E_GZ_BADFILE = -14,/* a member fails its CRC-32 / ISIZE check, or what follows a member is no
                             gzip header: gzip.BadGzipFile (an OSError)                    */
    TD_E_GZ_DATA = -15    /* invalid DEFLATE data: zlib.error                              */
};

/* stats[] slots filled by td_get_stats (all cumulative since td_reset) */
enum {
    TD_STAT_READS = 0,    /* readscount   of tagdigger_fun.py:246,255 */
    TD_STAT_BARCUT = 1,   /* barcutcount  of :247,259                 */
    TD_STAT_TAG = 2,      /* tagcount     of :248,263                 */
    TD_STAT_LINES = 3,    /* line terminators seen                    */
    TD_STAT_NSTATS = 8
};

const char *td_last_error(void);
uint32_t td_last_bad_index(void);

/* ---- lifetime ----------------------------------------------------------- */
int td_create(td_handle **out, int device_id);
void td_destroy(td_handle *h);

/* ---- index: replaces build_sequence_tree x2 inside find_tags_fastq --------
 * (tagdigger_fun.py:207-233).  The caller passes exactly the two string
 * lists the reference hands to build_sequence_tree:
 *   barcut[n_barcut]  upper-case barcode+cutsite strings, all cut-site
 *                     variants concatenated as at :215-217; entry k belongs to
 *                     barcode row k % barnum (:102-108)
 *   tagoff[barnum]    barcutlen of :209/:231 -- where the tag search starts
 *   tags[ntags]       upper-case tags after the strip decision of :222-231;
 *                     tag k is count-matrix column k
 * Duplicate / extension shadowing and the overlap assertion of :76-82 are
 * reproduced (TD_E_OVERLAP).  The count matrix becomes barnum x ntags, zeroed.
 * Limits (TD_E_LIMIT): barcode + cut site of at most 32 bases, tagoff at most 63, tags of at most 320 bases -- and
 * behind a tagoff above 32, as many fewer as the widest kernel stages (15 + tagoff + tag length <= 368). */
int td_set_index(td_handle *h,
                 const char *const *barcut, uint32_t n_barcut, uint32_t barnum,
                 const uint32_t *tagoff,
                 const char *const *tags, uint32_t ntags);

/* The shape of the tag hash table that the last td_set_index built: out[TD_INDEX_*].  Known on the host from the
 * insertion itself; nothing runs on the device.  For tests and diagnostics (has an index reached the chains, the ring
 * wrap, the width it was meant to?) -- no count depends on it.  TD_E_STATE without an index. */
enum {
    TD_INDEX_W = 0,           /* 64-bit words per packed tag: 1, 2, 3, 4, 6 or 10                                */
    TD_INDEX_M_BASES = 1,     /* leading bases that are hashed (at most 32); shorter tags are on the short list  */
    TD_INDEX_BUCKETS = 2,     /* buckets of the table (a power of two)                                           */
    TD_INDEX_SPB = 3,         /* slots per bucket                                                                */
    TD_INDEX_NSHORT = 4,      /* tags on the short list                                                          */
    TD_INDEX_DISPLACED = 5,   /* tags that found their home bucket full and lie in a later one                   */
    TD_INDEX_LONGEST = 6,     /* the farthest of them, in buckets from its home bucket                           */
    TD_INDEX_WRAPPED = 7,     /* 1: an insertion went on from the last bucket to bucket 0                        */
    TD_INDEX_NCH = 8,         /* 16-byte chunks staged per read by k_count / k_fast                              */
    TD_INDEX_NCH2 = 9,        /* 16-byte pieces packed per read by k_fast2 / k_fast4 (0: W > 3, they do not run) */
    TD_INDEX_NINFO = 10
};
int td_index_info(td_handle *h, uint64_t out[TD_INDEX_NINFO]);

/* Use caller-provided device memory (barnum*ntags uint32, zeroed by the
 * caller) for the count matrix, e.g. a torch tensor that is later all-reduced
 * over RCCL.  NULL returns to the internal buffer.
 * A bound matrix is the caller's: the library never moves it into its 64-bit host
 * accumulator (the internal matrix is flushed there before a cell could wrap), so a
 * cell wraps silently past 2^32 - 1 hits -- of ONE (barcode, tag) pair, summed over every
 * file counted into the matrix and, after an all-reduce, over every rank.  The reference's
 * default maxreads is 5e9 reads per file; BASELINE's largest job is 1.6e9 reads over
 * 384 x 500 000 cells.  A caller whose single cell may pass 4.29e9 must flush the
 * matrix into wider cells itself (or use the internal matrix and td_get_counts). */
int td_bind_counts(td_handle *h, void *d_counts);

/* Zero the count matrix, the statistics and the host-side accumulators. */
int td_reset(td_handle *h);

/* ---- the hot path: replaces the record loop of find_tags_fastq ------------
 * (tagdigger_fun.py:249-274) on a buffer already resident in HBM.
 *   d_fastq      device pointer, 16-byte aligned, nbytes bytes of FASTQ text
 *                made of whole lines (the last line may lack a terminator)
 *   first_line   global index of the buffer's first line (lineindex of :249)
 *   max_reads    reads (sequence lines) with ordinal > max_reads are ignored;
 *                pass max(1, ceil(maxreads)) for the semantics of :272-273
 *   weights      0 for the plain +1 count (:267); 1 for tassel_tagcount
 *                (:251-253,:264-265): header lines carry count=N, read as int() reads it (ASCII: blanks of
 *                str.strip() around it, a sign, digits with single underscores between them).  A header and
 *                its sequence line must lie in ONE buffer: a header that is the buffer's last line counts
 *                nothing (it still raises if malformed), and first_line = 1 (mod 4) -- a buffer that opens
 *                with a sequence line whose header went before -- is unsupported with weights (the reference
 *                has no answer either: its weight would be unbound).  td_count_host and td_count_file see
 *                to that themselves: with weights on, none of their pieces ends behind a header line.
 *   stream       hipStream_t to launch on (NULL = default stream)
 * Asynchronous: returns once the work is enqueued.  ONE stream in flight per handle: the launch's
 * scratch (per-tile words, fix-up queue, tail copy, block sums) belongs to the handle, so work
 * enqueued through the same handle on a second stream must be ordered behind the first (an event,
 * or a synchronise) -- two unordered launches of one handle would race on it.  Use one handle per
 * concurrent stream. */
int td_count_device(td_handle *h, const void *d_fastq, uint64_t nbytes,
                    uint64_t first_line, uint64_t max_reads, int weights, void *stream);

/* Same for a host buffer: staged through pinned memory in pieces cut at line
 * ends, copies overlapped with counting.  Synchronous.  *lines_out (optional)
 * receives the number of lines consumed; like the reference's loop (:272) the
 * input stops being consumed soon after read number max_reads. */
int td_count_host(td_handle *h, const void *fastq, uint64_t nbytes,
                  uint64_t first_line, uint64_t max_reads, int weights, uint64_t *lines_out);

/* Whole file, plain or gzip (chosen by name as at :240: last two characters
 * 'gz' in any case), streamed.  BGZF is inflated on the GPU; any other gzip stream is
 * decoded by the host's threads and -- from 8 MiB of compressed data -- resolved and
 * CRC-checked on the GPU (options "gpu_inflate", "gpu_resolve").  Synchronous.
 * Environment: TAGDIG_INFLATE_THREADS (default: the host's cores, at most 16),
 * TAGDIG_INFLATE_CHUNK (bytes of compressed data per chunk, default 1 MiB),
 * TAGDIG_COPY_STREAMS (1..3 copy streams side by side for large uploads, default 3),
 * TAGDIG_INFLATE_STATS=1 (a line of timings on stderr). */
int td_count_file(td_handle *h, const char *path, uint64_t max_reads, int weights);

/* The gzip reader td_count_file / td_split_file use, on its own (host only, no GPU; for tests):
 * inflates `path` into dst[0..capacity), asking the reader for `chunk` bytes at a time (0 = 1 MiB).
 * BGZF files (bgzip) are inflated member-parallel on TAGDIG_INFLATE_THREADS threads (default: the
 * host's cores, at most 16); any other gzip stream (what gzip.open reads at tagdigger_fun.py:241,
 * multi-member included) by the library's own DEFLATE decoder: on the calling thread below 8 MiB
 * of compressed data, chunk-parallel on the same number of threads from there (csrc/par_inflate.hpp).
 * Every member's CRC-32 and length are checked.
 * TAGDIG_GUNZIP_PIPELINE=1: the chunk-parallel decoder is driven the way td_count_file drives it for the GPU (its
 * device mode: dev_next / dev_release / dev_check), the markers resolved by the host -- so that the pipeline
 * can be tested where there is no GPU. */
int td_gunzip_file(const char *path, void *dst, uint64_t capacity, uint64_t chunk, uint64_t *n_out);

/* An ordinary (single-member) .gz file inflated ON THE DEVICE (csrc/gz_gpu.hpp: block search, Huffman decoding into
 * tokens, LZ77 and the 32 KiB windows between chunks, CRC-32 and length check -- what td_count_file does with such a
 * file before it counts), its text copied to host memory `dst`.  *on_gpu = 0 and *n_out = 0: the device decoder leaves
 * this file to the host decoders (too small -- option "gz_gpu_min", default 8 MiB of compressed data -- several members,
 * no room on the device, or a stream it does not chain); td_gunzip_file reads such a file.  TD_E_IO: the member fails its
 * CRC-32 check.  Replaces gzip.open(fqfile, 'rt') of tagdigger_fun.py:240-241 for the test of that decoder alone. */
int td_gunzip_file_gpu(td_handle *h, const char *path, void *dst, uint64_t capacity, uint64_t *n_out, int *on_gpu);
/* 1: the .gz file td_count_file counted last was inflated by the device decoder; 0: by one of the others. */
int td_last_gz_route(td_handle *h);

/* ONE ordinary gzip file over several devices (tagdigger_amd/multi.py count_file_sharded; what gzip.open of
 * tagdigger_fun.py:240-241 reads, decoded by N ranks): a rank's part of the pipeline of csrc/gz_gpu.hpp.
 * td_gz_shard_open: the rank's byte range [byte_lo, byte_hi) of the compressed file goes to the device (and the bytes a
 *   margin further); *start_bit = the first block start in it (`first` != 0 -- rank 0: the member's first block), ~0: none.
 * td_gz_shard_decode: the stretch from there to stop_bit -- the next rank's start; ~0: to the member's end -- is decoded
 *   into symbols; *end_bit where it ended (must equal the next rank's start: the caller checks the seams), *out_len its
 *   bytes, *final whether it ended the member, map_out[32768]: what each place of the 32 KiB window behind the stretch
 *   holds -- a byte, or 0x8000 | a place of the window in front of it.
 * td_gz_shard_resolve: with window_in[32768] (the caller applies the maps of the ranks before this one to an empty
 *   window) and the bytes the member inflated to before the stretch: the stretch's text in device memory (*d_text) and its
 *   CRC-32 (td_crc32_join combines the ranks' in order; the caller checks the member's trailer).
 * TD_E_LIMIT: the file is not one this scheme takes (a chunk that does not chain, a stretch larger than a segment): the
 * caller lets one rank count it through td_count_file. */
int td_gz_shard_open(td_handle *h, const char *path, uint64_t byte_lo, uint64_t byte_hi, int first, uint64_t *start_bit, uint64_t *file_bytes);
int td_gz_shard_decode(td_handle *h, uint64_t stop_bit, uint64_t *end_bit, uint64_t *out_len, int *final, uint16_t *map_out);
int td_gz_shard_resolve(td_handle *h, const uint8_t *window_in, uint64_t member_out_before, void **d_text, uint32_t *crc32);
uint32_t td_crc32_join(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* What the reference's loop over gzip.open(path, 'rt'), left at read number max_reads (:272-273), meets in this
 * file (host only, no GPU): TD_OK -- it ends without an exception -- or TD_E_GZ_EOF / TD_E_GZ_BADFILE /
 * TD_E_GZ_DATA with the exception's message in td_last_error.  td_count_file, td_gunzip_file and td_split_file
 * ask this whenever one of their decoders has refused a file (csrc/gz_pyrules.hpp: Lib/gzip.py restated call for
 * call over the same zlib); a file the reference reads to the bound although it is damaged further on is then
 * counted through that reader.  TD_E_IO: the file cannot be opened. */
int td_gzip_check(const char *path, uint64_t max_reads);

/* Line terminators (\n, \r\n, bare \r) in a device buffer -- what a shard of a
 * byte-split file must know about the shards before it.  Synchronous. */
int td_count_lines_device(td_handle *h, const void *d_fastq, uint64_t nbytes,
                          void *stream, uint64_t *terminators_out);

/* ---- one file over several GPUs (tagdigger_amd/multi.py count_file_sharded; the reference reads a file with one
 * text-mode loop, tagdigger_fun.py:240-250: a rank's byte range, or its range of BGZF members, replaces that loop's
 * input for the rank).  Both bring the bytes into DEVICE memory through the handle's pinned staging pieces -- the host
 * never holds more than two of them -- and return when they have landed. */
/* bytes [offset, offset + length) of `path` -> d_dst[0 .. length) */
int td_load_file_range(td_handle *h, const char *path, uint64_t offset, uint64_t length, void *d_dst);
/* the members of a BGZF file: file offset and inflated size of each (the end-of-file member included); *n_members is
 * the count whatever `capacity` holds.  TD_E_IO when some member is not BGZF. */
int td_bgzf_index(const char *path, uint64_t *member_off, uint32_t *member_isize, uint64_t capacity, uint64_t *n_members);
/* the members that START in [off_begin, off_end) of the file (off_begin must be a member's offset) inflated on the GPU,
 * one after the other, into d_dst[0 .. *nbytes); every member's size and CRC-32 are checked on the device. */
int td_bgzf_inflate_range(td_handle *h, const char *path, uint64_t off_begin, uint64_t off_end, void *d_dst, uint64_t capacity,
                          uint64_t *nbytes_out);

/* ---- barcode splitter (the adapter-trim branch) -----------------------------
 * Replaces the record loop of barcodeSplitter (tagdigger_fun.py:1318-1368) with its per-read
 * decisions -- sequence_index_lookup on barcode+cutsite (:1340) and findAdapterSeq (:1251-1283)
 * -- on the GPU; the host writes the clipped records.
 *
 * td_set_splitter: barcodes[nbar] and the single ACGT cut site (:1292-1293); fullsite0/1 = the two
 * full restriction sites (adapter[k][0] without '^', :1311-1312, at most 8 bases); and, per
 * barcode b, the adapter beginnings to look for at the END of a read, entries
 * ent_begin[b] .. ent_begin[b+1]-1: ent_seq[e] (forward orientation) and ent_slice[e] = the index
 * build_adapter_tree (:1208-1249) pairs with it.  The caller resolves that list with the
 * reference's rules (tagdigger_amd/tagdigger_fun.py does). */
int td_set_splitter(td_handle *h, const char *const *barcodes, uint32_t nbar, const char *cutsite,
                    const char *fullsite0, const char *fullsite1, const uint32_t *ent_begin,
                    const char *const *ent_seq, const int32_t *ent_slice, uint32_t nent);

/* Decisions for a buffer in device memory: d_out[2r], d_out[2r+1] = barcode index (-1: none) and
 * findAdapterSeq's return value (999: nothing to clip) for the buffer's r-th sequence line (lines
 * whose global index first_line + k is 1 mod 4).  out_capacity (in results) must be at least
 * (terminators + 1) / 4 + 2, terminators as td_count_lines_device reports them.
 * Synchronous; *n_terminators (optional) receives the buffer's line terminators. */
int td_split_device(td_handle *h, const void *d_fastq, uint64_t nbytes, uint64_t first_line,
                    int32_t *d_out, uint64_t out_capacity, void *stream, uint64_t *n_terminators);

/* Which kernel the splitter's decisions will come from, for the splitter set last and the option "split_kernel" as it
 * stands: *kernel_out = 2 (k_split2) or 1 (k_split).  k_split2 is asked for by default, and k_split runs all the same
 * when the entries do not fit its compact form (a group of entries that share their last three characters holds more
 * than eight, an entry is longer than 128 characters), a restriction site holds a letter outside ACGT, or the barcode
 * index does not fit beside the tile.  Nothing runs on the device; no decision depends on it (tests: which kernel
 * decided).  TD_E_STATE before td_set_splitter. */
int td_split_kernel_in_use(td_handle *h, int *kernel_out);

/* Both per-read branches over one resident buffer (BASELINE config 5: counting + adapter trim): td_count_device's
 * pass, then td_split_device's, enqueued on the same stream; arguments as theirs.  Synchronous. */
int td_count_and_split_device(td_handle *h, const void *d_fastq, uint64_t nbytes, uint64_t first_line,
                              uint64_t max_reads, int32_t *d_out, uint64_t out_capacity, void *stream,
                              uint64_t *n_terminators);

/* The whole loop on a file (plain or gzip by name, :1318-1321): out_paths[nbar] are created
 * (truncated) and receive the clipped records of their barcode; stops after max_reads records
 * (:1361-1362).  stats = reads, reads with barcode+cut site, reads clipped on the 3' end (:1359). */
int td_split_file(td_handle *h, const char *in_path, const char *const *out_paths,
                  uint64_t max_reads, uint64_t stats[3]);
/* What the splitter's loop prints every 50 000 reads (:1357-1360), for the last td_split_file of this handle:
 * out[2 w] = reads with barcode + cut site, out[2 w + 1] = reads clipped on the 3' end, among the reads of
 * window w (50 000 consecutive reads); *nwindows = ceil(reads / 50 000).  Running sums are the printed numbers. */
int td_split_progress(td_handle *h, uint64_t *out, uint64_t cap, uint64_t *nwindows);

/* ---- expected fragment sizes (the reference's exp_frag_size.py; tagdigger_amd/exp_frag_size.py drives these) -----
 *
 * td_fasta_frame_device: K1, the genome reading of exp_frag_size.py:152-189 over ONE genome file in device memory.
 * The reference reads the file in text mode (universal newlines: \n, \r\n and a lone \r end a line); a line whose first
 * character is '>' is a header (:164), and every other line contributes line.strip().upper() to the sequence (:189).
 * This writes exactly those bytes, concatenated, to d_out[0 .. *n_out) (*n_out <= nbytes) and one row per header line,
 * in file order, to rec_out[3 r .. 3 r + 2]: the input offsets [lo, hi) of the header's name line[1:].strip() (:166)
 * and the number of sequence bytes written before that header (where the record that precedes it ends).
 *   d_text     16-byte aligned, readable up to nbytes rounded up to 16
 *   d_out      any alignment; room for nbytes bytes
 *   rec_cap    rows rec_out can hold (the file's count of '>' bytes always suffices); TD_E_LIMIT if fewer
 *   *n_rec     header lines in the file
 *   *nonascii  1: the file holds a byte >= 0x80, which the reference decodes with the locale's codec -- nothing is written
 *              (*n_out = 0) and the caller reads the file on the host
 *   ms         optional: device time of the three kernels
 * Python's strip() set is ASCII \t \n \v \f \r, 0x1c-0x1f and space; upper() changes a-z only.  Synchronous. */
int td_fasta_frame_device(td_handle *h, const void *d_text, uint64_t nbytes, void *d_out, uint64_t *n_out,
                          uint64_t *rec_out, uint64_t rec_cap, uint64_t *n_rec, int *nonascii, double *ms);

/* One search of exp_frag_size.py:174-194 -- one tag in one record.  [lo, hi) is the window in the device sequence:
 * sequence[pos-1 : pos+3000] forward (:178), sequence[max(0, pos-3000) : pos] reverse (:181-182), both resolved by the
 * caller with Python's slice rules (slice(a, b).indices(len)); `reverse` != 0 searches reverseComplement of the window
 * (tagdigger_fun.py:1203-1206: A, C, G, T complemented, every other byte kept) without materialising it.  tagsize is
 * len(fields[9]) of the tag's SAM line (any value above the window's length + 64 behaves like that bound). */
typedef struct td_frag_job {
    uint64_t lo, hi;
    int32_t tagsize, reverse;
    uint64_t reserved;
} td_frag_job;

enum {
    TD_FRAG_MAX_SITES = 16,       /* non-empty cut sites per search; more: TD_E_LIMIT                         */
    TD_FRAG_MAX_SITE_LEN = 64,    /* bytes per cut site; longer: TD_E_LIMIT                                   */
    TD_FRAG_MAX_WINDOW = 3072     /* hi - lo; the reference's windows hold at most 3 001 bytes                */
};

/* K2: out[4 j .. 4 j + 3] = {size, G + C, N, 0} for jobs[j].  size is min over the sites of subseq.find(cs,
 * tagsize - len(cs)) + len(cs) over the hits (:186-189), -1 for "NA"; G + C and N are counted over subseq[:size]
 * (:192-194; the caller divides).  sites: nsites non-empty strings (an empty cut site needs no search: str.find
 * returns its start, and the caller decides it).  ms optional (device time).  Synchronous. */
int td_frag_search_device(td_handle *h, const void *d_seq, uint64_t seq_bytes, const td_frag_job *jobs, uint64_t njobs,
                          const char *const *sites, uint32_t nsites, int32_t *out, double *ms);

/* K3: subseq[:sizes[j]] of every job (:191), reverse-complemented for reverse jobs, packed in job order into host
 * memory out[0 .. *n_out) (sizes <= 0 contribute nothing); TD_E_LIMIT if that exceeds out_cap.  Synchronous. */
int td_frag_gather_device(td_handle *h, const void *d_seq, uint64_t seq_bytes, const td_frag_job *jobs,
                          const int32_t *sizes, uint64_t njobs, void *out, uint64_t out_cap, uint64_t *n_out, double *ms);

/* ---- Tag Manager (the reference's tag_manager.py; tagdigger_amd/tagdigger_fun.py drives these) --------------------
 *
 * Tags are passed as ASCII bytes seqs[offs[i] .. offs[i + 1]), i < n (offs has n + 1 entries, not decreasing).  The
 * device takes tags of at most TD_TAGSET_MAX_LEN bases: a longer one is TD_E_LIMIT, a byte outside ACGT TD_E_ALPHABET
 * (in both cases nothing is kept and the caller runs its host restatement).  ms (optional) reports device time.
 *
 * td_tagset_load: K1 packs the tags (2 bits per base, A-padded, plus the length), K2 sorts them on the device with a
 * stable LSD radix sort by (sequence, then the position in `order`), and the sorted set stays resident in *out until
 * td_tagset_free.  `order` (NULL: 0 .. n - 1) is the tags sorted by name in code-point order, so perm_out -- the input
 * index of every sorted position -- is the order of Python's sorted(zip(seqs, names)).  passes (optional): the radix
 * passes run (a digit every key shares is skipped).  ms[0] K1, ms[1] K2 (2 entries). */
typedef struct td_tagset td_tagset;
enum {
    TD_TAGSET_MAX_LEN = 256,
    TD_TAGSET_MAX_TAGS = 1 << 30
};
int td_tagset_load(td_handle *h, const char *seqs, const uint64_t *offs, uint32_t n, const uint32_t *order,
                   td_tagset **out, uint32_t *perm_out, uint32_t *passes, double *ms);
int td_tagset_free(td_handle *h, td_tagset *s);

/* K3: for every query tag q (nq of them, same layout), the walk of lookupMarkerByTag (tagdigger_fun.py:1674-1706) in
 * the sorted set, as sorted positions out[4 k .. 4 k + 3] = {f, a, b, c}: f the tag whose marker is added first (-1:
 * nothing found; then a = b = c = -1), a where the forward walk starts, b where it ends, c where the backward walk
 * ends.  The markers are added in the order f, a + 1 .. b, b - 1 down to c.  allow_diff_lengths as the reference's
 * allowDiffLengths.  Each walk costs at most len(q) + 4 binary searches.  Synchronous. */
int td_tagset_lookup(td_handle *h, const td_tagset *s, const char *seqs, const uint64_t *offs, uint32_t nq,
                     int allow_diff_lengths, int32_t *out, double *ms);

/* K4: compareTags (tagdigger_fun.py:376-393) for ngroups groups of tags; group g holds the tags idx[goff[g] ..
 * goff[g + 1]) (goff[0] = 0, no group empty).  mask_out[4 g .. 4 g + 3] gets bit c of column c that compareTags
 * reports (trim != 0: columns below the shortest tag; trim == 0: a column where two tags long enough to reach it
 * differ), nonacgt_out[g] = 1 when a tag of the group holds a byte outside ACGT (compareTags' AssertionError; the
 * group's mask then means nothing).  Synchronous. */
int td_tagset_varsites(td_handle *h, const char *seqs, const uint64_t *offs, uint32_t ntags, const uint32_t *idx,
                       const uint64_t *goff, uint32_t ngroups, int trim, uint64_t *mask_out, uint8_t *nonacgt_out,
                       double *ms);

/* ---- MD5 sums of many messages (writeMD5sums, tagdigger_fun.py:1370-1386; csrc/md5.hip) -----------------------------
 *
 * One lane per message (k_md5_update): a message's 64-byte blocks are one dependent chain, the messages are
 * independent.
 *
 * MD5 (RFC 1321) of n messages that lie whole in device memory: message i is d_data[offs[i] .. offs[i+1]) (offs: host
 * memory, n + 1 entries, not decreasing; any alignment).  digests[16 i .. 16 i + 15] = the digest's bytes in the order
 * hexdigest() prints them.  ms (optional): device time. */
int td_md5_device(td_handle *h, const void *d_data, const uint64_t *offs, uint32_t n, uint8_t *digests, double *ms);

/* The same for n files read from disk, of any size, streamed (writeMD5sums, tagdigger_fun.py:1376-1384): rounds of one
 * piece per unfinished file through two pinned slots, the reading of a round overlapping copy and kernel of the round
 * before.  A piece is 1 MiB (less when that would make a round exceed 384 MiB; option "md5_piece" sets it for tests).
 * TD_E_IO names the first file (lowest index) that cannot be opened or read; *bad_index (optional) receives it.
 * ms (optional): [0] reading into the slots, [1] waiting for the GPU, [2] kernel time. */
int td_md5_files(td_handle *h, const char *const *paths, uint32_t n, uint8_t *digests, uint32_t *bad_index, double ms[3]);

/* ---- tag census (csrc/census.hip; tagdigger_amd/tagdigger_fun.py tag_census drives these) ---------------------------
 *
 * Which sequences follow the barcodes of a library, and how often: for every read with a barcode + cut site (the
 * counter's rule, tagdigger_fun.py:250-259) the window line1[len(barcode) : len(barcode) + taglen] -- from the cut
 * site's first base on -- is counted in a table in device memory.  A window the line is too short for counts as
 * `short`, one that holds anything but ACGT as `ambiguous`.  Census state is independent of the count index
 * (td_set_index): one handle can hold both.
 *
 * td_census_begin: the barcode + cut-site index by td_set_index's rules, from the same list (barcut[n_barcut], entry k
 *   belongs to barcode k % barnum; TD_E_OVERLAP / TD_E_EMPTY / TD_E_ROOTLEAF / TD_E_ALPHABET / TD_E_LIMIT and
 *   td_last_bad_index as there); baroff[barnum] = len(barcode), at most 32; taglen 1 .. TD_CENSUS_MAX_TAGLEN.  The table
 *   gets `slots` slots (a power of two, 1024 .. 2^32; 0: 2^22) of 16 bytes (taglen <= 32) or 32 bytes, zeroed, and takes
 *   3/4 of them in distinct windows.  A census begun before is dropped.
 * td_census_device: one pass over a resident buffer (arguments as td_count_device's).  Asynchronous, accumulates; ONE
 *   stream in flight per handle.  What a kernel flags is reported by the calls below.
 * td_census_file: a whole file, plain, gzip or BGZF, through td_count_file's readers.  Synchronous, accumulates.
 * td_census_stats: out[TD_CENSUS_*], cumulative since td_census_begin.  Synchronises.
 * td_census_fetch: the windows with count >= min_count (0 counts as 1), ordered by count descending, then sequence
 *   ascending (A < C < G < T): window k as taglen characters at seqs_out[k * taglen] (no terminator) and its count in
 *   counts_out[k], for k < capacity; *n_out = how many there are, whatever capacity holds.  Synchronises.
 * td_census_end: frees the census.
 * Errors: TD_E_NONASCII as the counter's; TD_E_LIMIT when the table is full (the message names slots and the keys
 *   placed); TD_E_INTERNAL when a bounded wait ran out.  After any of them, and after a td_census_file that failed
 *   part-way, every call answers with that error until td_census_begin: a partly right census is never handed out. */
enum {
    TD_CENSUS_READS = 0,      /* read lines looked at (readscount of :255)                              */
    TD_CENSUS_BARCUT = 1,     /* ... with barcode + cut site: TD_STAT_BARCUT of a count pass            */
    TD_CENSUS_SHORT = 2,      /* ... whose line ends inside the window                                  */
    TD_CENSUS_AMBIGUOUS = 3,  /* ... whose window holds a character outside ACGT                        */
    TD_CENSUS_COUNTED = 4,    /* barcut - short - ambiguous                                             */
    TD_CENSUS_DISTINCT = 5,   /* distinct windows in the table                                          */
    TD_CENSUS_SLOTS = 6,      /* the table's slots                                                      */
    TD_CENSUS_MAX_KEYS = 7,   /* distinct windows it takes                                              */
    TD_CENSUS_MAX_TAGLEN = 64
};
int td_census_begin(td_handle *h, const char *const *barcut, uint32_t n_barcut, uint32_t barnum, const uint32_t *baroff,
                    uint32_t taglen, uint64_t slots);
int td_census_device(td_handle *h, const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, void *stream);
int td_census_file(td_handle *h, const char *path, uint64_t max_reads);
int td_census_stats(td_handle *h, uint64_t out[8]);
int td_census_fetch(td_handle *h, uint64_t min_count, char *seqs_out, uint64_t *counts_out, uint64_t capacity, uint64_t *n_out);
int td_census_end(td_handle *h);

/* ---- library QC (csrc/qc.hip; tagdigger_amd/tagdigger_fun.py library_qc drives these) ----------------------------------
 *
 * The first questions about a sequenced library, in one pass over all bytes of its sequence and quality lines
 * (DESIGN.md 4.19): reads, bases and reads with a non-ACGT character per barcode; base composition, quality values and
 * read lengths per cycle; the reads' mean quality.  Lines are the counter's; record r is lines 4r .. 4r + 3; records
 * r >= max_reads are not looked at; every line is decided on its own.  C = max_cycles; row C of a per-cycle table is
 * the overflow row for positions >= C.  Every counter is a uint64_t.
 *
 * td_qc_begin: the barcode + cut-site index as td_census_begin builds it (same list, same errors, baroff[barnum] =
 *   len(barcode), at most 32); max_cycles 1 .. TD_QC_MAX_CYCLES.  Zeroed tables; a QC begun before is dropped.
 * td_qc_device: one pass over a resident buffer whose first line has index first_line (it may start inside a record).
 *   Asynchronous, accumulates; ONE stream in flight per handle.
 * td_qc_file: a whole file, plain, gzip or BGZF, through td_count_file's readers, which are asked for one record more
 *   than max_reads so that the last record's quality line arrives.  Synchronous, accumulates.
 * td_qc_stats: out[TD_QC_*], cumulative since td_qc_begin.  Synchronises.
 * td_qc_fetch: the tables, each pointer may be NULL:
 *     barcode_out     [(B + 1) * 3]   row b: reads, bases, reads with a non-ACGT character; row B: no barcode + cut site
 *     base_cycle_out  [(C + 1) * 6]   row min(i, C): A, C, G, T, N, anything else
 *     qual_cycle_out  [(C + 1) * 95]  row min(i, C): byte values 33 .. 126 as 0 .. 93, column 94: any other byte
 *     length_out      [C + 1]         reads of length min(n, C)
 *     meanq_out       [94]            quality lines by floor(sum / count) of their valid values
 * td_qc_end: frees the QC.
 * Options (td_set_option): "qc_flush_tiles", the tiles after which a workgroup merges its LDS tables into device
 *   memory (0: the built-in 4096; at most 2^20); "max_grid" caps the grid.  Every setting gives the same result.
 * Errors: TD_E_NONASCII as the counter's.  After it, and after a td_qc_file that failed part-way, every call answers
 *   with that error until td_qc_begin. */
enum {
    TD_QC_READS = 0,          /* sequence lines looked at                                               */
    TD_QC_BARCUT = 1,         /* ... with barcode + cut site                                            */
    TD_QC_QUAL_LINES = 2,     /* quality lines looked at                                                */
    TD_QC_BASES = 3,          /* characters of the stripped sequence lines                              */
    TD_QC_QUAL_BASES = 4,     /* bytes 33 .. 126 of the stripped quality lines                          */
    TD_QC_QUAL_INVALID = 5,   /* their other bytes                                                      */
    TD_QC_EMPTY_QUAL = 6,     /* quality lines without a valid byte                                     */
    TD_QC_CYCLES = 7,         /* max_cycles of td_qc_begin                                              */
    TD_QC_MAX_CYCLES = 1024
};
int td_qc_begin(td_handle *h, const char *const *barcut, uint32_t n_barcut, uint32_t barnum, const uint32_t *baroff, uint32_t max_cycles);
int td_qc_device(td_handle *h, const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, void *stream);
int td_qc_file(td_handle *h, const char *path, uint64_t max_reads);
int td_qc_stats(td_handle *h, uint64_t out[8]);
int td_qc_fetch(td_handle *h, uint64_t *barcode_out, uint64_t *base_cycle_out, uint64_t *qual_cycle_out, uint64_t *length_out, uint64_t *meanq_out);
int td_qc_end(td_handle *h);

/* ---- tag rescue (csrc/rescue.hip; tagdigger_amd/tagdigger_fun.py rescue_tags_fastq drives these) ------------------------
 *
 * The reads the counter drops because they lie one or two substitutions from a known tag, per barcode and per tag
 * (DESIGN.md 4.21).  Per read the rule is the counter's up to the barcode + cut site; then w = the stripped, upper-cased
 * line from tagoff[b] on and avail = len(w).  A tag of n bases is a candidate iff n <= avail; its distance is the number
 * of positions i < n with w[i] != tag[i], a character of w outside ACGT mismatching every base.  A candidate at distance
 * 0: the read is `exact` and nothing is written (it is the counter's).  Otherwise, with m the smallest distance of a
 * candidate: m <= max_mismatch and one tag attains it -> rescued[b][tag] += 1, rescued_at[m] += 1 and positions[i] += 1
 * for every mismatching i; m <= max_mismatch and several attain it -> `ambiguous`; else `none`.  So
 * barcut == exact + rescued1 + rescued2 + ambiguous + none.  Rescue state is independent of the count index and of a
 * census or QC on the same handle.
 *
 * td_rescue_begin: barcut[n_barcut], barnum and tagoff[barnum] (at most 63) as td_set_index takes them, with its errors;
 *   tags[n_tags] as stored: 1 .. TD_RESCUE_MAX_TAGLEN upper-case ACGT (TD_E_EMPTY / TD_E_LIMIT / TD_E_ALPHABET, the
 *   tag in td_last_bad_index), none equal to or a prefix of another (TD_E_OVERLAP; of all such pairs the one whose
 *   later tag comes first, that tag in td_last_bad_index); max_mismatch 1 or 2.  The index: max_mismatch + 1 parts of
 *   P = min(32, shortest tag / (max_mismatch + 1)) bases at positions [pP, (p + 1)P) of every tag, per part the tags
 *   sorted by those bases under a hash directory.  TD_E_LIMIT with a message that begins "tag rescue: run" when P < 1 or
 *   when more tags share one part than the option "rescue_max_run" allows (td_set_option; 0: the built-in 4096).  The
 *   matrix and the counters start at zero.  A rescue begun before is dropped.
 * td_rescue_device: one pass over a resident buffer (arguments as td_count_device's).  Asynchronous, accumulates; ONE
 *   stream in flight per handle.  "max_grid" caps the grid.
 * td_rescue_file: a whole file, plain, gzip or BGZF, through td_count_file's readers.  Synchronous, accumulates.
 * td_rescue_stats: out[TD_RESCUE_*], cumulative since td_rescue_begin.  Synchronises.
 * td_rescue_work: what the passes cost: out[0] directory probes, out[1] tags verified, out[2] P, out[3] the longest
 *   displacement in a directory.  Synchronises.
 * td_rescue_fetch: rescued_out[barnum * n_tags] (uint32_t, row b column t) and positions_out[128]; each may be NULL.
 *   Synchronises.
 * td_rescue_matrix: the matrix where it lies in device memory, for callers that add it to a count matrix there; good
 *   until td_rescue_end or the next td_rescue_begin.
 * td_rescue_end: frees the rescue; TD_E_STATE without one.  td_destroy frees a rescue left open.
 * Errors: TD_E_NONASCII as the counter's.  After it, and after a td_rescue_file that failed part-way, every call answers
 *   with that error until td_rescue_begin. */
enum {
    TD_RESCUE_READS = 0,        /* read lines looked at                                                   */
    TD_RESCUE_BARCUT = 1,       /* ... with barcode + cut site                                            */
    TD_RESCUE_EXACT = 2,        /* ... that equal a tag: the counter's                                    */
    TD_RESCUE_RESCUED1 = 3,     /* ... one mismatch from exactly one nearest tag                          */
    TD_RESCUE_RESCUED2 = 4,     /* ... two mismatches from exactly one nearest tag                        */
    TD_RESCUE_AMBIGUOUS = 5,    /* ... whose smallest distance several tags attain                        */
    TD_RESCUE_NONE = 6,         /* ... with no tag within max_mismatch                                    */
    TD_RESCUE_LONGEST_RUN = 7,  /* tags that share one part, at most (known at begin)                     */
    TD_RESCUE_MAX_TAGLEN = 128
};
int td_rescue_begin(td_handle *h, const char *const *barcut, uint32_t n_barcut, uint32_t barnum, const uint32_t *tagoff,
                    const char *const *tags, uint32_t n_tags, uint32_t max_mismatch);
int td_rescue_device(td_handle *h, const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, void *stream);
int td_rescue_file(td_handle *h, const char *path, uint64_t max_reads);
int td_rescue_stats(td_handle *h, uint64_t out[8]);
int td_rescue_work(td_handle *h, uint64_t out[4]);
int td_rescue_fetch(td_handle *h, uint32_t *rescued_out, uint64_t *positions_out);
int td_rescue_matrix(td_handle *h, void **d_matrix);
int td_rescue_end(td_handle *h);

/* ---- barcode rescue (csrc/bcrescue.hip; tagdigger_amd/tagdigger_fun.py rescue_barcodes_fastq drives these) --------------
 *
 * The reads every other pass drops because their first bases are no stored barcode + cut site entry, brought back when
 * they lie one or two substitutions from the entries of exactly one barcode.  The entries are the
 * strings the index build leaves (of duplicates the first; an entry that extends an earlier one is shadowed); entry k of
 * the list belongs to row k % barnum.  Per read line (stripped, upper-cased), reads += 1, then:
 *   1  an entry is an exact prefix of the read (the counter's lookup): exact += 1, nothing else -- the read is the
 *      counter's;
 *   2  else every entry e of L_e <= len(read) bases is a candidate at d(e) = the positions i < L_e with read[i] != e[i],
 *      a character outside ACGT mismatching every base; m = the smallest d (m >= 1);
 *   3  m > max_mismatch, or no candidate: none += 1;
 *   4  the entries at distance m belong to more than one row: ambiguous += 1.  Cut-site variants of one row that tie are
 *      no tie: the earliest of them in the list is "the entry";
 *   5  else the read is rescued into that row b: rescued<m> += 1, row_rescued[b][m - 1] += 1, positions[i] += 1 for
 *      every mismatching i of the entry, and the counter's tag step: the one stored tag that is a prefix of the read from
 *      tagoff[b] on, all of its characters in ACGT, gives matrix[b][tag] += 1 and tagged += 1.
 * So reads == exact + rescued1 + rescued2 + ambiguous + none.  The state is independent of the count index and of a
 * census, a QC or a tag rescue on the same handle.
 *
 * td_bcrescue_begin: barcut[n_barcut], barnum and tagoff[barnum] (at most 63) as td_set_index takes them, with its
 *   errors; tags[n_tags] under td_rescue_begin's conditions, with its errors and td_last_bad_index; max_mismatch 1 or 2.
 *   Every surviving entry must be longer than 2 * max_mismatch bases: else TD_E_LIMIT with a message that begins
 *   "barcode rescue: entry" (the row in td_last_bad_index).  TD_E_LIMIT too when the index and the entry list -- 16-byte
 *   rounded (8 ne + 8-byte rounded (4 ne) + 2048) + 2 n bytes for n distinct entries in ne directory slots, ne == n when
 *   no entry is shorter than 5 bases -- exceed 40 KiB of a workgroup's LDS.  The matrix and the counters start at zero.
 *   A barcode rescue begun before is dropped.
 * td_bcrescue_device: one pass over a resident buffer (arguments as td_count_device's).  Asynchronous, accumulates; ONE
 *   stream in flight per handle.  "max_grid" caps the grid.
 * td_bcrescue_file: a whole file, plain, gzip or BGZF, through td_count_file's readers.  Synchronous, accumulates.
 * td_bcrescue_stats: out[TD_BCRESCUE_*], cumulative since td_bcrescue_begin.  Synchronises.
 * td_bcrescue_fetch: matrix_out[barnum * n_tags] (uint32_t, row b column t), row_rescued_out[barnum * 2] and
 *   positions_out[32]; each may be NULL.  Synchronises.
 * td_bcrescue_matrix: the matrix where it lies in device memory, for callers that add it to a count matrix there; good
 *   until td_bcrescue_end or the next td_bcrescue_begin.
 * td_bcrescue_end: frees the state; TD_E_STATE without one.  td_destroy frees a state left open.
 * Errors: TD_E_NONASCII as the counter's.  After it, and after a td_bcrescue_file that failed part-way, every call
 *   answers with that error until td_bcrescue_begin. */
enum {
    TD_BCRESCUE_READS = 0,               /* read lines looked at                                                  */
    TD_BCRESCUE_EXACT = 1,               /* ... that begin with an entry: the counter's                           */
    TD_BCRESCUE_RESCUED1 = 2,            /* ... one mismatch from the entries of exactly one row                  */
    TD_BCRESCUE_RESCUED2 = 3,            /* ... two mismatches from the entries of exactly one row                */
    TD_BCRESCUE_AMBIGUOUS = 4,           /* ... whose smallest distance entries of several rows attain            */
    TD_BCRESCUE_NONE = 5,                /* ... with no entry within max_mismatch                                 */
    TD_BCRESCUE_TAGGED = 6,              /* rescued reads that carry a stored tag: the sum of the matrix          */
    TD_BCRESCUE_MIN_ENTRY_DISTANCE = 7,  /* the smallest distance between two entries of different rows, over the
                                            shorter one's length (known at begin; 64 without two rows): at or below
                                            max_mismatch, exact reads of one sample lie one error from another     */
    TD_BCRESCUE_POSITIONS = 32
};
int td_bcrescue_begin(td_handle *h, const char *const *barcut, uint32_t n_barcut, uint32_t barnum, const uint32_t *tagoff,
                      const char *const *tags, uint32_t n_tags, uint32_t max_mismatch);
int td_bcrescue_device(td_handle *h, const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, void *stream);
int td_bcrescue_file(td_handle *h, const char *path, uint64_t max_reads);
int td_bcrescue_stats(td_handle *h, uint64_t out[8]);
int td_bcrescue_fetch(td_handle *h, uint32_t *matrix_out, uint64_t *row_rescued_out, uint64_t *positions_out);
int td_bcrescue_matrix(td_handle *h, void **d_matrix);
int td_bcrescue_end(td_handle *h);

/* ---- tag network (csrc/tagnet.hip; tagdigger_amd/tagdigger_fun.py tag_network and census_markers drive these) --------
 *
 * From a census to markers without a reference genome (the UNEAK network filter).  Input: n tags of one
 * length taglen (1 .. TD_TAGNET_MAX_TAGLEN), upper-case ACGT, pairwise distinct, as n * taglen ASCII bytes in
 * td_census_fetch's layout, and their counts.  The rule, in integers only:
 *   edge       an unordered pair i < j whose sequences differ at exactly one position (no indels, no distance 2)
 *   kept edge  min(c_i, c_j) * 1 000 000 >= ratio_ppm * max(c_i, c_j), exact as a 128-bit product
 *   degree     kept edges at a tag
 *   pair       a kept edge whose two ends both have degree 1
 * Edges and pairs are delivered ascending by (i, j).  A tag has at most 3 * taglen neighbours, so there are at most
 * 3 * taglen * n / 2 edges; nothing is ever sized by n^2.
 *
 * td_tagnet_build: packs, sorts twice, compares inside the runs and selects (the kernels are described in tagnet.hip);
 *   the result stays in *out until td_tagnet_free.  stats[TD_TAGNET_*] (optional).  `compares` is the number of tag
 *   comparisons the device makes: the sum of len * (len - 1) / 2 over the runs of both sorted orders, known before any
 *   comparing.  ms (optional, 6 entries): device time of K1 pack, K2 the two sorts, K3 run boundaries, K4 compare,
 *   K5 select, and the host's time for copying and ordering the results.  n = 0 and n = 1 give empty results.
 *   Errors: TD_E_ARG (taglen outside 1..64, ratio_ppm > 1 000 000), TD_E_ALPHABET (a byte outside ACGT;
 *   td_last_bad_index gives the tag), TD_E_OVERLAP (two equal tags; td_last_bad_index gives the later one),
 *   TD_E_LIMIT (more than 2^30 tags; or compares above the cap -- the message names both numbers, stats[0] and
 *   stats[TD_TAGNET_COMPARES] are set, and no comparing kernel has been launched).  The cap is
 *   TD_TAGNET_DEFAULT_MAX_COMPARES unless the option "tagnet_max_compares" sets another.
 * td_tagnet_edges / td_tagnet_pairs: ij_out[2 k], ij_out[2 k + 1] = i, j of entry k < capacity; *n_out = how many
 *   there are, whatever capacity holds.  kept_only != 0 leaves the cut edges out.
 * td_tagnet_degrees: deg_out[n]. */
typedef struct td_tagnet td_tagnet;
enum {
    TD_TAGNET_TAGS = 0,       /* n                                                                        */
    TD_TAGNET_EDGES = 1,      /* pairs of tags at distance 1                                              */
    TD_TAGNET_KEPT = 2,       /* ... that pass the ratio                                                  */
    TD_TAGNET_DEG0 = 3,       /* tags without a kept edge                                                 */
    TD_TAGNET_DEG1 = 4,       /* tags with exactly one                                                    */
    TD_TAGNET_HUBS = 5,       /* tags with two or more                                                    */
    TD_TAGNET_PAIRS = 6,      /* kept edges between two tags of degree 1                                  */
    TD_TAGNET_COMPARES = 7,   /* tag comparisons of the device path                                       */
    TD_TAGNET_MAX_TAGLEN = 64,
    TD_TAGNET_TILE = 256      /* rows and columns of a compare tile: a run longer than this spans several */
};
/* K4 at this many compares runs for about 2 s on an MI355X (NOT YET measured: see DESIGN.md 4.13) */
#define TD_TAGNET_DEFAULT_MAX_COMPARES 2000000000000ull
int td_tagnet_build(td_handle *h, const char *seqs, const uint64_t *counts, uint32_t n, uint32_t taglen, uint32_t ratio_ppm,
                    td_tagnet **out, uint64_t stats[8], double *ms);
int td_tagnet_edges(td_handle *h, const td_tagnet *net, int kept_only, uint32_t *ij_out, uint64_t capacity, uint64_t *n_out);
int td_tagnet_pairs(td_handle *h, const td_tagnet *net, uint32_t *ij_out, uint64_t capacity, uint64_t *n_out);
int td_tagnet_degrees(td_handle *h, const td_tagnet *net, uint32_t *deg_out);
int td_tagnet_free(td_handle *h, td_tagnet *net);

/* ---- tag placement (csrc/place.hip; tagdigger_amd/tagdigger_fun.py genome_cut_sites and place_tags drive these) -------
 *
 * Where on a genome the tags of a census come from.  A GBS tag begins at a cut site, so the only
 * places it can come from are the genome's cut sites: an in-silico digest, the window behind every site, and a bounded
 * Hamming join of the tags against those windows.  The rule, in integers only:
 *   genome     the bytes td_fasta_frame_device writes, d_seq[0 .. seq_bytes); record r = 0 .. R - 1 is
 *              [rec_start[r], rec_start[r + 1]), rec_start[0] = 0, rec_start[R] = seq_bytes, non-decreasing
 *   remnants   1 .. TD_PLACE_MAX_SITES non-empty ACGT strings no longer than taglen (what follows the barcode in a read)
 *   forward locus (r, x)   rec_start[r] <= x, x + L <= rec_start[r + 1], every byte of G[x, x + L) is one of ACGT, and
 *              G[x ...] begins with a remnant.  Window G[x, x + L); SAM position x - rec_start[r] + 1 = cut position
 *   reverse locus (r, x)   the same bounds and alphabet; reverseComplement(G[x, x + L)) begins with a remnant.  Window:
 *              that reverse complement; SAM position as above; cut position = SAM position + L - 1
 *   order      loci ascend by (r, x, strand), forward before reverse; a locus's id is its rank
 *   dropped    a remnant met on a strand whose window leaves its record (the record of the window's first base on the
 *              forward strand, of its last base on the reverse strand) or holds a byte outside ACGT is no locus and is
 *              counted; several remnants at one (x, strand) are one hit
 *   n_at[t][d] the loci whose window differs from tag t at exactly d positions, d = 0 .. k (plain Hamming distance over
 *              all L bases; loci are counted, not distinct windows)
 *   dist[t]    the smallest d with n_at[t][d] > 0, or 255; locus[t] the smallest locus id at that distance, or UINT64_MAX
 *   compares   the L bases are cut into P = k + 1 parts, part p = bases [floor(p L / P), floor((p + 1) L / P)); two
 *              sequences within distance k agree on at least one part; compares = sum over p and t of the DISTINCT
 *              windows that agree with tag t on all of part p.  A pair is reported in the lowest part it agrees on.
 * Nothing is ever sized by tags x loci.
 *
 * td_place_sites: the digest (count, scan, emit: loci come out in order without a sort), then the windows sorted and
 *   equal ones collapsed to (window, multiplicity, first locus id).  The result stays in *out until td_place_free or
 *   td_destroy: the handle owns it.  stats[TD_PLACE_*] (optional); ms (optional, 4 entries): device time of count, scan,
 *   emit, dedupe -- events around the launches only, every buffer allocated before; the radix sort inside dedupe (and
 *   inside td_place_tags' parts) reads 12 bytes back before its passes, which those two figures include.  seq_bytes = 0 gives an empty place without a launch.  Errors: TD_E_ARG (taglen outside 1..64, no or
 *   more than 16 remnants, a remnant empty, longer than taglen or outside ACGT, rec_start not as above), TD_E_LIMIT (more
 *   than TD_PLACE_MAX_LOCI loci, or 2^31 records and more).
 * td_place_loci: x_out[n] (offset in the genome), rec_out[n], strand_out[n] (0 forward, 1 reverse), and, unless NULL,
 *   windows_out[n * L] as ASCII; n = stats[TD_PLACE_LOCI].  Each pointer may be NULL.
 * td_place_tags: n tags of the place's L bases, upper-case ACGT, n * L ASCII bytes; equal tags are allowed, every tag
 *   is decided on its own.  n_at_out[4 n] (entries d > k are 0), dist_out[n], locus_out[n]; stats[TD_PLACED_*]
 *   (optional); ms (optional, 4 entries): device time of pack, the parts' sorted window tables (0 when this place has
 *   them for this k already), runs, join.  Zero tags or zero loci give all-none results without a launch.  Errors:
 *   TD_E_ARG (k > 3, L < k + 1), TD_E_ALPHABET (td_last_bad_index gives the tag), TD_E_LIMIT (more than 2^30 tags; or
 *   compares above the cap -- the message names both numbers, stats[TD_PLACED_TAGS] and stats[TD_PLACED_COMPARES] are
 *   set, and no comparing kernel has been launched).  The cap is TD_PLACE_DEFAULT_MAX_COMPARES unless the option
 *   "place_max_compares" sets another.
 * td_place_free: frees a place now. */
typedef struct td_place td_place;
enum {
    TD_PLACE_LOCI = 0,          /* loci                                                                     */
    TD_PLACE_FORWARD = 1,       /* ... on the forward strand                                                */
    TD_PLACE_REVERSE = 2,       /* ... on the reverse strand                                                */
    TD_PLACE_DISTINCT = 3,      /* distinct windows                                                         */
    TD_PLACE_DROP_BOUNDS = 4,   /* remnant hits whose window leaves its record                              */
    TD_PLACE_DROP_ALPHABET = 5, /* remnant hits whose window holds a byte outside ACGT                      */
    TD_PLACE_RECORDS = 6,       /* R                                                                        */
    TD_PLACED_TAGS = 0,         /* n                                                                        */
    TD_PLACED_UNIQUE = 1,       /* tags with exactly one locus at their smallest distance                   */
    TD_PLACED_MULTI = 2,        /* ... with more than one                                                   */
    TD_PLACED_NONE = 3,         /* ... with no locus within k                                               */
    TD_PLACED_COMPARES = 4,     /* tag x distinct window comparisons of the device path                     */
    TD_PLACE_MAX_TAGLEN = 64,
    TD_PLACE_MAX_SITES = 16,
    TD_PLACE_MAX_MISMATCH = 3
};
/* A 4-base degenerate site (CWGC) has about 2 * 2 * 3e9 / 256 = 4.7e7 loci in 3 GB; 2^27 leaves room for a genome three
 * times as dense.  A locus costs 28 bytes (x, record, window) and 10 more while the place is built, a distinct window
 * 24, and every part of a k 40 bytes per distinct window: under 30 GB at the limit with k = 3. */
#define TD_PLACE_MAX_LOCI (1u << 27)
/* k_pl_join on long runs (200 000 windows sharing a part, 7.1e9 compares): 6.56e11 compares / s on an MI355X
 * (profiles/place/bench_mi355x.txt); times 2 s, so that the kernel stays near two seconds on a shared card */
#define TD_PLACE_DEFAULT_MAX_COMPARES 1300000000000ull
int td_place_sites(td_handle *h, const void *d_seq, uint64_t seq_bytes, const uint64_t *rec_start /* HOST, R + 1 */, uint32_t R,
                   const char *const *remnants, uint32_t n_remnants, uint32_t taglen, td_place **out, uint64_t stats[8], double *ms);
int td_place_loci(td_handle *h, const td_place *pl, uint64_t *x_out, uint32_t *rec_out, uint8_t *strand_out, char *windows_out);
int td_place_tags(td_handle *h, td_place *pl, const char *seqs, uint32_t n, uint32_t max_mismatch, uint32_t *n_at_out,
                  uint8_t *dist_out, uint64_t *locus_out, uint64_t stats[8], double *ms);
int td_place_free(td_handle *h, td_place *pl);

/* ---- genotype calls and marker filters (csrc/genocall.hip; tagdigger_amd/tagdigger_fun.py call_genotypes drives it) --
 *
 * From the samples x tags count matrix to genotype calls, without bringing the matrix to the host.
 * d_counts is S x T uint32, row-major, in DEVICE memory: a handle's bound or internal matrix, the destination of
 * td_fold_rows, or any td_dev_alloc buffer.  Marker m is the pair of columns (i0[m], i1[m]) -- HOST arrays, both < T and
 * different; no order or adjacency is assumed.  The rule, in integers only, with a = counts[s][i0[m]],
 * b = counts[s][i1[m]], n = a + b (64-bit):
 *   TD_GENO_MISSING (3)  n < min_depth
 *   TD_GENO_PRESENCE     1 when a > 0 and b > 0, else 0 when a > 0, else 2 (with min_depth 1: writeDiploidGeno's table,
 *                        tagdigger_fun.py:1144-1180)
 *   TD_GENO_LIKELIHOOD   n > 127: a' = floor(127 a / n), b' = floor(127 b / n), n' = a' + b'; else the values themselves.
 *                        1 when min(a', b') >= het_min[n'], else 0 when a' >= b', else 2
 * The code is the number of allele-1 copies.  het_min[TD_GENO_TABLE] is DATA from the caller: het_min[n] = the smallest
 * k in 0 .. n / 2 with (1/2)^n > (1 - e)^(n - k) e^k for e = err_ppm / 10^6 as an exact rational, n + 1 when there is
 * none, het_min[0] = 1 (tagdigger_fun.het_threshold_table); the library evaluates no power and no logarithm, it checks
 * het_min[n] <= n + 1 only.
 * Per marker, stats_out[TD_GENO_NSTATS m + TD_GENO_*]: exact integers; depth0 / depth1 sum a and b over EVERY sample,
 * missing ones included.  Marker m passes (pass_out[m] = 1) when
 *   called * 10^6 >= min_call_ppm * S,  min(alt, 2 called - alt) * 10^6 >= min_maf_ppm * 2 called,
 *   n1 * 10^6 <= max_het_ppm * called
 * -- a marker nobody was called at passes only with min_call_ppm = 0.  *passed_out = the markers that pass.
 * calls_out (optional, host, S x M bytes, row-major) receives the codes; d_calls_out (optional) receives the DEVICE
 * buffer the kernel wrote them to, which is then the caller's (td_dev_free): a caller that wants the statistics and
 * the mask only passes calls_out = NULL.  ms (optional): device time of the two kernels.
 * Synchronous; waits for the work enqueued through this handle first.  M = 0 is answered without a launch; so is S = 0
 * (zero statistics, nothing passes).  TD_E_ARG: a parameter outside its range (rule 0 | 1, err_ppm 1 .. 499 999,
 * min_depth >= 1, min_call_ppm and max_het_ppm 0 .. 10^6, min_maf_ppm 0 .. 500 000), a table entry above n + 1, or a
 * marker whose columns are not both below T or are equal: td_last_bad_index gives the marker. */
typedef struct td_geno_params {
    uint32_t rule;            /* TD_GENO_LIKELIHOOD | TD_GENO_PRESENCE                                    */
    uint32_t err_ppm;         /* the error rate het_min was built for                                     */
    uint64_t min_depth;       /* a + b below this: missing                                                */
    uint32_t min_call_ppm;    /* marker filter: called / S                                                */
    uint32_t min_maf_ppm;     /* marker filter: minor allele frequency among the called                   */
    uint32_t max_het_ppm;     /* marker filter: heterozygous calls among the called; 10^6: off            */
    uint32_t reserved;
} td_geno_params;
enum {
    TD_GENO_LIKELIHOOD = 0,
    TD_GENO_PRESENCE = 1,
    TD_GENO_MISSING = 3,      /* the code of a cell below min_depth                                       */
    TD_GENO_CALLED = 0,       /* stats: n0 + n1 + n2                                                      */
    TD_GENO_N0 = 1,           /* calls by code                                                            */
    TD_GENO_N1 = 2,
    TD_GENO_N2 = 3,
    TD_GENO_ALT = 4,          /* n1 + 2 n2: copies of allele 1                                            */
    TD_GENO_DEPTH0 = 5,       /* sum of a                                                                 */
    TD_GENO_DEPTH1 = 6,       /* sum of b                                                                 */
    TD_GENO_NSTATS = 7,
    TD_GENO_TABLE = 128,      /* entries of het_min; deeper cells are scaled to 127                       */
    TD_GENO_CHUNK = 64        /* sample rows per workgroup of the call kernel (a choice, not yet measured) */
};
int td_geno_call(td_handle *h, const void *d_counts, uint32_t S, uint32_t T, uint32_t M, const uint32_t *i0,
                 const uint32_t *i1, const uint16_t *het_min, const td_geno_params *p, uint8_t *calls_out,
                 void **d_calls_out, uint64_t *stats_out, uint8_t *pass_out, uint64_t *passed_out, double *ms);

/* ---- polyploid allele dosage calls (csrc/dosage.hip; tagdigger_amd/tagdigger_fun.py call_dosage drives it) -----------
 *
 * From the samples x tags count matrix to the allele dosage 0 .. P of every cell, for one ploidy P of all samples
 * (DESIGN.md 4.23).  d_counts, S, T, M, i0, i1 as for td_geno_call: the matrix in DEVICE memory, the markers as pairs of
 * columns in HOST arrays, both < T and different.  The rule, in integers only.  The caller hands in three tables of
 * costs as DATA, cost(x) = round_half_even(-65536 log2 x) for a probability x (tagdigger_fun.dosage_tables builds them;
 * the library evaluates no logarithm and checks only that no entry exceeds TD_DOSE_COST_MAX):
 *   ca[0 .. P]      cost of a read of allele 1 from a cell of dosage d: p_d = (d (1 - e) + (P - d) e) / P
 *   cb[0 .. P]      cost of a read of allele 0: 1 - p_d
 *   cp[TD_DOSE_BINS][P + 1]   cost of dosage d under the prior C(P, d) q^d (1 - q)^(P - d), q = (2 k + 1) / (2 TD_DOSE_BINS)
 *                   the centre of bin k; read with TD_DOSE_HWE only (TD_DOSE_FLAT: may be NULL, every prior cost is 0)
 * Per marker: depth0 / depth1 = the uint64 sums of a and b over EVERY sample, tot = depth0 + depth1,
 *   bin = 0 when tot == 0, else min(TD_DOSE_BINS - 1, floor(TD_DOSE_BINS depth1 / tot))      (reported under both priors)
 * Per cell, a = counts[s][i0[m]], b = counts[s][i1[m]], n = a + b (64-bit):
 *   TD_DOSE_MISSING (255)   n < min_depth
 *   c[d] = b ca[d] + a cb[d] + cp[bin][d]  (uint64; below 2^57), d = 0 .. P      (b counts the reads of allele 1)
 *   best = the smallest d with minimal c[d]; second = the minimal c[d] over d != best
 *   the call is best when second - c[best] >= min_margin, else TD_DOSE_MISSING
 * so a tie gives the lower dosage at min_margin 0 and is missing at any min_margin >= 1.  The code is the number of
 * allele-1 copies.  The diploidised code of a cell is 0 for dosage 0, 2 for dosage P, 1 for everything between and
 * TD_GENO_MISSING (3) for a missing cell: what td_relate_joint, td_ld_pairs, td_impute_knn and td_parent_trios read.
 * stats_out[TD_DOSE_NSTATS m + TD_DOSE_*]: exact integers; the classes above P are 0.  Marker m passes when
 *   called * 10^6 >= min_call_ppm * S,  min(alt, P called - alt) * 10^6 >= min_maf_ppm * P * called
 * Outputs as for td_geno_call, each optional except passed_out, and stats_out / pass_out when M > 0: calls_out and
 * diploid_out (HOST, S * M bytes), d_calls_out and d_diploid_out (the DEVICE buffers, the caller's to td_dev_free; NULL
 * is stored when nothing was launched), ms (HIP events around the kernels).  The diploidised matrix is written only when
 * diploid_out or d_diploid_out asks for it.  The call waits for the handle's own streams first.  M = 0, T = 0 and S = 0
 * are answered as td_geno_call answers them, without a launch.  TD_E_ARG: ploidy outside 2 .. TD_DOSE_MAX_PLOIDY, prior
 * not 0 | 1, err_ppm outside 1 .. 499 999, min_depth 0, min_call_ppm above 10^6, min_maf_ppm above 500 000, S above 2^24
 * (64 depth1 must fit 64 bits), a table entry above TD_DOSE_COST_MAX, cp NULL with TD_DOSE_HWE, or a marker whose columns
 * are not both below T or are equal: td_last_bad_index gives the marker.  TD_E_LIMIT: more than 65 535 sample chunks. */
typedef struct td_dose_params {
    uint32_t ploidy;          /* P: allele copies of every sample, 2 .. TD_DOSE_MAX_PLOIDY                */
    uint32_t prior;           /* TD_DOSE_FLAT | TD_DOSE_HWE                                               */
    uint32_t err_ppm;         /* the error rate ca / cb were built for                                    */
    uint32_t min_margin;      /* second - best below this: missing; units of 2^-16 bit                    */
    uint64_t min_depth;       /* a + b below this: missing                                                */
    uint32_t min_call_ppm;    /* marker filter: called / S                                                */
    uint32_t min_maf_ppm;     /* marker filter: minor allele frequency among the called                   */
} td_dose_params;
enum {
    TD_DOSE_FLAT = 0,
    TD_DOSE_HWE = 1,
    TD_DOSE_MAX_PLOIDY = 8,
    TD_DOSE_BINS = 64,        /* rows of cp: bins of the marker's allele-1 read share                     */
    TD_DOSE_COST_MAX = 1 << 23,
    TD_DOSE_MISSING = 255,
    TD_DOSE_CALLED = 0,       /* stats: n0 + ... + n8                                                     */
    TD_DOSE_N0 = 1,           /* calls by dosage: TD_DOSE_N0 + d, d = 0 .. 8                              */
    TD_DOSE_ALT = 10,         /* sum of d n[d]: copies of allele 1                                        */
    TD_DOSE_DEPTH0 = 11,      /* sum of a                                                                 */
    TD_DOSE_DEPTH1 = 12,      /* sum of b                                                                 */
    TD_DOSE_BIN = 13,
    TD_DOSE_NSTATS = 14,
    TD_DOSE_CHUNK = 64        /* sample rows per workgroup of the call kernel (td_geno_call's choice)     */
};
int td_dose_call(td_handle *h, const void *d_counts, uint32_t S, uint32_t T, uint32_t M, const uint32_t *i0,
                 const uint32_t *i1, const uint32_t *ca, const uint32_t *cb, const uint32_t *cp, const td_dose_params *p,
                 uint8_t *calls_out, void **d_calls_out, uint8_t *diploid_out, void **d_diploid_out, uint64_t *stats_out,
                 uint8_t *pass_out, uint64_t *passed_out, double *ms);

/* ---- pairwise sample relations (csrc/relate.hip; tagdigger_amd/tagdigger_fun.py sample_relations drives it) -----------
 *
 * From the calls to the check of the samples themselves, without bringing the calls to the host.
 * d_calls is S x M uint8, row-major, in DEVICE memory: td_geno_call's d_calls_out or any td_dev_alloc buffer.  A
 * sample's row is M contiguous bytes and rows are exactly M bytes apart, so no alignment of a row is assumed.  Codes as
 * td_geno_call writes them: 0, 1, 2 copies of allele 1; ANY byte above 2 is missing (TD_GENO_MISSING = 3 included).
 * use (optional, HOST, M bytes): marker m takes part iff use == NULL or use[m] != 0.  The rule, in integers only:
 *   joint[i][j][a][b] = the participating markers m with calls[i][m] == a and calls[j][m] == b
 * for every ordered pair of samples, i == j included, and a, b in 0 .. 2: uint32, S x S x 3 x 3, row-major.  So
 * joint[j][i][b][a] == joint[i][j][a][b], joint[i][i][a][b] == 0 for a != b, and the trace of joint[i][i] is the calls of
 * sample i.  Every pairwise statistic in common use (IBS distance, IBS0 / 1 / 2, the KING-robust kinship) is a function of
 * this table; tagdigger_fun.sample_relations derives them.  The table is the Gram product of the one-hot planes of the
 * calls and is computed on the matrix cores in int8 with int32 accumulators: exact, and independent of scheduling (the
 * partial tables of the marker chunks are combined with integer atomics).  No byte beyond calls[S M - 1] is read.
 * joint_out (optional, HOST, 9 S S uint32) receives the table; d_joint_out (optional) the DEVICE buffer it was computed
 * in, which is then the caller's (td_dev_free).  ms (optional): device time of the kernel.
 * Synchronous; waits for the work enqueued through this handle first.  Checked before anything is read, allocated or
 * launched, whatever the other dimension is: S <= TD_RELATE_MAX_SAMPLES (the table is 9 S^2 4 bytes) and M < 2^31 (no
 * int32 accumulator or uint32 cell can overflow); a violation is TD_E_ARG, and so is a NULL matrix with S M > 0.  After
 * that S = 0 or M = 0 gives an all-zero (or empty) table without a launch. */
enum {
    TD_RELATE_MAX_SAMPLES = 16384,
    TD_RELATE_TILE = 64,      /* samples along a workgroup's tile edge                                    */
    TD_RELATE_KCHUNK = 32768  /* markers per workgroup; the chunks' partial tables are added with atomics */
};
int td_relate_joint(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const uint8_t *use /* HOST, M bytes, or NULL */,
                    uint32_t *joint_out /* HOST, 9*S*S, or NULL */, void **d_joint_out /* or NULL; the caller's, td_dev_free */,
                    double *ms);

/* ---- pairwise marker LD (csrc/ld.hip; tagdigger_amd/tagdigger_fun.py marker_ld drives it) ------------------------------
 *
 * From the calls to the check of the markers against each other: which pairs of markers are correlated
 * over the samples.  d_calls, the codes and use are those of the sample relations above: S x M uint8, row-major, in DEVICE
 * memory, rows exactly M bytes apart, 0 / 1 / 2 copies of allele 1, ANY byte above 2 missing; marker m takes part iff
 * use == NULL or use[m] != 0 (HOST, M bytes).  The rule, in integers only.  For two participating markers i < j (original
 * numbering), over the samples s at which BOTH are called, with x = calls[s][i] and y = calls[s][j]:
 *   n = sum 1, sx = sum x, sy = sum y, sxx = sum x^2, syy = sum y^2, sxy = sum x y
 *   cov = n sxy - sx sy (signed), var_i = n sxx - sx^2, var_j = n syy - sy^2
 * and the pair is an EDGE iff n >= min_shared, var_i > 0, var_j > 0 and cov^2 10^6 >= min_r2_ppm var_i var_j.  With
 * S <= TD_LD_MAX_SAMPLES cov, var_i and var_j fit 32 bits and their products 64; the two sides of the comparison reach 76
 * bits and are compared as 128-bit values.  r^2 = cov^2 / (var_i var_j) and the phase sign(cov) are the caller's to derive.
 * The six sums are Gram products over the samples and run on the matrix cores in int8 with int32 accumulators: exact.
 *
 * *n_out is always the number of edges.  edges_out == NULL counts only.  With a buffer of `capacity` records and
 * n <= capacity the edges are returned ascending by (i, j): the same bytes on every run.  With n > capacity the call
 * returns TD_E_LIMIT; *n_out, degree_out and called_out are complete all the same and no record past the capacity has been
 * written anywhere.  degree_out[m] (optional, HOST, M): the edges m takes part in, whether or not they fit the buffer;
 * called_out[m] (optional, HOST, M): the samples called at m; both 0 for a marker that does not take part.  ms (optional):
 * device time of the two kernels; td_ld_last_times gives the transpose, pair kernel (device ms) and sort (host ms) of the
 * CALLING THREAD's last td_ld_pairs apart, whichever handle that call used (the times are kept per thread, not per handle).  No byte beyond calls[S M - 1] or use[M - 1] is read.
 * Synchronous; waits for the work enqueued through this handle first.  Checked before anything is read, allocated or
 * launched: S <= TD_LD_MAX_SAMPLES, M < 2^31, min_r2_ppm <= 10^6, no NULL matrix with S M > 0 (TD_E_ARG each); then more
 * than TD_LD_MAX_MARKERS participating markers is TD_E_LIMIT.  After that S = 0 or fewer than two participating markers
 * gives no edges without a launch. */
typedef struct td_ld_edge {
    uint32_t i, j;            /* the markers, i < j, original numbering                                    */
    uint32_t shared;          /* n: samples called at both                                                */
    int32_t cov;
    uint32_t var_i, var_j;
} td_ld_edge;                 /* 24 bytes */
enum {
    TD_LD_MAX_SAMPLES = 16384,
    TD_LD_MAX_MARKERS = 1 << 20,
    TD_LD_TILE = 64           /* markers along a workgroup's tile edge                                    */
};
int td_ld_pairs(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const uint8_t *use /* HOST, M bytes, or NULL */,
                uint32_t min_r2_ppm, uint32_t min_shared, td_ld_edge *edges_out /* HOST, capacity records, or NULL */,
                uint64_t capacity, uint64_t *n_out, uint32_t *degree_out /* HOST, M, or NULL */,
                uint32_t *called_out /* HOST, M, or NULL */, double *ms);
int td_ld_last_times(td_handle *h, double *out3 /* transpose ms, pair kernel ms, sort ms of this thread's last td_ld_pairs */);

/* ---- linkage of the markers of a cross (csrc/link.hip; tagdigger_amd/tagdigger_fun.py linkage_map drives it) -------------
 *
 * From the calls of a mapping population to its linkage map: which markers are linked, in which phase, at
 * which recombination fraction.  d_calls and the codes are those of the sections above: S x M uint8, row-major, in DEVICE
 * memory, rows exactly M bytes apart, 0 / 1 / 2, ANY byte above 2 missing.  Only the OFFSPRING rows enter a count: rows
 * (HOST, R row indices below S, none twice, in any order) names them; rows == NULL takes all rows and needs R == S.
 *
 * td_link_counts: counts_out[m] = (c0, c1, c2, cmiss) of marker m over the offspring rows (HOST, M x 4 uint32; the four sum
 * to R).  ms (optional): device time of the kernel.  R = 0 or M = 0 gives zeros (or nothing) without a launch.
 *
 * td_link_pairs: cls (HOST, M bytes) gives every marker its two classes A and B: 0 = (A 0, B 1), 1 = (A 2, B 1),
 * 2 = (A 0, B 2), 255 = the marker takes no part.  A cell's value x is +1 for A, -1 for B and 0 for anything else (the third
 * genotype, missing).  The rule, in integers only.  For two participating markers i < j (original numbering) over the
 * offspring rows:
 *   N = sum x_i^2 x_j^2 (informative at both), D = sum x_i x_j (concordant minus discordant, signed; same parity as N)
 *   rec = (N - |D|) / 2, phase = 0 (coupling) if D >= 0 else 1 (repulsion)
 *   lod16 = 65536 N + lodtab[rec] + lodtab[N - rec] - lodtab[N]      (int64)
 * where lodtab (HOST, R + 1 int64) is the caller's table, lodtab[k] = round(65536 k log2 k) for the LOD in units of
 * log10(2) / 65536 (tagdigger_fun.linkage_tables); the library only looks it up.  The pair is an EDGE iff
 * N >= min_shared, rec 10^6 <= max_rf_ppm N and lod16 >= min_lod16.  D and N are Gram products over the offspring of the
 * planes X (signed) and X & 1 and run on the matrix cores in int8 with int32 accumulators: exact.
 *
 * *n_out is always the number of edges.  edges_out == NULL counts only.  With a buffer of `capacity` records and
 * n <= capacity the edges are returned ascending by (i, j): the same bytes on every run.  With n > capacity the call
 * returns TD_E_LIMIT; *n_out, degree_out and informative_out are complete all the same and no record past the capacity has
 * been written anywhere.  degree_out[m] (optional, HOST, M): the edges m takes part in; informative_out[m] (optional, HOST,
 * M): the offspring with x != 0 at m; both 0 for a marker that takes no part.  ms (optional): device time of the two
 * kernels; td_link_last_times gives the counts kernel of the CALLING THREAD's last td_link_counts and the gather, pair
 * kernel (device ms) and sort (host ms) of its last td_link_pairs apart.  No byte beyond calls[S M - 1], rows[R - 1],
 * cls[M - 1] or lodtab[R] is read.
 * Both are synchronous and wait for the work enqueued through this handle first.  Checked before anything is allocated or
 * launched, TD_E_ARG each: a NULL handle, R <= TD_LINK_MAX_SAMPLES, M < 2^31, rows == NULL with R != S, a row index >= S
 * (td_last_bad_index gives its place in rows), a row listed twice, a NULL counts_out with M > 0 (td_link_counts);
 * max_rf_ppm > 500000, a NULL lodtab, a NULL cls with M > 0, a cls byte outside {0, 1, 2, 255} (td_last_bad_index gives the
 * marker) (td_link_pairs); then more than TD_LINK_MAX_MARKERS participating markers is TD_E_LIMIT; last a NULL matrix with
 * R M > 0 (TD_E_ARG).  After that R = 0 or no participating marker gives no edges without a launch; one participating
 * marker has its informative offspring counted and no pair. */
typedef struct td_link_edge {
    uint32_t i, j;            /* the markers, i < j, original numbering                                    */
    uint32_t n;               /* N: offspring informative at both                                         */
    uint32_t rec_phase;       /* rec | phase << 31                                                        */
    int64_t lod16;
} td_link_edge;               /* 24 bytes */
enum {
    TD_LINK_MAX_SAMPLES = 16384,
    TD_LINK_MAX_MARKERS = 1 << 20,
    TD_LINK_TILE = 64         /* markers along a workgroup's tile edge                                    */
};
int td_link_counts(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const uint32_t *rows /* HOST, R, or NULL = all */,
                   uint32_t R, uint32_t *counts_out /* HOST, M x 4 */, double *ms);
int td_link_pairs(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const uint32_t *rows /* HOST, R, or NULL = all */,
                  uint32_t R, const uint8_t *cls /* HOST, M bytes */, const int64_t *lodtab /* HOST, R + 1 */, uint32_t max_rf_ppm,
                  int64_t min_lod16, uint32_t min_shared, td_link_edge *edges_out /* HOST, capacity records, or NULL */,
                  uint64_t capacity, uint64_t *n_out, uint32_t *degree_out /* HOST, M, or NULL */,
                  uint32_t *informative_out /* HOST, M, or NULL */, double *ms);
int td_link_last_times(td_handle *h, double *out4 /* counts, gather, pair kernel ms, sort ms of this thread's last calls */);

/* ---- LD-kNN imputation of the missing calls (csrc/impute.hip; tagdigger_amd/tagdigger_fun.py impute_calls drives it) ----
 *
 * Fills the holes of the call matrix from the samples most alike over the markers most in LD.  d_calls
 * and the codes are those of the two sections above: S x M uint8, row-major, in DEVICE memory, rows exactly M bytes apart,
 * 0 / 1 / 2 copies of allele 1, ANY byte above 2 missing.  nbr (HOST, M x L int32) is the neighbour table: row m lists the
 * markers whose calls stand in for marker m; an entry is -1 (skipped, anywhere in the row) or a marker below M, never m
 * itself, and none twice in a row (tagdigger_fun.ld_neighbours makes it from td_ld_pairs' edges).  The rule, in integers
 * only.  For marker m let N(m) be the entries of its row that are not -1.  For every TARGET sample t with calls[t][m] > 2,
 * every DONOR d != t with calls[d][m] <= 2 gets, over B = the q in N(m) with calls[t][q] <= 2 and calls[d][q] <= 2:
 *   ovl = |B|,  dist = sum over B of |calls[t][q] - calls[d][q]|,  eligible iff ovl >= min_overlap,
 *   w = floor(32768 (2 ovl - dist) / ovl), in 0 .. 65 536.
 * The VOTERS are the first k eligible donors by (w descending, d ascending); V[g] = the sum of w over the voters with
 * calls[d][m] == g, total = V[0] + V[1] + V[2].  The cell becomes g iff there is a voter, total > 0, exactly one g attains
 * max V, and V[g] 10^6 >= min_conf_ppm total (64-bit).  Otherwise it keeps its input byte, whatever value above 2 that
 * was; called cells are copied byte for byte.  Only the INPUT's calls are ever read: an imputed value serves nobody as a
 * donor's or a neighbour's call, so the result depends on no order.
 * Per marker, stats_out[TD_IMPUTE_STATS m + ...]: missing, imputed, no_donor (targets without an eligible donor, every
 * target of a marker with N(m) empty included), undecided (the rest: tie, zero total, under the confidence).
 * calls_out (optional, HOST, S x M) receives the filled matrix; d_calls_out (optional) the DEVICE buffer it was made in,
 * which is then the caller's (td_dev_free).  ms (optional): device time of the two kernels; td_impute_last_times gives the
 * transpose and the vote kernel of the CALLING THREAD's last td_impute_knn apart.  No byte beyond calls[S M - 1] is read.
 * Synchronous; waits for the work enqueued through this handle first.  Checked before anything is allocated or launched,
 * TD_E_ARG each: S <= TD_IMPUTE_MAX_SAMPLES (the samples' planes, 24 bytes each, lie in one workgroup's LDS), L in
 * 1 .. TD_IMPUTE_MAX_NBR, k in 1 .. TD_IMPUTE_MAX_K, min_overlap >= 1, min_conf_ppm <= 10^6, M < 2^31, no NULL matrix or
 * table with S M > 0, no bad row of the table (td_last_bad_index gives the marker).  After that S = 0 or M = 0 succeeds
 * without a launch. */
typedef struct td_impute_params { uint32_t L, k, min_overlap, min_conf_ppm; } td_impute_params;
enum {
    TD_IMPUTE_MAX_SAMPLES = 4096,
    TD_IMPUTE_MAX_NBR = 64,
    TD_IMPUTE_MAX_K = 32,
    TD_IMPUTE_STATS = 4       /* missing, imputed, no_donor, undecided                                    */
};
int td_impute_knn(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const int32_t *nbr /* HOST, M*L */,
                  const td_impute_params *p, uint8_t *calls_out /* HOST, S*M, or NULL */,
                  void **d_calls_out /* or NULL; the caller's, td_dev_free */, uint32_t *stats_out /* HOST, M*4, or NULL */, double *ms);
int td_impute_last_times(td_handle *h, double *out2 /* transpose ms, vote kernel ms of this thread's last td_impute_knn */);

/* ---- parent pairs by Mendelian trio counts (csrc/parent.hip; tagdigger_amd/tagdigger_fun.py parentage drives it) --------
 *
 * Which two samples are the parents of this one.  d_calls, the codes and use are those of
 * td_relate_joint: S x M uint8, row-major, in DEVICE memory, rows exactly M bytes apart, 0 / 1 / 2 copies of allele 1, ANY
 * byte above 2 missing; marker m takes part iff use == NULL or use[m] != 0 (HOST, M bytes).  offspring (HOST, O sample
 * indices) names the rows of the job; cand (HOST, O x C int32) gives row i its candidate slots 0 .. C - 1: a sample index
 * or -1 (an empty slot, anywhere in the row), never the row's own offspring, none twice in a row.  The rule, in integers
 * only.  TRIO COUNT: for an offspring o and two parents p, q, over the participating markers at which all three are called,
 *   n = their number,
 *   e = those among them at which the offspring's call is not one that parents (p, q) can produce; the allowed sets are
 *       (0,0) -> {0}, (0,1) -> {0,1}, (0,2) -> {1}, (1,1) -> {0,1,2}, (1,2) -> {1,2}, (2,2) -> {2}, symmetric in the parents.
 * With the one-hot bit planes C (called and used), H0, H1, H2 of 64 markers a word this is
 *   n = popc(Co & Cp & Cq),  e = popc(Cp & Cq & ((o2 & (p0 | q0)) | (o0 & (p2 | q2)) | (o1 & ((p0 & q0) | (p2 & q2))))).
 * TRIO NUMBERING: the trios of a row are its slot pairs (a, b), a <= b with TD_PARENT_SELFING in flags and a < b without,
 * numbered t = 0 .. T - 1 row-major, a ascending, then b ascending: T = C (C + 1) / 2 or C (C - 1) / 2.  A pair with an
 * empty slot has n = e = 0.  RANKING: only trios with n >= min_shared are ranked (min_shared >= 1).  Trio x comes before
 * trio y iff e_x n_y < e_y n_x (64-bit products; n, e < 2^31); if those are equal the larger n comes first; if those are
 * equal too the lower t.
 * best_out (HOST, O x K records) receives the first K ranked trios of every row, p = cand[a], q = cand[b]; where fewer than
 * K rank the rest are p = q = 0xFFFFFFFF, n = e = 0.  table_out (optional, HOST, O x T x 2 uint32) receives (n, e) of every
 * trio.  Accumulators are 32 bits wide (M < 2^31), every (n, e) is written exactly once and nothing is combined with
 * atomics: the same bytes on every run.  ms (optional): device time of the three kernels; td_parent_last_times gives the
 * pack, trio and rank kernel of the CALLING THREAD's last td_parent_trios apart.  No byte beyond calls[S M - 1] or
 * use[M - 1] is read.
 * Synchronous; waits for the work enqueued through this handle first.  Checked before anything is read on the device,
 * allocated or launched, TD_E_ARG each: S <= TD_PARENT_MAX_SAMPLES, M < 2^31, C in 1 .. TD_PARENT_MAX_CAND, K in
 * 1 .. TD_PARENT_MAX_TOP, min_shared >= 1, no flag bit but TD_PARENT_SELFING, no NULL matrix with S M > 0, no NULL list or
 * best_out with O > 0, every offspring index below S, every candidate in -1 .. S - 1, not the row's offspring and not named
 * twice in its row (for a bad offspring or candidate entry td_last_bad_index gives the row and the message the entry).
 * After that O = 0 succeeds without a launch, and M = 0 gives all-zero tables and unranked records without a launch (S = 0
 * admits no offspring). */
enum {
    TD_PARENT_MAX_SAMPLES = 16384,
    TD_PARENT_MAX_CAND = 128,
    TD_PARENT_MAX_TOP = 8,
    TD_PARENT_BLOCK = 64,     /* candidate slots along a workgroup's block edge (half of it up to 64 candidates) */
    TD_PARENT_WCHUNK = 16,    /* 64-marker words of the candidates' planes staged in LDS at a time         */
    TD_PARENT_SELFING = 1     /* flags bit 0: the pairs (a, a) are trios too                              */
};
typedef struct td_parent_trio { uint32_t p, q, n, e; } td_parent_trio;   /* 16 bytes; p = cand[a], q = cand[b] */
int td_parent_trios(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const uint8_t *use /* HOST, M bytes, or NULL */,
                    const uint32_t *offspring /* HOST, O sample indices */, uint32_t O,
                    const int32_t *cand /* HOST, O*C, -1 = empty */, uint32_t C, uint32_t flags, uint32_t K, uint32_t min_shared,
                    td_parent_trio *best_out /* HOST, O*K; p = q = 0xFFFFFFFF, n = e = 0 where fewer than K rank */,
                    uint32_t *table_out /* HOST, O*T*2 (n, e), or NULL */, double *ms);
int td_parent_last_times(td_handle *h, double *out3 /* pack, trio, rank: device ms of this thread's last call */);

/* ---- results ---------------------------------------------------------------
 * Both synchronise with all work enqueued through this handle first and
 * return TD_E_NONASCII / TD_E_INTERNAL if a kernel flagged a problem. */
int td_get_counts(td_handle *h, uint64_t *out_rows_by_cols);   /* barnum*ntags, row-major */
int td_get_stats(td_handle *h, uint64_t stats[TD_STAT_NSTATS]);

/* The reference prints its three counters every 50 000 reads (tagdigger_fun.py:268-271).  With
 * td_set_option(h, "progress", 1) set before counting, the device keeps, per window of 50 000 consecutive reads
 * (read ordinals of the whole stream, across streamed pieces), how many reads had a barcode + cut site and how
 * many a tag; this returns them: out[2 w] = barcutcount and out[2 w + 1] = tagcount of the reads in window w,
 * for w < cap (windows without reads are zero), and *nwindows = ceil(reads / 50 000) for the reads THIS handle
 * counted -- a handle that counted from read 0 on needs no more than that many; the shard of a byte-sharded file
 * (first_line > 0) asks for the windows of the whole file.  Running sums over w give the numbers the reference
 * prints after read 50 000 (w + 1).  Cumulative since td_reset; synchronises like td_get_stats. */
int td_get_progress(td_handle *h, uint64_t *out, uint64_t cap, uint64_t *nwindows);

/* K3 of SURVEY 8e: add this library's barcode rows into the run's sample rows on the device --
 * d_dst[row_of_barcode[b]][c] += counts[b][c] for the handle's barnum x ntags uint32 matrix (bound or internal);
 * d_dst is n_dst_rows x ntags uint32 in device memory (e.g. the torch tensor that is all-reduced over RCCL
 * afterwards).  This is what the reference's combineReadCounts (tagdigger_fun.py:1061-1098) does with Python lists
 * after every file: rows whose sample name was seen before are summed.  row_of_barcode is a HOST array of barnum
 * entries.  Synchronous; waits for the handle's own work first and reports what a kernel flagged. */
int td_fold_rows(td_handle *h, const uint32_t *row_of_barcode, uint32_t n_dst_rows, void *d_dst, void *stream);

/* The raw-DEFLATE decoder the GPU runs one BGZF member per lane with (csrc/gpu_inflate.hpp), on the host: inflates
 * in[0..in_len) into out[0..out_len), out_len being the exact inflated size; 0 or a decoder error code (tests). */
int td_inflate_raw_host(const void *in, uint32_t in_len, void *out, uint32_t out_len);

/* Host helper of the CSV writers: vals[0..n) as decimal integers separated by commas (what csv.writer writes for a
 * row of ints, reference writeCounts tagdigger_fun.py:1100-1111) into out[0..capacity); returns the bytes written,
 * -1 when they do not fit (24 bytes per value always do). */
int64_t td_format_csv_row(const int64_t *vals, uint64_t n, char *out, uint64_t capacity);

/* ---- environment ------------------------------------------------------------
 * TAGDIG_STAGE_THREADS    host threads that copy / pread a piece into pinned memory (default 16 on hosts with 32 cores or more, else 8; 1..16)
 * TAGDIG_INFLATE_THREADS  host threads for BGZF member-parallel and gzip chunk-parallel inflate (default: cores, at most 16)
 * TAGDIG_PAR_INFLATE      0: ordinary gzip always on one thread; 1: always chunk-parallel (default: from 8 MiB compressed)
 * TAGDIG_INFLATE_CHUNK    compressed bytes per chunk of the chunk-parallel decoder (default 1 MiB; two chunks per thread and batch)
 * TAGDIG_INFLATE_STATS    set: the chunk-parallel decoder reports batches, chunks and where its time went, on stderr
 * TAGDIG_ZLIB             set: ordinary gzip through zlib's gzread, BGZF members through zlib's inflate
 * TAGDIG_SPLIT_THREADS    writer threads of td_split_file (default 16, at most the host's cores and the number of barcodes)
 * TAGDIG_SPLIT_TIMING     set: td_split_file reports where its wall time went, on stderr
 * TAGDIG_SPLIT_DISCARD    set: td_split_file assembles the records but writes nothing (timing only)
 * TAGDIG_CENSUS_COMBINE   0: the census kernel sends every window to the table by itself (measurements; read at td_census_begin) */

/* ---- tuning / introspection ------------------------------------------------ */
/* Defaults are the measured best; every setting gives the same counts.  name:
 *   "tile_kb"        16 | 32 (default)           bytes of FASTQ per workgroup step
 *   "blocks_per_cu"  0 = what the occupancy query allows (default)
 *   "fastpath"       1 (default): predicted line phase + resolve + fix-up (kernel_fast.hpp);
 *                    0: the exact in-flight kernel with decoupled look-back (kernels.hpp)
 *   "prescan"        1: the exact kernel with a separate line-count pass instead of look-back
 *   "nt_loads"       1 (default): stream the FASTQ with non-temporal loads
 *   "prio"           wave priority per phase of the fast path, two bits each: phase A | B-C << 2 |
 *                    D << 4 | end of A << 6 (default 0xE4)
 *   "table_load_pct" fill of the tag hash table, 10..95 (default 25); applies to the next td_set_index
 *   "kernel"         main pass of the free-running path: 2 (default) k_fast2 -- raw tile in LDS, lines packed by the
 *                    lane that matches them, hot-cell cache (kernel_fast2.hpp); 1 k_fast (kernel_fast.hpp)
 *   "tile_kb2"       k_fast2's tile: 0 (default: chosen from the barcode index's LDS footprint) | 16 | 24 | 32
 *   "hot_cache"      1 (default): k_fast2 counts through its per-wave cache of hot cells in LDS (a wave rests its cache
 *                    while hardly anything hits); 0: plain atomics; 2: the cache never rests (measurements)
 *   "run"            consecutive tiles a workgroup of k_fast2 takes per turn (default 8): the line phase is carried
 *                    inside a run, only its first tile votes
 *   "stagger"        start-up stagger of co-resident workgroups, in 4096-cycle units (default 0)
 *   "timing"         1: record HIP events around every launch for td_kernel_time_ms
 *   "fast_max_matrix_bytes"  count matrices of this many bytes and more go to the exact kernel (the
 *                    free-running one addresses cells as base + 32-bit offset); 0 = the built-in 4 GiB
 *   "progress"       1: keep the reference's progress counters per window of 50 000 reads (td_get_progress); the main pass
 *                    is then k_fast2's recording instantiation (+6 % kernel time) or the exact kernel
 *   "split_kernel"   the splitter's per-read branch: 2 (default) k_split2 -- tile in LDS, one lane per read
 *                    (kernel_splitter2.hpp); 1 k_split (kernel_splitter.hpp)
 *   "gpu_resolve"    1 (default): ordinary gzip of 8 MiB and more -- DEFLATE decoded into 16-bit symbols on the host's
 *                    threads (copies that reach before a chunk stay markers), markers -> bytes and every member's CRC-32
 *                    on the GPU (csrc/gz_resolve.hpp), counted where it lands; 0: all of it on the host, the bytes then
 *                    staged like a plain file's.  (Environment TAGDIG_GPU_RESOLVE=0: the same, for every handle.)
 *   "gpu_inflate"    1 (default): BGZF members are inflated on the GPU; 0: on host threads
 *   "gpu_inflate_crc" 1 (default): every member's CRC-32 is checked on the device
 *   "zb_members"     BGZF members per GPU batch (tests; the built-in 49 152 is also the maximum)
 *   "stage_kb"       KiB per staged piece of a host buffer, plain file or host-inflated stream (tests; 64 .. 32 768,
 *                    0 = the built-in 32 MiB)
 *   "max_grid"       cap on the workgroups of the free-running path's main pass, k_fast, k_fast2 or k_fast4 (tests: with 1,
 *                    one workgroup takes every tile, run after run; 0 = no cap, the default).  The fix-up pass follows it.
 *                    It caps the splitter's grid (k_split2, k_split) in the same way: a workgroup then takes tile after
 *                    tile.  Every cap gives the same counts and the same decisions
 *   "md5_piece"      td_md5_files: bytes a file contributes per round (tests; a multiple of 64, 0 = the built-in size)
 *   "tagnet_max_compares"  td_tagnet_build: the compare cap (tests; 0 = TD_TAGNET_DEFAULT_MAX_COMPARES)
 *   "place_max_compares"   td_place_tags: the compare cap (tests; 0 = TD_PLACE_DEFAULT_MAX_COMPARES)
 *   "debug_ablate"   timing-only ablation bits -- the counts are WRONG when non-zero
 * Returns TD_E_ARG for unknown names. */
int td_set_option(td_handle *h, const char *name, int64_t value);
/* Average device time (ms) of the count kernel over the launches since the
 * last call (HIP events on the launch stream); launches_out optional. */
int td_kernel_time_ms(td_handle *h, double *ms_per_launch, uint32_t *launches_out);
/* The same per launch: out[0 .. min(launches, capacity)) in launch order; *launches_out = how many were written. */
int td_kernel_times_ms(td_handle *h, double *out, uint32_t capacity, uint32_t *launches_out);

/* Diagnostic counters (24 x uint64).  The device's slots are all zero in the shipped build; the phase-stamp
 * build (make prof -> libtagdig_prof.so) fills [0..19] with shader-clock cycles per phase (and so writes over [11]).  Two slots are the host's:
 *   [11]  length of the free-running path's fix-up queue in the last count launch
 *   [20]  where the last line prefix (td_split_device, td_count_and_split_device, td_count_lines_device) took its
 *         per-tile terminator counts from: 1 = counted from the bytes (k_count_lines), 2 = taken from the tile records
 *         the count pass of td_count_and_split_device had just left (k_info_counts); 0 = no prefix yet.  Nothing
 *         depends on it (tests: which source they exercised). */
int td_debug_counters(td_handle *h, uint64_t out[24]);

/* ---- VCF export: body lines formatted on the device (csrc/vcf.hip) ----
 * A body line is prefix[k], then for every sample a tab and the cell, then '\n'.  prefix[k] = prefix[prefix_off[k] ..
 * prefix_off[k + 1]) holds the eight fixed columns and FORMAT; the caller builds it, the library only copies it.  Line k
 * is marker m = sel[k] (any order, repeats allowed).  For sample s: a = counts[s][i0[m]], b = counts[s][i1[m]] (the S x T
 * uint32 matrix in device memory, as for td_geno_call), n = a + b (64-bit), code = calls[s][m] (the S x M uint8 matrix in
 * device memory that td_geno_call or td_dose_call wrote), P = ploidy.  The cell is GT:AD:DP --
 *   GT   code <= P: P - code times '0', then code times '1', joined by '/' (P = 2: 0/0, 0/1, 1/1); code > P (TD_GENO_MISSING
 *        at P = 2, TD_DOSE_MISSING, anything else above P): '.' P times, joined by '/'
 *   AD   a,b in decimal, allele 0 first        DP   n in decimal (up to 2^33 - 2)
 * and with likelihoods = 1 (P = 2 only) :GQ:PL -- ".:." for a missing cell, else GQ:PL0,PL1,PL2 by this integer rule:
 *   x, y = a, b scaled as td_geno_call scales them (n > 127: x = 127 a / n, y = 127 b / n, floor), whatever made the call
 *   c[g] = y ca[g] + x cb[g], g = 0, 1, 2 (ca, cb: the three-entry cost tables of td_dose_call for P = 2, handed in as
 *   data; the library checks only that no entry exceeds TD_DOSE_COST_MAX), cmin = min c
 *   PL[g] = min(255, ((c[g] - cmin) 30103 + 327680000) / 655360000)      (10 log10(2) per bit, rounded half up; uint64)
 *   GQ = min(99, min over g != code of PL[g])
 * A cell with its tab is at most TD_VCF_CELL_MAX bytes.
 *
 * td_vcf_format: line_off_out[0 .. K] (optional) = the byte offset of every line, *n_out = line_off[K].  out == NULL:
 * measure only, nothing is emitted.  Otherwise the text goes to out[0 .. *n_out) (HOST memory); a capacity below that is
 * TD_E_LIMIT with *n_out set to the bytes needed.  ms (optional, 3): device ms of measure, scan, emit.
 * td_vcf_file: the same text written to `path` (append = 0 truncates, 1 appends); *ranges_out (optional) = the ranges it
 * was emitted in; ms (optional, 4): the three and the wall ms spent in write().
 * Emission runs in ranges of consecutive lines of at most range_bytes bytes together (at least one line: a line longer
 * than the budget is a range of its own), double-buffered: a range is formatted while the one before it is copied to the
 * host and written.  K = 0 gives *n_out = 0, S = 0 lines of prefix and '\n'; neither launches anything (ranges: 0).
 * TD_E_ARG (td_last_bad_index where an index is at fault): NULL arguments, a ploidy outside 2 .. TD_DOSE_MAX_PLOIDY,
 * likelihoods with P != 2, a table entry above TD_DOSE_COST_MAX, a marker whose columns are not both below T or are equal
 * (index m), sel[k] >= M (index k), prefix_off[k + 1] < prefix_off[k] (index k), a count matrix that is not 4-byte
 * aligned.  TD_E_IO: the file cannot be opened or written.  TD_E_LIMIT: more than 65 535 chunks of TD_VCF_CHUNK samples,
 * more than TD_VCF_MAX_LINES lines.  The module keeps no state: nothing is left latched after an error. */
typedef struct td_vcf_params {
    uint32_t ploidy;          /* 2 .. TD_DOSE_MAX_PLOIDY                                                  */
    uint32_t likelihoods;     /* 0 | 1; 1 needs ploidy 2                                                  */
    uint64_t range_bytes;     /* 0: TD_VCF_RANGE_BYTES                                                    */
    uint32_t ca[3], cb[3];    /* read with likelihoods = 1                                                */
} td_vcf_params;
enum {
    TD_VCF_CELL_MAX = 64,     /* bytes of a cell with its tab, at most                                    */
    TD_VCF_CHUNK = 64,        /* samples per workgroup of the measure and emit kernels                    */
    TD_VCF_TILE = 64,         /* lines per workgroup of the emit kernel                                   */
    TD_VCF_MTILE = 256,       /* lines per workgroup of the measure kernel                                */
    TD_VCF_MAX_LINES = 1 << 30
};
/* the default budget of a range: a choice that has not been measured */
#define TD_VCF_RANGE_BYTES (256ull << 20)
int td_vcf_format(td_handle *h, const void *d_counts, uint32_t S, uint32_t T, uint32_t M, const uint32_t *i0, const uint32_t *i1,
                  const void *d_calls, const td_vcf_params *p, const uint32_t *sel /* HOST, K */, uint32_t K,
                  const uint8_t *prefix /* HOST */, const uint64_t *prefix_off /* HOST, K + 1 */, uint64_t *line_off_out,
                  uint8_t *out, uint64_t capacity, uint64_t *n_out, double *ms);
int td_vcf_file(td_handle *h, const void *d_counts, uint32_t S, uint32_t T, uint32_t M, const uint32_t *i0, const uint32_t *i1,
                const void *d_calls, const td_vcf_params *p, const uint32_t *sel, uint32_t K, const uint8_t *prefix,
                const uint64_t *prefix_off, const char *path, int append, uint64_t *n_out, uint64_t *ranges_out, double *ms);

/* ---- device memory helpers (so a binding needs no other GPU runtime) ------- */
int td_dev_alloc(td_handle *h, uint64_t nbytes, void **d_out);
int td_dev_free(td_handle *h, void *d_ptr);
int td_memcpy_h2d(td_handle *h, void *d_dst, const void *src, uint64_t nbytes);
int td_memcpy_d2h(td_handle *h, void *dst, const void *d_src, uint64_t nbytes);
int td_device_sync(td_handle *h);

/* ---- bench/test utility: canonical synthetic FASTQ written straight into
 * HBM (include/td_synth_spec.h).  Not on the counting path. */
struct td_synth_params_s;
int td_synth_fill_device(td_handle *h, const void *params /* td_synth_params* */,
                         uint64_t first_read, uint64_t nreads,
                         const char *bar_tab, const uint8_t *bar_len, const char *cut_tab,
                         const char *tag_tab, const uint16_t *tag_len,
                         void *d_out, void *stream);

/* The count matrix that stream implies by the generator's own choices (td_synth_hit: read i is a
 * counted hit of barcode j and tag k), ADDED to d_counts (uint32 [nbar][ntags]); *hits_out = hits.
 * What the bench checks the counting kernels against at full size, without parsing any FASTQ. */
int td_synth_expected_device(td_handle *h, const void *params /* td_synth_params* */,
                             uint64_t first_read, uint64_t nreads, uint32_t *d_counts,
                             uint64_t *hits_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
