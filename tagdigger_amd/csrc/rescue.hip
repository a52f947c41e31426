// Tag rescue: the reads that lie one or two substitutions from a known tag, per barcode and per tag.
// Per read the rule is the counter's up to the barcode (reference tagdigger_fun.py:250-259: lines as text mode splits
// them, line k a read when k % 4 == 1, line.strip().upper(), sequence_index_lookup on barcode + cut site); then
// w = the line from tagoff[b] on, avail = len(w).  A tag t of n bases is a candidate iff n <= avail; d(t) = the positions
// i < n with w[i] != t[i], a character outside ACGT mismatching every base.  A candidate at d = 0: `exact`, nothing is
// written (that read is the counter's).  Otherwise m = the smallest d: m <= K and one tag attains it -> rescued[b][t],
// rescued_at[m], positions[i] for every mismatching i; m <= K and several attain it -> `ambiguous`; else `none`.
//
// The index (built on the host in td_rescue_begin).  K + 1 parts of P = min(32, minlen / (K + 1)) bases at positions
// [pP, (p + 1)P) of every tag: a tag within K substitutions of a window agrees with it on one part at least.  Per part
// the tag ids sorted by the part's bases, and an open-addressing directory {key, run start, run length}; the tags
// themselves at 2 bits a base, 32 bytes each, with their lengths.  Nothing in it is written after begin.
//
//   k_rescue   one workgroup per 16 KiB tile (the handle's k_count_lines + k_scan_tiles give every tile its line index):
//              terminator masks -> the tile's read-line starts as a dense list in LDS -> one lane per read:
//              barcode_lookup (kernels.hpp), the window of up to 128 bases as 2-bit words and a mask of the positions
//              that hold no base, then per part without a masked position one directory probe and one XOR, pair-fold and
//              popcount per tag of the run.
//
// No lane waits for another: the only shared writes are atomic adds on the matrix, on the workgroup's position
// histogram in LDS and on the counters.  Every loop is bounded: a directory probe by the longest displacement and a run
// by the longest run, both known at begin.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#define TD_INST_ONLY                    // (k_scan_tiles is defined in tagdig.hip's translation unit)
#include "stream_pass.hpp"
#include "rescue_common.hpp"                // the window of up to 128 bases and the checks of the tags (shared with bcrescue.hip)

namespace tdr {
using namespace tdk;

constexpr int CPT = 4;                                   // 16-byte chunks per thread: tiles of 16 KiB, as k_count_lines<4> counts them
constexpr uint32_t TILE = CPT * BLOCK * 16u;
static_assert(TILE == tdi::STREAM_TILE, "td_line_prefix (tagdig.hip) counts terminators per 16 KiB tile with k_count_lines<4>");
constexpr uint32_t LIST_CAP = TILE / 4 + 4;              // read-line starts per tile: every fourth terminator, the buffer's own first line
constexpr uint32_t NO_TAG = 0xFFFFFFFFu;
// the rescue's words in device memory, behind the position histogram
enum { RS_READS = 0, RS_BARCUT = 1, RS_EXACT = 2, RS_RESC1 = 3, RS_RESC2 = 4, RS_AMBIG = 5, RS_NONE = 6, RS_ERR = 7, RS_TOTAL = 8,
       RS_PROBES = 9, RS_VERIFIED = 10, RS_NWORDS = 16 };

struct RescueParams {
    const uint8_t *buf;
    uint64_t nbytes;
    uint64_t first_line;       // global index of the buffer's first line (+ *cursor_in)
    uint64_t limit_line;       // last read line that is looked at (maxreads)
    const uint64_t *prefix;    // [ntiles] FLAG_INC | terminators up to the end of tile t
    uint32_t ntiles;
    const uint32_t *bblob;     // barcode + cut site index (the counting path's layout)
    uint32_t bblob_bytes, off_bmeta, off_bdir;
    const uint4 *tagw;         // [ntags][2]: the tag's 128 bases as four 64-bit words, first base in the top bits, zero padded
    const uint32_t *taglen;    // [ntags]
    const uint4 *dir;          // [nparts][dir_mask + 1] {key lo, key hi, run start, run length}; run length 0: empty
    const uint32_t *ent;       // [nparts][ntags] tag ids, sorted by the part's bases
    uint32_t ntags, nparts, P, K;
    uint32_t dir_mask, max_probe;          // slots - 1 (a power of two); the farthest a key sits from its home slot
    uint32_t *matrix;          // [barnum][ntags]
    unsigned long long *positions;         // [128]
    unsigned long long *rs;    // RS_*
    const unsigned long long *cursor_in;
    unsigned long long *cursor_out;
};

__host__ __device__ inline uint32_t part_hash(uint64_t k) {
    uint32_t x = ((uint32_t)k * 0x9E3779B1u) ^ ((uint32_t)(k >> 32) * 0x85EBCA77u);
    x ^= x >> 15; x *= 0x2C1B3C6Du;
    x ^= x >> 13;
    return x;
}
// The line's barcode: gpos moves over the leading blanks (strip), K = its first 32 bases.
__device__ __forceinline__ bool rescue_barcode(const KParams &kp, const TileCtx &cx, uint64_t &gpos, uint32_t &meta) {
    while (gpos < kp.nbytes && is_blank(kp.buf[gpos])) gpos++;          // ends at the terminator at the latest
    const uint32_t a = (uint32_t)(gpos & 15u);
    const uint64_t g0 = gpos & ~15ull;
    const uint2 e0 = convert_chunk(load_chunk(kp, g0)), e1 = convert_chunk(load_chunk(kp, g0 + 16)), e2 = convert_chunk(load_chunk(kp, g0 + 32));
    const uint64_t inv = ((((uint64_t)e2.y << 32) | ((uint64_t)e1.y << 16) | e0.y) >> a) | (1ull << 32);
    const uint32_t nvalid = (uint32_t)__builtin_ctzll(inv);
    const uint32_t r0 = (uint32_t)((((uint64_t)e0.x << 32) | e1.x) >> (32u - 2u * a));
    const uint32_t r1 = (uint32_t)((((uint64_t)e1.x << 32) | e2.x) >> (32u - 2u * a));
    return barcode_lookup(cx.L_bval, cx.L_bmeta, cx.L_bdir, ((uint64_t)r0 << 32) | r1, nvalid, meta);
}

__global__ __launch_bounds__(BLOCK) void k_rescue(const RescueParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint16_t L_mask[CPT * BLOCK];
    __shared__ uint16_t L_list[LIST_CAP];
    __shared__ uint32_t L_misc[16];
    __shared__ uint32_t L_pos[MAXLEN];
    const unsigned long long *L_bval = reinterpret_cast<const unsigned long long *>(lds);
    const uint32_t *L_bmeta = reinterpret_cast<const uint32_t *>(lds + p.off_bmeta);
    const uint16_t *L_bdir = reinterpret_cast<const uint16_t *>(lds + p.off_bdir);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = tid; i < p.bblob_bytes / 4; i += BLOCK) reinterpret_cast<uint32_t *>(lds)[i] = p.bblob[i];
    if (tid < (int)MAXLEN) L_pos[tid] = 0;
    KParams kp{};
    kp.buf = p.buf; kp.nbytes = p.nbytes;
    TileCtx cx{};
    cx.L_bval = L_bval; cx.L_bmeta = L_bmeta; cx.L_bdir = L_bdir;
    const unsigned long long cin = p.cursor_in ? *p.cursor_in : 0ull;
    const uint64_t fl = p.first_line + cin;
    if (blockIdx.x == 0 && tid == 0 && p.cursor_out) *p.cursor_out = cin + p.rs[RS_TOTAL];
    unsigned long long st_reads = 0, st_bar = 0, st_exact = 0, st_r1 = 0, st_r2 = 0, st_ambig = 0, st_none = 0, st_probes = 0, st_verified = 0;
    const uint32_t dir_slots = p.dir_mask + 1u;

    for (uint32_t t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const uint64_t tbase = (uint64_t)t * TILE;
        __syncthreads();
        if (tid == 0) L_misc[9] = 0;
        uint32_t hiacc = 0;
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            const uint32_t c = j * BLOCK + tid;
            const uint64_t g = tbase + (uint64_t)c * 16u;
            const uint4 v = load_chunk(kp, g);
            hiacc |= v.x | v.y | v.z | v.w;
            uint32_t nl = eq_mask16(v, 0x0A0A0A0Au), cr = eq_mask16(v, 0x0D0D0D0Du);
            uint32_t term = nl | (cr & ~(nl >> 1));
            if (cr & 0x8000u) { const uint64_t nx = g + 16; if (nx < p.nbytes && p.buf[nx] == 0x0A) term &= 0x7FFFu; }
            if (g + 16 > p.nbytes) term &= g < p.nbytes ? ((1u << (uint32_t)(p.nbytes - g)) - 1u) : 0u;
            L_mask[c] = (uint16_t)term;
        }
        __syncthreads();
        if (hiacc & 0x80808080u) L_misc[9] = 1;
        uint32_t mm[CPT / 2];
        uint32_t cnt = 0;
#pragma unroll
        for (int i = 0; i < CPT / 2; i++) {
            mm[i] = reinterpret_cast<const uint32_t *>(L_mask)[tid * (CPT / 2) + i];
            cnt += __builtin_popcount(mm[i]);
        }
        const uint32_t incl = wave_incl_scan(cnt, lane);
        if (lane == 63) L_misc[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0, tile_terms = 0;
        for (int w = 0; w < BLOCK / 64; w++) { if (w < wave) wbase += L_misc[w]; tile_terms += L_misc[w]; }
        const bool tile_has_hi = L_misc[9] != 0;
        // terminators before this tile: the previous tile's inclusive prefix.  The line behind the buffer's j-th
        // terminator has index fl + j; this tile holds terminators P + 1 .. P + tile_terms
        const uint64_t P = t ? (p.prefix[t - 1] & ~FLAG_INC) : 0ull;
        const uint64_t j0 = P + 1 + ((1 - (fl + P + 1)) & 3);                        // the first of them that a read line follows
        const uint32_t nlist = P + tile_terms >= j0 ? (uint32_t)((P + tile_terms - j0) >> 2) + 1u : 0u;
        const bool own_first = t == 0 && (fl & 3) == 1;                             // the buffer's own first line is a read
        uint64_t ord = P + wbase + incl - cnt;                                       // terminators before this thread's span
        const uint64_t ord0 = ord;
        const uint32_t span0 = tid * CPT * 16u;
#pragma unroll
        for (int k = 0; k < CPT / 2; k++) {
            uint32_t m = mm[k];
            while (m) {
                const uint32_t bit = __builtin_ctz(m);
                m &= m - 1;
                ord++;
                if (((fl + ord) & 3) == 1) {
                    const uint32_t pos = span0 + 32u * k + bit + 1u;                 // (<= TILE: the line may start the next tile)
                    L_list[(ord - j0) >> 2] = tbase + pos < p.nbytes ? (uint16_t)pos : (uint16_t)0xFFFFu;
                }
            }
        }
        if (own_first && tid == 0) L_list[nlist] = 0;
        __syncthreads();

        // ---------------- one lane per read line
        const uint32_t ntot = nlist + (own_first ? 1u : 0u);
        for (uint32_t base = 0; base < ntot; base += BLOCK) {
            const uint32_t i = base + tid;
            if (i >= ntot) continue;
            const uint32_t pos = L_list[i];
            const uint64_t line = i < nlist ? fl + j0 + 4ull * i : fl;
            if (pos == 0xFFFFu || line > p.limit_line) continue;
            st_reads++;
            uint64_t gpos = tbase + pos;
            uint32_t meta = 0;
            if (!rescue_barcode(kp, cx, gpos, meta)) continue;
            st_bar++;
            const uint32_t blen = meta & 63u, off = (meta >> 6) & 63u, row = meta >> 16;
            uint64_t ws = gpos + off;
            // (an offset behind the barcode entry -- the C-ABI takes one -- may lie behind the line's end: then w is empty)
            for (uint64_t g = gpos + blen; g < gpos + off; g++)
                if (g >= p.nbytes || p.buf[g] == 0x0Au || p.buf[g] == 0x0Du) { ws = g; break; }
            Window W;
            rescue_window(kp, ws, W);
            if (ws != gpos + off) W.avail = 0;

            uint32_t best_d = 0xFFu, best_t = NO_TAG;
            bool tied = false, exact = false;
            for (uint32_t part = 0; part < p.nparts && !exact; part++) {
                const uint32_t s0 = part * p.P;
                if (s0 + p.P > W.avail) break;                                       // (no tag this short: every later part lies behind it too)
                if (part_bits(W.m[0], W.m[1], W.m[2], W.m[3], s0, p.P)) continue;    // a part that holds no base cannot be intact
                const uint64_t key = part_bits(W.w[0], W.w[1], W.w[2], W.w[3], s0, p.P);
                st_probes++;
                const uint4 *dir = p.dir + (uint64_t)part * dir_slots;
                uint32_t slot = part_hash(key) & p.dir_mask, start = 0, len = 0;
                for (uint32_t n = 0; n <= p.max_probe; n++) {
                    const uint4 s = dir[slot];
                    if (s.w == 0) break;
                    if (s.x == (uint32_t)key && s.y == (uint32_t)(key >> 32)) { start = s.z; len = s.w; break; }
                    slot = (slot + 1u) & p.dir_mask;
                }
                const uint32_t *ent = p.ent + (uint64_t)part * p.ntags + start;
                for (uint32_t r = 0; r < len; r++) {
                    const uint32_t tg = ent[r];
                    const uint32_t n = p.taglen[tg];
                    if (n > W.avail || tg == best_t) continue;                       // no candidate; or reached through an earlier part already
                    st_verified++;
                    const uint4 a = p.tagw[2ull * tg];
                    uint32_t d = __builtin_popcountll(diff_bits(W.w[0], ((uint64_t)a.y << 32) | a.x, W.m[0], n, 0)) +
                                 __builtin_popcountll(diff_bits(W.w[1], ((uint64_t)a.w << 32) | a.z, W.m[1], n, 1));
                    if (n > 64u) {
                        const uint4 b = p.tagw[2ull * tg + 1];
                        d += __builtin_popcountll(diff_bits(W.w[2], ((uint64_t)b.y << 32) | b.x, W.m[2], n, 2)) +
                             __builtin_popcountll(diff_bits(W.w[3], ((uint64_t)b.w << 32) | b.z, W.m[3], n, 3));
                    }
                    if (d == 0) { exact = true; break; }
                    if (d > p.K) continue;
                    if (d < best_d) { best_d = d; best_t = tg; tied = false; }
                    else if (d == best_d) tied = true;
                }
            }
            if (exact) st_exact++;
            else if (best_t == NO_TAG) st_none++;
            else if (tied) st_ambig++;
            else {
                if (best_d == 1) st_r1++; else st_r2++;
                atomicAdd(p.matrix + (uint64_t)row * p.ntags + best_t, 1u);
                const uint32_t n = p.taglen[best_t];
                const uint4 a = p.tagw[2ull * best_t], b = p.tagw[2ull * best_t + 1];
                const uint64_t T[4] = {((uint64_t)a.y << 32) | a.x, ((uint64_t)a.w << 32) | a.z, ((uint64_t)b.y << 32) | b.x, ((uint64_t)b.w << 32) | b.z};
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    uint64_t bits = diff_bits(W.w[w], T[w], W.m[w], n, w);
                    while (bits) {
                        const uint32_t lz = (uint32_t)__builtin_clzll(bits);
                        bits &= ~(1ull << (63u - lz));
                        atomicAdd(&L_pos[32u * w + (lz >> 1)], 1u);
                    }
                }
            }
        }

        // ---------------- rare: bytes >= 0x80 in the tile -- are any inside a read line that is looked at?  (k_count's rule)
        if (tile_has_hi) {
            const uint64_t Lb = fl + ord0;               // index of the line this thread's span starts in
            uint32_t seen = 0;
#pragma unroll
            for (int k = 0; k < CPT / 2; k++) {
                const uint32_t m = mm[k];
#pragma nounroll
                for (uint32_t q = 0; q < 32u; q++) {
                    const uint64_t g = tbase + span0 + 32u * k + q;
                    if (g < p.nbytes && p.buf[g] >= 0x80u) {
                        const uint64_t line = Lb + seen;
                        if ((line & 3) == 1 && line <= p.limit_line) atomicOr(p.rs + RS_ERR, ERR_NONASCII);
                    }
                    seen += (m >> q) & 1u;
                }
            }
        }
        // the tile's share of the position histogram (a tile holds fewer than 2^13 reads: no cell wraps)
        __syncthreads();
        if (tid < (int)MAXLEN) {
            const uint32_t v = L_pos[tid];
            if (v) { L_pos[tid] = 0; atomicAdd(p.positions + tid, (unsigned long long)v); }
        }
    }
    const unsigned long long sums[9] = {wave_sum64(st_reads), wave_sum64(st_bar), wave_sum64(st_exact), wave_sum64(st_r1), wave_sum64(st_r2),
                                        wave_sum64(st_ambig), wave_sum64(st_none), wave_sum64(st_probes), wave_sum64(st_verified)};
    if (lane == 0) {
        const int at[9] = {RS_READS, RS_BARCUT, RS_EXACT, RS_RESC1, RS_RESC2, RS_AMBIG, RS_NONE, RS_PROBES, RS_VERIFIED};
#pragma unroll
        for (int k = 0; k < 9; k++) if (sums[k]) atomicAdd(p.rs + at[k], sums[k]);
    }
}

}  // namespace tdr

// ============================================================================ host side
namespace {

constexpr size_t RESCUE_LDS_INDEX = 40 * 1024;            // the barcode index's share of a workgroup's LDS, as the census's
// The longest run of tags under one part key that the device takes.  Every tag of a run is verified by the lane that
// reached it, so a run costs its length per read.  A GUESS: the sweep that would set it where one pass costs what the
// host rule costs has not been measured.
constexpr uint32_t RESCUE_DEFAULT_MAX_RUN = 4096;

struct Rescue : tdi::StreamPass {
    uint32_t barnum = 0, ntags = 0, K = 0, P = 0;
    uint32_t dir_mask = 0, max_probe = 0, longest_run = 0;
    tdi::DevBuf<uint32_t> d_taglen, d_ent, d_matrix;
    tdi::DevBuf<uint4> d_tagw, d_dir;
    tdi::DevBuf<unsigned long long> d_words;  // positions[128] | RS_*
    size_t cells() const { return (size_t)barnum * ntags; }
    unsigned long long *d_pos() const { return d_words.p; }
    unsigned long long *d_rs() const { return d_words.p + tdr::MAXLEN; }

    int zero(hipStream_t s) override {
        TD_HIPCHK(hipMemsetAsync(d_matrix.p, 0, std::max<size_t>(cells(), 1) * 4, s));
        TD_HIPCHK(hipMemsetAsync(d_words.p, 0, (tdr::MAXLEN + tdr::RS_NWORDS) * 8, s));
        return TD_OK;
    }

    int launch(const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, hipStream_t stream,
               const unsigned long long *cursor_in, unsigned long long *cursor_out) override {
        tdr::RescueParams p{};
        const int rc = prologue(d_fastq, nbytes, max_reads, stream, d_rs() + tdr::RS_TOTAL, p.prefix, p.ntiles);
        if (rc || !p.ntiles) return rc;
        p.buf = (const uint8_t *)d_fastq; p.nbytes = nbytes; p.first_line = first_line;
        p.limit_line = limit_line(max_reads);
        p.bblob = d_bblob.p; p.bblob_bytes = bblob_bytes; p.off_bmeta = off_bmeta; p.off_bdir = off_bdir;
        p.tagw = d_tagw.p; p.taglen = d_taglen.p; p.dir = d_dir.p; p.ent = d_ent.p;
        p.ntags = ntags; p.nparts = K + 1; p.P = P; p.K = K; p.dir_mask = dir_mask; p.max_probe = max_probe;
        p.matrix = d_matrix.p; p.positions = d_pos(); p.rs = d_rs();
        p.cursor_in = cursor_in; p.cursor_out = cursor_out;
        hipLaunchKernelGGL(tdr::k_rescue, dim3(grid(p.ntiles, 8, true)), dim3(tdk::BLOCK), bblob_bytes, stream, p);
        TD_HIPCHK(hipGetLastError());
        return TD_OK;
    }

    // after a synchronisation: what the kernel flagged
    int sync_stats(unsigned long long rs[tdr::RS_NWORDS]) { return sync_words(rs, d_rs(), tdr::RS_NWORDS, tdr::RS_ERR); }
};

Rescue *rescue_of(td_handle *h) { return tdi::state_of<Rescue>(h, tdi::RESCUE); }

// What td_rescue_begin builds on the host.  No HIP in here.
struct RescueIndex {
    uint32_t P = 0, longest_run = 0, dir_slots = 0, max_probe = 0;
    std::vector<uint64_t> words;              // [ntags][4]
    std::vector<uint32_t> lens;               // [ntags]
    std::vector<uint32_t> ent;                // [nparts][ntags]
    std::vector<uint32_t> dir;                // [nparts][dir_slots][4]
};

int rescue_build_index(const std::vector<std::string> &ts, uint32_t K, uint32_t max_run, RescueIndex &ix) {
    const uint32_t n = (uint32_t)ts.size(), nparts = K + 1;
    size_t minlen = ts[0].size();
    for (auto &t : ts) minlen = std::min(minlen, t.size());
    ix.P = (uint32_t)std::min<size_t>(32, minlen / nparts);
    if (ix.P < 1)
        return td_fail_internal(TD_E_LIMIT, ("tag rescue: run of all " + std::to_string(n) + " tags: the shortest tag has " + std::to_string(minlen) +
                                             " bases, which leaves no part for " + std::to_string(K) + " mismatches").c_str());
    ix.words.assign((size_t)n * 4, 0);
    ix.lens.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        ix.lens[i] = (uint32_t)ts[i].size();
        for (size_t q = 0; q < ts[i].size(); q++) {
            const char c = ts[i][q];
            const uint64_t code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'T' ? 2 : 3;       // (byte >> 1) & 3, as convert_chunk packs a read
            ix.words[(size_t)i * 4 + (q >> 5)] |= code << (62 - 2 * (q & 31));
        }
    }
    ix.dir_slots = 16;
    while (ix.dir_slots < 2ull * n) ix.dir_slots <<= 1;
    ix.ent.resize((size_t)nparts * n);
    ix.dir.assign((size_t)nparts * ix.dir_slots * 4, 0);
    std::vector<std::pair<uint64_t, uint32_t>> keyed(n);
    for (uint32_t part = 0; part < nparts; part++) {
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t *w = &ix.words[(size_t)i * 4];
            keyed[i] = {tdr::part_bits(w[0], w[1], w[2], w[3], part * ix.P, ix.P), i};
        }
        std::sort(keyed.begin(), keyed.end());
        uint32_t *dir = &ix.dir[(size_t)part * ix.dir_slots * 4];
        for (uint32_t i = 0; i < n;) {
            uint32_t j = i;
            while (j < n && keyed[j].first == keyed[i].first) { ix.ent[(size_t)part * n + j] = keyed[j].second; j++; }
            ix.longest_run = std::max(ix.longest_run, j - i);
            uint32_t slot = tdr::part_hash(keyed[i].first) & (ix.dir_slots - 1), hops = 0;
            while (dir[slot * 4 + 3]) { slot = (slot + 1) & (ix.dir_slots - 1); hops++; }
            dir[slot * 4] = (uint32_t)keyed[i].first; dir[slot * 4 + 1] = (uint32_t)(keyed[i].first >> 32);
            dir[slot * 4 + 2] = i; dir[slot * 4 + 3] = j - i;
            ix.max_probe = std::max(ix.max_probe, hops);
            i = j;
        }
    }
    if (ix.longest_run > max_run)
        return td_fail_internal(TD_E_LIMIT, ("tag rescue: run of " + std::to_string(ix.longest_run) + " tags share one part of " + std::to_string(ix.P) +
                                             " bases, rescue_max_run is " + std::to_string(max_run)).c_str());
    return TD_OK;
}

}  // namespace

extern "C" {

int td_rescue_begin(td_handle *h, const char *const *barcut, uint32_t n_barcut, uint32_t barnum, const uint32_t *tagoff,
                    const char *const *tags, uint32_t n_tags, uint32_t max_mismatch) {
    if (!h || !barcut || !tagoff || !tags) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (max_mismatch < 1 || max_mismatch > 2) return td_fail_internal(TD_E_ARG, "max_mismatch must be 1 or 2");
    int rc = tdi::quiet_reset(h, tdi::RESCUE); if (rc) return rc;
    std::unique_ptr<Rescue> r(new Rescue());
    rc = r->begin(h, barcut, n_barcut, barnum, tagoff, RESCUE_LDS_INDEX); if (rc) return rc;
    std::vector<std::string> ts;
    rc = rescue_check_tags(tags, n_tags, ts); if (rc) return rc;
    const uint32_t opt = td_handle_rescue_max_run(h);
    RescueIndex ix;
    rc = rescue_build_index(ts, max_mismatch, opt ? opt : RESCUE_DEFAULT_MAX_RUN, ix); if (rc) return rc;
    if ((uint64_t)barnum * n_tags >= (1ull << 32)) return td_fail_internal(TD_E_LIMIT, "rescue matrix beyond 2^32 cells");

    r->barnum = barnum; r->ntags = n_tags; r->K = max_mismatch; r->P = ix.P;
    r->dir_mask = ix.dir_slots - 1; r->max_probe = ix.max_probe; r->longest_run = ix.longest_run;
    hipError_t e = r->d_tagw.alloc(ix.words.size() / 2);
    if (e == hipSuccess) e = hipMemcpy(r->d_tagw.p, ix.words.data(), ix.words.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = r->d_taglen.alloc(ix.lens.size());
    if (e == hipSuccess) e = hipMemcpy(r->d_taglen.p, ix.lens.data(), ix.lens.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = r->d_ent.alloc(ix.ent.size());
    if (e == hipSuccess) e = hipMemcpy(r->d_ent.p, ix.ent.data(), ix.ent.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = r->d_dir.alloc(ix.dir.size() / 4);
    if (e == hipSuccess) e = hipMemcpy(r->d_dir.p, ix.dir.data(), ix.dir.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = r->d_matrix.alloc(r->cells());
    if (e == hipSuccess) e = r->d_words.alloc(tdr::MAXLEN + tdr::RS_NWORDS);
    if (e != hipSuccess) return tdi::StreamPass::hip_failed(e);
    return tdi::install(r, tdi::RESCUE);
}

int td_rescue_device(td_handle *h, const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, void *stream) {
    Rescue *r = rescue_of(h);
    if (!r) return tdi::no_state("rescue", h);
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    return r->launch(d_fastq, nbytes, first_line, max_reads, (hipStream_t)stream, nullptr, nullptr);
}

int td_rescue_file(td_handle *h, const char *path, uint64_t max_reads) {
    Rescue *r = rescue_of(h);
    if (!r || !path) return tdi::no_state("rescue", h && path);
    unsigned long long rs[tdr::RS_NWORDS];
    const int rc = r->file(path, max_reads);
    return rc ? rc : r->sync_stats(rs);
}

int td_rescue_stats(td_handle *h, uint64_t out[8]) {
    Rescue *r = rescue_of(h);
    if (!r || !out) return tdi::no_state("rescue", h && out);
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    unsigned long long rs[tdr::RS_NWORDS];
    const int rc = r->sync_stats(rs); if (rc) return rc;
    out[TD_RESCUE_READS] = rs[tdr::RS_READS]; out[TD_RESCUE_BARCUT] = rs[tdr::RS_BARCUT]; out[TD_RESCUE_EXACT] = rs[tdr::RS_EXACT];
    out[TD_RESCUE_RESCUED1] = rs[tdr::RS_RESC1]; out[TD_RESCUE_RESCUED2] = rs[tdr::RS_RESC2]; out[TD_RESCUE_AMBIGUOUS] = rs[tdr::RS_AMBIG];
    out[TD_RESCUE_NONE] = rs[tdr::RS_NONE]; out[TD_RESCUE_LONGEST_RUN] = r->longest_run;
    return TD_OK;
}

int td_rescue_work(td_handle *h, uint64_t out[4]) {
    Rescue *r = rescue_of(h);
    if (!r || !out) return tdi::no_state("rescue", h && out);
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    unsigned long long rs[tdr::RS_NWORDS];
    const int rc = r->sync_stats(rs); if (rc) return rc;
    out[0] = rs[tdr::RS_PROBES]; out[1] = rs[tdr::RS_VERIFIED]; out[2] = r->P; out[3] = r->max_probe;
    return TD_OK;
}

int td_rescue_fetch(td_handle *h, uint32_t *rescued_out, uint64_t *positions_out) {
    Rescue *r = rescue_of(h);
    if (!r) return tdi::no_state("rescue", h);
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    unsigned long long rs[tdr::RS_NWORDS];
    const int rc = r->sync_stats(rs); if (rc) return rc;
    if (rescued_out && r->cells()) TD_HIPCHK(hipMemcpy(rescued_out, r->d_matrix.p, r->cells() * 4, hipMemcpyDeviceToHost));
    if (positions_out) TD_HIPCHK(hipMemcpy(positions_out, r->d_pos(), tdr::MAXLEN * 8, hipMemcpyDeviceToHost));
    return TD_OK;
}

int td_rescue_matrix(td_handle *h, void **d_matrix) {
    Rescue *r = rescue_of(h);
    if (!r || !d_matrix) return tdi::no_state("rescue", h && d_matrix);
    if (r->dead) return r->answer_dead();
    *d_matrix = r->d_matrix.p;
    return TD_OK;
}

int td_rescue_end(td_handle *h) {
    if (!h) return td_fail_internal(TD_E_ARG, "handle is NULL");
    if (!rescue_of(h)) return tdi::no_state("rescue", true);
    return tdi::quiet_reset(h, tdi::RESCUE);
}

}  // extern "C"
