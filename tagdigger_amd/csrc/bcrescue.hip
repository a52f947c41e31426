// Barcode rescue: the reads whose first bases are no stored barcode + cut site entry but lie one or two
// substitutions from the entries of exactly one barcode, counted per barcode and per tag.  Lines as the counter takes
// them (line k a read when k % 4 == 1, line.strip().upper()).  Per read: an entry that is an exact prefix (barcode_lookup,
// kernels.hpp) -> `exact`, the read is the counter's.  Otherwise every entry e of L_e <= len(read) bases is a candidate
// at d(e) = the positions i < L_e with read[i] != e[i], a character outside ACGT mismatching every base; m = the smallest
// d.  m > K or no candidate -> `none`; the entries at m belong to several rows -> `ambiguous` (variants of one row that
// tie are no tie: the earliest in the list is "the entry"); else rescued: rescued_at[m], row_rescued[b][m - 1],
// positions[i] for every mismatching i of the entry, and the counter's tag step from tagoff[b] on: the one stored tag
// that is a prefix of the rest, all of its characters in ACGT, -> matrix[b][t] and `tagged`.
//
// The index (td_bcrescue_begin, on the host): td_barcut_blob's bval / bmeta / bdir as the counter's, a list `order` of
// the distinct surviving entries in list order (blob positions; an entry shorter than the directory's 5 bases lies in
// several buckets and is listed once), and for the exact tag step the tag ids sorted by their first P = min(32, shortest
// tag) bases under an open-addressing directory {key, run start, run length}.  Nothing in it is written after begin.
//
//   k_bcrescue  one workgroup per 16 KiB tile on td_line_prefix's line index: terminator masks -> the tile's read-line
//               starts as a dense list in LDS -> rounds of BLOCK reads:
//                 A  one lane per read: strip, the first 32 bases packed, barcode_lookup; a read without a hit goes
//                    into the round's no-hit list in LDS (ballot / mbcnt): packed bases, pair mask of the positions that
//                    hold no base or lie behind the line's end, length, line start
//                 B  one wave per no-hit read, its lanes strided over `order`: XOR with bval, pair-fold, OR with the
//                    mask, shift by 64 - 2 L_e, popcount; every lane keeps its nearest entry as (d << 16 | list rank),
//                    the wave's is a DPP min-reduce, the tie between rows one ballot
//                 C  one lane per rescued read: counters, positions, the window behind tagoff[b], one directory probe
//                    and one XOR per tag of the run
//
// No lane waits for another: the shared writes are atomic adds on the matrix and the per-row counters, on the
// workgroup's position histogram and list length in LDS, and on the counters once per wave.  Every loop is bounded: the
// entries by their number, a directory probe by the longest displacement, a run by its length, all known at begin.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#define TD_INST_ONLY                    // (k_scan_tiles is defined in tagdig.hip's translation unit)
#include "stream_pass.hpp"
#include "rescue_common.hpp"            // the window of up to 128 bases, td_rescue_begin's checks of the tags

namespace tdb {
using namespace tdk;

constexpr int CPT = 4;                                   // 16-byte chunks per thread: tiles of 16 KiB, as k_count_lines<4> counts them
constexpr uint32_t TILE = CPT * BLOCK * 16u;
static_assert(TILE == tdi::STREAM_TILE, "td_line_prefix (tagdig.hip) counts terminators per 16 KiB tile with k_count_lines<4>");
constexpr uint32_t LIST_CAP = TILE / 4 + 4;              // read-line starts per tile: every fourth terminator, the buffer's own first line
constexpr uint32_t ENTRY_BASES = 32;                     // bases of an entry at most, and of the packed read prefix
constexpr uint32_t RES_NONE = 0, RES_AMBIG = 1, RES_RESCUED = 2;      // a no-hit read's outcome: RES_RESCUED | m << 2 | blob position << 8
// the module's words in device memory, behind the per-row counters and the position histogram
enum { BS_READS = 0, BS_EXACT = 1, BS_RESC1 = 2, BS_RESC2 = 3, BS_AMBIG = 4, BS_NONE = 5, BS_TAGGED = 6, BS_ERR = 7, BS_TOTAL = 8, BS_NWORDS = 16 };

struct BcParams {
    const uint8_t *buf;
    uint64_t nbytes;
    uint64_t first_line;       // global index of the buffer's first line (+ *cursor_in)
    uint64_t limit_line;       // last read line that is looked at (maxreads)
    const uint64_t *prefix;    // [ntiles] FLAG_INC | terminators up to the end of tile t
    uint32_t ntiles;
    const uint32_t *bblob;     // barcode + cut site index (the counting path's layout) | order u16[n_order]
    uint32_t bblob_bytes, off_bmeta, off_bdir, off_order, n_order;
    const uint4 *tagw;         // [ntags][2]: the tag's 128 bases as four 64-bit words, first base in the top bits, zero padded
    const uint32_t *taglen;    // [ntags]
    const uint4 *dir;          // [dir_mask + 1] {key lo, key hi, run start, run length}; run length 0: empty
    const uint32_t *ent;       // [ntags] tag ids, sorted by their first P bases
    uint32_t ntags, P, K;
    uint32_t dir_mask, max_probe;          // slots - 1 (a power of two); the farthest a key sits from its home slot
    uint32_t *matrix;          // [barnum][ntags]
    unsigned long long *row_rescued;       // [barnum][2]
    unsigned long long *positions;         // [32]
    unsigned long long *bs;    // BS_*
    const unsigned long long *cursor_in;
    unsigned long long *cursor_out;
};

__host__ __device__ inline uint32_t dir_hash(uint64_t k) {
    uint32_t x = ((uint32_t)k * 0x9E3779B1u) ^ ((uint32_t)(k >> 32) * 0x85EBCA77u);
    x ^= x >> 15; x *= 0x2C1B3C6Du;
    x ^= x >> 13;
    return x;
}
// mismatching positions of an entry of L bases (1 .. 32): bit 2 (L - 1 - i) for base i
__host__ __device__ inline uint64_t entry_diff(uint64_t read, uint64_t mask, uint64_t val, uint32_t L) {
    const uint64_t x = read ^ val;
    return (((x | (x >> 1)) & 0x5555555555555555ull) | mask) >> (64u - 2u * L);
}
// the smallest value of the wave in six DPP steps (the shape of wave_incl_scan, kernels.hpp), read from lane 63
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x111, 0xf, 0xf, false));    // row_shr:1
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x112, 0xf, 0xf, false));    // row_shr:2
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x114, 0xf, 0xf, false));    // row_shr:4
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x118, 0xf, 0xf, false));    // row_shr:8
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x142, 0xa, 0xf, false));    // row_bcast:15 into rows 1, 3
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x143, 0xc, 0xf, false));    // row_bcast:31 into rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// The head of a line: gpos moves over the leading blanks (strip); R = its first 32 bases, packed.  True: an entry is an
// exact prefix (meta).  Else M = the pair mask of the positions that hold no base or lie behind the stripped line's
// end, len = min(len(line), 32).
__device__ __forceinline__ bool line_head(const KParams &kp, const TileCtx &cx, uint64_t &gpos, uint32_t &meta, uint64_t &R, uint64_t &M, uint32_t &len) {
    while (gpos < kp.nbytes && is_blank(kp.buf[gpos])) gpos++;          // ends at the terminator at the latest
    const uint32_t a = (uint32_t)(gpos & 15u);
    const uint64_t g0 = gpos & ~15ull;
    const uint4 v0 = load_chunk(kp, g0), v1 = load_chunk(kp, g0 + 16), v2 = load_chunk(kp, g0 + 32);
    const uint2 e0 = convert_chunk(v0), e1 = convert_chunk(v1), e2 = convert_chunk(v2);
    const uint64_t inv = (((uint64_t)e2.y << 32) | ((uint64_t)e1.y << 16) | e0.y) >> a;              // (33 positions at least)
    const uint32_t nvalid = (uint32_t)__builtin_ctzll(inv | (1ull << 32));
    const uint32_t r0 = (uint32_t)((((uint64_t)e0.x << 32) | e1.x) >> (32u - 2u * a));
    const uint32_t r1 = (uint32_t)((((uint64_t)e1.x << 32) | e2.x) >> (32u - 2u * a));
    R = ((uint64_t)r0 << 32) | r1;
    if (barcode_lookup(cx.L_bval, cx.L_bmeta, cx.L_bdir, R, nvalid, meta)) return true;
    // where the line ends inside the 32 positions: its terminator, or the buffer's end
    const uint32_t t0 = eq_mask16(v0, 0x0A0A0A0Au) | eq_mask16(v0, 0x0D0D0D0Du), t1 = eq_mask16(v1, 0x0A0A0A0Au) | eq_mask16(v1, 0x0D0D0D0Du),
                   t2 = eq_mask16(v2, 0x0A0A0A0Au) | eq_mask16(v2, 0x0D0D0D0Du);
    const uint64_t trm = (((uint64_t)t2 << 32) | ((uint64_t)t1 << 16) | t0) >> a;
    const uint32_t q = (uint32_t)__builtin_ctzll(trm | (1ull << 32));
    const uint64_t room = kp.nbytes - gpos;
    const uint32_t end = room < q ? (uint32_t)room : q;
    uint64_t e = gpos + end;
    // strip: blanks before the end do not belong to the line.  Its last byte is a base in every read but a few
    if (end && ((inv >> (end - 1u)) & 1u)) {
        if (end == ENTRY_BASES) while (e < kp.nbytes && kp.buf[e] != 0x0Au && kp.buf[e] != 0x0Du) e++;      // the line goes on behind the 32 positions
        while (e > gpos && is_blank(kp.buf[e - 1])) e--;
    }
    len = e - gpos < ENTRY_BASES ? (uint32_t)(e - gpos) : ENTRY_BASES;
    M = tdr::spread_mask((uint32_t)inv | (len < ENTRY_BASES ? ~0u << len : 0u));
    return false;
}

__global__ __launch_bounds__(BLOCK) void k_bcrescue(const BcParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint16_t L_mask[CPT * BLOCK];
    __shared__ uint16_t L_list[LIST_CAP];
    __shared__ uint32_t L_misc[16];
    __shared__ uint32_t L_pos[ENTRY_BASES];
    // the round's no-hit reads
    __shared__ uint64_t L_nhR[BLOCK], L_nhM[BLOCK], L_nhAt[BLOCK];
    __shared__ uint32_t L_nhLen[BLOCK], L_nhRes[BLOCK];
    const unsigned long long *L_bval = reinterpret_cast<const unsigned long long *>(lds);
    const uint32_t *L_bmeta = reinterpret_cast<const uint32_t *>(lds + p.off_bmeta);
    const uint16_t *L_bdir = reinterpret_cast<const uint16_t *>(lds + p.off_bdir);
    const uint16_t *L_order = reinterpret_cast<const uint16_t *>(lds + p.off_order);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = tid; i < p.bblob_bytes / 4; i += BLOCK) reinterpret_cast<uint32_t *>(lds)[i] = p.bblob[i];
    if (tid < (int)ENTRY_BASES) L_pos[tid] = 0;
    KParams kp{};
    kp.buf = p.buf; kp.nbytes = p.nbytes;
    TileCtx cx{};
    cx.L_bval = L_bval; cx.L_bmeta = L_bmeta; cx.L_bdir = L_bdir;
    const unsigned long long cin = p.cursor_in ? *p.cursor_in : 0ull;
    const uint64_t fl = p.first_line + cin;
    if (blockIdx.x == 0 && tid == 0 && p.cursor_out) *p.cursor_out = cin + p.bs[BS_TOTAL];
    unsigned long long st_reads = 0, st_exact = 0, st_r1 = 0, st_r2 = 0, st_ambig = 0, st_none = 0, st_tagged = 0;

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

        const uint32_t ntot = nlist + (own_first ? 1u : 0u);
        for (uint32_t base = 0; base < ntot; base += BLOCK) {
            __syncthreads();                                                         // the lists are written; the round before is read
            if (tid == 0) L_misc[8] = 0;
            __syncthreads();
            // ---------------- A: one lane per read line
            const uint32_t i = base + tid;
            bool nohit = false;
            uint64_t gpos = 0, R = 0, M = 0;
            uint32_t len = 0;
            if (i < ntot) {
                const uint32_t pos = L_list[i];
                const uint64_t line = i < nlist ? fl + j0 + 4ull * i : fl;
                if (pos != 0xFFFFu && line <= p.limit_line) {
                    st_reads++;
                    gpos = tbase + pos;
                    uint32_t meta = 0;
                    if (line_head(kp, cx, gpos, meta, R, M, len)) st_exact++;
                    else nohit = true;
                }
            }
            const uint64_t bal = __ballot(nohit);
            uint32_t wslot = 0;
            if (lane == 0 && bal) wslot = atomicAdd(&L_misc[8], (uint32_t)__builtin_popcountll(bal));
            wslot = (uint32_t)__builtin_amdgcn_readfirstlane((int)wslot);
            if (nohit) {
                const uint32_t s = wslot + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                L_nhR[s] = R; L_nhM[s] = M; L_nhAt[s] = gpos; L_nhLen[s] = len;
            }
            __syncthreads();
            const uint32_t nnh = L_misc[8];

            // ---------------- B: one wave per no-hit read, lanes strided over the entries in list order
            for (uint32_t s = wave; s < nnh; s += BLOCK / 64) {
                const uint64_t rd = L_nhR[s], mk = L_nhM[s];
                const uint32_t ln = L_nhLen[s];
                uint32_t best = 0xFFFFFFFFu, brow = 0;
                bool rows = false;                                                   // this lane's entries at its smallest distance lie in several rows
                for (uint32_t r = lane; r < p.n_order; r += 64) {
                    const uint32_t ci = L_order[r];
                    const uint32_t m = L_bmeta[ci];
                    const uint32_t L = m & 63u;
                    if (L > ln) continue;                                            // no candidate
                    const uint32_t d = (uint32_t)__builtin_popcountll(entry_diff(rd, mk, L_bval[ci], L));
                    if (d > p.K) continue;
                    if (d < (best >> 16)) { best = (d << 16) | r; brow = m >> 16; rows = false; }
                    else if (d == (best >> 16) && (m >> 16) != brow) rows = true;
                }
                const uint32_t win = wave_min_u32(best);                             // the smallest distance, of those the earliest entry
                uint32_t res = RES_NONE;
                if (win != 0xFFFFFFFFu) {
                    const uint32_t ci = L_order[win & 0xFFFFu];
                    const uint32_t wrow = L_bmeta[ci] >> 16;
                    const bool tie = __ballot((best >> 16) == (win >> 16) && (rows || brow != wrow)) != 0;
                    res = tie ? RES_AMBIG : RES_RESCUED | ((win >> 16) << 2) | (ci << 8);
                }
                if (lane == 0) {
                    L_nhRes[s] = res;
                    if (res == RES_NONE) st_none++; else if (res == RES_AMBIG) st_ambig++;
                }
            }
            __syncthreads();

            // ---------------- C: one lane per rescued read
            if ((uint32_t)tid < nnh && (L_nhRes[tid] & 3u) == RES_RESCUED) {
                const uint32_t res = L_nhRes[tid], ci = res >> 8;
                const uint32_t meta = L_bmeta[ci], blen = meta & 63u, off = (meta >> 6) & 63u, row = meta >> 16;
                // (m is 1 or 2: a read at distance 0 has its exact entry.  No address is computed from m or from blen <= len)
                const bool at1 = ((res >> 2) & 3u) == 1u;
                if (at1) st_r1++; else st_r2++;
                atomicAdd(p.row_rescued + 2ull * row + (at1 ? 0u : 1u), 1ull);
                uint64_t bits = entry_diff(L_nhR[tid], L_nhM[tid], L_bval[ci], blen);
                while (bits) {
                    const uint32_t hb = 63u - (uint32_t)__builtin_clzll(bits);
                    bits &= ~(1ull << hb);
                    atomicAdd(&L_pos[blen - 1u - (hb >> 1)], 1u);
                }
                // the counter's tag step: w = the line from tagoff[row] on
                const uint64_t at = L_nhAt[tid];
                uint64_t ws = at + off;
                // (an offset behind the barcode entry -- the C-ABI takes one -- may lie behind the line's end: then w is empty)
                for (uint64_t g = at + min(blen, L_nhLen[tid]); g < at + off; g++)
                    if (g >= p.nbytes || p.buf[g] == 0x0Au || p.buf[g] == 0x0Du) { ws = g; break; }
                tdr::Window W;
                tdr::rescue_window(kp, ws, W);
                if (ws != at + off) W.avail = 0;
                if (p.P <= W.avail && !tdr::part_bits(W.m[0], W.m[1], W.m[2], W.m[3], 0, p.P)) {
                    const uint64_t key = tdr::part_bits(W.w[0], W.w[1], W.w[2], W.w[3], 0, p.P);
                    uint32_t slot = dir_hash(key) & p.dir_mask, start = 0, run = 0;
                    for (uint32_t n = 0; n <= p.max_probe; n++) {
                        const uint4 sl = p.dir[slot];
                        if (sl.w == 0) break;
                        if (sl.x == (uint32_t)key && sl.y == (uint32_t)(key >> 32)) { start = sl.z; run = sl.w; break; }
                        slot = (slot + 1u) & p.dir_mask;
                    }
                    for (uint32_t r = 0; r < run; r++) {
                        const uint32_t tg = p.ent[start + r];
                        const uint32_t n = p.taglen[tg];
                        if (n > W.avail) continue;
                        const uint4 a = p.tagw[2ull * tg];
                        uint64_t dif = tdr::diff_bits(W.w[0], ((uint64_t)a.y << 32) | a.x, W.m[0], n, 0) |
                                       tdr::diff_bits(W.w[1], ((uint64_t)a.w << 32) | a.z, W.m[1], n, 1);
                        if (n > 64u) {
                            const uint4 b = p.tagw[2ull * tg + 1];
                            dif |= tdr::diff_bits(W.w[2], ((uint64_t)b.y << 32) | b.x, W.m[2], n, 2) |
                                   tdr::diff_bits(W.w[3], ((uint64_t)b.w << 32) | b.z, W.m[3], n, 3);
                        }
                        if (dif == 0) {                                              // (the tags are prefix-free: no other one matches)
                            atomicAdd(p.matrix + (uint64_t)row * p.ntags + tg, 1u);
                            st_tagged++;
                            break;
                        }
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
                        if ((line & 3) == 1 && line <= p.limit_line) atomicOr(p.bs + BS_ERR, ERR_NONASCII);
                    }
                    seen += (m >> q) & 1u;
                }
            }
        }
        // the tile's share of the position histogram (a tile holds fewer than 2^13 reads: no cell wraps)
        __syncthreads();
        if (tid < (int)ENTRY_BASES) {
            const uint32_t v = L_pos[tid];
            if (v) { L_pos[tid] = 0; atomicAdd(p.positions + tid, (unsigned long long)v); }
        }
    }
    const unsigned long long sums[7] = {wave_sum64(st_reads), wave_sum64(st_exact), wave_sum64(st_r1), wave_sum64(st_r2),
                                        wave_sum64(st_ambig), wave_sum64(st_none), wave_sum64(st_tagged)};
    if (lane == 0) {
        const int at[7] = {BS_READS, BS_EXACT, BS_RESC1, BS_RESC2, BS_AMBIG, BS_NONE, BS_TAGGED};
#pragma unroll
        for (int k = 0; k < 7; k++) if (sums[k]) atomicAdd(p.bs + at[k], sums[k]);
    }
}

}  // namespace tdb

// ============================================================================ host side
namespace {

// The share of a workgroup's LDS that the barcode index and the entry list take together: with the kernel's own 19 KiB
// the workgroup stays inside 64 KiB.  An index of ne blob entries and n distinct ones takes
// 16-byte-rounded(8 ne + 8-byte-rounded(4 ne) + 2048) + 2 n bytes.
constexpr size_t BCRESCUE_LDS_INDEX = 40 * 1024;

struct BcRescue : tdi::StreamPass {
    uint32_t barnum = 0, ntags = 0, K = 0, P = 0;
    uint32_t dir_mask = 0, max_probe = 0, n_order = 0, off_order = 0, min_dist = 0;   // (d_bblob: the barcode index blob | order)
    tdi::DevBuf<uint32_t> d_taglen, d_ent, d_matrix;
    tdi::DevBuf<uint4> d_tagw, d_dir;
    tdi::DevBuf<unsigned long long> d_words;  // row_rescued[barnum][2] | positions[32] | BS_*
    size_t cells() const { return (size_t)barnum * ntags; }
    unsigned long long *d_rows() const { return d_words.p; }
    unsigned long long *d_pos() const { return d_words.p + 2ull * barnum; }
    unsigned long long *d_bs() const { return d_pos() + tdb::ENTRY_BASES; }
    size_t nwords() const { return 2ull * barnum + tdb::ENTRY_BASES + tdb::BS_NWORDS; }

    int zero(hipStream_t s) override {
        TD_HIPCHK(hipMemsetAsync(d_matrix.p, 0, std::max<size_t>(cells(), 1) * 4, s));
        TD_HIPCHK(hipMemsetAsync(d_words.p, 0, nwords() * 8, s));
        return TD_OK;
    }

    int launch(const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, hipStream_t stream,
               const unsigned long long *cursor_in, unsigned long long *cursor_out) override {
        tdb::BcParams p{};
        const int rc = prologue(d_fastq, nbytes, max_reads, stream, d_bs() + tdb::BS_TOTAL, p.prefix, p.ntiles);
        if (rc || !p.ntiles) return rc;
        p.buf = (const uint8_t *)d_fastq; p.nbytes = nbytes; p.first_line = first_line;
        p.limit_line = limit_line(max_reads);
        p.bblob = d_bblob.p; p.bblob_bytes = bblob_bytes; p.off_bmeta = off_bmeta; p.off_bdir = off_bdir; p.off_order = off_order; p.n_order = n_order;
        p.tagw = d_tagw.p; p.taglen = d_taglen.p; p.dir = d_dir.p; p.ent = d_ent.p;
        p.ntags = ntags; p.P = P; p.K = K; p.dir_mask = dir_mask; p.max_probe = max_probe;
        p.matrix = d_matrix.p; p.row_rescued = d_rows(); p.positions = d_pos(); p.bs = d_bs();
        p.cursor_in = cursor_in; p.cursor_out = cursor_out;
        hipLaunchKernelGGL(tdb::k_bcrescue, dim3(grid(p.ntiles, 4, true)), dim3(tdk::BLOCK), bblob_bytes, stream, p);
        TD_HIPCHK(hipGetLastError());
        return TD_OK;
    }

    // after a synchronisation: what the kernel flagged
    int sync_stats(unsigned long long bs[tdb::BS_NWORDS]) { return sync_words(bs, d_bs(), tdb::BS_NWORDS, tdb::BS_ERR); }
};

BcRescue *bcrescue_of(td_handle *h) { return tdi::state_of<BcRescue>(h, tdi::BCRESCUE); }

// What td_bcrescue_begin builds on the host.  No HIP in here.
struct BcIndex {
    std::vector<uint16_t> order;              // blob positions of the distinct entries, in list order
    uint32_t min_dist = 64;
    uint32_t P = 0, dir_slots = 0, max_probe = 0;
    std::vector<uint64_t> words;              // [ntags][4]
    std::vector<uint32_t> lens, ent;          // [ntags]
    std::vector<uint32_t> dir;                // [dir_slots][4]
};

uint64_t pack32(const std::string &s) {
    uint64_t v = 0;
    for (size_t q = 0; q < s.size() && q < 32; q++) {
        const char c = s[q];
        v |= (uint64_t)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'T' ? 2 : 3) << (62 - 2 * q);          // (byte >> 1) & 3, as convert_chunk packs a read
    }
    return v;
}

// the entries the index build left, from the blob: the length condition, their list order
int bcrescue_entries(const std::vector<uint8_t> &blob, uint32_t off_bmeta, const char *const *barcut, uint32_t n_barcut, uint32_t K, BcIndex &ix) {
    const uint32_t ne = off_bmeta / 8;
    const uint64_t *bval = reinterpret_cast<const uint64_t *>(blob.data());
    const uint32_t *bmeta = reinterpret_cast<const uint32_t *>(blob.data() + off_bmeta);
    std::map<std::pair<uint32_t, uint64_t>, uint32_t> first_at;          // (length, bases) -> the first list position that holds them
    for (uint32_t k = 0; k < n_barcut; k++) {
        const std::string s = barcut[k];
        if (s.size() <= 32) first_at.emplace(std::make_pair((uint32_t)s.size(), pack32(s)), k);
    }
    std::map<uint32_t, uint32_t> by_rank;                                  // list position -> blob position (the first of an entry's copies)
    for (uint32_t ci = 0; ci < ne; ci++) {
        const uint32_t L = bmeta[ci] & 63u;
        if (L <= 2 * K) {
            td_set_bad_index(bmeta[ci] >> 16);
            return td_fail_internal(TD_E_LIMIT, ("barcode rescue: entry of " + std::to_string(L) + " bases leaves no room for " + std::to_string(K) +
                                                 " mismatches (every entry must be longer than " + std::to_string(2 * K) + ")").c_str());
        }
        const auto it = first_at.find(std::make_pair(L, bval[ci]));
        if (it == first_at.end()) return td_fail_internal(TD_E_INTERNAL, "barcode rescue: an index entry that is not in the list");
        by_rank.emplace(it->second, ci);
    }
    for (const auto &kv : by_rank) ix.order.push_back((uint16_t)kv.second);
    return TD_OK;
}

// the smallest distance between two entries of different rows, over the shorter one's length (64: no two rows)
void bcrescue_min_distance(const std::vector<uint8_t> &blob, uint32_t off_bmeta, BcIndex &ix) {
    const uint64_t *bval = reinterpret_cast<const uint64_t *>(blob.data());
    const uint32_t *bmeta = reinterpret_cast<const uint32_t *>(blob.data() + off_bmeta);
    const size_t n = ix.order.size();
    for (size_t i = 0; i < n; i++)
        for (size_t j = i + 1; j < n; j++) {
            const uint32_t a = bmeta[ix.order[i]], b = bmeta[ix.order[j]];
            if ((a >> 16) == (b >> 16)) continue;
            const uint32_t L = std::min(a & 63u, b & 63u);
            ix.min_dist = std::min(ix.min_dist, (uint32_t)__builtin_popcountll(tdb::entry_diff(bval[ix.order[i]], 0, bval[ix.order[j]], L)));
        }
}

void bcrescue_tag_index(const std::vector<std::string> &ts, BcIndex &ix) {
    const uint32_t n = (uint32_t)ts.size();
    size_t minlen = ts[0].size();
    for (auto &t : ts) minlen = std::min(minlen, t.size());
    ix.P = (uint32_t)std::min<size_t>(32, minlen);
    ix.words.assign((size_t)n * 4, 0);
    ix.lens.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        ix.lens[i] = (uint32_t)ts[i].size();
        for (size_t q = 0; q < ts[i].size(); q += 32) ix.words[(size_t)i * 4 + (q >> 5)] = pack32(ts[i].substr(q, 32));
    }
    ix.dir_slots = 16;
    while (ix.dir_slots < 2ull * n) ix.dir_slots <<= 1;
    ix.ent.resize(n);
    ix.dir.assign((size_t)ix.dir_slots * 4, 0);
    std::vector<std::pair<uint64_t, uint32_t>> keyed(n);
    for (uint32_t i = 0; i < n; i++) keyed[i] = {ix.words[(size_t)i * 4] >> (64u - 2u * ix.P), i};
    std::sort(keyed.begin(), keyed.end());
    for (uint32_t i = 0; i < n;) {
        uint32_t j = i;
        while (j < n && keyed[j].first == keyed[i].first) { ix.ent[j] = keyed[j].second; j++; }
        uint32_t slot = tdb::dir_hash(keyed[i].first) & (ix.dir_slots - 1), hops = 0;
        while (ix.dir[slot * 4 + 3]) { slot = (slot + 1) & (ix.dir_slots - 1); hops++; }
        ix.dir[slot * 4] = (uint32_t)keyed[i].first; ix.dir[slot * 4 + 1] = (uint32_t)(keyed[i].first >> 32);
        ix.dir[slot * 4 + 2] = i; ix.dir[slot * 4 + 3] = j - i;
        ix.max_probe = std::max(ix.max_probe, hops);
        i = j;
    }
}

}  // namespace

extern "C" {

int td_bcrescue_begin(td_handle *h, const char *const *barcut, uint32_t n_barcut, uint32_t barnum, const uint32_t *tagoff,
                      const char *const *tags, uint32_t n_tags, uint32_t max_mismatch) {
    if (!h || !barcut || !tagoff || !tags) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (max_mismatch < 1 || max_mismatch > 2) return td_fail_internal(TD_E_ARG, "max_mismatch must be 1 or 2");
    int rc = tdi::quiet_reset(h, tdi::BCRESCUE); if (rc) return rc;
    std::unique_ptr<BcRescue> r(new BcRescue());
    r->h = h;
    std::vector<uint8_t> blob;
    rc = td_barcut_blob(barcut, n_barcut, barnum, tagoff, blob, &r->off_bmeta, &r->off_bdir); if (rc) return rc;
    std::vector<std::string> ts;
    rc = rescue_check_tags(tags, n_tags, ts); if (rc) return rc;
    BcIndex ix;
    rc = bcrescue_entries(blob, r->off_bmeta, barcut, n_barcut, max_mismatch, ix); if (rc) return rc;
    if (blob.size() + 2 * ix.order.size() > BCRESCUE_LDS_INDEX) return td_fail_internal(TD_E_LIMIT, "barcode index does not fit the LDS budget");
    bcrescue_min_distance(blob, r->off_bmeta, ix);
    bcrescue_tag_index(ts, ix);
    if ((uint64_t)barnum * n_tags >= (1ull << 32)) return td_fail_internal(TD_E_LIMIT, "barcode rescue matrix beyond 2^32 cells");

    r->barnum = barnum; r->ntags = n_tags; r->K = max_mismatch; r->P = ix.P;
    r->dir_mask = ix.dir_slots - 1; r->max_probe = ix.max_probe; r->min_dist = ix.min_dist;
    r->n_order = (uint32_t)ix.order.size(); r->off_order = (uint32_t)blob.size();
    blob.resize((blob.size() + 2 * ix.order.size() + 15) / 16 * 16, 0);
    memcpy(blob.data() + r->off_order, ix.order.data(), 2 * ix.order.size());
    rc = r->upload(blob); if (rc) return rc;
    hipError_t e = r->d_tagw.alloc(ix.words.size() / 2);
    if (e == hipSuccess) e = hipMemcpy(r->d_tagw.p, ix.words.data(), ix.words.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = r->d_taglen.alloc(ix.lens.size());
    if (e == hipSuccess) e = hipMemcpy(r->d_taglen.p, ix.lens.data(), ix.lens.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = r->d_ent.alloc(ix.ent.size());
    if (e == hipSuccess) e = hipMemcpy(r->d_ent.p, ix.ent.data(), ix.ent.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = r->d_dir.alloc(ix.dir.size() / 4);
    if (e == hipSuccess) e = hipMemcpy(r->d_dir.p, ix.dir.data(), ix.dir.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = r->d_matrix.alloc(r->cells());
    if (e == hipSuccess) e = r->d_words.alloc(r->nwords());
    if (e != hipSuccess) return tdi::StreamPass::hip_failed(e);
    return tdi::install(r, tdi::BCRESCUE);
}

int td_bcrescue_device(td_handle *h, const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, void *stream) {
    BcRescue *r = bcrescue_of(h);
    if (!r) return tdi::no_state("bcrescue", h);
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    return r->launch(d_fastq, nbytes, first_line, max_reads, (hipStream_t)stream, nullptr, nullptr);
}

int td_bcrescue_file(td_handle *h, const char *path, uint64_t max_reads) {
    BcRescue *r = bcrescue_of(h);
    if (!r || !path) return tdi::no_state("bcrescue", h && path);
    unsigned long long bs[tdb::BS_NWORDS];
    const int rc = r->file(path, max_reads);
    return rc ? rc : r->sync_stats(bs);
}

int td_bcrescue_stats(td_handle *h, uint64_t out[8]) {
    BcRescue *r = bcrescue_of(h);
    if (!r || !out) return tdi::no_state("bcrescue", h && out);
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    unsigned long long bs[tdb::BS_NWORDS];
    const int rc = r->sync_stats(bs); if (rc) return rc;
    out[TD_BCRESCUE_READS] = bs[tdb::BS_READS]; out[TD_BCRESCUE_EXACT] = bs[tdb::BS_EXACT]; out[TD_BCRESCUE_RESCUED1] = bs[tdb::BS_RESC1];
    out[TD_BCRESCUE_RESCUED2] = bs[tdb::BS_RESC2]; out[TD_BCRESCUE_AMBIGUOUS] = bs[tdb::BS_AMBIG]; out[TD_BCRESCUE_NONE] = bs[tdb::BS_NONE];
    out[TD_BCRESCUE_TAGGED] = bs[tdb::BS_TAGGED]; out[TD_BCRESCUE_MIN_ENTRY_DISTANCE] = r->min_dist;
    return TD_OK;
}

int td_bcrescue_fetch(td_handle *h, uint32_t *matrix_out, uint64_t *row_rescued_out, uint64_t *positions_out) {
    BcRescue *r = bcrescue_of(h);
    if (!r) return tdi::no_state("bcrescue", h);
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    unsigned long long bs[tdb::BS_NWORDS];
    const int rc = r->sync_stats(bs); if (rc) return rc;
    if (matrix_out && r->cells()) TD_HIPCHK(hipMemcpy(matrix_out, r->d_matrix.p, r->cells() * 4, hipMemcpyDeviceToHost));
    if (row_rescued_out && r->barnum) TD_HIPCHK(hipMemcpy(row_rescued_out, r->d_rows(), 2ull * r->barnum * 8, hipMemcpyDeviceToHost));
    if (positions_out) TD_HIPCHK(hipMemcpy(positions_out, r->d_pos(), tdb::ENTRY_BASES * 8, hipMemcpyDeviceToHost));
    return TD_OK;
}

int td_bcrescue_matrix(td_handle *h, void **d_matrix) {
    BcRescue *r = bcrescue_of(h);
    if (!r || !d_matrix) return tdi::no_state("bcrescue", h && d_matrix);
    if (r->dead) return r->answer_dead();
    *d_matrix = r->d_matrix.p;
    return TD_OK;
}

int td_bcrescue_end(td_handle *h) {
    if (!h) return td_fail_internal(TD_E_ARG, "handle is NULL");
    if (!bcrescue_of(h)) return tdi::no_state("bcrescue", true);
    return tdi::quiet_reset(h, tdi::BCRESCUE);
}

}  // extern "C"
