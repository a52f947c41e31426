// Library QC: per-barcode read counts and per-cycle base and quality histograms of one library, in one
// streaming pass over ALL bytes of its sequence and quality lines.  Lines are the counter's (text mode's universal
// newlines); record r is lines 4r .. 4r + 3 and records r >= R are not looked at; every line is decided on its own.
//
//   sequence line   strip (the counter's set), upper-case; n = its length; the barcode row b by barcode_lookup
//                   (kernels.hpp, on the index td_set_index's rules build), b = B without a hit;
//                   barcode[b] += {1, n, any non-ACGT}; length[min(n, C)] += 1; base_cycle[min(i, C)][class] += 1
//   quality line    strip; qual_cycle[min(i, C)][v - 33 | 94] += 1; meanq[qsum / nvalid] += 1 or empty_qual += 1
//
//   k_qc   persistent workgroups over 16 KiB tiles (td_line_prefix gives every tile its line index, as for k_census):
//          terminator masks -> every lane holds the line starts of its own 64 bytes -> the sixteen lanes of a
//          quarter-wave take one line at a time from their own 1 KiB: 16-byte loads, the line's end and its
//          stripped extent by reductions inside the quarter-wave, then the bytes staged in LDS so that lane = position
//          and every byte is one LDS atomic on the cell (cycle, symbol).  The tables of the first QC_WIN cycles live in
//          LDS as 32-bit cells with odd row strides (95 and 7 dwords): sixteen lanes at consecutive cycles with equal
//          symbols hit sixteen banks.  Beyond the window: cycles QC_WIN .. C - 1 by 64-bit atomics on device memory,
//          the overflow row C through a small table per wave, which that wave alone merges.
//
// No cell wraps: a line adds at most 1 to a cell of the window tables (one position, one symbol), a tile starts at most
// TILE / 4 + 2 lines of one kind, and the workgroup merges after flush_tiles <= 2^20 tiles (4098 * 2^20 < 2^32); the
// per-wave overflow cells take at most 1024 per step of 1 KiB and are merged after 2^20 steps at the latest, inside
// a line if need be; the per-barcode rows are 64-bit.  A merge adds the non-zero cells to the 64-bit tables in device
// memory and zeroes them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>

#define TD_INST_ONLY                    // (k_scan_tiles is defined in tagdig.hip's translation unit)
#include "stream_pass.hpp"

namespace tdq {
using namespace tdk;

constexpr int CPT = 4;                                   // 16-byte chunks per thread: tiles of 16 KiB, as k_count_lines<4> counts them
constexpr uint32_t TILE = CPT * BLOCK * 16u;
static_assert(TILE == tdi::STREAM_TILE, "td_line_prefix (tagdig.hip) counts terminators per 16 KiB tile with k_count_lines<4>");
constexpr uint32_t QC_WIN = 152;                         // cycles whose tables live in LDS, at most (two workgroups per CU)
constexpr uint32_t QC_WIN_MIN = 100;                     // ... and at least, when the index and the barcode rows are large (then one workgroup per CU)
constexpr uint32_t QC_LDS_HALF = 80 * 1024;              // what a workgroup may take for two to fit a CU
constexpr uint32_t NQ = 95, NBASE = 6, NMEAN = 94;       // symbols of a quality row (94 Phred values + invalid), of a base row, mean bins
constexpr uint32_t QROW = 95, BROW = 7;                  // their row strides in LDS, in dwords: odd
constexpr uint32_t BAR_LDS_ROWS = 512;                   // per-barcode rows kept in LDS when B + 1 <= this (64-bit cells)
constexpr uint32_t OVF_CELLS = 8 + NQ + 1;               // a wave's overflow row: base classes at 0, quality symbols at 8
constexpr uint32_t OVF_STEPS = 1u << 20;                 // ... merged after this many steps of 1 KiB at the latest
constexpr uint32_t NONE16 = 0xFFFFu;
// the QC's words in device memory
enum { QS_READS = 0, QS_BARCUT = 1, QS_QLINES = 2, QS_BASES = 3, QS_QBASES = 4, QS_QINVALID = 5, QS_EMPTYQ = 6, QS_ERR = 7, QS_TOTAL = 8, QS_NWORDS = 16 };

struct QcParams {
    const uint8_t *buf;
    uint64_t nbytes;
    uint64_t first_line;       // global index of the buffer's first line (+ *cursor_in)
    uint64_t max_records;      // R: records below it are looked at
    const uint64_t *prefix;    // [ntiles] FLAG_INC | terminators up to the end of tile t
    uint32_t ntiles;
    const uint32_t *bblob;     // barcode + cut site index (the counting path's layout)
    uint32_t bblob_bytes, off_bmeta, off_bdir;
    uint32_t nbar;             // B
    uint32_t C;                // max_cycles
    uint32_t win;              // cycles whose tables live in LDS (<= C)
    uint32_t bar_lds;          // the per-barcode rows are kept in LDS
    uint32_t flush_tiles;      // tiles between two merges of a workgroup's tables
    unsigned long long *g_bar, *g_base, *g_qual, *g_len, *g_meanq;      // (B+1) x 3, (C+1) x 6, (C+1) x 95, C+1, 94
    unsigned long long *qs;    // QS_*
    const unsigned long long *cursor_in;
    unsigned long long *cursor_out;
};

// what a workgroup keeps in LDS behind the index: [mask 2 KiB][stage 4 x 1 KiB][overflow 4 x OVF_CELLS][qual win x 95 |
// base win x 7 | length win | meanq 96][barcode rows (B+1) x 3 x 8 bytes]
__host__ __device__ inline uint32_t qc_cells(uint32_t win) { return (win * (QROW + BROW + 1u) + 96u + 1u) & ~1u; }   // (even: the 64-bit rows follow)
__host__ __device__ inline uint32_t qc_lds_bytes(uint32_t blob_bytes, uint32_t win, uint32_t nbar, bool bar_lds) {
    return blob_bytes + CPT * BLOCK * 2u + (BLOCK / 64) * 1024u + (BLOCK / 64) * OVF_CELLS * 4u + qc_cells(win) * 4u + (bar_lds ? (nbar + 1u) * 24u : 0u);
}

__device__ __forceinline__ uint32_t row_min(uint32_t v) {            // over the sixteen lanes of a row: row_ror 1, 2, 4, 8
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false));
    return v;
}
__device__ __forceinline__ uint32_t row_max(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false));
    return v;
}
__device__ __forceinline__ uint64_t row_sum64(uint64_t v) {
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d, 16);
    return v;
}
__device__ __forceinline__ uint64_t row_or64(uint64_t v) {
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 16);
    return v;
}
// bit k = byte k of the chunk is <= 0x20: every blank and every terminator is, and hardly anything else in a FASTQ file
__device__ __forceinline__ uint32_t low_bytes(uint32_t x) {
    const uint32_t t = (((x & 0x7F7F7F7Fu) + 0x5F5F5F5Fu) | x) & 0x80808080u;
    return (~t & 0x80808080u) >> 7;
}
__device__ __forceinline__ uint32_t low_mask16(const uint4 &v) {
    uint32_t lo = udot4(low_bytes(v.x), 0x08040201u, 0u);
    lo = udot4(low_bytes(v.y), 0x80402010u, lo);
    uint32_t hi = udot4(low_bytes(v.z), 0x08040201u, 0u);
    hi = udot4(low_bytes(v.w), 0x80402010u, hi);
    return lo | (hi << 8);
}
__device__ __forceinline__ uint32_t blank_mask16(const uint4 &v) {    // (rare: only chunks with a byte <= 0x20 inside a line)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) m |= is_blank((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) ? 1u << k : 0u;
    return m;
}

__global__ __launch_bounds__(BLOCK) void k_qc(const QcParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t L_misc[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = lane & 15, grp = (lane >> 4) & 3;
    const unsigned long long *L_bval = reinterpret_cast<const unsigned long long *>(lds);
    const uint32_t *L_bmeta = reinterpret_cast<const uint32_t *>(lds + p.off_bmeta);
    const uint16_t *L_bdir = reinterpret_cast<const uint16_t *>(lds + p.off_bdir);
    uint16_t *L_mask = reinterpret_cast<uint16_t *>(lds + p.bblob_bytes);
    uint8_t *L_stage = lds + p.bblob_bytes + CPT * BLOCK * 2u;
    uint32_t *L_ovf_all = reinterpret_cast<uint32_t *>(L_stage + (BLOCK / 64) * 1024u);
    uint32_t *L_cells = L_ovf_all + (BLOCK / 64) * OVF_CELLS;
    const uint32_t win = p.win, ncells = qc_cells(win);
    uint32_t *L_qual = L_cells, *L_base = L_cells + win * QROW, *L_len = L_base + win * BROW, *L_meanq = L_len + win;
    unsigned long long *L_bar = reinterpret_cast<unsigned long long *>(L_cells + ncells);      // (8-byte aligned: every part before it is a multiple of 8)
    uint8_t *stg = L_stage + wave * 1024 + grp * 256;
    uint32_t *L_ovf = L_ovf_all + wave * OVF_CELLS;
    const uint32_t nbarcells = p.bar_lds ? (p.nbar + 1u) * 3u : 0u;

    for (uint32_t i = tid; i < p.bblob_bytes / 4; i += BLOCK) reinterpret_cast<uint32_t *>(lds)[i] = p.bblob[i];
    for (uint32_t i = tid; i < (BLOCK / 64) * OVF_CELLS + ncells; i += BLOCK) L_ovf_all[i] = 0;
    for (uint32_t i = tid; i < nbarcells; i += BLOCK) L_bar[i] = 0;
    KParams kp{};
    kp.buf = p.buf; kp.nbytes = p.nbytes;
    const unsigned long long cin = p.cursor_in ? *p.cursor_in : 0ull;
    const uint64_t fl = p.first_line + cin;
    if (blockIdx.x == 0 && tid == 0 && p.cursor_out) *p.cursor_out = cin + p.qs[QS_TOTAL];
    unsigned long long st_reads = 0, st_bar = 0, st_qlines = 0, st_bases = 0, st_qbases = 0, st_qinv = 0, st_empty = 0;
    uint32_t since = 0, ovf_steps = 0;
    const uint32_t C = p.C;

    // a wave's overflow row -> row C of the tables in device memory
    auto merge_overflow = [&]() {
        wave_lds_fence();
        for (uint32_t c = lane; c < OVF_CELLS; c += 64) {
            const uint32_t v = L_ovf[c];
            if (v) {
                L_ovf[c] = 0;
                if (c < NBASE) atomicAdd(p.g_base + (uint64_t)C * NBASE + c, (unsigned long long)v);
                else if (c >= 8 && c < 8 + NQ) atomicAdd(p.g_qual + (uint64_t)C * NQ + (c - 8), (unsigned long long)v);
            }
        }
        wave_lds_fence();
        ovf_steps = 0;
    };
    // the workgroup's tables -> device memory (the window rows have the same index there; base rows are 6 wide there)
    auto merge_tables = [&]() {
        __syncthreads();
        for (uint32_t c = tid; c < ncells; c += BLOCK) {
            const uint32_t v = L_cells[c];
            if (!v) continue;
            L_cells[c] = 0;
            unsigned long long *dst;
            if (c < win * QROW) dst = p.g_qual + c;
            else if (c < win * (QROW + BROW)) { const uint32_t c2 = c - win * QROW; dst = p.g_base + (c2 / BROW) * NBASE + c2 % BROW; }
            else if (c < win * (QROW + BROW + 1u)) dst = p.g_len + (c - win * (QROW + BROW));
            else if (c - win * (QROW + BROW + 1u) < NMEAN) dst = p.g_meanq + (c - win * (QROW + BROW + 1u));
            else continue;                               // (padding: never added to)
            atomicAdd(dst, (unsigned long long)v);
        }
        for (uint32_t c = tid; c < nbarcells; c += BLOCK) {
            const unsigned long long v = L_bar[c];
            if (v) { L_bar[c] = 0; atomicAdd(p.g_bar + c, v); }
        }
        __syncthreads();
        since = 0;
    };

    for (uint32_t t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const uint64_t tbase = (uint64_t)t * TILE;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            const uint32_t c = j * BLOCK + tid;
            const uint64_t g = tbase + (uint64_t)c * 16u;
            const uint4 v = load_chunk(kp, g);
            uint32_t nl = eq_mask16(v, 0x0A0A0A0Au), cr = eq_mask16(v, 0x0D0D0D0Du);
            uint32_t term = nl | (cr & ~(nl >> 1));
            if (cr & 0x8000u) { const uint64_t nx = g + 16; if (nx < p.nbytes && p.buf[nx] == 0x0A) term &= 0x7FFFu; }
            if (g + 16 > p.nbytes) term &= g < p.nbytes ? ((1u << (uint32_t)(p.nbytes - g)) - 1u) : 0u;
            L_mask[c] = (uint16_t)term;
        }
        __syncthreads();
        const uint32_t m_lo = reinterpret_cast<const uint32_t *>(L_mask)[tid * 2], m_hi = reinterpret_cast<const uint32_t *>(L_mask)[tid * 2 + 1];
        const uint64_t m0 = (uint64_t)m_lo | ((uint64_t)m_hi << 32);          // the terminators of this thread's 64 bytes
        const uint32_t cnt = __builtin_popcountll(m0);
        const uint32_t incl = wave_incl_scan(cnt, lane);
        if (lane == 63) L_misc[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0;
        for (int w = 0; w < wave; w++) wbase += L_misc[w];
        // terminators before this tile: the previous tile's inclusive prefix.  The line behind the buffer's j-th
        // terminator has index fl + j
        const uint64_t P = t ? (p.prefix[t - 1] & ~FLAG_INC) : 0ull;
        const uint64_t ord0 = P + wbase + incl - cnt;                         // terminators before this thread's span
        const uint32_t span0 = tid * CPT * 16u;

        // ---------------- sequence lines (line index = 1 mod 4), then quality lines (3 mod 4): the per-byte code is uniform
        for (uint32_t phase = 1; phase <= 3u; phase += 2) {
            uint64_t m = m0, ord = ord0;
            // the buffer's own first line has no terminator before it
            bool first_pending = t == 0 && tid == 0 && (fl & 3) == phase && (fl >> 2) < p.max_records && p.nbytes > 0;
            // drop the terminators at the head of m that no wanted line follows
            auto advance = [&]() {
                while (m) {
                    const uint64_t line = fl + ord + 1;
                    if ((line & 3) == phase && (line >> 2) < p.max_records && tbase + span0 + (uint32_t)__builtin_ctzll(m) + 1u < p.nbytes) break;
                    m &= m - 1; ord++;
                }
            };
            advance();
            for (;;) {
                const bool have = first_pending || m != 0;
                const uint64_t bal = __ballot(have);
                if (!bal) break;
                const uint32_t gb = (uint32_t)(bal >> (lane & 48)) & 0xFFFFu;
                const bool gact = gb != 0;                                   // this quarter-wave has a line
                const int src = (lane & 48) + (gact ? __builtin_ctz(gb) : 0);
                const uint32_t cpos = first_pending ? 0u : m ? span0 + (uint32_t)__builtin_ctzll(m) + 1u : 0u;
                const uint32_t pos = __shfl(cpos, src, 64);
                if (gact && lane == src) {
                    if (first_pending) first_pending = false;
                    else { m &= m - 1; ord++; advance(); }
                }
                const uint64_t gpos = tbase + pos;
                const uint64_t cbase = gpos & ~15ull;

                // ---- pass A: where the line ends, and what strip leaves of it: [s, e)
                uint64_t s = ~0ull, e = 0;
                bool open = gact;                                            // its terminator has not been seen
                uint4 v0 = make_uint4(0u, 0u, 0u, 0u);
                for (uint32_t step = 0;; step++) {
                    if (!__any(open)) break;
                    const uint64_t sbase = cbase + (uint64_t)step * 256u;
                    const uint64_t g = sbase + (uint32_t)sub * 16u;
                    uint4 v = make_uint4(0u, 0u, 0u, 0u);
                    uint32_t valid = 0;
                    if (open && g < p.nbytes) {
                        v = load_chunk(kp, g);
                        valid = g + 16 <= p.nbytes ? 0xFFFFu : (1u << (uint32_t)(p.nbytes - g)) - 1u;
                        if (g < gpos) valid &= 0xFFFFu << (uint32_t)(gpos - g);          // (the line's first chunk only)
                    }
                    if (step == 0) v0 = v;
                    const uint32_t term = (eq_mask16(v, 0x0A0A0A0Au) | eq_mask16(v, 0x0D0D0D0Du)) & valid;
                    const uint32_t endrel = row_min(term ? (uint32_t)sub * 16u + (uint32_t)__builtin_ctz(term) : NONE16);
                    const uint32_t lim = endrel > (uint32_t)sub * 16u ? std::min(endrel - (uint32_t)sub * 16u, 16u) : 0u;
                    uint32_t body = valid & ((1u << lim) - 1u);                         // bytes of the line in this chunk
                    if (low_mask16(v) & body) body &= ~blank_mask16(v);
                    const uint32_t firstrel = row_min(body ? (uint32_t)sub * 16u + (uint32_t)__builtin_ctz(body) : NONE16);
                    const uint32_t lastrel1 = row_max(body ? (uint32_t)sub * 16u + 32u - (uint32_t)__builtin_clz(body) : 0u);
                    if (open) {
                        if (s == ~0ull && firstrel != NONE16) s = sbase + firstrel;
                        if (lastrel1) e = sbase + lastrel1;
                        if (endrel != NONE16 || sbase + 256u >= p.nbytes) open = false;
                    }
                }
                if (s == ~0ull) { s = 0; e = 0; }
                const uint64_t n = e - s;

                // ---- pass B: the bytes of [s, e), lane = position
                uint64_t K = 0;
                uint32_t nlead = 0;
                bool f_amb = false, f_hi = false;
                unsigned long long qsum = 0, nvalid = 0;
                for (uint32_t step = 0;; step++) {
                    const uint64_t sbase = cbase + (uint64_t)step * 256u;
                    const bool act = gact && sbase < e;
                    if (!__any(act)) break;
                    const uint64_t g = sbase + (uint32_t)sub * 16u;
                    uint4 v = v0;
                    if (step) v = act && g < p.nbytes ? load_chunk(kp, g) : make_uint4(0u, 0u, 0u, 0u);
                    wave_lds_fence();
                    *reinterpret_cast<uint4 *>(stg + sub * 16) = v;
                    wave_lds_fence();
                    if (step == 0 && phase == 1u) {
                        // the first 32 bases, packed as the index packs them, and how many of them lead the line
                        uint32_t inv = 0;
#pragma unroll
                        for (uint32_t h = 0; h < 2u; h++) {
                            const uint32_t j = (uint32_t)sub + 16u * h;
                            const uint64_t a = s + j;
                            const bool inb = act && a < e;
                            uint32_t b = 0;
                            if (inb) { const uint64_t o = a - cbase; b = o < 256u ? stg[o] : p.buf[a]; }
                            if (b >= 'a' && b <= 'z') b -= 32u;
                            const bool ok = inb && (b == 'A' || b == 'C' || b == 'G' || b == 'T');
                            if (ok) K |= (uint64_t)((b >> 1) & 3u) << (62u - 2u * j);
                            inv |= ((uint32_t)(__ballot(!ok) >> (lane & 48)) & 0xFFFFu) << (16u * h);
                        }
                        K = row_or64(K);
                        nlead = inv ? (uint32_t)__builtin_ctz(inv) : 32u;
                    }
                    bool used_ovf = false;
#pragma nounroll
                    for (uint32_t k = 0; k < 16u; k++) {
                        const uint64_t a = sbase + k * 16u + (uint32_t)sub;
                        const bool in = act && a >= s && a < e;
                        if (!__any(in)) continue;
                        if (in) {
                            uint32_t b = stg[k * 16u + (uint32_t)sub];
                            const uint64_t i = a - s;
                            if (phase == 1u) {
                                if (b >= 0x80u) f_hi = true;
                                if (b >= 'a' && b <= 'z') b -= 32u;
                                const uint32_t cls = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : b == 'N' ? 4u : 5u;
                                if (cls >= 4u) f_amb = true;
                                if (i < win) atomicAdd(&L_base[(uint32_t)i * BROW + cls], 1u);
                                else if (i < C) atomicAdd(p.g_base + (uint32_t)i * NBASE + cls, 1ull);
                                else { atomicAdd(&L_ovf[cls], 1u); used_ovf = true; }
                            } else {
                                const bool okq = b >= 33u && b <= 126u;
                                const uint32_t bin = okq ? b - 33u : 94u;
                                if (okq) { qsum += bin; nvalid++; }
                                if (i < win) atomicAdd(&L_qual[(uint32_t)i * QROW + bin], 1u);
                                else if (i < C) atomicAdd(p.g_qual + (uint32_t)i * NQ + bin, 1ull);
                                else { atomicAdd(&L_ovf[8u + bin], 1u); used_ovf = true; }
                            }
                        }
                    }
                    if (__any(used_ovf) && ++ovf_steps >= OVF_STEPS) merge_overflow();
                }

                // ---- the line's own numbers, by the quarter-wave's first lane
                const uint32_t gshift = lane & 48;
                const bool any_amb = ((uint32_t)(__ballot(f_amb) >> gshift) & 0xFFFFu) != 0;
                const bool any_hi = ((uint32_t)(__ballot(f_hi) >> gshift) & 0xFFFFu) != 0;
                if (phase == 1u) {
                    if (gact && sub == 0) {
                        st_reads++; st_bases += n;
                        uint32_t meta = 0, b = p.nbar;
                        if (barcode_lookup(L_bval, L_bmeta, L_bdir, K, nlead, meta)) { b = meta >> 16; st_bar++; }
                        if (p.bar_lds) {
                            atomicAdd(&L_bar[b * 3u], 1ull);
                            if (n) atomicAdd(&L_bar[b * 3u + 1u], (unsigned long long)n);
                            if (any_amb) atomicAdd(&L_bar[b * 3u + 2u], 1ull);
                        } else {
                            atomicAdd(p.g_bar + b * 3u, 1ull);
                            if (n) atomicAdd(p.g_bar + b * 3u + 1u, (unsigned long long)n);
                            if (any_amb) atomicAdd(p.g_bar + b * 3u + 2u, 1ull);
                        }
                        if (n < win) atomicAdd(&L_len[(uint32_t)n], 1u);
                        else atomicAdd(p.g_len + (n < C ? (uint32_t)n : C), 1ull);
                        if (any_hi) atomicOr(p.qs + QS_ERR, ERR_NONASCII);
                    }
                } else {
                    const unsigned long long gq = row_sum64(qsum), gv = row_sum64(nvalid);
                    if (gact && sub == 0) {
                        st_qlines++; st_qbases += gv; st_qinv += n - gv;
                        if (gv == 0) st_empty++;
                        else {
                            const uint32_t mq = (gq >> 32) == 0 && (gv >> 32) == 0 ? (uint32_t)gq / (uint32_t)gv : (uint32_t)(gq / gv);
                            atomicAdd(&L_meanq[mq < NMEAN ? mq : NMEAN - 1u], 1u);
                        }
                    }
                }
            }
        }
        if (ovf_steps) merge_overflow();
        if (++since >= p.flush_tiles) merge_tables();
    }
    merge_tables();
    const unsigned long long r = wave_sum64(st_reads), b = wave_sum64(st_bar), q = wave_sum64(st_qlines), nb = wave_sum64(st_bases),
                             qb = wave_sum64(st_qbases), qi = wave_sum64(st_qinv), em = wave_sum64(st_empty);
    if (lane == 0) {
        if (r) atomicAdd(p.qs + QS_READS, r);
        if (b) atomicAdd(p.qs + QS_BARCUT, b);
        if (q) atomicAdd(p.qs + QS_QLINES, q);
        if (nb) atomicAdd(p.qs + QS_BASES, nb);
        if (qb) atomicAdd(p.qs + QS_QBASES, qb);
        if (qi) atomicAdd(p.qs + QS_QINVALID, qi);
        if (em) atomicAdd(p.qs + QS_EMPTYQ, em);
    }
}

}  // namespace tdq

// ============================================================================ host side
namespace {

constexpr size_t QC_LDS_INDEX = 40 * 1024;                // the barcode index's share of a workgroup's LDS, as the census's
constexpr uint32_t QC_FLUSH_DEFAULT = 4096, QC_FLUSH_MAX = 1u << 20;

struct Qc : tdi::StreamPass {
    uint32_t C = 0, nbar = 0;
    tdi::DevBuf<unsigned long long> d_all;    // QS_* | barcode rows | base_cycle | qual_cycle | length | meanq
    uint64_t file_records = 0;                // td_qc_file's bound (the readers are handed one record more)
    size_t n_bar() const { return ((size_t)nbar + 1) * 3; }
    size_t n_base() const { return ((size_t)C + 1) * tdq::NBASE; }
    size_t n_qual() const { return ((size_t)C + 1) * tdq::NQ; }
    size_t n_len() const { return (size_t)C + 1; }
    size_t words() const { return tdq::QS_NWORDS + n_bar() + n_base() + n_qual() + n_len() + tdq::NMEAN; }
    unsigned long long *d_qs() const { return d_all.p; }
    unsigned long long *d_bar() const { return d_all.p + tdq::QS_NWORDS; }
    unsigned long long *d_base() const { return d_bar() + n_bar(); }
    unsigned long long *d_qual() const { return d_base() + n_base(); }
    unsigned long long *d_len() const { return d_qual() + n_qual(); }
    unsigned long long *d_meanq() const { return d_len() + n_len(); }

    int zero(hipStream_t s) override {
        TD_HIPCHK(hipMemsetAsync(d_all.p, 0, words() * 8, s));
        return TD_OK;
    }

    // records below max_records of one buffer
    int run(const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_records, hipStream_t stream,
            const unsigned long long *cursor_in, unsigned long long *cursor_out) {
        tdq::QcParams p{};
        const int rc = prologue(d_fastq, nbytes, max_records, stream, d_qs() + tdq::QS_TOTAL, p.prefix, p.ntiles);
        if (rc || !p.ntiles) return rc;
        p.buf = (const uint8_t *)d_fastq; p.nbytes = nbytes; p.first_line = first_line;
        p.max_records = std::min<uint64_t>(max_records, 1ull << 61);
        p.bblob = d_bblob.p; p.bblob_bytes = bblob_bytes; p.off_bmeta = off_bmeta; p.off_bdir = off_bdir;
        p.nbar = nbar; p.C = C;
        p.bar_lds = nbar + 1 <= tdq::BAR_LDS_ROWS ? 1u : 0u;
        // the window: as many cycles as leave room for a second workgroup on the CU, within QC_WIN_MIN .. QC_WIN
        p.win = tdq::QC_WIN;
        while (p.win > tdq::QC_WIN_MIN && tdq::qc_lds_bytes(p.bblob_bytes, p.win, p.nbar, p.bar_lds != 0) > tdq::QC_LDS_HALF) p.win--;
        p.win = std::min(C, p.win);
        const uint32_t ft = td_handle_qc_flush_tiles(h);
        p.flush_tiles = ft ? std::min(ft, QC_FLUSH_MAX) : QC_FLUSH_DEFAULT;
        p.g_bar = d_bar(); p.g_base = d_base(); p.g_qual = d_qual(); p.g_len = d_len(); p.g_meanq = d_meanq(); p.qs = d_qs();
        p.cursor_in = cursor_in; p.cursor_out = cursor_out;
        const uint32_t lds = tdq::qc_lds_bytes(p.bblob_bytes, p.win, p.nbar, p.bar_lds != 0);
        TD_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(tdq::k_qc), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(tdq::k_qc, dim3(grid(p.ntiles, 2, true)), dim3(tdk::BLOCK), lds, stream, p);
        TD_HIPCHK(hipGetLastError());
        return TD_OK;
    }
    // a reader's piece: the readers' max_reads is one record beyond the QC's bound, so that they bring the last record's
    // quality line -- not used
    int launch(const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t, hipStream_t stream, const unsigned long long *cursor_in,
               unsigned long long *cursor_out) override {
        return run(d_fastq, nbytes, first_line, file_records, stream, cursor_in, cursor_out);
    }

    // after a synchronisation: what the kernel flagged
    int sync_stats(unsigned long long qs[tdq::QS_NWORDS]) { return sync_words(qs, d_qs(), tdq::QS_NWORDS, tdq::QS_ERR); }
};

Qc *qc_of(td_handle *h) { return tdi::state_of<Qc>(h, tdi::QC); }

}  // namespace

extern "C" {

int td_qc_begin(td_handle *h, const char *const *barcut, uint32_t n_barcut, uint32_t barnum, const uint32_t *baroff, uint32_t max_cycles) {
    if (!h || !barcut || !baroff) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (max_cycles < 1 || max_cycles > TD_QC_MAX_CYCLES) return td_fail_internal(TD_E_ARG, "max_cycles must be 1..1024");
    int rc = tdi::quiet_reset(h, tdi::QC); if (rc) return rc;
    std::unique_ptr<Qc> q(new Qc());
    rc = q->begin(h, barcut, n_barcut, barnum, baroff, QC_LDS_INDEX); if (rc) return rc;
    for (uint32_t b = 0; b < barnum; b++)
        if (baroff[b] > 32) return td_fail_internal(TD_E_LIMIT, "barcode longer than 32 bases");
    q->C = max_cycles; q->nbar = barnum;
    const hipError_t e = q->d_all.alloc(q->words());
    if (e != hipSuccess) return tdi::StreamPass::hip_failed(e);
    return tdi::install(q, tdi::QC);
}

int td_qc_device(td_handle *h, const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, void *stream) {
    Qc *q = qc_of(h);
    if (!q) return tdi::no_state("qc", h, "handle is NULL");
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    return q->run(d_fastq, nbytes, first_line, max_reads, (hipStream_t)stream, nullptr, nullptr);
}

int td_qc_file(td_handle *h, const char *path, uint64_t max_reads) {
    Qc *q = qc_of(h);
    if (!q || !path) return tdi::no_state("qc", h && path);
    if (max_reads == 0) max_reads = 1;
    q->file_records = max_reads;
    // the readers stop before the quality line of the last record they are asked for: ask for one more (saturating)
    const int rc = q->file(path, max_reads >= (1ull << 60) ? max_reads : max_reads + 1);
    unsigned long long qs[tdq::QS_NWORDS];
    return rc ? rc : q->sync_stats(qs);
}

int td_qc_stats(td_handle *h, uint64_t out[8]) {
    Qc *q = qc_of(h);
    if (!q || !out) return tdi::no_state("qc", h && out);
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    unsigned long long qs[tdq::QS_NWORDS];
    const int rc = q->sync_stats(qs); if (rc) return rc;
    out[TD_QC_READS] = qs[tdq::QS_READS]; out[TD_QC_BARCUT] = qs[tdq::QS_BARCUT]; out[TD_QC_QUAL_LINES] = qs[tdq::QS_QLINES];
    out[TD_QC_BASES] = qs[tdq::QS_BASES]; out[TD_QC_QUAL_BASES] = qs[tdq::QS_QBASES]; out[TD_QC_QUAL_INVALID] = qs[tdq::QS_QINVALID];
    out[TD_QC_EMPTY_QUAL] = qs[tdq::QS_EMPTYQ]; out[TD_QC_CYCLES] = q->C;
    return TD_OK;
}

int td_qc_fetch(td_handle *h, uint64_t *barcode_out, uint64_t *base_cycle_out, uint64_t *qual_cycle_out, uint64_t *length_out, uint64_t *meanq_out) {
    Qc *q = qc_of(h);
    if (!q) return tdi::no_state("qc", h, "handle is NULL");
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    unsigned long long qs[tdq::QS_NWORDS];
    const int rc = q->sync_stats(qs); if (rc) return rc;
    if (barcode_out) TD_HIPCHK(hipMemcpy(barcode_out, q->d_bar(), q->n_bar() * 8, hipMemcpyDeviceToHost));
    if (base_cycle_out) TD_HIPCHK(hipMemcpy(base_cycle_out, q->d_base(), q->n_base() * 8, hipMemcpyDeviceToHost));
    if (qual_cycle_out) TD_HIPCHK(hipMemcpy(qual_cycle_out, q->d_qual(), q->n_qual() * 8, hipMemcpyDeviceToHost));
    if (length_out) TD_HIPCHK(hipMemcpy(length_out, q->d_len(), q->n_len() * 8, hipMemcpyDeviceToHost));
    if (meanq_out) TD_HIPCHK(hipMemcpy(meanq_out, q->d_meanq(), tdq::NMEAN * 8, hipMemcpyDeviceToHost));
    return TD_OK;
}

int td_qc_end(td_handle *h) {
    if (!h) return td_fail_internal(TD_E_ARG, "handle is NULL");
    return tdi::quiet_reset(h, tdi::QC);
}

}  // extern "C"
