// exp_frag_size on the GPU (include/tagdig.h: td_fasta_frame_device, td_frag_search_device, td_frag_gather_device).
//
// K1 k_fasta_summary / k_fasta_scan / k_fasta_emit: the genome reading of the reference's exp_frag_size.py
//    (:152-189): text-mode lines (universal newlines: \n, \r\n and a lone \r end a line), a line starting with '>' is a
//    header, every other line contributes line.strip().upper().  A byte is kept iff its line is no header, it is no line
//    terminator, and its line holds a non-whitespace byte at or before it AND one at or after it.  Everything that
//    crosses tiles is two tiny monoids:
//      forward  (st, hdr, nw): "a line starts in this stretch", the open line's header flag, "non-whitespace seen in
//               the open line" (or, when no line starts, "any non-whitespace in the stretch");
//      backward (tm, nw): "a terminator in this stretch", "non-whitespace before the first terminator" (or in the
//               whole stretch when there is none).
//    Line starts are local (the byte before says it), so nothing else crosses a seam -- \r\n split over two tiles
//    included.  k_fasta_summary folds each 32 KiB tile into both elements, its header count and six kept-byte counters
//    (one per way the two unknown carries can decide a byte); k_fasta_scan (one workgroup) scans the tiles' elements
//    both ways and the counts; k_fasta_emit runs the tile again with its carries known, stages the kept bytes in LDS
//    and writes them with 16-byte stores, and writes one record row per header line.
// K2 k_frag_search: one wave per (tag, record) search; the window (<= 3 072 bytes) is copied into LDS in the
//    orientation the reference searches (reverse strand: complement of the reversed slice), each lane tests the 48
//    positions it owns against every cut site, a ballot picks the first hit; then a sweep counts G + C and N.
// K3 k_frag_gather: the fragments the host keeps, copied (reverse-complemented where needed) into one packed buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "td_internal.hpp"

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_BPT = 128;                      // bytes per thread: eight 16-byte loads
constexpr int FR_TILE = FR_THREADS * FR_BPT;     // 32 KiB per workgroup
constexpr int FR_SCAN_THREADS = 1024;

constexpr uint32_t F_ST = 1, F_HDR = 2, F_NW = 4;   // forward element
constexpr uint32_t B_TM = 1, B_NW = 2;              // backward element

// a stretch a, then b (text order)
__device__ __forceinline__ uint32_t fcomb(uint32_t a, uint32_t b) { return (b & F_ST) ? b : (a | (b & F_NW)); }
__device__ __forceinline__ uint32_t bcomb(uint32_t a, uint32_t b) { return (a & B_TM) ? a : (a | b); }

// Python's str.strip() set within ASCII: \t \n \v \f \r, 0x1c-0x1f, space
__device__ __forceinline__ bool fr_ws(uint32_t c) { return c == 32u || (c - 9u) <= 4u || (c - 28u) <= 3u; }
__device__ __forceinline__ bool fr_term(uint32_t c) { return c == 10u || c == 13u; }
__device__ __forceinline__ uint32_t fr_comp(uint32_t c) {
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}

struct TileSum {                 // 32 bytes
    uint32_t ef, eb, nhdr;
    uint32_t cnt[3];             // six 16-bit kept counters, see fr_kept
    uint32_t pad[2];
};
struct TileOut {                 // 32 bytes
    unsigned long long out_off, hdr_off;
    uint32_t fin, bin, pad[2];   // the carries: forward (F_HDR | F_NW of the open line), backward (B_NW)
};

// counter k = f * 2 + b: f = 0 decided "yes", 1 "yes unless the carried line is a header", 2 "yes if the carried
// line is no header and has non-whitespace"; b = 0 decided "yes", 1 "yes if the next tile's carry has non-whitespace"
__device__ __forceinline__ uint32_t fr_kept(const uint32_t cnt[3], uint32_t fin, uint32_t bin) {
    const bool nh = !(fin & F_HDR), nhnw = nh && (fin & F_NW), ib = (bin & B_NW) != 0;
    const uint32_t c0 = cnt[0] & 0xffff, c1 = cnt[0] >> 16, c2 = cnt[1] & 0xffff, c3 = cnt[1] >> 16,
                   c4 = cnt[2] & 0xffff, c5 = cnt[2] >> 16;
    return c0 + (ib ? c1 : 0) + (nh ? c2 + (ib ? c3 : 0) : 0) + (nhnw ? c4 + (ib ? c5 : 0) : 0);
}

// exclusive scans over a workgroup in thread order, op(left, right) in text order; *total = all threads
template <int NT, typename T, typename Op>
__device__ T fr_prefix(T v, T ident, Op op, T *sh, T *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(x, d, 64);
        if (lane >= d) x = op(o, x);
    }
    if (lane == 63) sh[w] = x;
    __syncthreads();
    T pre = ident, tot = ident;
    for (int i = 0; i < NT / 64; ++i) {
        if (i == w) pre = tot;
        tot = op(tot, sh[i]);
    }
    T ex = __shfl_up(x, 1, 64);
    if (lane == 0) ex = ident;
    __syncthreads();
    *total = tot;
    return op(pre, ex);
}
template <int NT, typename T, typename Op>
__device__ T fr_suffix(T v, T ident, Op op, T *sh, T *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_down(x, d, 64);
        if (lane + d < 64) x = op(x, o);
    }
    if (lane == 0) sh[w] = x;
    __syncthreads();
    T suf = ident, tot = ident;
    for (int i = NT / 64 - 1; i >= 0; --i) {
        if (i == w) suf = tot;
        tot = op(sh[i], tot);
    }
    T ex = __shfl_down(x, 1, 64);
    if (lane == 63) ex = ident;
    __syncthreads();
    *total = tot;
    return op(ex, suf);
}

struct FComb { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return fcomb(a, b); } };
struct BComb { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return bcomb(a, b); } };
template <typename T> struct Add { __device__ T operator()(T a, T b) const { return a + b; } };

// a thread's 128 bytes [s, s + 128) into 32 words; bytes at or past n read as 0 and are never used
__device__ __forceinline__ void fr_load(const uint8_t *text, uint64_t n, uint64_t s, uint32_t (&w)[32]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint64_t a = s + 16 * q;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (a + 16 <= n) {
            v = *(const uint4 *)(text + a);
        } else if (a < n) {
            uint32_t t[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (a + i < n) t[i >> 2] |= (uint32_t)text[a + i] << (8 * (i & 3));
            v = make_uint4(t[0], t[1], t[2], t[3]);
        }
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
}

#define FR_BYTE(k) ((w[(k) >> 2] >> (8 * ((k) & 3))) & 0xffu)

// One tile; EMIT = false: summary with unknown carries; EMIT = true: the emit pass with the carries of `to`.
template <bool EMIT>
__device__ __forceinline__ void fr_tile(const uint8_t *text, uint64_t n, TileSum *sums, const TileOut *outs, int *flags,
                        uint8_t *d_out, unsigned long long *rec, uint64_t rec_cap) {
    __shared__ uint32_t sh32[FR_THREADS / 64];
    __shared__ unsigned long long sh64[FR_THREADS / 64];
    __shared__ __align__(16) uint8_t stage[EMIT ? FR_TILE + 16 : 16];
    const uint64_t tile = blockIdx.x;
    const uint64_t s = tile * (uint64_t)FR_TILE + (uint64_t)threadIdx.x * FR_BPT;
    uint32_t w[32];
    fr_load(text, n, s, w);
    const uint32_t prev0 = (s > 0 && s - 1 < n) ? text[s - 1] : 10u;   // the file's first byte starts a line

    // this thread's elements
    uint32_t ef = 0, eb = 0, nh = 0, hi = 0;
    {
        uint32_t pc = prev0;
#pragma unroll
        for (int k = 0; k < FR_BPT; ++k) {
            if (s + k < n) {
                const uint32_t c = FR_BYTE(k);
                const bool ls = pc == 10u || (pc == 13u && c != 10u);
                const uint32_t nw = fr_ws(c) ? 0u : F_NW;
                ef = ls ? (F_ST | (c == '>' ? F_HDR : 0u) | nw) : (ef | nw);
                nh += (ls && c == '>') ? 1u : 0u;
                hi |= c;
                pc = c;
            }
        }
#pragma unroll
        for (int k = FR_BPT - 1; k >= 0; --k) {
            if (s + k < n) {
                const uint32_t c = FR_BYTE(k);
                eb = fr_term(c) ? B_TM : bcomb(fr_ws(c) ? 0u : B_NW, eb);
            }
        }
    }
    if ((hi & 0x80u) && flags) atomicOr(flags, 1);
    uint32_t tf, tb;
    uint32_t pf = fr_prefix<FR_THREADS>(ef, 0u, FComb(), sh32, &tf);
    uint32_t sb = fr_suffix<FR_THREADS>(eb, 0u, BComb(), sh32, &tb);
    if (EMIT) {
        const TileOut to = outs[tile];
        pf = fcomb(F_ST | to.fin, pf);   // the carried line's state as a line start: every byte is decided
        sb = bcomb(sb, B_TM | to.bin);
    }
    // backward state at every byte (inclusive), as two bit masks
    uint32_t mdet[4] = {0, 0, 0, 0}, mval[4] = {0, 0, 0, 0};
    {
        uint32_t g = sb;
#pragma unroll
        for (int k = FR_BPT - 1; k >= 0; --k) {
            if (s + k < n) {
                const uint32_t c = FR_BYTE(k);
                g = fr_term(c) ? B_TM : bcomb(fr_ws(c) ? 0u : B_NW, g);
                mdet[k >> 5] |= (g & B_TM) ? (1u << (k & 31)) : 0u;
                mval[k >> 5] |= (g & B_NW) ? (1u << (k & 31)) : 0u;
            }
        }
    }
    uint32_t cnt[3] = {0, 0, 0};
    uint32_t kept[4] = {0, 0, 0, 0};
    {
        uint32_t e = pf, pc = prev0;
#pragma unroll
        for (int k = 0; k < FR_BPT; ++k) {
            if (s + k < n) {
                const uint32_t c = FR_BYTE(k);
                const bool ls = pc == 10u || (pc == 13u && c != 10u);
                const uint32_t nw = fr_ws(c) ? 0u : F_NW;
                e = ls ? (F_ST | (c == '>' ? F_HDR : 0u) | nw) : (e | nw);
                pc = c;
                int f;                                  // -1: not kept
                if (e & F_ST) f = (!(e & F_HDR) && (e & F_NW)) ? 0 : -1;
                else f = (e & F_NW) ? 1 : 2;
                const bool det = (mdet[k >> 5] >> (k & 31)) & 1u, val = (mval[k >> 5] >> (k & 31)) & 1u;
                const int b = val ? 0 : (det ? -1 : 1);
                if (f >= 0 && b >= 0) {
                    const int idx = f * 2 + b;
                    cnt[idx >> 1] += 1u << (16 * (idx & 1));
                    kept[k >> 5] |= 1u << (k & 31);
                }
            }
        }
    }
    if (!EMIT) {
        uint32_t t0, t1, t2, tn;
        // (sums of packed 16-bit halves: a tile holds at most 32 768 bytes, no half overflows)
        (void)fr_prefix<FR_THREADS>(cnt[0], 0u, Add<uint32_t>(), sh32, &t0);
        (void)fr_prefix<FR_THREADS>(cnt[1], 0u, Add<uint32_t>(), sh32, &t1);
        (void)fr_prefix<FR_THREADS>(cnt[2], 0u, Add<uint32_t>(), sh32, &t2);
        (void)fr_prefix<FR_THREADS>(nh, 0u, Add<uint32_t>(), sh32, &tn);
        if (threadIdx.x == 0) {
            uint4 *d = (uint4 *)(sums + tile);
            d[0] = make_uint4(tf, tb, tn, t0);
            d[1] = make_uint4(t1, t2, 0, 0);
        }
        return;
    }
    // ---- emit: every byte was decided, so cnt[0] & 0xffff is this thread's kept count
    const TileOut to = outs[tile];
    const uint32_t mine = cnt[0] & 0xffffu;
    unsigned long long tot64;
    uint32_t totk;
    const uint32_t koff = fr_prefix<FR_THREADS>(mine, 0u, Add<uint32_t>(), sh32, &totk);
    const unsigned long long hbase = fr_prefix<FR_THREADS>((unsigned long long)nh, 0ull, Add<unsigned long long>(), sh64, &tot64);
    const uint8_t *dst = d_out + to.out_off;
    const uint32_t pad = (uint32_t)((uintptr_t)dst & 15u);
    uint32_t hmask[4] = {0, 0, 0, 0};
    {
        uint32_t j = pad + koff, pc = prev0;
#pragma unroll
        for (int k = 0; k < FR_BPT; ++k) {
            if (s + k < n) {
                const uint32_t c = FR_BYTE(k);
                const bool ls = pc == 10u || (pc == 13u && c != 10u);
                pc = c;
                hmask[k >> 5] |= (ls && c == '>') ? (1u << (k & 31)) : 0u;
                if ((kept[k >> 5] >> (k & 31)) & 1u) stage[j++] = (uint8_t)((c - 97u) <= 25u ? c - 32u : c);
            }
        }
    }
    // record rows: the name's input offsets after strip(), the compacted offset of the header line
    {
        uint32_t hk = 0, below = koff;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t m = hmask[q];
            while (m) {
                const uint32_t b = __builtin_ctz(m);
                m &= m - 1;
                const uint64_t pos = s + 32 * q + b;
                const unsigned long long idx = to.hdr_off + hbase + hk++;
                uint64_t nlo = pos + 1, nhi = pos + 1;
                bool any = false;
                for (uint64_t p = pos + 1; p < n; ++p) {
                    const uint32_t x = text[p];
                    if (fr_term(x)) break;
                    if (!fr_ws(x)) { if (!any) nlo = p; any = true; nhi = p + 1; }
                }
                if (!any) nhi = nlo;
                if (idx < rec_cap) {
                    rec[3 * idx] = nlo;
                    rec[3 * idx + 1] = nhi;
                    rec[3 * idx + 2] = to.out_off + below + __builtin_popcount(kept[q] & ((1u << b) - 1u));
                } else if (flags) {
                    atomicOr(flags, 2);
                }
            }
            below += __builtin_popcount(kept[q]);
        }
    }
    __syncthreads();
    if (to.out_off + totk > n) {                     // (kept bytes never outnumber the input: a scan gone wrong)
        if (threadIdx.x == 0 && flags) atomicOr(flags, 4);
        return;
    }
    const uint32_t total = pad + totk;
    uint8_t *base = (uint8_t *)dst - pad;
    for (uint32_t q = threadIdx.x; q * 16 < total; q += FR_THREADS) {
        const uint32_t a = q * 16;
        if (a >= pad && a + 16 <= total) {
            *(uint4 *)(base + a) = *(const uint4 *)(stage + a);
        } else {
            for (uint32_t i = 0; i < 16; ++i)
                if (a + i >= pad && a + i < total) base[a + i] = stage[a + i];
        }
    }
}

__global__ __launch_bounds__(FR_THREADS) void k_fasta_summary(const uint8_t *text, uint64_t n, TileSum *sums, int *flags) {
    fr_tile<false>(text, n, sums, nullptr, flags, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(FR_THREADS) void k_fasta_emit(const uint8_t *text, uint64_t n, const TileOut *outs, int *flags,
                                                           uint8_t *d_out, unsigned long long *rec, uint64_t rec_cap) {
    fr_tile<true>(text, n, nullptr, outs, flags, d_out, rec, rec_cap);
}

// One workgroup: the tiles' backward carries (right to left), then forward carries, kept-byte offsets and header
// offsets (left to right).  totals[0] = kept bytes, totals[1] = header lines.
__global__ __launch_bounds__(FR_SCAN_THREADS) void k_fasta_scan(const TileSum *sums, TileOut *outs, uint64_t ntiles,
                                                                unsigned long long *totals) {
    __shared__ uint32_t sh32[FR_SCAN_THREADS / 64];
    __shared__ unsigned long long sh64[FR_SCAN_THREADS / 64];
    uint32_t cb = B_TM;                      // past the file's end: a line end with nothing after it
    for (uint64_t hiT = ntiles; hiT > 0;) {
        const uint64_t loT = hiT > FR_SCAN_THREADS ? hiT - FR_SCAN_THREADS : 0;
        const uint64_t i = loT + threadIdx.x;
        const uint32_t e = i < hiT ? sums[i].eb : 0u;
        uint32_t tot;
        const uint32_t sfx = fr_suffix<FR_SCAN_THREADS>(e, 0u, BComb(), sh32, &tot);
        if (i < hiT) outs[i].bin = bcomb(sfx, cb) & B_NW;
        cb = bcomb(tot, cb);
        hiT = loT;
    }
    __syncthreads();
    uint32_t cf = F_ST;                      // before the file: a line start, no header, nothing seen
    unsigned long long koff = 0, hoff = 0;
    for (uint64_t loT = 0; loT < ntiles; loT += FR_SCAN_THREADS) {
        const uint64_t i = loT + threadIdx.x;
        TileSum t = {};
        if (i < ntiles) t = sums[i];
        uint32_t tot;
        const uint32_t pre = fr_prefix<FR_SCAN_THREADS>(i < ntiles ? t.ef : 0u, 0u, FComb(), sh32, &tot);
        const uint32_t fin = fcomb(cf, pre) & (F_HDR | F_NW);
        const uint32_t bin = i < ntiles ? outs[i].bin : 0u;
        const unsigned long long kept = i < ntiles ? fr_kept(t.cnt, fin, bin) : 0u;
        unsigned long long kt, ht;
        const unsigned long long kx = fr_prefix<FR_SCAN_THREADS>(kept, 0ull, Add<unsigned long long>(), sh64, &kt);
        const unsigned long long hx = fr_prefix<FR_SCAN_THREADS>((unsigned long long)t.nhdr, 0ull, Add<unsigned long long>(), sh64, &ht);
        if (i < ntiles) {
            outs[i].out_off = koff + kx;
            outs[i].hdr_off = hoff + hx;
            outs[i].fin = fin;
        }
        cf = fcomb(cf, tot);
        koff += kt;
        hoff += ht;
    }
    if (threadIdx.x == 0) {
        totals[0] = koff;
        totals[1] = hoff;
    }
}

// ---------------------------------------------------------------- K2 / K3
constexpr int FS_WAVES = 4;
constexpr int FS_WIN = 3072;                      // 64 lanes x 48 positions
constexpr int FS_LDS = FS_WIN + 128;              // the window and a zero halo for the longest site

struct FragSites {
    uint8_t s[TD_FRAG_MAX_SITES][TD_FRAG_MAX_SITE_LEN];
    int32_t len[TD_FRAG_MAX_SITES];
    int32_t n;
};

__global__ __launch_bounds__(FS_WAVES * 64) void k_frag_search(const uint8_t *seq, const td_frag_job *jobs, uint64_t njobs,
                                                               const FragSites *sites, int4 *out) {
    __shared__ __align__(16) uint8_t win[FS_WAVES][FS_LDS];
    __shared__ uint8_t shs[TD_FRAG_MAX_SITES * TD_FRAG_MAX_SITE_LEN];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < TD_FRAG_MAX_SITES * TD_FRAG_MAX_SITE_LEN; i += FS_WAVES * 64)
        shs[i] = sites->s[i / TD_FRAG_MAX_SITE_LEN][i % TD_FRAG_MAX_SITE_LEN];
    const int nsites = sites->n;
    const uint64_t j = (uint64_t)blockIdx.x * FS_WAVES + wv;
    const bool active = j < njobs;
    uint64_t lo = 0, hi = 0;
    int64_t tagsize = 0;
    bool rev = false;
    if (active) {
        lo = jobs[j].lo;
        hi = jobs[j].hi;
        tagsize = jobs[j].tagsize;
        rev = jobs[j].reverse != 0;
    }
    const uint32_t n = (uint32_t)(hi - lo);       // the host checked n <= FS_WIN
    uint8_t *w = win[wv];
    if (n) {
        const uint64_t base = lo & ~15ull;
        const uint32_t nch = (uint32_t)((hi + 15 - base) >> 4);
        for (uint32_t c = lane; c < nch; c += 64) {
            const uint64_t a = base + 16ull * c;
            const uint4 v = *(const uint4 *)(seq + a);
            const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint64_t g = a + i;
                if (g >= lo && g < hi) {
                    const uint32_t b = (vw[i >> 2] >> (8 * (i & 3))) & 0xffu;
                    if (rev) w[hi - 1 - g] = (uint8_t)fr_comp(b);
                    else w[g - lo] = (uint8_t)b;
                }
            }
        }
    }
    for (uint32_t k = n + lane; k < n + 128 && k < FS_LDS; k += 64) w[k] = 0;
    __syncthreads();
    int best = 0x7fffffff;
    for (int si = 0; si < nsites; ++si) {
        const int m = sites->len[si];
        const uint8_t *cs = shs + si * TD_FRAG_MAX_SITE_LEN;
        // str.find(cs, tagsize - len(cs)): a negative start counts from the end, clamped at 0
        int64_t st = tagsize - m;
        if (st < 0) { st += n; if (st < 0) st = 0; }
        const int64_t last = (int64_t)n - m;
        int found = 0x7fffffff;
        if (st <= last) {
            const int64_t p0 = std::max<int64_t>(st, 48 * lane), p1 = std::min<int64_t>(last, 48 * lane + 47);
            for (int64_t p = p0; p <= p1; ++p) {
                int q = 0;
                while (q < m && w[p + q] == cs[q]) ++q;
                if (q == m) { found = (int)p; break; }
            }
        }
        const unsigned long long bal = __ballot(found != 0x7fffffff);
        if (bal) {
            const int first = __ffsll((long long)bal) - 1;
            const int pos = __shfl(found, first, 64);
            best = std::min(best, pos + m);
        }
    }
    const int size = best == 0x7fffffff ? -1 : best;
    int gc = 0, nn = 0;
    for (int k = lane; k < size; k += 64) {
        const uint32_t c = w[k];
        gc += (c == 'G' || c == 'C') ? 1 : 0;
        nn += c == 'N' ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        gc += __shfl_xor(gc, d, 64);
        nn += __shfl_xor(nn, d, 64);
    }
    if (active && lane == 0) out[j] = make_int4(size, gc, nn, 0);
}

__global__ __launch_bounds__(256) void k_frag_gather(const uint8_t *seq, const td_frag_job *jobs, const int32_t *sizes,
                                                     const unsigned long long *offs, uint64_t njobs, uint8_t *out) {
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= njobs) return;
    const uint64_t lo = jobs[j].lo, hi = jobs[j].hi;
    const bool rev = jobs[j].reverse != 0;
    const int size = sizes[j];
    uint8_t *o = out + offs[j];
    for (int k = lane; k < size; k += 64) {
        if (rev) o[k] = (uint8_t)fr_comp(seq[hi - 1 - k]);
        else o[k] = seq[lo + k];
    }
}

}  // namespace

extern "C" int td_fasta_frame_device(td_handle *h, const void *d_text, uint64_t nbytes, void *d_out, uint64_t *n_out,
                                     uint64_t *rec_out, uint64_t rec_cap, uint64_t *n_rec, int *nonascii, double *ms) {
    if (!h || !n_out || !n_rec || !nonascii || (nbytes && (!d_text || !d_out)) || (rec_cap && !rec_out))
        return td_fail_internal(TD_E_ARG, "NULL argument");
    if ((uintptr_t)d_text & 15u) return td_fail_internal(TD_E_ARG, "d_text must be 16-byte aligned");
    *n_out = 0; *n_rec = 0; *nonascii = 0;
    if (ms) *ms = 0;
    if (!nbytes) return TD_OK;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    const uint64_t ntiles = (nbytes + FR_TILE - 1) / FR_TILE;
    if (ntiles > 0x7fffffffull) return td_fail_internal(TD_E_LIMIT, "genome file too large for one launch");
    tdi::DevBuf<TileSum> sums;
    tdi::DevBuf<TileOut> outs;
    tdi::DevBuf<unsigned long long> tot;   // [0] kept bytes, [1] header lines, [2] flags
    TD_HIPCHK(sums.alloc(ntiles));
    TD_HIPCHK(outs.alloc(ntiles));
    TD_HIPCHK(tot.alloc(4));
    TD_HIPCHK(hipMemset(tot.p, 0, 4 * sizeof(unsigned long long)));
    tdi::Events<2> ev;
    TD_HIPCHK(ev.create());
    int *flags = (int *)(tot.p + 2);
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    hipLaunchKernelGGL(k_fasta_summary, dim3((uint32_t)ntiles), dim3(FR_THREADS), 0, 0, (const uint8_t *)d_text, nbytes, sums.p, flags);
    TD_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_fasta_scan, dim3(1), dim3(FR_SCAN_THREADS), 0, 0, sums.p, outs.p, ntiles, tot.p);
    TD_HIPCHK(hipGetLastError());
    unsigned long long th[4];
    TD_HIPCHK(hipMemcpy(th, tot.p, sizeof th, hipMemcpyDeviceToHost));
    *n_rec = th[1];
    if (*(const int *)&th[2] & 1) {      // a byte >= 0x80: the caller reads this file on the host
        *nonascii = 1;
        return TD_OK;
    }
    if (th[0] > nbytes) return td_fail_internal(TD_E_INTERNAL, "k_fasta_scan: more kept bytes than input");
    if (th[1] > rec_cap) return td_fail_internal(TD_E_LIMIT, ("record table holds " + std::to_string(rec_cap) + " rows, the file has " +
                                                             std::to_string(th[1]) + " header lines").c_str());
    tdi::DevBuf<unsigned long long> rec;
    TD_HIPCHK(rec.alloc(3 * th[1]));
    hipLaunchKernelGGL(k_fasta_emit, dim3((uint32_t)ntiles), dim3(FR_THREADS), 0, 0, (const uint8_t *)d_text, nbytes, outs.p,
                       flags, (uint8_t *)d_out, rec.p, (uint64_t)th[1]);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[1]));
    if (ms) {
        float f = 0;
        TD_HIPCHK(hipEventElapsedTime(&f, ev.e[0], ev.e[1]));
        *ms = f;
    }
    TD_HIPCHK(hipMemcpy(th, tot.p, sizeof th, hipMemcpyDeviceToHost));
    if (*(const int *)&th[2] & 2) return td_fail_internal(TD_E_INTERNAL, "k_fasta_emit: header row past the table");
    if (*(const int *)&th[2] & 4) return td_fail_internal(TD_E_INTERNAL, "k_fasta_emit: kept bytes past the input's size");
    if (th[1]) TD_HIPCHK(hipMemcpy(rec_out, rec.p, 3 * th[1] * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n_out = th[0];
    return TD_OK;
}

static int frag_sites(const char *const *sites, uint32_t nsites, FragSites *fs) {
    if (nsites > TD_FRAG_MAX_SITES) return td_fail_internal(TD_E_LIMIT, "more than 16 cut sites");
    memset(fs, 0, sizeof *fs);
    for (uint32_t i = 0; i < nsites; ++i) {
        if (!sites[i]) return td_fail_internal(TD_E_ARG, "NULL cut site");
        const size_t m = strlen(sites[i]);
        if (m == 0) return td_fail_internal(TD_E_ARG, "empty cut site (the caller decides those)");
        if (m > TD_FRAG_MAX_SITE_LEN) return td_fail_internal(TD_E_LIMIT, "cut site longer than 64 bases");
        memcpy(fs->s[i], sites[i], m);
        fs->len[i] = (int32_t)m;
    }
    fs->n = (int32_t)nsites;
    return TD_OK;
}

static int frag_check_jobs(const td_frag_job *jobs, uint64_t njobs, uint64_t seq_bytes) {
    for (uint64_t j = 0; j < njobs; ++j) {
        if (jobs[j].lo > jobs[j].hi || jobs[j].hi > seq_bytes) return td_fail_internal(TD_E_ARG, "job window outside the sequence");
        if (jobs[j].hi - jobs[j].lo > TD_FRAG_MAX_WINDOW) return td_fail_internal(TD_E_LIMIT, "job window longer than 3 072 bytes");
        if (jobs[j].tagsize < 0) return td_fail_internal(TD_E_ARG, "negative tag size");
    }
    return TD_OK;
}

extern "C" int td_frag_search_device(td_handle *h, const void *d_seq, uint64_t seq_bytes, const td_frag_job *jobs, uint64_t njobs,
                                     const char *const *sites, uint32_t nsites, int32_t *out, double *ms) {
    if (!h || (njobs && (!jobs || !out || !d_seq)) || (nsites && !sites)) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (ms) *ms = 0;
    FragSites fs;
    int rc = frag_sites(sites, nsites, &fs);
    if (rc) return rc;
    if ((rc = frag_check_jobs(jobs, njobs, seq_bytes))) return rc;
    if (!njobs) return TD_OK;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    tdi::DevBuf<td_frag_job> dj;
    tdi::DevBuf<int4> dout;
    tdi::DevBuf<FragSites> dfs;
    TD_HIPCHK(dj.alloc(njobs));
    TD_HIPCHK(dout.alloc(njobs));
    TD_HIPCHK(dfs.alloc(1));
    TD_HIPCHK(hipMemcpy(dfs.p, &fs, sizeof fs, hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(dj.p, jobs, njobs * sizeof(td_frag_job), hipMemcpyHostToDevice));
    tdi::Events<2> ev;
    TD_HIPCHK(ev.create());
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    const uint64_t grid = (njobs + FS_WAVES - 1) / FS_WAVES;
    if (grid > 0x7fffffffull) return td_fail_internal(TD_E_LIMIT, "too many jobs for one launch");
    hipLaunchKernelGGL(k_frag_search, dim3((uint32_t)grid), dim3(FS_WAVES * 64), 0, 0, (const uint8_t *)d_seq, dj.p, njobs, dfs.p, dout.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[1]));
    if (ms) {
        float f = 0;
        TD_HIPCHK(hipEventElapsedTime(&f, ev.e[0], ev.e[1]));
        *ms = f;
    }
    TD_HIPCHK(hipMemcpy(out, dout.p, njobs * sizeof(int4), hipMemcpyDeviceToHost));
    return TD_OK;
}

extern "C" int td_frag_gather_device(td_handle *h, const void *d_seq, uint64_t seq_bytes, const td_frag_job *jobs,
                                     const int32_t *sizes, uint64_t njobs, void *out, uint64_t out_cap, uint64_t *n_out, double *ms) {
    if (!h || !n_out || (njobs && (!jobs || !sizes || !d_seq))) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (ms) *ms = 0;
    *n_out = 0;
    int rc = frag_check_jobs(jobs, njobs, seq_bytes);
    if (rc) return rc;
    std::vector<unsigned long long> offs(njobs ? njobs : 1);
    uint64_t total = 0;
    for (uint64_t j = 0; j < njobs; ++j) {
        if (sizes[j] > 0 && (uint64_t)sizes[j] > jobs[j].hi - jobs[j].lo) return td_fail_internal(TD_E_ARG, "fragment longer than its window");
        offs[j] = total;
        total += sizes[j] > 0 ? (uint64_t)sizes[j] : 0;
    }
    if (total > out_cap) return td_fail_internal(TD_E_LIMIT, "output buffer too small");
    if (!total) return TD_OK;
    if (!out) return td_fail_internal(TD_E_ARG, "NULL argument");
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    tdi::DevBuf<td_frag_job> dj;
    tdi::DevBuf<int32_t> dsz;
    tdi::DevBuf<unsigned long long> doff;
    tdi::DevBuf<uint8_t> dout;
    TD_HIPCHK(dj.alloc(njobs));
    TD_HIPCHK(dsz.alloc(njobs));
    TD_HIPCHK(doff.alloc(njobs));
    TD_HIPCHK(dout.alloc(total));
    TD_HIPCHK(hipMemcpy(dj.p, jobs, njobs * sizeof(td_frag_job), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(dsz.p, sizes, njobs * sizeof(int32_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(doff.p, offs.data(), njobs * sizeof(unsigned long long), hipMemcpyHostToDevice));
    tdi::Events<2> ev;
    TD_HIPCHK(ev.create());
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    const uint64_t grid = (njobs + 3) / 4;
    if (grid > 0x7fffffffull) return td_fail_internal(TD_E_LIMIT, "too many fragments for one launch");
    hipLaunchKernelGGL(k_frag_gather, dim3((uint32_t)grid), dim3(256), 0, 0, (const uint8_t *)d_seq, dj.p, dsz.p, doff.p, njobs, dout.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[1]));
    if (ms) {
        float f = 0;
        TD_HIPCHK(hipEventElapsedTime(&f, ev.e[0], ev.e[1]));
        *ms = f;
    }
    TD_HIPCHK(hipMemcpy(out, dout.p, total, hipMemcpyDeviceToHost));
    *n_out = total;
    return TD_OK;
}
