// Tag network on the GPU (include/tagdig.h: td_tagnet_build, td_tagnet_edges, td_tagnet_pairs, td_tagnet_degrees,
// td_tagnet_free): the one-mismatch self-join over n distinct tags of one length L <= 64, and the UNEAK filter on it.
//
// The rule: an edge joins two tags that differ at exactly one position; it is kept when
// min(c_i, c_j) * 1 000 000 >= ratio_ppm * max(c_i, c_j) (128-bit integers); a pair is a kept edge whose two ends
// both have exactly one kept edge.
//
// K1 k_tn_pack: one thread per tag packs its bases to 2 bits (A 0, C 1, G 2, T 3) and splits them at h = ceil(L / 2)
//    into part A = bases [0, h) and part B = bases [h, L): one 64-bit word each, base k of a part in bits 2k, 2k + 1.
//    The words are laid out word-major as [A | B | A], so that (A, B) and (B, A) are both two-word keys of
//    radix_sort.hpp.  A byte outside ACGT is flagged with the tag's index.
// K2 the tag permutation is sorted once by (A, B) and once by (B, A) (radix_sort.hpp, shared with tagset.hip).
//    k_tn_dup: equal neighbours after the first sort are duplicates.  Two tags at distance 1 agree in exactly one of
//    A and B, so every edge lies inside a run of equal leading words of exactly one of the two orders.
// K3 k_tn_gather lays the other word, the count and the tag's index out in sorted order; k_tn_runs gives every sorted
//    position p the end of its run, end[p] (the next position is looked at first, a binary search follows only inside a
//    run), and sums compares = sum (end[p] - p - 1) = sum over runs of len (len - 1) / 2; k_tn_tiles counts, for every
//    block of TD_TAGNET_TILE rows, the column blocks its rows reach: rows [256 r, 256 r + 256) meet columns up to
//    end[last row] - 1, since end[] does not decrease.  An exclusive scan (k_rs_scan) turns the counts into the tile list.
// K4 k_tn_compare: one workgroup per tile (row block r, column block c >= r).  The column block's other words, counts
//    and indices are staged in LDS; thread t owns row 256 r + t and walks the columns q with max(p + 1, c0) <= q <
//    min(end[p], c0 + 256): x = a ^ b, one mismatch when popcount((x | x >> 1) & 0x5555...) == 1.  A run of m tags
//    therefore spreads over about (m / 256)^2 / 2 workgroups, and a short run costs its rows a few iterations.  An edge
//    is judged by the kept rule where it is found, its two degrees are incremented with atomics, and the record
//    kept << 63 | i << 32 | j (i < j) goes to a queue in LDS that the workgroup appends to the edge buffer with one
//    atomic (a queue that is full sends the record there directly).  The buffer holds min(3 L n / 2, compares) records
//    -- a tag has at most 3 L neighbours -- and every write checks it.
// K5 k_tn_select: the kept edges whose two degrees are 1, appended per wave (ballot, one atomic per wave).
// The host sorts the edges and the pairs by (i, j) after the copy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "radix_sort.hpp"
#include "td_internal.hpp"

struct td_tagnet {
    uint32_t n;
    std::vector<uint64_t> edges;   // kept << 63 | i << 32 | j, ascending by (i, j)
    std::vector<uint64_t> pairs;   // i << 32 | j, ascending
    std::vector<uint32_t> deg;     // n
};

namespace {

constexpr int TN_TILE = TD_TAGNET_TILE;            // rows and columns of a tile = threads of a workgroup
constexpr int TN_QUEUE = 1024;                     // edge records a workgroup collects in LDS
constexpr uint64_t TN_KEPT = 1ull << 63;
constexpr uint64_t TN_MAX_TILES = 0x7fffffffull;
static_assert(TN_TILE == 256, "k_tn_compare is written for workgroups of 256 threads");

// one sorted order: what K3 prepares and K4 reads
struct TnOrder {
    tdi::DevBuf<uint64_t> lead, other, cnt;
    tdi::DevBuf<uint32_t> idx, end, tile_off;
    uint32_t ntiles = 0;
};

// ------------------------------------------------------------------ K1
__global__ __launch_bounds__(256) void k_tn_pack(const uint8_t *seqs, uint32_t n, uint32_t L, uint32_t h, uint64_t *key,
                                                 uint32_t *bad_first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *s = seqs + (uint64_t)i * L;
    uint64_t a = 0, b = 0;
    bool bad = false;
    for (uint32_t k = 0; k < L; ++k) {
        const uint32_t c = s[k];
        const uint64_t v = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
        if (v == 4u) bad = true;
        if (k < h) a |= (v & 3u) << (2 * k); else b |= (v & 3u) << (2 * (k - h));
    }
    key[i] = a;
    key[(uint64_t)n + i] = b;
    key[2ull * n + i] = a;
    if (bad) atomicMin(bad_first, i);
}

// ------------------------------------------------------------------ K2: duplicates after the (A, B) sort
__global__ __launch_bounds__(256) void k_tn_dup(const uint64_t *key, const uint32_t *perm, uint32_t n, uint32_t *dup_first) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0 || p >= n) return;
    const uint32_t u = perm[p - 1], v = perm[p];
    if (key[u] == key[v] && key[(uint64_t)n + u] == key[(uint64_t)n + v]) atomicMin(dup_first, u > v ? u : v);
}

// ------------------------------------------------------------------ K3
// key: the two words of this order (leading word first), word-major
__global__ __launch_bounds__(256) void k_tn_gather(const uint64_t *key, const uint64_t *counts, const uint32_t *perm, uint32_t n,
                                                   uint64_t *lead, uint64_t *other, uint64_t *cnt, uint32_t *idx) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t v = perm[p];
    lead[p] = key[v];
    other[p] = key[(uint64_t)n + v];
    cnt[p] = counts[v];
    idx[p] = v;
}

__global__ __launch_bounds__(256) void k_tn_runs(const uint64_t *lead, uint32_t n, uint32_t *end, unsigned long long *compares) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t mine = 0;
    if (p < n) {
        const uint64_t v = lead[p];
        uint32_t e = p + 1;
        if (e < n && lead[e] == v) {             // inside a run: the first position past it
            uint32_t lo = e + 1, hi = n;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (lead[mid] == v) lo = mid + 1; else hi = mid;
            }
            e = lo;
        }
        end[p] = e;
        mine = e - p - 1;
    }
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(compares, (unsigned long long)mine);
}

// tiles[r] = column blocks that row block r meets, r < nrb; tiles[nrb] = 0 (the scan leaves the total there)
__global__ __launch_bounds__(256) void k_tn_tiles(const uint32_t *end, uint32_t n, uint32_t nrb, uint32_t *tiles) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nrb) return;
    if (r == nrb) { tiles[r] = 0; return; }
    const uint32_t first = r * TN_TILE;
    const uint32_t last = first + TN_TILE - 1 < n - 1 ? first + TN_TILE - 1 : n - 1;
    const uint32_t e = end[last];                                    // <= n
    // nothing to compare in a row block whose every row is the last of its run
    bool any = false;
    for (uint32_t p = first; p <= last && !any; ++p) any = end[p] != p + 1;
    tiles[r] = any ? (e + TN_TILE - 1) / TN_TILE - r : 0u;
}

// ------------------------------------------------------------------ K4
__device__ __forceinline__ bool tn_kept(uint64_t a, uint64_t b, uint32_t ppm) {
    const uint64_t minor = a < b ? a : b, major = a < b ? b : a;
    const uint64_t lh = __umul64hi(minor, 1000000ull), ll = minor * 1000000ull;
    const uint64_t rh = __umul64hi(major, (uint64_t)ppm), rl = major * (uint64_t)ppm;
    return lh > rh || (lh == rh && ll >= rl);
}

__global__ __launch_bounds__(TN_TILE) void k_tn_compare(const uint64_t *other, const uint64_t *cnt, const uint32_t *idx,
                                                        const uint32_t *end, const uint32_t *tile_off, uint32_t nrb, uint32_t n,
                                                        uint32_t ppm, uint64_t *edges, uint64_t cap, unsigned long long *nedges,
                                                        uint32_t *deg, uint32_t *overflow) {
    __shared__ uint64_t s_other[TN_TILE];
    __shared__ uint64_t s_cnt[TN_TILE];
    __shared__ uint32_t s_idx[TN_TILE];
    __shared__ uint64_t s_q[TN_QUEUE];
    __shared__ uint32_t s_qn, s_r;
    __shared__ unsigned long long s_base;
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        // the row block this tile belongs to: the last r with tile_off[r] <= blockIdx.x (tile_off[nrb] = all tiles)
        uint32_t lo = 0, hi = nrb;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (tile_off[mid] <= blockIdx.x) lo = mid; else hi = mid;
        }
        s_r = lo;
        s_qn = 0;
    }
    __syncthreads();
    const uint32_t r = s_r;
    const uint32_t c0 = (r + (blockIdx.x - tile_off[r])) * TN_TILE;      // < n: the tile list ends at ceil(end / 256)
    if (c0 + t < n) {
        s_other[t] = other[c0 + t];
        s_cnt[t] = cnt[c0 + t];
        s_idx[t] = idx[c0 + t];
    }
    const uint32_t p = r * TN_TILE + t;
    uint64_t mine = 0, mycnt = 0;
    uint32_t myidx = 0, lo = 0, hi = 0;
    if (p < n) {
        mine = other[p];
        mycnt = cnt[p];
        myidx = idx[p];
        const uint32_t e = end[p];                                        // <= n, so every column read below was staged
        lo = p + 1 > c0 ? p + 1 : c0;
        hi = e < c0 + TN_TILE ? e : c0 + TN_TILE;
    }
    __syncthreads();
    for (uint32_t q = lo; q < hi; ++q) {
        const uint64_t x = mine ^ s_other[q - c0];
        const uint64_t m = (x | (x >> 1)) & 0x5555555555555555ull;
        if (__popcll(m) != 1) continue;
        const uint32_t oi = s_idx[q - c0];
        const uint32_t i = myidx < oi ? myidx : oi, j = myidx < oi ? oi : myidx;
        uint64_t rec = ((uint64_t)i << 32) | j;
        if (tn_kept(mycnt, s_cnt[q - c0], ppm)) {
            rec |= TN_KEPT;
            atomicAdd(&deg[i], 1u);
            atomicAdd(&deg[j], 1u);
        }
        const uint32_t slot = atomicAdd(&s_qn, 1u);
        if (slot < TN_QUEUE) {
            s_q[slot] = rec;
        } else {
            const unsigned long long g = atomicAdd(nedges, 1ull);
            if (g < cap) edges[g] = rec; else *overflow = 1u;
        }
    }
    __syncthreads();
    const uint32_t nq = s_qn < TN_QUEUE ? s_qn : TN_QUEUE;
    if (nq == 0) return;                                                  // uniform: s_qn is shared
    if (t == 0) s_base = atomicAdd(nedges, (unsigned long long)nq);
    __syncthreads();
    const unsigned long long base = s_base;
    for (uint32_t k = t; k < nq; k += TN_TILE) {
        if (base + k < cap) edges[base + k] = s_q[k]; else *overflow = 1u;
    }
}

// ------------------------------------------------------------------ K5
__global__ __launch_bounds__(256) void k_tn_select(const uint64_t *edges, uint64_t nedges, const uint32_t *deg, uint64_t *pairs,
                                                   uint64_t cap, unsigned long long *npairs, uint32_t *overflow) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool take = false;
    uint64_t rec = 0;
    if (k < nedges) {
        rec = edges[k];
        take = (rec & TN_KEPT) && deg[(uint32_t)((rec & ~TN_KEPT) >> 32)] == 1u && deg[(uint32_t)rec] == 1u;
    }
    const uint64_t votes = __ballot(take);
    if (!votes) return;
    unsigned long long base = 0;
    if (lane == __ffsll((unsigned long long)votes) - 1) base = atomicAdd(npairs, (unsigned long long)__popcll(votes));
    base = __shfl(base, __ffsll((unsigned long long)votes) - 1, 64);
    if (take) {
        const unsigned long long g = base + __popcll(votes & ((1ull << lane) - 1ull));
        if (g < cap) pairs[g] = rec & ~TN_KEPT; else *overflow = 1u;
    }
}

// K3 for one order: key = its two words (leading first); perm sorted by them
int tn_prepare(const uint64_t *key, const uint64_t *counts, const uint32_t *perm, uint32_t n, uint32_t nrb, TnOrder &o,
               unsigned long long *d_compares) {
    TD_HIPCHK(o.lead.alloc(n));
    TD_HIPCHK(o.other.alloc(n));
    TD_HIPCHK(o.cnt.alloc(n));
    TD_HIPCHK(o.idx.alloc(n));
    TD_HIPCHK(o.end.alloc(n));
    TD_HIPCHK(o.tile_off.alloc(nrb + 1ull));
    const dim3 grid((n + 255) / 256), block(256);
    hipLaunchKernelGGL(k_tn_gather, grid, block, 0, 0, key, counts, perm, n, o.lead.p, o.other.p, o.cnt.p, o.idx.p);
    hipLaunchKernelGGL(k_tn_runs, grid, block, 0, 0, o.lead.p, n, o.end.p, d_compares);
    hipLaunchKernelGGL(k_tn_tiles, dim3((nrb + 1 + 255) / 256), block, 0, 0, o.end.p, n, nrb, o.tile_off.p);
    hipLaunchKernelGGL(tdrs::k_rs_scan, dim3(1), dim3(tdrs::RS_SCAN_THREADS), 0, 0, o.tile_off.p, (uint64_t)nrb + 1);
    TD_HIPCHK(hipGetLastError());
    return TD_OK;
}

bool tn_less(uint64_t a, uint64_t b) { return (a & ~TN_KEPT) < (b & ~TN_KEPT); }

}  // namespace

extern "C" int td_tagnet_build(td_handle *h, const char *seqs, const uint64_t *counts, uint32_t n, uint32_t taglen,
                               uint32_t ratio_ppm, td_tagnet **out, uint64_t stats[8], double *ms) {
    if (!h || !out || (n && (!seqs || !counts))) return td_fail_internal(TD_E_ARG, "NULL argument");
    *out = nullptr;
    if (stats) for (int k = 0; k < 8; ++k) stats[k] = 0;
    if (ms) for (int k = 0; k < 6; ++k) ms[k] = 0;
    if (taglen < 1 || taglen > TD_TAGNET_MAX_TAGLEN) return td_fail_internal(TD_E_ARG, "taglen must be 1..64");
    if (ratio_ppm > 1000000u) return td_fail_internal(TD_E_ARG, "ratio_ppm must be 0..1000000");
    if (n > TD_TAGSET_MAX_TAGS) return td_fail_internal(TD_E_LIMIT, "more than 2^30 tags");
    const uint32_t L = taglen, half = (L + 1) / 2;
    td_tagnet *net = new td_tagnet;
    net->n = n;
    net->deg.assign(n, 0u);
    struct Guard { td_tagnet *p; ~Guard() { delete p; } } guard{net};
    uint64_t st[8] = {n, 0, 0, n, 0, 0, 0, 0};

    if (n) {
        TD_HIPCHK(hipSetDevice(td_handle_device(h)));
        tdi::Events<6> ev;
        TD_HIPCHK(ev.create());
        tdi::DevBuf<uint8_t> dseq;
        tdi::DevBuf<uint64_t> key, dcnt, edges, pairs;
        tdi::DevBuf<uint16_t> len;
        tdi::DevBuf<uint32_t> flags, perm0, perm1, perm2, differ, hist, deg;
        tdi::DevBuf<unsigned long long> ctr;                 // [0] compares, [1] edges, [2] pairs
        // ---- K1
        TD_HIPCHK(dseq.alloc((uint64_t)n * L));
        TD_HIPCHK(key.alloc(3ull * n));
        TD_HIPCHK(dcnt.alloc(n));
        TD_HIPCHK(flags.alloc(3));                         // [0] first bad tag, [1] first duplicate, [2] a write past a buffer
        TD_HIPCHK(ctr.alloc(3));
        TD_HIPCHK(hipMemcpy(dseq.p, seqs, (uint64_t)n * L, hipMemcpyHostToDevice));
        TD_HIPCHK(hipMemcpy(dcnt.p, counts, (uint64_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
        const uint32_t finit[3] = {0xffffffffu, 0xffffffffu, 0u};
        TD_HIPCHK(hipMemcpy(flags.p, finit, sizeof finit, hipMemcpyHostToDevice));
        TD_HIPCHK(hipMemset(ctr.p, 0, 3 * sizeof(unsigned long long)));
        const dim3 grid((n + 255) / 256), block(256);
        TD_HIPCHK(hipEventRecord(ev.e[0], 0));
        hipLaunchKernelGGL(k_tn_pack, grid, block, 0, 0, dseq.p, n, L, half, key.p, flags.p);
        TD_HIPCHK(hipGetLastError());
        TD_HIPCHK(hipEventRecord(ev.e[1], 0));
        uint32_t fl[3];
        TD_HIPCHK(hipMemcpy(fl, flags.p, sizeof fl, hipMemcpyDeviceToHost));
        if (fl[0] != 0xffffffffu) {
            td_set_bad_index(fl[0]);
            return td_fail_internal(TD_E_ALPHABET, ("tag " + std::to_string(fl[0]) + " holds a byte outside ACGT").c_str());
        }
        if (n > 1) {
            // ---- K2
            TD_HIPCHK(len.alloc(n));
            TD_HIPCHK(perm0.alloc(n));
            TD_HIPCHK(perm1.alloc(n));
            TD_HIPCHK(perm2.alloc(n));
            TD_HIPCHK(differ.alloc(3));
            TD_HIPCHK(hist.alloc(256ull * tdrs::rs_blocks(n)));
            TD_HIPCHK(hipMemset(len.p, 0, (uint64_t)n * sizeof(uint16_t)));
            std::vector<uint32_t> ident(n);
            for (uint32_t i = 0; i < n; ++i) ident[i] = i;
            uint32_t passes = 0;
            // (A, B): the result stays in perm0 / perm1; (B, A) then sorts in perm2 and the buffer that is left
            TD_HIPCHK(hipMemcpy(perm0.p, ident.data(), (uint64_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
            TD_HIPCHK(hipMemset(differ.p, 0, 3 * sizeof(uint32_t)));
            TD_HIPCHK(tdrs::rs_sort(key.p, len.p, n, 2, &perm0.p, &perm1.p, differ.p, hist.p, &passes));
            hipLaunchKernelGGL(k_tn_dup, grid, block, 0, 0, key.p, perm0.p, n, flags.p + 1);
            TD_HIPCHK(hipGetLastError());
            TD_HIPCHK(hipMemcpy(fl, flags.p, sizeof fl, hipMemcpyDeviceToHost));
            if (fl[1] != 0xffffffffu) {
                td_set_bad_index(fl[1]);
                return td_fail_internal(TD_E_OVERLAP, ("tag " + std::to_string(fl[1]) + " equals an earlier tag").c_str());
            }
            TD_HIPCHK(hipMemcpy(perm2.p, ident.data(), (uint64_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
            TD_HIPCHK(hipMemset(differ.p, 0, 3 * sizeof(uint32_t)));
            TD_HIPCHK(tdrs::rs_sort(key.p + n, len.p, n, 2, &perm2.p, &perm1.p, differ.p, hist.p, &passes));
            TD_HIPCHK(hipEventRecord(ev.e[2], 0));
            // ---- K3
            const uint32_t nrb = (n + TN_TILE - 1) / TN_TILE;
            TnOrder ord[2];
            int rc;
            if ((rc = tn_prepare(key.p, dcnt.p, perm0.p, n, nrb, ord[0], ctr.p))) return rc;
            if ((rc = tn_prepare(key.p + n, dcnt.p, perm2.p, n, nrb, ord[1], ctr.p))) return rc;
            TD_HIPCHK(hipEventRecord(ev.e[3], 0));
            unsigned long long compares = 0;
            TD_HIPCHK(hipMemcpy(&compares, ctr.p, sizeof compares, hipMemcpyDeviceToHost));
            for (auto &o : ord) TD_HIPCHK(hipMemcpy(&o.ntiles, o.tile_off.p + nrb, sizeof(uint32_t), hipMemcpyDeviceToHost));
            st[7] = compares;
            const uint64_t cap_opt = td_handle_tagnet_max_compares(h);
            const uint64_t max_compares = cap_opt ? cap_opt : (uint64_t)TD_TAGNET_DEFAULT_MAX_COMPARES;
            if (compares > max_compares) {
                if (stats) stats[0] = n, stats[7] = compares;
                return td_fail_internal(TD_E_LIMIT, ("tag network: compares = " + std::to_string(compares) +
                                                     " exceed the cap tagnet_max_compares = " + std::to_string(max_compares)).c_str());
            }
            // a row block reaches at most one column block more than its compares / 256^2 account for, twice over
            if (2ull * nrb + compares / (TN_TILE * TN_TILE / 2) > TN_MAX_TILES)
                return td_fail_internal(TD_E_LIMIT, "tag network: more tiles than one launch takes");
            // ---- K4
            const uint64_t bound = (3ull * L * n + 1) / 2;
            const uint64_t ecap = std::min<uint64_t>(bound, compares);
            TD_HIPCHK(deg.alloc(n));
            TD_HIPCHK(hipMemset(deg.p, 0, (uint64_t)n * sizeof(uint32_t)));
            TD_HIPCHK(edges.alloc(ecap));
            TD_HIPCHK(pairs.alloc(n / 2 + 1ull));
            for (auto &o : ord) {
                if (!o.ntiles) continue;
                hipLaunchKernelGGL(k_tn_compare, dim3(o.ntiles), dim3(TN_TILE), 0, 0, o.other.p, o.cnt.p, o.idx.p, o.end.p,
                                   o.tile_off.p, nrb, n, ratio_ppm, edges.p, ecap, ctr.p + 1, deg.p, flags.p + 2);
                TD_HIPCHK(hipGetLastError());
            }
            TD_HIPCHK(hipEventRecord(ev.e[4], 0));
            unsigned long long nedges = 0;
            TD_HIPCHK(hipMemcpy(&nedges, ctr.p + 1, sizeof nedges, hipMemcpyDeviceToHost));
            TD_HIPCHK(hipMemcpy(fl, flags.p, sizeof fl, hipMemcpyDeviceToHost));
            if (fl[2] || nedges > ecap)
                return td_fail_internal(TD_E_INTERNAL, ("tag network: " + std::to_string(nedges) + " edges, more than the bound of " +
                                                        std::to_string(ecap)).c_str());
            // ---- K5
            if (nedges) {
                hipLaunchKernelGGL(k_tn_select, dim3((uint32_t)((nedges + 255) / 256)), block, 0, 0, edges.p, (uint64_t)nedges, deg.p,
                                   pairs.p, n / 2 + 1ull, ctr.p + 2, flags.p + 2);
                TD_HIPCHK(hipGetLastError());
            }
            TD_HIPCHK(hipEventRecord(ev.e[5], 0));
            TD_HIPCHK(hipEventSynchronize(ev.e[5]));
            unsigned long long npairs = 0;
            TD_HIPCHK(hipMemcpy(&npairs, ctr.p + 2, sizeof npairs, hipMemcpyDeviceToHost));
            TD_HIPCHK(hipMemcpy(fl, flags.p, sizeof fl, hipMemcpyDeviceToHost));
            if (fl[2] || npairs > n / 2)
                return td_fail_internal(TD_E_INTERNAL, "tag network: more pairs than half the tags");
            const auto t0 = std::chrono::steady_clock::now();
            net->edges.resize(nedges);
            net->pairs.resize(npairs);
            if (nedges) TD_HIPCHK(hipMemcpy(net->edges.data(), edges.p, nedges * sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (npairs) TD_HIPCHK(hipMemcpy(net->pairs.data(), pairs.p, npairs * sizeof(uint64_t), hipMemcpyDeviceToHost));
            TD_HIPCHK(hipMemcpy(net->deg.data(), deg.p, (uint64_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            std::sort(net->edges.begin(), net->edges.end(), tn_less);
            std::sort(net->pairs.begin(), net->pairs.end());
            if (ms) {
                ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                for (int k = 0; k < 5; ++k) ms[k] = ev.elapsed(k, k + 1);
            }
            st[1] = nedges;
            st[6] = npairs;
            st[3] = 0;
            for (uint64_t e : net->edges) st[2] += e >> 63;
            for (uint32_t d : net->deg) st[d == 0 ? 3 : d == 1 ? 4 : 5] += 1;
        } else {
            TD_HIPCHK(hipEventSynchronize(ev.e[1]));
            if (ms) ms[0] = ev.elapsed(0, 1);
        }
    }
    if (stats) for (int k = 0; k < 8; ++k) stats[k] = st[k];
    guard.p = nullptr;
    *out = net;
    return TD_OK;
}

static int tn_fetch(const std::vector<uint64_t> &recs, bool kept_only, uint32_t *ij_out, uint64_t capacity, uint64_t *n_out) {
    uint64_t k = 0;
    for (uint64_t e : recs) {
        if (kept_only && !(e & TN_KEPT)) continue;
        if (k < capacity) {
            ij_out[2 * k] = (uint32_t)((e & ~TN_KEPT) >> 32);
            ij_out[2 * k + 1] = (uint32_t)e;
        }
        ++k;
    }
    *n_out = k;
    return TD_OK;
}

extern "C" int td_tagnet_edges(td_handle *h, const td_tagnet *net, int kept_only, uint32_t *ij_out, uint64_t capacity,
                               uint64_t *n_out) {
    if (!h || !net || !n_out || (capacity && !ij_out)) return td_fail_internal(TD_E_ARG, "NULL argument");
    return tn_fetch(net->edges, kept_only != 0, ij_out, capacity, n_out);
}

extern "C" int td_tagnet_pairs(td_handle *h, const td_tagnet *net, uint32_t *ij_out, uint64_t capacity, uint64_t *n_out) {
    if (!h || !net || !n_out || (capacity && !ij_out)) return td_fail_internal(TD_E_ARG, "NULL argument");
    return tn_fetch(net->pairs, false, ij_out, capacity, n_out);
}

extern "C" int td_tagnet_degrees(td_handle *h, const td_tagnet *net, uint32_t *deg_out) {
    if (!h || !net || (net->n && !deg_out)) return td_fail_internal(TD_E_ARG, "NULL argument");
    std::copy(net->deg.begin(), net->deg.end(), deg_out);
    return TD_OK;
}

extern "C" int td_tagnet_free(td_handle *h, td_tagnet *net) {
    (void)h;
    delete net;
    return TD_OK;
}
