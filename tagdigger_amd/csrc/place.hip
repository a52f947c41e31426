// Tag placement on the GPU (include/tagdig.h: td_place_sites, td_place_loci, td_place_tags, td_place_free): the in-silico
// digest of a framed genome, the window of L <= 64 bases behind every cut site on both strands, and the join of n tags
// against those windows at up to 3 mismatches.  The rule is DESIGN 4.20 and the header's; it is restated in
// tagdigger_fun._place_host and, by brute force, in tests/place_cases.py.
//
// Site scan.  The positions x = -64 .. seq_bytes - 1 are cut into tiles of PL_TILE; a workgroup stages its tile and a halo
// of 64 bytes in LDS with 16-byte loads (bytes outside the genome are 0 and match nothing) and every thread looks at 16
// consecutive x: forward, G[x ...] against every remnant; reverse, G[... x + L) against every reverse-complemented
// remnant.  A hit lane (about one position in 500) finds its record by binary search in the record starts, checks the
// bounds and the alphabet of its L window bytes, and counts what it drops.
//   k_pl_count  the loci of every tile (and the four statistics)
//   k_rs_scan   exclusive scan of the tile counts (radix_sort.hpp)
//   k_pl_emit   the same test again; a block scan of the threads' counts gives every locus its id, so loci come out in
//               (x, strand) order without a sort, look-back or spin.  Writes x, record << 1 | strand and the window packed
//               2 bits a base (A 0, C 1, G 2, T 3; base b in word b >> 5, bits 2 (b & 31); reverse-complemented for the
//               reverse strand), word-major as radix_sort.hpp reads keys.
// Window dedupe.  The loci are sorted by window (stable: equal windows stay in locus order); k_pl_heads marks the first
// of every run of equal windows (count, scan, emit again) and leaves (window, first locus id); k_pl_mult the run lengths.
// Join, for k mismatches: P = k + 1 parts, part p = bases [p L / P, (p + 1) L / P).
//   k_pl_part   the distinct windows' keys masked to part p; sorted by it, k_pl_gather lays the masked key, the window,
//               its multiplicity and first locus out in that order.  A place keeps these tables per k.
//   k_pl_pack   the tags, packed like the windows; a byte outside ACGT is flagged with the tag's index
//   k_pl_runs   every tag finds the run of windows with its masked key by two binary searches; the run lengths sum to
//               `compares`, and a run of m windows is ceil(m / PL_CHUNK) work items.  k_rs_scan numbers the items.
//   k_pl_join   one wave per item: its lanes walk the item's windows 64 at a time, d = popcount((x | x >> 1) & 0x5555...)
//               over both words; a pair within k that agrees on no lower part is this part's to report.  The wave sums the
//               multiplicities per distance and takes the minimum of d << 56 | first locus id, and lane 0 commits them
//               with an integer atomicAdd and a 64-bit atomicMin: both are order-independent.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "radix_sort.hpp"
#include "td_internal.hpp"

namespace {

constexpr int PL_TILE = 4096;                      // positions of a scan tile
constexpr int PL_HALO = 64;                        // >= L - 1, a multiple of 16
constexpr int PL_THREADS = 256;
constexpr int PL_PER = PL_TILE / PL_THREADS;       // positions of a thread
constexpr int PL_CHUNK = 1024;                     // windows of a run that one wave compares: a longer run spans several
constexpr uint64_t PL_ODD = 0x5555555555555555ull;
constexpr uint64_t PL_MAX_ITEMS = 0x7fffffffull;
static_assert(PL_PER == 16, "a thread's loci fit a 32-bit mask");
static_assert(PL_HALO >= TD_PLACE_MAX_TAGLEN - 1 && PL_HALO % 16 == 0 && PL_TILE % 16 == 0, "halo");

struct PlRem {                                     // remnants and their reverse complements: staged in LDS by the scan
    uint8_t f[TD_PLACE_MAX_SITES][TD_PLACE_MAX_TAGLEN];
    uint8_t r[TD_PLACE_MAX_SITES][TD_PLACE_MAX_TAGLEN];
    uint8_t len[TD_PLACE_MAX_SITES];
    uint32_t q;
};

struct PlMasks {                                   // part p of this k: its bases as 2-bit fields, and as the odd bit of each
    uint64_t key[4][2];
    uint64_t odd[4][2];
};

// one sorted part: the distinct windows in the order of their masked key
struct PlPart {
    tdi::DevBuf<uint64_t> m, w;                    // 2 D each, word-major: masked key, window
    tdi::DevBuf<uint32_t> mult, first;
};
struct PlPartSet { bool built = false; PlPart part[4]; };

}  // namespace

struct td_place {
    td_handle *h = nullptr;
    uint32_t L = 0, R = 0;
    uint64_t n = 0, D = 0;                         // loci, distinct windows
    uint64_t stats[8] = {};
    tdi::DevBuf<uint64_t> x, key, dkey;            // n; 2 n word-major; 2 D word-major
    tdi::DevBuf<uint32_t> rs, dmult, dfirst;       // n: record << 1 | strand; D; D
    PlPartSet sets[TD_PLACE_MAX_MISMATCH + 1];     // by k
};

namespace {

// the places alive on a handle: td_destroy frees those still open
struct Places : tdi::ModuleState {
    std::vector<td_place *> all;
    ~Places() override { for (td_place *pl : all) delete pl; }
};
Places *places_of(td_handle *h, bool make) {
    std::unique_ptr<tdi::ModuleState> &slot = tdi::module_slot(h, tdi::PLACES);
    if (!slot && make) slot.reset(new Places());
    return static_cast<Places *>(slot.get());
}

// ------------------------------------------------------------------ site scan
__device__ __forceinline__ void pl_stage(const uint8_t *g, uint64_t nbytes, int64_t base, uint8_t *s, const PlRem *rem, PlRem *s_rem) {
    const bool aligned = ((uintptr_t)g & 15u) == 0;
    for (int grp = threadIdx.x; grp < (PL_TILE + PL_HALO) / 16; grp += PL_THREADS) {
        const int64_t g0 = base + 16 * grp;
        if (aligned && g0 >= 0 && (uint64_t)g0 + 16 <= nbytes) {
            *(uint4 *)(s + 16 * grp) = *(const uint4 *)(g + g0);
        } else {
            for (int i = 0; i < 16; ++i) {
                const int64_t gi = g0 + i;
                s[16 * grp + i] = gi >= 0 && (uint64_t)gi < nbytes ? g[gi] : (uint8_t)0;
            }
        }
    }
    const uint32_t *src = (const uint32_t *)rem;
    uint32_t *dst = (uint32_t *)s_rem;
    for (uint32_t i = threadIdx.x; i < sizeof(PlRem) / 4; i += PL_THREADS) dst[i] = src[i];
    __syncthreads();
}

__device__ __forceinline__ bool pl_match(const uint8_t *s, const uint8_t *c, int len) {
    for (int i = 0; i < len; ++i)
        if (s[i] != c[i]) return false;
    return true;
}

// the last record r < R with rec_start[r] <= v (v < rec_start[R], R >= 1)
__device__ __forceinline__ uint32_t pl_record(const uint64_t *rec_start, uint32_t R, uint64_t v) {
    uint32_t lo = 0, hi = R;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rec_start[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// a remnant hit at LDS offset j (genome offset x) on `strand`: 1 a locus (*rec its record), 2 its window leaves the
// record, 3 its window holds a byte outside ACGT
__device__ int pl_classify(const uint8_t *s, int j, int64_t x, int strand, int L, const uint64_t *rec_start, uint32_t R, uint32_t *rec) {
    if (x < 0) return 2;                                                  // (a reverse hit whose window starts before the genome)
    uint32_t r;
    if (strand == 0) {
        r = pl_record(rec_start, R, (uint64_t)x);
        if ((uint64_t)x + L > rec_start[r + 1]) return 2;
    } else {
        r = pl_record(rec_start, R, (uint64_t)x + L - 1);
        if ((uint64_t)x < rec_start[r]) return 2;
    }
    for (int i = 0; i < L; ++i) {
        const uint8_t c = s[j + i];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return 3;
    }
    *rec = r;
    return 1;
}

// the loci among this thread's 16 positions: bit 2 i forward, bit 2 i + 1 reverse at position 16 t + i; drop[0], drop[1]
// count what was dropped for bounds and alphabet
__device__ uint32_t pl_thread_loci(const uint8_t *s, const PlRem *rem, int64_t base, int L, const uint64_t *rec_start, uint32_t R,
                                   uint32_t *drop) {
    uint32_t mask = 0;
    const int q = (int)rem->q;
    for (int i = 0; i < PL_PER; ++i) {
        const int j = threadIdx.x * PL_PER + i;
        bool fwd = false, rev = false;
        for (int c = 0; c < q; ++c) {
            const int len = rem->len[c];
            fwd = fwd || pl_match(s + j, rem->f[c], len);
            rev = rev || pl_match(s + j + L - len, rem->r[c], len);
        }
        if (!fwd && !rev) continue;
        uint32_t rec;
        if (fwd) {
            const int v = pl_classify(s, j, base + j, 0, L, rec_start, R, &rec);
            if (v == 1) mask |= 1u << (2 * i); else drop[v - 2] += 1;
        }
        if (rev) {
            const int v = pl_classify(s, j, base + j, 1, L, rec_start, R, &rec);
            if (v == 1) mask |= 2u << (2 * i); else drop[v - 2] += 1;
        }
    }
    return mask;
}

// ctr: [0] forward loci, [1] reverse loci, [2] dropped for bounds, [3] dropped for the alphabet
__global__ __launch_bounds__(PL_THREADS) void k_pl_count(const uint8_t *g, uint64_t nbytes, const uint64_t *rec_start, uint32_t R,
                                                         const PlRem *rem, int L, uint32_t *tile_cnt, unsigned long long *ctr) {
    __shared__ __attribute__((aligned(16))) uint8_t s[PL_TILE + PL_HALO];
    __shared__ PlRem s_rem;
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    const int64_t base = (int64_t)blockIdx.x * PL_TILE - PL_HALO;
    pl_stage(g, nbytes, base, s, rem, &s_rem);
    uint32_t drop[2] = {0, 0};
    const uint32_t mask = pl_thread_loci(s, &s_rem, base, L, rec_start, R, drop);
    uint32_t v[4] = {(uint32_t)__popc(mask & 0x55555555u), (uint32_t)__popc(mask & 0xaaaaaaaau), drop[0], drop[1]};
    for (int k = 0; k < 4; ++k)
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < 4; ++k)
            if (v[k]) atomicAdd(&ctr[k], (unsigned long long)v[k]);
        if (v[0] + v[1]) atomicAdd(&s_sum, v[0] + v[1]);
    }
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_sum;
}

__device__ __forceinline__ uint64_t pl_code(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }

// exclusive scan of one value per thread over the workgroup (256 threads)
__device__ __forceinline__ uint32_t pl_block_excl(uint32_t mine, uint32_t *part) {
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < PL_THREADS; d <<= 1) {
        const uint32_t v = threadIdx.x >= (uint32_t)d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    return part[threadIdx.x] - mine;
}

// tile_off: the scanned tile counts; n: all loci (every write is checked against it)
__global__ __launch_bounds__(PL_THREADS) void k_pl_emit(const uint8_t *g, uint64_t nbytes, const uint64_t *rec_start, uint32_t R,
                                                        const PlRem *rem, int L, const uint32_t *tile_off, uint32_t n, uint64_t *x_out,
                                                        uint32_t *rs_out, uint64_t *key) {
    __shared__ __attribute__((aligned(16))) uint8_t s[PL_TILE + PL_HALO];
    __shared__ PlRem s_rem;
    __shared__ uint32_t part[PL_THREADS];
    const int64_t base = (int64_t)blockIdx.x * PL_TILE - PL_HALO;
    pl_stage(g, nbytes, base, s, rem, &s_rem);
    uint32_t drop[2] = {0, 0};
    uint32_t mask = pl_thread_loci(s, &s_rem, base, L, rec_start, R, drop);
    uint32_t id = tile_off[blockIdx.x] + pl_block_excl((uint32_t)__popc(mask), part);
    while (mask) {
        const int bit = __ffs(mask) - 1;
        mask &= mask - 1;
        const int j = threadIdx.x * PL_PER + (bit >> 1), strand = bit & 1;
        const uint64_t x = (uint64_t)(base + j);
        const uint32_t rec = pl_record(rec_start, R, strand ? x + L - 1 : x);
        uint64_t w[2] = {0, 0};
        for (int b = 0; b < L; ++b) {
            const uint64_t v = strand ? 3u - pl_code(s[j + L - 1 - b]) : pl_code(s[j + b]);
            w[b >> 5] |= v << (2 * (b & 31));
        }
        if (id < n) {
            x_out[id] = x;
            rs_out[id] = rec << 1 | (uint32_t)strand;
            key[id] = w[0];
            key[(uint64_t)n + id] = w[1];
        }
        ++id;
    }
}

// ------------------------------------------------------------------ window dedupe
// sorted position p heads a run of equal windows; 16 consecutive positions per thread, 4 096 per workgroup.
// EMIT false: blk_cnt[b] = heads of workgroup b.  EMIT true: blk_cnt holds the scanned counts; head number d gets
// headpos[d] = p, its window and its first locus (the sort is stable, so perm[p] is the run's smallest id)
template <bool EMIT>
__global__ __launch_bounds__(PL_THREADS) void k_pl_heads(const uint64_t *key, const uint32_t *perm, uint32_t n, uint32_t *blk_cnt,
                                                         uint32_t D, uint32_t *headpos, uint64_t *dkey, uint32_t *dfirst) {
    __shared__ uint32_t part[PL_THREADS];
    const uint64_t p0 = (uint64_t)blockIdx.x * PL_TILE + (uint64_t)threadIdx.x * PL_PER;
    uint32_t mask = 0;
    uint64_t a0 = 0, a1 = 0;
    if (p0 > 0 && p0 < n) {
        const uint32_t u = perm[p0 - 1];
        a0 = key[u];
        a1 = key[(uint64_t)n + u];
    }
    for (int i = 0; i < PL_PER; ++i) {
        const uint64_t p = p0 + i;
        if (p >= n) break;
        const uint32_t v = perm[p];
        const uint64_t b0 = key[v], b1 = key[(uint64_t)n + v];
        if (p == 0 || b0 != a0 || b1 != a1) mask |= 1u << i;
        a0 = b0;
        a1 = b1;
    }
    if (!EMIT) {
        uint32_t c = (uint32_t)__popc(mask);
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
        part[threadIdx.x] = 0;
        __syncthreads();
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) blk_cnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
    } else {
        uint32_t d = blk_cnt[blockIdx.x] + pl_block_excl((uint32_t)__popc(mask), part);
        while (mask) {
            const int i = __ffs(mask) - 1;
            mask &= mask - 1;
            const uint32_t v = perm[p0 + i];
            if (d < D) {
                headpos[d] = (uint32_t)(p0 + i);
                dkey[d] = key[v];
                dkey[(uint64_t)D + d] = key[(uint64_t)n + v];
                dfirst[d] = v;
            }
            ++d;
        }
    }
}

__global__ __launch_bounds__(256) void k_pl_mult(const uint32_t *headpos, uint32_t D, uint32_t n, uint32_t *dmult) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    dmult[d] = (d + 1 < D ? headpos[d + 1] : n) - headpos[d];
}

__global__ __launch_bounds__(256) void k_pl_iota(uint32_t *perm, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = i;
}

// ------------------------------------------------------------------ join
__global__ __launch_bounds__(256) void k_pl_part(const uint64_t *dkey, uint32_t D, uint64_t m0, uint64_t m1, uint64_t *mkey) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D) return;
    mkey[i] = dkey[i] & m0;
    mkey[(uint64_t)D + i] = dkey[(uint64_t)D + i] & m1;
}

__global__ __launch_bounds__(256) void k_pl_gather(const uint64_t *dkey, const uint64_t *mkey, const uint32_t *dmult, const uint32_t *dfirst,
                                                   const uint32_t *perm, uint32_t D, uint64_t *m, uint64_t *w, uint32_t *mult,
                                                   uint32_t *first) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D) return;
    const uint32_t v = perm[p];
    m[p] = mkey[v];
    m[(uint64_t)D + p] = mkey[(uint64_t)D + v];
    w[p] = dkey[v];
    w[(uint64_t)D + p] = dkey[(uint64_t)D + v];
    mult[p] = dmult[v];
    first[p] = dfirst[v];
}

__global__ __launch_bounds__(256) void k_pl_pack(const uint8_t *seqs, uint32_t n, uint32_t L, uint64_t *tkey, uint32_t *bad_first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *s = seqs + (uint64_t)i * L;
    uint64_t w[2] = {0, 0};
    bool bad = false;
    for (uint32_t b = 0; b < L; ++b) {
        const uint32_t c = s[b];
        const uint64_t v = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
        if (v == 4u) bad = true;
        w[b >> 5] |= (v & 3u) << (2 * (b & 31));
    }
    tkey[i] = w[0];
    tkey[(uint64_t)n + i] = w[1];
    if (bad) atomicMin(bad_first, i);
}

// the first position in the sorted masked keys that is not below (a0, a1) [upper false] or above it [upper true]
__device__ __forceinline__ uint32_t pl_bound(const uint64_t *m, uint32_t D, uint64_t a0, uint64_t a1, bool upper) {
    uint32_t lo = 0, hi = D;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint64_t b0 = m[mid], b1 = m[(uint64_t)D + mid];
        const bool below = b0 < a0 || (b0 == a0 && (upper ? b1 <= a1 : b1 < a1));
        if (below) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// run[t], run[n + t] = the run of tag t in this part's order; items[t] = its work items (items[n] = 0: the scan leaves
// the total there)
__global__ __launch_bounds__(256) void k_pl_runs(const uint64_t *tkey, uint32_t n, const uint64_t *m, uint32_t D, uint64_t m0, uint64_t m1,
                                                 uint32_t *run, uint32_t *items, unsigned long long *compares) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t mine = 0;
    if (t < n) {
        const uint64_t a0 = tkey[t] & m0, a1 = tkey[(uint64_t)n + t] & m1;
        const uint32_t lo = pl_bound(m, D, a0, a1, false);
        uint32_t hi = lo;
        if (lo < D && m[lo] == a0 && m[(uint64_t)D + lo] == a1) hi = pl_bound(m, D, a0, a1, true);
        run[t] = lo;
        run[(uint64_t)n + t] = hi;
        items[t] = (hi - lo + PL_CHUNK - 1) / PL_CHUNK;
        mine = hi - lo;
    } else if (t == n) {
        items[t] = 0;
    }
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(compares, (unsigned long long)mine);
}

// one wave per work item; item_off[n] = nitems
__global__ __launch_bounds__(256) void k_pl_join(const uint64_t *tkey, uint32_t n, const uint32_t *run, const uint32_t *item_off,
                                                 uint32_t nitems, const uint64_t *w, const uint32_t *mult, const uint32_t *first,
                                                 uint32_t D, uint32_t k, uint32_t p, PlMasks masks, uint32_t *n_at,
                                                 unsigned long long *best) {
    const uint32_t item = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (item >= nitems) return;                                           // (per wave; the kernel has no barrier)
    // the tag of this item: the last t < n with item_off[t] <= item (a tag without items shares its offset with the next)
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (item_off[mid] <= item) lo = mid; else hi = mid;
    }
    const uint32_t t = lo;
    const uint64_t a0 = tkey[t], a1 = tkey[(uint64_t)n + t];
    const uint32_t begin = run[t] + (item - item_off[t]) * PL_CHUNK;
    const uint32_t run_end = run[(uint64_t)n + t];
    const uint32_t end = run_end - begin > (uint32_t)PL_CHUNK ? begin + PL_CHUNK : run_end;   // <= D
    uint32_t cnt[4] = {0, 0, 0, 0};
    unsigned long long mn = ~0ull;
    for (uint32_t c = begin + lane; c < end; c += 64) {
        const uint64_t x0 = a0 ^ w[c], x1 = a1 ^ w[(uint64_t)D + c];
        const uint64_t d0 = (x0 | (x0 >> 1)) & PL_ODD, d1 = (x1 | (x1 >> 1)) & PL_ODD;
        const uint32_t d = (uint32_t)(__popcll(d0) + __popcll(d1));
        if (d > k) continue;
        bool lower = false;                                               // agrees on a part below p: reported there
        for (uint32_t q = 0; q < p; ++q) lower = lower || ((d0 & masks.odd[q][0]) | (d1 & masks.odd[q][1])) == 0;
        if (lower) continue;
        const uint32_t mu = mult[c];
        cnt[0] += d == 0 ? mu : 0u;
        cnt[1] += d == 1 ? mu : 0u;
        cnt[2] += d == 2 ? mu : 0u;
        cnt[3] += d == 3 ? mu : 0u;
        const unsigned long long v = (unsigned long long)d << 56 | first[c];
        mn = v < mn ? v : mn;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        for (int q = 0; q < 4; ++q) cnt[q] += __shfl_xor(cnt[q], s, 64);
        const unsigned long long o = __shfl_xor(mn, s, 64);
        mn = o < mn ? o : mn;
    }
    if (lane == 0 && mn != ~0ull) {
        for (int q = 0; q < 4; ++q)
            if (cnt[q]) atomicAdd(&n_at[4ull * t + q], cnt[q]);
        atomicMin(&best[t], mn);
    }
}

// part p of k + 1 over L bases
void pl_masks(uint32_t L, uint32_t k, PlMasks &mk) {
    memset(&mk, 0, sizeof mk);
    const uint32_t P = k + 1;
    for (uint32_t p = 0; p < P; ++p)
        for (uint32_t b = p * L / P; b < (p + 1) * L / P; ++b) {
            mk.key[p][b >> 5] |= 3ull << (2 * (b & 31));
            mk.odd[p][b >> 5] |= 1ull << (2 * (b & 31));
        }
}

// perm0 <- the identity sorted by the two-word keys (D entries); len: D zeroed lengths
int pl_sort(const uint64_t *key, const uint16_t *len, uint32_t D, uint32_t **perm0, uint32_t **perm1, uint32_t *differ, uint32_t *hist) {
    hipLaunchKernelGGL(k_pl_iota, dim3((D + 255) / 256), dim3(256), 0, 0, *perm0, D);
    TD_HIPCHK(hipGetLastError());
    if (D > 1) {
        uint32_t passes = 0;
        TD_HIPCHK(hipMemset(differ, 0, 3 * sizeof(uint32_t)));
        TD_HIPCHK(tdrs::rs_sort(key, len, D, 2, perm0, perm1, differ, hist, &passes));
    }
    return TD_OK;
}

// the sorted window tables of every part of this k
// (e0 .. e1 bracket the launches: the allocations lie before e0)
int pl_build_parts(td_place *pl, uint32_t k, const PlMasks &mk, hipEvent_t e0, hipEvent_t e1) {
    PlPartSet &set = pl->sets[k];
    const uint32_t D = (uint32_t)pl->D;
    tdi::DevBuf<uint64_t> mkey;
    tdi::DevBuf<uint16_t> len;
    tdi::DevBuf<uint32_t> perm0, perm1, differ, hist;
    TD_HIPCHK(mkey.alloc(2ull * D));
    TD_HIPCHK(len.alloc(D));
    TD_HIPCHK(perm0.alloc(D));
    TD_HIPCHK(perm1.alloc(D));
    TD_HIPCHK(differ.alloc(3));
    TD_HIPCHK(hist.alloc(256ull * tdrs::rs_blocks(D)));
    TD_HIPCHK(hipMemset(len.p, 0, (uint64_t)D * sizeof(uint16_t)));
    const dim3 grid((D + 255) / 256), block(256);
    for (uint32_t p = 0; p <= k; ++p) {
        PlPart &pt = set.part[p];
        TD_HIPCHK(pt.m.ensure(2ull * D));
        TD_HIPCHK(pt.w.ensure(2ull * D));
        TD_HIPCHK(pt.mult.ensure(D));
        TD_HIPCHK(pt.first.ensure(D));
    }
    TD_HIPCHK(hipEventRecord(e0, 0));
    for (uint32_t p = 0; p <= k; ++p) {
        PlPart &pt = set.part[p];
        hipLaunchKernelGGL(k_pl_part, grid, block, 0, 0, pl->dkey.p, D, mk.key[p][0], mk.key[p][1], mkey.p);
        TD_HIPCHK(hipGetLastError());
        int rc;
        if ((rc = pl_sort(mkey.p, len.p, D, &perm0.p, &perm1.p, differ.p, hist.p))) return rc;
        hipLaunchKernelGGL(k_pl_gather, grid, block, 0, 0, pl->dkey.p, mkey.p, pl->dmult.p, pl->dfirst.p, perm0.p, D, pt.m.p, pt.w.p,
                           pt.mult.p, pt.first.p);
        TD_HIPCHK(hipGetLastError());
    }
    TD_HIPCHK(hipEventRecord(e1, 0));
    TD_HIPCHK(hipEventSynchronize(e1));                                   // (the temporaries go with this scope)
    set.built = true;
    return TD_OK;
}

uint8_t pl_comp(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

}  // namespace

extern "C" int td_place_sites(td_handle *h, const void *d_seq, uint64_t seq_bytes, const uint64_t *rec_start, uint32_t R,
                              const char *const *remnants, uint32_t n_remnants, uint32_t taglen, td_place **out, uint64_t stats[8],
                              double *ms) {
    if (!h || !out || !rec_start || !remnants || (seq_bytes && !d_seq)) return td_fail_internal(TD_E_ARG, "NULL argument");
    *out = nullptr;
    if (stats) for (int k = 0; k < 8; ++k) stats[k] = 0;
    if (ms) for (int k = 0; k < 4; ++k) ms[k] = 0;
    if (taglen < 1 || taglen > TD_PLACE_MAX_TAGLEN) return td_fail_internal(TD_E_ARG, "taglen must be 1..64");
    if (n_remnants < 1 || n_remnants > TD_PLACE_MAX_SITES) return td_fail_internal(TD_E_ARG, "1..16 remnants are needed");
    if (R >= 0x80000000u) return td_fail_internal(TD_E_LIMIT, "2^31 records or more");
    if (rec_start[0] != 0 || rec_start[R] != seq_bytes) return td_fail_internal(TD_E_ARG, "rec_start must run from 0 to seq_bytes");
    for (uint32_t r = 0; r < R; ++r)
        if (rec_start[r] > rec_start[r + 1]) return td_fail_internal(TD_E_ARG, "rec_start must not decrease");
    const uint32_t L = taglen;
    PlRem rem;
    memset(&rem, 0, sizeof rem);
    rem.q = n_remnants;
    for (uint32_t c = 0; c < n_remnants; ++c) {
        const char *s = remnants[c];
        const size_t len = s ? strlen(s) : 0;
        if (len < 1 || len > L) return td_fail_internal(TD_E_ARG, "a remnant must have 1..taglen bases");
        for (size_t i = 0; i < len; ++i) {
            if (!strchr("ACGT", s[i])) return td_fail_internal(TD_E_ARG, "a remnant holds a character outside ACGT");
            rem.f[c][i] = (uint8_t)s[i];
            rem.r[c][len - 1 - i] = pl_comp((uint8_t)s[i]);
        }
        rem.len[c] = (uint8_t)len;
    }
    std::unique_ptr<td_place> pl(new td_place);
    pl->h = h;
    pl->L = L;
    pl->R = R;
    pl->stats[TD_PLACE_RECORDS] = R;
    if (seq_bytes) {
        TD_HIPCHK(hipSetDevice(td_handle_device(h)));
        const uint64_t ntiles64 = (seq_bytes + PL_HALO + PL_TILE - 1) / PL_TILE;
        if (ntiles64 > 0x7ffffffeull) return td_fail_internal(TD_E_LIMIT, "genome too long for one scan");
        const uint32_t ntiles = (uint32_t)ntiles64;
        tdi::Events<8> ev;
        TD_HIPCHK(ev.create());
        tdi::DevBuf<uint64_t> d_rec;
        tdi::DevBuf<uint32_t> tile_cnt;
        tdi::DevBuf<unsigned long long> ctr;
        tdi::DevBuf<PlRem> d_rem;
        TD_HIPCHK(d_rem.alloc(1));
        TD_HIPCHK(hipMemcpy(d_rem.p, &rem, sizeof rem, hipMemcpyHostToDevice));
        TD_HIPCHK(d_rec.alloc(R + 1ull));
        TD_HIPCHK(tile_cnt.alloc(ntiles + 1ull));
        TD_HIPCHK(ctr.alloc(4));
        TD_HIPCHK(hipMemcpy(d_rec.p, rec_start, (R + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice));
        TD_HIPCHK(hipMemset(ctr.p, 0, 4 * sizeof(unsigned long long)));
        TD_HIPCHK(hipMemset(tile_cnt.p + ntiles, 0, sizeof(uint32_t)));
        TD_HIPCHK(hipEventRecord(ev.e[0], 0));
        hipLaunchKernelGGL(k_pl_count, dim3(ntiles), dim3(PL_THREADS), 0, 0, (const uint8_t *)d_seq, seq_bytes, d_rec.p, R, d_rem.p, (int)L,
                           tile_cnt.p, ctr.p);
        TD_HIPCHK(hipGetLastError());
        TD_HIPCHK(hipEventRecord(ev.e[1], 0));
        unsigned long long c4[4];
        TD_HIPCHK(hipMemcpy(c4, ctr.p, sizeof c4, hipMemcpyDeviceToHost));
        const uint64_t n64 = c4[0] + c4[1];
        pl->stats[TD_PLACE_LOCI] = n64;
        pl->stats[TD_PLACE_FORWARD] = c4[0];
        pl->stats[TD_PLACE_REVERSE] = c4[1];
        pl->stats[TD_PLACE_DROP_BOUNDS] = c4[2];
        pl->stats[TD_PLACE_DROP_ALPHABET] = c4[3];
        if (n64 > TD_PLACE_MAX_LOCI) {
            if (stats) for (int k = 0; k < 8; ++k) stats[k] = pl->stats[k];
            return td_fail_internal(TD_E_LIMIT, (std::to_string(n64) + " loci, more than TD_PLACE_MAX_LOCI = " +
                                                 std::to_string(TD_PLACE_MAX_LOCI)).c_str());
        }
        const uint32_t n = (uint32_t)n64;
        if (n) {
            // (every buffer of a step is allocated before the event that opens it: the times are the launches')
            tdi::DevBuf<uint16_t> len;
            tdi::DevBuf<uint32_t> perm0, perm1, differ, hist, blk, headpos;
            const uint32_t nblk = (n + PL_TILE - 1) / PL_TILE;
            TD_HIPCHK(pl->x.alloc(n));
            TD_HIPCHK(pl->rs.alloc(n));
            TD_HIPCHK(pl->key.alloc(2ull * n));
            TD_HIPCHK(len.alloc(n));
            TD_HIPCHK(perm0.alloc(n));
            TD_HIPCHK(perm1.alloc(n));
            TD_HIPCHK(differ.alloc(3));
            TD_HIPCHK(hist.alloc(256ull * tdrs::rs_blocks(n)));
            TD_HIPCHK(blk.alloc(nblk + 1ull));
            TD_HIPCHK(hipMemset(len.p, 0, (uint64_t)n * sizeof(uint16_t)));
            TD_HIPCHK(hipMemset(blk.p + nblk, 0, sizeof(uint32_t)));
            TD_HIPCHK(hipEventRecord(ev.e[2], 0));
            hipLaunchKernelGGL(tdrs::k_rs_scan, dim3(1), dim3(tdrs::RS_SCAN_THREADS), 0, 0, tile_cnt.p, (uint64_t)ntiles + 1);
            TD_HIPCHK(hipGetLastError());
            TD_HIPCHK(hipEventRecord(ev.e[3], 0));
            hipLaunchKernelGGL(k_pl_emit, dim3(ntiles), dim3(PL_THREADS), 0, 0, (const uint8_t *)d_seq, seq_bytes, d_rec.p, R, d_rem.p, (int)L,
                               tile_cnt.p, n, pl->x.p, pl->rs.p, pl->key.p);
            TD_HIPCHK(hipGetLastError());
            TD_HIPCHK(hipEventRecord(ev.e[4], 0));
            // ---- dedupe (the sort reads its 12 bytes of differing digit positions back in between)
            int rc;
            if ((rc = pl_sort(pl->key.p, len.p, n, &perm0.p, &perm1.p, differ.p, hist.p))) return rc;
            hipLaunchKernelGGL(k_pl_heads<false>, dim3(nblk), dim3(PL_THREADS), 0, 0, pl->key.p, perm0.p, n, blk.p, 0u, nullptr, nullptr,
                               nullptr);
            TD_HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(tdrs::k_rs_scan, dim3(1), dim3(tdrs::RS_SCAN_THREADS), 0, 0, blk.p, (uint64_t)nblk + 1);
            TD_HIPCHK(hipGetLastError());
            TD_HIPCHK(hipEventRecord(ev.e[5], 0));
            uint32_t D = 0;
            TD_HIPCHK(hipMemcpy(&D, blk.p + nblk, sizeof D, hipMemcpyDeviceToHost));
            if (D < 1 || D > n) return td_fail_internal(TD_E_INTERNAL, "place: the distinct windows do not add up");
            TD_HIPCHK(headpos.alloc(D));
            TD_HIPCHK(pl->dkey.alloc(2ull * D));
            TD_HIPCHK(pl->dmult.alloc(D));
            TD_HIPCHK(pl->dfirst.alloc(D));
            TD_HIPCHK(hipEventRecord(ev.e[6], 0));
            hipLaunchKernelGGL(k_pl_heads<true>, dim3(nblk), dim3(PL_THREADS), 0, 0, pl->key.p, perm0.p, n, blk.p, D, headpos.p, pl->dkey.p,
                               pl->dfirst.p);
            TD_HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_pl_mult, dim3((D + 255) / 256), dim3(256), 0, 0, headpos.p, D, n, pl->dmult.p);
            TD_HIPCHK(hipGetLastError());
            TD_HIPCHK(hipEventRecord(ev.e[7], 0));
            TD_HIPCHK(hipEventSynchronize(ev.e[7]));
            pl->n = n;
            pl->D = D;
            pl->stats[TD_PLACE_DISTINCT] = D;
            if (ms) ms[0] = ev.elapsed(0, 1), ms[1] = ev.elapsed(2, 3), ms[2] = ev.elapsed(3, 4), ms[3] = ev.elapsed(4, 5) + ev.elapsed(6, 7);
        } else {
            TD_HIPCHK(hipEventSynchronize(ev.e[1]));
            if (ms) ms[0] = ev.elapsed(0, 1);
        }
    }
    if (stats) for (int k = 0; k < 8; ++k) stats[k] = pl->stats[k];
    places_of(h, true)->all.push_back(pl.get());
    *out = pl.release();
    return TD_OK;
}

extern "C" int td_place_loci(td_handle *h, const td_place *pl, uint64_t *x_out, uint32_t *rec_out, uint8_t *strand_out, char *windows_out) {
    if (!h || !pl) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (pl->h != h) return td_fail_internal(TD_E_ARG, "not a place of this handle");
    const uint64_t n = pl->n;
    if (!n) return TD_OK;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    if (x_out) TD_HIPCHK(hipMemcpy(x_out, pl->x.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (rec_out || strand_out) {
        std::vector<uint32_t> rs(n);
        TD_HIPCHK(hipMemcpy(rs.data(), pl->rs.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; ++i) {
            if (rec_out) rec_out[i] = rs[i] >> 1;
            if (strand_out) strand_out[i] = (uint8_t)(rs[i] & 1u);
        }
    }
    if (windows_out) {
        std::vector<uint64_t> key(2 * n);
        TD_HIPCHK(hipMemcpy(key.data(), pl->key.p, 2 * n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        const uint32_t L = pl->L;
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t b = 0; b < L; ++b)
                windows_out[i * L + b] = "ACGT"[(key[(b >> 5) * n + i] >> (2 * (b & 31))) & 3u];
    }
    return TD_OK;
}

extern "C" int td_place_tags(td_handle *h, td_place *pl, const char *seqs, uint32_t n, uint32_t max_mismatch, uint32_t *n_at_out,
                             uint8_t *dist_out, uint64_t *locus_out, uint64_t stats[8], double *ms) {
    if (!h || !pl || (n && (!seqs || !n_at_out || !dist_out || !locus_out))) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (stats) for (int q = 0; q < 8; ++q) stats[q] = 0;
    if (ms) for (int q = 0; q < 4; ++q) ms[q] = 0;
    if (pl->h != h) return td_fail_internal(TD_E_ARG, "not a place of this handle");
    const uint32_t k = max_mismatch, L = pl->L;
    if (k > TD_PLACE_MAX_MISMATCH) return td_fail_internal(TD_E_ARG, "max_mismatch must be 0..3");
    if (L < k + 1) return td_fail_internal(TD_E_ARG, "the tag length must be at least max_mismatch + 1");
    if (n > (1u << 30)) return td_fail_internal(TD_E_LIMIT, "more than 2^30 tags");
    uint64_t st[8] = {n, 0, 0, n, 0, 0, 0, 0};
    for (uint64_t i = 0; i < 4ull * n; ++i) n_at_out[i] = 0;
    for (uint32_t t = 0; t < n; ++t) dist_out[t] = 255, locus_out[t] = ~0ull;
    if (n && !pl->n) {                                                    // nothing to compare with: the alphabet, on the host
        for (uint64_t i = 0; i < (uint64_t)n * L; ++i)
            if (!memchr("ACGT", seqs[i], 4)) {
                td_set_bad_index((uint32_t)(i / L));
                return td_fail_internal(TD_E_ALPHABET, ("tag " + std::to_string(i / L) + " holds a byte outside ACGT").c_str());
            }
    } else if (n) {
        TD_HIPCHK(hipSetDevice(td_handle_device(h)));
        tdi::Events<8> ev;
        TD_HIPCHK(ev.create());
        tdi::DevBuf<uint8_t> dseq;
        tdi::DevBuf<uint64_t> tkey;
        tdi::DevBuf<uint32_t> flag;
        // ---- pack
        TD_HIPCHK(dseq.alloc((uint64_t)n * L));
        TD_HIPCHK(tkey.alloc(2ull * n));
        TD_HIPCHK(flag.alloc(1));
        TD_HIPCHK(hipMemcpy(dseq.p, seqs, (uint64_t)n * L, hipMemcpyHostToDevice));
        TD_HIPCHK(hipMemset(flag.p, 0xff, sizeof(uint32_t)));
        const dim3 grid((n + 255) / 256), block(256);
        TD_HIPCHK(hipEventRecord(ev.e[0], 0));
        hipLaunchKernelGGL(k_pl_pack, grid, block, 0, 0, dseq.p, n, L, tkey.p, flag.p);
        TD_HIPCHK(hipGetLastError());
        TD_HIPCHK(hipEventRecord(ev.e[1], 0));
        uint32_t bad = 0;
        TD_HIPCHK(hipMemcpy(&bad, flag.p, sizeof bad, hipMemcpyDeviceToHost));
        if (bad != 0xffffffffu) {
            td_set_bad_index(bad);
            return td_fail_internal(TD_E_ALPHABET, ("tag " + std::to_string(bad) + " holds a byte outside ACGT").c_str());
        }
        {
            const uint32_t D = (uint32_t)pl->D, P = k + 1;
            PlMasks mk;
            pl_masks(L, k, mk);
            // ---- the parts' tables
            const bool build = !pl->sets[k].built;
            if (build) {
                const int rc = pl_build_parts(pl, k, mk, ev.e[2], ev.e[3]);
                if (rc) return rc;
            }
            // ---- runs (and the scans that number the work items)
            tdi::DevBuf<uint32_t> run, items, n_at;
            tdi::DevBuf<unsigned long long> ctr, best;
            TD_HIPCHK(run.alloc(2ull * n * P));
            TD_HIPCHK(items.alloc((n + 1ull) * P));
            TD_HIPCHK(ctr.alloc(4));
            TD_HIPCHK(hipMemset(ctr.p, 0, 4 * sizeof(unsigned long long)));
            TD_HIPCHK(n_at.alloc(4ull * n));
            TD_HIPCHK(best.alloc(n));
            TD_HIPCHK(hipMemset(n_at.p, 0, 4ull * n * sizeof(uint32_t)));
            TD_HIPCHK(hipMemset(best.p, 0xff, (uint64_t)n * sizeof(unsigned long long)));
            TD_HIPCHK(hipEventRecord(ev.e[4], 0));
            const dim3 grid1((n + 1 + 255) / 256);
            for (uint32_t p = 0; p < P; ++p) {
                hipLaunchKernelGGL(k_pl_runs, grid1, block, 0, 0, tkey.p, n, pl->sets[k].part[p].m.p, D, mk.key[p][0], mk.key[p][1],
                                   run.p + 2ull * n * p, items.p + (n + 1ull) * p, ctr.p + p);
                hipLaunchKernelGGL(tdrs::k_rs_scan, dim3(1), dim3(tdrs::RS_SCAN_THREADS), 0, 0, items.p + (n + 1ull) * p, (uint64_t)n + 1);
                TD_HIPCHK(hipGetLastError());
            }
            TD_HIPCHK(hipEventRecord(ev.e[5], 0));
            unsigned long long cmp[4];
            uint32_t nitems[4] = {0, 0, 0, 0};
            TD_HIPCHK(hipMemcpy(cmp, ctr.p, sizeof cmp, hipMemcpyDeviceToHost));
            for (uint32_t p = 0; p < P; ++p)
                TD_HIPCHK(hipMemcpy(&nitems[p], items.p + (n + 1ull) * p + n, sizeof(uint32_t), hipMemcpyDeviceToHost));
            const uint64_t compares = cmp[0] + cmp[1] + cmp[2] + cmp[3];
            st[TD_PLACED_COMPARES] = compares;
            const uint64_t cap_opt = td_handle_place_max_compares(h);
            const uint64_t max_compares = cap_opt ? cap_opt : (uint64_t)TD_PLACE_DEFAULT_MAX_COMPARES;
            if (compares > max_compares) {
                if (stats) stats[TD_PLACED_TAGS] = n, stats[TD_PLACED_COMPARES] = compares;
                return td_fail_internal(TD_E_LIMIT, ("tag placement: compares = " + std::to_string(compares) +
                                                     " exceed the cap place_max_compares = " + std::to_string(max_compares)).c_str());
            }
            for (uint32_t p = 0; p < P; ++p)                              // a run of m windows is at most m / 1024 + 1 items
                if (cmp[p] / PL_CHUNK + n > PL_MAX_ITEMS) return td_fail_internal(TD_E_LIMIT, "tag placement: more work items than one launch takes");
            for (uint32_t p = 0; p < P; ++p)
                if ((cmp[p] != 0) != (nitems[p] != 0) || nitems[p] > PL_MAX_ITEMS)
                    return td_fail_internal(TD_E_INTERNAL, "tag placement: the work items do not add up");
            // ---- join
            TD_HIPCHK(hipEventRecord(ev.e[6], 0));
            for (uint32_t p = 0; p < P; ++p) {
                if (!nitems[p]) continue;
                const PlPart &pt = pl->sets[k].part[p];
                hipLaunchKernelGGL(k_pl_join, dim3((nitems[p] + 3) / 4), block, 0, 0, tkey.p, n, run.p + 2ull * n * p,
                                   items.p + (n + 1ull) * p, nitems[p], pt.w.p, pt.mult.p, pt.first.p, D, k, p, mk, n_at.p, best.p);
                TD_HIPCHK(hipGetLastError());
            }
            TD_HIPCHK(hipEventRecord(ev.e[7], 0));
            TD_HIPCHK(hipEventSynchronize(ev.e[7]));
            std::vector<unsigned long long> hb(n);
            TD_HIPCHK(hipMemcpy(n_at_out, n_at.p, 4ull * n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            TD_HIPCHK(hipMemcpy(hb.data(), best.p, (uint64_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            st[TD_PLACED_NONE] = 0;
            for (uint32_t t = 0; t < n; ++t) {
                if (hb[t] == ~0ull) { st[TD_PLACED_NONE] += 1; continue; }
                const uint32_t d = (uint32_t)(hb[t] >> 56);
                dist_out[t] = (uint8_t)d;
                locus_out[t] = hb[t] & ((1ull << 56) - 1);
                st[n_at_out[4ull * t + d] == 1 ? TD_PLACED_UNIQUE : TD_PLACED_MULTI] += 1;
            }
            if (ms) ms[0] = ev.elapsed(0, 1), ms[1] = build ? ev.elapsed(2, 3) : 0.0, ms[2] = ev.elapsed(4, 5), ms[3] = ev.elapsed(6, 7);
        }
    }
    if (stats) for (int q = 0; q < 8; ++q) stats[q] = st[q];
    return TD_OK;
}

extern "C" int td_place_free(td_handle *h, td_place *pl) {
    if (!pl) return TD_OK;
    if (!h) return td_fail_internal(TD_E_ARG, "NULL argument");
    Places *places = places_of(h, false);
    if (!places) return td_fail_internal(TD_E_ARG, "not a place of this handle");
    auto it = std::find(places->all.begin(), places->all.end(), pl);
    if (it == places->all.end()) return td_fail_internal(TD_E_ARG, "not a place of this handle");
    places->all.erase(it);
    (void)hipSetDevice(td_handle_device(h));
    delete pl;
    return TD_OK;
}
