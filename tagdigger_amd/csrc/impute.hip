// LD-kNN imputation of the missing calls (include/tagdig.h: td_impute_knn).
//
// Input: the S x M uint8 call matrix where it lies in device memory (rows exactly M bytes apart), codes 0 / 1 / 2, any
// byte above 2 = missing, and the neighbour table nbr[M][L] (host): row m lists the markers whose calls stand in for
// marker m, -1 = no entry.  For a missing cell (t, m) every sample d called at m is a donor; over the neighbours q at
// which t and d are both called, ovl = their number and dist = the sum of |calls[t][q] - calls[d][q]|.  A donor with
// ovl >= min_overlap weighs w = floor(32768 (2 ovl - dist) / ovl); the first k by (w descending, d ascending) vote with
// their own call at m.  Only the INPUT's calls are read, so every cell is decided on its own.
//
// k_calls_transpose<false> (calls_transpose.hpp, shared with ld.hip) over ALL markers, no compaction: T is Mpad rows of
//    Spad bytes (both multiples of 64), codes 0 / 1 / 2 and 3 for everything else (missing, samples past S, rows past
//    M).  called[m] = the samples called at m falls out of the same pass; S - called[m] are missing there.
// k_impute: one workgroup of 256 threads per marker, decoded from a 2-D grid.  It leaves at once, after writing its
//    statistics, when nobody is missing at m or the row of the table is empty.
//      A. a thread takes samples s, s + 256, ...: it reads byte s of the L neighbour rows of T (the lanes are neighbouring
//         samples: one run of 64 bytes per row and wave) and packs them into three 64-bit words, bit q for neighbour q:
//         C (called), P1 (g >= 1), P2 (g >= 2) -- a thermometer code, so that with B = Ct & Cd
//             ovl = popc(B),  dist = popc(B & (P1t ^ P1d)) + popc(B & (P2t ^ P2d)).
//         The words lie in LDS as three arrays of Spad words (a wave reads 64 consecutive words: no bank conflict), the
//         marker's own codes as Spad bytes behind them: 25 Spad + 272 bytes, 100.3 KiB at S = 4 096.
//      B. a wave per target, lanes over the donors.  The key (w << 12) | (4095 - d) is unique per donor, so the voters are
//         the k largest keys.  Lane x owns the donors x, x + 64, ... and keeps the largest key among those of them that
//         have not voted; a round is a wave-wide maximum of these, and then only the winner's lane needs a new one: its
//         at most 64 donors are looked at by the 64 lanes, one each, and a second maximum gives it.  So a target costs
//         Spad / 64 + k keys a lane, not k Spad / 64.  w is an exact 32-bit integer division.  The winner's w and class
//         are known to the whole wave; the vote and the two comparisons follow in uniform registers, lane 0 writes the byte.
// The output starts as a device copy of the input; the kernel writes imputed cells only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "calls_transpose.hpp"
#include "td_internal.hpp"

namespace {

constexpr uint32_t IM_THREADS = 256;               // 4 waves
constexpr uint32_t IM_WAVES = IM_THREADS / 64;
constexpr uint32_t IM_GRID_X = 65536;              // markers along grid x: a dimension holds fewer than 2^32 threads
constexpr uint32_t IM_TAIL = TD_IMPUTE_MAX_NBR * 4 + 16;   // LDS behind the planes: the table's row, four counters
static_assert(CT_STEP % 64 == 0 && CT_MISSING > 2, "k_impute walks Spad by waves and takes a code above 2 as missing");
static_assert(TD_IMPUTE_MAX_NBR == 64, "a plane is one 64-bit word per sample");
static_assert(TD_IMPUTE_MAX_SAMPLES == 4096, "the key keeps 12 bits for the donor");
static_assert(TD_IMPUTE_MAX_NBR <= IM_THREADS, "one thread loads one entry of the table's row");
static_assert(25u * TD_IMPUTE_MAX_SAMPLES + IM_TAIL <= 160u * 1024u, "the planes of TD_IMPUTE_MAX_SAMPLES fit a CU's LDS");

// the transpose and the vote kernel (device ms) of the calling thread's last td_impute_knn
thread_local double g_im_times[2] = {0, 0};

// the key of donor d for a target with planes (ct, t1, t2): (w << 12) | (4095 - d), or -1 when d is not called at the marker
// (the target itself and the samples past S included) or shares fewer than min_overlap called neighbours with the target
__device__ __forceinline__ int im_key(uint32_t g, uint64_t ct, uint64_t t1, uint64_t t2, uint64_t cd, uint64_t d1, uint64_t d2, uint32_t d,
                                      uint32_t min_overlap) {
    const uint64_t b = ct & cd;
    const uint32_t ovl = (uint32_t)__popcll(b);
    if (g > 2u || ovl < min_overlap) return -1;    // min_overlap >= 1: ovl > 0 below
    const uint32_t dist = (uint32_t)__popcll(b & (t1 ^ d1)) + (uint32_t)__popcll(b & (t2 ^ d2));
    const uint32_t w = 32768u * (2u * ovl - dist) / ovl;           // <= 65 536, exact
    return (int)((w << 12) | (4095u - d));         // d <= 4 095; below 2^29
}

__device__ __forceinline__ int im_wave_max(int v) {
#pragma unroll
    for (uint32_t x = 32; x > 0; x >>= 1) {
        const int o = __shfl_xor(v, (int)x);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(IM_THREADS) void k_impute(const uint8_t *T, uint32_t Spad, uint32_t S, uint32_t M, const int32_t *nbr,
                                                       uint32_t L, uint32_t k, uint32_t min_overlap, uint32_t min_conf_ppm,
                                                       const uint32_t *called, uint8_t *out, uint32_t *stats) {
    extern __shared__ __attribute__((aligned(16))) uint64_t im_lds[];
    const uint32_t m = blockIdx.y * IM_GRID_X + blockIdx.x;
    if (m >= M) return;                            // (the last row of the grid; uniform over the workgroup)
    uint64_t *pc = im_lds, *p1 = pc + Spad, *p2 = p1 + Spad;
    uint8_t *own = reinterpret_cast<uint8_t *>(p2 + Spad);         // the marker's own codes 0 .. 3
    int32_t *nb = reinterpret_cast<int32_t *>(own + Spad);         // Spad is a multiple of 64: aligned
    uint32_t *cnt = reinterpret_cast<uint32_t *>(nb + TD_IMPUTE_MAX_NBR);          // imputed, no_donor, undecided
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t miss = S - called[m];
    if (tid < L) nb[tid] = nbr[(size_t)m * L + tid];
    if (tid < 4u) cnt[tid] = 0;
    __syncthreads();
    bool any = false;
    for (uint32_t q = 0; q < L; ++q) any |= nb[q] >= 0;
    if (miss == 0 || !any) {                       // uniform: nothing to impute, or nobody to ask
        if (tid == 0) {
            uint32_t *st = stats + (size_t)m * TD_IMPUTE_STATS;
            st[0] = miss;
            st[1] = 0;
            st[2] = miss;
            st[3] = 0;
        }
        return;
    }
    // A: the planes of every sample over the neighbours, and the marker's own row
    for (uint32_t s = tid; s < Spad; s += IM_THREADS) {
        uint64_t c = 0, a1 = 0, a2 = 0;
        for (uint32_t q = 0; q < L; ++q) {
            const int32_t j = nb[q];
            if (j < 0) continue;                   // (uniform)
            const uint32_t g = T[(size_t)(uint32_t)j * Spad + s];  // j < M (checked on the host), s < Spad
            c |= (uint64_t)(g <= 2u) << q;
            a1 |= (uint64_t)(g >= 1u) << q;
            a2 |= (uint64_t)(g >= 2u) << q;
        }
        pc[s] = c;
        p1[s] = a1;
        p2[s] = a2;
        own[s] = T[(size_t)m * Spad + s];
    }
    __syncthreads();
    // B: a wave per target
    uint32_t n_imp = 0, n_nod = 0, n_und = 0;      // uniform over the wave
    for (uint32_t t = wave; t < S; t += IM_WAVES) {
        if (own[t] <= 2u) continue;                // (uniform)
        const uint64_t ct = pc[t], t1 = p1[t], t2 = p2[t];
        // every lane's best key among its donors d = lane, lane + 64, ...
        int mine = -1;
        for (uint32_t d = lane; d < Spad; d += 64u) {
            const int key = im_key(own[d], ct, t1, t2, pc[d], p1[d], p2[d], d, min_overlap);
            mine = key > mine ? key : mine;
        }
        uint32_t v0 = 0, v1 = 0, v2 = 0, voters = 0;
        for (uint32_t r = 0; r < k; ++r) {
            const int best = im_wave_max(mine);
            if (best < 0) break;                   // fewer than k eligible donors (uniform)
            const uint32_t w = (uint32_t)best >> 12, win = 4095u - ((uint32_t)best & 4095u), cls = own[win];
            v0 += cls == 0u ? w : 0u;
            v1 += cls == 1u ? w : 0u;
            v2 += cls == 2u ? w : 0u;
            ++voters;
            if (r + 1 == k) break;
            // only the winner's lane needs a new best: its donors are (win & 63) + 64 j, at most 64 of them, and lane j
            // looks at one.  Whoever of them has voted holds a key above `best`, whoever has not a key below it.
            const uint32_t d = (win & 63u) + 64u * lane;
            int next = -1;
            if (d < Spad) {
                const int key = im_key(own[d], ct, t1, t2, pc[d], p1[d], p2[d], d, min_overlap);
                next = key < best ? key : -1;
            }
            next = im_wave_max(next);
            if (lane == (win & 63u)) mine = next;
        }
        if (voters == 0) {
            ++n_nod;
            continue;
        }
        const uint32_t total = v0 + v1 + v2;       // <= 32 * 65 536
        const uint32_t top = v0 > v1 ? (v0 > v2 ? v0 : v2) : (v1 > v2 ? v1 : v2);
        const uint32_t at = (uint32_t)(v0 == top) + (uint32_t)(v1 == top) + (uint32_t)(v2 == top);
        const bool sure = total > 0 && at == 1u && (uint64_t)top * 1000000ull >= (uint64_t)min_conf_ppm * total;
        if (!sure) {
            ++n_und;
            continue;
        }
        ++n_imp;
        if (lane == 0) out[(size_t)t * M + m] = (uint8_t)(v0 == top ? 0u : v1 == top ? 1u : 2u);   // t < S, m < M
    }
    if (lane == 0) {
        if (n_imp) atomicAdd(cnt + 0, n_imp);
        if (n_nod) atomicAdd(cnt + 1, n_nod);
        if (n_und) atomicAdd(cnt + 2, n_und);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t *st = stats + (size_t)m * TD_IMPUTE_STATS;
        st[0] = miss;
        st[1] = cnt[0];
        st[2] = cnt[1];
        st[3] = cnt[2];
    }
}

}  // namespace

extern "C" int td_impute_last_times(td_handle *h, double *out2) {
    if (!h || !out2) return td_fail_internal(TD_E_ARG, "NULL argument");
    out2[0] = g_im_times[0];
    out2[1] = g_im_times[1];
    return TD_OK;
}

extern "C" int td_impute_knn(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const int32_t *nbr, const td_impute_params *p,
                             uint8_t *calls_out, void **d_calls_out, uint32_t *stats_out, double *ms) {
    if (d_calls_out) *d_calls_out = nullptr;
    if (ms) *ms = 0;
    g_im_times[0] = g_im_times[1] = 0;
    if (!h || !p) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (S > TD_IMPUTE_MAX_SAMPLES) return td_fail_internal(TD_E_ARG, "more samples than TD_IMPUTE_MAX_SAMPLES");
    if (p->L < 1 || p->L > TD_IMPUTE_MAX_NBR) return td_fail_internal(TD_E_ARG, "L must be 1..64");
    if (p->k < 1 || p->k > TD_IMPUTE_MAX_K) return td_fail_internal(TD_E_ARG, "k must be 1..32");
    if (p->min_overlap < 1) return td_fail_internal(TD_E_ARG, "min_overlap must be at least 1");
    if (p->min_conf_ppm > 1000000u) return td_fail_internal(TD_E_ARG, "min_conf_ppm must be at most 1000000");
    if (M >= 0x80000000u) return td_fail_internal(TD_E_ARG, "markers must number below 2^31");
    if (S && M && !d_calls) return td_fail_internal(TD_E_ARG, "NULL call matrix");
    if (S && M && !nbr) return td_fail_internal(TD_E_ARG, "NULL neighbour table");
    const uint32_t L = p->L;
    if (nbr && M) {                                // a row names markers below M, not its own, none twice
        std::vector<uint32_t> seen(M, 0);          // seen[j] = m + 1: row m has named j
        for (uint32_t m = 0; m < M; ++m) {
            for (uint32_t q = 0; q < L; ++q) {
                const int32_t j = nbr[(size_t)m * L + q];
                if (j == -1) continue;
                const char *what = j < 0 || (uint32_t)j >= M ? " is outside -1 .. M - 1" : (uint32_t)j == m ? " is the marker itself" :
                                   seen[j] == m + 1 ? " appears twice" : nullptr;
                if (what) {
                    td_set_bad_index(m);
                    return td_fail_internal(TD_E_ARG, ("neighbours of marker " + std::to_string(m) + ": entry " + std::to_string(j) + what).c_str());
                }
                seen[j] = m + 1;
            }
        }
    }
    if (stats_out && M) memset(stats_out, 0, (size_t)M * TD_IMPUTE_STATS * sizeof(uint32_t));
    if (S == 0 || M == 0) return TD_OK;            // nothing missing, nothing to copy, no launch
    int rc = td_handle_wait_work(h);
    if (rc) return rc;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    const uint32_t ntiles = (M + CT_TILE - 1) / CT_TILE;
    const uint32_t Spad = (S + CT_STEP - 1) / CT_STEP * CT_STEP;
    const size_t Mpad = (size_t)ntiles * CT_TILE, cells = (size_t)S * M;
    const uint32_t lds = 25u * Spad + IM_TAIL;
    TD_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_impute), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    tdi::Events<3> ev;
    TD_HIPCHK(ev.create());
    tdi::DevBuf<uint8_t> d_T, d_out;
    tdi::DevBuf<uint32_t> d_called, d_stats;
    tdi::DevBuf<int32_t> d_nbr;
    TD_HIPCHK(d_T.alloc(Mpad * Spad));
    TD_HIPCHK(d_out.alloc(cells < 16 ? 16 : cells));   // (what td_dev_alloc would give)
    TD_HIPCHK(d_called.alloc(Mpad));
    TD_HIPCHK(d_stats.alloc((size_t)M * TD_IMPUTE_STATS));
    TD_HIPCHK(d_nbr.alloc((size_t)M * L));
    TD_HIPCHK(hipMemcpy(d_nbr.p, nbr, (size_t)M * L * sizeof(int32_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(d_out.p, d_calls, cells, hipMemcpyDeviceToDevice));
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    hipLaunchKernelGGL(k_calls_transpose<false>, dim3(ntiles), dim3(CT_THREADS), 0, 0, (const uint8_t *)d_calls, S, M, nullptr, M, Spad, d_T.p,
                       d_called.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    hipLaunchKernelGGL(k_impute, dim3(M < IM_GRID_X ? M : IM_GRID_X, (M + IM_GRID_X - 1) / IM_GRID_X), dim3(IM_THREADS), lds, 0,
                       d_T.p, Spad, S, M, d_nbr.p, L, p->k, p->min_overlap, p->min_conf_ppm, d_called.p, d_out.p, d_stats.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[2], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[2]));
    float f0 = 0, f1 = 0;
    TD_HIPCHK(hipEventElapsedTime(&f0, ev.e[0], ev.e[1]));
    TD_HIPCHK(hipEventElapsedTime(&f1, ev.e[1], ev.e[2]));
    g_im_times[0] = f0;
    g_im_times[1] = f1;
    if (ms) *ms = (double)f0 + (double)f1;
    if (stats_out) TD_HIPCHK(hipMemcpy(stats_out, d_stats.p, (size_t)M * TD_IMPUTE_STATS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (calls_out) TD_HIPCHK(hipMemcpy(calls_out, d_out.p, cells, hipMemcpyDeviceToHost));
    if (d_calls_out) *d_calls_out = d_out.release();
    return TD_OK;
}
