// Genotype calls and marker filters from the count matrix (include/tagdig.h: td_geno_call).
//
// Input: the S x T uint32 count matrix where it lies in device memory, and M markers as pairs of columns (i0[m], i1[m]).
// The rule, in integers only, for sample s and marker m with a = counts[s][i0], b = counts[s][i1], n = a + b (64-bit):
//   missing (3)  n < min_depth
//   presence     1 when a > 0 and b > 0, else 0 when a > 0, else 2
//   likelihood   n > 127: a' = 127 a / n, b' = 127 b / n (64-bit products, floor), n' = a' + b'; else the values
//                themselves.  Heterozygous (1) when min(a', b') >= het_min[n']; else 0 when a' >= b', else 2.
// het_min[0 .. 127] comes from the caller as data (Python's fractions.Fraction builds it): no power or logarithm is
// evaluated here.  Per marker: n0, n1, n2 (calls by code), called = n0 + n1 + n2, alt = n1 + 2 n2, depth0 / depth1 =
// the sums of a and of b over every sample.  A marker passes when
//   called * 10^6 >= min_call_ppm * S,  min(alt, 2 called - alt) * 10^6 >= min_maf_ppm * 2 called,
//   n1 * 10^6 <= max_het_ppm * called.
//
// K1 k_gc_call: grid (ceil(M / GC_TILE), ceil(S / TD_GENO_CHUNK)), GC_TILE threads.  A thread owns one marker and walks
//    the sample rows of its chunk, GC_ROWS at a time: lanes run along markers, so the 64 call bytes a wave writes per
//    row are contiguous, and its loads of a row fall into whole cache lines when the markers' columns are adjacent (a
//    marker at columns 2 k, 2 k + 1 comes in one 8-byte load).  The table sits in LDS.  The partial n0, n1, n2 (uint32)
//    and depth sums (uint64) of a chunk are added with integer atomics, lane m next to lane m + 1: the result does not
//    depend on the order of the chunks.
// K2 k_gc_filter: one thread per marker writes the statistics row and the pass byte; the passing markers are counted
//    with one atomic per wave (ballot).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "td_internal.hpp"

namespace {

constexpr int GC_TILE = 256;                       // markers of a workgroup = its threads
constexpr uint32_t GC_CHUNK = TD_GENO_CHUNK;       // sample rows of a workgroup
constexpr uint32_t GC_TABLE = TD_GENO_TABLE;       // entries of het_min
constexpr uint64_t GC_SCALE = GC_TABLE - 1;        // depths above this are scaled down to it
constexpr uint32_t GC_ROWS = 4;                    // sample rows whose loads a thread has in flight at once
static_assert(GC_CHUNK % GC_ROWS == 0, "a chunk is walked GC_ROWS rows at a time");

// the code of one cell; s_het: the table in LDS
__device__ __forceinline__ uint32_t gc_code(uint32_t a, uint32_t b, uint32_t rule, uint64_t min_depth, const uint16_t *s_het) {
    const uint64_t n = (uint64_t)a + b;
    if (n < min_depth) return 3u;
    if (rule == TD_GENO_PRESENCE) return a && b ? 1u : a ? 0u : 2u;
    uint32_t x = a, y = b;
    if (n > GC_SCALE) {
        x = (uint32_t)(GC_SCALE * a / n);
        y = (uint32_t)(GC_SCALE * b / n);
    }
    const uint32_t k = x < y ? x : y;
    if (k >= s_het[x + y]) return 1u;              // x + y <= 127: floor(127 a / n) + floor(127 b / n) <= 127
    return x >= y ? 0u : 2u;
}

// ------------------------------------------------------------------ K1
__global__ __launch_bounds__(GC_TILE) void k_gc_call(const uint32_t *counts, uint32_t S, uint32_t T, uint32_t M,
                                                     const uint32_t *i0, const uint32_t *i1, const uint16_t *het_min,
                                                     uint32_t rule, uint64_t min_depth, uint8_t *calls, uint32_t *ncode,
                                                     unsigned long long *depth) {
    __shared__ uint16_t s_het[GC_TABLE];
    if (threadIdx.x < GC_TABLE) s_het[threadIdx.x] = het_min[threadIdx.x];
    __syncthreads();
    const uint32_t m = blockIdx.x * GC_TILE + threadIdx.x;
    if (m >= M) return;
    const uint32_t s_lo = blockIdx.y * GC_CHUNK;
    const uint32_t s_hi = S - s_lo < GC_CHUNK ? S : s_lo + GC_CHUNK;
    const uint32_t c0 = i0[m], c1 = i1[m];         // both < T: the host checked them
    // two adjacent columns that start an aligned 8 bytes in every row (census_markers' layout) come in one load
    const bool pair = c1 == c0 + 1 && !(c0 & 1u) && !(T & 1u) && !((uintptr_t)counts & 7u);
    const uint32_t *row = counts + (size_t)s_lo * T;
    uint8_t *out = calls + (size_t)s_lo * M + m;
    uint32_t n0 = 0, n1 = 0, n2 = 0;
    uint64_t d0 = 0, d1 = 0;
    for (uint32_t s = s_lo; s < s_hi; s += GC_ROWS, row += (size_t)GC_ROWS * T, out += (size_t)GC_ROWS * M) {
        // the loads of GC_ROWS rows are issued before the first of them is used (s + u < s_hi is the same in every lane)
        uint32_t a[GC_ROWS], b[GC_ROWS];
#pragma unroll
        for (uint32_t u = 0; u < GC_ROWS; ++u) {
            a[u] = b[u] = 0;
            if (s + u < s_hi) {
                const uint32_t *r = row + (size_t)u * T;
                if (pair) {
                    const uint2 v = *reinterpret_cast<const uint2 *>(r + c0);
                    a[u] = v.x;
                    b[u] = v.y;
                } else {
                    a[u] = r[c0];
                    b[u] = r[c1];
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < GC_ROWS; ++u) {
            if (s + u < s_hi) {
                const uint32_t code = gc_code(a[u], b[u], rule, min_depth, s_het);
                out[(size_t)u * M] = (uint8_t)code;
                n0 += code == 0u;
                n1 += code == 1u;
                n2 += code == 2u;
                d0 += a[u];
                d1 += b[u];
            }
        }
    }
    if (n0) atomicAdd(&ncode[m], n0);
    if (n1) atomicAdd(&ncode[(size_t)M + m], n1);
    if (n2) atomicAdd(&ncode[2 * (size_t)M + m], n2);
    if (d0) atomicAdd(&depth[m], (unsigned long long)d0);
    if (d1) atomicAdd(&depth[(size_t)M + m], (unsigned long long)d1);
}

// ------------------------------------------------------------------ K2
__global__ __launch_bounds__(256) void k_gc_filter(const uint32_t *ncode, const unsigned long long *depth, uint32_t S, uint32_t M,
                                                   uint32_t min_call_ppm, uint32_t min_maf_ppm, uint32_t max_het_ppm,
                                                   uint64_t *stats, uint8_t *pass, unsigned long long *passed) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (m < M) {
        const uint64_t n0 = ncode[m], n1 = ncode[(size_t)M + m], n2 = ncode[2 * (size_t)M + m];
        const uint64_t called = n0 + n1 + n2, alt = n1 + 2 * n2;
        uint64_t *st = stats + (size_t)m * TD_GENO_NSTATS;
        st[TD_GENO_CALLED] = called;
        st[TD_GENO_N0] = n0;
        st[TD_GENO_N1] = n1;
        st[TD_GENO_N2] = n2;
        st[TD_GENO_ALT] = alt;
        st[TD_GENO_DEPTH0] = depth[m];
        st[TD_GENO_DEPTH1] = depth[(size_t)M + m];
        // every product stays below 2^54: called <= S < 2^32, alt <= 2^33, the ppm values <= 10^6 < 2^20
        const uint64_t minor = alt < 2 * called - alt ? alt : 2 * called - alt;
        ok = called * 1000000ull >= (uint64_t)min_call_ppm * S &&
             minor * 1000000ull >= (uint64_t)min_maf_ppm * 2 * called &&
             n1 * 1000000ull <= (uint64_t)max_het_ppm * called;
        pass[m] = ok ? 1 : 0;
    }
    const uint64_t votes = __ballot(ok);
    if (votes && (threadIdx.x & 63) == __ffsll((unsigned long long)votes) - 1)
        atomicAdd(passed, (unsigned long long)__popcll(votes));
}

}  // namespace

extern "C" int td_geno_call(td_handle *h, const void *d_counts, uint32_t S, uint32_t T, uint32_t M, const uint32_t *i0,
                            const uint32_t *i1, const uint16_t *het_min, const td_geno_params *p, uint8_t *calls_out,
                            void **d_calls_out, uint64_t *stats_out, uint8_t *pass_out, uint64_t *passed_out, double *ms) {
    if (d_calls_out) *d_calls_out = nullptr;
    if (passed_out) *passed_out = 0;
    if (ms) *ms = 0;
    if (!h || !p || !het_min || !passed_out) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (p->rule != TD_GENO_LIKELIHOOD && p->rule != TD_GENO_PRESENCE) return td_fail_internal(TD_E_ARG, "rule must be 0 (likelihood) or 1 (presence)");
    if (p->err_ppm < 1 || p->err_ppm > 499999u) return td_fail_internal(TD_E_ARG, "err_ppm must be 1..499999");
    if (p->min_depth < 1) return td_fail_internal(TD_E_ARG, "min_depth must be at least 1");
    if (p->min_call_ppm > 1000000u) return td_fail_internal(TD_E_ARG, "min_call_ppm must be 0..1000000");
    if (p->min_maf_ppm > 500000u) return td_fail_internal(TD_E_ARG, "min_maf_ppm must be 0..500000");
    if (p->max_het_ppm > 1000000u) return td_fail_internal(TD_E_ARG, "max_het_ppm must be 0..1000000");
    for (uint32_t n = 0; n < GC_TABLE; ++n)
        if (het_min[n] > n + 1) return td_fail_internal(TD_E_ARG, ("het_min[" + std::to_string(n) + "] exceeds n + 1").c_str());
    if (M && (!i0 || !i1 || !stats_out || !pass_out)) return td_fail_internal(TD_E_ARG, "NULL argument");
    for (uint32_t m = 0; m < M; ++m) {
        if (i0[m] >= T || i1[m] >= T || i0[m] == i1[m]) {
            td_set_bad_index(m);
            return td_fail_internal(TD_E_ARG, ("marker " + std::to_string(m) + ": columns " + std::to_string(i0[m]) + " and " +
                                               std::to_string(i1[m]) + (i0[m] == i1[m] && i0[m] < T ? " are the same" :
                                               " are not both below T = " + std::to_string(T))).c_str());
        }
    }
    if (M == 0 || T == 0) return TD_OK;            // (T = 0 with M > 0 has failed the index check above)
    if (S == 0) {                                  // no sample: zero statistics, and no marker passes on no evidence
        for (uint64_t k = 0; k < (uint64_t)M * TD_GENO_NSTATS; ++k) stats_out[k] = 0;
        for (uint32_t m = 0; m < M; ++m) pass_out[m] = 0;
        return TD_OK;
    }
    if (!d_counts) return td_fail_internal(TD_E_ARG, "NULL count matrix");
    if (((uintptr_t)d_counts & 3u) != 0) return td_fail_internal(TD_E_ARG, "the count matrix must be 4-byte aligned");
    const uint64_t chunks = ((uint64_t)S + GC_CHUNK - 1) / GC_CHUNK;
    if (chunks > 65535u) return td_fail_internal(TD_E_LIMIT, "more samples than one launch takes (65 535 chunks)");
    int rc = td_handle_wait_work(h);
    if (rc) return rc;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    tdi::Events<2> ev;
    TD_HIPCHK(ev.create());
    tdi::DevBuf<uint32_t> di, ncode;
    tdi::DevBuf<uint16_t> dhet;
    tdi::DevBuf<uint8_t> calls, pass;
    tdi::DevBuf<uint64_t> stats;
    tdi::DevBuf<unsigned long long> acc;                 // depth0[M] | depth1[M] | passed
    TD_HIPCHK(di.alloc(2ull * M));
    TD_HIPCHK(dhet.alloc(GC_TABLE));
    TD_HIPCHK(ncode.alloc(3ull * M));
    TD_HIPCHK(acc.alloc(2ull * M + 1));
    TD_HIPCHK(calls.alloc((uint64_t)S * M));
    TD_HIPCHK(pass.alloc(M));
    TD_HIPCHK(stats.alloc((uint64_t)M * TD_GENO_NSTATS));
    TD_HIPCHK(hipMemcpy(di.p, i0, (uint64_t)M * 4, hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(di.p + M, i1, (uint64_t)M * 4, hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(dhet.p, het_min, GC_TABLE * sizeof(uint16_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemset(ncode.p, 0, 3ull * M * 4));
    TD_HIPCHK(hipMemset(acc.p, 0, (2ull * M + 1) * 8));
    const uint32_t gx = (M + GC_TILE - 1) / GC_TILE;
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    hipLaunchKernelGGL(k_gc_call, dim3(gx, (uint32_t)chunks), dim3(GC_TILE), 0, 0, (const uint32_t *)d_counts, S, T, M, di.p,
                       di.p + M, dhet.p, p->rule, p->min_depth, calls.p, ncode.p, acc.p);
    TD_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_gc_filter, dim3((M + 255) / 256), dim3(256), 0, 0, ncode.p, acc.p, S, M, p->min_call_ppm, p->min_maf_ppm,
                       p->max_het_ppm, stats.p, pass.p, acc.p + 2ull * M);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[1]));
    if (ms) {
        float f = 0;
        TD_HIPCHK(hipEventElapsedTime(&f, ev.e[0], ev.e[1]));
        *ms = f;
    }
    unsigned long long passed = 0;
    TD_HIPCHK(hipMemcpy(&passed, acc.p + 2ull * M, sizeof passed, hipMemcpyDeviceToHost));
    TD_HIPCHK(hipMemcpy(stats_out, stats.p, (uint64_t)M * TD_GENO_NSTATS * 8, hipMemcpyDeviceToHost));
    TD_HIPCHK(hipMemcpy(pass_out, pass.p, M, hipMemcpyDeviceToHost));
    if (calls_out) TD_HIPCHK(hipMemcpy(calls_out, calls.p, (uint64_t)S * M, hipMemcpyDeviceToHost));
    *passed_out = passed;
    if (d_calls_out) *d_calls_out = calls.release();
    return TD_OK;
}
