// Polyploid allele dosage calls from the count matrix (include/tagdig.h: td_dose_call).
//
// Input: the S x T uint32 count matrix where it lies in device memory, M markers as pairs of columns (i0[m], i1[m]), one
// ploidy P = 2 .. 8 for every sample, and three tables of integer costs (round(-65536 log2 x) of a probability x) that the
// caller built: ca[d] for a read of allele 1 and cb[d] for a read of allele 0 from a cell of dosage d, cp[bin][d] for
// dosage d under the prior of the marker's bin.  The rule, in integers only, for sample s and marker m with
// a = counts[s][i0], b = counts[s][i1], n = a + b (64-bit):
//   per marker  depth0 / depth1 = the sums of a and of b over every sample, tot = depth0 + depth1,
//               bin = 0 when tot == 0, else min(63, floor(64 depth1 / tot))
//   missing     (255) n < min_depth
//   cost        c[d] = b ca[d] + a cb[d] + cp[bin][d] (uint64, below 2^57: the tables stay below 2^23 + 1), d = 0 .. P;
//               with the flat prior the last term is 0
//   call        best = the smallest d with minimal c[d], second = the minimum over d != best; best when
//               second - c[best] >= min_margin, else missing
//   diploidised 0 for dosage 0, 2 for dosage P, 1 between, 3 for missing
// Per marker: n[0 .. 8] (calls by dosage), called = their sum, alt = sum of d n[d].  A marker passes when
//   called * 10^6 >= min_call_ppm * S,  min(alt, P called - alt) * 10^6 >= min_maf_ppm * P * called.
//
// K0 k_dose_depth (HWE prior only): k_gc_call's geometry, grid (ceil(M / DS_TILE), ceil(S / TD_DOSE_CHUNK)), DS_TILE
//    threads; a thread owns one marker over a chunk of sample rows and adds its two partial sums with 64-bit atomics.  The
//    bin is a function of the two complete sums, so it exists only after this kernel: K1 derives it, once per thread.
// K1 k_dose_call<P, HWE>: the same geometry, DS_ROWS rows' loads in flight, an adjacent column pair in one 8-byte load.
//    ca / cb arrive as a kernel argument (uniform: scalar registers), the marker's prior row is loaded into registers once
//    per thread.  The loop over d is unrolled by the template: every cost is two 32 x 32 + 64-bit multiply-adds.  The
//    class counts of a chunk are added with integer atomics, lane m next to lane m + 1, so the result does not depend on
//    the order of the chunks.  With the flat prior the depth sums are gathered here and the matrix is read once.
// K2 k_dose_filter: one thread per marker writes the statistics row and the pass byte; the passing markers are counted
//    with one atomic per wave (ballot).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "td_internal.hpp"

namespace {

constexpr int DS_TILE = 256;                       // markers of a workgroup = its threads
constexpr uint32_t DS_CHUNK = TD_DOSE_CHUNK;       // sample rows of a workgroup
constexpr uint32_t DS_ROWS = 4;                    // sample rows whose loads a thread has in flight at once
constexpr uint32_t DS_NB = TD_DOSE_BINS;
constexpr uint32_t DS_NCLASS = TD_DOSE_MAX_PLOIDY + 1;
static_assert(DS_CHUNK % DS_ROWS == 0, "a chunk is walked DS_ROWS rows at a time");
static_assert(TD_DOSE_NSTATS == TD_DOSE_N0 + DS_NCLASS + 4, "called, n[0 .. 8], alt, depth0, depth1, bin");

struct DoseTables {                                // by value in the kernel arguments
    uint32_t ca[DS_NCLASS], cb[DS_NCLASS];
};

__device__ __forceinline__ uint32_t dose_bin(uint64_t d0, uint64_t d1) {
    const uint64_t tot = d0 + d1;                  // <= 2^24 * 2^33: 64 d1 stays below 2^63
    if (tot == 0) return 0;
    const uint64_t k = DS_NB * d1 / tot;
    return k < DS_NB - 1 ? (uint32_t)k : DS_NB - 1;
}

// the DS_ROWS rows from `row` on, of which `left` exist: the loads are issued before the first of them is used
__device__ __forceinline__ void dose_load(const uint32_t *row, uint32_t T, uint32_t c0, uint32_t c1, bool pair, uint32_t left,
                                          uint32_t (&a)[DS_ROWS], uint32_t (&b)[DS_ROWS]) {
#pragma unroll
    for (uint32_t u = 0; u < DS_ROWS; ++u) {
        a[u] = b[u] = 0;
        if (u < left) {
            const uint32_t *r = row + (size_t)u * T;
            if (pair) {
                const uint64_t v = *reinterpret_cast<const uint64_t *>(r + c0);   // (one 64-bit value: two 32-bit loads cannot be made of it)
                a[u] = (uint32_t)v;
                b[u] = (uint32_t)(v >> 32);
            } else {
                a[u] = r[c0];
                b[u] = r[c1];
            }
        }
    }
}

// two adjacent columns that start an aligned 8 bytes in every row (census_markers' layout) come in one load -- when that
// holds for every marker of the wave: the answer is uniform, so the row loop keeps one kind of load
__device__ __forceinline__ bool dose_pair(const uint32_t *counts, uint32_t T, uint32_t c0, uint32_t c1) {
    return __all(c1 == c0 + 1 && !(c0 & 1u) && !(T & 1u) && !((uintptr_t)counts & 7u));
}

// ------------------------------------------------------------------ K0
__global__ __launch_bounds__(DS_TILE) void k_dose_depth(const uint32_t *counts, uint32_t S, uint32_t T, uint32_t M,
                                                        const uint32_t *i0, const uint32_t *i1, unsigned long long *depth) {
    const uint32_t m = blockIdx.x * DS_TILE + threadIdx.x;
    if (m >= M) return;
    const uint32_t s_lo = blockIdx.y * DS_CHUNK;
    const uint32_t s_hi = S - s_lo < DS_CHUNK ? S : s_lo + DS_CHUNK;
    const uint32_t c0 = i0[m], c1 = i1[m];         // both < T: the host checked them
    const bool pair = dose_pair(counts, T, c0, c1);
    const uint32_t *row = counts + (size_t)s_lo * T;
    uint64_t d0 = 0, d1 = 0;
    for (uint32_t s = s_lo; s < s_hi; s += DS_ROWS, row += (size_t)DS_ROWS * T) {
        uint32_t a[DS_ROWS], b[DS_ROWS];
        dose_load(row, T, c0, c1, pair, s_hi - s, a, b);
#pragma unroll
        for (uint32_t u = 0; u < DS_ROWS; ++u) {   // (rows that do not exist were loaded as 0)
            d0 += a[u];
            d1 += b[u];
        }
    }
    if (d0) atomicAdd(&depth[m], (unsigned long long)d0);
    if (d1) atomicAdd(&depth[(size_t)M + m], (unsigned long long)d1);
}

// ------------------------------------------------------------------ K1
// depth: HWE: the complete sums K0 left (read); flat: the sums are gathered here (added).  diploid may be NULL.
template <int P, bool HWE>
__global__ __launch_bounds__(DS_TILE) void k_dose_call(const uint32_t *counts, uint32_t S, uint32_t T, uint32_t M,
                                                       const uint32_t *i0, const uint32_t *i1, const DoseTables tab,
                                                       const uint32_t *cp, uint64_t min_depth, uint32_t min_margin,
                                                       uint8_t *calls, uint8_t *diploid, uint32_t *ncode,
                                                       unsigned long long *depth) {
    const uint32_t m = blockIdx.x * DS_TILE + threadIdx.x;
    if (m >= M) return;
    const uint32_t s_lo = blockIdx.y * DS_CHUNK;
    const uint32_t s_hi = S - s_lo < DS_CHUNK ? S : s_lo + DS_CHUNK;
    const uint32_t c0 = i0[m], c1 = i1[m];         // both < T: the host checked them
    const bool pair = dose_pair(counts, T, c0, c1);
    uint32_t prior[P + 1];
#pragma unroll
    for (int d = 0; d <= P; ++d) prior[d] = 0;
    if (HWE) {
        const uint32_t *rowp = cp + (size_t)dose_bin(depth[m], depth[(size_t)M + m]) * (P + 1);
#pragma unroll
        for (int d = 0; d <= P; ++d) prior[d] = rowp[d];
    }
    const uint32_t *row = counts + (size_t)s_lo * T;
    const size_t cell = (size_t)s_lo * M + m;
    uint8_t *out = calls + cell;
    uint8_t *dip = diploid ? diploid + cell : nullptr;
    uint32_t nd[P + 1];
#pragma unroll
    for (int d = 0; d <= P; ++d) nd[d] = 0;
    uint64_t d0 = 0, d1 = 0;
    for (uint32_t s = s_lo; s < s_hi; s += DS_ROWS, row += (size_t)DS_ROWS * T) {
        uint32_t a[DS_ROWS], b[DS_ROWS];
        dose_load(row, T, c0, c1, pair, s_hi - s, a, b);
#pragma unroll
        for (uint32_t u = 0; u < DS_ROWS; ++u) {
            if (s + u < s_hi) {                    // (the same in every lane)
                // the first class opens, every later one either takes the lead or contends for second place
                uint64_t best = (uint64_t)b[u] * tab.ca[0] + (uint64_t)a[u] * tab.cb[0] + prior[0];
                uint64_t second = ~0ull;
                uint32_t code = 0;
#pragma unroll
                for (int d = 1; d <= P; ++d) {
                    const uint64_t c = (uint64_t)b[u] * tab.ca[d] + (uint64_t)a[u] * tab.cb[d] + prior[d];
                    const bool lead = c < best;    // strict: among equal costs the smallest d stays best
                    const uint64_t loser = lead ? best : c;
                    second = loser < second ? loser : second;
                    best = lead ? c : best;
                    code = lead ? (uint32_t)d : code;
                }
                if ((uint64_t)a[u] + b[u] < min_depth || second - best < min_margin) code = TD_DOSE_MISSING;
                const size_t off = (size_t)(s - s_lo + u) * M;
                out[off] = (uint8_t)code;
                if (dip) dip[off] = (uint8_t)(code == TD_DOSE_MISSING ? TD_GENO_MISSING : code == 0u ? 0u : code == (uint32_t)P ? 2u : 1u);
#pragma unroll
                for (int d = 0; d <= P; ++d) nd[d] += code == (uint32_t)d;
                if (!HWE) {
                    d0 += a[u];
                    d1 += b[u];
                }
            }
        }
    }
#pragma unroll
    for (int d = 0; d <= P; ++d)
        if (nd[d]) atomicAdd(&ncode[(size_t)d * M + m], nd[d]);
    if (!HWE) {
        if (d0) atomicAdd(&depth[m], (unsigned long long)d0);
        if (d1) atomicAdd(&depth[(size_t)M + m], (unsigned long long)d1);
    }
}

// ------------------------------------------------------------------ K2
__global__ __launch_bounds__(256) void k_dose_filter(const uint32_t *ncode, const unsigned long long *depth, uint32_t S, uint32_t M,
                                                     uint32_t P, uint32_t min_call_ppm, uint32_t min_maf_ppm, uint64_t *stats,
                                                     uint8_t *pass, unsigned long long *passed) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (m < M) {
        uint64_t *st = stats + (size_t)m * TD_DOSE_NSTATS;
        uint64_t called = 0, alt = 0;
#pragma unroll
        for (uint32_t d = 0; d < DS_NCLASS; ++d) { // (the classes above P were never added to: 0)
            const uint64_t n = ncode[(size_t)d * M + m];
            st[TD_DOSE_N0 + d] = n;
            called += n;
            alt += d * n;
        }
        const uint64_t d0 = depth[m], d1 = depth[(size_t)M + m];
        st[TD_DOSE_CALLED] = called;
        st[TD_DOSE_ALT] = alt;
        st[TD_DOSE_DEPTH0] = d0;
        st[TD_DOSE_DEPTH1] = d1;
        st[TD_DOSE_BIN] = dose_bin(d0, d1);
        // every product stays below 2^48: called <= S <= 2^24, alt <= 2^27, the ppm values <= 10^6 < 2^20
        const uint64_t minor = alt < P * called - alt ? alt : P * called - alt;
        ok = called * 1000000ull >= (uint64_t)min_call_ppm * S && minor * 1000000ull >= (uint64_t)min_maf_ppm * P * called;
        pass[m] = ok ? 1 : 0;
    }
    const uint64_t votes = __ballot(ok);
    if (votes && (threadIdx.x & 63) == __ffsll((unsigned long long)votes) - 1)
        atomicAdd(passed, (unsigned long long)__popcll(votes));
}

struct DoseLaunch {
    const uint32_t *counts; uint32_t S, T, M; const uint32_t *i0, *i1; DoseTables tab; const uint32_t *cp;
    uint64_t min_depth; uint32_t min_margin; uint8_t *calls, *diploid; uint32_t *ncode; unsigned long long *depth;
    dim3 grid;
};

template <int P> void dose_launch(const DoseLaunch &a, bool hwe) {
    if (hwe)
        hipLaunchKernelGGL((k_dose_call<P, true>), a.grid, dim3(DS_TILE), 0, 0, a.counts, a.S, a.T, a.M, a.i0, a.i1, a.tab, a.cp,
                           a.min_depth, a.min_margin, a.calls, a.diploid, a.ncode, a.depth);
    else
        hipLaunchKernelGGL((k_dose_call<P, false>), a.grid, dim3(DS_TILE), 0, 0, a.counts, a.S, a.T, a.M, a.i0, a.i1, a.tab, a.cp,
                           a.min_depth, a.min_margin, a.calls, a.diploid, a.ncode, a.depth);
}

}  // namespace

extern "C" int td_dose_call(td_handle *h, const void *d_counts, uint32_t S, uint32_t T, uint32_t M, const uint32_t *i0,
                            const uint32_t *i1, const uint32_t *ca, const uint32_t *cb, const uint32_t *cp, const td_dose_params *p,
                            uint8_t *calls_out, void **d_calls_out, uint8_t *diploid_out, void **d_diploid_out, uint64_t *stats_out,
                            uint8_t *pass_out, uint64_t *passed_out, double *ms) {
    if (d_calls_out) *d_calls_out = nullptr;
    if (d_diploid_out) *d_diploid_out = nullptr;
    if (passed_out) *passed_out = 0;
    if (ms) *ms = 0;
    if (!h || !p || !ca || !cb || !passed_out) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (p->ploidy < 2 || p->ploidy > TD_DOSE_MAX_PLOIDY) return td_fail_internal(TD_E_ARG, "ploidy must be 2..8");
    if (p->prior != TD_DOSE_FLAT && p->prior != TD_DOSE_HWE) return td_fail_internal(TD_E_ARG, "prior must be 0 (flat) or 1 (HWE)");
    if (p->err_ppm < 1 || p->err_ppm > 499999u) return td_fail_internal(TD_E_ARG, "err_ppm must be 1..499999");
    if (p->min_depth < 1) return td_fail_internal(TD_E_ARG, "min_depth must be at least 1");
    if (p->min_call_ppm > 1000000u) return td_fail_internal(TD_E_ARG, "min_call_ppm must be 0..1000000");
    if (p->min_maf_ppm > 500000u) return td_fail_internal(TD_E_ARG, "min_maf_ppm must be 0..500000");
    if (S > (1u << 24)) return td_fail_internal(TD_E_ARG, "more than 2^24 samples");
    const uint32_t P = p->ploidy;
    const bool hwe = p->prior == TD_DOSE_HWE;
    if (hwe && !cp) return td_fail_internal(TD_E_ARG, "the HWE prior needs the table cp");
    DoseTables tab = {};
    for (uint32_t d = 0; d <= P; ++d) {
        if (ca[d] > (uint32_t)TD_DOSE_COST_MAX || cb[d] > (uint32_t)TD_DOSE_COST_MAX)
            return td_fail_internal(TD_E_ARG, ("ca[" + std::to_string(d) + "] or cb[" + std::to_string(d) + "] exceeds 2^23").c_str());
        tab.ca[d] = ca[d];
        tab.cb[d] = cb[d];
    }
    const uint32_t ncp = DS_NB * (P + 1);
    if (hwe)
        for (uint32_t k = 0; k < ncp; ++k)
            if (cp[k] > (uint32_t)TD_DOSE_COST_MAX)
                return td_fail_internal(TD_E_ARG, ("cp[" + std::to_string(k / (P + 1)) + "][" + std::to_string(k % (P + 1)) + "] exceeds 2^23").c_str());
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
    if (S == 0) {                                  // no sample: zero statistics (bin 0 included), and no marker passes
        for (uint64_t k = 0; k < (uint64_t)M * TD_DOSE_NSTATS; ++k) stats_out[k] = 0;
        for (uint32_t m = 0; m < M; ++m) pass_out[m] = 0;
        return TD_OK;
    }
    if (!d_counts) return td_fail_internal(TD_E_ARG, "NULL count matrix");
    if (((uintptr_t)d_counts & 3u) != 0) return td_fail_internal(TD_E_ARG, "the count matrix must be 4-byte aligned");
    const uint64_t chunks = ((uint64_t)S + DS_CHUNK - 1) / DS_CHUNK;
    if (chunks > 65535u) return td_fail_internal(TD_E_LIMIT, "more samples than one launch takes (65 535 chunks)");
    int rc = td_handle_wait_work(h);
    if (rc) return rc;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    tdi::Events<2> ev;
    TD_HIPCHK(ev.create());
    const bool want_diploid = diploid_out || d_diploid_out;
    tdi::DevBuf<uint32_t> di, ncode, dcp;
    tdi::DevBuf<uint8_t> calls, diploid, pass;
    tdi::DevBuf<uint64_t> stats;
    tdi::DevBuf<unsigned long long> acc;                 // depth0[M] | depth1[M] | passed
    TD_HIPCHK(di.alloc(2ull * M));
    TD_HIPCHK(ncode.alloc((uint64_t)DS_NCLASS * M));
    TD_HIPCHK(acc.alloc(2ull * M + 1));
    TD_HIPCHK(calls.alloc((uint64_t)S * M));
    if (want_diploid) TD_HIPCHK(diploid.alloc((uint64_t)S * M));
    TD_HIPCHK(pass.alloc(M));
    TD_HIPCHK(stats.alloc((uint64_t)M * TD_DOSE_NSTATS));
    TD_HIPCHK(hipMemcpy(di.p, i0, (uint64_t)M * 4, hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(di.p + M, i1, (uint64_t)M * 4, hipMemcpyHostToDevice));
    if (hwe) {
        TD_HIPCHK(dcp.alloc(ncp));
        TD_HIPCHK(hipMemcpy(dcp.p, cp, (uint64_t)ncp * 4, hipMemcpyHostToDevice));
    }
    TD_HIPCHK(hipMemset(ncode.p, 0, (uint64_t)DS_NCLASS * M * 4));
    TD_HIPCHK(hipMemset(acc.p, 0, (2ull * M + 1) * 8));
    DoseLaunch a = {(const uint32_t *)d_counts, S, T, M, di.p, di.p + M, tab, dcp.p, p->min_depth, p->min_margin, calls.p,
                    want_diploid ? diploid.p : nullptr, ncode.p, acc.p, dim3((M + DS_TILE - 1) / DS_TILE, (uint32_t)chunks)};
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    if (hwe) {
        hipLaunchKernelGGL(k_dose_depth, a.grid, dim3(DS_TILE), 0, 0, a.counts, S, T, M, a.i0, a.i1, acc.p);
        TD_HIPCHK(hipGetLastError());
    }
    switch (P) {
    case 2: dose_launch<2>(a, hwe); break;
    case 3: dose_launch<3>(a, hwe); break;
    case 4: dose_launch<4>(a, hwe); break;
    case 5: dose_launch<5>(a, hwe); break;
    case 6: dose_launch<6>(a, hwe); break;
    case 7: dose_launch<7>(a, hwe); break;
    default: dose_launch<8>(a, hwe); break;
    }
    TD_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_dose_filter, dim3((M + 255) / 256), dim3(256), 0, 0, ncode.p, acc.p, S, M, P, p->min_call_ppm,
                       p->min_maf_ppm, stats.p, pass.p, acc.p + 2ull * M);
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
    TD_HIPCHK(hipMemcpy(stats_out, stats.p, (uint64_t)M * TD_DOSE_NSTATS * 8, hipMemcpyDeviceToHost));
    TD_HIPCHK(hipMemcpy(pass_out, pass.p, M, hipMemcpyDeviceToHost));
    if (calls_out) TD_HIPCHK(hipMemcpy(calls_out, calls.p, (uint64_t)S * M, hipMemcpyDeviceToHost));
    if (diploid_out) TD_HIPCHK(hipMemcpy(diploid_out, diploid.p, (uint64_t)S * M, hipMemcpyDeviceToHost));
    *passed_out = passed;
    if (d_calls_out) *d_calls_out = calls.release();
    if (d_diploid_out) *d_diploid_out = diploid.release();
    return TD_OK;
}
