// Pairwise marker LD from the call matrix (include/tagdig.h: td_ld_pairs).
//
// Input: the S x M uint8 call matrix where it lies in device memory (rows exactly M bytes apart), codes 0 / 1 / 2 =
// copies of allele 1, any byte above 2 = missing, and an optional marker mask use[M] (host).  Output: the pairs of
// participating markers i < j whose r^2 over the samples called at both reaches min_r2_ppm, as integer records
// (i, j, shared, cov, var_i, var_j), ascending by (i, j); per marker the samples called and the edges it takes part in.
// The six sums behind cov and var are Gram products over the SAMPLES of the planes C (called, 0 / 1), X (dosage,
// 0 / 1 / 2) and Q (dosage squared, 0 / 1 / 4), on the matrix cores (v_mfma_i32_32x32x32_i8): the transpose of relate.hip.
//
// k_calls_transpose<true> (calls_transpose.hpp, shared with impute.hip): gathers the participating columns through
//    idx[] and writes them as rows: T is M'pad rows of Spad bytes (both multiples of 64), codes 0 / 1 / 2 and 3 for
//    everything else (missing, samples past S, rows past M').  called[] falls out of the same pass.
// k_ld_pairs: grid (the tile pairs ti <= tj, LD_GRID_X to a row of the grid, decoded in closed form), 256 threads.  A
//    workgroup owns 64 markers of tile ti against 64 of tile tj over all samples, LD_KSTEP at a time:
//      - a thread loads 16 aligned bytes of one row of either tile (while the MFMAs of the step before run) and expands
//        them ONCE into the three planes in LDS;
//      - wave (wr, wc) multiplies C.C, X.C, C.X, X.X, Q.C, C.Q of markers 32 wr .. of tile ti with markers 32 wc .. of
//        tile tj: 6 blocks of 32 x 32 int32 accumulators.  Both operands come from LDS through the same function of
//        (row, lane), so the order of k inside an MFMA is the same on both sides whatever it is;
//      - the epilogue decides every pair of the lane in integers (32-bit cov and var, 64-bit squares, a 128-bit
//        comparison), adds the degrees with one atomic per row half and per column, and appends the edges of the wave
//        to the edge buffer behind ONE atomic on the edge counter.  A record past the buffer's capacity is counted and
//        not written.
// The host sorts the edges by (i, j): what the device appended in the order of its atomics comes back the same bytes
// on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "calls_transpose.hpp"
#include "td_internal.hpp"

namespace {

constexpr uint32_t LD_TILE = TD_LD_TILE;           // markers along a workgroup's tile edge
constexpr uint32_t LD_KSTEP = CT_STEP;             // samples staged in LDS at a time: two MFMAs of k = 32
constexpr uint32_t LD_THREADS = CT_THREADS;        // 4 waves, 2 x 2 over the tile pair
constexpr uint32_t LD_ROW = CT_ROW;                // bytes between plane rows in LDS (padded against bank conflicts)
constexpr uint32_t LD_PLANE = LD_TILE * LD_ROW;    // bytes of one plane of one tile
constexpr uint32_t LD_GRID_X = 32768;              // tile pairs along grid x: a dimension holds fewer than 2^32 threads, and y ends at 65 535
static_assert(LD_TILE == CT_TILE && CT_MISSING == 3, "a workgroup takes the rows of a transpose tile; ld_planes reads a code with bits 0 and 1 set as missing");
static_assert(LD_TILE == 64 && LD_THREADS == LD_TILE * (LD_KSTEP / 16), "a thread stages 16 samples of one marker; 2 x 2 waves of 32 markers");
static_assert(sizeof(td_ld_edge) == 24, "the edge record is six 32-bit words");

typedef int ld_v4i __attribute__((ext_vector_type(4)));
typedef int ld_v16i __attribute__((ext_vector_type(16)));

// the transpose, pair kernel (device ms) and sort (host ms) of the calling thread's last td_ld_pairs
thread_local double g_ld_times[3] = {0, 0, 0};

// the planes C, X, Q of 16 codes 0 .. 3 at dst, dst + LD_PLANE, dst + 2 LD_PLANE
__device__ __forceinline__ void ld_planes(uint8_t *dst, ld_v4i c) {
    ld_v4i pc, px, pq;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t w = (uint32_t)c[d];
        const uint32_t miss = w & (w >> 1) & 0x01010101u;          // 0x01 where the code is 3
        const uint32_t x = w ^ (miss * 3u);                        // the dosage, 0 where missing
        pc[d] = (int)(miss ^ 0x01010101u);
        px[d] = (int)x;
        pq[d] = (int)((x & 0x01010101u) | ((x & 0x02020202u) << 1));              // 0, 1, 4
    }
    *reinterpret_cast<ld_v4i *>(dst) = pc;
    *reinterpret_cast<ld_v4i *>(dst + LD_PLANE) = px;
    *reinterpret_cast<ld_v4i *>(dst + 2 * LD_PLANE) = pq;
}

// a * 10^6 >= b * ppm as 128-bit values (a, b <= 2^56: either side reaches 76 bits)
__device__ __forceinline__ bool ld_reaches(uint64_t a, uint64_t b, uint32_t ppm) {
    const uint64_t alo = a * 1000000ull, ahi = __umul64hi(a, 1000000ull);
    const uint64_t blo = b * (uint64_t)ppm, bhi = __umul64hi(b, (uint64_t)ppm);
    return ahi > bhi || (ahi == bhi && alo >= blo);
}

__global__ __launch_bounds__(LD_THREADS, 2) void k_ld_pairs(const uint8_t *T, uint32_t Spad, uint32_t Mp, uint32_t npairs, const uint32_t *idx,
                                                            uint32_t min_r2_ppm, uint32_t min_shared, td_ld_edge *edges,
                                                            unsigned long long cap, unsigned long long *count, uint32_t *degree) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 3 * LD_PLANE];
    // the tile pair ti <= tj of this workgroup: p = tj (tj + 1) / 2 + ti (below 2^28: exact in a double)
    const uint32_t p = blockIdx.y * LD_GRID_X + blockIdx.x;
    if (p >= npairs) return;                       // (the last row of the grid; uniform over the workgroup)
    uint32_t tj = (uint32_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (tj * (tj + 1u) / 2u > p) --tj;
    while ((tj + 1u) * (tj + 2u) / 2u <= p) ++tj;
    const uint32_t ti = p - tj * (tj + 1u) / 2u;
    const bool diag = ti == tj;
    const uint32_t nsteps = Spad / LD_KSTEP;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t wr = wave >> 1, wc = wave & 1u;
    // staging: this thread's row of either tile and its 16 samples of a step (T is padded: every load is whole and aligned)
    const uint32_t srow = tid >> 2, skof = (tid & 3u) * 16u;
    const uint8_t *row_i = T + (size_t)(ti * LD_TILE + srow) * Spad + skof;
    const uint8_t *row_j = T + (size_t)(tj * LD_TILE + srow) * Spad + skof;
    uint8_t *st_i = lds + srow * LD_ROW + skof, *st_j = st_i + 3 * LD_PLANE;
    // operands: row (lane & 31) of this wave's 32 markers, k half (lane >> 5), of plane a at + a LD_PLANE
    const uint8_t *op_a = lds + (wr * 32u + (lane & 31u)) * LD_ROW + (lane >> 5) * 16u;
    const uint8_t *op_b = lds + (diag ? 0u : 3 * LD_PLANE) + (wc * 32u + (lane & 31u)) * LD_ROW + (lane >> 5) * 16u;

    ld_v16i a_n, a_sx, a_sy, a_sxy, a_sxx, a_syy;
#pragma unroll
    for (int r = 0; r < 16; ++r) a_n[r] = a_sx[r] = a_sy[r] = a_sxy[r] = a_sxx[r] = a_syy[r] = 0;

    ld_v4i ci = *reinterpret_cast<const ld_v4i *>(row_i), cj = ci;
    if (!diag) cj = *reinterpret_cast<const ld_v4i *>(row_j);
    for (uint32_t step = 0; step < nsteps; ++step) {
        ld_planes(st_i, ci);
        if (!diag) ld_planes(st_j, cj);
        __syncthreads();
        if (step + 1 < nsteps) {                   // in flight while the MFMAs run
            ci = *reinterpret_cast<const ld_v4i *>(row_i + (size_t)(step + 1) * LD_KSTEP);
            if (!diag) cj = *reinterpret_cast<const ld_v4i *>(row_j + (size_t)(step + 1) * LD_KSTEP);
        }
#pragma unroll
        for (uint32_t kh = 0; kh < 2; ++kh) {
            ld_v4i fa[3], fb[3];                   // C, X, Q of the markers i (rows of the result) and j (columns)
#pragma unroll
            for (uint32_t a = 0; a < 3; ++a) {
                fa[a] = *reinterpret_cast<const ld_v4i *>(op_a + a * LD_PLANE + kh * 32u);
                fb[a] = *reinterpret_cast<const ld_v4i *>(op_b + a * LD_PLANE + kh * 32u);
            }
            a_n = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[0], fb[0], a_n, 0, 0, 0);
            a_sx = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[1], fb[0], a_sx, 0, 0, 0);
            a_sy = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[0], fb[1], a_sy, 0, 0, 0);
            a_sxy = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[1], fb[1], a_sxy, 0, 0, 0);
            a_sxx = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[2], fb[0], a_sxx, 0, 0, 0);
            a_syy = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[0], fb[2], a_syy, 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const uint32_t jc = tj * LD_TILE + wc * 32u + (lane & 31u);                  // compacted index of this lane's marker j
    const uint32_t ic0 = ti * LD_TILE + wr * 32u + 4u * (lane >> 5);              // ... of its marker i in register 0
    uint32_t emask = 0;                            // bit r: the pair of register r is an edge
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t ic = ic0 + (uint32_t)((r & 3) + 8 * (r >> 2));
        const uint32_t n = (uint32_t)a_n[r];
        bool e = ic < jc && jc < Mp && n >= min_shared;          // (compaction keeps the order: ic < jc iff i < j)
        if (e) {
            const uint32_t sx = (uint32_t)a_sx[r], sy = (uint32_t)a_sy[r];
            const uint32_t var_i = n * (uint32_t)a_sxx[r] - sx * sx, var_j = n * (uint32_t)a_syy[r] - sy * sy;     // <= 2^28
            e = var_i != 0u && var_j != 0u;
            if (e) {
                const int64_t cov = (int64_t)(int32_t)(n * (uint32_t)a_sxy[r] - sx * sy);      // |cov| <= 2^28
                e = ld_reaches((uint64_t)(cov * cov), (uint64_t)var_i * var_j, min_r2_ppm);
            }
        }
        const unsigned long long b = __ballot(e);
        if (b) {                                   // the 32 lanes of a half share the row: one atomic for its degree
            emask |= (uint32_t)e << r;
            const uint32_t half = (uint32_t)__popcll(lane < 32u ? b & 0xffffffffull : b >> 32);
            if ((lane & 31u) == 0 && half) atomicAdd(degree + ic, half);
        }
    }
    const uint32_t mine = (uint32_t)__popc(emask);
    uint32_t incl = mine;                          // inclusive scan over the wave
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const uint32_t total = __shfl(incl, 63);
    if (total == 0) return;                        // (uniform over the wave)
    if (mine) atomicAdd(degree + jc, mine);
    uint32_t base_lo = 0, base_hi = 0;
    if (lane == 0) {
        const unsigned long long base = atomicAdd(count, (unsigned long long)total);
        base_lo = (uint32_t)base;
        base_hi = (uint32_t)(base >> 32);
    }
    base_lo = __shfl(base_lo, 0);
    base_hi = __shfl(base_hi, 0);
    unsigned long long pos = (((unsigned long long)base_hi << 32) | base_lo) + (incl - mine);
    if (!mine) return;
    const uint32_t j = idx[jc];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (!(emask >> r & 1u)) continue;
        if (pos < cap) {                           // nothing past the caller's capacity is written
            const uint32_t n = (uint32_t)a_n[r], sx = (uint32_t)a_sx[r], sy = (uint32_t)a_sy[r];
            td_ld_edge ed;
            ed.i = idx[ic0 + (uint32_t)((r & 3) + 8 * (r >> 2))];
            ed.j = j;
            ed.shared = n;
            ed.cov = (int32_t)(n * (uint32_t)a_sxy[r] - sx * sy);
            ed.var_i = n * (uint32_t)a_sxx[r] - sx * sx;
            ed.var_j = n * (uint32_t)a_syy[r] - sy * sy;
            edges[pos] = ed;
        }
        ++pos;
    }
}

}  // namespace

extern "C" int td_ld_last_times(td_handle *h, double *out3) {
    if (!h || !out3) return td_fail_internal(TD_E_ARG, "NULL argument");
    for (int k = 0; k < 3; ++k) out3[k] = g_ld_times[k];
    return TD_OK;
}

extern "C" int td_ld_pairs(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const uint8_t *use, uint32_t min_r2_ppm,
                           uint32_t min_shared, td_ld_edge *edges_out, uint64_t capacity, uint64_t *n_out, uint32_t *degree_out,
                           uint32_t *called_out, double *ms) {
    if (n_out) *n_out = 0;
    if (ms) *ms = 0;
    g_ld_times[0] = g_ld_times[1] = g_ld_times[2] = 0;
    if (S > TD_LD_MAX_SAMPLES) return td_fail_internal(TD_E_ARG, "more samples than TD_LD_MAX_SAMPLES");
    if (M >= 0x80000000u) return td_fail_internal(TD_E_ARG, "markers must number below 2^31");
    if (min_r2_ppm > 1000000u) return td_fail_internal(TD_E_ARG, "min_r2_ppm must be at most 1000000");
    if (!h) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (S && M && !d_calls) return td_fail_internal(TD_E_ARG, "NULL call matrix");
    uint64_t taking = M;
    if (use) {
        taking = 0;
        for (uint32_t m = 0; m < M; ++m) taking += use[m] != 0;
    }
    if (taking > TD_LD_MAX_MARKERS)
        return td_fail_internal(TD_E_LIMIT, (std::to_string(taking) + " participating markers, more than TD_LD_MAX_MARKERS = " +
                                             std::to_string((uint64_t)TD_LD_MAX_MARKERS)).c_str());
    const uint32_t Mp = (uint32_t)taking;
    if (degree_out && M) memset(degree_out, 0, (size_t)M * sizeof(uint32_t));
    if (called_out && M) memset(called_out, 0, (size_t)M * sizeof(uint32_t));
    if (S == 0 || Mp == 0) return TD_OK;           // no edges, nothing called, no launch
    std::vector<uint32_t> idx(Mp);
    for (uint32_t m = 0, k = 0; m < M; ++m)
        if (!use || use[m]) idx[k++] = m;
    int rc = td_handle_wait_work(h);
    if (rc) return rc;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    if (Mp == 1) {                                 // no pair: the one column is counted on the host, without a launch
        if (called_out) {
            std::vector<uint8_t> col(S);
            TD_HIPCHK(hipMemcpy2D(col.data(), 1, (const uint8_t *)d_calls + idx[0], M, 1, S, hipMemcpyDeviceToHost));
            uint32_t n = 0;
            for (uint8_t c : col) n += c <= 2;
            called_out[idx[0]] = n;
        }
        return TD_OK;
    }
    const uint32_t ntiles = (Mp + LD_TILE - 1) / LD_TILE;          // <= 16 384: ntiles (ntiles + 1) / 2 < 2^28 tile pairs
    const uint32_t npairs = (uint32_t)((uint64_t)ntiles * (ntiles + 1) / 2);
    const uint32_t Mpad = ntiles * LD_TILE, Spad = (S + LD_KSTEP - 1) / LD_KSTEP * LD_KSTEP;
    const uint64_t pairs = (uint64_t)Mp * (Mp - 1) / 2;
    const uint64_t devcap = edges_out ? std::min(capacity, pairs) : 0;
    tdi::Events<3> ev;
    TD_HIPCHK(ev.create());
    tdi::DevBuf<uint32_t> d_idx, d_called, d_degree;
    tdi::DevBuf<uint8_t> d_T;
    tdi::DevBuf<unsigned long long> d_count;
    tdi::DevBuf<td_ld_edge> d_edges;
    TD_HIPCHK(d_idx.alloc(Mp));
    TD_HIPCHK(d_called.alloc(Mpad));
    TD_HIPCHK(d_degree.alloc(Mpad));
    TD_HIPCHK(d_T.alloc((size_t)Mpad * Spad));
    TD_HIPCHK(d_count.alloc(1));
    TD_HIPCHK(d_edges.alloc(devcap));
    TD_HIPCHK(hipMemcpy(d_idx.p, idx.data(), (size_t)Mp * sizeof(uint32_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemset(d_degree.p, 0, (size_t)Mpad * sizeof(uint32_t)));
    TD_HIPCHK(hipMemset(d_count.p, 0, sizeof(unsigned long long)));
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    hipLaunchKernelGGL(k_calls_transpose<true>, dim3(ntiles), dim3(CT_THREADS), 0, 0, (const uint8_t *)d_calls, S, M, d_idx.p, Mp, Spad,
                       d_T.p, d_called.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    hipLaunchKernelGGL(k_ld_pairs, dim3(std::min(npairs, LD_GRID_X), (npairs + LD_GRID_X - 1) / LD_GRID_X), dim3(LD_THREADS), 0, 0,
                       d_T.p, Spad, Mp, npairs, d_idx.p, min_r2_ppm, min_shared, d_edges.p, (unsigned long long)devcap, d_count.p, d_degree.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[2], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[2]));
    float f0 = 0, f1 = 0;
    TD_HIPCHK(hipEventElapsedTime(&f0, ev.e[0], ev.e[1]));
    TD_HIPCHK(hipEventElapsedTime(&f1, ev.e[1], ev.e[2]));
    g_ld_times[0] = f0;
    g_ld_times[1] = f1;
    if (ms) *ms = (double)f0 + (double)f1;
    unsigned long long total = 0;
    TD_HIPCHK(hipMemcpy(&total, d_count.p, sizeof(total), hipMemcpyDeviceToHost));
    if (n_out) *n_out = total;
    if (degree_out || called_out) {
        std::vector<uint32_t> tmp(Mp);
        if (degree_out) {
            TD_HIPCHK(hipMemcpy(tmp.data(), d_degree.p, (size_t)Mp * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (uint32_t k = 0; k < Mp; ++k) degree_out[idx[k]] = tmp[k];
        }
        if (called_out) {
            TD_HIPCHK(hipMemcpy(tmp.data(), d_called.p, (size_t)Mp * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (uint32_t k = 0; k < Mp; ++k) called_out[idx[k]] = tmp[k];
        }
    }
    if (!edges_out) return TD_OK;                  // counted only
    if (total > capacity)
        return td_fail_internal(TD_E_LIMIT, (std::to_string(total) + " edges, the buffer holds " + std::to_string(capacity)).c_str());
    if (total) {
        TD_HIPCHK(hipMemcpy(edges_out, d_edges.p, (size_t)total * sizeof(td_ld_edge), hipMemcpyDeviceToHost));
        const auto t0 = std::chrono::steady_clock::now();
        std::sort(edges_out, edges_out + total, [](const td_ld_edge &a, const td_ld_edge &b) {
            return a.i != b.i ? a.i < b.i : a.j < b.j;
        });
        g_ld_times[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return TD_OK;
}
