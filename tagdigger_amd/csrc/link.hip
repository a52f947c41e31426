// Linkage of the markers of a cross from the call matrix (include/tagdig.h: td_link_counts, td_link_pairs).
//
// Input: the S x M uint8 call matrix where it lies in device memory (rows exactly M bytes apart), codes 0 / 1 / 2, any
// byte above 2 = missing; the offspring rows rows[R] (the parents never enter a sum); per marker a class pair (A, B) or
// "takes no part".  A cell is x = +1 for A, -1 for B, 0 otherwise.  Output of the pair call: the pairs of participating
// markers i < j with N = sum x_i^2 x_j^2 >= min_shared, rec = (N - |D|) / 2 with D = sum x_i x_j, rec 10^6 <= max_rf_ppm N
// and lod16 = 65536 N + f[rec] + f[N - rec] - f[N] >= min_lod16, as records (i, j, N, rec | phase << 31, lod16) ascending by
// (i, j); per marker the informative offspring and the edges it takes part in.
//
// k_link_counts: grid (1024 columns, LC_ROWS offspring rows), one wave.  A lane owns 16 neighbouring columns: one 16-byte
//    load per row where the row's address allows (M a multiple of 16), single bytes otherwise (odd M puts rows at odd
//    addresses).  The four classes are counted in the byte lanes of four words per class -- LC_ROWS <= 255 rows cannot carry
//    -- and added to counts[M][4] with atomics at the end.
// k_link_gather: the pre-pass; grid (tiles of 64 participating markers), 256 threads, the tiling of calls_transpose.hpp.
//    Gathers the offspring rows through rows[] and the participating columns through idx[], maps every code through the
//    marker's class pair and writes x marker-major as int8 (0x01, 0xFF, 0): X is Mpad rows of Rpad bytes, both multiples
//    of 64, zeros in the padding.  informative[] falls out of the same pass.
// k_link_pairs: grid (the tile pairs ti <= tj, decoded in closed form as ld.hip does), 256 threads, 2 x 2 waves over a
//    64 x 64 tile pair.  Per k-step of 64 offspring a thread loads 16 bytes of one row of either tile and expands them
//    ONCE into the planes X (as loaded) and V = X & 1 in LDS; two MFMA chains, X.X and V.V, give D and N.  The epilogue
//    decides every pair of the lane in integers; a pair that passes the two cheap tests reads three entries of lodtab in
//    device memory.  Degrees and edges leave as in ld.hip: one atomic per row half and per column, the edges of the wave
//    behind ONE atomic on the edge counter, nothing written past the capacity.
// The host sorts the edges by (i, j): the same bytes on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "td_internal.hpp"

namespace {

constexpr uint32_t LK_TILE = TD_LINK_TILE;         // markers along a workgroup's tile edge
constexpr uint32_t LK_KSTEP = 64;                  // offspring staged in LDS at a time: two MFMAs of k = 32
constexpr uint32_t LK_THREADS = 256;               // 4 waves, 2 x 2 over the tile pair
constexpr uint32_t LK_ROW = LK_KSTEP + 16;         // bytes between plane rows in LDS (padded against bank conflicts)
constexpr uint32_t LK_PLANE = LK_TILE * LK_ROW;    // bytes of one plane of one tile
constexpr uint32_t LK_GRID_X = 32768;              // tile pairs along grid x; y ends at 65 535
constexpr uint32_t LC_COLS = 16;                   // columns of a lane of k_link_counts
constexpr uint32_t LC_THREADS = 64;
constexpr uint32_t LC_ROWS = 32;                   // offspring rows of a workgroup: at most 255, the byte lanes must not carry
static_assert(LK_TILE == 64 && LK_THREADS == LK_TILE * (LK_KSTEP / 16), "a thread stages 16 offspring of one marker; 2 x 2 waves of 32 markers");
static_assert(sizeof(td_link_edge) == 24, "the edge record is four 32-bit words and one of 64 bits");
static_assert(LC_ROWS <= 255, "a byte lane counts the rows of a workgroup");

typedef int lk_v4i __attribute__((ext_vector_type(4)));
typedef int lk_v16i __attribute__((ext_vector_type(16)));

// the counts kernel of the calling thread's last td_link_counts; gather, pair kernel (device ms) and sort (host ms) of its last td_link_pairs
thread_local double g_link_times[4] = {0, 0, 0, 0};

// 0x01 in every byte of w that equals c
__device__ __forceinline__ uint32_t lk_eq(uint32_t w, uint32_t c) {
    const uint32_t d = w ^ (c * 0x01010101u);
    const uint32_t nz = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;      // 0x80 where the byte differs
    return (nz >> 7) ^ 0x01010101u;
}

__global__ __launch_bounds__(LC_THREADS) void k_link_counts(const uint8_t *calls, uint32_t M, const uint32_t *rows, uint32_t R, uint32_t *counts) {
    const uint32_t c0 = (blockIdx.x * LC_THREADS + threadIdx.x) * LC_COLS;
    if (c0 >= M) return;
    const bool whole = c0 + LC_COLS <= M;
    const uint32_t r0 = blockIdx.y * LC_ROWS, r1 = min(R, r0 + LC_ROWS);
    uint32_t acc[3][4];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int d = 0; d < 4; ++d) acc[g][d] = 0;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint8_t *p = calls + (size_t)rows[r] * M + c0;          // rows[] < S, c0 < M: inside the matrix
        uint32_t w[4];
        if (whole && ((uintptr_t)p & 15u) == 0) {                      // (uniform over the wave but for its last lane)
            const lk_v4i v = *reinterpret_cast<const lk_v4i *>(p);
#pragma unroll
            for (int d = 0; d < 4; ++d) w[d] = (uint32_t)v[d];
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                w[d] = 0x03030303u;                                    // past the last column: counted nowhere that is read
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    if (c0 + 4u * d + k < M) w[d] = (w[d] & ~(0xffu << (8 * k))) | ((uint32_t)p[4u * d + k] << (8 * k));
            }
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            acc[0][d] += lk_eq(w[d], 0);
            acc[1][d] += lk_eq(w[d], 1);
            acc[2][d] += lk_eq(w[d], 2);
        }
    }
    const uint32_t nrows = r1 - r0;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t c = c0 + 4u * d + k;
            if (c >= M) continue;
            const uint32_t n0 = acc[0][d] >> (8 * k) & 0xffu, n1 = acc[1][d] >> (8 * k) & 0xffu, n2 = acc[2][d] >> (8 * k) & 0xffu;
            uint32_t *out = counts + (size_t)c * 4;
            if (n0) atomicAdd(out + 0, n0);
            if (n1) atomicAdd(out + 1, n1);
            if (n2) atomicAdd(out + 2, n2);
            if (nrows - n0 - n1 - n2) atomicAdd(out + 3, nrows - n0 - n1 - n2);
        }
}

__global__ __launch_bounds__(LK_THREADS) void k_link_gather(const uint8_t *calls, uint32_t M, const uint32_t *rows, uint32_t R, const uint32_t *idx,
                                                            const uint8_t *cls, uint32_t Mp, uint32_t Rpad, uint8_t *X, uint32_t *informative) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[LK_TILE * LK_ROW];
    const uint32_t tid = threadIdx.x;
    // gather: marker (tid & 63) of this tile, offspring 16 (tid >> 6) .. + 15 of a step
    const uint32_t gm = blockIdx.x * LK_TILE + (tid & 63u), gs = (tid >> 6) * 16u;
    const uint8_t *col = gm < Mp ? calls + idx[gm] : nullptr;                      // idx[] < M
    const uint32_t k = col ? (uint32_t)cls[gm] : 0u;                               // 0: (A 0, B 1), 1: (A 2, B 1), 2: (A 0, B 2)
    const uint32_t code_a = k == 1u ? 2u : 0u, code_b = k == 2u ? 2u : 1u;
    // write: row (tid >> 2) of this tile, bytes 16 (tid & 3) .. + 15 of a step
    const uint32_t wrow = tid >> 2, wq = (tid & 3u) * 16u;
    uint8_t *out = X + (size_t)(blockIdx.x * LK_TILE + wrow) * Rpad + wq;          // X has Mpad rows: inside it
    uint32_t ninf = 0;
    for (uint32_t s0 = 0; s0 < Rpad; s0 += LK_KSTEP) {
        lk_v4i v;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t w = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t s = s0 + gs + 4u * d + b;
                if (col && s < R) {
                    const uint32_t c = (uint32_t)col[(size_t)rows[s] * M];         // rows[] < S, column < M: inside the matrix
                    w |= (c == code_a ? 0x01u : c == code_b ? 0xffu : 0u) << (8 * b);
                }
            }
            v[d] = (int)w;
        }
        *reinterpret_cast<lk_v4i *>(tile + (tid & 63u) * LK_ROW + gs) = v;
        __syncthreads();
        const lk_v4i r = *reinterpret_cast<const lk_v4i *>(tile + wrow * LK_ROW + wq);
        *reinterpret_cast<lk_v4i *>(out + s0) = r;                 // Rpad and the steps are multiples of 64: aligned
#pragma unroll
        for (int d = 0; d < 4; ++d) ninf += (uint32_t)__popc((uint32_t)r[d] & 0x01010101u);      // 0x01 and 0xFF both have bit 0
        __syncthreads();
    }
    ninf += __shfl_xor(ninf, 1);
    ninf += __shfl_xor(ninf, 2);
    if ((tid & 3u) == 0) informative[blockIdx.x * LK_TILE + wrow] = ninf;         // (rows past the last marker count 0)
}

// the planes X (signed: 0x01, 0xFF, 0) and V = X & 1 of 16 cells at dst, dst + LK_PLANE
__device__ __forceinline__ void lk_planes(uint8_t *dst, lk_v4i x) {
    lk_v4i v;
#pragma unroll
    for (int d = 0; d < 4; ++d) v[d] = (int)((uint32_t)x[d] & 0x01010101u);
    *reinterpret_cast<lk_v4i *>(dst) = x;
    *reinterpret_cast<lk_v4i *>(dst + LK_PLANE) = v;
}

// the rule on one pair's sums: is it an edge, and its rec and lod16 (n <= 16 384, |d| <= n, same parity)
__device__ __forceinline__ bool lk_decide(int32_t n_, int32_t d, const long long *lodtab, uint32_t max_rf_ppm, long long min_lod16, uint32_t min_shared,
                                          uint32_t *rec_out, long long *lod_out) {
    const uint32_t n = (uint32_t)n_, rec = (n - (uint32_t)(d < 0 ? -d : d)) >> 1;
    *rec_out = rec;
    if (n < min_shared || (uint64_t)rec * 1000000ull > (uint64_t)max_rf_ppm * n) return false;
    const long long lod = 65536ll * (long long)n + lodtab[rec] + lodtab[n - rec] - lodtab[n];    // rec <= n - rec <= n <= R: inside the table
    *lod_out = lod;
    return lod >= min_lod16;
}

__global__ __launch_bounds__(LK_THREADS, 2) void k_link_pairs(const uint8_t *X, uint32_t Rpad, uint32_t Mp, uint32_t npairs, const uint32_t *idx,
                                                              const long long *lodtab, uint32_t max_rf_ppm, long long min_lod16, uint32_t min_shared,
                                                              td_link_edge *edges, unsigned long long cap, unsigned long long *count,
                                                              uint32_t *degree) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 2 * LK_PLANE];
    // the tile pair ti <= tj of this workgroup: p = tj (tj + 1) / 2 + ti (below 2^28: exact in a double)
    const uint32_t p = blockIdx.y * LK_GRID_X + blockIdx.x;
    if (p >= npairs) return;                       // (the last row of the grid; uniform over the workgroup)
    uint32_t tj = (uint32_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (tj * (tj + 1u) / 2u > p) --tj;
    while ((tj + 1u) * (tj + 2u) / 2u <= p) ++tj;
    const uint32_t ti = p - tj * (tj + 1u) / 2u;
    const bool diag = ti == tj;
    const uint32_t nsteps = Rpad / LK_KSTEP;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t wr = wave >> 1, wc = wave & 1u;
    // staging: this thread's row of either tile and its 16 offspring of a step (X is padded: every load is whole and aligned)
    const uint32_t srow = tid >> 2, skof = (tid & 3u) * 16u;
    const uint8_t *row_i = X + (size_t)(ti * LK_TILE + srow) * Rpad + skof;
    const uint8_t *row_j = X + (size_t)(tj * LK_TILE + srow) * Rpad + skof;
    uint8_t *st_i = lds + srow * LK_ROW + skof, *st_j = st_i + 2 * LK_PLANE;
    // operands: row (lane & 31) of this wave's 32 markers, k half (lane >> 5), plane X at + 0 and V at + LK_PLANE
    const uint8_t *op_a = lds + (wr * 32u + (lane & 31u)) * LK_ROW + (lane >> 5) * 16u;
    const uint8_t *op_b = lds + (diag ? 0u : 2 * LK_PLANE) + (wc * 32u + (lane & 31u)) * LK_ROW + (lane >> 5) * 16u;

    lk_v16i a_d, a_n;
#pragma unroll
    for (int r = 0; r < 16; ++r) a_d[r] = a_n[r] = 0;

    lk_v4i ci = *reinterpret_cast<const lk_v4i *>(row_i), cj = ci;
    if (!diag) cj = *reinterpret_cast<const lk_v4i *>(row_j);
    for (uint32_t step = 0; step < nsteps; ++step) {
        lk_planes(st_i, ci);
        if (!diag) lk_planes(st_j, cj);
        __syncthreads();
        if (step + 1 < nsteps) {                   // in flight while the MFMAs run
            ci = *reinterpret_cast<const lk_v4i *>(row_i + (size_t)(step + 1) * LK_KSTEP);
            if (!diag) cj = *reinterpret_cast<const lk_v4i *>(row_j + (size_t)(step + 1) * LK_KSTEP);
        }
#pragma unroll
        for (uint32_t kh = 0; kh < 2; ++kh) {
            const lk_v4i xa = *reinterpret_cast<const lk_v4i *>(op_a + kh * 32u), va = *reinterpret_cast<const lk_v4i *>(op_a + LK_PLANE + kh * 32u);
            const lk_v4i xb = *reinterpret_cast<const lk_v4i *>(op_b + kh * 32u), vb = *reinterpret_cast<const lk_v4i *>(op_b + LK_PLANE + kh * 32u);
            a_d = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa, xb, a_d, 0, 0, 0);
            a_n = __builtin_amdgcn_mfma_i32_32x32x32_i8(va, vb, a_n, 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const uint32_t jc = tj * LK_TILE + wc * 32u + (lane & 31u);                  // compacted index of this lane's marker j
    const uint32_t ic0 = ti * LK_TILE + wr * 32u + 4u * (lane >> 5);              // ... of its marker i in register 0
    uint32_t emask = 0;                            // bit r: the pair of register r is an edge
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t ic = ic0 + (uint32_t)((r & 3) + 8 * (r >> 2));
        uint32_t rec;
        long long lod;
        const bool e = ic < jc && jc < Mp &&       // (compaction keeps the order: ic < jc iff i < j)
                       lk_decide(a_n[r], a_d[r], lodtab, max_rf_ppm, min_lod16, min_shared, &rec, &lod);
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
            uint32_t rec = 0;
            long long lod = 0;
            (void)lk_decide(a_n[r], a_d[r], lodtab, max_rf_ppm, min_lod16, min_shared, &rec, &lod);
            td_link_edge ed;
            ed.i = idx[ic0 + (uint32_t)((r & 3) + 8 * (r >> 2))];
            ed.j = j;
            ed.n = (uint32_t)a_n[r];
            ed.rec_phase = rec | (a_d[r] < 0 ? 0x80000000u : 0u);
            ed.lod16 = lod;
            edges[pos] = ed;
        }
        ++pos;
    }
}

// the checks both entry points share, and the offspring rows as a list (rows == NULL: all of them)
int link_rows(td_handle *h, uint32_t S, uint32_t M, const uint32_t *rows, uint32_t R, std::vector<uint32_t> &list) {
    if (!h) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (R > TD_LINK_MAX_SAMPLES) return td_fail_internal(TD_E_ARG, "more offspring rows than TD_LINK_MAX_SAMPLES");
    if (M >= 0x80000000u) return td_fail_internal(TD_E_ARG, "markers must number below 2^31");
    if (!rows && R != S) return td_fail_internal(TD_E_ARG, "rows == NULL takes every row: R must equal S");
    list.resize(R);
    if (!rows) {
        for (uint32_t r = 0; r < R; ++r) list[r] = r;
        return TD_OK;
    }
    for (uint32_t r = 0; r < R; ++r) {
        if (rows[r] >= S) {
            td_set_bad_index(r);
            return td_fail_internal(TD_E_ARG, ("rows[" + std::to_string(r) + "] = " + std::to_string(rows[r]) + " is not below S = " + std::to_string(S)).c_str());
        }
        list[r] = rows[r];
    }
    std::vector<uint32_t> sorted(list);
    std::sort(sorted.begin(), sorted.end());
    for (uint32_t r = 1; r < R; ++r)
        if (sorted[r] == sorted[r - 1])
            return td_fail_internal(TD_E_ARG, ("row " + std::to_string(sorted[r]) + " is listed twice").c_str());
    return TD_OK;
}

}  // namespace

extern "C" int td_link_last_times(td_handle *h, double *out4) {
    if (!h || !out4) return td_fail_internal(TD_E_ARG, "NULL argument");
    for (int k = 0; k < 4; ++k) out4[k] = g_link_times[k];
    return TD_OK;
}

extern "C" int td_link_counts(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const uint32_t *rows, uint32_t R, uint32_t *counts_out,
                              double *ms) {
    if (ms) *ms = 0;
    g_link_times[0] = 0;
    std::vector<uint32_t> list;
    int rc = link_rows(h, S, M, rows, R, list);
    if (rc) return rc;
    if (M && !counts_out) return td_fail_internal(TD_E_ARG, "NULL counts_out");
    if (R && M && !d_calls) return td_fail_internal(TD_E_ARG, "NULL call matrix");
    if (M) memset(counts_out, 0, (size_t)M * 4 * sizeof(uint32_t));
    if (R == 0 || M == 0) return TD_OK;            // zeros, no launch
    rc = td_handle_wait_work(h);
    if (rc) return rc;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    tdi::Events<2> ev;
    TD_HIPCHK(ev.create());
    tdi::DevBuf<uint32_t> d_rows, d_counts;
    TD_HIPCHK(d_rows.alloc(R));
    TD_HIPCHK(d_counts.alloc((size_t)M * 4));
    TD_HIPCHK(hipMemcpy(d_rows.p, list.data(), (size_t)R * sizeof(uint32_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemset(d_counts.p, 0, (size_t)M * 4 * sizeof(uint32_t)));
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    const uint32_t per = LC_THREADS * LC_COLS;     // M < 2^31: at most 2^21 workgroups along x; R <= 16 384: 512 along y
    hipLaunchKernelGGL(k_link_counts, dim3((M + per - 1) / per, (R + LC_ROWS - 1) / LC_ROWS), dim3(LC_THREADS), 0, 0, (const uint8_t *)d_calls, M,
                       d_rows.p, R, d_counts.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[1]));
    g_link_times[0] = ev.elapsed(0, 1);
    if (ms) *ms = g_link_times[0];
    TD_HIPCHK(hipMemcpy(counts_out, d_counts.p, (size_t)M * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return TD_OK;
}

extern "C" int td_link_pairs(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const uint32_t *rows, uint32_t R, const uint8_t *cls,
                             const int64_t *lodtab, uint32_t max_rf_ppm, int64_t min_lod16, uint32_t min_shared, td_link_edge *edges_out,
                             uint64_t capacity, uint64_t *n_out, uint32_t *degree_out, uint32_t *informative_out, double *ms) {
    if (n_out) *n_out = 0;
    if (ms) *ms = 0;
    g_link_times[1] = g_link_times[2] = g_link_times[3] = 0;
    std::vector<uint32_t> list;
    int rc = link_rows(h, S, M, rows, R, list);
    if (rc) return rc;
    if (max_rf_ppm > 500000u) return td_fail_internal(TD_E_ARG, "max_rf_ppm must be at most 500000");
    if (!lodtab) return td_fail_internal(TD_E_ARG, "NULL lodtab");
    if (M && !cls) return td_fail_internal(TD_E_ARG, "NULL cls");
    uint64_t taking = 0;
    for (uint32_t m = 0; m < M; ++m) {
        if (cls[m] > 2 && cls[m] != 255) {
            td_set_bad_index(m);
            return td_fail_internal(TD_E_ARG, ("cls[" + std::to_string(m) + "] = " + std::to_string((unsigned)cls[m]) + " is none of 0, 1, 2, 255").c_str());
        }
        taking += cls[m] != 255;
    }
    if (taking > TD_LINK_MAX_MARKERS)
        return td_fail_internal(TD_E_LIMIT, (std::to_string(taking) + " participating markers, more than TD_LINK_MAX_MARKERS = " +
                                             std::to_string((uint64_t)TD_LINK_MAX_MARKERS)).c_str());
    if (R && M && !d_calls) return td_fail_internal(TD_E_ARG, "NULL call matrix");
    const uint32_t Mp = (uint32_t)taking;
    if (degree_out && M) memset(degree_out, 0, (size_t)M * sizeof(uint32_t));
    if (informative_out && M) memset(informative_out, 0, (size_t)M * sizeof(uint32_t));
    if (R == 0 || Mp == 0) return TD_OK;           // no edges, nothing informative, no launch
    std::vector<uint32_t> idx(Mp);
    std::vector<uint8_t> pcls(Mp);
    for (uint32_t m = 0, k = 0; m < M; ++m)
        if (cls[m] != 255) {
            idx[k] = m;
            pcls[k++] = cls[m];
        }
    rc = td_handle_wait_work(h);
    if (rc) return rc;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    const uint32_t ntiles = (Mp + LK_TILE - 1) / LK_TILE;          // <= 16 384: ntiles (ntiles + 1) / 2 < 2^28 tile pairs
    const uint32_t npairs = (uint32_t)((uint64_t)ntiles * (ntiles + 1) / 2);
    const uint32_t Mpad = ntiles * LK_TILE, Rpad = (R + LK_KSTEP - 1) / LK_KSTEP * LK_KSTEP;
    const uint64_t pairs = (uint64_t)Mp * (Mp - 1) / 2;
    const uint64_t devcap = edges_out ? std::min(capacity, pairs) : 0;
    tdi::Events<3> ev;
    TD_HIPCHK(ev.create());
    tdi::DevBuf<uint32_t> d_idx, d_rows, d_inf, d_degree;
    tdi::DevBuf<uint8_t> d_cls, d_X;
    tdi::DevBuf<long long> d_tab;
    tdi::DevBuf<unsigned long long> d_count;
    tdi::DevBuf<td_link_edge> d_edges;
    TD_HIPCHK(d_idx.alloc(Mp));
    TD_HIPCHK(d_rows.alloc(R));
    TD_HIPCHK(d_cls.alloc(Mp));
    TD_HIPCHK(d_tab.alloc((size_t)R + 1));
    TD_HIPCHK(d_inf.alloc(Mpad));
    TD_HIPCHK(d_degree.alloc(Mpad));
    TD_HIPCHK(d_X.alloc((size_t)Mpad * Rpad));
    TD_HIPCHK(d_count.alloc(1));
    TD_HIPCHK(d_edges.alloc(devcap));
    TD_HIPCHK(hipMemcpy(d_idx.p, idx.data(), (size_t)Mp * sizeof(uint32_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(d_rows.p, list.data(), (size_t)R * sizeof(uint32_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(d_cls.p, pcls.data(), (size_t)Mp, hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(d_tab.p, lodtab, ((size_t)R + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemset(d_degree.p, 0, (size_t)Mpad * sizeof(uint32_t)));
    TD_HIPCHK(hipMemset(d_count.p, 0, sizeof(unsigned long long)));
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    hipLaunchKernelGGL(k_link_gather, dim3(ntiles), dim3(LK_THREADS), 0, 0, (const uint8_t *)d_calls, M, d_rows.p, R, d_idx.p, d_cls.p, Mp, Rpad,
                       d_X.p, d_inf.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    if (Mp > 1) {                                  // (one participating marker: informative only)
        hipLaunchKernelGGL(k_link_pairs, dim3(std::min(npairs, LK_GRID_X), (npairs + LK_GRID_X - 1) / LK_GRID_X), dim3(LK_THREADS), 0, 0, d_X.p, Rpad,
                           Mp, npairs, d_idx.p, d_tab.p, max_rf_ppm, (long long)min_lod16, min_shared, d_edges.p, (unsigned long long)devcap,
                           d_count.p, d_degree.p);
        TD_HIPCHK(hipGetLastError());
    }
    TD_HIPCHK(hipEventRecord(ev.e[2], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[2]));
    g_link_times[1] = ev.elapsed(0, 1);
    g_link_times[2] = ev.elapsed(1, 2);
    if (ms) *ms = g_link_times[1] + g_link_times[2];
    unsigned long long total = 0;
    TD_HIPCHK(hipMemcpy(&total, d_count.p, sizeof(total), hipMemcpyDeviceToHost));
    if (n_out) *n_out = total;
    if (degree_out || informative_out) {
        std::vector<uint32_t> tmp(Mp);
        if (degree_out) {
            TD_HIPCHK(hipMemcpy(tmp.data(), d_degree.p, (size_t)Mp * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (uint32_t k = 0; k < Mp; ++k) degree_out[idx[k]] = tmp[k];
        }
        if (informative_out) {
            TD_HIPCHK(hipMemcpy(tmp.data(), d_inf.p, (size_t)Mp * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (uint32_t k = 0; k < Mp; ++k) informative_out[idx[k]] = tmp[k];
        }
    }
    if (!edges_out) return TD_OK;                  // counted only
    if (total > capacity)
        return td_fail_internal(TD_E_LIMIT, (std::to_string(total) + " edges, the buffer holds " + std::to_string(capacity)).c_str());
    if (total) {
        TD_HIPCHK(hipMemcpy(edges_out, d_edges.p, (size_t)total * sizeof(td_link_edge), hipMemcpyDeviceToHost));
        const auto t0 = std::chrono::steady_clock::now();
        std::sort(edges_out, edges_out + total, [](const td_link_edge &a, const td_link_edge &b) {
            return a.i != b.i ? a.i < b.i : a.j < b.j;
        });
        g_link_times[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return TD_OK;
}
