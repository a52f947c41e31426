// Pairwise sample relations from the call matrix (include/tagdig.h: td_relate_joint).
//
// Input: the S x M uint8 call matrix where it lies in device memory (rows exactly M bytes apart, so in general not
// aligned), codes 0 / 1 / 2 = copies of allele 1, any byte above 2 = missing, and an optional marker mask use[M].
// Output: joint[i][j][a][b] (uint32, S x S x 3 x 3) = the participating markers m with calls[i][m] == a and
// calls[j][m] == b.  That is the Gram product X X^T of the one-hot planes X in {0, 1}, 3 S x M, exact in integers, and
// runs on the matrix cores (v_mfma_i32_32x32x32_i8).
//
// k_relate: grid (chunks of M, tile pairs ti <= tj), 256 threads.  A workgroup owns RL_TILE samples of tile ti against
//    RL_TILE samples of tile tj over RL_KCHUNK markers, RL_KSTEP at a time:
//      - a thread loads 16 call bytes of one sample of either tile and the 16 mask bytes of its markers (whole 16 bytes
//        where they lie inside the row and the chunk, byte by byte at a tail; nothing outside is read: such lanes hold
//        the missing code) while the MFMAs of the step before run;
//      - it expands them ONCE into three 16-byte 0/1 planes, ANDed with the mask, in LDS (rl_planes): every plane row is
//        then an operand of three MFMAs of two waves, so the expansion is paid once per 6 MFMA operands;
//      - wave (wr, wc) multiplies the three planes of samples 32 wr .. 32 wr + 31 of tile ti with those of samples
//        32 wc .. of tile tj: 3 x 3 blocks of 32 x 32 int32 accumulators.  Both operands come from LDS through the same
//        function of (row, lane), so the order of k inside an MFMA is the same on both sides whatever it is.
//    The accumulators of a chunk are added to joint with integer atomics (and, off the diagonal, to the mirrored cell
//    joint[j][i][b][a]): the result does not depend on the order of the chunks.  Zero accumulators are not written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "td_internal.hpp"

namespace {

constexpr uint32_t RL_TILE = TD_RELATE_TILE;       // samples along a workgroup's tile edge
constexpr uint32_t RL_KCHUNK = TD_RELATE_KCHUNK;   // markers of a workgroup
constexpr uint32_t RL_KSTEP = 64;                  // markers staged in LDS at a time: two MFMAs of k = 32
constexpr uint32_t RL_THREADS = 256;               // 4 waves, 2 x 2 over the tile pair
constexpr uint32_t RL_ROW = RL_KSTEP + 16;         // bytes between plane rows in LDS (padded against bank conflicts)
constexpr uint32_t RL_PLANE = RL_TILE * RL_ROW;    // bytes of one plane of one tile
static_assert(RL_TILE == 64 && RL_THREADS == RL_TILE * (RL_KSTEP / 16), "a thread stages 16 markers of one sample; 2 x 2 waves of 32 samples");
static_assert(RL_KCHUNK % RL_KSTEP == 0, "a chunk is walked in whole steps");

typedef int rl_v4i __attribute__((ext_vector_type(4)));
typedef int rl_v16i __attribute__((ext_vector_type(16)));

// 0x01 in every byte of x that equals `code`, 0x00 elsewhere (any byte value)
__host__ __device__ __forceinline__ uint32_t rl_eq(uint32_t x, uint32_t code) {
    x ^= code * 0x01010101u;
    const uint32_t t = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;      // bit 7 of a byte: the byte is not zero
    return (~t >> 7) & 0x01010101u;
}

// 0x01 in every byte of x that is not zero
__host__ __device__ __forceinline__ uint32_t rl_nonzero(uint32_t x) {
    return ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7) & 0x01010101u;
}

// 16 bytes from p, of which only [0, n) may be read; the others come out as `fill`
__device__ __forceinline__ rl_v4i rl_load16(const uint8_t *p, uint32_t n, uint32_t fill) {
    rl_v4i v;
    if (n >= 16u) {
        __builtin_memcpy(&v, p, 16);               // (rows are M bytes apart: no alignment is assumed)
    } else {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t w = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) w |= (4u * d + k < n ? (uint32_t)p[4 * d + k] : fill) << (8 * k);
            v[d] = (int)w;
        }
    }
    return v;
}

// the three planes of 16 calls under 16 mask bytes (0x01 / 0x00) at dst, dst + RL_PLANE, dst + 2 RL_PLANE
__device__ __forceinline__ void rl_planes(uint8_t *dst, rl_v4i c, rl_v4i ok) {
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
        rl_v4i q;
#pragma unroll
        for (int d = 0; d < 4; ++d) q[d] = (int)(rl_eq((uint32_t)c[d], a) & (uint32_t)ok[d]);
        *reinterpret_cast<rl_v4i *>(dst + a * RL_PLANE) = q;
    }
}

__global__ __launch_bounds__(RL_THREADS, 2) void k_relate(const uint8_t *calls, uint32_t S, uint32_t M, const uint8_t *use,
                                                           uint32_t ntiles, uint32_t *joint
#ifdef TD_RELATE_CLOCK                             // diagnostic build of tools/relate_clock.hip only: never in the library
                                                           , unsigned long long *clk
#endif
) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 3 * RL_PLANE];
    // the tile pair of this workgroup: blockIdx.y counts the pairs ti <= tj row by row
    uint32_t ti = 0, rest = blockIdx.y;
    while (rest >= ntiles - ti) {
        rest -= ntiles - ti;
        ++ti;
    }
    const uint32_t tj = ti + rest;
    const bool diag = ti == tj;
    const uint32_t m_lo = blockIdx.x * RL_KCHUNK;                  // < M < 2^31
    const uint32_t m_hi = M - m_lo < RL_KCHUNK ? M : m_lo + RL_KCHUNK;
    const uint32_t nsteps = (m_hi - m_lo + RL_KSTEP - 1) / RL_KSTEP;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t wr = wave >> 1, wc = wave & 1u;
    // staging: this thread's sample of either tile and its 16 markers of a step
    const uint32_t srow = tid >> 2, skof = (tid & 3u) * 16u;
    const uint32_t si = ti * RL_TILE + srow, sj = tj * RL_TILE + srow;
    const uint8_t *row_i = si < S ? calls + (size_t)si * M : nullptr;
    const uint8_t *row_j = !diag && sj < S ? calls + (size_t)sj * M : nullptr;
    uint8_t *st_i = lds + srow * RL_ROW + skof, *st_j = st_i + 3 * RL_PLANE;
    // operands: row (lane & 31) of this wave's 32 samples, k half (lane >> 5), of plane a at + a RL_PLANE
    const uint8_t *op_a = lds + (wr * 32u + (lane & 31u)) * RL_ROW + (lane >> 5) * 16u;
    const uint8_t *op_b = lds + (diag ? 0u : 3 * RL_PLANE) + (wc * 32u + (lane & 31u)) * RL_ROW + (lane >> 5) * 16u;

#ifdef TD_RELATE_CLOCK
    const unsigned long long clk_core = clock64(), clk_real = wall_clock64();
#endif
    rl_v16i acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0;

    const rl_v4i none = {-1, -1, -1, -1};          // 0xff: missing
    rl_v4i ci = none, cj = none, mk = {0, 0, 0, 0};
    auto fetch = [&](uint32_t step) {
        const uint32_t m0 = m_lo + step * RL_KSTEP + skof;
        const uint32_t n = m0 < m_hi ? m_hi - m0 : 0u;             // markers of this thread's 16 inside the chunk
        ci = row_i && n ? rl_load16(row_i + m0, n, 0xffu) : none;
        cj = row_j && n ? rl_load16(row_j + m0, n, 0xffu) : none;
        if (!n) mk = rl_v4i{0, 0, 0, 0};
        else if (use) mk = rl_load16(use + m0, n, 0u);
        else mk = rl_v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};      // (markers past the end carry 0xff calls)
    };
    fetch(0);
    for (uint32_t step = 0; step < nsteps; ++step) {
        rl_v4i ok;
#pragma unroll
        for (int d = 0; d < 4; ++d) ok[d] = (int)rl_nonzero((uint32_t)mk[d]);
        rl_planes(st_i, ci, ok);
        if (!diag) rl_planes(st_j, cj, ok);
        __syncthreads();
        if (step + 1 < nsteps) fetch(step + 1);    // in flight while the MFMAs run
#pragma unroll
        for (uint32_t kh = 0; kh < 2; ++kh) {
            rl_v4i fa[3], fb[3];
#pragma unroll
            for (uint32_t a = 0; a < 3; ++a) {
                fa[a] = *reinterpret_cast<const rl_v4i *>(op_a + a * RL_PLANE + kh * 32u);
                fb[a] = *reinterpret_cast<const rl_v4i *>(op_b + a * RL_PLANE + kh * 32u);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }
#ifdef TD_RELATE_CLOCK                             // core cycles and 100 MHz ticks over the marker loop, summed over the workgroups
    if (tid == 0) {
        atomicAdd(clk, clock64() - clk_core);
        atomicAdd(clk + 1, wall_clock64() - clk_real);
    }
#endif

    // C/D of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const uint32_t j = tj * RL_TILE + wc * 32u + (lane & 31u);
    if (j >= S) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t i = ti * RL_TILE + wr * 32u + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5);
        if (i >= S) continue;
        uint32_t *cell = joint + ((size_t)i * S + j) * 9u, *mirror = joint + ((size_t)j * S + i) * 9u;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const uint32_t v = (uint32_t)acc[a][b][r];
                if (v) {
                    atomicAdd(cell + a * 3 + b, v);
                    if (!diag) atomicAdd(mirror + b * 3 + a, v);
                }
            }
    }
}

}  // namespace

#ifndef TD_RELATE_CLOCK                            // (the diagnostic build launches the kernel itself)
extern "C" int td_relate_joint(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const uint8_t *use,
                               uint32_t *joint_out, void **d_joint_out, double *ms) {
    if (d_joint_out) *d_joint_out = nullptr;
    if (ms) *ms = 0;
    if (S > TD_RELATE_MAX_SAMPLES) return td_fail_internal(TD_E_ARG, "more samples than TD_RELATE_MAX_SAMPLES");
    if (M >= 0x80000000u) return td_fail_internal(TD_E_ARG, "markers must number below 2^31");
    if (!h) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (S && M && !d_calls) return td_fail_internal(TD_E_ARG, "NULL call matrix");
    const uint64_t cells = 9ull * S * S;
    if (S == 0 || M == 0) {                        // nothing takes part: all zero (or empty), no launch
        if (joint_out) memset(joint_out, 0, cells * sizeof(uint32_t));
        if (d_joint_out) {
            TD_HIPCHK(hipSetDevice(td_handle_device(h)));
            tdi::DevBuf<uint32_t> out;
            TD_HIPCHK(out.alloc(cells));
            TD_HIPCHK(hipMemset(out.p, 0, (cells ? cells : 1) * sizeof(uint32_t)));
            *d_joint_out = out.release();
        }
        return TD_OK;
    }
    int rc = td_handle_wait_work(h);
    if (rc) return rc;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    tdi::Events<2> ev;
    TD_HIPCHK(ev.create());
    tdi::DevBuf<uint32_t> out;
    tdi::DevBuf<uint8_t> duse;
    TD_HIPCHK(out.alloc(cells));
    if (use) {
        TD_HIPCHK(duse.alloc(M));
        TD_HIPCHK(hipMemcpy(duse.p, use, M, hipMemcpyHostToDevice));
    }
    TD_HIPCHK(hipMemset(out.p, 0, cells * sizeof(uint32_t)));
    const uint32_t ntiles = (S + RL_TILE - 1) / RL_TILE;           // <= 256: ntiles (ntiles + 1) / 2 <= 32 896 in grid y
    const uint32_t chunks = (M + RL_KCHUNK - 1) / RL_KCHUNK;       // <= 65 536 in grid x
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    hipLaunchKernelGGL(k_relate, dim3(chunks, ntiles * (ntiles + 1) / 2), dim3(RL_THREADS), 0, 0, (const uint8_t *)d_calls, S, M,
                       use ? duse.p : nullptr, ntiles, out.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[1]));
    if (ms) {
        float f = 0;
        TD_HIPCHK(hipEventElapsedTime(&f, ev.e[0], ev.e[1]));
        *ms = f;
    }
    if (joint_out) TD_HIPCHK(hipMemcpy(joint_out, out.p, cells * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (d_joint_out) *d_joint_out = out.release();
    return TD_OK;
}
#endif
