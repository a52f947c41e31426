// The pre-pass of ld.hip and impute.hip: markers of the S x M call matrix (rows exactly M bytes apart) as rows.
//
// k_calls_transpose<COMPACT>: grid (tiles of CT_TILE markers), CT_THREADS threads.  COMPACT gathers the Mp participating
//    columns through idx[] (ld.hip's marker mask); otherwise row m of T is column m of the matrix and idx is not read.
//    T is Mpad rows of Spad bytes (multiples of CT_TILE and of CT_STEP), codes 0 / 1 / 2 and CT_MISSING for everything
//    else (missing, samples past S, rows past the last marker).  A thread reads 16 samples of one marker (the lanes of a
//    wave are 64 neighbouring markers of one sample: one run of bytes where the mask leaves neighbours), and the tile
//    goes through LDS so that four lanes write 64 contiguous bytes of a row.  called[] -- the samples called at every
//    one of the Mpad rows, 0 past the last marker -- falls out of the same pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {                                        // (internal to each including translation unit, as its other kernels are)

constexpr uint32_t CT_TILE = 64;                   // markers of a tile
constexpr uint32_t CT_STEP = 64;                   // samples staged at a time; Spad is a multiple
constexpr uint32_t CT_THREADS = 256;               // 4 waves
constexpr uint32_t CT_ROW = CT_STEP + 16;          // bytes between the tile's rows in LDS (padded against bank conflicts)
constexpr uint32_t CT_MISSING = 3;                 // what T holds for every byte that is not 0 / 1 / 2
static_assert(CT_THREADS == CT_TILE * (CT_STEP / 16), "a thread stages 16 samples of one marker");

typedef int ct_v4i __attribute__((ext_vector_type(4)));

template <bool COMPACT>
__global__ __launch_bounds__(CT_THREADS) void k_calls_transpose(const uint8_t *calls, uint32_t S, uint32_t M, const uint32_t *idx, uint32_t Mp,
                                                                uint32_t Spad, uint8_t *T, uint32_t *called) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[CT_TILE * CT_ROW];
    const uint32_t tid = threadIdx.x;
    // gather: marker (tid & 63) of this tile, samples 16 (tid >> 6) .. + 15 of a step
    const uint32_t gm = blockIdx.x * CT_TILE + (tid & 63u), gs = (tid >> 6) * 16u;
    const uint8_t *col = gm < (COMPACT ? Mp : M) ? calls + (COMPACT ? idx[gm] : gm) : nullptr;    // idx[] < M
    // write: row (tid >> 2) of this tile, bytes 16 (tid & 3) .. + 15 of a step
    const uint32_t wrow = tid >> 2, wq = (tid & 3u) * 16u;
    uint8_t *out = T + (size_t)(blockIdx.x * CT_TILE + wrow) * Spad + wq;          // T has Mpad rows: inside it
    uint32_t ncalled = 0;
    for (uint32_t s0 = 0; s0 < Spad; s0 += CT_STEP) {
        ct_v4i v;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t w = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t s = s0 + gs + 4u * d + k;
                uint32_t c = col && s < S ? (uint32_t)col[(size_t)s * M] : CT_MISSING;     // s < S, column < M: inside the matrix
                if (c > 2u) c = CT_MISSING;
                w |= c << (8 * k);
            }
            v[d] = (int)w;
        }
        *reinterpret_cast<ct_v4i *>(tile + (tid & 63u) * CT_ROW + gs) = v;
        __syncthreads();
        const ct_v4i r = *reinterpret_cast<const ct_v4i *>(tile + wrow * CT_ROW + wq);
        *reinterpret_cast<ct_v4i *>(out + s0) = r;                 // Spad and the steps are multiples of 64: aligned
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t w = (uint32_t)r[d];
            ncalled += 4u - (uint32_t)__popc(w & (w >> 1) & 0x01010101u);          // a byte is 3 iff its bits 0 and 1 are set
        }
        __syncthreads();
    }
    ncalled += __shfl_xor(ncalled, 1);
    ncalled += __shfl_xor(ncalled, 2);
    if ((tid & 3u) == 0) called[blockIdx.x * CT_TILE + wrow] = ncalled;           // (rows past the last marker count 0)
}

}  // namespace
