// The stable LSD radix sort of a permutation by multi-word keys, 8 bits per pass: K2 of csrc/tagset.hip (Tag Manager)
// and K2 of csrc/tagnet.hip (tag network).  Keys are word-major (key[w * n + i], word 0 the most significant) with a
// 16-bit length as the last tie-break; the permutation is sorted, the keys stay where they are.
//
// One pass: k_rs_hist (per-tile histograms, digit-major), k_rs_scan (one workgroup, exclusive scan), k_rs_scatter (per
// tile: a wave ranks its 64 elements by digit with eight ballots, waves and iterations in index order keep it stable).
// k_rs_same first marks the digit positions where some key differs from key 0; the others are skipped.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>

namespace tdrs {
namespace {   // internal linkage: every translation unit that includes this gets its own kernels

constexpr int RS_THREADS = 256;
constexpr int RS_ITEMS = 16;
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;     // 4 096 elements per workgroup
constexpr int RS_SCAN_THREADS = 1024;

// digit position p: 0, 1 the length's bytes; 2 + 8 r + k byte k of word W - 1 - r (least significant first)
__device__ __forceinline__ uint32_t rs_digit(const uint64_t *key, const uint16_t *len, uint32_t n, uint32_t W, uint32_t idx,
                                             uint32_t p) {
    if (p < 2) return (len[idx] >> (8 * p)) & 255u;
    const uint32_t r = (p - 2) >> 3, k = (p - 2) & 7;
    return (uint32_t)(key[(uint64_t)(W - 1 - r) * n + idx] >> (8 * k)) & 255u;
}

__global__ __launch_bounds__(256) void k_rs_same(const uint64_t *key, const uint16_t *len, uint32_t n, uint32_t W,
                                                 uint32_t *differ) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t npos = 2 + 8 * W;
    uint32_t m[3] = {0, 0, 0};
    if (i < n) {
        if (len[i] != len[0]) m[0] |= ((len[i] ^ len[0]) & 255u ? 1u : 0u) | ((len[i] ^ len[0]) >> 8 ? 2u : 0u);
        for (uint32_t w = 0; w < W; ++w) {
            const uint64_t x = key[(uint64_t)w * n + i] ^ key[(uint64_t)w * n];
            if (!x) continue;
            const uint32_t r = W - 1 - w;
            for (uint32_t k = 0; k < 8; ++k)
                if ((x >> (8 * k)) & 255u) {
                    const uint32_t p = 2 + 8 * r + k;
                    if (p < npos) m[p >> 5] |= 1u << (p & 31);
                }
        }
    }
    for (int q = 0; q < 3; ++q) {
        uint32_t v = m[q];
        for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicOr(&differ[q], v);
    }
}

__global__ __launch_bounds__(RS_THREADS) void k_rs_hist(const uint64_t *key, const uint16_t *len, const uint32_t *perm,
                                                        uint32_t n, uint32_t W, uint32_t p, uint32_t nblocks, uint32_t *hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * RS_TILE;
    for (int it = 0; it < RS_ITEMS; ++it) {
        const uint64_t j = base + (uint64_t)it * RS_THREADS + threadIdx.x;
        if (j < n) atomicAdd(&h[rs_digit(key, len, n, W, perm[j], p)], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of m entries in place, one workgroup
__global__ __launch_bounds__(RS_SCAN_THREADS) void k_rs_scan(uint32_t *a, uint64_t m) {
    __shared__ uint32_t part[RS_SCAN_THREADS];
    const uint64_t chunk = (m + RS_SCAN_THREADS - 1) / RS_SCAN_THREADS;
    const uint64_t lo0 = (uint64_t)threadIdx.x * chunk, lo = lo0 < m ? lo0 : m, hi = lo + chunk < m ? lo + chunk : m;
    uint32_t s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += a[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < RS_SCAN_THREADS; d <<= 1) {
        const uint32_t v = threadIdx.x >= (uint32_t)d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - s;
    for (uint64_t i = lo; i < hi; ++i) {
        const uint32_t v = a[i];
        a[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(RS_THREADS) void k_rs_scatter(const uint64_t *key, const uint16_t *len, const uint32_t *perm_in,
                                                           uint32_t *perm_out, uint32_t n, uint32_t W, uint32_t p,
                                                           uint32_t nblocks, const uint32_t *hist) {
    __shared__ uint32_t boff[256];
    __shared__ uint32_t wcnt[RS_THREADS / 64][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    boff[threadIdx.x] = hist[(uint64_t)threadIdx.x * nblocks + blockIdx.x];
    for (int w = 0; w < RS_THREADS / 64; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * RS_TILE;
    const uint64_t lt = (1ull << lane) - 1ull;
    for (int it = 0; it < RS_ITEMS; ++it) {
        const uint64_t j = base + (uint64_t)it * RS_THREADS + threadIdx.x;
        const bool valid = j < n;
        uint32_t v = 0, d = 0;
        if (valid) {
            v = perm_in[j];
            d = rs_digit(key, len, n, W, v, p);
        }
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bb = __ballot(valid && bit);
            peers &= bit ? bb : ~bb;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lt);
        if (valid && (peers >> lane) == 1ull) wcnt[wv][d] = (uint32_t)__popcll(peers);   // the highest peer
        __syncthreads();
        if (valid) {
            uint32_t dst = boff[d] + rank;
            for (int w = 0; w < wv; ++w) dst += wcnt[w][d];
            perm_out[dst] = v;
        }
        __syncthreads();
        uint32_t add = 0;
        for (int w = 0; w < RS_THREADS / 64; ++w) {
            add += wcnt[w][threadIdx.x];
            wcnt[w][threadIdx.x] = 0;
        }
        boff[threadIdx.x] += add;
        __syncthreads();
    }
}

inline uint32_t rs_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + RS_TILE - 1) / RS_TILE); }

// Sorts the permutation in *perm0 (n > 1 entries; *perm1 the second buffer) on the default stream; on return *perm0 is
// the sorted one (the two pointers are swapped after every pass).  differ: 3 words, zeroed by the caller; hist: 256 *
// rs_blocks(n) words.  Reads the differing digit positions back, so it synchronises once.  *passes: passes run.
inline hipError_t rs_sort(const uint64_t *key, const uint16_t *len, uint32_t n, uint32_t W, uint32_t **perm0, uint32_t **perm1,
                          uint32_t *differ, uint32_t *hist, uint32_t *passes) {
    const uint32_t nblocks = rs_blocks(n);
    hipLaunchKernelGGL(k_rs_same, dim3((n + 255) / 256), dim3(256), 0, 0, key, len, n, W, differ);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    uint32_t dif[3];
    if ((e = hipMemcpy(dif, differ, sizeof dif, hipMemcpyDeviceToHost)) != hipSuccess) return e;
    for (uint32_t p = 0; p < 2 + 8 * W; ++p) {
        if (!((dif[p >> 5] >> (p & 31)) & 1u)) continue;
        hipLaunchKernelGGL(k_rs_hist, dim3(nblocks), dim3(RS_THREADS), 0, 0, key, len, *perm0, n, W, p, nblocks, hist);
        hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(RS_SCAN_THREADS), 0, 0, hist, 256ull * nblocks);
        hipLaunchKernelGGL(k_rs_scatter, dim3(nblocks), dim3(RS_THREADS), 0, 0, key, len, *perm0, *perm1, n, W, p, nblocks, hist);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        std::swap(*perm0, *perm1);
        ++*passes;
    }
    return hipSuccess;
}

}  // namespace
}  // namespace tdrs
