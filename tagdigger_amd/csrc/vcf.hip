// VCF body lines (GT:AD:DP, optionally :GQ:PL) formatted on the device from the count matrix and the calls where they
// lie (include/tagdig.h: td_vcf_format, td_vcf_file).
//
// A body line is prefix[k] (the eight fixed columns and FORMAT, built by the caller; only copied here), then for every
// sample a tab and the cell, then a newline.  For line k, marker m = sel[k], sample s: a = counts[s][i0[m]],
// b = counts[s][i1[m]], n = a + b (64-bit), code = calls[s][m], P the ploidy.  The cell:
//   GT   code <= P: P - code times 0, then code times 1, joined by '/';  code > P: '.' P times, joined by '/'
//   AD   a,b     DP   n
//   with likelihoods (P = 2 only): missing (code > 2) ".:.", else GQ:PL0,PL1,PL2 in integers:
//        n > 127: x = 127 a / n, y = 127 b / n (floor), else a, b;  c[g] = y ca[g] + x cb[g];  cmin = min c
//        PL[g] = min(255, ((c[g] - cmin) 30103 + 327680000) / 655360000);  GQ = min(99, min over g != code of PL[g])
//
// The matrix is sample-major and a line runs along the samples, every cell has its own width and every offset depends on
// all cells before it: measure / scan / emit, as place.hip's count / scan / emit.
// K1 k_vcf_measure: grid (ceil(K / VCF_MTILE), sample chunks of VCF_CHUNK), one thread per line walking its chunk's rows
//    as k_gc_call does (lanes along markers: coalesced, an aligned adjacent pair of columns in one 8-byte load).  Writes
//    chunk_len[chunk][k], the bytes of that chunk's cells with their tabs.  No atomics.
// K2 k_vcf_line_len / k_vcf_scan_blocks / k_vcf_offsets: line_len[k] = prefix_len[k] + sum of chunk_len + 1, the exclusive
//    64-bit scan over the K lines into line_off[0 .. K] (block sums, one block over the sums, block scans), and the 64-bit
//    start of every (chunk, line).
// K3 k_vcf_emit: a workgroup takes (tile of VCF_TILE lines, sample chunk).  Counts and calls are loaded with lanes along
//    the lines (coalesced along markers) into LDS tiles whose rows are padded by one element; then a wave takes a line with
//    lane = sample: the cell's length comes from comparisons against powers of ten, the wave scans the 64 lengths with
//    __shfl_up, and every lane writes its cell's bytes into the wave's LDS segment at its offset (straight into LDS: a
//    byte-addressed buffer in registers would be scratch).  The segment starts at the line's residue mod 16, so the wave
//    copies it out with aligned 16-byte stores and writes the unaligned head and tail bytewise.  The chunk-0 wave copies the
//    prefix, the last chunk's wave appends the newline.
// The cell itself (fields, length, bytes) is vcf_cell.hpp: plain C++ that san/vcf_san.cpp also compiles for the host.
// Emission runs in ranges of consecutive lines (vcf_ranges.hpp), offsets relative to the range's first line, through two
// device and two pinned host buffers: range r + 1 is formatted while range r is copied out and consumed by the host.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>

#include <chrono>
#include <string>
#include <vector>

#include "td_internal.hpp"
#include "vcf_cell.hpp"
#include "vcf_ranges.hpp"

namespace {

constexpr uint32_t VCF_TILE = TD_VCF_TILE;         // lines of an emit workgroup
constexpr uint32_t VCF_MTILE = TD_VCF_MTILE;       // lines of a measure workgroup = its threads
constexpr uint32_t VCF_CHUNK = TD_VCF_CHUNK;       // samples of a workgroup = the lanes of a wave
constexpr uint32_t VCF_THREADS = 256;              // emit: 4 waves
constexpr uint32_t VCF_WAVES = VCF_THREADS / 64;
constexpr uint32_t VCF_ROWS = 4;                   // sample rows whose loads a thread has in flight at once
constexpr uint32_t VCF_PAD = VCF_CHUNK + 1;        // elements between the rows of an LDS tile (padded against bank conflicts)
constexpr uint32_t VCF_SCAN = 256;                 // lines of a scan workgroup = its threads
constexpr uint64_t VCF_LAUNCH_LINES = 1u << 22;    // lines of one emit launch: a range with more takes several launches
// A cell with its tab is at most 64 bytes: tab, GT (2 P - 1 <= 15), ':', AD (10 + 1 + 10), ':', DP (n <= 2^33 - 2: 10
// digits); with likelihoods P = 2 (GT 3) and ':' GQ (2) ':' PL (3 + 1 + 3 + 1 + 3) follow.
constexpr uint32_t VCF_CELL_PLAIN = 1 + (2 * TD_DOSE_MAX_PLOIDY - 1) + 1 + 21 + 1 + 10;
constexpr uint32_t VCF_CELL_LIK = 1 + 3 + 1 + 21 + 1 + 10 + 1 + 2 + 1 + 11;
static_assert(VCF_CELL_PLAIN <= TD_VCF_CELL_MAX && VCF_CELL_LIK <= TD_VCF_CELL_MAX, "a cell with its tab is at most 64 bytes");
constexpr uint32_t VCF_SEG = VCF_CHUNK * TD_VCF_CELL_MAX + 32;      // a wave's segment: 15 bytes of residue, the cells, the newline
static_assert(VCF_CHUNK == 64, "lane = sample");
static_assert(VCF_THREADS == VCF_WAVES * VCF_TILE, "a thread stages one line over every fourth sample row");
static_assert(VCF_CHUNK % (VCF_WAVES * VCF_ROWS) == 0 && VCF_CHUNK % VCF_ROWS == 0, "rows are walked VCF_ROWS at a time");
static_assert(VCF_SEG % 16 == 0, "segments stay 16-byte aligned");

// two adjacent columns that start an aligned 8 bytes in every row come in one load -- when that holds for every marker of
// the wave (lanes without a line agree): the answer is uniform, so the row loop keeps one kind of load
__device__ __forceinline__ bool vcf_pair(const uint32_t *counts, uint32_t T, uint32_t c0, uint32_t c1, bool live) {
    return __all(!live || (c1 == c0 + 1 && !(c0 & 1u) && !(T & 1u) && !((uintptr_t)counts & 7u)));
}

// the VCF_ROWS rows from `row` on, `step` rows apart, of which those with u < left exist: loads issued before the first use
__device__ __forceinline__ void vcf_load(const uint32_t *row, const uint8_t *call, uint32_t T, uint32_t M, uint32_t c0, uint32_t c1,
                                         bool pair, uint32_t step, uint32_t left, uint32_t (&a)[VCF_ROWS], uint32_t (&b)[VCF_ROWS],
                                         uint32_t (&c)[VCF_ROWS]) {
#pragma unroll
    for (uint32_t u = 0; u < VCF_ROWS; ++u) {
        a[u] = b[u] = c[u] = 0;
        if (u < left) {
            const uint32_t *r = row + (size_t)u * step * T;
            if (pair) {
                const uint64_t v = *reinterpret_cast<const uint64_t *>(r + c0);
                a[u] = (uint32_t)v;
                b[u] = (uint32_t)(v >> 32);
            } else {
                a[u] = r[c0];
                b[u] = r[c1];
            }
            c[u] = call[(size_t)u * step * M];
        }
    }
}

// ------------------------------------------------------------------ K1
template <bool LIK>
__global__ __launch_bounds__(VCF_MTILE) void k_vcf_measure(const uint32_t *counts, uint32_t S, uint32_t T, uint32_t M, const uint32_t *i0,
                                                           const uint32_t *i1, const uint8_t *calls, const uint32_t *sel, uint32_t K,
                                                           const VcfTab tab, uint32_t P, uint32_t *chunk_len) {
    const uint32_t k = blockIdx.x * VCF_MTILE + threadIdx.x;
    const bool live = k < K;
    const uint32_t m = live ? sel[k] : 0;          // < M: the host checked them
    const uint32_t c0 = live ? i0[m] : 0, c1 = live ? i1[m] : 0;  // both < T: the host checked them
    const bool pair = vcf_pair(counts, T, c0, c1, live);
    if (!live) return;
    const uint32_t s_lo = blockIdx.y * VCF_CHUNK;
    const uint32_t s_hi = S - s_lo < VCF_CHUNK ? S : s_lo + VCF_CHUNK;
    const uint32_t *row = counts + (size_t)s_lo * T;
    const uint8_t *call = calls + (size_t)s_lo * M + m;
    uint32_t total = 0;
    for (uint32_t s = s_lo; s < s_hi; s += VCF_ROWS, row += (size_t)VCF_ROWS * T, call += (size_t)VCF_ROWS * M) {
        uint32_t a[VCF_ROWS], b[VCF_ROWS], c[VCF_ROWS];
        vcf_load(row, call, T, M, c0, c1, pair, 1, s_hi - s, a, b, c);
#pragma unroll
        for (uint32_t u = 0; u < VCF_ROWS; ++u)
            if (s + u < s_hi) total += vcf_cell_len<LIK>(vcf_cell<LIK>(a[u], b[u], c[u], tab), P);
    }
    chunk_len[(size_t)blockIdx.y * K + k] = total;   // <= 64 * 64
}

// ------------------------------------------------------------------ K2
__device__ __forceinline__ uint64_t vcf_line_len(const uint32_t *chunk_len, const uint64_t *prefix_off, uint32_t K, uint32_t chunks, uint32_t k) {
    uint64_t len = prefix_off[k + 1] - prefix_off[k] + 1;
    for (uint32_t c = 0; c < chunks; ++c) len += chunk_len[(size_t)c * K + k];
    return len;
}

// inclusive scan of one value per thread over the VCF_SCAN threads of a block
__device__ __forceinline__ uint64_t vcf_block_scan(uint64_t v, uint64_t *s) {
    const uint32_t t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < VCF_SCAN; d <<= 1) {
        const uint64_t add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    return s[t];
}

__global__ __launch_bounds__(VCF_SCAN) void k_vcf_line_len(const uint32_t *chunk_len, const uint64_t *prefix_off, uint32_t K, uint32_t chunks,
                                                           uint64_t *line_len, uint64_t *block_sum) {
    __shared__ uint64_t s[VCF_SCAN];
    const uint32_t k = blockIdx.x * VCF_SCAN + threadIdx.x;
    const uint64_t len = k < K ? vcf_line_len(chunk_len, prefix_off, K, chunks, k) : 0;
    if (k < K) line_len[k] = len;
    const uint64_t incl = vcf_block_scan(len, s);
    if (threadIdx.x == VCF_SCAN - 1) block_sum[blockIdx.x] = incl;
}

// one block: block_sum[0 .. nb) -> its exclusive scan in place, the total -> *total
__global__ __launch_bounds__(VCF_SCAN) void k_vcf_scan_blocks(uint64_t *block_sum, uint32_t nb, uint64_t *total) {
    __shared__ uint64_t s[VCF_SCAN];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nb; base += VCF_SCAN) {
        const uint32_t j = base + threadIdx.x;
        const uint64_t v = j < nb ? block_sum[j] : 0;
        const uint64_t incl = vcf_block_scan(v, s);
        if (j < nb) block_sum[j] = carry + incl - v;
        carry += s[VCF_SCAN - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// line_off[k] and, where start is not NULL, the start of every (chunk, line): start[chunk][k]
__global__ __launch_bounds__(VCF_SCAN) void k_vcf_offsets(const uint32_t *chunk_len, const uint64_t *prefix_off, uint32_t K, uint32_t chunks,
                                                          const uint64_t *line_len, const uint64_t *block_off, uint64_t *line_off,
                                                          uint64_t *start) {
    __shared__ uint64_t s[VCF_SCAN];
    const uint32_t k = blockIdx.x * VCF_SCAN + threadIdx.x;
    const uint64_t len = k < K ? line_len[k] : 0;
    const uint64_t incl = vcf_block_scan(len, s);
    if (k >= K) return;
    const uint64_t off = block_off[blockIdx.x] + incl - len;
    line_off[k] = off;
    if (k == K - 1) line_off[K] = off + len;
    if (start) {
        uint64_t at = off + (prefix_off[k + 1] - prefix_off[k]);
        for (uint32_t c = 0; c < chunks; ++c) {
            start[(size_t)c * K + k] = at;
            at += chunk_len[(size_t)c * K + k];
        }
    }
}

// ------------------------------------------------------------------ K3
// lines k_lo .. k_hi - 1 into out[0 .. cap), offsets relative to base = line_off[k_lo]
template <bool LIK>
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_emit(const uint32_t *counts, uint32_t S, uint32_t T, uint32_t M, const uint32_t *i0,
                                                          const uint32_t *i1, const uint8_t *calls, const uint32_t *sel, uint32_t K,
                                                          uint32_t k_lo, uint32_t k_hi, const VcfTab tab, uint32_t P, const uint8_t *prefix,
                                                          const uint64_t *prefix_off, const uint64_t *line_off, const uint64_t *start,
                                                          uint64_t base, uint8_t *out, uint64_t cap) {
    __shared__ uint32_t s_a[VCF_TILE * VCF_PAD], s_b[VCF_TILE * VCF_PAD];
    __shared__ uint8_t s_c[VCF_TILE * VCF_PAD];
    __shared__ __attribute__((aligned(16))) uint8_t s_seg[VCF_WAVES * VCF_SEG];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k0 = k_lo + blockIdx.x * VCF_TILE;             // < k_hi by the grid
    const uint32_t s_lo = blockIdx.y * VCF_CHUNK;
    const uint32_t rows = S - s_lo < VCF_CHUNK ? S - s_lo : VCF_CHUNK;
    {   // stage: line `lane` of the tile, sample rows wave, wave + 4, ... of the chunk
        const uint32_t k = k0 + lane;
        const bool live = k < k_hi;
        const uint32_t m = live ? sel[k] : 0;      // < M: the host checked them
        const uint32_t c0 = live ? i0[m] : 0, c1 = live ? i1[m] : 0;
        const bool pair = vcf_pair(counts, T, c0, c1, live);
        if (live) {
            const uint32_t *row = counts + (size_t)(s_lo + wave) * T;
            const uint8_t *call = calls + (size_t)(s_lo + wave) * M + m;
            for (uint32_t r = wave; r < rows; r += VCF_WAVES * VCF_ROWS, row += (size_t)VCF_WAVES * VCF_ROWS * T,
                          call += (size_t)VCF_WAVES * VCF_ROWS * M) {
                uint32_t a[VCF_ROWS], b[VCF_ROWS], c[VCF_ROWS];
                vcf_load(row, call, T, M, c0, c1, pair, VCF_WAVES, (rows - r + VCF_WAVES - 1) / VCF_WAVES, a, b, c);
#pragma unroll
                for (uint32_t u = 0; u < VCF_ROWS; ++u) {
                    const uint32_t rr = r + u * VCF_WAVES;
                    if (rr < rows) {
                        s_a[lane * VCF_PAD + rr] = a[u];
                        s_b[lane * VCF_PAD + rr] = b[u];
                        s_c[lane * VCF_PAD + rr] = (uint8_t)c[u];
                    }
                }
            }
        }
    }
    __syncthreads();
    const bool first = blockIdx.y == 0, last = blockIdx.y == gridDim.y - 1;
    uint8_t *seg = s_seg + wave * VCF_SEG;
    // every wave runs the same number of rounds (the barrier inside is the workgroup's); a wave without a line idles
    for (uint32_t l0 = 0; l0 < VCF_TILE && k0 + l0 < k_hi; l0 += VCF_WAVES) {
        const uint32_t l = l0 + wave, k = k0 + l;
        const bool line = k < k_hi;                // (the same in every lane of the wave)
        const bool cell = line && lane < rows;
        VcfCell c = {};
        uint32_t len = 0;
        if (cell) {
            c = vcf_cell<LIK>(s_a[l * VCF_PAD + lane], s_b[l * VCF_PAD + lane], s_c[l * VCF_PAD + lane], tab);
            len = vcf_cell_len<LIK>(c, P);
        }
        uint32_t incl = len;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        uint32_t total = __shfl(incl, 63);         // <= 64 * 64
        uint64_t at = 0;                           // where this (chunk, line) starts in out
        uint32_t res = 0;
        if (line) {
            at = start[(size_t)blockIdx.y * K + k] - base;
            res = (uint32_t)at & 15u;              // out is 16-byte aligned: the segment starts at the same residue
            if (cell) vcf_put_cell<LIK>(seg + res + (incl - len), c, P);
            if (last) {
                if (lane == 0) seg[res + total] = '\n';
                total += 1;
            }
        }
        __syncthreads();
        if (line && at + total <= cap) {           // (always: the buffer holds the range the scan measured)
            uint8_t *dst = out + at;
            const uint8_t *src = seg + res;
            const uint32_t head = (16u - res) & 15u;
            const uint32_t nhead = head < total ? head : total;
            if (lane < nhead) dst[lane] = src[lane];
            const uint32_t nvec = (total - nhead) >> 4;
            for (uint32_t v = lane; v < nvec; v += 64)             // src + nhead and dst + nhead are 16-byte aligned
                *reinterpret_cast<uint4 *>(dst + nhead + 16u * v) = *reinterpret_cast<const uint4 *>(src + nhead + 16u * v);
            const uint32_t done = nhead + 16u * nvec;
            if (lane < total - done) dst[done + lane] = src[done + lane];
            if (first) {                           // the prefix, in front of chunk 0's cells
                const uint64_t p0 = prefix_off[k], plen = prefix_off[k + 1] - p0, lo = line_off[k] - base;
                for (uint64_t i = lane; i < plen; i += 64) out[lo + i] = prefix[p0 + i];
            }
        }
        // (the next round's writes to the segment follow this round's reads in the same wave: LDS keeps a wave's order)
    }
}


struct VcfInput {
    td_handle *h; const void *counts; uint32_t S, T, M; const uint32_t *i0, *i1; const void *calls; const td_vcf_params *p;
    const uint32_t *sel; uint32_t K; const uint8_t *prefix; const uint64_t *prefix_off;
};

// what the host does with a range: `n` bytes that lie `at` bytes into the output
struct VcfSink {
    virtual int take(const uint8_t *bytes, uint64_t n, uint64_t at) = 0;
    virtual ~VcfSink() = default;
};

struct MemorySink : VcfSink {
    uint8_t *out;
    explicit MemorySink(uint8_t *o) : out(o) {}
    int take(const uint8_t *bytes, uint64_t n, uint64_t at) override {
        memcpy(out + at, bytes, n);
        return TD_OK;
    }
};

struct FileSink : VcfSink {
    int fd = -1;
    std::string path;
    double write_ms = 0;
    ~FileSink() override { if (fd >= 0) (void)close(fd); }
    int open_at(const char *p, int append) {
        path = p;
        fd = open(p, O_WRONLY | O_CREAT | (append ? O_APPEND : O_TRUNC) | O_CLOEXEC, 0666);
        return fd >= 0 ? TD_OK : td_fail_internal(TD_E_IO, (path + ": " + strerror(errno)).c_str());
    }
    int take(const uint8_t *bytes, uint64_t n, uint64_t) override {
        const auto t0 = std::chrono::steady_clock::now();
        while (n) {
            const ssize_t w = write(fd, bytes, n < (1u << 30) ? (size_t)n : (size_t)1 << 30);
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) return td_fail_internal(TD_E_IO, (path + ": " + (w < 0 ? strerror(errno) : "write() wrote nothing")).c_str());
            bytes += w;
            n -= (uint64_t)w;
        }
        write_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return TD_OK;
    }
    int finish() {
        const int rc = close(fd);
        fd = -1;
        return rc == 0 ? TD_OK : td_fail_internal(TD_E_IO, (path + ": " + strerror(errno)).c_str());
    }
};

// the argument checks of both entry points: nothing is launched, opened or written before they pass
int vcf_check(const VcfInput &in) {
    if (!in.h || !in.p) return td_fail_internal(TD_E_ARG, "NULL argument");
    const td_vcf_params &p = *in.p;
    if (p.ploidy < 2 || p.ploidy > TD_DOSE_MAX_PLOIDY) return td_fail_internal(TD_E_ARG, "ploidy must be 2..8");
    if (p.likelihoods > 1) return td_fail_internal(TD_E_ARG, "likelihoods must be 0 or 1");
    if (p.likelihoods && p.ploidy != 2) return td_fail_internal(TD_E_ARG, "likelihoods need ploidy 2");
    if (p.likelihoods)
        for (uint32_t g = 0; g < 3; ++g)
            if (p.ca[g] > (uint32_t)TD_DOSE_COST_MAX || p.cb[g] > (uint32_t)TD_DOSE_COST_MAX)
                return td_fail_internal(TD_E_ARG, ("ca[" + std::to_string(g) + "] or cb[" + std::to_string(g) + "] exceeds 2^23").c_str());
    if (in.M && (!in.i0 || !in.i1)) return td_fail_internal(TD_E_ARG, "NULL argument");
    for (uint32_t m = 0; m < in.M; ++m) {
        if (in.i0[m] >= in.T || in.i1[m] >= in.T || in.i0[m] == in.i1[m]) {
            td_set_bad_index(m);
            return td_fail_internal(TD_E_ARG, ("marker " + std::to_string(m) + ": columns " + std::to_string(in.i0[m]) + " and " +
                                               std::to_string(in.i1[m]) + (in.i0[m] == in.i1[m] && in.i0[m] < in.T ? " are the same" :
                                               " are not both below T = " + std::to_string(in.T))).c_str());
        }
    }
    if (in.K && (!in.sel || !in.prefix_off)) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (in.K > (uint32_t)TD_VCF_MAX_LINES) return td_fail_internal(TD_E_LIMIT, "more lines than one call takes (2^30)");
    for (uint32_t k = 0; k < in.K; ++k) {
        if (in.sel[k] >= in.M) {
            td_set_bad_index(k);
            return td_fail_internal(TD_E_ARG, ("sel[" + std::to_string(k) + "] = " + std::to_string(in.sel[k]) + " is not below M = " +
                                               std::to_string(in.M)).c_str());
        }
    }
    for (uint32_t k = 0; k < in.K; ++k) {
        if (in.prefix_off[k + 1] < in.prefix_off[k]) {
            td_set_bad_index(k);
            return td_fail_internal(TD_E_ARG, ("prefix_off[" + std::to_string(k + 1) + "] is below prefix_off[" + std::to_string(k) + "]").c_str());
        }
    }
    if (in.K && in.prefix_off[in.K] > in.prefix_off[0] && !in.prefix) return td_fail_internal(TD_E_ARG, "NULL prefix bytes");
    if (in.K && in.S) {
        if (!in.counts || !in.calls) return td_fail_internal(TD_E_ARG, "NULL count matrix or call matrix");
        if (((uintptr_t)in.counts & 3u) != 0) return td_fail_internal(TD_E_ARG, "the count matrix must be 4-byte aligned");
        if (((uint64_t)in.S + VCF_CHUNK - 1) / VCF_CHUNK > 65535u)
            return td_fail_internal(TD_E_LIMIT, "more samples than one launch takes (65 535 chunks)");
    }
    return TD_OK;
}

template <bool LIK> void vcf_launch_measure(const VcfInput &in, const uint32_t *di, const uint32_t *dsel, const VcfTab &tab, uint32_t chunks,
                                            uint32_t *chunk_len) {
    hipLaunchKernelGGL(k_vcf_measure<LIK>, dim3((in.K + VCF_MTILE - 1) / VCF_MTILE, chunks), dim3(VCF_MTILE), 0, 0,
                       (const uint32_t *)in.counts, in.S, in.T, in.M, di, di + in.M, (const uint8_t *)in.calls, dsel, in.K, tab, in.p->ploidy,
                       chunk_len);
}

// measure, scan and -- with a sink -- emit.  *n_out = the bytes of all lines; with `capacity` below that: TD_E_LIMIT before
// anything is emitted.  ms: measure, scan, emit.  *ranges_out = the ranges emitted (0 where nothing was launched).
int vcf_run(const VcfInput &in, uint64_t *line_off_out, VcfSink *sink, uint64_t capacity, uint64_t *n_out, uint64_t *ranges_out, double *ms) {
    const uint32_t K = in.K, S = in.S;
    std::vector<uint64_t> line_off((size_t)K + 1, 0);
    if (K == 0) {
        if (line_off_out) line_off_out[0] = 0;
        return TD_OK;
    }
    if (S == 0) {                                  // no sample: every line is its prefix and the newline, put together here
        for (uint32_t k = 0; k < K; ++k) line_off[k + 1] = line_off[k] + (in.prefix_off[k + 1] - in.prefix_off[k]) + 1;
        *n_out = line_off[K];
        if (line_off_out) memcpy(line_off_out, line_off.data(), ((size_t)K + 1) * 8);
        if (!sink) return TD_OK;
        if (line_off[K] > capacity) return td_fail_internal(TD_E_LIMIT, ("the output takes " + std::to_string(line_off[K]) + " bytes").c_str());
        std::vector<uint8_t> text((size_t)line_off[K]);
        for (uint32_t k = 0; k < K; ++k) {
            const uint64_t n = in.prefix_off[k + 1] - in.prefix_off[k];
            if (n) memcpy(text.data() + line_off[k], in.prefix + in.prefix_off[k], n);
            text[line_off[k] + n] = '\n';
        }
        return sink->take(text.data(), text.size(), 0);
    }
    const td_vcf_params &p = *in.p;
    const uint32_t chunks = (uint32_t)(((uint64_t)S + VCF_CHUNK - 1) / VCF_CHUNK);
    const uint32_t nb = (K + VCF_SCAN - 1) / VCF_SCAN;
    const uint64_t pbase = in.prefix_off[0], pbytes = in.prefix_off[K] - pbase;
    VcfTab tab = {};
    if (p.likelihoods)
        for (uint32_t g = 0; g < 3; ++g) {
            tab.ca[g] = p.ca[g];
            tab.cb[g] = p.cb[g];
        }
    int rc = td_handle_wait_work(in.h);
    if (rc) return rc;
    TD_HIPCHK(hipSetDevice(td_handle_device(in.h)));
    tdi::Events<3> ev;
    TD_HIPCHK(ev.create());
    tdi::DevBuf<uint32_t> di, dsel, chunk_len;
    tdi::DevBuf<uint8_t> dprefix, dout[2];
    tdi::DevBuf<uint64_t> dpoff, line_len, block_sum, dline_off, start;
    tdi::PinBuf<uint8_t> pin[2];
    TD_HIPCHK(di.alloc(2ull * in.M));
    TD_HIPCHK(dsel.alloc(K));
    TD_HIPCHK(chunk_len.alloc((uint64_t)chunks * K));
    TD_HIPCHK(dpoff.alloc((uint64_t)K + 1));
    TD_HIPCHK(line_len.alloc(K));
    TD_HIPCHK(block_sum.alloc((uint64_t)nb + 1));
    TD_HIPCHK(dline_off.alloc((uint64_t)K + 1));
    TD_HIPCHK(hipMemcpy(di.p, in.i0, (uint64_t)in.M * 4, hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(di.p + in.M, in.i1, (uint64_t)in.M * 4, hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(dsel.p, in.sel, (uint64_t)K * 4, hipMemcpyHostToDevice));
    {   // the prefix offsets, from 0
        std::vector<uint64_t> rel((size_t)K + 1);
        for (uint32_t k = 0; k <= K; ++k) rel[k] = in.prefix_off[k] - pbase;
        TD_HIPCHK(hipMemcpy(dpoff.p, rel.data(), ((uint64_t)K + 1) * 8, hipMemcpyHostToDevice));
    }
    if (sink) {
        TD_HIPCHK(start.alloc((uint64_t)chunks * K));
        TD_HIPCHK(dprefix.alloc(pbytes));
        if (pbytes) TD_HIPCHK(hipMemcpy(dprefix.p, in.prefix + pbase, pbytes, hipMemcpyHostToDevice));
    }
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    if (p.likelihoods) vcf_launch_measure<true>(in, di.p, dsel.p, tab, chunks, chunk_len.p);
    else vcf_launch_measure<false>(in, di.p, dsel.p, tab, chunks, chunk_len.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    hipLaunchKernelGGL(k_vcf_line_len, dim3(nb), dim3(VCF_SCAN), 0, 0, chunk_len.p, dpoff.p, K, chunks, line_len.p, block_sum.p);
    TD_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_vcf_scan_blocks, dim3(1), dim3(VCF_SCAN), 0, 0, block_sum.p, nb, block_sum.p + nb);
    TD_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_vcf_offsets, dim3(nb), dim3(VCF_SCAN), 0, 0, chunk_len.p, dpoff.p, K, chunks, line_len.p, block_sum.p, dline_off.p,
                       sink ? start.p : nullptr);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[2], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[2]));
    if (ms) {
        ms[0] = ev.elapsed(0, 1);
        ms[1] = ev.elapsed(1, 2);
    }
    TD_HIPCHK(hipMemcpy(line_off.data(), dline_off.p, ((uint64_t)K + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t total = line_off[K];
    *n_out = total;
    if (line_off_out) memcpy(line_off_out, line_off.data(), ((size_t)K + 1) * 8);
    if (!sink) return TD_OK;
    if (total > capacity) return td_fail_internal(TD_E_LIMIT, ("the output takes " + std::to_string(total) + " bytes").c_str());

    uint64_t longest = 0;
    const std::vector<vcf::Range> ranges = vcf::plan_ranges(line_off.data(), K, p.range_bytes ? p.range_bytes : (uint64_t)TD_VCF_RANGE_BYTES, &longest);
    for (int b = 0; b < 2; ++b) {
        if (b == 1 && ranges.size() < 2) break;
        TD_HIPCHK(dout[b].alloc(longest));
        TD_HIPCHK(pin[b].alloc(longest));
    }
    // behind the buffers, so that they go first and their work is waited for before a buffer is freed
    tdi::Events<2> began, emitted, copied;
    tdi::Stream s_emit, s_copy;
    TD_HIPCHK(began.create());
    TD_HIPCHK(emitted.create());
    TD_HIPCHK(copied.create());
    TD_HIPCHK(s_emit.create());
    TD_HIPCHK(s_copy.create());
    double emit_ms = 0;
    // the host's side of range r: its bytes have arrived in pin[r & 1]
    auto consume = [&](size_t r) -> int {
        const int b = (int)(r & 1);
        TD_HIPCHK(hipEventSynchronize(copied.e[b]));
        float f = 0;
        if (hipEventElapsedTime(&f, began.e[b], emitted.e[b]) == hipSuccess) emit_ms += f;
        return sink->take(pin[b].p, line_off[ranges[r].last] - line_off[ranges[r].first], line_off[ranges[r].first]);
    };
    for (size_t r = 0; r < ranges.size(); ++r) {
        const int b = (int)(r & 1);
        const uint64_t base = line_off[ranges[r].first], bytes = line_off[ranges[r].last] - base;
        if (r >= 2) TD_HIPCHK(hipStreamWaitEvent(s_emit.s, copied.e[b], 0));      // range r - 2 has left dout[b]
        TD_HIPCHK(hipEventRecord(began.e[b], s_emit.s));
        for (uint64_t lo = ranges[r].first; lo < ranges[r].last; lo += VCF_LAUNCH_LINES) {
            const uint64_t hi = std::min<uint64_t>(lo + VCF_LAUNCH_LINES, ranges[r].last);
            const dim3 grid((uint32_t)((hi - lo + VCF_TILE - 1) / VCF_TILE), chunks);
            if (p.likelihoods)
                hipLaunchKernelGGL(k_vcf_emit<true>, grid, dim3(VCF_THREADS), 0, s_emit.s, (const uint32_t *)in.counts, S, in.T, in.M, di.p,
                                   di.p + in.M, (const uint8_t *)in.calls, dsel.p, K, (uint32_t)lo, (uint32_t)hi, tab, p.ploidy, dprefix.p,
                                   dpoff.p, dline_off.p, start.p, base, dout[b].p, bytes);
            else
                hipLaunchKernelGGL(k_vcf_emit<false>, grid, dim3(VCF_THREADS), 0, s_emit.s, (const uint32_t *)in.counts, S, in.T, in.M, di.p,
                                   di.p + in.M, (const uint8_t *)in.calls, dsel.p, K, (uint32_t)lo, (uint32_t)hi, tab, p.ploidy, dprefix.p,
                                   dpoff.p, dline_off.p, start.p, base, dout[b].p, bytes);
            TD_HIPCHK(hipGetLastError());
        }
        TD_HIPCHK(hipEventRecord(emitted.e[b], s_emit.s));
        TD_HIPCHK(hipStreamWaitEvent(s_copy.s, emitted.e[b], 0));
        TD_HIPCHK(hipMemcpyAsync(pin[b].p, dout[b].p, bytes, hipMemcpyDeviceToHost, s_copy.s));
        TD_HIPCHK(hipEventRecord(copied.e[b], s_copy.s));
        if (r >= 1) {                              // range r - 1 is written while range r is formatted
            rc = consume(r - 1);
            if (rc) return rc;
        }
    }
    rc = consume(ranges.size() - 1);
    if (rc) return rc;
    if (ms) ms[2] = emit_ms;
    if (ranges_out) *ranges_out = ranges.size();
    return TD_OK;
}

}  // namespace

extern "C" int td_vcf_format(td_handle *h, const void *d_counts, uint32_t S, uint32_t T, uint32_t M, const uint32_t *i0, const uint32_t *i1,
                             const void *d_calls, const td_vcf_params *p, const uint32_t *sel, uint32_t K, const uint8_t *prefix,
                             const uint64_t *prefix_off, uint64_t *line_off_out, uint8_t *out, uint64_t capacity, uint64_t *n_out,
                             double *ms) {
    if (n_out) *n_out = 0;
    if (ms) ms[0] = ms[1] = ms[2] = 0;
    if (!n_out) return td_fail_internal(TD_E_ARG, "NULL argument");
    const VcfInput in = {h, d_counts, S, T, M, i0, i1, d_calls, p, sel, K, prefix, prefix_off};
    int rc = vcf_check(in);
    if (rc) return rc;
    MemorySink sink(out);
    return vcf_run(in, line_off_out, out ? &sink : nullptr, capacity, n_out, nullptr, ms);
}

extern "C" int td_vcf_file(td_handle *h, const void *d_counts, uint32_t S, uint32_t T, uint32_t M, const uint32_t *i0, const uint32_t *i1,
                           const void *d_calls, const td_vcf_params *p, const uint32_t *sel, uint32_t K, const uint8_t *prefix,
                           const uint64_t *prefix_off, const char *path, int append, uint64_t *n_out, uint64_t *ranges_out, double *ms) {
    if (n_out) *n_out = 0;
    if (ranges_out) *ranges_out = 0;
    if (ms) ms[0] = ms[1] = ms[2] = ms[3] = 0;
    if (!n_out || !path) return td_fail_internal(TD_E_ARG, "NULL argument");
    const VcfInput in = {h, d_counts, S, T, M, i0, i1, d_calls, p, sel, K, prefix, prefix_off};
    int rc = vcf_check(in);
    if (rc) return rc;
    FileSink sink;
    rc = sink.open_at(path, append);
    if (rc) return rc;
    rc = vcf_run(in, nullptr, &sink, ~0ull, n_out, ranges_out, ms);
    if (rc) return rc;
    if (ms) ms[3] = sink.write_ms;
    return sink.finish();
}
