// Parent pairs by Mendelian trio counts (include/tagdig.h: td_parent_trios).
//
// Input: the S x M uint8 call matrix where it lies in device memory (rows exactly M bytes apart), codes 0 / 1 / 2, any
// byte above 2 = missing; the offspring list and, per offspring row, C candidate slots (sample indices or -1).  For every
// slot pair (a, b) of a row, over the participating markers at which offspring, cand[a] and cand[b] are all called:
// n = their number, e = those at which the offspring's call is not one the two parents can produce.  With one-hot bit
// planes C (called and used), H0, H2 and H1 = C & ~H0 & ~H2 per sample and 64 markers
//     n = popc(Co & Cp & Cq),  e = popc(Cp & Cq & ((o2 & (p0 | q0)) | (o0 & (p2 | q2)) | (o1 & ((p0 & q0) | (p2 & q2))))).
// This is a three-way count, not a Gram product: VALU and LDS work, no matrix cores.
//
// k_par_pack: a wave takes 64 neighbouring markers of one sample; three ballots give the words of C, H0 and H2.  The planes
//    lie as [plane][sample][Wpad] 64-bit words, Wpad = the words of M rounded up to TD_PARENT_WCHUNK; markers past M, masked
//    markers and codes above 2 give zero bits, so nothing behind them needs a bound.
// k_par_trios<TILE>: one offspring row per workgroup along grid y, one block of B x B slot pairs (ba <= bb), B = 16 TILE,
//    along grid x; 256 threads, thread (ty, tx) holds the TILE x TILE pairs of slots TILE ty + i and TILE tx + j of the block
//    in registers.  TILE = 4 (B = TD_PARENT_BLOCK = 64: three blocks) for more than 64 candidates; TILE = 2 (B = 32: one or
//    three blocks) up to 64, where 64-slot blocks would be few and mostly empty.  Per chunk of TD_PARENT_WCHUNK words the
//    planes of the block's 2 B slots are staged in LDS as [plane][word][column]: slot s of a side lies at column
//    (s % TILE) * 16 + s / TILE, so the 16 lanes that differ in tx read 16 neighbouring 64-bit words; a row is 2 B + 1 words
//    long, so the 16 lanes that stage the 16 words of one slot write 16 different banks.  The offspring's words are staged
//    once per chunk and read by every lane at one address (a broadcast).  Per word a thread forms the terms of its TILE
//    a-slots and TILE b-slots once and spends 9 64-bit operations a pair.  TILE = 2 has registers to spare and few
//    workgroups to hide a load behind: it fetches the next chunk from global memory before it counts the current one.
//    32-bit accumulators (M < 2^31); every (n, e) is written exactly once, by the thread that owns it: no atomics, no marker
//    chunking across workgroups.  Thread tiles wholly below the diagonal of a diagonal block only help staging.
// k_par_rank: one workgroup per offspring row selects the first K trios with n >= min_shared by (e / n ascending by
//    cross-multiplication, n descending, t ascending): K rounds, in each every thread finds its best trio behind the last
//    winner and a workgroup-wide best follows.  The comparison is the tuple rule on 64-bit products.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "td_internal.hpp"

namespace {

constexpr uint32_t PA_THREADS = 256;               // 4 waves; 16 x 16 thread tiles of TILE x TILE slot pairs
constexpr uint32_t PA_SIDE = 16;                   // thread tiles along a block's edge
constexpr uint32_t PA_BIG = TD_PARENT_BLOCK / PA_SIDE;             // TILE of the 64-slot block (C > 64); half of it below
constexpr uint32_t PA_STAGE_SLOTS = PA_THREADS / TD_PARENT_WCHUNK; // slots staged by one pass of the workgroup
constexpr uint32_t PA_NONE = 0xFFFFFFFFu;
static_assert(PA_SIDE * PA_SIDE == PA_THREADS && PA_BIG == 4, "one thread per 4 x 4 tile of a 64-slot block");
static_assert((TD_PARENT_WCHUNK & (TD_PARENT_WCHUNK - 1)) == 0 && TD_PARENT_WCHUNK >= 4 && TD_PARENT_WCHUNK <= 64,
              "k_par_pack writes four words a workgroup; the staging gives a word to each of WCHUNK lanes");
static_assert(3 * TD_PARENT_WCHUNK <= PA_THREADS, "one thread stages one word of the offspring");
static_assert(3 * TD_PARENT_WCHUNK * (2 * TD_PARENT_BLOCK + 2) * 8 <= 64 * 1024, "the chunk fits static LDS");
static_assert(TD_PARENT_MAX_CAND % TD_PARENT_BLOCK == 0, "whole blocks");

// pack, trio and rank kernel (device ms) of the calling thread's last td_parent_trios
thread_local double g_pa_times[3] = {0, 0, 0};

__global__ __launch_bounds__(PA_THREADS) void k_par_pack(const uint8_t *calls, uint32_t S, uint32_t M, const uint8_t *use, uint32_t Wpad,
                                                         uint64_t *planes) {
    const uint32_t s = blockIdx.y, w = blockIdx.x * (PA_THREADS / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= Wpad) return;                         // (uniform over the wave)
    const uint64_t m = (uint64_t)w * 64u + lane;
    uint32_t g = 3;
    if (m < M && (!use || use[m])) g = calls[(size_t)s * M + m];   // s < S, m < M
    const uint64_t c = __ballot(g <= 2u), h0 = __ballot(g == 0u), h2 = __ballot(g == 2u);
    if (lane < 3u) planes[((size_t)lane * S + s) * Wpad + w] = lane == 0u ? c : lane == 1u ? h0 : h2;
}

template <uint32_t PA_TILE>
__global__ __launch_bounds__(PA_THREADS) void k_par_trios(const uint64_t *planes, uint32_t S, uint32_t Wpad, const uint32_t *offspring,
                                                          const int32_t *cand, uint32_t C, uint32_t selfing, uint32_t T, uint32_t *table) {
    constexpr uint32_t PA_BLOCK = PA_SIDE * PA_TILE;               // candidate slots along the block's edge
    constexpr uint32_t PA_ROW = 2 * PA_BLOCK + 1;                  // words of an LDS row: the a side, the b side, one of padding
    constexpr uint32_t PA_STAGE_PASSES = 2 * PA_BLOCK / PA_STAGE_SLOTS;
    constexpr bool PA_PREFETCH = PA_TILE < PA_BIG;                 // few workgroups, few registers: the next chunk is fetched ahead
    __shared__ uint64_t sp[3][TD_PARENT_WCHUNK][PA_ROW];
    __shared__ uint64_t so[3][TD_PARENT_WCHUNK];
    const uint32_t row = blockIdx.y, tid = threadIdx.x;
    // the block (ba, bb), ba <= bb, numbered row-major over the upper triangle
    const uint32_t nb = (C + PA_BLOCK - 1) / PA_BLOCK;
    uint32_t ba = 0, bb = blockIdx.x;
    while (bb >= nb - ba) {
        bb -= nb - ba;
        ++ba;
    }
    bb += ba;
    const size_t plane = (size_t)S * Wpad;
    const uint64_t *own = planes + (size_t)offspring[row] * Wpad;  // offspring[row] < S (checked on the host)
    // staging: lane w of 16 takes word w of a slot, so a slot's chunk is one run of 128 bytes per plane
    const uint32_t sw = tid % TD_PARENT_WCHUNK, s0 = tid / TD_PARENT_WCHUNK;
    int32_t smp[PA_STAGE_PASSES];
    uint32_t col[PA_STAGE_PASSES];
#pragma unroll
    for (uint32_t k = 0; k < PA_STAGE_PASSES; ++k) {
        const uint32_t slot = s0 + PA_STAGE_SLOTS * k, side = slot / PA_BLOCK, sl = slot % PA_BLOCK;
        const uint32_t gs = (side ? bb : ba) * PA_BLOCK + sl;
        smp[k] = gs < C ? cand[(size_t)row * C + gs] : -1;         // -1 .. S - 1 (checked on the host)
        col[k] = side * PA_BLOCK + (sl % PA_TILE) * PA_SIDE + sl / PA_TILE;
    }
    const uint32_t tx = tid % PA_SIDE, ty = tid / PA_SIDE;
    const bool idle = ba == bb && ty > tx;         // a thread tile wholly below the diagonal
    uint32_t n[PA_TILE][PA_TILE], e[PA_TILE][PA_TILE];
#pragma unroll
    for (uint32_t i = 0; i < PA_TILE; ++i)
#pragma unroll
        for (uint32_t j = 0; j < PA_TILE; ++j) n[i][j] = e[i][j] = 0;
    // a chunk's words of this thread's slots and of the offspring, from global memory into registers
    uint64_t rc[PA_STAGE_PASSES], r0[PA_STAGE_PASSES], r2[PA_STAGE_PASSES], ro = 0;
    auto fetch = [&](uint32_t w0) {
#pragma unroll
        for (uint32_t k = 0; k < PA_STAGE_PASSES; ++k) {
            rc[k] = r0[k] = r2[k] = 0;
            if (smp[k] >= 0) {
                const uint64_t *src = planes + (size_t)(uint32_t)smp[k] * Wpad + w0 + sw;      // w0 + sw < Wpad
                rc[k] = src[0];
                r0[k] = src[plane];
                r2[k] = src[2 * plane];
            }
        }
        if (tid < 3u * TD_PARENT_WCHUNK) ro = own[(size_t)(tid / TD_PARENT_WCHUNK) * plane + w0 + sw];
    };
    if (PA_PREFETCH) fetch(0);                     // Wpad >= one chunk
    for (uint32_t w0 = 0; w0 < Wpad; w0 += TD_PARENT_WCHUNK) {     // Wpad is a multiple of the chunk
        if (!PA_PREFETCH) fetch(w0);
        __syncthreads();                           // the last chunk has been read
#pragma unroll
        for (uint32_t k = 0; k < PA_STAGE_PASSES; ++k) {
            sp[0][sw][col[k]] = rc[k];
            sp[1][sw][col[k]] = r0[k];
            sp[2][sw][col[k]] = r2[k];
        }
        if (tid < 3u * TD_PARENT_WCHUNK) so[tid / TD_PARENT_WCHUNK][sw] = ro;
        __syncthreads();
        if (PA_PREFETCH && w0 + TD_PARENT_WCHUNK < Wpad) fetch(w0 + TD_PARENT_WCHUNK);     // in flight while this chunk is counted
        if (idle) continue;
#pragma unroll 2
        for (uint32_t w = 0; w < TD_PARENT_WCHUNK; ++w) {
            const uint64_t oc = so[0][w], o0 = so[1][w], o2 = so[2][w], o1 = oc & ~o0 & ~o2;
            uint64_t ac[PA_TILE], ax[PA_TILE], a0[PA_TILE], a2[PA_TILE];
#pragma unroll
            for (uint32_t i = 0; i < PA_TILE; ++i) {
                const uint32_t ca = i * PA_SIDE + ty;
                const uint64_t p0 = sp[1][w][ca], p2 = sp[2][w][ca];
                ac[i] = sp[0][w][ca] & oc;         // called in the offspring and this parent
                ax[i] = (o2 & p0) | (o0 & p2);     // this parent alone rules the offspring's call out
                a0[i] = o1 & p0;
                a2[i] = o1 & p2;
            }
#pragma unroll
            for (uint32_t j = 0; j < PA_TILE; ++j) {
                const uint32_t cb = PA_BLOCK + j * PA_SIDE + tx;
                const uint64_t cq = sp[0][w][cb], q0 = sp[1][w][cb], q2 = sp[2][w][cb];
                const uint64_t bx = (o2 & q0) | (o0 & q2);
#pragma unroll
                for (uint32_t i = 0; i < PA_TILE; ++i) {
                    const uint64_t all = ac[i] & cq;
                    n[i][j] += (uint32_t)__popcll(all);
                    e[i][j] += (uint32_t)__popcll(all & (ax[i] | bx | (a0[i] & q0) | (a2[i] & q2)));
                }
            }
        }
    }
    if (idle) return;
#pragma unroll
    for (uint32_t i = 0; i < PA_TILE; ++i) {
#pragma unroll
        for (uint32_t j = 0; j < PA_TILE; ++j) {
            const uint32_t a = ba * PA_BLOCK + ty * PA_TILE + i, b = bb * PA_BLOCK + tx * PA_TILE + j;
            if (a >= C || b >= C || (selfing ? a > b : a >= b)) continue;
            const uint32_t t = selfing ? a * C - a * (a - 1u) / 2u + (b - a) : a * (C - 1u) - a * (a - 1u) / 2u + (b - a - 1u);
            *reinterpret_cast<uint2 *>(table + ((size_t)row * T + t) * 2u) = make_uint2(n[i][j], e[i][j]);    // t < T
        }
    }
}

struct PaKey {
    uint32_t n, e, t;                              // t == PA_NONE: no trio
};

// x comes before y: smaller e / n by cross-multiplication (n, e < 2^31: 64-bit products), then larger n, then lower t
__device__ __forceinline__ bool pa_before(const PaKey &x, const PaKey &y) {
    if (x.t == PA_NONE) return false;
    if (y.t == PA_NONE) return true;
    const uint64_t l = (uint64_t)x.e * y.n, r = (uint64_t)y.e * x.n;
    if (l != r) return l < r;
    if (x.n != y.n) return x.n > y.n;
    return x.t < y.t;
}

__global__ __launch_bounds__(PA_THREADS) void k_par_rank(const uint32_t *table, const int32_t *cand, uint32_t C, uint32_t selfing, uint32_t T,
                                                         uint32_t K, uint32_t min_shared, td_parent_trio *best_out) {
    __shared__ PaKey part[PA_THREADS / 64];
    const uint32_t row = blockIdx.x, tid = threadIdx.x;
    const uint32_t *tab = table + (size_t)row * T * 2u;
    PaKey prev = {0, 0, PA_NONE};
    for (uint32_t r = 0; r < K; ++r) {
        PaKey best = {0, 0, PA_NONE};
        if (r == 0 || prev.t != PA_NONE) {
            for (uint32_t t = tid; t < T; t += PA_THREADS) {
                const uint2 ne = *reinterpret_cast<const uint2 *>(tab + (size_t)t * 2u);
                if (ne.x < min_shared) continue;   // min_shared >= 1: a ranked trio has n > 0
                const PaKey cur = {ne.x, ne.y, t};
                if (r > 0 && !pa_before(prev, cur)) continue;      // it has been selected
                if (pa_before(cur, best)) best = cur;
            }
        }
#pragma unroll
        for (uint32_t x = 32; x > 0; x >>= 1) {
            const PaKey o = {(uint32_t)__shfl_xor((int)best.n, (int)x), (uint32_t)__shfl_xor((int)best.e, (int)x),
                             (uint32_t)__shfl_xor((int)best.t, (int)x)};
            if (pa_before(o, best)) best = o;
        }
        __syncthreads();                           // the last round's parts have been read
        if ((tid & 63u) == 0) part[tid >> 6] = best;
        __syncthreads();
        best = part[0];
#pragma unroll
        for (uint32_t v = 1; v < PA_THREADS / 64; ++v)
            if (pa_before(part[v], best)) best = part[v];
        if (tid == 0) {
            td_parent_trio rec = {PA_NONE, PA_NONE, 0, 0};
            if (best.t != PA_NONE) {
                uint32_t a = 0, rem = best.t, len = selfing ? C : C - 1u;      // t -> (a, b): rows of C, C - 1, ... (or one less)
                while (rem >= len) {
                    rem -= len;
                    --len;
                    ++a;
                }
                const uint32_t b = selfing ? a + rem : a + 1u + rem;
                rec.p = (uint32_t)cand[(size_t)row * C + a];       // n > 0: neither slot is empty
                rec.q = (uint32_t)cand[(size_t)row * C + b];
                rec.n = best.n;
                rec.e = best.e;
            }
            best_out[(size_t)row * K + r] = rec;
        }
        prev = best;                               // (uniform over the workgroup)
    }
}

}  // namespace

extern "C" int td_parent_last_times(td_handle *h, double *out3) {
    if (!h || !out3) return td_fail_internal(TD_E_ARG, "NULL argument");
    for (int k = 0; k < 3; ++k) out3[k] = g_pa_times[k];
    return TD_OK;
}

extern "C" int td_parent_trios(td_handle *h, const void *d_calls, uint32_t S, uint32_t M, const uint8_t *use, const uint32_t *offspring, uint32_t O,
                               const int32_t *cand, uint32_t C, uint32_t flags, uint32_t K, uint32_t min_shared, td_parent_trio *best_out,
                               uint32_t *table_out, double *ms) {
    if (ms) *ms = 0;
    g_pa_times[0] = g_pa_times[1] = g_pa_times[2] = 0;
    if (!h) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (S > TD_PARENT_MAX_SAMPLES) return td_fail_internal(TD_E_ARG, "more samples than TD_PARENT_MAX_SAMPLES");
    if (M >= 0x80000000u) return td_fail_internal(TD_E_ARG, "markers must number below 2^31");
    if (C < 1 || C > TD_PARENT_MAX_CAND) return td_fail_internal(TD_E_ARG, "C must be 1..128");
    if (K < 1 || K > TD_PARENT_MAX_TOP) return td_fail_internal(TD_E_ARG, "K must be 1..8");
    if (min_shared < 1) return td_fail_internal(TD_E_ARG, "min_shared must be at least 1");
    if (flags & ~(uint32_t)TD_PARENT_SELFING) return td_fail_internal(TD_E_ARG, "unknown flag bits");
    if (S && M && !d_calls) return td_fail_internal(TD_E_ARG, "NULL call matrix");
    if (O && (!offspring || !cand)) return td_fail_internal(TD_E_ARG, "NULL offspring or candidate list");
    if (O && !best_out) return td_fail_internal(TD_E_ARG, "NULL best_out");
    const uint32_t selfing = flags & TD_PARENT_SELFING;
    const uint32_t T = selfing ? C * (C + 1u) / 2u : C * (C - 1u) / 2u;
    {                                              // a row names samples below S, not its own offspring, none twice
        std::vector<uint32_t> seen(S, 0);          // seen[p] = i + 1: row i has named p
        for (uint32_t i = 0; i < O; ++i) {
            if (offspring[i] >= S) {
                td_set_bad_index(i);
                return td_fail_internal(TD_E_ARG, ("offspring row " + std::to_string(i) + ": sample " + std::to_string(offspring[i]) +
                                                   " is outside 0 .. S - 1").c_str());
            }
            for (uint32_t a = 0; a < C; ++a) {
                const int32_t p = cand[(size_t)i * C + a];
                if (p == -1) continue;
                const char *what = p < 0 || (uint32_t)p >= S ? " is outside -1 .. S - 1" : (uint32_t)p == offspring[i] ? " is the offspring itself" :
                                   seen[p] == i + 1 ? " appears twice" : nullptr;
                if (what) {
                    td_set_bad_index(i);
                    return td_fail_internal(TD_E_ARG, ("candidates of row " + std::to_string(i) + ": entry " + std::to_string(p) + what).c_str());
                }
                seen[p] = i + 1;
            }
        }
    }
    if (O == 0) return TD_OK;
    const size_t nrec = (size_t)O * K, ncell = (size_t)O * T * 2u;
    if (S == 0 || M == 0) {                        // (S == 0 cannot get here: no offspring index is below it)
        for (size_t k = 0; k < nrec; ++k) best_out[k] = td_parent_trio{PA_NONE, PA_NONE, 0, 0};
        if (table_out && ncell) memset(table_out, 0, ncell * sizeof(uint32_t));
        return TD_OK;
    }
    int rc = td_handle_wait_work(h);
    if (rc) return rc;
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    const uint32_t W = (M + 63u) / 64u, Wpad = (W + TD_PARENT_WCHUNK - 1u) / TD_PARENT_WCHUNK * TD_PARENT_WCHUNK;
    const bool big = C > TD_PARENT_BLOCK;           // blocks of 64 slots; of 32 up to 64 candidates: more workgroups, fewer idle pairs
    const uint32_t block = big ? TD_PARENT_BLOCK : TD_PARENT_BLOCK / 2u, nb = (C + block - 1u) / block;
    tdi::Events<4> ev;
    TD_HIPCHK(ev.create());
    tdi::DevBuf<uint64_t> d_planes;
    tdi::DevBuf<uint8_t> d_use;
    tdi::DevBuf<uint32_t> d_off, d_table;
    tdi::DevBuf<int32_t> d_cand;
    tdi::DevBuf<td_parent_trio> d_best;
    TD_HIPCHK(d_planes.alloc((size_t)3 * S * Wpad));
    TD_HIPCHK(d_off.alloc(O));
    TD_HIPCHK(d_cand.alloc((size_t)O * C));
    TD_HIPCHK(d_table.alloc(ncell));
    TD_HIPCHK(d_best.alloc(nrec));
    if (use) {
        TD_HIPCHK(d_use.alloc(M));
        TD_HIPCHK(hipMemcpy(d_use.p, use, M, hipMemcpyHostToDevice));
    }
    TD_HIPCHK(hipMemcpy(d_off.p, offspring, (size_t)O * sizeof(uint32_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(d_cand.p, cand, (size_t)O * C * sizeof(int32_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    hipLaunchKernelGGL(k_par_pack, dim3(Wpad / (PA_THREADS / 64u), S), dim3(PA_THREADS), 0, 0, (const uint8_t *)d_calls, S, M,
                       (const uint8_t *)d_use.p, Wpad, d_planes.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    for (uint32_t lo = 0; lo < O; lo += 65535u) {  // offspring rows along grid y
        const uint32_t rows = std::min(O - lo, 65535u);
        hipLaunchKernelGGL(big ? k_par_trios<PA_BIG> : k_par_trios<PA_BIG / 2u>, dim3(nb * (nb + 1u) / 2u, rows), dim3(PA_THREADS), 0, 0,
                           d_planes.p, S, Wpad, d_off.p + lo, d_cand.p + (size_t)lo * C, C, selfing, T, d_table.p + (size_t)lo * T * 2u);
        TD_HIPCHK(hipGetLastError());
    }
    TD_HIPCHK(hipEventRecord(ev.e[2], 0));
    for (uint32_t lo = 0; lo < O; lo += 65535u) {
        hipLaunchKernelGGL(k_par_rank, dim3(std::min(O - lo, 65535u)), dim3(PA_THREADS), 0, 0, d_table.p + (size_t)lo * T * 2u,
                           d_cand.p + (size_t)lo * C, C, selfing, T, K, min_shared, d_best.p + (size_t)lo * K);
        TD_HIPCHK(hipGetLastError());
    }
    TD_HIPCHK(hipEventRecord(ev.e[3], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[3]));
    double total = 0;
    for (int k = 0; k < 3; ++k) {
        float f = 0;
        TD_HIPCHK(hipEventElapsedTime(&f, ev.e[k], ev.e[k + 1]));
        g_pa_times[k] = f;
        total += f;
    }
    if (ms) *ms = total;
    TD_HIPCHK(hipMemcpy(best_out, d_best.p, nrec * sizeof(td_parent_trio), hipMemcpyDeviceToHost));
    if (table_out && ncell) TD_HIPCHK(hipMemcpy(table_out, d_table.p, ncell * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return TD_OK;
}
