// Tag census: the distinct sequences that follow barcode + cut site in one library, and how often each
// occurs.  Per read the rule is the counter's up to the barcode (reference tagdigger_fun.py:250-259: lines as text mode
// splits them, line k a read when k % 4 == 1, line.strip().upper(), sequence_index_lookup on barcode + cut site);
// then, instead of a tag lookup, the window line1[len(barcode) : len(barcode) + L] -- from the cut site's first base
// on -- is packed at 2 bits a base and counted in an open-addressing table in device memory.
//
//   k_census          one workgroup per 16 KiB tile (the handle's k_count_lines + k_scan_tiles give every tile its line
//                     index): terminator masks -> the tile's read-line starts as a dense list in LDS -> one lane per
//                     read: barcode_lookup (kernels.hpp, the index td_set_index's rules build), window -> key ->
//                     equal keys of a wave combined in LDS -> census_add
//   k_census_compact  the slots with count >= min_count -> dense arrays (the host orders them)
//
// The table.  Slots of {key, cc} (L <= 32: 16 bytes) or {key hi, key lo, cc, -} (32 bytes), linear probing from a hash
// of the key.  cc is ONE 64-bit word: state in bits 62-63 (0 empty, 1 claimed, 2 ready), the count below.  A lane
// claims an empty slot with a compare-and-swap 0 -> claimed, stores the key, and publishes ready | count with a
// release store; nobody reads a slot's key before an acquire load of cc has shown it ready, so a key is never seen
// half-written; from then on the count only takes atomic adds, so counts are exact under any interleaving.
// A lane that meets a claimed slot comes round again.  It never waits INSIDE an iteration: the probe loop runs until
// every lane of the wave is through (one wave-wide vote per iteration), and a claimer publishes in the iteration it
// claims in -- so a lane of the claimer's own wave, in lockstep with it, finds the slot ready one iteration later.
// Every loop is bounded: CENSUS_SPIN_LIMIT rounds at a claimed slot (ERR_SPIN -> TD_E_INTERNAL) and one lap of the
// table (ERR_FULL); both set the abort word, which ends every other loop at its next look.  The table takes at most
// 3/4 of its slots in distinct keys: the claim that exceeds it raises ERR_FULL -> TD_E_LIMIT.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#define TD_INST_ONLY                    // (k_scan_tiles is defined in tagdig.hip's translation unit)
#include "stream_pass.hpp"

namespace tdc {
using namespace tdk;

constexpr int CPT = 4;                                   // 16-byte chunks per thread: tiles of 16 KiB, as k_count_lines<4> counts them
constexpr uint32_t TILE = CPT * BLOCK * 16u;
static_assert(TILE == tdi::STREAM_TILE, "td_line_prefix (tagdig.hip) counts terminators per 16 KiB tile with k_count_lines<4>");
constexpr uint32_t LIST_CAP = TILE / 4 + 4;              // read-line starts per tile: every fourth terminator, the buffer's own first line
constexpr uint32_t CENSUS_SPIN_LIMIT = 1u << 20;
constexpr unsigned long long CC_CLAIMED = 1ull << 62, CC_READY = 2ull << 62, CC_COUNT = (1ull << 62) - 1;
constexpr unsigned long long ERR_FULL = 8;               // beside kernels.hpp's ERR_NONASCII, ERR_SPIN
// the census' words in device memory
enum { CS_READS = 0, CS_BARCUT = 1, CS_SHORT = 2, CS_AMBIG = 3, CS_DISTINCT = 4, CS_ERR = 5, CS_ABORT = 6, CS_TOTAL = 7, CS_NWORDS = 8 };

struct CensusParams {
    const uint8_t *buf;
    uint64_t nbytes;
    uint64_t first_line;       // global index of the buffer's first line (+ *cursor_in)
    uint64_t limit_line;       // last read line that is looked at (maxreads)
    const uint64_t *prefix;    // [ntiles] FLAG_INC | terminators up to the end of tile t
    uint32_t ntiles;
    const uint32_t *bblob;     // barcode + cut site index (the counting path's layout; bmeta's offset field = len(barcode))
    uint32_t bblob_bytes, off_bmeta, off_bdir;
    uint32_t taglen;           // L, 1..64
    unsigned long long *table; // slots of 2 (L <= 32) or 4 words
    uint64_t slot_mask;        // slots - 1 (a power of two)
    uint64_t max_keys;         // distinct keys the table takes
    unsigned long long *cs;    // CS_*
    const unsigned long long *cursor_in;
    unsigned long long *cursor_out;
    uint32_t combine;          // 1: equal keys of a wave are combined in LDS before they go to the table
};

__device__ __forceinline__ unsigned long long ld_relaxed(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t mix64(uint64_t hi, uint64_t lo) {
    uint64_t x = hi ^ (lo * 0x9E3779B97F4A7C15ull) ^ (lo >> 29);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

// n more of key (hi, lo) for every lane with `active`; called by whole waves (the loop ends on a wave-wide vote).
__device__ __forceinline__ void census_add(const CensusParams &p, bool active, uint64_t hi, uint64_t lo, uint64_t hash, unsigned long long n) {
    const bool two = p.taglen > 32;
    const uint32_t cc_at = two ? 2u : 1u;
    uint64_t i = hash & p.slot_mask, steps = 0;
    uint32_t spins = 0;
    bool done = !active;
    for (;;) {
        if (!done) {
            unsigned long long *s = p.table + (i << (two ? 2 : 1));
            unsigned long long c = __hip_atomic_load(s + cc_at, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            bool mine = false;
            if (c == 0) {
                mine = __hip_atomic_compare_exchange_strong(s + cc_at, &c, CC_CLAIMED, __ATOMIC_ACQUIRE, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (mine) {
                // the slot is this lane's alone until it publishes: key first, then ready | count
                __hip_atomic_store(s, (unsigned long long)hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (two) __hip_atomic_store(s + 1, (unsigned long long)lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(s + cc_at, CC_READY | n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long d = atomicAdd(p.cs + CS_DISTINCT, 1ull);
                if (d >= p.max_keys) { atomicOr(p.cs + CS_ERR, ERR_FULL); __hip_atomic_store(p.cs + CS_ABORT, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                done = true;
            } else if ((c >> 62) == 1) {
                // claimed by another lane, which publishes without waiting for anybody: look again in the next iteration
                if (++spins > CENSUS_SPIN_LIMIT || ld_relaxed(p.cs + CS_ABORT)) {
                    if (spins > CENSUS_SPIN_LIMIT) atomicOr(p.cs + CS_ERR, ERR_SPIN);
                    __hip_atomic_store(p.cs + CS_ABORT, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    done = true;
                }
            } else {
                const unsigned long long khi = ld_relaxed(s), klo = two ? ld_relaxed(s + 1) : 0ull;
                if (khi == hi && klo == lo) {
                    __hip_atomic_fetch_add(s + cc_at, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    done = true;
                } else {
                    i = (i + 1) & p.slot_mask;
                    spins = 0;
                    if (++steps > p.slot_mask) {      // one lap and no room
                        atomicOr(p.cs + CS_ERR, ERR_FULL);
                        __hip_atomic_store(p.cs + CS_ABORT, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        done = true;
                    }
                }
            }
        }
        if (__all(done)) break;
    }
}

// One read line starting at gpos -> 0: no barcode + cut site; 1: short; 2: ambiguous; 3: counted, key in (hi, lo).
__device__ __forceinline__ uint32_t census_line(const CensusParams &p, const KParams &kp, const TileCtx &cx, uint64_t gpos, uint64_t &hi, uint64_t &lo) {
    constexpr int W = 2;                       // fetch_stream<2>: seven chunks from the read's first chunk = 97 bases at least
    uint32_t S[2 * W + 4];
    uint32_t nvalid = 0;
    (void)fetch_stream<W, ML_SLOW>(kp, cx, gpos, 0u, true, S, nvalid);      // (strips the leading blanks, :256)
    const uint64_t K = ((uint64_t)S[0] << 32) | S[1];
    uint32_t meta = 0;
    if (!barcode_lookup(cx.L_bval, cx.L_bmeta, cx.L_bdir, K, nvalid, meta)) return 0u;
    const uint32_t off = (meta >> 6) & 63u, L = p.taglen;       // len(barcode) <= 32
    if (nvalid < off + L) {
        // the window holds something that is no base, or the line ends inside it: len(line.strip()) decides
        uint64_t s = gpos;
        while (s < p.nbytes && is_blank(p.buf[s])) s++;
        uint64_t e = s;
        while (e < p.nbytes && p.buf[e] != 0x0Au && p.buf[e] != 0x0Du) e++;
        while (e > s && is_blank(p.buf[e - 1])) e--;
        return e - s < (uint64_t)(off + L) ? 1u : 2u;
    }
    const uint32_t wo = off >> 4, sh = 2u * (off & 15u);
    for (uint32_t t = 0; t < 2u; t++) {
        if (wo > t) {
#pragma unroll
            for (int w = 0; w < 2 * W + 3; w++) S[w] = S[w + 1];
            S[2 * W + 3] = 0;
        }
    }
    uint32_t k32[4];
#pragma unroll
    for (int j = 0; j < 4; j++) k32[j] = (uint32_t)(((((uint64_t)S[j] << 32) | S[j + 1]) << sh) >> 32);
    hi = ((uint64_t)k32[0] << 32) | k32[1];
    lo = ((uint64_t)k32[2] << 32) | k32[3];
    if (L < 32) hi &= ~0ull << (64u - 2u * L);
    if (L <= 32) lo = 0;
    else if (L < 64) lo &= ~0ull << (128u - 2u * L);
    return 3u;
}

__global__ __launch_bounds__(BLOCK) void k_census(const CensusParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint16_t L_mask[CPT * BLOCK];
    __shared__ uint16_t L_list[LIST_CAP];
    __shared__ uint32_t L_misc[16];
    __shared__ uint8_t L_win[BLOCK / 64][128];
    __shared__ uint32_t L_cnt[BLOCK / 64][64];
    const unsigned long long *L_bval = reinterpret_cast<const unsigned long long *>(lds);
    const uint32_t *L_bmeta = reinterpret_cast<const uint32_t *>(lds + p.off_bmeta);
    const uint16_t *L_bdir = reinterpret_cast<const uint16_t *>(lds + p.off_bdir);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = tid; i < p.bblob_bytes / 4; i += BLOCK) reinterpret_cast<uint32_t *>(lds)[i] = p.bblob[i];
    KParams kp{};
    kp.buf = p.buf; kp.nbytes = p.nbytes; kp.nch = 7;
    TileCtx cx{};
    cx.L_bval = L_bval; cx.L_bmeta = L_bmeta; cx.L_bdir = L_bdir;
    const unsigned long long cin = p.cursor_in ? *p.cursor_in : 0ull;
    const uint64_t fl = p.first_line + cin;
    if (blockIdx.x == 0 && tid == 0 && p.cursor_out) *p.cursor_out = cin + p.cs[CS_TOTAL];
    unsigned long long st_reads = 0, st_bar = 0, st_short = 0, st_ambig = 0;

    for (uint32_t t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const uint64_t tbase = (uint64_t)t * TILE;
        __syncthreads();
        if (tid == 0) { L_misc[8] = (uint32_t)ld_relaxed(p.cs + CS_ABORT); L_misc[9] = 0; }
        uint32_t hiacc = 0;
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            const uint32_t c = j * BLOCK + tid;
            const uint64_t g = tbase + (uint64_t)c * 16u;
            const uint4 v = load_chunk(kp, g);
            hiacc |= v.x | v.y | v.z | v.w;
            uint32_t nl = eq_mask16(v, 0x0A0A0A0Au), cr = eq_mask16(v, 0x0D0D0D0Du);
            uint32_t term = nl | (cr & ~(nl >> 1));
            if (cr & 0x8000u) { const uint64_t nx = g + 16; if (nx < p.nbytes && p.buf[nx] == 0x0A) term &= 0x7FFFu; }
            if (g + 16 > p.nbytes) term &= g < p.nbytes ? ((1u << (uint32_t)(p.nbytes - g)) - 1u) : 0u;
            L_mask[c] = (uint16_t)term;
        }
        __syncthreads();
        if (L_misc[8]) break;                            // (the abort word: every thread of the workgroup read the same value)
        if (hiacc & 0x80808080u) L_misc[9] = 1;
        uint32_t mm[CPT / 2];
        uint32_t cnt = 0;
#pragma unroll
        for (int i = 0; i < CPT / 2; i++) {
            mm[i] = reinterpret_cast<const uint32_t *>(L_mask)[tid * (CPT / 2) + i];
            cnt += __builtin_popcount(mm[i]);
        }
        const uint32_t incl = wave_incl_scan(cnt, lane);
        if (lane == 63) L_misc[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0, tile_terms = 0;
        for (int w = 0; w < BLOCK / 64; w++) { if (w < wave) wbase += L_misc[w]; tile_terms += L_misc[w]; }
        const bool tile_has_hi = L_misc[9] != 0;
        // terminators before this tile: the previous tile's inclusive prefix.  The line behind the buffer's j-th
        // terminator has index fl + j; this tile holds terminators P + 1 .. P + tile_terms
        const uint64_t P = t ? (p.prefix[t - 1] & ~FLAG_INC) : 0ull;
        const uint64_t j0 = P + 1 + ((1 - (fl + P + 1)) & 3);                        // the first of them that a read line follows
        const uint32_t nlist = P + tile_terms >= j0 ? (uint32_t)((P + tile_terms - j0) >> 2) + 1u : 0u;
        const bool own_first = t == 0 && (fl & 3) == 1;                             // the buffer's own first line is a read
        uint64_t ord = P + wbase + incl - cnt;                                       // terminators before this thread's span
        const uint64_t ord0 = ord;
        const uint32_t span0 = tid * CPT * 16u;
#pragma unroll
        for (int k = 0; k < CPT / 2; k++) {
            uint32_t m = mm[k];
            while (m) {
                const uint32_t bit = __builtin_ctz(m);
                m &= m - 1;
                ord++;
                if (((fl + ord) & 3) == 1) {
                    const uint32_t pos = span0 + 32u * k + bit + 1u;                 // (<= TILE: the line may start the next tile)
                    L_list[(ord - j0) >> 2] = tbase + pos < p.nbytes ? (uint16_t)pos : (uint16_t)0xFFFFu;
                }
            }
        }
        if (own_first && tid == 0) L_list[nlist] = 0;
        __syncthreads();

        // ---------------- one lane per read line
        const uint32_t ntot = nlist + (own_first ? 1u : 0u);
        for (uint32_t base = 0; base < ntot; base += BLOCK) {
            if (base + (uint32_t)wave * 64u >= ntot) break;                          // (nothing for this wave: wave-uniform)
            const uint32_t i = base + tid;
            uint32_t kind = 0;
            uint64_t hi = 0, lo = 0;
            if (i < ntot) {
                const uint32_t pos = L_list[i];
                const uint64_t line = i < nlist ? fl + j0 + 4ull * i : fl;
                if (pos != 0xFFFFu && line <= p.limit_line) {
                    st_reads++;
                    kind = census_line(p, kp, cx, tbase + pos, hi, lo);
                    if (kind) st_bar++;
                    if (kind == 1) st_short++;
                    if (kind == 2) st_ambig++;
                }
            }
            bool pend = kind == 3;
            if (!__any(pend)) continue;
            const uint64_t hash = mix64(hi, lo);
            unsigned long long n = 1;
            if (p.combine) {
                // equal keys of this wave: two rounds of "write your lane under the key's hash, read who stayed": a lane
                // whose key is the winner's adds itself to the winner's count in LDS and is through; the winner goes to the
                // table for all of them.  A lane that lost to another key tries once more under other bits of the hash, then
                // goes alone.
                L_cnt[wave][lane] = 0;
                bool undecided = pend;
                for (uint32_t r = 0; r < 2u; r++) {
                    L_win[wave][lane] = 0xFF; L_win[wave][lane + 64] = 0xFF;
                    wave_lds_fence();
                    const uint32_t b = (uint32_t)(hash >> (40u + 7u * r)) & 127u;
                    if (undecided) L_win[wave][b] = (uint8_t)lane;
                    wave_lds_fence();
                    const uint32_t w = undecided ? L_win[wave][b] : (uint32_t)lane;
                    const uint64_t whi = __shfl(hi, (int)w, 64), wlo = __shfl(lo, (int)w, 64);
                    if (undecided) {
                        if (w == (uint32_t)lane) undecided = false;                  // the winner: goes to the table
                        else if (whi == hi && wlo == lo) { atomicAdd(&L_cnt[wave][w], 1u); undecided = false; pend = false; }
                    }
                }
                wave_lds_fence();
                n += L_cnt[wave][lane];
            }
            census_add(p, pend, hi, lo, hash, n);
        }

        // ---------------- rare: bytes >= 0x80 in the tile -- are any inside a read line that is looked at?  (k_count's rule)
        if (tile_has_hi) {
            const uint64_t Lb = fl + ord0;               // index of the line this thread's span starts in
            uint32_t seen = 0;
#pragma unroll
            for (int k = 0; k < CPT / 2; k++) {
                const uint32_t m = mm[k];
#pragma nounroll
                for (uint32_t q = 0; q < 32u; q++) {
                    const uint64_t g = tbase + span0 + 32u * k + q;
                    if (g < p.nbytes && p.buf[g] >= 0x80u) {
                        const uint64_t line = Lb + seen;
                        if ((line & 3) == 1 && line <= p.limit_line) atomicOr(p.cs + CS_ERR, ERR_NONASCII);
                    }
                    seen += (m >> q) & 1u;
                }
            }
        }
    }
    const unsigned long long r = wave_sum64(st_reads), b = wave_sum64(st_bar), s = wave_sum64(st_short), a = wave_sum64(st_ambig);
    if (lane == 0) {
        if (r) atomicAdd(p.cs + CS_READS, r);
        if (b) atomicAdd(p.cs + CS_BARCUT, b);
        if (s) atomicAdd(p.cs + CS_SHORT, s);
        if (a) atomicAdd(p.cs + CS_AMBIG, a);
    }
}

// slots with count >= min_count -> out[3 k .. 3 k + 2] = {key hi, key lo, count} for k < cap, in no order; *n_out: how many there are
__global__ __launch_bounds__(256) void k_census_compact(const unsigned long long *table, uint64_t nslots, uint32_t two, unsigned long long min_count,
                                                        unsigned long long *out, unsigned long long cap, unsigned long long *n_out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < nslots; i0 += stride) {      // (whole waves stay in the loop)
        const uint64_t i = i0 + threadIdx.x;
        unsigned long long hi = 0, lo = 0, c = 0;
        if (i < nslots) {
            const unsigned long long *s = table + (i << (two ? 2 : 1));
            c = s[two ? 2 : 1];
            hi = s[0]; lo = two ? s[1] : 0ull;
        }
        const bool keep = (c >> 62) == 2 && (c & CC_COUNT) >= min_count;
        const unsigned long long vote = __ballot(keep);
        if (!vote) continue;
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(n_out, (unsigned long long)__popcll(vote));
        at = __shfl(at, 0, 64) + __popcll(vote & ((1ull << lane) - 1ull));
        if (keep && at < cap) { out[3 * at] = hi; out[3 * at + 1] = lo; out[3 * at + 2] = c & CC_COUNT; }
    }
}

}  // namespace tdc

// ============================================================================ host side
namespace {

constexpr uint64_t CENSUS_MIN_SLOTS = 1024, CENSUS_DEFAULT_SLOTS = 1ull << 22, CENSUS_MAX_SLOTS = 1ull << 32;
constexpr size_t CENSUS_LDS_INDEX = 40 * 1024;            // the barcode index's share of a workgroup's LDS

struct Census : tdi::StreamPass {
    uint32_t taglen = 0;
    tdi::DevBuf<unsigned long long> d_table, d_cs;
    uint64_t slots = 0, max_keys = 0;
    int combine = 1;
    size_t slot_words() const { return taglen > 32 ? 4 : 2; }

    int zero(hipStream_t s) override {
        TD_HIPCHK(hipMemsetAsync(d_table.p, 0, slots * slot_words() * 8, s));
        TD_HIPCHK(hipMemsetAsync(d_cs.p, 0, tdc::CS_NWORDS * 8, s));
        return TD_OK;
    }

    int launch(const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, hipStream_t stream,
               const unsigned long long *cursor_in, unsigned long long *cursor_out) override {
        tdc::CensusParams p{};
        const int rc = prologue(d_fastq, nbytes, max_reads, stream, d_cs.p + tdc::CS_TOTAL, p.prefix, p.ntiles);
        if (rc || !p.ntiles) return rc;
        p.buf = (const uint8_t *)d_fastq; p.nbytes = nbytes; p.first_line = first_line;
        p.limit_line = limit_line(max_reads);
        p.bblob = d_bblob.p; p.bblob_bytes = bblob_bytes; p.off_bmeta = off_bmeta; p.off_bdir = off_bdir;
        p.taglen = taglen; p.table = d_table.p; p.slot_mask = slots - 1; p.max_keys = max_keys; p.cs = d_cs.p;
        p.cursor_in = cursor_in; p.cursor_out = cursor_out; p.combine = (uint32_t)combine;
        hipLaunchKernelGGL(tdc::k_census, dim3(grid(p.ntiles, 8, false)), dim3(tdk::BLOCK), bblob_bytes, stream, p);
        TD_HIPCHK(hipGetLastError());
        return TD_OK;
    }

    // after a synchronisation: what the kernels flagged
    int sync_stats(unsigned long long cs[tdc::CS_NWORDS]) {
        const int rc = sync_words(cs, d_cs.p, tdc::CS_NWORDS, tdc::CS_ERR);
        if (rc || !cs[tdc::CS_ERR]) return rc;
        if (cs[tdc::CS_ERR] & tdc::ERR_FULL)
            return latch(TD_E_LIMIT, "census table full: " + std::to_string(slots) + " slots take " + std::to_string(max_keys) + " distinct keys, " +
                                         std::to_string(std::min<unsigned long long>(cs[tdc::CS_DISTINCT], slots)) + " were placed; begin again with more slots");
        return latch(TD_E_INTERNAL, "a wait for a claimed slot timed out inside the census kernel");
    }
};

Census *census_of(td_handle *h) { return tdi::state_of<Census>(h, tdi::CENSUS); }

// A 0, C 1, T 2, G 3 -> A 0, C 1, G 2, T 3 in every 2-bit field: numeric order = the order of the strings
inline uint64_t acgt_order(uint64_t x) { return x ^ ((x >> 1) & 0x5555555555555555ull); }

}  // namespace

extern "C" {

int td_census_begin(td_handle *h, const char *const *barcut, uint32_t n_barcut, uint32_t barnum, const uint32_t *baroff,
                    uint32_t taglen, uint64_t slots) {
    if (!h || !barcut || !baroff) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (taglen < 1 || taglen > TD_CENSUS_MAX_TAGLEN) return td_fail_internal(TD_E_ARG, "taglen must be 1..64");
    if (slots == 0) slots = CENSUS_DEFAULT_SLOTS;
    if (slots < CENSUS_MIN_SLOTS || slots > CENSUS_MAX_SLOTS || (slots & (slots - 1)))
        return td_fail_internal(TD_E_ARG, "slots must be a power of two, 1024 .. 2^32 (0: the default, 2^22)");
    int rc = tdi::quiet_reset(h, tdi::CENSUS); if (rc) return rc;
    std::unique_ptr<Census> c(new Census());
    rc = c->begin(h, barcut, n_barcut, barnum, baroff, CENSUS_LDS_INDEX); if (rc) return rc;
    for (uint32_t b = 0; b < barnum; b++)
        if (baroff[b] > 32) return td_fail_internal(TD_E_LIMIT, "barcode longer than 32 bases");
    c->taglen = taglen; c->slots = slots; c->max_keys = slots / 4 * 3;
    const char *env = getenv("TAGDIG_CENSUS_COMBINE");
    c->combine = env ? (atoi(env) != 0) : 1;
    const hipError_t e = c->d_cs.alloc(tdc::CS_NWORDS);
    if (e != hipSuccess) return tdi::StreamPass::hip_failed(e);
    if (c->d_table.alloc(slots * c->slot_words()) != hipSuccess) {
        (void)hipGetLastError();
        return td_fail_internal(TD_E_HIP, ("no device memory for a census table of " + std::to_string(slots) + " slots").c_str());
    }
    return tdi::install(c, tdi::CENSUS);
}

int td_census_device(td_handle *h, const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, void *stream) {
    Census *c = census_of(h);
    if (!c) return tdi::no_state("census", h, "handle is NULL");
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    return c->launch(d_fastq, nbytes, first_line, max_reads, (hipStream_t)stream, nullptr, nullptr);
}

int td_census_file(td_handle *h, const char *path, uint64_t max_reads) {
    Census *c = census_of(h);
    if (!c || !path) return tdi::no_state("census", h && path);
    unsigned long long cs[tdc::CS_NWORDS];
    const int rc = c->file(path, max_reads);
    return rc ? rc : c->sync_stats(cs);
}

int td_census_stats(td_handle *h, uint64_t out[8]) {
    Census *c = census_of(h);
    if (!c || !out) return tdi::no_state("census", h && out);
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    unsigned long long cs[tdc::CS_NWORDS];
    const int rc = c->sync_stats(cs); if (rc) return rc;
    out[TD_CENSUS_READS] = cs[tdc::CS_READS]; out[TD_CENSUS_BARCUT] = cs[tdc::CS_BARCUT];
    out[TD_CENSUS_SHORT] = cs[tdc::CS_SHORT]; out[TD_CENSUS_AMBIGUOUS] = cs[tdc::CS_AMBIG];
    out[TD_CENSUS_COUNTED] = cs[tdc::CS_BARCUT] - cs[tdc::CS_SHORT] - cs[tdc::CS_AMBIG];
    out[TD_CENSUS_DISTINCT] = cs[tdc::CS_DISTINCT];
    out[TD_CENSUS_SLOTS] = c->slots; out[TD_CENSUS_MAX_KEYS] = c->max_keys;
    return TD_OK;
}

int td_census_fetch(td_handle *h, uint64_t min_count, char *seqs_out, uint64_t *counts_out, uint64_t capacity, uint64_t *n_out) {
    Census *c = census_of(h);
    if (!c || !n_out) return tdi::no_state("census", h && n_out);
    if (capacity && (!seqs_out || !counts_out)) return td_fail_internal(TD_E_ARG, "NULL argument");
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    *n_out = 0;
    unsigned long long cs[tdc::CS_NWORDS];
    int rc = c->sync_stats(cs); if (rc) return rc;
    if (min_count == 0) min_count = 1;
    const uint32_t two = c->taglen > 32 ? 1u : 0u;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((c->slots + 255) / 256, (uint64_t)td_handle_num_cu(h) * 8);
    tdi::DevBuf<unsigned long long> d_n, d_out;
    TD_HIPCHK(d_n.alloc(1));
    unsigned long long n = cs[tdc::CS_DISTINCT];
    // how many there are: a pass that keeps nothing -- run when only the number is asked for, or when room for every
    // distinct window (the bound that needs no pass) would be more than 1 GiB
    const bool count_first = min_count > 1 && (capacity == 0 || n * 24 > (1ull << 30));
    if (count_first) {
        TD_HIPCHK(hipMemset(d_n.p, 0, 8));
        hipLaunchKernelGGL(tdc::k_census_compact, dim3(grid), dim3(256), 0, 0, c->d_table.p, c->slots, two, (unsigned long long)min_count,
                           (unsigned long long *)nullptr, 0ull, d_n.p);
        TD_HIPCHK(hipGetLastError());
        TD_HIPCHK(hipMemcpy(&n, d_n.p, 8, hipMemcpyDeviceToHost));
    }
    if (n == 0 || capacity == 0) { *n_out = n; return TD_OK; }
    TD_HIPCHK(d_out.alloc(n * 3));
    TD_HIPCHK(hipMemset(d_n.p, 0, 8));
    hipLaunchKernelGGL(tdc::k_census_compact, dim3(grid), dim3(256), 0, 0, c->d_table.p, c->slots, two, (unsigned long long)min_count, d_out.p, n, d_n.p);
    TD_HIPCHK(hipGetLastError());
    unsigned long long n2 = 0;
    TD_HIPCHK(hipMemcpy(&n2, d_n.p, 8, hipMemcpyDeviceToHost));
    if (count_first || min_count <= 1 ? n2 != n : n2 > n)
        return td_fail_internal(TD_E_INTERNAL, "census compaction found another number of entries than the table holds");
    n = n2;
    *n_out = n;
    if (n == 0) return TD_OK;
    struct Ent { uint64_t hi, lo, count; };
    std::vector<Ent> ents(n);
    TD_HIPCHK(hipMemcpy(ents.data(), d_out.p, n * 24, hipMemcpyDeviceToHost));
    for (Ent &e : ents) { e.hi = acgt_order(e.hi); e.lo = acgt_order(e.lo); }
    // count descending, then sequence ascending (A < C < G < T)
    std::sort(ents.begin(), ents.end(), [](const Ent &a, const Ent &b) {
        if (a.count != b.count) return a.count > b.count;
        if (a.hi != b.hi) return a.hi < b.hi;
        return a.lo < b.lo;
    });
    const uint32_t L = c->taglen;
    const uint64_t give = std::min<uint64_t>(capacity, n);
    for (uint64_t k = 0; k < give; k++) {
        char *o = seqs_out + k * L;
        for (uint32_t q = 0; q < L; q++) {
            const uint64_t w = q < 32 ? ents[k].hi : ents[k].lo;
            o[q] = "ACGT"[(w >> (62 - 2 * (q & 31))) & 3];
        }
        counts_out[k] = ents[k].count;
    }
    return TD_OK;
}

int td_census_end(td_handle *h) {
    if (!h) return td_fail_internal(TD_E_ARG, "handle is NULL");
    return tdi::quiet_reset(h, tdi::CENSUS);
}

}  // extern "C"
