// What rescue.hip and bcrescue.hip share, moved here from rescue.hip unchanged: the window of a read line as both compare
// it with stored tags -- up to 128 bases from a position inside the line, packed at 2 bits a base into four 64-bit words,
// the first base in the top bits, with a mask of the positions that hold no base or lie behind the line's (stripped) end --
// and td_rescue_begin's checks of the stored tags.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "td_internal.hpp"

namespace tdr {
using namespace tdk;

constexpr uint32_t MAXLEN = TD_RESCUE_MAX_TAGLEN;        // bases of a tag and of the window
static_assert(MAXLEN == 128, "the window is four 64-bit words");

// the 2 * P bits of bases [s0, s0 + P) of four words that hold 32 bases each, first base in the top bits; s0 + P <= 128
__host__ __device__ inline uint64_t part_bits(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t s0, uint32_t P) {
    const uint32_t j = s0 >> 5, o = s0 & 31u;
    const uint64_t hi = j == 0 ? w0 : j == 1 ? w1 : j == 2 ? w2 : w3;
    const uint64_t lo = j == 0 ? w1 : j == 1 ? w2 : j == 2 ? w3 : 0ull;
    const uint64_t x = o ? (hi << (2u * o)) | (lo >> (64u - 2u * o)) : hi;
    return x >> (64u - 2u * P);
}
// bases of word w (32 each) that lie below n, as a mask over their bit pairs
__host__ __device__ inline uint64_t len_mask(uint32_t n, uint32_t w) {
    if (n <= 32u * w) return 0ull;
    const uint32_t c = n - 32u * w;
    return c >= 32u ? ~0ull : ~0ull << (64u - 2u * c);
}
// bit k of m (k = 0: the first base) -> bit 62 - 2k
__device__ __forceinline__ uint64_t spread_mask(uint32_t m) {
    uint64_t x = __brev(m);
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
// mismatching positions of word w between the window and a tag: bit 62 - 2i for base 32w + i
__device__ __forceinline__ uint64_t diff_bits(uint64_t win, uint64_t tag, uint64_t mask, uint32_t n, uint32_t w) {
    const uint64_t x = win ^ tag;
    return (((x | (x >> 1)) & 0x5555555555555555ull) | mask) & len_mask(n, w);
}

struct Window {
    uint64_t w[4];             // the bases, first in the top bits
    uint64_t m[4];             // bit 62 - 2i of word j: base 32j + i is no ACGT, or lies behind the line's end
    uint32_t avail;            // min(len(w), 128)
};

// The window from absolute position ws on, which lies inside the line or on its terminator.
__device__ __forceinline__ void rescue_window(const KParams &kp, uint64_t ws, Window &W) {
    const uint32_t a = (uint32_t)(ws & 15u);
    const uint64_t g0 = ws & ~15ull;
    uint32_t codes[10], inv[10], term[10];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const uint4 v = load_chunk(kp, g0 + 16ull * i);
        const uint2 e = convert_chunk(v);
        codes[i] = e.x; inv[i] = e.y;
        term[i] = eq_mask16(v, 0x0A0A0A0Au) | eq_mask16(v, 0x0D0D0D0Du);
    }
    codes[9] = 0; inv[9] = 0; term[9] = 0;
    uint32_t m32[4], t32[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        m32[j] = (uint32_t)(((((uint64_t)inv[2 * j + 2]) << 32) | (inv[2 * j + 1] << 16) | inv[2 * j]) >> a);
        t32[j] = (uint32_t)(((((uint64_t)term[2 * j + 2]) << 32) | (term[2 * j + 1] << 16) | term[2 * j]) >> a);
        const uint32_t r0 = (uint32_t)((((uint64_t)codes[2 * j] << 32) | codes[2 * j + 1]) >> (32u - 2u * a));
        const uint32_t r1 = (uint32_t)((((uint64_t)codes[2 * j + 1] << 32) | codes[2 * j + 2]) >> (32u - 2u * a));
        W.w[j] = ((uint64_t)r0 << 32) | r1;
    }
    // where the line ends inside the window: its terminator, or the buffer's end
    uint32_t q = MAXLEN;
#pragma unroll
    for (int j = 3; j >= 0; j--) if (t32[j]) q = 32u * j + (uint32_t)__builtin_ctz(t32[j]);
    const uint64_t room = kp.nbytes - ws;
    const uint32_t end = room < q ? (uint32_t)room : q;
    uint64_t e = ws + end;
    // strip: blanks before the end do not belong to the line.  Its last byte is a base in every read but a few
    bool flagged = false;
    if (end) {
        const uint32_t k = end - 1u;
        const uint32_t mw = (k >> 5) == 0 ? m32[0] : (k >> 5) == 1 ? m32[1] : (k >> 5) == 2 ? m32[2] : m32[3];
        flagged = (mw >> (k & 31u)) & 1u;
    }
    if (flagged) {
        if (end == MAXLEN) while (e < kp.nbytes && kp.buf[e] != 0x0Au && kp.buf[e] != 0x0Du) e++;      // the line goes on behind the window
        while (e > ws && is_blank(kp.buf[e - 1])) e--;
    }
    const uint32_t avail = e - ws < MAXLEN ? (uint32_t)(e - ws) : MAXLEN;
    W.avail = avail;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (avail < 32u * (j + 1)) m32[j] |= avail <= 32u * j ? ~0u : ~0u << (avail - 32u * j);
        W.m[j] = spread_mask(m32[j]);
    }
}

}  // namespace tdr

// tags: 1 .. 128 upper-case ACGT, none equal to or a prefix of another
inline int rescue_check_tags(const char *const *tags, uint32_t n_tags, std::vector<std::string> &ts) {
    if (n_tags == 0) return td_fail_internal(TD_E_EMPTY, "empty tag list");
    ts.resize(n_tags);
    for (uint32_t i = 0; i < n_tags; i++) {
        if (!tags[i]) return td_fail_internal(TD_E_ARG, "NULL argument");
        ts[i] = tags[i];
        if (ts[i].empty()) { td_set_bad_index(i); return td_fail_internal(TD_E_EMPTY, "empty tag"); }
        if (ts[i].size() > TD_RESCUE_MAX_TAGLEN) { td_set_bad_index(i); return td_fail_internal(TD_E_LIMIT, "tag longer than 128 bases"); }
        for (char c : ts[i])
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T') { td_set_bad_index(i); return td_fail_internal(TD_E_ALPHABET, "tags must be upper-case ACGT"); }
    }
    // sorted, the tags that begin the current one form a chain: the stack.  The pair reported is the one whose later
    // tag comes first in the input
    std::vector<uint32_t> order(n_tags);
    for (uint32_t i = 0; i < n_tags; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { const int c = ts[a].compare(ts[b]); return c < 0 || (c == 0 && a < b); });
    std::vector<std::pair<uint32_t, uint32_t>> stack;        // (tag, the smallest input position on the stack up to here)
    uint32_t bad = 0xFFFFFFFFu;
    for (uint32_t k : order) {
        while (!stack.empty() && ts[k].compare(0, ts[stack.back().first].size(), ts[stack.back().first]) != 0) stack.pop_back();
        uint32_t low = k;
        if (!stack.empty()) { bad = std::min(bad, std::max(k, stack.back().second)); low = std::min(low, stack.back().second); }
        stack.emplace_back(k, low);
    }
    if (bad != 0xFFFFFFFFu) { td_set_bad_index(bad); return td_fail_internal(TD_E_OVERLAP, "a tag equals another or begins it"); }
    return TD_OK;
}
