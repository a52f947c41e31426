// The range planner of vcf.hip: plain host C++ with no HIP in it, so that san/vcf_san.cpp can run it under the sanitizers.
//
// line_off[0 .. K] are the non-decreasing byte offsets of K lines (line k is line_off[k] .. line_off[k + 1]).  A range is
// a run of consecutive lines whose bytes total at most `budget`; it always holds at least one line, so a single line longer
// than the budget makes a range of its own that is longer than the budget.  Ranges are cut greedily from the front: a
// range ends in front of the first line that would take it past the budget.
#pragma once
#include <stdint.h>

#include <vector>

namespace [[gnu::visibility("hidden")]] vcf {

struct Range {
    uint64_t first, last;                          // lines first .. last - 1
};

// the ranges of K lines; the largest range's bytes -> *longest (0 for K = 0)
inline std::vector<Range> plan_ranges(const uint64_t *line_off, uint64_t K, uint64_t budget, uint64_t *longest) {
    std::vector<Range> out;
    uint64_t most = 0;
    for (uint64_t k = 0; k < K;) {
        uint64_t e = k + 1;                        // the first line always goes in
        while (e < K && line_off[e + 1] - line_off[k] <= budget) ++e;
        const uint64_t bytes = line_off[e] - line_off[k];
        if (bytes > most) most = bytes;
        out.push_back({k, e});
        k = e;
    }
    if (longest) *longest = most;
    return out;
}

}  // namespace vcf
