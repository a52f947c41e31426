// The host-checkable parts of vcf.hip under the sanitizers (make -C tagdigger_amd/csrc san-vcf; no HIP, never the GPU
// build): the range planner of vcf_ranges.hpp against its definition, and the cell of vcf_cell.hpp -- the code the kernels
// compile for the device -- against snprintf and a second statement of the PL rule.  Exit status 0 and "ok" when all hold.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../vcf_cell.hpp"
#include "../vcf_ranges.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                fprintf(stderr, "FAILED %s: ", #cond);    \
                fprintf(stderr, __VA_ARGS__);             \
                fputc('\n', stderr);                      \
            }                                             \
        }                                                 \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void check_plan(const std::vector<uint64_t> &len, uint64_t budget) {
    const uint64_t K = len.size();
    std::vector<uint64_t> off(K + 1, 0);
    for (uint64_t k = 0; k < K; ++k) off[k + 1] = off[k] + len[k];
    uint64_t longest = ~0ull;
    const std::vector<vcf::Range> r = vcf::plan_ranges(off.data(), K, budget, &longest);
    uint64_t next = 0, most = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].first == next && r[i].last > r[i].first && r[i].last <= K, "range %zu is [%" PRIu64 ", %" PRIu64 ")", i, r[i].first, r[i].last);
        const uint64_t bytes = off[r[i].last] - off[r[i].first];
        CHECK(bytes <= budget || r[i].last == r[i].first + 1, "range %zu holds %" PRIu64 " bytes in several lines", i, bytes);
        if (r[i].last < K)                         // greedy: the next line would not have fitted
            CHECK(off[r[i].last + 1] - off[r[i].first] > budget, "range %zu stops early", i);
        most = bytes > most ? bytes : most;
        next = r[i].last;
    }
    CHECK(next == K, "the ranges end at line %" PRIu64 " of %" PRIu64, next, K);
    CHECK(longest == most, "longest %" PRIu64 " != %" PRIu64, longest, most);
}

template <bool LIK> static void check_cell(uint32_t a, uint32_t b, uint32_t code, uint32_t P, const VcfTab &tab) {
    const VcfCell c = vcf_cell<LIK>(a, b, code, tab);
    const uint32_t len = vcf_cell_len<LIK>(c, P);
    std::vector<uint8_t> buf(len);                 // exactly len bytes: one byte past it is the sanitizer's to catch
    vcf_put_cell<LIK>(buf.data(), c, P);
    std::string want = "\t";
    for (uint32_t j = 0; j < P; ++j) {
        if (j) want += '/';
        want += code > P ? '.' : j < P - code ? '0' : '1';
    }
    char text[96];
    const uint64_t n = (uint64_t)a + b;
    snprintf(text, sizeof text, ":%" PRIu32 ",%" PRIu32 ":%" PRIu64, a, b, n);
    want += text;
    if (LIK) {
        if (code > 2) {
            want += ":.:.";
        } else {
            const uint64_t x = n > 127 ? 127ull * a / n : a, y = n > 127 ? 127ull * b / n : b;
            uint64_t cost[3], cmin = ~0ull, pl[3], gq = 99;
            for (int g = 0; g < 3; ++g) {
                cost[g] = y * tab.ca[g] + x * tab.cb[g];
                cmin = cost[g] < cmin ? cost[g] : cmin;
            }
            for (int g = 0; g < 3; ++g) {
                pl[g] = ((cost[g] - cmin) * 30103 + 327680000) / 655360000;
                if (pl[g] > 255) pl[g] = 255;
                if ((uint32_t)g != code && pl[g] < gq) gq = pl[g];
            }
            snprintf(text, sizeof text, ":%" PRIu64 ":%" PRIu64 ",%" PRIu64 ",%" PRIu64, gq, pl[0], pl[1], pl[2]);
            want += text;
        }
    }
    CHECK(len <= 64, "a cell of %u bytes", len);
    CHECK(want.size() == len && memcmp(want.data(), buf.data(), len) == 0, "a = %u b = %u code = %u P = %u: want '%s', got '%.*s'", a, b, code,
          P, want.c_str(), (int)len, (const char *)buf.data());
}

int main() {
    // the planner: every range one line, budgets hit exactly and missed by one, a line longer than the budget, no line
    check_plan({}, 10);
    check_plan({5, 5, 5, 5}, 1);
    check_plan({5, 5, 5, 5}, 10);
    check_plan({5, 5, 5, 5}, 9);
    check_plan({5, 5, 5, 5}, 11);
    check_plan({5, 50, 5, 5}, 10);
    check_plan({0, 0, 0}, 0);
    check_plan({7}, ~0ull);
    for (int round = 0; round < 300; ++round) {
        std::vector<uint64_t> len(rnd() % 40);
        for (uint64_t &x : len) x = rnd() % 3 ? rnd() % 100 : rnd() % 100000;
        check_plan(len, rnd() % 4 ? rnd() % 300 : rnd() % 200000);
    }
    // the cell: every digit width of both alleles, every code, both forms
    std::vector<uint32_t> edge = {0, 0xffffffffu};
    for (uint64_t p10 = 10; p10 <= 1000000000ull; p10 *= 10) {
        edge.push_back((uint32_t)(p10 - 1));
        edge.push_back((uint32_t)p10);
    }
    const VcfTab tab = {{435412, 65536, 951}, {951, 65536, 435412}};      // about the costs of a 1 % error rate
    const VcfTab steep = {{0, 0, 0}, {0, 10886, 1u << 23}};
    for (uint32_t a : edge)
        for (uint32_t b : edge)
            for (uint32_t code : {0u, 1u, 2u, 3u, 4u, 8u, 9u, 255u}) {
                for (uint32_t P = 2; P <= 8; ++P) check_cell<false>(a, b, code, P, tab);
                check_cell<true>(a, b, code, 2, tab);
                check_cell<true>(a, b, code, 2, steep);
            }
    for (int round = 0; round < 200000; ++round) {
        const uint32_t a = (uint32_t)(rnd() >> (rnd() % 64)), b = (uint32_t)(rnd() >> (rnd() % 64));
        const uint32_t small_a = rnd() % 128, small_b = rnd() % 128, code = rnd() % 4;
        check_cell<true>(a, b, code, 2, tab);
        check_cell<true>(small_a, small_b, code, 2, round & 1 ? tab : steep);
        check_cell<false>(a, small_b, (uint32_t)(rnd() % 10), 2 + (uint32_t)(rnd() % 7), tab);
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    puts("ok");
    return 0;
}
