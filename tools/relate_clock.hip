// Diagnostic: the core clock the chip holds while k_relate (csrc/relate.hip) runs, for the MFMA floor of
// tools/relate_bench.py.  Builds the kernel with stamps around its marker loop (core cycles by clock64, 100 MHz ticks by
// wall_clock64; one lane per workgroup, summed), launches it back to back on random calls for two seconds and then reads
// one stamped launch: clock = cycles / ticks x 100 MHz.  The library's kernel carries no stamp.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/relate_clock.hip -o relate_clock && ./relate_clock [samples] [markers]
#define TD_RELATE_CLOCK 1
#include "../tagdigger_amd/csrc/relate.hip"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
    const uint32_t S = argc > 1 ? (uint32_t)atoi(argv[1]) : 384u, M = argc > 2 ? (uint32_t)atoi(argv[2]) : 1000000u;
    if (S == 0 || S > TD_RELATE_MAX_SAMPLES || M == 0 || M >= 0x80000000u) return 2;
    std::vector<uint8_t> host((size_t)S * M);
    uint64_t x = 88172645463325252ull;
    for (auto &b : host) {                         // 0 / 1 / 2 and one missing cell in eight
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        b = (x & 7u) == 7u ? 3 : (uint8_t)((x >> 8) % 3u);
    }
    uint8_t *calls = nullptr;
    uint32_t *joint = nullptr;
    unsigned long long *clk = nullptr;
    CK(hipMalloc(&calls, host.size()));
    CK(hipMalloc(&joint, 9ull * S * S * 4));
    CK(hipMalloc(&clk, 16));
    CK(hipMemcpy(calls, host.data(), host.size(), hipMemcpyHostToDevice));
    CK(hipMemset(joint, 0, 9ull * S * S * 4));
    CK(hipMemset(clk, 0, 16));
    const uint32_t ntiles = (S + RL_TILE - 1) / RL_TILE, chunks = (M + RL_KCHUNK - 1) / RL_KCHUNK;
    const dim3 grid(chunks, ntiles * (ntiles + 1) / 2);
    auto launch = [&] { hipLaunchKernelGGL(k_relate, grid, dim3(RL_THREADS), 0, 0, calls, S, M, (const uint8_t *)nullptr, ntiles, joint, clk); };
    const auto t0 = std::chrono::steady_clock::now();
    int launches = 0;
    while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 2.0 && launches < 100000) {
        for (int k = 0; k < 8; ++k) launch();
        launches += 8;
        CK(hipDeviceSynchronize());
    }
    CK(hipMemset(clk, 0, 16));
    launch();
    CK(hipDeviceSynchronize());
    unsigned long long got[2] = {0, 0};
    CK(hipMemcpy(got, clk, 16, hipMemcpyDeviceToHost));
    if (!got[1]) return 3;
    printf("relate_clock samples %u markers %u launches_before %d workgroups %u cycles %llu ticks_100MHz %llu clock_ghz %.3f\n", S, M, launches,
           grid.x * grid.y, got[0], got[1], (double)got[0] / (double)got[1] * 0.1);
    return 0;
}
