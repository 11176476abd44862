// The builds of rware_gae_kernel (csrc/rware_advantages.h) against each other, without an engine: columns per lane (1: element accesses,
// 4: 16-byte ones), steps whose loads are in flight at once (U), non-temporal against plain 16-byte stores, and 64- against 256-thread
// workgroups — what rw_gae's geometry rule was chosen from (profiles/EXPERIMENTS.md, round 20).  Every build's output is compared
// with the first one's, bit for bit, before it is timed.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I robotic-warehouse_amd/csrc -o gae_geometry profiles/tools/gae_geometry.hip && ./gae_geometry
// Per line: us per launch by events, 20 launches between two events, median [min .. max] of 7 such runs, and GB/s of the bytes the
// definition has to move (rewards, values, advantages, returns, the flags twice, valid).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rware_cdna4.h"
using rw::store_f4_nt;
#define RW_ADVANTAGES_KERNEL_ONLY
#include "rware_advantages.h"

#define CHECK(call)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            fprintf(stderr, "%s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
            exit(1);                                                                         \
        }                                                                                    \
    } while (0)

struct Tape {
    rw::GaeArgs a{};
    size_t out_bytes = 0, moved = 0;
    std::vector<float> first[2];   // the first build's advantages, without and with the team sum
};

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

static Tape make_tape(int T, int B, int N, int K) {
    Tape t;
    const size_t cols = (size_t)B * K, rr = (size_t)B * N;
    std::vector<float> rew(T * rr), val(T * cols), last(cols);
    std::vector<uint8_t> term((size_t)T * B), trunc((size_t)T * B), prev(B);
    uint32_t s = 12345u;
    for (auto &x : rew) x = (float)(lcg(s) >> 8) / (float)(1 << 24) - 0.5f;
    for (auto &x : val) x = (float)(lcg(s) >> 8) / (float)(1 << 23) - 1.0f;
    for (auto &x : last) x = (float)(lcg(s) >> 8) / (float)(1 << 23) - 1.0f;
    for (auto &x : term) x = (lcg(s) >> 8) % 50 == 0;
    for (auto &x : trunc) x = (lcg(s) >> 8) % 50 == 0;
    for (auto &x : prev) x = (lcg(s) >> 8) % 2;
    auto up = [](const void *h, size_t n) {
        void *d = nullptr;
        CHECK(hipMalloc(&d, n));
        CHECK(hipMemcpy(d, h, n, hipMemcpyHostToDevice));
        return d;
    };
    t.out_bytes = T * cols * 4;
    t.a.rewards = (const float *)up(rew.data(), rew.size() * 4);
    t.a.values = (const float *)up(val.data(), val.size() * 4);
    t.a.last_values = (const float *)up(last.data(), last.size() * 4);
    t.a.terminated = (const uint8_t *)up(term.data(), term.size());
    t.a.truncated = (const uint8_t *)up(trunc.data(), trunc.size());
    t.a.prev_ended = (const uint8_t *)up(prev.data(), prev.size());
    CHECK(hipMalloc((void **)&t.a.advantages, t.out_bytes));
    CHECK(hipMalloc((void **)&t.a.returns, t.out_bytes));
    CHECK(hipMalloc((void **)&t.a.valid, (size_t)T * B));
    t.a.cols = (int64_t)cols; t.a.row_rewards = (int64_t)rr;
    t.a.T = T; t.a.B = B; t.a.N = N; t.a.K = K; t.a.next_step = 1;
    t.a.g = 0.99f; t.a.gl = 0.99f * 0.95f;
    t.moved = rew.size() * 4 + val.size() * 4 + 2 * t.out_bytes + 3 * (size_t)T * B;
    return t;
}

static void free_tape(Tape &t) {
    for (const void *p : {(const void *)t.a.rewards, (const void *)t.a.values, (const void *)t.a.last_values, (const void *)t.a.terminated,
                          (const void *)t.a.truncated, (const void *)t.a.prev_ended, (const void *)t.a.advantages, (const void *)t.a.returns,
                          (const void *)t.a.valid})
        CHECK(hipFree(const_cast<void *>(p)));
}

template <int CPL, int U, bool TEAM, bool NT>
static void measure(Tape &t, unsigned block, const char *what) {
    const uint64_t threads = (uint64_t)t.a.cols / CPL;
    if (t.a.cols % CPL) return;
    const unsigned blocks = (unsigned)((threads + block - 1) / block);
    const bool one = CPL == 4 && t.a.K % 4 == 0;   // (a lane's four columns lie in one env: rw_gae's choice of the build)
    auto go = [&]() {
        if (one) hipLaunchKernelGGL((rw::rware_gae_kernel<CPL, U, TEAM, NT, CPL == 4>), dim3(blocks), dim3(block), 0, 0, t.a);
        else hipLaunchKernelGGL((rw::rware_gae_kernel<CPL, U, TEAM, NT, false>), dim3(blocks), dim3(block), 0, 0, t.a);
    };
    CHECK(hipMemset(t.a.advantages, 0xA5, t.out_bytes));
    go();
    CHECK(hipDeviceSynchronize());
    std::vector<float> got(t.out_bytes / 4);
    CHECK(hipMemcpy(got.data(), t.a.advantages, t.out_bytes, hipMemcpyDeviceToHost));
    if (t.first[TEAM].empty()) t.first[TEAM] = got;
    const bool same = memcmp(got.data(), t.first[TEAM].data(), t.out_bytes) == 0;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<float> us;
    for (int rep = 0; rep < 7; ++rep) {
        CHECK(hipEventRecord(e0, 0));
        for (int i = 0; i < 20; ++i) go();
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        us.push_back(ms * 1000.0f / 20.0f);
    }
    std::sort(us.begin(), us.end());
    printf("%s T %d B %d N %d K %d: columns/lane %d, steps in flight %d, %s stores, %u-thread workgroups (%u): %.1f us [%.1f .. %.1f], %.0f GB/s%s\n",
           what, t.a.T, t.a.B, t.a.N, t.a.K, CPL, U, NT ? "non-temporal" : "plain", block, blocks, us[3], us[0], us[6],
           (double)t.moved / us[3] / 1e3, same ? "" : "  ** DIFFERS from the first build **");
    fflush(stdout);
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
}

template <bool TEAM>
static void sweep(Tape &t, const char *what) {
    for (unsigned block : {64u, 256u}) {
        measure<1, 1, TEAM, false>(t, block, what);
        measure<1, 2, TEAM, false>(t, block, what);
        measure<1, 4, TEAM, false>(t, block, what);
        measure<1, 8, TEAM, false>(t, block, what);
        measure<1, 16, TEAM, false>(t, block, what);
        measure<1, 4, TEAM, true>(t, block, what);
        measure<1, 8, TEAM, true>(t, block, what);
        measure<4, 1, TEAM, true>(t, block, what);
        measure<4, 2, TEAM, true>(t, block, what);
        measure<4, 4, TEAM, true>(t, block, what);
        measure<4, 8, TEAM, true>(t, block, what);
        measure<4, 4, TEAM, false>(t, block, what);
        measure<4, 8, TEAM, false>(t, block, what);
    }
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    printf("# gae_geometry: us per launch, median [min .. max] of 7 runs of 20 launches; %s\n", prop.name);
    {   // the headline shape: a 64-step tape of 16384 four-agent warehouses, a per-agent critic
        Tape t = make_tape(64, 16384, 4, 4);
        sweep<false>(t, "per-agent");
        free_tape(t);
    }
    {   // twice the columns
        Tape t = make_tape(64, 32768, 4, 4);
        sweep<false>(t, "per-agent");
        free_tape(t);
    }
    {   // four times the columns
        Tape t = make_tape(64, 65536, 4, 4);
        sweep<false>(t, "per-agent");
        free_tape(t);
    }
    {   // sixteen times the columns (1 048 576): the only shape above the rule's threshold, the two paths and both workgroup sizes
        Tape t = make_tape(64, 262144, 4, 4);
        for (unsigned block : {64u, 256u}) {
            measure<1, 4, false, true>(t, block, "per-agent");
            measure<1, 8, false, true>(t, block, "per-agent");
            measure<4, 4, false, true>(t, block, "per-agent");
            measure<4, 8, false, true>(t, block, "per-agent");
        }
        free_tape(t);
    }
    // the team reward: K = N lanes of an env that all sum its N rewards, against one lane per env (K = 1) and against the same tape
    // without the sum (what the N loads a step cost)
    for (int N : {16, 127}) {
        const int B = N == 16 ? 4096 : 512;
        Tape t = make_tape(64, B, N, N);
        for (unsigned block : {64u, 256u}) {
            measure<1, 4, false, false>(t, block, "no sum   ");
            measure<1, 4, true, false>(t, block, "team K=N ");
            measure<1, 8, true, false>(t, block, "team K=N ");
            if (t.a.cols % 4 == 0) {
                measure<4, 4, false, true>(t, block, "no sum   ");
                measure<4, 4, true, true>(t, block, "team K=N ");
            }
        }
        free_tape(t);
        Tape one = make_tape(64, B, N, 1);
        for (unsigned block : {64u, 256u}) {
            measure<1, 4, true, false>(one, block, "team K=1 ");
            measure<1, 8, true, false>(one, block, "team K=1 ");
            if (one.a.cols % 4 == 0) measure<4, 4, true, true>(one, block, "team K=1 ");
        }
        free_tape(one);
    }
    return 0;
}
