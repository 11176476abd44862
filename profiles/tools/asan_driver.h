// What the stand-alone AddressSanitizer / UBSan drivers of this directory (*_asan.cpp) share: the stubs that stand in for the parts of the
// product they do not link, the tiny warehouse they create their engines on, and the print-and-exit check of a status.  Each driver keeps
// its own main, cases and recomputation; profiles/tools/Makefile builds the product objects once and the drivers on them.
// ASAN_DRIVER_LINKS_GENERIC_R2, defined in front of the #include: the driver links the real sensor_range-2 generic kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rware_hip.h"
#include "rware_static_table.h"

// the exact-shape table groups and the generic kernels of the sensor ranges no driver steps are stubbed
namespace rw_tab {
#ifndef ASAN_DRIVER_LINKS_GENERIC_R2
step_kernel_t generic_r2(bool, bool, bool, bool) { return nullptr; }
#endif
step_kernel_t generic_r3(bool, bool, bool, bool) { return nullptr; }
step_kernel_t generic_r4(bool, bool, bool, bool) { return nullptr; }
step_kernel_t generic_r5(bool, bool, bool, bool) { return nullptr; }
#define STUB(g) const StaticEntry *static_group_##g(int *n) { *n = 0; return nullptr; }
STUB(0) STUB(1) STUB(2) STUB(3) STUB(4) STUB(5) STUB(6) STUB(7) STUB(8) STUB(9) STUB(10) STUB(11) STUB(12) STUB(13) STUB(14) STUB(15) STUB(16)
STUB(17) STUB(18)
#undef STUB
bool static_has_stats() { return false; }
}  // namespace rw_tab
extern "C" int rw_selftest(int32_t, char *, size_t) { return RW_OK; }

// (`eng`: the rw_engine * in scope at the call)
#define CK(call)                                                                                          \
    do {                                                                                                  \
        const int rc_ = (call);                                                                           \
        if (rc_ != RW_OK) { printf("FAILED %s -> %d: %s\n", #call, rc_, rw_last_error(eng)); exit(1); }   \
    } while (0)

// The tiny warehouse: every third column a highway, the highway rows `highway_row` names (by default the first, the last and every y % 9
// == 8), two goals in the middle of the last row; sensor_range 1, INDIVIDUAL rewards, NEXT_STEP autoreset, FLATTENED observations, 4 envs
// and 64 threads a workgroup, no run-time builds.  A driver overrides the fields of `cfg` its case changes, then create()s.
static inline bool asan_default_highway_row(int y, int H) { return y == 0 || y == H - 1 || y % 9 == 8; }

struct TinyWarehouse {
    std::vector<uint8_t> hw;
    std::vector<int32_t> goals;
    rw_config cfg;
    TinyWarehouse(int B, int H, int W, int N, int Q, int max_steps, bool (*highway_row)(int y, int H) = asan_default_highway_row)
        : hw((size_t)H * W), goals({W / 2 - 1, H - 1, W / 2, H - 1}) {
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) hw[y * W + x] = x % 3 == 0 || highway_row(y, H);
        memset(&cfg, 0, sizeof cfg);
        cfg.abi_version = RW_ABI_VERSION; cfg.num_envs = B; cfg.grid_h = H; cfg.grid_w = W; cfg.n_agents = N; cfg.sensor_range = 1;
        cfg.request_queue_size = Q; cfg.max_steps = max_steps; cfg.reward_type = RW_REWARD_INDIVIDUAL; cfg.autoreset_mode = RW_AUTORESET_NEXT_STEP;
        cfg.n_goals = 2; cfg.envs_per_workgroup = 4; cfg.threads_per_workgroup = 64; cfg.observation_type = RW_OBS_FLATTENED;
        cfg.stream_flags = RW_JIT_OFF; cfg.highways = hw.data(); cfg.goals_xy = goals.data();
    }
    TinyWarehouse(const TinyWarehouse &) = delete;
    rw_engine *create() const {
        rw_engine *eng = nullptr;
        if (rw_create(&cfg, &eng) != RW_OK) { printf("FAILED rw_create: %s\n", rw_last_error(nullptr)); exit(1); }
        return eng;
    }
};
