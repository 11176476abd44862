// Stand-alone AddressSanitizer / UBSan driver for warehouses of more than 64 agents on the host-thread build of the product sources (CPU
// only; no Python): the generic kernel's two-agents-per-lane agent phases (rware_phase_agents_wide.h) and everything behind them.
// The LDS behind a launch's dynamic shared memory is poisoned by the emulation's launch (tests/emu/hip/hip_runtime.h), the host arrays
// are heap blocks of exactly their size, so an out-of-bounds LDS index or store of a kernel faults.  After every step the state is read
// back and checked for what no step may break: every agent inside the grid, no two on one cell, layer 0 of the grid naming exactly the
// agents, every carried shelf under its carrier, the queue holding distinct shelf ids.  Build and run from the repository root:
//   F="-DRW_NO_JIT -DRW_WITH_PIPE=1 -DRW_STATS_BUILD=1 -O1 -g -std=c++17 -pthread -Itests/emu -Irobotic-warehouse_amd/csrc -Wno-unknown-pragmas \
//      -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
//   g++ $F -c -x c++ robotic-warehouse_amd/csrc/rware_capi.hip -o /tmp/wa_capi.o
//   g++ $F -DRW_GENERIC_R=1 -c -x c++ robotic-warehouse_amd/csrc/rware_generic.hip -o /tmp/wa_g1.o
//   g++ $F -c tests/emu/emu_globals.cpp -o /tmp/wa_glob.o
//   g++ $F profiles/tools/wide_agents_asan.cpp /tmp/wa_capi.o /tmp/wa_g1.o /tmp/wa_glob.o -o /tmp/wide_agents_asan && /tmp/wide_agents_asan
// (the exact-shape table groups and sensor ranges 2 .. 5 are stubbed below: the generic sensor_range-1 kernel steps the envs)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../../include/rware_hip.h"
#include "rware_static_table.h"

namespace rw_tab {
step_kernel_t generic_r2(bool, bool, bool, bool) { return nullptr; }
step_kernel_t generic_r3(bool, bool, bool, bool) { return nullptr; }
step_kernel_t generic_r4(bool, bool, bool, bool) { return nullptr; }
step_kernel_t generic_r5(bool, bool, bool, bool) { return nullptr; }
#define STUB(g) const StaticEntry *static_group_##g(int *n) { *n = 0; return nullptr; }
STUB(0) STUB(1) STUB(2) STUB(3) STUB(4) STUB(5) STUB(6) STUB(7) STUB(8) STUB(9) STUB(10) STUB(11) STUB(12) STUB(13) STUB(14) STUB(15) STUB(16)
STUB(17) STUB(18)
bool static_has_stats() { return false; }
}  // namespace rw_tab
extern "C" int rw_selftest(int32_t, char *, size_t) { return RW_OK; }

#define CK(call)                                                                                          \
    do {                                                                                                  \
        const int rc_ = (call);                                                                           \
        if (rc_ != RW_OK) { printf("FAILED %s -> %d: %s\n", #call, rc_, rw_last_error(eng)); exit(1); }   \
    } while (0)
#define REQUIRE(cond, ...) do { if (!(cond)) { printf("FAILED: " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

static long check_state(rw_engine *eng, int B, int H, int W, int N, int Q, int S) {
    std::vector<int32_t> grid((size_t)B * 2 * H * W), ax((size_t)B * N), ay(ax), ac(ax), q((size_t)B * Q);
    CK(rw_read(eng, RW_BUF_GRID, grid.data(), grid.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_X, ax.data(), ax.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_Y, ay.data(), ay.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_CARRY, ac.data(), ac.size() * 4));
    CK(rw_read(eng, RW_BUF_QUEUE, q.data(), q.size() * 4));
    long loaded = 0;
    for (int e = 0; e < B; ++e) {
        const int32_t *ag = grid.data() + (size_t)e * 2 * H * W, *sh = ag + H * W;
        int on_grid = 0, shelves = 0;
        for (int c = 0; c < H * W; ++c) { on_grid += ag[c] != 0; shelves += sh[c] != 0; }
        REQUIRE(on_grid == N && shelves == S, "env %d: %d agents and %d shelves on the grid", e, on_grid, shelves);
        for (int i = 0; i < N; ++i) {
            const size_t k = (size_t)e * N + i;
            REQUIRE(ax[k] >= 0 && ax[k] < W && ay[k] >= 0 && ay[k] < H, "env %d agent %d at (%d, %d)", e, i, ax[k], ay[k]);
            REQUIRE(ag[ay[k] * W + ax[k]] == i + 1, "env %d agent %d: layer 0 holds %d", e, i, ag[ay[k] * W + ax[k]]);
            REQUIRE(ac[k] >= 0 && ac[k] <= S && (ac[k] == 0 || sh[ay[k] * W + ax[k]] == ac[k]), "env %d agent %d carries %d", e, i, ac[k]);
            loaded += ac[k] != 0;
        }
        std::set<int32_t> ids(q.begin() + (size_t)e * Q, q.begin() + (size_t)(e + 1) * Q);
        REQUIRE((int)ids.size() == Q && *ids.begin() >= 1 && *ids.rbegin() <= S, "env %d: the queue", e);
    }
    return loaded;
}

static void run(const char *what, int B, int H, int W, int N, int Q, int T, int threads, uint32_t flags, int obs_type, int autoreset) {
    std::vector<uint8_t> hw((size_t)H * W);
    int S = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) S += !(hw[y * W + x] = x % 3 == 0 || y == 0 || y >= H - 2 || y % 9 == 0);
    std::vector<int32_t> goals = {W / 2 - 1, H - 1, W / 2, H - 1};
    rw_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = RW_ABI_VERSION; cfg.num_envs = B; cfg.grid_h = H; cfg.grid_w = W; cfg.n_agents = N; cfg.sensor_range = 1;
    cfg.request_queue_size = Q; cfg.max_steps = 20; cfg.reward_type = RW_REWARD_TWO_STAGE; cfg.autoreset_mode = autoreset;
    cfg.n_goals = 2; cfg.envs_per_workgroup = 4; cfg.threads_per_workgroup = threads; cfg.observation_type = obs_type;
    cfg.stream_flags = RW_JIT_OFF | flags; cfg.highways = hw.data(); cfg.goals_xy = goals.data();
    rw_engine *eng = nullptr;
    if (rw_create(&cfg, &eng) != RW_OK) { printf("FAILED rw_create: %s\n", rw_last_error(nullptr)); exit(1); }
    rw_info info;
    CK(rw_get_info(eng, &info));
    REQUIRE(info.build_kind == 0 && info.n_shelves == S, "build kind %d, %d shelves", info.build_kind, info.n_shelves);
    std::vector<uint64_t> seeds(B);
    for (int e = 0; e < B; ++e) seeds[e] = 100 + e;
    CK(rw_reset(eng, seeds.data(), nullptr));
    std::mt19937 rng(5);
    std::vector<int32_t> act((size_t)B * N);
    std::vector<uint8_t> term(B), mask(B);
    long loaded = 0, ended = 0;
    for (int t = 0; t < T; ++t) {
        for (auto &a : act) { const unsigned r = rng() % 20; a = r < 1 ? 0 : r < 13 ? 1 : r < 15 ? 2 : r < 17 ? 3 : 4; }
        CK(rw_step(eng, act.data()));
        loaded += check_state(eng, B, H, W, N, Q, S);
        CK(rw_read(eng, RW_BUF_TERMINATED, term.data(), term.size()));
        for (uint8_t d : term) ended += d;
        if (t == T / 2) {  // a masked reset: every second env, with seeds
            for (int e = 0; e < B; ++e) mask[e] = e % 2 == 0;
            CK(rw_reset(eng, seeds.data(), mask.data()));
            check_state(eng, B, H, W, N, Q, S);
        }
    }
    printf("asan-run %-44s B %d, %d x %d, %3d agents, %3d shelves, %d threads, build kind %d, E %d: %d steps + a masked reset, the state checked "
           "behind each; %ld loaded agent-steps, %ld episode ends\n", what, B, H, W, N, S, threads, info.build_kind, info.envs_per_workgroup, T, loaded, ended);
    CK(rw_destroy(eng));
}

int main() {
    const uint32_t opt_in = RW_STATS_ON | RW_EPISODES_ON | RW_ACTION_MASK_ON | RW_TIME_LIMIT_TRUNCATES;
    run("65 agents, 11 x 10 (one in the second slot)", 5, 11, 10, 65, 20, 50, 256, 0, RW_OBS_FLATTENED, RW_AUTORESET_NEXT_STEP);
    run("65 agents, one wavefront, every opt-in", 5, 11, 10, 65, 20, 50, 64, opt_in, RW_OBS_FLATTENED, RW_AUTORESET_SAME_STEP);
    run("65 agents, packed rows", 5, 11, 10, 65, 20, 50, 128, RW_OBS_PACKED, RW_OBS_FLATTENED, RW_AUTORESET_NEXT_STEP);
    run("127 agents, 20 x 10 (the last id: byte 0xFF)", 5, 20, 10, 127, 40, 50, 256, 0, RW_OBS_FLATTENED, RW_AUTORESET_NEXT_STEP);
    run("127 agents, one wavefront, every opt-in", 5, 20, 10, 127, 40, 50, 64, opt_in, RW_OBS_FLATTENED, RW_AUTORESET_SAME_STEP);
    run("127 agents, uint8 image dict", 5, 20, 10, 127, 40, 50, 256, RW_OBS_IMAGE_U8, RW_OBS_IMAGE_DICT, RW_AUTORESET_DISABLED);
    printf("asan-run done: no AddressSanitizer / UBSan report above = clean\n");
    return 0;
}
