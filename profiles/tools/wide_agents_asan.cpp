// Stand-alone AddressSanitizer / UBSan driver for warehouses of more than 64 agents on the host-thread build of the product sources (CPU
// only; no Python): the generic kernel's two-agents-per-lane agent phases (rware_phase_agents_wide.h) and everything behind them.
// The LDS behind a launch's dynamic shared memory is poisoned by the emulation's launch (tests/emu/hip/hip_runtime.h), the host arrays
// are heap blocks of exactly their size, so an out-of-bounds LDS index or store of a kernel faults.  After every step the state is read
// back and checked for what no step may break: every agent inside the grid, no two on one cell, layer 0 of the grid naming exactly the
// agents, every carried shelf under its carrier, the queue holding distinct shelf ids.
// Build, run and compare with profiles/wide_agents_asan.txt: make -C profiles/tools check
// (the exact-shape table groups and sensor ranges 2 .. 5 are stubbed in asan_driver.h: the generic sensor_range-1 kernel steps the envs)
#include "asan_driver.h"

#include <random>
#include <set>

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
    TinyWarehouse wh(B, H, W, N, Q, 20, [](int y, int H_) { return y == 0 || y >= H_ - 2 || y % 9 == 0; });   // (two highway rows at the bottom)
    int S = 0;
    for (uint8_t highway : wh.hw) S += !highway;
    wh.cfg.reward_type = RW_REWARD_TWO_STAGE; wh.cfg.autoreset_mode = autoreset; wh.cfg.threads_per_workgroup = threads;
    wh.cfg.observation_type = obs_type; wh.cfg.stream_flags = RW_JIT_OFF | flags;
    rw_engine *eng = wh.create();
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
