// Stand-alone AddressSanitizer / UBSan driver for rw_snapshot_restore_indexed on the host-thread build of the product sources (CPU only;
// no Python).  The snapshot, the engine's buffers and the index array are heap blocks (the index array of exactly num_envs ints, redzones
// on both sides), the LDS behind a launch's dynamic shared memory is poisoned by the emulation's launch (tests/emu/hip/hip_runtime.h), so
// an out-of-bounds load, store or LDS index of the gather kernel faults; UBSan reports a misaligned wide access.  Every restore is also
// recomputed here in plain loops from rw_read's state before and after, and compared.  Build and run from the repository root:
//   F="-DRW_NO_JIT -DRW_WITH_PIPE=1 -DRW_STATS_BUILD=1 -O1 -g -std=c++17 -pthread -Itests/emu -Irobotic-warehouse_amd/csrc -Wno-unknown-pragmas \
//      -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
//   g++ $F -c -x c++ robotic-warehouse_amd/csrc/rware_capi.hip -o /tmp/ri_capi.o
//   g++ $F -DRW_GENERIC_R=1 -c -x c++ robotic-warehouse_amd/csrc/rware_generic.hip -o /tmp/ri_g1.o
//   g++ $F -c tests/emu/emu_globals.cpp -o /tmp/ri_glob.o
//   g++ $F profiles/tools/restore_indexed_asan.cpp /tmp/ri_capi.o /tmp/ri_g1.o /tmp/ri_glob.o -o /tmp/restore_indexed_asan && /tmp/restore_indexed_asan
// (the exact-shape table groups and sensor ranges 2 .. 5 are stubbed below: the generic sensor_range-1 kernel steps the envs)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

// the state as rw_read shows it: one row of bytes per env and kind (RW_BUF_RNG, field-major on the device, transposed to env-major here)
struct Field { int kind; size_t row; };
using State = std::vector<std::vector<char>>;

static State read_state(rw_engine *eng, const std::vector<Field> &fields, int B) {
    State st;
    for (const Field &f : fields) {
        std::vector<char> raw((size_t)B * f.row);
        CK(rw_read(eng, f.kind, raw.data(), raw.size()));
        if (f.kind == RW_BUF_RNG) {
            std::vector<char> t(raw.size());
            for (int k = 0; k < 6; ++k)
                for (int e = 0; e < B; ++e) memcpy(&t[((size_t)e * 6 + k) * 8], &raw[((size_t)k * B + e) * 8], 8);
            raw.swap(t);
        }
        st.push_back(raw);
    }
    return st;
}

static void play(rw_engine *eng, std::mt19937 &rng, std::vector<int32_t> &act, int N, int M, int steps) {
    for (int t = 0; t < steps; ++t) {
        for (size_t i = 0; i < act.size(); ++i) {
            const unsigned r = rng() % 20;
            act[i] = i % (size_t)(1 + M) ? (int32_t)(r & 1) : r < 1 ? 0 : r < 13 ? 1 : r < 15 ? 2 : r < 17 ? 3 : 4;
        }
        (void)N;
        CK(rw_step(eng, act.data()));
    }
}

static void run(const char *what, int B, int H, int W, int N, int Q, int M) {
    std::vector<uint8_t> hw((size_t)H * W);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) hw[y * W + x] = x % 3 == 0 || y == 0 || y == H - 1 || y % 9 == 8;
    std::vector<int32_t> goals = {W / 2 - 1, H - 1, W / 2, H - 1};
    rw_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = RW_ABI_VERSION; cfg.num_envs = B; cfg.grid_h = H; cfg.grid_w = W; cfg.n_agents = N; cfg.sensor_range = 1;
    cfg.request_queue_size = Q; cfg.max_steps = 9; cfg.reward_type = RW_REWARD_INDIVIDUAL; cfg.autoreset_mode = RW_AUTORESET_NEXT_STEP;
    cfg.n_goals = 2; cfg.envs_per_workgroup = B >= 100 ? 32 : 4; cfg.threads_per_workgroup = 64; cfg.observation_type = RW_OBS_FLATTENED;
    cfg.msg_bits = M; cfg.stream_flags = RW_JIT_OFF; cfg.highways = hw.data(); cfg.goals_xy = goals.data();
    rw_engine *eng = nullptr;
    if (rw_create(&cfg, &eng) != RW_OK) { printf("FAILED rw_create: %s\n", rw_last_error(nullptr)); exit(1); }
    rw_info info;
    CK(rw_get_info(eng, &info));
    std::vector<Field> fields = {{RW_BUF_GRID, (size_t)2 * H * W * 4}, {RW_BUF_AGENT_X, (size_t)N * 4}, {RW_BUF_AGENT_Y, (size_t)N * 4},
                                 {RW_BUF_AGENT_DIR, (size_t)N * 4}, {RW_BUF_AGENT_CARRY, (size_t)N * 4}, {RW_BUF_AGENT_DELIVERED, (size_t)N * 4},
                                 {RW_BUF_QUEUE, (size_t)Q * 4}, {RW_BUF_STEPS, 4}, {RW_BUF_INACTIVE, 4}, {RW_BUF_RNG, 48}, {RW_BUF_NEED_RESET, 1}};
    if (M) fields.push_back({RW_BUF_AGENT_MSG, (size_t)N * 4});
    std::vector<uint64_t> seeds(B);
    for (int e = 0; e < B; ++e) seeds[e] = 100 + e;
    CK(rw_reset(eng, seeds.data(), nullptr));
    std::mt19937 rng(5);
    std::vector<int32_t> act((size_t)B * N * (1 + M));
    play(eng, rng, act, N, M, 7);
    rw_snapshot *snap = nullptr;
    CK(rw_snapshot_create(eng, &snap));
    CK(rw_snapshot_save(eng, snap));
    const State saved = read_state(eng, fields, B);
    long restores = 0, rows = 0;
    for (int round = 0; round < 4; ++round) {
        play(eng, rng, act, N, M, 3);
        for (int e = 0; e < B; ++e) seeds[e] = 1000 * (round + 1) + e;   // other streams: random play alone rarely draws
        CK(rw_reset(eng, seeds.data(), nullptr));
        play(eng, rng, act, N, M, 2);
        const State cur = read_state(eng, fields, B);
        // alternating: every third env keeps its state, between envs that take a random slot (repeats)
        int32_t *index = static_cast<int32_t *>(malloc((size_t)B * sizeof(int32_t)));   // exactly B ints: redzones on both sides
        for (int e = 0; e < B; ++e) index[e] = e % 3 == 2 ? -1 : (int32_t)(rng() % (unsigned)B);
        if (round == 2) for (int e = 0; e < B; ++e) index[e] = e % 3 == 2 ? -1 : B - 1 - e;
        const int keep_rng = round & 1;
        CK(rw_snapshot_restore_indexed(eng, snap, index, keep_rng ? RW_RESTORE_KEEP_RNG : 0));
        CK(rw_sync(eng));
        const State got = read_state(eng, fields, B);
        for (size_t f = 0; f < fields.size(); ++f)
            for (int e = 0; e < B; ++e) {
                const bool take = index[e] >= 0 && !(keep_rng && fields[f].kind == RW_BUF_RNG);
                const char *want = take ? &saved[f][(size_t)index[e] * fields[f].row] : &cur[f][(size_t)e * fields[f].row];
                if (memcmp(&got[f][(size_t)e * fields[f].row], want, fields[f].row) != 0) {
                    printf("FAILED: buffer kind %d of env %d (index %d, keep_rng %d) differs\n", fields[f].kind, e, index[e], keep_rng);
                    exit(1);
                }
                rows += take;
            }
        free(index);
        ++restores;
    }
    // an index outside -1 .. B-1 keeps its env and is reported once
    {
        const State cur = read_state(eng, fields, B);
        int32_t *index = static_cast<int32_t *>(malloc((size_t)B * sizeof(int32_t)));
        for (int e = 0; e < B; ++e) index[e] = e % 3 == 0 ? B : e % 3 == 1 ? -2 : 0x7fffffff;
        CK(rw_snapshot_restore_indexed(eng, snap, index, 0));
        if (rw_sync(eng) != RW_ERR_INVALID_ARG || rw_sync(eng) != RW_OK) { printf("FAILED: bad indices were not reported once\n"); exit(1); }
        const State got = read_state(eng, fields, B);
        if (got != cur) { printf("FAILED: bad indices changed the state\n"); exit(1); }
        free(index);
    }
    printf("asan-run %-30s B %d, %d x %d, %d agents, %d shelves (%s shadow), msg_bits %d: %ld indexed restores (alternating index, every "
           "second one with RW_RESTORE_KEEP_RNG), %ld rows equal the plain recomputation; bad indices left the state alone\n",
           what, B, H, W, N, info.n_shelves, info.n_shelves > 255 ? "uint16" : "uint8", M, restores, rows);
    CK(rw_snapshot_destroy(eng, snap));
    CK(rw_destroy(eng));
}

int main() {
    run("tiny-7: 110-byte shadow rows", 7, 11, 10, 2, 2, 0);
    run("tiny-300: several workgroups", 300, 11, 10, 2, 2, 0);
    run("wide-4x16: 12-byte records", 9, 4, 16, 3, 2, 0);
    run("29x28-10ag: uint16 shadow", 5, 29, 28, 10, 4, 0);
    run("msg: the message piece", 6, 11, 10, 2, 2, 2);
    run("70 agents", 5, 11, 10, 70, 2, 0);
    printf("asan-run done: no AddressSanitizer / UBSan report above = clean\n");
    return 0;
}
