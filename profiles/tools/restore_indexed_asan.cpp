// Stand-alone AddressSanitizer / UBSan driver for rw_snapshot_restore_indexed on the host-thread build of the product sources (CPU only;
// no Python).  The snapshot, the engine's buffers and the index array are heap blocks (the index array of exactly num_envs ints, redzones
// on both sides), the LDS behind a launch's dynamic shared memory is poisoned by the emulation's launch (tests/emu/hip/hip_runtime.h), so
// an out-of-bounds load, store or LDS index of the gather kernel faults; UBSan reports a misaligned wide access.  Every restore is also
// recomputed here in plain loops from rw_read's state before and after, and compared.
// Build, run and compare with profiles/restore_indexed_asan.txt: make -C profiles/tools check
// (the exact-shape table groups and sensor ranges 2 .. 5 are stubbed in asan_driver.h: the generic sensor_range-1 kernel steps the envs)
#include "asan_driver.h"

#include <random>


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
    TinyWarehouse wh(B, H, W, N, Q, 9);
    wh.cfg.envs_per_workgroup = B >= 100 ? 32 : 4; wh.cfg.msg_bits = M;
    rw_engine *eng = wh.create();
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
