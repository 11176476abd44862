// Stand-alone AddressSanitizer / UBSan driver for rw_global_records and rw_global_image_gather on the host-thread build of the product
// sources (CPU only; no Python).  The "device" arrays are heap blocks of exactly their sizes (redzones on both sides), the LDS behind a
// launch's dynamic shared memory is poisoned by the emulation's launch (tests/emu/hip/hip_runtime.h), so an out-of-bounds load, store or
// LDS index of a kernel faults.  Every record and every gathered image is also recomputed here in plain loops from rw_read's state and
// compared.
// Build, run and compare with profiles/global_records_asan.txt: make -C profiles/tools check
// (the exact-shape table groups and sensor ranges 2 .. 5 are stubbed in asan_driver.h: the generic sensor_range-1 kernel steps the envs)
#include "asan_driver.h"

#include <random>


// what a record says, recomputed from the state: the seven planes (the transposed ones without the agents that have no mirrored cell) and
// the two flags
struct Want {
    std::vector<uint8_t> plane[7];
    int flags = 0;
};
static long g_records = 0, g_images = 0, g_raised = 0, g_bad = 0;

static void recompute(rw_engine *eng, int B, int H, int W, int N, int Q, const std::vector<int32_t> &goals, std::vector<Want> &tape) {
    std::vector<int32_t> grid((size_t)B * 2 * H * W), ax((size_t)B * N), ay(ax), ad(ax), ac(ax), q((size_t)B * Q);
    CK(rw_read(eng, RW_BUF_GRID, grid.data(), grid.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_X, ax.data(), ax.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_Y, ay.data(), ay.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_DIR, ad.data(), ad.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_CARRY, ac.data(), ac.size() * 4));
    CK(rw_read(eng, RW_BUF_QUEUE, q.data(), q.size() * 4));
    for (int e = 0; e < B; ++e) {
        Want w;
        for (auto &p : w.plane) p.assign((size_t)H * W, 0);
        const int32_t *ag = grid.data() + (size_t)e * 2 * H * W, *sh = ag + H * W;
        for (int c = 0; c < H * W; ++c) {
            const int s = sh[c];
            w.plane[0][c] = s > 0;
            for (int k = 0; k < Q; ++k) w.plane[1][c] |= s > 0 && q[(size_t)e * Q + k] == s;
            w.plane[2][c] = ag[c] > 0;
            for (size_t g = 0; g < goals.size() / 2; ++g) w.plane[5][c] |= goals[2 * g] == c % W && goals[2 * g + 1] == c / W;
            w.plane[6][c] = !(ag[c] > 0);
        }
        for (int i = 0; i < N; ++i) {
            const size_t k = (size_t)e * N + i;
            if (ax[k] >= H || ay[k] >= W) { w.flags |= 1 | (ac[k] > 0 ? 2 : 0); continue; }
            w.plane[3][ax[k] * W + ay[k]] = (uint8_t)(ad[k] + 1);
            if (ac[k] > 0) w.plane[4][ax[k] * W + ay[k]] = 1;
        }
        tape.push_back(std::move(w));
    }
}

static void check_records(const uint8_t *rec, const Want *want, int B, int H, int W, int RB) {
    for (int e = 0; e < B; ++e) {
        const uint8_t *r = rec + (size_t)e * RB;
        const Want &w = want[e];
        for (int c = 0; c < H * W; ++c) {
            const int code = w.plane[0][c] | w.plane[1][c] << 1 | w.plane[2][c] << 2 | w.plane[5][c] << 3 | w.plane[4][c] << 4 | w.plane[3][c] << 5;
            if (r[c] != code) { printf("FAILED: record %d, cell %d: 0x%02x, expected 0x%02x\n", e, c, r[c], code); exit(1); }
        }
        if (r[H * W] != w.flags) { printf("FAILED: record %d: flags %d, expected %d\n", e, r[H * W], w.flags); exit(1); }
        for (int c = H * W + 1; c < RB; ++c)
            if (r[c]) { printf("FAILED: record %d: byte %d of the tail is 0x%02x\n", e, c, r[c]); exit(1); }
        ++g_records;
    }
}

static const uint16_t F16[5] = {0, 0x3C00, 0x4000, 0x4200, 0x4400}, BF16[5] = {0, 0x3F80, 0x4000, 0x4040, 0x4080};

template <typename T>
static T encode(int v, int elem) {
    if (elem == RW_GLOBAL_F32) { float f = (float)v; T t; memcpy(&t, &f, sizeof t); return t; }
    return (T)(elem == RW_GLOBAL_U8 ? v : elem == RW_GLOBAL_F16 ? F16[v] : BF16[v]);
}

// T: an unsigned integer of the element's size
template <typename T>
static void gather(rw_engine *eng, const uint8_t *records, const std::vector<Want> &tape, int H, int W, const std::vector<int64_t> &index, bool identity,
                   bool wide, const std::vector<int> &layers, const int *pad, int elem, int shift) {
    const int C = (int)layers.size(), Cp = pad ? pad[0] : C, Hp = pad ? pad[1] : H, Wp = pad ? pad[2] : W;
    const size_t n_index = identity ? tape.size() : index.size(), n = n_index * Cp * Hp * Wp;
    // exactly the images, `shift` bytes behind a 16-byte boundary: the allocation ends with the last image's last byte (or a few bytes on)
    char *block = static_cast<char *>(aligned_alloc(16, std::max<size_t>(16, (n * sizeof(T) + shift + 15) / 16 * 16)));
    T *out = reinterpret_cast<T *>(block + shift);
    // the index in a block of exactly its size, in its width
    void *idx = nullptr;
    if (!identity) {
        idx = malloc(std::max<size_t>(1, index.size() * (wide ? 8 : 4)));
        for (size_t i = 0; i < index.size(); ++i)
            if (wide) static_cast<int64_t *>(idx)[i] = index[i];
            else static_cast<int32_t *>(idx)[i] = (int32_t)index[i];
    }
    std::vector<int32_t> l32(layers.begin(), layers.end());
    CK(rw_global_image_gather(eng, records, (int64_t)tape.size(), idx, (int64_t)n_index, l32.data(), C, pad, elem, wide ? RW_GLOBAL_INDEX64 : 0, out));
    const int rc = rw_sync(eng);
    std::vector<T> want(n, (T)0);
    bool raised = false, bad = false;
    const int c0 = (Cp - C) / 2, h0 = (Hp - H) / 2, w0 = (Wp - W) / 2;
    for (size_t i = 0; i < n_index; ++i) {
        const int64_t j = identity ? (int64_t)i : index[i];
        if (j < 0 || j >= (int64_t)tape.size()) { bad = true; continue; }
        const Want &w = tape[(size_t)j];
        for (int c = 0; c < C; ++c) {
            if (layers[c] == 3 && (w.flags & 1)) raised = true;
            if (layers[c] == 4 && (w.flags & 2)) raised = true;
            T *plane = want.data() + ((i * Cp + c + c0) * Hp + h0) * Wp + w0;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) plane[y * Wp + x] = encode<T>(w.plane[layers[c]][y * W + x], elem);
        }
    }
    const int want_rc = raised ? RW_ERR_INDEX : bad ? RW_ERR_INVALID_ARG : RW_OK;
    if (rc != want_rc) { printf("FAILED: rw_sync -> %d, expected %d\n", rc, want_rc); exit(1); }
    if (rw_sync(eng) != RW_OK) { printf("FAILED: the status word was not cleared\n"); exit(1); }
    if (n && memcmp(want.data(), out, n * sizeof(T)) != 0) { printf("FAILED: images differ (%d layers, elem %d, shift %d)\n", C, elem, shift); exit(1); }
    g_images += (long)n_index;
    g_raised += raised;
    g_bad += bad;
    free(block);
    free(idx);
}

static void run(const char *what, int B, int H, int W, int N, int Q, int steps) {
    const TinyWarehouse wh(B, H, W, N, Q, 25);
    const std::vector<int32_t> &goals = wh.goals;
    rw_engine *eng = wh.create();
    rw_info info;
    CK(rw_get_info(eng, &info));
    const int RB = rw_global_record_bytes(eng);
    if (RB != ((H * W + 1 + 15) & ~15)) { printf("FAILED: RB %d\n", RB); exit(1); }
    std::vector<uint64_t> seeds(B);
    for (int e = 0; e < B; ++e) seeds[e] = 100 + e;
    CK(rw_reset(eng, seeds.data(), nullptr));
    std::mt19937 rng(5);
    std::vector<int32_t> act((size_t)B * N);
    // the tape: exactly steps * B * RB bytes
    uint8_t *records = static_cast<uint8_t *>(aligned_alloc(16, (size_t)steps * B * RB));
    memset(records, 0xA5, (size_t)steps * B * RB);
    std::vector<Want> tape;
    for (int t = 0; t < steps; ++t) {
        for (auto &a : act) { const unsigned r = rng() % 20; a = r < 1 ? 0 : r < 13 ? 1 : r < 15 ? 2 : r < 17 ? 3 : 4; }
        CK(rw_step(eng, act.data()));
        CK(rw_global_records(eng, records + (size_t)t * B * RB));
        CK(rw_sync(eng));
        recompute(eng, B, H, W, N, Q, goals, tape);
        check_records(records + (size_t)t * B * RB, tape.data() + (size_t)t * B, B, H, W, RB);
    }
    const int64_t R = (int64_t)tape.size();
    std::vector<int64_t> shuffled(R), repeats, with_bad;
    for (int64_t i = 0; i < R; ++i) shuffled[i] = (i * 7919 + 3) % R;
    for (int i = 0; i < 37; ++i) repeats.push_back((int64_t)(rng() % (unsigned)R));
    with_bad = {0, -1, R - 1, R, 1, 1};
    const int pads[3][3] = {{8, H + 3, W + 2}, {7, H, W + 5}, {2, H + 1, W}};
    const std::vector<int> all7 = {0, 1, 2, 3, 4, 5, 6}, plain = {0, 1, 2, 5, 6}, one1 = {1}, dup = {0, 0, 6}, eight = {5, 1, 2, 6, 0, 3, 4, 2}, two = {6, 2};
    const std::vector<int64_t> none;
    for (int elem = 0; elem < 4; ++elem) {
        const int sz = elem == RW_GLOBAL_F32 ? 4 : elem == RW_GLOBAL_U8 ? 1 : 2;
        auto go = [&](const std::vector<int64_t> &index, bool identity, bool wide, const std::vector<int> &layers, const int *pad, int shift) {
            shift = shift / sz * sz % 16;
            if (sz == 4) gather<uint32_t>(eng, records, tape, H, W, index, identity, wide, layers, pad, elem, shift);
            else if (sz == 2) gather<uint16_t>(eng, records, tape, H, W, index, identity, wide, layers, pad, elem, shift);
            else gather<uint8_t>(eng, records, tape, H, W, index, identity, wide, layers, pad, elem, shift);
        };
        go(none, true, false, all7, nullptr, 0);
        go(shuffled, false, true, plain, pads[0], 12);
        go(shuffled, false, false, one1, nullptr, 4 + 2 * elem);
        go(repeats, false, true, dup, pads[1], 5);
        go(repeats, false, false, eight, pads[0], 2);
        go(repeats, false, true, two, pads[2], 8);
        go(with_bad, false, true, plain, nullptr, 14);
        go(with_bad, false, false, two, pads[1], 6);
        go(none, false, true, plain, nullptr, 0);
    }
    printf("asan-run %-34s B %d, %d x %d, RB %d, %d agents, %d shelves (%s shadow): %ld records over %d steps and %ld gathered images in four "
           "element types equal the plain recomputation, %ld calls with RW_ERR_INDEX, %ld with an index out of range\n", what, B, H, W, RB, N,
           info.n_shelves, info.n_shelves > 255 ? "uint16" : "uint8", g_records, steps, g_images, g_raised, g_bad);
    g_records = g_images = g_raised = g_bad = 0;
    free(records);
    CK(rw_destroy(eng));
}

int main() {
    run("tall 11 x 10, one ragged workgroup", 7, 11, 10, 3, 2, 20);
    run("wide 4 x 16", 9, 4, 16, 3, 2, 20);
    run("3 x 5: a record of exactly 16", 5, 3, 5, 2, 1, 10);
    run("70 envs: two workgroups, ragged", 70, 11, 10, 2, 2, 6);
    run("40 x 30: uint16 shadow", 3, 40, 30, 10, 4, 8);
    run("100 x 100: the largest grid, E = 1", 2, 100, 100, 5, 3, 3);
    printf("asan-run done: no AddressSanitizer / UBSan report above = clean\n");
    return 0;
}
