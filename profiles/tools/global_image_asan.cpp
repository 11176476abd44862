// Stand-alone AddressSanitizer / UBSan driver for rw_global_image on the host-thread build of the product sources (CPU only; no Python).
// The "device" arrays are heap blocks of exactly the image's size (redzones on both sides), the LDS behind a launch's dynamic shared
// memory is poisoned by the emulation's launch (tests/emu/hip/hip_runtime.h), so an out-of-bounds store or LDS index of the kernel faults.
// Every image is also recomputed here in plain loops from rw_read's state and compared.
// Build, run and compare with profiles/global_image_asan.txt: make -C profiles/tools check
// (the exact-shape table groups and sensor ranges 2 .. 5 are stubbed in asan_driver.h: the generic sensor_range-1 kernel steps the envs)
#include "asan_driver.h"

#include <random>


static long g_images = 0, g_raised = 0;

template <typename T>
static void one(rw_engine *eng, int B, int H, int W, int N, int Q, const std::vector<int32_t> &goals, const std::vector<int> &layers,
                const int *pad, int shift) {
    const int C = (int)layers.size(), Cp = pad ? pad[0] : C, Hp = pad ? pad[1] : H, Wp = pad ? pad[2] : W;
    const size_t n = (size_t)B * Cp * Hp * Wp;
    // exactly the image, `shift` bytes behind a 16-byte boundary: the allocation ends with the image's last byte
    char *block = static_cast<char *>(aligned_alloc(16, (n * sizeof(T) + shift + 15) / 16 * 16));
    T *out = reinterpret_cast<T *>(block + shift);
    std::vector<int32_t> l32(layers.begin(), layers.end());
    CK(rw_global_image(eng, l32.data(), C, pad, sizeof(T) == 4 ? 0 : 1, out));
    const int rc = rw_sync(eng);
    if (rc != RW_OK && rc != RW_ERR_INDEX) { printf("FAILED rw_sync -> %d\n", rc); exit(1); }
    std::vector<int32_t> grid((size_t)B * 2 * H * W), ax((size_t)B * N), ay(ax), ad(ax), ac(ax), q((size_t)B * Q);
    CK(rw_read(eng, RW_BUF_GRID, grid.data(), grid.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_X, ax.data(), ax.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_Y, ay.data(), ay.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_DIR, ad.data(), ad.size() * 4));
    CK(rw_read(eng, RW_BUF_AGENT_CARRY, ac.data(), ac.size() * 4));
    CK(rw_read(eng, RW_BUF_QUEUE, q.data(), q.size() * 4));
    std::vector<T> want(n, (T)0);
    bool raised = false;
    const int c0 = (Cp - C) / 2, h0 = (Hp - H) / 2, w0 = (Wp - W) / 2;
    for (int e = 0; e < B; ++e)
        for (int c = 0; c < C; ++c) {
            T *plane = want.data() + (((size_t)e * Cp + c + c0) * Hp + h0) * Wp + w0;   // [y * Wp + x]
            const int32_t *ag = grid.data() + (size_t)e * 2 * H * W, *sh = ag + H * W;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const int s = sh[y * W + x];
                    int v = 0;
                    if (layers[c] == 0) v = s > 0;
                    if (layers[c] == 1) for (int k = 0; k < Q; ++k) v |= s > 0 && q[(size_t)e * Q + k] == s;
                    if (layers[c] == 2) v = ag[y * W + x] > 0;
                    if (layers[c] == 5) for (size_t g = 0; g < goals.size() / 2; ++g) v |= goals[2 * g] == x && goals[2 * g + 1] == y;
                    if (layers[c] == 6) v = !(ag[y * W + x] > 0);
                    plane[y * Wp + x] = (T)v;
                }
            if (layers[c] == 3 || layers[c] == 4)
                for (int i = 0; i < N; ++i) {
                    const size_t k = (size_t)e * N + i;
                    if (layers[c] == 4 && ac[k] <= 0) continue;
                    if (ax[k] >= H || ay[k] >= W) { raised = true; continue; }
                    plane[ax[k] * Wp + ay[k]] = (T)(layers[c] == 3 ? ad[k] + 1 : 1);
                }
        }
    if ((rc == RW_ERR_INDEX) != raised) { printf("FAILED: RW_ERR_INDEX %d, expected %d\n", rc == RW_ERR_INDEX, raised); exit(1); }
    if (memcmp(want.data(), out, n * sizeof(T)) != 0) { printf("FAILED: image differs (%d layers, %zu-byte elements, shift %d)\n", C, sizeof(T), shift); exit(1); }
    ++g_images;
    g_raised += raised;
    free(block);
}

static void run(const char *what, int B, int H, int W, int N, int Q, int steps) {
    const TinyWarehouse wh(B, H, W, N, Q, 25);
    const std::vector<int32_t> &goals = wh.goals;
    rw_engine *eng = wh.create();
    rw_info info;
    CK(rw_get_info(eng, &info));
    std::vector<uint64_t> seeds(B);
    for (int e = 0; e < B; ++e) seeds[e] = 100 + e;
    CK(rw_reset(eng, seeds.data(), nullptr));
    std::mt19937 rng(5);
    std::vector<int32_t> act((size_t)B * N);
    const int pads[3][3] = {{8, H + 3, W + 2}, {7, H, W + 5}, {2, H + 1, W}};
    for (int t = 0; t < steps; ++t) {
        for (auto &a : act) { const unsigned r = rng() % 20; a = r < 1 ? 0 : r < 13 ? 1 : r < 15 ? 2 : r < 17 ? 3 : 4; }
        CK(rw_step(eng, act.data()));
        const std::vector<int> all7 = {0, 1, 2, 3, 4, 5, 6}, plain = {0, 1, 2, 5, 6}, one1 = {1}, dup = {0, 0, 6}, eight = {5, 1, 2, 6, 0, 3, 4, 2};
        one<float>(eng, B, H, W, N, Q, goals, all7, nullptr, 0);
        one<uint8_t>(eng, B, H, W, N, Q, goals, all7, nullptr, 0);
        one<float>(eng, B, H, W, N, Q, goals, one1, nullptr, 4 * (t % 4));
        one<uint8_t>(eng, B, H, W, N, Q, goals, one1, nullptr, t % 16);
        one<float>(eng, B, H, W, N, Q, goals, plain, pads[t % 2], 12);
        one<uint8_t>(eng, B, H, W, N, Q, goals, dup, pads[t % 2], 5);
        one<uint8_t>(eng, B, H, W, N, Q, goals, eight, pads[0], t % 16);
        one<float>(eng, B, H, W, N, Q, goals, {6, 2}, pads[2], 8);
    }
    printf("asan-run %-34s B %d, %d x %d, %d agents, %d shelves (%s shadow), step kernel build kind %d: %ld images over %d steps equal the plain "
           "recomputation, %ld with RW_ERR_INDEX\n", what, B, H, W, N, info.n_shelves, info.n_shelves > 255 ? "uint16" : "uint8", info.build_kind,
           g_images, steps, g_raised);
    g_images = g_raised = 0;
    CK(rw_destroy(eng));
}

int main() {
    run("tall 11 x 10, one ragged workgroup", 7, 11, 10, 3, 2, 30);
    run("wide 4 x 16", 9, 4, 16, 3, 2, 30);
    run("70 envs: two workgroups, ragged", 70, 11, 10, 2, 2, 12);
    run("40 x 30: uint16 shadow", 3, 40, 30, 10, 4, 12);
    run("100 x 100: the largest grid, E = 1", 2, 100, 100, 5, 3, 3);
    printf("asan-run done: no AddressSanitizer / UBSan report above = clean\n");
    return 0;
}
