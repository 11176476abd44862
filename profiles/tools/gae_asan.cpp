// Stand-alone AddressSanitizer / UBSan driver for rw_gae on the host-thread build of the product sources (CPU only; no Python).  The
// "device" arrays are heap blocks of exactly their sizes (redzones on both sides), so a load or store of the kernel outside a tape
// faults.  Every result is also recomputed here in plain loops, one float operation a statement, and compared bit for bit.  The shapes
// are those of tests/test_gae.py, crossed with both modes, the optional arrays present and NULL, four (gamma, lambda) and both paths
// (every array on a 16-byte boundary; the float arrays one element behind one).
// Build, run and compare with profiles/gae_asan.txt: make -C profiles/tools check
// (the exact-shape table groups and sensor ranges 2 .. 5 are stubbed in asan_driver.h: rw_gae takes the device and the stream from the engine only)
#include "asan_driver.h"

#include <random>

static rw_engine *eng = nullptr;
static long g_calls = 0, g_elems = 0;

// a heap block of exactly `bytes` whose payload starts `shift` bytes behind a 16-byte boundary: the block is bytes + shift long and the
// payload ends where the block ends; in front of the payload lie `shift` poisoned bytes the kernel must leave alone
struct Block {
    uint8_t *base = nullptr, *p = nullptr;
    size_t bytes = 0, shift = 0;
    Block(size_t n, size_t s) : bytes(n), shift(s) {
        base = static_cast<uint8_t *>(malloc(n + s));   // (malloc gives 16-byte alignment on this ABI; checked)
        if (reinterpret_cast<uintptr_t>(base) % 16) { printf("FAILED: malloc is not 16-byte aligned\n"); exit(1); }
        memset(base, 0xA5, n + s);
        p = base + s;
    }
    ~Block() {
        for (size_t i = 0; i < shift; ++i)
            if (base[i] != 0xA5) { printf("FAILED: a byte in front of an array was written\n"); exit(1); }
        free(base);
    }
    Block(const Block &) = delete;
};

static void one_case(int T, int B, int N, int K, bool team, bool ns, bool has_trunc, bool has_fv, bool has_prev, bool has_ret, bool has_valid,
                     float gamma, float lam, size_t shift, std::mt19937 &rng) {
    const size_t cols = (size_t)B * K, rr = (size_t)B * N, tb = (size_t)T * B;
    Block rew(T * rr * 4, shift), val(T * cols * 4, shift), last(cols * 4, shift), fv(T * cols * 4, shift), adv(T * cols * 4, shift),
        ret(T * cols * 4, shift), term(tb, 0), trunc(tb, 0), prev(B, 0), valid(tb, 0);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    auto fill = [&](Block &b) { for (size_t i = 0; i < b.bytes / 4; ++i) { const float x = nd(rng); memcpy(b.p + 4 * i, &x, 4); } };
    fill(rew); fill(val); fill(last); fill(fv);
    for (size_t i = 0; i < tb; ++i) { term.p[i] = rng() % 5 == 0 ? (uint8_t)(1 + rng() % 255) : 0; trunc.p[i] = rng() % 5 == 0 ? 1 : 0; }
    for (int b = 0; b < B; ++b) prev.p[b] = rng() % 2;
    rw_gae_args a;
    memset(&a, 0, sizeof a);
    a.rewards_dev = (const float *)rew.p; a.values_dev = (const float *)val.p; a.last_values_dev = (const float *)last.p;
    a.terminated_dev = term.p; a.truncated_dev = has_trunc ? trunc.p : nullptr; a.final_values_dev = has_fv ? (const float *)fv.p : nullptr;
    a.prev_ended_dev = has_prev ? prev.p : nullptr; a.advantages_dev = (float *)adv.p; a.returns_dev = has_ret ? (float *)ret.p : nullptr;
    a.valid_dev = has_valid ? valid.p : nullptr;
    a.n_steps = T; a.n_envs = B; a.n_agents = N; a.n_heads = K; a.gamma = gamma; a.lam = lam;
    a.flags = (ns ? RW_GAE_NEXT_STEP : 0) | (team ? RW_GAE_TEAM_REWARD : 0);
    if (rw_gae(eng, &a) != RW_OK || rw_sync(eng) != RW_OK) { printf("FAILED rw_gae: %s\n", rw_last_error(eng)); exit(1); }
    // the definition in plain loops
    const float *R = (const float *)rew.p, *V = (const float *)val.p, *L = (const float *)last.p, *F = (const float *)fv.p;
    const float g = gamma;
    volatile float gl_ = gamma * lam;
    const float gl = gl_;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < K; ++k) {
            float carry = 0.0f, next_v = L[(size_t)b * K + k];
            for (int t = T - 1; t >= 0; --t) {
                float r;
                if (team) {
                    r = R[t * rr + (size_t)b * N];
                    for (int i = 1; i < N; ++i) { volatile float s = r + R[t * rr + (size_t)b * N + i]; r = s; }
                } else r = R[t * rr + (size_t)b * N + k];
                const size_t at = t * cols + (size_t)b * K + k, fl = (size_t)t * B + b;
                const float v = V[at];
                const bool te = term.p[fl] != 0, tr = has_trunc && trunc.p[fl] != 0;
                const bool reset = ns && (t > 0 ? (term.p[fl - B] | (has_trunc ? trunc.p[fl - B] : 0)) != 0 : has_prev && prev.p[b] != 0);
                const float boot = te ? 0.0f : tr ? (ns ? next_v : has_fv ? F[at] : 0.0f) : next_v;
                volatile float m = g * boot;
                volatile float s = r + m;
                volatile float delta = s - v;
                float x = delta;
                if (!(te || tr)) { volatile float c = gl * carry; volatile float y = delta + c; x = y; }
                if (reset) x = 0.0f;
                volatile float rt = x + v;
                const float rt_ = rt;
                if (memcmp(adv.p + 4 * at, &x, 4) != 0 || (has_ret && memcmp(ret.p + 4 * at, &rt_, 4) != 0) ||
                    (has_valid && valid.p[fl] != (reset ? 0 : 1))) {
                    printf("FAILED: T %d B %d N %d K %d team %d next_step %d differs at t %d b %d k %d\n", T, B, N, K, team, ns, t, b, k);
                    exit(1);
                }
                carry = x;
                next_v = v;
            }
        }
    // what was not handed over stays as it was
    for (size_t i = 0; i < ret.bytes; ++i) if (!has_ret && ret.p[i] != 0xA5) { printf("FAILED: returns written without a pointer\n"); exit(1); }
    for (size_t i = 0; i < tb; ++i) if (!has_valid && valid.p[i] != 0xA5) { printf("FAILED: valid written without a pointer\n"); exit(1); }
    ++g_calls;
    g_elems += (long)(T * cols);
}

int main() {
    const TinyWarehouse wh(2, 11, 10, 2, 2, 25);
    setenv("RWARE_HOOKS", "1", 1);
    eng = wh.create();
    const struct { const char *what; int T, B, N, K; bool team; } shapes[] = {
        {"one", 1, 1, 1, 1, false}, {"6 columns", 2, 3, 2, 2, false}, {"12 columns", 9, 4, 3, 3, false}, {"team, 1 head", 9, 5, 3, 1, true},
        {"team, 3 heads", 9, 4, 3, 3, true}, {"65 agents", 5, 2, 65, 65, false}, {"team, 65 agents", 5, 2, 65, 1, true},
        {"280 columns", 3, 70, 4, 4, false}, {"20 steps", 20, 5, 4, 4, false}, {"17 steps, team", 17, 3, 8, 8, true},
    };
    const float gl[4][2] = {{0.99f, 0.95f}, {1.0f, 1.0f}, {0.0f, 0.5f}, {0.9f, 0.0f}};
    std::mt19937 rng(7);
    for (const auto &s : shapes) {
        for (size_t shift : {(size_t)0, (size_t)4}) {
            // (rw_gae's rule gives a lane four columns from 64 * 1024 such lanes on; the hook of csrc/rware_hooks.h takes the rule's place,
            //  so that the aligned half of the calls runs the 16-byte path where B*K is a multiple of 4)
            setenv("RWARE_GAE_COLUMNS", shift == 0 ? "4" : "1", 1);
            for (int bits = 0; bits < 64; ++bits)
                one_case(s.T, s.B, s.N, s.K, s.team, bits & 1, bits & 2, bits & 4, bits & 8, bits & 16, bits & 32, gl[bits % 4][0],
                         gl[(bits / 4 + bits) % 4][1], shift, rng);
        }
        printf("asan-run rw_gae %-16s T %d B %d N %d K %d%s: %ld calls (both modes x truncated, final_values, prev_ended, returns, valid present "
               "or NULL x aligned and one element off), %ld elements equal the plain recomputation\n", s.what, s.T, s.B, s.N, s.K,
               s.team ? " team" : "", g_calls, g_elems);
        g_calls = g_elems = 0;
    }
    if (rw_destroy(eng) != RW_OK) return 1;
    printf("gae_asan: clean\n");
    return 0;
}
