// numpy-exact random draws for the RWARE engine (device + host).
//
// The reference draws from `numpy.random.Generator(PCG64)` at rware/warehouse.py:781 (agent
// cells), :788 (directions), :797 (request queue) and :916 (replacement request).  numpy is
// not vendored by the reference (setup.py:25, unpinned; 2.2.6 in the build image), so its
// published algorithms are restated here:
//   PCG64      128-bit LCG, multiplier 0x2360ED051FC65DA44385DF649FCCF645, XSL-RR 128/64
//              output of the post-step state; next_uint32 hands out the low half of a fresh
//              64-bit draw and buffers the high half (has_uint32 / uinteger).
//   bounded    random_bounded_uint64 -> buffered_bounded_lemire_uint32 (range < 2^32-1).
//   choice     Generator.choice(pop, size=k, replace=False): Floyd's sampling followed by a
//              Fisher-Yates pass (pop <= 10000).
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#define RW_HD __host__ __device__ __forceinline__

namespace rw {

typedef unsigned __int128 u128;

struct Pcg64 {
    u128 state, inc;
    uint32_t has_uint32, uinteger;
};

RW_HD u128 pcg_mult() { return ((((u128)0x2360ED051FC65DA4ULL) << 64) | 0x4385DF649FCCF645ULL); }

RW_HD uint64_t pcg_next64(Pcg64 &g) {
    g.state = g.state * pcg_mult() + g.inc;
    const uint64_t hi = (uint64_t)(g.state >> 64), lo = (uint64_t)g.state;
    const uint64_t x = hi ^ lo;
    const unsigned rot = (unsigned)(hi >> 58);
    return (x >> rot) | (x << ((0u - rot) & 63u));
}

RW_HD uint32_t pcg_next32(Pcg64 &g) {
    if (g.has_uint32) {
        g.has_uint32 = 0;
        return g.uinteger;
    }
    const uint64_t n = pcg_next64(g);
    g.has_uint32 = 1;
    g.uinteger = (uint32_t)(n >> 32);
    return (uint32_t)n;
}

// numpy SeedSequence(entropy=seed).generate_state(4, uint64) -> PCG64(seed_seq) initial state, as the 6 uint64 of an RW_BUF_RNG
// column {state hi, state lo, inc hi, inc lo, has_uint32 = 0, uinteger = 0}: what gymnasium.utils.seeding.np_random(seed) starts
// from (rware/warehouse.py:758-760).  The entropy words are the seed's low and — only if non-zero — high 32 bits; the pool has 4 words.
// Host (rw_seed_state, rw_reset) and device (rware_seed_kernel) run this one function.
RW_HD void pcg_seed_state(uint64_t seed, uint64_t out[6]) {
    const uint32_t ent[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    const int n_ent = ent[1] ? 2 : 1;
    uint32_t pool[4], hc = 0x43b0d7e5u;
    auto hashmix = [&hc](uint32_t v) {
        v ^= hc;
        hc *= 0x931e8875u;
        v *= hc;
        v ^= v >> 16;
        return v;
    };
    auto mix = [](uint32_t x, uint32_t y) {
        uint32_t r = 0xca01f9ddu * x - 0x4973f715u * y;
        r ^= r >> 16;
        return r;
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) pool[i] = hashmix(i < n_ent ? ent[i & 1] : 0u);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if (s != d) pool[d] = mix(pool[d], hashmix(pool[s]));
    uint32_t w[8], hb = 0x8b51f9ddu;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t v = pool[i & 3] ^ hb;
        hb *= 0x58f38dedu;
        v *= hb;
        v ^= v >> 16;
        w[i] = v;
    }
    uint64_t s64[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) s64[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    const u128 initstate = (((u128)s64[0]) << 64) | s64[1];
    const u128 initseq = (((u128)s64[2]) << 64) | s64[3];
    const u128 inc = (initseq << 1) | 1u;
    u128 state = 0;
    state = state * pcg_mult() + inc;
    state += initstate;
    state = state * pcg_mult() + inc;
    out[0] = (uint64_t)(state >> 64);
    out[1] = (uint64_t)state;
    out[2] = (uint64_t)(inc >> 64);
    out[3] = (uint64_t)inc;
    out[4] = 0;
    out[5] = 0;
}

// uniform integer in [0, rng] (inclusive); rng == 0 consumes nothing, as in numpy
RW_HD uint32_t pcg_bounded(Pcg64 &g, uint32_t rng) {
    if (rng == 0) return 0;
    const uint32_t rng_excl = rng + 1u;
    uint64_t m = (uint64_t)pcg_next32(g) * rng_excl;
    uint32_t leftover = (uint32_t)m;
    if (leftover < rng_excl) {
        const uint32_t threshold = (0xFFFFFFFFu - rng) % rng_excl;
        while (leftover < threshold) {
            m = (uint64_t)pcg_next32(g) * rng_excl;
            leftover = (uint32_t)m;
        }
    }
    return (uint32_t)(m >> 32);
}

// k distinct indices out of [0, pop) into out[0..k): Floyd + Fisher-Yates, numpy's draw order
template <typename IntPtr>
RW_HD void pcg_choice_no_replace(Pcg64 &g, int pop, int k, IntPtr out) {
    const int base = pop - k;
    for (int j = base; j < pop; ++j) {
        const int val = (int)pcg_bounded(g, (uint32_t)j);
        bool seen = false;
        for (int i = 0; i < j - base; ++i) seen |= (out[i] == val);
        out[j - base] = seen ? j : val;
    }
    for (int i = k - 1; i >= 1; --i) {
        const int j = (int)pcg_bounded(g, (uint32_t)i);
        const int t = out[j];
        out[j] = out[i];
        out[i] = t;
    }
}

}  // namespace rw
