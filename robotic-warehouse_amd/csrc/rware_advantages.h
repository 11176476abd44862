// Advantages and returns from the rollout tapes on the learner's side: rw_gae (include/rware_hip.h, include/rware_hip_advantages.h).
// Included at file scope of rware_capi.hip behind rware_global_state.h (by that header's last line, so that rware_capi.hip itself stays
// as it is): it needs float4 / store_f4_nt (rware_cdna4.h) and, for the host part at the end, the engine internals (rw_engine, fail, RW_HIP).  The kernel first, the host part below it.  Plain C++ throughout: the
// host-thread build of tests/emu compiles this file as it is.
//
// GAE(lambda) is a recurrence over t per column (b, k) of the [T][B][K] value tape, and include/rware_hip_advantages.h fixes the order
// of its float32 operations, so a column is never split over threads: one thread owns CPL adjacent columns — 4 (16-byte loads and
// stores) where every float array starts on a 16-byte boundary, B*K is a multiple of 4 and the tape is large enough for that to pay
// (rw_gae's rule, at the end of this file), else 1 (the element path) — and walks t from T-1 down to 0.  What a step reads does not depend on the recurrence, and with only B*K / CPL threads the memory system is kept busy by loads
// in flight per lane alone: the walk goes in chunks of U steps, whose loads are ALL issued before anything waits for one of them.
// That rules out every branch on a loaded value and every copy of one inside the load phase (either puts a wait for the whole queue
// there; the first build had them and ran one memory round trip per step whatever U was: profiles/EXPERIMENTS.md, round 20):
//   flags      the bytes of rows t .. t - U + 1, and once per chunk those of row t - U (the reset test of RW_GAE_NEXT_STEP looks at the
//              row before; row -1 is prev_ended).  A NULL array, row -1 and the other mode are a pointer select and a mask, no branch
//   env        col / K, found once per thread.  Where K is a multiple of CPL the thread's columns share one env — known without looking
//              at a loaded value — and the flags and the reward sum are loaded for the first column alone
//   TEAM       the env's N rewards summed left to right by every lane that needs the sum, the U steps of the chunk side by side in
//              one loop over the agents (U loads in flight per trip); the lanes of one env read the same address in the same instruction
//   final      V(final_obs) is read only where a step is truncated and not terminated: rare element loads, in a phase of their own
//              behind the flags, and only without RW_GAE_NEXT_STEP
//   stores     advantages, returns (16 bytes a lane on the vector path) and one valid byte per env from the lane of its head 0
// The arithmetic sits under `#pragma clang fp contract(off)`: hipcc otherwise fuses r + g * boot and delta + gl * carry into v_fmac_f32
// (also through __fadd_rn(__fmul_rn())), which rounds once where the definition rounds twice.
#pragma once

namespace rw {

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
__device__ __forceinline__ void store_f1_nt(float *dst, float v) { __builtin_nontemporal_store(v, dst); }
#else
inline void store_f1_nt(float *dst, float v) { *dst = v; }  // (the hint has no host meaning)
#endif

struct GaeArgs {
    const float *rewards, *values, *last_values, *final_values;   // final_values: NULL unless the mode reads them
    const uint8_t *terminated, *truncated, *prev_ended;           // prev_ended: NULL unless the mode reads it
    float *advantages, *returns;
    uint8_t *valid;
    int64_t cols, row_rewards;                                    // B * K, B * N: the elements of one step's row
    int32_t T, B, N, K, next_step;
    float g, gl;
};

template <int CPL>
struct GaeStep {
    float r[CPL], v[CPL], fv[CPL];
    uint32_t term[CPL], trunc[CPL];   // the flag bytes as loaded: non-zero = set
};

// flags[at] where `ok`, else 0 — without a branch: a byte that exists (any[0]) is loaded instead and masked away
__device__ __forceinline__ uint32_t gae_flag(const uint8_t *flags, int64_t at, const uint8_t *any, bool ok) {
    return (uint32_t)(ok ? flags : any)[ok ? at : 0] & (ok ? 0xFFu : 0u);
}

// the loads of step t for the columns c0 .. c0 + CPL - 1 (envs e[]): the flags first (the final_values phase waits for them alone)
template <int CPL, bool TEAM, bool ONE>
__device__ __forceinline__ void gae_load(const GaeArgs &a, int t, int64_t c0, const int32_t (&e)[CPL], GaeStep<CPL> &s) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        if (j == 0 || !ONE) {
            const int64_t at = (int64_t)t * a.B + e[j];
            s.term[j] = a.terminated[at];
            s.trunc[j] = gae_flag(a.truncated, at, a.terminated, a.truncated != nullptr);
        } else {
            s.term[j] = s.trunc[j] = 0u;
        }
    }
    const int64_t row = (int64_t)t * a.cols + c0;
    if constexpr (CPL == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(a.values + row);
        s.v[0] = v.x; s.v[1] = v.y; s.v[2] = v.z; s.v[3] = v.w;
        if constexpr (!TEAM) {
            const float4 r = *reinterpret_cast<const float4 *>(a.rewards + row);   // (K == N: the same index)
            s.r[0] = r.x; s.r[1] = r.y; s.r[2] = r.z; s.r[3] = r.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            s.v[j] = a.values[row + j];
            if constexpr (!TEAM) s.r[j] = a.rewards[row + j];
        }
    }
}

// whether the step before step t ended an episode, per column, as RW_GAE_NEXT_STEP asks: row t - 1, or prev_ended in front of row 0
template <int CPL, bool ONE>
__device__ __forceinline__ void gae_ended_before(const GaeArgs &a, int t, const int32_t (&e)[CPL], uint32_t (&ended)[CPL]) {
    const bool row = a.next_step && t > 0, prev = a.next_step && t == 0 && a.prev_ended != nullptr;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        if (j == 0 || !ONE) {
            const int64_t at = (int64_t)(t - 1) * a.B + e[j];
            ended[j] = gae_flag(a.terminated, at, a.terminated, row) | gae_flag(a.truncated, at, a.terminated, row && a.truncated != nullptr) |
                       gae_flag(a.prev_ended, e[j], a.terminated, prev);
        } else {
            ended[j] = 0u;
        }
    }
}

// step t of the recurrence for CPL columns, and its stores; ended_before[]: gae_ended_before(t), or the flags of step t - 1 of the chunk
template <int CPL, bool TEAM, bool NT, bool ONE>
__device__ __forceinline__ void gae_step(const GaeArgs &a, int t, int64_t c0, const int32_t (&e)[CPL], const bool (&head0)[CPL],
                                         const GaeStep<CPL> &s, const uint32_t (&ended_before)[CPL], float (&carry)[CPL], float (&next_v)[CPL]) {
#pragma clang fp contract(off)
    float adv[CPL], ret[CPL];
    bool reset[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        // (the column's flags and reward sum are where they were loaded: a select of values, no run-time index into registers)
        const bool term = (ONE ? s.term[0] : s.term[j]) != 0, trunc = (ONE ? s.trunc[0] : s.trunc[j]) != 0;
        reset[j] = (ONE ? ended_before[0] : ended_before[j]) != 0;
        const float v = s.v[j];
        const float boot = term ? 0.0f : trunc ? (a.next_step ? next_v[j] : s.fv[j]) : next_v[j];
        const float gb = a.g * boot;
        const float rb = (TEAM && ONE ? s.r[0] : s.r[j]) + gb;
        const float delta = rb - v;
        const float gc = a.gl * carry[j];
        const float more = delta + gc;
        float x = (term || trunc) ? delta : more;
        if (reset[j]) x = 0.0f;
        adv[j] = x;
        ret[j] = x + v;
        carry[j] = x;
        next_v[j] = v;
    }
    const int64_t row = (int64_t)t * a.cols + c0;
    if constexpr (CPL == 4) {
        float4 o;
        o.x = adv[0]; o.y = adv[1]; o.z = adv[2]; o.w = adv[3];
        if constexpr (NT) store_f4_nt(reinterpret_cast<float4 *>(a.advantages + row), o);
        else *reinterpret_cast<float4 *>(a.advantages + row) = o;
        if (a.returns) {
            o.x = ret[0]; o.y = ret[1]; o.z = ret[2]; o.w = ret[3];
            if constexpr (NT) store_f4_nt(reinterpret_cast<float4 *>(a.returns + row), o);
            else *reinterpret_cast<float4 *>(a.returns + row) = o;
        }
    } else {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            if constexpr (NT) store_f1_nt(a.advantages + row + j, adv[j]);
            else a.advantages[row + j] = adv[j];
            if (a.returns) {
                if constexpr (NT) store_f1_nt(a.returns + row + j, ret[j]);
                else a.returns[row + j] = ret[j];
            }
        }
    }
    if (a.valid) {
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (head0[j]) a.valid[(int64_t)t * a.B + e[j]] = reset[j] ? 0 : 1;
    }
}

// the steps t, t - 1, .. t - U + 1: every load of theirs, then the recurrence
template <int CPL, int U, bool TEAM, bool NT, bool ONE>
__device__ __forceinline__ void gae_chunk(const GaeArgs &a, int t, int64_t c0, const int32_t (&e)[CPL], const bool (&head0)[CPL],
                                          float (&carry)[CPL], float (&next_v)[CPL]) {
    GaeStep<CPL> s[U];
    uint32_t tail[CPL];
#pragma unroll
    for (int u = 0; u < U; ++u) gae_load<CPL, TEAM, ONE>(a, t - u, c0, e, s[u]);
    gae_ended_before<CPL, ONE>(a, t - U + 1, e, tail);
    if constexpr (TEAM) {
        const float *p[U][CPL];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < CPL; ++j)
                if (j == 0 || !ONE) {
                    p[u][j] = a.rewards + (int64_t)(t - u) * a.row_rewards + (int64_t)e[j] * a.N;
                    s[u].r[j] = p[u][j][0];
                }
        for (int i = 1; i < a.N; ++i) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < CPL; ++j)
                    if (j == 0 || !ONE) s[u].r[j] = s[u].r[j] + p[u][j][i];
        }
    }
    if (a.final_values) {   // (the one phase that looks at loaded flags before it loads)
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const bool read = (ONE ? s[u].trunc[0] : s[u].trunc[j]) != 0 && (ONE ? s[u].term[0] : s[u].term[j]) == 0;
                s[u].fv[j] = read ? a.final_values[(int64_t)(t - u) * a.cols + c0 + j] : 0.0f;
            }
    } else {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < CPL; ++j) s[u].fv[j] = 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const GaeStep<CPL> &older = s[u + 1 < U ? u + 1 : u];   // (step t - u - 1, where the chunk holds it)
        uint32_t before[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) before[j] = u + 1 < U ? (a.next_step ? older.term[j] | older.trunc[j] : 0u) : tail[j];
        gae_step<CPL, TEAM, NT, ONE>(a, t - u, c0, e, head0, s[u], before, carry, next_v);
    }
}

// CPL columns a thread, U steps' loads in flight, TEAM: summed rewards, NT: non-temporal stores, ONE: K is a multiple of CPL (the
// thread's columns share one env; a template argument, for as a run-time one it sent the chunk's registers to scratch memory)
template <int CPL, int U, bool TEAM, bool NT, bool ONE = false>
__global__ void __launch_bounds__(256) rware_gae_kernel(const GaeArgs a) {
    const int64_t c0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * CPL;
    if (c0 >= a.cols) return;   // (CPL 4: cols is a multiple of 4, so a thread has all of its columns or none)
    int32_t e[CPL];
    bool head0[CPL];
    float carry[CPL], next_v[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        e[j] = (int32_t)((uint32_t)(c0 + j) / (uint32_t)a.K);   // (cols < 2^31: a 32-bit division, once per thread)
        head0[j] = (uint32_t)(c0 + j) - (uint32_t)e[j] * (uint32_t)a.K == 0u;
        carry[j] = 0.0f;
        next_v[j] = a.last_values[c0 + j];
    }
    int t = a.T - 1;
    for (; t >= U - 1; t -= U) gae_chunk<CPL, U, TEAM, NT, ONE>(a, t, c0, e, head0, carry, next_v);
    for (; t >= 0; --t) gae_chunk<CPL, 1, TEAM, NT, ONE>(a, t, c0, e, head0, carry, next_v);
}

}  // namespace rw

#ifndef RW_ADVANTAGES_KERNEL_ONLY   // (profiles/tools/gae_geometry.hip times the kernel's builds on their own, without an engine)
// ---- host part ----------------------------------------------------------------------------------------------------------------------

// rw_gae's measured threshold: the lanes below which four columns a lane lose to one
enum : uint64_t { GAE_VEC_MIN_THREADS = 64u * 1024u };

extern "C" {

int rw_gae(rw_engine *eng, const rw_gae_args *args) {
    // One launch of rware_gae_kernel on the engine's stream and nothing else: the host reads none of the arrays, so the call is legal
    // inside a stream capture and is replayed with the graph.  The engine gives the device and the stream; the shape is the tape's.
    if (!eng) return RW_ERR_INVALID_ARG;
    if (!args) return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: NULL args");
    const rw_gae_args &g = *args;
    if (g.n_steps < 0 || g.n_envs < 0 || g.n_agents < 0 || g.n_heads < 0)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: n_steps %d, n_envs %d, n_agents %d, n_heads %d: none may be negative", (int)g.n_steps,
                    (int)g.n_envs, (int)g.n_agents, (int)g.n_heads);
    if (g.n_heads != 1 && g.n_heads != g.n_agents)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: n_heads %d is neither 1 nor n_agents (%d)", (int)g.n_heads, (int)g.n_agents);
    if (g.flags & ~(int32_t)(RW_GAE_NEXT_STEP | RW_GAE_TEAM_REWARD))
        return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: unknown flag bits 0x%x", (unsigned)(g.flags & ~(int32_t)(RW_GAE_NEXT_STEP | RW_GAE_TEAM_REWARD)));
    if (g.reserved != 0) return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: reserved is %d, has to be 0", (int)g.reserved);
    const bool team = (g.flags & RW_GAE_TEAM_REWARD) != 0, next_step = (g.flags & RW_GAE_NEXT_STEP) != 0;
    if (g.n_heads == 1 && g.n_agents != 1 && !team)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: n_heads 1 with n_agents %d needs RW_GAE_TEAM_REWARD", (int)g.n_agents);
    if (!(g.gamma >= 0.0f && g.gamma <= 1.0f) || !(g.lam >= 0.0f && g.lam <= 1.0f))   // (a NaN fails both comparisons)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: gamma %g, lam %g: both have to lie in [0, 1]", (double)g.gamma, (double)g.lam);
    const char *missing = !g.rewards_dev ? "rewards_dev" : !g.values_dev ? "values_dev" : !g.last_values_dev ? "last_values_dev"
                          : !g.terminated_dev ? "terminated_dev" : !g.advantages_dev ? "advantages_dev" : nullptr;
    if (missing) return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: NULL %s", missing);
    // what the mode does not read is not looked at
    const float *final_values = next_step ? nullptr : g.final_values_dev;
    const uint8_t *prev_ended = next_step ? g.prev_ended_dev : nullptr;
    const uint64_t T = (uint64_t)g.n_steps, B = (uint64_t)g.n_envs, cols = B * (uint64_t)g.n_heads, row_rewards = B * (uint64_t)g.n_agents;
    if (cols >= (1ull << 31) || row_rewards >= (1ull << 31) || T * std::max(cols, row_rewards) >= (1ull << 40))
        return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: %d steps of %d envs with %d agents and %d heads are more columns or elements than one launch "
                    "holds; compute in slices of envs", (int)g.n_steps, (int)g.n_envs, (int)g.n_agents, (int)g.n_heads);
    struct Range { const char *name; uintptr_t lo; uint64_t bytes; bool is_float, is_out; };
    const auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    const Range ranges[] = {
        {"rewards_dev", at(g.rewards_dev), T * row_rewards * 4, true, false}, {"values_dev", at(g.values_dev), T * cols * 4, true, false},
        {"last_values_dev", at(g.last_values_dev), cols * 4, true, false},   {"terminated_dev", at(g.terminated_dev), T * B, false, false},
        {"truncated_dev", at(g.truncated_dev), T * B, false, false},         {"final_values_dev", at(final_values), T * cols * 4, true, false},
        {"prev_ended_dev", at(prev_ended), B, false, false},                 {"advantages_dev", at(g.advantages_dev), T * cols * 4, true, true},
        {"returns_dev", at(g.returns_dev), T * cols * 4, true, true},        {"valid_dev", at(g.valid_dev), T * B, false, true},
    };
    bool aligned16 = true;
    for (const Range &r : ranges) {
        if (!r.lo) continue;
        if (r.is_float && (r.lo & 3u)) return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: %s has to be 4-byte aligned", r.name);
        if (r.is_float && (r.lo & 15u)) aligned16 = false;
        if (!r.is_out || !r.bytes) continue;
        for (const Range &o : ranges)
            if (&o != &r && o.lo && o.bytes && r.lo < o.lo + o.bytes && o.lo < r.lo + r.bytes)
                return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: the output %s overlaps %s", r.name, o.name);
    }
    if (T == 0 || cols == 0) return RW_OK;
    if (g.n_agents == 0) return fail(eng, RW_ERR_INVALID_ARG, "rw_gae: n_heads 1 needs n_agents >= 1");
    rw::GaeArgs a{};
    a.rewards = g.rewards_dev; a.values = g.values_dev; a.last_values = g.last_values_dev; a.final_values = final_values;
    a.terminated = g.terminated_dev; a.truncated = g.truncated_dev; a.prev_ended = prev_ended;
    a.advantages = g.advantages_dev; a.returns = g.returns_dev; a.valid = g.valid_dev;
    a.cols = (int64_t)cols; a.row_rewards = (int64_t)row_rewards;
    a.T = g.n_steps; a.B = g.n_envs; a.N = g.n_agents; a.K = g.n_heads; a.next_step = next_step ? 1 : 0;
    a.g = g.gamma;
    a.gl = g.gamma * g.lam;   // (one float32 multiply: part of the definition)
    // Geometry, from the shape (measured on the MI355X: profiles/EXPERIMENTS.md round 20, profiles/gae_geometry.txt).
    //   columns a lane   four, with 16-byte accesses, where the arrays allow it, no sum is asked for AND that still leaves
    //                    GAE_VEC_MIN_THREADS lanes.  Below, a launch is short of wavefronts, not of bytes per instruction: one column a lane
    //                    took 16.5 us against 31.7 at 65 536 columns, 23.8 against 34.5 at 131 072, 47.7 against 48.2 at 262 144.  With
    //                    the team sum the loop over the agents dominates and four columns a lane lost at every size (27 against 150 us
    //                    at 16 agents).  (RWARE_GAE_COLUMNS=1|4, a test / A-B hook of rware_hooks.h, takes the size condition's
    //                    place: the tests run the 16-byte path on tapes of a few columns.)
    //                    At 1 048 576 columns, the one shape measured above the threshold, four columns a lane take 201 us against 208.
    //   steps in flight  eight with one column a lane (19.1 -> 16.5 us from four at 65 536 columns, 18.0 with sixteen); four with four
    //                    columns a lane (201 against 216 us at 1 048 576 columns, 48.9 against 48.2 at 262 144)
    //   workgroups       four wavefronts from 64 * 1024 lanes on (16.5 against 18.9 us there), one below: few lanes do better spread over
    //                    many compute units (4096 lanes that sum 16 rewards each: 53 against 117 us)
    //   stores           non-temporal on both paths: 47.7 against 59.7 us at 262 144 columns, nothing lost at 65 536
    const bool can_vec = aligned16 && cols % 4 == 0 && !team;
    bool vec = can_vec && cols / 4 >= GAE_VEC_MIN_THREADS;
    if (const char *h = rw_hook("RWARE_GAE_COLUMNS")) vec = can_vec && h[0] == '4';
    const uint64_t threads = vec ? cols / 4 : cols;
    const unsigned block = threads >= 64u * 1024u ? 256u : 64u;
    const unsigned blocks = (unsigned)((threads + block - 1) / block);
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    if (!vec) {
        if (team) hipLaunchKernelGGL((rw::rware_gae_kernel<1, 8, true, true>), dim3(blocks), dim3(block), 0, eng->stream, a);
        else hipLaunchKernelGGL((rw::rware_gae_kernel<1, 8, false, true>), dim3(blocks), dim3(block), 0, eng->stream, a);
    } else if (g.n_heads % 4 == 0) {   // (a lane's four columns lie in one env)
        hipLaunchKernelGGL((rw::rware_gae_kernel<4, 4, false, true, true>), dim3(blocks), dim3(block), 0, eng->stream, a);
    } else {
        hipLaunchKernelGGL((rw::rware_gae_kernel<4, 4, false, true, false>), dim3(blocks), dim3(block), 0, eng->stream, a);
    }
    RW_HIP(eng, hipGetLastError());
    return RW_OK;
}

}  // extern "C"
#endif  // RW_ADVANTAGES_KERNEL_ONLY
