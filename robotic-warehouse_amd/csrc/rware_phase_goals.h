// rware_phase_goals.h — part of rw::rware_step_kernel (rware_kernels.h), included INSIDE the kernel body: P5 — goals, request replacement (numpy-exact draw), rewards, counters, termination: one env, run by its leader lane; count_events (RW_STATS_ON)
// A textual unit, not a function: the phases share ~60 locals (LDS pointers, shapes, the agent lanes' registers), and every
// way of passing them that was tried — lambdas, always_inline or not — reschedules the kernels around it (round 5: +-10
// instructions per kernel, two 13/14-agent builds over a register cliff).  Splitting the text keeps every build's ISA.
    // P5 of one env, run by its leader lane once the moves are applied (:903-942): goals in list order, request replacement
    // with the numpy-exact draw, rewards, the env's counters and termination.  ONE copy, used by both agent-phase
    // implementations below (each kernel instantiation has exactly one call site, so it is inlined there).
#if RW_STATS_BUILD
    // done_split (RW_STATS_BUILD kernels with RW_TIME_LIMIT_TRUNCATES): what ENVI_DONE holds for an env whose step ended its episode — bit 0
    // `done` as ever, bit 1 the inactivity rule fired (`terminated`), bit 2 the step limit did (`truncated`).  Computed where `done` is, from
    // the counters of that step: the reset path zeroes them before it stores the flags.  Every other reader of ENVI_DONE tests it against 0;
    // without the flag the word stays 0 / 1.
    auto done_split = [&](int inact, int steps) {
        return 1 | ((k_max_inactivity && inact >= k_max_inactivity) ? 2 : 0) | ((k_max_steps && steps >= k_max_steps) ? 4 : 0);
    };
#endif
    auto goals_and_termination = [&](int e, int ge, int base, int32_t *ev, CellT *gS, uint8_t *gA) {
        int32_t *q = s_queue + e * Q;
        bool delivered = false;
        int n_deliv = 0;  // (only read by the RW_STATS_BUILD kernels)
        for (int gi = 0; gi < k_n_goals; ++gi) {  // in list order (:904)
            const int cell = gi == 0 ? k_goal0 : gi == 1 ? k_goal1 : p.goal_cells[gi];
            const int sid = gS[cell];
            if (!sid) continue;
            int slot = -1;  // first queue slot holding sid; all Q entries read in one LDS batch (no early exit)
            for (int k = Q - 1; k >= 0; --k) slot = (q[k] == sid) ? k : slot;
            if (slot < 0) continue;
            delivered = true;
            ++n_deliv;
            ev[ENVI_QDIRTY] = 1;
            // candidates = shelves not in the queue, id order; one bounded draw (:915-916)
            Pcg64 rg;
            rng_load(rg, p.rng, B, ge);
            const int idx = (int)pcg_bounded(rg, (uint32_t)(S - Q - 1));
            rng_store(rg, p.rng, B, ge);
            int cand = idx + 1;  // idx-th id (0-based) among ids 1..S that are not queued
            for (;;) {
                int c = 0;
                for (int k = 0; k < Q; ++k) c += (q[k] <= cand) ? 1 : 0;
                const int nc = idx + 1 + c;
                if (nc == cand) break;
                cand = nc;
            }
            q[slot] = cand;
            if (k_reward_type == REW_GLOBAL) {
                for (int k = 0; k < N; ++k) s_rew[base + k] += 1.0f;
            } else {
                const int aid = gA[cell] & 0x7f;
                const int ai = aid > 0 ? aid - 1 : N - 1;  // rewards[-1] when nobody stands there
                if (k_reward_type == REW_INDIVIDUAL) {
                    s_rew[base + ai] += 1.0f;
                } else {
                    s_deliv[base + ai] = 1;
                    s_rew[base + ai] += 0.5f;
                }
            }
        }
        if (stats_on) ev[ENVI_NDELIV] = n_deliv;
        ev[ENVI_INACTIVE] = delivered ? 0 : ev[ENVI_INACTIVE] + 1;
        ev[ENVI_STEPS] += 1;
        const int done = ((k_max_inactivity && ev[ENVI_INACTIVE] >= k_max_inactivity) ||
                          (k_max_steps && ev[ENVI_STEPS] >= k_max_steps)) ? 1 : 0;
        ev[ENVI_DONE] = done;
#if RW_STATS_BUILD
        if (RW_RARE(trunc_on) && done) ev[ENVI_DONE] = done_split(ev[ENVI_INACTIVE], ev[ENVI_STEPS]);
#endif
        if (done && k_autoreset == AR_SAME_STEP) {
            ev[ENVI_RESET] = 1;
            atomicOr(&s_misc[0], 1);
        }
    };
    // count_events (RW_STATS_BUILD kernels with RW_STATS_ON; off the common path everywhere): adds the step's deliveries and failed moves of the chunk's envs
    // to the per-env running totals in HBM.  Nothing of it lives in the agent phases: a delivery count is left in ENVI_NDELIV by the
    // (rare) goal path, and a failed move is re-derived here from what the write-back holds anyway — the agent asked for FORWARD
    // (its action, re-read: an L2 hit), did not move (s_mv) and the cell ahead is inside the grid (a wall-clamped FORWARD is a
    // self-target the reference leaves alone, :105-112): the shelf-block cancel (:843-846) or a lost resolution (:871-876).
    //   terminal == false  the envs this launch stepped and did not reset (from the write-back, role 1);
    //   terminal == true   SAME_STEP autoreset: the envs this step terminated, before RS overwrites their arrays (from RS).
    auto count_events = [&](bool terminal, int first, int stride) {
        if (op != OP_STEP) return;
        for (int i = first; i < nea; i += stride) {
            const int e = rw_div18(i, mN);
            const int32_t *ev = s_envi + e * ENVI_W;
            if (ev[ENVI_SKIP] || (terminal ? !(ev[ENVI_DONE] && ev[ENVI_RESET]) : ev[ENVI_RESET] != 0)) continue;
            const int x = s_ax[i], y = s_ay[i], d = s_dir[i];
            const bool ahead = d == DIR_UP ? y > 0 : d == DIR_DOWN ? y < H - 1 : d == DIR_LEFT ? x > 0 : x < W - 1;
            if (act_t[((size_t)e0 * N + i) * AM] == ACT_FORWARD && s_mv[i] < 0 && ahead) atomicAdd(p.stat_failed_moves + (e0 + e), 1);
        }
        for (int e = first; e < ne; e += stride) {
            const int32_t *ev = s_envi + e * ENVI_W;
            if (ev[ENVI_SKIP] || (terminal ? !(ev[ENVI_DONE] && ev[ENVI_RESET]) : ev[ENVI_RESET] != 0)) continue;
            if (ev[ENVI_INACTIVE] == 0) atomicAdd(p.stat_deliveries + (e0 + e), ev[ENVI_NDELIV]);
        }
    };
#if RW_STATS_BUILD
    // ep_tick (RW_STATS_BUILD kernels with RW_EPISODES_ON): one step of the per-episode return / length of agent i / env e, by the ONE lane
    // that writes that agent / env back this step — the write-back roles for the envs that stepped and stay, RS for the envs it resets.
    // The running values live in LDS for the launch (s_epr, s_epl): add, record-and-clear, add is an ORDERED sequence, and in a fused
    // rollout step t's write-back and step t + 1's reset path run on different wavefronts with LDS-only barriers between them — HBM would not
    // order them, LDS does.  HBM sees the running values once, at the launch's last step (`last`).
    //   the env stepped (not ENVI_SKIP)   ret += reward, len += 1; `terminated` set: last_* = the sums, count += 1, then both 0 — in every
    //                                     autoreset mode (SAME_STEP: RS calls this for the env it is about to reset; s_rew still holds the
    //                                     terminating step's rewards, ENVI_DONE its flag)
    //   it did not (ENVI_SKIP)            a NEXT_STEP reset step or rw_reset: both 0, nothing recorded
    // last_* and count have one writer per element for an engine's lifetime — the same lane of the same wavefront every step (the mode is
    // fixed per engine: RS under SAME_STEP, the write-back role otherwise) — so plain stores stay in order; count is an integer atomic.
    const bool ep_last = !kRollout || t + 1 == n_steps;
    auto ep_tick_agent = [&](int i, const int32_t *ev) {
        const size_t gi = (size_t)e0 * N + i;
        float r = 0.0f;
        if (op == OP_STEP && !ev[ENVI_SKIP]) {
            r = s_epr[i] + s_rew[i];
            if (ev[ENVI_DONE]) { as_global(p.ep_last_return)[gi] = r; r = 0.0f; }
        }
        s_epr[i] = r;
        if (ep_last) as_global(p.ep_return)[gi] = r;
    };
    auto ep_tick_env = [&](int e, const int32_t *ev) {
        const int ge = e0 + e;
        int l = 0;
        if (op == OP_STEP && !ev[ENVI_SKIP]) {
            l = s_epl[e] + 1;
            if (ev[ENVI_DONE]) { as_global(p.ep_last_length)[ge] = l; atomicAdd(p.ep_count + ge, 1); l = 0; }
        }
        s_epl[e] = l;
        if (ep_last) as_global(p.ep_length)[ge] = l;
    };
    // action_mask_store (RW_STATS_BUILD kernels with RW_ACTION_MASK_ON): the valid-action byte of agent i of env e — the contract is at
    // RW_ACTION_MASK_ON in include/rware_hip.h — from the state the observation of this step is built from: the agent's own record, the
    // final per-cell layers (agent layer s_ga, shelf layer s_gs with every carried shelf under its carrier) and the highway bitmap.  Two
    // call sites, one writer per byte and launch: OS for the envs that stay (rware_phase_gather.h), RS for the envs this launch resets
    // (rware_phase_reset.h; OS skips those).  The occupant's load comes from its own record (s_carry), not from the agent layer's load
    // bit, which only the IMAGE gathers depend on.  All LDS reads unconditional (an off-map cell ahead reads the agent's own cell and is
    // masked).  Fused rollout: only the launch's last step stores (`ep_last`), nothing reads the earlier ones.
    auto action_mask_store = [&](int i, int e) {
        if (!ep_last) return;
        const int x = s_ax[i], y = s_ay[i], d = s_dir[i], carry = s_carry[i];
        const bool inside = d == DIR_UP ? y > 0 : d == DIR_DOWN ? y < H - 1 : d == DIR_LEFT ? x > 0 : x < W - 1;  // (Agent.req_location before clamping, :102-112)
        const int own = y * W + x;
        const int tc = e * HW + (inside ? own + (d == DIR_UP ? -W : d == DIR_DOWN ? W : d == DIR_LEFT ? -1 : 1) : own);
        const int ga_t = s_ga[tc] & 0x7f, gs_t = (int)s_gs[tc], gs_own = (int)s_gs[e * HW + own];
        const int occ = inside ? ga_t : 0;                        // the agent standing on the cell ahead, 1-based
        const int occ_carry = s_carry[e * N + (occ ? occ - 1 : 0)];
        const bool cancel = carry && gs_t != 0 && !(occ && occ_carry);  // a loaded agent in front of a standing shelf (:829-844)
        const bool fwd = inside && !cancel;
        const bool toggle = carry ? !on_highway(own) : gs_own != 0;    // unload off the highway (:893-895), load where a shelf stands (:889-892)
        const uint32_t m = 1u | 4u | 8u | ((fwd && !occ) ? 2u : 0u) | (toggle ? 16u : 0u) | ((fwd && occ) ? 32u : 0u);
        as_global(p.action_mask)[(size_t)e0 * N + i] = (uint8_t)m;
    };
#endif
