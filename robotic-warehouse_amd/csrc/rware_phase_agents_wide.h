// rware_phase_agents_wide.h — part of rw::rware_step_kernel (rware_kernels.h), included INSIDE the kernel body: AG — the agent phases for 65 .. 127 agents: ONE wavefront per env, two agents per lane (generic kernels only)
// A textual unit like the other phase files.  rware_phase_agents_lds.h is the model: the same LDS arrays, the same sub-phases
// (R1, P1, P2a, P2b, P2c + P3, the set phase, P5, the hand-off) under wave_sync(), the same algorithm statement for statement.
// What differs: an env no longer fits the 64 lanes of a wavefront, so a wavefront takes one env at a time and lane l owns agent l
// (slot 0, always an agent: N > 64) and agent l + 64 (slot 1, an agent iff l + 64 < N).  A sub-phase is a lambda over one slot and
// runs for BOTH slots before the wave_sync() that closes it: what the 64-lane form gets from lockstep — every agent of the env has
// finished a sub-phase when the next one reads its results — holds here only across a sync.
// Registers: a slot carries FOUR values from sub-phase to sub-phase (WideSlot: named fields, two instances — nothing is indexed at run
// time); the agent's record (x, y, dir, load, delivered) is re-read from its LDS arrays where a sub-phase needs it, and everything that
// follows from the lane number is recomputed.  The generic kernels take their register count from their widest phase, for every shape
// they serve: kept in registers across the winner loops, two slots of the 64-lane form's fifteen values would be that phase.
    struct WideSlot {
        int a;        // the action, as the sub-phases cancel it
        int tg, nxt;  // target cell; the agent on it (-1 nobody, -2 the agent stays)
        int mv;       // P2b: lost its cell; from P3 on the hand-off word: st | tg << 16 for an agent that moved, else -1
    };
    for (int e = wave; e < ne; e += nw) {  // wave-uniform: one env per wavefront and turn
        const int base = e * N;
        CellT *gS = s_gs + e * HW;
        uint8_t *gA = s_ga + e * HW;
        int32_t *ev = s_envi + e * ENVI_W;
        const int ge = e0 + e;  // global env index
        const int ev_skip = ev[ENVI_SKIP], ev_reset = ev[ENVI_RESET];
        // (an idle slot — l + 64 >= N — addresses the env's agent 0 and writes nothing)
        auto mine_of = [&](int a_idx) RW_INLINE -> bool { return a_idx < N; };
        auto index_of = [&](int a_idx) RW_INLINE -> int { return base + (a_idx < N ? a_idx : 0); };
        auto stepping_of = [&](int a_idx) RW_INLINE -> bool { return (op == OP_STEP) && a_idx < N && !ev_skip; };
        WideSlot s0, s1;
        // ---- R1: the action; rebuild the agent layer (id | 0x80 if loaded: ids up to 127 fill the byte)
        auto r1 = [&](WideSlot &s, int a_idx) RW_INLINE {
            const int i = index_of(a_idx);
            const bool mine = mine_of(a_idx), stepping = stepping_of(a_idx);
            const int x = s_ax[i], y = s_ay[i], carry = s_carry[i];
            const int a_lds = (t == 0) ? s_act[i * AM] : (int)ACT_NOOP;
            s.a = ACT_NOOP;
            if (mine) {
                if (stepping) s.a = (t == 0) ? a_lds : act_t[((size_t)ge * N + a_idx) * AM];
                if (kMsg && stepping) {  // agent.message[:] = action[1:] — for every agent, whatever its move does (:812)
                    int msg = 0;
                    for (int k = 0; k < M; ++k) {
                        const int v = (t == 0) ? s_act[i * AM + 1 + k] : act_t[((size_t)ge * N + a_idx) * AM + 1 + k];
                        if ((unsigned)v > 1u) atomicOr(p.status, STATUS_INVALID_ACTION);  // MultiDiscrete([5, 2, 2, ...])
                        msg |= (v & 1) << k;
                    }
                    s_msg[i] = msg;
                }
            }
            if (mine && !ev_reset) gA[y * W + x] = (uint8_t)((a_idx + 1) | (carry ? 0x80 : 0));
        };
        r1(s0, lane);
        r1(s1, lane + 64);
        wave_sync();
        // ------------------------------------------------------------ P1: intent (:825-846)
        auto p1 = [&](WideSlot &s, int a_idx) RW_INLINE {
            const int i = index_of(a_idx);
            const int x = s_ax[i], y = s_ay[i], d = s_dir[i], carry = s_carry[i], st = y * W + x;
            s.tg = st; s.nxt = -2;
            if (stepping_of(a_idx)) {
                if ((unsigned)s.a > 4u) {  // Action(a) raises in the reference (:814); flagged, runs as NOOP
                    atomicOr(p.status, STATUS_INVALID_ACTION);
                    s.a = ACT_NOOP;
                }
                const int fwd = (s.a == ACT_FORWARD) ? 1 : 0;
                const int dx = fwd & ((d == DIR_RIGHT) ? 1 : 0), dxn = fwd & ((d == DIR_LEFT) ? 1 : 0);
                const int dy = fwd & ((d == DIR_DOWN) ? 1 : 0), dyn = fwd & ((d == DIR_UP) ? 1 : 0);
                const int tx = min(max(x + dx - dxn, 0), W - 1);  // clamped at the walls (:105-112)
                const int ty = min(max(y + dy - dyn, 0), H - 1);
                int tg = ty * W + tx;
                const int sh_tg = gS[tg], ag_tg = gA[tg];
                // a standing shelf blocks a loaded agent (:836-846)
                const bool blocked = (carry != 0) & (tg != st) & (sh_tg != 0) & ((ag_tg & 0x80) == 0);
                s.a = blocked ? (int)ACT_NOOP : s.a;
                tg = blocked ? st : tg;
                // successor on the chain: agent index on the target cell, -1 empty, -2 == i is stationary
                s.nxt = (tg == st) ? -2 : ((ag_tg & 0x7f) - 1);
                s.tg = tg;
                s_tgt[i] = (s.nxt == -2) ? -1 : tg;  // contested-cell key: only movers compete
                s_nxt[i] = s.nxt;
            }
        };
        p1(s0, lane);
        p1(s1, lane + 64);
        wave_sync();
        // (no chain in the env — over BOTH slots: P2a, the depth reads and the s_win exchange drop out, as in the 64-lane form)
        const bool chains = wave_any((stepping_of(lane) && s0.nxt >= 0) || (stepping_of(lane + 64) && s1.nxt >= 0));  // wave-uniform
        // ------------------------------------------------------------ P2a: follower depth
        if (chains) {
            auto p2a = [&](const WideSlot &s, int a_idx) RW_INLINE {
                if (stepping_of(a_idx) && s.nxt >= 0) {
                    int j = s.nxt, dd = 1;
                    while (j >= 0 && j != a_idx && dd <= N && s_nxt[base + j] != -2) {
                        atomicMax(&s_depth[base + j], dd);
                        j = s_nxt[base + j];
                        ++dd;
                    }
                }
            };
            p2a(s0, lane);
            p2a(s1, lane + 64);
            wave_sync();
        }
        // ------------------------------------------------------------ P2b: winner per contested cell
        auto p2b = [&](WideSlot &s, int a_idx) RW_INLINE {
            const int i = index_of(a_idx);
            const bool stepping = stepping_of(a_idx);
            int lose = 0;  // larger follower depth wins, then the LOWER agent id
            if (stepping && s.nxt != -2) {
                if (chains) {
                    const int dme = s_depth[i];
                    for (int k = 0; k < N; ++k) {  // (bitwise on purpose: no short-circuit branches)
                        const int tk = s_tgt[base + k], dk = s_depth[base + k];
                        lose |= ((tk == s.tg) & (k != a_idx) & ((dk > dme) | ((dk == dme) & (k < a_idx)))) ? 1 : 0;
                    }
                } else {
                    for (int k = 0; k < N; ++k) lose |= ((s_tgt[base + k] == s.tg) & (k < a_idx)) ? 1 : 0;
                }
            }
            s.mv = lose;
            if (chains && stepping) s_win[i] = lose ^ 1;
        };
        p2b(s0, lane);
        p2b(s1, lane + 64);
        if (chains) wave_sync();
        // ------------------------------------------------------------ P2c + P3: commit, apply (:871-899); the clear phase
        auto p3 = [&](WideSlot &s, int a_idx) RW_INLINE {
            const int i = index_of(a_idx);
            const int lose = s.mv;
            float rew = 0.0f;
            s.mv = -1;
            if (stepping_of(a_idx)) {
                int x = s_ax[i], y = s_ay[i], d = s_dir[i], carry = s_carry[i], deliv = s_deliv[i];
                const int st = y * W + x, tg = s.tg;
                const int shelf_here = gS[st];  // (only the agent on a cell clears that cell's shelf, below: still the start-of-step value)
                int a = s.a;
                if (s.nxt == -1) {  // drains into an empty cell: commits iff it won the cell
                    if (lose) a = ACT_NOOP;
                } else if (s.nxt >= 0) {  // walk the chain ahead
                    int j = a_idx, hops = 0, ok = 1, commit = 0;
                    for (;;) {
                        ok &= s_win[base + j];
                        const int nj = s_nxt[base + j];
                        ++hops;
                        if (nj == -1) { commit = ok; break; }              // drains into an empty cell
                        if (nj == a_idx) { commit = (hops >= 3); break; }  // a cycle through me; 2-swap refused
                        if (s_nxt[base + nj] == -2) break;                 // blocked by a stationary agent
                        if (hops >= N) break;                              // feeds a cycle it is not part of
                        j = nj;
                    }
                    if (!commit) a = ACT_NOOP;
                }
                const bool moved = (a == ACT_FORWARD) & (tg != st);
                if (moved) {  // (an agent that moved was not clamped at a wall: its target is the neighbour cell)
                    const int ty = (d == DIR_DOWN) ? y + 1 : (d == DIR_UP) ? y - 1 : y;
                    x = tg - ty * W;
                    y = ty;
                    gA[st] = 0;  // clear phase of the incremental _recalc_grid
                    if (carry) gS[st] = 0;
                    s.mv = st | (tg << 16);
                }
                // wraplist [UP, RIGHT, DOWN, LEFT] (:119): RIGHT 0->3->1->2->0, LEFT 0->2->1->3->0
                const int right = (0x1023 >> (4 * d)) & 0xF;  // d: 0->3, 1->2, 2->0, 3->1
                const int left = (0x0132 >> (4 * d)) & 0xF;   // d: 0->2, 1->3, 2->1, 3->0
                d = (a == ACT_RIGHT) ? right : ((a == ACT_LEFT) ? left : d);
                // TOGGLE_LOAD (:886-899): pick up the shelf under the agent, or put the carried one down off the highways
                const bool toggle = (a == ACT_TOGGLE);
                const bool drop = toggle & (carry != 0) & !on_highway(st);
                const bool pick = toggle & (carry == 0) & (shelf_here != 0);
                rew = (drop & (deliv != 0) & (k_reward_type == REW_TWO_STAGE)) ? 0.5f : 0.0f;
                deliv = drop ? 0 : deliv;
                carry = drop ? 0 : (pick ? shelf_here : carry);
                s_ax[i] = x; s_ay[i] = y; s_dir[i] = d; s_carry[i] = carry; s_deliv[i] = deliv;
            }
            if (mine_of(a_idx)) s_rew[i] = rew;  // every agent of the chunk gets its reward slot
        };
        p3(s0, lane);
        p3(s1, lane + 64);
        wave_sync();  // every mover of the env has cleared the cell it left ...
        auto set_phase = [&](const WideSlot &s, int a_idx) RW_INLINE {  // ... before anybody marks the cell it stands on now (also the loaded flag after a pick-up / drop)
            if (stepping_of(a_idx)) {
                const int i = index_of(a_idx);
                const int cell = s_ay[i] * W + s_ax[i], carry = s_carry[i];  // (its own stores of P3: the target cell if it moved)
                gA[cell] = (uint8_t)((a_idx + 1) | (carry ? 0x80 : 0));
                if (s.mv >= 0 && carry) gS[cell] = (CellT)carry;
            }
        };
        set_phase(s0, lane);
        set_phase(s1, lane + 64);
        wave_sync();
        // ------------------------------------------------------------ P5: goals, rewards, termination — once per env (agent 0: slot 0 of lane 0)
        if (stepping_of(lane) && lane == 0) {
            goals_and_termination(e, ge, base, ev, gS, gA);
        }
        wave_sync();
        // ------------------------------------------------------------ hand-off to the write-back roles
        const int ev_reset_now = ev[ENVI_RESET];
        auto hand_off = [&](const WideSlot &s, int a_idx) RW_INLINE {
            if (!mine_of(a_idx)) return;
            s_mv[index_of(a_idx)] = s.mv;  // which two cells changed
            if (!ev_reset_now)  // requested-shelf bitmap of the (post-step) queue; RS builds it for reset envs
                for (int k = a_idx; k < Q; k += N) {  // (a_idx runs over 0 .. N - 1 across the two slots: the queue once)
                    const int sid = s_queue[e * Q + k];
                    atomicOr(&s_req[e * SW + (sid >> 5)], 1u << (sid & 31));
                }
        };
        hand_off(s0, lane);
        hand_off(s1, lane + 64);
    }
