// rware_phase_expand_packed.h — part of rw::rware_step_kernel (rware_kernels.h), included INSIDE the kernel body, RW_PACKED_BUILD only: STP — the bit string stored AS BITS, one uint32 row of PW words per agent (RW_OBS_PACKED / RW_BUF_OBS_PACKED)
// A textual unit, not a function: the phases share ~60 locals (LDS pointers, shapes, the agent lanes' registers), and every
// way of passing them that was tried — lambdas, always_inline or not — reschedules the kernels around it (round 5: +-10
// instructions per kernel, two 13/14-agent builds over a register cliff).  Splitting the text keeps every build's ISA.
    // ---------------------------------------------------------------- STP: packed rows, PW = 1 + ceil(L / 32) words per agent
    //   word 0        x | y << 16   (cell indices, whatever `normalised_coordinates` says)
    //   word 1 + w    bits [32 w, 32 w + 32) of the agent's row: bit k of the row == obs[k] != 0 for 2 <= k < L; bits 0, 1 (the
    //                 coordinate slots) are 0 in the bit string already, bits from L on belong to the next agent there and are masked
    // The row of agent i starts at bit i * L of the workgroup's string — any bit offset — so word w of it is a funnel shift over two
    // adjacent LDS words.  The destination is the launch's `obs` pointer, reinterpreted: uint32 [B][N][PW], strides in words.
    if (!kImage && packed_on) {  // (the IMAGE kernels: rware_phase_expand_image_u8.h)
        const int PW = 1 + OW;              // (OW == ceil(L / 32) for the FLATTENED kinds)
        const int nwd = nea * PW;           // words of this chunk
        uint32_t *pout = reinterpret_cast<uint32_t *>(obs_t) + (size_t)e0 * N * PW;
        // 16-byte stores where the chunk starts on a 16-byte boundary: a compile-time fact for the per-step launches of a build with chunks of
        // a multiple of 4 envs (every exact-shape build: they write the engine's own buffer), checked otherwise — a run-time geometry, and
        // every fused rollout, whose destination may be a caller's tape at any 4-byte offset; the rest is the scalar tail below
        constexpr bool kPackAligned = Cfg::kE != 0 && Cfg::kE % 4 == 0 && !kRollout;
        const int nq = (kPackAligned || (reinterpret_cast<uintptr_t>(pout) & 15u) == 0) ? nwd >> 2 : 0;
        const int tail_bits = L & 31;
        const uint32_t tail_mask = tail_bits ? (1u << tail_bits) - 1u : 0xFFFFFFFFu;
        // (s_xy holds x | y << 8: layouts wider or taller than 256 cells read the two coordinate arrays instead — workgroup-uniform)
        const bool xy_small = W <= 256 && H <= 256;
        // word g of the chunk from what was read for it: `lo`, `hi` the two LDS words under the row's 32-bit window, `xy` the agent's s_xy
        auto pword = [&](int i, int w, uint32_t lo, uint32_t hi, uint32_t xy) -> uint32_t {
            const uint32_t c = xy_small ? ((xy & 0xFFu) | ((xy >> 8) << 16)) : ((uint32_t)s_ax[i] | ((uint32_t)s_ay[i] << 16));
            const uint32_t b = funnel_shr(lo, hi, (uint32_t)(i * L) & 31u) & (w == PW - 1 ? tail_mask : 0xFFFFFFFFu);
            return w == 0 ? c : b;
        };
        // where the window of word (i, w) starts in the string (word 0 of a row reads the row's first window: unconditional reads)
        auto pwin = [&](int i, int w) -> int { return (i * L + 32 * (w > 0 ? w - 1 : 0)) >> 5; };
        auto store_rows = [&](auto nt) {
            // thread t takes 16-byte piece t, t + x_TW, ...; per piece 4 x (two window words + the agent's coordinates), read in ONE
            // unconditional batch (a window's second word may lie one word past the string: still inside the slack words of its LDS slot)
            for (int q = x_tid; q < nq; q += x_TW) {
                uint32_t lo[4], hi[4], xy[4];
                int iv[4], wv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int g = 4 * q + j;
                    iv[j] = g / PW;
                    wv[j] = g - iv[j] * PW;
                    const int wd = pwin(iv[j], wv[j]);
                    lo[j] = s_obits[wd];
                    hi[j] = s_obits[wd + 1];
                    xy[j] = (uint32_t)s_xy[iv[j]];
                }
                u32x4 v;
                v.x = pword(iv[0], wv[0], lo[0], hi[0], xy[0]);
                v.y = pword(iv[1], wv[1], lo[1], hi[1], xy[1]);
                v.z = pword(iv[2], wv[2], lo[2], hi[2], xy[2]);
                v.w = pword(iv[3], wv[3], lo[3], hi[3], xy[3]);
                u32x4 *dst = reinterpret_cast<u32x4 *>(pout) + q;
                if constexpr (decltype(nt)::value) store_u4_nt(dst, v); else store_u4(dst, v);
            }
        };
        if (x_worker) {
            // the non-temporal rule, as for the float rows: a build-time fact (Cfg::kNT) or Params::nt_obs; the fused rollouts store cached
            if constexpr (kRollout || Cfg::kNT == 0) store_rows(no_t{});
            else if constexpr (Cfg::kNT == 1) store_rows(yes_t{});
            else {
                if (k_nt) store_rows(yes_t{}); else store_rows(no_t{});
            }
            for (int g = (nq << 2) + x_tid; g < nwd; g += x_TW) {  // the words no 16-byte piece covers (an unaligned chunk: all of them)
                const int i = g / PW, w = g - i * PW, wd = pwin(i, w);
                pout[g] = pword(i, w, s_obits[wd], s_obits[wd + 1], (uint32_t)s_xy[i]);
            }
        }
    }
