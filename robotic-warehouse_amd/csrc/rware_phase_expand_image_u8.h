// rware_phase_expand_image_u8.h — part of rw::rware_step_kernel (rware_kernels.h), included INSIDE the kernel body, RW_PACKED_BUILD only: STI8 — the image's bit string stored as BYTES, uint8 [B][N][C][2r+1][2r+1] (RW_OBS_IMAGE_U8, through RW_BUF_OBS)
// A textual unit, not a function: the phases share ~60 locals (LDS pointers, shapes, the agent lanes' registers), and every
// way of passing them that was tried — lambdas, always_inline or not — reschedules the kernels around it (round 5: +-10
// instructions per kernel, two 13/14-agent builds over a register cliff).  Splitting the text keeps every build's ISA.
    // ---------------------------------------------------------------- STI8: uint8 image rows, byte #g == bit #g of the string
    // Every element the float expansion writes is an integer in 0 .. 4 (six layers are 0 / 1, AGENT_DIRECTION holds dir + 1): the byte is
    // (uint8) of that float.  The destination is the launch's `obs` pointer, reinterpreted: uint8 [B][N][Limg], strides in BYTES.  A row is
    // Limg bytes — 27, 45, 63, ... — so a chunk of E envs (E % 4 == 0) is a multiple of 4 bytes and often not of 16 (5 agents x 27 bytes x
    // 4 envs = 540), and step t of a fused rollout starts t * B * N * Limg bytes into a caller's tape that may itself start anywhere: ANY
    // byte address.  The address is looked at per workgroup, at run time (workgroup-uniform), and picks the store width —
    //   16-byte aligned   16-byte pieces (16 bits of the string -> 16 bytes per lane), then the < 4 dwords and < 4 bytes they leave
    //   4-byte aligned    dword stores (4 bits -> 4 bytes, the float path's multiply), then the < 4 bytes they leave
    //   otherwise         byte stores
    if constexpr (kImage) {
    if (packed_on) {
        const int Limg = k_n_layers * CELLS;
        const int nb = nea * Limg;  // bytes of this chunk
        uint8_t *out8 = reinterpret_cast<uint8_t *>(la.obs) + (size_t)t * la.obs_stride + (size_t)e0 * N * Limg;
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(out8) & 15u);
        const int n16 = mis == 0 ? nb >> 4 : 0;        // whole 16-byte pieces stored as such
        const int n4 = (mis & 3u) == 0 ? nb >> 2 : 0;  // whole dwords stored as 16-byte pieces or dwords
        auto spread4 = [&](uint32_t nib) -> uint32_t { return (nib * 0x00204081u) & 0x01010101u; };  // 4 bits -> 4 bytes (0 / 1 each)
        if (worker) {
            // (AGENT_DIRECTION patches its cells afterwards: cached — the float rows' rule)
            const bool nt = (Cfg::kNT == 1 ? true : Cfg::kNT == 0 ? false : (k_nt != 0)) && !(k_transposed & 1);
            for (int q = tid; q < n16; q += TW) {
                const uint32_t h = (s_obits[q >> 1] >> ((q & 1) << 4)) & 0xFFFFu;
                u32x4 v;
                v.x = spread4(h & 0xFu);
                v.y = spread4((h >> 4) & 0xFu);
                v.z = spread4((h >> 8) & 0xFu);
                v.w = spread4(h >> 12);
                u32x4 *dst = reinterpret_cast<u32x4 *>(out8) + q;
                if (nt) store_u4_nt(dst, v); else store_u4(dst, v);
            }
            uint32_t *out32 = reinterpret_cast<uint32_t *>(out8);  // (dereferenced only where n4 > 0: a 4-byte aligned chunk)
            for (int d = (n16 << 2) + tid; d < n4; d += TW) out32[d] = spread4((s_obits[d >> 3] >> ((d & 7) << 2)) & 0xFu);
            for (int g = (n4 << 2) + tid; g < nb; g += TW) out8[g] = (uint8_t)((s_obits[g >> 5] >> (g & 31)) & 1u);
        }
        if (k_transposed & 1) {
            // AGENT_DIRECTION (:547-552): the marked cells hold dir + 1, not 1.  Patched after every 0/1 store of
            // the workgroup has completed (full barrier: vmcnt), one thread per (agent, image row) — the float rows' pass, storing a byte.
            dma_wait();
            __syncthreads();
            if (worker)
            for (int w = tid; w < nea * WIN; w += TW) {
                const int i = w / WIN, r = w - i * WIN;
                const int e = rw_div18(i, mN);
                const int ax = s_ax[i], ay = s_ay[i], d = k_directional ? s_dir[i] : DIR_UP;
                for (int cc = 0; cc < WIN; ++cc) {
                    int wr = r, wc = cc;
                    if (d == DIR_DOWN) { wr = WIN - 1 - r; wc = WIN - 1 - cc; }
                    else if (d == DIR_LEFT) { wr = WIN - 1 - cc; wc = r; }
                    else if (d == DIR_RIGHT) { wr = cc; wc = WIN - 1 - r; }
                    const int y = ay - R + wr, x = ax - R + wc;
                    if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H || x >= H || y >= W) continue;
                    const int ida = s_ga[e * HW + x * W + y] & 0x7f;
                    if (!ida) continue;
                    const uint8_t v = (uint8_t)(s_dir[e * N + ida - 1] + 1);
#pragma unroll
                    for (int l = 0; l < 8; ++l)
                        if (l < k_n_layers && k_layer[l] == LAYER_AGENT_DIRECTION) out8[(size_t)i * Limg + (l * WIN + r) * WIN + cc] = v;
                }
            }
        }
    }
    }
