// The critic's global state on the device: rw_global_image, rw_global_records, rw_global_image_gather (include/rware_hip.h,
// include/rware_hip_global_state.h).  Included by rware_capi.hip at file scope, after rware_kernels.h (rec_cell / rec_dir / rec_carry,
// u32x4, store_u4_nt, store_f4_nt, STATUS_*, LAYER_*), after rware_minibatch.h (gather_index_args) and after the engine
// internals the host part at the end uses (rw_engine, fail, RW_HIP).  The kernels first, the host part below them.  Plain C++ throughout:
// the host-thread build of tests/emu compiles this file as it is, so the 16-bit element types are written as bit patterns.
//
// Warehouse.get_global_image (rware/warehouse.py:966-1040) is a pure function of ONE code byte per cell,
//     bit 0 shelf | bit 1 requested | bit 2 agent | bit 3 goal | bit 4 AGENT_LOAD | bits 5..7 AGENT_DIRECTION (dir + 1),
// the last two on the MIRRORED cell (the reference writes `layer[ag.x, ag.y]` on an (H, W) array, :1003, :1008): an agent at x >= H or
// y >= W writes nothing there (the reference raises IndexError), "a later agent overwrites an earlier one" is an LDS atomicMax of
// (agent index << 3 | dir + 1).  The work has two halves, each a __device__ function over a workgroup's LDS:
//     global_image_build    the state the step kernels keep (shelf shadow, packed agent records, queue) -> the code bytes of `ne` envs
//     global_image_expand   code bytes -> the workgroup's slice of [n][C'][H'][W']: every output element looks up the byte of the cell
//                           it shows (zero in the padding) and takes its layer's bits out of it, so no store can leave the slice.  A pure
//                           store stream: 16-byte non-temporal stores on the 16-byte boundaries of the ADDRESS (`phase`: the element
//                           index of `out` within its 16-byte line), single elements in front of the first and behind the last boundary
// and three kernels:
//     rware_global_image_kernel          build + expand                                        (rw_global_image, as before the split)
//     rware_global_records_kernel        build with both transposed layers and the flags byte, then 16-byte stores of the records
//     rware_global_image_gather_kernel   records by index into LDS with 16-byte loads, then expand; float32, uint8, float16, bfloat16
// The record of one env is uint8 [RB], RB = (H*W + 1 + 15) & ~15: the H*W code bytes, the flags byte (bit 0: some agent has no
// mirrored cell, bit 1: some CARRYING agent has none), zeros.  No thread returns before its kernel's last barrier.
#pragma once

namespace rw {

struct GlobalImageArgs {
    int32_t B, H, W, HW, N, Q, S, SW, n_goals;   // B: envs (gather: output images)
    int32_t E;                       // envs per workgroup
    int32_t n_layers, Cp, Hp, Wp;    // layers asked for; the padded shape
    int32_t c0, h0, w0;              // zero padding in front, per axis (:1029)
    int32_t phase;                   // (address of out / element size) % (16 / element size)
    int32_t de, dch, dy, dx;         // blockDim.x 16-byte pieces further on in [env][C'][H'][W'] — that many elements, decomposed
    uint32_t layers;                 // 4 bits per channel: its rw_image_layer
    uint32_t transposed;             // bit 0: AGENT_DIRECTION among the layers, bit 1: AGENT_LOAD
};

// the 16-bit element types: integers 0 .. 7 as bit patterns (every image value is an integer in 0 .. 4, exact in both)
struct F16Bits { uint16_t v; };
struct BF16Bits { uint16_t v; };
enum : uint32_t { GLOBAL_CODE_NO_RECORD = 0xFFu };   // (gather, in LDS only) the cells of an image whose index is out of range: no code
                                                     // byte is above 0x9F — direction + 1 is at most 4
enum : int { RECORD_FLAG_NO_MIRROR = 1, RECORD_FLAG_LOADED_NO_MIRROR = 2 };

template <typename ElemT>
__device__ __forceinline__ uint32_t global_image_elem16(uint32_t v) {   // v in 0 .. 7
    if constexpr (std::is_same<ElemT, F16Bits>::value) {
        // 0, 1, 2, 3, 4, 5, 6, 7 in float16: 0x0000 0x3C00 0x4000 0x4200 0x4400 0x4500 0x4600 0x4700 — the high bytes, one per value
        return (uint32_t)((0x4746454442403C00ull >> (8u * v)) & 0xFFu) << 8;
    } else {
        float f = (float)v;
        uint32_t u;
        __builtin_memcpy(&u, &f, 4);
        return u >> 16;              // (three mantissa bits at most: the upper half of the float32 is the bfloat16)
    }
}
template <typename ElemT>
__device__ __forceinline__ void global_image_put(ElemT *o, uint32_t v) {
    if constexpr (sizeof(ElemT) == 2) o->v = (uint16_t)global_image_elem16<ElemT>(v);
    else *o = (ElemT)v;
}

// s_lut [8], by the first eight threads: layer -> where its value sits in the code byte — SHELVES bit 0, REQUESTS 1, AGENTS 2,
// AGENT_DIRECTION bits 5..7, AGENT_LOAD 4, GOALS 3, ACCESSIBLE bit 2 inverted —, per channel shift | mask << 8 | xor << 16; a channel
// beyond the list (padding) reads 0 through a zero mask
__device__ __forceinline__ void global_image_lut(uint32_t *s_lut, int tid, const GlobalImageArgs &a) {
    if (tid < 8) {
        const uint32_t l = (a.layers >> (4 * tid)) & 15u;
        const uint32_t sh = (0x2345210u >> (4 * l)) & 15u, mask = l == (uint32_t)LAYER_AGENT_DIRECTION ? 7u : 1u;
        s_lut[tid] = tid < a.n_layers ? sh | mask << 8 | (l == (uint32_t)LAYER_ACCESSIBLE ? 1u : 0u) << 16 : 0u;
    }
}

// ---- build: state -> code bytes -------------------------------------------------------------------------------------------------
// s_zero / n_zero: the workgroup's LDS behind the table, s_req [E][SW] | s_mir [E][HW] | s_codew [E][CQ] in any order (CQ words of code
// per env, >= ceil(HW / 4)), zeroed here; s_lut [8] or nullptr.  RECORD: both transposed layers whatever `transposed` says, the two
// flags into byte HW of the env's code words instead of STATUS_IMAGE_INDEX into `status`.  Ends behind a barrier.
template <typename CellT, bool RECORD>
__device__ __forceinline__ void global_image_build(const CellT *__restrict__ shadow, const uint32_t *__restrict__ rec,
                                                   const int32_t *__restrict__ queue, const int32_t *__restrict__ goal_cells, int32_t *status,
                                                   uint32_t *s_lut, uint32_t *s_zero, int n_zero, uint32_t *s_req, int *s_mir,
                                                   uint32_t *s_codew, int CQ, int e0, int ne, const GlobalImageArgs &a) {
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int HW = a.HW;
    const uint32_t transposed = RECORD ? 3u : a.transposed;
    uint8_t *const s_code = reinterpret_cast<uint8_t *>(s_codew);
    for (int i = tid; i < n_zero; i += nt) s_zero[i] = 0u;
    if (s_lut) global_image_lut(s_lut, tid, a);
    __syncthreads();
    for (int idx = tid; idx < ne * a.Q; idx += nt) {
        const int e = idx / a.Q, s = queue[(size_t)e0 * a.Q + idx];
        if (s > 0 && s <= a.S) atomicOr(&s_req[e * a.SW + (s >> 5)], 1u << (s & 31));
    }
    for (int idx = tid; idx < ne * a.n_goals; idx += nt) {
        const int e = idx / a.n_goals, c = goal_cells[idx - e * a.n_goals];
        if ((unsigned)c < (unsigned)HW) atomicOr(&s_codew[e * CQ + (c >> 2)], 8u << (8 * (c & 3)));
    }
    for (int idx = tid; idx < ne * a.N; idx += nt) {
        const int e = idx / a.N, i = idx - e * a.N;
        const uint32_t r = rec[(size_t)e0 * a.N + idx];
        const int c = rec_cell(r);
        if (c >= HW) continue;  // (no state the engine produces; a record written from outside could say so)
        atomicOr(&s_codew[e * CQ + (c >> 2)], 4u << (8 * (c & 3)));
        if (transposed) {
            const int y = c / a.W, x = c - y * a.W;
            const bool inside = x < a.H && y < a.W;   // `layer[ag.x, ag.y]`: row x of H, column y of W
            const int m = x * a.W + y;
            const bool loaded = (transposed & 2u) && rec_carry(r) > 0;
            if (inside) {
                if (transposed & 1u) atomicMax(&s_mir[e * HW + m], i << 3 | (rec_dir(r) + 1));
                if (loaded) atomicOr(&s_codew[e * CQ + (m >> 2)], 16u << (8 * (m & 3)));
            } else if constexpr (RECORD) {
                const uint32_t f = (uint32_t)RECORD_FLAG_NO_MIRROR | (loaded ? (uint32_t)RECORD_FLAG_LOADED_NO_MIRROR : 0u);
                atomicOr(&s_codew[e * CQ + (HW >> 2)], f << (8 * (HW & 3)));
            } else if ((transposed & 1u) || loaded) {
                atomicOr(status, (int)STATUS_IMAGE_INDEX);
            }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < ne * HW; idx += nt) {  // (every thread owns the bytes it rewrites)
        const int e = idx / HW, c = idx - e * HW;
        const uint32_t s = (uint32_t)shadow[(size_t)e0 * HW + idx];
        uint32_t code = s_code[e * CQ * 4 + c] | ((uint32_t)s_mir[e * HW + c] & 7u) << 5;
        if (s) code |= 1u | (s <= (uint32_t)a.S && ((s_req[e * a.SW + (s >> 5)] >> (s & 31)) & 1u) ? 2u : 0u);
        s_code[e * CQ * 4 + c] = (uint8_t)code;
    }
    __syncthreads();
}

// ---- expand: code bytes -> the workgroup's slice of the output ----------------------------------------------------------------------
// s_code: [ne][code_stride] bytes, cell c of env e at e * code_stride + c.  GATHER: a cell that holds GLOBAL_CODE_NO_RECORD reads 0 in
// every layer (ACCESSIBLE included).  The slice: n = ne * C'H'W' elements from element e0 * C'H'W' of `out` (host-checked:
// E * C' H' W' < 2^31).  All four element types take the same path: 16 bytes a store, 4, 16 or 8 elements of them.
template <typename ElemT, bool GATHER>
__device__ __forceinline__ void global_image_expand(const uint32_t *s_lut, const uint8_t *s_code, int code_stride, int e0, int ne,
                                                    ElemT *__restrict__ out, const GlobalImageArgs &a) {
    constexpr int VE = 16 / (int)sizeof(ElemT);  // elements of a 16-byte store
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int HpWp = a.Hp * a.Wp, CHW = a.Cp * HpWp, n = ne * CHW;
    const size_t g0 = (size_t)e0 * (size_t)CHW;
    ElemT *const o = out + g0;
    int head = (VE - (int)(((size_t)a.phase + g0) % VE)) % VE;  // elements in front of the slice's first 16-byte boundary
    if (head > n) head = n;
    const int nv = (n - head) / VE, tail = head + nv * VE;
    struct Pos { int e, ch, y, x; };
    auto pos_of = [&](int l) -> Pos {
        Pos p;
        p.e = l / CHW;
        const int r = l - p.e * CHW;
        p.ch = r / HpWp;
        const int r2 = r - p.ch * HpWp;
        p.y = r2 / a.Wp;
        p.x = r2 - p.y * a.Wp;
        return p;
    };
    auto value = [&](const Pos &p) -> uint32_t {
        const unsigned ch = (unsigned)(p.ch - a.c0), y = (unsigned)(p.y - a.h0), x = (unsigned)(p.x - a.w0);
        if (ch >= (unsigned)a.n_layers || y >= (unsigned)a.H || x >= (unsigned)a.W) return 0u;
        const uint32_t t = s_lut[ch], code = s_code[p.e * code_stride + (int)(y * (unsigned)a.W + x)];
        if (GATHER && code == (uint32_t)GLOBAL_CODE_NO_RECORD) return 0u;
        return ((code >> (t & 255u)) & ((t >> 8) & 255u)) ^ (t >> 16);
    };
    auto next = [&](Pos &p) {
        if (++p.x == a.Wp) {
            p.x = 0;
            if (++p.y == a.Hp) {
                p.y = 0;
                if (++p.ch == a.Cp) { p.ch = 0; ++p.e; }
            }
        }
    };
    // (a thread's 16-byte pieces lie blockDim.x * VE elements apart: it decomposes the first one's index and steps on by that
    //  distance as the host decomposed it — three integer divisions per thread instead of per piece)
    auto advance = [&](Pos &p) {
        p.x += a.dx; if (p.x >= a.Wp) { p.x -= a.Wp; ++p.y; }
        p.y += a.dy; if (p.y >= a.Hp) { p.y -= a.Hp; ++p.ch; }
        p.ch += a.dch; if (p.ch >= a.Cp) { p.ch -= a.Cp; ++p.e; }
        p.e += a.de;
    };
    Pos first = pos_of(head + (tid < nv ? tid : 0) * VE);
    for (int v = tid; v < nv; v += nt, advance(first)) {
        const int l = head + v * VE;
        Pos p = first;
        if constexpr (sizeof(ElemT) == 4) {
            float4 f;
            f.x = (float)value(p); next(p);
            f.y = (float)value(p); next(p);
            f.z = (float)value(p); next(p);
            f.w = (float)value(p);
            store_f4_nt(reinterpret_cast<float4 *>(o + l), f);
        } else if constexpr (sizeof(ElemT) == 2) {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t lo = global_image_elem16<ElemT>(value(p)); next(p);
                const uint32_t hi = global_image_elem16<ElemT>(value(p)); next(p);
                w[k] = lo | hi << 16;
            }
            store_u4_nt(reinterpret_cast<u32x4 *>(o + l), u32x4{w[0], w[1], w[2], w[3]});
        } else {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t acc = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc |= value(p) << (8 * j); next(p); }
                w[k] = acc;
            }
            store_u4_nt(reinterpret_cast<u32x4 *>(o + l), u32x4{w[0], w[1], w[2], w[3]});
        }
    }
    for (int k = tid; k < head + (n - tail); k += nt) {
        const int l = k < head ? k : tail + (k - head);
        global_image_put(o + l, value(pos_of(l)));
    }
}

// ---- rw_global_image: build + expand; a workgroup takes `E` consecutive envs -----------------------------------------------------
template <typename CellT, typename ElemT>
__global__ void __launch_bounds__(256) rware_global_image_kernel(const CellT *__restrict__ shadow, const uint32_t *__restrict__ rec,
                                                                  const int32_t *__restrict__ queue, const int32_t *__restrict__ goal_cells,
                                                                  int32_t *status, ElemT *__restrict__ out, const GlobalImageArgs a) {
    extern __shared__ __align__(16) int32_t smem[];
    const int e0 = (int)blockIdx.x * a.E;
    const int ne = a.B - e0 < a.E ? a.B - e0 : a.E;  // (the last workgroup may be ragged; the launch has ceil(B / E) of them: ne >= 1)
    const int HW = a.HW, HWQ = (HW + 3) >> 2;         // code words per env: one byte per cell
    uint32_t *const s_lut = reinterpret_cast<uint32_t *>(smem);                 // [8]       per channel: shift | mask << 8 | xor << 16
    uint32_t *const s_req = s_lut + 8;                                          // [E][SW]   bit s: shelf id s is in the queue
    int *const s_mir = reinterpret_cast<int *>(s_req + a.E * a.SW);             // [E][HW]   agent index << 3 | dir + 1, on the mirrored cell
    uint32_t *const s_codew = reinterpret_cast<uint32_t *>(s_mir + a.E * HW);   // [E][HWQ]  the code bytes, as words for the atomics
    global_image_build<CellT, false>(shadow, rec, queue, goal_cells, status, s_lut, s_req, a.E * (a.SW + HW + HWQ), s_req, s_mir, s_codew,
                                     HWQ, e0, ne, a);
    global_image_expand<ElemT, false>(s_lut, reinterpret_cast<const uint8_t *>(s_codew), HWQ * 4, e0, ne, out, a);
}

// ---- rw_global_records: build, flags, 16-byte stores ------------------------------------------------------------------------------
// LDS: s_codew [E][RB / 4] first (16-byte aligned: the records leave as whole u32x4), then s_req [E][SW], s_mir [E][HW].  The
// workgroup's records are RB * ne consecutive bytes of LDS and of `records` (16-byte aligned, host-checked); the zeroed LDS behind
// byte HW of each record is its zero tail.  `a`: B, H, W, HW, N, Q, S, SW, n_goals, E only.
template <typename CellT>
__global__ void __launch_bounds__(256) rware_global_records_kernel(const CellT *__restrict__ shadow, const uint32_t *__restrict__ rec,
                                                                    const int32_t *__restrict__ queue, const int32_t *__restrict__ goal_cells,
                                                                    uint8_t *__restrict__ records, const int RB, const GlobalImageArgs a) {
    extern __shared__ __align__(16) int32_t smem[];
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int e0 = (int)blockIdx.x * a.E;
    const int ne = a.B - e0 < a.E ? a.B - e0 : a.E;
    const int CQ = RB >> 2;
    uint32_t *const s_codew = reinterpret_cast<uint32_t *>(smem);
    uint32_t *const s_req = s_codew + a.E * CQ;
    int *const s_mir = reinterpret_cast<int *>(s_req + a.E * a.SW);
    global_image_build<CellT, true>(shadow, rec, queue, goal_cells, nullptr, nullptr, s_codew, a.E * (CQ + a.SW + a.HW), s_req, s_mir, s_codew,
                                    CQ, e0, ne, a);
    const u32x4 *const src = reinterpret_cast<const u32x4 *>(s_codew);
    u32x4 *const dst = reinterpret_cast<u32x4 *>(records + (size_t)e0 * (size_t)RB);
    for (int q = tid; q < ne * (RB >> 4); q += nt) store_u4_nt(dst + q, src[q]);
}

// ---- rw_global_image_gather: records by index -> LDS, then expand --------------------------------------------------------------------
// A workgroup takes `E` consecutive OUTPUT images.  LDS: s_lut [8] | s_code [E][RB] (16-byte aligned) | s_src int64 [E].  The index is
// read once per image; an index outside 0 .. n_records-1 reads no record: its cells become GLOBAL_CODE_NO_RECORD (an all-zero image)
// and the status word gets STATUS_RESTORE_INDEX.  A gathered record whose flags byte says that a requested transposed layer had an
// agent without a mirrored cell sets STATUS_IMAGE_INDEX, as rw_global_image does for that state.
struct GlobalGatherArgs {
    const uint8_t *records;   // [n_records][RB], 16-byte aligned
    const void *index;        // [a.B] int32 or int64 (index64), NULL: the identity
    int64_t n_records;
    int32_t RB, index64;
};
template <typename ElemT>
__global__ void __launch_bounds__(256) rware_global_image_gather_kernel(const GlobalGatherArgs g, int32_t *status, ElemT *__restrict__ out,
                                                                         const GlobalImageArgs a) {
    extern __shared__ __align__(16) int32_t smem[];
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int e0 = (int)blockIdx.x * a.E;
    const int ne = a.B - e0 < a.E ? a.B - e0 : a.E;
    const int RB = g.RB, RQ = RB >> 4;
    uint32_t *const s_lut = reinterpret_cast<uint32_t *>(smem);
    u32x4 *const s_rec = reinterpret_cast<u32x4 *>(smem + 8);
    const uint8_t *const s_code = reinterpret_cast<const uint8_t *>(s_rec);
    int64_t *const s_src = reinterpret_cast<int64_t *>(smem + 8 + a.E * (RB >> 2));
    global_image_lut(s_lut, tid, a);
    for (int e = tid; e < ne; e += nt) {   // (as rw::gather_source of rware_minibatch.h, the identity range-checked too)
        const size_t i = (size_t)e0 + (size_t)e;
        int64_t j = !g.index ? (int64_t)i : g.index64 ? static_cast<const int64_t *>(g.index)[i] : (int64_t)static_cast<const int32_t *>(g.index)[i];
        if (j < 0 || j >= g.n_records) {
            atomicOr(status, (int)STATUS_RESTORE_INDEX);
            j = -1;
        }
        s_src[e] = j;
    }
    __syncthreads();
    for (int q = tid; q < ne * RQ; q += nt) {
        const int e = q / RQ, part = q - e * RQ;
        const int64_t j = s_src[e];
        u32x4 v = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (j >= 0) v = *reinterpret_cast<const u32x4 *>(g.records + (size_t)j * (size_t)RB + (size_t)part * 16u);
        s_rec[q] = v;
    }
    __syncthreads();
    if (a.transposed)
        for (int e = tid; e < ne; e += nt)
            if (s_src[e] >= 0 && ((uint32_t)s_code[e * RB + a.HW] & a.transposed)) atomicOr(status, (int)STATUS_IMAGE_INDEX);
    global_image_expand<ElemT, true>(s_lut, s_code, RB, e0, ne, out, a);
}

}  // namespace rw

// ---- host part ----------------------------------------------------------------------------------------------------------------------

// What rw_global_image and rw_global_image_gather share: the layer list, the padded shape and the element's alignment, checked and
// written into `a` (layers, transposed, n_layers, the padded shape and its offsets, phase); `chw`: elements per image.
static int global_image_plan(rw_engine *eng, const char *who, const int32_t *layers, int32_t n_layers, const int32_t *pad_to_shape,
                             size_t esize, const void *out_dev, rw::GlobalImageArgs &a, uint64_t &chw) {
    const rw::Params &p = eng->prm;
    for (int l = 0; l < n_layers; ++l) {
        const int v = layers[l];
        if (v < RW_LAYER_SHELVES || v > RW_LAYER_ACCESSIBLE)  // (the reference: ValueError, rware/warehouse.py:1018)
            return fail(eng, RW_ERR_INVALID_ARG, "%s: unknown image layer %d", who, v);
        a.layers |= (uint32_t)v << (4 * l);
        a.transposed |= v == RW_LAYER_AGENT_DIRECTION ? 1u : v == RW_LAYER_AGENT_LOAD ? 2u : 0u;
    }
    const int shape[3] = {n_layers, p.H, p.W};
    int padded[3], before[3];
    for (int k = 0; k < 3; ++k) {
        padded[k] = pad_to_shape ? pad_to_shape[k] : shape[k];
        if (padded[k] < shape[k])  // (the reference: AssertionError, :1028)
            return fail(eng, RW_ERR_INVALID_ARG, "%s: pad_to_shape[%d] = %d is smaller than the image's %d", who, k, padded[k], shape[k]);
        before[k] = (padded[k] - shape[k]) / 2;
    }
    chw = (uint64_t)padded[0] * (uint64_t)padded[1] * (uint64_t)padded[2];  // (three factors below 2^31: no overflow)
    if (chw > (1ull << 30))
        return fail(eng, RW_ERR_INVALID_ARG, "%s: %llu elements per env are more than one launch holds; slice it (smaller "
                    "padding, or fewer layers per call)", who, (unsigned long long)chw);
    const uintptr_t addr = reinterpret_cast<uintptr_t>(out_dev);
    if (addr % esize) return fail(eng, RW_ERR_INVALID_ARG, "%s: a %s out_dev has to be %d-byte aligned", who, esize == 4 ? "float32" : "16-bit", (int)esize);
    a.H = p.H; a.W = p.W; a.HW = p.HW; a.N = p.N; a.Q = p.Q; a.S = p.S; a.SW = p.SW; a.n_goals = p.n_goals;
    a.n_layers = n_layers; a.Cp = padded[0]; a.Hp = padded[1]; a.Wp = padded[2];
    a.c0 = before[0]; a.h0 = before[1]; a.w0 = before[2];
    a.phase = (int32_t)((addr / esize) % (16 / esize));
    return RW_OK;
}
// ... and the distance between two 16-byte pieces of one thread, decomposed over [env][C'][H'][W']
static void global_image_stride(rw::GlobalImageArgs &a, unsigned threads, size_t esize, uint64_t chw) {
    const uint64_t plane = (uint64_t)a.Hp * (uint64_t)a.Wp;
    const uint64_t stride = (uint64_t)threads * (16 / esize), in_env = stride % chw, in_plane = in_env % plane;
    a.de = (int32_t)(stride / chw); a.dch = (int32_t)(in_env / plane);
    a.dy = (int32_t)(in_plane / a.Wp); a.dx = (int32_t)(in_plane % a.Wp);
}
// the goal cells as the build half reads them: out of the engine's device copy of its parameters
static const int32_t *goal_cells_dev(const rw_engine *eng) { return reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(eng->d_prm) + offsetof(rw::Params, goal_cells)); }

extern "C" {

int rw_global_image(rw_engine *eng, const int32_t *layers, int32_t n_layers, const int32_t *pad_to_shape, int32_t elem, void *out_dev) {
    // One launch of rware_global_image_kernel on the engine's stream and nothing else: everything the kernel needs beyond the state
    // travels in its arguments, so the call is legal inside a stream capture and is replayed with the graph.
    if (!eng) return RW_ERR_INVALID_ARG;
    if (!layers || !out_dev) return fail(eng, RW_ERR_INVALID_ARG, "rw_global_image: NULL %s", !layers ? "layers" : "out_dev");
    if (n_layers < 1 || n_layers > rw::MAX_IMAGE_LAYERS) return fail(eng, RW_ERR_INVALID_ARG, "rw_global_image: n_layers %d not in 1..8", n_layers);
    if (elem != 0 && elem != 1) return fail(eng, RW_ERR_INVALID_ARG, "rw_global_image: elem %d is neither 0 (float32) nor 1 (uint8)", elem);
    const rw::Params &p = eng->prm;
    rw::GlobalImageArgs a{};
    const size_t esize = elem == 0 ? sizeof(float) : 1;
    uint64_t chw = 0;
    if (const int rc = global_image_plan(eng, "rw_global_image", layers, n_layers, pad_to_shape, esize, out_dev, a, chw)) return rc;
    a.B = p.B;
    // Envs per workgroup: some 8192 elements to store, within 60 KB of LDS (9 words of table, then per env: the request bitmap, a
    // word and a byte per cell — at most 51 KB at the 10000 cells rw_create admits) and within what an int indexes.
    const int words_per_env = p.SW + p.HW + (p.HW + 3) / 4;
    const int by_work = (int)std::max<uint64_t>(1, 8192 / chw), by_lds = (60 * 1024 / 4 - 8) / words_per_env;
    a.E = std::max(1, std::min(std::min(p.B, 64), std::min(by_work, by_lds)));
    const size_t lds = sizeof(int32_t) * (8 + (size_t)a.E * words_per_env);
    const unsigned n_wg = (unsigned)((p.B + a.E - 1) / a.E);
    // (a workgroup that has little to store is one wavefront: a 3-env batch does not need four)
    const unsigned threads = (uint64_t)a.E * std::max<uint64_t>(chw / (16 / esize), (uint64_t)p.HW) >= 1024 ? 256u : 64u;
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    global_image_stride(a, threads, esize, chw);
    auto go = [&](auto cell, auto el) {  // (`cell`: the shelf shadow's element type; `el`: the output's)
        using Cell = decltype(cell);
        using Elem = decltype(el);
        hipLaunchKernelGGL((rw::rware_global_image_kernel<Cell, Elem>), dim3(n_wg), dim3(threads), lds, eng->stream, (const Cell *)eng->d_shadow,
                           (const uint32_t *)eng->d_rec, (const int32_t *)p.queue, goal_cells_dev(eng), eng->d_status, (Elem *)out_dev, a);
    };
    if (eng->wide) elem == 0 ? go(uint16_t(), float()) : go(uint16_t(), uint8_t());
    else elem == 0 ? go(uint8_t(), float()) : go(uint8_t(), uint8_t());
    RW_HIP(eng, hipGetLastError());
    return RW_OK;
}

int32_t rw_global_record_bytes(const rw_engine *eng) {
    if (!eng) return RW_ERR_INVALID_ARG;
    return (eng->prm.HW + 1 + 15) & ~15;
}

int rw_global_records(rw_engine *eng, void *records_dev) {
    // One launch of rware_global_records_kernel on the engine's stream and nothing else (as rw_global_image); the status word is
    // neither read nor written.
    if (!eng) return RW_ERR_INVALID_ARG;
    if (!records_dev) return fail(eng, RW_ERR_INVALID_ARG, "rw_global_records: NULL records_dev");
    if (reinterpret_cast<uintptr_t>(records_dev) & 15u)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_global_records: records_dev has to be 16-byte aligned");
    const rw::Params &p = eng->prm;
    const int RB = rw_global_record_bytes(eng);
    rw::GlobalImageArgs a{};
    a.B = p.B; a.H = p.H; a.W = p.W; a.HW = p.HW; a.N = p.N; a.Q = p.Q; a.S = p.S; a.SW = p.SW; a.n_goals = p.n_goals;
    // Envs per workgroup: some 4096 cells to read and as many bytes to store, within 60 KB of LDS (per env: the record, the request
    // bitmap and a word per cell).
    const int words_per_env = RB / 4 + p.SW + p.HW;
    const int by_work = std::max(1, 4096 / p.HW), by_lds = (60 * 1024 / 4) / words_per_env;
    a.E = std::max(1, std::min(std::min(p.B, 64), std::min(by_work, by_lds)));
    const size_t lds = sizeof(int32_t) * (size_t)a.E * words_per_env;
    const unsigned n_wg = (unsigned)((p.B + a.E - 1) / a.E);
    const unsigned threads = (uint64_t)a.E * (uint64_t)p.HW >= 1024 ? 256u : 64u;
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    auto go = [&](auto cell) {  // (`cell`: the shelf shadow's element type)
        hipLaunchKernelGGL((rw::rware_global_records_kernel<decltype(cell)>), dim3(n_wg), dim3(threads), lds, eng->stream, (const decltype(cell) *)eng->d_shadow,
                           (const uint32_t *)eng->d_rec, (const int32_t *)p.queue, goal_cells_dev(eng), (uint8_t *)records_dev, RB, a);
    };
    eng->wide ? go(uint16_t()) : go(uint8_t());
    RW_HIP(eng, hipGetLastError());
    return RW_OK;
}

int rw_global_image_gather(rw_engine *eng, const uint8_t *records_dev, int64_t n_records, const void *index_dev, int64_t n_index,
                           const int32_t *layers, int32_t n_layers, const int32_t *pad_to_shape, int32_t elem, int32_t flags, void *out_dev) {
    // One launch of rware_global_image_gather_kernel on the engine's stream and nothing else: the host never reads the index or a record.
    if (!eng) return RW_ERR_INVALID_ARG;
    if (!records_dev || !layers || !out_dev)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_global_image_gather: NULL %s", !records_dev ? "records_dev" : !layers ? "layers" : "out_dev");
    if (n_records < 0 || n_index < 0)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_global_image_gather: n_records %lld, n_index %lld", (long long)n_records, (long long)n_index);
    if (elem < RW_GLOBAL_F32 || elem > RW_GLOBAL_BF16) return fail(eng, RW_ERR_INVALID_ARG, "rw_global_image_gather: unknown element type %d", (int)elem);
    if (n_layers < 1 || n_layers > rw::MAX_IMAGE_LAYERS)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_global_image_gather: n_layers %d not in 1..8", n_layers);
    int index64 = 0;
    const bool aligned = !(reinterpret_cast<uintptr_t>(records_dev) & 15u);
    if (const int rc = gather_index_args(eng, "rw_global_image_gather", flags, index_dev, n_index, n_records, "n_records", aligned,
                                         "records_dev has to be 16-byte aligned, index_dev to its element", index64)) return rc;
    const size_t esize = elem == RW_GLOBAL_F32 ? 4 : elem == RW_GLOBAL_U8 ? 1 : 2;
    rw::GlobalImageArgs a{};
    uint64_t chw = 0;
    if (const int rc = global_image_plan(eng, "rw_global_image_gather", layers, n_layers, pad_to_shape, esize, out_dev, a, chw)) return rc;
    const int RB = rw_global_record_bytes(eng);
    // (image numbers are ints in the kernel; record offsets are size_t bytes)
    if (n_index > 0x7fffffff || (uint64_t)n_records > ((uint64_t)1 << 52) / (uint64_t)RB)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_global_image_gather: %lld images of %lld records are more than one launch holds; gather in slices",
                    (long long)n_index, (long long)n_records);
    if (n_index == 0) return RW_OK;
    a.B = (int32_t)n_index;
    // Images per workgroup: some 8192 elements to store (as rw_global_image), within 60 KB of LDS (the table, then per image its
    // record and 8 bytes of index — at most 10 KB at the 10000 cells rw_create admits).
    const int by_work = (int)std::max<uint64_t>(1, 8192 / chw), by_lds = (60 * 1024 - 32) / (RB + 8);
    a.E = std::max(1, std::min((int)std::min<int64_t>(n_index, 64), std::min(by_work, by_lds)));
    const size_t lds = 32 + (size_t)a.E * ((size_t)RB + 8);
    const unsigned n_wg = (unsigned)((n_index + a.E - 1) / a.E);
    // (four wavefronts once there are 16 lookups a thread — counted in ELEMENTS, whatever their size: a uint8 store has 16 lookups in
    //  front of it, and one wavefront per workgroup left the narrow types a quarter of the float32 kernel's waves, 2048 against 8192)
    const unsigned threads = (uint64_t)a.E * chw >= 4096 ? 256u : 64u;
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    global_image_stride(a, threads, esize, chw);
    const rw::GlobalGatherArgs g{records_dev, index_dev, n_records, RB, index64};
    auto go = [&](auto el) {
        hipLaunchKernelGGL((rw::rware_global_image_gather_kernel<decltype(el)>), dim3(n_wg), dim3(threads), lds, eng->stream, g, eng->d_status,
                           (decltype(el) *)out_dev, a);
    };
    if (elem == RW_GLOBAL_F32) go(float());
    else if (elem == RW_GLOBAL_U8) go(uint8_t());
    else if (elem == RW_GLOBAL_F16) go(rw::F16Bits());
    else go(rw::BF16Bits());
    RW_HIP(eng, hipGetLastError());
    return RW_OK;
}

}  // extern "C"

// The next learner-side op, rw_gae.  Included from here and not from rware_capi.hip: that file's code is part of what
// bench.kernel_sources_sha() identifies the step path's measured evidence by (profiles/pmc_traffic.json), and this op changes nothing there.
#include "rware_advantages.h"
