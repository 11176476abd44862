// Packed observation rows on the learner's side: rw_unpack_obs and rw_unpack_obs_gather (include/rware_hip.h, include/rware_hip_minibatch.h).
// Included by rware_capi.hip at file scope, after rware_kernels.h (funnel_shr, opaque, u32x4, store_u4*, store_f4_nt, STATUS_RESTORE_INDEX)
// and after the engine internals the host part at the end uses (rw_engine, fail, RW_HIP).  The kernels first, the host part below them.
// Plain C++ throughout: the host-thread build of tests/emu compiles this file as it is, so the 16-bit element types are written as bit
// patterns (no __half, no __hip_bfloat16).  gather_index_args is shared with rware_global_state.h, which comes next.
//
// rw_unpack_obs_gather: packed rows uint32 [n_groups][G][PW] -> [n_index][G][L] float32, float16 or bfloat16, output group i from source
// group index[i] (NULL index: the identity) — what unpack_obs(packed[index]).to(dtype) computes, in one launch and without its intermediates.
// The output is one flat stream of elements; a thread takes one 16-byte chunk of it — 4 float32 or 8 halves — so a wavefront stores 1 KiB
// of consecutive bytes.  The chunk's first element f gives its output row f / L (by a multiplication with 1 / L in double and one
// correction step: f stays below 2^53), the row its group, and the group ONE read of the index.
//   fast path   the chunk lies in the bit part of one row (k >= 2, k + EPC <= L): EPC bits from one or two packed words with the funnel
//               shift, spread into element patterns — 0 and 1 are constants in every type — and one 16-byte store;
//   slow path   a chunk that holds a coordinate, straddles two rows (the index is read again only where the group changes), ends behind
//               the stream's last element, or an output that does not start on a 16-byte boundary: element by element.
// A source group outside 0 .. n_groups-1: the elements of that output group are zeros, no packed word of it is read, and the status
// word gets STATUS_RESTORE_INDEX (rw_sync: RW_ERR_INVALID_ARG).
// Stores: non-temporal 16-byte ones, as in rw_unpack_obs.  Measured on the MI355X against plain stores (profiles/EXPERIMENTS.md, round 17):
// the float32 kernel is 8 .. 17 % faster with them (147.6 against 178.0 us for 298 MB), the 16-bit kernels 1 .. 8 %; nothing was slower.
#pragma once

namespace rw {

enum : int { UNPACK_F32 = 0, UNPACK_F16 = 1, UNPACK_BF16 = 2 };   // enum rw_unpack_elem

// float32 bits -> bfloat16 / float16 bits, round to nearest even, in integer arithmetic (checked against a conversion by frexp / nearbyint
// on every tie, its two neighbours and a 1-in-61 sample of all float32 patterns: profiles/tools/unpack_gather_asan.cpp)
__device__ __forceinline__ uint32_t f32_bits_to_bf16(uint32_t x) {
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (x >> 16) | 0x0040u;   // NaN stays one
    return (x + 0x7FFFu + ((x >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ uint32_t f32_bits_to_f16(uint32_t x) {
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7FFFFFFFu;
    if (x >= 0x47800000u) return sign | (x > 0x7F800000u ? 0x7E00u : 0x7C00u);   // 65536 and beyond: infinity; NaN
    if (x < 0x38800000u) {                                                        // below 2^-14: a float16 subnormal, m * 2^(e - 126) halves of 2^-24
        const uint32_t e = x >> 23;
        if (e < 102u) return sign;                                                // below 2^-25: zero
        const uint32_t m = (x & 0x7FFFFFu) | 0x800000u, sh = 126u - e;            // sh: 14 .. 24
        uint32_t r = m >> sh;
        const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
        if (rem > half || (rem == half && (r & 1u))) ++r;
        return sign | r;
    }
    const uint32_t r = x - 0x38000000u;                                           // exponent rebiased; a carry out of the mantissa lands in it
    return sign | ((r + 0xFFFu + ((r >> 13) & 1u)) >> 13);
}
__device__ __forceinline__ uint32_t f32_as_bits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}

}  // namespace rw

#ifndef RW_MINIBATCH_CONVERSIONS_ONLY   // (profiles/tools/unpack_gather_asan.cpp includes the conversions above on their own, without an engine)
namespace rw {

// rw_unpack_obs: packed rows uint32 [n_rows][PW] -> float32 [n_rows][L], bit for bit what RW_BUF_OBS would hold.  One thread per float4
// of the output.  A float4 that lies inside the bit part of one row (all but ~2 in 18 at sensor_range 1) takes its four bits from one
// or two packed words, spreads them into four bytes with one multiply (bit j -> byte j) and converts each byte (v_cvt_f32_ubyteN), as
// the step kernel's expansion does; one that holds a coordinate slot or straddles two rows goes element by element.  The output is a
// pure stream: non-temporal stores.  `aligned`: the output starts on a 16-byte boundary (else scalar stores).
__device__ __forceinline__ float unpack_elem(const uint32_t *__restrict__ packed, size_t row, int k, int PW, int W, int H, int normalised) {
    const uint32_t *r = packed + row * (size_t)PW;
    if (k < 2) {
        const int v = (int)(k == 0 ? (r[0] & 0xFFFFu) : (r[0] >> 16));
        if (normalised) return (float)((double)v / (double)((k == 0 ? W : H) - 1));  // coordf of the step kernel (rware/warehouse.py:636-638)
        return (float)v;
    }
    return ((r[1 + (k >> 5)] >> (k & 31)) & 1u) ? 1.0f : 0.0f;
}
template <typename Dummy = void>
__global__ void __launch_bounds__(256) rware_unpack_obs_kernel(const uint32_t *__restrict__ packed, float *__restrict__ out, size_t n_floats,
                                                                int L, int PW, int W, int H, int normalised, int aligned) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t f = q << 2;
    if (f >= n_floats) return;
    const size_t row = f / (size_t)L;
    const int k = (int)(f - row * (size_t)L);
    if (aligned && k >= 2 && k + 3 < L && f + 3 < n_floats) {
        const uint32_t *r = packed + row * (size_t)PW + 1 + (k >> 5);
        const int sh = k & 31;
        const uint32_t lo = r[0], hi = sh > 28 ? r[1] : 0u;  // (sh > 28 implies k + 3 crosses into the next word, which the row still owns: k + 3 < L)
        const uint32_t nib = funnel_shr(lo, hi, (uint32_t)sh) & 0xFu;
        const uint32_t b = opaque((nib * 0x00204081u) & 0x01010101u);
        float4 v;
        v.x = (float)(b & 0xFFu);
        v.y = (float)((b >> 8) & 0xFFu);
        v.z = (float)((b >> 16) & 0xFFu);
        v.w = (float)(b >> 24);
        store_f4_nt(reinterpret_cast<float4 *>(out + f), v);
        return;
    }
    float e[4];
    size_t rw_ = row;
    int kk = k;
    const int n = (int)(n_floats - f < 4 ? n_floats - f : 4);
    for (int j = 0; j < n; ++j) {
        e[j] = unpack_elem(packed, rw_, kk, PW, W, H, normalised);
        if (++kk == L) { kk = 0; ++rw_; }
    }
    if (aligned && n == 4) {
        float4 v;
        v.x = e[0]; v.y = e[1]; v.z = e[2]; v.w = e[3];
        store_f4_nt(reinterpret_cast<float4 *>(out + f), v);
    } else {
        for (int j = 0; j < n; ++j) out[f + j] = e[j];
    }
}

template <int ELEM>
__device__ __forceinline__ uint32_t unpack_elem_bits(const uint32_t *__restrict__ packed, size_t row, int k, int PW, int W, int H, int normalised) {
    const uint32_t x = f32_as_bits(unpack_elem(packed, row, k, PW, W, H, normalised));
    return ELEM == UNPACK_F32 ? x : ELEM == UNPACK_F16 ? f32_bits_to_f16(x) : f32_bits_to_bf16(x);
}

// a / d and a % d for a < 2^53, 1 <= d < 2^31, `inv` = 1.0 / d: the product is off by less than one, so one step either way corrects it
__device__ __forceinline__ void divmod_by(uint64_t a, int d, double inv, uint64_t &q, int &r) {
    uint64_t qq = (uint64_t)((double)a * inv);
    int64_t rr = (int64_t)a - (int64_t)(qq * (uint64_t)d);
    if (rr < 0) { --qq; rr += d; }
    else if (rr >= d) { ++qq; rr -= d; }
    q = qq;
    r = (int)rr;
}

struct UnpackGatherArgs {
    const uint32_t *packed;   // [n_groups][G][PW]
    const void *index;        // [n_index] int32 or int64 (index64), NULL: the identity
    void *out;                // [n_index][G][L] elements
    uint64_t n_elems;         // n_index * G * L
    int64_t n_groups;
    double inv_L, inv_G;
    int32_t *status;
    int32_t G, L, PW, W, H, normalised, aligned, index64;
};

// the source group of output group i, -1 for one outside 0 .. n_groups-1 (and the status bit).  (rware_global_image_gather_kernel reads its
// index the same way but range-checks the identity too; either form, shared, changes the other kernel's instructions: two copies)
__device__ __forceinline__ int64_t gather_source(const UnpackGatherArgs &a, uint64_t i) {
    if (!a.index) return (int64_t)i;
    const int64_t j = a.index64 ? static_cast<const int64_t *>(a.index)[i] : (int64_t)static_cast<const int32_t *>(a.index)[i];
    if (j < 0 || j >= a.n_groups) {
        atomicOr(a.status, (int)STATUS_RESTORE_INDEX);
        return -1;
    }
    return j;
}

template <int ELEM>
__global__ void __launch_bounds__(256) rware_unpack_gather_kernel(const UnpackGatherArgs a) {
    constexpr int EPC = ELEM == UNPACK_F32 ? 4 : 8;                      // elements per 16-byte chunk
    constexpr uint32_t ONE = ELEM == UNPACK_F32 ? 0x3F800000u : ELEM == UNPACK_F16 ? 0x3C00u : 0x3F80u;
    const uint64_t f = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * (uint64_t)EPC;
    if (f >= a.n_elems) return;
    const int L = a.L, G = a.G;
    uint64_t row, grp;
    int k, g = 0;
    divmod_by(f, L, a.inv_L, row, k);
    if (G > 1) divmod_by(row, G, a.inv_G, grp, g);
    else grp = row;
    int64_t src = gather_source(a, grp);
    if (a.aligned && k >= 2 && k + EPC <= L) {                           // (inside a row, so inside the stream: f + EPC <= n_elems)
        u32x4 v = {0u, 0u, 0u, 0u};
        if (src >= 0) {
            const uint32_t *r = a.packed + ((size_t)src * (size_t)G + (size_t)g) * (size_t)a.PW + 1 + (k >> 5);
            const int sh = k & 31;
            const uint32_t lo = r[0], hi = sh > 32 - EPC ? r[1] : 0u;    // (then k + EPC - 1 lies in the next word, which the row still owns)
            const uint32_t bits = funnel_shr(lo, hi, (uint32_t)sh) & ((1u << EPC) - 1u);
            if constexpr (ELEM == UNPACK_F32) {
                v.x = (bits & 1u) * ONE;
                v.y = ((bits >> 1) & 1u) * ONE;
                v.z = ((bits >> 2) & 1u) * ONE;
                v.w = ((bits >> 3) & 1u) * ONE;
            } else {                                                     // two elements a dword: bits 2j, 2j+1 -> bits 0 and 16, times the pattern of 1
                v.x = ((bits | (bits << 15)) & 0x00010001u) * ONE;
                v.y = (((bits >> 2) | (bits << 13)) & 0x00010001u) * ONE;
                v.z = (((bits >> 4) | (bits << 11)) & 0x00010001u) * ONE;
                v.w = (((bits >> 6) | (bits << 9)) & 0x00010001u) * ONE;
            }
        }
        store_u4_nt(reinterpret_cast<u32x4 *>(static_cast<char *>(a.out) + f * (ELEM == UNPACK_F32 ? 4u : 2u)), v);
        return;
    }
    uint32_t e[EPC];
    const int n = (int)(a.n_elems - f < (uint64_t)EPC ? a.n_elems - f : (uint64_t)EPC);
    for (int j = 0; j < n; ++j) {
        e[j] = src >= 0 ? unpack_elem_bits<ELEM>(a.packed, (size_t)src * (size_t)G + (size_t)g, k, a.PW, a.W, a.H, a.normalised) : 0u;
        if (++k == L) {
            k = 0;
            if (++g == G) {
                g = 0;
                ++grp;
                if (j + 1 < n) src = gather_source(a, grp);              // (the chunk goes on into the next group: its index, read once)
            }
        }
    }
    if constexpr (ELEM == UNPACK_F32) {
        uint32_t *o = static_cast<uint32_t *>(a.out) + f;
        if (a.aligned && n == EPC) {
            u32x4 v = {e[0], e[1], e[2], e[3]};
            store_u4_nt(reinterpret_cast<u32x4 *>(o), v);
        } else {
            for (int j = 0; j < n; ++j) o[j] = e[j];
        }
    } else {
        uint16_t *o = static_cast<uint16_t *>(a.out) + f;
        if (a.aligned && n == EPC) {
            u32x4 v = {e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
            store_u4_nt(reinterpret_cast<u32x4 *>(o), v);
        } else {
            for (int j = 0; j < n; ++j) o[j] = (uint16_t)e[j];
        }
    }
}

}  // namespace rw

// ---- host part ----------------------------------------------------------------------------------------------------------------------

// The index arguments of a gather, checked for `who` (rw_unpack_obs_gather, rw_global_image_gather): no flag but INDEX64; without an index
// the output is the source, so n_index has to be the `n_name` n; index_dev aligned to its element — `others_aligned`, `alignment`: whether
// the caller's other pointers are, and the sentence that names them all.  index64: whether index_dev holds int64.
static_assert((int)RW_UNPACK_INDEX64 == (int)RW_GLOBAL_INDEX64,"the two gathers share one check of their flags");
static int gather_index_args(rw_engine *eng, const char *who, int32_t flags, const void *index_dev, int64_t n_index, int64_t n, const char *n_name,
                             bool others_aligned, const char *alignment, int &index64) {
    if (flags & ~(int32_t)RW_UNPACK_INDEX64)
        return fail(eng, RW_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~(int32_t)RW_UNPACK_INDEX64));
    if (!index_dev && n_index != n)
        return fail(eng, RW_ERR_INVALID_ARG, "%s: without an index n_index (%lld) has to be %s (%lld)", who, (long long)n_index, n_name, (long long)n);
    index64 = (flags & RW_UNPACK_INDEX64) ? 1 : 0;
    if (!others_aligned || (reinterpret_cast<uintptr_t>(index_dev) & (index64 ? 7u : 3u))) return fail(eng, RW_ERR_INVALID_ARG, "%s: %s", who, alignment);
    return RW_OK;
}

extern "C" {

int rw_unpack_obs(rw_engine *eng, const uint32_t *packed_dev, float *obs_f32_dev, int64_t n_rows) {
    if (!eng || n_rows < 0 || (n_rows && (!packed_dev || !obs_f32_dev))) return RW_ERR_INVALID_ARG;
    if (eng->image)  // (RW_OBS_IMAGE_U8 included: a uint8 image needs no unpacking)
        return fail(eng, RW_ERR_UNSUPPORTED, "rw_unpack_obs: packed rows exist for FLATTENED observations only");
    if (n_rows == 0) return RW_OK;
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    const size_t n_floats = (size_t)n_rows * (size_t)eng->L, n_q = (n_floats + 3) / 4;
    const size_t blocks = (n_q + 255) / 256;
    if (blocks > 0x7fffffffu) return fail(eng, RW_ERR_INVALID_ARG, "rw_unpack_obs: %lld rows are more than one launch holds; unpack in slices", (long long)n_rows);
    const int aligned = (reinterpret_cast<uintptr_t>(obs_f32_dev) & 15u) == 0 ? 1 : 0;
    hipLaunchKernelGGL((rw::rware_unpack_obs_kernel<>), dim3((unsigned)blocks), dim3(256), 0, eng->stream, packed_dev, obs_f32_dev, n_floats,
                       eng->L, eng->PW, eng->prm.W, eng->prm.H, eng->prm.normalised, aligned);
    RW_HIP(eng, hipGetLastError());
    return RW_OK;
}

int rw_unpack_obs_gather(rw_engine *eng, const uint32_t *packed_dev, int64_t n_groups, int32_t rows_per_group, const void *index_dev,
                         int64_t n_index, int32_t elem, int32_t flags, void *out_dev) {
    // One launch of rware_unpack_gather_kernel on the engine's stream and nothing else: the host never reads the index array, so the call
    // is legal inside a stream capture and is replayed with the graph.
    if (!eng) return RW_ERR_INVALID_ARG;
    if (eng->image)  // (RW_OBS_IMAGE_U8 included)
        return fail(eng, RW_ERR_UNSUPPORTED, "rw_unpack_obs_gather: packed rows exist for FLATTENED observations only");
    if (!packed_dev || !out_dev) return fail(eng, RW_ERR_INVALID_ARG, "rw_unpack_obs_gather: NULL %s", !packed_dev ? "packed_dev" : "out_dev");
    if (n_groups < 0 || n_index < 0 || rows_per_group < 1)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_unpack_obs_gather: n_groups %lld, n_index %lld, rows_per_group %d", (long long)n_groups,
                    (long long)n_index, (int)rows_per_group);
    if (elem != RW_UNPACK_F32 && elem != RW_UNPACK_F16 && elem != RW_UNPACK_BF16)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_unpack_obs_gather: unknown element type %d", (int)elem);
    const unsigned elem_bytes = elem == RW_UNPACK_F32 ? 4u : 2u;
    rw::UnpackGatherArgs a{};
    const bool aligned = !(reinterpret_cast<uintptr_t>(packed_dev) & 3u) && !(reinterpret_cast<uintptr_t>(out_dev) & (elem_bytes - 1u));
    if (const int rc = gather_index_args(eng, "rw_unpack_obs_gather", flags, index_dev, n_index, n_groups, "n_groups", aligned,
                                         "packed_dev has to be 4-byte aligned, index_dev and out_dev to their elements", a.index64)) return rc;
    // one thread per 16 bytes of output, 256 a workgroup, at most 2^31 - 1 workgroups; the source rows are addressed in size_t words
    const uint64_t per_group = (uint64_t)rows_per_group * (uint64_t)eng->L, chunk = 16u / elem_bytes;
    const uint64_t max_elems = (uint64_t)0x7fffffffu * 256u * chunk;
    if ((uint64_t)n_index > max_elems / per_group || (uint64_t)n_groups > ((uint64_t)1 << 52) / ((uint64_t)rows_per_group * (uint64_t)eng->PW))
        return fail(eng, RW_ERR_INVALID_ARG, "rw_unpack_obs_gather: %lld groups of %d rows are more than one launch holds; unpack in slices",
                    (long long)std::max(n_index, n_groups), (int)rows_per_group);
    if (n_index == 0) return RW_OK;
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    a.packed = packed_dev;
    a.index = index_dev;
    a.out = out_dev;
    a.n_elems = (uint64_t)n_index * per_group;
    a.n_groups = n_groups;
    a.inv_L = 1.0 / (double)eng->L;
    a.inv_G = 1.0 / (double)rows_per_group;
    a.status = eng->d_status;
    a.G = rows_per_group;
    a.L = eng->L;
    a.PW = eng->PW;
    a.W = eng->prm.W;
    a.H = eng->prm.H;
    a.normalised = eng->prm.normalised;
    a.aligned = (reinterpret_cast<uintptr_t>(out_dev) & 15u) == 0 ? 1 : 0;
    const unsigned blocks = (unsigned)(((a.n_elems + chunk - 1) / chunk + 255) / 256);
    auto go = [&](auto el) {
        hipLaunchKernelGGL((rw::rware_unpack_gather_kernel<decltype(el)::value>), dim3(blocks), dim3(256), 0, eng->stream, a);
    };
    if (elem == RW_UNPACK_F32) go(std::integral_constant<int, rw::UNPACK_F32>());
    else if (elem == RW_UNPACK_F16) go(std::integral_constant<int, rw::UNPACK_F16>());
    else go(std::integral_constant<int, rw::UNPACK_BF16>());
    RW_HIP(eng, hipGetLastError());
    return RW_OK;
}

}  // extern "C"
#endif  // RW_MINIBATCH_CONVERSIONS_ONLY
