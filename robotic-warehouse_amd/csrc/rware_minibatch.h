// rw_unpack_obs_gather: packed rows uint32 [n_groups][G][PW] -> [n_index][G][L] float32, float16 or bfloat16, output group i from source
// group index[i] (NULL index: the identity) — what unpack_obs(packed[index]).to(dtype) computes, in one launch and without its
// intermediates.  Included by rware_capi.hip, inside namespace-free scope, after rware_kernels.h (funnel_shr, u32x4, store_u4*,
// STATUS_RESTORE_INDEX) and rw::unpack_elem.  Plain C++ throughout: the host-thread build of tests/emu compiles this file as it is, so
// the 16-bit element types are written as bit patterns (no __half, no __hip_bfloat16).
//
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

#ifndef RW_MINIBATCH_CONVERSIONS_ONLY   // (profiles/tools/unpack_gather_asan.cpp includes the two conversions above on their own)
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

// the source group of output group i, -1 for one outside 0 .. n_groups-1 (and the status bit)
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

#endif  // RW_MINIBATCH_CONVERSIONS_ONLY

}  // namespace rw
