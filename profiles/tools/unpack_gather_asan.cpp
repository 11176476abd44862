// Stand-alone AddressSanitizer / UBSan driver for rw_unpack_obs_gather on the host-thread build of the product sources (CPU only; no
// Python), and the check of its two float32 -> 16-bit conversions.  The packed rows, the index array and the output are heap blocks of
// exactly their sizes (redzones on both sides), so an out-of-bounds load or store of the kernel faults; UBSan reports a misaligned wide
// access.  Every output is recomputed here in plain loops — the 16-bit values by frexp / nearbyint, not by the code under test — and compared.
// Build, run and compare with profiles/unpack_gather_asan.txt: make -C profiles/tools check
// (the exact-shape table groups and sensor ranges 3 .. 5 are stubbed in asan_driver.h)
#define ASAN_DRIVER_LINKS_GENERIC_R2
#include "asan_driver.h"

#include <cmath>
#include <random>

#define RW_MINIBATCH_CONVERSIONS_ONLY
#include "rware_minibatch.h"

// float -> a 16-bit float of `mant` explicit mantissa bits and minimum normal exponent `emin`, round to nearest even, by frexp / nearbyint
static uint32_t ref_convert(float v, int mant, int emin, int bias, uint32_t inf) {
    uint32_t sign = std::signbit(v) ? 0x8000u : 0u;
    if (std::isnan(v)) return ~0u;          // (NaN patterns are not compared)
    if (std::isinf(v)) return sign | inf;
    double a = std::fabs((double)v);
    if (a == 0.0) return sign;
    int e;
    (void)std::frexp(a, &e);                // a = m * 2^e, m in [0.5, 1): the leading bit has weight 2^(e-1)
    int E = e - 1 < emin ? emin : e - 1;
    const double q = std::ldexp(1.0, E - mant);
    const double r = std::nearbyint(a / q); // (the default rounding mode: to nearest, ties to even)
    if (r == 0.0) return sign;              // rounded to zero
    double val = r * q;
    (void)std::frexp(val, &e);
    if (e - 1 > bias) return sign | inf;    // rounded past the largest finite value
    if (e - 1 < emin) return sign | (uint32_t)r;                                  // subnormal: the count of quanta
    return sign | ((uint32_t)(e - 1 + bias) << mant) | ((uint32_t)std::llround(val / std::ldexp(1.0, e - 1 - mant)) - (1u << mant));
}
static uint32_t ref_f16(float v) { return ref_convert(v, 10, -14, 15, 0x7C00u); }
static uint32_t ref_bf16(float v) { return ref_convert(v, 7, -126, 127, 0x7F80u); }
static float from_bits(uint32_t x) { float v; memcpy(&v, &x, 4); return v; }

static void check_conversions() {
    long n = 0;
    auto one = [&](uint32_t x) {
        const float v = from_bits(x);
        if (std::isnan(v)) return;
        const uint32_t h = rw::f32_bits_to_f16(x), hr = ref_f16(v), b = rw::f32_bits_to_bf16(x), br = ref_bf16(v);
        if (h != hr || b != br) { printf("FAILED: float32 0x%08x -> f16 0x%04x (want 0x%04x), bf16 0x%04x (want 0x%04x)\n", x, h, hr, b, br); exit(1); }
        ++n;
    };
    // every tie between two neighbouring float16 values (normal and subnormal) and between two bfloat16 values, with its two neighbours
    for (uint32_t h = 0; h < 0x7C00u; ++h) {
        const uint32_t e = h >> 10, m = h & 0x3FFu;
        const double lo = e ? std::ldexp(1024.0 + m, (int)e - 25) : std::ldexp((double)m, -24), step = std::ldexp(1.0, (e ? (int)e : 1) - 25);
        const float mid = (float)(lo + step / 2);
        uint32_t x;
        memcpy(&x, &mid, 4);
        for (uint32_t d = 0; d < 3; ++d) { one(x - 1 + d); one((x - 1 + d) | 0x80000000u); }
    }
    for (uint32_t b = 0; b < 0x7F80u; ++b)
        for (uint32_t d = 0; d < 3; ++d) { one((b << 16) + 0x7FFFu + d); one(((b << 16) + 0x7FFFu + d) | 0x80000000u); }
    // ... and one float32 pattern in 61 of all of them
    for (uint64_t x = 0; x < (1ull << 32); x += 61) one((uint32_t)x);
    // every value a coordinate can take: integers up to 65535 and every quotient v / (dim - 1) of a grid the engine admits (H * W <= 10000)
    for (uint32_t v = 0; v < 65536; ++v) { float f = (float)v; uint32_t x; memcpy(&x, &f, 4); one(x); }
    for (int dim = 2; dim <= 10000; ++dim)
        for (int v = 0; v < dim; ++v) { float f = (float)((double)v / (double)(dim - 1)); uint32_t x; memcpy(&x, &f, 4); one(x); }
    printf("asan-run conversions: %ld float32 patterns (every float16 and bfloat16 tie with its neighbours, 1 in 61 of all patterns, every "
           "coordinate value) round as frexp / nearbyint do\n", n);
}

static void run(const char *what, int H, int W, int sensor_range, int M, int normalised) {
    TinyWarehouse wh(2, H, W, 2, 2, 9, [](int y, int H_) { return y == 0 || y == H_ - 1; });   // (no highway rows inside)
    wh.cfg.sensor_range = sensor_range; wh.cfg.msg_bits = M; wh.cfg.normalised_coordinates = normalised;
    rw_engine *eng = wh.create();
    rw_info info;
    CK(rw_get_info(eng, &info));
    const int L = info.obs_length, PW = 1 + (L + 31) / 32;
    std::mt19937 rng(7);
    long calls = 0, elems = 0;
    for (int G = 1; G <= 3; ++G) {
        const int n_groups = 7;
        const size_t rows = (size_t)n_groups * G;
        uint32_t *packed = static_cast<uint32_t *>(malloc(rows * PW * 4));          // exactly the rows: redzones on both sides
        for (size_t r = 0; r < rows; ++r) {
            uint32_t *p = packed + r * PW;
            const uint32_t x = r == 0 ? 0 : r + 1 == rows ? W - 1 : rng() % W, y = r == 0 ? 0 : r + 1 == rows ? H - 1 : rng() % H;
            p[0] = x | (y << 16);
            for (int w = 1; w < PW; ++w) p[w] = 0;
            for (int k = 2; k < L; ++k) p[1 + k / 32] |= (uint32_t)(rng() & 1u) << (k % 32);
        }
        for (int pattern = 0; pattern < 5; ++pattern) {
            // 0: identity (NULL), 1: reversed, 2: random with repeats and more indices than groups, 3: one index, 4: bad indices among good ones
            const int n = pattern == 2 ? n_groups + 4 : pattern == 3 ? 1 : pattern == 4 ? 6 : n_groups;
            std::vector<int64_t> idx(n);
            for (int i = 0; i < n; ++i)
                idx[i] = pattern <= 1 ? (pattern ? n_groups - 1 - i : i) : pattern == 4 && i % 2 ? (i == 1 ? -1 : i == 3 ? n_groups : (int64_t)1 << 31)
                                                                                               : (int64_t)(rng() % n_groups);
            for (int wide = 0; wide < 2; ++wide) {
                if (pattern == 0 && wide) continue;
                void *index = nullptr;
                if (pattern) {
                    index = malloc((size_t)n * (wide ? 8 : 4));
                    for (int i = 0; i < n; ++i)
                        if (wide) static_cast<int64_t *>(index)[i] = idx[i];
                        else static_cast<int32_t *>(index)[i] = (int32_t)idx[i];   // (2^31 becomes INT32_MIN: as bad)
                }
                for (int elem = 0; elem < 3; ++elem)
                    for (int off = 0; off < 2; ++off) {
                        const size_t es = elem == RW_UNPACK_F32 ? 4 : 2, count = (size_t)n * G * L;
                        // posix_memalign: a 16-byte aligned block of exactly the output (+ one element when the output starts one element in)
                        void *block = nullptr;
                        if (posix_memalign(&block, 16, (count + off) * es)) exit(1);
                        char *out = static_cast<char *>(block) + off * es;
                        memset(block, 0xA5, (count + off) * es);
                        CK(rw_unpack_obs_gather(eng, packed, n_groups, G, index, n, elem, wide ? RW_UNPACK_INDEX64 : 0, out));
                        const int rc = rw_sync(eng);
                        if (rc != (pattern == 4 ? RW_ERR_INVALID_ARG : RW_OK) || rw_sync(eng) != RW_OK) { printf("FAILED: rw_sync -> %d\n", rc); exit(1); }
                        if (off && (unsigned char)static_cast<char *>(block)[0] != 0xA5) { printf("FAILED: wrote in front of the output\n"); exit(1); }
                        for (int i = 0; i < n; ++i)
                            for (int g = 0; g < G; ++g)
                                for (int k = 0; k < L; ++k) {
                                    const int64_t j = wide || !pattern ? idx[i] : (int64_t)(int32_t)idx[i];
                                    float want = 0.0f;
                                    if (j >= 0 && j < n_groups) {
                                        const uint32_t *p = packed + ((size_t)j * G + g) * PW;
                                        const uint32_t c = k == 0 ? p[0] & 0xFFFFu : p[0] >> 16;
                                        want = k < 2 ? (normalised ? (float)((double)c / (double)((k ? H : W) - 1)) : (float)c)
                                                     : (float)((p[1 + k / 32] >> (k % 32)) & 1u);
                                    }
                                    const size_t at = ((size_t)i * G + g) * L + k;
                                    uint32_t got = 0, wb;
                                    memcpy(&got, out + at * es, es);
                                    memcpy(&wb, &want, 4);
                                    if (elem == RW_UNPACK_F16) wb = ref_f16(want);
                                    if (elem == RW_UNPACK_BF16) wb = ref_bf16(want);
                                    if (got != wb) {
                                        printf("FAILED: %s G %d pattern %d elem %d offset %d: group %d row %d element %d is 0x%x, not 0x%x\n", what, G,
                                               pattern, elem, off, i, g, k, got, wb);
                                        exit(1);
                                    }
                                    ++elems;
                                }
                        free(block);
                        ++calls;
                    }
                free(index);
            }
        }
        free(packed);
    }
    printf("asan-run %-34s %d x %d, L %d, PW %d, normalised %d: %ld calls (1-3 rows a group; identity, reversed, repeats, one, bad indices; int32 and "
           "int64; three element types; aligned and one element in), %ld elements equal the plain recomputation\n", what, H, W, L, PW, normalised, calls, elems);
    CK(rw_destroy(eng));
}

int main() {
    check_conversions();
    run("L 71: rows straddle chunks", 11, 10, 1, 0, 0);
    run("L 71, normalised coordinates", 11, 10, 1, 0, 1);
    run("L 80: rows on chunk boundaries", 11, 10, 1, 1, 1);
    run("L 258: word-crossing nibbles", 11, 10, 2, 3, 1);
    run("4 x 262: x beyond 256", 4, 262, 1, 0, 0);
    printf("asan-run done: no AddressSanitizer / UBSan report above = clean\n");
    return 0;
}
