// Counter-based random numbers on the device: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy
// as 1, 2, 3", SC'11; the Random123 constants), and the dropout mask built on it.
//
// The mask of element e = b * C + c of a [B, C] tensor is a pure function of (seed, offset, p, e):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = ((e >> 2) & 0xffffffff, (e >> 2) >> 32, offset & 0xffffffff, offset >> 32)
//   r       = philox(counter, key)[e & 3]
//   keep    = r < thr,  thr = min(floor((1 - p) * 2^32), 2^32 - 1) computed in double (dir_dropout_thr)
// so one Philox call serves four consecutive elements, and a backward regenerates exactly the forward's mask.
#pragma once
#include <math.h>
#include <stdint.h>

#define DIR_PHILOX_M0 0xD2511F53u
#define DIR_PHILOX_M1 0xCD9E8D57u
#define DIR_PHILOX_W0 0x9E3779B9u
#define DIR_PHILOX_W1 0xBB67AE85u

struct DirU32x4 { uint32_t v[4]; };

// Philox4x32 with 10 rounds; the key is bumped by the Weyl increments between rounds.
__device__ __forceinline__ DirU32x4 dir_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        if (i) { k0 += DIR_PHILOX_W0; k1 += DIR_PHILOX_W1; }
        const uint32_t hi0 = __umulhi(DIR_PHILOX_M0, c0), lo0 = DIR_PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(DIR_PHILOX_M1, c2), lo1 = DIR_PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    }
    return DirU32x4{{c0, c1, c2, c3}};
}

// Dropout parameters of one call: the keep threshold and the scale of the kept values.
struct DirDropout {
    uint64_t seed, offset;
    uint32_t thr;                           // keep = r < thr
    float scale;                            // (float)(1 / (1 - p)); 0 at p == 1 (nothing is kept)
};

// Host side: thr / scale of a drop probability p in [0, 1] (the caller rejects anything else).
static inline DirDropout dir_dropout_params(uint64_t seed, uint64_t offset, double p) {
    double t = floor((1.0 - p) * 4294967296.0);
    if (t > 4294967295.0) t = 4294967295.0;
    DirDropout d;
    d.seed = seed; d.offset = offset;
    d.thr = (uint32_t)t;
    d.scale = p == 1.0 ? 0.0f : (float)(1.0 / (1.0 - p));
    return d;
}

// The four random words of the group of elements q = e >> 2.
__device__ __forceinline__ DirU32x4 dir_dropout_bits(const DirDropout& d, uint64_t q) {
    return dir_philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)d.offset, (uint32_t)(d.offset >> 32),
                             (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
}

__device__ __forceinline__ float dir_dropout_apply(const DirDropout& d, uint32_t r, float v) {
    return r < d.thr ? v * d.scale : 0.0f;
}
