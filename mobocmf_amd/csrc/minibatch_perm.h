// The epoch permutation of the mini-batch sampler (minibatch.hip): a stateless keyed bijection of 0..N-1.  ONE definition,
// compiled for the device (the index launch) and for the host (mobocmf_minibatch_permutation_host), so that both give the
// same rows bitwise.  DESIGN.md 5.3 states it in words precise enough to restate in numpy (tests/test_minibatch_cpu.py does).
//
//   b  = bit length of N - 1 (0 for N = 1), hb = b / 2 low bits, ha = b - hb high bits: the domain 2^b is below 2N.
//   A value v < 2^b is split as v = (A << hb) | B.  Round r = 0 .. MB_ROUNDS-1 changes ONE half, keyed by the other:
//     r even:  A ^= F(r, B) & (2^ha - 1)          r odd:  B ^= F(r, A) & (2^hb - 1)
//   F(r, h) = word 0 of Philox4x32-10 with counter (h, r, epoch_lo, epoch_hi) and key (seed_lo, seed_hi).
//   Each round is an involution for a fixed other half, so the whole map is a bijection of 0..2^b-1 (an unbalanced Feistel
//   network when b is odd).  Cycle-walking restricts it to 0..N-1: the map is applied again while the value is >= N.  The walk
//   ends because it starts below N and a bijection's cycles return to their start; it is bounded by the domain size anyway.
// Included after common.h (the __host__ / __device__ qualifiers and the PHILOX_* constants come from there).
#pragma once
#include <stdint.h>

#define MB_ROUNDS 6

// common.h's philox4x32_10 (same constants: PHILOX_*) with the high products formed in 64 bits instead of __umulhi, so that the
// host compiles it too; word 0 of the output only.
__host__ __device__ inline uint32_t mb_philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                    uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    return c0;
}

struct mb_perm_key {
    uint32_t seed_lo, seed_hi, epoch_lo, epoch_hi;
    int ha, hb;          // bits of the high / low half
    uint32_t n;          // N - 1 (N <= 2^31)
};

__host__ __device__ inline mb_perm_key mb_perm_make(int64_t seed, int64_t epoch, int64_t N) {
    mb_perm_key k;
    k.seed_lo = (uint32_t)(uint64_t)seed; k.seed_hi = (uint32_t)((uint64_t)seed >> 32);
    k.epoch_lo = (uint32_t)(uint64_t)epoch; k.epoch_hi = (uint32_t)((uint64_t)epoch >> 32);
    k.n = (uint32_t)(N - 1);
    int b = 0;
    while (b < 32 && ((uint64_t)k.n >> b) != 0) ++b;
    k.hb = b / 2;
    k.ha = b - k.hb;
    return k;
}

// one pass of the network over the domain 0..2^(ha+hb)-1
__host__ __device__ inline uint32_t mb_perm_once(const mb_perm_key& k, uint32_t v) {
    const uint32_t ma = (1u << k.ha) - 1u, mb = (1u << k.hb) - 1u;      // ha, hb <= 16
    uint32_t A = v >> k.hb, B = v & mb;
    for (uint32_t r = 0; r < MB_ROUNDS; ++r) {
        if ((r & 1u) == 0) A ^= mb_philox_word0(B, r, k.epoch_lo, k.epoch_hi, k.seed_lo, k.seed_hi) & ma;
        else B ^= mb_philox_word0(A, r, k.epoch_lo, k.epoch_hi, k.seed_lo, k.seed_hi) & mb;
    }
    return (A << k.hb) | B;
}

// source row of position i (0 <= i < N) of the epoch
__host__ __device__ inline int64_t mb_perm_at(const mb_perm_key& k, int64_t i) {
    uint32_t v = mb_perm_once(k, (uint32_t)i);
    const uint64_t domain = (uint64_t)1 << (k.ha + k.hb);
    for (uint64_t walk = 0; v > k.n && walk < domain; ++walk) v = mb_perm_once(k, v);
    return (int64_t)v;
}
