// gat_dropout.hpp -- the attention-dropout multiplier of the fused GAT passes as a pure function of (seed, row, column, head).
//
// sparseGatConv drops attention weights between the row sum and the aggregation (gatconv.py:132: the denominator keeps every edge,
// the numerator loses a fraction p of them and the survivors are scaled by 1 / (1 - p)).  The gather passes (gat_kernel.hpp) store
// nothing per edge, so the mask is not stored either: each of the three passes evaluates THIS function for the edges it walks.  The
// forward and the rows pass see edge (i, j) as column j of row i; the transposed pass walks A^T, sees it as column i of row j and
// calls the function with the two ids swapped back -- no edge slot, no permutation lookup.
//
// Keyed on the ids, not on the slot: duplicate (i, j) entries of an adjacency that was not coalesced share one draw.
//
// Generator.  A counter hash, not Philox4x32-10 (layerwise.hip): the row-score forward is VALU bound and 32-bit integer multiplies
// issue at a quarter of the full rate; one Philox call is 40 of them for four heads, every lane group of a row would have to make it,
// and its other three words have no taker when a lane owns one head.  Here a draw is
//       mix( R(i) + k G  ^  rotl( C(j), 5 k + 1 ) ),        mix = a 2-multiply avalanche finaliser of the murmur3 kind
//       R(i) = mix(mix(i ^ seed0) + seed1)                         (x ^= x >> 16; x *= 0x21f0aaad; x ^= x >> 15; x *= 0x735a2d97;
//       C(j) = mix(~j ^ seed1) + seed0                              x ^= x >> 15), G = 0x9E3779B9
// R is per (row, seed), C per (column, seed) -- each a bijection of its full 32-bit id (ids reach 2^27 on RMAT-27 and are admitted up
// to 2^31) -- and only the last mix is per (edge, head): two multiplies.  Whichever id is wave-uniform in a pass (i in the forward and
// rows pass, j in the transposed pass) has its half hoisted out of the edge loop.  The head enters twice, as an odd-constant offset and
// as a rotation of the column half: two edges whose 32-bit states collide for one head (unavoidable: 62 bits of ids, 32 bits of state)
// do not collide for the others, so no two edges share their whole pattern over the heads.  R and C differ in form (i against ~j, the
// seed words in the other order), so (i, j) and (j, i) are unrelated draws.  tests/test_gat_dropout_host.py checks the keep rate and
// the independence between seeds, between heads and between (i, j) and (j, i) to 5 sigma on 10^6 .. 10^7 draws.
//
// Decision: drop iff draw < floor(p 2^32) -- P(drop) is p to within 2^-32 -- and the result is exactly 0.0f or exactly
// (float)(1 / (1 - p)) (the division in double, rounded once: what F.dropout multiplies with) for every one of the 2^32 draws: no
// conversion of the draw to a float is involved.  Host and device evaluate the same integer code: bit-equal by construction
// (dgll_host_gat_dropout_mask / dgll_hip_gat_dropout_mask write the [nnz, heads] multipliers of a CSR for tests and for callers that
// want the mask as a tensor; the training path never materialises it).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DGLL_HD __host__ __device__
#else
#define DGLL_HD
#endif

namespace dgll {

struct GatDropout {
    uint32_t thresh;   // drop iff draw < thresh
    float scale;       // multiplier of a kept edge
};

// p in [0, 1) (the entry points refuse anything else)
DGLL_HD inline GatDropout gat_dropout_params(double p) {
    GatDropout d;
    d.thresh = (uint32_t)(p * 4294967296.0);
    d.scale = (float)(1.0 / (1.0 - p));
    return d;
}

DGLL_HD inline uint32_t gat_dropout_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x21f0aaadu;
    x ^= x >> 15; x *= 0x735a2d97u;
    x ^= x >> 15;
    return x;
}

// the half of the key that belongs to the destination row i / to the source column j
DGLL_HD inline uint32_t gat_dropout_row_key(uint32_t seed0, uint32_t seed1, uint32_t i) { return gat_dropout_mix(gat_dropout_mix(i ^ seed0) + seed1); }
DGLL_HD inline uint32_t gat_dropout_col_key(uint32_t seed0, uint32_t seed1, uint32_t j) { return gat_dropout_mix(~j ^ seed1) + seed0; }

// the 32-bit draw of head k of the edge whose key halves are rk = row_key(i), ck = col_key(j)
DGLL_HD inline uint32_t gat_dropout_draw(uint32_t rk, uint32_t ck, uint32_t k) {
    const uint32_t rot = (5u * k + 1u) & 31u;
    return gat_dropout_mix((rk + k * 0x9E3779B9u) ^ ((ck << rot) | (ck >> ((32u - rot) & 31u))));
}

DGLL_HD inline float gat_dropout_keep(uint32_t draw, GatDropout d) { return draw < d.thresh ? 0.0f : d.scale; }

// Multiplier of edge (row i, column j), head k.
DGLL_HD inline float gat_dropout_multiplier(uint32_t seed0, uint32_t seed1, uint32_t i, uint32_t j, uint32_t k, GatDropout d) {
    return gat_dropout_keep(gat_dropout_draw(gat_dropout_row_key(seed0, seed1, i), gat_dropout_col_key(seed0, seed1, j), k), d);
}
DGLL_HD inline float gat_dropout_multiplier(uint64_t seed, uint32_t i, uint32_t j, uint32_t k, double p) {
    return gat_dropout_multiplier((uint32_t)seed, (uint32_t)(seed >> 32), i, j, k, gat_dropout_params(p));
}

}  // namespace dgll
