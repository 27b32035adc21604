/*
 * insider_sample.h — keyed random subsets of [0, p) for the permutation null of the gene-set enrichment
 * (insider_hip_enrichment).
 *
 * Null draw b of size m is the position set { phi(j) : j = 0..m-1 }, phi a keyed bijection of [0, p): a balanced Feistel
 * network of 8 rounds on `bits` bits (the smallest even number >= 2 with 2^bits >= p), walked until the value falls below p
 * (cycle walking: a bijection of [0, 2^bits) restricted to [0, p) this way is a bijection of [0, p), and 2^bits < 4 p keeps
 * the expected walk under four steps).  The round function is insider_h32 of insider_perm.h.  A draw is a pure function of
 * (seed, b, p): it depends neither on the profile nor on the set, the draws of different sizes are nested (size m is a prefix
 * of size m + 1), and any element is computed without the others, so a wave generates a draw one element per lane.
 *
 * With 8 rounds the inclusion frequencies are those of uniform sampling without replacement (chi^2 / df within 1 +- 0.03 at
 * (p, m, draws) = (1000, 50, 20000) and (5000, 100, 20000)); with 4 rounds they are visibly worse.
 *
 * Pure uint32 wrap-around arithmetic: bit-identical in gcc and in hipcc device code.
 */
#ifndef INSIDER_SAMPLE_H
#define INSIDER_SAMPLE_H

#include "insider_perm.h"

#define INSIDER_SAMPLE_ROUNDS 8u

/* Half the width of the Feistel network for [0, p), 2 <= p <= INT32_MAX: bits / 2 with bits the smallest even number >= 2
 * such that 2^bits >= p (1..16). */
INSIDER_HD uint32_t insider_sample_half(uint32_t p)
{
    uint32_t half = 1U;
    while (half < 16U && (1U << (2U * half)) < p) ++half;
    return half;
}

/* Per-(seed, draw) key; uniform across the elements of a draw. */
INSIDER_HD uint32_t insider_sample_key(uint64_t seed, uint32_t b)
{
    uint32_t k = insider_h32((uint32_t)seed ^ 0x9E3779B9U);
    return insider_h32(k ^ (uint32_t)(seed >> 32) ^ (0x85EBCA6BU * b));
}

/* phi(j), 0 <= j < p: element j of the draw with this key. */
INSIDER_HD uint32_t insider_sample_phi(uint32_t key, uint32_t half, uint32_t p, uint32_t j)
{
    const uint32_t mask = (1U << half) - 1U;
    uint32_t x = j;
    do {
        uint32_t L = x >> half, R = x & mask;
        for (uint32_t i = 1U; i <= INSIDER_SAMPLE_ROUNDS; ++i) {
            const uint32_t t = L ^ (insider_h32(R ^ key ^ (0xC2B2AE35U * i)) & mask);
            L = R;
            R = t;
        }
        x = (L << half) | R;
    } while (x >= p);
    return x;
}

/* Start coordinate e = 2 i + d of insider_hip_tsne's drawn map (point i, coordinate d), key = insider_sample_key(seed, 0):
 * u = h32(key ^ 0x27D4EB2F * (e + 1)), y = ((u + 0.5) 2^-32 - 0.5) * 1e-4.  Everything before the last product is exact in
 * fp64, so the value is the same bits wherever it is computed; it lies strictly within +-0.5e-4. */
INSIDER_HD double insider_tsne_draw(uint32_t key, uint32_t e)
{
    const uint32_t u = insider_h32(key ^ (0x27D4EB2FU * (e + 1U)));
    return (((double)u + 0.5) * (1.0 / 4294967296.0) - 0.5) * 1e-4;
}

#endif /* INSIDER_SAMPLE_H */
