// The library's normal stream (sgp_sample_mvn, sgp_joint_nlp, sgp_mc_nlp).
//
// R's stream (rnorm by inversion on Mersenne-Twister, rmvnorm through an eigen-decomposition)
// cannot be reproduced on a device, so the draws come from a counter-based generator of our own,
// defined here and in include/sgp.h so that a host can regenerate every draw:
//   generator  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl 0x9E3779B9, 0xBB67AE85)
//   key        (seed low 32 bits, seed high 32 bits)
//   output     w0..w3 -> a = ((w1 << 32) | w0) >> 12, b = ((w3 << 32) | w2) >> 12,
//              u1 = (a + 0.5) 2^-52, u2 = (b + 0.5) 2^-52 (exact in fp64, inside (0, 1)),
//              r = sqrt(-2 log u1), the pair (r cos(2 pi u2), r sin(2 pi u2))
//   stream 0   (joint draws) draw s, row j: counter (s low, s high, j >> 1, 0); the cosine value
//              for even j, the sine value for odd j
//   stream 1   (per-row Monte Carlo) draw t of row i: counter (q low, q high, i, 1), q = t >> 1;
//              the cosine value for even t, the sine value for odd t
// This header is free of HIP: the functions marked SGP_RNG_HD compile for the device (k_joint.hip)
// and for a host program (tests/joint/rng_driver.cc), which therefore runs the kernel's arithmetic.
#ifndef SGP_RNG_H
#define SGP_RNG_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SGP_RNG_HD __host__ __device__ inline
#else
#define SGP_RNG_HD inline
#endif

constexpr int SGP_RNG_STREAM_JOINT = 0, SGP_RNG_STREAM_ROW = 1;

// Philox4x32-10: ctr (4 words) under key (2 words) -> out (4 words)
SGP_RNG_HD void sgp_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
  uint32_t k0 = key[0], k1 = key[1];
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// the Box-Muller pair of one counter
SGP_RNG_HD void sgp_rng_pair(uint64_t seed, uint64_t c01, uint32_t c2, uint32_t c3, double* zc,
                             double* zs) {
  const uint32_t ctr[4] = {(uint32_t)c01, (uint32_t)(c01 >> 32), c2, c3};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  sgp_philox4x32(ctr, key, w);
  const uint64_t a = (((uint64_t)w[1] << 32) | w[0]) >> 12;
  const uint64_t b = (((uint64_t)w[3] << 32) | w[2]) >> 12;
  const double u1 = ((double)a + 0.5) * 2.220446049250313e-16;   // 2^-52
  const double u2 = ((double)b + 0.5) * 2.220446049250313e-16;
  const double r = sqrt(-2.0 * log(u1));
  const double th = 6.283185307179586 * u2;
  *zc = r * cos(th);
  *zs = r * sin(th);
}

// stream 0: the normal of draw s, row j
SGP_RNG_HD double sgp_rng_joint(uint64_t seed, uint64_t s, uint64_t j) {
  double zc, zs;
  sgp_rng_pair(seed, s, (uint32_t)(j >> 1), SGP_RNG_STREAM_JOINT, &zc, &zs);
  return (j & 1) ? zs : zc;
}

// stream 1: draw t of row i
SGP_RNG_HD double sgp_rng_row(uint64_t seed, uint64_t t, uint64_t i) {
  double zc, zs;
  sgp_rng_pair(seed, t >> 1, (uint32_t)i, SGP_RNG_STREAM_ROW, &zc, &zs);
  return (t & 1) ? zs : zc;
}

#endif  // SGP_RNG_H
