// Held-out scoring: the per-row negative log predictive probability (sgp_nlp).
//
// The reference's my_nlp (R/evaluation_functions.R:12-145) integrates, per test row,
//   nlp = -log int p(y | f) N(f; pred_mean, pred_var) df
// with R's integrate() for family = "poisson" (l.84-110) and "bernoulli" (l.30-52), and has the
// closed form -dnorm(y, pred_mean, sqrt(pred_var + tau^2), log = TRUE) for "gaussian" (l.14-20).
// This header is that integral as the kernel computes it, free of HIP: the functions marked
// SGP_HD compile for the device (k_score.hip) and for a host program (tests/nlp/quad_driver.cc),
// which therefore runs the arithmetic the kernel runs.
//
// With mu = pred_mean, s2 = pred_var and h(f) = log p(y | f) - (f - mu)^2 / (2 s2):
//   poisson    log p = y (f + log m) - m e^f - lgamma(y + 1)
//   bernoulli  log p = log sigma(f) (y = 1), log sigma(-f) (y = 0), formed as -softplus(-+f)
// h is strictly concave with h'' <= -1 / s2.  Three fixed-cap steps:
//   (a) the mode fh of h: Newton on h' inside a closed-form bracket, bisecting when a step
//       leaves it;
//   (b) the level-set points a < fh < b with h = h(fh) - C, C = 36: Newton for h(f) = h(fh) - C
//       from fh -+ s sqrt(2 C), which lie outside because h'' <= -1 / s2, moves monotonically
//       inward on a concave h;
//   (c) the N-point midpoint rule on [a, b] of exp(h(x) - h(fh)): the integrand and all its
//       derivatives vanish to rounding at both ends, so the rule converges geometrically.
//   nlp = -(h(fh) + log sum + log((b - a) / N) - log(2 pi s2) / 2), all in log space: an integral
//   below the smallest double still has a finite nlp.
// h(x) - h(fh) is formed as a difference in t = x - fh (no cancellation of two large values).
#ifndef SGP_QUAD_H
#define SGP_QUAD_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SGP_HD __host__ __device__ inline
// the loops stay loops: unrolled, their inlined exp / expm1 bodies cost the kernel registers
#define SGP_QUAD_LOOP _Pragma("unroll 1")
// the row function is inlined into the kernel, whose family is a template constant: called out of
// line it carries both families' code and 180 VGPRs instead of 114
#define SGP_QUAD_ROW __host__ __device__ __forceinline__
#else
#define SGP_HD inline
#define SGP_QUAD_LOOP
#define SGP_QUAD_ROW inline
#endif

// the family argument of sgp_nlp (include/sgp.h: SGP_FAM_*)
constexpr int SGP_QUAD_POISSON = 0, SGP_QUAD_BERNOULLI = 1, SGP_QUAD_GAUSSIAN = 2;

constexpr int SGP_QUAD_N = 128;          // midpoint-rule points
constexpr double SGP_QUAD_C = 36.0;      // level set: exp(-36) ~ 2e-16
constexpr int SGP_QUAD_MODE_ITERS = 60;  // caps: a wave's lanes never wait on one row for long
constexpr int SGP_QUAD_EDGE_ITERS = 80;

// One row's integrand: h around a reference point f0 as d(t) = h(f0 + t) - h(f0) and its
// derivative in t.
struct QuadRow {
  int fam;
  double y;     // poisson: the count; bernoulli: +1 for y = 1, -1 for y = 0
  double mu, is2;   // pred_mean, 1 / pred_var
  double logm;  // poisson: log(exposure)
};

// log sigma(z) = min(z, 0) - log1p(exp(-|z|)); neither tail loses digits
SGP_HD double quad_log_sigmoid(double z) {
  return (z < 0.0 ? z : 0.0) - log1p(exp(-fabs(z)));
}

// log p(y | f) without the poisson -lgamma(y + 1) (constant in f; added once by quad_nlp_row)
SGP_HD double quad_logp(const QuadRow& r, double f) {
  if (r.fam == SGP_QUAD_POISSON) return r.y * (f + r.logm) - exp(f + r.logm);
  return quad_log_sigmoid(r.y * f);
}

// log(y!) for an integer y >= 0 (lgamma(y + 1)): the product below 21 (every k! up to 20! is
// exact in a double), else Stirling's series, whose first dropped term 1 / (1188 y^9) is below
// 2e-15 there.  (The device lgamma costs the kernel half its waves: 256 VGPRs against 114.)
SGP_HD double quad_lfact(double y) {
  if (y < 21.0) {
    double p = 1.0;
    SGP_QUAD_LOOP
    for (double k = 2.0; k <= y; k += 1.0) p *= k;
    return log(p);
  }
  const double r = 1.0 / y, r2 = r * r;
  const double ser = r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0))));
  return y * log(y) - y + 0.5 * log(6.28318530717958647692 * y) + ser;
}

// h'(f) and h''(f)
SGP_HD void quad_dh(const QuadRow& r, double f, double& d1, double& d2) {
  if (r.fam == SGP_QUAD_POISSON) {
    const double lam = exp(f + r.logm);
    d1 = r.y - lam;
    d2 = -lam;
  } else {
    const double z = r.y * f, e = exp(-fabs(z)), q = 1.0 / (1.0 + e);
    d1 = r.y * (z >= 0.0 ? e * q : q);   // +-sigma(-z)
    d2 = -e * q * q;
  }
  d1 -= (f - r.mu) * r.is2;
  d2 -= r.is2;
}

// d(t) = h(f0 + t) - h(f0) and d'(t); lam0 = m exp(f0) (poisson), lp0 = log p at f0 (bernoulli)
SGP_HD double quad_delta(const QuadRow& r, double f0, double aux0, double t, double* slope) {
  const double gq = -t * (t + 2.0 * (f0 - r.mu)) * (0.5 * r.is2);
  const double gs = -(t + (f0 - r.mu)) * r.is2;
  if (r.fam == SGP_QUAD_POISSON) {
    const double em = expm1(t);
    if (slope) *slope = r.y - aux0 * (em + 1.0) + gs;
    return r.y * t - aux0 * em + gq;
  }
  const double z = r.y * (f0 + t), e = exp(-fabs(z));
  if (slope) *slope = r.y * (z >= 0.0 ? e : 1.0) / (1.0 + e) + gs;
  return ((z < 0.0 ? z : 0.0) - log1p(e)) - aux0 + gq;
}

// (a): the mode of h inside [lo, hi] (h' >= 0 at lo, <= 0 at hi)
SGP_HD double quad_mode(const QuadRow& r, double lo, double hi) {
  double f = r.mu < lo ? lo : (r.mu > hi ? hi : r.mu);
  SGP_QUAD_LOOP
  for (int it = 0; it < SGP_QUAD_MODE_ITERS; ++it) {
    double d1, d2;
    quad_dh(r, f, d1, d2);
    if (d1 == 0.0) break;
    if (d1 > 0.0) lo = f;
    else hi = f;
    double fn = f - d1 / d2;
    if (!(fn > lo && fn < hi)) fn = 0.5 * (lo + hi);
    const double step = fabs(fn - f);
    f = fn;
    if (step <= 1e-14 * (1.0 + fabs(f)) || !(hi > lo)) break;
  }
  return f;
}

// (b): one level-set point, from the outer start t0 (sign of t0 = the side)
SGP_HD double quad_edge(const QuadRow& r, double f0, double aux0, double t0) {
  double t = t0;
  SGP_QUAD_LOOP
  for (int it = 0; it < SGP_QUAD_EDGE_ITERS; ++it) {
    double sl;
    const double g = quad_delta(r, f0, aux0, t, &sl) + SGP_QUAD_C;
    // inside 1e-3 of the level (from outside): the rule needs no more of its end points
    if (!(g < -1e-3) || sl == 0.0) break;
    const double tn = t - g / sl;
    // a step is inward and never crosses the mode on a concave h; anything else is rounding
    if (!((t0 > 0.0) ? (tn < t && tn > 0.0) : (tn > t && tn < 0.0))) break;
    t = tn;
  }
  return t;
}

// One row after steps (a) and (b): what the midpoint rule (c) needs.  ok = 0: the row's
// pred_mean is not finite or its variance is not finite or <= 0 (nlp = NaN).
struct QuadPrep {
  QuadRow r;
  double f0, aux0, h0, ta, w, s2;
  int ok;
};

// steps (a) and (b) of one poisson / bernoulli row; m = the exposure (poisson)
SGP_HD QuadPrep quad_prepare(int fam, double y, double mu, double s2, double m) {
  QuadPrep p;
  p.ok = (fabs(mu) <= 1.79769313486231570815e308) && (s2 > 0.0) &&
         (s2 <= 1.79769313486231570815e308);
  if (!p.ok) { mu = 0.0; s2 = 1.0; }   // the lanes of a wave stay together; the result is dropped
  QuadRow& r = p.r;
  r.fam = fam;
  r.mu = mu;
  r.is2 = 1.0 / s2;
  r.logm = 0.0;
  p.s2 = s2;
  double lo, hi, lconst = 0.0;
  if (fam == SGP_QUAD_POISSON) {
    r.y = y;
    r.logm = log(m);
    lconst = -quad_lfact(y);
    if (y > 0.0) {
      const double fy = log(y) - r.logm;   // log p peaks here; the prior at mu
      lo = mu < fy ? mu : fy;
      hi = mu < fy ? fy : mu;
    } else {
      lo = mu - s2 * exp(mu + r.logm);
      hi = mu;
    }
  } else {
    r.y = y > 0.5 ? 1.0 : -1.0;
    lo = mu - s2;
    hi = mu + s2;
  }
  p.f0 = quad_mode(r, lo, hi);
  const double lp0 = quad_logp(r, p.f0);
  p.aux0 = fam == SGP_QUAD_POISSON ? exp(p.f0 + r.logm) : lp0;
  p.h0 = lp0 + lconst - (p.f0 - mu) * (p.f0 - mu) * (0.5 * r.is2);
  const double span = sqrt(2.0 * SGP_QUAD_C * s2);
  p.ta = quad_edge(r, p.f0, p.aux0, -span);
  p.w = (quad_edge(r, p.f0, p.aux0, span) - p.ta) / SGP_QUAD_N;
  return p;
}

// nlp of one poisson / bernoulli row: steps (a), (b), then (c), the rule's points in order
SGP_QUAD_ROW double quad_nlp_row(int fam, double y, double mu, double s2, double m) {
  const QuadPrep p = quad_prepare(fam, y, mu, s2, m);
  double sum = 0.0;
  SGP_QUAD_LOOP
  for (int k = 0; k < SGP_QUAD_N; ++k)
    sum += exp(quad_delta(p.r, p.f0, p.aux0, p.ta + (k + 0.5) * p.w, nullptr));
  if (!p.ok) return (double)NAN;
  return -(p.h0 + log(sum) + log(p.w) - 0.5 * log(6.28318530717958647692 * p.s2));
}

// gaussian: -dnorm(y, pred_mean, sqrt(pred_var + tau^2), log = TRUE); the reference's
// pred_var + tau^2 as written (evaluation_functions.R:19)
SGP_HD double quad_nlp_gaussian(double y, double mu, double s2, double tau) {
  const double v = s2 + tau * tau;
  if (!(fabs(mu) <= 1.79769313486231570815e308) || !(v > 0.0) ||
      !(v <= 1.79769313486231570815e308))
    return (double)NAN;
  const double z = (y - mu) / sqrt(v);
  return 0.5 * log(6.28318530717958647692 * v) + 0.5 * z * z;
}

SGP_HD double quad_nlp(int fam, double y, double mu, double s2, double par) {
  return fam == SGP_QUAD_GAUSSIAN ? quad_nlp_gaussian(y, mu, s2, par)
                                  : quad_nlp_row(fam, y, mu, s2, par);
}

#endif  // SGP_QUAD_H
