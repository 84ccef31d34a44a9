// The data likelihoods of the Laplace paths, shared by the context route's
// row kernels (k_lap.hip) and the batch's (k_batch_laplace.hip).  Internal linkage: each
// translation unit compiles its own copy.
#pragma once
#include <math.h>

#include "../../include/sgp.h"

namespace {

// The data likelihood of one row: d1 = d log p / df, W = d2, W3 = d3 and the row's log p(y|f)
// term, as the reference writes them.  Everything else in the Laplace kernels is family-free.
template <int FAM>
struct LapLik;

// Poisson with exposure a (derivative_functions_of_data_likelihoods.R:7-61): W = W3 = -a e^f.
// The expressions stand as the kernels held them before the families were split, so this
// instantiation's results are unchanged.
template <>
struct LapLik<SGP_FAM_POISSON> {
  double ai, e;
  __device__ __forceinline__ LapLik(double fi, double /*yi*/, double a) : ai(a), e(exp(fi)) {}
  __device__ __forceinline__ static double expo(const double* av, int64_t i, double ex) {
    return av ? av[i] : ex;
  }
  __device__ __forceinline__ static double logexpo(const double* av, double ai, double lex) {
    return av ? log(ai) : lex;
  }
  __device__ __forceinline__ double W() const { return -ai * e; }
  __device__ __forceinline__ double W3() const { return -ai * e; }
  __device__ __forceinline__ double d1(double yi) const { return -ai * e + yi; }
  __device__ __forceinline__ double logp(double fi, double yi, double lai) const {
    return yi * lai - lgamma(yi + 1.0) - ai * e + yi * fi;
  }
};

// R's log1pexp (nmath/plogis.c, behind plogis(..., log.p = TRUE)): log(1 + e^x) without overflow
__device__ __forceinline__ double log1pexp(double x) {
  if (x <= 18.0) return log1p(exp(x));
  if (x > 33.3) return x;
  return x + exp(-x);
}

// Bernoulli with the logistic link, pi = 1/(1 + e^-f) (my_logistic, laplace_approx_obj_funs.R:
// 178-183).  d1 l.182, W l.108-109 (= obj_fun_bern l.225-226), W3 l.141-142, log p
// obj_fun_bern l.209-210, 249-251.  For y = 1 the reference's W is -pi - pi^2, not the true
// -pi(1 - pi), and W3 is that W's derivative (quirk Q19): reproduced as written.
// The exposure is not read.
template <>
struct LapLik<SGP_FAM_BERNOULLI> {
  double pi, yi;
  __device__ __forceinline__ LapLik(double fi, double y, double /*a*/)
      : pi(1.0 / (1.0 + exp(-fi))), yi(y) {}
  __device__ __forceinline__ static double expo(const double*, int64_t, double) { return 1.0; }
  __device__ __forceinline__ static double logexpo(const double*, double, double) { return 0.0; }
  __device__ __forceinline__ double W() const {
    return (1.0 - 2.0 * pi) * (yi - pi) -
           (yi * ((1.0 - pi) * (1.0 - pi)) + pi * pi + yi * (pi * pi));
  }
  __device__ __forceinline__ double W3() const {
    const double dp = pi * (1.0 - pi);
    return -2.0 * dp * (yi - pi) - dp * (1.0 - 2.0 * pi) -
           (2.0 * yi * (1.0 - pi) * (-dp) + 2.0 * pi * dp + 2.0 * yi * pi * dp);
  }
  __device__ __forceinline__ double d1(double y) const { return y * (1.0 - pi) - pi + y * pi; }
  __device__ __forceinline__ double logp(double fi, double y, double) const {
    return y * -log1pexp(-fi) + (1.0 - y) * -log1pexp(fi);
  }
};

}  // namespace
