// Device helpers shared by the batch kernels (k_batch.hip, k_batch_fitc.hip,
// k_batch_laplace.hip): the fixed-order sums, the sweep operator of the m x m stages and the knot
// distances.  Internal linkage: each translation unit compiles its own copy.
#pragma once
#include <math.h>

#include "sgp_internal.h"

namespace {

constexpr int MM = SGP_BATCH_MMAX;   // 64: the LDS matrices' row stride

// sum of v over the 256 threads in a fixed tree order; red: 256 doubles
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  return red[0];
}

// sum of rec[q * stride], q = 0 .. n - 1, in that order; the loads go out eight at a time
__device__ __forceinline__ double rec_sum(const double* __restrict__ rec, int64_t stride, int n) {
  double s = 0.0;
  int q = 0;
  for (; q + 8 <= n; q += 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = rec[(q + k) * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  for (; q < n; ++q) s += rec[q * stride];
  return s;
}

// The sweep operator on the leading m x m of A (row stride 64, in LDS): after the m sweeps A holds
// -A^-1.  On an SPD matrix the pivot of sweep k is the ratio of the leading minors of order k + 1
// and k (the square of Cholesky's k-th diagonal), so the first pivot that is not positive gives
// chol()'s "leading minor of order k + 1".  Returns 0 or that order; *ld = the log-determinant.
__device__ int sweep_spd(double* A, int m, double* ck, double* ld) {
  const int tid = threadIdx.x;
  double l = 0.0;
  for (int k = 0; k < m; ++k) {
    __syncthreads();
    const double dk = A[k * MM + k];
    if (!(dk > 0.0)) return k + 1;
    l += log(dk);
    if (tid < m) ck[tid] = A[tid * MM + k];   // = row k: A stays symmetric
    __syncthreads();
    const double rd = 1.0 / dk;
    for (int e = tid; e < m * MM; e += 256) {
      const int i = e >> 6, j = e & (MM - 1);
      if (j >= m) continue;
      double v;
      if (i == k) v = j == k ? -rd : ck[j] * rd;
      else if (j == k) v = ck[i] * rd;
      else v = A[i * MM + j] - ck[i] * (ck[j] * rd);
      A[i * MM + j] = v;
    }
  }
  __syncthreads();
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    A[i * MM + j] = -A[i * MM + j];
  }
  __syncthreads();
  *ld = l;
  return 0;
}

// (U_i - U_j) scaled, squared and summed: the exponent's -2 x
__device__ __forceinline__ double knot_dist2(const double* __restrict__ P, int d, int i, int j) {
  double s = 0.0;
  for (int c = 0; c < d; ++c) {
    const double t = (P[BP_U + c * MM + i] - P[BP_U + c * MM + j]) * P[BP_RL + c];
    s = fma(t, t, s);
  }
  return s;
}

}  // namespace
