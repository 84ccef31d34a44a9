// Joint predictive scoring and GP draws (sgp_sample_mvn, sgp_joint_nlp, sgp_joint_kl, sgp_mc_nlp;
// DESIGN.md sec. 0l): what the reference does with mvtnorm::rmvnorm / dmvnorm and an R apply over
// the draws (R/evaluation_functions.R:21-26, 53-80, 120-133, 153-164).
//
// dense_chol        A = L L^T, right-looking in 64-wide steps, one launch per stage: the 64 x 64
//                   diagonal block is factored and its factor inverted in LDS by one wave
//                   (k_chol_diag), the panel below it is A_panel inv(L_kk)^T and the trailing
//                   update A -= L_panel L_panel^T (lower blocks only), both on launch_gemm64.
//                   The first non-positive pivot's 1-based order goes to the status word (R's
//                   chol() leading-minor order, as the Gauss-Jordan chains report it).
// chol_solve_lower  X = L^-1 B by block rows on launch_gemm64 and the stored diagonal inverses.
// k_joint_fill      Z (n_p x S_c) from the normal stream (sgp_rng.h) and F = mean in every column;
//                   launch_joint_product then adds L Z to F per block-row panel of L, K cut at
//                   the panel's last non-zero column.
// k_joint_score     per draw, sum_i log p(y_i | f_i) over the n real rows in row order.
// k_joint_stats     one block over the whole S-vector: lmax, mean(w), sd(w), w = exp(ll - lmax).
// k_mc_rows         the per-row Monte Carlo of my_nlp(family = "bernoulli", mc = TRUE), a lane per row.
// Every reduction has a fixed shape: results are bit-identical on repeat and independent of the
// chunk length and of the grid.  No atomics but the status word's compare-and-swap.
#include <math.h>

#include "sgp_internal.h"
#include "sgp_quad.h"
#include "sgp_rng.h"

namespace {

constexpr int CH_LS = 65;    // LDS row stride (doubles) of the 64 x 64 images: odd, conflict-free
constexpr int JOINT_PANEL = 256;   // block-row panel of L per product launch

// dst (np x np, row-major, full symmetric) from the lower triangle of the column-major src
// (n x n, ld lds): dst_ij = src[max(i,j) + min(i,j) lds] (+ diag_add on the diagonal), padded
// with the identity
__global__ void __launch_bounds__(256) k_chol_prep(const double* __restrict__ src, int64_t n,
                                                   int64_t lds, double diag_add,
                                                   double* __restrict__ dst, int64_t np) {
  const int64_t total = np * np;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / np, j = e - i * np;
    double v;
    if (i < n && j < n) {
      const int64_t hi = i > j ? i : j, lo = i > j ? j : i;
      v = src[hi + lo * lds];
      if (i == j) v += diag_add;
    } else {
      v = (i == j) ? 1.0 : 0.0;
    }
    dst[e] = v;
  }
}

// Stage k's diagonal block: the lower triangle of the 64 x 64 block of A at (k, k) -> its
// Cholesky factor (L's block, strict upper triangle zero), the factor's inverse (Li: 64 x 64
// row-major) and *logd = sum log L_jj.  One wave; lane t owns row t (factor) and column t (inverse).
__global__ void __launch_bounds__(64) k_chol_diag(const double* __restrict__ A, int64_t lda, int k,
                                                  double* __restrict__ L, int64_t ldl,
                                                  double* __restrict__ Li,
                                                  double* __restrict__ logd,
                                                  int* __restrict__ status) {
  // Both loops are fully unrolled with the lane's row (then its column of the inverse) in
  // registers: per step one LDS write of the new column and broadcast reads of it, the updates
  // independent of each other.  With the row left in LDS (a read-modify-write per element, loop
  // bounds that differ per lane) a block took ~170 us and the factor of n = 4096 12.2 ms
  // (profiles/joint/README.md).
  __shared__ double a[64 * CH_LS];
  __shared__ double col[64];
  const int t = threadIdx.x;
  const int64_t o = (int64_t)k * 64;
  const double* Ab = A + o * lda + o;
  for (int r = 0; r < 64; ++r) a[r * CH_LS + t] = (t <= r) ? Ab[(int64_t)r * lda + t] : 0.0;
  __syncthreads();
  int first_bad = 0;
  double row[64];   // row t; the entries right of the diagonal are never used
#pragma unroll
  for (int c = 0; c < 64; ++c) row[c] = a[t * CH_LS + c];
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    double d = __shfl(row[j], j, 64);
    if (!(d > 0.0) || !(fabs(d) <= 1.79769313486231570815e308)) {
      // the leading minor of order o + j + 1 is not positive definite; go on with a harmless
      // pivot (recorded, not reported here: a branch per unrolled step cost 2023 spilled VGPRs)
      first_bad = first_bad ? first_bad : j + 1;
      d = 1.0;
    }
    const double sj = sqrt(d);
    const double l = (t == j) ? sj : row[j] / sj;   // L_tj (t >= j)
    row[j] = l;
    col[t] = l;
    __syncthreads();
#pragma unroll
    for (int c = j + 1; c < 64; ++c) row[c] -= l * col[c];
    __syncthreads();   // col is rewritten by the next step
  }
  if (t == 0 && first_bad) atomicCAS(status, 0, (int)(o + first_bad));
#pragma unroll
  for (int c = 0; c < 64; ++c) a[t * CH_LS + c] = (c <= t) ? row[c] : 0.0;
  __syncthreads();
  // column t of inv(L): forward substitution of L x = e_t
  // (column by column: x_p is final once the columns before p are taken off, and the updates of
  // a step are independent; the compiler barrier keeps a step's LDS reads inside the step)
  double x[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) x[i] = (i == t) ? 1.0 : 0.0;
#pragma unroll
  for (int p = 0; p < 64; ++p) {
    x[p] = x[p] / a[p * CH_LS + p];
#pragma unroll
    for (int i = p + 1; i < 64; ++i) x[i] -= a[i * CH_LS + p] * x[p];
    asm volatile("" ::: "memory");
  }
  double* Lb = L + o * ldl + o;
#pragma unroll
  for (int r = 0; r < 64; ++r) {
    Lb[(int64_t)r * ldl + t] = a[r * CH_LS + t];
    Li[r * 64 + t] = x[r];
  }
  double lg = log(a[t * CH_LS + t]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lg += __shfl_xor(lg, off, 64);
  if (t == 0) logd[k] = lg;
}

// Z and F of one chunk: work item (jp, s), s fastest, fills rows 2 jp and 2 jp + 1 of column s
// from one Philox counter.  Columns >= sc and rows >= n of Z are zero; F = mean (0 past n).
__global__ void __launch_bounds__(256) k_joint_fill(uint64_t seed, int64_t s0, int64_t sc,
                                                    int64_t ldz, int64_t n, int64_t np,
                                                    const double* __restrict__ mean,
                                                    double* __restrict__ Z,
                                                    double* __restrict__ F) {
  const int64_t total = (np / 2) * ldz;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int64_t jp = e / ldz, s = e - jp * ldz, r0 = 2 * jp, r1 = r0 + 1;
    double zc = 0.0, zs = 0.0;
    if (s < sc && r0 < n) {
      sgp_rng_pair(seed, (uint64_t)(s0 + s), (uint32_t)jp, SGP_RNG_STREAM_JOINT, &zc, &zs);
      if (r1 >= n) zs = 0.0;
    }
    Z[r0 * ldz + s] = zc;
    Z[r1 * ldz + s] = zs;
    F[r0 * ldz + s] = r0 < n ? mean[r0] : 0.0;
    F[r1 * ldz + s] = r1 < n ? mean[r1] : 0.0;
  }
}

// ll[s] = sum_i log p(y_i | F_is) over i < n.  A workgroup takes 64 draws; its wave r adds rows
// r, r + SCORE_WAVES, ... in row order (a lane per draw: the reads of a row are one 512-byte
// line), and the SCORE_WAVES partial sums of a draw are added in wave order.  The shape is fixed,
// so ll does not depend on the chunk or the grid.  With one lane per draw and no row split a
// chunk of 8192 draws filled an eighth of the device's SIMDs with one wave each (n = 4096,
// S = 1e5: 37.6 ms of scoring beside 49.5 ms of products; profiles/joint/README.md).
// aux: poisson's per-row {log m_i, m_i, log(y_i!)} (3 n values), unused for bernoulli
constexpr int SCORE_WAVES = 8;
template <int FAM>
__global__ void __launch_bounds__(64 * SCORE_WAVES)
k_joint_score(const double* __restrict__ y, const double* __restrict__ aux, int64_t n,
              const double* __restrict__ F, int64_t ldf, int64_t sc, double* __restrict__ ll) {
  __shared__ double part[SCORE_WAVES][64];
  const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int64_t ntile = (sc + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t s = tile * 64 + lane;
    double acc = 0.0;
    if (s < sc) {
      for (int64_t i = r; i < n; i += SCORE_WAVES) {
        const double f = F[i * ldf + s];
        const double yi = y[i];
        if (FAM == SGP_QUAD_BERNOULLI) {
          acc += quad_log_sigmoid((2.0 * yi - 1.0) * f);
        } else {
          acc += yi * (f + aux[i]) - aux[n + i] * exp(f) - aux[2 * n + i];
        }
      }
    }
    part[r][lane] = acc;
    __syncthreads();
    if (r == 0 && s < sc) {
      double t = part[0][lane];
#pragma unroll
      for (int q = 1; q < SCORE_WAVES; ++q) t += part[q][lane];
      ll[s] = t;
    }
    __syncthreads();   // part is rewritten by the next tile
  }
}

constexpr int ST_THREADS = 1024;
// fixed-order sum (or max) over the block's 1024 threads; valid in every thread.  red: 16 doubles
template <bool MAX>
__device__ __forceinline__ double stats_block(double v, double* red) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = MAX ? fmax(v, o) : v + o;
  }
  __syncthreads();   // the previous use of red
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
  for (int q = 1; q < ST_THREADS / 64; ++q) t = MAX ? fmax(t, red[q]) : t + red[q];
  return t;
}

// out = {lmax, mean(w), sd(w)} over the S values of ll, w = exp(ll - lmax); sd in R's n - 1 form
// (NaN at S = 1), the squares taken about the mean in a second pass
__global__ void __launch_bounds__(ST_THREADS) k_joint_stats(const double* __restrict__ ll,
                                                            int64_t S, double* __restrict__ out) {
  __shared__ double red[ST_THREADS / 64];
  const double ninf = -__builtin_huge_val();
  double m = ninf;
  for (int64_t s = threadIdx.x; s < S; s += ST_THREADS) m = fmax(m, ll[s]);
  const double lmax = stats_block<true>(m, red);
  const bool dead = !(lmax > ninf);   // every draw has probability 0
  double a = 0.0;
  for (int64_t s = threadIdx.x; s < S; s += ST_THREADS) a += dead ? 0.0 : exp(ll[s] - lmax);
  const double mean = stats_block<false>(a, red) / (double)S;
  double q = 0.0;
  for (int64_t s = threadIdx.x; s < S; s += ST_THREADS) {
    const double d = (dead ? 0.0 : exp(ll[s] - lmax)) - mean;
    q += d * d;
  }
  const double ss = stats_block<false>(q, red);
  if (threadIdx.x == 0) {
    out[0] = lmax;
    out[1] = mean;
    out[2] = sqrt(ss / (double)(S - 1));
  }
}

// p(y | f) of a bernoulli response in linear space: 1 / (1 + exp(-(2y - 1) f))
__device__ __forceinline__ double bern_prob(double ysign, double f) {
  return 1.0 / (1.0 + exp(-ysign * f));
}

// my_nlp(family = "bernoulli", mc = TRUE): row i draws S values f = pred_mean + sqrt(pred_var) z
// from stream 1, ll = p(y | f); nlp = -log mean(ll), mcsd = sd(ll) (n - 1 form), in linear space
// as the reference.  The stream is generated twice (mean, then squares about it): nothing is stored.
__global__ void __launch_bounds__(256) k_mc_rows(uint64_t seed, const double* __restrict__ y,
                                                 const double* __restrict__ pm,
                                                 const double* __restrict__ pv, int64_t n,
                                                 int64_t S, double* __restrict__ nlp,
                                                 double* __restrict__ mcsd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double ys = 2.0 * y[i] - 1.0, mu = pm[i], sd = sqrt(pv[i]);
  const int64_t nq = (S + 1) / 2;
  double acc = 0.0;
  for (int64_t q = 0; q < nq; ++q) {
    double zc, zs;
    sgp_rng_pair(seed, (uint64_t)q, (uint32_t)i, SGP_RNG_STREAM_ROW, &zc, &zs);
    acc += bern_prob(ys, mu + sd * zc);
    if (2 * q + 1 < S) acc += bern_prob(ys, mu + sd * zs);
  }
  const double mean = acc / (double)S;
  double ss = 0.0;
  for (int64_t q = 0; q < nq; ++q) {
    double zc, zs;
    sgp_rng_pair(seed, (uint64_t)q, (uint32_t)i, SGP_RNG_STREAM_ROW, &zc, &zs);
    double d = bern_prob(ys, mu + sd * zc) - mean;
    ss += d * d;
    if (2 * q + 1 < S) {
      d = bern_prob(ys, mu + sd * zs) - mean;
      ss += d * d;
    }
  }
  nlp[i] = -log(mean);
  mcsd[i] = sqrt(ss / (double)(S - 1));
}

// out[s + S j] = the normal of draw s, row j of the given stream (sgp_diag_normals)
__global__ void __launch_bounds__(256) k_normals(uint64_t seed, int stream, int64_t S, int64_t n,
                                                 double* __restrict__ out) {
  const int64_t total = S * n;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int64_t j = e / S, s = e - j * S;
    out[e] = stream == SGP_RNG_STREAM_JOINT ? sgp_rng_joint(seed, (uint64_t)s, (uint64_t)j)
                                            : sgp_rng_row(seed, (uint64_t)s, (uint64_t)j);
  }
}

unsigned grid_for(int64_t items, int max_blocks) {
  int64_t g = (items + 255) / 256;
  if (g > max_blocks) g = max_blocks;
  return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace

hipError_t launch_chol_prep(const double* src, int64_t n, int64_t lds, double diag_add,
                            double* dst, int64_t np, hipStream_t s) {
  if (n < 1 || np < n || np % 64 || lds < n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_chol_prep, dim3(grid_for(np * np, 8192)), dim3(256), 0, s, src, n, lds,
                     diag_add, dst, np);
  return hipGetLastError();
}

hipError_t dense_chol(double* A, int64_t np, double* L, double* Linv, double* logd, int* status,
                      hipStream_t s) {
  if (np < 64 || np % 64 || !A || !L || !Linv || !logd || !status || A == L)
    return hipErrorInvalidValue;
  const int nb = (int)(np / 64);
  hipError_t e = hipMemsetAsync(L, 0, sizeof(double) * (size_t)np * (size_t)np, s);
  for (int k = 0; k < nb && e == hipSuccess; ++k) {
    const int64_t o = (int64_t)k * 64, rem = np - o - 64;
    double* Li = Linv + (int64_t)k * 4096;
    hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(64), 0, s, A, np, k, L, np, Li, logd, status);
    e = hipGetLastError();
    if (e != hipSuccess || rem == 0) break;
    double* Lp = L + (o + 64) * np + o;   // the panel below the diagonal block
    e = launch_gemm64(false, true, false, rem, 64, 64, 1.0, A + (o + 64) * np + o, np, Li, 64, 0.0,
                      Lp, np, s);
    if (e != hipSuccess) break;
    e = launch_gemm64(false, true, true, rem, rem, 64, -1.0, Lp, np, Lp, np, 1.0,
                      A + (o + 64) * np + o + 64, np, s);
  }
  return e;
}

hipError_t chol_solve_lower(const double* L, const double* Linv, int64_t np, double* B, int64_t N,
                            double* X, hipStream_t s) {
  if (np < 64 || np % 64 || N < 64 || N % 64 || B == X) return hipErrorInvalidValue;
  const int nb = (int)(np / 64);
  hipError_t e = hipSuccess;
  for (int k = 0; k < nb && e == hipSuccess; ++k) {
    const int64_t o = (int64_t)k * 64;
    if (k > 0)
      e = launch_gemm64(false, false, false, 64, N, o, -1.0, L + o * np, np, X, N, 1.0, B + o * N,
                        N, s);
    if (e == hipSuccess)
      e = launch_gemm64(false, false, false, 64, N, 64, 1.0, Linv + (int64_t)k * 4096, 64,
                        B + o * N, N, 0.0, X + o * N, N, s);
  }
  return e;
}

hipError_t launch_joint_fill(uint64_t seed, int64_t s0, int64_t sc, int64_t ldz, int64_t n,
                             int64_t np, const double* mean, double* Z, double* F,
                             int max_blocks, hipStream_t s) {
  if (sc < 1 || ldz < sc || ldz % 64 || n < 1 || np < n || np % 64 || max_blocks < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_joint_fill, dim3(grid_for((np / 2) * ldz, max_blocks)), dim3(256), 0, s,
                     seed, s0, sc, ldz, n, np, mean, Z, F);
  return hipGetLastError();
}

hipError_t launch_joint_product(const double* L, int64_t np, const double* Z, double* F,
                                int64_t ldz, hipStream_t s) {
  hipError_t e = hipSuccess;
  for (int64_t i0 = 0; i0 < np && e == hipSuccess; i0 += JOINT_PANEL) {
    const int64_t M = np - i0 < JOINT_PANEL ? np - i0 : JOINT_PANEL;
    e = launch_gemm64(false, false, false, M, ldz, i0 + M, 1.0, L + i0 * np, np, Z, ldz, 1.0,
                      F + i0 * ldz, ldz, s);
  }
  return e;
}

hipError_t launch_joint_score(int fam, const double* y, const double* aux, int64_t n,
                              const double* F, int64_t ldf, int64_t sc, double* ll,
                              int max_blocks, hipStream_t s) {
  if (n < 1 || sc < 1 || ldf < sc || max_blocks < 1) return hipErrorInvalidValue;
  const int64_t ntile = (sc + 63) / 64;
  const dim3 grid((unsigned)(ntile < max_blocks ? ntile : max_blocks)), block(64 * SCORE_WAVES);
  if (fam == SGP_QUAD_BERNOULLI)
    hipLaunchKernelGGL(k_joint_score<SGP_QUAD_BERNOULLI>, grid, block, 0, s, y, aux, n, F, ldf,
                       sc, ll);
  else if (fam == SGP_QUAD_POISSON && aux)
    hipLaunchKernelGGL(k_joint_score<SGP_QUAD_POISSON>, grid, block, 0, s, y, aux, n, F, ldf,
                       sc, ll);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_joint_stats(const double* ll, int64_t S, double* out, hipStream_t s) {
  if (S < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_joint_stats, dim3(1), dim3(ST_THREADS), 0, s, ll, S, out);
  return hipGetLastError();
}

hipError_t launch_mc_rows(uint64_t seed, const double* y, const double* pm, const double* pv,
                          int64_t n, int64_t S, double* nlp, double* mcsd, hipStream_t s) {
  if (n < 1 || S < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mc_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, seed, y, pm,
                     pv, n, S, nlp, mcsd);
  return hipGetLastError();
}

hipError_t launch_normals(uint64_t seed, int stream, int64_t S, int64_t n, double* out,
                          hipStream_t s) {
  if (S < 1 || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_normals, dim3(grid_for(S * n, 8192)), dim3(256), 0, s, seed, stream, S, n,
                     out);
  return hipGetLastError();
}
