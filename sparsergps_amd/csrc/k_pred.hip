// The resident predictor's tile route (sgp_predictor_*, include/sgp.h).
//
// Every prediction method reduces to, per row i with k_i = K(x_i, U) (no nugget),
//   mean_i = mu_i + k_i^T w,     var_i = c0 + k_i^T T22 k_i,     T22 symmetric (m x m).
// With the knots in column blocks of 128 (nb = mp / 128) and S = 1/2 (T22 + T22^T),
//   k^T S k = sum_cb [ sum_{kb < cb} 2 k_kb^T S[kb,cb] k_cb + k_cb^T S[cb,cb] k_cb ]
//           = sum_cb  k_cb . (sum_{kb <= cb} A'[kb,cb]^T k_kb),
//   A'[kb,cb] = 2 S[kb,cb] (kb < cb),  S[cb,cb] (kb == cb),  0 (kb > cb)        (k_pred_sym)
// so the tile (row tile ti, column block cb) needs the k range 0 .. 128 (cb + 1) only:
// nb (nb + 1) / 2 block products per row tile instead of the nb^2 of the full quadratic form.
//
//  k_pred_sym     A' from T22, once per predictor.
//  k_pred_tile    P = K[ti, 0 .. 128 (cb + 1)) A'[0 .. 128 (cb + 1), cb] on f64 MFMA accumulators
//                 (128 x 128 tile, BK = 16, two-stage LDS: the k-loop of k_contract's row-quadratic
//                 instantiation, k_mfma.hip), then from one set of fragment loads of K[ti, cb]
//                 both the row dot sum_j K_ij P_ij and the mean's partial sum_j K_ij w_j, written
//                 to two [cb][row] slabs.
//  k_pred_rows    the slabs summed over cb in ascending order; mean = mu + ., var = c0 + . .
//
// No atomics; every sum has a fixed order that depends on the knot index only, so a row's result
// does not depend on the chunk it arrives in, its place in a tile, the grid or the repeat.
//
// MFMA f64 16x16x4 lane maps (cdna_hip_programming.md Sec.3):
//   A: lane l holds A[l&15][l>>4];  B: lane l holds B[l>>4][l&15];
//   C/D: register r of lane l is C[(l>>4) + 4r][l&15].
#include "sgp_internal.h"

namespace {

constexpr int T128 = 128;
constexpr int BK = 16;
constexpr int SB = 144;   // LDS row stride of the [k][128] B image (k_mfma.hip: 2*144 % 64 == 32)
constexpr int SA = 17;    // LDS row stride of the [128][16] A image (odd: conflict-free reads)
constexpr int A_SZ = T128 * SA;   // 2176 (keeps the B image 16-byte aligned)
constexpr int B_SZ = BK * SB;     // 2304
constexpr int PRED_LDS = 2 * (A_SZ + B_SZ);

// Issue order of one k-step as a scheduling request (k_mfma.hip mfma_interleave with the
// contraction's settings): each of the 64 MFMAs is followed by at most one global load (the
// first 8), one LDS read (the first 32) and, in the last 8 slots, one LDS store.
__device__ __forceinline__ void pred_interleave() {
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                      // MFMA
    if (i < 8) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);           // VMEM read
    if (i < 32) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);          // DS read
    if (i >= 56) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);         // DS write
  }
}

// A'[k][j] (row-major mp x mp; see the head of the file)
__global__ void __launch_bounds__(256)
k_pred_sym(const double* __restrict__ T, int64_t mp, double* __restrict__ Ap) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= mp * mp) return;
  const int64_t k = e / mp, j = e - k * mp;
  const int64_t kb = k / T128, cb = j / T128;
  const double s = T[k * mp + j] + T[j * mp + k];
  Ap[e] = kb < cb ? s : (kb == cb ? 0.5 * s : 0.0);
}

// One (row tile, column block) tile per workgroup, column-block-major with the last column block
// (the longest k range, 8 nb steps) first and the first (8 steps) last: longest work first, so
// the launch ends on its shortest tiles.  Row-tile-major order (a row tile's nb tiles adjacent
// on one XCD, its K panel shared in L2) left a tail of long tiles behind every chunk's launch and
// cost 26.3 ms against 18.7 ms at C3's rows with m = 1024 (profiles/predictor/README.md).
__global__ void __launch_bounds__(256, 2)
k_pred_tile(const double* __restrict__ K, const double* __restrict__ Ap,
            const double* __restrict__ w, int64_t ld, int64_t mp, double* __restrict__ qslab,
            double* __restrict__ yslab) {
  __shared__ __attribute__((aligned(16))) double lds[PRED_LDS];
  const int nb = (int)(mp / T128);
  const int64_t nti = gridDim.x / nb;
  const int64_t ti = blockIdx.x % nti;
  const int cb = nb - 1 - (int)(blockIdx.x / nti);
  const int64_t i0 = ti * T128, j0 = (int64_t)cb * T128;
  const int ke = (cb + 1) * (T128 / BK);

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wr = wv >> 1, wc = wv & 1;

  d4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};

  // A loader: 128 rows x 16 k, thread -> (row = tid>>1, 8 doubles at (tid&1)*8)
  const int arow = tid >> 1, acol = (tid & 1) * 8;
  const double2* gA = reinterpret_cast<const double2*>(K + (i0 + arow) * mp + acol);
  // B loader: 16 k x 128 cols, thread -> (k = tid>>4, double2 columns (tid&15) + 16 q)
  const int bk = tid >> 4, bc = tid & 15;
  const double2* gB = reinterpret_cast<const double2*>(Ap + (int64_t)bk * mp + j0) + bc;
  const int64_t bstep = BK * mp / 2;
  double2 va0, va1, va2, va3, vb0, vb1, vb2, vb3;

#define PRED_GLOAD(step)                                                         \
  {                                                                              \
    const int64_t oa_ = (int64_t)(step) * (BK / 2), ob_ = (int64_t)(step) * bstep; \
    va0 = gA[oa_]; va1 = gA[oa_ + 1]; va2 = gA[oa_ + 2]; va3 = gA[oa_ + 3];      \
    vb0 = gB[ob_]; vb1 = gB[ob_ + 16]; vb2 = gB[ob_ + 32]; vb3 = gB[ob_ + 48];   \
  }
#define PRED_SSTORE(buf)                                                         \
  {                                                                              \
    double* As_ = lds + (buf) * (A_SZ + B_SZ);                                   \
    double* pa_ = &As_[arow * SA + acol];                                        \
    double2* pb_ = reinterpret_cast<double2*>(&As_[A_SZ + bk * SB]) + bc;        \
    pa_[0] = va0.x; pa_[1] = va0.y; pa_[2] = va1.x; pa_[3] = va1.y;              \
    pa_[4] = va2.x; pa_[5] = va2.y; pa_[6] = va3.x; pa_[7] = va3.y;              \
    pb_[0] = vb0; pb_[16] = vb1; pb_[32] = vb2; pb_[48] = vb3;                   \
  }

  PRED_GLOAD(0);
  PRED_SSTORE(0);
  __syncthreads();
  for (int step = 0; step < ke; ++step) {
    const int cur = step & 1;
    PRED_GLOAD(step + 1 < ke ? step + 1 : step);   // the last step reloads its own slice
    const double* As = lds + cur * (A_SZ + B_SZ);
    const double* Bs = As + A_SZ;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int kx = kk * 4 + (lane >> 4);
      double af[4], bf[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        af[f] = As[(wr * 64 + f * 16 + (lane & 15)) * SA + kx];
        bf[f] = Bs[kx * SB + wc * 64 + f * 16 + (lane & 15)];
      }
#pragma unroll
      for (int fm = 0; fm < 4; ++fm)
#pragma unroll
        for (int fn = 0; fn < 4; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[fm], bf[fn], acc[fm][fn], 0, 0, 0);
    }
    PRED_SSTORE(cur ^ 1);   // on the last step into the idle buffer
    pred_interleave();
    __syncthreads();
  }
#undef PRED_GLOAD
#undef PRED_SSTORE

  // ---------------- epilogue: row dots with K[ti, cb] and the mean's partial ----------------
  // (the loop's last barrier has passed: the LDS images are free)
  double* s_q = lds;                 // [2][128]: the two column halves (wc)
  double* s_y = lds + 2 * T128;      // [2][128]
  const double* Kt = K + i0 * mp + j0;
  double wf[4];
#pragma unroll
  for (int fn = 0; fn < 4; ++fn) wf[fn] = w[j0 + wc * 64 + fn * 16 + (lane & 15)];
  // per lane: 16 rows (fm, q) x 4 cols (fn) -> row sums over this wave's 64 columns
#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
    double kv[4][4];   // the 16 K values of this row fragment, issued together
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int fn = 0; fn < 4; ++fn)
        kv[q][fn] = Kt[(int64_t)(wr * 64 + fm * 16 + (lane >> 4) + 4 * q) * mp + wc * 64 +
                       fn * 16 + (lane & 15)];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = wr * 64 + fm * 16 + (lane >> 4) + 4 * q;
      double v = 0.0, y = 0.0;
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) {
        v = fma(kv[q][fn], acc[fm][fn][q], v);   // K = 0 in padded rows and columns
        y = fma(kv[q][fn], wf[fn], y);
      }
      v += __shfl_xor(v, 1, 64);
      y += __shfl_xor(y, 1, 64);
      v += __shfl_xor(v, 2, 64);
      y += __shfl_xor(y, 2, 64);
      v += __shfl_xor(v, 4, 64);
      y += __shfl_xor(y, 4, 64);
      v += __shfl_xor(v, 8, 64);
      y += __shfl_xor(y, 8, 64);
      if ((lane & 15) == 0) {
        s_q[wc * T128 + row] = v;
        s_y[wc * T128 + row] = y;
      }
    }
  }
  __syncthreads();
  if (tid < T128) {
    qslab[(int64_t)cb * ld + i0 + tid] = s_q[tid] + s_q[T128 + tid];
  } else {
    const int t = tid - T128;
    yslab[(int64_t)cb * ld + i0 + t] = s_y[t] + s_y[T128 + t];
  }
}

__global__ void __launch_bounds__(256)
k_pred_rows(const double* __restrict__ qslab, const double* __restrict__ yslab, int nb, int64_t ld,
            const double* __restrict__ mu, double c0, int64_t n, double* __restrict__ pm,
            double* __restrict__ pv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double q = 0.0, y = 0.0;
  for (int cb = 0; cb < nb; ++cb) {
    q += qslab[(int64_t)cb * ld + i];
    y += yslab[(int64_t)cb * ld + i];
  }
  pm[i] = mu[i] + y;
  pv[i] = c0 + q;
}

}  // namespace

hipError_t launch_pred_sym(const double* T22, int64_t mp, double* Ap, hipStream_t s) {
  if (mp < T128 || mp % T128) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pred_sym, dim3((unsigned)((mp * mp + 255) / 256)), dim3(256), 0, s, T22, mp,
                     Ap);
  return hipGetLastError();
}

hipError_t launch_pred_tiles(const double* K, const double* Ap, const double* w, int64_t n,
                             int64_t n_pad, int64_t ld, int64_t mp, const double* mu, double c0,
                             double* qslab, double* yslab, double* pm, double* pv,
                             hipStream_t s) {
  if (n < 1 || n > n_pad || n_pad % T128 || n_pad > ld || mp < T128 || mp % T128)
    return hipErrorInvalidValue;
  const int64_t nwg = (n_pad / T128) * (mp / T128);
  if (nwg > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pred_tile, dim3((unsigned)nwg), dim3(256), 0, s, K, Ap, w, ld, mp, qslab,
                     yslab);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pred_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, qslab, yslab,
                     (int)(mp / T128), ld, mu, c0, n, pm, pv);
  return hipGetLastError();
}
