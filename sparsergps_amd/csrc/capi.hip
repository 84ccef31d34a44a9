// C ABI of libsgp.so (include/sgp.h): context management and the fused VI evaluation.
//
// One evaluation of sgp_eval_vi == one optimizer-iteration body of the reference's
// norm_grad_ascent_vi (R/vi_functions.R:1089-1128): build K12/K22 at (theta, U), the ELBO
// (elbo_fun, vi_functions.R:64-121) and its gradient w.r.t. log(theta)
// (delbo_dcov_par, vi_functions.R:126-602).  The reference evaluates the gradient as
// P separate n x m^2 pipelines; this implementation uses the adjoint form
//     S = K^T K, t = K^T r (one SYRK)              -> every m x m quantity
//     G = alpha u^T + K P (one GEMM) contracted with dK/dtheta in the epilogue
// which is algebraically identical and needs ~3 n m^2 flops in total.
#include <math.h>

#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sgp.h"
#include "../../include/sgp_diag.h"
#include "sgp_internal.h"
#include "sgp_quad.h"

#ifdef SGP_HOST_PROBE
// entry, before the readback's synchronisation, after it, exit of the last sgp_eval_vi
// (CLOCK_MONOTONIC seconds: Python's time.perf_counter reads the same clock)
extern "C" __attribute__((visibility("default"))) double sgp_probe_t[4] = {0.0, 0.0, 0.0, 0.0};
#endif
#include "sgp_probe.h"
#include "sgp_multi.h"

namespace {

thread_local std::string g_err;

void set_err(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      set_err("HIP error '%s' at %s:%d", hipGetErrorString(e_), __FILE__, __LINE__);      \
      return SGP_EHIP;                                                                     \
    }                                                                                      \
  } while (0)

// Entry points a multi-device context (sgp_ctx_create_multi) answers through multi.hip, and the
// ones it refuses (their reductions and streams are internal to it)
#define MULTI_FWD(c, call)                   \
  do {                                       \
    if ((c) && (c)->multi) return (call);    \
  } while (0)
#define MULTI_REFUSE(c, name)                                                                  \
  do {                                                                                         \
    if ((c) && (c)->multi) {                                                                   \
      set_err("%s is not available on a multi-device context (sgp_ctx_create_multi runs its " \
              "reductions inside the library)", name);                                         \
      return SGP_EINVAL;                                                                       \
    }                                                                                          \
  } while (0)

int multi_bad_args() {
  set_err("invalid arguments");
  return SGP_EINVAL;
}

inline int64_t round_up(int64_t v, int64_t q) { return (v + q - 1) / q * q; }

int num_ls(int kernel, int d) { return kernel == SGP_KERNEL_ARD ? d : 1; }

int make_params(int kernel, int d, const double* theta, double delta, KernParams* kp) {
  if (kernel < 0 || kernel > 2) {
    set_err("invalid covariance function (kernel=%d)", kernel);
    return SGP_EINVAL;
  }
  if (d < 1 || d > SGP_MAXD) {
    set_err("input dimension d=%d outside [1, %d]", d, SGP_MAXD);
    return SGP_EINVAL;
  }
  if (!theta) {
    set_err("theta is NULL");
    return SGP_EINVAL;
  }
  memset(kp, 0, sizeof(*kp));
  kp->kernel = kernel;
  kp->d = d;
  kp->L = num_ls(kernel, d);
  kp->P = kp->L + 2;
  kp->sigma = theta[0];
  kp->sig2 = theta[0] * theta[0];
  kp->tau = theta[kp->L + 1];
  kp->tau2 = kp->tau * kp->tau;
  kp->delta = delta;
  for (int c = 0; c < kp->L; ++c) {
    const double l = theta[1 + c];
    if (!(l > 0.0)) {
      set_err("length scale %d is not positive (%g)", c + 1, l);
      return SGP_EINVAL;
    }
    kp->l[c] = l;
    kp->rl[c] = 1.0 / l;
    kp->rl2[c] = 1.0 / (l * l);
  }
  if (kernel == SGP_KERNEL_SQEXP) kp->coef = -1.0 / (2.0 * (theta[1] * theta[1]));
  else if (kernel == SGP_KERNEL_ARD) kp->coef = -0.5;
  else kp->coef = -1.0 / theta[1];
  if (kernel != SGP_KERNEL_ARD)
    for (int c = 1; c < d; ++c) { kp->l[c] = kp->l[0]; kp->rl[c] = kp->rl[0]; kp->rl2[c] = kp->rl2[0]; }
  kp->lsig2 = log(kp->sig2);
  // The matrix-core builder clamps its exponent at lsig2 so that K <= sig2.  log's rounding is
  // |lsig2| 2^-53 relative in exp(lsig2): at sigma = 1e-150 the clamp's end came out as
  // sig2 (1 + 2.4e-14).  Step lsig2 down until exp(lsig2) <= sig2 (1 + 2^-53); for
  // |lsig2| < 2 (sigma in 0.37 .. 2.7) the rounding is within that already and nothing moves.
  const long double cap = (long double)kp->sig2 * (1.0L + 0x1p-53L);
  while (std::isfinite(kp->lsig2) && expl((long double)kp->lsig2) > cap)
    kp->lsig2 = nextafter(kp->lsig2, -INFINITY);
  set_exp_consts(kp);
  return SGP_OK;
}

}  // namespace

void set_exp_consts(KernParams* kp) {
  kp->ec[0] = 1.4426950408889634074;
  kp->ec[1] = 6.93147180369123816490e-01;
  kp->ec[2] = 1.90821492927058770002e-10;
  double f = 1.0;
  for (int q = 2; q <= 13; ++q) f *= (double)q;   // 13!
  for (int q = 13; q >= 2; --q) {                 // ec[3] = 1/13!, ..., ec[14] = 1/2!
    kp->ec[3 + (13 - q)] = 1.0 / f;
    f /= (double)q;
  }
  kp->ec[15] = 0.0;
  kp->xt[0] = 46.166241308446828384;                 // 32 / ln2
  kp->xt[1] = 6.93147180369123816490e-01 / 32.0;      // fdlibm ln2_hi (low 21 bits zero) / 32
  kp->xt[2] = 1.90821492927058770002e-10 / 32.0;      // ln2_lo / 32
  kp->xt[3] = 1.0 / 720.0;
  kp->xt[4] = 1.0 / 120.0;
  kp->xt[5] = 1.0 / 24.0;
  kp->xt[6] = 1.0 / 6.0;
  kp->xt[7] = 0.5;
  for (int j = 0; j < 32; ++j) kp->et[j] = (double)exp2l((long double)j / 32.0L);
}

namespace {

// kp->ctr = column means of the m x d knot matrix U (column-major, ld ldu; host memory), and
// kp->span2 = a bound on |x~|^2 over the knots and the data box [xlo, xhi] (per coordinate;
// NULL = knots only) that the matrix-core builder's accuracy guard reads (knm_mfma_ok).
// extra (T points, column-major, ld ldx; NULL = none): further points the same parameters will
// be built against (OAT candidate knots, which may lie outside the data box): they widen
// span2 but do not move the centre.
void set_center(KernParams* kp, const double* U, int64_t m, int64_t ldu, const double* xlo,
                const double* xhi, const double* extra = nullptr, int64_t T = 0,
                int64_t ldx = 0) {
  double span2 = 0.0;
  bool nan = false;   // the comparisons and fmax below drop a NaN: note it here
  for (int c = 0; c < kp->d; ++c) {
    double s = 0.0, lo = U[c * ldu], hi = U[c * ldu];
    for (int64_t j = 0; j < m; ++j) {
      const double v = U[j + c * ldu];
      s += v;
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    kp->ctr[c] = m > 0 ? s / (double)m : 0.0;
    if (xlo && xhi) {
      nan = nan || xlo[c] != xlo[c] || xhi[c] != xhi[c];
      lo = xlo[c] < lo ? xlo[c] : lo;
      hi = xhi[c] > hi ? xhi[c] : hi;
    }
    for (int64_t j = 0; extra && j < T; ++j) {
      const double v = extra[j + c * ldx];
      nan = nan || v != v;
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    const double e = fmax(fabs(lo - kp->ctr[c]), fabs(hi - kp->ctr[c])) * kp->rl[c];
    span2 += e * e;
  }
  // NaN coordinates: the VALU form (the matrix-core builder's clamp would turn them into 0)
  kp->span2 = (span2 == span2 && !nan) ? span2 : INFINITY;
}

// column ranges of an n x d column-major host matrix; a NaN entry makes both ends of its column
// NaN (set_center then keeps the builder off the matrix-core route)
void col_range(const double* X, int64_t n, int64_t ldx, int d, std::vector<double>* lo,
               std::vector<double>* hi) {
  lo->assign((size_t)d, 0.0);
  hi->assign((size_t)d, 0.0);
  for (int c = 0; c < d; ++c) {
    double a = n > 0 ? X[c * ldx] : 0.0, b = a;
    for (int64_t i = 1; i < n; ++i) {
      const double v = X[i + c * ldx];
      a = (v < a || v != v) ? v : a;
      b = (v > b || v != v) ? v : b;
    }
    (*lo)[(size_t)c] = a;
    (*hi)[(size_t)c] = b;
  }
}

struct Timer {
  std::string name;
  hipEvent_t a, b;
};

}  // namespace

struct sgp_ctx {
  // a row-sharded multi-device context (sgp_ctx_create_multi): the entry points below forward
  // to multi.hip, and none of the members after this one is used
  MultiCtx* multi = nullptr;
  int device = 0;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  int64_t n = 0, n_pad = 0, m_max = 0, mp_max = 0;
  int d = 0;
  // per-row data (HBM-resident for the context's lifetime)
  double* X = nullptr;      // n_pad x d, column-major, ld = n_pad
  double* r = nullptr;      // y - mu, n_pad
  double* K = nullptr;      // n_pad x mp (row-major, ld = mp)
  double* alpha = nullptr;  // n_pad
  double* zinv = nullptr;   // n_pad (FITC weights 1/Z)
  double* omega = nullptr;  // n_pad (FITC 2 W_ii)
  double* pvec = nullptr;   // n_pad (row quadratic forms)
  double* rowq = nullptr;   // (mp_max/128) x n_pad row-partial work
  double* red2f = nullptr;  // internal FITC second reduction
  // knots and m x m work
  double* U = nullptr;      // mp_max x d, column-major, ld = mp_max
  double *K22 = nullptr, *K22inv = nullptr, *Bm = nullptr, *Binv = nullptr, *Pm = nullptr;
  double *Xt = nullptr, *T1 = nullptr, *M3 = nullptr;
  double *Xt22 = nullptr, *T22 = nullptr;  // K22-stage temporaries (aux stream)
  // sync words of the two Gauss-Jordan chains that can run together: [0] main stream (Bm),
  // [SGP_GJ_SYNC_WORDS] the aux stream's K22 chain (dense_spd_inverse: zero between launches)
  unsigned* gjs = nullptr;
  double *dinv = nullptr, *dinv22 = nullptr, *logd22 = nullptr, *logdB = nullptr;
  double *uvec = nullptr, *cdiag = nullptr;
  int* status = nullptr;
  double *red1 = nullptr, *red2 = nullptr;
  double *slab_syrk = nullptr, *slab_con = nullptr, *slab_small = nullptr, *sc = nullptr;
  // the balanced gradient contraction's hand-over slots and flags (k_contract_sk)
  double* sk_ws = nullptr;
  unsigned* sk_flags = nullptr;
  unsigned sk_epoch = 0;
  int sk_slots = 0;
  double* tslab = nullptr;                // builder t = K^T r partials (VI), n_pad/64 x mp
  // stored products of the FITC / Laplace row-quadratic passes (n_pad x mp each, allocated on
  // first use): tq = K K22^-1, tp = K Bm^-1 (FITC) or K C (Laplace).  The gradient
  // contraction passes read them instead of recomputing the same 2 n m^2 GEMMs.
  double *tq = nullptr, *tp = nullptr;
  int tstore_state = 0;                   // 0 untried, 1 allocated, -1 unavailable
  int64_t slab_syrk_cap = 0, slab_con_cap = 0, slab_small_cap = 0;
  // state carried between phases
  KernParams kp;
  int64_t m = 0, mp = 0, n_global = 0;
  double delta = 0.0;
  unsigned flags = 0;
  // knot gradients (opt-in)
  bool knot_on = false;
  double *knot_slab = nullptr, *knot_part = nullptr, *knot_kmm = nullptr;
  std::vector<double> knot_raw;           // d F / d u (m x d, row-major), before the chain factor
  std::vector<double> hU;                 // host copy of the knots (m x d, column-major)
  double* pin = nullptr;                  // pinned staging for knot uploads
  hipEvent_t ev_pin = nullptr;            // the last upload's copies have been issued before it
  bool knots_valid = false;               // c->U / khash / kidx hold hU (layout knots_mp)
  int64_t knots_mp = 0;
  uint64_t* khash = nullptr;              // sorted knot coordinate hashes (k_coinc)
  int* kidx = nullptr;                    // knot index of each sorted hash
  uint8_t* cflag = nullptr;               // per data row: equals some knot (k_coinc)
  int64_t knots_gen = 0;                  // bumped whenever the resident knot set changes
  int64_t cflag_gen = -1;                 // knot set cflag was computed for
  std::vector<double> xmin, xmax;         // column ranges of this context's rows
  int phase = 0;
  int last_mode = 0;   // 1 VI, 2 FITC, 3 Laplace: the evaluation sgp_posterior_u refers to
  // K22 stage runs on `aux` concurrently with phase 1 (it depends only on U and theta)
  hipStream_t aux = nullptr;
  hipEvent_t ev_knots = nullptr, ev_k22 = nullptr;
  hipEvent_t ev_k22m = nullptr;           // K22 itself built (aux); ev_k22: K22 inverted too
  // phase 2's Bm-independent m x m work (K22inv S K22inv, tr(K22inv S)) also runs on `aux`,
  // concurrently with the latency-bound Bm inversion on the main stream
  hipEvent_t ev_s = nullptr, ev_m3 = nullptr, ev_bm = nullptr;
  hipEvent_t ev_lo = nullptr;             // VI phase 1: builder done (main) / side work done (aux_lo)
  bool vi_k22_ordered = true;             // VI phase 1 ordered main behind K22's build (ev_lo)
  // sgp_eval_vi (no reduction between the phases): at m_p = 256 t's row sums leave phase 1's
  // critical path for aux_lo in phase 2 (t is first read by the m-vectors, after the Bm chain)
  bool fused_vi = false, t_deferred = false;
  // sgp_eval_vi's phase 2: the contraction records' second pass is left to the readback kernel
  bool defer_rec = false;
  RecPass2 rec_defer{};
  int64_t t_rows_def = 0;
  hipEvent_t ev_t = nullptr;
  bool pack_red1 = false;                 // VI red1 carries S as packed lower 64-blocks
  bool borrowed_streams = false;          // own / aux / aux_lo belong to another context
  double* Sfull = nullptr;                // S unpacked from a packed red1 (mp_max^2)
  hipStream_t aux_lo = nullptr;           // ... at normal priority (the Bm chain keeps its CUs)
  double* slab_aux = nullptr;             // partials of the aux stream's small reductions
  double* rr_dev = nullptr;               // r^T r of the resident r (set with r)
  double* mmpart = nullptr;               // VI's m-vector row terms (mp), read on aux_lo;
                                          // then the folded adjoint's column terms (2 mp)
  unsigned* rsync = nullptr;              // the SYRK reduction's slice tickets (kept zeroed)
  // launch-bound Bm factorisation captured once per (mp, S pointer) and replayed
  // Poisson-Laplace state (row/knot vectors allocated on first use)
  double *y = nullptr, *mu = nullptr;     // per-row data (n_pad), kept for the Laplace path
  double* lv = nullptr;                   // LV_N x n_pad row vectors
  bool lap_gpsi_valid = false;            // LV_GPSI holds the last NR step's grad psi
  double* lm = nullptr;                   // LM_N x mp_max knot vectors
  double* lslab = nullptr;                // K^T V row-chunk partials
  double* Cprev = nullptr;                // (K22 + S_B)^-1 of the previous NR iterate
  // refined m x m solves (lap_refine): A_Z = K22 + S_Z, A_B = K22 + S_B and two m-vectors
  double *lapAZ = nullptr, *lapAB = nullptr, *laprv = nullptr;
  int64_t lslab_cap = 0;
  double* lred[2] = {nullptr, nullptr};   // ping-pong reduction buffers of sgp_eval_laplace
  int lap_state = 0, lap_it = 0, lap_maxit = 0;
  double lap_obj = 0.0, lap_obj_prev = 0.0, lap_cnt = 0.0, lap_tol = 0.0, lap_expo = 1.0;
  bool lap_expo_rows = false;             // LV_AEXP holds a per-row exposure (sgp_lap_set_expo)
  const double* lap_av = nullptr;         // this NR run's per-row exposure (nullptr: lap_expo)
  int lap_family = SGP_FAM_POISSON;       // sgp_lap_set_family
  std::vector<double> lap_objs;           // objective_function_values of the last NR run
  // full-GP Laplace (sgp_eval_full_laplace): FL_N x n_pad row vectors, allocated on first use
  double* fl = nullptr;
  bool fl_valid = false;                  // FL_W0 / FL_D10 hold a full-Laplace NR's returned state
  // EGO scan (sgp_ego_scan): the meta-model's work space (EGO_* offsets), its chain's sync and
  // status words, the three optional per-row vectors (3 x n_pad) and the sorted exclusion list;
  // allocated on first use
  double* ego = nullptr;
  unsigned* ego_sync = nullptr;
  int* ego_status = nullptr;
  double* ego_rows = nullptr;
  double* ego_ex = nullptr;
  int64_t ego_ex_cap = 0;
  int ego_blocks = 0;                     // workgroups of the scan: 8 per CU
  // sgp_fit_scan: its own m x m work space and per-row f (SCAN_* offsets) beside the EGO scan's
  // (knots, K22, its inverse, the chain's scratch, records), allocated on first use
  double* scan = nullptr;
  // timing
  bool timing = false;
  std::string timing_only;                // record only the scopes of this name ("" = all)
  int64_t timing_evals = 0;               // evaluations recorded since timing was enabled
  std::vector<Timer> timers;
  std::vector<hipEvent_t> pool;
  size_t pool_used = 0;
};

namespace {

constexpr int SC_LD22 = 0, SC_LDB = 1, SC_TU = 2, SC_TRKS = 3, SC_TRBS = 4, SC_RR = 5,
              // VI's folded adjoint (launch_vi_fold_cols): sum_j c_j, alpha^T alpha, and
              // SC_EL .. SC_EL + L - 1 = sum_j u~_jc^2 c_j
              SC_ESIG = 6, SC_ATA = 7,
              SC_G22 = 16,  // SC_G22 .. SC_G22 + P - 1 (contract_kmm records)
              SC_EL = 64;
constexpr int SC_N = 96;
static_assert(SC_G22 + SGP_MAXD + 2 <= SC_EL && SC_EL + SGP_MAXD <= SC_N, "sc slots overlap");
// per-block partials of the small reductions: k_contract_kmm writes up to 1024 blocks x (P-1)
// records (P <= SGP_MAXD + 2), the dot/colsum helpers at most 1024 x 1
constexpr int SLAB_SMALL = 1024 * (SGP_MAXD + 2);
constexpr int KNOT_PART_ROWS = 256;   // row groups of the knot / t column-sum first pass
constexpr int RB_N = 256;             // pinned readback doubles at the end of c->pin

// The end-of-evaluation results are gathered by ONE small kernel straight into pinned host
// memory (device-visible, hipHostMalloc) and unpacked into the caller's host arrays after one
// synchronisation.  (Three hipMemcpyAsync D2H copies were three blit kernels plus their launch
// gaps on the critical path of every evaluation: ~15 us at C2.)
constexpr int RB_SEGS = SGP_RB_SEGS;

#ifdef SGP_HOST_PROBE
// host time of sgp_eval_vi: entry -> the readback's synchronisation (issue) and the wait in it;
// averages printed to stderr every 200 evaluations (variant builds only)
static double hp_now() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
static double hp_t0 = 0.0, hp_issue = 0.0, hp_wait = 0.0, hp_tail = 0.0, hp_prev_end = 0.0,
              hp_gap = 0.0;
static long hp_n = 0;
#endif

struct Readback {
  sgp_ctx* c;
  double* base;
  size_t off = 0;   // doubles
  struct Item { void* host; size_t off, bytes; };
  std::vector<Item> items;
  GatherSegs segs{};
  explicit Readback(sgp_ctx* ctx)
      : c(ctx), base(ctx->pin + ctx->mp_max * ctx->d + ctx->m_max + (ctx->m_max + 1) / 2 + 8) {}
  // a readback abandoned before wait() (a failed add) drops the deferred record pass too: it
  // belongs to this readback's evaluation, and a later readback must not replay it
  ~Readback() { c->rec_defer = RecPass2{}; }
  // dev: device memory of `bytes` bytes, 8-byte aligned (copied as whole doubles)
  hipError_t add(void* host, const void* dev, size_t bytes) {
    const size_t nd = (bytes + 7) / 8;
    if (off + nd > (size_t)RB_N || segs.count == RB_SEGS) return hipErrorInvalidValue;
    items.push_back({host, off, bytes});
    segs.src[segs.count] = reinterpret_cast<const double*>(dev);
    segs.off[segs.count] = (int)off;
    segs.n[segs.count] = (int)nd;
    ++segs.count;
    off += nd;
    return hipSuccess;
  }
  hipError_t wait() {
    hipError_t e = launch_rec_gather(c->rec_defer, segs, base, c->stream);
    c->rec_defer = RecPass2{};
    if (e != hipSuccess) return e;
#ifdef SGP_HOST_PROBE
    const double t1 = hp_now();
    sgp_probe_t[1] = t1;
#endif
    e = hipStreamSynchronize(c->stream);
#ifdef SGP_HOST_PROBE
    const double t2 = hp_now();
    sgp_probe_t[2] = t2;
    if (hp_t0 > 0.0) {
      hp_issue += t1 - hp_t0;
      hp_wait += t2 - t1;
      hp_tail = t2;
    }
#endif
    if (e != hipSuccess) return e;
    for (const Item& it : items) memcpy(it.host, base + it.off, it.bytes);
    return hipSuccess;
  }
};

constexpr size_t kTimingPoolReserve = 1024;

hipEvent_t pool_event(sgp_ctx* c) {
  if (c->pool_used < c->pool.size()) return c->pool[c->pool_used++];
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  c->pool.push_back(e);
  c->pool_used++;
  return e;
}

struct Scope {
  sgp_ctx* c;
  hipStream_t s;
  size_t idx;
  Scope(sgp_ctx* ctx, const char* name, hipStream_t st = nullptr)
      : c(ctx), s(st ? st : ctx->stream), idx((size_t)-1) {
    if (!c->timing) return;
    if (!c->timing_only.empty() && c->timing_only != name) return;
    Timer t;
    t.name = name;
    t.a = pool_event(c);
    t.b = pool_event(c);
    if (!t.a || !t.b) return;
    (void)hipEventRecord(t.a, s);
    c->timers.push_back(t);
    idx = c->timers.size() - 1;
  }
  ~Scope() {
    if (idx != (size_t)-1) (void)hipEventRecord(c->timers[idx].b, s);
  }
};

// start of an evaluation: with timing on, its scopes are appended to those of the earlier
// evaluations (read out once, after the timed loop, by sgp_ctx_timings)
void timers_reset(sgp_ctx* c) {
  if (c->timing) {
    ++c->timing_evals;
    return;
  }
  c->timers.clear();
  c->pool_used = 0;
}

// a Gauss-Jordan chain whose watchdog expired (k_dense.hip: status -1; never expected)
static bool chain_watchdog(const int* status) {
  for (int q = 0; q < 3; ++q)
    if (status[q] < 0) {
      set_err("internal error: a Gauss-Jordan chain's wait watchdog expired");
      return true;
    }
  if (status[3] < 0) {
    set_err("internal error: the gradient contraction's hand-over wait watchdog expired");
    return true;
  }
  return false;
}

template <typename T>
int dalloc(T** p, int64_t count) {
  *p = nullptr;
  if (count <= 0) count = 1;
  hipError_t e = hipMalloc((void**)p, sizeof(T) * (size_t)count);
  if (e != hipSuccess) {
    set_err("hipMalloc of %lld bytes failed: %s", (long long)(sizeof(T) * count),
            hipGetErrorString(e));
    return SGP_ENOMEM;
  }
  return SGP_OK;
}

// Stored-product buffers for the FITC / Laplace passes; false (GEMM path) when HBM is short --
// the evaluation is the same either way.
bool tstore_ready(sgp_ctx* c) {
  if (c->tstore_state == 0) {
    // SGP_TSTORE=0: the recompute-everything passes, as when the memory is not there (tests)
    const char* env = getenv("SGP_TSTORE");
    if (env && env[0] == '0') {
      c->tstore_state = -1;
      return false;
    }
    const int64_t cnt = c->n_pad * c->mp_max;
    if (hipMalloc(reinterpret_cast<void**>(&c->tq), sizeof(double) * cnt) == hipSuccess &&
        hipMalloc(reinterpret_cast<void**>(&c->tp), sizeof(double) * cnt) == hipSuccess) {
      c->tstore_state = 1;
    } else {
      (void)hipGetLastError();
      if (c->tq) (void)hipFree(c->tq);
      if (c->tp) (void)hipFree(c->tp);
      c->tq = c->tp = nullptr;
      c->tstore_state = -1;
    }
  }
  return c->tstore_state == 1;
}

// FITC / Laplace: both stored products read in ONE gradient pass (ConArgs::tin2; d <= 8)
static bool fuse_tt(sgp_ctx* c) { return c->kp.d <= 8 && tstore_ready(c); }

void ctx_free(sgp_ctx* c) {
  void* ptrs[] = {c->X,      c->r,     c->K,      c->alpha,   c->zinv,  c->U,    c->K22,
                  c->K22inv, c->Bm,    c->Binv,   c->Pm,      c->Xt,    c->T1,   c->M3,
                  c->dinv,   c->logd22, c->logdB, c->uvec,    c->cdiag, c->status, c->red1,
                  c->red2,   c->slab_syrk, c->slab_con, c->slab_small, c->slab_aux, c->sc,
                  c->sk_ws,  c->sk_flags,
                  c->Xt22,   c->T22,    c->dinv22, c->omega, c->pvec, c->rowq, c->red2f,
                  c->y,      c->mu,     c->lv,     c->lm,    c->lslab, c->lred[0], c->lred[1],
                  c->Cprev,  c->lapAZ,  c->lapAB,  c->laprv,  c->fl,
                  c->knot_slab, c->knot_part, c->knot_kmm, c->tslab, c->tq, c->tp,
                  c->rr_dev, c->Sfull, c->gjs, c->mmpart, c->rsync,
                  c->ego,    c->ego_sync, c->ego_status, c->ego_rows, c->ego_ex, c->scan};
  for (void* p : ptrs)
    if (p) hipFree(p);
  if (c->khash) hipFree(c->khash);
  if (c->kidx) hipFree(c->kidx);
  if (c->cflag) hipFree(c->cflag);
  if (c->ev_knots) hipEventDestroy(c->ev_knots);
  if (c->ev_pin) hipEventDestroy(c->ev_pin);
  if (c->pin) hipHostFree(c->pin);
  if (c->ev_k22) hipEventDestroy(c->ev_k22);
  if (c->ev_k22m) hipEventDestroy(c->ev_k22m);
  if (c->ev_s) hipEventDestroy(c->ev_s);
  if (c->ev_m3) hipEventDestroy(c->ev_m3);
  if (c->ev_bm) hipEventDestroy(c->ev_bm);
  if (c->ev_lo) hipEventDestroy(c->ev_lo);
  if (c->ev_t) hipEventDestroy(c->ev_t);
  if (c->aux && !c->borrowed_streams) hipStreamDestroy(c->aux);
  if (c->aux_lo && !c->borrowed_streams) hipStreamDestroy(c->aux_lo);
  for (hipEvent_t e : c->pool) hipEventDestroy(e);
  if (c->own && !c->borrowed_streams) hipStreamDestroy(c->own);
}

// n host values -> device vector of n_pad (zero padded), synchronous
hipError_t upload_rows(double* dst, const double* src, int64_t n, int64_t n_pad) {
  std::vector<double> h((size_t)n_pad, 0.0);
  for (int64_t i = 0; i < n; ++i) h[(size_t)i] = src[i];
  return hipMemcpy(dst, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice);
}

// FNV-1a over the coordinates' bytes, +0/-0 canonicalised (k_mfma.hip coord_hash)
uint64_t coord_hash_host(const double* x, int64_t stride, int d) {
  uint64_t h = 1469598103934665603ull;
  for (int q = 0; q < d; ++q) {
    double v = x[q * stride];
    if (v == 0.0) v = 0.0;
    uint64_t b;
    memcpy(&b, &v, sizeof(b));
    for (int k = 0; k < 8; ++k) {
      h ^= (b >> (8 * k)) & 0xffu;
      h *= 1099511628211ull;
    }
  }
  return h;
}

// An evaluation that was begun but never finished (an error or an abandoned caller between
// the phases) can leave the K22 chain (aux: writes status[0], sc[SC_LD22], reads U) and aux_lo
// work queued.  Every entry that begins an evaluation (VI / FITC phase 1, Laplace begin, the
// full GP) calls this before it touches phase, U, status or sc, so the new evaluation's knot
// upload and resets on the main stream cannot overtake that work.  Only an abandoned
// evaluation (phase != 0) pays the two cross-stream waits.
int drain_abandoned(sgp_ctx* c) {
  if (c->phase != 0) {
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_k22, 0));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_m3, 0));
    c->phase = 0;
  }
  return SGP_OK;
}

int upload_knots(sgp_ctx* c, const double* U, int64_t m, int64_t ldu) {
  // optimizer iterations with fixed knots (xu_opt = "fixed") pass the same U every time: keep
  // the resident copy and its hash table
  if (c->knots_valid && c->knots_mp == c->mp && (int64_t)c->hU.size() == m * c->d) {
    bool same = true;
    for (int q = 0; q < c->d && same; ++q)
      same = memcmp(&c->hU[(size_t)(q * m)], U + q * ldu, sizeof(double) * m) == 0;
    if (same) return SGP_OK;
  }
  c->knots_valid = false;
  ++c->knots_gen;
  // staging through pinned host memory, copies async on the context stream; the previous
  // upload's copies must have drained before the buffer is rewritten
  HIPCHK(hipEventSynchronize(c->ev_pin));
  double* hU_dev = c->pin;                                        // mp x d (device layout)
  uint64_t* hh = reinterpret_cast<uint64_t*>(c->pin + c->mp_max * c->d);
  int* hi = reinterpret_cast<int*>(hh + c->m_max);
  {
    std::vector<std::pair<uint64_t, int>> hk((size_t)m);
    for (int64_t j = 0; j < m; ++j) hk[(size_t)j] = {coord_hash_host(U + j, ldu, c->d), (int)j};
    std::sort(hk.begin(), hk.end());
    for (int64_t j = 0; j < m; ++j) {
      hh[j] = hk[(size_t)j].first;
      hi[j] = hk[(size_t)j].second;
    }
  }
  c->hU.assign((size_t)(m * c->d), 0.0);
  for (int q = 0; q < c->d; ++q)
    for (int64_t j = 0; j < m; ++j) c->hU[(size_t)(j + q * m)] = U[j + q * ldu];
  for (int q = 0; q < c->d; ++q)
    for (int64_t j = 0; j < c->mp; ++j) hU_dev[q * c->mp + j] = j < m ? U[j + q * ldu] : 0.0;
  HIPCHK(hipMemcpyAsync(c->khash, hh, sizeof(uint64_t) * m, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->kidx, hi, sizeof(int) * m, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->U, hU_dev, sizeof(double) * c->mp * c->d, hipMemcpyHostToDevice,
                        c->stream));
  HIPCHK(hipEventRecord(c->ev_pin, c->stream));
  c->knots_valid = true;
  c->knots_mp = c->mp;
  return SGP_OK;
}

int check_eval_args(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
                    int64_t ldu, double delta, KernParams* kp) {
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  if (kernel == SGP_KERNEL_EXP) {
    set_err("fused evaluation supports 'sqexp' and 'ard' (optimize_gp.R:263 rejects others)");
    return SGP_EINVAL;
  }
  int st = make_params(kernel, c->d, theta, delta, kp);
  if (st) return st;
  if (!U || m < 1 || m > c->m_max || ldu < m) {
    set_err("invalid knots: m=%lld (m_max=%lld), ldu=%lld", (long long)m, (long long)c->m_max,
            (long long)ldu);
    return SGP_EINVAL;
  }
  if (!(kp->tau > 0.0) || !(kp->sigma > 0.0)) {
    set_err("sigma and tau must be positive");
    return SGP_EINVAL;
  }
  set_center(kp, U, m, ldu, c->xmin.data(), c->xmax.data());
  return SGP_OK;
}

}  // namespace

// An evaluation (or a scorer's base) is about to overwrite m, the knots and the m x m state that
// sgp_posterior_u and sgp_knot_gradient read: from here until an evaluation's finish sets
// last_mode again there is no completed evaluation to answer for, whether this one succeeds,
// fails (SGP_ENOTPD) or, as in sgp_vi_candidates, never finishes at all.
static void forget_posterior(sgp_ctx* c) {
  c->last_mode = 0;
  c->knot_raw.clear();
}

// multi.hip's hooks (sgp_multi.h)
void sgp_internal_set_err(const char* msg) { set_err("%s", msg); }

void sgp_internal_forget_eval(sgp_ctx* c) {
  forget_posterior(c);
  c->lap_gpsi_valid = false;
  c->fl_valid = false;
}

hipStream_t sgp_internal_stream(sgp_ctx* c) { return c->stream; }

// c takes over src's three streams (same device; c's own are idle after creation): the shards
// of one device then use the streams of the first, not three more hardware-queue clients each
int sgp_internal_share_streams(sgp_ctx* c, sgp_ctx* src) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->own));
  HIPCHK(hipStreamSynchronize(c->aux));
  HIPCHK(hipStreamSynchronize(c->aux_lo));
  (void)hipStreamDestroy(c->own);
  (void)hipStreamDestroy(c->aux);
  (void)hipStreamDestroy(c->aux_lo);
  c->own = src->own;
  c->stream = src->stream;
  c->aux = src->aux;
  c->aux_lo = src->aux_lo;
  c->borrowed_streams = true;
  return SGP_OK;
}

// =========================================================================== public API
extern "C" {

const char* sgp_last_error(void) { return g_err.c_str(); }
int sgp_abi_version(void) { return SGP_ABI_VERSION; }

int sgp_device_count(int* count) {
  if (!count) return SGP_EINVAL;
  HIPCHK(hipGetDeviceCount(count));
  return SGP_OK;
}

int sgp_num_params(int kernel, int d) {
  if (kernel < 0 || kernel > 2 || d < 1) return -1;
  return num_ls(kernel, d) + 2;
}

double sgp_kernel_pair(int kernel, const double* x1, const double* x2, int d,
                       const double* theta) {
  KernParams kp;
  if (make_params(kernel, d, theta, 0.0, &kp)) return NAN;
  double s = 0.0;
  if (kernel == SGP_KERNEL_SQEXP) {
    for (int c = 0; c < d; ++c) { double t = x1[c] - x2[c]; s = fma(t, t, s); }
    return kp.sig2 * exp(kp.coef * s);
  } else if (kernel == SGP_KERNEL_ARD) {
    for (int c = 0; c < d; ++c) { double t = (x1[c] - x2[c]) * kp.rl[c]; s = fma(t, t, s); }
    return kp.sig2 * exp(-s / 2.0);
  }
  for (int c = 0; c < d; ++c) s += fabs(x1[c] - x2[c]);
  return kp.sig2 * exp(kp.coef * s);
}

double sgp_dkernel_pair(int kernel, const double* x1, const double* x2, int d,
                        const double* theta, int param) {
  KernParams kp;
  if (make_params(kernel, d, theta, 0.0, &kp)) return NAN;
  if (param < 0 || param >= kp.P) { set_err("invalid parameter index %d", param); return NAN; }
  if (param == kp.P - 1) {
    bool eq = true;
    for (int c = 0; c < d; ++c) eq = eq && (x1[c] == x2[c]);
    return eq ? 2.0 * kp.tau * kp.tau : 0.0;
  }
  double s = 0.0;
  if (kernel == SGP_KERNEL_SQEXP) {
    for (int c = 0; c < d; ++c) { double t = x1[c] - x2[c]; s = fma(t, t, s); }
    const double e = exp(kp.coef * s);
    if (param == 0) return 2.0 * kp.sigma * e * kp.sigma;
    return (kp.sig2 * e) * ((1.0 / (kp.l[0] * kp.l[0] * kp.l[0])) * s) * kp.l[0];
  } else if (kernel == SGP_KERNEL_ARD) {
    for (int c = 0; c < d; ++c) { double t = (x1[c] - x2[c]) * kp.rl[c]; s = fma(t, t, s); }
    const double e = exp(-(s / 2.0));
    if (param == 0) return 2.0 * kp.sigma * e * kp.sigma;
    const int c = param - 1;
    const double dc = x1[c] - x2[c], lc = kp.l[c];
    return (kp.sig2 * e) * ((1.0 / (lc * lc * lc)) * (dc * dc)) * lc;
  }
  for (int c = 0; c < d; ++c) { double t = x1[c] - x2[c]; s = fma(t, t, s); }
  const double dist = sqrt(s);
  const double e = exp(-(1.0 / kp.l[0]) * dist);
  if (param == 0) return 2.0 * kp.sigma * e * kp.sigma;
  return (kp.sig2 * e) * ((1.0 / (kp.l[0] * kp.l[0])) * dist) * kp.l[0];
}

static int fill_common(int device, int kernel, const double* x, int64_t n, int64_t ldx,
                       const double* xp, int64_t np, int64_t ldxp, int d, const double* theta,
                       double delta, int param, bool deriv, double* out, int64_t ldo) {
  KernParams kp;
  int st = make_params(kernel, d, theta, delta, &kp);
  if (st) return st;
  const bool sym = (xp == nullptr);
  if (sym) { xp = x; np = n; ldxp = ldx; }
  if (!x || !out || n < 0 || np < 0 || ldx < n || ldxp < np || ldo < n) {
    set_err("invalid matrix arguments");
    return SGP_EINVAL;
  }
  if (deriv && (param < 0 || param >= kp.P)) {
    set_err("invalid parameter name for chosen covariance function (index %d)", param);
    return SGP_EINVAL;
  }
  if (n == 0 || np == 0) return SGP_OK;
  HIPCHK(hipSetDevice(device));
  double *dx = nullptr, *dxp = nullptr, *dout = nullptr;
  st = dalloc(&dx, n * d);
  if (!st) st = dalloc(&dxp, np * d);
  if (!st) st = dalloc(&dout, n * np);
  if (st) { hipFree(dx); hipFree(dxp); hipFree(dout); return st; }
  std::vector<double> hx((size_t)(n * d)), hxp((size_t)(np * d));
  for (int c = 0; c < d; ++c) {
    for (int64_t i = 0; i < n; ++i) hx[(size_t)(i + c * n)] = x[i + c * ldx];
    for (int64_t j = 0; j < np; ++j) hxp[(size_t)(j + c * np)] = xp[j + c * ldxp];
  }
  hipError_t e = hipMemcpy(dx, hx.data(), sizeof(double) * n * d, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dxp, hxp.data(), sizeof(double) * np * d, hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = deriv ? launch_fill_dcov(kp, dx, n, n, dxp, np, np, sym, param, dout, n, 0)
              : launch_fill_cov(kp, dx, n, n, dxp, np, np, sym, dout, n, 0);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  std::vector<double> ho;
  if (e == hipSuccess) {
    ho.resize((size_t)(n * np));
    e = hipMemcpy(ho.data(), dout, sizeof(double) * n * np, hipMemcpyDeviceToHost);
  }
  hipFree(dx);
  hipFree(dxp);
  hipFree(dout);
  if (e != hipSuccess) {
    set_err("HIP error '%s' in covariance fill", hipGetErrorString(e));
    return SGP_EHIP;
  }
  for (int64_t j = 0; j < np; ++j)
    memcpy(out + j * ldo, ho.data() + j * n, sizeof(double) * (size_t)n);
  return SGP_OK;
}

int sgp_make_cov(int device, int kernel, const double* x, int64_t n, int64_t ldx,
                 const double* xp, int64_t np, int64_t ldxp, int d, const double* theta,
                 double delta, double* out, int64_t ldo) {
  return fill_common(device, kernel, x, n, ldx, xp, np, ldxp, d, theta, delta, 0, false, out,
                     ldo);
}

int sgp_dsig_dtheta(int device, int kernel, const double* x, int64_t n, int64_t ldx,
                    const double* xp, int64_t np, int64_t ldxp, int d, const double* theta,
                    int param, double* out, int64_t ldo) {
  return fill_common(device, kernel, x, n, ldx, xp, np, ldxp, d, theta, 0.0, param, true, out,
                     ldo);
}

// The balanced (Stream-K) contraction launch, k_contract_sk: opt-in with SGP_CON_SK=1.  It is
// equivalent to the tile grid (tests/test_gpu_contract_sk.py) but measured no faster at C2 and
// slower on the n = 125 000 shard, so the product launches the grid by default and
// does not allocate the hand-over workspace.
static bool con_sk_enabled() {
  static const bool on = getenv("SGP_CON_SK") && atoi(getenv("SGP_CON_SK")) == 1;
  return on;
}
// SGP_CON_SK_DP=k: the balanced launch runs only k whole rounds as the grid (default: all but the
// last); 0 balances every tile's k-steps over the resident workgroups
static int con_sk_dp() {
  static const int dp = getenv("SGP_CON_SK_DP") ? atoi(getenv("SGP_CON_SK_DP")) : -1;
  return dp;
}

// ------------------------------------------------------------------------- context
int sgp_ctx_create(sgp_ctx** out, int device, const double* X, int64_t n, int64_t ldx, int d,
                   const double* y, const double* mu, int64_t m_max) {
  if (!out || !X || !y || !mu || n < 1 || ldx < n || d < 1 || d > SGP_MAXD || m_max < 1) {
    set_err("invalid sgp_ctx_create arguments (n=%lld, d=%d, m_max=%lld)", (long long)n, d,
            (long long)m_max);
    return SGP_EINVAL;
  }
  *out = nullptr;
  HIPCHK(hipSetDevice(device));
  sgp_ctx* c = new sgp_ctx();
  c->device = device;
  c->n = n;
  c->d = d;
  c->n_pad = round_up(n, SGP_TILE);
  c->m_max = m_max;
  c->mp_max = round_up(m_max, SGP_TILE);
  const int64_t np_ = c->n_pad, mp = c->mp_max, mm = mp * mp;
  int st = SGP_OK;
  if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
    set_err("hipStreamCreate failed");
    delete c;
    return SGP_EHIP;
  }
  c->stream = c->own;
  // aux at the highest priority: its K22 chain (a few hundred short workgroups per launch)
  // would otherwise queue behind the builder's tens of thousands
  int prio_least = 0, prio_greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess)
    prio_greatest = 0;
  if (hipStreamCreateWithPriority(&c->aux, hipStreamNonBlocking, prio_greatest) != hipSuccess ||
      hipStreamCreateWithPriority(&c->aux_lo, hipStreamNonBlocking, prio_least) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_knots, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_k22, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_k22m, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_s, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_m3, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_bm, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_lo, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_t, hipEventDisableTiming) != hipSuccess) {
    set_err("hipStream/hipEvent creation failed");
    ctx_free(c);
    delete c;
    return SGP_EHIP;
  }
  c->slab_syrk_cap = syrk_slab_doubles(np_, mp);
  c->slab_con_cap = (np_ / SGP_TILE) * (mp / SGP_TILE) * (SGP_MAXD + 5);   // nrec <= L + 5
  st = st ? st : dalloc(&c->X, np_ * d);
  st = st ? st : dalloc(&c->r, np_);
  st = st ? st : dalloc(&c->K, np_ * mp);
  st = st ? st : dalloc(&c->alpha, np_);
  st = st ? st : dalloc(&c->zinv, np_);
  st = st ? st : dalloc(&c->omega, np_);
  st = st ? st : dalloc(&c->pvec, np_);
  st = st ? st : dalloc(&c->rowq, np_ * (mp / SGP_TILE));
  st = st ? st : dalloc(&c->U, mp * d);
  st = st ? st : dalloc(&c->K22, mm);
  st = st ? st : dalloc(&c->K22inv, mm);
  st = st ? st : dalloc(&c->Bm, mm);
  st = st ? st : dalloc(&c->Binv, mm);
  st = st ? st : dalloc(&c->Pm, mm);
  st = st ? st : dalloc(&c->Xt, mm);
  st = st ? st : dalloc(&c->T1, mm);
  st = st ? st : dalloc(&c->M3, mm);
  st = st ? st : dalloc(&c->dinv, mm / SGP_DB * SGP_DB);
  st = st ? st : dalloc(&c->dinv22, mm / SGP_DB * SGP_DB);
  st = st ? st : dalloc(&c->Xt22, mm);
  st = st ? st : dalloc(&c->T22, mm);
  st = st ? st : dalloc(&c->gjs, 2 * SGP_GJ_SYNC_WORDS);
  if (!st && hipMemset(c->gjs, 0, sizeof(unsigned) * 2 * SGP_GJ_SYNC_WORDS) != hipSuccess) {
    set_err("hipMemset of the Gauss-Jordan sync words failed");
    st = SGP_EHIP;
  }
  st = st ? st : dalloc(&c->rsync, SGP_SYRK_RSYNC_WORDS);
  if (!st && hipMemset(c->rsync, 0, sizeof(unsigned) * SGP_SYRK_RSYNC_WORDS) != hipSuccess) {
    set_err("hipMemset of the SYRK reduction tickets failed");
    st = SGP_EHIP;
  }
  st = st ? st : dalloc(&c->logd22, mp / SGP_DB);
  st = st ? st : dalloc(&c->logdB, mp / SGP_DB);
  st = st ? st : dalloc(&c->uvec, mp);
  st = st ? st : dalloc(&c->cdiag, mp);
  st = st ? st : dalloc(&c->status, 4);
  st = st ? st : dalloc(&c->red1, sgp_vi_red1_count(m_max));
  // second reductions, with room for the knot partials (mp x d) after the records
  st = st ? st : dalloc(&c->red2, 64 + mp * d);
  st = st ? st : dalloc(&c->red2f, sgp_fitc_red2_count(SGP_KERNEL_ARD, SGP_MAXD, m_max) + mp * d);
  st = st ? st : dalloc(&c->slab_syrk, c->slab_syrk_cap);
  st = st ? st : dalloc(&c->slab_con, c->slab_con_cap);
  if (con_sk_enabled()) {   // resident workgroups of the balanced contraction: two per CU
    int cus = 0;
    if (!st && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) ==
                   hipSuccess && cus > 0)
      c->sk_slots = 2 * cus;
    if (c->sk_slots > 0) {
      st = st ? st : dalloc(&c->sk_ws, sgp_con_sk_doubles(c->sk_slots));
      st = st ? st : dalloc(&c->sk_flags, c->sk_slots + 1);
      if (!st && hipMemset(c->sk_flags, 0, sizeof(unsigned) * (c->sk_slots + 1)) != hipSuccess) {
        set_err("hipMemset of the contraction hand-over flags failed");
        st = SGP_EHIP;
      }
    }
  }
  // small-reduction partials: the dot/colsum helpers, and k_contract_kmm's one record per knot
  c->slab_small_cap = std::max<int64_t>(SLAB_SMALL, mp * (SGP_MAXD + 2));
  st = st ? st : dalloc(&c->slab_small, c->slab_small_cap);
  st = st ? st : dalloc(&c->slab_aux, c->slab_small_cap);
  st = st ? st : dalloc(&c->rr_dev, 1);
  st = st ? st : dalloc(&c->mmpart, 3 * mp);
  st = st ? st : dalloc(&c->sc, SC_N);
  st = st ? st : dalloc(&c->y, np_);
  st = st ? st : dalloc(&c->mu, np_);
  st = st ? st : dalloc(&c->tslab, (np_ / 64) * mp);
  st = st ? st : dalloc(&c->khash, mp);
  st = st ? st : dalloc(&c->kidx, mp);
  st = st ? st : dalloc(&c->cflag, np_);
  if (!st && (hipHostMalloc(reinterpret_cast<void**>(&c->pin),
                            sizeof(double) * (mp * d + m_max + (m_max + 1) / 2 + 8 + RB_N),
                            hipHostMallocDefault) != hipSuccess ||
              hipEventCreateWithFlags(&c->ev_pin, hipEventDisableTiming) != hipSuccess)) {
    set_err("pinned staging allocation failed");
    st = SGP_ENOMEM;
  }
  if (st) {
    ctx_free(c);
    delete c;
    return st;
  }
  col_range(X, n, ldx, d, &c->xmin, &c->xmax);
  // X: column-major with ld = n_pad, zero padded
  std::vector<double> hx((size_t)(np_ * d), 0.0);
  for (int q = 0; q < d; ++q)
    for (int64_t i = 0; i < n; ++i) hx[(size_t)(i + q * np_)] = X[i + q * ldx];
  std::vector<double> hr((size_t)np_, 0.0);
  for (int64_t i = 0; i < n; ++i) hr[(size_t)i] = y[i] - mu[i];
  hipError_t e = hipMemcpy(c->X, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(c->r, hr.data(), sizeof(double) * hr.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(c->K, 0, sizeof(double) * np_ * mp);
  if (e == hipSuccess) e = upload_rows(c->y, y, n, np_);
  if (e == hipSuccess) e = upload_rows(c->mu, mu, n, np_);
  if (e == hipSuccess) e = launch_dot(c->r, c->r, np_, c->slab_aux, c->rr_dev, c->stream);
  // the set-up's hipMemset calls (sync words, tickets, K) run on the null stream, which the
  // context's non-blocking streams do not wait for: finish them before the first evaluation
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    set_err("HIP error '%s' uploading data", hipGetErrorString(e));
    ctx_free(c);
    delete c;
    return SGP_EHIP;
  }
  *out = c;
  return SGP_OK;
}

int sgp_ctx_destroy(sgp_ctx* c) {
  if (!c) return SGP_OK;
  if (c->multi) {
    multi_destroy(c->multi);
    delete c;
    return SGP_OK;
  }
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->aux) (void)hipStreamSynchronize(c->aux);
  if (c->aux_lo) (void)hipStreamSynchronize(c->aux_lo);
  ctx_free(c);
  delete c;
  return SGP_OK;
}

// Row-sharded multi-device context: shards = contiguous row blocks as dist.shard_rows, one per
// entry of `devices` (NULL: 0 .. nshards - 1; entries may repeat), reductions inside the library
// (multi.hip: device-side sums over a device's shards, RCCL all-reduce over the devices)
int sgp_ctx_create_multi(sgp_ctx** out, const int* devices, int nshards, const double* X,
                         int64_t n, int64_t ldx, int d, const double* y, const double* mu,
                         int64_t m_max) {
  if (!out || !X || !y || !mu || n < 1 || ldx < n || d < 1 || d > SGP_MAXD || m_max < 1 ||
      nshards < 1 || nshards > SGP_MAX_SHARDS || n < nshards) {
    set_err("invalid sgp_ctx_create_multi arguments (n=%lld, d=%d, m_max=%lld, nshards=%d; "
            "1 <= nshards <= min(n, %d))", (long long)n, d, (long long)m_max, nshards,
            SGP_MAX_SHARDS);
    return SGP_EINVAL;
  }
  *out = nullptr;
  if (devices)
    for (int k = 0; k < nshards; ++k)
      if (devices[k] < 0) {
        set_err("sgp_ctx_create_multi: device %d of shard %d", devices[k], k);
        return SGP_EINVAL;
      }
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  for (int k = 0; k < nshards; ++k) {
    const int dv = devices ? devices[k] : k;
    if (dv >= ndev) {
      set_err("sgp_ctx_create_multi: shard %d on device %d, but %d device(s) are visible", k, dv,
              ndev);
      return SGP_EINVAL;
    }
  }
  MultiCtx* mc = nullptr;
  const int st = multi_create(&mc, devices, nshards, X, n, ldx, d, y, mu, m_max);
  if (st) return st;
  sgp_ctx* c = new sgp_ctx();
  c->multi = mc;
  c->n = n;
  c->d = d;
  c->m_max = m_max;
  *out = c;
  return SGP_OK;
}

int sgp_ctx_shards(const sgp_ctx* c, int* nshards, int* ndevices) {
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  if (c->multi) return multi_shards(c->multi, nshards, ndevices);
  if (nshards) *nshards = 1;
  if (ndevices) *ndevices = 1;
  return SGP_OK;
}

int sgp_ctx_set_stream(sgp_ctx* c, void* s) {
  MULTI_REFUSE(c, "sgp_ctx_set_stream");
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  c->stream = s ? (hipStream_t)s : c->own;
  return SGP_OK;
}

int sgp_ctx_set_data(sgp_ctx* c, const double* y, const double* mu) {
  MULTI_FWD(c, y && mu ? multi_set_data(c->multi, y, mu) : multi_bad_args());
  if (!c || !y || !mu) { set_err("invalid arguments"); return SGP_EINVAL; }
  if (c->lap_family == SGP_FAM_BERNOULLI && sgp_internal_check_bernoulli_y(y, c->n, 0))
    return SGP_EINVAL;   // nothing replaced
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> hr((size_t)c->n_pad, 0.0);
  for (int64_t i = 0; i < c->n; ++i) hr[(size_t)i] = y[i] - mu[i];
  HIPCHK(hipMemcpyAsync(c->r, hr.data(), sizeof(double) * hr.size(), hipMemcpyHostToDevice,
                        c->stream));
  HIPCHK(launch_dot(c->r, c->r, c->n_pad, c->slab_aux, c->rr_dev, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(upload_rows(c->y, y, c->n, c->n_pad));
  HIPCHK(upload_rows(c->mu, mu, c->n, c->n_pad));
  return SGP_OK;
}

int64_t sgp_ctx_rows(const sgp_ctx* c) { return c ? c->n : -1; }

int sgp_ctx_enable_timing(sgp_ctx* c, int enable) {
  MULTI_FWD(c, sgp_ctx_enable_timing(multi_lead(c->multi), enable));
  if (!c) return SGP_EINVAL;
  c->timing = enable != 0;
  if (c->timing) {
    c->timers.clear();
    c->pool_used = 0;
    c->timing_evals = 0;
    // events for the timed evaluations created here, not one pair per scope inside them
    // (hipEventCreate on the host between evaluations showed up at C2's 0.66 ms per step)
    while (c->pool.size() < kTimingPoolReserve) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) break;
      c->pool.push_back(e);
    }
  }
  return SGP_OK;
}

int sgp_ctx_timing_filter(sgp_ctx* c, const char* name) {
  MULTI_FWD(c, sgp_ctx_timing_filter(multi_lead(c->multi), name));
  if (!c) return SGP_EINVAL;
  c->timing_only = name ? name : "";
  return SGP_OK;
}

int64_t sgp_ctx_timing_evals(const sgp_ctx* c) {
  if (c && c->multi) return sgp_ctx_timing_evals(multi_lead(c->multi));
  return c ? c->timing_evals : -1;
}

int sgp_ctx_timings(sgp_ctx* c, char* names, int64_t names_len, double* ms, int max_n,
                    int* count) {
  MULTI_FWD(c, sgp_ctx_timings(multi_lead(c->multi), names, names_len, ms, max_n, count));
  if (!c || !count) return SGP_EINVAL;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipStreamSynchronize(c->aux));
  HIPCHK(hipStreamSynchronize(c->aux_lo));
  // per-phase totals over the recorded evaluations, in first-seen order
  std::vector<std::string> nm;
  std::vector<double> tot;
  for (const Timer& t : c->timers) {
    float v = 0.f;
    HIPCHK(hipEventElapsedTime(&v, t.a, t.b));
    size_t q = 0;
    while (q < nm.size() && nm[q] != t.name) ++q;
    if (q == nm.size()) {
      nm.push_back(t.name);
      tot.push_back(0.0);
    }
    tot[q] += v;
  }
  std::string all;
  int k = 0;
  for (size_t q = 0; q < nm.size() && k < max_n; ++q, ++k) {
    if (ms) ms[k] = tot[q];
    all += nm[q];
    all += '\n';
  }
  *count = k;
  if (names && names_len > 0) {
    strncpy(names, all.c_str(), (size_t)names_len - 1);
    names[names_len - 1] = 0;
  }
  return SGP_OK;
}

// ------------------------------------------------------------------------- VI phases
int64_t sgp_vi_red1_count(int64_t m) {
  const int64_t mp = round_up(m, SGP_TILE);
  return mp * mp + mp + 8;
}

int64_t sgp_vi_red2_count(int kernel, int d) { return num_ls(kernel, d) + 5; }

int64_t sgp_vi_red1_packed_count(int64_t m) {
  const int64_t mp = round_up(m, SGP_TILE);
  return syrk_packed_doubles(mp) + mp + 8;
}

int sgp_ctx_set_packed_reduction(sgp_ctx* c, int enable) {
  MULTI_REFUSE(c, "sgp_ctx_set_packed_reduction");
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  if (c->phase != 0) { set_err("cannot change the reduction layout inside an evaluation"); return SGP_EINVAL; }
  if (enable && !c->Sfull) {
    HIPCHK(hipSetDevice(c->device));
    int st = dalloc(&c->Sfull, c->mp_max * c->mp_max);
    if (st) return st;
  }
  c->pack_red1 = enable != 0;
  return SGP_OK;
}

// offset of t in VI's red1 (after S, full or packed); r'r follows t
static int64_t vi_red1_toff(const sgp_ctx* c, int64_t mp) {
  return c->pack_red1 ? syrk_packed_doubles(mp) : mp * mp;
}

int64_t sgp_knot_red_extra(int d, int64_t m) { return round_up(m, SGP_TILE) * d; }

// One K12 contraction pass: per-tile records summed into rec_out (L + 5 doubles) and, with
// knot gradients on, the per-knot column sums summed (or accumulated) into knot_out (mp x d).
static int contract_pass(sgp_ctx* c, const double* M, ConArgs ca, double* rec_out,
                         double* knot_out, bool knot_acc) {
  int64_t nrec = 0, nwg = 0;
  if (c->knot_on) ca.knot_slab = c->knot_slab;
  const bool fused = ca.uvec != nullptr && ca.alpha_in == nullptr && !ca.vi_fold;
  if (fused) ca.alpha_out = c->alpha;   // k_coinc needs the fused alpha_i
  // (VI's folded adjoint: the coincidence scan reads the same pair as the contraction, r / z
  // and P', launch_records)
  // the balanced launch where the tile grid leaves a mostly idle last round (opt-in, see
  // con_sk_enabled)
  if (c->sk_ws) {
    if (++c->sk_epoch == 0) ++c->sk_epoch;   // 0 is the flags' initial value
    ca.sk_ws = c->sk_ws;
    ca.sk_flags = c->sk_flags;
    ca.sk_epoch = c->sk_epoch;
    ca.sk_slots = c->sk_slots;
    ca.sk_status = c->status + 3;
    ca.sk_dp = con_sk_dp();
  }
  HIPCHK(launch_contract_args(c->kp, c->K, M, c->X, c->n_pad, c->n, c->n_pad, c->U, c->mp, c->m,
                              c->mp, ca, c->slab_con, &nrec, &nwg, c->stream));
  // the per-tile records summed, and tau's coincidence sums added to record fields 1+L .. 3+L
  // (two launches); the rows that equal some knot depend only on (X, knot set): found by
  // hashing once per knot set (cflag written), later evaluations only revisit the flagged rows
  const bool flags_known = c->cflag_gen == c->knots_gen;
  HIPCHK(launch_records(c->slab_con, nrec, nwg, c->X, c->n_pad, c->n, c->kp.d, c->U, c->mp, c->m,
                        c->khash, c->kidx, c->K, c->mp, M, ca,
                        ca.vi_fold ? ca.r : (fused ? c->alpha : ca.alpha_in),
                        c->slab_small, c->slab_small_cap, 1 + c->kp.L, rec_out, c->cflag,
                        flags_known ? 2 : 1, c->stream, c->defer_rec ? &c->rec_defer : nullptr));
  c->cflag_gen = c->knots_gen;
  if (c->knot_on)
    HIPCHK(launch_knot_reduce(c->knot_slab, c->n_pad / SGP_TILE, c->mp, c->kp.d, c->knot_part,
                              KNOT_PART_ROWS * c->mp_max * c->d,
                              knot_out, knot_acc, c->stream));
  return SGP_OK;
}

// d F / d u_kc = sum_i G_ik dK12_ik/du_kc + <G22, dK22/du_kc> (the knot branches of
// delbo_dcov_par / dlogp_dcov_par / dlogq_dcov_par, vi_functions.R:425-593): combines the
// reduced K12 part (knot_red, device) with the m x m part into c->knot_raw.
static int knot_finish(sgp_ctx* c, const double* knot_red, const double* uvec, const double* Ainv,
                       const double* Binv, const double* M3, double a, double b, double cc,
                       const double* v, const double* w, double e2) {
  if (!c->knot_on) return SGP_OK;
  const KernParams& kp = c->kp;
  const int64_t m = c->m, d = kp.d;
  HIPCHK(launch_knot_kmm(kp, c->U, c->mp, m, c->mp, uvec, Ainv, Binv, M3, a, b, cc, v, w, e2,
                         c->knot_kmm, c->stream));
  std::vector<double> h12((size_t)(m * d)), h22((size_t)(m * d));
  HIPCHK(hipMemcpyAsync(h12.data(), knot_red, sizeof(double) * m * d, hipMemcpyDeviceToHost,
                        c->stream));
  HIPCHK(hipMemcpyAsync(h22.data(), c->knot_kmm, sizeof(double) * m * d, hipMemcpyDeviceToHost,
                        c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->knot_raw.assign((size_t)(m * d), 0.0);
  const bool ard = kp.kernel == SGP_KERNEL_ARD;
  for (int64_t k = 0; k < m; ++k)
    for (int q = 0; q < d; ++q) {
      // the K12 part carries (x - u)/l_c (ARD) or (x - u) (sqexp); the m x m part raw u - u
      const double f12 = ard ? kp.rl[q] : kp.rl2[0];
      c->knot_raw[(size_t)(k * d + q)] =
          h12[(size_t)(k * d + q)] * f12 + h22[(size_t)(k * d + q)] * kp.rl2[q];
    }
  return SGP_OK;
}

int sgp_ctx_enable_knot_grad(sgp_ctx* c, int enable) {
  MULTI_FWD(c, multi_enable_knot_grad(c->multi, enable));
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  if (!enable) { c->knot_on = false; return SGP_OK; }
  HIPCHK(hipSetDevice(c->device));
  if (!c->knot_slab) {
    int st = dalloc(&c->knot_slab, (c->n_pad / SGP_TILE) * c->mp_max * c->d);
    st = st ? st : dalloc(&c->knot_part, KNOT_PART_ROWS * c->mp_max * c->d);
    st = st ? st : dalloc(&c->knot_kmm, c->mp_max * c->d);
    if (st) return st;
  }
  c->knot_on = true;
  return SGP_OK;
}

int sgp_ctx_row_bounds(sgp_ctx* c, double* lo, double* hi) {
  MULTI_FWD(c, lo && hi ? multi_row_bounds(c->multi, lo, hi) : multi_bad_args());
  if (!c || !lo || !hi) { set_err("invalid arguments"); return SGP_EINVAL; }
  for (int q = 0; q < c->d; ++q) {
    lo[q] = c->xmin[(size_t)q];
    hi[q] = c->xmax[(size_t)q];
  }
  return SGP_OK;
}

int sgp_knot_gradient(sgp_ctx* c, const double* bounds, double* grad_knot) {
  MULTI_FWD(c, grad_knot ? multi_knot_gradient(c->multi, bounds, grad_knot) : multi_bad_args());
  if (!c || !grad_knot) { set_err("invalid arguments"); return SGP_EINVAL; }
  const int64_t m = c->m, d = c->d;
  if (c->last_mode == 0) { set_err("no completed evaluation in this context"); return SGP_EINVAL; }
  if (c->knot_raw.size() != (size_t)(m * d)) {
    set_err("no knot gradient: enable it with sgp_ctx_enable_knot_grad before the evaluation");
    return SGP_EINVAL;
  }
  if (!bounds && c->last_mode != 3 && c->n_global > c->n) {
    // the default bounds are this context's row range, which differs between the ranks of a
    // row-sharded evaluation: the caller must pass the bounds of the whole data set
    set_err("row-sharded context (n_global %lld > local rows %lld): pass the global knot bounds",
            (long long)c->n_global, (long long)c->n);
    return SGP_EINVAL;
  }
  std::vector<double> lb((size_t)d), ub((size_t)d);
  for (int q = 0; q < d; ++q) {
    if (bounds) {
      lb[(size_t)q] = bounds[q];
      ub[(size_t)q] = bounds[d + q];
    } else {   // vi_functions.R:175-178: column range of xy widened by a tenth on each side
      const double diff = c->xmax[(size_t)q] - c->xmin[(size_t)q];
      lb[(size_t)q] = c->xmin[(size_t)q] - diff / 10;
      ub[(size_t)q] = c->xmax[(size_t)q] + diff / 10;
    }
  }
  // dsqexp_dx2(_ard) transform = TRUE factor dx2_dx2t (covariance_function_derivatives.R:186)
  for (int64_t k = 0; k < m; ++k)
    for (int q = 0; q < d; ++q) {
      const double u = c->hU[(size_t)(k + q * m)];
      const double chain = (ub[(size_t)q] - lb[(size_t)q]) /
                           (((u - lb[(size_t)q]) * (ub[(size_t)q] - u)) + 1e-4);
      grad_knot[k * d + q] = c->knot_raw[(size_t)(k * d + q)] * chain;
    }
  return SGP_OK;
}

static int k22_sync(sgp_ctx* c);
static int k22_launch(sgp_ctx* c, double diag_sub);
static int k22_build(sgp_ctx* c, double diag_sub);
static int k22_factor(sgp_ctx* c, bool after_main);
static int k22_stage(sgp_ctx* c, double diag_sub) {
  int st = k22_sync(c);
  return st ? st : k22_launch(c, diag_sub);
}

int sgp_vi_phase1(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
                  int64_t ldu, double delta, double* red1) {
  MULTI_REFUSE(c, "sgp_vi_phase1");
  KernParams kp;
  int st = check_eval_args(c, kernel, theta, U, m, ldu, delta, &kp);
  if (st) return st;
  if (!red1) { set_err("red1 is NULL"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(c->device));
  st = drain_abandoned(c);
  if (st) return st;
  timers_reset(c);
  forget_posterior(c);
  c->kp = kp;
  c->m = m;
  c->mp = round_up(m, SGP_TILE);
  c->delta = delta;
  st = upload_knots(c, U, m, ldu);
  if (st) return st;
  const int64_t mpv = c->mp, mmv = mpv * mpv;
  int64_t t_rows = 0;
  // mp = 256 (C2): the fragment-balanced SYRK finishes ~35 us sooner, and the side work that
  // the main stream waited for on aux_lo (t's partial sums, r^T r, red1's zeroing), starved of
  // CUs beside the SYRK, would then sit on the critical path; instead t is summed on the main
  // stream right after the SYRK (a free GPU: two short launches), r^T r is the context's
  // precomputed constant, red1 needs no zeroing (S, t, rr are all written), and phase 2 waits
  // for K22's build itself
  const bool small_syrk = syrk_use_s256(mpv, false);
  c->vi_k22_ordered = !small_syrk;
  c->t_deferred = false;
  {
    // K12, and t = K^T r riding along in the memory-bound builder (keeps the SYRK's
    // diagonal tiles as cheap as the others); the first HIP call of the evaluation, so the
    // GPU starts on it as soon as the host gets here
    Scope t(c, "build_knm");
    if (SGP_VI_BUILD_NO_T)
      HIPCHK(launch_build_knm(kp, c->X, c->n_pad, c->n, c->n_pad, c->U, mpv, m, mpv, c->K,
                              c->stream, false));
    else
      HIPCHK(launch_build_knm_t(kp, c->X, c->n_pad, c->n, c->n_pad, c->U, mpv, m, mpv, c->K,
                                c->r, c->tslab, &t_rows, c->stream, false));
  }
  // ev_knots after the builder: aux may build K22 from here on (first needed by phase 2), and
  // aux_lo may reduce the builder's t partials.  The SYRK goes right behind the builder (it
  // needs only K12); red1's reset and the small t / rr reductions run on aux_lo beside it
  // instead of between the two on the main stream, where at small n (C2) the GPU idled while
  // the host issued them one by one
  st = k22_sync(c);
  if (st) return st;
  {
    Scope t(c, "syrk");
    HIPCHK(launch_syrk_aug(c->K, c->n_pad, mpv, c->r, nullptr, c->slab_syrk, c->slab_syrk_cap,
                           red1, c->stream, 1, nullptr, 0));
  }
  // K22 itself only (aux); its inverse runs in phase 2 beside the Bm inverse -- nothing in
  // phase 1 needs it, and the latency-bound chain no longer gates the one-round SYRK or shares
  // the CUs with the builder
  // status / scalar resets on aux ahead of K22's build: the K22 chain (aux; at small n queued
  // right behind the build) is their first writer, phase 2 (main, behind ev_lo, which covers
  // ev_k22m) the next.  (On aux_lo they raced the small-n chain.)
  HIPCHK(hipMemsetAsync(c->status, 0, sizeof(int) * 4, c->aux));
  HIPCHK(hipMemsetAsync(c->sc, 0, sizeof(double) * SC_N, c->aux));
  st = k22_build(c, kp.tau2);
  if (st) return st;
  // red1 = [S (full, or its packed lower 64-blocks), t, r'r]
  const int64_t toff = vi_red1_toff(c, mpv);
  if (small_syrk && c->fused_vi) {
    c->t_deferred = true;   // summed on aux_lo in phase 2
    c->t_rows_def = t_rows;
  } else if (small_syrk) {
    HIPCHK(launch_knot_reduce(c->tslab, t_rows, mpv, 1, c->T1, c->mp_max * c->mp_max,
                              red1 + toff, false, c->stream));
  } else {
    // aux_lo, after the builder: red1's zeroing (before the SYRK reduction below writes S and
    // r^T r into it: the main stream waits for ev_lo) and t
    HIPCHK(hipStreamWaitEvent(c->aux_lo, c->ev_knots, 0));
    HIPCHK(hipMemsetAsync(red1, 0, sizeof(double) * (toff + mpv + 8), c->aux_lo));
    HIPCHK(launch_knot_reduce(c->tslab, t_rows, mpv, 1, c->T1, c->mp_max * c->mp_max,
                              red1 + toff, false, c->aux_lo));
    // ev_lo also covers K22's build (aux): the main stream, which waits for ev_lo here, needs
    // no second cross-stream wait before forming Bm = K22 + S/z in phase 2 (bm_stage)
    HIPCHK(hipStreamWaitEvent(c->aux_lo, c->ev_k22m, 0));
    HIPCHK(hipEventRecord(c->ev_lo, c->aux_lo));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_lo, 0));
  }
  {
    // S into red1, and r^T r (the context's constant; the 7 words past it zeroed)
    Scope t(c, "syrk_reduce");
    HIPCHK(launch_syrk_aug(c->K, c->n_pad, mpv, c->r, nullptr, c->slab_syrk, c->slab_syrk_cap,
                           red1, c->stream, 2, nullptr, 0, c->rr_dev, c->pack_red1, false,
                           c->rsync));
  }
  // K22's inverse (aux) is queued behind the SYRK here rather than in phase 2: it needs only
  // theta and U, so with several ranks it runs while the first all-reduce is in flight (the
  // caller issues it on the main stream between the phases); alone it starts where it did
  // Small SYRKs (C2: n m^2 = 6.6e9): the chain is queued right behind K22's build, not behind
  // the SYRK; its workgroups still find no slots until the one-round SYRK ends, and the
  // cross-stream event wait it saves was ~20 us of C2's critical path (1376 -> 1423 evals/s,
  // profiles/r3/k22_nowait_ab.txt).  At C3 and the 8-GPU shard the same change was neutral
  // overall but slowed the phase-2 chains by ~0.03 ms, so they keep the wait.
  const bool k22_after_syrk = (double)c->n_pad * (double)mpv * (double)mpv > 3e10;
  st = k22_factor(c, k22_after_syrk);
  if (st) return st;
  c->phase = 1;
  return SGP_OK;
}

static int k22_factor_launches(sgp_ctx* c, hipStream_t s) {
  const int64_t mp = c->mp;
  // K22inv holds a copy of K22 already (k22_build writes both)
  HIPCHK(dense_spd_inverse(c->K22inv, mp, c->Xt22, c->dinv22, c->logd22, c->status,
                           c->gjs + SGP_GJ_SYNC_WORDS, s));
  HIPCHK(launch_sum_and_diag(c->logd22, mp / SGP_DB, c->sc + SC_LD22, c->K22inv, mp, mp,
                             c->cdiag, s));
  return SGP_OK;
}

// K22 = Kuu + (tau^2 + delta - diag_sub) I factored and inverted on the aux stream.  It
// depends only on (U, theta), so it runs concurrently with phase 1's memory-bound builder; the
// SYRK (whose grid fills exactly one residency round) waits for it.  A pristine copy of K22
// goes to Bm for phase 2.
// The aux stream's K22 work may start once the knots (and the status/scalar resets) are on
// the main stream.  Split from the launches so that callers can enqueue the K12 builder on the
// main stream first: the chain's ~20 launches cost the host ~0.2 ms, which otherwise delayed
// the builder's start by as much.
static int k22_sync(sgp_ctx* c) {
  HIPCHK(hipEventRecord(c->ev_knots, c->stream));
  HIPCHK(hipStreamWaitEvent(c->aux, c->ev_knots, 0));
  return SGP_OK;
}

// K22 = Kuu + (tau^2 + delta - diag_sub) I on aux (ev_k22m), and its factorisation/inverse
// after it on aux (ev_k22).  VI runs the two halves in different phases.
static int k22_build(sgp_ctx* c, double diag_sub) {
  HIPCHK(launch_build_kmm(c->kp, c->U, c->mp, c->m, c->mp, diag_sub, c->K22, c->aux,
                          c->K22inv));   // and the copy the in-place inverse starts from
  HIPCHK(hipEventRecord(c->ev_k22m, c->aux));
  return SGP_OK;
}

static int k22_factor(sgp_ctx* c, bool after_main = false) {
  if (after_main) {   // not before the main stream's queued work (VI: the one-round SYRK)
    HIPCHK(hipEventRecord(c->ev_s, c->stream));
    HIPCHK(hipStreamWaitEvent(c->aux, c->ev_s, 0));
  }
  Scope t(c, "k22_aux", c->aux);
  int st = k22_factor_launches(c, c->aux);
  if (st) return st;
  HIPCHK(hipEventRecord(c->ev_k22, c->aux));
  return SGP_OK;
}

static int k22_launch(sgp_ctx* c, double diag_sub) {
  int st = k22_build(c, diag_sub);
  return st ? st : k22_factor(c, false);
}

// Binv = (K22 + S * s_scale)^-1 (one Gauss-Jordan launch per pivot; the sum is formed by the
// chain's first pivot and step as they read K22 and S)
// logdet_later: the caller sums the pivots' log-determinants itself (VI: on aux_lo, where only
// the finish waits for it, instead of one more launch between the chain and the m-vectors)
static int bm_stage(sgp_ctx* c, const double* S, double s_scale, bool k22_ordered = false,
                    bool logdet_later = false) {
  const int64_t mp = c->mp;
  Scope t(c, "dense_bm");
  if (!k22_ordered)   // Bm needs K22, not its inverse (VI: ordered through phase 1's ev_lo)
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_k22m, 0));
  HIPCHK(dense_spd_inverse_sum(c->K22, s_scale, S, c->Binv, mp, c->Xt, c->dinv, c->logdB,
                               c->status + 1, c->gjs, c->stream));
  if (!logdet_later) HIPCHK(launch_sum_small(c->logdB, mp / SGP_DB, c->sc + SC_LDB, c->stream));
  return SGP_OK;
}

int sgp_vi_phase2(sgp_ctx* c, const double* red1, int64_t n_global, unsigned flags,
                  double* red2) {
  MULTI_REFUSE(c, "sgp_vi_phase2");
  if (!c || !red1 || !red2) { set_err("invalid arguments"); return SGP_EINVAL; }
  if (c->phase != 1) { set_err("sgp_vi_phase2 called before sgp_vi_phase1"); return SGP_EINVAL; }
  if (n_global < c->n) { set_err("n_global < local rows"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(c->device));
  const KernParams& kp = c->kp;
  const int64_t mp = c->mp, mm = mp * mp;
  const double z = kp.tau2 + c->delta;
  const double* S = red1;
  const int64_t toff = vi_red1_toff(c, mp);
  const double* t = red1 + toff;
  c->n_global = n_global;
  c->flags = flags;
  if (c->pack_red1) {   // the summed packed blocks -> full S (m x m consumers below)
    HIPCHK(launch_unpack_lower64(red1, mp, c->Sfull, c->stream));
    S = c->Sfull;
  }
  // K22's inverse (queued on aux at the end of phase 1) runs concurrently with Bm's on the
  // main stream.  The Bm chain is enqueued before the side work below: the host's issue of
  // the aux_lo launches first left the GPU idle ~20 us between phase 1's last kernel and the
  // chain at C2 (kernel trace)
  HIPCHK(hipEventRecord(c->ev_s, c->stream));   // S (red1, summed) is ready
  // K22's build ordered by phase 1's ev_lo (or waited for here when phase 1 had no side work)
  const bool obj_only = (flags & SGP_FLAG_OBJ_ONLY) != 0;
  int st = bm_stage(c, S, 1.0 / z, c->vi_k22_ordered, !obj_only);
  if (st) return st;
  {
    // tr(K22inv S) and M3 = K22inv S K22inv need S and K22inv only: on aux_lo beside the Bm
    // inversion (T22 and K22inv are final once the K22 chain on `aux` has finished).  Beside
    // the K12 contraction instead, the GEMMs' workgroups starved and slowed it more.
    HIPCHK(hipStreamWaitEvent(c->aux_lo, c->ev_s, 0));
    if (c->t_deferred) {   // t = K^T r from the builder's partials (phase 1 deferred it; only
                           // sgp_eval_vi does, whose red1 is the context's own)
      HIPCHK(launch_knot_reduce(c->tslab, c->t_rows_def, mp, 1, c->T1, c->mp_max * c->mp_max,
                                c->red1 + toff, false, c->aux_lo));
    }
    HIPCHK(hipStreamWaitEvent(c->aux_lo, c->ev_k22, 0));
    // ev_t: t summed AND K22's inverse done -- the m-vectors then wait on one event, not two
    // (each cross-stream wait in front of them cost the critical path several us at C2)
    if (c->t_deferred) HIPCHK(hipEventRecord(c->ev_t, c->aux_lo));
    Scope ta(c, "m3_aux", c->aux_lo);
    HIPCHK(launch_dot(c->K22inv, S, mm, c->slab_aux, c->sc + SC_TRKS, c->aux_lo));
    if (!(flags & SGP_FLAG_OBJ_ONLY)) {
      HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, c->K22inv, mp, S, mp, 0.0,
                           c->T22, mp, c->aux_lo));
      HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, c->T22, mp, c->K22inv, mp, 0.0,
                           c->M3, mp, c->aux_lo));
    } else {
      HIPCHK(hipEventRecord(c->ev_m3, c->aux_lo));
    }
  }
  {
    Scope tm(c, "mm_vectors");
    const bool k22_via_t = c->t_deferred;   // ev_t covers K22's inverse too
    if (c->t_deferred) {
      HIPCHK(hipStreamWaitEvent(c->stream, c->ev_t, 0));
      c->t_deferred = false;
    }
    if (flags & SGP_FLAG_OBJ_ONLY) {   // elbo_fun alone: no adjoint work
      HIPCHK(dense_gemv(c->Binv, mp, t, 1.0 / z, c->uvec, c->stream));       // u = Binv t / z
      HIPCHK(launch_dot(t, c->uvec, mp, c->slab_small, c->sc + SC_TU, c->stream));
      HIPCHK(hipMemcpyAsync(c->sc + SC_RR, red1 + toff + mp, sizeof(double),
                            hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipStreamWaitEvent(c->stream, c->ev_m3, 0));
      c->phase = 2;
      return SGP_OK;
    }
    // u = Binv t / z, then P' = tau^-2 K22inv - z^-1 Binv - z^-1 u u^T and tr(Binv S)'s row
    // terms, between the Bm chain and the contraction (the critical path).  The rank-1 term
    // makes K P' = K P - (K u) u^T / z, so the contraction's adjoint G = (r/z) u^T + K P' needs
    // no K u.  Two launches: every row of P' needs all of u, and u all of Binv.  t.u,
    // tr(Binv S) and r^T r on aux_lo below (only the finish reads them)
    HIPCHK(dense_gemv(c->Binv, mp, t, 1.0 / z, c->uvec, c->stream));
    if (!k22_via_t) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_k22, 0));
    HIPCHK(launch_vi_mm_rows(c->Binv, c->K22inv, S, c->uvec, mp, 1.0 / kp.tau2, -1.0 / z,
                             -1.0 / z, c->Pm, c->mmpart, c->stream));
    HIPCHK(hipEventRecord(c->ev_bm, c->stream));
  }
  {
    // sum G22 o dK22/dtheta needs only m x m operands: on aux_lo beside the K12 contraction
    // (off the critical path; joined before the phase ends)
    HIPCHK(hipStreamWaitEvent(c->aux_lo, c->ev_bm, 0));
    HIPCHK(launch_vi_mm_scalars(t, c->uvec, c->mmpart, mp, red1 + toff + mp, c->sc + SC_TU,
                                c->sc + SC_TRBS, c->sc + SC_RR, c->aux_lo));
    HIPCHK(launch_sum_small(c->logdB, mp / SGP_DB, c->sc + SC_LDB, c->aux_lo));   // bm_stage's
    Scope tm(c, "contract_kmm", c->aux_lo);
    int nb = 0;
    HIPCHK(launch_contract_kmm(kp, c->U, c->mp, c->m, mp, c->uvec, c->K22inv, c->Binv, c->M3,
                               -0.5, 0.5, -1.0 / (2.0 * kp.tau2), nullptr, nullptr, 0.0,
                               c->slab_aux, c->slab_small_cap, &nb, c->aux_lo));
    HIPCHK(launch_colsum(c->slab_aux, nb, kp.P, c->sc + SC_G22, c->aux_lo));
  }
  int st2 = SGP_OK;
  {
    Scope tm(c, "contract_knm");
    ConArgs ca;
    ca.r = c->r;
    ca.invz = 1.0 / z;
    ca.uvec = c->uvec;
    ca.cdiag = c->cdiag;
    ca.vi_fold = true;   // G = (r/z) u^T + K P': no K u fold, no column sums, no alpha^T alpha
    st2 = contract_pass(c, c->Pm, ca, red2, red2 + sgp_vi_red2_count(kp.kernel, kp.d), false);
  }
  // the terms the folded contraction leaves out (its column sums c_j and alpha^T alpha), from
  // the reduced S, t and r^T r: with several ranks they enter once, like tr(Binv S).  On aux_lo
  // behind the G22 records, issued after the contraction so that the host reaches the
  // contraction's launch no later than before
  if (!st2)
    HIPCHK(launch_vi_fold_cols(kp, S, c->Pm, t, c->uvec, c->U, c->mp, c->m, mp, 1.0 / z,
                               red1 + toff + mp, c->mmpart + mp, !c->knot_on, c->sc + SC_ESIG,
                               c->sc + SC_EL, c->sc + SC_ATA, c->aux_lo));
  HIPCHK(hipEventRecord(c->ev_m3, c->aux_lo));
  if (st2) return st2;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_m3, 0));   // G22 records, folded terms (aux_lo)
  c->phase = 2;
  return SGP_OK;
}

int sgp_vi_finish(sgp_ctx* c, const double* red2, double* obj, double* grad) {
  MULTI_REFUSE(c, "sgp_vi_finish");
  const bool obj_only = c && (c->flags & SGP_FLAG_OBJ_ONLY);
  if (!c || !red2 || !obj || (!grad && !obj_only)) {
    set_err("invalid arguments");
    return SGP_EINVAL;
  }
  if (c->phase != 2) { set_err("sgp_vi_finish called before sgp_vi_phase2"); return SGP_EINVAL; }
  {
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) {
      // the evaluation is abandoned: no later readback may replay its deferred record pass
      c->rec_defer = RecPass2{};
      c->phase = 0;
      set_err("HIP error '%s' in hipSetDevice", hipGetErrorString(e));
      return SGP_EHIP;
    }
  }
  const KernParams& kp = c->kp;
  const int L = kp.L;
  double sc[SC_N], r2[SGP_MAXD + 8];
  int status[4];
  const int64_t n2 = sgp_vi_red2_count(kp.kernel, kp.d);
  {
    Readback rb(c);
    HIPCHK(rb.add(sc, c->sc, sizeof(sc)));
    if (!obj_only) HIPCHK(rb.add(r2, red2, sizeof(double) * n2));
    HIPCHK(rb.add(status, c->status, sizeof(status)));
    HIPCHK(rb.wait());
  }
  c->phase = 0;
  if (chain_watchdog(status)) return SGP_EHIP;
  if (status[0] || status[1]) {
    set_err("chol(): the leading minor of order %d of %s is not positive definite",
            status[0] ? status[0] : status[1],
            status[0] ? "Sigma22" : "Sigma22 + t(Sigma12) %*% ZSig12");
    return SGP_ENOTPD;
  }
  c->last_mode = 1;
  if (getenv("SGP_DEBUG_SC")) {
    fprintf(stderr, "[sgp sc] ld22 %.17g ldB %.17g tu %.17g trKS %.17g trBS %.17g rr %.17g g22",
            sc[SC_LD22], sc[SC_LDB], sc[SC_TU], sc[SC_TRKS], sc[SC_TRBS], sc[SC_RR]);
    for (int q = 0; q < kp.P; ++q) fprintf(stderr, " %.17g", sc[SC_G22 + q]);
    fprintf(stderr, "\n");
  }
  const double n = (double)c->n_global;
  const double z = kp.tau2 + c->delta;
  const double ld22 = 2.0 * sc[SC_LD22], ldB = 2.0 * sc[SC_LDB];
  const double rr = sc[SC_RR], tu = sc[SC_TU], trKS = sc[SC_TRKS], trBS = sc[SC_TRBS];
  // elbo_fun (vi_functions.R:102-118)
  const double quad = -0.5 * rr / z + 0.5 * tu / z;
  const double logdet22 = (c->flags & SGP_FLAG_R_DET) ? log(exp(ld22)) : ld22;
  const double det_part = -0.5 * (n * log(z) - logdet22 + ldB);
  const double trace_term = -(1.0 / (2.0 * kp.tau2)) * (n * (kp.sig2 + c->delta) - trKS);
  *obj = quad + det_part - (n / 2.0) * log(2.0 * M_PI) + trace_term;
  if (obj_only) {
    c->knot_raw.clear();
    return SGP_OK;
  }
  // delbo_dcov_par (vi_functions.R:259-419) in adjoint form
  // red2 = [e_sig, e_l(L), c_sum, c_cnt, c_dg, alpha^T alpha]: alpha^T alpha is zero from the
  // folded contraction and, with knots fixed, so is e_sig, and e_l lacks sum_j u~_jc^2 c_j;
  // those terms are replicated scalars (sc) of the reduced S, t and r^T r, added here once
  // (zero where the contraction formed them itself)
  const double e_sig = r2[0] + sc[SC_ESIG];
  const double c_sum = r2[1 + L], c_cnt = r2[2 + L], c_dg = r2[3 + L];
  const double aTa = r2[4 + L] + sc[SC_ATA];
  const double trSinv = n / z - trBS / (z * z);
  const double trW = 0.5 * (aTa - trSinv);
  grad[0] = 2.0 * e_sig + sc[SC_G22] - n * kp.sig2 / kp.tau2;
  for (int q = 0; q < L; ++q) grad[1 + q] = r2[1 + q] + sc[SC_EL + q] + sc[SC_G22 + 1 + q];
  grad[L + 1] = 2.0 * kp.tau2 * (c_sum - (c_cnt - c->delta * c_dg) / kp.tau2) +
                2.0 * kp.tau2 * trW - 2.0 * trace_term;
  return knot_finish(c, red2 + n2, c->uvec, c->K22inv, c->Binv, c->M3, -0.5, 0.5,
                     -1.0 / (2.0 * kp.tau2), nullptr, nullptr, 0.0);
}

int sgp_eval_vi(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
                int64_t ldu, double delta, unsigned flags, double* obj, double* grad) {
  MULTI_FWD(c, obj && (grad || (flags & SGP_FLAG_OBJ_ONLY)) ? multi_eval_vi(c->multi, kernel, theta, U, m, ldu, delta, flags, obj, grad) : multi_bad_args());
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  // sgp_vi_finish's own argument checks must not be the first to fail: phase 2 below defers the
  // records' second pass to finish's readback, and an early return there would leave it queued
  if (!obj || (!grad && !(flags & SGP_FLAG_OBJ_ONLY))) {
    set_err("obj is NULL, or grad is NULL without SGP_FLAG_OBJ_ONLY");
    return SGP_EINVAL;
  }
#ifdef SGP_HOST_PROBE
  hp_t0 = hp_now();
  sgp_probe_t[0] = hp_t0;
  if (hp_prev_end > 0.0) hp_gap += hp_t0 - hp_prev_end;
#endif
  c->fused_vi = true;   // nothing reduces red1 between the phases
  int st = sgp_vi_phase1(c, kernel, theta, U, m, ldu, delta, c->red1);
  c->fused_vi = false;
  if (st) return st;
  c->rec_defer = RecPass2{};
  c->defer_rec = true;   // the records' pass 2 runs in sgp_vi_finish's readback kernel
  st = sgp_vi_phase2(c, c->red1, c->n, flags, c->red2);
  c->defer_rec = false;
  if (st) {
    c->rec_defer = RecPass2{};
    return st;
  }
#ifdef SGP_HOST_PROBE
  const int fst = sgp_vi_finish(c, c->red2, obj, grad);
  const double t3 = hp_now();
  sgp_probe_t[3] = t3;
  hp_prev_end = t3;
  hp_tail = t3 - hp_tail;
  static double tail_sum = 0.0;
  tail_sum += hp_tail;
  if (++hp_n % 200 == 0) {
    fprintf(stderr, "[host probe] %ld evals: issue %.1f us, sync wait %.1f us, after sync %.1f us, "
            "caller gap %.1f us per eval\n", hp_n, 1e6 * hp_issue / 200, 1e6 * hp_wait / 200,
            1e6 * tail_sum / 200, 1e6 * hp_gap / 200);
    hp_issue = hp_wait = hp_gap = tail_sum = 0.0;
  }
  return fst;
#else
  return sgp_vi_finish(c, c->red2, obj, grad);
#endif
}

// ------------------------------------------------------------------------- FITC phases
// obj_fun_norm (laplace_approx_obj_funs.R:6-52) + dlogp_dcov_par (laplace_approx_gradient.R:
// 720-971) in adjoint form.  Z = sigma^2 + tau^2 + delta - q,
// q_i = K_i K22^-1 K_i^T, D = diag(Z), S_D = K^T D^-1 K, Bm = K22 + S_D, u = Bm^-1 K^T D^-1 r,
// alpha = D^-1 (r - K u), omega_i = alpha_i^2 - (Sigma^-1)_ii,
// G = alpha u^T - D^-1 K Bm^-1 - diag(omega) K K22^-1,
// G22 = -1/2 u u^T + 1/2 (K22^-1 - Bm^-1) + 1/2 K22^-1 S_omega K22^-1.
// red1 = [S_D (mp^2), t (mp), r^T D^-1 r, sum log Z]
// red2 = [S_omega (mp^2), t_omega (mp), rr_omega, sum omega, rec_1 (L+5), rec_2 (L+5)]
int64_t sgp_fitc_red1_count(int64_t m) { return sgp_vi_red1_count(m); }

int64_t sgp_fitc_red2_count(int kernel, int d, int64_t m) {
  const int64_t mp = round_up(m, SGP_TILE);
  return mp * mp + mp + 8 + 2 * (num_ls(kernel, d) + 5);
}

static int64_t fitc_rec_off(int64_t mp) { return mp * mp + mp + 8; }

int sgp_fitc_phase1(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
                    int64_t ldu, double delta, double* red1) {
  MULTI_REFUSE(c, "sgp_fitc_phase1");
  KernParams kp;
  int st = check_eval_args(c, kernel, theta, U, m, ldu, delta, &kp);
  if (st) return st;
  if (!red1) { set_err("red1 is NULL"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(c->device));
  st = drain_abandoned(c);
  if (st) return st;
  timers_reset(c);
  forget_posterior(c);
  c->kp = kp;
  c->m = m;
  c->mp = round_up(m, SGP_TILE);
  c->delta = delta;
  const int64_t mp = c->mp, mm = mp * mp;
  st = upload_knots(c, U, m, ldu);
  if (st) return st;
  HIPCHK(hipMemsetAsync(c->status, 0, sizeof(int) * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->sc, 0, sizeof(double) * SC_N, c->stream));
  st = k22_sync(c);
  if (st) return st;
  {
    Scope t(c, "build_knm");
    HIPCHK(launch_build_knm(kp, c->X, c->n_pad, c->n, c->n_pad, c->U, c->mp, m, mp, c->K,
                            c->stream, true));   // beside the K22 chain on aux
  }
  st = k22_launch(c, kp.tau2);   // K22 = Kuu + delta I, same as the VI path (laplace_gradient_ascent.R:1238-1257)
  if (st) return st;
  HIPCHK(hipMemsetAsync(red1, 0, sizeof(double) * sgp_fitc_red1_count(m), c->stream));
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_k22, 0));
  {
    Scope t(c, "rowquad_q");
    HIPCHK(launch_rowquad_knm(kp, c->K, c->K22inv, c->n, c->n_pad, m, mp, c->r, 0.0, nullptr,
                              nullptr, nullptr, c->rowq, c->pvec, c->stream,
                              tstore_ready(c) ? c->tq : nullptr));
    int nb = 0;
    HIPCHK(launch_fitc_z(c->pvec, c->n, c->n_pad, kp.sig2 + kp.tau2 + delta, c->zinv,
                         c->slab_small, &nb, c->stream));
    HIPCHK(launch_colsum(c->slab_small, nb, 1, red1 + mm + mp + 1, c->stream));
  }
  {
    Scope t(c, "syrk");
    HIPCHK(launch_syrk_aug(c->K, c->n_pad, mp, c->r, c->zinv, c->slab_syrk, c->slab_syrk_cap,
                           red1, c->stream, 3));
  }
  c->phase = 11;
  return SGP_OK;
}

int sgp_fitc_phase2(sgp_ctx* c, const double* red1, int64_t n_global, unsigned flags,
                    double* red2) {
  MULTI_REFUSE(c, "sgp_fitc_phase2");
  if (!c || !red1 || !red2) { set_err("invalid arguments"); return SGP_EINVAL; }
  if (c->phase != 11) { set_err("sgp_fitc_phase2 called before sgp_fitc_phase1"); return SGP_EINVAL; }
  if (n_global < c->n) { set_err("n_global < local rows"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(c->device));
  const KernParams& kp = c->kp;
  const int64_t mp = c->mp, mm = mp * mp;
  const double* S = red1;
  const double* t = red1 + mm;
  c->n_global = n_global;
  c->flags = flags;
  int st = bm_stage(c, S, 1.0);
  if (st) return st;
  HIPCHK(hipMemsetAsync(red2, 0, sizeof(double) * (sgp_fitc_red2_count(kp.kernel, kp.d, c->m) +
                                                    (c->knot_on ? mp * kp.d : 0)),
                        c->stream));
  {
    Scope tm(c, "mm_vectors");
    HIPCHK(dense_gemv(c->Binv, mp, t, 1.0, c->uvec, c->stream));             // u = Bm^-1 t
    HIPCHK(launch_dot(t, c->uvec, mp, c->slab_small, c->sc + SC_TU, c->stream));
    HIPCHK(hipMemcpyAsync(c->sc + SC_RR, red1 + mm + mp, 2 * sizeof(double),
                          hipMemcpyDeviceToDevice, c->stream));               // rr_w, sum log Z
  }
  if (flags & SGP_FLAG_OBJ_ONLY) {   // obj_fun_norm alone
    c->phase = 12;
    return SGP_OK;
  }
  {
    Scope tm(c, "rowquad_p");
    HIPCHK(launch_rowquad_knm(kp, c->K, c->Binv, c->n, c->n_pad, c->m, mp, c->r, 0.0, c->zinv,
                              c->uvec, c->alpha, c->rowq, c->pvec, c->stream,
                              tstore_ready(c) ? c->tp : nullptr));
    int nb = 0;
    HIPCHK(launch_fitc_omega(c->alpha, c->zinv, c->pvec, c->n, c->n_pad, c->omega,
                             c->slab_small, &nb, c->stream));
    HIPCHK(launch_colsum(c->slab_small, nb, 1, red2 + mm + mp + 1, c->stream));
  }
  {
    Scope tm(c, "syrk_omega");
    HIPCHK(launch_syrk_aug(c->K, c->n_pad, mp, c->r, c->omega, c->slab_syrk, c->slab_syrk_cap,
                           red2, c->stream, 3, nullptr, 0));
    // the SYRK reduce wrote rr_omega at mm + mp; keep sum(omega) at mm + mp + 1
  }
  const int64_t off = fitc_rec_off(mp);
  const int64_t nrec = kp.L + 5;
  double* kout = red2 + off + 2 * nrec;
  {
    Scope tm(c, "contract_knm");
    // pass 1: G1 = alpha u^T - diag(1/Z) K Bm^-1
    ConArgs a1;
    a1.r = c->r;
    a1.invz_vec = c->zinv;
    a1.uvec = c->uvec;
    a1.rs_vec = c->zinv;
    a1.rs = -1.0;
    if (tstore_ready(c)) {   // K Bm^-1 and alpha were produced by rowquad_p
      a1.tin = c->tp;
      a1.alpha_in = c->alpha;
    }
    if (fuse_tt(c)) {
      // with both products stored, pass 2's term -diag(omega) K K22^-1 joins this pass (one
      // read of K instead of two; its records stay zero -- the finish sums the two sets)
      a1.tin2 = c->tq;
      a1.M2 = c->K22inv;
      a1.rs_vec2 = c->omega;
      a1.rs2 = -1.0;
    }
    st = contract_pass(c, c->Binv, a1, red2 + off, kout, false);
    if (st) return st;
  }
  if (!fuse_tt(c)) {
    Scope tm(c, "contract_knm_b");
    // pass 2: G2 = -diag(omega) K K22^-1
    ConArgs a2;
    a2.rs_vec = c->omega;
    a2.rs = -1.0;
    if (tstore_ready(c)) a2.tin = c->tq;   // K K22^-1 from phase 1's rowquad_q
    st = contract_pass(c, c->K22inv, a2, red2 + off + nrec, kout, true);
    if (st) return st;
  }
  c->phase = 12;
  return SGP_OK;
}

int sgp_fitc_finish(sgp_ctx* c, const double* red2, double* obj, double* grad) {
  MULTI_REFUSE(c, "sgp_fitc_finish");
  const bool obj_only = c && (c->flags & SGP_FLAG_OBJ_ONLY);
  if (!c || !red2 || !obj || (!grad && !obj_only)) {
    set_err("invalid arguments");
    return SGP_EINVAL;
  }
  if (c->phase != 12) { set_err("sgp_fitc_finish called before sgp_fitc_phase2"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(c->device));
  const KernParams& kp = c->kp;
  const int L = kp.L;
  const int64_t mp = c->mp;
  if (!obj_only) {
    Scope tm(c, "contract_kmm");
    // M3 = K22^-1 S_omega K22^-1 ; G22 = -1/2 uu^T + 1/2 (K22^-1 - Bm^-1) + 1/2 M3
    HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, c->K22inv, mp, red2, mp, 0.0,
                         c->T1, mp, c->stream));
    HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, c->T1, mp, c->K22inv, mp, 0.0,
                         c->M3, mp, c->stream));
    int nb = 0;
    HIPCHK(launch_contract_kmm(kp, c->U, c->mp, c->m, mp, c->uvec, c->K22inv, c->Binv, c->M3,
                               -0.5, 0.5, 0.5, nullptr, nullptr, 0.0, c->slab_small,
                               c->slab_small_cap, &nb, c->stream));
    HIPCHK(launch_colsum(c->slab_small, nb, kp.P, c->sc + SC_G22, c->stream));
  }
  double sc[SC_N], r2[2 * (SGP_MAXD + 5) + 2];
  int status[4];
  const int64_t off = fitc_rec_off(mp);
  const int nrec = L + 5;
  {
    Readback rb(c);
    HIPCHK(rb.add(sc, c->sc, sizeof(sc)));
    if (!obj_only) {
      HIPCHK(rb.add(r2, red2 + mp * mp + mp + 1, sizeof(double)));
      HIPCHK(rb.add(r2 + 1, red2 + off, sizeof(double) * 2 * nrec));
    }
    HIPCHK(rb.add(status, c->status, sizeof(status)));
    HIPCHK(rb.wait());
  }
  c->phase = 0;
  if (chain_watchdog(status)) return SGP_EHIP;
  if (status[0] || status[1]) {
    set_err("chol(): the leading minor of order %d of %s is not positive definite",
            status[0] ? status[0] : status[1],
            status[0] ? "Sigma22" : "Sigma22 + t(Sigma12) %*% ZSig12");
    return SGP_ENOTPD;
  }
  c->last_mode = 2;
  const double n = (double)c->n_global;
  const double ld22 = 2.0 * sc[SC_LD22], ldB = 2.0 * sc[SC_LDB];
  const double rr = sc[SC_RR], sumlogz = sc[SC_RR + 1], tu = sc[SC_TU];
  const double logdet22 = (c->flags & SGP_FLAG_R_DET) ? log(exp(ld22)) : ld22;
  *obj = -0.5 * rr + 0.5 * tu - 0.5 * (sumlogz - logdet22 + ldB) - (n / 2.0) * log(2.0 * M_PI);
  if (obj_only) {
    c->knot_raw.clear();
    return SGP_OK;
  }
  const double sum_omega = r2[0];
  const double* a = r2 + 1;
  const double* b = r2 + 1 + nrec;
  grad[0] = 2.0 * (a[0] + b[0]) + sc[SC_G22] + kp.sig2 * sum_omega;
  for (int q = 0; q < L; ++q) grad[1 + q] = a[1 + q] + b[1 + q] + sc[SC_G22 + 1 + q];
  grad[L + 1] = 2.0 * kp.tau2 * (a[1 + L] + b[1 + L]) + kp.tau2 * sum_omega;
  return knot_finish(c, red2 + off + 2 * nrec, c->uvec, c->K22inv, c->Binv, c->M3, -0.5, 0.5, 0.5,
                     nullptr, nullptr, 0.0);
}

int sgp_eval_fitc(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
                  int64_t ldu, double delta, unsigned flags, double* obj, double* grad) {
  MULTI_FWD(c, obj && (grad || (flags & SGP_FLAG_OBJ_ONLY)) ? multi_eval_fitc(c->multi, kernel, theta, U, m, ldu, delta, flags, obj, grad) : multi_bad_args());
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  int st = sgp_fitc_phase1(c, kernel, theta, U, m, ldu, delta, c->red1);
  if (st) return st;
  st = sgp_fitc_phase2(c, c->red1, c->n, flags, c->red2f);
  if (st) return st;
  return sgp_fitc_finish(c, c->red2f, obj, grad);
}


// ------------------------------------------------------------------------- Poisson Laplace
// State machine over the reduction points of newtrap_sparseGP + dlogq_dcov_par (adjoint form,
// DESIGN.md sec. 3.4; numpy twin: tests/adjoint_ref.py NumpyLaplaceRank).
//   begin   : K12, K22 = Kuu + (tau^2+delta) I, Z, S_Z;  obj partials at f0
//   OBJ(0)  : C = (K22+S_B)^-1, x1 = (K22+S_Z)^-1 t_Z, objective; NR part a -> [K^T v, cnt]
//             or, once the stop rule holds, gradient part a -> [K^T c2, K^T g, K^T (B sv)]
//   NRB     : f += ...; obj partials at the new f
//   GRADB   : h, a;  [S_a, sum a, contraction records]
//   FIN     : G22 contraction, gradient
enum { LS_NONE = 0, LS_OBJ0, LS_NRB, LS_OBJ, LS_GRADB, LS_FIN };
enum { LV_F = 0, LV_Z, LV_ZI, LV_B, LV_RF, LV_TV, LV_OMZW, LV_Y1, LV_Y2, LV_DMT, LV_SV, LV_H,
       LV_A, LV_V, LV_P, LV_C2, LV_G, LV_BSV, LV_GPSI, LV_AEXP, LV_N };   // C2, G, BSV adjacent (one K^T pass)
enum { LM_X1 = 0, LM_X2, LM_S, LM_GG, LM_NGG, LM_CW, LM_N };

static double* lvec(sgp_ctx* c, int k) { return c->lv + (int64_t)k * c->n_pad; }
static double* lmv(sgp_ctx* c, int k) { return c->lm + (int64_t)k * c->mp_max; }
static int64_t lap_obj_off(int64_t mp) { return mp * mp + mp + 8; }
static int64_t lap_rec_off(int64_t mp) { return mp * mp + mp + 8; }

int64_t sgp_lap_red_count(int kernel, int d, int64_t m) {
  const int64_t mp = round_up(m, SGP_TILE);
  return 2 * (mp * mp + mp + 8) + 2 * (num_ls(kernel, d) + 5) + 8 + mp * d;   // + knot partials
}

static int lap_ensure(sgp_ctx* c) {
  if (c->lv) return SGP_OK;
  const int64_t np_ = c->n_pad, mp = c->mp_max;
  int st = dalloc(&c->lv, LV_N * np_);
  st = st ? st : dalloc(&c->lm, LM_N * mp);
  c->lslab_cap = 4 * 128 * 4096;
  if (c->lslab_cap < 4 * mp) c->lslab_cap = 4 * mp;
  st = st ? st : dalloc(&c->lslab, c->lslab_cap);
  const int64_t rc = sgp_lap_red_count(SGP_KERNEL_ARD, SGP_MAXD, c->m_max);
  st = st ? st : dalloc(&c->lred[0], rc);
  st = st ? st : dalloc(&c->lred[1], rc);
  st = st ? st : dalloc(&c->Cprev, mp * mp);
  if (st) return st;
  HIPCHK(hipMemset(c->lv, 0, sizeof(double) * LV_N * np_));
  HIPCHK(hipMemset(c->lm, 0, sizeof(double) * LM_N * mp));
  // (null-stream memsets: done before the Laplace kernels run on the context's streams)
  HIPCHK(hipDeviceSynchronize());
  return SGP_OK;
}

int sgp_lap_set_f(sgp_ctx* c, const double* f, double fill) {
  MULTI_FWD(c, multi_lap_set_f(c->multi, f, fill));
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(c->device));
  int st = lap_ensure(c);
  if (st) return st;
  std::vector<double> h((size_t)c->n_pad, 0.0);
  for (int64_t i = 0; i < c->n; ++i) h[(size_t)i] = f ? f[i] : fill;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(lvec(c, LV_F), h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  c->lap_gpsi_valid = false;
  c->fl_valid = false;
  return SGP_OK;
}

// the reference's `m` per row ("a vector of the areas of each grid cell",
// R/derivative_functions_of_data_likelihoods.R:38; optimize_gp.R:461-468 passes `a` through as m)
int sgp_lap_set_expo(sgp_ctx* c, const double* a, double fill) {
  MULTI_FWD(c, multi_lap_set_expo(c->multi, a, fill));
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  if (!a && !(fill > 0.0 && std::isfinite(fill))) {
    set_err("sgp_lap_set_expo: the fill exposure %g is not a positive finite number", fill);
    return SGP_EINVAL;
  }
  for (int64_t i = 0; a && i < c->n; ++i)
    if (!(a[i] > 0.0 && std::isfinite(a[i]))) {
      set_err("sgp_lap_set_expo: exposure a[%lld] = %g is not a positive finite number",
              (long long)i, a[i]);
      return SGP_EINVAL;
    }
  HIPCHK(hipSetDevice(c->device));
  int st = lap_ensure(c);
  if (st) return st;
  std::vector<double> h((size_t)c->n_pad, 1.0);
  for (int64_t i = 0; i < c->n; ++i) h[(size_t)i] = a ? a[i] : fill;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(lvec(c, LV_AEXP), h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  c->lap_expo_rows = true;
  return SGP_OK;
}

extern "C++" {   // sgp_multi.h hooks
// family = "bernoulli" takes responses in {0, 1} (R/optimize_gp.R:570-665)
int sgp_internal_check_bernoulli_y(const double* y, int64_t n, int64_t row0) {
  for (int64_t i = 0; i < n; ++i)
    if (!(y[i] == 0.0 || y[i] == 1.0)) {
      set_err("Bernoulli family: response y[%lld] = %g is not 0 or 1", (long long)(row0 + i),
              y[i]);
      return SGP_EINVAL;
    }
  return SGP_OK;
}

// one shard's (or a one-device context's) family; row0 = its first row in the caller's y
int sgp_internal_lap_set_family(sgp_ctx* c, int family, int64_t row0) {
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  if (family != SGP_FAM_POISSON && family != SGP_FAM_BERNOULLI) {
    set_err("sgp_lap_set_family: unknown family %d", family);
    return SGP_EINVAL;
  }
  if (family == SGP_FAM_BERNOULLI && c->lap_family != family) {
    HIPCHK(hipSetDevice(c->device));
    std::vector<double> hy((size_t)c->n);
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(hy.data(), c->y, sizeof(double) * hy.size(), hipMemcpyDeviceToHost));
    if (sgp_internal_check_bernoulli_y(hy.data(), c->n, row0)) return SGP_EINVAL;
  }
  c->lap_family = family;   // from the next evaluation on; the last one's results stay readable
  return SGP_OK;
}
}  // extern "C++"

int sgp_lap_set_family(sgp_ctx* c, int family) {
  MULTI_FWD(c, multi_lap_set_family(c->multi, family));
  return sgp_internal_lap_set_family(c, family, 0);
}

int sgp_lap_get_grad_psi(sgp_ctx* c, double* out) {
  MULTI_FWD(c, out ? multi_lap_get_grad_psi(c->multi, out) : multi_bad_args());
  if (!c || !out) { set_err("invalid arguments"); return SGP_EINVAL; }
  if (!c->lap_gpsi_valid) {
    set_err("no Newton-Raphson step has run since the mode was last set");
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, lvec(c, LV_GPSI), sizeof(double) * c->n, hipMemcpyDeviceToHost));
  return SGP_OK;
}

int sgp_lap_get_f(sgp_ctx* c, double* f) {
  MULTI_FWD(c, f ? multi_lap_get_f(c->multi, f) : multi_bad_args());
  if (!c || !f) { set_err("invalid arguments"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(c->device));
  int st = lap_ensure(c);
  if (st) return st;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(f, lvec(c, LV_F), sizeof(double) * c->n, hipMemcpyDeviceToHost));
  return SGP_OK;
}

// The m x m systems are solved through explicit Gauss-Jordan inverses, and x = inv(A) b carries
// an error of order cond(A) eps |inv(A)| |b|: with many knots per length scale (A_Z = K22 + S_Z
// at condition 1e7, |t_Z| ~ 1e4) that reaches 1e-3 in x1 and 1e-5 in the mode.  One step of
// iterative refinement, x += inv(A) (b - A x), brings it down to cond(A) eps |x|, what a
// Cholesky solve gives.  It runs for the Bernoulli family, whose NR takes hundreds of slow steps
// through such systems; the Poisson path keeps its solves, and so its results, as they were.
static bool lap_refine(const sgp_ctx* c) { return c->lap_family == SGP_FAM_BERNOULLI; }

static int lap_refine_ensure(sgp_ctx* c) {
  if (c->lapAZ) return SGP_OK;
  const int64_t mp = c->mp_max;
  int st = dalloc(&c->lapAZ, mp * mp);
  st = st ? st : dalloc(&c->lapAB, mp * mp);
  st = st ? st : dalloc(&c->laprv, 2 * mp);
  return st;
}

// x <- x + Ainv (b - A x)   (A, Ainv: mp x mp; b, x: mp)
static int lap_refine_solve(sgp_ctx* c, const double* A, const double* Ainv, const double* b,
                            double* x) {
  const int64_t mp = c->mp;
  double *r = c->laprv, *d = c->laprv + c->mp_max;
  HIPCHK(dense_gemv(A, mp, x, 1.0, d, c->stream));
  HIPCHK(dense_axpby(1.0, b, -1.0, d, r, mp, c->stream));
  HIPCHK(dense_gemv(Ainv, mp, r, 1.0, d, c->stream));
  HIPCHK(dense_axpby(1.0, x, 1.0, d, r, mp, c->stream));
  HIPCHK(hipMemcpyAsync(x, r, sizeof(double) * mp, hipMemcpyDeviceToDevice, c->stream));
  return SGP_OK;
}

// objective partials at the current f into red[o ..]: [S_B, t_Z, r'Z^-1 r, log p(y|f), log Z2]
static int lap_obj_partials(sgp_ctx* c, double* red, int64_t o) {
  const int64_t mp = c->mp, mm = mp * mp;
  Scope t(c, "lap_obj");
  int nb = 0;
  HIPCHK(launch_lap_obj(c->n, c->n_pad, lvec(c, LV_F), c->y, c->mu, lvec(c, LV_Z),
                        lvec(c, LV_ZI), c->lap_expo, c->lap_av, c->lap_family, lvec(c, LV_B),
                        lvec(c, LV_RF), lvec(c, LV_TV), c->slab_small, &nb, c->stream));
  HIPCHK(launch_syrk_aug(c->K, c->n_pad, mp, lvec(c, LV_RF), lvec(c, LV_B), c->slab_syrk,
                         c->slab_syrk_cap, red + o, c->stream, 3, lvec(c, LV_TV)));
  HIPCHK(launch_colsum(c->slab_small, nb, 2, red + o + mm + mp + 1, c->stream));
  return SGP_OK;
}

int sgp_lap_begin(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
                  int64_t ldu, double delta, double expo, double tol, int maxit, unsigned flags,
                  double* red_out, int64_t* count) {
  MULTI_REFUSE(c, "sgp_lap_begin");
  KernParams kp;
  int st = check_eval_args(c, kernel, theta, U, m, ldu, delta, &kp);
  if (st) return st;
  if (!red_out || !count) { set_err("red_out/count is NULL"); return SGP_EINVAL; }
  if (!(expo >= 0.0) || !std::isfinite(expo) || !(tol >= 0.0) || maxit < 0) {
    set_err("invalid Laplace controls (expo=%g, tol=%g, maxit=%d)", expo, tol, maxit);
    return SGP_EINVAL;
  }
  if (expo == SGP_EXPO_ROWS && !c->lap_expo_rows) {
    set_err("expo = SGP_EXPO_ROWS but no per-row exposure was set (sgp_lap_set_expo)");
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(c->device));
  st = drain_abandoned(c);
  if (st) return st;
  st = lap_ensure(c);
  if (st) return st;
  timers_reset(c);
  forget_posterior(c);
  c->kp = kp;
  c->m = m;
  c->mp = round_up(m, SGP_TILE);
  c->delta = delta;
  c->lap_expo = expo == SGP_EXPO_ROWS ? 1.0 : expo;
  c->lap_av = expo == SGP_EXPO_ROWS ? lvec(c, LV_AEXP) : nullptr;
  c->lap_tol = tol;
  c->lap_maxit = maxit;
  c->flags = flags;
  c->lap_it = 0;
  c->lap_cnt = 0.0;
  c->lap_gpsi_valid = false;   // grad psi belongs to the NR run that starts here
  c->fl_valid = false;
  c->lap_objs.clear();
  const int64_t mp = c->mp;
  st = upload_knots(c, U, m, ldu);
  if (st) return st;
  HIPCHK(hipMemsetAsync(c->status, 0, sizeof(int) * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->sc, 0, sizeof(double) * SC_N, c->stream));
  st = k22_sync(c);
  if (st) return st;
  {
    Scope t(c, "build_knm");
    HIPCHK(launch_build_knm(kp, c->X, c->n_pad, c->n, c->n_pad, c->U, c->mp, m, mp, c->K,
                            c->stream, true));   // beside the K22 chain on aux
  }
  st = k22_launch(c, 0.0);   // K22 = Kuu + (tau^2 + delta) I (newtrap_sparseGP.R:51-59)
  if (st) return st;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_k22, 0));
  {
    Scope t(c, "rowquad_q");
    HIPCHK(launch_rowquad_knm(kp, c->K, c->K22inv, c->n, c->n_pad, m, mp, c->r, 0.0, nullptr,
                              nullptr, nullptr, c->rowq, lvec(c, LV_P), c->stream,
                              tstore_ready(c) ? c->tq : nullptr));
    HIPCHK(launch_lap_z(lvec(c, LV_P), c->n, c->n_pad, kp.sig2 + kp.tau2 + delta, lvec(c, LV_Z),
                        lvec(c, LV_ZI), c->stream));
  }
  {
    Scope t(c, "syrk_z");
    HIPCHK(launch_syrk_aug(c->K, c->n_pad, mp, c->r, lvec(c, LV_ZI), c->slab_syrk,
                           c->slab_syrk_cap, red_out, c->stream, 3, nullptr, 0, nullptr, false,
                           true));   // 1/Z > 0
  }
  st = lap_obj_partials(c, red_out, lap_obj_off(mp));
  if (st) return st;
  *count = lap_obj_off(mp) + mp * mp + mp + 3;
  c->lap_state = LS_OBJ0;
  return SGP_OK;
}

// consume objective sums: factor, solve, evaluate obj_fun_pois; returns the objective
static int lap_consume_obj(sgp_ctx* c, const double* red, int64_t o, bool first, double* obj) {
  const int64_t mp = c->mp, mm = mp * mp;
  {
    Scope t(c, "lap_dense");
    if (first)   // (K22 + S_Z)^-1 is fixed for the whole NR run (Z depends on theta only)
      HIPCHK(dense_spd_inverse_sum(c->K22, 1.0, red, c->Bm, mp, c->Xt, c->dinv, c->logdB,
                                   c->status + 1, c->gjs, c->stream));
    if (!first)   // newtrap_sparseGP's u posterior uses the W of the last update's start
      HIPCHK(hipMemcpyAsync(c->Cprev, c->Binv, sizeof(double) * mm, hipMemcpyDeviceToDevice,
                            c->stream));
    HIPCHK(dense_spd_inverse_sum(c->K22, 1.0, red + o, c->Binv, mp, c->Xt, c->dinv, c->logdB,
                                 c->status + 2, c->gjs, c->stream));
    HIPCHK(launch_sum_small(c->logdB, mp / SGP_DB, c->sc + SC_LDB, c->stream));
    HIPCHK(dense_gemv(c->Bm, mp, red + o + mm, 1.0, lmv(c, LM_X1), c->stream));
    if (lap_refine(c)) {
      int st = lap_refine_ensure(c);
      if (st) return st;
      if (first) HIPCHK(dense_axpby(1.0, c->K22, 1.0, red, c->lapAZ, mm, c->stream));
      HIPCHK(dense_axpby(1.0, c->K22, 1.0, red + o, c->lapAB, mm, c->stream));
      st = lap_refine_solve(c, c->lapAZ, c->Bm, red + o + mm, lmv(c, LM_X1));
      if (st) return st;
    }
    HIPCHK(launch_dot(red + o + mm, lmv(c, LM_X1), mp, c->slab_small, c->sc + SC_TU, c->stream));
    HIPCHK(hipMemcpyAsync(c->sc + SC_RR, red + o + mm + mp, 3 * sizeof(double),
                          hipMemcpyDeviceToDevice, c->stream));
  }
  double sc[SC_N];
  int status[4];
  HIPCHK(hipMemcpyAsync(sc, c->sc, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(status, c->status, sizeof(status), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (chain_watchdog(status)) return SGP_EHIP;
  if (status[0] || status[1] || status[2]) {
    c->lap_state = LS_NONE;
    set_err("chol(): the leading minor of order %d of %s is not positive definite",
            status[0] ? status[0] : (status[1] ? status[1] : status[2]),
            status[0] ? "Sigma22" : (status[1] ? "Sigma22 + t(Sigma12) %*% ZSig12"
                                               : "Sigma22 + t(Sigma12) %*% (B * Sigma12)"));
    return SGP_ENOTPD;
  }
  if (!first) c->lap_cnt = sc[SC_RR + 3];   // the count of the step that led here (nr_b)
  const double ld22 = 2.0 * sc[SC_LD22], ldB = 2.0 * sc[SC_LDB];
  const double rr = sc[SC_RR], logpy = sc[SC_RR + 1], logz2 = sc[SC_RR + 2], tu = sc[SC_TU];
  // laplace_approx_obj_funs.R:158-172: quad + log p(y|f) + det_part_1 + det_part_2
  *obj = (-0.5 * rr + 0.5 * tu) + logpy + (-0.5 * (-ld22 + ldB)) + (-0.5 * logz2);
  return SGP_OK;
}

int sgp_lap_step(sgp_ctx* c, const double* red_in, double* red_out, int64_t* count, int* done,
                 double* obj, double* grad, int* nr_iters) {
  MULTI_REFUSE(c, "sgp_lap_step");
  if (!c || !red_in || !red_out || !count || !done || red_in == red_out) {
    set_err("invalid arguments (red_in and red_out must be distinct device buffers)");
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(c->device));
  *done = 0;
  const KernParams& kp = c->kp;
  const int64_t n = c->n, n_pad = c->n_pad, mp = c->mp, mm = mp * mp;
  const int st_in = c->lap_state;
  if (st_in == LS_OBJ0 || st_in == LS_OBJ) {
    double o = 0.0;
    int st = lap_consume_obj(c, red_in, st_in == LS_OBJ0 ? lap_obj_off(mp) : 0, st_in == LS_OBJ0,
                             &o);
    if (st) return st;
    c->lap_obj_prev = c->lap_obj;
    c->lap_obj = o;
    c->lap_it += 1;
    c->lap_objs.push_back(o);
    // maxit = 0 is this ABI's "evaluate at the given f" mode (sgp.h); any maxit >= 1 performs
    // the first update before the loop as newtrap_sparseGP.R:79-96 does (iter >= 2)
    // maxit = 0 is the C ABI's "objective and gradient at the given f" mode (dlogq_dcov_par);
    // every reference-facing caller passes maxit >= 1, so the first update always runs there,
    // as newtrap_sparseGP.R:79-96 run it before the loop whatever maxit is
    const bool go = (st_in == LS_OBJ0 && c->lap_maxit > 0) ||
                    (c->lap_it < c->lap_maxit &&
                     (fabs(c->lap_obj - c->lap_obj_prev) > c->lap_tol || c->lap_cnt > 0.0));
    if (go) {   // NR part a: grad_psi and K^T (grad_psi / omzw)
      Scope t(c, "lap_nr_a");
      if (mp <= 2048 && lap_rowpass_slab(n_pad, mp) <= c->lslab_cap) {
        // one pass over K12: y1 = K x1, the row update and K^T v from the same staged rows
        HIPCHK(launch_lap_nr_a_fused(c->K, n, n_pad, mp, lmv(c, LM_X1), lvec(c, LV_F), c->y,
                                     c->mu, lvec(c, LV_Z), lvec(c, LV_ZI), c->lap_expo,
                                     c->lap_av, c->lap_family, c->lap_tol, lvec(c, LV_Y1),
                                     lvec(c, LV_G), lvec(c, LV_OMZW),
                                     lvec(c, LV_V), lvec(c, LV_GPSI), c->lslab, c->lslab_cap,
                                     red_out, red_out + mp, c->stream));
      } else {
        HIPCHK(launch_gemv_rows(c->K, n_pad, mp, lmv(c, LM_X1), nullptr, lvec(c, LV_Y1), nullptr,
                                c->stream));
        int nb = 0;
        HIPCHK(launch_lap_nr_a(n, n_pad, lvec(c, LV_F), c->y, c->mu, lvec(c, LV_Z),
                               lvec(c, LV_ZI), c->lap_expo, c->lap_av, c->lap_family,
                               lvec(c, LV_Y1), c->lap_tol, lvec(c, LV_G), lvec(c, LV_OMZW),
                               lvec(c, LV_V), lvec(c, LV_GPSI), c->slab_small, &nb, c->stream));
        HIPCHK(launch_gemv_cols(c->K, n_pad, mp, lvec(c, LV_V), n_pad, 1, c->lslab, c->lslab_cap,
                                red_out, c->stream));
        HIPCHK(launch_colsum(c->slab_small, nb, 1, red_out + mp, c->stream));
      }
      c->lap_gpsi_valid = true;
      *count = mp + 1;
      c->lap_state = LS_NRB;
      return SGP_OK;
    }
    if (c->flags & SGP_FLAG_OBJ_ONLY) {   // newtrap_sparseGP alone: stop at the mode
      if (obj) *obj = c->lap_obj;
      if (nr_iters) *nr_iters = c->lap_it;
      c->last_mode = 3;
      c->knot_raw.clear();
      *count = 0;
      *done = 1;
      c->lap_state = LS_NONE;
      return SGP_OK;
    }
    // gradient part a (dlogq_dcov_par at the final f)
    Scope t(c, "lap_grad_a");
    // c2 = (rf - K x1) / Z rides in the row-quadratic pass's k-loop as its fused alpha (the
    // K x1 dot products from the staged K values): no separate K x1 pass
    HIPCHK(launch_rowquad_knm(kp, c->K, c->Binv, n, n_pad, c->m, mp, lvec(c, LV_RF), 0.0,
                              lvec(c, LV_ZI), lmv(c, LM_X1), lvec(c, LV_C2), c->rowq,
                              lvec(c, LV_P), c->stream, tstore_ready(c) ? c->tp : nullptr));
    HIPCHK(launch_lap_grad_a(n, n_pad, lvec(c, LV_F), c->y, c->mu, lvec(c, LV_Z), lvec(c, LV_ZI),
                             c->lap_expo, c->lap_av, c->lap_family, nullptr, lvec(c, LV_P),
                             lvec(c, LV_C2),
                             lvec(c, LV_G), lvec(c, LV_B), lvec(c, LV_DMT), lvec(c, LV_SV),
                             lvec(c, LV_BSV), c->stream));
    HIPCHK(launch_gemv_cols(c->K, n_pad, mp, lvec(c, LV_C2), n_pad, 3, c->lslab, c->lslab_cap,
                            red_out, c->stream));
    *count = 3 * mp;
    c->lap_state = LS_GRADB;
    return SGP_OK;
  }
  if (st_in == LS_NRB) {
    // NR part b and the next objective's rows fused into one K pass where the knot count allows
    const bool fused = mp <= 2048 && lap_rowpass_slab(n_pad, mp) <= c->lslab_cap;
    {
      Scope t(c, "lap_nr_b");
      // the stop-rule count rides to the host with the next objective's scalars (sc is read
      // back by lap_consume_obj): no host round trip inside the Newton step
      HIPCHK(hipMemcpyAsync(c->sc + SC_RR + 3, red_in + mp, sizeof(double),
                            hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(dense_gemv(c->Binv, mp, red_in, 1.0, lmv(c, LM_X2), c->stream));
      if (lap_refine(c)) {
        int st = lap_refine_solve(c, c->lapAB, c->Binv, red_in, lmv(c, LM_X2));
        if (st) return st;
      }
      if (!fused) {
        HIPCHK(launch_gemv_rows(c->K, n_pad, mp, lmv(c, LM_X2), nullptr, lvec(c, LV_Y2),
                                nullptr, c->stream));
        HIPCHK(launch_lap_nr_b(n, n_pad, lvec(c, LV_F), c->mu, lvec(c, LV_Z), lvec(c, LV_G),
                               lvec(c, LV_OMZW), lvec(c, LV_Y1), lvec(c, LV_Y2), c->stream));
      }
    }
    if (fused) {
      // one K pass: y2 = K x2, the f update and t = K^T tv at the new f (red_out + mm) with
      // tv'(f - mu) (red_out + mm + mp); k_lap_obj's rows (B, rf, tv, the likelihood sums) and
      // S_B by the weighted SYRK without t (red_out)
      Scope t(c, "lap_obj");
      HIPCHK(launch_lap_nr_b_t_fused(c->K, n, n_pad, mp, lmv(c, LM_X2), lvec(c, LV_F), c->y,
                                     c->mu, lvec(c, LV_Z), lvec(c, LV_ZI), lvec(c, LV_G),
                                     lvec(c, LV_OMZW), lvec(c, LV_Y1), c->lslab, c->lslab_cap,
                                     red_out + mm, red_out + mm + mp, c->stream));
      int nb = 0;
      HIPCHK(launch_lap_obj(n, n_pad, lvec(c, LV_F), c->y, c->mu, lvec(c, LV_Z), lvec(c, LV_ZI),
                            c->lap_expo, c->lap_av, c->lap_family, lvec(c, LV_B), lvec(c, LV_RF),
                            lvec(c, LV_TV), c->slab_small, &nb, c->stream));
      // B = W / (Z W - 1) >= 0 (Z > 0 and W <= 0: -a e^f, or the Bernoulli -pi (1 - pi) at
      // y = 0 and -pi - pi^2 at y = 1)
      HIPCHK(launch_syrk_aug(c->K, n_pad, mp, lvec(c, LV_RF), lvec(c, LV_B), c->slab_syrk,
                             c->slab_syrk_cap, red_out, c->stream, 3, nullptr, 0, nullptr, false,
                             true));
      HIPCHK(launch_colsum(c->slab_small, nb, 2, red_out + mm + mp + 1, c->stream));
      *count = mm + mp + 3;
      c->lap_state = LS_OBJ;
      return SGP_OK;
    }
    int st = lap_obj_partials(c, red_out, 0);
    if (st) return st;
    *count = mm + mp + 3;
    c->lap_state = LS_OBJ;
    return SGP_OK;
  }
  if (st_in == LS_GRADB) {
    Scope t(c, "lap_grad_b");
    const double* sr = red_in;
    const double* ggr = red_in + mp;
    const double* w = red_in + 2 * mp;
    HIPCHK(dense_gemv(c->K22inv, mp, sr, 1.0, lmv(c, LM_S), c->stream));
    HIPCHK(dense_gemv(c->K22inv, mp, ggr, 1.0, lmv(c, LM_GG), c->stream));
    HIPCHK(dense_gemv(c->K22inv, mp, ggr, -1.0, lmv(c, LM_NGG), c->stream));
    HIPCHK(dense_gemv(c->Binv, mp, w, 1.0, lmv(c, LM_CW), c->stream));
    if (lap_refine(c)) {
      int st = lap_refine_solve(c, c->lapAB, c->Binv, w, lmv(c, LM_CW));
      if (st) return st;
    }
    HIPCHK(launch_gemv_rows(c->K, n_pad, mp, lmv(c, LM_CW), nullptr, lvec(c, LV_Y2), nullptr,
                            c->stream));
    int nb = 0;
    HIPCHK(launch_lap_grad_b(n, n_pad, lvec(c, LV_B), lvec(c, LV_SV), lvec(c, LV_Y2),
                             lvec(c, LV_DMT), lvec(c, LV_C2), lvec(c, LV_G), lvec(c, LV_H),
                             lvec(c, LV_A), c->slab_small, &nb, c->stream));
    const int64_t off = lap_rec_off(mp);
    HIPCHK(hipMemsetAsync(red_out, 0, sizeof(double) * (off + 2 * (kp.L + 5)), c->stream));
    HIPCHK(launch_syrk_aug(c->K, n_pad, mp, c->r, lvec(c, LV_A), c->slab_syrk, c->slab_syrk_cap,
                           red_out, c->stream, 3, nullptr, 0));
    HIPCHK(launch_colsum(c->slab_small, nb, 1, red_out + mm + mp + 1, c->stream));
    int64_t nrec = kp.L + 5;
    double* kout = red_out + off + 2 * nrec;
    // G1 = c2 s^T - h GG^T - diag(B) K C
    ConArgs a1;
    a1.alpha_in = lvec(c, LV_C2);
    a1.uvec = lmv(c, LM_S);
    a1.beta_in = lvec(c, LV_H);
    a1.vvec = lmv(c, LM_NGG);
    a1.rs_vec = lvec(c, LV_B);
    a1.rs = -1.0;
    if (tstore_ready(c)) a1.tin = c->tp;   // K C from lap_grad_a's row-quadratic pass
    if (fuse_tt(c)) {
      // and G2 = -diag(2a) K K22^-1 from lap_begin's rowquad_q in the same pass (one read of
      // K; the second record set stays zero -- the finish sums the two)
      a1.tin2 = c->tq;
      a1.M2 = c->K22inv;
      a1.rs_vec2 = lvec(c, LV_A);
      a1.rs2 = -2.0;
    }
    int st = contract_pass(c, c->Binv, a1, red_out + off, kout, false);
    if (st) return st;
    if (fuse_tt(c)) {
      *count = off + 2 * nrec + (c->knot_on ? mp * kp.d : 0);
      c->lap_state = LS_FIN;
      return SGP_OK;
    }
    // G2 = -diag(2a) K K22^-1
    ConArgs a2;
    a2.rs_vec = lvec(c, LV_A);
    a2.rs = -2.0;
    if (tstore_ready(c)) a2.tin = c->tq;   // K K22^-1 from lap_begin's rowquad_q
    st = contract_pass(c, c->K22inv, a2, red_out + off + nrec, kout, true);
    if (st) return st;
    *count = off + 2 * nrec + (c->knot_on ? mp * kp.d : 0);
    c->lap_state = LS_FIN;
    return SGP_OK;
  }
  if (st_in == LS_FIN) {
    const int L = kp.L;
    {
      Scope t(c, "contract_kmm");
      // G22 = (K22^-1 - C)/2 - s s^T/2 + (Cw GG^T + GG Cw^T)/4 + K22^-1 S_a K22^-1
      HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, c->K22inv, mp, red_in, mp, 0.0,
                           c->T1, mp, c->stream));
      HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, c->T1, mp, c->K22inv, mp, 0.0,
                           c->M3, mp, c->stream));
      int nb = 0;
      HIPCHK(launch_contract_kmm(kp, c->U, c->mp, c->m, mp, lmv(c, LM_S), c->K22inv, c->Binv,
                                 c->M3, -0.5, 0.5, 1.0, lmv(c, LM_CW), lmv(c, LM_GG), 0.25,
                                 c->slab_small, c->slab_small_cap, &nb, c->stream));
      HIPCHK(launch_colsum(c->slab_small, nb, kp.P, c->sc + SC_G22, c->stream));
    }
    const int64_t off = lap_rec_off(mp);
    const int nrec = L + 5;
    double sc[SC_N], r2[2 * (SGP_MAXD + 5) + 2];
    HIPCHK(hipMemcpyAsync(sc, c->sc, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(r2, red_in + mm + mp + 1, sizeof(double), hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipMemcpyAsync(r2 + 1, red_in + off, sizeof(double) * 2 * nrec, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const double suma = r2[0];
    const double* a = r2 + 1;
    const double* b = r2 + 1 + nrec;
    const double* g22 = sc + SC_G22;
    if (grad) {
      grad[0] = 2.0 * (a[0] + b[0]) + g22[0] + 2.0 * kp.sig2 * suma;
      for (int q = 0; q < L; ++q) grad[1 + q] = a[1 + q] + b[1 + q] + g22[1 + q];
      grad[L + 1] = 2.0 * kp.tau2 * (a[1 + L] + b[1 + L]) + 2.0 * kp.tau2 * g22[kp.P - 1] +
                    2.0 * kp.tau2 * suma;
    }
    if (obj) *obj = c->lap_obj;
    if (nr_iters) *nr_iters = c->lap_it;
    c->last_mode = 3;
    int st = knot_finish(c, red_in + off + 2 * nrec, lmv(c, LM_S), c->K22inv, c->Binv, c->M3,
                         -0.5, 0.5, 1.0, lmv(c, LM_CW), lmv(c, LM_GG), 0.25);
    if (st) return st;
    *count = 0;
    *done = 1;
    c->lap_state = LS_NONE;
    return SGP_OK;
  }
  set_err("sgp_lap_step called without sgp_lap_begin");
  return SGP_EINVAL;
}

int sgp_lap_objective_values(sgp_ctx* c, double* out, int max_n, int* count) {
  MULTI_FWD(c, sgp_lap_objective_values(multi_lead(c->multi), out, max_n, count));
  if (!c || !count) { set_err("invalid arguments"); return SGP_EINVAL; }
  int k = 0;
  for (double v : c->lap_objs) {
    if (k >= max_n) break;
    if (out) out[k] = v;
    ++k;
  }
  *count = (int)c->lap_objs.size();
  return SGP_OK;
}

int sgp_eval_laplace(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
                     int64_t ldu, double delta, double expo, double tol, int maxit, double* obj,
                     double* grad, int* nr_iters) {
  MULTI_FWD(c, multi_eval_laplace(c->multi, kernel, theta, U, m, ldu, delta, expo, tol, maxit, 0u, obj, grad, nr_iters));
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(c->device));
  int st = lap_ensure(c);
  if (st) return st;
  int64_t count = 0;
  st = sgp_lap_begin(c, kernel, theta, U, m, ldu, delta, expo, tol, maxit, 0u, c->lred[0],
                     &count);
  if (st) return st;
  int cur = 0, done = 0;
  while (!done) {
    st = sgp_lap_step(c, c->lred[cur], c->lred[cur ^ 1], &count, &done, obj, grad, nr_iters);
    if (st) return st;
    cur ^= 1;
  }
  return SGP_OK;
}

int sgp_lap_nr(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
               int64_t ldu, double delta, double expo, double tol, int maxit, double* obj,
               int* nr_iters) {
  MULTI_FWD(c, multi_eval_laplace(c->multi, kernel, theta, U, m, ldu, delta, expo, tol, maxit, SGP_FLAG_OBJ_ONLY, obj, nullptr, nr_iters));
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(c->device));
  int st = lap_ensure(c);
  if (st) return st;
  int64_t count = 0;
  st = sgp_lap_begin(c, kernel, theta, U, m, ldu, delta, expo, tol, maxit, SGP_FLAG_OBJ_ONLY,
                     c->lred[0], &count);
  if (st) return st;
  int cur = 0, done = 0;
  while (!done) {
    st = sgp_lap_step(c, c->lred[cur], c->lred[cur ^ 1], &count, &done, obj, nullptr, nr_iters);
    if (st) return st;
    cur ^= 1;
  }
  return SGP_OK;
}


// ------------------------------------------------------------------------- full GP
// Config 1 (norm_grad_ascent_full, R/laplace_gradient_ascent.R:1700-2011): the n x n system
// Sigma11 = k(xy, xy) + (tau^2 + delta) I over the context's own rows, factored like K22.
//   obj  = obj_fun_norm_full = log dmvnorm(y; mu, Sigma11)  (R/laplace_approx_obj_funs.R:56-61)
//   grad = dlogp_dcov_par_full (R/laplace_approx_gradient.R:1140-1269):
//          1/2 tr((a a^T - Sigma11^-1) dSigma11/dlog theta) with a = Sigma11^-1 y -- y, not
//          y - mu (the reference's quirk) -- contracted by k_contract_kmm with
//          G = 1/2 a a^T - 1/2 Sigma11^-1; tau's derivative is 2 tau^2 on coincident pairs.
int sgp_eval_full(sgp_ctx* c, int kernel, const double* theta, double delta, unsigned flags,
                  double* obj, double* grad) {
  MULTI_REFUSE(c, "sgp_eval_full (the full GP needs every row on one device)");
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  const bool obj_only = (flags & SGP_FLAG_OBJ_ONLY) != 0;
  if (!obj || (!grad && !obj_only)) { set_err("invalid arguments"); return SGP_EINVAL; }
  if (kernel == SGP_KERNEL_EXP) {
    set_err("fused evaluation supports 'sqexp' and 'ard' (optimize_gp.R:263 rejects others)");
    return SGP_EINVAL;
  }
  if (c->n > c->m_max) {
    set_err("the full GP needs m_max >= n (n = %lld, m_max = %lld)", (long long)c->n,
            (long long)c->m_max);
    return SGP_EINVAL;
  }
  KernParams kp;
  int st = make_params(kernel, c->d, theta, delta, &kp);
  if (st) return st;
  HIPCHK(hipSetDevice(c->device));
  st = drain_abandoned(c);   // before U is overwritten below
  if (st) return st;
  timers_reset(c);
  c->kp = kp;
  c->m = c->n;
  c->mp = round_up(c->n, SGP_TILE);
  c->delta = delta;
  c->flags = flags;
  c->phase = 0;
  forget_posterior(c);
  const int64_t mp = c->mp, mm = mp * mp;
  // the rows are the "knots": X (ld n_pad) -> U (ld mp), zero padded alike (mp == n_pad)
  HIPCHK(hipMemcpy2DAsync(c->U, sizeof(double) * mp, c->X, sizeof(double) * c->n_pad,
                          sizeof(double) * mp, (size_t)c->d, hipMemcpyDeviceToDevice, c->stream));
  c->knots_valid = false;
  ++c->knots_gen;
  HIPCHK(hipMemsetAsync(c->status, 0, sizeof(int) * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->sc, 0, sizeof(double) * SC_N, c->stream));
  st = k22_stage(c, 0.0);   // Sigma11 = k(xy, xy) + (tau^2 + delta) I and its inverse
  if (st) return st;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_k22, 0));
  {
    Scope t(c, "full_vectors");
    HIPCHK(dense_gemv(c->K22inv, mp, c->y, 1.0, c->uvec, c->stream));    // a = Sigma11^-1 y
    HIPCHK(dense_gemv(c->K22inv, mp, c->r, 1.0, c->alpha, c->stream));   // Sigma11^-1 (y - mu)
    HIPCHK(launch_dot(c->r, c->alpha, mp, c->slab_small, c->sc + SC_RR, c->stream));
  }
  if (!obj_only) {
    Scope t(c, "contract_kmm");
    HIPCHK(hipMemsetAsync(c->T1, 0, sizeof(double) * mm, c->stream));
    int nb = 0;
    HIPCHK(launch_contract_kmm(kp, c->U, mp, c->m, mp, c->uvec, c->T1, c->K22inv, c->T1, 0.5,
                               0.5, 0.0, nullptr, nullptr, 0.0, c->slab_small, c->slab_small_cap, &nb,
                               c->stream));
    HIPCHK(launch_colsum(c->slab_small, nb, kp.P, c->sc + SC_G22, c->stream));
  }
  double sc[SC_N];
  int status[4];
  {
    Readback rb(c);
    HIPCHK(rb.add(sc, c->sc, sizeof(sc)));
    HIPCHK(rb.add(status, c->status, sizeof(status)));
    HIPCHK(rb.wait());
  }
  if (chain_watchdog(status)) return SGP_EHIP;
  if (status[0]) {
    set_err("Sigma11 is not positive definite (leading minor of order %d)", status[0]);
    return SGP_ENOTPD;
  }
  const double n = (double)c->n;
  *obj = -0.5 * sc[SC_RR] - sc[SC_LD22] - (n / 2.0) * log(2.0 * M_PI);   // sc: 1/2 log det
  if (!obj_only) {
    const double* g22 = sc + SC_G22;
    grad[0] = g22[0];
    for (int q = 0; q < kp.L; ++q) grad[1 + q] = g22[1 + q];
    grad[kp.L + 1] = 2.0 * kp.tau2 * g22[kp.P - 1];
  }
  return SGP_OK;
}

// ------------------------------------------------------------------------- full-GP Laplace
// family = "poisson" / "bernoulli" with sparse = FALSE (optimize_gp.R:687-732): one evaluation is
// newtrapGP (R/newtrapGP.R:6-177) from the resident f followed by dlogq_dcov_par_full
// (R/laplace_approx_gradient.R:558-711) at the mode, as one iteration of
// laplace_grad_ascent_full (R/laplace_gradient_ascent.R:742-771, 957-985).
//   Sigma = k(xy, xy) + (tau^2 + delta) I and Sigma^-1 come from the K22 stage, once per theta.
//   State at f:  B = I + sW Sigma sW (sW = sqrt(-W)), b = -W (f - mu) + d1,
//                a = b - sW o (B^-1 (sW o (Sigma b)))                      (newtrapGP.R:163-170)
//   objective:   -1/2 a^T (f - mu) + log p(y | f) - 1/2 log det B  (obj_fun_pois_full l.85-100)
//   Newton step: f <- Sigma a + mu                                         (newtrapGP.R:172)
//   grad psi:    d1 - Sigma^-1 (f - mu)  (grad_loglik_fn_pois_full l.78-83: a real solve)
// One inverse of B serves the objective at f, the step taken from f and, at the last f, the
// gradient: R = sW B^-1 sW, s2 = 1/2 (diag Sigma - diag(Sigma R Sigma)) o W3,
// v = s2 - R Sigma s2 and grad_p = sum_ij G_ij (dSigma_p)_ij with
// G = 1/2 a a^T - 1/2 R + 1/2 (v d1^T + d1 v^T) (the adjoint of l.693-706).
enum { FL_W = 0, FL_D1, FL_W0, FL_D10, FL_SW, FL_W3, FL_B, FL_RF, FL_Q, FL_GP, FL_T2, FL_A, FL_Y,
       FL_S2, FL_TMP, FL_V, FL_N };   // (W, D1) and (W0, D10) adjacent: one copy saves both
constexpr int SC_FL_LOGP = 8, SC_FL_GMAX = 9;   // launch_flap_rows' two results, adjacent

static double* flvec(sgp_ctx* c, int k) { return c->fl + (int64_t)k * c->n_pad; }

static int flap_ensure(sgp_ctx* c) {
  int st = lap_ensure(c);
  if (st || c->fl) return st;
  st = dalloc(&c->fl, FL_N * c->n_pad);
  if (st) return st;
  HIPCHK(hipMemset(c->fl, 0, sizeof(double) * FL_N * c->n_pad));
  HIPCHK(hipDeviceSynchronize());   // null-stream memset before the context's streams use it
  return SGP_OK;
}

// The state at the resident f (FL_RF current): row vectors, B^-1 in Binv, a in FL_A, and the
// objective value read back with grad psi's maximum and the chains' status.
static int flap_state(sgp_ctx* c, double* obj, double* gmax) {
  const int64_t n = c->n, mp = c->mp;
  hipStream_t s = c->stream;
  {
    Scope t(c, "flap_state");
    HIPCHK(launch_flap_gemv(c->K22inv, mp, flvec(c, FL_RF), nullptr, nullptr, flvec(c, FL_Q), s));
    HIPCHK(launch_flap_rows(n, c->n_pad, lvec(c, LV_F), c->y, c->mu, flvec(c, FL_Q), c->lap_expo,
                            c->lap_av, c->lap_family, flvec(c, FL_W), flvec(c, FL_SW),
                            flvec(c, FL_D1), flvec(c, FL_W3), flvec(c, FL_B), flvec(c, FL_GP),
                            c->slab_small, c->slab_small_cap, c->sc + SC_FL_LOGP, s));
    HIPCHK(launch_flap_scale(true, c->K22, flvec(c, FL_SW), c->Binv, mp, n, s));
  }
  {
    Scope t(c, "flap_inverse");
    HIPCHK(dense_spd_inverse(c->Binv, mp, c->Xt, c->dinv, c->logdB, c->status + 1, c->gjs, s));
    HIPCHK(launch_sum_small(c->logdB, mp / SGP_DB, c->sc + SC_LDB, s));
  }
  {
    Scope t(c, "flap_step");
    HIPCHK(launch_flap_gemv(c->K22, mp, flvec(c, FL_B), flvec(c, FL_SW), nullptr,
                            flvec(c, FL_T2), s));
    HIPCHK(launch_flap_gemv(c->Binv, mp, flvec(c, FL_T2), flvec(c, FL_SW), flvec(c, FL_B),
                            flvec(c, FL_A), s));
    HIPCHK(launch_dot(flvec(c, FL_A), flvec(c, FL_RF), mp, c->slab_small, c->sc + SC_RR, s));
  }
  double sc[SC_N];
  int status[4];
  {
    Readback rb(c);
    HIPCHK(rb.add(sc, c->sc, sizeof(sc)));
    HIPCHK(rb.add(status, c->status, sizeof(status)));
    HIPCHK(rb.wait());
  }
  if (chain_watchdog(status)) return SGP_EHIP;
  if (status[0] || status[1]) {
    set_err("chol(): the leading minor of order %d of %s is not positive definite",
            status[0] ? status[0] : status[1],
            status[0] ? "Sigma" : "I + sqrt(-W) %*% Sigma %*% sqrt(-W)");
    return SGP_ENOTPD;
  }
  // -(1/2) t(a) %*% (ff - mu) + log_py - sum(log(diag(L)))   (sc[SC_LDB] = 1/2 log det B)
  *obj = -0.5 * sc[SC_RR] + sc[SC_FL_LOGP] - sc[SC_LDB];
  *gmax = sc[SC_FL_GMAX];
  if (!std::isfinite(*obj)) {
    set_err("the full-GP Laplace objective is not finite (I + sqrt(-W) %%*%% Sigma %%*%% sqrt(-W) "
            "holds non-finite values)");
    return SGP_ENOTPD;
  }
  return SGP_OK;
}

int sgp_eval_full_laplace(sgp_ctx* c, int kernel, const double* theta, double delta, double expo,
                          double tol, int maxit, unsigned flags, double* obj, double* grad,
                          int* nr_iters) {
  MULTI_REFUSE(c, "sgp_eval_full_laplace (the full GP needs every row on one device)");
  if (!c) { set_err("context is NULL"); return SGP_EINVAL; }
  const bool obj_only = (flags & SGP_FLAG_OBJ_ONLY) != 0;
  if (!obj || (!grad && !obj_only)) { set_err("invalid arguments"); return SGP_EINVAL; }
  if (kernel == SGP_KERNEL_EXP) {
    set_err("fused evaluation supports 'sqexp' and 'ard' (optimize_gp.R:263 rejects others)");
    return SGP_EINVAL;
  }
  if (c->n > c->m_max) {
    set_err("the full GP needs m_max >= n (n = %lld, m_max = %lld)", (long long)c->n,
            (long long)c->m_max);
    return SGP_EINVAL;
  }
  if (!(expo >= 0.0) || !std::isfinite(expo) || !(tol >= 0.0) || maxit < 0) {
    set_err("invalid Laplace controls (expo=%g, tol=%g, maxit=%d)", expo, tol, maxit);
    return SGP_EINVAL;
  }
  if (expo == SGP_EXPO_ROWS && !c->lap_expo_rows) {
    set_err("expo = SGP_EXPO_ROWS but no per-row exposure was set (sgp_lap_set_expo)");
    return SGP_EINVAL;
  }
  KernParams kp;
  int st = make_params(kernel, c->d, theta, delta, &kp);
  if (st) return st;
  if (!(kp.tau > 0.0) || !(kp.sigma > 0.0)) {
    set_err("sigma and tau must be positive");
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(c->device));
  st = drain_abandoned(c);   // before U is overwritten below
  if (st) return st;
  st = flap_ensure(c);
  if (st) return st;
  timers_reset(c);
  c->kp = kp;
  c->m = c->n;
  c->mp = round_up(c->n, SGP_TILE);
  c->delta = delta;
  c->flags = flags;
  c->phase = 0;
  forget_posterior(c);
  c->lap_state = LS_NONE;
  c->lap_expo = expo == SGP_EXPO_ROWS ? 1.0 : expo;
  c->lap_av = expo == SGP_EXPO_ROWS ? lvec(c, LV_AEXP) : nullptr;
  c->lap_tol = tol;
  c->lap_maxit = maxit;
  c->lap_it = 0;
  c->lap_gpsi_valid = false;
  c->fl_valid = false;
  c->lap_objs.clear();
  const int64_t n = c->n, n_pad = c->n_pad, mp = c->mp;
  hipStream_t s = c->stream;
  // the rows are the "knots": X (ld n_pad) -> U (ld mp), zero padded alike (mp == n_pad)
  HIPCHK(hipMemcpy2DAsync(c->U, sizeof(double) * mp, c->X, sizeof(double) * n_pad,
                          sizeof(double) * mp, (size_t)c->d, hipMemcpyDeviceToDevice, s));
  c->knots_valid = false;
  ++c->knots_gen;
  HIPCHK(hipMemsetAsync(c->status, 0, sizeof(int) * 4, s));
  HIPCHK(hipMemsetAsync(c->sc, 0, sizeof(double) * SC_N, s));
  st = k22_stage(c, 0.0);   // Sigma (K22) and Sigma^-1 (K22inv): newtrapGP.R:43-56
  if (st) return st;
  HIPCHK(launch_flap_update(n, n_pad, nullptr, c->mu, lvec(c, LV_F), flvec(c, FL_RF), s));
  HIPCHK(hipStreamWaitEvent(s, c->ev_k22, 0));
  double o = 0.0, gmax = 0.0;
  st = flap_state(c, &o, &gmax);   // obj_fun_vals[1] (newtrapGP.R:60)
  if (st) return st;
  c->lap_objs.push_back(o);
  c->lap_it = 1;
  // maxit = 0: objective and gradient at the resident f as given (the sparse path's convention);
  // any maxit >= 1 runs the first update unconditionally, as newtrapGP.R:63-75 does
  bool go = maxit > 0;
  while (go) {
    {
      Scope t(c, "flap_step");
      // newtrapGP returns W, grad_log_py_ff and grad_psi of the iterate this update starts from
      HIPCHK(hipMemcpyAsync(flvec(c, FL_W0), flvec(c, FL_W), sizeof(double) * 2 * n_pad,
                            hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(lvec(c, LV_GPSI), flvec(c, FL_GP), sizeof(double) * n_pad,
                            hipMemcpyDeviceToDevice, s));
      HIPCHK(launch_flap_gemv(c->K22, mp, flvec(c, FL_A), nullptr, nullptr, flvec(c, FL_Y), s));
      HIPCHK(launch_flap_update(n, n_pad, flvec(c, FL_Y), c->mu, lvec(c, LV_F),
                                flvec(c, FL_RF), s));
    }
    c->lap_gpsi_valid = true;
    c->fl_valid = true;
    const double o_prev = o, g_start = gmax;
    st = flap_state(c, &o, &gmax);
    if (st) return st;
    c->lap_objs.push_back(o);
    c->lap_it += 1;
    go = c->lap_it < maxit && (fabs(o - o_prev) > tol || g_start > tol);   // newtrapGP.R:77
  }
  c->lap_obj = o;
  *obj = o;
  if (nr_iters) *nr_iters = c->lap_it;
  if (obj_only) return SGP_OK;
  {
    Scope t(c, "flap_grad");
    HIPCHK(launch_flap_scale(false, c->Binv, flvec(c, FL_SW), c->Binv, mp, n, s));   // R
    HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, c->K22, mp, c->Binv, mp, 0.0,
                         c->T1, mp, s));                                              // Sigma R
    HIPCHK(launch_flap_rowdot(c->K22, c->T1, mp, n, flvec(c, FL_W3), flvec(c, FL_S2), s));
    HIPCHK(launch_flap_gemv(c->K22, mp, flvec(c, FL_S2), nullptr, nullptr, flvec(c, FL_TMP), s));
    HIPCHK(launch_flap_gemv(c->Binv, mp, flvec(c, FL_TMP), nullptr, flvec(c, FL_S2),
                            flvec(c, FL_V), s));                          // v = s2 - R Sigma s2
    int nb = 0;
    // b = 0: the (Ainv - Binv) operand is not used; R stands in for both
    HIPCHK(launch_contract_kmm(kp, c->U, mp, c->m, mp, flvec(c, FL_A), c->Binv, c->Binv, c->Binv,
                               0.5, 0.0, -0.5, flvec(c, FL_V), flvec(c, FL_D1), 0.5,
                               c->slab_small, c->slab_small_cap, &nb, s));
    HIPCHK(launch_colsum(c->slab_small, nb, kp.P, c->sc + SC_G22, s));
  }
  double sc[SC_N];
  int status[4];
  {
    Readback rb(c);
    HIPCHK(rb.add(sc, c->sc, sizeof(sc)));
    HIPCHK(rb.add(status, c->status, sizeof(status)));
    HIPCHK(rb.wait());
  }
  if (chain_watchdog(status)) return SGP_EHIP;
  const double* g22 = sc + SC_G22;
  grad[0] = g22[0];
  for (int q = 0; q < kp.L; ++q) grad[1 + q] = g22[1 + q];
  grad[kp.L + 1] = 2.0 * kp.tau2 * g22[kp.P - 1];   // tau: 2 tau^2 on coincident pairs (Q5)
  return SGP_OK;
}

// newtrapGP's returned `W` and `grad_log_py_ff` (R/newtrapGP.R:96-99): the values at the iterate
// the last update started from, which predict_laplace_full consumes
int sgp_full_laplace_state(sgp_ctx* c, double* W, double* grad_log_py_ff) {
  MULTI_REFUSE(c, "sgp_full_laplace_state");
  if (!c || !W || !grad_log_py_ff) { set_err("invalid arguments"); return SGP_EINVAL; }
  if (!c->fl_valid) {
    set_err("no full-GP Laplace Newton-Raphson step has run since the mode was last set");
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(W, flvec(c, FL_W0), sizeof(double) * c->n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(grad_log_py_ff, flvec(c, FL_D10), sizeof(double) * c->n,
                   hipMemcpyDeviceToHost));
  return SGP_OK;
}

// ------------------------------------------------------------------------- knot posterior
// u | y at the end of the drivers, from the replicated state of the last evaluation:
//   VI / FITC (vi_functions.R:1161-1180, laplace_gradient_ascent.R:1635-1655):
//     u_mean = muu + K22 Bm^-1 t,  u_var = K22 Bm^-1 K22   (= Sigma22 - S + S Bm^-1 S)
//   Laplace (newtrap_sparseGP.R:137-176): u_mean = muu + K22 (K22+S_Z)^-1 t_Z(f_hat),
//     u_var = K22 (K22 + S_B(W_prev))^-1 K22   (= Sigma22 + TT + TT (Sigma22 - TT)^-1 TT)
int sgp_posterior_u(sgp_ctx* c, const double* muu, double* u_mean, double* u_var) {
  MULTI_FWD(c, sgp_posterior_u(multi_lead(c->multi), muu, u_mean, u_var));
  if (!c || !muu || !u_mean || !u_var) { set_err("invalid arguments"); return SGP_EINVAL; }
  if (c->last_mode == 0) { set_err("no completed evaluation in this context"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(c->device));
  const int64_t mp = c->mp, m = c->m;
  const double* vec = c->uvec;
  const double* inv = c->Binv;
  if (c->last_mode == 3) {
    vec = lmv(c, LM_X1);
    if (c->lap_it >= 2) inv = c->Cprev;
  }
  HIPCHK(dense_gemv(c->K22, mp, vec, 1.0, c->T22, c->stream));   // T22 row 0 as scratch
  HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, c->K22, mp, inv, mp, 0.0, c->T1, mp,
                       c->stream));
  HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, c->T1, mp, c->K22, mp, 0.0, c->M3,
                       mp, c->stream));
  std::vector<double> hv((size_t)mp), hm((size_t)(mp * mp));
  HIPCHK(hipMemcpyAsync(hv.data(), c->T22, sizeof(double) * mp, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hm.data(), c->M3, sizeof(double) * mp * mp, hipMemcpyDeviceToHost,
                        c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int64_t j = 0; j < m; ++j) u_mean[j] = muu[j] + hv[(size_t)j];
  for (int64_t j = 0; j < m; ++j)
    for (int64_t i = 0; i < m; ++i) u_var[i + j * m] = hm[(size_t)(i * mp + j)];
  return SGP_OK;
}

// ------------------------------------------------------------------------- EGO scan
// The expected-improvement scan of the EGO knot proposals (include/sgp.h; k_ego.hip).
namespace {
// c->ego (doubles): meta points (128 x SGP_MAXD, column-major) | K22 | its inverse | chain scratch
// R | pivot inverses P (128 x 64) | logd | v - v1 | alpha | out (8) | per-workgroup records
constexpr int64_t EGO_TT = (int64_t)SGP_EGO_TMAX * SGP_EGO_TMAX;
constexpr int64_t EGO_XM = 0, EGO_K22 = EGO_XM + (int64_t)SGP_EGO_TMAX * SGP_MAXD,
                  EGO_INV = EGO_K22 + EGO_TT, EGO_R = EGO_INV + EGO_TT, EGO_P = EGO_R + EGO_TT,
                  EGO_LOGD = EGO_P + (int64_t)SGP_EGO_TMAX * 64, EGO_VEC = EGO_LOGD + 8,
                  EGO_ALPHA = EGO_VEC + SGP_EGO_TMAX, EGO_OUT = EGO_ALPHA + SGP_EGO_TMAX,
                  EGO_REC = EGO_OUT + 8;
constexpr int EGO_MAX_BLOCKS = 4096;
constexpr int64_t EGO_DOUBLES = EGO_REC + 2 * EGO_MAX_BLOCKS;
static_assert(SGP_EGO_TMAX == SGP_TILE, "the meta-model's K22 is one tile of dense_spd_inverse");

int ego_check_args(int d, int kernel, const double* theta, double delta, const double* xm,
                   int64_t T, int64_t ldxm, const double* vals, const double* excl, int64_t E,
                   int64_t ldexcl) {
  if (kernel == SGP_KERNEL_ARD) {
    set_err("sgp_ego_scan supports 'exp' and 'sqexp' (the reference's make_cov_matC returns a "
            "0 x 0 matrix for 'ard')");
    return SGP_EINVAL;
  }
  if (kernel != SGP_KERNEL_SQEXP && kernel != SGP_KERNEL_EXP) {
    set_err("invalid covariance function (kernel=%d)", kernel);
    return SGP_EINVAL;
  }
  if (d < 1 || d > SGP_MAXD) {
    set_err("input dimension d=%d outside [1, %d]", d, SGP_MAXD);
    return SGP_EINVAL;
  }
  if (!theta || !xm || !vals) {
    set_err("sgp_ego_scan: theta_meta, xm and vals must not be NULL");
    return SGP_EINVAL;
  }
  if (T < 1 || T > SGP_EGO_TMAX) {
    set_err("sgp_ego_scan: T=%lld outside [1, %d]", (long long)T, SGP_EGO_TMAX);
    return SGP_EINVAL;
  }
  if (ldxm < T) {
    set_err("sgp_ego_scan: ldxm=%lld < T=%lld", (long long)ldxm, (long long)T);
    return SGP_EINVAL;
  }
  if (excl && (E < 0 || ldexcl < E)) {
    set_err("sgp_ego_scan: invalid exclusion list (E=%lld, ldexcl=%lld)", (long long)E,
            (long long)ldexcl);
    return SGP_EINVAL;
  }
  for (int p = 0; p < 3; ++p)
    if (!std::isfinite(theta[p])) {
      set_err("sgp_ego_scan: theta_meta[%d] is not finite", p);
      return SGP_EINVAL;
    }
  if (!(theta[0] > 0.0) || !(theta[1] > 0.0) || !(theta[2] >= 0.0)) {
    set_err("sgp_ego_scan: needs sigma > 0, l > 0 and tau >= 0 (sigma=%g, l=%g, tau=%g)",
            theta[0], theta[1], theta[2]);
    return SGP_EINVAL;
  }
  if (!(delta >= 0.0) || !std::isfinite(delta)) {
    set_err("sgp_ego_scan: delta_meta=%g is not a finite value >= 0", delta);
    return SGP_EINVAL;
  }
  for (int64_t j = 0; j < T; ++j)
    if (!std::isfinite(vals[j])) {
      set_err("sgp_ego_scan: vals[%lld] is not finite", (long long)j);
      return SGP_EINVAL;
    }
  for (int q = 0; q < d; ++q)
    for (int64_t j = 0; j < T; ++j)
      if (!std::isfinite(xm[j + q * ldxm])) {
        set_err("sgp_ego_scan: xm[%lld, %d] is not finite", (long long)j, q);
        return SGP_EINVAL;
      }
  return SGP_OK;
}

int ego_ensure(sgp_ctx* c, int64_t E) {
  if (!c->ego) {
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    c->ego_blocks = std::min(EGO_MAX_BLOCKS, std::max(1, 8 * cus));
    int st = dalloc(&c->ego_sync, SGP_GJ_SYNC_WORDS);
    st = st ? st : dalloc(&c->ego_status, 4);
    st = st ? st : dalloc(&c->ego_rows, 3 * c->n_pad);
    st = st ? st : dalloc(&c->ego, EGO_DOUBLES);   // last: marks the set as complete
    if (st) {
      if (c->ego_sync) (void)hipFree(c->ego_sync);
      if (c->ego_status) (void)hipFree(c->ego_status);
      if (c->ego_rows) (void)hipFree(c->ego_rows);
      c->ego_sync = nullptr;
      c->ego_status = nullptr;
      c->ego_rows = nullptr;
      c->ego = nullptr;
      return st;
    }
  }
  const int64_t need = E * c->d;
  if (need > c->ego_ex_cap) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->ego_ex) (void)hipFree(c->ego_ex);
    c->ego_ex = nullptr;
    c->ego_ex_cap = 0;
    const int st = dalloc(&c->ego_ex, need);
    if (st) return st;
    c->ego_ex_cap = need;
  }
  return SGP_OK;
}
}  // namespace

extern "C++" {   // sgp_multi.h hook
// sgp_ego_scan on a one-device context (or one shard); *best_row = -1 when every row is excluded
int sgp_internal_ego_scan(sgp_ctx* c, int kernel, const double* theta, double delta,
                          const double* xm, int64_t T, int64_t ldxm, const double* vals,
                          const double* excl, int64_t E, int64_t ldexcl, int64_t* best_row,
                          double* best_ei, double* ei_out, double* mean_out, double* var_out) {
  KernParams kp;
  int st = make_params(kernel, c->d, theta, delta, &kp);
  if (st) return st;
  const int d = c->d;
  constexpr int64_t TM = SGP_EGO_TMAX;
  // exclusion list: the rows that can match something (no NaN), sorted by coordinate 0
  std::vector<double> hex;
  int64_t Ex = 0;
  if (excl && E > 0) {
    std::vector<int64_t> idx;
    for (int64_t k = 0; k < E; ++k) {
      bool ok = true;
      for (int q = 0; q < d && ok; ++q) ok = !std::isnan(excl[k + q * ldexcl]);
      if (ok) idx.push_back(k);
    }
    std::stable_sort(idx.begin(), idx.end(),
                     [&](int64_t a, int64_t b) { return excl[a] < excl[b]; });
    Ex = (int64_t)idx.size();
    hex.resize((size_t)(Ex * d));
    for (int q = 0; q < d; ++q)
      for (int64_t k = 0; k < Ex; ++k) hex[(size_t)(k + q * Ex)] = excl[idx[(size_t)k] + q * ldexcl];
  }
  HIPCHK(hipSetDevice(c->device));
  st = ego_ensure(c, Ex);
  if (st) return st;
  hipStream_t s = c->stream;
  double vmax = vals[0];
  std::vector<double> hxm((size_t)(TM * d), 0.0), hv((size_t)TM, 0.0);
  for (int q = 0; q < d; ++q)
    for (int64_t j = 0; j < T; ++j) hxm[(size_t)(q * TM + j)] = xm[j + q * ldxm];
  for (int64_t j = 0; j < T; ++j) {
    hv[(size_t)j] = vals[j] - vals[0];
    vmax = vals[j] > vmax ? vals[j] : vmax;
  }
  double* w = c->ego;
  timers_reset(c);
  {
    Scope sc(c, "ego_meta");   // uploads, K22, its inverse, alpha
    // (the host buffers outlive the copies: every path below synchronises the stream or fails)
    HIPCHK(hipMemcpyAsync(w + EGO_XM, hxm.data(), sizeof(double) * hxm.size(),
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w + EGO_VEC, hv.data(), sizeof(double) * TM, hipMemcpyHostToDevice, s));
    if (Ex > 0)
      HIPCHK(hipMemcpyAsync(c->ego_ex, hex.data(), sizeof(double) * hex.size(),
                            hipMemcpyHostToDevice, s));
    // the chain's sync words must be zero when it starts (a failed chain may leave them set)
    HIPCHK(hipMemsetAsync(c->ego_status, 0, sizeof(int) * 4, s));
    HIPCHK(hipMemsetAsync(c->ego_sync, 0, sizeof(unsigned) * SGP_GJ_SYNC_WORDS, s));
    // K22 = k(xm, xm) + (tau^2 + delta_meta) I, padded to the tile with a unit diagonal
    HIPCHK(launch_build_kmm(kp, w + EGO_XM, TM, T, TM, 0.0, w + EGO_K22, s, w + EGO_INV));
    HIPCHK(dense_spd_inverse(w + EGO_INV, TM, w + EGO_R, w + EGO_P, w + EGO_LOGD, c->ego_status,
                             c->ego_sync, s));
    HIPCHK(dense_gemv(w + EGO_INV, TM, w + EGO_VEC, 1.0, w + EGO_ALPHA, s));
  }
  EgoScan a;
  a.X = c->X;
  a.ldx = c->n_pad;
  a.n = c->n;
  a.d = d;
  a.T = (int)T;
  a.kexp = kernel == SGP_KERNEL_EXP ? 1 : 0;
  a.coef = kp.coef;
  a.sig2 = kp.sig2;
  a.c0 = kp.sig2 + kp.tau2;
  a.tau2 = kp.tau2;
  a.v1 = vals[0];
  a.vmax = vmax;
  a.xm = w + EGO_XM;
  a.Ainv = w + EGO_INV;
  a.alpha = w + EGO_ALPHA;
  a.ex = c->ego_ex;
  a.E = Ex;
  a.ei_out = ei_out ? c->ego_rows : nullptr;
  a.mean_out = mean_out ? c->ego_rows + c->n_pad : nullptr;
  a.var_out = var_out ? c->ego_rows + 2 * c->n_pad : nullptr;
  a.rec = w + EGO_REC;
  {
    Scope sc(c, "ego_scan");   // the pass over X and its one-block final reduction
    HIPCHK(launch_ego_scan(a, c->ego_blocks, c->ego_status, w + EGO_OUT, s));
  }
  double ho[3] = {0.0, -1.0, 0.0};
  HIPCHK(hipMemcpyAsync(ho, w + EGO_OUT, sizeof(ho), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (ho[2] < 0.0) {
    set_err("internal error: a Gauss-Jordan chain's wait watchdog expired");
    return SGP_EHIP;
  }
  if (ho[2] != 0.0) {
    set_err("meta-model K22 is not positive definite (leading minor of order %d)", (int)ho[2]);
    return SGP_ENOTPD;
  }
  const size_t nb = sizeof(double) * (size_t)c->n;
  if (ei_out) HIPCHK(hipMemcpyAsync(ei_out, a.ei_out, nb, hipMemcpyDeviceToHost, s));
  if (mean_out) HIPCHK(hipMemcpyAsync(mean_out, a.mean_out, nb, hipMemcpyDeviceToHost, s));
  if (var_out) HIPCHK(hipMemcpyAsync(var_out, a.var_out, nb, hipMemcpyDeviceToHost, s));
  if (ei_out || mean_out || var_out) HIPCHK(hipStreamSynchronize(s));
  *best_row = (int64_t)ho[1];
  *best_ei = ho[0];
  return SGP_OK;
}
}  // extern "C++"

int sgp_diag_ego_args(int d, int kernel, const double* theta_meta, double delta_meta,
                      const double* xm, int64_t T, int64_t ldxm, const double* vals,
                      const double* excl, int64_t E, int64_t ldexcl) {
  return ego_check_args(d, kernel, theta_meta, delta_meta, xm, T, ldxm, vals, excl, E, ldexcl);
}

int sgp_ego_scan(sgp_ctx* c, int kernel, const double* theta_meta, double delta_meta,
                 const double* xm, int64_t T, int64_t ldxm, const double* vals,
                 const double* excl, int64_t E, int64_t ldexcl, int64_t* best_row,
                 double* best_ei, double* ei_out, double* mean_out, double* var_out) {
  if (!c || !best_row || !best_ei) {
    set_err("sgp_ego_scan: ctx, best_row and best_ei must not be NULL");
    return SGP_EINVAL;
  }
  int st = ego_check_args(c->d, kernel, theta_meta, delta_meta, xm, T, ldxm, vals, excl, E, ldexcl);
  if (st) return st;
  if (c->multi)
    st = multi_ego_scan(c->multi, kernel, theta_meta, delta_meta, xm, T, ldxm, vals, excl, E,
                        ldexcl, best_row, best_ei, ei_out, mean_out, var_out);
  else
    st = sgp_internal_ego_scan(c, kernel, theta_meta, delta_meta, xm, T, ldxm, vals, excl, E,
                               ldexcl, best_row, best_ei, ei_out, mean_out, var_out);
  if (st) return st;
  if (*best_row < 0) {
    set_err("sgp_ego_scan: no data row outside the knots (every row is excluded)");
    return SGP_EINVAL;
  }
  return SGP_OK;
}

// ------------------------------------------------------------------------- fit scan
// The predictive variance / error scan of knot_prop_var and knot_prop_error (include/sgp.h;
// k_scan.hip): predict_laplace(full_cov = FALSE) at the context's own rows, and the arg-max.
namespace {
// c->scan (doubles): u_var | K22^-1 u_var | K22^-1 u_var K22^-1 | A | the d scales | f (n_pad)
constexpr int64_t SCAN_V = 0, SCAN_T1 = SCAN_V + EGO_TT, SCAN_T22 = SCAN_T1 + EGO_TT,
                  SCAN_A = SCAN_T22 + EGO_TT, SCAN_RL = SCAN_A + EGO_TT,
                  SCAN_F = SCAN_RL + SGP_MAXD;

int scan_check_args(int d, int kernel, const double* theta, double delta, const double* U,
                    int64_t m, int64_t ldu, const double* u_mean, const double* muu,
                    const double* u_var, int64_t ldv, int mode, const double* excl, int64_t E,
                    int64_t ldexcl) {
  if (kernel == SGP_KERNEL_EXP) {   // as sgp_predict: no fit carries it (optimize_gp.R:263)
    set_err("sgp_fit_scan supports 'sqexp' and 'ard', as prediction does");
    return SGP_EINVAL;
  }
  if (kernel != SGP_KERNEL_SQEXP && kernel != SGP_KERNEL_ARD) {
    set_err("invalid covariance function (kernel=%d)", kernel);
    return SGP_EINVAL;
  }
  if (d < 1 || d > SGP_MAXD) {
    set_err("input dimension d=%d outside [1, %d]", d, SGP_MAXD);
    return SGP_EINVAL;
  }
  if (!theta || !U || !u_mean || !muu || !u_var) {
    set_err("sgp_fit_scan: theta, U, u_mean, muu and u_var must not be NULL");
    return SGP_EINVAL;
  }
  if (mode != SGP_SCAN_VAR && mode != SGP_SCAN_ERROR) {
    set_err("sgp_fit_scan: mode=%d is neither SGP_SCAN_VAR nor SGP_SCAN_ERROR", mode);
    return SGP_EINVAL;
  }
  if (m < 1 || m > SGP_EGO_TMAX) {
    set_err("sgp_fit_scan: m=%lld outside [1, %d]", (long long)m, SGP_EGO_TMAX);
    return SGP_EINVAL;
  }
  if (ldu < m) {
    set_err("sgp_fit_scan: ldu=%lld < m=%lld", (long long)ldu, (long long)m);
    return SGP_EINVAL;
  }
  if (ldv < m) {
    set_err("sgp_fit_scan: ldv=%lld < m=%lld", (long long)ldv, (long long)m);
    return SGP_EINVAL;
  }
  if (excl && (E < 0 || ldexcl < E)) {
    set_err("sgp_fit_scan: invalid exclusion list (E=%lld, ldexcl=%lld)", (long long)E,
            (long long)ldexcl);
    return SGP_EINVAL;
  }
  const int L = num_ls(kernel, d);
  for (int p = 0; p < L + 2; ++p)
    if (!std::isfinite(theta[p])) {
      set_err("sgp_fit_scan: theta[%d] is not finite", p);
      return SGP_EINVAL;
    }
  if (!(theta[0] > 0.0) || !(theta[L + 1] >= 0.0)) {
    set_err("sgp_fit_scan: needs sigma > 0 and tau >= 0 (sigma=%g, tau=%g)", theta[0],
            theta[L + 1]);
    return SGP_EINVAL;
  }
  for (int p = 0; p < L; ++p)
    if (!(theta[1 + p] > 0.0)) {
      set_err("sgp_fit_scan: needs l > 0 (length scale %d is %g)", p + 1, theta[1 + p]);
      return SGP_EINVAL;
    }
  if (!(delta >= 0.0) || !std::isfinite(delta)) {
    set_err("sgp_fit_scan: delta=%g is not a finite value >= 0", delta);
    return SGP_EINVAL;
  }
  for (int64_t j = 0; j < m; ++j) {
    if (!std::isfinite(u_mean[j])) {
      set_err("sgp_fit_scan: u_mean[%lld] is not finite", (long long)j);
      return SGP_EINVAL;
    }
    if (!std::isfinite(muu[j])) {
      set_err("sgp_fit_scan: muu[%lld] is not finite", (long long)j);
      return SGP_EINVAL;
    }
  }
  for (int q = 0; q < d; ++q)
    for (int64_t j = 0; j < m; ++j)
      if (!std::isfinite(U[j + q * ldu])) {
        set_err("sgp_fit_scan: U[%lld, %d] is not finite", (long long)j, q);
        return SGP_EINVAL;
      }
  for (int64_t k = 0; k < m; ++k)
    for (int64_t j = 0; j < m; ++j)
      if (!std::isfinite(u_var[j + k * ldv])) {
        set_err("sgp_fit_scan: u_var[%lld, %lld] is not finite", (long long)j, (long long)k);
        return SGP_EINVAL;
      }
  return SGP_OK;
}

int fit_scan_run(sgp_ctx* c, int kernel, const double* theta, double delta, int gaussian,
                 const double* U, int64_t m, int64_t ldu, const double* u_mean, const double* muu,
                 const double* u_var, int64_t ldv, int mode, const double* f, const double* excl,
                 int64_t E, int64_t ldexcl, int64_t* best_row, double* best_key, double* key_out,
                 double* mean_out, double* var_out) {
  KernParams kp;
  int st = make_params(kernel, c->d, theta, delta, &kp);
  if (st) return st;
  const int d = c->d;
  constexpr int64_t TM = SGP_EGO_TMAX;
  const bool resident_f = mode == SGP_SCAN_ERROR && !f;
  if (resident_f && (!c->lv || c->lap_objs.empty())) {
    set_err("sgp_fit_scan: f is NULL and no Laplace evaluation has run on this context");
    return SGP_EINVAL;
  }
  // exclusion list: the rows that can match something (no NaN), sorted by coordinate 0
  std::vector<double> hex;
  int64_t Ex = 0;
  if (excl && E > 0) {
    std::vector<int64_t> idx;
    for (int64_t k = 0; k < E; ++k) {
      bool ok = true;
      for (int q = 0; q < d && ok; ++q) ok = !std::isnan(excl[k + q * ldexcl]);
      if (ok) idx.push_back(k);
    }
    std::stable_sort(idx.begin(), idx.end(),
                     [&](int64_t a, int64_t b) { return excl[a] < excl[b]; });
    Ex = (int64_t)idx.size();
    hex.resize((size_t)(Ex * d));
    for (int q = 0; q < d; ++q)
      for (int64_t k = 0; k < Ex; ++k) hex[(size_t)(k + q * Ex)] = excl[idx[(size_t)k] + q * ldexcl];
  }
  HIPCHK(hipSetDevice(c->device));
  st = ego_ensure(c, Ex);
  if (st) return st;
  if (!c->scan) {
    st = dalloc(&c->scan, SCAN_F + c->n_pad);
    if (st) return st;
  }
  hipStream_t s = c->stream;
  std::vector<double> hxu((size_t)(TM * d), 0.0), hd((size_t)TM, 0.0), hV((size_t)EGO_TT, 0.0),
      hrl((size_t)SGP_MAXD, 1.0);
  for (int q = 0; q < d; ++q)
    for (int64_t j = 0; j < m; ++j) hxu[(size_t)(q * TM + j)] = U[j + q * ldu];
  for (int64_t j = 0; j < m; ++j) hd[(size_t)j] = u_mean[j] - muu[j];
  for (int64_t i = 0; i < m; ++i)
    for (int64_t j = 0; j < m; ++j) hV[(size_t)(i * TM + j)] = u_var[i + j * ldv];
  if (kernel == SGP_KERNEL_ARD)
    for (int q = 0; q < d; ++q) hrl[(size_t)q] = kp.rl[q];
  double* w = c->ego;
  double* w2 = c->scan;
  timers_reset(c);
  {
    Scope sc(c, "scan_mm");   // uploads, K22, its inverse, w and A
    // (the host buffers outlive the copies: every path below synchronises the stream or fails)
    HIPCHK(hipMemcpyAsync(w + EGO_XM, hxu.data(), sizeof(double) * hxu.size(),
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w + EGO_VEC, hd.data(), sizeof(double) * TM, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w2 + SCAN_V, hV.data(), sizeof(double) * EGO_TT, hipMemcpyHostToDevice,
                          s));
    HIPCHK(hipMemcpyAsync(w2 + SCAN_RL, hrl.data(), sizeof(double) * SGP_MAXD,
                          hipMemcpyHostToDevice, s));
    if (mode == SGP_SCAN_ERROR && f)
      HIPCHK(hipMemcpyAsync(w2 + SCAN_F, f, sizeof(double) * (size_t)c->n, hipMemcpyHostToDevice,
                            s));
    if (Ex > 0)
      HIPCHK(hipMemcpyAsync(c->ego_ex, hex.data(), sizeof(double) * hex.size(),
                            hipMemcpyHostToDevice, s));
    // the chain's sync words must be zero when it starts (a failed chain may leave them set):
    // zeroed on the launch stream, which a null-stream hipMemset would not be ordered with
    HIPCHK(hipMemsetAsync(c->ego_status, 0, sizeof(int) * 4, s));
    HIPCHK(hipMemsetAsync(c->ego_sync, 0, sizeof(unsigned) * SGP_GJ_SYNC_WORDS, s));
    // K22 = Kuu + delta I (gaussian: the tau^2 I is subtracted again) or Kuu + (tau^2 + delta) I
    // (laplace_approx_prediction.R:25-62), padded to the tile with a unit diagonal
    HIPCHK(launch_build_kmm(kp, w + EGO_XM, TM, m, TM, gaussian ? kp.tau2 : 0.0, w + EGO_K22, s,
                            w + EGO_INV));
    HIPCHK(dense_spd_inverse(w + EGO_INV, TM, w + EGO_R, w + EGO_P, w + EGO_LOGD, c->ego_status,
                             c->ego_sync, s));
    HIPCHK(dense_gemv(w + EGO_INV, TM, w + EGO_VEC, 1.0, w + EGO_ALPHA, s));
    HIPCHK(launch_gemm64(false, false, false, TM, TM, TM, 1.0, w + EGO_INV, TM, w2 + SCAN_V, TM,
                         0.0, w2 + SCAN_T1, TM, s));
    HIPCHK(launch_gemm64(false, false, false, TM, TM, TM, 1.0, w2 + SCAN_T1, TM, w + EGO_INV, TM,
                         0.0, w2 + SCAN_T22, TM, s));
    HIPCHK(dense_axpby(1.0, w + EGO_INV, -1.0, w2 + SCAN_T22, w2 + SCAN_A, EGO_TT, s));
  }
  FitScan a;
  a.X = c->X;
  a.ldx = c->n_pad;
  a.n = c->n;
  a.d = d;
  a.m = (int)m;
  a.mode = mode;
  a.coef = kp.coef;
  a.sig2 = kp.sig2;
  a.c0 = kp.sig2 + kp.tau2;
  a.rl = w2 + SCAN_RL;
  a.mu = c->mu;
  a.f = mode == SGP_SCAN_ERROR ? (resident_f ? lvec(c, LV_F) : w2 + SCAN_F) : nullptr;
  a.xu = w + EGO_XM;
  a.A = w2 + SCAN_A;
  a.w = w + EGO_ALPHA;
  a.ex = c->ego_ex;
  a.E = Ex;
  a.key_out = key_out ? c->ego_rows : nullptr;
  a.mean_out = mean_out ? c->ego_rows + c->n_pad : nullptr;
  a.var_out = var_out ? c->ego_rows + 2 * c->n_pad : nullptr;
  a.rec = w + EGO_REC;
  {
    Scope sc(c, "fit_scan");   // the pass over X and its one-block final reduction
    HIPCHK(launch_fit_scan(a, c->ego_blocks, c->ego_status, w + EGO_OUT, s));
  }
  double ho[3] = {0.0, -1.0, 0.0};
  HIPCHK(hipMemcpyAsync(ho, w + EGO_OUT, sizeof(ho), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (ho[2] < 0.0) {
    set_err("internal error: a Gauss-Jordan chain's wait watchdog expired");
    return SGP_EHIP;
  }
  if (ho[2] != 0.0) {
    set_err("scan K22 is not positive definite (leading minor of order %d)", (int)ho[2]);
    return SGP_ENOTPD;
  }
  const size_t nb = sizeof(double) * (size_t)c->n;
  if (key_out) HIPCHK(hipMemcpyAsync(key_out, a.key_out, nb, hipMemcpyDeviceToHost, s));
  if (mean_out) HIPCHK(hipMemcpyAsync(mean_out, a.mean_out, nb, hipMemcpyDeviceToHost, s));
  if (var_out) HIPCHK(hipMemcpyAsync(var_out, a.var_out, nb, hipMemcpyDeviceToHost, s));
  if (key_out || mean_out || var_out) HIPCHK(hipStreamSynchronize(s));
  *best_row = (int64_t)ho[1];
  *best_key = ho[0];
  return SGP_OK;
}
}  // namespace

int sgp_diag_fit_scan_args(int d, int kernel, const double* theta, double delta, const double* U,
                           int64_t m, int64_t ldu, const double* u_mean, const double* muu,
                           const double* u_var, int64_t ldv, int mode, const double* excl,
                           int64_t E, int64_t ldexcl) {
  return scan_check_args(d, kernel, theta, delta, U, m, ldu, u_mean, muu, u_var, ldv, mode, excl,
                         E, ldexcl);
}

int sgp_fit_scan(sgp_ctx* c, int kernel, const double* theta, double delta, int gaussian,
                 const double* U, int64_t m, int64_t ldu, const double* u_mean, const double* muu,
                 const double* u_var, int64_t ldv, int mode, const double* f, const double* excl,
                 int64_t E, int64_t ldexcl, int64_t* best_row, double* best_key, double* key_out,
                 double* mean_out, double* var_out) {
  if (!c || !best_row || !best_key) {
    set_err("sgp_fit_scan: ctx, best_row and best_key must not be NULL");
    return SGP_EINVAL;
  }
  int st = scan_check_args(c->d, kernel, theta, delta, U, m, ldu, u_mean, muu, u_var, ldv, mode,
                           excl, E, ldexcl);
  if (st) return st;
  if (c->multi) {
    set_err("sgp_fit_scan: multi-device contexts are not supported (predict at the rows instead)");
    return SGP_EINVAL;
  }
  st = fit_scan_run(c, kernel, theta, delta, gaussian, U, m, ldu, u_mean, muu, u_var, ldv, mode, f,
                    excl, E, ldexcl, best_row, best_key, key_out, mean_out, var_out);
  if (st) return st;
  if (*best_row < 0) {
    set_err("sgp_fit_scan: every row is excluded");
    return SGP_EINVAL;
  }
  return SGP_OK;
}

// ------------------------------------------------------------------------- prediction
namespace {
struct DevBuf {
  double* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};
struct StreamGuard {
  hipStream_t s = nullptr;
  ~StreamGuard() {
    if (s) {
      (void)hipStreamSynchronize(s);
      (void)hipStreamDestroy(s);
    }
  }
};
struct IntBuf {
  int* p = nullptr;
  ~IntBuf() { if (p) (void)hipFree(p); }
};

// sgp_predict_nlp's scoring request (checked by nlp_check_args before predict_run is entered)
struct PredScore {
  int family;
  const double* y;
  double par;
  const double* expo;
  double* nlp;
  double* stats;
};

bool is_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// The argument checks of sgp_nlp / sgp_predict_nlp; no device call.
int nlp_check_args(const char* who, int family, const double* y, int64_t n, double par,
                   const double* expo, const double* nlp, const double* stats) {
  if (!y || !nlp || !stats || n < 1) {
    set_err("%s: NULL argument or n < 1", who);
    return SGP_EINVAL;
  }
  if (family != SGP_FAM_POISSON && family != SGP_FAM_BERNOULLI && family != SGP_FAM_GAUSSIAN) {
    set_err("%s: unknown family %d", who, family);
    return SGP_EINVAL;
  }
  if (expo && family != SGP_FAM_POISSON) {
    set_err("%s: a per-row exposure is for the poisson family only", who);
    return SGP_EINVAL;
  }
  if (family == SGP_FAM_GAUSSIAN && !(is_finite(par) && par >= 0.0)) {
    set_err("%s: gaussian tau = %g is not finite and >= 0", who, par);
    return SGP_EINVAL;
  }
  if (family == SGP_FAM_POISSON && !expo && !(is_finite(par) && par > 0.0)) {
    set_err("%s: poisson exposure m = %g is not positive and finite", who, par);
    return SGP_EINVAL;
  }
  for (int64_t i = 0; i < n; ++i) {
    if (!is_finite(y[i])) {
      set_err("%s: y[%lld] = %g is not finite", who, (long long)i, y[i]);
      return SGP_EINVAL;
    }
    if (family == SGP_FAM_BERNOULLI && !(y[i] == 0.0 || y[i] == 1.0)) {
      set_err("%s: bernoulli y[%lld] = %g is not 0 or 1", who, (long long)i, y[i]);
      return SGP_EINVAL;
    }
    if (family == SGP_FAM_POISSON && !(y[i] >= 0.0 && y[i] == floor(y[i]))) {
      set_err("%s: poisson y[%lld] = %g is not a non-negative integer", who, (long long)i, y[i]);
      return SGP_EINVAL;
    }
    if (expo && !(is_finite(expo[i]) && expo[i] > 0.0)) {
      set_err("%s: poisson exposure expo[%lld] = %g is not positive and finite", who,
              (long long)i, expo[i]);
      return SGP_EINVAL;
    }
  }
  return SGP_OK;
}

// the scoring grid's cap: eight workgroups per compute unit
int nlp_max_blocks(int device, int* out) {
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  *out = 8 * (cus > 0 ? cus : 1);
  return SGP_OK;
}

// sgp_nlp's body.  max_blocks = 0: the product's; kernel_ms (or NULL): the two scoring launches'
// time by HIP events (sgp_diag_nlp)
int nlp_run(int device, int family, int max_blocks, const double* y,
            const double* pred_mean, const double* pred_var, int64_t n, double par,
            const double* expo, double* nlp, double* stats, double* kernel_ms) {
  if (!pred_mean || !pred_var) {
    set_err("sgp_nlp: NULL argument or n < 1");
    return SGP_EINVAL;
  }
  int st = nlp_check_args("sgp_nlp", family, y, n, par, expo, nlp, stats);
  if (st) return st;
  if (max_blocks < 0) {
    set_err("sgp_nlp: max_blocks < 0");
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  if (max_blocks == 0 && (st = nlp_max_blocks(device, &max_blocks))) return st;
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t s = sg.s;
  DevBuf dy, dm, dv, de, dn, part, dst;
  st = dalloc(&dy.p, n);
  st = st ? st : dalloc(&dm.p, n);
  st = st ? st : dalloc(&dv.p, n);
  st = st ? st : dalloc(&dn.p, n);
  st = st ? st : dalloc(&part.p, nlp_part_doubles(n));
  st = st ? st : dalloc(&dst.p, 4);
  if (!st && expo) st = dalloc(&de.p, n);
  if (st) return st;
  const size_t nb = sizeof(double) * (size_t)n;
  HIPCHK(hipMemcpyAsync(dy.p, y, nb, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dm.p, pred_mean, nb, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dv.p, pred_var, nb, hipMemcpyHostToDevice, s));
  if (expo) HIPCHK(hipMemcpyAsync(de.p, expo, nb, hipMemcpyHostToDevice, s));
  NlpArgs a{dy.p, dm.p, dv.p, expo ? de.p : nullptr, par, n, dn.p, part.p};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (kernel_ms) {
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, s));
  }
  hipError_t le = launch_nlp_rows(family, a, max_blocks, dst.p, s);
  if (kernel_ms && le == hipSuccess) le = hipEventRecord(e1, s);
  if (le == hipSuccess) le = hipMemcpyAsync(nlp, dn.p, nb, hipMemcpyDeviceToHost, s);
  if (le == hipSuccess) le = hipMemcpyAsync(stats, dst.p, sizeof(double) * 4, hipMemcpyDeviceToHost, s);
  if (le == hipSuccess) le = hipStreamSynchronize(s);
  if (kernel_ms) {
    float ms = 0.0f;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, e0, e1);
    *kernel_ms = (double)ms;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  HIPCHK(le);
  return SGP_OK;
}

int predict_run(int device, int kernel, const double* theta, double delta, int method,
                int gaussian, const double* U, int64_t m, int64_t ldu, const double* u_mean,
                const double* muu, const double* u_var, int64_t ldv, const double* x_pred,
                int64_t np, int64_t ldxp, int d, const double* mu_pred, int full_cov,
                double* pred_mean, double* pred_var, int64_t ldpv, const PredScore* sc);
}  // namespace

int sgp_nlp(int device, int family, const double* y, const double* pred_mean,
            const double* pred_var, int64_t n, double par, const double* expo, double* nlp,
            double* stats) {
  return nlp_run(device, family, 0, y, pred_mean, pred_var, n, par, expo, nlp, stats, nullptr);
}

int sgp_diag_nlp(int device, int family, int max_blocks, const double* y,
                 const double* pred_mean, const double* pred_var, int64_t n, double par,
                 const double* expo, double* nlp, double* stats, double* kernel_ms) {
  return nlp_run(device, family, max_blocks, y, pred_mean, pred_var, n, par, expo, nlp, stats,
                 kernel_ms);
}

int sgp_predict(int device, int kernel, const double* theta, double delta, int method,
                int gaussian, const double* U, int64_t m, int64_t ldu, const double* u_mean,
                const double* muu, const double* u_var, int64_t ldv, const double* x_pred,
                int64_t np, int64_t ldxp, int d, const double* mu_pred, int full_cov,
                double* pred_mean, double* pred_var, int64_t ldpv) {
  return predict_run(device, kernel, theta, delta, method, gaussian, U, m, ldu, u_mean, muu, u_var,
                     ldv, x_pred, np, ldxp, d, mu_pred, full_cov, pred_mean, pred_var, ldpv,
                     nullptr);
}

int sgp_predict_nlp(int device, int kernel, const double* theta, double delta, int method,
                    int gaussian, const double* U, int64_t m, int64_t ldu, const double* u_mean,
                    const double* muu, const double* u_var, int64_t ldv, const double* x_pred,
                    int64_t np, int64_t ldxp, int d, const double* mu_pred, double* pred_mean,
                    double* pred_var, int family, const double* y_pred, double par,
                    const double* expo, double* nlp, double* stats) {
  int st = nlp_check_args("sgp_predict_nlp", family, y_pred, np, par, expo, nlp, stats);
  if (st) return st;
  const PredScore sc{family, y_pred, par, expo, nlp, stats};
  return predict_run(device, kernel, theta, delta, method, gaussian, U, m, ldu, u_mean, muu, u_var,
                     ldv, x_pred, np, ldxp, d, mu_pred, 0, pred_mean, pred_var, 0, &sc);
}

// ------------------------------------------------------- joint scoring and draws (k_joint.hip)
namespace {
// A covariance on the device and its Cholesky factor (dense_chol)
struct CholWork {
  DevBuf raw, A, L, Linv, logd;
  IntBuf status;
  int64_t n = 0, np = 0;
  double logdet = 0.0;
};

// a stage's time by HIP events, added to *acc; off (no events, no waits) when acc == nullptr
struct StageTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double* acc = nullptr;
  hipStream_t s = nullptr;
  ~StageTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  hipError_t init(double* a, hipStream_t st) {
    acc = a;
    s = st;
    if (!acc) return hipSuccess;
    hipError_t e = hipEventCreate(&e0);
    return e != hipSuccess ? e : hipEventCreate(&e1);
  }
  hipError_t begin() { return acc ? hipEventRecord(e0, s) : hipSuccess; }
  hipError_t end(int stage) {
    if (!acc) return hipSuccess;
    hipError_t e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    acc[stage] += (double)ms;
    return e;
  }
};

bool all_finite(const double* v, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!is_finite(v[i])) return false;
  return true;
}

// cov (n x n column-major, ld ldc, lower triangle read) + diag_add I -> w.L, w.Linv, w.logdet.
// SGP_ENOTPD names `name` and the order.  The upload and the Schur-complement copy are freed.
int chol_factor(CholWork& w, const char* who, const char* name, const double* cov, int64_t n,
                int64_t ldc, double diag_add, hipStream_t s, StageTimer* tm) {
  const int64_t np = round_up(n, SGP_DB), nb = np / SGP_DB;
  w.n = n;
  w.np = np;
  int st = dalloc(&w.raw.p, n * n);
  st = st ? st : dalloc(&w.A.p, np * np);
  st = st ? st : dalloc(&w.L.p, np * np);
  st = st ? st : dalloc(&w.Linv.p, np * SGP_DB);
  st = st ? st : dalloc(&w.logd.p, nb);
  st = st ? st : dalloc(&w.status.p, 4);
  if (st) return st;
  HIPCHK(hipMemcpy2DAsync(w.raw.p, sizeof(double) * n, cov, sizeof(double) * ldc,
                          sizeof(double) * n, (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(w.status.p, 0, sizeof(int) * 4, s));
  HIPCHK(launch_chol_prep(w.raw.p, n, n, diag_add, w.A.p, np, s));
  if (tm) HIPCHK(tm->begin());
  HIPCHK(dense_chol(w.A.p, np, w.L.p, w.Linv.p, w.logd.p, w.status.p, s));
  if (tm) HIPCHK(tm->end(0));
  int hs[4];
  std::vector<double> ld((size_t)nb);
  HIPCHK(hipMemcpyAsync(hs, w.status.p, sizeof(hs), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(ld.data(), w.logd.p, sizeof(double) * nb, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  (void)hipFree(w.raw.p);
  w.raw.p = nullptr;
  (void)hipFree(w.A.p);
  w.A.p = nullptr;
  if (hs[0]) {
    set_err("%s: chol(): the leading minor of order %d of %s is not positive definite", who, hs[0],
            name);
    return SGP_ENOTPD;
  }
  double a = 0.0;
  for (int64_t k = 0; k < nb; ++k) a += ld[(size_t)k];
  w.logdet = 2.0 * a;
  return SGP_OK;
}

// |L^-1 v|^2 for a host n-vector v: the solve on an np x 64 right-hand side whose first column is v
int chol_quad(const CholWork& w, const double* v, hipStream_t s, double* q) {
  const int64_t np = w.np, cnt = np * SGP_DB;
  DevBuf B, X, part, out;
  int st = dalloc(&B.p, cnt);
  st = st ? st : dalloc(&X.p, cnt);
  st = st ? st : dalloc(&part.p, 256);
  st = st ? st : dalloc(&out.p, 1);
  if (st) return st;
  std::vector<double> h((size_t)cnt, 0.0);
  for (int64_t i = 0; i < w.n; ++i) h[(size_t)(i * SGP_DB)] = v[i];
  HIPCHK(hipMemcpyAsync(B.p, h.data(), sizeof(double) * cnt, hipMemcpyHostToDevice, s));
  HIPCHK(chol_solve_lower(w.L.p, w.Linv.p, np, B.p, SGP_DB, X.p, s));
  HIPCHK(launch_dot(X.p, X.p, cnt, part.p, out.p, s));
  HIPCHK(hipMemcpyAsync(q, out.p, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return SGP_OK;
}

// draws per chunk: the workspace Z and F (2 np S_c doubles) stays under 512 MB; the chunks are
// of equal length (a multiple of 64), so that the last one's padding stays below 64 columns each
int64_t joint_chunk(int64_t np, int64_t S, int chunk_draws) {
  if (chunk_draws > 0) return chunk_draws < S ? chunk_draws : S;
  int64_t cap = ((int64_t)512 << 20) / (16 * np) / 64 * 64;
  if (cap < 64) cap = 64;
  const int64_t nchunk = (S + cap - 1) / cap;
  const int64_t sc = round_up((S + nchunk - 1) / nchunk, 64);
  return sc < S ? sc : S;
}

int joint_common_args(const char* who, const double* mean, int64_t n, int64_t ldc) {
  if (n > SGP_JOINT_NMAX) {
    set_err("%s: n = %lld above the limit %d", who, (long long)n, SGP_JOINT_NMAX);
    return SGP_EINVAL;
  }
  if (ldc < n) {
    set_err("%s: leading dimension %lld below n = %lld", who, (long long)ldc, (long long)n);
    return SGP_EINVAL;
  }
  if (!all_finite(mean, n)) {
    set_err("%s: the mean is not finite", who);
    return SGP_EINVAL;
  }
  return SGP_OK;
}

// sgp_sample_mvn's body.  chunk_draws / max_blocks = 0: the product's; stage_ms (or NULL): 4
// doubles {factor, Z fill, products, scoring} by HIP events
int sample_run(int device, const double* mean, const double* cov, int64_t n, int64_t ldc,
               int64_t S, uint64_t seed, double* out, int64_t ldo, int chunk_draws,
               int max_blocks, double* stage_ms) {
  const char* who = "sgp_sample_mvn";
  if (!mean || !cov || !out || n < 1 || S < 1) {
    set_err("%s: NULL argument, n < 1 or S < 1", who);
    return SGP_EINVAL;
  }
  int st = joint_common_args(who, mean, n, ldc);
  if (st) return st;
  if (ldo < S) {
    set_err("%s: leading dimension ldo = %lld below S = %lld", who, (long long)ldo, (long long)S);
    return SGP_EINVAL;
  }
  if (chunk_draws < 0 || max_blocks < 0) {
    set_err("%s: chunk_draws < 0 or max_blocks < 0", who);
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  if (max_blocks == 0 && (st = nlp_max_blocks(device, &max_blocks))) return st;
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t s = sg.s;
  StageTimer tm;
  if (stage_ms) stage_ms[0] = stage_ms[1] = stage_ms[2] = stage_ms[3] = 0.0;
  HIPCHK(tm.init(stage_ms, s));
  CholWork w;
  if ((st = chol_factor(w, who, "cov", cov, n, ldc, 0.0, s, &tm))) return st;
  const int64_t np = w.np, sc = joint_chunk(np, S, chunk_draws), ldz = round_up(sc, 64);
  DevBuf dm, Z, F;
  st = dalloc(&dm.p, n);
  st = st ? st : dalloc(&Z.p, np * ldz);
  st = st ? st : dalloc(&F.p, np * ldz);
  if (st) return st;
  HIPCHK(hipMemcpyAsync(dm.p, mean, sizeof(double) * n, hipMemcpyHostToDevice, s));
  for (int64_t s0 = 0; s0 < S; s0 += sc) {
    const int64_t cnt = S - s0 < sc ? S - s0 : sc;
    HIPCHK(tm.begin());
    HIPCHK(launch_joint_fill(seed, s0, cnt, ldz, n, np, dm.p, Z.p, F.p, max_blocks, s));
    HIPCHK(tm.end(1));
    HIPCHK(tm.begin());
    HIPCHK(launch_joint_product(w.L.p, np, Z.p, F.p, ldz, s));
    HIPCHK(tm.end(2));
    // row i of F holds draws s0 .. s0 + cnt - 1 of f_i: column i of out, rows s0 ..
    HIPCHK(hipMemcpy2DAsync(out + s0, sizeof(double) * ldo, F.p, sizeof(double) * ldz,
                            sizeof(double) * cnt, (size_t)n, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return SGP_OK;
}

// sgp_joint_nlp's body (chunk_draws, max_blocks, stage_ms as sample_run)
int joint_run(int device, int family, const double* y, const double* pred_mean,
              const double* pred_cov, int64_t n, int64_t ldc, double par, const double* expo,
              int64_t S, uint64_t seed, double* out, int chunk_draws, int max_blocks,
              double* stage_ms) {
  const char* who = "sgp_joint_nlp";
  if (!pred_mean || !pred_cov) {
    set_err("%s: NULL argument or n < 1", who);
    return SGP_EINVAL;
  }
  int st = nlp_check_args(who, family, y, n, par, expo, out, out);
  if (st) return st;
  if ((st = joint_common_args(who, pred_mean, n, ldc))) return st;
  if (family != SGP_FAM_GAUSSIAN && S < 1) {
    set_err("%s: S = %lld < 1", who, (long long)S);
    return SGP_EINVAL;
  }
  if (chunk_draws < 0 || max_blocks < 0) {
    set_err("%s: chunk_draws < 0 or max_blocks < 0", who);
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  if (max_blocks == 0 && (st = nlp_max_blocks(device, &max_blocks))) return st;
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t s = sg.s;
  StageTimer tm;
  if (stage_ms) stage_ms[0] = stage_ms[1] = stage_ms[2] = stage_ms[3] = 0.0;
  HIPCHK(tm.init(stage_ms, s));
  CholWork w;
  if (family == SGP_FAM_GAUSSIAN) {
    // -dmvnorm(y, pred_mean, pred_cov + tau^2 I, log = TRUE) as written (quirk Q23)
    if ((st = chol_factor(w, who, "pred_cov + tau^2 I", pred_cov, n, ldc, par * par, s, &tm)))
      return st;
    std::vector<double> r((size_t)n);
    for (int64_t i = 0; i < n; ++i) r[(size_t)i] = y[i] - pred_mean[i];
    double q = 0.0;
    if ((st = chol_quad(w, r.data(), s, &q))) return st;
    out[0] = 0.5 * ((double)n * 1.8378770664093454836 + w.logdet + q);   // log(2 pi)
    out[1] = out[2] = nan("");
    return SGP_OK;
  }
  if ((st = chol_factor(w, who, "pred_cov", pred_cov, n, ldc, 0.0, s, &tm))) return st;
  const int64_t np = w.np, sc = joint_chunk(np, S, chunk_draws), ldz = round_up(sc, 64);
  const bool pois = family == SGP_FAM_POISSON;
  DevBuf dy, dm, da, Z, F, ll, dst;
  st = dalloc(&dy.p, n);
  st = st ? st : dalloc(&dm.p, n);
  st = st ? st : dalloc(&Z.p, np * ldz);
  st = st ? st : dalloc(&F.p, np * ldz);
  st = st ? st : dalloc(&ll.p, S);
  st = st ? st : dalloc(&dst.p, 3);
  if (!st && pois) st = dalloc(&da.p, 3 * n);
  if (st) return st;
  HIPCHK(hipMemcpyAsync(dy.p, y, sizeof(double) * n, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dm.p, pred_mean, sizeof(double) * n, hipMemcpyHostToDevice, s));
  std::vector<double> aux;
  if (pois) {
    // dpois(y, exp(f) m): the per-row constants log m_i, m_i, log(y_i!)
    aux.resize((size_t)(3 * n));
    for (int64_t i = 0; i < n; ++i) {
      const double m = expo ? expo[i] : par;
      aux[(size_t)i] = log(m);
      aux[(size_t)(n + i)] = m;
      aux[(size_t)(2 * n + i)] = quad_lfact(y[i]);
    }
    HIPCHK(hipMemcpyAsync(da.p, aux.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
  }
  for (int64_t s0 = 0; s0 < S; s0 += sc) {
    const int64_t cnt = S - s0 < sc ? S - s0 : sc;
    HIPCHK(tm.begin());
    HIPCHK(launch_joint_fill(seed, s0, cnt, ldz, n, np, dm.p, Z.p, F.p, max_blocks, s));
    HIPCHK(tm.end(1));
    HIPCHK(tm.begin());
    HIPCHK(launch_joint_product(w.L.p, np, Z.p, F.p, ldz, s));
    HIPCHK(tm.end(2));
    HIPCHK(tm.begin());
    HIPCHK(launch_joint_score(family, dy.p, pois ? da.p : nullptr, n, F.p, ldz, cnt, ll.p + s0,
                              max_blocks, s));
    HIPCHK(tm.end(3));
  }
  HIPCHK(tm.begin());
  HIPCHK(launch_joint_stats(ll.p, S, dst.p, s));
  HIPCHK(tm.end(3));
  double hs[3];
  HIPCHK(hipMemcpyAsync(hs, dst.p, sizeof(hs), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const double lmax = hs[0], mean = hs[1], sd = hs[2];
  out[0] = -(lmax + log(mean));
  out[1] = exp(lmax) * sd;
  out[2] = sd / (mean * sqrt((double)S));
  return SGP_OK;
}
}  // namespace

int sgp_sample_mvn(int device, const double* mean, const double* cov, int64_t n, int64_t ldc,
                   int64_t S, uint64_t seed, double* out, int64_t ldo) {
  return sample_run(device, mean, cov, n, ldc, S, seed, out, ldo, 0, 0, nullptr);
}

int sgp_diag_sample_mvn(int device, int chunk_draws, int max_blocks, const double* mean,
                        const double* cov, int64_t n, int64_t ldc, int64_t S, uint64_t seed,
                        double* out, int64_t ldo, double* stage_ms) {
  return sample_run(device, mean, cov, n, ldc, S, seed, out, ldo, chunk_draws, max_blocks,
                    stage_ms);
}

int sgp_joint_nlp(int device, int family, const double* y, const double* pred_mean,
                  const double* pred_cov, int64_t n, int64_t ldc, double par, const double* expo,
                  int64_t S, uint64_t seed, double* out) {
  return joint_run(device, family, y, pred_mean, pred_cov, n, ldc, par, expo, S, seed, out, 0, 0,
                   nullptr);
}

int sgp_diag_joint_nlp(int device, int family, int chunk_draws, int max_blocks, const double* y,
                       const double* pred_mean, const double* pred_cov, int64_t n, int64_t ldc,
                       double par, const double* expo, int64_t S, uint64_t seed, double* out,
                       double* stage_ms) {
  return joint_run(device, family, y, pred_mean, pred_cov, n, ldc, par, expo, S, seed, out,
                   chunk_draws, max_blocks, stage_ms);
}

int sgp_joint_kl(int device, const double* mean1, const double* mean2, const double* sigma1,
                 int64_t ld1, const double* sigma2, int64_t ld2, int64_t n, double* kl) {
  const char* who = "sgp_joint_kl";
  if (!mean1 || !mean2 || !sigma1 || !sigma2 || !kl || n < 1) {
    set_err("%s: NULL argument or n < 1", who);
    return SGP_EINVAL;
  }
  int st = joint_common_args(who, mean1, n, ld1);
  if (!st) st = joint_common_args(who, mean2, n, ld2);
  if (st) return st;
  HIPCHK(hipSetDevice(device));
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t s = sg.s;
  CholWork w1, w2;
  if ((st = chol_factor(w1, who, "sigma1", sigma1, n, ld1, 0.0, s, nullptr))) return st;
  if ((st = chol_factor(w2, who, "sigma2", sigma2, n, ld2, 0.0, s, nullptr))) return st;
  // my_kl(mv = TRUE) as written (R/evaluation_functions.R:155-163):
  //   tr(sigma2^-1 sigma1) = |L2^-1 L1|_F^2, the padded identity's np - n ones taken off
  const int64_t np = w1.np;
  DevBuf X, part, out;
  st = dalloc(&X.p, np * np);
  st = st ? st : dalloc(&part.p, 256);
  st = st ? st : dalloc(&out.p, 1);
  if (st) return st;
  HIPCHK(chol_solve_lower(w2.L.p, w2.Linv.p, np, w1.L.p, np, X.p, s));   // L1 is overwritten
  HIPCHK(launch_dot(X.p, X.p, np * np, part.p, out.p, s));
  double tr = 0.0, q = 0.0;
  HIPCHK(hipMemcpyAsync(&tr, out.p, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  tr -= (double)(np - n);
  std::vector<double> dmean((size_t)n);
  for (int64_t i = 0; i < n; ++i) dmean[(size_t)i] = mean2[i] - mean1[i];
  if ((st = chol_quad(w2, dmean.data(), s, &q))) return st;
  // sum(log(diag(chol2))) - sum(log(diag(chol1))): half the log-determinant difference
  *kl = 0.5 * (tr + q - (double)n + 0.5 * w2.logdet - 0.5 * w1.logdet);
  return SGP_OK;
}

int sgp_mc_nlp(int device, const double* y, const double* pred_mean, const double* pred_var,
               int64_t n, int64_t S, uint64_t seed, double* nlp, double* mcsd) {
  const char* who = "sgp_mc_nlp";
  if (!pred_mean || !pred_var || !mcsd) {
    set_err("%s: NULL argument or n < 1", who);
    return SGP_EINVAL;
  }
  int st = nlp_check_args(who, SGP_FAM_BERNOULLI, y, n, 0.0, nullptr, nlp, mcsd);
  if (st) return st;
  if (S < 1) {
    set_err("%s: S = %lld < 1", who, (long long)S);
    return SGP_EINVAL;
  }
  if (!all_finite(pred_mean, n)) {
    set_err("%s: the mean is not finite", who);
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t s = sg.s;
  DevBuf dy, dm, dv, dn, ds;
  st = dalloc(&dy.p, n);
  st = st ? st : dalloc(&dm.p, n);
  st = st ? st : dalloc(&dv.p, n);
  st = st ? st : dalloc(&dn.p, n);
  st = st ? st : dalloc(&ds.p, n);
  if (st) return st;
  const size_t nb = sizeof(double) * (size_t)n;
  HIPCHK(hipMemcpyAsync(dy.p, y, nb, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dm.p, pred_mean, nb, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dv.p, pred_var, nb, hipMemcpyHostToDevice, s));
  HIPCHK(launch_mc_rows(seed, dy.p, dm.p, dv.p, n, S, dn.p, ds.p, s));
  HIPCHK(hipMemcpyAsync(nlp, dn.p, nb, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(mcsd, ds.p, nb, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return SGP_OK;
}

int sgp_diag_chol(int device, const double* A, int64_t n, int64_t lda, double* L, int64_t ldl,
                  double* logdet) {
  const char* who = "sgp_diag_chol";
  if (!A || !L || !logdet || n < 1) {
    set_err("%s: NULL argument or n < 1", who);
    return SGP_EINVAL;
  }
  if (n > SGP_JOINT_NMAX || lda < n || ldl < n) {
    set_err("%s: n = %lld above the limit %d or a leading dimension below n", who, (long long)n,
            SGP_JOINT_NMAX);
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  CholWork w;
  int st = chol_factor(w, who, "A", A, n, lda, 0.0, sg.s, nullptr);
  if (st) return st;
  const int64_t np = w.np;
  std::vector<double> h((size_t)(np * np));
  HIPCHK(hipMemcpyAsync(h.data(), w.L.p, sizeof(double) * np * np, hipMemcpyDeviceToHost, sg.s));
  HIPCHK(hipStreamSynchronize(sg.s));
  for (int64_t j = 0; j < n; ++j)
    for (int64_t i = 0; i < n; ++i) L[i + j * ldl] = h[(size_t)(i * np + j)];
  *logdet = w.logdet;
  return SGP_OK;
}

int sgp_diag_gemm64(int device, int64_t n, int reps, double* best_ms) {
  if (!best_ms || n < 64 || n % 64 || n > SGP_JOINT_NMAX || reps < 1) {
    set_err("sgp_diag_gemm64: NULL argument, n not a multiple of 64 in [64, %d] or reps < 1",
            SGP_JOINT_NMAX);
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  DevBuf A, B, Cm;
  int st = dalloc(&A.p, n * n);
  st = st ? st : dalloc(&B.p, n * n);
  st = st ? st : dalloc(&Cm.p, n * n);
  if (st) return st;
  HIPCHK(launch_normals(1, 0, n, n, A.p, sg.s));
  HIPCHK(launch_normals(2, 0, n, n, B.p, sg.s));
  double ms[1] = {0.0}, best = 0.0;
  StageTimer tm;
  HIPCHK(tm.init(ms, sg.s));
  for (int r = 0; r <= reps; ++r) {   // the first launch is a warm-up
    ms[0] = 0.0;
    HIPCHK(tm.begin());
    HIPCHK(launch_gemm64(false, false, false, n, n, n, 1.0, A.p, n, B.p, n, 0.0, Cm.p, n, sg.s));
    HIPCHK(tm.end(0));
    if (r == 1 || (r > 1 && ms[0] < best)) best = ms[0];
  }
  *best_ms = best;
  return SGP_OK;
}

int sgp_diag_normals(int device, uint64_t seed, int stream, int64_t S, int64_t n, double* out) {
  if (!out || S < 1 || n < 1 || (stream != 0 && stream != 1)) {
    set_err("sgp_diag_normals: NULL argument, S < 1, n < 1 or a stream other than 0 and 1");
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  DevBuf d;
  int st = dalloc(&d.p, S * n);
  if (st) return st;
  HIPCHK(launch_normals(seed, stream, S, n, d.p, sg.s));
  HIPCHK(hipMemcpyAsync(out, d.p, sizeof(double) * S * n, hipMemcpyDeviceToHost, sg.s));
  HIPCHK(hipStreamSynchronize(sg.s));
  return SGP_OK;
}

namespace {
// sgp_predict (sc == nullptr) and sgp_predict_nlp (sc: score the prediction on the device)
int predict_run(int device, int kernel, const double* theta, double delta, int method,
                int gaussian, const double* U, int64_t m, int64_t ldu, const double* u_mean,
                const double* muu, const double* u_var, int64_t ldv, const double* x_pred,
                int64_t np, int64_t ldxp, int d, const double* mu_pred, int full_cov,
                double* pred_mean, double* pred_var, int64_t ldpv, const PredScore* sc) {
  KernParams kp;
  int st = make_params(kernel, d, theta, delta, &kp);
  if (st) return st;
  if (kernel == SGP_KERNEL_EXP) {   // build_knm_range has no 'exp' form; no fit carries it
    set_err("prediction supports 'sqexp' and 'ard' (optimize_gp.R:263 rejects others)");
    return SGP_EINVAL;
  }
  // predict_laplace_full (R/laplace_approx_prediction.R:128-214): U = xy, u_mean =
  // grad_log_py_ff, muu = W of the newtrapGP fit
  const bool lapfull = method == SGP_PRED_LAPLACE_FULL;
  // u_var unused (zero): Sigma22 = the data block
  const bool full = method == SGP_PRED_FULL || lapfull;
  if (!U || m < 1 || ldu < m || !u_mean || !muu || (!u_var && !full) || (!full && ldv < m) ||
      !x_pred || np < 1 ||
      ldxp < np || !mu_pred || !pred_mean || !pred_var || (full_cov && ldpv < np)) {
    set_err("invalid sgp_predict arguments");
    return SGP_EINVAL;
  }
  {
    std::vector<double> plo, phi;
    col_range(x_pred, np, ldxp, d, &plo, &phi);
    set_center(&kp, U, m, ldu, plo.data(), phi.data());
  }
  if (method != SGP_PRED_VI && method != SGP_PRED_LAPLACE && method != SGP_PRED_FULL &&
      !lapfull) {
    set_err("invalid prediction method %d", method);
    return SGP_EINVAL;
  }
  for (int64_t j = 0; lapfull && j < m; ++j)
    if (!(muu[j] <= 0.0)) {   // W = d2 log p(y|f) / df2 enters as sqrt(-W)
      set_err("SGP_PRED_LAPLACE_FULL: W[%lld] = %g is not <= 0", (long long)j, muu[j]);
      return SGP_EINVAL;
    }
  if (method == SGP_PRED_VI && !gaussian) {
    set_err("Error: VI not supported for non-gaussian data.");   // predict_gp, l.424-427
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t s = sg.s;
  const int64_t mp = round_up(m, SGP_TILE), npp = round_up(np, SGP_TILE), mm = mp * mp;
  DevBuf dU, K22, Kinv, R, Pb, logd, V, T1, T22, wv, Xp, Kp, yv, rowq, q, S, Y;
  IntBuf status, gsync;
  st = dalloc(&dU.p, mp * d);
  st = st ? st : dalloc(&K22.p, mm);
  st = st ? st : dalloc(&Kinv.p, mm);
  st = st ? st : dalloc(&R.p, mm);
  st = st ? st : dalloc(&Pb.p, mp * 64);
  st = st ? st : dalloc(&logd.p, mp / SGP_DB);
  st = st ? st : dalloc(&V.p, mm);
  st = st ? st : dalloc(&T1.p, mm);
  st = st ? st : dalloc(&T22.p, mm);
  st = st ? st : dalloc(&wv.p, 2 * mp);
  st = st ? st : dalloc(&Xp.p, npp * d);
  st = st ? st : dalloc(&Kp.p, npp * mp);
  st = st ? st : dalloc(&yv.p, npp);
  st = st ? st : dalloc(&rowq.p, npp * (mp / SGP_TILE));
  st = st ? st : dalloc(&q.p, npp);
  st = st ? st : dalloc(&status.p, 4);
  st = st ? st : dalloc(&gsync.p, SGP_GJ_SYNC_WORDS);
  if (!st && full_cov) {
    st = dalloc(&S.p, npp * npp);
    st = st ? st : dalloc(&Y.p, npp * mp);
  }
  if (st) return st;
  {
    std::vector<double> hU((size_t)(mp * d), 0.0), hX((size_t)(npp * d), 0.0);
    for (int c = 0; c < d; ++c) {
      for (int64_t j = 0; j < m; ++j) hU[(size_t)(c * mp + j)] = U[j + c * ldu];
      for (int64_t i = 0; i < np; ++i) hX[(size_t)(c * npp + i)] = x_pred[i + c * ldxp];
    }
    std::vector<double> hd((size_t)mp, 0.0), hV((size_t)mm, 0.0);
    for (int64_t j = 0; j < m; ++j)
      hd[(size_t)j] = lapfull ? sqrt(-muu[j]) : u_mean[j] - muu[j];   // lapfull: sqrt(-W)
    if (lapfull) {
      std::vector<double> hg((size_t)mp, 0.0);
      for (int64_t j = 0; j < m; ++j) hg[(size_t)j] = u_mean[j];
      HIPCHK(hipMemcpy(wv.p, hg.data(), sizeof(double) * mp, hipMemcpyHostToDevice));
    }
    if (!full)
      for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j < m; ++j) hV[(size_t)(i * mp + j)] = u_var[i + j * ldv];
    HIPCHK(hipMemcpy(dU.p, hU.data(), sizeof(double) * hU.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(Xp.p, hX.data(), sizeof(double) * hX.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(wv.p + mp, hd.data(), sizeof(double) * mp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(V.p, hV.data(), sizeof(double) * mm, hipMemcpyHostToDevice));
    // on the launch stream: the null stream's hipMemset is not ordered before a non-blocking
    // stream's kernels (the chain's sync words must be zero when it starts)
    HIPCHK(hipMemsetAsync(status.p, 0, sizeof(int) * 4, s));
    HIPCHK(hipMemsetAsync(gsync.p, 0, sizeof(int) * SGP_GJ_SYNC_WORDS, s));
  }
  // Sigma22: the gaussian family subtracts tau^2 I again (vi_functions.R:1246-1260,
  // laplace_approx_prediction.R:25-43) -> diagonal sigma^2 + delta; otherwise Kuu+(tau^2+delta)I
  // (predict_gp_full, laplace_approx_prediction.R:281-405: Sigma22 = k(xy, xy) + (tau^2+delta) I)
  const double diag_sub = (gaussian && !full) ? kp.tau2 : 0.0;
  HIPCHK(launch_build_kmm(kp, dU.p, mp, m, mp, diag_sub, K22.p, s));
  const bool lap_full = (method == SGP_PRED_LAPLACE) && full_cov;
  if (lapfull) {
    // t(v) %*% v = Sigma12 R Sigma21 with R = sW (I + sW Sigma sW)^-1 sW (l.169, 188, 206):
    // temp22 = -R; the mean's multiplier grad_log_py_ff is in wv already (l.209)
    HIPCHK(launch_flap_scale(true, K22.p, wv.p + mp, Kinv.p, mp, m, s));
    HIPCHK(dense_spd_inverse(Kinv.p, mp, R.p, Pb.p, logd.p, status.p,
                             reinterpret_cast<unsigned*>(gsync.p), s));
    HIPCHK(launch_flap_scale(false, Kinv.p, wv.p + mp, Kinv.p, mp, m, s));
    HIPCHK(dense_axpby(0.0, V.p, -1.0, Kinv.p, T22.p, mm, s));   // V holds zeros
  } else {
    HIPCHK(hipMemcpyAsync(Kinv.p, K22.p, sizeof(double) * mm, hipMemcpyDeviceToDevice, s));
    HIPCHK(dense_spd_inverse(Kinv.p, mp, R.p, Pb.p, logd.p, status.p,
                             reinterpret_cast<unsigned*>(gsync.p), s));
    HIPCHK(dense_gemv(Kinv.p, mp, wv.p + mp, 1.0, wv.p, s));        // Sigma22^-1 (u_mean - muu)
    HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, Kinv.p, mp, V.p, mp, 0.0, T1.p, mp,
                         s));
    HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, T1.p, mp, Kinv.p, mp, 0.0, T22.p,
                         mp, s));                                     // Sigma22^-1 u_var Sigma22^-1
    if (!lap_full) HIPCHK(dense_axpby(1.0, T22.p, -1.0, Kinv.p, T22.p, mm, s));   // temp22
  }
  HIPCHK(launch_build_knm(kp, Xp.p, npp, np, npp, dU.p, mp, m, mp, Kp.p, s));
  HIPCHK(launch_gemv_rows(Kp.p, npp, mp, wv.p, nullptr, yv.p, nullptr, s));
  std::vector<double> hy((size_t)npp), hq((size_t)npp, 0.0);
  // vi_functions.R:1321: tau^2 + sigma^2 + delta; laplace_approx_prediction.R:114: sigma^2 + tau^2
  // predict_gp_full: diag(Sigma11) = sigma^2 + tau^2 + delta
  const double c0 = (method == SGP_PRED_VI) ? (kp.tau2 + kp.sig2) + delta
                                            : (full ? (kp.sig2 + kp.tau2) + delta
                                                    : kp.sig2 + kp.tau2);
  if (!full_cov) {
    HIPCHK(launch_rowquad_knm(kp, Kp.p, T22.p, np, npp, m, mp, nullptr, 0.0, nullptr, nullptr,
                              nullptr, rowq.p, q.p, s));
    if (sc) {
      // pred_mean and pred_var formed and scored on the device; one readback of the np-vectors
      int max_blocks = 0;
      if ((st = nlp_max_blocks(device, &max_blocks))) return st;
      DevBuf dmu, dy, de, dpm, dpv, dn, part, dst;
      st = dalloc(&dmu.p, np);
      st = st ? st : dalloc(&dy.p, np);
      st = st ? st : dalloc(&dpm.p, np);
      st = st ? st : dalloc(&dpv.p, np);
      st = st ? st : dalloc(&dn.p, np);
      st = st ? st : dalloc(&part.p, nlp_part_doubles(np));
      st = st ? st : dalloc(&dst.p, 4);
      if (!st && sc->expo) st = dalloc(&de.p, np);
      if (st) return st;
      const size_t nb = sizeof(double) * (size_t)np;
      HIPCHK(hipMemcpyAsync(dmu.p, mu_pred, nb, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(dy.p, sc->y, nb, hipMemcpyHostToDevice, s));
      if (sc->expo) HIPCHK(hipMemcpyAsync(de.p, sc->expo, nb, hipMemcpyHostToDevice, s));
      HIPCHK(launch_pred_finish(dmu.p, yv.p, q.p, c0, np, dpm.p, dpv.p, s));
      NlpArgs a{dy.p, dpm.p, dpv.p, sc->expo ? de.p : nullptr, sc->par, np, dn.p, part.p};
      HIPCHK(launch_nlp_rows(sc->family, a, max_blocks, dst.p, s));
      int hst[4];
      HIPCHK(hipMemcpyAsync(pred_mean, dpm.p, nb, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(pred_var, dpv.p, nb, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(sc->nlp, dn.p, nb, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(sc->stats, dst.p, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(hst, status.p, sizeof(hst), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (hst[0]) {
        set_err("%s is not positive definite (leading minor of order %d)",
                lapfull ? "I + sqrt(-W) %*% Sigma %*% sqrt(-W)" : "Sigma22", hst[0]);
        return SGP_ENOTPD;
      }
      return SGP_OK;
    }
  } else {
    if (lap_full)
      HIPCHK(launch_rowquad_knm(kp, Kp.p, Kinv.p, np, npp, m, mp, nullptr, 0.0, nullptr, nullptr,
                                nullptr, rowq.p, q.p, s));
    if (method == SGP_PRED_VI || full)   // Sigma11 of x_pred with its tau^2 + delta diagonal
      HIPCHK(launch_fill_cov(kp, Xp.p, np, npp, Xp.p, np, npp, true, S.p, npp, s));
    else
      HIPCHK(hipMemsetAsync(S.p, 0, sizeof(double) * npp * npp, s));
    HIPCHK(launch_gemm64(false, false, false, npp, mp, mp, 1.0, Kp.p, mp, T22.p, mp, 0.0, Y.p, mp,
                         s));
    HIPCHK(launch_gemm64(false, true, false, npp, npp, mp, 1.0, Y.p, mp, Kp.p, mp, 1.0, S.p, npp,
                         s));
  }
  int hst[4];
  HIPCHK(hipMemcpyAsync(hy.data(), yv.p, sizeof(double) * npp, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hq.data(), q.p, sizeof(double) * npp, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hst, status.p, sizeof(hst), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (hst[0]) {
    set_err("%s is not positive definite (leading minor of order %d)",
            lapfull ? "I + sqrt(-W) %*% Sigma %*% sqrt(-W)" : "Sigma22", hst[0]);
    return SGP_ENOTPD;
  }
  for (int64_t i = 0; i < np; ++i) pred_mean[i] = mu_pred[i] + hy[(size_t)i];
  if (!full_cov) {
    for (int64_t i = 0; i < np; ++i) pred_var[i] = c0 + hq[(size_t)i];
    return SGP_OK;
  }
  std::vector<double> hS((size_t)(npp * npp));
  HIPCHK(hipMemcpyAsync(hS.data(), S.p, sizeof(double) * hS.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int64_t j = 0; j < np; ++j)
    for (int64_t i = 0; i < np; ++i) pred_var[i + j * ldpv] = hS[(size_t)(i * npp + j)];
  if (lap_full) {   // diag(diag(Sigma11 - Q)) + Q with Sigma11_ii = sigma^2 + tau^2 + delta
    const double c11 = (kp.sig2 + kp.tau2) + delta;
    for (int64_t i = 0; i < np; ++i) pred_var[i + i * ldpv] += c11 - hq[(size_t)i];
  }
  return SGP_OK;
}
}  // namespace

// ------------------------------------------------------------------------- resident predictor
// sgp_predictor_* (include/sgp.h): sgp_predict's m x m stage once, at create,
// and then any number of batches streamed through a fixed chunk work space.
struct sgp_predictor {
  int device = 0;
  hipStream_t stream = nullptr;   // non-blocking, owned: create and the host-buffer runs
  KernParams kp;                  // without the builder's centre and span (set per run)
  int d = 0, method = 0;
  int64_t m = 0, mp = 0;
  double c0 = 0.0;
  std::vector<double> hU;         // m x d column-major (ld m): the centre and span of a run
  // resident: knots (mp x d, ld mp), w (mp), T22 and its symmetric block form A' (mp x mp), the
  // register route's -S and scales (mp = 128 only), the chain's status
  double *dU = nullptr, *w = nullptr, *T22 = nullptr, *Ap = nullptr, *negA = nullptr,
         *rl = nullptr, *scan_rec = nullptr;
  int* status = nullptr;
  int max_blocks = 1;
  int64_t chunk_rows = 0;         // the product's chunk (SGP_PRED_BUDGET)
  // chunk work space for `cap` rows: X (ld cap), K (cap x mp), mu, mean, var, the two slabs
  int64_t cap = 0;
  double *Xc = nullptr, *K = nullptr, *mu = nullptr, *pm = nullptr, *pv = nullptr,
         *qslab = nullptr, *yslab = nullptr;
};

namespace {
// The K work space's byte budget: of 64, 128, 256 and 1024 MiB at C3's rows with m = 1024 the
// largest had the shortest call (profiles/predictor/README.md: the tile kernel itself is a
// little faster at 256 MiB, the per-chunk copies and launches cost more than that)
constexpr int64_t SGP_PRED_BUDGET = (int64_t)1024 << 20;
// knots up to which route 0 takes the register route (k_fit_scan's pass)
constexpr int64_t SGP_PRED_M0 = 64;

void pred_free_ws(sgp_predictor* p) {
  for (double** q : {&p->Xc, &p->K, &p->mu, &p->pm, &p->pv, &p->qslab, &p->yslab}) {
    if (*q) (void)hipFree(*q);
    *q = nullptr;
  }
  p->cap = 0;
}

void pred_free(sgp_predictor* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  pred_free_ws(p);
  for (double** q : {&p->dU, &p->w, &p->T22, &p->Ap, &p->negA, &p->rl, &p->scan_rec})
    if (*q) (void)hipFree(*q);
  if (p->status) (void)hipFree(p->status);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

struct PredGuard {
  sgp_predictor* p = nullptr;
  ~PredGuard() { pred_free(p); }
};

// The chunk plan: the largest multiple of 128 rows whose K work space stays within the budget
// (never below one tile), no more than np needs.
void pred_plan(int64_t m, int64_t np, int64_t budget, int64_t* chunk_rows, int64_t* nchunks) {
  const int64_t mp = round_up(m, SGP_TILE);
  int64_t rows = budget / (mp * (int64_t)sizeof(double)) / SGP_TILE * SGP_TILE;
  if (rows < SGP_TILE) rows = SGP_TILE;
  const int64_t need = round_up(np, SGP_TILE);
  if (rows > need) rows = need;
  *chunk_rows = rows;
  *nchunks = (np + rows - 1) / rows;
}

int pred_ensure(sgp_predictor* p, int64_t rows) {
  if (rows <= p->cap) return SGP_OK;
  HIPCHK(hipStreamSynchronize(p->stream));
  pred_free_ws(p);
  const int64_t nb = p->mp / SGP_TILE;
  int st = dalloc(&p->Xc, rows * p->d);
  st = st ? st : dalloc(&p->K, rows * p->mp);
  st = st ? st : dalloc(&p->mu, rows);
  st = st ? st : dalloc(&p->pm, rows);
  st = st ? st : dalloc(&p->pv, rows);
  st = st ? st : dalloc(&p->qslab, rows * nb);
  st = st ? st : dalloc(&p->yslab, rows * (nb < 2 ? 2 : nb));
  if (st) {
    pred_free_ws(p);
    return st;
  }
  // rows past a chunk's end are read by the builder (and written as K = 0): finite values
  HIPCHK(hipMemsetAsync(p->Xc, 0, sizeof(double) * rows * p->d, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  p->cap = rows;
  return SGP_OK;
}

// The argument checks of sgp_predictor_create (sgp_diag_predictor_args); no device call.
int pred_check_args(int d, int kernel, const double* theta, double delta, int method,
                    int gaussian, const double* U, int64_t m, int64_t ldu, const double* u_mean,
                    const double* muu, const double* u_var, int64_t ldv) {
  if (kernel == SGP_KERNEL_EXP) {   // as sgp_predict: no fit carries it (optimize_gp.R:263)
    set_err("sgp_predictor supports 'sqexp' and 'ard' (optimize_gp.R:263 rejects others)");
    return SGP_EINVAL;
  }
  if (kernel != SGP_KERNEL_SQEXP && kernel != SGP_KERNEL_ARD) {
    set_err("invalid covariance function (kernel=%d)", kernel);
    return SGP_EINVAL;
  }
  if (d < 1 || d > SGP_MAXD) {
    set_err("input dimension d=%d outside [1, %d]", d, SGP_MAXD);
    return SGP_EINVAL;
  }
  if (method != SGP_PRED_VI && method != SGP_PRED_LAPLACE && method != SGP_PRED_FULL &&
      method != SGP_PRED_LAPLACE_FULL) {
    set_err("invalid prediction method %d", method);
    return SGP_EINVAL;
  }
  const bool lapfull = method == SGP_PRED_LAPLACE_FULL;
  const bool full = method == SGP_PRED_FULL || lapfull;
  if (!theta || !U || !u_mean || !muu || (!u_var && !full)) {
    set_err("sgp_predictor: theta, U, u_mean, muu and (sparse methods) u_var must not be NULL");
    return SGP_EINVAL;
  }
  if (m < 1) {
    set_err("sgp_predictor: m=%lld < 1", (long long)m);
    return SGP_EINVAL;
  }
  if (ldu < m) {
    set_err("sgp_predictor: ldu=%lld < m=%lld", (long long)ldu, (long long)m);
    return SGP_EINVAL;
  }
  if (!full && ldv < m) {
    set_err("sgp_predictor: ldv=%lld < m=%lld", (long long)ldv, (long long)m);
    return SGP_EINVAL;
  }
  const int L = num_ls(kernel, d);
  for (int p = 0; p < L + 2; ++p)
    if (!std::isfinite(theta[p])) {
      set_err("sgp_predictor: theta[%d] is not finite", p);
      return SGP_EINVAL;
    }
  if (!(theta[0] > 0.0) || !(theta[L + 1] >= 0.0)) {
    set_err("sgp_predictor: needs sigma > 0 and tau >= 0 (sigma=%g, tau=%g)", theta[0],
            theta[L + 1]);
    return SGP_EINVAL;
  }
  for (int p = 0; p < L; ++p)
    if (!(theta[1 + p] > 0.0)) {
      set_err("sgp_predictor: needs l > 0 (length scale %d is %g)", p + 1, theta[1 + p]);
      return SGP_EINVAL;
    }
  if (!std::isfinite(delta)) {   // its sign is left to the factorisation, as in sgp_predict
    set_err("sgp_predictor: delta=%g is not finite", delta);
    return SGP_EINVAL;
  }
  for (int64_t j = 0; j < m; ++j) {
    if (!std::isfinite(u_mean[j])) {
      set_err("sgp_predictor: u_mean[%lld] is not finite", (long long)j);
      return SGP_EINVAL;
    }
    if (!std::isfinite(muu[j])) {
      set_err("sgp_predictor: muu[%lld] is not finite", (long long)j);
      return SGP_EINVAL;
    }
  }
  for (int q = 0; q < d; ++q)
    for (int64_t j = 0; j < m; ++j)
      if (!std::isfinite(U[j + q * ldu])) {
        set_err("sgp_predictor: U[%lld, %d] is not finite", (long long)j, q);
        return SGP_EINVAL;
      }
  for (int64_t k = 0; !full && k < m; ++k)
    for (int64_t j = 0; j < m; ++j)
      if (!std::isfinite(u_var[j + k * ldv])) {
        set_err("sgp_predictor: u_var[%lld, %lld] is not finite", (long long)j, (long long)k);
        return SGP_EINVAL;
      }
  for (int64_t j = 0; lapfull && j < m; ++j)
    if (!(muu[j] <= 0.0)) {   // W = d2 log p(y|f) / df2 enters as sqrt(-W)
      set_err("SGP_PRED_LAPLACE_FULL: W[%lld] = %g is not <= 0", (long long)j, muu[j]);
      return SGP_EINVAL;
    }
  if (method == SGP_PRED_VI && !gaussian) {
    set_err("Error: VI not supported for non-gaussian data.");   // predict_gp, l.424-427
    return SGP_EINVAL;
  }
  return SGP_OK;
}

// One batch.  dev: x_pred, mu_pred, pred_mean, pred_var are device pointers and the work runs on
// `s`; else host pointers, staged chunk by chunk on the predictor's stream.  box_lo / box_hi (d
// host values each, or NULL: host buffers -> the column range of x_pred, device buffers -> the
// builder's exact-difference form).  chunk_rows = 0 and route = 0: the product's.  sc: score the
// assembled vectors on the device (host buffers only).
int pred_run(sgp_predictor* p, int64_t chunk_rows, int route, const double* x_pred, int64_t np,
             int64_t ldxp, const double* mu_pred, double* pred_mean, double* pred_var, bool dev,
             const double* box_lo, const double* box_hi, hipStream_t s, const PredScore* sc,
             double* stage_ms) {
  if (!p) {
    set_err("sgp_predictor: the predictor is NULL");
    return SGP_EINVAL;
  }
  if (!x_pred || np < 1 || ldxp < np || !mu_pred || !pred_mean || !pred_var) {
    set_err("invalid sgp_predictor_run arguments");
    return SGP_EINVAL;
  }
  if (chunk_rows < 0 || chunk_rows % SGP_TILE) {
    set_err("sgp_predictor: chunk_rows=%lld is not a non-negative multiple of %d",
            (long long)chunk_rows, SGP_TILE);
    return SGP_EINVAL;
  }
  if (route < 0 || route > 3) {
    set_err("sgp_predictor: route=%d outside [0, 3]", route);
    return SGP_EINVAL;
  }
  if (route == 3 && p->m > SGP_EGO_TMAX) {
    set_err("sgp_predictor: the register route takes at most %d knots (m=%lld)", SGP_EGO_TMAX,
            (long long)p->m);
    return SGP_EINVAL;
  }
  if (route == 0) route = p->m <= SGP_PRED_M0 ? 3 : 1;
  const int d = p->d;
  const int64_t m = p->m, mp = p->mp;
  KernParams kp = p->kp;
  if (!dev) {
    std::vector<double> plo, phi;
    col_range(x_pred, np, ldxp, d, &plo, &phi);
    set_center(&kp, p->hU.data(), m, m, plo.data(), phi.data());
  } else {
    set_center(&kp, p->hU.data(), m, m, box_lo && box_hi ? box_lo : nullptr,
               box_lo && box_hi ? box_hi : nullptr);
    if (!(box_lo && box_hi)) kp.span2 = INFINITY;
  }
  HIPCHK(hipSetDevice(p->device));
  int64_t rows_max = 0, nchunks = 0;
  if (chunk_rows > 0) {
    rows_max = std::min(chunk_rows, round_up(np, SGP_TILE));
    nchunks = (np + rows_max - 1) / rows_max;
  } else {
    pred_plan(m, np, SGP_PRED_BUDGET, &rows_max, &nchunks);
  }
  int st = pred_ensure(p, rows_max);
  if (st) return st;
  const int64_t cap = p->cap;
  // scoring: the np-vectors assembled on the device (k_nlp_final's partial order spans all tiles)
  DevBuf dpm, dpv, dy, de, dn, part, dst;
  int max_blocks = 0;
  if (sc) {
    if ((st = nlp_max_blocks(p->device, &max_blocks))) return st;
    st = dalloc(&dpm.p, np);
    st = st ? st : dalloc(&dpv.p, np);
    st = st ? st : dalloc(&dy.p, np);
    st = st ? st : dalloc(&dn.p, np);
    st = st ? st : dalloc(&part.p, nlp_part_doubles(np));
    st = st ? st : dalloc(&dst.p, 4);
    if (!st && sc->expo) st = dalloc(&de.p, np);
    if (st) return st;
  }
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  struct EvGuard {
    hipEvent_t* e;
    ~EvGuard() { for (int k = 0; k < 5; ++k) if (e[k]) (void)hipEventDestroy(e[k]); }
  } evg{ev};
  if (stage_ms) {
    for (int k = 0; k < 4; ++k) stage_ms[k] = 0.0;
    for (int k = 0; k < 5; ++k) HIPCHK(hipEventCreate(&ev[k]));
  }
  for (int64_t r0 = 0; r0 < np; r0 += rows_max) {
    const int64_t rows = std::min(rows_max, np - r0), n_pad = round_up(rows, SGP_TILE);
    const size_t rb = sizeof(double) * (size_t)rows;
    if (stage_ms) HIPCHK(hipEventRecord(ev[0], s));
    HIPCHK(hipMemcpy2DAsync(p->Xc, sizeof(double) * cap, x_pred + r0, sizeof(double) * ldxp, rb,
                            (size_t)d, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    const double* mu = mu_pred + r0;
    double *pm = pred_mean + r0, *pv = pred_var + r0;
    if (!dev) {
      HIPCHK(hipMemcpyAsync(p->mu, mu_pred + r0, rb, hipMemcpyHostToDevice, s));
      mu = p->mu;
      pm = sc ? dpm.p + r0 : p->pm;
      pv = sc ? dpv.p + r0 : p->pv;
    }
    if (stage_ms) HIPCHK(hipEventRecord(ev[1], s));
    if (route != 3)
      HIPCHK(launch_build_knm(kp, p->Xc, cap, rows, n_pad, p->dU, mp, m, mp, p->K, s));
    if (stage_ms) HIPCHK(hipEventRecord(ev[2], s));
    if (route == 1) {
      HIPCHK(launch_pred_tiles(p->K, p->Ap, p->w, rows, n_pad, cap, mp, mu, p->c0, p->qslab,
                               p->yslab, pm, pv, s));
    } else if (route == 2) {   // sgp_predict's arithmetic on the chunk
      double *yv = p->yslab, *q = p->yslab + cap;
      HIPCHK(launch_gemv_rows(p->K, n_pad, mp, p->w, nullptr, yv, nullptr, s));
      HIPCHK(launch_rowquad_knm(kp, p->K, p->T22, rows, n_pad, m, mp, nullptr, 0.0, nullptr,
                                nullptr, nullptr, p->qslab, q, s));
      HIPCHK(launch_pred_finish(mu, yv, q, p->c0, rows, pm, pv, s));
    } else {   // k_fit_scan's pass over the chunk: K in registers, var = c0 - k^T (-S) k
      FitScan a;
      a.X = p->Xc;
      a.ldx = cap;
      a.n = rows;
      a.d = d;
      a.m = (int)m;
      a.mode = SGP_SCAN_VAR;
      a.coef = kp.coef;
      a.sig2 = kp.sig2;
      a.c0 = p->c0;
      a.rl = p->rl;
      a.mu = mu;
      a.f = nullptr;
      a.xu = p->dU;
      a.A = p->negA;
      a.w = p->w;
      a.ex = nullptr;
      a.E = 0;
      a.key_out = nullptr;
      a.mean_out = pm;
      a.var_out = pv;
      a.rec = p->scan_rec;
      HIPCHK(launch_fit_scan(a, p->max_blocks, p->status, p->scan_rec + 2 * p->max_blocks, s));
    }
    if (stage_ms) HIPCHK(hipEventRecord(ev[3], s));
    if (!dev && !sc) {
      HIPCHK(hipMemcpyAsync(pred_mean + r0, p->pm, rb, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(pred_var + r0, p->pv, rb, hipMemcpyDeviceToHost, s));
    }
    if (stage_ms) {
      HIPCHK(hipEventRecord(ev[4], s));
      HIPCHK(hipStreamSynchronize(s));
      for (int k = 0; k < 4; ++k) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        stage_ms[k] += (double)ms;
      }
    }
    // (the next chunk reuses the work space in stream order: no host wait between chunks)
  }
  if (sc) {
    const size_t nb = sizeof(double) * (size_t)np;
    HIPCHK(hipMemcpyAsync(dy.p, sc->y, nb, hipMemcpyHostToDevice, s));
    if (sc->expo) HIPCHK(hipMemcpyAsync(de.p, sc->expo, nb, hipMemcpyHostToDevice, s));
    NlpArgs a{dy.p, dpm.p, dpv.p, sc->expo ? de.p : nullptr, sc->par, np, dn.p, part.p};
    HIPCHK(launch_nlp_rows(sc->family, a, max_blocks, dst.p, s));
    HIPCHK(hipMemcpyAsync(pred_mean, dpm.p, nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pred_var, dpv.p, nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sc->nlp, dn.p, nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sc->stats, dst.p, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
  }
  if (!dev) HIPCHK(hipStreamSynchronize(s));
  return SGP_OK;
}
}  // namespace

int sgp_diag_predictor_args(int d, int kernel, const double* theta, double delta, int method,
                            int gaussian, const double* U, int64_t m, int64_t ldu,
                            const double* u_mean, const double* muu, const double* u_var,
                            int64_t ldv) {
  return pred_check_args(d, kernel, theta, delta, method, gaussian, U, m, ldu, u_mean, muu, u_var,
                         ldv);
}

int sgp_diag_predictor_plan(int64_t m, int d, int64_t np, int64_t budget_bytes,
                            int64_t* chunk_rows, int64_t* nchunks, int64_t* block_products_sym,
                            int64_t* block_products_full) {
  if (m < 1 || d < 1 || d > SGP_MAXD || np < 1 || budget_bytes < 0 || !chunk_rows || !nchunks ||
      !block_products_sym || !block_products_full) {
    set_err("sgp_diag_predictor_plan: invalid arguments");
    return SGP_EINVAL;
  }
  pred_plan(m, np, budget_bytes ? budget_bytes : SGP_PRED_BUDGET, chunk_rows, nchunks);
  const int64_t nb = round_up(m, SGP_TILE) / SGP_TILE;
  *block_products_sym = nb * (nb + 1) / 2;
  *block_products_full = nb * nb;
  return SGP_OK;
}

int sgp_predictor_create(sgp_predictor** out, int device, int kernel, const double* theta,
                         double delta, int method, int gaussian, const double* U, int64_t m,
                         int64_t ldu, int d, const double* u_mean, const double* muu,
                         const double* u_var, int64_t ldv) {
  if (!out) {
    set_err("sgp_predictor_create: out is NULL");
    return SGP_EINVAL;
  }
  *out = nullptr;
  int st = pred_check_args(d, kernel, theta, delta, method, gaussian, U, m, ldu, u_mean, muu,
                           u_var, ldv);
  if (st) return st;
  KernParams kp;
  if ((st = make_params(kernel, d, theta, delta, &kp))) return st;
  const bool lapfull = method == SGP_PRED_LAPLACE_FULL;
  const bool full = method == SGP_PRED_FULL || lapfull;
  HIPCHK(hipSetDevice(device));
  PredGuard g;
  sgp_predictor* p = g.p = new sgp_predictor;
  p->device = device;
  p->kp = kp;
  p->d = d;
  p->method = method;
  p->m = m;
  const int64_t mp = p->mp = round_up(m, SGP_TILE), mm = mp * mp;
  // vi_functions.R:1321: tau^2 + sigma^2 + delta; laplace_approx_prediction.R:114: sigma^2 + tau^2
  // predict_gp_full: diag(Sigma11) = sigma^2 + tau^2 + delta
  p->c0 = (method == SGP_PRED_VI) ? (kp.tau2 + kp.sig2) + delta
                                  : (full ? (kp.sig2 + kp.tau2) + delta : kp.sig2 + kp.tau2);
  p->hU.assign((size_t)(m * d), 0.0);
  for (int c = 0; c < d; ++c)
    for (int64_t j = 0; j < m; ++j) p->hU[(size_t)(c * m + j)] = U[j + c * ldu];
  int64_t nchunks = 0;
  pred_plan(m, INT64_MAX / 2, SGP_PRED_BUDGET, &p->chunk_rows, &nchunks);
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  p->max_blocks = std::min(4096, std::max(1, 8 * cus));
  HIPCHK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  hipStream_t s = p->stream;
  // the m x m stage of sgp_predict (predict_run), its temporaries freed when create returns
  DevBuf K22, Kinv, R, Pb, logd, V, T1, wv;
  IntBuf gsync;
  const bool reg = mp == SGP_EGO_TMAX;   // the register route's operands
  st = dalloc(&p->dU, mp * d);
  st = st ? st : dalloc(&p->w, mp);
  st = st ? st : dalloc(&p->T22, mm);
  st = st ? st : dalloc(&p->Ap, mm);
  st = st ? st : dalloc(&p->status, 4);
  if (!st && reg) {
    st = dalloc(&p->negA, mm);
    st = st ? st : dalloc(&p->rl, SGP_MAXD);
    st = st ? st : dalloc(&p->scan_rec, 2 * p->max_blocks + 4);
  }
  st = st ? st : dalloc(&K22.p, mm);
  st = st ? st : dalloc(&Kinv.p, mm);
  st = st ? st : dalloc(&R.p, mm);
  st = st ? st : dalloc(&Pb.p, mp * 64);
  st = st ? st : dalloc(&logd.p, mp / SGP_DB);
  st = st ? st : dalloc(&V.p, mm);
  st = st ? st : dalloc(&T1.p, mm);
  st = st ? st : dalloc(&wv.p, 2 * mp);
  st = st ? st : dalloc(&gsync.p, SGP_GJ_SYNC_WORDS);
  if (st) return st;
  // (the host buffers outlive the copies: the stream is synchronised before they go)
  std::vector<double> hU((size_t)(mp * d), 0.0), hd((size_t)mp, 0.0), hg((size_t)mp, 0.0),
      hV((size_t)mm, 0.0), hrl((size_t)SGP_MAXD, 1.0);
  for (int c = 0; c < d; ++c)
    for (int64_t j = 0; j < m; ++j) hU[(size_t)(c * mp + j)] = U[j + c * ldu];
  for (int64_t j = 0; j < m; ++j) {
    hd[(size_t)j] = lapfull ? sqrt(-muu[j]) : u_mean[j] - muu[j];   // lapfull: sqrt(-W)
    hg[(size_t)j] = u_mean[j];
  }
  if (!full)
    for (int64_t i = 0; i < m; ++i)
      for (int64_t j = 0; j < m; ++j) hV[(size_t)(i * mp + j)] = u_var[i + j * ldv];
  if (kernel == SGP_KERNEL_ARD)
    for (int q = 0; q < d; ++q) hrl[(size_t)q] = kp.rl[q];
  const size_t mb = sizeof(double) * (size_t)mp;
  HIPCHK(hipMemcpyAsync(p->dU, hU.data(), sizeof(double) * hU.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(wv.p + mp, hd.data(), mb, hipMemcpyHostToDevice, s));
  if (lapfull) HIPCHK(hipMemcpyAsync(p->w, hg.data(), mb, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(V.p, hV.data(), sizeof(double) * mm, hipMemcpyHostToDevice, s));
  if (reg)
    HIPCHK(hipMemcpyAsync(p->rl, hrl.data(), sizeof(double) * SGP_MAXD, hipMemcpyHostToDevice, s));
  // on the launch stream: the null stream's hipMemset is not ordered before a non-blocking
  // stream's kernels (the chain's sync words must be zero when it starts)
  HIPCHK(hipMemsetAsync(p->status, 0, sizeof(int) * 4, s));
  HIPCHK(hipMemsetAsync(gsync.p, 0, sizeof(int) * SGP_GJ_SYNC_WORDS, s));
  // Sigma22: the gaussian family subtracts tau^2 I again (vi_functions.R:1246-1260,
  // laplace_approx_prediction.R:25-43) -> diagonal sigma^2 + delta; otherwise Kuu+(tau^2+delta)I
  // (predict_gp_full, laplace_approx_prediction.R:281-405: Sigma22 = k(xy, xy) + (tau^2+delta) I)
  const double diag_sub = (gaussian && !full) ? kp.tau2 : 0.0;
  HIPCHK(launch_build_kmm(kp, p->dU, mp, m, mp, diag_sub, K22.p, s));
  if (lapfull) {
    // temp22 = -R, R = sW (I + sW Sigma sW)^-1 sW (laplace_approx_prediction.R:169, 188, 206);
    // the mean's multiplier grad_log_py_ff is in w already (l.209)
    HIPCHK(launch_flap_scale(true, K22.p, wv.p + mp, Kinv.p, mp, m, s));
    HIPCHK(dense_spd_inverse(Kinv.p, mp, R.p, Pb.p, logd.p, p->status,
                             reinterpret_cast<unsigned*>(gsync.p), s));
    HIPCHK(launch_flap_scale(false, Kinv.p, wv.p + mp, Kinv.p, mp, m, s));
    HIPCHK(dense_axpby(0.0, V.p, -1.0, Kinv.p, p->T22, mm, s));   // V holds zeros
  } else {
    HIPCHK(hipMemcpyAsync(Kinv.p, K22.p, sizeof(double) * mm, hipMemcpyDeviceToDevice, s));
    HIPCHK(dense_spd_inverse(Kinv.p, mp, R.p, Pb.p, logd.p, p->status,
                             reinterpret_cast<unsigned*>(gsync.p), s));
    HIPCHK(dense_gemv(Kinv.p, mp, wv.p + mp, 1.0, p->w, s));        // Sigma22^-1 (u_mean - muu)
    HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, Kinv.p, mp, V.p, mp, 0.0, T1.p, mp,
                         s));
    HIPCHK(launch_gemm64(false, false, false, mp, mp, mp, 1.0, T1.p, mp, Kinv.p, mp, 0.0, p->T22,
                         mp, s));                                     // Sigma22^-1 u_var Sigma22^-1
    HIPCHK(dense_axpby(1.0, p->T22, -1.0, Kinv.p, p->T22, mm, s));   // temp22
  }
  HIPCHK(launch_pred_sym(p->T22, mp, p->Ap, s));
  if (reg) HIPCHK(dense_axpby(0.0, p->Ap, -1.0, p->Ap, p->negA, mm, s));   // one block: A' = S
  int hst[4];
  HIPCHK(hipMemcpyAsync(hst, p->status, sizeof(hst), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (hst[0]) {
    set_err("%s is not positive definite (leading minor of order %d)",
            lapfull ? "I + sqrt(-W) %*% Sigma %*% sqrt(-W)" : "Sigma22", hst[0]);
    return SGP_ENOTPD;
  }
  g.p = nullptr;
  *out = p;
  return SGP_OK;
}

int sgp_predictor_destroy(sgp_predictor* p) {
  if (!p) {
    set_err("sgp_predictor_destroy: the predictor is NULL");
    return SGP_EINVAL;
  }
  pred_free(p);
  return SGP_OK;
}

int sgp_predictor_run(sgp_predictor* p, const double* x_pred, int64_t np, int64_t ldxp,
                      const double* mu_pred, double* pred_mean, double* pred_var) {
  return pred_run(p, 0, 0, x_pred, np, ldxp, mu_pred, pred_mean, pred_var, false, nullptr,
                  nullptr, p ? p->stream : nullptr, nullptr, nullptr);
}

int sgp_predictor_run_nlp(sgp_predictor* p, const double* x_pred, int64_t np, int64_t ldxp,
                          const double* mu_pred, double* pred_mean, double* pred_var, int family,
                          const double* y_pred, double par, const double* expo, double* nlp,
                          double* stats) {
  if (!p) {
    set_err("sgp_predictor_run_nlp: the predictor is NULL");
    return SGP_EINVAL;
  }
  int st = nlp_check_args("sgp_predictor_run_nlp", family, y_pred, np, par, expo, nlp, stats);
  if (st) return st;
  PredScore sc{family, y_pred, par, expo, nlp, stats};
  return pred_run(p, 0, 0, x_pred, np, ldxp, mu_pred, pred_mean, pred_var, false, nullptr,
                  nullptr, p->stream, &sc, nullptr);
}

int sgp_predictor_run_dev(sgp_predictor* p, const double* x_pred, int64_t np, int64_t ldxp,
                          const double* mu_pred, double* pred_mean, double* pred_var,
                          const double* box_lo, const double* box_hi, void* stream) {
  return pred_run(p, 0, 0, x_pred, np, ldxp, mu_pred, pred_mean, pred_var, true, box_lo, box_hi,
                  static_cast<hipStream_t>(stream), nullptr, nullptr);
}

int sgp_diag_predictor_run(sgp_predictor* p, int64_t chunk_rows, int route, const double* x_pred,
                           int64_t np, int64_t ldxp, const double* mu_pred, double* pred_mean,
                           double* pred_var, double* stage_ms) {
  return pred_run(p, chunk_rows, route, x_pred, np, ldxp, mu_pred, pred_mean, pred_var, false,
                  nullptr, nullptr, p ? p->stream : nullptr, nullptr, stage_ms);
}


// ------------------------------------------------------------------------- OAT candidates
// ELBO of the knot sets [U; x*_t] for T candidate knots at fixed theta, as the meta-model
// y values of knot_prop_random_norm_vi / knot_prop_ego_norm_vi (R/vi_functions.R:2196-2300)
// compute them -- but without rebuilding K12 per candidate: a candidate borders K22, S and
// Bm by one row/column, so its ELBO follows from the base evaluation plus Schur complements
// (DESIGN.md sec. 3.5).  Work per 128 candidates: one K(X, x*) build and one n x m x 128 TN
// GEMM (K^T Kc) instead of 128 SYRKs.
int sgp_vi_candidates(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
                      int64_t ldu, double delta, unsigned flags, const double* cand, int64_t T,
                      int64_t ldc, double* obj_out) {
  MULTI_FWD(c, U && cand && T >= 1 && ldc >= T && obj_out && m >= 1 && ldu >= m ? multi_vi_candidates(c->multi, kernel, theta, U, m, ldu, delta, flags, cand, T, ldc, obj_out) : multi_bad_args());
  if (!c || !cand || T < 1 || ldc < T || !obj_out) {
    set_err("invalid sgp_vi_candidates arguments");
    return SGP_EINVAL;
  }
  int st = sgp_vi_phase1(c, kernel, theta, U, m, ldu, delta, c->red1);
  if (st) return st;
  const KernParams& kp = c->kp;
  const int64_t mp = c->mp, mm = mp * mp, n_pad = c->n_pad, d = kp.d;
  const double z = kp.tau2 + delta;
  const double* S = c->red1;
  const int64_t toff = vi_red1_toff(c, mp);
  const double* t = c->red1 + toff;
  if (c->pack_red1) {
    HIPCHK(launch_unpack_lower64(c->red1, mp, c->Sfull, c->stream));
    S = c->Sfull;
  }
  // K22's inverse was queued on aux by sgp_vi_phase1; it runs beside Bm's
  st = bm_stage(c, S, 1.0 / z, c->vi_k22_ordered);   // as sgp_vi_phase2
  if (st) return st;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_k22, 0));
  {
    Scope tm(c, "mm_vectors");
    HIPCHK(dense_gemv(c->Binv, mp, t, 1.0 / z, c->uvec, c->stream));
    HIPCHK(launch_dot(t, c->uvec, mp, c->slab_small, c->sc + SC_TU, c->stream));
    HIPCHK(launch_dot(c->K22inv, S, mm, c->slab_small, c->sc + SC_TRKS, c->stream));
    HIPCHK(hipMemcpyAsync(c->sc + SC_RR, c->red1 + toff + mp, sizeof(double),
                          hipMemcpyDeviceToDevice, c->stream));
  }
  // the candidate builds' parameters: phase 1's (same centre), with the accuracy guard's span
  // widened to the candidates, which may lie outside the data box (knot bounds, Q9)
  KernParams kpc = kp;
  set_center(&kpc, U, m, ldu, c->xmin.data(), c->xmax.data(), cand, T, ldc);
  constexpr int64_t TP = 128;
  DevBuf Kc, slab, P, part, rk, cc, Uc, K22c, W, SW, Bt, BB, base, out;
  const int64_t slab_cap = gemm_tn_slab_doubles(n_pad, mp, TP);
  const int64_t part_cap = lap_gemv_cols_slab(n_pad, TP, 1);
  st = dalloc(&Kc.p, n_pad * TP);
  st = st ? st : dalloc(&slab.p, slab_cap);
  st = st ? st : dalloc(&P.p, mp * TP);
  st = st ? st : dalloc(&part.p, part_cap);
  st = st ? st : dalloc(&rk.p, TP);
  st = st ? st : dalloc(&cc.p, TP);
  st = st ? st : dalloc(&Uc.p, TP * d);
  st = st ? st : dalloc(&K22c.p, mp * TP);
  st = st ? st : dalloc(&W.p, mp * TP);
  st = st ? st : dalloc(&SW.p, mp * TP);
  st = st ? st : dalloc(&Bt.p, mp * TP);
  st = st ? st : dalloc(&BB.p, mp * TP);
  st = st ? st : dalloc(&base.p, 2);
  st = st ? st : dalloc(&out.p, TP * 4);
  if (st) return st;
  // Sigma22' diagonal entry of the new knot: make_cov (sigma^2 + tau^2 + delta) - tau^2
  const double kxx = ((kp.sig2 + kp.tau2) + delta) - kp.tau2;
  const double hb[2] = {kxx, z};
  HIPCHK(hipMemcpyAsync(base.p, hb, sizeof(hb), hipMemcpyHostToDevice, c->stream));
  double sc[SC_N];
  int status[4];
  HIPCHK(hipMemcpyAsync(sc, c->sc, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(status, c->status, sizeof(status), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->phase = 0;
  if (chain_watchdog(status)) return SGP_EHIP;
  if (status[0] || status[1]) {
    set_err("chol(): the leading minor of order %d of %s is not positive definite",
            status[0] ? status[0] : status[1],
            status[0] ? "Sigma22" : "Sigma22 + t(Sigma12) %*% ZSig12");
    return SGP_ENOTPD;
  }
  const double n = (double)c->n;
  const double ld22 = 2.0 * sc[SC_LD22], ldB = 2.0 * sc[SC_LDB];
  const double quad = -0.5 * sc[SC_RR] / z + 0.5 * sc[SC_TU] / z;   // u = Bm^-1 t / z
  const double trKS = sc[SC_TRKS];
  std::vector<double> hU((size_t)(TP * d)), ho((size_t)(TP * 4));
  for (int64_t t0 = 0; t0 < T; t0 += TP) {
    const int64_t tc = (T - t0 < TP) ? T - t0 : TP;
    std::fill(hU.begin(), hU.end(), 0.0);
    for (int q = 0; q < d; ++q)
      for (int64_t j = 0; j < tc; ++j) hU[(size_t)(q * TP + j)] = cand[(t0 + j) + q * ldc];
    HIPCHK(hipMemcpyAsync(Uc.p, hU.data(), sizeof(double) * hU.size(), hipMemcpyHostToDevice,
                          c->stream));
    Scope tm(c, "candidates");
    HIPCHK(launch_build_knm(kpc, c->X, n_pad, c->n, n_pad, Uc.p, TP, tc, TP, Kc.p, c->stream));
    HIPCHK(launch_gemm_tn(c->K, mp, mp, Kc.p, TP, TP, n_pad, slab.p, slab_cap, P.p, c->stream));
    HIPCHK(launch_gemv_cols(Kc.p, n_pad, TP, c->r, n_pad, 1, part.p, part_cap, rk.p, c->stream));
    HIPCHK(launch_colnorm2(Kc.p, n_pad, TP, part.p, part_cap, cc.p, c->stream));
    HIPCHK(launch_build_knm(kpc, c->U, mp, m, mp, Uc.p, TP, tc, TP, K22c.p, c->stream));
    HIPCHK(launch_gemm64(false, false, false, mp, TP, mp, 1.0, c->K22inv, mp, K22c.p, TP, 0.0,
                         W.p, TP, c->stream));
    HIPCHK(launch_gemm64(false, false, false, mp, TP, mp, 1.0, S, mp, W.p, TP, 0.0, SW.p, TP,
                         c->stream));
    HIPCHK(dense_axpby(1.0, K22c.p, 1.0 / z, P.p, Bt.p, mp * TP, c->stream));
    HIPCHK(launch_gemm64(false, false, false, mp, TP, mp, 1.0, c->Binv, mp, Bt.p, TP, 0.0, BB.p,
                         TP, c->stream));
    HIPCHK(launch_vi_cand_scalars(m, mp, tc, TP, K22c.p, W.p, SW.p, P.p, Bt.p, BB.p, c->uvec,
                                  rk.p, cc.p, base.p, out.p, c->stream));
    HIPCHK(hipMemcpyAsync(ho.data(), out.p, sizeof(double) * tc * 4, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int64_t j = 0; j < tc; ++j) {
      const double sK = ho[(size_t)(j * 4)], sB = ho[(size_t)(j * 4 + 1)];
      const double dq = ho[(size_t)(j * 4 + 2)], trinc = ho[(size_t)(j * 4 + 3)];
      if (!(sK > 0.0) || !(sB > 0.0)) {   // the reference's chol() would fail (try-error)
        obj_out[t0 + j] = NAN;
        continue;
      }
      const double ld22c = ld22 + log(sK), ldBc = ldB + log(sB);
      const double logdet22 = (flags & SGP_FLAG_R_DET) ? log(exp(ld22c)) : ld22c;
      const double qd = quad + 0.5 * dq * dq / (z * z * sB);
      const double det_part = -0.5 * (n * log(z) - logdet22 + ldBc);
      const double tt = -(1.0 / (2.0 * kp.tau2)) * (n * (kp.sig2 + delta) - (trKS + trinc / sK));
      obj_out[t0 + j] = qd + det_part - (n / 2.0) * log(2.0 * M_PI) + tt;
    }
  }
  // as the FITC and Laplace scorers: phase 1 above forgot the evaluation before this call, and
  // the base state it left (no phase 2, no finish) is no completed evaluation either
  forget_posterior(c);
  return SGP_OK;
}

// [U; cand_t] (m + 1) x d column-major on the host
static void bordered_knots(const double* U, int64_t m, int64_t ldu, int d, const double* cand,
                           int64_t t, int64_t ldc, std::vector<double>& Ub) {
  Ub.resize((size_t)((m + 1) * d));
  for (int q = 0; q < d; ++q) {
    for (int64_t k = 0; k < m; ++k) Ub[(size_t)(k + q * (m + 1))] = U[k + q * ldu];
    Ub[(size_t)(m + q * (m + 1))] = cand[t + q * ldc];
  }
}

// FITC meta-model values (knot_proposal_functions.R:1292-1319 per candidate): obj_fun_norm at
// [U; cand_t].  Each candidate changes Z for every row, so unlike VI there is no bordered
// shortcut for the weighted Gram matrix; each one is an objective-only FITC evaluation
// (builder, row-quadratic, SYRK, m x m inverse) on the resident rows.
int sgp_fitc_candidates(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
                        int64_t ldu, double delta, unsigned flags, const double* cand, int64_t T,
                        int64_t ldc, double* obj_out) {
  MULTI_FWD(c, U && cand && T >= 1 && ldc >= T && obj_out && m >= 1 && ldu >= m ? multi_fitc_candidates(c->multi, kernel, theta, U, m, ldu, delta, flags, cand, T, ldc, obj_out) : multi_bad_args());
  if (!c || !U || !cand || T < 1 || ldc < T || !obj_out || m < 1 || ldu < m) {
    set_err("invalid sgp_fitc_candidates arguments");
    return SGP_EINVAL;
  }
  if (m + 1 > c->m_max) {
    set_err("m + 1 = %lld knots exceed the context's m_max = %lld", (long long)(m + 1),
            (long long)c->m_max);
    return SGP_EINVAL;
  }
  std::vector<double> Ub;
  for (int64_t t = 0; t < T; ++t) {
    bordered_knots(U, m, ldu, c->d, cand, t, ldc, Ub);
    double o = 0.0;
    int st = sgp_eval_fitc(c, kernel, theta, Ub.data(), m + 1, m + 1, delta,
                           flags | SGP_FLAG_OBJ_ONLY, &o, nullptr);
    if (st == SGP_ENOTPD) {   // the reference's try-error
      obj_out[t] = NAN;
      continue;
    }
    if (st) return st;
    obj_out[t] = o;
  }
  forget_posterior(c);   // the context's posterior state belongs to the last candidate
  return SGP_OK;
}

// Laplace meta-model values (knot_proposal_functions.R:1116-1160 per candidate): the last NR
// objective value of newtrap_sparseGP at [U; cand_t], started from the same f every time.
int sgp_lap_candidates(sgp_ctx* c, int kernel, const double* theta, const double* U, int64_t m,
                       int64_t ldu, double delta, double expo, double tol, int maxit,
                       const double* cand, int64_t T, int64_t ldc, double* obj_out) {
  MULTI_FWD(c, U && cand && T >= 1 && ldc >= T && obj_out && m >= 1 && ldu >= m ? multi_lap_candidates(c->multi, kernel, theta, U, m, ldu, delta, expo, tol, maxit, cand, T, ldc, obj_out) : multi_bad_args());
  if (!c || !U || !cand || T < 1 || ldc < T || !obj_out || m < 1 || ldu < m) {
    set_err("invalid sgp_lap_candidates arguments");
    return SGP_EINVAL;
  }
  if (m + 1 > c->m_max) {
    set_err("m + 1 = %lld knots exceed the context's m_max = %lld", (long long)(m + 1),
            (long long)c->m_max);
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(c->device));
  int st = lap_ensure(c);
  if (st) return st;
  DevBuf f0;
  st = dalloc(&f0.p, c->n_pad);
  if (st) return st;
  HIPCHK(hipMemcpyAsync(f0.p, lvec(c, LV_F), sizeof(double) * c->n_pad, hipMemcpyDeviceToDevice,
                        c->stream));
  std::vector<double> Ub;
  for (int64_t t = 0; t < T && st == SGP_OK; ++t) {
    bordered_knots(U, m, ldu, c->d, cand, t, ldc, Ub);
    if (t > 0)
      HIPCHK(hipMemcpyAsync(lvec(c, LV_F), f0.p, sizeof(double) * c->n_pad,
                            hipMemcpyDeviceToDevice, c->stream));
    double o = 0.0;
    int it = 0;
    st = sgp_lap_nr(c, kernel, theta, Ub.data(), m + 1, m + 1, delta, expo, tol, maxit, &o, &it);
    if (st == SGP_ENOTPD) {
      obj_out[t] = NAN;
      st = SGP_OK;
      continue;
    }
    if (st == SGP_OK) obj_out[t] = o;
  }
  HIPCHK(hipMemcpyAsync(lvec(c, LV_F), f0.p, sizeof(double) * c->n_pad, hipMemcpyDeviceToDevice,
                        c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  forget_posterior(c);   // the context's posterior state belongs to the last candidate
  c->lap_gpsi_valid = false;
  return st;
}

// ------------------------------------------------------------------------- diagnostics
// (include/sgp_diag.h)

int sgp_diag_gj_pair(int device, int64_t m, const double* A, const double* B, double beta,
                     int per_step, double* invA, double* invS, double* logdet) {
  if (m < 1 || m > 16384 || !A || !B || !invA || !invS || !logdet ||
      !(beta == beta) || (per_step != 0 && per_step != 1)) {
    set_err("invalid sgp_diag_gj_pair arguments (m=%lld, per_step=%d)", (long long)m, per_step);
    return SGP_EINVAL;
  }
  const int64_t mp = round_up(m, SGP_TILE), mm = mp * mp, nb = mp / SGP_DB;
  if (!per_step && nb > 64) {
    set_err("sgp_diag_gj_pair: the persistent chain takes m <= 4096 (m = %lld)", (long long)m);
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  StreamGuard s_main, s_aux;
  HIPCHK(hipStreamCreateWithFlags(&s_main.s, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&s_aux.s, hipStreamNonBlocking));
  DevBuf dA, dB, dInvA, dInvS, R1, R2, P1, P2, L1, L2;
  IntBuf status, sync;
  int st = dalloc(&dA.p, mm);
  st = st ? st : dalloc(&dB.p, mm);
  st = st ? st : dalloc(&dInvA.p, mm);
  st = st ? st : dalloc(&dInvS.p, mm);
  st = st ? st : dalloc(&R1.p, mm);
  st = st ? st : dalloc(&R2.p, mm);
  st = st ? st : dalloc(&P1.p, mp * 64);
  st = st ? st : dalloc(&P2.p, mp * 64);
  st = st ? st : dalloc(&L1.p, nb);
  st = st ? st : dalloc(&L2.p, nb);
  st = st ? st : dalloc(&status.p, 4);
  st = st ? st : dalloc(&sync.p, 2 * SGP_GJ_SYNC_WORDS);
  if (st) return st;
  // row-major padded as the contexts hold them: A padded with the identity, B with zeros
  std::vector<double> hA((size_t)mm, 0.0), hB((size_t)mm, 0.0);
  for (int64_t i = 0; i < mp; ++i)
    for (int64_t j = 0; j < mp; ++j) {
      const bool in = i < m && j < m;
      hA[(size_t)(i * mp + j)] = in ? A[i + j * m] : (i == j ? 1.0 : 0.0);
      hB[(size_t)(i * mp + j)] = in ? B[i + j * m] : 0.0;
    }
  HIPCHK(hipMemcpy(dA.p, hA.data(), sizeof(double) * mm, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dB.p, hB.data(), sizeof(double) * mm, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dInvA.p, hA.data(), sizeof(double) * mm, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(status.p, 0, sizeof(int) * 4));
  HIPCHK(hipMemset(sync.p, 0, sizeof(int) * 2 * SGP_GJ_SYNC_WORDS));
  // hipMemset runs on the null stream, which non-blocking streams do not wait for: the chains'
  // sync words must be zero before either chain starts
  HIPCHK(hipDeviceSynchronize());
  unsigned* sy = reinterpret_cast<unsigned*>(sync.p);
  // both chains in flight together, as VI's phase 2 issues them
  HIPCHK(dense_spd_inverse_chain(dInvA.p, mp, R1.p, P1.p, L1.p, status.p, sy + SGP_GJ_SYNC_WORDS,
                                 s_aux.s, per_step != 0));
  HIPCHK(dense_spd_inverse_sum_chain(dA.p, beta, dB.p, dInvS.p, mp, R2.p, P2.p, L2.p,
                                     status.p + 1, sy, s_main.s, per_step != 0));
  HIPCHK(hipStreamSynchronize(s_aux.s));
  HIPCHK(hipStreamSynchronize(s_main.s));
  int hs[4];
  std::vector<double> ld1((size_t)nb), ld2((size_t)nb);
  HIPCHK(hipMemcpy(hs, status.p, sizeof(hs), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ld1.data(), L1.p, sizeof(double) * nb, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ld2.data(), L2.p, sizeof(double) * nb, hipMemcpyDeviceToHost));
  if (chain_watchdog(hs)) return SGP_EHIP;
  if (hs[0] || hs[1]) {
    set_err("chol(): the leading minor of order %d of %s is not positive definite",
            hs[0] ? hs[0] : hs[1], hs[0] ? "A" : "A + beta B");
    return SGP_ENOTPD;
  }
  HIPCHK(hipMemcpy(hA.data(), dInvA.p, sizeof(double) * mm, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hB.data(), dInvS.p, sizeof(double) * mm, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < m; ++i)
    for (int64_t j = 0; j < m; ++j) {
      invA[i + j * m] = hA[(size_t)(i * mp + j)];
      invS[i + j * m] = hB[(size_t)(i * mp + j)];
    }
  // block log-determinant halves summed in block order (the evaluations' order)
  double a = 0.0, b = 0.0;
  for (int64_t k = 0; k < nb; ++k) {
    a += ld1[(size_t)k];
    b += ld2[(size_t)k];
  }
  logdet[0] = 2.0 * a;
  logdet[1] = 2.0 * b;
  return SGP_OK;
}

namespace {
typedef double sgp_d2 __attribute__((ext_vector_type(2)));
// pattern 0: one linear stream, 16 B per lane per instruction
__global__ void __launch_bounds__(256) k_diag_store_lin(sgp_d2* __restrict__ p, int64_t n2,
                                                        double v) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256)
    __builtin_nontemporal_store(sgp_d2{v, v}, &p[i]);
}
// pattern 1: the K12 builder's store shape -- per wave instruction 4 rows x 256 B of a
// row-major matrix with mp = 1024 doubles per row; a workgroup owns 128 columns and walks 64-row
// blocks
__global__ void __launch_bounds__(256) k_diag_store_tile(double* __restrict__ K, int64_t nrb,
                                                         int64_t mp, double v) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, ln = lane & 15, lq = lane >> 4;
  const int64_t j0 = (int64_t)blockIdx.x * 128;
  for (int64_t rb = blockIdx.y; rb < nrb; rb += gridDim.y) {
    const int64_t ib = rb * 64 + 16 * w;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = ib + lq + 4 * r;
        __builtin_nontemporal_store(sgp_d2{v, v},
                                    reinterpret_cast<sgp_d2*>(&K[i * mp + j0 + 32 * p + 2 * ln]));
      }
  }
}
}  // namespace

int sgp_diag_store_bw(int device, int64_t bytes, int reps, int pattern, double* gbs) {
  if (!gbs || bytes < (int64_t)(1 << 20) || reps < 1 || (pattern != 0 && pattern != 1)) {
    set_err("invalid sgp_diag_store_bw arguments");
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  const int64_t mp = 1024;
  const int64_t nrb = bytes / (64 * mp * 8);
  if (nrb < 1) { set_err("sgp_diag_store_bw: bytes < one 64-row block"); return SGP_EINVAL; }
  const int64_t used = nrb * 64 * mp * 8;
  DevBuf buf;
  int st = dalloc(&buf.p, used / 8);
  if (st) return st;
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  double best = 0.0;
  hipError_t err = hipSuccess;
  for (int r = 0; r <= reps && err == hipSuccess; ++r) {   // pass 0 warms up
    err = hipEventRecord(e0, sg.s);
    if (pattern == 0)
      hipLaunchKernelGGL(k_diag_store_lin, dim3((unsigned)(cus * 16)), dim3(256), 0, sg.s,
                         reinterpret_cast<sgp_d2*>(buf.p), used / 16, (double)r);
    else
      hipLaunchKernelGGL(k_diag_store_tile, dim3((unsigned)(mp / 128), (unsigned)(cus * 2)),
                         dim3(256), 0, sg.s, buf.p, nrb, mp, (double)r);
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipEventRecord(e1, sg.s);
    if (err == hipSuccess) err = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    if (err == hipSuccess && r > 0 && ms > 0.0f) best = std::max(best, (double)used / (ms * 1e6));
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  HIPCHK(err);
  *gbs = best;
  return SGP_OK;
}

int sgp_diag_syrk_plan(int64_t n, int64_t m, int* plan, int* workgroups, double* t_balanced,
                       double* t_packed) {
  if (n < 1 || m < 1 || !plan || !workgroups || !t_balanced || !t_packed) {
    set_err("invalid sgp_diag_syrk_plan arguments");
    return SGP_EINVAL;
  }
  syrk_plan_info(round_up(n, SGP_TILE), round_up(m, SGP_TILE), plan, workgroups, t_balanced,
                 t_packed);
  return SGP_OK;
}

int sgp_diag_exp(int device, int which, const double* x, int64_t n, double hi, double* out) {
  if (!x || !out || n < 1) {
    set_err("sgp_diag_exp: NULL argument or n < 1");
    return SGP_EINVAL;
  }
  if (which != 0 && which != 1) {
    set_err("sgp_diag_exp: which=%d is neither 0 (sgp_exp_nonpos) nor 1 (sgp_exp_tab)", which);
    return SGP_EINVAL;
  }
  if (which == 1 && !(hi <= 709.782712893384)) {
    set_err("sgp_diag_exp: hi=%g is NaN or above log(DBL_MAX)", hi);
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  KernParams kp;
  memset(&kp, 0, sizeof(kp));
  set_exp_consts(&kp);
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  DevBuf dx, dout;
  int st = dalloc(&dx.p, n);
  st = st ? st : dalloc(&dout.p, n);
  if (st) return st;
  HIPCHK(hipMemcpyAsync(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice, sg.s));
  HIPCHK(launch_diag_exp(kp, which, hi, dx.p, n, dout.p, sg.s));
  HIPCHK(hipMemcpyAsync(out, dout.p, sizeof(double) * n, hipMemcpyDeviceToHost, sg.s));
  HIPCHK(hipStreamSynchronize(sg.s));
  return SGP_OK;
}

int sgp_diag_build_knm(int device, int kernel, int d, const double* theta, const double* X,
                       int64_t n, int64_t ldx, const double* U, int64_t m, int64_t ldu,
                       const double* r, int route, int64_t max_rows, int64_t shared_rb, double* K,
                       double* t, int* route_taken, int64_t* t_rows) {
  const char* who = "sgp_diag_build_knm";
  if (!X || !U || !K || !route_taken) {
    set_err("%s: X, U, K or route_taken is NULL", who);
    return SGP_EINVAL;
  }
  if (r && (!t || !t_rows)) {
    set_err("%s: r is given but t or t_rows is NULL", who);
    return SGP_EINVAL;
  }
  if (n < 1 || ldx < n || m < 1 || ldu < m) {
    set_err("%s: n=%lld, ldx=%lld, m=%lld, ldu=%lld (need n >= 1, ldx >= n, m >= 1, ldu >= m)",
            who, (long long)n, (long long)ldx, (long long)m, (long long)ldu);
    return SGP_EINVAL;
  }
  if (route < 0 || route > 2 || max_rows < 0 || shared_rb < -1) {
    set_err("%s: route=%d outside 0..2, max_rows=%lld < 0 or shared_rb=%lld < -1", who, route,
            (long long)max_rows, (long long)shared_rb);
    return SGP_EINVAL;
  }
  if (kernel == SGP_KERNEL_EXP) {
    set_err("%s: the K12 builders support 'sqexp' and 'ard', not 'exp'", who);
    return SGP_EINVAL;
  }
  KernParams kp;
  int st = make_params(kernel, d, theta, 0.0, &kp);   // kernel, d in [1, SGP_MAXD], theta, l > 0
  if (st) return st;
  if (!(kp.sigma > 0.0)) {
    set_err("%s: sigma must be positive", who);
    return SGP_EINVAL;
  }
  if (route == 1 && d > 32) {
    set_err("%s: the matrix-core builder needs d <= 32 (d=%d)", who, d);
    return SGP_EINVAL;
  }
  // as sgp_ctx: the centre and the span guard from the knots and the data box
  std::vector<double> xlo, xhi;
  col_range(X, n, ldx, d, &xlo, &xhi);
  set_center(&kp, U, m, ldu, xlo.data(), xhi.data());
  if (route == 1) kp.span2 = 0.0;             // the guard (knm_mfma_ok) reads nothing else
  else if (route == 2) kp.span2 = INFINITY;
  *route_taken = knm_mfma_ok(kp) ? 1 : 2;
  const int64_t np_ = round_up(n, SGP_TILE), mp = round_up(m, SGP_TILE);
  HIPCHK(hipSetDevice(device));
  StreamGuard sg;
  HIPCHK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  DevBuf dX, dU, dK, dr, dts, dpart, dt;
  st = dalloc(&dX.p, np_ * d);
  st = st ? st : dalloc(&dU.p, mp * d);
  st = st ? st : dalloc(&dK.p, np_ * mp);
  if (r) {
    st = st ? st : dalloc(&dr.p, np_);
    st = st ? st : dalloc(&dts.p, (np_ / 64) * mp);
    st = st ? st : dalloc(&dpart.p, 64 * mp);
    st = st ? st : dalloc(&dt.p, mp);
  }
  if (st) return st;
  std::vector<double> hx((size_t)(np_ * d), 0.0), hu((size_t)(mp * d), 0.0);
  for (int q = 0; q < d; ++q) {
    for (int64_t i = 0; i < n; ++i) hx[(size_t)(i + q * np_)] = X[i + q * ldx];
    for (int64_t j = 0; j < m; ++j) hu[(size_t)(j + q * mp)] = U[j + q * ldu];
  }
  HIPCHK(hipMemcpyAsync(dX.p, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, sg.s));
  HIPCHK(hipMemcpyAsync(dU.p, hu.data(), sizeof(double) * hu.size(), hipMemcpyHostToDevice, sg.s));
  // every entry is the builder's own: start from a pattern that is neither 0 nor a covariance
  HIPCHK(hipMemsetAsync(dK.p, 0xff, sizeof(double) * np_ * mp, sg.s));
  std::vector<double> hr;
  if (r) {
    hr.assign((size_t)np_, 0.0);
    for (int64_t i = 0; i < n; ++i) hr[(size_t)i] = r[i];
    HIPCHK(hipMemcpyAsync(dr.p, hr.data(), sizeof(double) * np_, hipMemcpyHostToDevice, sg.s));
  }
  int64_t trows = 0;
  HIPCHK(launch_build_knm_diag(kp, dX.p, np_, n, np_, dU.p, mp, m, mp, dK.p, r ? dr.p : nullptr,
                               dts.p, &trows, shared_rb, max_rows, sg.s));
  if (r) {
    HIPCHK(launch_knot_reduce(dts.p, trows, mp, 1, dpart.p, 64 * mp, dt.p, false, sg.s));
    HIPCHK(hipMemcpyAsync(t, dt.p, sizeof(double) * mp, hipMemcpyDeviceToHost, sg.s));
  }
  HIPCHK(hipMemcpyAsync(K, dK.p, sizeof(double) * np_ * mp, hipMemcpyDeviceToHost, sg.s));
  HIPCHK(hipStreamSynchronize(sg.s));
  if (t_rows) *t_rows = trows;
  return SGP_OK;
}


// ------------------------------------------------------------------------- batched VI
// sgp_batch (include/sgp.h; k_batch.hip): B independent small-knot VI problems
// on rows of one resident X / y / mu, four launches per evaluation of the whole batch.
}  // extern "C"

struct sgp_batch {
  int device = 0, d = 0, pst = 0, post_stride = 0;
  int64_t nrows = 0, B = 0, nseg = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  double *X = nullptr, *y = nullptr, *mu = nullptr, *par = nullptr, *rec1 = nullptr,
         *rec2 = nullptr, *pm = nullptr, *sc = nullptr, *out = nullptr, *post = nullptr,
         *res = nullptr;
  int *seg_prob = nullptr, *seg_rows = nullptr;
  int64_t* seg_row0 = nullptr;
  double *h_par = nullptr, *h_out = nullptr;   // pinned
  // sgp_batch_eval_vi_knots (sec. 0p): par and h_par end in B bound blocks of 2 d, out and h_out
  // in the packed knot gradients (up to 64 d per problem), so a call is one copy each way
  double *hk = nullptr, *rec3 = nullptr;
  // sgp_batch_eval_fitc (sec. 0q): the problems' work slots and the gradient pass's records
  double *fw = nullptr, *rec4 = nullptr;
  hipEvent_t fev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  float fstage_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  bool ftiming = false;
  hipEvent_t kev[3] = {nullptr, nullptr, nullptr};
  float kstage_ms[2] = {0.f, 0.f};
  bool ktiming = false;
  std::vector<int64_t> row0, nrow, seg0, nsegs, last_m;
  std::vector<char> has_state;
  int last_ard = 0;
  float stage_ms[4] = {0.f, 0.f, 0.f, 0.f};
  bool timing = false;
  // the held-out rows (sgp_batch_set_test) and what sgp_batch_predict works in
  bool have_test = false, have_yt = false, ptiming = false;
  int64_t ntest = 0, ntseg = 0, ttot = 0;
  std::vector<int64_t> tnrow, toff;
  double *Xt = nullptr, *yt = nullptr, *mut = nullptr, *pw = nullptr, *prec = nullptr,
         *pout = nullptr;            // pout: pred_mean | pred_var | nlp (ttot each) | stats (4 B)
  int *act = nullptr, *tseg_prob = nullptr, *tseg_rows = nullptr, *tprob_seg = nullptr;
  int64_t *tseg_row0 = nullptr, *tseg_out = nullptr;
  double* h_pout = nullptr;          // pinned
  int* h_act = nullptr;              // pinned
  hipEvent_t pev[4] = {nullptr, nullptr, nullptr, nullptr};
  float pstage_ms[3] = {0.f, 0.f, 0.f};
  // sgp_batch_lap_init / sgp_batch_eval_laplace (sec. 0s): the family (-1: none set), the
  // exposure, the latent vectors packed by problem (loff: B + 1 offsets), the work slots, the
  // control blocks, the vector records and the Newton iteration's objective values
  int lap_family = -1;
  std::vector<double> hy;              // y on the host: the Bernoulli check of lap_init / set_data
  std::vector<int64_t> loff;
  double *lexpo = nullptr, *lf = nullptr, *lzv = nullptr, *llw = nullptr, *llc = nullptr,
         *llrec = nullptr, *lobjs = nullptr;
  int64_t* lseg_loc = nullptr;
  int* lcount = nullptr;
  double* h_lc = nullptr;              // pinned
  int* h_count = nullptr;              // pinned
  hipEvent_t lev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double lstage_ms[11] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  bool ltiming = false;
};

namespace {

bool finite_all(const double* v, int64_t n, int64_t* bad) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) { *bad = i; return false; }
  return true;
}

int batch_check_create(const double* X, int64_t nrows, int64_t ldx, int d, const double* y,
                       const double* mu, const int64_t* row0, const int64_t* nrow, int64_t B) {
  if (!X || !y || !mu || !row0 || !nrow) {
    set_err("sgp_batch: X, y, mu, row0 and nrow must not be NULL");
    return SGP_EINVAL;
  }
  if (B < 1 || B > INT32_MAX) { set_err("sgp_batch: B=%lld < 1", (long long)B); return SGP_EINVAL; }
  if (d < 1 || d > SGP_MAXD) {
    set_err("input dimension d=%d outside [1, %d]", d, SGP_MAXD);
    return SGP_EINVAL;
  }
  if (nrows < 1 || ldx < nrows) {
    set_err("sgp_batch: nrows=%lld, ldx=%lld (need nrows >= 1 and ldx >= nrows)", (long long)nrows,
            (long long)ldx);
    return SGP_EINVAL;
  }
  int64_t segs = 0;
  for (int64_t b = 0; b < B; ++b) {
    if (nrow[b] < 1) {
      set_err("sgp_batch: problem %lld has nrow=%lld < 1", (long long)b, (long long)nrow[b]);
      return SGP_EINVAL;
    }
    if (row0[b] < 0 || row0[b] > nrows - nrow[b]) {
      set_err("sgp_batch: problem %lld's rows [%lld, %lld) leave [0, %lld)", (long long)b,
              (long long)row0[b], (long long)(row0[b] + nrow[b]), (long long)nrows);
      return SGP_EINVAL;
    }
    segs += (nrow[b] + SGP_BATCH_SEG_ROWS - 1) / SGP_BATCH_SEG_ROWS;
  }
  if (segs > INT32_MAX / 2) { set_err("sgp_batch: too many segments"); return SGP_EINVAL; }
  return SGP_OK;
}

int batch_check_eval(int d, int64_t B, int kernel, const double* theta, int64_t ldt,
                     const double* U, const int64_t* uoff, const int64_t* m, double delta,
                     unsigned flags, const unsigned char* active, const double* obj,
                     const double* grad, int64_t ldg, const int* status) {
  if (kernel == SGP_KERNEL_EXP) {
    set_err("sgp_batch_eval_vi supports 'sqexp' and 'ard' (optimize_gp.R:263 rejects others)");
    return SGP_EINVAL;
  }
  if (kernel != SGP_KERNEL_SQEXP && kernel != SGP_KERNEL_ARD) {
    set_err("invalid covariance function (kernel=%d)", kernel);
    return SGP_EINVAL;
  }
  const bool obj_only = flags & SGP_FLAG_OBJ_ONLY;
  if (!theta || !U || !uoff || !m || !obj || !status || (!grad && !obj_only)) {
    set_err("sgp_batch_eval_vi: theta, U, uoff, m, obj, status (and grad without "
            "SGP_FLAG_OBJ_ONLY) must not be NULL");
    return SGP_EINVAL;
  }
  const int P = num_ls(kernel, d) + 2;
  if (ldt < P) { set_err("sgp_batch_eval_vi: ldt=%lld < P=%d", (long long)ldt, P); return SGP_EINVAL; }
  if (grad && ldg < P) { set_err("sgp_batch_eval_vi: ldg=%lld < P=%d", (long long)ldg, P); return SGP_EINVAL; }
  if (!std::isfinite(delta)) { set_err("sgp_batch_eval_vi: delta is not finite"); return SGP_EINVAL; }
  for (int64_t b = 0; b < B; ++b) {
    if (active && !active[b]) continue;
    if (m[b] < 1 || m[b] > SGP_BATCH_MMAX) {
      set_err("sgp_batch_eval_vi: problem %lld has m=%lld outside [1, %d]", (long long)b,
              (long long)m[b], SGP_BATCH_MMAX);
      return SGP_EINVAL;
    }
    if (uoff[b] < 0) {
      set_err("sgp_batch_eval_vi: problem %lld has uoff=%lld < 0", (long long)b, (long long)uoff[b]);
      return SGP_EINVAL;
    }
    const double* th = theta + b * ldt;
    for (int p = 0; p < P; ++p)
      if (!std::isfinite(th[p]) || !(th[p] > 0.0)) {
        set_err("sgp_batch_eval_vi: problem %lld's theta[%d] = %g is not a positive finite number",
                (long long)b, p, th[p]);
        return SGP_EINVAL;
      }
    int64_t bad = 0;
    if (!finite_all(U + uoff[b], m[b] * d, &bad)) {
      set_err("sgp_batch_eval_vi: problem %lld's U[%lld, %lld] is not finite", (long long)b,
              (long long)(bad % m[b]), (long long)(bad / m[b]));
      return SGP_EINVAL;
    }
  }
  return SGP_OK;
}

// What sgp_batch_eval_vi_knots checks beyond batch_check_eval; sgp_diag_batch_knot_args is this
// function.
int batch_check_knots(int d, int64_t B, unsigned flags, const unsigned char* active,
                      const double* bounds, const double* grad_knot) {
  if (B < 1 || d < 1 || d > SGP_MAXD) {
    set_err("sgp_batch_eval_vi_knots: B=%lld, d=%d", (long long)B, d);
    return SGP_EINVAL;
  }
  if (!grad_knot) { set_err("sgp_batch_eval_vi_knots: grad_knot must not be NULL"); return SGP_EINVAL; }
  if (flags & SGP_FLAG_OBJ_ONLY) {
    set_err("sgp_batch_eval_vi_knots: flags has SGP_FLAG_OBJ_ONLY (the knot gradient needs the "
            "second row pass)");
    return SGP_EINVAL;
  }
  if (bounds)
    for (int64_t b = 0; b < B; ++b) {
      if (active && !active[b]) continue;
      int64_t bad = 0;
      if (!finite_all(bounds + 2 * d * b, 2 * d, &bad)) {
        set_err("sgp_batch_eval_vi_knots: problem %lld's bounds[%lld, %lld] is not finite",
                (long long)b, (long long)(bad % d), (long long)(bad / d));
        return SGP_EINVAL;
      }
    }
  return SGP_OK;
}

// The test-row plan: problem p's tnrow[p] test rows in segments of at most SGP_BATCH_SEG_ROWS
// counted from its own first test row (sgp_diag_batch_plan's rule; a problem without rows has no
// segment), and toff, the problems' first rows in the packed outputs.
int64_t batch_test_plan(const int64_t* trow0, const int64_t* tnrow, int64_t B, int64_t cap,
                        int64_t* seg_prob, int64_t* seg_row0, int64_t* seg_rows, int64_t* toff) {
  int64_t k = 0, at = 0;
  for (int64_t p = 0; p < B; ++p) {
    if (toff) toff[p] = at;
    for (int64_t r = 0; r < tnrow[p]; r += SGP_BATCH_SEG_ROWS, ++k)
      if (k < cap) {
        seg_prob[k] = p;
        seg_row0[k] = trow0[p] + r;
        seg_rows[k] = std::min<int64_t>(SGP_BATCH_SEG_ROWS, tnrow[p] - r);
      }
    at += tnrow[p];
  }
  if (toff) toff[B] = at;
  return k;
}

// The argument checks of sgp_batch_set_test (stage 0) and sgp_batch_predict (stage 1), made
// before the first device call; sgp_diag_batch_test_args is this function.
int batch_check_test(int stage, int d, int64_t B, const double* Xt, int64_t ntest, int64_t ldxt,
                     const double* yt, const double* mut, const int64_t* trow0,
                     const int64_t* tnrow, int have_test, int have_yt,
                     const unsigned char* has_state, const unsigned char* active,
                     const double* pred_mean, const double* pred_var, const double* nlp,
                     const double* stats) {
  if (B < 1 || B > INT32_MAX) { set_err("sgp_batch: B=%lld < 1", (long long)B); return SGP_EINVAL; }
  if (stage == 0) {
    if (!Xt || !mut || !trow0 || !tnrow) {
      set_err("sgp_batch_set_test: Xt, mut, trow0 and tnrow must not be NULL");
      return SGP_EINVAL;
    }
    if (d < 1 || d > SGP_MAXD) {
      set_err("input dimension d=%d outside [1, %d]", d, SGP_MAXD);
      return SGP_EINVAL;
    }
    if (ntest < 1 || ldxt < ntest) {
      set_err("sgp_batch_set_test: ntest=%lld, ldxt=%lld (need ntest >= 1 and ldxt >= ntest)",
              (long long)ntest, (long long)ldxt);
      return SGP_EINVAL;
    }
    int64_t segs = 0, tot = 0;
    for (int64_t b = 0; b < B; ++b) {
      if (tnrow[b] < 0) {
        set_err("sgp_batch_set_test: problem %lld has tnrow=%lld < 0", (long long)b,
                (long long)tnrow[b]);
        return SGP_EINVAL;
      }
      if (trow0[b] < 0 || trow0[b] > ntest - tnrow[b]) {
        set_err("sgp_batch_set_test: problem %lld's test rows [%lld, %lld) leave [0, %lld)",
                (long long)b, (long long)trow0[b], (long long)(trow0[b] + tnrow[b]),
                (long long)ntest);
        return SGP_EINVAL;
      }
      segs += (tnrow[b] + SGP_BATCH_SEG_ROWS - 1) / SGP_BATCH_SEG_ROWS;
      tot += tnrow[b];
      if (segs > INT32_MAX / 2 || tot > (int64_t)1 << 40) {
        set_err("sgp_batch_set_test: too many test rows");
        return SGP_EINVAL;
      }
    }
    int64_t bad = 0;
    for (int c = 0; c < d; ++c)
      if (!finite_all(Xt + (int64_t)c * ldxt, ntest, &bad)) {
        set_err("sgp_batch_set_test: Xt[%lld, %d] is not finite", (long long)bad, c);
        return SGP_EINVAL;
      }
    if (yt && !finite_all(yt, ntest, &bad)) {
      set_err("sgp_batch_set_test: yt[%lld] is not finite", (long long)bad);
      return SGP_EINVAL;
    }
    return SGP_OK;
  }
  if (stage != 1) { set_err("sgp_diag_batch_test_args: stage=%d", stage); return SGP_EINVAL; }
  if (!pred_mean || !pred_var) {
    set_err("sgp_batch_predict: pred_mean and pred_var must not be NULL");
    return SGP_EINVAL;
  }
  if ((nlp == nullptr) != (stats == nullptr)) {
    set_err("sgp_batch_predict: nlp and stats must both be given or both be NULL");
    return SGP_EINVAL;
  }
  if (!have_test) {
    set_err("sgp_batch_predict: no test rows (call sgp_batch_set_test first)");
    return SGP_EINVAL;
  }
  if (nlp && !have_yt) {
    set_err("sgp_batch_predict: nlp asked for, but sgp_batch_set_test had yt = NULL");
    return SGP_EINVAL;
  }
  if (!has_state) { set_err("sgp_batch_predict: has_state is NULL"); return SGP_EINVAL; }
  for (int64_t b = 0; b < B; ++b)
    if ((!active || active[b]) && !has_state[b]) {
      set_err("sgp_batch_predict: problem %lld has no posterior (no successful evaluation since "
              "create / set_data)", (long long)b);
      return SGP_EINVAL;
    }
  return SGP_OK;
}

// Under the Bernoulli family every y in a problem's range is 0 or 1
// (R/derivative_functions_of_data_likelihoods.R:86-184 take y as a class label).
int batch_check_bern(const char* who, const double* y, const int64_t* row0, const int64_t* nrow,
                     int64_t B) {
  for (int64_t p = 0; p < B; ++p)
    for (int64_t i = row0[p]; i < row0[p] + nrow[p]; ++i)
      if (!(y[i] == 0.0 || y[i] == 1.0)) {
        set_err("%s: y[%lld] = %g (problem %lld) is not 0 or 1 under SGP_FAM_BERNOULLI", who,
                (long long)i, y[i], (long long)p);
        return SGP_EINVAL;
      }
  return SGP_OK;
}

// The argument checks of sgp_batch_lap_init, made before its first device call;
// sgp_diag_batch_lap_args is this function.
int batch_check_lap(const double* y, int64_t nrows, const int64_t* row0, const int64_t* nrow,
                    int64_t B, int family, const double* expo) {
  if (family != SGP_FAM_POISSON && family != SGP_FAM_BERNOULLI) {
    set_err("sgp_batch_lap_init: family=%d (need SGP_FAM_POISSON or SGP_FAM_BERNOULLI)", family);
    return SGP_EINVAL;
  }
  if (!y || !row0 || !nrow || B < 1 || nrows < 1) {
    set_err("sgp_batch_lap_init: y, row0 and nrow must not be NULL");
    return SGP_EINVAL;
  }
  for (int64_t p = 0; p < B; ++p)
    if (nrow[p] < 1 || row0[p] < 0 || row0[p] > nrows - nrow[p]) {
      set_err("sgp_batch: problem %lld's rows [%lld, %lld) leave [0, %lld)", (long long)p,
              (long long)row0[p], (long long)(row0[p] + nrow[p]), (long long)nrows);
      return SGP_EINVAL;
    }
  if (expo)
    for (int64_t i = 0; i < nrows; ++i)
      if (!std::isfinite(expo[i]) || !(expo[i] > 0.0)) {
        set_err("sgp_batch_lap_init: expo[%lld] = %g is not a positive finite number",
                (long long)i, expo[i]);
        return SGP_EINVAL;
      }
  if (family == SGP_FAM_BERNOULLI) return batch_check_bern("sgp_batch_lap_init", y, row0, nrow, B);
  return SGP_OK;
}

// What sgp_batch_eval_laplace checks beyond batch_check_eval
int batch_check_lap_eval(int family, double tol, int maxit, const int* nr_iters) {
  if (family < 0) {
    set_err("sgp_batch_eval_laplace: no family set (call sgp_batch_lap_init first)");
    return SGP_EINVAL;
  }
  if (!(tol >= 0.0) || !std::isfinite(tol) || maxit < 0) {
    set_err("invalid Laplace controls (tol=%g, maxit=%d)", tol, maxit);
    return SGP_EINVAL;
  }
  if (!nr_iters) { set_err("sgp_batch_eval_laplace: nr_iters must not be NULL"); return SGP_EINVAL; }
  return SGP_OK;
}

void batch_free_lap(sgp_batch* b);

void batch_free_test(sgp_batch* b) {
  for (double** p : {&b->Xt, &b->yt, &b->mut, &b->pw, &b->prec, &b->pout})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  for (int** p : {&b->act, &b->tseg_prob, &b->tseg_rows, &b->tprob_seg})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  for (int64_t** p : {&b->tseg_row0, &b->tseg_out})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (b->h_pout) { (void)hipHostFree(b->h_pout); b->h_pout = nullptr; }
  if (b->h_act) { (void)hipHostFree(b->h_act); b->h_act = nullptr; }
  b->have_test = b->have_yt = false;
}

void batch_free_lap(sgp_batch* b) {
  for (double** p : {&b->lexpo, &b->lf, &b->lzv, &b->llw, &b->llc, &b->llrec, &b->lobjs})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (b->lseg_loc) { (void)hipFree(b->lseg_loc); b->lseg_loc = nullptr; }
  if (b->lcount) { (void)hipFree(b->lcount); b->lcount = nullptr; }
  if (b->h_lc) { (void)hipHostFree(b->h_lc); b->h_lc = nullptr; }
  if (b->h_count) { (void)hipHostFree(b->h_count); b->h_count = nullptr; }
  for (hipEvent_t& e : b->lev)
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
  b->lap_family = -1;
}

void batch_free(sgp_batch* b) {
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  batch_free_test(b);
  for (hipEvent_t e : b->pev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : b->kev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : b->fev)
    if (e) (void)hipEventDestroy(e);
  batch_free_lap(b);
  for (double* p : {b->X, b->y, b->mu, b->par, b->rec1, b->rec2, b->pm, b->sc, b->out, b->post,
                    b->res, b->hk, b->rec3, b->fw, b->rec4})
    if (p) (void)hipFree(p);
  if (b->seg_prob) (void)hipFree(b->seg_prob);
  if (b->seg_rows) (void)hipFree(b->seg_rows);
  if (b->seg_row0) (void)hipFree(b->seg_row0);
  if (b->h_par) (void)hipHostFree(b->h_par);
  if (b->h_out) (void)hipHostFree(b->h_out);
  for (hipEvent_t e : b->ev)
    if (e) (void)hipEventDestroy(e);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
}

BatchArgs batch_args(const sgp_batch* b, int ard, int obj_only) {
  BatchArgs a;
  a.X = b->X; a.y = b->y; a.mu = b->mu; a.ldx = b->nrows;
  a.par = b->par; a.pst = b->pst; a.d = b->d; a.ard = ard; a.obj_only = obj_only;
  a.B = (int)b->B; a.nseg = (int)b->nseg;
  a.seg_prob = b->seg_prob; a.seg_row0 = b->seg_row0; a.seg_rows = b->seg_rows;
  a.rec1 = b->rec1; a.rec2 = b->rec2; a.pm = b->pm; a.sc = b->sc; a.out = b->out;
  a.post = b->post; a.post_stride = b->post_stride;
  a.hk = nullptr; a.rec3 = nullptr; a.bnd = nullptr; a.gk = nullptr;
  a.fw = b->fw; a.rec4 = b->rec4;
  return a;
}

int batch_create_impl(sgp_batch* b, const double* X, int64_t ldx, const double* y,
                      const double* mu) {
  const int64_t B = b->B, n = b->nrows;
  const int d = b->d;
  std::vector<int> sp, sr;
  std::vector<int64_t> s0;
  for (int64_t p = 0; p < B; ++p) {
    b->seg0[(size_t)p] = (int64_t)sp.size();
    for (int64_t r = 0; r < b->nrow[(size_t)p]; r += SGP_BATCH_SEG_ROWS) {
      sp.push_back((int)p);
      s0.push_back(b->row0[(size_t)p] + r);
      sr.push_back((int)std::min<int64_t>(SGP_BATCH_SEG_ROWS, b->nrow[(size_t)p] - r));
    }
    b->nsegs[(size_t)p] = (int64_t)sp.size() - b->seg0[(size_t)p];
  }
  b->nseg = (int64_t)sp.size();
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  for (hipEvent_t& e : b->ev) HIPCHK(hipEventCreate(&e));
  for (hipEvent_t& e : b->kev) HIPCHK(hipEventCreate(&e));
  for (hipEvent_t& e : b->fev) HIPCHK(hipEventCreate(&e));
  const int64_t gcap = B * SGP_BATCH_MMAX * d;   // the packed knot gradients at their largest
  HIPCHK(hipMalloc(&b->X, sizeof(double) * n * d));
  HIPCHK(hipMalloc(&b->y, sizeof(double) * n));
  HIPCHK(hipMalloc(&b->mu, sizeof(double) * n));
  HIPCHK(hipMalloc(&b->par, sizeof(double) * B * (b->pst + 2 * d)));
  HIPCHK(hipMalloc(&b->rec1, sizeof(double) * b->nseg * BATCH_REC1));
  HIPCHK(hipMalloc(&b->rec2, sizeof(double) * b->nseg * BATCH_REC2));
  HIPCHK(hipMalloc(&b->pm, sizeof(double) * B * BATCH_PM));
  HIPCHK(hipMalloc(&b->sc, sizeof(double) * B * BATCH_SC));
  HIPCHK(hipMalloc(&b->out, sizeof(double) * (B * BATCH_OUT + gcap)));
  HIPCHK(hipMalloc(&b->hk, sizeof(double) * B * BR_T));
  HIPCHK(hipMalloc(&b->rec3, sizeof(double) * b->nseg * BATCH_REC3));
  HIPCHK(hipMalloc(&b->fw, sizeof(double) * B * BATCH_FW));
  HIPCHK(hipMalloc(&b->rec4, sizeof(double) * b->nseg * BATCH_REC4));
  HIPCHK(hipMalloc(&b->post, sizeof(double) * B * b->post_stride));
  HIPCHK(hipMalloc(&b->res, sizeof(double) * B * (BR_T + SGP_BATCH_MMAX)));
  HIPCHK(hipMalloc(&b->seg_prob, sizeof(int) * b->nseg));
  HIPCHK(hipMalloc(&b->seg_rows, sizeof(int) * b->nseg));
  HIPCHK(hipMalloc(&b->seg_row0, sizeof(int64_t) * b->nseg));
  HIPCHK(hipHostMalloc(&b->h_par, sizeof(double) * B * (b->pst + 2 * d)));
  HIPCHK(hipHostMalloc(&b->h_out, sizeof(double) * (B * BATCH_OUT + gcap)));
  HIPCHK(hipMemsetAsync(b->post, 0, sizeof(double) * B * b->post_stride, b->stream));
  HIPCHK(hipMemsetAsync(b->out, 0, sizeof(double) * B * BATCH_OUT, b->stream));
  HIPCHK(hipMemcpy2DAsync(b->X, sizeof(double) * n, X, sizeof(double) * ldx, sizeof(double) * n,
                          (size_t)d, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->y, y, sizeof(double) * n, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->mu, mu, sizeof(double) * n, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->seg_prob, sp.data(), sizeof(int) * sp.size(), hipMemcpyHostToDevice,
                        b->stream));
  HIPCHK(hipMemcpyAsync(b->seg_rows, sr.data(), sizeof(int) * sr.size(), hipMemcpyHostToDevice,
                        b->stream));
  HIPCHK(hipMemcpyAsync(b->seg_row0, s0.data(), sizeof(int64_t) * s0.size(),
                        hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return SGP_OK;
}

}  // namespace

extern "C" {

int sgp_diag_batch_args(int stage, const double* X, int64_t nrows, int64_t ldx, int d,
                        const double* y, const double* mu, const int64_t* row0,
                        const int64_t* nrow, int64_t B, int kernel, const double* theta,
                        int64_t ldt, const double* U, const int64_t* uoff, const int64_t* m,
                        double delta, unsigned flags, const unsigned char* active,
                        const double* obj, const double* grad, int64_t ldg, const int* status) {
  if (stage != 0 && stage != 1) { set_err("sgp_diag_batch_args: stage=%d", stage); return SGP_EINVAL; }
  const int st = batch_check_create(X, nrows, ldx, d, y, mu, row0, nrow, B);
  if (st != SGP_OK || stage == 0) return st;
  return batch_check_eval(d, B, kernel, theta, ldt, U, uoff, m, delta, flags, active, obj, grad,
                          ldg, status);
}

int sgp_diag_batch_plan(const int64_t* row0, const int64_t* nrow, int64_t B, int64_t cap,
                        int64_t* nseg, int64_t* seg_prob, int64_t* seg_row0, int64_t* seg_rows,
                        int64_t* seg_rows_max) {
  if (!row0 || !nrow || B < 1 || !nseg || cap < 0 ||
      (cap > 0 && (!seg_prob || !seg_row0 || !seg_rows))) {
    set_err("invalid sgp_diag_batch_plan arguments");
    return SGP_EINVAL;
  }
  int64_t k = 0;
  for (int64_t p = 0; p < B; ++p) {
    if (nrow[p] < 1 || row0[p] < 0) {
      set_err("sgp_diag_batch_plan: problem %lld has row0=%lld, nrow=%lld", (long long)p,
              (long long)row0[p], (long long)nrow[p]);
      return SGP_EINVAL;
    }
    for (int64_t r = 0; r < nrow[p]; r += SGP_BATCH_SEG_ROWS, ++k)
      if (k < cap) {
        seg_prob[k] = p;
        seg_row0[k] = row0[p] + r;
        seg_rows[k] = std::min<int64_t>(SGP_BATCH_SEG_ROWS, nrow[p] - r);
      }
  }
  *nseg = k;
  if (seg_rows_max) *seg_rows_max = SGP_BATCH_SEG_ROWS;
  return SGP_OK;
}

int sgp_batch_create(sgp_batch** out, int device, const double* X, int64_t nrows, int64_t ldx,
                     int d, const double* y, const double* mu, const int64_t* row0,
                     const int64_t* nrow, int64_t B) {
  if (!out) { set_err("sgp_batch_create: out is NULL"); return SGP_EINVAL; }
  *out = nullptr;
  const int st = batch_check_create(X, nrows, ldx, d, y, mu, row0, nrow, B);
  if (st != SGP_OK) return st;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    set_err("sgp_batch_create: no HIP device visible (there is no CPU path)");
    return SGP_EHIP;
  }
  if (device < 0 || device >= ndev) {
    set_err("sgp_batch_create: device %d, but %d device(s) are visible", device, ndev);
    return SGP_EINVAL;
  }
  sgp_batch* b = new sgp_batch;
  b->device = device;
  b->d = d;
  b->nrows = nrows;
  b->B = B;
  b->pst = BP_U + SGP_BATCH_MMAX * d;
  b->post_stride = BR_T + SGP_BATCH_MMAX + b->pst;
  b->row0.assign(row0, row0 + B);
  b->nrow.assign(nrow, nrow + B);
  b->seg0.assign((size_t)B, 0);
  b->nsegs.assign((size_t)B, 0);
  b->last_m.assign((size_t)B, 0);
  b->has_state.assign((size_t)B, 0);
  b->hy.assign(y, y + nrows);
  const int cst = batch_create_impl(b, X, ldx, y, mu);
  if (cst != SGP_OK) {
    const std::string keep = g_err;
    batch_free(b);
    g_err = keep;
    return cst;
  }
  *out = b;
  return SGP_OK;
}

int sgp_batch_destroy(sgp_batch* b) {
  if (!b) { set_err("sgp_batch_destroy: the sgp_batch is NULL"); return SGP_EINVAL; }
  batch_free(b);
  return SGP_OK;
}

int sgp_batch_set_data(sgp_batch* b, const double* y, const double* mu) {
  if (!b) { set_err("sgp_batch_set_data: the sgp_batch is NULL"); return SGP_EINVAL; }
  if (!y || !mu) { set_err("sgp_batch_set_data: y and mu must not be NULL"); return SGP_EINVAL; }
  if (b->lap_family == SGP_FAM_BERNOULLI) {
    const int bst = batch_check_bern("sgp_batch_set_data", y, b->row0.data(), b->nrow.data(), b->B);
    if (bst != SGP_OK) return bst;
  }
  b->hy.assign(y, y + b->nrows);
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(b->y, y, sizeof(double) * b->nrows, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->mu, mu, sizeof(double) * b->nrows, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  std::fill(b->has_state.begin(), b->has_state.end(), 0);   // the posteriors were of the old data
  HIPCHK(hipMemsetAsync(b->post, 0, sizeof(double) * b->B * b->post_stride, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return SGP_OK;
}

}  // extern "C"

namespace {

// The problems' parameter blocks into h_par (objective: BP_OBJ's value); *gtot: the active
// problems' m d values.  Returns whether any problem is active.
bool batch_fill_par(sgp_batch* b, int objective, int kernel, const double* theta, int64_t ldt,
                    const double* U, const int64_t* uoff, const int64_t* m, double delta,
                    unsigned flags, const unsigned char* active, int64_t* gtot) {
  const int d = b->d, ard = kernel == SGP_KERNEL_ARD, L = ard ? d : 1;
  bool any = false;
  *gtot = 0;
  for (int64_t p = 0; p < b->B; ++p) {
    double* h = b->h_par + p * b->pst;
    const bool on = !active || active[p];
    h[BP_ACTIVE] = on ? 1.0 : 0.0;
    if (!on) continue;
    any = true;
    const double* th = theta + p * ldt;
    const double tau2 = th[L + 1] * th[L + 1];
    h[BP_M] = (double)m[p];
    h[BP_SIG2] = th[0] * th[0];
    h[BP_TAU2] = tau2;
    h[BP_Z] = tau2 + delta;
    h[BP_DELTA] = delta;
    h[BP_NROW] = (double)b->nrow[(size_t)p];
    h[BP_RDET] = (flags & SGP_FLAG_R_DET) ? 1.0 : 0.0;
    h[BP_SEG0] = (double)b->seg0[(size_t)p];
    h[BP_NSEG] = (double)b->nsegs[(size_t)p];
    h[BP_GOFF] = (double)*gtot;
    h[BP_OBJ] = (double)objective;
    *gtot += m[p] * d;
    for (int c = 0; c < d; ++c) h[BP_RL + c] = 1.0 / th[1 + (ard ? c : 0)];
    const double* u = U + uoff[p];
    for (int c = 0; c < d; ++c)
      for (int j = 0; j < SGP_BATCH_MMAX; ++j)
        h[BP_U + c * SGP_BATCH_MMAX + j] = j < m[p] ? u[(int64_t)c * m[p] + j] : 0.0;
  }
  return any;
}

// sgp_batch_eval_vi (grad_knot = nullptr) and sgp_batch_eval_vi_knots after their checks: the
// same four launches on the same arguments, and with grad_knot the two knot launches behind them;
// sgp_batch_eval_fitc (fitc = 1, grad_knot = nullptr): its five launches on the same arguments
int batch_eval_impl(sgp_batch* b, int fitc, int kernel, const double* theta, int64_t ldt, const double* U,
                    const int64_t* uoff, const int64_t* m, double delta, unsigned flags,
                    const unsigned char* active, double* obj, double* grad, int64_t ldg,
                    int* status, const double* bounds, double* grad_knot) {
  const int d = b->d, ard = kernel == SGP_KERNEL_ARD, L = ard ? d : 1, P = L + 2;
  const bool obj_only = flags & SGP_FLAG_OBJ_ONLY;
  int64_t gtot = 0;   // the packed knot gradients: the active problems' m d values in order
  const bool any = batch_fill_par(b, fitc ? 1 : 0, kernel, theta, ldt, U, uoff, m, delta, flags,
                                  active, &gtot);
  if (!any) return SGP_OK;
  const int64_t npar = b->B * b->pst;
  if (grad_knot && bounds) std::copy(bounds, bounds + b->B * 2 * d, b->h_par + npar);
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(b->par, b->h_par,
                        sizeof(double) * (npar + (grad_knot && bounds ? b->B * 2 * d : 0)),
                        hipMemcpyHostToDevice, b->stream));
  BatchArgs a = batch_args(b, ard, obj_only ? 1 : 0);
  if (grad_knot) {
    a.hk = b->hk;
    a.rec3 = b->rec3;
    a.bnd = bounds ? b->par + npar : nullptr;
    a.gk = b->out + b->B * BATCH_OUT;
  }
  if (fitc) HIPCHK(launch_batch_eval_fitc(a, b->stream, b->ftiming ? b->fev : nullptr));
  else HIPCHK(launch_batch_eval(a, b->stream, b->timing ? b->ev : nullptr));
  if (grad_knot) HIPCHK(launch_batch_knots(a, b->stream, b->ktiming ? b->kev : nullptr));
  HIPCHK(hipMemcpyAsync(b->h_out, b->out,
                        sizeof(double) * (b->B * BATCH_OUT + (grad_knot ? gtot : 0)),
                        hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (!fitc && b->timing)
    for (int q = 0; q < 4; ++q) HIPCHK(hipEventElapsedTime(&b->stage_ms[q], b->ev[q], b->ev[q + 1]));
  if (fitc && b->ftiming)
    for (int q = 0; q < 5; ++q)
      HIPCHK(hipEventElapsedTime(&b->fstage_ms[q], b->fev[q], b->fev[q + 1]));
  if (grad_knot && b->ktiming)
    for (int q = 0; q < 2; ++q)
      HIPCHK(hipEventElapsedTime(&b->kstage_ms[q], b->kev[q], b->kev[q + 1]));
  b->last_ard = ard;
  bool failed = false;
  for (int64_t p = 0; p < b->B; ++p) {
    if (active && !active[p]) continue;
    const double* o = b->h_out + p * BATCH_OUT;
    const int st = (int)o[1];
    status[p] = st;
    if (st) {
      obj[p] = NAN;
      if (grad)
        for (int q = 0; q < P; ++q) grad[p * ldg + q] = NAN;
      if (grad_knot)
        for (int64_t q = 0; q < m[p] * d; ++q) grad_knot[uoff[p] + q] = NAN;
      if (!failed)
        set_err("problem %lld: chol(): the leading minor of order %d of %s is not positive definite",
                (long long)p, st > 0 ? st : -st,
                st > 0 ? "Sigma22" : "Sigma22 + t(Sigma12) %*% ZSig12");
      failed = true;
      continue;
    }
    obj[p] = o[0];
    if (fitc && std::isnan(o[0])) {   // some Z_i is not positive and finite: no posterior
      if (grad)
        for (int q = 0; q < P; ++q) grad[p * ldg + q] = NAN;
      continue;
    }
    if (!obj_only)
      for (int q = 0; q < P; ++q) grad[p * ldg + q] = o[2 + q];
    if (grad_knot) {
      const double* gk = b->h_out + b->B * BATCH_OUT + (int64_t)b->h_par[p * b->pst + BP_GOFF];
      std::copy(gk, gk + m[p] * d, grad_knot + uoff[p]);
    }
    b->has_state[(size_t)p] = 1;
    b->last_m[(size_t)p] = m[p];
  }
  return SGP_OK;
}

}  // namespace

extern "C" {

int sgp_batch_eval_vi(sgp_batch* b, int kernel, const double* theta, int64_t ldt, const double* U,
                      const int64_t* uoff, const int64_t* m, double delta, unsigned flags,
                      const unsigned char* active, double* obj, double* grad, int64_t ldg,
                      int* status) {
  if (!b) { set_err("sgp_batch_eval_vi: the sgp_batch is NULL"); return SGP_EINVAL; }
  const int cst = batch_check_eval(b->d, b->B, kernel, theta, ldt, U, uoff, m, delta, flags,
                                   active, obj, grad, ldg, status);
  if (cst != SGP_OK) return cst;
  return batch_eval_impl(b, 0, kernel, theta, ldt, U, uoff, m, delta, flags, active, obj, grad,
                         ldg, status, nullptr, nullptr);
}

int sgp_batch_eval_fitc(sgp_batch* b, int kernel, const double* theta, int64_t ldt,
                        const double* U, const int64_t* uoff, const int64_t* m, double delta,
                        unsigned flags, const unsigned char* active, double* obj, double* grad,
                        int64_t ldg, int* status) {
  if (!b) { set_err("sgp_batch_eval_fitc: the sgp_batch is NULL"); return SGP_EINVAL; }
  const int cst = batch_check_eval(b->d, b->B, kernel, theta, ldt, U, uoff, m, delta, flags,
                                   active, obj, grad, ldg, status);
  if (cst != SGP_OK) return cst;
  return batch_eval_impl(b, 1, kernel, theta, ldt, U, uoff, m, delta, flags, active, obj, grad,
                         ldg, status, nullptr, nullptr);
}

/* stage_ms (5 doubles, or NULL): the HIP-event times of K22's stage, the weighted pass 1, Bm's
 * stage, the gradient pass and the G22 stage of the last sgp_batch_eval_fitc; enable != 0 records
 * them from the next such call on. */
int sgp_diag_batch_fitc_timing(sgp_batch* b, int enable, double* stage_ms) {
  if (!b) { set_err("sgp_diag_batch_fitc_timing: the sgp_batch is NULL"); return SGP_EINVAL; }
  if (stage_ms)
    for (int q = 0; q < 5; ++q) stage_ms[q] = b->ftiming ? (double)b->fstage_ms[q] : 0.0;
  b->ftiming = enable != 0;
  return SGP_OK;
}

// ------------------------------------------------------------------------- batched Laplace
// sgp_batch_lap_* / sgp_batch_eval_laplace (include/sgp.h; k_batch_laplace.hip)
int sgp_diag_batch_lap_args(const double* y, int64_t nrows, const int64_t* row0,
                            const int64_t* nrow, int64_t B, int family, const double* expo) {
  return batch_check_lap(y, nrows, row0, nrow, B, family, expo);
}

int sgp_batch_lap_init(sgp_batch* b, int family, const double* expo) {
  if (!b) { set_err("sgp_batch_lap_init: the sgp_batch is NULL"); return SGP_EINVAL; }
  const int cst = batch_check_lap(b->hy.data(), b->nrows, b->row0.data(), b->nrow.data(), b->B,
                                  family, expo);
  if (cst != SGP_OK) return cst;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (b->loff.empty()) {   // the first call allocates; a repeat replaces family, exposure and f
    std::vector<int64_t> off((size_t)b->B + 1, 0), sl((size_t)b->nseg, 0);
    for (int64_t p = 0; p < b->B; ++p) {
      off[(size_t)p + 1] = off[(size_t)p] + b->nrow[(size_t)p];
      for (int64_t q = 0; q < b->nsegs[(size_t)p]; ++q)
        sl[(size_t)(b->seg0[(size_t)p] + q)] = off[(size_t)p] + q * SGP_BATCH_SEG_ROWS;
    }
    const int64_t tot = off[(size_t)b->B];
    for (hipEvent_t& e : b->lev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipMalloc(&b->lexpo, sizeof(double) * b->nrows));
    HIPCHK(hipMalloc(&b->lf, sizeof(double) * tot));
    HIPCHK(hipMalloc(&b->lzv, sizeof(double) * tot));
    HIPCHK(hipMalloc(&b->llw, sizeof(double) * b->B * BATCH_LW));
    HIPCHK(hipMalloc(&b->llc, sizeof(double) * b->B * BATCH_LC));
    HIPCHK(hipMalloc(&b->llrec, sizeof(double) * b->nseg * BATCH_LREC));
    HIPCHK(hipMalloc(&b->lobjs, sizeof(double) * b->B * BATCH_LAP_NOBJ));
    HIPCHK(hipMalloc(&b->lseg_loc, sizeof(int64_t) * b->nseg));
    HIPCHK(hipMalloc(&b->lcount, sizeof(int)));
    HIPCHK(hipHostMalloc(&b->h_lc, sizeof(double) * b->B * BATCH_LC));
    HIPCHK(hipHostMalloc(&b->h_count, sizeof(int)));
    HIPCHK(hipMemcpy(b->lseg_loc, sl.data(), sizeof(int64_t) * sl.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(b->llc, 0, sizeof(double) * b->B * BATCH_LC, b->stream));
    HIPCHK(hipMemsetAsync(b->lobjs, 0, sizeof(double) * b->B * BATCH_LAP_NOBJ, b->stream));
    b->loff = off;
  }
  const int64_t tot = b->loff[(size_t)b->B];
  if (expo) {
    HIPCHK(hipMemcpy(b->lexpo, expo, sizeof(double) * b->nrows, hipMemcpyHostToDevice));
  } else {
    const std::vector<double> one((size_t)b->nrows, 1.0);
    HIPCHK(hipMemcpy(b->lexpo, one.data(), sizeof(double) * b->nrows, hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemsetAsync(b->lf, 0, sizeof(double) * tot, b->stream));   // f starts at 0
  HIPCHK(hipStreamSynchronize(b->stream));
  b->lap_family = family;
  return SGP_OK;
}

int sgp_batch_lap_set_f(sgp_batch* b, const double* f, const double* fill) {
  if (!b) { set_err("sgp_batch_lap_set_f: the sgp_batch is NULL"); return SGP_EINVAL; }
  if (b->lap_family < 0) {
    set_err("sgp_batch_lap_set_f: no family set (call sgp_batch_lap_init first)");
    return SGP_EINVAL;
  }
  if (!f && !fill) { set_err("sgp_batch_lap_set_f: f and fill are both NULL"); return SGP_EINVAL; }
  const int64_t tot = b->loff[(size_t)b->B];
  int64_t bad = 0;
  if (!finite_all(f ? f : fill, f ? tot : b->B, &bad)) {
    set_err("sgp_batch_lap_set_f: %s[%lld] is not finite", f ? "f" : "fill", (long long)bad);
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (f) {
    HIPCHK(hipMemcpy(b->lf, f, sizeof(double) * tot, hipMemcpyHostToDevice));
  } else {
    std::vector<double> h((size_t)tot);
    for (int64_t p = 0; p < b->B; ++p)
      std::fill(h.begin() + b->loff[(size_t)p], h.begin() + b->loff[(size_t)p + 1], fill[p]);
    HIPCHK(hipMemcpy(b->lf, h.data(), sizeof(double) * tot, hipMemcpyHostToDevice));
  }
  return SGP_OK;
}

int sgp_batch_lap_get_f(sgp_batch* b, double* f) {
  if (!b) { set_err("sgp_batch_lap_get_f: the sgp_batch is NULL"); return SGP_EINVAL; }
  if (b->lap_family < 0) {
    set_err("sgp_batch_lap_get_f: no family set (call sgp_batch_lap_init first)");
    return SGP_EINVAL;
  }
  if (!f) { set_err("sgp_batch_lap_get_f: f is NULL"); return SGP_EINVAL; }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(f, b->lf, sizeof(double) * b->loff[(size_t)b->B], hipMemcpyDeviceToHost));
  return SGP_OK;
}

}  // extern "C"

namespace {

// sgp_batch_eval_laplace after its checks.  The per-theta stages and the first objective, then
// one Newton iteration per turn of the loop over the problems still running: the stop decisions
// are the device's, and the host reads back their count alone.
int batch_eval_laplace_impl(sgp_batch* b, int kernel, const double* theta, int64_t ldt,
                            const double* U, const int64_t* uoff, const int64_t* m, double delta,
                            unsigned flags, const unsigned char* active, double* obj,
                            double* grad, int64_t ldg, int* status, double tol, int maxit,
                            int* nr_iters) {
  const int d = b->d, ard = kernel == SGP_KERNEL_ARD, L = ard ? d : 1, P = L + 2;
  const bool obj_only = flags & SGP_FLAG_OBJ_ONLY;
  int64_t gtot = 0;
  if (!batch_fill_par(b, 2, kernel, theta, ldt, U, uoff, m, delta, flags, active, &gtot))
    return SGP_OK;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(b->par, b->h_par, sizeof(double) * b->B * b->pst, hipMemcpyHostToDevice,
                        b->stream));
  const BatchArgs a = batch_args(b, ard, obj_only ? 1 : 0);
  BatchLapArgs l;
  l.family = b->lap_family; l.maxit = maxit; l.tol = tol;
  l.expo = b->lap_family == SGP_FAM_POISSON ? b->lexpo : nullptr;   // only Poisson reads it
  l.seg_loc = b->lseg_loc;
  l.f = b->lf; l.zv = b->lzv; l.lw = b->llw; l.lc = b->llc; l.lrec = b->llrec;
  l.objs = b->lobjs; l.count = b->lcount;
  const bool tm = b->ltiming;
  if (tm) std::fill(b->lstage_ms, b->lstage_ms + 11, 0.0);
  // stages[q] runs between events q and q + 1; their times are added to lstage_ms[slot[q]]
  auto run = [&](const int* stages, const int* slot, int n, bool count) -> int {
    for (int q = 0; q < n; ++q) {
      if (tm) HIPCHK(hipEventRecord(b->lev[q], b->stream));
      HIPCHK(launch_batch_laplace(stages[q], a, l, b->stream));
    }
    if (tm) HIPCHK(hipEventRecord(b->lev[n], b->stream));
    if (count) {
      HIPCHK(launch_batch_laplace(BL_COUNT, a, l, b->stream));
      HIPCHK(hipMemcpyAsync(b->h_count, b->lcount, sizeof(int), hipMemcpyDeviceToHost, b->stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    if (tm)
      for (int q = 0; q < n; ++q) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, b->lev[q], b->lev[q + 1]));
        b->lstage_ms[slot[q]] += (double)ms;
      }
    return SGP_OK;
  };
  {
    const int st[5] = {BL_K22, BL_PASSZ, BL_MMZ, BL_OBJ0, BL_MM0}, sl[5] = {0, 1, 2, 3, 4};
    const int rc = run(st, sl, 5, true);
    if (rc != SGP_OK) return rc;
  }
  for (int it = 0; it < maxit && *b->h_count > 0; ++it) {
    const int st[4] = {BL_NRA, BL_X2, BL_UPD, BL_MM}, sl[4] = {5, 6, 3, 4};
    const int rc = run(st, sl, 4, true);
    if (rc != SGP_OK) return rc;
  }
  if (!obj_only) {
    const int st[4] = {BL_GA, BL_GM, BL_GB, BL_GF}, sl[4] = {7, 8, 9, 10};
    for (int q = 0; q < 4; ++q) {
      if (tm) HIPCHK(hipEventRecord(b->lev[q], b->stream));
      HIPCHK(launch_batch_laplace(st[q], a, l, b->stream));
    }
    if (tm) HIPCHK(hipEventRecord(b->lev[4], b->stream));
    (void)sl;
  }
  HIPCHK(hipMemcpyAsync(b->h_out, b->out, sizeof(double) * b->B * BATCH_OUT,
                        hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipMemcpyAsync(b->h_lc, b->llc, sizeof(double) * b->B * BATCH_LC, hipMemcpyDeviceToHost,
                        b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (tm && !obj_only)
    for (int q = 0; q < 4; ++q) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, b->lev[q], b->lev[q + 1]));
      b->lstage_ms[7 + q] = (double)ms;
    }
  b->last_ard = ard;
  bool failed = false;
  for (int64_t p = 0; p < b->B; ++p) {
    if (active && !active[p]) continue;
    const double* o = b->h_out + p * BATCH_OUT;
    const int st = (int)o[1];
    status[p] = st;
    nr_iters[p] = (int)b->h_lc[p * BATCH_LC + LC_IT];
    if (st) {
      obj[p] = NAN;
      if (grad)
        for (int q = 0; q < P; ++q) grad[p * ldg + q] = NAN;
      if (!failed)
        set_err("problem %lld: chol(): the leading minor of order %d of %s is not positive definite",
                (long long)p, st > 0 ? st : -st,
                st > 0 ? "Sigma22" : "Sigma22 + t(Sigma12) %*% ZSig12 (or B * Sigma12)");
      failed = true;
      continue;
    }
    obj[p] = o[0];
    if (!obj_only)
      for (int q = 0; q < P; ++q) grad[p * ldg + q] = o[2 + q];
    b->has_state[(size_t)p] = 1;
    b->last_m[(size_t)p] = m[p];
  }
  return SGP_OK;
}

}  // namespace

extern "C" {

int sgp_batch_eval_laplace(sgp_batch* b, int kernel, const double* theta, int64_t ldt,
                           const double* U, const int64_t* uoff, const int64_t* m, double delta,
                           unsigned flags, const unsigned char* active, double* obj, double* grad,
                           int64_t ldg, int* status, double tol, int maxit, int* nr_iters) {
  if (!b) { set_err("sgp_batch_eval_laplace: the sgp_batch is NULL"); return SGP_EINVAL; }
  int cst = batch_check_eval(b->d, b->B, kernel, theta, ldt, U, uoff, m, delta, flags, active,
                             obj, grad, ldg, status);
  if (cst != SGP_OK) return cst;
  cst = batch_check_lap_eval(b->lap_family, tol, maxit, nr_iters);
  if (cst != SGP_OK) return cst;
  return batch_eval_laplace_impl(b, kernel, theta, ldt, U, uoff, m, delta, flags, active, obj,
                                 grad, ldg, status, tol, maxit, nr_iters);
}

int sgp_diag_batch_lap_eval_args(int family, double tol, int maxit, const int* nr_iters) {
  return batch_check_lap_eval(family, tol, maxit, nr_iters);
}

/* The Newton iteration's objective values of problem `prob` in the last sgp_batch_eval_laplace
 * that evaluated it (newtrap_sparseGP's objective_function_values): *count = nr_iters, of which
 * the first min(*count, max_n, SGP_BATCH_LAP_NOBJ) are written to out. */
int sgp_diag_batch_lap_objective_values(sgp_batch* b, int64_t prob, double* out, int max_n,
                                        int* count) {
  if (!b) { set_err("sgp_diag_batch_lap_objective_values: the sgp_batch is NULL"); return SGP_EINVAL; }
  if (b->lap_family < 0 || prob < 0 || prob >= b->B || !out || max_n < 0 || !count) {
    set_err("sgp_diag_batch_lap_objective_values: prob=%lld of %lld, max_n=%d (and "
            "sgp_batch_lap_init first)", (long long)prob, (long long)b->B, max_n);
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  double lc[BATCH_LC];
  HIPCHK(hipMemcpy(lc, b->llc + prob * BATCH_LC, sizeof(lc), hipMemcpyDeviceToHost));
  *count = (int)lc[LC_IT];
  const int n = std::min(std::min(*count, max_n), BATCH_LAP_NOBJ);
  if (n > 0)
    HIPCHK(hipMemcpy(out, b->lobjs + prob * BATCH_LAP_NOBJ, sizeof(double) * n,
                     hipMemcpyDeviceToHost));
  return SGP_OK;
}

/* stage_ms (11 doubles, or NULL): the HIP-event times of the last sgp_batch_eval_laplace: K22's
 * stage, the Z pass, the (K22 + S_Z) stage | summed over the Newton iterations: the objective
 * pass, the C stage, NR's part a, x2 | the gradient's part a, its vector stage, part b, the G22
 * stage (zero under SGP_FLAG_OBJ_ONLY); enable != 0 records them from the next such call on. */
int sgp_diag_batch_laplace_timing(sgp_batch* b, int enable, double* stage_ms) {
  if (!b) { set_err("sgp_diag_batch_laplace_timing: the sgp_batch is NULL"); return SGP_EINVAL; }
  if (stage_ms)
    for (int q = 0; q < 11; ++q) stage_ms[q] = b->ltiming ? b->lstage_ms[q] : 0.0;
  b->ltiming = enable != 0;
  return SGP_OK;
}

int sgp_diag_batch_knot_args(int d, int64_t B, unsigned flags, const unsigned char* active,
                             const double* bounds, const double* grad_knot) {
  return batch_check_knots(d, B, flags, active, bounds, grad_knot);
}

int sgp_batch_eval_vi_knots(sgp_batch* b, int kernel, const double* theta, int64_t ldt,
                            const double* U, const int64_t* uoff, const int64_t* m, double delta,
                            unsigned flags, const unsigned char* active, double* obj, double* grad,
                            int64_t ldg, int* status, const double* bounds, double* grad_knot) {
  if (!b) { set_err("sgp_batch_eval_vi_knots: the sgp_batch is NULL"); return SGP_EINVAL; }
  int cst = batch_check_knots(b->d, b->B, flags, active, bounds, grad_knot);
  if (cst != SGP_OK) return cst;
  cst = batch_check_eval(b->d, b->B, kernel, theta, ldt, U, uoff, m, delta, flags, active, obj,
                         grad, ldg, status);
  if (cst != SGP_OK) return cst;
  return batch_eval_impl(b, 0, kernel, theta, ldt, U, uoff, m, delta, flags, active, obj, grad,
                         ldg, status, bounds, grad_knot);
}

/* stage_ms (2 doubles, or NULL): the HIP-event times of the knot pass and the knot finish of the
 * last sgp_batch_eval_vi_knots; enable != 0 records them from the next such call on. */
int sgp_diag_batch_knot_timing(sgp_batch* b, int enable, double* stage_ms) {
  if (!b) { set_err("sgp_diag_batch_knot_timing: the sgp_batch is NULL"); return SGP_EINVAL; }
  if (stage_ms)
    for (int q = 0; q < 2; ++q) stage_ms[q] = b->ktiming ? (double)b->kstage_ms[q] : 0.0;
  b->ktiming = enable != 0;
  return SGP_OK;
}

int sgp_batch_posterior_u(sgp_batch* b, const double* muu, double* u_mean, double* u_var) {
  if (!b) { set_err("sgp_batch_posterior_u: the sgp_batch is NULL"); return SGP_EINVAL; }
  if (!muu || !u_mean || !u_var) {
    set_err("sgp_batch_posterior_u: muu, u_mean and u_var must not be NULL");
    return SGP_EINVAL;
  }
  if (std::find(b->has_state.begin(), b->has_state.end(), (char)1) == b->has_state.end()) {
    set_err("sgp_batch_posterior_u: no problem of the batch has a successful evaluation");
    return SGP_EINVAL;
  }
  HIPCHK(hipSetDevice(b->device));
  const int64_t rs = BR_T + SGP_BATCH_MMAX;
  std::vector<double> h((size_t)(b->B * rs));
  HIPCHK(launch_batch_post(batch_args(b, b->last_ard, 0), b->res, b->stream));
  HIPCHK(hipMemcpyAsync(h.data(), b->res, sizeof(double) * h.size(), hipMemcpyDeviceToHost,
                        b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  int64_t o1 = 0, o2 = 0;
  for (int64_t p = 0; p < b->B; ++p) {
    const int64_t m = b->has_state[(size_t)p] ? b->last_m[(size_t)p] : 0;   // none: no entries
    const double* r = h.data() + p * rs;
    for (int64_t j = 0; j < m; ++j) u_mean[o1 + j] = muu[o1 + j] + r[BR_T + j];
    for (int64_t j = 0; j < m; ++j)
      for (int64_t i = 0; i < m; ++i) u_var[o2 + i + j * m] = r[i * SGP_BATCH_MMAX + j];
    o1 += m;
    o2 += m * m;
  }
  return SGP_OK;
}

/* stage_ms (4 floats as doubles): HIP-event times of pass 1, the m x m stage, pass 2 and the finish
 * of the last evaluation; enable = 1 records the events from the next evaluation on. */
int sgp_diag_batch_timing(sgp_batch* b, int enable, double* stage_ms) {
  if (!b) { set_err("sgp_diag_batch_timing: the sgp_batch is NULL"); return SGP_EINVAL; }
  if (stage_ms)
    for (int q = 0; q < 4; ++q) stage_ms[q] = b->timing ? (double)b->stage_ms[q] : 0.0;
  b->timing = enable != 0;
  return SGP_OK;
}

// ------------------------------------------------------------------------- batched prediction
// sgp_batch_set_test / sgp_batch_predict (include/sgp.h)
int sgp_diag_batch_test_args(int stage, int d, int64_t B, const double* Xt, int64_t ntest,
                             int64_t ldxt, const double* yt, const double* mut,
                             const int64_t* trow0, const int64_t* tnrow, int have_test,
                             int have_yt, const unsigned char* has_state,
                             const unsigned char* active, const double* pred_mean,
                             const double* pred_var, const double* nlp, const double* stats) {
  return batch_check_test(stage, d, B, Xt, ntest, ldxt, yt, mut, trow0, tnrow, have_test, have_yt,
                          has_state, active, pred_mean, pred_var, nlp, stats);
}

int sgp_diag_batch_test_plan(const int64_t* trow0, const int64_t* tnrow, int64_t B, int64_t cap,
                             int64_t* nseg, int64_t* seg_prob, int64_t* seg_row0,
                             int64_t* seg_rows, int64_t* toff) {
  if (!trow0 || !tnrow || B < 1 || !nseg || cap < 0 ||
      (cap > 0 && (!seg_prob || !seg_row0 || !seg_rows))) {
    set_err("invalid sgp_diag_batch_test_plan arguments");
    return SGP_EINVAL;
  }
  for (int64_t p = 0; p < B; ++p)
    if (tnrow[p] < 0 || trow0[p] < 0) {
      set_err("sgp_diag_batch_test_plan: problem %lld has trow0=%lld, tnrow=%lld", (long long)p,
              (long long)trow0[p], (long long)tnrow[p]);
      return SGP_EINVAL;
    }
  *nseg = batch_test_plan(trow0, tnrow, B, cap, seg_prob, seg_row0, seg_rows, toff);
  return SGP_OK;
}

int sgp_batch_set_test(sgp_batch* b, const double* Xt, int64_t ntest, int64_t ldxt,
                       const double* yt, const double* mut, const int64_t* trow0,
                       const int64_t* tnrow) {
  if (!b) { set_err("sgp_batch_set_test: the sgp_batch is NULL"); return SGP_EINVAL; }
  const int cst = batch_check_test(0, b->d, b->B, Xt, ntest, ldxt, yt, mut, trow0, tnrow, 0, 0,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (cst != SGP_OK) return cst;
  const int64_t B = b->B;
  const int d = b->d;
  std::vector<int64_t> toff((size_t)B + 1);
  const int64_t nseg = batch_test_plan(trow0, tnrow, B, 0, nullptr, nullptr, nullptr, toff.data());
  std::vector<int64_t> sp((size_t)nseg + 1), s0((size_t)nseg + 1), sr((size_t)nseg + 1);
  batch_test_plan(trow0, tnrow, B, nseg, sp.data(), s0.data(), sr.data(), nullptr);
  std::vector<int> spi((size_t)nseg + 1), sri((size_t)nseg + 1), ps((size_t)(2 * B), 0);
  std::vector<int64_t> so((size_t)nseg + 1);
  for (int64_t k = 0; k < nseg; ++k) {
    const int64_t p = sp[(size_t)k];
    spi[(size_t)k] = (int)p;
    sri[(size_t)k] = (int)sr[(size_t)k];
    so[(size_t)k] = toff[(size_t)p] + (s0[(size_t)k] - trow0[p]);
    if (ps[(size_t)(2 * p + 1)]++ == 0) ps[(size_t)(2 * p)] = (int)k;
  }
  const int64_t tot = toff[(size_t)B], nout = 3 * std::max<int64_t>(tot, 1) + 4 * B;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  batch_free_test(b);
  for (hipEvent_t& e : b->pev)
    if (!e) HIPCHK(hipEventCreate(&e));
  b->ntest = ntest;
  b->ntseg = nseg;
  b->ttot = tot;
  b->tnrow.assign(tnrow, tnrow + B);
  b->toff = toff;
  HIPCHK(hipMalloc(&b->Xt, sizeof(double) * ntest * d));
  HIPCHK(hipMalloc(&b->mut, sizeof(double) * ntest));
  if (yt) HIPCHK(hipMalloc(&b->yt, sizeof(double) * ntest));
  HIPCHK(hipMalloc(&b->pw, sizeof(double) * B * BATCH_PW));
  HIPCHK(hipMalloc(&b->prec, sizeof(double) * (nseg + 1) * BATCH_PREC));
  HIPCHK(hipMalloc(&b->pout, sizeof(double) * nout));
  HIPCHK(hipMalloc(&b->act, sizeof(int) * B));
  HIPCHK(hipMalloc(&b->tseg_prob, sizeof(int) * (nseg + 1)));
  HIPCHK(hipMalloc(&b->tseg_rows, sizeof(int) * (nseg + 1)));
  HIPCHK(hipMalloc(&b->tprob_seg, sizeof(int) * 2 * B));
  HIPCHK(hipMalloc(&b->tseg_row0, sizeof(int64_t) * (nseg + 1)));
  HIPCHK(hipMalloc(&b->tseg_out, sizeof(int64_t) * (nseg + 1)));
  HIPCHK(hipHostMalloc(&b->h_pout, sizeof(double) * nout));
  HIPCHK(hipHostMalloc(&b->h_act, sizeof(int) * B));
  HIPCHK(hipMemsetAsync(b->pw, 0, sizeof(double) * B * BATCH_PW, b->stream));
  HIPCHK(hipMemsetAsync(b->pout, 0, sizeof(double) * nout, b->stream));
  HIPCHK(hipMemcpy2DAsync(b->Xt, sizeof(double) * ntest, Xt, sizeof(double) * ldxt,
                          sizeof(double) * ntest, (size_t)d, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->mut, mut, sizeof(double) * ntest, hipMemcpyHostToDevice, b->stream));
  if (yt) HIPCHK(hipMemcpyAsync(b->yt, yt, sizeof(double) * ntest, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->tseg_prob, spi.data(), sizeof(int) * (nseg + 1), hipMemcpyHostToDevice,
                        b->stream));
  HIPCHK(hipMemcpyAsync(b->tseg_rows, sri.data(), sizeof(int) * (nseg + 1), hipMemcpyHostToDevice,
                        b->stream));
  HIPCHK(hipMemcpyAsync(b->tprob_seg, ps.data(), sizeof(int) * 2 * B, hipMemcpyHostToDevice,
                        b->stream));
  HIPCHK(hipMemcpyAsync(b->tseg_row0, s0.data(), sizeof(int64_t) * (nseg + 1),
                        hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->tseg_out, so.data(), sizeof(int64_t) * (nseg + 1),
                        hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  b->have_test = true;
  b->have_yt = yt != nullptr;
  return SGP_OK;
}

int sgp_batch_predict(sgp_batch* b, const unsigned char* active, double* pred_mean,
                      double* pred_var, double* nlp, double* stats) {
  if (!b) { set_err("sgp_batch_predict: the sgp_batch is NULL"); return SGP_EINVAL; }
  const int cst = batch_check_test(
      1, b->d, b->B, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, b->have_test, b->have_yt,
      reinterpret_cast<const unsigned char*>(b->has_state.data()), active, pred_mean, pred_var,
      nlp, stats);
  if (cst != SGP_OK) return cst;
  const int64_t B = b->B, tot = b->ttot, cap = std::max<int64_t>(tot, 1);
  bool any = false;
  for (int64_t p = 0; p < B; ++p) {
    b->h_act[p] = (!active || active[p]) ? 1 : 0;
    any = any || b->h_act[p];
  }
  if (!any) return SGP_OK;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(b->act, b->h_act, sizeof(int) * B, hipMemcpyHostToDevice, b->stream));
  BatchPredArgs p;
  p.Xt = b->Xt; p.yt = b->yt; p.mut = b->mut; p.ldxt = b->ntest;
  p.act = b->act;
  p.seg_prob = b->tseg_prob; p.seg_row0 = b->tseg_row0; p.seg_rows = b->tseg_rows;
  p.seg_out = b->tseg_out; p.prob_seg = b->tprob_seg;
  p.nseg = (int)b->ntseg; p.score = nlp ? 1 : 0;
  p.pw = b->pw; p.rec = b->prec;
  p.pm = b->pout; p.pv = b->pout + cap; p.nlp = b->pout + 2 * cap; p.stats = b->pout + 3 * cap;
  HIPCHK(launch_batch_predict(batch_args(b, b->last_ard, 0), p, b->stream,
                              b->ptiming ? b->pev : nullptr));
  const int64_t ncopy = nlp ? 3 * cap + 4 * B : 2 * cap;
  HIPCHK(hipMemcpyAsync(b->h_pout, b->pout, sizeof(double) * ncopy, hipMemcpyDeviceToHost,
                        b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (b->ptiming)
    for (int q = 0; q < 3; ++q)
      HIPCHK(hipEventElapsedTime(&b->pstage_ms[q], b->pev[q], b->pev[q + 1]));
  for (int64_t q = 0; q < B; ++q) {
    if (!b->h_act[q]) continue;
    const int64_t o = b->toff[(size_t)q], nr = b->tnrow[(size_t)q];
    if (nr == 0) continue;   // no segment: nothing is written
    std::copy(b->h_pout + o, b->h_pout + o + nr, pred_mean + o);
    std::copy(b->h_pout + cap + o, b->h_pout + cap + o + nr, pred_var + o);
    if (nlp) {
      std::copy(b->h_pout + 2 * cap + o, b->h_pout + 2 * cap + o + nr, nlp + o);
      std::copy(b->h_pout + 3 * cap + 4 * q, b->h_pout + 3 * cap + 4 * q + 4, stats + 4 * q);
    }
  }
  return SGP_OK;
}

/* stage_ms (3 doubles, or NULL): HIP-event times of the m x m stage, the row pass and the finish
 * of the last sgp_batch_predict; enable != 0 records them from the next call on. */
int sgp_diag_batch_predict_timing(sgp_batch* b, int enable, double* stage_ms) {
  if (!b) { set_err("sgp_diag_batch_predict_timing: the sgp_batch is NULL"); return SGP_EINVAL; }
  if (stage_ms)
    for (int q = 0; q < 3; ++q) stage_ms[q] = b->ptiming ? (double)b->pstage_ms[q] : 0.0;
  b->ptiming = enable != 0;
  return SGP_OK;
}

}  // extern "C"
