// sgp_syrk_plan.h -- row-chunk plans of S = K^T K (k_mfma.hip), HIP-free.
//
// Host code decides how the lower 64-blocks of S and the n_pad / 16 row steps are dealt to the
// workgroups of one residency round; tests/syrk_plan/plan_driver.cc checks the plans without a
// GPU.  The functions marked SGP_HD are also what the kernels run to find their own work, so
// the tested partition is the executed one.
//
//   syrk_plan, syrk_plan_blk   equal row chunks over equal workgroups (the packed plan: 34
//                              workgroups per chunk at m = 1024, every diagonal 64-block
//                              computed in full: 16 fragments where 10 are needed)
//   syrk_plan_balanced         the work-balanced plan of the unweighted S (VI): every workgroup
//                              the same modelled MFMA count, no strictly-upper fragment of a
//                              diagonal 64-block computed
//
// Work-balanced plan.  Unit: one MFMA slot of a wave (a 16-row step of a strictly-lower
// 128-tile costs 64 per wave, one of a diagonal 128-tile `wd`: 36 issued, SGP_SDT_W modelled).
//   * The noff = nb (nb - 1) / 2 strictly-lower 128-tile groups run in B equal row bands (the
//     first N % B of them one step longer); the noff workgroups of one band have consecutive ids, so
//     after xcd_remap they sit together on one XCD and walk the same rows in step -- each
//     128-column panel of K, read by nb - 1 of them, comes from HBM once per band.
//   * A diagonal tile reads its own panel only (A = B) and shares it with nobody, so its rows
//     are the filler.  The tail of tile t is cut into pieces of e steps that the off-diagonal
//     workgroups run as a second segment after their band chunk (e + 1 steps behind a band of
//     the shorter kind when wd <= 64; every piece full, none across a tile boundary).  The tiles' remaining heads, afirst[t + 1] - afirst[t]
//     steps each, form one axis of A steps that the other D = slots - B noff workgroups take in
//     runs of Ld = ceil(A / D); a run that meets a tile boundary is that workgroup's two
//     segments (every head is at least Ld long, so never three).
//   * Makespan: max(64 ceil(N / B) + c0 + wd e + c0, wd Ld + 2 c0), c0 a segment's start-up and
//     flush.  e is the step count at which the two sides cross, or the next one above it that
//     leaves every workgroup within one off-diagonal step of the mean; B the band count with
//     the smallest such makespan (the smallest B within 0.1 % of it: fewer partial slabs).
// A workgroup runs at most two segments and writes each segment's blocks to a partial slab of
// its own: band s's group g to off-diagonal partial s of its 4 blocks, a diagonal segment to
// one entry of its tile's ordered list (3 blocks; the head's runs first, then the pieces, so
// ascending rows).  k_syrk_reduce_bal sums every block's partials in that order: no atomics.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SGP_HD __host__ __device__ inline
#else
#define SGP_HD inline
#endif

namespace sgp_plan {

constexpr int kStep = 16;      // rows per k-step (BK)
constexpr int kTile = 128;     // columns per K panel (T128)
constexpr int kMaxNb = 31;     // nb >= 32 (m > 3968): the strictly-lower groups alone fill a round

// bijective XCD-aware remap: work items that share operands get consecutive ids on one XCD
SGP_HD int64_t xcd_remap(int64_t orig, int64_t nwg) {
  const int64_t x = orig % 8, q = nwg / 8, r = nwg % 8;
  const int64_t base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return base + orig / 8;
}

struct SyrkPlan {
  int nb, T, splits;
  int64_t chunk;
};

inline SyrkPlan syrk_plan(int64_t n_pad, int64_t mp, int64_t kSlots = 512) {
  // One resident "round" = 256 CUs x 2 workgroups (216 VGPRs, 74 KB LDS each).  Pick the
  // split count so splits * T fills an integer number of rounds as fully as possible.
  SyrkPlan p;
  p.nb = (int)(mp / kTile);
  p.T = p.nb * (p.nb + 1) / 2;
  const int64_t max_splits = n_pad / kStep > 0 ? n_pad / kStep : 1;
  int64_t best = 1;
  double best_fill = 0.0;
  for (int64_t rounds = 1; rounds <= 4; ++rounds) {
    int64_t sp = rounds * kSlots / p.T;
    if (sp < 1) sp = 1;
    if (sp > max_splits) sp = max_splits;
    const double fill = (double)(sp * p.T) / (double)(((sp * p.T + kSlots - 1) / kSlots) * kSlots);
    if (fill > best_fill + 1e-9) { best_fill = fill; best = sp; }
    if (best_fill >= 0.95) break;
  }
  int64_t chunk = (n_pad + best - 1) / best;
  chunk = (chunk + kStep - 1) / kStep * kStep;
  p.chunk = chunk;
  p.splits = (int)((n_pad + chunk - 1) / chunk);
  return p;
}

// k_syrk_blk: the same split rule over its packed groups (T = workgroups per row chunk)
inline SyrkPlan syrk_plan_blk(int64_t n_pad, int64_t mp, int64_t kSlots = 512) {
  SyrkPlan p = syrk_plan(n_pad, mp, kSlots);   // nb, and a starting point
  const int nb = p.nb;
  const int groups = nb * (nb - 1) / 2 + (3 * nb + 3) / 4;
  const int64_t max_splits = n_pad / kStep > 0 ? n_pad / kStep : 1;
  int64_t best = 1;
  double best_fill = 0.0;
  for (int64_t rounds = 1; rounds <= 4; ++rounds) {
    int64_t sp = rounds * kSlots / groups;
    if (sp < 1) sp = 1;
    if (sp > max_splits) sp = max_splits;
    const double fill = (double)(sp * groups) /
                        (double)(((sp * groups + kSlots - 1) / kSlots) * kSlots);
    if (fill > best_fill + 1e-9) { best_fill = fill; best = sp; }
    if (best_fill >= 0.95) break;
  }
  int64_t chunk = (n_pad + best - 1) / best;
  chunk = (chunk + kStep - 1) / kStep * kStep;
  p.T = groups;
  p.chunk = chunk;
  p.splits = (int)((n_pad + chunk - 1) / chunk);
  return p;
}

// the packed plan's makespan in MFMA slots: one or more rounds of equal workgroups
inline double syrk_packed_makespan(int64_t n_pad, int64_t mp, int64_t kSlots, double c0) {
  const SyrkPlan q = syrk_plan_blk(n_pad, mp, kSlots);
  const int64_t rounds = ((int64_t)q.splits * q.T + kSlots - 1) / kSlots;
  return (64.0 * (double)(q.chunk / kStep) + c0) * (double)rounds;
}

// strictly-lower 128-tile group gi = a (a - 1) / 2 + b, a > b: K panels a (rows) and b (columns)
SGP_HD void syrk_off_panels(int gi, int& a, int& b) {
  int x = 1;
  while ((x + 1) * x / 2 <= gi) ++x;
  a = x;
  b = gi - x * (x - 1) / 2;
}

enum { SEG_NONE = 0, SEG_OFF = 1, SEG_DIAG = 2 };

struct SyrkSeg {
  int kind;        // SEG_*
  int id;          // SEG_OFF: group gi; SEG_DIAG: diagonal tile t
  int64_t step0;   // first 16-row step
  int nsteps;      // > 0
  int slab;        // SEG_OFF: partial (band) index of the group's 4 blocks; SEG_DIAG: entry of
                   // the diagonal partial list (3 blocks each)
};

struct SyrkBalPlan {
  int on;                  // 0: declined
  int nb, noff;
  int B;                   // row bands of the strictly-lower groups
  int M;                   // B * noff: plan ids [0, M) (launch id -> plan id: xcd_remap over M)
  int nwg;                 // M + diagonal-tile workgroups (plan id = launch id from M on)
  int Ld;                  // steps per diagonal-tile workgroup
  int e;                   // steps per second segment
  int xfirst;              // plan ids from here on (the shorter bands) take e + 1
  int64_t N;               // n_pad / 16
  int64_t afirst[kMaxNb + 1];  // tile t's head on the diagonal-tile workgroups' axis
  int dseg[kMaxNb];        // segments of diagonal-tile workgroups in tile t
  int pfirst[kMaxNb + 1];  // first plan id (< M) whose second segment is a piece of tile t
  int sfirst[kMaxNb + 1];  // tile t's first entry in the diagonal partial list
  double T_bal, T_pack;    // modelled makespans, MFMA slots
};

SGP_HD int64_t syrk_bp_band(const SyrkBalPlan& p, int s) {
  const int64_t q = p.N / p.B, r = p.N % p.B;
  return s * q + (s < r ? s : r);
}

// the (at most two) segments of plan id wg
SGP_HD void syrk_bp_segments(const SyrkBalPlan& p, int wg, SyrkSeg& s0, SyrkSeg& s1) {
  s0 = s1 = SyrkSeg{SEG_NONE, 0, 0, 0, 0};
  if (wg < p.M) {
    const int band = wg / p.noff;
    s0.kind = SEG_OFF;
    s0.id = wg % p.noff;
    s0.step0 = syrk_bp_band(p, band);
    s0.nsteps = (int)(syrk_bp_band(p, band + 1) - s0.step0);
    s0.slab = band;
    if (wg >= p.pfirst[p.nb]) return;
    int t = 0;
    while (wg >= p.pfirst[t + 1]) ++t;
    const int i = wg - p.pfirst[t];
    s1.kind = SEG_DIAG;
    s1.id = t;
    const int x0 = p.pfirst[t] > p.xfirst ? p.pfirst[t] : p.xfirst;
    s1.step0 = (p.afirst[t + 1] - p.afirst[t]) + (int64_t)i * p.e + (wg > x0 ? wg - x0 : 0);
    s1.nsteps = p.e + (wg >= p.xfirst ? 1 : 0);
    s1.slab = p.sfirst[t] + p.dseg[t] + i;
    return;
  }
  const int j = wg - p.M;
  const int64_t A = p.afirst[p.nb], x0 = (int64_t)j * p.Ld;
  const int64_t x1 = x0 + p.Ld < A ? x0 + p.Ld : A;
  int t = 0;
  while (x0 >= p.afirst[t + 1]) ++t;   // skips tiles without a head
  const int64_t end0 = x1 < p.afirst[t + 1] ? x1 : p.afirst[t + 1];
  s0.kind = SEG_DIAG;
  s0.id = t;
  s0.step0 = x0 - p.afirst[t];
  s0.nsteps = (int)(end0 - x0);
  s0.slab = p.sfirst[t] + (j - (int)(p.afirst[t] / p.Ld));
  if (x1 > end0) {   // into the next tile's head, whose first run this is
    s1.kind = SEG_DIAG;
    s1.id = t + 1;
    s1.step0 = 0;
    s1.nsteps = (int)(x1 - end0);
    s1.slab = p.sfirst[t + 1];
  }
}

// a segment's modelled cost
SGP_HD double syrk_bp_cost(const SyrkSeg& s, double wd, double c0) {
  if (s.kind == SEG_NONE) return 0.0;
  return (s.kind == SEG_OFF ? 64.0 : wd) * (double)s.nsteps + c0;
}

// doubles of the two slab regions: off-diagonal partials [band][group][4][4096], then the
// diagonal partial list [entry][3][4096]
inline int64_t syrk_bp_off_doubles(const SyrkBalPlan& p) {
  return (int64_t)p.B * p.noff * 4 * 4096;
}
inline int64_t syrk_bp_slab_doubles(const SyrkBalPlan& p) {
  return syrk_bp_off_doubles(p) + (int64_t)p.sfirst[p.nb] * 3 * 4096;
}

namespace detail {
struct Deal {
  bool ok;
  int Ld, e;
  int64_t A;
  double T;
};
// first plan id behind a band of the shorter kind (M: none, or no extra step for them)
inline int syrk_bp_xfirst(int64_t N, int nb, int B, double wd) {
  const int noff = nb * (nb - 1) / 2;
  return N % B == 0 || wd > 64.0 ? B * noff : (int)(N % B) * noff;
}
// pieces of tile t: the M off-diagonal workgroups dealt evenly; steps: what they take together
inline int64_t syrk_bp_pieces(int nb, int M, int xfirst, int e, int t, int64_t* steps) {
  *steps = 0;
  if (e <= 0) return 0;
  const int64_t q = M / nb, r = M % nb, k = q + (t < r ? 1 : 0);
  const int64_t first = t * q + (t < r ? t : r), x0 = first > xfirst ? first : xfirst;
  *steps = k * e + (first + k > x0 ? first + k - x0 : 0);
  return k;
}
// B bands, D diagonal-tile workgroups, second segments of e steps
inline Deal syrk_bp_deal(int64_t N, int nb, int B, int D, double wd, double c0, int e) {
  const int M = B * (nb * (nb - 1) / 2);
  Deal d{false, 0, e, 0, 0.0};
  const int xfirst = syrk_bp_xfirst(N, nb, B, wd);
  int64_t K = 0, amin = N;
  d.A = 0;
  for (int t = 0; t < nb; ++t) {
    int64_t st;
    K += syrk_bp_pieces(nb, M, xfirst, e, t, &st);
    if (N - st < amin) amin = N - st;
    d.A += N - st;
  }
  if (amin < 1) return d;
  const int64_t Ld = (d.A + D - 1) / D;
  d.Ld = (int)Ld;
  const double f = 64.0 * (double)((N + B - 1) / B) + c0 + (K > 0 ? wd * (double)e + c0 : 0.0);
  const double g = wd * (double)Ld + 2.0 * c0;
  d.T = f > g ? f : g;
  d.ok = Ld >= 1 && Ld <= amin && (e == 0 || K > 0);
  // where the band side sets the makespan: as few diagonal-tile workgroups as stay under it
  // (the slots left over are free for what runs beside the SYRK)
  int64_t fill = (int64_t)((d.T - 2.0 * c0) / wd);
  if (fill > amin) fill = amin;
  if (d.ok && fill > Ld) d.Ld = (int)fill;
  return d;
}
// the best e for B bands: the band side grows with e, the diagonal side shrinks
inline Deal syrk_bp_best(int64_t N, int nb, int B, int D, double wd, double c0) {
  Deal best = syrk_bp_deal(N, nb, B, D, wd, c0, 0);
  int64_t lo = 1, hi = N / 2;
  while (lo < hi) {   // the smallest e from which the band side is the longer one
    const int64_t mid = lo + (hi - lo) / 2;
    const Deal d = syrk_bp_deal(N, nb, B, D, wd, c0, (int)mid);
    const double g = wd * (double)((d.A + D - 1) / D) + 2.0 * c0;
    if (d.T > g || !d.ok) hi = mid;
    else lo = mid + 1;
  }
  for (int64_t e = lo > 2 ? lo - 2 : 1; e <= lo + 1 && e <= N / 2; ++e) {
    const Deal d = syrk_bp_deal(N, nb, B, D, wd, c0, (int)e);
    if (d.ok && (!best.ok || d.T < best.T)) best = d;
  }
  return best;
}
}  // namespace detail

// the plan struct of B bands dealt as d
inline SyrkBalPlan syrk_bp_build(int64_t N, int nb, int B, const detail::Deal& d, double wd) {
  SyrkBalPlan p{};
  p.nb = nb;
  p.noff = nb * (nb - 1) / 2;
  p.B = B;
  p.M = B * p.noff;
  p.N = N;
  p.Ld = d.Ld;
  p.e = d.e;
  p.xfirst = detail::syrk_bp_xfirst(N, nb, B, wd);
  p.T_bal = d.T;
  p.afirst[0] = 0;
  p.pfirst[0] = 0;
  p.sfirst[0] = 0;
  for (int t = 0; t < nb; ++t) {
    int64_t st;
    const int64_t k = detail::syrk_bp_pieces(nb, p.M, p.xfirst, p.e, t, &st), a = N - st;
    p.afirst[t + 1] = p.afirst[t] + a;
    p.dseg[t] = a > 0 ? (int)((p.afirst[t + 1] - 1) / p.Ld - p.afirst[t] / p.Ld + 1) : 0;
    p.pfirst[t + 1] = p.pfirst[t] + (int)k;
    p.sfirst[t + 1] = p.sfirst[t] + p.dseg[t] + (int)k;
  }
  p.nwg = p.M + (int)((p.afirst[nb] + p.Ld - 1) / p.Ld);
  return p;
}

// largest and mean modelled cost over the plan's workgroups
inline void syrk_bp_spread(const SyrkBalPlan& p, double wd, double c0, double* mx, double* mean) {
  double sum = 0.0;
  *mx = 0.0;
  for (int wg = 0; wg < p.nwg; ++wg) {
    SyrkSeg s0, s1;
    syrk_bp_segments(p, wg, s0, s1);
    const double c = syrk_bp_cost(s0, wd, c0) + syrk_bp_cost(s1, wd, c0);
    sum += c;
    if (c > *mx) *mx = c;
  }
  *mean = p.nwg > 0 ? sum / (double)p.nwg : 0.0;
}
// balanced: no workgroup above the mean by more than one off-diagonal step
inline bool syrk_bp_balanced(const SyrkBalPlan& p, double wd, double c0) {
  double mx, mean;
  syrk_bp_spread(p, wd, c0, &mx, &mean);
  return mx <= mean + 64.0;
}

// slots: workgroups of one residency round to plan for; wd: a diagonal-tile wave-step's cost;
// c0: start-up and flush of one segment.  Declines (on = 0) for nb < 3, nb > kMaxNb, and when
// the makespan is not more than 2 % under the packed plan's.  With little work the grid shrinks
// (B <= N bands, ceil(A / Ld) diagonal-tile workgroups): no segment is empty.
//
// Selection: per band count the deal of smallest makespan that is balanced, looked for among
// the piece lengths from the crossing of the two sides upwards while the makespan stays within
// 0.5 % of the best of all deals.  (Where the band chunk alone sets the makespan the cheapest
// deal can leave its slots unevenly filled -- nb = 12, n = 1e6: 7 bands, chunk 571528 against a
// mean of 571334 over 512 workgroups; second segments of 25 steps on 511 workgroups level them
// at 572486, 0.17 % later in the model and one slot fewer.)  Then the longest bands within 0.1 %
// of the best balanced makespan; without any balanced deal, within 0.1 % of the best of all.
inline SyrkBalPlan syrk_plan_balanced(int64_t n_pad, int64_t mp, int slots, double wd,
                                      double c0 = 8.0) {
  SyrkBalPlan none{};
  none.T_pack = mp >= kTile && n_pad >= kStep ? syrk_packed_makespan(n_pad, mp, 512, c0) : 0.0;
  const int nb = (int)(mp / kTile);
  const int64_t N = n_pad / kStep;
  if (nb < 3 || nb > kMaxNb || N < 1 || wd <= 0.0 || c0 < 0.0) return none;
  const int noff = nb * (nb - 1) / 2;
  // at least one diagonal-tile workgroup per tile, so that a run is no longer than a tile
  int Bmax = (slots - nb) / noff;
  if ((int64_t)Bmax > N) Bmax = (int)N;
  if (slots < nb || Bmax < 1) return none;
  double Tmin = 0.0;
  for (int b = 1; b <= Bmax; ++b) {
    const detail::Deal d = detail::syrk_bp_best(N, nb, b, slots - b * noff, wd, c0);
    if (d.ok && (Tmin == 0.0 || d.T < Tmin)) Tmin = d.T;
  }
  if (Tmin == 0.0) return none;
  // per band count: its cheapest balanced deal within 0.5 % of Tmin
  SyrkBalPlan bal[512 / 3 + 1];
  double Tbb = 0.0;
  for (int b = 1; b <= Bmax && b <= 512 / 3; ++b) {
    bal[b].nwg = 0;
    const detail::Deal d0 = detail::syrk_bp_best(N, nb, b, slots - b * noff, wd, c0);
    if (!d0.ok || d0.T > 1.005 * Tmin) continue;
    for (int64_t e = d0.e > 2 ? d0.e - 2 : 0; e <= N / 2; ++e) {
      const detail::Deal d = detail::syrk_bp_deal(N, nb, b, slots - b * noff, wd, c0, (int)e);
      if (e > d0.e && (!d.ok || d.T > 1.005 * Tmin)) break;
      if (!d.ok || d.T > 1.005 * Tmin || (bal[b].nwg > 0 && d.T >= bal[b].T_bal)) continue;
      const SyrkBalPlan q = syrk_bp_build(N, nb, b, d, wd);
      if (syrk_bp_balanced(q, wd, c0)) bal[b] = q;
    }
    if (bal[b].nwg > 0 && (Tbb == 0.0 || bal[b].T_bal < Tbb)) Tbb = bal[b].T_bal;
  }
  SyrkBalPlan p{};
  for (int b = 1; b <= Bmax && b <= 512 / 3 && p.nwg == 0; ++b) {
    if (Tbb > 0.0) {
      if (bal[b].nwg > 0 && bal[b].T_bal <= 1.001 * Tbb) p = bal[b];
    } else {
      const detail::Deal d = detail::syrk_bp_best(N, nb, b, slots - b * noff, wd, c0);
      if (d.ok && d.T <= 1.001 * Tmin) p = syrk_bp_build(N, nb, b, d, wd);
    }
  }
  if (p.nwg == 0) return none;
  p.T_pack = none.T_pack;
  p.on = p.T_bal < 0.98 * p.T_pack ? 1 : 0;
  return p;
}

}  // namespace sgp_plan
