// Stand-alone checks of sparsergps_amd/csrc/sgp_syrk_plan.h (tests/test_syrk_plan.py builds
// and runs this; no GPU, no HIP).  Every failed check prints a line and the program exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sparsergps_amd/csrc/sgp_syrk_plan.h"

using namespace sgp_plan;

static int g_fail = 0, g_unbalanced = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++g_fail <= 40) {                               \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
    }                                                     \
  } while (0)

static const int kSlots = 512;
static const double kWd = 38.0, kC0 = 8.0;

static bool same_seg(const SyrkSeg& a, const SyrkSeg& b) {
  if (a.kind != b.kind) return false;
  if (a.kind == SEG_NONE) return true;
  return a.id == b.id && a.step0 == b.step0 && a.nsteps == b.nsteps && a.slab == b.slab;
}

static void check_plan(int nb, int64_t n_pad) {
  const int64_t mp = (int64_t)nb * kTile;
  const SyrkBalPlan p = syrk_plan_balanced(n_pad, mp, kSlots, kWd, kC0);
  const SyrkBalPlan p2 = syrk_plan_balanced(n_pad, mp, kSlots, kWd, kC0);
  std::printf("nb %2d n_pad %8lld: on %d B %3d nwg %3d Ld %5d e %4d T_bal %.0f T_pack %.0f ratio %.4f\n",
              nb, (long long)n_pad, p.on, p.B, p.nwg, p.Ld, p.e, p.T_bal, p.T_pack,
              p.T_pack > 0 ? p.T_bal / p.T_pack : 0.0);
  CHECK(p.nwg > 0, "no plan at nb %d n_pad %lld", nb, (long long)n_pad);
  if (p.nwg <= 0) return;
  const int64_t N = n_pad / kStep;
  const int nb64 = 2 * nb, nblk = nb64 * (nb64 + 1) / 2, noff = nb * (nb - 1) / 2;
  // a pure function of its arguments
  CHECK(p.on == p2.on && p.B == p2.B && p.nwg == p2.nwg && p.Ld == p2.Ld && p.e == p2.e &&
            p.T_bal == p2.T_bal && p.T_pack == p2.T_pack, "plan differs between two calls");
  CHECK(p.on == (p.T_bal < 0.98 * p.T_pack ? 1 : 0), "selection rule");
  CHECK(p.nb == nb && p.noff == noff && p.N == N && p.M == p.B * noff, "header fields");
  CHECK(p.nwg <= kSlots && p.nwg >= p.M, "grid %d", p.nwg);

  std::vector<unsigned char> cover((size_t)nblk * (size_t)N, 0);
  auto mark = [&](int rp, int cp, const SyrkSeg& s) {
    CHECK(rp >= cp && rp < nb64, "block (%d, %d)", rp, cp);
    unsigned char* c = &cover[((size_t)rp * (rp + 1) / 2 + cp) * (size_t)N];
    for (int64_t k = s.step0; k < s.step0 + s.nsteps; ++k) ++c[k];
  };
  std::vector<double> cost(p.nwg, 0.0);
  std::vector<int> dslab_used(p.sfirst[nb], 0);
  std::vector<int64_t> dslab_step(p.sfirst[nb], -1);
  std::vector<int> oslab_used((size_t)p.B * noff, 0);
  std::vector<int64_t> band_lo(p.B, -1), band_n(p.B, -1);
  int64_t slab_need = 0;
  for (int wg = 0; wg < p.nwg; ++wg) {
    SyrkSeg s[2], r[2];
    syrk_bp_segments(p, wg, s[0], s[1]);
    syrk_bp_segments(p2, wg, r[0], r[1]);
    CHECK(same_seg(s[0], r[0]) && same_seg(s[1], r[1]), "segments differ between two calls");
    // at most two segments, the first never empty, none of zero length
    CHECK(s[0].kind != SEG_NONE, "workgroup %d has no work", wg);
    CHECK(s[0].kind == (wg < p.M ? SEG_OFF : SEG_DIAG), "workgroup %d kinds %d %d", wg,
          s[0].kind, s[1].kind);
    CHECK(s[1].kind == SEG_NONE || s[1].kind == SEG_DIAG, "second segment kind");
    for (int q = 0; q < 2; ++q) {
      const SyrkSeg& g = s[q];
      if (g.kind == SEG_NONE) continue;
      CHECK(g.nsteps > 0, "workgroup %d segment %d has %d steps", wg, q, g.nsteps);
      CHECK(g.step0 >= 0 && g.step0 + g.nsteps <= N, "rows [%lld, +%d) of %lld",
            (long long)g.step0, g.nsteps, (long long)N);
      if (g.nsteps <= 0 || g.step0 < 0 || g.step0 + g.nsteps > N) continue;
      cost[wg] += syrk_bp_cost(g, kWd, kC0);
      if (g.kind == SEG_OFF) {
        int a, b;
        syrk_off_panels(g.id, a, b);
        // a strictly-lower 128-tile: none of its 4 blocks is a diagonal 64-block
        CHECK(g.id >= 0 && g.id < noff && a > b && a < nb && b >= 0 &&
                  a * (a - 1) / 2 + b == g.id, "group %d -> (%d, %d)", g.id, a, b);
        for (int wr = 0; wr < 2; ++wr)
          for (int wc = 0; wc < 2; ++wc) mark(2 * a + wr, 2 * b + wc, g);
        const int band = wg / noff;
        CHECK(g.slab == band && wg % noff == g.id, "band / group of plan id %d", wg);
        // the groups of one band cover identical rows
        if (band_lo[band] < 0) { band_lo[band] = g.step0; band_n[band] = g.nsteps; }
        CHECK(band_lo[band] == g.step0 && band_n[band] == g.nsteps, "band %d rows differ", band);
        ++oslab_used[(size_t)g.slab * noff + g.id];
        slab_need = std::max<int64_t>(slab_need, ((int64_t)g.slab * noff + g.id + 1) * 4 * 4096);
      } else {
        const int t = g.id;
        CHECK(t >= 0 && t < nb, "tile %d", t);
        // the diagonal-tile body issues the 36 fragments (R, c), c <= R, of the 8 x 8 fragment
        // tile: inside a diagonal 64-block (R / 4 == c / 4) never a strictly-upper one
        for (int R = 0; R < 8; ++R)
          for (int c = 0; c <= R; ++c)
            CHECK(!(R / 4 == c / 4 && R % 4 < c % 4), "upper fragment (%d, %d)", R, c);
        mark(2 * t, 2 * t, g);
        mark(2 * t + 1, 2 * t, g);
        mark(2 * t + 1, 2 * t + 1, g);
        CHECK(g.slab >= p.sfirst[t] && g.slab < p.sfirst[t + 1], "tile %d entry %d", t, g.slab);
        if (g.slab >= 0 && g.slab < p.sfirst[nb]) {
          ++dslab_used[g.slab];
          dslab_step[g.slab] = g.step0;
        }
        slab_need = std::max<int64_t>(
            slab_need, syrk_bp_off_doubles(p) + ((int64_t)g.slab + 1) * 3 * 4096);
      }
    }
  }
  // every (lower 64-block, step) exactly once
  size_t bad = 0;
  for (size_t i = 0; i < cover.size(); ++i) bad += cover[i] != 1;
  CHECK(bad == 0, "%zu (block, step) cells not covered exactly once", bad);
  // every partial slab written by exactly one segment; a tile's list ascends in rows
  for (size_t i = 0; i < oslab_used.size(); ++i) CHECK(oslab_used[i] == 1, "off partial %zu", i);
  for (size_t i = 0; i < dslab_used.size(); ++i) CHECK(dslab_used[i] == 1, "diag partial %zu", i);
  for (int t = 0; t < nb; ++t)
    for (int i = p.sfirst[t] + 1; i < p.sfirst[t + 1]; ++i)
      CHECK(dslab_step[i] > dslab_step[i - 1], "tile %d list not in row order at %d", t, i);
  for (int b = 1; b < p.B; ++b)
    CHECK(band_lo[b] == band_lo[b - 1] + band_n[b - 1], "bands not consecutive at %d", b);
  CHECK(slab_need <= syrk_bp_slab_doubles(p), "slab need %lld > %lld", (long long)slab_need,
        (long long)syrk_bp_slab_doubles(p));
  // balance: nobody above the mean by more than one off-diagonal step; the model's makespan
  // bounds every workgroup
  double sum = 0.0, mx = 0.0;
  for (double c : cost) { sum += c; mx = std::max(mx, c); }
  const double mean = sum / (double)p.nwg;
  if (!(mx <= mean + 64.0)) {   // reported apart: tests/test_syrk_plan.py::test_plan_balance
    ++g_unbalanced;
    std::printf("UNBALANCED nb %d n_pad %lld: max cost %.0f, mean %.1f, mean + 64 = %.1f\n", nb,
                (long long)n_pad, mx, mean, mean + 64.0);
  }
  CHECK(mx <= p.T_bal, "max cost %.0f above the modelled makespan %.0f", mx, p.T_bal);
  // launch id -> plan id is a bijection on [0, M); launch id L runs on XCD L % 8, which takes
  // its launch ids in order: the groups of a band are consecutive plan ids, and consecutive plan
  // ids are either the next dispatch of the same XCD or the first of the next XCD
  std::vector<int64_t> launch_of(p.M, -1);
  for (int64_t L = 0; L < p.M; ++L) {
    const int64_t id = xcd_remap(L, p.M);
    CHECK(id >= 0 && id < p.M && launch_of[id] < 0, "remap of %lld", (long long)L);
    if (id >= 0 && id < p.M) launch_of[id] = L;
  }
  for (int band = 0; band < p.B; ++band) {
    int breaks = 0;
    for (int g = 1; g < noff; ++g) {
      const int64_t l0 = launch_of[(size_t)band * noff + g - 1], l1 = launch_of[(size_t)band * noff + g];
      if (l1 == l0 + 8) continue;
      CHECK(l1 % 8 == l0 % 8 + 1 && l1 / 8 == 0, "band %d group %d: launches %lld, %lld", band, g,
            (long long)l0, (long long)l1);
      ++breaks;
    }
    CHECK(breaks <= (noff + p.M / 8 - 1) / (p.M / 8 > 0 ? p.M / 8 : 1),
          "band %d spread over %d XCD boundaries", band, breaks);
  }
}

int main() {
  const int64_t ns[] = {128, 1024, 4096, 4224, 125056, 1000064};
  for (int nb = 3; nb <= 12; ++nb)
    for (int64_t n_pad : ns) check_plan(nb, n_pad);
  // the headline: derived 2096 / 2176 / (512 / 510) = 0.9595, the rest is the start-up term
  {
    const SyrkBalPlan p = syrk_plan_balanced(1000064, 1024, kSlots, kWd, kC0);
    CHECK(p.on == 1, "headline plan declined");
    CHECK(p.T_bal <= 0.965 * p.T_pack, "headline ratio %.4f", p.T_bal / p.T_pack);
    CHECK(p.B == 16 && p.nwg == 512, "headline B %d nwg %d", p.B, p.nwg);
  }
  // declines: nb < 3, nb >= 32
  for (int64_t mp : {128, 256, 4096, 4224, 8192})
    for (int64_t n_pad : ns) {
      const SyrkBalPlan p = syrk_plan_balanced(n_pad, mp, kSlots, kWd, kC0);
      CHECK(p.on == 0 && p.nwg == 0, "mp %lld not declined", (long long)mp);
    }
  // fewer slots, another diagonal cost: still a valid selection
  {
    const SyrkBalPlan p = syrk_plan_balanced(1000064, 1024, 504, 40.0, 64.0);
    CHECK(p.nwg > 0 && p.nwg <= 504, "504-slot plan grid %d", p.nwg);
  }
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("all plan checks passed\n");
  if (g_unbalanced) {
    std::printf("%d plans above mean + 64\n", g_unbalanced);
    return 2;
  }
  return 0;
}
