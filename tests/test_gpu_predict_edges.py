"""GPU prediction (sgp_predict behind predict_vi / predict_laplace / predict_gp_full) at the
shapes where its kernels change path, entrywise against the fp64 oracle.

The bar is |got - ref| <= 1e-8 s per entry (1e-8: tests/test_gpu_predict.py's RTOL), s the
entry's magnitude budget -- the sum of the absolute values of the terms it is made of
(``_budget`` below, the fp64 twin of oracle/mp_ref.py's) -- so a far-apart pair of a full_cov
matrix is held as tightly as the diagonal.  Every case asserts cond(Sigma22) <= 4e4
(tests/test_gpu_sweep.py's COND_MAX: fp64 forward error ~ 4e4 * 2^-53 ~ 5e-12 s, three decades
below the bar) and that the knots matter to the rows: the median over rows of
k_i' Sigma22^-1 k_i / sigma^2 is >= 0.2.

Shapes (m, np, d, kernel) and what each reaches first:
  (7, 1, 3, sqexp)         one prediction row, m << tile
  (128, 128, 8, ard)       no padding on either axis
  (129, 129, 8, ard)       mp = npp = 256: two knot tiles in k_rowq_reduce, nb = 4 inverse
                           chain, 4 x 4 k_gemm64 tiles
  (257, 130, 3, sqexp)     mp = 384, nb = 6
  (20, 64, 1, sqexp), (20, 65, 1, ard)   d = 1 (knot grid), k_fill's 64-row block edge
  (40, 257, 12, ard)       d > 8 (the builder's NC = 4 form), npp = 384
  (33, 70, 20, ard), (20, 70, 32, ard)   NC = 8, the <SGP_MAXD> fillers
  offset (40, 150, 3, sqexp)  knots and rows at 5e3 + [0, 10]: the builder's centring
  wide (40, 150, 2, sqexp)    l = 0.7, half the rows spread over [0, 400], the knots in two
                              clusters 390 apart: span^2 above SGP_MFMA_SPAN2_MAX, so the
                              direct-difference VALU builder runs (held to 1e-12 s, WIDE_RTOL)
each for VI, predict_laplace in the gaussian and another family, diagonal and full_cov;
predict_gp_full (U = xy) at the two multi-tile shapes.  Inputs follow tests/test_gpu_edges.py's
_gauss recipe (knots uniform on [0, 10]^d, sigma = 1.2, tau = 0.5, delta = 1e-6); half the rows
(rounded up) are a knot plus N(0, (0.3 l)^2) jitter, two more equal knots exactly (np = 1: the
one row is a jittered knot), the rest are uniform.  Per coordinate that jitter costs a factor
exp(-0.09) of k^2, so for d = 20 and 32 the length scales are 2.2 sqrt(d) rather than
tests/test_gpu_edges.py's 1.2 sqrt(d): the other knots then carry enough of each row for the
0.2 floor (cond stays below 200).  u_var is a random SPD matrix of scale 0.05 sigma^2 and
u_mean = muu + N(0, 0.5): real posteriors are tests/test_gpu_predict.py's business.

Largest measured |got - ref| / s on an MI355X (mean / variance), over all shapes and both
covariance forms:
  predict_vi                 5.8e-15 / 5.7e-14  (d = 1, 64 rows / wide full_cov: Sigma11's far
                                                 pairs, exp of an exponent near -700)
  predict_laplace gaussian   5.8e-15 / 6.5e-15
  predict_laplace poisson    5.1e-15 / 7.0e-15
  predict_gp_full            1.7e-15 / 1.2e-15
  against mpmath directly    4.0e-15 / 7.1e-16  (all four calls, both fixtures)
With the matrix-core builder forced on the wide case the errors are 2.0e-11 / 1.7e-11.
"""
import math
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

import predict_cases as PC
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-8            # of the entry's budget s
# The wide case is held to 1e-12 s on top.  At the issue's 1e-8 the builder's form cannot be
# told apart: the GEMM-form exponent x~.u~ - |x~|^2/2 - |u~|^2/2 is off by ~2^-53 (|x~|^2 +
# |u~|^2) ~ 3e-11 at |x~|^2 ~ |u~|^2 ~ 1.6e5, three decades inside 1e-8.  1e-12 is what
# SGP_MFMA_SPAN2_MAX promises of the matrix-core builder (sgp_internal.h: K within ~1e-12 of the
# direct-difference form) and what the direct-difference form the oracle shares keeps with
# room: a few roundings of an exponent of at most 745 (745 * 3 * 2^-53 ~ 2.5e-13 relative in K,
# k_fill's far pairs of Sigma11 included) plus cond(Sigma22) 2^-53 ~ 1e-14.
WIDE_RTOL = 1e-12
COND_MAX = 4e4         # tests/test_gpu_sweep.py
RATIO_MIN = 0.2
SIGMA, TAU, DELTA = 1.2, 0.5, 1e-6


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


# name -> (m, np, d, kernel, layout)
SHAPES = OrderedDict([
    ("one_row", (7, 1, 3, "sqexp", "plain")),
    ("on_grid", (128, 128, 8, "ard", "plain")),
    ("one_past", (129, 129, 8, "ard", "plain")),
    ("three_tiles", (257, 130, 3, "sqexp", "plain")),
    ("rows64_d1", (20, 64, 1, "sqexp", "plain")),
    ("rows65_d1", (20, 65, 1, "ard", "plain")),
    ("np_past_256_d12", (40, 257, 12, "ard", "plain")),
    ("d20", (33, 70, 20, "ard", "plain")),
    ("d32", (20, 70, 32, "ard", "plain")),
    ("offset", (40, 150, 3, "sqexp", "offset")),
    ("wide", (40, 150, 2, "sqexp", "wide")),
])
FULL_SHAPES = ("one_past", "three_tiles")
_CASES, _REFS = {}, {}


def _length_scales(m, d, cov_fun, layout):
    """Base length scale per shape, chosen on the CPU for cond(Sigma22) <= COND_MAX and the
    0.2 relevance floor (the module docstring has the reasoning for d >= 20)."""
    if layout == "wide":
        l0 = 0.7
    elif d == 1:
        l0 = 0.5                     # knot grid of spacing ~0.5
    elif d == 8:
        l0 = 3.4
    elif d == 3:
        l0 = 1.2 if m > 128 else 1.7
    elif d == 12:
        l0 = 1.2 * math.sqrt(d)
    else:
        l0 = 2.2 * math.sqrt(d)
    if cov_fun == "sqexp":
        return [l0]
    step = 0.25 if d <= 8 else 0.2   # _gauss / _gauss_hd of tests/test_gpu_edges.py
    return [l0 + step * c for c in range(d)]


def _case(name):
    if name in _CASES:
        return _CASES[name]
    m, npred, d, cov_fun, layout = SHAPES[name]
    g = np.random.Generator(np.random.PCG64(700 + 13 * m + npred + d))
    base = 5.0e3 if layout == "offset" else 0.0
    U = base + g.uniform(0.0, 10.0, size=(m, d))
    if d == 1:
        U = np.linspace(0.1, 9.9, m)[:, None]
    if layout == "wide":
        # two clusters of knots 390 apart: their mean, the builder's centre, is ~280 length
        # scales from every knot, so the rows that matter (those near knots) are the ones a
        # GEMM-form exponent would get wrong
        U[m // 2:] += 390.0
    ls = _length_scales(m, d, cov_fun, layout)
    lvec = np.array(ls if cov_fun == "ard" else ls * d)
    if cov_fun == "ard":
        cp = OrderedDict([("sigma", SIGMA)] + [(f"l{c + 1}", ls[c]) for c in range(d)]
                         + [("tau", TAU)])
    else:
        cp = OrderedDict([("sigma", SIGMA), ("l", ls[0]), ("tau", TAU)])
    nj = (npred + 1) // 2
    hi = 400.0 if layout == "wide" else 10.0
    xp = base + g.uniform(0.0, hi, size=(npred, d))
    src = g.integers(0, m, size=nj)
    xp[:nj] = U[src] + g.normal(0.0, 1.0, size=(nj, d)) * (0.3 * lvec)
    if npred >= 4:
        xp[nj], xp[nj + 1] = U[0], U[m - 1]          # exact coincidence with knots
    A = g.normal(0.0, 1.0, size=(m, m))
    u_var = 0.05 * SIGMA ** 2 * (A @ A.T) / m
    muu = np.full(m, 0.3)
    u_mean = muu + g.normal(0.0, 0.5, size=m)
    y = np.sin(U - base).sum(axis=1) / math.sqrt(d) + g.normal(0.0, 0.5, size=m)
    post = dict(u_mean=u_mean, u_var=u_var, muu=muu)
    _CASES[name] = dict(cov_fun=cov_fun, cov_par=cp, U=U, xp=xp, delta=DELTA, lvec=lvec,
                        mu_pred=0.25 + 0.1 * np.sin(np.arange(npred)), gauss=post,
                        nongauss=post, full=dict(y=y, mu=np.full(m, y.mean())))
    return _CASES[name]


def _sigma22(F, method):
    """Sigma22 of the method and K = k(x_pred, U) (fp64, the oracle's fillers)."""
    s12, s22, _ = O._pred_mats(F["U"], F["xp"], F["cov_fun"], F["cov_par"], F["delta"],
                               method in ("vi", "lap_gauss"))
    return s22, s12


def _budget(F, method, full_cov):
    """fp64 magnitude budgets (s_mean, s_var): |mu_i| + sum_j |k_ij| |w_j|;
    c0 + sum_jl |k_ij| |T_jl| |k_il|; full_cov |Sigma11_ij| + |K| |T| |K|', for predict_laplace
    with the Q = K Sigma22^-1 K' terms of diag(diag(Sigma11 - Q)) + Q (off the diagonal Q_ij
    alone, on it Sigma11_ii - Q_ii + Q_ii)."""
    s22, K = _sigma22(F, method)
    cp = F["cov_par"]
    s22i = np.linalg.inv(s22)
    if method == "gp_full":
        dm, T = F["full"]["y"] - F["full"]["mu"], -s22i
    else:
        P = F["nongauss" if method == "lap_nongauss" else "gauss"]
        dm, T = P["u_mean"] - P["muu"], -s22i + s22i @ P["u_var"] @ s22i
    Ka, Ta = np.abs(K), np.abs(T)
    s_mean = np.abs(F["mu_pred"]) + Ka @ np.abs(s22i @ dm)
    c2 = float(cp["sigma"]) ** 2 + float(cp["tau"]) ** 2
    if not full_cov:
        c0 = c2 if method in ("lap_gauss", "lap_nongauss") else c2 + F["delta"]
        return s_mean, c0 + np.sum((Ka @ Ta) * Ka, axis=1)
    ktk = Ka @ Ta @ Ka.T
    xp = F["xp"]
    if F["cov_fun"] == "ard":
        s11 = O.make_cov_mat_ardC(xp, None, cp, "ard", F["delta"], O.lnames_for("ard", xp.shape[1]))
    else:
        s11 = O.make_cov_matC(xp, None, cp, F["cov_fun"], F["delta"])
    if method in ("vi", "gp_full"):
        return s_mean, np.abs(s11) + ktk
    qa = Ka @ np.abs(s22i) @ Ka.T
    s_var = qa + ktk
    s_var[np.diag_indices_from(s_var)] = np.abs(np.diag(s11)) + 2 * np.diag(qa) + np.diag(ktk)
    return s_mean, s_var


def _conditioning(F, method):
    """(cond(Sigma22), median_i k_i' Sigma22^-1 k_i / sigma^2)."""
    s22, K = _sigma22(F, method)
    ratio = np.sum(K * np.linalg.solve(s22, K.T).T, axis=1) / float(F["cov_par"]["sigma"]) ** 2
    return float(np.linalg.cond(s22)), float(np.median(ratio))


def _span2(F):
    """|x~|^2 bound as sgp_predict's set_center computes it: centre = the knots' column means,
    per coordinate the farthest of the knots' and rows' extremes, in length scales."""
    U, xp = F["U"], F["xp"]
    ctr = U.mean(axis=0)
    lo = np.minimum(U.min(axis=0), xp.min(axis=0))
    hi = np.maximum(U.max(axis=0), xp.max(axis=0))
    e = np.maximum(np.abs(lo - ctr), np.abs(hi - ctr)) / F["lvec"]
    return float(np.sum(e * e))


def _span2_max():
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "sparsergps_amd", "csrc", "sgp_internal.h")
    with open(hdr) as f:
        mt = re.search(r"SGP_MFMA_SPAN2_MAX\s*=\s*([0-9.eE+-]+)\s*;", f.read())
    assert mt, "SGP_MFMA_SPAN2_MAX not found in sgp_internal.h"
    return float(mt.group(1))


def _reference(F, key, method, full_cov):
    """Oracle output and budgets, computed once per (case, method, form) and left unchanged."""
    k = (key, method, full_cov)
    if k not in _REFS:
        ref = PC.call(O, method, F, full_cov)
        _REFS[k] = (np.asarray(ref["pred_mean"], dtype=np.float64).reshape(-1),
                    np.asarray(ref["pred_var"], dtype=np.float64), *_budget(F, method, full_cov))
    return _REFS[k]


def _err(got, ref, s):
    """|got - ref| / s entrywise.  Where every term of an entry underflows to zero (a pair of
    rows hundreds of length scales apart, far from every knot) s is 0 and the bar
    |got - ref| <= 1e-8 s asks for got == ref exactly: 0 there if so, inf if not."""
    e = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, e / s, np.where(e == 0, 0.0, np.inf))


def _check(sgp, F, key, method, full_cov, rtol=RTOL):
    cond, ratio = _conditioning(F, method)
    assert cond <= COND_MAX, (key, method, cond)
    assert ratio >= RATIO_MIN, (key, method, ratio)
    rm, rv, sm, sv = _reference(F, key, method, full_cov)
    got = PC.call(sgp, method, F, full_cov)
    gm = np.asarray(got["pred_mean"]).reshape(-1)
    gv = np.asarray(got["pred_var"])
    assert gm.shape == rm.shape and gv.shape == rv.shape
    assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gv))
    em, ev = _err(gm, rm, sm), _err(gv, rv, sv)
    print(f"{key} {method} full_cov={full_cov}: cond {cond:.3g} ratio {ratio:.3g} "
          f"mean {em.max():.3e} var {ev.max():.3e}")
    assert em.max() <= rtol, (key, method, "mean", int(em.argmax()), em.max())
    assert ev.max() <= rtol, (key, method, "var", np.unravel_index(ev.argmax(), ev.shape),
                              ev.max())
    if full_cov:
        assert _err(gv, gv.T, sv).max() <= rtol


@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("method", ["vi", "lap_gauss", "lap_nongauss"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_sparse_prediction_edges(sgp, name, method, full_cov):
    F = _case(name)
    smax = _span2_max()
    if SHAPES[name][4] == "wide":
        # span^2 ~ 2 (200 / 0.7)^2 ~ 1.6e5 against SGP_MFMA_SPAN2_MAX = 1e4: the VALU builder
        assert _span2(F) > smax, (_span2(F), smax)
        _check(sgp, F, name, method, full_cov, WIDE_RTOL)
    else:
        assert _span2(F) <= smax, (_span2(F), smax)       # ... and the matrix-core one here
        _check(sgp, F, name, method, full_cov)


@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("name", FULL_SHAPES)
def test_full_gp_prediction_edges(sgp, name, full_cov):
    """predict_gp_full with U = xy (m = n) at the two multi-tile shapes."""
    _check(sgp, _case(name), name, "gp_full", full_cov)


@pytest.mark.parametrize("name", list(PC.MP_FIXTURES))
def test_prediction_matches_mpmath(sgp, name):
    """The GPU against 50-digit mpmath directly (tests/predict_cases.py's fixtures, the ones
    tests/test_mpmath.py pins the oracle on): every entry within 1e-8 s, s mpmath's budget."""
    F = PC.mp_fixture(name)
    for method in PC.METHODS:
        for full_cov in (False, True):
            ref = PC.mp_predict(name, method, full_cov)
            # the fp64 budgets the edge cases use are mpmath's
            sm, sv = _budget(F, method, full_cov)
            np.testing.assert_allclose(sm, ref["s_mean"], rtol=1e-9)
            np.testing.assert_allclose(sv.reshape(ref["s_var"].shape), ref["s_var"], rtol=1e-9)
            got = PC.call(sgp, method, F, full_cov)
            em = np.abs(np.asarray(got["pred_mean"]).reshape(-1) - ref["pred_mean"]) / ref["s_mean"]
            ev = np.abs(np.asarray(got["pred_var"]) - ref["pred_var"]) / ref["s_var"]
            print(f"mpmath {name} {method} full_cov={full_cov}: mean {em.max():.3e} "
                  f"var {ev.max():.3e}")
            assert em.max() <= RTOL and ev.max() <= RTOL, (method, full_cov, em.max(), ev.max())


def test_not_positive_definite_then_recovers(sgp):
    """A duplicated knot with delta = -1e-3 (tests/test_gpu_edges.py's
    test_not_positive_definite_order) makes the gaussian Sigma22 = Kuu + delta I indefinite from
    the leading minor of order 151 on, in the second knot tile: NotPositiveDefinite names that
    order, and the next valid call matches the oracle."""
    from sparsergps_amd._lib import NotPositiveDefinite
    g = np.random.Generator(np.random.PCG64(77))
    m, d, npred = 200, 3, 9
    U = g.uniform(0.0, 10.0, size=(m, d))
    U[150] = U[3]
    xp = g.uniform(0.0, 10.0, size=(npred, d))
    cp = OrderedDict([("sigma", 1.0), ("l", 0.3), ("tau", 0.5)])
    with pytest.raises(NotPositiveDefinite, match="order 151"):
        sgp.predict_vi(np.zeros(m), np.eye(m), U, xp, "sqexp", cp, np.zeros(npred), np.zeros(m),
                       False, delta=-1e-3)
    F = _case("one_past")
    _check(sgp, F, "one_past", "vi", True)


def test_exp_kernel_is_refused(sgp):
    """No fit carries the 'exp' kernel (optimize_gp.R:263); sgp_predict refuses it with
    SGP_EINVAL before any device work instead of failing inside the K12 builder."""
    from sparsergps_amd._lib import SGP_EINVAL, SGPError
    F = _case("one_row")
    P = F["gauss"]
    cp = OrderedDict([("sigma", 1.2), ("l", 1.7), ("tau", 0.5)])
    with pytest.raises(SGPError, match="sqexp") as ei:
        sgp.predict_vi(P["u_mean"], P["u_var"], F["U"], F["xp"], "exp", cp, F["mu_pred"],
                       P["muu"])
    assert ei.value.status == SGP_EINVAL
