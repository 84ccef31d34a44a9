"""GPU knot gradients against the literal oracle past a single tile.

sgp_knot_gradient is what a fit with xu_opt = "simultaneous" follows at every step.  Each case here
goes through an R-level entry point (delbo_dcov_par / dlogp_dcov_par / dlogq_dcov_par) and compares
knot_gradient, trans_knot and the theta gradient with oracle/sgp_oracle.py (tests/bern_oracle.py
for the Bernoulli family; tests/test_knot_oracle.py pins the knot branch of both), at the shapes
where the FITC / Laplace knot path runs code that VI never runs:

  two tiles both ways   n = 300, m = 130 (padded second row tile and second knot tile; knots on
                        data rows, one of them the last knot): FITC, Poisson Laplace (scalar and
                        per-row exposure), Bernoulli; with the stored products (d <= 8: both G
                        terms in ONE contraction pass, ConArgs::tin2 / M2 / rs_vec2) and with
                        SGP_TSTORE=0 (two passes, the second ACCUMULATES into the knot sums)
  coordinate chunks     ARD at d = 8 (m = 128: last shape of the one-pass path, every coordinate
                        column used), d = 9 (m = 129: first shape of the two-pass path with stored
                        products) and Poisson Laplace at d = 12, m = 129; knot_opt subsets
  tall column sums      n = 8321, m = 5: 66 row tiles, so launch_knot_reduce runs two row groups,
                        k_knot_reduce1's unrolled loop and its remainder loop; n = 12417: three
  sharded Laplace       three row shards, knot_gradient(None) with the bounds of all rows
  after a Newton run    knot_gradient() at the f that eval_laplace leaves

SGP_TSTORE is read once per context, so every run here makes its own context under the setting
it asks for; where the library records phase timings (FITC) the test also asserts which path ran
(the second pass is the phase "contract_knm_b").

Norm and bound.  Errors are max|got - ref| / max|ref|, separately for the knot gradient and the
theta gradient, with no floor of 1 (knot-gradient entries are of size 1e-2: a floor of 1 makes
a relative bound an absolute one).  The bound is 1000 eta, where eta is the reference's own
sensitivity to one ulp of input: the same oracle call with every entry of X and U multiplied by
1 +- 2^-52 (fixed seed; knots placed on data rows stay on them), same norm.  The factor 1000
covers the different algebra (adjoint contraction and a Gauss-Jordan inverse on the GPU, literal
loops and Cholesky solves in the oracle), both fp64 over the same ~n m terms.  A raised bound
needs a written reason and never exceeds CAP = 1e-9 (RAISED below).  The stored-product run and
the SGP_TSTORE=0 run agree with each other to 1e-11 (test_gpu_tstore.py's bound, in this norm).

Measured on an MI355X (eta is computed by the CPU of the same machine; err is the larger of the
stored-product run and the SGP_TSTORE=0 run where both exist; "s/0" is the two against each other):

  case                    eta knot  eta theta  err knot  err theta  s/0 knot  s/0 theta
  fitc_sqexp_300_130      3.4e-15   6.0e-16    2.5e-14   3.8e-15    2.3e-15   2.4e-15
  fitc_ard_300_130        2.6e-12   2.0e-12    1.8e-10   2.4e-11    4.1e-14   2.3e-14
  lap_sqexp_300_130       1.7e-14   1.1e-15    3.9e-14   2.0e-15    4.6e-15   5.7e-16
  lap_ard_300_130         6.4e-15   5.7e-16    2.5e-14   8.4e-16    2.8e-15   7.0e-16
  lap_rowexpo_300_130     1.2e-14   2.4e-15    3.1e-14   6.9e-16
  bern_sqexp_200_7        2.0e-14   1.1e-14    1.7e-14   1.3e-15
  bern_sqexp_300_130      1.1e-14   3.0e-16    4.1e-14   6.2e-16    2.1e-14   1.4e-16
  bern_ard_300_130        1.8e-14   2.5e-16    6.3e-14   4.1e-16    1.9e-14   6.7e-16
  fitc_ard_d8_257_128     5.4e-15   8.0e-16    1.4e-14   1.3e-15
  fitc_ard_d9_257_129     1.6e-15   4.4e-17    4.0e-15   4.7e-16
  lap_ard_d12_200_129     1.6e-15   1.8e-16    3.2e-15   5.4e-16
  vi_tall_8321_5          4.5e-14   2.5e-17    1.5e-12   3.8e-14 (bound raised, see RAISED)
  fitc_tall_8321_5        2.1e-14   2.1e-15    1.9e-13   8.9e-14    2.9e-16   4.8e-16
  lap_tall_8321_5         1.6e-15   9.6e-18    3.3e-15   3.4e-16
  fitc_tall_12417_5       7.0e-14   1.1e-14    1.0e-12   3.7e-13
  lap_sharded_301_20      3.2e-15   1.4e-16    1.5e-15   4.7e-16
  lap_newton_300_20       4.6e-15   1.1e-16    3.2e-15   2.3e-16

Every bound is 1000 eta except two.  fitc_ard_300_130: 1000 eta is 2.6e-9 and 2.0e-9 (cond K22 is
5e4 at that ARD parameter set), so both bounds are the cap, 1e-9.
vi_tall_8321_5, theta gradient: RAISED below.  trans_knot is bit-equal to the oracle's everywhere.
"""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest

import bern_oracle as B
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
FACTOR = 1000.0
CAP = 1e-9
BOTH_TOL = 1e-11
EPS = float(np.finfo(np.float64).eps)

# case -> (bound on the knot gradient or None, bound on the theta gradient or None, reason):
# bounds above 1000 eta, each with where the error arises; none may exceed CAP
RAISED = {
    "vi_tall_8321_5": (
        None, 3e-13,
        "the error sits in d/dlog(l) (4.0e3 against the largest entry, 7.2e4), a sum of "
        "n m = 41605 cancelling terms.  The oracle's own result moves by 1.2e-14 to 2.8e-14 in "
        "this norm when its rows are merely reordered (five random orders and the reversed "
        "one), and the numpy model of the adjoint algebra (oracle/adjoint_ref.py: no kernel "
        "involved) differs from the oracle by 3.77e-14, the GPU's figure to three digits.  "
        "eta = 2.5e-17 is below the unit roundoff: one-ulp moves of X and U leave the order of "
        "the sums as it is, so they do not show this rounding.  Bound: ten times the largest "
        "reorder change."),
}


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def _theta(g, cp):
    return np.array([g[k] for k in cp])


def _ard_par(d, l0=1.3, dl=0.4, sigma=1.2, tau=0.45):   # test_gpu_knots.py's
    return OrderedDict([("sigma", sigma)] + [(f"l{c + 1}", l0 + dl * c) for c in range(d)] +
                       [("tau", tau)])


def _ulp(a, seed):
    """Every entry times 1 +- 2^-52."""
    rng = np.random.default_rng(seed)
    return a * (1.0 + rng.choice([-1.0, 1.0], size=a.shape) * 2.0 ** -52)


# --------------------------------------------------------------------------------------- cases
def _finish(P, path, cov_fun, cp, pert, on_rows=(), ff=None, knot_opt=None):
    """One case: `pert` moves X and U by one ulp first; on_rows = [(knot, row)] then puts knots
    on data rows (so they coincide in the perturbed problem too)."""
    X, U = P["X"], P["U"].copy()
    if pert:
        X, U = _ulp(X, 71), _ulp(U, 72)
    for k, i in on_rows:
        U[k] = X[i]
    return dict(path=path, cov_fun=cov_fun, cov_par=cp, X=X, U=U, y=P["y"], mu=P["mu"],
                delta=P["delta"], ff=ff, a=P.get("a", 1.0), knot_opt=knot_opt)


def _gauss(path, cov_fun, n, m, pert, on_rows=()):
    P = O.make_gaussian_problem("C2", n=n, m=m)
    return _finish(P, path, cov_fun, P["cov_par"] if cov_fun == "sqexp" else _ard_par(3), pert,
                   on_rows)


def _poisson(cov_fun, n, m, pert, per_row=False):
    P = O.make_poisson_problem(n=n, m=m, per_row_exposure=per_row)
    ff = P["f0"] + 0.05 * np.cos(np.arange(n))
    return _finish(P, "lap", cov_fun, P["cov_par"] if cov_fun == "sqexp" else _ard_par(5), pert,
                   ff=ff)


def _bern(cov_fun, n, m, d, pert, theta=None):
    from sparsergps_amd.workloads import make_bernoulli_problem
    cp = None
    if theta is not None:
        cp = OrderedDict([("sigma", theta[0]), ("l", theta[1]), ("tau", theta[2])])
    P = make_bernoulli_problem(n, m, d=d, cov_par=cp)
    cp = P["cov_par"]
    if cov_fun == "ard":   # distinct length scales around the sqexp case's l = 1.5
        cp = OrderedDict([("sigma", cp["sigma"])] +
                         [(f"l{c + 1}", v) for c, v in enumerate((1.4, 1.7, 1.6, 1.5))] +
                         [("tau", cp["tau"])])
    return _finish(P, "bern", cov_fun, cp, pert, ff=0.3 * np.sin(np.arange(n)))


def _subset(m):
    """First, last and tile-edge knots (1-based): the literal oracle costs m d n Python calls."""
    return [k for k in (1, 2, 64, 65, 127, 128, 129) if k < m] + [m]


def _high_d(path, n, m, d, pert):
    g = np.random.Generator(np.random.PCG64(900 + d))
    X = g.uniform(0.0, 10.0, size=(n, d))
    U = g.uniform(0.0, 10.0, size=(m, d))
    cp = OrderedDict([("sigma", 1.2)] + [(f"l{c + 1}", math.sqrt(d) + 0.2 * c) for c in range(d)]
                     + [("tau", 0.45 if path == "fitc" else 0.1)])
    if path == "fitc":
        y = np.sin(X).sum(axis=1) / math.sqrt(d) + g.normal(0.0, 0.5, size=n)
        P = dict(X=X, U=U, y=y, mu=np.full(n, y.mean()), delta=1e-6)
        ff = None
    else:
        f = 0.5 * np.sin(X).sum(axis=1) / math.sqrt(d) + math.log(2.0)
        y = g.poisson(np.exp(f)).astype(np.float64)
        P = dict(X=X, U=U, y=y, mu=np.full(n, math.log(y.mean())), delta=1e-6, a=1.0)
        ff = P["mu"] + 0.05 * np.cos(np.arange(n))
    return _finish(P, path, "ard", cp, pert, ff=ff, knot_opt=_subset(m))


ON_ROWS = [(1, 4), (129, 299)]   # coincident rows; knot 129 is the last of the padded second tile
CASES = {
    "fitc_sqexp_300_130": lambda p: _gauss("fitc", "sqexp", 300, 130, p, ON_ROWS),
    "fitc_ard_300_130": lambda p: _gauss("fitc", "ard", 300, 130, p, ON_ROWS),
    "lap_sqexp_300_130": lambda p: _poisson("sqexp", 300, 130, p),
    "lap_ard_300_130": lambda p: _poisson("ard", 300, 130, p),
    "lap_rowexpo_300_130": lambda p: _poisson("sqexp", 300, 130, p, per_row=True),
    "bern_sqexp_200_7": lambda p: _bern("sqexp", 200, 7, 2, p),
    "bern_sqexp_300_130": lambda p: _bern("sqexp", 300, 130, 4, p, (2.0, 1.5, 0.1)),
    "bern_ard_300_130": lambda p: _bern("ard", 300, 130, 4, p, (2.0, 1.5, 0.1)),
    "fitc_ard_d8_257_128": lambda p: _high_d("fitc", 257, 128, 8, p),
    "fitc_ard_d9_257_129": lambda p: _high_d("fitc", 257, 129, 9, p),
    "lap_ard_d12_200_129": lambda p: _high_d("lap", 200, 129, 12, p),
    "vi_tall_8321_5": lambda p: _gauss("vi", "sqexp", 8321, 5, p),
    "fitc_tall_8321_5": lambda p: _gauss("fitc", "sqexp", 8321, 5, p),
    "lap_tall_8321_5": lambda p: _poisson("sqexp", 8321, 5, p),
    "fitc_tall_12417_5": lambda p: _gauss("fitc", "sqexp", 12417, 5, p),
    "lap_sharded_301_20": lambda p: _poisson("sqexp", 301, 20, p),
}


# ------------------------------------------------------------------------------------ the oracle
def _oracle(c):
    cp, fun = c["cov_par"], c["cov_fun"]
    kw = dict(dcov_fun_dknot=fun, knot_opt=c["knot_opt"])
    if c["path"] == "vi":
        return O.delbo_dcov_par(cp, fun, c["U"], c["X"], c["y"], c["mu"], c["delta"], **kw)
    if c["path"] == "fitc":
        return O.dlogp_dcov_par(cp, fun, c["U"], c["X"], c["y"], c["mu"], c["delta"], **kw)
    if c["path"] == "lap":
        return O.dlogq_dcov_par(cp, fun, c["U"], c["X"], c["y"], c["ff"], c["mu"], c["a"],
                                c["delta"], **kw)
    return B.dlogq_dcov_par(cp, fun, c["U"], c["X"], c["y"], c["ff"], c["mu"], c["delta"], **kw)


def _rows(c):
    """The knot-gradient rows a case compares (all, or those of its knot_opt), flattened."""
    m, d = c["U"].shape
    ks = np.arange(m) if c["knot_opt"] is None else np.asarray(c["knot_opt"]) - 1
    return (ks[:, None] * d + np.arange(d)[None, :]).reshape(-1)


def _reference_of(c, c_pert):
    """(oracle outputs, eta of the knot gradient, eta of the theta gradient)."""
    ref, per = _oracle(c), _oracle(c_pert)
    r = _rows(c)
    eta_k = _err(per["knot_gradient"][r], ref["knot_gradient"][r])
    eta_t = _err(_theta(per["gradient"], c["cov_par"]), _theta(ref["gradient"], c["cov_par"]))
    return ref, eta_k, eta_t


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Computed once per case (the literal knot loop takes seconds) and shared, unchanged."""
    return _reference_of(CASES[name](False), CASES[name](True))


# --------------------------------------------------------------------------------------- the GPU
def _gpu(sgp, c, ctx=None, knot_opt=None):
    cp, fun = c["cov_par"], c["cov_fun"]
    if c["path"] == "vi":
        return sgp.delbo_dcov_par(cp, fun, True, "dsqexp_dx2" if fun == "sqexp" else
                                  "dsqexp_dx2_ard", knot_opt, c["U"], c["X"], c["y"], None,
                                  c["mu"], True, c["delta"], ctx=ctx)
    if c["path"] == "fitc":
        return sgp.dlogp_dcov_par(cp, fun, True, fun, knot_opt, c["U"], c["X"], c["y"], None,
                                  c["mu"], True, c["delta"], ctx=ctx)
    return sgp.dlogq_dcov_par(cp, fun, True, fun, knot_opt, c["U"], c["X"], c["y"], c["ff"],
                              c["mu"], c["a"], c["delta"], ctx=ctx,
                              family="bernoulli" if c["path"] == "bern" else "poisson")


def _fresh(sgp, monkeypatch, c, stored, knot_opt=None, devices=None):
    """One evaluation on a context of its own, made with or without the stored products.
    Returns (outputs, whether a second contraction pass ran; None where no phase shows it)."""
    if stored:
        monkeypatch.delenv("SGP_TSTORE", raising=False)
    else:
        monkeypatch.setenv("SGP_TSTORE", "0")
    try:
        with sgp.SparseGPContext(c["X"], c["y"], c["mu"], m_max=c["U"].shape[0],
                                 devices=devices) as ctx:
            timed = c["path"] == "fitc" and devices is None
            if timed:
                ctx.enable_timing(True)
            got = _gpu(sgp, c, ctx, knot_opt)
            second = ("contract_knm_b" in [nm for nm, _ in ctx.timings()]) if timed else None
            if devices is not None:
                got["knot_gradient_default_bounds"] = ctx.knot_gradient(None)
    finally:
        monkeypatch.delenv("SGP_TSTORE", raising=False)
    return got, second


def _bounds(name, eta_k, eta_t):
    bk, bt = FACTOR * eta_k, FACTOR * eta_t
    if name in RAISED:
        rk, rt, reason = RAISED[name]
        assert reason
        bk, bt = (rk or bk), (rt or bt)
    return min(bk, CAP), min(bt, CAP)   # the cap is a condition, whatever eta is


def _compare(name, label, c, got, reference):
    """knot_gradient, trans_knot and the theta gradient of one GPU run against the oracle."""
    ref, eta_k, eta_t = reference
    r = _rows(c)
    e_k = _err(np.asarray(got["knot_gradient"])[r], ref["knot_gradient"][r])
    e_t = _err(_theta(got["gradient"], c["cov_par"]), _theta(ref["gradient"], c["cov_par"]))
    e_u = 0.0
    if "trans_knot" in got:
        e_u = float(np.max(np.abs(np.asarray(got["trans_knot"]) - ref["trans_knot"])))
    bk, bt = _bounds(name, eta_k, eta_t)
    print(f"\n[knot_tiles] {name} {label}: eta knot {eta_k:.2e} theta {eta_t:.2e} | "
          f"err knot {e_k:.2e} (bound {bk:.2e}) theta {e_t:.2e} (bound {bt:.2e}) "
          f"trans_knot {e_u:.1e}")
    return e_k < bk, e_t < bt, e_u <= 4 * EPS * float(np.max(np.abs(ref["trans_knot"])))


def _check(name, label, c, got, reference):
    ok = _compare(name, label, c, got, reference)
    assert ok[0], f"{name} {label}: knot gradient"
    assert ok[1], f"{name} {label}: theta gradient"
    assert ok[2], f"{name} {label}: trans_knot"


def _check_both(sgp, monkeypatch, name):
    """With the stored products and with SGP_TSTORE=0: each against the oracle, and the two
    against each other."""
    c, reference = CASES[name](False), _reference(name)
    a, second_a = _fresh(sgp, monkeypatch, c, True)
    b, second_b = _fresh(sgp, monkeypatch, c, False)
    if c["path"] == "fitc":   # d <= 8: one pass with the stored products, two without
        assert (second_a, second_b) == (False, True)
    e_k = _err(a["knot_gradient"], b["knot_gradient"])
    e_t = _err(_theta(a["gradient"], c["cov_par"]), _theta(b["gradient"], c["cov_par"]))
    print(f"\n[knot_tiles] {name} stored vs SGP_TSTORE=0: knot {e_k:.2e} theta {e_t:.2e}")
    oks = [_compare(name, lab, c, g, reference) for lab, g in (("stored", a), ("tstore0", b))]
    assert all(all(ok) for ok in oks), oks
    assert e_k < BOTH_TOL and e_t < BOTH_TOL
    assert np.array_equal(a["trans_knot"], b["trans_knot"])


# ----------------------------------------------------------------------- two tiles both ways
@pytest.mark.parametrize("name", ["fitc_sqexp_300_130", "fitc_ard_300_130", "lap_sqexp_300_130",
                                  "lap_ard_300_130", "bern_sqexp_300_130", "bern_ard_300_130"])
def test_two_tiles_both_ways(sgp, monkeypatch, name):
    _check_both(sgp, monkeypatch, name)


def test_two_tiles_per_row_exposure(sgp, monkeypatch):
    name = "lap_rowexpo_300_130"
    c = CASES[name](False)
    assert np.ndim(c["a"]) == 1
    _check(name, "stored", c, _fresh(sgp, monkeypatch, c, True)[0], _reference(name))


def test_bernoulli_knot_gradient_cached_context(sgp):
    """The vignette's theta at d = 2, through the entry point's own cached context."""
    name = "bern_sqexp_200_7"
    c = CASES[name](False)
    _check(name, "cached ctx", c, _gpu(sgp, c), _reference(name))


# ---------------------------------------------------------------------- coordinate chunks
@pytest.mark.parametrize("name,second_pass", [("fitc_ard_d8_257_128", False),
                                              ("fitc_ard_d9_257_129", True),
                                              ("lap_ard_d12_200_129", None)])
def test_coordinate_chunks(sgp, monkeypatch, name, second_pass):
    """d = 8: the last shape on the one-pass path, every coordinate column used; d = 9: the first
    on the two-pass accumulating path with stored products; d = 12 (Laplace): two chunks."""
    c = CASES[name](False)
    m, d = c["U"].shape
    full, second = _fresh(sgp, monkeypatch, c, True)
    assert second == second_pass
    sub, _ = _fresh(sgp, monkeypatch, c, True, knot_opt=c["knot_opt"])
    r = _rows(c)
    gf, gs = np.asarray(full["knot_gradient"]), np.asarray(sub["knot_gradient"])
    assert gf.shape == gs.shape == (m * d,)
    assert np.array_equal(gs[r], gf[r])               # the subset call: its own full call's rows,
    assert not np.any(np.delete(gs, r))               # bit for bit, and 0 elsewhere
    assert np.all(gf != 0.0)
    _check(name, "knot_opt", c, sub, _reference(name))


# -------------------------------------------------------------------------- tall column sums
@pytest.mark.parametrize("name", ["vi_tall_8321_5", "lap_tall_8321_5", "fitc_tall_12417_5"])
def test_tall_column_sums(sgp, monkeypatch, name):
    """66 row tiles: gy = 2 row groups, the unrolled loop and its remainder (98 tiles: gy = 3)."""
    c = CASES[name](False)
    _check(name, "stored", c, _fresh(sgp, monkeypatch, c, True)[0], _reference(name))


def test_tall_column_sums_fitc_both_ways(sgp, monkeypatch):
    _check_both(sgp, monkeypatch, "fitc_tall_8321_5")


# ------------------------------------------------------------------------------ sharded Laplace
def test_sharded_laplace_knot_gradient(sgp, monkeypatch):
    """Three row shards on one device, passed as ctx=: the knot sums cross the shards, and
    knot_gradient(None) uses the bounds of ALL rows (a shard's own range would change the
    chain factor by percents)."""
    name = "lap_sharded_301_20"
    c = CASES[name](False)
    got, _ = _fresh(sgp, monkeypatch, c, True, devices=[0, 0, 0])
    _check(name, "devices=[0,0,0]", c, got, _reference(name))
    kd, kg = got["knot_gradient_default_bounds"], np.asarray(got["knot_gradient"])
    assert np.max(np.abs(kd - kg)) <= 4 * EPS * np.max(np.abs(kg))


# --------------------------------------------------------------------------- after a Newton run
def test_knot_gradient_after_newton(sgp):
    """eval_laplace(tol = 1e-5) from f0, then knot_gradient(): compared with the oracle AT the f
    the context returns, so the mode's own convergence does not enter."""
    n, m = 300, 20
    P = O.make_poisson_problem(n=n, m=m)
    cp = P["cov_par"]
    th = np.array(list(cp.values()))
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=m) as ctx:
        ctx.enable_knot_grad(True)
        ctx.lap_set_f(P["f0"])
        _, g, it = ctx.eval_laplace(th, "sqexp", P["U"], P["delta"], P["a"], 1e-5, 1000)
        kg = ctx.knot_gradient()
        f = ctx.lap_get_f()
    assert it > 2
    c, c_pert = (_finish(P, "lap", "sqexp", cp, p, ff=f) for p in (False, True))
    got = {"knot_gradient": kg, "gradient": OrderedDict(zip(cp, g))}   # [sigma, l, tau]
    _check("lap_newton_300_20", f"{it} NR steps", c, got, _reference_of(c, c_pert))
