"""CPU pins of the oracle's knot branch (_knot_loop, _dknot_mats, dsqexp_dx2 and the knot closures
of delbo_dcov_par / dlogp_dcov_par / dlogq_dcov_par), which test_oracle.py and test_mpmath.py
never call and which every GPU knot-gradient test trusts.

VI and FITC: there the knot gradient is the objective's derivative in the transformed knot
coordinate, so it is compared with central differences (h = 1e-5) of elbo_eval / fitc_obj_eval in
U[k, c] times the chain factor (ub - lb) / ((u - lb)(ub - u) + 1e-4), at C2 with n = 300,
m = 130 (sqexp and an ARD parameter set), knots 0, 64 and 129, every coordinate.  Bound: 1e-7 of
the largest knot-gradient entry (FITC sqexp differs by 8.6e-9, 2.1e-9, 7e-10 against a largest
entry of 2.85: 3e-9 relative, which leaves about 30x for truncation error elsewhere).

The differences are taken of an extended-precision (numpy longdouble, eps 1.1e-19) evaluation of
the same two objectives, _objective_ld below, which a test of its own ties to elbo_eval /
fitc_obj_eval (1e-11 relative).  In fp64 the difference quotient cannot resolve the bound at the
ARD set: cond K22 is 5e4 there, moving every entry of X and U by one ulp moves elbo_eval /
fitc_obj_eval by 1e-11 to 1e-10 (1e-13 at the sqexp set), and dividing by 2h = 2e-5 turns that
into up to 5e-6 against bounds of 5.2e-7 (VI) and 2.4e-7 (FITC); the fp64 quotient's worst miss
with h = 1e-3, 1e-4, 1e-5, 1e-6 is 3.7e-7, 1.1e-7, 4.9e-6, 2.5e-5 for VI and 3.1e-7, 4.5e-7,
4.6e-6, 2.6e-5 for FITC, growing as 1 / h as rounding noise does.  With the objective in extended
precision, same h, knots, cases and bound, the worst |fd - g| is 2.1e-10 / 4.4e-11 (VI / FITC,
sqexp) and 1.1e-9 / 2.6e-9 (ARD).  The fp64 quotient of elbo_eval / fitc_obj_eval themselves is
kept at the sqexp set, where fp64 resolves the bound.

Laplace: its knot gradient is NOT the objective's derivative (the comp3 quirk),
so it gets no finite-difference pin.  Its closure shares _gaussian_comps and _dknot_mats with the
two pinned above, and its comp3 lines are those of the theta loop that test_mpmath.py pins.

Bernoulli: tests/bern_oracle.py's gradient takes the likelihood derivatives as arguments and is
otherwise family-free; run with the Poisson derivatives it must reproduce O.dlogq_dcov_par's
gradient and knot gradient bit for bit.
"""
import functools
from collections import OrderedDict

import numpy as np
import pytest

import bern_oracle as B
from oracle import sgp_oracle as O

N, M = 300, 130
KNOTS = (0, 64, 129)
H = 1e-5


def _ard_par(d):   # test_gpu_knots.py's
    return OrderedDict([("sigma", 1.2)] + [(f"l{c + 1}", 1.3 + 0.4 * c) for c in range(d)] +
                       [("tau", 0.45)])


def _problem(cov_fun):
    P = O.make_gaussian_problem("C2", n=N, m=M)
    if cov_fun == "ard":
        P["cov_par"] = _ard_par(3)
    return P


_PATHS = {"vi": (O.elbo_eval, O.delbo_dcov_par), "fitc": (O.fitc_obj_eval, O.dlogp_dcov_par)}


def _grad(path, cov_fun, knot_opt=None):
    P = _problem(cov_fun)
    return _PATHS[path][1](P["cov_par"], cov_fun, P["U"], P["X"], P["y"], P["mu"], P["delta"],
                           dcov_fun_dknot=cov_fun, knot_opt=knot_opt)


@functools.lru_cache(maxsize=None)
def _full(path, cov_fun):
    """All m d knot coordinates (seconds on the CPU): computed once per case."""
    return _grad(path, cov_fun)


LD = np.longdouble


def _chol_ld(A):
    """Lower Cholesky factor, column by column, in A's own precision."""
    m = len(A)
    L = np.zeros((m, m), dtype=A.dtype)
    for j in range(m):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    return L


def _forward_ld(L, B):
    """L^-1 B by forward substitution."""
    X = np.zeros_like(B)
    for i in range(len(L)):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def _kern_ld(A, B, cp, cov_fun):
    ls = [cp["l"]] * A.shape[1] if cov_fun == "sqexp" else [cp[f"l{c + 1}"]
                                                            for c in range(A.shape[1])]
    s = np.zeros((len(A), len(B)), dtype=LD)
    for c, l in enumerate(ls):
        s += ((A[:, c, None] - B[None, :, c]) / LD(l)) ** 2
    return LD(cp["sigma"]) ** 2 * np.exp(-s / 2)


def _objective_ld(path, cp, cov_fun, U, X, y, mu, delta):
    """elbo_eval (path "vi": vi_mats + elbo_fun) / fitc_obj_eval (fitc_mats + obj_fun_norm) in
    numpy longdouble: K22 = k(U, U) + delta I, Z = tau^2 + delta (VI) or the FITC diagonal, the
    Woodbury quadratic form and determinants by Cholesky, VI's trace term."""
    assert np.finfo(LD).eps < 1e-18, "numpy longdouble is no wider than double here"
    X, U = X.astype(LD), U.astype(LD)
    r = y.astype(LD) - mu.astype(LD)
    sig2, tau2, dl = LD(cp["sigma"]) ** 2, LD(cp["tau"]) ** 2, LD(delta)
    n, m = len(X), len(U)
    K12 = _kern_ld(X, U, cp, cov_fun)
    K22 = _kern_ld(U, U, cp, cov_fun) + dl * np.eye(m, dtype=LD)
    L22 = _chol_ld(K22)
    W = _forward_ld(L22, K12.T)
    q = np.sum(W * W, axis=0)                      # rowsum(K12 * t(K22^-1 K21))
    Z = np.full(n, tau2 + dl) if path == "vi" else sig2 + tau2 + dl - q
    ZS = K12 / Z[:, None]
    LA = _chol_ld(K22 + K12.T @ ZS)
    v = _forward_ld(LA, (ZS.T @ r)[:, None])[:, 0]
    quad = -(r @ (r / Z)) / 2 + (v @ v) / 2
    det_part = -(np.sum(np.log(Z)) - 2 * np.sum(np.log(np.diag(L22))) +
                 2 * np.sum(np.log(np.diag(LA)))) / 2
    out = quad + det_part - LD(n) / 2 * np.log(2 * LD(np.pi))
    if path == "vi":
        out += -np.sum(sig2 + dl - q) / (2 * tau2)   # trace_term_fun
    return out


def _chain(b, u, c):
    return (b[c, 1] - b[c, 0]) / ((u - b[c, 0]) * (b[c, 1] - u) + 1e-4)


@pytest.mark.parametrize("cov_fun", ["sqexp", "ard"])
@pytest.mark.parametrize("path", ["vi", "fitc"])
def test_extended_objective_is_the_oracles(path, cov_fun):
    """1e-11 relative: the fp64 objectives themselves move by up to 3e-13 relative (1e-10 of
    about 400) when X and U move by one ulp at the ARD set."""
    P = _problem(cov_fun)
    args = (P["cov_par"], cov_fun, P["U"], P["X"], P["y"], P["mu"], P["delta"])
    o = _PATHS[path][0](*args)
    assert abs(float(_objective_ld(path, *args)) - o) < 1e-11 * abs(o)


@pytest.mark.parametrize("cov_fun", ["sqexp", "ard"])
@pytest.mark.parametrize("path", ["vi", "fitc"])
def test_knot_gradient_is_the_objective_derivative(path, cov_fun):
    P = _problem(cov_fun)
    g = _full(path, cov_fun)["knot_gradient"].reshape(M, 3)
    b = O.knot_bounds_of(P["X"])
    bound = 1e-7 * float(np.max(np.abs(g)))
    for k in KNOTS:
        for c in range(3):
            Up, Um = P["U"].copy(), P["U"].copy()
            Up[k, c] += H
            Um[k, c] -= H
            fd = float((_objective_ld(path, P["cov_par"], cov_fun, Up, P["X"], P["y"], P["mu"],
                                      P["delta"]) -
                        _objective_ld(path, P["cov_par"], cov_fun, Um, P["X"], P["y"], P["mu"],
                                      P["delta"])) / (LD(Up[k, c]) - LD(Um[k, c])))
            err = abs(fd * _chain(b, P["U"][k, c], c) - g[k, c])
            print(f"\n[knot_oracle] {path} {cov_fun} knot {k} coord {c}: |fd - g| {err:.2e} "
                  f"(bound {bound:.2e})")
            assert err < bound, (path, cov_fun, k, c, fd, g[k, c])


@pytest.mark.parametrize("path", ["vi", "fitc"])
def test_fp64_differences_at_the_sqexp_set(path):
    """Central differences of elbo_eval / fitc_obj_eval themselves, where fp64 resolves them."""
    P = _problem("sqexp")
    obj = _PATHS[path][0]
    g = _full(path, "sqexp")["knot_gradient"].reshape(M, 3)
    b = O.knot_bounds_of(P["X"])
    bound = 1e-7 * float(np.max(np.abs(g)))
    for k in KNOTS:
        for c in range(3):
            Up, Um = P["U"].copy(), P["U"].copy()
            Up[k, c] += H
            Um[k, c] -= H
            fd = (obj(P["cov_par"], "sqexp", Up, P["X"], P["y"], P["mu"], P["delta"]) -
                  obj(P["cov_par"], "sqexp", Um, P["X"], P["y"], P["mu"], P["delta"])) / (2 * H)
            assert abs(fd * _chain(b, P["U"][k, c], c) - g[k, c]) < bound, (path, k, c)


@pytest.mark.parametrize("cov_fun", ["sqexp", "ard"])
@pytest.mark.parametrize("path", ["vi", "fitc"])
def test_knot_opt_subset(path, cov_fun):
    """knot_opt (1-based, as in R): the listed knots' rows as in the full call, 0 elsewhere."""
    full = _full(path, cov_fun)
    sub = _grad(path, cov_fun, knot_opt=[k + 1 for k in KNOTS])
    gs, gf = sub["knot_gradient"].reshape(M, 3), full["knot_gradient"].reshape(M, 3)
    rows = list(KNOTS)
    assert np.array_equal(gs[rows], gf[rows])
    assert np.all(gs[rows] != 0.0)
    assert not np.any(np.delete(gs, rows, axis=0))
    assert np.array_equal(sub["trans_knot"], full["trans_knot"])
    assert sub["gradient"] == full["gradient"]


@pytest.mark.parametrize("ard", [False, True])
def test_dknot_mats_are_the_covariance_derivatives(ard):
    """_dknot_mats / dsqexp_dx2 against central differences of the covariance matrices the
    gradient functions build (O._cov_mats) in U[k, c], times the chain factor."""
    cov_fun = "ard" if ard else "sqexp"
    P = O.make_gaussian_problem("C2", n=40, m=9)
    cp = _ard_par(3) if ard else P["cov_par"]
    U = P["U"].copy()
    U[2] = P["X"][5]    # a knot on a data row (the cross matrix adds nothing there)
    b = O.knot_bounds_of(P["X"])
    lnames = O.lnames_for(cov_fun, 3)
    for k, c in [(0, 0), (2, 1), (8, 2)]:
        d12, d22 = O._dknot_mats(k, c, cp, U, P["X"], b, ard)
        Up, Um = U.copy(), U.copy()
        Up[k, c] += H
        Um[k, c] -= H
        p12, p22 = O._cov_mats(cp, cov_fun, Up, P["X"], P["delta"], lnames)
        m12, m22 = O._cov_mats(cp, cov_fun, Um, P["X"], P["delta"], lnames)
        chain = (b[c, 1] - b[c, 0]) / ((U[k, c] - b[c, 0]) * (b[c, 1] - U[k, c]) + 1e-4)
        scale = float(cp["sigma"]) ** 2 * chain
        assert np.max(np.abs((p12 - m12) / (2 * H) * chain - d12)) < 1e-8 * scale
        assert np.max(np.abs((p22 - m22) / (2 * H) * chain - d22)) < 1e-8 * scale
        assert np.count_nonzero(d12[:, np.arange(9) != k]) == 0


@pytest.mark.parametrize("cov_fun,knot_opt", [("sqexp", None), ("ard", None), ("sqexp", [2, 5])])
def test_bernoulli_closure_with_poisson_derivatives_is_the_poisson_oracle(cov_fun, knot_opt):
    P = O.make_poisson_problem(n=90, m=6)
    cp = P["cov_par"] if cov_fun == "sqexp" else _ard_par(5)
    ff = P["f0"] + 0.05 * np.cos(np.arange(90))
    a = P["a"]
    ref = O.dlogq_dcov_par(cp, cov_fun, P["U"], P["X"], P["y"], ff, P["mu"], a, P["delta"],
                           dcov_fun_dknot=cov_fun, knot_opt=knot_opt)
    got = B.dlogq_dcov_par_with(lambda f, y: O.dlog_py_dff_pois(f, y, a),
                                lambda f, y: O.d2log_py_dff_pois(f, a),
                                lambda f, y: O.d3log_py_dff_pois(f, a),
                                cp, cov_fun, P["U"], P["X"], P["y"], ff, P["mu"], P["delta"],
                                dcov_fun_dknot=cov_fun, knot_opt=knot_opt)
    assert list(got["gradient"].items()) == list(ref["gradient"].items())
    assert np.array_equal(got["knot_gradient"], ref["knot_gradient"])
    assert np.array_equal(got["trans_knot"], ref["trans_knot"])
    assert np.count_nonzero(got["knot_gradient"]) == (6 if knot_opt is None else 2) * 5
    # and without knots the Bernoulli entry point is what it was
    Q = B.problem("sqexp_300_20")
    f = 0.3 * np.sin(np.arange(300))
    g0 = B.dlogq_dcov_par(Q["cov_par"], "sqexp", Q["U"], Q["X"], Q["y"], f, Q["mu"], Q["delta"])
    g1 = B.dlogq_dcov_par(Q["cov_par"], "sqexp", Q["U"], Q["X"], Q["y"], f, Q["mu"], Q["delta"],
                          dcov_fun_dknot="sqexp", knot_opt=[1])
    assert list(g0) == ["gradient"] and g0["gradient"] == g1["gradient"]
