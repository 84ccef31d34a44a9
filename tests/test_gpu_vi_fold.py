"""VI's folded adjoint on the GPU: G = (r/z) u^T + K P', P' = P - u u^T / z.

The gradient contraction runs without the K u fold in its k-loop and, with knots fixed, without
the column sums C_j = sum_i G_ij K_ij in its epilogue; sum_j C_j, sum_j u~_jc^2 C_j and
alpha^T alpha are formed from the reduced m x m operands (S, t, r^T r, P') and enter once in
sgp_vi_finish (with knot gradients the epilogue keeps its column sums and only alpha^T alpha
comes from there).  Objective, gradient and knot gradient are compared with the literal oracle
(oracle/sgp_oracle.py) at the tolerances of test_gpu_vi.py / test_gpu_knots.py (1e-6 relative,
floor 1), at the smallest shapes where the change can go wrong: two row and two column tiles with
padding, the <8> kernel with every coordinate column used, the <32> kernel with two coordinate
chunks, n < m, knot gradients, data rows equal to knots (tau's coincidence sums read r/z and P'),
the objective alone, rows split over two contexts (a replicated term added per shard would show),
and a high-signal problem (alpha^T alpha = (r^T r - 2 u^T t + u^T S u) / z^2 cancels there).

FITC and Laplace keep their kernels: their outputs are compared bit for bit with those recorded
from the library before this change (tests/golden/fold_fitc_laplace_bits.npz, written by
`_bit_outputs` below on that library).
"""
import functools
import math
import os
from collections import OrderedDict

import numpy as np
import pytest

from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "fold_fitc_laplace_bits.npz")


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def _ard_par(d, l0=1.3, dl=0.4, sigma=1.2, tau=0.45):
    return OrderedDict([("sigma", sigma)] + [(f"l{c + 1}", l0 + dl * c) for c in range(d)] +
                       [("tau", tau)])


def _random_problem(seed, n, m, d, cov_fun):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, size=(n, d))
    U = rng.uniform(0, 10, size=(m, d))
    y = np.sin(X).sum(axis=1) / math.sqrt(d) + rng.normal(0, 0.5, size=n)
    mu = np.full(n, y.mean())
    ls = 2.0 * math.sqrt(d)
    if cov_fun == "ard":
        cp = _ard_par(d, ls, 0.02 * ls, tau=0.5)
    else:
        cp = OrderedDict([("sigma", 1.2), ("l", ls), ("tau", 0.5)])
    return dict(X=X, U=U, y=y, mu=mu, cov_par=cp, cov_fun=cov_fun, delta=1e-6)


def _two_tile_problem(cov_fun):
    """n = 300, m = 130, d = 3: two row tiles, two column tiles, padding in both directions."""
    P = O.make_gaussian_problem("C2", n=300, m=130)
    if cov_fun == "ard":
        P["cov_par"], P["cov_fun"] = _ard_par(3), "ard"
    return P


@functools.lru_cache(maxsize=None)
def _two_tile_reference(cov_fun):
    """The oracle's objective, gradient and knot gradient of _two_tile_problem, computed once
    (the literal knot gradient loops over all m d knot coordinates: seconds on the CPU)."""
    P = _two_tile_problem(cov_fun)
    ref = O.delbo_dcov_par(P["cov_par"], cov_fun, P["U"], P["X"], P["y"], P["mu"], P["delta"],
                           dcov_fun_dknot=cov_fun)
    o_ref = O.elbo_eval(P["cov_par"], cov_fun, P["U"], P["X"], P["y"], P["mu"], P["delta"])
    return o_ref, ref


def _check(sgp, P, knots=False, label="", reference=None):
    cp, fun = P["cov_par"], P["cov_fun"]
    if reference is not None:
        o_ref, ref = reference
    else:
        ref = O.delbo_dcov_par(cp, fun, P["U"], P["X"], P["y"], P["mu"], P["delta"],
                               **({"dcov_fun_dknot": fun} if knots else {}))
        o_ref = O.elbo_eval(cp, fun, P["U"], P["X"], P["y"], P["mu"], P["delta"])
    obj, grad = sgp.vi_eval(cp, fun, P["U"], P["X"], P["y"], P["mu"], P["delta"])
    e_obj = abs(obj - o_ref) / abs(o_ref)
    e_grad = max(abs(grad[k] - ref["gradient"][k]) / max(1.0, abs(ref["gradient"][k])) for k in cp)
    e_knot = 0.0
    if knots:
        got = sgp.delbo_dcov_par(cp, fun, True, "dsqexp_dx2" if fun == "sqexp" else
                                 "dsqexp_dx2_ard", None, P["U"], P["X"], P["y"], None, P["mu"],
                                 True, P["delta"])
        e_knot = _rel(got["knot_gradient"], ref["knot_gradient"])
        e_grad = max(e_grad, max(abs(got["gradient"][k] - ref["gradient"][k]) /
                                 max(1.0, abs(ref["gradient"][k])) for k in cp))
    print(f"\n[vi_fold] {label}: obj {e_obj:.3e} grad {e_grad:.3e} knot {e_knot:.3e}")
    assert e_obj < RTOL
    assert e_grad < RTOL
    assert e_knot < RTOL


def test_two_tiles_both_ways_sqexp(sgp):
    _check(sgp, _two_tile_problem("sqexp"), label="case 1",
           reference=_two_tile_reference("sqexp"))


def test_every_coordinate_column_ard_d8(sgp):
    """n = 257, m = 128, d = 8, ARD: the <8> kernel with all 8 coordinate columns in use."""
    _check(sgp, _random_problem(31, 257, 128, 8, "ard"), label="case 2")


def test_two_coordinate_chunks_ard_d12(sgp):
    """n = 200, m = 129, d = 12, ARD: the <32> kernel, two chunks of coordinates."""
    _check(sgp, _random_problem(32, 200, 129, 12, "ard"), label="case 3")


def test_fewer_rows_than_knots_d1(sgp):
    """n = 100 < m = 140, d = 1 (knots on a jittered grid, l of the order of their spacing:
    140 random knots on a line leave K22 singular to working precision)."""
    P = _random_problem(33, 100, 140, 1, "sqexp")
    rng = np.random.default_rng(133)
    P["U"] = (np.linspace(0, 10, 140) + rng.uniform(-0.02, 0.02, size=140)).reshape(140, 1)
    P["cov_par"]["l"] = 0.1
    _check(sgp, P, label="case 4")


@pytest.mark.parametrize("cov_fun", ["sqexp", "ard"])
def test_knot_gradients(sgp, cov_fun):
    """Case 1's shape with knot gradients: the KNOT instantiation without the K u fold (its
    column sums stay in the epilogue, so the m x m column terms must stay out of the finish)."""
    _check(sgp, _two_tile_problem(cov_fun), knots=True, label=f"case 5 {cov_fun}",
           reference=_two_tile_reference(cov_fun))


@pytest.mark.parametrize("knots", [False, True])
def test_rows_equal_to_knots(sgp, knots):
    """Several data rows equal knots: tau's coincidence sums recompute G from r/z and P'."""
    P = O.make_gaussian_problem("C2", n=200, m=40)
    U = P["U"].copy()
    U[0], U[5], U[39] = P["X"][3], P["X"][150], P["X"][199]
    P["U"] = U
    _check(sgp, P, knots=knots, label=f"case 6 knots={knots}")


def test_objective_only(sgp):
    P = O.make_gaussian_problem("C3", n=300, m=130)
    obj, _ = sgp.vi_eval(P["cov_par"], P["cov_fun"], P["U"], P["X"], P["y"], P["mu"], P["delta"],
                         obj_only=True)
    o_ref = O.elbo_eval(P["cov_par"], P["cov_fun"], P["U"], P["X"], P["y"], P["mu"], P["delta"])
    assert abs(obj - o_ref) / abs(o_ref) < RTOL


@pytest.mark.parametrize("cov_fun", ["sqexp", "ard"])
def test_rows_split_over_two_contexts(sgp, cov_fun):
    """The phase API on two contexts of one device (red1 / red2 summed between the phases) and
    the in-library context with devices = [0, 0], with knot gradients: the terms formed from
    the reduced S, t and r^T r enter once, not once per shard."""
    import torch
    n, m = 300, 130
    P = _two_tile_problem(cov_fun)
    cp = P["cov_par"]
    th = np.array(list(cp.values()))
    o_ref, ref = _two_tile_reference(cov_fun)
    g_ref = np.array([ref["gradient"][k] for k in cp])
    bounds = O.knot_bounds_of(P["X"])
    cut = 170
    parts = [slice(0, cut), slice(cut, n)]
    ctxs = [sgp.SparseGPContext(P["X"][s], P["y"][s], P["mu"][s], m_max=m) for s in parts]
    try:
        for c in ctxs:
            c.enable_knot_grad(True)
        n1 = ctxs[0].vi_red1_count(m)
        n2 = ctxs[0].vi_red2_count(cov_fun) + ctxs[0].knot_red_extra(m)
        red1 = [torch.zeros(n1, dtype=torch.float64, device="cuda") for _ in ctxs]
        red2 = [torch.zeros(n2, dtype=torch.float64, device="cuda") for _ in ctxs]
        torch.cuda.synchronize()
        for c, r in zip(ctxs, red1):
            c.vi_phase1(th, cov_fun, P["U"], P["delta"], r.data_ptr())
        torch.cuda.synchronize()
        s1 = red1[0] + red1[1]
        torch.cuda.synchronize()
        for c, r in zip(ctxs, red2):
            c.vi_phase2(s1.data_ptr(), n, r.data_ptr())
        torch.cuda.synchronize()
        s2 = red2[0] + red2[1]
        torch.cuda.synchronize()
        obj, grad = ctxs[0].vi_finish(s2.data_ptr(), th.size)
        kg = ctxs[0].knot_gradient(bounds)
    finally:
        for c in ctxs:
            c.close()
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=m, devices=[0, 0]) as c:
        c.enable_knot_grad(True)
        obj_m, grad_m = c.eval_vi(th, cov_fun, P["U"], P["delta"])
        kg_m = c.knot_gradient(bounds)
    kr = np.asarray(ref["knot_gradient"]).reshape(-1)
    for name, o, g, k in (("phases", obj, grad, kg), ("devices=[0,0]", obj_m, grad_m, kg_m)):
        e = (abs(o - o_ref) / abs(o_ref), _rel(g, g_ref), _rel(np.asarray(k).reshape(-1), kr))
        print(f"\n[vi_fold] case 8 {cov_fun} {name}: obj {e[0]:.3e} grad {e[1]:.3e} knot {e[2]:.3e}")
        assert max(e) < RTOL, name


def test_high_signal_alpha_norm(sgp):
    """y = the model's own mean plus noise of relative size 1e-4, at a theta whose tau matches
    that noise: r^T r, 2 u^T t and u^T S u nearly cancel in alpha^T alpha."""
    rng = np.random.default_rng(41)
    n, d = 300, 2
    grid = np.stack(np.meshgrid(np.linspace(0.7, 9.3, 7), np.linspace(0.8, 9.2, 6)), -1)
    U = grid.reshape(-1, 2) + rng.uniform(-0.3, 0.3, size=(42, 2))   # K22 well conditioned
    X = rng.uniform(0, 10, size=(n, d))
    cp = OrderedDict([("sigma", 1.5), ("l", 1.5), ("tau", 0.0)])
    K12 = O.make_cov_matC(X, U, cp, "sqexp", 0.0)
    f = K12 @ rng.normal(0, 0.3, size=42)   # in the span of the knots' kernel functions
    noise = 1e-4 * float(np.sqrt(np.mean(f * f)))
    y = f + rng.normal(0, noise, size=n)
    cp["tau"] = noise
    P = dict(X=X, U=U, y=y, mu=np.zeros(n), cov_par=cp, cov_fun="sqexp", delta=1e-6)
    _check(sgp, P, label="case 9")


# ---------------------------------------------------------------- FITC / Laplace: unchanged bits
def _bit_outputs(sgp):
    """One FITC and one Laplace evaluation per contraction instantiation they use, at the small
    shapes of their own tests."""
    out = {}
    P = O.make_gaussian_problem("C2", n=300, m=20)
    th = np.array(list(P["cov_par"].values()))
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=20) as ctx:
        o, g = ctx.eval_fitc(th, "sqexp", P["U"], P["delta"])
        out["fitc_sqexp"] = np.concatenate([[o], g])
    P = O.make_gaussian_problem("C3", n=350, m=130)
    th = np.array(list(P["cov_par"].values()))
    U = P["U"].copy()
    U[2] = P["X"][11]
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=130) as ctx:
        ctx.enable_knot_grad(True)
        o, g = ctx.eval_fitc(th, "ard", U, P["delta"])
        out["fitc_ard_knots"] = np.concatenate([[o], g, ctx.knot_gradient(None)])
    Q = _random_problem(34, 300, 24, 12, "ard")
    th = np.array(list(Q["cov_par"].values()))
    with sgp.SparseGPContext(Q["X"], Q["y"], Q["mu"], m_max=24) as ctx:
        o, g = ctx.eval_fitc(th, "ard", Q["U"], Q["delta"])
        out["fitc_ard_d12"] = np.concatenate([[o], g])
    P = O.make_poisson_problem(n=400, m=25)
    th = np.array(list(P["cov_par"].values()))
    for knots in (False, True):
        with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=25) as ctx:
            if knots:
                ctx.enable_knot_grad(True)
            ctx.lap_set_f(P["f0"])
            o, g, it = ctx.eval_laplace(th, "sqexp", P["U"], P["delta"], P["a"], 1e-5, 1000)
            extra = ctx.knot_gradient(None) if knots else []
            out["laplace_knots" if knots else "laplace"] = np.concatenate([[o, it], g, extra])
    return out


def test_fitc_and_laplace_bits_unchanged(sgp):
    got = _bit_outputs(sgp)
    with np.load(GOLDEN) as z:
        assert sorted(z.files) == sorted(got)
        for k in z.files:
            assert np.array_equal(z[k], got[k]), (k, float(np.max(np.abs(z[k] - got[k]))))
