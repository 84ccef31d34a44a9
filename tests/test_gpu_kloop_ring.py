"""The ring k-loop of VI's gradient contraction (k_contract<.., VIF>, con_tile's RING).

The operands of the product K P' are staged in LDS as a ring of four 8-deep sub-stages: a wave
prefetches the first fragments of sub-stage j + 1 while it runs sub-stage j, stores j + 2 and
loads j + 3.  A wrong ring index, staging set or fragment carried over the barrier gives a wrong
product, so objective, theta-gradient and knot gradient are compared with the literal oracle
(oracle/sgp_oracle.py) at the tolerance of test_gpu_vi.py (1e-6 relative, floor 1) at the shapes
where the ring can go wrong:

  m = 128          16 sub-stages: prologue, one wrap of the ring, drain
  m = 130          m_p = 256: a second column tile whose columns are almost all zero padding
  m = 1024         128 sub-stages, eight column tiles (n = 1000: eight row tiles, the last padded)
  n = 129, 257     a second and a third row tile, almost all padding
  d = 3 sqexp and d = 8 ARD (the <8> kernel), d = 12 ARD (the <32> kernel)

Every case with knot gradients runs both instantiations: vi_eval the one without the knot
epilogue, delbo_dcov_par the one with it.  The literal oracle costs m d n Python calls for the
knot gradient, so at d = 8 and d = 12 it is asked for the first, last and tile-edge knots only
(the GPU computes all; those rows are compared), and at m = 1024 the knot gradient is left
out: the KNOT kernel's k-loop is the same code as at m = 130.  One case runs on three row
shards through the multi-device context on device 0, and one checks that two evaluations give
the same bits.
"""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest

from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-6


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def _ard_problem(seed, n, m, d):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, size=(n, d))
    U = rng.uniform(0, 10, size=(m, d))
    y = np.sin(X).sum(axis=1) / math.sqrt(d) + rng.normal(0, 0.5, size=n)
    ls = 2.0 * math.sqrt(d)
    cp = OrderedDict([("sigma", 1.2)] + [(f"l{c + 1}", ls * (1.0 + 0.02 * c)) for c in range(d)] +
                     [("tau", 0.5)])
    return dict(X=X, U=U, y=y, mu=np.full(n, y.mean()), cov_par=cp, cov_fun="ard", delta=1e-6)


SUBSET = [1, 2, 64, 65, 127, 128, 129, 130]   # 1-based: first, last and tile-edge knots


# name -> (problem, knots whose gradient is compared: None = none, a list, or "all")
@functools.lru_cache(maxsize=None)
def _problem(name):
    if name == "m128_n129_d3_sqexp":
        return O.make_gaussian_problem("C2", n=129, m=128), "all"
    if name == "m130_n257_d8_ard":
        return _ard_problem(71, 257, 130, 8), SUBSET
    if name == "m130_n129_d12_ard":
        return _ard_problem(72, 129, 130, 12), SUBSET
    if name == "m1024_n1000_d8_ard":
        return O.make_gaussian_problem("C3", n=1000, m=1024), None
    raise KeyError(name)


def _knot_rows(P, knots):
    """Flat indices of the compared knot-gradient entries."""
    m, d = P["U"].shape
    ks = np.arange(m) if knots == "all" else np.asarray(knots) - 1
    return (ks[:, None] * d + np.arange(d)[None, :]).reshape(-1)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle's objective, gradient and (where compared) knot gradient, computed once and
    shared by the tests that use the problem."""
    P, knots = _problem(name)
    cp, fun = P["cov_par"], P["cov_fun"]
    kw = {}
    if knots is not None:
        kw = dict(dcov_fun_dknot=fun, knot_opt=None if knots == "all" else knots)
    ref = O.delbo_dcov_par(cp, fun, P["U"], P["X"], P["y"], P["mu"], P["delta"], **kw)
    o_ref = O.elbo_eval(cp, fun, P["U"], P["X"], P["y"], P["mu"], P["delta"])
    return o_ref, ref


CASES = ["m128_n129_d3_sqexp", "m130_n257_d8_ard", "m130_n129_d12_ard", "m1024_n1000_d8_ard"]


@pytest.mark.parametrize("name", CASES)
def test_against_oracle(sgp, name):
    P, knots = _problem(name)
    o_ref, ref = _reference(name)
    cp, fun = P["cov_par"], P["cov_fun"]
    obj, grad = sgp.vi_eval(cp, fun, P["U"], P["X"], P["y"], P["mu"], P["delta"])
    e_obj = abs(obj - o_ref) / abs(o_ref)
    e_grad = max(abs(grad[k] - ref["gradient"][k]) / max(1.0, abs(ref["gradient"][k])) for k in cp)
    e_knot = 0.0
    if knots is not None:
        got = sgp.delbo_dcov_par(cp, fun, True, "dsqexp_dx2" if fun == "sqexp" else
                                 "dsqexp_dx2_ard", None, P["U"], P["X"], P["y"], None, P["mu"],
                                 True, P["delta"])
        r = _knot_rows(P, knots)
        e_knot = _rel(np.asarray(got["knot_gradient"]).reshape(-1)[r],
                      np.asarray(ref["knot_gradient"]).reshape(-1)[r])
        e_grad = max(e_grad, max(abs(got["gradient"][k] - ref["gradient"][k]) /
                                 max(1.0, abs(ref["gradient"][k])) for k in cp))
    print(f"\n[kloop_ring] {name}: obj {e_obj:.3e} grad {e_grad:.3e} knot {e_knot:.3e}")
    assert e_obj < RTOL
    assert e_grad < RTOL
    assert e_knot < RTOL


def test_three_row_shards_on_one_device(sgp):
    """n = 257 over devices = [0, 0, 0]: shards of one row tile each, mostly padding, with knot
    gradients."""
    name = "m130_n257_d8_ard"
    P, knots = _problem(name)
    o_ref, ref = _reference(name)
    r = _knot_rows(P, knots)
    cp = P["cov_par"]
    th = np.array(list(cp.values()))
    g_ref = np.array([ref["gradient"][k] for k in cp])
    bounds = O.knot_bounds_of(P["X"])
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=130, devices=[0, 0, 0]) as c:
        c.enable_knot_grad(True)
        obj, grad = c.eval_vi(th, P["cov_fun"], P["U"], P["delta"])
        kg = c.knot_gradient(bounds)
    e = (abs(obj - o_ref) / abs(o_ref), _rel(grad, g_ref),
         _rel(np.asarray(kg).reshape(-1)[r], np.asarray(ref["knot_gradient"]).reshape(-1)[r]))
    print(f"\n[kloop_ring] three shards: obj {e[0]:.3e} grad {e[1]:.3e} knot {e[2]:.3e}")
    assert max(e) < RTOL


@pytest.mark.parametrize("name", ["m130_n257_d8_ard", "m1024_n1000_d8_ard"])
def test_repeat_is_bit_identical(sgp, name):
    """Two evaluations at one theta: the ring leaves nothing behind (a fragment or a staging
    set carried into the next tile or launch) that the second evaluation could pick up."""
    P, knots = _problem(name)
    th = np.array(list(P["cov_par"].values()))
    m = P["U"].shape[0]
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=m) as c:
        if knots is not None:
            c.enable_knot_grad(True)
        outs = []
        for _ in range(2):
            obj, grad = c.eval_vi(th, P["cov_fun"], P["U"], P["delta"])
            kg = np.asarray(c.knot_gradient(None)) if knots is not None else np.zeros(0)
            outs.append((np.float64(obj), np.array(grad, dtype=np.float64), kg.copy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
