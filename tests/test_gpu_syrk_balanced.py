"""The work-balanced SYRK plan of VI's S = K12^T K12 on the GPU (k_syrk_bal, k_syrk_reduce_bal).

S is read from sgp_vi_phase1's red1, in both layouts (full mp x mp, and the packed lower
64-blocks), and compared element by element with numpy's K^T K on the K12 that sgp_make_cov
returns.  Both sides are sums of n non-negative products, each within gamma_n of the exact sum,
so |dS_jk| <= 2 n 2^-53 S_jk.  Shapes: the headline's 8 column panels with full, ragged and few
row steps, the smallest panel count the plan accepts (3), an odd one (5) and padded knot columns;
each asserts through sgp_diag_syrk_plan that the work-balanced plan is the one that ran, and
m = 256 that it is not.  The VI objective and gradient at two of the shapes against
oracle/adjoint_chunked.eval_vi (1e-9 / 1e-7, the bars of tests/test_gpu_configs.py at full
size), and two evaluations on one context give bit-identical red1.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAN_PACKED, PLAN_TWO_CHUNKS, PLAN_BALANCED, PLAN_S256 = 0, 1, 2, 3
# (n, m, d): d = 3 is C2's sqexp problem, otherwise C3's ARD one
SHAPES = [(4096, 1024, 8), (4100, 1024, 8), (1000, 1024, 8), (6000, 384, 3), (6000, 640, 5),
          (3000, 1000, 8)]


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _plan(n, m):
    from sparsergps_amd import _lib
    plan, nwg = C.c_int(-1), C.c_int(-1)
    tb, tp = C.c_double(0.0), C.c_double(0.0)
    _lib.check(_lib.lib().sgp_diag_syrk_plan(n, m, C.byref(plan), C.byref(nwg), C.byref(tb),
                                             C.byref(tp)))
    return plan.value, nwg.value, tb.value, tp.value


_CACHE = {}


def _case(sgp, n, m, d):
    """The problem, the reference S (computed once per shape) and both red1 layouts."""
    import torch
    from sparsergps_amd.workloads import make_gaussian_problem
    key = (n, m, d)
    if key in _CACHE:
        return _CACHE[key]
    P = make_gaussian_problem("C2" if d == 3 else "C3", n=n, m=m, d=None if d == 3 else d)
    th = np.array(list(P["cov_par"].values()))
    if P["cov_fun"] == "ard":
        K = sgp.make_cov_mat_ardC(P["X"], P["U"], P["cov_par"], "ard", P["delta"],
                                  [f"l{c + 1}" for c in range(d)])
    else:
        K = sgp.make_cov_matC(P["X"], P["U"], P["cov_par"], P["cov_fun"], P["delta"])
    assert K.shape == (n, m) and K.min() >= 0.0
    S_ref = K.T @ K
    red = {}
    with sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=m) as ctx:
        for packed in (False, True):
            ctx.set_packed_reduction(packed)
            for rep in range(2):
                buf = torch.full((ctx.vi_red1_count(m),), float("nan"), dtype=torch.float64,
                                 device="cuda")
                ctx.vi_phase1(th, P["cov_fun"], P["U"], P["delta"], buf.data_ptr())
                torch.cuda.synchronize()
                red[(packed, rep)] = buf.cpu().numpy()
                # finish the evaluation: the layout cannot change inside one
                red2 = torch.zeros(ctx.vi_red2_count(P["cov_fun"]), dtype=torch.float64,
                                   device="cuda")
                torch.cuda.synchronize()
                ctx.vi_phase2(buf.data_ptr(), n, red2.data_ptr())
                ctx.vi_finish(red2.data_ptr(), th.size)
    _CACHE[key] = (P, th, S_ref, red)
    return _CACHE[key]


def _unpack(blocks, mp):
    """Lower triangle (by 16 x 16 fragments) of S from its packed lower 64-blocks."""
    nb64 = mp // 64
    S = np.full((mp, mp), np.nan)
    k = 0
    for rp in range(nb64):
        for cp in range(rp + 1):
            S[rp * 64:(rp + 1) * 64, cp * 64:(cp + 1) * 64] = blocks[k * 4096:(k + 1) * 4096].reshape(64, 64)
            k += 1
    return S


def _check_S(S_got, S_ref, n, m, what):
    low = np.tril_indices(m)
    got, ref = S_got[:m, :m][low], S_ref[low]
    err = np.abs(got - ref)
    bound = 2.0 * n * 2.0 ** -53 * ref
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: max |dS| / (2 n 2^-53 S) = {worst:.3e}")
    assert np.all(np.isfinite(got)), what
    assert np.all(err <= bound), f"{what}: {worst:.3e} of the bound"


@pytest.mark.parametrize("n,m,d", SHAPES)
def test_s_matches_numpy_both_layouts(sgp, n, m, d):
    plan, nwg, tb, tp = _plan(n, m)
    assert plan == PLAN_BALANCED and 0 < nwg <= 512 and tb < 0.98 * tp, (plan, nwg, tb, tp)
    P, th, S_ref, red = _case(sgp, n, m, d)
    mp = -(-m // 128) * 128
    full = red[(False, 0)][:mp * mp].reshape(mp, mp)
    _check_S(full, S_ref, n, m, f"full ({n}, {m}, {d})")
    np.testing.assert_array_equal(full, full.T)
    # knot columns past m are zero rows and columns of S
    assert not full[m:, :].any() and not full[:, m:].any()
    npk = (mp // 64) * (mp // 64 + 1) // 2 * 4096
    pk = _unpack(red[(True, 0)][:npk], mp)
    _check_S(pk, S_ref, n, m, f"packed ({n}, {m}, {d})")
    # the two layouts hold the same sums
    low = np.tril_indices(mp)
    np.testing.assert_array_equal(pk[low], full[low])


def test_small_m_keeps_its_kernel(sgp):
    plan, nwg, tb, tp = _plan(3000, 256)
    assert plan == PLAN_S256 and tb == 0.0
    P, th, S_ref, red = _case(sgp, 3000, 256, 3)
    _check_S(red[(False, 0)][:256 * 256].reshape(256, 256), S_ref, 3000, 256, "full (3000, 256, 3)")


@pytest.mark.parametrize("n,m,d", SHAPES)
def test_second_evaluation_is_bit_identical(sgp, n, m, d):
    P, th, S_ref, red = _case(sgp, n, m, d)
    for packed in (False, True):
        np.testing.assert_array_equal(red[(packed, 0)], red[(packed, 1)])


@pytest.mark.parametrize("n,m,d", [(4096, 1024, 8), (6000, 384, 3)])
def test_vi_objective_and_gradient(sgp, n, m, d):
    from oracle import adjoint_chunked as AC
    assert _plan(n, m)[0] == PLAN_BALANCED
    P, th, S_ref, red = _case(sgp, n, m, d)
    o, g = AC.eval_vi(P["cov_fun"], th, P["X"], P["y"], P["mu"], P["U"], P["delta"])
    obj, grad = sgp.vi_eval(P["cov_par"], P["cov_fun"], P["U"], P["X"], P["y"], P["mu"], P["delta"])
    grad = np.asarray(list(grad.values()), dtype=np.float64)
    rel_o = abs(obj - o) / abs(o)
    rel_g = float(np.max(np.abs(grad - g) / np.maximum(1.0, np.abs(g))))
    print(f"({n}, {m}, {d}): objective rel {rel_o:.3e}, gradient rel {rel_g:.3e}")
    assert rel_o < 1e-9
    assert rel_g < 1e-7
