"""The batch's knot gradient (sgp_batch_eval_vi_knots) without a GPU: symbols,
prototypes and header text, the new SGP_EINVAL cases (sgp_diag_batch_knot_args is the very check
the entry point runs first), the refusals of the Python surface, and the lockstep driver with
xu_opt = "simultaneous" on a fake batch that evaluates with the CPU oracle."""
import ctypes as C
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

from oracle import drivers as OD
from oracle import sgp_oracle as O
from test_batch_abi import FakeBatch, _decl_commas, _good

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"sgp_batch_eval_vi_knots": 16, "sgp_diag_batch_knot_args": 6,
         "sgp_diag_batch_knot_timing": 3}


@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    return _lib.lib()


def test_symbols_prototypes_and_header(lib):
    from sparsergps_amd import _lib
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    diag = open(os.path.join(ROOT, "include", "sgp_diag.h")).read()
    for name, n in NARGS.items():
        assert hasattr(lib, name), name
        assert _lib.PROTOTYPES[name][0] is C.c_int and len(_lib.PROTOTYPES[name][1]) == n, name
        src = diag if name.startswith("sgp_diag_") else text
        assert _decl_commas(src, name) == n - 1, name
    # sgp_batch_eval_vi's arguments, then bounds and grad_knot
    assert _lib.PROTOTYPES["sgp_batch_eval_vi_knots"][1][:14] == \
        _lib.PROTOTYPES["sgp_batch_eval_vi"][1]
    assert len(_lib.PROTOTYPES["sgp_diag_batch_args"][1]) == 23
    doc = text[text.index("sgp_batch_eval_vi with the knot gradient"):
               text.index("int sgp_batch_eval_vi_knots(")]
    for cite in ("vi_functions.R:425-593", "covariance_function_derivatives.R:178-302",
                 "optimize_gp.R:317-333, 396-412", "Q8", "Q16", "bit-identical"):
        assert cite in doc, cite
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", text) and lib.sgp_abi_version() == 1


def _knot_check(lib, d=2, B=3, flags=0, active=None, bounds="good", grad_knot="good"):
    from sparsergps_amd import _lib
    if isinstance(bounds, str):
        bounds = np.tile(np.concatenate([np.zeros(d), np.ones(d)]), B)
    if isinstance(grad_knot, str):
        grad_knot = np.zeros(64 * d * B)
    act = None if active is None else active.ctypes.data_as(_lib.c_ubyte_p)
    return lib.sgp_diag_batch_knot_args(d, B, flags, act,
                                        None if bounds is None else _lib.dptr(bounds),
                                        None if grad_knot is None else _lib.dptr(grad_knot))


def test_knot_arguments(lib):
    from sparsergps_amd import _lib
    assert _knot_check(lib) == _lib.SGP_OK
    assert _knot_check(lib, bounds=None) == _lib.SGP_OK                 # the raw gradient
    assert _knot_check(lib, d=32, B=1, flags=_lib.SGP_FLAG_R_DET) == _lib.SGP_OK
    assert _knot_check(lib, grad_knot=None) == _lib.SGP_EINVAL
    assert b"grad_knot" in lib.sgp_last_error()
    assert _knot_check(lib, flags=_lib.SGP_FLAG_OBJ_ONLY) == _lib.SGP_EINVAL
    assert b"SGP_FLAG_OBJ_ONLY" in lib.sgp_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        bd = np.tile(np.array([0.0, 0.0, 1.0, 1.0]), 3)
        bd[4 + 3] = bad                                                 # problem 1, upper, c = 1
        assert _knot_check(lib, bounds=bd) == _lib.SGP_EINVAL
        assert b"problem 1's bounds[1, 1]" in lib.sgp_last_error(), lib.sgp_last_error()
        # an inactive problem's bounds are not read
        assert _knot_check(lib, bounds=bd, active=np.array([1, 0, 1], dtype=np.uint8)) == _lib.SGP_OK


def test_null_handle(lib):
    from sparsergps_amd import _lib
    a = _good()
    q = lambda w: w.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    gk = np.zeros(a["U"].size)
    st = lib.sgp_batch_eval_vi_knots(None, 0, _lib.dptr(a["theta"]), 3, _lib.dptr(a["U"]),
                                     q(a["uoff"]), q(a["m"]), 1e-6, 0, None, _lib.dptr(a["obj"]),
                                     _lib.dptr(a["grad"]), 3,
                                     a["status"].ctypes.data_as(_lib.c_int_p), None, _lib.dptr(gk))
    assert st == _lib.SGP_EINVAL and b"sgp_batch_eval_vi_knots" in lib.sgp_last_error()
    assert lib.sgp_diag_batch_knot_timing(None, 1, None) == _lib.SGP_EINVAL


def test_python_surface():
    import sparsergps_amd as S
    for meth in ("eval_vi_knots", "knot_bounds", "knot_stage_ms"):
        assert callable(getattr(S.SparseGPBatch, meth))
    with pytest.raises(ValueError, match="knot gradients"):
        S.norm_grad_ascent_vi_batch([], "sqexp", [], [], dcov_fun_dknot="sqexp")
    probs = [(np.zeros((8, 2)), np.zeros(8), None)] * 2
    cp = OrderedDict([("sigma", 1.0), ("l1", 1.0), ("l2", 1.0), ("tau", 0.5)])
    xu = np.zeros((2, 2))
    with pytest.raises(ValueError, match="simultaneous.*sqexp"):                       # Q10
        S.optimize_gp_batch(probs, "ard", cp, xu, xu_opt="simultaneous")
    with pytest.raises(ValueError, match="simultaneous.*sqexp"):
        S.cross_validate_gp(np.zeros(8), np.zeros((8, 2)), "ard", cp, xu, folds=2,
                            xu_opt="simultaneous")
    for bad in ("oat", "random"):
        with pytest.raises(ValueError, match=f"batches do not support.*{bad}"):
            S.optimize_gp_batch(probs, "sqexp", cp, xu, xu_opt=bad)
        with pytest.raises(ValueError, match=f"batches do not support.*{bad}"):
            S.cross_validate_gp(np.zeros(8), np.zeros((8, 2)), "sqexp", cp, xu, folds=2,
                                xu_opt=bad)
        with pytest.raises(ValueError, match="batches do not support"):
            S.norm_grad_ascent_vi_batch([], "sqexp", [], [], xu_opt=bad)
    with pytest.raises(ValueError, match="xu_opt"):
        S.optimize_gp_batch(probs, "sqexp", cp, xu, xu_opt="moving")


# ------------------------------------------------------------------ the lockstep driver's host logic
class FakeKnotBatch(FakeBatch):
    """FakeBatch with eval_vi_knots from the oracle's knot branch."""

    def eval_vi_knots(self, cov_pars, cov_fun, xus, delta=1e-6, active=None, bounds="data",
                      r_det=False):
        obj, grads, kgs = np.full(self.B, np.nan), [None] * self.B, [None] * self.B
        ran = []
        for b, (xy, y, mu) in enumerate(self.problems):
            if active is not None and not active[b]:
                continue
            ran.append(b)
            # the driver passes knot_bounds of the problem's own rows: the oracle's own bounds
            np.testing.assert_array_equal(bounds[b], O.knot_bounds_of(xy))
            obj[b] = O.elbo_eval(cov_pars[b], cov_fun, xus[b], xy, y, mu, delta)
            r = O.delbo_dcov_par(cov_pars[b], cov_fun, xus[b], xy, y, mu, delta, cov_fun)
            grads[b], kgs[b] = r["gradient"], r["knot_gradient"]
            self.last[b] = (OrderedDict(cov_pars[b]), np.array(xus[b]), delta)
        self.calls.append(ran)
        return obj, grads, kgs, np.zeros(self.B, dtype=np.int32)

    def eval_vi(self, *a, **k):
        raise AssertionError('xu_opt = "simultaneous" evaluates through eval_vi_knots only')


def _problems():
    """Three problems with n <= 60, m <= 6, d = 2 and the knots inside the data box."""
    out = []
    for i, (n, m) in enumerate([(40, 4), (60, 6), (50, 5)]):
        g = np.random.Generator(np.random.PCG64(1900 + i))
        X = g.uniform(0.0, 10.0, size=(n, 2))
        y = np.sin(X).sum(axis=1) / np.sqrt(2.0) + g.normal(0.0, 0.5, size=n)
        lo, hi = X.min(axis=0), X.max(axis=0)
        U = lo + (hi - lo) * g.uniform(0.05, 0.95, size=(m, 2))
        out.append(((X, y, np.full(n, y.mean())), U,
                    OrderedDict([("sigma", 1.2 + 0.1 * i), ("l", 1.7), ("tau", 0.5)])))
    return out


def _run(opt, knot_opt):
    import sparsergps_amd as S
    ps = _problems()
    fake = FakeKnotBatch([p[0] for p in ps])
    res = S.norm_grad_ascent_vi_batch([p[2] for p in ps], "sqexp", [p[1] for p in ps], fake,
                                      opt=opt, xu_opt="simultaneous", knot_opt=knot_opt)
    iters = []
    for b, ((xy, y, mu), xu, cp) in enumerate(ps):
        ko = knot_opt[b] if knot_opt is not None and np.ndim(knot_opt[0]) > 0 else knot_opt
        ref = OD.norm_grad_ascent_vi(cp, "sqexp", xu, xy, y, mu, dcov_fun_dknot="sqexp",
                                     knot_opt=ko, opt=opt)
        r = res[b]
        assert r["iter"] == ref["iter"] and list(r["cov_par"]) == list(cp)
        m = xu.shape[0]
        assert r["knot_grad"].shape == (ref["iter"], m * 2)
        assert r["knot_history"].shape == (m, 2, ref["iter"])
        for key in ("obj_fun", "grad", "knot_grad", "knot_history", "cov_par_history", "xu"):
            np.testing.assert_allclose(r[key], np.asarray(ref[key]), rtol=1e-12, atol=0.0,
                                       err_msg=key)
        np.testing.assert_array_equal(r["xu"], r["knot_history"][:, :, -1])
        assert not np.array_equal(r["xu"], xu)                      # the knots did move
        if ko is not None:                                          # ... and only those asked for
            still = sorted(set(range(m)) - {k - 1 for k in ko})
            assert (r["knot_grad"].reshape(-1, m, 2)[:, still] == 0).all()
            # the others take no step: they sit where the transform's 1e-4 first puts them
            hist = r["knot_history"][still]
            assert (hist[:, :, 1:] == hist[:, :, 1:2]).all()
            np.testing.assert_allclose(hist[:, :, 1], xu[still], rtol=1e-4)
        np.testing.assert_allclose(r["u_mean"], ref["u_mean"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(r["u_var"], ref["u_var"], rtol=1e-9, atol=1e-12)
        assert "error" not in r
        iters.append(ref["iter"])
    # one evaluation per iteration for the whole batch, and a retired problem never runs again
    assert len(fake.calls) == max(iters)
    for b, k in enumerate(iters):
        assert [b in ran for ran in fake.calls] == [True] * k + [False] * (max(iters) - k)
    return iters


@pytest.mark.parametrize("opt,knot_opt", [
    ({"maxit": 6, "obj_tol": 0.0}, None),
    ({"maxit": 6, "obj_tol": 0.0}, [1, 3]),
    ({"maxit": 6, "obj_tol": 0.0}, [[1, 3], [2, 6], [5]]),
    ({"maxit": 6, "obj_tol": 0.0, "optim_method": "ga", "learn_rate": 1e-3}, [2, 4])])
def test_simultaneous_lockstep_equals_the_single_driver(opt, knot_opt):
    assert _run(opt, knot_opt) == [6, 6, 6]


def test_simultaneous_lockstep_stops_at_different_iterations():
    """obj_tol between the problems' objective steps: they retire at different iterations (the
    steps are printed, so a change of the recipe shows what to choose)."""
    ps = _problems()
    steps = []
    for (xy, y, mu), xu, cp in ps:
        ref = OD.norm_grad_ascent_vi(cp, "sqexp", xu, xy, y, mu, dcov_fun_dknot="sqexp",
                                     opt={"maxit": 6, "obj_tol": 0.0})
        steps.append(np.abs(np.diff(ref["obj_fun"])))
    print(np.array(steps))
    # the middle of the range of the steps of iteration 3: some problems are above, some below
    third = sorted(s[1] for s in steps)
    tol = 0.5 * (third[0] + third[-1])
    iters = _run({"maxit": 6, "obj_tol": float(tol)}, None)
    assert len(set(iters)) > 1, iters


def test_simultaneous_lockstep_retires_a_failing_problem():
    import sparsergps_amd as S
    ps = _problems()

    class Failing(FakeKnotBatch):
        def eval_vi_knots(self, *a, **k):
            obj, grads, kgs, st = super().eval_vi_knots(*a, **k)
            if len(self.calls) == 3:
                obj[1], st[1] = np.nan, -4
                kgs[1] = np.full_like(kgs[1], np.nan)
            return obj, grads, kgs, st

    fake = Failing([p[0] for p in ps])
    res = S.norm_grad_ascent_vi_batch([p[2] for p in ps], "sqexp", [p[1] for p in ps], fake,
                                      opt={"maxit": 5, "obj_tol": 0.0}, xu_opt="simultaneous")
    assert isinstance(res[1]["error"], S.NotPositiveDefinite) and res[1]["u_mean"] is None
    assert len(res[1]["obj_fun"]) == 2 and res[1]["knot_grad"].shape == (2, 12)
    assert all(1 not in ran for ran in fake.calls[3:])
    for b in (0, 2):
        assert res[b]["iter"] == 5 and "error" not in res[b] and res[b]["u_mean"] is not None
