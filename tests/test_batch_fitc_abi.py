"""The batched FITC path's C ABI and host logic without a GPU: the symbol, its
prototype and header text, its SGP_EINVAL cases (sgp_diag_batch_args is the very check
sgp_batch_eval_fitc runs before its first device call), the Python surface, and the lockstep FITC
driver on a fake batch that evaluates with the CPU oracle."""
import ctypes as C
import inspect
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

from oracle import drivers as OD
from oracle import sgp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    return _lib.lib()


def _decl(text, name):
    decl = re.sub(r"\s+", " ", text[text.index(f"int {name}("):])
    return decl[:decl.index(";")]


def test_symbol_prototype_and_header(lib):
    from sparsergps_amd import _lib
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    diag = open(os.path.join(ROOT, "include", "sgp_diag.h")).read()
    for name, nargs, src in (("sgp_batch_eval_fitc", 14, text),
                             ("sgp_diag_batch_fitc_timing", 3, diag)):
        assert hasattr(lib, name), name
        assert _lib.PROTOTYPES[name][0] is C.c_int
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert _decl(src, name).count(",") == nargs - 1
    # the argument list is sgp_batch_eval_vi's, type for type and name for name
    strip = lambda n: _decl(text, n)[len(f"int {n}("):]   # noqa: E731
    assert strip("sgp_batch_eval_fitc") == strip("sgp_batch_eval_vi")
    assert _lib.PROTOTYPES["sgp_batch_eval_fitc"][1] == _lib.PROTOTYPES["sgp_batch_eval_vi"][1]
    doc = text[text.index("The batch's other Gaussian objective"):text.index("int sgp_batch_eval_fitc(")]
    for cite in ("laplace_approx_obj_funs.R:6-52", "laplace_gradient_ascent.R:1238-1263",
                 "laplace_approx_gradient.R:720-971", "laplace_approx_prediction.R:3-123",
                 "not positive and finite", "no delta"):
        assert cite in doc, cite
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", text) and lib.sgp_abi_version() == 1


def test_null_handle_and_the_shared_check(lib):
    """sgp_batch_eval_fitc refuses a NULL handle, and what it refuses beyond that is
    sgp_diag_batch_args' list (tests/test_batch_abi.py walks every case of it): the entry calls
    the same function before its first device call, which the source shows."""
    from sparsergps_amd import _lib
    q = lambda w: w.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    th, U, obj, grad = np.full((1, 3), 0.7), np.zeros(4), np.zeros(1), np.zeros((1, 3))
    uoff, m, st = np.zeros(1, dtype=np.int64), np.full(1, 2, dtype=np.int64), np.zeros(1, np.int32)
    rc = lib.sgp_batch_eval_fitc(None, 0, _lib.dptr(th), 3, _lib.dptr(U), q(uoff), q(m), 1e-6, 0,
                                 None, _lib.dptr(obj), _lib.dptr(grad), 3,
                                 st.ctypes.data_as(_lib.c_int_p))
    assert rc == _lib.SGP_EINVAL and b"sgp_batch_eval_fitc" in lib.sgp_last_error()
    assert lib.sgp_diag_batch_fitc_timing(None, 1, None) == _lib.SGP_EINVAL
    src = open(os.path.join(ROOT, "sparsergps_amd", "csrc", "capi.hip")).read()
    body = src[src.index("int sgp_batch_eval_fitc("):]
    body = body[:body.index("\n}\n")]
    diag = src[src.index("int sgp_diag_batch_args("):]
    diag = diag[:diag.index("\n}\n")]
    assert "batch_check_eval(" in diag and "batch_check_eval(" in body
    assert body.index("batch_check_eval(") < body.index("batch_eval_impl(")
    assert "hip" not in body[:body.index("batch_eval_impl(")]        # no device call before it


@pytest.mark.parametrize("change,needle", [
    ({"m": np.array([3, 65, 64], dtype=np.int64)}, b"m=65 outside [1, 64]"),
    ({"kernel": 2}, b"'sqexp' and 'ard'"),
    ({"delta": float("nan")}, b"delta"),
    ({"ldg": 2}, b"ldg"),
    ({"d": 33}, b"dimension")])
def test_einval_cases_of_the_shared_check(lib, change, needle):
    from sparsergps_amd import _lib
    g = np.random.default_rng(0)
    d, B, n = 2, 3, 50
    m = np.array([3, 1, 64], dtype=np.int64)
    packs = [g.uniform(size=int(k) * d) for k in m]
    a = {"X": np.asfortranarray(g.uniform(size=(n, d))), "d": d, "kernel": 0, "m": m,
         "delta": 1e-6, "ldg": 3}
    a.update(change)
    uoff = np.concatenate([[0], np.cumsum([p.size for p in packs])[:-1]]).astype(np.int64)
    q = lambda v: v.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    y, mu = g.normal(size=n), np.zeros(n)
    row0, nrow = np.array([0, 10, 0], dtype=np.int64), np.array([50, 40, 1], dtype=np.int64)
    theta, U = np.full((B, 3), 0.7), np.concatenate(packs)
    obj, grad, st = np.zeros(B), np.zeros((B, 3)), np.zeros(B, dtype=np.int32)
    rc = lib.sgp_diag_batch_args(1, _lib.dptr(a["X"]), n, n, a["d"], _lib.dptr(y), _lib.dptr(mu),
                                 q(row0), q(nrow), B, a["kernel"], _lib.dptr(theta), 3,
                                 _lib.dptr(U), q(uoff), q(a["m"]), a["delta"], 0, None,
                                 _lib.dptr(obj), _lib.dptr(grad), a["ldg"],
                                 st.ctypes.data_as(_lib.c_int_p))
    assert rc == _lib.SGP_EINVAL and needle in lib.sgp_last_error(), lib.sgp_last_error()


def test_python_surface_exists():
    import sparsergps_amd as S
    assert callable(S.norm_grad_ascent_batch) and "norm_grad_ascent_batch" in S.__all__
    for meth in ("eval_fitc", "eval_fitc_raw", "fitc_stage_ms"):
        assert callable(getattr(S.SparseGPBatch, meth))
    assert inspect.signature(S.SparseGPBatch.eval_fitc) == inspect.signature(S.SparseGPBatch.eval_vi)
    assert inspect.signature(S.norm_grad_ascent_batch) == \
        inspect.signature(S.norm_grad_ascent_vi_batch)
    for fn in (S.optimize_gp_batch, S.cross_validate_gp):
        assert inspect.signature(fn).parameters["vi"].default is True
        assert "FALSE" in fn.__doc__                      # the reference's own default is named
    with pytest.raises(ValueError, match="knot gradients"):
        S.norm_grad_ascent_batch([], "sqexp", [], [], dcov_fun_dknot="sqexp")


def test_simultaneous_is_refused_for_fitc():
    import sparsergps_amd as S
    X, y = np.zeros((8, 1)), np.zeros(8)
    cp = OrderedDict([("sigma", 1.0), ("l", 1.0), ("tau", 0.5)])
    for call in (lambda: S.optimize_gp_batch([(X, y, None)], "sqexp", cp, np.zeros((2, 1)),
                                             xu_opt="simultaneous", vi=False),
                 lambda: S.cross_validate_gp(y, X, "sqexp", cp, np.zeros((2, 1)), folds=2,
                                             xu_opt="simultaneous", vi=False),
                 lambda: S.norm_grad_ascent_batch([cp], "sqexp", [np.zeros((2, 1))], [(X, y, y)],
                                                  xu_opt="simultaneous")):
        with pytest.raises(ValueError, match="FITC batches have no knot gradient yet"):
            call()
    for bad in ("oat", "random"):                         # refused as today
        with pytest.raises(ValueError, match="batches do not support"):
            S.optimize_gp_batch([(X, y, None)], "sqexp", cp, np.zeros((2, 1)), xu_opt=bad,
                                vi=False)


# ------------------------------------------------------------------ the lockstep driver's host logic
class FakeBatch:
    """The interface norm_grad_ascent_batch uses, evaluated by the CPU oracle."""

    def __init__(self, problems):
        self.problems, self.B = problems, len(problems)
        self.calls = []
        self.last = [None] * self.B

    def rows(self, b):
        return self.problems[b]

    def eval_vi(self, *a, **k):
        raise AssertionError("the FITC driver evaluated the VI objective")

    def eval_fitc(self, cov_pars, cov_fun, xus, delta=1e-6, active=None, obj_only=False,
                  r_det=False):
        obj, grads = np.full(self.B, np.nan), [None] * self.B
        ran = []
        for b, (xy, y, mu) in enumerate(self.problems):
            if active is not None and not active[b]:
                continue
            ran.append(b)
            obj[b] = O.fitc_obj_eval(cov_pars[b], cov_fun, xus[b], xy, y, mu, delta)
            grads[b] = O.dlogp_dcov_par(cov_pars[b], cov_fun, xus[b], xy, y, mu, delta)["gradient"]
            self.last[b] = (OrderedDict(cov_pars[b]), np.array(xus[b]), delta)
        self.calls.append(ran)
        return obj, grads, np.zeros(self.B, dtype=np.int32)

    def posterior_u(self, muus):
        res = [O.fitc_posterior_u(cp, "sqexp", xu, *self.problems[b], muus[b], dl)
               for b, (cp, xu, dl) in enumerate(self.last)]
        return [r[0] for r in res], [r[1] for r in res]


def _problems():
    out = []
    for i, (n, m) in enumerate([(40, 4), (60, 6), (50, 5)]):
        g = np.random.Generator(np.random.PCG64(900 + i))
        X = g.uniform(0.0, 10.0, size=(n, 2))
        y = np.sin(X).sum(axis=1) / np.sqrt(2.0) + g.normal(0.0, 0.5, size=n)
        out.append(((X, y, np.full(n, y.mean())), g.uniform(0.0, 10.0, size=(m, 2)),
                    OrderedDict([("sigma", 1.2 + 0.1 * i), ("l", 1.7), ("tau", 0.5)])))
    return out


@pytest.mark.parametrize("opt", [{"maxit": 6, "obj_tol": 0.0},
                                 {"maxit": 14, "obj_tol": "spread"},
                                 {"maxit": 6, "obj_tol": 0.0, "optim_method": "ga",
                                  "learn_rate": 1e-3}])
def test_lockstep_driver_equals_the_single_driver(opt):
    import sparsergps_amd as S
    ps = _problems()
    opt = dict(opt)
    if opt["obj_tol"] == "spread":
        # a tolerance between the problems' |obj steps| at iteration 8, so they stop apart
        free = [OD.norm_grad_ascent(cp, "sqexp", xu, xy, y, mu, opt={"maxit": 14, "obj_tol": 0.0})
                for (xy, y, mu), xu, cp in ps]
        steps = sorted(abs(r["obj_fun"][7] - r["obj_fun"][6]) for r in free)
        opt["obj_tol"] = float(0.5 * (steps[0] + steps[1]))
    fake = FakeBatch([p[0] for p in ps])
    res = S.norm_grad_ascent_batch([p[2] for p in ps], "sqexp", [p[1] for p in ps], fake, opt=opt)
    iters = []
    for b, ((xy, y, mu), xu, cp) in enumerate(ps):
        ref = OD.norm_grad_ascent(cp, "sqexp", xu, xy, y, mu, opt=opt)
        r = res[b]
        assert r["iter"] == ref["iter"] and list(r["cov_par"]) == list(cp)
        for key in ("obj_fun", "grad", "cov_par_history"):
            np.testing.assert_allclose(r[key], np.asarray(ref[key]), rtol=1e-12, atol=0.0,
                                       err_msg=key)
        np.testing.assert_allclose(r["u_mean"], ref["u_mean"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(r["u_var"], ref["u_var"], rtol=1e-9, atol=1e-12)
        assert "error" not in r
        iters.append(ref["iter"])
    assert len(fake.calls) == max(iters)
    for b, k in enumerate(iters):
        assert [b in ran for ran in fake.calls] == [True] * k + [False] * (max(iters) - k)
    if opt["obj_tol"] > 0:
        assert len(set(iters)) > 1, iters


def test_result_dict_has_the_single_drivers_keys():
    import sparsergps_amd as S
    ps = _problems()[:1]
    fake = FakeBatch([p[0] for p in ps])
    r = S.norm_grad_ascent_batch([p[2] for p in ps], "sqexp", [p[1] for p in ps], fake,
                                 opt={"maxit": 2})[0]
    assert set(r) == {"cov_par", "xu", "iter", "obj_fun", "grad", "cov_par_history", "knot_grad",
                      "knot_history", "cov_fun", "xy", "mu", "muu", "u_mean", "u_var"}
    src = inspect.getsource(S.drivers._ascent) + inspect.getsource(S.drivers._gaussian_driver)
    for key in r:
        assert f'"{key}"' in src, key
