"""The batched Laplace path's C ABI and host logic without a GPU: the symbols,
their prototypes and header text, every SGP_EINVAL of sgp_batch_lap_init / sgp_batch_eval_laplace
through the host-only checks (the very functions the entries run before their first device
call), the Python surface and its refusals, and the lockstep Laplace driver on a fake batch that
evaluates with the CPU oracle."""
import ctypes as C
import inspect
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

import bern_oracle as BO
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


def test_symbols_prototypes_and_header(lib):
    from sparsergps_amd import _lib
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    diag = open(os.path.join(ROOT, "include", "sgp_diag.h")).read()
    for name, nargs, src in (("sgp_batch_lap_init", 3, text), ("sgp_batch_lap_set_f", 3, text),
                             ("sgp_batch_lap_get_f", 2, text),
                             ("sgp_batch_eval_laplace", 17, text),
                             ("sgp_diag_batch_lap_args", 7, diag),
                             ("sgp_diag_batch_lap_eval_args", 4, diag),
                             ("sgp_diag_batch_lap_objective_values", 5, diag),
                             ("sgp_diag_batch_laplace_timing", 3, diag)):
        assert hasattr(lib, name), name
        assert _lib.PROTOTYPES[name][0] is C.c_int
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert _decl(src, name).count(",") == nargs - 1
    # up to status the argument list is sgp_batch_eval_vi's, type for type and name for name
    strip = lambda n: _decl(text, n)[len(f"int {n}("):]   # noqa: E731
    vi = strip("sgp_batch_eval_vi")
    assert strip("sgp_batch_eval_laplace") == vi[:-1] + ", double tol, int maxit, int* nr_iters)"
    assert _lib.PROTOTYPES["sgp_batch_eval_laplace"][1][:14] == \
        _lib.PROTOTYPES["sgp_batch_eval_vi"][1]
    doc = text[text.index("Laplace fits on a batch"):text.index("int sgp_batch_lap_init(")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)               # the comment's line breaks
    for cite in ("derivative_functions_of_data_likelihoods.R:7-61", "optimize_gp.R:480",
                 "optimize_gp.R:583", "newtrap_sparseGP.R:6-186", "newtrap_sparseGP.R:137-176",
                 "laplace_approx_gradient.R:25-336", "laplace_approx_prediction.R:3-123",
                 "quirk Q1", "quirk Q5", "unspecified until"):
        assert cite in doc, cite
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", text) and lib.sgp_abi_version() == 1
    assert f"#define SGP_BATCH_LAP_NOBJ {_lib.SGP_BATCH_LAP_NOBJ}" in diag


def test_null_handles_and_the_shared_check(lib):
    """Every entry refuses a NULL handle; sgp_batch_eval_laplace runs sgp_diag_batch_args' check
    (tests/test_batch_abi.py walks its cases) and then its own before the first device call,
    which the source shows."""
    from sparsergps_amd import _lib
    z = np.zeros(4)
    for rc in (lib.sgp_batch_lap_init(None, 0, None), lib.sgp_batch_lap_set_f(None, None, None),
               lib.sgp_batch_lap_get_f(None, _lib.dptr(z)),
               lib.sgp_diag_batch_lap_objective_values(None, 0, _lib.dptr(z), 4, None),
               lib.sgp_diag_batch_laplace_timing(None, 1, None)):
        assert rc == _lib.SGP_EINVAL
    q = lambda w: w.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    th, U, obj, grad = np.full((1, 3), 0.7), np.zeros(4), np.zeros(1), np.zeros((1, 3))
    uoff, m = np.zeros(1, dtype=np.int64), np.full(1, 2, dtype=np.int64)
    st, it = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = lib.sgp_batch_eval_laplace(None, 0, _lib.dptr(th), 3, _lib.dptr(U), q(uoff), q(m), 1e-6,
                                    0, None, _lib.dptr(obj), _lib.dptr(grad), 3,
                                    st.ctypes.data_as(_lib.c_int_p), 1e-6, 10,
                                    it.ctypes.data_as(_lib.c_int_p))
    assert rc == _lib.SGP_EINVAL and b"sgp_batch_eval_laplace" in lib.sgp_last_error()
    src = open(os.path.join(ROOT, "sparsergps_amd", "csrc", "capi.hip")).read()
    body = src[src.index("int sgp_batch_eval_laplace("):]
    body = body[:body.index("\n}\n")]
    assert body.index("batch_check_eval(") < body.index("batch_check_lap_eval(") < \
        body.index("batch_eval_laplace_impl(")
    assert "hip" not in body[:body.index("batch_eval_laplace_impl(")]
    init = src[src.index("int sgp_batch_lap_init("):]
    init = init[:init.index("\n}\n")]
    assert init.index("batch_check_lap(") < init.index("hipSetDevice")
    for name, check in (("sgp_diag_batch_lap_args", "batch_check_lap("),
                        ("sgp_diag_batch_lap_eval_args", "batch_check_lap_eval(")):
        d = src[src.index(f"int {name}("):]
        assert check in d[:d.index("\n}\n")]
    # the evaluation allocates nothing
    impl = src[src.index("int batch_eval_laplace_impl("):]
    impl = impl[:impl.index("\n}\n")]
    assert "Malloc" not in impl and "std::vector" not in impl


def _lap_args(lib, y, row0, nrow, family, expo):
    from sparsergps_amd import _lib
    q = lambda w: np.asarray(w, dtype=np.int64).ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    y = np.ascontiguousarray(y, dtype=np.float64)
    r0, nr = np.asarray(row0, dtype=np.int64), np.asarray(nrow, dtype=np.int64)
    ex = None if expo is None else np.ascontiguousarray(expo, dtype=np.float64)
    return lib.sgp_diag_batch_lap_args(_lib.dptr(y), y.size, q(r0), q(nr), r0.size, family,
                                       None if ex is None else _lib.dptr(ex))


@pytest.mark.parametrize("change,needle", [
    ({"family": 2}, b"family=2"),                               # SGP_FAM_GAUSSIAN
    ({"family": 7}, b"family=7"),
    ({"family": -1}, b"family=-1"),
    ({"expo": [1.0, 0.0, 1.0, 1.0, 1.0, 1.0]}, b"expo[1] = 0"),
    ({"expo": [1.0, 1.0, -2.0, 1.0, 1.0, 1.0]}, b"expo[2] = -2"),
    ({"expo": [1.0, 1.0, 1.0, float("inf"), 1.0, 1.0]}, b"expo[3] = inf"),
    ({"expo": [1.0, 1.0, 1.0, 1.0, float("nan"), 1.0]}, b"expo[4] = nan"),
    ({"family": 1, "expo": [1.0, 1.0, 1.0, 1.0, 1.0, -1.0]}, b"expo[5]"),   # validated for both
    ({"family": 1, "y": [0.0, 1.0, 1.0, 0.5, 2.0, 1.0]}, b"y[3] = 0.5 (problem 0)"),
    ({"family": 1, "y": [0.0, 1.0, 1.0, 0.0, 2.0, 1.0], "row0": [0, 4], "nrow": [2, 2]},
     b"y[4] = 2 (problem 1)"),
    ({"row0": [0, 5], "nrow": [4, 2]}, b"leave [0, 6)")])
def test_einval_cases_of_lap_init(lib, change, needle):
    from sparsergps_amd import _lib
    a = {"y": [0.0, 1.0, 1.0, 0.0, 1.0, 1.0], "row0": [0, 2], "nrow": [4, 4], "family": 0,
         "expo": None}
    a.update(change)
    rc = _lap_args(lib, a["y"], a["row0"], a["nrow"], a["family"], a["expo"])
    assert rc == _lib.SGP_EINVAL and needle in lib.sgp_last_error(), lib.sgp_last_error()


def test_lap_init_accepts_what_it_should(lib):
    from sparsergps_amd import _lib
    y = [0.0, 3.0, 1.0, 7.0, 2.0, 1.0]
    assert _lap_args(lib, y, [0, 2], [4, 4], 0, None) == _lib.SGP_OK          # counts, Poisson
    assert _lap_args(lib, y, [0, 2], [4, 4], 0, [0.5] * 6) == _lib.SGP_OK
    # Bernoulli looks only at the rows some problem covers
    assert _lap_args(lib, [0.0, 1.0, 9.0, 1.0], [0, 3], [2, 1], 1, None) == _lib.SGP_OK


@pytest.mark.parametrize("family,tol,maxit,with_it,needle", [
    (-1, 1e-6, 10, True, b"sgp_batch_lap_init first"),
    (0, -1e-6, 10, True, b"tol="), (0, float("nan"), 10, True, b"tol="),
    (0, float("inf"), 10, True, b"tol="), (1, 1e-6, -1, True, b"maxit=-1"),
    (1, 1e-6, 10, False, b"nr_iters")])
def test_einval_cases_of_eval_laplace(lib, family, tol, maxit, with_it, needle):
    from sparsergps_amd import _lib
    it = np.zeros(2, dtype=np.int32)
    rc = lib.sgp_diag_batch_lap_eval_args(family, tol, maxit,
                                          it.ctypes.data_as(_lib.c_int_p) if with_it else None)
    assert rc == _lib.SGP_EINVAL and needle in lib.sgp_last_error(), lib.sgp_last_error()
    assert lib.sgp_diag_batch_lap_eval_args(0, 0.0, 0, it.ctypes.data_as(_lib.c_int_p)) == \
        _lib.SGP_OK


def test_python_surface_and_refusals():
    import sparsergps_amd as S
    from sparsergps_amd.optimize import ERR_VI
    assert callable(S.laplace_grad_ascent_batch) and "laplace_grad_ascent_batch" in S.__all__
    for meth in ("lap_init", "set_f", "get_f", "eval_laplace", "eval_laplace_raw",
                 "laplace_stage_ms", "lap_objective_values"):
        assert callable(getattr(S.SparseGPBatch, meth))
    sig = inspect.signature(S.SparseGPBatch.eval_laplace).parameters
    assert list(sig) == ["self", "cov_pars", "cov_fun", "xus", "delta", "active", "obj_only",
                         "tol", "maxit"]
    assert (sig["delta"].default, sig["tol"].default, sig["maxit"].default) == (1e-6, 1e-6, 1000)
    assert list(inspect.signature(S.SparseGPBatch.lap_init).parameters) == ["self", "family", "expo"]
    assert inspect.signature(S.SparseGPBatch.score).parameters["par"].default is None
    # norm_grad_ascent_batch's signature, then family, expo and ff
    a = list(inspect.signature(S.norm_grad_ascent_batch).parameters)
    assert list(inspect.signature(S.laplace_grad_ascent_batch).parameters) == \
        a + ["family", "expo", "ff"]
    for fn in (S.optimize_gp_batch, S.cross_validate_gp):
        p = inspect.signature(fn).parameters
        assert p["family"].default == "gaussian" and p["expo"].default is None
        assert p["vi"].default is True
    X, y = np.zeros((8, 1)), np.zeros(8)
    cp = OrderedDict([("sigma", 1.0), ("l", 1.0), ("tau", 0.5)])
    U = np.zeros((2, 1))
    for fam in ("poisson", "bernoulli"):
        for call in (lambda: S.optimize_gp_batch([(X, y, None)], "sqexp", cp, U, family=fam),
                     lambda: S.cross_validate_gp(y, X, "sqexp", cp, U, folds=2, family=fam)):
            with pytest.raises(ValueError) as e:      # vi defaults to True
                call()
            assert ERR_VI in str(e.value)
        for bad in ("simultaneous", "oat", "random"):
            with pytest.raises(ValueError, match="Laplace batches have no knot gradient"):
                S.optimize_gp_batch([(X, y, None)], "sqexp", cp, U, xu_opt=bad, vi=False,
                                    family=fam)
            with pytest.raises(ValueError, match="Laplace batches have no knot gradient"):
                S.laplace_grad_ascent_batch([cp], "sqexp", [U], [(X, y, y)], xu_opt=bad,
                                            family=fam)
    with pytest.raises(ValueError, match="family must be"):
        S.optimize_gp_batch([(X, y, None)], "sqexp", cp, U, vi=False, family="binomial")
    with pytest.raises(ValueError, match="family must be"):
        S.laplace_grad_ascent_batch([cp], "sqexp", [U], [(X, y, y)], family="gaussian")
    with pytest.raises(ValueError, match="knot gradients"):
        S.laplace_grad_ascent_batch([cp], "sqexp", [U], [(X, y, y)], dcov_fun_dknot="sqexp")


# ------------------------------------------------------------------ the lockstep driver's host logic
class FakeBatch:
    """The interface laplace_grad_ascent_batch uses, evaluated by the CPU oracle; problem `fail`
    reports a K22 that is not positive definite at its `fail_at`-th evaluation."""

    def __init__(self, problems, family, expos, fail=None, fail_at=2):
        self.problems, self.B, self.family = problems, len(problems), family
        self.expos = expos
        self.nrow = np.array([p[1].size for p in problems])
        self.f = [np.zeros(p[1].size) for p in problems]
        self.calls, self.count = [], [0] * self.B
        self.last = [None] * self.B
        self.fail, self.fail_at = fail, fail_at

    def rows(self, b):
        return self.problems[b]

    def lap_init(self, family, expo=None):
        raise AssertionError("the driver re-initialised a batch that has its family")

    def set_f(self, f=None, fill=None):
        self.f = [np.array(v, dtype=np.float64) for v in f]

    def get_f(self):
        return [v.copy() for v in self.f]

    def eval_vi(self, *a, **k):
        raise AssertionError("the Laplace driver evaluated the VI objective")

    eval_fitc = eval_vi

    def eval_laplace(self, cov_pars, cov_fun, xus, delta=1e-6, active=None, obj_only=False,
                     tol=1e-6, maxit=1000):
        obj, grads = np.full(self.B, np.nan), [None] * self.B
        st, it = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        ran = []
        for b, (xy, y, mu) in enumerate(self.problems):
            if active is not None and not active[b]:
                continue
            ran.append(b)
            self.count[b] += 1
            if b == self.fail and self.count[b] == self.fail_at:
                st[b] = 3
                grads[b] = OrderedDict((k, np.nan) for k in cov_pars[b])
                continue
            muu = np.zeros(np.shape(xus[b])[0])
            if self.family == "bernoulli":
                nr = BO.newtrap_sparseGP(self.f[b], cov_pars[b], cov_fun, xy, xus[b], y, mu, delta,
                                         maxit, tol, muu=muu)
                g = BO.dlogq_dcov_par(cov_pars[b], cov_fun, xus[b], xy, y, nr["gp"], mu,
                                      delta)["gradient"]
            else:
                nr = O.newtrap_sparseGP(self.f[b], cov_pars[b], cov_fun, xy, xus[b], y, mu,
                                        self.expos[b], delta, maxit, tol, muu=muu)
                g = O.dlogq_dcov_par(cov_pars[b], cov_fun, xus[b], xy, y, nr["gp"], mu,
                                     self.expos[b], delta)["gradient"]
            self.f[b] = nr["gp"]
            obj[b] = nr["objective_function_values"][-1]
            it[b] = len(nr["objective_function_values"])
            grads[b] = g
            self.last[b] = (nr["u_posterior_mean"], nr["u_posterior_variance"])
        self.calls.append(ran)
        return obj, grads, st, it

    def posterior_u(self, muus):
        return ([None if r is None else r[0] for r in self.last],
                [None if r is None else r[1] for r in self.last])


def _problems(family):
    out = []
    for i, (n, m) in enumerate([(40, 4), (60, 6), (50, 5)]):
        g = np.random.Generator(np.random.PCG64(930 + i))
        X = g.uniform(0.0, 10.0, size=(n, 2))
        lat = 0.8 * np.sin(X).sum(axis=1) / np.sqrt(2.0)
        if family == "poisson":
            expo = g.uniform(0.5, 2.0, size=n)
            y = g.poisson(expo * np.exp(0.7 + lat)).astype(np.float64)
            f0, mu = np.full(n, np.log(y.mean())) - np.log(expo), np.full(n, 0.5)
        else:
            expo = np.ones(n)
            y = (g.uniform(size=n) < 1.0 / (1.0 + np.exp(-2.0 * lat))).astype(np.float64)
            f0, mu = np.zeros(n), np.zeros(n)
        out.append(dict(data=(X, y, mu), expo=expo, f0=f0, U=g.uniform(0.0, 10.0, size=(m, 2)),
                        cp=OrderedDict([("sigma", 1.2 + 0.1 * i), ("l", 1.7), ("tau", 0.5)])))
    return out


def _single(family, P, opt):
    (X, y, mu), muu = P["data"], np.zeros(P["U"].shape[0])
    if family == "bernoulli":
        return BO.laplace_grad_ascent(P["cp"], "sqexp", P["U"], X, y, P["f0"], mu, muu, opt=opt)
    return OD.laplace_grad_ascent(P["cp"], "sqexp", P["U"], X, y, P["f0"], mu, muu, P["expo"],
                                  opt=opt)


@pytest.mark.parametrize("family", ["poisson", "bernoulli"])
@pytest.mark.parametrize("opt", [{"maxit": 4, "obj_tol": 0.0}, {"maxit": 9, "obj_tol": "spread"}])
def test_lockstep_driver_equals_the_single_driver(family, opt):
    import sparsergps_amd as S
    ps = _problems(family)
    opt = dict(opt, tol_nr=1e-5, maxit_nr=200)
    if opt["obj_tol"] == "spread":
        # a tolerance between the problems' |obj steps| at iteration 5, so they stop apart
        free = [_single(family, P, dict(opt, obj_tol=0.0)) for P in ps]
        steps = sorted(abs(r["obj_fun"][4] - r["obj_fun"][3]) for r in free)
        opt["obj_tol"] = float(0.5 * (steps[0] + steps[1]))
    fake = FakeBatch([P["data"] for P in ps], family, [P["expo"] for P in ps])
    res = S.laplace_grad_ascent_batch([P["cp"] for P in ps], "sqexp", [P["U"] for P in ps], fake,
                                      [np.zeros(P["U"].shape[0]) for P in ps], opt,
                                      family=family, ff=[P["f0"] for P in ps])
    iters = []
    for b, P in enumerate(ps):
        ref, r = _single(family, P, opt), res[b]
        assert r["iter"] == ref["iter"] and list(r["cov_par"]) == list(P["cp"])
        assert list(r["nr_iter"]) == list(ref["nr_iter"])
        for key in ("obj_fun", "grad", "cov_par_history", "fmax", "u_mean", "u_var"):
            np.testing.assert_allclose(r[key], np.asarray(ref[key]), rtol=1e-12, atol=0.0,
                                       err_msg=key)
        assert "error" not in r
        iters.append(ref["iter"])
    assert len(fake.calls) == max(iters)
    for b, k in enumerate(iters):
        assert [b in ran for ran in fake.calls] == [True] * k + [False] * (max(iters) - k)
    if opt["obj_tol"] > 0:
        assert len(set(iters)) > 1, iters


@pytest.mark.parametrize("family", ["poisson", "bernoulli"])
def test_a_failing_problem_retires_alone(family):
    import sparsergps_amd as S
    ps = _problems(family)
    opt = {"maxit": 4, "obj_tol": 0.0, "tol_nr": 1e-5, "maxit_nr": 200}
    fake = FakeBatch([P["data"] for P in ps], family, [P["expo"] for P in ps], fail=1, fail_at=2)
    res = S.laplace_grad_ascent_batch([P["cp"] for P in ps], "sqexp", [P["U"] for P in ps], fake,
                                      None, opt, family=family, ff=[P["f0"] for P in ps])
    assert "leading minor of order 3" in str(res[1]["error"])
    assert res[1]["u_mean"] is None and res[1]["fmax"] is None and len(res[1]["obj_fun"]) == 1
    assert [1 in ran for ran in fake.calls] == [True, True, False, False]
    for b in (0, 2):
        ref = _single(family, ps[b], opt)
        assert "error" not in res[b] and res[b]["iter"] == ref["iter"] == 4
        for key in ("obj_fun", "grad", "fmax"):
            np.testing.assert_allclose(res[b][key], np.asarray(ref[key]), rtol=1e-12, atol=0.0)


def test_result_dict_has_the_single_drivers_keys():
    import sparsergps_amd as S
    P = _problems("bernoulli")[0]
    fake = FakeBatch([P["data"]], "bernoulli", [P["expo"]])
    r = S.laplace_grad_ascent_batch([P["cp"]], "sqexp", [P["U"]], fake, opt={"maxit": 2},
                                    family="bernoulli", ff=[P["f0"]])[0]
    assert set(r) == {"cov_par", "xu", "iter", "obj_fun", "grad", "cov_par_history", "knot_grad",
                      "knot_history", "cov_fun", "xy", "mu", "muu", "u_mean", "u_var", "fmax",
                      "nr_iter"}
    src = inspect.getsource(S.drivers._ascent) + inspect.getsource(S.drivers.laplace_grad_ascent)
    for key in r:
        assert f'"{key}"' in src, key
