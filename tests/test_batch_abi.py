"""The batched VI path's C ABI and host logic without a GPU: symbols, prototypes, header text, every
SGP_EINVAL case (sgp_diag_batch_args is the very check sgp_batch_create / sgp_batch_eval_vi run
before their first device call), the segment plan, NULL handles, the loud failure without a
device, and the lockstep driver on a fake batch that evaluates with the CPU oracle."""
import ctypes as C
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

from oracle import drivers as OD
from oracle import sgp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sgp_batch_create", "sgp_batch_destroy", "sgp_batch_set_data", "sgp_batch_eval_vi",
           "sgp_batch_posterior_u", "sgp_diag_batch_args", "sgp_diag_batch_plan",
           "sgp_diag_batch_timing")


@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    return _lib.lib()


def _decl_commas(text, name):
    decl = re.sub(r"\s+", " ", text[text.index(f"int {name}("):])
    return decl[:decl.index(";")].count(",")


def test_symbols_prototypes_and_header(lib):
    from sparsergps_amd import _lib
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
        assert _lib.PROTOTYPES[name][0] is C.c_int
    nargs = {name: len(_lib.PROTOTYPES[name][1]) for name in SYMBOLS}
    assert nargs == {"sgp_batch_create": 11, "sgp_batch_destroy": 1, "sgp_batch_set_data": 3,
                     "sgp_batch_eval_vi": 14, "sgp_batch_posterior_u": 4,
                     "sgp_diag_batch_args": 23, "sgp_diag_batch_plan": 9,
                     "sgp_diag_batch_timing": 3}
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    diag = open(os.path.join(ROOT, "include", "sgp_diag.h")).read()
    assert "typedef struct sgp_batch sgp_batch;" in text
    for name in SYMBOLS:
        src = diag if name.startswith("sgp_diag_") else text
        assert _decl_commas(src, name) == nargs[name] - 1, name
    doc = text[text.index("A batch of small-knot VI problems"):text.index("typedef struct sgp_batch")]
    for cite in ("vi_functions.R:64-121", "vi_functions.R:14-27", "vi_functions.R:126-419",
                 "vi_functions.R:1161-1180"):
        assert cite in doc, cite
    assert re.search(r"#define\s+SGP_BATCH_MMAX\s+64\b", text) and _lib.SGP_BATCH_MMAX == 64
    assert re.search(r"#define\s+SGP_BATCH_SEG_ROWS\s+\d+\b", diag)
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", text) and lib.sgp_abi_version() == 1


def _good(B=3, d=2, kernel=0, n=50):
    g = np.random.default_rng(0)
    P = (d if kernel == 1 else 1) + 2
    m = np.array([3, 1, 64][:B] + [5] * max(0, B - 3), dtype=np.int64)
    packs = [np.asfortranarray(g.uniform(size=(int(k), d))).reshape(-1, order="F") for k in m]
    uoff = np.concatenate([[0], np.cumsum([p.size for p in packs])[:-1]]).astype(np.int64)
    return {"stage": 1, "X": np.asfortranarray(g.uniform(size=(n, d))), "nrows": n, "ldx": n,
            "d": d, "y": g.normal(size=n), "mu": np.zeros(n),
            "row0": np.array([0, 10, 0][:B] + [0] * max(0, B - 3), dtype=np.int64),
            "nrow": np.array([50, 40, 1][:B] + [50] * max(0, B - 3), dtype=np.int64), "B": B,
            "kernel": kernel, "theta": np.full((B, P), 0.7), "ldt": P,
            "U": np.concatenate(packs), "uoff": uoff, "m": m, "delta": 1e-6, "flags": 0,
            "active": None, "obj": np.zeros(B), "grad": np.zeros((B, P)), "ldg": P,
            "status": np.zeros(B, dtype=np.int32)}


def _check(lib, a):
    from sparsergps_amd import _lib
    p = lambda v: None if v is None else _lib.dptr(v)   # noqa: E731
    q = lambda v: None if v is None else v.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    act = None if a["active"] is None else a["active"].ctypes.data_as(_lib.c_ubyte_p)
    st = None if a["status"] is None else a["status"].ctypes.data_as(_lib.c_int_p)
    return lib.sgp_diag_batch_args(a["stage"], p(a["X"]), a["nrows"], a["ldx"], a["d"], p(a["y"]),
                                   p(a["mu"]), q(a["row0"]), q(a["nrow"]), a["B"], a["kernel"],
                                   p(a["theta"]), a["ldt"], p(a["U"]), q(a["uoff"]), q(a["m"]),
                                   a["delta"], a["flags"], act, p(a["obj"]), p(a["grad"]), a["ldg"],
                                   st)


def test_good_arguments_pass(lib):
    from sparsergps_amd import _lib
    assert _check(lib, _good()) == _lib.SGP_OK
    assert _check(lib, _good(kernel=1, d=32)) == _lib.SGP_OK
    assert _check(lib, _good(B=1)) == _lib.SGP_OK
    assert _check(lib, {**_good(), "delta": -1e-3}) == _lib.SGP_OK   # the factorisation's to judge
    # SGP_FLAG_OBJ_ONLY reads no grad and no ldg
    assert _check(lib, {**_good(), "flags": 2, "grad": None, "ldg": 0}) == _lib.SGP_OK
    # stage 0 is create's check: nothing of the evaluation's arguments is read
    a = {**_good(), "stage": 0, "theta": None, "U": None, "m": None, "kernel": 2}
    assert _check(lib, a) == _lib.SGP_OK
    # an inactive problem's m and theta are not read
    a = _good()
    a["m"][1] = 0
    a["theta"][1] = np.nan
    a["active"] = np.array([1, 0, 1], dtype=np.uint8)
    assert _check(lib, a) == _lib.SGP_OK


def _with(key, idx, val):
    a = _good()
    a[key] = a[key].copy()
    a[key][idx] = val
    return {key: a[key]}


BAD = {
    "X NULL": ({"X": None}, b"NULL"),
    "y NULL": ({"y": None}, b"NULL"),
    "mu NULL": ({"mu": None}, b"NULL"),
    "row0 NULL": ({"row0": None}, b"NULL"),
    "nrow NULL": ({"nrow": None}, b"NULL"),
    "theta NULL": ({"theta": None}, b"NULL"),
    "U NULL": ({"U": None}, b"NULL"),
    "uoff NULL": ({"uoff": None}, b"NULL"),
    "m NULL": ({"m": None}, b"NULL"),
    "obj NULL": ({"obj": None}, b"NULL"),
    "grad NULL": ({"grad": None}, b"NULL"),
    "status NULL": ({"status": None}, b"NULL"),
    "B = 0": ({"B": 0}, b"B=0"),
    "B < 0": ({"B": -2}, b"B=-2"),
    "d = 0": ({"d": 0}, b"dimension"),
    "d = 33": ({"d": 33}, b"dimension"),
    "m = 0": (_with("m", 0, 0), b"m=0 outside [1, 64]"),
    "m = 65": (_with("m", 2, 65), b"m=65 outside [1, 64]"),
    "nrow = 0": (_with("nrow", 1, 0), b"nrow=0"),
    "nrow < 0": (_with("nrow", 1, -3), b"nrow=-3"),
    "range past the end": (_with("row0", 1, 11), b"leave [0, 50)"),
    "range before the start": (_with("row0", 2, -1), b"leave [0, 50)"),
    "ldx < nrows": ({"ldx": 49}, b"ldx"),
    "nrows = 0": ({"nrows": 0}, b"nrows"),
    "ldt < P": ({"ldt": 2}, b"ldt"),
    "ldg < P": ({"ldg": 2}, b"ldg"),
    "exp refused": ({"kernel": 2}, b"'sqexp' and 'ard'"),
    "unknown kernel": ({"kernel": 7}, b"covariance function"),
    "sigma = 0": (_with("theta", (0, 0), 0.0), b"theta[0]"),
    "l < 0": (_with("theta", (1, 1), -0.8), b"problem 1's theta[1]"),
    "tau = 0": (_with("theta", (2, 2), 0.0), b"problem 2's theta[2]"),
    "sigma NaN": (_with("theta", (0, 0), np.nan), b"theta[0]"),
    "l inf": (_with("theta", (0, 1), np.inf), b"theta[1]"),
    "delta NaN": ({"delta": float("nan")}, b"delta"),
    "knot NaN": (_with("U", 4, np.nan), b"U[1, 1]"),
    "stage": ({"stage": 2}, b"stage"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_einval_before_any_device_call(lib, name):
    from sparsergps_amd import _lib
    change, needle = BAD[name]
    assert _check(lib, {**_good(), **change}) == _lib.SGP_EINVAL
    assert needle in lib.sgp_last_error(), lib.sgp_last_error()


def test_ard_length_scales_are_each_checked(lib):
    from sparsergps_amd import _lib
    a = _good(kernel=1, d=3)
    a["theta"][1, 3] = -0.2
    assert _check(lib, a) == _lib.SGP_EINVAL and b"problem 1's theta[3]" in lib.sgp_last_error()
    assert _check(lib, {**_good(kernel=1, d=3), "ldt": 4}) == _lib.SGP_EINVAL


def test_create_runs_the_same_check_first(lib):
    """sgp_batch_create returns these before its first device call: the same status and message
    on a machine without a GPU, and no handle."""
    from sparsergps_amd import _lib
    q = lambda v: None if v is None else v.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    p = lambda v: None if v is None else _lib.dptr(v)   # noqa: E731
    for name in ("X NULL", "B = 0", "d = 33", "nrow = 0", "range past the end", "ldx < nrows"):
        change, needle = BAD[name]
        a = {**_good(), **change}
        h = C.c_void_p()
        st = lib.sgp_batch_create(C.byref(h), 0, p(a["X"]), a["nrows"], a["ldx"], a["d"], p(a["y"]),
                                  p(a["mu"]), q(a["row0"]), q(a["nrow"]), a["B"])
        assert st == _lib.SGP_EINVAL and needle in lib.sgp_last_error(), name
        assert h.value is None
    a = _good()
    assert lib.sgp_batch_create(None, 0, p(a["X"]), 50, 50, 2, p(a["y"]), p(a["mu"]), q(a["row0"]),
                                q(a["nrow"]), 3) == _lib.SGP_EINVAL


def _plan(lib, row0, nrow):
    from sparsergps_amd import _lib
    r0 = np.asarray(row0, dtype=np.int64)
    nr = np.asarray(nrow, dtype=np.int64)
    q = lambda v: v.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    nseg, mx = C.c_int64(0), C.c_int64(0)
    assert lib.sgp_diag_batch_plan(q(r0), q(nr), r0.size, 0, C.byref(nseg), None, None, None,
                                   C.byref(mx)) == _lib.SGP_OK
    sp, s0, sr = (np.full(nseg.value + 2, -7, dtype=np.int64) for _ in range(3))
    assert lib.sgp_diag_batch_plan(q(r0), q(nr), r0.size, nseg.value, C.byref(nseg), q(sp), q(s0),
                                   q(sr), None) == _lib.SGP_OK
    assert (sp[nseg.value:] == -7).all() and (sr[nseg.value:] == -7).all()    # cap is respected
    k = nseg.value
    return sp[:k], s0[:k], sr[:k], mx.value


def test_plan(lib):
    diag = open(os.path.join(ROOT, "include", "sgp_diag.h")).read()
    seg = int(re.search(r"#define\s+SGP_BATCH_SEG_ROWS\s+(\d+)", diag).group(1))
    assert seg % 64 == 0 and seg >= 64
    row0 = [0, 5, 0, 7000, 3, 0]
    nrow = [1, 64, seg, seg + 1, 5 * seg - 1, 100_000]
    sp, s0, sr, mx = _plan(lib, row0, nrow)
    assert mx == seg
    assert (np.diff(sp) >= 0).all() and set(sp) == set(range(len(row0)))   # problems in order
    for b, (r0, nr) in enumerate(zip(row0, nrow)):
        mine = sp == b
        assert mine.sum() == -(-nr // seg)
        # the segments cover [r0, r0 + nr) exactly once, in order, and none exceeds the limit
        assert s0[mine][0] == r0 and (s0[mine][1:] == s0[mine][:-1] + sr[mine][:-1]).all()
        assert sr[mine].sum() == nr and (sr[mine] >= 1).all() and (sr[mine] <= seg).all()
        assert (sr[mine][:-1] == seg).all()
        # ... and are the same whatever else the batch holds
        sp1, s01, sr1, _ = _plan(lib, [r0], [nr])
        assert (s01 == s0[mine]).all() and (sr1 == sr[mine]).all() and (sp1 == 0).all()
    rev = _plan(lib, row0[::-1], nrow[::-1])
    for b in range(len(row0)):
        mine, theirs = sp == b, rev[0] == len(row0) - 1 - b
        assert (rev[1][theirs] == s0[mine]).all() and (rev[2][theirs] == sr[mine]).all()


def test_plan_einval(lib):
    from sparsergps_amd import _lib
    one = np.array([0], dtype=np.int64)
    q = lambda v: v.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    n = C.c_int64(0)
    assert lib.sgp_diag_batch_plan(None, q(one), 1, 0, C.byref(n), None, None, None,
                                   None) == _lib.SGP_EINVAL
    assert b"sgp_diag_batch_plan" in lib.sgp_last_error()
    assert lib.sgp_diag_batch_plan(q(one), q(one), 1, 0, C.byref(n), None, None, None,
                                   None) == _lib.SGP_EINVAL           # nrow = 0
    assert lib.sgp_diag_batch_plan(q(one), q(one + 1), 0, 0, C.byref(n), None, None, None,
                                   None) == _lib.SGP_EINVAL           # B = 0
    assert lib.sgp_diag_batch_plan(q(one), q(one + 1), 1, 0, None, None, None, None,
                                   None) == _lib.SGP_EINVAL
    assert lib.sgp_diag_batch_plan(q(one), q(one + 1), 1, 4, C.byref(n), None, None, None,
                                   None) == _lib.SGP_EINVAL           # cap without arrays


def test_null_handles(lib):
    from sparsergps_amd import _lib
    a = _good()
    v = np.zeros(4)
    q = lambda w: w.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    st = lib.sgp_batch_eval_vi(None, 0, _lib.dptr(a["theta"]), 3, _lib.dptr(a["U"]), q(a["uoff"]),
                               q(a["m"]), 1e-6, 0, None, _lib.dptr(a["obj"]), _lib.dptr(a["grad"]),
                               3, a["status"].ctypes.data_as(_lib.c_int_p))
    assert st == _lib.SGP_EINVAL and b"sgp_batch" in lib.sgp_last_error()
    assert lib.sgp_batch_set_data(None, _lib.dptr(v), _lib.dptr(v)) == _lib.SGP_EINVAL
    assert lib.sgp_batch_posterior_u(None, _lib.dptr(v), _lib.dptr(v),
                                     _lib.dptr(v)) == _lib.SGP_EINVAL
    assert lib.sgp_diag_batch_timing(None, 1, None) == _lib.SGP_EINVAL
    assert lib.sgp_batch_destroy(None) == _lib.SGP_EINVAL
    assert b"sgp_batch_destroy" in lib.sgp_last_error()


def test_no_gpu_no_fallback():
    """Without a HIP device SparseGPBatch(...) raises SGPError (argument errors come first, also
    as SGPError); there is no CPU path behind it."""
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    X, y = np.zeros((6, 2)), np.zeros(6)
    with pytest.raises(S.SGPError, match="leave"):
        S.SparseGPBatch(X, y, 0.0, [0, 4], [4, 3])
    n = C.c_int(0)
    if _lib.lib().sgp_device_count(C.byref(n)) == _lib.SGP_OK and n.value > 0:
        return                                            # the GPU suite covers the rest
    with pytest.raises(S.SGPError, match="no HIP device"):
        S.SparseGPBatch(X, y, 0.0)


def test_python_surface_exists():
    import sparsergps_amd as S
    for name in ("SparseGPBatch", "norm_grad_ascent_vi_batch", "optimize_gp_batch"):
        assert callable(getattr(S, name)) and name in S.__all__
    for meth in ("from_problems", "eval_vi", "posterior_u", "set_data", "close", "__enter__",
                 "__exit__"):
        assert callable(getattr(S.SparseGPBatch, meth))
    with pytest.raises(ValueError, match="knot gradients"):
        S.norm_grad_ascent_vi_batch([], "sqexp", [], [], dcov_fun_dknot="sqexp")
    assert S.optimize_gp_batch([(np.zeros((4, 1)), np.zeros(4), None)] * 2, "exp", {}, None) == \
        ["Error: invalid covariance function"] * 2


# ------------------------------------------------------------------ the lockstep driver's host logic
class FakeBatch:
    """The interface norm_grad_ascent_vi_batch uses, evaluated by the CPU oracle."""

    def __init__(self, problems):
        self.problems, self.B = problems, len(problems)
        self.calls = []            # per evaluation: the problems it ran
        self.last = [None] * self.B

    def rows(self, b):
        return self.problems[b]

    def eval_vi(self, cov_pars, cov_fun, xus, delta=1e-6, active=None, obj_only=False,
                r_det=False):
        obj, grads = np.full(self.B, np.nan), [None] * self.B
        ran = []
        for b, (xy, y, mu) in enumerate(self.problems):
            if active is not None and not active[b]:
                continue
            ran.append(b)
            obj[b] = O.elbo_eval(cov_pars[b], cov_fun, xus[b], xy, y, mu, delta)
            grads[b] = O.delbo_dcov_par(cov_pars[b], cov_fun, xus[b], xy, y, mu, delta)["gradient"]
            self.last[b] = (OrderedDict(cov_pars[b]), np.array(xus[b]), delta)
        self.calls.append(ran)
        return obj, grads, np.zeros(self.B, dtype=np.int32)

    def posterior_u(self, muus):
        res = [O.vi_posterior_u(cp, "sqexp", xu, *self.problems[b], muus[b], dl)
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
                                 # problem 0's |obj step| falls to 1.753 at iteration 7 (1.805
                                 # before); the others stay above 2.0 to the end
                                 {"maxit": 14, "obj_tol": 1.78},
                                 {"maxit": 6, "obj_tol": 0.0, "optim_method": "ga",
                                  "learn_rate": 1e-3}])
def test_lockstep_driver_equals_the_single_driver(opt):
    import sparsergps_amd as S
    ps = _problems()
    fake = FakeBatch([p[0] for p in ps])
    res = S.norm_grad_ascent_vi_batch([p[2] for p in ps], "sqexp", [p[1] for p in ps], fake,
                                      opt=opt)
    iters = []
    for b, ((xy, y, mu), xu, cp) in enumerate(ps):
        ref = OD.norm_grad_ascent_vi(cp, "sqexp", xu, xy, y, mu, opt=opt)
        r = res[b]
        assert r["iter"] == ref["iter"] and list(r["cov_par"]) == list(cp)
        for key in ("obj_fun", "grad", "cov_par_history"):
            np.testing.assert_allclose(r[key], np.asarray(ref[key]), rtol=1e-12, atol=0.0,
                                       err_msg=key)
        np.testing.assert_allclose(r["u_mean"], ref["u_mean"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(r["u_var"], ref["u_var"], rtol=1e-9, atol=1e-12)
        assert "error" not in r
        iters.append(ref["iter"])
    # one evaluation per iteration for the whole batch, and a retired problem never runs again
    assert len(fake.calls) == max(iters)
    for b, k in enumerate(iters):
        assert [b in ran for ran in fake.calls] == [True] * k + [False] * (max(iters) - k)
    if "obj_tol" in opt and opt["obj_tol"] > 0:
        assert len(set(iters)) > 1, iters          # the problems do stop at different iterations


def test_lockstep_driver_retires_a_failing_problem():
    import sparsergps_amd as S
    ps = _problems()

    class Failing(FakeBatch):
        def eval_vi(self, *a, **k):
            obj, grads, st = super().eval_vi(*a, **k)
            if len(self.calls) == 3:
                obj[1], st[1] = np.nan, 5
            return obj, grads, st

    fake = Failing([p[0] for p in ps])
    res = S.norm_grad_ascent_vi_batch([p[2] for p in ps], "sqexp", [p[1] for p in ps], fake,
                                      opt={"maxit": 6, "obj_tol": 0.0})
    assert isinstance(res[1]["error"], S.NotPositiveDefinite)
    assert "order 5 of Sigma22" in str(res[1]["error"]) and res[1]["u_mean"] is None
    assert len(res[1]["obj_fun"]) == 2
    assert all(1 not in ran for ran in fake.calls[3:])
    for b in (0, 2):
        assert res[b]["iter"] == 6 and "error" not in res[b] and res[b]["u_mean"] is not None
