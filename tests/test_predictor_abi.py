"""The resident predictor's C ABI without a GPU: symbols, prototypes, header text, every
SGP_EINVAL case (sgp_diag_predictor_args is the very check sgp_predictor_create runs before its
first device call), NULL handles, the chunk plan, and the loud failure without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sgp_predictor_create", "sgp_predictor_destroy", "sgp_predictor_run",
           "sgp_predictor_run_nlp", "sgp_predictor_run_dev", "sgp_diag_predictor_args",
           "sgp_diag_predictor_plan", "sgp_diag_predictor_run")


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
    assert nargs == {"sgp_predictor_create": 15, "sgp_predictor_destroy": 1,
                     "sgp_predictor_run": 7, "sgp_predictor_run_nlp": 13,
                     "sgp_predictor_run_dev": 10, "sgp_diag_predictor_args": 13,
                     "sgp_diag_predictor_plan": 8, "sgp_diag_predictor_run": 10}
    create = _lib.PROTOTYPES["sgp_predictor_create"][1]
    assert create[0] is C.POINTER(C.c_void_p) and create[4] is C.c_double
    assert create[8] is C.c_int64 and create[9] is C.c_int64 and create[10] is C.c_int
    assert create[14] is C.c_int64
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    diag = open(os.path.join(ROOT, "include", "sgp_diag.h")).read()
    assert "typedef struct sgp_predictor sgp_predictor;" in text
    for name in SYMBOLS:
        src = diag if name.startswith("sgp_diag_") else text
        assert _decl_commas(src, name) == nargs[name] - 1, name
    doc = text[text.index("A resident predictor"):text.index("typedef struct sgp_predictor")]
    for cite in ("vi_functions.R:1222-1333", "laplace_approx_prediction.R:3-123",
                 "laplace_approx_prediction.R:281-405", "laplace_approx_prediction.R:128-214",
                 "laplace_approx_prediction.R:408-542"):
        assert cite in doc, cite
    assert "scored once" in doc            # which of the issue's two stats orders run_nlp takes
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", text) and lib.sgp_abi_version() == 1


def _good(d=2, m=3, kernel=0, method=1):
    U = np.asfortranarray(np.arange(m * d, dtype=np.float64).reshape(m, d))
    theta = np.array([1.5, 0.8, 0.3]) if kernel != 1 else np.array([1.5] + [0.8] * d + [0.3])
    return {"d": d, "kernel": kernel, "theta": theta, "delta": 1e-6, "method": method,
            "gaussian": 1, "U": U, "m": m, "ldu": m, "u_mean": np.linspace(-1.0, 1.0, m),
            "muu": np.zeros(m), "u_var": np.asfortranarray(0.1 * np.eye(m)), "ldv": m}


def _check(lib, a):
    from sparsergps_amd import _lib
    p = lambda v: None if v is None else _lib.dptr(v)   # noqa: E731
    return lib.sgp_diag_predictor_args(a["d"], a["kernel"], p(a["theta"]), a["delta"], a["method"],
                                       a["gaussian"], p(a["U"]), a["m"], a["ldu"], p(a["u_mean"]),
                                       p(a["muu"]), p(a["u_var"]), a["ldv"])


def test_good_arguments_pass(lib):
    from sparsergps_amd import _lib
    for method in (0, 1, 2, 3):
        assert _check(lib, _good(method=method)) == _lib.SGP_OK, method
    assert _check(lib, _good(kernel=1)) == _lib.SGP_OK                                  # ard
    assert _check(lib, {**_good(), "gaussian": 0}) == _lib.SGP_OK       # laplace, non-gaussian
    assert _check(lib, {**_good(), "delta": 0.0}) == _lib.SGP_OK
    # delta's sign is the factorisation's to judge, as in sgp_predict (SGP_ENOTPD, not SGP_EINVAL)
    assert _check(lib, {**_good(), "delta": -1e-3}) == _lib.SGP_OK
    assert _check(lib, {**_good(), "theta": np.array([1.5, 0.8, 0.0])}) == _lib.SGP_OK  # tau = 0
    assert _check(lib, _good(m=1)) == _lib.SGP_OK
    big = _good(m=300)                                                   # no 128-knot limit
    big["U"] = np.asfortranarray(np.random.default_rng(0).uniform(size=(300, 2)))
    assert _check(lib, big) == _lib.SGP_OK
    # the full methods read no u_var and no ldv
    for method in (2, 3):
        assert _check(lib, {**_good(method=method), "u_var": None, "ldv": 0}) == _lib.SGP_OK
    assert _check(lib, {**_good(method=3), "muu": np.array([-1.0, 0.0, -0.5])}) == _lib.SGP_OK


BAD = {
    "exp refused": ({"kernel": 2}, b"'sqexp' and 'ard'"),
    "unknown kernel": ({"kernel": 7}, b"covariance function"),
    "unknown method": ({"method": 4}, b"invalid prediction method 4"),
    "method < 0": ({"method": -1}, b"invalid prediction method -1"),
    "theta NULL": ({"theta": None}, b"NULL"),
    "U NULL": ({"U": None}, b"NULL"),
    "u_mean NULL": ({"u_mean": None}, b"NULL"),
    "muu NULL": ({"muu": None}, b"NULL"),
    "u_var NULL, laplace": ({"u_var": None}, b"NULL"),
    "u_var NULL, vi": ({"u_var": None, "method": 0}, b"NULL"),
    "m = 0": ({"m": 0}, b"m=0"),
    "ldu < m": ({"ldu": 2}, b"ldu"),
    "ldv < m": ({"ldv": 2}, b"ldv"),
    "sigma = 0": ({"theta": np.array([0.0, 0.8, 0.3])}, b"sigma"),
    "sigma < 0": ({"theta": np.array([-1.5, 0.8, 0.3])}, b"sigma"),
    "l = 0": ({"theta": np.array([1.5, 0.0, 0.3])}, b"l > 0"),
    "l < 0": ({"theta": np.array([1.5, -0.8, 0.3])}, b"l > 0"),
    "tau < 0": ({"theta": np.array([1.5, 0.8, -0.1])}, b"tau"),
    "sigma NaN": ({"theta": np.array([np.nan, 0.8, 0.3])}, b"theta[0]"),
    "l inf": ({"theta": np.array([1.5, np.inf, 0.3])}, b"theta[1]"),
    "tau NaN": ({"theta": np.array([1.5, 0.8, np.nan])}, b"theta[2]"),
    "delta NaN": ({"delta": float("nan")}, b"delta"),
    "delta inf": ({"delta": float("inf")}, b"delta"),
    "u_mean NaN": ({"u_mean": np.array([0.0, np.nan, 1.0])}, b"u_mean[1]"),
    "muu inf": ({"muu": np.array([0.0, 0.0, np.inf])}, b"muu[2]"),
    "d = 0": ({"d": 0}, b"dimension"),
    "d = 33": ({"d": 33}, b"dimension"),
    "vi, non-gaussian": ({"method": 0, "gaussian": 0},
                         b"Error: VI not supported for non-gaussian data."),
    "W > 0": ({"method": 3, "muu": np.array([-1.0, 0.25, -1.0])}, b"W[1] = 0.25 is not <= 0"),
    "W NaN": ({"method": 3, "muu": np.array([-1.0, -1.0, np.nan])}, b"muu[2]"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_einval_before_any_device_call(lib, name):
    from sparsergps_amd import _lib
    change, needle = BAD[name]
    assert _check(lib, {**_good(), **change}) == _lib.SGP_EINVAL
    assert needle in lib.sgp_last_error(), lib.sgp_last_error()


def test_create_runs_the_same_check_first(lib):
    """sgp_predictor_create returns these before its first device call: the same status and
    message on a machine without a GPU, and no handle."""
    from sparsergps_amd import _lib
    for name in ("exp refused", "unknown method", "vi, non-gaussian", "W > 0", "u_var NULL, vi"):
        change, needle = BAD[name]
        a = {**_good(), **change}
        p = lambda v: None if v is None else _lib.dptr(v)   # noqa: E731
        h = C.c_void_p()
        st = lib.sgp_predictor_create(C.byref(h), 0, a["kernel"], p(a["theta"]), a["delta"],
                                      a["method"], a["gaussian"], p(a["U"]), a["m"], a["ldu"],
                                      a["d"], p(a["u_mean"]), p(a["muu"]), p(a["u_var"]), a["ldv"])
        assert st == _lib.SGP_EINVAL and needle in lib.sgp_last_error(), name
        assert h.value is None
    assert lib.sgp_predictor_create(None, 0, 0, None, 0.0, 0, 1, None, 1, 1, 1, None, None, None,
                                    1) == _lib.SGP_EINVAL


def test_ard_length_scales_are_each_checked(lib):
    from sparsergps_amd import _lib
    a = _good(kernel=1)
    assert _check(lib, {**a, "theta": np.array([1.5, 0.8, -0.2, 0.3])}) == _lib.SGP_EINVAL
    assert b"length scale 2" in lib.sgp_last_error()
    assert _check(lib, {**a, "theta": np.array([1.5, 0.8, 0.8, np.nan])}) == _lib.SGP_EINVAL
    assert b"theta[3]" in lib.sgp_last_error()


def test_non_finite_knots_and_u_var_are_einval(lib):
    from sparsergps_amd import _lib
    for bad in (np.nan, np.inf):
        a = _good()
        a["U"][1, 1] = bad
        assert _check(lib, a) == _lib.SGP_EINVAL and b"U[1, 1]" in lib.sgp_last_error()
        a = _good()
        a["u_var"][2, 0] = bad
        assert _check(lib, a) == _lib.SGP_EINVAL and b"u_var[2, 0]" in lib.sgp_last_error()
        a = _good(method=2)          # the full methods do not read u_var
        a["u_var"][2, 0] = bad
        assert _check(lib, a) == _lib.SGP_OK


def test_null_handles(lib):
    from sparsergps_amd import _lib
    x, v = np.zeros((4, 2), order="F"), np.zeros(4)
    st = lib.sgp_predictor_run(None, _lib.dptr(x), 4, 4, _lib.dptr(v), _lib.dptr(v), _lib.dptr(v))
    assert st == _lib.SGP_EINVAL and b"sgp_predictor" in lib.sgp_last_error()
    st = lib.sgp_predictor_run_nlp(None, _lib.dptr(x), 4, 4, _lib.dptr(v), _lib.dptr(v),
                                   _lib.dptr(v), 2, _lib.dptr(v), 0.1, None, _lib.dptr(v),
                                   _lib.dptr(v))
    assert st == _lib.SGP_EINVAL and b"sgp_predictor" in lib.sgp_last_error()
    assert lib.sgp_predictor_run_dev(None, None, 4, 4, None, None, None, None, None,
                                     None) == _lib.SGP_EINVAL
    assert lib.sgp_diag_predictor_run(None, 0, 0, _lib.dptr(x), 4, 4, _lib.dptr(v), _lib.dptr(v),
                                      _lib.dptr(v), None) == _lib.SGP_EINVAL
    assert lib.sgp_predictor_destroy(None) == _lib.SGP_EINVAL
    assert b"sgp_predictor_destroy" in lib.sgp_last_error()


def _plan(lib, m, np_, budget, d=8):
    out = [C.c_int64(0) for _ in range(4)]
    st = lib.sgp_diag_predictor_plan(m, d, np_, budget, *(C.byref(o) for o in out))
    return st, [o.value for o in out]


@pytest.mark.parametrize("m", [20, 130, 300, 1024])
def test_plan(lib, m):
    from sparsergps_amd import _lib
    mp = (m + 127) // 128 * 128
    nb = mp // 128
    for np_ in (1, 129, 100_000, 1_000_000, 3_000_000_000):
        for budget in (0, 64 << 20, 128 << 20, 256 << 20, 1024 << 20, 1):
            st, (rows, nchunks, sym, full) = _plan(lib, m, np_, budget)
            assert st == _lib.SGP_OK
            assert rows % 128 == 0 and rows >= 128
            assert nchunks * rows >= np_ and (nchunks - 1) * rows < np_
            assert rows <= (np_ + 127) // 128 * 128
            if budget >= 128 * mp * 8:
                assert rows * mp * 8 <= budget
                # the largest such multiple, unless np needs fewer rows
                assert (rows + 128) * mp * 8 > budget or rows == (np_ + 127) // 128 * 128
            elif budget:
                assert rows == 128                                     # never below one tile
            assert sym == nb * (nb + 1) // 2 and full == nb * nb
    # the product's budget is a fixed one: the plan at budget 0 is one of the measured candidates
    rows0 = _plan(lib, m, 10 ** 9, 0)[1][0]
    assert rows0 in [_plan(lib, m, 10 ** 9, b << 20)[1][0] for b in (64, 128, 256, 1024)]


def test_plan_einval(lib):
    from sparsergps_amd import _lib
    for args in ((0, 100, 0), (20, 0, 0), (20, 100, -1)):
        st, _ = _plan(lib, *args)
        assert st == _lib.SGP_EINVAL and b"sgp_diag_predictor_plan" in lib.sgp_last_error()
    assert _plan(lib, 20, 100, 0, d=0)[0] == _lib.SGP_EINVAL
    assert lib.sgp_diag_predictor_plan(20, 2, 100, 0, None, None, None, None) == _lib.SGP_EINVAL


def test_no_gpu_no_fallback():
    """Without a HIP device Predictor(...) raises SGPError (argument errors come first, also as
    SGPError); there is no CPU path behind it."""
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    cp = {"sigma": 1.5, "l": 0.8, "tau": 0.3}
    xu = np.arange(6.0).reshape(3, 2)
    with pytest.raises(S.SGPError, match="'sqexp' and 'ard'"):
        S.Predictor("laplace", np.zeros(3), 0.1 * np.eye(3), xu, "exp", cp, 0.0)
    with pytest.raises(S.SGPError, match="VI not supported"):
        S.Predictor("vi", np.zeros(3), 0.1 * np.eye(3), xu, "sqexp", cp, 0.0, family="poisson")
    n = C.c_int(0)
    if _lib.lib().sgp_device_count(C.byref(n)) == _lib.SGP_OK and n.value > 0:
        return                                            # the GPU suite covers the rest
    with pytest.raises(S.SGPError):
        S.Predictor("laplace", np.zeros(3), 0.1 * np.eye(3), xu, "sqexp", cp, 0.0)


def test_python_surface_exists():
    import sparsergps_amd as S
    for name in ("Predictor", "predictor_gp"):
        assert callable(getattr(S, name)) and name in S.__all__
    for meth in ("predict", "score", "predict_torch", "close", "__enter__", "__exit__"):
        assert callable(getattr(S.Predictor, meth))
    with pytest.raises(ValueError, match="method"):
        S.Predictor("nope", np.zeros(3), None, np.zeros((3, 2)), "sqexp", {}, 0.0)
    mod = {"family": "poisson", "sparse": True, "results": {}}
    assert S.predictor_gp(mod, vi=True) == "Error: VI not supported for non-gaussian data."
