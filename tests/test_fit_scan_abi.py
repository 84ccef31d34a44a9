"""sgp_fit_scan's C ABI without a GPU: the symbol, its prototype, the header text, and every
SGP_EINVAL case, all of which return before the first device call (sgp_diag_fit_scan_args is the
very check sgp_fit_scan runs, callable without a context)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    return _lib.lib()


def test_symbol_prototype_and_header(lib):
    from sparsergps_amd import _lib
    assert hasattr(lib, "sgp_fit_scan") and hasattr(lib, "sgp_diag_fit_scan_args")
    res, args = _lib.PROTOTYPES["sgp_fit_scan"]
    assert res is C.c_int and len(args) == 22
    assert args[0] is C.c_void_p and args[1] is C.c_int and args[3] is C.c_double
    assert args[4] is C.c_int and args[6] is C.c_int64 and args[7] is C.c_int64
    assert args[11] is C.c_int64 and args[12] is C.c_int
    assert args[15] is C.c_int64 and args[16] is C.c_int64 and args[17] is C.POINTER(C.c_int64)
    assert (_lib.SGP_SCAN_VAR, _lib.SGP_SCAN_ERROR) == (0, 1)
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert re.search(r"enum\s*\{\s*SGP_SCAN_VAR\s*=\s*0\s*,\s*SGP_SCAN_ERROR\s*=\s*1\s*\}", text)
    assert re.search(r"#define\s+SGP_EGO_TMAX\s+128\b", text)
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", text) and lib.sgp_abi_version() == 1
    decl = re.sub(r"\s+", " ", text[text.index("int sgp_fit_scan("):])
    decl = decl[:decl.index(";")]
    assert decl.count(",") == 21
    for cite in ("knot_proposal_functions.R:4-42", "laplace_approx_prediction.R:3-123"):
        assert cite in text
    diag = open(os.path.join(ROOT, "include", "sgp_diag.h")).read()
    assert "int sgp_diag_fit_scan_args(" in diag


def _good(d=2, m=3, kernel=0):
    U = np.asfortranarray(np.arange(m * d, dtype=np.float64).reshape(m, d))
    theta = np.array([1.5, 0.8, 0.3]) if kernel != 1 else np.array([1.5] + [0.8] * d + [0.3])
    return {"d": d, "kernel": kernel, "theta": theta, "delta": 1e-6, "U": U, "m": m, "ldu": m,
            "u_mean": np.linspace(-1.0, 1.0, m), "muu": np.zeros(m),
            "u_var": np.asfortranarray(0.1 * np.eye(m)), "ldv": m, "mode": 0,
            "excl": np.asfortranarray(np.zeros((2, d))), "E": 2, "ldexcl": 2}


def _check(lib, a):
    from sparsergps_amd import _lib
    p = lambda v: None if v is None else _lib.dptr(v)   # noqa: E731
    return lib.sgp_diag_fit_scan_args(a["d"], a["kernel"], p(a["theta"]), a["delta"], p(a["U"]),
                                      a["m"], a["ldu"], p(a["u_mean"]), p(a["muu"]),
                                      p(a["u_var"]), a["ldv"], a["mode"], p(a["excl"]), a["E"],
                                      a["ldexcl"])


def _big(m):
    g = _good(m=m)
    g["U"] = np.asfortranarray(np.random.default_rng(0).uniform(size=(m, 2)))
    return g


def test_good_arguments_pass(lib):
    from sparsergps_amd import _lib
    assert _check(lib, _good()) == _lib.SGP_OK
    assert _check(lib, _good(kernel=1)) == _lib.SGP_OK                                  # ard
    assert _check(lib, {**_good(), "mode": 1}) == _lib.SGP_OK
    assert _check(lib, {**_good(), "excl": None, "E": 0, "ldexcl": 0}) == _lib.SGP_OK
    assert _check(lib, {**_good(), "delta": 0.0}) == _lib.SGP_OK
    assert _check(lib, {**_good(), "theta": np.array([1.5, 0.8, 0.0])}) == _lib.SGP_OK  # tau = 0
    assert _check(lib, _big(128)) == _lib.SGP_OK
    assert _check(lib, _good(m=1)) == _lib.SGP_OK


BAD = {
    "exp refused": ({"kernel": 2}, b"'sqexp' and 'ard'"),
    "unknown kernel": ({"kernel": 7}, b"covariance function"),
    "theta NULL": ({"theta": None}, b"NULL"),
    "U NULL": ({"U": None}, b"NULL"),
    "u_mean NULL": ({"u_mean": None}, b"NULL"),
    "muu NULL": ({"muu": None}, b"NULL"),
    "u_var NULL": ({"u_var": None}, b"NULL"),
    "m = 0": ({"m": 0}, b"m=0"),
    "ldu < m": ({"ldu": 2}, b"ldu"),
    "ldv < m": ({"ldv": 2}, b"ldv"),
    "mode = 2": ({"mode": 2}, b"mode=2"),
    "mode < 0": ({"mode": -1}, b"mode=-1"),
    "E < 0": ({"E": -1}, b"exclusion"),
    "ldexcl < E": ({"ldexcl": 1}, b"exclusion"),
    "sigma = 0": ({"theta": np.array([0.0, 0.8, 0.3])}, b"sigma"),
    "sigma < 0": ({"theta": np.array([-1.5, 0.8, 0.3])}, b"sigma"),
    "l = 0": ({"theta": np.array([1.5, 0.0, 0.3])}, b"l > 0"),
    "l < 0": ({"theta": np.array([1.5, -0.8, 0.3])}, b"l > 0"),
    "tau < 0": ({"theta": np.array([1.5, 0.8, -0.1])}, b"tau"),
    "sigma NaN": ({"theta": np.array([np.nan, 0.8, 0.3])}, b"theta[0]"),
    "l inf": ({"theta": np.array([1.5, np.inf, 0.3])}, b"theta[1]"),
    "tau NaN": ({"theta": np.array([1.5, 0.8, np.nan])}, b"theta[2]"),
    "delta < 0": ({"delta": -1e-9}, b"delta"),
    "delta NaN": ({"delta": float("nan")}, b"delta"),
    "u_mean NaN": ({"u_mean": np.array([0.0, np.nan, 1.0])}, b"u_mean[1]"),
    "muu inf": ({"muu": np.array([0.0, 0.0, np.inf])}, b"muu[2]"),
    "d = 0": ({"d": 0}, b"dimension"),
    "d = 33": ({"d": 33}, b"dimension"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_einval_before_any_device_call(lib, name):
    from sparsergps_amd import _lib
    change, needle = BAD[name]
    assert _check(lib, {**_good(), **change}) == _lib.SGP_EINVAL
    assert needle in lib.sgp_last_error(), lib.sgp_last_error()


def test_129_knots_are_einval(lib):
    from sparsergps_amd import _lib
    assert _check(lib, _big(129)) == _lib.SGP_EINVAL
    assert b"m=129" in lib.sgp_last_error() and b"128" in lib.sgp_last_error()


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
    a = _good()
    wide = np.asfortranarray(np.vstack([a["U"], [[np.nan, np.nan]]]))   # ld 4, row 3 unused
    assert _check(lib, {**a, "U": wide, "ldu": 4}) == _lib.SGP_OK


def test_null_context_and_outputs(lib):
    from sparsergps_amd import _lib
    a = _good()
    row, key = C.c_int64(0), C.c_double(0.0)
    st = lib.sgp_fit_scan(None, 0, _lib.dptr(a["theta"]), 1e-6, 1, _lib.dptr(a["U"]), 3, 3,
                          _lib.dptr(a["u_mean"]), _lib.dptr(a["muu"]), _lib.dptr(a["u_var"]), 3,
                          0, None, None, 0, 0, C.byref(row), C.byref(key), None, None, None)
    assert st == _lib.SGP_EINVAL and b"sgp_fit_scan" in lib.sgp_last_error()


def test_python_surface_exists():
    import sparsergps_amd as S
    assert callable(S.SparseGPContext.fit_scan)
    for name in ("knot_prop_var", "knot_prop_error"):
        assert callable(getattr(S, name)) and name in S.__all__
