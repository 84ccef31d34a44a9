"""sgp_ego_scan's C ABI without a GPU: the symbol, its prototype, and every SGP_EINVAL case,
all of which return before the first device call (sgp_diag_ego_args is the very check
sgp_ego_scan runs, callable without a context)."""
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
    assert hasattr(lib, "sgp_ego_scan") and hasattr(lib, "sgp_diag_ego_args")
    res, args = _lib.PROTOTYPES["sgp_ego_scan"]
    assert res is C.c_int and len(args) == 16
    assert args[0] is C.c_void_p and args[1] is C.c_int and args[3] is C.c_double
    assert args[5] is C.c_int64 and args[6] is C.c_int64 and args[9] is C.c_int64
    assert args[11] is C.POINTER(C.c_int64)
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert re.search(r"#define\s+SGP_EGO_TMAX\s+128\b", text)
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", text) and lib.sgp_abi_version() == 1
    decl = re.sub(r"\s+", " ", text[text.index("int sgp_ego_scan("):])
    decl = decl[:decl.index(";")]
    assert decl.count(",") == 15
    for cite in ("vi_functions.R:1927-1950", "2074-2097", "knot_proposal_functions.R:355-379"):
        assert cite in text


def _good(d=2, T=3):
    xm = np.asfortranarray(np.arange(T * d, dtype=np.float64).reshape(T, d))
    return {"d": d, "kernel": 2, "theta": np.array([3.0, 1.0, 0.0]), "delta": 1e-9, "xm": xm,
            "T": T, "ldxm": T, "vals": np.array([-50.0, -49.0, -51.0][:T]),
            "excl": np.asfortranarray(np.zeros((2, d))), "E": 2, "ldexcl": 2}


def _check(lib, a):
    from sparsergps_amd import _lib
    p = lambda v: None if v is None else _lib.dptr(v)   # noqa: E731
    return lib.sgp_diag_ego_args(a["d"], a["kernel"], p(a["theta"]), a["delta"], p(a["xm"]),
                                 a["T"], a["ldxm"], p(a["vals"]), p(a["excl"]), a["E"], a["ldexcl"])


def test_good_arguments_pass(lib):
    from sparsergps_amd import _lib
    assert _check(lib, _good()) == _lib.SGP_OK
    assert _check(lib, {**_good(), "kernel": 0}) == _lib.SGP_OK                      # sqexp
    assert _check(lib, {**_good(), "excl": None, "E": 0, "ldexcl": 0}) == _lib.SGP_OK
    assert _check(lib, {**_good(), "delta": 0.0}) == _lib.SGP_OK
    # tau = 0 is the reference's default ego_cov_par$tau
    assert _check(lib, {**_good(), "theta": np.array([3.0, 1.0, 0.0])}) == _lib.SGP_OK
    big = np.asfortranarray(np.random.default_rng(0).uniform(size=(128, 2)))
    assert _check(lib, {**_good(), "xm": big, "T": 128, "ldxm": 128,
                        "vals": np.arange(128.0)}) == _lib.SGP_OK


BAD = {
    "ard refused": ({"kernel": 1}, b"ard"),
    "unknown kernel": ({"kernel": 7}, b"covariance function"),
    "theta NULL": ({"theta": None}, b"NULL"),
    "xm NULL": ({"xm": None}, b"NULL"),
    "vals NULL": ({"vals": None}, b"NULL"),
    "T = 0": ({"T": 0}, b"T=0"),
    "T = 129": ({"T": 129, "ldxm": 129}, b"T=129"),
    "ldxm < T": ({"ldxm": 2}, b"ldxm"),
    "E < 0": ({"E": -1}, b"exclusion"),
    "ldexcl < E": ({"ldexcl": 1}, b"exclusion"),
    "sigma = 0": ({"theta": np.array([0.0, 1.0, 0.0])}, b"sigma"),
    "sigma < 0": ({"theta": np.array([-3.0, 1.0, 0.0])}, b"sigma"),
    "l = 0": ({"theta": np.array([3.0, 0.0, 0.0])}, b"l > 0"),
    "tau < 0": ({"theta": np.array([3.0, 1.0, -0.1])}, b"tau"),
    "sigma NaN": ({"theta": np.array([np.nan, 1.0, 0.0])}, b"theta_meta[0]"),
    "l inf": ({"theta": np.array([3.0, np.inf, 0.0])}, b"theta_meta[1]"),
    "tau NaN": ({"theta": np.array([3.0, 1.0, np.nan])}, b"theta_meta[2]"),
    "delta < 0": ({"delta": -1e-9}, b"delta_meta"),
    "delta NaN": ({"delta": float("nan")}, b"delta_meta"),
    "vals NaN": ({"vals": np.array([-50.0, np.nan, -51.0])}, b"vals[1]"),
    "vals inf": ({"vals": np.array([-50.0, -49.0, np.inf])}, b"vals[2]"),
    "d = 0": ({"d": 0}, b"dimension"),
    "d = 33": ({"d": 33}, b"dimension"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_einval_before_any_device_call(lib, name):
    from sparsergps_amd import _lib
    change, needle = BAD[name]
    assert _check(lib, {**_good(), **change}) == _lib.SGP_EINVAL
    assert needle in lib.sgp_last_error(), lib.sgp_last_error()


def test_non_finite_xm_is_einval(lib):
    from sparsergps_amd import _lib
    for bad in (np.nan, np.inf):
        a = _good()
        a["xm"][1, 1] = bad
        assert _check(lib, a) == _lib.SGP_EINVAL and b"xm[1, 1]" in lib.sgp_last_error()
    a = _good()
    wide = np.asfortranarray(np.vstack([a["xm"], [[np.nan, np.nan]]]))   # ld 4, row 3 unused
    assert _check(lib, {**a, "xm": wide, "ldxm": 4}) == _lib.SGP_OK


def test_null_context_and_outputs(lib):
    from sparsergps_amd import _lib
    a = _good()
    row, ei = C.c_int64(0), C.c_double(0.0)
    st = lib.sgp_ego_scan(None, 2, _lib.dptr(a["theta"]), 1e-9, _lib.dptr(a["xm"]), 3, 3,
                          _lib.dptr(a["vals"]), None, 0, 0, C.byref(row), C.byref(ei), None, None,
                          None)
    assert st == _lib.SGP_EINVAL and b"sgp_ego_scan" in lib.sgp_last_error()


def test_python_surface_exists():
    import sparsergps_amd as S
    for name in ("knot_prop_ego_norm_vi", "knot_prop_ego_norm", "knot_prop_ego"):
        assert callable(getattr(S, name)) and name in S.__all__
    assert callable(S.SparseGPContext.ego_scan)
