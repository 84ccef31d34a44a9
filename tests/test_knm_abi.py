"""sgp_diag_exp and sgp_diag_build_knm without a GPU: the symbols, their prototypes, and every
SGP_EINVAL case, all of which return before the first device call; and the check, on the CPU,
that the derived direct-difference bar of tests/knm_cases.py admits the correctly computed answer
(K by direct differences in plain float64 numpy) on every case tests/test_gpu_knm.py runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import knm_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    return _lib.lib()


def test_symbols_prototypes_and_header(lib):
    from sparsergps_amd import _lib
    assert hasattr(lib, "sgp_diag_exp") and hasattr(lib, "sgp_diag_build_knm")
    res, args = _lib.PROTOTYPES["sgp_diag_exp"]
    assert res is C.c_int and len(args) == 6 and args[3] is C.c_int64 and args[4] is C.c_double
    res, args = _lib.PROTOTYPES["sgp_diag_build_knm"]
    assert res is C.c_int and len(args) == 18
    assert args[5] is C.c_int64 and args[11] is C.c_int and args[12] is C.c_int64
    assert args[16] is C.POINTER(C.c_int) and args[17] is C.POINTER(C.c_int64)
    text = open(os.path.join(ROOT, "include", "sgp_diag.h")).read()
    for name, commas in (("sgp_diag_exp", 5), ("sgp_diag_build_knm", 17)):
        decl = re.sub(r"\s+", " ", text[text.index(f"int {name}("):])
        assert decl[:decl.index(";")].count(",") == commas
    sgp_h = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", sgp_h) and lib.sgp_abi_version() == 1


def test_dead_exp_variant_is_gone():
    csrc = os.path.join(ROOT, "sparsergps_amd", "csrc")
    for f in os.listdir(csrc):
        assert "sgp_exp_kp" not in open(os.path.join(csrc, f)).read(), f


def _exp(lib, which=0, x=np.array([-1.0, -2.0]), n=2, hi=0.0, out=np.zeros(2)):
    from sparsergps_amd import _lib
    p = lambda v: None if v is None else _lib.dptr(v)   # noqa: E731
    return lib.sgp_diag_exp(0, which, p(x), n, hi, p(out))


EXP_BAD = {
    "x NULL": ({"x": None}, b"NULL"),
    "out NULL": ({"out": None}, b"NULL"),
    "n = 0": ({"n": 0}, b"n < 1"),
    "which = 2": ({"which": 2}, b"which=2"),
    "which = -1": ({"which": -1}, b"which=-1"),
    "hi NaN": ({"which": 1, "hi": float("nan")}, b"hi="),
    "hi above log(DBL_MAX)": ({"which": 1, "hi": 709.79}, b"hi="),
}


@pytest.mark.parametrize("name", sorted(EXP_BAD))
def test_exp_einval_before_any_device_call(lib, name):
    from sparsergps_amd import _lib
    change, needle = EXP_BAD[name]
    assert _exp(lib, **change) == _lib.SGP_EINVAL
    assert b"sgp_diag_exp" in lib.sgp_last_error() and needle in lib.sgp_last_error()


def _good(d=2, n=5, m=3, kernel=0):
    X = np.asfortranarray(np.arange(n * d, dtype=np.float64).reshape(n, d))
    U = np.asfortranarray(X[:m].copy())
    theta = np.array([1.2, 1.0, 0.5]) if kernel != 1 else np.array([1.2] + [1.0] * d + [0.5])
    return {"kernel": kernel, "d": d, "theta": theta, "X": X, "n": n, "ldx": n, "U": U, "m": m,
            "ldu": m, "r": None, "route": 0, "max_rows": 0, "shared_rb": 0,
            "K": np.zeros((128, 128)), "t": None, "taken": C.c_int(0), "t_rows": None}


def _build(lib, a):
    from sparsergps_amd import _lib
    p = lambda v: None if v is None else _lib.dptr(v)   # noqa: E731
    ref = lambda v: None if v is None else C.byref(v)   # noqa: E731
    return lib.sgp_diag_build_knm(0, a["kernel"], a["d"], p(a["theta"]), p(a["X"]), a["n"],
                                  a["ldx"], p(a["U"]), a["m"], a["ldu"], p(a["r"]), a["route"],
                                  a["max_rows"], a["shared_rb"], p(a["K"]), p(a["t"]),
                                  ref(a["taken"]), ref(a["t_rows"]))


BUILD_BAD = {
    "X NULL": ({"X": None}, b"NULL"),
    "U NULL": ({"U": None}, b"NULL"),
    "K NULL": ({"K": None}, b"NULL"),
    "theta NULL": ({"theta": None}, b"NULL"),
    "route_taken NULL": ({"taken": None}, b"NULL"),
    "r without t": ({"r": np.zeros(5), "t_rows": C.c_int64(0)}, b"t or t_rows"),
    "r without t_rows": ({"r": np.zeros(5), "t": np.zeros(128)}, b"t or t_rows"),
    "n = 0": ({"n": 0}, b"n=0"),
    "ldx < n": ({"ldx": 4}, b"ldx=4"),
    "m = 0": ({"m": 0}, b"m=0"),
    "ldu < m": ({"ldu": 2}, b"ldu=2"),
    "d = 0": ({"d": 0}, b"dimension"),
    "d = 33": ({"d": 33}, b"dimension"),
    "d = 33, matrix cores": ({"d": 33, "route": 1}, b"dimension"),
    "route = 3": ({"route": 3}, b"route=3"),
    "route = -1": ({"route": -1}, b"route=-1"),
    "max_rows < 0": ({"max_rows": -1}, b"max_rows=-1"),
    "shared_rb < -1": ({"shared_rb": -2}, b"shared_rb=-2"),
    "exp kernel": ({"kernel": 2}, b"'exp'"),
    "unknown kernel": ({"kernel": 7}, b"covariance function"),
    "sigma = 0": ({"theta": np.array([0.0, 1.0, 0.5])}, b"sigma"),
    "sigma NaN": ({"theta": np.array([np.nan, 1.0, 0.5])}, b"sigma"),
    "l = 0": ({"theta": np.array([1.2, 0.0, 0.5])}, b"length scale"),
    "l NaN": ({"theta": np.array([1.2, np.nan, 0.5])}, b"length scale"),
}


@pytest.mark.parametrize("name", sorted(BUILD_BAD))
def test_build_einval_before_any_device_call(lib, name):
    from sparsergps_amd import _lib
    change, needle = BUILD_BAD[name]
    a = {**_good(), **change}
    assert _build(lib, a) == _lib.SGP_EINVAL
    assert needle in lib.sgp_last_error(), lib.sgp_last_error()
    assert a["taken"] is None or a["taken"].value == 0      # nothing was decided, nothing ran


def test_ard_theta_length_scale_is_checked(lib):
    from sparsergps_amd import _lib
    a = _good(d=3, kernel=1)
    a["theta"][2] = -1.0
    assert _build(lib, a) == _lib.SGP_EINVAL and b"length scale 2" in lib.sgp_last_error()


# --------------------------------------------------------------------- the bars, on the CPU
def test_case_list_is_the_issue_s():
    cases = KC.build_cases()
    shapes = {(c["n"], c["m"]) for c in cases.values()}
    for m in (1, 127, 128, 129):
        assert (65, m) in shapes
    for n in (1, 63, 64, 65, 130):
        assert (n, 17) in shapes
    assert (321, 129) in shapes
    for d in (1, 4, 8, 9, 16, 17, 32):
        for k in ("sqexp", "ard"):
            c = cases[f"nc_d{d}_{k}"]
            assert (c["n"], c["m"], c["d"], c["kernel"]) == (65, 33, d, k) and c["routes"] == (1, 2)
    assert {c["sigma"] for c in cases.values()} >= {1e-150, 1.2, 1e150}
    assert cases["offset_5e3"]["X"].min() >= 5e3 and cases["offset_5e3"]["d"] == 3
    assert cases["tail_l025"]["ls"][0] == 0.25 and cases["tail_l025"]["m"] == 5


def test_tail_cases_reach_the_underflow_tail():
    cases = KC.build_cases()
    smax = KC.span2_max()
    K, e, _ = KC.reference(cases["tail_l025"])
    K64 = K.astype(np.float64)
    tiny = np.finfo(np.float64).tiny
    assert e.min() == -800.0
    assert (K64 == 0).any() and ((K64 > 0) & (K64 < tiny)).any() and (K64 >= tiny).any()
    # span^2 = (5 / 0.25)^2 = 400 is inside the guard: the product builds this case on the matrix
    # cores (d = 1 on [0, 10] cannot exceed the guard before the exponents reach -20000)
    assert KC.span2(cases["tail_l025"]) == 400.0 and KC.expected_route(cases["tail_l025"]) == 1
    c9 = cases["tail_span09"]
    assert 0.899 * smax <= KC.span2(c9) <= 0.901 * smax and KC.expected_route(c9) == 1
    K9 = KC.reference(c9)[0].astype(np.float64)
    assert int((K9 < tiny).sum()) >= 50                  # subnormal or zero
    assert KC.span2(cases["tail_span16"]) > smax and KC.expected_route(cases["tail_span16"]) == 2
    bad, fin, i_inf, i_nan = KC.nonfinite_case()
    assert KC.expected_route(bad) == 2 and KC.expected_route(fin) == 1 and i_inf != i_nan


def test_direct_bar_admits_float64_numpy():
    """A bar that rejects the correctly computed answer is wrong: K by direct differences in plain
    float64 numpy stays inside the direct-difference bar on every case (largest ratio of error to
    bar over all cases: 0.36, profiles/knm_direct/README.md)."""
    worst = 0.0
    for name, c in sorted(KC.build_cases().items()):
        ref = KC.reference(c)
        bar = KC.bars(c, ref)[2]
        err = np.abs(KC.numpy_direct(c).astype(np.longdouble) - ref[0])
        assert (bar > 0).all(), name
        ratio = float((err / bar).max())
        print(f"{name}: numpy float64 direct differences, max err / bar = {ratio:.3f}")
        assert (err <= bar).all(), (name, ratio)
        worst = max(worst, ratio)
    print(f"worst: {worst:.3f}")
