"""Inputs, references and bars shared by tests/test_gpu_exp.py, tests/test_gpu_knm.py,
and tests/test_knm_abi.py.

Two things are pinned entry by entry:

* the device exp functions (sgp_internal.h: sgp_exp_nonpos, sgp_exp_tab) against mpmath.exp at 60
  digits, in ulps of the correctly rounded result (np.spacing, so a subnormal result is measured in
  subnormal spacing): EXP_BAR_ULP = 2 everywhere;
* the two K12 builders (k_cov.hip: k_build_knm, k_build_knm_mfma) against
  K_ij = sigma^2 exp(-1/2 sum_c ((x_ic - u_jc) / l_c)^2) computed from the double inputs in
  np.longdouble, with the derived bars of ``bars`` below.

Nothing here touches the library: every reference is recomputed from the inputs.
"""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
EXP_BAR_ULP = 2.0
LOG_DBL_MAX = 709.782712893384          # the largest double whose exp is finite
UNDERFLOW = -745.13321910194110842      # below it exp rounds to 0
SUBNORMAL = -708.3964185322641          # below it exp is subnormal


# ------------------------------------------------------------------------------- exp points
def _around(x, k):
    """x and the k doubles either side of it, ascending."""
    lo, hi = [x], [x]
    for _ in range(k):
        lo.append(np.nextafter(lo[-1], -np.inf))
        hi.append(np.nextafter(hi[-1], np.inf))
    return lo[:0:-1] + [x] + hi[1:]


def exp_bands(which):
    """name -> float64 array of arguments for sgp_diag_exp(which)."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 60
    ln2 = mp.log(2)
    b = {}
    b["zero_and_tiny"] = np.array([0.0, -0.0] + [-(2.0 ** -q) for q in range(1074, 29, -1)])
    pts = []
    for k in (1, 2, 3, 511, 512, 1021, 1022, 1023, 1074, 1075):
        for c in (-k * ln2, -(k + mp.mpf(1) / 2) * ln2):
            pts += _around(float(c), 2)
    b["rint_switch"] = np.array(pts)
    if which == 1:
        pts = []
        for j in list(range(65)) + [32 * 1022 + q for q in (-2, -1, 0, 1, 2)]:
            for c in (-j * ln2 / 32, -(j + mp.mpf(1) / 2) * ln2 / 32):
                pts += _around(float(c), 2)
        b["table_switch"] = np.array(pts)
    band = list(np.arange(-745.14, -708.39, 1.0 / 64))
    b["subnormal_band"] = np.array(band + _around(UNDERFLOW, 5) + _around(SUBNORMAL, 5))
    b["below"] = np.array([-746.0, -750.0, -1e3, -1e6, -1e300, -np.inf])
    rng = np.random.default_rng(20240607)
    b["log_uniform"] = -np.exp(rng.uniform(math.log(1e-8), math.log(745.0), size=2000))
    if which == 1:
        top = np.nextafter(LOG_DBL_MAX, np.inf)      # _around's lower half: the 5 doubles below
        b["positive"] = np.array(list(rng.uniform(0.0, 709.78, size=199)) + [709.78]
                                 + _around(LOG_DBL_MAX, 5)[:5])
        assert b["positive"].max() < top
    return b


def exp_ulp_error(x, got):
    """|got - exp(x)| in ulps of the correctly rounded exp(x), per entry (float64 array)."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 60
    out = np.empty(len(x))
    for i, (xi, gi) in enumerate(zip(x, got)):
        if np.isneginf(xi):
            exact = mp.mpf(0)
        else:
            exact = mp.exp(mp.mpf(float(xi)))
        cr = float(exact)                      # nearest double (its spacing is all that is used)
        sp = float(np.spacing(abs(cr)))
        if not np.isfinite(gi):
            out[i] = np.inf
        else:
            out[i] = float(abs(mp.mpf(float(gi)) - exact) / mp.mpf(sp))
    return out


# ------------------------------------------------------------------------------- K12 cases
def span2_max():
    with open(os.path.join(ROOT, "sparsergps_amd", "csrc", "sgp_internal.h")) as f:
        mt = re.search(r"SGP_MFMA_SPAN2_MAX\s*=\s*([0-9.eE+-]+)\s*;", f.read())
    assert mt, "SGP_MFMA_SPAN2_MAX not found in sgp_internal.h"
    return float(mt.group(1))


def _theta(kernel, d, sigma, ls):
    if kernel == "sqexp":
        return np.array([sigma, ls[0], 0.5])
    return np.array([sigma] + list(ls[:d]) + [0.5])


def _case(name, n, m, d, kernel, seed, sigma=1.2, l=None, offset=0.0, X=None, U=None,
          routes=(1, 2), with_r=True, note=""):
    rng = np.random.default_rng(seed)
    if X is None:
        X = offset + rng.uniform(0.0, 10.0, size=(n, d))
    if U is None:
        U = offset + rng.uniform(0.0, 10.0, size=(m, d))
        k = (m + 1) // 2                       # half the knots are rows: coincidences occur
        idx = rng.choice(n, size=k, replace=False) if k <= n else rng.integers(0, n, size=k)
        U[rng.choice(m, size=k, replace=False)] = X[idx]
    s = math.sqrt(d)
    if l is not None:
        ls = np.full(d, float(l))
    elif kernel == "ard":
        ls = np.array([1.2 * s + 0.2 * c for c in range(d)])
    else:
        ls = np.full(d, 1.4 * s)
    r = rng.standard_normal(n)
    return {"name": name, "n": n, "m": m, "d": d, "kernel": kernel, "sigma": sigma, "ls": ls,
            "theta": _theta(kernel, d, sigma, ls), "X": np.asfortranarray(X),
            "U": np.asfortranarray(U), "r": r, "routes": routes, "with_r": with_r, "note": note}


def _tail_inputs(n=161):
    X = np.linspace(0.0, 10.0, n).reshape(n, 1)          # spacing 1/16: exact
    U = X[[0, 40, 80, 120, 160]].copy()                  # 0, 2.5, 5, 7.5, 10: all rows
    return X, U


def span2(c):
    """capi.hip's set_center: the bound on |x~|^2 the route guard reads (inf for NaN input)."""
    X, U, ls = c["X"], c["U"], c["ls"]
    if np.isnan(X).any() or np.isnan(U).any():
        return np.inf
    tot = 0.0
    for q in range(c["d"]):
        s = 0.0
        for v in U[:, q]:
            s += v
        ctr = s / c["m"]
        lo = min(U[:, q].min(), X[:, q].min())
        hi = max(U[:, q].max(), X[:, q].max())
        e = max(abs(lo - ctr), abs(hi - ctr)) * (1.0 / ls[q])
        tot += e * e
    return tot if tot == tot else np.inf


def expected_route(c):
    return 1 if span2(c) <= span2_max() else 2


def build_cases():
    C = []
    for m in (1, 127, 128, 129):
        C.append(_case(f"cols_m{m}", 65, m, 3, "sqexp", 100 + m))
    for n in (1, 63, 64, 65, 130):
        C.append(_case(f"rows_n{n}", n, 17, 3, "ard", 200 + n))
    # 6 row blocks, 2 column blocks: max_rows = 1 and 2 walk the persistent loop 6 and 3 times
    C.append(_case("persistent_n321_m129", 321, 129, 3, "sqexp", 321))
    for d in (1, 4, 8, 9, 16, 17, 32):
        for kernel in ("sqexp", "ard"):
            C.append(_case(f"nc_d{d}_{kernel}", 65, 33, d, kernel, 1000 + d))
    # the tail: exponents to -8 * 10^2 = -800: normal, subnormal and exactly 0 entries
    X, U = _tail_inputs()
    C.append(_case("tail_l025", 161, 5, 1, "sqexp", 7, l=0.25, X=X, U=U,
                   note="span^2 = (5 / 0.25)^2 = 400: the guard keeps the matrix-core route"))
    # the same with span^2 = 0.9 SGP_MFMA_SPAN2_MAX: the widest span the guard lets through
    l9 = 5.0 / math.sqrt(0.9 * span2_max())
    C.append(_case("tail_span09", 161, 5, 1, "sqexp", 7, l=l9, X=X, U=U))
    # and beyond the guard, where the product itself takes the direct-difference route
    C.append(_case("tail_span16", 161, 5, 1, "sqexp", 7, l=0.04, X=X, U=U))
    for sigma in (1e-150, 1.2, 1e150):
        C.append(_case(f"sigma_{sigma:g}", 65, 17, 3, "ard", 31, sigma=sigma))
    C.append(_case("offset_5e3", 65, 17, 3, "sqexp", 53, offset=5e3))
    return {c["name"]: c for c in C}


def nonfinite_case():
    """(case with a +inf and a NaN coordinate, the same with those two rows finite, rows)."""
    fin = _case("nonfinite", 65, 17, 3, "sqexp", 77, routes=(2,), with_r=False)
    # rows no knot was copied from
    free = [i for i in range(fin["n"])
            if not (fin["X"][i][None, :] == fin["U"]).all(axis=1).any()]
    i_inf, i_nan = free[3], free[-2]
    bad = dict(fin)
    bad["X"] = fin["X"].copy(order="F")
    bad["X"][i_inf, 1] = np.inf
    bad["X"][i_nan, 2] = np.nan
    return bad, fin, i_inf, i_nan


# ------------------------------------------------------------------------------- reference
def nc_of(d):
    return 2 if d <= 8 else (4 if d <= 16 else 8)


def reference(c):
    """K_ref (longdouble, n x m), e (the exponent), S (the matrix-core bound's magnitude)."""
    LD = np.longdouble
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is not extended precision on this platform"
    X, U, ls = c["X"].astype(LD), c["U"].astype(LD), c["ls"].astype(LD)
    n, m, d = c["n"], c["m"], c["d"]
    e = np.zeros((n, m), dtype=LD)
    for q in range(d):
        t = (X[:, q, None] - U[None, :, q]) / ls[q]
        e -= t * t / LD(2)
    sig2 = LD(c["sigma"]) * LD(c["sigma"])
    K = sig2 * np.exp(e)
    ctr = U.sum(axis=0) / LD(m)
    xt, ut = (X - ctr) / ls, (U - ctr) / ls
    S = ((xt * xt).sum(axis=1)[:, None] + (ut * ut).sum(axis=1)[None, :]) / LD(2) \
        + np.abs(xt @ ut.T) + abs(np.log(sig2))
    return K, e, S


def bars(c, ref):
    """route -> the bar on |K - K_ref| per entry (longdouble).

    sp = np.spacing of K_ref rounded to double (subnormal spacing where K_ref is subnormal).
    Direct differences (route 2): each squared difference carries at most 3 roundings (5 with
    ARD's scaling), the d positive terms add with one rounding each, exp has condition number |e|,
    then 2 ulp of its own and one rounding for the multiply by sigma^2:
        2^-52 (4 + (d + 6) |e_ij|) K_ref + 2 sp.
    Matrix cores (route 1): the standard bound of a dot product of length 4 NC + 4 over terms of
    total magnitude S_ij, with the roundings of x~ and u~ added, and doubled:
        2^-52 (4 + 2 (4 NC + 10) S_ij) K_ref + 2 sp.
    'promise': the header's |K - K_ref| <= 4 SGP_MFMA_SPAN2_MAX 2^-52 K_ref (8.9e-12), asserted
    wherever the guard itself chose the matrix cores; + 2 sp, since below the normal range no
    double -- the correctly rounded one included -- is within 8.9e-12 of K_ref."""
    LD = np.longdouble
    K, e, S = ref
    sp = np.spacing(np.abs(K.astype(np.float64))).astype(LD)
    d, nc = c["d"], nc_of(c["d"])
    return {2: LD(EPS) * (4 + (d + 6) * np.abs(e)) * K + 2 * sp,
            1: LD(EPS) * (4 + 2 * (4 * nc + 10) * S) * K + 2 * sp,
            "promise": LD(4 * span2_max() * EPS) * K + 2 * sp}


def numpy_direct(c):
    """The same K by direct differences in plain float64 numpy."""
    X, U, ls = c["X"], c["U"], c["ls"]
    e = np.zeros((c["n"], c["m"]))
    for q in range(c["d"]):
        t = (X[:, q, None] - U[None, :, q]) / ls[q]
        e -= 0.5 * t * t
    with np.errstate(under="ignore"):
        return (c["sigma"] * c["sigma"]) * np.exp(e)


def t_reference(c, ref, bar):
    """t_ref = K_ref^T r and its bar: sum_i |r_i| bar_ij + n 2^-52 sum_i |K_ij r_i|."""
    LD = np.longdouble
    K = ref[0]
    r = c["r"].astype(LD)
    t = (K * r[:, None]).sum(axis=0)
    tb = (np.abs(r)[:, None] * bar).sum(axis=0) \
        + c["n"] * LD(EPS) * np.abs(K * r[:, None]).sum(axis=0)
    return t, tb


# ------------------------------------------------------------------------------- the call
def run_build(lib, c, route=0, max_rows=0, shared_rb=0, with_r=False, device=0):
    """sgp_diag_build_knm -> (K padded n_pad x m_p, route taken, t (m_p) or None, t_rows)."""
    import ctypes as C

    from sparsergps_amd import _lib
    n, m, d = c["n"], c["m"], c["d"]
    npad, mp = (n + 127) // 128 * 128, (m + 127) // 128 * 128
    K = np.empty((npad, mp))
    t = np.full(mp, np.nan) if with_r else None
    taken, trows = C.c_int(0), C.c_int64(0)
    st = lib.sgp_diag_build_knm(device, _lib.KERNELS[c["kernel"]], d, _lib.dptr(c["theta"]),
                                _lib.dptr(c["X"]), n, n, _lib.dptr(c["U"]), m, m,
                                _lib.dptr(c["r"]) if with_r else None, route, max_rows, shared_rb,
                                _lib.dptr(K), _lib.dptr(t) if with_r else None, C.byref(taken),
                                C.byref(trows) if with_r else None)
    _lib.check(st)
    return K, taken.value, t, trows.value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)
