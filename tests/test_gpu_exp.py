"""The device exp functions every K12 entry goes through (sgp_internal.h), entry by entry against
mpmath.exp at 60 digits through sgp_diag_exp, which calls the very inline functions:

  which = 0  sgp_exp_nonpos(x): the direct-difference builder, the batched kernels, the scans
  which = 1  sgp_exp_tab(fmin(fmax(x, -746), hi)) with hi = log(DBL_MAX): the matrix-core builder

Error is |got - exact| / np.spacing(|correctly rounded|), so a subnormal result is measured in
subnormal spacing.  The bar is 2 ulp everywhere (tests/knm_cases.py: EXP_BAR_ULP): the header's
claim for sgp_exp_nonpos; for sgp_exp_tab 1/2 ulp for the rounded table entry, 1/2 for the final
fma(t, p, t), 1/2 for ldexp into the subnormal range and under 0.1 for the reduction and the
polynomial.  Points (tests/knm_cases.py: exp_bands): +-0 and -2^-1074 .. -2^-30; the doubles at and
+-1, +-2 ulp around the rint switch points -k ln2 and -(k + 1/2) ln2 (for the table form also
-j ln2/32 and -(j + 1/2) ln2/32, j = 0..64 and near 32 * 1022); the subnormal band every 1/64 and
the doubles around its two ends; below the band (exactly 0); NaN; 2000 points log-uniform in
[-745, -1e-8]; for the table form 200 points in (0, 709.78] and the 5 doubles below log(DBL_MAX).

Largest errors measured on an MI355X are in profiles/knm_direct/README.md.
"""
import numpy as np
import pytest

import knm_cases as KC

pytestmark = pytest.mark.gpu
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return _lib.lib()


def _run(lib, which, x, hi=KC.LOG_DBL_MAX):
    from sparsergps_amd import _lib
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.full(len(x), np.nan)
    _lib.check(lib.sgp_diag_exp(0, which, _lib.dptr(x), len(x), hi, _lib.dptr(out)))
    return out


def _results(lib, which):
    """band -> (x, got, ulp error): one launch and one mpmath pass per function, then shared."""
    if which not in _CACHE:
        bands = KC.exp_bands(which)
        x = np.concatenate(list(bands.values()))
        got = _run(lib, which, x)
        err = KC.exp_ulp_error(x, got)
        res, o = {}, 0
        for name, pts in bands.items():
            res[name] = (pts, got[o:o + len(pts)], err[o:o + len(pts)])
            o += len(pts)
        _CACHE[which] = res
    return _CACHE[which]


BANDS = [(0, b) for b in ("zero_and_tiny", "rint_switch", "subnormal_band", "below", "log_uniform")] \
    + [(1, b) for b in ("zero_and_tiny", "rint_switch", "table_switch", "subnormal_band", "below",
                        "log_uniform", "positive")]


@pytest.mark.parametrize("which,band", BANDS)
def test_exp_within_two_ulp(lib, which, band):
    x, got, err = _results(lib, which)[band]
    i = int(np.argmax(err))
    print(f"which={which} {band}: {len(x)} points, max {err[i]:.3f} ulp at x = {x[i]!r}")
    assert np.isfinite(got).all()
    assert err[i] <= KC.EXP_BAR_ULP, (which, band, x[i], got[i], err[i])


@pytest.mark.parametrize("which", [0, 1])
def test_exact_values(lib, which):
    res = _results(lib, which)
    assert sum(len(v[0]) for v in res.values()) >= 4000
    x, got, _ = res["zero_and_tiny"]
    assert x[0] == 0.0 and not np.signbit(x[0]) and x[1] == 0.0 and np.signbit(x[1])
    assert got[0] == 1.0 and got[1] == 1.0                       # exp(+-0) is exactly 1
    x, got, _ = res["below"]
    assert (got == 0.0).all() and not np.signbit(got).any(), got   # exactly +0 below the band
    x, got, _ = res["subnormal_band"]
    tiny = np.finfo(np.float64).tiny
    assert ((got > 0) & (got < tiny)).sum() > 2000               # the band is subnormal results
    assert (np.diff(got[:len(np.arange(-745.14, -708.39, 1.0 / 64))]) >= 0).all()   # monotone


def test_nan_in_nan_out(lib):
    got = _run(lib, 0, np.array([np.nan, -1.0, np.nan]))
    assert np.isnan(got[0]) and np.isnan(got[2]) and abs(got[1] - np.exp(-1.0)) < 1e-15


def test_table_form_clamps_at_hi(lib):
    """The builder passes hi = log sigma^2: nothing above exp(hi) comes out, NaN clamps away."""
    hi = np.log(1.44)
    got = _run(lib, 1, np.array([hi, 0.5, 700.0, np.inf]), hi=hi)
    assert (got == got[0]).all() and abs(got[0] - 1.44) <= 2 * np.spacing(1.44)
