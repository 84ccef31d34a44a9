"""The two K12 builders (k_cov.hip: the matrix-core k_build_knm_mfma<WITH_T, NC> and the
direct-difference k_build_knm), entry by entry through sgp_diag_build_knm against
K_ij = sigma^2 exp(-1/2 sum_c ((x_ic - u_jc) / l_c)^2) computed from the double inputs in
np.longdouble (tests/knm_cases.py, where the two derived bars are written out).

Every case, on each route it names (1 the matrix cores, 2 direct differences):
  * |K - K_ref| <= the route's bar, per entry; where the guard itself chose the matrix cores also
    the header's promise 4 SGP_MFMA_SPAN2_MAX 2^-52 K_ref (+ 2 spacings: below the normal range
    no double is that close);
  * rows >= n and columns >= m of the padded matrix are +0.0 bit for bit;
  * K <= sigma^2 (1 + 2 2^-52); on the direct-difference route a row that equals its knot gives
    exactly sigma^2;
  * the guard's route is the one tests/knm_cases.py's twin of set_center expects;
  * K is the same bits for max_rows in {0, 1, 2} x shared_rb in {0, 1, -1}, with and without the
    fused t = K^T r (max_rows = 1 makes one workgroup row walk every 64-row block: the persistent
    loop's prefetch and the carry of t's sums in LDS, at a size where an error shows per entry);
  * t is within sum_i |r_i| bar_ij + n 2^-52 sum_i |K_ij r_i| on every grid, +0.0 in columns >= m,
    and the same bits on a repeat.

Cases: knot columns m in {1, 127, 128, 129} at n = 65; rows n in {1, 63, 64, 65, 130} at m = 17;
the persistent loop n = 321, m = 129 (6 row blocks, 2 column blocks); the NC boundaries d in
{1, 4, 8, 9, 16, 17, 32} x {sqexp, ard} at n = 65, m = 33; the tail (d = 1, l = 0.25, a grid on
[0, 10], m = 5: exponents to -800) and two copies at span^2 = 0.9 and 1.56 SGP_MFMA_SPAN2_MAX;
sigma in {1e-150, 1.2, 1e150}; X = 5e3 + [0, 10]^3; one +inf and one NaN row.  Data uniform on
[0, 10]^d, length scales ~ sqrt(d), half the knots copied from rows.

The tail at l = 0.25 has span^2 = (5 / 0.25)^2 = 400, inside the guard, so the product builds it
on the matrix cores (in d = 1 on [0, 10] the guard is passed only once the exponents reach
-20000): that case asserts the matrix-core route, tail_span16 the direct-difference one.

Largest ratios of error to bar measured on an MI355X are in profiles/knm_direct/README.md.
"""
import itertools

import numpy as np
import pytest

import knm_cases as KC

pytestmark = pytest.mark.gpu
CASES = KC.build_cases()
GRIDS = list(itertools.product((0, 1, 2), (0, 1, -1)))     # (max_rows, shared_rb)


@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return _lib.lib()


def _check_matrix(c, route, K, ref, bar, what):
    n, m = c["n"], c["m"]
    Kref = ref[0]
    pad = np.ones(K.shape, dtype=bool)
    pad[:n, :m] = False
    assert (KC.bits(K)[pad] == 0).all(), (what, "padding is not +0.0",
                                          np.argwhere(pad & (KC.bits(K) != 0))[:4])
    got = K[:n, :m]
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.longdouble) - Kref)
    ratio = err / bar
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{what}: max err / bar = {float(ratio[i, j]):.3f} at ({i}, {j}): got {got[i, j]!r}, "
          f"ref {float(Kref[i, j])!r}")
    assert (err <= bar).all(), (what, (i, j), got[i, j], float(Kref[i, j]), float(ratio[i, j]))
    sig2 = c["sigma"] * c["sigma"]
    assert (got <= sig2 * (1 + 2 * KC.EPS)).all(), (what, got.max(), sig2)
    if route == 2:
        same = (c["X"][:, None, :] == c["U"][None, :, :]).all(axis=2)
        assert same.any() and (got[same] == sig2).all(), (what, got[same], sig2)
    return float(ratio[i, j])


def _check_t(c, t, tref, tbar, what):
    m = c["m"]
    assert (KC.bits(t)[m:] == 0).all(), (what, "t padding is not +0.0")
    err = np.abs(t[:m].astype(np.longdouble) - tref)
    assert (err <= tbar).all(), (what, int(np.argmax(err / tbar)), float((err / tbar).max()))
    return float((err / tbar).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_build_knm(lib, name):
    c = CASES[name]
    ref = KC.reference(c)
    bar = KC.bars(c, ref)
    want = KC.expected_route(c)
    K0, taken, _, _ = KC.run_build(lib, c, route=0)
    assert taken == want, (name, taken, want, KC.span2(c))
    if taken == 1:
        _check_matrix(c, 1, K0, ref, bar["promise"], f"{name} guard's route, header's promise")
    for route in c["routes"]:
        what = f"{name} route {route}"
        K, tk, _, _ = KC.run_build(lib, c, route=route)
        assert tk == route
        if route == taken:
            assert (KC.bits(K) == KC.bits(K0)).all(), what      # forcing the guard's route: same K
        _check_matrix(c, route, K, ref, bar[route], what)
        tref, tbar = KC.t_reference(c, ref, bar[route])
        worst_t = 0.0
        for (max_rows, shared_rb), with_r in itertools.product(GRIDS, (False, True)):
            if (max_rows, shared_rb, with_r) == (0, 0, False):
                continue
            Kg, _, t, trows = KC.run_build(lib, c, route=route, max_rows=max_rows,
                                           shared_rb=shared_rb, with_r=with_r)
            g = f"{what} max_rows={max_rows} shared_rb={shared_rb} r={with_r}"
            diff = KC.bits(Kg) != KC.bits(K)
            assert not diff.any(), (g, np.argwhere(diff)[:4], Kg[diff][:4], K[diff][:4])
            if with_r:
                assert trows >= 1
                worst_t = max(worst_t, _check_t(c, t, tref, tbar, g))
        _, _, t1, _ = KC.run_build(lib, c, route=route, max_rows=2, shared_rb=1, with_r=True)
        _, _, t2, _ = KC.run_build(lib, c, route=route, max_rows=2, shared_rb=1, with_r=True)
        assert (KC.bits(t1) == KC.bits(t2)).all(), what
        print(f"{what}: t max err / bar = {worst_t:.3f}")


def test_tail_counts(lib):
    """The span^2 = 0.9 SGP_MFMA_SPAN2_MAX copy of the tail reaches the subnormal range and 0 on
    the matrix cores; the l = 0.25 tail holds normal, subnormal and zero entries."""
    tiny = np.finfo(np.float64).tiny
    c = CASES["tail_span09"]
    Kref = KC.reference(c)[0].astype(np.float64)
    assert int((Kref < tiny).sum()) >= 50
    K, taken, _, _ = KC.run_build(lib, c, route=0)
    assert taken == 1
    got = K[:c["n"], :c["m"]]
    assert int((got < tiny).sum()) >= 50 and (got == 0).any() and (got >= tiny).any()
    c = CASES["tail_l025"]
    K = KC.run_build(lib, c, route=0)[0][:c["n"], :c["m"]]
    assert (K == 0).any() and ((K > 0) & (K < tiny)).any() and (K >= tiny).any()


def test_nonfinite_rows(lib):
    """A +inf coordinate gives a row of +0.0, a NaN coordinate a row of NaN, on the
    direct-difference route (the guard's span is then not finite; the matrix-core builder's clamp
    would turn the NaN into 0); every other row is the same bits as with those two rows finite."""
    bad, fin, i_inf, i_nan = KC.nonfinite_case()
    n, m = bad["n"], bad["m"]
    Kb, taken, _, _ = KC.run_build(lib, bad, route=0)
    assert taken == 2
    Kf, tf, _, _ = KC.run_build(lib, fin, route=2)      # the same builder on the finite rows
    assert tf == 2 and KC.run_build(lib, fin, route=0)[1] == 1
    assert (KC.bits(Kb[i_inf]) == 0).all(), Kb[i_inf, :m]
    assert np.isnan(Kb[i_nan, :m]).all(), Kb[i_nan, :m]
    assert (KC.bits(Kb[i_nan, m:]) == 0).all() and (KC.bits(Kb[n:]) == 0).all()
    rest = np.ones(Kb.shape[0], dtype=bool)
    rest[[i_inf, i_nan]] = False
    assert (KC.bits(Kb[rest]) == KC.bits(Kf[rest])).all()
    # a NaN in the first row too (the column ranges start from it)
    first = dict(bad)
    first["X"] = fin["X"].copy(order="F")
    first["X"][0, 0] = np.nan
    K1, taken, _, _ = KC.run_build(lib, first, route=0)
    assert taken == 2 and np.isnan(K1[0, :m]).all()
    assert (KC.bits(K1[1:]) == KC.bits(Kf[1:])).all()
