"""sgp_fit_scan (the predictive variance / error scan of knot_prop_var and knot_prop_error,
k_scan.hip) on the GPU against the numpy oracle tests/oat_oracle.py.

Bars: mean and var within RTOL = 1e-8 normwise (tests/test_gpu_predict.py's _rel); the winning
row equal to the oracle's, after asserting that the oracle's own top-two relative gap is >= 1e-6
(fp64 rounding cannot swap the winner); cond(K22) <= 1e6 asserted per case, so the reference's own
forward error (~ cond * 2^-53 ~ 1e-10) stays two digits below the bar.

Shapes: n in {1, 63, 64, 65, 200} (one row, both sides of the 64-row step, four steps); m in
{1, 4, 15, 16, 17, 33, 50, 81, 97, 128} (every NT instantiation of the kernel -- 1, 2, 3, 4, 6,
8 column blocks -- and both sides of the 16-column padding edge); d in {1, 8, 9, 32}; m = 50
with d = 9 stages A in LDS, with d = 32 (and every m > 64) A is read through the caches.

Largest measured on an MI355X over the twelve shapes: mean 1.0e-11, var 6.8e-11 (both at
cond(K22) ~ 4e4-5e4; 3e-14 where cond < 1e3); every winner is the oracle's row.
"""
import functools

import numpy as np
import pytest

import ego_oracle as E
import oat_oracle as OO
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-8
COND_MAX = 1e6
DELTA = 1e-6

# (n, d, m, cov_fun, family, mode)
CASES = [(1, 1, 1, "sqexp", "gaussian", "var"),
         (63, 8, 4, "ard", "poisson", "error"),
         (64, 9, 15, "sqexp", "poisson", "var"),
         (65, 32, 16, "ard", "gaussian", "var"),
         (200, 1, 17, "sqexp", "gaussian", "error"),
         (200, 8, 33, "ard", "poisson", "var"),
         (200, 9, 50, "sqexp", "gaussian", "var"),
         (200, 32, 50, "ard", "poisson", "error"),
         (200, 32, 81, "sqexp", "poisson", "error"),
         (200, 8, 97, "ard", "gaussian", "var"),
         (200, 32, 128, "ard", "poisson", "var"),
         (200, 9, 128, "sqexp", "gaussian", "error")]


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _cond(P, cov_fun, family):
    s22 = O._pred_mats(P["xu"], P["X"][:1], cov_fun, P["cov_par"], DELTA, family == "gaussian")[1]
    return float(np.linalg.cond(s22))


@functools.lru_cache(maxsize=None)
def _case(n, d, m, cov_fun, family, mode, excl_knots=False):
    P = OO.scan_recipe(n, d, m, cov_fun)
    ref = OO.fit_scan(P["X"], P["mu"], P["cov_par"], cov_fun, P["xu"], P["u_mean"], P["u_var"],
                      P["muu"], mode, family, f=P["f"], excl=P["xu"] if excl_knots else None,
                      delta=DELTA)
    ref["cond"] = _cond(P, cov_fun, family)
    for a in (*[v for v in P.values() if isinstance(v, np.ndarray)],
              *[v for v in ref.values() if isinstance(v, np.ndarray)]):
        a.setflags(write=False)
    return P, ref


def _ctx(sgp, P, m_max=8):
    n = P["X"].shape[0]
    return sgp.SparseGPContext(P["X"], np.zeros(n), P["mu"], m_max=m_max)


def _scan(ctx, P, cov_fun, family, mode, excl=None, f="host", want=("key", "mean", "var")):
    return ctx.fit_scan(P["cov_par"], cov_fun, P["xu"], P["u_mean"], P["u_var"], P["muu"], mode,
                        family, f=P["f"] if (f == "host" and mode == "error") else None,
                        excl=excl, delta=DELTA, want=want)


def _check(ref, got, n, mode, tag="", winner=True):
    assert ref["cond"] <= COND_MAX, ref["cond"]
    e_mean, e_var = _rel(got["mean"], ref["mean"]), _rel(got["var"], ref["var"])
    gap = E.top_two_gap(ref["key"])
    print(f"{tag} n={n}: cond {ref['cond']:.3g}, mean rel {e_mean:.2e}, var rel {e_var:.2e}, "
          f"top-two gap {gap:.2e}, row {got['row']} (oracle {ref['row']})")
    assert gap >= 1e-6 or not winner, gap
    assert e_mean < RTOL and e_var < RTOL
    assert np.array_equal(np.isnan(got["key"]), ref["excluded"])
    on = ~ref["excluded"]
    # the key inherits the bar: var itself, or |d exp(mean)| <= exp(mean) |d mean|
    if mode == "error":
        kbar = RTOL * np.max(np.abs(ref["mean"])) * np.max(np.exp(ref["mean"])) * 1.0001
    else:
        kbar = RTOL * np.max(np.abs(ref["var"]))
    assert np.max(np.abs(got["key"][on] - ref["key"][on])) <= kbar
    assert got["row"] == ref["row"] or not winner
    assert got["key"][got["row"]] == got["key_best"]


@pytest.mark.parametrize("n,d,m,cov_fun,family,mode", CASES)
def test_scan_matches_oracle(sgp, n, d, m, cov_fun, family, mode):
    P, ref = _case(n, d, m, cov_fun, family, mode)
    with _ctx(sgp, P) as ctx:
        got = _scan(ctx, P, cov_fun, family, mode)
        bare = _scan(ctx, P, cov_fun, family, mode, want=())
        again = _scan(ctx, P, cov_fun, family, mode)
    assert set(bare) == {"row", "key"} and bare["row"] == got["row"]
    assert bare["key"] == got["key"][got["row"]]
    got["key_best"] = bare["key"]
    _check(ref, got, n, mode, f"d={d} m={m} {cov_fun} {family} {mode}")
    assert not np.isnan(got["key"]).any()          # excl = None: the knots' rows can win
    for k in ("key", "mean", "var"):               # bit-identical on repeat
        assert np.array_equal(got[k], again[k])
    assert again["row"] == got["row"]


@pytest.mark.parametrize("n,d,m,cov_fun,family,mode", [CASES[2], CASES[5], CASES[8]])
def test_excluded_knots_never_win(sgp, n, d, m, cov_fun, family, mode):
    P, ref = _case(n, d, m, cov_fun, family, mode, True)
    assert ref["excluded"][:m].all() and ref["excluded"].sum() == m
    with _ctx(sgp, P) as ctx:
        got = _scan(ctx, P, cov_fun, family, mode, excl=P["xu"])
        got["key_best"] = got["key"][got["row"]]
        _check(ref, got, n, mode, "excl = U")
        assert got["row"] >= m and np.isnan(got["key"][:m]).all()
        # the knot posterior's own rows excluded one by one: all rows gone is SGP_EINVAL
        with pytest.raises(sgp.SGPError) as ei:
            _scan(ctx, P, cov_fun, family, mode, excl=P["X"])
        assert ei.value.status == 1 and "every row is excluded" in str(ei.value)


def test_duplicated_rows_tie_and_the_lowest_wins(sgp):
    n, d, m, cov_fun, family, mode = CASES[5]
    P, ref = _case(n, d, m, cov_fun, family, mode)
    r = ref["row"]
    for where in ("after", "before"):
        Q = dict(P)
        if where == "after":
            idx = np.r_[np.arange(n), r]
            first, second = r, n
        else:
            idx = np.r_[r, np.arange(n)]
            first, second = 0, r + 1
        Q["X"], Q["mu"], Q["f"] = P["X"][idx], P["mu"][idx], P["f"][idx]
        with _ctx(sgp, Q) as ctx:
            got = _scan(ctx, Q, cov_fun, family, mode)
        assert got["key"][first] == got["key"][second]       # bit for bit
        assert got["mean"][first] == got["mean"][second]
        assert got["row"] == first


def test_more_steps_than_workgroups(sgp):
    """131109 rows = 2049 64-row steps: one more than the scan launches workgroups on an MI355X
    (eight per compute unit, 2048), so some workgroup takes a second step."""
    n, d, m = 64 * 2048 + 37, 2, 5
    P, ref = _case(n, d, m, "sqexp", "poisson", "var")
    with _ctx(sgp, P) as ctx:
        got = _scan(ctx, P, "sqexp", "poisson", "var")
    got["key_best"] = got["key"][got["row"]]
    _check(ref, got, n, "var", "grid-stride")


def test_error_mode_reads_the_resident_laplace_mode(sgp):
    Pp = O.make_poisson_problem(n=300, m=6)
    X, y, mu, xu = Pp["X"], Pp["y"], Pp["mu"], Pp["U"]
    n, m = X.shape[0], xu.shape[0]
    muu = np.full(m, float(np.mean(mu)))
    from sparsergps_amd.covariance import theta_vector
    with sgp.SparseGPContext(X, y, mu, m_max=8) as ctx:
        with pytest.raises(sgp.SGPError) as ei:       # no Laplace evaluation has run yet
            ctx.fit_scan(Pp["cov_par"], Pp["cov_fun"], xu, np.zeros(m), np.eye(m), muu, "error",
                         "poisson")
        assert ei.value.status == 1 and "Laplace" in str(ei.value)
        theta = theta_vector(Pp["cov_par"], Pp["cov_fun"], X.shape[1], None)
        ctx.lap_set_f(None, 0.0)
        ctx.eval_laplace(theta, Pp["cov_fun"], xu, delta=Pp["delta"])
        um, uv = ctx.posterior_u(muu)
        f = ctx.lap_get_f()
        got = ctx.fit_scan(Pp["cov_par"], Pp["cov_fun"], xu, um, uv, muu, "error", "poisson",
                           delta=Pp["delta"], want=("key", "mean", "var"))
        host = ctx.fit_scan(Pp["cov_par"], Pp["cov_fun"], xu, um, uv, muu, "error", "poisson",
                            f=f, delta=Pp["delta"], want=("key",))
        um2, uv2 = ctx.posterior_u(muu)
    ref = OO.fit_scan(X, np.broadcast_to(mu, (n,)), Pp["cov_par"], Pp["cov_fun"], xu, um, uv, muu,
                      "error", "poisson", f=f, delta=Pp["delta"])
    ref["cond"] = 1.0
    got["key_best"] = got["key"][got["row"]]
    _check(ref, got, n, "error", "resident f")
    assert np.array_equal(host["key"], got["key"]) and host["row"] == got["row"]
    # a completed evaluation is left as it was: the knot posterior answers bit for bit
    assert np.array_equal(um, um2) and np.array_equal(uv, uv2)


def test_posterior_u_is_untouched_by_a_scan(sgp):
    G = O.make_gaussian_problem("C2", n=260, m=7)
    muu = np.full(7, float(np.mean(G["mu"])))
    from sparsergps_amd.covariance import theta_vector
    theta = theta_vector(G["cov_par"], G["cov_fun"], G["X"].shape[1], None, need_tau=True)
    with sgp.SparseGPContext(G["X"], G["y"], G["mu"], m_max=8) as ctx:
        ctx.eval_vi(theta, G["cov_fun"], G["U"], delta=G["delta"])
        um, uv = ctx.posterior_u(muu)
        got = ctx.fit_scan(G["cov_par"], G["cov_fun"], G["U"], um, uv, muu, "var", "gaussian",
                           delta=G["delta"], want=("key", "mean", "var"))
        um2, uv2 = ctx.posterior_u(muu)
    assert np.array_equal(um, um2) and np.array_equal(uv, uv2)
    ref = OO.fit_scan(G["X"], np.broadcast_to(G["mu"], (260,)), G["cov_par"], G["cov_fun"], G["U"],
                      um, uv, muu, "var", "gaussian", delta=G["delta"])
    ref["cond"] = 1.0
    got["key_best"] = got["key"][got["row"]]
    # (rows far from every knot all have var = sigma^2 + tau^2 to the last bit: this case pins
    # the knot posterior, the mean and the variance; the winner is the other tests' subject)
    _check(ref, got, 260, "var", "after eval_vi", winner=False)


def test_singular_k22_is_notpd_and_the_next_scan_is_right(sgp):
    n, d, m, cov_fun, family, mode = CASES[2]
    P, ref = _case(n, d, m, cov_fun, family, mode)
    # two identical knots, tau = 0, delta = 0, gaussian Sigma22: with sigma = 3 the first pivot is
    # exactly 9, its factor exactly 3 and the second pivot exactly 0
    xu = np.vstack([P["xu"][:1], P["xu"]])
    with _ctx(sgp, P) as ctx:
        with pytest.raises(sgp.NotPositiveDefinite) as enp:
            ctx.fit_scan({"sigma": 3.0, "l": 1.5, "tau": 0.0}, "sqexp", xu, np.zeros(m + 1),
                         np.eye(m + 1), np.zeros(m + 1), "var", "gaussian", delta=0.0)
        assert "scan K22" in str(enp.value)
        got = _scan(ctx, P, cov_fun, family, mode)          # the chain's sync words were reset
    got["key_best"] = got["key"][got["row"]]
    _check(ref, got, n, mode, "after ENOTPD")


def test_129_knots_take_the_predict_route(sgp):
    n, d, m = 200, 8, 129
    P, ref = _case(n, d, m, "sqexp", "poisson", "var")
    with _ctx(sgp, P) as ctx:
        got = _scan(ctx, P, "sqexp", "poisson", "var")
        from sparsergps_amd import _lib
        import ctypes as C
        row, key = C.c_int64(-1), C.c_double(0.0)
        th = np.array([1.3, 1.0, 0.4])
        U = np.asfortranarray(P["xu"])
        uv = np.asfortranarray(P["u_var"])
        st = _lib.lib().sgp_fit_scan(ctx.handle, 0, _lib.dptr(th), DELTA, 0, _lib.dptr(U), m, m,
                                     _lib.dptr(np.ascontiguousarray(P["u_mean"])),
                                     _lib.dptr(np.ascontiguousarray(P["muu"])), _lib.dptr(uv), m,
                                     0, None, None, 0, 0, C.byref(row), C.byref(key), None, None,
                                     None)
        assert st == _lib.SGP_EINVAL and b"m=129" in _lib.lib().sgp_last_error()
    got["key_best"] = got["key"][got["row"]]
    _check(ref, got, n, "var", "m = 129")
