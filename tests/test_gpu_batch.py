"""The batched small-knot VI path on the GPU (SparseGPBatch, norm_grad_ascent_vi_batch,
optimize_gp_batch) against the CPU oracle, at the project's bars: 1e-6
relative on the objective, |d| / max(1, |ref|) < 1e-6 per gradient entry, rtol 1e-6 / atol 1e-9
for trajectories and 1e-7 for u_mean / u_var; independence of the batch bit for bit."""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest

from oracle import drivers as OD
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
EVAL_RTOL = 1e-6
SEG = 512   # SGP_BATCH_SEG_ROWS (tests/test_batch_abi.py reads it from the header)


@functools.lru_cache(maxsize=None)
def _gauss(n, m, d, cov_fun, seed):
    """The recipe of tests/test_gpu_edges.py::_gauss."""
    g = np.random.Generator(np.random.PCG64(seed))
    X = g.uniform(0.0, 10.0, size=(n, d))
    U = g.uniform(0.0, 10.0, size=(m, d))
    y = np.sin(X).sum(axis=1) / math.sqrt(d) + g.normal(0.0, 0.5, size=n)
    l0 = 1.7
    if d == 1:
        U = np.linspace(0.1, 9.9, m)[:, None]
        l0 = 0.5
    if cov_fun == "ard":
        cp = OrderedDict([("sigma", 1.2)] + [(f"l{c + 1}", l0 + 0.25 * c) for c in range(d)]
                         + [("tau", 0.5)])
    else:
        cp = OrderedDict([("sigma", 1.2), ("l", l0), ("tau", 0.5)])
    return dict(X=X, U=U, y=y, mu=np.full(n, y.mean()), cov_par=cp, cov_fun=cov_fun, delta=1e-6)


@functools.lru_cache(maxsize=None)
def _gauss_hd(n, m, d, cov_fun, seed):
    """tests/test_gpu_edges.py::_gauss_hd: length scales ~ sqrt(d)."""
    P = dict(_gauss(n, m, d, cov_fun, seed))
    s = math.sqrt(d)
    if cov_fun == "ard":
        P["cov_par"] = OrderedDict([("sigma", 1.2)] + [(f"l{c + 1}", 1.2 * s + 0.2 * c)
                                                        for c in range(d)] + [("tau", 0.5)])
    else:
        P["cov_par"] = OrderedDict([("sigma", 1.2), ("l", 1.4 * s), ("tau", 0.5)])
    return P


_REF = {}


def _ref(P, U=None, cp=None, delta=None):
    """(objective, gradient) of the oracle, computed once per problem."""
    U = P["U"] if U is None else U
    cp = P["cov_par"] if cp is None else cp
    delta = P["delta"] if delta is None else delta
    key = (id(P["X"]), U.tobytes(), tuple(cp.items()), delta)
    if key not in _REF:
        o = O.elbo_eval(cp, P["cov_fun"], U, P["X"], P["y"], P["mu"], delta)
        g = O.delbo_dcov_par(cp, P["cov_fun"], U, P["X"], P["y"], P["mu"], delta)["gradient"]
        _REF[key] = (o, g)
    return _REF[key]


def _close(obj, grad, o_ref, g_ref, what=""):
    print(what, "obj rel", abs(obj - o_ref) / abs(o_ref), "grad",
          max(abs(grad[k] - g_ref[k]) / max(1.0, abs(g_ref[k])) for k in g_ref))
    assert abs(obj - o_ref) / abs(o_ref) < EVAL_RTOL, (what, obj, o_ref)
    for k in g_ref:
        assert abs(grad[k] - g_ref[k]) / max(1.0, abs(g_ref[k])) < EVAL_RTOL, \
            (what, k, grad[k], g_ref[k])


def _batch(Ps):
    import sparsergps_amd as S
    return S.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"]) for P in Ps])


def _eval(Ps, Us=None, **kw):
    with _batch(Ps) as b:
        return b.eval_vi([P["cov_par"] for P in Ps], Ps[0]["cov_fun"],
                         [P["U"] for P in Ps] if Us is None else Us, Ps[0]["delta"], **kw)


# (n, m, d, cov_fun): n < one step, n < m, n off the 16 / 64 grid, m on and off a 16-block and at
# the limit, d past the 8-coordinate chunk and at 32, problems longer than one segment
MIXED = [(1, 1, 1, "sqexp"), (65, 1, 1, "sqexp"), (5, 7, 2, "sqexp"), (63, 17, 3, "sqexp"),
         (64, 16, 3, "ard"), (129, 64, 8, "ard"), (1000, 64, 3, "sqexp"),
         (300, 33, 9, "ard"), (300, 20, 32, "ard"), (2 * SEG + 37, 30, 3, "sqexp")]


def _mixed():
    out = []
    for i, (n, m, d, cf) in enumerate(MIXED):
        make = _gauss_hd if d > 8 else _gauss
        out.append(make(n, m, d, cf, 500 + i))
    return out


def _groups():
    groups = OrderedDict()
    for P in _mixed():
        groups.setdefault((P["X"].shape[1], P["cov_fun"]), []).append(P)
    return groups


@pytest.mark.parametrize("key", list(_groups()))
def test_parity_in_one_mixed_batch(key):
    Ps = _groups()[key]
    obj, grad, status = _eval(Ps)
    assert (status == 0).all()
    for b, P in enumerate(Ps):
        o, g = _ref(P)
        assert list(grad[b]) == list(P["cov_par"])
        _close(obj[b], grad[b], o, g, (P["X"].shape, P["U"].shape))
    if key == (3, "sqexp"):     # sizes differ inside the one call
        assert sorted(P["X"].shape[0] for P in Ps) == [63, 1000, 2 * SEG + 37]
        assert max(abs(v) for v in _ref(Ps[1])[1].values()) > 1.0


@pytest.mark.parametrize("n,m,d,cov_fun,seed", [(200, 16, 3, "sqexp", 520), (257, 48, 5, "ard", 521)])
def test_coincident_knots(n, m, d, cov_fun, seed):
    """Quirk Q5: knots that equal data rows exactly enter the tau derivative."""
    P = _gauss(n, m, d, cov_fun, seed)
    Q = _gauss(150, 20, d, cov_fun, seed + 10)
    U = P["X"][:m].copy()
    obj, grad, status = _eval([Q, P], [Q["U"], U])
    assert (status == 0).all()
    o, g = _ref(P, U)
    _close(obj[1], grad[1], o, g, "coincident")
    _close(obj[0], grad[0], *_ref(Q), "beside it")
    assert abs(grad[1]["tau"] - g["tau"]) / max(1.0, abs(g["tau"])) < EVAL_RTOL


EIGHT = [(40, 5, 700), (700, 33, 701), (64, 16, 702), (513, 64, 703), (129, 17, 704),
         (1100, 48, 705), (16, 20, 706), (300, 1, 707)]


def _raw(b, Ps, order, active=None, sentinel=-123.25, flags=0):
    P_ = 3
    B = len(order)
    theta = np.array([[Ps[i]["cov_par"][k] for k in ("sigma", "l", "tau")] for i in order])
    obj = np.full(B, sentinel)
    grad = np.full((B, P_), sentinel)
    status = np.full(B, 99, dtype=np.int32)
    b.eval_raw("sqexp", theta, [Ps[i]["U"] for i in order], 1e-6, flags, active, obj, grad, status)
    return obj, grad, status


def test_independence_bit_for_bit():
    Ps = [_gauss(n, m, 3, "sqexp", seed) for n, m, seed in EIGHT]
    order = list(range(8))
    muus = [np.zeros(P["U"].shape[0]) for P in Ps]
    with _batch(Ps) as b:
        obj, grad, status = _raw(b, Ps, order)
        um, uv = b.posterior_u(muus)
        obj2, grad2, status2 = _raw(b, Ps, order)                    # the same call repeated
        um2, uv2 = b.posterior_u(muus)
    assert (status == 0).all() and (status2 == 0).all()
    assert np.array_equal(obj, obj2) and np.array_equal(grad, grad2)
    for i in order:
        assert np.array_equal(um[i], um2[i]) and np.array_equal(uv[i], uv2[i])
    for i in order:                                                  # each problem alone
        with _batch([Ps[i]]) as b:
            o1, g1, s1 = _raw(b, Ps, [i])
            m1, v1 = b.posterior_u([muus[i]])
        assert s1[0] == 0 and np.array_equal(o1[0], obj[i]) and np.array_equal(g1[0], grad[i]), i
        assert np.array_equal(m1[0], um[i]) and np.array_equal(v1[0], uv[i]), i
    rev = order[::-1]                                                # the batch in reverse order
    with _batch([Ps[i] for i in rev]) as b:
        o3, g3, s3 = _raw(b, Ps, rev)
        m3, v3 = b.posterior_u([muus[i] for i in rev])
    assert np.array_equal(o3[::-1], obj) and np.array_equal(g3[::-1], grad)
    for k, i in enumerate(rev):
        assert np.array_equal(m3[k], um[i]) and np.array_equal(v3[k], uv[i])
    act = np.array([1, 0] * 4, dtype=np.uint8)                       # every other one inactive
    with _batch(Ps) as b:
        o4, g4, s4 = _raw(b, Ps, order, active=act)
        m4, v4 = b.posterior_u(muus)
    for i in order:
        if act[i]:
            assert s4[i] == 0 and np.array_equal(o4[i], obj[i]) and np.array_equal(g4[i], grad[i])
            assert np.array_equal(m4[i], um[i]) and np.array_equal(v4[i], uv[i])
        else:                                   # the sentinel stands, and there is no posterior
            assert o4[i] == -123.25 and (g4[i] == -123.25).all() and s4[i] == 99
            assert m4[i] is None and v4[i] is None
    for i in (1, 3):                            # ... and all of it is the right answer
        _close(obj[i], dict(zip(("sigma", "l", "tau"), grad[i])), *_ref(Ps[i]), i)


def test_aliased_rows():
    """Four problems on one row range (a multi-start): four thetas and knot sets."""
    import sparsergps_amd as S
    P = _gauss(600, 24, 3, "sqexp", 530)
    g = np.random.Generator(np.random.PCG64(531))
    cps = [OrderedDict([("sigma", 1.2 - 0.1 * k), ("l", 1.7 + 0.3 * k), ("tau", 0.5 + 0.05 * k)])
           for k in range(4)]
    Us = [g.uniform(0.0, 10.0, size=(m, 3)) for m in (24, 7, 40, 16)]
    with S.SparseGPBatch(P["X"], P["y"], P["mu"], [0] * 4, [600] * 4) as b:
        obj, grad, status = b.eval_vi(cps, "sqexp", Us, 1e-6)
    assert (status == 0).all()
    for k in range(4):
        _close(obj[k], grad[k], *_ref(P, Us[k], cps[k]), k)
        with S.SparseGPBatch(P["X"], P["y"], P["mu"]) as b1:
            o1, g1, _ = b1.eval_vi([cps[k]], "sqexp", [Us[k]], 1e-6)
        assert np.array_equal(o1[0], obj[k]) and list(g1[0].values()) == list(grad[k].values())


def test_flags():
    from sparsergps_amd import _lib
    Ps = [_gauss(n, m, 3, "sqexp", seed) for n, m, seed in EIGHT[:4]]
    order = list(range(4))
    with _batch(Ps) as b:
        obj, grad, status = _raw(b, Ps, order)
        o2, g2, s2 = _raw(b, Ps, order, flags=_lib.SGP_FLAG_OBJ_ONLY)
        o3, g3, s3 = _raw(b, Ps, order, flags=_lib.SGP_FLAG_R_DET)
        o4, _, s4 = b.eval_vi([P["cov_par"] for P in Ps], "sqexp", [P["U"] for P in Ps], 1e-6,
                              obj_only=True)
    assert np.array_equal(o2, obj) and (g2 == -123.25).all() and (s2 == 0).all()   # grad untouched
    assert np.array_equal(o4, obj) and (s4 == 0).all()
    for i, P in enumerate(Ps):
        s22 = O.vi_mats(P["cov_par"], "sqexp", P["U"], P["X"], 1e-6)[1]
        assert abs(np.linalg.slogdet(s22)[1]) < 700
    np.testing.assert_allclose(o3, obj, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(g3, grad, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("m,dup,order", [(40, 25, 26), (64, 63, 64), (17, 16, 17)])
def test_one_bad_problem(m, dup, order):
    """A duplicated knot with a negative jitter (tests/test_gpu_edges.py::
    test_not_positive_definite_order at small m): the bad problem reports chol()'s leading-minor
    order and NaN, its neighbours in the same call are unaffected, and the batch recovers."""
    d = 3
    g = np.random.Generator(np.random.PCG64(77))
    U = g.uniform(0.0, 10.0, size=(m, d))
    U[dup] = U[3]
    X = g.uniform(0.0, 10.0, size=(300, d))
    y = np.sin(X).sum(axis=1) + g.normal(0.0, 0.5, size=300)
    cp = OrderedDict([("sigma", 1.0), ("l", 0.3), ("tau", 0.5)])
    delta = -1e-3
    bad = dict(X=X, U=U, y=y, mu=np.full(300, y.mean()), cov_par=cp, cov_fun="sqexp", delta=delta)
    good = [dict(bad, U=g.uniform(0.0, 10.0, size=(k, d))) for k in (m, 12)]
    Ps = [good[0], bad, good[1]]
    with _batch(Ps) as b:
        obj, grad, status = b.eval_vi([cp] * 3, "sqexp", [P["U"] for P in Ps], delta)
        assert list(status) == [0, order, 0]
        assert b"problem 1" in b._lib.sgp_last_error() and b"Sigma22" in b._lib.sgp_last_error()
        assert np.isnan(obj[1]) and all(np.isnan(v) for v in grad[1].values())
        for i in (0, 2):
            _close(obj[i], grad[i], *_ref(Ps[i], delta=delta), i)
        # a valid evaluation of the whole batch right afterwards succeeds
        Us = [good[0]["U"], good[0]["U"], good[1]["U"]]
        obj2, grad2, status2 = b.eval_vi([cp] * 3, "sqexp", Us, delta)
        assert (status2 == 0).all() and np.isfinite(obj2).all()
        assert np.array_equal(obj2[0], obj[0]) and np.array_equal(obj2[1], obj2[0])


def test_posterior():
    Ps = _groups()[(3, "sqexp")] + [_gauss(200, 16, 3, "sqexp", 520)]
    muus = [np.full(P["U"].shape[0], 0.1 * (i + 1)) for i, P in enumerate(Ps)]
    with _batch(Ps) as b:
        _, _, status = b.eval_vi([P["cov_par"] for P in Ps], "sqexp", [P["U"] for P in Ps], 1e-6)
        um, uv = b.posterior_u(muus)
    assert (status == 0).all()
    for i, P in enumerate(Ps):
        m_ref, v_ref = O.vi_posterior_u(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["mu"],
                                        muus[i], 1e-6)
        np.testing.assert_allclose(um[i], m_ref, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(uv[i], v_ref, rtol=1e-6, atol=1e-7)


ASCENT = [(90, 6), (200, 12), (333, 20), (150, 33)]


@functools.lru_cache(maxsize=None)
def _ascent_ref(opt_items):
    opt = dict(opt_items)
    out = []
    for i, (n, m) in enumerate(ASCENT):
        P = _gauss(n, m, 3, "sqexp", 700 + i)
        out.append(OD.norm_grad_ascent_vi(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["mu"],
                                          opt=opt))
    return out


def _same_fit(r, ref):
    assert r["iter"] == ref["iter"]
    for key in ("obj_fun", "grad", "cov_par_history"):
        np.testing.assert_allclose(r[key], np.asarray(ref[key]), rtol=1e-6, atol=1e-9, err_msg=key)
    np.testing.assert_allclose(list(r["cov_par"].values()), list(ref["cov_par"].values()),
                               rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(r["u_mean"], ref["u_mean"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(r["u_var"], ref["u_var"], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("opt,iters", [
    ({"maxit": 5, "obj_tol": 0.0}, [5, 5, 5, 5]),
    ({"maxit": 30, "obj_tol": 2.5}, [23, 30, 30, 30]),
    # "ga" steps log theta by learn_rate x gradient; the gradients here reach 1e3, so the default
    # 1e-2 would leave the parameters' range in one step
    ({"maxit": 5, "obj_tol": 0.0, "optim_method": "ga", "learn_rate": 1e-4}, [5, 5, 5, 5])])
def test_lockstep_ascent(opt, iters):
    import sparsergps_amd as S
    Ps = [_gauss(n, m, 3, "sqexp", 700 + i) for i, (n, m) in enumerate(ASCENT)]
    ref = _ascent_ref(tuple(sorted(opt.items())))
    assert [r["iter"] for r in ref] == iters
    res = S.norm_grad_ascent_vi_batch([P["cov_par"] for P in Ps], "sqexp", [P["U"] for P in Ps],
                                      [(P["X"], P["y"], P["mu"]) for P in Ps], opt=opt)
    assert [r["iter"] for r in res] == iters
    for r, rf in zip(res, ref):        # problem 0's results are those of its own last iteration
        _same_fit(r, rf)
        assert "error" not in r


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif isinstance(a, str) or a is None:
        assert a == b, path
    else:
        np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64),
                                   rtol=1e-6, atol=1e-7, err_msg=path)


def test_end_to_end():
    import sparsergps_amd as S
    Ps = [_gauss(n, m, 3, "sqexp", 700 + i) for i, (n, m) in enumerate(ASCENT[:3])]
    opt = {"maxit": 5}
    mods = S.optimize_gp_batch([(P["X"], P["y"], P["mu"]) for P in Ps], "sqexp", Ps[0]["cov_par"],
                               [P["U"] for P in Ps], opt=opt)
    g = np.random.Generator(np.random.PCG64(799))
    xt = g.uniform(0.0, 10.0, size=(50, 3))
    yt = np.sin(xt).sum(axis=1) / math.sqrt(3)
    for P, mod in zip(Ps, mods):
        one = S.optimize_gp(P["y"], P["X"], "sqexp", Ps[0]["cov_par"], P["mu"], sparse=True,
                            xu_opt="fixed", xu=P["U"], vi=True, opt=opt)
        assert set(mod) == set(one) and mod["sparse"] is True and mod["family"] == "gaussian"
        assert mod["results"]["iter"] == one["results"]["iter"] == 5
        for key in ("obj_fun", "grad", "cov_par_history", "u_mean", "u_var", "muu"):
            np.testing.assert_allclose(mod["results"][key], one["results"][key], rtol=1e-6,
                                       atol=1e-7, err_msg=key)
        _same(S.predict_gp(mod, xt, vi=True), S.predict_gp(one, xt, vi=True), "predict_gp")
        sa, sb = S.score_gp(mod, xt, yt, vi=True), S.score_gp(one, xt, yt, vi=True)
        _same(sa, sb, "score_gp")
