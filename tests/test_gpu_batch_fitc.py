"""The batched small-knot FITC path on the GPU (SparseGPBatch.eval_fitc, norm_grad_ascent_batch,
optimize_gp_batch / cross_validate_gp with vi = False) against the CPU oracle, at
the project's bars: 1e-6 relative on the objective, |d| / max(1, |ref|) < 1e-6 per gradient entry,
rtol 1e-6 / atol 1e-9 for trajectories, 1e-7 for u_mean / u_var and 1e-8 of the largest reference
magnitude for predictions; independence of the batch bit for bit.  The problems are
tests/test_gpu_batch.py's (tests/batch_fitc_cases.py draws them)."""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest

from batch_fitc_cases import COINCIDENT, SEG, cases, gauss
from oracle import drivers as OD
from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
EVAL_RTOL = 1e-6
PRED_RTOL = 1e-8

_REF = {}


def _ref(P, U=None, cp=None, delta=None):
    """(objective, gradient) of the oracle, computed once per problem."""
    U = P["U"] if U is None else U
    cp = P["cov_par"] if cp is None else cp
    delta = P["delta"] if delta is None else delta
    key = (id(P["X"]), U.tobytes(), tuple(cp.items()), delta)
    if key not in _REF:
        o = O.fitc_obj_eval(cp, P["cov_fun"], U, P["X"], P["y"], P["mu"], delta)
        g = O.dlogp_dcov_par(cp, P["cov_fun"], U, P["X"], P["y"], P["mu"], delta)["gradient"]
        _REF[key] = (o, g)
    return _REF[key]


def _close(obj, grad, o_ref, g_ref, what=""):
    print(what, "obj rel", abs(obj - o_ref) / abs(o_ref), "grad",
          max(abs(grad[k] - g_ref[k]) / max(1.0, abs(g_ref[k])) for k in g_ref))
    assert abs(obj - o_ref) / abs(o_ref) < EVAL_RTOL, (what, obj, o_ref)
    for k in g_ref:
        assert abs(grad[k] - g_ref[k]) / max(1.0, abs(g_ref[k])) < EVAL_RTOL, \
            (what, k, grad[k], g_ref[k])


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _batch(Ps):
    import sparsergps_amd as S
    return S.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"]) for P in Ps])


def _groups():
    groups = OrderedDict()
    for name, P, _ in cases():
        if name.startswith("mixed"):
            groups.setdefault((P["X"].shape[1], P["cov_fun"]), []).append(P)
    return groups


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("key", list(_groups()))
def test_parity_in_one_mixed_batch(key):
    Ps = _groups()[key]
    with _batch(Ps) as b:
        obj, grad, status = b.eval_fitc([P["cov_par"] for P in Ps], key[1], [P["U"] for P in Ps],
                                        Ps[0]["delta"])
    assert (status == 0).all()
    for i, P in enumerate(Ps):
        o, g = _ref(P)
        assert list(grad[i]) == list(P["cov_par"])
        _close(obj[i], grad[i], o, g, (P["X"].shape, P["U"].shape))
    if key == (3, "sqexp"):     # sizes differ inside the one call, one of more than one segment
        assert sorted(P["X"].shape[0] for P in Ps) == [63, 1000, 2 * SEG + 37]


@pytest.mark.parametrize("n,m,d,cov_fun,seed", COINCIDENT)
def test_coincident_knots(n, m, d, cov_fun, seed):
    """Quirk Q5: knots that equal data rows exactly enter the tau derivative (half of them do)."""
    name, P, U = next(c for c in cases() if c[0] == f"coincident{m}")
    Q = gauss(150, 20, d, cov_fun, seed + 10)
    with _batch([Q, P]) as b:
        obj, grad, status = b.eval_fitc([Q["cov_par"], P["cov_par"]], cov_fun, [Q["U"], U], 1e-6)
    assert (status == 0).all()
    o, g = _ref(P, U)
    _close(obj[1], grad[1], o, g, name)
    _close(obj[0], grad[0], *_ref(Q), "beside it")
    # without the coincident pairs' 2 tau^2 G the tau entry is far outside the bar
    plain = _ref(P, U + 1e-9)[1]["tau"]
    assert abs(plain - g["tau"]) / max(1.0, abs(g["tau"])) > 1e-3


# ------------------------------------------------------------------ 2. independence
EIGHT = [(40, 5, 700), (700, 33, 701), (64, 16, 702), (513, 64, 703), (129, 17, 704),
         (1100, 48, 705), (16, 20, 706), (300, 1, 707)]


def _raw(b, Ps, order, active=None, sentinel=-123.25, flags=0, vi=False):
    B = len(order)
    theta = np.array([[Ps[i]["cov_par"][k] for k in ("sigma", "l", "tau")] for i in order])
    obj = np.full(B, sentinel)
    grad = np.full((B, 3), sentinel)
    status = np.full(B, 99, dtype=np.int32)
    run = b.eval_raw if vi else b.eval_fitc_raw
    run("sqexp", theta, [Ps[i]["U"] for i in order], 1e-6, flags, active, obj, grad, status)
    return obj, grad, status


def test_independence_bit_for_bit():
    Ps = [gauss(n, m, 3, "sqexp", seed) for n, m, seed in EIGHT]
    order = list(range(8))
    muus = [np.zeros(P["U"].shape[0]) for P in Ps]
    with _batch(Ps) as b:
        obj, grad, status = _raw(b, Ps, order)
        um, uv = b.posterior_u(muus)
        obj2, grad2, status2 = _raw(b, Ps, order)                    # the same call repeated
        um2, uv2 = b.posterior_u(muus)
        ov, gv, sv = _raw(b, Ps, order, vi=True)                     # a VI evaluation between two
        umv, uvv = b.posterior_u(muus)
        obj5, grad5, status5 = _raw(b, Ps, order)
        um5, uv5 = b.posterior_u(muus)
    assert (status == 0).all() and (status2 == 0).all() and (sv == 0).all() and (status5 == 0).all()
    assert np.array_equal(obj, obj2) and np.array_equal(grad, grad2)
    assert np.array_equal(obj, obj5) and np.array_equal(grad, grad5)
    for i in order:
        assert np.array_equal(um[i], um2[i]) and np.array_equal(uv[i], uv2[i])
        assert np.array_equal(um[i], um5[i]) and np.array_equal(uv[i], uv5[i])
    with _batch(Ps) as b:                                            # VI only: the same VI bits
        ov1, gv1, sv1 = _raw(b, Ps, order, vi=True)
        umv1, uvv1 = b.posterior_u(muus)
    assert np.array_equal(ov, ov1) and np.array_equal(gv, gv1) and (sv1 == 0).all()
    assert not np.array_equal(ov, obj)                               # ... of another objective
    for i in order:
        assert np.array_equal(umv[i], umv1[i]) and np.array_equal(uvv[i], uvv1[i])
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
    """Four problems on one row range (a multi-start) with four thetas and knot sets: each alias
    has the bits it has alone (row weights indexed by the resident row would not)."""
    import sparsergps_amd as S
    P = gauss(600, 24, 3, "sqexp", 530)
    g = np.random.Generator(np.random.PCG64(531))
    cps = [OrderedDict([("sigma", 1.2 - 0.1 * k), ("l", 1.7 + 0.3 * k), ("tau", 0.5 + 0.05 * k)])
           for k in range(4)]
    Us = [g.uniform(0.0, 10.0, size=(m, 3)) for m in (24, 7, 40, 16)]
    with S.SparseGPBatch(P["X"], P["y"], P["mu"], [0] * 4, [600] * 4) as b:
        obj, grad, status = b.eval_fitc(cps, "sqexp", Us, 1e-6)
    assert (status == 0).all()
    for k in range(4):
        _close(obj[k], grad[k], *_ref(P, Us[k], cps[k]), k)
        with S.SparseGPBatch(P["X"], P["y"], P["mu"]) as b1:
            o1, g1, _ = b1.eval_fitc([cps[k]], "sqexp", [Us[k]], 1e-6)
        assert np.array_equal(o1[0], obj[k]) and list(g1[0].values()) == list(grad[k].values())


def test_flags():
    from sparsergps_amd import _lib
    Ps = [gauss(n, m, 3, "sqexp", seed) for n, m, seed in EIGHT[:4]]
    order = list(range(4))
    with _batch(Ps) as b:
        obj, grad, status = _raw(b, Ps, order)
        o2, g2, s2 = _raw(b, Ps, order, flags=_lib.SGP_FLAG_OBJ_ONLY)
        o3, g3, s3 = _raw(b, Ps, order, flags=_lib.SGP_FLAG_R_DET)
        o4, g4, s4 = b.eval_fitc([P["cov_par"] for P in Ps], "sqexp", [P["U"] for P in Ps], 1e-6,
                                 obj_only=True)
    assert np.array_equal(o2, obj) and (g2 == -123.25).all() and (s2 == 0).all()   # grad untouched
    assert np.array_equal(o4, obj) and (s4 == 0).all() and all(g is None for g in g4)
    # the oracle's obj_fun_norm takes log(det(Sigma22)) as R does: what SGP_FLAG_R_DET evaluates
    for i, P in enumerate(Ps):
        assert abs(np.linalg.slogdet(O.fitc_mats(P["cov_par"], "sqexp", P["U"], P["X"], 1e-6)[1])[1]) < 700
        assert abs(o3[i] - _ref(P)[0]) / abs(_ref(P)[0]) < EVAL_RTOL
    np.testing.assert_allclose(o3, obj, rtol=1e-12, atol=0.0)
    assert np.array_equal(g3, grad) and (s3 == 0).all()   # the gradient does not read the flag


# ------------------------------------------------------------------ 3. one bad problem
@pytest.mark.parametrize("m,dup", [(40, 25), (64, 63), (17, 16)])
def test_one_bad_problem(m, dup):
    """A duplicated knot with delta = 0: K22 is singular.  Knot `dup` copies knot 0 and sigma = 1,
    so the first pivot is exactly 1 and the sweep leaves an exact zero on the copy's diagonal and
    in its row: the leading minor of order dup + 1 is the first that is not positive, with no
    rounding to decide it.  The bad problem reports that order and NaN, its neighbours in the same
    call have the bits of the call before, and its posterior is the earlier one's."""
    d = 3
    g = np.random.Generator(np.random.PCG64(77))
    X = g.uniform(0.0, 10.0, size=(300, d))
    y = np.sin(X).sum(axis=1) + g.normal(0.0, 0.5, size=300)
    cp = OrderedDict([("sigma", 1.0), ("l", 0.3), ("tau", 0.5)])
    Us = [g.uniform(0.0, 10.0, size=(k, d)) for k in (m, m, 12)]
    Ubad = Us[1].copy()
    Ubad[dup] = Ubad[0]
    xt = g.uniform(0.0, 10.0, size=(70, d))
    yt = np.sin(xt).sum(axis=1)
    probs = [(X, y, np.full(300, y.mean()))] * 3
    muus = [np.zeros(u.shape[0]) for u in Us]
    import sparsergps_amd as S

    def predict(b):
        pm, pv, nlp, stats = (np.full(210, -1.5), np.full(210, -1.5), np.full(210, -1.5),
                              np.full((3, 4), -1.5))
        b.predict_raw(None, pm, pv, nlp, stats)
        return pm, pv, nlp, stats

    with S.SparseGPBatch.from_problems(probs) as b:
        b.set_test(xt, yt, 0.1)
        obj, grad, st = b.eval_fitc([cp] * 3, "sqexp", Us, 0.0)
        assert (st == 0).all() and np.isfinite(obj).all()
        um, uv = b.posterior_u(muus)
        first = predict(b)
        obj2, grad2, st2 = b.eval_fitc([cp] * 3, "sqexp", [Us[0], Ubad, Us[2]], 0.0)
        assert list(st2) == [0, dup + 1, 0]
        assert b"problem 1" in b._lib.sgp_last_error() and b"Sigma22" in b._lib.sgp_last_error()
        assert np.isnan(obj2[1]) and all(np.isnan(v) for v in grad2[1].values())
        for i in (0, 2):
            assert np.array_equal(obj2[i], obj[i])
            assert list(grad2[i].values()) == list(grad[i].values())
        um2, uv2 = b.posterior_u(muus)
        second = predict(b)
    for i in range(3):                                   # `post` untouched, the bad problem's too
        assert np.array_equal(um2[i], um[i]) and np.array_equal(uv2[i], uv[i])
    for u, w in zip(first, second):
        assert np.array_equal(u, w)
    _close(obj[0], grad[0], *_ref(dict(X=X, y=y, mu=probs[0][2], U=Us[0], cov_par=cp,
                                       cov_fun="sqexp", delta=0.0)), "the good neighbour")


# ------------------------------------------------------------------ 4. posterior
def test_posterior():
    Ps = _groups()[(3, "sqexp")] + [gauss(200, 16, 3, "sqexp", 520)]
    muus = [np.full(P["U"].shape[0], 0.1 * (i + 1)) for i, P in enumerate(Ps)]
    with _batch(Ps) as b:
        _, _, status = b.eval_fitc([P["cov_par"] for P in Ps], "sqexp", [P["U"] for P in Ps], 1e-6)
        um, uv = b.posterior_u(muus)
    assert (status == 0).all()
    for i, P in enumerate(Ps):
        m_ref, v_ref = O.fitc_posterior_u(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["mu"],
                                          muus[i], 1e-6)
        print("posterior", i, np.abs(um[i] - m_ref).max(), np.abs(uv[i] - v_ref).max())
        np.testing.assert_allclose(um[i], m_ref, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(uv[i], v_ref, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------ 5. prediction and scoring
# (m, test rows): every knot count 1, 15, 16, 17, 33, 64 and every row count 1, 63, 64, 65, 513, 1100
PRED = [(1, 1), (15, 63), (16, 64), (17, 65), (33, 513), (64, 1100)]
PAD = 5


@functools.lru_cache(maxsize=None)
def _pcase(m, nt, delta):
    """tests/test_gpu_batch_predict.py::_case with the FITC posterior and predict_laplace."""
    P = dict(O.make_gaussian_problem("C2", n=400, m=m), delta=delta)
    muu = np.full(m, P["y"].mean())
    um, uv = O.fitc_posterior_u(P["cov_par"], P["cov_fun"], P["U"], P["X"], P["y"], P["mu"], muu,
                                delta)
    g = np.random.default_rng(21 + m)
    xp = g.uniform(0, 10, size=(nt, P["X"].shape[1]))
    k = min(2, m, nt)
    xp[:k] = P["U"][:k]                               # prediction at knots (exact coincidence)
    mup = P["y"].mean() + 0.1 * np.cos(np.arange(nt))
    yp = np.sin(xp).sum(axis=1) + g.normal(0, 0.5, nt)
    ref = O.predict_laplace(um, uv, P["U"], xp, P["cov_fun"], P["cov_par"], mup, muu, False,
                            "gaussian", delta)
    return dict(P=P, muu=muu, um=um, uv=uv, xp=xp, mup=mup, yp=yp, ref=ref)


def _tests(cs):
    d = cs[0]["xp"].shape[1]
    X = np.vstack([np.full((PAD, d), 3.0)] + [c["xp"] for c in cs])
    y = np.concatenate([np.zeros(PAD)] + [c["yp"] for c in cs])
    mu = np.concatenate([np.zeros(PAD)] + [c["mup"] for c in cs])
    nrow = np.array([c["xp"].shape[0] for c in cs], dtype=np.int64)
    row0 = PAD + np.concatenate([[0], np.cumsum(nrow)[:-1]])
    return X, y, mu, row0, nrow


def _model_of(c):
    P = c["P"]
    return {"family": "gaussian", "sparse": True, "delta": P["delta"],
            "results": {"u_mean": c["um_gpu"], "u_var": c["uv_gpu"], "xu": P["U"],
                        "cov_fun": P["cov_fun"], "cov_par": P["cov_par"], "muu": c["muu"]}}


@pytest.mark.parametrize("delta", [1e-6, 1e-2])
def test_prediction_and_scoring(delta):
    """predict_laplace(family = "gaussian") on fitc_posterior_u, and a loop of score_gp(vi=False).
    At delta = 1e-2 a constant carrying delta (predict_vi's) is 1e-2 / 1.7 off: far past 1e-8."""
    import sparsergps_amd as S
    cs = [dict(_pcase(m, nt, delta)) for m, nt in (PRED if delta == 1e-6 else PRED[3:5])]
    Ps = [c["P"] for c in cs]
    X, y, mu, row0, nrow = _tests(cs)
    with _batch(Ps) as b:
        _, _, st = b.eval_fitc([P["cov_par"] for P in Ps], "sqexp", [P["U"] for P in Ps], delta)
        assert (st == 0).all()
        b.set_test(X, y, mu, row0, nrow)
        out = b.predict()
        scores = b.score()
        ums, uvs = b.posterior_u([c["muu"] for c in cs])
    for i, c in enumerate(cs):
        P = c["P"]
        em = _rel(out[i]["pred_mean"], c["ref"]["pred_mean"])
        ev = _rel(out[i]["pred_var"], c["ref"]["pred_var"])
        print(f"delta={delta} m={P['U'].shape[0]} rows={nrow[i]}: mean {em:.2e} var {ev:.2e}")
        assert em < PRED_RTOL and ev < PRED_RTOL, (i, em, ev)
        c["um_gpu"], c["uv_gpu"] = ums[i], uvs[i]
        one = S.score_gp(_model_of(c), c["xp"], c["yp"], c["mup"], vi=False)
        s = scores[i]
        assert np.array_equal(s["pred"]["pred_mean"], out[i]["pred_mean"])
        assert _rel(s["pred"]["pred_mean"], one["pred"]["pred_mean"]) < PRED_RTOL
        assert _rel(s["pred"]["pred_var"], one["pred"]["pred_var"]) < PRED_RTOL
        np.testing.assert_allclose(s["nlp"], one["nlp"], rtol=1e-6, atol=1e-7)
        for key in ("median_nlp", "mean_nlp", "rmse", "srmse", "n_nan"):
            np.testing.assert_allclose(s[key], one[key], rtol=1e-6, atol=1e-7, err_msg=key)
        tau = P["cov_par"]["tau"]                        # quirk Q23: pred_var + tau^2 as written
        v = s["pred"]["pred_var"] + tau ** 2
        want = 0.5 * np.log(2 * np.pi * v) + (c["yp"] - s["pred"]["pred_mean"].reshape(-1)) ** 2 / (2 * v)
        np.testing.assert_allclose(s["nlp"], want, rtol=1e-13, atol=1e-13)


def test_one_batch_of_both_kinds():
    """Problem 0's last evaluation is VI, problem 1's FITC: each is predicted by its own rule, and
    the VI problem's outputs are those of a batch that never saw FITC, bit for bit."""
    delta = 1e-2
    cs = [_pcase(17, 65, delta), _pcase(33, 513, delta)]
    Ps = [c["P"] for c in cs]
    X, y, mu, row0, nrow = _tests(cs)
    off = np.concatenate([[0], np.cumsum(nrow)])
    pars, Us = [P["cov_par"] for P in Ps], [P["U"] for P in Ps]

    def run(b):
        pm, pv, nlp, stats = (np.zeros(off[-1]), np.zeros(off[-1]), np.zeros(off[-1]),
                              np.zeros((2, 4)))
        b.predict_raw(None, pm, pv, nlp, stats)
        return pm, pv, nlp, stats

    with _batch(Ps) as b:
        b.set_test(X, y, mu, row0, nrow)
        _, _, st = b.eval_vi(pars, "sqexp", Us, delta)
        assert (st == 0).all()
        vi_only = run(b)
        _, _, st = b.eval_fitc(pars, "sqexp", Us, delta, active=np.array([0, 1], dtype=np.uint8))
        assert st[1] == 0
        mixed = run(b)
    s0, s1 = slice(off[0], off[1]), slice(off[1], off[2])
    for k in range(3):
        assert np.array_equal(mixed[k][s0], vi_only[k][s0])
        assert not np.array_equal(mixed[k][s1], vi_only[k][s1])
    assert np.array_equal(mixed[3][0], vi_only[3][0])
    assert _rel(mixed[0][s1], cs[1]["ref"]["pred_mean"]) < PRED_RTOL
    assert _rel(mixed[1][s1], cs[1]["ref"]["pred_var"]) < PRED_RTOL
    P = Ps[0]
    um, uv = O.vi_posterior_u(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["mu"], cs[0]["muu"],
                              delta)
    vref = O.predict_vi(um, uv, P["U"], cs[0]["xp"], "sqexp", P["cov_par"], cs[0]["mup"],
                        cs[0]["muu"], False, delta)
    assert _rel(mixed[0][s0], vref["pred_mean"]) < PRED_RTOL
    assert _rel(mixed[1][s0], vref["pred_var"]) < PRED_RTOL


# ------------------------------------------------------------------ 6. the lockstep ascent
ASCENT = [(90, 6), (200, 12), (333, 20), (150, 33)]


@functools.lru_cache(maxsize=None)
def _ascent_ref(opt_items):
    opt = dict(opt_items)
    out = []
    for i, (n, m) in enumerate(ASCENT):
        P = gauss(n, m, 3, "sqexp", 700 + i)
        out.append(OD.norm_grad_ascent(P["cov_par"], "sqexp", P["U"], P["X"], P["y"], P["mu"],
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


# tests/test_gpu_batch.py::test_lockstep_ascent's option sets
@pytest.mark.parametrize("opt", [
    {"maxit": 5, "obj_tol": 0.0},
    {"maxit": 30, "obj_tol": 2.5},
    {"maxit": 5, "obj_tol": 0.0, "optim_method": "ga", "learn_rate": 1e-4},
    # the FITC objective's steps are smaller than the ELBO's: 2.5 stops every problem at once.
    # The reference's |obj steps| are 0.30 from the start for problem 0, fall from 0.594 to 0.585
    # at iteration 8 for problem 1 and from 0.593 to 0.588 at iteration 10 for problem 3, and stay
    # above 0.57 to the end for problem 2: the four retire at different iterations
    {"maxit": 30, "obj_tol": 0.59}])
def test_lockstep_ascent(opt):
    import sparsergps_amd as S
    Ps = [gauss(n, m, 3, "sqexp", 700 + i) for i, (n, m) in enumerate(ASCENT)]
    ref = _ascent_ref(tuple(sorted(opt.items())))
    res = S.norm_grad_ascent_batch([P["cov_par"] for P in Ps], "sqexp", [P["U"] for P in Ps],
                                   [(P["X"], P["y"], P["mu"]) for P in Ps], opt=opt)
    print("iterations", [r["iter"] for r in ref])
    assert [r["iter"] for r in res] == [r["iter"] for r in ref]
    assert all(2 <= r["iter"] <= opt["maxit"] for r in ref)
    if opt["obj_tol"] == 0.59:
        assert len({r["iter"] for r in ref}) == 4 and max(r["iter"] for r in ref) == 30
    for r, rf in zip(res, ref):
        _same_fit(r, rf)
        assert "error" not in r


# ------------------------------------------------------------------ 7. end to end
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
    Ps = [gauss(n, m, 3, "sqexp", 700 + i) for i, (n, m) in enumerate(ASCENT[:3])]
    opt = {"maxit": 5}
    mods = S.optimize_gp_batch([(P["X"], P["y"], P["mu"]) for P in Ps], "sqexp", Ps[0]["cov_par"],
                               [P["U"] for P in Ps], opt=opt, vi=False)
    g = np.random.Generator(np.random.PCG64(799))
    xt = g.uniform(0.0, 10.0, size=(50, 3))
    yt = np.sin(xt).sum(axis=1) / math.sqrt(3)
    for P, mod in zip(Ps, mods):
        one = S.optimize_gp(P["y"], P["X"], "sqexp", Ps[0]["cov_par"], P["mu"], sparse=True,
                            xu_opt="fixed", xu=P["U"], vi=False, opt=opt)
        assert set(mod) == set(one) and mod["sparse"] is True and mod["family"] == "gaussian"
        assert set(mod["results"]) == set(one["results"])
        assert mod["results"]["iter"] == one["results"]["iter"] == 5
        for key in ("obj_fun", "grad", "cov_par_history"):
            np.testing.assert_allclose(mod["results"][key], one["results"][key], rtol=1e-6,
                                       atol=1e-9, err_msg=key)
        for key in ("u_mean", "u_var", "muu"):
            np.testing.assert_allclose(mod["results"][key], one["results"][key], rtol=1e-6,
                                       atol=1e-7, err_msg=key)
        _same(S.predict_gp(mod, xt, vi=False), S.predict_gp(one, xt, vi=False), "predict_gp")
        _same(S.score_gp(mod, xt, yt, vi=False), S.score_gp(one, xt, yt, vi=False), "score_gp")


def test_cross_validate_end_to_end():
    import sparsergps_amd as S
    g = np.random.Generator(np.random.PCG64(4242))
    n, d, m = 300, 3, 10
    X = g.uniform(0.0, 10.0, size=(n, d))
    y = np.sin(X).sum(axis=1) / math.sqrt(d) + g.normal(0.0, 0.5, size=n) + 1.0
    xu = g.uniform(0.0, 10.0, size=(m, d))
    cp = OrderedDict([("sigma", 1.2), ("l", 1.7), ("tau", 0.5)])
    opt = {"maxit": 10}
    res = S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=3, opt=opt, vi=False)
    assert len(res["folds"]) == 3
    assert sorted(np.concatenate([f["test_rows"] for f in res["folds"]])) == list(range(n))
    nlps = []
    for f in res["folds"]:
        te = f["test_rows"]
        tr = np.setdiff1d(np.arange(n), te)
        mu_tr = y[tr].mean()
        seq = S.optimize_gp(y[tr], X[tr], "sqexp", cp, np.full(tr.size, mu_tr), sparse=True,
                            xu_opt="fixed", xu=xu, vi=False, opt=opt)
        assert f["model"]["results"]["iter"] == seq["results"]["iter"]
        np.testing.assert_allclose(f["model"]["results"]["obj_fun"], seq["results"]["obj_fun"],
                                   rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(list(f["model"]["results"]["cov_par"].values()),
                                   list(seq["results"]["cov_par"].values()), rtol=1e-6, atol=1e-9)
        one = S.score_gp(seq, X[te], y[te], np.full(te.size, mu_tr), vi=False)
        s = f["score"]
        assert _rel(s["pred"]["pred_mean"], one["pred"]["pred_mean"]) < 1e-6
        assert _rel(s["pred"]["pred_var"], one["pred"]["pred_var"]) < 1e-6
        # on the batch's own model the two scorers meet at the prediction bar
        own = S.score_gp(f["model"], X[te], y[te], np.full(te.size, mu_tr), vi=False)
        assert _rel(s["pred"]["pred_mean"], own["pred"]["pred_mean"]) < PRED_RTOL
        assert _rel(s["pred"]["pred_var"], own["pred"]["pred_var"]) < PRED_RTOL
        np.testing.assert_allclose(s["nlp"], one["nlp"], rtol=1e-6, atol=1e-7)
        for key in ("median_nlp", "mean_nlp", "rmse", "srmse", "n_nan"):
            np.testing.assert_allclose(s[key], one[key], rtol=1e-6, atol=1e-7, err_msg=key)
        nlps.append(s["nlp"])
    assert res["mean_nlp"] == pytest.approx(np.concatenate(nlps).mean(), rel=1e-13)
    assert res["rmse"] < np.std(y)          # the fits do predict
    # vi = True is the default and stays what it was: the same call with and without the keyword
    a = S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=3, opt=opt)
    b = S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=3, opt=opt, vi=True)
    assert a["mean_nlp"] == b["mean_nlp"] and a["rmse"] == b["rmse"]
    assert a["mean_nlp"] != res["mean_nlp"]
    for fa, fb in zip(a["folds"], b["folds"]):
        assert np.array_equal(fa["score"]["nlp"], fb["score"]["nlp"])
        te = fa["test_rows"]
        tr = np.setdiff1d(np.arange(n), te)
        one = S.score_gp(fa["model"], X[te], y[te], np.full(te.size, y[tr].mean()), vi=True)
        assert _rel(fa["score"]["pred"]["pred_var"], one["pred"]["pred_var"]) < PRED_RTOL


def test_stage_times():
    Ps = [gauss(n, m, 3, "sqexp", seed) for n, m, seed in EIGHT[:2]]
    with _batch(Ps) as b:
        assert (b.fitc_stage_ms(True) == 0).all()
        b.eval_fitc([P["cov_par"] for P in Ps], "sqexp", [P["U"] for P in Ps], 1e-6)
        ms = b.fitc_stage_ms(True)
        assert ms.shape == (5,) and (ms > 0).all()
        b.eval_fitc([P["cov_par"] for P in Ps], "sqexp", [P["U"] for P in Ps], 1e-6, obj_only=True)
        ms = b.fitc_stage_ms(False)
        assert (ms[:3] > 0).all() and ms[3] + ms[4] < ms[:3].sum()   # no gradient stages ran
