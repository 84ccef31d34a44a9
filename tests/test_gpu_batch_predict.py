"""Batched held-out prediction and scoring on the GPU (SparseGPBatch.set_test / predict / score,
cross_validate_gp).

Parity is against oracle.sgp_oracle.predict_vi on oracle.sgp_oracle.vi_posterior_u at the same
theta, at the project's prediction tolerance RTOL = 1e-8 in tests/test_gpu_predictor.py's _rel norm
(largest absolute difference over the largest reference magnitude); the data are
make_gaussian_problem's as its _pred_inputs draws them (the first two test rows equal to knots, a
per-row mu).  Every knot count 1, 15, 16, 17, 33, 64 (nb = 1 .. 4, partial and full 16-blocks) and
every row count 1, 63, 64, 65, 513, 1100 (partial steps, a second segment of one row, three
segments) is in the d = 3 batch; d = 8 and d = 12 (ard) hold two of each.  d = 1 is C2's first
column with m = 1 and m = 8 only: knots drawn from U(0, 10) at l = 1 in one dimension give
cond(K22 + S / z) = 7.6e7 at m = 15 and 4.8e8 at m = 16, where two fp64 evaluations of the
reference's own formulas differ by 9e-11 and 4e-9 on the CPU -- no room under 1e-8 that a test
could hold a kernel to -- against 1.7e3 at m = 8 (the d = 3, m = 64 case has 3.7e3).
The parity test prints every measured error (DESIGN.md sec. 0o records them).
Independence of the batch is asserted bit for bit."""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest

from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-8
PAD = 5     # rows of Xt in front of the first problem's: no test range starts on a 64-row grid

# group -> (cfg, m, test rows, d override, first column only)
GROUPS = OrderedDict([
    ("d1_sqexp", [("C2", 1, 1, None, True), ("C2", 8, 63, None, True)]),
    ("d3_sqexp", [("C2", 1, 1, None, False), ("C2", 15, 63, None, False),
                  ("C2", 16, 64, None, False), ("C2", 17, 65, None, False),
                  ("C2", 33, 513, None, False), ("C2", 64, 1100, None, False)]),
    ("d8_ard", [("C3", 16, 64, None, False), ("C3", 64, 513, None, False)]),
    ("d12_ard", [("C3", 17, 65, 12, False), ("C3", 33, 1100, 12, False)]),
])


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


@functools.lru_cache(maxsize=None)
def _case(cfg, m, nt, d, col1):
    """One problem, its test rows and the oracle's prediction; computed once."""
    P = O.make_gaussian_problem(cfg, n=400, m=m, d=d) if d else \
        O.make_gaussian_problem(cfg, n=400, m=m)
    if col1:
        P = dict(P, X=P["X"][:, :1].copy(), U=P["U"][:, :1].copy())
    dd = P["X"].shape[1]
    muu = np.full(m, P["y"].mean())
    um, uv = O.vi_posterior_u(P["cov_par"], P["cov_fun"], P["U"], P["X"], P["y"], P["mu"], muu,
                              P["delta"])
    g = np.random.default_rng(21 + m)
    xp = g.uniform(0, 10, size=(nt, dd))
    k = min(2, m, nt)
    xp[:k] = P["U"][:k]                               # prediction at knots (exact coincidence)
    mup = P["y"].mean() + 0.1 * np.cos(np.arange(nt))
    yp = np.sin(xp).sum(axis=1) / (math.sqrt(dd) if cfg == "C3" else 1.0) + g.normal(0, 0.5, nt)
    ref = O.predict_vi(um, uv, P["U"], xp, P["cov_fun"], P["cov_par"], mup, muu, False, P["delta"])
    return dict(P=P, muu=muu, xp=xp, mup=mup, yp=yp, ref=ref)


def _group(name):
    return [_case(*c) for c in GROUPS[name]]


def _tests(cases, with_y=True, pad=PAD):
    """One Xt / yt / mut with `pad` unused rows in front, and the problems' ranges."""
    d = cases[0]["xp"].shape[1]
    X = np.vstack([np.full((pad, d), 3.0)] + [c["xp"] for c in cases])
    y = np.concatenate([np.zeros(pad)] + [c["yp"] for c in cases])
    mu = np.concatenate([np.zeros(pad)] + [c["mup"] for c in cases])
    nrow = np.array([c["xp"].shape[0] for c in cases], dtype=np.int64)
    row0 = pad + np.concatenate([[0], np.cumsum(nrow)[:-1]])
    return X, (y if with_y else None), mu, row0, nrow


def _fitted(S, cases, order=None):
    """A batch of the cases' training problems, evaluated once at their theta and knots."""
    order = list(range(len(cases))) if order is None else order
    Ps = [cases[i]["P"] for i in order]
    b = S.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"]) for P in Ps])
    _, _, status = b.eval_vi([P["cov_par"] for P in Ps], Ps[0]["cov_fun"], [P["U"] for P in Ps],
                             Ps[0]["delta"])
    assert (status == 0).all()
    return b


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", list(GROUPS))
def test_parity_in_one_mixed_batch(sgp, name):
    cases = _group(name)
    X, y, mu, row0, nrow = _tests(cases, with_y=False)
    assert all(r % 64 for r in row0)
    with _fitted(sgp, cases) as b:
        b.set_test(X, y, mu, row0, nrow)
        out = b.predict()
        ums, uvs = b.posterior_u([c["muu"] for c in cases])
    worst = [0.0] * 4
    for i, c in enumerate(cases):
        P = c["P"]
        assert out[i]["pred_mean"].shape == (nrow[i], 1) and out[i]["pred_var"].shape == (nrow[i],)
        em = _rel(out[i]["pred_mean"], c["ref"]["pred_mean"])
        ev = _rel(out[i]["pred_var"], c["ref"]["pred_var"])
        # the existing GPU route, fed the posterior the batch hands out
        old = sgp.predict_vi(ums[i], uvs[i], P["U"], c["xp"], P["cov_fun"], P["cov_par"], c["mup"],
                             c["muu"], delta=P["delta"])
        gm = _rel(out[i]["pred_mean"], old["pred_mean"])
        gv = _rel(out[i]["pred_var"], old["pred_var"])
        print(f"{name} m={P['U'].shape[0]} rows={nrow[i]}: oracle mean {em:.2e} var {ev:.2e}; "
              f"predict_vi mean {gm:.2e} var {gv:.2e}")
        worst = [max(w, e) for w, e in zip(worst, (em, ev, gm, gv))]
        assert em < RTOL and ev < RTOL, (name, i, em, ev)
        assert gm < RTOL and gv < RTOL, (name, i, gm, gv)
    print(f"{name} worst: oracle {worst[0]:.1e} / {worst[1]:.1e}; predict_vi {worst[2]:.1e} / "
          f"{worst[3]:.1e}")


# ------------------------------------------------------------------ 2. scoring
def _raw(b, tot, B, active=None, score=True, fill=-123.25):
    pm, pv = np.full(tot, fill), np.full(tot, fill)
    nlp = np.full(tot, fill) if score else None
    stats = np.full((B, 4), fill) if score else None
    b.predict_raw(active, pm, pv, nlp, stats)
    return pm, pv, nlp, stats


def test_scoring(sgp):
    cases = _group("d3_sqexp")
    X, y, mu, row0, nrow = _tests(cases)
    off = np.concatenate([[0], np.cumsum(nrow)])
    with _fitted(sgp, cases) as b:
        b.set_test(X, y, mu, row0, nrow)
        pm, pv, nlp, stats = _raw(b, off[-1], len(cases))
        scores = b.score()
        only = b.predict()
        # one row of problem 4 with mu = inf: data, not an error
        bad = mu.copy()
        bad[row0[4] + 70] = np.inf
        b.set_test(X, y, bad, row0, nrow)
        pm2, pv2, nlp2, stats2 = _raw(b, off[-1], len(cases))
        s2 = b.score()
    for i, c in enumerate(cases):
        sl = slice(off[i], off[i + 1])
        tau = c["P"]["cov_par"]["tau"]
        yt = c["yp"]
        v = pv[sl] + tau ** 2
        want = 0.5 * np.log(2 * np.pi * v) + (yt - pm[sl]) ** 2 / (2 * v)
        print("nlp", i, float(np.max(np.abs(nlp[sl] - want) / np.abs(want))))
        np.testing.assert_allclose(nlp[sl], want, rtol=1e-13, atol=1e-13)
        # a missing or doubled tau^2 is far outside that
        for wrong in (pv[sl], pv[sl] + 2 * tau ** 2):
            off_by = 0.5 * np.log(2 * np.pi * wrong) + (yt - pm[sl]) ** 2 / (2 * wrong)
            assert np.max(np.abs(off_by - want)) > 1e-3
        assert np.isfinite(nlp[sl]).all()
        np.testing.assert_allclose(stats[i], [nlp[sl].sum(), nrow[i], 0.0,
                                              ((pm[sl] - yt) ** 2).sum()], rtol=1e-12, atol=0.0)
        # score(): the same vectors, and score_gp's host formulas on them
        s = scores[i]
        assert np.array_equal(s["nlp"], nlp[sl]) and np.array_equal(s["pred"]["pred_var"], pv[sl])
        assert np.array_equal(s["pred"]["pred_mean"], pm[sl].reshape(-1, 1))
        assert np.array_equal(only[i]["pred_mean"], s["pred"]["pred_mean"])      # scoring or not
        assert np.array_equal(only[i]["pred_var"], s["pred"]["pred_var"])
        rmse = math.sqrt(stats[i][3] / nrow[i])
        assert s["median_nlp"] == float(np.median(nlp[sl])) and s["n_nan"] == 0
        assert s["mean_nlp"] == float(stats[i][0] / stats[i][1]) and s["rmse"] == rmse
        if nrow[i] > 1:
            assert s["srmse"] == rmse / float(np.std(yt, ddof=1))
        else:
            assert math.isnan(s["srmse"])
        np.testing.assert_allclose(s["mean_nlp"], nlp[sl].mean(), rtol=1e-12)
        np.testing.assert_allclose(s["rmse"], np.sqrt(np.mean((pm[sl] - yt) ** 2)), rtol=1e-12)
    # the mu = inf row: its mean is inf, its nlp NaN, it is counted, and nothing else moved
    r = off[4] + 70
    assert np.isinf(pm2[r]) and np.isnan(nlp2[r]) and stats2[4][2] == 1.0 and s2[4]["n_nan"] == 1
    assert stats2[4][1] == nrow[4] - 1
    keep = np.arange(off[-1]) != r
    assert np.array_equal(pm2[keep], pm[keep]) and np.array_equal(nlp2[keep], nlp[keep])
    assert np.array_equal(pv2, pv)
    fin = np.delete(nlp2[off[4]:off[5]], 70)
    assert s2[4]["median_nlp"] == float(np.median(fin))
    np.testing.assert_allclose(stats2[4][0], fin.sum(), rtol=1e-12)
    for i in (0, 1, 2, 3, 5):
        assert np.array_equal(stats2[i], stats[i])


# ------------------------------------------------------------------ 3. independence
FIVE = [("C2", 5, 1, None, False), ("C2", 33, 513, None, False), ("C2", 16, 64, None, False),
        ("C2", 64, 1100, None, False), ("C2", 17, 65, None, False)]


def _run(S, cases, order, active=None, repeat=False):
    sub = [cases[i] for i in order]
    X, y, mu, row0, nrow = _tests(sub)
    off = np.concatenate([[0], np.cumsum(nrow)])
    with _fitted(S, cases, order) as b:
        b.set_test(X, y, mu, row0, nrow)
        pm, pv, nlp, stats = _raw(b, off[-1], len(order), active)
        if repeat:
            again = _raw(b, off[-1], len(order), active)
            for u, w in zip((pm, pv, nlp, stats), again):
                assert np.array_equal(u, w)
    return {i: (pm[off[k]:off[k + 1]], pv[off[k]:off[k + 1]], nlp[off[k]:off[k + 1]], stats[k])
            for k, i in enumerate(order)}


def _same(a, b):
    return all(np.array_equal(u, w) for u, w in zip(a, b))


def test_independence_bit_for_bit(sgp):
    cases = [_case(*c) for c in FIVE]
    order = list(range(5))
    full = _run(sgp, cases, order, repeat=True)
    for i in order:
        assert np.isfinite(full[i][2]).all() and full[i][3][1] == cases[i]["xp"].shape[0]
        assert _same(_run(sgp, cases, [i])[i], full[i]), i                  # alone
    rev = _run(sgp, cases, order[::-1])                                      # reversed
    assert all(_same(rev[i], full[i]) for i in order)
    act = np.array([1, 0, 1, 0, 1], dtype=np.uint8)                          # under a mask
    part = _run(sgp, cases, order, active=act)
    for i in order:
        if act[i]:
            assert _same(part[i], full[i]), i
        else:                                                                # the sentinel stands
            assert all((v == -123.25).all() for v in part[i]), i


def test_aliased_test_range(sgp):
    """Two problems with the same fit name one test range: the same bits, packed twice."""
    c = _case("C2", 33, 513, None, False)
    P = c["P"]
    with sgp.SparseGPBatch(P["X"], P["y"], P["mu"], [0, 0], [400, 400]) as b:
        _, _, status = b.eval_vi([P["cov_par"]] * 2, "sqexp", [P["U"]] * 2, P["delta"])
        assert (status == 0).all()
        b.set_test(c["xp"], c["yp"], c["mup"])                # every problem takes all rows
        pm, pv, nlp, stats = _raw(b, 2 * 513, 2)
    assert np.array_equal(pm[:513], pm[513:]) and np.array_equal(pv[:513], pv[513:])
    assert np.array_equal(nlp[:513], nlp[513:]) and np.array_equal(stats[0], stats[1])
    alone = _run(sgp, [c], [0])[0]
    assert _same((pm[:513], pv[:513], nlp[:513], stats[0]), alone)
    assert _rel(pm[:513], c["ref"]["pred_mean"]) < RTOL


# ------------------------------------------------------------------ 4. which posterior
def test_a_failed_evaluation_leaves_the_posterior(sgp):
    """tests/test_gpu_batch.py::test_one_bad_problem's construction: after a good evaluation at
    theta_1, problem 1 is evaluated with a duplicated knot and a negative jitter and is not
    positive definite; the others move to theta_2."""
    d, m = 3, 17
    g = np.random.Generator(np.random.PCG64(77))
    U = g.uniform(0.0, 10.0, size=(m, d))
    X = g.uniform(0.0, 10.0, size=(300, d))
    y = np.sin(X).sum(axis=1) + g.normal(0.0, 0.5, size=300)
    Us = [g.uniform(0.0, 10.0, size=(k, d)) for k in (m, m, 12)]
    Ubad = U.copy()
    Ubad[16] = Ubad[3]
    xt = g.uniform(0.0, 10.0, size=(70, d))
    yt = np.sin(xt).sum(axis=1)
    cp1 = OrderedDict([("sigma", 1.0), ("l", 0.3), ("tau", 0.5)])
    cp2 = OrderedDict([("sigma", 1.1), ("l", 0.35), ("tau", 0.45)])
    delta = -1e-3
    probs = [(X, y, np.full(300, y.mean()))] * 3

    def predict(b):
        return _raw(b, 210, 3)

    with sgp.SparseGPBatch.from_problems(probs) as b:
        b.set_test(xt, yt, 0.1)
        _, _, st = b.eval_vi([cp1] * 3, "sqexp", Us, delta)
        assert (st == 0).all()
        first = predict(b)
        _, _, st = b.eval_vi([cp2] * 3, "sqexp", [Us[0], Ubad, Us[2]], delta)
        assert st[0] == 0 and st[1] == 17 and st[2] == 0
        second = predict(b)
    with sgp.SparseGPBatch.from_problems(probs) as b:       # theta_2 alone, for the other two
        b.set_test(xt, yt, 0.1)
        _, _, st = b.eval_vi([cp2] * 3, "sqexp", Us, delta)
        assert (st == 0).all()
        fresh = predict(b)
    mid = slice(70, 140)
    for k in range(3):
        assert np.array_equal(second[k][mid], first[k][mid])             # theta_1's, bit for bit
    assert np.array_equal(second[3][1], first[3][1])
    for sl, p in ((slice(0, 70), 0), (slice(140, 210), 2)):
        for k in range(3):
            assert np.array_equal(second[k][sl], fresh[k][sl])           # their latest evaluation
            assert not np.array_equal(second[k][sl], first[k][sl])
        assert np.array_equal(second[3][p], fresh[3][p])


# ------------------------------------------------------------------ 5. errors
def test_errors(sgp):
    cases = _group("d8_ard")
    X, y, mu, row0, nrow = _tests(cases)
    Ps = [c["P"] for c in cases]
    b = sgp.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"]) for P in Ps])
    with pytest.raises(sgp.SGPError, match="sgp_batch_set_test first"):
        b.predict()
    b.set_test(X, None, mu, row0, nrow)
    with pytest.raises(sgp.SGPError, match="problem 0 has no posterior"):
        b.predict()
    act = np.array([1, 0], dtype=np.uint8)
    _, _, st = b.eval_vi([Ps[0]["cov_par"], None], "ard", [Ps[0]["U"], None], 1e-6, active=act)
    assert st[0] == 0
    with pytest.raises(sgp.SGPError, match="problem 1 has no posterior"):
        b.predict()
    assert b.predict(act)[1] is None and b.predict(act)[0]["pred_var"].shape == (64,)
    with pytest.raises(ValueError, match="no y_test"):
        b.score(act)
    b.set_test(X, y, mu, row0, nrow)                       # replaced: now with y
    assert b.score(act)[0]["n_nan"] == 0
    with pytest.raises(sgp.SGPError, match="leave"):
        b.set_test(X, y, mu, row0 + 1, nrow)
    assert b.score(act)[0]["n_nan"] == 0                   # a refused set_test changed nothing
    b.set_data(b.y, b.mu)                                  # the posteriors are dropped ...
    with pytest.raises(sgp.SGPError, match="problem 0 has no posterior"):
        b.predict(act)
    _, _, st = b.eval_vi([P["cov_par"] for P in Ps], "ard", [P["U"] for P in Ps], 1e-6)
    assert (st == 0).all()
    out = b.predict()                                      # ... and the test rows are not
    assert _rel(out[1]["pred_mean"], cases[1]["ref"]["pred_mean"]) < RTOL
    ms = b.predict_stage_ms(True)
    assert (ms == 0).all()
    b.score()
    ms = b.predict_stage_ms(False)
    assert ms.shape == (3,) and (ms > 0).all()
    b.close()
    for call in (b.predict, b.score, lambda: b.set_test(X, y, mu, row0, nrow)):
        with pytest.raises(RuntimeError, match="closed"):
            call()


def test_zero_row_problem(sgp):
    cases = _group("d8_ard")
    X, y, mu, row0, nrow = _tests(cases)
    nrow = np.array([0, nrow[1]])
    with _fitted(sgp, cases) as b:
        b.set_test(X, y, mu, row0, nrow)
        pm, pv, nlp, stats = _raw(b, 513, 2)
        s = b.score()
    assert (stats[0] == -123.25).all() and stats[1][1] == 513       # nothing written for no rows
    assert _rel(pm, cases[1]["ref"]["pred_mean"]) < RTOL
    assert s[0]["nlp"].size == 0 and math.isnan(s[0]["mean_nlp"]) and s[1]["n_nan"] == 0


# ------------------------------------------------------------------ 6. end to end
def test_cross_validate_end_to_end(sgp):
    S = sgp
    g = np.random.Generator(np.random.PCG64(4242))
    n, d, m = 300, 3, 10
    X = g.uniform(0.0, 10.0, size=(n, d))
    y = np.sin(X).sum(axis=1) / math.sqrt(d) + g.normal(0.0, 0.5, size=n) + 1.0
    xu = g.uniform(0.0, 10.0, size=(m, d))
    cp = OrderedDict([("sigma", 1.2), ("l", 1.7), ("tau", 0.5)])
    opt = {"maxit": 20}
    res = S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=5, opt=opt)
    assert len(res["folds"]) == 5
    assert sorted(np.concatenate([f["test_rows"] for f in res["folds"]])) == list(range(n))
    nlps, errs = [], []
    for f in res["folds"]:
        te = f["test_rows"]
        tr = np.setdiff1d(np.arange(n), te)
        mu_tr = y[tr].mean()
        s = f["score"]
        one = S.score_gp(f["model"], X[te], y[te], np.full(te.size, mu_tr), vi=True)
        assert _rel(s["pred"]["pred_mean"], one["pred"]["pred_mean"]) < RTOL
        assert _rel(s["pred"]["pred_var"], one["pred"]["pred_var"]) < RTOL
        np.testing.assert_allclose(s["nlp"], one["nlp"], rtol=1e-6, atol=1e-7)
        for key in ("median_nlp", "mean_nlp", "rmse", "srmse", "n_nan"):
            np.testing.assert_allclose(s[key], one[key], rtol=1e-6, atol=1e-7, err_msg=key)
        seq = S.optimize_gp(y[tr], X[tr], "sqexp", cp, np.full(tr.size, mu_tr), sparse=True,
                            xu_opt="fixed", xu=xu, vi=True, opt=opt)
        assert f["model"]["results"]["iter"] == seq["results"]["iter"]
        np.testing.assert_allclose(list(f["model"]["results"]["cov_par"].values()),
                                   list(seq["results"]["cov_par"].values()), rtol=1e-6, atol=1e-7)
        nlps.append(s["nlp"])
        errs.append(s["pred"]["pred_mean"].reshape(-1) - y[te])
    nlp, err = np.concatenate(nlps), np.concatenate(errs)
    assert res["mean_nlp"] == pytest.approx(nlp.mean(), rel=1e-13)
    assert res["median_nlp"] == pytest.approx(np.median(nlp), rel=1e-13)
    assert res["rmse"] == pytest.approx(np.sqrt(np.mean(err ** 2)), rel=1e-13)
    assert res["rmse"] < np.std(y)          # the fits do predict
