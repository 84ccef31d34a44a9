"""Batched held-out prediction and scoring (sgp_batch_set_test / sgp_batch_predict, DESIGN.md sec.
0o) without a GPU: symbols, prototypes and header text, every SGP_EINVAL case
(sgp_diag_batch_test_args is the very check both entry points run before their first device call),
NULL handles, the test-segment plan and the packing offsets, the loud failure without a device,
and cross_validate_gp's host logic on a fake batch that evaluates and predicts with the CPU
oracle."""
import ctypes as C
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

from oracle import sgp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"sgp_batch_set_test": 8, "sgp_batch_predict": 6, "sgp_diag_batch_test_args": 18,
         "sgp_diag_batch_test_plan": 9, "sgp_diag_batch_predict_timing": 3}


@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    return _lib.lib()


def _decl_commas(text, name):
    decl = re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", text[text.index(f"int {name}("):]))
    return decl[:decl.index(";")].count(",")


def test_symbols_prototypes_and_header(lib):
    from sparsergps_amd import _lib
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    diag = open(os.path.join(ROOT, "include", "sgp_diag.h")).read()
    for name, n in NARGS.items():
        assert hasattr(lib, name), name
        assert _lib.PROTOTYPES[name][0] is C.c_int and len(_lib.PROTOTYPES[name][1]) == n, name
        src = diag if name.startswith("sgp_diag_") else text
        assert _decl_commas(src, name) == n - 1, name
    # declared after sgp_batch_posterior_u, documented with the two reference locations
    assert text.index("int sgp_batch_posterior_u(") < text.index("int sgp_batch_set_test(") < \
        text.index("int sgp_batch_predict(")
    doc = text[text.index("Held-out prediction and scoring for a batch"):
               text.index("int sgp_batch_set_test(")]
    for cite in ("vi_functions.R:1222-1336", "evaluation_functions.R:14-20"):
        assert cite in doc, cite
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", text) and lib.sgp_abi_version() == 1


def _good(B=3, d=2, nt=40):
    g = np.random.default_rng(0)
    return {"stage": 0, "d": d, "B": B, "Xt": np.asfortranarray(g.uniform(size=(nt, d))),
            "ntest": nt, "ldxt": nt, "yt": g.normal(size=nt), "mut": np.zeros(nt),
            "trow0": np.array([0, 7, 0][:B], dtype=np.int64),
            "tnrow": np.array([40, 33, 0][:B], dtype=np.int64),
            "have_test": 1, "have_yt": 1, "has_state": np.ones(B, dtype=np.uint8), "active": None,
            "pred_mean": np.zeros(73), "pred_var": np.zeros(73), "nlp": np.zeros(73),
            "stats": np.zeros(4 * B)}


def _check(lib, a):
    from sparsergps_amd import _lib
    p = lambda v: None if v is None else _lib.dptr(v)   # noqa: E731
    q = lambda v: None if v is None else v.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    u = lambda v: None if v is None else v.ctypes.data_as(_lib.c_ubyte_p)   # noqa: E731
    return lib.sgp_diag_batch_test_args(
        a["stage"], a["d"], a["B"], p(a["Xt"]), a["ntest"], a["ldxt"], p(a["yt"]), p(a["mut"]),
        q(a["trow0"]), q(a["tnrow"]), a["have_test"], a["have_yt"], u(a["has_state"]),
        u(a["active"]), p(a["pred_mean"]), p(a["pred_var"]), p(a["nlp"]), p(a["stats"]))


def test_good_arguments_pass(lib):
    from sparsergps_amd import _lib
    assert _check(lib, _good()) == _lib.SGP_OK
    assert _check(lib, {**_good(), "yt": None}) == _lib.SGP_OK             # predict only
    assert _check(lib, {**_good(), "stage": 1}) == _lib.SGP_OK
    assert _check(lib, {**_good(), "stage": 1, "nlp": None, "stats": None}) == _lib.SGP_OK
    # a non-finite mut entry is data, not an error
    a = _good()
    a["mut"][3] = np.inf
    a["mut"][4] = np.nan
    assert _check(lib, a) == _lib.SGP_OK
    # aliased ranges; stage 1 reads none of set_test's arguments
    assert _check(lib, {**_good(), "trow0": np.zeros(3, dtype=np.int64),
                        "tnrow": np.full(3, 40, dtype=np.int64)}) == _lib.SGP_OK
    assert _check(lib, {**_good(), "stage": 1, "Xt": None, "mut": None, "trow0": None,
                        "tnrow": None, "ntest": 0}) == _lib.SGP_OK
    # an inactive problem needs no posterior
    assert _check(lib, {**_good(), "stage": 1, "has_state": np.array([1, 0, 1], dtype=np.uint8),
                        "active": np.array([1, 0, 1], dtype=np.uint8)}) == _lib.SGP_OK


def _with(key, idx, val):
    a = _good()
    a[key] = a[key].copy(order="K")
    a[key][idx] = val
    return {key: a[key]}


BAD = {
    "Xt NULL": ({"Xt": None}, b"NULL"),
    "mut NULL": ({"mut": None}, b"NULL"),
    "trow0 NULL": ({"trow0": None}, b"NULL"),
    "tnrow NULL": ({"tnrow": None}, b"NULL"),
    "ntest = 0": ({"ntest": 0}, b"ntest=0"),
    "ldxt < ntest": ({"ldxt": 39}, b"ldxt=39"),
    "tnrow < 0": (_with("tnrow", 1, -1), b"problem 1 has tnrow=-1"),
    "range past the end": (_with("trow0", 1, 8), b"leave [0, 40)"),
    "range before the start": (_with("trow0", 2, -1), b"leave [0, 40)"),
    "Xt NaN": (_with("Xt", (5, 1), np.nan), b"Xt[5, 1]"),
    "Xt inf": (_with("Xt", (0, 0), np.inf), b"Xt[0, 0]"),
    "yt NaN": (_with("yt", 9, np.nan), b"yt[9]"),
    "yt inf": (_with("yt", 39, -np.inf), b"yt[39]"),
    "stage": ({"stage": 2}, b"stage"),
    "pred_mean NULL": ({"stage": 1, "pred_mean": None}, b"NULL"),
    "pred_var NULL": ({"stage": 1, "pred_var": None}, b"NULL"),
    "predict before set_test": ({"stage": 1, "have_test": 0}, b"sgp_batch_set_test first"),
    "nlp without yt": ({"stage": 1, "have_yt": 0}, b"yt = NULL"),
    "nlp without stats": ({"stage": 1, "stats": None}, b"both"),
    "stats without nlp": ({"stage": 1, "nlp": None}, b"both"),
    "no posterior": ({"stage": 1, "has_state": np.array([1, 0, 0], dtype=np.uint8)},
                     b"problem 1 has no posterior"),
    "no posterior, masked": ({"stage": 1, "has_state": np.array([1, 0, 0], dtype=np.uint8),
                              "active": np.array([1, 0, 1], dtype=np.uint8)},
                             b"problem 2 has no posterior"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_einval_before_any_device_call(lib, name):
    from sparsergps_amd import _lib
    change, needle = BAD[name]
    assert _check(lib, {**_good(), **change}) == _lib.SGP_EINVAL
    assert needle in lib.sgp_last_error(), lib.sgp_last_error()


def test_null_handles(lib):
    from sparsergps_amd import _lib
    a = _good()
    q = lambda w: w.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    st = lib.sgp_batch_set_test(None, _lib.dptr(a["Xt"]), 40, 40, _lib.dptr(a["yt"]),
                                _lib.dptr(a["mut"]), q(a["trow0"]), q(a["tnrow"]))
    assert st == _lib.SGP_EINVAL and b"sgp_batch_set_test" in lib.sgp_last_error()
    st = lib.sgp_batch_predict(None, None, _lib.dptr(a["pred_mean"]), _lib.dptr(a["pred_var"]),
                               None, None)
    assert st == _lib.SGP_EINVAL and b"sgp_batch_predict" in lib.sgp_last_error()
    assert lib.sgp_diag_batch_predict_timing(None, 1, None) == _lib.SGP_EINVAL
    assert b"sgp_diag_batch_predict_timing" in lib.sgp_last_error()


def _plan(lib, trow0, tnrow):
    from sparsergps_amd import _lib
    r0 = np.asarray(trow0, dtype=np.int64)
    nr = np.asarray(tnrow, dtype=np.int64)
    q = lambda v: v.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    nseg = C.c_int64(-1)
    assert lib.sgp_diag_batch_test_plan(q(r0), q(nr), r0.size, 0, C.byref(nseg), None, None, None,
                                        None) == _lib.SGP_OK
    k = nseg.value
    sp, s0, sr = (np.full(k + 2, -7, dtype=np.int64) for _ in range(3))
    toff = np.full(r0.size + 1, -7, dtype=np.int64)
    assert lib.sgp_diag_batch_test_plan(q(r0), q(nr), r0.size, k, C.byref(nseg), q(sp), q(s0),
                                        q(sr), q(toff)) == _lib.SGP_OK
    assert nseg.value == k and (sp[k:] == -7).all() and (sr[k:] == -7).all()
    return sp[:k], s0[:k], sr[:k], toff


def test_test_plan_and_packing(lib):
    from sparsergps_amd import _lib
    diag = open(os.path.join(ROOT, "include", "sgp_diag.h")).read()
    seg = int(re.search(r"#define\s+SGP_BATCH_SEG_ROWS\s+(\d+)", diag).group(1))
    assert seg == 512
    trow0, tnrow = [3, 5, 37, 1], [0, 1, 512, 513]
    sp, s0, sr, toff = _plan(lib, trow0, tnrow)
    assert [int((sp == b).sum()) for b in range(4)] == [0, 1, 1, 2]      # no segment for 0 rows
    assert list(sr) == [1, 512, 512, 1] and list(s0) == [5, 37, 1, 513]
    assert list(toff) == [0, 0, 1, 513, 1026]
    # a problem's segments are its own: the same alone, and behind other problems
    for b in range(1, 4):
        sp1, s01, sr1, toff1 = _plan(lib, [trow0[b]], [tnrow[b]])
        assert (s01 == s0[sp == b]).all() and (sr1 == sr[sp == b]).all()
        assert list(toff1) == [0, tnrow[b]]
    rsp, rs0, rsr, rtoff = _plan(lib, trow0[::-1], tnrow[::-1])
    assert list(rtoff) == [0, 513, 1025, 1026, 1026]
    for b in range(4):
        assert (rs0[rsp == 3 - b] == s0[sp == b]).all() and (rsr[rsp == 3 - b] == sr[sp == b]).all()
    # aliased ranges are packed separately
    assert list(_plan(lib, [0, 0], [10, 10])[3]) == [0, 10, 20]
    # all-empty: no segment at all
    assert _plan(lib, [0, 0], [0, 0])[0].size == 0
    one = np.array([0], dtype=np.int64)
    q = lambda v: v.ctypes.data_as(_lib.c_int64_p)   # noqa: E731
    n = C.c_int64(0)
    assert lib.sgp_diag_batch_test_plan(q(one), q(one - 1), 1, 0, C.byref(n), None, None, None,
                                        None) == _lib.SGP_EINVAL
    assert b"sgp_diag_batch_test_plan" in lib.sgp_last_error()
    assert lib.sgp_diag_batch_test_plan(None, q(one), 1, 0, C.byref(n), None, None, None,
                                        None) == _lib.SGP_EINVAL
    assert lib.sgp_diag_batch_test_plan(q(one), q(one + 1), 1, 2, C.byref(n), None, None, None,
                                        None) == _lib.SGP_EINVAL


def _cv_data(n=60, d=2, seed=3):
    g = np.random.Generator(np.random.PCG64(seed))
    X = g.uniform(0.0, 10.0, size=(n, d))
    y = np.sin(X).sum(axis=1) / np.sqrt(d) + g.normal(0.0, 0.5, size=n) + 2.0
    xu = g.uniform(0.0, 10.0, size=(5, d))
    cp = OrderedDict([("sigma", 1.2), ("l", 1.7), ("tau", 0.5)])
    return X, y, xu, cp


def test_no_gpu_no_fallback():
    """Without a HIP device cross_validate_gp raises SGPError from the batch it creates: there is
    no CPU path behind it."""
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    n = C.c_int(0)
    if _lib.lib().sgp_device_count(C.byref(n)) == _lib.SGP_OK and n.value > 0:
        return                                            # the GPU suite covers the rest
    X, y, xu, cp = _cv_data()
    with pytest.raises(S.SGPError, match="no HIP device"):
        S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=3, opt={"maxit": 2, "maxknot": 5})


def test_python_surface_exists():
    import sparsergps_amd as S
    assert callable(S.cross_validate_gp) and "cross_validate_gp" in S.__all__
    for meth in ("set_test", "set_test_problems", "predict", "score", "predict_stage_ms",
                 "predict_raw"):
        assert callable(getattr(S.SparseGPBatch, meth))


# ------------------------------------------------------------------ cross_validate_gp's host logic
class FakeBatch:
    """What cross_validate_gp and norm_grad_ascent_vi_batch use of a SparseGPBatch, evaluated and
    predicted by the CPU oracle."""
    made = []

    def __init__(self, problems):
        self.problems, self.B = problems, len(problems)
        self.last = [None] * self.B
        self.tests = self.scored = None
        self.closed = False
        FakeBatch.made.append(self)

    @classmethod
    def from_problems(cls, problems, device=None):
        return cls([(np.asarray(p[0]), np.asarray(p[1]), np.asarray(p[2])) for p in problems])

    def rows(self, b):
        return self.problems[b]

    def eval_vi(self, cov_pars, cov_fun, xus, delta=1e-6, active=None, obj_only=False,
                r_det=False):
        obj, grads = np.full(self.B, np.nan), [None] * self.B
        for b, (xy, y, mu) in enumerate(self.problems):
            if active is not None and not active[b]:
                continue
            obj[b] = O.elbo_eval(cov_pars[b], cov_fun, xus[b], xy, y, mu, delta)
            grads[b] = O.delbo_dcov_par(cov_pars[b], cov_fun, xus[b], xy, y, mu, delta)["gradient"]
            self.last[b] = (OrderedDict(cov_pars[b]), cov_fun, np.array(xus[b]), delta)
        return obj, grads, np.zeros(self.B, dtype=np.int32)

    def _post(self, b, muu):
        cp, cf, xu, dl = self.last[b]
        return O.vi_posterior_u(cp, cf, xu, *self.problems[b], muu, dl)

    def posterior_u(self, muus):
        res = [self._post(b, muus[b]) for b in range(self.B)]
        return [r[0] for r in res], [r[1] for r in res]

    def set_test_problems(self, tests):
        self.tests = tests

    def score(self, active=None):
        self.scored = None if active is None else np.array(active)
        out = []
        for b, (xt, yt, mut) in enumerate(self.tests):
            if active is not None and not active[b]:
                out.append(None)
                continue
            cp, cf, xu, dl = self.last[b]
            muu = np.zeros(xu.shape[0])
            um, uv = self._post(b, muu)
            pr = O.predict_vi(um, uv, xu, xt, cf, cp, mut, muu, False, dl)
            v = pr["pred_var"] + cp["tau"] ** 2
            nlp = 0.5 * np.log(2 * np.pi * v) + (yt - pr["pred_mean"]) ** 2 / (2 * v)
            rmse = float(np.sqrt(np.mean((pr["pred_mean"] - yt) ** 2)))
            out.append({"pred": {"pred_mean": pr["pred_mean"].reshape(-1, 1),
                                 "pred_var": pr["pred_var"]}, "nlp": nlp,
                        "median_nlp": float(np.median(nlp)), "mean_nlp": float(nlp.mean()),
                        "rmse": rmse, "srmse": rmse / float(np.std(yt, ddof=1)), "n_nan": 0})
        return out

    def close(self):
        self.closed = True


@pytest.fixture
def fake(monkeypatch):
    import sparsergps_amd.batch as SB
    FakeBatch.made = []
    monkeypatch.setattr(SB, "SparseGPBatch", FakeBatch)
    return FakeBatch


OPT = {"maxit": 3, "maxknot": 5}


def test_cross_validate_folds_from_an_integer(fake):
    import sparsergps_amd as S
    X, y, xu, cp = _cv_data()
    res = S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=4, opt=OPT)
    assert set(res) == {"folds", "mean_nlp", "median_nlp", "rmse", "fold_id"}
    assert len(res["folds"]) == 4 and res["fold_id"].shape == (60,)
    assert sorted(np.bincount(res["fold_id"])) == [15, 15, 15, 15]
    # every row is held out exactly once, by the fold its id names
    held = np.concatenate([f["test_rows"] for f in res["folds"]])
    assert sorted(held) == list(range(60))
    for k, f in enumerate(res["folds"]):
        assert (res["fold_id"][f["test_rows"]] == k).all()
        assert set(f) == {"model", "score", "test_rows"}
        assert set(f["model"]) == {"results", "sparse", "family", "delta", "xu_init"}
        assert f["model"]["sparse"] is True and f["model"]["family"] == "gaussian"
        assert set(f["score"]) == {"pred", "nlp", "median_nlp", "mean_nlp", "rmse", "srmse", "n_nan"}
        assert f["model"]["results"]["iter"] == 3 and f["model"]["results"]["u_mean"] is not None
    # the default partition is np.random.default_rng(0)'s; another generator gives another one
    again = S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=4, opt=OPT)
    other = S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=4, opt=OPT,
                                rng=np.random.default_rng(5))
    assert np.array_equal(again["fold_id"], res["fold_id"])
    assert not np.array_equal(other["fold_id"], res["fold_id"])
    # one batch, the fit's problems are the other folds' rows, and it is closed afterwards
    b = fake.made[0]
    assert len(fake.made) == 3 and b.closed and b.B == 4 and (b.scored == 1).all()
    for k, f in enumerate(res["folds"]):
        train = np.setdiff1d(np.arange(60), f["test_rows"])
        assert np.array_equal(b.problems[k][0], X[train]) and np.array_equal(b.problems[k][1], y[train])
        assert np.array_equal(b.tests[k][0], X[f["test_rows"]])
        assert np.array_equal(b.tests[k][1], y[f["test_rows"]])
        # mu = None: the fold's training mean, for the training rows and for the held-out rows
        assert np.array_equal(b.problems[k][2], np.full(45, y[train].mean()))
        assert np.array_equal(b.tests[k][2], np.full(15, y[train].mean()))
    # the pooled figures are numpy's over the concatenated held-out rows
    nlp = np.concatenate([f["score"]["nlp"] for f in res["folds"]])
    err = np.concatenate([f["score"]["pred"]["pred_mean"].reshape(-1) - y[f["test_rows"]]
                          for f in res["folds"]])
    assert res["mean_nlp"] == pytest.approx(nlp.mean(), rel=1e-14)
    assert res["median_nlp"] == pytest.approx(np.median(nlp), rel=1e-14)
    assert res["rmse"] == pytest.approx(np.sqrt(np.mean(err ** 2)), rel=1e-14)


def test_cross_validate_folds_from_ids_and_mu_array(fake):
    import sparsergps_amd as S
    X, y, xu, cp = _cv_data()
    ids = np.array(([7] * 10 + [2] * 25 + [4] * 25))          # any labels, unequal sizes
    mu = np.linspace(1.0, 3.0, 60)
    g = np.random.Generator(np.random.PCG64(11))
    xus = [g.uniform(0.0, 10.0, size=(m, 2)) for m in (4, 5, 3)]
    cps = [OrderedDict(cp, sigma=1.0 + 0.1 * k) for k in range(3)]
    res = S.cross_validate_gp(y, X, "sqexp", cps, xus, folds=ids, mu=mu, opt=OPT)
    assert np.array_equal(res["fold_id"], ids)
    assert [list(f["test_rows"]) for f in res["folds"]] == \
        [list(range(10, 35)), list(range(35, 60)), list(range(10))]       # sorted labels 2, 4, 7
    b = fake.made[0]
    for k, f in enumerate(res["folds"]):
        train = np.setdiff1d(np.arange(60), f["test_rows"])
        assert np.array_equal(b.problems[k][2], mu[train])               # an array mu is split
        assert np.array_equal(b.tests[k][2], mu[f["test_rows"]])
        assert f["model"]["results"]["xu"].shape == xus[k].shape          # one knot set per fold
        assert f["model"]["results"]["cov_par_history"][0][0] == cps[k]["sigma"]
        assert np.array_equal(f["model"]["xu_init"], xus[k])
    with pytest.raises(ValueError, match="fold ids"):
        S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=ids[:-1], opt=OPT)
    with pytest.raises(ValueError, match="one per fold"):
        S.cross_validate_gp(y, X, "sqexp", cps[:2], xu, folds=ids, opt=OPT)
    with pytest.raises(ValueError, match="fewer than two"):
        S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=np.zeros(60, dtype=int), opt=OPT)


def test_cross_validate_refusals(fake):
    import sparsergps_amd as S
    X, y, xu, cp = _cv_data()
    ones = S.optimize_gp_batch([(X, y, None)], "sqexp", cp, xu, opt={"optim_method": "ga"})
    assert S.cross_validate_gp(y, X, "sqexp", cp, xu, opt={"optim_method": "ga"}) == ones[0]
    assert S.cross_validate_gp(y, X, "exp", cp, xu, opt=OPT) == \
        S.optimize_gp_batch([(X, y, None)], "exp", cp, xu)[0]
    # maxknot >= a fold's training rows: 60 rows in 4 folds train on 45
    assert S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=4, opt={"maxknot": 45}) == \
        S.optimize_gp_batch([(X[:45], y[:45], None)], "sqexp", cp, xu, opt={"maxknot": 45})[0]
    assert not fake.made                                               # refused before any batch
    with pytest.raises(ValueError, match="folds=1"):
        S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=1, opt=OPT)


def test_cross_validate_skips_a_fold_that_failed(fake, monkeypatch):
    """A fold whose fit retires with an error carries that error as its score, is not scored, and
    stays out of the pooled figures."""
    import sparsergps_amd as S
    import sparsergps_amd.batch as SB
    X, y, xu, cp = _cv_data()
    real = SB.norm_grad_ascent_vi_batch

    def failing(*a, **k):
        res = real(*a, **k)
        res[1]["error"] = SB._not_pd(4)
        return res

    monkeypatch.setattr(SB, "norm_grad_ascent_vi_batch", failing)
    res = S.cross_validate_gp(y, X, "sqexp", cp, xu, folds=3, opt=OPT)
    assert isinstance(res["folds"][1]["score"], S.NotPositiveDefinite)
    assert list(fake.made[0].scored) == [1, 0, 1]
    nlp = np.concatenate([res["folds"][k]["score"]["nlp"] for k in (0, 2)])
    assert res["mean_nlp"] == pytest.approx(nlp.mean(), rel=1e-14)
