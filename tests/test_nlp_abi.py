"""The scoring entries of the C ABI and the host side of sparsergps_amd.evaluation, without a GPU.

sgp_nlp and sgp_predict_nlp are declared and exported; every SGP_EINVAL case of their argument
checks returns before any device call (so it returns here, where there is no device);
SGP_FAM_GAUSSIAN is still refused by sgp_lap_set_family; my_rmse and my_kl agree with the
reference as written; my_nlp's mc / mv branches answer as documented.
"""
import os
import re

import numpy as np
import pytest

import nlp_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    return _lib.lib()


def test_header_declares_and_library_exports(lib):
    from sparsergps_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp.h")).read(), flags=re.S)
    for name in ("sgp_nlp", "sgp_predict_nlp"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert re.search(r"SGP_FAM_GAUSSIAN\s*=\s*2", text)
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", text) and lib.sgp_abi_version() == 1
    assert _lib.SCORE_FAMILIES == {"poisson": 0, "bernoulli": 1, "gaussian": 2}


def _nlp(lib, family, y, pm=None, pv=None, par=1.0, expo=None, n=None, nlp=True, stats=True):
    from sparsergps_amd import _lib
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    k = 3 if y is None else y.size
    pm = np.zeros(k) if pm is None else pm
    pv = np.ones(k) if pv is None else pv
    out, st = np.zeros(k), np.zeros(4)
    p = lambda a: None if a is None or a is False else _lib.dptr(a)   # noqa: E731
    code = lib.sgp_nlp(0, family, p(y), p(pm), p(pv), k if n is None else n, par,
                       p(None if expo is None else np.ascontiguousarray(expo, dtype=np.float64)),
                       p(out if nlp else None), p(st if stats else None))
    return code, lib.sgp_last_error().decode()


EINVAL_CASES = [
    ("y NULL", dict(family=0, y=None), "NULL"),
    ("pred_mean NULL", dict(family=0, y=[1.0], pm=False), "NULL"),
    ("pred_var NULL", dict(family=0, y=[1.0], pv=False), "NULL"),
    ("nlp NULL", dict(family=0, y=[1.0], nlp=False), "NULL"),
    ("stats NULL", dict(family=0, y=[1.0], stats=False), "NULL"),
    ("n = 0", dict(family=0, y=[1.0], n=0), "n < 1"),
    ("n < 0", dict(family=1, y=[1.0], n=-4), "n < 1"),
    ("unknown family", dict(family=3, y=[1.0]), "unknown family 3"),
    ("negative family", dict(family=-1, y=[1.0]), "unknown family"),
    ("bernoulli y = 2", dict(family=1, y=[0.0, 1.0, 2.0]), "y[2]"),
    ("bernoulli y = 0.5", dict(family=1, y=[0.5]), "not 0 or 1"),
    ("poisson y < 0", dict(family=0, y=[3.0, -1.0]), "y[1]"),
    ("poisson y not an integer", dict(family=0, y=[2.5]), "non-negative integer"),
    ("poisson m = 0", dict(family=0, y=[1.0], par=0.0), "exposure"),
    ("poisson m < 0", dict(family=0, y=[1.0], par=-2.0), "exposure"),
    ("poisson m = inf", dict(family=0, y=[1.0], par=float("inf")), "exposure"),
    ("poisson m = nan", dict(family=0, y=[1.0], par=float("nan")), "exposure"),
    ("poisson expo row 0", dict(family=0, y=[1.0, 2.0], expo=[1.0, 0.0]), "expo[1]"),
    ("poisson expo nan", dict(family=0, y=[1.0, 2.0], expo=[float("nan"), 1.0]), "expo[0]"),
    ("expo with bernoulli", dict(family=1, y=[1.0], expo=[1.0]), "poisson family only"),
    ("gaussian tau < 0", dict(family=2, y=[1.0], par=-0.1), "tau"),
    ("gaussian tau nan", dict(family=2, y=[1.0], par=float("nan")), "tau"),
    ("gaussian tau inf", dict(family=2, y=[1.0], par=float("inf")), "tau"),
    ("y nan", dict(family=2, y=[0.0, float("nan")], par=0.1), "y[1]"),
    ("y inf, poisson", dict(family=0, y=[float("inf")]), "not finite"),
    ("y -inf, bernoulli", dict(family=1, y=[-float("inf")]), "not finite"),
]


@pytest.mark.parametrize("name,kw,needle", EINVAL_CASES, ids=[c[0] for c in EINVAL_CASES])
def test_sgp_nlp_einval_before_any_device_call(lib, name, kw, needle):
    from sparsergps_amd import _lib
    code, msg = _nlp(lib, **kw)
    assert code == _lib.SGP_EINVAL, (name, code, msg)
    assert msg.startswith("sgp_nlp") and needle in msg, msg


def test_sgp_predict_nlp_einval_before_any_device_call(lib):
    from sparsergps_amd import _lib
    d, m, npred = 2, 4, 3
    th = np.array([1.0, 1.0, 0.5])
    U = np.asfortranarray(np.arange(m * d, dtype=np.float64).reshape(m, d))
    xp = np.asfortranarray(np.ones((npred, d)))
    um, muu, uv = np.zeros(m), np.zeros(m), np.asfortranarray(np.eye(m))
    mup, pm, pv, nlp = (np.zeros(npred) for _ in range(4))
    st = np.zeros(4)
    P = _lib.dptr

    def call(family, y, par=1.0, expo=None, kernel=0, npp=npred):
        y = np.ascontiguousarray(y, dtype=np.float64)
        return lib.sgp_predict_nlp(0, kernel, P(th), 1e-6, _lib.SGP_PRED_LAPLACE, 0, P(U), m, m,
                                   P(um), P(muu), P(uv), m, P(xp), npp, npred, d, P(mup), P(pm),
                                   P(pv), family, P(y), par,
                                   None if expo is None else P(np.ascontiguousarray(expo)),
                                   P(nlp), P(st))

    for args, needle in ((dict(family=1, y=[0, 1, 3]), "y[2]"),
                         (dict(family=0, y=[0, 1.5, 3]), "y[1]"),
                         (dict(family=0, y=[0, 1, 3], par=0.0), "exposure"),
                         (dict(family=2, y=[0, 1, 3], par=-1.0), "tau"),
                         (dict(family=9, y=[0, 1, 3]), "unknown family"),
                         (dict(family=0, y=[0, 1, 3], npp=0), "n < 1")):
        assert call(**args) == _lib.SGP_EINVAL, args
        msg = lib.sgp_last_error().decode()
        assert msg.startswith("sgp_predict_nlp") and needle in msg, msg
    # the prediction's own checks still answer (the 'exp' kernel has no fitted posterior)
    assert call(family=0, y=[0, 1, 3], kernel=2) == _lib.SGP_EINVAL
    assert "prediction supports" in lib.sgp_last_error().decode()


def test_lap_set_family_still_refuses_gaussian(lib):
    from sparsergps_amd import _lib
    assert lib.sgp_lap_set_family(None, 2) == _lib.SGP_EINVAL


def test_my_rmse_and_my_kl_against_the_reference_as_written():
    import sparsergps_amd as S
    rng = np.random.default_rng(11)
    n = 7
    m1, m2 = rng.normal(size=n), rng.normal(size=n)
    s1, s2 = rng.uniform(0.1, 3.0, n), rng.uniform(0.1, 3.0, n)
    ref = NO.literal_kl(m1, m2, s1, s2)
    got = S.my_kl(m1.reshape(-1, 1), m2.reshape(-1, 1), s1, s2)
    assert abs(got - ref) <= 1e-14 * max(1.0, abs(ref))
    assert abs(S.my_rmse(m1.reshape(-1, 1), m2.reshape(-1, 1)) - NO.literal_rmse(m1, m2)) <= 1e-15
    with pytest.raises(NotImplementedError, match="153-164"):
        S.my_kl(m1, m2, np.eye(n), np.eye(n), mv=True)


def test_my_nlp_mc_and_mv_branches():
    import sparsergps_amd as S
    y, pm, pv = np.array([1.0, 0.0]), np.zeros(2), np.ones(2)
    assert S.my_nlp(y, pm, pv, family="poisson", par={"m": 1.0, "n": 10}, mc=True) == \
        "Error: Monte Carlo estimate of marginal NLP for Poisson data must be fixed."
    with pytest.raises(NotImplementedError, match="53-65"):
        S.my_nlp(y, pm, pv, family="bernoulli", par={"n": 10}, mc=True)
    for fam, par in (("gaussian", {"tau": 0.1}), ("bernoulli", None), ("poisson", {"m": 1.0})):
        with pytest.raises(NotImplementedError, match="evaluation_functions.R"):
            S.my_nlp(y, pm, pv, family=fam, par=par, mv=True)
    with pytest.raises(ValueError):
        S.my_nlp(y, pm, pv, family="binomial")
    # a bad response is the library's SGP_EINVAL, raised before any device is needed
    with pytest.raises(S.SGPError, match="not 0 or 1"):
        S.my_nlp(np.array([2.0]), pm[:1], pv[:1], family="bernoulli")
