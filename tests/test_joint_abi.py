"""The joint-scoring and sampling entries of the C ABI and their Python wrappers, without a GPU.

Every new prototype of include/sgp.h and include/sgp_diag.h matches the ctypes table; every
SGP_EINVAL case of their argument checks returns with a message before any device call (so it
returns here, where there is no device); the Python wrappers validate shapes; my_nlp(mv = TRUE) and
my_kl(mv = TRUE) still raise, the new capability has new names.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SGP_H = ("sgp_sample_mvn", "sgp_joint_nlp", "sgp_joint_kl", "sgp_mc_nlp")
DIAG_H = ("sgp_diag_chol", "sgp_diag_normals", "sgp_diag_gemm64", "sgp_diag_sample_mvn",
          "sgp_diag_joint_nlp")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from sparsergps_amd import _lib
    return _lib.lib()


def _declared(header, name):
    """The ctypes argument list of `int name(...)` as the header declares it."""
    from sparsergps_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in {header}"
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double,
             "const double*": _lib.c_double_p, "double*": _lib.c_double_p}
    out = []
    for arg in m.group(1).split(","):
        typ = re.sub(r"\s*\b\w+\s*$", "", " ".join(arg.split()))   # drop the parameter name
        typ = typ.replace(" *", "*")
        assert typ in kinds, (name, arg)
        out.append(kinds[typ])
    return out


@pytest.mark.parametrize("header,names", [("sgp.h", SGP_H), ("sgp_diag.h", DIAG_H)])
def test_prototypes_match_the_headers(lib, header, names):
    from sparsergps_amd import _lib
    for name in names:
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int
        assert args == _declared(header, name), name
    text = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert re.search(r"#define\s+SGP_JOINT_NMAX\s+16384\b", text)
    assert "Philox4x32-10" in text and "0xD2511F53" in text and "0xBB67AE85" in text


P = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
A = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)   # noqa: E731


def _sample(lib, mean=(0.0, 0.0), cov=True, n=2, ldc=2, S=3, out=True, ldo=3):
    cov = np.eye(2) if cov is True else cov
    o = np.zeros(64) if out else None
    return lib.sgp_sample_mvn(0, P(A(mean)), P(A(cov)), n, ldc, S, 1, P(o), ldo)


def _joint(lib, family=1, y=(1.0, 0.0), pm=(0.0, 0.0), cov=True, n=2, ldc=2, par=1.0, expo=None,
           S=3, out=True):
    cov = np.eye(2) if cov is True else cov
    o = np.zeros(3) if out else None
    return lib.sgp_joint_nlp(0, family, P(A(y)), P(A(pm)), P(A(cov)), n, ldc, par, P(A(expo)), S,
                             1, P(o))


def _kl(lib, m1=(0.0, 0.0), m2=(0.0, 0.0), s1=True, s2=True, ld1=2, ld2=2, n=2, kl=True):
    s1 = np.eye(2) if s1 is True else s1
    s2 = np.eye(2) if s2 is True else s2
    o = np.zeros(1) if kl else None
    return lib.sgp_joint_kl(0, P(A(m1)), P(A(m2)), P(A(s1)), ld1, P(A(s2)), ld2, n, P(o))


def _mc(lib, y=(1.0, 0.0), pm=(0.0, 0.0), pv=(1.0, 1.0), n=2, S=3, nlp=True, mcsd=True):
    o1 = np.zeros(2) if nlp else None
    o2 = np.zeros(2) if mcsd else None
    return lib.sgp_mc_nlp(0, P(A(y)), P(A(pm)), P(A(pv)), n, S, 1, P(o1), P(o2))


BIG = 16385   # SGP_JOINT_NMAX + 1: refused before the buffers are read

EINVAL_CASES = [
    ("sample: mean NULL", _sample, dict(mean=None), "sgp_sample_mvn", "NULL"),
    ("sample: cov NULL", _sample, dict(cov=None), "sgp_sample_mvn", "NULL"),
    ("sample: out NULL", _sample, dict(out=False), "sgp_sample_mvn", "NULL"),
    ("sample: n = 0", _sample, dict(n=0), "sgp_sample_mvn", "n < 1"),
    ("sample: S = 0", _sample, dict(S=0), "sgp_sample_mvn", "S < 1"),
    ("sample: ldc < n", _sample, dict(ldc=1), "sgp_sample_mvn", "leading dimension"),
    ("sample: ldo < S", _sample, dict(ldo=2), "sgp_sample_mvn", "ldo"),
    ("sample: mean nan", _sample, dict(mean=(0.0, NAN)), "sgp_sample_mvn", "mean is not finite"),
    ("sample: mean inf", _sample, dict(mean=(INF, 0.0)), "sgp_sample_mvn", "mean is not finite"),
    ("joint: y NULL", _joint, dict(y=None), "sgp_joint_nlp", "NULL"),
    ("joint: pred_mean NULL", _joint, dict(pm=None), "sgp_joint_nlp", "NULL"),
    ("joint: pred_cov NULL", _joint, dict(cov=None), "sgp_joint_nlp", "NULL"),
    ("joint: out NULL", _joint, dict(out=False), "sgp_joint_nlp", "NULL"),
    ("joint: n = 0", _joint, dict(n=0), "sgp_joint_nlp", "n < 1"),
    ("joint: S = 0", _joint, dict(S=0), "sgp_joint_nlp", "S = 0 < 1"),
    ("joint: S < 0, poisson", _joint, dict(family=0, S=-2), "sgp_joint_nlp", "< 1"),
    ("joint: ldc < n", _joint, dict(ldc=1), "sgp_joint_nlp", "leading dimension"),
    ("joint: unknown family", _joint, dict(family=3), "sgp_joint_nlp", "unknown family 3"),
    ("joint: bernoulli y = 2", _joint, dict(y=(1.0, 2.0)), "sgp_joint_nlp", "y[1]"),
    ("joint: poisson y = 1.5", _joint, dict(family=0, y=(1.5, 2.0)), "sgp_joint_nlp",
     "non-negative integer"),
    ("joint: poisson m = 0", _joint, dict(family=0, par=0.0), "sgp_joint_nlp", "exposure"),
    ("joint: poisson expo nan", _joint, dict(family=0, expo=(1.0, NAN)), "sgp_joint_nlp",
     "expo[1]"),
    ("joint: expo with bernoulli", _joint, dict(expo=(1.0, 1.0)), "sgp_joint_nlp",
     "poisson family only"),
    ("joint: gaussian tau < 0", _joint, dict(family=2, par=-1.0), "sgp_joint_nlp", "tau"),
    ("joint: y nan", _joint, dict(family=2, y=(NAN, 0.0)), "sgp_joint_nlp", "y[0]"),
    ("joint: mean nan", _joint, dict(pm=(NAN, 0.0)), "sgp_joint_nlp", "mean is not finite"),
    ("kl: mean1 NULL", _kl, dict(m1=None), "sgp_joint_kl", "NULL"),
    ("kl: mean2 NULL", _kl, dict(m2=None), "sgp_joint_kl", "NULL"),
    ("kl: sigma1 NULL", _kl, dict(s1=None), "sgp_joint_kl", "NULL"),
    ("kl: sigma2 NULL", _kl, dict(s2=None), "sgp_joint_kl", "NULL"),
    ("kl: kl NULL", _kl, dict(kl=False), "sgp_joint_kl", "NULL"),
    ("kl: n = 0", _kl, dict(n=0), "sgp_joint_kl", "n < 1"),
    ("kl: ld1 < n", _kl, dict(ld1=1), "sgp_joint_kl", "leading dimension"),
    ("kl: ld2 < n", _kl, dict(ld2=1), "sgp_joint_kl", "leading dimension"),
    ("kl: mean1 nan", _kl, dict(m1=(NAN, 0.0)), "sgp_joint_kl", "mean is not finite"),
    ("kl: mean2 inf", _kl, dict(m2=(0.0, -INF)), "sgp_joint_kl", "mean is not finite"),
    ("mc: y NULL", _mc, dict(y=None), "sgp_mc_nlp", "NULL"),
    ("mc: pred_mean NULL", _mc, dict(pm=None), "sgp_mc_nlp", "NULL"),
    ("mc: pred_var NULL", _mc, dict(pv=None), "sgp_mc_nlp", "NULL"),
    ("mc: nlp NULL", _mc, dict(nlp=False), "sgp_mc_nlp", "NULL"),
    ("mc: mcsd NULL", _mc, dict(mcsd=False), "sgp_mc_nlp", "NULL"),
    ("mc: n = 0", _mc, dict(n=0), "sgp_mc_nlp", "n < 1"),
    ("mc: S = 0", _mc, dict(S=0), "sgp_mc_nlp", "S = 0 < 1"),
    ("mc: y = 0.5", _mc, dict(y=(0.5, 1.0)), "sgp_mc_nlp", "not 0 or 1"),
    ("mc: mean nan", _mc, dict(pm=(0.0, NAN)), "sgp_mc_nlp", "mean is not finite"),
]


@pytest.mark.parametrize("name,fn,kw,who,needle", EINVAL_CASES, ids=[c[0] for c in EINVAL_CASES])
def test_einval_before_any_device_call(lib, name, fn, kw, who, needle):
    from sparsergps_amd import _lib
    code = fn(lib, **kw)
    msg = lib.sgp_last_error().decode()
    assert code == _lib.SGP_EINVAL, (name, code, msg)
    assert msg.startswith(who) and needle in msg, msg


def test_n_above_the_limit_is_refused(lib):
    from sparsergps_amd import _lib
    z = np.zeros(BIG)
    one = np.zeros(1)
    assert lib.sgp_sample_mvn(0, P(z), P(one), BIG, BIG, 1, 0, P(one), 1) == _lib.SGP_EINVAL
    assert "above the limit 16384" in lib.sgp_last_error().decode()
    assert lib.sgp_joint_nlp(0, 2, P(z), P(z), P(one), BIG, BIG, 0.1, None, 1, 0,
                             P(np.zeros(3))) == _lib.SGP_EINVAL
    assert "above the limit 16384" in lib.sgp_last_error().decode()
    assert lib.sgp_joint_kl(0, P(z), P(z), P(one), BIG, P(one), BIG, BIG, P(one)) == _lib.SGP_EINVAL
    assert "above the limit 16384" in lib.sgp_last_error().decode()
    assert lib.sgp_diag_chol(0, P(one), BIG, BIG, P(one), BIG, P(one)) == _lib.SGP_EINVAL
    assert "above the limit 16384" in lib.sgp_last_error().decode()


def test_diag_entries_einval(lib):
    from sparsergps_amd import _lib
    a, one = np.eye(2), np.zeros(1)
    for args in ((None, 2, 2, P(a.copy()), 2, P(one)), (P(a), 0, 2, P(a.copy()), 2, P(one)),
                 (P(a), 2, 1, P(a.copy()), 2, P(one)), (P(a), 2, 2, P(a.copy()), 1, P(one)),
                 (P(a), 2, 2, None, 2, P(one)), (P(a), 2, 2, P(a.copy()), 2, None)):
        assert lib.sgp_diag_chol(0, *args) == _lib.SGP_EINVAL
        assert lib.sgp_last_error().decode().startswith("sgp_diag_chol")
    out = np.zeros(4)
    for args in ((2, 2, 2, P(out)), (0, 0, 2, P(out)), (0, 2, 0, P(out)), (1, 2, 2, None),
                 (-1, 2, 2, P(out))):
        assert lib.sgp_diag_normals(0, 5, *args) == _lib.SGP_EINVAL
        assert lib.sgp_last_error().decode().startswith("sgp_diag_normals")
    for args in ((64, 1, None), (65, 1, P(one)), (0, 1, P(one)), (64, 0, P(one)),
                 (BIG + 63, 1, P(one))):
        assert lib.sgp_diag_gemm64(0, *args) == _lib.SGP_EINVAL
        assert lib.sgp_last_error().decode().startswith("sgp_diag_gemm64")
    y, pm, o3 = np.array([1.0, 0.0]), np.zeros(2), np.zeros(3)
    for chunk, blocks in ((-1, 0), (0, -1)):
        assert lib.sgp_diag_joint_nlp(0, 1, chunk, blocks, P(y), P(pm), P(a), 2, 2, 1.0, None, 3,
                                      1, P(o3), None) == _lib.SGP_EINVAL
        assert "chunk_draws < 0 or max_blocks < 0" in lib.sgp_last_error().decode()
        assert lib.sgp_diag_sample_mvn(0, chunk, blocks, P(pm), P(a), 2, 2, 3, 1, P(np.zeros(6)),
                                       3, None) == _lib.SGP_EINVAL
        assert "chunk_draws < 0 or max_blocks < 0" in lib.sgp_last_error().decode()


def test_python_wrappers_validate_shapes():
    import sparsergps_amd as S
    y, pm, cov = np.array([1.0, 0.0, 1.0]), np.zeros(3), np.eye(3)
    with pytest.raises(ValueError, match="pred_cov must be 3 x 3"):
        S.joint_nlp(y, pm, np.eye(2), family="bernoulli", n_draws=4)
    with pytest.raises(ValueError, match="pred_cov must be 3 x 3"):
        S.joint_nlp(y, pm, np.ones(3), family="bernoulli", n_draws=4)
    with pytest.raises(ValueError, match="pred_mean has 2 values"):
        S.joint_nlp(y, pm[:2], cov, family="bernoulli", n_draws=4)
    with pytest.raises(ValueError, match="needs n_draws"):
        S.joint_nlp(y, pm, cov, family="bernoulli")
    with pytest.raises(ValueError, match="family must be"):
        S.joint_nlp(y, pm, cov, family="binomial", n_draws=4)
    with pytest.raises(ValueError, match="needs par"):
        S.joint_nlp(y, pm, cov, family="gaussian")
    with pytest.raises(ValueError, match="par\\['m'\\] has 2 values"):
        S.joint_nlp(y, pm, cov, family="poisson", par={"m": [1.0, 2.0]}, n_draws=4)
    with pytest.raises(ValueError, match="seed"):
        S.joint_nlp(y, pm, cov, family="bernoulli", n_draws=4, seed=-1)
    with pytest.raises(ValueError, match="mean2 has 2 values"):
        S.joint_kl(pm, pm[:2], cov, cov)
    with pytest.raises(ValueError, match="sigma2 must be 3 x 3"):
        S.joint_kl(pm, pm, cov, np.eye(4))
    with pytest.raises(ValueError, match="pred_mean / pred_var"):
        S.mc_nlp(y, pm, np.ones(2), 8)
    with pytest.raises(ValueError, match="cov must be 3 x 3"):
        S.sample_mvn(pm, np.eye(2), 4)
    # the library's own checks answer through the wrappers, before any device is needed
    with pytest.raises(S.SGPError, match="not 0 or 1"):
        S.joint_nlp(np.array([2.0, 0.0, 1.0]), pm, cov, family="bernoulli", n_draws=4)
    with pytest.raises(S.SGPError, match="S = 0 < 1"):
        S.mc_nlp(y, pm, np.ones(3), 0)
    with pytest.raises(S.SGPError, match="S < 1"):
        S.sample_mvn(pm, cov, 0)
    with pytest.raises(S.SGPError, match="mean is not finite"):
        S.joint_kl(np.array([0.0, NAN, 0.0]), pm, cov, cov)
    for name in ("joint_nlp", "joint_kl", "mc_nlp", "sample_mvn", "sample_gp"):
        assert name in S.__all__ and callable(getattr(S, name))


def test_score_gp_signature_keeps_joint_keyword_only():
    import inspect

    import sparsergps_amd as S
    sig = inspect.signature(S.score_gp)
    for name, default in (("joint", False), ("n_draws", None), ("seed", 0)):
        p = sig.parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default
    assert list(sig.parameters)[:6] == ["mod", "x_test", "y_test", "mu_pred", "vi", "par"]


def test_my_nlp_and_my_kl_still_refuse_mv():
    import sparsergps_amd as S
    y, pm, pv = np.array([1.0, 0.0]), np.zeros(2), np.ones(2)
    for fam, par in (("gaussian", {"tau": 0.1}), ("bernoulli", None), ("poisson", {"m": 1.0})):
        with pytest.raises(NotImplementedError, match="evaluation_functions.R"):
            S.my_nlp(y, pm, pv, family=fam, par=par, mv=True)
    with pytest.raises(NotImplementedError, match="53-65"):
        S.my_nlp(y, pm, pv, family="bernoulli", par={"n": 10}, mc=True)
    with pytest.raises(NotImplementedError, match="153-164"):
        S.my_kl(pm, pm, np.eye(2), np.eye(2), mv=True)
