"""Leading dimensions of the C ABI (include/sgp.h): ldx, ldxp, ldo, ldu, ldv, ldc, ldpv.

Every caller in the repository (the Python wrappers, the R shim) passes ld = rows, so these are
raw ctypes calls on libsgp.  For each matrix argument: the matrix sits in a buffer with
ld = rows + 3 whose padding rows are NaN (inputs) or a sentinel (outputs); the call must give
results BIT-identical to the packed call (ld = rows) -- the device layout does not depend on
the host stride, so not one ulp may move -- leave the output padding untouched, and refuse
ld = rows - 1 with SGP_EINVAL.  A NaN that leaks in from the padding poisons the result; a read
at the wrong stride changes it.

Covers the host packing loops of the fillers, sgp_ctx_create, sgp_predict and the candidate
scorers, the knot cache's comparison in upload_knots (same knots at another stride must hit,
other knots must miss) and the per-shard X + row0 of sgp_ctx_create_multi.
Sizes: n = 300, m = 20, d = 3, np = 70, T = 3.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, M, D, NP, T = 300, 20, 3, 70, 3
PAD = 3
SENTINEL = -3.0e300
DELTA = 1e-6
THETA = {"sqexp": np.array([1.2, 1.7, 0.5]), "ard": np.array([1.2, 1.7, 1.95, 2.2, 0.5])}


@pytest.fixture(scope="module")
def L():
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def data():
    g = np.random.Generator(np.random.PCG64(314))
    X = g.uniform(0.0, 10.0, size=(N, D))
    U = g.uniform(0.0, 10.0, size=(M, D))
    U[4] = X[17]                                   # a knot equal to a data row (tau's rule)
    U2 = g.uniform(0.0, 10.0, size=(M, D))
    xp = g.uniform(0.0, 10.0, size=(NP, D))
    xp[0] = U[2]
    cand = g.uniform(0.0, 10.0, size=(T, D))
    y = np.sin(X).sum(axis=1) / math.sqrt(D) + g.normal(0.0, 0.5, size=N)
    lam = np.exp(0.5 * np.sin(X).sum(axis=1) / math.sqrt(D) + math.log(2.0))
    yp = g.poisson(lam).astype(np.float64)
    A = g.normal(0.0, 1.0, size=(M, M))
    return dict(X=X, U=U, U2=U2, xp=xp, cand=cand, y=y, mu=np.full(N, y.mean()), yp=yp,
                mup=np.full(N, math.log(yp.mean())), u_var=0.07 * (A @ A.T) / M,
                u_mean=0.3 + g.normal(0.0, 0.5, size=M), muu=np.full(M, 0.3),
                mu_pred=0.25 + 0.1 * np.sin(np.arange(NP)))


def _mat(a, strided, fill=np.nan):
    """(buffer, ld): `a` column-major, packed or inside an ld = rows + PAD buffer whose
    padding rows hold `fill`."""
    a = np.asarray(a, dtype=np.float64)
    rows, cols = a.shape
    ld = rows + PAD if strided else rows
    buf = np.full((ld, cols), fill, dtype=np.float64, order="F")
    buf[:rows] = a
    return buf, ld


def _out(rows, cols, strided):
    ld = rows + PAD if strided else rows
    return np.full((ld, cols), SENTINEL, dtype=np.float64, order="F"), ld


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check_out(buf, rows, packed):
    assert np.all(buf[rows:] == SENTINEL), "output padding rows were written"
    assert not np.any(buf[:rows] == SENTINEL), "output entries left unwritten"
    assert _same_bits(buf[:rows], packed[:rows])


# ----------------------------------------------------------------------------- fillers
def _fill(L, fn, kernel, x, ldx, xp, ldxp, out, ldo, param):
    lib = L.lib()
    th = THETA[kernel]
    xpp = None if xp is None else L.dptr(xp)
    k = L.KERNELS[kernel]
    if fn == "cov":
        return lib.sgp_make_cov(0, k, L.dptr(x), N, ldx, xpp, 0 if xp is None else NP, ldxp, D,
                                L.dptr(th), DELTA, L.dptr(out), ldo)
    return lib.sgp_dsig_dtheta(0, k, L.dptr(x), N, ldx, xpp, 0 if xp is None else NP, ldxp, D,
                               L.dptr(th), param, L.dptr(out), ldo)


@pytest.mark.parametrize("kernel", ["sqexp", "ard"])
@pytest.mark.parametrize("mode", ["cross", "sym"])
@pytest.mark.parametrize("fn", ["cov", "dsig"])
def test_filler_leading_dimensions(L, data, fn, mode, kernel):
    cols = NP if mode == "cross" else N
    Xd = data["X"].copy()
    Xd[5] = data["xp"][5]                          # a coincident pair in cross mode
    names = ("ldx", "ldxp", "ldo") if mode == "cross" else ("ldx", "ldo")
    params = [0] if fn == "cov" else [1, THETA[kernel].size - 1]     # a length scale, tau
    for param in params:
        def run(which):
            x, ldx = _mat(Xd, "ldx" in which)
            xp, ldxp = _mat(data["xp"], "ldxp" in which) if mode == "cross" else (None, 0)
            out, ldo = _out(N, cols, "ldo" in which)
            assert _fill(L, fn, kernel, x, ldx, xp, ldxp, out, ldo, param) == L.SGP_OK, \
                L.lib().sgp_last_error()
            return out
        packed = run(())
        assert np.all(np.isfinite(packed))
        for which in [names] + [(nm,) for nm in names]:
            _check_out(run(which), N, packed)
        for short in names:                        # ld = rows - 1
            x, ldx = _mat(Xd, False)
            xp, ldxp = _mat(data["xp"], False) if mode == "cross" else (None, 0)
            out, ldo = _out(N, cols, False)
            ldx, ldxp, ldo = (ldx - (short == "ldx"), ldxp - (short == "ldxp"),
                              ldo - (short == "ldo"))
            assert _fill(L, fn, kernel, x, ldx, xp, ldxp, out, ldo, param) == L.SGP_EINVAL, short
            assert np.all(out == SENTINEL)


# ----------------------------------------------------------------------------- contexts
class _Ctx:
    def __init__(self, L, data, mode, strided, shards=0):
        self.L, self.lib, self.mode = L, L.lib(), mode
        y, mu = (data["yp"], data["mup"]) if mode == "laplace" else (data["y"], data["mu"])
        self.f0 = np.ascontiguousarray(mu)
        X, ldx = _mat(data["X"], strided)
        self.h = C.c_void_p()
        y, mu = np.ascontiguousarray(y), np.ascontiguousarray(mu)
        if shards:
            dv = (C.c_int * shards)(*([0] * shards))
            st = self.lib.sgp_ctx_create_multi(C.byref(self.h), dv, shards, L.dptr(X), N, ldx, D,
                                               L.dptr(y), L.dptr(mu), M + 1)
        else:
            st = self.lib.sgp_ctx_create(C.byref(self.h), 0, L.dptr(X), N, ldx, D, L.dptr(y),
                                         L.dptr(mu), M + 1)
        L.check(st)

    def close(self):
        if self.h:
            self.lib.sgp_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def eval(self, kernel, U, strided, mode=None, ldu=None):
        """(status, objective, gradient) of one evaluation at knots U."""
        L, lib, mode = self.L, self.lib, mode or self.mode
        Ub, ld = _mat(U, strided)
        ld = ld if ldu is None else ldu
        th = THETA[kernel]
        obj, grad, it = C.c_double(0.0), np.zeros(th.size), C.c_int(0)
        k = L.KERNELS[kernel]
        if mode == "laplace":
            # the resident mode warm-starts an evaluation: the same start for every call
            L.check(lib.sgp_lap_set_f(self.h, L.dptr(self.f0), 0.0))
            st = lib.sgp_eval_laplace(self.h, k, L.dptr(th), L.dptr(Ub), M, ld, DELTA, 1.0, 1e-5,
                                      1000, C.byref(obj), L.dptr(grad), C.byref(it))
        else:
            fn = lib.sgp_eval_vi if mode == "vi" else lib.sgp_eval_fitc
            st = fn(self.h, k, L.dptr(th), L.dptr(Ub), M, ld, DELTA, 0, C.byref(obj), L.dptr(grad))
        return st, np.array([obj.value]), grad

    def candidates(self, kernel, U, cand, s_u, s_c, ldu=None, ldc=None):
        L, lib = self.L, self.lib
        Ub, ld_u = _mat(U, s_u)
        Cb, ld_c = _mat(cand, s_c)
        ld_u = ld_u if ldu is None else ldu
        ld_c = ld_c if ldc is None else ldc
        th, out, k = THETA[kernel], np.full(T, SENTINEL), L.KERNELS[kernel]
        if self.mode == "laplace":
            L.check(lib.sgp_lap_set_f(self.h, L.dptr(self.f0), 0.0))
            st = lib.sgp_lap_candidates(self.h, k, L.dptr(th), L.dptr(Ub), M, ld_u, DELTA, 1.0,
                                        1e-5, 1000, L.dptr(Cb), T, ld_c, L.dptr(out))
        else:
            fn = lib.sgp_vi_candidates if self.mode == "vi" else lib.sgp_fitc_candidates
            st = fn(self.h, k, L.dptr(th), L.dptr(Ub), M, ld_u, DELTA, 0, L.dptr(Cb), T, ld_c,
                    L.dptr(out))
        return st, out


def _ok(L, res):
    assert res[0] == L.SGP_OK, L.lib().sgp_last_error()
    assert all(np.all(np.isfinite(v)) for v in res[1:])
    return res[1:]


def _same(a, b):
    return all(_same_bits(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("kernel", ["sqexp", "ard"])
@pytest.mark.parametrize("mode", ["vi", "fitc", "laplace"])
def test_context_and_knot_leading_dimensions(L, data, mode, kernel):
    """ldx of sgp_ctx_create and ldu of the evaluation, together and one at a time."""
    with _Ctx(L, data, mode, False) as packed, _Ctx(L, data, mode, True) as strided:
        ref = _ok(L, packed.eval(kernel, data["U"], False))
        assert _same(_ok(L, strided.eval(kernel, data["U2"], True)),
                     _ok(L, packed.eval(kernel, data["U2"], False)))
        assert _same(_ok(L, strided.eval(kernel, data["U"], True)), ref)      # ldx and ldu
        assert _same(_ok(L, strided.eval(kernel, data["U"], False)), ref)     # ldx alone
        assert _same(_ok(L, packed.eval(kernel, data["U2"], False)),
                     _ok(L, packed.eval(kernel, data["U2"], True)))           # ldu alone
        assert packed.eval(kernel, data["U"], False, ldu=M - 1)[0] == L.SGP_EINVAL
    X, _ = _mat(data["X"], False)
    h = C.c_void_p()
    y = np.ascontiguousarray(data["y"])
    assert L.lib().sgp_ctx_create(C.byref(h), 0, L.dptr(X), N, N - 1, D, L.dptr(y), L.dptr(y),
                                  M) == L.SGP_EINVAL
    assert not h


@pytest.mark.parametrize("mode", ["vi", "fitc", "laplace"])
def test_knot_cache_across_strides(L, data, mode):
    """One context: strided U, then the same U packed (the cache must hit and give the same
    result), then other knots strided (it must miss: equal to a fresh context given them
    packed)."""
    with _Ctx(L, data, mode, False) as ctx:
        a = _ok(L, ctx.eval("sqexp", data["U"], True))
        b = _ok(L, ctx.eval("sqexp", data["U"], False))
        assert _same(a, b)
        c = _ok(L, ctx.eval("sqexp", data["U2"], True))
        assert not _same(c, a)
        # knots whose first column alone is unchanged: a comparison at the wrong stride that
        # happened to read column 0 right would call these cached
        U3 = data["U2"].copy()
        U3[:, 0] = data["U"][:, 0]
        e = _ok(L, ctx.eval("sqexp", U3, True))
    with _Ctx(L, data, mode, False) as fresh:
        assert _same(c, _ok(L, fresh.eval("sqexp", data["U2"], False)))
    with _Ctx(L, data, mode, False) as fresh:
        assert _same(e, _ok(L, fresh.eval("sqexp", U3, False)))


def test_multi_context_strided_rows(L, data):
    """sgp_ctx_create_multi, 3 shards on device 0: shard k reads X + row0 at the caller's ldx."""
    with _Ctx(L, data, "vi", False, shards=3) as packed, \
            _Ctx(L, data, "vi", True, shards=3) as strided:
        for mode in ("vi", "fitc"):                # one pair of contexts serves both
            ref = _ok(L, packed.eval("ard", data["U"], False, mode=mode))
            assert _same(_ok(L, strided.eval("ard", data["U"], True, mode=mode)), ref)
    X, _ = _mat(data["X"], False)
    h = C.c_void_p()
    y = np.ascontiguousarray(data["y"])
    dv = (C.c_int * 3)(0, 0, 0)
    assert L.lib().sgp_ctx_create_multi(C.byref(h), dv, 3, L.dptr(X), N, N - 1, D, L.dptr(y),
                                        L.dptr(y), M) == L.SGP_EINVAL


@pytest.mark.parametrize("mode", ["vi", "fitc", "laplace"])
def test_candidate_leading_dimensions(L, data, mode):
    """ldc and ldu of the OAT candidate scorers."""
    with _Ctx(L, data, mode, False) as ctx:
        ref = _ok(L, ctx.candidates("sqexp", data["U"], data["cand"], False, False))
        for s_u, s_c in [(True, True), (True, False), (False, True)]:
            assert _same(_ok(L, ctx.candidates("sqexp", data["U"], data["cand"], s_u, s_c)), ref)
        st, out = ctx.candidates("sqexp", data["U"], data["cand"], False, False, ldc=T - 1)
        assert st == L.SGP_EINVAL and np.all(out == SENTINEL)
        st, out = ctx.candidates("sqexp", data["U"], data["cand"], False, False, ldu=M - 1)
        assert st == L.SGP_EINVAL and np.all(out == SENTINEL)


# ----------------------------------------------------------------------------- prediction
def _predict(L, data, kernel, method, full_cov, which, short=None):
    lib = L.lib()
    U, ldu = _mat(data["U"], "ldu" in which)
    V, ldv = _mat(data["u_var"], "ldv" in which)
    xp, ldxp = _mat(data["xp"], "ldxp" in which)
    pv, ldpv = _out(NP, NP if full_cov else 1, full_cov and "ldpv" in which)
    pm = np.full(NP, SENTINEL)
    if short:
        ldu, ldv, ldxp, ldpv = (ldu - (short == "ldu"), ldv - (short == "ldv"),
                                ldxp - (short == "ldxp"), ldpv - (short == "ldpv"))
    th = THETA[kernel]
    st = lib.sgp_predict(0, L.KERNELS[kernel], L.dptr(th), DELTA, method, 1, L.dptr(U), M, ldu,
                         L.dptr(np.ascontiguousarray(data["u_mean"])),
                         L.dptr(np.ascontiguousarray(data["muu"])), L.dptr(V), ldv, L.dptr(xp),
                         NP, ldxp, D, L.dptr(np.ascontiguousarray(data["mu_pred"])),
                         1 if full_cov else 0, L.dptr(pm), L.dptr(pv), ldpv)
    return st, pm, pv


@pytest.mark.parametrize("kernel", ["sqexp", "ard"])
@pytest.mark.parametrize("method", ["vi", "laplace"])
def test_predict_leading_dimensions(L, data, method, kernel):
    """ldu, ldv, ldxp and (full_cov) ldpv of sgp_predict: all strided at once and one at a
    time."""
    meth = L.SGP_PRED_VI if method == "vi" else L.SGP_PRED_LAPLACE
    names = ("ldu", "ldv", "ldxp", "ldpv")
    for full_cov in (True, False):
        st, pm0, pv0 = _predict(L, data, kernel, meth, full_cov, ())
        assert st == L.SGP_OK, L.lib().sgp_last_error()
        assert np.all(np.isfinite(pm0)) and np.all(np.isfinite(pv0))
        for which in [names] + [(nm,) for nm in names]:
            if not full_cov and which == ("ldpv",):
                continue                           # ldpv is not read without full_cov
            st, pm, pv = _predict(L, data, kernel, meth, full_cov, which)
            assert st == L.SGP_OK, (which, L.lib().sgp_last_error())
            assert _same_bits(pm, pm0), which
            _check_out(pv, NP, pv0)
        for short in names if full_cov else names[:3]:
            st, pm, pv = _predict(L, data, kernel, meth, full_cov, (), short)
            assert st == L.SGP_EINVAL, short
            assert np.all(pm == SENTINEL) and np.all(pv == SENTINEL)
