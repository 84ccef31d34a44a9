"""Times of the held-out scoring entries on one MI355X, best of five.

sgp_nlp at n = 1e6 for the three families: the host's wall time of the whole call (three uploads,
the launches, the readback), the two scoring launches alone by HIP events (sgp_diag_nlp), and,
timed in the same run, plain copies of the same bytes (3 n doubles to the device, n back; pageable
host memory, as the entry's arguments are).  The poisson / bernoulli kernels alone at n = 1e3,
1e5 and 1e6.  sgp_predict_nlp against sgp_predict(full_cov = 0) -- the
parent-equivalent call, whose caller would then score on the host -- at np = 1e5, m = 256, d = 3
and np = 1e6, m = 1024, d = 8.  One JSON line per measurement; also written to argv[1].
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sparsergps_amd import _lib  # noqa: E402
from sparsergps_amd.predict import _predict  # noqa: E402

REPS = 5
FAM = {"poisson": 0, "bernoulli": 1, "gaussian": 2}
OUT = []


def emit(rec):
    OUT.append(rec)
    print(json.dumps(rec), flush=True)


def rows(family, n, seed=0):
    rng = np.random.default_rng(7 * n + seed)
    mu = rng.uniform(-6.0, 6.0, n)
    s2 = 10.0 ** rng.uniform(-6.0, np.log10(25.0), n)
    if family == "poisson":
        y = rng.integers(0, 201, n).astype(np.float64)
        y[rng.random(n) < 0.3] = 0.0
        return y, mu, s2, 1.7
    if family == "bernoulli":
        return (rng.random(n) < 0.5).astype(np.float64), mu, s2, 0.0
    return mu + rng.normal(0.0, 2.0, n), mu, s2, 0.3


def nlp_times(family, n):
    """(best wall ms of sgp_nlp, best kernel ms of sgp_diag_nlp) over REPS after a warm-up."""
    lib = _lib.lib()
    y, mu, s2, par = rows(family, n)
    nlp, st, ms = np.zeros(n), np.zeros(4), C.c_double(0.0)
    args = (_lib.dptr(y), _lib.dptr(mu), _lib.dptr(s2), n, par, None, _lib.dptr(nlp),
            _lib.dptr(st))
    wall = kern = float("inf")
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        _lib.check(lib.sgp_nlp(0, FAM[family], *args))
        w = (time.perf_counter() - t0) * 1e3
        _lib.check(lib.sgp_diag_nlp(0, FAM[family], 0, *args,
                                    C.cast(C.byref(ms), _lib.c_double_p)))
        if rep:
            wall, kern = min(wall, w), min(kern, ms.value)
    return wall, kern


def copy_times(n):
    """Pageable host -> device of 3 n doubles and device -> host of n doubles, best of REPS."""
    h = [np.random.default_rng(k).random(n) for k in range(3)]
    d = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3)]
    back = torch.empty(n, dtype=torch.float64)
    up = down = float("inf")
    for rep in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a, b in zip(d, h):
            a.copy_(torch.from_numpy(b))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        back.copy_(d[0])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:
            up, down = min(up, (t1 - t0) * 1e3), min(down, (t2 - t1) * 1e3)
    return up, down


def predict_times(npred, m, d):
    rng = np.random.default_rng(npred + m)
    U = rng.uniform(0.0, 10.0, size=(m, d))
    xp = rng.uniform(0.0, 10.0, size=(npred, d))
    cp = {"sigma": 1.2, "l": 1.2 * np.sqrt(d), "tau": 0.5}
    A = rng.normal(size=(m, m))
    u_var = 0.05 * 1.44 * (A @ A.T) / m
    muu = np.full(m, 0.3)
    u_mean = muu + rng.normal(0.0, 0.5, m)
    mup = np.zeros(npred)
    yp = rng.normal(0.3, 1.0, npred)
    base = (_lib.SGP_PRED_VI, True, u_mean, u_var, U, xp, "sqexp", cp, mup, muu, False, 1e-6)
    plain = scored = host = float("inf")
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        a = _predict(*base)
        t1 = time.perf_counter()
        b = _predict(*base, ("gaussian", yp, cp["tau"], None))
        t2 = time.perf_counter()
        # the gaussian closed form on the host, what a caller of the parent would add
        v = a["pred_var"] + cp["tau"] ** 2
        ref = 0.5 * np.log(2 * np.pi * v) + (yp - a["pred_mean"].reshape(-1)) ** 2 / (2 * v)
        t3 = time.perf_counter()
        assert np.array_equal(a["pred_var"], b["pred_var"])
        assert np.max(np.abs(ref - b["nlp"]) / np.maximum(1.0, np.abs(ref))) < 1e-12
        if rep:
            plain, scored = min(plain, (t1 - t0) * 1e3), min(scored, (t2 - t1) * 1e3)
            host = min(host, (t3 - t2) * 1e3)
    # the bernoulli quadrature on the same prediction (a laplace fit's call)
    yb = (rng.random(npred) < 0.5).astype(np.float64)
    lap = (_lib.SGP_PRED_LAPLACE, False, u_mean, u_var, U, xp, "sqexp", cp, mup, muu, False, 1e-6)
    lplain = lscored = float("inf")
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        _predict(*lap)
        t1 = time.perf_counter()
        _predict(*lap, ("bernoulli", yb, 0.0, None))
        t2 = time.perf_counter()
        if rep:
            lplain, lscored = min(lplain, (t1 - t0) * 1e3), min(lscored, (t2 - t1) * 1e3)
    emit({"what": "predict", "np": npred, "m": m, "d": d,
          "sgp_predict_vi_ms": round(plain, 3), "sgp_predict_nlp_vi_gaussian_ms": round(scored, 3),
          "host_gaussian_score_ms": round(host, 3),
          "sgp_predict_laplace_ms": round(lplain, 3),
          "sgp_predict_nlp_laplace_bernoulli_ms": round(lscored, 3)})


def main():
    _lib.require_gpu()
    n = 1_000_000
    up, down = copy_times(n)
    for family in FAM:
        wall, kern = nlp_times(family, n)
        emit({"what": "sgp_nlp", "family": family, "n": n, "call_wall_ms": round(wall, 3),
              "kernels_ms": round(kern, 4), "copy_h2d_3n_ms": round(up, 3),
              "copy_d2h_n_ms": round(down, 3)})
    for nn in (1000, 100_000, 1_000_000):
        for family in ("poisson", "bernoulli"):
            emit({"what": "kernels", "family": family, "n": nn,
                  "kernels_ms": round(nlp_times(family, nn)[1], 4)})
    predict_times(100_000, 256, 3)
    predict_times(1_000_000, 1024, 8)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in OUT:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
