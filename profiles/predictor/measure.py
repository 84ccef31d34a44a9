"""Times of the resident predictor (sgp_predictor_*, sparsergps_amd.Predictor).

  measure.py predictor OUT.jsonl  C3's rows (np = 1e6, d = 8, ard) at m = 30, 64, 128, 1024 and
                                  C2's (np = 1e5, d = 3, sqexp) at m = 30, 64, 128, 256: the wall
                                  time of create, the steady-state wall time of predict (the
                                  product's route and chunk), and per route (1 tile, 2 the
                                  per-call arithmetic on the chunk, 3 register; 3 up to 128 knots)
                                  the four HIP-event stage times of sgp_diag_predictor_run.
  measure.py budget OUT.jsonl     C3 at m = 1024: route 1 with the K work space held to 64, 128,
                                  256 and 1024 MiB (stage times and wall time).
  measure.py percall OUT.jsonl    predict_laplace at the same shapes, host wall time.  It uses
                                  nothing this revision added, so it also runs against a library
                                  built from the parent revision (SGP_AB_LIB=tools/ab/<name>/
                                  libsgp.so, _build.build_variant).

One warm-up call first, then the best of REPS."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import sparsergps_amd as S  # noqa: E402
from sparsergps_amd import _lib  # noqa: E402

REPS = 3
# name -> (np, d, cov_fun, knot counts)
SHAPES = {"C3": (1_000_000, 8, "ard", (30, 64, 128, 1024)),
          "C2": (100_000, 3, "sqexp", (30, 64, 128, 256))}
STAGES = ("upload", "build", "quad", "download")


def make(n, d, cov_fun, m):
    """profiles/fit_scan/measure.py's inputs: the same rows for every m, knots = m of the rows."""
    X = np.random.default_rng(1000 * n).uniform(0.0, 10.0, size=(n, d))
    rng = np.random.default_rng(1000 * n + m)
    xu = X[rng.choice(n, size=m, replace=False)].copy()
    if cov_fun == "ard":
        cp = {"sigma": 1.3, **{f"l{c + 1}": 4.0 + 0.5 * c for c in range(d)}, "tau": 0.4}
    else:
        cp = {"sigma": 1.3, "l": 3.0, "tau": 0.4}
    mu = np.full(n, 0.3)
    muu = np.full(m, 0.3)
    u_mean = muu + np.sin(xu).sum(axis=1) / np.sqrt(d)
    B = rng.normal(size=(m, m))
    u_var = 0.05 * (B @ B.T) / m + 0.01 * np.eye(m)
    return X, xu, cp, mu, muu, u_mean, u_var


def best_of(fn):
    fn()
    best = float("inf")
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def stages(p, X, mu, route, chunk_rows=0):
    best = None
    for rep in range(REPS + 1):
        ms = np.zeros(4)
        p.predict(X, mu, chunk_rows=chunk_rows, route=route, stage_ms=ms)
        if rep and (best is None or ms[1] + ms[2] < best[1] + best[2]):
            best = ms
    return {f"{s}_ms": round(float(v), 4) for s, v in zip(STAGES, best)}


def emit(out, rec):
    out.append(rec)
    print(json.dumps(rec), flush=True)


def predictor_mode(out):
    for k, (n, d, cf, ms) in SHAPES.items():
        for m in ms:
            X, xu, cp, mu, muu, um, uv = make(n, d, cf, m)
            holder = []

            def create():
                while holder:
                    holder.pop().close()
                holder.append(S.Predictor("laplace", um, uv, xu, cf, cp, muu, "poisson"))
            create_ms = best_of(create)
            p = holder[0]
            ref = p.predict(X, mu)
            wall = best_of(lambda: p.predict(X, mu))
            rec = {"mode": "predictor", "shape": k, "np": n, "d": d, "cov_fun": cf, "m": m,
                   "create_wall_ms": round(create_ms, 3), "predict_wall_ms": round(wall, 3)}
            for route in (1, 2, 3):
                if route == 3 and m > 128:
                    continue
                rec[f"route{route}"] = stages(p, X, mu, route)
                got = p.predict(X, mu, route=route)
                rec[f"route{route}"]["max_rel_var_vs_product"] = float(
                    np.max(np.abs(got["pred_var"] - ref["pred_var"])) / np.max(np.abs(ref["pred_var"])))
            p.close()
            emit(out, rec)


def budget_mode(out):
    k, m = "C3", 1024
    n, d, cf, _ = SHAPES[k]
    X, xu, cp, mu, muu, um, uv = make(n, d, cf, m)
    lib = _lib.lib()
    with S.Predictor("laplace", um, uv, xu, cf, cp, muu, "poisson") as p:
        for mib in (64, 128, 256, 1024, 64, 128, 256, 1024):   # twice: the order is not the cause
            o = [C.c_int64(0) for _ in range(4)]
            _lib.check(lib.sgp_diag_predictor_plan(m, d, n, mib << 20, *(C.byref(v) for v in o)))
            rows = o[0].value
            wall = best_of(lambda: p.predict(X, mu, chunk_rows=rows, route=1))
            emit(out, {"mode": "budget", "shape": k, "np": n, "m": m, "budget_mib": mib,
                       "chunk_rows": rows, "nchunks": o[1].value,
                       "predict_wall_ms": round(wall, 3), **stages(p, X, mu, 1, rows)})


def percall_mode(out):
    for k, (n, d, cf, ms) in SHAPES.items():
        for m in ms:
            X, xu, cp, mu, muu, um, uv = make(n, d, cf, m)
            wall = best_of(lambda: S.predict_laplace(um, uv, xu, X, cf, cp, mu, muu,
                                                     full_cov=False, family="poisson"))
            emit(out, {"mode": "percall", "shape": k, "np": n, "d": d, "cov_fun": cf, "m": m,
                       "predict_laplace_wall_ms": round(wall, 3),
                       "lib": os.environ.get("SGP_AB_LIB", "product")})


if __name__ == "__main__":
    recs = []
    {"predictor": predictor_mode, "budget": budget_mode, "percall": percall_mode}[sys.argv[1]](recs)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
