"""Device time of the variance / error scan (sgp_fit_scan) and the shape of one OAT run.

  measure.py scan OUT.jsonl     sgp_fit_scan at C3's rows (n = 1e6, d = 8, ard) and C2's
                                (n = 1e5, d = 3, sqexp) with m = 30 and m = 128 knots: the
                                context's HIP-event scopes "fit_scan" (the pass over X and the
                                final reduction) and "scan_mm" (uploads, K22, its inverse, w, A),
                                and the host's wall time of the whole call.
  measure.py predict OUT.jsonl  the route every fit took before sgp_fit_scan existed, at the same
                                shapes: predict_laplace(x_pred = xy) and a numpy arg-max, host
                                wall time.  It uses nothing this revision added, so it also runs
                                against a library built from the parent revision
                                (SGP_AB_LIB=tools/ab/<name>/libsgp.so, _build.build_variant).
  measure.py oat OUT.jsonl      one OAT run on C2's data (VI, EGO proposals, maxknot 15, maxit
                                300): wall time split by wrapping the context's entry points,
                                and the per-evaluation time of eval_vi at m = 5, 15, 30.

Warm-up call first, then best of five, the shapes interleaved in one process."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import sparsergps_amd as S  # noqa: E402

REPS = 5
# name -> (n, d, cov_fun)
SHAPES = {"C3": (1_000_000, 8, "ard"), "C2": (100_000, 3, "sqexp")}
MS = (30, 128)


def make(n, d, cov_fun, m):
    X = np.random.default_rng(1000 * n).uniform(0.0, 10.0, size=(n, d))   # the same rows for every m
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


def scan_mode(out):
    ctxs, data = {}, {}
    for k, (n, d, cf) in SHAPES.items():
        for m in MS:
            data[k, m] = make(n, d, cf, m)
        ctxs[k] = S.SparseGPContext(data[k, MS[0]][0], np.zeros(n), data[k, MS[0]][3], m_max=8)
    best, rows = {}, {}
    for (k, m), (X, xu, cp, mu, muu, um, uv) in data.items():       # warm-up
        rows[k, m] = ctxs[k].fit_scan(cp, SHAPES[k][2], xu, um, uv, muu, "var", "poisson")["row"]
        best[k, m] = {"fit_scan": float("inf"), "scan_mm": float("inf"), "wall": float("inf")}
    for _ in range(REPS):
        for (k, m), (X, xu, cp, mu, muu, um, uv) in data.items():
            c = ctxs[k]
            c.enable_timing(True)
            t0 = time.perf_counter()
            r = c.fit_scan(cp, SHAPES[k][2], xu, um, uv, muu, "var", "poisson")
            wall = (time.perf_counter() - t0) * 1e3
            tm = dict(c.timings())
            c.enable_timing(False)
            assert r["row"] == rows[k, m]
            b = best[k, m]
            b["wall"] = min(b["wall"], wall)
            for name in ("fit_scan", "scan_mm"):
                b[name] = min(b[name], tm[name])
    for (k, m), b in best.items():
        n, d, cf = SHAPES[k]
        rec = {"mode": "scan", "shape": k, "n": n, "d": d, "cov_fun": cf, "m": m,
               "fit_scan_ms": round(b["fit_scan"], 5), "scan_mm_ms": round(b["scan_mm"], 5),
               "call_wall_ms": round(b["wall"], 4), "row": rows[k, m]}
        out.append(rec)
        print(json.dumps(rec), flush=True)


def predict_mode(out):
    # every (shape, m) shares its rows with scan mode: the same generator seeds
    for k, (n, d, cf) in SHAPES.items():
        for m in MS:
            X, xu, cp, mu, muu, um, uv = make(n, d, cf, m)
            best, row = float("inf"), None
            for rep in range(REPS + 1):
                t0 = time.perf_counter()
                pr = S.predict_laplace(um, uv, xu, X, cf, cp, mu, muu, full_cov=False,
                                       family="poisson")
                row = int(np.argmax(np.asarray(pr["pred_var"]).reshape(-1)))
                wall = (time.perf_counter() - t0) * 1e3
                if rep:
                    best = min(best, wall)
            rec = {"mode": "predict", "shape": k, "n": n, "d": d, "cov_fun": cf, "m": m,
                   "predict_route_wall_ms": round(best, 3), "row": row,
                   "lib": os.environ.get("SGP_AB_LIB", "product")}
            out.append(rec)
            print(json.dumps(rec), flush=True)


def oat_mode(out):
    from sparsergps_amd.workloads import make_gaussian_problem
    G = make_gaussian_problem("C2", m=3)
    n = G["y"].size
    spent = {"eval": 0.0, "candidates": 0.0, "scan": 0.0, "posterior": 0.0}
    counts = dict.fromkeys(spent, 0)
    ctx = S.SparseGPContext(G["X"], G["y"], G["mu"], m_max=30)

    def wrap(name, key):
        fn = getattr(ctx, name)

        def timed(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                spent[key] += time.perf_counter() - t0
                counts[key] += 1
        setattr(ctx, name, timed)
    for name, key in (("eval_vi", "eval"), ("knot_gradient", "eval"),
                      ("vi_candidates", "candidates"), ("ego_scan", "scan"),
                      ("posterior_u", "posterior")):
        wrap(name, key)
    opt = {"maxknot": 15, "maxit": 300}
    t0 = time.perf_counter()
    mod = S.optimize_gp(G["y"], G["X"], G["cov_fun"], G["cov_par"], G["mu"], "gaussian",
                        sparse=True, xu_opt="oat", xu=G["U"],
                        muu=np.full(3, float(G["y"].mean())), vi=True, opt=opt,
                        rng=np.random.default_rng(0), ctx=ctx)
    wall = time.perf_counter() - t0
    res = mod["results"]
    rec = {"mode": "oat", "n": n, "d": G["X"].shape[1], "knots": int(res["xu"].shape[0]),
           "ga_steps": [int(v) for v in res["ga_steps"]], "wall_s": round(wall, 3),
           **{f"{k}_s": round(v, 3) for k, v in spent.items()},
           **{f"{k}_calls": v for k, v in counts.items()},
           "host_s": round(wall - sum(spent.values()), 3)}
    out.append(rec)
    print(json.dumps(rec), flush=True)
    ctx.close()
    theta = np.array([float(v) for v in G["cov_par"].values()])
    with S.SparseGPContext(G["X"], G["y"], G["mu"], m_max=30) as c2:
        for m in (5, 15, 30):
            U = G["X"][np.random.default_rng(m).choice(n, size=m, replace=False)]
            c2.eval_vi(theta, G["cov_fun"], U)
            best = float("inf")
            for _ in range(REPS):
                t0 = time.perf_counter()
                for _ in range(20):
                    c2.eval_vi(theta, G["cov_fun"], U)
                best = min(best, (time.perf_counter() - t0) / 20 * 1e3)
            rec = {"mode": "eval_vi", "n": n, "m": m, "per_eval_ms": round(best, 4)}
            out.append(rec)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    recs = []
    {"scan": scan_mode, "predict": predict_mode, "oat": oat_mode}[sys.argv[1]](recs)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
