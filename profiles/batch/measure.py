"""Wall and device time of the batched small-knot VI path against the route the parent commit has.

  measure.py eval OUT.jsonl     one evaluation of B problems: SparseGPBatch.eval_vi (one call)
                                against a loop of SparseGPContext.eval_vi, one context per
                                problem, alternated in one process.  Shapes: (i) B = 64, n = 400,
                                d = 3, sqexp, m = 20; (ii) B = 16, n = 8000, d = 4, ard, m = 40;
                                (iii) B = 1, n = 1e5, d = 3, sqexp, m = 5 / 15 / 30.  Host clock
                                around calls that end in a synchronise, and the batch's four
                                stages by HIP events (sgp_diag_batch_timing).
  measure.py parent OUT.jsonl   the context loop alone: it uses nothing this revision added, so it
                                also runs against a library built from the parent revision
                                (SGP_AB_LIB=tools/ab/parent/libsgp.so, _build.build_variant).
  measure.py ascent OUT.jsonl   (iv) one lockstep ascent of (i), maxit 300, against 64 sequential
                                norm_grad_ascent_vi runs on resident contexts.

Warm-up call first, then best of five."""
import json
import os
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import sparsergps_amd as S  # noqa: E402

REPS = 5
# name -> (B, n, d, cov_fun, m)
SHAPES = OrderedDict([("i", (64, 400, 3, "sqexp", 20)), ("ii", (16, 8000, 4, "ard", 40)),
                      ("iii_m5", (1, 100_000, 3, "sqexp", 5)),
                      ("iii_m15", (1, 100_000, 3, "sqexp", 15)),
                      ("iii_m30", (1, 100_000, 3, "sqexp", 30))])


def make(name):
    B, n, d, cf, m = SHAPES[name]
    probs, xus = [], []
    for b in range(B):
        g = np.random.default_rng(1000 * n + b)          # (iii): the same rows for every m
        X = g.uniform(0.0, 10.0, size=(n, d))
        y = np.sin(X).sum(axis=1) / np.sqrt(d) + g.normal(0.0, 0.5, size=n)
        probs.append((X, y, np.full(n, y.mean())))
        xus.append(X[np.random.default_rng(7 * m + b).choice(n, size=m, replace=False)].copy())
    if cf == "ard":
        cp = OrderedDict([("sigma", 1.3)] + [(f"l{c + 1}", 4.0 + 0.5 * c) for c in range(d)] +
                         [("tau", 0.4)])
    else:
        cp = OrderedDict([("sigma", 1.3), ("l", 3.0), ("tau", 0.4)])
    return probs, xus, cp, cf


def ctx_route(ctxs, theta, cf, xus):
    return np.array([c.eval_vi(theta, cf, u)[0] for c, u in zip(ctxs, xus)])


def eval_mode(out, with_batch=True):
    state = {}
    for name in SHAPES:
        probs, xus, cp, cf = make(name)
        theta = np.array([float(v) for v in cp.values()])
        ctxs = [S.SparseGPContext(X, y, mu, m_max=u.shape[0]) for (X, y, mu), u in zip(probs, xus)]
        bt = S.SparseGPBatch.from_problems(probs) if with_batch else None
        o_ctx = ctx_route(ctxs, theta, cf, xus)                                    # warm-up
        if with_batch:
            bt.stage_ms(True)
            o_b, _, st = bt.eval_vi([cp] * len(probs), cf, xus)
            # the two routes invert by different algorithms: the project's 1e-6 bar, not bits
            assert (st == 0).all() and np.allclose(o_b, o_ctx, rtol=1e-6, atol=0.0), \
                (name, st, np.max(np.abs(o_b - o_ctx) / np.abs(o_ctx)))
        state[name] = (probs, xus, cp, cf, theta, ctxs, bt)
    best = {k: {"ctx": float("inf"), "batch": float("inf"), "stages": None} for k in SHAPES}
    for _ in range(REPS):
        for name, (probs, xus, cp, cf, theta, ctxs, bt) in state.items():
            t0 = time.perf_counter()
            ctx_route(ctxs, theta, cf, xus)
            best[name]["ctx"] = min(best[name]["ctx"], (time.perf_counter() - t0) * 1e3)
            if with_batch:
                pars = [cp] * len(probs)
                t0 = time.perf_counter()
                bt.eval_vi(pars, cf, xus)
                wall = (time.perf_counter() - t0) * 1e3
                if wall < best[name]["batch"]:
                    best[name]["batch"], best[name]["stages"] = wall, bt.stage_ms(True)
    for name, b in best.items():
        B, n, d, cf, m = SHAPES[name]
        rec = {"mode": "eval" if with_batch else "parent", "shape": name, "B": B, "n": n, "d": d,
               "cov_fun": cf, "m": m, "context_loop_ms": round(b["ctx"], 4),
               "lib": os.environ.get("SGP_AB_LIB", "product")}
        if with_batch:
            rec.update({"batch_call_ms": round(b["batch"], 4),
                        "ratio": round(b["ctx"] / b["batch"], 2),
                        **{f"{k}_ms": round(float(v), 4) for k, v in
                           zip(("pass1", "mm", "pass2", "finish"), b["stages"])}})
        out.append(rec)
        print(json.dumps(rec), flush=True)


def ascent_mode(out):
    probs, xus, cp, cf = make("i")
    opt = {"maxit": 300}
    ctxs = [S.SparseGPContext(X, y, mu, m_max=u.shape[0]) for (X, y, mu), u in zip(probs, xus)]
    bt = S.SparseGPBatch.from_problems(probs)
    best = {"ctx": float("inf"), "batch": float("inf")}
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        one = [S.norm_grad_ascent_vi(cp, cf, True, None, None, u, X, y, mu, None, opt, False, c)
               for (X, y, mu), u, c in zip(probs, xus, ctxs)]
        t1 = time.perf_counter()
        res = S.norm_grad_ascent_vi_batch([cp] * len(probs), cf, xus, bt, opt=opt)
        t2 = time.perf_counter()
        if rep:
            best["ctx"] = min(best["ctx"], t1 - t0)
            best["batch"] = min(best["batch"], t2 - t1)
    iters = [r["iter"] for r in res]
    assert iters == [r["iter"] for r in one]
    rec = {"mode": "ascent", "shape": "i", "B": len(probs), "maxit": 300,
           "iter_min": min(iters), "iter_max": max(iters), "iter_sum": sum(iters),
           "sequential_s": round(best["ctx"], 4), "lockstep_s": round(best["batch"], 4),
           "ratio": round(best["ctx"] / best["batch"], 2)}
    out.append(rec)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    recs = []
    {"eval": eval_mode, "parent": lambda o: eval_mode(o, False), "ascent": ascent_mode}[
        sys.argv[1]](recs)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
