"""Wall and device time of the batched small-knot FITC path against the route the parent commit has.

  measure.py eval OUT.jsonl     one evaluation of B problems: SparseGPBatch.eval_fitc (one call)
                                against a loop of SparseGPContext.eval_fitc, one context per
                                problem, alternated in one process.  Shapes (profiles/batch's):
                                (i) B = 64, n = 400, d = 3, sqexp, m = 20; (ii) B = 16, n = 8000,
                                d = 4, ard, m = 40; (iii) B = 1, n = 1e5, d = 3, sqexp, m = 5 / 15 /
                                30.  Host clock around calls that end in a synchronise, and the
                                batch's five stages by HIP events (sgp_diag_batch_fitc_timing).
  measure.py parent OUT.jsonl   the context loop alone: it uses nothing this revision added, so it
                                also runs against a library built from the parent revision
                                (SGP_AB_LIB=tools/ab/parent/libsgp.so, _build.build_variant).
  measure.py ascent OUT.jsonl   one lockstep FITC ascent of (i), maxit 300, against 64 sequential
                                norm_grad_ascent runs on resident contexts.
  measure.py score OUT.jsonl    SparseGPBatch.score() of (i)'s 64 problems, 100 held-out rows
                                each, against a loop of score_gp(vi=False).

Warm-up call first, then best of five; each record also keeps the worst of the five."""
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
STAGES = ("k22", "pass1", "mm", "pass2", "g22")


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
    return np.array([c.eval_fitc(theta, cf, u)[0] for c, u in zip(ctxs, xus)])


def eval_mode(out, with_batch=True):
    state = {}
    for name in SHAPES:
        probs, xus, cp, cf = make(name)
        theta = np.array([float(v) for v in cp.values()])
        ctxs = [S.SparseGPContext(X, y, mu, m_max=u.shape[0]) for (X, y, mu), u in zip(probs, xus)]
        bt = S.SparseGPBatch.from_problems(probs) if with_batch else None
        o_ctx = ctx_route(ctxs, theta, cf, xus)                                    # warm-up
        if with_batch:
            bt.fitc_stage_ms(True)
            o_b, _, st = bt.eval_fitc([cp] * len(probs), cf, xus)
            # the two routes invert by different algorithms: the project's 1e-6 bar, not bits
            assert (st == 0).all() and np.allclose(o_b, o_ctx, rtol=1e-6, atol=0.0), \
                (name, st, np.max(np.abs(o_b - o_ctx) / np.abs(o_ctx)))
        state[name] = (probs, xus, cp, cf, theta, ctxs, bt)
    t = {k: {"ctx": [], "batch": [], "stages": None} for k in SHAPES}
    for _ in range(REPS):
        for name, (probs, xus, cp, cf, theta, ctxs, bt) in state.items():
            t0 = time.perf_counter()
            ctx_route(ctxs, theta, cf, xus)
            t[name]["ctx"].append((time.perf_counter() - t0) * 1e3)
            if with_batch:
                pars = [cp] * len(probs)
                t0 = time.perf_counter()
                bt.eval_fitc(pars, cf, xus)
                wall = (time.perf_counter() - t0) * 1e3
                if not t[name]["batch"] or wall < min(t[name]["batch"]):
                    t[name]["stages"] = bt.fitc_stage_ms(True)
                t[name]["batch"].append(wall)
    for name, b in t.items():
        B, n, d, cf, m = SHAPES[name]
        rec = {"mode": "eval" if with_batch else "parent", "shape": name, "B": B, "n": n, "d": d,
               "cov_fun": cf, "m": m, "context_loop_ms": round(min(b["ctx"]), 4),
               "context_loop_max_ms": round(max(b["ctx"]), 4),
               "lib": os.environ.get("SGP_AB_LIB", "product")}
        if with_batch:
            rec.update({"batch_call_ms": round(min(b["batch"]), 4),
                        "batch_call_max_ms": round(max(b["batch"]), 4),
                        "ratio": round(min(b["ctx"]) / min(b["batch"]), 2),
                        **{f"{k}_ms": round(float(v), 4) for k, v in zip(STAGES, b["stages"])}})
        out.append(rec)
        print(json.dumps(rec), flush=True)


def ascent_mode(out):
    probs, xus, cp, cf = make("i")
    opt = {"maxit": 300}
    ctxs = [S.SparseGPContext(X, y, mu, m_max=u.shape[0]) for (X, y, mu), u in zip(probs, xus)]
    bt = S.SparseGPBatch.from_problems(probs)
    seq, lock = [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        one = [S.norm_grad_ascent(cp, cf, True, None, None, u, X, y, mu, None, opt, False, c)
               for (X, y, mu), u, c in zip(probs, xus, ctxs)]
        t1 = time.perf_counter()
        res = S.norm_grad_ascent_batch([cp] * len(probs), cf, xus, bt, opt=opt)
        t2 = time.perf_counter()
        if rep:
            seq.append(t1 - t0)
            lock.append(t2 - t1)
    iters = [r["iter"] for r in res]
    assert iters == [r["iter"] for r in one]
    rec = {"mode": "ascent", "shape": "i", "B": len(probs), "maxit": 300,
           "iter_min": min(iters), "iter_max": max(iters), "iter_sum": sum(iters),
           "sequential_s": round(min(seq), 4), "sequential_max_s": round(max(seq), 4),
           "lockstep_s": round(min(lock), 4), "lockstep_max_s": round(max(lock), 4),
           "ratio": round(min(seq) / min(lock), 2)}
    out.append(rec)
    print(json.dumps(rec), flush=True)


def score_mode(out):
    probs, xus, cp, cf = make("i")
    B, nt = len(probs), 100
    tests = []
    for b in range(B):
        g = np.random.default_rng(50_000 + b)
        xt = g.uniform(0.0, 10.0, size=(nt, 3))
        tests.append((xt, np.sin(xt).sum(axis=1) / np.sqrt(3) + g.normal(0.0, 0.5, size=nt),
                      np.full(nt, probs[b][1].mean())))
    bt = S.SparseGPBatch.from_problems(probs)
    _, _, st = bt.eval_fitc([cp] * B, cf, xus)
    assert (st == 0).all()
    bt.set_test_problems(tests)
    muus = [np.zeros(u.shape[0]) for u in xus]
    um, uv = bt.posterior_u(muus)
    mods = [{"family": "gaussian", "sparse": True, "delta": 1e-6,
             "results": {"u_mean": um[b], "u_var": uv[b], "xu": xus[b], "cov_fun": cf,
                         "cov_par": cp, "muu": muus[b]}} for b in range(B)]
    loop, batch = [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        one = [S.score_gp(mods[b], *tests[b], vi=False) for b in range(B)]
        t1 = time.perf_counter()
        res = bt.score()
        t2 = time.perf_counter()
        if rep:
            loop.append((t1 - t0) * 1e3)
            batch.append((t2 - t1) * 1e3)
    worst = max(float(np.max(np.abs(res[b]["nlp"] - one[b]["nlp"]))) for b in range(B))
    assert worst < 1e-7, worst
    rec = {"mode": "score", "shape": "i", "B": B, "test_rows": nt,
           "score_gp_loop_ms": round(min(loop), 4), "score_gp_loop_max_ms": round(max(loop), 4),
           "batch_score_ms": round(min(batch), 4), "batch_score_max_ms": round(max(batch), 4),
           "ratio": round(min(loop) / min(batch), 2), "worst_nlp_abs_diff": worst}
    out.append(rec)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    recs = []
    {"eval": eval_mode, "parent": lambda o: eval_mode(o, False), "ascent": ascent_mode,
     "score": score_mode}[sys.argv[1]](recs)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
