"""Wall and device time of the batch's knot gradient (SparseGPBatch.eval_vi_knots) against the
routes that existed before it.

  measure.py eval OUT.jsonl     one evaluation with knot gradients of B problems, three routes
                                alternated in one process: SparseGPBatch.eval_vi_knots (one call),
                                SparseGPBatch.eval_vi on the same batch (the added cost is the
                                difference), and a loop of SparseGPContext.eval_vi + knot_gradient
                                with enable_knot_grad, one context per problem.  Shapes: those of
                                profiles/batch/measure.py.  Host clock around calls that end in a
                                synchronise; the six stages by HIP events (sgp_diag_batch_timing,
                                sgp_diag_batch_knot_timing).
  measure.py parent OUT.jsonl   the context loop alone: it uses nothing this revision added, so it
                                also runs against a library built from the parent revision
                                (SGP_AB_LIB=tools/ab/parent/libsgp.so, _build.build_variant).
  measure.py ascent OUT.jsonl   one lockstep xu_opt = "simultaneous" ascent of (i), maxit 300,
                                against 64 sequential norm_grad_ascent_vi runs with knot gradients
                                on resident contexts.

Warm-up call first, then best of five."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles", "batch"))

import numpy as np  # noqa: E402

import sparsergps_amd as S  # noqa: E402
from measure import REPS, SHAPES, make  # noqa: E402  (profiles/batch/measure.py: the shapes)
from sparsergps_amd.vi import knot_bounds  # noqa: E402


def ctx_route(ctxs, theta, cf, xus, bounds):
    out = []
    for c, u, b in zip(ctxs, xus, bounds):
        c.eval_vi(theta, cf, u)
        out.append(c.knot_gradient(b))
    return out


def eval_mode(out, with_batch=True):
    state = {}
    for name in SHAPES:
        probs, xus, cp, cf = make(name)
        theta = np.array([float(v) for v in cp.values()])
        bounds = [knot_bounds(X) for X, _, _ in probs]
        ctxs = [S.SparseGPContext(X, y, mu, m_max=u.shape[0]) for (X, y, mu), u in zip(probs, xus)]
        for c in ctxs:
            c.enable_knot_grad(True)
        bt = S.SparseGPBatch.from_problems(probs) if with_batch else None
        k_ctx = ctx_route(ctxs, theta, cf, xus, bounds)                            # warm-up
        agree = None
        if with_batch:
            bt.stage_ms(True)
            bt.knot_stage_ms(True)
            bt.eval_vi([cp] * len(probs), cf, xus)
            _, _, k_b, st = bt.eval_vi_knots([cp] * len(probs), cf, xus)
            agree = max(float(np.max(np.abs(a - b)) / np.max(np.abs(b))) for a, b in zip(k_b, k_ctx))
            # the two routes invert by different algorithms: recorded, not bits
            assert (st == 0).all(), (name, st)
        state[name] = (probs, xus, cp, cf, theta, bounds, ctxs, bt, agree)
    inf = float("inf")
    best = {k: {"ctx": inf, "knots": inf, "plain": inf, "stages": None} for k in SHAPES}
    for _ in range(REPS):
        for name, (probs, xus, cp, cf, theta, bounds, ctxs, bt, _) in state.items():
            t0 = time.perf_counter()
            ctx_route(ctxs, theta, cf, xus, bounds)
            best[name]["ctx"] = min(best[name]["ctx"], (time.perf_counter() - t0) * 1e3)
            if with_batch:
                pars = [cp] * len(probs)
                t0 = time.perf_counter()
                bt.eval_vi(pars, cf, xus)
                best[name]["plain"] = min(best[name]["plain"], (time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                bt.eval_vi_knots(pars, cf, xus)
                wall = (time.perf_counter() - t0) * 1e3
                if wall < best[name]["knots"]:
                    best[name]["knots"] = wall
                    best[name]["stages"] = np.concatenate([bt.stage_ms(True),
                                                           bt.knot_stage_ms(True)])
    for name, b in best.items():
        B, n, d, cf, m = SHAPES[name]
        rec = {"mode": "eval" if with_batch else "parent", "shape": name, "B": B, "n": n, "d": d,
               "cov_fun": cf, "m": m, "context_loop_ms": round(b["ctx"], 4),
               "lib": os.environ.get("SGP_AB_LIB", "product")}
        if with_batch:
            rec.update({"eval_vi_knots_ms": round(b["knots"], 4),
                        "eval_vi_ms": round(b["plain"], 4),
                        "ratio": round(b["ctx"] / b["knots"], 2),
                        "max_rel_diff_to_context": state[name][8],
                        **{f"{k}_ms": round(float(v), 4) for k, v in
                           zip(("pass1", "mm", "pass2", "finish", "knot_pass", "knot_finish"),
                               b["stages"])}})
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
        one = [S.norm_grad_ascent_vi(cp, cf, True, cf, None, u, X, y, mu, None, opt, False, c)
               for (X, y, mu), u, c in zip(probs, xus, ctxs)]
        t1 = time.perf_counter()
        res = S.norm_grad_ascent_vi_batch([cp] * len(probs), cf, xus, bt, opt=opt,
                                          xu_opt="simultaneous")
        t2 = time.perf_counter()
        if rep:
            best["ctx"] = min(best["ctx"], t1 - t0)
            best["batch"] = min(best["batch"], t2 - t1)
    iters = [r["iter"] for r in res]
    rec = {"mode": "ascent", "shape": "i", "B": len(probs), "maxit": 300,
           "iter_min": min(iters), "iter_max": max(iters), "iter_sum": sum(iters),
           "iter_sum_sequential": sum(r["iter"] for r in one),
           "same_iters": iters == [r["iter"] for r in one],
           "max_rel_diff_final_obj": max(abs(r["obj_fun"][-1] - s["obj_fun"][-1]) /
                                         abs(s["obj_fun"][-1]) for r, s in zip(res, one)),
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
