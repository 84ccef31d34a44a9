"""Wall and device time of the batched small-knot Laplace path against the route the parent commit
has (profiles/batch_fitc's protocol).

  measure.py eval OUT.jsonl     one evaluation of B problems: SparseGPBatch.eval_laplace (one call)
                                against a loop of SparseGPContext.eval_laplace, one context per
                                problem, alternated in one process, for both families, cold (from
                                the reference's start of f) and warm-started (from the mode).
                                Shapes: (i) B = 64, n = 400, d = 3, sqexp, m = 20; (ii) B = 16,
                                n = 8000, d = 4, ard, m = 40; (iii) B = 1, n = 1e5, d = 3, sqexp,
                                m = 5 / 15 / 30.  Host clock around calls that end in a
                                synchronise, the batch's eleven stages by HIP events
                                (sgp_diag_batch_laplace_timing), and the NR counts.
  measure.py parent OUT.jsonl   the context loop alone: it uses nothing this revision added, so it
                                also runs against a library built from the parent revision
                                (SGP_AB_LIB=tools/ab/parent/libsgp.so, _build.build_variant).
  measure.py ascent OUT.jsonl   one lockstep Poisson ascent of (i), maxit 30, against 64 sequential
                                laplace_grad_ascent runs on resident contexts.

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
TOL, MAXIT = 1e-6, 1000
# name -> (B, n, d, cov_fun, m)
SHAPES = OrderedDict([("i", (64, 400, 3, "sqexp", 20)), ("ii", (16, 8000, 4, "ard", 40)),
                      ("iii_m5", (1, 100_000, 3, "sqexp", 5)),
                      ("iii_m15", (1, 100_000, 3, "sqexp", 15)),
                      ("iii_m30", (1, 100_000, 3, "sqexp", 30))])
STAGES = ("k22", "passz", "mmz", "obj_sum", "mm_sum", "nra_sum", "x2_sum", "ga", "gm", "gb", "gf")
FAMILIES = ("poisson", "bernoulli")


def make(name, family):
    B, n, d, cf, m = SHAPES[name]
    probs, xus, expos, f0s = [], [], [], []
    for b in range(B):
        g = np.random.default_rng(1000 * n + b)          # (iii): the same rows for every m
        X = g.uniform(0.0, 10.0, size=(n, d))
        lat = 0.8 * np.sin(X).sum(axis=1) / np.sqrt(d)
        if family == "poisson":
            expo = g.uniform(0.5, 2.0, size=n)
            y = g.poisson(expo * np.exp(0.7 + lat)).astype(np.float64)
            f0, mu = np.full(n, np.log(y.mean())) - np.log(expo), np.full(n, 0.5)
        else:
            expo = np.ones(n)
            y = (g.uniform(size=n) < 1.0 / (1.0 + np.exp(-2.0 * lat))).astype(np.float64)
            f0, mu = np.zeros(n), np.zeros(n)
        probs.append((X, y, mu))
        expos.append(expo)
        f0s.append(f0)
        xus.append(X[np.random.default_rng(7 * m + b).choice(n, size=m, replace=False)].copy())
    if cf == "ard":
        cp = OrderedDict([("sigma", 1.3)] + [(f"l{c + 1}", 4.0 + 0.5 * c) for c in range(d)] +
                         [("tau", 0.4)])
    else:
        cp = OrderedDict([("sigma", 1.3), ("l", 3.0), ("tau", 0.4)])
    return probs, xus, expos, f0s, cp, cf


def open_ctxs(probs, xus, expos, family):
    ctxs = []
    for (X, y, mu), u, e in zip(probs, xus, expos):
        c = S.SparseGPContext(X, y, mu, m_max=u.shape[0])
        c.lap_set_family(family)
        if family == "poisson":
            c.lap_set_expo(e)
        ctxs.append(c)
    return ctxs


def ctx_route(ctxs, theta, cf, xus, family, f0s=None):
    """(wall ms of the evaluations alone, objectives, NR counts); f0s: cold starts set first."""
    if f0s is not None:
        for c, f in zip(ctxs, f0s):
            c.lap_set_f(f)
    expo = S._lib.SGP_EXPO_ROWS if family == "poisson" else 1.0
    t0 = time.perf_counter()
    res = [c.eval_laplace(theta, cf, u, 1e-6, expo, TOL, MAXIT) for c, u in zip(ctxs, xus)]
    wall = (time.perf_counter() - t0) * 1e3
    return wall, np.array([r[0] for r in res]), np.array([r[2] for r in res])


def batch_route(bt, pars, cf, xus, f0s=None):
    if f0s is not None:
        bt.set_f(f0s)
    t0 = time.perf_counter()
    obj, _, st, it = bt.eval_laplace(pars, cf, xus, 1e-6, tol=TOL, maxit=MAXIT)
    wall = (time.perf_counter() - t0) * 1e3
    assert (st == 0).all(), st
    return wall, obj, it


def eval_mode(out, with_batch=True):
    for family in FAMILIES:
        for name in SHAPES:
            probs, xus, expos, f0s, cp, cf = make(name, family)
            B = len(probs)
            theta = np.array([float(v) for v in cp.values()])
            ctxs = open_ctxs(probs, xus, expos, family)
            bt = None
            if with_batch:
                bt = S.SparseGPBatch.from_problems(probs)
                bt.lap_init(family, np.concatenate(expos))
                bt.laplace_stage_ms(True)
            t = {k: {"ctx": [], "batch": [], "stages": None, "it_ctx": None, "it_b": None}
                 for k in ("cold", "warm")}
            for rep in range(REPS + 1):                     # rep 0 is the warm-up
                for kind in ("cold", "warm"):               # warm: from the mode cold left
                    start = f0s if kind == "cold" else None
                    w, o_c, it_c = ctx_route(ctxs, theta, cf, xus, family, start)
                    if with_batch:
                        wb, o_b, it_b = batch_route(bt, [cp] * B, cf, xus, start)
                        # two routes, two inversion algorithms: the project's 1e-6 bar, not bits
                        assert np.allclose(o_b, o_c, rtol=1e-6, atol=0.0), (name, family, kind)
                    if not rep:
                        continue
                    t[kind]["ctx"].append(w)
                    t[kind]["it_ctx"] = it_c
                    if with_batch:
                        if not t[kind]["batch"] or wb < min(t[kind]["batch"]):
                            t[kind]["stages"] = bt.laplace_stage_ms(True)
                        t[kind]["batch"].append(wb)
                        t[kind]["it_b"] = it_b
            for c in ctxs:
                c.close()
            if with_batch:
                bt.close()
            _, n, d, _, m = SHAPES[name]
            for kind, b in t.items():
                rec = {"mode": "eval" if with_batch else "parent", "family": family, "start": kind,
                       "shape": name, "B": B, "n": n, "d": d, "cov_fun": cf, "m": m,
                       "context_loop_ms": round(min(b["ctx"]), 4),
                       "context_loop_max_ms": round(max(b["ctx"]), 4),
                       "nr_min": int(b["it_ctx"].min()), "nr_max": int(b["it_ctx"].max()),
                       "nr_sum": int(b["it_ctx"].sum()),
                       "lib": os.environ.get("SGP_AB_LIB", "product")}
                if with_batch:
                    rec.update({"batch_call_ms": round(min(b["batch"]), 4),
                                "batch_call_max_ms": round(max(b["batch"]), 4),
                                "ratio": round(min(b["ctx"]) / min(b["batch"]), 2),
                                "nr_equal": bool(np.array_equal(b["it_b"], b["it_ctx"])),
                                **{f"{k}_ms": round(float(v), 4)
                                   for k, v in zip(STAGES, b["stages"])}})
                out.append(rec)
                print(json.dumps(rec), flush=True)


def ascent_mode(out):
    family = "poisson"
    probs, xus, expos, f0s, cp, cf = make("i", family)
    B = len(probs)
    opt = {"maxit": 30, "tol_nr": TOL}
    ctxs = open_ctxs(probs, xus, expos, family)
    bt = S.SparseGPBatch.from_problems(probs)
    bt.lap_init(family, np.concatenate(expos))
    muus = [np.zeros(u.shape[0]) for u in xus]
    seq, lock = [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        one = [S.laplace_grad_ascent(cp, cf, True, None, None, u, X, y, f0, mu, mb, e, opt, False,
                                     c, family)
               for (X, y, mu), u, f0, mb, e, c in zip(probs, xus, f0s, muus, expos, ctxs)]
        t1 = time.perf_counter()
        res = S.laplace_grad_ascent_batch([cp] * B, cf, xus, bt, muus, opt, family=family, ff=f0s)
        t2 = time.perf_counter()
        if rep:
            seq.append(t1 - t0)
            lock.append(t2 - t1)
    iters = [r["iter"] for r in res]
    assert iters == [r["iter"] for r in one]
    rec = {"mode": "ascent", "family": family, "shape": "i", "B": B, "maxit": 30,
           "iter_min": min(iters), "iter_max": max(iters), "iter_sum": sum(iters),
           "nr_sum": int(sum(r["nr_iter"].sum() for r in res)),
           "nr_equal": bool(all(list(a["nr_iter"]) == list(b["nr_iter"]) for a, b in zip(res, one))),
           "sequential_s": round(min(seq), 4), "sequential_max_s": round(max(seq), 4),
           "lockstep_s": round(min(lock), 4), "lockstep_max_s": round(max(lock), 4),
           "ratio": round(min(seq) / min(lock), 2)}
    out.append(rec)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    recs = []
    {"eval": eval_mode, "parent": lambda o: eval_mode(o, False),
     "ascent": ascent_mode}[sys.argv[1]](recs)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
