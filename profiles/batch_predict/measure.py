"""Wall and device time of batched held-out scoring against the route the parent commit has.

  measure.py score OUT.jsonl    SparseGPBatch.score() (one call for all problems) against a loop of
                                score_gp(model_b, x_b, y_b, mu_b, vi = True) over the problems'
                                fit objects, alternated in one process.  Shapes: (i) B = 64,
                                n = 400, d = 3, sqexp, m = 20, 100 test rows per problem; (ii)
                                B = 16, n = 8000, d = 4, ard, m = 40, 2000 test rows per problem;
                                (iii) B = 1, n = 1e5, d = 3, sqexp, m = 30, C2's 1e5 rows as test
                                rows, also against a steady-state Predictor.score.  The training
                                problems are profiles/batch/measure.py's; the posterior is that of
                                one evaluation at its theta.  Host clock around calls that end in
                                a synchronise, and the batch's three stages by HIP events
                                (sgp_diag_batch_predict_timing).
  measure.py parent OUT.jsonl   the score_gp loop (and the resident predictor) alone: they use
                                nothing this revision added, so they also run against a library
                                built from the parent revision
                                (SGP_AB_LIB=tools/ab/parent/libsgp.so, _build.build_variant).

Warm-up call first, then best of five."""
import importlib.util
import json
import os
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import sparsergps_amd as S  # noqa: E402
from sparsergps_amd.workloads import make_gaussian_problem  # noqa: E402

# the training problems are profiles/batch/measure.py's
_spec = importlib.util.spec_from_file_location(
    "batch_measure", os.path.join(ROOT, "profiles", "batch", "measure.py"))
_bm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_bm)
make = _bm.make

REPS = 5
# name -> (profiles/batch's shape, test rows per problem)
SHAPES = OrderedDict([("i", ("i", 100)), ("ii", ("ii", 2000)), ("iii", ("iii_m30", 100_000))])


def tests_for(name, probs):
    src, nt = SHAPES[name]
    if name == "iii":
        P = make_gaussian_problem("C2")
        return [(P["X"], P["y"], np.full(nt, probs[0][1].mean()))]
    out = []
    for b, (X, y, mu) in enumerate(probs):
        g = np.random.default_rng(55_000 + b)
        d = X.shape[1]
        xt = g.uniform(0.0, 10.0, size=(nt, d))
        yt = np.sin(xt).sum(axis=1) / np.sqrt(d) + g.normal(0.0, 0.5, size=nt)
        out.append((xt, yt, np.full(nt, y.mean())))
    return out


def loop_route(mods, tests):
    return [S.score_gp(mod, x, y, mu, vi=True) for mod, (x, y, mu) in zip(mods, tests)]


def run(out, with_batch=True):
    state = {}
    for name, (src, nt) in SHAPES.items():
        probs, xus, cp, cf = make(src)
        tests = tests_for(name, probs)
        B = len(probs)
        bt = S.SparseGPBatch.from_problems(probs)
        _, _, st = bt.eval_vi([cp] * B, cf, xus)
        assert (st == 0).all()
        muus = [np.zeros(u.shape[0]) for u in xus]
        ums, uvs = bt.posterior_u(muus)
        mods = [{"results": {"u_mean": ums[b], "u_var": uvs[b], "xu": xus[b], "cov_fun": cf,
                             "cov_par": cp, "muu": muus[b]},
                 "sparse": True, "family": "gaussian", "delta": 1e-6} for b in range(B)]
        pred = S.predictor_gp(mods[0], vi=True) if name == "iii" else None
        ref = loop_route(mods, tests)                                             # warm-up
        if pred is not None:
            pred.score(*tests[0], par=cp["tau"])
        if with_batch:
            bt.set_test_problems(tests)
            bt.predict_stage_ms(True)
            got = bt.score()
            for a, b_ in zip(got, ref):     # the project's prediction tolerance, not bits
                for key in ("pred_mean", "pred_var"):
                    err = np.max(np.abs(a["pred"][key] - b_["pred"][key])) / \
                        np.max(np.abs(b_["pred"][key]))
                    assert err < 1e-8, (name, key, err)
                assert abs(a["mean_nlp"] - b_["mean_nlp"]) < 1e-8 * abs(b_["mean_nlp"])
        else:
            bt.close()
            bt = None
        state[name] = (mods, tests, bt, pred)
    best = {k: {"loop": float("inf"), "batch": float("inf"), "pred": float("inf"), "stages": None}
            for k in SHAPES}
    for _ in range(REPS):
        for name, (mods, tests, bt, pred) in state.items():
            t0 = time.perf_counter()
            loop_route(mods, tests)
            best[name]["loop"] = min(best[name]["loop"], (time.perf_counter() - t0) * 1e3)
            if pred is not None:
                t0 = time.perf_counter()
                pred.score(*tests[0], par=mods[0]["results"]["cov_par"]["tau"])
                best[name]["pred"] = min(best[name]["pred"], (time.perf_counter() - t0) * 1e3)
            if with_batch:
                t0 = time.perf_counter()
                bt.score()
                wall = (time.perf_counter() - t0) * 1e3
                if wall < best[name]["batch"]:
                    best[name]["batch"], best[name]["stages"] = wall, bt.predict_stage_ms(True)
    for name, b in best.items():
        mods, tests, bt, pred = state[name]
        rec = {"mode": "score" if with_batch else "parent", "shape": name, "B": len(mods),
               "m": int(np.shape(mods[0]["results"]["xu"])[0]), "test_rows": SHAPES[name][1],
               "score_gp_loop_ms": round(b["loop"], 4),
               "lib": os.environ.get("SGP_AB_LIB", "product")}
        if pred is not None:
            rec["predictor_score_ms"] = round(b["pred"], 4)
        if with_batch:
            rec.update({"batch_score_ms": round(b["batch"], 4),
                        "ratio": round(b["loop"] / b["batch"], 2),
                        **{f"{k}_ms": round(float(v), 4) for k, v in
                           zip(("pred_mm", "predict", "pred_finish"), b["stages"])}})
        out.append(rec)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    recs = []
    run(recs, sys.argv[1] != "parent")
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
