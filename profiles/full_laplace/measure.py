"""Per-scope device timings: sgp_eval_full (the Sigma11 inverse stage k22_aux and contract_kmm) and,
when the library has it, sgp_eval_full_laplace (flap_state / flap_inverse / flap_step / flap_grad).
The library is the one SGP_AB_LIB names.  Prints one JSON line per (n, family)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import full_laplace_oracle as F  # noqa: E402
import sparsergps_amd as S  # noqa: E402

label = sys.argv[1]
REPS = 5
NSTATE = 6


def timed(ctx, fn):
    fn()                                  # warm-up
    ctx.enable_timing(True)
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    wall = (time.perf_counter() - t0) / REPS * 1e3
    tm = {}
    for k, v in ctx.timings():
        tm[k] = tm.get(k, 0.0) + v / REPS
    ctx.enable_timing(False)
    return wall, tm


for n in (1024, 2048):
    for family in F.FAMILIES:
        P = F.make_problem(n, 2, "sqexp", family)
        th = np.array(list(P["cov_par"].values()))
        with S.SparseGPContext(P["X"], P["y"], P["mu"], m_max=n) as ctx:
            wall, tm = timed(ctx, lambda: ctx.eval_full(th, "sqexp", P["delta"]))
            rec = {"lib": label, "n": n, "family": family, "full_eval_wall_ms": round(wall, 4),
                   "full_eval_scopes_ms": {k: round(v, 4) for k, v in tm.items()}}
            if hasattr(ctx, "eval_full_laplace") and hasattr(ctx._lib, "sgp_eval_full_laplace"):
                ctx.lap_set_family(family)

                def run():
                    ctx.lap_set_f(P["f0"])
                    return ctx.eval_full_laplace(th, "sqexp", P["delta"], P["a"], 0.0, NSTATE)

                wall, tm = timed(ctx, run)
                it = run()[2]
                assert it == NSTATE
                per = {k: round(v / (NSTATE if k != "flap_grad" and k != "k22_aux" else 1), 4)
                       for k, v in tm.items()}
                rec.update({"flap_wall_ms": round(wall, 4), "flap_states": NSTATE,
                            "flap_scopes_ms_per_state": per,
                            "nr_step_ms": round(per.get("flap_state", 0) + per.get("flap_inverse", 0)
                                                + per.get("flap_step", 0), 4)})
            print(json.dumps(rec), flush=True)
