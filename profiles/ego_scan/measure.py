"""Device time of the EGO scan (sgp_ego_scan) at the C3 and C2 shapes, next to its floor (one
read of X at this box's measured HBM read rate) and to the only route the parent commit has (an
sgp_make_cov "exp" fill of the n x T matrix to the host, then numpy).  Best of five, the shapes
interleaved in one process; the scan's time is the context's own HIP-event scope "ego_scan"
(the pass over X and the final reduction), "ego_meta" the T x T stage before it.  One JSON line
per shape; also written to the file given as argv[1]."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sparsergps_amd as S  # noqa: E402

REPS = 5
PAR = {"sigma": 3.0, "l": 3.0, "tau": 0.0}
# name -> (n, d, T, E)
SHAPES = {"C3": (1_000_000, 8, 40, 1024), "C2": (100_000, 3, 40, 256)}


def hbm_read_rate():
    """GB/s of one streaming read: torch.sum over 2 GiB of fp64, best of five."""
    x = torch.ones(1 << 28, dtype=torch.float64, device="cuda")
    best = float("inf")
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        x.sum()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return x.numel() * 8 / (best * 1e-3) / 1e9


def make(n, d, T, E):
    rng = np.random.default_rng(1000 * n + T)
    X = rng.uniform(0.0, 10.0, size=(n, d))
    pick = rng.choice(n, size=T + E, replace=False)
    xm, xu = X[pick[:T]].copy(), X[pick[T:]].copy()
    v = -50.0 + 3.0 * np.sin(xm).sum(axis=1) / np.sqrt(d) + rng.normal(0.0, 0.1, size=T)
    return X, xm, xu, v


def host_route(X, xm, xu, v):
    """What the parent can do: K12 through the Layer-1 filler to the host, the rest in numpy."""
    t0 = time.perf_counter()
    K12 = S.make_cov_matC(X, xm, PAR, "exp", 1e-9)
    t1 = time.perf_counter()
    K22 = S.make_cov_matC(xm, None, PAR, "exp", 1e-9)
    A = np.linalg.inv(K22)
    mean = v[0] + K12 @ (A @ (v - v[0]))
    var = PAR["sigma"] ** 2 + PAR["tau"] ** 2 - ((K12 @ A) * K12).sum(axis=1)
    sd = np.sqrt(np.maximum(var, 1e-300))
    z = (mean - v.max()) / sd
    from math import erfc
    Phi = 0.5 * np.frompyfunc(erfc, 1, 1)(-z / np.sqrt(2.0)).astype(np.float64)
    ei = np.where(var > PAR["tau"] ** 2, sd * (z * Phi + np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)), 0.0)
    hit = np.isin(X[:, 0], xu[:, 0])
    ei[hit] = -1.0      # (coordinate 0 alone: enough for distinct uniform rows)
    row = int(np.argmax(ei))
    t2 = time.perf_counter()
    return row, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    rate = hbm_read_rate()
    data = {k: make(*s) for k, s in SHAPES.items()}
    ctxs = {k: S.SparseGPContext(data[k][0], np.zeros(s[0]), np.zeros(s[0]), m_max=8)
            for k, s in SHAPES.items()}
    best = {k: {"ego_scan": float("inf"), "ego_meta": float("inf"), "wall": float("inf")}
            for k in SHAPES}
    rows = {}
    for k, c in ctxs.items():       # warm-up: first-use allocations
        rows[k] = c.ego_scan(PAR, "exp", data[k][1], data[k][3], excl=data[k][2], want=())["row"]
    for _ in range(REPS):
        for k, c in ctxs.items():
            X, xm, xu, v = data[k]
            c.enable_timing(True)
            t0 = time.perf_counter()
            r = c.ego_scan(PAR, "exp", xm, v, excl=xu, want=())
            wall = (time.perf_counter() - t0) * 1e3
            tm = dict(c.timings())
            c.enable_timing(False)
            assert r["row"] == rows[k]
            best[k]["wall"] = min(best[k]["wall"], wall)
            for name in ("ego_scan", "ego_meta"):
                best[k][name] = min(best[k][name], tm[name])
    out = []
    for k, (n, d, T, E) in SHAPES.items():
        X, xm, xu, v = data[k]
        host = [host_route(X, xm, xu, v) for _ in range(3)]
        assert host[0][0] == rows[k], (host[0][0], rows[k])
        floor_ms = n * d * 8 / (rate * 1e9) * 1e3
        rec = {"shape": k, "n": n, "d": d, "T": T, "E": E, "hbm_read_GBs": round(rate, 1),
               "floor_ms": round(floor_ms, 5), "ego_scan_ms": round(best[k]["ego_scan"], 5),
               "x_floor": round(best[k]["ego_scan"] / floor_ms, 2),
               "ego_meta_ms": round(best[k]["ego_meta"], 5), "call_wall_ms": round(best[k]["wall"], 4),
               "host_route_fill_ms": round(min(h[1] for h in host), 2),
               "host_route_numpy_ms": round(min(h[2] for h in host), 2), "row": rows[k]}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    for c in ctxs.values():
        c.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in out:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
