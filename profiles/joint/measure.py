"""Times of the joint-scoring and sampling entries on one MI355X, best of five after a warm-up.

sgp_sample_mvn and sgp_joint_nlp (bernoulli) at n in {1024, 4096} and S in {1e4, 1e5}: the host's
wall time of the whole call, the factor, the Z fills, the products and the scoring split by HIP
events (sgp_diag_sample_mvn / sgp_diag_joint_nlp), the products' rate against launch_gemm64 on one
square n x n x n product in the same run (sgp_diag_gemm64), and, timed once in the same run, the
numpy restatement of the same arithmetic (tests/joint_oracle.py: the Philox stream, Z L^T, the
log-space score) on the box's CPUs.  One JSON line per measurement; also written to argv[1].
"""
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT =os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import joint_oracle as JO  # noqa: E402
from sparsergps_amd import _lib  # noqa: E402

REPS = 5
SEED = 12345
PANEL = 256      # k_joint.hip: JOINT_PANEL
CPU_CHUNK = 2048
CPU_THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))
OUT = []


def emit(rec):
    OUT.append(rec)
    print(json.dumps(rec), flush=True)


def problem(n):
    rng = np.random.default_rng(n)
    cov = np.asfortranarray(JO.sqexp_cov(n, n))
    mean = 0.5 * rng.normal(size=n)
    y = (rng.random(n) < 0.5).astype(np.float64)
    return mean, cov, y


def product_flops(n, S):
    """(executed, useful) flops of the draws' products: panels of PANEL rows of the padded factor
    with K cut at the panel's end over chunks padded to 64 columns, against n^2 S."""
    np_ = -(-n // 64) * 64
    cap = max((512 << 20) // (16 * np_) // 64 * 64, 64)
    nchunk = -(-S // cap)
    sc = min(-(-(-(-S // nchunk)) // 64) * 64, S)   # capi.hip: joint_chunk
    cols = -(-S // sc) * (-(-sc // 64) * 64)   # every chunk runs the full padded width
    ex = 0
    for i0 in range(0, np_, PANEL):
        m = min(PANEL, np_ - i0)
        ex += 2 * m * (i0 + m) * cols
    return ex, float(n) * n * S


def gpu_times(n, S, mean, cov, y):
    lib = _lib.lib()
    out = np.zeros((S, n), order="F")
    o3 = np.zeros(3)
    st = np.zeros(4)
    best = {"sample_wall": np.inf, "joint_wall": np.inf, "sample_st": None, "joint_st": None}
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        _lib.check(lib.sgp_sample_mvn(0, _lib.dptr(mean), _lib.dptr(cov), n, n, S, SEED,
                                      _lib.dptr(out), S))
        t1 = time.perf_counter()
        _lib.check(lib.sgp_joint_nlp(0, 1, _lib.dptr(y), _lib.dptr(mean), _lib.dptr(cov), n, n,
                                     0.0, None, S, SEED, _lib.dptr(o3)))
        t2 = time.perf_counter()
        if rep:
            best["sample_wall"] = min(best["sample_wall"], (t1 - t0) * 1e3)
            best["joint_wall"] = min(best["joint_wall"], (t2 - t1) * 1e3)
        _lib.check(lib.sgp_diag_joint_nlp(0, 1, 0, 0, _lib.dptr(y), _lib.dptr(mean),
                                          _lib.dptr(cov), n, n, 0.0, None, S, SEED, _lib.dptr(o3),
                                          _lib.dptr(st)))
        if rep and (best["joint_st"] is None or st.sum() < best["joint_st"].sum()):
            best["joint_st"] = st.copy()
    for rep in range(2):   # the stages of the sampling entry (its products are the same launches)
        _lib.check(lib.sgp_diag_sample_mvn(0, 0, 0, _lib.dptr(mean), _lib.dptr(cov), n, n, S, SEED,
                                           _lib.dptr(out), S, _lib.dptr(st)))
        best["sample_st"] = st.copy()
    return best, out, o3.copy()


def cpu_times(n, S, mean, cov, y):
    """The numpy restatement, once, its chunks of CPU_CHUNK draws spread over CPU_THREADS threads
    (numpy's element-wise loops release the interpreter lock): (sampling seconds, scoring seconds
    on top, the summary, the last chunk's draws and its first draw).  The wall time is split
    between sampling and scoring in the ratio of the threads' own times."""
    w0 = time.perf_counter()
    L = np.linalg.cholesky(cov)
    LT = np.ascontiguousarray(L.T)
    ll = np.empty(S)
    starts = list(range(0, S, CPU_CHUNK))

    def chunk(s0):
        cnt = min(CPU_CHUNK, S - s0)
        t0 = time.perf_counter()
        F = mean[None, :] + JO.normals(SEED, 0, cnt, n, s0=s0) @ LT
        t1 = time.perf_counter()
        ll[s0:s0 + cnt] = JO.loglik("bernoulli", y, F)
        return t1 - t0, time.perf_counter() - t1, F if s0 == starts[-1] else None

    with ThreadPoolExecutor(CPU_THREADS) as pool:
        res = list(pool.map(chunk, starts))
    r = JO.mc_summary(ll)
    wall = time.perf_counter() - w0
    ts, tl = sum(v[0] for v in res), sum(v[1] for v in res)
    return wall * ts / (ts + tl), wall * tl / (ts + tl), r, res[-1][2], starts[-1]


def main():
    _lib.require_gpu()
    lib = _lib.lib()
    for n in (1024, 4096):
        mean, cov, y = problem(n)
        ms = C.c_double(0.0)
        _lib.check(lib.sgp_diag_gemm64(0, n, REPS, C.cast(C.byref(ms), _lib.c_double_p)))
        gemm_tfs = 2.0 * n ** 3 / (ms.value * 1e-3) / 1e12
        emit({"what": "gemm64_square", "n": n, "ms": round(ms.value, 4),
              "tflops": round(gemm_tfs, 2)})
        for S in (10_000, 100_000):
            g, out, o3 = gpu_times(n, S, mean, cov, y)
            t_s, t_l, r, F, s0 = cpu_times(n, S, mean, cov, y)
            # the two computed the same thing
            err = np.abs(out[s0:] - F).max()
            assert err <= 1e-11, err
            assert abs(o3[0] - r["nlp"]) <= 1e-9 * abs(r["nlp"]), (o3, r)
            ex, useful = product_flops(n, S)
            for what, wall, st, cpu in (("sgp_sample_mvn", g["sample_wall"], g["sample_st"], t_s),
                                        ("sgp_joint_nlp", g["joint_wall"], g["joint_st"],
                                         t_s + t_l)):
                prod_s = st[2] * 1e-3
                emit({"what": what, "n": n, "S": S, "call_wall_ms": round(wall, 2),
                      "factor_ms": round(st[0], 3), "fill_ms": round(st[1], 3),
                      "products_ms": round(st[2], 3), "scoring_ms": round(st[3], 3),
                      "products_tflops_executed": round(ex / prod_s / 1e12, 2),
                      "products_tflops_useful": round(useful / prod_s / 1e12, 2),
                      "gemm64_square_tflops": round(gemm_tfs, 2),
                      "numpy_cpu_s": round(cpu, 2),
                      "nlp": None if what == "sgp_sample_mvn" else float(o3[0]),
                      "nlp_se": None if what == "sgp_sample_mvn" else float(o3[2])})
            del out
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in OUT:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
