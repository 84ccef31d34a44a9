"""The problems the batched FITC tests share (tests/test_batch_fitc_model.py, tests/
test_gpu_batch_fitc.py): the recipe and shapes of tests/test_gpu_batch.py::MIXED and its
coincident-knot cases, each drawn once."""
import functools
import math
from collections import OrderedDict

import numpy as np

SEG = 512
# tests/test_gpu_batch.py::MIXED and its recipe
MIXED = [(1, 1, 1, "sqexp"), (65, 1, 1, "sqexp"), (5, 7, 2, "sqexp"), (63, 17, 3, "sqexp"),
         (64, 16, 3, "ard"), (129, 64, 8, "ard"), (1000, 64, 3, "sqexp"),
         (300, 33, 9, "ard"), (300, 20, 32, "ard"), (2 * SEG + 37, 30, 3, "sqexp")]
COINCIDENT = [(200, 16, 3, "sqexp", 520), (257, 48, 5, "ard", 521)]


@functools.lru_cache(maxsize=None)
def gauss(n, m, d, cov_fun, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    X = g.uniform(0.0, 10.0, size=(n, d))
    U = g.uniform(0.0, 10.0, size=(m, d))
    y = np.sin(X).sum(axis=1) / math.sqrt(d) + g.normal(0.0, 0.5, size=n)
    l0 = 1.7
    if d == 1:
        U = np.linspace(0.1, 9.9, m)[:, None]
        l0 = 0.5
    if d > 8:                       # _gauss_hd: length scales ~ sqrt(d)
        s = math.sqrt(d)
        ls = [1.2 * s + 0.2 * c for c in range(d)] if cov_fun == "ard" else [1.4 * s]
    else:
        ls = [l0 + 0.25 * c for c in range(d)] if cov_fun == "ard" else [l0]
    if cov_fun == "ard":
        cp = OrderedDict([("sigma", 1.2)] + [(f"l{c + 1}", v) for c, v in enumerate(ls)]
                         + [("tau", 0.5)])
    else:
        cp = OrderedDict([("sigma", 1.2), ("l", ls[0]), ("tau", 0.5)])
    return dict(X=X, U=U, y=y, mu=np.full(n, y.mean()), cov_par=cp, cov_fun=cov_fun, delta=1e-6)


def cases():
    out = [(f"mixed{i}", gauss(n, m, d, cf, 500 + i), None) for i, (n, m, d, cf) in enumerate(MIXED)]
    for n, m, d, cf, seed in COINCIDENT:
        P = gauss(n, m, d, cf, seed)
        U = P["X"][:m].copy()
        U[1::2] = P["U"][1::2]      # half the knots copied from rows
        out.append((f"coincident{m}", P, U))
    return out
