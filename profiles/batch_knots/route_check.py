"""Where the batch's knot gradient and the single-context route differ at profiles/batch/measure.py's
(ill-conditioned) shapes: both against an 80-bit (numpy longdouble) evaluation of DESIGN.md sec.
0p's formulas on the host, for the first two problems of (ii), (iii) m = 30 and (i).  The inverses
are numpy's fp64 ones refined by three Newton steps in long double."""
import os
import sys

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "profiles", "batch"))
import sparsergps_amd as S
from measure import make
from sparsergps_amd.vi import knot_bounds
for name in ("ii", "iii_m30", "i"):
    probs, xus, cp, cf = make(name)
    probs, xus = probs[:2], xus[:2]
    theta = np.array([float(v) for v in cp.values()])
    with S.SparseGPBatch.from_problems(probs) as bt:
        _, _, kb, st = bt.eval_vi_knots([cp] * 2, cf, xus) if len(probs) == 2 else bt.eval_vi_knots([cp], cf, xus)
    for i, ((X, y, mu), U) in enumerate(zip(probs, xus)):
        with S.SparseGPContext(X, y, mu, m_max=U.shape[0]) as c:
            c.enable_knot_grad(True)
            c.eval_vi(theta, cf, U)
            kc = c.knot_gradient(knot_bounds(X))
        d = X.shape[1]; m = U.shape[0]
        ls = np.array([v for k, v in cp.items() if k.startswith("l")]); ls = np.full(d, ls[0]) if ls.size == 1 else ls
        s2, t2 = cp["sigma"] ** 2, cp["tau"] ** 2; z = t2 + 1e-6
        X_, U_, y_, mu_ = (np.asarray(a, dtype=np.longdouble) for a in (X, U, y, mu))
        ls_ = ls.astype(np.longdouble)
        k = lambda A, B: s2 * np.exp(-.5 * (((A[:, None, :] - B[None, :, :]) / ls_) ** 2).sum(2))
        K = k(X_, U_); Kuu = k(U_, U_); K22 = Kuu + np.longdouble(1e-6) * np.eye(m)
        Sm = K.T @ K; r = y_ - mu_; t = K.T @ r
        A = np.linalg.inv(K22.astype(np.float64)).astype(np.longdouble)
        for _ in range(3): A = A + A @ (np.eye(m) - K22 @ A)          # Newton refinement in long double
        Bmat = K22 + Sm / z
        Bi = np.linalg.inv(Bmat.astype(np.float64)).astype(np.longdouble)
        for _ in range(3): Bi = Bi + Bi @ (np.eye(m) - Bmat @ Bi)
        u = Bi @ t / z
        Pp = A / t2 - Bi / z - np.outer(u, u) / z
        G = np.outer(r / z, u) + K @ Pp; W = G * K
        G22 = -.5 * np.outer(u, u) + .5 * (A - Bi) - A @ Sm @ A / (2 * t2); H = G22 * Kuu
        R = W.T @ X_ - U_ * W.sum(0)[:, None]
        Q = 2 * (H @ U_ - U_ * H.sum(1)[:, None])
        b = knot_bounds(X).astype(np.longdouble)
        ref = ((R + Q) / ls_ ** 2 * (b[:, 1] - b[:, 0]) / ((U_ - b[:, 0]) * (b[:, 1] - U_) + 1e-4)).reshape(-1).astype(np.float64)
        f = lambda a: float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))
        print(name, i, "batch vs longdouble", f(kb[i]), "context vs longdouble", f(kc), "batch vs context",
              float(np.max(np.abs(kb[i] - kc)) / np.max(np.abs(kc))), flush=True)
