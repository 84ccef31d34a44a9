"""Oracles for the joint scores and the GP draws (sparsergps_amd.evaluation / sampling, sgp_joint_nlp,
sgp_sample_mvn, sgp_joint_kl, sgp_mc_nlp): a numpy restatement of

  the normal stream of include/sgp.h (Philox4x32-10, the 52-bit uniforms, Box-Muller),
  the draws F = mean + Z L^T,
  the three families' joint scores in log space,
  my_kl(mv = TRUE) as written, and the true KL divergence beside it,
  the per-row Monte Carlo of my_nlp(family = "bernoulli", mc = TRUE).
"""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SH32 = np.uint64(32)


def philox4x32(ctr, key):
    """Philox4x32-10.  ctr: four arrays (or scalars) of 32-bit words, key: two; returns four
    uint64 arrays holding the 32-bit output words."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        n0 = (p1 >> SH32) ^ c[1] ^ np.uint64(k0)
        n2 = (p0 >> SH32) ^ c[3] ^ np.uint64(k1)
        c = [n0, p1 & MASK, n2, p0 & MASK]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return c


def normal_pair(seed, c01, c2, c3):
    """The Box-Muller pair (cosine value, sine value) of the counter (c01 low, c01 high, c2, c3)."""
    seed = int(seed)
    c01 = np.asarray(c01, dtype=np.uint64)
    w = philox4x32((c01 & MASK, c01 >> SH32, c2, c3), (seed & 0xFFFFFFFF, seed >> 32))
    a = ((w[1] << SH32) | w[0]) >> np.uint64(12)
    b = ((w[3] << SH32) | w[2]) >> np.uint64(12)
    u1 = (a.astype(np.float64) + 0.5) * 2.0 ** -52
    u2 = (b.astype(np.float64) + 0.5) * 2.0 ** -52
    r = np.sqrt(-2.0 * np.log(u1))
    th = 6.283185307179586 * u2
    return r * np.cos(th), r * np.sin(th)


def normals(seed, stream, S, n, s0=0):
    """S x n normals: stream 0, entry (s, j) = draw s0 + s, row j of the joint stream; stream 1,
    entry (t, i) = draw s0 + t of row i of the per-row stream."""
    out = np.empty((S, n))
    if stream == 0:   # one counter per (draw, row pair)
        s = np.arange(s0, s0 + S, dtype=np.uint64)[:, None]
        jp = np.arange((n + 1) // 2, dtype=np.uint64)[None, :]
        zc, zs = normal_pair(seed, s, jp, 0)
        out[:, 0::2] = zc
        out[:, 1::2] = zs[:, :n // 2]
        return out
    # one counter per (draw pair, row): the pairs that cover draws s0 .. s0 + S - 1
    q0, q1 = s0 // 2, (s0 + S + 1) // 2
    q = np.arange(q0, q1, dtype=np.uint64)[:, None]
    i = np.arange(n, dtype=np.uint64)[None, :]
    zc, zs = normal_pair(seed, q, i, 1)
    both = np.empty((2 * (q1 - q0), n))
    both[0::2] = zc
    both[1::2] = zs
    out[:] = both[s0 - 2 * q0:s0 - 2 * q0 + S]
    return out


def draws(mean, cov, S, seed):
    """S x n: row s = mean + L z_s, L = chol(cov) lower."""
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    L = np.linalg.cholesky(np.asarray(cov, dtype=np.float64))
    return mean[None, :] + normals(seed, 0, S, mean.size) @ L.T


def log_sigmoid(z):
    return np.minimum(z, 0.0) - np.log1p(np.exp(-np.abs(z)))


def loglik(family, y, F, m=1.0):
    """sum_i log p(y_i | F_si) per draw s (F: S x n)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if family == "bernoulli":
        return np.sum(log_sigmoid((2.0 * y - 1.0)[None, :] * F), axis=1)
    if family == "poisson":
        m = np.broadcast_to(np.asarray(m, dtype=np.float64), y.shape)
        lf = np.array([math.lgamma(v + 1.0) for v in y])
        return np.sum(y[None, :] * (F + np.log(m)[None, :]) - m[None, :] * np.exp(F)
                      - lf[None, :], axis=1)
    raise ValueError(family)


def mc_summary(ll):
    """{nlp, mcsd, nlp_se, p} of the reference's Monte Carlo estimate from the draws' log
    likelihoods, in log space."""
    S = ll.size
    lmax = ll.max()
    w = np.exp(ll - lmax)
    mean = w.mean()
    sd = w.std(ddof=1) if S > 1 else float("nan")
    return {"nlp": -(lmax + math.log(mean)), "mcsd": math.exp(lmax) * sd,
            "nlp_se": sd / (mean * math.sqrt(S)), "p": math.exp(lmax) * mean}


def joint_nlp(family, y, pred_mean, pred_cov, par=1.0, S=1, seed=0):
    """my_nlp(mv = TRUE).  par: tau (gaussian) / the exposure, scalar or per row (poisson)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    mu = np.asarray(pred_mean, dtype=np.float64).reshape(-1)
    cov = np.asarray(pred_cov, dtype=np.float64)
    n = y.size
    if family == "gaussian":
        sig = cov + par * par * np.eye(n)
        r = y - mu
        _, ld = np.linalg.slogdet(sig)
        return {"nlp": 0.5 * (n * math.log(2.0 * math.pi) + ld + r @ np.linalg.solve(sig, r)),
                "mcsd": float("nan"), "nlp_se": float("nan")}
    return mc_summary(loglik(family, y, draws(mu, cov, S, seed), par))


def kl_as_written(mean1, mean2, sigma1, sigma2):
    """R/evaluation_functions.R:155-163, term by term."""
    chol1 = np.linalg.cholesky(sigma1)
    chol2 = np.linalg.cholesky(sigma2)
    d = np.asarray(mean2, dtype=np.float64).reshape(-1) - np.asarray(mean1, dtype=np.float64).reshape(-1)
    return 0.5 * (np.trace(np.linalg.solve(sigma2, sigma1)) + d @ np.linalg.solve(sigma2, d)
                  - d.size + np.sum(np.log(np.diag(chol2))) - np.sum(np.log(np.diag(chol1))))


def kl_true(mean1, mean2, sigma1, sigma2):
    d = np.asarray(mean2, dtype=np.float64).reshape(-1) - np.asarray(mean1, dtype=np.float64).reshape(-1)
    return 0.5 * (np.trace(np.linalg.solve(sigma2, sigma1)) + d @ np.linalg.solve(sigma2, d)
                  - d.size + np.linalg.slogdet(sigma2)[1] - np.linalg.slogdet(sigma1)[1])


def mc_nlp(y, pred_mean, pred_var, S, seed):
    """my_nlp(family = "bernoulli", mc = TRUE): (nlp, mcsd) per row, in linear space."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    mu = np.asarray(pred_mean, dtype=np.float64).reshape(-1)
    sd = np.sqrt(np.asarray(pred_var, dtype=np.float64).reshape(-1))
    z = normals(seed, 1, S, y.size)
    f = mu[None, :] + sd[None, :] * z
    ll = 1.0 / (1.0 + np.exp(-(2.0 * y - 1.0)[None, :] * f))
    mcsd = ll.std(axis=0, ddof=1) if S > 1 else np.full(y.size, np.nan)
    return -np.log(ll.mean(axis=0)), mcsd


def sqexp_cov(n, seed, tau=0.5, delta=1e-6):
    """The GPU tests' matrices: sqexp K(x, x) + (tau^2 + delta) I, x ~ U(0, 10)^2, sigma = l = 1."""
    x = np.random.default_rng(seed).uniform(0.0, 10.0, (n, 2))
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * d2) + (tau * tau + delta) * np.eye(n)
