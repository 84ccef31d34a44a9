"""A numpy model of the batched FITC evaluation's algebra against the CPU oracle
(fitc_obj_eval / dlogp_dcov_par, fitc_posterior_u, predict_laplace): explicit inverses from an
in-order sweep, as sweep_spd forms them, K never stored beyond the rows at hand.  This pins the
algebra independently of the kernels; no GPU."""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest

from oracle import sgp_oracle as O

from batch_fitc_cases import cases


def sweep_inverse(A):
    """(A^-1, log|A|) by the in-order sweep operator (k_batch.hip's sweep_spd)."""
    A = np.array(A, dtype=np.float64)
    m = A.shape[0]
    ld = 0.0
    for k in range(m):
        dk = A[k, k]
        assert dk > 0.0
        ld += math.log(dk)
        ck = A[:, k].copy()
        A = A - np.outer(ck, ck) / dk
        A[k, :] = ck / dk
        A[:, k] = ck / dk
        A[k, k] = -1.0 / dk
    return -A, ld


def model(cov_par, cov_fun, U, X, y, mu, delta):
    """sec. 0q: the objective, the gradient in log theta, and what `post` keeps."""
    n, d = X.shape
    m = U.shape[0]
    ard = cov_fun == "ard"
    sig2, tau2 = float(cov_par["sigma"]) ** 2, float(cov_par["tau"]) ** 2
    rl = np.array([1.0 / float(cov_par[f"l{c + 1}"]) for c in range(d)]) if ard else \
        np.full(d, 1.0 / float(cov_par["l"]))
    r = y - mu
    Tu = (U[:, None, :] - U[None, :, :]) * rl              # m x m x d
    Kuu = sig2 * np.exp(-0.5 * (Tu ** 2).sum(axis=2))
    K22 = Kuu + delta * np.eye(m)
    A, ld22 = sweep_inverse(K22)
    Tx = (X[:, None, :] - U[None, :, :]) * rl              # n x m x d
    e2 = (Tx ** 2).sum(axis=2)
    K = sig2 * np.exp(-0.5 * e2)
    q = np.einsum("ij,jk,ik->i", K, A, K)
    Z = sig2 + tau2 + delta - q
    w = 1.0 / Z
    S = K.T @ (w[:, None] * K)
    t = K.T @ (w * r)
    Bi, ldB = sweep_inverse(K22 + S)
    u = Bi @ t
    obj = -0.5 * np.sum(w * r * r) + 0.5 * (t @ u) - 0.5 * (np.sum(np.log(Z)) - ld22 + ldB) - \
        (n / 2.0) * math.log(2.0 * math.pi)
    alpha = w * (r - K @ u)
    p = np.einsum("ij,jk,ik->i", K, Bi, K)
    omega = alpha ** 2 - (w - w * w * p)
    G = np.outer(alpha, u) - w[:, None] * (K @ Bi) - omega[:, None] * (K @ A)
    W = G * K
    So = K.T @ (omega[:, None] * K)
    G22 = -0.5 * np.outer(u, u) + 0.5 * (A - Bi) + 0.5 * (A @ So @ A)
    H = G22 * Kuu
    coinc = (Tx == 0.0).all(axis=2)                        # quirk Q5: the raw differences are all zero
    grad = OrderedDict()
    grad["sigma"] = 2.0 * W.sum() + 2.0 * H.sum() + sig2 * omega.sum()
    if ard:
        for c in range(d):
            grad[f"l{c + 1}"] = (W * Tx[:, :, c] ** 2).sum() + (H * Tu[:, :, c] ** 2).sum()
    else:
        grad["l"] = (W * e2).sum() + (H * (Tu ** 2).sum(axis=2)).sum()
    grad["tau"] = 2.0 * tau2 * G[coinc].sum() + tau2 * omega.sum()
    return dict(obj=obj, grad=grad, Z=Z, omega=omega, Bi=Bi, u=u, A=A, K22=K22, K=K, rl=rl,
                sig2=sig2, tau2=tau2)


@functools.lru_cache(maxsize=None)
def _run(name):
    P, U = next((P, U) for k, P, U in cases() if k == name)
    U = P["U"] if U is None else U
    M = model(P["cov_par"], P["cov_fun"], U, P["X"], P["y"], P["mu"], P["delta"])
    o = O.fitc_obj_eval(P["cov_par"], P["cov_fun"], U, P["X"], P["y"], P["mu"], P["delta"])
    g = O.dlogp_dcov_par(P["cov_par"], P["cov_fun"], U, P["X"], P["y"], P["mu"],
                         P["delta"])["gradient"]
    return P, U, M, o, g


NAMES = [k for k, _, _ in cases()]


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_oracle(name):
    P, U, M, o, g = _run(name)
    # the oracle's own rounding: cond(K22 + S) <= 1e4 at these shapes, so 1e-9 is four digits
    # above what two double-precision routes can differ by, and a thousandth of the kernels' bar
    assert abs(M["obj"] - o) / abs(o) < 1e-9, (M["obj"], o)
    assert list(M["grad"]) == list(g)
    for k in g:
        assert abs(M["grad"][k] - g[k]) / max(1.0, abs(g[k])) < 1e-9, (k, M["grad"][k], g[k])
    assert M["Z"].min() > 0.0


def test_signed_weights_and_coincidence_are_exercised():
    both = [name for name in NAMES
            if (_run(name)[2]["omega"] > 0).any() and (_run(name)[2]["omega"] < 0).any()]
    assert both, "no problem has omega of both signs"
    for name in NAMES:
        assert _run(name)[2]["Z"].min() > 0.0
    for name in NAMES:
        if name.startswith("coincident"):
            P, U, M, _, g = _run(name)
            Tx = P["X"][:, None, :] - U[None, :, :]
            assert (Tx == 0.0).all(axis=2).sum() == (U.shape[0] + 1) // 2
            assert abs(g["tau"]) > 0.0


@pytest.mark.parametrize("name", ["mixed3", "mixed5", "mixed9", "coincident16"])
def test_posterior_and_prediction_identities(name):
    """u_mean - muu = K22 u, u_var = K22 Bm^-1 K22 (fitc_posterior_u), and predict_laplace's
    pred_mean = mu + k^T u, pred_var = (sigma^2 + tau^2) + k^T (Bm^-1 - K22^-1) k: no delta."""
    P, U, M, _, _ = _run(name)
    m = U.shape[0]
    muu = np.full(m, 0.3)
    um, uv = O.fitc_posterior_u(P["cov_par"], P["cov_fun"], U, P["X"], P["y"], P["mu"], muu,
                                P["delta"])
    np.testing.assert_allclose(muu + M["K22"] @ M["u"], um, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(M["K22"] @ M["Bi"] @ M["K22"], uv, rtol=1e-9, atol=1e-9)
    g = np.random.Generator(np.random.PCG64(5))
    xt = g.uniform(0.0, 10.0, size=(40, U.shape[1]))
    ref = O.predict_laplace(um, uv, U, xt, P["cov_fun"], P["cov_par"], 0.25, muu,
                            family="gaussian", delta=P["delta"])
    kt = M["sig2"] * np.exp(-0.5 * (((xt[:, None, :] - U[None, :, :]) * M["rl"]) ** 2).sum(axis=2))
    mean = 0.25 + kt @ M["u"]
    var = (M["sig2"] + M["tau2"]) + np.einsum("ij,jk,ik->i", kt, M["Bi"] - M["A"], kt)
    np.testing.assert_allclose(mean, np.asarray(ref["pred_mean"]).reshape(-1), rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(var, ref["pred_var"], rtol=0, atol=1e-8 * np.abs(ref["pred_var"]).max())
