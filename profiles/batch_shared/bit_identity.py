"""The three batch translation units were rewritten in terms of one set of device pieces
(sgp_batch_dev.h): show that no result of the batch path moved.

  bit_identity.py dump OUT.npz      with the library the process loads (SGP_AB_LIB=
                                    tools/ab/parent/libsgp.so: the parent revision's):
      what profiles/batch_laplace/bit_identity.py dumps of the Gaussian batch: obj, grad, status,
        the knot gradient, posterior_u, predict and score of SparseGPBatch.eval_vi /
        eval_vi_knots / eval_fitc at tests/test_gpu_batch.py's MIXED shapes, one batch per
        (d, cov_fun) group, and the same (without predict / score) at the two coincident-knot
        cases of tests/batch_fitc_cases.py;
      SparseGPBatch.eval_laplace for both families at every shape of
        tests/batch_laplace_cases.py: objective, gradient, status, all recorded objective
        values, the NR count, the mode f and posterior_u;
      one obj_only call per evaluator;
      one sqexp and one ard batch of d = 3 with m = 7, 17, 33 and 64 (all four block counts in
        one launch), through every evaluator.
  bit_identity.py compare A B       np.array_equal of every array of the two dumps
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def _vec(g):
    return np.array(list(g.values()))


def _gauss_batch(S, out, tag, Ps, Us, cf, test=None):
    """eval_vi, eval_fitc, eval_vi_knots and one obj_only call of each evaluator on one batch."""
    pars = [P["cov_par"] for P in Ps]
    zeros = [np.zeros(U.shape[0]) for U in Us]
    with S.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"]) for P in Ps]) as b:
        if test is not None:
            b.set_test(*test)
        for kind, run in (("vi", b.eval_vi), ("fitc", b.eval_fitc)):
            obj, grad, status = run(pars, cf, Us, 1e-6)
            um, uv = b.posterior_u(zeros)
            out[f"{kind}_obj_{tag}"], out[f"{kind}_status_{tag}"] = obj, status
            for i in range(len(Ps)):
                out[f"{kind}_grad_{tag}_{i}"] = _vec(grad[i])
                out[f"{kind}_u_mean_{tag}_{i}"], out[f"{kind}_u_var_{tag}_{i}"] = um[i], uv[i]
            if test is not None:
                pred, score = b.predict(), b.score()
                for i in range(len(Ps)):
                    out[f"{kind}_pred_mean_{tag}_{i}"] = pred[i]["pred_mean"]
                    out[f"{kind}_pred_var_{tag}_{i}"] = pred[i]["pred_var"]
                    out[f"{kind}_nlp_{tag}_{i}"] = score[i]["nlp"]
                    out[f"{kind}_score_{tag}_{i}"] = np.array(
                        [score[i][k] for k in ("median_nlp", "mean_nlp", "rmse", "srmse", "n_nan")])
            oo, _, so = run(pars, cf, Us, 1e-6, obj_only=True)
            out[f"{kind}_objonly_{tag}"] = np.concatenate([oo, so])
        ko, kg, kk, ks = b.eval_vi_knots(pars, cf, Us, 1e-6)
        um, uv = b.posterior_u(zeros)
        out[f"knots_obj_{tag}"], out[f"knots_status_{tag}"] = ko, ks
        for i in range(len(Ps)):
            out[f"knots_grad_{tag}_{i}"] = _vec(kg[i])
            out[f"knot_grad_{tag}_{i}"] = kk[i]
            out[f"knots_u_mean_{tag}_{i}"], out[f"knots_u_var_{tag}_{i}"] = um[i], uv[i]


def _laplace_batch(S, out, tag, family, Ps, tol, maxit):
    """eval_laplace from the reference's start and one obj_only call from the mode."""
    cf = Ps[0]["cov_fun"]
    expo = None if Ps[0]["expo"] is None else np.concatenate([P["expo"] for P in Ps])
    pars, Us = [P["cov_par"] for P in Ps], [P["U"] for P in Ps]
    with S.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"]) for P in Ps]) as b:
        b.lap_init(family, expo)
        b.set_f([P["f0"] for P in Ps])
        obj, grad, status, it = b.eval_laplace(pars, cf, Us, 1e-6, tol=tol, maxit=maxit)
        um, uv = b.posterior_u([np.zeros(U.shape[0]) for U in Us])
        fs = b.get_f()
        out[f"{family}_obj_{tag}"], out[f"{family}_status_{tag}"] = obj, status
        out[f"{family}_nr_{tag}"] = it
        for i in range(len(Ps)):
            out[f"{family}_grad_{tag}_{i}"] = _vec(grad[i])
            out[f"{family}_objs_{tag}_{i}"] = b.lap_objective_values(i)
            out[f"{family}_f_{tag}_{i}"] = fs[i]
            out[f"{family}_u_mean_{tag}_{i}"], out[f"{family}_u_var_{tag}_{i}"] = um[i], uv[i]
        oo, _, so, io = b.eval_laplace(pars, cf, Us, 1e-6, obj_only=True, tol=tol, maxit=maxit)
        out[f"{family}_objonly_{tag}"] = np.concatenate([oo, so, io])


def _counts(P, family, seed):
    """P's rows with Poisson counts or Bernoulli classes, as tests/batch_laplace_cases.py draws
    them."""
    g = np.random.Generator(np.random.PCG64(seed))
    n, d = P["X"].shape
    lat = 0.8 * np.sin(P["X"]).sum(axis=1) / math.sqrt(d)
    Q = dict(P)
    if family == "poisson":
        Q["expo"] = g.uniform(0.5, 2.0, size=n)
        Q["y"] = g.poisson(Q["expo"] * np.exp(0.7 + lat)).astype(np.float64)
        Q["f0"] = np.full(n, math.log(Q["y"].mean())) - np.log(Q["expo"])
        Q["mu"] = np.full(n, 0.5)
    else:
        Q["expo"] = None
        Q["y"] = (g.uniform(size=n) < 1.0 / (1.0 + np.exp(-2.0 * lat))).astype(np.float64)
        Q["f0"], Q["mu"] = np.zeros(n), np.zeros(n)
    return Q


def dump(path):
    import sparsergps_amd as S
    import batch_fitc_cases as FC
    import batch_laplace_cases as LC
    from test_gpu_batch import _groups
    out = {}
    for (d, cf), Ps in _groups().items():
        g = np.random.default_rng(100 + d)
        xt = g.uniform(0.0, 10.0, size=(70, d))
        yt = np.sin(xt).sum(axis=1) / np.sqrt(d)
        _gauss_batch(S, out, f"mixed_{d}_{cf}", Ps, [P["U"] for P in Ps], cf, (xt, yt, 0.1))
    for name, P, U in FC.cases():
        if U is not None:
            _gauss_batch(S, out, name, [P], [U], P["cov_fun"])
    for family, name in LC.all_cases():
        _laplace_batch(S, out, name, family, [LC.problem(family, name)], LC.TOL, LC.MAXIT)
    # all four counts of 16-knot blocks in one launch
    for cf in ("sqexp", "ard"):
        Ps = [FC.gauss(n, m, 3, cf, 800 + m) for n, m in ((130, 7), (65, 17), (200, 33), (100, 64))]
        _gauss_batch(S, out, f"blocks_{cf}", Ps, [P["U"] for P in Ps], cf)
        for family in LC.FAMILIES:
            Qs = [_counts(P, family, 900 + i) for i, P in enumerate(Ps)]
            _laplace_batch(S, out, f"blocks_{cf}", family, Qs, LC.TOL, 200)
    np.savez(path, **out)
    print("lib", os.environ.get("SGP_AB_LIB", "product"), "arrays", len(out))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files)
    bad = [k for k in A.files if not np.array_equal(A[k], B[k], equal_nan=True)]
    for k in sorted(A.files):
        print(k, A[k].shape, "DIFFERS" if k in bad else "equal")
    print(f"{len(A.files) - len(bad)} of {len(A.files)} arrays bit-identical")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        compare(sys.argv[2], sys.argv[3])
