"""The Laplace batch added a translation unit, moved the likelihood policies of k_lap.hip into a
header both Laplace routes include, factored the parameter-block fill of the batch evaluations and
gave k_batch_post / k_batch_pred_mm a third case of K22's diagonal: show that the Gaussian batch
results and the context route's Laplace results did not move.

  bit_identity.py dump OUT.npz      obj, grad, status, the knot gradient and posterior_u of
                                    SparseGPBatch.eval_vi / eval_vi_knots / eval_fitc at
                                    tests/test_gpu_batch.py's MIXED shapes, one batch per
                                    (d, cov_fun) group, predict / score of the VI and of the FITC
                                    posteriors on 70 held-out rows each, and a Poisson and a
                                    Bernoulli SparseGPContext.eval_laplace (objective values, mode,
                                    gradient, posterior_u), with the library the process loads
                                    (SGP_AB_LIB=tools/ab/parent/libsgp.so: the parent revision's)
  bit_identity.py compare A B       np.array_equal of every array of the two dumps
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def dump(path):
    import sparsergps_amd as S
    import batch_laplace_cases as LC
    from test_gpu_batch import _groups
    out = {}
    for (d, cf), Ps in _groups().items():
        g = np.random.default_rng(100 + d)
        xt = g.uniform(0.0, 10.0, size=(70, d))
        yt = np.sin(xt).sum(axis=1) / np.sqrt(d)
        pars, Us = [P["cov_par"] for P in Ps], [P["U"] for P in Ps]
        zeros = [np.zeros(P["U"].shape[0]) for P in Ps]
        with S.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"]) for P in Ps]) as b:
            b.set_test(xt, yt, 0.1)
            res = {}
            for kind, run in (("vi", b.eval_vi), ("fitc", b.eval_fitc)):
                obj, grad, status = run(pars, cf, Us, 1e-6)
                res[kind] = (obj, grad, status, b.posterior_u(zeros), b.predict(), b.score())
            ko, kg, kk, ks = b.eval_vi_knots(pars, cf, Us, 1e-6)
            um2, uv2 = b.posterior_u(zeros)
        out[f"knots_obj_{d}_{cf}"] = ko
        out[f"knots_status_{d}_{cf}"] = ks
        for kind, (obj, grad, status, (um, uv), pred, score) in res.items():
            out[f"{kind}_obj_{d}_{cf}"] = obj
            out[f"{kind}_status_{d}_{cf}"] = status
            for i, P in enumerate(Ps):
                tag = f"{kind}_{d}_{cf}_{P['X'].shape[0]}_{P['U'].shape[0]}"
                out[f"grad_{tag}"] = np.array(list(grad[i].values()))
                out[f"u_mean_{tag}"] = um[i]
                out[f"u_var_{tag}"] = uv[i]
                out[f"pred_mean_{tag}"] = pred[i]["pred_mean"]
                out[f"pred_var_{tag}"] = pred[i]["pred_var"]
                out[f"nlp_{tag}"] = score[i]["nlp"]
                out[f"score_{tag}"] = np.array([score[i][k] for k in
                                                ("median_nlp", "mean_nlp", "rmse", "srmse", "n_nan")])
        for i, P in enumerate(Ps):
            tag = f"{d}_{cf}_{P['X'].shape[0]}_{P['U'].shape[0]}"
            out[f"knots_grad_{tag}"] = np.array(list(kg[i].values()))
            out[f"knot_grad_{tag}"] = kk[i]
            out[f"knots_u_mean_{tag}"] = um2[i]
            out[f"knots_u_var_{tag}"] = uv2[i]
    # the context route's Laplace evaluation (k_lap.hip now includes the shared likelihood header)
    for family, name in (("poisson", "mixed9"), ("bernoulli", "mixed7")):
        P = LC.problem(family, name)
        m = P["U"].shape[0]
        with S.SparseGPContext(P["X"], P["y"], P["mu"], m_max=m) as c:
            c.lap_set_family(family)
            c.lap_set_f(P["f0"])
            expo = 1.0
            if family == "poisson":
                c.lap_set_expo(P["expo"])
                expo = S._lib.SGP_EXPO_ROWS
            o, g, it = c.eval_laplace(np.array(list(P["cov_par"].values())), P["cov_fun"], P["U"],
                                      P["delta"], expo, LC.TOL, LC.MAXIT)
            um, uv = c.posterior_u(np.zeros(m))
            out[f"ctx_{family}_objs"] = c.lap_objective_values()
            out[f"ctx_{family}_f"] = c.lap_get_f()
        out[f"ctx_{family}_obj_grad_it"] = np.array([o, *g, it])
        out[f"ctx_{family}_u_mean"] = um
        out[f"ctx_{family}_u_var"] = uv
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
