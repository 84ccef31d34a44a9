"""The FITC batch added a translation unit, moved the batch kernels' helpers into a header, put the
objective into the parameter block and gave k_batch_pred_mm a choice of constant: show that the VI
batch did not move.

  bit_identity.py dump OUT.npz      obj, grad, status, the knot gradient and posterior_u of
                                    SparseGPBatch.eval_vi / eval_vi_knots at tests/test_gpu_batch.py's
                                    MIXED shapes, one batch per (d, cov_fun) group, and predict /
                                    score of those VI problems on 70 held-out rows each, with the
                                    library the process loads (SGP_AB_LIB=tools/ab/parent/libsgp.so:
                                    the parent revision's)
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
    from test_gpu_batch import _groups
    out = {}
    for (d, cf), Ps in _groups().items():
        g = np.random.default_rng(100 + d)
        xt = g.uniform(0.0, 10.0, size=(70, d))
        yt = np.sin(xt).sum(axis=1) / np.sqrt(d)
        pars, Us = [P["cov_par"] for P in Ps], [P["U"] for P in Ps]
        with S.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"]) for P in Ps]) as b:
            obj, grad, status = b.eval_vi(pars, cf, Us, 1e-6)
            um, uv = b.posterior_u([np.zeros(P["U"].shape[0]) for P in Ps])
            b.set_test(xt, yt, 0.1)
            pred = b.predict()
            score = b.score()
            ko, kg, kk, ks = b.eval_vi_knots(pars, cf, Us, 1e-6)
            um2, uv2 = b.posterior_u([np.zeros(P["U"].shape[0]) for P in Ps])
        out[f"obj_{d}_{cf}"] = obj
        out[f"status_{d}_{cf}"] = status
        out[f"knots_obj_{d}_{cf}"] = ko
        out[f"knots_status_{d}_{cf}"] = ks
        for i, P in enumerate(Ps):
            tag = f"{d}_{cf}_{P['X'].shape[0]}_{P['U'].shape[0]}"
            out[f"grad_{tag}"] = np.array(list(grad[i].values()))
            out[f"u_mean_{tag}"] = um[i]
            out[f"u_var_{tag}"] = uv[i]
            out[f"pred_mean_{tag}"] = pred[i]["pred_mean"]
            out[f"pred_var_{tag}"] = pred[i]["pred_var"]
            out[f"nlp_{tag}"] = score[i]["nlp"]
            out[f"score_{tag}"] = np.array([score[i][k] for k in ("median_nlp", "mean_nlp", "rmse",
                                                                 "srmse", "n_nan")])
            out[f"knots_grad_{tag}"] = np.array(list(kg[i].values()))
            out[f"knot_grad_{tag}"] = kk[i]
            out[f"knots_u_mean_{tag}"] = um2[i]
            out[f"knots_u_var_{tag}"] = uv2[i]
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
