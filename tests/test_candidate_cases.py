"""The inputs of tests/test_gpu_candidate_edges.py, checked without a GPU so that no GPU test
there can pass or fail for a reason in its inputs (tests/candidate_cases.py):
  * every finite expected value is finite in the literal rebuild (or in its named substitute,
    with the literal value -inf), and the numpy model of the bordered algebra
    (oracle.adjoint_ref.vi_candidates) agrees with it to the 1e-9 the device is held to;
  * every try-error rests on a sign that is far from rounding: the base K22's smallest eigenvalue
    is above 0.05, the bordered one's below -1e-4, and so is the model's Schur complement sK;
  * both stop margins of every Laplace candidate run are >= 1e-3, so a last-bit difference cannot
    change an iteration count;
  * the near-knot case's fp64 model meets the errors against the 50-digit value that
    candidate_cases.NEAR_KNOT_MODEL_ERR records (the device's bar is derived from them)."""
import numpy as np
import pytest

import candidate_cases as CC


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


def _check_scored(c, with_model):
    good = [t for t in c["check"] if t not in c["bad"]]
    assert good
    ref, lit = c["ref"][good], c["lit"][good]
    assert np.all(np.isfinite(ref))
    sub = ~np.isfinite(lit)
    assert np.all(lit[sub] == -np.inf)                 # the only substitution: R's det() underflow
    assert np.array_equal(ref[~sub], lit[~sub])
    for t in c["bad"]:
        assert np.isnan(c["ref"][t])
    if with_model:
        every = [t for t in range(len(c["ref"])) if t not in c["bad"]]
        assert np.all(np.isfinite(c["model"][every]))
        assert _rel(c["model"][good], ref) < CC.VI_RTOL


VI_CASES = ([("vi_tile", (m,)) for m in CC.VI_TILE_M] +
            [("row_edge", ("vi", n)) for n in CC.ROW_N] +
            [("chunk", (T,)) for T in CC.CHUNK_T] +
            [("dims", ("vi",) + s) for s in CC.DIMS] +
            [("try_error", ("vi",)), ("near_knot", ()), ("outside", ("vi",))])
FITC_CASES = ([("fitc_tile", (m,)) for m in CC.FITC_TILE_M] +
              [("row_edge", ("fitc", n)) for n in CC.ROW_N] +
              [("dims", ("fitc",) + s) for s in CC.DIMS] +
              [("try_error", ("fitc",)), ("outside", ("fitc",))])
LAP_CASES = ([("lap_tile", ("poisson", m)) for m in CC.LAP_TILE_M] +
             [("lap_tile", ("bernoulli", 127)), ("try_error", ("laplace",))])


@pytest.mark.parametrize("fn,args", VI_CASES)
def test_vi_references(fn, args):
    c = getattr(CC, fn)(*args)
    _check_scored(c, True)
    if fn == "chunk":
        T = args[0]
        assert c["check"] == tuple(t for t in CC.CHUNK_LITERAL if t < T)
        if T > 130:
            assert np.array_equal(c["cand"][3], c["cand"][130])
        if T in (129, 257):
            assert np.array_equal(c["cand"][-1], CC.chunk(1)["cand"][0])
        assert np.all((c["cand"][:, None, :] == c["P"]["X"][None, :, :]).all(axis=2).any(axis=1))


@pytest.mark.parametrize("fn,args", FITC_CASES)
def test_fitc_references(fn, args):
    c = getattr(CC, fn)(*args)
    _check_scored(c, False)
    if "base" in c:
        assert np.isfinite(c["base"])
        assert c["base"] == c["base_lit"] or c["base_lit"] == -np.inf


@pytest.mark.parametrize("fn,args", LAP_CASES)
def test_laplace_references_and_stop_margins(fn, args):
    c = getattr(CC, fn)(*args)
    good = [t for t in c["check"] if t not in c["bad"]]
    assert np.all(np.isfinite(c["ref"][good])) and np.all(np.isfinite(c["fmax"]))
    print(fn, args, "stop margins", c["margins"][good].tolist())
    assert np.min(c["margins"][good]) >= CC.MARGIN_MIN
    for t in c["bad"]:
        assert np.isnan(c["ref"][t])


@pytest.mark.parametrize("mode", ["vi", "fitc", "laplace"])
def test_try_error_rests_on_a_clear_sign(mode):
    c = CC.try_error(mode)
    assert c["bad"] == (CC.TRY_BAD,)
    assert np.array_equal(c["cand"][CC.TRY_BAD], c["P"]["U"][CC.TRY_DUP])   # an exact copy
    lo_base, lo_bordered, sK, e = CC.border_margins(c["P"], laplace=mode == "laplace")
    print(mode, "min eig K22", lo_base, "bordered", lo_bordered, "sK", sK, "K22 jitter", e)
    assert e < 0.0
    assert lo_base > 0.05
    assert lo_bordered < -1e-4
    assert sK < -1e-4
    # sK = 2 e - e^2 (K22^-1)_jj for an exact copy of knot j
    th = c["theta"]
    K22 = CC.A._kmat("sqexp", c["P"]["U"], c["P"]["U"], th[0], th[1:-1])[0]
    K22 = K22 + e * np.eye(K22.shape[0])
    j = CC.TRY_DUP
    assert abs(sK - (2 * e - e * e * np.linalg.inv(K22)[j, j])) < 1e-12


def test_near_knot_model_errors():
    """The relative error of the fp64 bordered model against the 50-digit ELBO, per candidate
    [0.5 l, 0.05 l, far]: the constants the device's bar max(1e-9, 100 x error) is made from."""
    c = CC.near_knot()
    l = c["P"]["cov_par"]["l"]
    d0 = np.linalg.norm(c["cand"] - c["P"]["U"][0], axis=1) / l
    assert abs(d0[0] - CC.NEAR_DIST[0]) < 1e-12 and abs(d0[1] - CC.NEAR_DIST[1]) < 1e-12
    near_any = np.linalg.norm(c["cand"][2] - c["P"]["U"], axis=1).min() / l
    assert near_any > 1.0                               # the far candidate is far from every knot
    assert c["P"]["delta"] == 1e-6 and c["P"]["X"].shape == (60, 2) and c["P"]["U"].shape == (8, 2)
    err = np.abs(c["model"] - c["truth"]) / np.abs(c["truth"])
    err_lit = np.abs(c["ref"] - c["truth"]) / np.abs(c["truth"])
    print("near-knot model errors", err.tolist(), "literal rebuild", err_lit.tolist())
    assert np.all(err <= np.array(CC.NEAR_KNOT_MODEL_ERR))
    assert np.all(err_lit < CC.VI_RTOL)


def test_outside_candidates_are_where_the_case_says():
    for mode in ("vi", "fitc"):
        c = CC.outside(mode)
        X = c["P"]["X"]
        lo, hi = X.min(axis=0), X.max(axis=0)
        x_in, x_edge, x_far = c["cand"]
        assert np.all((x_in > lo) & (x_in < hi))
        assert abs(x_edge[0] - (hi[0] + (hi[0] - lo[0]) / 10)) < 1e-12 and lo[1] < x_edge[1] < hi[1]
        assert np.array_equal(x_far, [400.0, 400.0])
        # the far candidate's K column underflows: bordering changes nothing but the determinants
        assert abs(c["ref"][2] - c["base"]) <= 1e-12 * abs(c["base"])


def test_state_references():
    g, lp, k = CC.state_gauss(), CC.state_laplace(), CC.state_knots()
    assert g["U21"].shape == (21, 3) and not np.array_equal(g["theta"], g["theta2"])
    for um, uv in (g["post_vi"], g["post_fitc"]):
        assert um.shape == (20,) and uv.shape == (20, 20) and np.all(np.isfinite(uv))
    assert np.all(np.isfinite(lp["nr"]["u_posterior_variance"]))
    assert k["knot_gradient"].shape == (21,) and np.max(np.abs(k["knot_gradient"])) > 1e-3
    for mode in ("vi", "fitc"):
        s = CC.state_try(mode)
        assert s["U_bad"].shape == (41, 3) and np.all(np.isfinite(s["post"][1]))
