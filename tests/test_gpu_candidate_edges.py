"""The OAT candidate scorers (vi_candidates / fitc_candidates / lap_candidates) at their edges, and
what a context may be asked for after one returns.  Inputs and CPU references:
tests/candidate_cases.py (checked without a GPU by tests/test_candidate_cases.py).

  a  knot-tile edges      the bordered column on, at and past a 128 tile; the m <= 256 SYRK / the
                          balanced plan; m_max = m (VI needs no room), m_max = m + 1 across a tile
  b  row edges            n = 1, 128, 129 (column norms and the candidate GEMV over padded rows)
  c  candidate chunks     T = 1, 127, 128, 129, 257: the zero-filled upload of the last chunk
  d  dimensions           d = 12, 20, 32 (ARD and sqexp) and d = 1
  e  try-error            NaN from the device for a candidate whose bordered K22 is not positive
                          definite, the candidates around it unharmed; on three shards as well
  f  near a knot          0.5 l and 0.05 l from a knot, against the 50-digit ELBO
  g  outside the box      a tenth of the range outside, and (400, 400): the widened span guard
  h  packed reduction     the unpack of S ahead of the candidate GEMMs
  i  afterwards           posterior_u / knot_gradient after a scorer or a failed evaluation: refuse,
                          or answer for the last evaluation that completed -- never anything else

Bars: the VI scorer against the rebuild 1e-9 (tests/test_gpu_candidates.py), FITC and Laplace 1e-6
(tests/test_gpu_objonly_candidates.py).  Every group prints its largest relative error; the last
test prints them all with the file's wall time."""
import time

import numpy as np
import pytest

import candidate_cases as CC

pytestmark = pytest.mark.gpu
_ERR = {}
_WALL = [0.0]


@pytest.fixture(scope="module")
def sgp():
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    return S


@pytest.fixture(autouse=True)
def _wall():
    t0 = time.perf_counter()
    yield
    _WALL[0] += time.perf_counter() - t0


def _ctx(sgp, P, m_max, **kw):
    return sgp.SparseGPContext(P["X"], P["y"], P["mu"], m_max=m_max, **kw)


def _note(group, err):
    _ERR[group] = max(_ERR.get(group, 0.0), float(err))


def _check(group, got, want, rtol, idx, what):
    """Entries idx of got against want at rtol; prints and records the largest error first."""
    idx = list(idx)
    got, want = np.asarray(got, dtype=np.float64)[idx], np.asarray(want, dtype=np.float64)[idx]
    assert np.all(np.isfinite(want))
    err = np.abs(got - want) / np.abs(want)
    err = np.where(np.isfinite(got), err, np.inf)
    print(f"[{group}] {what}: max rel err {np.max(err):.2e} (bar {rtol:g})")
    _note(group, np.max(err))
    assert np.all(err < rtol), (what, got.tolist(), want.tolist())


def _good(c):
    return [t for t in c["check"] if t not in c["bad"]]


def _vi(ctx, c, cand=None):
    P = c["P"]
    return ctx.vi_candidates(c["theta"], P["cov_fun"], P["U"], c["cand"] if cand is None else cand,
                             P["delta"])


def _fitc(ctx, c, cand=None):
    P = c["P"]
    return ctx.fitc_candidates(c["theta"], P["cov_fun"], P["U"],
                               c["cand"] if cand is None else cand, P["delta"])


def _fitc_base_still_right(group, ctx, c):
    P = c["P"]
    base, _ = ctx.eval_fitc(c["theta"], P["cov_fun"], P["U"], P["delta"])
    _check(group, [base], [c["base"]], CC.EVAL_RTOL, [0], "eval_fitc at the original knots")


def _lap(sgp, group, c, family):
    """lap_candidates from the oracle's mode; the resident f is bit-equal afterwards."""
    P = c["P"]
    m = P["U"].shape[0]
    with _ctx(sgp, P, m + 1) as ctx:
        ctx.lap_set_family(family)
        ctx.lap_set_f(c["fmax"])
        got = ctx.lap_candidates(c["theta"], "sqexp", P["U"], c["cand"], P["delta"], 1.0,
                                 CC.LAP_TOL, 1000)
        f_after = ctx.lap_get_f()
    assert np.array_equal(f_after, c["fmax"])
    for t in c["bad"]:
        assert np.isnan(got[t]), (t, got[t])
    _check(group, got, c["ref"], CC.EVAL_RTOL, _good(c), f"{family} m={m}")
    return got


# ----------------------------------------------------------------------------- a. knot tiles
@pytest.mark.parametrize("m", CC.VI_TILE_M)
def test_a_vi_knot_tile_edges(sgp, m):
    c = CC.vi_tile(m)
    P = c["P"]
    with _ctx(sgp, P, m) as ctx:                        # m_max = m: the scorer needs no spare knot
        got = _vi(ctx, c)
        base, _ = ctx.eval_vi(c["theta"], P["cov_fun"], P["U"], P["delta"])
    _check("a", got, c["ref"], CC.VI_RTOL, _good(c), f"VI m={m}")
    assert np.all(got >= base - 1e-8 * abs(base))       # Titsias: a knot can only tighten the bound


@pytest.mark.parametrize("m", CC.FITC_TILE_M)
def test_a_fitc_knot_tile_edges(sgp, m):
    c = CC.fitc_tile(m)
    with _ctx(sgp, c["P"], m + 1) as ctx:
        got = _fitc(ctx, c)
        _fitc_base_still_right("a", ctx, c)
    _check("a", got, c["ref"], CC.EVAL_RTOL, _good(c), f"FITC m={m}")


@pytest.mark.parametrize("m", CC.LAP_TILE_M)
def test_a_poisson_knot_tile_edges(sgp, m):
    _lap(sgp, "a", CC.lap_tile("poisson", m), "poisson")


def test_a_bernoulli_knot_tile_edge(sgp):
    _lap(sgp, "a", CC.lap_tile("bernoulli", 127), "bernoulli")


# ----------------------------------------------------------------------------- b. row edges
@pytest.mark.parametrize("n", CC.ROW_N)
@pytest.mark.parametrize("mode", ["vi", "fitc"])
def test_b_row_edges(sgp, mode, n):
    c = CC.row_edge(mode, n)
    with _ctx(sgp, c["P"], 7 if mode == "vi" else 8) as ctx:
        got = _vi(ctx, c) if mode == "vi" else _fitc(ctx, c)
    _check("b", got, c["ref"], CC.VI_RTOL if mode == "vi" else CC.EVAL_RTOL, _good(c),
           f"{mode} n={n}")


# ----------------------------------------------------------------------------- c. chunk edges
_CHUNK = {}


def _chunk_got(sgp, T):
    if T not in _CHUNK:
        c = CC.chunk(T)
        with _ctx(sgp, c["P"], 9) as ctx:
            _CHUNK[T] = _vi(ctx, c)
    return _CHUNK[T]


@pytest.mark.parametrize("T", CC.CHUNK_T)
def test_c_candidate_chunk_edges(sgp, T):
    c = CC.chunk(T)
    got = _chunk_got(sgp, T)
    assert got.shape == (T,) and np.all(np.isfinite(got))
    _check("c", got, c["model"], CC.VI_RTOL, range(T), f"T={T} every entry against the model")
    _check("c", got, c["ref"], CC.VI_RTOL, c["check"], f"T={T} entries {c['check']} rebuilt")
    if T in (129, 257):
        # the last chunk holds one candidate in column 0 beside 127 zero-filled ones, as the T = 1
        # call does: the same kernels on the same column data.  The implementation makes the two
        # bit-identical (measured on the MI355X), so equality is asserted: a padded column
        # leaking into a live one would break it
        one = _chunk_got(sgp, 1)[0]
        print(f"[c] T={T} last entry vs the T=1 call: {float(got[-1])!r} {float(one)!r}")
        assert got[-1] == one
    if T == 257:
        # one candidate at 3 (chunk 0, column 3) and at 130 (chunk 1, column 2): another column of
        # the same kernels, held to 1e-12 (measured: equal)
        print(f"[c] repeated candidate: {float(got[3])!r} {float(got[130])!r}")
        assert abs(got[3] - got[130]) <= 1e-12 * abs(got[3])


# ----------------------------------------------------------------------------- d. dimensions
@pytest.mark.parametrize("cov_fun,d,n,m", CC.DIMS)
@pytest.mark.parametrize("mode", ["vi", "fitc"])
def test_d_dimensions(sgp, mode, cov_fun, d, n, m):
    c = CC.dims(mode, cov_fun, d, n, m)
    with _ctx(sgp, c["P"], m if mode == "vi" else m + 1) as ctx:
        got = _vi(ctx, c) if mode == "vi" else _fitc(ctx, c)
    _check("d", got, c["ref"], CC.VI_RTOL if mode == "vi" else CC.EVAL_RTOL, _good(c),
           f"{mode} {cov_fun} d={d}")


# ----------------------------------------------------------------------------- e. try-error
def _try_gauss(ctx, mode, c):
    got = _vi(ctx, c) if mode == "vi" else _fitc(ctx, c)
    assert np.isnan(got[CC.TRY_BAD]), got
    assert np.all(np.isfinite(got[_good(c)])), got
    return got


@pytest.mark.parametrize("mode", ["vi", "fitc"])
def test_e_try_error_is_nan_and_spares_the_others(sgp, mode):
    """The middle candidate copies a knot at delta = -1e-3: its bordered K22 has an eigenvalue of
    -1e-3 (sK = -2e-3), the reference's chol() fails there and try() makes it NA.  VI reads the
    sign of sK; FITC's evaluation returns SGP_ENOTPD inside the loop, and the loop goes on."""
    c = CC.try_error(mode)
    m = c["P"]["U"].shape[0]
    with _ctx(sgp, c["P"], m + 1) as ctx:
        got = _try_gauss(ctx, mode, c)
        if mode == "fitc":
            _fitc_base_still_right("e", ctx, c)
    _check("e", got, c["ref"], CC.VI_RTOL if mode == "vi" else CC.EVAL_RTOL, _good(c), mode)


def test_e_try_error_laplace(sgp):
    """Poisson, K22 = Kuu + (tau^2 + delta) I = Kuu - 9e-4 I: the copy's Newton run is not
    positive definite; the next candidate starts from the restored f and f is restored at the
    end."""
    c = CC.try_error("laplace")
    got = _lap(sgp, "e", c, "poisson")
    assert np.isnan(got[CC.TRY_BAD])


def test_e_try_error_on_three_shards(sgp):
    """devices = [0, 0, 0], n = 500: shards of 167, 167, 166 rows.  multi.hip's cand_loop scores
    VI and FITC by objective-only evaluations over all shards; NaN in the same position, the
    finite entries equal to the one-device values at test_candidates_on_shards's 1e-8."""
    for mode in ("vi", "fitc"):
        c = CC.try_error(mode)
        m = c["P"]["U"].shape[0]
        with _ctx(sgp, c["P"], m + 1) as one, _ctx(sgp, c["P"], m + 1, devices=[0, 0, 0]) as tri:
            assert tri.shards() == (3, 1)
            a, b = _try_gauss(one, mode, c), _try_gauss(tri, mode, c)
        _check("e", b, a, 1e-8, _good(c), f"{mode} three shards against one device")
        _check("e", b, c["ref"], CC.EVAL_RTOL, _good(c), f"{mode} three shards against the rebuild")


# ----------------------------------------------------------------------------- f. near a knot
def test_f_candidate_close_to_a_knot(sgp):
    c = CC.near_knot()
    with _ctx(sgp, c["P"], 8) as ctx:
        got = _vi(ctx, c)
    for t, e in enumerate(CC.NEAR_KNOT_MODEL_ERR):
        _check("f", got, c["truth"], max(1e-9, 100.0 * e), [t],
               f"candidate {t} against the 50-digit ELBO")


# ----------------------------------------------------------------------------- g. outside the box
@pytest.mark.parametrize("mode", ["vi", "fitc"])
def test_g_candidates_outside_the_box(sgp, mode):
    c = CC.outside(mode)
    rtol = CC.VI_RTOL if mode == "vi" else CC.EVAL_RTOL
    score = _vi if mode == "vi" else _fitc
    with _ctx(sgp, c["P"], 41) as ctx:
        got = score(ctx, c)
        alone = score(ctx, c, c["cand"][:1])
    _check("g", got, c["ref"], rtol, _good(c), f"{mode} [x_in, x_edge, x_far]")
    _check("g", got, [c["base"]] * 3, rtol, [2], f"{mode} x_far against the base objective")
    # the far candidate may change the builder route of the whole call: 1e-9, not bits
    _check("g", alone, got, 1e-9, [0], f"{mode} x_in alone against x_in beside x_far")


# ----------------------------------------------------------------------------- h. packed S
def test_h_packed_first_reduction(sgp):
    c = CC.vi_tile(129)
    with _ctx(sgp, c["P"], 129) as ctx:
        ctx.set_packed_reduction(True)
        got = _vi(ctx, c)
    _check("h", got, c["ref"], CC.VI_RTOL, _good(c), "VI m=129, packed S")


# ----------------------------------------------------------------------------- i. afterwards
def _max_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _posterior_refused_or_right(sgp, ctx, what, muu, post, size=None):
    """posterior_u must raise SGPError or return `post` (the oracle's posterior of the last
    evaluation that completed) at tests/test_gpu_predict.py's bars; returns which.  size: ask
    with room for that many knots (the context's current count may be larger than post's)."""
    m = len(muu)
    ask = np.asarray(muu, dtype=np.float64)
    if size is not None:
        ask = np.concatenate([ask, np.full(size - m, ask[0])])
    try:
        um, uv = ctx.posterior_u(ask)
    except sgp.SGPError as e:
        print(f"[i] {what}: refused ({e})")
        return "refused"
    um, uv = um[:m], np.ravel(uv, order="F")[:m * m].reshape(m, m, order="F")
    em, ev = _max_rel(um, post[0]), _max_rel(uv, post[1])
    print(f"[i] {what}: answered, mean rel err {em:.2e} variance {ev:.2e}")
    assert em < 1e-8 and ev < 1e-7, f"{what}: numbers that belong to no evaluation"
    return "right"


def test_i_posterior_after_fitc_then_vi_candidates(sgp):
    s = CC.state_gauss()
    P = s["P"]
    with _ctx(sgp, P, 21) as ctx:
        ctx.eval_fitc(s["theta"], "sqexp", P["U"], P["delta"])
        assert _posterior_refused_or_right(sgp, ctx, "eval_fitc", s["muu"], s["post_fitc"]) == "right"
        ctx.vi_candidates(s["theta"], "sqexp", P["U"], s["cand"], P["delta"])
        _posterior_refused_or_right(sgp, ctx, "eval_fitc -> vi_candidates", s["muu"], s["post_fitc"])


def test_i_posterior_after_laplace_then_vi_candidates(sgp):
    s = CC.state_laplace()
    P, nr = s["P"], s["nr"]
    post = (nr["u_posterior_mean"], nr["u_posterior_variance"])
    with _ctx(sgp, P, 21) as ctx:
        ctx.lap_set_f(P["f0"])
        ctx.eval_laplace(s["theta"], "sqexp", P["U"], P["delta"], 1.0, CC.LAP_TOL, 1000)
        assert _posterior_refused_or_right(sgp, ctx, "eval_laplace", s["muu"], post) == "right"
        ctx.vi_candidates(s["theta"], "sqexp", P["U"], s["cand"], P["delta"])
        _posterior_refused_or_right(sgp, ctx, "eval_laplace -> vi_candidates", s["muu"], post)


def test_i_posterior_after_vi_candidates_with_another_knot_count(sgp):
    s = CC.state_gauss()
    P = s["P"]
    with _ctx(sgp, P, 22) as ctx:
        ctx.eval_vi(s["theta"], "sqexp", P["U"], P["delta"])
        ctx.vi_candidates(s["theta"], "sqexp", s["U21"], s["cand"], P["delta"])
        _posterior_refused_or_right(sgp, ctx, "eval_vi(m=20) -> vi_candidates(m=21)", s["muu"],
                                    s["post_vi"], size=21)


@pytest.mark.parametrize("mode", ["vi", "fitc"])
def test_i_posterior_after_a_failed_evaluation(sgp, mode):
    s = CC.state_try(mode)
    P = s["P"]
    with _ctx(sgp, P, 41) as ctx:
        ev = ctx.eval_vi if mode == "vi" else ctx.eval_fitc
        ev(s["theta"], "sqexp", P["U"], P["delta"])
        with pytest.raises(sgp.NotPositiveDefinite):
            ev(s["theta"], "sqexp", s["U_bad"], P["delta"])
        _posterior_refused_or_right(sgp, ctx, f"eval_{mode} ok -> eval_{mode} not PD", s["muu"],
                                    s["post"], size=41)


@pytest.mark.parametrize("move_knots", [False, True])
def test_i_knot_gradient_after_vi_candidates(sgp, move_knots):
    """eval_vi(theta_1) -> vi_candidates(theta_2): knot_gradient must raise or be the oracle's at
    theta_1 (tests/test_gpu_knots.py's bar).  move_knots: the scorer's call also moves the knots
    (same count), which changes the chain factor's u."""
    s = CC.state_knots()
    P = s["P"]
    U2 = 0.9 * P["U"] + 0.5 if move_knots else P["U"]
    with _ctx(sgp, P, 8) as ctx:
        ctx.enable_knot_grad(True)
        ctx.eval_vi(s["theta"], "sqexp", P["U"], P["delta"])
        g0 = ctx.knot_gradient(s["bounds"])
        e0 = np.max(np.abs(g0 - s["knot_gradient"]) / np.maximum(1.0, np.abs(s["knot_gradient"])))
        assert e0 < 1e-6
        ctx.vi_candidates(s["theta2"], "sqexp", U2, s["cand"], P["delta"])
        what = f"eval_vi(theta_1) -> vi_candidates(theta_2{', moved knots' if move_knots else ''})"
        try:
            g = ctx.knot_gradient(s["bounds"])
        except sgp.SGPError as e:
            print(f"[i] {what} -> knot_gradient: refused ({e})")
            return
        err = np.max(np.abs(g - s["knot_gradient"]) / np.maximum(1.0, np.abs(s["knot_gradient"])))
        print(f"[i] {what} -> knot_gradient: answered, err {err:.2e}")
        assert err < 1e-6, f"{what}: a knot gradient that belongs to no evaluation"


def test_i_scorer_forgets_even_its_own_base(sgp):
    """eval_vi(U) -> vi_candidates(U, the same theta): the m x m state is the base's own, but the
    scorer forgets the evaluation like its FITC and Laplace siblings (include/sgp.h): posterior_u
    and knot_gradient refuse until the next evaluation completes, which they then answer for."""
    s = CC.state_gauss()
    P = s["P"]
    with _ctx(sgp, P, 20) as ctx:
        ctx.enable_knot_grad(True)
        ctx.eval_vi(s["theta"], "sqexp", P["U"], P["delta"])
        ctx.vi_candidates(s["theta"], "sqexp", P["U"], s["cand"], P["delta"])
        with pytest.raises(sgp.SGPError, match="no completed evaluation"):
            ctx.posterior_u(s["muu"])
        with pytest.raises(sgp.SGPError):
            ctx.knot_gradient()
        ctx.eval_vi(s["theta"], "sqexp", P["U"], P["delta"])
        assert _posterior_refused_or_right(sgp, ctx, "eval_vi again", s["muu"], s["post_vi"]) == "right"


# ----------------------------------------------------------------------------- report
def test_z_report():
    print("\n[candidate edges] largest relative error per group: " +
          ", ".join(f"{g} {_ERR[g]:.2e}" for g in sorted(_ERR)) +
          f"; wall time of this file's tests {_WALL[0]:.1f} s")
