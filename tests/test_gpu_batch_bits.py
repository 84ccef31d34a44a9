"""The batch kernels' bits, kept: the three batch translation units (k_batch.hip,
k_batch_fitc.hip, k_batch_laplace.hip) are built from one set of device pieces
(sgp_batch_dev.h), and the same source inlined into two kernels is not guaranteed the same fma
contraction, so every evaluator's objective, gradient and status (and Newton's objective values and
count) are compared bit for bit with those recorded from the library before the pieces were
shared (tests/golden/batch_bits.npz, written by `_bit_outputs` below on that library: run this
file as a script, `PYTHONPATH=. python tests/test_gpu_batch_bits.py OUT.npz`, with SGP_AB_LIB
naming it).

The shapes are the smallest of tests/batch_fitc_cases.py that reach every shared piece: a row
tail inside a wave (65 = a full step plus one row; 63), a full step (64), NT = 1 .. 4 blocks of 16
knots (m = 1, 16 | 17 | 33 | 64: on and off a block), sqexp and the ARD per-coordinate sums,
d past the 8-coordinate chunk (9), and knots that equal data rows (quirk Q5's sums)."""
import os
import sys

import numpy as np
import pytest

import batch_fitc_cases as FC
import batch_laplace_cases as LC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_bits.npz")
# (n, m, d) = (65, 1, 1) sqexp, (63, 17, 3) sqexp, (64, 16, 3) ard, (129, 64, 8) ard,
# (300, 33, 9) ard, and (200, 16, 3) sqexp with half the knots copied from rows
CASES = ["mixed1", "mixed3", "mixed4", "mixed5", "mixed7", "coincident16"]


def _grad(g):
    return np.array(list(g.values()))


def _bit_outputs(S, name):
    """VI, VI with knot gradients, FITC, Poisson and Bernoulli on the case's problem, one batch
    of one problem each."""
    _, P, U = next(c for c in FC.cases() if c[0] == name)
    U = P["U"] if U is None else U
    cp, cf, out = P["cov_par"], P["cov_fun"], {}
    with S.SparseGPBatch.from_problems([(P["X"], P["y"], P["mu"])]) as b:
        for kind, run in (("vi", b.eval_vi), ("fitc", b.eval_fitc)):
            obj, grad, st = run([cp], cf, [U], P["delta"])
            out[f"{name}/{kind}"] = np.concatenate([obj, st, _grad(grad[0])])
        obj, grad, kg, st = b.eval_vi_knots([cp], cf, [U], P["delta"])
        out[f"{name}/vi_knots"] = np.concatenate([obj, st, _grad(grad[0]), kg[0]])
    for family in LC.FAMILIES:
        Q = LC.problem(family, name)
        with S.SparseGPBatch(Q["X"], Q["y"], Q["mu"]) as b:
            b.lap_init(family, Q["expo"])
            b.set_f([Q["f0"]])
            obj, grad, st, it = b.eval_laplace([Q["cov_par"]], Q["cov_fun"], [Q["U"]], Q["delta"],
                                               tol=LC.TOL, maxit=LC.MAXIT)
            out[f"{name}/{family}"] = np.concatenate([obj, st, it, _grad(grad[0]),
                                                      b.lap_objective_values(0)])
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", CASES)
def test_bits_unchanged(golden, name):
    import sparsergps_amd as S
    from sparsergps_amd import _lib
    _lib.require_gpu()
    got = _bit_outputs(S, name)
    assert sorted(got) == sorted(k for k in golden if k.startswith(name + "/"))
    assert len(got) == 5
    for k, v in got.items():
        assert np.isfinite(v).all(), k        # status 0 and a gradient: the kernels ran
        assert np.array_equal(golden[k], v, equal_nan=True), \
            (k, float(np.max(np.abs(golden[k] - v))))


if __name__ == "__main__":
    import sparsergps_amd as S
    rec = {}
    for case in CASES:
        rec.update(_bit_outputs(S, case))
    np.savez(sys.argv[1], **rec)
    print("lib", os.environ.get("SGP_AB_LIB", "product"), "arrays", len(rec),
          "values", sum(v.size for v in rec.values()))
