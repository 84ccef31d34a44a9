"""The quadrature core (sparsergps_amd/csrc/sgp_quad.h) without a GPU.

The header is HIP-free, so tests/nlp/quad_driver.cc runs the arithmetic of k_nlp_rows on the host:
the whole fixture tests/golden/nlp_grid.npz (the 612-case grid, the confident bernoulli row, the
far-tail poisson row and the y = 5000 row) plus gaussian and invalid rows, against the 50-digit
truth at 1e-11 max(1, |nlp|).  Built optimised and under AddressSanitizer + UBSan, run as a
program of its own.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "tests", "nlp", "quad_driver.cc")
OUT = os.path.join(ROOT, "build", "nlp")
GOLD = os.path.join(ROOT, "tests", "golden", "nlp_grid.npz")


def _gxx():
    c = shutil.which("g++")
    if not c:
        pytest.skip("g++ not available")
    return c


def _build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    res = subprocess.run([_gxx(), "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", *flags, DRV,
                          "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert res.returncode == 0, res.stdout.decode(errors="replace")[-4000:]
    return exe


# gaussian rows (family 2; par = tau) and rows that must come out NaN
GAUSS = [(2, 0.3, -0.2, 0.5, 0.7), (2, -4.0, 6.0, 1e-6, 0.0), (2, 1.0, 1.0, 25.0, 3.0)]
INVALID = [(0, 3.0, float("nan"), 1.0, 1.0), (1, 1.0, 0.0, 0.0, 1.0), (1, 0.0, 0.0, -1.0, 1.0),
           (0, 0.0, 0.0, float("nan"), 1.0), (0, 2.0, float("inf"), 1.0, 1.0),
           (1, 1.0, 0.0, float("inf"), 1.0), (2, 0.0, 0.0, -1.0, 0.5)]


def _check(exe, env=None):
    g = np.load(GOLD)
    rows = [(int(f), y, mu, s2, m) for f, y, mu, s2, m in
            zip(g["fam"], g["y"], g["mu"], g["s2"], g["m"])] + GAUSS + INVALID
    text = "".join("%d %.17g %.17g %.17g %.17g\n" % r for r in rows)
    run = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300, env=env)
    err = run.stderr.decode(errors="replace")
    assert run.returncode == 0, err[-6000:]
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-6000:]
    got = np.array([float(v) for v in run.stdout.decode().split()])
    assert got.size == len(rows)
    ng = g["nlp"].size
    truth = g["nlp"]
    errs = np.abs(got[:ng] - truth) / np.maximum(1.0, np.abs(truth))
    print("quad_driver: max error / max(1, |nlp|) = %.3g at row %d" % (errs.max(), errs.argmax()))
    assert np.all(np.isfinite(got[:ng]))
    assert errs.max() <= 1e-11
    for r, v in zip(GAUSS, got[ng:ng + len(GAUSS)]):
        var = r[3] + r[4] ** 2
        ref = 0.5 * np.log(2 * np.pi * var) + (r[1] - r[2]) ** 2 / (2 * var)
        assert abs(v - ref) <= 1e-13 * max(1.0, abs(ref))
    assert np.all(np.isnan(got[ng + len(GAUSS):]))


def test_quad_core_against_truth():
    _check(_build("quad_opt", ["-O2"]))


def test_quad_core_under_asan_ubsan():
    exe = _build("quad_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    _check(exe, env)
