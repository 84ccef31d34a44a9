"""bench.py's plain line, --full and --dump-outputs.

A plain run times its steps and prints the contract fields; what takes runs of its own (the
per-phase pass, the per-kernel rooflines, the CPU baseline) appears only with --full.
--dump-outputs writes the last timed step's objective and gradient as float64 arrays; the
inputs are seeded, so a second process with the same arguments reproduces them (the one-GPU
evaluation is deterministic: tests/test_gpu_determinism.py) and they agree with the CPU oracle.
Two bench processes in all, shared by the tests.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, KNOTS, STEPS, WARMUP = 3001, 96, 3, 1


def _bench(out_dir, *extra):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup",
           str(WARMUP), "--rows", str(ROWS), "--m", str(KNOTS), "--dump-outputs", str(out_dir),
           *extra]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return json.loads(lines[0]), arrays


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("plain"))


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("full"), "--full", "--no-cpu-baseline")


def test_plain_line_has_the_contract_fields_only(plain):
    line, _ = plain
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "evals/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["config"]["n"] == ROWS and line["config"]["m"] == KNOTS
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * 1e3
    for key in ("phases_ms", "kernel_rooflines", "cpu_baseline"):
        assert key not in line, key


def test_full_line_adds_phases_and_kernel_rooflines(full):
    line, _ = full
    assert line["steps"] == STEPS and line["value"] > 0
    assert line["phases_ms"]["contract_knm"] > 0
    assert {r["bound"] for r in line["kernel_rooflines"]} == {"hbm", "mfma"}
    assert "cpu_baseline" not in line      # --no-cpu-baseline


def test_dumped_outputs_are_the_last_timed_step(plain):
    from oracle import sgp_oracle as O
    from sparsergps_amd import param_names
    from sparsergps_amd.workloads import make_gaussian_problem
    line, arrays = plain
    assert sorted(arrays) == ["gradient", "objective"]
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert arrays["objective"].shape == (1,) and arrays["objective"][0] == line["objective"]
    P = make_gaussian_problem("C3", n=ROWS, m=KNOTS)
    names = param_names(P["cov_fun"], P["X"].shape[1])
    assert arrays["gradient"].shape == (len(names),)
    theta0 = np.array([P["cov_par"][k] for k in names])
    k = WARMUP + STEPS - 1                 # bench.py's theta trajectory at the last timed step
    par = dict(zip(names, theta0 * np.exp(1e-3 * np.sin(np.arange(theta0.size) + k))))
    o_ref = O.elbo_eval(par, P["cov_fun"], P["U"], P["X"], P["y"], P["mu"], P["delta"])
    g_ref = O.delbo_dcov_par(par, P["cov_fun"], P["U"], P["X"], P["y"], P["mu"],
                             P["delta"])["gradient"]
    # the suite's bar for a fused evaluation against the oracle (EVAL_RTOL of test_gpu_vi.py,
    # the bounds of __graft_entry__.smoke())
    assert abs(arrays["objective"][0] - o_ref) < 1e-6 * abs(o_ref)
    for i, name in enumerate(names):
        assert abs(arrays["gradient"][i] - g_ref[name]) < 1e-6 * max(1.0, abs(g_ref[name])), name


def test_same_arguments_same_outputs(plain, full):
    (_, a), (_, b) = plain, full
    assert sorted(a) == sorted(b)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
