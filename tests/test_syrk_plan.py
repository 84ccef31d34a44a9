"""The work-balanced SYRK plan (sparsergps_amd/csrc/sgp_syrk_plan.h) without a GPU.

The planner and the functions the kernel runs to find its segments are host-compilable;
tests/syrk_plan/plan_driver.cc walks every workgroup's segments for nb = 3 ... 12 column panels
and n_pad in {128, 1024, 4096, 4224, 125056, 1000064} and checks: every (lower 64-block, 16-row
step) covered exactly once; no strictly-upper fragment of a diagonal 64-block scheduled; at most
two segments per workgroup and none empty; every workgroup's modelled cost within one
off-diagonal step (64 MFMA slots) of the mean; the groups of a row band on identical rows and
adjacent after the XCD remap; the partial slabs inside the size the library reserves, each
written once, each diagonal tile's list in row order; the plan a pure function of its arguments;
the headline's modelled makespan at most 0.965 of the packed plan's; nb < 3 and nb >= 32 declined.
Built optimised and under AddressSanitizer + UBSan, run as a program of its own.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "tests", "syrk_plan", "plan_driver.cc")
OUT = os.path.join(ROOT, "build", "syrk_plan")


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


def _run(exe, env=None):
    """Exit status 0: every check holds; 2: every check but the balance bound, whose misses the
    driver lists as UNBALANCED lines (test_plan_balance)."""
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600,
                         env=env)
    text = run.stdout.decode(errors="replace")
    assert run.returncode in (0, 2), text[-6000:]
    assert "all plan checks passed" in text and "FAIL" not in text, text[-2000:]
    return text


def test_plan_invariants():
    text = _run(_build("plan_opt", ["-O2"]))
    # the headline plan: 16 bands of 28 groups and 64 diagonal-tile workgroups
    line = [ln for ln in text.splitlines() if ln.startswith("nb  8 n_pad  1000064")]
    assert line and " on 1 B  16 nwg 512 " in line[0], text[-2000:]


def test_plan_balance():
    """Every workgroup's modelled cost <= the mean + one off-diagonal step (64 slots), for every
    nb = 3 ... 12 and n_pad of the list (the driver lists a miss as an UNBALANCED line).  The
    planner prefers balanced deals: at (nb = 12, n_pad = 1000064), where 7 bands are all that fit
    and a band chunk alone (571528) is 194 above the mean over 512 workgroups, it levels 511
    workgroups at 572486 with second segments of 25 steps."""
    text = _run(_build("plan_opt", ["-O2"]))
    bad = [ln for ln in text.splitlines() if ln.startswith("UNBALANCED")]
    assert not bad, "\n".join(bad)


def test_plan_invariants_under_asan_ubsan():
    exe = _build("plan_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    text = _run(exe, env)
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-6000:]
