"""The normal stream (sparsergps_amd/csrc/sgp_rng.h, defined in include/sgp.h) without a GPU.

The header is HIP-free, so tests/joint/rng_driver.cc runs the generator on the host: the three
Philox4x32-10 known answers, its normals against the numpy restatement (tests/joint_oracle.py) at
1e-13 absolute for both streams, and the moments of 2^20 normals within five standard errors --
asserted of the oracle first, then of the driver.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import joint_oracle as JO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "tests", "joint", "rng_driver.cc")
OUT = os.path.join(ROOT, "build", "joint")

# (counter, key, output) of Philox4x32-10
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.fixture(scope="module")
def exe():
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "rng_driver")
    res = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", DRV, "-o",
                          path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert res.returncode == 0, res.stdout.decode(errors="replace")[-4000:]
    return path


def _run(exe, text, env=None):
    run = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300, env=env)
    err = run.stderr.decode(errors="replace")
    assert run.returncode == 0, err[-4000:]
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
    return run.stdout.decode()


def _driver_normals(exe, seed, stream, S, n):
    out = np.array(_run(exe, "N %d %d %d %d\n" % (seed, stream, S, n)).split(), dtype=np.float64)
    assert out.size == S * n
    return out.reshape(S, n)


def test_philox_known_answers_oracle():
    for ctr, key, want in KAT:
        got = tuple(int(w[0]) for w in JO.philox4x32(ctr, key))
        assert got == want, (ctr, key, [hex(v) for v in got])


def test_philox_known_answers_driver(exe):
    text = "".join("K %x %x %x %x %x %x\n" % (*ctr, *key) for ctr, key, _ in KAT)
    lines = _run(exe, text).strip().split("\n")
    assert len(lines) == len(KAT)
    for line, (_, _, want) in zip(lines, KAT):
        assert tuple(int(v, 16) for v in line.split()) == want, line


@pytest.mark.parametrize("stream", [0, 1])
@pytest.mark.parametrize("S,n", [(3, 5), (257, 130)])
def test_driver_normals_equal_the_oracle(exe, S, n, stream):
    seed = 0x1234567890abcdef
    ref = JO.normals(seed, stream, S, n)
    got = _driver_normals(exe, seed, stream, S, n)
    err = np.abs(got - ref).max()
    print("rng_driver: stream %d, (S, n) = (%d, %d): max |z - oracle| = %.3g" % (stream, S, n, err))
    assert err <= 1e-13


def test_driver_under_asan_ubsan():
    """The generator as a program of its own under AddressSanitizer + UBSan (the unsigned
    wrap-around of the Philox key schedule is defined behaviour and must stay silent)."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "rng_driver_san")
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                          "-fsanitize=address,undefined", "-fno-sanitize-recover=all", DRV, "-o",
                          path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert res.returncode == 0, res.stdout.decode(errors="replace")[-4000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    seed = 0xffffffffffffffff
    text = "K ffffffff ffffffff ffffffff ffffffff ffffffff ffffffff\nN %d 0 7 9\nN %d 1 7 9\n" % (
        seed, seed)
    out = _run(path, text, env).split()
    assert [int(v, 16) for v in out[:4]] == list(KAT[1][2])
    got = np.array(out[4:], dtype=np.float64)
    ref = np.concatenate([JO.normals(seed, 0, 7, 9).reshape(-1),
                          JO.normals(seed, 1, 7, 9).reshape(-1)])
    assert np.abs(got - ref).max() <= 1e-13


def test_streams_and_seeds_differ():
    a = JO.normals(7, 0, 4, 6)
    assert not np.any(a == JO.normals(7, 1, 4, 6))
    assert not np.any(a == JO.normals(8, 0, 4, 6))
    # the high half of the seed is the second key word
    assert not np.any(a == JO.normals(7 + (1 << 32), 0, 4, 6))
    # a pair shares one counter: rows 2k and 2k + 1 of a draw (stream 0), draws 2q and 2q + 1 of a
    # row (stream 1); a later chunk continues the stream
    assert np.array_equal(JO.normals(7, 0, 9, 6)[5:], JO.normals(7, 0, 4, 6, s0=5))
    assert np.array_equal(JO.normals(7, 1, 9, 6)[4:], JO.normals(7, 1, 5, 6, s0=4))


def _moments_ok(z, label):
    N = z.size
    m1, m2, m4 = z.mean(), (z * z).mean(), (z ** 4).mean()
    print("%s: N = %d, mean %.3g, second moment %.6g, fourth moment %.6g" % (label, N, m1, m2, m4))
    # standard errors of the sample moments of a standard normal: var z = 1, var z^2 = 2,
    # var z^4 = E z^8 - 9 = 96
    assert abs(m1) <= 5.0 / math.sqrt(N)
    assert abs(m2 - 1.0) <= 5.0 * math.sqrt(2.0 / N)
    assert abs(m4 - 3.0) <= 5.0 * math.sqrt(96.0 / N)
    assert np.all(np.isfinite(z)) and np.abs(z).max() < 8.58   # sqrt(-2 log 2^-53) = 8.57


@pytest.mark.parametrize("stream", [0, 1])
def test_moments_of_2_to_20_normals(exe, stream):
    S = n = 1024
    ref = JO.normals(2, stream, S, n)
    _moments_ok(ref, "oracle stream %d" % stream)
    got = _driver_normals(exe, 2, stream, S, n)
    _moments_ok(got, "driver stream %d" % stream)
    assert np.abs(got - ref).max() <= 1e-13
