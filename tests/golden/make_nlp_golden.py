"""Writes tests/golden/nlp_grid.npz: the 612-case (family, y, mu, s2, m) grid of
tests/nlp_oracle.py plus its three named rows, with the 50-digit mpmath nlp rounded to double.

    python tests/golden/make_nlp_golden.py

Takes about nine minutes on one core (50-digit tanh-sinh quadrature over eleven sub-ranges per
row); tests/test_nlp_oracle.py recomputes a few rows on every run.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nlp_oracle as O  # noqa: E402


def main():
    fam, y, mu, s2, m = O.grid_cases()
    nlp = np.array([O.mp_nlp(O.FAMILY_NAMES[int(f)], yy, a, b, c)
                    for f, yy, a, b, c in zip(fam, y, mu, s2, m)])
    assert np.all(np.isfinite(nlp))
    out = os.path.join(HERE, "nlp_grid.npz")
    np.savez_compressed(out, fam=fam, y=y, mu=mu, s2=s2, m=m, nlp=nlp)
    print(out, nlp.size, "rows", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
