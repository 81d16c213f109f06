#!/usr/bin/env python3
"""The electrode regression cases of programs/standard_2d as fixtures.

tests/golden/rtest_test_2d_pos_electrode.npz, rtest_test_2d_neg_electrode.npz,
rtest_test_2d_pos_electrode_photoi.npz and
rtest_test_2d_neg_electrode_photoi.npz: the set-up the reference's own
initializers export for tests/test_2d_{pos,neg}_electrode[_photoi].cfg (the
NDIM = 2 export_case harness, make -C oracle _ref/2d/export_case; it dumps
use_electrode, the rod's end points and radius and every photoi% setting),
packed with the committed <name>_rtest.log exactly as oracle/make_cases.py
packs test_2d. Data only, about 90 KB each. Run in the build container, where
the reference is mounted:

    make -C oracle _ref/2d/export_case
    python3 scripts/make_electrode2d_cases.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import make_cases  # noqa: E402  (run / parse_dump)

CASES_ELECTRODE_2D = ["test_2d_pos_electrode", "test_2d_neg_electrode",
                      "test_2d_pos_electrode_photoi", "test_2d_neg_electrode_photoi"]


def main():
    only = set(sys.argv[1:])
    make_cases.run(os.path.join(REPO, "oracle", "_ref", "2d", "export_case"),
                   make_cases.TESTS_2D, CASES_ELECTRODE_2D, {}, only)


if __name__ == "__main__":
    main()
