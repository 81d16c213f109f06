#!/usr/bin/env python3
"""The mobile-ion regression cases of programs/standard_2d as fixtures.

tests/golden/rtest_test_cyl_ion_motion.npz and
rtest_test_cyl_ion_motion_v2.npz: the set-up the reference's own initializers
export for tests/test_cyl_ion_motion.cfg and tests/test_cyl_ion_motion_v2.cfg
(the NDIM = 2 export_case harness, make -C oracle _ref/2d/export_case; it
dumps n_mobile_ions, flux_species, flux_variables, flux_species_charge_sign
and ion_mobilities), packed with the committed <name>_rtest.log exactly as
oracle/make_cases.py packs test_2d. Run in the build container, where the
reference is mounted:

    make -C oracle _ref/2d/export_case
    python3 scripts/make_ions2d_cases.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import make_cases  # noqa: E402  (run / parse_dump)

CASES_IONS_2D = ["test_cyl_ion_motion", "test_cyl_ion_motion_v2"]


def main():
    only = set(sys.argv[1:])
    make_cases.run(os.path.join(REPO, "oracle", "_ref", "2d", "export_case"),
                   make_cases.TESTS_2D, CASES_IONS_2D, {}, only)


if __name__ == "__main__":
    main()
