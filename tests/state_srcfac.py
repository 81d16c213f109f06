"""The states and fixtures of the source-factor tests (test infrastructure).

scripts/make_srcfac_cases.py hands the deterministic states of
tests/state_periodic.py (3-D, tree P) and tests/state2d.py (2-D Cartesian) to
the reference's own forward_euler with ``-fixes%source_factor=flux`` and
``-fixes%write_source_factor=t``, with and without
``-fixes%source_min_electrons_per_cell=5e4``, and commits what the reference
wrote (tests/golden/srcfac_<model>_<variant>.npz): dt_lim, the new densities
and the stored factor on the interiors of a fixed subset of the leaves, both
Heun stages, plus the electrons of the same step without the factor.

MODELS: name -> (ndim, exported case, state). The 3-D state is built for
either 3-D model by pointing state_periodic at the model's case.
"""
import contextlib
import os

import numpy as np

import golden
import state2d
import state_periodic as sp

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = {
    "test_3d": (3, "rtest_test_3d"),
    "test_3d_chem": (3, "rtest_test_3d_chem"),
    "test_2d": (2, "rtest_test_2d"),
    "s2d": (2, "case_s2d"),
}
VARIANTS = {"flux": -1.0, "min": 5e4}  # source_min_electrons_per_cell
MAX_BYTES = 900 * 1024  # of the arrays of one fixture file


@contextlib.contextmanager
def _sp_case(case):
    old, sp.CASE = sp.CASE, case
    try:
        yield
    finally:
        sp.CASE = old


def build_state(model):
    """(Case, AfTree, {iv: cc}, {ivf: fc}, dt, case dict) of `model`."""
    ndim, case = MODELS[model]
    if ndim == 3:
        with _sp_case(case):
            c, af, cc, fc = sp.build_state()
            d = sp.case_dict()
        return c, af, cc, fc, sp.DT, d
    c, af, cc, fc, dt = state2d.build_state(model)
    return c, af, cc, fc, dt, dict(c.d)


def stages(model):
    return sp.STAGES if MODELS[model][0] == 3 else state2d.STAGES


def stage_dt(model, k, dt):
    """The 3-D replay halves dt on the second stage (scripts/
    make_periodic_cases.py); the 2-D one keeps it (oracle/make_replay2d.py)."""
    return dt * (0.5 if (MODELS[model][0] == 3 and k == 1) else 1.0)


def kept_leaves(model, af, n_species):
    """The leaves a fixture keeps: every stride-th, the stride the smallest
    that keeps one file (two stages of every density and the factor, and the
    electrons without the factor) under MAX_BYTES."""
    leaves = af.leaves()
    per_leaf = 8 * af.nc ** MODELS[model][0] * 2 * (n_species + 2)
    stride = -(-per_leaf * len(leaves) // MAX_BYTES)
    return leaves[::max(1, stride)]


def load(model, variant):
    return np.load(os.path.join(HERE, "golden", "srcfac_%s_%s.npz" % (model, variant)))


def ionization(c):
    """reaction_type == ionization_reaction per reaction (m_chemistry.f90:14)."""
    n_reac = c.ia("n_species")[2]
    return [c.ia("reaction_%d" % n)[1] == 1 for n in range(1, n_reac + 1)]


def case_with_factor(d, variant, write=True):
    """The case dict with the driver's source-factor entries (and the srcfac
    variable appended to the registry when it is written)."""
    d = dict(d)
    d["source_factor"] = np.array(["flux"])
    d["source_min_electrons_per_cell"] = np.array([VARIANTS[variant]])
    if write:
        d["write_source_factor"] = np.array([1])
        d["cc_names"] = np.array(list(d["cc_names"]) + ["srcfac"])
    return d


def interior(a, ndim):
    return a[(slice(None),) + (slice(1, -1),) * ndim]


class Model:
    """What the numpy step needs of a fluid model: ndim, species_iv (the
    plasma species' cc variables), i_electron, i_efld, reactions (driver
    form), ionization, chem, td, N, dt_chemistry_nmin, td_energy_col, Tg,
    cylindrical, photo_species (1-based plasma slot), gas_fractions."""

    def __init__(self, **kw):
        self.dt_chemistry_nmin, self.td_energy_col, self.Tg = -1.0, 0, 300.0
        self.cylindrical, self.photo_species, self.gas_fractions = False, 0, ()
        self.__dict__.update(kw)


def model_of(sim):
    """The Model of an afh.driver.Simulation."""
    return Model(ndim=sim.ndim, species_iv=[sim.species_itree[n] for n in sim.plasma],
                 i_electron=sim.i_electron, i_efld=sim.i_efld, reactions=sim.reactions,
                 ionization=sim.ionization, chem=sim.chem, td=sim.td, N=sim.N,
                 dt_chemistry_nmin=sim.c.r("dt_chemistry_nmin"),
                 td_energy_col=max(0, sim.c.ia("td_cols")[4]),
                 Tg=sim.c.r("gas_temperature_value"), cylindrical=sim.cylindrical,
                 photo_species=sim.photo_species if sim.photoi else 0,
                 gas_fractions=sim.gas_fractions if sim.i_gas_dens else ())


def numpy_step(sim, dr, cc, F, stage, dt, boxes, factor=True, min_e=-1.0, last_step=True,
               lsf=None, photo=None, Ng=None, ion_F=(), r_min=None):
    """tests/srcfac_numpy.update_box over the leaf boxes `boxes` with the
    model `sim` (a Model or an afh.driver.Simulation): dr {box: spacings} (or
    an AfTree), cc {iv: tree-wide array}, F the tree-wide electron face flux,
    lsf / photo / Ng tree-wide arrays or None, ion_F [(plasma species slot,
    tree-wide face flux)], r_min {box: r_min} of a cylindrical tree. Returns
    {box: ([new interiors per plasma species], factor or None, chemistry
    limit)}."""
    import srcfac_numpy as sn
    m = sim if isinstance(sim, Model) else model_of(sim)
    if hasattr(dr, "dr"):
        dr, r_min = dr.dr, dr.r_min
    s_deriv, s_prev, w_prev, s_out = stage
    inner = (slice(1, -1),) * m.ndim
    iv_s = m.species_iv
    out = {}
    for b in boxes:
        def at(a):
            return None if a is None else a[b - 1][inner]
        out[b] = sn.update_box(
            [[at(cc[iv + q]) for iv in iv_s] for q in s_prev], w_prev,
            [at(cc[iv + s_deriv]) for iv in iv_s], at(cc[m.i_efld]), F[b - 1], dt, dr[b],
            m.reactions, m.chem, m.td, m.N,
            ionization=m.ionization if factor else None, min_electrons=min_e,
            e_index=iv_s.index(m.i_electron), last_step=last_step,
            dt_chemistry_nmin=m.dt_chemistry_nmin,
            mask=None if lsf is None else ~(at(lsf) <= 0.0), photo=at(photo),
            photo_s=(m.photo_species - 1) if photo is not None else 0, Ng=at(Ng),
            gas_fractions=m.gas_fractions if Ng is not None else (),
            r_min=r_min[b][0] if m.cylindrical else None,
            ions=[(sl, G[b - 1]) for sl, G in ion_F],
            td_energy_col=m.td_energy_col, Tg=m.Tg)
    return out


def flux_2d_numpy(sim, af, cc, fc, s_deriv):
    """The electron face flux of a 2-D Cartesian state as flux_upwind_tree and
    af_consistent_fluxes leave it (tests/ions2d_numpy.py), tree-wide."""
    import ions2d_numpy as inp
    a = cc[sim.i_electron + s_deriv].copy()
    h = af.nc // 2
    # af_restrict_ref_boundary: the children that touch a refinement boundary
    # (leaves, by the 2:1 balance) restricted into their parent's quadrant
    for p in range(1, af.highest_id + 1):
        if not af.in_use[p] or not af.has_children(p):
            continue
        for k, ch in enumerate(af.children[p]):
            if all(nb != inp.NO_BOX for nb in af.neighbors[ch][:4]):
                continue
            x = a[ch - 1][1:-1, 1:-1]
            i0, j0 = (k & 1) * h, (k >> 1) * h
            a[p - 1][1 + j0:1 + j0 + h, 1 + i0:1 + i0 + h] = 0.25 * (
                x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2])
    F = np.zeros((af.highest_id, 2, af.nc + 1, af.nc + 1))
    # af_gc2_box writes ghost layer 1 back into the box, level by level from
    # the coarsest: the prolongation at a refinement boundary reads the
    # coarse leaf's ghost cells as that left them
    leaves = sorted(af.leaves(), key=lambda b: af.lvl[b])
    for b in leaves:
        l1 = inp.gc2_layers(af, a, b)[0]
        g = a[b - 1]
        g[1:-1, 0], g[1:-1, -1], g[0, 1:-1], g[-1, 1:-1] = l1[0], l1[1], l1[2], l1[3]
    for b in leaves:
        P = inp.padded(af, a, b)
        F[b - 1] = inp.box_fluxes(np.array([P]), cc[sim.i_efld][b - 1], fc[sim.f_field][b - 1],
                                  af.dr[b], sim.td, 1 / sim.N, [], [-1])[0][0]
    return inp.consistent_fluxes(af, F, False)


__all__ = ["MODELS", "VARIANTS", "build_state", "stages", "stage_dt", "kept_leaves", "load",
           "ionization", "case_with_factor", "interior", "golden"]
