"""Mobile ions in libafivo_hip_2d.so, on the device: the ion list checks, the
fluxes of every flux species and both limits of afh_flux_upwind_tree against
tests/ions2d_numpy.py (bitwise), the per-face conductivity sum, the update
with the ions' divergences through every entry point (bitwise), conservation,
a regrid, and the two regression cases of programs/standard_2d with mobile
ions against the logs the reference committed.

Tree: 8^2 boxes, a 2 x 2 level 1 with the box at the origin refined once --
physical boundaries, same-level neighbours, refinement boundaries normal to
both axes (gc2 prolongation, consistent fluxes) and, cylindrical, the axis.
"""
import re

import numpy as np
import pytest

import cyl_numpy as cn
import golden
import ions2d_numpy as inp
from afh import capi
from afh.amr import AF_CYL, AF_XYZ, AfTree, DO_REF, KEEP_REF
from afh.driver import Case, Simulation

pytestmark = pytest.mark.gpu

PFMG = dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
CASE = "rtest_test_cyl_ion_motion"
PHOTO_CASE = "rtest_test_cyl_photoi_chem"
ERR_ARG = -1
EPS = np.finfo(np.float64).eps


def _code(exc):
    return int(re.search(r"failed \((-?\d+)\)", str(exc.value)).group(1))


def _refine(af, ix):
    """One af_adjust_refinement that refines the level-1 box at index ix."""
    def fn(ids):
        f = [DO_REF if af.lvl[b] == 1 and tuple(af.ix[b][:2]) == ix else KEEP_REF for b in ids]
        return np.array(f), np.zeros(len(ids), np.uint32)
    return af.adjust_refinement(fn)


def _af(cyl, case=CASE, nc=8):
    c = Case(golden.load(case))
    L, o = c.ra("domain_len"), c.ra("domain_origin")
    af = AfTree(nc, o + L, [2 * nc, 2 * nc], r_min=o, coord=AF_CYL if cyl else AF_XYZ)
    _refine(af, (1, 1))
    assert af.highest_lvl == 2 and len(af.leaves()) == 7
    return af


def _sim(cyl, n_ions, af=None, case=CASE, reactions=True, nc=8):
    """A Simulation of `case` bound to the two-level tree (or `af`) with the
    first n_ions of: the case's mobile ions, then every other charged species
    on face variables of its own. Each ion gets a mobility of its own."""
    d = dict(golden.load(case))
    d["coarse_grid_size_value"] = np.array([2 * nc, 2 * nc])
    d["box_size"] = np.array([nc])
    sim = Simulation(capi.hip_library_2d(), d, device=0, **PFMG)
    sim.af = af if af is not None else _af(cyl, case, nc)
    sim.cylindrical = cyl
    plasma_iv = [sim.species_itree[n] for n in sim.plasma]
    ions = list(sim.ions)
    mob = ions[0][2] if ions else 2.4e23
    have = {sp for sp, _, _ in ions}
    n_face = sim.n_var_face
    for sp in range(1, len(plasma_iv) + 1):
        if sp in have or plasma_iv[sp - 1] == sim.i_electron:
            continue
        if sim.species_charge[sim.plasma[sp - 1]] != 0:
            n_face += 1
            ions.append((sp, n_face, mob))
    assert len(ions) >= n_ions
    sim.ions = [(sp, fv, mob * (1 + 0.25 * q)) for q, (sp, fv, _) in enumerate(ions[:n_ions])]
    sim.n_var_face = max([sim.n_var_face] + [fv for _, fv, _ in sim.ions])
    if not reactions:
        sim.reactions = []
    sim._bind(sim._create_tree())
    assert sim.tree.coord == (capi.COORD_CYL if cyl else capi.COORD_XYZ)
    return sim


def _flux_vars(sim, s=0):
    """[(cc variable at state s, face variable, charge sign, species slot)] of
    the flux species, the electrons first."""
    plasma_iv = [sim.species_itree[n] for n in sim.plasma]
    out = [(sim.i_electron + s, sim.f_flux, -1.0, plasma_iv.index(sim.i_electron))]
    for sp, fv, _ in sim.ions:
        ch = sim.species_charge[sim.plasma[sp - 1]]
        out.append((plasma_iv[sp - 1] + s, fv, 1.0 if ch > 0 else -1.0, sp - 1))
    return out


def _shape(af):
    return (af.highest_id, af.nc + 2, af.nc + 2)


def _leaf_inner(af):
    m = np.zeros(_shape(af), bool)
    for b in af.leaves():
        m[b - 1, 1:-1, 1:-1] = True
    return m


def _random_state(sim, seed, s=0, field=3e6):
    """Random positive densities of every species at state s, a random |E| and
    a random face field of both signs."""
    af = sim.af
    rng = np.random.default_rng(seed)
    nf = af.nc + 1
    for iv in sim.densities:
        sim.tree.put_cc(iv + s, 1e15 * (0.2 + rng.random(_shape(af)) ** 2))
    sim.tree.put_cc(sim.i_efld, field * (0.1 + 2 * rng.random(_shape(af))))
    sim.tree.put_fc(sim.f_field, field * rng.standard_normal((af.highest_id, 2, nf, nf)))


def _restricted(af, a, p, cyl):
    """af_restrict_ref_boundary on box p: af_restrict_box of its children
    that touch a refinement boundary into p's interior ((nc, nc)); the other
    quadrants keep a's values."""
    nc = af.nc
    h = nc // 2
    out = a[p - 1][1:-1, 1:-1].copy()
    for k, c in enumerate(af.children[p]):
        if all(nb != inp.NO_BOX for nb in af.neighbors[c][:4]):
            continue
        x = a[c - 1][1:-1, 1:-1]
        c00, c10, c01, c11 = x[0::2, 0::2], x[0::2, 1::2], x[1::2, 0::2], x[1::2, 1::2]
        i0, j0 = (k & 1) * h, (k >> 1) * h
        if cyl:
            w1, w2 = cn.child_weights(af.r_min[p][0], af.dr[p][0], np.arange(i0 + 1, i0 + h + 1))
            r = 0.25 * (w1[None, :] * (c00 + c01) + w2[None, :] * (c10 + c11))
        else:
            r = 0.25 * (c00 + c10 + c01 + c11)
        out[j0:j0 + h, i0:i0 + h] = r
    return out


def _numpy_flux(sim, cyl):
    """The numpy statement on the tree's state as the flux call left it (ghost
    layer 1 and the restricted parent are read back and checked on the way):
    ({face variable: tree-wide F}, limits, per-leaf sigma and terms)."""
    af = sim.af
    fvs = _flux_vars(sim)
    a = [sim.tree.get_cc(iv) for iv, _, _, _ in fvs]
    E, Ef = sim.tree.get_cc(sim.i_efld), sim.tree.get_fc(sim.f_field)
    parents = [p for p in af.lvls[1]["ids"] if af.has_children(p)]
    assert parents
    for x in a:  # af_restrict_ref_boundary ran on every flux species
        for p in parents:
            want = _restricted(af, x, p, cyl)
            assert np.array_equal(x[p - 1][1:-1, 1:-1], want)
    mob = [m for _, _, m in sim.ions]
    q = [s for _, _, s, _ in fvs]
    F = np.zeros((len(fvs), af.highest_id, 2, af.nc + 1, af.nc + 1))
    cfl_max, sig_max, detail = -np.inf, -np.inf, {}
    for b in af.leaves():
        pads = []
        for x in a:
            P = inp.padded(af, x, b)
            # layer 1 is what the library wrote into the box
            g = x[b - 1]
            assert np.array_equal(P[2:-2, 1], g[1:-1, 0]) and np.array_equal(P[2:-2, -2], g[1:-1, -1])
            assert np.array_equal(P[1, 2:-2], g[0, 1:-1]) and np.array_equal(P[-2, 2:-2], g[-1, 1:-1])
            pads.append(P)
        Fb, cfl, sigma, terms = inp.box_fluxes(np.array(pads), E[b - 1], Ef[b - 1], af.dr[b],
                                               sim.td, 1 / sim.N, mob, q)
        F[:, b - 1] = Fb
        cfl_max = max(cfl_max, cfl.max())
        sig_max = max(sig_max, max(s.max() for s in sigma))
        detail[b] = (sigma, terms)
    for n in range(len(fvs)):
        inp.consistent_fluxes(af, F[n], cyl)
    return ({fv: F[n] for n, (_, fv, _, _) in enumerate(fvs)}, inp.limits(cfl_max, sig_max),
            detail)


def _leaf_faces(af):
    m = np.zeros((af.highest_id, 2, af.nc + 1, af.nc + 1), bool)
    for b in af.leaves():
        m[b - 1] = inp.face_valid(af.nc)
    return m


# ------------------------------------------------------------ 1. the ion list
def test_bad_ion_lists_are_refused():
    sim = _sim(True, 6)
    good = list(sim.ions)
    plasma_iv = [sim.species_itree[n] for n in sim.plasma]
    e_sp = plasma_iv.index(sim.i_electron) + 1
    sp0, fv0, mob = good[0]
    cases = [[(e_sp, fv0, mob)],                    # the electrons are no ion
             [(0, fv0, mob)],
             [(len(plasma_iv) + 1, fv0, mob)],      # no such species
             [(sp0, sim.f_flux, mob)],              # the electrons' flux variable
             [(sp0, 0, mob)],
             [(sp0, sim.n_var_face + 1, mob)],      # no such face variable
             [good[0]] * (capi.MAX_IONS + 1)]       # too many
    for ions in cases:
        sim.ions = ions
        with pytest.raises(capi.AfhError) as e:
            sim._bind(sim.tree)
        assert _code(e) == ERR_ARG, ions
    sim.ions = good
    sim._bind(sim.tree)
    sim.tree.close()


# --------------------------------------------------- 2. fluxes and the limits
@pytest.mark.parametrize("n_ions", [1, 6, 7])
@pytest.mark.parametrize("cyl", [False, True])
def test_fluxes_and_limits_bitwise(cyl, n_ions):
    _fluxes_and_limits(cyl, n_ions, 8)


@pytest.mark.parametrize("nc", [6, 12])
@pytest.mark.parametrize("cyl", [False, True])
def test_fluxes_and_limits_bitwise_box_size(cyl, nc):
    """Box sizes without kernels of their own (the t % nc decodes of the flux
    kernels and of k2_gc2), six ions of both signs."""
    _fluxes_and_limits(cyl, 6, nc)


def _fluxes_and_limits(cyl, n_ions, nc):
    sim = _sim(cyl, n_ions, nc=nc)
    af = sim.af
    assert len(sim.ions) == n_ions
    if n_ions >= 6:
        assert {s for _, _, s, _ in _flux_vars(sim)[1:]} == {-1.0, 1.0}
    _random_state(sim, 100 + n_ions)
    before = {iv: sim.tree.get_cc(iv) for iv in sim.densities}
    E, Ef = sim.tree.get_cc(sim.i_efld), sim.tree.get_fc(sim.f_field)
    lim = sim.fluid.flux_upwind_tree(0)
    ref, ref_lim, _ = _numpy_flux(sim, cyl)
    ok = _leaf_faces(af)
    for _, fv, _, _ in _flux_vars(sim):
        got = sim.tree.get_fc(fv)
        assert np.array_equal(got[ok], ref[fv][ok]), fv
        assert np.count_nonzero(got[ok]) > ok.sum() // 2
    print("cyl %s, %d ions: limits" % (cyl, n_ions), lim, ref_lim)
    assert lim == ref_lim
    # the electrons' flux and the CFL limit are those of a fluid without ions
    f_e = sim.tree.get_fc(sim.f_flux)
    sim.tree.close()
    sim0 = _sim(cyl, 0, nc=nc)
    assert sim0.ions == []
    for iv, x in before.items():
        sim0.tree.put_cc(iv, x)
    sim0.tree.put_cc(sim0.i_efld, E)
    sim0.tree.put_fc(sim0.f_field, Ef)
    lim0 = sim0.fluid.flux_upwind_tree(0)
    assert np.array_equal(sim0.tree.get_fc(sim0.f_flux)[ok], f_e[ok])
    assert lim0[0] == lim[0] and lim0[1] > lim[1]
    sim0.tree.close()


# ------------------------------------------------------------------ 3. sigma
@pytest.mark.parametrize("cyl", [False, True])
def test_sigma_is_folded_per_face(cyl):
    """The electrons peak in one level-1 leaf, the ion in another, and the
    third holds less of each but more of their sum: the dielectric limit is
    that of the per-face sum there, where no species has its own maximum."""
    sim = _sim(cyl, 1)
    af = sim.af
    nf = af.nc + 1
    # (with the field along +x and +y the electrons take a face's high side
    # and the positive ion its low side: placed so that no face between two
    # boxes pairs one species' peak with the other's)
    at_ix = {tuple(af.ix[b][:2]): b for b in af.lvls[1]["ids"]}
    A, B, C = at_ix[(1, 2)], at_ix[(2, 2)], at_ix[(2, 1)]
    assert sim.species_charge[sim.plasma[sim.ions[0][0] - 1]] > 0
    E0 = 2e6
    N_inv = 1 / sim.N
    mu_e = float(inp.lt_col(sim.td, 1, np.array(0.5 * (E0 + E0) * 1e21 * N_inv)) * N_inv)
    mu_i = sim.ions[0][2] * N_inv
    (iv_e, _, _, _), (iv_i, _, _, _) = _flux_vars(sim)
    ne = np.full(_shape(af), 1e15)
    ni = np.full(_shape(af), 1e15 * mu_e / mu_i)
    ne[A - 1] *= 3.0
    ni[B - 1] *= 3.0
    ne[C - 1] *= 2.5
    ni[C - 1] *= 2.5
    sim.tree.put_cc(iv_e, ne)
    sim.tree.put_cc(iv_i, ni)
    sim.tree.put_cc(sim.i_efld, np.full(_shape(af), E0))
    sim.tree.put_fc(sim.f_field, np.full((af.highest_id, 2, nf, nf), E0))
    lim = sim.fluid.flux_upwind_tree(0)
    _, ref_lim, detail = _numpy_flux(sim, cyl)
    sim.tree.close()
    assert lim == ref_lim
    tmax = [max(t[n].max() for b in detail for t in detail[b][1]) for n in range(2)]
    smax, where = max((s.max(), b) for b in detail for s in detail[b][0])
    assert where == C and smax > 1.5 * max(tmax) and smax < 0.9 * (tmax[0] + tmax[1])
    for d in range(2):
        s = detail[C][0][d]
        at = np.unravel_index(np.argmax(s), s.shape)
        assert all(detail[C][1][d][n][at] < tmax[n] for n in range(2))
    assert lim[1] == inp.EPS0 / (inp.ELEM_CHARGE * smax)


# ----------------------------------------------------------------- 4. update
def _expected_update(sim, cyl, prev, F, dt, add=None, mask=None):
    """{cc variable (state 0): prev + divergence of its flux on the leaf
    interiors} for the flux species; prev for the others. add: {species slot:
    array added before the divergence}; mask: cells that keep prev."""
    af = sim.af
    slot_of = {slot: fv for _, fv, _, slot in _flux_vars(sim)}
    plasma_iv = [sim.species_itree[n] for n in sim.plasma]
    out = {}
    for slot, iv in enumerate(plasma_iv):
        y = prev[iv].copy()
        for b in af.leaves():
            yb = prev[iv][b - 1][1:-1, 1:-1]
            if add is not None and slot in add:
                yb = yb + add[slot][b - 1][1:-1, 1:-1]
            if slot in slot_of:
                yb = inp.add_divergence(yb, F[slot_of[slot]][b - 1], dt, af.dr[b],
                                        af.r_min[b][0] if cyl else None)
            if mask is not None:
                yb = np.where(mask[b - 1][1:-1, 1:-1], prev[iv][b - 1][1:-1, 1:-1], yb)
            y[b - 1][1:-1, 1:-1] = yb
        out[iv] = y
    return out


def _random_fluxes(sim, seed, dt):
    af = sim.af
    rng = np.random.default_rng(seed)
    nf = af.nc + 1
    scale = 0.1 * 1e15 * min(af.dr[af.lvls[2]["ids"][0]]) / dt
    F = {}
    for _, fv, _, _ in _flux_vars(sim):
        F[fv] = scale * rng.standard_normal((af.highest_id, 2, nf, nf))
        sim.tree.put_fc(fv, F[fv])
    return F


@pytest.mark.parametrize("n_ions", [1, 6])
@pytest.mark.parametrize("cyl", [False, True])
def test_update_densities_bitwise(cyl, n_ions):
    """afh_flux_update_densities with the whole chemistry: the derivative
    state (1) is zero, so every source vanishes; each flux species ends as the
    previous state (0) plus its own divergence, the others unchanged; ghost
    cells and the refined box of the output state (2) are not written."""
    _update_densities(cyl, n_ions, 8)


@pytest.mark.parametrize("nc", [6, 12])
@pytest.mark.parametrize("cyl", [False, True])
def test_update_densities_bitwise_box_size(cyl, nc):
    _update_densities(cyl, 6, nc)


def _update_densities(cyl, n_ions, nc):
    sim = _sim(cyl, n_ions, nc=nc)
    af = sim.af
    dt = 2e-12
    _random_state(sim, 7)
    rng = np.random.default_rng(8)
    zero, sentinel = np.zeros(_shape(af)), rng.standard_normal(_shape(af))
    for iv in sim.densities:
        sim.tree.put_cc(iv + 1, zero)
        sim.tree.put_cc(iv + 2, sentinel)
    prev = {iv: sim.tree.get_cc(iv) for iv in sim.densities}
    F = _random_fluxes(sim, 9, dt)
    sim.fluid.flux_update_densities(dt, 1, [0], [1.0], 2, True)
    want = _expected_update(sim, cyl, prev, F, dt)
    inner = _leaf_inner(af)
    flux_iv = {iv for iv, _, _, _ in _flux_vars(sim)}
    assert len(flux_iv) == 1 + n_ions
    for iv in sim.densities:
        got = sim.tree.get_cc(iv + 2)
        assert np.array_equal(got[inner], want[iv][inner]), iv
        assert np.array_equal(got[~inner], sentinel[~inner]), iv
        assert np.array_equal(got[inner], prev[iv][inner]) == (iv not in flux_iv), iv
    sim.tree.close()


def _euler_case(sim, cyl, dt, fold, add=None, mask=None, last=True):
    """One chemistry-free forward Euler step (derivative state 0, previous
    state 2, output state 1) with the fluxes the step itself stores."""
    inner = _leaf_inner(sim.af)
    prev = {iv: sim.tree.get_cc(iv + 2) for iv in sim.densities}
    if fold:
        sim.fluid.forward_euler_fold(dt, 0, [2], [1.0], 1, last)
        lim = sim.fluid.fetch_step(last)[0]
    else:
        lim = sim.fluid.forward_euler(dt, 0, [2], [1.0], 1, last)
    F = {fv: sim.tree.get_fc(fv) for _, fv, _, _ in _flux_vars(sim)}
    ok = _leaf_faces(sim.af)
    for fv in F:
        assert np.count_nonzero(F[fv][ok]) > ok.sum() // 2
    want = _expected_update(sim, cyl, prev, F, dt, add, mask)
    flux_iv = {iv for iv, _, _, _ in _flux_vars(sim)}
    got = {}
    for iv in sim.densities:
        got[iv] = sim.tree.get_cc(iv + 1)
        assert np.array_equal(got[iv][inner], want[iv][inner]), iv
        if iv not in flux_iv and add is None:
            assert np.array_equal(got[iv][inner], prev[iv][inner]), iv
    return lim, got, F


@pytest.mark.parametrize("cyl", [False, True])
def test_forward_euler_and_fold_bitwise(cyl):
    """afh_fluid_forward_euler and the _fold / fetch_step form of a fluid
    without reactions: previous state + divergence for every flux species,
    the other species unchanged, the two forms equal in every density, flux
    and limit, and the fluxes those of afh_flux_upwind_tree."""
    sim = _sim(cyl, 6, reactions=False)
    dt = 1e-12
    _random_state(sim, 21)
    _random_state(sim, 22, s=2)
    lim_a, got_a, F_a = _euler_case(sim, cyl, dt, False)
    for iv in sim.densities:
        sim.tree.put_cc(iv + 1, np.zeros(_shape(sim.af)))
    lim_b, got_b, F_b = _euler_case(sim, cyl, dt, True)
    assert tuple(lim_a) == tuple(lim_b)
    for iv in got_a:
        assert np.array_equal(got_a[iv], got_b[iv])
    lim_c = sim.fluid.flux_upwind_tree(0)
    assert tuple(lim_c) == tuple(lim_a[:2])
    ref, ref_lim, _ = _numpy_flux(sim, cyl)
    assert ref_lim == lim_c
    ok = _leaf_faces(sim.af)
    for fv in F_a:
        assert np.array_equal(F_a[fv], F_b[fv])
        assert np.array_equal(sim.tree.get_fc(fv), F_a[fv])
        assert np.array_equal(F_a[fv][ok], ref[fv][ok])
    sim.tree.close()


def _photo_update(cyl, masked):
    """The photoionization deck with its photo_species mobile: the rate is
    added to the electrons and that ion before their divergences (y + dt *
    photo, then the flux terms); masked: a cell whose level set is <= 0 keeps
    the previous state, without the rate."""
    sim = _sim(cyl, 3, case=PHOTO_CASE, reactions=False)
    assert sim.photoi and sim.photo_species in [sp for sp, _, _ in sim.ions]
    af = sim.af
    dt = 1e-12
    _random_state(sim, 31)
    _random_state(sim, 32, s=2)
    photo = 1e26 * np.random.default_rng(33).random(_shape(af))
    sim.tree.put_cc(sim.i_photo, photo)
    mask = None
    if masked:
        lsf = np.random.default_rng(34).standard_normal(_shape(af))
        lsf[af.leaves()[0] - 1] = -1.0  # a leaf with no cell to update
        sim.tree.put_cc(sim.i_tmp, lsf)
        sim.fluid.set_update_mask(sim.i_tmp)
        mask = lsf <= 0
    e_slot = _flux_vars(sim)[0][3]
    add = {e_slot: dt * photo, sim.photo_species - 1: dt * photo}
    _, got, _ = _euler_case(sim, cyl, dt, False, add=add, mask=mask)
    inner = _leaf_inner(af)
    prev = sim.tree.get_cc(sim.i_electron + 2)
    if masked:
        assert (inner & mask).any() and (inner & ~mask).any()
        assert np.array_equal(got[sim.i_electron][inner & mask], prev[inner & mask])
        assert (got[sim.i_electron][inner & ~mask] != prev[inner & ~mask]).mean() > 0.9
    else:
        assert not np.array_equal(got[sim.i_electron][inner], prev[inner])
    sim.tree.close()


def test_update_with_photoionization():
    """Mobile ions with photoionization, cylindrical and Cartesian."""
    _photo_update(True, False)
    _photo_update(False, False)


def test_update_with_the_mask():
    """Cartesian, afh_fluid_set_update_mask: a cell whose level set is <= 0
    keeps the previous state for every species, ions included; the others get
    their divergences. Then the same with photoionization."""
    _mask_update()
    _photo_update(False, True)


def _mask_update():
    sim = _sim(False, 6, reactions=False)
    af = sim.af
    dt = 1e-12
    _random_state(sim, 41)
    _random_state(sim, 42, s=2)
    lsf = np.random.default_rng(43).standard_normal(_shape(af))
    lsf[af.leaves()[0] - 1] = -1.0  # a leaf with no cell to update
    sim.tree.put_cc(sim.i_tmp, lsf)
    sim.fluid.set_update_mask(sim.i_tmp)
    mask = lsf <= 0
    _, got, _ = _euler_case(sim, False, dt, False, mask=mask)
    inner = _leaf_inner(af)
    for iv, _, _, _ in _flux_vars(sim):
        prev = sim.tree.get_cc(iv + 2)
        assert np.array_equal(got[iv][inner & mask], prev[inner & mask])
        assert (got[iv][inner & ~mask] != prev[inner & ~mask]).mean() > 0.9
    sim.tree.close()


def test_cylindrical_mask_stays_refused():
    sim = _sim(True, 1, reactions=False)
    _random_state(sim, 5)
    sim.fluid.set_update_mask(sim.i_tmp)
    with pytest.raises(capi.AfhError) as e:
        sim.fluid.flux_update_densities(1e-12, 0, [0], [1.0], 1, False)
    assert _code(e) == -2
    sim.tree.close()


# ----------------------------------------------------------- 5. conservation
@pytest.mark.parametrize("cyl", [False, True])
def test_ions_are_conserved(cyl):
    """No face field on the domain walls, so no ion crosses them: one
    chemistry-free step conserves the volume-weighted sum (2 pi r in
    cylindrical coordinates) of every ion over the leaves. Bound: the
    rounding of the sums themselves, 8 eps x leaf cells x the largest term
    (each cell's update rounds a few times relative to its own term, and so
    does each of the two sums)."""
    sim = _sim(cyl, 6, reactions=False)
    af = sim.af
    nc = af.nc
    _random_state(sim, 51)
    # one state for both sides of a face between two boxes of a level: |E| in
    # the ghost cells from the neighbour, the face field single-valued (a
    # leaf's face next to the refined box takes the fine fluxes anyway)
    sim.tree.gc_tree(sim.i_efld)
    Ef = sim.tree.get_fc(sim.f_field)
    for b in range(1, af.highest_id + 1):
        if not af.in_use[b]:
            continue
        for nb in range(4):
            nid = af.neighbors[b][nb]
            d, low = nb >> 1, (nb & 1) == 0
            if nid < 0:
                if d == 0:
                    Ef[b - 1, 0, :, 0 if low else nc] = 0.0
                else:
                    Ef[b - 1, 1, 0 if low else nc, :] = 0.0
            elif nid > 0 and not low:
                if d == 0:
                    Ef[nid - 1, 0, :, 0] = Ef[b - 1, 0, :, nc]
                else:
                    Ef[nid - 1, 1, 0, :] = Ef[b - 1, 1, nc, :]
    sim.tree.put_fc(sim.f_field, Ef)
    dx = min(af.dr[af.lvls[2]["ids"][0]])
    mu_max = sim.td["rows_cols"][:, 0].max() / sim.N
    dt = 0.05 * dx / (mu_max * np.abs(Ef).max())
    sim.fluid.forward_euler(dt, 0, [0], [1.0], 1, False)

    def total(a):
        terms = []
        for b in af.leaves():
            w = af.dr[b][0] * af.dr[b][1]
            if cyl:
                w = w * cn.TWO_PI * cn.radius_cc(af.r_min[b][0], af.dr[b][0], nc)[None, :]
            terms.append((a[b - 1][1:-1, 1:-1] * w).ravel())
        t = np.concatenate(terms)
        return t.sum(), np.abs(t).max(), t.size

    for iv, fv, _, _ in _flux_vars(sim)[1:]:
        s0, big, n = total(sim.tree.get_cc(iv))
        s1, _, _ = total(sim.tree.get_cc(iv + 1))
        moved = np.abs(sim.tree.get_cc(iv + 1) - sim.tree.get_cc(iv))[_leaf_inner(af)].max()
        bound = 8 * EPS * n * big
        print("cyl %s ion %d: sum %.17g -> %.17g, |diff| %.3g, bound %.3g, largest change "
              "%.3g" % (cyl, iv, s0, s1, abs(s1 - s0), bound, moved))
        assert moved > 1e10
        assert abs(s1 - s0) <= bound
    sim.tree.close()


# ------------------------------------------------------------------ 6. regrid
@pytest.mark.parametrize("cyl", [False, True])
def test_flux_after_a_regrid(cyl):
    """afh_tree_regrid refining a second box, a new fluid on the new tree
    (its second ghost layers sized for it), a flux call: the fluxes of every
    flux variable and both limits equal those of a tree created in that shape
    and loaded with the same state."""
    sim = _sim(cyl, 6)
    _random_state(sim, 61)
    sim.fluid.flux_upwind_tree(0)
    info = _refine(sim.af, (2, 2))
    assert info.n_add == 4
    new = sim.tree.regrid(sim.af.topology())
    if cyl:
        new.set_coord(capi.COORD_CYL)
    old = sim.tree
    sim._bind(new)
    old.close()
    cc = {iv: sim.tree.get_cc(iv) for iv in range(1, sim.n_var_cell + 1)}
    fc = {fv: sim.tree.get_fc(fv) for fv in range(1, sim.n_var_face + 1)}
    lim = sim.fluid.flux_upwind_tree(0)
    got = {fv: sim.tree.get_fc(fv) for _, fv, _, _ in _flux_vars(sim)}
    sim.tree.close()
    af2 = _af(cyl)
    _refine(af2, (2, 2))
    assert af2.highest_id == sim.af.highest_id and len(af2.leaves()) == 10
    other = _sim(cyl, 6, af=af2)
    for iv, x in cc.items():
        other.tree.put_cc(iv, x)
    for fv, x in fc.items():
        other.tree.put_fc(fv, x)
    lim2 = other.fluid.flux_upwind_tree(0)
    assert lim == lim2
    ok = _leaf_faces(af2)
    for fv in got:
        assert np.array_equal(got[fv][ok], other.tree.get_fc(fv)[ok]), fv
        assert np.count_nonzero(got[fv][ok]) > ok.sum() // 2
    # and the numpy statement on the regridded shape
    ref, ref_lim, _ = _numpy_flux(other, cyl)
    assert ref_lim == lim2
    for fv in got:
        assert np.array_equal(got[fv][ok], ref[fv][ok]), fv
    other.tree.close()


# -------------------------------------------------------------- 7. time loops
# Both cases run whole (on an MI355X 4.3 s and 0.6 s per run). Measured maximum
# relative deviation from the reference's logs: 4.48e-8 and 4.26e-8,
# the logs' print precision; the bound is 10 x that, never above compare_logs'
# own 1e-5.
RTOL = {"rtest_test_cyl_ion_motion": 4.5e-7, "rtest_test_cyl_ion_motion_v2": 4.3e-7}


def _run_case(name):
    sim = Simulation(capi.hip_library_2d(), golden.load(name), device=0, **PFMG)
    assert sim.ndim == 2 and sim.cylindrical and len(sim.ions) == 6
    log = sim.run()
    sim.tree.close()
    return log


@pytest.mark.parametrize("name", sorted(RTOL))
def test_ion_motion_rtest_hip(name):
    """test_cyl_ion_motion.cfg and test_cyl_ion_motion_v2.cfg (10 ns, rows
    0 .. 10), each run whole. Every row is within compare_logs' criterion,
    the reference's own (rtol 1e-5, atol 1e-8), and within RTOL; `it` equal
    and `time` within 1e-12; a second run of test_cyl_ion_motion_v2 (the
    shorter of the two) is bitwise the first."""
    ref = golden.load(name)["rtest_log"]
    log = _run_case(name)
    assert log.shape == ref.shape
    rel = np.abs(log - ref) / np.maximum(np.abs(ref), 1e-300)
    print("%s: %d rows, max rel per row" % (name, len(log)), rel[:, 2:].max(axis=1),
          "max", rel[:, 2:].max())
    assert np.array_equal(log[:, 0], ref[:, 0])
    assert np.allclose(log[:, 1], ref[:, 1], rtol=1e-12, atol=0)
    assert np.allclose(log, ref, rtol=1e-5, atol=1e-8)
    bad = ~np.isclose(log, ref, rtol=RTOL[name], atol=1e-8)
    assert not bad.any(), (np.argwhere(bad)[:5], rel.max())
    if name.endswith("_v2"):
        assert np.array_equal(_run_case(name), log)
