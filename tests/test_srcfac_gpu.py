"""The flux-based source factor (fixes%source_factor = flux) on the GPU, in
libafivo_hip.so (k_update's SF instantiations) and libafivo_hip_2d.so
(k2_update's SRCFAC option).

* The reference's own step (tests/golden/srcfac_*.npz, scripts/
  make_srcfac_cases.py): both Heun stages, with and without the electron
  threshold, two 3-D and two 2-D models; dt_lim, the densities and the stored
  factor on the fixtures' leaves. Bitwise for test_3d / test_2d (no exp or pow
  in their rates); 1e-13 relative otherwise (tests/test_2d_replay.py's bar for
  last-ulp libm differences), the count of values not bitwise printed.
* tests/srcfac_numpy.py (held to the same fixtures on the CPU,
  tests/test_srcfac_cpu.py) where no fixture reaches: cylindrical trees with
  photoionization and mobile ions, box size 6, a variable gas density, the
  update mask. The numpy step takes the face fluxes the device's
  flux_upwind_tree left, so the update alone is compared -- bitwise when the
  model's rates are tabulated, constant or linear.
* The paths around it: the fused 3-D step is not taken with the factor on,
  AFH_SRCFAC_NONE restores the step bit for bit, two thread ranks equal one,
  and every argument check.
"""
import ctypes as C
import re

import numpy as np
import pytest

import golden
import state_srcfac as ss
from afh import capi
from afh.amr import AF_CYL, AF_XYZ, AfTree, DO_REF, KEEP_REF
from afh.driver import Case, Simulation
from afh.model import Fluid, Tree
from afh.streamer import FV, IV, StreamerCase, seed_state, standard_reactions, tables_from
from afh.tree import uniform_tree

pytestmark = pytest.mark.gpu

DEVICE = 0
PFMG = dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
ERR_ARG, ERR_STATE = -1, -4
CASES = [(m, v) for m in ss.MODELS for v in ss.VARIANTS]
EXACT_RATES = (capi.RATE_TABULATED_FIELD, capi.RATE_CONSTANT, capi.RATE_LINEAR)


def _lib(ndim):
    return capi.hip_library() if ndim == 3 else capi.hip_library_2d()


def _code(exc):
    """The AFH_ERR_* code of an AfhError (or of pytest's record of one)."""
    return int(re.search(r"failed \((-?\d+)\)", str(getattr(exc, "value", exc))).group(1))


STAGES = ss.sp.STAGES  # the two Heun sub-steps (s_deriv, s_prev, w_prev, s_out)


def _bitwise(reactions):
    return all(r.get("rate_type", capi.RATE_TABULATED_FIELD) in EXACT_RATES for r in reactions)


def _close(a, b, exact, what):
    """a == b (exact), else to 1e-13 relative; the count of values not bitwise."""
    n = int(np.count_nonzero(a != b))
    if exact:
        assert n == 0, (what, n, float(np.max(np.abs(a - b))))
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))
        assert rel.max() <= 1e-13, (what, float(rel.max()))
    return n


# ------------------------------------------------- the reference's fixtures
@pytest.fixture(scope="module")
def states():
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = ss.build_state(model)
        return cache[model]
    return get


@pytest.mark.parametrize("model,variant", CASES)
def test_step_equals_the_reference(states, monkeypatch, model, variant):
    monkeypatch.setenv("AFH_FACES_FROM_PHI", "0")  # the stored face field, as the reference
    ndim = ss.MODELS[model][0]
    c, af, cc, fc, dt0, d = states(model)
    fx = ss.load(model, variant)
    li = fx["leaves"] - 1
    inner = (slice(None),) + (slice(1, -1),) * ndim
    n_diff = 0
    for k, (s_deriv, s_prev, w_prev, s_out) in enumerate(ss.stages(model)):
        sim = Simulation(_lib(ndim), ss.case_with_factor(d, variant), device=0)
        sim.af = af
        sim._bind(sim._create_tree())
        assert not sim.faces_from_phi and sim.i_srcfac == len(cc) + 1
        for iv, a in cc.items():
            sim.tree.put_cc(iv, a)
        for ivf, a in fc.items():
            sim.tree.put_fc(ivf, a)
        exact = _bitwise(sim.reactions)
        lim = sim.fluid.forward_euler(ss.stage_dt(model, k, dt0), s_deriv, s_prev, w_prev,
                                      s_out, True)
        ours = min(sim.dt_max, min(lim[0] * sim.cfl, lim[1], lim[2], lim[3]))
        ref_lim = float(fx["dt_lim_%d" % (k + 1)][0])
        print(model, variant, "stage", k + 1, "dt_lim", ours, ref_lim)
        if exact:
            assert ours == ref_lim
        else:
            assert abs(ours - ref_lim) <= 1e-13 * ref_lim
        s = sim.tree.get_cc(sim.i_srcfac)[li][inner]
        assert np.array_equal(s, fx["srcfac_%d" % (k + 1)]), \
            (k, int(np.count_nonzero(s != fx["srcfac_%d" % (k + 1)])))
        for q, iv in enumerate(sim.densities):
            mine = sim.tree.get_cc(iv + s_out)[li][inner]
            n_diff += _close(mine, fx["dens_%d" % (k + 1)][q], exact,
                             (k, sim.cc_names[iv - 1]))
        # and the step does differ from the one without the factor
        e = sim.tree.get_cc(sim.i_electron + s_out)[li][inner]
        assert np.mean(np.abs(e / fx["off_e_%d" % (k + 1)] - 1) > 1e-10) >= 0.20
        sim.tree.close()
    print("%s %s: %d densities not bitwise" % (model, variant, n_diff))


# ------------------------------------------- the update against the numpy step
def _two_level(case, nc, ndim, cyl=False):
    """2^ndim level-1 boxes of nc^ndim, the last of them refined."""
    c = Case(golden.load(case))
    L, o = c.ra("domain_len"), c.ra("domain_origin")
    af = AfTree(nc, o + L, [2 * nc] * ndim, r_min=o, coord=AF_CYL if cyl else AF_XYZ)

    def fn(ids):
        f = [DO_REF if af.lvl[b] == 1 and all(x == 2 for x in af.ix[b][:ndim]) else KEEP_REF
             for b in ids]
        return np.array(f), np.zeros(len(ids), np.uint32)
    af.adjust_refinement(fn)
    assert af.highest_lvl == 2 and len(af.leaves()) == 2 ** (ndim + 1) - 1
    return af


def _sim(case, nc, ndim, variant, cyl=False, n_ions=0):
    """A Simulation of `case` on the two-level tree with the factor of
    `variant` (None: the srcfac variable registered, the factor never set)."""
    d = dict(golden.load(case))
    d["coarse_grid_size_value"] = np.array([2 * nc] * ndim)
    d["box_size"] = np.array([nc])
    d = ss.case_with_factor(d, variant or "flux")
    if variant is None:
        d["source_factor"] = np.array(["none"])
    sim = Simulation(_lib(ndim), d, device=DEVICE, **(PFMG if ndim == 2 else {}))
    sim.af = _two_level(case, nc, ndim, cyl)
    sim.cylindrical = cyl
    # mobile ions: the first charged species after the electrons, on face
    # variables of their own
    if n_ions:
        plasma_iv = [sim.species_itree[n] for n in sim.plasma]
        ions, n_face = [], sim.n_var_face
        for sp in range(1, len(plasma_iv) + 1):
            if plasma_iv[sp - 1] != sim.i_electron and sim.species_charge[sim.plasma[sp - 1]] and \
                    len(ions) < n_ions:
                n_face += 1
                ions.append((sp, n_face, 2.4e23 * (1 + 0.25 * len(ions))))
        assert len(ions) == n_ions
        sim.ions, sim.n_var_face = ions, n_face
    sim._bind(sim._create_tree())
    if sim.faces_from_phi:  # these tests give the face field, not phi
        sim.fluid.set_field_source(0)
    sim.i_sf = sim.cc_names.index("srcfac") + 1
    return sim


def _random_state(sim, seed, field=3e6):
    af, rng = sim.af, np.random.default_rng(seed)
    shp = (af.highest_id,) + (af.nc + 2,) * sim.ndim
    fshp = (af.highest_id, sim.ndim) + (af.nc + 1,) * sim.ndim
    for iv in sim.densities:
        for s in (0, 1):
            # (some cells below the electron threshold of the variant `min`)
            sim.tree.put_cc(iv + s, 1e15 * (0.2 + rng.random(shp)) ** 4)
    sim.tree.put_cc(sim.i_efld, field * (0.1 + 2 * rng.random(shp)))
    sim.tree.put_fc(sim.f_field, field * rng.standard_normal(fshp))
    if sim.photoi:
        sim.tree.put_cc(sim.i_photo, 1e24 * rng.random(shp))


def _update_equals_numpy(sim, stage, dt, variant, lsf=None):
    """flux_upwind_tree, then flux_update_densities on the device against the
    numpy step with the device's fluxes: densities, the stored factor, the
    chemistry limit. Returns the factor on the leaves."""
    s_deriv, s_prev, w_prev, s_out = stage
    af, t = sim.af, sim.tree
    sim.fluid.flux_upwind_tree(s_deriv)
    F = t.get_fc(sim.f_flux)
    ion_F = [(sp - 1, t.get_fc(fv)) for sp, fv, _ in sim.ions]
    ivs = {iv + s for iv in sim.densities for s in set(s_prev) | {s_deriv}} | {sim.i_efld}
    cc = {iv: t.get_cc(iv) for iv in ivs}
    photo = t.get_cc(sim.i_photo) if sim.photoi else None
    t.put_cc(sim.i_srcfac, np.full(cc[sim.i_efld].shape, -7.0))
    lim = sim.fluid.flux_update_densities(dt, s_deriv, s_prev, w_prev, s_out, True)
    leaves = af.leaves()
    want = ss.numpy_step(sim, af, cc, F, stage, dt, leaves, min_e=ss.VARIANTS[variant],
                         photo=photo, ion_F=ion_F, lsf=lsf)
    exact = _bitwise(sim.reactions)
    inner = (slice(1, -1),) * sim.ndim
    got_s = t.get_cc(sim.i_srcfac)
    for b in leaves:
        ys, s, _ = want[b]
        if s is None:  # a wholly masked box: untouched
            assert np.all(got_s[b - 1][inner] == -7.0)
        else:
            assert np.array_equal(got_s[b - 1][inner], s), b
        for q, iv in enumerate(ss.model_of(sim).species_iv):
            _close(t.get_cc(iv + s_out)[b - 1][inner], ys[q], exact, (b, iv))
    want_lim = min(w[2] for w in want.values())
    assert lim[0] == want_lim if exact else abs(lim[0] - want_lim) <= 1e-13 * want_lim
    return np.stack([got_s[b - 1][inner] for b in leaves if want[b][1] is not None])


def _factor_is_exercised(s, variant):
    assert (s == 1).any() and ((s > 0) & (s < 1)).mean() >= 0.10
    if variant == "min":
        assert (s == 0).any()


@pytest.mark.parametrize("what", ["plain", "photo", "ions"])
def test_cylindrical_update_equals_numpy(what):
    case = {"plain": "rtest_test_2d", "photo": "rtest_test_2d_photoi",
            "ions": "rtest_test_2d"}[what]
    sim = _sim(case, 8, 2, "min", cyl=True, n_ions=2 if what == "ions" else 0)
    assert sim.tree.coord == capi.COORD_CYL and sim.photoi == (what == "photo")
    _random_state(sim, 11)
    for stage in STAGES:
        s = _update_equals_numpy(sim, stage, 1e-12, "min")
        _factor_is_exercised(s, "min")
    sim.tree.close()


@pytest.mark.parametrize("ndim,variant", [(3, "flux"), (3, "min"), (2, "flux"), (2, "min")])
def test_box_size_6_equals_numpy(ndim, variant):
    """n_cell 6 has no kernel of its own in either library: the general
    decode, on a two-level tree."""
    sim = _sim("rtest_test_3d" if ndim == 3 else "rtest_test_2d", 6, ndim, variant)
    _random_state(sim, 5 + ndim)
    for stage in STAGES:
        s = _update_equals_numpy(sim, stage, 1e-12, variant)
        _factor_is_exercised(s, variant)
    sim.tree.close()


def test_chemistry_model_with_ions_3d_equals_numpy():
    """The 3-D update with mobile ions and the temperature rate forms (the
    SLOW instantiation), ionization reactions a strict subset."""
    sim = _sim("rtest_test_3d_chem", 8, 3, "min", n_ions=2)
    assert 0 < sum(sim.ionization) < len(sim.ionization) and not _bitwise(sim.reactions)
    _random_state(sim, 17)
    s = _update_equals_numpy(sim, STAGES[1], 1e-12, "min")
    _factor_is_exercised(s, "min")
    sim.tree.close()


# --------------------------------------------------- variable gas density
NP_, N0, FRAC = 64, 2.414e25, (0.79, 0.21)


def _gas_case(seed=3):
    """tests/test_gas_density.py's case with a ninth variable for the factor:
    a two-level uniform tree (64 leaves of 4^3), e, M+, M- (2 states each),
    |E| (7), N (8) varying by +-40 %; N2 + e -> 2 e + M+ (linear rate, the
    ionization), O2 + e -> M- (constant)."""
    X = np.linspace(0.0, 1000.0, NP_)
    td = {"rows_cols": np.stack([1e24 * (1 + X / 500), 1e24 + X * 1e20], axis=1), "x_min": 0.0,
          "inv_fac": (NP_ - 1) / 1000.0}
    chem = {"rows_cols": np.stack([1e-16 * (1 + X / 100)], axis=1), "x_min": 0.0,
            "inv_fac": (NP_ - 1) / 1000.0}
    rng = np.random.default_rng(seed)
    topo = uniform_tree(4, (8, 8, 8), (2e-3, 2e-3, 2e-3), 2)
    t = Tree(capi.hip_library(), topo, 9, 2, device=0)
    neu = [(capi.BC_NEUMANN, 0.0)] * 6
    for iv in range(1, 10):
        t.set_cc_methods(iv, neu, capi.RB_GC_INTERP_LIM)
    shp = t.cc_shape
    for iv, a in ((1, 1e15), (3, 1e15), (5, 1e14)):
        t.put_cc(iv, a * (0.2 + rng.random(shp)) ** 4)
        t.put_cc(iv + 1, np.zeros(shp))
    t.put_cc(7, 3e6 * (1 + rng.random(shp)))
    t.put_cc(8, N0 * (0.6 + 0.8 * rng.random(shp)))
    t.put_fc(2, 3e6 * (rng.random(t.fc_shape) - 0.5))
    t.put_fc(1, np.zeros(t.fc_shape))
    for iv in (1, 7, 8):
        t.gc_tree(iv)
    g = len(FRAC)
    reac = [{"rate_type": capi.RATE_LINEAR, "c": [1.0e-18, 50.0], "rate_factor": 1.0,
             "ix_in": [1, g + 1], "ix_out": [g + 1, g + 2], "mult_out": [2, 1]},
            {"rate_type": capi.RATE_CONSTANT, "c": [2.0e-17], "rate_factor": 1.0,
             "ix_in": [2, g + 1], "ix_out": [g + 3], "mult_out": [1]}]
    f = Fluid(t, [1, 3, 5], [-1, 1, -1], 1, 7, 1, 2, N0, td, chem, reac,
              limiter=capi.LIM_KOREN, i_gas_dens=8, gas_fractions=FRAC)
    m = ss.Model(ndim=3, species_iv=[1, 3, 5], i_electron=1, i_efld=7, reactions=reac,
                 ionization=[True, False], chem=chem, td=td, N=N0, gas_fractions=FRAC)
    return t, f, topo, m


@pytest.mark.parametrize("variant", ["flux", "min"])
def test_variable_gas_density_equals_numpy(variant):
    """GAS: mu = LT(E / N) / N per cell, the gas species in the products."""
    t, f, topo, m = _gas_case()
    leaves = [int(b) for b in topo["lvl_leaves_2"]]
    dr = {b: topo["meta_dr"][b - 1] for b in leaves}
    # the threshold of `min` on this tree's 62.5 um cells: the median
    # electron count of its cells, so that half of them are cleared
    ne = np.stack([t.get_cc(1)[b - 1][1:-1, 1:-1, 1:-1] for b in leaves])
    min_e = float(np.median(ne) * min(dr[leaves[0]]) ** 3) if variant == "min" else -1.0
    f.set_source_factor(capi.SRCFAC_FLUX, m.ionization, min_e, 9)
    f.flux_upwind_tree(0)
    F = t.get_fc(1)
    cc = {iv: t.get_cc(iv) for iv in (1, 3, 5, 7, 8)}
    dt, stage = 1e-12, (0, [0], [1.0], 1)
    lim = f.flux_update_densities(dt, 0, [0], [1.0], 1, True)
    want = ss.numpy_step(m, dr, cc, F, stage, dt, leaves, min_e=min_e, Ng=cc[8])
    got_s = t.get_cc(9)
    for b in leaves:
        ys, s, _ = want[b]
        assert np.array_equal(got_s[b - 1][1:-1, 1:-1, 1:-1], s), b
        for q, iv in enumerate(m.species_iv):
            assert np.array_equal(t.get_cc(iv + 1)[b - 1][1:-1, 1:-1, 1:-1], ys[q]), (b, iv)
    assert lim[0] == min(w[2] for w in want.values())
    s = np.stack([got_s[b - 1][1:-1, 1:-1, 1:-1] for b in leaves])
    if variant == "flux":
        _factor_is_exercised(s, variant)
    else:
        assert 0.3 < (s == 0).mean() < 0.7 and (s == 1).any() and ((s > 0) & (s < 1)).any()
    t.close()


# ---------------------------------------------------------- the update mask
def _rod_case():
    g = golden.load("rod8")
    c = golden.make_case(capi.hip_library(), g, coarse_cycles=12, device=0)
    golden.upload(c, {**golden.stage_outputs(g, "init"), **golden.stage_outputs(g, "rhs")})
    c.field_compute(0, check_residual=False)
    td, chem = tables_from(g)
    m = ss.Model(ndim=3, species_iv=[IV["e"], IV["pos"], IV["neg"]], i_electron=IV["e"],
                 i_efld=IV["efld"], reactions=standard_reactions(), ionization=[True, False],
                 chem=chem, td=td, N=c.n_gas)
    return g, c, m


def test_update_mask_equals_numpy_and_skips_masked_boxes():
    """The rod electrode's level set as update mask: masked cells of a box
    with gas cells get a factor too; a wholly masked box keeps i_srcfac."""
    g, c, m = _rod_case()
    t = c.tree
    i_lsf, i_sf = golden.IVS["lsf"], IV["e"] + 2  # (the electrons' unused third state)
    leaves = [int(b) for l in range(1, int(g["highest_lvl"]) + 1) for b in g["lvl_leaves_%d" % l]]
    lsf = t.get_cc(i_lsf)
    cut = [b for b in leaves if (lsf[b - 1][1:-1, 1:-1, 1:-1] <= 0).any()
           and (lsf[b - 1][1:-1, 1:-1, 1:-1] > 0).any()]
    assert cut
    # one leaf wholly inside the electrode
    lsf[leaves[-1] - 1] = -1.0
    t.put_cc(i_lsf, lsf)
    c.fluid.set_update_mask(i_lsf)
    c.fluid.set_source_factor(capi.SRCFAC_FLUX, m.ionization, -1.0, i_sf)
    c.fluid.flux_upwind_tree(0)
    # (the solved state is drift dominated, factor 1 everywhere: scale the
    # fluxes down at random so that the factor takes every value)
    F = t.get_fc(FV["flux"]) * np.random.default_rng(7).random(t.fc_shape)
    t.put_fc(FV["flux"], F)
    cc = {iv: t.get_cc(iv) for iv in m.species_iv + [m.i_efld]}
    t.put_cc(i_sf, np.full(lsf.shape, -7.0))
    dt, stage = 1e-12, (0, [0], [1.0], 1)
    lim = c.fluid.flux_update_densities(dt, 0, [0], [1.0], 1, True)
    dr = {b: g["meta_dr"][b - 1] for b in leaves}
    want = ss.numpy_step(m, dr, cc, F, stage, dt, leaves, lsf=lsf)
    got_s = t.get_cc(i_sf)
    for b in leaves:
        ys, s, _ = want[b]
        mine = got_s[b - 1][1:-1, 1:-1, 1:-1]
        if s is None:
            assert b == leaves[-1] and np.all(mine == -7.0)
        else:
            assert np.array_equal(mine, s), b  # masked cells included
        for q, iv in enumerate(m.species_iv):
            assert np.array_equal(t.get_cc(iv + 1)[b - 1][1:-1, 1:-1, 1:-1], ys[q]), (b, iv)
    assert want[leaves[-1]][1] is None
    assert lim[0] == min(w[2] for w in want.values())
    t.close()


# ------------------------------------------------------------ around the step
def _uniform16(monkeypatch, fused, factor):
    monkeypatch.setenv("AFH_FE_FUSED", str(fused))
    g = golden.load("uni8")
    td, chem = tables_from(g)
    topo = uniform_tree(16, (32, 32, 32), (2e-3, 2e-3, 2e-3), 1)
    c = StreamerCase(capi.hip_library(), topo, td, chem, float(g["current_voltage"]),
                     coarse_cycles=12, device=0)
    seed_state(c)
    c.fluid.field_set_rhs(IV["rhs"], 0)
    c.field_compute(0, check_residual=False)
    if factor:
        c.fluid.set_source_factor(capi.SRCFAC_FLUX, [True, False], 5e4, 0)
    c.lib.call("profile_enable", c.tree.h, capi.PROF_FE)
    lim = c.fluid.forward_euler(1e-12, 0, [0], [1.0], 1, True)
    ms, nl, by = C.c_double(), C.c_int64(), C.c_double()
    c.lib.call("profile_read", c.tree.h, C.byref(ms), C.byref(nl), C.byref(by))
    out = [c.tree.get_cc(IV[s] + 1) for s in ("e", "pos", "neg")]
    c.tree.close()
    return list(lim), out, nl.value


def test_no_fused_step_with_the_factor(monkeypatch):
    """16^3 boxes with AFH_FE_FUSED=2 take k_fe_lds -- which has no factor --
    only while the factor is off."""
    lim_a, a, fe_a = _uniform16(monkeypatch, 2, True)
    lim_b, b, fe_b = _uniform16(monkeypatch, 0, True)
    lim_c, c, fe_c = _uniform16(monkeypatch, 2, False)
    assert fe_c > 0 and fe_a == 0 and fe_b == 0
    assert lim_a == lim_b
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])


@pytest.mark.parametrize("ndim", [3, 2])
def test_off_is_off(ndim):
    """set(FLUX) then set(NONE): the step of a fluid that never set it."""
    out = []
    for toggle in (False, True):
        sim = _sim("rtest_test_3d" if ndim == 3 else "rtest_test_2d", 8, ndim, None)
        assert sim.source_factor == capi.SRCFAC_NONE  # the driver never set it
        if toggle:
            sim.fluid.set_source_factor(capi.SRCFAC_FLUX, sim.ionization, 5e4, sim.i_sf)
            sim.fluid.set_source_factor(capi.SRCFAC_NONE, None, 5e4, sim.i_sf)
        _random_state(sim, 23)
        sim.tree.put_cc(sim.i_sf, np.full(sim.tree.cc_shape, -7.0))
        lim = sim.fluid.forward_euler(1e-12, 0, [0], [1.0], 1, True)
        out.append((list(lim), [sim.tree.get_cc(iv + 1) for iv in sim.densities],
                    sim.tree.get_cc(sim.i_sf)))
        # ... and on: a different step
        sim.fluid.set_source_factor(capi.SRCFAC_FLUX, sim.ionization, 5e4, sim.i_sf)
        sim.fluid.forward_euler(1e-12, 0, [0], [1.0], 1, True)
        assert not np.array_equal(sim.tree.get_cc(sim.i_electron + 1), out[-1][1][0])
        sim.tree.close()
    assert out[0][0] == out[1][0]
    for x, y in zip(out[0][1], out[1][1]):
        assert np.array_equal(x, y)
    assert np.all(out[1][2] == -7.0)  # off: nothing stored


def _run_sharded(lib, topo, shard=None):
    g = golden.load("uni8")
    td, chem = tables_from(g)
    c = StreamerCase(lib, topo, td, chem, float(g["current_voltage"]), coarse_cycles=12,
                     shard=shard)
    seed_state(c)
    c.fluid.field_set_rhs(IV["rhs"], 0)
    c.mg.fas_fmg(True, have_guess=False)
    c.field_compute(0)
    # (50 electrons per cell: on this tree's cells -- down to 15.6 um -- the
    # threshold clears most cells and leaves factors of 1 and in between)
    c.fluid.set_source_factor(capi.SRCFAC_FLUX, [True, False], 50.0, IV["e"] + 2)
    out = {"lim": np.asarray(c.heun_step(1e-12)), "res": np.zeros(0)}
    for iv in (IV["e"], IV["e"] + 1, IV["e"] + 2, IV["pos"], IV["neg"]):
        out["cc%d" % iv] = c.tree.get_cc(iv)
    if shard is not None:
        shard.detach()
    return out


def test_two_thread_ranks_equal_one():
    """The update reads only its own box: the sharded AMR tree of
    tests/test_dist_native.py (local transport, 2 ranks) with the factor on
    equals the single-rank run bitwise, the stored factor included."""
    from concurrent.futures import ThreadPoolExecutor
    from afh.dist import NativeGroup, NativeShard
    from test_dist import TOPOS
    from test_dist_native import _compare
    lib, world = capi.hip_library(), 2
    topo = TOPOS["amr8"]()
    ref = _run_sharded(lib, topo)
    group = NativeGroup(lib, world)
    shards = [NativeShard(lib, topo, world, r, group=group) for r in range(world)]
    try:
        with ThreadPoolExecutor(world) as ex:
            futs = [ex.submit(_run_sharded, lib, topo, shards[r]) for r in range(world)]
            parts = [f.result() for f in futs]
    finally:
        group.close()
    _compare(ref, shards, parts)
    s = ref["cc%d" % (IV["e"] + 2)]
    assert ((s > 0) & (s < 1)).any() and (s == 1).any()


# ------------------------------------------------------------ argument checks
@pytest.mark.parametrize("ndim", [3, 2])
def test_argument_checks(ndim):
    sim = _sim("rtest_test_3d" if ndim == 3 else "rtest_test_2d", 8, ndim, "flux")
    lib, f = sim.lib, sim.fluid
    flags = (C.c_uint8 * 2)(1, 0)

    def call(h, mode, fl, min_e, iv):
        with pytest.raises(capi.AfhError) as e:
            lib.call("fluid_set_source_factor", h, mode, fl, min_e, iv)
        return _code(e), str(e.value)

    code, msg = call(None, capi.SRCFAC_FLUX, flags, -1.0, 0)
    assert code == ERR_ARG and "null" in msg
    code, msg = call(f.h, 2, flags, -1.0, 0)
    assert code == ERR_ARG and "unknown mode 2" in msg
    code, msg = call(f.h, capi.SRCFAC_FLUX, None, -1.0, 0)
    assert code == ERR_ARG and "no ionization flags" in msg
    for iv in (-1, sim.n_var_tree + 1):
        code, msg = call(f.h, capi.SRCFAC_FLUX, flags, -1.0, iv)
        assert code == ERR_ARG and "bad i_srcfac" in msg
    for iv in [sim.i_efld] + list(sim.densities):
        code, msg = call(f.h, capi.SRCFAC_FLUX, flags, -1.0, iv)
        assert code == ERR_ARG and "a variable the step uses" in msg
    # a further state of a species: refused by the step that uses it
    lib.call("fluid_set_source_factor", f.h, capi.SRCFAC_FLUX, flags, -1.0, sim.i_electron + 1)
    _random_state(sim, 3)
    with pytest.raises(capi.AfhError) as e:
        f.forward_euler(1e-12, 0, [0], [1.0], 1, True)
    assert _code(e) == ERR_ARG and "a variable the step uses" in str(e.value)
    # ... while the step that does not touch that state runs
    lib.call("fluid_set_source_factor", f.h, capi.SRCFAC_FLUX, flags, -1.0, sim.i_electron + 2)
    f.forward_euler(1e-12, 0, [0], [1.0], 1, True)
    # the update mask's variable
    f.set_source_factor(capi.SRCFAC_NONE)
    f.set_update_mask(sim.i_tmp)
    code, msg = call(f.h, capi.SRCFAC_FLUX, flags, -1.0, sim.i_tmp)
    assert code == ERR_ARG and "a variable the step uses" in msg
    f.set_update_mask(0)
    with pytest.raises(ValueError, match="ionization flags"):
        f.set_source_factor(capi.SRCFAC_FLUX, [True], -1.0, 0)
    sim.tree.close()


def test_refused_during_a_graph_capture():
    """AFH_ERR_STATE while the tree's stream is capturing (3-D: the 2-D
    library keeps its stream to itself, so only its own V-cycle captures
    could meet the call). Nothing is launched; the empty graph is dropped."""
    hip = C.CDLL("libamdhip64.so")
    sim = _sim("rtest_test_3d", 8, 3, "flux")
    stream, graph = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    sim.lib.call("tree_set_stream", sim.tree.h, stream)
    relaxed = 2  # hipStreamCaptureModeRelaxed
    assert hip.hipStreamBeginCapture(stream, relaxed) == 0
    err = None
    try:
        sim.fluid.set_source_factor(capi.SRCFAC_FLUX, sim.ionization, -1.0, 0)
    except capi.AfhError as e:
        err = e
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
    if graph:
        hip.hipGraphDestroy(graph)
    assert err is not None and _code(err) == ERR_STATE
    assert "during a graph capture" in str(err)
    # outside the capture the same call goes through
    sim.fluid.set_source_factor(capi.SRCFAC_FLUX, sim.ionization, -1.0, 0)
    sim.lib.call("tree_set_stream", sim.tree.h, None)
    sim.tree.close()
    hip.hipStreamDestroy(stream)
