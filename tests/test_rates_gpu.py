"""The rate and J.E sums of the species step (include/afivo_hip_rates.h) on
the GPU, in libafivo_hip.so (k_update's RS instantiations) and
libafivo_hip_2d.so (k2_update's RATES option).

* The sums against tests/rates_numpy.py, which restates chemical_rates_box and
  sum_global_JdotE and sums its terms exactly (math.fsum). The numpy side
  takes the face fluxes the device's flux_upwind_tree left, so the update's
  sums alone are compared. The bound is derived, not measured: a sum of n
  terms in any order is within (n - 1) u sum|x_i| of the exact sum, u =
  2**-53, and each term carries a few roundings of its own (the weight,
  product(dr), 1 ulp of pow / exp), so

      |device - exact| <= (n_cells + 8) * 2**-53 * sum|term|

  with n_cells and the terms from the restatement. Every comparison prints the
  observed error next to the bound.
* A balance that does not use the restatement: for a species without a flux,
  sum_cc(out) - sum_cc(prev) = dt * sum_r nu_r rates_r.
* The paths around it: the state and the limits are those of a step without
  the sums bit for bit, the fused 3-D kernel still takes Heun's first
  sub-step, two runs give the same bits, the error codes, and the driver's
  time loop with global_rates.
"""
import ctypes as C
import math

import numpy as np
import pytest

import golden
import rates_numpy as rn
import state2d
import state_srcfac as ss
from afh import capi
from afh.driver import Simulation
from afh.streamer import FV, IV, StreamerCase, seed_state, standard_reactions, tables_from
from afh.tree import uniform_tree
from test_srcfac_gpu import (PFMG, _code, _gas_case, _lib, _random_state, _rod_case, _sim)

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED, ERR_STATE = -2, -4
STAGE1 = (0, [0], [1.0], 1)  # (s_deriv, s_prev, w_prev, s_out)
STAGE2 = (1, [0, 1], [0.5, 0.5], 0)


def _within(what, got_rates, got_je, want):
    """The device's sums within the derived bound of the exact sums of the
    restated terms; prints every figure before it asserts."""
    br, bj = want.bounds()
    err = np.abs(np.asarray(got_rates) - want.rates)
    ej = abs(got_je - want.jdote)
    print("%s: %d cells; rates err/bound %s; J.E %.17g err %.3g bound %.3g"
          % (what, want.n_cells, ["%.3g/%.3g" % (e, b) for e, b in zip(err, br)],
             got_je, ej, bj))
    assert np.all(np.isfinite(got_rates)) and math.isfinite(got_je)
    assert np.all(err <= br), (what, err, br)
    assert ej <= bj, (what, ej, bj)


def _step_with_sums(fluid, stage, dt):
    s_deriv, s_prev, w_prev, s_out = stage
    fluid.set_rate_sums(True)
    lim = fluid.flux_update_densities(dt, s_deriv, s_prev, w_prev, s_out, True)
    return lim, fluid.fetch_rate_sums()


# ------------------------------------------------- 3-D sums against numpy
@pytest.fixture(scope="module")
def states():
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = ss.build_state(model)
        return cache[model]
    return get


def _amr_sim(states, model, monkeypatch, factor):
    """tests/state_srcfac.py's AMR state (tree P at nc = 8: non-leaf boxes and
    refinement boundaries) on the device, the stored face field."""
    monkeypatch.setenv("AFH_FACES_FROM_PHI", "0")
    ndim = ss.MODELS[model][0]
    c, af, cc, fc, dt0, d = states(model)
    d = ss.case_with_factor(d, "min") if factor else dict(d)
    sim = Simulation(_lib(ndim), d, device=0, **(PFMG if ndim == 2 else {}))
    sim.af = af
    sim._bind(sim._create_tree())
    assert not sim.faces_from_phi and af.nc == 8
    for iv, a in cc.items():
        sim.tree.put_cc(iv, a)
    for ivf, a in fc.items():
        sim.tree.put_fc(ivf, a)
    return sim, af, dt0


def _sums_of(sim, af, stage, dt, factor, min_e=-1.0, lsf=None):
    """flux_upwind_tree, the update with the sums on, and the restatement on
    the same inputs: (rates, J.E, rates_numpy.Sums, restate) -- restate(**kw)
    the restatement again with further arguments of rates_numpy.tree_sums."""
    t = sim.tree
    s_deriv = stage[0]
    sim.fluid.flux_upwind_tree(s_deriv)
    F, Ef = t.get_fc(sim.f_flux), t.get_fc(sim.f_field)
    m = ss.model_of(sim)
    cc = {iv + s_deriv: t.get_cc(iv + s_deriv) for iv in m.species_iv}
    cc[m.i_efld] = t.get_cc(m.i_efld)
    _, (rates, je) = _step_with_sums(sim.fluid, stage, dt)

    def restate(**kw):
        return rn.tree_sums(m, af, cc, F, Ef, s_deriv, af.leaves(), factor=factor,
                            min_e=min_e, lsf=lsf, **kw)
    return rates, je, restate(), restate


@pytest.mark.parametrize("model", ["test_3d", "test_3d_chem"])
def test_amr_sums_3d_equal_numpy_and_see_the_source_factor(states, monkeypatch, model):
    out = {}
    for factor in (False, True):
        sim, af, dt0 = _amr_sim(states, model, monkeypatch, factor)
        assert len(af.leaves()) < sum(1 for b in range(1, af.highest_id + 1) if af.in_use[b])
        for k, stage in enumerate(ss.stages(model)):
            dt = ss.stage_dt(model, k, dt0)
            rates, je, want, _ = _sums_of(sim, af, stage, dt, factor,
                                          ss.VARIANTS["min"] if factor else -1.0)
            _within("%s factor=%d stage %d" % (model, factor, k + 1), rates, je, want)
            assert np.all(rates >= 0) and rates.max() > 0 and je != 0.0
            out[factor, k] = rates
            if k == 0:
                # two runs from the same state (the first stage does not
                # write its inputs): the same bits
                _, (r2, j2) = _step_with_sums(sim.fluid, stage, dt)
                assert np.array_equal(r2, rates) and j2 == je
        ion = np.array(sim.ionization, bool)
        sim.tree.close()
    # the scaled rates are the ones summed: every flagged reaction differs,
    # and is smaller (the factor is at most 1)
    for k in range(2):
        assert np.all(out[True, k][ion] < out[False, k][ion]), (out[True, k], out[False, k])


@pytest.mark.parametrize("what", ["ions", "photo"])
@pytest.mark.parametrize("factor", [False, True])
def test_sums_3d_with_ions_and_photoionization(what, factor):
    """tests/test_srcfac_gpu.py's two-level tree and random state: mobile ions
    with the temperature rate forms (SLOW), photoionization."""
    case = {"ions": "rtest_test_3d_chem", "photo": "rtest_test_3d_photoi_chem"}[what]
    sim = _sim(case, 8, 3, "min" if factor else None, n_ions=2 if what == "ions" else 0)
    assert sim.photoi == (what == "photo")  # (_sim: the stored face field)
    _random_state(sim, 29)
    for stage in (STAGE1, STAGE2):
        rates, je, want, _ = _sums_of(sim, sim.af, stage, 1e-12, factor, ss.VARIANTS["min"])
        _within("3d %s factor=%d" % (what, factor), rates, je, want)
    sim.tree.close()


@pytest.mark.parametrize("factor", [False, True])
def test_sums_3d_with_variable_gas_density(factor):
    t, f, topo, m = _gas_case()
    leaves = [int(b) for b in topo["lvl_leaves_2"]]
    dr = {b: topo["meta_dr"][b - 1] for b in leaves}
    if factor:
        f.set_source_factor(capi.SRCFAC_FLUX, m.ionization, -1.0, 9)
    f.flux_upwind_tree(0)
    F, Ef = t.get_fc(1), t.get_fc(2)
    cc = {iv: t.get_cc(iv) for iv in (1, 3, 5, 7, 8)}
    _, (rates, je) = _step_with_sums(f, STAGE1, 1e-12)
    want = rn.tree_sums(m, dr, cc, F, Ef, 0, leaves, factor=factor, Ng=cc[8])
    _within("3d gas factor=%d" % factor, rates, je, want)
    assert np.all(rates > 0)
    t.close()


def _uniform_case(nc, cells):
    g = golden.load("uni8")
    td, chem = tables_from(g)
    topo = uniform_tree(nc, (cells,) * 3, (2e-3, 2e-3, 2e-3), 1)
    c = StreamerCase(capi.hip_library(), topo, td, chem, float(g["current_voltage"]),
                     coarse_cycles=12, device=0)
    seed_state(c)
    c.fluid.field_set_rhs(IV["rhs"], 0)
    c.field_compute(0, check_residual=False)
    m = ss.Model(ndim=3, species_iv=[IV["e"], IV["pos"], IV["neg"]], i_electron=IV["e"],
                 i_efld=IV["efld"], reactions=standard_reactions(), ionization=[True, False],
                 chem=chem, td=td, N=c.n_gas)
    return c, topo, m


@pytest.mark.parametrize("nc,cells", [(2, 16), (4, 16), (6, 12), (16, 32)])
def test_box_sizes_3d_and_the_face_field_from_phi(nc, cells):
    """Boxes of 2^3, 4^3 and 6^3 cells leave lanes (and whole waves) of the
    256-lane workgroup idle; 16^3 boxes take 16 workgroups each. A solved
    field on a uniform tree: the sums with the stored face field, and bitwise
    the same sums with the face field formed from phi."""
    c, topo, m = _uniform_case(nc, cells)
    t, f = c.tree, c.fluid
    leaves = [int(b) for b in topo["lvl_leaves_1"]]
    assert len(leaves) == (cells // nc) ** 3
    dr = {b: topo["meta_dr"][b - 1] for b in leaves}
    f.flux_upwind_tree(0)
    F, Ef = t.get_fc(FV["flux"]), t.get_fc(FV["field"])
    cc = {iv: t.get_cc(iv) for iv in m.species_iv + [m.i_efld]}
    _, (rates, je) = _step_with_sums(f, STAGE1, 1e-12)
    want = rn.tree_sums(m, dr, cc, F, Ef, 0, leaves)
    _within("3d uniform nc=%d" % nc, rates, je, want)
    assert np.all(rates > 0) and je > 0
    f.set_field_source(IV["phi"], -1.0)
    f.flux_upwind_tree(0)
    assert np.array_equal(t.get_fc(FV["flux"]), F)
    _, (r2, j2) = _step_with_sums(f, STAGE1, 1e-12)
    assert np.array_equal(r2, rates) and j2 == je
    t.close()


# ------------------------------------------------------------- the 3-D mask
def test_mask_3d_whole_box_adds_nothing_partly_masked_box_all_cells():
    g, c, m = _rod_case()
    t = c.tree
    i_lsf = golden.IVS["lsf"]
    leaves = [int(b) for l in range(1, int(g["highest_lvl"]) + 1) for b in g["lvl_leaves_%d" % l]]
    lsf = t.get_cc(i_lsf)
    cut = [b for b in leaves if (lsf[b - 1][1:-1, 1:-1, 1:-1] <= 0).any()
           and (lsf[b - 1][1:-1, 1:-1, 1:-1] > 0).any()]
    assert cut
    lsf[leaves[-1] - 1] = -1.0  # one leaf wholly inside the electrode
    t.put_cc(i_lsf, lsf)
    c.fluid.set_update_mask(i_lsf)
    # a random state on the rod tree (the golden one has no electrons yet),
    # the stored face field
    rng = np.random.default_rng(43)
    for iv in m.species_iv:
        t.put_cc(iv, 1e15 * (0.2 + rng.random(t.cc_shape)) ** 4)
    t.put_cc(m.i_efld, 3e6 * (0.1 + 2 * rng.random(t.cc_shape)))
    t.put_fc(FV["field"], 3e6 * rng.standard_normal(t.fc_shape))
    c.fluid.set_field_source(0)
    c.fluid.flux_upwind_tree(0)
    F, Ef = t.get_fc(FV["flux"]), t.get_fc(FV["field"])
    cc = {iv: t.get_cc(iv) for iv in m.species_iv + [m.i_efld]}
    dr = {b: g["meta_dr"][b - 1] for b in leaves}
    _, (rates, je) = _step_with_sums(c.fluid, STAGE1, 1e-12)
    want = rn.tree_sums(m, dr, cc, F, Ef, 0, leaves, lsf=lsf)
    _within("3d mask", rates, je, want)
    assert np.all(rates > 0) and je != 0.0
    # the restriction matters: with the wholly masked box, or without the
    # masked cells of the cut boxes, the sums miss the bound
    every = rn.tree_sums(m, dr, cc, F, Ef, 0, leaves)
    assert every.n_cells == want.n_cells + (t.cc_shape[-1] - 2) ** 3
    gas_only = rn.tree_sums(m, dr, cc, F, Ef, 0, leaves, lsf=lsf, unmasked_only=True)
    for other in (every, gas_only):
        print("3d mask, other restriction:", np.abs(rates - other.rates), other.bounds()[0])
        assert np.any(np.abs(rates - other.rates) > other.bounds()[0])
    t.close()


# ------------------------------------------------------------------- 2-D
def _state2d(nc):
    """tests/state2d.py's test_2d state, at box size nc."""
    if nc == 8:
        return state2d.build_state("test_2d")
    real = golden.load

    def load(name):
        d = dict(real(name))
        d["box_size"] = np.array([nc])
        return d
    golden.load = load
    try:
        return state2d.build_state("test_2d")
    finally:
        golden.load = real


@pytest.fixture(scope="module")
def states2d():
    cache = {}

    def get(nc):
        if nc not in cache:
            cache[nc] = _state2d(nc)
        return cache[nc]
    return get


def _sim2d(states2d, nc, cyl, what="plain", global_rates=False):
    """A Simulation on the state2d tree with its state: Cartesian or
    cylindrical, with photoionization (a random rate) or two mobile ions."""
    c, af, cc, fc, dt = states2d(nc)
    d = dict(golden.load("rtest_test_2d_photoi" if what == "photo" else "rtest_test_2d"))
    d["box_size"] = np.array([nc])
    sim = Simulation(capi.hip_library_2d(), d, device=0, **PFMG)
    sim.af = af
    sim.cylindrical = cyl
    if what == "ions":
        plasma_iv = [sim.species_itree[n] for n in sim.plasma]
        ions, n_face = [], sim.n_var_face
        for sp in range(1, len(plasma_iv) + 1):
            if plasma_iv[sp - 1] != sim.i_electron and sim.species_charge[sim.plasma[sp - 1]] \
                    and len(ions) < 2:
                n_face += 1
                ions.append((sp, n_face, 2.4e23 * (1 + 0.25 * len(ions))))
        sim.ions, sim.n_var_face = ions, n_face
    sim._bind(sim._create_tree())
    assert sim.tree.coord == (capi.COORD_CYL if cyl else capi.COORD_XYZ)
    assert sim.photoi == (what == "photo") and len(sim.ions) == (2 if what == "ions" else 0)
    # (by name: the photoionization case registers further variables)
    for iv, a in cc.items():
        name = c.sa("cc_names")[iv - 1]
        if name in sim.cc_names:
            sim.tree.put_cc(sim.cc_names.index(name) + 1, a)
    fc_names = list(sim.c.sa("fc_names"))
    for ivf, a in fc.items():
        sim.tree.put_fc(fc_names.index(c.sa("fc_names")[ivf - 1]) + 1, a)
    if sim.photoi:
        rng = np.random.default_rng(41)
        sim.tree.put_cc(sim.i_photo, 1e24 * rng.random(sim.tree.cc_shape))
    return sim, af, dt


@pytest.mark.parametrize("what", ["plain", "photo", "ions"])
@pytest.mark.parametrize("nc", [8, 4])
@pytest.mark.parametrize("cyl", [False, True])
def test_sums_2d_equal_numpy(states2d, cyl, nc, what):
    sim, af, dt = _sim2d(states2d, nc, cyl, what)
    for stage in state2d.STAGES:
        rates, je, want, restate = _sums_of(sim, af, stage, dt, False)
        _within("2d cyl=%d nc=%d %s" % (cyl, nc, what), rates, je, want)
        assert np.all(rates > 0) and je != 0.0
        if cyl:
            # the weight is af_cyl_volume_cc: product(dr) on the same state
            # misses the bound
            flat = restate(cyl_weight=False)
            assert np.all(np.abs(rates - flat.rates) > flat.bounds()[0])
            assert abs(je - flat.jdote) > flat.bounds()[1]
    sim.tree.close()


def test_sums_2d_with_the_source_factor(states2d):
    sim, af, dt = _sim2d(states2d, 8, True)
    rates0, _, _, _ = _sums_of(sim, af, STAGE1, dt, False)
    sim.fluid.set_source_factor(capi.SRCFAC_FLUX, sim.ionization, ss.VARIANTS["min"], 0)
    rates, je, want, _ = _sums_of(sim, af, STAGE1, dt, True, ss.VARIANTS["min"])
    _within("2d cyl factor", rates, je, want)
    ion = np.array(sim.ionization, bool)
    assert np.all(rates[ion] < rates0[ion]) and np.array_equal(rates[~ion], rates0[~ion])
    sim.tree.close()


# ------------------------------------- balance, independent of the restatement
def _balance(sim, af, dt, cyl):
    """One forward_euler (s_prev = [0], w_prev = [1], last step, no
    photoionization): for every plasma species without a flux,
    sum_cc(out) - sum_cc(prev) = dt * sum_r nu_r rates_r within the bound
    applied to the two tree sums and the rate sums together."""
    assert not sim.photoi and not sim.ions
    t, nd = sim.tree, sim.ndim
    sim.fluid.set_rate_sums(True)
    sim.fluid.forward_euler(dt, 0, [0], [1.0], 1, True)
    rates, _ = sim.fluid.fetch_rate_sums()
    assert np.all(rates >= 0)
    leaves = af.leaves()
    inner = (slice(1, -1),) * nd
    n_cells = len(leaves) * af.nc ** nd
    plasma_iv = [sim.species_itree[n] for n in sim.plasma]
    checked = 0
    for slot, iv in enumerate(plasma_iv, start=1):
        if iv == sim.i_electron:
            continue
        nu = np.array([sum(m for ix, m in zip(r["ix_out"], r["mult_out"]) if ix == slot)
                       - sum(1 for ix in r["ix_in"] if ix == slot) for r in sim.reactions], float)
        lhs = t.sum_cc(iv + 1) - t.sum_cc(iv)
        rhs = dt * float(np.dot(nu, rates))
        mag = 0.0
        for s in (0, 1):
            a = t.get_cc(iv + s)
            mag += math.fsum(float(np.sum(np.abs(a[b - 1][inner]) * rn.cell_volumes(
                af.dr[b], af.nc, nd, af.r_min[b][0] if cyl else None))) for b in leaves)
        # (rates are sums of non-negative terms: their magnitude is the sum)
        mag += dt * float(np.dot(np.abs(nu), rates))
        bound = (n_cells + 8) * rn.U * mag
        print("balance iv %d: lhs %.17g rhs %.17g err %.3g bound %.3g"
              % (iv, lhs, rhs, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound and lhs != 0.0
        checked += 1
    assert checked >= 1


def test_balance_3d(states, monkeypatch):
    sim, af, dt0 = _amr_sim(states, "test_3d", monkeypatch, False)
    _balance(sim, af, dt0, False)
    sim.tree.close()


@pytest.mark.parametrize("cyl", [False, True])
def test_balance_2d(states2d, cyl):
    sim, af, dt = _sim2d(states2d, 8, cyl)
    _balance(sim, af, dt, cyl)
    sim.tree.close()


# ----------------------------------------------------- the state is untouched
def _one_step(sim, on, fold, stage, dt):
    s_deriv, s_prev, w_prev, s_out = stage
    f = sim.fluid
    f.set_rate_sums(on)
    if fold:
        f.forward_euler_fold(dt, s_deriv, s_prev, w_prev, s_out, True)
        lim = f.fetch_step(True)[0]
    else:
        lim = f.forward_euler(dt, s_deriv, s_prev, w_prev, s_out, True)
    out = [sim.tree.get_cc(iv + s_out) for iv in sim.densities]
    if sim.fused_rhs:
        out.append(sim.tree.get_cc(sim.i_rhs))
    return list(lim), out


@pytest.mark.parametrize("ndim", [3, 2])
@pytest.mark.parametrize("fold", [False, True])
def test_state_and_limits_are_those_without_the_sums(ndim, fold):
    res = []
    for on in (False, True, False):
        sim = _sim("rtest_test_3d" if ndim == 3 else "rtest_test_2d", 8, ndim, None)
        _random_state(sim, 31)
        res.append(_one_step(sim, on, fold, STAGE2, 1e-12))
        if on:
            rates, je = sim.fluid.fetch_rate_sums()
            assert rates.max() > 0
        sim.tree.close()
    for lim, out in res[1:]:
        assert lim == res[0][0] and len(lim) == 4
        for x, y in zip(out, res[0][1]):
            assert np.array_equal(x, y)
    # (3-D: the rhs output of the fused field_set_rhs is among them)
    assert len(res[0][1]) == len(sim.densities) + (1 if ndim == 3 else 0)


def _uniform16(monkeypatch, on, last):
    """16^3 boxes with AFH_FE_FUSED=2: one forward_euler; the launches of
    AFH_PROF_FE and AFH_PROF_UPDATE it made."""
    monkeypatch.setenv("AFH_FE_FUSED", "2")
    c, topo, m = _uniform_case(16, 32)
    c.fluid.set_rate_sums(on)
    n = {}
    out = None
    for cls in (capi.PROF_FE, capi.PROF_UPDATE):
        c.lib.call("profile_enable", c.tree.h, cls)
        lim = c.fluid.forward_euler(1e-12, 0, [0], [1.0], 1, last)
        ms, nl, by = C.c_double(), C.c_int64(), C.c_double()
        c.lib.call("profile_read", c.tree.h, C.byref(ms), C.byref(nl), C.byref(by))
        n[cls] = nl.value
        cur = (list(lim), [c.tree.get_cc(IV[s] + 1) for s in ("e", "pos", "neg")])
        if out is not None:  # (the same step twice)
            assert cur[0] == out[0] and all(np.array_equal(x, y) for x, y in zip(cur[1], out[1]))
        out = cur
    sums = c.fluid.fetch_rate_sums() if on and last else None
    c.tree.close()
    return out, n, sums


def test_fused_first_sub_step_stays_fused_with_the_sums_on(monkeypatch):
    off_last, n_off_last, _ = _uniform16(monkeypatch, False, True)
    on_last, n_on_last, sums = _uniform16(monkeypatch, True, True)
    on_first, n_on_first, _ = _uniform16(monkeypatch, True, False)
    off_first, n_off_first, _ = _uniform16(monkeypatch, False, False)
    # last_step = 0 with the sums on: the fused kernel, no update launch
    assert n_on_first[capi.PROF_FE] > 0 and n_on_first[capi.PROF_UPDATE] == 0
    assert n_on_first == n_off_first
    # last_step = 1: fused without the sums, flux + update with them
    assert n_off_last[capi.PROF_FE] > 0 and n_off_last[capi.PROF_UPDATE] == 0
    assert n_on_last[capi.PROF_FE] == 0 and n_on_last[capi.PROF_UPDATE] > 0
    for a, b in ((on_last, off_last), (on_first, off_first)):
        assert a[0] == b[0]
        for x, y in zip(a[1], b[1]):
            assert np.array_equal(x, y)
    assert sums[0].min() > 0 and sums[1] > 0


# ------------------------------------------------------------- error codes
@pytest.mark.parametrize("ndim", [3, 2])
def test_fetch_needs_the_sums_on_and_a_last_step(ndim):
    sim = _sim("rtest_test_3d" if ndim == 3 else "rtest_test_2d", 8, ndim, None)
    f = sim.fluid
    _random_state(sim, 37)

    def refused(msg):
        with pytest.raises(capi.AfhError) as e:
            f.fetch_rate_sums()
        assert _code(e) == ERR_STATE and msg in str(e.value)

    refused("the sums are off")
    f.set_rate_sums(True)
    refused("no last step")
    f.forward_euler(1e-12, 0, [0], [1.0], 1, False)  # not a last step: nothing summed
    refused("no last step")
    f.forward_euler(1e-12, 1, [0, 1], [0.5, 0.5], 0, True)
    rates, je = f.fetch_rate_sums()
    # a step that is no last step leaves them untouched
    f.forward_euler(1e-12, 0, [0], [1.0], 1, False)
    r2, j2 = f.fetch_rate_sums()
    assert np.array_equal(r2, rates) and j2 == je
    f.set_rate_sums(False)
    refused("the sums are off")
    f.set_rate_sums(True)
    refused("no last step")  # switched on again: the old sums are gone
    with pytest.raises(capi.AfhError) as e:
        sim.lib.call("fluid_set_rate_sums", None, 1)
    assert "null" in str(e.value)
    sim.tree.close()


def test_refused_during_a_graph_capture():
    hip = C.CDLL("libamdhip64.so")
    sim = _sim("rtest_test_3d", 8, 3, None)
    stream, graph = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    sim.lib.call("tree_set_stream", sim.tree.h, stream)
    assert hip.hipStreamBeginCapture(stream, 2) == 0  # hipStreamCaptureModeRelaxed
    err = None
    try:
        sim.fluid.set_rate_sums(True)
    except capi.AfhError as e:
        err = e
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
    if graph:
        hip.hipGraphDestroy(graph)
    assert err is not None and _code(err) == ERR_STATE and "graph capture" in str(err)
    sim.fluid.set_rate_sums(True)
    sim.lib.call("tree_set_stream", sim.tree.h, None)
    sim.tree.close()
    hip.hipStreamDestroy(stream)


def test_sharded_tree_is_unsupported():
    """Thread ranks, as tests/test_dist_driver.py builds them."""
    from concurrent.futures import ThreadPoolExecutor
    from afh.dist import NativeGroup, NativeShard
    from test_dist import TOPOS
    lib, world = capi.hip_library(), 2
    topo = TOPOS["amr8"]()
    g = golden.load("uni8")
    td, chem = tables_from(g)
    group = NativeGroup(lib, world)
    shards = [NativeShard(lib, topo, world, r, group=group) for r in range(world)]

    def rank(r):
        c = StreamerCase(lib, topo, td, chem, float(g["current_voltage"]), coarse_cycles=12,
                         shard=shards[r])
        try:
            with pytest.raises(capi.AfhError) as e:
                c.fluid.set_rate_sums(True)
            return _code(e), str(e.value)
        finally:
            shards[r].detach()
    try:
        with ThreadPoolExecutor(world) as ex:
            got = list(ex.map(rank, range(world)))
    finally:
        group.close()
    for code, msg in got:
        assert code == ERR_UNSUPPORTED and "sharded" in msg


# ------------------------------------------------------------ the time loop
def _run_rows(name, rows, global_rates, per_steps=2):
    """The driver to `rows` log rows after the initial one, the currents
    formed every per_steps iterations; the diagnostics after every step."""
    d = dict(golden.load(name))
    d["current_update_per_steps"] = np.array([per_steps])
    ndim = len(d["coarse_grid_size_value"])
    sim = Simulation(_lib(ndim), d, device=0, global_rates=global_rates,
                     **(PFMG if ndim == 2 else {}))
    sim.start()
    diag = []
    while len(sim.log) < rows + 1 and sim.step():
        if global_rates:
            diag.append((sim.dt, sim.diagnostics()))
    return sim, diag


@pytest.mark.parametrize("name,rows", [("rtest_test_2d", 2), ("rtest_test_cyl_chem", 2),
                                       ("rtest_test_3d_chem", 1)])
def test_time_loop_with_global_rates(name, rows, tmp_path):
    plain, _ = _run_rows(name, rows, False)
    sim, diag = _run_rows(name, rows, True)
    # the log rows are bitwise those of a run without the sums
    assert len(sim.log) == rows + 1 and np.array_equal(np.array(sim.log), np.array(plain.log))
    plain.tree.close()
    assert len(diag) >= 2
    prev_r, prev_j = np.zeros(len(sim.reactions)), 0.0
    for it, (_, dg) in enumerate(diag, start=1):
        assert np.all(dg["global_rates"] >= prev_r) and np.all(dg["global_rates"] >= 0)
        if it % 2 == 0 and sim.voltage != 0:
            # Sato: the J.E current has the sign of the increment of
            # global_JdotE over the voltage
            inc = dg["global_JdotE"] - prev_j
            assert inc != 0 and dg["JdotE_current"] != 0
            assert (dg["JdotE_current"] > 0) == (inc / sim.voltage > 0)
            assert math.isfinite(dg["displ_current"]) and dg["field_energy"] > 0
        prev_r, prev_j = dg["global_rates"], dg["global_JdotE"]
    last = diag[-1][1]
    assert last["global_JdotE"] > 0 and last["global_rates"].max() > 0
    print(name, "steps", len(diag), "global_rates", last["global_rates"], "global_JdotE",
          last["global_JdotE"], "I_JdotE", last["JdotE_current"], "I_displ",
          last["displ_current"])
    # write_dat / restart carries both bitwise, and a continued run adds to
    # them. afh.datfile writes 3-D trees only (NDIM = 3, its docstring): a 2-D
    # run is held to the record's bytes, and continues in place.
    if sim.ndim == 3:
        sim.write_dat(str(tmp_path / "run"))
        other = Simulation(_lib(3), dict(golden.load(name)), device=0, global_rates=True)
        other.restart(str(tmp_path / "run.dat"))
    else:
        from afh.datfile import parse_sim_data, sim_data_bytes
        raw = sim_data_bytes(sim.it, sim.output_cnt, sim.time, sim.global_time,
                             sim.photoi_prev_time, sim.global_dt, sim.global_rates,
                             sim.global_JdotE, sim.frac_rejected)
        rec = parse_sim_data(raw, len(sim.reactions))
        other = sim
        other.global_rates = np.array(rec["global_rates"], float)
        other.global_JdotE = float(rec["global_JdotE"])
    assert np.array_equal(other.global_rates, last["global_rates"])
    assert other.global_JdotE == last["global_JdotE"]
    assert other.step()
    assert np.all(other.global_rates >= last["global_rates"])
    assert other.global_rates.max() > last["global_rates"].max()
    assert other.global_JdotE > last["global_JdotE"]
    if other is not sim:
        other.tree.close()
    sim.tree.close()


def test_driver_refuses_a_sharded_run_with_global_rates():
    sim = Simulation(capi.hip_library(), golden.load("rtest_test_3d"), device=0,
                     global_rates=True)
    with pytest.raises(NotImplementedError, match="sharded"):
        sim.shard_over(object())
