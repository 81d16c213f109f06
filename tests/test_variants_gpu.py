"""Every limiter and every boundary-condition type, on the device.

3-D: HIP == C oracle with np.array_equal on every cell or face of every box
in use, plus equal time-step limits (the pattern of test_box_sizes.py); the
oracle is held to the reference's compiled numerics for these options by
test_variants_cpu.py. 2-D (no C oracle): HIP == the numpy statement of
tests/variants_numpy.py, which test_variants_cpu.py holds to the reference's
2-D build. At box size 4 both libraries are also compared with the reference
fixtures themselves (tests/golden/variants3d.npz, variants2d.npz).

Inputs are lattice-valued (k 2^50): test_variants_cpu.py asserts, for every
input used here, that every branch of the limiters is reached, equalities
included. The shapes are the smallest that reach the named kernel:

  k_flux_staged<true, 0>   box size 4, AMR (+ k_consistent, k_flux_ion<0>)
  k_flux_staged<false, 0>  box size 6, AMR
  k_flux_lds<16, 0>        box size 16, AMR
  k_flux_lds<32|64, 0>     one level of two boxes
  k2_flux, k2_flux_ions    box sizes 4, 6, 16, AMR
  k_gc_faces, k_gc_corners box sizes 2, 4, 6, 16; k2_gc_box (corners) and
                           k2_gc (no corners, or AFH2_GC_BOX=0) 2, 4, 6, 32
  k_prolong_new, k2_prolong_new   box sizes 4, 6
"""
import ctypes as C

import numpy as np
import pytest

import golden
import variants_numpy as vn
from afh import capi
from afh.amr import AF_CYL, AfTree, DO_REF, KEEP_REF
from afh.streamer import IV, tables_from
from test_variants_cpu import (FLUX_INPUTS_2D, FLUX_INPUTS_3D, IONS, RB, FluxCase, assignment,
                               check_phi_refusal, check_prolong_against_numpy, fixture,
                               fixture_inputs, flux_input, flux_refusal, gc_filled, lattice_inputs,
                               leaf_faces, regrid_prolong, rotation, run_flux, two_box_tree,
                               variants_tree)

pytestmark = pytest.mark.gpu

N0_2D = [(capi.BC_NEUMANN, 0.0)] * 4


def hip3():
    return capi.hip_library(), 0


def hip2():
    return capi.hip_library_2d(), 0


def oracle():
    return capi.oracle_library(), -1


def launches(case, kclass, call):
    """call() with the kernel class profiled: (its result, the launches of
    that class)."""
    case.lib.call("profile_enable", case.tree.h, kclass)
    out = call()
    ms, nl, by = C.c_double(), C.c_int64(), C.c_double()
    case.lib.call("profile_read", case.tree.h, C.byref(ms), C.byref(nl), C.byref(by))
    case.lib.call("profile_enable", case.tree.h, 0)
    return out, nl.value


def same_flux(a, b, topo, what):
    """([F per species], [densities], limits) of two flux calls: the leaves'
    faces, the densities of every box in use, the limits."""
    (Fa, ca, la), (Fb, cb, lb) = a, b
    use = vn.in_use(topo)
    assert len(Fa) == len(Fb)
    for n, (x, y) in enumerate(zip(Fa, Fb)):
        for d, (p, q) in enumerate(zip(leaf_faces(x, topo), leaf_faces(y, topo))):
            assert np.array_equal(p, q), (what, n, d, np.max(np.abs(p - q)))
            assert np.count_nonzero(q) > q.size // 4
    for n, (x, y) in enumerate(zip(ca, cb)):
        assert np.array_equal(x[use], y[use]), (what, n)
    assert tuple(la) == tuple(lb), (what, la, lb)


def numpy_flux_2d(topo, x, lim=vn.LIM_KOREN, prolong=vn.LIM_MC, bc=N0_2D, ions=(), cyl=False):
    """vn.flux_2d in the shape of FluxCase.flux."""
    g = fixture(2)
    sp = ["e"] + [("e", "pos", "neg")[q[0] - 1] for q in ions]
    sign = [-1.0] + [(-1.0, 1.0, -1.0)[q[0] - 1] for q in ions]
    F, cc, lims = vn.flux_2d(topo, [x[s] for s in sp], x["efld"], x["fc_field"],
                             tables_from(g)[0], 1 / float(g["gas_number_density"]), lim,
                             prolong, bc, [q[2] for q in ions], sign, cyl)
    return F, cc, lims


# ------------------------------------------------------- flux limiters, 3-D
@pytest.mark.parametrize("phi", [False, True])
@pytest.mark.parametrize("lim", vn.LIMITERS)
@pytest.mark.parametrize("kind,nc,seed", FLUX_INPUTS_3D)
def test_flux_limiter_equals_oracle(kind, nc, seed, lim, phi):
    """afh_flux_upwind_tree with each limiter (Koren the control), the face
    field stored or taken from the potential (the PHI templates). The tables
    fit the LDS kernels' limit, so 16, 32 and 64 take k_flux_lds: on the AMR
    tree one launch per leaf level, where k_flux_staged launches once."""
    topo, x = flux_input(kind, nc, seed)
    tabs = fixture(3)
    assert tabs["td_rows_cols"].shape[0] <= 2048
    c = FluxCase(*hip3(), topo, tabs, limiter=lim, phi=phi)
    c.put(x)
    a, n_launch = launches(c, capi.PROF_FLUX, c.flux)
    c.close()
    b = run_flux(*oracle(), topo, tabs, x, limiter=lim, phi=phi)
    same_flux(a, b, topo, (kind, nc, lim, phi))
    if kind == "amr":
        assert n_launch == (2 if nc == 16 else 1)
    if lim != capi.LIM_KOREN:
        k = run_flux(*oracle(), topo, tabs, x, phi=phi)
        assert not np.array_equal(k[0][0], b[0][0])


@pytest.mark.parametrize("phi", [False, True])
@pytest.mark.parametrize("lim", vn.LIMITERS)
def test_ion_flux_limiter_equals_oracle(lim, phi):
    """k_flux_ion<0, PHI> (and k_flux_staged, which a fluid with mobile ions
    takes): a positive and a negative ion, box size 4."""
    topo, x = flux_input("amr", 4, 1)
    tabs = fixture(3)
    a = run_flux(*hip3(), topo, tabs, x, limiter=lim, phi=phi, ions=IONS)
    b = run_flux(*oracle(), topo, tabs, x, limiter=lim, phi=phi, ions=IONS)
    assert len(a[0]) == 3
    same_flux(a, b, topo, ("ions", lim, phi))


def _euler(lib, dev, topo, x, fused, **kw):
    """One forward Euler step 0 -> 1, as one call (fused) or as the flux and
    the update: (limits, new densities, electron flux, k_fe_lds launches)."""
    c = FluxCase(lib, dev, topo, fixture(3), **kw)
    c.put(x)
    n_fe = 0
    if fused:
        step = lambda: c.fluid.forward_euler(1e-12, 0, [0], [1.0], 1, True, store_flux=True)
        lim, n_fe = launches(c, capi.PROF_FE, step) if dev >= 0 else (step(), 0)
    else:
        lim = c.fluid.flux_upwind_tree(0) + c.fluid.flux_update_densities(
            1e-12, 0, [0], [1.0], 1, True)
    out = [c.tree.get_cc(IV[s] + 1) for s in ("e", "pos", "neg")]
    F = c.tree.get_fc(1)
    c.close()
    return tuple(lim)[:3], out, F, n_fe


def _same_step(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    for n, (p, q) in enumerate(zip(a[1], b[1])):
        assert np.array_equal(p, q), (what, n, np.max(np.abs(p - q)))
        assert np.count_nonzero(q) > q.size // 2
    for p, q in zip(golden.faces(a[2]), golden.faces(b[2])):
        assert np.array_equal(p, q), what


def test_fused_step_falls_back_for_other_limiters(monkeypatch):
    """AFH_FE_FUSED=2 on 16^3 boxes: k_fe_lds is Koren only; with another
    limiter afh_fluid_forward_euler is the two kernels, and equals the two
    calls and the oracle. With Koren it is k_fe_lds (the control)."""
    monkeypatch.setenv("AFH_FE_FUSED", "2")
    topo, x = two_box_tree(16), lattice_inputs(two_box_tree(16), 21)
    for lim in (capi.LIM_MC, capi.LIM_VANLEER, capi.LIM_KOREN):
        one = _euler(*hip3(), topo, x, True, limiter=lim)
        two = _euler(*hip3(), topo, x, False, limiter=lim)
        ref = _euler(*oracle(), topo, x, True, limiter=lim)
        assert (one[3] > 0) == (lim == capi.LIM_KOREN)
        _same_step(one, two, ("two calls", lim))
        _same_step(one, ref, ("oracle", lim))


# ------------------------------------------------------- flux limiters, 2-D
@pytest.mark.parametrize("lim", vn.LIMITERS)
@pytest.mark.parametrize("kind,nc,seed", FLUX_INPUTS_2D)
def test_2d_flux_limiter_equals_numpy(kind, nc, seed, lim):
    """k2_flux with each limiter against the numpy statement."""
    topo, x = flux_input(kind, nc, seed, 2)
    a = run_flux(*hip2(), topo, fixture(2), x, limiter=lim)
    F, cc, lims = numpy_flux_2d(topo, x, lim)
    same_flux(a, (F, cc, lims), topo, ("2-D", nc, lim))


@pytest.mark.parametrize("lim", vn.LIMITERS)
@pytest.mark.parametrize("kind,nc,seed", FLUX_INPUTS_2D)
def test_2d_ion_flux_limiter_equals_numpy(kind, nc, seed, lim):
    """k2_flux_ions with each limiter: a positive and a negative ion."""
    topo, x = flux_input(kind, nc, seed, 2)
    a = run_flux(*hip2(), topo, fixture(2), x, limiter=lim, ions=IONS)
    same_flux(a, numpy_flux_2d(topo, x, lim, ions=IONS), topo, ("2-D ions", nc, lim))


@pytest.mark.parametrize("ions", [(), IONS])
def test_2d_cylindrical_flux_with_mc_equals_numpy(ions):
    """A limiter other than Koren on a cylindrical tree (the radial weights
    of the restriction and of the coarse z faces)."""
    nc = 4
    af = AfTree(nc, [2.0 ** -10] * 2, [4 * nc] * 2, coord=AF_CYL)

    def fn(ids):
        f = [DO_REF if af.lvl[b] == 1 or (af.lvl[b] == 2 and tuple(af.ix[b][:2]) in
                                          ((1, 1), (8, 8))) else KEEP_REF for b in ids]
        return np.array(f), np.zeros(len(ids), np.uint32)

    af.adjust_refinement(fn)
    af.adjust_refinement(fn)
    topo = af.topology()
    x = lattice_inputs(topo, 1)
    a = run_flux(*hip2(), topo, fixture(2), x, limiter=capi.LIM_MC, ions=ions, cyl=True)
    b = numpy_flux_2d(topo, x, capi.LIM_MC, ions=ions, cyl=True)
    same_flux(a, b, topo, "cyl")
    flat = numpy_flux_2d(topo, x, capi.LIM_MC, ions=ions, cyl=False)
    assert not np.array_equal(flat[0][0], b[0][0])


# ------------------------------------------------------ prolongation limiters
@pytest.mark.parametrize("lim", vn.LIMITERS)
@pytest.mark.parametrize("nc,seed", [(4, 1), (6, 2)])
def test_prolong_limiter_in_the_flux_equals_oracle(nc, seed, lim):
    """The species' prolongation limiter in the second ghost layer
    (gc2_prolong_rb), Koren flux."""
    topo, x = flux_input("amr", nc, seed)
    tabs = fixture(3)
    a = run_flux(*hip3(), topo, tabs, x, prolong=lim)
    b = run_flux(*oracle(), topo, tabs, x, prolong=lim)
    same_flux(a, b, topo, ("prolong", nc, lim))
    if lim != capi.LIM_GMINMOD43:
        assert not np.array_equal(b[0][0], run_flux(*oracle(), topo, tabs, x)[0][0])


@pytest.mark.parametrize("lim", vn.LIMITERS)
@pytest.mark.parametrize("nc,seed", [(4, 1), (6, 2)])
def test_2d_prolong_limiter_in_the_flux_equals_numpy(nc, seed, lim):
    topo, x = flux_input("amr", nc, seed, 2)
    a = run_flux(*hip2(), topo, fixture(2), x, prolong=lim)
    same_flux(a, numpy_flux_2d(topo, x, prolong=lim), topo, ("2-D prolong", nc, lim))


@pytest.mark.parametrize("lim", vn.LIMITERS)
@pytest.mark.parametrize("nc", [4, 6])
def test_regrid_prolong_limit_equals_oracle_and_numpy(nc, lim):
    """afh_tree_regrid with AFH_PROLONG_LIMIT (k_prolong_new): a uniform
    level refined; the oracle, and af_prolong_limit stated in numpy."""
    before, after, t1 = regrid_prolong(*hip3(), nc, 3, lim)
    b0, a0, _ = regrid_prolong(*oracle(), nc, 3, lim)
    assert np.array_equal(before, b0) and np.array_equal(after, a0)
    check_prolong_against_numpy(before, after, t1, 3, lim)


@pytest.mark.parametrize("lim", vn.LIMITERS)
@pytest.mark.parametrize("nc", [4, 6])
def test_2d_regrid_prolong_limit_equals_numpy(nc, lim):
    """k2_prolong_new."""
    before, after, t1 = regrid_prolong(*hip2(), nc, 2, lim)
    check_prolong_against_numpy(before, after, t1, 2, lim)


# ------------------------------------------------ boundary types, one layer
def _gc_input(topo, seed):
    rng = np.random.default_rng(seed)
    nd = int(topo.get("ndim", 3))
    return vn.lattice(rng, (int(topo["n_boxes"]),) + (int(topo["nc"]) + 2,) * nd)


@pytest.mark.parametrize("corners", [True, False])
@pytest.mark.parametrize("rb", sorted(RB))
@pytest.mark.parametrize("nc", [2, 4, 6, 16])
def test_gc_tree_boundary_types_equal_oracle(nc, rb, corners):
    """afh_gc_tree under the four rotations of the four types (every face
    sees Dirichlet, Neumann, continuous and dirichlet_copy, with non-zero
    values): k_gc_faces, k_gc_corners."""
    topo = variants_tree(nc, 3)
    v = _gc_input(topo, nc)
    use = vn.in_use(topo)
    seen = []
    for rot in range(4):
        a = gc_filled(*hip3(), topo, rotation(rot, 3), RB[rb], corners, v)
        b = gc_filled(*oracle(), topo, rotation(rot, 3), RB[rb], corners, v)
        assert np.array_equal(a[use], b[use]), (rot, np.argwhere(a[use] != b[use])[:3])
        assert np.array_equal(golden.interior(a), golden.interior(v))
        if not corners:
            assert np.array_equal(a[:, ::nc + 1, ::nc + 1, ::nc + 1],
                                  v[:, ::nc + 1, ::nc + 1, ::nc + 1])
        assert all(not np.array_equal(a, s) for s in seen)
        seen.append(a)


def _physical_ghosts_2d(a, topo, bc):
    """The physical-boundary ghost cells of a are bc_to_gc of its interiors."""
    nc, n = int(topo["nc"]), 0
    for b in vn.in_use(topo):
        for nb in range(4):
            if topo["meta_neighbors"][b, nb] >= 0:
                continue
            want = vn.bc_ghost_2d(a[b], nb, bc[nb], topo["meta_dr"][b], nc)
            got = (a[b][1:-1, 0 if nb == 0 else nc + 1] if nb < 2 else
                   a[b][0 if nb == 2 else nc + 1, 1:-1])
            assert np.array_equal(got, want), (b, nb)
            n += 1
    return n


@pytest.mark.parametrize("rb", sorted(RB))
@pytest.mark.parametrize("nc", [2, 4, 6, 32])
def test_2d_gc_tree_boundary_types(nc, rb, monkeypatch):
    """The 2-D afh_gc_tree under the four rotations. With corners it is one
    launch of k2_gc_box, without (or with AFH2_GC_BOX=0, read when the tree
    is created) k2_gc, then k2_corners: the three agree on every cell they
    all fill, and the physical faces hold bc_to_gc of the interiors."""
    topo = variants_tree(nc, 2)
    v = _gc_input(topo, nc)
    use = vn.in_use(topo)
    for rot in range(4):
        bc = rotation(rot, 2)
        box = gc_filled(*hip2(), topo, bc, RB[rb], True, v)
        sides = gc_filled(*hip2(), topo, bc, RB[rb], False, v)
        monkeypatch.setenv("AFH2_GC_BOX", "0")
        split = gc_filled(*hip2(), topo, bc, RB[rb], True, v)
        monkeypatch.delenv("AFH2_GC_BOX")
        assert np.array_equal(box[use], split[use]), rot
        corner = np.zeros(v.shape[1:], bool)
        corner[::nc + 1, ::nc + 1] = True
        assert np.array_equal(box[use][:, ~corner], sides[use][:, ~corner])
        assert np.array_equal(sides[use][:, corner], v[use][:, corner])
        assert not np.array_equal(box[use][:, corner], v[use][:, corner])
        assert _physical_ghosts_2d(box, topo, bc) > 30


@pytest.mark.parametrize("meth", [1, 2])
@pytest.mark.parametrize("rot", range(4))
@pytest.mark.parametrize("ndim", [3, 2])
def test_gc_tree_matches_reference(ndim, rot, meth):
    """Box size 4: the reference's own ghost cells, every box, every cell."""
    g = fixture(ndim)
    a = gc_filled(*(hip3() if ndim == 3 else hip2()), g, rotation(rot, ndim), meth, True,
                  g["in_e"])
    assert np.array_equal(a, g["gc_%d_%d" % (rot, meth)])


@pytest.mark.parametrize("corners", [True, False])
def test_set_bc_between_two_fills_equals_oracle(corners):
    """afh_set_bc changes every face's type and value after a first fill."""
    topo = variants_tree(4, 3)
    v = _gc_input(topo, 9)
    use = vn.in_use(topo)
    for rb in sorted(RB):
        a = gc_filled(*hip3(), topo, rotation(0, 3), RB[rb], corners, v, bc2=rotation(2, 3))
        b = gc_filled(*oracle(), topo, rotation(0, 3), RB[rb], corners, v, bc2=rotation(2, 3))
        assert np.array_equal(a[use], b[use]), rb
        if rb != "mg_sides":
            first = gc_filled(*oracle(), topo, rotation(0, 3), RB[rb], corners, v)
            assert not np.array_equal(a[use], first[use])


def test_2d_set_bc_between_two_fills_matches_reference():
    g = fixture(2)
    a = gc_filled(*hip2(), g, rotation(0, 2), 2, True, g["in_e"], bc2=rotation(3, 2))
    # the second fill of the same interiors under rotation 3
    assert np.array_equal(a, g["gc_3_2"])


# ----------------------------------------------- boundary types, two layers
@pytest.mark.parametrize("asg", range(3))
@pytest.mark.parametrize("kind,nc,seed", FLUX_INPUTS_3D[:3])
def test_two_layer_boundary_equals_oracle(kind, nc, seed, asg):
    """k_gc2 with Dirichlet, Neumann and dirichlet_copy faces of non-zero
    value, seen through the flux; the Neumann assignment has the c0 of
    m_af_ghostcell.f90:361 on the second layer of the high-y face."""
    topo, x = flux_input(kind, nc, seed)
    tabs, bc = fixture(3), assignment(asg, 3)
    a = run_flux(*hip3(), topo, tabs, x, bc=bc)
    b = run_flux(*oracle(), topo, tabs, x, bc=bc)
    same_flux(a, b, topo, ("bc", nc, asg))
    assert not np.array_equal(b[0][0], run_flux(*oracle(), topo, tabs, x)[0][0])


@pytest.mark.parametrize("asg", range(3))
@pytest.mark.parametrize("kind,nc,seed", FLUX_INPUTS_2D[:2])
def test_2d_two_layer_boundary_equals_numpy(kind, nc, seed, asg):
    """k2_gc2."""
    topo, x = flux_input(kind, nc, seed, 2)
    bc = assignment(asg, 2)
    a = run_flux(*hip2(), topo, fixture(2), x, bc=bc)
    same_flux(a, numpy_flux_2d(topo, x, bc=bc), topo, ("2-D bc", nc, asg))


@pytest.mark.parametrize("asg", range(3))
def test_fused_step_sees_the_boundary_values(asg, monkeypatch):
    """AFH_FE_FUSED=2, Koren, 16^3: the fused step's prelude fills the second
    layer under the same boundary (the non-zero high-y Neumann value among
    them); it equals the two calls and the oracle."""
    monkeypatch.setenv("AFH_FE_FUSED", "2")
    topo, x = two_box_tree(16), lattice_inputs(two_box_tree(16), 22)
    bc = assignment(asg, 3)
    one = _euler(*hip3(), topo, x, True, bc=bc)
    two = _euler(*hip3(), topo, x, False, bc=bc)
    ref = _euler(*oracle(), topo, x, True, bc=bc)
    assert one[3] > 0
    _same_step(one, two, ("two calls", asg))
    _same_step(one, ref, ("oracle", asg))
    plain = _euler(*oracle(), topo, x, True)
    assert not np.array_equal(plain[1][0], ref[1][0])


# ------------------------------------------------------- reference fixtures
def _fixture_flux(ndim, key, **kw):
    g = fixture(ndim)
    F, _, lim = run_flux(*(hip3() if ndim == 3 else hip2()), g, g, fixture_inputs(g), **kw)
    for a, b in zip(leaf_faces(F[0], g), leaf_faces(g[key], g)):
        assert np.array_equal(a, b), key
    assert list(lim) == list(g[key + "_dt"]), key


@pytest.mark.parametrize("lim", vn.LIMITERS)
@pytest.mark.parametrize("ndim", [3, 2])
def test_flux_limiter_matches_reference(ndim, lim):
    _fixture_flux(ndim, "flux_%d" % lim, limiter=lim)


@pytest.mark.parametrize("lim", vn.LIMITERS)
@pytest.mark.parametrize("ndim", [3, 2])
def test_prolong_limiter_matches_reference(ndim, lim):
    _fixture_flux(ndim, "pflux_%d" % lim, prolong=lim)


@pytest.mark.parametrize("asg", range(3))
@pytest.mark.parametrize("ndim", [3, 2])
def test_two_layer_boundary_matches_reference(ndim, asg):
    _fixture_flux(ndim, "bflux_%d" % (asg + 1), bc=assignment(asg, ndim))


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [capi.BC_CONTINUOUS, capi.BC_DIRICHLET_COPY])
def test_hip_refuses_potential_boundary(bad):
    """As the oracle and the 2-D library: AFH_ERR_UNSUPPORTED with the type
    in the text, before anything changes; the Dirichlet / Neumann solves
    around the refused calls agree."""
    check_phi_refusal(*hip3(), bad)


@pytest.mark.parametrize("species", ["e", "pos"])
def test_hip_refuses_continuous_flux_species(species):
    flux_refusal(*hip3(), two_box_tree(4), fixture(3), ions=IONS if species != "e" else (),
                 species=species)


@pytest.mark.parametrize("species", ["e", "pos"])
def test_2d_hip_refuses_continuous_flux_species(species):
    flux_refusal(*hip2(), two_box_tree(4, 2), fixture(2), ions=IONS if species != "e" else (),
                 species=species)
