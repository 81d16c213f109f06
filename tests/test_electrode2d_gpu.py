"""Electrodes (level-set boundaries) in libafivo_hip_2d.so, on the device.

The operators are held to tests/electrode2d_numpy.py (the reference's NDIM ==
2 formulas in numpy, float64 in the stated order) bitwise, the fused variable
pair to the split half-sweeps bitwise, and the whole time loop to the
regression logs the reference committed for programs/standard_2d/tests/
test_2d_{pos,neg}_electrode[_photoi].cfg.

Trees (8^2 boxes, the rod of test_2d_pos_electrode.cfg: from the low-y wall
at x = L/2 to 0.15 L, radius 1 mm; at the applied voltage here, so that
bc_correction is not zero):
  A  one level-1 box and one uniform refinement. The rod crosses the face
     between the two lower level-2 boxes and ends below the upper two, which
     stay constant-stencil: var/var across an x face, var/const across y
     faces, a variable level-1 box (dr > radius: the gradient-line search).
  B  tests/state2d.py's AMR tree, levels 4..7 around the rod's shaft: the rod
     crosses coarse-fine boundaries (electrode leaves on two levels).
"""
import functools
import re

import numpy as np
import pytest

import electrode2d_numpy as en
import golden
import state2d
from afh import capi, electrode
from afh.amr import AfTree
from afh.driver import Case, Simulation
from afh.model import Multigrid, Tree

pytestmark = pytest.mark.gpu

PFMG = dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
ERR_ARG, ERR_UNSUPPORTED = -1, -2
CASE = "rtest_test_2d_pos_electrode"


def _code(exc):
    return int(re.search(r"failed \((-?\d+)\)", str(exc.value)).group(1))


def _used(af):
    return [b for b in range(1, af.highest_id + 1) if af.in_use[b]]


@functools.lru_cache(maxsize=None)
def _tree(which, nc=8):
    c = Case(golden.load(CASE))
    L, o = c.ra("domain_len"), c.ra("domain_origin")
    if which == "A":
        af = AfTree(nc, o + L, [nc, nc], r_min=o)
        af.refine_up_to_lvl(2)
        return af
    assert nc == 8
    return state2d.build_tree(c, 4, 7, (0.5, 0.06), 0.05)


def _sim(which, monkeypatch, pair=True, case=CASE, grounded=False, nc=8):
    """A Simulation of the electrode case bound to tree A or B (its
    _set_electrode hands the stencils and distance lists to the library)."""
    d = dict(golden.load(case))
    if nc != 8:
        d["box_size"] = np.array([nc])
        d["coarse_grid_size_value"] = np.array([nc, nc])
    monkeypatch.setenv("AFH_PAIR2D", "1" if pair else "0")
    sim = Simulation(capi.hip_library_2d(), d, device=0, **PFMG)
    sim.af = _tree(which, nc)
    sim.electrode_grounded = grounded
    sim._bind(sim._create_tree())
    monkeypatch.delenv("AFH_PAIR2D")
    return sim


def _rand(af, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    ng = af.nc + 2
    a = np.zeros((af.highest_id, ng, ng))
    for b in _used(af):
        a[b - 1] = rng.standard_normal((ng, ng)) * scale
    return a


def _ops(sim, b):
    """(v, bc_correction, ix, dd) of box b as the driver handed them over, or
    None."""
    op = sim._ops[(tuple(sim.af.r_min[b]), tuple(sim.af.dr[b]))]
    if op is None:
        return None
    v, fb, ix, dd = op
    return v, fb * sim.lsf_boundary_value(), ix, dd


def _start(sim, seed=5):
    af = sim.af
    inv_h2 = 1 / np.min(af.dr[af.lvls[af.highest_lvl]["ids"][0]]) ** 2
    sim.tree.put_cc(sim.i_phi, _rand(af, seed, abs(sim.voltage)))
    sim.tree.put_cc(sim.i_rhs, _rand(af, seed + 1, abs(sim.voltage) * inv_h2))
    sim.tree.gc_tree(sim.i_phi)


def _fields(sim):
    return [sim.tree.get_cc(iv) for iv in (sim.i_phi, sim.i_rhs, sim.i_tmp)]


# ------------------------------------------------------------------ trees
def test_trees_have_the_cases(monkeypatch):
    sa = _sim("A", monkeypatch)
    af = sa.af
    var = {b: _ops(sa, b) is not None for b in _used(af)}
    l2 = af.lvls[2]["ids"]
    assert var[af.lvls[1]["ids"][0]] and len(l2) == 4
    assert sorted(var[b] for b in l2) == [False, False, True, True]
    # the two variable boxes are x-neighbours, each has a constant y-neighbour
    vb = [b for b in l2 if var[b]]
    assert af.ix[vb[0]][1] == af.ix[vb[1]][1] == 1
    assert np.min(af.dr[vb[0]]) > sa.lsf.length_scale
    sa.tree.close()
    sb = _sim("B", monkeypatch)
    af = sb.af
    lv = sorted({af.lvl[b] for b in sb.electrode_ids})
    leaf_lv = sorted({af.lvl[b] for b in sb.electrode_ids if not af.has_children(b)})
    assert len(lv) >= 4 and len(leaf_lv) >= 2, (lv, leaf_lv)
    # (a smoothed level's boxes are whole families of four, so no level above
    # the first has an odd box count: a wave of two 8^2 boxes is never half
    # filled there; level 1 is solved, not smoothed)
    assert all(len(af.lvls[l]["ids"]) % 4 == 0 for l in range(2, af.highest_lvl + 1))
    # fine electrode boxes take the direct distances, coarse ones the search
    drs = [np.min(af.dr[b]) for b in sb.electrode_ids]
    assert min(drs) < sb.lsf.length_scale < max(drs)
    sb.tree.close()


# -------------------------------------------------------------------- ABI
def test_abi_rules():
    lib = capi.hip_library_2d()
    for name in ("mg_set_box_stencil", "mg_set_box_lsf", "electrode_species_bc",
                 "fluid_set_update_mask"):
        assert lib.has(name), name
    nc = 8
    af = AfTree(nc, [1e-3, 1e-3], [nc, nc])
    af.refine_up_to_lvl(2)
    bc = [(capi.BC_NEUMANN, 0.0)] * 2 + [(capi.BC_DIRICHLET, 0.0)] * 2
    t = Tree(lib, af.topology(), 4, 1, device=0)
    t.set_cc_methods(1, bc, capi.RB_MG_SIDES)
    t.set_cc_prolong(1, capi.PROLONG_LINEAR)
    v = np.ones((nc, nc, 5))
    v[..., 0] = -4.0
    fb = np.zeros((nc, nc))
    ix, dd = np.array([[1, 2], [3, 4]]), np.full((2, 4), 0.5)
    mg = Multigrid(t, 1, 2, 3, **PFMG)
    mg.set_box_stencil(2, v, fb)
    mg.set_box_stencil(2, v)            # without a correction
    mg.set_box_stencil(2, None)         # removal
    mg.set_box_stencil(1, v, fb)        # a level-1 box: PFMG takes it
    mg.set_box_stencil(1, None)
    mg.set_box_lsf(3, ix, dd, fb, 4)
    mg.set_box_lsf(3, np.zeros((0, 2)), np.zeros((0, 4)), fb, 4)  # n = 0 removes
    for bad in (0, af.highest_id + 1):
        with pytest.raises(capi.AfhError) as e:
            mg.set_box_stencil(bad, v, fb)
        assert _code(e) == ERR_ARG
        with pytest.raises(capi.AfhError) as e:
            mg.set_box_lsf(bad, ix, dd, fb, 4)
        assert _code(e) == ERR_ARG
    with pytest.raises(capi.AfhError) as e:
        mg.set_box_lsf(3, np.array([[1, nc + 1]]), dd[:1], fb, 4)  # cell outside the box
    assert _code(e) == ERR_ARG
    with pytest.raises(capi.AfhError) as e:
        mg.set_box_lsf(3, ix, dd, fb, 9)  # no such variable
    assert _code(e) == ERR_ARG
    mg.fas_vcycle(True)  # nothing is left set: an ordinary V-cycle
    mg.close()
    # the exact level-1 solve takes no level-1 stencil (other levels: yes)
    md = Multigrid(t, 1, 2, 3, coarse_cycles=0, coarse_mode=capi.COARSE_DIRECT)
    md.set_box_stencil(2, v, fb)
    with pytest.raises(capi.AfhError) as e:
        md.set_box_stencil(1, v, fb)
    assert _code(e) == ERR_UNSUPPORTED and "AFH_COARSE_PFMG" in str(e.value)
    md.close()
    t.close()
    # a cylindrical tree
    tc = Tree(lib, af.topology(), 4, 1, device=0)
    tc.set_coord(capi.COORD_CYL)
    tc.set_cc_methods(1, bc, capi.RB_MG_SIDES)
    tc.set_cc_prolong(1, capi.PROLONG_LINEAR)
    mc = Multigrid(tc, 1, 2, 3, **PFMG)
    with pytest.raises(capi.AfhError) as e:
        mc.set_box_stencil(2, v, fb)
    assert _code(e) == ERR_UNSUPPORTED and "cylindrical" in str(e.value)
    with pytest.raises(capi.AfhError) as e:
        mc.set_box_lsf(2, ix, dd, fb, 4)
    assert _code(e) == ERR_UNSUPPORTED and "cylindrical" in str(e.value)
    mc.close()
    tc.close()


def test_abi_box_not_in_use():
    """A box id inside 1 .. n_boxes that the tree does not use (the children
    of a box that was derefined leave such ids behind): AFH_ERR_ARG."""
    from afh.amr import KEEP_REF, RM_REF
    lib = capi.hip_library_2d()
    nc = 8
    af = AfTree(nc, [1e-3, 1e-3], [nc, nc])
    af.refine_up_to_lvl(3)

    def fn(ids):
        return (np.array([RM_REF if af.lvl[b] == 3 and af.parent[b] == 2 else KEEP_REF
                          for b in ids]), np.zeros(len(ids), np.uint32))
    af.adjust_refinement(fn)
    free = [b for b in range(1, af.highest_id + 1) if not af.in_use[b]]
    assert len(free) == 4
    bc = [(capi.BC_NEUMANN, 0.0)] * 2 + [(capi.BC_DIRICHLET, 0.0)] * 2
    t = Tree(lib, af.topology(), 4, 1, device=0)
    t.set_cc_methods(1, bc, capi.RB_MG_SIDES)
    t.set_cc_prolong(1, capi.PROLONG_LINEAR)
    mg = Multigrid(t, 1, 2, 3, **PFMG)
    v = np.ones((nc, nc, 5))
    v[..., 0] = -4.0
    fb = np.zeros((nc, nc))
    for b in free:
        with pytest.raises(capi.AfhError) as e:
            mg.set_box_stencil(b, v, fb)
        assert _code(e) == ERR_ARG and "not in use" in str(e.value)
        with pytest.raises(capi.AfhError) as e:
            mg.set_box_lsf(b, np.array([[1, 1]]), np.full((1, 4), 0.5), fb, 4)
        assert _code(e) == ERR_ARG and "not in use" in str(e.value)
    mg.set_box_stencil(free[0] - 1, v, fb)  # its neighbour in the id space is in use
    mg.close()
    t.close()


def test_driver_rejects_cylindrical_electrode():
    d = dict(golden.load(CASE))
    d["cylindrical"] = np.array([1])
    with pytest.raises(NotImplementedError):
        Simulation(capi.hip_library_2d(), d, device=0, **PFMG)


# -------------------------------------------------------------- V-cycle
@pytest.mark.parametrize("which", ["A", "B"])
def test_residual_and_rhs_roundtrip_bitwise(which, monkeypatch):
    """After a V-cycle with set_residual, tmp of every variable box is rhs -
    (L phi - bc_correction) of the phi and rhs the device holds
    (k2_residual<StVar>), and the rhs of a variable leaf of the finest level -- 8
    half-sweeps, nothing else writes it -- is 8 round trips (rhs + b) - b of
    what was put (k2_gsrb_v / k2_rhs_roundtrip)."""
    for pair in (True, False):
        sim = _sim(which, monkeypatch, pair=pair)
        af = sim.af
        _start(sim)
        rhs0 = sim.tree.get_cc(sim.i_rhs)
        sim.mg.fas_vcycle(True)
        phi, rhs, tmp = _fields(sim)
        n_var = n_rt = 0
        for b in _used(af):
            op = _ops(sim, b)
            if op is None:
                continue
            v, fb = op[0], op[1]
            assert np.any(fb != 0)
            assert np.array_equal(tmp[b - 1][1:-1, 1:-1],
                                  en.residual_v(phi[b - 1], rhs[b - 1], v, fb)), b
            n_var += 1
            if af.lvl[b] == af.highest_lvl:
                assert np.array_equal(rhs[b - 1], en.rhs_roundtrip(rhs0[b - 1], fb, 8)), b
                assert not np.array_equal(rhs[b - 1], rhs0[b - 1])
                n_rt += 1
        assert n_var >= 3 and n_rt >= 2
        sim.tree.close()


def test_down_leg_bitwise(monkeypatch):
    """One V-cycle's down leg on tree A with the split sweeps, against numpy
    box by box: the ghost fill, four half sweeps with fills (k2_gsrb_v on the
    two variable level-2 boxes, k2_gsrb on the other two), the children's
    residual and phi restricted into the level-1 box (k2_rstr_fas<StVar>,
    k2_rstr_fas), its ghost fill, and rhs = L phi - bc_correction + tmp with
    the level-1 box's own variable stencil (k2_parent_rhs<StVar>). fas_vcycle
    without the residual pass leaves that rhs on level 1; it holds phi of the
    level-2 boxes after the sweeps through the restricted phi. The level-2
    rhs is the 8 round trips of the whole cycle."""
    _down_leg(monkeypatch, 8)


@pytest.mark.parametrize("nc", [6, 12])
def test_down_leg_bitwise_box_size(nc, monkeypatch):
    """The same at box sizes without kernels of their own."""
    _down_leg(monkeypatch, nc)


def _down_leg(monkeypatch, nc):
    sim = _sim("A", monkeypatch, pair=False, nc=nc)
    af = sim.af
    _start(sim, seed=41)
    phi0, rhs0 = sim.tree.get_cc(sim.i_phi), sim.tree.get_cc(sim.i_rhs)
    sim.mg.fas_vcycle(False)
    rhs_dev = sim.tree.get_cc(sim.i_rhs)
    kinds = {capi.BC_NEUMANN: "n", capi.BC_DIRICHLET: "d"}
    bc = [(kinds[t], v) for t, v in sim.phi_bc()]
    assert all(v == 0 for k, v in bc if k == "n")
    b1, l2 = af.lvls[1]["ids"][0], list(af.lvls[2]["ids"])
    ops = {b: _ops(sim, b) for b in [b1] + l2}
    assert ops[b1] is not None and sum(ops[b] is not None for b in l2) == 2
    sim.tree.close()
    assert nc == af.nc
    h = nc // 2
    # (put_cc leaves the ghost cells it was given; gc_tree fills the sides)
    P = {b: phi0[b - 1].copy() for b in l2}
    R = {b: rhs0[b - 1].copy() for b in l2}
    nbs = {b: tuple(af.neighbors[b][:4]) for b in l2}
    c2 = en.lpl_coef(af.dr[l2[0]])
    en.fill_sides(P, nbs, bc)
    for s in range(1, 5):
        for b in l2:
            if ops[b] is not None:
                en.gsrb_v(P[b], R[b], ops[b][0], ops[b][1], s)
            else:
                en.gsrb_c(P[b], R[b], c2, s)
        en.fill_sides(P, nbs, bc)
    p1 = phi0[b1 - 1].copy()
    tmp1 = np.zeros((nc + 2, nc + 2))
    for b in l2:
        if ops[b] is not None:
            rr, rp = en.rstr_fas_v(P[b], R[b], ops[b][0], ops[b][1])
        else:
            res = R[b][1:-1, 1:-1] - en.apply_c(P[b], c2)
            f = P[b][1:-1, 1:-1]
            rr = 0.25 * (res[0::2, 0::2] + res[0::2, 1::2] + res[1::2, 0::2] + res[1::2, 1::2])
            rp = 0.25 * (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2])
        i0, j0 = ((af.ix[b][0] - 1) & 1) * h, ((af.ix[b][1] - 1) & 1) * h
        tmp1[1 + j0:1 + j0 + h, 1 + i0:1 + i0 + h] = rr
        p1[1 + j0:1 + j0 + h, 1 + i0:1 + i0 + h] = rp
    en.fill_sides({b1: p1}, {b1: tuple(af.neighbors[b1][:4])}, bc)
    ref, _ = en.parent_rhs_v(p1, rhs0[b1 - 1], tmp1, ops[b1][0], ops[b1][1])
    got = rhs_dev[b1 - 1][1:-1, 1:-1]
    print("down leg level-1 rhs: %d of %d not bitwise" %
          (np.count_nonzero(got != ref[1:-1, 1:-1]), got.size))
    assert np.array_equal(got, ref[1:-1, 1:-1])
    for b in l2:
        fb = ops[b][1] if ops[b] is not None else None
        assert np.array_equal(rhs_dev[b - 1], en.rhs_roundtrip(rhs0[b - 1], fb, 8)), b


def test_vcycles_converge_through_the_electrode(monkeypatch):
    """FAS V-cycles on tree B with variable boxes on every level (k2_gsrb_v,
    k2_rstr_fas<StVar>, k2_parent_rhs<StVar> and the level-1 rows together): the
    residual falls to rounding."""
    sim = _sim("B", monkeypatch)
    _start(sim)
    r = [sim.mg.fas_vcycle_maxres() for _ in range(14)]
    print("electrode V-cycle residuals", r)
    assert r[-1] < 1e-9 * r[0]
    sim.tree.close()


@pytest.mark.parametrize("which,nc", [("A", 8), ("B", 8), ("A", 4), ("A", 16), ("A", 6),
                                      ("A", 12)])
def test_fused_variable_pair_equals_split(which, nc, monkeypatch):
    """AFH_PAIR2D=1 (k2_pair_box<VAR = true> on the levels with variable boxes) against
    AFH_PAIR2D=0 (k2_gsrb + k2_gsrb_v + k2_gc twice), bitwise: after a
    V-cycle without the residual pass -- the rhs and tmp of the coarser levels
    are then as the down leg left them (restriction and rhs = L phi + tmp),
    phi as the up leg did -- then after a whole V-cycle with the residual,
    one more (captured) and one more (replayed from the graph). phi is
    compared with its face ghost cells (the gradient reads them), rhs and tmp
    on the interiors."""
    out = {}
    for pair in (True, False):
        sim = _sim(which, monkeypatch, pair=pair, nc=nc)
        _start(sim)
        sim.mg.fas_vcycle(False)
        snaps = [_fields(sim)]
        for _ in range(3):  # eager, capture, replay
            sim.mg.fas_vcycle(True)
            snaps.append(_fields(sim))
        out[pair] = snaps
        sim.tree.close()
    ix = np.asarray(_used(_tree(which, nc))) - 1
    inner = (slice(None), slice(1, -1), slice(1, -1))

    def faces(a):  # the image without its four corner ghost cells
        a = a[ix].copy()
        a[:, 0, 0] = a[:, 0, -1] = a[:, -1, 0] = a[:, -1, -1] = 0.0
        return a
    for a, b in zip(out[True], out[False]):
        assert np.array_equal(faces(a[0]), faces(b[0]))
        for fa, fb in zip(a[1:], b[1:]):
            assert np.array_equal(fa[ix][inner], fb[ix][inner])
    assert not np.array_equal(out[True][1][0][ix], out[True][3][0][ix])


def test_graph_invalidation(monkeypatch):
    """V-cycle, change one box's bc_correction, V-cycle (twice: the second is
    captured): bitwise a fresh multigrid given the second correction from
    the start, run from the same phi and rhs."""
    sim = _sim("B", monkeypatch)
    af = sim.af
    b = next(b for b in sim.electrode_ids if af.lvl[b] == af.highest_lvl)
    v, fb, ix, dd = _ops(sim, b)
    fb2 = fb * 1.25
    _start(sim)
    for _ in range(3):  # the graph of this variant is captured and replayed
        sim.mg.fas_vcycle(True)
    sim.mg.set_box_stencil(b, v, fb2)
    _start(sim, seed=9)
    got = []
    for _ in range(3):
        sim.mg.fas_vcycle(True)
        got.append(_fields(sim))
    sim.tree.close()
    ref_sim = _sim("B", monkeypatch)
    ref_sim.mg.set_box_stencil(b, v, fb2)
    _start(ref_sim, seed=9)
    ix_ = np.asarray(_used(af)) - 1
    for g in got:
        ref_sim.mg.fas_vcycle(True)
        for fa, fr in zip(g, _fields(ref_sim)):
            assert np.array_equal(fa[ix_][:, 1:-1, 1:-1], fr[ix_][:, 1:-1, 1:-1])
    ref_sim.tree.close()


def test_level1_solve(monkeypatch):
    """Tree A with PFMG: after a V-cycle of level 1 alone (the level-1 solve)
    the level-1 residual with the variable rows satisfies PFMG's stopping
    rule, |r|_2 <= coarse_tol |b|_2 with b the gathered rhs (+ boundary terms
    and bc_correction). With every stencil removed the solve is bitwise that
    of a multigrid that never had one."""
    sim = _sim("A", monkeypatch)
    af = sim.af
    b1 = af.lvls[1]["ids"][0]
    v, fb, _, _ = _ops(sim, b1)
    _start(sim)
    sim.mg.fas_vcycle(True, 1)
    phi, rhs, tmp = _fields(sim)
    res = en.residual_v(phi[b1 - 1], rhs[b1 - 1], v, fb)
    assert np.array_equal(tmp[b1 - 1][1:-1, 1:-1], res)
    # b: the rhs the solver gathers, rhs + bc_correction + the Dirichlet walls'
    # terms -2 c value with c the cell's own coefficient towards the wall
    # (stencil_handle_boundaries; the x walls are homogeneous Neumann)
    bcs = sim.phi_bc()
    assert [t for t, _ in bcs] == [capi.BC_NEUMANN] * 2 + [capi.BC_DIRICHLET] * 2
    assert bcs[0][1] == 0 and bcs[1][1] == 0
    bvec = rhs[b1 - 1][1:-1, 1:-1] + fb
    bvec[0] = bvec[0] + (-2 * v[0, :, 3]) * bcs[2][1]
    bvec[-1] = bvec[-1] + (-2 * v[-1, :, 4]) * bcs[3][1]
    ratio = np.linalg.norm(res) / np.linalg.norm(bvec)
    print("level-1 |r|/|b| =", ratio)
    assert ratio < 1e-6
    for b in _used(af):
        if _ops(sim, b) is not None:
            sim.mg.set_box_stencil(b, None)
            sim.mg.set_box_lsf(b, np.zeros((0, 2)), np.zeros((0, 4)), fb, sim.i_lsf)
    _start(sim, seed=3)
    sim.mg.fas_vcycle(True)
    got = _fields(sim)
    sim.tree.close()
    d = dict(golden.load(CASE))
    d["use_electrode"] = np.array([0])
    plain = Simulation(capi.hip_library_2d(), d, device=0, **PFMG)
    plain.af = af
    plain._bind(plain._create_tree())
    _start(plain, seed=3)
    plain.mg.fas_vcycle(True)
    for fa, fr in zip(got, _fields(plain)):
        assert np.array_equal(fa, fr)
    plain.tree.close()


# -------------------------------------------------------------- gradient
def test_lsf_gradient_bitwise(monkeypatch):
    """Faces and |E| of every box: mg_box_lpl_gradient, on electrode leaves
    then mg_box_lpllsf_gradient in list order and the norm of the corrected
    faces. The rod's lists hold cells with lsf < 0."""
    n_corr, n_neg, n_shared = _lsf_gradient(_sim("B", monkeypatch))
    # (the rod's lists hold no two cells that write one face: that case is
    # test_lsf_gradient_shared_faces_bitwise)
    assert n_corr > 20 and n_neg > 0, (n_corr, n_neg, n_shared)


@pytest.mark.parametrize("nc", [6, 12, 32])
def test_lsf_gradient_bitwise_box_size(nc, monkeypatch):
    """k2_lsf_gradient and k2_gradient on the two-level tree at box sizes
    without kernels of their own, and at 32, the largest size whose cells the
    kernel's entry map holds; the electrode's two leaves have corrected
    faces."""
    n_corr, _, _ = _lsf_gradient(_sim("A", monkeypatch, nc=nc))
    assert n_corr > 0


def test_lsf_above_32_is_refused(monkeypatch):
    """afh_mg_set_box_lsf with n_cell > 32: AFH_ERR_UNSUPPORTED, the size in
    the text (afivo_hip_2d.h); the driver hands its lists over in _bind."""
    with pytest.raises(capi.AfhError, match="box size 34") as e:
        _sim("A", monkeypatch, nc=34)
    assert _code(e) == ERR_UNSUPPORTED


def _lsf_gradient(sim):
    af = sim.af
    sim.tree.put_cc(sim.i_phi, _rand(af, 21, abs(sim.voltage)))
    sim.mg.compute_phi_gradient(sim.f_field, -1.0, sim.i_efld)
    phi, lsf = sim.tree.get_cc(sim.i_phi), sim.tree.get_cc(sim.i_lsf)
    fc, nrm = sim.tree.get_fc(sim.f_field), sim.tree.get_cc(sim.i_efld)
    nc = af.nc
    n_shared = n_neg = n_corr = 0
    for b in _used(af):
        ref = en.lpl_gradient(phi[b - 1], af.dr[b], -1.0)
        op = _ops(sim, b)
        if op is not None and not af.has_children(b):
            _, _, ix, dd = op
            cells = {(int(i), int(j)): n for n, (i, j) in enumerate(ix)}
            for (i, j), n in cells.items():
                if lsf[b - 1][j, i] < 0:
                    n_neg += 1
                m = cells.get((i + 1, j))
                if m is not None and dd[n][1] < 1 and dd[m][0] < 1 and \
                        lsf[b - 1][j, i] >= 0 and lsf[b - 1][j, i + 1] >= 0:
                    n_shared += 1
            before = ref.copy()
            en.lsf_gradient(phi[b - 1], lsf[b - 1], ref, ix, dd,
                            np.full((nc, nc), sim.lsf_boundary_value()), af.dr[b], -1.0)
            n_corr += int(np.sum(before != ref))
        got = fc[b - 1]
        assert np.array_equal(got[0][:nc, :], ref[0][:nc, :]), b
        assert np.array_equal(got[1][:, :nc], ref[1][:, :nc]), b
        assert np.array_equal(nrm[b - 1][1:-1, 1:-1], en.field_norm(ref)), b
    sim.tree.close()
    return n_corr, n_neg, n_shared


def test_lsf_gradient_shared_faces_bitwise(monkeypatch):
    """A distance list in which neighbouring cells write the same face, in
    both list orders and in both directions, and a cell with lsf < 0: the
    face keeps the later entry's value, as the serial loop leaves it
    (k2_lsf_gradient's entry map and its skip of faces a later entry
    rewrites). The rod's own lists have no such pair, so the list, the level
    set and the boundary values of one finest electrode leaf are set here."""
    sim = _sim("B", monkeypatch)
    af = sim.af
    nc = af.nc
    b = next(b for b in sim.electrode_ids
             if af.lvl[b] == af.highest_lvl and not af.has_children(b))
    # (i, j), distances towards i-1, i+1, j-1, j+1
    entries = [((2, 2), (1, .5, 1, 1)), ((3, 2), (.25, 1, 1, 1)),      # x, low cell first
               ((6, 4), (.3, 1, 1, 1)), ((5, 4), (1, .6, 1, 1)),       # x, high cell first
               ((2, 6), (1, 1, 1, .4)), ((2, 7), (1, 1, .7, 1)),       # y, low cell first
               ((5, 7), (1, 1, .2, .9)), ((5, 6), (.8, 1, 1, .35)),    # y, high cell first
               ((7, 2), (.5, .5, .5, .5)),                             # lsf < 0: skipped
               ((8, 2), (.45, 1, 1, 1)),       # its neighbour: not rewritten by (7, 2)
               ((1, 8), (.5, 1, 1, .5)), ((8, 8), (1, .5, 1, .5))]     # the box's outer faces
    ix = np.array([e[0] for e in entries], np.int32)
    dd = np.array([e[1] for e in entries], float)
    rng = np.random.default_rng(77)
    bval = rng.standard_normal((nc, nc)) * abs(sim.voltage)
    lsf = sim.tree.get_cc(sim.i_lsf)
    lsf[b - 1] = 1.0
    lsf[b - 1][2, 7] = -1.0
    sim.tree.put_cc(sim.i_lsf, lsf)
    sim.mg.set_box_lsf(b, ix, dd, bval, sim.i_lsf)
    sim.tree.put_cc(sim.i_phi, _rand(af, 23, abs(sim.voltage)))
    sim.mg.compute_phi_gradient(sim.f_field, -1.0, sim.i_efld)
    phi = sim.tree.get_cc(sim.i_phi)
    fc, nrm = sim.tree.get_fc(sim.f_field), sim.tree.get_cc(sim.i_efld)
    sim.tree.close()
    cells = {tuple(c): n for n, c in enumerate(ix.tolist())}
    n_shared = 0
    for (i, j), n in cells.items():
        for d, (di, dj) in enumerate(((1, 0), (0, 1))):
            m = cells.get((i + di, j + dj))
            if m is not None and dd[n][2 * d + 1] < 1 and dd[m][2 * d] < 1 and \
                    lsf[b - 1][j, i] >= 0 and lsf[b - 1][j + dj, i + di] >= 0:
                n_shared += 1
    assert n_shared == 4
    plain = en.lpl_gradient(phi[b - 1], af.dr[b], -1.0)
    ref = plain.copy()
    en.lsf_gradient(phi[b - 1], lsf[b - 1], ref, ix, dd, bval, af.dr[b], -1.0)
    assert np.count_nonzero(ref != plain) == 11  # 15 writes, 4 of them rewritten
    # the order matters: the reversed list gives other faces
    rev = plain.copy()
    en.lsf_gradient(phi[b - 1], lsf[b - 1], rev, ix[::-1], dd[::-1], bval, af.dr[b], -1.0)
    assert np.count_nonzero(rev != ref) == 4
    got = fc[b - 1]
    assert np.array_equal(got[0][:nc, :], ref[0][:nc, :])
    assert np.array_equal(got[1][:, :nc], ref[1][:, :nc])
    assert np.array_equal(nrm[b - 1][1:-1, 1:-1], en.field_norm(ref))


# --------------------------------------------------------------- species
@pytest.mark.parametrize("neumann_zero", [True, False])
def test_electrode_species_bc_bitwise(neumann_zero, monkeypatch):
    sim = _sim("B", monkeypatch)
    af = sim.af
    ivs = [sim.species_itree[n] for n in sim.plasma]
    a = {iv: np.abs(_rand(af, 30 + iv, 1e15)) for iv in ivs}
    for iv in ivs:
        sim.tree.put_cc(iv, a[iv])
    sim.fluid.electrode_species_bc(sim.i_lsf, sim.i_1pos_ion, sim.electrode_ids, neumann_zero)
    lsf = sim.tree.get_cc(sim.i_lsf)
    n_in = n_edge = 0
    for b in _used(af):
        ref = {iv: a[iv][b - 1].copy() for iv in ivs}
        if b in sim.electrode_ids:
            en.electrode_species_bc([ref[iv] for iv in ivs], ref[sim.i_electron],
                                    ref[sim.i_1pos_ion], lsf[b - 1], neumann_zero)
            inside = lsf[b - 1][1:-1, 1:-1] < 0
            n_in += int(inside.sum())
            n_edge += int((ref[sim.i_electron][1:-1, 1:-1][inside] > 0).sum())
        for iv in ivs:
            assert np.array_equal(sim.tree.get_cc(iv)[b - 1], ref[iv]), (b, iv)
    assert n_in > 50 and (n_edge > 10) == neumann_zero
    sim.tree.close()


@pytest.mark.parametrize("case", [CASE, CASE + "_photoi"])
def test_update_mask_bitwise(case, monkeypatch):
    """k2_update<MASK = true>, with and without PHOTO, against the unmasked
    update of the same state: a cell with lsf <= 0 is the weighted sum of the previous
    states, every other cell the unmasked result; the last step's chemistry
    limit is the minimum over the leaves that have a cell to update, and
    1e100 when the only leaves given such cells lie inside the electrode."""
    sim = _sim("B", monkeypatch, case=case)
    af = sim.af
    ivs = [sim.species_itree[n] for n in sim.plasma]
    for iv in ivs:
        for s in (0, 1):
            sim.tree.put_cc(iv + s, np.abs(_rand(af, 50 + 3 * iv + s, 1e16)) + 1e13)
    sim.tree.put_cc(sim.i_efld, np.abs(_rand(af, 70, 3e6)))
    sim.tree.put_fc(sim.f_flux, np.random.default_rng(71).standard_normal(
        (af.highest_id, 2, af.nc + 1, af.nc + 1)) * 1e20)
    if sim.photoi:
        sim.tree.put_cc(sim.i_photo, np.abs(_rand(af, 72, 1e24)))
    dt, w = 1e-12, [0.5, 0.5]
    lim_m = sim.fluid.flux_update_densities(dt, 1, [0, 1], w, 0, True)
    masked = {iv: sim.tree.get_cc(iv) for iv in ivs}
    for iv in ivs:  # state 0 was overwritten: put it back
        sim.tree.put_cc(iv, np.abs(_rand(af, 50 + 3 * iv, 1e16)) + 1e13)
    sim.fluid.set_update_mask(0)
    lim_u = sim.fluid.flux_update_densities(dt, 1, [0, 1], w, 0, True)
    plain = {iv: sim.tree.get_cc(iv) for iv in ivs}
    lsf = sim.tree.get_cc(sim.i_lsf)
    prev = {iv: [np.abs(_rand(af, 50 + 3 * iv + s, 1e16)) + 1e13 for s in (0, 1)] for iv in ivs}
    n_off = 0
    for l in range(1, af.highest_lvl + 1):
        for b in af.lvls[l]["leaves"]:
            m = en.update_mask(lsf[b - 1])
            n_off += int((~m).sum())
            for iv in ivs:
                keep = (0.0 + w[0] * prev[iv][0][b - 1]) + w[1] * prev[iv][1][b - 1]
                ref = np.where(m, plain[iv][b - 1][1:-1, 1:-1], keep[1:-1, 1:-1])
                assert np.array_equal(masked[iv][b - 1][1:-1, 1:-1], ref), (b, iv)
    assert n_off > 20
    assert lim_m[0] >= lim_u[0] and lim_m[0] < 1e100
    # the limit is the minimum over the leaves that have a cell to update:
    # with every second leaf put wholly inside (either half), the masked
    # limit is bitwise the unmasked limit of the same state with no field in
    # those leaves (they then hold no minimum); one of the halves holds the
    # tree's minimum, so for it the limit really moves
    leaves = [b for l in range(1, af.highest_lvl + 1) for b in af.lvls[l]["leaves"]]
    E = np.abs(_rand(af, 70, 3e6))

    def limit(field, mask):
        for iv in ivs:
            sim.tree.put_cc(iv, prev[iv][0])
        sim.tree.put_cc(sim.i_efld, field)
        sim.fluid.set_update_mask(sim.i_lsf if mask else 0)
        return sim.fluid.flux_update_densities(dt, 1, [0, 1], w, 0, True)[0]
    hot = limit(E, False)
    assert hot == lim_u[0]
    moved = 0
    for half in (leaves[0::2], leaves[1::2]):
        lsf2, E_cold = np.ones_like(lsf), E.copy()
        for b in half:
            lsf2[b - 1] = -1.0
            E_cold[b - 1] = 0.0
        sim.tree.put_cc(sim.i_lsf, lsf2)
        cold = limit(E_cold, False)
        assert limit(E, True) == cold
        assert cold >= hot
        moved += cold > hot
    assert moved >= 1
    # every leaf wholly inside the electrode: no chemistry limit at all
    sim.fluid.set_update_mask(sim.i_lsf)
    sim.tree.put_cc(sim.i_lsf, -np.ones_like(lsf))
    lim_in = sim.fluid.flux_update_densities(dt, 1, [0, 1], w, 0, True)
    assert lim_in[0] == 1e100
    sim.tree.close()


def test_refine_flags_electrode_box(monkeypatch):
    sim = _sim("B", monkeypatch)
    af = sim.af
    for iv in (sim.i_electron, sim.i_efld):
        sim.tree.put_cc(iv, np.zeros((af.highest_id, af.nc + 2, af.nc + 2)))
    desc = sim.refine_desc()
    f0, _ = sim.fluid.refine_flags(desc, None)
    f1, _ = sim.fluid.refine_flags(desc, sim.electrode_box)
    ids = range(1, af.highest_id + 1)
    max_dx = np.array([np.max(af.dr[b]) if af.in_use[b] else 0.0 for b in ids])
    # the refine_min_dx rule does not apply on this tree
    assert np.min(max_dx[max_dx > 0]) >= 2 * desc.min_dx
    forced = max_dx > desc.max_dx
    limited = np.zeros(af.highest_id, bool)
    for b in _used(af):
        rmin, rmax = af.r_min[b], af.r_min[b] + af.dr[b] * af.nc
        for n in range(desc.n_limits):
            lo, hi = list(desc.limit_rmin[n])[:2], list(desc.limit_rmax[n])[:2]
            if max_dx[b - 1] < 2 * desc.limit_dr[n] and np.all(rmin >= lo) and np.all(rmax <= hi):
                limited[b - 1] = True
    ref = en.refine_electrode(f0, sim.electrode_box, max_dx, desc.electrode_dx, limited, forced)
    used = np.asarray(_used(af)) - 1
    assert np.array_equal(f1[used], ref[used])
    assert np.sum(f1[used] != f0[used]) > 3
    sim.tree.close()


# ------------------------------------------------------------- time loops
# Largest relative deviation of a log row from the reference's, measured on
# the MI355X (profiles/electrode2d_pytest_gpu.txt), and the bound: ten times
# that, never above compare_logs' 1e-5
MEASURED = {"test_2d_pos_electrode": 4.3e-8, "test_2d_pos_electrode_photoi": 3.9e-8,
            "test_2d_neg_electrode": 3.8e-8, "test_2d_neg_electrode_photoi": 4.9e-8}


@pytest.mark.parametrize("name", sorted(MEASURED))
def test_electrode_rtest_hip(name):
    """The whole time loop of programs/standard_2d/tests/<name>.cfg on the
    device with the reference's PFMG level-1 solve (50 cycles, 1e-6): every
    row of the committed regression log within compare_logs' atol 1e-8 and
    min(10 x measured, 1e-5).

    Measured on the MI355X: 4.2e-8, 3.7e-8, 3.8e-8 and 4.9e-8 (pos, neg,
    pos_photoi, neg_photoi), the logs' print precision. The rows depend on
    the driver refreshing the densities' parents and ghost cells at every
    output, as the reference's output_write does (its silo branch): without
    it electrode_species_bc reads stale ghost cells after the second output
    and the negative cases, where electrons leave the electrode, drift to
    1e-3 (plain) and 1e-2 (photoionization) from the 0.4 ns row on."""
    sim = Simulation(capi.hip_library_2d(), golden.load("rtest_" + name), device=0, **PFMG)
    assert sim.ndim == 2 and sim.lsf is not None and not sim.faces_from_phi
    log = np.asarray(sim.run())
    ref = golden.load("rtest_" + name)["rtest_log"]
    assert log.shape == ref.shape
    rel = np.abs(log - ref) / np.maximum(np.abs(ref), 1e-300)
    print(name, "max rel per row", rel.max(axis=1))
    assert np.array_equal(log[:, 0], ref[:, 0])
    assert np.allclose(log[:, 1], ref[:, 1], rtol=1e-12, atol=0)
    rtol = min(10 * MEASURED[name], 1e-5)
    bad = ~np.isclose(log, ref, rtol=rtol, atol=1e-8)
    assert not bad.any(), (rtol, np.argwhere(bad)[:5], rel.max())
