"""Box sizes outside the kernels' power-of-two templates: the kernels that the
Heun / FMG chain of test_hip_parity.py (SIZE_TOPOS there) does not reach, at
n_cell 6 and 12 (no template, decodes by division; column width 2 and 4) and,
for the tree operations, at 2 (the smallest legal size: a child covers one
parent cell, hnc = 1, the second ghost layer is cell 1).

Every comparison is HIP == C oracle on every cell of every box; the oracle is
held to the reference's compiled numerics at these sizes by
test_oracle_golden.py (fixtures amr2, amr6, amr12). The tree is the one of
test_hip_parity.size_tree: 82 boxes on 3 levels, coarse-fine faces on levels
2 and 3.

CPU: what both libraries refuse (n_cell odd, below 2, above the largest size
the kernels serve) is refused before any device call, with the size in the
text.
"""
import numpy as np
import pytest

import golden
from afh import capi, electrode
from afh.amr import DO_REF, RM_REF, AfTree
from afh.model import Tree
from afh.streamer import FV, IV, StreamerCase, seed_state, tables_from
from afh.tree import uniform_tree_2d
from test_hip_parity import size_tree
from test_regrid import refine_desc

DOM = (2e-3, 1e-3, 1e-3)  # size_tree's domain


def both():
    """(library, device) of the HIP library and of the oracle."""
    return (capi.hip_library(), 0), (capi.oracle_library(), -1)


def in_use(topo):
    return np.concatenate([np.asarray(topo["lvl_ids_%d" % l]) for l in
                           range(1, int(topo["highest_lvl"]) + 1)]) - 1


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("nc", [0, 1, 3, 7, 130, 256])
def test_3d_tree_create_refuses_box_size(nc):
    """afh_tree_create: n_cell even, 2 .. 128 (include/afivo_hip.h); the
    check comes before the first device call, so it needs no GPU."""
    topo = dict(size_tree(4))
    topo["nc"] = np.int32(nc)
    with pytest.raises(capi.AfhError, match=r"n_cell %d\b" % nc):
        Tree(capi.hip_library(), topo, 1, 0)


@pytest.mark.parametrize("nc", [0, 3, 1026, 4096])
def test_2d_tree_create_refuses_box_size(nc):
    """The 2-D afh_tree_create: n_cell even, 2 .. 1024 (afivo_hip_2d.h)."""
    topo = dict(uniform_tree_2d(4, (8, 8), (1e-3, 1e-3), 2))
    topo["nc"] = np.int32(nc)
    with pytest.raises(capi.AfhError, match=r"n_cell %d\b" % nc):
        Tree(capi.hip_library_2d(), topo, 1, 0)


# ------------------------------------------------------- ghost cells, restrict
RB = {"interp": capi.RB_GC_INTERP, "interp_lim": capi.RB_GC_INTERP_LIM,
      "mg_sides": capi.RB_MG_SIDES}


def _filled(nc, rb, corners, restrict):
    topo = size_tree(nc)
    out = []
    v = None
    for lib, dev in both():
        t = Tree(lib, topo, 1, 0, device=dev)
        if v is None:
            v = 0.5 + np.random.default_rng(nc).random(t.cc_shape)
        # Neumann and Dirichlet faces (field_bc_homogeneous)
        t.set_cc_methods(1, StreamerCase.phi_bc(3.0), RB[rb])
        t.put_cc(1, v)
        if restrict:
            t.restrict_tree(1)
        t.gc_tree(1, corners)
        out.append(t.get_cc(1))
        t.close()
    return v, out


@pytest.mark.gpu
@pytest.mark.parametrize("corners", [True, False])
@pytest.mark.parametrize("rb", sorted(RB))
@pytest.mark.parametrize("nc", [2, 6, 12])
def test_gc_tree_equals_oracle(nc, rb, corners):
    """af_gc_tree: copies, physical boundaries and every refinement-boundary
    method, with and without edges and corners (k_gc_faces, k_gc_corners)."""
    v, (a, b) = _filled(nc, rb, corners, False)
    assert np.array_equal(a, b), np.max(np.abs(a - b))
    assert not np.array_equal(a, v)
    # interiors untouched; without corners the corner cells keep their values
    assert np.array_equal(golden.interior(a), golden.interior(v))
    if not corners:
        assert np.array_equal(a[:, ::nc + 1, ::nc + 1, ::nc + 1],
                              v[:, ::nc + 1, ::nc + 1, ::nc + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("nc", [2, 6, 12])
def test_restrict_tree_equals_oracle(nc):
    v, (a, b) = _filled(nc, "interp", True, True)
    assert np.array_equal(a, b), np.max(np.abs(a - b))
    assert not np.array_equal(golden.interior(a), golden.interior(v))


# --------------------------------------------------------------------- regrid
def _regrid_steps(nc):
    """Topologies of a tree that is refined near one corner, then refined
    near the other while the first region is derefined."""
    af = AfTree(nc, list(DOM), [2 * nc, nc, nc])
    af.refine_up_to_lvl(2)
    topos = [af.topology()]

    def rule(corner):
        def fn(ids):
            f = []
            for b in ids:
                r0 = np.asarray(af.r_min[b])
                r1 = r0 + nc * np.asarray(af.dr[b])
                if corner == 0:
                    near = np.all(r0 < 0.6e-3)
                else:
                    near = r1[0] > 1.4e-3 and np.all(r0[1:] < 0.6e-3)
                f.append(DO_REF if near and af.lvl[b] < 3 else RM_REF)
            return np.array(f), np.zeros(len(ids), np.uint32)
        return fn

    for corner in (0, 1):
        info = af.adjust_refinement(rule(corner))
        assert info.n_add > 0
        if corner:
            assert info.n_rm > 0
        topos.append(af.topology())
    return topos


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["linear", "limit"])
@pytest.mark.parametrize("nc", [6, 12])
def test_regrid_equals_oracle(nc, method):
    """afh_tree_regrid with af_prolong_linear and af_prolong_limit: restricted
    parents, copied boxes, prolonged new boxes with their ghost cells."""
    topos = _regrid_steps(nc)
    res = []
    v = None
    for lib, dev in both():
        t = Tree(lib, topos[0], 1, 0, device=dev)
        t.set_cc_methods(1, [(capi.BC_NEUMANN, 0.0)] * 6, capi.RB_GC_INTERP_LIM)
        t.set_cc_prolong(1, capi.PROLONG_LINEAR if method == "linear" else capi.PROLONG_LIMIT)
        if v is None:
            c = np.stack([electrode.cell_centers(topos[0]["meta_r_min"][b],
                                                 topos[0]["meta_dr"][b], nc, 0, nc + 1)
                          for b in range(t.n_boxes)])
            # a steep bump (the limiter acts) on a background
            d2 = np.sum((c - np.array([0.5e-3, 0.4e-3, 0.45e-3])) ** 2, axis=-1)
            v = 1e15 + 5e18 * np.exp(-d2 / (1.2e-4) ** 2)
            assert v.shape == t.cc_shape
        t.put_cc(1, v)
        t.restrict_tree(1)
        t.gc_tree(1)
        states = []
        for topo in topos[1:]:
            t = t.regrid(topo)
            states.append(t.get_cc(1)[in_use(topo)])
        res.append(states)
    for a, b in zip(*res):
        assert np.array_equal(a, b), np.max(np.abs(a - b))
        assert np.max(a) > 1e18


# -------------------------------------------------------------- refine flags
def _case_pair(nc, coarse=0, **kw):
    g = golden.load("uni8")
    td, chem = tables_from(g)
    topo = size_tree(nc)
    cases = []
    for lib, dev in both():
        c = StreamerCase(lib, topo, td, chem, float(g["current_voltage"]), device=dev,
                         coarse_cycles=coarse, **kw)
        seed_state(c)
        cases.append(c)
    return topo, cases


@pytest.mark.gpu
@pytest.mark.parametrize("nc", [6, 12])
def test_refine_flags_equal_oracle(nc):
    """afh_refine_flags (default_refinement + cell_to_ref_flags) on the
    seeded state's field: flags and neighbour masks of every box."""
    topo, cases = _case_pair(nc)
    p = np.zeros(28)
    # adx, adx_fac, min_dens, derefine_dx, max_dx, min_dx, init_fac
    p[:7] = [0.05, 1.0, 1e16, 1e-4, 1e-3, 1e-7, 0.25]
    p[7:10] = [0.8e-3, 0.5e-3, 0.5e-3]      # seed r0, r1, width
    p[10:13] = [0.8e-3, 0.5e-3, 0.8e-3]
    p[13] = 5e-5
    p[14] = 2e-5                             # region: dr, rmin, rmax
    p[15:18] = [1.5e-3, 0.0, 0.75e-3]
    p[18:21] = [2e-3, 0.3e-3, 1e-3]
    p[21] = 1e-4                             # limit: dr, rmin, rmax
    p[22:25] = [0.0, 0.5e-3, 0.0]
    p[25:28] = [1e-3, 1e-3, 0.5e-3]
    desc = refine_desc({"refine_params": p, "refine_buffer": [2]})
    out = []
    for c in cases:
        c.field_compute(0, check_residual=False)
        out.append(c.fluid.refine_flags(desc))
    (fa, ma), (fb, mb) = out
    assert np.array_equal(fa, fb) and np.array_equal(ma, mb)
    assert len(set(fa[in_use(topo)].tolist())) >= 2 and np.any(ma != 0)


# ------------------------------------------------------------------ electrode
def _rod_case_pair(nc, coarse):
    """The field solve with a rod electrode from the top face (the stencils
    of afh.electrode, held to the reference's by test_electrode_ops.py)."""
    topo, cases = _case_pair(nc, coarse, n_var_cell=15)
    dom = np.asarray(DOM)
    f = electrode.RodLSF(np.array([0.25, 0.5, 1.0]) * dom, np.array([0.25, 0.5, 0.6]) * dom,
                         0.12 * dom[2])
    nb = int(topo["n_boxes"])
    lsf = np.stack([f(electrode.cell_centers(topo["meta_r_min"][b], topo["meta_dr"][b],
                                             nc, 0, nc + 1)) for b in range(nb)])
    v0 = cases[0].voltage
    ops = electrode.boxes_operators(
        f, [(lsf[b][1:-1, 1:-1, 1:-1], topo["meta_r_min"][b], topo["meta_dr"][b])
            for b in range(nb)], nc, v0)
    st = {b + 1: (op[0], op[1]) for b, op in enumerate(ops) if op is not None}
    faces = {b + 1: (op[2], op[3], np.full((nc, nc, nc), v0))
             for b, op in enumerate(ops) if op is not None}
    lvl = np.asarray(topo["meta_lvl"])
    assert {int(lvl[b - 1]) for b in st} == {1, 2, 3}  # electrode boxes on every level
    for c in cases:
        c.tree.put_cc(golden.IVS["lsf"], lsf)
        c.set_electrode(golden.IVS["lsf"], st, faces)
    return topo, cases, lsf, sorted(st)


@pytest.mark.gpu
@pytest.mark.parametrize("nc", [6, 12])
def test_electrode_field_solve_equals_oracle(nc):
    """Two V-cycles through the electrode stencils, the gradient with the
    electrode faces (k_lsf_gradient), FMG without and with guess. Level 1
    with AFH_COARSE_DIRECT (the electrode's level-1 boxes make the other
    solve a Gauss-Seidel iteration to stationarity, a minute on the oracle
    at this level-1 grid)."""
    topo, cases, _, _ = _rod_case_pair(nc, 0)
    out = []
    for c in cases:
        c.fluid.field_set_rhs(IV["rhs"], 0)
        c.mg.fas_vcycle(True)
        c.mg.fas_vcycle(True)
        c.field_from_potential()
        r = [c.tree.get_cc(IV[n]) for n in ("phi", "tmp", "rhs", "efld")]
        r += golden.faces(c.tree.get_fc(FV["field"]))
        c.mg.fas_fmg(True, have_guess=False)
        c.mg.fas_fmg(True, have_guess=True)
        r += [c.tree.get_cc(IV[n]) for n in ("phi", "tmp", "rhs")]
        out.append(r)
    for q, (a, b) in enumerate(zip(*out)):
        assert np.array_equal(a, b), (q, np.max(np.abs(a - b)))


@pytest.mark.gpu
@pytest.mark.parametrize("neumann", [True, False])
@pytest.mark.parametrize("nc", [6, 12])
def test_electrode_species_bc_and_mask_equal_oracle(nc, neumann):
    """afh_electrode_species_bc on the electrode's boxes, then a species step
    under the update mask (no update inside the electrode)."""
    topo, cases, lsf, ids = _rod_case_pair(nc, 0)
    out = []
    for c in cases:
        c.field_compute(0, check_residual=False)
        c.fluid.electrode_species_bc(golden.IVS["lsf"], IV["pos"], ids, neumann)
        r = [c.tree.get_cc(IV[s]) for s in ("e", "pos", "neg")]
        c.fluid.set_update_mask(golden.IVS["lsf"])
        lim = c.fluid.forward_euler(1e-12, 0, [0], [1.0], 1, False, store_flux=1)
        r += [c.tree.get_cc(IV[s] + 1) for s in ("e", "pos", "neg")]
        out.append((list(lim), r))
    assert out[0][0] == out[1][0]
    for q, (a, b) in enumerate(zip(out[0][1], out[1][1])):
        assert np.array_equal(a, b), (q, np.max(np.abs(a - b)))
    # inside the electrode: zeroed (Neumann: but for the layer next to the gas)
    inside = golden.interior(lsf) < 0
    e0 = golden.interior(out[0][1][0])
    assert inside.any() and np.any(e0[inside] == 0)
    assert np.any(e0[inside] != 0) == neumann
