"""A deterministic species-step state on the periodic 2-D tree P (test
infrastructure, after tests/state_periodic.py and tests/state2d.py).

``build_state`` gives every variable a forward-Euler species step reads --
the densities of both states, |E| and the face field -- on
periodic2d_numpy.tree_P as smooth closed forms of the cell and face centres,
periodic in x with P's period, so that the ghost cells across the seam hold
the neighbours' values to rounding. scripts/make_periodic2d_cases.py hands it
to the reference's own forward_euler (oracle/_ref/2d/replay_step with
test_2d.cfg and ``-periodic=T F``) and commits the result
(tests/golden/replay_periodic2d.npz); tests/test_periodic2d_gpu.py runs the
device step on the same state and compares bit for bit.
"""
import numpy as np

import golden
import periodic2d_numpy as p2
from afh.driver import Case
from state2d import STAGES, write_record  # noqa: F401  (the record is state2d's)

CASE = "rtest_test_2d"
DT = 2e-12


def case_dict():
    """rtest_test_2d on P's domain, periodic (T, F)."""
    d = dict(golden.load(CASE))
    P = p2.tree_P()
    d["periodic"] = np.array([1, 0])
    d["coarse_grid_size_value"] = np.array(P.coarse_grid_size)
    d["domain_len"] = np.array(P.domain - P.r_base)
    d["domain_origin"] = np.array(P.r_base)
    d["dt_max"] = np.array([1e-6])  # (so that the step's own limits are what dt_lim shows)
    return d


def cfg_args():
    """The same as settings of the reference (after test_2d.cfg)."""
    P = p2.tree_P()
    L = P.domain - P.r_base
    return ["-periodic=T F", "-coarse_grid_size=%d %d" % tuple(P.coarse_grid_size),
            "-domain_len=%r %r" % tuple(float(x) for x in L), "-dt_max=1e-6"]


def _points(af, b, shift, n):
    idx = np.arange(n, dtype=float)
    ax = [af.r_min[b][d] + (idx - shift[d]) * af.dr[b][d] for d in range(2)]
    yy, xx = np.meshgrid(ax[1], ax[0], indexing="ij")
    return xx, yy


def build_state():
    """(Case, AfTree, {iv: cc array}, {ivf: fc array}) on tree_P."""
    c = Case(case_dict())
    af = p2.tree_P()
    assert np.all(af.r_base == 0.0)  # (the reference's domain starts at the origin)
    L = af.domain - af.r_base
    nb, nc = af.highest_id, af.nc
    ng, nf = nc + 2, nc + 1
    n_cc, n_fc = len(c.sa("cc_names")), len(c.sa("fc_names"))
    (i_phi, i_e, i_pos, i_efld, i_rhs, i_tmp, _, f_flux, f_field, _) = c.ia("ivars")
    cc = {iv: np.zeros((nb, ng, ng)) for iv in range(1, n_cc + 1)}
    fc = {iv: np.zeros((nb, 2, nf, nf)) for iv in range(1, n_fc + 1)}
    E0, amp = -2.5e6, 0.3 * 2.5e6
    kx, ky = 2 * np.pi / L[0], np.pi / L[1]

    def grad_of(x, y):  # of phi = -E0 y + (amp / kx) sin(kx x + 0.4) sin(ky y)
        gx = amp * np.cos(kx * x + 0.4) * np.sin(ky * y)
        gy = -E0 + amp * np.sin(kx * x + 0.4) * np.cos(ky * y) * (ky / kx)
        return gx, gy

    def phi_of(x, y):
        return -E0 * y + amp / kx * np.sin(kx * x + 0.4) * np.sin(ky * y)

    for b in p2.used(af):
        xx, yy = _points(af, b, (0.5, 0.5), ng)
        for k, iv in enumerate(c.ia("all_densities")):
            # a background and two periodic humps, the second across the seam
            a = 1e15 * (1 + 0.1 * k) + 5e18 / (1 + k) * np.exp(
                -(np.sin(0.5 * kx * (xx - 0.1 * L[0])) ** 2
                  + ((yy - 0.4 * L[1]) / (0.2 * L[1])) ** 2) / 0.15)
            a = a + 1e17 * (1 + np.cos(kx * xx + k)) * (1 + np.sin(ky * yy - k) ** 2)
            cc[iv][b - 1] = a
            cc[iv + 1][b - 1] = a * (1 + 0.01 * np.sin(3 * kx * xx + 2 * ky * yy + k))
        cc[i_phi][b - 1] = phi_of(xx, yy)
        gx, gy = grad_of(xx, yy)
        cc[i_efld][b - 1] = np.sqrt(gx * gx + gy * gy)
        # fc(1:nc+1, 1:nc+1, dim): dim's faces at r_min + (i - 1) dx, at the
        # centres of cells 1..nc+1 in the other direction
        for d in range(2):
            shift = [-0.5, -0.5]
            shift[d] = 0.0
            fx, fy = _points(af, b, shift, nf)
            fc[f_field][b - 1, d] = -grad_of(fx, fy)[d]
    return c, af, cc, fc


def replay_against_reference(lib, device):
    """The species step of `lib` on this state against
    tests/golden/replay_periodic2d.npz (the reference's forward_euler with
    periodic = T F, scripts/make_periodic2d_cases.py): densities on the
    leaves' interiors and dt_lim of both Heun stages, bitwise."""
    from afh import capi
    from afh.driver import Simulation
    ref = golden.load("replay_periodic2d")
    c, af, cc, fc = build_state()
    assert list(ref["leaves"]) == af.leaves()
    li = np.asarray(af.leaves()) - 1
    for k, (s_deriv, s_prev, w_prev, s_out) in enumerate(STAGES):
        sim = Simulation(lib, case_dict(), device=device, coarse_mode=capi.COARSE_PFMG,
                         coarse_cycles=50, coarse_tol=1e-6)
        sim.af = af
        sim._bind(sim._create_tree())
        assert not sim.faces_from_phi
        for iv, a in cc.items():
            sim.tree.put_cc(iv, a)
        for ivf, a in fc.items():
            sim.tree.put_fc(ivf, a)
        dt = DT * (1.0 if k == 0 else 0.5)
        lim = sim.fluid.forward_euler(dt, s_deriv, s_prev, w_prev, s_out, True)
        ours = min(sim.dt_max, min(lim[0] * sim.cfl, lim[1], lim[2], lim[3]))
        assert ours == ref["dt_lim_%d" % (k + 1)][0], (k, ours)
        assert ours < sim.dt_max
        for q, iv in enumerate(sim.densities):
            mine = sim.tree.get_cc(iv + s_out)[li][:, 1:-1, 1:-1]
            assert np.array_equal(mine, ref["dens_%d" % (k + 1)][q]), (k, sim.cc_names[iv - 1])
        sim.tree.close()
