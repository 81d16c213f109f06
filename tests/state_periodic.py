"""A deterministic species-step state on the periodic tree P (test
infrastructure, after tests/state2d.py).

``build_state`` gives every variable a forward-Euler species step reads --
the densities of both states, |E| and the face field -- on
periodic_numpy.tree_P as smooth closed forms of the cell and face centres,
periodic in x and y with P's periods, so that the ghost cells across the
seams hold the neighbours' values to rounding. scripts/make_periodic_cases.py
hands it to the reference's own forward_euler (oracle/_ref/replay_step with
test_3d.cfg and ``-periodic=T T F``) and commits the result
(tests/golden/replay_periodic.npz); tests/test_periodic_gpu.py runs the
device step on the same state and compares bit for bit.
"""
import numpy as np

import golden
import periodic_numpy as pn
from afh.driver import Case

CASE = "rtest_test_3d"
DT = 2e-12
STAGES = (  # (s_deriv, s_prev, w_prev, s_out): the two Heun sub-steps
    (0, [0], [1.0], 1),
    (1, [0, 1], [0.5, 0.5], 0),
)


def case_dict():
    """rtest_test_3d on P's domain, periodic (T, T, F)."""
    d = dict(golden.load(CASE))
    P = pn.tree_P()
    d["periodic"] = np.array([1, 1, 0])
    d["coarse_grid_size_value"] = np.array(P.coarse_grid_size)
    d["domain_len"] = np.array(P.domain - P.r_base)
    d["domain_origin"] = np.array(P.r_base)
    d["dt_max"] = np.array([1e-6])  # (so that the step's own limits are what dt_lim shows)
    return d


def cfg_args():
    """The same as settings of the reference (after test_3d.cfg)."""
    P = pn.tree_P()
    L = P.domain - P.r_base
    return ["-periodic=T T F", "-coarse_grid_size=%d %d %d" % tuple(P.coarse_grid_size),
            "-domain_len=%r %r %r" % tuple(float(x) for x in L), "-dt_max=1e-6"]


def _points(af, b, shift, n):
    idx = np.arange(n, dtype=float)
    ax = [af.r_min[b][d] + (idx - shift[d]) * af.dr[b][d] for d in range(3)]
    zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return xx, yy, zz


def build_state():
    """(Case, AfTree, {iv: cc array}, {ivf: fc array}) on tree_P."""
    c = Case(case_dict())
    af = pn.tree_P()
    L = af.domain - af.r_base
    nb, nc = af.highest_id, af.nc
    ng, nf = nc + 2, nc + 1
    n_cc, n_fc = len(c.sa("cc_names")), len(c.sa("fc_names"))
    (i_phi, i_e, i_pos, i_efld, i_rhs, i_tmp, _, f_flux, f_field, _) = c.ia("ivars")
    cc = {iv: np.zeros((nb, ng, ng, ng)) for iv in range(1, n_cc + 1)}
    fc = {iv: np.zeros((nb, 3, nf, nf, nf)) for iv in range(1, n_fc + 1)}
    E0, amp = -2.5e6, 0.3 * 2.5e6
    kx, ky, kz = 2 * np.pi / L[0], 2 * np.pi / L[1], np.pi / L[2]

    def grad_of(x, y, z):  # of phi = -E0 z + (amp / k) sin sin sin-like terms
        gx = amp * np.cos(kx * x) * np.sin(ky * y + 0.4) * np.sin(kz * z)
        gy = amp * np.sin(kx * x) * np.cos(ky * y + 0.4) * np.sin(kz * z) * (ky / kx)
        gz = -E0 + amp * np.sin(kx * x) * np.sin(ky * y + 0.4) * np.cos(kz * z) * (kz / kx)
        return gx, gy, gz

    def phi_of(x, y, z):
        return -E0 * z + amp / kx * np.sin(kx * x) * np.sin(ky * y + 0.4) * np.sin(kz * z)

    for b in range(1, nb + 1):
        if not af.in_use[b]:
            continue
        xx, yy, zz = _points(af, b, (0.5, 0.5, 0.5), ng)
        for k, iv in enumerate(c.ia("all_densities")):
            # a background and two periodic humps, the second across the seams
            a = 1e15 * (1 + 0.1 * k) + 5e18 / (1 + k) * np.exp(
                -(np.sin(0.5 * kx * (xx - 0.1 * L[0])) ** 2 + np.sin(0.5 * ky * (yy - 0.05 * L[1])) ** 2
                  + ((zz - 0.4 * L[2]) / (0.2 * L[2])) ** 2) / 0.15)
            a = a + 1e17 * (1 + np.cos(kx * xx + k)) * (1 + np.sin(ky * yy - k))
            cc[iv][b - 1] = a
            cc[iv + 1][b - 1] = a * (1 + 0.01 * np.sin(3 * kx * xx + 2 * ky * yy + k))
        cc[i_phi][b - 1] = phi_of(xx, yy, zz)
        gx, gy, gz = grad_of(xx, yy, zz)
        cc[i_efld][b - 1] = np.sqrt(gx * gx + gy * gy + gz * gz)
        # fc(1:nc+1, 1:nc+1, 1:nc+1, dim): dim's faces at r_min + (i - 1) dx
        for d in range(3):
            # and at the centres of cells 1..nc+1 in the other two directions
            shift = [-0.5, -0.5, -0.5]
            shift[d] = 0.0
            fx, fy, fz = _points(af, b, shift, nf)
            fc[f_field][b - 1, d] = -grad_of(fx, fy, fz)[d]
    return c, af, cc, fc


def write_record(path, af, cc, fc, dt, time, stage):
    """oracle/harness/replay_step.f90's record."""
    import struct
    s_deriv, s_prev, w_prev, s_out = stage
    hid = af.highest_id
    used = [b for b in range(1, hid + 1) if af.in_use[b]]
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", hid, len(cc), len(fc), af.nc))
        for b in range(1, hid + 1):
            ix = tuple(af.ix[b]) if af.in_use[b] else (0, 0, 0)
            f.write(struct.pack("<6i", af.parent[b], af.lvl[b], *ix, int(af.in_use[b])))
        f.write(struct.pack("<ddii", dt, time, s_deriv, len(s_prev)))
        f.write(struct.pack("<%di" % len(s_prev), *s_prev))
        f.write(struct.pack("<%dd" % len(w_prev), *w_prev))
        f.write(struct.pack("<i", s_out))
        for iv in range(1, len(cc) + 1):
            for b in used:
                f.write(np.ascontiguousarray(cc[iv][b - 1]).tobytes())
        for iv in range(1, len(fc) + 1):
            for b in used:
                f.write(np.ascontiguousarray(fc[iv][b - 1]).tobytes())
    return used


def replay_against_reference(lib, device, monkeypatch):
    """The species step of `lib` on tests/state_periodic.py's state against
    tests/golden/replay_periodic.npz (the reference's forward_euler with
    periodic = T T F, scripts/make_periodic_cases.py): densities on the
    leaves' interiors and dt_lim of both Heun stages, bitwise."""
    from afh.driver import Simulation
    # the stored face field, as the reference reads it
    monkeypatch.setenv("AFH_FACES_FROM_PHI", "0")
    ref = golden.load("replay_periodic")
    c, af, cc, fc = build_state()
    assert list(ref["leaves"]) == af.leaves()
    li = np.asarray(af.leaves()) - 1
    for k, (s_deriv, s_prev, w_prev, s_out) in enumerate(STAGES):
        sim = Simulation(lib, case_dict(), device=device)
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
            mine = sim.tree.get_cc(iv + s_out)[li][:, 1:-1, 1:-1, 1:-1]
            assert np.array_equal(mine, ref["dens_%d" % (k + 1)][q]), (k, sim.cc_names[iv - 1])
        sim.tree.close()
