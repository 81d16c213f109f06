#!/usr/bin/env python3
"""ORACLE TEST INFRASTRUCTURE -- pack the limiter and boundary-type variants
(build container only).

Runs oracle/_ref/variants_gen and oracle/_ref/2d/variants_gen (the reference's
afivo numerics driven by oracle/harness/variants_gen.f90) and packs their raw
dumps into tests/golden/variants3d*.npz and variants2d*.npz. Usage:

    make -C oracle ref && python3 oracle/make_variants.py

Beside the topology and table keys of make_golden.py (arrays [box][k][j][i],
face arrays [box][dim][k][j][i]):
  in_e, in_efld           the input density (ghost cells included) and |E|
  in_fc_field             the input face field
  flux_<L>, flux_<L>_dt   face flux and both limits with flux limiter L = 1..7
  pflux_<L>, pflux_<L>_dt the Koren flux with prolongation limiter L
  gc_bc_types (4, 2 ndim) int32, gc_bc_vals    the four rotations of the types
  gc_<R>_<M>              the density after af_gc_tree with corners, rotation
                          R, M = 1 af_gc_interp, 2 af_gc_interp_lim
  bflux_bc_types (3, 2 ndim), bflux_bc_vals    Dirichlet, Neumann, copy
  bflux_<A>, bflux_<A>_dt the Koren flux under assignment A = 1..3
Only the arrays a variant changes are stored. The packer asserts the tree
conditions the tests rely on (physical faces, coarse-fine faces in every
direction, same-level leaf neighbours).
"""
import os
import subprocess
import sys

import numpy as np

from make_golden import HERE, TD_FILE, read_tables, read_topology, save_parts

N_LIM = 7


def check_tree(topo, ndim):
    """Every physical face of the domain touched by a leaf; every face
    direction with a coarse-fine face whose fine side is on a level >= 2; a
    leaf with a same-level leaf neighbour."""
    nlvl = int(topo["highest_lvl"])
    leaves = np.concatenate([topo["lvl_leaves_%d" % l] for l in range(1, nlvl + 1)])
    nbs, lvl, ch = topo["meta_neighbors"], topo["meta_lvl"], topo["meta_children"]
    is_leaf = np.zeros(len(lvl) + 1, bool)
    is_leaf[leaves] = True
    assert nlvl == 3 and np.all(ch[leaves - 1] <= 0)
    phys, cf, same = set(), set(), False
    for b in leaves:
        for nb in range(2 * ndim):
            n = nbs[b - 1, nb]
            if n < 0:
                phys.add(nb)
            elif n == 0:
                assert lvl[b - 1] >= 2
                cf.add(nb)
            elif is_leaf[n]:
                same = True
    assert phys == set(range(2 * ndim)), phys
    assert cf == set(range(2 * ndim)), cf
    assert same


def pack(ndim, raw):
    topo = read_topology(os.path.join(raw, "topology.bin"), ndim)
    check_tree(topo, ndim)
    out = dict(topo)
    out.update(read_tables(os.path.join(raw, "tables.bin")))
    nb, nc = int(topo["n_boxes"]), int(topo["nc"])
    cc_shape = (nb,) + (nc + 2,) * ndim
    fc_shape = (nb, ndim) + (nc + 1,) * ndim
    nfc = int(np.prod(fc_shape))

    def cc(name):
        return np.fromfile(os.path.join(raw, name + ".bin")).reshape(cc_shape)

    def fc(name, with_dt=True):
        a = np.fromfile(os.path.join(raw, name + ".bin"))
        assert a.size == nfc + (2 if with_dt else 0)
        return a[:nfc].reshape(fc_shape), a[nfc:]

    out["in_e"], out["in_efld"] = cc("in_e"), cc("in_efld")
    out["in_fc_field"] = fc("in_field", False)[0]
    for kind, n in (("flux", N_LIM), ("pflux", N_LIM), ("bflux", 3)):
        for q in range(1, n + 1):
            key = "%s_%d" % (kind, q)
            out[key], out[key + "_dt"] = fc(key)
    bc = open(os.path.join(raw, "bc.bin"), "rb").read()
    rec = 2 * ndim * 12
    assert len(bc) == 7 * rec
    ty = np.array([np.frombuffer(bc, np.int32, 2 * ndim, q * rec) for q in range(7)])
    va = np.array([np.frombuffer(bc, np.float64, 2 * ndim, q * rec + 8 * ndim)
                   for q in range(7)])
    out["gc_bc_types"], out["gc_bc_vals"] = ty[:4], va[:4]
    out["bflux_bc_types"], out["bflux_bc_vals"] = ty[4:], va[4:]
    # every face sees every type, with a value that is not zero
    assert all(sorted(ty[:4, f]) == [-13, -12, -11, -10] for f in range(2 * ndim))
    assert np.all(va != 0)
    for r in range(4):
        for m in (1, 2):
            out["gc_%d_%d" % (r, m)] = cc("gc_%d_%d" % (r, m))
    return save_parts("variants%dd" % ndim, out)


def main():
    for ndim, sub in ((3, ""), (2, "2d")):
        gen = os.path.join(HERE, "_ref", sub, "variants_gen")
        if not os.path.exists(gen):
            sys.exit("build the harness first: make -C oracle ref")
        raw = os.path.join("/tmp", "variants_raw", "%dd" % ndim)
        os.makedirs(raw, exist_ok=True)
        for f in os.listdir(raw):
            os.remove(os.path.join(raw, f))
        subprocess.run([gen, TD_FILE, raw], check=True, stdout=subprocess.DEVNULL)
        for dst in pack(ndim, raw):
            print("%dd -> %s (%.0f kB)" % (ndim, dst, os.path.getsize(dst) / 1e3))


if __name__ == "__main__":
    main()
