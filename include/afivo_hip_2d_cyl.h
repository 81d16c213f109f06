/*
 * afivo_hip_2d_cyl.h -- the entry points of libafivo_hip_2d.so that are not
 * part of the common ABI of afivo_hip.h: the tree's coordinate type. Included
 * by afivo_hip_2d.h (which itself lists the subset of the common ABI the 2-D
 * library exports); a 2-D program includes that header.
 */
#ifndef AFIVO_HIP_2D_CYL_H
#define AFIVO_HIP_2D_CYL_H

#include "afivo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tree's coordinate type: afivo's af_xyz / af_cyl, the values a .dat file
 * stores as coord_t. A tree is created Cartesian. */
#define AFH_COORD_XYZ 1
#define AFH_COORD_CYL 2

/* Cylindrical (axisymmetric) coordinates, 2-D only. afh_tree_set_coord is
 * legal between afh_tree_create and the first afh_mg_create or
 * afh_fluid_create on the tree (AFH_ERR_STATE afterwards); AFH_ERR_ARG for an
 * unknown value and, for AFH_COORD_CYL, for a tree periodic in r
 * (periodic[0] != 0) or starting left of the axis (r_base[0] < 0). The tree
 * afh_tree_regrid returns inherits the type. On a cylindrical tree:
 *   - the multigrid operator is the Laplacian with cylindrical_gradient
 *     (smoother, residual, FAS right-hand side, the PFMG level-1 operator);
 *     phi is restricted without geometry, everything else -- afh_restrict_tree
 *     included -- with af_cyl_child_weights;
 *   - the density update multiplies the r-fluxes by af_cyl_flux_factors and
 *     the consistent fluxes weight the fine z-faces;
 *   - afh_tree_sum_cc weights by 2 pi r (afh_tree_reduce_loc and the maxima
 *     are unchanged);
 *   - afh_mg_create with AFH_COARSE_DIRECT returns AFH_ERR_UNSUPPORTED: the
 *     cosine / sine basis of the direct solve does not diagonalise the
 *     operator in r. Use AFH_COARSE_PFMG.
 * Ghost cells, the gradient, field_set_rhs, the flux computation, the
 * prolongations and the refinement flags are the same in both types. */
int32_t afh_tree_set_coord(afh_tree *t, int32_t coord);
int32_t afh_tree_get_coord(afh_tree *t, int32_t *coord);

#ifdef __cplusplus
}
#endif
#endif
