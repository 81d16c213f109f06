/*
 * afivo_hip_analysis.h -- the tree reductions behind the simulation log
 * (output_log, src/m_output.f90:496-670) and the list of field maxima
 * (output_fld_maxima, src/m_output.f90:869-912): a face variable's extremum
 * with its location, the extent of a variable above a threshold along the last
 * dimension, the maximum over the boxes that touch a region, and the local
 * maxima. Four entry points, exported by libafivo_hip.so and
 * libafivo_hip_2d.so and not part of the common ABI of afivo_hip.h (the C
 * oracle does not have them). A program that uses them includes this header
 * next to afivo_hip.h or afivo_hip_2d.h.
 *
 * Common to the four:
 *  - they read the interiors of the leaf boxes (the maxima also one ghost
 *    layer) and change nothing on the tree;
 *  - a location is an af_loc_t as afh_tree_reduce_loc returns it: loc[4] =
 *    (box id, i, j, k), 1-based, k = 0 in the 2-D library; where there is no
 *    location the id and the indices are -1 (k stays 0 in 2-D); loc may be
 *    NULL;
 *  - ties go to the first position (first index fastest) of the first box in
 *    the reference's loop order (levels ascending, then lvls(l)%leaves order),
 *    the rule of afh_tree_reduce_loc;
 *  - each is formed on the device by selections only -- per-leaf results in
 *    the leaf-list order, then one fold, no floating-point atomics: two calls
 *    on the same data give the same bits and the same locations -- and costs
 *    one host synchronisation;
 *  - none carries geometry: a cylindrical and a periodic tree are served as
 *    any other;
 *  - AFH_ERR_ARG: a null tree or output, an unknown variable, dimension or
 *    operation; AFH_ERR_UNSUPPORTED ("sharded"): a sharded tree
 *    (afh_tree_set_hook, afh_dist_create) -- the fold over ranks is not built.
 */
#ifndef AFIVO_HIP_ANALYSIS_H
#define AFIVO_HIP_ANALYSIS_H

#include "afivo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* af_tree_max_fc / af_tree_min_fc with box_max_fc / box_min_fc
 * (m_af_utils.f90:803-952): op = AFH_RED_MAX or AFH_RED_MIN of face variable
 * ivf, direction dim (1-based), over fc(1:nc, .., dim, ivf) with the index
 * along dim running 1:nc+1 -- the faces on a box's upper boundary are in the
 * range, so loc may hold nc+1 along dim. The layout is the one afh_fc_get
 * documents. The initial value is -huge(1d0)/10 (max) or +huge(1d0)/10 (min):
 * without a leaf *out is that value and there is no location. */
int32_t afh_tree_reduce_fc(afh_tree *t, int32_t ivf, int32_t dim, int32_t op, double *out,
                           int32_t *loc);

/* analysis_zmin_zmax_threshold (src/m_analysis.f90:81-149), as written: per
 * leaf, plane n along the last dimension is "above" when the maximum of
 * cc(1:nc, [1:nc,] n, iv) is > threshold (a value equal to it is not). A leaf
 * contributes the cell-centre coordinate r_min + (n - 0.5) dr of its FIRST
 * plane above for both entries: the reference sets ix(NDIM) = i in its zmin
 * and in its zmax branch (lines 127-137), so a leaf's zmax is that of its
 * first plane above, not of its last. This is kept, for logs that equal the
 * reference's. A leaf with no plane above contributes (1e100, -1e100).
 * out[0] = min(limits[0], the leaves' first entries), out[1] = max(limits[1],
 * the leaves' second entries). */
int32_t afh_tree_zminmax_threshold(afh_tree *t, int32_t iv, double threshold,
                                   const double *limits, double *out);

/* analysis_max_var_region (src/m_analysis.f90:153-186): the maximum of cc(iv)
 * over the leaves that touch the box r0 .. r1, and where it is. A leaf takes
 * part unless any(r_min > r1) or any(r_min + nc * dr < r0) -- a leaf that only
 * touches the region's edge takes part -- and then with its whole interior.
 * The initial value is -1e100: with no leaf taking part *out = -1e100 and
 * there is no location. r0 and r1 have 3 entries; the 2-D library reads the
 * first two. */
int32_t afh_tree_max_region(afh_tree *t, int32_t iv, const double *r0, const double *r1,
                            double *out, int32_t *loc);

/* analysis_get_maxima (src/m_analysis.f90:23-78): a leaf cell is a maximum
 * when cc(iv) > threshold there, cc(iv) >= each of its 2 NDIM face neighbours
 * and cc(iv) > at least one of them. The neighbours of a cell on the box's
 * boundary are the ghost cells as they stand: the caller fills them first
 * (afh_gc_tree). coord_val is (NDIM + 1) x n_max, first index fastest: the
 * cell-centre coordinates r_min + (ix - 0.5) dr, then the value. *n_found is
 * the number of maxima on the tree, which may exceed n_max; the first n_max
 * are stored and the rest of coord_val is left as it was. The reference fills
 * its list in the order its threads arrive; here the order is fixed: leaves
 * in loop order, cells in array order within a leaf (a count per leaf, an
 * exclusive scan, then the write -- no atomic cursor). n_max >= 0; coord_val
 * may be NULL when n_max is 0. */
int32_t afh_tree_local_maxima(afh_tree *t, int32_t iv, double threshold, int32_t n_max,
                              double *coord_val, int32_t *n_found);

#ifdef __cplusplus
}
#endif
#endif
