/*
 * afivo_hip_rates.h -- the space integrals of the species step: per reaction
 * the number of events per second (chemical_rates_box, src/m_fluid.f90:665-699)
 * and the deposited power J.E (sum_global_JdotE, src/m_fluid.f90:702-731), the
 * ST_current_rates and ST_current_JdotE of the reference. Two entry points,
 * exported by libafivo_hip.so and libafivo_hip_2d.so and not part of the
 * common ABI of afivo_hip.h (the C oracle does not have them). A program that
 * reads the sums includes this header next to afivo_hip.h or afivo_hip_2d.h.
 */
#ifndef AFIVO_HIP_RATES_H
#define AFIVO_HIP_RATES_H

#include "afivo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: every density update with last_step != 0 (afh_flux_update_densities,
 * afh_fluid_forward_euler[_fold]) also sums, over all interior cells of every
 * leaf box that has at least one cell the update mask leaves on (masked cells
 * of such a box included; a wholly masked box and a box that is no leaf add
 * nothing, m_fluid.f90:332, 402-428):
 *   rates[r]  the final rate of reaction r -- the rate coefficient, scaled by
 *             the source factor where that is on (afivo_hip_srcfac.h), times
 *             the input densities -- times the cell volume: product(dr), or
 *             af_cyl_volume_cc on a cylindrical tree;
 *   jdote     fc_inner_product(electron flux, face field) (m_fluid.f90:259-280:
 *             0.5 times the sum of the low faces' products plus 0.5 times the
 *             sum of the high faces' products), times the cell volume, times
 *             UC_elec_charge. The flux is the one the update reads (after the
 *             consistent fluxes and the ion secondary emission); the face field
 *             is the stored one, or with afh_fluid_set_field_source the one the
 *             flux kernels form from the potential.
 * The sums are formed in a fixed order without floating-point atomics: two
 * steps from the same state give the same bits. A step with last_step == 0
 * leaves them untouched and launches what it launches without them.
 *
 * The call may come at any time after afh_fluid_create and holds from the next
 * step on; on = 0 restores the step without the sums exactly (the same kernels
 * as a fluid that never set them). The fused forward-Euler kernel of the 3-D
 * library forms no sums: with the sums on, a step with last_step != 0 takes the
 * flux, then update path; a step with last_step == 0 (Heun's first sub-step)
 * stays fused. The compiled reaction networks form no sums either: such a step
 * takes the generic reaction loop, which gives the same densities bitwise.
 *
 * AFH_ERR_ARG: null fluid. AFH_ERR_STATE: during a graph capture on the tree's
 * stream. AFH_ERR_UNSUPPORTED: a sharded tree (afh_tree_set_hook,
 * afh_dist_create); summing over ranks is not built, and a step of a fluid
 * with the sums on whose tree has been sharded since returns the same. */
int32_t afh_fluid_set_rate_sums(afh_fluid *f, int32_t on);

/* The sums of the most recent step with last_step != 0 since the sums were
 * switched on: rates[n_reactions] (afh_fluid_desc.reactions order) and *jdote.
 * Synchronises the tree's stream. AFH_ERR_ARG: a null pointer (rates may be
 * null without reactions). AFH_ERR_STATE: the sums are off, or no such step
 * has run since they were switched on. */
int32_t afh_fluid_fetch_rate_sums(afh_fluid *f, double *rates, double *jdote);

#ifdef __cplusplus
}
#endif
#endif
