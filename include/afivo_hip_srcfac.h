/*
 * afivo_hip_srcfac.h -- the flux-based source factor of the species step
 * (fixes%source_factor = flux of the reference, src/m_streamer.f90:420-440,
 * src/m_fluid.f90:368-397 with compute_source_factor at 525-583). One entry
 * point, exported by libafivo_hip.so and libafivo_hip_2d.so and not part of
 * the common ABI of afivo_hip.h (the C oracle does not have it). A program
 * that sets the factor includes this header next to afivo_hip.h or
 * afivo_hip_2d.h.
 */
#ifndef AFIVO_HIP_SRCFAC_H
#define AFIVO_HIP_SRCFAC_H

#include "afivo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AFH_SRCFAC_NONE 0
#define AFH_SRCFAC_FLUX 1

/* With AFH_SRCFAC_FLUX the density update (afh_flux_update_densities,
 * afh_fluid_forward_euler[_fold]) scales the rate coefficient of every
 * flagged reaction of a cell by
 *     s = (fl + 1e-9) / (1e-9 + n mu |E|),  min(1, s), max(0, s)
 * before the product with the input densities, in the reference's operation
 * order:
 *   n   max(n_e(s_deriv), 0);
 *   mu  LT_get_col(transport table, mobility column, field in Td) times 1/N
 *       (the constant 1 / gas_number_density, or 1 / N(cell) with a variable
 *       gas density);
 *   fl  0.5 NORM2 of the sums of the electron flux over the cell's two faces
 *       per dimension, the flux as the update reads it (after the consistent
 *       fluxes and the ion secondary emission), NORM2 evaluated as the
 *       reference build's Fortran runtime does (scaled by the largest
 *       component).
 * min_electrons_per_cell > 0: s = 0 where n min(dr)**3 is below it (the
 * exponent is 3 in 2-D too, and no radius enters on a cylindrical tree, as in
 * the reference). The chemistry time-step limit of the last step sees the
 * scaled derivatives; the photoionization term is not scaled.
 *
 * ionization: n_reactions flags (afh_fluid_desc.reactions order), nonzero for
 * an ionization_reaction (m_chemistry.f90:14); copied by the call.
 * i_srcfac > 0: s is stored in that cc variable on every interior cell of
 * every leaf box that has at least one cell the update mask leaves on (masked
 * cells of such a box included; a wholly masked box is not written).
 *
 * The call may come at any time after afh_fluid_create and holds from the
 * next step on; AFH_SRCFAC_NONE restores the step without the factor exactly
 * (the same kernels as a fluid that never set it). The fused forward-Euler
 * kernel of the 3-D library has no factor: with the factor on the step takes
 * the flux, then update path.
 *
 * AFH_ERR_ARG: null fluid, unknown mode, AFH_SRCFAC_FLUX without flags,
 * i_srcfac outside 0..n_var_cell or equal to a variable the step reads or
 * writes (a species variable, i_efld, i_photo, the gas density, the update
 * mask's level set, the rhs output; the further states of the species are
 * checked against the states of each step, which then returns AFH_ERR_ARG).
 * AFH_ERR_STATE: during a graph capture on the tree's stream. */
int32_t afh_fluid_set_source_factor(afh_fluid *f, int32_t mode, const uint8_t *ionization,
                                    double min_electrons_per_cell, int32_t i_srcfac);

#ifdef __cplusplus
}
#endif
#endif
