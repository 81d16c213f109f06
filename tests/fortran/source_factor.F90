!> INTEGRATION.md's source-factor snippet: after afh_fluid_create a driver
!> with fixes%source_factor = flux hands the library the ionization flags of
!> its reaction list (reaction_type == ionization_reaction), the electron
!> threshold and the variable of write_source_factor (i_srcfac, 0 when the
!> factor is not written).
subroutine source_factor(fluid_h, n_reactions, reaction_type, min_electrons, i_srcfac, ierr)
  use iso_c_binding
  use m_afivo_hip
  use m_afivo_hip_srcfac
  implicit none
  type(c_ptr), intent(in)         :: fluid_h
  integer, intent(in)             :: n_reactions
  integer, intent(in)             :: reaction_type(n_reactions)
  real(c_double), intent(in)      :: min_electrons
  integer(c_int32_t), intent(in)  :: i_srcfac
  integer(c_int32_t), intent(out) :: ierr
  integer, parameter              :: ionization_reaction = 1
  integer(c_int8_t)               :: flags(n_reactions)

  flags = 0
  where (reaction_type == ionization_reaction) flags = 1
  ierr = afh_fluid_set_source_factor(fluid_h, AFH_SRCFAC_FLUX, flags, min_electrons, &
       max(i_srcfac, 0_c_int32_t))
end subroutine source_factor
