!> ISO_C_BINDING interface of the source factor's entry point
!> (include/afivo_hip_srcfac.h), which libafivo_hip.so and libafivo_hip_2d.so
!> export outside the common ABI of m_afivo_hip. A driver with
!> fixes%source_factor = flux uses this module next to m_afivo_hip and calls
!> afh_fluid_set_source_factor after afh_fluid_create (INTEGRATION.md).
module m_afivo_hip_srcfac
  use iso_c_binding
  use m_afivo_hip
  implicit none
  public

  !> source_factor_none / source_factor_flux (m_streamer.f90:104-105)
  integer(c_int32_t), parameter :: AFH_SRCFAC_NONE = 0
  integer(c_int32_t), parameter :: AFH_SRCFAC_FLUX = 1

  interface
     !> ionization(n_reactions): nonzero for reaction_type ==
     !> ionization_reaction; min_electrons_per_cell <= 0: no threshold;
     !> i_srcfac: the cc variable the factor is stored in, 0: not stored
     function afh_fluid_set_source_factor(f, mode, ionization, min_electrons_per_cell, &
          i_srcfac) bind(C, name=afh_pfx//"fluid_set_source_factor")
       import
       type(c_ptr), value            :: f
       integer(c_int32_t), value     :: mode
       integer(c_int8_t), intent(in) :: ionization(*)
       real(c_double), value         :: min_electrons_per_cell
       integer(c_int32_t), value     :: i_srcfac
       integer(c_int32_t)            :: afh_fluid_set_source_factor
     end function afh_fluid_set_source_factor
  end interface

end module m_afivo_hip_srcfac
