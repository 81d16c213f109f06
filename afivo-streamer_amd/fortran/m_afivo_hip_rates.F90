!> ISO_C_BINDING interface of the rate and J.E sums' entry points
!> (include/afivo_hip_rates.h), which libafivo_hip.so and libafivo_hip_2d.so
!> export outside the common ABI of m_afivo_hip. A driver that keeps
!> ST_global_rates and ST_global_JdotE uses this module next to m_afivo_hip:
!> afh_fluid_set_rate_sums(f, 1) after afh_fluid_create, and after every
!> accepted step afh_fluid_fetch_rate_sums for ST_current_rates and
!> ST_current_JdotE (src/streamer.f90:290-294).
module m_afivo_hip_rates
  use iso_c_binding
  use m_afivo_hip
  implicit none
  public

  interface
     !> on /= 0: every update with last_step also sums the rates and J.E
     function afh_fluid_set_rate_sums(f, on) bind(C, name=afh_pfx//"fluid_set_rate_sums")
       import
       type(c_ptr), value        :: f
       integer(c_int32_t), value :: on
       integer(c_int32_t)        :: afh_fluid_set_rate_sums
     end function afh_fluid_set_rate_sums

     !> rates(n_reactions) and J.E of the most recent step with last_step
     function afh_fluid_fetch_rate_sums(f, rates, jdote) &
          bind(C, name=afh_pfx//"fluid_fetch_rate_sums")
       import
       type(c_ptr), value          :: f
       real(c_double), intent(out) :: rates(*)
       real(c_double), intent(out) :: jdote
       integer(c_int32_t)          :: afh_fluid_fetch_rate_sums
     end function afh_fluid_fetch_rate_sums
  end interface

end module m_afivo_hip_rates
