!> INTEGRATION.md's simulation-log snippet: the device reductions output_log
!> and output_fld_maxima need (src/m_output.f90:532-560, 878) through
!> m_afivo_hip_analysis, here for a 3-D tree handle.
subroutine simulation_log(tree_h, i_electron, i_electric_fld, electric_fld, &
     threshold, domain_origin, domain_len, max_Er, min_Er, ne_zminmax, &
     max_field_tip, loc_tip, coord_val, n_found, ierr)
  use iso_c_binding
  use m_afivo_hip
  use m_afivo_hip_analysis
  implicit none
  integer, parameter              :: n_max = 1000
  type(c_ptr), intent(in)         :: tree_h
  integer(c_int32_t), intent(in)  :: i_electron, i_electric_fld, electric_fld
  real(c_double), intent(in)      :: threshold, domain_origin(3), domain_len(3)
  real(c_double), intent(out)     :: max_Er, min_Er, ne_zminmax(2), max_field_tip
  integer(c_int32_t), intent(out) :: loc_tip(4)
  real(c_double), intent(inout)   :: coord_val(4, n_max)
  integer(c_int32_t), intent(out) :: n_found, ierr
  integer(c_int32_t)              :: loc_Er(4), loc_tmp(4)
  real(c_double)                  :: r0(3), r1(3)

  ierr = afh_tree_reduce_fc(tree_h, electric_fld, 1_c_int32_t, AFH_RED_MAX, max_Er, loc_Er)
  if (ierr /= 0) return
  ierr = afh_tree_reduce_fc(tree_h, electric_fld, 1_c_int32_t, AFH_RED_MIN, min_Er, loc_tmp)
  if (ierr /= 0) return
  ierr = afh_tree_zminmax_threshold(tree_h, i_electron, threshold, &
       [domain_len(3), 0.0_c_double], ne_zminmax)
  if (ierr /= 0) return

  r0 = domain_origin
  r1 = domain_origin + domain_len
  if (ne_zminmax(1) - domain_origin(3) < &
       domain_origin(3) + domain_len(3) - ne_zminmax(2)) then
     r0(3) = ne_zminmax(2) - 0.02_c_double * domain_len(3)
     r1(3) = ne_zminmax(2) + 0.02_c_double * domain_len(3)
  else
     r0(3) = ne_zminmax(1) - 0.02_c_double * domain_len(3)
     r1(3) = ne_zminmax(1) + 0.02_c_double * domain_len(3)
  end if
  ierr = afh_tree_max_region(tree_h, i_electric_fld, r0, r1, max_field_tip, loc_tip)
  if (ierr /= 0) return

  ierr = afh_gc_tree(tree_h, i_electric_fld, 1_c_int32_t)
  if (ierr /= 0) return
  ierr = afh_tree_local_maxima(tree_h, i_electric_fld, threshold, &
       int(n_max, c_int32_t), coord_val, n_found)
end subroutine simulation_log
