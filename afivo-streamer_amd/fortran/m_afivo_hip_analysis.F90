!> ISO_C_BINDING interface of the reductions behind output_log and
!> output_fld_maxima (include/afivo_hip_analysis.h), which libafivo_hip.so and
!> libafivo_hip_2d.so export outside the common ABI of m_afivo_hip. They take
!> the place of af_tree_max_fc / af_tree_min_fc, analysis_zmin_zmax_threshold,
!> analysis_max_var_region and analysis_get_maxima (src/m_output.f90:532-560,
!> 878) in a driver whose boxes live on the device. A location is an af_loc_t
!> flattened to loc(4) = (id, i, j, k), k = 0 in 2-D; r0 and r1 have three
!> entries, of which the 2-D library reads two.
module m_afivo_hip_analysis
  use iso_c_binding
  use m_afivo_hip
  implicit none
  public

  interface
     !> af_tree_max_fc / af_tree_min_fc (op = AFH_RED_MAX / AFH_RED_MIN) of
     !> fc(.., dim, ivf), the upper-boundary faces included
     function afh_tree_reduce_fc(t, ivf, dim, op, out, loc) &
          bind(C, name=afh_pfx//"tree_reduce_fc")
       import
       type(c_ptr), value              :: t
       integer(c_int32_t), value       :: ivf, dim, op
       real(c_double), intent(out)     :: out
       integer(c_int32_t), intent(out) :: loc(4)
       integer(c_int32_t)              :: afh_tree_reduce_fc
     end function afh_tree_reduce_fc

     !> analysis_zmin_zmax_threshold, as written (a box's zmax entry is that
     !> of its first plane above the threshold)
     function afh_tree_zminmax_threshold(t, iv, threshold, limits, out) &
          bind(C, name=afh_pfx//"tree_zminmax_threshold")
       import
       type(c_ptr), value          :: t
       integer(c_int32_t), value   :: iv
       real(c_double), value       :: threshold
       real(c_double), intent(in)  :: limits(2)
       real(c_double), intent(out) :: out(2)
       integer(c_int32_t)          :: afh_tree_zminmax_threshold
     end function afh_tree_zminmax_threshold

     !> analysis_max_var_region
     function afh_tree_max_region(t, iv, r0, r1, out, loc) &
          bind(C, name=afh_pfx//"tree_max_region")
       import
       type(c_ptr), value              :: t
       integer(c_int32_t), value       :: iv
       real(c_double), intent(in)      :: r0(3), r1(3)
       real(c_double), intent(out)     :: out
       integer(c_int32_t), intent(out) :: loc(4)
       integer(c_int32_t)              :: afh_tree_max_region
     end function afh_tree_max_region

     !> analysis_get_maxima; coord_val(NDIM+1, n_max), filled in a fixed order
     !> (leaves in loop order, cells in array order)
     function afh_tree_local_maxima(t, iv, threshold, n_max, coord_val, n_found) &
          bind(C, name=afh_pfx//"tree_local_maxima")
       import
       type(c_ptr), value              :: t
       integer(c_int32_t), value       :: iv, n_max
       real(c_double), value           :: threshold
       real(c_double), intent(inout)   :: coord_val(*)
       integer(c_int32_t), intent(out) :: n_found
       integer(c_int32_t)              :: afh_tree_local_maxima
     end function afh_tree_local_maxima
  end interface

end module m_afivo_hip_analysis
