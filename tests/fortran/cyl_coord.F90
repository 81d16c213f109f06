!> INTEGRATION.md's cylindrical snippet: a 2-D driver with coord_type = af_cyl
!> sets the coordinate type right after afh_tree_create, before any multigrid
!> or fluid object exists on the tree.
subroutine cyl_coord(desc, cylindrical, tree_h, ierr)
  use iso_c_binding
  use m_afivo_hip
  use m_afivo_hip_2d
  implicit none
  type(afh_tree_desc), intent(in) :: desc
  logical, intent(in)             :: cylindrical
  type(c_ptr), intent(out)        :: tree_h
  integer(c_int32_t), intent(out) :: ierr
  integer(c_int32_t)              :: coord

  ierr = afh_tree_create(desc, -1_c_int32_t, tree_h)
  if (ierr /= 0) return
  if (cylindrical) then
     ierr = afh_tree_set_coord(tree_h, AFH_COORD_CYL)
     if (ierr /= 0) return
  end if
  ierr = afh_tree_get_coord(tree_h, coord)
  if (ierr == 0 .and. cylindrical .and. coord /= AFH_COORD_CYL) ierr = -1
end subroutine cyl_coord
