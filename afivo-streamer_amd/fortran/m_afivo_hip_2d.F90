!> ISO_C_BINDING interfaces of the entry points only libafivo_hip_2d.so has
!> (include/afivo_hip_2d_cyl.h): the tree's coordinate type. A 2-D driver
!> binds m_afivo_hip against the 2-D library and uses this module next to it;
!> with coord_type = af_cyl it calls afh_tree_set_coord right after
!> afh_tree_create (INTEGRATION.md).
module m_afivo_hip_2d
  use iso_c_binding
  use m_afivo_hip
  implicit none
  public

  !> afivo's af_xyz / af_cyl (m_af_types.f90), the values of tree%coord_t
  integer(c_int32_t), parameter :: AFH_COORD_XYZ = 1
  integer(c_int32_t), parameter :: AFH_COORD_CYL = 2

  interface
     !> Legal between afh_tree_create and the first afh_mg_create or
     !> afh_fluid_create on the tree (AFH_ERR_STATE afterwards)
     function afh_tree_set_coord(t, coord) bind(C, name=afh_pfx//"tree_set_coord")
       import
       type(c_ptr), value        :: t
       integer(c_int32_t), value :: coord
       integer(c_int32_t)        :: afh_tree_set_coord
     end function afh_tree_set_coord

     function afh_tree_get_coord(t, coord) bind(C, name=afh_pfx//"tree_get_coord")
       import
       type(c_ptr), value              :: t
       integer(c_int32_t), intent(out) :: coord
       integer(c_int32_t)              :: afh_tree_get_coord
     end function afh_tree_get_coord
  end interface

end module m_afivo_hip_2d
