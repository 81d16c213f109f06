!> ORACLE TEST INFRASTRUCTURE -- limiter and boundary-type variants (build
!> container only).
!>
!> Drives the afivo numerics compiled from the reference sources (NDIM = 3 or
!> 2, oracle/Makefile) through the options no golden chain reaches, on one
!> small AMR tree with a lattice-valued input, and dumps the results as raw
!> binary for oracle/make_variants.py:
!>
!>   flux_<L>   flux_upwind_tree (hx_physics callbacks) with flux limiter
!>              L = 1..7 and the default prolongation limiter
!>   pflux_<L>  the same with Koren and prolongation limiter L = 1..7 on the
!>              species (gc2_prolong_rb)
!>   gc_<R>_<M> af_gc_tree with corners under rotation R = 0..3 of the four
!>              boundary types over the faces, M = 1 af_gc_interp, 2
!>              af_gc_interp_lim
!>   bflux_<A>  the Koren flux with every face Dirichlet (A = 1), Neumann (2)
!>              or dirichlet_copy (3), non-zero values: bc_to_gc2, with the c0
!>              of m_af_ghostcell.f90:361 on the high-y face in 3-D
!>
!> Tree: boxes of 4^NDIM cells; level 1 (one box in 3-D, 4 x 4 in 2-D)
!> refined with af_adjust_refinement into its children, of which the two at
!> opposite corners of the domain are refined again: 25 boxes in 3-D, 88 in
!> 2-D, on three levels, a refinement boundary with the fine side on level 3
!> in every face direction, every physical face touched by leaves of levels 2
!> and 3, same-level neighbours on both. (2-D has more boxes because a line
!> of a box holds few slope pairs: the rarest limiter branch, the tie of the
!> generalised minmod limiter with theta = 4/3, takes one pair in 400.)
!>
!> Input: densities k 2^50 with k = 0..8 from a linear congruential generator
!> (differences of neighbours are small integers times a power of two, so the
!> limiters' arguments land on every equality of their branches), |E| =
!> (1 + k) 2^20, a face field (k - 4) 2^18 of both signs and zero. The cell
!> size is a power of two, and so are the boundary values but for a small
!> integer factor: the ghost-cell arithmetic is exact. Three leaves also carry
!> the slope pairs of plant_edges, on which the two sides of each Koren
!> threshold differ in the last bit.
!>
!> Usage: variants_gen <td_file> <out_dir>
program variants_gen
#include "cpp_macros.h"
  use m_af_types
  use m_af_core
  use m_af_utils
  use m_af_ghostcell
  use m_af_restrict
  use m_af_flux_schemes
  use m_af_limiters
  use hx_physics

  implicit none

  integer, parameter :: nc = 4
  real(dp), parameter :: two50 = 2.0_dp**50, two60 = 2.0_dp**60

  type(af_t)         :: tree
  type(ref_info_t)   :: ref_info
  character(len=256) :: td_file, out_dir
  character(len=40)  :: tag
  integer            :: grid(NDIM), lim, rot, meth, asg, nb, id, u_bc
  integer(8)         :: lcg_state = 20240917_8
  real(dp)           :: dom(NDIM), dtl(2)
  ! the boundary condition var_bc hands out, per face
  integer            :: bc_types(2*NDIM)
  real(dp)           :: bc_vals(2*NDIM)
  real(dp), allocatable :: save_e(:, :)
  integer, parameter :: four_types(4) = [af_bc_dirichlet, af_bc_neumann, &
       af_bc_continuous, af_bc_dirichlet_copy]

  call get_command_argument(1, td_file)
  call get_command_argument(2, out_dir)

#if NDIM == 3
  grid = nc
#else
  grid = 4 * nc
#endif
  dom  = 2.0_dp**(-10)

  call hx_init_gas(1.0_dp, 300.0_dp)
  call hx_init_transport(trim(td_file))
  current_voltage = 0.0_dp

  ! the layout of hx_physics
  call af_add_cc_variable(tree, "e", n_copies=3)
  call af_add_cc_variable(tree, "M+", n_copies=3)
  call af_add_cc_variable(tree, "M-", n_copies=3)
  call af_add_cc_variable(tree, "phi", n_copies=2)
  call af_add_cc_variable(tree, "electric_fld")
  call af_add_cc_variable(tree, "rhs")
  call af_add_cc_variable(tree, "tmp")
  call af_add_fc_variable(tree, "flux_elec")
  call af_add_fc_variable(tree, "field")
  if (tree%n_var_cell /= n_cc_vars) error stop "variable layout"

  call set_bc_all(af_bc_neumann, 0.0_dp, 0.0_dp)
  call af_set_cc_methods(tree, i_e, var_bc, af_gc_interp_lim)
  call af_set_cc_methods(tree, i_pos, af_bc_neumann_zero, af_gc_interp_lim)
  call af_set_cc_methods(tree, i_neg, af_bc_neumann_zero, af_gc_interp_lim)
  call af_set_cc_methods(tree, i_efld, af_bc_neumann_zero, af_gc_interp)
  call af_set_cc_methods(tree, i_phi, af_bc_neumann_zero, af_gc_interp)

  call af_init(tree, nc, dom, grid)
  call af_adjust_refinement(tree, ref_rule, ref_info)
  call af_adjust_refinement(tree, ref_rule, ref_info)
  if (tree%highest_lvl /= 3) error stop "tree: three levels expected"

  ! the input, box by box in id order
  do id = 1, tree%highest_id
     if (tree%boxes(id)%in_use) call set_input(tree%boxes(id))
  end do
  do id = 1, 3
     call plant_edges(tree%boxes(tree%lvls(2)%leaves(id)))
  end do
  call af_restrict_tree(tree, [i_e])
  call af_gc_tree(tree, [i_e])

  allocate(save_e((nc+2)**NDIM, tree%highest_id))
  do id = 1, tree%highest_id
     save_e(:, id) = pack(tree%boxes(id)%cc(DTIMES(:), i_e), .true.)
  end do

  call dump_topology("topology.bin")
  call dump_tables()
  call dump_cc("in_e.bin", i_e)
  call dump_cc("in_efld.bin", i_efld)
  call dump_fc("in_field.bin", f_field)

  ! flux limiters, the default prolongation limiter
  do lim = 1, 7
     call restore()
     call flux_upwind_tree(tree, 1, [i_e], 0, [f_flux], 2, dtl, &
          hx_flux_upwind, hx_flux_direction, flux_dummy_line_modify, lim)
     write(tag, "(A,I0,A)") "flux_", lim, ".bin"
     call dump_fc(trim(tag), f_flux, dtl)
  end do

  ! prolongation limiters through gc2_prolong_rb, Koren flux
  do lim = 1, 7
     call restore()
     tree%cc_methods(i_e)%prolong_limiter = lim
     call flux_upwind_tree(tree, 1, [i_e], 0, [f_flux], 2, dtl, &
          hx_flux_upwind, hx_flux_direction, flux_dummy_line_modify, &
          af_limiter_koren_t)
     write(tag, "(A,I0,A)") "pflux_", lim, ".bin"
     call dump_fc(trim(tag), f_flux, dtl)
  end do
#if NDIM == 3
  tree%cc_methods(i_e)%prolong_limiter = af_limiter_gminmod43_t
#else
  tree%cc_methods(i_e)%prolong_limiter = af_limiter_mc_t
#endif

  ! the types and values of the boundary variants, in their order
  open(newunit=u_bc, file=trim(out_dir)//"/bc.bin", &
       access="stream", form="unformatted", status="replace")

  ! one ghost layer: the four boundary types rotated over the faces
  do rot = 0, 3
     do nb = 1, 2*NDIM
        bc_types(nb) = four_types(1 + modulo(nb - 1 + rot, 4))
        bc_vals(nb)  = face_value(bc_types(nb), nb)
     end do
     write(u_bc) bc_types, bc_vals
     do meth = 1, 2
        call restore()
        if (meth == 1) then
           tree%cc_methods(i_e)%rb => af_gc_interp
        else
           tree%cc_methods(i_e)%rb => af_gc_interp_lim
        end if
        call af_gc_tree(tree, [i_e], corners=.true.)
        write(tag, "(A,I0,A,I0,A)") "gc_", rot, "_", meth, ".bin"
        call dump_cc(trim(tag), i_e)
     end do
  end do
  tree%cc_methods(i_e)%rb => af_gc_interp_lim

  ! two ghost layers: one type on every face, a value of its own per face
  do asg = 1, 3
     select case (asg)
     case (1)
        bc_types = af_bc_dirichlet
     case (2)
        bc_types = af_bc_neumann
     case (3)
        bc_types = af_bc_dirichlet_copy
     end select
     do nb = 1, 2*NDIM
        bc_vals(nb) = face_value(bc_types(nb), nb)
     end do
     write(u_bc) bc_types, bc_vals
     call restore()
     call flux_upwind_tree(tree, 1, [i_e], 0, [f_flux], 2, dtl, &
          hx_flux_upwind, hx_flux_direction, flux_dummy_line_modify, &
          af_limiter_koren_t)
     write(tag, "(A,I0,A)") "bflux_", asg, ".bin"
     call dump_fc(trim(tag), f_flux, dtl)
  end do
  close(u_bc)

contains

  !> k = 0..8 from the high bits of a 31-bit linear congruential generator
  integer function next_k()
    lcg_state = modulo(lcg_state * 1103515245_8 + 12345_8, 2147483648_8)
    next_k = int(modulo(lcg_state / 65536_8, 9_8))
  end function next_k

  subroutine set_input(box)
    type(box_t), intent(inout) :: box
    integer                    :: IJK, d
    do KJI_DO(0, nc+1)
       box%cc(IJK, i_e) = next_k() * two50
       box%cc(IJK, i_efld) = (1 + next_k()) * 2.0_dp**20
    end do; CLOSE_DO
    do d = 1, NDIM
       do KJI_DO(1, nc+1)
          box%fc(IJK, d, f_field) = (next_k() - 4) * 2.0_dp**18
       end do; CLOSE_DO
    end do
    box%fc(DTIMES(:), :, f_flux) = 0.0_dp
  end subroutine set_input

  !> On the lattice the two sides of a Koren threshold give the same number
  !> (the limiter is continuous, and third * 6 a rounds to 2 a). These slope
  !> pairs sit on the thresholds in floating point only -- a a == 0.25 (a b)
  !> with b one ulp from 4 a, and a a == 2.5 (a b) with a one ulp from 2.5 b,
  !> after the products are rounded -- and there the two sides differ in the
  !> last bit. Three cells in a row (0, a, a + b) along every dimension, from
  !> cell (1, 1[, 1]) for the first pair and from (2, 2[, 2]) for the second
  !> (all sums and differences exact), with a face field >= 0 on the faces
  !> between them, so that the electrons' flux takes limiter(a, b) there.
  subroutine plant_edges(box)
    type(box_t), intent(inout) :: box
    real(dp), parameter :: ea(2) = [8775936924003012.0_dp, 12780040261468158.0_dp]
    real(dp), parameter :: eb(2) = [35103747696012044.0_dp, 5112016104587264.0_dp]
    integer :: q, d, ix(NDIM)
    do q = 1, 2
       ix = q
       box%cc(DINDEX(ix), i_e) = 0.0_dp
       do d = 1, NDIM
          ix = q
          ix(d) = q + 1
          box%cc(DINDEX(ix), i_e) = ea(q)
          box%fc(DINDEX(ix), d, f_field) = 2.0_dp**18
          ix(d) = q + 2
          box%cc(DINDEX(ix), i_e) = ea(q) + eb(q)
          box%fc(DINDEX(ix), d, f_field) = 2.0_dp**18
       end do
    end do
  end subroutine plant_edges

  !> The boundary value of face nb: a power of two times a small integer,
  !> non-zero, another on every face
  real(dp) function face_value(bc_type, nb)
    integer, intent(in) :: bc_type, nb
    if (bc_type == af_bc_neumann) then
       face_value = nb * two60
    else
       face_value = (nb + 1) * two50
    end if
  end function face_value

  subroutine set_bc_all(bc_type, v_neumann, v_other)
    integer, intent(in)  :: bc_type
    real(dp), intent(in) :: v_neumann, v_other
    bc_types = bc_type
    bc_vals  = merge(v_neumann, v_other, bc_type == af_bc_neumann)
  end subroutine set_bc_all

  !> Uniform per face: type and value from bc_types / bc_vals
  subroutine var_bc(box, nb, iv, coords, bc_val, bc_type)
    type(box_t), intent(in) :: box
    integer, intent(in)     :: nb
    integer, intent(in)     :: iv
    real(dp), intent(in)    :: coords(NDIM, box%n_cell**(NDIM-1))
    real(dp), intent(out)   :: bc_val(box%n_cell**(NDIM-1))
    integer, intent(out)    :: bc_type
    bc_type = bc_types(nb)
    bc_val  = bc_vals(nb)
  end subroutine var_bc

  !> Level 1 and the two level-2 boxes at opposite corners of the domain
  subroutine ref_rule(box, cell_flags)
    type(box_t), intent(in) :: box
    integer, intent(out)    :: cell_flags(DTIMES(box%n_cell))
    if (box%lvl == 1 .or. (box%lvl == 2 .and. &
         (all(box%ix == 1) .or. all(box%ix == 2 * grid / nc)))) then
       cell_flags = af_do_ref
    else
       cell_flags = af_keep_ref
    end if
  end subroutine ref_rule

  !> The input densities back (ghost cells included), the fluxes cleared
  subroutine restore()
    integer :: id
    do id = 1, tree%highest_id
       tree%boxes(id)%cc(DTIMES(:), i_e) = reshape(save_e(:, id), &
            shape(tree%boxes(id)%cc(DTIMES(:), i_e)))
       tree%boxes(id)%fc(DTIMES(:), :, f_flux) = 0.0_dp
    end do
  end subroutine restore

  subroutine dump_cc(fname, iv)
    character(len=*), intent(in) :: fname
    integer, intent(in)          :: iv
    integer                      :: u, id
    open(newunit=u, file=trim(out_dir)//"/"//fname, &
         access="stream", form="unformatted", status="replace")
    do id = 1, tree%highest_id
       write(u) tree%boxes(id)%cc(DTIMES(:), iv)
    end do
    close(u)
  end subroutine dump_cc

  subroutine dump_fc(fname, ifc, dt_lim)
    character(len=*), intent(in)   :: fname
    integer, intent(in)            :: ifc
    real(dp), intent(in), optional :: dt_lim(2)
    integer                        :: u, id
    open(newunit=u, file=trim(out_dir)//"/"//fname, &
         access="stream", form="unformatted", status="replace")
    do id = 1, tree%highest_id
       write(u) tree%boxes(id)%fc(DTIMES(:), :, ifc)
    end do
    if (present(dt_lim)) write(u) dt_lim
    close(u)
  end subroutine dump_fc

  subroutine dump_topology(fname)
    character(len=*), intent(in) :: fname
    integer :: u, id, lvl
    open(newunit=u, file=trim(out_dir)//"/"//fname, &
         access="stream", form="unformatted", status="replace")
    write(u) tree%n_cell, tree%highest_id, tree%highest_lvl, &
         tree%n_var_cell, tree%n_var_face
    write(u) tree%coarse_grid_size(1:NDIM)
    write(u) tree%r_base, tree%dr_base
    do id = 1, tree%highest_id
       associate (b => tree%boxes(id))
         write(u) b%lvl, b%ix, b%parent, b%children, b%neighbors, &
              b%neighbor_mat, b%r_min, b%dr
       end associate
    end do
    do lvl = 1, tree%highest_lvl
       write(u) size(tree%lvls(lvl)%ids), size(tree%lvls(lvl)%leaves), &
            size(tree%lvls(lvl)%parents)
       write(u) tree%lvls(lvl)%ids, tree%lvls(lvl)%leaves, &
            tree%lvls(lvl)%parents
    end do
    write(u) current_voltage, gas_number_density, dom
    close(u)
  end subroutine dump_topology

  subroutine dump_tables()
    integer :: u
    open(newunit=u, file=trim(out_dir)//"/tables.bin", &
         access="stream", form="unformatted", status="replace")
    write(u) td_tbl%n_points, td_tbl%n_cols, td_tbl%x_min, td_tbl%inv_fac
    write(u) td_tbl%rows_cols
    write(u) chemtbl_fld%n_points, chemtbl_fld%n_cols, chemtbl_fld%x_min, &
         chemtbl_fld%inv_fac
    write(u) chemtbl_fld%rows_cols
    close(u)
  end subroutine dump_tables

end program variants_gen
