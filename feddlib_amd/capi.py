"""ctypes binding of include/fedd_hip.h -- the same C ABI a reference-side stub would bind
(INTEGRATION.md).  Host-side plumbing for tests and bench.py only: every numeric call lands in
the HIP library; if libfedd_hip.so is missing this module raises (no fallback path)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfedd_hip.so")

FORM_LAPLACE, FORM_LAPLACE_VEC, FORM_MASS, FORM_MASS_VEC, FORM_LINELAS, FORM_BDSTAB, FORM_STRESS, FORM_LAPLACE_XDIM = range(8)
BLOCK_SCALAR, BLOCK_DIAG, BLOCK_FULL = range(3)
COMBINE_RESTRICTED, COMBINE_AVERAGING, COMBINE_FULL = range(3)
(T_SYMBOLIC, T_ASSEMBLE, T_RHS, T_DIRICHLET, T_SPMV, T_SCHWARZ_SETUP, T_SCHWARZ_APPLY, T_ORTHO, T_COARSE_SETUP,
 T_COARSE_APPLY, T_HALO, T_ALLREDUCE, T_SPMV_SETUP) = range(13)
TIMER_NAMES = ["symbolic", "assemble", "rhs", "dirichlet", "spmv", "schwarz_setup", "schwarz_apply", "ortho",
               "coarse_setup", "coarse_apply", "halo", "allreduce", "spmv_setup", "gs_dot", "gs_update", "gs_fused",
               "full_park_mfma", "full_park", "full_gather", "cg_pq", "cg_xr", "cg_rz", "cg_p", "newmark_state", "block_apply", "multistep_state", "blockprec_bt",
               "newton_residual", "newton_update", "mesh_move", "move_check", "interface_distance", "fsi_match", "fsi_merge",
               "fsi_apply"]
COARSE_Q1 = 1
COARSE_GDSW = 2
COARSE_RGDSW = 3
LEVELS_ADDITIVE = 0         # FROSch "Level Combination" (fedd_schwarz_set_level_combination)
LEVELS_MULTIPLICATIVE = 1
ADV_N, ADV_W, ADV_NEWTON = range(3)     # fedd_assemble_advection
ALE_P, ALE_FIXEDPOINT, ALE_NEWTON = range(3)     # fedd_assemble_advection_ale
HYPER_NEOHOOKE, HYPER_MOONEY_RIVLIN, HYPER_STVK = range(3)   # fedd_assemble_hyperelastic: model
HYPER_TANGENT, HYPER_FORCE = 1, 2                            # ... what (or-ed)
BLOCKPREC_DIAGONAL, BLOCKPREC_TRIANGULAR = 1, 2              # fedd_block_prec_attach: kind
STAGE_ERR_EUCLIDEAN, STAGE_ERR_L2 = 0, 1                     # fedd_stage_error: kind

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

# name -> argtypes; every symbol declared in include/fedd_hip.h (tests check the two lists agree)
SIGNATURES = {
    "fedd_ctx_create": [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_int],
    "fedd_ctx_destroy": [C.c_void_p],
    "fedd_last_error": [],
    "fedd_sync": [C.c_void_p],
    "fedd_nccl_unique_id": [C.c_void_p],
    "fedd_mesh_structured_sizes": [C.c_int, _ip, _ip, C.c_int, C.c_int, _i64p, _i64p, _i64p, _i64p],
    "fedd_mesh_structured_build": [C.c_int, _ip, _ip, C.c_int, _f64p, _f64p, C.c_int, C.c_int, _i32p, _f64p,
                                   _i64p, _i32p, _i64p, _i32p],
    "fedd_mesh_structured_owner": [C.c_int, _ip, _ip, C.c_int64, _i64p, _i32p],
    "fedd_mesh_structured_row_ghosts": [C.c_int, _ip, _ip, C.c_int, C.c_int, _f64p, _f64p, C.c_int, _i64p, _i64p, _i32p],
    "fedd_mesh_structured_p2_sizes": [C.c_int, _ip, _ip, C.c_int, _i64p, _i64p, _i64p],
    "fedd_mesh_structured_p2_build": [C.c_int, _ip, _ip, C.c_int, C.c_int, _f64p, _i64p, _i64p, _i32p, _i32p, _i32p,
                                      _i32p, _i32p],
    "fedd_mesh_p2_vertices_first": [C.c_int, _ip, _ip, C.c_int, _i32p, _i64p],
    "fedd_mesh_read_sizes": [C.c_char_p, C.c_int, _i64p, _i64p, _i64p],
    "fedd_mesh_read": [C.c_char_p, C.c_int, _f64p, _i32p, _i32p, _i32p, _i32p, _i32p],
    "fedd_mesh_p2_sizes": [C.c_int, C.c_int64, _i32p, _i64p],
    "fedd_mesh_p2_build": [C.c_int, C.c_int64, C.c_int64, _i32p, _f64p, _i32p, C.c_int64, _i32p, _i32p, C.c_int,
                           _i32p, _f64p, _i32p],
    "fedd_mesh_partition": [C.c_int, C.c_int, C.c_int64, _i32p, C.c_int64, _f64p, C.c_int, _i32p],
    "fedd_mesh_partition_sizes": [C.c_int, C.c_int64, _i32p, C.c_int64, _i32p, C.c_int, C.c_int, C.c_int, _i64p, _i64p, _i64p, _i64p],
    "fedd_mesh_partition_extract": [C.c_int, C.c_int, C.c_int64, _i32p, C.c_int64, _f64p, _i32p, _i32p, C.c_int, C.c_int, C.c_int,
                                    _i32p, _f64p, _i64p, _i32p, _i32p, _i64p, _i32p, _i64p, _i32p, _i64p],
    "fedd_mesh_boundary_faces": [C.c_int, C.c_int, C.c_int64, _i32p, C.c_int64, _i64p, _i32p],
    "fedd_mesh_p2_surfaces": [C.c_int, C.c_int64, C.c_int64, _i32p, C.c_int64, _i32p, _i32p],
    "fedd_mesh_structured_surfaces_sizes": [C.c_int, _ip, _ip, C.c_int, C.c_int, _i64p],
    "fedd_mesh_structured_surfaces": [C.c_int, _ip, _ip, C.c_int, C.c_int, C.c_int, _i32p, _i32p],
    "fedd_surface_set": [C.c_void_p, C.c_int, C.c_int64, _i32p, _i32p],
    "fedd_assemble_surface": [C.c_void_p, C.c_int, C.c_int, _i32p, _f64p, C.c_int, C.c_int],
    "fedd_assemble_surface_values": [C.c_void_p, C.c_int, _f64p, C.c_int, C.c_int],
    "fedd_fe_quadrature": [C.c_int, C.c_int, _ip, _f64p, _f64p],
    "fedd_fe_basis": [C.c_int, C.c_int, C.c_int, _f64p, _f64p],
    "fedd_mesh_set": [C.c_void_p, C.c_int, C.c_int, C.c_int64, _i32p, C.c_int64, _f64p, _i64p, C.c_int64,
                      _i64p, _i32p],
    "fedd_mesh_set_rows": [C.c_void_p, C.c_int, C.c_int, C.c_int64, _i32p, C.c_int64, _f64p, _i64p, C.c_int64,
                           _i64p, _i32p, C.c_int64, _i64p, _i32p],
    "fedd_mesh_move": [C.c_void_p, _f64p],
    "fedd_mesh_move_info": [C.c_void_p, _i64p, _i64p, _f64p],
    "fedd_mesh_coords_get": [C.c_void_p, _f64p],
    "fedd_pattern_build": [C.c_void_p, C.c_int, C.c_int, _i64p],
    "fedd_assemble": [C.c_void_p, C.c_int, _f64p],
    "fedd_assemble_stress": [C.c_void_p, _f64p, C.c_int64],
    "fedd_assemble_rhs": [C.c_void_p, C.c_int, _f64p, C.c_int],
    "fedd_dirichlet": [C.c_void_p, C.c_int, _i32p, _i32p, _f64p],
    "fedd_dirichlet_nodes": [C.c_void_p, C.c_int64, _i32p, _i32p, _f64p],
    "fedd_dirichlet_rows": [C.c_void_p, C.c_int64, _i32p, _f64p],
    "fedd_matrix_store": [C.c_void_p, C.c_int],
    "fedd_matrix_scale": [C.c_void_p, C.c_int, C.c_double],
    "fedd_assemble_div": [C.c_void_p, C.c_int64, C.c_int, C.c_int],
    "fedd_block_merge": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int],
    "fedd_matrix_sizes": [C.c_void_p, C.c_int, _i64p, _i64p, _i64p],
    "fedd_matrix_get": [C.c_void_p, C.c_int, _i64p, _i32p, _f64p],
    "fedd_velocity_set": [C.c_void_p, _f64p],
    "fedd_assemble_advection": [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int],
    "fedd_mesh_velocity_set": [C.c_void_p, _f64p],
    "fedd_mesh_velocity_diff": [C.c_void_p, _f64p, _f64p, C.c_double],
    "fedd_mesh_velocity_get": [C.c_void_p, _f64p],
    "fedd_interface_distance": [C.c_void_p, C.c_int, _i32p, _i64p],
    "fedd_interface_distance_points": [C.c_void_p, C.c_int64, _f64p],
    "fedd_interface_distance_set": [C.c_void_p, _f64p],
    "fedd_interface_distance_get": [C.c_void_p, _f64p],
    "fedd_interface_distance_info": [C.c_void_p, _ip, _i64p, _ip],
    "fedd_laplace_scale_get": [C.c_void_p, _f64p],
    "fedd_assemble_advection_ale": [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int],
    "fedd_assemble_hyperelastic": [C.c_void_p, C.c_int, _f64p, C.c_int, C.c_int],
    "fedd_hyperelastic_force_get": [C.c_void_p, _f64p],
    "fedd_assemble_hyperelastic_time": [C.c_void_p, C.c_int, _f64p, C.c_int, C.c_int, C.c_int, C.c_double],
    "fedd_newton_begin": [C.c_void_p],
    "fedd_newton_source_set": [C.c_void_p, _f64p],
    "fedd_newton_residual": [C.c_void_p, C.c_int, C.c_double, C.c_int, _i32p, _i32p, _f64p, _f64p],
    "fedd_newton_update": [C.c_void_p, C.c_double, _f64p],
    "fedd_newton_end": [C.c_void_p],
    "fedd_newton_get": [C.c_void_p, _f64p],
    "fedd_newton_info": [C.c_void_p, _ip, _i64p, _ip, _ip, _i64p, _i64p],
    "fedd_matrix_combine": [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double],
    "fedd_matrix_combine_current": [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, _ip],
    "fedd_matrix_apply": [C.c_void_p, C.c_int, C.c_double, _f64p, _f64p],
    "fedd_newmark_begin": [C.c_void_p],
    "fedd_newmark_set": [C.c_void_p, _f64p, _f64p, _f64p],
    "fedd_newmark_get": [C.c_void_p, _f64p, _f64p, _f64p],
    "fedd_newmark_advance": [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double],
    "fedd_multistep_begin": [C.c_void_p, C.c_int],
    "fedd_multistep_advance": [C.c_void_p, C.c_int, C.c_int, _f64p],
    "fedd_multistep_set": [C.c_void_p, C.c_int, _f64p],
    "fedd_multistep_get": [C.c_void_p, C.c_int, _f64p],
    "fedd_multistep_info": [C.c_void_p, _ip, _ip],
    "fedd_stage_begin": [C.c_void_p, C.c_int],
    "fedd_stage_push": [C.c_void_p, C.c_int],
    "fedd_stage_rhs": [C.c_void_p, C.c_int, C.c_int, C.c_int, _f64p, _f64p],
    "fedd_block_merge_scaled": [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int],
    "fedd_stage_error": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _f64p],
    "fedd_stage_get": [C.c_void_p, C.c_int, _f64p, _f64p],
    "fedd_stage_info": [C.c_void_p, _ip, _ip, _i64p, _i64p],
    "fedd_rhs_axpy": [C.c_void_p, C.c_double, _f64p],
    "fedd_solution_set": [C.c_void_p, _f64p],
    "fedd_dirichlet_rhs": [C.c_void_p, C.c_int, _i32p, _i32p, _f64p],
    "fedd_csr_sizes": [C.c_void_p, _i64p, _i64p, _i64p],
    "fedd_csr_get": [C.c_void_p, _i64p, _i32p, _f64p, _i64p],
    "fedd_rhs_get": [C.c_void_p, _f64p],
    "fedd_rhs_set": [C.c_void_p, _f64p],
    "fedd_solution_get": [C.c_void_p, _f64p],
    "fedd_spmv": [C.c_void_p, _f64p, _f64p],
    "fedd_spmv_device": [C.c_void_p, C.c_int],
    "fedd_spmv_info": [C.c_void_p, _i64p, _i64p],
    "fedd_schwarz_setup": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int],
    "fedd_schwarz_set_target": [C.c_void_p, C.c_int, C.c_double],
    "fedd_schwarz_set_coarse": [C.c_void_p, C.c_double],
    "fedd_schwarz_set_level_combination": [C.c_void_p, C.c_int],
    "fedd_schwarz_get_level_combination": [C.c_void_p, _ip],
    "fedd_schwarz_coarse_sizes": [C.c_void_p, _i32p, _i64p],
    "fedd_schwarz_coarse_get": [C.c_void_p, _f64p],
    "fedd_schwarz_apply": [C.c_void_p, _f64p, _f64p],
    "fedd_schwarz_apply_device": [C.c_void_p, C.c_int],
    "fedd_schwarz_info": [C.c_void_p, _i64p, _i64p, _i64p],
    "fedd_schwarz_reuse_info": [C.c_void_p, _ip, _i64p],
    "fedd_pattern_reuse_info": [C.c_void_p, _ip, _i64p],
    "fedd_spmv_reuse_info": [C.c_void_p, _ip, _i64p],
    "fedd_setup_fused_info": [C.c_void_p, _i64p, _i64p, _i64p],
    "fedd_schwarz_unique": [C.c_void_p, _i64p],
    "fedd_schwarz_sizes": [C.c_void_p, _i64p, _i64p],
    "fedd_schwarz_conforming": [C.c_void_p, _i64p],
    "fedd_spmv_patterns": [C.c_void_p, _i64p, _i64p],
    "fedd_spmv_classes": [C.c_void_p, _i64p, _i64p, _i64p],
    "fedd_spmv_cls_blocks": [C.c_void_p, _i64p, _i64p],
    "fedd_spmv_col_bytes": [C.c_void_p, C.POINTER(C.c_int), _i64p],
    "fedd_gmres": [C.c_void_p, _f64p, _f64p, C.c_double, C.c_int, C.c_int, C.c_int, _ip, _f64p],
    "fedd_set_option": [C.c_void_p, C.c_char_p, C.c_double],
    "fedd_timing_enable": [C.c_void_p, C.c_int],
    "fedd_timing_reset": [C.c_void_p],
    "fedd_timing_get": [C.c_void_p, C.c_int, _f64p, _i64p],
    "fedd_timing_get_sampled": [C.c_void_p, C.c_int, _f64p, _i64p, _f64p],
    "fedd_gmres_info": [C.c_void_p, _ip, _ip, _ip, _ip],
    "fedd_gmres_capture_arm": [C.c_void_p, C.c_int],
    "fedd_gmres_capture_info": [C.c_void_p, _i64p],
    "fedd_gmres_capture_get": [C.c_void_p, C.c_char_p, _f64p, C.c_int64],
    "fedd_gmres_fused_blocks": [C.c_void_p, C.POINTER(C.c_int)],
    "fedd_gmres_x0": [C.c_void_p, _f64p, _f64p, C.c_double, C.c_int, C.c_int, C.c_int, _ip, _f64p],
    "fedd_gmres_status": [C.c_void_p, _ip, _f64p],
    "fedd_cg": [C.c_void_p, _f64p, _f64p, C.c_double, C.c_int, C.c_int, _ip, _f64p],
    "fedd_cg_x0": [C.c_void_p, _f64p, _f64p, C.c_double, C.c_int, C.c_int, _ip, _f64p],
    "fedd_cg_info": [C.c_void_p, _ip, _ip],
    "fedd_schwarz_full_info": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "fedd_mesh_setup_info": [C.c_void_p, _f64p, _f64p, _ip, _i64p],
    "fedd_schwarz_coarse_apply": [C.c_void_p, _f64p, _f64p],
    "fedd_read_bandwidth": [C.c_void_p, C.c_int64, C.c_int, _f64p],
    "fedd_rccl_selftest": [C.c_void_p, C.c_int, _f64p],
    "fedd_comm_selftest": [C.c_void_p, C.c_int, _f64p],
    "fedd_halo_plan_sizes": [C.c_void_p, _ip, _i64p, _i64p],
    "fedd_halo_plan_get": [C.c_void_p, _i32p, _i64p, _i32p, _i64p, _i32p],
    "fedd_halo_set_owners": [C.c_void_p, C.c_int64, _i64p, _i32p],
    "fedd_halo_requests_sizes": [C.c_void_p, _i64p],
    "fedd_halo_requests_get": [C.c_void_p, _i64p],
    "fedd_halo_requests_set": [C.c_void_p, _i64p, _i64p],
    "fedd_halo_exchange_setup": [C.c_void_p],
    "fedd_comm_set_host_callbacks": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "fedd_matrix_import": [C.c_void_p, C.c_void_p, C.c_int],
    "fedd_block_prec_attach": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int],
    "fedd_block_prec_detach": [C.c_void_p],
    "fedd_block_prec_info": [C.c_void_p, _ip, _f64p, _ip, _i64p],
    "fedd_interface_match": [C.c_void_p, C.c_void_p, C.c_int, _i32p],
    "fedd_interface_match_sizes": [C.c_void_p, _i64p, _ip, _ip],
    "fedd_interface_match_get": [C.c_void_p, _i32p, _i32p, _i64p],
    "fedd_interface_match_info": [C.c_void_p, _ip, _i64p, _f64p, _ip],
    "fedd_fsi_merge": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_uint8)],
    "fedd_fsi_interface_rhs": [C.c_void_p, _f64p],
    "fedd_fsi_info": [C.c_void_p, _i64p, _i64p, _i64p, _i64p, _i64p, _ip, _i64p],
    "fedd_fsi_prec_attach": [C.c_void_p, C.c_void_p, C.c_void_p],
    "fedd_fsi_prec_detach": [C.c_void_p],
    "fedd_fsi_prec_info": [C.c_void_p, _ip, _i64p],
}

def butcher_table(number):
    """(c, A) of the reference's Butcher table `number` (TimeSteppingTools::setTableInformationRK, TimeSteppingTools.cpp:309-487):
    0 = implicit Euler, 1 = Crank-Nicolson, 2 = the pressure-corrected fractional-step theta scheme, 3 = DIRK3L, 4 = DIRK34.
    c[s] and A[s, j] for the stages s = 0 .. S - 1; all are diagonally implicit with a dummy first stage (a_00 = 0) and
    stiffly accurate, so b is the last row of A.  The derived constants are evaluated in the reference's order.

    One entry differs from the reference ON PURPOSE: a_22 of table 2 is Theta_t * beta, the middle substep of the fractional-step
    theta scheme, u_2 = u_1 + Theta_t dt (alpha f_1 + beta f_2).  TimeSteppingTools.cpp:369 writes Theta_t * alpha there; with it
    row 2 no longer sums to c_2 = Theta + Theta_t and the scheme falls from the order 2 the reference states (convOrder_ = 2, :397)
    to order 1 (tests/test_singlestep_ref.py measures both).

    Two constants of table 4 differ ON PURPOSE as well: alpha = 0.158983899988677, the smallest root of
    x^3 - 3 x^2 + (3/2) x - 1/6, and sigma = 0.0966483609791597.  With c = (0, 2 alpha, 1, 1) and this alpha the third-order
    conditions sum b_i c_i = 1/2, sum b_i c_i^2 = 1/3, sum b_i a_ij c_j = 1/6 give exactly the reference's gamma and beta, and this
    sigma.  TimeSteppingTools.cpp:426, 429 write 0.1558983899988677 and 0.09666483609791597, each with one digit doubled; with
    them sum b_i c_i = 0.4922 and the scheme is of order 1 where the reference states 3 (convOrder_ = 3, :453)."""
    theta = 1.0 - np.sqrt(2.0) / 2.0
    theta_t = 1.0 - 2.0 * theta
    alpha = theta_t / (1.0 - theta)
    beta = 1.0 - alpha
    if number == 0:
        c = [0.0, 1.0]
        a = [[0.0, 0.0],
             [0.0, 1.0]]
    elif number == 1:
        c = [0.0, 1.0]
        a = [[0.0, 0.0],
             [0.5, 0.5]]
    elif number == 2:
        c = [0.0, theta, theta + theta_t, 1.0]
        a = [[0.0, 0.0, 0.0, 0.0],
             [theta * beta, theta * alpha, 0.0, 0.0],
             [theta * beta, (theta + theta_t) * alpha, theta_t * beta, 0.0],
             [theta * beta, (theta + theta_t) * alpha, (theta + theta_t) * beta, theta * alpha]]
    elif number == 3:
        alpha = 1.0 - np.sqrt(2.0) / 2.0
        a21 = 1.0 / (4.0 * (1.0 - alpha))
        c = [0.0, 2.0 * alpha, 1.0]
        a = [[0.0, 0.0, 0.0],
             [alpha, alpha, 0.0],
             [1.0 - a21 - alpha, a21, alpha]]
    elif number == 4:
        alpha, beta, gamma, sigma = 0.158983899988677, 1.072486270734370, 0.7685298292769537, 0.0966483609791597
        c = [0.0, 2.0 * alpha, 1.0, 1.0]
        a = [[0.0, 0.0, 0.0, 0.0],
             [alpha, alpha, 0.0, 0.0],
             [1.0 - beta - alpha, beta, alpha, 0.0],
             [1.0 - gamma - sigma - alpha, gamma, sigma, alpha]]
    else:
        raise ValueError("butcher_table: tables 0 .. 4 are built (got %r)" % (number,))
    c, a = np.array(c, dtype=np.float64), np.array(a, dtype=np.float64)
    if a[0, 0] != 0.0:
        raise ValueError("butcher_table: table %r has a_00 = %g; the first stage must be a dummy stage" % (number, a[0, 0]))
    return c, a


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _i32p, _i64p, _f64p, _i64p, _f64p, C.c_int)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _f64p, C.c_int)


class ThreadGroup:
    """In-process stand-in for a communicator: `world` threads of one process, one rank (and one
    fedd_ctx) each.  Lets the complete N > 1 path run with more ranks than a one-GPU box admits
    processes (the 2 x 2 x 2 decomposition: 8 ranks).  Functional tests only."""

    def __init__(self, world, timeout=120.0):
        import collections
        import threading
        self.world = world
        self.timeout = timeout
        self._barrier = threading.Barrier(world)
        self._slots = [None] * world
        self._cv = threading.Condition()
        self._box = collections.defaultdict(collections.deque)

    def allgather(self, rank, obj):
        self._slots[rank] = obj
        self._barrier.wait(self.timeout)
        out = list(self._slots)
        self._barrier.wait(self.timeout)
        return out

    def send(self, src, dst, arr):
        with self._cv:
            self._box[(src, dst)].append(np.array(arr, copy=True))
            self._cv.notify_all()

    def recv(self, src, dst):
        with self._cv:
            if not self._cv.wait_for(lambda: len(self._box[(src, dst)]) > 0, self.timeout):
                raise TimeoutError("ThreadGroup.recv %d <- %d" % (dst, src))
            return self._box[(src, dst)].popleft()

_lib = None


class FeddError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FeddError("%s is missing: build it with `python -m feddlib_amd.build` "
                            "(hipcc, gfx950); there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
        L.fedd_last_error.restype = C.c_char_p
        L.fedd_ctx_destroy.restype = None
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise FeddError(lib().fedd_last_error().decode())


def _p(a, ty):
    return None if a is None else a.ctypes.data_as(ty)


def _ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def _decomp(dim, N):
    return [int(N)] * dim if np.isscalar(N) else [int(x) for x in N]


def structured_mesh(dim, N, M, rank=0, origin=None, size=None, flags_option=1, ghosts=False):
    """Product-side structured generator (host code in the library).  N, M: ints or per-direction lists.
    ghosts: False / 0 = the reference's block, True / 1 = plus the elements that complete the owned rows,
    L >= 2 = L element layers around the owned nodes, which complete the rows of the ghost nodes within
    L - 1 layers (the dict then carries row_ghost_gid / row_ghost_flag, which Context.mesh_set_dict hands
    to fedd_mesh_set_rows)."""
    L = lib()
    dec, cel = _decomp(dim, N), _decomp(dim, M)
    ne, nr, nu, ng = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _chk(L.fedd_mesh_structured_sizes(dim, _ints(dec), _ints(cel), rank, int(ghosts), C.byref(ne), C.byref(nr),
                                      C.byref(nu), C.byref(ng)))
    conn = np.zeros((ne.value, dim + 1), dtype=np.int32)
    xyz = np.zeros((nr.value, dim), dtype=np.float64)
    gid_rep = np.zeros(nr.value, dtype=np.int64)
    flag_rep = np.zeros(nr.value, dtype=np.int32)
    gid_uni = np.zeros(nu.value, dtype=np.int64)
    flag_uni = np.zeros(nu.value, dtype=np.int32)
    o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
    s = None if size is None else np.ascontiguousarray(size, dtype=np.float64)
    _chk(L.fedd_mesh_structured_build(dim, _ints(dec), _ints(cel), rank, _p(o, _f64p), _p(s, _f64p), flags_option,
                                      int(ghosts), _p(conn, _i32p), _p(xyz, _f64p), _p(gid_rep, _i64p),
                                      _p(flag_rep, _i32p), _p(gid_uni, _i64p), _p(flag_uni, _i32p)))
    out = dict(dim=dim, nen=dim + 1, conn=conn, xyz=xyz, gid_rep=gid_rep, flag_rep=flag_rep, gid_uni=gid_uni,
               flag_uni=flag_uni, n_global=ng.value, decomp=dec, cells=cel, rank=rank)
    if int(ghosts) >= 2:
        nrg = C.c_int64()
        _chk(L.fedd_mesh_structured_row_ghosts(dim, _ints(dec), _ints(cel), rank, int(ghosts), _p(o, _f64p), _p(s, _f64p),
                                               flags_option, C.byref(nrg), None, None))
        rg = np.zeros(nrg.value, dtype=np.int64)
        rf = np.zeros(nrg.value, dtype=np.int32)
        _chk(L.fedd_mesh_structured_row_ghosts(dim, _ints(dec), _ints(cel), rank, int(ghosts), _p(o, _f64p), _p(s, _f64p),
                                               flags_option, C.byref(nrg), _p(rg, _i64p), _p(rf, _i32p)))
        out["row_ghost_gid"], out["row_ghost_flag"] = rg, rf
    return out


def _inverse(perm):
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.shape[0], dtype=perm.dtype)
    return inv


def vertices_first_perm(dim, N, M, rank=0):
    """(perm, n_p1) of fedd_mesh_p2_vertices_first: perm[new] = reference local id, the P1 lattice nodes first"""
    dec, cel = _decomp(dim, N), _decomp(dim, M)
    nr, np1 = C.c_int64(), C.c_int64()
    _chk(lib().fedd_mesh_structured_p2_sizes(dim, _ints(dec), _ints(cel), rank, C.byref(nr), None, None))
    perm = np.zeros(nr.value, dtype=np.int32)
    _chk(lib().fedd_mesh_p2_vertices_first(dim, _ints(dec), _ints(cel), rank, _p(perm, _i32p), C.byref(np1)))
    return perm, int(np1.value)


def structured_mesh_p2(dim, N, M, rank=0, flags_option=1, vertices_first=False):
    """Structured P2 mesh of the unit square / cube, the rank-local mesh of the reference (no ghost layers): the keys of
    structured_mesh plus owner_rep, elem_flag, perm and n_p1.  perm[new] = reference local id puts the P1 lattice nodes
    first in the P1 generator's order; with vertices_first the node arrays and conn come renumbered by it (the order the
    device layer wants for Stokes: pressure dof k = P1 node k), otherwise they are in the reference's numbering."""
    L = lib()
    dec, cel = _decomp(dim, N), _decomp(dim, M)
    nr, nu, ne, np1 = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _chk(L.fedd_mesh_structured_p2_sizes(dim, _ints(dec), _ints(cel), rank, C.byref(nr), C.byref(nu), C.byref(ne)))
    nen = 10 if dim == 3 else 6
    conn = np.zeros((ne.value, nen), dtype=np.int32)
    xyz = np.zeros((nr.value, dim), dtype=np.float64)
    gid_rep = np.zeros(nr.value, dtype=np.int64)
    owner = np.zeros(nr.value, dtype=np.int32)
    flag_rep = np.zeros(nr.value, dtype=np.int32)
    gid_uni = np.zeros(nu.value, dtype=np.int64)
    flag_uni = np.zeros(nu.value, dtype=np.int32)
    eflag = np.zeros(ne.value, dtype=np.int32)
    _chk(L.fedd_mesh_structured_p2_build(dim, _ints(dec), _ints(cel), rank, flags_option, _p(xyz, _f64p), _p(gid_rep, _i64p),
                                         _p(gid_uni, _i64p), _p(owner, _i32p), _p(flag_rep, _i32p), _p(flag_uni, _i32p),
                                         _p(conn, _i32p), _p(eflag, _i32p)))
    perm, n_p1 = vertices_first_perm(dim, dec, cel, rank)
    if vertices_first:
        inv = _inverse(perm)
        mine = owner == rank
        uni_of_rep = np.cumsum(mine) - 1                      # unique index of an owned node in the reference order
        conn = np.ascontiguousarray(inv[conn])
        xyz, gid_rep, flag_rep, owner = (np.ascontiguousarray(a[perm]) for a in (xyz, gid_rep, flag_rep, owner))
        keep = perm[mine[perm]]
        gid_uni, flag_uni = gid_uni[uni_of_rep[keep]], flag_uni[uni_of_rep[keep]]
    n_global = int(np.prod([2 * n * m + 1 for n, m in zip(dec, cel)]))
    return dict(dim=dim, nen=nen, conn=conn, xyz=xyz, gid_rep=gid_rep, flag_rep=flag_rep, gid_uni=gid_uni, flag_uni=flag_uni,
                n_global=n_global, decomp=dec, cells=cel, rank=rank, owner_rep=owner, elem_flag=eflag, perm=perm,
                n_p1=n_p1, vertices_first=bool(vertices_first))


def read_mesh(path, dim):
    """INRIA .mesh file -> one-rank P1 mesh dict (repeated = unique = identity numbering)."""
    L = lib()
    nv, ne, ns = C.c_int64(), C.c_int64(), C.c_int64()
    _chk(L.fedd_mesh_read_sizes(path.encode(), dim, C.byref(nv), C.byref(ne), C.byref(ns)))
    xyz = np.zeros((nv.value, dim)); vflag = np.zeros(nv.value, dtype=np.int32)
    conn = np.zeros((ne.value, dim + 1), dtype=np.int32); eflag = np.zeros(ne.value, dtype=np.int32)
    surf = np.zeros((ns.value, dim), dtype=np.int32); sflag = np.zeros(ns.value, dtype=np.int32)
    _chk(L.fedd_mesh_read(path.encode(), dim, _p(xyz, _f64p), _p(vflag, _i32p), _p(conn, _i32p), _p(eflag, _i32p),
                          _p(surf, _i32p), _p(sflag, _i32p)))
    gid = np.arange(nv.value, dtype=np.int64)
    return dict(dim=dim, nen=dim + 1, conn=conn, xyz=xyz, gid_rep=gid, flag_rep=vflag, gid_uni=gid.copy(),
                flag_uni=vflag.copy(), n_global=nv.value, elem_flag=eflag, surf=surf, surf_flag=sflag)


def p2_of_p1(m, volume_id=10):
    """P2 mesh dict from a one-rank P1 mesh dict (edge mid-points)."""
    L = lib()
    dim = m["dim"]
    conn = np.ascontiguousarray(m["conn"], dtype=np.int32)
    ned = C.c_int64()
    _chk(L.fedd_mesh_p2_sizes(dim, conn.shape[0], _p(conn, _i32p), C.byref(ned)))
    nv = m["xyz"].shape[0]
    nen2 = 10 if dim == 3 else 6
    conn2 = np.zeros((conn.shape[0], nen2), dtype=np.int32)
    xyz2 = np.zeros((nv + ned.value, dim)); flag2 = np.zeros(nv + ned.value, dtype=np.int32)
    xyz = np.ascontiguousarray(m["xyz"], dtype=np.float64); vf = np.ascontiguousarray(m["flag_rep"], dtype=np.int32)
    surf = np.ascontiguousarray(m.get("surf", np.zeros((0, dim), np.int32)), dtype=np.int32)
    sflag = np.ascontiguousarray(m.get("surf_flag", np.zeros(0, np.int32)), dtype=np.int32)
    _chk(L.fedd_mesh_p2_build(dim, nv, conn.shape[0], _p(conn, _i32p), _p(xyz, _f64p), _p(vf, _i32p), surf.shape[0],
                              _p(surf, _i32p), _p(sflag, _i32p), volume_id, _p(conn2, _i32p), _p(xyz2, _f64p),
                              _p(flag2, _i32p)))
    gid = np.arange(nv + ned.value, dtype=np.int64)
    return dict(dim=dim, nen=nen2, conn=conn2, xyz=xyz2, gid_rep=gid, flag_rep=flag2, gid_uni=gid.copy(),
                flag_uni=flag2.copy(), n_global=nv + ned.value, n_p1=nv, elem_flag=m.get("elem_flag"))


def partition_mesh(m, nparts):
    """element -> part of a one-rank mesh dict (read_mesh / p2_of_p1 / structured_mesh on one block)"""
    conn = np.ascontiguousarray(m["gid_rep"][m["conn"]], dtype=np.int32) if "gid_rep" in m else np.ascontiguousarray(m["conn"], np.int32)
    xyz = np.ascontiguousarray(m["xyz"], dtype=np.float64)
    part = np.zeros(conn.shape[0], dtype=np.int32)
    _chk(lib().fedd_mesh_partition(m["dim"], conn.shape[1], conn.shape[0], _p(conn, _i32p), xyz.shape[0], _p(xyz, _f64p),
                                   nparts, _p(part, _i32p)))
    return part


def partitioned_mesh(m, part, nparts, rank, ghosts=1):
    """rank's mesh dict (what structured_mesh(..., rank, ghosts=L) returns for the structured grid) cut out of the
    one-rank mesh dict m by the element partition `part`; carries owner_rep for Context.halo_set_owners"""
    L = lib()
    dim = m["dim"]
    conn = np.ascontiguousarray(m["conn"], dtype=np.int32)
    xyz = np.ascontiguousarray(m["xyz"], dtype=np.float64)
    flag = np.ascontiguousarray(m["flag_rep"], dtype=np.int32)
    part = np.ascontiguousarray(part, dtype=np.int32)
    nen = conn.shape[1]
    ne, nr, nu, ng = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _chk(L.fedd_mesh_partition_sizes(nen, conn.shape[0], _p(conn, _i32p), xyz.shape[0], _p(part, _i32p), nparts, rank, int(ghosts),
                                     C.byref(ne), C.byref(nr), C.byref(nu), C.byref(ng)))
    out = dict(dim=dim, nen=nen, conn=np.zeros((ne.value, nen), np.int32), xyz=np.zeros((nr.value, dim)),
               gid_rep=np.zeros(nr.value, np.int64), flag_rep=np.zeros(nr.value, np.int32), owner_rep=np.zeros(nr.value, np.int32),
               gid_uni=np.zeros(nu.value, np.int64), flag_uni=np.zeros(nu.value, np.int32),
               row_ghost_gid=np.zeros(ng.value, np.int64), row_ghost_flag=np.zeros(ng.value, np.int32),
               elem_gid=np.zeros(ne.value, np.int64), n_global=xyz.shape[0], rank=rank)
    _chk(L.fedd_mesh_partition_extract(dim, nen, conn.shape[0], _p(conn, _i32p), xyz.shape[0], _p(xyz, _f64p), _p(flag, _i32p),
                                       _p(part, _i32p), nparts, rank, int(ghosts), _p(out["conn"], _i32p), _p(out["xyz"], _f64p),
                                       _p(out["gid_rep"], _i64p), _p(out["flag_rep"], _i32p), _p(out["owner_rep"], _i32p),
                                       _p(out["gid_uni"], _i64p), _p(out["flag_uni"], _i32p), _p(out["row_ghost_gid"], _i64p),
                                       _p(out["row_ghost_flag"], _i32p), _p(out["elem_gid"], _i64p)))
    if int(ghosts) < 2:
        del out["row_ghost_gid"], out["row_ghost_flag"]
    return out


def boundary_faces(dim, conn, n_node):
    """the (dim-1)-faces that belong to exactly one element, [n, dim] with ascending vertex ids"""
    conn = np.ascontiguousarray(conn, dtype=np.int32)
    n = C.c_int64()
    _chk(lib().fedd_mesh_boundary_faces(dim, conn.shape[1], conn.shape[0], _p(conn, _i32p), n_node, C.byref(n), None))
    faces = np.zeros((n.value, dim), dtype=np.int32)
    _chk(lib().fedd_mesh_boundary_faces(dim, conn.shape[1], conn.shape[0], _p(conn, _i32p), n_node, C.byref(n), _p(faces, _i32p)))
    return faces


def p2_surfaces(m, surf=None):
    """P2 surface elements [n, 3 | 6] of the P1 surface elements `surf` (default m["surf"]) of the one-rank P1 mesh dict m,
    numbered as p2_of_p1(m) numbers the mid nodes"""
    dim = m["dim"]
    conn = np.ascontiguousarray(m["conn"], dtype=np.int32)
    s1 = np.ascontiguousarray(m["surf"] if surf is None else surf, dtype=np.int32).reshape(-1, dim)
    s2 = np.zeros((s1.shape[0], 3 if dim == 2 else 6), dtype=np.int32)
    _chk(lib().fedd_mesh_p2_surfaces(dim, m["xyz"].shape[0], conn.shape[0], _p(conn, _i32p), s1.shape[0], _p(s1, _i32p),
                                     _p(s2, _i32p)))
    return s2


def structured_surfaces(dim, N, M, rank=0, flags_option=1, ghosts=False, p2=False, vertices_first=False):
    """(surf [n, dim] local repeated ids, flags [n]): the boundary faces of structured_mesh(dim, N, M, rank, ghosts=ghosts).
    p2: the boundary edges [n, 3] / triangles [n, 6] of structured_mesh_p2(dim, N, M, rank, vertices_first=...) instead: the
    same faces with the same flags, vertices then mid nodes in the slot order of fedd_mesh_p2_surfaces."""
    dec, cel = _decomp(dim, N), _decomp(dim, M)
    if p2:
        if ghosts:
            raise FeddError("structured P2 meshes have no ghost layers")
        s1, sflag = structured_surfaces(dim, dec, cel, rank, flags_option)
        n1 = [c + 1 for c in cel] + [1] * (3 - dim)
        p2m = [2 * c + 1 for c in cel] + [1] * (3 - dim)
        r, s, t = s1 % n1[0], (s1 // n1[0]) % n1[1], s1 // (n1[0] * n1[1])
        v = 2 * r + p2m[0] * (2 * s + p2m[1] * 2 * t)          # the P1 lattice node (r,s,t) is P2 lattice node (2r,2s,2t)
        pairs = [(0, 1)] if dim == 2 else [(0, 1), (1, 2), (0, 2)]
        surf = np.concatenate([v] + [((v[:, a] + v[:, b]) // 2)[:, None] for a, b in pairs], axis=1).astype(np.int32)
        if vertices_first:
            surf = _inverse(vertices_first_perm(dim, dec, cel, rank)[0])[surf]
        return np.ascontiguousarray(surf), sflag
    n = C.c_int64()
    _chk(lib().fedd_mesh_structured_surfaces_sizes(dim, _ints(dec), _ints(cel), rank, int(ghosts), C.byref(n)))
    surf = np.zeros((n.value, dim), dtype=np.int32)
    sflag = np.zeros(n.value, dtype=np.int32)
    _chk(lib().fedd_mesh_structured_surfaces(dim, _ints(dec), _ints(cel), rank, flags_option, int(ghosts), _p(surf, _i32p),
                                             _p(sflag, _i32p)))
    return surf, sflag


def fe_quadrature(dim, degree):
    """(points [nq, dim], weights [nq]) of the product's quadrature rule"""
    nq = C.c_int()
    _chk(lib().fedd_fe_quadrature(dim, degree, C.byref(nq), None, None))
    pts = np.zeros((nq.value, dim)); w = np.zeros(nq.value)
    _chk(lib().fedd_fe_quadrature(dim, degree, C.byref(nq), _p(pts, _f64p), _p(w, _f64p)))
    return pts, w


def fe_basis(dim, nen, degree):
    """(phi [nq, nen], dphi [nq, nen, dim]) at the points of fe_quadrature(dim, degree)"""
    nq = fe_quadrature(dim, degree)[1].shape[0]
    phi = np.zeros((nq, nen)); dphi = np.zeros((nq, nen, dim))
    _chk(lib().fedd_fe_basis(dim, nen, degree, _p(phi, _f64p), _p(dphi, _f64p)))
    return phi, dphi


def structured_owner(dim, N, M, gids):
    dec, cel = _decomp(dim, N), _decomp(dim, M)
    g = np.ascontiguousarray(gids, dtype=np.int64)
    out = np.zeros(g.shape[0], dtype=np.int32)
    _chk(lib().fedd_mesh_structured_owner(dim, _ints(dec), _ints(cel), g.shape[0], _p(g, _i64p), _p(out, _i32p)))
    return out


def nccl_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _chk(lib().fedd_nccl_unique_id(buf))
    return buf.raw


class Context:
    """One per GPU / rank.  device < 0 gives a host-only context (numbering and halo planning only)."""

    def __init__(self, device=0, rank=0, nranks=1, nccl_id: bytes | None = None):
        self._L = lib()
        h = C.c_void_p()
        idbuf = C.create_string_buffer(nccl_id, 128) if nccl_id is not None else None
        _chk(self._L.fedd_ctx_create(C.byref(h), device, idbuf, rank, nranks))
        self._h = h
        self.rank, self.nranks = rank, nranks
        self.dofs = 1

    def close(self):
        if self._h:
            self._L.fedd_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _chk(self._L.fedd_sync(self._h))

    def mesh_set(self, dim, conn, xyz, gid_rep, gid_uni, flag_uni, row_ghost_gid=None, row_ghost_flag=None):
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        gid_rep = np.ascontiguousarray(gid_rep, dtype=np.int64)
        gid_uni = np.ascontiguousarray(gid_uni, dtype=np.int64)
        flag_uni = None if flag_uni is None else np.ascontiguousarray(flag_uni, dtype=np.int32)
        if row_ghost_gid is not None and len(row_ghost_gid):
            rg = np.ascontiguousarray(row_ghost_gid, dtype=np.int64)
            rf = None if row_ghost_flag is None else np.ascontiguousarray(row_ghost_flag, dtype=np.int32)
            _chk(self._L.fedd_mesh_set_rows(self._h, dim, conn.shape[1], conn.shape[0], _p(conn, _i32p), xyz.shape[0],
                                            _p(xyz, _f64p), _p(gid_rep, _i64p), gid_uni.shape[0], _p(gid_uni, _i64p),
                                            _p(flag_uni, _i32p), rg.shape[0], _p(rg, _i64p), _p(rf, _i32p)))
        else:
            _chk(self._L.fedd_mesh_set(self._h, dim, conn.shape[1], conn.shape[0], _p(conn, _i32p), xyz.shape[0],
                                       _p(xyz, _f64p), _p(gid_rep, _i64p), gid_uni.shape[0], _p(gid_uni, _i64p),
                                       _p(flag_uni, _i32p)))
        self.n_own = gid_uni.shape[0]
        self._dim = dim
        self._n_rep = xyz.shape[0]
        self._n_elem = conn.shape[0]

    def mesh_set_dict(self, m):
        self.mesh_set(m["dim"], m["conn"], m["xyz"], m["gid_rep"], m["gid_uni"], m["flag_uni"],
                      m.get("row_ghost_gid"), m.get("row_ghost_flag"))

    def mesh_move(self, disp=None):
        """x = x_ref + disp on the repeated map of mesh_set ([n_rep, dim] or flat), relative to the uploaded coordinates and not
        cumulative; None restores them.  Raises, and moves nothing, if an element would be inverted (fedd_mesh_move)"""
        d = None
        if disp is not None:
            d = np.ascontiguousarray(disp, dtype=np.float64).ravel()
            n = getattr(self, "_n_rep", None)
            if n is not None and d.shape[0] != n * self._dim:
                raise FeddError("mesh_move: displacement of %d entries, the repeated map has %d nodes in %dD" % (d.shape[0], n, self._dim))
        _chk(self._L.fedd_mesh_move(self._h, _p(d, _f64p)))

    def mesh_move_info(self):
        a, g, r = C.c_int64(), C.c_int64(), C.c_double()
        _chk(self._L.fedd_mesh_move_info(self._h, C.byref(a), C.byref(g), C.byref(r)))
        return {"n_moves": a.value, "geometry_id": g.value, "min_det_ratio": r.value}

    def mesh_coords(self):
        """the coordinates in force, [n_rep, dim] on the repeated map of mesh_set"""
        n = getattr(self, "_n_rep", 0)
        out = np.zeros((max(n, 1), getattr(self, "_dim", 1)))
        _chk(self._L.fedd_mesh_coords_get(self._h, _p(out, _f64p)))
        return out[:n]

    def pattern_build(self, dofs=1, block_mode=BLOCK_SCALAR) -> int:
        nnz = C.c_int64()
        _chk(self._L.fedd_pattern_build(self._h, dofs, block_mode, C.byref(nnz)))
        self.dofs = dofs
        return nnz.value

    def assemble(self, form, params=None):
        p = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
        _chk(self._L.fedd_assemble(self._h, form, _p(p, _f64p)))

    def assemble_stress(self, coeff=None):
        """the velocity block in stress form, c grad v : (grad u + grad u^T), into the FULL system pattern (fedd_assemble_stress);
        coeff[n_elem, nq] = c at the quadrature points of every element, None: c = 1"""
        q = None if coeff is None else np.ascontiguousarray(coeff, dtype=np.float64).reshape(-1)
        _chk(self._L.fedd_assemble_stress(self._h, _p(q, _f64p), 0 if q is None else q.shape[0]))

    def assemble_rhs(self, f_const, extra_degree=0):
        f = np.ascontiguousarray(np.atleast_1d(f_const), dtype=np.float64)
        _chk(self._L.fedd_assemble_rhs(self._h, self.dofs, _p(f, _f64p), extra_degree))

    def surface_set(self, surf, sflag):
        """surface elements [n, nsn] (local repeated node ids) with their flags; n = 0 clears the set"""
        s = np.ascontiguousarray(surf, dtype=np.int32)
        f = np.ascontiguousarray(sflag, dtype=np.int32)
        nsn = s.shape[1] if s.ndim == 2 and s.shape[1] else self._dim
        _chk(self._L.fedd_surface_set(self._h, nsn, f.shape[0], _p(s, _i32p), _p(f, _i32p)))

    def assemble_surface(self, g, flags=None, extra_degree=0, accumulate=False):
        """rhs (+)= int g phi_i over the surface elements: g[dofs] on all of them, or g[len(flags), dofs] by flag"""
        gg = np.ascontiguousarray(g, dtype=np.float64).ravel()
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.int32)
        _chk(self._L.fedd_assemble_surface(self._h, self.dofs, 0 if fl is None else fl.shape[0], _p(fl, _i32p), _p(gg, _f64p),
                                           extra_degree, int(accumulate)))

    def assemble_surface_values(self, g_surf, extra_degree=0, accumulate=False):
        """the same with one load per surface element, g_surf[n_surf, dofs]"""
        gg = np.ascontiguousarray(g_surf, dtype=np.float64).ravel()
        _chk(self._L.fedd_assemble_surface_values(self._h, self.dofs, _p(gg, _f64p), extra_degree, int(accumulate)))

    def dirichlet(self, flags, values=None, comp_mask=None):
        fl = np.ascontiguousarray(flags, dtype=np.int32)
        n = fl.shape[0]
        v = np.zeros(n * self.dofs) if values is None else np.ascontiguousarray(values, dtype=np.float64).ravel()
        m = None if comp_mask is None else np.ascontiguousarray(comp_mask, dtype=np.int32).ravel()
        _chk(self._L.fedd_dirichlet(self._h, n, _p(fl, _i32p), _p(m, _i32p), _p(v, _f64p)))

    def dirichlet_nodes(self, nodes, values, comp_mask=None):
        nd = np.ascontiguousarray(nodes, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        m = None if comp_mask is None else np.ascontiguousarray(comp_mask, dtype=np.int32).ravel()
        _chk(self._L.fedd_dirichlet_nodes(self._h, nd.shape[0], _p(nd, _i32p), _p(m, _i32p), _p(v, _f64p)))

    def dirichlet_rows(self, rows, values):
        r = np.ascontiguousarray(rows, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=np.float64)
        _chk(self._L.fedd_dirichlet_rows(self._h, r.shape[0], _p(r, _i32p), _p(v, _f64p)))

    def matrix_store(self, slot):
        _chk(self._L.fedd_matrix_store(self._h, slot))

    def matrix_scale(self, slot, alpha):
        _chk(self._L.fedd_matrix_scale(self._h, slot, float(alpha)))

    def assemble_div(self, n_pressure_nodes, slot_b, slot_bt):
        _chk(self._L.fedd_assemble_div(self._h, n_pressure_nodes, slot_b, slot_bt))

    def block_merge(self, slot_a, slot_bt, slot_b, slot_c=-1):
        _chk(self._L.fedd_block_merge(self._h, slot_a, slot_bt, slot_b, slot_c))
        self.dofs = 1

    def matrix_get(self, slot):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_matrix_sizes(self._h, slot, C.byref(a), C.byref(b), C.byref(c)))
        rowptr = np.zeros(a.value + 1, dtype=np.int64)
        col = np.zeros(c.value, dtype=np.int32)
        val = np.zeros(c.value, dtype=np.float64)
        _chk(self._L.fedd_matrix_get(self._h, slot, _p(rowptr, _i64p), _p(col, _i32p), _p(val, _f64p)))
        import scipy.sparse as sp
        return sp.csr_matrix((val, col, rowptr), shape=(a.value, b.value))

    def velocity_set(self, u_rep):
        """u_rep: [n_rep, dim] or flat dim * node + d, on the repeated map of mesh_set"""
        u = np.ascontiguousarray(u_rep, dtype=np.float64).ravel()
        _chk(self._L.fedd_velocity_set(self._h, _p(u, _f64p)))

    def assemble_advection(self, kind, scale=1.0, slot_add=-1, slot_out=4):
        """slot_out <- scale * (N | W | N + W)(u) + M[slot_add], FULL velocity pattern (fedd_assemble_advection)"""
        _chk(self._L.fedd_assemble_advection(self._h, kind, float(scale), slot_add, slot_out))

    def mesh_velocity_set(self, w_rep):
        """w_rep: [n_rep, dim] or flat dim * node + d, on the repeated map of mesh_set; None clears (fedd_mesh_velocity_set)"""
        w = None if w_rep is None else np.ascontiguousarray(w_rep, dtype=np.float64).ravel()
        _chk(self._L.fedd_mesh_velocity_set(self._h, _p(w, _f64p)))

    def mesh_velocity_diff(self, d_new_rep, d_old_rep, dt):
        """w <- (d_new - d_old) * (1.0 / dt) on the device (fedd_mesh_velocity_diff)"""
        a = np.ascontiguousarray(d_new_rep, dtype=np.float64).ravel()
        b = np.ascontiguousarray(d_old_rep, dtype=np.float64).ravel()
        _chk(self._L.fedd_mesh_velocity_diff(self._h, _p(a, _f64p), _p(b, _f64p), float(dt)))

    def mesh_velocity(self):
        """the mesh velocity in force, [n_rep, dim] on the repeated map of mesh_set (fedd_mesh_velocity_get)"""
        n = getattr(self, "_n_rep", 0)
        out = np.zeros((max(n, 1), getattr(self, "_dim", 1)))
        _chk(self._L.fedd_mesh_velocity_get(self._h, _p(out, _f64p)))
        return out[:n]

    def interface_distance(self, flags):
        """distances of every repeated node to the nodes whose flag is in `flags`, at the coordinates in force, capped at 1000
        (fedd_interface_distance); returns the number of interface nodes"""
        fl = np.ascontiguousarray(np.atleast_1d(flags), dtype=np.int32)
        n = C.c_int64()
        _chk(self._L.fedd_interface_distance(self._h, fl.shape[0], _p(fl, _i32p), C.byref(n)))
        return n.value

    def interface_distance_points(self, pts):
        """the same against points of the caller's, [n_pts, dim] (fedd_interface_distance_points)"""
        p = np.ascontiguousarray(pts, dtype=np.float64)
        dim = getattr(self, "_dim", 1)
        if p.size % dim:
            raise FeddError("interface_distance_points: %d coordinates are no multiple of the dimension %d" % (p.size, dim))
        _chk(self._L.fedd_interface_distance_points(self._h, p.size // dim, _p(p.ravel(), _f64p)))

    def interface_distance_set(self, dist_rep):
        """distances of the caller's on the repeated map of mesh_set, [n_rep]; None releases them (fedd_interface_distance_set)"""
        d = None
        if dist_rep is not None:
            d = np.ascontiguousarray(dist_rep, dtype=np.float64).ravel()
            n = getattr(self, "_n_rep", None)
            if n is not None and d.shape[0] != n:
                raise FeddError("interface_distance_set: %d distances, the repeated map has %d nodes" % (d.shape[0], n))
        _chk(self._L.fedd_interface_distance_set(self._h, _p(d, _f64p)))

    def interface_distances(self):
        """the distances held, [n_rep] on the repeated map of mesh_set (fedd_interface_distance_get)"""
        n = getattr(self, "_n_rep", 0)
        out = np.zeros(max(n, 1))
        _chk(self._L.fedd_interface_distance_get(self._h, _p(out, _f64p)))
        return out[:n]

    def interface_distance_info(self):
        h, n, t = C.c_int(), C.c_int64(), C.c_int()
        _chk(self._L.fedd_interface_distance_info(self._h, C.byref(h), C.byref(n), C.byref(t)))
        return {"have": bool(h.value), "n_interface": n.value, "tile_points": t.value}

    def laplace_scale(self):
        """the coefficient per element of the last FORM_LAPLACE_XDIM assembly, [n_elem] (fedd_laplace_scale_get)"""
        n = getattr(self, "_n_elem", 0)
        out = np.zeros(max(n, 1))
        _chk(self._L.fedd_laplace_scale_get(self._h, _p(out, _f64p)))
        return out[:n]

    def assemble_advection_ale(self, kind, scale=1.0, slot_add=-1, slot_out=4):
        """slot_out <- scale * (P(w) | N(u - w) - P(w) | N(u - w) + W(u) - P(w)) + M[slot_add], FULL velocity pattern
        (fedd_assemble_advection_ale)"""
        _chk(self._L.fedd_assemble_advection_ale(self._h, kind, float(scale), slot_add, slot_out))

    def assemble_hyperelastic(self, model, params, what=HYPER_TANGENT | HYPER_FORCE):
        """tangent -> system matrix (FULL pattern, dim dofs per node) and / or force vector of the material at the displacement
        given by velocity_set (fedd_assemble_hyperelastic); params: {E, nu} | {E, nu, C} | {lambda, mu}"""
        p = np.ascontiguousarray(params, dtype=np.float64).ravel()
        _chk(self._L.fedd_assemble_hyperelastic(self._h, int(model), _p(p, _f64p), p.shape[0], int(what)))

    def hyperelastic_force_get(self):
        f = np.zeros(self.n_own * self._dim, dtype=np.float64)
        _chk(self._L.fedd_hyperelastic_force_get(self._h, _p(f, _f64p)))
        return f

    def assemble_hyperelastic_time(self, model, params, slot_m, cm, what=HYPER_TANGENT | HYPER_FORCE):
        """assemble_hyperelastic with (cm * M[slot_m]) + K(u) as tangent, in one pass (fedd_assemble_hyperelastic_time)"""
        p = np.ascontiguousarray(params, dtype=np.float64).ravel()
        _chk(self._L.fedd_assemble_hyperelastic_time(self._h, int(model), _p(p, _f64p), p.shape[0], int(what), int(slot_m), float(cm)))

    def newton_begin(self):
        """u_k <- the current solution, b <- the current right-hand side (held), nodal vector field <- u_k"""
        _chk(self._L.fedd_newton_begin(self._h))

    def newton_source_set(self, s=None):
        """the step's source vector (None clears it)"""
        if s is not None:
            s = np.ascontiguousarray(s, dtype=np.float64)
            if s.shape[0] != self.csr_sizes()[0]:
                raise FeddError("newton_source_set: vector of %d entries, the system has %d rows" % (s.shape[0], self.csr_sizes()[0]))
        _chk(self._L.fedd_newton_source_set(self._h, _p(s, _f64p)))

    def newton_residual(self, slot_m, cm, flags=(), values=None, comp_mask=None):
        """rhs <- ((b - f) + s) - cm M u_k, Dirichlet rows g - u_k; returns ||rhs||_2 (fedd_newton_residual)"""
        fl = np.ascontiguousarray(flags, dtype=np.int32)
        n = fl.shape[0]
        v = np.zeros(max(1, n * self.dofs)) if values is None else np.ascontiguousarray(values, dtype=np.float64).ravel()
        m = None if comp_mask is None else np.ascontiguousarray(comp_mask, dtype=np.int32).ravel()
        nr = C.c_double()
        _chk(self._L.fedd_newton_residual(self._h, int(slot_m), float(cm), n, _p(fl, _i32p), _p(m, _i32p), _p(v, _f64p), C.byref(nr)))
        return nr.value

    def newton_update(self, alpha=1.0):
        """u_k <- u_k + alpha * (the device's solution vector), nodal vector field <- u_k; returns the update's 2-norm"""
        nd = C.c_double()
        _chk(self._L.fedd_newton_update(self._h, float(alpha), C.byref(nd)))
        return nd.value

    def newton_end(self):
        """solution vector <- u_k, right-hand side <- the held one"""
        _chk(self._L.fedd_newton_end(self._h))

    def newton_info(self):
        a, hs, ff = C.c_int(), C.c_int(), C.c_int()
        n, nr, nu = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_newton_info(self._h, C.byref(a), C.byref(n), C.byref(hs), C.byref(ff), C.byref(nr), C.byref(nu)))
        return {"active": bool(a.value), "n": n.value, "have_source": bool(hs.value), "force_fresh": bool(ff.value),
                "residuals": nr.value, "updates": nu.value}

    def newton_get(self):
        info = self.newton_info()
        if not info["active"]:      # the length of the host buffer comes from the state: none, no copy
            raise FeddError("newton_get: no Newton state (fedd_newton_begin first; fedd_newton_end and fedd_mesh_set end it)")
        out = np.zeros(info["n"])
        _chk(self._L.fedd_newton_get(self._h, _p(out, _f64p)))
        return out

    def matrix_combine(self, slot_m, cm, slot_a, ca):
        """system matrix <- (cm * M[slot_m]) + (ca * A[slot_a]) on the pattern of slot_a (TimeProblem::combineSystems)"""
        _chk(self._L.fedd_matrix_combine(self._h, slot_m, float(cm), slot_a, float(ca)))
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_matrix_sizes(self._h, slot_a, C.byref(a), C.byref(b), C.byref(c)))
        self.dofs = max(1, a.value // max(1, self.n_own))

    def matrix_combine_current(self, slot_m, cm, slot_a, ca):
        """True while the system matrix still is that combine (Dirichlet rows apart): nothing to rebuild"""
        k = C.c_int()
        _chk(self._L.fedd_matrix_combine_current(self._h, slot_m, float(cm), slot_a, float(ca), C.byref(k)))
        return bool(k.value)

    def matrix_apply(self, slot, x, alpha=1.0):
        """y = alpha * M[slot] x (Matrix::apply on a stored block)"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_matrix_sizes(self._h, slot, C.byref(a), C.byref(b), C.byref(c)))
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape[0] != b.value:
            raise FeddError("matrix_apply: x has %d entries, the block %d columns" % (x.shape[0], b.value))
        y = np.zeros(a.value)
        _chk(self._L.fedd_matrix_apply(self._h, slot, float(alpha), _p(x, _f64p), _p(y, _f64p)))
        return y

    def matrix_import(self, src, slot):
        """system matrix <- the block in `slot` of the context `src`, device to device (fedd_matrix_import); this context
        carries the block's mesh"""
        _chk(self._L.fedd_matrix_import(self._h, src._h, slot))
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_csr_sizes(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.dofs = max(1, a.value // max(1, self.n_own))

    def block_prec_attach(self, kind, velocity, schur, schur_scale=-1.0, slot_bt=2):
        """Diagonal / Triangular block preconditioner of this context's merged system out of two child contexts, which
        are not owned: detach (or close this context) before closing a child"""
        _chk(self._L.fedd_block_prec_attach(self._h, kind, None if velocity is None else velocity._h,
                                            None if schur is None else schur._h, float(schur_scale), slot_bt))
        self._bp_children = (velocity, schur)       # keeps them alive while attached

    def block_prec_detach(self):
        _chk(self._L.fedd_block_prec_detach(self._h))
        self._bp_children = None

    def block_prec_info(self):
        k, sl, n, sc = C.c_int(), C.c_int(), C.c_int64(), C.c_double()
        _chk(self._L.fedd_block_prec_info(self._h, C.byref(k), C.byref(sc), C.byref(sl), C.byref(n)))
        return {"kind": k.value, "schur_scale": sc.value, "slot_bt": sl.value, "applies": n.value}

    def interface_match(self, other, flags):
        """this context is the fluid, `other` the structure: the nodes that carry each of `flags`, at the reference coordinates,
        ordered lexicographically and paired by rank (fedd_interface_match); returns the number of pairs"""
        fl = np.ascontiguousarray(np.atleast_1d(flags), dtype=np.int32)
        _chk(self._L.fedd_interface_match(self._h, None if other is None else other._h, fl.shape[0], _p(fl, _i32p)))
        return self.interface_match_info()["n_pairs"]

    def interface_match_table(self):
        """(iface_fluid, iface_structure, flag_ptr): owned node ids of pair k on both sides, the flags concatenated"""
        n, nf, d = C.c_int64(), C.c_int(), C.c_int()
        _chk(self._L.fedd_interface_match_sizes(self._h, C.byref(n), C.byref(nf), C.byref(d)))
        f = np.zeros(n.value, dtype=np.int32)
        s = np.zeros(n.value, dtype=np.int32)
        ptr = np.zeros(nf.value + 1, dtype=np.int64)
        _chk(self._L.fedd_interface_match_get(self._h, _p(f, _i32p), _p(s, _i32p), _p(ptr, _i64p)))
        return f, s, ptr

    def interface_match_info(self):
        h, n, d, t = C.c_int(), C.c_int64(), C.c_double(), C.c_int()
        _chk(self._L.fedd_interface_match_info(self._h, C.byref(h), C.byref(n), C.byref(d), C.byref(t)))
        return {"have": bool(h.value), "n_pairs": n.value, "max_pair_distance": d.value, "tile_points": t.value}

    def fsi_merge(self, fluid, structure, dt, coupled_mask=None):
        """this (mesh-less) context's system <- the four-block coupled system of the children's current systems and the
        coupling entries of their matched interface (fedd_fsi_merge); coupled_mask: one byte per interface dof, 0 = uncoupled"""
        m = None if coupled_mask is None else np.ascontiguousarray(coupled_mask, dtype=np.uint8)
        _chk(self._L.fedd_fsi_merge(self._h, None if fluid is None else fluid._h, None if structure is None else structure._h,
                                    float(dt), _p(m, C.POINTER(C.c_uint8))))

    def fsi_interface_rhs(self, d_old):
        """rhs_lambda <- C2 d_old on the coupled interface dofs, 0 elsewhere (fedd_fsi_interface_rhs); d_old: [n_s]"""
        d = np.ascontiguousarray(d_old, dtype=np.float64).ravel()
        n_s = self.fsi_info()["n_s"]
        if d.shape[0] != n_s:
            raise FeddError("fsi_interface_rhs: %d entries, the structure block has %d" % (d.shape[0], n_s))
        _chk(self._L.fedd_fsi_interface_rhs(self._h, _p(d, _f64p)))

    def fsi_info(self):
        a, b, c, d, lv, nv = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int(), C.c_int64()
        off = np.zeros(4, dtype=np.int64)
        _chk(self._L.fedd_fsi_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), _p(off, _i64p), C.byref(lv), C.byref(nv)))
        return {"n_u": a.value, "n_p": b.value, "n_s": c.value, "n_l": d.value, "offsets": off,
                "last_values_only": bool(lv.value), "n_values_only": nv.value}

    def fsi_prec_attach(self, fluid, structure):
        """FaCSI preconditioner of this context's coupled system out of the two child contexts, which are not owned"""
        _chk(self._L.fedd_fsi_prec_attach(self._h, None if fluid is None else fluid._h, None if structure is None else structure._h))
        self._fp_children = (fluid, structure)      # keeps them alive while attached

    def fsi_prec_detach(self):
        _chk(self._L.fedd_fsi_prec_detach(self._h))
        self._fp_children = None

    def fsi_prec_info(self):
        a, n = C.c_int(), C.c_int64()
        _chk(self._L.fedd_fsi_prec_info(self._h, C.byref(a), C.byref(n)))
        return {"attached": bool(a.value), "applies": n.value}

    def newmark_begin(self):
        """u_n <- the current solution, v = w = 0; the next advance is the first step"""
        _chk(self._L.fedd_newmark_begin(self._h))

    def newmark_set(self, u_n=None, v=None, w=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (u_n, v, w)]
        nr = self.csr_sizes()[0]
        for a in arrs:
            if a is not None and a.shape[0] != nr:
                raise FeddError("newmark_set: vector of %d entries, the system has %d rows" % (a.shape[0], nr))
        _chk(self._L.fedd_newmark_set(self._h, *[_p(a, _f64p) for a in arrs]))

    def newmark_get(self):
        """(u_n, v, w) of the Newmark state"""
        nr = self.csr_sizes()[0]
        out = [np.zeros(nr) for _ in range(3)]
        _chk(self._L.fedd_newmark_get(self._h, *[_p(a, _f64p) for a in out]))
        return tuple(out)

    def newmark_advance(self, slot_m, dt, beta, gamma, coeff=1.0):
        """updateSolutionNewmarkPreviousStep + updateNewmarkRhs: the state moves to the solved step, rhs <- coeff * M t"""
        _chk(self._L.fedd_newmark_advance(self._h, slot_m, float(dt), float(beta), float(gamma), float(coeff)))

    def multistep_begin(self, order):
        """`order` (1 or 2) zeroed history vectors of the current system's length, count = 0"""
        _chk(self._L.fedd_multistep_begin(self._h, int(order)))

    def multistep_advance(self, slot_m, coeff):
        """updateSolutionMultiPreviousStep + updateMultistepRhs: the current solution enters the history,
        rhs <- [M (coeff[0] u + coeff[1] u_0) ; 0]; coeff already divided by dt, len(coeff) = n_use"""
        cf = np.ascontiguousarray(np.atleast_1d(coeff), dtype=np.float64)
        _chk(self._L.fedd_multistep_advance(self._h, slot_m, cf.shape[0], _p(cf, _f64p)))

    def multistep_info(self):
        """(order, count): order 0 = no history"""
        o, k = C.c_int(), C.c_int()
        _chk(self._L.fedd_multistep_info(self._h, C.byref(o), C.byref(k)))
        return o.value, k.value

    def multistep_set(self, k, u_k):
        u_k = np.ascontiguousarray(u_k, dtype=np.float64)
        if self.multistep_info()[0] > 0 and u_k.shape[0] != self.csr_sizes()[0]:
            raise FeddError("multistep_set: vector of %d entries, the system has %d rows" % (u_k.shape[0], self.csr_sizes()[0]))
        _chk(self._L.fedd_multistep_set(self._h, int(k), _p(u_k, _f64p)))

    def multistep_get(self, k):
        if self.multistep_info()[0] <= 0:       # the length of the host buffer comes from the history: none, no copy
            raise FeddError("multistep_get: no multistep history (fedd_multistep_begin first; a fedd_mesh_set releases it)")
        out = np.zeros(self.csr_sizes()[0])
        _chk(self._L.fedd_multistep_get(self._h, int(k), _p(out, _f64p)))
        return out

    def stage_begin(self, max_stages):
        """opens a single-step (Runge-Kutta) step for up to max_stages (2 .. 8) stages, count = 0; the buffers are kept"""
        _chk(self._L.fedd_stage_begin(self._h, int(max_stages)))

    def stage_push(self, slot_f):
        """stage `count` <- the values of M[slot_f] and the device's current solution vector"""
        _chk(self._L.fedd_stage_push(self._h, int(slot_f)))

    def stage_info(self):
        """(max_stages, count, nnz, n): max_stages 0 = no open step; nnz and n of the first push"""
        a, b, c, d = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_stage_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def stage_rhs(self, slot_m, slot_bt, coeff_f, coeff_bt=None):
        """buildMultiStageRhs: rhs <- [M u_0 + sum_j (coeff_f[j] (F_j u_j) + coeff_bt[j] (B^T p_j)) ; 0], n_prior = len(coeff_f);
        coeff_bt None = all 0.0 ("Full implicit pressure")"""
        cf = np.ascontiguousarray(np.atleast_1d(coeff_f), dtype=np.float64)
        cb = np.zeros_like(cf) if coeff_bt is None else np.ascontiguousarray(np.atleast_1d(coeff_bt), dtype=np.float64)
        if cb.shape != cf.shape:
            raise FeddError("stage_rhs: coeff_f has %d entries, coeff_bt %d" % (cf.shape[0], cb.shape[0]))
        _chk(self._L.fedd_stage_rhs(self._h, int(slot_m), int(slot_bt), cf.shape[0], _p(cf, _f64p), _p(cb, _f64p)))

    def stage_error(self, kind, slot_m, ja, jb):
        """||U_ja - U_jb||, Euclidean over all rows or sqrt(d^T M d) over the velocity rows; -1 = the current solution"""
        e = C.c_double()
        _chk(self._L.fedd_stage_error(self._h, int(kind), int(slot_m), int(ja), int(jb), C.byref(e)))
        return e.value

    def stage_get(self, j):
        """(values of F_j, U_j) of stored stage j"""
        mx, count, nnz, n = self.stage_info()
        if not 0 <= j < count:      # the lengths of the host buffers come from the store: no such stage, no copy
            raise FeddError("stage_get: stage %d of %d (fedd_stage_push first; a fedd_mesh_set releases the stage store)" % (j, count))
        val, u = np.zeros(nnz), np.zeros(n)
        _chk(self._L.fedd_stage_get(self._h, int(j), _p(val, _f64p), _p(u, _f64p)))
        return val, u

    def block_merge_scaled(self, slot_a, slot_bt, s_bt, slot_b, slot_c=-1):
        """block_merge with every B^T value multiplied by s_bt on its way into the merged matrix"""
        _chk(self._L.fedd_block_merge_scaled(self._h, slot_a, slot_bt, float(s_bt), slot_b, slot_c))
        self.dofs = 1

    def rhs_axpy(self, alpha, f):
        f = np.ascontiguousarray(f, dtype=np.float64)
        if f.shape[0] != self.csr_sizes()[0]:
            raise FeddError("rhs_axpy: vector length differs from the system's rows")
        _chk(self._L.fedd_rhs_axpy(self._h, float(alpha), _p(f, _f64p)))

    def solution_set(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape[0] != self.csr_sizes()[0]:
            raise FeddError("solution_set: vector length differs from the system's rows")
        _chk(self._L.fedd_solution_set(self._h, _p(x, _f64p)))

    def dirichlet_rhs(self, flags, values=None, comp_mask=None):
        """the right-hand-side half of dirichlet(): the rows are unit rows already, the matrix is not touched"""
        fl = np.ascontiguousarray(flags, dtype=np.int32)
        n = fl.shape[0]
        v = np.zeros(n * self.dofs) if values is None else np.ascontiguousarray(values, dtype=np.float64).ravel()
        m = None if comp_mask is None else np.ascontiguousarray(comp_mask, dtype=np.int32).ravel()
        _chk(self._L.fedd_dirichlet_rhs(self._h, n, _p(fl, _i32p), _p(m, _i32p), _p(v, _f64p)))

    def csr_sizes(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_csr_sizes(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def csr_get(self):
        nr, nc, nnz = self.csr_sizes()
        rowptr = np.zeros(nr + 1, dtype=np.int64)
        col = np.zeros(nnz, dtype=np.int32)
        val = np.zeros(nnz, dtype=np.float64)
        gid = np.zeros(nc, dtype=np.int64)
        _chk(self._L.fedd_csr_get(self._h, _p(rowptr, _i64p), _p(col, _i32p), _p(val, _f64p), _p(gid, _i64p)))
        return rowptr, col, val, gid

    def rhs_get(self):
        nr = self.csr_sizes()[0]
        out = np.zeros(nr)
        _chk(self._L.fedd_rhs_get(self._h, _p(out, _f64p)))
        return out

    def rhs_set(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64)
        _chk(self._L.fedd_rhs_set(self._h, _p(b, _f64p)))

    def solution_get(self):
        nr = self.csr_sizes()[0]
        out = np.zeros(nr)
        _chk(self._L.fedd_solution_get(self._h, _p(out, _f64p)))
        return out

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        _chk(self._L.fedd_spmv(self._h, _p(x, _f64p), _p(y, _f64p)))
        return y

    def spmv_info(self):
        a, b = C.c_int64(), C.c_int64()
        _chk(self._L.fedd_spmv_info(self._h, C.byref(a), C.byref(b)))
        p, e = C.c_int64(), C.c_int64()
        _chk(self._L.fedd_spmv_patterns(self._h, C.byref(p), C.byref(e)))
        cb, wide = C.c_int(), C.c_int64()
        _chk(self._L.fedd_spmv_col_bytes(self._h, C.byref(cb), C.byref(wide)))
        nc, rc, rest = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_spmv_classes(self._h, C.byref(nc), C.byref(rc), C.byref(rest)))
        bl, bf = C.c_int64(), C.c_int64()
        _chk(self._L.fedd_spmv_cls_blocks(self._h, C.byref(bl), C.byref(bf)))
        return dict(nnz_pattern=a.value, nnz_streamed=b.value, column_patterns=p.value, rows_with_explicit_columns=e.value,
                    column_index_bytes=cb.value, entries_with_32bit_columns=wide.value, row_classes=nc.value,
                    rows_in_classes=rc.value, nnz_streamed_outside_classes=rest.value, class_blocks_lds=bl.value,
                    class_blocks_fallback=bf.value)

    def spmv_device(self, reps):
        _chk(self._L.fedd_spmv_device(self._h, reps))

    def schwarz_set_target(self, target, scale=1.0):
        _chk(self._L.fedd_schwarz_set_target(self._h, target, scale))

    def schwarz_setup(self, overlap=1, combine=COMBINE_RESTRICTED, two_level=0, coarse_kind=0):
        _chk(self._L.fedd_schwarz_setup(self._h, overlap, combine, two_level, coarse_kind))

    def schwarz_set_coarse(self, cells_target):
        _chk(self._L.fedd_schwarz_set_coarse(self._h, float(cells_target)))

    def schwarz_set_level_combination(self, combination):
        """LEVELS_ADDITIVE (default) or LEVELS_MULTIPLICATIVE: z = (I - Pc A) M1^-1 r, read at apply time"""
        _chk(self._L.fedd_schwarz_set_level_combination(self._h, int(combination)))

    def schwarz_get_level_combination(self):
        k = C.c_int()
        _chk(self._L.fedd_schwarz_get_level_combination(self._h, C.byref(k)))
        return k.value

    def schwarz_coarse_sizes(self):
        g = np.zeros(3, dtype=np.int32)
        n0 = C.c_int64()
        _chk(self._L.fedd_schwarz_coarse_sizes(self._h, _p(g, _i32p), C.byref(n0)))
        return g, n0.value

    def schwarz_coarse(self):
        """(cells per direction, K0^-1) of the coarse level"""
        g = np.zeros(3, dtype=np.int32)
        n0 = C.c_int64()
        _chk(self._L.fedd_schwarz_coarse_sizes(self._h, _p(g, _i32p), C.byref(n0)))
        K = np.empty((n0.value, n0.value), dtype=np.float64)
        _chk(self._L.fedd_schwarz_coarse_get(self._h, _p(K, _f64p)))
        return g, K

    def schwarz_info(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_schwarz_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        u = C.c_int64()
        _chk(self._L.fedd_schwarz_unique(self._h, C.byref(u)))
        out = dict(n_subdomains=a.value, max_size=b.value, inverse_bytes=c.value, n_unique=u.value)
        if a.value and b.value <= 256:      # (the large-subdomain path keeps no per-box lists)
            ss, so = C.c_int64(), C.c_int64()
            if self._L.fedd_schwarz_sizes(self._h, C.byref(ss), C.byref(so)) == 0:
                out.update(sum_sizes=ss.value, sum_owned=so.value)
            nc = C.c_int64()
            if self._L.fedd_schwarz_conforming(self._h, C.byref(nc)) == 0:
                out.update(n_conforming=nc.value)
        return out

    def schwarz_reuse_info(self):
        """whether the last schwarz_setup kept the box structure of the one before, and how many setups of this context have"""
        a, n = C.c_int(), C.c_int64()
        _chk(self._L.fedd_schwarz_reuse_info(self._h, C.byref(a), C.byref(n)))
        return {"last_reused": bool(a.value), "n_reused": n.value}

    def pattern_reuse_info(self):
        """whether the last pattern_build kept the pattern arrays of the one before, and how many builds of this context have"""
        a, n = C.c_int(), C.c_int64()
        _chk(self._L.fedd_pattern_reuse_info(self._h, C.byref(a), C.byref(n)))
        return {"last_reused": bool(a.value), "n_reused": n.value}

    def setup_fused_info(self):
        """what option "setup_fused" has done on this context (fedd_setup_fused_info)"""
        a, b, d = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_setup_fused_info(self._h, C.byref(a), C.byref(b), C.byref(d)))
        return {"n_walks": a.value, "n_checks_used": b.value, "n_absdet_kept": d.value}

    def spmv_reuse_info(self):
        """whether the solver's SpMV stream in use was kept from the matrix before (verified, not built), and how often it was"""
        a, n = C.c_int(), C.c_int64()
        _chk(self._L.fedd_spmv_reuse_info(self._h, C.byref(a), C.byref(n)))
        return {"last_reused": bool(a.value), "n_reused": n.value}

    def schwarz_apply(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        _chk(self._L.fedd_schwarz_apply(self._h, _p(r, _f64p), _p(z, _f64p)))
        return z

    def schwarz_apply_device(self, reps):
        _chk(self._L.fedd_schwarz_apply_device(self._h, reps))

    def gmres(self, b=None, rtol=1e-8, max_it=100, restart=100, use_prec=True, want_x=True):
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        nr = self.csr_sizes()[0]
        x = np.zeros(nr) if want_x else None
        its, rel = C.c_int(), C.c_double()
        _chk(self._L.fedd_gmres(self._h, _p(bb, _f64p), _p(x, _f64p), rtol, max_it, restart, int(use_prec),
                                C.byref(its), C.byref(rel)))
        return x, its.value, rel.value

    def gmres_x0(self, x0=None, b=None, rtol=1e-8, max_it=100, restart=100, use_prec=True):
        """the solve from an initial guess ("Zero Initial Guess" = false); x0 None: from the vector the device holds"""
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        x = None if x0 is None else np.array(x0, dtype=np.float64, copy=True)
        its, rel = C.c_int(), C.c_double()
        _chk(self._L.fedd_gmres_x0(self._h, _p(bb, _f64p), _p(x, _f64p), rtol, max_it, restart, int(use_prec),
                                   C.byref(its), C.byref(rel)))
        return (x if x is not None else self.solution_get()), its.value, rel.value

    def cg(self, b=None, rtol=1e-8, max_it=1000, use_prec=True, want_x=True):
        """preconditioned CG (symmetric positive definite systems; the preconditioner needs COMBINE_FULL)"""
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        nr = self.csr_sizes()[0]
        x = np.zeros(nr) if want_x else None
        its, rel = C.c_int(), C.c_double()
        _chk(self._L.fedd_cg(self._h, _p(bb, _f64p), _p(x, _f64p), rtol, max_it, int(use_prec), C.byref(its), C.byref(rel)))
        return x, its.value, rel.value

    def cg_x0(self, x0=None, b=None, rtol=1e-8, max_it=1000, use_prec=True):
        """CG from an initial guess; x0 None: from the vector the device holds"""
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        x = None if x0 is None else np.array(x0, dtype=np.float64, copy=True)
        its, rel = C.c_int(), C.c_double()
        _chk(self._L.fedd_cg_x0(self._h, _p(bb, _f64p), _p(x, _f64p), rtol, max_it, int(use_prec), C.byref(its), C.byref(rel)))
        return (x if x is not None else self.solution_get()), its.value, rel.value

    def cg_info(self):
        a, b = C.c_int(), C.c_int()
        _chk(self._L.fedd_cg_info(self._h, C.byref(a), C.byref(b)))
        return {"replacements": a.value, "breakdown": b.value}

    def schwarz_full_info(self):
        """subdomains the symmetric apply parks on the matrix cores / with the one-workgroup kernel"""
        a, b = C.c_int64(), C.c_int64()
        _chk(self._L.fedd_schwarz_full_info(self._h, C.byref(a), C.byref(b)))
        return {"n_mfma": a.value, "n_plain": b.value}

    def mesh_setup_info(self):
        a, t, st, nt = C.c_double(), C.c_double(), C.c_int(), C.c_int64()
        _chk(self._L.fedd_mesh_setup_info(self._h, C.byref(a), C.byref(t), C.byref(st), C.byref(nt)))
        return {"adjacency_ms": a.value, "tiles_ms": t.value, "tiles_state": st.value, "n_tiles": nt.value}

    def gmres_status(self):
        fl, rr = C.c_int(), C.c_double()
        _chk(self._L.fedd_gmres_status(self._h, C.byref(fl), C.byref(rr)))
        return {"floor_reached": fl.value, "recurrence_relres": rr.value}

    def schwarz_coarse_apply(self, r=None):
        """z = Phi K0^-1 Phi^T r (FROSch's "Only apply coarse"); r None: the assembled rhs, z stays on the device as the
        solution vector (Level Combination = Multiplicative: then gmres_x0(None))"""
        if r is None:
            _chk(self._L.fedd_schwarz_coarse_apply(self._h, None, None))
            return None
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        _chk(self._L.fedd_schwarz_coarse_apply(self._h, _p(r, _f64p), _p(z, _f64p)))
        return z

    def set_option(self, key, value):
        _chk(self._L.fedd_set_option(self._h, key.encode(), float(value)))

    def timing_enable(self, on=True):
        _chk(self._L.fedd_timing_enable(self._h, int(on)))

    def timing_reset(self):
        _chk(self._L.fedd_timing_reset(self._h))

    def timing_get(self):
        out = {}
        for i, name in enumerate(TIMER_NAMES):
            ms, n = C.c_double(), C.c_int64()
            _chk(self._L.fedd_timing_get(self._h, i, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def timing_get_sampled(self):
        """per class: (device ms, launches, algorithmic bytes) of the launches that were actually timed"""
        out = {}
        for i, name in enumerate(TIMER_NAMES):
            ms, n, b = C.c_double(), C.c_int64(), C.c_double()
            _chk(self._L.fedd_timing_get_sampled(self._h, i, C.byref(ms), C.byref(n), C.byref(b)))
            out[name] = (ms.value, n.value, b.value)
        return out

    def gmres_info(self):
        k, s, nb, nc, nf = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _chk(self._L.fedd_gmres_info(self._h, C.byref(k), C.byref(s), C.byref(nb), C.byref(nc)))
        _chk(self._L.fedd_gmres_fused_blocks(self._h, C.byref(nf)))
        return {"kind": k.value, "s": s.value, "blocks": nb.value, "cut_blocks": nc.value, "fused_blocks": nf.value}

    CAPTURE_PIECES = ("V0", "C0", "P1", "CF1", "RI1", "SA1", "W1", "P2", "CF2", "RI2", "SA2", "TH", "W2", "H", "VEND")

    def gmres_capture_arm(self, block):
        """copy the block-th orthogonalised block of the next s-step solve stage by stage (block < 0: disarm, free the copies)"""
        if int(block) != block:
            raise ValueError("gmres_capture_arm: block must be an integer, got %r" % (block,))
        _chk(self._L.fedd_gmres_capture_arm(self._h, int(block)))

    def gmres_capture_info(self):
        v = np.zeros(8, dtype=np.int64)
        _chk(self._L.fedd_gmres_capture_info(self._h, _p(v, _i64p)))
        names = ("captured", "n", "ldv", "k", "sa_req", "S", "m", "fused")
        return {k: int(x) for k, x in zip(names, v)}

    def gmres_capture_get(self, what, cap=None):
        """one piece of the captured block, shaped: basis pieces (ldv, columns) column-major, coefficient pieces (rows, S),
        H (m + 1, columns) column-major, SA1 / SA2 / TH flat.  cap: doubles to make room for (default: what the piece takes)"""
        if what not in self.CAPTURE_PIECES:
            raise ValueError("gmres_capture_get: no piece is named %r (pieces: %s)" % (what, " ".join(self.CAPTURE_PIECES)))
        i = self.gmres_capture_info()
        k, sa, S, ldv, m = i["k"], i["sa_req"], i["S"], i["ldv"], i["m"]
        can = 1 if k + sa <= m else 0
        sa2 = 0
        if what in ("H", "VEND") and i["captured"]:
            sa2 = int(self.gmres_capture_get("SA2")[0])
        shape = {"V0": (k + sa, ldv), "C0": (1, ldv), "P1": (k + sa, S), "P2": (k + sa, S), "CF1": (k, S), "CF2": (k, S),
                 "RI1": (S, S), "RI2": (S, S), "SA1": (1,), "SA2": (2,), "TH": (S,), "W1": (sa + can, ldv), "W2": (sa + can, ldv),
                 "H": (k - 1 + max(sa2, 1), m + 1), "VEND": (k + sa2, ldv)}[what]
        out = np.zeros(max(int(np.prod(shape)) if cap is None else int(cap), 1))
        _chk(self._L.fedd_gmres_capture_get(self._h, what.encode(), _p(out, _f64p), out.shape[0] if cap is None else int(cap)))
        out = out[:int(np.prod(shape))].reshape(shape)
        return out.T if what in ("V0", "C0", "W1", "W2", "H", "VEND") else out

    def read_bandwidth(self, nbytes=2 << 30, reps=10):
        """GB/s of a read-only stream on this GPU (roofline calibration)."""
        g = C.c_double()
        _chk(self._L.fedd_read_bandwidth(self._h, int(nbytes), reps, C.byref(g)))
        return g.value

    # ---- halo plan ----
    def halo_set_owners(self, gid_rep, owner_rep):
        g = np.ascontiguousarray(gid_rep, dtype=np.int64)
        o = np.ascontiguousarray(owner_rep, dtype=np.int32)
        _chk(self._L.fedd_halo_set_owners(self._h, g.shape[0], _p(g, _i64p), _p(o, _i32p)))

    def halo_requests(self):
        cnt = np.zeros(self.nranks, dtype=np.int64)
        _chk(self._L.fedd_halo_requests_sizes(self._h, _p(cnt, _i64p)))
        g = np.zeros(int(cnt.sum()), dtype=np.int64)
        _chk(self._L.fedd_halo_requests_get(self._h, _p(g, _i64p)))
        return cnt, g

    def halo_requests_set(self, count_from_rank, gids):
        cnt = np.ascontiguousarray(count_from_rank, dtype=np.int64)
        g = np.ascontiguousarray(gids, dtype=np.int64)
        _chk(self._L.fedd_halo_requests_set(self._h, _p(cnt, _i64p), _p(g, _i64p)))

    def comm_set_torch_dist(self, dist):
        """Host-staged transport over an initialised torch.distributed group (gloo): functional
        tests of the N > 1 path where RCCL cannot run.  Also finalises the halo plan over it."""
        import torch

        def exchange(user, n_peers, peers, send_ptr, send_buf, recv_ptr, recv_buf, dofs):
            try:
                reqs, keep = [], []
                for k in range(n_peers):
                    s0, s1 = send_ptr[k] * dofs, send_ptr[k + 1] * dofs
                    r0, r1 = recv_ptr[k] * dofs, recv_ptr[k + 1] * dofs
                    if s1 > s0:
                        t = torch.from_numpy(np.ctypeslib.as_array(send_buf, shape=(send_ptr[n_peers] * dofs,))[s0:s1].copy())
                        keep.append(t)
                        reqs.append(dist.isend(t, int(peers[k])))
                    if r1 > r0:
                        t = torch.zeros(r1 - r0, dtype=torch.float64)
                        keep.append((t, r0, r1))
                        reqs.append(dist.irecv(t, int(peers[k])))
                for r in reqs:
                    r.wait()
                out = np.ctypeslib.as_array(recv_buf, shape=(max(1, recv_ptr[n_peers] * dofs),))
                for item in keep:
                    if isinstance(item, tuple):
                        out[item[1]:item[2]] = item[0].numpy()
                return 0
            except Exception as e:  # pragma: no cover
                print("exchange callback failed:", e, flush=True)
                return 1

        def allreduce(user, buf, n):
            try:
                a = np.ctypeslib.as_array(buf, shape=(n,))
                t = torch.from_numpy(a.copy())
                dist.all_reduce(t)
                a[:] = t.numpy()
                return 0
            except Exception as e:  # pragma: no cover
                print("allreduce callback failed:", e, flush=True)
                return 1

        self._cb = (EXCHANGE_FN(exchange), ALLREDUCE_FN(allreduce))     # keep alive
        _chk(self._L.fedd_comm_set_host_callbacks(self._h, C.cast(self._cb[0], C.c_void_p), C.cast(self._cb[1], C.c_void_p), None))
        # halo plan over the same group
        cnt, gids = self.halo_requests()
        world = self.nranks
        cnt_all = [torch.zeros(world, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(cnt_all, torch.from_numpy(cnt.copy()))
        from_me = np.array([int(cnt_all[p][self.rank]) for p in range(world)], dtype=np.int64)
        recv = [torch.zeros(int(n), dtype=torch.int64) for n in from_me]
        off = np.concatenate([[0], np.cumsum(cnt)])
        reqs = []
        for p in range(world):
            if p == self.rank:
                continue
            if cnt[p] > 0:
                reqs.append(dist.isend(torch.from_numpy(gids[off[p]:off[p + 1]].copy()), p))
            if from_me[p] > 0:
                reqs.append(dist.irecv(recv[p], p))
        for r in reqs:
            r.wait()
        self.halo_requests_set(from_me, np.concatenate([t.numpy() for t in recv]) if from_me.sum() else np.zeros(0, np.int64))

    def comm_set_thread_group(self, group):
        """Host-staged transport between the threads of a `ThreadGroup` (see there); finalises the halo
        plan over it.  Sums of the all-reduce are formed in rank order on every rank (same bits everywhere)."""
        rank = self.rank

        def exchange(user, n_peers, peers, send_ptr, send_buf, recv_ptr, recv_buf, dofs):
            try:
                if n_peers == 0:
                    return 0
                sb = np.ctypeslib.as_array(send_buf, shape=(max(1, send_ptr[n_peers] * dofs),))
                out = np.ctypeslib.as_array(recv_buf, shape=(max(1, recv_ptr[n_peers] * dofs),))
                for k in range(n_peers):
                    s0, s1 = send_ptr[k] * dofs, send_ptr[k + 1] * dofs
                    if s1 > s0:
                        group.send(rank, int(peers[k]), sb[s0:s1])
                for k in range(n_peers):
                    r0, r1 = recv_ptr[k] * dofs, recv_ptr[k + 1] * dofs
                    if r1 > r0:
                        out[r0:r1] = group.recv(int(peers[k]), rank)
                return 0
            except Exception as e:  # pragma: no cover
                print("exchange callback failed:", repr(e), flush=True)
                return 1

        def allreduce(user, buf, n):
            try:
                a = np.ctypeslib.as_array(buf, shape=(n,))
                parts = group.allgather(rank, a.copy())
                tot = parts[0].copy()
                for q in parts[1:]:
                    tot += q
                a[:] = tot
                return 0
            except Exception as e:  # pragma: no cover
                print("allreduce callback failed:", repr(e), flush=True)
                return 1

        self._cb = (EXCHANGE_FN(exchange), ALLREDUCE_FN(allreduce))     # keep alive
        _chk(self._L.fedd_comm_set_host_callbacks(self._h, C.cast(self._cb[0], C.c_void_p), C.cast(self._cb[1], C.c_void_p), None))
        cnt, gids = self.halo_requests()
        off = np.concatenate([[0], np.cumsum(cnt)])
        everyone = group.allgather(rank, (cnt.copy(), gids.copy(), off))
        from_me = np.array([int(everyone[p][0][rank]) for p in range(group.world)], dtype=np.int64)
        lists = [everyone[p][1][everyone[p][2][rank]:everyone[p][2][rank + 1]] for p in range(group.world)]
        self.halo_requests_set(from_me, np.concatenate(lists).astype(np.int64) if from_me.sum() else np.zeros(0, np.int64))

    def rccl_selftest(self, n=4096):
        e = C.c_double()
        _chk(self._L.fedd_rccl_selftest(self._h, n, C.byref(e)))
        return e.value

    def comm_selftest(self, n=4096):
        """the solver's collectives on this context's own communicator (every rank calls it); largest deviation"""
        e = C.c_double()
        _chk(self._L.fedd_comm_selftest(self._h, n, C.byref(e)))
        return e.value

    def halo_exchange_setup(self):
        _chk(self._L.fedd_halo_exchange_setup(self._h))

    def halo_plan(self):
        npeers, ns, nr = C.c_int(), C.c_int64(), C.c_int64()
        _chk(self._L.fedd_halo_plan_sizes(self._h, C.byref(npeers), C.byref(ns), C.byref(nr)))
        peers = np.zeros(npeers.value, dtype=np.int32)
        sp = np.zeros(npeers.value + 1, dtype=np.int64)
        rp = np.zeros(npeers.value + 1, dtype=np.int64)
        sl = np.zeros(ns.value, dtype=np.int32)
        rl = np.zeros(nr.value, dtype=np.int32)
        _chk(self._L.fedd_halo_plan_get(self._h, _p(peers, _i32p), _p(sp, _i64p), _p(sl, _i32p), _p(rp, _i64p),
                                        _p(rl, _i32p)))
        return dict(peers=peers, send_ptr=sp, send_lid=sl, recv_ptr=rp, recv_lid=rl)
