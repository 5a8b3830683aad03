/* fedd_hip.h -- C ABI of the MI355X (gfx950) FE-assembly + Schwarz/GMRES hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ / torch / Trilinos types.
 * Every entry point names the reference interface (path:line under /root/reference) whose work
 * it replaces.  Conventions:
 *   - all functions return 0 on success, non-zero on failure; fedd_last_error() gives the message
 *     (the reference throws std::logic_error / std::runtime_error via TEUCHOS_TEST_FOR_EXCEPTION);
 *   - the caller owns every host buffer; the library owns device memory behind fedd_ctx;
 *   - one fedd_ctx per GPU / rank, not thread-safe per handle;
 *   - scalar = double, local ordinal = int32_t, global ordinal = int64_t
 *     (feddlib/core/General/DefaultTypeDefs.hpp:6-15).
 *   - vector fields are node-wise interleaved: dof = dofs_per_node*node + d
 *     (feddlib/core/LinearAlgebra/Map_def.hpp:101-104).
 * Problem classes covered: Laplace, LinElas, Stokes (fedd_assemble, fedd_assemble_div, fedd_block_merge) and the matrices of
 * steady Navier-Stokes that change with the velocity (fedd_velocity_set, fedd_assemble_advection).
 */
#ifndef FEDD_HIP_H
#define FEDD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fedd_ctx fedd_ctx;

/* ---- forms understood by fedd_assemble (feddlib/core/FE/FE_decl.hpp:130-257) ---- */
enum fedd_form {
    FEDD_FORM_LAPLACE     = 0, /* FE::assemblyLaplace          FE_def.hpp:604-667   (dofs 1)          */
    FEDD_FORM_LAPLACE_VEC = 1, /* FE::assemblyLaplaceVecField  FE_def.hpp:670-734   (dofs dim, diag)  */
    FEDD_FORM_MASS        = 2, /* FE::assemblyMass "Scalar"    FE_def.hpp:454-524   (dofs 1)          */
    FEDD_FORM_MASS_VEC    = 3, /* FE::assemblyMass "Vector"    FE_def.hpp:454-524   (dofs dim, diag)  */
    FEDD_FORM_LINELAS     = 4, /* FE::assemblyLinElasXDim      FE_def.hpp:2739-3040 (dofs dim, full);
                                  params = {lambda, mu}                                              */
    FEDD_FORM_BDSTAB      = 5, /* FE::assemblyBDStabilization  FE_def.hpp:2151-2220 (dofs 1, P1 only): the Bochev-Dohrmann
                                  pressure block of P1/P1 Stokes, C_ij = |det B| (sum_q w_q phi_i phi_j - |ref| scale),
                                  scaled by -1/viscosity by the caller (Stokes_def.hpp:98-105)        */
    FEDD_FORM_STRESS      = 6, /* FE::assemblyStress           FE_def.hpp:2407-2733 (dofs dim, full): the velocity block in
                                  stress form with c = 1; fedd_assemble_stress takes a coefficient     */
    FEDD_FORM_LAPLACE_XDIM = 7 /* FE::assemblyLaplaceXDim      FE_def.hpp:2225-2402 (dofs dim, diag): the vector Laplacian with
                                  one coefficient per element from the interface distances; params = {distance, coefficient}
                                  (section "Interface distances")                                       */
};

/* ---- what fedd_assemble_advection builds from the velocity of fedd_velocity_set ---- */
enum fedd_advection {
    FEDD_ADV_N      = 0,       /* FE::assemblyAdvectionVecField     FE_def.hpp:1759-1832: n_ij = |det B| sum_q w_q (u_h . grad phi_j) phi_i
                                  on the dim pairs (dim*i+d, dim*j+d) -- the fixed-point linearisation                       */
    FEDD_ADV_W      = 1,       /* FE::assemblyAdvectionInUVecField  FE_def.hpp:1839-1925: (dim*i+d1, dim*j+d2) =
                                  |det B| sum_q w_q (d u_d1 / d x_d2) phi_i phi_j                                            */
    FEDD_ADV_NEWTON = 2        /* N + W, both from one pass over the elements -- the Newton linearisation                   */
};

/* ---- what fedd_assemble_advection_ale builds from that velocity u and the mesh velocity w of fedd_mesh_velocity_* ---- */
enum fedd_advection_ale {
    FEDD_ALE_P          = 0,   /* FE::assemblyAdditionalConvection  FE_def.hpp:3044-3255: p_ij = |det B| sum_q w_q (div w_h) phi_i phi_j
                                  on the dim pairs (dim*i+d, dim*j+d), sign as the reference returns it; needs no u          */
    FEDD_ALE_FIXEDPOINT = 1,   /* N(u - w) - P(w): the velocity block of NavierStokes::reAssembleFSI                         */
    FEDD_ALE_NEWTON     = 2    /* N(u - w) + W(u) - P(w): W sees u, not u - w                                                */
};

/* ---- how the dofs of a node couple in the CSR pattern ---- */
enum fedd_block_mode {
    FEDD_BLOCK_SCALAR = 0,     /* dofs_per_node == 1                                                  */
    FEDD_BLOCK_DIAG   = 1,     /* (dim*i+d, dim*j+d) only        -- what assemblyLaplaceVecField inserts */
    FEDD_BLOCK_FULL   = 2      /* every (a,b) pair                -- what assemblyLinElasXDim inserts    */
};

enum fedd_combine {            /* FROSch "Combine Values in Overlap" (laplace/parametersPrec.xml:31)    */
    FEDD_COMBINE_RESTRICTED = 0,
    FEDD_COMBINE_AVERAGING  = 1,
    FEDD_COMBINE_FULL       = 2
};

/* kernel classes whose device time the library accumulates with HIP events when timing is on */
enum fedd_timer {
    FEDD_T_SYMBOLIC = 0,  /* adjacency + CSR pattern                           */
    FEDD_T_ASSEMBLE = 1,  /* matrix gather-assembly kernel                     */
    FEDD_T_RHS      = 2,
    FEDD_T_DIRICHLET= 3,
    FEDD_T_SPMV     = 4,
    FEDD_T_SCHWARZ_SETUP = 5,
    FEDD_T_SCHWARZ_APPLY = 6,
    FEDD_T_ORTHO    = 7,  /* GMRES multi-dot / multi-axpy kernels              */
    FEDD_T_COARSE_SETUP = 8,  /* second level: Galerkin product + dense inverse */
    FEDD_T_COARSE_APPLY = 9,  /* second level: restrict, K0^-1, prolongate      */
    FEDD_T_HALO     = 10, /* ghost import: pack, send / receive, unpack (several ranks)  */
    FEDD_T_ALLREDUCE= 11, /* all-reduce calls (inside the classes that issue them)        */
    FEDD_T_SPMV_SETUP = 12, /* compaction of the solver's SpMV stream (once per assembled matrix) */
    FEDD_T_GS_DOT   = 13, /* Gram-Schmidt sweep 1 alone: the multi-dot kernel over the Krylov basis (inside ORTHO)   */
    FEDD_T_GS_UPDATE= 14, /* Gram-Schmidt sweep 2 alone: the multi-axpy kernel over the Krylov basis (inside ORTHO)  */
    FEDD_T_GS_FUSED = 15, /* s-step solver: first update and second dot of a block in one sweep, k_blockfuse (inside ORTHO) */
    FEDD_T_FULL_PARK_MFMA = 16, /* symmetric Schwarz apply: k_full_park_mfma (inside SCHWARZ_APPLY) */
    FEDD_T_FULL_PARK = 17,      /* ... k_full_park                                       */
    FEDD_T_FULL_GATHER = 18,    /* ... k_full_gather                                     */
    FEDD_T_CG_PQ    = 19, /* CG sweeps: k_cg_pq                                */
    FEDD_T_CG_XR    = 20, /* ... k_cg_xr                                       */
    FEDD_T_CG_RZ    = 21, /* ... k_cg_rz                                       */
    FEDD_T_CG_P     = 22, /* ... k_cg_p                                        */
    FEDD_T_NEWMARK  = 23, /* Newmark state update: k_newmark (timestep.hip)             */
    FEDD_T_BLOCK_APPLY = 24, /* y = alpha M x on a stored block: k_block_apply          */
    FEDD_T_MULTISTEP = 25, /* BDF history update: k_multistep (timestep.hip)              */
    FEDD_T_BLOCKPREC_BT = 26, /* Triangular block preconditioner: t = r_u - B^T z_p, k_bt_sub (blockprec.hip) */
    FEDD_T_NEWTON_RESIDUAL = 27, /* Newton residual of a Newmark step: k_newton_residual (newton.hip) */
    FEDD_T_NEWTON_UPDATE = 28,   /* ... the iterate's update: k_newton_update                      */
    FEDD_T_MESH_MOVE = 29,  /* fedd_mesh_move: k_mesh_move, candidate = x_ref + d (mesh_move.hip)  */
    FEDD_T_MOVE_CHECK = 30, /* ... k_move_check + k_move_min, det B of every element against the reference */
    FEDD_T_INTERFACE_DIST = 31, /* fedd_interface_distance*: k_interface_distance (interface_distance.hip) */
    FEDD_T_FSI_MATCH = 32,  /* fedd_interface_match: k_iface_rank + k_iface_scatter (fsi.hip)            */
    FEDD_T_FSI_MERGE = 33,  /* fedd_fsi_merge: count / fill / values kernels of the four-block system     */
    FEDD_T_FSI_APPLY = 34,  /* FaCSI apply: k_facsi_inject + k_facsi_rows (the children's applies are SCHWARZ_APPLY of theirs) */
    FEDD_T_COUNT    = 35
};

/* ------------------------------------------------------------------------------------------------
 * context  (replaces the per-rank Teuchos::Comm + Tpetra node the reference gets from
 * Xpetra::DefaultPlatform, feddlib/problems/tests/laplace/main.cpp:60-62)
 * nccl_unique_id: NULL for a single rank; else the 128-byte ncclUniqueId shared by all ranks.
 * ---------------------------------------------------------------------------------------------- */
/* (the environment variable FEDD_OPTIONS=key=value,... is applied to every new context through fedd_set_option) */
int  fedd_ctx_create(fedd_ctx** out, int device, const void* nccl_unique_id, int rank, int nranks);
void fedd_ctx_destroy(fedd_ctx* ctx);
const char* fedd_last_error(void);
int  fedd_sync(fedd_ctx* ctx);                       /* hipStreamSynchronize on the context's stream (and on the streams of
                                                        the children of an attached block preconditioner) */
int  fedd_nccl_unique_id(void* id128);               /* rank 0 calls this, then shares the 128 bytes */

/* ------------------------------------------------------------------------------------------------
 * structured mesh generator, host side
 * replaces MeshStructured::buildMesh2D/3D P1 branch + setStructuredMeshFlags + Map::buildUniqueMap
 * (feddlib/core/Mesh/MeshStructured_def.hpp:348-463, 703-806, 2974-3203;
 *  feddlib/core/LinearAlgebra/Map_def.hpp:184-210) as sequenced by Domain::buildMesh
 * (feddlib/core/FE/Domain_def.hpp:201-265).
 * decomp[3] = blocks per direction (the reference supports only N x N x N; {N,N,N} reproduces it
 * exactly, other shapes are the 1x1x2 / 1x2x2 splits of the same global grid used for the 2- and
 * 4-GPU scaling points).  cells[3] = cells per block and direction (the reference's M).
 * with_ghost_elements = 1 appends the neighbour blocks' elements that touch an owned node (and
 * their nodes), so that every owned row can be assembled without a matrix exchange.
 * with_ghost_elements = L >= 2 (at most 8) appends L layers of elements around the owned nodes on every
 * side with a neighbour, so that the rows of the ghost nodes within L - 1 layers are complete on this rank
 * too (row ghosts, see fedd_mesh_set_rows; what FROSch obtains by importing the overlapping matrix rows
 * from their owners).  fedd_mesh_structured_row_ghosts lists them (count with NULL arrays first).
 * L = 2 gives the Schwarz subdomains at a rank boundary true overlap rows; L = 4 (27-node boxes, overlap 1)
 * lets every rank build whole every box that holds one of its nodes, see fedd_schwarz_setup.
 * ---------------------------------------------------------------------------------------------- */
int fedd_mesh_structured_sizes(int dim, const int* decomp, const int* cells, int rank,
                               int with_ghost_elements,
                               int64_t* n_elem, int64_t* n_rep, int64_t* n_uni, int64_t* n_global);
int fedd_mesh_structured_build(int dim, const int* decomp, const int* cells, int rank,
                               const double* origin, const double* size, int flags_option,
                               int with_ghost_elements,
                               int32_t* conn /*[n_elem*(dim+1)] local repeated ids*/,
                               double* xyz /*[n_rep*dim]*/, int64_t* gid_rep /*[n_rep]*/,
                               int32_t* flag_rep /*[n_rep]*/,
                               int64_t* gid_uni /*[n_uni]*/, int32_t* flag_uni /*[n_uni]*/);
int fedd_mesh_structured_row_ghosts(int dim, const int* decomp, const int* cells, int rank, int with_ghost_elements,
                                    const double* origin, const double* size, int flags_option,
                                    int64_t* n_row_ghosts, int64_t* gid /*nullable*/, int32_t* flag /*nullable*/);

/* ------------------------------------------------------------------------------------------------
 * structured P2 mesh generator, host side: the rank-local mesh of the reference, no ghost layers
 * replaces MeshStructured::buildMesh2D/3D P2 branch (MeshStructured_def.hpp:468-619, 808-994: 6-node triangles,
 * 10-node tetrahedra, six per cell) + setStructuredMeshFlags as it acts on P2 meshes (:2984-3011, :3137-3202)
 * + Map::buildUniqueMap (Map_def.hpp:184-210, lowest-rank owner as in the P1 generator), on the unit square / cube.
 *   local ids      r + s*(2M+1) + t*(2M+1)^2 on the block's lattice; element order and node slots are the reference's:
 *                  vertices, then the mid nodes of (0,1),(1,2),(0,2)[,(0,3),(1,3),(2,3)]
 *   global ids     r + s*n1 + t*n1^2, n1 = 2*N*M + 1, plus the rank offsets of :504 / :849-850
 *   coordinates    r*h/2 + offset*H, snapped to 0.0 below 100 eps (2D) / eps (3D), in the reference's operation order
 *   flags          the generator's 1 on the sides, then flags_option 1 (0 leaves them).  3D: the unique flags are
 *                  decided on the coordinates the reference recomputes from the global id (:872-886), and its loop over
 *                  the repeated points stops at n_uni (:3170), so later repeated points keep the generator's flag
 *   owner          owning rank of every repeated node, nullable
 *   eflag          element flag, nullable: 2D the reference's patch 0.3 <= x <= 0.7, y >= 0.6 (:580-586), 3D zero
 * fedd_mesh_p2_vertices_first: perm[n_rep] (nullable) with perm[new] = local id, the P1 lattice nodes (all indices even)
 * first in the order fedd_mesh_structured_build numbers the P1 mesh of the same decomp / cells, then the others in
 * their reference order; n_p1 = their count.  A mesh renumbered by it obeys the device layer's convention "pressure
 * dofs = the first n_pressure_nodes node ids", and pressure dof k is the pressure domain's node k.
 * ---------------------------------------------------------------------------------------------- */
int fedd_mesh_structured_p2_sizes(int dim, const int* decomp, const int* cells, int rank,
                                  int64_t* n_rep, int64_t* n_uni, int64_t* n_elem);
int fedd_mesh_structured_p2_build(int dim, const int* decomp, const int* cells, int rank, int flags_option,
                                  double* xyz /*[n_rep*dim]*/, int64_t* gid_rep /*[n_rep]*/, int64_t* gid_uni /*[n_uni]*/,
                                  int32_t* owner /*[n_rep], nullable*/, int32_t* bcflag_rep /*[n_rep]*/,
                                  int32_t* bcflag_uni /*[n_uni]*/, int32_t* conn /*[n_elem*(6|10)]*/,
                                  int32_t* eflag /*[n_elem], nullable*/);
int fedd_mesh_p2_vertices_first(int dim, const int* decomp, const int* cells, int rank, int32_t* perm /*nullable*/,
                                int64_t* n_p1);

/* ------------------------------------------------------------------------------------------------
 * unstructured input, host side, one rank: INRIA/medit ".mesh" reader (MeshFileReader.cpp:16-106,
 * MeshFileReader.hpp:35-127, 1-based ids converted as MeshUnstructured_def.hpp:1181-1190) and the
 * P2-from-P1 construction (MeshUnstructured::buildP2ofP1MeshEdge, MeshUnstructured_def.hpp:129-410;
 * edge ids = rank in the sorted (min,max) list, EdgeElements.cpp:105-155; mid node id = n_vert + edge id;
 * slots (0,1)->4 (1,2)->5 (0,2)->6 (0,3)->7 (1,3)->8 (2,3)->9, :755-772; flags :806-900).
 * surf = boundary entities (Edges in 2D, Triangles in 3D), dim nodes each.
 * ---------------------------------------------------------------------------------------------- */
int fedd_mesh_read_sizes(const char* path, int dim, int64_t* n_vert, int64_t* n_elem, int64_t* n_surf);
int fedd_mesh_read(const char* path, int dim, double* xyz, int32_t* vflag, int32_t* conn, int32_t* eflag,
                   int32_t* surf, int32_t* sflag);
int fedd_mesh_p2_sizes(int dim, int64_t n_elem, const int32_t* conn_p1, int64_t* n_edges);
int fedd_mesh_p2_build(int dim, int64_t n_vert, int64_t n_elem, const int32_t* conn_p1, const double* xyz_p1,
                       const int32_t* vflag_p1, int64_t n_surf, const int32_t* surf, const int32_t* sflag,
                       int volume_id, int32_t* conn_p2, double* xyz_p2, int32_t* flag_p2);

/* Surface elements (boundary edges in 2D, triangles in 3D), host side.
 *   fedd_mesh_boundary_faces   the (dim-1)-faces that belong to exactly one of the n_elem elements (nen nodes each, the first
 *                              dim + 1 the vertices): what a mesh file lists as Edges / Triangles.  Vertex ids ascend within a
 *                              face, as the reference stores sub-elements (MeshPartitioner_def.hpp:766-773, 809-810); faces in
 *                              lexicographic order.  faces = NULL: count only.
 *   fedd_mesh_p2_surfaces      P2 surface elements from P1 ones: the dim vertices, then the mid nodes of the edges in the order of
 *                              the line / triangle bases -- 2D: mid(0,1); 3D: mid(0,1), mid(1,2), mid(0,2) -- with the node ids
 *                              fedd_mesh_p2_build gives them (n_vert + rank of the edge in the sorted edge list).  The reference
 *                              reaches the same node sets through the elements' local surfaces (MeshUnstructured_def.hpp:459-557);
 *                              only the assembled vector is normative, not the node order.  surf_p2[n_surf * (3 | 6)].
 *   fedd_mesh_structured_surfaces[_sizes]
 *                              the boundary faces of a rank's structured mesh (same arguments as fedd_mesh_structured_build,
 *                              ghost elements included): every face of a local element that lies on a side of the square /
 *                              cube, local repeated vertex ids ascending, in element order.  The reference builds no
 *                              sub-elements for its structured meshes (MeshStructured::buildSurfaceLinesSquare,
 *                              MeshStructured_def.hpp:230-238, has an empty body), so the flag rule is this library's: a face
 *                              carries the flag setStructuredMeshFlags (:2974-3203) gives to the nodes strictly inside its side
 *                              -- flags_option 0: 1 everywhere; flags_option 1: 2 on x = origin, 3 on x = origin + size, 1 on
 *                              the other sides. */
int fedd_mesh_boundary_faces(int dim, int nen, int64_t n_elem, const int32_t* conn, int64_t n_node, int64_t* n_faces,
                             int32_t* faces /*[n_faces*dim], nullable*/);
int fedd_mesh_p2_surfaces(int dim, int64_t n_vert, int64_t n_elem, const int32_t* conn_p1, int64_t n_surf,
                          const int32_t* surf_p1, int32_t* surf_p2);
int fedd_mesh_structured_surfaces_sizes(int dim, const int* decomp, const int* cells, int rank, int with_ghost_elements,
                                        int64_t* n_surf);
int fedd_mesh_structured_surfaces(int dim, const int* decomp, const int* cells, int rank, int flags_option,
                                  int with_ghost_elements, int32_t* surf /*[n_surf*dim]*/, int32_t* sflag /*[n_surf]*/);

/* ------------------------------------------------------------------------------------------------
 * element partitioner for unstructured meshes, host side: replaces MeshPartitioner::readAndPartitionMesh and the maps
 * it builds (feddlib/core/Mesh/MeshPartitioner_def.hpp:224-530; METIS_PartMeshDual :324, repeated map :358-397,
 * Map::buildUniqueMap Map_def.hpp:184-210) with a deterministic balanced recursive coordinate bisection of the element
 * centroids (every element on exactly one part).  conn holds GLOBAL node ids (0-based), nen nodes per element, the
 * first dim + 1 of them the vertices.
 *   fedd_mesh_partition          elem_part[n_elem] in [0, nparts)
 *   fedd_mesh_partition_sizes    sizes of rank's mesh: its own elements + `ghost_layers` layers of elements around
 *                                the owned nodes (1: owned rows complete; L >= 2: also the rows of the ghost nodes within
 *                                L - 1 layers, the row ghosts of fedd_mesh_set_rows)
 *   fedd_mesh_partition_extract  the rank's mesh in the form fedd_mesh_set / fedd_mesh_set_rows / fedd_halo_set_owners
 *                                take: local connectivity, coordinates, repeated map (ascending global ids) with flags
 *                                and owner ranks (lowest rank among the parts whose own elements hold the node),
 *                                unique map, row ghosts; elem_gid = global ids of the local elements.  Any output may
 *                                be NULL.
 * ---------------------------------------------------------------------------------------------- */
int fedd_mesh_partition(int dim, int nen, int64_t n_elem, const int32_t* conn, int64_t n_node, const double* xyz,
                        int nparts, int32_t* elem_part);
int fedd_mesh_partition_sizes(int nen, int64_t n_elem, const int32_t* conn, int64_t n_node, const int32_t* elem_part,
                              int nparts, int rank, int ghost_layers, int64_t* n_elem_loc, int64_t* n_rep, int64_t* n_uni,
                              int64_t* n_row_ghosts);
int fedd_mesh_partition_extract(int dim, int nen, int64_t n_elem, const int32_t* conn, int64_t n_node, const double* xyz,
                                const int32_t* flag, const int32_t* elem_part, int nparts, int rank, int ghost_layers,
                                int32_t* conn_loc, double* xyz_loc, int64_t* gid_rep, int32_t* flag_rep, int32_t* owner_rep,
                                int64_t* gid_uni, int32_t* flag_uni, int64_t* row_ghost_gid, int32_t* row_ghost_flag,
                                int64_t* elem_gid);

/* ------------------------------------------------------------------------------------------------
 * reference-element tables the assembly kernels stage in LDS (host side, no GPU needed): quadrature points and
 * weights of FE::getQuadratureValues (feddlib/core/FE/FE_def.hpp:6023-6727, degree remapping included) and the
 * values / gradients of FE::phi / FE::gradPhi (:4947-5087, :5565-5713) at those points.  Read-back for parity
 * tests against the reference's literals (tests/golden/ref_tables.json).
 * fedd_fe_quadrature: pts[nq*dim], w[nq] (call with NULL arrays for nq).  fedd_fe_basis: phi[nq*nen], dphi[nq*nen*dim].
 * ---------------------------------------------------------------------------------------------- */
/* dim = 1: the rules on [0,1] (FE_def.hpp:6031-6066: degrees 0 ... 3, a higher degree is an error) and the line bases with 2 and
 * 3 nodes (:4962-4985; P2 node order end, end, mid) that the boundary edges of a 2D mesh need; the boundary triangles of a 3D
 * mesh use the dim = 2 tables.  The surface form integrates at degree determineDegree(dim - 1, FEType, Std) + extra_degree
 * (:4530-4531, 5516-5562: P1 -> 1, P2 -> 2). */
int fedd_fe_quadrature(int dim, int degree, int* nq, double* pts, double* w);
int fedd_fe_basis(int dim, int nen, int degree, double* phi, double* dphi);

/* ------------------------------------------------------------------------------------------------
 * mesh upload: what FE::assemblyXxx reads through domainVec_[FEloc]->getElementsC(),
 * getPointsRepeated(), getMapRepeated() (feddlib/core/FE/FE_def.hpp:617-621) and what BCBuilder
 * reads through getBCFlagUnique()/getMapUnique() (feddlib/core/General/BCBuilder_def.hpp:625-626).
 * nen = nodes per element (P1: dim+1, P2: 6 / 10).  The first dim+1 nodes are the vertices
 * (FE::buildTransformation uses only those, FE_def.hpp:5342-5357).
 * ---------------------------------------------------------------------------------------------- */
int fedd_mesh_set(fedd_ctx* ctx, int dim, int nen, int64_t n_elem, const int32_t* conn,
                  int64_t n_rep, const double* xyz, const int64_t* gid_rep,
                  int64_t n_uni, const int64_t* gid_uni, const int32_t* bcflag_uni);
/* The same with row ghosts: nodes of the repeated map that another rank owns but ALL of whose elements are
 * in this rank's mesh.  Their matrix rows are then built, assembled and given the Dirichlet treatment
 * like owned rows (they follow the owned rows in the CSR arrays), and the overlapping Schwarz
 * subdomains take the true rows of such nodes instead of identity rows.  The boxes of the subdomains come
 * from one lattice over all ranks, and a box that holds an owned node is built whole -- with the other
 * ranks' nodes inside it and the full overlap -- wherever all its dofs have stored rows (with 27-node boxes
 * and overlap 1: row ghosts 3 node layers deep); each rank keeps the rows of its own nodes.  The
 * preconditioner is then the one a single rank would build, whatever the number of ranks.  Where the row
 * ghosts do not reach, a rank takes its own part of the box (true overlap rows still).  Everything else
 * (SpMV, vectors, fedd_csr_get, the coarse level) stays on the owned rows.  With row ghosts declared, only
 * they are imported in the halo exchange.  Every ghost node adjacent to an owned node must be listed. */
int fedd_mesh_set_rows(fedd_ctx* ctx, int dim, int nen, int64_t n_elem, const int32_t* conn,
                       int64_t n_rep, const double* xyz, const int64_t* gid_rep,
                       int64_t n_uni, const int64_t* gid_uni, const int32_t* bcflag_uni,
                       int64_t n_row_ghosts, const int64_t* row_ghost_gid, const int32_t* row_ghost_bcflag);

/* ------------------------------------------------------------------------------------------------
 * Moving mesh: new coordinates for the mesh that is on the device (one rank).
 * Replaces Mesh::moveMesh (feddlib/core/Mesh/Mesh_def.hpp:297-330) as Domain::moveMesh calls it in the ALE / FSI loops and in
 * problems/tests/geometry/main.cpp:683.
 *
 * fedd_mesh_move sets x[i][j] = x_ref[i][j] + disp_rep[dim*i + j] on the repeated map of fedd_mesh_set, ghost nodes included:
 * one addition in double per entry (Mesh_def.hpp:312).  x_ref is what the last fedd_mesh_set* uploaded (kept in a second
 * device buffer from the first move on).  Moves are relative to x_ref and NOT cumulative; disp_rep = NULL restores x_ref.
 *
 * Commit only on success.  The candidate coordinates are written to a buffer of their own and every element is checked: det B
 * of the candidate and of the reference element from the first dim + 1 nodes (FE::buildTransformation, FE_def.hpp:5342-5357).
 * If det * det_ref <= 0 for an element, the call fails with a message that names the smallest such element and its ratio
 * det / det_ref, and NOTHING is committed: coordinates, geometry_id and every cache stay as they were.  Otherwise the
 * coordinates are in force, n_moves and geometry_id go up by one and min_det_ratio = min over the elements of |det| / |det_ref|
 * is recorded (1.0 after a restore, which is not checked).  The check is a host-visible error, never a device fault.
 * An element that is degenerate in the REFERENCE mesh (det_ref == 0) fails the check under every displacement, the zero
 * displacement included: such a mesh cannot be moved (only restored, which is a copy).
 *
 * A move KEEPS (none of these reads a coordinate; after fedd_mesh_set* all of them are built again):
 *   - the node -> element adjacency;
 *   - the assembly's tile structures and tile shapes (the coordinate copies that lead the tile blobs are written again by the
 *     move; node lists, element records, gather lists and shapes stand -- the tiles keep the clusters they were built on);
 *   - the node and dof patterns: the system pattern (the next fedd_pattern_build repeats, fedd_pattern_reuse_info), the patterns
 *     of the stored slots, the node-level pattern of the advection matrices;
 *   - the gather lists (P2 row sums, advection, the FULL-pattern lists of the hyperelastic tangent and the stress form);
 *   - the advection / stress / hyperelastic scratch and reference tables, the velocity of fedd_velocity_set and the mesh
 *     velocity of fedd_mesh_velocity_set / fedd_mesh_velocity_diff (section "ALE convection"; nodal values, they read no
 *     coordinate);
 *   - the interface distances of fedd_interface_distance* (section "Interface distances"; nodal values: the reference never
 *     recomputes them on the moved mesh) and the coefficients of the last FEDD_FORM_LAPLACE_XDIM assembly;
 *   - the surface set of fedd_surface_set;
 *   - the Dirichlet flag tables (boundary flags of the nodes);
 *   - the halo plan;
 *   - the time-stepping histories (Newmark state, multistep history) and the Newton state;
 *   - the system matrix, right-hand side and solution, the solver's SpMV stream, and the stored slots with their VALUES: they
 *     belong to the coordinates they were assembled on, and geometry_id lets the caller tell (record it beside a store).
 * A move DROPS, to be built at next use (everything derived from coordinates, as opposed to matrix values):
 *   - the Schwarz box lattice and box structure (the next fedd_schwarz_setup builds its structure stage: the lattice is laid
 *     over the bounding box of the owned nodes, a node belongs to box floor((x - lo) / w) per direction, see fedd_schwarz_setup);
 *   - the preconditioner with its coarse level: coarse lattice, classification of the nodes, prolongation (a solve wants
 *     fedd_schwarz_setup again, as after an assembly);
 *   - the park + gather lists of the symmetric apply (they follow the box structure);
 *   - kept per-element geometry: the coordinate copies in the tile blobs (written again at once, above); there is no other;
 *   - the record of the last fedd_matrix_combine: fedd_matrix_combine_current answers 0.
 * What is derived from VALUES is left to the next assembly, which drops it already: the SpMV stream, dictionary and classes,
 * the Schwarz inverses and fingerprints, the CG setup.
 *
 * Errors: a host-only context ("needs a GPU context"), no mesh, more than one rank.
 * Left out: more than one rank.
 *
 * fedd_mesh_move_info: moves committed since the last fedd_mesh_set*, moves committed since the context was made, the ratio
 * above (0, 0, 1.0 on a fresh context).  Needs no device; outputs may be NULL.
 * fedd_mesh_coords_get: the coordinates in force, xyz_rep[n_rep * dim] on the repeated map.
 * ---------------------------------------------------------------------------------------------- */
int fedd_mesh_move(fedd_ctx* ctx, const double* disp_rep);
int fedd_mesh_move_info(fedd_ctx* ctx, int64_t* n_moves, int64_t* geometry_id, double* min_det_ratio);
int fedd_mesh_coords_get(fedd_ctx* ctx, double* xyz_rep);

/* ------------------------------------------------------------------------------------------------
 * Interface distances and the scaled vector Laplacian of the mesh extension (one rank).
 * Replaces Domain::calculateDistancesToInterface (feddlib/core/FE/Domain_def.hpp:568-648), the distance loop of
 * MeshInterface::buildMeshInterfaceParallelAndDistance (feddlib/core/Mesh/MeshInterface_def.hpp:473-491) and
 * FE::assemblyLaplaceXDim (feddlib/core/FE/FE_def.hpp:2225-2402) with HeuristicScaling
 * (feddlib/problems/specific/Geometry_def.hpp:24-34), the default model of the Geometry problem (Geometry_def.hpp:63-76).
 *
 * NORMATIVE -- the distances (Domain_def.hpp:621-647), for every node i of the repeated map, ghost nodes included:
 *     dist[i] = min(1000.0, min_j sqrt(sum_k (x_i[k] - p_j[k])^2))
 *   - the difference, then its square, per coordinate; the squares summed in ascending k; every product and every sum is
 *     rounded on its own (no fused multiply-add);
 *   - the kernel takes the minimum of the SQUARED distances and one sqrt per node: a correctly rounded sqrt is monotone, so
 *     the bits are those of the minimum of the roots;
 *   - a minimum does not depend on order: the result is independent of the order of the interface points and of the tiling;
 *   - no floating-point atomic; two calls agree bit for bit;
 *   - with no interface point every entry is 1000.0 and n_interface = 0; that is not an error.
 * fedd_interface_distance: the interface points are the nodes of this context whose node flag (bcflag_uni of fedd_mesh_set)
 * is one of flags[n_flags], at the coordinates IN FORCE at the call, i.e. after any fedd_mesh_move.  *n_interface (may be
 * NULL) receives their number.
 * fedd_interface_distance_points: the same against n_pts points of the caller's, xyz_pts[n_pts * dim].
 * fedd_interface_distance_set: distances of the caller's on the repeated map, dist_rep[n_rep]; NULL releases them.
 * fedd_interface_distance_get: dist_rep[n_rep] on the repeated map; an error without distances.
 * fedd_interface_distance_info: whether distances are held, the number of interface points of the last computing call (0
 * after _set), and the number of points the kernel stages in LDS per tile.  Needs no device; outputs may be NULL.
 * Lifetime: the distances are nodal values.  fedd_mesh_move KEEPS them (the reference never recomputes them on the moved
 * mesh); fedd_mesh_set* releases them.
 *
 * NORMATIVE -- fedd_assemble(ctx, FEDD_FORM_LAPLACE_XDIM, params = {distance, coefficient}), on the pattern of
 * FEDD_FORM_LAPLACE_VEC (fedd_pattern_build(dim, FEDD_BLOCK_DIAG)), on the coordinates in force:
 *   - per element (FE_def.hpp:2273-2278, 2343-2349): mean = (d_0 + d_1 + d_2) / 3.0 in 2D, (d_0 + d_1 + d_2 + d_3) / 4.0 in
 *     3D, summed left to right over the FIRST dim + 1 nodes of the element (P2 mid-edge nodes do not enter);
 *     f = coefficient if mean < distance (strict), else f = 1.0;
 *   - K[(i,a),(j,a)] = |det B| sum_k (f w_k) (grad phi_j . grad phi_i) for every component a: k ascending, the dot product
 *     summed in ascending coordinate, f w_k formed first, |det B| multiplied last; rule determineDegree(dim, FE, FE, Grad, Grad);
 *   - NO doSetZeros: the reference's routine has none (unlike assemblyLaplaceVecField), option "asm_zero_eps" does not apply;
 *   - the rows are summed in adjacency order through gather lists, no floating-point atomic: two calls agree bit for bit.
 * fedd_laplace_scale_get: f_elem[n_elem], the coefficients of the last such assembly on this mesh.
 *
 * Errors: a host-only context ("needs a GPU context"), no mesh, more than one rank, n_pts < 0, n_flags < 0, _get without
 * distances; the assembly without distances (the message names fedd_interface_distance), with params == NULL, on another
 * pattern.  Each is a message, never a device fault.
 * Left out: recomputing the distances on the moved mesh, more than one rank.  (The matched interface tables are "FSI coupling"
 * below.)
 * ---------------------------------------------------------------------------------------------- */
int fedd_interface_distance(fedd_ctx* ctx, int n_flags, const int32_t* flags, int64_t* n_interface);
int fedd_interface_distance_points(fedd_ctx* ctx, int64_t n_pts, const double* xyz_pts);
int fedd_interface_distance_set(fedd_ctx* ctx, const double* dist_rep);
int fedd_interface_distance_get(fedd_ctx* ctx, double* dist_rep);
int fedd_interface_distance_info(fedd_ctx* ctx, int* have, int64_t* n_interface, int* tile_points);
int fedd_laplace_scale_get(fedd_ctx* ctx, double* f_elem);

/* symbolic CSR on the owned (unique-map) rows: what Tpetra's dynamic insert + fillComplete
 * discover (feddlib/core/LinearAlgebra/Matrix_def.hpp:88-92,192-199). */
int fedd_pattern_build(fedd_ctx* ctx, int dofs_per_node, int block_mode, int64_t* nnz_out);
/* A fedd_pattern_build that repeats the one the system pattern came from -- same mesh, dofs per node, block mode and "pat_hash",
 * and nothing wrote the pattern since (fedd_block_merge, fedd_assemble_div, a fedd_matrix_combine that brings another pattern,
 * fedd_mesh_set*) -- keeps the arrays on the device and does only what the call promises beside them: values, right-hand side,
 * solution and Dirichlet marks zeroed, solver setups dropped, nnz returned.  Option "pattern_reuse" = 0 builds every time (the
 * same integers; the A/B switch).  last_reused: 1 if the last build kept the pattern; n_reused: builds that kept it since the
 * context was made.  Needs no device; outputs may be NULL. */
int fedd_pattern_reuse_info(fedd_ctx* ctx, int* last_reused, int64_t* n_reused);

/* numeric assembly into the pattern; FE::assemblyXxx + fillComplete (file:line per form above). */
int fedd_assemble(fedd_ctx* ctx, int form, const double* params);

/* ------------------------------------------------------------------------------------------------
 * Stress form of the velocity block ("Symmetric gradient" of Stokes and Navier-Stokes, Stokes_def.hpp:69-70,
 * NavierStokes_def.hpp:142-143): FE::assemblyStress (feddlib/core/FE/FE_def.hpp:2407-2733; element loops :2457-2562 in 2D,
 * :2587-2727 in 3D), int c(x) grad v : (grad u + grad u^T) in place of the vector Laplacian.  One rank.
 *   For element T, local nodes i, j, row component a, column component b, with the transformed gradients (dPhiTrans):
 *       K[(i,a),(j,b)] = |det B| sum_k c_k w_k ( delta_ab grad phi_i . grad phi_j + d_b phi_i d_a phi_j )
 *   at row dim * gid(i) + a, column dim * gid(j) + b: e_a^i.innerProduct(e_b^j) with e_b^j = E + E^T (:2495-2559, 2629-2724;
 *   SmallMatrix::innerProduct is the Frobenius product, SmallMatrix.hpp:164-196).
 *   Quadrature: determineDegree(dim, FEType, FEType, Grad, Grad) (:2427) -- P1 one point, P2 degree 2 (nq = 3 in 2D, 5 in 3D);
 *   the points and weights are those of fedd_fe_quadrature.
 *   coeff_q  NULL: c = 1 (the reference's OneFunction, the only coefficient its two problem classes pass).  Otherwise
 *            coeff_q[e * nq + k] = c(x_k) of element e (in the order of fedd_mesh_set) at x_k = B xi_k + p_1, p_1 the element's
 *            first vertex (:2487-2493, 2616-2625), and n_coeff must equal n_elem * nq.
 *   The system matrix must have the pattern of fedd_pattern_build(dim, FEDD_BLOCK_FULL); every (a, b) pair of every node pair is
 *   written, structural zeros kept.  fedd_assemble(ctx, FEDD_FORM_STRESS, NULL) is this call with c = 1.
 *   Operation order: per element and node pair i <= j the dim x dim sums O[b][a] = sum_k (c_k w_k d_b phi_i) d_a phi_j, k
 *   ascending; then tr O is added on a == b and the block is multiplied by |det B|; the block of (j, i) is the transpose of that
 *   of (i, j), taken from the same numbers.  The element blocks are added to their rows in the order of the node -> element
 *   adjacency.  No floating-point atomics: two calls on one input agree bit for bit.  Parity with the reference's loop is at
 *   1e-10 of a row's largest magnitude, not bit for bit.
 *   Like every assemble the call overwrites the values of the system matrix: Dirichlet rows are to be set again, Schwarz, SpMV
 *   and CG setups are dropped.  The gather lists of the row sums are those of fedd_assemble_hyperelastic (one copy per mesh and
 *   pattern, built at the first call of either: FEDD_T_SYMBOLIC); later calls move values only (FEDD_T_ASSEMBLE).
 *   Memory: the pair blocks pass through the scratch of fedd_assemble_advection, here 8 * n_elem * nen (nen + 1) / 2 * dim^2
 *   bytes -- 3960 bytes per P2 tetrahedron, 0.78 GB on the P2 mesh of a 32^3-cell cube -- held between calls and released by the
 *   next fedd_mesh_set*.
 *   Errors: a host-only context ("needs a GPU context"); no pattern, or one that is not dim dofs per node / FULL;
 *   n_coeff != n_elem * nq; more than one rank.
 * ---------------------------------------------------------------------------------------------- */
int fedd_assemble_stress(fedd_ctx* ctx, const double* coeff_q, int64_t n_coeff);

/* FE::assemblyRHS + MultiVector::exportFromVector(...,"Add") (FE_def.hpp:4694-4766,
 * feddlib/problems/abstract/Problem_def.hpp:184-216): constant f per dof, quadrature degree
 * determineDegree(dim,FE,Std) + extra_degree. */
int fedd_assemble_rhs(fedd_ctx* ctx, int dofs_per_node, const double* f_const, int extra_degree);

/* Surface loads and Neumann terms: f_(i,d) += int_Gamma g_d phi_i over the surface elements of fedd_surface_set -- what
 * FE::assemblySurfaceIntegral / assemblySurfaceIntegralFlag (FE_def.hpp:4511-4691) compute for Problem::assembleSourceTerm
 * with "Source Type" = "surface" (Problem_def.hpp:170-181, 219-254) and for the "Neumann" entries of BCBuilder::setRHS
 * (BCBuilder_def.hpp:172-199).  Per surface element S and local node li the contribution is
 *   scaling_S * (sum_q w_q phi_q,li) * g[d],  scaling_S = |B[:,0]| in 2D, |B[:,0] x B[:,1]| in 3D, B = vertex differences from
 * vertex 0 (buildTransformationSurface :5406-5428, SmallMatrix::computeScaling SmallMatrix.hpp:360-378), times the number of
 * local volume elements that hold all vertices of S (1 on a boundary): the reference integrates a sub-element once per element
 * that holds it (:4550-4553).  With at least one ghost layer every element at an owned node is local, so the owned rows are
 * complete on any number of ranks without an exchange.  Like the reference (:4519, 4610) only constant loads are taken.
 *   fedd_surface_set   surf[n_surf * nsn] local repeated node ids, nsn = dim (P1) or 3 / 6 (P2 in 2D / 3D: the vertices, then
 *                      the mid nodes in the order of fedd_mesh_p2_surfaces), sflag[n_surf].  After fedd_mesh_set[_rows]; a later
 *                      fedd_mesh_set drops the set.  n_surf = 0 is valid and clears it.
 *   fedd_assemble_surface         g[n_flags * dofs]: the load of the elements that carry flags[k] (others contribute nothing);
 *                                 n_flags = 0, flags = NULL: g[dofs] on every element.
 *   fedd_assemble_surface_values  g_surf[n_surf * dofs]: one load per surface element.
 * accumulate = 1 adds into the right-hand side (mv->update(1., *aUnique, 1.)); nodes without surface elements keep their value
 * bit for bit.  accumulate = 0 overwrites it (assemblySurfaceIntegral after putScalar(0.)); such nodes get 0.  After
 * fedd_pattern_build, owned rows only.  No atomics: each node sums its elements in ascending order, two calls agree bit for bit.
 * Dirichlet rows: call fedd_dirichlet* afterwards; it overwrites, so where a Neumann and a Dirichlet flag meet on a node the
 * Dirichlet value stands (the reference, in code it marks experimental, adds the Neumann vector after the Dirichlet values). */
int fedd_surface_set(fedd_ctx* ctx, int nsn, int64_t n_surf, const int32_t* surf, const int32_t* sflag);
int fedd_assemble_surface(fedd_ctx* ctx, int dofs_per_node, int n_flags, const int32_t* flags, const double* g,
                          int extra_degree, int accumulate);
int fedd_assemble_surface_values(fedd_ctx* ctx, int dofs_per_node, const double* g_surf, int extra_degree, int accumulate);

/* BCBuilder::setSystem + setRHS for constant boundary values (BCBuilder_def.hpp:589-707, 93-170):
 * rows of nodes whose flag is in flags[] become unit rows (pattern kept), rhs <- values.
 * comp_mask[n_bc*dofs] (nullable = all components), values[n_bc*dofs]. */
int fedd_dirichlet(fedd_ctx* ctx, int n_bc, const int32_t* flags, const int32_t* comp_mask,
                   const double* values);

/* same, for boundary values that depend on the node (the host evaluates the user's BC function at
 * every flagged unique node, BCBuilder_def.hpp:128-143, and passes the results): owned_nodes[n]
 * local unique-map node ids, comp_mask[n*dofs] (nullable), values[n*dofs]. */
int fedd_dirichlet_nodes(fedd_ctx* ctx, int64_t n, const int32_t* owned_nodes, const int32_t* comp_mask,
                         const double* values);

/* unit rows on arbitrary system rows (merged block systems): what setLocalRowOne on the diagonal
 * block + setLocalRowZero on the off-diagonal blocks (BCBuilder_def.hpp:653-707) leave in that row. */
int fedd_dirichlet_rows(fedd_ctx* ctx, int64_t n, const int32_t* rows, const double* values);

/* ------------------------------------------------------------------------------------------------
 * mixed / block problems (one rank for now).  Blocks live in numbered slots beside the system matrix.
 *   fedd_matrix_store     copy the system matrix into `slot` (0..6; Stokes uses 0..3 = A, B, B^T, C, Navier-Stokes adds 4 = the
 *                         linearised velocity block of fedd_assemble_advection, its time loop 5 = the velocity mass matrix and
 *                         6 = the time-combined constant velocity block (cm * M) + (ca * A), "BDF time stepping" below)
 *   fedd_matrix_scale     Matrix::scale (Stokes_def.hpp:83-85,102); slot < 0 = system matrix
 *   fedd_assemble_div     FE::assemblyDivAndDivT (FE_def.hpp:1932-2057): velocity = the mesh's element,
 *                         pressure = P1 on the vertices = the first n_pressure_nodes node ids; B -> slot_b
 *                         (n_p x dim*n_v), B^T -> slot_bt.  Overwrites the system slot (scratch).
 *   fedd_block_merge      BlockMatrix::merge + BlockMap::merge (BlockMatrix_def.hpp:119-148,212-287;
 *                         BlockMap_def.hpp:55-80): system <- [A B^T; B C] (slot < 0 = empty block); merged
 *                         global ids = block-local gid + cumulated (maxAllGlobalIndex + 1).  A merge of the same slots
 *                         whose patterns have not been rewritten since the last merge (values may have: the blocks of a
 *                         nonlinear iteration) keeps the merged pattern and moves values only; right-hand side, solution
 *                         and Dirichlet marks are reset as by every merge.
 *   fedd_matrix_sizes/get read a stored block back (local column ids).
 * ---------------------------------------------------------------------------------------------- */
int fedd_matrix_store(fedd_ctx* ctx, int slot);
int fedd_matrix_scale(fedd_ctx* ctx, int slot, double alpha);
int fedd_assemble_div(fedd_ctx* ctx, int64_t n_pressure_nodes, int slot_b, int slot_bt);
int fedd_block_merge(fedd_ctx* ctx, int slot_a, int slot_bt, int slot_b, int slot_c);
int fedd_matrix_sizes(fedd_ctx* ctx, int slot, int64_t* n_rows, int64_t* n_cols, int64_t* nnz);
int fedd_matrix_get(fedd_ctx* ctx, int slot, int64_t* rowptr, int32_t* colind, double* val);

/* ------------------------------------------------------------------------------------------------
 * Newmark time stepping for linear single-block problems (unsteady linear elasticity), one rank like the block slots it uses:
 * what DAESolverInTime::advanceInTimeLinearNewmark (feddlib/problems/Solver/DAESolverInTime_def.hpp:519-607) does per step with
 * Tpetra vectors and matrix additions.  On a context with more than one rank every entry below is an error that says so; on a
 * host-only context they fail with "needs a GPU context".  No multiplication is fused with an addition in any of them.
 *
 *   fedd_matrix_combine   system matrix <- (cm * M[slot_m]) + (ca * A[slot_a]): TimeProblem::combineSystems
 *                         (feddlib/problems/abstract/TimeProblem_def.hpp:359-408: systemMass_->addMatrix(massParameters_,
 *                         combined, 0) followed by system->addMatrix(timeParameters_, combined, 1)).  The two products are
 *                         rounded separately and then added, as the two addMatrix calls do.  The result has the pattern of
 *                         slot_a, structural zeros included.  slot_m holds a matrix of the same mesh with the same pattern
 *                         (same block mode of fedd_pattern_build) or the DIAG node-block pattern where slot_a has the FULL one
 *                         (mass against elasticity; an entry M does not have counts as 0.0).  Errors: an empty slot, slots stored
 *                         before the last fedd_mesh_set, FULL into DIAG and every other pairing.  When the system slot already
 *                         holds slot_a's pattern (a fedd_matrix_store into slot_a or an earlier combine put it there and nothing
 *                         rewrote it since) only values move and the pattern generation stands, so the next fedd_schwarz_setup
 *                         keeps its structure stage (fedd_schwarz_reuse_info).  Right-hand side and solution are NOT reset
 *                         (unlike fedd_block_merge) unless their length changes; Dirichlet marks are: the rows are real rows
 *                         again until fedd_dirichlet* is called.
 *   fedd_matrix_combine_current
 *                         *current = 1 while the system matrix still is that combine: same slots and coefficients, neither slot
 *                         written since (fedd_matrix_store, fedd_matrix_scale, fedd_assemble_div, fedd_assemble_advection each
 *                         count as a write), the system matrix not rebuilt by anything else.  Dirichlet rows do not count: a time
 *                         loop that finds 1 skips the combine, fedd_dirichlet and both solver setups and calls
 *                         fedd_dirichlet_rhs only.  The reference combines and builds its preconditioner in every step
 *                         (DAESolverInTime_def.hpp:565); the results are the same.  Needs no device.
 *   fedd_matrix_apply     y = alpha * (M[slot] x), host pointers (x[n_cols], y[n_rows]): Matrix::apply on a stored block, i.e.
 *                         BlockMatrix::apply with a coefficient (TimeProblem_def.hpp:413, 519).  A group of lanes per row; each
 *                         lane adds its products in ascending column order and the lane sums meet in a fixed tree: two calls
 *                         agree bit for bit.  The same kernel forms the Newmark right-hand side on device vectors.
 *   fedd_newmark_begin    u_n <- the current solution, v = w = 0 (the start values of TimeProblem_def.hpp:913-926); the next
 *                         fedd_newmark_advance is the first step.
 *   fedd_newmark_set/get  the state vectors u_n, v (velocity), w (acceleration), host pointers of the system's length, any of
 *                         them NULL (tests, restarts).  A state that was set counts as a state after some step: the next advance
 *                         is not a first step.
 *   fedd_newmark_advance  TimeProblem::updateSolutionNewmarkPreviousStep (:875-981) followed by updateNewmarkRhs (:473-524).
 *                         With u = the current solution (the result u_{n+1} of the step just solved) and the coefficients,
 *                         evaluated in double precision exactly as written,
 *                             cuu = 1.0 / ((dt * dt) * beta)      cuv = 1.0 / (dt * beta)        cuw = (0.5 - beta) / beta
 *                             cvu = gamma / (dt * beta)            cvv = 1.0 - (gamma / beta)     cvw = (dt * (beta - (0.5 * gamma))) / beta
 *                         every row does, each product and each sum rounded on its own, in this order (NORMATIVE):
 *                             unless this is the first step:   d  = u - u_n
 *                                                              v' = ((cvu * d) + (cvv * v)) + (cvw * w)
 *                                                              w' = ((cuu * d) - (cuv * v)) - (cuw * w)        (the old v)
 *                             first step:                      v' = v,  w' = w
 *                             u_n <- u
 *                             t   = ((cuu * u) + (cuv * v')) + (cuw * w')
 *                         in ONE kernel that reads u, u_n, v, w and writes u_n, v, w, t once (56 bytes per row), and then
 *                             rhs <- coeff * (M[slot_m] t)          (the kernel of fedd_matrix_apply)
 *                         Errors: dt <= 0, beta <= 0, an empty slot, a slot of another size or mesh, no state.
 *   fedd_rhs_axpy         rhs += alpha * f, host pointer: DAESolverInTime::addSourceTermToRHS (DAESolverInTime_def.hpp:1444-1450).
 *                         fedd_assemble_rhs overwrites the right-hand side, so a loop assembles the load once, reads it back and
 *                         adds it here with the step's factor.
 *   fedd_solution_set     the device's solution vector <- x (the counterpart of fedd_solution_get: initial values, restarts, tests)
 *   fedd_dirichlet_rhs    the right-hand-side half of fedd_dirichlet (BCBuilder::setRHS, BCBuilder_def.hpp:93-170): rhs <- values
 *                         on the flagged rows; the matrix, whose rows an earlier fedd_dirichlet made unit rows, is not touched, so
 *                         the preconditioner and the solver's SpMV setup stand.
 * ---------------------------------------------------------------------------------------------- */
int fedd_matrix_combine(fedd_ctx* ctx, int slot_m, double cm, int slot_a, double ca);
int fedd_matrix_combine_current(fedd_ctx* ctx, int slot_m, double cm, int slot_a, double ca, int* current);
int fedd_matrix_apply(fedd_ctx* ctx, int slot, double alpha, const double* x_owned, double* y_owned);
int fedd_newmark_begin(fedd_ctx* ctx);
int fedd_newmark_set(fedd_ctx* ctx, const double* u_n, const double* v, const double* w);
int fedd_newmark_get(fedd_ctx* ctx, double* u_n, double* v, double* w);
int fedd_newmark_advance(fedd_ctx* ctx, int slot_m, double dt, double beta, double gamma, double coeff);
int fedd_rhs_axpy(fedd_ctx* ctx, double alpha, const double* f_owned);
int fedd_solution_set(fedd_ctx* ctx, const double* x_owned);
int fedd_dirichlet_rhs(fedd_ctx* ctx, int n_bc, const int32_t* flags, const int32_t* comp_mask, const double* values);

/* ------------------------------------------------------------------------------------------------
 * BDF time stepping for nonlinear block problems (unsteady Navier-Stokes), one rank: the vector part of the reference's
 * "Class" = "Multistep" loop, DAESolverInTime::advanceInTimeNonLinearMultistep (DAESolverInTime_def.hpp:1209-1333) with the
 * BDF tables of TimeSteppingTools.cpp:493-515.  Error conventions as for Newmark: "needs a GPU context" on a host-only context,
 * an error that says so on more than one rank.  No multiplication is fused with an addition.
 *
 * The matrices need no entry of their own: the velocity mass matrix is stored in slot 5, the constant velocity block
 * A' = (cm * M) + (ca * A) is a fedd_matrix_combine of slots 5 and 0 followed by a fedd_matrix_store into slot 6 (both DIAG, so
 * only values move), once per coefficient set, i.e. twice in a BDF2 run (BDF1 for the first step, BDF2 afterwards).  Every
 * nonlinear iteration then calls fedd_assemble_advection(kind, rho, slot_add = 6, slot_out = 4) and the values-only
 * fedd_block_merge of slots 4, 2, 1, C.
 *
 *   n   = the length of the current system (the merged one: velocity dofs, then pressure dofs)
 *   n_m = the rows of M[slot_m], the velocity block; n_m <= n
 *   u   = the device's current solution vector; the caller sets it with fedd_solution_set, because fedd_block_merge resets it
 *
 *   fedd_multistep_begin    allocates `order` (1 or 2) history vectors u_0, u_1 of length n, zeroed, and sets count = 0.  Does
 *                           not read the solution.  The vectors are buffers of their own: they survive fedd_block_merge,
 *                           fedd_assemble_advection, fedd_matrix_combine and fedd_dirichlet*; the next fedd_mesh_set* releases
 *                           them.
 *   fedd_multistep_advance  TimeProblem::updateSolutionMultiPreviousStep (TimeProblem_def.hpp:833-849: the first call fills [0],
 *                           the second grows the list, later calls shift) followed by updateMultistepRhs (:417-438).
 *                           coeff[0 .. n_use) are the caller's coefficients, already divided by dt.  ONE streaming kernel does on
 *                           every row of the system, each product and each sum rounded on its own, in this order (NORMATIVE):
 *                               old0 = u_0                                   (only if count >= 1)
 *                               u_1 <- old0                                  (only if order == 2 and count >= 1)
 *                               u_0 <- u
 *                               t   = coeff[0] * u                           (n_use == 1)
 *                               t   = (coeff[0] * u) + (coeff[1] * old0)     (n_use == 2)
 *                           and after it
 *                               count = min(count + 1, order)
 *                               rhs[0 .. n_m) <- M[slot_m] t                 (the kernel of fedd_matrix_apply, alpha = 1.0)
 *                               rhs[n_m .. n) <- 0.0                         (updateMultistepRhs zeroes the right-hand side and
 *                                                                             adds mass terms only where massParameters_ != 0)
 *                           A full BDF2 step reads u, u_0 and writes u_0, u_1, t: 40 bytes per row; a first step 24.
 *                           The reference forms sum_i coeff_i * (M u_i) with one apply per history vector; here M is applied ONCE
 *                           to the combination -- a deliberate difference at rounding level.
 *                           Errors: no history (fedd_multistep_begin first), n_use < 1 or n_use > min(count + 1, order), an empty
 *                           slot, a slot of an earlier mesh, a slot with more rows than the system, a system whose length has
 *                           changed since fedd_multistep_begin.
 *   fedd_multistep_set/get  history vector k = 0 .. order - 1, host pointer of length n (tests, restarts).  A vector that was set
 *                           counts as a state after some step: count = max(count, k + 1).
 *   fedd_multistep_info     order (0: no history) and count.  Needs no device.
 * ---------------------------------------------------------------------------------------------- */
int fedd_multistep_begin(fedd_ctx* ctx, int order);
int fedd_multistep_advance(fedd_ctx* ctx, int slot_m, int n_use, const double* coeff);
int fedd_multistep_set(fedd_ctx* ctx, int k, const double* u_k);
int fedd_multistep_get(fedd_ctx* ctx, int k, double* u_k);
int fedd_multistep_info(fedd_ctx* ctx, int* order, int* count);

/* ------------------------------------------------------------------------------------------------
 * Single-step time stepping for nonlinear block problems (unsteady Navier-Stokes), one rank: the multi-stage part of the
 * reference's "Class" = "Singlestep" loop, DAESolverInTime::advanceInTimeNonLinear (DAESolverInTime_def.hpp:384-516), for the
 * diagonally implicit, stiffly accurate Butcher tables with a_00 = 0 of TimeSteppingTools::setTableInformationRK
 * (TimeSteppingTools.cpp:309-487, tables 0-4), the time definition [[1,1],[0,0]] and size = 2 blocks.  Error conventions as for
 * Newmark and BDF: "needs a GPU context" on a host-only context (fedd_stage_info excepted), an error that says so on more than
 * one rank.  No multiplication is fused with an addition.
 *
 * What the reference does per step, and the calls that restate it (slots as in "BDF time stepping": 0 = A, 1 = B, 2 = B^T,
 * 4 = F, 5 = M, 6 = the time-combined constant block):
 *   stage 0 (dummy)       reAssembleAndFill gives F_0 = A + rho N(u_n); U_0 = [u_n ; p_n] is kept:
 *                             fedd_stage_begin(S); fedd_assemble_advection(N, rho, slot_add = 0, slot_out = 4); fedd_solution_set(U_0);
 *                             fedd_stage_push(4)
 *   stage s = 1 .. S - 1  buildMultiStageRhs: fedd_stage_rhs(5, 2, s, coeff_f, coeff_bt) with coeff_f[j] = -(dt * a_sj) and
 *                             coeff_bt[j] = coeff_f[j], or 0.0 under "Full implicit pressure".
 *                         The stage system [(1.0 * M) + (dt * a_ss) (A + rho N(u)), s_bt B^T ; B, C], s_bt = dt * a_ss, or dt under
 *                             full implicit pressure: fedd_matrix_combine(5, 1.0, 0, dt * a_ss) + fedd_matrix_store(6) when dt * a_ss
 *                             changed, then per nonlinear iteration fedd_assemble_advection(kind, (dt * a_ss) * rho, 6, 4) and
 *                             fedd_block_merge_scaled(4, 2, s_bt, 1, C), which moves values only.
 *                         After the solve, unless s is the last stage: F_s = A + rho N(u_s) (fedd_assemble_advection(N, rho, 0, 4)),
 *                             fedd_solution_set(U_s), fedd_stage_push(4).  The last stage's solution is the step's result.
 *   adaptive steps        TimeSteppingTools::adaptiveTimestep / calculateNewDt take ||U_a - U_b||: fedd_stage_error.
 *
 *   n   = the length of the current system (the merged one: velocity dofs, then pressure dofs)
 *   n_m = the rows of the stage operators = the rows of M[slot_m], the velocity block
 *
 *   fedd_stage_begin   opens a step for max_stages = 2 .. 8 stages and sets count = 0.  The stages are buffers of their own, NOT
 *                      matrix slots (the slots stay 0 .. 6): per stored stage one value array of the length of the stored velocity
 *                      block's nonzeros and one vector of length n, allocated on first need and kept from step to step.
 *                      Memory per stage: 8 * nnz(FULL velocity pattern) + 8 * n bytes.  fedd_mesh_set* releases the store;
 *                      fedd_mesh_move, fedd_block_merge*, fedd_assemble_advection*, fedd_matrix_combine and fedd_dirichlet* keep it.
 *   fedd_stage_push    appends stage j = count: the VALUES of M[slot_f] and the device's current solution vector, device to
 *                      device.  The first push of a step records the pattern of slot_f (its pattern identity and its slot, whose
 *                      row pointers and columns fedd_stage_rhs reads); later pushes must present the same slot with the same
 *                      pattern (fedd_assemble_advection into the same slot keeps it).  Errors: no open step, count ==
 *                      max_stages, an empty slot, a slot of an earlier mesh, a slot with another pattern, a slot with more rows
 *                      than the system, a system whose length changed since the first push.
 *   fedd_stage_rhs     n_prior = 1 .. count; coeff_f, coeff_bt host arrays of length n_prior.  ONE kernel over the n_m velocity
 *                      rows, every product and every sum rounded on its own, in this order (NORMATIVE):
 *                          t = rowsum(M[slot_m], u_0)
 *                          for j = 0 .. n_prior - 1 ascending:
 *                              mv = coeff_f[j] * rowsum(F_j, u_j)
 *                              if coeff_bt[j] != 0.0:  mv = mv + (coeff_bt[j] * rowsum(B^T[slot_bt], p_j))
 *                              t = t + mv
 *                          rhs[row] = t ;   rhs[n_m .. n) = 0.0
 *                      u_j = the first n_m entries of stage vector j, p_j the rest.  rowsum is the row sum of
 *                      fedd_matrix_apply on that block, bit for bit: the block's own lane group (8 lanes up to 32 entries in
 *                      its longest row, else 16), each lane adding in ascending column order, the same fixed tree.  The row
 *                      pointers and columns of the stages' pattern are read once per row for all n_prior value arrays, those
 *                      of B^T once for all p_j; no atomics, two calls agree bit for bit.  slot_bt < 0 is allowed only when
 *                      every coeff_bt[j] is 0.0.  Where coeff_bt[j] is 0.0 the reference adds 0.0 * (B^T p_j); for finite data
 *                      that equals skipping the term, which is what happens here.
 *                      Errors: no stages, n_prior out of range, an empty slot, a slot of the wrong size or mesh, B^T columns
 *                      != n - n_m, the slot of the first push no longer holding the stages' pattern.
 *   fedd_block_merge_scaled
 *                      fedd_block_merge with every B^T value multiplied by s_bt (one product per entry) on its way into the
 *                      merged matrix; the stored slot is not modified.  Same values-only path and the same resets of right-hand
 *                      side, solution and Dirichlet marks; s_bt == 1.0 gives the bits of fedd_block_merge.  Where only values
 *                      move -- a change of s_bt alone is such a case -- the pattern generation stands (fedd_block_merge, which
 *                      keeps its code path and its bits, declares the pattern written there too).
 *   fedd_stage_error   *err = ||d||, d = U_ja - U_jb formed on the fly; ja, jb stage indices, -1 = the device's current solution.
 *                      FEDD_STAGE_ERR_EUCLIDEAN: sqrt(sum_i d_i^2) over all n rows; FEDD_STAGE_ERR_L2: sqrt(sum_i d_i *
 *                      rowsum(M[slot_m], d)_i) over the velocity rows (slot_m is not read for the Euclidean kind).  Partial sums
 *                      per wave in a fixed tree, summed in a fixed order by a second small kernel, the root on the host: no
 *                      floating-point atomics, two calls agree bit for bit.
 *   fedd_stage_get     stage j = 0 .. count - 1: the value array (nnz doubles) and the vector (n doubles), host pointers, either
 *                      may be NULL (tests, restarts).
 *   fedd_stage_info    max_stages (0: no open step), count, and nnz and n of the first push (0 while count is 0).  Needs no device.
 * ---------------------------------------------------------------------------------------------- */
enum fedd_stage_err { FEDD_STAGE_ERR_EUCLIDEAN = 0, FEDD_STAGE_ERR_L2 = 1 };
int fedd_stage_begin(fedd_ctx* ctx, int max_stages);
int fedd_stage_push(fedd_ctx* ctx, int slot_f);
int fedd_stage_rhs(fedd_ctx* ctx, int slot_m, int slot_bt, int n_prior, const double* coeff_f, const double* coeff_bt);
int fedd_block_merge_scaled(fedd_ctx* ctx, int slot_a, int slot_bt, double s_bt, int slot_b, int slot_c);
int fedd_stage_error(fedd_ctx* ctx, int kind, int slot_m, int ja, int jb, double* err);
int fedd_stage_get(fedd_ctx* ctx, int j, double* f_val, double* u);
int fedd_stage_info(fedd_ctx* ctx, int* max_stages, int* count, int64_t* nnz, int64_t* n);

/* ------------------------------------------------------------------------------------------------
 * steady Navier-Stokes (one rank, like the block system it feeds): the matrices NavierStokes::reAssemble builds in every
 * nonlinear iteration (feddlib/problems/specific/NavierStokes_def.hpp:282-321) from the current velocity.
 *   fedd_velocity_set        u_rep[n_rep * dim], node-wise interleaved on the repeated map of fedd_mesh_set: what
 *                            NavierStokes::u_rep_ holds (NavierStokes_def.hpp:290-291, 305-306).
 *   fedd_assemble_advection  slot_out <- scale * (N(u) | W(u) | N(u) + W(u)) + M[slot_add]   (slot_add < 0: nothing added):
 *                            FE::assemblyAdvectionVecField / assemblyAdvectionInUVecField (FE_def.hpp:1759-1832, 1839-1925)
 *                            with scale = density (N->scale(density), :295, 313), then A_->addMatrix(1., ANW, 0.) and
 *                            N->addMatrix(1., ANW, 1.) (:297-298, 316-319) in one device pass.  slot_out has the FULL
 *                            dim x dim node-block pattern of the velocity space whatever the kind (N leaves structural zeros
 *                            off the diagonal pairs); M[slot_add] is a velocity matrix of the same mesh with the DIAG pattern
 *                            (the stored FEDD_FORM_LAPLACE_VEC block) or the FULL one, in a slot other than slot_out.
 *                            Quadrature: determineDegree (FE_def.hpp:1770-1772, 1859-1861) -- P2 degree 5 for both, P1 2 for N
 *                            and 3 for W.  Option "asm_zero_eps" thresholds the element values of N and of W as the reference
 *                            does under setZeros_ (:1816, 1908).  The node-level pattern, the gather lists of the row sums and
 *                            the adjacency are built at the first call after fedd_mesh_set (timer FEDD_T_SYMBOLIC) and kept;
 *                            later calls move values only (timer FEDD_T_ASSEMBLE), also after fedd_block_merge has replaced
 *                            the system matrix, which this call never touches.  No atomics: two calls on the same input
 *                            agree bit for bit.  fedd_matrix_get reads the result.
 *                            Memory: the element blocks pass through a device scratch of 8 * n_elem * nen^2 * dim^2 bytes
 *                            (N alone: 8 * n_elem * nen^2) -- 7.2 KB per P2 tetrahedron, 11.3 GB on the P2 mesh of a 64^3-cell
 *                            cube -- held between calls and released by the next fedd_mesh_set.
 * ---------------------------------------------------------------------------------------------- */
int fedd_velocity_set(fedd_ctx* ctx, const double* u_rep);
int fedd_assemble_advection(fedd_ctx* ctx, int kind, double scale, int slot_add, int slot_out);

/* ------------------------------------------------------------------------------------------------
 * ALE convection (one rank, like the advection path it extends): the velocity block of the fluid on a moving mesh,
 * A + rho N(u - w) - rho P(w) and in a Newton step + rho W(u) (feddlib/problems/specific/FSI_def.hpp:445-464, 497-503, 533-541;
 * NavierStokes::reAssembleFSI, NavierStokes_def.hpp:245-278, 754-760), on the coordinates fedd_mesh_move put in force.
 *   fedd_mesh_velocity_set   w_rep[n_rep * dim], node-wise interleaved (dim * node + d) on the repeated map of fedd_mesh_set:
 *                            what FSI::meshVelocity / w_rep_ holds.  It lives in a device buffer of its own beside the one of
 *                            fedd_velocity_set, with the same lifetime: kept by fedd_mesh_move, released by fedd_mesh_set*.
 *                            w_rep = NULL clears it (the next fedd_assemble_advection_ale is an error).
 *   fedd_mesh_velocity_diff  w = (d_new - d_old) * (1.0 / dt), the arithmetic in one device kernel after the host has permuted both
 *                            arrays to the mesh's numbering and copied them up (the cost of the call, made once per time
 *                            step, is that host side, as for fedd_velocity_set), NORMATIVE in this order: one subtraction
 *                            per entry, one multiplication by the reciprocal formed in double on the host -- what
 *                            w_rep_->update(-1, old, 1); w_rep_->scale(1.0 / dt) does (FSI_def.hpp:460-462).  d_new_rep,
 *                            d_old_rep: displacements on the repeated map, like fedd_mesh_move's.  Errors: dt <= 0, a dt that
 *                            is not finite, a null array.
 *   fedd_mesh_velocity_get   w_rep[n_rep * dim] back.  Errors: no mesh velocity, more than one rank.
 *   fedd_assemble_advection_ale
 *                            slot_out <- scale * E + M[slot_add] on the FULL velocity pattern, u from fedd_velocity_set, w from
 *                            the calls above:
 *                              FEDD_ALE_P           E = P(w), FE::assemblyAdditionalConvection (FE_def.hpp:3044-3255): entry
 *                                                   (dim*i+d, dim*j+d) = |det B| sum_q w_q (div w_h)(x_q) phi_i(x_q) phi_j(x_q),
 *                                                   div w_h(x_q) = sum_i sum_d w[i][d] (grad phi_i B^-1)_d; positive sign, as
 *                                                   the reference returns it; off-diagonal component pairs are structural
 *                                                   zeros of the FULL pattern
 *                              FEDD_ALE_FIXEDPOINT  E = N(u - w) - P(w)
 *                              FEDD_ALE_NEWTON      E = N(u - w) + W(u) - P(w); W takes u, not u - w (FSI_def.hpp:540 ->
 *                                                   NavierStokes::reAssemble("Newton") on u_rep_)
 *                            With scale = density the fused kinds are the reference's A + (-rho) P + rho N [+ rho W]
 *                            (FSI_def.hpp:497-503, NavierStokes_def.hpp:262-272).  The pattern, gather lists, slot rules (slot_add
 *                            < 0, DIAG or FULL, never slot_out) and error texts are those of fedd_assemble_advection, and so are
 *                            the structures: a first call on a mesh may build them (FEDD_T_SYMBOLIC), later calls -- also after
 *                            fedd_mesh_move -- move values only (FEDD_T_ASSEMBLE).  The write of slot_out is recorded like
 *                            every other slot write: fedd_matrix_combine_current answers 0 for a combine that read the slot.
 *                            Quadrature: N as in fedd_assemble_advection; P by determineDegree(dim, FE, FE, Std, Std,
 *                            determineDegree(dim, FE, Grad)) (FE_def.hpp:3064-3065).  The inner call returns 1 for P1 as well as
 *                            for P2 (a degree 0 is raised to 1, :5540-5541), so the rule is degree 3 for P1 and 5 for P2: the
 *                            rule of W, not the one of N (they coincide for P2 only).  No third table is staged.
 *                            Operation order, NORMATIVE: per element c = u - w at its nodes (one subtraction); beta from c and
 *                            grad u_h from u as in fedd_assemble_advection; per point q of the rule of W,
 *                            div = sum_d sum_r (sum_i w[i][d] dphi_i,r) Binv[r][d] (i, r, d ascending), pw_q = w_q * div; per node
 *                            pair p_ij = |det B| * sum_q (phi_i phi_j) pw_q (q ascending).  N and W keep their setZeros threshold
 *                            ("asm_zero_eps") per element value; P has none in the reference and gets none; the threshold is
 *                            applied to n_ij (and the W block) BEFORE p_ij is subtracted.  With w = 0 the fused kinds return
 *                            the bits of FEDD_ADV_N / FEDD_ADV_NEWTON and FEDD_ALE_P is zero.  No atomics: two calls agree bit
 *                            for bit.  Memory: the scratch of fedd_assemble_advection.
 *                            Errors: a host-only context ("needs a GPU context"), more than one rank, no velocity (except
 *                            FEDD_ALE_P, which needs none), no mesh velocity, unknown kind, every slot error of
 *                            fedd_assemble_advection.
 * Left out: the FSI problem class, geometry-implicit coupling, shape derivatives, more than one rank.
 * ---------------------------------------------------------------------------------------------- */
int fedd_mesh_velocity_set(fedd_ctx* ctx, const double* w_rep);               /* NULL clears */
int fedd_mesh_velocity_diff(fedd_ctx* ctx, const double* d_new_rep, const double* d_old_rep, double dt);
int fedd_mesh_velocity_get(fedd_ctx* ctx, double* w_rep);
int fedd_assemble_advection_ale(fedd_ctx* ctx, int kind, double scale, int slot_add, int slot_out);

/* ------------------------------------------------------------------------------------------------
 * nonlinear elasticity (one rank, like the advection path): tangent and internal forces of a hyperelastic material for the
 * displacement u, FE::assemblyElasticityJacobianAndStressAceFEM (feddlib/core/FE/FE_def.hpp:837-1291; element loops :1123-1267
 * in 3D, :928-1066 in 2D), which NonLinElasticity::reAssemble("Newton-Residual") calls in every Newton step
 * (feddlib/problems/specific/NonLinElasticity_def.hpp:89-103).
 *   u   is what fedd_velocity_set uploaded: u_rep[n_rep * dim], node-wise interleaved on the repeated map (the buffer is the
 *       nodal vector field of the context; for this entry it holds NonLinElasticity::u_rep_, :69-71, 90-92).
 *   Per element T and quadrature point p of the rule determineDegree(dim, FEType, FEType, Grad, Grad) (:856; P1 one point, P2
 *   degree 2), in this order:
 *       g_i = B^-T grad phi_i(x_p)                         transformed gradients
 *       F   = I + sum_i u_i (x) g_i                        nodes in element order, (:1143-1156)
 *       P(F), A[i][j][k][l] = dP_ij / dF_kl                the material, both multiplied by w_p at once
 *       H_j[d1][k][d2] = sum_l A[d1][k][d2][l] g_j,l
 *       K_(i,d1),(j,d2) += sum_k g_i,k H_j[d1][k][d2]      summed over p, then multiplied by |det B|   (:1200-1222, 1258-1262)
 *       f_(i,d)         += sum_k P_dk g_i,k                summed over p, then multiplied by |det B|   (:1229-1243, 1251-1253)
 *   The element blocks are then added to their rows in the order of the node -> element adjacency.  No floating-point atomics:
 *   two calls on the same input agree bit for bit, and tangent-only / force-only calls give the bits of the combined call.
 *   Materials (one per call), with C = F^T F, I1 = tr C, I2 = (I1^2 - tr C^2) / 2, J = det F; the reference's generated routines
 *   nh3d, mr3d, stvk3d, stvk2d (:6969-7803) evaluate the same functions:
 *       FEDD_HYPER_NEOHOOKE       params {E, nu}:     mu = E / (2 (1 + nu)), lambda = E nu / ((1 + nu)(1 - 2 nu)),
 *                                 psi = mu / 2 (I1 - 3) - mu ln J + lambda / 2 (ln J)^2
 *       FEDD_HYPER_MOONEY_RIVLIN  params {E, nu, C}:  mu as above, kappa = E / (3 (1 - 2 nu)),
 *                                 psi = (1 - C) mu / 2 (I1 - 3) + C mu / 2 (I2 - 3) - mu (1 + C) ln J + kappa / 2 (ln J)^2
 *       FEDD_HYPER_STVK           params {lambda, mu} (the caller derives them as :887-896 does):
 *                                 P = F (lambda tr(E) I + 2 mu E), E = (C - I) / 2
 *   In 2D only FEDD_HYPER_STVK exists (:903); the other two are an error there.
 *   what  FEDD_HYPER_TANGENT: K overwrites the values of the system matrix, which must have the pattern of
 *         fedd_pattern_build(dim, FEDD_BLOCK_FULL) -- the one FEDD_FORM_LINELAS fills -- so fedd_dirichlet, fedd_schwarz_setup,
 *         fedd_gmres and the reuse keys work as after fedd_assemble (Dirichlet rows are to be set again, the preconditioner to be
 *         set up again).  FEDD_HYPER_FORCE: f goes into a device vector of the owned rows, read by fedd_hyperelastic_force_get.
 *         Both: one pass over the elements.
 *   Inverted elements: where J <= 0 at a quadrature point and the material takes ln J (Neo-Hooke, Mooney-Rivlin) the call
 *   returns non-zero and fedd_last_error names the first such element; the system matrix and the force vector are NOT written
 *   then (the element pass ends before the rows are summed).  Saint Venant-Kirchhoff is a polynomial in F and is evaluated for
 *   any F, as in the reference.
 *   The gather lists of the row sums are built at the first call on a pattern (timer FEDD_T_SYMBOLIC) and kept; later calls move
 *   values only (FEDD_T_ASSEMBLE).  Memory: the element blocks pass through the scratch of fedd_assemble_advection,
 *   8 * n_elem * nen^2 * dim^2 bytes (7.2 KB per P2 tetrahedron), and the element forces through 8 * n_elem * nen * dim bytes.
 * ---------------------------------------------------------------------------------------------- */
enum fedd_hyper_model { FEDD_HYPER_NEOHOOKE = 0, FEDD_HYPER_MOONEY_RIVLIN = 1, FEDD_HYPER_STVK = 2 };
#define FEDD_HYPER_TANGENT 1
#define FEDD_HYPER_FORCE 2
int fedd_assemble_hyperelastic(fedd_ctx* ctx, int model, const double* params, int n_params, int what);
int fedd_hyperelastic_force_get(fedd_ctx* ctx, double* f_owned);

/* ------------------------------------------------------------------------------------------------
 * Nonlinear Newmark (unsteady nonlinear elasticity), one rank and one block like the Newmark and the hyperelastic entries it
 * pairs: what DAESolverInTime::advanceInTimeNonLinearNewmark (feddlib/problems/Solver/DAESolverInTime_def.hpp:613-722) does in
 * the Newton iterations of a time step -- TimeProblem::calculateNonLinResidualVec (feddlib/problems/abstract/
 * TimeProblem_def.hpp:693-738), NonLinElasticity::calculateNonLinResidualVec (feddlib/problems/specific/
 * NonLinElasticity_def.hpp:251-271), NonLinearSolver::solveNewton (feddlib/problems/Solver/NonLinearSolver_def.hpp:459-531) --
 * with the iterate, the residual and the update resident on the device.  On a context with more than one rank every entry below
 * is an error that says so; on a host-only context they fail with "needs a GPU context" (fedd_newton_info needs no device).  No
 * multiplication is fused with an addition in any of them and there is no floating-point atomic.
 *
 *   fedd_assemble_hyperelastic_time
 *                         fedd_assemble_hyperelastic with one difference in the tangent half: the system matrix receives
 *                         (cm * M[slot_m]) + K(u), the time tangent of TimeProblem::combineSystems with the coefficients
 *                         1 / (dt^2 beta) and 1.0, in the pass that sums the rows.  M has the system's FULL pattern or the DIAG
 *                         node-block pattern, the pairings of fedd_matrix_combine.  NORMATIVE: the stored values are bit for bit
 *                         those of fedd_assemble_hyperelastic(FEDD_HYPER_TANGENT), fedd_matrix_store(a free slot),
 *                         fedd_matrix_combine(slot_m, cm, that slot, 1.0): the product cm * m is rounded, then added to the row
 *                         sum; where M has no entry 0.0 is multiplied and added all the same (a row sum of -0.0 is stored as
 *                         +0.0 for cm >= 0, as the sequence stores it).  The force half, the inverted-element behaviour (nothing
 *                         written), the timers and the kept gather lists are those of fedd_assemble_hyperelastic; the Dirichlet
 *                         marks are not reset (the sequence's combine resets them): fedd_dirichlet follows either.  Errors: an
 *                         empty slot, a slot of an earlier mesh, a pairing fedd_matrix_combine would refuse.
 *   fedd_newton_begin     u_k <- the device's current solution vector; b <- the device's current right-hand side, held in a
 *                         buffer of its own; the nodal vector field (the buffer of fedd_velocity_set) <- u_k: on one rank without
 *                         ghost nodes the repeated map is the owned map.  Clears the source vector and the counters.  The system
 *                         must have dim dofs per node.
 *   fedd_newton_source_set
 *                         the step's source vector s, host pointer of the system's length, uploaded once; NULL clears it.
 *   fedd_newton_residual  ONE kernel forms, per row i, m_i = cm * (sum_k M[slot_m]_ik u_k,col(k)) with the lanes per row (8 for rows
 *                         of at most 32 entries, else 16), the ascending column order per lane and the fixed tree of
 *                         fedd_matrix_apply, so that m carries the bits of fedd_matrix_apply(slot_m, cm, u_k), and then, each
 *                         operation rounded on its own, in this order (NORMATIVE; the "reverse" residual):
 *                             r = b - f
 *                             r = r + s                    (only if a source is set)
 *                             r = r - m
 *                         f = the force vector of the last FEDD_HYPER_FORCE call.  Rows whose node flag is flags[k] and whose
 *                         component has comp_mask[k * dofs + comp] != 0 (NULL: all), first match, get
 *                             r = g - u_k                  g = values[k * dofs + comp]   (BCBuilder::setBCMinusVector)
 *                         r is written into the context's right-hand side, so that fedd_gmres(ctx, NULL, NULL, ...) solves for the
 *                         Newton update; fedd_dirichlet on the tangent comes BEFORE this call (it writes the right-hand side of
 *                         its rows).  *norm2 = ||r||_2: every workgroup adds the squares of its rows by a fixed tree, one
 *                         workgroup adds those partial sums in a fixed order, the host takes the root: two calls agree bit for
 *                         bit.  Bytes: 12 nnz(M) + 4 (n + 1) + 32 n (+ 8 n with a source) + 4 n / dofs.
 *                         Errors: no state, an empty slot, a slot of another size or mesh, no force vector, a force vector older
 *                         than the last fedd_newton_begin / fedd_newton_update ("stale").
 *   fedd_newton_update    u_k <- u_k + (alpha * delta), delta = the device's solution vector (what fedd_gmres left); the nodal
 *                         vector field <- u_k; *norm_delta = ||delta||_2 (the reference's "Criterion" = "Update"), summed as
 *                         above.  One streaming kernel, 32 bytes per row.
 *   fedd_newton_end       solution vector <- u_k, right-hand side <- b: fedd_newmark_advance finds u_{n+1} where it looks for it.
 *                         Ends the state.
 *   fedd_newton_get       u_k to the host.
 *   fedd_newton_info      active (0 / 1), the length, whether a source is set, whether the force vector is newer than the iterate,
 *                         residual and update calls since the begin.  active, the length and the source flag describe the open
 *                         state (0 after fedd_newton_end); the force flag and the two counters outlive fedd_newton_end and show the
 *                         finished step until the next fedd_newton_begin.  Needs no device; outputs may be NULL.
 *
 * The source term is restated as the reference has it, not corrected: DAESolverInTime::addSourceTermToRHS adds it to the
 * right-hand side b (here: fedd_rhs_axpy before fedd_newton_begin) and NonLinElasticity::calculateNonLinResidualVec adds it
 * again (here: s), so a caller that follows the reference passes the same vector twice.  The steady class has the same doubling.
 * ---------------------------------------------------------------------------------------------- */
int fedd_assemble_hyperelastic_time(fedd_ctx* ctx, int model, const double* params, int n_params, int what, int slot_m, double cm);
int fedd_newton_begin(fedd_ctx* ctx);
int fedd_newton_source_set(fedd_ctx* ctx, const double* s_owned);
int fedd_newton_residual(fedd_ctx* ctx, int slot_m, double cm, int n_bc, const int32_t* flags, const int32_t* comp_mask,
                         const double* values, double* norm2);
int fedd_newton_update(fedd_ctx* ctx, double alpha, double* norm_delta);
int fedd_newton_end(fedd_ctx* ctx);
int fedd_newton_get(fedd_ctx* ctx, double* u_k);
int fedd_newton_info(fedd_ctx* ctx, int* active, int64_t* n, int* have_source, int* force_fresh, int64_t* n_residuals,
                     int64_t* n_updates);

/* read-back for Tpetra::CrsMatrix fill / parity (Matrix::getLocalRowView analog). col_gid maps
 * a local column index to its global dof id. */
int fedd_csr_sizes(fedd_ctx* ctx, int64_t* n_rows, int64_t* n_cols, int64_t* nnz);
int fedd_csr_get(fedd_ctx* ctx, int64_t* rowptr, int32_t* colind, double* val, int64_t* col_gid);
int fedd_rhs_get(fedd_ctx* ctx, double* rhs_owned);
int fedd_rhs_set(fedd_ctx* ctx, const double* rhs_owned);
int fedd_solution_get(fedd_ctx* ctx, double* x_owned);

/* y = A x on owned rows incl. ghost import: Matrix::apply (Matrix_def.hpp:245-254).
 * host pointers; fedd_spmv_device runs `reps` launches on the resident vectors (bench). */
int fedd_spmv(fedd_ctx* ctx, const double* x_owned, double* y_owned);
int fedd_spmv_device(fedd_ctx* ctx, int reps);
/* what the SpMV streams: nnz of the parity CSR (owned rows), nnz of the compacted stream actually read
 * (= nnz_pattern with "spmv_compact" 0 or when the windowed kernel is not in use) */
int fedd_spmv_info(fedd_ctx* ctx, int64_t* nnz_pattern, int64_t* nnz_streamed);

/* one-level overlapping additive Schwarz (replaces Thyra::initializePrec on the FROSch factory,
 * feddlib/problems/Solver/Preconditioner_def.hpp:243-463; options from
 * feddlib/problems/tests/laplace/parametersPrec.xml:10-61).  Subdomains are `target_nodes`-node
 * boxes of the rank's owned nodes (batched, many per GPU), extended by `overlap` graph
 * layers; exact dense local solves.
 * two_level != 0 adds a coarse level, M^-1 = M_one^-1 + Phi K0^-1 Phi^T, the role FROSch's
 * GDSWCoarseOperator plays under "TwoLevel" = true (parametersPrec.xml:62-122).  coarse_kind:
 * FEDD_COARSE_Q1 = multilinear hat functions of a regular lattice over the global bounding box
 * (DESIGN.md "two-level" gives the normative definition and why it stands in for GDSW here);
 * K0 = Phi^T A Phi is formed and inverted on the device, replicated on every rank. */
#define FEDD_COARSE_Q1 1
/* FEDD_COARSE_GDSW: FROSch's GDSWCoarseOperator on a second, coarse decomposition -- the cells of the same regular lattice
 * (fedd_schwarz_set_coarse; default one cell per 1000 nodes, at most what the dense coarse solver takes: 10^3 cells for scalar, 7^3 for 3-dof problems in 3D):
 * interface nodes are classified into the faces / edges / vertices between the cells, the coarse basis is the null space
 * (constants per dof component: what FROSch has without node coordinates, parametersPrec.xml:5 "Use node lists" = false)
 * restricted to each interface component and extended discrete-harmonically into the cell interiors (device GMRES +
 * one-level Schwarz on the constrained operator, option "gdsw_tol", default 1e-4 for GDSW and 1e-3 for RGDSW: the outer iteration count is that of exact extensions down to there, see
 * profiles/r02_gdsw_tol_sweep.txt and r03_gdsw_tol_sweep_stacked.txt; the parity tests ask for 1e-13; option "gdsw_block" 1 (default) = sixteen columns at a
 * time as one stacked system over an SpMM and a matrix-core Schwarz apply, multi.hip, 0 = column by column; "multi_ch" 4 / 8 / 16 = matrix-core
 * steps per flight of gathers of that apply), K0 = Phi^T A Phi inverted on the
 * matrix cores.  (2g - 1)^dim * dofs coarse dofs for g cells per direction.
 * Option "gdsw_rotations" 1 (default 0; GDSW and RGDSW, vector problems with dofs = dim): what FROSch builds with "Use node
 * lists" = true and "Rotations" = true (steadyLinElas/parametersPrec.xml:6, 100) -- every interface component carries the
 * linearised rotations about its centre next to the translations (3 + 3 functions in 3D, 2 + 1 in 2D; the coarse space then
 * holds the rigid-body modes of every cell).  Functions that are linearly dependent on a component's free dofs are dropped
 * (a Cholesky sweep over the component's Gram matrix: a one-node vertex keeps its translations, a straight edge 5 of 6);
 * (2g - 1)^dim * (dofs + rotations) coarse dofs, the dropped ones with a unit diagonal in K0.  Normative definition:
 * oracle/fedd_oracle.py CoarseGDSW(rotations=True). */
#define FEDD_COARSE_GDSW 2
/* FEDD_COARSE_RGDSW: the reduced GDSW space (FROSch RGDSWCoarseOperator, the one steadyLinElas_Perf/parametersPrec.xml:18
 * names; Dohrmann & Widlund 2017, option 1): coarse functions only for the coarse nodes of the same decomposition (its
 * vertices; for slab / pencil decompositions the interface components without lower-dimensional neighbours), an interface
 * node of component e carrying 1 / |C(e)| for each adjacent coarse node; harmonic extensions and K0 as for GDSW.
 * (g - 1)^dim * dofs coarse dofs: the default lattice is one cell per 400 nodes, at most what the dense coarse solver takes
 * (14^3 cells for 3-dof problems in 3D). */
#define FEDD_COARSE_RGDSW 3
int fedd_schwarz_setup(fedd_ctx* ctx, int overlap, int combine, int two_level, int coarse_kind);
/* target_nodes = 0 (the default): 27 nodes for scalar problems, 27 / dofs-per-node for vector ones */
int fedd_schwarz_set_target(fedd_ctx* ctx, int target_nodes, double scale);
/* number of lattice cells the coarse level aims at (0 = default: global nodes / 1000, clamped to
 * [1, 1728]); call before fedd_schwarz_setup */
int fedd_schwarz_set_coarse(fedd_ctx* ctx, double cells_target);
/* How the two levels combine (FROSch "Level Combination", parametersPrec.xml:19 of laplace, stokes, steadyLinElas, ...; the
 * reference pre-applies the coarse level for "Multiplicative", LinearSolver_def.hpp:98-104, and FROSch's TwoLevelPreconditioner
 * then combines the levels in every apply).  FEDD_LEVELS_ADDITIVE (the default): z = M1^-1 r + Pc r.  FEDD_LEVELS_MULTIPLICATIVE:
 * y1 = M1^-1 r, z = y1 - Pc (A y1), i.e. z = (I - Pc A) M1^-1 r (the overlapping level first, then the coarse one; no + Pc r
 * term), with Pc = Phi K0^-1 Phi^T.  This operator cannot reduce the part of a residual that Phi^T sees, so under it
 * fedd_gmres and fedd_gmres_x0 start from x_0 + Pc (b - A x_0) (for x_0 = 0: the reference's pre-apply; the step is taken twice,
 * as K0^-1 carries a 1e-12 diagonal shift) and project the true residual the same way at every restart.  A property of the
 * context, read at apply time (no new fedd_schwarz_setup needed; it may be set before the setup, whose coarse-space solves stay
 * one-level).  fedd_schwarz_apply and fedd_gmres* report an error
 * when the multiplicative combination meets a setup without a coarse level, the large-subdomain path or a merged block system. */
#define FEDD_LEVELS_ADDITIVE 0
#define FEDD_LEVELS_MULTIPLICATIVE 1
int fedd_schwarz_set_level_combination(fedd_ctx* ctx, int combination);
int fedd_schwarz_get_level_combination(fedd_ctx* ctx, int* combination);
/* coarse level read-back (parity): lattice cells per direction, coarse dofs n0, K0^-1 row-major */
int fedd_schwarz_coarse_sizes(fedd_ctx* ctx, int32_t cells[3], int64_t* n0);
int fedd_schwarz_coarse_get(fedd_ctx* ctx, double* k0_inverse);
int fedd_schwarz_apply(fedd_ctx* ctx, const double* r_owned, double* z_owned);
int fedd_schwarz_apply_device(fedd_ctx* ctx, int reps);
int fedd_schwarz_info(fedd_ctx* ctx, int64_t* n_subdomains, int64_t* max_size, int64_t* inverse_bytes);
/* The setup has a structure stage (box lattice, bins, overlapping dof lists: a function of the node coordinates, the matrix
 * graph and the setup parameters) and a numeric stage (everything that reads matrix values), as FROSch's initialize() /
 * compute().  The structure is kept from one fedd_schwarz_setup to the next while the mesh, the pattern (a repeated
 * fedd_pattern_build with the same arguments on the same mesh counts as the same pattern), target, scale, overlap and the box
 * options stand; with several ranks all ranks keep it or none does.  Option "schwarz_reuse" = 0 builds it in every setup.
 * last_reused: 1 if the last setup kept the structure; n_reused: setups that kept it since the context was made. */
int fedd_schwarz_reuse_info(fedd_ctx* ctx, int* last_reused, int64_t* n_reused);
/* number of DISTINCT local matrices of the last setup: subdomains whose principal submatrices agree (to 2^-44 of each row's
 * largest entry; option "schwarz_dedupe", default 1) share one stored inverse, which fedd_schwarz_info's inverse_bytes
 * counts once.  On the structured cube of the headline a few hundred of the 389 017 subdomains are distinct. */
int fedd_schwarz_unique(fedd_ctx* ctx, int64_t* n_unique);
/* sum over this rank's subdomains of their sizes (owned + overlap dofs) and of their owned dofs: what one apply gathers
 * and scatters (byte model of the apply kernel in bench.py); either output may be NULL */
int fedd_schwarz_sizes(fedd_ctx* ctx, int64_t* sum_sizes, int64_t* sum_owned);
/* subdomains whose dof list is their representative's list shifted by a constant (every box of a class on a structured mesh):
 * the matrix-core apply computes their dof ids from the representative's offsets and does not read their lists */
int fedd_schwarz_conforming(fedd_ctx* ctx, int64_t* n_conforming);
/* The symmetric apply without floating-point atomics (FEDD_COMBINE_FULL / FEDD_COMBINE_AVERAGING; options "apply_gather" and
 * "apply_full_kind" below; fedd_cg always uses it): every subdomain parks y_i = A_i^-1 R_i r, a lane per owned dof then adds the
 * parked entries of its dof in the fixed order of a list sorted at setup, so two applies of one r give the same bits.  This call
 * builds the lists if they are not built yet and tells how many subdomains the matrix-core park kernel takes (those that share
 * their inverse with another subdomain, in batches of up to sixteen) and how many the one-workgroup-per-subdomain kernel. */
int fedd_schwarz_full_info(fedd_ctx* ctx, int64_t* n_mfma, int64_t* n_plain);

/* right-preconditioned restarted GMRES (replaces Thyra::solve on the Belos "Block GMRES"
 * LOWS, feddlib/problems/Solver/LinearSolver_def.hpp:72-135; parametersSolver.xml:5-15).
 * b_owned / x_owned may be NULL: then the assembled rhs is used and the solution stays on the
 * device (fedd_solution_get reads it).  use_prec = 0 runs unpreconditioned. Returns the iteration
 * count the way Problem::solve does (its_out). */
int fedd_gmres(fedd_ctx* ctx, const double* b_owned, double* x_owned, double rtol, int max_it,
               int restart, int use_prec, int* its_out, double* relres_out);
/* The same solve from a given initial guess: the reference's "Zero Initial Guess" = false (LinearSolver_def.hpp:76-78, where
 * the solution vector is only cleared when the key is true).  x_owned in: x_0, out: the solution; NULL: x_0 is the vector the
 * device holds (the last solution, or what fedd_schwarz_coarse_apply(ctx, NULL, NULL) left there) and the solution stays on
 * the device.  The relative residual refers to ||r_0|| = ||b - A x_0||, as Belos' default scaling does.  Under
 * FEDD_LEVELS_MULTIPLICATIVE x_0 is first projected, x_0 + Pc (b - A x_0) twice, and r_0 is the residual of the projected guess
 * (for a guess that fedd_schwarz_coarse_apply made, the projection changes nothing in exact arithmetic). */
int fedd_gmres_x0(fedd_ctx* ctx, const double* b_owned, double* x_owned, double rtol, int max_it,
                  int restart, int use_prec, int* its_out, double* relres_out);
/* Preconditioned conjugate gradients for systems that are symmetric positive definite on their free dofs (Laplace, linear
 * elasticity): Belos "Block CG" / "Pseudo Block CG" with block size 1.  Arguments and NULL conventions are those of fedd_gmres /
 * fedd_gmres_x0 without `restart`.  The algorithm (normative):
 *   1. den = ||b - A x_0|| for the caller's x_0 (fedd_cg: x_0 = 0), Belos' default scaling as in fedd_gmres_x0.  (fedd_cg_x0: a
 *      guess with ||b - A x_0|| <= 1e-13 (||b|| + ||A x_0||) is at the rounding floor of the product and is returned as it is,
 *      0 iterations.)
 *   2. Dirichlet lift: x_0[d] <- b[d] on every Dirichlet row d.  Those rows are identity rows (rows are zeroed, not columns), so
 *      r is then exactly 0 there, z, p and q stay 0 there, and the iteration runs on A_II, which is symmetric.
 *   3. r = b - A x, z = M^-1 r (or z = r), p = mask z, rho = r.z            (mask: 0 on the Dirichlet rows, 1 elsewhere)
 *   4. loop: q = A p; alpha = rho / (p.q); x += alpha p; r -= alpha q; stop if ||r|| <= rtol den; z = M^-1 r; rho' = r.z;
 *      beta = rho' / rho; p = mask (z + beta p)
 * The test runs on the device; the returned x is exactly the iterate that met it and its_out its index.  Every claim of
 * convergence is checked against ||b - A x|| (the product fedd_gmres checks with): if it fails, r is replaced by the true
 * residual, z, p and rho start again and the loop continues; after three replacements in a row without progress the solve
 * stops.  relres_out is always the true relative residual.  p.q <= 0, rho <= 0 or a non-finite value is a breakdown: the call
 * returns an error that names it.  The preconditioner must be symmetric: FEDD_COMBINE_FULL (applied by the park + gather kernels,
 * whatever "apply_gather" says), one level or with the additive coarse level.  Errors before any work: FEDD_COMBINE_RESTRICTED /
 * FEDD_COMBINE_AVERAGING ("not symmetric: use FEDD_COMBINE_FULL"), FEDD_LEVELS_MULTIPLICATIVE, a merged block system, the
 * large-subdomain path, and a context with more than one rank (summing the overlap contributions across ranks needs an
 * export-add of the ghost entries that does not exist yet: the follow-up). */
int fedd_cg(fedd_ctx* ctx, const double* b_owned, double* x_owned, double rtol, int max_it, int use_prec, int* its_out,
            double* relres_out);
int fedd_cg_x0(fedd_ctx* ctx, const double* b_owned, double* x_owned, double rtol, int max_it, int use_prec, int* its_out,
               double* relres_out);
/* the last fedd_cg / fedd_cg_x0: residual replacements, and the breakdown word (0 = none); outputs may be NULL */
#define FEDD_CG_BREAKDOWN_PQ 1          /* p.Ap <= 0 */
#define FEDD_CG_BREAKDOWN_RHO 2         /* r.z <= 0 */
#define FEDD_CG_BREAKDOWN_NONFINITE 3   /* a dot product was not finite */
#define FEDD_CG_BREAKDOWN_NONSYMMETRIC 4 /* the matrix is not symmetric on its free rows (probed on the first direction) */
int fedd_cg_info(fedd_ctx* ctx, int* replacements, int* breakdown);

/* ------------------------------------------------------------------------------------------------
 * Block preconditioners for merged 2 x 2 systems (Stokes, Navier-Stokes), one rank: the reference's "Preconditioner Method" =
 * "Diagonal" / "Triangular", PrecBlock2x2::applyIt (feddlib/problems/Solver/PrecBlock2x2_def.hpp:114-164) as built by
 * Preconditioner::buildPreconditionerBlock2x2 (Preconditioner_def.hpp:979-1062) with the pressure mass matrix of
 * Stokes_def.hpp:122-132 / NavierStokes_def.hpp:177-183.  The reference keeps a small problem of its own per block
 * (MinPrecProblem); here each block is a CHILD CONTEXT: a fedd_ctx with the block's mesh, whose system matrix is the block and
 * whose fedd_schwarz_setup -- one-level or two-level, Q1 / GDSW / RGDSW, rotations, every option of the single-block path -- is the
 * block's preconditioner.  A context holds one Schwarz preconditioner, so two of them need two contexts.
 *
 *   fedd_matrix_import    dst's system matrix <- the block stored in src's slot, pattern and values, device to device (no host
 *                         round trip); both contexts on one device, one rank each.  dst must carry a mesh (fedd_mesh_set) without
 *                         ghost nodes whose owned nodes x dofs per node (1 .. 3) equal the block's rows; the block must be square.
 *                         Right-hand side and solution of dst are zeroed and its Dirichlet marks cleared, as by fedd_block_merge;
 *                         the solver setups of dst are dropped.  The generations move as after a fedd_matrix_store in the other
 *                         direction.  A second import of a block whose pattern id has not changed (the slot of
 *                         fedd_assemble_advection in a Newton loop) moves values only and keeps dst's pattern generation, so the
 *                         next fedd_schwarz_setup of dst keeps its structure stage (fedd_schwarz_reuse_info).  The copies run in
 *                         dst's stream behind what src's stream has written, and src's stream waits for them: no host
 *                         synchronisation.  Errors that name the cause: an empty slot, a non-square block, a size mismatch,
 *                         contexts on different devices, more than one rank, a host-only context ("needs a GPU context").
 *   fedd_block_prec_attach
 *                         ctx holds a merged system (fedd_block_merge; block row 0 = n_A rows, block row 1 = n_p rows); velocity
 *                         and schur are contexts on the same device whose systems have n_A and n_p rows.  The pointers are NOT
 *                         owned: destroying ctx leaves the children alive.  fedd_ctx_destroy of a child that is still attached
 *                         first waits for ctx's stream and detaches ctx (whose next preconditioned solve is then the error of a
 *                         context without a preconditioner); detaching before destroying a child remains the orderly way.  While attached, fedd_gmres / fedd_gmres_x0 with use_prec = 1 and fedd_schwarz_apply /
 *                         fedd_schwarz_apply_device on ctx apply the block operator below in the place of ctx's own Schwarz
 *                         preconditioner (which need not exist); fedd_cg on a merged system stays an error.
 *                         Checked at the attach: NULL children, the kind, more than one rank, child meshes that cannot belong to
 *                         ctx (the velocity child's owned nodes differ from ctx's), an unmerged parent, other devices.  Checked at
 *                         EVERY apply, because a child may be set up again between two solves, with errors that name the child: a
 *                         child without a current fedd_schwarz_setup, wrong sizes, an unmerged parent, slot_bt empty or of another
 *                         shape than n_A x n_p (Triangular), more than one rank, a child under FEDD_LEVELS_MULTIPLICATIVE (that
 *                         operator is singular by construction).
 *   fedd_block_prec_detach
 *                         ctx's own preconditioner is in force again (an error in fedd_gmres if none was set up).
 *   fedd_block_prec_info  kind (0: none attached), schur_scale, slot_bt (-1 for Diagonal), applies since the attach.  Needs no
 *                         device; outputs may be NULL.
 *
 * The apply (NORMATIVE; PrecBlock2x2_def.hpp:135-160).  r = [r_u; r_p], z = [z_u; z_p], both contiguous in the merged layout;
 * V and S are the children's Schwarz applies, called on pointers into ctx's device vectors (no staging copy of r or z):
 *     FEDD_BLOCKPREC_DIAGONAL:     z_u = V(r_u)
 *                                  z_p = schur_scale * S(r_p)
 *     FEDD_BLOCKPREC_TRIANGULAR:   s   = S(r_p)
 *                                  z_p = schur_scale * s                                         (rounded)
 *                                  t_i = r_u,i - (sum_k B^T_ik z_p,col(k))     on the rows that are no Dirichlet rows of ctx's system
 *                                  t_i = r_u,i                                  on Dirichlet rows (the reference's B^T has had
 *                                                                               setLocalRowZero there, BCBuilder_def.hpp:653-707;
 *                                                                               the stored slot has not)
 *                                  z_u = V(t)
 * z_p and t are written by ONE kernel, a single pass over the rectangular CSR of slot_bt that reads s, r_u and the Dirichlet
 * marks.  Its row sums are those of fedd_matrix_apply: the same group of lanes per row (8 for rows of at most 32 entries, else
 * 16), each lane adding its products in ascending column order, the same fixed tree; every product is rounded before it is
 * added (no contraction) and the sum is rounded before the subtraction.  So B^T z_p is bit for bit what
 * fedd_matrix_apply(ctx, slot_bt, 1.0, z_p) returns, and two applies agree bit for bit whenever the children's do
 * (FEDD_COMBINE_RESTRICTED one-level children do).  Bytes: 12 nnz(B^T) + 4 (n_A + 1) + 4 n_A + 16 n_A + 16 n_p.
 *
 * schur_scale: one-level and additive two-level Schwarz are homogeneous of degree -1 in the matrix, S_{aM} = S_M / a.  The Schur
 * child holds the POSITIVE definite (1/nu) M_p, the caller passes schur_scale = -1, and the result is what the reference gets
 * from -(1/nu) M_p -- without the local and coarse factorisations ever seeing a negative definite matrix.
 *
 * Ordering: while attached, the children's apply kernels are enqueued in ctx's stream, so V, S and the kernel between them are
 * ordered by the stream alone -- no event and no host synchronisation inside the Krylov loop -- and fedd_sync(ctx) covers them
 * (it also waits for the children's own streams).  What a child did in its own stream before (import, Dirichlet rows, setup) is
 * ordered in front by one event per fedd_schwarz_setup of the child.  The caller synchronises ctx (fedd_sync, or a solve that
 * returned x) before it changes a child.
 * ---------------------------------------------------------------------------------------------- */
#define FEDD_BLOCKPREC_DIAGONAL 1
#define FEDD_BLOCKPREC_TRIANGULAR 2
int fedd_matrix_import(fedd_ctx* dst, fedd_ctx* src, int src_slot);
int fedd_block_prec_attach(fedd_ctx* ctx, int kind, fedd_ctx* velocity, fedd_ctx* schur, double schur_scale, int slot_bt);
int fedd_block_prec_detach(fedd_ctx* ctx);
int fedd_block_prec_info(fedd_ctx* ctx, int* kind, double* schur_scale, int* slot_bt, int64_t* n_applies);

/* ------------------------------------------------------------------------------------------------
 * FSI coupling (one rank, geometry-explicit, four blocks): the matched interface of a fluid and a structure context, the
 * coupled system, and the FaCSI preconditioner.  Replaces MeshInterface::determineInterfaceParallelAndDistance
 * (feddlib/core/Mesh/MeshInterface_def.hpp), FE::assemblyFSICoupling / FE::assemblyDummyCoupling as FSI::assemble places them
 * (feddlib/problems/specific/FSI_def.hpp:223-318), FSI::addInterfaceBlockRHS, Preconditioner::buildPreconditionerFaCSI
 * (Preconditioner_def.hpp:789-971) and the geometry-explicit branch of PrecOpFaCSI::applyImpl (PrecOpFaCSI_def.hpp:367-589).
 * The FSI problem class, its TimeProblem and advanceInTimeFSI are NOT built; these entries are what they will call.
 *
 *     [ F    B^T  0    C1^T ] [u]        C1   : n_l x n_u, +1 at (lambda-dof, fluid interface dof)
 *     [ B    C    0    0    ] [p]        C1^T : its transpose
 *     [ 0    0    S    C3^T ] [d]        C2   : -(1/dt) at (lambda-dof, structure interface dof)
 *     [ C1   0    C2   D    ] [l]        C3^T : -1 at (structure interface dof, lambda-dof)
 *                                        D    : 1 on the diagonal of uncoupled lambda-dofs (assemblyDummyCoupling), else no entry
 *
 * NORMATIVE -- the match.  fedd_interface_match(fluid, structure, n_flags, flags): per flag, in the order given, the nodes of
 * each context that carry the flag (bcflag_uni of fedd_mesh_set), at the REFERENCE coordinates (those of the last
 * fedd_mesh_set*, not the moved ones), ordered lexicographically by (x, y[, z]) with exact double comparison and paired by
 * rank -- the reference's std::sort on vec_dbl followed by pairing by position.  The result is two tables of owned
 * (unique-map) node ids in interface order, iface_f[k] and iface_s[k], the flags concatenated; interface dof dim * k + c is
 * component c of pair k.  They are formed on the device (rank, then scatter) and read back once: what is kept are the host
 * copies, which fedd_interface_match_get serves and from which fedd_fsi_merge derives the dof maps its kernels read; no kernel
 * reads the tables themselves.  Both contexts keep a reference to the same table.  The call first releases the earlier match of
 * BOTH contexts; a call that then fails (unequal counts, identical coordinates, ...) leaves both without one.  The rank is formed by counting,
 * rank_i = #{ j : p_j <lex p_i }, one lane per interface node against LDS tiles of 1024 points: deterministic, quadratic in the
 * interface only.  Paired points need NOT coincide (the reference does not check it): fedd_interface_match_info returns the
 * largest Euclidean distance between paired points so that a caller can.
 *   fedd_interface_match_sizes  pairs, flags of the match, dofs per interface node (= dim); on either context of the match.
 *   fedd_interface_match_get    iface_f[n], iface_s[n], flag_ptr[n_flags + 1] (the pairs of flag i are [flag_ptr[i], flag_ptr[i + 1]));
 *                               outputs may be NULL.
 *   fedd_interface_match_info   have (0 / 1), pairs, the largest pair distance, the points per LDS tile.  Needs no device.
 * Lifetime: fedd_mesh_move KEEPS the table; fedd_mesh_set* on either context releases it on both, and a coupled system built on
 * it is an error at the next fedd_fsi_merge and at the next FaCSI apply -- never a dangling pointer.  At the apply a
 * fedd_mesh_set* on a child is reported as "the merge is older than the <child>'s mesh", a table released by a new
 * fedd_interface_match as "the matched interface ... has been released".
 * Errors that name the cause: different counts per flag (the flag and both counts), two nodes of one side with identical
 * coordinates (both node ids), an empty interface, contexts on different devices, more than one rank, a host-only context
 * ("needs a GPU context"), a context without a mesh, the same context twice, meshes of different dimension.
 *
 * The coupled context is an ordinary fedd_ctx that never gets a mesh: system matrix, right-hand side, solution and Dirichlet
 * marks are those of the four-block system; fedd_gmres*, fedd_spmv, fedd_csr_get, fedd_rhs_* work on it as on any system; the
 * entries that need a mesh refuse it by name.
 *   fedd_fsi_merge(cpl, fluid, structure, dt, coupled_mask)
 *       cpl's system <- the merged CSR of fluid's current system (the merged [F B^T; B C] of fedd_block_merge with its wall
 *       Dirichlet rows applied; an unmerged fluid is an error), structure's current system, and the coupling entries; device to
 *       device, ordered as fedd_matrix_import orders its copies; columns ascending within a row.  Rows that are Dirichlet rows of
 *       fluid / structure stay unit rows and get NO C1^T / C3^T entry (setBoundariesSystem on the block system); their marks are
 *       copied, lambda-rows carry none.  The children's right-hand sides are copied, the lambda part is zero, the solution is
 *       zeroed.  coupled_mask[n_l] (bytes; NULL = all coupled): 0 makes lambda-dof k uncoupled -- no entries in C1, C1^T, C2, C3^T
 *       and a 1 on the lambda diagonal.  The coupling values are exactly 1.0, -1.0 and -(1.0 / dt).  A second merge of the same
 *       children whose patterns, Dirichlet marks on the interface, match and mask have not changed moves values only and keeps
 *       cpl's pattern generation (the rule of fedd_matrix_import); fedd_fsi_info reports it.
 *       Errors: dt <= 0, no match between exactly these two contexts (or a released one), a child without a system, an
 *       unmerged fluid, more than one rank, other devices, a host-only context.
 *   fedd_fsi_interface_rhs(cpl, d_old_structure[n_s])
 *       rhs_l[k] = (-(1.0 / dt)) * d_old[sdof(k)] on coupled dofs, 0 elsewhere (FSI::addInterfaceBlockRHS, C2 d_s^n); the
 *       coefficient is formed first, the product rounded once.
 *   fedd_fsi_info  n_u, n_p, n_s, n_l, offsets[4] of the blocks u, p, d, l in the vectors, whether the last merge moved values
 *       only, merges that did since the context was made.  Needs no device; outputs may be NULL.
 *
 * NORMATIVE -- FaCSI.  fedd_fsi_prec_attach(cpl, fluid, structure) / _detach / _info, with the ownership and ordering rules of
 * fedd_block_prec_attach: the children are not owned, destroying an attached child detaches, the children's apply kernels run
 * in cpl's stream behind one event per child setup, no host synchronisation in the Krylov loop.  While attached, fedd_gmres[_x0]
 * with use_prec = 1 and fedd_schwarz_apply[_device] on cpl apply (PrecOpFaCSI_def.hpp:414-589), with S~ and F~ the children's
 * Schwarz applies (F~ the monolithic one on fluid's merged velocity-pressure system), c2 = -(1.0 / dt):
 *     y_d       = S~(x_d)
 *     g_k       = x_l,k - c2 * y_d[sdof(k)]                      coupled k   (Y_l = X_l - C2 Y_s; the product is rounded first)
 *     t         = [x_u; x_p] with t_u[fdof(k)] <- g_k            coupled k   (the two C1^T updates of :504-507)
 *     [y_u;y_p] = F~(t)
 *     z_r       = (x_u,r - (B^T y_p)_r) - (F y_u)_r              on the rows r = fdof(k) only; F, B^T as they stand in cpl's CSR
 *     y_l,k     = z_fdof(k)                                      coupled k
 *     y_l,k     = x_l,k                                          uncoupled k
 * The last line DEVIATES from the reference, which returns 0 there and so makes the operator singular.  The C3^T coupling of
 * the d block is dropped, as in the reference: with exact child inverses A P^-1 x equals x in the u, p and l blocks and differs
 * by C3^T y_l in the d block.  g and the injection are one kernel; z and y_l are one kernel with a group of 8 lanes (16 for rows
 * of more than 32 entries) per interface row over cpl's CSR, columns < n_u + n_p only: the two row sums are formed separately,
 * each lane adds its products in ascending column order, one fixed tree per sum, no contraction -- two applies agree bit for bit
 * whenever the children's do.  Only n_l rows of F and B^T are read, not the whole blocks.
 * The caller gives fluid homogeneous Dirichlet rows on the interface velocity dofs AFTER the merge and BEFORE
 * fedd_schwarz_setup(fluid): the reference's faCSIBCFactory_.  On the merged fluid system that is fedd_dirichlet_rows with the
 * rows dim * iface_f[k] + c of the table of fedd_interface_match_get (fedd_dirichlet_nodes addresses one dof per node of a
 * merged system).  The attach does not do it.
 * Checked at every apply, with errors that name the child: a child without a current fedd_schwarz_setup, sizes that no longer
 * fit the merge, a merge older than a child's mesh, a released match, FEDD_LEVELS_MULTIPLICATIVE children.
 * ---------------------------------------------------------------------------------------------- */
int fedd_interface_match(fedd_ctx* fluid, fedd_ctx* structure, int n_flags, const int32_t* flags);
int fedd_interface_match_sizes(fedd_ctx* ctx, int64_t* n_pairs, int* n_flags, int* dofs_per_node);
int fedd_interface_match_get(fedd_ctx* ctx, int32_t* iface_fluid, int32_t* iface_structure, int64_t* flag_ptr);
int fedd_interface_match_info(fedd_ctx* ctx, int* have, int64_t* n_pairs, double* max_pair_distance, int* tile_points);
int fedd_fsi_merge(fedd_ctx* cpl, fedd_ctx* fluid, fedd_ctx* structure, double dt, const uint8_t* coupled_mask);
int fedd_fsi_interface_rhs(fedd_ctx* cpl, const double* d_old_structure);
int fedd_fsi_info(fedd_ctx* cpl, int64_t* n_u, int64_t* n_p, int64_t* n_s, int64_t* n_l, int64_t* offsets, int* last_values_only,
                  int64_t* n_values_only);
int fedd_fsi_prec_attach(fedd_ctx* cpl, fedd_ctx* fluid, fedd_ctx* structure);
int fedd_fsi_prec_detach(fedd_ctx* cpl);
int fedd_fsi_prec_info(fedd_ctx* cpl, int* attached, int64_t* n_applies);
/* The structures that depend on the mesh alone are built once per mesh, at the first call that needs them, and reused by every
 * later assembly: the node -> element adjacency (fedd_pattern_build) and the element-major tile structures of the assembly
 * kernel (fedd_assemble, P1 forms).  Their wall time (ms, device synchronised before and after) is not part of a steady-state
 * step; a driver that assembles once (the reference's do: laplace/main.cpp:199-208) pays it once.  tiles_state: 0 = not built
 * (yet), 1 = built, -1 = the mesh does not fit the tile limits (pair kernels are used).  Outputs may be NULL.  Both are built
 * by device kernels (option "asm_tiles_host" 1: the tile structures by the round-3 host builder, for A/B). */
int fedd_mesh_setup_info(fedd_ctx* ctx, double* adjacency_ms, double* tiles_ms, int* tiles_state, int64_t* n_tiles);
/* how the last solve ended: floor_reached = 1 when the s-step solver stopped because b - A x had reached its rounding floor
 * (the recurrence residual kept falling, the true residual did not follow, and a restart from the true residual did not help
 * either; relres_out of that solve is the TRUE residual and may exceed rtol by up to 100x), 2 when three restart cycles in a
 * row made no progress; recurrence_relres = the recurrence residual at that point (-1 otherwise); outputs may be NULL */
int fedd_gmres_status(fedd_ctx* ctx, int* floor_reached, double* recurrence_relres);
/* The second level alone, z = Phi K0^-1 Phi^T r: FROSch's "Only apply coarse", which the reference uses for
 * "Level Combination" = "Multiplicative" (LinearSolver_def.hpp:98-104: one coarse pre-apply of the right-hand side into the
 * solution vector, then the solve).  That pre-apply is half of "Multiplicative": the other half is the preconditioner of the
 * solve itself, fedd_schwarz_set_level_combination(FEDD_LEVELS_MULTIPLICATIVE).  r_owned / z_owned both NULL: r = the assembled
 * right-hand side, z -> the device's solution vector (then fedd_gmres_x0(ctx, NULL, NULL, ...) continues from it).  Needs
 * fedd_schwarz_setup(two_level = 1). */
int fedd_schwarz_coarse_apply(fedd_ctx* ctx, const double* r_owned, double* z_owned);
/* the orthogonalisation in use ("gmres_kind") and, for the s-step form, its block length and the blocks of the last solve
 * (all, and those that were cut short because the block basis became numerically dependent); outputs may be NULL */
int fedd_gmres_info(fedd_ctx* ctx, int* kind, int* s, int* blocks, int* cut_blocks);
/* blocks of the last s-step solve orthogonalised with three sweeps instead of four (option "gmres_fuse": k_blockfuse) */
int fedd_gmres_fused_blocks(fedd_ctx* ctx, int* blocks);
/* One block of an s-step solve (gmres_kind 2), copied stage by stage for the tests.  block >= 0 arms the capture for the
 * block-th orthogonalised block of the next s-step solve (counted as fedd_gmres_info counts blocks, from 0); that solve
 * consumes the arm whether it reaches the block or not.  block < 0 disarms and frees the copies.  The armed solve makes the
 * launches of an unarmed one, with the same arguments in the same order; the copies are device-to-device on its stream
 * between them.  One rank, one right-hand side: an arm on a context of several ranks and an armed stacked solve are errors.
 * fedd_gmres_capture_info: out = { captured (0/1), n, ldv, k, sa_req, S, m, fused } -- rows and leading dimension of the
 * basis, final basis vectors before the block, block columns asked for, block size of the kernels, restart length, and
 * whether k_blockfuse ran.
 * fedd_gmres_capture_get copies one piece to the host (cap: doubles `out` holds; too few is an error).  Column-major
 * pieces have ldv rows per column (rows n .. ldv - 1 are padding), coefficient pieces are row-wise with S entries a row:
 *   "V0"   basis columns 0 .. k + sa_req - 1 before the first dot sweep;  "C0" the column behind them (the canary; not
 *          captured when the block ends at the last column of the basis, k + sa_req = m + 1)
 *   "P1" / "P2"   [Q W]^T W after the first / second reduction, (k + sa_req) x S
 *   "CF1" "RI1" "SA1"   after pass 1: coefficients k x S, inverse factor S x S, accepted columns
 *   "W1"   block columns k .. k + sa_req - 1 after the first update, then the canary column if there is one;  columns
 *          SA1 .. sa_req - 1 of a cut block are not written by the updates: they still hold the operator's products
 *   "CF2" "RI2" "TH"   after pass 2, TH = the S shifts;  "SA2" two values: accepted columns on the device and as the host reads them
 *   "W2"   as W1, after the last update
 *   "H"    raw Hessenberg columns 0 .. k + max(SA2, 1) - 2, leading dimension m + 1 (shifts folded in; the solver neither
 *          writes nor reads below the sub-diagonal: whatever the array held stays there)
 *   "VEND" basis columns 0 .. k + SA2 - 1 after the last update */
int fedd_gmres_capture_arm(fedd_ctx* ctx, int block);
int fedd_gmres_capture_info(fedd_ctx* ctx, int64_t* out);
int fedd_gmres_capture_get(fedd_ctx* ctx, const char* what, double* out, int64_t cap);

/* "apply_gather" 0 (default) = fedd_schwarz_apply and GMRES keep the atomicAdd combine for Full and Averaging, 1 = they use the
 * park + gather kernels (bitwise reproducible); "apply_full_kind" 0 = the matrix-core park kernel for subdomains that share their
 * inverse, the one-workgroup kernel for the rest, 1 = the one-workgroup kernel only, 2 = the matrix-core kernel wherever an
 * inverse is shared (an error at the apply if the setup kept no shared inverses, "schwarz_dedupe" 0).
 * tuning knobs (A/B tests), 0 is the default of each: "spmv_kind" 0 = CSR-window (CSR-stream when a row has more than 256 entries), 1 = row-per-lane-group, 2 = CSR-stream;
 * "pat_hash" 1 (default) = node pattern of vertex-only elements merged through a hash table of list positions (symbolic.hip), 0 = ordered insertion;
 * "asm_tiles" 1 (default) = the P1 Laplace / vector-Laplace / elasticity forms are assembled element-major over tiles of ~27 nodes
 * (every element of a tile evaluated once, contributions gathered per CSR slot from lists built once per mesh), 0 = the pair
 * kernels (0 or 1, any other value is an error); "asm_kind" 0 (default) = tiles where "asm_tiles" and the form allow, else pair-parallel
 * assembly (slot-addressed accumulation for the block forms -- elasticity, B / B^T --, slot sweep for the scalar forms), 2 = slot
 * sweep always, 3 = slot-addressed wherever it fits (2 and 3 never take the tiles; any other value is an error); "apply_kind" 0 = restricted Schwarz
 * apply by the setup's outcome (batched matrix-core kernel when at most a quarter of at least 4096 subdomains have distinct
 * local matrices -- on the batch table of the setup, k_apply_bt, when every subdomain conforms to its representative, on chunk
 * records, k_apply_mfma, otherwise --, else the flat streaming kernel), 1 = strided, 2 = flat without the compact LDS layout,
 * 4 = matrix-core kernel whenever the inverses are shared (any number of subdomains), 6 = as 4, with the chunk-record kernel
 * k_apply_mfma also where the batch table exists (A/B and tests; same bits), any other value is an error; "apply_bt" 1
 * (default) = the setup builds the batch table (0: never); "apply_span" places per workgroup of the matrix-core kernels
 * (multiples of 16; 0 = one round of workgroups with the batch table, 32 / 64 / 96 / 128 by the number of subdomains without);
 * "md2_gy" column groups in flight per row block of the
 * Gram-Schmidt dot sweep (0 = by vector length);
 * "gmres_hostwrite" 1 (default) = the solver's small kernel writes the three numbers of the host's lagged convergence test
 * into mapped pinned memory itself, 0 = an asynchronous copy per iteration;
 * "spmv_pattern" 1 (default) = column patterns for matrices beyond the Infinity Cache (fedd_spmv_patterns), 2 = for every
 * matrix, 0 = off; "spmv_pat_nu" / "spmv_win_nu" window sizes of the pattern / per-entry SpMV kernels (0 = default); "inv_kind" 0 = scalar-pivot local inverses that drop finished overlap rows, 1 = rank-4 block sweep on the
 * matrix cores, 2 = scalar-pivot without dropping rows;
 * "gmres_kind" 0 = two-pass Gram-Schmidt with the second pass delayed (DCGS2), 1 = plain two passes, 2 = s-step GMRES: the
 * basis grows "gmres_s" (1 ... 16; 0, the default: 16 from 1.2 million rows per rank, else 8) vectors at a time -- blocks longer than 8 on the Newton block basis ("gmres_newton" 1, the
 * default: shifts = Leja-ordered Ritz values of the first gmres_s Arnoldi steps, which run in monomial blocks of at most 8; 0 =
 * monomial basis, blocks of at most 8) -- and each block is orthogonalised by block Gram-Schmidt with two
 * passes (four sweeps over the basis -- three with "gmres_fuse" -- and two reductions per block instead of two sweeps and one reduction per iteration; same
 * iterates as 0 / 1 in exact arithmetic; a block is cut where the squared sine of a new vector against its predecessors falls
 * to "gmres_chol_tol", default 1e-13; the convergence claim is checked against the true residual and the residual returned is
 * the true one; tolerances below 1e-9 / 1e-11 take blocks of at most 5 / 3 vectors, because the recurrence of a longer block
 * loses touch with the true residual there ("gmres_tol_blocks" 0 lifts that cap: measurements held to an iteration count
 * instead of a tolerance); "gmres_fuse" 1 = blocks of 16: the first pass' update and the second pass' dot products run as one
 * sweep (k_blockfuse: three sweeps per block; the second read of a workgroup's rows comes from the Infinity Cache), 0 = four
 * sweeps, -1 (default) = one sweep from 4 million rows per rank on; unless 0 the last update of a block that fills a restart cycle
 * also forms the solution update sum_c y_c V_c (one read of the basis less per cycle); "gmres_dot_own" 1 (default) = the dot
 * sweeps of a block (k_blockdot, and the second walk of k_blockfuse) stream the final basis columns only and take W^T W from the
 * rows of the block they hold in registers, 0 = they stream the block's own columns too (8 n s bytes more per sweep; the same
 * bits either way: an A/B switch); "gmres_spec" n > 0: n operator applications of the next block are put into the
 * stream before the host reads a block's outcome, so that the GPU works through that round trip -- default 0: on one GPU the
 * round trip is not what the step waits for (tools/share_n8.py), an A/B switch for multi-GPU runs), see fedd_gmres_info;
 * "box_kind" 0 = Schwarz boxes from one lattice over the nodes of all ranks, 1 = a lattice per rank;
 * "asm_lds_kb" (default 37) = LDS budget in KB of the assembly kernel's contribution park, i.e. rows per workgroup;
 * "spmv_nt" 1 = the window SpMV streams the matrix non-temporally (x then survives in L2 between node planes:
 * -6 % back to back on a 1.8 GB matrix, 0 to -4 % inside the solver, slower on matrices that fit the Infinity
 * Cache), 0 = never, -1 (default) = for matrices larger than the Infinity Cache;
 * "spmv_compact" 1 (default) = SpMV streams a solver-private copy of the owned rows without their numerically zero
 * entries (the structural zeros kept for pattern parity, the zeroed entries of Dirichlet rows); fedd_csr_get always
 * returns the reference pattern and values; 0 = stream the parity CSR itself;
 * "spmv_drop_tol" (default 2^-52) = an entry is left out of that copy when |a_ij| <= tol * max_k |a_ik|: 0 drops the
 * entries that are exactly 0.0 only (y then identical bit for bit, for finite x, to the product with the parity CSR), the
 * default also drops cancellation noise below one ulp of the row's largest entry (cf. the reference's optional setZeros_
 * threshold, FE_def.hpp:719-721), which changes y by less than the rounding error of the row sum;
 * "spmv_exact_public" 1 (default) = fedd_spmv itself (Matrix::apply for the caller, residual checks) multiplies with the parity
 * CSR, every stored entry, so its y is the reference's product whatever the solver streams; 0 = fedd_spmv runs the solver's
 * compacted stream (tests and measurements of those kernels);
 * "schwarz_dedupe" 1 (default) = subdomains with the same local matrix share one inverse (see fedd_schwarz_unique), 0 = every
 * subdomain is inverted and stored on its own;
 * "schwarz_reuse" 1 (default) = fedd_schwarz_setup keeps the box lattice, the bins and the overlapping dof lists of the setup
 * before while mesh, pattern and parameters stand (see fedd_schwarz_reuse_info), 0 = they are built by every setup (the same
 * preconditioner bit for bit; the A/B switch).  With several ranks a rank that has it off makes every rank build;
 * "pattern_reuse" 1 (default) = a fedd_pattern_build that repeats the last one keeps the pattern arrays (see
 * fedd_pattern_reuse_info), 0 = every call builds them; "spmv_reuse" 1 (default) = the solver's SpMV stream is verified
 * against the reassembled matrix in one pass and kept (see fedd_spmv_reuse_info), 0 = built for every matrix;
 * "setup_fused" 1 (default) = work of the setup side that two calls would each do is done once: fedd_schwarz_setup's walk over
 * the finished rows (row maxima and hashes of "schwarz_fp_kind" 0) also makes the "spmv_reuse" check the next SpMV would walk
 * them again for, used only while nothing has written the system matrix in between; fedd_assemble_rhs keeps |det B| of every
 * element (8 bytes per element) until fedd_mesh_set* or fedd_mesh_move changes the geometry; fedd_schwarz_setup reads the
 * counts it has before its first host decision back in one copy; 0 = every call for itself, every count with a wait of its
 * own (the same bits everywhere; the A/B switch);
 * "schwarz_fp_kind" 0 (default) = the fingerprints of that sharing are built from one hash per matrix ROW (column offsets and
 * quantised values of all its entries) and the rows' positions in the subdomain, 1 = entry by entry over the entries inside the
 * subdomain (the round-2 form; finds the same classes on the structured grids, four times slower);
 * "halo_overlap" 1 = several ranks, restricted combine: the subdomains that hold no dof of another rank are applied while the
 * ghost entries of r are imported on a second stream, the others after the import (same operator bit for bit); 0 (default) =
 * import, then all subdomains.  The SpMV on row classes does the same with its import of x: all rows while it travels, the
 * rows that read ghost columns once more after it has arrived.  An A/B switch for multi-GPU runs: on one GPU there is
 * nothing to hide;
 * "whole_boxes" 1 (default) = with row ghosts, a box that a rank boundary crosses is built whole (with its full
 * overlap) on every rank that owns a part of it wherever the stored rows reach, 0 = each rank takes its part;
 * "asm_zero_eps" eps > 0 = FE::doSetZeros(eps) (FE_def.hpp:74-79): element contributions of magnitude below eps are set to zero
 * before they are added, in the forms the reference thresholds -- the vector Laplacian (FEDD_FORM_LAPLACE_VEC, :719-721) and the
 * divergence blocks (fedd_assemble_div, :2002-2004, 2032-2034); 0 (default) = off;
 * "asm_p2_elem" 1 (default) = the P2 scalar forms (Laplace, vector Laplace, mass) evaluate every element once, one element per
 * wavefront with the reference gradients and quadrature weights staged in LDS (k_elem_matrix), and the rows are summed from
 * those element matrices through gather lists built once per mesh; 2 = the element matrices, the rows summed by the pair kernels;
 * 0 = the pair kernels alone re-derive the row of every (row, element) pair (any other value is an error);
 * "asm_tiles_host" 1 = the tile structures of the assembly kernel are built by the round-3 host builder instead of the device
 * kernels (A/B and tests; see fedd_mesh_setup_info), 0 (default) = on the device (any other value is an error). */
int fedd_set_option(fedd_ctx* ctx, const char* key, double value);

/* device-time accounting (HIP events on the context's stream around each kernel class) */
/* on = 0 off, 1 every launch, N > 1: the per-iteration classes (SpMV, Schwarz apply, coarse apply,
 * orthogonalisation) are timed on every N-th launch only and fedd_timing_get scales the sampled
 * average by the launches seen (an event pair per launch costs 3-6 % of a solve). */
int fedd_timing_enable(fedd_ctx* ctx, int on);
int fedd_timing_reset(fedd_ctx* ctx);
int fedd_timing_get(fedd_ctx* ctx, int timer, double* total_ms, int64_t* launches);
/* the launches of a class that were actually timed: their device time, their number and the algorithmic bytes their launch
 * sites stated (Gram-Schmidt sweeps: 8 bytes x rows x columns read and written; 0 for classes that state none): the
 * achieved-bandwidth figure of a class is sampled_bytes / sampled_ms, whatever the sampling stride */
int fedd_timing_get_sampled(fedd_ctx* ctx, int timer, double* sampled_ms, int64_t* sampled_launches, double* sampled_bytes);
/* calibration for the roofline figures: GB/s of a read-only stream over a scratch buffer of `bytes` (16-byte
 * non-temporal loads, `reps` launches back to back, best of three batches) on this GPU, i.e. the ceiling that
 * the measured fractions of the 8 TB/s spec can be compared with ("of spec" and "of
 * measured") */
/* column patterns of the solver's compacted SpMV stream (option "spmv_pattern", default 1): rows that repeat their column
 * offsets (col - row) share an offset list, so the stream carries 8 instead of 12 bytes per entry (values per row, exact; a
 * 16-bit pattern id per row).  n_patterns = 0: not in use (option off, no solve yet, or the matrix has no repeated rows);
 * n_rows_explicit = rows that keep explicit column indices. */
int fedd_spmv_patterns(fedd_ctx* ctx, int64_t* n_patterns, int64_t* n_rows_explicit);
/* Row classes of the solver's stream (option "spmv_classes", default on; built with the column patterns, so for matrices beyond
 * the Infinity Cache): rows with the same column pattern AND the same values, bit for bit, share a class -- on a structured
 * grid the assembled matrix has a few thousand distinct rows among millions.  The SpMV then reads a 4-byte (class, pattern) word per row and
 * the row's values from a table of at most 16384 classes instead of 8 bytes per entry; same products, same order: y identical
 * bit for bit.  n_classes = 0: not in use (fewer than 90 % of the rows repeat); n_rows_in_classes: rows served from the table;
 * nnz_streamed_rest: stream entries of the other rows.  Outputs may be NULL.  Option "spmv_keep_dictionary" 1: the pattern
 * dictionary and the classes of the previous matrix are kept while the new matrix still matches them bit for bit (one
 * verifying pass instead of the build -- for drivers that reassemble the same operator); default 0: built for every matrix.
 * Option "spmv_classes_cover" (default 90): the percentage of the rows the classes must cover to be used. */
int fedd_spmv_classes(fedd_ctx* ctx, int64_t* n_classes, int64_t* n_rows_in_classes, int64_t* nnz_streamed_rest);
/* Block-local class lists (option "spmv_cls_lds", default 1): every workgroup of the class kernel copies the values of the
 * classes its rows use to LDS -- a list per block of 1024 (512 at the widest table stride) rows, built once with the classes --
 * and its rows read them from there; rows whose pattern holds offsets d - 1, d, d + 1 take x at d -/+ 1 from the neighbouring
 * lanes.  Same products, same order: y identical bit for bit.  A block with more classes than its list holds (160 / 64 / 31 at
 * table stride 8 / 16 / 48; development option "spmv_cls_lds_cap": fewer), or with a row in no class, is flagged and runs the
 * table path.  n_blocks_lds / n_blocks_fallback: blocks with a list / flagged; both 0: not in use.  Outputs may be NULL. */
int fedd_spmv_cls_blocks(fedd_ctx* ctx, int64_t* n_blocks_lds, int64_t* n_blocks_fallback);
/* The solver's stream is kept from one matrix to the next while the pattern, the sizes and the SpMV options stand (option
 * "spmv_reuse", default 1): the first SpMV after the matrix changed walks the ASSEMBLED rows once, applies the drop rule and
 * checks every kept entry against what the stream already holds -- count and columns always; with row classes in use also
 * the values, bit for bit (nothing is written: the stream is the one a build would produce); without classes the values are
 * written to their places (same graph, new numbers: Newton steps, time loops).  Any mismatch runs the full build.
 * last_reused: 1 if the stream in use was kept; n_reused: keeps since the context was made.  Outputs may be NULL. */
int fedd_spmv_reuse_info(fedd_ctx* ctx, int* last_reused, int64_t* n_reused);
/* What option "setup_fused" (fedd_set_option) has done since the context was made: n_walks = Schwarz setups whose row walk also
 * made the SpMV stream check; n_checks_used = of those, the checks the next SpMV found still valid (no write to the system matrix
 * in between) and used in place of a walk of its own; n_absdet_kept = fedd_assemble_rhs calls that found |det B| of the elements
 * kept from an earlier call.  Outputs may be NULL. */
int fedd_setup_fused_info(fedd_ctx* ctx, int64_t* n_walks, int64_t* n_checks_used, int64_t* n_absdet_kept);
/* bytes per column index of the solver's SpMV stream: 0 = column patterns in use (above), 2 = 16-bit offsets from a base per
 * window of the stream (option "spmv_col16", default 1; 10 instead of 12 bytes per entry) in every window whose columns span less
 * than 65536 -- any mesh numbered with some locality; entries_with_32bit_columns (nullable) = the entries of the windows that
 * span more (ghost columns on several ranks, far neighbours) and keep plain indices --, 4 = plain indices throughout.  Replaces
 * nothing in the reference (Tpetra's local column indices are 32-bit, feddlib/core/LinearAlgebra/Matrix_def.hpp:88-92); a
 * property of this library's stream. */
int fedd_spmv_col_bytes(fedd_ctx* ctx, int* bytes_per_column_index, int64_t* entries_with_32bit_columns);

int fedd_read_bandwidth(fedd_ctx* ctx, int64_t bytes, int reps, double* gb_per_s);

/* multi-GPU: exchange plan for the owned/ghost split (import of ghost x / r entries before SpMV
 * and Schwarz -- the Tpetra Import behind Matrix::apply, Matrix_def.hpp:245-254; GMRES dots are
 * ncclAllReduce).  After fedd_mesh_set:
 *   fedd_halo_set_owners   owner rank of every repeated node (what the Tpetra directory knows);
 *   fedd_halo_exchange_setup  swaps the request lists over RCCL and finalises the plan;
 * or, transport-agnostic (used by the gloo CPU tests): fedd_halo_requests_sizes/_get on every
 * rank, all-to-all of the lists by the caller, fedd_halo_requests_set.
 * fedd_mesh_structured_owner: owner of structured-grid nodes under the lowest-rank rule. */
/* Host-staged transport for functional tests of the N > 1 path where RCCL cannot run (several ranks
 * on one GPU, CPU-side harnesses): the same plan, pack / unpack kernels and solver flow, with the
 * two communication steps handed to the caller.  exchange: send_buf / recv_buf are host buffers laid
 * out by send_ptr / recv_ptr (in nodes; multiply by dofs).  With callbacks set, fedd_ctx_create may
 * be given nranks > 1 and a NULL ncclUniqueId.  Production runs use RCCL (no callbacks). */
typedef int (*fedd_exchange_fn)(void* user, int n_peers, const int32_t* peers, const int64_t* send_ptr,
                                const double* send_buf, const int64_t* recv_ptr, double* recv_buf, int dofs);
typedef int (*fedd_allreduce_fn)(void* user, double* buf, int n);
int fedd_comm_set_host_callbacks(fedd_ctx* ctx, fedd_exchange_fn exchange, fedd_allreduce_fn allreduce, void* user);

/* one-rank RCCL self-test on the context's device and stream: communicator, grouped send / receive, in-place
 * all-reduce, all-gather -- the call shapes of the halo import and the Gram-Schmidt reductions (what can run of the
 * RCCL path on a one-GPU box).  max_abs_err = deviation from the expected values (0 when RCCL works). */
int fedd_rccl_selftest(fedd_ctx* ctx, int n, double* max_abs_err);
/* The collectives of the N > 1 path on the context's OWN communicator, in the shapes the solver uses them: the in-place
 * all-reduce of the Gram-Schmidt reductions, a grouped send / receive with every other rank (the halo import of a block that
 * touches all others) and a ring shift, n doubles each; max_abs_err = largest deviation from the expected values (0 on one
 * rank).  A pre-flight for multi-GPU runs (bench.py calls it under a watchdog before the first step): every rank must call it. */
int fedd_comm_selftest(fedd_ctx* ctx, int n, double* max_abs_err);

int fedd_mesh_structured_owner(int dim, const int* decomp, const int* cells, int64_t n,
                               const int64_t* gid, int32_t* owner_rank);
int fedd_halo_set_owners(fedd_ctx* ctx, int64_t n_rep, const int64_t* gid_rep, const int32_t* owner_rep);
int fedd_halo_requests_sizes(fedd_ctx* ctx, int64_t* count_to_rank /*[nranks]*/);
int fedd_halo_requests_get(fedd_ctx* ctx, int64_t* gids /*concatenated by rank*/);
int fedd_halo_requests_set(fedd_ctx* ctx, const int64_t* count_from_rank /*[nranks]*/, const int64_t* gids);
int fedd_halo_exchange_setup(fedd_ctx* ctx);
int fedd_halo_plan_sizes(fedd_ctx* ctx, int* n_peers, int64_t* n_send_total, int64_t* n_recv_total);
int fedd_halo_plan_get(fedd_ctx* ctx, int32_t* peers, int64_t* send_ptr, int32_t* send_lid,
                       int64_t* recv_ptr, int32_t* recv_lid);

#ifdef __cplusplus
}
#endif
#endif /* FEDD_HIP_H */
