// Internal declarations shared by the translation units of libfedd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <cstdio>
#include <cstdarg>
#include <memory>
#include "../../include/fedd_hip.h"

struct ncclComm;

namespace fedd {

void set_error(const char* fmt, ...);

#define FEDD_HIP(call)                                                                          \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess) {                                                                \
            fedd::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

#define FEDD_CHECK(cond, ...)                                                                   \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            fedd::set_error(__VA_ARGS__);                                                       \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

#define FEDD_TRY(expr)                                                                          \
    do {                                                                                        \
        int r__ = (expr);                                                                       \
        if (r__) return r__;                                                                    \
    } while (0)

// the argument checks of the entry points (fsi.hip words its own for calls that take several contexts)
#define NEED_DEVICE(c)                                                                           \
    FEDD_CHECK((c) && (c)->device >= 0,                                                          \
               "this call needs a GPU context (fedd_ctx_create with device >= 0); there is no CPU fallback")
#define ONE_RANK(c, who) FEDD_CHECK((c)->nranks == 1, "%s: one rank only (a context with %d ranks was given)", who, (c)->nranks)
#define CHECK_SLOT(s) FEDD_CHECK((s) >= 0 && (s) < fedd::MAX_AUX, "matrix slot %d out of range", (s))

// A device allocation that remembers its size; grows on demand, never shrinks.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;             // owns its allocation: no copies (a copy once leaked the halo buffers)
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t n) {
        if (n <= cap && p) return 0;
        if (p) {
            hipError_t e = hipFree(p);
            (void)e;
            p = nullptr;
            cap = 0;
        }
        if (n == 0) n = 1;
        FEDD_HIP(hipMalloc((void**)&p, n * sizeof(T)));
        cap = n;
        return 0;
    }
    void release() {
        if (p) {
            hipError_t e = hipFree(p);
            (void)e;
        }
        p = nullptr;
        cap = 0;
    }
};

// Gather lists of an element-major assembly path (gather_lists_ensure below, gather_lists.hpp; DESIGN.md section 4 "Gather lists
// and the row walk" has the format): soff [node-level nnz + 2], src [adjacency entries * nen + 2], and the mesh and pattern they
// were built for (pattern_gen, or GATHER_NODE_PATTERN for a node-level pattern, which follows from the mesh alone)
constexpr int GATHER_MAX_DEG = 4095;        // incident elements of a node: the adjacency entry has 12 bits
constexpr int GATHER_MAX_SRC = 65535;       // sources of a node, deg * nen: the starts have 16 bits
constexpr uint64_t GATHER_NODE_PATTERN = ~(uint64_t)0;
struct GatherLists {
    enum { NOT_BUILT = 0, READY = 1, NO_FIT = -1 };   // NO_FIT: a node beyond the limits above, or nothing to build the lists on
    DevBuf<uint16_t> soff, src;
    uint64_t mesh_id = 0, pattern = 0;
    int state = NOT_BUILT;
    bool ready_for(uint64_t m, uint64_t p) const { return state == READY && mesh_id == m && pattern == p; }
    void reset() { state = NOT_BUILT; }     // (the buffers stay: the next mesh is usually of the same size)
};

constexpr int MAX_BC = 16;
constexpr int MAX_DOFS = 3;

// The Dirichlet conditions of a call, by value into its kernel: condition k holds on the nodes with flag[k], for the components
// with mask[k * dofs + comp] != 0 (no mask given: all), with value[k * dofs + comp].  The first condition that fits decides.
struct BcTable {
    int n, dofs;
    int32_t flag[MAX_BC];
    int32_t mask[MAX_BC * MAX_DOFS];
    double value[MAX_BC * MAX_DOFS];
};
inline BcTable bc_table_fill(int dofs, int n_bc, const int32_t* flags, const int32_t* comp_mask, const double* values) {
    BcTable b;
    b.n = n_bc;
    b.dofs = dofs;
    for (int k = 0; k < n_bc; ++k) {
        b.flag[k] = flags[k];
        for (int d = 0; d < dofs; ++d) {
            b.mask[k * dofs + d] = comp_mask ? comp_mask[k * dofs + d] : 1;
            b.value[k * dofs + d] = values[k * dofs + d];
        }
    }
    return b;
}
// the condition of component comp of a node with this flag, -1: none
__device__ __forceinline__ int bc_hit(const BcTable& b, int32_t flag, int comp) {
    int hit = -1;
    for (int k = 0; k < b.n; ++k)
        if (hit < 0 && b.flag[k] == flag && b.mask[k * b.dofs + comp]) hit = k;
    return hit;
}
constexpr int SPMV_PAT_LMAX = 48;       // longest offset list of the SpMV pattern table (spmv.hip SPAT_L)
constexpr int SCHWARZ_NMAX = 256;  // largest overlapping subdomain (dofs) the register / LDS dense kernels take
constexpr int SCHWARZ_NMAX_BIG = 1024;  // ... and the batched matrix-core inversion of the large-subdomain path

struct HaloPlan {
    std::vector<int32_t> peers;
    std::vector<int64_t> send_ptr, recv_ptr;   // per peer, in dofs-per-node = 1 units (nodes)
    std::vector<int32_t> send_lid, recv_lid;   // owned node ids to pack / ghost node ids to fill
    std::vector<int64_t> req_count, req_gid;   // what this rank asks of every other rank (by rank, gid asc)
    DevBuf<int32_t> d_send_lid, d_recv_lid;
    DevBuf<double> d_send_buf, d_recv_buf;     // sized for MAX_DOFS * nodes
    bool ready = false;
    // back to the empty plan; the device buffers are kept (DevBuf grows on demand and is freed with the context)
    void reset() {
        peers.clear();
        send_ptr.clear();
        recv_ptr.clear();
        send_lid.clear();
        recv_lid.clear();
        req_count.clear();
        req_gid.clear();
        ready = false;
    }
};

// a device CSR matrix held beside the system matrix (blocks of a mixed problem before the merge)
struct DevCsr {
    DevBuf<int32_t> rowptr, colind;
    DevBuf<double> val;
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    int max_row_nnz = 0;
    bool valid = false;
    int dofs = 0, block_mode = -1;  // velocity-space matrices (fedd_matrix_store of a fedd_pattern_build pattern, fedd_assemble_advection): dofs per node and
    uint64_t mesh_id = 0;           // FEDD_BLOCK_* of the pattern, and the fedd_ctx::mesh_id it was built on; block_mode -1 = another origin
    uint64_t pattern_id = 0;    // drawn from fedd_ctx::pattern_counter whenever rowptr / colind are rewritten: equal ids = same pattern
    uint64_t value_id = 0;      // drawn from fedd_ctx::value_counter by every writer of val: equal ids = same contents (timestep.hip)
};
constexpr int MAX_STAGES = 8;   // stages a single-step (Runge-Kutta) step may store (singlestep.hip): buffers of their own, not slots
constexpr int MAX_AUX = 7;      // A, B, B^T, C, the linearised velocity block F = A + rho (N | N + W) of Navier-Stokes, and of its time loop
                                // the velocity mass matrix (5) and the time-combined constant velocity block (cm M) + (ca A) (6)

// regular lattice of the coarse level: g cells and np = g + 1 points per direction (1 point in
// directions beyond dim), over the global bounding box [lo, lo + L]
struct CoarseGeom {
    int dim = 0;
    int g[3] = {1, 1, 1}, np[3] = {1, 1, 1};
    double lo[3] = {0, 0, 0}, L[3] = {1, 1, 1};
    int reduced = 0;   // GDSW family: 1 = RGDSW (coarse dofs on the coarse nodes only), 0 = GDSW (every interface entity)
};
constexpr int COARSE_MAX_DOFS = 8192;   // dense K0^-1: 8192^2 * 8 B = 512 MiB

struct TimerSlot {
    double total_ms = 0.0;
    int64_t launches = 0;   // launches that were timed
    int64_t seen = 0;       // launches that passed through (timed or not)
    double bytes = 0.0;     // algorithmic bytes of the timed launches (classes whose launch sites state them)
    struct Pair {
        hipEvent_t first, second;
        bool cont;          // second half of a launch that was interrupted (e.g. by a collective): time, not a launch
    };
    std::vector<Pair> pending;
};

// The solver's SpMV stream (spmv.hip): a solver-private compacted copy of the owned rows -- the numerically zero entries left
// out (the structural zeros the reference's insertGlobalValues keeps in the pattern, the zeroed entries of Dirichlet rows) -- and
// what is built from it.  fedd_csr_get keeps returning the reference pattern; the SpMV streams this one.  It stands from a build
// to the next write to the system matrix (system_written); the options that decide it are members of fedd_ctx, and every one
// of their setters drops it (OPT_DROPS_STREAM).
struct SpmvStream {
    bool valid = false;                         // false after any write to the system matrix (system_written)
    // the kernel the stream takes, recorded at the end of a build and of a kept build: no entries | k_spmv_cls | k_spmv_pat |
    // k_spmv_win with 32-bit | 16-bit columns
    enum Path { EMPTY, CLASSES, PATTERNS, ENTRY32, ENTRY16 } path = EMPTY;
    bool takes(Path p) const { return valid && path == p; }
    bool has_dictionary() const { return valid && (path == CLASSES || path == PATTERNS); }
    // ---- the compacted arrays ----
    int64_t nnz = 0;
    int32_t tot32 = 0;                          // nnz as the last row pointer (lives here: its copy to the device is asynchronous)
    DevBuf<int32_t> d_rowptr, d_col;
    DevBuf<double> d_val;
    bool col16 = false;                         // 16-bit column offsets were built (k_cs_col16): d_col16, and
    DevBuf<uint16_t> d_col16;
    DevBuf<int32_t> d_wbase;                    // ... their bases per window (-1: the window keeps 32-bit columns)
    int32_t max_len = 1;                        // longest row of the compacted stream
    // ---- window -> first row lists ----
    DevBuf<int32_t> d_rows_csr;                 // of the parity CSR (2048-entry windows), once per pattern
    bool rows_csr_ready = false;                // ... cleared by a write to the pattern (system_written)
    int win_nu = 8, pat_nu = 8;                 // windows of the compacted stream: 256 win_nu entries (k_spmv_win), 512 pat_nu values (k_spmv_pat)
    DevBuf<int32_t> d_rows_win, d_rows_pat;     // ... first row of each of those windows
    // ---- column-pattern dictionary and row classes ----
    int32_t npat = 0, nexpl = 0;                // patterns in use (0: dictionary off), rows that keep explicit columns
    int pat_len = SPMV_PAT_LMAX;                // longest pattern in the table
    DevBuf<int32_t> d_pati;                     // slot of row [n] | table min row | pattern of slot | lengths | offset lists | counters (spmv.hip pat_layout)
    DevBuf<uint16_t> d_pat;                     // pattern id per row (0xffff: explicit columns)
    int32_t ncls = 0, cls_rows = 0, cls_rest = 0;   // classes in use (0: off), rows in a class, stream entries of the other rows
    int cls_len = 8;                            // stride of the class table (8, 16 or 48 values)
    DevBuf<uint32_t> d_cls;                     // per row: class << 8 | column pattern (0xffffffff: none)
    DevBuf<uint16_t> d_clspat;                  // column pattern of a class
    DevBuf<double> d_clsval;                    // [classes][cls_len] values of a class
    DevBuf<int32_t> d_clsi;                     // slot of row [n] | table min row | class of slot | counters (spmv.hip cls_layout)
    // ---- block-local class lists (option "spmv_cls_lds", spmv.hip k_cls_blocks): per workgroup of k_spmv_cls_lds the distinct
    //      classes of its rows, whose values the workgroup brings to LDS ----
    bool cls_lds = false;                       // the lists stand for d_cls and the class kernel takes them
    int32_t blk_lds = 0, blk_fallback = 0;      // workgroups with a list | flagged (more classes than the cap, or a row without a class)
    DevBuf<uint16_t> d_cls16;                   // per row: slot in its block's list << 6 | column pattern
    DevBuf<int32_t> d_blkn;                     // per block: classes in its list, -1: flagged
    DevBuf<uint16_t> d_blklist;                 // [blocks][cap of the stride] class ids, ascending
    struct BlkTab { int32_t n = -1, len = 0, cap = 0, lds = 0; } blk_tab;   // rows, stride and cap the lists were built for (n = -1: d_cls was rewritten since), blocks with a list
    // ---- rows that read ghost columns (several ranks, overlapped import) ----
    int32_t nbnd = -1;                          // their number (-1: not listed)
    DevBuf<int32_t> d_bnd;                      // flags / positions [n + 2] | the rows
    // ---- option "spmv_keep_dictionary": the builds the dictionary and the class table on the device come from; they are kept
    //      while the next matrix' stream still matches them bit for bit ----
    struct PatTab { int32_t n = -1, npat = 0, nexpl = 0, len = 0; } pat_tab;    // rows, patterns, explicit rows, longest pattern
    struct ClsTab { int32_t n = -1, len = 0, ncls = 0, rows = 0; } cls_tab;     // rows, stride, classes, classed rows
    // ---- option "spmv_reuse": the stream, its dictionary, classes and row lists are kept from matrix to matrix while this key
    //      stands (spmv_reuse_try): written by a build, dropped by every option setter that invalidates the stream ----
    struct Key {
        bool valid = false;
        uint64_t pattern_gen = 0;
        int64_t n = 0, n_cols = 0, nnz = 0;
        double drop_tol = 0.0;
        bool cls_tried = false;                 // the build ran the class stage: its outcome follows the VALUES, so the keep must find them unchanged
    } key;
    int64_t last_reused = 0, reuse_count = 0;   // the stream in use was kept, not built; streams kept since the context was made
    // ---- build scratch: written and read inside one build only ----
    DevBuf<int32_t> d_wincnt;                   // kept entries per window of the parity CSR -> their offsets
    DevBuf<uint64_t> d_clskey;                  // keys of the class hash table
};

// The matched interface of a fluid and a structure context (fsi.hip fedd_interface_match): both contexts hold the same table.
// fedd_mesh_set* on either side marks it released (valid = false) and lets go of its own reference; a coupled context that was
// merged on it keeps a reference of its own and finds it released at its next merge or apply.
struct IfaceTable {
    bool valid = true;
    int device = -1, dim = 0;
    int64_t n = 0;                              // pairs
    uint64_t uid_f = 0, uid_s = 0;              // fedd_ctx::uid of the two sides
    uint64_t id = 0;                            // process-wide: which match this is
    std::vector<int32_t> h_f, h_s;              // [n] owned node ids of pair k, fluid / structure side (read back from the device)
    std::vector<int32_t> flags;                 // the flags of the match, in the order given
    std::vector<int64_t> flag_ptr;              // [flags + 1] pairs of flag i: [flag_ptr[i], flag_ptr[i + 1])
    double max_dist = 0.0;                      // largest distance between paired points
};

// A preconditioner of a context out of two child contexts applied as blocks (DESIGN.md section 4 "Stored blocks: the lane-group
// row walk and child contexts").  The children are not owned; each keeps its parents in fedd_ctx::prec_parents.
struct PrecChild {
    fedd_ctx* ctx = nullptr;
    uint64_t seen = 0;                          // the child's sw_setup_gen when its own stream was last ordered before the parent's
};
struct AttachedPrec {
    enum { NONE = 0, BLOCK = 1, FACSI = 2 };
    int kind = NONE;
    PrecChild child[2];                         // BLOCK: velocity, Schur complement; FACSI: fluid, structure
    hipEvent_t ev = nullptr;                    // orders a child's own stream before the parent's (one event serves both children)
    int64_t applies = 0;                        // applies since the attach
};

// One block of an s-step solve, copied stage by stage (fedd_gmres_capture_*): device-to-device copies on the solver's stream
// between the launches the block makes anyway.  `buf` holds the pieces one behind the other, piece i at off[i] with len[i]
// doubles (the two d_sa values are stored as int32 in a double's slot); len 0 = not captured.
struct GmresCapture {
    enum Piece { V0, C0, P1, CF1, RI1, SA1, W1, P2, CF2, RI2, SA2, TH, W2, H, VEND, NPIECE };
    int armed = -1;                             // block of the next s-step solve to copy (counted by gmres_blocks); -1: none
    bool captured = false;
    int64_t n = 0, ldv = 0;
    int k = 0, sa_req = 0, S = 0, m = 0, fused = 0;
    int canary = 0;                             // the basis has a column behind the block (k + sa_req <= m): W1 / W2 carry it
    size_t off[NPIECE] = {}, len[NPIECE] = {};
    DevBuf<double> buf;
};

}  // namespace fedd

struct fedd_ctx {
    int device = -1;  // < 0: host-only context (no HIP calls; host logic tests)
    int rank = 0, nranks = 1;
    hipStream_t stream = nullptr;
    ncclComm* comm = nullptr;
    // host-staged transport (functional testing of the N > 1 path without RCCL, e.g. over gloo)
    fedd_exchange_fn cb_exchange = nullptr;
    fedd_allreduce_fn cb_allreduce = nullptr;
    void* cb_user = nullptr;
    std::vector<double> h_send, h_recv;

    // ---- mesh (column-local numbering: owned nodes [0,n_own) in unique-map order, then ghosts
    //      sorted by global id) ----
    int dim = 0, nen = 0;
    int64_t n_elem = 0, n_own = 0, n_node = 0;  // n_node = owned + ghost
    int64_t n_rowg = 0;                         // ghost nodes [n_own, n_own + n_rowg) whose rows are complete here (fedd_mesh_set_rows)
    std::vector<int64_t> h_node_gid;            // [n_node]
    std::vector<int32_t> h_ghost_owner;         // [n_node - n_own]
    fedd::DevBuf<int32_t> d_conn;               // [n_elem*nen]
    fedd::DevBuf<double> d_xyz;                 // [n_node*dim]
    fedd::DevBuf<int32_t> d_flag;               // [n_own] bc flags of owned nodes
    // ---- moving mesh (mesh_move.hip fedd_mesh_move; one rank): d_xyz = x_ref + d of the last move ----
    bool have_xref = false;                     // d_xyz_ref holds what the last fedd_mesh_set* uploaded (copied at the first move: until then d_xyz is it)
    fedd::DevBuf<double> d_xyz_ref, d_xyz_cand; // [n_node*dim] the reference; the candidate of a move (changes places with d_xyz when the check passes)
    fedd::DevBuf<double> d_mv_disp, d_mv_part;  // the displacement in column-local numbering; partial minima of k_move_check | its three results
    fedd::DevBuf<int32_t> d_mv_flag;            // [2] elements with det * det_ref <= 0, the smallest of them
    std::vector<double> h_mv_disp;              // host staging of the permuted displacement (kept: its copy to the device is asynchronous)
    int64_t n_moves = 0;                        // moves committed since the last fedd_mesh_set*
    uint64_t geometry_id = 0;                   // moves committed since the context was made: which coordinates a result belongs to
    double min_det_ratio = 1.0;                 // smallest |det B| / |det B_ref| of the last committed move
    // ---- interface distances and the scaled-Laplace coefficient (interface_distance.hip; one rank) ----
    bool have_idist = false;                    // d_idist holds distances: kept by fedd_mesh_move (nodal values), released by fedd_mesh_set*
    fedd::DevBuf<double> d_idist;               // [n_node] distance of every node to the interface, column-local numbering
    fedd::DevBuf<double> d_ipts;                // [dim][n_interface] the interface points of the last computing call, structure-of-arrays
    int64_t n_interface = 0;                    // ... and their number (0 after fedd_interface_distance_set)
    bool have_lscale = false;                   // d_lscale holds the coefficients of the last FEDD_FORM_LAPLACE_XDIM assembly on this mesh
    fedd::DevBuf<double> d_lscale;              // [n_elem] f per element (k_laplace_scale)

    // ---- node -> (element, local index) adjacency of owned nodes ----
    fedd::DevBuf<int32_t> d_n2e_ptr, d_n2e;     // [n_own+1], [sum]
    int max_deg = 0;
    bool have_adj = false;

    // ---- surface elements (fedd_surface_set): boundary edges / triangles for the surface load vector ----
    bool have_surf = false;                     // a set (possibly empty) has been given for the current mesh
    int surf_nsn = 0;                           // nodes per surface element: dim (P1), 3 / 6 (P2 in 2D / 3D)
    int64_t n_surf = 0;
    fedd::DevBuf<int32_t> d_surf, d_sflag;      // [n_surf*nsn] column-local node ids, [n_surf] flags
    fedd::DevBuf<int32_t> d_sweight;            // [n_surf] local volume elements that hold all vertices of the surface element
    fedd::DevBuf<int32_t> d_s2n_ptr, d_s2n;     // owned node -> (surface element * nsn + local index), ascending: [n_own+1], [sum]
    fedd::DevBuf<double> d_sscal, d_sg;         // per call: [n_surf] scaling * weight, the load table
    fedd::DevBuf<int32_t> d_sgi;                // per call: [n_surf] row of the load table (-1: flag not asked for)

    // ---- CSR (dof level, owned rows) ----
    int dofs = 0, block_mode = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    // with row ghosts the CSR arrays continue past the owned rows: rows [n_rows, n_rows_ext) are those of the
    // row-ghost nodes (read by the Schwarz local matrices only); n_rows / nnz stay the owned part
    int64_t n_rows_ext = 0, nnz_ext = 0;
    int max_row_nnz = 0;
    fedd::DevBuf<int32_t> d_rowptr, d_colind;
    fedd::DevBuf<double> d_val;
    fedd::DevBuf<double> d_rhs, d_x;            // [n_rows]
    fedd::DevBuf<double> d_xcol, d_ycol;        // [n_cols] work vectors with ghost tail
    fedd::DevBuf<int32_t> d_isdir;              // [n_rows] 1 = Dirichlet row
    bool have_pattern = false;
    int whole_boxes = 1;                        // row ghosts: build boxes whole across rank boundaries where the stored rows reach
    fedd::DevBuf<int32_t> d_fbin_ptr, d_fbin_nodes;   // [nsub+1], [row-ghost dofs] other ranks' dofs grouped by box
    int32_t sw_max_size_all = 0;                // largest subdomain over all ranks
    int spmv_nt = -1;                           // window SpMV streams the matrix non-temporally: -1 = if larger than the Infinity Cache, 0 / 1
    int asm_lds_kb = 37;                        // LDS budget of the assembly kernel's contribution park (KB): 4 workgroups per CU
    int box_kind = 0;                           // Schwarz boxes: 0 = one lattice over all ranks' nodes, 1 = per-rank lattice
    int spmv_kind = 0;                          // 0 = CSR-window / automatic, 1 = row-per-lane-group, 2 = CSR-stream
    int asm_kind = 0;                           // option "asm_kind": 0 = the default dispatch (assemble.hip launch_assemble), 2 = the pair sweep always, 3 = slot-addressed where it fits
    // element-major tile structures of the current mesh (assemble_tiles.hip build_tiles): 0 = not built, 1 = ready, -1 = mesh does not fit
    int asm_p2_elem = 1;                        // option "asm_p2_elem": P2 scalar forms take their element matrices from k_elem_matrix (one element per wavefront); 0 = pair kernels alone
    fedd::GatherLists gl_p2;                    // of the node-level system pattern: row sums of the P2 scalar forms, FEDD_FORM_LAPLACE_XDIM (NO_FIT: the pair kernels)
    fedd::DevBuf<double> d_ke;                  // [n_elem * nen * nen] element matrices of the assembly in progress (P2)
    double asm_zero_eps = 0.0;                  // option "asm_zero_eps": FE::doSetZeros(eps) -- element contributions below eps are dropped (vector Laplacian, B, B^T); 0 = off
    int asm_tiles_host = 0;                     // option "asm_tiles_host": 1 = the tile structures are built on the host (the round-3 builder; A/B and tests), 0 = on the device
    double tl_build_ms = 0.0, adj_build_ms = 0.0;   // wall ms of the per-mesh structures of the current mesh: tile build, node -> element adjacency
    int tl_state = 0, asm_tiles = 1;            // option "asm_tiles": the P1 Laplace / elasticity forms take the element-major tile kernel (0: pair kernels)
    int64_t tl_ntile = 0;
    int tl_max_el = 0, tl_max_ext = 0, tl_max_blob = 0;
    fedd::DevBuf<uint32_t> tl_hdr, tl_blob;     // per-tile headers (16 bytes each) and blobs (assemble_tiles.hip TileHdr)
    fedd::DevBuf<uint32_t> tl_shape;            // [tl_ntile] first word of the shape part every tile reads (its own or an earlier tile's)
    int tl_nshared = 0;                         // tiles that read the shape of an earlier tile
    fedd::DevBuf<int32_t> d_pat_stash;          // pattern build: merged node lists of the count pass, [k][node]
    // ---- the solver's SpMV: options here, everything built from the matrix in `cs` (fedd::SpmvStream above) ----
    int spmv_compact = 1;                       // option "spmv_compact": 1 = on (default), 0 = stream the parity CSR
    double spmv_drop_tol = 2.220446049250313e-16;   // option "spmv_drop_tol": drop |a_ij| <= tol * max_k |a_ik|; 0 = exact zeros only
    int spmv_exact_public = 1;                  // option "spmv_exact_public": fedd_spmv multiplies with the parity CSR (every stored entry), not with the solver's compacted stream
    int spmv_col16 = 1;                         // option "spmv_col16": 16-bit columns in the per-entry window SpMV where the windows allow it
    int spmv_pattern = 1;                       // option "spmv_pattern": rows that repeat their column offsets share a pattern (spmv.hip)
    int spmv_win_nu = 0;                        // option "spmv_win_nu": entries per lane of k_spmv_win on the compacted stream (4 ... 8; 0 = by row length)
    int spmv_pat_nu = 0;                        // option "spmv_pat_nu": 16-byte loads per lane of k_spmv_pat (2 ... 8; 0 = by the usual row length)
    int spmv_classes = 1;                       // option "spmv_classes": rows that repeat their column pattern AND their values bit for bit share a class (spmv.hip k_spmv_cls)
    int spmv_cls_lds = 1;                       // option "spmv_cls_lds": the class kernel takes its block's class values from LDS and unit-stride x from the neighbouring lanes (spmv.hip k_spmv_cls_lds); 0: k_spmv_cls
    int spmv_cls_lds_cap = 0;                   // option "spmv_cls_lds_cap" (development): classes a block's list may hold, 0 = what the kernel's LDS holds; fewer: more blocks are flagged
    int spmv_cls_cover = 90;                    // option "spmv_classes_cover": the classes are used when they cover at least this percentage of the rows
    int spmv_keep_dict = 0;                     // option "spmv_keep_dictionary": 1 = the previous matrix' pattern dictionary and row classes are kept while the new stream matches them bit for bit (one verifying pass instead of the build: time loops that reassemble the same operator); 0 (default) = built per matrix
    int spmv_reuse = 1;                         // option "spmv_reuse"
    fedd::SpmvStream cs;
    fedd::DevCsr aux[fedd::MAX_AUX];            // stored blocks (A, B, B^T, C, F, M, A') of a mixed problem
    uint64_t pattern_counter = 0;               // source of DevCsr::pattern_id
    uint64_t mesh_id = 0;                       // counts the fedd_mesh_set calls: which mesh a stored pattern belongs to
    uint64_t value_counter = 0;                 // source of DevCsr::value_id
    int merge_slots[4] = {-2, -2, -2, -2};      // the slots and pattern ids the merged system matrix was built from: a merge of the
    uint64_t merge_ids[4] = {0, 0, 0, 0};       // same patterns moves values only (blocks.hip)

    // ---- advection matrices N(u), W(u) of Navier-Stokes (assemble.hip assemble_advection; one rank) ----
    std::vector<int32_t> h_col_of_rep;          // [n_rep] column-local node id of every repeated node (fedd_mesh_set)
    fedd::DevBuf<double> d_vel;                 // [n_node * dim] velocity at the nodes, column-local numbering (fedd_velocity_set)
    bool have_vel = false;
    fedd::DevBuf<double> d_mvel;                // [n_node * dim] mesh velocity w at the nodes, same numbering (fedd_mesh_velocity_set / _diff)
    bool have_mvel = false;
    fedd::GatherLists gl_adv;                   // of the node-level pattern below; READY: every per-mesh structure below is built
    int64_t adv_node_nnz = 0;                   // nonzeros of the node-level pattern
    int adv_max_nn = 0;                         // its longest row
    fedd::DevBuf<int32_t> d_adv_nptr, d_adv_ncol;   // node-level pattern [n_own + 1], [adv_node_nnz]: the FULL dof pattern follows in closed form
    fedd::DevBuf<double> d_adv_tab;             // quadrature tables of N, then of W where its rule differs (w | phi | dphi each)
    int adv_nq[2] = {0, 0}, adv_tab_off_w = 0;
    fedd::DevBuf<double> d_adv_ke;              // [n_elem][nen][nen][1 | dim * dim] element blocks of the assembly in progress
    uint64_t adv_pattern_id[fedd::MAX_AUX] = {};   // pattern id of the slots that hold the FULL pattern written here
    // ---- hyperelastic tangent and forces (hyperelastic.hip assemble_hyperelastic; one rank): u is d_vel, the element blocks
    //      pass through d_adv_ke, the tangent goes into the system matrix.  The lists and tables (full_lists_ensure) also serve
    //      the stress form (assemble.hip k_stress_elem, k_stress_gather), whose packed pair blocks pass through d_adv_ke too ----
    fedd::GatherLists gl_full;                  // of the system's FULL pattern; the tables below are uploaded with them
    fedd::DevBuf<double> d_hy_tab;              // w | dphi of the rule determineDegree(Grad, Grad)
    int hy_nq = 0;
    fedd::DevBuf<double> d_hy_fe;               // [n_elem][nen][dim] element forces of the assembly in progress
    fedd::DevBuf<double> d_hy_f;                // [n_own * dim] the force vector of the last call that asked for it
    bool have_hy_f = false;
    fedd::DevBuf<int32_t> d_hy_flag;            // [1] smallest element with det F <= 0 at a quadrature point (INT32_MAX: none)
    // ---- device-resident Newton state (newton.hip; one rank): buffers of their own, the state ends with fedd_mesh_set ----
    fedd::DevBuf<double> d_nw_u, d_nw_b, d_nw_s;   // [nw_n] the iterate u_k, the held right-hand side b, the step's source vector
    fedd::DevBuf<double> d_nw_part;             // per-workgroup partial sums of a norm | [1] the norm's square
    int64_t nw_n = -1;                          // length of the system at fedd_newton_begin
    bool nw_active = false;                     // between fedd_newton_begin and fedd_newton_end
    bool nw_have_src = false;                   // fedd_newton_source_set gave a vector since the begin
    bool nw_f_fresh = false;                    // d_hy_f was formed after the last fedd_newton_begin / fedd_newton_update
    int64_t nw_residuals = 0, nw_updates = 0;   // calls since the last fedd_newton_begin
    bool merged = false;                        // system matrix = merged blocks (dof -> node map below)
    int64_t merged_nA = 0;                      // rows of block row 0
    int merged_dofsA = 1;                       // dofs per node of block row 0
    fedd::DevBuf<int32_t> d_dof_node;           // [n_rows] node whose coordinates place the dof (merged systems)

    // ---- Schwarz ----
    int sw_target = 0;                          // nodes per box; 0 = default (27 / dofs per node)
    double sw_scale = 1.0;
    int sw_overlap = 1, sw_combine = 0;
    int64_t sw_nsub = 0, sw_max_size = 0, sw_max_own = 0, sw_inv_elems = 0;
    int apply_kind = 0;                         // restricted apply: 0 = by the setup (matrix cores where inverses are shared, else flat), 1 = strided, 2 = flat without the compact LDS layout, 4 = matrix cores also below 4096 subdomains, 6 = chunk records instead of the batch table (A/B)
    int inv_kind = 0;                           // local inverses: 0 = scalar-pivot kernel (drops finished rows), 1 = MFMA block sweep, 2 = scalar-pivot, all rows (A/B)
    int ghost_overlap = 1;                      // subdomains may contain ghost dofs (identity rows): 1 = yes (A/B)
    int gmres_kind = 2;                         // Gram-Schmidt: 0 = delayed second pass (DCGS2), 1 = two passes (CGS2), 2 = s-step blocks (BCGS-PIP2)
    int gmres_s = 0;                            // s-step GMRES: Krylov vectors per block (1 ... 16; 0 = 16 from 1.2 M rows per rank, else 8)
    int gmres_tol_blocks = 1;                   // ... tolerances below 1e-9 / 1e-11 take blocks of at most 5 / 3 vectors (0: no cap)
    int gmres_dot_own = 1;                      // ... 1 = W^T W of a block dot sweep from the W tile in registers, 0 = its columns are streamed like the basis (A/B)
    int gmres_dot_gy = 0;                       // ... column groups in flight per row block of the block dot kernel (0 = by vector length) (A/B)
    int gmres_s_used = 0;                       // ... the block length of the last solve
    int gmres_spec = 0;                         // ... operator applications of the next block issued before the host reads a block's outcome (A/B switch for multi-GPU runs)
    int gmres_newton = 1;                       // ... Newton block basis (Leja-ordered Ritz shifts) once the first s Arnoldi steps exist; 0 = monomial, blocks <= 8
    double gmres_chol_tol = 1e-13;              // ... a block is cut where the squared sine of a new vector against its predecessors falls to this
    int gmres_blocks = 0, gmres_cut_blocks = 0; // ... blocks / blocks that were cut in the last solve
    int gmres_floor = 0;                        // ... the last solve stopped at the rounding floor of b - A x (relres returned = true residual, may exceed rtol)
    double gmres_rec_relres = -1.0;             // ... and the recurrence residual it had reached then (-1: not that case)
    fedd::DevBuf<int32_t> d_node_bin;           // [n_own] compact bin id of each owned node
    fedd::DevBuf<int32_t> d_bin_ptr, d_bin_nodes;   // [nsub+1], [n_own]
    fedd::DevBuf<int32_t> d_sub_n, d_sub_nown;  // [nsub] total / owned dofs of each subdomain
    fedd::DevBuf<int32_t> d_sub_dofs;           // [nsub*NMAX] local dof ids (owned first)
    // structure stage of the setup (lattice, bins, dof lists: the five buffers above, d_fbin_* and the sizes sw_nsub, sw_max_size,
    // sw_max_own, sw_max_size_all): a function of the node coordinates, the matrix graph and the parameters of SwStructKey, kept
    // from setup to setup while those stand (option "schwarz_reuse", default 1; 0 = built by every setup)
    uint64_t mesh_gen = 0;                      // bumped by whatever can change node counts, ghost layout, owners or halo (fedd_mesh_set*, which
                                                // also brings new coordinates; a fedd_mesh_move moves geometry_id instead and leaves this one)
    uint64_t pattern_gen = 0;                   // bumped by whatever writes d_rowptr / d_colind (system_written), except a fedd_pattern_build that repeats
                                                // the one the pattern came from (same mesh_gen, dofs per node, block mode)
    bool pat_repeatable = false;                // the system pattern is the output of build_pattern on pat_mesh_gen (and nothing wrote it since)
    uint64_t pat_mesh_gen = 0;
    int pat_reuse = 1;                          // option "pattern_reuse": a build_pattern that repeats keeps d_rowptr / d_colind (0: writes them again)
    int pat_last_reused = 0;                    // the last build_pattern kept them
    int64_t pat_reuse_count = 0;                // builds that kept them since the context was made
    struct SwStructKey {
        uint64_t mesh_gen = 0, pattern_gen = 0, geometry_id = 0;
        int64_t n_own = 0, n_rows = 0, n_rows_ext = 0, merged_nA = 0;
        double scale = 0.0;
        int target = 0, overlap = 0, box_kind = 0, whole_boxes = 0, ghost_overlap = 0, merged = 0, dofs = 0, dim = 0, nranks = 0;
        bool operator==(const SwStructKey& o) const {
            return mesh_gen == o.mesh_gen && pattern_gen == o.pattern_gen && geometry_id == o.geometry_id && n_own == o.n_own && n_rows == o.n_rows &&
                   n_rows_ext == o.n_rows_ext && merged_nA == o.merged_nA && scale == o.scale && target == o.target &&
                   overlap == o.overlap && box_kind == o.box_kind && whole_boxes == o.whole_boxes &&
                   ghost_overlap == o.ghost_overlap && merged == o.merged && dofs == o.dofs && dim == o.dim && nranks == o.nranks;
        }
    } sw_struct_key;
    bool sw_struct_valid = false;               // the kept structure belongs to sw_struct_key (false after the large-subdomain path)
    int sw_reuse = 1;                           // option "schwarz_reuse"
    int sw_last_reused = 0;                     // the last setup kept the structure
    int64_t sw_reuse_count = 0;                 // setups that kept it since the context was made
    fedd::DevBuf<int64_t> d_inv_ptr;           // [nsub+1] offsets into d_inv (elements)
    fedd::DevBuf<int64_t> d_sw_gather;         // [8] scalars of the numeric stage read back in one copy (schwarz.hip k_setup_gather)
    fedd::DevBuf<double> d_inv;                 // per subdomain [n_i][rp_i] column-major slab
    fedd::DevBuf<double> d_mult;                // [n_cols] multiplicity (averaging)
    bool have_schwarz = false;                  // cleared by system_written (below): a parent that applies this context as a block (blockprec.hip)
                                                // trusts it, and orders this context's stream in front of its own whenever sw_setup_gen moved or this stream still has work
    int md2_gy = 0;                             // k_multidot2: column groups in flight per row block (0 = by vector length)
    int halo_overlap = 0;                       // several ranks: interior subdomains first, ghost import of r on a second stream meanwhile
    hipStream_t stream2 = nullptr;              // (created on first use)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int64_t sw_nconf = 0;                       // subdomains whose dof list is their representative's list shifted (ids computed in the apply)
    int64_t sw_nint = -1;                       // subdomains without ghost dofs at the front of d_sw_order (-1: not split)
    int apply_span = 0;                         // matrix-core apply: places per workgroup (0 = by subdomain count with chunk records, one round of workgroups with the batch table)
    int sw_dedupe = 1;                          // option "schwarz_dedupe": subdomains with the same local matrix share one slab
    int sw_fp_kind = 0;                         // option "schwarz_fp_kind": fingerprints from row hashes (0) or entry by entry (1)
    int64_t sw_nrep = 0;                        // distinct local matrices (= slabs) of the last setup
    fedd::DevBuf<double> d_sw_rmax;             // [n_rows_ext] largest magnitude of every stored row
    fedd::DevBuf<uint64_t> d_sw_fp;             // fingerprints [2 nsub] | hash table keys [2 tsize]
    fedd::DevBuf<int32_t> d_sw_order;           // subdomains sorted by representative [nsub] | sort scratch [2 nsub] | pad | records int4[nsub]
    int64_t sw_order_off = 0;                   // where the records start (in int32 units, 16-byte aligned)
    fedd::DevBuf<int32_t> d_sw_bt;              // batch table of k_apply_bt: BT_W ints per batch (schwarz.hip)
    fedd::DevBuf<int32_t> d_sw_btw;             // ... its build scratch
    int64_t sw_nbatch = 0;                      // batches in the table (0: no table, the chunk-record kernel runs)
    int64_t sw_nbatch_int = 0;                  // ... of which belong to the subdomains without ghost dofs (split order)
    int apply_bt = 1;                           // build and use the batch table (option "apply_bt")
    fedd::DevBuf<int32_t> d_sw_replist;         // the representatives (the subdomains that are inverted)
    fedd::DevBuf<int32_t> d_sw_rep;             // representative [nsub] | sizes for the inversion [nsub] | slot [nsub] | table min [tsize]
    int sw_big = -1;                            // large-subdomain path: -1 = for merged block systems, 0 = never, 1 = always
    bool sw_big_active = false;                 // the current preconditioner was built by schwarz_setup_big
    int sw_big_target = 0;                      // owned dofs per box of the bisection (0 = default 120)
    fedd::DevBuf<double> d_big_ws;              // dense matrices of one chunk of subdomains
    fedd::DevBuf<int32_t> d_big_nblk;           // 64-blocks per subdomain
    fedd::DevBuf<int32_t> d_big_ids, d_big_pos; // subdomains taken by the batched dense inversion (compacted ids)

    // ---- symmetric apply without floating-point atomics (schwarz_sym.hip): park + gather ----
    int apply_gather = 0;                       // option "apply_gather": 1 = fedd_schwarz_apply / GMRES take the park + gather kernels for Full and Averaging
    int apply_full_kind = 0;                    // option "apply_full_kind": 0 = matrix cores where a representative is shared, 1 = k_full_park only, 2 = matrix cores asked for
    bool sym_force = false;                     // fedd_cg is running: the park + gather kernels whatever "apply_gather" says
    bool sym_ready = false;                     // the structures below belong to the current preconditioner
    int sym_kind_built = 0;                     // ... and to this value of "apply_full_kind"
    bool sw_full_records = false;               // k_full_park walks d_sw_fplain (else every subdomain)
    int64_t sw_sum_n = 0;                       // sum of the subdomain sizes = entries of the park
    int64_t sw_full_nbatch = 0, sw_full_nmfma = 0, sw_full_nplain = 0;   // matrix-core batches; subdomains by park kernel
    fedd::DevBuf<int32_t> d_sw_off;             // [nsub + 1] offset of every subdomain in the park
    fedd::DevBuf<int32_t> d_sw_tptr, d_sw_tsrc; // transpose of sub_dofs: [n_cols + 1] list starts, [sum n_i] park positions, ascending per dof
    fedd::DevBuf<double> d_sw_park;             // [sum n_i] y_i = A_i^-1 R_i r
    fedd::DevBuf<int32_t> d_sw_fbatch, d_sw_fplain;   // (first place, places) per matrix-core batch; subdomains of k_full_park

    // ---- CG (cg.hip) ----
    fedd::DevBuf<double> d_cg;                  // r, z, p, q and the slots of the dot partials
    int cg_replacements = 0, cg_breakdown = 0;  // of the last fedd_cg: residual replacements, breakdown word (FEDD_CG_BREAKDOWN_*)

    // ---- Newmark time stepping (timestep.hip; one rank) ----
    fedd::DevBuf<double> d_nm_un, d_nm_v, d_nm_w;   // [n_rows] u_n, velocity, acceleration of the last completed step
    fedd::DevBuf<double> d_nm_t;                // [n_rows] the vector M is applied to for the right-hand side
    int64_t nm_n = -1;                          // length the state was allocated and zeroed for (-1: none)
    bool nm_first = true;                       // the next fedd_newmark_advance is the first step: v and w stay
    // ---- multistep (BDF) history (timestep.hip; one rank): buffers of their own, released by fedd_mesh_set ----
    fedd::DevBuf<double> d_ms_u[2];             // [ms_n] u_0 (the last recorded solution), u_1 (the one before; order 2 only)
    fedd::DevBuf<double> d_ms_t;                // [ms_n] the combination M is applied to for the right-hand side
    int ms_order = 0, ms_count = 0;             // 0 = no history (fedd_multistep_begin); vectors recorded so far (<= ms_order)
    int64_t ms_n = -1;                          // length of the system at fedd_multistep_begin
    // ---- single-step (Runge-Kutta) stage store (singlestep.hip; one rank): buffers of their own, not matrix slots; kept from
    //      step to step, released by fedd_mesh_set ----
    fedd::DevBuf<double> d_st_val[fedd::MAX_STAGES];   // [st_nnz] the values of the stage operator F_j, on the pattern of the first push
    fedd::DevBuf<double> d_st_u[fedd::MAX_STAGES];     // [st_n] the stage solution U_j = [u_j ; p_j]
    fedd::DevBuf<double> d_st_part;             // fedd_stage_error: partial sums per workgroup | [1] their sum
    int st_max = 0, st_count = 0;               // 0 = no open step (fedd_stage_begin); stages pushed in this step
    int st_slot = -1;                           // the slot of the first push: its row pointers and columns are the stages' pattern
    uint64_t st_pattern_id = 0;                 // ... while it still holds the pattern with this DevCsr::pattern_id
    int64_t st_nnz = 0, st_n = 0, st_rows = 0;  // nonzeros and rows of that pattern, length of the system at the first push
    uint64_t sys_pattern_id = 0;               // the system slot holds the pattern with this DevCsr::pattern_id (copied by
    uint64_t sys_pattern_gen = 0;               // fedd_matrix_store / fedd_matrix_combine) ... while pattern_gen still has this value
    uint64_t sys_value_gen = 0;                 // bumped by every writer of the system matrix' values (system_written; Dirichlet rows excepted)
    uint64_t sys_write_count = 0;               // bumped by every system_written, whatever it wrote (Dirichlet rows included)
    // ---- option "setup_fused" (default 1; 0 = every consumer walks the matrix and the elements for itself) ----
    int setup_fused = 1;
    struct SetupWalk {                          // the SpMV stream check, made by the walk that forms the Schwarz row hashes (spmv.hip setup_walk)
        bool valid = false;
        uint64_t write_count = 0;               // sys_write_count of the rows that were walked: any write since makes the result stale
        int32_t bad = 0;                        // what k_cs_reuse leaves in *n_bad
    } setup_walk;
    int64_t fused_walks = 0, fused_checks_used = 0, fused_absdet_kept = 0;   // fedd_setup_fused_info
    fedd::DevBuf<double> d_absdet;              // [n_elem] |det B| of every element (assemble.hip assemble_rhs), kept while the
    bool absdet_valid = false;                  // connectivity (mesh_gen: fedd_mesh_set*) and the coordinates (geometry_id: fedd_mesh_move)
    uint64_t absdet_mesh_gen = 0, absdet_geometry_id = 0;   // are the ones it was computed from
    int comb_slot_m = -1, comb_slot_a = -1;     // the last fedd_matrix_combine: slots, coefficients, the slots' value ids
    double comb_cm = 0.0, comb_ca = 0.0;        // and the sys_value_gen it left (none yet: a value sys_value_gen never takes)
    uint64_t comb_id_m = 0, comb_id_a = 0, comb_sys_gen = ~(uint64_t)0;

    // ---- a preconditioner out of two child contexts that this one does not own (blockprec.hip "child link"; one rank): the
    //      block preconditioner of a merged 2 x 2 system (blockprec.hip) or FaCSI of a coupled system (fsi.hip) ----
    fedd::AttachedPrec prec;
    std::vector<fedd_ctx*> prec_parents;        // contexts that hold this one as a child of their attached preconditioner
    int bp_kind = 0;                            // 0 = none attached, FEDD_BLOCKPREC_DIAGONAL / FEDD_BLOCKPREC_TRIANGULAR
    double bp_scale = 1.0;                      // z_p = bp_scale * S(r_p)
    int bp_slot_bt = -1;                        // B^T of the Triangular form
    fedd::DevBuf<double> d_bp_ws;               // [n_rows] S(r_p) | t of the Triangular form
    uint64_t sw_setup_gen = 0;                  // counts the fedd_schwarz_setup calls of this context
    // the system matrix is an import (fedd_matrix_import) of this block: the source context's uid, its mesh, the block's pattern id, and the
    // pattern_gen the import left here -- while all four stand, the next import of that block moves values only
    uint64_t uid = 0;                           // process-wide unique id of this context (fedd_ctx_create): an address can come back
    uint64_t imp_src_uid = 0;                   // ... after a destroy, this number cannot
    uint64_t imp_mesh_id = 0, imp_pattern_id = 0, imp_pattern_gen = 0;

    // ---- FSI coupling (fsi.hip; one rank) ----
    std::shared_ptr<fedd::IfaceTable> iface;    // the matched interface this context is one side of (fedd_interface_match)
    // a coupled context: the system matrix is the four-block system of fedd_fsi_merge (the context carries no mesh)
    bool fsi_coupled = false;
    std::shared_ptr<fedd::IfaceTable> fsi_table;   // the match the merge was built on
    uint64_t fsi_uid_f = 0, fsi_uid_s = 0;      // the children of the merge: uid, and their mesh_gen / pattern_gen at the merge
    uint64_t fsi_mesh_gen_f = 0, fsi_mesh_gen_s = 0, fsi_pat_gen_f = 0, fsi_pat_gen_s = 0;
    uint64_t fsi_pat_gen = 0;                   // ... and the pattern_gen the merge left here
    int64_t fsi_nu = 0, fsi_np = 0, fsi_ns = 0, fsi_nl = 0;   // block sizes: velocity, pressure, structure, lambda
    double fsi_dt = 0.0;
    std::vector<uint8_t> fsi_mask;              // [fsi_nl] 1 = coupled lambda-dof
    fedd::DevBuf<int32_t> d_fsi_fdof, d_fsi_sdof;   // [fsi_nl] fluid / structure dof of lambda-dof k (-1: uncoupled)
    fedd::DevBuf<int32_t> d_fsi_lam_f, d_fsi_lam_s; // [n_u + n_p], [n_s] lambda-dof of a fluid / structure dof (-1: none)
    int fsi_last_values_only = 0;               // the last merge moved values only
    int64_t fsi_values_only_count = 0;          // merges that did since the context was made
    fedd::DevBuf<double> d_fp_t;                // [n_u + n_p] t of the FaCSI apply (the children: `prec` above)

    // ---- coarse level (two-level Schwarz) ----
    int sw_two_level = 0;
    int sw_levels = FEDD_LEVELS_ADDITIVE;       // fedd_schwarz_set_level_combination, read at apply time
    double co_cells_target = 0.0;               // 0 = default
    fedd::CoarseGeom co_geom;
    int64_t co_ncell = 0, co_nlat = 0, co_n0 = 0, co_ld = 0;
    fedd::DevBuf<int32_t> d_co_key[2], d_co_val[2];   // radix split ping-pong (cell id, node)
    fedd::DevBuf<int32_t> d_co_cell_ptr;        // [ncell+1]; nodes of cell: d_co_val[co_sorted]
    int co_sorted = 0;
    fedd::DevBuf<double> d_co_mask;             // [n_cols] 1 = free dof, 0 = Dirichlet
    fedd::DevBuf<double> d_co_cellK;            // per-cell Galerkin blocks
    fedd::DevBuf<double> d_co_K;                // [ld*ld] K0, then K0^-1
    fedd::DevBuf<double> d_dense_ws;            // dense_invert_batched: per matrix Dinv [64*64] | R [64*ld] | C [ld*64]
    fedd::DevBuf<double> d_co_part, d_co_r0, d_co_z0;
    fedd::DevBuf<double> d_co_w;                // [n_rows] A z of the multiplicative combination
    bool have_coarse = false;                   // implies have_schwarz: system_written clears both
    int co_kind = FEDD_COARSE_Q1;               // FEDD_COARSE_Q1 (lattice hat functions) / FEDD_COARSE_GDSW
    double gdsw_tol = 0.0;                      // option "gdsw_tol": relative residual of the interior extension solves; 0 = GDSW 1e-4, RGDSW 1e-3
    int gdsw_ext_its = 0;                       // most iterations / largest final residual of the last setup's extension solves
    double gdsw_ext_rel = 0.0;
    fedd::DevBuf<int32_t> d_gd_ent;             // [n_own] interface entity (doubled-lattice id) of every owned node
    fedd::DevBuf<double> d_gd_phi;              // [n_rows * (3^dim - 1) * dofs] coarse basis, row-wise by class of the home cell
    fedd::DevBuf<double> d_gd_imask;            // [n_rows] 1 = free interior dof
    fedd::DevBuf<double> d_gd_tmp;
    fedd::DevBuf<double> d_gd_stack;            // stacked vectors of the extension solves (gdsw_block)

    // ---- GMRES workspace ----
    fedd::DevBuf<double> d_V, d_Z;              // [(m+1)*n_rows], [n_cols] scratch
    fedd::DevBuf<double> d_w;                   // [n_rows]
    fedd::DevBuf<double> d_part;                // dot partials
    fedd::DevBuf<double> d_small;               // H, cs, sn, g, h, scalars
    double* h_pinned_map = nullptr;             // device pointer of h_pinned (kept while the option switches h_pinned_dev off)
    double* h_pinned_dev = nullptr;             // the same buffer as the device sees it (nullptr: not mapped, copies are used)
    double* h_pinned = nullptr;                 // small pinned host mirror
    int gm_restart_alloc = 0;
    int64_t gm_V_ldv = -1;                      // leading dimension the zeroed padding rows of d_V belong to (s-step solver)
    int multi_ch = 4;                           // option "multi_ch": matrix-core steps per flight of gathers in k_apply_multi (4, 8, 16)
    int pat_hash = 1;                           // option "pat_hash": 1 = hashed node-pattern merge for vertex-only elements (symbolic.hip)
    int gmres_fused_blocks = 0;                 // blocks of the last s-step solve whose first update and second dot ran as one sweep
    fedd::GmresCapture gm_cap;                  // fedd_gmres_capture_*: one block of an s-step solve, stage by stage (tests)
    int gmres_fuse = -1;                        // option "gmres_fuse": s-step solver, first update and second dot of a block in one sweep (k_blockfuse); -1 = from 4 M rows on
    int gdsw_rot = 0;                           // option "gdsw_rotations": rotations in the null space of vector problems (dofs = dim)
    int co_nns = 1;                             // coarse functions per entity of the last GDSW setup (dofs, or dofs + rotations)
    fedd::DevBuf<double> d_gd_gram;             // [entities * 21] Gram matrices of the entities' functions (selection of the independent ones)
    fedd::DevBuf<int32_t> d_gd_keep;            // [entities] bit masks of the functions kept
    int gdsw_block = 1;                         // option "gdsw_block": 1 = extension solves sixteen columns at a time, 0 = one by one

    // ---- generic scratch ----
    fedd::DevBuf<int32_t> d_itmp0, d_itmp1, d_itmp2;
    fedd::DevBuf<int64_t> d_scan[3];            // block sums of the device scan, one per level
    fedd::DevBuf<int32_t> d_rs_hist;            // radix sort: digit histograms [256][tiles]
    fedd::DevBuf<double> d_dtmp0;
    fedd::DevBuf<uint64_t> d_u64tmp;            // hashes and hash-table keys of a build in progress (SpMV dictionary, tile shapes)
    fedd::DevBuf<int32_t> d_flags;              // [16] device flags: 0 max scratch, 1 bad pivot, 2 DGKS gate, 3-5 coarse setup, 8-11 Schwarz setup counters, 12 s-step block length, 13 SpMV stream keep, 14 interface match twin, 15 coupled merge row check

    fedd::HaloPlan halo;

    // ---- timing ----
    bool timing = false;
    int timing_stride = 1;
    fedd::TimerSlot timers[FEDD_T_COUNT];
    std::vector<hipEvent_t> ev_pool;            // timer events waiting for reuse (ScopedTimer::take, timing_flush)
};

namespace fedd {

// What a write to the system matrix invalidates (DESIGN.md has the table of writers).  Every writer of the system slot says
// what it wrote, once, in the worker that launches the writing kernel, after its argument checks and before the first launch;
// nothing else clears these fields or moves the two generations (assemble_div records a second time, after the build_pattern it
// calls: see there).  A builder sets its own product (cs.valid, have_schwarz,
// have_coarse, sym_ready, cs.rows_csr_ready, pat_repeatable, have_pattern) at the end of its build and may clear it at the start.
enum : unsigned {
    SYS_VALUES = 1,      // d_val rewritten: assembly, scale of the system slot, merge, combine, import, tangent
    SYS_DIRICHLET = 2,   // unit rows / rhs / isdir written: not a new operator, sys_value_gen stays
    SYS_PATTERN = 4,     // d_rowptr / d_colind rewritten, or declared rewritten (the values-only merge)
    SYS_GONE = 8,        // the slot holds no system matrix any more
    SYS_GEOMETRY = 16,   // the node coordinates moved (fedd_mesh_move), on its own: the matrix and its SpMV stream stand, what was laid
                         // over the old coordinates goes -- the preconditioner here, the Schwarz box structure through
                         // SwStructKey::geometry_id, the last combine's record (its matrices belong to the old coordinates)
};
inline void system_written(fedd_ctx* c, unsigned what) {
    ++c->sys_write_count;
    if (what & SYS_GEOMETRY) {
        ++c->geometry_id;
        c->comb_sys_gen = ~(uint64_t)0;        // fedd_matrix_combine_current answers 0
    }
    if (what & ~SYS_GEOMETRY) c->cs.valid = false;   // the solver's SpMV stream (cs.key stands: the next build may find the stream still fits)
    c->have_schwarz = false;     // the numeric stage of the preconditioner: a parent that applies this context as a block sees it
    c->have_coarse = c->sym_ready = false;     // ... and what was built on it: the coarse level, the park + gather lists
    if (what & SYS_VALUES) ++c->sys_value_gen;
    if (what & SYS_PATTERN) {
        ++c->pattern_gen;
        c->pat_repeatable = false;
        c->cs.rows_csr_ready = false;
    }
    if (what & SYS_GONE) c->have_pattern = false;
}

// ... what a new mesh does to the gather lists (a fedd_mesh_move keeps them: they follow connectivity and patterns, not coordinates)
inline void gather_lists_reset(fedd_ctx* c) { c->gl_p2.reset(), c->gl_adv.reset(), c->gl_full.reset(); }

// ... and what an option drops when it is set (fedd_set_option's table names one of these per key)
enum : unsigned {
    OPT_DROPS_STREAM = 1,    // the solver's SpMV stream and the key it is kept by
    OPT_DROPS_SCHWARZ = 2,   // the preconditioner
    OPT_DROPS_TILES = 4,     // the assembly's tile structures
    OPT_DROPS_REPEAT = 8,    // the next fedd_pattern_build builds
    OPT_DROPS_FUSED = 16,    // what option "setup_fused" keeps from one call for a later one: the stream check, |det B|
};
inline void option_drops(fedd_ctx* c, unsigned what) {
    if (what & OPT_DROPS_STREAM) c->cs.valid = c->cs.key.valid = c->setup_walk.valid = false;
    if (what & OPT_DROPS_SCHWARZ) c->have_schwarz = false;
    if (what & OPT_DROPS_TILES) c->tl_state = 0;
    if (what & OPT_DROPS_REPEAT) c->pat_repeatable = false;
    if (what & OPT_DROPS_FUSED) {
        c->setup_walk.valid = c->absdet_valid = false;
        c->d_absdet.release();      // (470 MB at the headline: not held by a context that has switched the option off)
    }
}

// RAII-ish helper: records a start event at construction and a stop event at stop().
struct ScopedTimer {
    fedd_ctx* c;
    int id;
    hipEvent_t a = nullptr, b = nullptr;
    bool sampled = false, cont = false;
    ScopedTimer(fedd_ctx* ctx, int timer) : c(ctx), id(timer) {   // timer < 0: no-op
        if (c->timing && timer >= 0) {
            // the per-iteration classes are sampled every timing_stride-th launch: an event pair
            // around each of several hundred small launches per solve costs a few percent
            const bool per_iteration = timer == FEDD_T_SPMV || timer == FEDD_T_SCHWARZ_APPLY ||
                                       timer == FEDD_T_ORTHO || timer == FEDD_T_COARSE_APPLY ||
                                       timer == FEDD_T_HALO || timer == FEDD_T_ALLREDUCE || timer == FEDD_T_GS_DOT ||
                                       timer == FEDD_T_GS_UPDATE || timer == FEDD_T_GS_FUSED;
            // (the s-step solver launches its sweeps once per block, each over a different number of columns: all timed)
            const bool block_sweeps = c->gmres_kind == 2 && (timer == FEDD_T_ORTHO || timer == FEDD_T_GS_DOT || timer == FEDD_T_GS_UPDATE || timer == FEDD_T_GS_FUSED);
            const int64_t k = c->timers[id].seen++;
            if (per_iteration && !block_sweeps && c->timing_stride > 1 && k % c->timing_stride != 0) return;
            sampled = true;
            if (take(&a) && take(&b)) (void)hipEventRecord(a, c->stream);
        }
    }
    // events come from the context's pool (timing_flush returns them): creating a pair per timed launch cost about 2 ms of
    // host time per 100 ms step -- inside the timed region of the bench
    bool take(hipEvent_t* e) {
        if (!c->ev_pool.empty()) {
            *e = c->ev_pool.back();
            c->ev_pool.pop_back();
            return true;
        }
        return hipEventCreate(e) == hipSuccess;
    }
    // algorithmic bytes of this launch (counted when the launch is timed)
    void bytes(double nbytes) {
        if (sampled && !cont) c->timers[id].bytes += nbytes;
    }
    void stop() {
        if (c->timing && a && b) {
            (void)hipEventRecord(b, c->stream);
            c->timers[id].pending.push_back({a, b, cont});
            a = b = nullptr;
        }
    }
    // after stop(): time the rest of the same launch (same sampling decision, not another launch)
    void resume() {
        if (c->timing && sampled && !a) {
            cont = true;
            if (take(&a) && take(&b)) (void)hipEventRecord(a, c->stream);
        }
    }
    ~ScopedTimer() { stop(); }
};

int timing_flush(fedd_ctx* c);

// device utilities (scan.hip)
int exclusive_scan_i32(fedd_ctx* c, const int32_t* d_in, int32_t* d_out, int64_t n, int64_t* total_out);
int exclusive_scan_i64(fedd_ctx* c, const int64_t* d_in, int64_t* d_out, int64_t n, int64_t* total_out);
int reduce_max_i32(fedd_ctx* c, const int32_t* d_in, int64_t n, int32_t* out);
// stable radix sort of (key, value) pairs on bits [0, bits) of the non-negative keys; keys[0] / vals[0] = input, the passes
// ping-pong between the two buffers, *cur_out = the one that holds the result
int radix_sort_pairs_i32(fedd_ctx* c, int32_t* keys[2], int32_t* vals[2], int32_t n, int bits, int* cur_out);

// symbolic.hip
int build_adjacency(fedd_ctx* c);
int build_node_lists(fedd_ctx* c, const int32_t* d_conn, int64_t n_ent, int32_t n_nodes, DevBuf<int32_t>& ptr, DevBuf<int32_t>& lst,
                     int32_t* max_deg);
int build_pattern(fedd_ctx* c, int dofs, int block_mode);
bool pattern_repeats(const fedd_ctx* c, int dofs, int block_mode);   // build_pattern would keep d_rowptr / d_colind: no symbolic work
// the node-level pattern alone into buffers of the caller's (the system slot is not touched), and its closed-form expansion to dofs
int build_node_pattern(fedd_ctx* c, DevBuf<int32_t>& nptr, DevBuf<int32_t>& ncol, int32_t* max_nn, int64_t* node_nnz);
int expand_node_pattern(fedd_ctx* c, const int32_t* nptr, const int32_t* ncol, int dofs, int full, int32_t* rowptr, int32_t* colind);

// assemble.hip
// (coeff_q / n_coeff: the coefficient array of FEDD_FORM_STRESS, nullptr = 1; the other forms ignore them)
int assemble_matrix(fedd_ctx* c, int form, const double* params, const double* coeff_q = nullptr, int64_t n_coeff = 0);
// gather lists of the system's FULL pattern + the tables w | dphi of the (Grad, Grad) rule, kept per (mesh, pattern) in
// gl_full / d_hy_tab / hy_nq: shared by the hyperelastic tangent and the stress form
int full_lists_ensure(fedd_ctx* c, const char* who);
int assemble_rhs(fedd_ctx* c, int dofs, const double* f_const, int extra_degree);
int surface_set(fedd_ctx* c, int nsn, int64_t n_surf, const int32_t* surf, const int32_t* sflag);
// g_surf != nullptr: one load per surface element; else n_flags == 0: g[dofs] on every element, n_flags > 0: g[n_flags * dofs] by flag
int assemble_surface(fedd_ctx* c, int dofs, int n_flags, const int32_t* flags, const double* g, const double* g_surf,
                     int extra_degree, int accumulate);
int apply_dirichlet(fedd_ctx* c, int n_bc, const int32_t* flags, const int32_t* comp_mask,
                    const double* values);
int apply_dirichlet_nodes(fedd_ctx* c, int64_t n, const int32_t* nodes, const int32_t* comp_mask,
                          const double* values);
int apply_dirichlet_rows(fedd_ctx* c, int64_t n, const int32_t* rows, const double* values);
int assemble_div(fedd_ctx* c, int64_t n_pressure_nodes, int slot_b, int slot_bt);
int velocity_set(fedd_ctx* c, const double* u_rep);
int mesh_velocity_set(fedd_ctx* c, const double* w_rep);
int mesh_velocity_diff(fedd_ctx* c, const double* d_new_rep, const double* d_old_rep, double dt);
int mesh_velocity_get(fedd_ctx* c, double* w_rep);
int assemble_advection_ale(fedd_ctx* c, int kind, double scale, int slot_add, int slot_out);
int assemble_advection(fedd_ctx* c, int kind, double scale, int slot_add, int slot_out);
// The one builder of gather lists (k_p2_lists): gl for the first nn nodes of a pattern of the caller's with node_nnz node-level
// nonzeros (full: FULL blocks, else scalar / DIAG); nothing to do where gl is ready for this mesh and `pattern`.  Lists that do not
// fit are an error naming `who`; who == nullptr (the caller has another path): no error, NO_FIT also without pattern, adjacency or nodes
int gather_lists_ensure(fedd_ctx* c, GatherLists& gl, uint64_t pattern, const int32_t* rowptr, const int32_t* colind, int dofs,
                        int full, int64_t nn, int64_t node_nnz, const char* who);

// interface_distance.hip
int interface_distance_tile();
int interface_distance_flags(fedd_ctx* c, int n_flags, const int32_t* flags, int64_t* n_interface);
int interface_distance_points(fedd_ctx* c, int64_t n_pts, const double* xyz_pts);
int interface_distance_set(fedd_ctx* c, const double* dist_rep);    // nullptr releases
int interface_distance_get(fedd_ctx* c, double* dist_rep);
int laplace_scale(fedd_ctx* c, double distance, double coefficient);   // f per element into d_lscale, in the stream
int laplace_scale_get(fedd_ctx* c, double* f_elem);

// mesh_move.hip
int mesh_move(fedd_ctx* c, const double* disp_rep);     // nullptr: back to the reference coordinates
int mesh_coords_get(fedd_ctx* c, double* xyz_rep);

// hyperelastic.hip
int assemble_hyperelastic(fedd_ctx* c, int model, const double* params, int n_params, int what);
int assemble_hyperelastic_time(fedd_ctx* c, int model, const double* params, int n_params, int what, int slot_m, double cm);

// assemble_tiles.hip: the element-major tile path (P1 simplices; kform = Laplace or elasticity of assemble_common.hpp).
// Returns -1, without error, when the mesh does not fit the tiles.
struct AsmArgs;
int assemble_tiles(fedd_ctx* c, int kform, const AsmArgs& a, int ntab);
int tiles_refresh_coords(fedd_ctx* c);   // the coordinate copies at the head of the tile blobs, from d_xyz (after a move; no-op without tiles)

// blocks.hip
int matrix_store(fedd_ctx* c, int slot);
int matrix_scale(fedd_ctx* c, int slot, double alpha);
int block_merge(fedd_ctx* c, int slot_a, int slot_bt, int slot_b, int slot_c);
// ... with every B^T value multiplied by s_bt on its way into the merged matrix (fedd_block_merge_scaled)
int block_merge_scaled(fedd_ctx* c, int slot_a, int slot_bt, double s_bt, int slot_b, int slot_c);
// timestep.hip: the system slot adopts the pattern of the stored block m (fedd_matrix_combine, fedd_matrix_import): buffers, row
// pointers and columns (copied in c's stream), sizes; the values are the caller's.  n_xcol = the length of d_xcol;
// zero_other_len: a right-hand side and a solution of another length are zeroed; pattern_id = what sys_pattern_id becomes
int system_adopt_pattern(fedd_ctx* c, const DevCsr& m, int dofs, int block_mode, size_t n_xcol, bool zero_other_len, uint64_t pattern_id);

// blockprec.hip: Diagonal / Triangular block preconditioner of a merged system out of two child contexts
int block_prec_check(fedd_ctx* c, const char* who);    // everything an apply needs, with errors that name the child
int block_prec_apply(fedd_ctx* c, const double* d_r_owned, double* d_z_owned);
// ... and the child link that the block preconditioner and FaCSI share.  `label` is the kind as the messages name it, `nm` the
// child, `parent` the parent; a kind's own checks of the child's system stand between the two halves of the check
void prec_attach(fedd_ctx* c, int kind, fedd_ctx* first, fedd_ctx* second);   // (after prec_unlink of an earlier attach)
void prec_unlink(fedd_ctx* c);                         // c gives up its children (detach, re-attach, destroy of c)
void prec_child_gone(fedd_ctx* child);                 // a child is being destroyed: its parents are detached first
int child_check_context(const fedd_ctx* c, const fedd_ctx* ch, const char* who, const char* label, const char* nm, const char* parent);
int child_check_schwarz(const fedd_ctx* ch, const char* who, const char* label, const char* nm, const char* mult_operator);
int child_order(fedd_ctx* c, PrecChild& ch);           // the child's own stream is ordered before c's, where that is needed
int child_apply(fedd_ctx* c, fedd_ctx* ch, const double* d_r, double* d_z);   // the child's Schwarz apply, in c's stream
// the preconditioner of the context: the attached block operator, else its own Schwarz preconditioner
int schwarz_apply(fedd_ctx* c, const double* d_r_owned, double* d_z_owned, bool r_has_tail);
// fsi.hip: matched interface, the coupled four-block system, the FaCSI preconditioner out of two child contexts
void iface_release(fedd_ctx* c);                       // fedd_mesh_set* / destroy: the match of this context is released on both sides
int fsi_prec_check(fedd_ctx* c, const char* who);      // everything an apply needs, with errors that name the child
int fsi_prec_apply(fedd_ctx* c, const double* d_r_owned, double* d_z_owned);
inline bool has_attached_prec(const fedd_ctx* c) { return c->prec.kind != AttachedPrec::NONE; }
inline int attached_prec_check(fedd_ctx* c, const char* who) {
    return c->prec.kind == AttachedPrec::FACSI ? fsi_prec_check(c, who) : block_prec_check(c, who);
}
inline int prec_apply(fedd_ctx* c, const double* d_r_owned, double* d_z_owned, bool r_has_tail) {
    if (c->prec.kind == AttachedPrec::FACSI) return fsi_prec_apply(c, d_r_owned, d_z_owned);
    return c->prec.kind ? block_prec_apply(c, d_r_owned, d_z_owned) : schwarz_apply(c, d_r_owned, d_z_owned, r_has_tail);
}

// spmv.hip
// x_has_tail: the buffer behind d_x_owned has room for all n_cols entries; the ghost values are then imported in
// place (behind the owned entries) instead of into a copy of x
// d_sub != nullptr: y = A x - theta * d_sub (owned rows), fused into the kernel's store
// use_compact: -1 = as option "spmv_compact" says, 0 = the parity CSR (every stored entry), 1 = the solver's compacted stream
int spmv_owned(fedd_ctx* c, const double* d_x_owned, double* d_y_owned, bool x_has_tail = false, const double* d_sub = nullptr,
               double theta = 0.0, int use_compact = -1);   // incl. ghost import
int halo_import(fedd_ctx* c, double* d_xcol, int dofs);                    // fill ghost tail
int read_bandwidth(fedd_ctx* c, int64_t bytes, int reps, double* gbs);     // read-only streaming calibration

// schwarz.hip
int schwarz_setup(fedd_ctx* c);
int schwarz_apply(fedd_ctx* c, const double* d_r_owned, double* d_z_owned, bool r_has_tail = false);

// The row hash of the Schwarz fingerprints (schwarz.hip k_row_hash) as the two kernels that form it share it: 128 bits,
// order-independent (wrapping sums), over (column - row, value quantised to 2^-44 of the row's largest magnitude) of every
// entry that does not quantise to zero.
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
__device__ __forceinline__ double row_hash_scale(double row_max) { return row_max > 0.0 ? 17592186044416.0 / row_max : 0.0; }   // 2^44 / row max
__device__ __forceinline__ void row_hash_add(double a, double scale, int32_t cidx, int32_t r, uint64_t& h1, uint64_t& h2) {
    const int64_t qv = (int64_t)llrint(a * scale);
    if (qv == 0) return;
    const uint64_t key = (uint64_t)(uint32_t)(cidx - r);
    h1 += mix64((key + 0x2545f4914f6cdd1dull) * 0x9e3779b97f4a7c15ull + (uint64_t)qv);
    h2 += mix64((key + 0x632be59bd9b4e019ull) * 0xd6e8feb86659fd93ull ^ ((uint64_t)qv * 0xa0761d6478bd642full));
}
// spmv.hip, option "setup_fused": one walk over the finished rows for the Schwarz setup's row maxima and row hashes AND the
// check of the kept SpMV stream (spmv_reuse_try finds its result in fedd_ctx::setup_walk).  *ran = false: there is no stream to
// check against (or the rows are not the stream's), nothing was launched and the caller runs its own kernel.
int setup_walk(fedd_ctx* c, double* d_rmax, uint64_t* d_row_hash, bool* ran);
// schwarz_sym.hip: Full / Averaging combine by park + gather (no floating-point atomics, fixed summation order)
int schwarz_sym_setup(fedd_ctx* c);
int schwarz_apply_sym(fedd_ctx* c, const double* d_r_cols, double* d_z_owned);
int bounding_box(fedd_ctx* c, int64_t n_nodes, double lo[3], double hi[3], double* d_scratch = nullptr);   // of d_xyz[0, n_nodes)
int global_box(fedd_ctx* c, int64_t n_own, double lo[3], double hi[3], double* n_global);   // over all ranks

// schwarz_big.hip: subdomains of up to 1024 dofs (balanced coordinate-bisection boxes, batched dense inverses on the
// f64 matrix cores); the default for merged block systems (option "schwarz_big": -1 auto, 0 never, 1 always)
bool schwarz_use_big(const fedd_ctx* c);
int schwarz_setup_big(fedd_ctx* c);
int schwarz_apply_big(fedd_ctx* c, const double* d_r_owned, double* d_z_owned, bool r_has_tail);
int schwarz_overlap_lists_big(fedd_ctx* c, int64_t nsub, int32_t* max_n, int32_t* max_own);
int schwarz_slab_offsets(fedd_ctx* c, int64_t nsub, int restricted);
int schwarz_dense_batched(fedd_ctx* c, int64_t nsub, int dstride, int n_lo, int32_t p_off, int restricted, int max_n,
                          int32_t* d_bad, const int32_t* d_sub_n_sel);

// invert_mfma.hip: local inverses of plain systems, n <= 128, on the f64 matrix cores
int schwarz_invert_mfma(fedd_ctx* c, int restricted, int32_t* d_bad, int max_n);

// dense.hip: in-place inverses of a batch of dense matrices on the f64 matrix cores (blocked Gauss-Jordan, no pivoting)
int dense_invert_batched(fedd_ctx* c, double* K, int64_t ld, int batch, int64_t stride, const int32_t* d_nblk,
                         int max_nblk, int spd, int32_t* d_bad);

// coarse.hip
int coarse_setup(fedd_ctx* c);
int coarse_apply_add(fedd_ctx* c, const double* d_r_owned, double* d_z_owned);   // z += Phi K0^-1 Phi^T r
// the multiplicative level combination is in force: asked for (sw_levels) and a coarse level built.  The GDSW extension solves
// run before have_coarse is set, and so stay one-level
inline bool levels_mult(const fedd_ctx* c) { return c->sw_levels == FEDD_LEVELS_MULTIPLICATIVE && c->have_coarse; }
int coarse_apply_mult(fedd_ctx* c, double* d_z_owned);   // z -= Phi K0^-1 Phi^T (A z)

// multi.hip: operator and one-level Schwarz preconditioner on sixteen stacked right-hand sides, X[row * MULTI_NR + j]
constexpr int MULTI_NR = 16;
bool multi_rhs_ok(const fedd_ctx* c);
int spmm_owned(fedd_ctx* c, double* d_X, double* d_Y, const double* mk, const double* alt);
int schwarz_apply_multi(fedd_ctx* c, double* d_R, double* d_Z, const double* mk);

// gmres.hip (dispatcher, one-vector solvers), gmres_sstep.hip (s-step solver, capture)
struct GmresCall {
    const double* b;                // right-hand side (device, owned rows)
    double* x;                      // solution; the initial guess if x0
    double rtol;
    int max_it, restart, use_prec;
    bool x0 = false;                // start from the vector in x ("Zero Initial Guess" = false) instead of zero
    const double* mask = nullptr;   // != nullptr: the constrained system (dofs with mask 0 held), see Frame in gmres_frame.hpp
    int nr = 1;                     // > 1: stacked vectors X[row * nr + j] (multi.hip; the GDSW extension solves)
};
int gmres_solve(fedd_ctx* c, const GmresCall& call, int* its_out, double* relres_out);
int gmres_capture_arm(fedd_ctx* c, int block);
int gmres_capture_get(fedd_ctx* c, const char* what, double* out, int64_t cap);
int allreduce_sum(fedd_ctx* c, double* d_buf, int n);

// cg.hip
struct CgCall {
    const double* b;                // right-hand side (device, owned rows)
    double* x;                      // solution; the initial guess if x0
    double rtol;
    int max_it, use_prec;
    bool x0 = false;
};
int cg_solve(fedd_ctx* c, const CgCall& call, int* its_out, double* relres_out);

// FE tables (fe_tables.cpp): reference-simplex quadrature and basis values
struct FeTables {
    int dim = 0, nen = 0, nq = 0;
    std::vector<double> w;      // [nq]
    std::vector<double> phi;    // [nq*nen]
    std::vector<double> dphi;   // [nq*nen*dim]
};
int fe_quadrature(int dim, int degree, std::vector<double>& pts, std::vector<double>& w);
int fe_tables(int dim, int nen, int degree, FeTables& out);
int fe_surface_base(int dim, int nsn, int extra_degree, double* base);   // sum_q w_q phi_q,i of the surface form, base[nsn]
int fe_degree(int nen, int dim, bool grad);   // determineDegree building block: P1 Std 1/Grad 0, P2 2/1

}  // namespace fedd
