// extern "C" entry points: context, mesh upload, read-back, timing.  gfx950 only.
#include "fedd_internal.hpp"
#include <rccl/rccl.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <unordered_map>

namespace fedd {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

int timing_flush(fedd_ctx* c) {
    for (int t = 0; t < FEDD_T_COUNT; ++t) {
        auto& s = c->timers[t];
        for (auto& pr : s.pending) {
            float ms = 0.f;
            FEDD_HIP(hipEventSynchronize(pr.second));
            FEDD_HIP(hipEventElapsedTime(&ms, pr.first, pr.second));
            s.total_ms += ms;
            if (!pr.cont) s.launches += 1;
            c->ev_pool.push_back(pr.first);
            c->ev_pool.push_back(pr.second);
        }
        s.pending.clear();
    }
    return 0;
}

}  // namespace fedd

using namespace fedd;

extern "C" const char* fedd_last_error(void) { return g_err.c_str(); }

extern "C" int fedd_nccl_unique_id(void* id128) {
    FEDD_CHECK(id128, "fedd_nccl_unique_id: null output");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    FEDD_CHECK(r == ncclSuccess, "ncclGetUniqueId: %s", ncclGetErrorString(r));
    memcpy(id128, &id, 128);
    return 0;
}

extern "C" int fedd_ctx_create(fedd_ctx** out, int device, const void* nccl_unique_id, int rank, int nranks) {
    FEDD_CHECK(out, "fedd_ctx_create: null output pointer");
    FEDD_CHECK(nranks >= 1 && rank >= 0 && rank < nranks, "fedd_ctx_create: bad rank %d of %d", rank, nranks);
    fedd_ctx* c = new fedd_ctx();
    static std::atomic<uint64_t> next_uid{0};
    c->uid = ++next_uid;
    c->device = device;
    c->rank = rank;
    c->nranks = nranks;
    if (device >= 0) {
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0) {
            set_error("fedd_ctx_create: no HIP device visible (%s); this library has no CPU path",
                      hipGetErrorString(e));
            delete c;
            return 1;
        }
        if (device >= ndev) {
            set_error("fedd_ctx_create: device %d requested, %d visible", device, ndev);
            delete c;
            return 1;
        }
        if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) {
            set_error("fedd_ctx_create: cannot initialise device %d", device);
            delete c;
            return 1;
        }
        if (hipHostMalloc((void**)&c->h_pinned, 4096 * sizeof(double), hipHostMallocMapped) != hipSuccess) {
            set_error("fedd_ctx_create: pinned allocation failed");
            fedd_ctx_destroy(c);   // frees the stream too
            return 1;
        }
        // the solver's small kernel writes its convergence numbers straight into this buffer (option "gmres_hostwrite" 0: copies)
        if (hipHostGetDevicePointer((void**)&c->h_pinned_dev, c->h_pinned, 0) != hipSuccess) c->h_pinned_dev = nullptr;
        c->h_pinned_map = c->h_pinned_dev;
        if (nranks > 1 && nccl_unique_id) {  // without an id: host-callback transport (tests only)
            ncclUniqueId id;
            memcpy(&id, nccl_unique_id, 128);
            ncclComm_t comm;
            ncclResult_t r = ncclCommInitRank(&comm, nranks, id, rank);
            if (r != ncclSuccess) {
                set_error("ncclCommInitRank: %s", ncclGetErrorString(r));
                fedd_ctx_destroy(c);   // frees the stream and the pinned buffer
                return 1;
            }
            c->comm = comm;
        }
    }
    *out = c;
    // FEDD_OPTIONS=key=value,...: fedd_set_option calls applied to every new context (the solver defaults stay
    // switchable from the environment of a multi-GPU run -- e.g. FEDD_OPTIONS=gmres_kind=0,halo_overlap=1 -- without a rebuild)
    if (const char* env = getenv("FEDD_OPTIONS")) {
        std::string all(env);
        size_t pos = 0;
        while (pos < all.size()) {
            size_t end = all.find(',', pos);
            if (end == std::string::npos) end = all.size();
            const std::string kv = all.substr(pos, end - pos);
            const size_t eq = kv.find('=');
            if (eq != std::string::npos && eq > 0) {
                char* endp = nullptr;
                const double v = strtod(kv.c_str() + eq + 1, &endp);
                if (endp != kv.c_str() + eq + 1 && fedd_set_option(c, kv.substr(0, eq).c_str(), v) != 0) {
                    fedd_ctx_destroy(c);
                    *out = nullptr;
                    return 1;       // (fedd_set_option set the message: an unknown key is an error, not ignored)
                }
            }
            pos = end + 1;
        }
    }
    return 0;
}

extern "C" void fedd_ctx_destroy(fedd_ctx* c) {
    if (!c) return;
    prec_child_gone(c);         // parents that apply this context as a block (block preconditioner, FaCSI) are detached, their
    prec_unlink(c);             // streams finished first ... and this context's own children forget it
    iface_release(c);           // the other side of a match finds it released
    if (c->device >= 0) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        (void)timing_flush(c);
        for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
        c->ev_pool.clear();
        if (c->comm) ncclCommDestroy((ncclComm_t)c->comm);
        // (the device buffers are DevBuf members: `delete c` below frees them)
        if (c->h_pinned) (void)hipHostFree(c->h_pinned);
        if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
        if (c->ev_join) (void)hipEventDestroy(c->ev_join);
        if (c->prec.ev) (void)hipEventDestroy(c->prec.ev);
        if (c->stream2) (void)hipStreamDestroy(c->stream2);
        (void)hipStreamDestroy(c->stream);
    }
    delete c;
}

extern "C" int fedd_sync(fedd_ctx* c) {
    NEED_DEVICE(c);
    FEDD_HIP(hipStreamSynchronize(c->stream));
    // an attached preconditioner runs its children's applies in this stream; their own streams hold their setups
    for (const PrecChild& ch : c->prec.child)
        if (ch.ctx && ch.ctx->device >= 0) FEDD_HIP(hipStreamSynchronize(ch.ctx->stream));
    return 0;
}

static int mesh_set_impl(fedd_ctx* c, int dim, int nen, int64_t n_elem, const int32_t* conn, int64_t n_rep,
                         const double* xyz, const int64_t* gid_rep, int64_t n_uni, const int64_t* gid_uni,
                         const int32_t* bcflag_uni, int64_t n_rg, const int64_t* rg_gid, const int32_t* rg_flag) {
    FEDD_CHECK(c, "fedd_mesh_set: null context");
    FEDD_CHECK(dim == 2 || dim == 3, "fedd_mesh_set: dimension must be 2 or 3");
    const bool okel = (dim == 2 && (nen == 3 || nen == 6)) || (dim == 3 && (nen == 4 || nen == 10));
    FEDD_CHECK(okel, "fedd_mesh_set: unsupported element with %d nodes in %dD (P1/P2 simplices only)", nen, dim);
    FEDD_CHECK(n_elem >= 0 && n_rep >= 0 && n_uni >= 0, "fedd_mesh_set: negative size");
    FEDD_CHECK(n_rep < (int64_t)1 << 31 && n_elem * nen < (int64_t)1 << 31,
               "fedd_mesh_set: local mesh too large for 32-bit local ordinals");
    FEDD_CHECK((n_elem == 0 || conn) && (n_rep == 0 || (xyz && gid_rep)) && (n_uni == 0 || gid_uni),
               "fedd_mesh_set: null array");
    c->dim = dim;
    c->nen = nen;
    c->n_elem = n_elem;
    c->n_own = n_uni;
    c->n_rowg = 0;
    system_written(c, SYS_VALUES | SYS_PATTERN | SYS_GONE);
    c->have_adj = false;
    c->tl_state = 0;     // the assembly's tile structures belong to the old mesh
    gather_lists_reset(c);  // ... and so do the gather lists (with gl_adv: the pattern and tables of the advection matrices)
    c->have_vel = false;    // the velocity belonged to the old nodes
    c->have_mvel = false;   // ... and so did the mesh velocity, whose buffer goes with them
    c->d_mvel.release();
    c->have_idist = c->have_lscale = false;   // ... and the interface distances and the coefficients made from them
    c->n_interface = 0;
    c->d_idist.release();
    c->d_lscale.release();
    iface_release(c);       // ... and the matched interface, on both sides (a coupled system built on it finds it released)
    c->fsi_coupled = false; // (a coupled context that is given a mesh is an ordinary context again)
    c->have_hy_f = false;   // ... and the force vector of the hyperelastic path
    c->nw_active = c->nw_have_src = c->nw_f_fresh = false;   // ... and the Newton state (newton.hip)
    c->nw_n = -1;
    c->have_surf = false;   // ... and the surface elements
    c->n_surf = 0;
    for (auto& id : c->adv_pattern_id) id = 0;
    c->d_adv_ke.release();   // the element-block scratch is sized by the mesh (the largest buffer of the advection path)
    c->absdet_valid = false; // ... and so is |det B| of the old elements (assemble_rhs, option "setup_fused")
    c->d_absdet.release();
    ++c->mesh_id;
    c->nm_n = -1;           // the Newmark state belonged to the old rows
    c->ms_order = c->ms_count = 0;   // ... and so did the multistep history, whose buffers go with it
    c->ms_n = -1;
    c->d_ms_u[0].release();
    c->d_ms_u[1].release();
    c->d_ms_t.release();
    c->st_max = c->st_count = 0;     // ... and the stage store of a single-step loop (singlestep.hip)
    c->st_slot = -1;
    c->st_pattern_id = 0;
    c->st_nnz = c->st_n = c->st_rows = 0;
    for (int j = 0; j < fedd::MAX_STAGES; ++j) {
        c->d_st_val[j].release();
        c->d_st_u[j].release();
    }
    c->d_st_part.release();
    ++c->mesh_gen;         // the Schwarz structure (schwarz.hip) belongs to the old nodes
    c->have_xref = false;   // the coordinates uploaded below are the new reference of fedd_mesh_move
    c->n_moves = 0;
    c->min_det_ratio = 1.0;
    c->halo.reset();

    // column-local numbering: owned nodes in unique-map order, then ghosts sorted by global id
    std::unordered_map<int64_t, int32_t> own;
    own.reserve((size_t)n_uni * 2);
    for (int64_t i = 0; i < n_uni; ++i) {
        auto ins = own.emplace(gid_uni[i], (int32_t)i);
        FEDD_CHECK(ins.second, "fedd_mesh_set: global id %lld listed twice in the unique map", (long long)gid_uni[i]);
    }
    // row ghosts (nodes of other ranks whose rows are complete here) are numbered before the other ghosts
    std::unordered_map<int64_t, int32_t> rowg;
    rowg.reserve((size_t)n_rg * 2);
    for (int64_t i = 0; i < n_rg; ++i) {
        FEDD_CHECK(own.find(rg_gid[i]) == own.end(), "fedd_mesh_set_rows: node %lld is owned by this rank", (long long)rg_gid[i]);
        auto ins = rowg.emplace(rg_gid[i], rg_flag ? rg_flag[i] : 0);
        FEDD_CHECK(ins.second, "fedd_mesh_set_rows: global id %lld listed twice", (long long)rg_gid[i]);
    }
    const int64_t CLASS2 = (int64_t)1 << 62;        // sort key offset of the ghosts without rows
    std::vector<int32_t> col_of_rep((size_t)n_rep, -1);
    std::vector<std::pair<int64_t, int32_t>> ghosts;
    std::vector<char> seen((size_t)n_uni, 0);
    for (int64_t i = 0; i < n_rep; ++i) {
        auto it = own.find(gid_rep[i]);
        if (it != own.end()) {
            col_of_rep[i] = it->second;
            seen[it->second] = 1;
        } else {
            FEDD_CHECK(gid_rep[i] >= 0 && gid_rep[i] < CLASS2, "fedd_mesh_set: global id %lld out of range", (long long)gid_rep[i]);
            ghosts.emplace_back(gid_rep[i] + (rowg.count(gid_rep[i]) ? 0 : CLASS2), (int32_t)i);
        }
    }
    for (int64_t i = 0; i < n_uni; ++i)
        FEDD_CHECK(seen[i], "fedd_mesh_set: unique node %lld is missing from the repeated map", (long long)gid_uni[i]);
    std::sort(ghosts.begin(), ghosts.end());
    int64_t ng = 0, ng_rows = 0;
    std::vector<int64_t> ghost_gid;
    std::vector<int32_t> flags_rg;
    for (size_t k = 0; k < ghosts.size(); ++k) {
        if (k == 0 || ghosts[k].first != ghosts[k - 1].first) {
            const bool with_rows = ghosts[k].first < CLASS2;
            const int64_t g = with_rows ? ghosts[k].first : ghosts[k].first - CLASS2;
            ghost_gid.push_back(g);
            if (with_rows) {
                flags_rg.push_back(rowg[g]);
                ++ng_rows;
            }
            ++ng;
        }
        col_of_rep[ghosts[k].second] = (int32_t)(n_uni + ng - 1);
    }
    FEDD_CHECK(ng_rows == n_rg, "fedd_mesh_set_rows: %lld of the %lld row ghosts are not in the repeated map",
               (long long)(n_rg - ng_rows), (long long)n_rg);
    c->n_rowg = ng_rows;
    c->n_node = n_uni + ng;
    c->h_col_of_rep = col_of_rep;
    c->h_node_gid.assign(gid_uni, gid_uni + n_uni);
    c->h_node_gid.insert(c->h_node_gid.end(), ghost_gid.begin(), ghost_gid.end());

    std::vector<int32_t> conn2((size_t)(n_elem * nen));
    for (int64_t k = 0; k < n_elem * nen; ++k) {
        FEDD_CHECK(conn[k] >= 0 && conn[k] < n_rep, "fedd_mesh_set: element node id %d out of range", conn[k]);
        conn2[k] = col_of_rep[conn[k]];
    }
    if (ng_rows > 0) {
        // only the row ghosts are imported in the halo exchange: every column of an owned row must be one
        const int32_t first_plain = (int32_t)(n_uni + ng_rows);
        for (int64_t e = 0; e < n_elem; ++e) {
            bool touches_owned = false, has_plain = false;
            for (int v = 0; v < nen; ++v) {
                const int32_t id = conn2[e * nen + v];
                touches_owned = touches_owned || id < n_uni;
                has_plain = has_plain || id >= first_plain;
            }
            FEDD_CHECK(!(touches_owned && has_plain),
                       "fedd_mesh_set_rows: element %lld joins an owned node and a ghost node that is not listed as a row ghost",
                       (long long)e);
        }
    }
    std::vector<double> xyz2((size_t)(c->n_node * dim));
    for (int64_t i = 0; i < n_rep; ++i)
        for (int d = 0; d < dim; ++d) xyz2[(size_t)col_of_rep[i] * dim + d] = xyz[i * dim + d];

    if (c->device < 0) return 0;  // host-only context: numbering only
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_TRY(c->d_conn.ensure(conn2.size()));
    FEDD_TRY(c->d_xyz.ensure(xyz2.size()));
    FEDD_TRY(c->d_flag.ensure((size_t)(n_uni + ng_rows)));
    FEDD_HIP(hipMemcpyAsync(c->d_conn.p, conn2.data(), conn2.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipMemcpyAsync(c->d_xyz.p, xyz2.data(), xyz2.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (bcflag_uni)
        FEDD_HIP(hipMemcpyAsync(c->d_flag.p, bcflag_uni, (size_t)n_uni * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    else
        FEDD_HIP(hipMemsetAsync(c->d_flag.p, 0, (size_t)n_uni * sizeof(int32_t), c->stream));
    if (ng_rows)
        FEDD_HIP(hipMemcpyAsync(c->d_flag.p + n_uni, flags_rg.data(), (size_t)ng_rows * sizeof(int32_t), hipMemcpyHostToDevice,
                                c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fedd_mesh_set(fedd_ctx* c, int dim, int nen, int64_t n_elem, const int32_t* conn,
                             int64_t n_rep, const double* xyz, const int64_t* gid_rep, int64_t n_uni,
                             const int64_t* gid_uni, const int32_t* bcflag_uni) {
    return mesh_set_impl(c, dim, nen, n_elem, conn, n_rep, xyz, gid_rep, n_uni, gid_uni, bcflag_uni, 0, nullptr, nullptr);
}

extern "C" int fedd_mesh_set_rows(fedd_ctx* c, int dim, int nen, int64_t n_elem, const int32_t* conn, int64_t n_rep,
                                  const double* xyz, const int64_t* gid_rep, int64_t n_uni, const int64_t* gid_uni,
                                  const int32_t* bcflag_uni, int64_t n_row_ghosts, const int64_t* row_ghost_gid,
                                  const int32_t* row_ghost_bcflag) {
    FEDD_CHECK(n_row_ghosts >= 0 && (n_row_ghosts == 0 || row_ghost_gid), "fedd_mesh_set_rows: null row-ghost list");
    return mesh_set_impl(c, dim, nen, n_elem, conn, n_rep, xyz, gid_rep, n_uni, gid_uni, bcflag_uni, n_row_ghosts,
                         row_ghost_gid, row_ghost_bcflag);
}

extern "C" int fedd_mesh_move(fedd_ctx* c, const double* disp_rep) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_mesh_move: call fedd_mesh_set first");
    FEDD_HIP(hipSetDevice(c->device));
    return mesh_move(c, disp_rep);
}

extern "C" int fedd_mesh_move_info(fedd_ctx* c, int64_t* n_moves, int64_t* geometry_id, double* min_det_ratio) {
    FEDD_CHECK(c, "fedd_mesh_move_info: null context");
    if (n_moves) *n_moves = c->n_moves;
    if (geometry_id) *geometry_id = (int64_t)c->geometry_id;
    if (min_det_ratio) *min_det_ratio = c->min_det_ratio;
    return 0;
}

extern "C" int fedd_mesh_coords_get(fedd_ctx* c, double* xyz_rep) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_mesh_coords_get: call fedd_mesh_set first");
    FEDD_CHECK(xyz_rep, "fedd_mesh_coords_get: null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    return mesh_coords_get(c, xyz_rep);
}

extern "C" int fedd_interface_distance(fedd_ctx* c, int n_flags, const int32_t* flags, int64_t* n_interface) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_interface_distance: call fedd_mesh_set first");
    FEDD_CHECK(n_flags >= 0, "fedd_interface_distance: negative number of flags %d", n_flags);
    FEDD_CHECK(n_flags == 0 || flags, "fedd_interface_distance: null flag list");
    FEDD_HIP(hipSetDevice(c->device));
    return interface_distance_flags(c, n_flags, flags, n_interface);
}

extern "C" int fedd_interface_distance_points(fedd_ctx* c, int64_t n_pts, const double* xyz_pts) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_interface_distance_points: call fedd_mesh_set first");
    FEDD_CHECK(n_pts >= 0, "fedd_interface_distance_points: negative number of points %lld", (long long)n_pts);
    FEDD_CHECK(n_pts == 0 || xyz_pts, "fedd_interface_distance_points: null point array");
    FEDD_HIP(hipSetDevice(c->device));
    return interface_distance_points(c, n_pts, xyz_pts);
}

extern "C" int fedd_interface_distance_set(fedd_ctx* c, const double* dist_rep) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_interface_distance_set: call fedd_mesh_set first");
    FEDD_HIP(hipSetDevice(c->device));
    return interface_distance_set(c, dist_rep);
}

extern "C" int fedd_interface_distance_get(fedd_ctx* c, double* dist_rep) {
    NEED_DEVICE(c);
    FEDD_CHECK(dist_rep, "fedd_interface_distance_get: null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    return interface_distance_get(c, dist_rep);
}

extern "C" int fedd_interface_distance_info(fedd_ctx* c, int* have, int64_t* n_interface, int* tile_points) {
    FEDD_CHECK(c, "fedd_interface_distance_info: null context");
    if (have) *have = c->have_idist ? 1 : 0;
    if (n_interface) *n_interface = c->n_interface;
    if (tile_points) *tile_points = interface_distance_tile();
    return 0;
}

extern "C" int fedd_laplace_scale_get(fedd_ctx* c, double* f_elem) {
    NEED_DEVICE(c);
    FEDD_CHECK(f_elem, "fedd_laplace_scale_get: null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    return laplace_scale_get(c, f_elem);
}

extern "C" int fedd_pattern_build(fedd_ctx* c, int dofs_per_node, int block_mode, int64_t* nnz_out) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_pattern_build: call fedd_mesh_set first");
    FEDD_CHECK(dofs_per_node >= 1 && dofs_per_node <= MAX_DOFS, "fedd_pattern_build: dofs_per_node %d", dofs_per_node);
    FEDD_CHECK(block_mode >= 0 && block_mode <= 2, "fedd_pattern_build: block mode %d", block_mode);
    FEDD_CHECK((dofs_per_node == 1) == (block_mode == FEDD_BLOCK_SCALAR),
               "fedd_pattern_build: block mode SCALAR <=> one dof per node");
    FEDD_HIP(hipSetDevice(c->device));
    {
        // (a build that repeats runs nothing of the symbolic class, and is not counted as a launch of it: a time loop on a moving
        // mesh shows by this counter that a move costs no symbolic work)
        ScopedTimer t(c, c->have_adj && pattern_repeats(c, dofs_per_node, block_mode) ? -1 : FEDD_T_SYMBOLIC);
        if (!c->have_adj) FEDD_TRY(build_adjacency(c));
        FEDD_TRY(build_pattern(c, dofs_per_node, block_mode));
    }
    if (nnz_out) *nnz_out = c->nnz;
    return 0;
}

// (an imported system, or a merge of blocks of an earlier mesh, has a pattern without the adjacency the assembly kernels walk)
// (the coupled context of fedd_fsi_merge holds a system and never a mesh)
static const char* const NO_MESH = "this context carries no mesh (a coupled context of fedd_fsi_merge never does): the call needs "
                                   "the nodes of a fedd_mesh_set";
static const char* const NO_ADJACENCY = "this context has not built the node -> element adjacency of its mesh (the system matrix "
                                        "was imported or merged, not built here): fedd_pattern_build builds it";

extern "C" int fedd_assemble(fedd_ctx* c, int form, const double* params) {
    NEED_DEVICE(c);
    if (form == FEDD_FORM_LAPLACE_XDIM)     // (before the pattern: a context of several ranks is refused whatever it holds)
        FEDD_CHECK(c->nranks == 1, "fedd_assemble(FEDD_FORM_LAPLACE_XDIM): one rank only (a context with %d ranks was given)", c->nranks);
    FEDD_CHECK(c->have_pattern, "fedd_assemble: call fedd_pattern_build first");
    FEDD_CHECK(c->have_adj, "fedd_assemble: %s", NO_ADJACENCY);
    FEDD_HIP(hipSetDevice(c->device));
    return assemble_matrix(c, form, params);
}

extern "C" int fedd_assemble_stress(fedd_ctx* c, const double* coeff_q, int64_t n_coeff) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_assemble_stress: no pattern; call fedd_pattern_build(dim, FEDD_BLOCK_FULL) first");
    FEDD_CHECK(c->have_adj, "fedd_assemble_stress: %s", NO_ADJACENCY);
    FEDD_CHECK(!coeff_q || n_coeff >= 0, "fedd_assemble_stress: negative n_coeff %lld", (long long)n_coeff);
    FEDD_HIP(hipSetDevice(c->device));
    return assemble_matrix(c, FEDD_FORM_STRESS, nullptr, coeff_q, n_coeff);
}

extern "C" int fedd_assemble_rhs(fedd_ctx* c, int dofs_per_node, const double* f_const, int extra_degree) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_assemble_rhs: call fedd_pattern_build first");
    FEDD_CHECK(c->have_adj, "fedd_assemble_rhs: %s", NO_ADJACENCY);
    FEDD_CHECK(dofs_per_node == c->dofs, "fedd_assemble_rhs: dofs_per_node %d differs from the pattern's %d", dofs_per_node, c->dofs);
    FEDD_CHECK(f_const, "fedd_assemble_rhs: null f_const");
    FEDD_HIP(hipSetDevice(c->device));
    return assemble_rhs(c, dofs_per_node, f_const, extra_degree);
}

extern "C" int fedd_surface_set(fedd_ctx* c, int nsn, int64_t n_surf, const int32_t* surf, const int32_t* sflag) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_surface_set: call fedd_mesh_set first");
    const bool okel = nsn == c->dim || (c->dim == 2 && nsn == 3) || (c->dim == 3 && nsn == 6);
    FEDD_CHECK(okel, "fedd_surface_set: surface elements of a %dD mesh have %d (P1) or %d (P2) nodes, not %d", c->dim, c->dim,
               c->dim == 2 ? 3 : 6, nsn);
    FEDD_CHECK(n_surf >= 0 && n_surf * nsn < (int64_t)1 << 31, "fedd_surface_set: bad number of surface elements %lld", (long long)n_surf);
    FEDD_CHECK(n_surf == 0 || (surf && sflag), "fedd_surface_set: null array");
    FEDD_HIP(hipSetDevice(c->device));
    return surface_set(c, nsn, n_surf, surf, sflag);
}

static int surface_entry(fedd_ctx* c, const char* who, int dofs, int n_flags, const int32_t* flags, const double* g,
                         const double* g_surf, int extra_degree, int accumulate) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern && !c->merged, "%s: call fedd_pattern_build first (the load vector of a block, not of a merged system)", who);
    FEDD_CHECK(c->have_surf, "%s: call fedd_surface_set first", who);
    FEDD_CHECK(dofs == c->dofs, "%s: dofs_per_node %d differs from the pattern's %d", who, dofs, c->dofs);
    FEDD_CHECK(n_flags >= 0 && (n_flags == 0 || flags), "%s: null flag list", who);
    FEDD_CHECK(g || g_surf || c->n_surf == 0, "%s: null load array", who);
    FEDD_CHECK(extra_degree >= 0, "%s: negative extra degree", who);
    FEDD_CHECK(accumulate == 0 || accumulate == 1, "%s: accumulate must be 0 or 1", who);
    FEDD_HIP(hipSetDevice(c->device));
    return assemble_surface(c, dofs, n_flags, flags, g, g_surf, extra_degree, accumulate);
}

extern "C" int fedd_assemble_surface(fedd_ctx* c, int dofs_per_node, int n_flags, const int32_t* flags, const double* g,
                                     int extra_degree, int accumulate) {
    FEDD_CHECK(g, "fedd_assemble_surface: null load array");
    return surface_entry(c, "fedd_assemble_surface", dofs_per_node, n_flags, flags, g, nullptr, extra_degree, accumulate);
}

extern "C" int fedd_assemble_surface_values(fedd_ctx* c, int dofs_per_node, const double* g_surf, int extra_degree, int accumulate) {
    return surface_entry(c, "fedd_assemble_surface_values", dofs_per_node, 0, nullptr, nullptr, g_surf, extra_degree, accumulate);
}

extern "C" int fedd_dirichlet(fedd_ctx* c, int n_bc, const int32_t* flags, const int32_t* comp_mask, const double* values) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_dirichlet: call fedd_pattern_build first");
    FEDD_CHECK(c->n_node > 0, "fedd_dirichlet: %s", NO_MESH);
    FEDD_CHECK(n_bc >= 0 && n_bc <= MAX_BC, "fedd_dirichlet: at most %d boundary conditions", MAX_BC);
    FEDD_CHECK(n_bc == 0 || (flags && values), "fedd_dirichlet: null array");
    FEDD_HIP(hipSetDevice(c->device));
    return apply_dirichlet(c, n_bc, flags, comp_mask, values);
}

extern "C" int fedd_dirichlet_nodes(fedd_ctx* c, int64_t n, const int32_t* owned_nodes, const int32_t* comp_mask,
                                    const double* values) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_dirichlet_nodes: call fedd_pattern_build first");
    FEDD_CHECK(c->n_node > 0, "fedd_dirichlet_nodes: %s", NO_MESH);
    FEDD_CHECK(n >= 0 && (n == 0 || (owned_nodes && values)), "fedd_dirichlet_nodes: null array");
    FEDD_HIP(hipSetDevice(c->device));
    return apply_dirichlet_nodes(c, n, owned_nodes, comp_mask, values);
}

extern "C" int fedd_dirichlet_rows(fedd_ctx* c, int64_t n, const int32_t* rows, const double* values) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_dirichlet_rows: no system matrix");
    FEDD_CHECK(n >= 0 && (n == 0 || (rows && values)), "fedd_dirichlet_rows: null array");
    FEDD_HIP(hipSetDevice(c->device));
    return apply_dirichlet_rows(c, n, rows, values);
}

extern "C" int fedd_matrix_store(fedd_ctx* c, int slot) {
    NEED_DEVICE(c);
    CHECK_SLOT(slot);
    FEDD_CHECK(c->have_pattern, "fedd_matrix_store: no system matrix");
    FEDD_HIP(hipSetDevice(c->device));
    return matrix_store(c, slot);
}

extern "C" int fedd_matrix_scale(fedd_ctx* c, int slot, double alpha) {
    NEED_DEVICE(c);
    if (slot >= 0) {
        CHECK_SLOT(slot);
        FEDD_CHECK(c->aux[slot].valid, "fedd_matrix_scale: slot %d is empty", slot);
    } else {
        FEDD_CHECK(c->have_pattern, "fedd_matrix_scale: no system matrix");
    }
    FEDD_HIP(hipSetDevice(c->device));
    return matrix_scale(c, slot, alpha);
}

extern "C" int fedd_assemble_div(fedd_ctx* c, int64_t n_pressure_nodes, int slot_b, int slot_bt) {
    NEED_DEVICE(c);
    CHECK_SLOT(slot_b);
    CHECK_SLOT(slot_bt);
    FEDD_CHECK(slot_b != slot_bt, "fedd_assemble_div: B and B^T need different slots");
    FEDD_CHECK(c->n_node > 0, "fedd_assemble_div: call fedd_mesh_set first");
    FEDD_HIP(hipSetDevice(c->device));
    return assemble_div(c, n_pressure_nodes, slot_b, slot_bt);
}

extern "C" int fedd_block_merge(fedd_ctx* c, int slot_a, int slot_bt, int slot_b, int slot_c) {
    NEED_DEVICE(c);
    CHECK_SLOT(slot_a);
    FEDD_CHECK(slot_bt < fedd::MAX_AUX && slot_b < fedd::MAX_AUX && slot_c < fedd::MAX_AUX, "fedd_block_merge: slot out of range");
    FEDD_HIP(hipSetDevice(c->device));
    return block_merge(c, slot_a, slot_bt, slot_b, slot_c);
}

extern "C" int fedd_block_merge_scaled(fedd_ctx* c, int slot_a, int slot_bt, double s_bt, int slot_b, int slot_c) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_block_merge_scaled");
    CHECK_SLOT(slot_a);
    FEDD_CHECK(slot_bt < fedd::MAX_AUX && slot_b < fedd::MAX_AUX && slot_c < fedd::MAX_AUX, "fedd_block_merge_scaled: slot out of range");
    FEDD_HIP(hipSetDevice(c->device));
    return block_merge_scaled(c, slot_a, slot_bt, s_bt, slot_b, slot_c);
}

extern "C" int fedd_velocity_set(fedd_ctx* c, const double* u_rep) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_velocity_set: call fedd_mesh_set first");
    FEDD_CHECK(u_rep, "fedd_velocity_set: null array");
    FEDD_HIP(hipSetDevice(c->device));
    return velocity_set(c, u_rep);
}

extern "C" int fedd_assemble_advection(fedd_ctx* c, int kind, double scale, int slot_add, int slot_out) {
    NEED_DEVICE(c);
    FEDD_CHECK(kind == FEDD_ADV_N || kind == FEDD_ADV_W || kind == FEDD_ADV_NEWTON, "fedd_assemble_advection: unknown kind %d", kind);
    CHECK_SLOT(slot_out);
    FEDD_CHECK(slot_add < fedd::MAX_AUX, "matrix slot %d out of range", slot_add);
    FEDD_CHECK(slot_add != slot_out, "fedd_assemble_advection: slot_add and slot_out must differ");
    FEDD_CHECK(c->n_node > 0, "fedd_assemble_advection: call fedd_mesh_set first");
    FEDD_HIP(hipSetDevice(c->device));
    return assemble_advection(c, kind, scale, slot_add, slot_out);
}

extern "C" int fedd_mesh_velocity_set(fedd_ctx* c, const double* w_rep) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_mesh_velocity_set: call fedd_mesh_set first");
    FEDD_HIP(hipSetDevice(c->device));
    return mesh_velocity_set(c, w_rep);
}

extern "C" int fedd_mesh_velocity_diff(fedd_ctx* c, const double* d_new_rep, const double* d_old_rep, double dt) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_mesh_velocity_diff: call fedd_mesh_set first");
    FEDD_CHECK(d_new_rep && d_old_rep, "fedd_mesh_velocity_diff: null array");
    FEDD_CHECK(std::isfinite(dt) && dt > 0.0, "fedd_mesh_velocity_diff: the time step must be positive and finite (dt = %g was given)", dt);
    FEDD_HIP(hipSetDevice(c->device));
    return mesh_velocity_diff(c, d_new_rep, d_old_rep, dt);
}

extern "C" int fedd_mesh_velocity_get(fedd_ctx* c, double* w_rep) {
    NEED_DEVICE(c);
    FEDD_CHECK(w_rep, "fedd_mesh_velocity_get: null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    return mesh_velocity_get(c, w_rep);
}

extern "C" int fedd_assemble_advection_ale(fedd_ctx* c, int kind, double scale, int slot_add, int slot_out) {
    NEED_DEVICE(c);
    FEDD_CHECK(kind == FEDD_ALE_P || kind == FEDD_ALE_FIXEDPOINT || kind == FEDD_ALE_NEWTON,
               "fedd_assemble_advection_ale: unknown kind %d", kind);
    CHECK_SLOT(slot_out);
    FEDD_CHECK(slot_add < fedd::MAX_AUX, "matrix slot %d out of range", slot_add);
    FEDD_CHECK(slot_add != slot_out, "fedd_assemble_advection_ale: slot_add and slot_out must differ");
    FEDD_CHECK(c->n_node > 0, "fedd_assemble_advection_ale: call fedd_mesh_set first");
    FEDD_HIP(hipSetDevice(c->device));
    return assemble_advection_ale(c, kind, scale, slot_add, slot_out);
}

extern "C" int fedd_assemble_hyperelastic(fedd_ctx* c, int model, const double* params, int n_params, int what) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->n_node > 0, "fedd_assemble_hyperelastic: call fedd_mesh_set first");
    FEDD_HIP(hipSetDevice(c->device));
    return assemble_hyperelastic(c, model, params, n_params, what);
}

extern "C" int fedd_assemble_hyperelastic_time(fedd_ctx* c, int model, const double* params, int n_params, int what, int slot_m,
                                               double cm) {
    NEED_DEVICE(c);
    CHECK_SLOT(slot_m);
    FEDD_CHECK(c->n_node > 0, "fedd_assemble_hyperelastic_time: call fedd_mesh_set first");
    FEDD_HIP(hipSetDevice(c->device));
    return assemble_hyperelastic_time(c, model, params, n_params, what, slot_m, cm);
}

extern "C" int fedd_hyperelastic_force_get(fedd_ctx* c, double* f_owned) {
    NEED_DEVICE(c);
    FEDD_CHECK(f_owned, "fedd_hyperelastic_force_get: null pointer");
    FEDD_CHECK(c->have_hy_f, "fedd_hyperelastic_force_get: no fedd_assemble_hyperelastic call with FEDD_HYPER_FORCE on this mesh yet");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_HIP(hipMemcpy(f_owned, c->d_hy_f.p, (size_t)c->n_own * c->dim * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int fedd_matrix_sizes(fedd_ctx* c, int slot, int64_t* n_rows, int64_t* n_cols, int64_t* nnz) {
    FEDD_CHECK(c, "null context");
    CHECK_SLOT(slot);
    FEDD_CHECK(c->aux[slot].valid, "fedd_matrix_sizes: slot %d is empty", slot);
    if (n_rows) *n_rows = c->aux[slot].n_rows;
    if (n_cols) *n_cols = c->aux[slot].n_cols;
    if (nnz) *nnz = c->aux[slot].nnz;
    return 0;
}

extern "C" int fedd_matrix_get(fedd_ctx* c, int slot, int64_t* rowptr, int32_t* colind, double* val) {
    NEED_DEVICE(c);
    CHECK_SLOT(slot);
    const fedd::DevCsr& m = c->aux[slot];
    FEDD_CHECK(m.valid, "fedd_matrix_get: slot %d is empty", slot);
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    if (rowptr) {
        std::vector<int32_t> rp((size_t)m.n_rows + 1);
        FEDD_HIP(hipMemcpy(rp.data(), m.rowptr.p, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < rp.size(); ++i) rowptr[i] = rp[i];
    }
    if (colind) FEDD_HIP(hipMemcpy(colind, m.colind.p, (size_t)m.nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (val) FEDD_HIP(hipMemcpy(val, m.val.p, (size_t)m.nnz * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int fedd_csr_sizes(fedd_ctx* c, int64_t* n_rows, int64_t* n_cols, int64_t* nnz) {
    FEDD_CHECK(c && c->have_pattern, "fedd_csr_sizes: no pattern");
    if (n_rows) *n_rows = c->n_rows;
    if (n_cols) *n_cols = c->n_cols;
    if (nnz) *nnz = c->nnz;
    return 0;
}

extern "C" int fedd_csr_get(fedd_ctx* c, int64_t* rowptr, int32_t* colind, double* val, int64_t* col_gid) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_csr_get: no pattern");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    if (rowptr) {
        std::vector<int32_t> rp((size_t)c->n_rows + 1);
        FEDD_HIP(hipMemcpy(rp.data(), c->d_rowptr.p, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < rp.size(); ++i) rowptr[i] = rp[i];
    }
    if (colind) FEDD_HIP(hipMemcpy(colind, c->d_colind.p, (size_t)c->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (val) FEDD_HIP(hipMemcpy(val, c->d_val.p, (size_t)c->nnz * sizeof(double), hipMemcpyDeviceToHost));
    if (col_gid && c->merged) {
        // BlockMap::merge: block-local global id + cumulated (maxAllGlobalIndex + 1) of the blocks before
        const int da = c->merged_dofsA;
        int64_t mx = -1;
        for (int64_t n = 0; n < c->n_own; ++n) mx = std::max(mx, c->h_node_gid[n]);
        const int64_t off = (mx + 1) * da;
        for (int64_t r = 0; r < c->merged_nA; ++r) col_gid[r] = c->h_node_gid[r / da] * da + r % da;
        for (int64_t r = c->merged_nA; r < c->n_rows; ++r) col_gid[r] = off + c->h_node_gid[r - c->merged_nA];
    } else if (col_gid)
        for (int64_t n = 0; n < c->n_node; ++n)
            for (int d = 0; d < c->dofs; ++d) col_gid[n * c->dofs + d] = c->h_node_gid[n] * c->dofs + d;
    return 0;
}

extern "C" int fedd_rhs_get(fedd_ctx* c, double* rhs) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern && rhs, "fedd_rhs_get: no pattern / null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_HIP(hipMemcpy(rhs, c->d_rhs.p, (size_t)c->n_rows * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int fedd_rhs_set(fedd_ctx* c, const double* rhs) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern && rhs, "fedd_rhs_set: no pattern / null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipMemcpy(c->d_rhs.p, rhs, (size_t)c->n_rows * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int fedd_solution_get(fedd_ctx* c, double* x) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern && x, "fedd_solution_get: no pattern / null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_HIP(hipMemcpy(x, c->d_x.p, (size_t)c->n_rows * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int fedd_spmv(fedd_ctx* c, const double* x_owned, double* y_owned) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern && x_owned && y_owned, "fedd_spmv: no matrix / null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_TRY(c->d_dtmp0.ensure((size_t)c->n_rows * 2));
    double* dx = c->d_dtmp0.p;
    double* dy = dx + c->n_rows;
    FEDD_HIP(hipMemcpyAsync(dx, x_owned, (size_t)c->n_rows * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // the caller's product (Matrix::apply, residual checks) is formed with the parity CSR itself, every stored entry:
    // the compacted stream that leaves out sub-ulp cancellation noise is the solver's private copy (fedd_spmv_device times it)
    // (option "spmv_exact_public" 0: this call runs the solver's stream instead -- how the tests reach those kernels)
    FEDD_TRY(spmv_owned(c, dx, dy, false, nullptr, 0.0, c->spmv_exact_public ? 0 : -1));
    FEDD_HIP(hipMemcpyAsync(y_owned, dy, (size_t)c->n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fedd_spmv_device(fedd_ctx* c, int reps) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_spmv_device: no matrix");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_TRY(c->d_dtmp0.ensure((size_t)c->n_rows * 2));
    double* dx = c->d_dtmp0.p;
    double* dy = dx + c->n_rows;
    FEDD_HIP(hipMemcpyAsync(dx, c->d_rhs.p, (size_t)c->n_rows * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    for (int r = 0; r < reps; ++r) FEDD_TRY(spmv_owned(c, dx, dy));
    return 0;
}

// host-only: the product's reference-element tables, for parity checks against the reference's literals
extern "C" int fedd_fe_quadrature(int dim, int degree, int* nq, double* pts, double* w) {
    FEDD_CHECK(nq, "fedd_fe_quadrature: null output");
    std::vector<double> p, ww;
    FEDD_TRY(fe_quadrature(dim, degree, p, ww));
    *nq = (int)ww.size();
    if (pts) std::copy(p.begin(), p.end(), pts);
    if (w) std::copy(ww.begin(), ww.end(), w);
    return 0;
}

extern "C" int fedd_fe_basis(int dim, int nen, int degree, double* phi, double* dphi) {
    FeTables t;
    FEDD_TRY(fe_tables(dim, nen, degree, t));
    if (phi) std::copy(t.phi.begin(), t.phi.end(), phi);
    if (dphi) std::copy(t.dphi.begin(), t.dphi.end(), dphi);
    return 0;
}

extern "C" int fedd_schwarz_unique(fedd_ctx* c, int64_t* n_unique) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_schwarz && n_unique, "fedd_schwarz_unique: no preconditioner");
    *n_unique = c->sw_big_active ? c->sw_nsub : c->sw_nrep;
    return 0;
}

extern "C" int fedd_schwarz_conforming(fedd_ctx* c, int64_t* n_conforming) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_schwarz && n_conforming, "fedd_schwarz_conforming: no preconditioner");
    *n_conforming = c->sw_big_active ? 0 : c->sw_nconf;
    return 0;
}

extern "C" int fedd_schwarz_sizes(fedd_ctx* c, int64_t* sum_sizes, int64_t* sum_owned) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_schwarz && !c->sw_big_active, "fedd_schwarz_sizes: no preconditioner of the small-subdomain path");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_TRY(c->d_itmp0.ensure((size_t)c->sw_nsub + 1));
    int64_t t = 0;
    if (sum_sizes) {
        FEDD_TRY(exclusive_scan_i32(c, c->d_sub_n.p, c->d_itmp0.p, c->sw_nsub, &t));
        *sum_sizes = t;
    }
    if (sum_owned) {
        FEDD_TRY(exclusive_scan_i32(c, c->d_sub_nown.p, c->d_itmp0.p, c->sw_nsub, &t));
        *sum_owned = t;
    }
    return 0;
}

extern "C" int fedd_spmv_info(fedd_ctx* c, int64_t* nnz_pattern, int64_t* nnz_streamed) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_spmv_info: no matrix");
    if (nnz_pattern) *nnz_pattern = c->nnz;
    if (nnz_streamed) *nnz_streamed = c->cs.valid ? c->cs.nnz : c->nnz;
    return 0;
}

extern "C" int fedd_spmv_patterns(fedd_ctx* c, int64_t* n_patterns, int64_t* n_rows_explicit) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_spmv_patterns: no matrix");
    const bool on = c->cs.has_dictionary();
    if (n_patterns) *n_patterns = on ? c->cs.npat : 0;
    if (n_rows_explicit) *n_rows_explicit = on ? c->cs.nexpl : c->n_rows;
    return 0;
}

extern "C" int fedd_spmv_classes(fedd_ctx* c, int64_t* n_classes, int64_t* n_rows_in_classes, int64_t* nnz_streamed_rest) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_spmv_classes: no matrix");
    const bool on = c->cs.takes(fedd::SpmvStream::CLASSES);
    if (n_classes) *n_classes = on ? c->cs.ncls : 0;
    if (n_rows_in_classes) *n_rows_in_classes = on ? c->cs.cls_rows : 0;
    if (nnz_streamed_rest) *nnz_streamed_rest = on ? c->cs.cls_rest : c->cs.nnz;
    return 0;
}

extern "C" int fedd_spmv_cls_blocks(fedd_ctx* c, int64_t* n_blocks_lds, int64_t* n_blocks_fallback) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_spmv_cls_blocks: no matrix");
    const bool on = c->cs.takes(fedd::SpmvStream::CLASSES);
    if (n_blocks_lds) *n_blocks_lds = on ? c->cs.blk_lds : 0;
    if (n_blocks_fallback) *n_blocks_fallback = on ? c->cs.blk_fallback : 0;
    return 0;
}

extern "C" int fedd_spmv_col_bytes(fedd_ctx* c, int* bytes_per_column_index, int64_t* entries_with_32bit_columns) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern && bytes_per_column_index, "fedd_spmv_col_bytes: no matrix / null output");
    const bool pat = c->cs.has_dictionary(), c16 = c->cs.takes(fedd::SpmvStream::ENTRY16);
    *bytes_per_column_index = pat ? 0 : (c16 ? 2 : 4);
    if (entries_with_32bit_columns) {
        int32_t wide = 0;
        if (c16) {
            FEDD_HIP(hipMemcpyAsync(&wide, c->d_flags.p + 7, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            FEDD_HIP(hipStreamSynchronize(c->stream));
        }
        *entries_with_32bit_columns = pat ? 0 : (c16 ? (int64_t)wide : (c->cs.valid ? c->cs.nnz : c->nnz));
    }
    return 0;
}

extern "C" int fedd_read_bandwidth(fedd_ctx* c, int64_t bytes, int reps, double* gb_per_s) {
    NEED_DEVICE(c);
    FEDD_CHECK(bytes >= (1 << 20) && reps > 0 && gb_per_s, "fedd_read_bandwidth: bytes %lld reps %d", (long long)bytes, reps);
    FEDD_HIP(hipSetDevice(c->device));
    return read_bandwidth(c, bytes, reps, gb_per_s);
}

extern "C" int fedd_schwarz_set_target(fedd_ctx* c, int target_nodes, double scale) {
    FEDD_CHECK(c, "null context");
    FEDD_CHECK(target_nodes >= 0 && scale > 0, "fedd_schwarz_set_target: target %d scale %g", target_nodes, scale);
    c->sw_target = target_nodes;
    c->sw_scale = scale;
    return 0;
}

extern "C" int fedd_schwarz_setup(fedd_ctx* c, int overlap, int combine, int two_level, int coarse_kind) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "fedd_schwarz_setup: assemble the matrix first");
    FEDD_CHECK(c->n_node > 0, "fedd_schwarz_setup: %s (its preconditioner is fedd_fsi_prec_attach)", NO_MESH);
    FEDD_CHECK(overlap >= 0 && overlap <= 4, "fedd_schwarz_setup: overlap %d", overlap);
    FEDD_CHECK(combine >= 0 && combine <= 2, "fedd_schwarz_setup: combine mode %d", combine);
    FEDD_CHECK(two_level == 0 || coarse_kind == FEDD_COARSE_Q1 || coarse_kind == FEDD_COARSE_GDSW || coarse_kind == FEDD_COARSE_RGDSW,
               "fedd_schwarz_setup: coarse_kind %d is not built (FEDD_COARSE_Q1 = %d, FEDD_COARSE_GDSW = %d and FEDD_COARSE_RGDSW = %d are)",
               coarse_kind, FEDD_COARSE_Q1, FEDD_COARSE_GDSW, FEDD_COARSE_RGDSW);
    FEDD_CHECK(two_level == 0 || !c->merged,
               "fedd_schwarz_setup: the coarse level takes node-interleaved systems, not a merged block system");
    FEDD_HIP(hipSetDevice(c->device));
    c->sw_overlap = overlap;
    c->sw_combine = combine;
    c->sw_two_level = two_level ? 1 : 0;
    if (two_level) c->co_kind = coarse_kind;
    ++c->sw_setup_gen;      // (a parent that applies this context as a block orders this stream in front of its own once more)
    return schwarz_setup(c);
}

extern "C" int fedd_schwarz_set_coarse(fedd_ctx* c, double cells_target) {
    FEDD_CHECK(c, "null context");
    FEDD_CHECK(cells_target >= 0 && cells_target < 1e9, "fedd_schwarz_set_coarse: cells_target %g", cells_target);
    c->co_cells_target = cells_target;
    return 0;
}

// FROSch "Level Combination" (parametersPrec.xml:19; the pre-apply of LinearSolver_def.hpp:98-104 is fedd_schwarz_coarse_apply,
// the combination inside every apply of the solve is this setting)
extern "C" int fedd_schwarz_set_level_combination(fedd_ctx* c, int combination) {
    FEDD_CHECK(c, "null context");
    FEDD_CHECK(combination == FEDD_LEVELS_ADDITIVE || combination == FEDD_LEVELS_MULTIPLICATIVE,
               "fedd_schwarz_set_level_combination: %d (FEDD_LEVELS_ADDITIVE = %d, FEDD_LEVELS_MULTIPLICATIVE = %d)", combination,
               FEDD_LEVELS_ADDITIVE, FEDD_LEVELS_MULTIPLICATIVE);
    c->sw_levels = combination;
    return 0;
}

extern "C" int fedd_schwarz_get_level_combination(fedd_ctx* c, int* combination) {
    FEDD_CHECK(c && combination, "fedd_schwarz_get_level_combination: null context / pointer");
    *combination = c->sw_levels;
    return 0;
}

// the multiplicative combination is refused where it is not built, rather than run as the additive one
static int levels_check(const fedd_ctx* c, const char* who) {
    if (c->sw_levels != FEDD_LEVELS_MULTIPLICATIVE) return 0;
    FEDD_CHECK(!c->merged, "%s: the multiplicative level combination is not built for merged block systems", who);
    FEDD_CHECK(!c->sw_big_active, "%s: the multiplicative level combination is not built on the large-subdomain path (schwarz_big)", who);
    FEDD_CHECK(c->have_coarse, "%s: the multiplicative level combination needs a coarse level (fedd_schwarz_setup with two_level = 1)", who);
    return 0;
}

extern "C" int fedd_schwarz_coarse_sizes(fedd_ctx* c, int32_t cells[3], int64_t* n0) {
    FEDD_CHECK(c && c->have_coarse, "fedd_schwarz_coarse_sizes: no coarse level");
    if (cells)
        for (int d = 0; d < 3; ++d) cells[d] = c->co_geom.g[d];
    if (n0) *n0 = c->co_n0;
    return 0;
}

extern "C" int fedd_schwarz_coarse_get(fedd_ctx* c, double* k0_inverse) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_coarse && k0_inverse, "fedd_schwarz_coarse_get: no coarse level / null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipMemcpy2DAsync(k0_inverse, (size_t)c->co_n0 * sizeof(double), c->d_co_K.p, (size_t)c->co_ld * sizeof(double),
                              (size_t)c->co_n0 * sizeof(double), (size_t)c->co_n0, hipMemcpyDeviceToHost, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fedd_schwarz_info(fedd_ctx* c, int64_t* n_sub, int64_t* max_size, int64_t* inverse_bytes) {
    FEDD_CHECK(c && c->have_schwarz, "fedd_schwarz_info: no preconditioner");
    if (n_sub) *n_sub = c->sw_nsub;
    if (max_size) *max_size = c->sw_max_size;
    if (inverse_bytes) *inverse_bytes = c->sw_inv_elems * (int64_t)sizeof(double);
    return 0;
}

extern "C" int fedd_schwarz_reuse_info(fedd_ctx* c, int* last_reused, int64_t* n_reused) {
    FEDD_CHECK(c, "fedd_schwarz_reuse_info: null context");
    if (last_reused) *last_reused = c->have_schwarz ? c->sw_last_reused : 0;
    if (n_reused) *n_reused = c->sw_reuse_count;
    return 0;
}

extern "C" int fedd_pattern_reuse_info(fedd_ctx* c, int* last_reused, int64_t* n_reused) {
    FEDD_CHECK(c, "fedd_pattern_reuse_info: null context");
    if (last_reused) *last_reused = c->have_pattern ? c->pat_last_reused : 0;
    if (n_reused) *n_reused = c->pat_reuse_count;
    return 0;
}

extern "C" int fedd_spmv_reuse_info(fedd_ctx* c, int* last_reused, int64_t* n_reused) {
    FEDD_CHECK(c, "fedd_spmv_reuse_info: null context");
    if (last_reused) *last_reused = c->cs.valid ? c->cs.last_reused : 0;
    if (n_reused) *n_reused = c->cs.reuse_count;
    return 0;
}

extern "C" int fedd_setup_fused_info(fedd_ctx* c, int64_t* n_walks, int64_t* n_checks_used, int64_t* n_absdet_kept) {
    FEDD_CHECK(c, "fedd_setup_fused_info: null context");
    if (n_walks) *n_walks = c->fused_walks;
    if (n_checks_used) *n_checks_used = c->fused_checks_used;
    if (n_absdet_kept) *n_absdet_kept = c->fused_absdet_kept;
    return 0;
}

extern "C" int fedd_schwarz_apply(fedd_ctx* c, const double* r_owned, double* z_owned) {
    NEED_DEVICE(c);
    FEDD_CHECK((c->have_schwarz || has_attached_prec(c)) && r_owned && z_owned, "fedd_schwarz_apply: no preconditioner / null pointer");
    if (has_attached_prec(c)) FEDD_TRY(attached_prec_check(c, "fedd_schwarz_apply"));
    else FEDD_TRY(levels_check(c, "fedd_schwarz_apply"));
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_TRY(c->d_dtmp0.ensure((size_t)c->n_rows * 2));
    double* dr = c->d_dtmp0.p;
    double* dz = dr + c->n_rows;
    FEDD_HIP(hipMemcpyAsync(dr, r_owned, (size_t)c->n_rows * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FEDD_TRY(prec_apply(c, dr, dz, false));
    FEDD_HIP(hipMemcpyAsync(z_owned, dz, (size_t)c->n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fedd_schwarz_apply_device(fedd_ctx* c, int reps) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_schwarz || has_attached_prec(c), "fedd_schwarz_apply_device: no preconditioner");
    if (has_attached_prec(c)) FEDD_TRY(attached_prec_check(c, "fedd_schwarz_apply_device"));
    else FEDD_TRY(levels_check(c, "fedd_schwarz_apply_device"));
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_TRY(c->d_dtmp0.ensure((size_t)c->n_rows * 2));
    double* dr = c->d_dtmp0.p;
    double* dz = dr + c->n_rows;
    FEDD_HIP(hipMemcpyAsync(dr, c->d_rhs.p, (size_t)c->n_rows * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    for (int r = 0; r < reps; ++r) FEDD_TRY(prec_apply(c, dr, dz, false));
    return 0;
}

// x0: "Zero Initial Guess" = false (LinearSolver_def.hpp:76-78): the solve starts from x_owned (NULL: from the vector the
// device holds -- the last solution, or what fedd_schwarz_coarse_apply(ctx, NULL, NULL) left there)
static int gmres_entry(fedd_ctx* c, const char* who, bool x0, const double* b_owned, double* x_owned, double rtol, int max_it,
                       int restart, int use_prec, int* its_out, double* relres_out) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "%s: no matrix", who);
    FEDD_CHECK(!use_prec || has_attached_prec(c) || c->have_schwarz, "%s: preconditioner requested but fedd_schwarz_setup was not called", who);
    FEDD_CHECK(rtol > 0 && max_it >= 1 && restart >= 1 && restart <= 1000, "%s: bad rtol/max_it/restart", who);
    if (use_prec && has_attached_prec(c)) FEDD_TRY(attached_prec_check(c, who));     // (and again at every apply)
    else if (use_prec) FEDD_TRY(levels_check(c, who));
    FEDD_HIP(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->n_rows * sizeof(double);
    if (b_owned) FEDD_HIP(hipMemcpyAsync(c->d_rhs.p, b_owned, bytes, hipMemcpyHostToDevice, c->stream));
    if (x0 && x_owned) FEDD_HIP(hipMemcpyAsync(c->d_x.p, x_owned, bytes, hipMemcpyHostToDevice, c->stream));
    GmresCall call{c->d_rhs.p, c->d_x.p, rtol, max_it, restart, use_prec};
    call.x0 = x0;
    FEDD_TRY(gmres_solve(c, call, its_out, relres_out));
    if (x_owned) {
        FEDD_HIP(hipMemcpyAsync(x_owned, c->d_x.p, bytes, hipMemcpyDeviceToHost, c->stream));
        FEDD_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int fedd_gmres(fedd_ctx* c, const double* b_owned, double* x_owned, double rtol, int max_it,
                          int restart, int use_prec, int* its_out, double* relres_out) {
    return gmres_entry(c, "fedd_gmres", false, b_owned, x_owned, rtol, max_it, restart, use_prec, its_out, relres_out);
}

extern "C" int fedd_gmres_x0(fedd_ctx* c, const double* b_owned, double* x_owned, double rtol, int max_it,
                             int restart, int use_prec, int* its_out, double* relres_out) {
    return gmres_entry(c, "fedd_gmres_x0", true, b_owned, x_owned, rtol, max_it, restart, use_prec, its_out, relres_out);
}

static int cg_entry(fedd_ctx* c, const char* who, bool x0, const double* b_owned, double* x_owned, double rtol, int max_it,
                    int use_prec, int* its_out, double* relres_out) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_pattern, "%s: no matrix", who);
    FEDD_CHECK(rtol > 0 && max_it >= 1, "%s: bad rtol/max_it", who);
    FEDD_CHECK(c->nranks == 1, "%s: a context with more than one rank (summing the overlap contributions across ranks needs an export-add that is not built)", who);
    FEDD_CHECK(!c->merged, "%s: a merged block system is not symmetric positive definite; use fedd_gmres", who);
    if (use_prec) {
        FEDD_CHECK(c->have_schwarz, "%s: preconditioner requested but fedd_schwarz_setup was not called", who);
        FEDD_CHECK(!c->sw_big_active, "%s: the large-subdomain path (schwarz_big) has no symmetric apply", who);
        FEDD_CHECK(c->sw_combine == FEDD_COMBINE_FULL, "%s: preconditioner not symmetric: use FEDD_COMBINE_FULL", who);
        FEDD_CHECK(c->sw_levels != FEDD_LEVELS_MULTIPLICATIVE, "%s: FEDD_LEVELS_MULTIPLICATIVE is not symmetric: use FEDD_LEVELS_ADDITIVE", who);
    }
    FEDD_HIP(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->n_rows * sizeof(double);
    if (b_owned) FEDD_HIP(hipMemcpyAsync(c->d_rhs.p, b_owned, bytes, hipMemcpyHostToDevice, c->stream));
    if (x0 && x_owned) FEDD_HIP(hipMemcpyAsync(c->d_x.p, x_owned, bytes, hipMemcpyHostToDevice, c->stream));
    CgCall call{c->d_rhs.p, c->d_x.p, rtol, max_it, use_prec};
    call.x0 = x0;
    const int rc = cg_solve(c, call, its_out, relres_out);
    if (x_owned) {
        FEDD_HIP(hipMemcpyAsync(x_owned, c->d_x.p, bytes, hipMemcpyDeviceToHost, c->stream));
        FEDD_HIP(hipStreamSynchronize(c->stream));
    }
    return rc;
}

extern "C" int fedd_cg(fedd_ctx* c, const double* b_owned, double* x_owned, double rtol, int max_it, int use_prec, int* its_out,
                       double* relres_out) {
    return cg_entry(c, "fedd_cg", false, b_owned, x_owned, rtol, max_it, use_prec, its_out, relres_out);
}

extern "C" int fedd_cg_x0(fedd_ctx* c, const double* b_owned, double* x_owned, double rtol, int max_it, int use_prec, int* its_out,
                          double* relres_out) {
    return cg_entry(c, "fedd_cg_x0", true, b_owned, x_owned, rtol, max_it, use_prec, its_out, relres_out);
}

extern "C" int fedd_cg_info(fedd_ctx* c, int* replacements, int* breakdown) {
    FEDD_CHECK(c, "fedd_cg_info: null context");
    if (replacements) *replacements = c->cg_replacements;
    if (breakdown) *breakdown = c->cg_breakdown;
    return 0;
}

extern "C" int fedd_schwarz_full_info(fedd_ctx* c, int64_t* n_mfma, int64_t* n_plain) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_schwarz, "fedd_schwarz_full_info: no preconditioner");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_TRY(schwarz_sym_setup(c));
    if (n_mfma) *n_mfma = c->sw_full_nmfma;
    if (n_plain) *n_plain = c->sw_full_nplain;
    return 0;
}

extern "C" int fedd_mesh_setup_info(fedd_ctx* c, double* adjacency_ms, double* tiles_ms, int* tiles_state, int64_t* n_tiles) {
    FEDD_CHECK(c, "fedd_mesh_setup_info: null context");
    if (adjacency_ms) *adjacency_ms = c->have_adj ? c->adj_build_ms : 0.0;
    // (P2 meshes: the gather lists of the row sums take the place of the tile structures)
    if (tiles_ms) *tiles_ms = (c->tl_state != 0 || c->gl_p2.state != 0) ? c->tl_build_ms : 0.0;
    if (tiles_state) *tiles_state = c->tl_state != 0 ? c->tl_state : c->gl_p2.state;
    if (n_tiles) *n_tiles = c->tl_state == 1 ? c->tl_ntile : 0;
    return 0;
}

extern "C" int fedd_gmres_status(fedd_ctx* c, int* floor_reached, double* recurrence_relres) {
    FEDD_CHECK(c, "fedd_gmres_status: null context");
    if (floor_reached) *floor_reached = c->gmres_floor;
    if (recurrence_relres) *recurrence_relres = c->gmres_rec_relres;
    return 0;
}

// FROSch's "Only apply coarse" (LinearSolver_def.hpp:98-104): z = Phi K0^-1 Phi^T r, the second level alone
extern "C" int fedd_schwarz_coarse_apply(fedd_ctx* c, const double* r_owned, double* z_owned) {
    NEED_DEVICE(c);
    FEDD_CHECK(c->have_schwarz && c->sw_two_level && c->have_coarse, "fedd_schwarz_coarse_apply: no coarse level (fedd_schwarz_setup with two_level = 1)");
    FEDD_CHECK((r_owned == nullptr) == (z_owned == nullptr), "fedd_schwarz_coarse_apply: r and z both host pointers or both NULL");
    FEDD_HIP(hipSetDevice(c->device));
    const int64_t nc = std::max(c->n_rows, c->n_cols);
    FEDD_TRY(c->d_dtmp0.ensure((size_t)nc * 2));
    double* dr = c->d_dtmp0.p;
    double* dz = r_owned ? dr + nc : c->d_x.p;
    if (r_owned) FEDD_HIP(hipMemcpyAsync(dr, r_owned, (size_t)c->n_rows * sizeof(double), hipMemcpyHostToDevice, c->stream));
    else FEDD_HIP(hipMemcpyAsync(dr, c->d_rhs.p, (size_t)c->n_rows * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    FEDD_HIP(hipMemsetAsync(dz, 0, (size_t)c->n_rows * sizeof(double), c->stream));
    FEDD_TRY(coarse_apply_add(c, dr, dz));
    if (z_owned) {
        FEDD_HIP(hipMemcpyAsync(z_owned, dz, (size_t)c->n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        FEDD_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int fedd_comm_set_host_callbacks(fedd_ctx* c, fedd_exchange_fn exchange, fedd_allreduce_fn allreduce, void* user) {
    FEDD_CHECK(c, "fedd_comm_set_host_callbacks: null context");
    c->cb_exchange = exchange;
    c->cb_allreduce = allreduce;
    c->cb_user = user;
    return 0;
}

// fedd_set_option: one row per key -- the member it sets, the legal values, and what setting it drops (option_drops)
namespace {
struct Legal {
    // any value | the integers v with bit v of `set` | [lo, hi] | [lo, hi) | (lo, hi) | [lo, inf)
    enum Kind { ANY, ONE_OF, CLOSED, HALF_OPEN, OPEN, AT_LEAST } kind;
    unsigned set;
    double lo, hi;
    const char* text;   // how the error text names them
    bool holds(double v) const {
        switch (kind) {
            case ONE_OF: return v >= 0 && v < 32 && v == (int)v && (set >> (int)v & 1);
            case CLOSED: return v >= lo && v <= hi;
            case HALF_OPEN: return v >= lo && v < hi;
            case OPEN: return v > lo && v < hi;
            case AT_LEAST: return v >= lo;
            default: return true;
        }
    }
};
constexpr Legal any{Legal::ANY, 0, 0, 0, ""};
constexpr Legal one_of(unsigned set, const char* text) { return {Legal::ONE_OF, set, 0, 0, text}; }
constexpr Legal range(Legal::Kind kind, double lo, double hi, const char* text = "") { return {kind, 0, lo, hi, text}; }
constexpr Legal zero_one = one_of(0x3, " (0 or 1)"), upto_two = one_of(0x7, " (one of 0, 1, 2)");
struct Option {
    const char* key;
    int fedd_ctx::*i;       // the member: an int (`flag`: it holds value != 0) ...
    double fedd_ctx::*d;    // ... or a double; neither: the special cases below the lookup set it
    bool flag;
    Legal legal;
    unsigned drops;
};
#define INT(m) &fedd_ctx::m, nullptr, false
#define FLAG(m) &fedd_ctx::m, nullptr, true
#define REAL(m) nullptr, &fedd_ctx::m, false
const Option OPTIONS[] = {
    {"spmv_kind", INT(spmv_kind), any, 0},
    {"box_kind", INT(box_kind), any, 0},
    {"asm_lds_kb", INT(asm_lds_kb), any, 0},     // (at least 2: below)
    {"spmv_nt", INT(spmv_nt), any, 0},
    {"spmv_drop_tol", REAL(spmv_drop_tol), range(Legal::HALF_OPEN, 0.0, 1.0), OPT_DROPS_STREAM},
    {"spmv_compact", INT(spmv_compact), any, OPT_DROPS_STREAM},
    {"spmv_exact_public", INT(spmv_exact_public), any, 0},
    {"spmv_classes", INT(spmv_classes), any, OPT_DROPS_STREAM},
    {"spmv_keep_dictionary", INT(spmv_keep_dict), any, 0},
    {"spmv_classes_cover", INT(spmv_cls_cover), any, OPT_DROPS_STREAM},
    {"spmv_cls_lds", INT(spmv_cls_lds), any, OPT_DROPS_STREAM},
    {"spmv_cls_lds_cap", INT(spmv_cls_lds_cap), any, OPT_DROPS_STREAM},     // (development: 0 = what the kernel's LDS holds)
    {"asm_tiles_host", INT(asm_tiles_host), zero_one, OPT_DROPS_TILES},
    {"asm_p2_elem", INT(asm_p2_elem), upto_two, 0},
    {"asm_zero_eps", REAL(asm_zero_eps), range(Legal::AT_LEAST, 0.0, 0.0), 0},
    {"whole_boxes", INT(whole_boxes), any, 0},
    {"gdsw_tol", REAL(gdsw_tol), range(Legal::HALF_OPEN, 0.0, 1.0, " (0 = by coarse space)"), 0},
    {"schwarz_dedupe", INT(sw_dedupe), any, 0},
    {"schwarz_fp_kind", INT(sw_fp_kind), any, OPT_DROPS_SCHWARZ},
    {"apply_gather", FLAG(apply_gather), any, 0},
    {"apply_full_kind", INT(apply_full_kind), upto_two, 0},
    {"apply_span", INT(apply_span), any, 0},
    {"apply_bt", INT(apply_bt), any, 0},
    {"gdsw_block", FLAG(gdsw_block), any, 0},
    {"gdsw_rotations", FLAG(gdsw_rot), any, 0},
    {"gmres_fuse", INT(gmres_fuse), any, 0},
    {"multi_ch", INT(multi_ch), any, 0},
    {"spmv_col16", FLAG(spmv_col16), any, OPT_DROPS_STREAM},
    {"pat_hash", FLAG(pat_hash), any, OPT_DROPS_REPEAT},
    {"md2_gy", INT(md2_gy), any, 0},
    {"gmres_hostwrite", nullptr, nullptr, true, any, 0},     // (switches h_pinned_dev: below)
    {"spmv_pattern", INT(spmv_pattern), any, OPT_DROPS_STREAM},
    {"spmv_pat_nu", INT(spmv_pat_nu), any, OPT_DROPS_STREAM},
    {"spmv_win_nu", INT(spmv_win_nu), any, OPT_DROPS_STREAM},
    {"halo_overlap", INT(halo_overlap), any, OPT_DROPS_SCHWARZ},
    {"schwarz_big", INT(sw_big), any, 0},
    {"schwarz_big_target", INT(sw_big_target), any, 0},
    // (the dispatches launch_assemble has: 0 = default, 2 = the pair sweep always, 3 = slot-addressed where it fits)
    {"asm_kind", INT(asm_kind), one_of(0xd, " (one of 0, 2, 3)"), 0},
    {"asm_tiles", INT(asm_tiles), zero_one, 0},
    // (the kernel families schwarz_apply has: any other value would be left to whatever its predicates happen to give)
    {"apply_kind", INT(apply_kind), one_of(0x57, " (one of 0, 1, 2, 4, 6)"), 0},
    {"inv_kind", INT(inv_kind), any, 0},
    {"gmres_kind", INT(gmres_kind), one_of(0x7, ""), 0},
    {"gmres_s", INT(gmres_s), range(Legal::CLOSED, 0, 16, " (0 = automatic, 1 ... 16)"), 0},
    {"gmres_spec", INT(gmres_spec), range(Legal::CLOSED, 0, 16), 0},
    {"gmres_tol_blocks", INT(gmres_tol_blocks), any, 0},
    {"gmres_dot_gy", INT(gmres_dot_gy), range(Legal::CLOSED, 0, 8), 0},
    {"gmres_dot_own", INT(gmres_dot_own), zero_one, 0},
    {"gmres_newton", INT(gmres_newton), any, 0},
    {"gmres_chol_tol", REAL(gmres_chol_tol), range(Legal::OPEN, 0.0, 1.0), 0},
    {"ghost_overlap", INT(ghost_overlap), any, 0},
    {"schwarz_reuse", FLAG(sw_reuse), any, 0},
    {"pattern_reuse", FLAG(pat_reuse), any, 0},
    {"spmv_reuse", FLAG(spmv_reuse), any, 0},
    // (drops the stream check a Schwarz setup may have left for the next SpMV: switched off, that SpMV makes its own)
    {"setup_fused", FLAG(setup_fused), any, OPT_DROPS_FUSED},
};
#undef INT
#undef FLAG
#undef REAL
}  // namespace

extern "C" int fedd_set_option(fedd_ctx* c, const char* key, double value) {
    FEDD_CHECK(c && key, "fedd_set_option: null");
    const std::string k(key);
    const Option* o = std::find_if(std::begin(OPTIONS), std::end(OPTIONS), [&](const Option& e) { return k == e.key; });
    FEDD_CHECK(o != std::end(OPTIONS), "fedd_set_option: unknown key '%s'", key);
    FEDD_CHECK(o->legal.holds(value), "fedd_set_option: %s %g%s", key, value, o->legal.text);
    if (o->d) c->*(o->d) = value;
    else if (o->i) c->*(o->i) = o->flag ? value != 0.0 : (int)value;
    if (k == "asm_lds_kb") c->asm_lds_kb = std::max(2, c->asm_lds_kb);
    if (k == "gmres_hostwrite") c->h_pinned_dev = value != 0 ? c->h_pinned_map : nullptr;
    option_drops(c, o->drops);
    return 0;
}

extern "C" int fedd_timing_enable(fedd_ctx* c, int on) {
    NEED_DEVICE(c);
    FEDD_CHECK(on >= 0 && on <= 1024, "fedd_timing_enable: %d", on);
    c->timing = on != 0;
    c->timing_stride = on > 1 ? on : 1;
    // the events of the timed launches, created here rather than inside the region the caller is about to time
    // (ScopedTimer::take falls back to creating one when the pool runs dry)
    if (on) {
        (void)hipSetDevice(c->device);
        while (c->ev_pool.size() < 4096) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) break;
            c->ev_pool.push_back(e);
        }
    }
    return 0;
}

extern "C" int fedd_timing_reset(fedd_ctx* c) {
    NEED_DEVICE(c);
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_TRY(timing_flush(c));
    for (int t = 0; t < FEDD_T_COUNT; ++t) {
        c->timers[t].total_ms = 0;
        c->timers[t].launches = 0;
        c->timers[t].seen = 0;
        c->timers[t].bytes = 0;
    }
    return 0;
}

extern "C" int fedd_timing_get(fedd_ctx* c, int timer, double* total_ms, int64_t* launches) {
    NEED_DEVICE(c);
    FEDD_CHECK(timer >= 0 && timer < FEDD_T_COUNT, "fedd_timing_get: timer %d", timer);
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_TRY(timing_flush(c));
    // sampled classes: the total is the sampled average times the number of launches seen
    const auto& s = c->timers[timer];
    if (total_ms) *total_ms = s.launches > 0 ? s.total_ms * (double)s.seen / (double)s.launches : 0.0;
    if (launches) *launches = s.seen;
    return 0;
}

extern "C" int fedd_timing_get_sampled(fedd_ctx* c, int timer, double* sampled_ms, int64_t* sampled_launches, double* sampled_bytes) {
    NEED_DEVICE(c);
    FEDD_CHECK(timer >= 0 && timer < FEDD_T_COUNT, "fedd_timing_get_sampled: timer %d", timer);
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_TRY(timing_flush(c));
    const auto& s = c->timers[timer];
    if (sampled_ms) *sampled_ms = s.total_ms;
    if (sampled_launches) *sampled_launches = s.launches;
    if (sampled_bytes) *sampled_bytes = s.bytes;
    return 0;
}

extern "C" int fedd_gmres_info(fedd_ctx* c, int* kind, int* s, int* blocks, int* cut_blocks) {
    FEDD_CHECK(c, "fedd_gmres_info: null context");
    if (kind) *kind = c->gmres_kind;
    if (s) *s = c->gmres_s > 0 ? c->gmres_s : c->gmres_s_used;
    if (blocks) *blocks = c->gmres_blocks;
    if (cut_blocks) *cut_blocks = c->gmres_cut_blocks;
    return 0;
}

extern "C" int fedd_gmres_fused_blocks(fedd_ctx* c, int* blocks) {
    FEDD_CHECK(c && blocks, "fedd_gmres_fused_blocks: null argument");
    *blocks = c->gmres_fused_blocks;
    return 0;
}

extern "C" int fedd_gmres_capture_arm(fedd_ctx* c, int block) {
    FEDD_CHECK(c, "fedd_gmres_capture_arm: null context");
    return fedd::gmres_capture_arm(c, block);
}

extern "C" int fedd_gmres_capture_info(fedd_ctx* c, int64_t* out) {
    FEDD_CHECK(c && out, "fedd_gmres_capture_info: null argument");
    const fedd::GmresCapture& g = c->gm_cap;
    const int64_t v[8] = {g.captured ? 1 : 0, g.n, g.ldv, g.k, g.sa_req, g.S, g.m, g.fused};
    std::copy(v, v + 8, out);
    return 0;
}

extern "C" int fedd_gmres_capture_get(fedd_ctx* c, const char* what, double* out, int64_t cap) {
    FEDD_CHECK(c && what && out, "fedd_gmres_capture_get: null argument");
    return fedd::gmres_capture_get(c, what, out, cap);
}

extern "C" int fedd_halo_plan_sizes(fedd_ctx* c, int* n_peers, int64_t* n_send_total, int64_t* n_recv_total) {
    FEDD_CHECK(c, "null context");
    if (n_peers) *n_peers = (int)c->halo.peers.size();
    if (n_send_total) *n_send_total = (int64_t)c->halo.send_lid.size();
    if (n_recv_total) *n_recv_total = (int64_t)c->halo.recv_lid.size();
    return 0;
}

extern "C" int fedd_halo_plan_get(fedd_ctx* c, int32_t* peers, int64_t* send_ptr, int32_t* send_lid,
                                  int64_t* recv_ptr, int32_t* recv_lid) {
    FEDD_CHECK(c, "null context");
    const auto& h = c->halo;
    if (peers) std::copy(h.peers.begin(), h.peers.end(), peers);
    if (send_ptr) std::copy(h.send_ptr.begin(), h.send_ptr.end(), send_ptr);
    if (send_lid) std::copy(h.send_lid.begin(), h.send_lid.end(), send_lid);
    if (recv_ptr) std::copy(h.recv_ptr.begin(), h.recv_ptr.end(), recv_ptr);
    if (recv_lid) std::copy(h.recv_lid.begin(), h.recv_lid.end(), recv_lid);
    return 0;
}
