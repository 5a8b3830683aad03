// FSI coupling on the device, one rank, geometry-explicit (four blocks): the matched interface of a fluid and a structure
// context, the coupled system, the FaCSI preconditioner.  gfx950 only.
//
// Replaces MeshInterface::determineInterfaceParallelAndDistance (feddlib/core/Mesh/MeshInterface_def.hpp: std::sort of the
// interface points of each side, pairing by position), FE::assemblyFSICoupling / FE::assemblyDummyCoupling as FSI::assemble
// places them in the block system (feddlib/problems/specific/FSI_def.hpp:223-318), FSI::addInterfaceBlockRHS,
// Preconditioner::buildPreconditionerFaCSI (Preconditioner_def.hpp:789-971) and the geometry-explicit branch of
// PrecOpFaCSI::applyImpl (PrecOpFaCSI_def.hpp:367-589).  The normative statements are in include/fedd_hip.h.
//
//   k_iface_rank     the matcher: rank_i = #{ j : p_j <lex p_i } by counting.  One lane per interface node, its coordinates in
//                    registers; the other points staged through LDS in tiles of IM_TILE, structure-of-arrays, in the shape of
//                    k_interface_distance: in the pair loop every lane of a wave reads the same LDS address (a broadcast).
//                    Exact double comparisons, no sort key; a lane that meets an equal point reports the smallest such index.
//                    Cost: n^2 (2 dim - 1) comparisons for n interface nodes of one side and one flag, n / 256 workgroups that
//                    each read the n points once (from L2 after the first): quadratic in the interface only.
//   k_iface_scatter  table[offset + rank_i] = node id of point i.
//   k_fsi_count / k_fsi_fill   the coupled CSR over the n_f + n_s + n_l rows, count -> scan -> fill in the style of k_merge_*
//                    (blocks.hip); the fill with PATTERN = false moves values only.  k_fsi_check compares the counts with a
//                    pattern in place (the Dirichlet marks of the children decide whether a row has its C1^T / C3^T entry).
//   k_facsi_inject   t = [x_u; x_p] with t[fdof(k)] = x_l,k - c2 * y_d[sdof(k)]: g and the injection, one lane per fluid dof
//                    through the dof -> lambda map, so no two lanes write the same entry.
//   k_facsi_rows     z and y_l: the lane-group row walk of stored_rows.hpp per interface row over cpl's CSR, columns < n_f only,
//                    with two sums, over F (columns < n_u) and over B^T (columns in [n_u, n_f)), one fixed tree per sum.
//                    Bytes of an apply beside the children's: inject 8 (2 n_f) + 4 n_f + 20 n_l; rows 12 nnz(rows fdof(k) of
//                    cpl) + 8 n_l (row pointers) + 4 n_l + 24 n_l -- n_l rows of F and B^T, not the whole blocks.
#include "stored_rows.hpp"
#include <algorithm>
#include <atomic>
#include <cmath>

#pragma clang fp contract(off)

namespace fedd {
namespace {

constexpr int IM_BS = 256;
constexpr int IM_TILE = 1024;       // interface points per LDS tile (fedd_interface_match_info reports it)

// pts: structure-of-arrays, coordinate k of point j at pts[k * np + j].  dup[0] (initialised to INT32_MAX) receives the
// smallest index of a point that has an equal partner.
template <int DIM>
__global__ __launch_bounds__(IM_BS) void k_iface_rank(const double* __restrict__ pts, int32_t np, int32_t* __restrict__ rank,
                                                      int32_t* __restrict__ dup) {
    __shared__ double s_p[DIM][IM_TILE];
    const int32_t i = (int32_t)blockIdx.x * IM_BS + (int32_t)threadIdx.x;
    const bool on = i < np;
    double x[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) x[k] = on ? pts[(int64_t)k * np + i] : 0.0;
    int32_t r = 0;
    bool twin = false;
    for (int32_t t0 = 0; t0 < np; t0 += IM_TILE) {      // (np is uniform over the grid: so are the barriers)
        const int n = np - t0 < IM_TILE ? (int)(np - t0) : IM_TILE;
        for (int j = threadIdx.x; j < n; j += IM_BS)
#pragma unroll
            for (int k = 0; k < DIM; ++k) s_p[k][j] = pts[(int64_t)k * np + t0 + j];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            bool less = false, same = true;     // p_j <lex x: the first coordinate that differs decides
#pragma unroll
            for (int k = 0; k < DIM; ++k) {
                const double q = s_p[k][j];
                less = less || (same && q < x[k]);
                same = same && q == x[k];
            }
            r += less ? 1 : 0;
            twin = twin || (same && t0 + j != i);
        }
        __syncthreads();        // the next tile overwrites s_p
    }
    if (on) {
        rank[i] = r;            // 0 <= r < np
        if (twin) atomicMin(dup, i);
    }
}

__global__ __launch_bounds__(256) void k_iface_scatter(const int32_t* __restrict__ rank, const int32_t* __restrict__ ids, int32_t np,
                                                       int32_t* __restrict__ table) {
    const int32_t i = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;
    if (i < np) table[rank[i]] = ids[i];
}

__global__ __launch_bounds__(256) void k_fsi_lam(const int32_t* __restrict__ dof, int32_t n_l, int32_t* __restrict__ lam) {
    const int32_t k = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;
    if (k < n_l && dof[k] >= 0) lam[dof[k]] = k;
}

struct FsiView {
    const int32_t *rp_f, *ci_f, *dir_f;     // fluid: its merged system and Dirichlet marks
    const double* v_f;
    const int32_t *rp_s, *ci_s, *dir_s;     // structure
    const double* v_s;
    const int32_t *lam_f, *lam_s;           // lambda-dof of a fluid / structure dof (-1: none)
    const int32_t *fdof, *sdof;             // fluid / structure dof of a lambda-dof (-1: uncoupled)
    int32_t n_f, n_s, n_l;
};

__device__ inline int32_t fsi_row_count(const FsiView& V, int32_t r) {
    if (r < V.n_f) return V.rp_f[r + 1] - V.rp_f[r] + ((V.lam_f[r] >= 0 && V.dir_f[r] == 0) ? 1 : 0);
    if (r < V.n_f + V.n_s) {
        const int32_t i = r - V.n_f;
        return V.rp_s[i + 1] - V.rp_s[i] + ((V.lam_s[i] >= 0 && V.dir_s[i] == 0) ? 1 : 0);
    }
    return V.fdof[r - V.n_f - V.n_s] >= 0 ? 2 : 1;
}

__global__ void k_fsi_count(FsiView V, int32_t* __restrict__ cnt) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < V.n_f + V.n_s + V.n_l) cnt[r] = fsi_row_count(V, r);
}

// flag[0] |= 1 where the pattern in place has another row length than this merge would give
__global__ void k_fsi_check(FsiView V, const int32_t* __restrict__ rowptr, int32_t* __restrict__ flag) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < V.n_f + V.n_s + V.n_l && fsi_row_count(V, r) != rowptr[r + 1] - rowptr[r]) atomicOr(flag, 1);
}

// c2 = -(1.0 / dt).  Columns ascending: a child's own columns, then the lambda column; in a lambda row fdof < n_f <= n_f + sdof.
template <bool PATTERN>
__global__ void k_fsi_fill(FsiView V, double c2, const int32_t* __restrict__ rowptr, int32_t* __restrict__ colind,
                           double* __restrict__ val) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= V.n_f + V.n_s + V.n_l) return;
    int32_t p = rowptr[r];
    const int32_t off_l = V.n_f + V.n_s;
    if (r < off_l) {
        const bool fl = r < V.n_f;
        const int32_t i = fl ? r : r - V.n_f;
        const int32_t* rp = fl ? V.rp_f : V.rp_s;
        const int32_t* ci = fl ? V.ci_f : V.ci_s;
        const double* v = fl ? V.v_f : V.v_s;
        const int32_t shift = fl ? 0 : V.n_f;
        for (int32_t q = rp[i]; q < rp[i + 1]; ++q, ++p) {
            if (PATTERN) colind[p] = ci[q] + shift;
            val[p] = v[q];
        }
        const int32_t k = fl ? V.lam_f[i] : V.lam_s[i];
        const int32_t dir = fl ? V.dir_f[i] : V.dir_s[i];
        if (k >= 0 && dir == 0) {       // C1^T: +1, C3^T: -1; none on a Dirichlet row
            if (PATTERN) colind[p] = off_l + k;
            val[p] = fl ? 1.0 : -1.0;
        }
        return;
    }
    const int32_t k = r - off_l;
    const int32_t fd = V.fdof[k];
    if (fd >= 0) {                      // C1: +1, C2: -(1 / dt)
        if (PATTERN) {
            colind[p] = fd;
            colind[p + 1] = V.n_f + V.sdof[k];
        }
        val[p] = 1.0;
        val[p + 1] = c2;
    } else {                            // the dummy diagonal of an uncoupled dof
        if (PATTERN) colind[p] = r;
        val[p] = 1.0;
    }
}

__global__ __launch_bounds__(256) void k_fsi_rhs(const int32_t* __restrict__ sdof, int32_t n_l, double c2,
                                                 const double* __restrict__ d_old, double* __restrict__ rhs_l) {
    const int32_t k = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;
    if (k < n_l) rhs_l[k] = sdof[k] >= 0 ? c2 * d_old[sdof[k]] : 0.0;
}

// x = [x_u; x_p; x_d; x_l] of the coupled system, y_d = S~(x_d).  t[i] = x[i], and on the fluid dof of a coupled lambda-dof k
//   t[fdof(k)] = x_l,k - c2 * y_d[sdof(k)]         (the product rounded, then the difference)
__global__ __launch_bounds__(256) void k_facsi_inject(const double* __restrict__ x, const double* __restrict__ y_d,
                                                      const int32_t* __restrict__ lam_f, const int32_t* __restrict__ sdof, int32_t n_f,
                                                      int32_t off_l, double c2, double* __restrict__ t) {
    const int32_t i = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;
    if (i >= n_f) return;
    const int32_t k = lam_f[i];
    if (k >= 0) {
        const double prod = c2 * y_d[sdof[k]];
        t[i] = x[off_l + k] - prod;
    } else {
        t[i] = x[i];
    }
}

// the two sums of a fluid row of cpl: the C1^T entry of the row lies behind n_f and is dropped
struct FacsiSums {
    const double* __restrict__ y;
    int32_t n_u, n_f;
    double sF = 0.0, sB = 0.0;
    __device__ bool keep(int32_t col) const { return col < n_f; }
    __device__ double x(int32_t col) const { return y[col]; }
    __device__ void add(int32_t col, double p) {
        if (col >= 0 && col < n_u) sF += p;
        if (col >= n_u) sB += p;
    }
    template <int G>
    __device__ void fold(int o) {
        sF += __shfl_xor(sF, o, G);
        sB += __shfl_xor(sB, o, G);
    }
};

// G lanes per lambda-dof k.  y = [y_u; y_p] (the first n_f entries of the output vector), x as above.
//   sF = sum over the columns < n_u of row fdof(k), sB = sum over the columns in [n_u, n_f)      (cpl's CSR, as it stands)
//   y_l,k = (x_u[fdof(k)] - sB) - sF        coupled;      y_l,k = x_l,k        uncoupled
template <int G>
__global__ __launch_bounds__(256) void k_facsi_rows(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                    const double* __restrict__ val, const int32_t* __restrict__ fdof,
                                                    const double* __restrict__ x, const double* __restrict__ y, int32_t n_u,
                                                    int32_t n_f, int32_t off_l, int32_t n_l, double* __restrict__ y_l) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t k = (int32_t)(tid / G);
    const int g = (int)(tid % G);
    const bool live = k < n_l;
    const int32_t r = live ? fdof[k] : -1;
    const int32_t st = r >= 0 ? rowptr[r] : 0;
    const int32_t len = r >= 0 ? rowptr[r + 1] - st : 0;
    FacsiSums sums{y, n_u, n_f};
    row_walk<G>(colind, val, st, len, g, sums);
    const double sF = sums.sF, sB = sums.sB;
    if (live && g == 0) {
        if (r >= 0) {
            const double a = x[r] - sB;
            y_l[k] = a - sF;
        } else {
            y_l[k] = x[off_l + k];
        }
    }
}

std::atomic<uint64_t> g_table_id{0};

struct Side {
    std::vector<int32_t> flag;      // [n_own]
    std::vector<double> xyz;        // [n_node * dim], the reference coordinates
};

int side_read(fedd_ctx* c, Side& s) {
    s.flag.resize((size_t)c->n_own);
    s.xyz.resize((size_t)c->n_node * c->dim);
    FEDD_HIP(hipStreamSynchronize(c->stream));
    if (c->n_own > 0) FEDD_HIP(hipMemcpy(s.flag.data(), c->d_flag.p, s.flag.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    const double* ref = c->have_xref ? c->d_xyz_ref.p : c->d_xyz.p;   // what the last fedd_mesh_set* uploaded
    FEDD_HIP(hipMemcpy(s.xyz.data(), ref, s.xyz.size() * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// the nodes of one side that carry `flag`, ranked on the device and scattered into table[0, ids.size())
int side_rank(fedd_ctx* run, const char* name, int flag, int dim, const Side& s, const std::vector<int32_t>& ids, DevBuf<double>& d_pts,
              DevBuf<int32_t>& d_ids, DevBuf<int32_t>& d_rank, int32_t* d_dup, int32_t* table) {
    const int32_t np = (int32_t)ids.size();
    std::vector<double> pts((size_t)np * dim);
    for (int32_t j = 0; j < np; ++j)
        for (int k = 0; k < dim; ++k) {
            const double v = s.xyz[(size_t)ids[(size_t)j] * dim + k];
            FEDD_CHECK(std::isfinite(v), "fedd_interface_match: %s node %d (flag %d) has a coordinate that is not finite", name,
                       ids[(size_t)j], flag);
            pts[(size_t)k * np + j] = v;
        }
    hipStream_t st = run->stream;
    FEDD_TRY(d_pts.ensure(pts.size()));
    FEDD_TRY(d_ids.ensure((size_t)np));
    FEDD_TRY(d_rank.ensure((size_t)np));
    const int32_t none = INT32_MAX;
    FEDD_HIP(hipMemcpyAsync(d_pts.p, pts.data(), pts.size() * sizeof(double), hipMemcpyHostToDevice, st));
    FEDD_HIP(hipMemcpyAsync(d_ids.p, ids.data(), (size_t)np * sizeof(int32_t), hipMemcpyHostToDevice, st));
    FEDD_HIP(hipMemcpyAsync(d_dup, &none, sizeof(int32_t), hipMemcpyHostToDevice, st));
    {
        ScopedTimer t(run, FEDD_T_FSI_MATCH);
        // the points once per workgroup (from L2 after the first), one rank and one table entry per node
        t.bytes((double)np * dim * 8.0 + (double)np * 12.0);
        const unsigned grid = (unsigned)((np + IM_BS - 1) / IM_BS);
        if (dim == 3)
            hipLaunchKernelGGL(k_iface_rank<3>, dim3(grid), dim3(IM_BS), 0, st, (const double*)d_pts.p, np, d_rank.p, d_dup);
        else
            hipLaunchKernelGGL(k_iface_rank<2>, dim3(grid), dim3(IM_BS), 0, st, (const double*)d_pts.p, np, d_rank.p, d_dup);
        hipLaunchKernelGGL(k_iface_scatter, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, (const int32_t*)d_rank.p,
                           (const int32_t*)d_ids.p, np, table);
    }
    FEDD_HIP(hipGetLastError());
    int32_t dup = none;
    FEDD_HIP(hipMemcpyAsync(&dup, d_dup, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FEDD_HIP(hipStreamSynchronize(st));     // (`pts`, `none` and `dup` are locals)
    if (dup != none) {
        int32_t other = -1;
        for (int32_t j = 0; j < np && other < 0; ++j) {
            bool same = j != dup;
            for (int k = 0; k < dim && same; ++k) same = pts[(size_t)k * np + j] == pts[(size_t)k * np + dup];
            if (same) other = j;
        }
        set_error("fedd_interface_match: %s nodes %d and %d (flag %d) have identical coordinates: the order of the interface is "
                  "not defined",
                  name, ids[(size_t)std::min(dup, other < 0 ? dup : other)], ids[(size_t)std::max(dup, other)], flag);
        return 1;
    }
    return 0;
}

// (the checks in the order of the messages: a fedd_mesh_set* on a child says more than its sizes)
int child_check(fedd_ctx* c, int which, int64_t n_expected, uint64_t uid, uint64_t mesh_gen, const char* who) {
    const fedd_ctx* ch = c->prec.child[which].ctx;
    const char* nm = which == 0 ? "fluid" : "structure";
    FEDD_TRY(child_check_context(c, ch, who, "FaCSI", nm, "coupled context"));
    FEDD_CHECK(ch->uid == uid, "%s: FaCSI: the %s child is not the %s context the coupled system was merged from", who, nm, nm);
    FEDD_CHECK(ch->mesh_gen == mesh_gen,
               "%s: FaCSI: the merge is older than the %s child's mesh (fedd_mesh_set since the last fedd_fsi_merge)", who, nm);
    FEDD_CHECK(ch->have_pattern && ch->n_rows == n_expected && ch->n_cols == n_expected,
               "%s: FaCSI: wrong sizes: the %s child's system has %lld rows, the coupled system's block %lld", who, nm,
               (long long)(ch->have_pattern ? ch->n_rows : 0), (long long)n_expected);
    return child_check_schwarz(ch, who, "FaCSI", nm, "");
}

}  // namespace

void iface_release(fedd_ctx* c) {
    if (c->iface) c->iface->valid = false;      // the other side and a coupled context see it
    c->iface.reset();
}

int fsi_prec_check(fedd_ctx* c, const char* who) {
    FEDD_CHECK(c->prec.kind == AttachedPrec::FACSI && c->prec.child[0].ctx && c->prec.child[1].ctx, "%s: no FaCSI preconditioner attached", who);
    FEDD_CHECK(c->nranks == 1, "%s: FaCSI: one rank only (a context with %d ranks was given)", who, c->nranks);
    FEDD_CHECK(c->have_pattern && c->fsi_coupled && c->pattern_gen == c->fsi_pat_gen,
               "%s: FaCSI: the context does not hold a coupled system (fedd_fsi_merge first)", who);
    // (the children first: a fedd_mesh_set* on a child also releases the table, and the message that names the child and its
    // mesh says more than the one about the table, which is left for a table released by a new fedd_interface_match)
    FEDD_TRY(child_check(c, 0, c->fsi_nu + c->fsi_np, c->fsi_uid_f, c->fsi_mesh_gen_f, who));
    FEDD_TRY(child_check(c, 1, c->fsi_ns, c->fsi_uid_s, c->fsi_mesh_gen_s, who));
    FEDD_CHECK(c->fsi_table && c->fsi_table->valid,
               "%s: FaCSI: the matched interface the coupled system was built on has been released (a new fedd_interface_match of a "
               "child since the last fedd_fsi_merge)",
               who);
    const fedd_ctx* F = c->prec.child[0].ctx;
    FEDD_CHECK(F->merged && F->merged_nA == c->fsi_nu,
               "%s: FaCSI: wrong sizes: the fluid child's velocity block has %lld rows, the coupled system's %lld", who,
               (long long)(F->merged ? F->merged_nA : 0), (long long)c->fsi_nu);
    return 0;
}

int fsi_prec_apply(fedd_ctx* c, const double* x, double* y) {
    FEDD_TRY(fsi_prec_check(c, "FaCSI apply"));
    fedd_ctx *F = c->prec.child[0].ctx, *S = c->prec.child[1].ctx;
    const int32_t n_u = (int32_t)c->fsi_nu, n_f = (int32_t)(c->fsi_nu + c->fsi_np), n_s = (int32_t)c->fsi_ns, n_l = (int32_t)c->fsi_nl;
    const int32_t off_l = n_f + n_s;
    const double c2 = -(1.0 / c->fsi_dt);
    FEDD_TRY(child_order(c, c->prec.child[0]));
    FEDD_TRY(child_order(c, c->prec.child[1]));
    ++c->prec.applies;
    FEDD_TRY(c->d_fp_t.ensure((size_t)n_f));
    double* t = c->d_fp_t.p;
    FEDD_TRY(child_apply(c, S, x + n_f, y + n_f));          // y_d = S~(x_d)
    {
        ScopedTimer tm(c, FEDD_T_FSI_APPLY);
        tm.bytes(16.0 * (double)n_f + 4.0 * (double)n_f + 20.0 * (double)n_l);
        hipLaunchKernelGGL(k_facsi_inject, dim3((unsigned)((n_f + 255) / 256)), dim3(256), 0, c->stream, x, (const double*)(y + n_f),
                           (const int32_t*)c->d_fsi_lam_f.p, (const int32_t*)c->d_fsi_sdof.p, n_f, off_l, c2, t);
        tm.stop();
        FEDD_HIP(hipGetLastError());
    }
    FEDD_TRY(child_apply(c, F, t, y));                      // [y_u; y_p] = F~(t)
    {
        ScopedTimer tm(c, FEDD_T_FSI_APPLY);
        tm.bytes(12.0 * (double)c->max_row_nnz * (double)n_l + 36.0 * (double)n_l);    // (an upper bound: the longest row for every one)
        with_row_groups(c->max_row_nnz, n_l, [&](auto G, unsigned grid) {
            hipLaunchKernelGGL(k_facsi_rows<decltype(G)::value>, dim3(grid), dim3(256), 0, c->stream, (const int32_t*)c->d_rowptr.p,
                               (const int32_t*)c->d_colind.p, (const double*)c->d_val.p, (const int32_t*)c->d_fsi_fdof.p, x,
                               (const double*)y, n_u, n_f, off_l, n_l, y + off_l);
            return 0;
        });
        tm.stop();
        FEDD_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace fedd

using namespace fedd;

static const char* const NEEDS_GPU = "needs a GPU context (fedd_ctx_create with device >= 0); there is no CPU fallback";

extern "C" int fedd_interface_match(fedd_ctx* fluid, fedd_ctx* structure, int n_flags, const int32_t* flags) {
    FEDD_CHECK(fluid && structure, "fedd_interface_match: null context");
    FEDD_CHECK(fluid != structure, "fedd_interface_match: fluid and structure are the same context");
    FEDD_CHECK(n_flags >= 1 && flags, "fedd_interface_match: no flags given (n_flags = %d): an empty interface", n_flags);
    FEDD_CHECK(fluid->nranks == 1 && structure->nranks == 1, "fedd_interface_match: one rank only (contexts with %d and %d ranks were given)",
               fluid->nranks, structure->nranks);
    FEDD_CHECK(fluid->device >= 0 && structure->device >= 0, "fedd_interface_match: this call %s (%s is host-only)", NEEDS_GPU,
               fluid->device < 0 ? "the fluid" : "the structure");
    FEDD_CHECK(fluid->device == structure->device, "fedd_interface_match: contexts on different devices (%d and %d)", fluid->device,
               structure->device);
    FEDD_CHECK(fluid->n_node > 0 && structure->n_node > 0, "fedd_interface_match: %s carries no mesh (fedd_mesh_set first)",
               fluid->n_node > 0 ? "the structure" : "the fluid");
    FEDD_CHECK(fluid->dim == structure->dim, "fedd_interface_match: meshes of different dimension (%d and %d)", fluid->dim, structure->dim);
    FEDD_HIP(hipSetDevice(fluid->device));
    const int dim = fluid->dim;
    iface_release(fluid);       // an earlier match of either side ends here
    iface_release(structure);
    Side sf, ss;
    FEDD_TRY(side_read(fluid, sf));
    FEDD_TRY(side_read(structure, ss));
    auto tab = std::make_shared<IfaceTable>();
    tab->device = fluid->device;
    tab->dim = dim;
    tab->uid_f = fluid->uid;
    tab->uid_s = structure->uid;
    tab->id = ++g_table_id;
    tab->flags.assign(flags, flags + n_flags);
    tab->flag_ptr.assign(1, 0);
    std::vector<std::vector<int32_t>> idf((size_t)n_flags), ids((size_t)n_flags);
    int64_t total = 0;
    for (int q = 0; q < n_flags; ++q) {
        for (int64_t i = 0; i < fluid->n_own; ++i)
            if (sf.flag[(size_t)i] == flags[q]) idf[(size_t)q].push_back((int32_t)i);
        for (int64_t i = 0; i < structure->n_own; ++i)
            if (ss.flag[(size_t)i] == flags[q]) ids[(size_t)q].push_back((int32_t)i);
        FEDD_CHECK(idf[(size_t)q].size() == ids[(size_t)q].size(),
                   "fedd_interface_match: interface has different number of nodes in fluid and structure: flag %d has %lld fluid "
                   "and %lld structure nodes",
                   flags[q], (long long)idf[(size_t)q].size(), (long long)ids[(size_t)q].size());
        total += (int64_t)idf[(size_t)q].size();
        tab->flag_ptr.push_back(total);
    }
    FEDD_CHECK(total > 0, "fedd_interface_match: an empty interface: no node of either context carries one of the %d flags", n_flags);
    tab->n = total;
    // the tables are scattered on the device and read back; what is kept are the host copies (fedd_interface_match_get, and
    // fedd_fsi_merge, which derives its dof maps from them and uploads those): no kernel reads the tables themselves
    DevBuf<double> d_pts;
    DevBuf<int32_t> d_ids, d_rank, d_tab_f, d_tab_s;
    FEDD_TRY(d_tab_f.ensure((size_t)total));
    FEDD_TRY(d_tab_s.ensure((size_t)total));
    FEDD_TRY(fluid->d_flags.ensure(16));
    int32_t* d_dup = fluid->d_flags.p + 14;
    for (int q = 0; q < n_flags; ++q) {
        if (idf[(size_t)q].empty()) continue;
        const int64_t off = tab->flag_ptr[(size_t)q];
        FEDD_TRY(side_rank(fluid, "fluid", flags[q], dim, sf, idf[(size_t)q], d_pts, d_ids, d_rank, d_dup, d_tab_f.p + off));
        FEDD_TRY(side_rank(fluid, "structure", flags[q], dim, ss, ids[(size_t)q], d_pts, d_ids, d_rank, d_dup, d_tab_s.p + off));
    }
    tab->h_f.resize((size_t)total);
    tab->h_s.resize((size_t)total);
    FEDD_HIP(hipMemcpy(tab->h_f.data(), d_tab_f.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
    FEDD_HIP(hipMemcpy(tab->h_s.data(), d_tab_s.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
    double m2 = 0.0;
    for (int64_t k = 0; k < total; ++k) {
        double d2 = 0.0;
        for (int a = 0; a < dim; ++a) {
            const double t = sf.xyz[(size_t)tab->h_f[(size_t)k] * dim + a] - ss.xyz[(size_t)tab->h_s[(size_t)k] * dim + a];
            d2 += t * t;
        }
        m2 = std::max(m2, d2);
    }
    tab->max_dist = std::sqrt(m2);
    fluid->iface = tab;
    structure->iface = tab;
    return 0;
}

extern "C" int fedd_interface_match_sizes(fedd_ctx* c, int64_t* n_pairs, int* n_flags, int* dofs_per_node) {
    FEDD_CHECK(c, "fedd_interface_match_sizes: null context");
    FEDD_CHECK(c->iface && c->iface->valid, "fedd_interface_match_sizes: no matched interface (fedd_interface_match first; fedd_mesh_set releases it)");
    if (n_pairs) *n_pairs = c->iface->n;
    if (n_flags) *n_flags = (int)c->iface->flags.size();
    if (dofs_per_node) *dofs_per_node = c->iface->dim;
    return 0;
}

extern "C" int fedd_interface_match_get(fedd_ctx* c, int32_t* iface_fluid, int32_t* iface_structure, int64_t* flag_ptr) {
    FEDD_CHECK(c, "fedd_interface_match_get: null context");
    FEDD_CHECK(c->iface && c->iface->valid, "fedd_interface_match_get: no matched interface (fedd_interface_match first; fedd_mesh_set releases it)");
    const IfaceTable& t = *c->iface;
    if (iface_fluid) std::copy(t.h_f.begin(), t.h_f.end(), iface_fluid);
    if (iface_structure) std::copy(t.h_s.begin(), t.h_s.end(), iface_structure);
    if (flag_ptr) std::copy(t.flag_ptr.begin(), t.flag_ptr.end(), flag_ptr);
    return 0;
}

extern "C" int fedd_interface_match_info(fedd_ctx* c, int* have, int64_t* n_pairs, double* max_pair_distance, int* tile_points) {
    FEDD_CHECK(c, "fedd_interface_match_info: null context");
    const bool on = c->iface && c->iface->valid;
    if (have) *have = on ? 1 : 0;
    if (n_pairs) *n_pairs = on ? c->iface->n : 0;
    if (max_pair_distance) *max_pair_distance = on ? c->iface->max_dist : 0.0;
    if (tile_points) *tile_points = IM_TILE;
    return 0;
}

extern "C" int fedd_fsi_merge(fedd_ctx* c, fedd_ctx* fluid, fedd_ctx* structure, double dt, const uint8_t* coupled_mask) {
    FEDD_CHECK(c && fluid && structure, "fedd_fsi_merge: null context");
    FEDD_CHECK(c != fluid && c != structure && fluid != structure, "fedd_fsi_merge: the coupled context and the children must be three different contexts");
    FEDD_CHECK(dt > 0.0 && std::isfinite(dt), "fedd_fsi_merge: dt must be positive (got %g)", dt);
    FEDD_CHECK(c->nranks == 1 && fluid->nranks == 1 && structure->nranks == 1,
               "fedd_fsi_merge: one rank only (contexts with %d, %d and %d ranks were given)", c->nranks, fluid->nranks, structure->nranks);
    FEDD_CHECK(c->device >= 0 && fluid->device >= 0 && structure->device >= 0, "fedd_fsi_merge: this call %s (%s is host-only)", NEEDS_GPU,
               c->device < 0 ? "the coupled context" : (fluid->device < 0 ? "the fluid" : "the structure"));
    FEDD_CHECK(c->device == fluid->device && c->device == structure->device,
               "fedd_fsi_merge: contexts on different devices (coupled %d, fluid %d, structure %d)", c->device, fluid->device, structure->device);
    FEDD_CHECK(c->n_node == 0, "fedd_fsi_merge: the coupled context carries a mesh; it must be a context that never got one");
    const std::shared_ptr<IfaceTable> tab = fluid->iface;
    FEDD_CHECK(tab && tab == structure->iface && tab->valid && tab->uid_f == fluid->uid && tab->uid_s == structure->uid,
               "fedd_fsi_merge: no matched interface between exactly these two contexts (fedd_interface_match(fluid, structure) "
               "first; fedd_mesh_set on either releases it)");
    FEDD_CHECK(fluid->have_pattern, "fedd_fsi_merge: the fluid child holds no system");
    FEDD_CHECK(structure->have_pattern, "fedd_fsi_merge: the structure child holds no system");
    const int dim = tab->dim;
    FEDD_CHECK(fluid->merged, "fedd_fsi_merge: unmerged fluid: the fluid child does not hold the merged [F B^T; B C] (fedd_block_merge first)");
    FEDD_CHECK(fluid->merged_dofsA == dim && fluid->merged_nA == (int64_t)dim * fluid->n_own,
               "fedd_fsi_merge: the fluid child's velocity block has %lld rows, its mesh %lld nodes in %dD", (long long)fluid->merged_nA,
               (long long)fluid->n_own, dim);
    FEDD_CHECK(!structure->merged && structure->dofs == dim && structure->n_rows == (int64_t)dim * structure->n_own,
               "fedd_fsi_merge: the structure child's system has %lld rows, its mesh %lld nodes in %dD (a displacement system with %d "
               "dofs per node is expected)",
               (long long)structure->n_rows, (long long)structure->n_own, dim, dim);
    FEDD_CHECK(fluid->n_cols == fluid->n_rows && structure->n_cols == structure->n_rows, "fedd_fsi_merge: a child's system has ghost columns");
    const int64_t n_u = fluid->merged_nA, n_f = fluid->n_rows, n_s = structure->n_rows, n_l = (int64_t)dim * tab->n;
    const int64_t n = n_f + n_s + n_l;
    FEDD_CHECK(n < ((int64_t)1 << 31) && fluid->nnz + structure->nnz + 4 * n_l < ((int64_t)1 << 31),
               "fedd_fsi_merge: coupled system too large for 32-bit local offsets");
    FEDD_HIP(hipSetDevice(c->device));
    std::vector<uint8_t> mask((size_t)n_l, 1);
    if (coupled_mask)
        for (int64_t k = 0; k < n_l; ++k) mask[(size_t)k] = coupled_mask[k] ? 1 : 0;

    // the children's systems were written in their streams; the copies run in the coupled context's
    hipEvent_t ev = nullptr;
    FEDD_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    auto body = [&]() -> int {
        for (fedd_ctx* ch : {fluid, structure}) {
            FEDD_HIP(hipEventRecord(ev, ch->stream));
            FEDD_HIP(hipStreamWaitEvent(c->stream, ev, 0));
        }
        bool same = c->fsi_coupled && c->have_pattern && c->pattern_gen == c->fsi_pat_gen && c->fsi_table == tab &&
                    c->fsi_uid_f == fluid->uid && c->fsi_uid_s == structure->uid && c->fsi_mesh_gen_f == fluid->mesh_gen &&
                    c->fsi_mesh_gen_s == structure->mesh_gen && c->fsi_pat_gen_f == fluid->pattern_gen &&
                    c->fsi_pat_gen_s == structure->pattern_gen && c->fsi_nu == n_u && c->fsi_np == n_f - n_u && c->fsi_ns == n_s &&
                    c->fsi_nl == n_l && c->n_rows == n && c->fsi_mask == mask;
        if (!same) {
            // lambda-dof <-> child dof maps: dof dim * pair + component, -1 where the mask uncouples
            std::vector<int32_t> fd((size_t)n_l), sd((size_t)n_l);
            for (int64_t k = 0; k < n_l; ++k) {
                const int32_t nf = tab->h_f[(size_t)(k / dim)], ns = tab->h_s[(size_t)(k / dim)];
                FEDD_CHECK(nf >= 0 && nf < fluid->n_own && ns >= 0 && ns < structure->n_own, "fedd_fsi_merge: interface table out of range");
                fd[(size_t)k] = mask[(size_t)k] ? (int32_t)(dim * nf + k % dim) : -1;
                sd[(size_t)k] = mask[(size_t)k] ? (int32_t)(dim * ns + k % dim) : -1;
            }
            FEDD_TRY(c->d_fsi_fdof.ensure((size_t)n_l));
            FEDD_TRY(c->d_fsi_sdof.ensure((size_t)n_l));
            FEDD_TRY(c->d_fsi_lam_f.ensure((size_t)n_f));
            FEDD_TRY(c->d_fsi_lam_s.ensure((size_t)n_s));
            FEDD_HIP(hipStreamSynchronize(c->stream));      // (kernels of an earlier apply may still read the maps)
            FEDD_HIP(hipMemcpy(c->d_fsi_fdof.p, fd.data(), (size_t)n_l * sizeof(int32_t), hipMemcpyHostToDevice));
            FEDD_HIP(hipMemcpy(c->d_fsi_sdof.p, sd.data(), (size_t)n_l * sizeof(int32_t), hipMemcpyHostToDevice));
            FEDD_HIP(hipMemsetAsync(c->d_fsi_lam_f.p, 0xff, (size_t)n_f * sizeof(int32_t), c->stream));
            FEDD_HIP(hipMemsetAsync(c->d_fsi_lam_s.p, 0xff, (size_t)n_s * sizeof(int32_t), c->stream));
            const dim3 gl((unsigned)((n_l + 255) / 256));
            hipLaunchKernelGGL(k_fsi_lam, gl, dim3(256), 0, c->stream, (const int32_t*)c->d_fsi_fdof.p, (int32_t)n_l, c->d_fsi_lam_f.p);
            hipLaunchKernelGGL(k_fsi_lam, gl, dim3(256), 0, c->stream, (const int32_t*)c->d_fsi_sdof.p, (int32_t)n_l, c->d_fsi_lam_s.p);
            FEDD_HIP(hipGetLastError());
        }
        FsiView V;
        V.rp_f = fluid->d_rowptr.p, V.ci_f = fluid->d_colind.p, V.dir_f = fluid->d_isdir.p, V.v_f = fluid->d_val.p;
        V.rp_s = structure->d_rowptr.p, V.ci_s = structure->d_colind.p, V.dir_s = structure->d_isdir.p, V.v_s = structure->d_val.p;
        V.lam_f = c->d_fsi_lam_f.p, V.lam_s = c->d_fsi_lam_s.p, V.fdof = c->d_fsi_fdof.p, V.sdof = c->d_fsi_sdof.p;
        V.n_f = (int32_t)n_f, V.n_s = (int32_t)n_s, V.n_l = (int32_t)n_l;
        const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
        const double c2 = -(1.0 / dt);
        if (same) {     // the children's Dirichlet marks decide the coupling entries of their rows: the row lengths must still fit
            FEDD_TRY(c->d_flags.ensure(16));
            int32_t* d_flag = c->d_flags.p + 15;
            int32_t bad = 0;
            FEDD_HIP(hipMemsetAsync(d_flag, 0, sizeof(int32_t), c->stream));
            hipLaunchKernelGGL(k_fsi_check, grid, blk, 0, c->stream, V, (const int32_t*)c->d_rowptr.p, d_flag);
            FEDD_HIP(hipGetLastError());
            FEDD_HIP(hipMemcpyAsync(&bad, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            FEDD_HIP(hipStreamSynchronize(c->stream));
            same = bad == 0;
        }
        // a values-only merge keeps the pattern generation: the rule of fedd_matrix_import
        system_written(c, same ? SYS_VALUES : SYS_VALUES | SYS_PATTERN);
        c->fsi_last_values_only = same ? 1 : 0;
        if (same) {
            ++c->fsi_values_only_count;
            ScopedTimer t(c, FEDD_T_FSI_MERGE);
            t.bytes(16.0 * (double)c->nnz + 8.0 * (double)n);
            hipLaunchKernelGGL(k_fsi_fill<false>, grid, blk, 0, c->stream, V, c2, (const int32_t*)c->d_rowptr.p, c->d_colind.p, c->d_val.p);
            t.stop();
            FEDD_HIP(hipGetLastError());
        } else {
            c->have_pattern = false;
            c->fsi_coupled = false;     // until this merge has completed
            FEDD_TRY(c->d_rowptr.ensure((size_t)n + 1));
            int32_t mx = 0;
            int64_t nnz = 0;
            {
                ScopedTimer t(c, FEDD_T_FSI_MERGE);
                hipLaunchKernelGGL(k_fsi_count, grid, blk, 0, c->stream, V, c->d_rowptr.p);
                t.stop();
            }
            FEDD_HIP(hipGetLastError());
            FEDD_TRY(reduce_max_i32(c, c->d_rowptr.p, n, &mx));
            FEDD_TRY(exclusive_scan_i32(c, c->d_rowptr.p, c->d_rowptr.p, n, &nnz));
            FEDD_TRY(c->d_colind.ensure((size_t)nnz));
            FEDD_TRY(c->d_val.ensure((size_t)nnz));
            {
                ScopedTimer t(c, FEDD_T_FSI_MERGE);
                t.bytes(24.0 * (double)nnz + 8.0 * (double)n);
                hipLaunchKernelGGL(k_fsi_fill<true>, grid, blk, 0, c->stream, V, c2, (const int32_t*)c->d_rowptr.p, c->d_colind.p, c->d_val.p);
                t.stop();
            }
            FEDD_HIP(hipGetLastError());
            c->n_rows = c->n_rows_ext = c->n_cols = n;
            c->nnz = c->nnz_ext = nnz;
            c->max_row_nnz = mx;
            c->dofs = 1;
            c->block_mode = FEDD_BLOCK_SCALAR;
            c->merged = false;
            c->sys_pattern_id = 0;      // the system slot holds the pattern of none of this context's own slots
            c->sys_pattern_gen = c->pattern_gen;
            FEDD_TRY(c->d_rhs.ensure((size_t)n));
            FEDD_TRY(c->d_x.ensure((size_t)n));
            FEDD_TRY(c->d_xcol.ensure((size_t)n));
            FEDD_TRY(c->d_isdir.ensure((size_t)n));
        }
        // right-hand sides and Dirichlet marks of the children, lambda part zero; solution zeroed
        FEDD_HIP(hipMemcpyAsync(c->d_rhs.p, fluid->d_rhs.p, (size_t)n_f * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        FEDD_HIP(hipMemcpyAsync(c->d_rhs.p + n_f, structure->d_rhs.p, (size_t)n_s * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        FEDD_HIP(hipMemsetAsync(c->d_rhs.p + n_f + n_s, 0, (size_t)n_l * sizeof(double), c->stream));
        FEDD_HIP(hipMemcpyAsync(c->d_isdir.p, fluid->d_isdir.p, (size_t)n_f * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        FEDD_HIP(hipMemcpyAsync(c->d_isdir.p + n_f, structure->d_isdir.p, (size_t)n_s * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        FEDD_HIP(hipMemsetAsync(c->d_isdir.p + n_f + n_s, 0, (size_t)n_l * sizeof(int32_t), c->stream));
        FEDD_HIP(hipMemsetAsync(c->d_x.p, 0, (size_t)n * sizeof(double), c->stream));
        // a later writer of a child's system, in the child's stream, waits for the copies
        FEDD_HIP(hipEventRecord(ev, c->stream));
        FEDD_HIP(hipStreamWaitEvent(fluid->stream, ev, 0));
        FEDD_HIP(hipStreamWaitEvent(structure->stream, ev, 0));
        return 0;
    };
    const int rc = body();
    (void)hipEventDestroy(ev);
    if (rc) return rc;
    c->have_pattern = true;
    c->fsi_coupled = true;
    c->fsi_table = tab;
    c->fsi_uid_f = fluid->uid;
    c->fsi_uid_s = structure->uid;
    c->fsi_mesh_gen_f = fluid->mesh_gen;
    c->fsi_mesh_gen_s = structure->mesh_gen;
    c->fsi_pat_gen_f = fluid->pattern_gen;
    c->fsi_pat_gen_s = structure->pattern_gen;
    c->fsi_pat_gen = c->pattern_gen;
    c->fsi_nu = n_u;
    c->fsi_np = n_f - n_u;
    c->fsi_ns = n_s;
    c->fsi_nl = n_l;
    c->fsi_dt = dt;
    c->fsi_mask = mask;
    return 0;
}

extern "C" int fedd_fsi_interface_rhs(fedd_ctx* c, const double* d_old_structure) {
    FEDD_CHECK(c, "fedd_fsi_interface_rhs: null context");
    FEDD_CHECK(d_old_structure, "fedd_fsi_interface_rhs: null pointer");
    FEDD_CHECK(c->device >= 0, "fedd_fsi_interface_rhs: this call %s", NEEDS_GPU);
    FEDD_CHECK(c->have_pattern && c->fsi_coupled && c->pattern_gen == c->fsi_pat_gen,
               "fedd_fsi_interface_rhs: the context does not hold a coupled system (fedd_fsi_merge first)");
    FEDD_HIP(hipSetDevice(c->device));
    const int64_t n_s = c->fsi_ns, n_l = c->fsi_nl, off_l = c->fsi_nu + c->fsi_np + c->fsi_ns;
    FEDD_TRY(c->d_dtmp0.ensure((size_t)std::max<int64_t>(1, n_s)));
    FEDD_HIP(hipMemcpyAsync(c->d_dtmp0.p, d_old_structure, (size_t)n_s * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double c2 = -(1.0 / c->fsi_dt);
    if (n_l > 0)
        hipLaunchKernelGGL(k_fsi_rhs, dim3((unsigned)((n_l + 255) / 256)), dim3(256), 0, c->stream, (const int32_t*)c->d_fsi_sdof.p,
                           (int32_t)n_l, c2, (const double*)c->d_dtmp0.p, c->d_rhs.p + off_l);
    FEDD_HIP(hipGetLastError());
    FEDD_HIP(hipStreamSynchronize(c->stream));      // (the caller's array)
    return 0;
}

extern "C" int fedd_fsi_info(fedd_ctx* c, int64_t* n_u, int64_t* n_p, int64_t* n_s, int64_t* n_l, int64_t* offsets,
                             int* last_values_only, int64_t* n_values_only) {
    FEDD_CHECK(c, "fedd_fsi_info: null context");
    const bool on = c->have_pattern && c->fsi_coupled && c->pattern_gen == c->fsi_pat_gen;
    FEDD_CHECK(on, "fedd_fsi_info: the context does not hold a coupled system (fedd_fsi_merge first)");
    if (n_u) *n_u = c->fsi_nu;
    if (n_p) *n_p = c->fsi_np;
    if (n_s) *n_s = c->fsi_ns;
    if (n_l) *n_l = c->fsi_nl;
    if (offsets) {
        offsets[0] = 0;
        offsets[1] = c->fsi_nu;
        offsets[2] = c->fsi_nu + c->fsi_np;
        offsets[3] = c->fsi_nu + c->fsi_np + c->fsi_ns;
    }
    if (last_values_only) *last_values_only = c->fsi_last_values_only;
    if (n_values_only) *n_values_only = c->fsi_values_only_count;
    return 0;
}

extern "C" int fedd_fsi_prec_attach(fedd_ctx* c, fedd_ctx* fluid, fedd_ctx* structure) {
    FEDD_CHECK(c, "fedd_fsi_prec_attach: null context");
    FEDD_CHECK(fluid, "fedd_fsi_prec_attach: null child: the fluid context is NULL");
    FEDD_CHECK(structure, "fedd_fsi_prec_attach: null child: the structure context is NULL");
    FEDD_CHECK(fluid != c && structure != c && fluid != structure, "fedd_fsi_prec_attach: the coupled context and the children must be three different contexts");
    FEDD_CHECK(c->nranks == 1 && fluid->nranks == 1 && structure->nranks == 1,
               "fedd_fsi_prec_attach: one rank only (contexts with %d, %d and %d ranks were given)", c->nranks, fluid->nranks, structure->nranks);
    FEDD_CHECK(c->device >= 0 && fluid->device >= 0 && structure->device >= 0, "fedd_fsi_prec_attach: this call %s (%s is host-only)", NEEDS_GPU,
               c->device < 0 ? "the coupled context" : (fluid->device < 0 ? "the fluid" : "the structure"));
    FEDD_CHECK(fluid->device == c->device && structure->device == c->device,
               "fedd_fsi_prec_attach: contexts on different devices (coupled %d, fluid %d, structure %d)", c->device, fluid->device, structure->device);
    FEDD_CHECK(c->have_pattern && c->fsi_coupled && c->pattern_gen == c->fsi_pat_gen,
               "fedd_fsi_prec_attach: the context does not hold a coupled system (fedd_fsi_merge first)");
    FEDD_CHECK(c->fsi_uid_f == fluid->uid && c->fsi_uid_s == structure->uid,
               "fedd_fsi_prec_attach: the coupled system was merged from other contexts than these two");
    FEDD_CHECK(c->prec.kind != AttachedPrec::BLOCK, "fedd_fsi_prec_attach: a block preconditioner is attached (fedd_block_prec_detach first)");
    prec_unlink(c);             // (an earlier attach)
    prec_attach(c, AttachedPrec::FACSI, fluid, structure);
    return 0;
}

extern "C" int fedd_fsi_prec_detach(fedd_ctx* c) {
    FEDD_CHECK(c, "fedd_fsi_prec_detach: null context");
    const bool on = c->prec.kind == AttachedPrec::FACSI;
    if (on && c->device >= 0) {             // the children's kernels run in this context's stream: let them finish
        FEDD_HIP(hipSetDevice(c->device));
        FEDD_HIP(hipStreamSynchronize(c->stream));
    }
    if (on) prec_unlink(c);
    return 0;
}

extern "C" int fedd_fsi_prec_info(fedd_ctx* c, int* attached, int64_t* n_applies) {
    FEDD_CHECK(c, "fedd_fsi_prec_info: null context");
    const bool on = c->prec.kind == AttachedPrec::FACSI;
    if (attached) *attached = on ? 1 : 0;
    if (n_applies) *n_applies = on ? c->prec.applies : 0;
    return 0;
}
