// Device-resident Newton state for a Newmark step of a nonlinear single-block problem (unsteady hyperelasticity), one rank.
// gfx950 only.
//
// Replaces, on the device, what the reference does with Tpetra vectors in every Newton iteration of a time step:
//   TimeProblem::calculateNonLinResidualVec ("reverse")   feddlib/problems/abstract/TimeProblem_def.hpp:693-738
//   NonLinElasticity::calculateNonLinResidualVec           feddlib/problems/specific/NonLinElasticity_def.hpp:251-271
//   the update of NonLinearSolver::solveNewton             feddlib/problems/Solver/NonLinearSolver_def.hpp:459-531
// as sequenced by DAESolverInTime::advanceInTimeNonLinearNewmark (DAESolverInTime_def.hpp:613-722).
//
// Three kernels:
//   k_newton_residual  r = ((b - f) + s) - cm (M u_k), Dirichlet rows r = g - u_k, and the workgroup's share of |r|^2 in one pass:
//                      the row walk is the one of stored_rows.hpp, as k_block_apply (timestep.hip) makes it, so cm (M u_k)
//                      carries the bits of fedd_matrix_apply(slot_m, cm, u_k); the lane that finishes a row has loaded its b, f,
//                      s, u_k and node flag before the walk starts
//   k_newton_update    u_k <- u_k + alpha delta, nodal vector field <- u_k, the workgroup's share of |delta|^2: a pure stream of
//                      16-byte accesses over the row pairs (32 bytes per row), one scalar tail row when n is odd
//   k_newton_sum       the partial sums of either kernel added by one workgroup in a fixed order
// The normative operation order is in include/fedd_hip.h; no product is fused with a sum anywhere in this file and there is no
// floating-point atomic, so the residual can be restated bit for bit on the host and two calls agree bit for bit.
#include "stored_rows.hpp"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace fedd {
namespace {

// the workgroup's 256 values added by a fixed tree; the result in red[0]
__device__ __forceinline__ void wg_sum(double* red, double v) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
        __syncthreads();
    }
}

template <int G, bool SRC>
__global__ __launch_bounds__(256) void k_newton_residual(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                         const double* __restrict__ val, const double* __restrict__ u,
                                                         const double* __restrict__ b, const double* __restrict__ f,
                                                         const double* __restrict__ src, const int32_t* __restrict__ nflag, BcTable bc,
                                                         int32_t n_rows, double cm, double* __restrict__ r, double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t row = (int32_t)(t / G);
    const int g = (int)(t % G);
    const bool live = row < n_rows;
    const bool lead = live && g == 0;
    const int32_t s = live ? rowptr[row] : 0;
    const int32_t len = live ? rowptr[row + 1] - s : 0;
    double bv = 0.0, fv = 0.0, sv = 0.0, uv = 0.0;
    int32_t fl = 0;
    if (lead) {
        bv = b[row];
        fv = f[row];
        if (SRC) sv = src[row];
        uv = u[row];
        fl = nflag[row / bc.dofs];
    }
    const double acc = row_sum<G>(colind, val, s, len, g, [=](int32_t col) { return u[col]; });
    double sq = 0.0;
    if (lead) {
        const double m = cm * acc;
        double rv = bv - fv;
        if (SRC) rv = rv + sv;
        rv = rv - m;
        const int comp = row - (row / bc.dofs) * bc.dofs;
        const int hit = bc_hit(bc, fl, comp);
        if (hit >= 0) rv = bc.value[hit * bc.dofs + comp] - uv;
        r[row] = rv;
        sq = rv * rv;
    }
    wg_sum(red, sq);
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_newton_update(double* __restrict__ u, const double* __restrict__ d, double* __restrict__ vel,
                                                       int64_t n, double alpha, double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t n2 = n >> 1;
    double2* __restrict__ u2 = reinterpret_cast<double2*>(u);
    const double2* __restrict__ d2 = reinterpret_cast<const double2*>(d);
    double2* __restrict__ vel2 = reinterpret_cast<double2*>(vel);
    double sq = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
        double2 a = u2[i];
        const double2 dd = d2[i];
        const double px = alpha * dd.x, py = alpha * dd.y;
        a.x = a.x + px;
        a.y = a.y + py;
        u2[i] = a;
        vel2[i] = a;
        const double qx = dd.x * dd.x, qy = dd.y * dd.y;
        sq = sq + qx;
        sq = sq + qy;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        const double dd = d[i];
        const double p = alpha * dd;
        const double a = u[i] + p;
        u[i] = a;
        vel[i] = a;
        const double q = dd * dd;
        sq = sq + q;
    }
    wg_sum(red, sq);
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// out[0] = part[0] + ... in a fixed order: lane t adds part[t], part[t + 256], ..., then the tree
__global__ __launch_bounds__(256) void k_newton_sum(const double* __restrict__ part, int32_t n_part, double* __restrict__ out) {
    __shared__ double red[256];
    double sq = 0.0;
    for (int32_t i = threadIdx.x; i < n_part; i += 256) sq = sq + part[i];
    wg_sum(red, sq);
    if (threadIdx.x == 0) out[0] = red[0];
}

// sqrt of the sum of the n_part partial sums in d_nw_part (the sum goes behind them)
int norm_from_parts(fedd_ctx* c, int32_t n_part, double* norm) {
    double h = 0.0;
    hipLaunchKernelGGL(k_newton_sum, dim3(1), dim3(256), 0, c->stream, (const double*)c->d_nw_part.p, n_part, c->d_nw_part.p + n_part);
    FEDD_HIP(hipGetLastError());
    FEDD_HIP(hipMemcpyAsync(&h, c->d_nw_part.p + n_part, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    *norm = std::sqrt(h);
    return 0;
}

}  // namespace
}  // namespace fedd

using namespace fedd;

#define NEED_NEWTON(c, who)                                                                                          \
    FEDD_CHECK((c)->nw_active && (c)->nw_n == (c)->n_rows && (c)->d_nw_u.p,                                          \
               "%s: no Newton state (fedd_newton_begin first; fedd_newton_end and fedd_mesh_set end it)", who)

extern "C" int fedd_newton_begin(fedd_ctx* c) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_newton_begin");
    FEDD_CHECK(c->have_pattern && !c->merged && c->n_rowg == 0,
               "fedd_newton_begin: no single-block system (fedd_pattern_build or fedd_matrix_combine first)");
    FEDD_CHECK(c->dofs == c->dim && c->n_node == c->n_own && c->n_rows == c->n_own * c->dim,
               "fedd_newton_begin: the system must have dim dofs per node on a mesh without ghost nodes (the solution vector is "
               "also the nodal vector field)");
    FEDD_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)c->n_rows;
    FEDD_TRY(c->d_nw_u.ensure(n));
    FEDD_TRY(c->d_nw_b.ensure(n));
    FEDD_TRY(c->d_vel.ensure(n));
    const size_t bytes = n * sizeof(double);
    FEDD_HIP(hipMemcpyAsync(c->d_nw_u.p, c->d_x.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    FEDD_HIP(hipMemcpyAsync(c->d_nw_b.p, c->d_rhs.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    FEDD_HIP(hipMemcpyAsync(c->d_vel.p, c->d_x.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    c->have_vel = true;
    c->nw_n = (int64_t)n;
    c->nw_active = true;
    c->nw_have_src = false;
    c->nw_f_fresh = false;
    c->nw_residuals = c->nw_updates = 0;
    return 0;
}

extern "C" int fedd_newton_source_set(fedd_ctx* c, const double* s_owned) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_newton_source_set");
    NEED_NEWTON(c, "fedd_newton_source_set");
    FEDD_HIP(hipSetDevice(c->device));
    if (!s_owned) {
        c->nw_have_src = false;
        return 0;
    }
    FEDD_TRY(c->d_nw_s.ensure((size_t)c->nw_n));
    FEDD_HIP(hipMemcpyAsync(c->d_nw_s.p, s_owned, (size_t)c->nw_n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));   // the host buffer is the caller's
    c->nw_have_src = true;
    return 0;
}

extern "C" int fedd_newton_residual(fedd_ctx* c, int slot_m, double cm, int n_bc, const int32_t* flags, const int32_t* comp_mask,
                                    const double* values, double* norm2) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_newton_residual");
    CHECK_SLOT(slot_m);
    NEED_NEWTON(c, "fedd_newton_residual");
    const DevCsr& M = c->aux[slot_m];
    FEDD_CHECK(M.valid, "fedd_newton_residual: slot %d is empty", slot_m);
    FEDD_CHECK(M.n_rows == c->n_rows && M.n_cols == c->n_rows && M.mesh_id == c->mesh_id,
               "fedd_newton_residual: slot %d does not hold a square matrix of the system's size on the current mesh", slot_m);
    FEDD_CHECK(n_bc >= 0 && n_bc <= MAX_BC, "fedd_newton_residual: at most %d boundary conditions", MAX_BC);
    FEDD_CHECK(n_bc == 0 || (flags && values), "fedd_newton_residual: null array");
    FEDD_CHECK(c->have_hy_f, "fedd_newton_residual: no force vector (fedd_assemble_hyperelastic* with FEDD_HYPER_FORCE first)");
    FEDD_CHECK(c->nw_f_fresh,
               "fedd_newton_residual: the force vector is stale: it is older than the last fedd_newton_begin / fedd_newton_update "
               "(fedd_assemble_hyperelastic* with FEDD_HYPER_FORCE first)");
    FEDD_HIP(hipSetDevice(c->device));
    const BcTable bc = bc_table_fill(c->dofs, n_bc, flags, comp_mask, values);
    const int32_t n = (int32_t)c->n_rows;
    int32_t n_part = 1;     // one partial sum per workgroup of the walk (one, zero, where there is no row)
    FEDD_TRY(with_row_groups(M.max_row_nnz, n, [&](auto G, unsigned grid) {
        n_part = (int32_t)std::max(1u, grid);
        FEDD_TRY(c->d_nw_part.ensure((size_t)n_part + 1));
        if (n == 0) {
            FEDD_HIP(hipMemsetAsync(c->d_nw_part.p, 0, sizeof(double), c->stream));
            return 0;
        }
        const bool src = c->nw_have_src;
        ScopedTimer t(c, FEDD_T_NEWTON_RESIDUAL);
        // byte model: the block as k_block_apply counts it (values, columns, row pointers, u_k once), b, f, the source where set
        // and the node flags read, r written
        t.bytes(12.0 * (double)M.nnz + 4.0 * (double)(n + 1) + (src ? 40.0 : 32.0) * (double)n + 4.0 * (double)(n / c->dofs));
        auto launch = [&](auto SRC) {
            hipLaunchKernelGGL((k_newton_residual<decltype(G)::value, decltype(SRC)::value>), dim3(grid), dim3(256), 0, c->stream,
                               (const int32_t*)M.rowptr.p, (const int32_t*)M.colind.p, (const double*)M.val.p, (const double*)c->d_nw_u.p,
                               (const double*)c->d_nw_b.p, (const double*)c->d_hy_f.p, (const double*)c->d_nw_s.p,
                               (const int32_t*)c->d_flag.p, bc, n, cm, c->d_rhs.p, c->d_nw_part.p);
        };
        if (src) launch(std::true_type());
        else launch(std::false_type());
        t.stop();
        FEDD_HIP(hipGetLastError());
        return 0;
    }));
    ++c->nw_residuals;
    double nr = 0.0;
    FEDD_TRY(norm_from_parts(c, n_part, &nr));
    if (norm2) *norm2 = nr;
    return 0;
}

extern "C" int fedd_newton_update(fedd_ctx* c, double alpha, double* norm_delta) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_newton_update");
    NEED_NEWTON(c, "fedd_newton_update");
    FEDD_HIP(hipSetDevice(c->device));
    const int64_t n = c->n_rows;
    const int32_t n_part = (int32_t)std::min<int64_t>(2048, std::max<int64_t>(1, ((n >> 1) + 255) / 256));
    FEDD_TRY(c->d_nw_part.ensure((size_t)n_part + 1));
    {
        ScopedTimer t(c, FEDD_T_NEWTON_UPDATE);
        t.bytes(32.0 * (double)n);      // reads u_k, delta; writes u_k, the nodal vector field
        hipLaunchKernelGGL(k_newton_update, dim3((unsigned)n_part), dim3(256), 0, c->stream, c->d_nw_u.p, (const double*)c->d_x.p,
                           c->d_vel.p, n, alpha, c->d_nw_part.p);
        t.stop();
        FEDD_HIP(hipGetLastError());
    }
    c->nw_f_fresh = false;
    ++c->nw_updates;
    double nd = 0.0;
    FEDD_TRY(norm_from_parts(c, n_part, &nd));
    if (norm_delta) *norm_delta = nd;
    return 0;
}

extern "C" int fedd_newton_end(fedd_ctx* c) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_newton_end");
    NEED_NEWTON(c, "fedd_newton_end");
    FEDD_HIP(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->nw_n * sizeof(double);
    FEDD_HIP(hipMemcpyAsync(c->d_x.p, c->d_nw_u.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    FEDD_HIP(hipMemcpyAsync(c->d_rhs.p, c->d_nw_b.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    c->nw_active = false;
    return 0;
}

extern "C" int fedd_newton_get(fedd_ctx* c, double* u_k) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_newton_get");
    NEED_NEWTON(c, "fedd_newton_get");
    FEDD_CHECK(u_k, "fedd_newton_get: null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_HIP(hipMemcpy(u_k, c->d_nw_u.p, (size_t)c->nw_n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int fedd_newton_info(fedd_ctx* c, int* active, int64_t* n, int* have_source, int* force_fresh, int64_t* n_residuals,
                                int64_t* n_updates) {
    FEDD_CHECK(c, "fedd_newton_info: null context");
    if (active) *active = c->nw_active ? 1 : 0;
    if (n) *n = c->nw_active ? c->nw_n : 0;
    if (have_source) *have_source = c->nw_active && c->nw_have_src ? 1 : 0;
    if (force_fresh) *force_fresh = c->nw_f_fresh ? 1 : 0;
    if (n_residuals) *n_residuals = c->nw_residuals;
    if (n_updates) *n_updates = c->nw_updates;
    return 0;
}
