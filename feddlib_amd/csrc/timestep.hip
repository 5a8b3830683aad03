// Newmark time stepping for linear, single-block, SPD systems (unsteady linear elasticity), one rank.  gfx950 only.
//
// Replaces, on the device, what the reference does with Tpetra vectors and matrix-matrix additions per time step:
//   TimeProblem::combineSystems                       feddlib/problems/abstract/TimeProblem_def.hpp:359-408
//   TimeProblem::updateNewmarkRhs                     :473-524
//   TimeProblem::updateSolutionNewmarkPreviousStep    :875-981
//   DAESolverInTime::addSourceTermToRHS               feddlib/problems/Solver/DAESolverInTime_def.hpp:1444-1450
// as sequenced by DAESolverInTime::advanceInTimeLinearNewmark (:519-607).
//
// Four kernels:
//   k_combine_*   system <- cm M + ca A, one lane per stored entry of A; the position of M's entry inside A's row is closed form
//                 (both patterns expand from the same node-level pattern, symbolic.hip k_expand_pattern)
//   k_block_apply y = alpha M x on a stored block: the lane-group row walk of stored_rows.hpp, one sum per row
//   k_newmark     the vector part of a step in one pass: reads u, u_n, v, w, writes u_n, v, w, t (56 bytes per row)
//   k_multistep   the history of a BDF loop on a merged (velocity, pressure) system in one pass: reads u and u_0, writes u_0, u_1
//                 and t = coeff[0] u (+ coeff[1] u_0) (40 bytes per row), zeroes the pressure rows of the right-hand side
//                 (TimeProblem::updateSolutionMultiPreviousStep :833-849, updateMultistepRhs :417-438, as sequenced by
//                 DAESolverInTime::advanceInTimeNonLinearMultistep, DAESolverInTime_def.hpp:1209-1333)
// The normative operation order is in include/fedd_hip.h; no product is fused with a sum anywhere in this file, so the
// combine and the state update can be restated bit for bit on the host.
#include "stored_rows.hpp"
#include <algorithm>

#pragma clang fp contract(off)

namespace fedd {
namespace {

// ---- combine ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_combine_same(const double* __restrict__ m, const double* __restrict__ a, double cm,
                                                      double ca, int64_t nnz, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnz) return;
    const double pm = cm * m[i];
    const double pa = ca * a[i];
    out[i] = pm + pa;
}

// M has the DIAG node-block pattern, A the FULL one: entry k of A's row r = dofs * node + comp is (slot k / dofs, component
// k % dofs) of the node row; M's row r holds one entry per slot, in the same slot order.  Where M has no entry its value is 0.0.
constexpr int COMBINE_G = 16;
__global__ __launch_bounds__(256) void k_combine_diag(const int32_t* __restrict__ a_rowptr, const double* __restrict__ a_val,
                                                      const int32_t* __restrict__ m_rowptr, const double* __restrict__ m_val,
                                                      int32_t n_rows, int dofs, double cm, double ca, double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t row = (int32_t)(t / COMBINE_G);
    const int g = (int)(t % COMBINE_G);
    if (row >= n_rows) return;
    const int32_t s = a_rowptr[row], len = a_rowptr[row + 1] - s;
    const int32_t ms = m_rowptr[row], mlen = m_rowptr[row + 1] - ms;
    const int comp = row % dofs;
    for (int32_t k = g; k < len; k += COMBINE_G) {
        const int32_t sl = k / dofs;
        const int b = k - sl * dofs;
        const double mv = (b == comp && sl < mlen) ? m_val[ms + sl] : 0.0;
        const double pm = cm * mv;
        const double pa = ca * a_val[s + k];
        out[s + k] = pm + pa;
    }
}

// ---- y = alpha M x on a stored block ---------------------------------------------------------------------------------------
// G lanes per row, the walk and its order in stored_rows.hpp.  No stream, dictionary or classes: a stored block is read as it
// lies.
template <int G>
__global__ __launch_bounds__(256) void k_block_apply(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                     const double* __restrict__ val, const double* __restrict__ x, int32_t n_rows,
                                                     double alpha, double* __restrict__ y) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t row = (int32_t)(t / G);
    const int g = (int)(t % G);
    const bool live = row < n_rows;
    const int32_t s = live ? rowptr[row] : 0;
    const int32_t len = live ? rowptr[row + 1] - s : 0;
    const double acc = row_sum<G>(colind, val, s, len, g, [=](int32_t col) { return x[col]; });
    if (live && g == 0) y[row] = alpha * acc;
}

// ---- Newmark state ---------------------------------------------------------------------------------------------------------
struct NmCoef {
    double cuu, cuv, cuw;   // 1 / (dt^2 beta), 1 / (dt beta), (1/2 - beta) / beta
    double cvu, cvv, cvw;   // gamma / (dt beta), 1 - gamma / beta, dt (beta - gamma / 2) / beta
};

// one row of the step, in the operation order of include/fedd_hip.h (every product and every sum rounded on its own)
template <bool FIRST>
__device__ __forceinline__ void nm_row(const NmCoef& k, double u, double un, double& v, double& w, double& t) {
    if (!FIRST) {
        const double d = u - un;
        const double v1 = ((k.cvu * d) + (k.cvv * v)) + (k.cvw * w);
        const double w1 = ((k.cuu * d) - (k.cuv * v)) - (k.cuw * w);
        v = v1;
        w = w1;
    }
    t = ((k.cuu * u) + (k.cuv * v)) + (k.cuw * w);
}

// Pure stream: 16-byte accesses over the row pairs, one scalar tail row when n is odd (hipMalloc aligns every vector to 256
// bytes).  FIRST is a template parameter, not a run-time select behind the loads: the first step neither reads u_n nor writes
// v and w.
template <bool FIRST>
__global__ __launch_bounds__(256) void k_newmark(const double* __restrict__ u, double* __restrict__ un, double* __restrict__ v,
                                                 double* __restrict__ w, double* __restrict__ t, int64_t n, NmCoef k) {
    const int64_t n2 = n >> 1;
    const double2* __restrict__ u2 = reinterpret_cast<const double2*>(u);
    double2* __restrict__ un2 = reinterpret_cast<double2*>(un);
    double2* __restrict__ v2 = reinterpret_cast<double2*>(v);
    double2* __restrict__ w2 = reinterpret_cast<double2*>(w);
    double2* __restrict__ t2 = reinterpret_cast<double2*>(t);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
        const double2 a = u2[i];
        double2 b = FIRST ? a : un2[i];
        double2 c = v2[i], d = w2[i], e;
        nm_row<FIRST>(k, a.x, b.x, c.x, d.x, e.x);
        nm_row<FIRST>(k, a.y, b.y, c.y, d.y, e.y);
        un2[i] = a;
        if (!FIRST) {
            v2[i] = c;
            w2[i] = d;
        }
        t2[i] = e;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        const double a = u[i];
        const double b = FIRST ? a : un[i];
        double c = v[i], d = w[i], e;
        nm_row<FIRST>(k, a, b, c, d, e);
        un[i] = a;
        if (!FIRST) {
            v[i] = c;
            w[i] = d;
        }
        t[i] = e;
    }
}

// ---- multistep (BDF) history ---------------------------------------------------------------------------------------------------
// One row pair of fedd_multistep_advance, in the operation order of include/fedd_hip.h.  NUSE = coefficients in use, SHIFT2 =
// the old u_0 moves to u_1 (order 2 with a recorded vector).  The old u_0 is read where NUSE == 2 or SHIFT2 asks for it and
// nowhere else: a first step, and every step of an order-1 history, neither reads u_0 nor writes u_1.
template <int NUSE, bool SHIFT2>
__device__ __forceinline__ double ms_row(double c0, double c1, double u, double old0) {
    (void)c1;
    (void)old0;
    if (NUSE == 2) {
        const double p0 = c0 * u;
        const double p1 = c1 * old0;
        return p0 + p1;
    }
    return c0 * u;
}

// Pure stream like k_newmark: 16-byte accesses over the row pairs, one scalar tail row when n is odd.  The zero fill of
// rhs[n_m, n) rides along: a pair that lies at or above n_m stores 16 bytes, the pair n_m cuts (n_m odd) stores its upper row
// alone, so every 16-byte store is pair-aligned and none crosses n_m; rows below n_m are k_block_apply's.
template <int NUSE, bool SHIFT2>
__global__ __launch_bounds__(256) void k_multistep(const double* __restrict__ u, double* __restrict__ h0, double* __restrict__ h1,
                                                   double* __restrict__ t, double* __restrict__ rhs, int64_t n, int64_t n_m, double c0,
                                                   double c1) {
    constexpr bool HAVE0 = NUSE == 2 || SHIFT2;
    const int64_t n2 = n >> 1;
    const double2* __restrict__ u2 = reinterpret_cast<const double2*>(u);
    double2* __restrict__ h02 = reinterpret_cast<double2*>(h0);
    double2* __restrict__ h12 = reinterpret_cast<double2*>(h1);
    double2* __restrict__ t2 = reinterpret_cast<double2*>(t);
    double2* __restrict__ rhs2 = reinterpret_cast<double2*>(rhs);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
        const double2 a = u2[i];
        double2 o = a, e;
        if (HAVE0) o = h02[i];
        e.x = ms_row<NUSE, SHIFT2>(c0, c1, a.x, o.x);
        e.y = ms_row<NUSE, SHIFT2>(c0, c1, a.y, o.y);
        if (SHIFT2) h12[i] = o;
        h02[i] = a;
        t2[i] = e;
        const int64_t r = 2 * i;
        if (r >= n_m) rhs2[i] = make_double2(0.0, 0.0);
        else if (r + 1 >= n_m) rhs[r + 1] = 0.0;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        const double a = u[i];
        double o = a;
        if (HAVE0) o = h0[i];
        const double e = ms_row<NUSE, SHIFT2>(c0, c1, a, o);
        if (SHIFT2) h1[i] = o;
        h0[i] = a;
        t[i] = e;
        if (i >= n_m) rhs[i] = 0.0;
    }
}

__global__ __launch_bounds__(256) void k_axpy(double* __restrict__ y, const double* __restrict__ x, double alpha, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double p = alpha * x[i];
    y[i] = y[i] + p;
}

// the right-hand-side half of k_dirichlet (assemble.hip): the rows are unit rows already
__global__ void k_dirichlet_rhs(BcTable b, const int32_t* __restrict__ nflag, double* __restrict__ rhs, int32_t n_rows) {
    const int32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const int32_t node = row / b.dofs;
    const int comp = row - node * b.dofs;
    const int hit = bc_hit(b, nflag[node], comp);
    if (hit < 0) return;
    rhs[row] = b.value[hit * b.dofs + comp];
}

int block_apply_device(fedd_ctx* c, const DevCsr& m, double alpha, const double* d_x, double* d_y) {
    const int32_t n = (int32_t)m.n_rows;
    if (n == 0) return 0;
    ScopedTimer t(c, FEDD_T_BLOCK_APPLY);
    t.bytes(12.0 * (double)m.nnz + 4.0 * (double)(n + 1) + 16.0 * (double)n);
    with_row_groups(m.max_row_nnz, n, [&](auto G, unsigned grid) {
        hipLaunchKernelGGL(k_block_apply<decltype(G)::value>, dim3(grid), dim3(256), 0, c->stream, (const int32_t*)m.rowptr.p,
                           (const int32_t*)m.colind.p, (const double*)m.val.p, d_x, n, alpha, d_y);
        return 0;
    });
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}

int newmark_alloc(fedd_ctx* c) {
    const size_t n = (size_t)c->n_rows;
    if (c->nm_n == (int64_t)n && c->d_nm_un.p) return 0;
    FEDD_TRY(c->d_nm_un.ensure(n));
    FEDD_TRY(c->d_nm_v.ensure(n));
    FEDD_TRY(c->d_nm_w.ensure(n));
    FEDD_TRY(c->d_nm_t.ensure(n));
    FEDD_HIP(hipMemsetAsync(c->d_nm_un.p, 0, n * sizeof(double), c->stream));
    FEDD_HIP(hipMemsetAsync(c->d_nm_v.p, 0, n * sizeof(double), c->stream));
    FEDD_HIP(hipMemsetAsync(c->d_nm_w.p, 0, n * sizeof(double), c->stream));
    FEDD_HIP(hipMemsetAsync(c->d_nm_t.p, 0, n * sizeof(double), c->stream));
    c->nm_n = (int64_t)n;
    c->nm_first = true;
    return 0;
}

}  // namespace

int system_adopt_pattern(fedd_ctx* c, const DevCsr& m, int dofs, int block_mode, size_t n_xcol, bool zero_other_len, uint64_t pattern_id) {
    ScopedTimer t(c, FEDD_T_SYMBOLIC);
    const size_t n = (size_t)m.n_rows;
    const bool same_len = c->n_rows == m.n_rows && c->d_rhs.p && c->d_x.p && c->d_rhs.cap >= n && c->d_x.cap >= n;
    c->have_pattern = false;
    FEDD_TRY(c->d_rowptr.ensure(n + 1));
    FEDD_TRY(c->d_colind.ensure((size_t)m.nnz));
    FEDD_TRY(c->d_val.ensure((size_t)m.nnz));
    FEDD_TRY(c->d_rhs.ensure(n));
    FEDD_TRY(c->d_x.ensure(n));
    FEDD_TRY(c->d_xcol.ensure(n_xcol));
    FEDD_TRY(c->d_isdir.ensure(n));
    FEDD_HIP(hipMemcpyAsync(c->d_rowptr.p, m.rowptr.p, (n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    FEDD_HIP(hipMemcpyAsync(c->d_colind.p, m.colind.p, (size_t)m.nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    if (zero_other_len && !same_len) {
        FEDD_HIP(hipMemsetAsync(c->d_rhs.p, 0, n * sizeof(double), c->stream));
        FEDD_HIP(hipMemsetAsync(c->d_x.p, 0, n * sizeof(double), c->stream));
    }
    c->dofs = dofs;
    c->block_mode = block_mode;
    c->n_rows = c->n_rows_ext = m.n_rows;
    c->n_cols = m.n_cols;
    c->nnz = c->nnz_ext = m.nnz;
    c->max_row_nnz = m.max_row_nnz;
    c->merged = false;
    c->sys_pattern_id = pattern_id;
    c->sys_pattern_gen = c->pattern_gen;
    return 0;
}

}  // namespace fedd

using namespace fedd;

// what a combine of these slots would pair: 0 = same pattern, 1 = DIAG into FULL; errors otherwise
static int combine_pairing(fedd_ctx* c, int slot_m, int slot_a, int* kind) {
    const DevCsr& M = c->aux[slot_m];
    const DevCsr& A = c->aux[slot_a];
    FEDD_CHECK(M.valid, "fedd_matrix_combine: slot %d is empty", slot_m);
    FEDD_CHECK(A.valid, "fedd_matrix_combine: slot %d is empty", slot_a);
    FEDD_CHECK(M.mesh_id == c->mesh_id && A.mesh_id == c->mesh_id,
               "fedd_matrix_combine: slots %d and %d must hold matrices of the current mesh (a fedd_mesh_set came between)", slot_m, slot_a);
    FEDD_CHECK(M.block_mode >= 0 && A.block_mode >= 0 && M.dofs == A.dofs && M.n_rows == A.n_rows && M.n_cols == A.n_cols,
               "fedd_matrix_combine: slots %d and %d do not hold matrices of one space built by fedd_pattern_build", slot_m, slot_a);
    if (M.block_mode == A.block_mode && M.nnz == A.nnz) {
        *kind = 0;
        return 0;
    }
    FEDD_CHECK(!(M.block_mode == FEDD_BLOCK_FULL && A.block_mode == FEDD_BLOCK_DIAG),
               "fedd_matrix_combine: a FULL matrix (slot %d) does not fit into a DIAG pattern (slot %d); the result has the pattern of slot_a",
               slot_m, slot_a);
    FEDD_CHECK(M.block_mode == FEDD_BLOCK_DIAG && A.block_mode == FEDD_BLOCK_FULL && M.nnz * M.dofs == A.nnz,
               "fedd_matrix_combine: unsupported pattern pairing (block modes %d and %d): same pattern, or DIAG into FULL", M.block_mode,
               A.block_mode);
    *kind = 1;
    return 0;
}

extern "C" int fedd_matrix_combine(fedd_ctx* c, int slot_m, double cm, int slot_a, double ca) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_matrix_combine");
    CHECK_SLOT(slot_m);
    CHECK_SLOT(slot_a);
    int kind = 0;
    FEDD_TRY(combine_pairing(c, slot_m, slot_a, &kind));
    FEDD_CHECK(c->n_rowg == 0, "fedd_matrix_combine: a mesh with row ghosts belongs to several ranks");
    FEDD_HIP(hipSetDevice(c->device));
    const DevCsr& M = c->aux[slot_m];
    const DevCsr& A = c->aux[slot_a];
    const size_t n = (size_t)A.n_rows;
    const bool in_place = c->have_pattern && !c->merged && c->sys_pattern_id == A.pattern_id && c->sys_pattern_gen == c->pattern_gen &&
                          c->n_rows == A.n_rows && c->nnz == A.nnz;
    system_written(c, in_place ? SYS_VALUES : SYS_VALUES | SYS_PATTERN);
    // (vectors of another length are not a right-hand side and a solution of this system: they are zeroed)
    if (!in_place) FEDD_TRY(system_adopt_pattern(c, A, A.dofs, A.block_mode, (size_t)A.n_cols, true, A.pattern_id));
    FEDD_HIP(hipMemsetAsync(c->d_isdir.p, 0, n * sizeof(int32_t), c->stream));
    {
        ScopedTimer t(c, FEDD_T_ASSEMBLE);
        if (A.nnz > 0) {
            if (kind == 0)
                hipLaunchKernelGGL(k_combine_same, dim3((unsigned)((A.nnz + 255) / 256)), dim3(256), 0, c->stream, (const double*)M.val.p,
                                   (const double*)A.val.p, cm, ca, A.nnz, c->d_val.p);
            else
                hipLaunchKernelGGL(k_combine_diag, dim3((unsigned)(((int64_t)n * COMBINE_G + 255) / 256)), dim3(256), 0, c->stream,
                                   (const int32_t*)A.rowptr.p, (const double*)A.val.p, (const int32_t*)M.rowptr.p,
                                   (const double*)M.val.p, (int32_t)n, A.dofs, cm, ca, c->d_val.p);
        }
    }
    FEDD_HIP(hipGetLastError());
    c->have_pattern = true;
    c->comb_slot_m = slot_m;
    c->comb_slot_a = slot_a;
    c->comb_cm = cm;
    c->comb_ca = ca;
    c->comb_id_m = M.value_id;
    c->comb_id_a = A.value_id;
    c->comb_sys_gen = c->sys_value_gen;
    return 0;
}

extern "C" int fedd_matrix_combine_current(fedd_ctx* c, int slot_m, double cm, int slot_a, double ca, int* current) {
    FEDD_CHECK(c && current, "fedd_matrix_combine_current: null pointer");
    CHECK_SLOT(slot_m);
    CHECK_SLOT(slot_a);
    *current = c->have_pattern && c->comb_slot_m == slot_m && c->comb_slot_a == slot_a && c->comb_cm == cm &&
               c->comb_ca == ca && c->aux[slot_m].valid && c->aux[slot_a].valid && c->comb_id_m == c->aux[slot_m].value_id &&
               c->comb_id_a == c->aux[slot_a].value_id && c->comb_sys_gen == c->sys_value_gen;
    return 0;
}

extern "C" int fedd_matrix_apply(fedd_ctx* c, int slot, double alpha, const double* x_owned, double* y_owned) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_matrix_apply");
    CHECK_SLOT(slot);
    const DevCsr& m = c->aux[slot];
    FEDD_CHECK(m.valid, "fedd_matrix_apply: slot %d is empty", slot);
    FEDD_CHECK(x_owned && y_owned, "fedd_matrix_apply: null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_TRY(c->d_dtmp0.ensure(std::max<size_t>((size_t)(m.n_cols + m.n_rows), c->d_dtmp0.cap)));
    double* dx = c->d_dtmp0.p;
    double* dy = dx + m.n_cols;
    FEDD_HIP(hipMemcpyAsync(dx, x_owned, (size_t)m.n_cols * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FEDD_TRY(block_apply_device(c, m, alpha, dx, dy));
    FEDD_HIP(hipMemcpyAsync(y_owned, dy, (size_t)m.n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fedd_newmark_begin(fedd_ctx* c) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_newmark_begin");
    FEDD_CHECK(c->have_pattern && !c->merged, "fedd_newmark_begin: no single-block system (fedd_pattern_build or fedd_matrix_combine first)");
    FEDD_HIP(hipSetDevice(c->device));
    c->nm_n = -1;                       // zero v, w (and the scratch t)
    FEDD_TRY(newmark_alloc(c));
    FEDD_HIP(hipMemcpyAsync(c->d_nm_un.p, c->d_x.p, (size_t)c->n_rows * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    c->nm_first = true;
    return 0;
}

extern "C" int fedd_newmark_set(fedd_ctx* c, const double* u_n, const double* v, const double* w) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_newmark_set");
    FEDD_CHECK(c->have_pattern && !c->merged, "fedd_newmark_set: no single-block system");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_TRY(newmark_alloc(c));
    const size_t bytes = (size_t)c->n_rows * sizeof(double);
    if (u_n) FEDD_HIP(hipMemcpyAsync(c->d_nm_un.p, u_n, bytes, hipMemcpyHostToDevice, c->stream));
    if (v) FEDD_HIP(hipMemcpyAsync(c->d_nm_v.p, v, bytes, hipMemcpyHostToDevice, c->stream));
    if (w) FEDD_HIP(hipMemcpyAsync(c->d_nm_w.p, w, bytes, hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));   // the host buffers are the caller's
    c->nm_first = false;                // a state that was given is a state after some step (restart)
    return 0;
}

extern "C" int fedd_newmark_get(fedd_ctx* c, double* u_n, double* v, double* w) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_newmark_get");
    FEDD_CHECK(c->nm_n == c->n_rows && c->d_nm_un.p, "fedd_newmark_get: no Newmark state (fedd_newmark_begin or fedd_newmark_set first)");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    const size_t bytes = (size_t)c->n_rows * sizeof(double);
    if (u_n) FEDD_HIP(hipMemcpy(u_n, c->d_nm_un.p, bytes, hipMemcpyDeviceToHost));
    if (v) FEDD_HIP(hipMemcpy(v, c->d_nm_v.p, bytes, hipMemcpyDeviceToHost));
    if (w) FEDD_HIP(hipMemcpy(w, c->d_nm_w.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int fedd_newmark_advance(fedd_ctx* c, int slot_m, double dt, double beta, double gamma, double coeff) {
    FEDD_CHECK(dt > 0.0, "fedd_newmark_advance: dt must be positive (got %g)", dt);
    FEDD_CHECK(beta > 0.0, "fedd_newmark_advance: beta must be positive (got %g)", beta);
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_newmark_advance");
    CHECK_SLOT(slot_m);
    const DevCsr& M = c->aux[slot_m];
    FEDD_CHECK(M.valid, "fedd_newmark_advance: slot %d is empty", slot_m);
    FEDD_CHECK(c->have_pattern && !c->merged, "fedd_newmark_advance: no single-block system");
    FEDD_CHECK(M.n_rows == c->n_rows && M.n_cols == c->n_rows && M.mesh_id == c->mesh_id,
               "fedd_newmark_advance: slot %d does not hold a square matrix of the system's size on the current mesh", slot_m);
    FEDD_CHECK(c->nm_n == c->n_rows && c->d_nm_un.p, "fedd_newmark_advance: no Newmark state (fedd_newmark_begin or fedd_newmark_set first)");
    FEDD_HIP(hipSetDevice(c->device));
    NmCoef k;
    k.cuu = 1.0 / ((dt * dt) * beta);
    k.cuv = 1.0 / (dt * beta);
    k.cuw = (0.5 - beta) / beta;
    k.cvu = gamma / (dt * beta);
    k.cvv = 1.0 - (gamma / beta);
    k.cvw = (dt * (beta - (0.5 * gamma))) / beta;
    const int64_t n = c->n_rows;
    if (n > 0) {
        ScopedTimer t(c, FEDD_T_NEWMARK);
        t.bytes((c->nm_first ? 40.0 : 56.0) * (double)n);
        const unsigned grid = (unsigned)std::min<int64_t>(2048, std::max<int64_t>(1, ((n >> 1) + 255) / 256));
        if (c->nm_first)
            hipLaunchKernelGGL(k_newmark<true>, dim3(grid), dim3(256), 0, c->stream, (const double*)c->d_x.p, c->d_nm_un.p, c->d_nm_v.p,
                               c->d_nm_w.p, c->d_nm_t.p, n, k);
        else
            hipLaunchKernelGGL(k_newmark<false>, dim3(grid), dim3(256), 0, c->stream, (const double*)c->d_x.p, c->d_nm_un.p, c->d_nm_v.p,
                               c->d_nm_w.p, c->d_nm_t.p, n, k);
        t.stop();
        FEDD_HIP(hipGetLastError());
    }
    c->nm_first = false;
    return block_apply_device(c, M, coeff, c->d_nm_t.p, c->d_rhs.p);
}

// ---- multistep (BDF) history: include/fedd_hip.h "BDF time stepping" -------------------------------------------------------------
#define NEED_MULTISTEP(c, who)                                                                                   \
    FEDD_CHECK((c)->ms_order > 0 && (c)->d_ms_u[0].p && (c)->d_ms_t.p,                                           \
               "%s: no multistep history (fedd_multistep_begin first; a fedd_mesh_set releases it)", who)

extern "C" int fedd_multistep_begin(fedd_ctx* c, int order) {
    FEDD_CHECK(order == 1 || order == 2, "fedd_multistep_begin: order must be 1 or 2 (got %d)", order);
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_multistep_begin");
    FEDD_CHECK(c->have_pattern, "fedd_multistep_begin: no system (fedd_block_merge, fedd_pattern_build or fedd_matrix_combine first)");
    FEDD_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)c->n_rows;
    c->ms_order = c->ms_count = 0;
    for (int k = 0; k < 2; ++k) {
        if (k < order) {
            FEDD_TRY(c->d_ms_u[k].ensure(n));
            FEDD_HIP(hipMemsetAsync(c->d_ms_u[k].p, 0, n * sizeof(double), c->stream));
        } else {
            c->d_ms_u[k].release();
        }
    }
    FEDD_TRY(c->d_ms_t.ensure(n));   // (not zeroed: k_multistep writes all n rows before k_block_apply reads them)
    c->ms_n = (int64_t)n;
    c->ms_order = order;
    return 0;
}

extern "C" int fedd_multistep_info(fedd_ctx* c, int* order, int* count) {
    FEDD_CHECK(c, "fedd_multistep_info: null context");
    if (order) *order = c->ms_order;
    if (count) *count = c->ms_count;
    return 0;
}

extern "C" int fedd_multistep_set(fedd_ctx* c, int k, const double* u_k) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_multistep_set");
    NEED_MULTISTEP(c, "fedd_multistep_set");
    FEDD_CHECK(k >= 0 && k < c->ms_order, "fedd_multistep_set: k must be 0 .. order - 1 = %d (got %d)", c->ms_order - 1, k);
    FEDD_CHECK(u_k, "fedd_multistep_set: null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipMemcpyAsync(c->d_ms_u[k].p, u_k, (size_t)c->ms_n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));   // the host buffer is the caller's
    c->ms_count = std::max(c->ms_count, k + 1);  // a vector that was given is a state after some step (restart)
    return 0;
}

extern "C" int fedd_multistep_get(fedd_ctx* c, int k, double* u_k) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_multistep_get");
    NEED_MULTISTEP(c, "fedd_multistep_get");
    FEDD_CHECK(k >= 0 && k < c->ms_order, "fedd_multistep_get: k must be 0 .. order - 1 = %d (got %d)", c->ms_order - 1, k);
    FEDD_CHECK(u_k, "fedd_multistep_get: null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_HIP(hipMemcpy(u_k, c->d_ms_u[k].p, (size_t)c->ms_n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int fedd_multistep_advance(fedd_ctx* c, int slot_m, int n_use, const double* coeff) {
    FEDD_CHECK(n_use >= 1, "fedd_multistep_advance: n_use must be at least 1 (got %d)", n_use);
    FEDD_CHECK(coeff, "fedd_multistep_advance: null coefficient array");
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_multistep_advance");
    CHECK_SLOT(slot_m);
    NEED_MULTISTEP(c, "fedd_multistep_advance");
    FEDD_CHECK(c->have_pattern, "fedd_multistep_advance: no system");
    FEDD_CHECK(c->n_rows == c->ms_n,
               "fedd_multistep_advance: the system has %lld rows, the history was begun on %lld (fedd_multistep_begin again)",
               (long long)c->n_rows, (long long)c->ms_n);
    FEDD_CHECK(n_use <= std::min(c->ms_count + 1, c->ms_order),
               "fedd_multistep_advance: n_use %d exceeds min(count + 1, order) = %d (order %d, %d vectors recorded)", n_use,
               std::min(c->ms_count + 1, c->ms_order), c->ms_order, c->ms_count);
    const DevCsr& M = c->aux[slot_m];
    FEDD_CHECK(M.valid, "fedd_multistep_advance: slot %d is empty", slot_m);
    FEDD_CHECK(M.mesh_id == c->mesh_id, "fedd_multistep_advance: slot %d holds a matrix of an earlier mesh", slot_m);
    FEDD_CHECK(M.n_rows <= c->n_rows && M.n_cols <= c->n_rows,
               "fedd_multistep_advance: slot %d holds a %lld x %lld matrix, more rows or columns than the system's %lld", slot_m,
               (long long)M.n_rows, (long long)M.n_cols, (long long)c->n_rows);
    FEDD_HIP(hipSetDevice(c->device));
    const int64_t n = c->n_rows, n_m = M.n_rows;
    const bool shift2 = c->ms_order == 2 && c->ms_count >= 1;
    if (n > 0) {
        ScopedTimer t(c, FEDD_T_MULTISTEP);
        const unsigned grid = (unsigned)std::min<int64_t>(2048, std::max<int64_t>(1, ((n >> 1) + 255) / 256));
        const double c0 = coeff[0], c1 = n_use == 2 ? coeff[1] : 0.0;
        const double* u = c->d_x.p;
        double *h0 = c->d_ms_u[0].p, *h1 = c->d_ms_u[1].p, *tt = c->d_ms_t.p, *rhs = c->d_rhs.p;
        double row_bytes;       // the byte model of the instance launched (DESIGN section 4 "BDF")
        if (n_use == 2) {       // needs order 2 and a recorded vector: the shift is on
            row_bytes = 40.0;   // reads u, u_0; writes u_0, u_1, t
            hipLaunchKernelGGL((k_multistep<2, true>), dim3(grid), dim3(256), 0, c->stream, u, h0, h1, tt, rhs, n, n_m, c0, c1);
        } else if (shift2) {
            row_bytes = 40.0;
            hipLaunchKernelGGL((k_multistep<1, true>), dim3(grid), dim3(256), 0, c->stream, u, h0, h1, tt, rhs, n, n_m, c0, c1);
        } else {
            row_bytes = 24.0;   // reads u; writes u_0, t
            hipLaunchKernelGGL((k_multistep<1, false>), dim3(grid), dim3(256), 0, c->stream, u, h0, h1, tt, rhs, n, n_m, c0, c1);
        }
        t.bytes(row_bytes * (double)n + 8.0 * (double)(n - n_m));   // + the zero fill of the pressure rows
        t.stop();
        FEDD_HIP(hipGetLastError());
    }
    c->ms_count = std::min(c->ms_count + 1, c->ms_order);
    return block_apply_device(c, M, 1.0, c->d_ms_t.p, c->d_rhs.p);
}

extern "C" int fedd_rhs_axpy(fedd_ctx* c, double alpha, const double* f_owned) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_rhs_axpy");
    FEDD_CHECK(c->have_pattern && f_owned, "fedd_rhs_axpy: no pattern / null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    const int64_t n = c->n_rows;
    FEDD_TRY(c->d_dtmp0.ensure(std::max<size_t>((size_t)n, c->d_dtmp0.cap)));
    FEDD_HIP(hipMemcpyAsync(c->d_dtmp0.p, f_owned, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (n > 0) hipLaunchKernelGGL(k_axpy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_rhs.p, (const double*)c->d_dtmp0.p, alpha, n);
    FEDD_HIP(hipGetLastError());
    FEDD_HIP(hipStreamSynchronize(c->stream));   // the host buffer is the caller's
    return 0;
}

extern "C" int fedd_solution_set(fedd_ctx* c, const double* x_owned) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_solution_set");
    FEDD_CHECK(c->have_pattern, "fedd_solution_set: no system (fedd_pattern_build or fedd_matrix_combine first)");
    FEDD_CHECK(x_owned, "fedd_solution_set: null pointer");
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipMemcpy(c->d_x.p, x_owned, (size_t)c->n_rows * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int fedd_dirichlet_rhs(fedd_ctx* c, int n_bc, const int32_t* flags, const int32_t* comp_mask, const double* values) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_dirichlet_rhs");
    FEDD_CHECK(c->have_pattern && !c->merged, "fedd_dirichlet_rhs: no single-block system");
    // (the kernel reads the flag of every row's node: a coupled context of fedd_fsi_merge has rows and no nodes)
    FEDD_CHECK(c->n_node > 0 && c->n_rows <= (int64_t)c->dofs * c->n_node,
               "fedd_dirichlet_rhs: this context carries no mesh (a coupled context of fedd_fsi_merge never does), or its system has "
               "more rows than its mesh has dofs: the call needs the flags of the nodes of a fedd_mesh_set");
    FEDD_CHECK(n_bc >= 0 && n_bc <= MAX_BC, "fedd_dirichlet_rhs: at most %d boundary conditions", MAX_BC);
    FEDD_CHECK(n_bc == 0 || (flags && values), "fedd_dirichlet_rhs: null array");
    FEDD_HIP(hipSetDevice(c->device));
    const BcTable b = bc_table_fill(c->dofs, n_bc, flags, comp_mask, values);
    ScopedTimer t(c, FEDD_T_DIRICHLET);
    if (c->n_rows > 0)
        hipLaunchKernelGGL(k_dirichlet_rhs, dim3((unsigned)((c->n_rows + 255) / 256)), dim3(256), 0, c->stream, b,
                           (const int32_t*)c->d_flag.p, c->d_rhs.p, (int32_t)c->n_rows);
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}
