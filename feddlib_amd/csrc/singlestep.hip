// Single-step (Runge-Kutta) time stepping for nonlinear block problems (unsteady Navier-Stokes), one rank.  gfx950 only.
//
// The multi-stage part of the reference's "Class" = "Singlestep" loop, DAESolverInTime::advanceInTimeNonLinear
// (feddlib/problems/Solver/DAESolverInTime_def.hpp:384-516) with the Butcher tables of TimeSteppingTools::setTableInformationRK
// (TimeSteppingTools.cpp:309-487): what it keeps in matrixPrevStages / solutionPrevStages, what buildMultiStageRhs forms from
// them with BlockMatrix::apply (BlockMatrix_def.hpp:371-392), and the error norm of TimeSteppingTools::adaptiveTimestep.
//
// Three kernels:
//   k_stage_rhs    rhs <- [M u_0 + sum_j (cf_j (F_j u_j) + cbt_j (B^T p_j)) ; 0] over the velocity rows: the lane-group row walk of
//                  stored_rows.hpp with one sum per stage.  All F_j lie on one pattern, so its row pointers and columns are read
//                  once per row for all of them, and the B^T pattern once for all p_j
//   k_err_*        d = U_a - U_b on the fly: sum d_i^2 over all rows, or sum d_i (M d)_i over the velocity rows; one partial per
//                  wave, each a fixed shuffle tree
//   k_err_final    the partials in a fixed order by one wave
// The stage operators and solutions are buffers of their own (fedd_ctx::d_st_val, d_st_u), not matrix slots.  The normative
// operation order is in include/fedd_hip.h; no product is fused with a sum anywhere in this file.
#include "stored_rows.hpp"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace fedd {
namespace {

// what a launch of k_stage_rhs needs of the stages, by value: no device table, no copy per call
struct StageArgs {
    const double* f[MAX_STAGES];    // values of F_j on the stages' pattern
    const double* u[MAX_STAGES];    // U_j = [u_j ; p_j]
    double cf[MAX_STAGES], cbt[MAX_STAGES];
    int n_prior;
};

struct PatView {
    const int32_t* rowptr;
    const int32_t* colind;
    const double* val;
    int g;                          // the lane group fedd_matrix_apply takes for this block (with_row_groups)
};

// NP sums over one pattern: sum j has the value array v[j] (nullptr: off; v[0] is the walk's own) and the vector xv[j]
template <int NP>
struct StageSums {
    static constexpr int EXTRA = NP - 1;
    const double* v[NP];
    const double* xv[NP];
    double acc[NP];
    __device__ bool keep(int32_t) const { return true; }
    __device__ double x(int32_t col) const { return xv[0][col]; }
    __device__ void add(int32_t, double p) { acc[0] += p; }
    __device__ const double* val_extra(int e) const { return v[e + 1]; }
    __device__ double x_extra(int e, int32_t col) const { return xv[e + 1][col]; }
    __device__ void add_extra(int e, double p) { acc[e + 1] += p; }
    template <int G>
    __device__ void fold(int o) {
#pragma unroll
        for (int j = 0; j < NP; ++j) acc[j] += __shfl_xor(acc[j], o, G);
    }
};

// The walk of a block whose own lane group is gsub inside a kernel with GK >= gsub lanes per row: the first gsub lanes of the
// row's GK walk it exactly as k_block_apply<gsub> does, the others walk an empty row (the tree needs all lanes); lane 0 holds
// the sum either way.  gsub is uniform over the launch.
template <int GK, class Sums>
__device__ __forceinline__ void walk_in_group(int gsub, const int32_t* __restrict__ colind, const double* __restrict__ val, int32_t s,
                                              int32_t len, int g, Sums& sums) {
    if constexpr (GK == 16) {
        if (gsub == 16) row_walk<16>(colind, val, s, len, g, sums);
        else row_walk<8>(colind, val, s, g < 8 ? len : 0, g, sums);
    } else {
        row_walk<8>(colind, val, s, len, g, sums);
    }
}

// GK lanes per velocity row; NP = the sums compiled in (n_prior <= NP of them on).  Threads [0, n - n_m) also zero the
// pressure rows of the right-hand side.
template <int GK, int NP>
__global__ __launch_bounds__(256) void k_stage_rhs(PatView M, PatView F, PatView BT, StageArgs a, int32_t n_m, int64_t n,
                                                   double* __restrict__ rhs) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n - n_m) rhs[n_m + t] = 0.0;
    const int32_t row = (int32_t)(t / GK);
    const int g = (int)(t % GK);
    const bool live = row < n_m;
    // t = rowsum(M, u_0)
    const double* __restrict__ u0 = a.u[0];
    auto x0 = [=](int32_t col) { return u0[col]; };
    RowSum<decltype(x0)> sm{x0};
    {
        const int32_t s = live ? M.rowptr[row] : 0;
        const int32_t len = live ? M.rowptr[row + 1] - s : 0;
        walk_in_group<GK>(M.g, M.colind, M.val, s, len, g, sm);
    }
    // rowsum(F_j, u_j) of every prior stage in one walk of the stages' pattern
    StageSums<NP> sf, sb;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        sf.v[j] = j < a.n_prior ? a.f[j] : nullptr;
        sf.xv[j] = a.u[j];
        sf.acc[j] = 0.0;
        sb.v[j] = j < a.n_prior && a.cbt[j] != 0.0 ? BT.val : nullptr;
        sb.xv[j] = a.u[j] + n_m;
        sb.acc[j] = 0.0;
    }
    {
        const int32_t s = live ? F.rowptr[row] : 0;
        const int32_t len = live ? F.rowptr[row + 1] - s : 0;
        walk_in_group<GK>(F.g, F.colind, a.f[0], s, len, g, sf);
    }
    // rowsum(B^T, p_j) where coeff_bt[j] != 0.0 (BT.rowptr == nullptr: no such j); the first sum rides along unasked where
    // coeff_bt[0] == 0.0 and is not read then
    if (BT.rowptr) {
        const int32_t s = live ? BT.rowptr[row] : 0;
        const int32_t len = live ? BT.rowptr[row + 1] - s : 0;
        walk_in_group<GK>(BT.g, BT.colind, BT.val, s, len, g, sb);
    }
    if (!live || g != 0) return;
    double tt = sm.acc;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        if (j < a.n_prior) {
            double mv = a.cf[j] * sf.acc[j];
            if (a.cbt[j] != 0.0) {
                const double pb = a.cbt[j] * sb.acc[j];
                mv = mv + pb;
            }
            tt = tt + mv;
        }
    }
    rhs[row] = tt;
}

// ---- error norms ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum_i (ua_i - ub_i)^2: a fixed grid, every lane adds its rows in ascending order, one partial per wave
__global__ __launch_bounds__(256) void k_err_euclid(const double* __restrict__ ua, const double* __restrict__ ub, int64_t n,
                                                    double* __restrict__ part) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double acc = 0.0;
    for (int64_t i = t; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double d = ua[i] - ub[i];
        const double p = d * d;
        acc = acc + p;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[t >> 6] = acc;
}

// sum_i d_i * rowsum(M, d)_i over the rows of M, d = ua - ub formed where it is read; rowsum as k_block_apply<G> forms it
template <int G>
__global__ __launch_bounds__(256) void k_err_l2(PatView M, const double* __restrict__ ua, const double* __restrict__ ub, int32_t n_rows,
                                                double* __restrict__ part) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t row = (int32_t)(t / G);
    const int g = (int)(t % G);
    const bool live = row < n_rows;
    const int32_t s = live ? M.rowptr[row] : 0;
    const int32_t len = live ? M.rowptr[row + 1] - s : 0;
    const double acc = row_sum<G>(M.colind, M.val, s, len, g, [=](int32_t col) { return ua[col] - ub[col]; });
    double term = 0.0;
    if (live && g == 0) {
        const double d = ua[row] - ub[row];
        term = d * acc;
    }
    term = wave_sum(term);
    if ((threadIdx.x & 63) == 0) part[t >> 6] = term;
}

// one wave: lane l adds partials l, l + 64, ... in ascending order, then the tree
__global__ __launch_bounds__(64) void k_err_final(const double* __restrict__ part, int64_t n_part, double* __restrict__ out) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n_part; i += 64) acc = acc + part[i];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) out[0] = acc;
}

PatView view_of(const DevCsr& m) {
    PatView v{m.rowptr.p, m.colind.p, m.val.p, 8};
    with_row_groups(m.max_row_nnz, m.n_rows, [&](auto G, unsigned) {
        v.g = decltype(G)::value;
        return 0;
    });
    return v;
}

template <int GK>
void launch_stage_rhs(fedd_ctx* c, unsigned grid, const PatView& M, const PatView& F, const PatView& BT, const StageArgs& a, int32_t n_m,
                      int64_t n) {
    const dim3 gr(grid), blk(256);
    if (a.n_prior <= 1) hipLaunchKernelGGL((k_stage_rhs<GK, 1>), gr, blk, 0, c->stream, M, F, BT, a, n_m, n, c->d_rhs.p);
    else if (a.n_prior <= 2) hipLaunchKernelGGL((k_stage_rhs<GK, 2>), gr, blk, 0, c->stream, M, F, BT, a, n_m, n, c->d_rhs.p);
    else if (a.n_prior <= 4) hipLaunchKernelGGL((k_stage_rhs<GK, 4>), gr, blk, 0, c->stream, M, F, BT, a, n_m, n, c->d_rhs.p);
    else hipLaunchKernelGGL((k_stage_rhs<GK, MAX_STAGES>), gr, blk, 0, c->stream, M, F, BT, a, n_m, n, c->d_rhs.p);
}

// the slot the stages' pattern is read from still holds it
bool stage_pattern_stands(const fedd_ctx* c) {
    return c->st_slot >= 0 && c->aux[c->st_slot].valid && c->aux[c->st_slot].pattern_id == c->st_pattern_id &&
           c->aux[c->st_slot].mesh_id == c->mesh_id;
}

}  // namespace
}  // namespace fedd

using namespace fedd;

#define NEED_STEP(c, who)                                                                                                            \
    FEDD_CHECK((c)->st_max > 0, "%s: no open step (fedd_stage_begin first; a fedd_mesh_set releases the stage store)", who)

extern "C" int fedd_stage_begin(fedd_ctx* c, int max_stages) {
    FEDD_CHECK(max_stages >= 2 && max_stages <= MAX_STAGES, "fedd_stage_begin: max_stages must be 2 .. %d (got %d)", MAX_STAGES,
               max_stages);
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_stage_begin");
    c->st_max = max_stages;
    c->st_count = 0;            // (the buffers stay: the next step's stages are of the same size)
    return 0;
}

extern "C" int fedd_stage_info(fedd_ctx* c, int* max_stages, int* count, int64_t* nnz, int64_t* n) {
    FEDD_CHECK(c, "fedd_stage_info: null context");
    if (max_stages) *max_stages = c->st_max;
    if (count) *count = c->st_count;
    if (nnz) *nnz = c->st_count > 0 ? c->st_nnz : 0;
    if (n) *n = c->st_count > 0 ? c->st_n : 0;
    return 0;
}

extern "C" int fedd_stage_push(fedd_ctx* c, int slot_f) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_stage_push");
    CHECK_SLOT(slot_f);
    NEED_STEP(c, "fedd_stage_push");
    FEDD_CHECK(c->st_count < c->st_max, "fedd_stage_push: the step was opened for %d stages and holds %d", c->st_max, c->st_count);
    const DevCsr& F = c->aux[slot_f];
    FEDD_CHECK(F.valid, "fedd_stage_push: slot %d is empty", slot_f);
    FEDD_CHECK(F.mesh_id == c->mesh_id, "fedd_stage_push: slot %d holds a matrix of an earlier mesh", slot_f);
    FEDD_CHECK(c->have_pattern, "fedd_stage_push: no system (fedd_block_merge first): the stage solution is the system's solution vector");
    FEDD_CHECK(F.n_rows <= c->n_rows && F.n_cols <= c->n_rows,
               "fedd_stage_push: slot %d holds a %lld x %lld matrix, more rows or columns than the system's %lld", slot_f,
               (long long)F.n_rows, (long long)F.n_cols, (long long)c->n_rows);
    if (c->st_count > 0) {
        FEDD_CHECK(F.pattern_id == c->st_pattern_id && slot_f == c->st_slot && F.nnz == c->st_nnz && F.n_rows == c->st_rows,
                   "fedd_stage_push: slot %d holds another pattern than the first stage of this step (slot %d): the stages of a step "
                   "share one pattern",
                   slot_f, c->st_slot);
        FEDD_CHECK(c->n_rows == c->st_n, "fedd_stage_push: the system has %lld rows, the first stage of this step was pushed on %lld",
                   (long long)c->n_rows, (long long)c->st_n);
    }
    FEDD_HIP(hipSetDevice(c->device));
    const int j = c->st_count;
    const size_t nnz = (size_t)F.nnz, n = (size_t)c->n_rows;
    FEDD_TRY(c->d_st_val[j].ensure(nnz));
    FEDD_TRY(c->d_st_u[j].ensure(n));
    FEDD_HIP(hipMemcpyAsync(c->d_st_val[j].p, F.val.p, nnz * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    FEDD_HIP(hipMemcpyAsync(c->d_st_u[j].p, c->d_x.p, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (j == 0) {
        c->st_slot = slot_f;
        c->st_pattern_id = F.pattern_id;
        c->st_nnz = F.nnz;
        c->st_rows = F.n_rows;
        c->st_n = c->n_rows;
    }
    c->st_count = j + 1;
    return 0;
}

extern "C" int fedd_stage_get(fedd_ctx* c, int j, double* f_val, double* u) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_stage_get");
    NEED_STEP(c, "fedd_stage_get");
    FEDD_CHECK(j >= 0 && j < c->st_count, "fedd_stage_get: stage %d of %d", j, c->st_count);
    FEDD_HIP(hipSetDevice(c->device));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    if (f_val) FEDD_HIP(hipMemcpy(f_val, c->d_st_val[j].p, (size_t)c->st_nnz * sizeof(double), hipMemcpyDeviceToHost));
    if (u) FEDD_HIP(hipMemcpy(u, c->d_st_u[j].p, (size_t)c->st_n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int fedd_stage_rhs(fedd_ctx* c, int slot_m, int slot_bt, int n_prior, const double* coeff_f, const double* coeff_bt) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_stage_rhs");
    CHECK_SLOT(slot_m);
    FEDD_CHECK(slot_bt < MAX_AUX, "matrix slot %d out of range", slot_bt);
    NEED_STEP(c, "fedd_stage_rhs");
    FEDD_CHECK(c->st_count > 0, "fedd_stage_rhs: no stages (fedd_stage_push first)");
    FEDD_CHECK(n_prior >= 1 && n_prior <= c->st_count, "fedd_stage_rhs: n_prior must be 1 .. count = %d (got %d)", c->st_count, n_prior);
    FEDD_CHECK(coeff_f && coeff_bt, "fedd_stage_rhs: null coefficient array");
    bool any_bt = false;
    for (int j = 0; j < n_prior; ++j) any_bt = any_bt || coeff_bt[j] != 0.0;
    FEDD_CHECK(slot_bt >= 0 || !any_bt, "fedd_stage_rhs: slot_bt < 0 needs every coeff_bt to be 0.0");
    FEDD_CHECK(stage_pattern_stands(c),
               "fedd_stage_rhs: slot %d no longer holds the pattern of the stages (it was stored or assembled anew since the first fedd_stage_push)",
               c->st_slot);
    FEDD_CHECK(c->have_pattern && c->n_rows == c->st_n, "fedd_stage_rhs: the system has %lld rows, the stages were pushed on %lld",
               (long long)(c->have_pattern ? c->n_rows : 0), (long long)c->st_n);
    const DevCsr& M = c->aux[slot_m];
    FEDD_CHECK(M.valid, "fedd_stage_rhs: slot %d is empty", slot_m);
    FEDD_CHECK(M.mesh_id == c->mesh_id, "fedd_stage_rhs: slot %d holds a matrix of an earlier mesh", slot_m);
    const int64_t n = c->st_n, n_m = c->st_rows;
    FEDD_CHECK(M.n_rows == n_m && M.n_cols <= n, "fedd_stage_rhs: slot %d holds a %lld x %lld matrix, the stage operators have %lld rows",
               slot_m, (long long)M.n_rows, (long long)M.n_cols, (long long)n_m);
    const DevCsr& F = c->aux[c->st_slot];
    PatView vBT{nullptr, nullptr, nullptr, 8};
    if (any_bt) {
        const DevCsr& BT = c->aux[slot_bt];
        FEDD_CHECK(BT.valid, "fedd_stage_rhs: slot %d is empty", slot_bt);
        // (fedd_assemble_div stamps no mesh on its blocks: the shape is what can be checked)
        FEDD_CHECK(BT.n_rows == n_m, "fedd_stage_rhs: B^T in slot %d has %lld rows, the stage operators %lld", slot_bt,
                   (long long)BT.n_rows, (long long)n_m);
        FEDD_CHECK(BT.n_cols == n - n_m, "fedd_stage_rhs: B^T in slot %d has %lld columns, the system %lld pressure rows", slot_bt,
                   (long long)BT.n_cols, (long long)(n - n_m));
        vBT = view_of(BT);
    }
    FEDD_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    const PatView vM = view_of(M);
    PatView vF = view_of(F);
    vF.val = nullptr;   // (the slot's values are the caller's next operator: the stages' values are in the store)
    StageArgs a;
    for (int j = 0; j < MAX_STAGES; ++j) {
        const bool on = j < n_prior;
        a.f[j] = on ? c->d_st_val[j].p : nullptr;
        a.u[j] = on ? c->d_st_u[j].p : c->d_st_u[0].p;
        a.cf[j] = on ? coeff_f[j] : 0.0;
        a.cbt[j] = on ? coeff_bt[j] : 0.0;
    }
    a.n_prior = n_prior;
    const int gk = std::max(vM.g, std::max(vF.g, vBT.g));
    const unsigned grid = (unsigned)((std::max<int64_t>(n_m * gk, n - n_m) + 255) / 256);
    if (gk == 16) launch_stage_rhs<16>(c, grid, vM, vF, vBT, a, (int32_t)n_m, n);
    else launch_stage_rhs<8>(c, grid, vM, vF, vBT, a, (int32_t)n_m, n);
    FEDD_HIP(hipGetLastError());
    return 0;
}

extern "C" int fedd_stage_error(fedd_ctx* c, int kind, int slot_m, int ja, int jb, double* err) {
    NEED_DEVICE(c);
    ONE_RANK(c, "fedd_stage_error");
    FEDD_CHECK(kind == FEDD_STAGE_ERR_EUCLIDEAN || kind == FEDD_STAGE_ERR_L2, "fedd_stage_error: unknown kind %d", kind);
    FEDD_CHECK(err, "fedd_stage_error: null pointer");
    NEED_STEP(c, "fedd_stage_error");
    FEDD_CHECK(c->st_count > 0, "fedd_stage_error: no stages (fedd_stage_push first)");
    FEDD_CHECK(ja >= -1 && ja < c->st_count && jb >= -1 && jb < c->st_count,
               "fedd_stage_error: stage indices must be -1 (the current solution) .. count - 1 = %d (got %d and %d)", c->st_count - 1, ja, jb);
    FEDD_CHECK((ja >= 0 && jb >= 0) || (c->have_pattern && c->n_rows == c->st_n),
               "fedd_stage_error: the system has %lld rows, the stages were pushed on %lld", (long long)(c->have_pattern ? c->n_rows : 0),
               (long long)c->st_n);
    const int64_t n = c->st_n;
    const DevCsr* M = nullptr;
    if (kind == FEDD_STAGE_ERR_L2) {
        CHECK_SLOT(slot_m);
        M = &c->aux[slot_m];
        FEDD_CHECK(M->valid, "fedd_stage_error: slot %d is empty", slot_m);
        FEDD_CHECK(M->mesh_id == c->mesh_id, "fedd_stage_error: slot %d holds a matrix of an earlier mesh", slot_m);
        FEDD_CHECK(M->n_rows <= n && M->n_cols <= n, "fedd_stage_error: slot %d holds a %lld x %lld matrix, the stage vectors have %lld rows",
                   slot_m, (long long)M->n_rows, (long long)M->n_cols, (long long)n);
    }
    FEDD_HIP(hipSetDevice(c->device));
    const double* ua = ja < 0 ? c->d_x.p : c->d_st_u[ja].p;
    const double* ub = jb < 0 ? c->d_x.p : c->d_st_u[jb].p;
    const int64_t work = kind == FEDD_STAGE_ERR_L2 ? M->n_rows : n;
    if (work == 0) {
        *err = 0.0;
        return 0;
    }
    unsigned grid = 0;
    if (kind == FEDD_STAGE_ERR_EUCLIDEAN) {
        grid = (unsigned)std::min<int64_t>(1024, (n + 255) / 256);
        FEDD_TRY(c->d_st_part.ensure((size_t)grid * 4 + 1));
        hipLaunchKernelGGL(k_err_euclid, dim3(grid), dim3(256), 0, c->stream, ua, ub, n, c->d_st_part.p + 1);
    } else {
        const PatView vM = view_of(*M);
        grid = (unsigned)((M->n_rows * vM.g + 255) / 256);
        FEDD_TRY(c->d_st_part.ensure((size_t)grid * 4 + 1));
        if (vM.g == 16) hipLaunchKernelGGL(k_err_l2<16>, dim3(grid), dim3(256), 0, c->stream, vM, ua, ub, (int32_t)M->n_rows, c->d_st_part.p + 1);
        else hipLaunchKernelGGL(k_err_l2<8>, dim3(grid), dim3(256), 0, c->stream, vM, ua, ub, (int32_t)M->n_rows, c->d_st_part.p + 1);
    }
    hipLaunchKernelGGL(k_err_final, dim3(1), dim3(64), 0, c->stream, (const double*)(c->d_st_part.p + 1), (int64_t)grid * 4, c->d_st_part.p);
    FEDD_HIP(hipGetLastError());
    double sum = 0.0;
    FEDD_HIP(hipMemcpyAsync(&sum, c->d_st_part.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    *err = std::sqrt(sum);      // (on the host: correctly rounded)
    return 0;
}
