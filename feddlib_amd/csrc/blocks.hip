// Block systems on the device: stored blocks and their merge into one monolithic CSR matrix.
//
// Replaces BlockMatrix::merge / mergeBlockNew and BlockMap::merge
// (feddlib/core/LinearAlgebra/BlockMatrix_def.hpp:119-148, 212-287; BlockMap_def.hpp:55-80), which
// re-insert every row of every block into a new Tpetra matrix with the global ids of block k
// shifted by the cumulated (maxAllGlobalIndex + 1) of the blocks before it.  Here: row counts ->
// scan -> one fill kernel; column ids of the second block column are shifted by the first block's
// column count, so concatenated rows stay sorted.
// Layout of the 2 x 2 system (Stokes_def.hpp:47-138):  [ A  B^T ; B  C ],  C optional.
#include "fedd_internal.hpp"
#include <algorithm>

namespace fedd {
namespace {

__global__ void k_scale(double* __restrict__ v, int64_t n, double a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] *= a;
}

struct CsrView {
    const int32_t* rowptr;
    const int32_t* colind;
    const double* val;
};

__global__ void k_merge_count(CsrView A, CsrView BT, CsrView B, CsrView C, int32_t nA, int32_t nB,
                              int32_t* __restrict__ cnt) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nA + nB) return;
    int32_t n = 0;
    if (r < nA) {
        n = A.rowptr[r + 1] - A.rowptr[r];
        if (BT.rowptr) n += BT.rowptr[r + 1] - BT.rowptr[r];
    } else {
        const int32_t i = r - nA;
        if (B.rowptr) n += B.rowptr[i + 1] - B.rowptr[i];
        if (C.rowptr) n += C.rowptr[i + 1] - C.rowptr[i];
    }
    cnt[r] = n;
}

// SCALED (fedd_block_merge_scaled): the values of B^T, the second block column of the rows below nA, are multiplied by s_bt, one
// product per entry; the unscaled instance is the code fedd_block_merge has always run
template <bool SCALED>
__global__ void k_merge_fill(CsrView A, CsrView BT, CsrView B, CsrView C, int32_t nA, int32_t nB, int32_t col_off,
                             const int32_t* __restrict__ rowptr, int32_t* __restrict__ colind,
                             double* __restrict__ val, double s_bt) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nA + nB) return;
    int32_t p = rowptr[r];
    const CsrView& L = r < nA ? A : B;   // block in the first block column
    const CsrView& R = r < nA ? BT : C;  // block in the second block column
    const int32_t i = r < nA ? r : r - nA;
    if (L.rowptr)
        for (int32_t q = L.rowptr[i]; q < L.rowptr[i + 1]; ++q, ++p) {
            colind[p] = L.colind[q];
            val[p] = L.val[q];
        }
    if (R.rowptr)
        for (int32_t q = R.rowptr[i]; q < R.rowptr[i + 1]; ++q, ++p) {
            colind[p] = R.colind[q] + col_off;
            val[p] = SCALED && r < nA ? s_bt * R.val[q] : R.val[q];
        }
}

// the same rows with the pattern already in place: values only
template <bool SCALED>
__global__ void k_merge_values(CsrView A, CsrView BT, CsrView B, CsrView C, int32_t nA, int32_t nB,
                               const int32_t* __restrict__ rowptr, double* __restrict__ val, double s_bt) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nA + nB) return;
    int32_t p = rowptr[r];
    const CsrView& L = r < nA ? A : B;
    const CsrView& R = r < nA ? BT : C;
    const int32_t i = r < nA ? r : r - nA;
    if (L.rowptr)
        for (int32_t q = L.rowptr[i]; q < L.rowptr[i + 1]; ++q, ++p) val[p] = L.val[q];
    if (R.rowptr)
        for (int32_t q = R.rowptr[i]; q < R.rowptr[i + 1]; ++q, ++p) val[p] = SCALED && r < nA ? s_bt * R.val[q] : R.val[q];
}

__global__ void k_dof_node(int32_t nA, int32_t nB, int dofsA, int32_t* __restrict__ dof_node) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nA + nB) return;
    dof_node[r] = r < nA ? r / dofsA : r - nA;  // pressure dof i sits on vertex node i (P1 nodes come first)
}

CsrView view(const DevCsr* m) {
    CsrView v{nullptr, nullptr, nullptr};
    if (m && m->valid) {
        v.rowptr = m->rowptr.p;
        v.colind = m->colind.p;
        v.val = m->val.p;
    }
    return v;
}

int merge_blocks(fedd_ctx* c, int slot_a, int slot_bt, int slot_b, int slot_c, bool scaled, double s_bt);

}  // namespace

int matrix_store(fedd_ctx* c, int slot) {
    DevCsr& m = c->aux[slot];
    FEDD_TRY(m.rowptr.ensure((size_t)c->n_rows + 1));
    FEDD_TRY(m.colind.ensure((size_t)c->nnz));
    FEDD_TRY(m.val.ensure((size_t)c->nnz));
    FEDD_HIP(hipMemcpyAsync(m.rowptr.p, c->d_rowptr.p, ((size_t)c->n_rows + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    FEDD_HIP(hipMemcpyAsync(m.colind.p, c->d_colind.p, (size_t)c->nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    FEDD_HIP(hipMemcpyAsync(m.val.p, c->d_val.p, (size_t)c->nnz * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    m.n_rows = c->n_rows;
    m.n_cols = c->n_cols;
    m.nnz = c->nnz;
    m.max_row_nnz = c->max_row_nnz;
    m.valid = true;
    m.pattern_id = ++c->pattern_counter;
    m.value_id = ++c->value_counter;
    c->sys_pattern_id = m.pattern_id;       // the system slot and this slot now hold the same pattern (timestep.hip)
    c->sys_pattern_gen = c->pattern_gen;
    m.dofs = c->dofs;
    m.block_mode = c->merged ? -1 : c->block_mode;
    m.mesh_id = c->mesh_id;
    return 0;
}

int matrix_scale(fedd_ctx* c, int slot, double alpha) {
    if (slot < 0) system_written(c, SYS_VALUES);
    double* v = slot < 0 ? c->d_val.p : c->aux[slot].val.p;
    const int64_t n = slot < 0 ? c->nnz : c->aux[slot].nnz;
    if (n > 0) hipLaunchKernelGGL(k_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, v, n, alpha);
    FEDD_HIP(hipGetLastError());
    if (slot >= 0) c->aux[slot].value_id = ++c->value_counter;
    return 0;
}

int block_merge(fedd_ctx* c, int slot_a, int slot_bt, int slot_b, int slot_c) {
    return merge_blocks(c, slot_a, slot_bt, slot_b, slot_c, false, 1.0);
}

int block_merge_scaled(fedd_ctx* c, int slot_a, int slot_bt, double s_bt, int slot_b, int slot_c) {
    return merge_blocks(c, slot_a, slot_bt, slot_b, slot_c, true, s_bt);
}

namespace {

int merge_blocks(fedd_ctx* c, int slot_a, int slot_bt, int slot_b, int slot_c, bool scaled, double s_bt) {
    FEDD_CHECK(c->nranks == 1, "block merge: one rank only for now");
    const DevCsr* A = &c->aux[slot_a];
    const DevCsr* BT = slot_bt >= 0 ? &c->aux[slot_bt] : nullptr;
    const DevCsr* B = slot_b >= 0 ? &c->aux[slot_b] : nullptr;
    const DevCsr* C = slot_c >= 0 ? &c->aux[slot_c] : nullptr;
    FEDD_CHECK(A->valid, "block merge: block (0,0) is empty");
    FEDD_CHECK((B && B->valid) || (BT && BT->valid), "block merge: needs at least one off-diagonal block");
    const int64_t nA = A->n_rows;
    const int64_t nB = B && B->valid ? B->n_rows : BT->n_cols;
    FEDD_CHECK(!BT || !BT->valid || (BT->n_rows == nA && BT->n_cols == nB), "block merge: B^T has the wrong shape");
    FEDD_CHECK(!B || !B->valid || B->n_cols == A->n_cols, "block merge: B has the wrong shape");
    FEDD_CHECK(!C || !C->valid || (C->n_rows == nB && C->n_cols == nB), "block merge: C has the wrong shape");
    const int64_t n = nA + nB;
    FEDD_CHECK(n < ((int64_t)1 << 31), "block merge: too many rows");
    const int dofsA = (int)(nA / std::max<int64_t>(1, c->n_own));
    const CsrView vA = view(A), vBT = view(BT), vB = view(B), vC = view(C);
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    // The blocks of a nonlinear iteration change their values, not their patterns: when the system matrix still is the merge of
    // these slots and none of their patterns has been rewritten since, the merged pattern stands and only values move.
    const int slots[4] = {slot_a, slot_bt, slot_b, slot_c};
    const DevCsr* blocks[4] = {A, BT, B, C};
    bool same = c->merged && c->n_rows == n;
    for (int k = 0; k < 4; ++k) {
        const uint64_t id = blocks[k] && blocks[k]->valid ? blocks[k]->pattern_id : 0;
        same = same && c->merge_slots[k] == slots[k] && c->merge_ids[k] == id && (id != 0 || !(blocks[k] && blocks[k]->valid));
    }
    // (a merge that only moves values declares the pattern written too: a missed reuse is cheap, a wrong one is not.  The scaled
    // merge of a stage loop, which changes s_bt from stage to stage, says what it wrote: values, and the pattern generation stands)
    system_written(c, scaled && same ? SYS_VALUES : SYS_VALUES | SYS_PATTERN);
    if (same) {
        if (scaled)
            hipLaunchKernelGGL(k_merge_values<true>, grid, blk, 0, c->stream, vA, vBT, vB, vC, (int32_t)nA, (int32_t)nB,
                               (const int32_t*)c->d_rowptr.p, c->d_val.p, s_bt);
        else
            hipLaunchKernelGGL(k_merge_values<false>, grid, blk, 0, c->stream, vA, vBT, vB, vC, (int32_t)nA, (int32_t)nB,
                               (const int32_t*)c->d_rowptr.p, c->d_val.p, 1.0);
        FEDD_HIP(hipMemsetAsync(c->d_rhs.p, 0, (size_t)n * sizeof(double), c->stream));
        FEDD_HIP(hipMemsetAsync(c->d_x.p, 0, (size_t)n * sizeof(double), c->stream));
        FEDD_HIP(hipMemsetAsync(c->d_isdir.p, 0, (size_t)n * sizeof(int32_t), c->stream));
        FEDD_HIP(hipGetLastError());
        c->have_pattern = true;
        return 0;
    }
    c->merged = false;      // until this merge has completed, the system matrix is not the merge of anything
    FEDD_TRY(c->d_rowptr.ensure((size_t)n + 1));
    hipLaunchKernelGGL(k_merge_count, grid, blk, 0, c->stream, vA, vBT, vB, vC, (int32_t)nA, (int32_t)nB, c->d_rowptr.p);
    int32_t mx = 0;
    FEDD_TRY(reduce_max_i32(c, c->d_rowptr.p, n, &mx));
    int64_t nnz = 0;
    FEDD_TRY(exclusive_scan_i32(c, c->d_rowptr.p, c->d_rowptr.p, n, &nnz));
    FEDD_TRY(c->d_colind.ensure((size_t)nnz));
    FEDD_TRY(c->d_val.ensure((size_t)nnz));
    if (scaled)
        hipLaunchKernelGGL(k_merge_fill<true>, grid, blk, 0, c->stream, vA, vBT, vB, vC, (int32_t)nA, (int32_t)nB, (int32_t)A->n_cols,
                           (const int32_t*)c->d_rowptr.p, c->d_colind.p, c->d_val.p, s_bt);
    else
        hipLaunchKernelGGL(k_merge_fill<false>, grid, blk, 0, c->stream, vA, vBT, vB, vC, (int32_t)nA, (int32_t)nB, (int32_t)A->n_cols,
                           (const int32_t*)c->d_rowptr.p, c->d_colind.p, c->d_val.p, 1.0);
    FEDD_TRY(c->d_dof_node.ensure((size_t)n));
    hipLaunchKernelGGL(k_dof_node, grid, blk, 0, c->stream, (int32_t)nA, (int32_t)nB, dofsA, c->d_dof_node.p);
    c->n_rows = n;
    c->n_rows_ext = n;
    c->n_cols = n;
    c->nnz = nnz;
    c->nnz_ext = nnz;
    c->max_row_nnz = mx;
    c->merged_nA = nA;
    c->merged_dofsA = dofsA;
    c->dofs = 1;
    c->block_mode = FEDD_BLOCK_SCALAR;
    FEDD_TRY(c->d_rhs.ensure((size_t)n));
    FEDD_TRY(c->d_x.ensure((size_t)n));
    FEDD_TRY(c->d_xcol.ensure((size_t)n));
    FEDD_TRY(c->d_isdir.ensure((size_t)n));
    FEDD_HIP(hipMemsetAsync(c->d_rhs.p, 0, (size_t)n * sizeof(double), c->stream));
    FEDD_HIP(hipMemsetAsync(c->d_x.p, 0, (size_t)n * sizeof(double), c->stream));
    FEDD_HIP(hipMemsetAsync(c->d_isdir.p, 0, (size_t)n * sizeof(int32_t), c->stream));
    FEDD_HIP(hipGetLastError());
    c->have_pattern = true;
    // recorded last: a merge that failed on the way leaves merged = false, and the next one builds the pattern again
    c->merged = true;
    for (int k = 0; k < 4; ++k) {
        c->merge_slots[k] = slots[k];
        c->merge_ids[k] = blocks[k] && blocks[k]->valid ? blocks[k]->pattern_id : 0;
    }
    return 0;
}

}  // namespace

}  // namespace fedd
