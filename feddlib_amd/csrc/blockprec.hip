// Block preconditioners of a merged 2 x 2 system (Stokes, Navier-Stokes), one rank.  gfx950 only.
//
// Replaces PrecBlock2x2::applyIt (feddlib/problems/Solver/PrecBlock2x2_def.hpp:114-164: "Diagonal" :135-143, "Triangular"
// :145-160) as built by Preconditioner::buildPreconditionerBlock2x2 (Preconditioner_def.hpp:979-1062): one Schwarz
// preconditioner V on the velocity block, one S on the Schur complement's stand-in -(1/nu) M_p, combined block-diagonally or
// block-upper-triangularly.  The reference's MinPrecProblem is a small problem of its own per block; here each block lives in a
// child fedd_ctx (a Schwarz preconditioner is a property of a context), filled by fedd_matrix_import, and the parent holds two
// pointers it does not own.
//
// One kernel of its own: k_bt_sub, t = r_u - B^T (scale * s) over the rectangular CSR of the stored B^T with the Dirichlet mask
// of the merged system and the scale of z_p fused in.  Its row sums are the lane-group row walk of stored_rows.hpp, as
// k_block_apply (timestep.hip) makes them, with x_j = scale * s[j] rounded before it is used.
// The normative operation order is in include/fedd_hip.h.
//
// The child link ("a child context applied as a block") that this preconditioner and FaCSI (fsi.hip) share is also here:
// attach, unlink, the destroy of a child, the ordering of a child's own stream, its apply in the parent's stream, and the
// checks both kinds make of a child.
#include "stored_rows.hpp"
#include <algorithm>
#include <cassert>

#pragma clang fp contract(off)

namespace fedd {
namespace {

// G lanes per row of B^T (rows < n_rows, columns < n_p by the shape check of block_prec_check).  s = S(r_p), unscaled.
//   x_j   = scale * s[j]                                 (rounded: the entry z_p[j] this kernel also stores)
//   acc   = sum_k val[k] * x_col[k]                      (the row walk; a Dirichlet row walks with len = 0)
//   t[i]  = isdir[i] ? r_u[i] : r_u[i] - acc
// The first n_p threads of the grid (grid-stride) write z_p = scale * s: s and z_p are different buffers, so no lane reads what
// another one writes.
template <int G>
__global__ __launch_bounds__(256) void k_bt_sub(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                const double* __restrict__ val, const double* __restrict__ s, double scale,
                                                const int32_t* __restrict__ isdir, const double* __restrict__ r_u, int32_t n_rows,
                                                int32_t n_p, double* __restrict__ t, double* __restrict__ z_p) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = tid; i < n_p; i += (int64_t)gridDim.x * blockDim.x) z_p[i] = scale * s[i];
    const int32_t row = (int32_t)(tid / G);
    const int g = (int)(tid % G);
    const bool live = row < n_rows;
    const bool dir = live ? isdir[row] != 0 : false;
    const int32_t st = live ? rowptr[row] : 0;
    const int32_t len = (live && !dir) ? rowptr[row + 1] - st : 0;
    const double acc = row_sum<G>(colind, val, st, len, g, [=](int32_t col) { return scale * s[col]; });
    if (live && g == 0) {
        const double ru = r_u[row];
        t[row] = dir ? ru : ru - acc;
    }
}

__global__ __launch_bounds__(256) void k_scale_vec(double* __restrict__ v, int64_t n, double a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = a * v[i];
}

const char* const BP = "block preconditioner";

int child_check(fedd_ctx* c, int which, int64_t n_expected, const char* who) {
    const fedd_ctx* ch = c->prec.child[which].ctx;
    const char* nm = which == 0 ? "velocity" : "Schur complement";
    FEDD_TRY(child_check_context(c, ch, who, BP, nm, "parent"));
    FEDD_CHECK(ch->have_pattern && !ch->merged, "%s: block preconditioner: the %s child holds no single-block system", who, nm);
    FEDD_CHECK(ch->n_rows == n_expected && ch->n_cols == n_expected,
               "%s: block preconditioner: wrong sizes: the %s child's system has %lld rows, the parent's block row %lld", who, nm,
               (long long)ch->n_rows, (long long)n_expected);
    return child_check_schwarz(ch, who, BP, nm, " (I - Pc A) M1^-1");
}

}  // namespace

// ---- the child link -------------------------------------------------------------------------------------------------------
int child_check_context(const fedd_ctx* c, const fedd_ctx* ch, const char* who, const char* label, const char* nm, const char* parent) {
    FEDD_CHECK(ch->device >= 0, "%s: %s: the %s child is a host-only context", who, label, nm);
    FEDD_CHECK(ch->nranks == 1, "%s: %s: one rank only (the %s child has %d ranks)", who, label, nm, ch->nranks);
    FEDD_CHECK(ch->device == c->device, "%s: %s: the %s child is on device %d, the %s on device %d", who, label, nm, ch->device, parent,
               c->device);
    return 0;
}

int child_check_schwarz(const fedd_ctx* ch, const char* who, const char* label, const char* nm, const char* mult_operator) {
    FEDD_CHECK(ch->have_schwarz, "%s: %s: the %s child has no current fedd_schwarz_setup (never set up, or its matrix changed since)", who,
               label, nm);
    FEDD_CHECK(ch->sw_levels != FEDD_LEVELS_MULTIPLICATIVE,
               "%s: %s: the %s child asks for FEDD_LEVELS_MULTIPLICATIVE, whose operator%s is singular and is not built as a block of a "
               "block preconditioner; use FEDD_LEVELS_ADDITIVE",
               who, label, nm, mult_operator);
    return 0;
}

// The child's kernels go into the parent's stream (child_apply): the applies and the parent's own kernels between them are then
// ordered by the stream itself, with no event and no host synchronisation inside the Krylov loop, and fedd_sync(parent) covers
// them.  What the child put into its OWN stream before (fedd_matrix_import, a merge, fedd_dirichlet, fedd_schwarz_setup) is
// ordered in front by an event: after every setup of the child, and whenever its stream is not idle.
int child_order(fedd_ctx* c, PrecChild& ch) {
    // (the query costs no device work; it covers whatever else may have gone into the child's stream since its setup)
    // Both children share the one event: a hipStreamWaitEvent captures the record made before it, so the next record does not
    // disturb a wait already enqueued.
    if (ch.seen == ch.ctx->sw_setup_gen) {
        const hipError_t q = hipStreamQuery(ch.ctx->stream);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) FEDD_HIP(q);     // a real error is reported, not cleared
        (void)hipGetLastError();                    // hipErrorNotReady is an answer, not a failure
    }
    if (!c->prec.ev) FEDD_HIP(hipEventCreateWithFlags(&c->prec.ev, hipEventDisableTiming));
    FEDD_HIP(hipEventRecord(c->prec.ev, ch.ctx->stream));
    FEDD_HIP(hipStreamWaitEvent(c->stream, c->prec.ev, 0));
    ch.seen = ch.ctx->sw_setup_gen;
    return 0;
}

int child_apply(fedd_ctx* c, fedd_ctx* ch, const double* r, double* z) {
    hipStream_t own = ch->stream;
    ch->stream = c->stream;
    const int rc = schwarz_apply(ch, r, z, false);
    ch->stream = own;
    return rc;
}

void prec_attach(fedd_ctx* c, int kind, fedd_ctx* first, fedd_ctx* second) {
    c->prec.kind = kind;
    c->prec.applies = 0;
    for (int i = 0; i < 2; ++i) {
        fedd_ctx* ch = i == 0 ? first : second;
        ch->prec_parents.push_back(c);
        c->prec.child[i] = {ch, ~(uint64_t)0};      // the first apply orders the children's streams in front
    }
}

void prec_unlink(fedd_ctx* c) {
    for (PrecChild& ch : c->prec.child) {
        if (ch.ctx) {       // c is a parent of ch once: one entry goes, those of ch's other parents stay
            auto it = std::find(ch.ctx->prec_parents.begin(), ch.ctx->prec_parents.end(), c);
            if (it != ch.ctx->prec_parents.end()) ch.ctx->prec_parents.erase(it);
        }
        ch = PrecChild();
    }
    c->prec.kind = AttachedPrec::NONE;
    c->bp_kind = 0;
    c->bp_slot_bt = -1;
    c->bp_scale = 1.0;
}

// The child's buffers may still be read by kernels in a parent's stream: each parent finishes them, then lets go of both children.
void prec_child_gone(fedd_ctx* child) {
    while (!child->prec_parents.empty()) {
        fedd_ctx* p = child->prec_parents.back();
        if (p->device >= 0 && hipSetDevice(p->device) == hipSuccess) (void)hipStreamSynchronize(p->stream);
        prec_unlink(p);     // erases p from child->prec_parents: p held the child as one of its two
        assert(child->prec_parents.empty() || child->prec_parents.back() != p);
    }
}

// ---- the block preconditioner ----------------------------------------------------------------------------------------------
int block_prec_check(fedd_ctx* c, const char* who) {
    FEDD_CHECK(c->prec.kind == AttachedPrec::BLOCK && (c->bp_kind == FEDD_BLOCKPREC_DIAGONAL || c->bp_kind == FEDD_BLOCKPREC_TRIANGULAR),
               "%s: no block preconditioner attached", who);
    FEDD_CHECK(c->nranks == 1, "%s: block preconditioner: one rank only (a context with %d ranks was given)", who, c->nranks);
    FEDD_CHECK(c->prec.child[0].ctx && c->prec.child[1].ctx, "%s: block preconditioner: null child", who);
    FEDD_CHECK(c->have_pattern && c->merged,
               "%s: block preconditioner: unmerged parent: the context does not hold a merged 2 x 2 system (fedd_block_merge first)", who);
    const int64_t nA = c->merged_nA, nP = c->n_rows - c->merged_nA;
    FEDD_TRY(child_check(c, 0, nA, who));
    FEDD_TRY(child_check(c, 1, nP, who));
    if (c->bp_kind == FEDD_BLOCKPREC_TRIANGULAR) {
        FEDD_CHECK(c->bp_slot_bt >= 0 && c->bp_slot_bt < MAX_AUX, "%s: block preconditioner: matrix slot %d out of range", who, c->bp_slot_bt);
        const DevCsr& bt = c->aux[c->bp_slot_bt];
        FEDD_CHECK(bt.valid, "%s: block preconditioner: slot %d (B^T of the Triangular form) is empty", who, c->bp_slot_bt);
        FEDD_CHECK(bt.n_rows == nA && bt.n_cols == nP,
                   "%s: block preconditioner: slot %d holds a %lld x %lld matrix, B^T of this system is %lld x %lld", who, c->bp_slot_bt,
                   (long long)bt.n_rows, (long long)bt.n_cols, (long long)nA, (long long)nP);
    }
    return 0;
}

int block_prec_apply(fedd_ctx* c, const double* r, double* z) {
    FEDD_TRY(block_prec_check(c, "block preconditioner apply"));
    fedd_ctx *V = c->prec.child[0].ctx, *S = c->prec.child[1].ctx;
    const int64_t nA = c->merged_nA, nP = c->n_rows - nA;
    FEDD_TRY(child_order(c, c->prec.child[0]));
    FEDD_TRY(child_order(c, c->prec.child[1]));
    ++c->prec.applies;
    const double* r_u = r;
    const double* r_p = r + nA;
    double* z_u = z;
    double* z_p = z + nA;
    if (c->bp_kind == FEDD_BLOCKPREC_DIAGONAL) {
        FEDD_TRY(child_apply(c, V, r_u, z_u));
        FEDD_TRY(child_apply(c, S, r_p, z_p));
        if (c->bp_scale != 1.0 && nP > 0)
            hipLaunchKernelGGL(k_scale_vec, dim3((unsigned)((nP + 255) / 256)), dim3(256), 0, c->stream, z_p, nP, c->bp_scale);
        FEDD_HIP(hipGetLastError());
        return 0;
    }
    const int64_t off_t = (nP + 1) & ~(int64_t)1;
    FEDD_TRY(c->d_bp_ws.ensure((size_t)(off_t + nA)));
    double* s = c->d_bp_ws.p;
    double* t = c->d_bp_ws.p + off_t;
    if (nA == 0) {      // no velocity rows: nothing to couple (and no launch of k_bt_sub, which would have written z_p)
        FEDD_TRY(child_apply(c, S, r_p, z_p));
        if (nP > 0) hipLaunchKernelGGL(k_scale_vec, dim3((unsigned)((nP + 255) / 256)), dim3(256), 0, c->stream, z_p, nP, c->bp_scale);
        FEDD_HIP(hipGetLastError());
        return 0;
    }
    FEDD_TRY(child_apply(c, S, r_p, s));
    {
        const DevCsr& bt = c->aux[c->bp_slot_bt];
        ScopedTimer tm(c, FEDD_T_BLOCKPREC_BT);
        // values and columns, row pointer, Dirichlet marks, r_u and t, s (read once from memory, then cache resident) and z_p
        tm.bytes(12.0 * (double)bt.nnz + 4.0 * (double)(nA + 1) + 4.0 * (double)nA + 16.0 * (double)nA + 16.0 * (double)nP);
        with_row_groups(bt.max_row_nnz, nA, [&](auto G, unsigned grid) {
            hipLaunchKernelGGL(k_bt_sub<decltype(G)::value>, dim3(grid), dim3(256), 0, c->stream, (const int32_t*)bt.rowptr.p,
                               (const int32_t*)bt.colind.p, (const double*)bt.val.p, (const double*)s, c->bp_scale,
                               (const int32_t*)c->d_isdir.p, r_u, (int32_t)nA, (int32_t)nP, t, z_p);
            return 0;
        });
        tm.stop();
        FEDD_HIP(hipGetLastError());
    }
    return child_apply(c, V, t, z_u);
}

}  // namespace fedd

using namespace fedd;

extern "C" int fedd_matrix_import(fedd_ctx* dst, fedd_ctx* src, int src_slot) {
    FEDD_CHECK(dst && src, "fedd_matrix_import: null context");
    FEDD_CHECK(dst != src, "fedd_matrix_import: source and destination are the same context (fedd_matrix_combine copies a slot into its own system)");
    FEDD_CHECK(dst->nranks == 1 && src->nranks == 1, "fedd_matrix_import: one rank only (contexts with %d and %d ranks were given)",
               dst->nranks, src->nranks);
    FEDD_CHECK(dst->device >= 0 && src->device >= 0,
               "fedd_matrix_import: this call needs a GPU context on both sides (%s is host-only); there is no CPU fallback",
               dst->device < 0 ? "the destination" : "the source");
    FEDD_CHECK(dst->device == src->device, "fedd_matrix_import: contexts on different devices (%d and %d)", dst->device, src->device);
    FEDD_CHECK(src_slot >= 0 && src_slot < MAX_AUX, "matrix slot %d out of range", src_slot);
    const DevCsr& m = src->aux[src_slot];
    FEDD_CHECK(m.valid, "fedd_matrix_import: slot %d of the source is empty", src_slot);
    FEDD_CHECK(m.n_rows == m.n_cols, "fedd_matrix_import: slot %d holds a non-square block (%lld x %lld)", src_slot, (long long)m.n_rows,
               (long long)m.n_cols);
    FEDD_CHECK(dst->n_node > 0, "fedd_matrix_import: the destination carries no mesh (fedd_mesh_set first)");
    FEDD_CHECK(dst->n_rowg == 0 && dst->n_node == dst->n_own, "fedd_matrix_import: the destination's mesh has ghost nodes: it belongs to several ranks");
    const int64_t dofs = dst->n_own > 0 ? m.n_rows / dst->n_own : 0;
    FEDD_CHECK(dofs >= 1 && dofs <= MAX_DOFS && dofs * dst->n_own == m.n_rows,
               "fedd_matrix_import: size mismatch: the block has %lld rows, the destination's mesh %lld owned nodes (1 to %d dofs per node)",
               (long long)m.n_rows, (long long)dst->n_own, MAX_DOFS);
    FEDD_CHECK(m.n_rows < ((int64_t)1 << 31) && m.nnz < ((int64_t)1 << 31), "fedd_matrix_import: block too large for 32-bit local offsets");
    FEDD_CHECK(m.max_row_nnz > 0 || m.nnz == 0, "fedd_matrix_import: slot %d does not know its longest row", src_slot);
    FEDD_HIP(hipSetDevice(dst->device));
    fedd_ctx* c = dst;
    const size_t n = (size_t)m.n_rows;
    // the block was written in the source's stream; the copies run in the destination's
    hipEvent_t ev = nullptr;
    FEDD_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e1 = hipEventRecord(ev, src->stream);
    hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(c->stream, ev, 0) : e1;
    if (e2 != hipSuccess) {
        (void)hipEventDestroy(ev);
        FEDD_HIP(e2);
    }
    const bool values_only = c->have_pattern && !c->merged && c->imp_src_uid == src->uid && c->imp_mesh_id == m.mesh_id &&
                             c->imp_pattern_id == m.pattern_id && m.pattern_id != 0 && c->imp_pattern_gen == c->pattern_gen &&
                             c->n_rows == m.n_rows && c->nnz == m.nnz;
    system_written(c, values_only ? SYS_VALUES : SYS_VALUES | SYS_PATTERN);
    int rc = 0;
    auto body = [&]() -> int {
        if (!values_only) {
            // (the system slot then holds the pattern of none of this context's own slots: pattern id 0)
            FEDD_TRY(system_adopt_pattern(c, m, (int)dofs, m.block_mode >= 0 ? m.block_mode : (dofs == 1 ? FEDD_BLOCK_SCALAR : FEDD_BLOCK_FULL),
                                          n, false, 0));
        }
        FEDD_HIP(hipMemcpyAsync(c->d_val.p, m.val.p, (size_t)m.nnz * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        // reset as by a merge
        FEDD_HIP(hipMemsetAsync(c->d_rhs.p, 0, n * sizeof(double), c->stream));
        FEDD_HIP(hipMemsetAsync(c->d_x.p, 0, n * sizeof(double), c->stream));
        FEDD_HIP(hipMemsetAsync(c->d_isdir.p, 0, n * sizeof(int32_t), c->stream));
        // a later writer of the slot, in the source's stream, waits for the copies
        FEDD_HIP(hipEventRecord(ev, c->stream));
        FEDD_HIP(hipStreamWaitEvent(src->stream, ev, 0));
        return 0;
    };
    rc = body();
    (void)hipEventDestroy(ev);
    if (rc) return rc;
    c->have_pattern = true;
    c->imp_src_uid = src->uid;
    c->imp_mesh_id = m.mesh_id;
    c->imp_pattern_id = m.pattern_id;
    c->imp_pattern_gen = c->pattern_gen;
    return 0;
}

extern "C" int fedd_block_prec_attach(fedd_ctx* c, int kind, fedd_ctx* velocity, fedd_ctx* schur, double schur_scale, int slot_bt) {
    FEDD_CHECK(c, "fedd_block_prec_attach: null context");
    FEDD_CHECK(velocity, "fedd_block_prec_attach: null child: the velocity context is NULL");
    FEDD_CHECK(schur, "fedd_block_prec_attach: null child: the Schur complement context is NULL");
    FEDD_CHECK(velocity != c && schur != c && velocity != schur, "fedd_block_prec_attach: parent and children must be three different contexts");
    FEDD_CHECK(kind == FEDD_BLOCKPREC_DIAGONAL || kind == FEDD_BLOCKPREC_TRIANGULAR,
               "fedd_block_prec_attach: kind %d (FEDD_BLOCKPREC_DIAGONAL = %d, FEDD_BLOCKPREC_TRIANGULAR = %d)", kind,
               FEDD_BLOCKPREC_DIAGONAL, FEDD_BLOCKPREC_TRIANGULAR);
    FEDD_CHECK(c->nranks == 1 && velocity->nranks == 1 && schur->nranks == 1,
               "fedd_block_prec_attach: one rank only (contexts with %d, %d and %d ranks were given)", c->nranks, velocity->nranks,
               schur->nranks);
    FEDD_CHECK(schur_scale != 0.0 && schur_scale == schur_scale, "fedd_block_prec_attach: schur_scale must be a nonzero number (got %g)", schur_scale);
    FEDD_CHECK(kind != FEDD_BLOCKPREC_TRIANGULAR || (slot_bt >= 0 && slot_bt < MAX_AUX), "matrix slot %d out of range", slot_bt);
    // the velocity child carries the parent's mesh (block row 0 lives on it), the Schur child the pressure nodes, a subset
    FEDD_CHECK(velocity->n_own == c->n_own,
               "fedd_block_prec_attach: wrong sizes: the velocity child's mesh has %lld owned nodes, the parent's %lld",
               (long long)velocity->n_own, (long long)c->n_own);
    FEDD_CHECK(schur->n_own <= c->n_own,
               "fedd_block_prec_attach: wrong sizes: the Schur complement child's mesh has %lld owned nodes, more than the parent's %lld",
               (long long)schur->n_own, (long long)c->n_own);
    FEDD_CHECK(c->have_pattern && c->merged,
               "fedd_block_prec_attach: unmerged parent: the context does not hold a merged 2 x 2 system (fedd_block_merge first)");
    FEDD_CHECK(velocity->device == c->device && schur->device == c->device,
               "fedd_block_prec_attach: contexts on different devices (parent %d, velocity %d, Schur complement %d)", c->device,
               velocity->device, schur->device);
    prec_unlink(c);             // (an earlier attach, of either kind)
    prec_attach(c, AttachedPrec::BLOCK, velocity, schur);
    c->bp_kind = kind;
    c->bp_scale = schur_scale;
    c->bp_slot_bt = kind == FEDD_BLOCKPREC_TRIANGULAR ? slot_bt : -1;
    return 0;
}

extern "C" int fedd_block_prec_detach(fedd_ctx* c) {
    FEDD_CHECK(c, "fedd_block_prec_detach: null context");
    if (c->bp_kind && c->device >= 0) {     // the children's kernels run in this context's stream: let them finish
        FEDD_HIP(hipSetDevice(c->device));
        FEDD_HIP(hipStreamSynchronize(c->stream));
    }
    if (c->bp_kind) prec_unlink(c);
    return 0;
}

extern "C" int fedd_block_prec_info(fedd_ctx* c, int* kind, double* schur_scale, int* slot_bt, int64_t* n_applies) {
    FEDD_CHECK(c, "fedd_block_prec_info: null context");
    if (kind) *kind = c->bp_kind;
    if (schur_scale) *schur_scale = c->bp_scale;
    if (slot_bt) *slot_bt = c->bp_slot_bt;
    if (n_applies) *n_applies = c->bp_kind ? c->prec.applies : 0;
    return 0;
}
