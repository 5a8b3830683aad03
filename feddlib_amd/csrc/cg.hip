// Preconditioned conjugate gradients for systems that are symmetric positive definite on their free dofs (Laplace, linear
// elasticity): Belos CG with block size 1.  The normative algorithm is stated at fedd_cg in include/fedd_hip.h.
//
// Vectors: x, r, z, p, q (5 n doubles).  Per iteration: q = A p (spmv.hip), k_cg_pq (partials of p.q), k_cg_scalars (alpha),
// k_cg_xr (x += alpha p, r -= alpha q, partials of r.r), k_cg_scalars (convergence test), z = M^-1 r (schwarz_sym.hip + coarse
// level), k_cg_rz (partials of r.z), k_cg_scalars (beta), k_cg_p (p = mask (z + beta p)).  Sweep traffic per row:
// 16 + 48 + 16 + 24 + 4 (mask) bytes.  The partial sums of the dot products sit in fixed slots (one per workgroup, every
// workgroup walks its rows in a fixed order) and one workgroup adds them in slot order: no floating-point atomics, the same
// bits in every run.
//
// alpha, beta and the convergence test stay on the device.  When the test is met (or a breakdown is seen) k_cg_scalars sets a
// `done` word; every CG kernel queued behind it reads that word first and returns at once, so x, r, p and the scalars are those
// of the iterate that met the test (operator and preconditioner kernels of iterations queued past it still run: they write q
// and z only).  The host never waits inside an iteration: it reads the words of iteration j - CG_LAG from mapped pinned
// memory (the mechanism of option "gmres_hostwrite") while later iterations are already queued.
#include "fedd_internal.hpp"

#include <algorithm>
#include <cmath>

namespace fedd {
namespace {

constexpr int CG_MAXBLK = 1024;     // slots of a dot product
constexpr int CG_LAG = 3;           // iterations the host's view trails the queue by
// scalars on the device
enum { S_RHO = 0, S_ALPHA = 1, S_BETA = 2, S_PQ = 3, S_RR = 4, S_TOL2 = 5, S_DONE = 8, S_BRK = 9, S_ITS = 10, S_CONV = 11, S_COUNT = 16 };

__device__ __forceinline__ void cg_block_sum(double v, double* __restrict__ slot) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) *slot = red[0];
}

// partials of p.q
__global__ __launch_bounds__(256) void k_cg_pq(const double* __restrict__ p, const double* __restrict__ q, int64_t n,
                                               const double* __restrict__ S, double* __restrict__ part) {
    if (S[S_DONE] != 0.0) return;
    const int64_t stride = (int64_t)gridDim.x * 256;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) acc += p[i] * q[i];
    cg_block_sum(acc, part + blockIdx.x);
}

// x += alpha p, r -= alpha q, partials of r.r
__global__ __launch_bounds__(256) void k_cg_xr(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                               const double* __restrict__ q, int64_t n, const double* __restrict__ S,
                                               double* __restrict__ part) {
    if (S[S_DONE] != 0.0) return;
    const double alpha = S[S_ALPHA];
    const int64_t stride = (int64_t)gridDim.x * 256;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * q[i];
        r[i] = ri;
        acc += ri * ri;
    }
    cg_block_sum(acc, part + blockIdx.x);
}

// partials of r.z
__global__ __launch_bounds__(256) void k_cg_rz(const double* __restrict__ r, const double* __restrict__ z, int64_t n,
                                               const double* __restrict__ S, double* __restrict__ part) {
    if (S[S_DONE] != 0.0) return;
    const int64_t stride = (int64_t)gridDim.x * 256;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) acc += r[i] * z[i];
    cg_block_sum(acc, part + blockIdx.x);
}

// p = mask (z + beta p): the Dirichlet rows stay 0 whatever the preconditioner leaves there
__global__ __launch_bounds__(256) void k_cg_p(double* __restrict__ p, const double* __restrict__ z, const int32_t* __restrict__ isdir,
                                              int64_t n, const double* __restrict__ S) {
    if (S[S_DONE] != 0.0) return;
    const double beta = S[S_BETA];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = isdir[i] ? 0.0 : z[i] + beta * p[i];
}

// the small algebra: one workgroup adds the partials in slot order and forms alpha / beta / the convergence test.
// mode 0: p.q -> alpha;  1: r.r -> iteration count and convergence test;  2: r.z -> beta, rho;  3: r.z of a (re)start -> rho
// hostw != nullptr: the words the host reads (iterations, done, breakdown, r.r) go to mapped pinned memory
__global__ __launch_bounds__(256) void k_cg_scalars(double* __restrict__ S, const double* __restrict__ part, int nblk, int mode,
                                                    double* __restrict__ hostw) {
    __shared__ double sp[CG_MAXBLK];
    const bool done = S[S_DONE] != 0.0;
    if (!done) {
        for (int i = threadIdx.x; i < nblk; i += 256) sp[i] = part[i];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (!done) {
        double sum = 0.0;
        for (int i = 0; i < nblk; ++i) sum += sp[i];
        const bool finite = sum - sum == 0.0;
        if (mode == 0) {
            S[S_PQ] = sum;
            if (!finite || !(sum > 0.0)) {
                S[S_BRK] = finite ? (double)FEDD_CG_BREAKDOWN_PQ : (double)FEDD_CG_BREAKDOWN_NONFINITE;
                S[S_DONE] = 1.0;
            } else {
                S[S_ALPHA] = S[S_RHO] / sum;
            }
        } else if (mode == 1) {
            S[S_RR] = sum;
            S[S_ITS] += 1.0;
            if (!finite) {
                S[S_BRK] = (double)FEDD_CG_BREAKDOWN_NONFINITE;
                S[S_DONE] = 1.0;
            } else if (sum <= S[S_TOL2]) {
                S[S_CONV] = 1.0;
                S[S_DONE] = 1.0;
            }
        } else {
            if (!finite || !(sum > 0.0)) {
                S[S_BRK] = finite ? (double)FEDD_CG_BREAKDOWN_RHO : (double)FEDD_CG_BREAKDOWN_NONFINITE;
                S[S_DONE] = 1.0;
            } else {
                S[S_BETA] = mode == 2 ? sum / S[S_RHO] : 0.0;
                S[S_RHO] = sum;
            }
        }
    }
    if (hostw && mode == 1) {
        hostw[0] = S[S_ITS];
        hostw[1] = S[S_DONE];
        hostw[2] = S[S_BRK];
        hostw[3] = S[S_RR];
    }
}

// Dirichlet lift: x[d] = b[d] on the identity rows
__global__ void k_cg_lift(double* __restrict__ x, const double* __restrict__ b, const int32_t* __restrict__ isdir, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && isdir[i]) x[i] = b[i];
}

// r = b - ax, partials of r.r and of ax.ax
__global__ __launch_bounds__(256) void k_cg_resid(const double* __restrict__ b, const double* __restrict__ ax, double* __restrict__ r,
                                                  int64_t n, double* __restrict__ part_rr, double* __restrict__ part_aa) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    double acc = 0.0, aa = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const double a = ax[i], ri = b[i] - a;
        r[i] = ri;
        acc += ri * ri;
        aa += a * a;
    }
    cg_block_sum(acc, part_rr + blockIdx.x);
    __syncthreads();
    cg_block_sum(aa, part_aa + blockIdx.x);
}

// out[0] = sum of part_a, out[1] = sum of part_b, in slot order
__global__ void k_cg_sum2(const double* __restrict__ part_a, const double* __restrict__ part_b, int nblk, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a = 0.0, b = 0.0;
    for (int i = 0; i < nblk; ++i) {
        a += part_a[i];
        b += part_b[i];
    }
    out[0] = a;
    out[1] = b;
}

__global__ void k_cg_set(double* __restrict__ S, int i, double v) { S[i] = v; }

const char* breakdown_name(int w) {
    switch (w) {
    case FEDD_CG_BREAKDOWN_PQ: return "p.Ap <= 0";
    case FEDD_CG_BREAKDOWN_RHO: return "r.z <= 0";
    case FEDD_CG_BREAKDOWN_NONFINITE: return "non-finite value";
    case FEDD_CG_BREAKDOWN_NONSYMMETRIC: return "operator not symmetric";
    default: return "none";
    }
}

}  // namespace

int cg_solve(fedd_ctx* c, const CgCall& call, int* its_out, double* relres_out) {
    const int64_t n = c->n_rows;
    const int64_t nv = (n + 15) & ~(int64_t)15;
    const int nblk = (int)std::min<int64_t>(CG_MAXBLK, std::max<int64_t>(1, (n + 1023) / 1024));
    hipStream_t st = c->stream;
    const dim3 blk(256), gn((unsigned)((n + 255) / 256)), gb((unsigned)nblk);
    c->cg_replacements = 0;
    c->cg_breakdown = 0;
    FEDD_TRY(c->d_cg.ensure((size_t)(4 * nv + 4 * CG_MAXBLK + S_COUNT + 16)));
    double* r = c->d_cg.p;
    double* z = r + nv;
    double* p = z + nv;
    double* q = p + nv;
    double* part = q + nv;                  // p.q | r.r | r.z | scratch, CG_MAXBLK slots each
    double* part_rr = part + CG_MAXBLK;
    double* part_rz = part + 2 * CG_MAXBLK;
    double* part_x = part + 3 * CG_MAXBLK;
    double* S = part + 4 * CG_MAXBLK;
    double* x = call.x;
    const double* b = call.b;
    const int32_t* isdir = c->d_isdir.p;
    double* hp = c->h_pinned;
    // the park + gather kernels whatever "apply_gather" says; put back on every way out
    struct Force {
        fedd_ctx* c;
        explicit Force(fedd_ctx* ctx) : c(ctx) { c->sym_force = true; }
        ~Force() { c->sym_force = false; }
    } force(c);

    auto read2 = [&](const double* pa, const double* pb, double* a_out, double* b_out) -> int {
        hipLaunchKernelGGL(k_cg_sum2, dim3(1), dim3(64), 0, st, pa, pb, nblk, S + 12);
        FEDD_HIP(hipMemcpyAsync(hp + 32, S + 12, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        FEDD_HIP(hipStreamSynchronize(st));
        *a_out = hp[32];
        *b_out = hp[33];
        return 0;
    };
    // r = b - A x with the product fedd_gmres checks its residual with; ||r||^2 and ||A x||^2 on the host
    auto true_residual = [&](double* rr_out, double* aa_out) -> int {
        FEDD_TRY(spmv_owned(c, x, q, false, nullptr, 0.0, -1));
        hipLaunchKernelGGL(k_cg_resid, gb, blk, 0, st, b, (const double*)q, r, n, part_rr, part_x);
        return read2(part_rr, part_x, rr_out, aa_out);
    };
    // z = M^-1 r, p = mask z, rho = r.z  (start and residual replacement)
    auto restart_direction = [&]() -> int {
        if (call.use_prec) FEDD_TRY(schwarz_apply(c, r, z, false));
        FEDD_HIP(hipMemsetAsync(p, 0, (size_t)n * sizeof(double), st));
        hipLaunchKernelGGL(k_cg_rz, gb, blk, 0, st, (const double*)r, (const double*)(call.use_prec ? z : r), n, (const double*)S, part_rz);
        hipLaunchKernelGGL(k_cg_scalars, dim3(1), blk, 0, st, S, (const double*)part_rz, nblk, 3, (double*)nullptr);
        hipLaunchKernelGGL(k_cg_p, gn, blk, 0, st, p, (const double*)(call.use_prec ? z : r), isdir, n, (const double*)S);
        return 0;
    };

    FEDD_HIP(hipMemsetAsync(S, 0, S_COUNT * sizeof(double), st));
    // 1. den = ||b - A x_0|| for the caller's x_0
    double den2 = 0.0, aa = 0.0, bb = 0.0;
    if (call.x0) {
        FEDD_TRY(true_residual(&den2, &aa));
    } else {
        FEDD_HIP(hipMemsetAsync(x, 0, (size_t)n * sizeof(double), st));
        FEDD_HIP(hipMemsetAsync(q, 0, (size_t)n * sizeof(double), st));
        hipLaunchKernelGGL(k_cg_resid, gb, blk, 0, st, b, (const double*)q, r, n, part_rr, part_x);
        FEDD_TRY(read2(part_rr, part_x, &den2, &aa));
    }
    const double den = std::sqrt(std::max(den2, 0.0));
    if (its_out) *its_out = 0;
    if (relres_out) *relres_out = 0.0;
    if (!(den > 0.0)) {     // nothing to solve
        FEDD_CHECK(den == 0.0, "fedd_cg: the right-hand side or the initial guess holds a non-finite value");
        return 0;
    }
    if (call.x0) {
        // an initial guess at the rounding floor of b - A x_0 (||r_0|| <= 1e-13 (||b|| + ||A x_0||), the smallest tolerance the
        // project tests at): its residual is rounding noise of the product, there is no direction to gain from it
        hipLaunchKernelGGL(k_cg_rz, gb, blk, 0, st, b, b, n, (const double*)S, part_x);
        double dummy = 0.0;
        FEDD_TRY(read2(part_x, part_x, &bb, &dummy));
        if (den <= 1e-13 * (std::sqrt(bb) + std::sqrt(aa))) {
            if (relres_out) *relres_out = 1.0;
            return 0;
        }
    }
    // 2. Dirichlet lift, 3. start
    hipLaunchKernelGGL(k_cg_lift, gn, blk, 0, st, x, b, isdir, n);
    double rr = 0.0;
    FEDD_TRY(true_residual(&rr, &aa));
    const double tol = call.rtol * den;
    double relres = std::sqrt(std::max(rr, 0.0)) / den;
    int its = 0;
    if (relres <= call.rtol) {
        if (relres_out) *relres_out = relres;
        return 0;
    }
    hipLaunchKernelGGL(k_cg_set, dim3(1), dim3(1), 0, st, S, (int)S_TOL2, tol * tol);
    FEDD_TRY(restart_direction());
    // The recurrences hold for A = A^T on the free rows only; on another matrix they neither break down nor converge (the
    // residual grows for as long as the budget lasts), so the first direction probes it, once per solve: with q = A p,
    // q.q = p.A^T A p and p.(A q) = p.A A p agree for a symmetric matrix (p, and with it q, vanishes on the unit Dirichlet
    // rows).  Rounding and the last bits in which a_ij and a_ji differ stay below 1e-14 ||p|| ||A q||; 1e-8 is asked.
    // (z is free here: the loop forms it again before it reads it.)
    {
        FEDD_TRY(spmv_owned(c, p, q, false, nullptr, 0.0, -1));
        FEDD_TRY(spmv_owned(c, q, z, false, nullptr, 0.0, -1));
        double qq = 0.0, paq = 0.0, pp = 0.0, zz = 0.0;
        hipLaunchKernelGGL(k_cg_rz, gb, blk, 0, st, (const double*)q, (const double*)q, n, (const double*)S, part);
        hipLaunchKernelGGL(k_cg_rz, gb, blk, 0, st, (const double*)p, (const double*)z, n, (const double*)S, part_x);
        FEDD_TRY(read2(part, part_x, &qq, &paq));
        hipLaunchKernelGGL(k_cg_rz, gb, blk, 0, st, (const double*)p, (const double*)p, n, (const double*)S, part);
        hipLaunchKernelGGL(k_cg_rz, gb, blk, 0, st, (const double*)z, (const double*)z, n, (const double*)S, part_x);
        FEDD_TRY(read2(part, part_x, &pp, &zz));
        const double scale = std::sqrt(std::max(pp, 0.0)) * std::sqrt(std::max(zz, 0.0));
        if (std::isfinite(qq) && std::isfinite(paq) && std::isfinite(scale) && std::fabs(qq - paq) > 1e-8 * scale) {
            c->cg_breakdown = FEDD_CG_BREAKDOWN_NONSYMMETRIC;
            if (relres_out) *relres_out = relres;
            FEDD_CHECK(false, "fedd_cg: breakdown (%s): p.A(Ap) = %.6e against (Ap).(Ap) = %.6e on the first direction; conjugate "
                              "gradients need a symmetric positive definite matrix on the free rows -- nonsymmetric systems "
                              "(advection, Navier-Stokes) are solved with fedd_gmres",
                       breakdown_name(FEDD_CG_BREAKDOWN_NONSYMMETRIC), paq, qq);
        }
    }

    hipEvent_t ev[CG_LAG + 1];
    for (auto& e : ev) e = nullptr;
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i <= CG_LAG; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } guard{ev};
    for (auto& e : ev) FEDD_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    double* hostw_dev = c->h_pinned_dev;
    constexpr int W = 8;    // doubles per slot of the pinned mirror

    int stalled = 0;
    double best_true = relres;
    bool finished = false;
    while (!finished) {
        // ---- queue iterations until the host sees `done` or the budget is spent ----
        int queued = 0;
        bool seen_done = false;
        const int budget = call.max_it - its;
        for (int j = 0; j < budget && !seen_done; ++j) {
            FEDD_TRY(spmv_owned(c, p, q, false, nullptr, 0.0, -1));
            {
                ScopedTimer t(c, FEDD_T_CG_PQ);
                t.bytes(16.0 * (double)n);
                hipLaunchKernelGGL(k_cg_pq, gb, blk, 0, st, (const double*)p, (const double*)q, n, (const double*)S, part);
                t.stop();
            }
            hipLaunchKernelGGL(k_cg_scalars, dim3(1), blk, 0, st, S, (const double*)part, nblk, 0, (double*)nullptr);
            {
                ScopedTimer t(c, FEDD_T_CG_XR);
                t.bytes(48.0 * (double)n);
                hipLaunchKernelGGL(k_cg_xr, gb, blk, 0, st, x, r, (const double*)p, (const double*)q, n, (const double*)S, part_rr);
                t.stop();
            }
            const int slot = j % (CG_LAG + 1);
            hipLaunchKernelGGL(k_cg_scalars, dim3(1), blk, 0, st, S, (const double*)part_rr, nblk, 1,
                               hostw_dev ? hostw_dev + W * slot : (double*)nullptr);
            if (!hostw_dev) FEDD_HIP(hipMemcpyAsync(hp + W * slot, S + S_DONE, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
            FEDD_HIP(hipEventRecord(ev[slot], st));
            ++queued;
            if (call.use_prec) FEDD_TRY(schwarz_apply(c, r, z, false));
            {
                ScopedTimer t(c, FEDD_T_CG_RZ);
                t.bytes(16.0 * (double)n);
                hipLaunchKernelGGL(k_cg_rz, gb, blk, 0, st, (const double*)r, (const double*)(call.use_prec ? z : r), n, (const double*)S, part_rz);
                t.stop();
            }
            hipLaunchKernelGGL(k_cg_scalars, dim3(1), blk, 0, st, S, (const double*)part_rz, nblk, 2, (double*)nullptr);
            {
                ScopedTimer t(c, FEDD_T_CG_P);
                t.bytes(24.0 * (double)n + 4.0 * (double)n);
                hipLaunchKernelGGL(k_cg_p, gn, blk, 0, st, p, (const double*)(call.use_prec ? z : r), isdir, n, (const double*)S);
                t.stop();
            }
            if (j >= CG_LAG) {      // the words of iteration j - CG_LAG: written long ago, no wait in the usual case
                const int ls = (j - CG_LAG) % (CG_LAG + 1);
                FEDD_HIP(hipEventSynchronize(ev[ls]));
                // (mapped: iterations | done | breakdown | r.r;  copied: done | breakdown | iterations)
                seen_done = hostw_dev ? hp[W * ls + 1] != 0.0 : hp[W * ls] != 0.0;
            }
        }
        // ---- the state the device stopped at ----
        FEDD_HIP(hipMemcpyAsync(hp + 40, S, S_COUNT * sizeof(double), hipMemcpyDeviceToHost, st));
        FEDD_HIP(hipStreamSynchronize(st));
        (void)queued;
        its = (int)hp[40 + S_ITS];
        const int brk = (int)hp[40 + S_BRK];
        const bool conv = hp[40 + S_CONV] != 0.0;
        if (brk) {
            c->cg_breakdown = brk;
            double rt = 0.0;
            FEDD_TRY(true_residual(&rt, &aa));
            relres = std::sqrt(std::max(rt, 0.0)) / den;
            if (its_out) *its_out = its;
            if (relres_out) *relres_out = relres;
            FEDD_CHECK(false, "fedd_cg: breakdown (%s) in iteration %d: operator or preconditioner not positive definite on the Krylov space",
                       breakdown_name(brk), its + 1);
        }
        // every claim of convergence, and the end of the budget, is checked against b - A x
        double rt = 0.0;
        FEDD_TRY(true_residual(&rt, &aa));      // (r now holds the true residual)
        relres = std::sqrt(std::max(rt, 0.0)) / den;
        if (!conv || relres <= call.rtol || its >= call.max_it) {
            finished = true;
            break;
        }
        // the claim failed: r is the true residual; z, p and rho start again
        ++c->cg_replacements;
        stalled = relres < 0.5 * best_true ? 0 : stalled + 1;
        best_true = std::min(best_true, relres);
        if (stalled >= 3) break;    // three replacements in a row without progress: the rounding floor of b - A x
        FEDD_HIP(hipMemsetAsync(S + S_DONE, 0, sizeof(double), st));
        FEDD_HIP(hipMemsetAsync(S + S_CONV, 0, sizeof(double), st));
        FEDD_TRY(restart_direction());
    }
    FEDD_HIP(hipGetLastError());
    FEDD_HIP(hipStreamSynchronize(st));
    if (its_out) *its_out = its;
    if (relres_out) *relres_out = relres;
    return 0;
}

}  // namespace fedd
