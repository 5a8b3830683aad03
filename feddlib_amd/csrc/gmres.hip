// Right-preconditioned restarted GMRES on the device, block size 1.
//
// Stands in for Thyra::solve on the Belos "Block GMRES" LOWS that
// LinearSolver::solveMonolithic builds (feddlib/problems/Solver/LinearSolver_def.hpp:72-135) with
// the settings of feddlib/problems/tests/laplace/parametersSolver.xml:5-15 (Block Size 1, DGKS
// orthogonalisation, relative residual tolerance, maximum iterations) and the preconditioner
// attached as Thyra "unspecified" side = right.  Belos is not in the reference tree; this is the
// published algorithm (Saad, Iterative Methods, Alg. 9.5):
//   - classical Gram-Schmidt with two passes (what Belos' DGKS / ICGS managers do), default
//     formulation: the second pass of a basis vector is delayed and fused with the first pass of
//     the next Krylov vector (DCGS2, see k_multidot2 below): two sweeps over the basis and one
//     reduction per iteration.  fedd_set_option("gmres_kind", 1) selects the plain two-pass form
//     (fused multi-dot + multi-axpy twice, second pass gated by the DGKS test on the device);
//   - Givens QR of the Hessenberg matrix on the device (single lane), the host reads one double
//     per iteration (implicit relative residual) to decide convergence, one iteration behind;
//   - x = x0 + M^-1 (V y) at the end of a cycle (M is a fixed linear operator, so Z is not stored).
// All sums run in a fixed order: results are bitwise reproducible run to run.
//
// This file: the one-vector kernels, the all-reduce, the coarse projection, the solve frame of all three solvers (Frame,
// declared in gmres_frame.hpp), the one-vector solvers (DCGS2, CGS2) and the dispatcher gmres_solve.  The default solver,
// s-step GMRES (gmres_kind 2), is in gmres_sstep.hip with its block kernels; its stopping rule in gmres_stop_rule.hpp.
#include "gmres_frame.hpp"
#include <rccl/rccl.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace fedd {
namespace {

// partial[col*nblk + blk] = sum over the workgroup's rows of V_col . w ; col == ncolsV means w . w.
// A workgroup keeps its 2048 rows of w in registers and sweeps MD_CG basis columns, so the basis
// is read from HBM exactly once per pass with 16-byte loads; w is re-read from L2.
__global__ __launch_bounds__(256) void k_multidot(const double* __restrict__ V, int64_t ldv, int64_t n, int ncolsV,
                                                  const double* __restrict__ w, double* __restrict__ partial,
                                                  int nblk, const int32_t* __restrict__ gate) {
    if (gate && !*gate) return;
    __shared__ double sh[4][MD_CG];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * MD_ROWS + 2 * tid;
    double2 wv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wv[k] = ld2c(w, r0 + 512 * k, n);
    double acc[MD_CG];
#pragma unroll
    for (int cc = 0; cc < MD_CG; ++cc) {
        const int col = blockIdx.y * MD_CG + cc;
        double s = 0.0;
        if (col <= ncolsV) {
            const double* __restrict__ a = col < ncolsV ? V + (int64_t)col * ldv : w;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double2 v = ld2(a, r0 + 512 * k, n);
                s += v.x * wv[k].x + v.y * wv[k].y;
            }
        }
        acc[cc] = s;
    }
#pragma unroll
    for (int cc = 0; cc < MD_CG; ++cc) {
        double s = acc[cc];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((tid & 63) == 0) sh[tid >> 6][cc] = s;
    }
    __syncthreads();
    if (tid < MD_CG) {
        const int col = blockIdx.y * MD_CG + tid;
        if (col <= ncolsV) partial[(int64_t)col * nblk + blockIdx.x] = sh[0][tid] + sh[1][tid] + sh[2][tid] + sh[3][tid];
    }
}

// out[col] = sum_blk partial[col][blk]   (one workgroup per column, fixed order)
__global__ __launch_bounds__(256) void k_reduce_cols(const double* __restrict__ partial, double* __restrict__ out,
                                                     int nblk, const int32_t* __restrict__ gate) {
    if (gate && !*gate) return;
    __shared__ double sh[256];
    const int col = blockIdx.x;
    double s = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 256) s += partial[(int64_t)col * nblk + k];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[col] = sh[0];
}

// w -= sum_c h[c] V_c ; also partial sums of ||w_new||^2 into partial[blk].  One double2 of w per
// lane, the column loop unrolled 8x keeps 8 x 16 B loads in flight per lane.
__global__ __launch_bounds__(256) void k_multiaxpy(const double* __restrict__ V, int64_t ldv, int64_t n, int ncols,
                                                   const double* __restrict__ h, double* __restrict__ w,
                                                   double* __restrict__ partial, const int32_t* __restrict__ gate) {
    if (gate && !*gate) return;
    __shared__ double sh_h[1024];
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    for (int c = tid; c < ncols; c += 256) sh_h[c] = h[c];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * AX_ROWS + 2 * tid;
    double2 v = ld2c(w, r, n);
    int c = 0;
    for (; c + 8 <= ncols; c += 8) {
        double2 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = ld2(V + (int64_t)(c + u) * ldv, r, n);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            v.x -= sh_h[c + u] * t[u].x;
            v.y -= sh_h[c + u] * t[u].y;
        }
    }
    for (; c < ncols; ++c) {
        const double2 t = ld2(V + (int64_t)c * ldv, r, n);
        v.x -= sh_h[c] * t.x;
        v.y -= sh_h[c] * t.y;
    }
    double nrm = 0.0;
    if (r + 1 < n) {
        *reinterpret_cast<double2*>(w + r) = v;
        nrm = v.x * v.x + v.y * v.y;
    } else if (r < n) {
        w[r] = v.x;
        nrm = v.x * v.x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nrm += __shfl_down(nrm, off, 64);
    if ((tid & 63) == 0) sh[tid >> 6] = nrm;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// DGKS test from the pass-1 coefficients alone: with an orthonormal basis ||w - V h||^2 =
// ||w||^2 - ||h||^2, so the second pass is needed iff ||h||^2 > 1/2 ||w||^2 (h1[0..j] = V^T w,
// h1[j+1] = w.w, all already reduced over ranks).  When the test does not fire the difference has
// no cancellation and is the squared norm after the pass (nrm1); when it fires the norm comes from
// the second pass.  No extra reduction, no extra all-reduce.
__global__ void k_dgks_gate(const double* __restrict__ h1, int j, int32_t* __restrict__ gate, double* __restrict__ nrm1) {
    double s = 0.0;
    for (int c = 0; c <= j; ++c) s += h1[c] * h1[c];
    const double ww = h1[j + 1];
    gate[0] = s > 0.5 * ww ? 1 : 0;
    nrm1[0] = fmax(ww - s, 0.0);
}

// Finish column j of the Hessenberg matrix: h = h1 (+ h2), h_{j+1,j} = ||w||; apply the previous
// rotations, create the new one, update g.  misc[0] = |g_{j+1}|, misc[1] = 1/h_{j+1,j}.
// One workgroup: all lanes stage the column and the stored rotations in LDS (independent loads),
// lane 0 then runs the inherently sequential rotation chain out of LDS instead of a chain of
// dependent global loads.
__global__ __launch_bounds__(256) void k_givens(double* __restrict__ S, Off o, int j, int m,
                                                const int32_t* __restrict__ gate,
                                                const double* __restrict__ nrm2_partial, int npart) {
    extern __shared__ double gs[];  // hcol[m+2] | cs[m] | sn[m]
    __shared__ double red[256];
    double* hc = gs;
    double* lcs = hc + (m + 2);
    double* lsn = lcs + m;
    const bool two = gate[0] != 0;
    // one rank: the partial sums of ||w||^2 of the second pass are added here (fixed order) instead
    // of in a launch of their own; several ranks reduce and all-reduce before this kernel
    if (nrm2_partial && two) {
        double s = 0.0;
        for (int k = threadIdx.x; k < npart; k += 256) s += nrm2_partial[k];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int k = 128; k > 0; k >>= 1) {
            if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
            __syncthreads();
        }
        if (threadIdx.x == 0) S[o.nrm + 2] = red[0];
    }
    for (int i = threadIdx.x; i <= j; i += blockDim.x) hc[i] = S[o.h1 + i] + (two ? S[o.h2 + i] : 0.0);
    for (int i = threadIdx.x; i < j; i += blockDim.x) {
        lcs[i] = S[o.cs + i];
        lsn[i] = S[o.sn + i];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double hn = sqrt(two ? S[o.nrm + 2] : S[o.nrm + 1]);
    hc[j + 1] = hn;
    for (int i = 0; i < j; ++i) {
        const double t = lcs[i] * hc[i] + lsn[i] * hc[i + 1];
        hc[i + 1] = -lsn[i] * hc[i] + lcs[i] * hc[i + 1];
        hc[i] = t;
    }
    const double d = hypot(hc[j], hc[j + 1]);
    const double cj = d > 0 ? hc[j] / d : 1.0, sj = d > 0 ? hc[j + 1] / d : 0.0;
    S[o.cs + j] = cj;
    S[o.sn + j] = sj;
    hc[j] = d;
    double* H = S + o.H + (int64_t)j * (m + 1);
    for (int i = 0; i <= j; ++i) H[i] = hc[i];
    H[j + 1] = 0.0;
    const double gj = S[o.g + j];
    S[o.g + j + 1] = -sj * gj;
    S[o.g + j] = cj * gj;
    S[o.misc + 0] = fabs(sj * gj);
    S[o.misc + 1] = hn > 0 ? 1.0 / hn : 0.0;
    S[o.misc + 2] = hn;
}

__global__ void k_scale_to(const double* __restrict__ w, const double* __restrict__ scal, double* __restrict__ out,
                           int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = w[i] * scal[0];
}

// start of a cycle: beta = sqrt(nrm2[0]); V0 = r / beta; g = (beta, 0, ...)
__global__ void k_cycle_init(double* __restrict__ S, Off o, int m, const double* __restrict__ rr) {
    const double beta = sqrt(rr[0]);
    for (int i = 0; i <= m; ++i) S[o.g + i] = 0.0;
    S[o.g] = beta;
    S[o.misc + 1] = beta > 0 ? 1.0 / beta : 0.0;
    S[o.misc + 3] = beta;
}

// y = R^-1 g for the k x k upper triangle (column-major H with leading dimension m+1)
// Column-oriented back substitution by one workgroup: y_i = t_i / R_ii, then every lane r < i
// updates t_r -= R_ri y_i (column i of H is contiguous).  Fixed order => reproducible.
__global__ __launch_bounds__(256) void k_backsolve(double* __restrict__ S, Off o, int k, int m) {
    extern __shared__ double t[];  // [k]
    const double* H = S + o.H;
    for (int i = threadIdx.x; i < k; i += blockDim.x) t[i] = S[o.g + i];
    __syncthreads();
    for (int i = k - 1; i >= 0; --i) {
        const double yi = t[i] / H[(int64_t)i * (m + 1) + i];
        __syncthreads();
        if (threadIdx.x == 0) S[o.y + i] = yi;
        for (int r = threadIdx.x; r < i; r += blockDim.x) t[r] -= H[(int64_t)i * (m + 1) + r] * yi;
        __syncthreads();
    }
}

// u = sum_c y[c] V_c : one double2 of u per lane, the column loop unrolled 8x (8 x 16 B non-temporal loads in flight per lane;
// the first version, a scalar load per lane and column, ran at half the bandwidth: 1.1 ms for 45 columns at 9.9 M rows)
__global__ __launch_bounds__(256) void k_combine(const double* __restrict__ V, int64_t ldv, int64_t n, int k,
                                                 const double* __restrict__ y, double* __restrict__ u) {
    __shared__ double sh_y[1024];
    const int tid = threadIdx.x;
    for (int c = tid; c < k; c += 256) sh_y[c] = y[c];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * AX_ROWS + 2 * tid;
    double2 v = {0.0, 0.0};
    int c = 0;
    for (; c + 8 <= k; c += 8) {
        double2 t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = ld2(V + (int64_t)(c + q) * ldv, r, n);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            v.x += sh_y[c + q] * t[q].x;
            v.y += sh_y[c + q] * t[q].y;
        }
    }
    for (; c < k; ++c) {
        const double2 t = ld2(V + (int64_t)c * ldv, r, n);
        v.x += sh_y[c] * t.x;
        v.y += sh_y[c] * t.y;
    }
    if (r + 1 < n) *reinterpret_cast<double2*>(u + r) = v;
    else if (r < n) u[r] = v.x;
}

// ------------------------------------------------------------------------------------------------
// Delayed re-orthogonalisation (DCGS2; Bielich, Langou, Thomas, Swirydowicz, Yamazaki, Boman,
// "Low-synch Gram-Schmidt with delayed reorthogonalization for Krylov solvers", 2022): the second
// Gram-Schmidt pass of basis vector k+1 and the first pass of the next Krylov vector are one sweep
// of dot products and one sweep of updates over the basis, instead of two and two.
//
// State before a step: V_k = [v_1 .. v_k] final (orthonormal), u = first-pass result that becomes
// v_{k+1}, hp = first-pass coefficients of column k of H.  With B = A M^-1:
//   wt = B u                                        (u is NOT yet re-orthogonalised or normalised)
//   sweep 1:  s = V_k^T u,  t = V_k^T wt,  alpha2 = u.u,  gamma = u.wt      (one reduction)
//   beta = sqrt(alpha2 - s.s);  column k of H = [hp + s ; beta]   -> Givens, residual
//   v_{k+1} = (u - V_k s) / beta,   B v_{k+1} = (wt - V_{k+1} Hbar_k s) / beta   (B V_k = V_{k+1} Hbar_k)
//   hp'_i = (t_i - (Hbar_k s)_i) / beta  (i <= k),  hp'_{k+1} = ((gamma - s.t)/beta - (Hbar_k s)_{k+1}) / beta
//   sweep 2:  v_{k+1} as above,  u' = (wt - V_k t)/beta - v_{k+1} (gamma - s.t)/beta^2
// u' is the first-pass result for the next vector; every basis column is read twice per iteration.

// partial[(2 col + which) * nblk + blk]: which = 0: V_col . u, 1: V_col . w; col == ncolsV: u.u and u.w
template <int NCH>
__global__ __launch_bounds__(256) void k_multidot2(const double* __restrict__ V, int64_t ldv, int64_t n, int ncolsV,
                                                   const double* __restrict__ u, const double* __restrict__ w,
                                                   double* __restrict__ partial, int nblk) {
    __shared__ double sh[4][2 * MD2_CG];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * (512 * NCH) + 2 * tid;
    double2 uv[NCH], wv[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        uv[k] = ld2c(u, r0 + 512 * k, n);
        wv[k] = ld2c(w, r0 + 512 * k, n);
    }
    // column groups cg = blockIdx.y, blockIdx.y + gridDim.y, ...: u and w stay in registers across them
    for (int cg = blockIdx.y; cg * MD2_CG <= ncolsV; cg += gridDim.y) {
        double au[MD2_CG], aw[MD2_CG];
#pragma unroll
        for (int cc = 0; cc < MD2_CG; ++cc) {
            const int col = cg * MD2_CG + cc;
            double su = 0.0, sw = 0.0;
            if (col <= ncolsV) {
                const double* __restrict__ a = col < ncolsV ? V + (int64_t)col * ldv : u;
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    const double2 v = ld2(a, r0 + 512 * k, n);
                    su += v.x * uv[k].x + v.y * uv[k].y;
                    sw += v.x * wv[k].x + v.y * wv[k].y;
                }
            }
            au[cc] = su;
            aw[cc] = sw;
        }
#pragma unroll
        for (int cc = 0; cc < MD2_CG; ++cc) {
            double su = au[cc], sw = aw[cc];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                su += __shfl_down(su, off, 64);
                sw += __shfl_down(sw, off, 64);
            }
            if ((tid & 63) == 0) {
                sh[tid >> 6][2 * cc] = su;
                sh[tid >> 6][2 * cc + 1] = sw;
            }
        }
        __syncthreads();
        if (tid < 2 * MD2_CG) {
            const int col = cg * MD2_CG + (tid >> 1);
            if (col <= ncolsV)
                partial[(int64_t)(2 * col + (tid & 1)) * nblk + blockIdx.x] = sh[0][tid] + sh[1][tid] + sh[2][tid] + sh[3][tid];
        }
        __syncthreads();
    }
}

struct Off2 {
    int Hraw, hp, st, cf;  // unrotated Hessenberg (m+1) x m, first-pass column, reduced dots, sweep-2 coefficients
};

// The small algebra of a DCGS2 step (one workgroup): finalise column kc = k - 1 of H, rotate it,
// update g and the residual, and prepare the coefficients of sweep 2 and the next first-pass column.
// misc[0] = |g_k| (residual), misc[2] = beta (0: breakdown), cf = [s (m) | t (m) | 1/beta | c_last].
// host_out (pinned host memory, device-visible): the three numbers the host's lagged convergence test reads -- written by
// the kernel itself, so that no copy engine call sits in the stream between two iterations (8.7 us each)
__global__ __launch_bounds__(256) void k_dcgs2_small(double* __restrict__ S, Off o, Off2 o2, int k, int m,
                                                     double* __restrict__ host_out) {
    extern __shared__ double sm[];  // s[m] | t[m] | hc[m+2] | lcs[m] | lsn[m] | Hs[m+1]
    __shared__ double red[2][256];
    double* s = sm;
    double* t = s + m;
    double* hc = t + m;
    double* lcs = hc + (m + 2);
    double* lsn = lcs + m;
    double* Hs = lsn + m;
    const int tid = threadIdx.x, kc = k - 1, ldh = m + 1;
    const double* st = S + o2.st;
    double ps = 0.0, pd = 0.0;
    for (int i = tid; i < k; i += 256) {
        const double si = st[2 * i], ti = st[2 * i + 1];
        s[i] = si;
        t[i] = ti;
        ps += si * si;
        pd += si * ti;
    }
    for (int i = tid; i < kc; i += 256) {
        lcs[i] = S[o.cs + i];
        lsn[i] = S[o.sn + i];
    }
    red[0][tid] = ps;
    red[1][tid] = pd;
    __syncthreads();
    for (int q = 128; q > 0; q >>= 1) {
        if (tid < q) {
            red[0][tid] += red[0][tid + q];
            red[1][tid] += red[1][tid + q];
        }
        __syncthreads();
    }
    const double ss = red[0][0], sd = red[1][0];
    const double alpha2 = st[2 * k], gamma = st[2 * k + 1];
    const double beta2 = alpha2 - ss;
    const double beta = beta2 > 0.0 ? sqrt(beta2) : 0.0;
    const double ib = beta > 0.0 ? 1.0 / beta : 0.0;
    // unrotated column kc
    double* Hraw = S + o2.Hraw;
    for (int i = tid; i <= k; i += 256) {
        const double v = i < k ? S[o2.hp + i] + s[i] : beta;
        Hraw[(int64_t)kc * ldh + i] = v;
        hc[i] = v;
    }
    __syncthreads();
    // Hs = Hbar_k s  (rows 0..k, columns 0..kc; entries below the sub-diagonal are zero)
    for (int i = tid; i <= k; i += 256) {
        // (eight independent loads in flight: the Hessenberg matrix is read from L2, and a chain of
        // dependent-latency loads was the whole cost of this kernel)
        double a = 0.0;
        int c = i > 0 ? i - 1 : 0;
        for (; c + 8 <= kc; c += 8) {
            double hv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) hv[q] = Hraw[(int64_t)(c + q) * ldh + i];
#pragma unroll
            for (int q = 0; q < 8; ++q) a += hv[q] * s[c + q];
        }
        for (; c < kc; ++c) a += Hraw[(int64_t)c * ldh + i] * s[c];
        a += hc[i] * s[kc];  // the column written above, taken from LDS
        Hs[i] = a;
    }
    __syncthreads();
    // next first-pass column and the coefficients of sweep 2
    for (int i = tid; i <= k; i += 256) {
        const double v = i < k ? (t[i] - Hs[i]) * ib : ((gamma - sd) * ib - Hs[k]) * ib;
        S[o2.hp + i] = v;
    }
    for (int i = tid; i < k; i += 256) {
        S[o2.cf + i] = s[i];
        S[o2.cf + m + i] = t[i];
    }
    if (tid == 0) {
        S[o2.cf + 2 * m] = ib;
        S[o2.cf + 2 * m + 1] = (gamma - sd) * ib * ib;
        // Givens: previous rotations on the new column, new rotation, g and the residual
        for (int i = 0; i < kc; ++i) {
            const double a = lcs[i] * hc[i] + lsn[i] * hc[i + 1];
            hc[i + 1] = -lsn[i] * hc[i] + lcs[i] * hc[i + 1];
            hc[i] = a;
        }
        const double d = hypot(hc[kc], hc[kc + 1]);
        const double cj = d > 0 ? hc[kc] / d : 1.0, sj = d > 0 ? hc[kc + 1] / d : 0.0;
        S[o.cs + kc] = cj;
        S[o.sn + kc] = sj;
        hc[kc] = d;
        double* H = S + o.H + (int64_t)kc * ldh;
        for (int i = 0; i <= kc; ++i) H[i] = hc[i];
        H[kc + 1] = 0.0;
        const double gj = S[o.g + kc];
        S[o.g + kc + 1] = -sj * gj;
        S[o.g + kc] = cj * gj;
        S[o.misc + 0] = fabs(sj * gj);
        S[o.misc + 1] = ib;
        S[o.misc + 2] = beta;
        if (host_out) {
            host_out[0] = fabs(sj * gj);
            host_out[1] = ib;
            host_out[2] = beta;
            __threadfence_system();
        }
    }
}

// sweep 2: V[:, k] = (u - V_k s) / beta ;  u <- (w - V_k t) / beta - V[:, k] * c_last
__global__ __launch_bounds__(256) void k_axpy2(double* __restrict__ V, int64_t ldv, int64_t n, int k,
                                               const double* __restrict__ cf, int m, double* __restrict__ u,
                                               const double* __restrict__ w) {
    __shared__ double sh_s[1024], sh_t[1024];
    const int tid = threadIdx.x;
    for (int c = tid; c < k; c += 256) {
        sh_s[c] = cf[c];
        sh_t[c] = cf[m + c];
    }
    __syncthreads();
    const double ib = cf[2 * m], cl = cf[2 * m + 1];
    const int64_t r = (int64_t)blockIdx.x * AX_ROWS + 2 * tid;
    double2 as = {0.0, 0.0}, at = {0.0, 0.0};
    int c = 0;
    for (; c + 8 <= k; c += 8) {
        double2 q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = ld2(V + (int64_t)(c + j) * ldv, r, n);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            as.x += sh_s[c + j] * q[j].x;
            as.y += sh_s[c + j] * q[j].y;
            at.x += sh_t[c + j] * q[j].x;
            at.y += sh_t[c + j] * q[j].y;
        }
    }
    for (; c < k; ++c) {
        const double2 q = ld2(V + (int64_t)c * ldv, r, n);
        as.x += sh_s[c] * q.x;
        as.y += sh_s[c] * q.y;
        at.x += sh_t[c] * q.x;
        at.y += sh_t[c] * q.y;
    }
    const double2 uu = ld2c(u, r, n), ww = ld2c(w, r, n);
    double2 vn, un;
    vn.x = (uu.x - as.x) * ib;
    vn.y = (uu.y - as.y) * ib;
    un.x = (ww.x - at.x) * ib - vn.x * cl;
    un.y = (ww.y - at.y) * ib - vn.y * cl;
    double* vk = V + (int64_t)k * ldv;
    if (r + 1 < n) {
        {
            typedef double v2d __attribute__((ext_vector_type(2)));
            v2d tv;
            tv.x = vn.x;
            tv.y = vn.y;
            __builtin_nontemporal_store(tv, reinterpret_cast<v2d*>(vk + r));  // next read is a basis sweep
        }
        *reinterpret_cast<double2*>(u + r) = un;
    } else if (r < n) {
        vk[r] = vn.x;
        u[r] = un.x;
    }
}

// out = m o a + (1 - m) o b  (m = 0 / 1 mask): the constrained operator of the interior solves, see Frame::mk
__global__ void k_mask_mix(const double* __restrict__ m, const double* __restrict__ a, const double* __restrict__ b,
                           double* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = m[i] != 0.0 ? a[i] : b[i];
}

__global__ void k_axpby(double a, const double* __restrict__ x, double b, const double* __restrict__ y,
                        double* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a * x[i] + b * y[i];
}

}  // namespace

int allreduce_sum(fedd_ctx* c, double* d_buf, int n) {
    if (c->nranks == 1) return 0;
    ScopedTimer timer(c, FEDD_T_ALLREDUCE);
    if (c->cb_allreduce) {  // host-staged transport (functional tests)
        std::vector<double> tmp((size_t)n);
        FEDD_HIP(hipMemcpyAsync(tmp.data(), d_buf, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        FEDD_HIP(hipStreamSynchronize(c->stream));
        const int rc = c->cb_allreduce(c->cb_user, tmp.data(), n);
        FEDD_CHECK(rc == 0, "allreduce: the host callback failed (%d)", rc);
        FEDD_HIP(hipMemcpyAsync(d_buf, tmp.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        FEDD_HIP(hipStreamSynchronize(c->stream));
        return 0;
    }
    FEDD_CHECK(c->comm, "allreduce: no communicator");
    ncclResult_t r = ncclAllReduce(d_buf, d_buf, (size_t)n, ncclDouble, ncclSum, (ncclComm_t)c->comm, c->stream);
    FEDD_CHECK(r == ncclSuccess, "ncclAllReduce: %s", ncclGetErrorString(r));
    return 0;
}

// Multiplicative level combination (fedd_schwarz_set_level_combination): Phi^T A (I - Pc A) M1^-1 = (I - K0 K0^-1) Phi^T A M1^-1
// vanishes up to the regularisation of K0^-1, so the Krylov space cannot reduce the part of the residual that Phi^T sees.  Every
// cycle therefore starts from a coarse-orthogonal residual: x += Pc r, r = b - A x (in exact arithmetic r -= A Pc r), one coarse
// apply and one SpMV.  K0^-1 inverts K0 + 1e-12 diag(K0), so one such step leaves 1e-12 of Phi^T r behind.  At a restart that is
// far below the target; at the start, where r = b and ||b - A Pc b|| can be orders of magnitude below ||b||, it is not (3D
// Laplace, 27-node boxes, Q1: 29 iterations to 1e-12 after one step, 14 after two), so the start takes two steps:
// x_0 + Pc (b - A x_0), the reference's pre-apply for x_0 = 0, refined once.  At a restart the step removes what the shift let
// grow during the cycle.
static int coarse_project(fedd_ctx* c, const double* d_b, double* d_x, double* d_r, int use_compact, int steps) {
    const int64_t n = c->n_rows;
    for (int k = 0; k < steps; ++k) {
        FEDD_TRY(coarse_apply_add(c, d_r, d_x));
        FEDD_TRY(spmv_owned(c, d_x, d_r, false, nullptr, 0.0, use_compact));
        hipLaunchKernelGGL(k_axpby, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, 1.0, d_b, -1.0, (const double*)d_r, d_r, n);
    }
    return 0;
}

int Frame::setup(fedd_ctx* ctx, const GmresCall& call, bool with_tail) {
    c = ctx;
    a = &call;
    nr = std::max(call.nr, 1);
    tail = with_tail;
    ghosts = c->n_cols != c->n_rows || !c->halo.peers.empty();
    n = c->n_rows * nr;
    m = std::min(call.restart, call.max_it);
    ldv = (n + 15) & ~(int64_t)15;
    FEDD_CHECK(m + 2 <= 1024, "gmres: restart length above 1022 is not supported");
    nblk = (int)((n + MD_ROWS - 1) / MD_ROWS);
    nblk2 = (int)((n + AX_ROWS - 1) / AX_ROWS);
    nc = tail ? (std::max<int64_t>(c->n_rows, c->n_cols) * nr + 15) & ~(int64_t)15 : n;
    p = 0;
    o.H = p; p += (m + 1) * m;
    o.cs = p; p += m;
    o.sn = p; p += m;
    o.g = p; p += m + 1;
    o.h1 = p; p += m + 2;
    o.h2 = p; p += m + 2;
    o.nrm = p; p += 4;
    o.y = p; p += m;
    o.misc = p; p += 8;
    gn = dim3((unsigned)((n + 255) / 256));
    blk = dim3(256);
    st = c->stream;
    mk = call.mask;
    project = call.use_prec && levels_mult(c) && !mk && nr <= 1;
    return 0;
}

// block_kernels (s-step solver): they read whole 16-byte row pairs and rely on the padding rows [n, ldv) of every basis
// column being zero (and on finite data everywhere): a freshly (re)allocated basis, or one last used with another
// vector length, is cleared
int Frame::alloc(size_t part, bool block_kernels) {
    const double* before = c->d_V.p;
    FEDD_TRY(c->d_V.ensure((size_t)(m + 1) * ldv));
    if (!block_kernels) {
        if (c->gm_V_ldv != ldv) c->gm_V_ldv = -1;   // another column layout: the s-step solver clears the basis before its next use
    } else {
        // (a buffer that another vector length used holds finite values everywhere: only its padding rows need the clearing)
        if (c->d_V.p != before) FEDD_HIP(hipMemsetAsync(c->d_V.p, 0, c->d_V.cap * sizeof(double), st));
        else if (c->gm_V_ldv != ldv && ldv != n) FEDD_HIP(hipMemsetAsync(c->d_V.p, 0, (size_t)(m + 1) * ldv * sizeof(double), st));
        c->gm_V_ldv = ldv;
    }
    FEDD_TRY(c->d_w.ensure(std::max<size_t>((size_t)(tail ? 2 : 1) * nc, c->d_w.cap)));
    FEDD_TRY(c->d_Z.ensure((size_t)nc * (nr > 1 && ghosts ? 3 : 2)));   // (stacked, several ranks: + a copy with a ghost tail)
    FEDD_TRY(c->d_part.ensure(part));
    FEDD_TRY(c->d_small.ensure((size_t)p + 8));
    S = c->d_small.p;
    V = c->d_V.p;
    w0 = c->d_w.p;
    w1 = c->d_w.p + nc;
    z = c->d_Z.p;
    r = c->d_Z.p + nc;
    return 0;
}

void Frame::reduce_cols(int ncols, double* out, int nblk_part, const int32_t* gate) {
    hipLaunchKernelGGL(k_reduce_cols, dim3(ncols), blk, 0, st, (const double*)c->d_part.p, out, nblk_part, gate);
}
void Frame::first_basis_vector() {
    hipLaunchKernelGGL(k_scale_to, gn, blk, 0, st, (const double*)r, (const double*)(S + o.misc + 1), V, n);
}
void Frame::backsolve(int cols) {
    hipLaunchKernelGGL(k_backsolve, dim3(1), dim3(256), (size_t)(cols + 1) * sizeof(double), st, S, o, cols, m);
}

int Frame::norm2(const double* v, double* out) {   // out[0] = v.v (global)
    hipLaunchKernelGGL(k_multidot, dim3(nblk, 1), blk, 0, st, v, ldv, n, 0, v, c->d_part.p, nblk, (const int32_t*)nullptr);
    reduce_cols(1, out, nblk);
    return allreduce_sum(c, out, 1);
}
// the host reads sqrt(S[nrm + 3]) (every rank takes the same decision)
int Frame::read_norm(double* out) {
    FEDD_HIP(hipMemcpyAsync(c->h_pinned, S + o.nrm + 3, sizeof(double), hipMemcpyDeviceToHost, st));
    FEDD_HIP(hipStreamSynchronize(st));
    *out = std::sqrt(std::max(c->h_pinned[0], 0.0));
    return 0;
}

// out = A M^-1 in - theta in  (in_tail: `in` is a work vector with a ghost tail, a basis column has none; the shift rides
// in the SpMV kernel's store)
int Frame::apply(const double* in, double* out, bool in_tail, double theta) {
    const int use_prec = a->use_prec;
    if (nr > 1) {       // masks ride in the kernels' stores
        double* src = const_cast<double*>(in);
        if (ghosts) {
            src = c->d_Z.p + 2 * nc;
            FEDD_HIP(hipMemcpyAsync(src, in, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        FEDD_TRY(schwarz_apply_multi(c, src, z, mk));
        return spmm_owned(c, z, out, mk, z);
    }
    if (use_prec) FEDD_TRY(prec_apply(c, in, z, in_tail));   // (the attached block operator, else Schwarz)
    if (mk) {
        // z <- D M^-1 D in + (I - D) in   (M^-1 D in: the masked entries of `in` are excluded by a copy)
        if (use_prec) hipLaunchKernelGGL(k_mask_mix, gn, blk, 0, st, mk, (const double*)z, in, z, n);
        else FEDD_HIP(hipMemcpyAsync(z, in, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
        FEDD_TRY(spmv_owned(c, z, out, tail));
        hipLaunchKernelGGL(k_mask_mix, gn, blk, 0, st, mk, (const double*)out, (const double*)z, out, n);
        return 0;
    }
    return spmv_owned(c, use_prec ? z : in, out, use_prec ? tail : in_tail, theta != 0.0 ? in : nullptr, theta);
}

// r = b - A x, the product landing in ax (which may be r)
int Frame::residual(double* x, double* ax, bool x_tail, int use_compact) {
    if (nr > 1) {
        FEDD_TRY(spmm_owned(c, x, ax, mk, x));
    } else {
        FEDD_TRY(spmv_owned(c, x, ax, x_tail, nullptr, 0.0, use_compact));
        if (mk) hipLaunchKernelGGL(k_mask_mix, gn, blk, 0, st, mk, (const double*)ax, (const double*)x, ax, n);
    }
    hipLaunchKernelGGL(k_axpby, gn, blk, 0, st, 1.0, a->b, -1.0, (const double*)ax, r, n);
    return 0;
}

// initial guess, two projection steps, beta0 = ||r_0|| on the host (0: nothing to solve, report() and return)
int Frame::start(double* ax, int use_compact) {
    if (a->x0 && !mk && nr == 1) {   // "Zero Initial Guess" = false (LinearSolver_def.hpp:76-78): x holds x_0, r_0 = b - A x_0
        FEDD_TRY(residual(a->x, ax, false, -1));
    } else {
        FEDD_HIP(hipMemsetAsync(a->x, 0, (size_t)n * sizeof(double), st));  // "Zero Initial Guess" (LinearSolver_def.hpp:76-78)
        FEDD_HIP(hipMemcpyAsync(r, a->b, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    if (project) FEDD_TRY(coarse_project(c, a->b, a->x, r, use_compact, 2));
    FEDD_TRY(norm2(r, S + o.nrm + 3));
    FEDD_TRY(read_norm(&beta0));
    its = 0;
    relres = beta0 > 0 ? 1.0 : 0.0;
    return 0;
}

// dst = x + M^-1 (V y) with `cols` columns of this cycle (combined: sum_c y_c V_c is already in r)
int Frame::add_correction(int cols, double* dst, bool combined) {
    const double* x = a->x;
    if (!combined) {
        backsolve(cols);
        hipLaunchKernelGGL(k_combine, dim3((unsigned)((n + AX_ROWS - 1) / AX_ROWS)), blk, 0, st, (const double*)V, ldv, n, cols, (const double*)(S + o.y), r);
    }
    if (nr > 1) {
        FEDD_TRY(schwarz_apply_multi(c, r, z, mk));
        hipLaunchKernelGGL(k_axpby, gn, blk, 0, st, 1.0, x, 1.0, (const double*)z, dst, n);
    } else if (a->use_prec) {
        FEDD_TRY(prec_apply(c, r, z, tail));
        if (mk) hipLaunchKernelGGL(k_mask_mix, gn, blk, 0, st, mk, (const double*)z, (const double*)r, z, n);
        hipLaunchKernelGGL(k_axpby, gn, blk, 0, st, 1.0, x, 1.0, (const double*)z, dst, n);
    } else {
        hipLaunchKernelGGL(k_axpby, gn, blk, 0, st, 1.0, x, 1.0, (const double*)r, dst, n);
    }
    return 0;
}

// r = b - A x [one projection step], ||r||^2 -> S[nrm + 3].  use_compact: -1 = the stream the Krylov process runs on;
// 0 = the parity CSR (every stored entry), like fedd_spmv (the compacted stream leaves out sub-ulp cancellation noise)
int Frame::true_residual(double* x, double* ax, bool x_tail, int use_compact, bool proj) {
    FEDD_TRY(residual(x, ax, x_tail, use_compact));
    if (proj) FEDD_TRY(coarse_project(c, a->b, a->x, r, use_compact, 1));
    return norm2(r, S + o.nrm + 3);
}

void Frame::report(int* its_out, double* relres_out) const {
    if (its_out) *its_out = its;
    if (relres_out) *relres_out = relres;
}
int Frame::finish(int* its_out, double* relres_out) {
    FEDD_HIP(hipGetLastError());
    FEDD_HIP(hipStreamSynchronize(st));
    report(its_out, relres_out);
    return 0;
}

namespace {


// The convergence test of the one-vector solvers: iteration j is read on the host while iteration j + 1 is already queued
// (two pinned slots of three doubles -- residual, 1 / norm, norm -- one event each): the device never waits for the host
// round trip.  An iteration queued past convergence only writes basis column j + 2, Hessenberg column j + 1 and
// g[j+1..j+2], none of which the update of x with cols = j + 1 columns reads.
struct LaggedCheck {
    Frame& f;
    // what a breakdown (norm <= 0) that has not converged yields: 2 = the cycle ends and the true residual decides (DCGS2:
    // beta^2 = u.u - s.s <= 0 is a lucky breakdown, or cancellation after the first pass lost orthogonality); 1 = stop
    // (CGS2: ||w|| after both passes, behind the DGKS gate, is a true breakdown)
    const int on_breakdown;
    hipEvent_t ev[2] = {nullptr, nullptr};
    int cols = 0, issued = 0, checked = 0, queued = 0;   // of this cycle: columns read, iterations issued / read / queued

    LaggedCheck(Frame& frame, int breakdown) : f(frame), on_breakdown(breakdown) {}
    ~LaggedCheck() {
        for (int q = 0; q < 2; ++q)
            if (ev[q]) (void)hipEventDestroy(ev[q]);
    }
    int create() {
        for (int q = 0; q < 2; ++q) FEDD_HIP(hipEventCreateWithFlags(&ev[q], hipEventDisableTiming));
        return 0;
    }
    void begin_cycle() {
        cols = checked = queued = 0;
        issued = f.its;
    }
    int check(int jj) {   // 0 = go on, 1 = converged, on_breakdown, < 0 = error
        if (hipEventSynchronize(ev[jj & 1]) != hipSuccess) return -1;
        const double* hp = f.c->h_pinned + 4 * (jj & 1);
        ++f.its;
        ++checked;
        cols = jj + 1;
        f.relres = hp[0] / f.beta0;
        const bool breakdown = !(hp[2] > 0.0);
        return f.relres <= f.a->rtol ? 1 : (breakdown ? on_breakdown : 0);
    }
    // iteration j is in the stream (copy: its three numbers still have to be copied to the host): read iteration j - 1
    int record(int j, bool copy, int* stop) {
        if (copy) FEDD_HIP(hipMemcpyAsync(f.c->h_pinned + 4 * (j & 1), f.S + f.o.misc, 3 * sizeof(double), hipMemcpyDeviceToHost, f.st));
        FEDD_HIP(hipEventRecord(ev[j & 1], f.st));
        ++issued;
        ++queued;
        if (j > 0) {
            *stop = check(j - 1);
            FEDD_CHECK(*stop >= 0, "gmres: waiting for iteration %d failed", j - 1);
        }
        return 0;
    }
    int drain(int* stop) {   // end of the cycle: the iteration still in flight
        if (!*stop && checked < queued) {
            *stop = check(queued - 1);
            FEDD_CHECK(*stop >= 0, "gmres: waiting for iteration %d failed", queued - 1);
        }
        return 0;
    }
};

}  // namespace

// GMRES with the delayed second Gram-Schmidt pass (kernels and formulas above).  Same iterates as
// the two-pass variant below in exact arithmetic; one operator application more per restart cycle
// (the lag), half the passes over the basis and one all-reduce per iteration.
static int gmres_solve_dcgs2(fedd_ctx* c, const GmresCall& call, int* its_out, double* relres_out) {
    Frame f;
    FEDD_TRY(f.setup(c, call, true));
    const int64_t n = f.n, ldv = f.ldv;
    const int m = f.m, nblk = f.nblk, nblk2 = f.nblk2, max_it = call.max_it;
    const Off o = f.o;
    Off2 o2;
    o2.Hraw = f.p; f.p += (m + 1) * m;
    o2.hp = f.p; f.p += m + 2;
    o2.st = f.p; f.p += 2 * m + 4;
    o2.cf = f.p; f.p += 2 * m + 4;
    FEDD_TRY(f.alloc(std::max((size_t)(2 * m + 4) * nblk * 2, (size_t)nblk2), false));
    double* S = f.S;
    double* V = f.V;
    double* u = f.w0;    // first-pass result / next basis vector before its second pass
    double* wt = f.w1;   // B u
    double* r = f.r;
    const dim3 blk = f.blk;
    hipStream_t st = f.st;

    FEDD_TRY(f.start(wt, -1));
    if (!(f.beta0 > 0)) {
        f.report(its_out, relres_out);
        return 0;
    }
    LaggedCheck lag(f, 2);
    FEDD_TRY(lag.create());
    // launch shape of k_multidot2: 2048 rows per workgroup, one grid row per group of 8 columns.
    // Measured alternatives on cfg 2 (ms per step): 1024 rows 43.9, column groups looped inside one
    // grid row 46.4 (2048 rows) / 44.5 (1024 rows), 2 or 4 grid rows 42.7-44.6; this one 43.1.
    // grid rows of k_multidot2 = column groups in flight per row block: every workgroup reads its rows of u and B u once
    // and keeps them across its column groups, so fewer grid rows = fewer re-reads of those two vectors (PMC: 1.24x the
    // algorithmic bytes with one group per workgroup at 214^3); enough of them to fill the GPU when the vectors are short
    const int nblkd = (int)((n + 2047) / 2048);
    const int md2_gy = c->md2_gy > 0 ? c->md2_gy : (int)std::max<int64_t>(1, (2048 + nblkd - 1) / nblkd);
    bool converged = false;
    while (!converged && f.its < max_it) {
        // v_1 = r / ||r||, then the (not delayed) first pass of B v_1: hp = v_1 . w, u = w - v_1 hp
        hipLaunchKernelGGL(k_cycle_init, dim3(1), dim3(1), 0, st, S, o, m, (const double*)(S + o.nrm + 3));
        f.first_basis_vector();
        FEDD_TRY(f.apply(V, u));
        {
            ScopedTimer t(c, FEDD_T_ORTHO);
            hipLaunchKernelGGL(k_multidot, dim3(nblk, 1), blk, 0, st, (const double*)V, ldv, n, 1, (const double*)u,
                               c->d_part.p, nblk, (const int32_t*)nullptr);
            f.reduce_cols(1, S + o2.hp, nblk);
            FEDD_TRY(allreduce_sum(c, S + o2.hp, 1));
            hipLaunchKernelGGL(k_multiaxpy, dim3(nblk2), blk, 0, st, (const double*)V, ldv, n, 1, (const double*)(S + o2.hp),
                               u, c->d_part.p, (const int32_t*)nullptr);
            t.stop();
        }
        lag.begin_cycle();
        int stop = 0;   // 1: converged, 2: breakdown
        for (int j = 0; j < m && lag.issued < max_it && !stop; ++j) {
            const int k = j + 1;  // basis vectors final before this step; the step finalises column j of H
            FEDD_TRY(f.apply(u, wt, true));
            {
                ScopedTimer t(c, FEDD_T_ORTHO);
                const int ncg = (k + 1 + MD2_CG - 1) / MD2_CG;
                ScopedTimer td(c, FEDD_T_GS_DOT);
                td.bytes(8.0 * (double)n * (k + 2));   // k basis columns, u, B u
                hipLaunchKernelGGL(k_multidot2<4>, dim3(nblkd, std::min(md2_gy, ncg)), blk, 0, st, (const double*)V, ldv, n,
                                   k, (const double*)u, (const double*)wt, c->d_part.p, nblkd);
                td.stop();
                f.reduce_cols(2 * k + 2, S + o2.st, nblkd);
                FEDD_TRY(allreduce_sum(c, S + o2.st, 2 * k + 2));
                hipLaunchKernelGGL(k_dcgs2_small, dim3(1), blk, (size_t)(6 * m + 8) * sizeof(double), st, S, o, o2, k, m,
                                   c->h_pinned_dev ? c->h_pinned_dev + 4 * (j & 1) : (double*)nullptr);
                if (k < m) {  // the last step of a cycle needs no further basis vector
                    ScopedTimer tu(c, FEDD_T_GS_UPDATE);
                    tu.bytes(8.0 * (double)n * (k + 4));   // k basis columns, u and B u in, v_{k+1} and the next u out
                    hipLaunchKernelGGL(k_axpy2, dim3(nblk2), blk, 0, st, V, ldv, n, k, (const double*)(S + o2.cf), m, u,
                                       (const double*)wt);
                    tu.stop();
                }
                t.stop();
            }
            FEDD_TRY(lag.record(j, !c->h_pinned_dev, &stop));
        }
        FEDD_TRY(lag.drain(&stop));
        converged = stop == 1;
        const bool broke = stop == 2;   // only the implicit residual says "converged"; here the true residual decides
        FEDD_TRY(f.add_correction(lag.cols, call.x));   // the columns whose results the host has read
        if (!converged && (f.its < max_it || broke)) {
            FEDD_TRY(f.true_residual(call.x, r, false, -1, f.project));
            if (broke) {   // rare path: the host reads the true residual
                double ta = 0.0;
                FEDD_TRY(f.read_norm(&ta));
                f.relres = ta / f.beta0;
                if (f.relres <= call.rtol) converged = true;
            }
        }
    }
    return f.finish(its_out, relres_out);
}

// GMRES with classical Gram-Schmidt in two passes (gmres_kind 1): fused multi-dot + multi-axpy twice, the second pass gated
// by the DGKS test on the device.  The work vectors have no ghost tail here.
static int gmres_solve_cgs2(fedd_ctx* c, const GmresCall& call, int* its_out, double* relres_out) {
    Frame f;
    FEDD_TRY(f.setup(c, call, false));
    const int64_t n = f.n, ldv = f.ldv;
    const int m = f.m, nblk = f.nblk, nblk2 = f.nblk2, max_it = call.max_it;
    const Off o = f.o;
    FEDD_TRY(f.alloc(std::max((size_t)(m + 2) * nblk, (size_t)nblk2), false));
    FEDD_TRY(c->d_flags.ensure(16));
    int32_t* gate = c->d_flags.p + 2;
    double* S = f.S;
    double* V = f.V;
    double* w = f.w0;
    double* r = f.r;
    const dim3 gn = f.gn, blk = f.blk;
    hipStream_t st = f.st;

    FEDD_TRY(f.start(r, -1));
    if (!(f.beta0 > 0)) {
        f.report(its_out, relres_out);
        return 0;
    }
    LaggedCheck lag(f, 1);
    FEDD_TRY(lag.create());
    int stop = 0;   // 1: converged or breakdown
    while (!stop && f.its < max_it) {
        hipLaunchKernelGGL(k_cycle_init, dim3(1), dim3(1), 0, st, S, o, m, (const double*)(S + o.nrm + 3));
        f.first_basis_vector();
        lag.begin_cycle();
        for (int j = 0; j < m && lag.issued < max_it && !stop; ++j) {
            FEDD_TRY(f.apply(V + (int64_t)j * ldv, w));
            {
                ScopedTimer t(c, FEDD_T_ORTHO);
                // pass 1: h1 = V^T w, nrm[0] = w.w ; w -= V h1, nrm[1] = ||w||^2
                hipLaunchKernelGGL(k_multidot, dim3(nblk, (j + 2 + MD_CG - 1) / MD_CG), blk, 0, st, (const double*)V, ldv, n,
                                   j + 1, (const double*)w, c->d_part.p, nblk, (const int32_t*)nullptr);
                f.reduce_cols(j + 2, S + o.h1, nblk);
                FEDD_TRY(allreduce_sum(c, S + o.h1, j + 2));
                // h1[j+1] now holds w.w: gate and the norm after pass 1 follow from h1 alone
                hipLaunchKernelGGL(k_dgks_gate, dim3(1), dim3(1), 0, st, (const double*)(S + o.h1), j, gate, S + o.nrm + 1);
                hipLaunchKernelGGL(k_multiaxpy, dim3(nblk2), blk, 0, st, (const double*)V, ldv, n, j + 1,
                                   (const double*)(S + o.h1), w, c->d_part.p, (const int32_t*)nullptr);
                // pass 2 (gated on the device; on several ranks the gate is identical everywhere
                // because it is computed from all-reduced numbers, so the collectives stay matched)
                hipLaunchKernelGGL(k_multidot, dim3(nblk, (j + 2 + MD_CG - 1) / MD_CG), blk, 0, st, (const double*)V, ldv, n,
                                   j + 1, (const double*)w, c->d_part.p, nblk, (const int32_t*)gate);
                f.reduce_cols(j + 1, S + o.h2, nblk, gate);
                FEDD_TRY(allreduce_sum(c, S + o.h2, j + 1));
                hipLaunchKernelGGL(k_multiaxpy, dim3(nblk2), blk, 0, st, (const double*)V, ldv, n, j + 1,
                                   (const double*)(S + o.h2), w, c->d_part.p, (const int32_t*)gate);
                if (c->nranks > 1) {
                    f.reduce_cols(1, S + o.nrm + 2, nblk2, gate);
                    FEDD_TRY(allreduce_sum(c, S + o.nrm + 2, 1));
                }
                t.stop();
            }
            hipLaunchKernelGGL(k_givens, dim3(1), dim3(256), (size_t)(3 * m + 2) * sizeof(double), st, S, o, j, m,
                               (const int32_t*)gate, (const double*)(c->nranks > 1 ? nullptr : c->d_part.p), nblk2);
            hipLaunchKernelGGL(k_scale_to, gn, blk, 0, st, (const double*)w, (const double*)(S + o.misc + 1),
                               V + (int64_t)(j + 1) * ldv, n);
            FEDD_TRY(lag.record(j, true, &stop));
        }
        FEDD_TRY(lag.drain(&stop));
        FEDD_TRY(f.add_correction(lag.cols, call.x));
        if (!stop && f.its < max_it) FEDD_TRY(f.true_residual(call.x, r, false, -1, f.project));
    }
    return f.finish(its_out, relres_out);
}

int gmres_solve(fedd_ctx* c, const GmresCall& call, int* its_out, double* relres_out) {
    c->gmres_floor = 0;
    c->gmres_rec_relres = -1.0;
    FEDD_CHECK(call.nr <= 1 || c->gmres_kind == 2, "gmres: a stacked solve (%d right-hand sides) needs the s-step solver (gmres_kind 2)", call.nr);
    if (c->gm_cap.armed >= 0 && (c->gmres_kind != 2 || call.nr > 1 || c->nranks > 1)) {
        c->gm_cap.armed = -1;
        FEDD_CHECK(c->nranks == 1, "gmres capture: one rank only (this context has %d)", c->nranks);
        FEDD_CHECK(call.nr <= 1, "gmres capture: not for the stacked solve (%d right-hand sides)", call.nr);
        FEDD_CHECK(false, "gmres capture: the s-step solver only (gmres_kind 2; %d is set and keeps no raw Hessenberg matrix)", c->gmres_kind);
    }
    if (c->gmres_kind == 0) return gmres_solve_dcgs2(c, call, its_out, relres_out);
    if (c->gmres_kind == 1) return gmres_solve_cgs2(c, call, its_out, relres_out);
    // block length: "gmres_s" 0 = by the vector length per rank -- 16-vector (Newton-basis) blocks where the sweeps over the
    // basis dominate, 8-vector blocks on short vectors, where the longer blocks' fixed costs (two monomial blocks first,
    // a 16 x 16 Cholesky per pass, one more vector per SpMV) are not paid back.  Measured: 1.03 M rows / 71 iterations (cfg 2)
    // 11.8 ms with 8, 12.2 with 16; 1.26 M rows / 145 iterations (one GPU's share of cfg 3) 24.4 against 22.5; 9.9 M rows
    // 122.5 against 108.0.  Every rank must take the same one: the decision uses the global row count
    int s = c->gmres_s;
    if (s == 0) {
        double ng = (double)c->n_rows;
        if (c->nranks > 1) {
            FEDD_TRY(c->d_small.ensure(std::max<size_t>(16, c->d_small.cap)));
            FEDD_HIP(hipMemcpyAsync(c->d_small.p, &ng, sizeof(double), hipMemcpyHostToDevice, c->stream));
            FEDD_HIP(hipStreamSynchronize(c->stream));
            FEDD_TRY(allreduce_sum(c, c->d_small.p, 1));
            FEDD_HIP(hipMemcpyAsync(&ng, c->d_small.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            FEDD_HIP(hipStreamSynchronize(c->stream));
        }
        s = ng / c->nranks >= 1.2e6 ? 16 : 8;
    }
    c->gmres_s_used = s;
    // the 8-column kernels for longer blocks too: the constrained solves run monomial blocks of at most eight vectors; in
    // cycles of more than 800 vectors the 16-column block kernel's LDS image of its new Hessenberg columns does not fit
    if (s > 8 && (call.mask || std::min(call.restart, call.max_it) > 800)) s = 8;
    return gmres_solve_sstep(c, call, s, its_out, relres_out);
}

}  // namespace fedd
