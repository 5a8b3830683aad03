// Nonlinear elasticity: tangent and internal forces of a hyperelastic material for a displacement u given at the nodes
// (d_vel, dim * node + d): FE::assemblyElasticityJacobianAndStressAceFEM (feddlib/core/FE/FE_def.hpp:837-1291; element loop
// :1123-1267 in 3D, :928-1066 in 2D).  gfx950 only.
//
// Per element T and quadrature point p of the rule determineDegree(dim, FEType, FEType, Grad, Grad) (P1: one point, P2: degree 2)
//   g_i = B^-T grad phi_i(x_p),  F = I + sum_i u_i (x) g_i                                    (:1143-1156)
//   P(F) first Piola-Kirchhoff stress, A[i][j][k][l] = dP_ij / dF_kl of the material          (:1176-1181)
//   f_(i,d)          += |det B| w_p sum_k  P_dk g_i,k                                         (:1229-1243, 1251-1253)
//   K_(i,d1),(j,d2)  += |det B| w_p sum_kl g_i,k A[d1][k][d2][l] g_j,l                        (:1200-1222, 1258-1262)
// The materials are written from their closed forms (the reference's routines nh3d, mr3d, stvk3d, stvk2d are machine-generated
// evaluations of the same): with C = F^T F, b = F F^T, G = F^-T, J = det F, I1 = tr C
//   Neo-Hooke               P = mu (F - G) + lambda ln J G
//                           A_ijkl = mu d_ik d_jl + lambda G_ij G_kl + (mu - lambda ln J) G_il G_kj
//   Mooney-Rivlin           P = (1 - c) mu (F - G) + c mu (I1 F - F C - 2 G) + kappa ln J G        (each bracket is exactly 0 at F = I)
//                           A_ijkl = (1 - c) mu d_ik d_jl + c mu (2 F_ij F_kl + I1 d_ik d_jl - d_ik C_lj - F_il F_kj - d_jl b_ik)
//                                    + kappa G_ij G_kl + (mu (1 + c) - kappa ln J) G_il G_kj
//   Saint Venant-Kirchhoff  S = lambda tr(E) I + 2 mu E, E = (C - I) / 2, P = F S
//                           A_ijkl = d_ik S_lj + lambda F_ij F_kl + mu (F_il F_kj + b_ik d_jl)
// A is major-symmetric (A_ijkl = A_klij): the 45 (2D: 10) entries with ij <= kl are evaluated and mirrored.
//
// Element-major like k_adv_elem, ONE ELEMENT PER WAVEFRONT, four phases per element with the intermediate results in LDS:
//   1  lanes over (p, i):            the transformed gradients g_i(x_p)
//   2  lane p:                       F, J, the material: w_p P and w_p A  (the weight is folded in here; the reference multiplies
//                                    the point's element matrix by it, :1219, 1240)
//   3  lanes over (p, j, d1, k):     H_j[d1][k][d2] = sum_l w_p A[d1][k][d2][l] g_j,l
//   4  lanes over (i, j):            the dim x dim block sum_p sum_k g_i,k H_j[d1][k][d2], times |det B| -> ke[T][i][j][d1][d2];
//      lanes over (i, d):            sum_p sum_k w_p P_dk g_i,k, times |det B|                           -> fe[T][i][d]
// The rows are then summed by gather lists (gather_lists.hpp; on the system's FULL pattern, built once per pattern): the tangent as in
// k_adv_gather, the force by a thread per node over its adjacency.  Every sum runs in a fixed order and there is no
// floating-point atomic: two calls agree bit for bit, and so do tangent-only and force-only calls with the combined one (the
// same instructions produce each).  The one atomic is the integer minimum that records an inverted element.
#include "assemble_common.hpp"
#include "gather_lists.hpp"
#include <algorithm>
#include <climits>
#include <cmath>

namespace fedd {
namespace {

struct HyArgs {
    const int32_t* conn;
    const double* xyz;
    const double* u;
    const double* tab;      // w[nq] | dphi[nq * NEN * DIM]
    int nq, model, what;
    double p0, p1, p2;      // Neo-Hooke: mu, lambda; Mooney-Rivlin: mu, kappa, c; Saint Venant-Kirchhoff: lambda, mu
    int32_t* flag;
};

// G = F^-T = cof(F) / det F; returns det F (G is not written when det F <= 0)
template <int D>
__device__ __forceinline__ double cof_inv_t(const double (&F)[D][D], double (&G)[D][D]) {
    double cf[D][D];
    double det;
    if constexpr (D == 2) {
        cf[0][0] = F[1][1]; cf[0][1] = -F[1][0];
        cf[1][0] = -F[0][1]; cf[1][1] = F[0][0];
        det = F[0][0] * F[1][1] - F[0][1] * F[1][0];
    } else {
        cf[0][0] = F[1][1] * F[2][2] - F[1][2] * F[2][1];
        cf[0][1] = F[1][2] * F[2][0] - F[1][0] * F[2][2];
        cf[0][2] = F[1][0] * F[2][1] - F[1][1] * F[2][0];
        cf[1][0] = F[0][2] * F[2][1] - F[0][1] * F[2][2];
        cf[1][1] = F[0][0] * F[2][2] - F[0][2] * F[2][0];
        cf[1][2] = F[0][1] * F[2][0] - F[0][0] * F[2][1];
        cf[2][0] = F[0][1] * F[1][2] - F[0][2] * F[1][1];
        cf[2][1] = F[0][2] * F[1][0] - F[0][0] * F[1][2];
        cf[2][2] = F[0][0] * F[1][1] - F[0][1] * F[1][0];
        det = F[0][0] * cf[0][0] + F[0][1] * cf[0][1] + F[0][2] * cf[0][2];
    }
    if (det > 0.0) {
        const double r = 1.0 / det;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) G[i][j] = cf[i][j] * r;
    }
    return det;
}

// wq P -> Ps[D * D], wq A -> As[(i D + j) D D + k D + l]; false (nothing written) where the law takes ln J and J <= 0
template <int D>
__device__ __forceinline__ bool material(const HyArgs& a, const double (&F)[D][D], double wq, double* __restrict__ Ps,
                                         double* __restrict__ As) {
    constexpr int DD = D * D;
    double Cm[D][D], b[D][D];
    double I1 = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double s = 0.0, t = 0.0;
#pragma unroll
            for (int m = 0; m < D; ++m) {
                s += F[m][i] * F[m][j];
                t += F[i][m] * F[j][m];
            }
            Cm[i][j] = s;
            b[i][j] = t;
            if (i == j) I1 += s;
        }
    if (a.model == FEDD_HYPER_STVK) {
        const double lam = a.p0, mu = a.p1;
        double trE = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) trE += 0.5 * (Cm[i][i] - 1.0);
        double S[D][D];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) S[i][j] = (i == j ? lam * trE : 0.0) + mu * (Cm[i][j] - (i == j ? 1.0 : 0.0));
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < D; ++m) s += F[i][m] * S[m][j];
                Ps[i * D + j] = wq * s;
            }
#pragma unroll
        for (int ij = 0; ij < DD; ++ij)
#pragma unroll
            for (int kl = ij; kl < DD; ++kl) {
                const int i = ij / D, j = ij % D, k = kl / D, l = kl % D;
                double v = lam * F[i][j] * F[k][l] + mu * (F[i][l] * F[k][j] + (j == l ? b[i][k] : 0.0));
                if (i == k) v += S[l][j];
                v *= wq;
                As[ij * DD + kl] = v;
                As[kl * DD + ij] = v;
            }
        return true;
    }
    double G[D][D];
    const double J = cof_inv_t<D>(F, G);
    if (!(J > 0.0)) return false;
    const double lnJ = log(J);
    if (a.model == FEDD_HYPER_NEOHOOKE) {
        const double mu = a.p0, lam = a.p1;
        const double cg = mu - lam * lnJ;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) Ps[i * D + j] = wq * (mu * (F[i][j] - G[i][j]) + lam * lnJ * G[i][j]);
#pragma unroll
        for (int ij = 0; ij < DD; ++ij)
#pragma unroll
            for (int kl = ij; kl < DD; ++kl) {
                const int i = ij / D, j = ij % D, k = kl / D, l = kl % D;
                double v = lam * G[i][j] * G[k][l] + cg * G[i][l] * G[k][j];
                if (ij == kl) v += mu;
                v *= wq;
                As[ij * DD + kl] = v;
                As[kl * DD + ij] = v;
            }
        return true;
    }
    // Mooney-Rivlin
    const double mu = a.p0, kap = a.p1, cc = a.p2;
    const double c1 = (1.0 - cc) * mu, c2 = cc * mu;
    const double cg = mu * (1.0 + cc) - kap * lnJ;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double fc = 0.0;
#pragma unroll
            for (int m = 0; m < D; ++m) fc += F[i][m] * Cm[m][j];
            Ps[i * D + j] = wq * (c1 * (F[i][j] - G[i][j]) + c2 * (I1 * F[i][j] - fc - 2.0 * G[i][j]) + kap * lnJ * G[i][j]);
        }
#pragma unroll
    for (int ij = 0; ij < DD; ++ij)
#pragma unroll
        for (int kl = ij; kl < DD; ++kl) {
            const int i = ij / D, j = ij % D, k = kl / D, l = kl % D;
            double m2 = 2.0 * F[i][j] * F[k][l] - F[i][l] * F[k][j];
            if (i == k) m2 -= Cm[l][j];
            if (j == l) m2 -= b[i][k];
            if (ij == kl) m2 += I1;
            double v = c2 * m2 + kap * G[i][j] * G[k][l] + cg * G[i][l] * G[k][j];
            if (ij == kl) v += c1;
            v *= wq;
            As[ij * DD + kl] = v;
            As[kl * DD + ij] = v;
        }
    return true;
}

template <int DIM, int NEN>
__global__ __launch_bounds__(256) void k_hyper_elem(HyArgs a, int64_t n_elem, double* __restrict__ ke, double* __restrict__ fe) {
    constexpr int DD = DIM * DIM, D3 = DD * DIM, D4 = DD * DD;
    extern __shared__ double sm[];
    const int nq = a.nq;
    const int ntab = nq * (1 + NEN * DIM);
    const double* s_w = sm;
    const double* s_dphi = sm + nq;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int per_wave = NEN * DIM + nq * (NEN * DIM + DD + D4 + NEN * D3);
    double* Us = sm + ntab + (size_t)w * per_wave;      // this wave's displacements [i][d]
    double* Gs = Us + NEN * DIM;                        // g_i(x_p) [p][i][k]
    double* Ps = Gs + nq * NEN * DIM;                   // w_p P [p][d][k]
    double* As = Ps + nq * DD;                          // w_p A [p][d1 k][d2 l]
    double* Hs = As + nq * D4;                          // H [p][j][d1][k][d2]
    for (int i = tid; i < ntab; i += 256) sm[i] = a.tab[i];
    __syncthreads();
    const int64_t nwave = (int64_t)gridDim.x * 4;
    const int64_t trips = (n_elem + nwave - 1) / nwave;
    for (int64_t t0 = 0; t0 < trips; ++t0) {
        const int64_t e = t0 * nwave + (int64_t)blockIdx.x * 4 + w;
        const bool on = e < n_elem;
        double xv = 0.0;
        if (on && lane < (DIM + 1) * DIM) xv = a.xyz[(int64_t)a.conn[e * NEN + lane / DIM] * DIM + (lane % DIM)];
        if (on && lane < NEN * DIM) Us[lane] = a.u[(int64_t)a.conn[e * NEN + lane / DIM] * DIM + (lane % DIM)];
        double X[DIM + 1][DIM];
#pragma unroll
        for (int v = 0; v <= DIM; ++v)
#pragma unroll
            for (int d = 0; d < DIM; ++d) X[v][d] = __shfl(xv, v * DIM + d, 64);
        double Binv[DIM][DIM];
        const double absdet = on ? fabs(affine<DIM>(X, Binv)) : 0.0;
        if (on)
            for (int t = lane; t < nq * NEN; t += 64) {
                double g[DIM];
                grad_t<DIM, NEN>(s_dphi, t / NEN, t % NEN, Binv, g);
#pragma unroll
                for (int d = 0; d < DIM; ++d) Gs[t * DIM + d] = g[d];
            }
        __syncthreads();        // Us, Gs
        if (on)
            for (int q = lane; q < nq; q += 64) {
                double F[DIM][DIM];
#pragma unroll
                for (int d = 0; d < DIM; ++d)
#pragma unroll
                    for (int k = 0; k < DIM; ++k) F[d][k] = d == k ? 1.0 : 0.0;
                for (int i = 0; i < NEN; ++i)
#pragma unroll
                    for (int d = 0; d < DIM; ++d)
#pragma unroll
                        for (int k = 0; k < DIM; ++k) F[d][k] += Us[i * DIM + d] * Gs[(q * NEN + i) * DIM + k];
                if (!material<DIM>(a, F, s_w[q], Ps + q * DD, As + q * D4)) {
                    atomicMin(a.flag, (int32_t)e);
                    for (int m = 0; m < DD; ++m) Ps[q * DD + m] = 0.0;
                    for (int m = 0; m < D4; ++m) As[q * D4 + m] = 0.0;
                }
            }
        __syncthreads();        // Ps, As
        if (on && (a.what & FEDD_HYPER_TANGENT))
            for (int t = lane; t < nq * NEN * DD; t += 64) {
                const int dk = t % DD, qj = t / DD;     // (d1, k); (p, j)
                const double* __restrict__ Aq = As + (qj / NEN) * D4 + dk * DD;
                const double* __restrict__ gj = Gs + qj * DIM;
#pragma unroll
                for (int d2 = 0; d2 < DIM; ++d2) {
                    double s = 0.0;
#pragma unroll
                    for (int l = 0; l < DIM; ++l) s += Aq[d2 * DIM + l] * gj[l];
                    Hs[t * DIM + d2] = s;
                }
            }
        __syncthreads();        // Hs
        if (on) {
            if (a.what & FEDD_HYPER_TANGENT) {
                double* __restrict__ out = ke + e * (NEN * NEN * DD);
                for (int t = lane; t < NEN * NEN; t += 64) {
                    const int i = t / NEN, j = t - i * NEN;
                    double blk[DD];
#pragma unroll
                    for (int m = 0; m < DD; ++m) blk[m] = 0.0;
                    for (int q = 0; q < nq; ++q) {
                        const double* __restrict__ gi = Gs + (q * NEN + i) * DIM;
                        const double* __restrict__ Hj = Hs + (q * NEN + j) * D3;
#pragma unroll
                        for (int d1 = 0; d1 < DIM; ++d1)
#pragma unroll
                            for (int k = 0; k < DIM; ++k)
#pragma unroll
                                for (int d2 = 0; d2 < DIM; ++d2) blk[d1 * DIM + d2] += gi[k] * Hj[(d1 * DIM + k) * DIM + d2];
                    }
#pragma unroll
                    for (int m = 0; m < DD; ++m) out[t * DD + m] = absdet * blk[m];
                }
            }
            if ((a.what & FEDD_HYPER_FORCE) && lane < NEN * DIM) {
                const int i = lane / DIM, d = lane - i * DIM;
                double s = 0.0;
                for (int q = 0; q < nq; ++q)
#pragma unroll
                    for (int k = 0; k < DIM; ++k) s += Ps[q * DD + d * DIM + k] * Gs[(q * NEN + i) * DIM + k];
                fe[e * (NEN * DIM) + lane] = absdet * s;
            }
        }
        __syncthreads();        // the wave's LDS is rewritten by the next trip
    }
}

// rows of the system's FULL pattern from the element blocks, in the order of the gather lists.  MASS != 0 (the time tangent of
// fedd_assemble_hyperelastic_time): (cm * M) + K is stored, the product and the sum rounded on their own as k_combine_same
// (MASS 1: M on the same FULL pattern) and k_combine_diag (MASS 2: M on the DIAG node-block pattern, one entry per slot in the
// same slot order; an entry M does not have counts as 0.0 and is still multiplied and added) round them.  The mass entries of
// a slot are loaded before its sources are walked.  From here to the end of the file no product is fused with a sum (the
// kernels above this line keep the compiler's default; the ones below contain no other product followed by a sum).
#pragma clang fp contract(off)

struct HyMass {
    int kind = 0;                   // 0 = none, 1 = same pattern, 2 = DIAG into FULL
    const int32_t* rowptr = nullptr;
    const double* val = nullptr;
    double cm = 0.0;
    int64_t nnz = 0;
};

// one DIM x DIM block per source (gather_lists.hpp).  This struct stays below the pragma above: store() forms cm * M and + K as
// two roundings.  The mass entries of the slot are loaded before its sources are walked.
template <int DIM, int NEN, int MASS>
struct HyperSum : GatherBlockSum<NEN, DIM * DIM> {
    const int32_t* m_rowptr;
    const double* m_val;
    double cm;
    double* val;
    double mv[MASS == 1 ? DIM * DIM : DIM];
    __device__ void init(const GatherRow& g, int sl) {
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
            if (MASS == 1) {
#pragma unroll
                for (int cc = 0; cc < DIM; ++cc) mv[r * DIM + cc] = m_val[(int64_t)g.rs + (int64_t)r * g.nslot * DIM + (int64_t)sl * DIM + cc];
            }
            if (MASS == 2) {
                const int32_t ms = m_rowptr[g.row + r];
                mv[r] = sl < m_rowptr[g.row + r + 1] - ms ? m_val[ms + sl] : 0.0;
            }
        }
        this->zero();
    }
    __device__ void store(const GatherRow& g, int sl) {
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
            const int64_t at = (int64_t)g.rs + (int64_t)r * g.nslot * DIM + (int64_t)sl * DIM;
#pragma unroll
            for (int cc = 0; cc < DIM; ++cc) {
                double v = this->acc[r * DIM + cc];
                if (MASS != 0) {
                    const double pm = cm * (MASS == 1 ? mv[r * DIM + cc] : cc == r ? mv[r] : 0.0);
                    v = pm + v;
                }
                val[at + cc] = v;
            }
        }
    }
};

template <int DIM, int NEN, int MASS>
__global__ __launch_bounds__(256) void k_hyper_gather(const int32_t* __restrict__ n2e_ptr, const int32_t* __restrict__ n2e,
                                                      const int32_t* __restrict__ rowptr, int32_t nn,
                                                      const uint16_t* __restrict__ soff, const uint16_t* __restrict__ src,
                                                      const double* __restrict__ ke, const int32_t* __restrict__ m_rowptr,
                                                      const double* __restrict__ m_val, double cm, double* __restrict__ val) {
    gather_walk<NEN>(n2e_ptr, n2e, soff, src, nn, GatherRows{rowptr, DIM, 1}, HyperSum<DIM, NEN, MASS>{{ke}, m_rowptr, m_val, cm, val});
}

// f_(p,d) = sum over the adjacency of node p, in its order, of the element forces
template <int DIM>
__global__ void k_hyper_force(const int32_t* __restrict__ n2e_ptr, const int32_t* __restrict__ n2e, int32_t nn,
                              const double* __restrict__ fe, double* __restrict__ f) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nn) return;
    double acc[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) acc[d] = 0.0;
    for (int32_t q = n2e_ptr[p]; q < n2e_ptr[p + 1]; ++q) {
        const double* __restrict__ s = fe + (int64_t)n2e[q] * DIM;
#pragma unroll
        for (int d = 0; d < DIM; ++d) acc[d] += s[d];
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) f[p * DIM + d] = acc[d];
}

template <int DIM, int NEN>
int launch_hyper(fedd_ctx* c, HyArgs a, const HyMass& mass, const char* who) {
    constexpr int DD = DIM * DIM;
    const int64_t nn = c->n_own;
    const int ntab = a.nq * (1 + NEN * DIM);
    const int per_wave = NEN * DIM + a.nq * (NEN * DIM + DD + DD * DD + NEN * DD * DIM);
    const size_t lds = ((size_t)ntab + 4 * (size_t)per_wave) * sizeof(double);
    FEDD_CHECK(lds <= 64 * 1024, "%s: the element workspace (%zu bytes) does not fit the LDS", who, lds);
    int32_t h_flag = INT32_MAX;
    FEDD_HIP(hipMemsetD32Async((hipDeviceptr_t)a.flag, INT32_MAX, 1, c->stream));
    ScopedTimer t(c, FEDD_T_ASSEMBLE);
    // byte model: geometry, u and connectivity once per element; the element blocks and forces written and read once; the values
    // and the force vector written; the time tangent reads the mass values once more (DIAG: with their row pointers)
    const bool kt = a.what & FEDD_HYPER_TANGENT, kf = a.what & FEDD_HYPER_FORCE;
    const double mass_bytes = !kt || mass.kind == 0 ? 0.0 : (double)mass.nnz * 8.0 + (mass.kind == 2 ? 4.0 * (double)(nn * DIM + 1) : 0.0);
    // (stated before the first stop: a resumed timer counts time, not another launch's bytes)
    t.bytes((double)c->n_elem * (NEN * 4.0 + (kt ? 2.0 * NEN * NEN * DD * 8.0 : 0.0) + (kf ? 2.0 * NEN * DIM * 8.0 : 0.0)) +
            (double)c->n_node * DIM * 16.0 + (kt ? (double)c->nnz * 8.0 : 0.0) + (kf ? (double)nn * DIM * 8.0 : 0.0) + mass_bytes);
    if (c->n_elem > 0) {
        const int64_t nwg = std::min<int64_t>((c->n_elem + 3) / 4, 256 * 8);
        hipLaunchKernelGGL((k_hyper_elem<DIM, NEN>), dim3((unsigned)nwg), dim3(256), lds, c->stream, a, c->n_elem, c->d_adv_ke.p,
                           c->d_hy_fe.p);
    }
    t.stop();
    FEDD_HIP(hipGetLastError());
    // the element pass is complete before anything the caller can read is written: an inverted element leaves the system
    // matrix and the force vector of the previous call as they were
    FEDD_HIP(hipMemcpyAsync(&h_flag, a.flag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_CHECK(h_flag == INT32_MAX,
               "%s: element %d is inverted (det F <= 0 at a quadrature point, and the material takes ln det F); "
               "the system matrix and the force vector were not written", who, h_flag);
    t.resume();
    if (a.what & FEDD_HYPER_TANGENT) {
        system_written(c, SYS_VALUES);
        const dim3 grid2((unsigned)gather_grid(nn)), blk(256);
        const int32_t *n2e_ptr = c->d_n2e_ptr.p, *n2e = c->d_n2e.p, *rowptr = c->d_rowptr.p;
        const uint16_t *soff = c->gl_full.soff.p, *src = c->gl_full.src.p;
        const double* ke = c->d_adv_ke.p;
        auto kern = mass.kind == 0 ? k_hyper_gather<DIM, NEN, 0> : mass.kind == 1 ? k_hyper_gather<DIM, NEN, 1> : k_hyper_gather<DIM, NEN, 2>;
        hipLaunchKernelGGL(kern, grid2, blk, 0, c->stream, n2e_ptr, n2e, rowptr, (int32_t)nn, soff, src, ke, mass.rowptr, mass.val,
                           mass.cm, c->d_val.p);       // (without a mass: null pointers and cm = 0, which that kernel does not read)
    }
    if (a.what & FEDD_HYPER_FORCE) {
        hipLaunchKernelGGL(k_hyper_force<DIM>, dim3((unsigned)std::max<int64_t>(1, (nn + 255) / 256)), dim3(256), 0, c->stream,
                           (const int32_t*)c->d_n2e_ptr.p, (const int32_t*)c->d_n2e.p, (int32_t)nn, (const double*)c->d_hy_fe.p,
                           c->d_hy_f.p);
        c->have_hy_f = true;
        c->nw_f_fresh = true;       // newer than the last fedd_newton_begin / fedd_newton_update (newton.hip)
    }
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}

int assemble_hyper(fedd_ctx* c, int model, const double* params, int n_params, int what, const HyMass& mass, const char* who) {
    FEDD_CHECK(c->nranks == 1, "%s: one rank only for now", who);
    FEDD_CHECK(model == FEDD_HYPER_NEOHOOKE || model == FEDD_HYPER_MOONEY_RIVLIN || model == FEDD_HYPER_STVK,
               "%s: unknown material model %d (built: Neo-Hooke, Mooney-Rivlin, Saint Venant-Kirchhoff)", who, model);
    FEDD_CHECK(what >= 1 && what <= (FEDD_HYPER_TANGENT | FEDD_HYPER_FORCE), "%s: what = %d selects neither tangent nor force", who, what);
    const int dim = c->dim, nen = c->nen;
    FEDD_CHECK(dim == 3 || model == FEDD_HYPER_STVK, "%s: only Saint Venant-Kirchhoff in 2D (FE_def.hpp:903)", who);
    const int want = model == FEDD_HYPER_MOONEY_RIVLIN ? 3 : 2;
    FEDD_CHECK(params && n_params == want, "%s: the model takes %d parameters (%s), %d given", who, want,
               model == FEDD_HYPER_NEOHOOKE ? "E, nu" : model == FEDD_HYPER_MOONEY_RIVLIN ? "E, nu, C" : "lambda, mu", n_params);
    FEDD_CHECK(c->have_pattern && !c->merged && c->dofs == dim && c->block_mode == FEDD_BLOCK_FULL && c->n_rowg == 0,
               "%s: needs the FULL pattern with dim dofs per node (fedd_pattern_build(dim, FEDD_BLOCK_FULL)) as system matrix", who);
    FEDD_CHECK(c->have_vel, "%s: call fedd_velocity_set (the displacement u) first", who);
    HyArgs a;
    a.model = model;
    a.what = what;
    a.p0 = a.p1 = a.p2 = 0.0;
    if (model == FEDD_HYPER_STVK) {
        a.p0 = params[0];
        a.p1 = params[1];
    } else {
        const double E = params[0], nu = params[1];
        FEDD_CHECK(nu > -1.0 && nu < 0.5, "%s: Poisson ratio %g outside (-1, 0.5)", who, nu);
        a.p0 = E / (2.0 * (1.0 + nu));                                              // mu
        if (model == FEDD_HYPER_NEOHOOKE) a.p1 = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu));   // lambda
        else {
            a.p1 = E / (3.0 * (1.0 - 2.0 * nu));                                    // kappa
            a.p2 = params[2];
        }
    }
    if (!c->have_adj) {
        ScopedTimer t(c, FEDD_T_SYMBOLIC);
        FEDD_TRY(build_adjacency(c));
    }
    FEDD_TRY(full_lists_ensure(c, who));    // determineDegree(dim, FEType, FEType, Grad, Grad) (FE_def.hpp:856)
    if (what & FEDD_HYPER_TANGENT) FEDD_TRY(c->d_adv_ke.ensure((size_t)c->n_elem * nen * nen * dim * dim));
    FEDD_TRY(c->d_hy_fe.ensure((size_t)c->n_elem * nen * dim));
    FEDD_TRY(c->d_hy_f.ensure((size_t)c->n_own * dim));
    FEDD_TRY(c->d_hy_flag.ensure(1));
    a.conn = c->d_conn.p; a.xyz = c->d_xyz.p; a.u = c->d_vel.p; a.tab = c->d_hy_tab.p;
    a.nq = c->hy_nq;
    a.flag = c->d_hy_flag.p;
    return with_element(dim, nen, [&](auto d, auto n) { return launch_hyper<decltype(d)::value, decltype(n)::value>(c, a, mass, who); });
}

}  // namespace

int assemble_hyperelastic(fedd_ctx* c, int model, const double* params, int n_params, int what) {
    return assemble_hyper(c, model, params, n_params, what, HyMass(), "fedd_assemble_hyperelastic");
}

// the same with (cm * M[slot_m]) + K(u) as tangent: the pairings of fedd_matrix_combine (timestep.hip combine_pairing) with the
// system matrix in the place of slot_a
int assemble_hyperelastic_time(fedd_ctx* c, int model, const double* params, int n_params, int what, int slot_m, double cm) {
    const char* who = "fedd_assemble_hyperelastic_time";
    FEDD_CHECK(c->nranks == 1, "%s: one rank only (a context with %d ranks was given)", who, c->nranks);
    const DevCsr& M = c->aux[slot_m];
    FEDD_CHECK(M.valid, "%s: slot %d is empty", who, slot_m);
    FEDD_CHECK(M.mesh_id == c->mesh_id, "%s: slot %d must hold a matrix of the current mesh (a fedd_mesh_set came between)", who, slot_m);
    FEDD_CHECK(c->have_pattern && !c->merged && c->dofs == c->dim && c->block_mode == FEDD_BLOCK_FULL && c->n_rowg == 0,
               "%s: needs the FULL pattern with dim dofs per node (fedd_pattern_build(dim, FEDD_BLOCK_FULL)) as system matrix", who);
    FEDD_CHECK(M.block_mode >= 0 && M.dofs == c->dofs && M.n_rows == c->n_rows && M.n_cols == c->n_cols,
               "%s: slot %d and the system matrix do not hold matrices of one space built by fedd_pattern_build", who, slot_m);
    HyMass mass;
    if (M.block_mode == FEDD_BLOCK_FULL && M.nnz == c->nnz) mass.kind = 1;
    else {
        FEDD_CHECK(M.block_mode == FEDD_BLOCK_DIAG && M.nnz * M.dofs == c->nnz,
                   "%s: unsupported pattern pairing (block mode %d into the FULL system matrix): same pattern, or DIAG into FULL", who,
                   M.block_mode);
        mass.kind = 2;
    }
    mass.rowptr = M.rowptr.p;
    mass.val = M.val.p;
    mass.cm = cm;
    mass.nnz = M.nnz;
    return assemble_hyper(c, model, params, n_params, what, mass, who);
}

}  // namespace fedd
