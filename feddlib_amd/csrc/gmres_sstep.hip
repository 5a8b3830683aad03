// Right-preconditioned restarted s-step GMRES on the device (gmres_kind 2, the default): the block Gram-Schmidt kernels, the
// solver and fedd_gmres_capture_*.  The one-vector solvers, the solve frame's member functions and the dispatcher are in
// gmres.hip; gmres_frame.hpp is what the two files share, gmres_stop_rule.hpp the host-only stopping rule.
#include "gmres_frame.hpp"
#include "gmres_stop_rule.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace fedd {

// ------------------------------------------------------------------------------------------------
// s-step GMRES (gmres_kind 2).  The Krylov basis is extended s vectors at a time: w_i = B w_{i-1},
// w_0 = q_{k-1} (monomial block basis), and the block W = [w_1 .. w_s] is orthogonalised against the k
// final basis vectors and within itself by block classical Gram-Schmidt with the Pythagorean inner
// product, twice (BCGS-PIP2; Carson, Lund, Rozloznik, Thomas, "Block Gram-Schmidt algorithms and their
// stability properties", 2022):
//   pass:  [C; G] = [Q_k W]^T W  (ONE sweep over the basis, one reduction);  R^T R = G - C^T C (Cholesky of an
//          s x s matrix);  W <- (W - Q_k C) R^-1  (one sweep).
// Two passes = four sweeps over the basis per s iterations instead of two per iteration, and two all-reduces per
// block instead of one per iteration.  With W = Q_k C + Q_new R (C = C1 + C2 R1, R = R2 R1) the Hessenberg
// columns follow from B q_{k-1} = w_1 and B w_i = w_{i+1}:
//   column k-1        = [C(:,0); R(0,0)]
//   columns k..k+s-2  = ([C(:,1:s); R(:,1:s)] - [Hbar_k C(:,0:s-1); 0]) R(0:s-1,0:s-1)^-1
// (Hoemmen, "Communication-avoiding Krylov subspace methods", 2010, section 3.3).  In exact arithmetic the
// iterates are those of standard GMRES.  A block whose Cholesky factorisation meets a pivot below the
// threshold is cut there (the columns before it are valid) and the following blocks are shorter; the
// convergence claim of the recurrence is checked against the true residual before it is accepted.

// basis columns per group of the block dot kernel: groups x block columns = the wave totals one transpose reduction yields
constexpr int ss_cg(int S) { return S >= 16 ? 2 : 4; }

// exchange step of the transpose reduction between lanes l and l ^ OFF for one pair of values: afterwards `lo` holds, in
// the lanes with bit OFF clear, lo(l) + lo(l ^ OFF) and, in the lanes with it set, hi(l) + hi(l ^ OFF).
// OFF = 32 / 16: gfx950's v_permlane32_swap / v_permlane16_swap move the halves (rows 2-3 of the first operand <-> rows
// 0-1 of the second; odd rows of the first <-> even rows of the second) without going through the LDS crossbar.
template <int OFF>
__device__ __forceinline__ double xchg_add(double lo, double hi, int lane) {
    if constexpr (OFF == 32 || OFF == 16) {
        const unsigned l0 = __double2loint(lo), l1 = __double2hiint(lo), h0 = __double2loint(hi), h1 = __double2hiint(hi);
        if constexpr (OFF == 32) {
            const auto r0 = __builtin_amdgcn_permlane32_swap(l0, h0, false, false);
            const auto r1 = __builtin_amdgcn_permlane32_swap(l1, h1, false, false);
            return __hiloint2double(r1[0], r0[0]) + __hiloint2double(r1[1], r0[1]);
        } else {
            const auto r0 = __builtin_amdgcn_permlane16_swap(l0, h0, false, false);
            const auto r1 = __builtin_amdgcn_permlane16_swap(l1, h1, false, false);
            return __hiloint2double(r1[0], r0[0]) + __hiloint2double(r1[1], r0[1]);
        }
    } else {
        const bool up = (lane & OFF) != 0;
        const double keep = up ? hi : lo;
        const double send = up ? lo : hi;
        return keep + __shfl_xor(send, OFF, 64);
    }
}

// all-lanes transpose reduction of NV values: afterwards lane l holds the wave total of value l >> (6 - log2 NV)
// (values first, then selects on values: a select between two array ELEMENTS becomes an indexed access and sends the whole
// array to scratch memory)
template <int NV, int OFF, int W>
__device__ __forceinline__ void wave_reduce_step(double (&a)[NV], int lane) {
    if constexpr (W > 1) {
#pragma unroll
        for (int i = 0; i < W / 2; ++i) a[i] = xchg_add<OFF>(a[i], a[i + W / 2], lane);
    } else {
        a[0] += __shfl_xor(a[0], OFF, 64);
    }
    if constexpr (OFF > 1) wave_reduce_step<NV, OFF / 2, (W > 1 ? W / 2 : 1)>(a, lane);
}
template <int NV>
__device__ __forceinline__ double wave_reduce_transpose(double (&a)[NV], int lane) {
    wave_reduce_step<NV, 32, NV>(a, lane);
    return a[0];
}

// branch-free 16-byte load of rows (r, r + 1) of a basis column (columns are padded to ldv >= n + (n & 1), so the pair
// at a clamped row is always readable; rows past n read as zero through selects, never through arithmetic on padding)
struct RowPair {
    int64_t rc;   // clamped row
    bool v0, v1;
};
__device__ __forceinline__ RowPair row_pair(int64_t r, int64_t n) {
    RowPair q;
    q.v0 = r < n;
    q.v1 = r + 1 < n;
    q.rc = q.v0 ? r : 0;
    return q;
}
template <bool NT>
__device__ __forceinline__ double2 ldraw(const double* __restrict__ p, const RowPair& q) {
    typedef double v2d __attribute__((ext_vector_type(2)));
    const v2d t = NT ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p + q.rc)) : *reinterpret_cast<const v2d*>(p + q.rc);
    return double2{t.x, t.y};
}
template <bool NT>
__device__ __forceinline__ double2 ldp(const double* __restrict__ p, const RowPair& q) {
    typedef double v2d __attribute__((ext_vector_type(2)));
    const v2d t = NT ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p + q.rc)) : *reinterpret_cast<const v2d*>(p + q.rc);
    double2 v;
    v.x = q.v0 ? t.x : 0.0;
    v.y = q.v1 ? t.y : 0.0;
    return v;
}

constexpr int SS_LDS_GROUPS = 32;   // column groups whose wave totals are parked in LDS between two workgroup barriers

// the products of one group of the block's own columns, W_i . W_j for i = g * SS_CG + cc and j >= i, from the W tile in
// registers (G = W^T W is symmetric: the flush stores each total to (i, j) and (j, i)).  The per-lane expression is the one
// the streamed columns go through, with a register copy of W_i in the place of the loaded column: same bits.
// Called from fully unrolled loops only -- g, and with it every index into w, is a compile-time constant there.
template <int S, int NCH, int SS_CG>
__device__ __forceinline__ void own_products(const double2 (&w)[S][NCH], int g, double (&acc)[SS_CG * S]) {
#pragma unroll
    for (int cc = 0; cc < SS_CG; ++cc)
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const int i = g * SS_CG + cc;
            double s = 0.0;
            if (j >= i) {
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) s += w[i][ch].x * w[j][ch].x + w[i][ch].y * w[j][ch].y;
            }
            acc[cc * S + j] = s;
        }
}

// partial[(col * S + j) * nblk + blk] = sum over the workgroup's rows of V_col . W_j, col < k + sa
// (W_j = V_{k+j}); the W tile stays in registers across the column groups, every basis column is read once.
// The wave totals of a column group are parked in LDS and added (fixed order) once per SS_LDS_GROUPS groups:
// no barrier between the loads of consecutive groups.
// OWN (option "gmres_dot_own"): only the k final basis columns are streamed; the rows k .. k + sa - 1 of the result, W^T W,
// come from the W tile the lanes already hold (own_products) -- 8 n sa bytes less per sweep, the same bits.  The groups
// are then numbered: first those of the block's own columns, then those of the basis (a group never holds both kinds);
// the workgroups of a row block share them round robin as before.  The first basis group is loaded before the own
// groups are worked on, so its latency passes behind them.  !OWN streams all k + sa columns (the A/B reference).
template <int S, int NCH, int SS_CG, bool OWN>
__global__ __launch_bounds__(256) void k_blockdot(const double* __restrict__ V, int64_t ldv, int64_t n, int k, int sa_req,
                                                  const int32_t* __restrict__ d_sa, double* __restrict__ partial, int nblk) {
    constexpr int NV = SS_CG * S;
    static_assert(NV == 16 || NV == 32 || NV == 64, "block size");
    __shared__ double sh[SS_LDS_GROUPS][4][NV];
    const int sa = d_sa ? min(*d_sa, sa_req) : sa_req;
    if (sa <= 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (th == tid and half == 0 under the launch bounds.  They stay spelled this way: the compiler folds them late, and with
    // plain tid / 0 it schedules the loads of the three instantiations differently from the code that was measured)
    const int half = tid / 256, th = tid % 256;
    RowPair rp[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
        rp[ch] = row_pair((int64_t)blockIdx.x * (512 * NCH) + 512 * ch + 2 * th, n);
    double2 w[S][NCH];
#pragma unroll
    for (int j = 0; j < S; ++j)
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            // (columns past sa: any readable column, zeroed by the select)
            const int jj = half * S + j;
            const double2 t = ldp<false>(V + (int64_t)(k + (jj < sa ? jj : 0)) * ldv, rp[ch]);
            w[j][ch].x = jj < sa ? t.x : 0.0;
            w[j][ch].y = jj < sa ? t.y : 0.0;
        }
    constexpr int NWG = S / SS_CG;                          // OWN: groups the block's own columns fill at most ...
    static_assert(NWG <= SS_LDS_GROUPS, "own groups are parked without a flush");
    const int nwg = OWN ? (sa + SS_CG - 1) / SS_CG : 0;     // ... and those with a column below sa: group numbers 0 .. nwg - 1
    const int ncol = OWN ? k : k + sa;                      // streamed columns: group numbers nwg .. ncg - 1
    const int ncg = nwg + (ncol + SS_CG - 1) / SS_CG;
    int parked = 0, first_cg = blockIdx.y;
    constexpr int GRP = 64 / NV;
    auto flush = [&](int count) {
        __syncthreads();
        for (int e = tid; e < count * NV; e += 256) {
            const int g = e / NV, idx = e % NV;
            const int grp = first_cg + g * (int)gridDim.y;
            const double tot = ((sh[g][0][idx] + sh[g][1][idx]) + sh[g][2][idx]) + sh[g][3][idx];
            if (OWN && grp < nwg) {
                // W_i . W_j, formed for j >= i: row k + i takes it at j and, if W_j is part of the block, row k + j at i
                // (columns j >= sa of a row stay zero: w[j] is)
                const int i = grp * SS_CG + idx / S, j = idx % S;
                if (i < sa && j >= i) {
                    partial[((int64_t)(k + i) * S + j) * nblk + blockIdx.x] = tot;
                    if (j > i && j < sa) partial[((int64_t)(k + j) * S + i) * nblk + blockIdx.x] = tot;
                }
            } else {
                const int col = (grp - nwg) * SS_CG + idx / S;
                if (col < ncol) partial[((int64_t)col * S + (idx % S)) * nblk + blockIdx.x] = tot;
            }
        }
        __syncthreads();
    };
    double2 v[SS_CG][NCH];
    auto load_group = [&](int cg) {   // cg: number of a group of streamed columns
#pragma unroll
        for (int cc = 0; cc < SS_CG; ++cc) {
            const int col = (cg - nwg) * SS_CG + cc;
            const double* __restrict__ a = V + (int64_t)(col < ncol ? col : 0) * ldv;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                // final basis columns are streamed (non-temporal); the block's own columns (!OWN) are re-read soon.
                // Raw loads, no selects behind them (a select would make the wave wait for the load right here instead of
                // at the products after the reduction of the previous group): rows past n meet w = 0 there (the padding
                // rows of the basis are zeroed when it is allocated), columns past ncol are dropped when the sums are stored
                v[cc][ch] = OWN || col < k ? ldraw<true>(a, rp[ch]) : ldraw<false>(a, rp[ch]);
            }
        }
    };
    int cg = blockIdx.y;
    if constexpr (OWN) {
        // this workgroup's first group of streamed columns, in flight while its own groups are formed
        const int gy = gridDim.y;
        const int cq = cg >= nwg ? cg : cg + (nwg - cg + gy - 1) / gy * gy;
        if (cq < ncg) load_group(cq);
#pragma unroll
        for (int g = 0; g < NWG; ++g)
            if (g == cg && g < nwg) {
                double acc[NV];
                own_products<S, NCH, SS_CG>(w, g, acc);
                const double tot = wave_reduce_transpose<NV>(acc, lane);
                if ((lane & (GRP - 1)) == 0) sh[parked][wave][lane / GRP] = tot;
                ++parked;
                cg += gy;
            }
    } else {
        if (cg < ncg) load_group(cg);
    }
    for (; cg < ncg; cg += gridDim.y) {
        double acc[NV];
#pragma unroll
        for (int cc = 0; cc < SS_CG; ++cc)
#pragma unroll
            for (int j = 0; j < S; ++j) {
                double s = 0.0;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) s += v[cc][ch].x * w[j][ch].x + v[cc][ch].y * w[j][ch].y;
                acc[cc * S + j] = s;
            }
        // the next group's loads are in flight while this one is reduced
        if (cg + (int)gridDim.y < ncg) load_group(cg + gridDim.y);
        const double tot = wave_reduce_transpose<NV>(acc, lane);
        if ((lane & (GRP - 1)) == 0) sh[parked][wave][lane / GRP] = tot;
        if (++parked == SS_LDS_GROUPS) {
            flush(parked);
            parked = 0;
            first_cg = cg + gridDim.y;
        }
    }
    if (parked) flush(parked);
}

// W <- (W - V_k C) Rinv : cf = C [k][S] row-wise, rinv [S][S] row-wise upper triangular; columns >= sa untouched
// COMB (the block that fills a restart cycle, second update): the sweep also forms  comb = sum_{c < k + sa - 1} y_c V_c  with
// the finished columns of the block -- the combination k_combine would read the whole basis for right afterwards (y from
// k_backsolve over all k - 1 + sa Hessenberg columns; only valid if the block is not cut, which the host knows later)
template <int S, bool COMB = false>
__global__ __launch_bounds__(256) void k_blockaxpy(double* __restrict__ V, int64_t ldv, int64_t n, int k, int sa_req,
                                                   const int32_t* __restrict__ d_sa, const double* __restrict__ cf,
                                                   const double* __restrict__ rinv, const double* __restrict__ yv = nullptr,
                                                   double* __restrict__ comb = nullptr) {
    const int sa = min(*d_sa, sa_req);
    if (sa <= 0) return;
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * AX_ROWS + 2 * tid;
    const RowPair rp = row_pair(r, n);
    double2 cb = double2{0.0, 0.0};
    double2 acc[S];
#pragma unroll
    for (int j = 0; j < S; ++j) acc[j] = double2{0.0, 0.0};
    int c = 0;
    for (; c + 8 <= k; c += 8) {
        double2 q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = ldp<true>(V + (int64_t)(c + u) * ldv, rp);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const double cc = cf[(c + u) * S + j];   // wave-uniform: scalar loads
                acc[j].x += cc * q[u].x;
                acc[j].y += cc * q[u].y;
            }
            if constexpr (COMB) {
                const double yc = yv[c + u];
                cb.x += yc * q[u].x;
                cb.y += yc * q[u].y;
            }
        }
    }
    for (; c < k; ++c) {
        const double2 q = ldp<true>(V + (int64_t)c * ldv, rp);
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const double cc = cf[c * S + j];
            acc[j].x += cc * q.x;
            acc[j].y += cc * q.y;
        }
        if constexpr (COMB) {
            const double yc = yv[c];
            cb.x += yc * q.x;
            cb.y += yc * q.y;
        }
    }
    double2 t[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const double2 wv = ldp<false>(V + (int64_t)(k + (j < sa ? j : 0)) * ldv, rp);
        t[j].x = j < sa ? wv.x - acc[j].x : 0.0;
        t[j].y = j < sa ? wv.y - acc[j].y : 0.0;
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
        if (j < sa) {
            double2 o = double2{0.0, 0.0};
#pragma unroll
            for (int i = 0; i <= j; ++i) {
                const double ri = rinv[i * S + j];
                o.x += ri * t[i].x;
                o.y += ri * t[i].y;
            }
            double* wj = V + (int64_t)(k + j) * ldv;
            if (rp.v1) *reinterpret_cast<double2*>(wj + r) = o;
            else if (rp.v0) wj[r] = o.x;
            if constexpr (COMB) {
                if (j < sa - 1) {       // (the last basis vector takes no part in the solution update)
                    const double yc = yv[k + j];
                    cb.x += yc * o.x;
                    cb.y += yc * o.y;
                }
            }
        }
    }
    if constexpr (COMB) {
        if (rp.v1) *reinterpret_cast<double2*>(comb + r) = cb;
        else if (rp.v0) comb[r] = cb.x;
    }
}

// First update and second dot of the block Gram-Schmidt in ONE sweep (option "gmres_fuse"): a lane takes a row pair, forms
//   W' = (W - V_k C1) R1^-1   (k_blockaxpy: all k basis columns read once, W' stored)
// and then, with W' still in registers, the second pass' products  [V_k W']^T W'  (k_blockdot) over the same rows: the
// basis columns are read a second time -- from the Infinity Cache, where the first read of the workgroup's rows left them
// (tools/microbench/reread.hip: two passes over the same rows of 64 columns 1.43 ms against 2 x 0.84 for two sweeps).
// partial[(col * S + j) * nblk + blk] as k_blockdot writes it, nblk = gridDim.x (512 rows per workgroup).
// OWN (option "gmres_dot_own"): as in k_blockdot, the second walk streams the k basis columns only and W'^T W' comes from the
// W' the lane has just stored (its groups numbered first); !OWN reads those columns back (the A/B reference).
template <int S, bool OWN>
__global__ __launch_bounds__(256) void k_blockfuse(double* __restrict__ V, int64_t ldv, int64_t n, int k, int sa_req,
                                                   const int32_t* __restrict__ d_sa, const double* __restrict__ cf,
                                                   const double* __restrict__ rinv, double* __restrict__ partial, int nblk) {
    constexpr int SS_CG = 2, NV = SS_CG * S;
    static_assert(NV == 32, "block size");
    __shared__ double sh[SS_LDS_GROUPS][4][NV];
    const int sa = min(*d_sa, sa_req);
    if (sa <= 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = (int64_t)blockIdx.x * AX_ROWS + 2 * tid;
    const RowPair rp = row_pair(r, n);
    double2 w[S];
    {
        double2 acc[S];
#pragma unroll
        for (int j = 0; j < S; ++j) acc[j] = double2{0.0, 0.0};
        int c = 0;
        for (; c + 8 <= k; c += 8) {
            double2 q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = ldp<false>(V + (int64_t)(c + u) * ldv, rp);
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    const double cc = cf[(c + u) * S + j];   // wave-uniform: scalar loads
                    acc[j].x += cc * q[u].x;
                    acc[j].y += cc * q[u].y;
                }
        }
        for (; c < k; ++c) {
            const double2 q = ldp<false>(V + (int64_t)c * ldv, rp);
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const double cc = cf[c * S + j];
                acc[j].x += cc * q.x;
                acc[j].y += cc * q.y;
            }
        }
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const double2 wv = ldp<false>(V + (int64_t)(k + (j < sa ? j : 0)) * ldv, rp);
            acc[j].x = j < sa ? wv.x - acc[j].x : 0.0;
            acc[j].y = j < sa ? wv.y - acc[j].y : 0.0;
        }
#pragma unroll
        for (int j = 0; j < S; ++j) {
            double2 o = double2{0.0, 0.0};
            if (j < sa) {
#pragma unroll
                for (int i = 0; i <= j; ++i) {
                    const double ri = rinv[i * S + j];
                    o.x += ri * acc[i].x;
                    o.y += ri * acc[i].y;
                }
                double* wj = V + (int64_t)(k + j) * ldv;
                if (rp.v1) *reinterpret_cast<double2*>(wj + r) = o;
                else if (rp.v0) wj[r] = o.x;
            }
            // (rows past n: every value above came through ldp's zeros, so o is 0 there)
            w[j] = o;
        }
    }
    // ---- second pass' dot products over the same rows ----
    constexpr int NWG = S / SS_CG;
    static_assert(NWG <= SS_LDS_GROUPS, "own groups are parked without a flush");
    const int nwg = OWN ? (sa + SS_CG - 1) / SS_CG : 0;     // groups 0 .. nwg - 1: the block's own columns (OWN)
    const int ncol = OWN ? k : k + sa;                      // groups nwg .. ncg - 1: the streamed columns
    const int ncg = nwg + (ncol + SS_CG - 1) / SS_CG;
    int parked = 0, first_cg = 0;
    constexpr int GRP = 64 / NV;
    auto flush = [&](int count) {
        __syncthreads();
        for (int e = tid; e < count * NV; e += 256) {
            const int g = e / NV, idx = e % NV;
            const int grp = first_cg + g;
            const double tot = ((sh[g][0][idx] + sh[g][1][idx]) + sh[g][2][idx]) + sh[g][3][idx];
            if (OWN && grp < nwg) {   // (k_blockdot: formed for j >= i, stored to both halves)
                const int i = grp * SS_CG + idx / S, j = idx % S;
                if (i < sa && j >= i) {
                    partial[((int64_t)(k + i) * S + j) * nblk + blockIdx.x] = tot;
                    if (j > i && j < sa) partial[((int64_t)(k + j) * S + i) * nblk + blockIdx.x] = tot;
                }
            } else {
                const int col = (grp - nwg) * SS_CG + idx / S;
                if (col < ncol) partial[((int64_t)col * S + (idx % S)) * nblk + blockIdx.x] = tot;
            }
        }
        __syncthreads();
    };
    double2 v[SS_CG];
    auto load_group = [&](int cg) {   // cg: number of a group of streamed columns
#pragma unroll
        for (int cc = 0; cc < SS_CG; ++cc) {
            const int col = (cg - nwg) * SS_CG + cc;
            const double* __restrict__ a = V + (int64_t)(col < ncol ? col : 0) * ldv;
            // basis columns: second and last read of this sweep (non-temporal); the block's own columns (!OWN) were stored above by this lane
            v[cc] = OWN || col < k ? ldraw<true>(a, rp) : ldp<false>(a, rp);
        }
    };
    int cg = 0;
    if (nwg < ncg) load_group(nwg);   // (OWN: in flight while the own groups are formed)
    if constexpr (OWN) {
#pragma unroll
        for (int g = 0; g < NWG; ++g)
            if (g < nwg) {
                double acc[NV];
                // (the expression of the loop below with w[i] in the place of the loaded column; g, i, j: compile-time constants)
#pragma unroll
                for (int cc = 0; cc < SS_CG; ++cc)
#pragma unroll
                    for (int j = 0; j < S; ++j) {
                        const int i = g * SS_CG + cc;
                        acc[cc * S + j] = j >= i ? w[i].x * w[j].x + w[i].y * w[j].y : 0.0;
                    }
                const double tot = wave_reduce_transpose<NV>(acc, lane);
                if ((lane & (GRP - 1)) == 0) sh[parked][wave][lane / GRP] = tot;
                ++parked;
                ++cg;
            }
    }
    for (; cg < ncg; ++cg) {
        double acc[NV];
#pragma unroll
        for (int cc = 0; cc < SS_CG; ++cc)
#pragma unroll
            for (int j = 0; j < S; ++j) acc[cc * S + j] = v[cc].x * w[j].x + v[cc].y * w[j].y;
        if (cg + 1 < ncg) load_group(cg + 1);
        const double tot = wave_reduce_transpose<NV>(acc, lane);
        if ((lane & (GRP - 1)) == 0) sh[parked][wave][lane / GRP] = tot;
        if (++parked == SS_LDS_GROUPS) {
            flush(parked);
            parked = 0;
            first_cg = cg + 1;
        }
    }
    if (parked) flush(parked);
}

struct Off3 {
    int Hraw, P, C1, R1, R1i, Cc, cf1, ri1, cf2, ri2, th, res;
};

// Upper Cholesky factor of the sa x sa leading block of the symmetric A (upper part read) via the unit-diagonal scaling, cut
// at the first column whose pivot (relative to gdiag: the squared sine of the angle between the column and the span of
// everything before it) is <= tol.  Returns the accepted columns; R and its inverse Ri are zero outside the accepted upper
// triangle.  Called by the whole workgroup (>= S * S lanes), A / W / R / Ri / dd in LDS; right-looking, one barrier-separated
// step per column.
template <int S>
__device__ int chol_cut(double (&A)[S][S], const double* gdiag, int sa, double tol, double (&W)[S][S], double (&R)[S][S],
                        double (&Ri)[S][S], double* dd, int* s_ok, int tid) {
    const int i = tid / S, j = tid % S;
    if (tid < S) dd[tid] = (tid < sa && A[tid][tid] > 0.0) ? sqrt(A[tid][tid]) : 0.0;
    if (tid == 0) *s_ok = sa;
    __syncthreads();
    if (tid < S * S) {
        W[i][j] = (i <= j && dd[i] > 0.0 && dd[j] > 0.0) ? A[i][j] / (dd[i] * dd[j]) : 0.0;
        R[i][j] = 0.0;
        Ri[i][j] = 0.0;
    }
    __syncthreads();
    for (int c = 0; c < sa; ++c) {
        if (tid == 0) {
            const double piv = W[c][c];
            if (!(dd[c] > 0.0) || !(piv > 0.0) || !(piv * A[c][c] > tol * gdiag[c])) *s_ok = c;
        }
        __syncthreads();
        if (*s_ok <= c) break;   // (uniform: read after the barrier)
        const double rp = 1.0 / sqrt(W[c][c]);
        __syncthreads();
        if (tid < S && tid >= c) R[c][tid] = W[c][tid] * rp;   // row c of U (R[c][c] = sqrt(piv))
        __syncthreads();
        if (tid < S * S && i > c && i <= j) W[i][j] -= R[c][i] * R[c][j];
        __syncthreads();
    }
    const int ok = *s_ok;
    if (tid < S * S) R[i][j] = (i <= j && j < ok) ? R[i][j] * dd[j] : 0.0;
    __syncthreads();
    if (tid < ok) {   // column tid of the inverse by back substitution
        const int cj = tid;
        Ri[cj][cj] = 1.0 / R[cj][cj];
        for (int r = cj - 1; r >= 0; --r) {
            double acc = 0.0;
            for (int p = r + 1; p <= cj; ++p) acc += R[r][p] * Ri[p][cj];
            Ri[r][cj] = -acc / R[r][r];
        }
    }
    __syncthreads();
    return ok;
}

// S1 = G - C^T C from the reduced dot products P [(k + sa)][S]
template <int S>
__device__ void gram_minus(const double* __restrict__ P, int k, double (&G)[S][S], double (&A)[S][S], int tid) {
    if (tid < S * S) {
        const int i = tid / S, j = tid % S;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int c = 0;
        for (; c + 4 <= k; c += 4) {
            s0 += P[(c + 0) * S + i] * P[(c + 0) * S + j];
            s1 += P[(c + 1) * S + i] * P[(c + 1) * S + j];
            s2 += P[(c + 2) * S + i] * P[(c + 2) * S + j];
            s3 += P[(c + 3) * S + i] * P[(c + 3) * S + j];
        }
        for (; c < k; ++c) s0 += P[c * S + i] * P[c * S + j];
        const double g = P[(k + i) * S + j];
        G[i][j] = g;
        A[i][j] = g - ((s0 + s1) + (s2 + s3));
    }
}

// pass 1 of a block: Cholesky of G - C1^T C1 (cut where the block basis becomes dependent), coefficients of sweep 2
template <int S>
__global__ __launch_bounds__(256) void k_ss_pass1(double* __restrict__ Sx, Off3 o3, int k, int sa_req, double tol,
                                                  int32_t* __restrict__ d_sa) {
    __shared__ double G[S][S], A[S][S], W[S][S], R[S][S], Ri[S][S];
    __shared__ double gd[S], dd[S];
    __shared__ int s_ok;
    const int tid = threadIdx.x;
    const double* P = Sx + o3.P;
    gram_minus<S>(P, k, G, A, tid);
    __syncthreads();
    if (tid < S) gd[tid] = G[tid][tid];
    __syncthreads();
    const int ok1 = chol_cut<S>(A, gd, sa_req, tol, W, R, Ri, dd, &s_ok, tid);
    if (tid == 0) d_sa[0] = ok1;
    __syncthreads();
    for (int i = tid; i < k * S; i += 256) {
        const double v = P[i];
        Sx[o3.C1 + i] = v;
        Sx[o3.cf1 + i] = v;
    }
    if (tid < S * S) {
        Sx[o3.R1 + tid] = R[tid / S][tid % S];
        Sx[o3.R1i + tid] = Ri[tid / S][tid % S];
        Sx[o3.ri1 + tid] = Ri[tid / S][tid % S];
    }
}

// pass 2 of a block: second Cholesky, combined coefficients, the new Hessenberg columns (formulas above), their
// Givens rotations and the residual after each of them.
// host_out: [0] = accepted columns (0: breakdown, the column k-1 is still final), [1] = 1 if breakdown, [2 + i] =
// residual after column k-1+i
template <int S>
__global__ __launch_bounds__(256) void k_ss_pass2(double* __restrict__ Sx, Off o, Off3 o3, int k, int sa_req, int m, double tol,
                                                  int32_t* __restrict__ d_sa, double* __restrict__ host_out) {
    extern __shared__ double dyn[];   // hc[S][m+2] | lcs[m] | lsn[m]
    __shared__ double G[S][S], A[S][S], W[S][S], R2[S][S], R2i[S][S], R1[S][S], R1i[S][S], Rc[S][S], Rci[S][S];
    __shared__ double gd[S], th[S], dd[S];
    __shared__ int s_sa;
    double* hc = dyn;
    double* lcs = hc + (size_t)S * (m + 2);
    double* lsn = lcs + m;
    const int tid = threadIdx.x, ldh = m + 1;
    const double* P = Sx + o3.P;
    double* Hraw = Sx + o3.Hraw;
    const int sa1 = min(d_sa[0], sa_req);
    if (tid < S * S) {
        R1[tid / S][tid % S] = Sx[o3.R1 + tid];
        R1i[tid / S][tid % S] = Sx[o3.R1i + tid];
    }
    if (tid < S) th[tid] = Sx[o3.th + tid];
    for (int i = tid; i < k - 1; i += 256) {
        lcs[i] = Sx[o.cs + i];
        lsn[i] = Sx[o.sn + i];
    }
    int sa = 0;
    if (sa1 > 0) {
        gram_minus<S>(P, k, G, A, tid);
        __syncthreads();
        if (tid < S) gd[tid] = G[tid][tid];
        __syncthreads();
        sa = chol_cut<S>(A, gd, sa1, tol, W, R2, R2i, dd, &s_sa, tid);
    }
    __syncthreads();
    const bool brk = sa == 0;
    if (!brk) {
        if (tid < S * S) {
            const int i = tid / S, j = tid % S;
            double s = 0.0, t = 0.0;
            for (int p = 0; p < S; ++p) {
                s += R2[i][p] * R1[p][j];
                t += R1i[i][p] * R2i[p][j];
            }
            Rc[i][j] = (i < sa && j < sa) ? s : 0.0;
            Rci[i][j] = (i < sa && j < sa) ? t : 0.0;
        }
        // combined C = C1 + C2 R1 ; sweep-4 coefficients C2
        for (int idx = tid; idx < k * S; idx += 256) {
            const int cc = idx / S, j = idx % S;
            double s = Sx[o3.C1 + idx];
            for (int i = 0; i <= j; ++i) s += P[cc * S + i] * R1[i][j];
            Sx[o3.Cc + idx] = s;
            Sx[o3.cf2 + idx] = P[idx];
        }
        if (tid < S * S) Sx[o3.ri2 + tid] = R2i[tid / S][tid % S];
    } else {
        // breakdown: w_1 lies in the span of the basis (to the threshold): column k-1 = [C1(:,0); 0]
        for (int idx = tid; idx < k * S; idx += 256) Sx[o3.Cc + idx] = Sx[o3.C1 + idx];
        if (tid < S * S) Rc[tid / S][tid % S] = 0.0;
    }
    __syncthreads();
    // column k-1
    for (int cidx = tid; cidx <= k; cidx += 256) {
        const double v = cidx < k ? Sx[o3.Cc + cidx * S] + (cidx == k - 1 ? th[0] : 0.0) : Rc[0][0];
        Hraw[(int64_t)(k - 1) * ldh + cidx] = v;
    }
    __syncthreads();
    // columns k .. k+sa-2
    const int nc = brk ? 0 : sa - 1;
    if (nc > 0) {
        for (int r = tid; r < k + sa; r += 256) {
            double x[S];
#pragma unroll
            for (int cidx = 0; cidx < S; ++cidx) x[cidx] = 0.0;
            // y = (Hbar_k C)(r, :): the same q for every lane, so that the coefficients C(q, :) are wave-uniform (scalar loads)
            // and only Hbar(r, q) is a per-lane load (coalesced over r); entries below the sub-diagonal are zero by structure
            // (with a per-lane loop start every lane fetched its own 15 coefficients per step: 89 us per block at k ~ 60)
            // (eight entries of the Hessenberg row requested before any is used: one global round trip per eight columns instead
            // of one per column -- the kernel is a single workgroup, nothing else hides that latency)
            for (int q0 = 0; q0 < k; q0 += 8) {
                double h[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = q0 + u;
                    h[u] = (q < k && r <= k && q + 1 >= r) ? Hraw[(int64_t)q * ldh + r] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = q0 + u;
                    if (q < k) {
#pragma unroll
                        for (int cidx = 0; cidx < S - 1; ++cidx) x[cidx] -= h[u] * Sx[o3.Cc + q * S + cidx];
                    }
                }
            }
#pragma unroll
            for (int cidx = 0; cidx < S - 1; ++cidx) {
                if (cidx < nc) {
                    if (r < k) x[cidx] += Sx[o3.Cc + r * S + cidx + 1] + th[cidx + 1] * Sx[o3.Cc + r * S + cidx];
                    else x[cidx] += Rc[r - k][cidx + 1] + th[cidx + 1] * Rc[r - k][cidx];
                }
            }
#pragma unroll
            for (int cidx = 0; cidx < S - 1; ++cidx) {
                if (cidx < nc && r <= k + cidx + 1) {
                    double hv = 0.0;
#pragma unroll
                    for (int cp = 0; cp < S - 1; ++cp)
                        if (cp <= cidx) hv += x[cp] * Rci[cp][cidx];
                    Hraw[(int64_t)(k + cidx) * ldh + r] = hv;
                }
            }
        }
    }
    __syncthreads();
    // Givens.  The rotations of the earlier columns (q < k - 1) are applied to all new columns at once, a lane per column (each
    // chain is sequential in q, the columns are independent); then lane 0 runs the triangular rest -- the rotations the block
    // itself creates -- column by column.  Per column the same operations in the same order as one chain after the other
    // (which took 16 x k dependent LDS steps on one lane: 67 of the kernel's 95 us at k ~ 60).
    const int ncolH = brk ? 1 : sa;
    for (int i = 0; i < ncolH; ++i) {
        const int jj = k - 1 + i;
        double* hci = hc + (size_t)i * (m + 2);
        for (int q = tid; q <= jj + 1; q += 256) hci[q] = Hraw[(int64_t)jj * ldh + q];
    }
    __syncthreads();
    if (tid < ncolH) {
        double* hci = hc + (size_t)tid * (m + 2);
        for (int q = 0; q < k - 1; ++q) {
            const double a = lcs[q] * hci[q] + lsn[q] * hci[q + 1];
            hci[q + 1] = -lsn[q] * hci[q] + lcs[q] * hci[q + 1];
            hci[q] = a;
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 0; i < ncolH; ++i) {
            const int jj = k - 1 + i;
            double* hci = hc + (size_t)i * (m + 2);
            for (int q = k - 1; q < jj; ++q) {
                const double a = lcs[q] * hci[q] + lsn[q] * hci[q + 1];
                hci[q + 1] = -lsn[q] * hci[q] + lcs[q] * hci[q + 1];
                hci[q] = a;
            }
            const double d = hypot(hci[jj], hci[jj + 1]);
            const double cj = d > 0 ? hci[jj] / d : 1.0, sj = d > 0 ? hci[jj + 1] / d : 0.0;
            lcs[jj] = cj;
            lsn[jj] = sj;
            Sx[o.cs + jj] = cj;
            Sx[o.sn + jj] = sj;
            hci[jj] = d;
            hci[jj + 1] = 0.0;
            const double gj = Sx[o.g + jj];
            Sx[o.g + jj + 1] = -sj * gj;
            Sx[o.g + jj] = cj * gj;
            Sx[o3.res + i] = fabs(sj * gj);
        }
    }
    __syncthreads();
    for (int i = 0; i < ncolH; ++i) {
        const int jj = k - 1 + i;
        const double* hci = hc + (size_t)i * (m + 2);
        double* H = Sx + o.H + (int64_t)jj * ldh;
        for (int q = tid; q <= jj + 1; q += 256) H[q] = hci[q];
    }
    __syncthreads();
    if (tid == 0) {
        d_sa[0] = sa;
        Sx[o.misc + 4] = (double)sa;
        Sx[o.misc + 5] = brk ? 1.0 : 0.0;
        if (host_out) {
            host_out[0] = (double)sa;
            host_out[1] = brk ? 1.0 : 0.0;
            for (int i = 0; i < S; ++i) host_out[2 + i] = i < ncolH ? Sx[o3.res + i] : 0.0;
            __threadfence_system();
        }
    }
}

__global__ void k_ss_cycle_init(double* __restrict__ S, Off o, Off3 o3, int m, int s, const double* __restrict__ rr) {
    const double beta = sqrt(rr[0]);
    for (int i = threadIdx.x; i <= m; i += blockDim.x) S[o.g + i] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        S[o.g] = beta;
        S[o.misc + 1] = beta > 0 ? 1.0 / beta : 0.0;
        S[o.misc + 3] = beta;
    }
}

// Real parts of the eigenvalues of a small upper Hessenberg matrix (column-major, leading dimension ld) by the unshifted QR
// iteration with Givens rotations: crude (linear convergence), but the Ritz values only have to place the shifts of the Newton
// block basis over the spectrum; whatever 2 x 2 blocks are left on the diagonal are resolved in closed form.
static void hessenberg_real_parts(std::vector<double> H, int n, int ld, double* out) {
    std::vector<double> cs((size_t)n), sn((size_t)n);
    auto at = [&](int i, int j) -> double& { return H[(size_t)j * ld + i]; };
    for (int sweep = 0; sweep < 500; ++sweep) {
        for (int i = 0; i + 1 < n; ++i) {   // H <- Q^T H
            const double a = at(i, i), b = at(i + 1, i), d = std::hypot(a, b);
            cs[i] = d > 0 ? a / d : 1.0;
            sn[i] = d > 0 ? b / d : 0.0;
            for (int j = i; j < n; ++j) {
                const double u = at(i, j), v = at(i + 1, j);
                at(i, j) = cs[i] * u + sn[i] * v;
                at(i + 1, j) = -sn[i] * u + cs[i] * v;
            }
        }
        for (int i = 0; i + 1 < n; ++i)     // H <- H Q
            for (int r = 0; r <= std::min(i + 1, n - 1); ++r) {
                const double u = at(r, i), v = at(r, i + 1);
                at(r, i) = cs[i] * u + sn[i] * v;
                at(r, i + 1) = -sn[i] * u + cs[i] * v;
            }
    }
    for (int i = 0; i < n;) {
        const double sub = i + 1 < n ? std::fabs(at(i + 1, i)) : 0.0;
        if (i + 1 < n && sub > 1e-10 * (std::fabs(at(i, i)) + std::fabs(at(i + 1, i + 1)))) {
            const double a = at(i, i), b = at(i, i + 1), c2 = at(i + 1, i), d = at(i + 1, i + 1);
            const double tr = 0.5 * (a + d), disc = 0.25 * (a - d) * (a - d) + b * c2;
            const double rt = disc > 0.0 ? std::sqrt(disc) : 0.0;   // complex pair: its real part, twice
            out[i] = tr + rt;
            out[i + 1] = tr - rt;
            i += 2;
        } else {
            out[i] = at(i, i);
            ++i;
        }
    }
}

// Leja ordering: the largest point first, then always the point that maximises the product of its distances to the points taken;
// every prefix of the sequence is then spread over the whole set (a short last block uses a prefix)
static void leja_order(double* v, int n) {
    std::vector<double> in(v, v + n), out;
    std::vector<char> used((size_t)n, 0);
    for (int t = 0; t < n; ++t) {
        int best = -1;
        double bestv = -1e300;
        for (int i = 0; i < n; ++i) {
            if (used[(size_t)i]) continue;
            double score = 0.0;
            if (out.empty()) score = std::fabs(in[(size_t)i]);
            else for (double o : out) score += std::log(std::max(std::fabs(in[(size_t)i] - o), 1e-300));
            if (score > bestv) {
                bestv = score;
                best = i;
            }
        }
        used[(size_t)best] = 1;
        out.push_back(in[(size_t)best]);
    }
    std::copy(out.begin(), out.end(), v);
}

// fedd_gmres_capture_*: the armed block is copied piece by piece, device to device on the solver's stream, between the
// launches the block makes anyway (no launch is added, moved or given other arguments).  Every call is a no-op unless
// begin() found that this is the armed block.
struct BlockCapture {
    typedef GmresCapture G;
    GmresCapture& gc;
    hipStream_t st;
    const int block;   // fedd_gmres_capture_arm: the block to copy, -1 (no block's number) when unarmed
    bool on = false;

    // the sizes of the pieces, and the first of them: the basis before the block (the canary column C0 lies right behind)
    int begin(int number, const Frame& f, int S, int k, int sa) {
        on = number == block;
        if (!on) return 0;
        gc.captured = false;
        gc.n = f.n; gc.ldv = f.ldv; gc.k = k; gc.sa_req = sa; gc.S = S; gc.m = f.m; gc.fused = 0;
        gc.canary = k + sa <= f.m ? 1 : 0;
        const size_t cols = (size_t)(k + sa), L = (size_t)f.ldv;
        for (int p = 0; p < G::NPIECE; ++p) gc.len[p] = 0;
        gc.len[G::V0] = gc.len[G::VEND] = cols * L;
        gc.len[G::C0] = gc.canary * L;
        gc.len[G::P1] = gc.len[G::P2] = cols * S;
        gc.len[G::CF1] = gc.len[G::CF2] = (size_t)k * S;
        gc.len[G::RI1] = gc.len[G::RI2] = (size_t)S * S;
        gc.len[G::SA1] = 1;
        gc.len[G::SA2] = 2;
        gc.len[G::TH] = S;
        gc.len[G::W1] = gc.len[G::W2] = (size_t)(sa + gc.canary) * L;
        gc.len[G::H] = (cols - 1) * (size_t)(f.m + 1);
        size_t tot = 0;
        for (int p = 0; p < G::NPIECE; ++p) {
            gc.off[p] = tot;
            tot += gc.len[p];
        }
        FEDD_TRY(gc.buf.ensure(tot));
        return piece(G::V0, f.V, (cols + gc.canary) * L);
    }
    // `count` values of `elem` bytes into the piece, from its slot `at` on
    int piece(int p, const void* src, size_t count, size_t elem = sizeof(double), size_t at = 0) {
        if (on) FEDD_HIP(hipMemcpyAsync(gc.buf.p + gc.off[p] + at, src, count * elem, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    int piece(int p, const void* src) { return on ? piece(p, src, gc.len[p]) : 0; }   // the whole piece
    void end(bool fused) {
        if (!on) return;
        gc.fused = fused ? 1 : 0;
        gc.captured = true;
    }
};

// One s-step solve.  S: the kernels' block size, >= the blocks actually run.
template <int S>
struct SStep {
    static constexpr int dot_cg = ss_cg(S);   // block dot kernel: 1024 rows per workgroup (two 512-row chunks), ss_cg(S) columns per transpose reduction
    static constexpr bool wide = S == 16;     // the fused sweep and the combining update exist for the 16-column blocks only
    fedd_ctx* c;
    const GmresCall& call;
    Frame f;
    Off3 o3;
    BlockCapture cap;
    hipEvent_t ev = nullptr;      // recorded behind a block's outcome
    double *xt, *axt;             // trial solution (ghost tail behind it), A xt
    int32_t* d_sa;
    double *hout, *hout_dev;      // host mirror of the block result
    int nblkd, gy_dot;
    size_t pass2_lds;
    bool dot_own, fused, newton, dbg;
    int s_goal, max_it;
    bool have_shifts = false;
    std::vector<double> theta;
    // columns whose combination sum_c y_c V_c is already in r: written by the second update of a block that filled its restart
    // cycle (k_blockaxpy<S, true>), -1: none
    int precomb_cols = -1;
    int spec_done = 0, spec_k = -1;   // operator applications of the block starting at spec_k that are already in the stream

    SStep(fedd_ctx* ctx, const GmresCall& cl) : c(ctx), call(cl), cap{ctx->gm_cap, ctx->stream, ctx->gm_cap.armed}, theta((size_t)S, 0.0) {
        c->gm_cap.armed = -1;   // this solve consumes the arm
    }
    ~SStep() {
        if (ev) (void)hipEventDestroy(ev);
    }

    // s: the block length asked for.  Layout of the scalars, buffers, launch shapes and the block-length policy
    int setup(int s) {
        FEDD_TRY(f.setup(c, call, true));
        FEDD_CHECK(f.nr == 1 || (f.nr == MULTI_NR && call.use_prec && multi_rhs_ok(c)), "gmres: stacked solve with %d right-hand sides", f.nr);
        const int m = f.m;
        max_it = call.max_it;
        nblkd = (int)((f.n + 1023) / 1024);
        o3.Hraw = f.p; f.p += (m + 1) * m;
        o3.P = f.p; f.p += (m + 1 + S) * S;
        o3.C1 = f.p; f.p += m * S;
        o3.Cc = f.p; f.p += m * S;
        o3.cf1 = f.p; f.p += m * S;
        o3.cf2 = f.p; f.p += m * S;
        o3.R1 = f.p; f.p += S * S;
        o3.R1i = f.p; f.p += S * S;
        o3.ri1 = f.p; f.p += S * S;
        o3.ri2 = f.p; f.p += S * S;
        o3.th = f.p; f.p += S;
        o3.res = f.p; f.p += S;
        FEDD_TRY(f.alloc(std::max((size_t)(m + 1 + S) * S * (c->gmres_fuse != 0 ? std::max(nblkd, f.nblk2) : nblkd), (size_t)std::max(f.nblk, f.nblk2)), true));
        FEDD_TRY(c->d_flags.ensure(16));
        xt = f.w0;
        axt = f.w1;
        d_sa = c->d_flags.p + 12;   // (0 max scratch, 1 bad pivot, 2 DGKS gate, 3-5 coarse setup, 8-11 Schwarz setup)
        // k_ss_pass2 keeps the S new Hessenberg columns in dynamic LDS (beside 18 KB of static block matrices): long restart cycles
        // go beyond the 64 KB a kernel gets without asking
        pass2_lds = (size_t)(S * (m + 2) + 2 * m) * sizeof(double);
        FEDD_CHECK(pass2_lds <= 128 * 1024, "gmres (s-step): restart length %d with blocks of %d vectors exceeds the LDS of the block kernel", m, S);
        if (pass2_lds > 40 * 1024)
            FEDD_HIP(hipFuncSetAttribute((const void*)k_ss_pass2<S>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pass2_lds));
        // column groups in flight per row block of the dot kernel: one when the vectors are long (every workgroup then
        // reads its rows of W once), more to fill the GPU when they are short
        // (round 4, measured at 145 iterations: 1.26 M rows 1 / 2 / 3 / 4 groups 14.60 / 14.74 / 14.99 / 15.10 ms per solve, 1.03 M rows
        // 15.54 / 15.64 / 15.77 / 15.97, 275 k rows 9.24 / 9.32 / 9.29 / 9.09; the old rule, 2048 workgroups in flight, took 2, 3 and 8)
        gy_dot = c->gmres_dot_gy > 0 ? c->gmres_dot_gy
                                     : (int)std::max<int64_t>(1, std::min<int64_t>(4, (1024 + nblkd / 2) / std::max(nblkd, 1)));
        dot_own = c->gmres_dot_own != 0;   // W^T W from the W tile in registers (k_blockdot, k_blockfuse)
        // first update + second dot in one sweep (auto: long vectors only -- at 9.9 M rows the step gains 1.1 ms, at the 1.26 M rows of
        // the N = 8 share the two separate kernels are 0.15 ms ahead: their second read finds much of the basis in the Infinity Cache anyway)
        fused = wide && (c->gmres_fuse > 0 || (c->gmres_fuse < 0 && f.n >= 4000000));
        hout = c->h_pinned + 16;
        hout_dev = c->h_pinned_dev ? c->h_pinned_dev + 16 : nullptr;
        s_goal = std::max(1, std::min(std::min(s, S), StopRule::s_tol(c->gmres_tol_blocks != 0, call.rtol)));
        // Blocks longer than 8 need a better conditioned block basis than the monomial one (its condition grows tenfold every
        // two vectors, 1e7 at s = 8): the Newton basis w_i = (B - theta_i) w_{i-1} with the Ritz values of the first s_goal
        // Arnoldi steps as shifts, Leja-ordered (Bai, Hu, Reichel, "A Newton basis GMRES implementation", 1994).  Until those
        // steps exist the blocks are monomial and at most 8 long.
        // (the constrained system of the GDSW extension solves (Frame::mk) runs monomial blocks only: the shift would have to
        // reach the held rows too)
        newton = c->gmres_newton && s_goal > 8 && !f.mk && f.nr == 1;
        FEDD_HIP(hipMemsetAsync(f.S + o3.th, 0, (size_t)S * sizeof(double), f.st));   // monomial block basis (shifts 0)
        dbg = getenv("FEDD_GMRES_DEBUG") != nullptr;
        return 0;
    }

    // xt = x + M^-1 V(:, 0:cols) y, r = b - A xt, ||r|| to the host: the true residual with `cols` columns of this cycle
    // (the residual that decides is formed with the parity CSR, see Frame::true_residual)
    int trial(int cols, double* true_abs) {
        if (cols > 0) {
            FEDD_TRY(f.add_correction(cols, xt, cols == precomb_cols));
            precomb_cols = -1;      // (r becomes the residual below)
        } else {
            FEDD_HIP(hipMemcpyAsync(xt, call.x, (size_t)f.n * sizeof(double), hipMemcpyDeviceToDevice, f.st));
        }
        FEDD_TRY(f.true_residual(xt, axt, true, 0, false));
        return f.read_norm(true_abs);
    }
    // what the stopping rule wants done with the trial solution
    int keep(StopRule::Keep what) {
        double ta = 0.0;
        if (what == StopRule::COMMIT)   // x <- xt (r and ||r||^2 already belong to it)
            FEDD_HIP(hipMemcpyAsync(call.x, xt, (size_t)f.n * sizeof(double), hipMemcpyDeviceToDevice, f.st));
        else if (what == StopRule::RECOMPUTE)   // r, ||r||^2 of the current x again
            FEDD_TRY(trial(0, &ta));
        return 0;
    }

    // columns the cycle still has room for behind k final basis vectors (restart length, iteration limit)
    int room(int k, int its) const { return std::min(f.m - (k - 1), max_it - its - (k - 1)); }

    // V(:, k + i) = (B - theta_i) V(:, k - 1 + i) for i0 <= i < i1
    int apply_cols(int k, int i0, int i1) {
        for (int i = i0; i < i1; ++i)
            FEDD_TRY(f.apply(f.V + (int64_t)(k - 1 + i) * f.ldv, f.V + (int64_t)(k + i) * f.ldv, false, have_shifts ? theta[(size_t)i] : 0.0));
        return 0;
    }
    // the block's operator applications, less those speculate() has put into the stream already
    int apply_block(int k, int sa) {
        const int i0 = spec_k == k ? std::min(spec_done, sa) : 0;
        spec_done = 0;
        spec_k = -1;
        return apply_cols(k, i0, sa);
    }
    // The head of the next block goes into the stream before the host waits for this block's outcome: the GPU works
    // through the round trip.  It assumes the ordinary outcome (no cut, no convergence, same shifts); otherwise the
    // two applications wrote columns nobody reads.
    int speculate(int k_next, int its, int s_cur) {
        if (c->gmres_spec <= 0 || (newton && !have_shifts)) return 0;
        const int ns = std::min(std::min(c->gmres_spec, s_cur), room(k_next, its));
        FEDD_TRY(apply_cols(k_next, 0, ns));
        if (ns > 0) {
            spec_done = ns;
            spec_k = k_next;
        }
        return 0;
    }

    // the shifts of the Newton block basis, once per solve: Ritz values of the leading s_goal x s_goal Hessenberg matrix,
    // Leja-ordered, uploaded for k_ss_pass2 and kept for apply_cols (have_shifts stays false if they are not finite)
    int newton_shifts() {
        std::vector<double> Hh((size_t)s_goal * s_goal);
        FEDD_HIP(hipMemcpy2DAsync(Hh.data(), (size_t)s_goal * sizeof(double), f.S + o3.Hraw, (size_t)(f.m + 1) * sizeof(double),
                                  (size_t)s_goal * sizeof(double), (size_t)s_goal, hipMemcpyDeviceToHost, f.st));
        FEDD_HIP(hipStreamSynchronize(f.st));
        hessenberg_real_parts(Hh, s_goal, s_goal, theta.data());
        leja_order(theta.data(), s_goal);
        bool finite = true;
        for (int i = 0; i < s_goal; ++i) finite = finite && std::isfinite(theta[(size_t)i]);
        if (!finite) return 0;
        for (int i = 0; i < S; ++i) c->h_pinned[64 + i] = i < s_goal ? theta[(size_t)i] : 0.0;
        FEDD_HIP(hipMemcpyAsync(f.S + o3.th, c->h_pinned + 64, (size_t)S * sizeof(double), hipMemcpyHostToDevice, f.st));
        have_shifts = true;
        if (dbg) {
            fprintf(stderr, "[gmres s-step] Newton shifts:");
            for (int i = 0; i < s_goal; ++i) fprintf(stderr, " %.4f", theta[(size_t)i]);
            fprintf(stderr, "\n");
        }
        return 0;
    }

    // algorithmic bytes of a dot sweep: the basis and the block read once -- the block's own columns a second time where they
    // are streamed past the W tile (gmres_dot_own 0); of an update: the basis and the block read, the block written
    double dot_bytes(int k, int sa) const { return 8.0 * (double)f.n * (k + (dot_own ? sa : 2 * sa)); }
    double upd_bytes(int k, int sa) const { return 8.0 * (double)f.n * (k + 2 * sa); }

    // [V_k W]^T W into d_part (dsa: the block is as long as pass 1 left it)
    void dot(int k, int sa, const int32_t* dsa) {
        ScopedTimer td(c, FEDD_T_GS_DOT);
        td.bytes(dot_bytes(k, sa));
        const int ncg = (k + sa + dot_cg - 1) / dot_cg;
        const dim3 gd(nblkd, std::min(gy_dot, ncg));
        if (dot_own)
            hipLaunchKernelGGL((k_blockdot<S, 2, dot_cg, true>), gd, f.blk, 0, f.st, (const double*)f.V, f.ldv, f.n, k, sa, dsa, c->d_part.p, nblkd);
        else
            hipLaunchKernelGGL((k_blockdot<S, 2, dot_cg, false>), gd, f.blk, 0, f.st, (const double*)f.V, f.ldv, f.n, k, sa, dsa, c->d_part.p, nblkd);
    }
    // first update + second dot in one sweep (k_blockfuse), a timer class of its own; algorithmic bytes: what the two
    // operations together must move once -- the basis and the block read, the block written: those of the update alone
    void fuse(int k, int sa) {
        if constexpr (wide) {
            ScopedTimer tu(c, FEDD_T_GS_FUSED);
            tu.bytes(upd_bytes(k, sa));
            if (dot_own)
                hipLaunchKernelGGL((k_blockfuse<S, true>), dim3(f.nblk2), f.blk, 0, f.st, f.V, f.ldv, f.n, k, sa, (const int32_t*)d_sa,
                                   (const double*)(f.S + o3.cf1), (const double*)(f.S + o3.ri1), c->d_part.p, f.nblk2);
            else
                hipLaunchKernelGGL((k_blockfuse<S, false>), dim3(f.nblk2), f.blk, 0, f.st, f.V, f.ldv, f.n, k, sa, (const int32_t*)d_sa,
                                   (const double*)(f.S + o3.cf1), (const double*)(f.S + o3.ri1), c->d_part.p, f.nblk2);
        }
    }
    // W <- (W - V_k C) R^-1 with the coefficients at cf / ri.  comb: the sweep also forms sum_c y_c V_c in r (k_blockaxpy)
    void update(int k, int sa, int cf, int ri, bool comb) {
        ScopedTimer tu(c, FEDD_T_GS_UPDATE);
        tu.bytes(upd_bytes(k, sa) + (comb ? 8.0 * (double)f.n : 0.0));
        if (comb) {
            if constexpr (wide)
                hipLaunchKernelGGL((k_blockaxpy<S, true>), dim3(f.nblk2), f.blk, 0, f.st, f.V, f.ldv, f.n, k, sa, (const int32_t*)d_sa,
                                   (const double*)(f.S + cf), (const double*)(f.S + ri), (const double*)(f.S + f.o.y), f.r);
        } else {
            hipLaunchKernelGGL(k_blockaxpy<S>, dim3(f.nblk2), f.blk, 0, f.st, f.V, f.ldv, f.n, k, sa, (const int32_t*)d_sa,
                               (const double*)(f.S + cf), (const double*)(f.S + ri));
        }
    }

    // One block: W = V(:, k : k + sa) against the k final basis vectors and within itself, twice (BCGS-PIP2).  On return the
    // block's outcome is on its way to hout and `ev` is recorded behind it; the second update follows it in the stream.
    int orthogonalise(int k, int sa) {
        typedef GmresCapture G;
        ScopedTimer t(c, FEDD_T_ORTHO);
        double* Sx = f.S;
        double* W = f.V + (int64_t)k * f.ldv;
        const int np = (k + sa) * S;
        FEDD_TRY(cap.begin(c->gmres_blocks, f, S, k, sa));
        dot(k, sa, nullptr);
        f.reduce_cols(np, Sx + o3.P, nblkd);
        FEDD_TRY(allreduce_sum(c, Sx + o3.P, np));
        FEDD_TRY(cap.piece(G::P1, Sx + o3.P));
        hipLaunchKernelGGL(k_ss_pass1<S>, dim3(1), f.blk, 0, f.st, Sx, o3, k, sa, c->gmres_chol_tol, d_sa);
        FEDD_TRY(cap.piece(G::CF1, Sx + o3.cf1));
        FEDD_TRY(cap.piece(G::RI1, Sx + o3.ri1));
        FEDD_TRY(cap.piece(G::SA1, d_sa, 1, sizeof(int32_t)));
        if (fused) {
            ++c->gmres_fused_blocks;
            fuse(k, sa);
            FEDD_TRY(cap.piece(G::W1, W));
        } else {
            update(k, sa, o3.cf1, o3.ri1, false);
            FEDD_TRY(cap.piece(G::W1, W));
            dot(k, sa, d_sa);
        }
        f.reduce_cols(np, Sx + o3.P, fused ? f.nblk2 : nblkd);
        FEDD_TRY(allreduce_sum(c, Sx + o3.P, np));
        FEDD_TRY(cap.piece(G::P2, Sx + o3.P));
        hipLaunchKernelGGL(k_ss_pass2<S>, dim3(1), f.blk, pass2_lds, f.st, Sx, f.o, o3, k, sa, f.m, c->gmres_chol_tol, d_sa, hout_dev);
        FEDD_TRY(cap.piece(G::CF2, Sx + o3.cf2));
        FEDD_TRY(cap.piece(G::RI2, Sx + o3.ri2));
        FEDD_TRY(cap.piece(G::SA2, d_sa, 1, sizeof(int32_t)));
        FEDD_TRY(cap.piece(G::SA2, Sx + f.o.misc + 4, 1, sizeof(double), 1));   // the accepted count as the host reads it
        FEDD_TRY(cap.piece(G::TH, Sx + o3.th));
        FEDD_TRY(cap.piece(G::H, Sx + o3.Hraw));
        if (!hout_dev) {
            FEDD_HIP(hipMemcpyAsync(hout, Sx + f.o.misc + 4, 2 * sizeof(double), hipMemcpyDeviceToHost, f.st));
            FEDD_HIP(hipMemcpyAsync(hout + 2, Sx + o3.res, S * sizeof(double), hipMemcpyDeviceToHost, f.st));
        }
        FEDD_HIP(hipEventRecord(ev, f.st));
        // a block that fills the restart cycle is followed by the solution update over all its columns: the second
        // update forms that combination while it has the basis in hand (one read of the basis less per cycle)
        const bool comb = wide && c->gmres_fuse != 0 && f.nr == 1 && k - 1 + sa == f.m && sa >= 2;
        if (comb) f.backsolve(k - 1 + sa);
        update(k, sa, o3.cf2, o3.ri2, comb);
        precomb_cols = comb ? k - 1 + sa : -1;
        FEDD_TRY(cap.piece(G::W2, W));
        FEDD_TRY(cap.piece(G::VEND, f.V));
        cap.end(fused);
        t.stop();
        return 0;
    }

    // a cycle starts from r = b - A x, the true residual (start / trial): [project it, x += Pc r, r = b - A x;] V_0 = r / ||r||
    int begin_cycle(StopRule& rule, bool first) {
        if (f.project && !first) {
            double ta = 0.0;
            FEDD_TRY(coarse_apply_add(c, f.r, call.x));
            FEDD_TRY(trial(0, &ta));
            rule.projected(ta);
        }
        hipLaunchKernelGGL(k_ss_cycle_init, dim3(1), dim3(256), 0, f.st, f.S, f.o, o3, f.m, S, (const double*)(f.S + f.o.nrm + 3));
        f.first_basis_vector();
        spec_done = 0;
        spec_k = -1;
        return 0;
    }

    // The block's outcome as the host reads it: the accepted columns, breakdown, the recurrence residual after each new column.
    // A claim of the recurrence is checked against the true residual of a trial solution, and the stopping rule says how to go
    // on; k moves behind the accepted columns if it says nothing else.
    int block_result(StopRule& rule, int& k, int sa, StopRule::Next* next) {
        const int sa_eff = (int)hout[0];
        const bool brk = hout[1] != 0.0;
        const int ncolH = brk ? 1 : sa_eff;
        ++c->gmres_blocks;
        if (sa_eff < sa) ++c->gmres_cut_blocks;
        if (sa_eff < sa || brk) precomb_cols = -1;      // (the columns behind a cut are not what y was solved for)
        FEDD_CHECK(ncolH >= 1 && ncolH <= S, "gmres (s-step): block result %d", ncolH);
        double ta = 0.0;
        for (int i = 0; i < ncolH && *next == StopRule::GO_ON; ++i) {
            const double rec = hout[2 + i];
            if (!rule.column(rec)) continue;
            const int cols = k + i;
            FEDD_TRY(trial(cols, &ta));
            if (dbg) fprintf(stderr, "[gmres s-step] k %d block col %d: claim with %d columns, recurrence %.3e true %.3e target %.3e (s %d)\n",
                             k, i, cols, rec / f.beta0, ta / f.beta0, call.rtol, rule.s_cur);
            const StopRule::Answer ans = rule.claim(cols, rec, ta);
            FEDD_TRY(keep(ans.keep));
            *next = ans.next;
        }
        if (*next != StopRule::GO_ON) return 0;
        if (brk) {   // the Krylov space is exhausted (or numerically so): the true residual decides
            FEDD_TRY(trial(k, &ta));
            const StopRule::Answer ans = rule.breakdown(k, ta);
            FEDD_TRY(keep(ans.keep));
            *next = ans.next;
            return 0;
        }
        k += sa_eff;
        if (sa_eff < sa) {
            rule.cut(sa_eff);
        } else if (newton && !have_shifts && k - 1 >= s_goal) {
            FEDD_TRY(newton_shifts());
            if (have_shifts) rule.s_cur = s_goal;
        }
        return 0;
    }

    int solve(int s, int* its_out, double* relres_out) {
        FEDD_TRY(setup(s));
        FEDD_TRY(f.start(axt, 0));
        if (!(f.beta0 > 0)) {
            f.report(its_out, relres_out);
            return 0;
        }
        FEDD_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (dbg) fprintf(stderr, "[gmres s-step] basis at %p (%zu MB), ldv %lld\n", (void*)f.V, c->d_V.cap * sizeof(double) >> 20, (long long)f.ldv);
        c->gmres_blocks = 0;
        c->gmres_cut_blocks = 0;
        c->gmres_fused_blocks = 0;
        StopRule rule(call.rtol, f.beta0, std::min(s_goal, 8));
        StopRule::Next next = StopRule::RESTART;
        for (bool first = true; next != StopRule::STOP && rule.its < max_it; first = false) {
            FEDD_TRY(begin_cycle(rule, first));
            next = StopRule::GO_ON;
            int k = 1;                 // final basis vectors; k - 1 Hessenberg columns are final
            while (next == StopRule::GO_ON) {
                const int sa = std::min(rule.s_cur, room(k, rule.its));
                if (sa <= 0) break;
                FEDD_TRY(apply_block(k, sa));
                FEDD_TRY(orthogonalise(k, sa));
                FEDD_TRY(speculate(k + sa, rule.its, rule.s_cur));
                FEDD_HIP(hipEventSynchronize(ev));
                FEDD_TRY(block_result(rule, k, sa, &next));
            }
            if (next == StopRule::GO_ON) {   // cycle used up (restart length or iteration limit)
                double ta = 0.0;
                FEDD_TRY(trial(k - 1, &ta));
                const StopRule::Answer ans = rule.cycle_used_up(k - 1, ta);
                FEDD_TRY(keep(ans.keep));
                next = ans.next;
            }
        }
        f.its = rule.its;
        f.relres = rule.relres;
        c->gmres_floor = rule.floor;
        c->gmres_rec_relres = rule.rec_relres;
        return f.finish(its_out, relres_out);
    }
};

int gmres_solve_sstep(fedd_ctx* c, const GmresCall& call, int s, int* its_out, double* relres_out) {
    if (s <= 4) return SStep<4>(c, call).solve(s, its_out, relres_out);
    if (s <= 8) return SStep<8>(c, call).solve(s, its_out, relres_out);
    return SStep<16>(c, call).solve(s, its_out, relres_out);
}

int gmres_capture_arm(fedd_ctx* c, int block) {
    GmresCapture& g = c->gm_cap;
    if (block < 0) {
        g.armed = -1;
        g.captured = false;
        g.buf.release();
        return 0;
    }
    FEDD_CHECK(c->nranks == 1, "fedd_gmres_capture_arm: one rank only (this context has %d)", c->nranks);
    FEDD_CHECK(c->device >= 0, "this call needs a GPU context (fedd_ctx_create with device >= 0); there is no CPU fallback");
    g.armed = block;
    g.captured = false;
    return 0;
}

static const char* const capture_names[GmresCapture::NPIECE] = {"V0", "C0", "P1", "CF1", "RI1", "SA1", "W1", "P2",
                                                                "CF2", "RI2", "SA2", "TH", "W2", "H", "VEND"};

int gmres_capture_get(fedd_ctx* c, const char* what, double* out, int64_t cap) {
    typedef GmresCapture G;
    G& g = c->gm_cap;
    int p = 0;
    while (p < G::NPIECE && strcmp(what, capture_names[p]) != 0) ++p;
    FEDD_CHECK(p < G::NPIECE, "fedd_gmres_capture_get: no piece is named '%s'", what);
    FEDD_CHECK(g.captured, "fedd_gmres_capture_get: nothing captured (fedd_gmres_capture_arm, then an s-step solve that reaches that block)");
    FEDD_CHECK(g.len[p] > 0, "fedd_gmres_capture_get: '%s' was not captured (block at k %d with %d of %d columns asked)", what, g.k, g.sa_req,
               g.m + 1);
    FEDD_HIP(hipStreamSynchronize(c->stream));
    size_t cnt = g.len[p];
    int32_t sa[2] = {0, 0};
    if (p == G::SA1 || p == G::SA2 || p == G::H || p == G::VEND)
        FEDD_HIP(hipMemcpy(sa, g.buf.p + g.off[p == G::SA1 ? G::SA1 : G::SA2], sizeof(sa), hipMemcpyDeviceToHost));
    // the pieces taken after pass 2 end at the columns it accepted (a breakdown still writes Hessenberg column k - 1)
    if (p == G::H) cnt = (size_t)(g.k - 1 + std::max(sa[0], 1)) * (g.m + 1);
    if (p == G::VEND) cnt = (size_t)(g.k + sa[0]) * g.ldv;
    FEDD_CHECK(cap >= (int64_t)cnt, "fedd_gmres_capture_get: '%s' has %lld values, the buffer holds %lld", what, (long long)cnt, (long long)cap);
    if (p == G::SA1 || p == G::SA2) {
        out[0] = (double)sa[0];
        if (p == G::SA2) FEDD_HIP(hipMemcpy(out + 1, g.buf.p + g.off[p] + 1, sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    }
    FEDD_HIP(hipMemcpy(out, g.buf.p + g.off[p], cnt * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace fedd
