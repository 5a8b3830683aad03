// Numeric FE assembly on the device.  Every kernel is a gather: each CSR slot receives its element contributions in the
// order of its node's sorted (element, local index) adjacency, with no atomics, so the matrices are bitwise reproducible.
//   element-major tiles (assemble_tiles.hip): P1 Laplace, vector Laplace and elasticity, the default for those forms;
//   k_elem_matrix + k_p2_gather: the P2 scalar forms -- element matrices once per element, rows summed through gather lists;
//   k_assemble_slots: one lane per (row, element) pair, contributions added by CSR slot -- the block forms (elasticity,
//       B / B^T) where tiles do not apply;
//   k_assemble_pairs: one lane per (row, element) pair, every slot sweeps its row's contributions -- the other forms and
//       the fallback of all of the above.
// launch_assemble is the dispatch (option "asm_kind": 0 = as above, 2 = the pair sweep always, 3 = slot-addressed where it
// fits).  The load vector, the Dirichlet rows, B / B^T, the advection forms and the surface terms follow further down.
//
// Arithmetic follows (not copies) the reference's element loops:
//   FE::assemblyLaplace          feddlib/core/FE/FE_def.hpp:604-667
//   FE::assemblyLaplaceVecField  feddlib/core/FE/FE_def.hpp:670-734
//   FE::assemblyMass             feddlib/core/FE/FE_def.hpp:454-524
//   FE::assemblyLinElasXDim      feddlib/core/FE/FE_def.hpp:2739-3040 (epsilonTensor :4931-4944)
//   FE::assemblyRHS              feddlib/core/FE/FE_def.hpp:4694-4766
//   FE::buildTransformation      feddlib/core/FE/FE_def.hpp:5342-5357
//   SmallMatrix::computeInverse  feddlib/core/General/SmallMatrix.hpp:306-357
//   FE::applyBTinv               feddlib/core/FE/FE_def.hpp:83-96
//   BCBuilder::setSystem/setRHS  feddlib/core/General/BCBuilder_def.hpp:589-707, 93-170
// Quadrature points/weights and reference basis values/gradients are staged in LDS once per
// workgroup.  The forms, the kernel arguments and the simplex geometry are in assemble_common.hpp.
#include "assemble_common.hpp"
#include "gather_lists.hpp"
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <type_traits>
#include <unordered_map>

namespace fedd {
namespace {

__device__ __forceinline__ int find_slot(const int32_t* __restrict__ cols, int n, int32_t col) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cols[mid] < col) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------
// Pair-parallel variant (the fallback; asm_kind 2: always).  A workgroup owns R consecutive dof rows.
//   phase 1: one lane per (row, incident element) pair evaluates that row of the element matrix
//            and parks (column id, value) in LDS -- all global-memory latency (adjacency, element
//            nodes, coordinates) is overlapped across ~24x more lanes than rows;
//   phase 2: `tpr` lanes per row, lane s owns CSR slot s: it sweeps the row's parked
//            contributions in their fixed order and adds those whose column id is its own
//            (LDS broadcast reads, no search, no atomics), then the workgroup's CSR range
//            is written as one contiguous coalesced stream.
// Summation order is fixed by the sorted adjacency list => bitwise reproducible.
// ---------------------------------------------------------------------------------------------
template <int DIM, int NEN, int FORM>
struct PairCfg {
    // contributions per (row, element) pair
    static constexpr int CPP = (FORM == F_LINELAS || FORM == F_DIV) ? NEN * DIM : (FORM == F_DIVT ? DIM + 1 : NEN);
};

// row `li` (component `comp`) of the element matrix of an element with nodes nd and vertex coordinates X:
// CPP (column id, value) contributions
template <int DIM, int NEN, int FORM>
__device__ __forceinline__ void compute_pair(const AsmArgs& a, const double* __restrict__ s_w,
                                             const double* __restrict__ s_phi, const double* __restrict__ s_dphi, int nq,
                                             const int32_t (&nd)[NEN], const double (&X)[DIM + 1][DIM], int li, int comp,
                                             int dofs, int32_t (&cols)[PairCfg<DIM, NEN, FORM>::CPP],
                                             double (&vals)[PairCfg<DIM, NEN, FORM>::CPP]) {
    if constexpr (FORM == F_MASS) {
        const double absdet = fabs(affine_det<DIM>(X));
#pragma unroll
        for (int j = 0; j < NEN; ++j) {
            double v = 0.0;
            for (int q = 0; q < nq; ++q) v += s_w[q] * s_phi[q * NEN + li] * s_phi[q * NEN + j];
            cols[j] = nd[j] * dofs + comp;
            // assemblyBDStabilization (FE_def.hpp:2204-2206): value *= absDetB; value -= refElementSize * absDetB * refElementScale
            // (p0 = p1 = 0 for the plain mass matrix: x - 0 = x)
            vals[j] = v * absdet - a.p0 * absdet * a.p1;
        }
    } else {
        // Quadrature loop outermost, the transformed gradient of the row's basis function once per point and that
        // of each column function once per (point, column).  On P1 elements the gradients do not depend on the
        // point: all of them are formed once.  (The kernel is bound by f64 issue: the earlier form re-derived both
        // gradients inside the column loop, 345 f64 instructions per pair for P1 Laplace against ~130 now; the
        // expressions and their order are unchanged, so are the bits.)
        constexpr bool P1 = NEN == DIM + 1;
        double Binv[DIM][DIM];
        const double absdet = fabs(affine<DIM>(X, Binv));
        double gi[DIM], G[P1 ? NEN : 1][DIM];
        if constexpr (P1) {
            grad_t<DIM, NEN>(s_dphi, 0, li, Binv, gi);
#pragma unroll
            for (int j = 0; j < NEN; ++j) grad_t<DIM, NEN>(s_dphi, 0, j, Binv, G[j]);
        }
        if constexpr (FORM == F_LAPLACE) {
            double v[NEN];
#pragma unroll
            for (int j = 0; j < NEN; ++j) v[j] = 0.0;
            for (int q = 0; q < nq; ++q) {
                if constexpr (!P1) grad_t<DIM, NEN>(s_dphi, q, li, Binv, gi);
                double wg[DIM];
#pragma unroll
                for (int d = 0; d < DIM; ++d) wg[d] = s_w[q] * gi[d];
#pragma unroll
                for (int j = 0; j < NEN; ++j) {
                    double gj[DIM];
                    if constexpr (P1) {
#pragma unroll
                        for (int d = 0; d < DIM; ++d) gj[d] = G[j][d];
                    } else {
                        grad_t<DIM, NEN>(s_dphi, q, j, Binv, gj);
                    }
#pragma unroll
                    for (int d = 0; d < DIM; ++d) v[j] += wg[d] * gj[d];
                }
            }
#pragma unroll
            for (int j = 0; j < NEN; ++j) {
                cols[j] = nd[j] * dofs + comp;
                vals[j] = zero_small(a, v[j] * absdet);
            }
        } else if constexpr (FORM == F_DIV) {
            // row = pressure node (vertex li): B_{i,(j,d)} = |detB| sum_q w_q psi_qi dphi_qjd  (FE_def.hpp:1992-2004)
            const double* __restrict__ s_psi = s_dphi + nq * NEN * DIM;
            double vd[NEN][DIM];
#pragma unroll
            for (int j = 0; j < NEN; ++j)
#pragma unroll
                for (int d = 0; d < DIM; ++d) vd[j][d] = 0.0;
            for (int q = 0; q < nq; ++q) {
                const double wp = s_w[q] * s_psi[q * (DIM + 1) + li];
#pragma unroll
                for (int j = 0; j < NEN; ++j) {
                    double gj[DIM];
                    if constexpr (P1) {
#pragma unroll
                        for (int d = 0; d < DIM; ++d) gj[d] = G[j][d];
                    } else {
                        grad_t<DIM, NEN>(s_dphi, q, j, Binv, gj);
                    }
#pragma unroll
                    for (int d = 0; d < DIM; ++d) vd[j][d] += wp * gj[d];
                }
            }
#pragma unroll
            for (int j = 0; j < NEN; ++j)
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    cols[j * DIM + d] = nd[j] * DIM + d;
                    vals[j * DIM + d] = zero_small(a, absdet * vd[j][d]);
                }
        } else if constexpr (FORM == F_DIVT) {
            // row = velocity dof (node li, component comp): B^T_{(i,d),j} = |detB| sum_q w_q psi_qj dphi_qid  (:2022-2046)
            const double* __restrict__ s_psi = s_dphi + nq * NEN * DIM;
            double vj[DIM + 1];
#pragma unroll
            for (int j = 0; j <= DIM; ++j) vj[j] = 0.0;
            for (int q = 0; q < nq; ++q) {
                if constexpr (!P1) grad_t<DIM, NEN>(s_dphi, q, li, Binv, gi);
                double gc = 0.0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) gc = d == comp ? gi[d] : gc;
#pragma unroll
                for (int j = 0; j <= DIM; ++j) vj[j] += s_w[q] * s_psi[q * (DIM + 1) + j] * gc;
            }
#pragma unroll
            for (int j = 0; j <= DIM; ++j) {
                cols[j] = nd[j];
                vals[j] = zero_small(a, absdet * vj[j]);
            }
        } else {
            const double lam = a.p0, mu = a.p1;
            double vb[NEN][DIM];
#pragma unroll
            for (int j = 0; j < NEN; ++j)
#pragma unroll
                for (int b = 0; b < DIM; ++b) vb[j][b] = 0.0;
            for (int q = 0; q < nq; ++q) {
                if constexpr (!P1) grad_t<DIM, NEN>(s_dphi, q, li, Binv, gi);
                double gia = 0.0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) gia = d == comp ? gi[d] : gia;
#pragma unroll
                for (int j = 0; j < NEN; ++j) {
                    double gj[DIM];
                    if constexpr (P1) {
#pragma unroll
                        for (int d = 0; d < DIM; ++d) gj[d] = G[j][d];
                    } else {
                        grad_t<DIM, NEN>(s_dphi, q, j, Binv, gj);
                    }
                    double dot = 0.0, gja = 0.0;
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        dot += gi[d] * gj[d];
                        gja = d == comp ? gj[d] : gja;
                    }
                    // 2 mu eps_i:eps_j + lam tr(eps_i) tr(eps_j) with eps from epsilonTensor (FE_def.hpp:4931-4944)
#pragma unroll
                    for (int b = 0; b < DIM; ++b)
                        vb[j][b] += s_w[q] * (mu * ((b == comp ? dot : 0.0) + gi[b] * gja) + lam * gia * gj[b]);
                }
            }
#pragma unroll
            for (int j = 0; j < NEN; ++j)
#pragma unroll
                for (int b = 0; b < DIM; ++b) {
                    cols[j * DIM + b] = nd[j] * dofs + b;
                    vals[j * DIM + b] = absdet * vb[j][b];
                }
        }
    }
}

template <int DIM, int NEN, int FORM>
__device__ __forceinline__ void eval_pair(const AsmArgs& a, const double* __restrict__ s_w,
                                          const double* __restrict__ s_phi, const double* __restrict__ s_dphi, int nq,
                                          int32_t e, int li, int comp, int dofs,
                                          int32_t (&cols)[PairCfg<DIM, NEN, FORM>::CPP],
                                          double (&vals)[PairCfg<DIM, NEN, FORM>::CPP]) {
    int32_t nd[NEN];
#pragma unroll
    for (int j = 0; j < NEN; ++j) nd[j] = a.conn[(int64_t)e * NEN + j];
    if constexpr ((FORM == F_LAPLACE || FORM == F_MASS) && NEN > DIM + 1) {
        if (a.ke) {     // row li of the element matrix k_elem_matrix left behind: NEN contiguous values
            const double* __restrict__ kr = a.ke + ((int64_t)e * NEN + li) * NEN;
#pragma unroll
            for (int j = 0; j < NEN; ++j) {
                cols[j] = nd[j] * dofs + comp;
                vals[j] = kr[j];
            }
            return;
        }
    }
    double X[DIM + 1][DIM];
#pragma unroll
    for (int v = 0; v <= DIM; ++v)
#pragma unroll
        for (int d = 0; d < DIM; ++d) X[v][d] = a.xyz[(int64_t)nd[v] * DIM + d];
    compute_pair<DIM, NEN, FORM>(a, s_w, s_phi, s_dphi, nq, nd, X, li, comp, dofs, cols, vals);
}

template <int DIM, int NEN, int FORM>
__global__ __launch_bounds__(256) void k_assemble_pairs(AsmArgs a, int R, int tpr_log2, int cap_contrib) {
    constexpr int CPP = PairCfg<DIM, NEN, FORM>::CPP;
    extern __shared__ double sm[];
    const int nq = a.nq;
    const int ntab = nq * (1 + NEN + NEN * DIM + DIM + 1);
    double* s_w = sm;
    double* s_phi = s_w + nq;
    double* s_dphi = s_phi + nq * NEN;
    double* cval = sm + ntab;
    int32_t* ccol = reinterpret_cast<int32_t*>(cval + cap_contrib);
    int32_t* off = ccol + cap_contrib;
    const int tid = threadIdx.x;
    for (int i = tid; i < ntab; i += 256) sm[i] = a.tab[i];
    const int dofs = a.dofs;
    // each XCD takes a contiguous eighth of the rows: rows of neighbouring node lines share elements, whose
    // connectivity and coordinates then meet in one L2 (PMC traffic 2.7x -> 1.75x the algorithmic bytes at 100^3 cells)
    const int32_t nwg = gridDim.x, q8 = nwg >> 3, rem8 = nwg & 7, xcd = blockIdx.x & 7, within = blockIdx.x >> 3;
    const int32_t wg = (xcd < rem8 ? xcd * (q8 + 1) : rem8 * (q8 + 1) + (xcd - rem8) * q8) + within;
    const int32_t r0 = wg * R;
    const int nrows = min(R, a.n_rows - r0);
    // exclusive prefix of the rows' pair counts: first wave, one lane per row (R <= 64), DPP scan
    if (tid < 64) {
        int deg = 0;
        if (tid < nrows) {
            const int32_t node = (r0 + tid) / dofs;
            deg = a.n2e_ptr[node + 1] - a.n2e_ptr[node];
        }
        int incl = deg;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (tid >= d) incl += t;
        }
        if (tid <= nrows) off[tid] = incl - deg;
    }
    __syncthreads();
    const int npairs = off[nrows];
    // the contributions of local row r start at (off[r]*CPP + r*PAD): the odd-ish shift keeps the
    // rows that one wave sweeps together in phase 2 on different LDS banks
    constexpr int PAD = 2;
    for (int i = tid; i < npairs; i += 256) {
        int lo = 0, hi = nrows - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        const int32_t row = r0 + lo;
        const int32_t node = row / dofs;
        const int comp = row - node * dofs;
        const int32_t idx = a.n2e[a.n2e_ptr[node] + (i - off[lo])];
        const int32_t e = idx / NEN;
        const int li = idx - e * NEN;
        int32_t cols[CPP];
        double vals[CPP];
        eval_pair<DIM, NEN, FORM>(a, s_w, s_phi, s_dphi, nq, e, li, comp, dofs, cols, vals);
        const int base = i * CPP + lo * PAD;
#pragma unroll
        for (int c = 0; c < CPP; ++c) {
            ccol[base + c] = cols[c];
            cval[base + c] = vals[c];
        }
    }
    __syncthreads();
    const int tpr = 1 << tpr_log2;
    for (int item = tid; item < (nrows << tpr_log2); item += 256) {
        const int rl = item >> tpr_log2, s0 = item & (tpr - 1);
        const int32_t rs = a.rowptr[r0 + rl];
        const int rn = a.rowptr[r0 + rl + 1] - rs;
        const int cb = off[rl] * CPP + rl * PAD, ce = off[rl + 1] * CPP + rl * PAD;
        for (int s = s0; s < rn; s += tpr) {
            const int32_t mycol = a.colind[rs + s];
            double acc = 0.0;
            int c = cb;
            // 8 contributions per trip, all 16 LDS reads issued before the first use (a
            // data-dependent read of cval would serialise two LDS latencies per contribution)
            for (; c + 8 <= ce; c += 8) {
                int32_t cc[8];
                double vv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    cc[u] = ccol[c + u];
                    vv[u] = cval[c + u];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += cc[u] == mycol ? vv[u] : 0.0;
            }
            for (; c < ce; ++c) {
                const int32_t cc = ccol[c];
                const double vv = cval[c];
                acc += cc == mycol ? vv : 0.0;
            }
            a.val[rs + s] = acc;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Slot-addressed variant (asm_kind 0: the block forms; 3: wherever it fits).  A workgroup owns R consecutive dof rows, i.e. one
// contiguous range of the CSR arrays, and keeps an image of that range in LDS:
//   phase 0: the range's column ids -> LDS (coalesced), accumulators zeroed;
//   phase 1: one lane per (row, incident element) pair, as in the pair-parallel kernel (adjacency
//            entry -> element nodes -> vertex coordinates); each contribution's CSR slot is found
//            by a binary search of its column id in the row's LDS-resident column list, and
//            (slot, value) is parked in LDS;
//   phase 2: one lane per row adds its parked contributions into the LDS image in their fixed order
//            (adjacency order, then local column order): no atomics, no sweep over the row's other
//            contributions -- 96 read-modify-writes per P1 row instead of 15 slots x 96 compares;
//   phase 3: the image is written to HBM as one contiguous coalesced stream.
// Summation order is fixed by the sorted adjacency list => bitwise reproducible.  Workgroups are
// remapped so that each XCD takes a contiguous eighth of the rows (rows of neighbouring node lines
// share elements: their connectivity and coordinates then meet in one L2).
// ---------------------------------------------------------------------------------------------
template <int DIM, int NEN, int FORM>
__global__ __launch_bounds__(256) void k_assemble_slots(AsmArgs a, int R, int cap_contrib, int cap_cols, int nwg) {
    constexpr int CPP = PairCfg<DIM, NEN, FORM>::CPP;
    constexpr int PADV = 1, PADS = 2;        // per-row shifts of the parks: the lanes of phase 2 (one per row) hit different banks
    extern __shared__ double sm[];
    const int nq = a.nq;
    const int ntab = nq * (1 + NEN + NEN * DIM + DIM + 1);
    double* s_w = sm;
    double* s_phi = s_w + nq;
    double* s_dphi = s_phi + nq * NEN;
    double* cval = sm + ntab;                                   // [cap_contrib]
    double* acc = cval + cap_contrib;                           // [cap_cols]   image of val[rs0, rs0 + ncols)
    int32_t* scol = reinterpret_cast<int32_t*>(acc + cap_cols); // [cap_cols]   image of colind[...]
    int32_t* off = scol + cap_cols;                             // [R + 1]      pair offsets of the rows
    int32_t* rbase = off + R + 1;                               // [R + 1]      row starts relative to rs0
    uint16_t* cslot = reinterpret_cast<uint16_t*>(rbase + R + 1);   // [cap_contrib] position in the image
    const int tid = threadIdx.x;
    const int32_t q8 = nwg >> 3, rem8 = nwg & 7, xcd = blockIdx.x & 7, within = blockIdx.x >> 3;
    const int32_t wg = (xcd < rem8 ? xcd * (q8 + 1) : rem8 * (q8 + 1) + (xcd - rem8) * q8) + within;
    for (int i = tid; i < ntab; i += 256) sm[i] = a.tab[i];
    const int dofs = a.dofs;
    const int32_t r0 = wg * R;
    const int nrows = min(R, a.n_rows - r0);
    const int32_t rs0 = a.rowptr[r0];
    if (tid < 64) {   // exclusive prefix of the rows' pair counts; row starts
        int deg = 0;
        if (tid < nrows) {
            const int32_t node = (r0 + tid) / dofs;
            deg = a.n2e_ptr[node + 1] - a.n2e_ptr[node];
        }
        int incl = deg;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (tid >= d) incl += t;
        }
        if (tid <= nrows) {
            off[tid] = incl - deg;
            rbase[tid] = a.rowptr[r0 + tid] - rs0;
        }
    }
    __syncthreads();
    const int npairs = off[nrows];
    const int ncols = rbase[nrows];
    for (int i = tid; i < ncols; i += 256) {
        scol[i] = a.colind[rs0 + i];
        acc[i] = 0.0;
    }
    __syncthreads();
    for (int i = tid; i < npairs; i += 256) {
        // the row of the pair by binary search over the offsets, its adjacency entry
        int lo = 0, hi = nrows - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        const int32_t node = (r0 + lo) / dofs;
        const int32_t idx = a.n2e[a.n2e_ptr[node] + (i - off[lo])];
        const int32_t e = idx / NEN;
        const int li = idx - e * NEN;
        int32_t nd[NEN];
#pragma unroll
        for (int j = 0; j < NEN; ++j) nd[j] = a.conn[(int64_t)e * NEN + j];
        double X[DIM + 1][DIM];
#pragma unroll
        for (int v = 0; v <= DIM; ++v)
#pragma unroll
            for (int d = 0; d < DIM; ++d) X[v][d] = a.xyz[(int64_t)nd[v] * DIM + d];
        const int comp = (r0 + lo) % dofs;
        int32_t cols[CPP];
        double vals[CPP];
        compute_pair<DIM, NEN, FORM>(a, s_w, s_phi, s_dphi, nq, nd, X, li, comp, dofs, cols, vals);
        const int lb = rbase[lo], ln = rbase[lo + 1] - lb;
        const int bv = i * CPP + lo * PADV, bs = i * CPP + lo * PADS;
#pragma unroll
        for (int c = 0; c < CPP; ++c) {
            cval[bv + c] = vals[c];
            cslot[bs + c] = (uint16_t)(lb + find_slot(scol + lb, ln, cols[c]));
        }
    }
    __syncthreads();
    // L lanes per row: lane t adds the contributions c = j L + t, j = 0..NEN-1 (for the block forms: column
    // component t of every element node).  Two contributions of one pair never share a slot, and lanes t != t' never
    // touch the same slot at all, so every slot still receives its terms in adjacency order.
    constexpr int L = CPP % NEN == 0 ? CPP / NEN : 1, CPL = CPP / L;
    if (tid < nrows * L) {
        const int row = tid / L, t = tid - row * L;
        const int pb = off[row], pe = off[row + 1];
        for (int i = pb; i < pe; ++i) {
            const int bv = i * CPP + row * PADV, bs = i * CPP + row * PADS;
            double vv[CPL];
            int ss[CPL];
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                vv[j] = cval[bv + j * L + t];
                ss[j] = cslot[bs + j * L + t];
            }
#pragma unroll
            for (int j = 0; j < CPL; ++j) acc[ss[j]] += vv[j];
        }
    }
    __syncthreads();
    for (int i = tid; i < ncols; i += 256) a.val[rs0 + i] = acc[i];
}

struct RhsArgs {
    const int32_t* conn;
    const int32_t* n2e_ptr;
    const int32_t* n2e;
    const double* xyz;
    double* rhs;
    int32_t n_own;
    int nen, dofs;
    double base[10];  // sum_q w_q phi_q,i
    double f[MAX_DOFS];
};

// load vector in two phases: |det B_e| of every element (coalesced over elements), then each owned
// node sums base[local index] * |det| over its adjacent elements in adjacency order
template <int DIM>
__global__ void k_elem_absdet(const int32_t* __restrict__ conn, int nen, const double* __restrict__ xyz,
                              int64_t n_elem, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_elem) return;
    double X[DIM + 1][DIM];
#pragma unroll
    for (int v = 0; v <= DIM; ++v) {
        const int32_t nd = conn[e * nen + v];
#pragma unroll
        for (int d = 0; d < DIM; ++d) X[v][d] = xyz[(int64_t)nd * DIM + d];
    }
    out[e] = fabs(affine_det<DIM>(X));
}

// RHS_NPB nodes per workgroup: the (node, element) pairs of the workgroup are one contiguous run
// of the adjacency, read coalesced with one lane per pair into an LDS park; then one lane per
// node adds its segment in adjacency order (the order does not depend on the launch shape).
constexpr int RHS_NPB = 64;

__global__ __launch_bounds__(256) void k_rhs(RhsArgs a, const double* __restrict__ absdet, int cap) {
    extern __shared__ double park[];
    const int32_t node0 = blockIdx.x * RHS_NPB;
    const int32_t node1 = min(a.n_own, node0 + RHS_NPB);
    const int32_t p0 = a.n2e_ptr[node0];
    const int tid = threadIdx.x;
    const int32_t node = node0 + tid;
    const bool mine = tid < RHS_NPB && node < node1;
    const int32_t nb = mine ? a.n2e_ptr[node] : 0, ne = mine ? a.n2e_ptr[node + 1] : 0;
    double sum = 0.0;
    // the run is processed in windows of `cap` pairs (one window unless a node has very many elements)
    for (int32_t w0 = p0; w0 < a.n2e_ptr[node1]; w0 += cap) {
        const int32_t w1 = min(a.n2e_ptr[node1], w0 + cap);
        // (four pairs per lane and trip: their adjacency entries, then their |det B|, requested together)
        for (int32_t q0 = w0 + tid; q0 < w1; q0 += 256 * 4) {
            int32_t idx[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) idx[u] = a.n2e[min(q0 + 256 * u, w1 - 1)];
            double ad[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) ad[u] = absdet[idx[u] / a.nen];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t p = q0 + 256 * u;
                if (p < w1) {
                    const int li = idx[u] - (idx[u] / a.nen) * a.nen;
                    double b = 0.0;
                    for (int i = 0; i < 10; ++i) b = i == li ? a.base[i] : b;
                    park[p - w0] = b * ad[u];
                }
            }
        }
        __syncthreads();
        for (int32_t p = max(nb, w0); p < min(ne, w1); ++p) sum += park[p - w0];
        __syncthreads();
    }
    if (mine)
        for (int d = 0; d < a.dofs; ++d) a.rhs[(int64_t)node * a.dofs + d] = sum * a.f[d];
}

__global__ void k_dirichlet(BcTable b, const int32_t* __restrict__ nflag, const int32_t* __restrict__ rowptr,
                            const int32_t* __restrict__ colind, double* val, double* rhs, int32_t* isdir,
                            int32_t n_rows) {
    const int32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const int32_t node = row / b.dofs;
    const int comp = row - node * b.dofs;
    const int hit = bc_hit(b, nflag[node], comp);
    if (hit < 0) return;
    for (int32_t p = rowptr[row]; p < rowptr[row + 1]; ++p) val[p] = colind[p] == row ? 1.0 : 0.0;
    rhs[row] = b.value[hit * b.dofs + comp];
    isdir[row] = 1;
}

// per-node variant: node list + per-dof mask/value (what BCBuilder::setRHS obtains by evaluating
// the user's boundary function at every flagged unique node, BCBuilder_def.hpp:128-143)
__global__ void k_dirichlet_nodes(const int32_t* __restrict__ nodes, const int32_t* __restrict__ mask,
                                  const double* __restrict__ values, int32_t n, int dofs,
                                  const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind, double* val,
                                  double* rhs, int32_t* isdir) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * dofs) return;
    const int32_t k = t / dofs;
    const int comp = t - k * dofs;
    if (mask && !mask[t]) return;
    const int32_t row = nodes[k] * dofs + comp;
    for (int32_t p = rowptr[row]; p < rowptr[row + 1]; ++p) val[p] = colind[p] == row ? 1.0 : 0.0;
    rhs[row] = values[t];
    isdir[row] = 1;
}

// ---------------------------------------------------------------------------------------------
// P2 elements, scalar forms (FE::assemblyLaplace / assemblyMass with the 10 x 10 -- 2D: 6 x 6 -- element matrices of
// FE_def.hpp:637-665, 485-499): element-major evaluation, ONE ELEMENT PER WAVEFRONT.  The quadrature weights and the reference
// basis values / gradients are staged in LDS once per workgroup; a wave loads its element's vertices, forms B^-1 and |det B|,
// parks the transformed gradients of all basis functions at all quadrature points in LDS (nq x NEN x DIM values), and its
// lanes then take the NEN^2 entries of the element matrix, which leave as one contiguous 800-byte stream.  The rows of the
// global matrix are then summed from these element matrices by the pair kernels (k_assemble_pairs reads row li of element e
// instead of re-deriving it: the pair kernels alone evaluate every P2 element ten times, 11.4 ms at a 64^3-cell cube against
// the figure in DESIGN.md section 4 with this kernel) -- in adjacency order, no atomics: bitwise reproducible as before.
// ---------------------------------------------------------------------------------------------
// SCALED (a compile-time switch; F_LAPLACE only): the element carries a coefficient f = a.fscale[e], the scaled vector
// Laplacian of FE::assemblyLaplaceXDim (FE_def.hpp:2225-2402): val += (f w_k) (grad phi_j . grad phi_i), |det B| last, and no
// doSetZeros.  The unscaled instantiations keep their code and their bits.
template <int DIM, int NEN, int FORM, bool SCALED = false>
__global__ __launch_bounds__(256) void k_elem_matrix(AsmArgs a, int64_t n_elem, double* __restrict__ ke) {
    extern __shared__ double sm[];
    const int nq = a.nq, ntab = nq * (1 + NEN + NEN * DIM + DIM + 1);
    double* s_w = sm;
    double* s_phi = s_w + nq;
    double* s_dphi = s_phi + nq * NEN;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    double* Gs = sm + ntab + (ntab & 1) + (size_t)w * nq * NEN * DIM;       // this wave's transformed gradients [q][i][d]
    for (int i = tid; i < ntab; i += 256) sm[i] = a.tab[i];
    __syncthreads();
    const int64_t nwave = (int64_t)gridDim.x * 4;
    const int64_t trips = (n_elem + nwave - 1) / nwave;
    for (int64_t k = 0; k < trips; ++k) {
        const int64_t e = k * nwave + (int64_t)blockIdx.x * 4 + w;
        const bool on = e < n_elem;
        // vertices = the first DIM + 1 nodes of the element; lane l < (DIM + 1) DIM holds coordinate (l / DIM, l % DIM)
        double xv = 0.0;
        if (on && lane < (DIM + 1) * DIM) xv = a.xyz[(int64_t)a.conn[e * NEN + lane / DIM] * DIM + (lane % DIM)];
        double X[DIM + 1][DIM];
#pragma unroll
        for (int v = 0; v <= DIM; ++v)
#pragma unroll
            for (int d = 0; d < DIM; ++d) X[v][d] = __shfl(xv, v * DIM + d, 64);
        double absdet = 0.0;
        if constexpr (FORM == F_LAPLACE) {
            double Binv[DIM][DIM];
            absdet = on ? fabs(affine<DIM>(X, Binv)) : 0.0;
            if (on)
                for (int t = lane; t < nq * NEN; t += 64) {
                    double g[DIM];
                    grad_t<DIM, NEN>(s_dphi, t / NEN, t % NEN, Binv, g);
#pragma unroll
                    for (int d = 0; d < DIM; ++d) Gs[t * DIM + d] = g[d];
                }
        } else {
            absdet = on ? fabs(affine_det<DIM>(X)) : 0.0;
        }
        __syncthreads();
        if (on) {
            double* __restrict__ out = ke + e * (NEN * NEN);
            for (int t = lane; t < NEN * NEN; t += 64) {
                const int i = t / NEN, j = t - i * NEN;
                double v = 0.0;
                if constexpr (SCALED) {
                    const double f = a.fscale[e];
                    for (int q = 0; q < nq; ++q) {
                        const double* gi = Gs + (q * NEN + i) * DIM;
                        const double* gj = Gs + (q * NEN + j) * DIM;
                        double dot = 0.0;
#pragma unroll
                        for (int d = 0; d < DIM; ++d) dot += gj[d] * gi[d];
                        v += (f * s_w[q]) * dot;
                    }
                    out[t] = absdet * v;
                } else if constexpr (FORM == F_LAPLACE) {
                    for (int q = 0; q < nq; ++q) {
                        const double* gi = Gs + (q * NEN + i) * DIM;
                        const double* gj = Gs + (q * NEN + j) * DIM;
#pragma unroll
                        for (int d = 0; d < DIM; ++d) v += s_w[q] * gi[d] * gj[d];
                    }
                    out[t] = zero_small(a, v * absdet);
                } else {
                    for (int q = 0; q < nq; ++q) v += s_w[q] * s_phi[q * NEN + i] * s_phi[q * NEN + j];
                    out[t] = v * absdet - a.p0 * absdet * a.p1;
                }
            }
        }
        __syncthreads();        // Gs is rewritten by the next trip
    }
}

// element matrices of the whole mesh into c->d_ke (P2, F_LAPLACE / F_MASS); returns the args with ke set
template <int DIM, int NEN, int FORM, bool SCALED = false>
int launch_elem_matrices(fedd_ctx* c, AsmArgs& a, int ntab) {
    FEDD_TRY(c->d_ke.ensure((size_t)c->n_elem * NEN * NEN));
    const size_t lds = ((size_t)ntab + (ntab & 1) + 4 * (size_t)a.nq * NEN * DIM) * sizeof(double);
    FEDD_CHECK(lds <= 64 * 1024, "element matrices: quadrature tables of %d points do not fit the LDS", a.nq);
    const int64_t nwg = std::min<int64_t>((c->n_elem + 3) / 4, 256 * 8);
    ScopedTimer t(c, FEDD_T_ASSEMBLE);
    hipLaunchKernelGGL((k_elem_matrix<DIM, NEN, FORM, SCALED>), dim3((unsigned)nwg), dim3(256), lds, c->stream, a, c->n_elem, c->d_ke.p);
    t.stop();
    FEDD_HIP(hipGetLastError());
    a.ke = c->d_ke.p;
    return 0;
}

template <int DIM, int NEN, int FORM>
int launch_pairs(fedd_ctx* c, const AsmArgs& a, int ntab, int64_t n_rows, int rowcap) {
    constexpr int CPP = PairCfg<DIM, NEN, FORM>::CPP;
    const int maxdeg = std::max(1, c->max_deg);
    const size_t per_row = (size_t)maxdeg * CPP * 12;  // f64 value + i32 column per contribution
    // rows per workgroup from the LDS budget: 37 KB lets four workgroups share the 160 KB of a CU (40 KB: three;
    // P1 Laplace 3D: 32 rows, 0.81 -> 0.59 ms at 100^3 cells, 7.9 -> 5.7 ms at 214^3; smaller budgets gain nothing more)
    int R = (int)std::min<size_t>(63, ((size_t)c->asm_lds_kb * 1024) / per_row);  // <= 63: one wave scans the row offsets
    if (R < 1) R = 1;
    const int cap = R * maxdeg * CPP + R * 2;                   // + the per-row bank-shift padding
    const size_t lds = (size_t)ntab * 8 + (size_t)cap * 12 + (size_t)(R + 1) * 4 + 16;
    FEDD_CHECK(lds <= 160 * 1024, "assembly: a node with %d incident elements does not fit the LDS contribution buffer", maxdeg);
    int tl = 0;
    while ((1 << tl) < std::min(64, std::max(1, rowcap))) ++tl;
    auto kern = k_assemble_pairs<DIM, NEN, FORM>;
    if (lds > 64 * 1024)
        FEDD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((unsigned)((n_rows + R - 1) / R)), block(256);
    ScopedTimer t(c, FEDD_T_ASSEMBLE);
    hipLaunchKernelGGL(kern, grid, block, lds, c->stream, a, R, tl, cap);
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}

// slot-addressed kernel; returns -1 (without error) when a row or the LDS budget does not suit it
template <int DIM, int NEN, int FORM>
int launch_slots(fedd_ctx* c, const AsmArgs& a, int ntab, int64_t n_rows, int rowcap) {
    constexpr int CPP = PairCfg<DIM, NEN, FORM>::CPP;
    const int maxdeg = std::max(1, c->max_deg);
    rowcap = std::max(1, rowcap);
    // per row: parked contributions (f64 value + u16 slot, + the bank shifts), image of the CSR row (f64 + i32)
    const size_t per_row = (size_t)maxdeg * CPP * 10 + 12 + (size_t)rowcap * 12 + 8;
    const size_t budget = (size_t)c->asm_lds_kb * 1024;
    // (R <= 63: one wave scans the row offsets, lane nrows writes the total)
    int R = (int)std::min<size_t>(63, budget > (size_t)ntab * 8 ? (budget - (size_t)ntab * 8) / per_row : 0);
    if (R < 1) R = (int)std::min<size_t>(63, (150 * 1024 - (size_t)ntab * 8) / per_row);   // large P2 rows: one workgroup per CU
    if (R < 1) return -1;
    const int cap_cols = R * rowcap;
    if (cap_cols > 65535) return -1;    // u16 positions
    int cap_contrib = R * maxdeg * CPP + R * 2 + 2;
    cap_contrib += cap_contrib & 1;     // keeps the arrays behind it 8-byte aligned
    const size_t lds = (size_t)ntab * 8 + (size_t)cap_contrib * 8 + (size_t)cap_cols * 12 + (size_t)(2 * R + 2) * 4 +
                       (size_t)cap_contrib * 2 + 16;
    if (lds > 160 * 1024) return -1;
    const int nwg = (int)((n_rows + R - 1) / R);
    auto kern = k_assemble_slots<DIM, NEN, FORM>;
    if (lds > 64 * 1024)
        FEDD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ScopedTimer t(c, FEDD_T_ASSEMBLE);
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(256), lds, c->stream, a, R, cap_contrib, cap_cols, nwg);
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}

// asm_kind 0: slot-addressed kernel, falling back to the pair-parallel sweep where it does not fit; 2: the sweep
template <int DIM, int NEN, int FORM>
int launch_matrix(fedd_ctx* c, const AsmArgs& a, int ntab, int64_t n_rows, int rowcap) {
    // Measured (one MI355X): elasticity, 94^3 cells, FULL blocks: sweep 7.9 ms, slots 5.5 ms; B / B^T likewise;
    // Laplace, 214^3 cells: sweep 5.15 ms, slots 5.5-5.7 ms (the one-wave accumulation of phase 2 costs what the sweep
    // over 96 contributions costs).  asm_kind 0 picks by the contributions per pair, 3 forces the slot kernel.
    constexpr bool many = PairCfg<DIM, NEN, FORM>::CPP > NEN;
    if (((c->asm_kind == 0 && many) || c->asm_kind == 3) && n_rows > 0) {
        const int rc = launch_slots<DIM, NEN, FORM>(c, a, ntab, n_rows, rowcap);
        if (rc >= 0) return rc;
    }
    return launch_pairs<DIM, NEN, FORM>(c, a, ntab, n_rows, rowcap);
}

// ---------------------------------------------------------------------------------------------
// Row sums of the P2 scalar forms from the element matrices of k_elem_matrix, by GATHER LISTS built once per mesh (k_p2_lists;
// gather_lists.hpp).  k_p2_gather: every lane adds its few (2.6 on average) element-matrix entries in list order, the summation
// order of the pair kernels.  (Those spend their time searching the row for every one of the 157 M contributions of a 64^3-cell
// P2 cube: 11.4 ms with or without the element matrices.)
// ---------------------------------------------------------------------------------------------
template <int NEN>
__global__ __launch_bounds__(256) void k_p2_lists(const int32_t* __restrict__ conn, const int32_t* __restrict__ n2e_ptr,
                                                  const int32_t* __restrict__ n2e, const int32_t* __restrict__ rowptr,
                                                  const int32_t* __restrict__ colind, int dofs, int full, int32_t nn,
                                                  uint16_t* __restrict__ soff, uint16_t* __restrict__ src, int32_t* __restrict__ bad) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t p = (int64_t)blockIdx.x * 4 + w; p < nn; p += (int64_t)gridDim.x * 4) {
        const int32_t ab = n2e_ptr[p], deg = n2e_ptr[p + 1] - ab;
        const GatherRow r = GatherRows{rowptr, dofs, full}(p);
        const int32_t rs = r.rs, nbn = r.nb, nslot = r.nslot, step = full ? dofs : 1;
        const int64_t base = (int64_t)ab * NEN;
        if (deg > GATHER_MAX_DEG || deg * NEN > GATHER_MAX_SRC) {
            if (lane == 0) atomicMax(bad, 1);
            continue;
        }
        int running = 0;
        for (int s0 = 0; s0 < nslot; s0 += 64) {
            const int sl = s0 + lane;
            const bool on = sl < nslot;
            const int32_t v = on ? colind[rs + sl * step] / dofs : -1;
            int cnt = 0;
            for (int q = 0; q < deg; ++q) {
                const int32_t* __restrict__ en = conn + (int64_t)(n2e[ab + q] / NEN) * NEN;
#pragma unroll
                for (int j = 0; j < NEN; ++j) cnt += en[j] == v ? 1 : 0;
            }
            int incl = cnt;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            int k = running + incl - cnt;
            if (on) soff[nbn + sl] = (uint16_t)k;
            if (on)
                for (int q = 0; q < deg; ++q) {
                    const int32_t* __restrict__ en = conn + (int64_t)(n2e[ab + q] / NEN) * NEN;
#pragma unroll
                    for (int j = 0; j < NEN; ++j)
                        if (en[j] == v) src[base + k++] = gather_pack(q, j);
                }
            running += __shfl(incl, 63, 64);
        }
    }
}

// one element-matrix entry per source; the sum goes to the slot of every component's row (scalar rows or diagonal blocks)
template <int NEN>
struct P2Sum : GatherBlockSum<NEN, 1> {
    const int32_t* rowptr;
    int dofs;
    double* val;
    __device__ void store(const GatherRow& r, int sl) {
        for (int comp = 0; comp < dofs; ++comp) val[rowptr[r.row + comp] + sl] = this->acc[0];
    }
};

template <int NEN>
__global__ __launch_bounds__(256) void k_p2_gather(const int32_t* __restrict__ n2e_ptr, const int32_t* __restrict__ n2e,
                                                   const int32_t* __restrict__ rowptr, int dofs, int32_t nn,
                                                   const uint16_t* __restrict__ soff, const uint16_t* __restrict__ src,
                                                   const double* __restrict__ ke, double* __restrict__ val) {
    gather_walk<NEN>(n2e_ptr, n2e, soff, src, nn, GatherRows{rowptr, dofs, 0}, P2Sum<NEN>{{ke}, rowptr, dofs, val});
}

// f(std::integral_constant<int, FORM>()) for the matrix form kform (F_LAPLACE, F_MASS or F_LINELAS)
template <class F>
int with_form(int kform, F&& f) {
    if (kform == F_LAPLACE) return f(std::integral_constant<int, F_LAPLACE>());
    if (kform == F_MASS) return f(std::integral_constant<int, F_MASS>());
    return f(std::integral_constant<int, F_LINELAS>());
}

// rows of the P2 scalar forms (scalar or diagonal blocks) from c->d_ke through the gather lists; -1 (no error) where they do not apply
template <int NEN>
int launch_p2_gather(fedd_ctx* c) {
    if (c->block_mode == FEDD_BLOCK_FULL) return -1;
    // the lists of the current mesh, built at the first P2 assembly that uses them: of the node-level pattern, which the scalar
    // and the DIAG patterns of a mesh share (nnz of a scalar pattern; diagonal blocks have dofs rows of that length each)
    GatherLists& gl = c->gl_p2;
    const int64_t nn = c->n_own + c->n_rowg;
    if (gl.state == GatherLists::NOT_BUILT) {
        FEDD_HIP(hipStreamSynchronize(c->stream));
        const auto t0 = std::chrono::steady_clock::now();
        FEDD_TRY(gather_lists_ensure(c, gl, GATHER_NODE_PATTERN, c->d_rowptr.p, c->d_colind.p, c->dofs, 0, nn, c->nnz_ext / c->dofs, nullptr));
        FEDD_HIP(hipStreamSynchronize(c->stream));
        c->tl_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (gl.state != GatherLists::READY) return -1;
    ScopedTimer t(c, FEDD_T_ASSEMBLE);
    hipLaunchKernelGGL(k_p2_gather<NEN>, dim3((unsigned)gather_grid(nn)), dim3(256), 0, c->stream, c->d_n2e_ptr.p, c->d_n2e.p,
                       c->d_rowptr.p, c->dofs, (int32_t)nn, gl.soff.p, gl.src.p, c->d_ke.p, c->d_val.p);
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Stress form of the velocity block, FE::assemblyStress (FE_def.hpp:2407-2733; 2D element loop :2457-2562, 3D :2587-2727):
//   K[(i,a),(j,b)] = |det B| sum_k c_k w_k ( delta_ab grad phi_i . grad phi_j + d_b phi_i d_a phi_j )
// with the transformed gradients (dPhiTrans) and c_k the coefficient at x_k = B xi_k + p_1 (a.coeff, nullptr: 1).
// A node pair (i, j) holds dim^2 distinct sums O[b][a] = sum_k c_k w_k d_b phi_i d_a phi_j; the scalar part is their trace, and
// the block of (j, i) is the transpose of the block of (i, j).  So the element pass, ONE ELEMENT PER WAVEFRONT with the
// reference gradients and weights staged in LDS, evaluates the NEN (NEN + 1) / 2 pairs i <= j only -- 55 lanes of one wave for
// a P2 tetrahedron, dim^2 sums each, in place of the 900 entries of the 30 x 30 element matrix -- and writes
// S_ij[a][b] = |det B| (O[b][a] + delta_ab tr O) as one contiguous stream [pair][a][b]: 8 * n_elem * NEN (NEN + 1) / 2 * dim^2
// bytes of scratch (d_adv_ke; 3960 bytes per P2 tetrahedron, 55 % of a full element matrix).
// The rows are then summed through the gather lists of the system's FULL pattern (full_lists_ensure, shared with the
// hyperelastic tangent; gather_lists.hpp), the element blocks read transposed where the row's local index is the larger one.
// Operation order per pair: k ascending; (c_k w_k) d_b phi_i, times d_a phi_j, accumulated; the trace added; times |det B|.
// ---------------------------------------------------------------------------------------------
template <int DIM, int NEN>
__global__ __launch_bounds__(256) void k_stress_elem(AsmArgs a, int64_t n_elem, double* __restrict__ ke) {
    constexpr int DD = DIM * DIM, NP = NEN * (NEN + 1) / 2;
    extern __shared__ double sm[];
    const int nq = a.nq;
    const int ntab = nq * (1 + NEN * DIM);      // w[nq] | dphi[nq * NEN * DIM]
    const double* s_w = sm;
    const double* s_dphi = sm + nq;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int per_wave = nq * NEN * DIM + nq;
    double* Gs = sm + ntab + (size_t)w * per_wave;      // this wave's transformed gradients [k][i][d]
    double* cw = Gs + nq * NEN * DIM;                   // c_k w_k
    for (int i = tid; i < ntab; i += 256) sm[i] = a.tab[i];
    __syncthreads();
    const int64_t nwave = (int64_t)gridDim.x * 4;
    const int64_t trips = (n_elem + nwave - 1) / nwave;
    for (int64_t k = 0; k < trips; ++k) {
        const int64_t e = k * nwave + (int64_t)blockIdx.x * 4 + w;
        const bool on = e < n_elem;
        double xv = 0.0;
        if (on && lane < (DIM + 1) * DIM) xv = a.xyz[(int64_t)a.conn[e * NEN + lane / DIM] * DIM + (lane % DIM)];
        double X[DIM + 1][DIM];
#pragma unroll
        for (int v = 0; v <= DIM; ++v)
#pragma unroll
            for (int d = 0; d < DIM; ++d) X[v][d] = __shfl(xv, v * DIM + d, 64);
        double Binv[DIM][DIM];
        const double absdet = on ? fabs(affine<DIM>(X, Binv)) : 0.0;
        if (on) {
            for (int t = lane; t < nq * NEN; t += 64) {
                double g[DIM];
                grad_t<DIM, NEN>(s_dphi, t / NEN, t % NEN, Binv, g);
#pragma unroll
                for (int d = 0; d < DIM; ++d) Gs[t * DIM + d] = g[d];
            }
            for (int q = lane; q < nq; q += 64) cw[q] = (a.coeff ? a.coeff[e * nq + q] : 1.0) * s_w[q];
        }
        __syncthreads();
        if (on) {
            double* __restrict__ out = ke + e * (NP * DD);
            for (int t = lane; t < NP; t += 64) {
                int i = 0, rem = t;
                while (rem >= NEN - i) {
                    rem -= NEN - i;
                    ++i;
                }
                const int j = i + rem;
                double O[DIM][DIM];
#pragma unroll
                for (int b = 0; b < DIM; ++b)
#pragma unroll
                    for (int d = 0; d < DIM; ++d) O[b][d] = 0.0;
                for (int q = 0; q < nq; ++q) {
                    const double* gi = Gs + (q * NEN + i) * DIM;
                    const double* gj = Gs + (q * NEN + j) * DIM;
#pragma unroll
                    for (int b = 0; b < DIM; ++b) {
                        const double s = cw[q] * gi[b];
#pragma unroll
                        for (int d = 0; d < DIM; ++d) O[b][d] += s * gj[d];
                    }
                }
                double tr = 0.0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) tr += O[d][d];
#pragma unroll
                for (int r = 0; r < DIM; ++r)
#pragma unroll
                    for (int cc = 0; cc < DIM; ++cc) out[t * DD + r * DIM + cc] = absdet * (O[cc][r] + (r == cc ? tr : 0.0));
            }
        }
        // Gs and cw are rewritten by the next trip.  Both barriers of the loop order one wave's LDS writes against its own lanes'
        // reads only (the buffers are private to the wave), so a wave-level barrier would do; the workgroup barrier is what the
        // other one-element-per-wave kernels of this file use (k_elem_matrix, k_adv_elem), it is legal because `trips` is uniform
        // over the workgroup, and its cost -- four waves in step, each with the same work per trip -- has not been measured apart.
        __syncthreads();
    }
}

// rows of the system's FULL pattern from the packed pair blocks of k_stress_elem: one per source, read transposed where the
// row's local index is the larger one
template <int DIM, int NEN>
struct StressSum : GatherBlockSum<NEN, DIM * DIM> {
    static constexpr int DD = DIM * DIM, NP = NEN * (NEN + 1) / 2;
    double* val;
    __device__ void add(int32_t at, int j) {
        const int32_t el = at / NEN;
        const int i = at - el * NEN;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const double* __restrict__ kb = this->ke + ((int64_t)el * NP + (lo * NEN - lo * (lo - 1) / 2 + (hi - lo))) * DD;
        if (i <= j) {
#pragma unroll
            for (int m = 0; m < DD; ++m) this->acc[m] += kb[m];
        } else {
#pragma unroll
            for (int r = 0; r < DIM; ++r)
#pragma unroll
                for (int cc = 0; cc < DIM; ++cc) this->acc[r * DIM + cc] += kb[cc * DIM + r];
        }
    }
    __device__ void store(const GatherRow& g, int sl) {
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
            const int64_t to = (int64_t)g.rs + (int64_t)r * g.nslot * DIM + (int64_t)sl * DIM;
#pragma unroll
            for (int cc = 0; cc < DIM; ++cc) val[to + cc] = this->acc[r * DIM + cc];
        }
    }
};

template <int DIM, int NEN>
__global__ __launch_bounds__(256) void k_stress_gather(const int32_t* __restrict__ n2e_ptr, const int32_t* __restrict__ n2e,
                                                       const int32_t* __restrict__ rowptr, int32_t nn,
                                                       const uint16_t* __restrict__ soff, const uint16_t* __restrict__ src,
                                                       const double* __restrict__ ke, double* __restrict__ val) {
    gather_walk<NEN>(n2e_ptr, n2e, soff, src, nn, GatherRows{rowptr, DIM, 1}, StressSum<DIM, NEN>{{ke}, val});
}

// a.tab / a.nq: the tables of full_lists_ensure (w | dphi); the lists are c->gl_full
template <int DIM, int NEN>
int launch_stress(fedd_ctx* c, const AsmArgs& a) {
    constexpr int DD = DIM * DIM, NP = NEN * (NEN + 1) / 2;
    const int64_t nn = c->n_own;
    FEDD_TRY(c->d_adv_ke.ensure((size_t)c->n_elem * NP * DD));
    const int ntab = a.nq * (1 + NEN * DIM);
    const int per_wave = a.nq * NEN * DIM + a.nq;
    const size_t lds = ((size_t)ntab + 4 * (size_t)per_wave) * sizeof(double);
    FEDD_CHECK(lds <= 64 * 1024, "fedd_assemble_stress: the quadrature tables of %d points do not fit the LDS", a.nq);
    ScopedTimer t(c, FEDD_T_ASSEMBLE);
    // byte model: connectivity, geometry and c once; the pair blocks written and read once; the values written; the lists read
    t.bytes((double)c->n_elem * (NEN * 4.0 + 2.0 * NP * DD * 8.0 + (a.coeff ? a.nq * 8.0 : 0.0)) + (double)c->n_node * DIM * 8.0 +
            (double)c->nnz * 8.0 + (double)(c->nnz / DD) * 2.0 * 2.0);
    if (c->n_elem > 0) {
        const int64_t nwg = std::min<int64_t>((c->n_elem + 3) / 4, 256 * 8);
        hipLaunchKernelGGL((k_stress_elem<DIM, NEN>), dim3((unsigned)nwg), dim3(256), lds, c->stream, a, c->n_elem, c->d_adv_ke.p);
    }
    hipLaunchKernelGGL((k_stress_gather<DIM, NEN>), dim3((unsigned)gather_grid(nn)), dim3(256), 0, c->stream, c->d_n2e_ptr.p,
                       c->d_n2e.p, c->d_rowptr.p, (int32_t)nn, c->gl_full.soff.p, c->gl_full.src.p, c->d_adv_ke.p, c->d_val.p);
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}

// The scaled vector Laplacian (FEDD_FORM_LAPLACE_XDIM), all four element types on ONE path: the element matrices with the
// element's coefficient (k_elem_matrix<..., SCALED>, one element per wavefront), the rows summed from them through the
// node-level gather lists of k_p2_lists (built once per mesh, kept by a move), each value written to the dim diagonal-block
// slots.  P1 takes this path too, not the tiles: the tile kernel keeps no per-element scalar in its blobs, and one path has
// one summation order to state and to test (DESIGN.md section 4 "Interface distances" has what it costs).
template <int DIM, int NEN>
int launch_laplace_xdim(fedd_ctx* c, AsmArgs a, int ntab) {
    if (c->n_elem == 0 || c->n_own == 0) {
        FEDD_HIP(hipMemsetAsync(c->d_val.p, 0, (size_t)c->nnz_ext * sizeof(double), c->stream));
        return 0;
    }
    {
        ScopedTimer t(c, FEDD_T_ASSEMBLE);
        // byte model on top of the unscaled pass: four distances per element through the connectivity (shared lines), one
        // coefficient written and read per element
        t.bytes((double)c->n_elem * ((DIM + 1) * 4.0 + 16.0) + (double)c->n_node * 8.0);
        FEDD_TRY(laplace_scale(c, a.p0, a.p1));
    }
    a.fscale = c->d_lscale.p;
    FEDD_TRY((launch_elem_matrices<DIM, NEN, F_LAPLACE, true>(c, a, ntab)));
    const double keep_ms = c->tl_build_ms;
    const int rc = launch_p2_gather<NEN>(c);
    if constexpr (NEN == DIM + 1) c->tl_build_ms = keep_ms;     // (on a P1 mesh that figure is the tile build's)
    FEDD_CHECK(rc >= 0, "fedd_assemble(FEDD_FORM_LAPLACE_XDIM): the gather lists do not fit this mesh (a node with more than %d "
                        "incident elements)", GATHER_MAX_SRC / NEN);
    return rc;
}

// The dispatch: the stress form, tiles, then P2 element matrices + gather lists, then launch_matrix.
template <int DIM, int NEN>
int launch_assemble(fedd_ctx* c, int kform, AsmArgs a, int ntab, bool xdim = false) {
    if (kform == F_STRESS) return launch_stress<DIM, NEN>(c, a);
    if (xdim) return launch_laplace_xdim<DIM, NEN>(c, a, ntab);
    if constexpr (NEN == DIM + 1) {
        // element-major tiles for the P1 forms they cover (option "asm_tiles" 0: the pair kernels)
        if (c->asm_kind == 0 && c->asm_tiles && a.nq == 1 && (kform == F_LAPLACE || kform == F_LINELAS)) {
            const int rc = assemble_tiles(c, kform, a, ntab);
            if (rc >= 0) return rc;
        }
    }
    if constexpr (NEN > DIM + 1) {
        // P2: the element matrices once per element (k_elem_matrix), the rows summed from them (option "asm_p2_elem" 0: the pair
        // kernels re-derive the row of every (row, element) pair)
        if (c->asm_p2_elem && (kform == F_LAPLACE || kform == F_MASS)) {
            if (kform == F_LAPLACE) FEDD_TRY((launch_elem_matrices<DIM, NEN, F_LAPLACE>(c, a, ntab)));
            else FEDD_TRY((launch_elem_matrices<DIM, NEN, F_MASS>(c, a, ntab)));
            // rows from the gather lists ("asm_p2_elem" 2: through the pair kernels, which read a.ke)
            if (c->asm_p2_elem == 1) {
                const int rc = launch_p2_gather<NEN>(c);
                if (rc >= 0) return rc;
            }
        }
    }
    return with_form(kform, [&](auto form) {
        return launch_matrix<DIM, NEN, decltype(form)::value>(c, a, ntab, c->n_rows_ext, c->max_row_nnz);
    });
}

// quadrature weights, basis values / gradients of the mesh's element and the P1 (pressure) basis at
// the same points -> d_dtmp0, layout w | phi | dphi | psi
int upload_tables(fedd_ctx* c, int degree, int& nq, int& ntab) {
    const int dim = c->dim, nen = c->nen;
    FeTables tb, tp;
    FEDD_TRY(fe_tables(dim, nen, degree, tb));
    FEDD_TRY(fe_tables(dim, dim + 1, degree, tp));
    nq = tb.nq;
    ntab = nq * (1 + nen + nen * dim + dim + 1);
    std::vector<double> host(ntab);
    std::copy(tb.w.begin(), tb.w.end(), host.begin());
    std::copy(tb.phi.begin(), tb.phi.end(), host.begin() + nq);
    std::copy(tb.dphi.begin(), tb.dphi.end(), host.begin() + nq + nq * nen);
    std::copy(tp.phi.begin(), tp.phi.end(), host.begin() + nq + nq * nen + nq * nen * dim);
    FEDD_TRY(c->d_dtmp0.ensure(std::max<size_t>(ntab, c->d_dtmp0.cap)));
    FEDD_HIP(hipMemcpyAsync(c->d_dtmp0.p, host.data(), ntab * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));  // `host` is a local
    return 0;
}

// B pattern from the scalar node pattern: pressure node i (< n_p) couples to all dim components of
// every velocity node of its elements.
__global__ void k_div_pattern(const int32_t* __restrict__ nptr, const int32_t* __restrict__ ncol, int32_t n_p, int dim,
                              int32_t* __restrict__ rowptr, int32_t* __restrict__ colind) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_p) return;
    rowptr[i] = nptr[i] * dim;
    if (i == n_p) return;
    const int32_t b = nptr[i], nn = nptr[i + 1] - b;
    for (int32_t s = 0; s < nn; ++s)
        for (int d = 0; d < dim; ++d) colind[(b + s) * dim + d] = ncol[b + s] * dim + d;
}

// B^T: velocity node j couples to the vertices (< n_p) of its elements
__global__ void k_divt_count(const int32_t* __restrict__ nptr, const int32_t* __restrict__ ncol, int32_t n_v, int32_t n_p,
                             int32_t* __restrict__ cnt) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_v) return;
    int32_t k = 0;
    for (int32_t p = nptr[j]; p < nptr[j + 1]; ++p) k += ncol[p] < n_p ? 1 : 0;
    cnt[j] = k;
}

__global__ void k_divt_fill(const int32_t* __restrict__ nptr, const int32_t* __restrict__ ncol, int32_t n_v, int32_t n_p,
                            int dim, const int32_t* __restrict__ cptr, int32_t* __restrict__ rowptr,
                            int32_t* __restrict__ colind) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_v) return;
    if (j == n_v) {
        rowptr[(int64_t)n_v * dim] = cptr[n_v] * dim;
        return;
    }
    const int32_t nn = cptr[j + 1] - cptr[j];
    for (int d = 0; d < dim; ++d) {
        const int32_t start = cptr[j] * dim + d * nn;
        rowptr[(int64_t)j * dim + d] = start;
        int32_t k = 0;
        for (int32_t p = nptr[j]; p < nptr[j + 1]; ++p)
            if (ncol[p] < n_p) colind[start + k++] = ncol[p];
    }
}

}  // namespace

// FE::assemblyDivAndDivT (feddlib/core/FE/FE_def.hpp:1932-2057) for velocity = the mesh's element
// (P2 or P1) and pressure = P1 on the vertices; the P1 nodes are the first n_p node ids (that is how
// the P2 mesh is built from the P1 mesh).  Unscaled; Stokes::assemble applies the -1 afterwards.
// Uses (and overwrites) the system slot for the scalar node pattern, so blocks that must survive
// have to be stored first.
int assemble_div(fedd_ctx* c, int64_t n_p, int slot_b, int slot_bt) {
    FEDD_CHECK(c->nranks == 1, "assemblyDivAndDivT: one rank only for now");
    FEDD_CHECK(n_p > 0 && n_p <= c->n_own, "assemblyDivAndDivT: %lld pressure nodes of %lld nodes", (long long)n_p, (long long)c->n_own);
    const int dim = c->dim, nen = c->nen;
    const int32_t n_v = (int32_t)c->n_own;
    if (!c->have_adj) FEDD_TRY(build_adjacency(c));
    FEDD_TRY(build_pattern(c, 1, FEDD_BLOCK_SCALAR));  // scalar node pattern -> system slot
    // ... which is scratch, not a system matrix, nor a pattern to repeat.  The one writer that records twice: build_pattern
    // has recorded its own write, and what it set at its end (have_pattern, pat_repeatable) is taken back here, before
    // anything can read it
    system_written(c, SYS_VALUES | SYS_PATTERN | SYS_GONE);
    const int32_t* nptr = c->d_rowptr.p;
    const int32_t* ncol = c->d_colind.p;
    const int node_rowcap = c->max_row_nnz;
    DevCsr& B = c->aux[slot_b];
    DevCsr& BT = c->aux[slot_bt];
    // ---- patterns ----
    int32_t h_np = 0;
    FEDD_HIP(hipMemcpyAsync(&h_np, nptr + n_p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    B.n_rows = n_p; B.n_cols = (int64_t)n_v * dim; B.nnz = (int64_t)h_np * dim; B.max_row_nnz = node_rowcap * dim;
    FEDD_TRY(B.rowptr.ensure((size_t)n_p + 1));
    FEDD_TRY(B.colind.ensure((size_t)B.nnz));
    FEDD_TRY(B.val.ensure((size_t)B.nnz));
    const dim3 blk(256);
    hipLaunchKernelGGL(k_div_pattern, dim3((unsigned)((n_p + 1 + 255) / 256)), blk, 0, c->stream, nptr, ncol, (int32_t)n_p, dim,
                       B.rowptr.p, B.colind.p);
    FEDD_TRY(c->d_itmp1.ensure(std::max<size_t>((size_t)n_v + 1, c->d_itmp1.cap)));
    int32_t* cptr = c->d_itmp1.p;
    hipLaunchKernelGGL(k_divt_count, dim3((unsigned)((n_v + 255) / 256)), blk, 0, c->stream, nptr, ncol, n_v, (int32_t)n_p, cptr);
    int32_t mx = 0;
    FEDD_TRY(reduce_max_i32(c, cptr, n_v, &mx));
    int64_t tot = 0;
    FEDD_TRY(exclusive_scan_i32(c, cptr, cptr, n_v, &tot));
    BT.n_rows = (int64_t)n_v * dim; BT.n_cols = n_p; BT.nnz = tot * dim; BT.max_row_nnz = mx;
    FEDD_TRY(BT.rowptr.ensure((size_t)BT.n_rows + 1));
    FEDD_TRY(BT.colind.ensure((size_t)BT.nnz));
    FEDD_TRY(BT.val.ensure((size_t)BT.nnz));
    hipLaunchKernelGGL(k_divt_fill, dim3((unsigned)((n_v + 1 + 255) / 256)), blk, 0, c->stream, nptr, ncol, n_v, (int32_t)n_p, dim,
                       (const int32_t*)cptr, BT.rowptr.p, BT.colind.p);
    FEDD_HIP(hipGetLastError());
    // ---- values: determineDegree(dim, FE1, FE2, Grad, Std) (FE_def.hpp:1962) ----
    int degree = fe_degree(nen, dim, true) + 1;
    if (degree == 0) degree = 1;
    int nq = 0, ntab = 0;
    FEDD_TRY(upload_tables(c, degree, nq, ntab));
    AsmArgs a;
    a.conn = c->d_conn.p; a.n2e_ptr = c->d_n2e_ptr.p; a.n2e = c->d_n2e.p; a.xyz = c->d_xyz.p; a.tab = c->d_dtmp0.p;
    a.nq = nq; a.p0 = a.p1 = 0.0;
    a.ke = nullptr;
    a.zero_eps = c->asm_zero_eps;       // doSetZeros: B and B^T threshold their element contributions (FE_def.hpp:2002-2004, 2032-2034)
    AsmArgs ab = a, at = a;
    ab.rowptr = B.rowptr.p; ab.colind = B.colind.p; ab.val = B.val.p; ab.n_rows = (int32_t)n_p; ab.dofs = 1;
    at.rowptr = BT.rowptr.p; at.colind = BT.colind.p; at.val = BT.val.p; at.n_rows = (int32_t)BT.n_rows; at.dofs = dim;
    FEDD_TRY(with_element(dim, nen, [&](auto d, auto n) {
        constexpr int D = decltype(d)::value, N = decltype(n)::value;
        FEDD_TRY((launch_matrix<D, N, F_DIV>(c, ab, ntab, n_p, B.max_row_nnz)));
        return launch_matrix<D, N, F_DIVT>(c, at, ntab, BT.n_rows, BT.max_row_nnz);
    }));
    B.valid = BT.valid = true;
    B.pattern_id = ++c->pattern_counter;
    BT.pattern_id = ++c->pattern_counter;
    B.value_id = ++c->value_counter;
    BT.value_id = ++c->value_counter;
    B.block_mode = BT.block_mode = -1;
    return 0;
}

namespace {

// ---------------------------------------------------------------------------------------------
// Advection matrices of Navier-Stokes for a velocity u given at the nodes (d_vel, dim * node + d):
//   N(u)  FE::assemblyAdvectionVecField     FE_def.hpp:1759-1832   n_ij = |det B| sum_q w_q (u_h . grad phi_j) phi_i, on the dim
//                                                                   diagonal component pairs (dim * i + d, dim * j + d)
//   W(u)  FE::assemblyAdvectionInUVecField  FE_def.hpp:1839-1925   (dim * i + d1, dim * j + d2) = |det B| sum_q w_q (d u_d1 / d x_d2) phi_i phi_j
// Element-major like the P2 scalar forms, ONE ELEMENT PER WAVEFRONT: the reference tables of both rules are staged in LDS once per
// workgroup; a wave loads its element's vertices and its NEN x dim velocity values once, its lanes evaluate u_h (as the weighted
// reference-space vector w_q B^-1 u_h) and w_q grad u_h at the quadrature points into LDS, and then take the NEN^2 node pairs:
// n_ij and the dim x dim block of W are summed in registers and leave as one contiguous stream, [i][j][dim x dim] (N alone:
// [i][j]).  ADV_NEWTON adds n_ij to the diagonal of the block, so N + W costs one pass over the geometry and u.
// The rows are then summed by gather lists on the node-level pattern (gather_lists.hpp; built once per mesh) and written as
// scale * block + M[slot_add] into the FULL pattern, whose positions follow from the node-level pattern in closed form.
//
// ALE convection on a moved mesh (fedd_assemble_advection_ale; template parameter ALE, 0 = the fixed-mesh kinds above, whose
// code it leaves untouched) for a mesh velocity w given at the nodes (d_mvel):
//   P(w)  FE::assemblyAdditionalConvection  FE_def.hpp:3044-3255   p_ij = |det B| sum_q w_q (div w_h)(x_q) phi_i phi_j on the dim
//                                                                   diagonal component pairs, rule of W (below)
// ALE_FUSED: the wave stages u, w and c = u - w (one subtraction per nodal value); beta is formed from c, grad u_h from u, and
// its lanes add pw_q = w_q (div w_h)(x_q) per quadrature point next to beta:  for d: g_r = sum_i w[i][d] dphi_i,r (i ascending),
// div += g_r Binv[r][d] (r ascending); pw_q = w_q * div.  Pair (i, j): p = |det B| * sum_q (phi_i phi_j) pw_q (q ascending), taken
// from n_ij AFTER the setZeros threshold of n_ij (and of the W block): FIXEDPOINT writes n_ij - p_ij, NEWTON adds n_ij - p_ij to the
// diagonal of the thresholded W block.  ALE_P_ONLY writes p_ij alone and reads no u.  With w = 0 every p is a zero and c = u, so
// the fused kinds return the bits of the fixed-mesh kinds.
// ---------------------------------------------------------------------------------------------
enum { ALE_NONE = 0, ALE_FUSED = 1, ALE_P_ONLY = 2 };

struct AdvArgs {
    const int32_t* conn;
    const double* xyz;
    const double* u;
    const double* w;        // mesh velocity at the nodes (ALE kinds only)
    const double* tab;      // w | phi | dphi of the rule of N; the same of the rule of W at off_w (0: one rule for both)
    int nq_n, nq_w, off_w;
    double zero_eps;        // setZeros_ / myeps_ (FE_def.hpp:1816, 1908): element values of N and of W below it are set to zero
};

// LDS doubles of one wave: u, beta, grad u_h; the ALE kinds add w, u - w and pw
template <int DIM, int NEN, int ALE>
__host__ __device__ constexpr int adv_per_wave(int nqn, int nqw) {
    return NEN * DIM + nqn * DIM + nqw * DIM * DIM + (ALE != ALE_NONE ? 2 * NEN * DIM + nqw : 0);
}

template <int DIM, int NEN, int KIND, int ALE = ALE_NONE>
__global__ __launch_bounds__(256) void k_adv_elem(AdvArgs a, int64_t n_elem, double* __restrict__ ke) {
    static_assert(ALE != ALE_P_ONLY || KIND == FEDD_ADV_N, "P alone leaves as one value per node pair");
    static_assert(ALE == ALE_NONE || KIND != FEDD_ADV_W, "no ALE form of W alone");
    constexpr int BLK = KIND == FEDD_ADV_N ? 1 : DIM * DIM;
    extern __shared__ double sm[];
    const int nqn = a.nq_n, nqw = a.nq_w;
    const int ntab = a.off_w + nqw * (1 + NEN + NEN * DIM);
    const double* wn = sm;
    const double* phin = wn + nqn;
    const double* dphin = phin + nqn * NEN;
    const double* ww = sm + a.off_w;
    const double* phiw = ww + nqw;
    const double* dphiw = phiw + nqw * NEN;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int per_wave = adv_per_wave<DIM, NEN, ALE>(nqn, nqw);
    double* Us = sm + ntab + (size_t)w * per_wave;      // this wave's velocity values [i][d]
    double* beta = Us + NEN * DIM;                      // w_q B^-1 u_h(x_q) [q][r]
    double* wG = beta + nqn * DIM;                      // w_q (d u_d1 / d x_d2)(x_q) [q][d1][d2]
    double* Ws = wG + nqw * DIM * DIM;                  // ALE: mesh velocity values [i][d]
    double* Cs = Ws + NEN * DIM;                        // ALE: u - w [i][d], what convects
    double* pw = Cs + NEN * DIM;                        // ALE: w_q (div w_h)(x_q) [q]
    const double* Ub = ALE == ALE_FUSED ? Cs : Us;      // the field behind beta
    for (int i = tid; i < ntab; i += 256) sm[i] = a.tab[i];
    const int64_t nwave = (int64_t)gridDim.x * 4;
    const int64_t trips = (n_elem + nwave - 1) / nwave;
    for (int64_t k = 0; k < trips; ++k) {
        const int64_t e = k * nwave + (int64_t)blockIdx.x * 4 + w;
        const bool on = e < n_elem;
        double xv = 0.0;
        if (on && lane < (DIM + 1) * DIM) xv = a.xyz[(int64_t)a.conn[e * NEN + lane / DIM] * DIM + (lane % DIM)];
        if constexpr (ALE == ALE_NONE) {
            if (on && lane < NEN * DIM) Us[lane] = a.u[(int64_t)a.conn[e * NEN + lane / DIM] * DIM + (lane % DIM)];
        } else {
            if (on && lane < NEN * DIM) {
                const int64_t at = (int64_t)a.conn[e * NEN + lane / DIM] * DIM + (lane % DIM);
                const double wv = a.w[at];
                Ws[lane] = wv;
                if constexpr (ALE == ALE_FUSED) {
                    const double uv = a.u[at];
                    Us[lane] = uv;
                    Cs[lane] = uv - wv;
                }
            }
        }
        double X[DIM + 1][DIM];
#pragma unroll
        for (int v = 0; v <= DIM; ++v)
#pragma unroll
            for (int d = 0; d < DIM; ++d) X[v][d] = __shfl(xv, v * DIM + d, 64);
        double Binv[DIM][DIM];
        const double absdet = on ? fabs(affine<DIM>(X, Binv)) : 0.0;
        __syncthreads();        // tables (first trip) and Us
        if (on) {
            if constexpr (KIND != FEDD_ADV_W && ALE != ALE_P_ONLY) {
                for (int q = lane; q < nqn; q += 64) {
                    double uq[DIM];
#pragma unroll
                    for (int d = 0; d < DIM; ++d) uq[d] = 0.0;
                    for (int i = 0; i < NEN; ++i)
#pragma unroll
                        for (int d = 0; d < DIM; ++d) uq[d] += Ub[i * DIM + d] * phin[q * NEN + i];
#pragma unroll
                    for (int r = 0; r < DIM; ++r) {
                        double s = 0.0;
#pragma unroll
                        for (int d = 0; d < DIM; ++d) s += Binv[r][d] * uq[d];
                        beta[q * DIM + r] = wn[q] * s;
                    }
                }
            }
            if constexpr (KIND != FEDD_ADV_N) {
                for (int t = lane; t < nqw * DIM; t += 64) {
                    const int q = t / DIM, d1 = t - q * DIM;
                    double gr[DIM];
#pragma unroll
                    for (int r = 0; r < DIM; ++r) gr[r] = 0.0;
                    for (int i = 0; i < NEN; ++i)
#pragma unroll
                        for (int r = 0; r < DIM; ++r) gr[r] += Us[i * DIM + d1] * dphiw[(q * NEN + i) * DIM + r];
#pragma unroll
                    for (int d2 = 0; d2 < DIM; ++d2) {
                        double s = 0.0;
#pragma unroll
                        for (int r = 0; r < DIM; ++r) s += gr[r] * Binv[r][d2];
                        wG[t * DIM + d2] = ww[q] * s;
                    }
                }
            }
            if constexpr (ALE != ALE_NONE) {
                for (int q = lane; q < nqw; q += 64) {
                    double dv = 0.0;
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        double gr[DIM];
#pragma unroll
                        for (int r = 0; r < DIM; ++r) gr[r] = 0.0;
                        for (int i = 0; i < NEN; ++i)
#pragma unroll
                            for (int r = 0; r < DIM; ++r) gr[r] += Ws[i * DIM + d] * dphiw[(q * NEN + i) * DIM + r];
#pragma unroll
                        for (int r = 0; r < DIM; ++r) dv += gr[r] * Binv[r][d];
                    }
                    pw[q] = ww[q] * dv;
                }
            }
        }
        __syncthreads();
        if (on) {
            double* __restrict__ out = ke + e * (NEN * NEN * BLK);
            for (int t = lane; t < NEN * NEN; t += 64) {
                const int i = t / NEN, j = t - i * NEN;
                double n = 0.0;
                if constexpr (KIND != FEDD_ADV_W && ALE != ALE_P_ONLY) {
                    for (int q = 0; q < nqn; ++q) {
                        const double* dp = dphin + (q * NEN + j) * DIM;
                        double cq = 0.0;
#pragma unroll
                        for (int r = 0; r < DIM; ++r) cq += dp[r] * beta[q * DIM + r];
                        n += cq * phin[q * NEN + i];
                    }
                    n *= absdet;
                    n = (a.zero_eps > 0.0 && fabs(n) < a.zero_eps) ? 0.0 : n;
                }
                if constexpr (ALE != ALE_NONE) {        // after the threshold of n
                    double p = 0.0;
                    for (int q = 0; q < nqw; ++q) p += (phiw[q * NEN + i] * phiw[q * NEN + j]) * pw[q];
                    p *= absdet;
                    n = ALE == ALE_P_ONLY ? p : n - p;
                }
                if constexpr (KIND == FEDD_ADV_N) {
                    out[t] = n;
                } else {
                    double blk[BLK];
#pragma unroll
                    for (int m = 0; m < BLK; ++m) blk[m] = 0.0;
                    for (int q = 0; q < nqw; ++q) {
                        const double pp = phiw[q * NEN + i] * phiw[q * NEN + j];
#pragma unroll
                        for (int m = 0; m < BLK; ++m) blk[m] += pp * wG[q * BLK + m];
                    }
#pragma unroll
                    for (int m = 0; m < BLK; ++m) {
                        double v = blk[m] * absdet;
                        v = (a.zero_eps > 0.0 && fabs(v) < a.zero_eps) ? 0.0 : v;
                        if (KIND == FEDD_ADV_NEWTON && m / DIM == m % DIM) v += n;
                        out[t * BLK + m] = v;
                    }
                }
            }
        }
        __syncthreads();        // Us, beta, wG (and Ws, Cs, pw of the ALE kinds) are rewritten by the next trip
    }
}

// one BLK block per source (BLK 1: a scalar for the diagonal of the block); val = scale * sum + M[slot_add] (add_full: M has the
// FULL pattern, else DIAG), under the compiler's default contraction
template <int DIM, int NEN, int BLK>
struct AdvSum : GatherBlockSum<NEN, BLK> {
    double scale;
    const double* addval;
    int add_full;
    double* val;
    __device__ void store(const GatherRow& g, int sl) {
        const int32_t nb = g.nb, nslot = g.nslot;
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
            const int64_t rs = (int64_t)nb * DIM * DIM + (int64_t)r * nslot * DIM + (int64_t)sl * DIM;
#pragma unroll
            for (int cc = 0; cc < DIM; ++cc) {
                double v = scale * (BLK == 1 ? (r == cc ? this->acc[0] : 0.0) : this->acc[(r * DIM + cc) % BLK]);
                if (addval) {
                    if (add_full) v += addval[rs + cc];
                    else if (r == cc) v += addval[(int64_t)nb * DIM + (int64_t)r * nslot + sl];
                }
                val[rs + cc] = v;
            }
        }
    }
};

template <int DIM, int NEN, int BLK>
__global__ __launch_bounds__(256) void k_adv_gather(const int32_t* __restrict__ n2e_ptr, const int32_t* __restrict__ n2e,
                                                    const int32_t* __restrict__ nptr, int32_t nn, const uint16_t* __restrict__ soff,
                                                    const uint16_t* __restrict__ src, const double* __restrict__ ke, double scale,
                                                    const double* __restrict__ addval, int add_full, double* __restrict__ val) {
    gather_walk<NEN>(n2e_ptr, n2e, soff, src, nn, GatherRows{nptr, 1, 0}, AdvSum<DIM, NEN, BLK>{{ke}, scale, addval, add_full, val});
}

// the per-mesh structures: node-level pattern, gather lists, quadrature tables (determineDegree, FE_def.hpp:1770-1772, 1859-1861:
// P2 5 / 5; P1 2 / 3, remapped by fe_quadrature)
int adv_setup(fedd_ctx* c) {
    const int dim = c->dim, nen = c->nen;
    {
        ScopedTimer t(c, FEDD_T_SYMBOLIC);
        int32_t mx = 0;
        FEDD_TRY(build_node_pattern(c, c->d_adv_nptr, c->d_adv_ncol, &mx, &c->adv_node_nnz));
        c->adv_max_nn = mx;
        FEDD_CHECK(c->adv_node_nnz * dim * dim < ((int64_t)1 << 31), "advection: %lld nonzeros exceed 32-bit local offsets",
                   (long long)(c->adv_node_nnz * dim * dim));
        FEDD_TRY(gather_lists_ensure(c, c->gl_adv, GATHER_NODE_PATTERN, c->d_adv_nptr.p, c->d_adv_ncol.p, 1, 0, c->n_own, c->adv_node_nnz,
                                     "advection"));
    }
    c->gl_adv.reset();      // ready when the tables are
    const bool p2 = nen > dim + 1;
    const int deg_n = p2 ? 5 : 2, deg_w = p2 ? 5 : 3;
    FeTables tn, tw;
    FEDD_TRY(fe_tables(dim, nen, deg_n, tn));
    FEDD_TRY(fe_tables(dim, nen, deg_w, tw));
    const bool same = tn.nq == tw.nq && tn.w == tw.w && tn.phi == tw.phi;
    std::vector<double> host;
    auto put = [&](const FeTables& t) {
        host.insert(host.end(), t.w.begin(), t.w.end());
        host.insert(host.end(), t.phi.begin(), t.phi.end());
        host.insert(host.end(), t.dphi.begin(), t.dphi.end());
    };
    put(tn);
    c->adv_tab_off_w = same ? 0 : (int)host.size();
    if (!same) put(tw);
    c->adv_nq[0] = tn.nq;
    c->adv_nq[1] = tw.nq;
    FEDD_TRY(c->d_adv_tab.ensure(host.size()));
    FEDD_HIP(hipMemcpyAsync(c->d_adv_tab.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));  // `host` is a local
    c->gl_adv.state = GatherLists::READY;
    return 0;
}

template <int DIM, int NEN, int KIND, int ALE = ALE_NONE>
int launch_advection(fedd_ctx* c, double scale, const DevCsr* add, DevCsr& out) {
    constexpr int BLK = KIND == FEDD_ADV_N ? 1 : DIM * DIM;
    FEDD_TRY(c->d_adv_ke.ensure((size_t)c->n_elem * NEN * NEN * BLK));
    AdvArgs a;
    a.conn = c->d_conn.p; a.xyz = c->d_xyz.p; a.u = c->d_vel.p; a.w = c->d_mvel.p; a.tab = c->d_adv_tab.p;
    a.nq_n = c->adv_nq[0]; a.nq_w = c->adv_nq[1]; a.off_w = c->adv_tab_off_w;
    a.zero_eps = c->asm_zero_eps;
    const int ntab = a.off_w + a.nq_w * (1 + NEN + NEN * DIM);
    const int per_wave = adv_per_wave<DIM, NEN, ALE>(a.nq_n, a.nq_w);
    const size_t lds = ((size_t)ntab + 4 * (size_t)per_wave) * sizeof(double);
    FEDD_CHECK(lds <= 64 * 1024, "advection: the quadrature tables do not fit the LDS");
    const int64_t nn = c->n_own;
    ScopedTimer t(c, FEDD_T_ASSEMBLE);
    if (c->n_elem > 0) {
        const int64_t nwg = std::min<int64_t>((c->n_elem + 3) / 4, 256 * 8);
        hipLaunchKernelGGL((k_adv_elem<DIM, NEN, KIND, ALE>), dim3((unsigned)nwg), dim3(256), lds, c->stream, a, c->n_elem, c->d_adv_ke.p);
    }
    const int add_full = add && add->block_mode == FEDD_BLOCK_FULL ? 1 : 0;
    hipLaunchKernelGGL((k_adv_gather<DIM, NEN, BLK>), dim3((unsigned)gather_grid(nn)), dim3(256), 0, c->stream, c->d_n2e_ptr.p,
                       c->d_n2e.p, c->d_adv_nptr.p, (int32_t)nn, c->gl_adv.soff.p, c->gl_adv.src.p, c->d_adv_ke.p, scale,
                       add ? (const double*)add->val.p : nullptr, add_full, out.val.p);
    // byte model: geometry, u and connectivity once per element, the element blocks written and read once, the FULL values written;
    // the fused ALE kinds read one more nodal field, w (P alone reads w in the place of u)
    t.bytes(((double)c->n_elem * (NEN * 4.0 + 2.0 * NEN * NEN * BLK * 8.0) + (double)c->n_node * DIM * (ALE == ALE_FUSED ? 24.0 : 16.0) +
             (double)c->adv_node_nnz * (DIM * DIM * 8.0 + (add ? (add_full ? DIM * DIM : DIM) * 8.0 : 0.0))));
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}

template <int DIM, int NEN>
int advection_kind(fedd_ctx* c, int kind, double scale, const DevCsr* add, DevCsr& out) {
    if (kind == FEDD_ADV_N) return launch_advection<DIM, NEN, FEDD_ADV_N>(c, scale, add, out);
    if (kind == FEDD_ADV_W) return launch_advection<DIM, NEN, FEDD_ADV_W>(c, scale, add, out);
    return launch_advection<DIM, NEN, FEDD_ADV_NEWTON>(c, scale, add, out);
}

template <int DIM, int NEN>
int advection_ale_kind(fedd_ctx* c, int kind, double scale, const DevCsr* add, DevCsr& out) {
    if (kind == FEDD_ALE_P) return launch_advection<DIM, NEN, FEDD_ADV_N, ALE_P_ONLY>(c, scale, add, out);
    if (kind == FEDD_ALE_FIXEDPOINT) return launch_advection<DIM, NEN, FEDD_ADV_N, ALE_FUSED>(c, scale, add, out);
    return launch_advection<DIM, NEN, FEDD_ADV_NEWTON, ALE_FUSED>(c, scale, add, out);
}

// w_i = (a_i - b_i) * rdt: one subtraction, one multiplication by the reciprocal the host formed (FSI_def.hpp:460-462)
__global__ __launch_bounds__(256) void k_mesh_velocity_diff(const double* __restrict__ d_new, const double* __restrict__ d_old,
                                                            int64_t n, double rdt, double* __restrict__ w) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        w[i] = (d_new[i] - d_old[i]) * rdt;
}

}  // namespace

int gather_lists_ensure(fedd_ctx* c, GatherLists& gl, uint64_t pattern, const int32_t* rowptr, const int32_t* colind, int dofs,
                        int full, int64_t nn, int64_t node_nnz, const char* who) {
    if (!gl.ready_for(c->mesh_id, pattern)) {
        gl.mesh_id = c->mesh_id;
        gl.pattern = pattern;
        gl.state = GatherLists::NO_FIT;
        if (!who && (!c->have_pattern || !c->have_adj || nn <= 0)) return 0;
        int32_t n2e_total = 0, h_bad = 0;
        FEDD_HIP(hipMemcpyAsync(&n2e_total, c->d_n2e_ptr.p + nn, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        FEDD_HIP(hipStreamSynchronize(c->stream));
        FEDD_TRY(gl.soff.ensure((size_t)node_nnz + 2));
        FEDD_TRY(gl.src.ensure((size_t)n2e_total * c->nen + 2));
        FEDD_TRY(c->d_flags.ensure(16));
        int32_t* bad = c->d_flags.p + 6;
        FEDD_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), c->stream));
        with_nen(c->nen, [&](auto nen) {
            hipLaunchKernelGGL(k_p2_lists<decltype(nen)::value>, dim3((unsigned)gather_grid(nn)), dim3(256), 0, c->stream,
                               (const int32_t*)c->d_conn.p, (const int32_t*)c->d_n2e_ptr.p, (const int32_t*)c->d_n2e.p, rowptr, colind,
                               dofs, full, (int32_t)nn, gl.soff.p, gl.src.p, bad);
            return 0;
        });
        FEDD_HIP(hipMemcpyAsync(&h_bad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        FEDD_HIP(hipStreamSynchronize(c->stream));
        FEDD_HIP(hipGetLastError());
        if (!h_bad) gl.state = GatherLists::READY;
    }
    FEDD_CHECK(gl.state == GatherLists::READY || !who, "%s: a node with more than %d incident elements does not fit the gather lists",
               who, GATHER_MAX_DEG);
    return 0;
}

// The gather lists of the system's FULL pattern and the tables w | dphi of the rule determineDegree(dim, FEType, FEType, Grad,
// Grad) (P1 0 + 0 -> 1, FE_def.hpp:5508-5509; P2 1 + 1), built once per (mesh, pattern) and kept: one copy for the hyperelastic
// tangent and the stress form, which sum their element blocks into the same rows from the same rule.
int full_lists_ensure(fedd_ctx* c, const char* who) {
    if (c->gl_full.ready_for(c->mesh_id, c->pattern_gen)) return 0;
    const int dim = c->dim, nen = c->nen;
    ScopedTimer t(c, FEDD_T_SYMBOLIC);
    FEDD_TRY(gather_lists_ensure(c, c->gl_full, c->pattern_gen, c->d_rowptr.p, c->d_colind.p, dim, 1, c->n_own, c->nnz / (dim * dim), who));
    t.stop();
    c->gl_full.reset();     // ready when the tables are
    int degree = 2 * fe_degree(nen, dim, true);
    if (degree == 0) degree = 1;
    FeTables tb;
    FEDD_TRY(fe_tables(dim, nen, degree, tb));
    std::vector<double> host(tb.w);
    host.insert(host.end(), tb.dphi.begin(), tb.dphi.end());
    FEDD_TRY(c->d_hy_tab.ensure(host.size()));
    FEDD_HIP(hipMemcpyAsync(c->d_hy_tab.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));  // `host` is a local
    c->hy_nq = tb.nq;
    c->gl_full.state = GatherLists::READY;
    return 0;
}

// a nodal vector field on the repeated map, brought to the column-local numbering of the mesh
static void field_to_columns(const fedd_ctx* c, const double* rep, std::vector<double>& col) {
    const int dim = c->dim;
    const size_t n_rep = c->h_col_of_rep.size();
    col.assign((size_t)c->n_node * dim, 0.0);
    for (size_t i = 0; i < n_rep; ++i)
        for (int d = 0; d < dim; ++d) col[(size_t)c->h_col_of_rep[i] * dim + d] = rep[i * dim + d];
}

// what NavierStokes::u_rep_ holds (NavierStokes_def.hpp:282-321), brought to the column-local numbering of the mesh
int velocity_set(fedd_ctx* c, const double* u_rep) {
    FEDD_CHECK(c->nranks == 1, "fedd_velocity_set: one rank only for now");
    std::vector<double> u;
    field_to_columns(c, u_rep, u);
    FEDD_TRY(c->d_vel.ensure(u.size()));
    FEDD_HIP(hipMemcpyAsync(c->d_vel.p, u.data(), u.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));  // `u` is a local
    c->have_vel = true;
    return 0;
}

// what FSI::w_rep_ holds (FSI_def.hpp:445-464), in a buffer of its own beside d_vel; NULL clears
int mesh_velocity_set(fedd_ctx* c, const double* w_rep) {
    FEDD_CHECK(c->nranks == 1, "fedd_mesh_velocity_set: one rank only (a context with %d ranks was given)", c->nranks);
    if (!w_rep) {
        c->have_mvel = false;
        return 0;
    }
    std::vector<double> w;
    field_to_columns(c, w_rep, w);
    FEDD_TRY(c->d_mvel.ensure(w.size()));
    FEDD_HIP(hipMemcpyAsync(c->d_mvel.p, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));  // `w` is a local
    c->have_mvel = true;
    return 0;
}

// w = (d_new - d_old) * (1.0 / dt): w_rep_->update(-1, old, 1); w_rep_->scale(1.0 / dt) (FSI_def.hpp:460-462), the arithmetic on
// the device.  Around it the host permutes both arrays to the column-local numbering and copies them up (pageable, one
// synchronise), like fedd_velocity_set: a call made once per time step, whose cost is that host side, not the kernel.
int mesh_velocity_diff(fedd_ctx* c, const double* d_new_rep, const double* d_old_rep, double dt) {
    FEDD_CHECK(c->nranks == 1, "fedd_mesh_velocity_diff: one rank only (a context with %d ranks was given)", c->nranks);
    const double rdt = 1.0 / dt;
    std::vector<double> both, old;
    field_to_columns(c, d_new_rep, both);
    field_to_columns(c, d_old_rep, old);
    const size_t n = both.size();
    both.insert(both.end(), old.begin(), old.end());
    FEDD_TRY(c->d_mvel.ensure(n));
    FEDD_TRY(c->d_dtmp0.ensure(2 * n));
    FEDD_HIP(hipMemcpyAsync(c->d_dtmp0.p, both.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (n > 0) {
        const int nwg = (int)std::min<int64_t>(((int64_t)n + 255) / 256, 256 * 8);
        hipLaunchKernelGGL(k_mesh_velocity_diff, dim3((unsigned)nwg), dim3(256), 0, c->stream, (const double*)c->d_dtmp0.p,
                           (const double*)(c->d_dtmp0.p + n), (int64_t)n, rdt, c->d_mvel.p);
    }
    FEDD_HIP(hipStreamSynchronize(c->stream));  // `both` is a local
    FEDD_HIP(hipGetLastError());
    c->have_mvel = true;
    return 0;
}

int mesh_velocity_get(fedd_ctx* c, double* w_rep) {
    FEDD_CHECK(c->nranks == 1, "fedd_mesh_velocity_get: one rank only (a context with %d ranks was given)", c->nranks);
    FEDD_CHECK(c->have_mvel, "fedd_mesh_velocity_get: no mesh velocity (fedd_mesh_velocity_set or fedd_mesh_velocity_diff first)");
    const int dim = c->dim;
    std::vector<double> w((size_t)c->n_node * dim);
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_HIP(hipMemcpy(w.data(), c->d_mvel.p, w.size() * sizeof(double), hipMemcpyDeviceToHost));
    const size_t n_rep = c->h_col_of_rep.size();
    for (size_t i = 0; i < n_rep; ++i)
        for (int d = 0; d < dim; ++d) w_rep[i * dim + d] = w[(size_t)c->h_col_of_rep[i] * dim + d];
    return 0;
}

// aux[slot_out] <- scale * E + aux[slot_add] on the FULL velocity pattern; ale = false: E = (N | W | N + W)(u), kind a
// fedd_advection; ale = true: E = (P(w) | N(u - w) - P(w) | N(u - w) + W(u) - P(w)), kind a fedd_advection_ale.  The one writer
// of these slots: structures, slot rules and the record of the write (value_id) are the same for both entries.
static int advection_into_slot(fedd_ctx* c, const char* who, bool ale, int kind, double scale, int slot_add, int slot_out) {
    const int dim = c->dim, nen = c->nen;
    if (!c->have_adj) {
        ScopedTimer t(c, FEDD_T_SYMBOLIC);
        FEDD_TRY(build_adjacency(c));
    }
    if (c->gl_adv.state != GatherLists::READY) FEDD_TRY(adv_setup(c));
    const int64_t n_rows = c->n_own * dim, nnz = c->adv_node_nnz * dim * dim;
    const DevCsr* add = slot_add >= 0 ? &c->aux[slot_add] : nullptr;
    if (add) {
        FEDD_CHECK(add->valid, "%s: slot %d is empty", who, slot_add);
        // stored from a fedd_pattern_build pattern of THIS mesh (or written here): its entries then sit where the closed form says
        const bool tagged = add->mesh_id == c->mesh_id && add->dofs == dim &&
                            (add->block_mode == FEDD_BLOCK_DIAG || add->block_mode == FEDD_BLOCK_FULL);
        const int64_t want = add->block_mode == FEDD_BLOCK_FULL ? nnz : c->adv_node_nnz * dim;
        FEDD_CHECK(tagged && add->n_rows == n_rows && add->n_cols == c->n_node * dim && add->nnz == want,
                   "%s: slot %d does not hold a DIAG or FULL velocity matrix of this mesh", who, slot_add);
    }
    DevCsr& out = c->aux[slot_out];
    if (!(out.valid && out.pattern_id != 0 && out.pattern_id == c->adv_pattern_id[slot_out])) {
        FEDD_TRY(out.rowptr.ensure((size_t)n_rows + 1));
        FEDD_TRY(out.colind.ensure((size_t)nnz));
        FEDD_TRY(out.val.ensure((size_t)nnz));
        FEDD_TRY(expand_node_pattern(c, c->d_adv_nptr.p, c->d_adv_ncol.p, dim, 1, out.rowptr.p, out.colind.p));
        out.n_rows = n_rows;
        out.n_cols = c->n_node * dim;
        out.nnz = nnz;
        out.max_row_nnz = c->adv_max_nn * dim;
        out.pattern_id = c->adv_pattern_id[slot_out] = ++c->pattern_counter;
    }
    out.dofs = dim;
    out.block_mode = FEDD_BLOCK_FULL;
    out.mesh_id = c->mesh_id;
    FEDD_TRY(with_element(dim, nen, [&](auto d, auto n) {
        constexpr int D = decltype(d)::value, N = decltype(n)::value;
        return ale ? advection_ale_kind<D, N>(c, kind, scale, add, out) : advection_kind<D, N>(c, kind, scale, add, out);
    }));
    out.valid = true;
    out.value_id = ++c->value_counter;
    return 0;
}

// aux[slot_out] <- scale * (N | W | N + W)(u) + aux[slot_add]: NavierStokes::reAssemble (NavierStokes_def.hpp:282-321) in one pass
int assemble_advection(fedd_ctx* c, int kind, double scale, int slot_add, int slot_out) {
    FEDD_CHECK(c->nranks == 1, "fedd_assemble_advection: one rank only for now");
    FEDD_CHECK(c->have_vel, "fedd_assemble_advection: call fedd_velocity_set first");
    return advection_into_slot(c, "fedd_assemble_advection", false, kind, scale, slot_add, slot_out);
}

// ... and on a moving mesh: NavierStokes::reAssembleFSI (NavierStokes_def.hpp:245-278) with the P of FSI_def.hpp:497-503
int assemble_advection_ale(fedd_ctx* c, int kind, double scale, int slot_add, int slot_out) {
    FEDD_CHECK(c->nranks == 1, "fedd_assemble_advection_ale: one rank only (a context with %d ranks was given)", c->nranks);
    FEDD_CHECK(kind == FEDD_ALE_P || c->have_vel, "fedd_assemble_advection_ale: no velocity: call fedd_velocity_set first");
    FEDD_CHECK(c->have_mvel,
               "fedd_assemble_advection_ale: no mesh velocity: call fedd_mesh_velocity_set or fedd_mesh_velocity_diff first");
    return advection_into_slot(c, "fedd_assemble_advection_ale", true, kind, scale, slot_add, slot_out);
}

int assemble_matrix(fedd_ctx* c, int form, const double* params, const double* coeff_q, int64_t n_coeff) {
    const int dim = c->dim, nen = c->nen;
    int kform, degree;
    const int dg = fe_degree(nen, dim, true), ds = fe_degree(nen, dim, false);
    switch (form) {
        case FEDD_FORM_LAPLACE:
            FEDD_CHECK(c->dofs == 1, "assemblyLaplace needs a scalar pattern");
            kform = F_LAPLACE; degree = dg + dg; break;
        case FEDD_FORM_LAPLACE_VEC:
            FEDD_CHECK(c->dofs == dim && c->block_mode == FEDD_BLOCK_DIAG, "assemblyLaplaceVecField needs a DIAG pattern with dim dofs per node");
            kform = F_LAPLACE; degree = dg + dg; break;
        case FEDD_FORM_MASS:
            FEDD_CHECK(c->dofs == 1, "assemblyMass(Scalar) needs a scalar pattern");
            kform = F_MASS; degree = ds + ds; break;
        case FEDD_FORM_MASS_VEC:
            FEDD_CHECK(c->dofs == dim && c->block_mode == FEDD_BLOCK_DIAG, "assemblyMass(Vector) needs a DIAG pattern with dim dofs per node");
            kform = F_MASS; degree = ds + ds; break;
        case FEDD_FORM_BDSTAB:
            FEDD_CHECK(c->dofs == 1, "assemblyBDStabilization needs a scalar pattern");
            FEDD_CHECK(nen == dim + 1, "assemblyBDStabilization: only implemented for P1 (FE_def.hpp:2156)");
            kform = F_MASS; degree = ds + ds; break;
        case FEDD_FORM_LINELAS:
            FEDD_CHECK(c->dofs == dim && c->block_mode == FEDD_BLOCK_FULL, "assemblyLinElasXDim needs a FULL pattern with dim dofs per node");
            FEDD_CHECK(params, "assemblyLinElasXDim needs params = {lambda, mu}");
            kform = F_LINELAS; degree = dg + dg; break;
        case FEDD_FORM_STRESS:
            FEDD_CHECK(c->nranks == 1, "fedd_assemble_stress: one rank only (a context with %d ranks was given)", c->nranks);
            FEDD_CHECK(!c->merged && c->dofs == dim && c->block_mode == FEDD_BLOCK_FULL && c->n_rowg == 0,
                       "fedd_assemble_stress: assemblyStress needs a FULL pattern with dim dofs per node "
                       "(fedd_pattern_build(dim, FEDD_BLOCK_FULL)) as system matrix");
            kform = F_STRESS; degree = dg + dg; break;
        case FEDD_FORM_LAPLACE_XDIM:
            FEDD_CHECK(!c->merged && c->dofs == dim && c->block_mode == FEDD_BLOCK_DIAG && c->n_rowg == 0,
                       "assemblyLaplaceXDim needs a DIAG pattern with dim dofs per node (fedd_pattern_build(dim, FEDD_BLOCK_DIAG)) "
                       "as system matrix");
            FEDD_CHECK(params, "assemblyLaplaceXDim needs params = {distance, coefficient} (\"Distance Laplace\", \"Coefficient Laplace\")");
            FEDD_CHECK(c->have_idist, "assemblyLaplaceXDim needs the distances to the interface: call fedd_interface_distance "
                                      "(or fedd_interface_distance_points / fedd_interface_distance_set) first");
            kform = F_LAPLACE; degree = dg + dg; break;
        default:
            FEDD_CHECK(false, "fedd_assemble: unknown form %d", form);
    }
    if (degree == 0) degree = 1;  // FE::determineDegree, FE_def.hpp:5508-5509
    int nq = 0, ntab = 0;
    if (kform == F_STRESS) {
        // the lists of the FULL pattern and the tables of this rule are kept per (mesh, pattern); c(x_k) goes up beside them
        FEDD_TRY(full_lists_ensure(c, "fedd_assemble_stress"));
        nq = c->hy_nq;
        FEDD_CHECK(!coeff_q || n_coeff == c->n_elem * nq,
                   "fedd_assemble_stress: n_coeff = %lld, but the mesh has %lld elements x %d quadrature points = %lld", (long long)n_coeff,
                   (long long)c->n_elem, nq, (long long)(c->n_elem * nq));
        if (coeff_q && n_coeff > 0) {
            FEDD_TRY(c->d_dtmp0.ensure(std::max<size_t>((size_t)n_coeff, c->d_dtmp0.cap)));
            FEDD_HIP(hipMemcpyAsync(c->d_dtmp0.p, coeff_q, (size_t)n_coeff * sizeof(double), hipMemcpyHostToDevice, c->stream));
            FEDD_HIP(hipStreamSynchronize(c->stream));  // the array is the caller's
        }
    }
    system_written(c, SYS_VALUES);
    if (kform != F_STRESS) FEDD_TRY(upload_tables(c, degree, nq, ntab));
    AsmArgs a;
    a.conn = c->d_conn.p; a.n2e_ptr = c->d_n2e_ptr.p; a.n2e = c->d_n2e.p; a.rowptr = c->d_rowptr.p;
    a.colind = c->d_colind.p; a.xyz = c->d_xyz.p; a.val = c->d_val.p; a.tab = c->d_dtmp0.p;
    a.nq = nq; a.n_rows = (int32_t)c->n_rows_ext; a.dofs = c->dofs;
    a.p0 = params ? params[0] : 0.0;
    a.p1 = params ? params[1] : 0.0;
    a.ke = nullptr;
    // doSetZeros: of the matrix forms built here only the vector Laplacian thresholds (FE_def.hpp:719-721; assemblyLaplace does not)
    a.zero_eps = form == FEDD_FORM_LAPLACE_VEC ? c->asm_zero_eps : 0.0;
    if (kform == F_STRESS) {
        a.tab = c->d_hy_tab.p;
        a.coeff = coeff_q && n_coeff > 0 ? c->d_dtmp0.p : nullptr;
    }
    const bool xdim = form == FEDD_FORM_LAPLACE_XDIM;
    if (kform == F_MASS) {   // the constant the Bochev-Dohrmann block takes off every mass entry: |ref. element| x scale (FE_def.hpp:2183-2192)
        a.p0 = form == FEDD_FORM_BDSTAB ? (dim == 2 ? 0.5 : 1.0 / 6.0) : 0.0;
        a.p1 = form == FEDD_FORM_BDSTAB ? (dim == 2 ? 1.0 / 9.0 : 1.0 / 16.0) : 0.0;
    }
    return with_element(dim, nen, [&](auto d, auto n) {
        return launch_assemble<decltype(d)::value, decltype(n)::value>(c, kform, a, ntab, xdim);
    });
}

int assemble_rhs(fedd_ctx* c, int dofs, const double* f_const, int extra_degree) {
    const int dim = c->dim, nen = c->nen;
    int degree = fe_degree(nen, dim, false);
    if (degree == 0) degree = 1;
    degree += extra_degree;  // FE_def.hpp:4717-4718
    FeTables tb;
    FEDD_TRY(fe_tables(dim, nen, degree, tb));
    RhsArgs a;
    a.conn = c->d_conn.p; a.n2e_ptr = c->d_n2e_ptr.p; a.n2e = c->d_n2e.p; a.xyz = c->d_xyz.p;
    a.rhs = c->d_rhs.p; a.n_own = (int32_t)c->n_own; a.nen = nen; a.dofs = dofs;
    for (int i = 0; i < 10; ++i) a.base[i] = 0.0;
    for (int i = 0; i < nen; ++i) {
        double s = 0.0;
        for (int q = 0; q < tb.nq; ++q) s += tb.w[q] * tb.phi[(size_t)q * nen + i];
        a.base[i] = s;
    }
    for (int d = 0; d < MAX_DOFS; ++d) a.f[d] = d < dofs ? f_const[d] : 0.0;
    const dim3 grid((unsigned)((c->n_own + 255) / 256)), block(256);
    // |det B_e| follows d_conn and d_xyz alone.  Option "setup_fused" keeps it in a buffer of its own from call to call (a Newton
    // loop, a time loop and the bench assemble again and again on one geometry) while the two stand: d_conn and d_xyz are
    // written by fedd_mesh_set* (mesh_gen; a P2 mesh, a second mesh, the sides of an FSI problem all arrive through it) and d_xyz by
    // a committed fedd_mesh_move (geometry_id; the ALE and FSI geometry steps move the mesh through it), and by nothing else.
    const bool keep = c->setup_fused != 0;
    const bool kept = keep && c->absdet_valid && c->absdet_mesh_gen == c->mesh_gen && c->absdet_geometry_id == c->geometry_id &&
                      c->d_absdet.cap >= (size_t)c->n_elem;
    if (keep) FEDD_TRY(c->d_absdet.ensure((size_t)c->n_elem));
    else FEDD_TRY(c->d_dtmp0.ensure(std::max<size_t>((size_t)c->n_elem, c->d_dtmp0.cap)));
    double* absdet = keep ? c->d_absdet.p : c->d_dtmp0.p;
    const dim3 egrid((unsigned)((c->n_elem + 255) / 256));
    ScopedTimer t(c, FEDD_T_RHS);
    if (!kept && dim == 2)
        hipLaunchKernelGGL(k_elem_absdet<2>, egrid, block, 0, c->stream, (const int32_t*)c->d_conn.p, nen,
                           (const double*)c->d_xyz.p, c->n_elem, absdet);
    else if (!kept)
        hipLaunchKernelGGL(k_elem_absdet<3>, egrid, block, 0, c->stream, (const int32_t*)c->d_conn.p, nen,
                           (const double*)c->d_xyz.p, c->n_elem, absdet);
    if (kept) ++c->fused_absdet_kept;
    if (keep) {
        c->absdet_valid = true;
        c->absdet_mesh_gen = c->mesh_gen;
        c->absdet_geometry_id = c->geometry_id;
    }
    const int cap = std::max(256, std::min(RHS_NPB * std::max(1, c->max_deg), 6144));
    hipLaunchKernelGGL(k_rhs, dim3((unsigned)((c->n_own + RHS_NPB - 1) / RHS_NPB)), block, (size_t)cap * sizeof(double),
                       c->stream, a, (const double*)absdet, cap);
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}

int apply_dirichlet_nodes(fedd_ctx* c, int64_t n, const int32_t* nodes, const int32_t* comp_mask, const double* values) {
    const int dofs = c->dofs;
    for (int64_t k = 0; k < n; ++k)
        FEDD_CHECK(nodes[k] >= 0 && nodes[k] < c->n_own + c->n_rowg, "fedd_dirichlet_nodes: node %d has no rows on this rank", nodes[k]);
    system_written(c, SYS_DIRICHLET);
    if (n == 0) return 0;
    FEDD_TRY(c->d_itmp0.ensure(std::max<size_t>((size_t)n * (1 + dofs), c->d_itmp0.cap)));
    FEDD_TRY(c->d_dtmp0.ensure(std::max<size_t>((size_t)n * dofs, c->d_dtmp0.cap)));
    int32_t* d_nodes = c->d_itmp0.p;
    int32_t* d_mask = comp_mask ? c->d_itmp0.p + n : nullptr;
    FEDD_HIP(hipMemcpyAsync(d_nodes, nodes, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (comp_mask) FEDD_HIP(hipMemcpyAsync(d_mask, comp_mask, (size_t)n * dofs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipMemcpyAsync(c->d_dtmp0.p, values, (size_t)n * dofs * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ScopedTimer t(c, FEDD_T_DIRICHLET);
    hipLaunchKernelGGL(k_dirichlet_nodes, dim3((unsigned)((n * dofs + 255) / 256)), dim3(256), 0, c->stream,
                       (const int32_t*)d_nodes, (const int32_t*)d_mask, (const double*)c->d_dtmp0.p, (int32_t)n, dofs,
                       (const int32_t*)c->d_rowptr.p, (const int32_t*)c->d_colind.p, c->d_val.p, c->d_rhs.p, c->d_isdir.p);
    t.stop();
    FEDD_HIP(hipGetLastError());
    FEDD_HIP(hipStreamSynchronize(c->stream));  // host staging buffers are the caller's
    return 0;
}

// generic variant on system rows (merged block systems): row <- unit row, rhs <- value.  On a merged
// matrix this equals setLocalRowOne on the diagonal block + setLocalRowZero on the off-diagonal
// blocks of that block row (BCBuilder_def.hpp:589-707) applied before the merge.
int apply_dirichlet_rows(fedd_ctx* c, int64_t n, const int32_t* rows, const double* values) {
    for (int64_t k = 0; k < n; ++k)
        FEDD_CHECK(rows[k] >= 0 && rows[k] < c->n_rows, "fedd_dirichlet_rows: row %d out of range", rows[k]);
    system_written(c, SYS_DIRICHLET);
    if (n == 0) return 0;
    FEDD_TRY(c->d_itmp0.ensure(std::max<size_t>((size_t)n, c->d_itmp0.cap)));
    FEDD_TRY(c->d_dtmp0.ensure(std::max<size_t>((size_t)n, c->d_dtmp0.cap)));
    FEDD_HIP(hipMemcpyAsync(c->d_itmp0.p, rows, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipMemcpyAsync(c->d_dtmp0.p, values, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // reuse the node kernel with one dof per "node": row ids are the node ids
    ScopedTimer t(c, FEDD_T_DIRICHLET);
    hipLaunchKernelGGL(k_dirichlet_nodes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       (const int32_t*)c->d_itmp0.p, (const int32_t*)nullptr, (const double*)c->d_dtmp0.p, (int32_t)n, 1,
                       (const int32_t*)c->d_rowptr.p, (const int32_t*)c->d_colind.p, c->d_val.p, c->d_rhs.p, c->d_isdir.p);
    t.stop();
    FEDD_HIP(hipGetLastError());
    FEDD_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int apply_dirichlet(fedd_ctx* c, int n_bc, const int32_t* flags, const int32_t* comp_mask, const double* values) {
    system_written(c, SYS_DIRICHLET);
    const BcTable b = bc_table_fill(c->dofs, n_bc, flags, comp_mask, values);
    // row-ghost rows get the same treatment as owned ones (their flags follow the owned flags in d_flag)
    const dim3 grid((unsigned)((c->n_rows_ext + 255) / 256)), block(256);
    ScopedTimer t(c, FEDD_T_DIRICHLET);
    hipLaunchKernelGGL(k_dirichlet, grid, block, 0, c->stream, b, c->d_flag.p, c->d_rowptr.p, c->d_colind.p,
                       c->d_val.p, c->d_rhs.p, c->d_isdir.p, (int32_t)c->n_rows_ext);
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Surface load vector: f_(i,d) = sum over the surface elements S that hold node i (as their local node li) of
//   scaling_S * (sum_q w_q phi_q,li) * g_S[d],   scaling_S = |B[:,0]| (2D) or |B[:,0] x B[:,1]| (3D),
// B = the vertex differences from vertex 0 (FE::assemblySurfaceIntegral[Flag] FE_def.hpp:4511-4691,
// buildTransformationSurface :5406-5428, SmallMatrix::computeScaling SmallMatrix.hpp:360-378), counted once per local
// volume element that holds the surface element (the reference walks the sub-elements of every element, :4550-4553).
// Two phases like the volume load vector above: one lane per surface element for the scaling, then a gather over the
// owned nodes' (surface element, local index) lists in list order -- no atomics, the sums do not depend on the launch shape.
// ------------------------------------------------------------------------------------------------
namespace {

// gmode 0: every element reads row 0 of the load table, 1: the row of its flag in flags[n_flags] (-1: none), 2: its own row
template <int DIM>
__global__ void k_surf_scaling(const int32_t* __restrict__ surf, int nsn, const double* __restrict__ xyz,
                               const int32_t* __restrict__ weight, const int32_t* __restrict__ sflag, int64_t n_surf, int gmode,
                               const int32_t* __restrict__ flags, int n_flags, double* __restrict__ scal, int32_t* __restrict__ gi) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_surf) return;
    double X[DIM][DIM];
#pragma unroll
    for (int v = 0; v < DIM; ++v) {
        const int32_t nd = surf[s * nsn + v];
#pragma unroll
        for (int d = 0; d < DIM; ++d) X[v][d] = xyz[(int64_t)nd * DIM + d];
    }
    double len;
    if constexpr (DIM == 2) {
        const double bx = X[1][0] - X[0][0], by = X[1][1] - X[0][1];
        len = sqrt(bx * bx + by * by);
    } else {
        double u[3], v[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            u[d] = X[1][d] - X[0][d];
            v[d] = X[2][d] - X[0][d];
        }
        const double c0 = u[1] * v[2] - u[2] * v[1], c1 = u[2] * v[0] - u[0] * v[2], c2 = u[0] * v[1] - u[1] * v[0];
        len = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    }
    scal[s] = len * (double)weight[s];
    int32_t row = gmode == 2 ? (int32_t)s : 0;
    if (gmode == 1) {
        row = -1;
        const int32_t f = sflag[s];
        for (int k = n_flags - 1; k >= 0; --k) row = flags[k] == f ? k : row;   // the first entry that names the flag
    }
    gi[s] = row;
}

// SURF_NPB owned nodes per workgroup: their pairs are one contiguous run of the adjacency, read coalesced (one lane per pair)
// into an LDS park in windows of SURF_CAP pairs; then one lane per node adds its segment in adjacency order.
constexpr int SURF_NPB = 64, SURF_CAP = 256;

struct SurfArgs {
    const int32_t* s2n_ptr;
    const int32_t* s2n;
    const double* scal;
    const int32_t* gi;
    const double* g;
    double* rhs;
    int32_t n_own;
    int nsn, dofs, accumulate;
    double base[6];  // sum_q w_q phi_q,i
};

__global__ __launch_bounds__(SURF_CAP) void k_surf_rhs(SurfArgs a) {
    __shared__ double park[SURF_CAP];
    __shared__ int32_t parkg[SURF_CAP];
    const int32_t node0 = blockIdx.x * SURF_NPB;
    const int32_t node1 = min(a.n_own, node0 + SURF_NPB);
    const int32_t p0 = a.s2n_ptr[node0], p1 = a.s2n_ptr[node1];
    const int tid = threadIdx.x;
    const int32_t node = node0 + tid;
    const bool mine = tid < SURF_NPB && node < node1;
    const int32_t nb = mine ? a.s2n_ptr[node] : 0, ne = mine ? a.s2n_ptr[node + 1] : 0;
    double sum[MAX_DOFS];
#pragma unroll
    for (int d = 0; d < MAX_DOFS; ++d) sum[d] = 0.0;
    for (int32_t w0 = p0; w0 < p1; w0 += SURF_CAP) {
        const int32_t w1 = min(p1, w0 + SURF_CAP);
        if (w0 + tid < w1) {
            const int32_t idx = a.s2n[w0 + tid];
            const int32_t s = idx / a.nsn;
            const int li = idx - s * a.nsn;
            double b = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) b = i == li ? a.base[i] : b;
            park[tid] = a.scal[s] * b;
            parkg[tid] = a.gi[s];
        }
        __syncthreads();
        for (int32_t p = max(nb, w0); p < min(ne, w1); ++p) {
            const int32_t row = parkg[p - w0];
            if (row < 0) continue;
            const double v = park[p - w0];
#pragma unroll
            for (int d = 0; d < MAX_DOFS; ++d)
                if (d < a.dofs) sum[d] += v * a.g[(int64_t)row * a.dofs + d];
        }
        __syncthreads();
    }
    if (!mine || (a.accumulate && nb == ne)) return;   // accumulating: a node without surface elements keeps its value
#pragma unroll
    for (int d = 0; d < MAX_DOFS; ++d)
        if (d < a.dofs) {
            double* out = a.rhs + (int64_t)node * a.dofs + d;
            *out = a.accumulate ? *out + sum[d] : sum[d];
        }
}

struct FaceKeyHash {
    size_t operator()(const std::array<int32_t, 3>& k) const {
        uint64_t h = 0x9E3779B97F4A7C15ull;
        for (int32_t v : k) h = (h ^ (uint64_t)(uint32_t)v) * 0xFF51AFD7ED558CCDull, h ^= h >> 32;
        return (size_t)h;
    }
};

}  // namespace

int surface_set(fedd_ctx* c, int nsn, int64_t n_surf, const int32_t* surf, const int32_t* sflag) {
    const int dim = c->dim;
    c->have_surf = false;
    c->n_surf = 0;
    c->surf_nsn = nsn;
    if (n_surf == 0) {
        c->have_surf = true;
        return 0;
    }
    const int64_t n_rep = (int64_t)c->h_col_of_rep.size();
    std::vector<int32_t> surf2((size_t)(n_surf * nsn));
    for (int64_t k = 0; k < n_surf * nsn; ++k) {
        FEDD_CHECK(surf[k] >= 0 && surf[k] < n_rep, "fedd_surface_set: surface node id %d out of range", surf[k]);
        surf2[k] = c->h_col_of_rep[surf[k]];
    }
    // weight: the local volume elements that hold all vertices of the surface element, through a map of the listed faces
    typedef std::array<int32_t, 3> Key;
    auto key_of = [dim](const int32_t* v) {
        Key k = {v[0], v[1], dim == 3 ? v[2] : -1};
        std::sort(k.begin(), k.begin() + dim);
        return k;
    };
    std::unordered_map<Key, int32_t, FaceKeyHash> count;
    count.reserve((size_t)n_surf * 2);
    for (int64_t s = 0; s < n_surf; ++s) count.emplace(key_of(&surf2[s * nsn]), 0);
    std::vector<int32_t> conn((size_t)(c->n_elem * c->nen));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    if (!conn.empty()) FEDD_HIP(hipMemcpy(conn.data(), c->d_conn.p, conn.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<char> on_surf((size_t)c->n_node, 0);   // (only elements with dim vertices on listed faces are looked up)
    for (int64_t s = 0; s < n_surf; ++s)
        for (int v = 0; v < dim; ++v) on_surf[surf2[s * nsn + v]] = 1;
    for (int64_t e = 0; e < c->n_elem; ++e) {
        int marked = 0;
        for (int j = 0; j <= dim; ++j) marked += on_surf[conn[e * c->nen + j]];
        if (marked < dim) continue;
        for (int skip = 0; skip <= dim; ++skip) {
            int32_t v[3] = {0, 0, 0};
            int k = 0;
            for (int j = 0; j <= dim; ++j)
                if (j != skip) v[k++] = conn[e * c->nen + j];
            auto it = count.find(key_of(v));
            if (it != count.end()) ++it->second;
        }
    }
    std::vector<int32_t> weight((size_t)n_surf);
    for (int64_t s = 0; s < n_surf; ++s) weight[s] = count[key_of(&surf2[s * nsn])];
    FEDD_TRY(c->d_surf.ensure(surf2.size()));
    FEDD_TRY(c->d_sflag.ensure((size_t)n_surf));
    FEDD_TRY(c->d_sweight.ensure((size_t)n_surf));
    FEDD_HIP(hipMemcpy(c->d_surf.p, surf2.data(), surf2.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    FEDD_HIP(hipMemcpy(c->d_sflag.p, sflag, (size_t)n_surf * sizeof(int32_t), hipMemcpyHostToDevice));
    FEDD_HIP(hipMemcpy(c->d_sweight.p, weight.data(), (size_t)n_surf * sizeof(int32_t), hipMemcpyHostToDevice));
    int32_t max_deg = 0;
    FEDD_TRY(build_node_lists(c, c->d_surf.p, n_surf * nsn, (int32_t)c->n_own, c->d_s2n_ptr, c->d_s2n, &max_deg));
    FEDD_HIP(hipStreamSynchronize(c->stream));
    c->n_surf = n_surf;
    c->have_surf = true;
    return 0;
}

int assemble_surface(fedd_ctx* c, int dofs, int n_flags, const int32_t* flags, const double* g, const double* g_surf,
                     int extra_degree, int accumulate) {
    SurfArgs a;
    for (int i = 0; i < 6; ++i) a.base[i] = 0.0;
    FEDD_TRY(fe_surface_base(c->dim, c->surf_nsn, extra_degree, a.base));
    const int64_t n_surf = c->n_surf;
    if (n_surf == 0 || c->n_own == 0) {   // the empty set: nothing to add; overwriting leaves the zero vector
        if (!accumulate) FEDD_HIP(hipMemsetAsync(c->d_rhs.p, 0, (size_t)c->n_rows * sizeof(double), c->stream));
        return 0;
    }
    const int gmode = g_surf ? 2 : (n_flags > 0 ? 1 : 0);
    const size_t ng = (size_t)(gmode == 2 ? n_surf : (gmode == 1 ? n_flags : 1)) * dofs;
    FEDD_TRY(c->d_sg.ensure(ng));
    FEDD_TRY(c->d_sscal.ensure((size_t)n_surf));
    FEDD_TRY(c->d_sgi.ensure((size_t)n_surf + (size_t)n_flags));
    int32_t* d_flags = c->d_sgi.p + n_surf;
    FEDD_HIP(hipStreamSynchronize(c->stream));   // an earlier launch may still read the tables
    FEDD_HIP(hipMemcpy(c->d_sg.p, g_surf ? g_surf : g, ng * sizeof(double), hipMemcpyHostToDevice));
    if (n_flags > 0) FEDD_HIP(hipMemcpy(d_flags, flags, (size_t)n_flags * sizeof(int32_t), hipMemcpyHostToDevice));
    a.s2n_ptr = c->d_s2n_ptr.p; a.s2n = c->d_s2n.p; a.scal = c->d_sscal.p; a.gi = c->d_sgi.p; a.g = c->d_sg.p;
    a.rhs = c->d_rhs.p; a.n_own = (int32_t)c->n_own; a.nsn = c->surf_nsn; a.dofs = dofs; a.accumulate = accumulate;
    const dim3 sgrid((unsigned)((n_surf + 255) / 256)), block(256);
    ScopedTimer t(c, FEDD_T_RHS);
    if (c->dim == 2)
        hipLaunchKernelGGL(k_surf_scaling<2>, sgrid, block, 0, c->stream, (const int32_t*)c->d_surf.p, c->surf_nsn,
                           (const double*)c->d_xyz.p, (const int32_t*)c->d_sweight.p, (const int32_t*)c->d_sflag.p, n_surf, gmode,
                           (const int32_t*)d_flags, n_flags, c->d_sscal.p, c->d_sgi.p);
    else
        hipLaunchKernelGGL(k_surf_scaling<3>, sgrid, block, 0, c->stream, (const int32_t*)c->d_surf.p, c->surf_nsn,
                           (const double*)c->d_xyz.p, (const int32_t*)c->d_sweight.p, (const int32_t*)c->d_sflag.p, n_surf, gmode,
                           (const int32_t*)d_flags, n_flags, c->d_sscal.p, c->d_sgi.p);
    hipLaunchKernelGGL(k_surf_rhs, dim3((unsigned)((c->n_own + SURF_NPB - 1) / SURF_NPB)), dim3(SURF_CAP), 0, c->stream, a);
    t.stop();
    FEDD_HIP(hipGetLastError());
    return 0;
}

}  // namespace fedd
