#pragma once
// The device side of the gather lists (GatherLists in fedd_internal.hpp; DESIGN.md section 4 "Gather lists and the row walk"):
// the encoding of a source, the node-level view of a pattern, the row walk.  Sums only, and no contraction pragma: an epilogue
// is compiled under the setting of the place it is written at -- k_adv_gather's scale * sum + M (assemble.hip) under the
// compiler's default, so it may be one fused multiply-add; k_hyper_gather's (cm * M) + K below `#pragma clang fp contract(off)`
// of hyperelastic.hip, two roundings as fedd_matrix_combine makes them (test_gpu_newton_newmark.py pins the bits).
#include "fedd_internal.hpp"
#include <algorithm>

namespace fedd {

__host__ __device__ constexpr uint16_t gather_pack(int q, int j) { return (uint16_t)((q << 4) | j); }
__host__ __device__ constexpr uint32_t gather_q(uint32_t sr) { return sr >> 4; }
__host__ __device__ constexpr uint32_t gather_j(uint32_t sr) { return sr & 15u; }

// workgroups (of 256 threads) of k_p2_lists or of a gather kernel over nn nodes: a wave per node, grid-stride
inline int gather_grid(int64_t nn) { return (int)std::max<int64_t>(1, std::min<int64_t>((nn + 3) / 4, 256 * 32)); }

// one node's slots: the node's first row, their first index in soff, their number, where the first row starts in the values
struct GatherRow { int32_t row, nb, nslot, rs; };

// The node-level view of a CSR pattern with dofs rows per node: scalar rows or DIAG blocks (a node's row holds its slots), or
// FULL dofs x dofs blocks (dofs entries per slot and row).  A node-level pattern is the scalar case.
struct GatherRows {
    const int32_t* rowptr;
    int dofs, full;
    __device__ GatherRow operator()(int64_t p) const {
        const int32_t row = (int32_t)p * dofs, rs = rowptr[row], len = rowptr[row + 1] - rs;
        return {row, dofs == 1 ? rs : (full ? rs / (dofs * dofs) : rs / dofs), full ? len / dofs : len, rs};
    }
};

// The sums of one slot where a source is a block of BLK doubles at ke[(at * NEN + j) * BLK]
template <int NEN, int BLK>
struct GatherBlockSum {
    const double* ke;
    double acc[BLK];
    __device__ void zero() {
#pragma unroll
        for (int m = 0; m < BLK; ++m) acc[m] = 0.0;
    }
    __device__ void init(const GatherRow&, int) { zero(); }
    __device__ void add(int32_t at, int j) {
        const double* __restrict__ kb = ke + ((int64_t)at * NEN + j) * BLK;
#pragma unroll
        for (int m = 0; m < BLK; ++m) acc[m] += kb[m];
    }
};

// The walk: a wave per node, a lane per node-level nonzero, every lane takes its sources in list order.  256 threads.  Acc:
// init(r, sl) before the sources of slot sl of the node with rows r (loads that must precede the sums go here), add(at, j) for
// one source (at = the n2e entry, element * NEN + local index of the node in it; j = local column), store(r, sl) at the end
template <int NEN, class Acc>
__device__ __forceinline__ void gather_walk(const int32_t* __restrict__ n2e_ptr, const int32_t* __restrict__ n2e,
                                            const uint16_t* __restrict__ soff, const uint16_t* __restrict__ src, int32_t nn,
                                            GatherRows rows, Acc acc) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t p = (int64_t)blockIdx.x * 4 + w; p < nn; p += (int64_t)gridDim.x * 4) {
        const int32_t ab = n2e_ptr[p], deg = n2e_ptr[p + 1] - ab;
        const GatherRow r = rows(p);
        const uint16_t* __restrict__ sp = src + (int64_t)ab * NEN;
        const int total = deg * NEN;
        for (int sl = lane; sl < r.nslot; sl += 64) {
            const int b = soff[r.nb + sl], e2 = sl + 1 < r.nslot ? (int)soff[r.nb + sl + 1] : total;
            acc.init(r, sl);
            for (int k = b; k < e2; ++k) {
                const uint32_t sr = sp[k];
                acc.add(n2e[ab + gather_q(sr)], (int)gather_j(sr));
            }
            acc.store(r, sl);
        }
    }
}

}  // namespace fedd
