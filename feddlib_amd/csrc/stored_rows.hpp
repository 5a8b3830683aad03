#pragma once
// The lane-group row walk over a stored CSR (DESIGN.md section 4 "Stored blocks: the lane-group row walk and child contexts";
// the order is normative, include/fedd_hip.h): the loop of k_block_apply (timestep.hip), k_newton_residual (newton.hip), k_bt_sub
// (blockprec.hip) and k_facsi_rows (fsi.hip), and the host ladder that picks their lane groups.  The products and the sums are
// made here, and a host restatement adds every rounded product on its own, so this header must not depend on its includer's
// contraction setting and must not change it: `#pragma clang fp contract(off)` stands inside the function bodies, where it has
// compound-statement scope.  gather_lists.hpp makes the opposite choice for a walk that only adds.
#include "fedd_internal.hpp"
#include <type_traits>

namespace fedd {

// The walk of one row by its G lanes: lane g takes entries g, g + G, ... of the len entries behind s, four trips at a time.  The
// column indices and values of the four trips are loaded first, then the four x entries, then the products go to the sums in
// trip order; the lane sums are combined by a fixed shuffle tree, so two calls give the same bits.  A dead lane group walks with
// len = 0 (the tree needs all lanes).  Sums:
//   keep(col)       false drops the entry: its value is not loaded and it reaches no sum
//   x(col)          the entry of the vector (a load, or a load and a product rounded before it is used)
//   add(col, p)     the rounded product val * x(col) of a kept entry; of a dropped or missing one, col = -1 and p = 0.0
//   fold<G>(o)      one level of the tree: every sum += __shfl_xor(sum, o, G)
// Sums that declare `static constexpr int EXTRA = E` carry E further sums over the same columns, each with a value array and a
// vector of its own (singlestep.hip: the stage operators of a Runge-Kutta step share one pattern, so its row pointers and
// columns are read once for all of them).  Their loads and products follow the first sum's at every step of the order above:
//   val_extra(e)        the value array of extra sum e (same pattern as val), nullptr: the sum is off and nothing is loaded for it
//   x_extra(e, col)     its vector entry
//   add_extra(e, p)     the rounded product of a kept entry, or 0.0
// A walk without EXTRA compiles to what it was before they existed.
template <class Sums, class = void>
struct extra_sums : std::integral_constant<int, 0> {};
template <class Sums>
struct extra_sums<Sums, std::void_t<decltype(Sums::EXTRA)>> : std::integral_constant<int, Sums::EXTRA> {};

template <int G, class Sums>
__device__ __forceinline__ void row_walk(const int32_t* __restrict__ colind, const double* __restrict__ val, int32_t s, int32_t len,
                                         int g, Sums& sums) {
#pragma clang fp contract(off)
    constexpr int E = extra_sums<Sums>::value;
    for (int32_t k0 = g; k0 < len; k0 += 4 * G) {
        int32_t cc[4];
        double vv[4], xx[4];
        double ve[E > 0 ? E : 1][4], xe[E > 0 ? E : 1][4];
        (void)ve;
        (void)xe;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int32_t k = k0 + u * G;
            const int32_t col = k < len ? colind[s + k] : -1;
            const bool in = k < len && sums.keep(col);
            cc[u] = in ? col : -1;
            vv[u] = in ? val[s + k] : 0.0;
        }
        if constexpr (E > 0) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double* __restrict__ v = sums.val_extra(e);
#pragma unroll
                for (int u = 0; u < 4; ++u) ve[e][u] = v && cc[u] >= 0 ? v[s + k0 + u * G] : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) xx[u] = cc[u] >= 0 ? sums.x(cc[u]) : 0.0;
        if constexpr (E > 0) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const bool on = sums.val_extra(e) != nullptr;
#pragma unroll
                for (int u = 0; u < 4; ++u) xe[e][u] = on && cc[u] >= 0 ? sums.x_extra(e, cc[u]) : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) sums.add(cc[u], vv[u] * xx[u]);
        if constexpr (E > 0) {
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int u = 0; u < 4; ++u) sums.add_extra(e, ve[e][u] * xe[e][u]);
        }
    }
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) sums.template fold<G>(o);
}

// One sum over every entry of the row: acc = sum_k val[k] * x(col[k])
template <class X>
struct RowSum {
    X x;
    double acc = 0.0;
    __device__ bool keep(int32_t) const { return true; }
    __device__ void add(int32_t, double p) {
#pragma clang fp contract(off)
        acc += p;
    }
    template <int G>
    __device__ void fold(int o) { acc += __shfl_xor(acc, o, G); }
};

template <int G, class X>
__device__ __forceinline__ double row_sum(const int32_t* __restrict__ colind, const double* __restrict__ val, int32_t s, int32_t len,
                                          int g, X x) {
    RowSum<X> sums{x};
    row_walk<G>(colind, val, s, len, g, sums);
    return sums.acc;
}

// The lane groups of a walk over n_rows rows of a block whose longest row has max_row_nnz entries: 8 lanes per row up to 32
// entries, else 16.  f(std::integral_constant<int, G>(), grid), grid = the workgroups of 256 threads that hold n_rows * G lanes
template <class F>
int with_row_groups(int32_t max_row_nnz, int64_t n_rows, F&& f) {
    if (max_row_nnz <= 32) return f(std::integral_constant<int, 8>(), (unsigned)((n_rows * 8 + 255) / 256));
    return f(std::integral_constant<int, 16>(), (unsigned)((n_rows * 16 + 255) / 256));
}

}  // namespace fedd
