#pragma once
// What the assembly translation units share: the forms, the kernel arguments and the affine geometry of a simplex.
#include "fedd_internal.hpp"
#include <type_traits>

namespace fedd {

// F_DIV / F_DIVT: FE::assemblyDivAndDivT (feddlib/core/FE/FE_def.hpp:1932-2057), pressure = P1 on
// the element's vertices.  F_DIV rows = pressure nodes, columns = DIM*velocity node + d;
// F_DIVT rows = velocity dofs, columns = pressure nodes.
// F_STRESS: FE::assemblyStress (FE_def.hpp:2407-2733), the velocity block in stress form; assemble.hip k_stress_elem.
enum { F_LAPLACE = 0, F_MASS = 1, F_LINELAS = 2, F_DIV = 3, F_DIVT = 4, F_STRESS = 5 };

struct AsmArgs {
    const int32_t* conn;
    const int32_t* n2e_ptr;
    const int32_t* n2e;
    const int32_t* rowptr;
    const int32_t* colind;
    const double* xyz;
    double* val;
    const double* tab;  // w[nq] | phi[nq*nen] | dphi[nq*nen*dim] | psi[nq*(dim+1)] (P1 pressure basis)
    int nq;
    int32_t n_rows;
    int dofs;
    double p0, p1;  // LINELAS: lambda, mu
    const double* ke;   // != nullptr: element matrices [E][NEN][NEN] computed beforehand by k_elem_matrix (P2 scalar forms)
    double zero_eps; // > 0: element contributions of magnitude below it are set to zero before they are added (the reference's
                     // optional setZeros_ / myeps_, FE_def.hpp:74-79, 719-721, 2002-2004, 2032-2034: vector Laplacian, B, B^T)
    const double* coeff = nullptr;  // F_STRESS: c(x_k) per element and quadrature point [E][nq]; nullptr: c = 1
    const double* fscale = nullptr; // FEDD_FORM_LAPLACE_XDIM: the coefficient f per element [E] (k_elem_matrix<..., SCALED>)
};

namespace {

// f(std::integral_constant<int, DIM>(), std::integral_constant<int, NEN>()) for the element of the mesh: P1 / P2 simplices in
// 2D and 3D (fedd_mesh_set admits no other); with_nen where the code depends on NEN alone
template <class F>
int with_element(int dim, int nen, F&& f) {
    if (dim == 2 && nen == 3) return f(std::integral_constant<int, 2>(), std::integral_constant<int, 3>());
    if (dim == 2 && nen == 6) return f(std::integral_constant<int, 2>(), std::integral_constant<int, 6>());
    if (dim == 3 && nen == 4) return f(std::integral_constant<int, 3>(), std::integral_constant<int, 4>());
    return f(std::integral_constant<int, 3>(), std::integral_constant<int, 10>());
}

template <class F>
int with_nen(int nen, F&& f) {
    if (nen == 3) return f(std::integral_constant<int, 3>());
    if (nen == 4) return f(std::integral_constant<int, 4>());
    if (nen == 6) return f(std::integral_constant<int, 6>());
    return f(std::integral_constant<int, 10>());
}

__device__ __forceinline__ double zero_small(const AsmArgs& a, double v) { return (a.zero_eps > 0.0 && fabs(v) < a.zero_eps) ? 0.0 : v; }

// affine map of a simplex: B[i][j] = x_{j+1}[i] - x_0[i]; returns det, fills Binv = adj(B)/det
template <int DIM>
__device__ __forceinline__ double affine(const double (&X)[DIM + 1][DIM], double (&Binv)[DIM][DIM]) {
    double B[DIM][DIM];
#pragma unroll
    for (int j = 0; j < DIM; ++j)
#pragma unroll
        for (int i = 0; i < DIM; ++i) B[i][j] = X[j + 1][i] - X[0][i];
    if constexpr (DIM == 2) {
        // one f64 division (the reference divides each adjugate entry by det; multiplying by the
        // correctly rounded reciprocal differs by <= 1 ulp per entry, far inside the 1e-10 bar)
        const double det = B[0][0] * B[1][1] - B[1][0] * B[0][1];
        const double rdet = 1.0 / det;
        Binv[0][0] = B[1][1] * rdet;
        Binv[0][1] = (-B[0][1]) * rdet;
        Binv[1][0] = (-B[1][0]) * rdet;
        Binv[1][1] = B[0][0] * rdet;
        return det;
    } else {
        const double det = B[0][0] * B[1][1] * B[2][2] + B[0][1] * B[1][2] * B[2][0] + B[0][2] * B[1][0] * B[2][1] -
                           B[2][0] * B[1][1] * B[0][2] - B[2][1] * B[1][2] * B[0][0] - B[2][2] * B[1][0] * B[0][1];
        const double rdet = 1.0 / det;
        Binv[0][0] = (B[1][1] * B[2][2] - B[1][2] * B[2][1]) * rdet;
        Binv[0][1] = (B[0][2] * B[2][1] - B[0][1] * B[2][2]) * rdet;
        Binv[0][2] = (B[0][1] * B[1][2] - B[0][2] * B[1][1]) * rdet;
        Binv[1][0] = (B[1][2] * B[2][0] - B[1][0] * B[2][2]) * rdet;
        Binv[1][1] = (B[0][0] * B[2][2] - B[0][2] * B[2][0]) * rdet;
        Binv[1][2] = (B[0][2] * B[1][0] - B[0][0] * B[1][2]) * rdet;
        Binv[2][0] = (B[1][0] * B[2][1] - B[1][1] * B[2][0]) * rdet;
        Binv[2][1] = (B[0][1] * B[2][0] - B[0][0] * B[2][1]) * rdet;
        Binv[2][2] = (B[0][0] * B[1][1] - B[0][1] * B[1][0]) * rdet;
        return det;
    }
}

template <int DIM>
__device__ __forceinline__ double affine_det(const double (&X)[DIM + 1][DIM]) {
    double B[DIM][DIM];
#pragma unroll
    for (int j = 0; j < DIM; ++j)
#pragma unroll
        for (int i = 0; i < DIM; ++i) B[i][j] = X[j + 1][i] - X[0][i];
    if constexpr (DIM == 2) {
        return B[0][0] * B[1][1] - B[1][0] * B[0][1];
    } else {
        return B[0][0] * B[1][1] * B[2][2] + B[0][1] * B[1][2] * B[2][0] + B[0][2] * B[1][0] * B[2][1] -
               B[2][0] * B[1][1] * B[0][2] - B[2][1] * B[1][2] * B[0][0] - B[2][2] * B[1][0] * B[0][1];
    }
}

// transformed gradient of basis function i at quadrature point q: g[d] = sum_d2 dphi[q][i][d2] Binv[d2][d]
template <int DIM, int NEN>
__device__ __forceinline__ void grad_t(const double* __restrict__ s_dphi, int q, int i, const double (&Binv)[DIM][DIM],
                                       double (&g)[DIM]) {
    const double* dp = s_dphi + (q * NEN + i) * DIM;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        double s = 0.0;
#pragma unroll
        for (int d2 = 0; d2 < DIM; ++d2) s += dp[d2] * Binv[d2][d];
        g[d] = s;
    }
}

}  // namespace
}  // namespace fedd
