// Interface distances and the element coefficient of the scaled-Laplace mesh extension, one rank.  gfx950 only.
//
// Replaces Domain::calculateDistancesToInterface (feddlib/core/FE/Domain_def.hpp:568-648) and the loop at the end of
// MeshInterface::buildMeshInterfaceParallelAndDistance (feddlib/core/Mesh/MeshInterface_def.hpp:473-491): for every node of
// the repeated map the distance to the nearest interface point, capped at 1000.0 -- an all-pairs minimum -- and the
// coefficient HeuristicScaling (feddlib/problems/specific/Geometry_def.hpp:24-34) gives an element in
// FE::assemblyLaplaceXDim (feddlib/core/FE/FE_def.hpp:2273-2278, 2343-2349).
//
//   k_interface_distance  one lane per mesh node, its coordinates in registers.  The interface points are staged through LDS in
//                 tiles of ID_TILE points, structure-of-arrays (one array per coordinate), by all lanes of the workgroup,
//                 coalesced from the structure-of-arrays copy the host uploaded.  In the pair loop every lane of a wave reads
//                 the same LDS address: a broadcast, no bank conflict.  Per pair: dim subtractions, dim products and dim - 1
//                 sums, each rounded on its own (fp contract(off): no product is fused with a sum), the squares summed in
//                 ascending k, and a minimum of the SQUARED distances in a register.  One sqrt and one store per node: the
//                 correctly rounded sqrt is monotone, so sqrt(min d^2) has the bits of min sqrt(d^2), and a minimum does not
//                 depend on the order of the points or on the tiling.  No atomics.
//                 LDS: ID_TILE * dim * 8 bytes = 24 KiB in 3D, 16 KiB in 2D, per workgroup of ID_BS = 256 lanes: six (ten)
//                 workgroups fit the 160 KiB of a compute unit, so the 32-wave cap of the compute unit (eight such workgroups),
//                 not the LDS, bounds the occupancy in 2D and the LDS leaves 24 of 32 waves in 3D -- a compute-bound loop of
//                 independent lanes needs no more.  A longer tile saves nothing (the two barriers per tile are already spread
//                 over 1024 pairs per lane), a shorter one only adds barriers.
//   k_laplace_scale  one lane per element: mean of the distances of its first dim + 1 nodes, summed left to right and divided
//                 by 3.0 / 4.0, f = coefficient where mean < distance (strict), else 1.0.
#include "fedd_internal.hpp"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace fedd {
namespace {

constexpr int ID_BS = 256;
constexpr int ID_TILE = 1024;       // interface points per LDS tile (fedd_interface_distance_info reports it)

// pts: structure-of-arrays, coordinate k of point j at pts[k * np + j]
template <int DIM>
__global__ __launch_bounds__(ID_BS) void k_interface_distance(const double* __restrict__ xyz, int64_t n_node,
                                                              const double* __restrict__ pts, int64_t np,
                                                              double* __restrict__ dist) {
    __shared__ double s_p[DIM][ID_TILE];
    const int64_t i = (int64_t)blockIdx.x * ID_BS + threadIdx.x;
    const bool on = i < n_node;
    double x[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) x[k] = on ? xyz[i * DIM + k] : 0.0;
    double m2 = INFINITY;
    for (int64_t t0 = 0; t0 < np; t0 += ID_TILE) {      // (np is uniform over the grid: so are the barriers)
        const int n = np - t0 < ID_TILE ? (int)(np - t0) : ID_TILE;
        for (int j = threadIdx.x; j < n; j += ID_BS)
#pragma unroll
            for (int k = 0; k < DIM; ++k) s_p[k][j] = pts[(int64_t)k * np + t0 + j];
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < n; ++j) {
            double d2 = 0.0;
#pragma unroll
            for (int k = 0; k < DIM; ++k) {
                const double t = x[k] - s_p[k][j];
                d2 = k == 0 ? t * t : d2 + t * t;
            }
            m2 = fmin(m2, d2);
        }
        __syncthreads();        // the next tile overwrites s_p
    }
    if (on) dist[i] = fmin(1000.0, sqrt(m2));
}

template <int DIM>
__global__ __launch_bounds__(256) void k_laplace_scale(const int32_t* __restrict__ conn, int nen, const double* __restrict__ dist,
                                                       int64_t n_elem, double distance, double coefficient,
                                                       double* __restrict__ f) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elem) return;
    double s = dist[conn[e * nen]];
#pragma unroll
    for (int v = 1; v <= DIM; ++v) s = s + dist[conn[e * nen + v]];
    const double mean = s / (DIM == 2 ? 3.0 : 4.0);
    f[e] = mean < distance ? coefficient : 1.0;
}

// the all-pairs minimum against the n_pts points of h_pts (structure-of-arrays, [dim][n_pts]) on the coordinates in force
int distance_run(fedd_ctx* c, int64_t n_pts, const std::vector<double>& h_pts) {
    const int dim = c->dim;
    hipStream_t st = c->stream;
    FEDD_TRY(c->d_idist.ensure((size_t)c->n_node));
    FEDD_TRY(c->d_ipts.ensure((size_t)std::max<int64_t>(1, n_pts * dim)));
    if (n_pts > 0) {
        FEDD_HIP(hipMemcpyAsync(c->d_ipts.p, h_pts.data(), (size_t)(n_pts * dim) * sizeof(double), hipMemcpyHostToDevice, st));
        FEDD_HIP(hipStreamSynchronize(st));     // (`h_pts` is the caller's)
    }
    const unsigned grid = (unsigned)((c->n_node + ID_BS - 1) / ID_BS);
    {
        ScopedTimer t(c, FEDD_T_INTERFACE_DIST);
        // every coordinate once, one distance per node; the points are read once per workgroup (from L2 after the first)
        t.bytes((double)c->n_node * (dim + 1) * 8.0 + (double)n_pts * dim * 8.0);
        if (dim == 3)
            hipLaunchKernelGGL(k_interface_distance<3>, dim3(grid), dim3(ID_BS), 0, st, (const double*)c->d_xyz.p, c->n_node,
                               (const double*)c->d_ipts.p, n_pts, c->d_idist.p);
        else
            hipLaunchKernelGGL(k_interface_distance<2>, dim3(grid), dim3(ID_BS), 0, st, (const double*)c->d_xyz.p, c->n_node,
                               (const double*)c->d_ipts.p, n_pts, c->d_idist.p);
    }
    FEDD_HIP(hipGetLastError());
    c->have_idist = true;
    c->n_interface = n_pts;
    return 0;
}

}  // namespace

int interface_distance_tile() { return ID_TILE; }

int interface_distance_points(fedd_ctx* c, int64_t n_pts, const double* xyz_pts) {
    FEDD_CHECK(c->nranks == 1, "fedd_interface_distance_points: one rank only (a context with %d ranks was given)", c->nranks);
    const int dim = c->dim;
    std::vector<double> pts((size_t)(n_pts * dim));
    for (int64_t j = 0; j < n_pts; ++j)
        for (int k = 0; k < dim; ++k) pts[(size_t)(k * n_pts + j)] = xyz_pts[j * dim + k];
    return distance_run(c, n_pts, pts);
}

int interface_distance_flags(fedd_ctx* c, int n_flags, const int32_t* flags, int64_t* n_interface) {
    FEDD_CHECK(c->nranks == 1, "fedd_interface_distance: one rank only (a context with %d ranks was given)", c->nranks);
    const int dim = c->dim;
    // the nodes that carry a flag: the owned ones and the row ghosts (one rank: every node), in column-local numbering
    const int64_t nf = c->n_own + c->n_rowg;
    std::vector<int32_t> nflag((size_t)nf);
    std::vector<double> x((size_t)c->n_node * dim);
    FEDD_HIP(hipStreamSynchronize(c->stream));
    if (nf > 0) FEDD_HIP(hipMemcpy(nflag.data(), c->d_flag.p, (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost));
    FEDD_HIP(hipMemcpy(x.data(), c->d_xyz.p, x.size() * sizeof(double), hipMemcpyDeviceToHost));   // the coordinates in force
    std::vector<int64_t> ids;
    for (int64_t i = 0; i < nf; ++i)
        if (std::find(flags, flags + n_flags, nflag[(size_t)i]) != flags + n_flags) ids.push_back(i);
    const int64_t n_pts = (int64_t)ids.size();
    std::vector<double> pts((size_t)(n_pts * dim));
    for (int64_t j = 0; j < n_pts; ++j)
        for (int k = 0; k < dim; ++k) pts[(size_t)(k * n_pts + j)] = x[(size_t)ids[(size_t)j] * dim + k];
    FEDD_TRY(distance_run(c, n_pts, pts));
    if (n_interface) *n_interface = n_pts;
    return 0;
}

int interface_distance_set(fedd_ctx* c, const double* dist_rep) {
    FEDD_CHECK(c->nranks == 1, "fedd_interface_distance_set: one rank only (a context with %d ranks was given)", c->nranks);
    c->n_interface = 0;
    if (!dist_rep) {
        FEDD_HIP(hipStreamSynchronize(c->stream));      // a kernel in flight may read the buffer
        c->d_idist.release();
        c->have_idist = false;
        return 0;
    }
    std::vector<double> d((size_t)c->n_node, 1000.0);
    const size_t n_rep = c->h_col_of_rep.size();
    for (size_t i = 0; i < n_rep; ++i) d[(size_t)c->h_col_of_rep[i]] = dist_rep[i];
    FEDD_TRY(c->d_idist.ensure((size_t)c->n_node));
    FEDD_HIP(hipMemcpyAsync(c->d_idist.p, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FEDD_HIP(hipStreamSynchronize(c->stream));  // (`d` is a local)
    c->have_idist = true;
    return 0;
}

int interface_distance_get(fedd_ctx* c, double* dist_rep) {
    FEDD_CHECK(c->nranks == 1, "fedd_interface_distance_get: one rank only (a context with %d ranks was given)", c->nranks);
    FEDD_CHECK(c->have_idist, "fedd_interface_distance_get: no distances (fedd_interface_distance, fedd_interface_distance_points "
                              "or fedd_interface_distance_set first)");
    std::vector<double> d((size_t)c->n_node);
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_HIP(hipMemcpy(d.data(), c->d_idist.p, d.size() * sizeof(double), hipMemcpyDeviceToHost));
    const size_t n_rep = c->h_col_of_rep.size();
    for (size_t i = 0; i < n_rep; ++i) dist_rep[i] = d[(size_t)c->h_col_of_rep[i]];
    return 0;
}

// f per element into c->d_lscale, in the stream (the assembly that follows reads it there)
int laplace_scale(fedd_ctx* c, double distance, double coefficient) {
    FEDD_TRY(c->d_lscale.ensure((size_t)std::max<int64_t>(1, c->n_elem)));
    if (c->n_elem > 0) {
        const unsigned grid = (unsigned)((c->n_elem + 255) / 256);
        if (c->dim == 3)
            hipLaunchKernelGGL(k_laplace_scale<3>, dim3(grid), dim3(256), 0, c->stream, (const int32_t*)c->d_conn.p, c->nen,
                               (const double*)c->d_idist.p, c->n_elem, distance, coefficient, c->d_lscale.p);
        else
            hipLaunchKernelGGL(k_laplace_scale<2>, dim3(grid), dim3(256), 0, c->stream, (const int32_t*)c->d_conn.p, c->nen,
                               (const double*)c->d_idist.p, c->n_elem, distance, coefficient, c->d_lscale.p);
        FEDD_HIP(hipGetLastError());
    }
    c->have_lscale = true;
    return 0;
}

int laplace_scale_get(fedd_ctx* c, double* f_elem) {
    FEDD_CHECK(c->have_lscale, "fedd_laplace_scale_get: no fedd_assemble(FEDD_FORM_LAPLACE_XDIM) on this mesh yet");
    FEDD_HIP(hipStreamSynchronize(c->stream));
    if (c->n_elem > 0) FEDD_HIP(hipMemcpy(f_elem, c->d_lscale.p, (size_t)c->n_elem * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace fedd
