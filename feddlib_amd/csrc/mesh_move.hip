// Moving mesh: new node coordinates for a mesh that is already on the device, one rank.  gfx950 only.
//
// Replaces Mesh::moveMesh (feddlib/core/Mesh/Mesh_def.hpp:297-330: x = x_ref + d on the repeated and the unique points) for the
// device copy of the coordinates, as Domain::moveMesh calls it in the ALE / FSI loops and in problems/tests/geometry/main.cpp:683.
// fedd_mesh_set* is the other way to give a context coordinates; it releases every per-mesh structure.  A move keeps all of
// them that do not depend on where the nodes lie (include/fedd_hip.h lists both sides; DESIGN.md section 4 "Moving mesh" goes
// through every cache of fedd_internal.hpp).
//
// Two kernels, and nothing is committed unless the second one finds every element the right way round:
//   k_mesh_move   candidate = x_ref + d, one addition in double per entry (Mesh_def.hpp:312), into a buffer of its own: a pure
//                 stream with 16-byte accesses over the entry pairs and one scalar tail entry, like k_newmark (24 bytes per entry)
//   k_move_check  one lane per element: det B of the candidate and of the reference element from the first dim + 1 nodes
//                 (FE::buildTransformation, the affine map every assembly kernel takes), both by affine_det; counts the elements
//                 with det * det_ref <= 0 (NaN included), takes the smallest such element and the smallest |det| / |det_ref| of
//                 the others.  Wave shuffles, then LDS, then per workgroup one integer atomic each for count and element
//                 (none when the workgroup found nothing) and one partial minimum; k_move_min folds the partials.  No
//                 floating-point atomic: the minimum is the same bits every time.
// On success the candidate and d_xyz change places, the coordinate copies at the head of the assembly's tile blobs are
// written again (assemble_tiles.hip tiles_refresh_coords) and system_written(SYS_GEOMETRY) drops what was laid over the old
// coordinates.  No product is fused with a sum in this file: the check can be restated bit for bit on the host.
#include "assemble_common.hpp"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace fedd {
namespace {

__global__ __launch_bounds__(256) void k_mesh_move(const double* __restrict__ ref, const double* __restrict__ disp,
                                                   double* __restrict__ out, int64_t n) {
    const int64_t n2 = n >> 1;
    const double2* __restrict__ r2 = reinterpret_cast<const double2*>(ref);
    const double2* __restrict__ d2 = reinterpret_cast<const double2*>(disp);
    double2* __restrict__ o2 = reinterpret_cast<double2*>(out);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
        const double2 a = r2[i], b = d2[i];
        o2[i] = make_double2(a.x + b.x, a.y + b.y);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = ref[n - 1] + disp[n - 1];
}

constexpr int MC_BS = 256;
constexpr int MC_MAXGRID = 2048;    // partial minima of k_move_check (k_move_min folds them in one workgroup)

// flags[0] += elements with det * det_ref <= 0, flags[1] = min(their ids); part[block] = smallest |det| / |det_ref| of the others
template <int DIM>
__global__ __launch_bounds__(MC_BS) void k_move_check(const int32_t* __restrict__ conn, int nen, const double* __restrict__ ref,
                                                      const double* __restrict__ cand, int64_t n_elem,
                                                      int32_t* __restrict__ flags, double* __restrict__ part) {
    __shared__ double s_min[MC_BS / 64];
    __shared__ int32_t s_cnt[MC_BS / 64], s_id[MC_BS / 64];
    double rmin = INFINITY;
    int32_t cnt = 0, id = INT32_MAX;
    for (int64_t e = (int64_t)blockIdx.x * MC_BS + threadIdx.x; e < n_elem; e += (int64_t)gridDim.x * MC_BS) {
        double X[DIM + 1][DIM], R[DIM + 1][DIM];
#pragma unroll
        for (int v = 0; v <= DIM; ++v) {
            const size_t nd = (size_t)conn[e * nen + v] * DIM;
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                X[v][d] = cand[nd + d];
                R[v][d] = ref[nd + d];
            }
        }
        const double det = affine_det<DIM>(X), det_ref = affine_det<DIM>(R);
        if (det * det_ref > 0.0) {
            rmin = fmin(rmin, fabs(det) / fabs(det_ref));
        } else {        // (a NaN lands here too)
            ++cnt;
            id = min(id, (int32_t)e);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        rmin = fmin(rmin, __shfl_xor(rmin, o, 64));
        cnt += __shfl_xor(cnt, o, 64);
        id = min(id, __shfl_xor(id, o, 64));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_min[w] = rmin;
        s_cnt[w] = cnt;
        s_id[w] = id;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < MC_BS / 64; ++k) {
            rmin = fmin(rmin, s_min[k]);
            cnt += s_cnt[k];
            id = min(id, s_id[k]);
        }
        part[blockIdx.x] = rmin;
        if (cnt > 0) {
            atomicAdd(&flags[0], cnt);
            atomicMin(&flags[1], id);
        }
    }
}

// second stage: out = { min of part[0, n), flags[0], flags[1] } (the two integers as doubles: one copy to the host)
__global__ __launch_bounds__(MC_BS) void k_move_min(const double* __restrict__ part, int n, const int32_t* __restrict__ flags,
                                                    double* __restrict__ out) {
    __shared__ double s_min[MC_BS / 64];
    double rmin = INFINITY;
    for (int i = threadIdx.x; i < n; i += MC_BS) rmin = fmin(rmin, part[i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) rmin = fmin(rmin, __shfl_xor(rmin, o, 64));
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = rmin;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < MC_BS / 64; ++k) rmin = fmin(rmin, s_min[k]);
        out[0] = rmin;
        out[1] = (double)flags[0];
        out[2] = (double)flags[1];
    }
}

double host_det(int dim, const double* X) {     // affine_det on the host, for the error text
    double B[3][3];
    for (int j = 0; j < dim; ++j)
        for (int i = 0; i < dim; ++i) B[i][j] = X[(j + 1) * dim + i] - X[i];
    if (dim == 2) return B[0][0] * B[1][1] - B[1][0] * B[0][1];
    return B[0][0] * B[1][1] * B[2][2] + B[0][1] * B[1][2] * B[2][0] + B[0][2] * B[1][0] * B[2][1] -
           B[2][0] * B[1][1] * B[0][2] - B[2][1] * B[1][2] * B[0][0] - B[2][2] * B[1][0] * B[0][1];
}

// det / det_ref of one element, read back from the device (the error path only)
int element_ratio(fedd_ctx* c, int64_t e, const double* d_cand, double* ratio) {
    const int dim = c->dim;
    int32_t nodes[4];
    double X[12], R[12];
    FEDD_HIP(hipMemcpy(nodes, c->d_conn.p + e * c->nen, (size_t)(dim + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int v = 0; v <= dim; ++v) {
        FEDD_HIP(hipMemcpy(X + v * dim, d_cand + (size_t)nodes[v] * dim, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost));
        FEDD_HIP(hipMemcpy(R + v * dim, c->d_xyz_ref.p + (size_t)nodes[v] * dim, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost));
    }
    *ratio = host_det(dim, X) / host_det(dim, R);
    return 0;
}

}  // namespace

int mesh_move(fedd_ctx* c, const double* disp_rep) {
    FEDD_CHECK(c->nranks == 1, "fedd_mesh_move: one rank only for now (this context is rank %d of %d)", c->rank, c->nranks);
    const int dim = c->dim;
    const int64_t n = c->n_node * dim;
    hipStream_t st = c->stream;
    if (!c->have_xref) {    // until the first move d_xyz IS the reference
        FEDD_TRY(c->d_xyz_ref.ensure((size_t)n));
        FEDD_HIP(hipMemcpyAsync(c->d_xyz_ref.p, c->d_xyz.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
        c->have_xref = true;
    }
    FEDD_TRY(c->d_xyz_cand.ensure((size_t)n));
    double ratio = 1.0;
    if (!disp_rep) {        // back to the reference: a copy (x_ref + 0.0 would turn a -0.0 into +0.0), nothing to check
        FEDD_HIP(hipMemcpyAsync(c->d_xyz_cand.p, c->d_xyz_ref.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    } else {
        const size_t n_rep = c->h_col_of_rep.size();
        std::vector<double>& d = c->h_mv_disp;     // a member, not a local: an error between the copy below and the synchronise leaves the stream reading it
        d.assign((size_t)n, 0.0);
        for (size_t i = 0; i < n_rep; ++i)
            for (int k = 0; k < dim; ++k) d[(size_t)c->h_col_of_rep[i] * dim + k] = disp_rep[i * dim + k];
        FEDD_TRY(c->d_mv_disp.ensure((size_t)n));
        const int grid_c = (int)std::min<int64_t>(MC_MAXGRID, std::max<int64_t>(1, (c->n_elem + MC_BS - 1) / MC_BS));
        FEDD_TRY(c->d_mv_part.ensure((size_t)MC_MAXGRID + 4));
        FEDD_TRY(c->d_mv_flag.ensure(2));
        double* d_out = c->d_mv_part.p + MC_MAXGRID;
        static const int32_t flag0[2] = {0, INT32_MAX};
        FEDD_HIP(hipMemcpyAsync(c->d_mv_disp.p, d.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        FEDD_HIP(hipMemcpyAsync(c->d_mv_flag.p, flag0, sizeof(flag0), hipMemcpyHostToDevice, st));
        {
            ScopedTimer t(c, FEDD_T_MESH_MOVE);
            t.bytes(24.0 * (double)n);
            const unsigned grid = (unsigned)std::min<int64_t>(2048, std::max<int64_t>(1, ((n >> 1) + 255) / 256));
            hipLaunchKernelGGL(k_mesh_move, dim3(grid), dim3(256), 0, st, (const double*)c->d_xyz_ref.p, (const double*)c->d_mv_disp.p,
                               c->d_xyz_cand.p, n);
        }
        {
            ScopedTimer t(c, FEDD_T_MOVE_CHECK);
            // dim + 1 node ids per element, every coordinate of both sets once (the gathers of neighbouring elements share lines)
            t.bytes(4.0 * (dim + 1) * (double)c->n_elem + 16.0 * (double)n);
            if (dim == 3)
                hipLaunchKernelGGL(k_move_check<3>, dim3(grid_c), dim3(MC_BS), 0, st, (const int32_t*)c->d_conn.p, c->nen,
                                   (const double*)c->d_xyz_ref.p, (const double*)c->d_xyz_cand.p, c->n_elem, c->d_mv_flag.p, c->d_mv_part.p);
            else
                hipLaunchKernelGGL(k_move_check<2>, dim3(grid_c), dim3(MC_BS), 0, st, (const int32_t*)c->d_conn.p, c->nen,
                                   (const double*)c->d_xyz_ref.p, (const double*)c->d_xyz_cand.p, c->n_elem, c->d_mv_flag.p, c->d_mv_part.p);
            hipLaunchKernelGGL(k_move_min, dim3(1), dim3(MC_BS), 0, st, (const double*)c->d_mv_part.p, grid_c,
                               (const int32_t*)c->d_mv_flag.p, d_out);
        }
        FEDD_HIP(hipGetLastError());
        double h_out[3] = {0, 0, 0};
        FEDD_HIP(hipMemcpyAsync(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost, st));
        FEDD_HIP(hipStreamSynchronize(st));     // (`h_out` is a local)
        if (h_out[1] > 0.0) {
            const int64_t e = (int64_t)h_out[2];
            double r = 0.0;
            FEDD_TRY(element_ratio(c, e, c->d_xyz_cand.p, &r));
            set_error("fedd_mesh_move: element %lld is inverted or degenerate under this displacement (det B / det B_ref = %.6g; "
                      "%lld such elements); nothing was moved", (long long)e, r, (long long)h_out[1]);
            return 1;
        }
        ratio = c->n_elem > 0 ? h_out[0] : 1.0;
    }
    // ---- commit ----
    std::swap(c->d_xyz.p, c->d_xyz_cand.p);
    std::swap(c->d_xyz.cap, c->d_xyz_cand.cap);
    FEDD_TRY(tiles_refresh_coords(c));
    system_written(c, SYS_GEOMETRY);
    ++c->n_moves;
    c->min_det_ratio = ratio;
    return 0;
}

int mesh_coords_get(fedd_ctx* c, double* xyz_rep) {
    const int dim = c->dim;
    std::vector<double> x((size_t)c->n_node * dim);
    FEDD_HIP(hipStreamSynchronize(c->stream));
    FEDD_HIP(hipMemcpy(x.data(), c->d_xyz.p, x.size() * sizeof(double), hipMemcpyDeviceToHost));
    const size_t n_rep = c->h_col_of_rep.size();
    for (size_t i = 0; i < n_rep; ++i)
        for (int k = 0; k < dim; ++k) xyz_rep[i * dim + k] = x[(size_t)c->h_col_of_rep[i] * dim + k];
    return 0;
}

}  // namespace fedd
