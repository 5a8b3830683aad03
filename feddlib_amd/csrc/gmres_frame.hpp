// What gmres.hip (one-vector solvers, dispatcher) and gmres_sstep.hip (s-step solver) share: the row-block constants and loads
// of the basis sweeps, the layout of the scalars, the solve frame and the entry point of the s-step solver.  Kernels stay
// private to the file that launches them; Frame's member functions are defined in gmres.hip, and the s-step solver reaches
// the small one-vector kernels (k_reduce_cols, k_scale_to, k_backsolve, k_axpby, ...) through them.
#pragma once
#include "fedd_internal.hpp"

namespace fedd {

constexpr int MD_ROWS = 2048;  // rows per workgroup of the multi-dot (256 lanes x 4 x double2)
constexpr int MD_CG = 8;       // basis columns per workgroup of the multi-dot
constexpr int MD2_CG = 8;      // basis columns per workgroup of the two-vector multi-dot (16: 13 % slower)
constexpr int AX_ROWS = 512;   // rows per workgroup of the multi-axpy (256 lanes x double2)

// cached load for the work vectors (u, w): every column group of the multi-dot re-reads them
__device__ __forceinline__ double2 ld2c(const double* __restrict__ p, int64_t r, int64_t n) {
    if (r + 1 < n) return *reinterpret_cast<const double2*>(p + r);
    double2 v;
    v.x = r < n ? p[r] : 0.0;
    v.y = 0.0;
    return v;
}

__device__ __forceinline__ double2 ld2(const double* __restrict__ p, int64_t r, int64_t n) {
    // basis columns are streamed (each is read twice per iteration, 0.8 GB apart): non-temporal loads
    // keep them from displacing the vectors and the matrix in L2 / Infinity Cache (-1.5 ms per step)
    if (r + 1 < n) {
        typedef double v2d __attribute__((ext_vector_type(2)));
        const v2d t = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p + r));
        double2 v;
        v.x = t.x;
        v.y = t.y;
        return v;
    }
    double2 v;
    v.x = r < n ? p[r] : 0.0;
    v.y = 0.0;
    return v;
}

// scalars layout in d_small (doubles): see Frame::setup
struct Off {
    int H, cs, sn, g, h1, h2, nrm, y, misc;
};

// What the three solvers share, built once per solve: sizes, the layout of the scalars, the work vectors, the operator, the
// start, the solution update, the true residual and the tail.  A solver appends its own scalars behind `p` before alloc().
struct Frame {
    fedd_ctx* c;
    const GmresCall* a;
    // a->nr > 1: stacked vectors X[row * nr + j] (nr right-hand sides with one matrix: the GDSW extension solves); the
    // operator and the preconditioner are the stacked ones of multi.hip, everything else sees vectors nr times as long
    int nr;
    // tail: the work vectors carry room for the ghost entries behind the owned ones (several ranks): the halo import of an
    // operator input then goes straight into the vector, without a copy into a column-length buffer first
    bool tail, ghosts;
    int64_t n, ldv, nc;    // vector length, leading dimension of the basis (128-byte aligned columns), stride of the work vectors
    int m, nblk, nblk2;
    Off o;
    int p;                 // doubles of d_small taken so far
    double *S, *V, *w0, *w1, *z, *r;   // scalars, basis, two work vectors (w1 only with tail), M^-1 v, residual / V y
    dim3 gn, blk;
    hipStream_t st;
    // mk != nullptr: the constrained system  A^ = D A D + (I - D),  M^^-1 = D M^-1 D + (I - D)  with D = diag(mask): dofs
    // with mask 0 are held at the value the right-hand side gives them and decouple (the discrete harmonic extensions of
    // the GDSW coarse space: interface dofs held, interiors solved).  The inputs already carry D x = x wherever it
    // matters: in = D in + (I - D) in.
    const double* mk;
    bool project;          // every cycle starts from a coarse-orthogonal residual (coarse_project in gmres.hip)
    double beta0 = 0.0, relres = 0.0;
    int its = 0;

    int setup(fedd_ctx* ctx, const GmresCall& call, bool with_tail);
    int alloc(size_t part, bool block_kernels);
    // the launches of the small one-vector kernels that more than one solver makes
    void reduce_cols(int ncols, double* out, int nblk_part, const int32_t* gate = nullptr);   // out[col] = sum of its partials in d_part
    void first_basis_vector();                                                               // V_0 = r * S[misc + 1] (1 / beta)
    void backsolve(int cols);                                                                // S[y] = R^-1 g, cols columns
    int norm2(const double* v, double* out);
    int read_norm(double* out);
    int apply(const double* in, double* out, bool in_tail = false, double theta = 0.0);
    int residual(double* x, double* ax, bool x_tail, int use_compact);
    int start(double* ax, int use_compact);
    int add_correction(int cols, double* dst, bool combined = false);
    int true_residual(double* x, double* ax, bool x_tail, int use_compact, bool proj);
    void report(int* its_out, double* relres_out) const;
    int finish(int* its_out, double* relres_out);
};

// gmres_sstep.hip: the s-step solver (gmres_kind 2) with blocks of at most s vectors
int gmres_solve_sstep(fedd_ctx* c, const GmresCall& call, int s, int* its_out, double* relres_out);

}  // namespace fedd
