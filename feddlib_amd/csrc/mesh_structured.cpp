// Host-side structured P1 mesh generator (square / cube, Kuhn split) of the product path.
//
// Follows the behaviour of the reference generator, not its code:
//   MeshStructured::buildMesh2D P1 branch   feddlib/core/Mesh/MeshStructured_def.hpp:348-463
//   MeshStructured::buildMesh3D P1 branch   feddlib/core/Mesh/MeshStructured_def.hpp:703-806
//   setStructuredMeshFlags(1)               feddlib/core/Mesh/MeshStructured_def.hpp:2974-3203
//   Map::buildUniqueMap                     feddlib/core/LinearAlgebra/Map_def.hpp:184-210
// and, at the end of the file, the structured P2 lattice (no ghost layers):
//   MeshStructured::buildMesh2D P2 branch   feddlib/core/Mesh/MeshStructured_def.hpp:468-619
//   MeshStructured::buildMesh3D P2 branch   feddlib/core/Mesh/MeshStructured_def.hpp:808-994
// Layout differences: flat SoA arrays instead of vector<vector<>>, per-direction block counts
// (the reference only knows N x N x N), optional ghost-element layers, lowest-rank owner rule.
// Ghost layers L: 0 = the reference's block; 1 = plus the layer of cells above the block that completes the
// rows of the owned nodes; L >= 2 = L layers of cells around the owned nodes on every side that has a
// neighbour, which completes the rows of the ghost nodes within L - 1 layers as well ("row ghosts": the
// Schwarz local matrices then hold true rows for nodes that belong to other ranks).
#include "fedd_internal.hpp"
#include <algorithm>
#include <cmath>
#include <limits>

namespace {

struct Block {
    int dim;
    int N[3], M[3], off[3];
    int up[3];        // ghost lattice planes above the block in d (0 .. L, clipped to the grid)
    int dn[3];        // planes below (0 .. L - 1, clipped to the grid)
    int mode;         // L
    int lo_owned[3];  // first owned lattice index in d (0, or 1 when a lower neighbour owns the face)
    int64_t P[3];     // global points per direction
    int n1[3];        // own lattice points per direction (M+1)
    int ne[3];        // extended lattice points per direction (dn + M+1 + up)
};

int make_block(int dim, const int* decomp, const int* cells, int rank, int ghosts, Block& b) {
    b.dim = dim;
    b.mode = ghosts;
    if (ghosts < 0 || ghosts > 8) {
        fedd::set_error("structured mesh: %d ghost layers (0 .. 8)", ghosts);
        return 1;
    }
    int64_t nr = 1;
    for (int d = 0; d < 3; ++d) {
        b.N[d] = d < dim ? decomp[d] : 1;
        b.M[d] = d < dim ? cells[d] : 0;
        if (d < dim && (b.N[d] < 1 || b.M[d] < 1)) {
            fedd::set_error("structured mesh: decomp and cells must be >= 1 (H/h is too small)");
            return 1;
        }
        nr *= b.N[d];
    }
    if (rank < 0 || rank >= nr) {
        fedd::set_error("structured mesh: rank %d outside decomposition of %lld blocks", rank, (long long)nr);
        return 1;
    }
    // rank -> block offsets: x fastest (MeshStructured_def.hpp:712-722)
    b.off[0] = rank % b.N[0];
    b.off[1] = (rank / b.N[0]) % b.N[1];
    b.off[2] = rank / (b.N[0] * b.N[1]);
    for (int d = 0; d < 3; ++d) {
        b.P[d] = d < dim ? (int64_t)b.N[d] * b.M[d] + 1 : 1;
        b.n1[d] = d < dim ? b.M[d] + 1 : 1;
        // planes above: L, below: L - 1 (the lower neighbour owns the shared face), clipped to the grid
        const int64_t above = d < dim ? (int64_t)(b.N[d] - 1 - b.off[d]) * b.M[d] : 0;
        const int64_t below = d < dim ? (int64_t)b.off[d] * b.M[d] : 0;
        b.up[d] = (int)std::min<int64_t>(ghosts, above);
        b.dn[d] = (int)std::min<int64_t>(ghosts > 1 ? ghosts - 1 : 0, below);
        b.ne[d] = b.dn[d] + b.n1[d] + b.up[d];
        b.lo_owned[d] = (d < dim && b.off[d] > 0) ? 1 : 0;
    }
    return 0;
}

// lattice indices run over [-dn, M + up] per direction (0 .. M = the reference's own block)
inline bool in_own_lattice(const Block& b, int r, int s, int t) {
    return r >= 0 && r < b.n1[0] && s >= 0 && s < b.n1[1] && t >= 0 && t < b.n1[2];
}
// the nodes whose rows are complete with L >= 2 layers: both cells around the plane are present (or the
// plane is on the boundary of the grid) in every direction
inline bool in_row_box(const Block& b, int r, int s, int t) {
    const int l[3] = {r, s, t};
    for (int d = 0; d < b.dim; ++d) {
        const int64_t gl = (int64_t)l[d] + (int64_t)b.off[d] * b.M[d];   // global plane index
        const bool lo_ok = gl == 0 || l[d] - 1 >= -b.dn[d];
        const bool hi_ok = gl == b.P[d] - 1 || l[d] <= b.M[d] + b.up[d] - 1;
        if (!lo_ok || !hi_ok || l[d] < -b.dn[d] || l[d] > b.M[d] + b.up[d]) return false;
    }
    return true;
}

// local repeated id of lattice point (r,s,t): the reference's (M+1)^dim block first in its own order
// (r fastest), then the extra points of the first plane above the block, then (mode 2) the outer layer,
// each class in extended-lattice order.
struct Numbering {
    const Block& b;
    std::vector<int32_t> ext_id;  // only for points outside the own lattice
    int64_t n_own_lattice;
    int64_t n_first = 0;          // extra points of the first class
    explicit Numbering(const Block& blk) : b(blk) {
        n_own_lattice = (int64_t)b.n1[0] * b.n1[1] * b.n1[2];
        ext_id.assign((size_t)b.ne[0] * b.ne[1] * b.ne[2], -1);
        int32_t next = (int32_t)n_own_lattice;
        for (int cls = 0; cls < 2; ++cls) {
            for (int t = -b.dn[2]; t < b.n1[2] + b.up[2]; ++t)
                for (int s = -b.dn[1]; s < b.n1[1] + b.up[1]; ++s)
                    for (int r = -b.dn[0]; r < b.n1[0] + b.up[0]; ++r) {
                        if (in_own_lattice(b, r, s, t)) continue;
                        if ((cls == 0) != in_row_box(b, r, s, t)) continue;
                        ext_id[slot(r, s, t)] = next++;
                    }
            if (cls == 0) n_first = next - n_own_lattice;
        }
        n_rep = next;
    }
    int64_t n_rep = 0;
    size_t slot(int r, int s, int t) const {
        return ((size_t)(t + b.dn[2]) * b.ne[1] + (size_t)(s + b.dn[1])) * b.ne[0] + (size_t)(r + b.dn[0]);
    }
    int32_t id(int r, int s, int t) const {
        if (in_own_lattice(b, r, s, t)) return (int32_t)(r + (int64_t)b.n1[0] * (s + (int64_t)b.n1[1] * t));
        return ext_id[slot(r, s, t)];
    }
};

// Kuhn split of a cell into 6 tets, corner offsets in the reference's order
// (MeshStructured_def.hpp:772-801), and the 2 triangles of a 2D cell (:431-446).
const int KUHN[6][4][3] = {
    {{1, 0, 0}, {0, 0, 0}, {1, 0, 1}, {1, 1, 1}}, {{0, 0, 1}, {0, 0, 0}, {1, 0, 1}, {1, 1, 1}},
    {{1, 0, 0}, {0, 0, 0}, {1, 1, 0}, {1, 1, 1}}, {{0, 0, 0}, {0, 1, 0}, {1, 1, 0}, {1, 1, 1}},
    {{0, 0, 0}, {0, 1, 0}, {0, 1, 1}, {1, 1, 1}}, {{0, 0, 0}, {0, 0, 1}, {0, 1, 1}, {1, 1, 1}}};
const int TRIS[2][3][2] = {{{1, 0}, {0, 0}, {1, 1}}, {{0, 1}, {0, 0}, {1, 1}}};

inline bool owned_pt(const Block& b, int r, int s, int t) {
    return r >= b.lo_owned[0] && r < b.n1[0] && s >= b.lo_owned[1] && s < b.n1[1] &&
           t >= b.lo_owned[2] && t < b.n1[2];
}

// visit every element: own cells first in the reference order, then the ghost cells that touch an owned
// point (mode 1) or a point of the row box (mode 2)
template <class F>
void for_each_element(const Block& b, F&& f) {
    const int dim = b.dim;
    const int nsub = dim == 3 ? 6 : 2;
    for (int pass = 0; pass < 2; ++pass) {
        const int t0 = pass ? -b.dn[2] : 0, t1 = dim == 3 ? b.M[2] + (pass ? b.up[2] : 0) : 1;
        const int s0 = pass ? -b.dn[1] : 0, s1 = b.M[1] + (pass ? b.up[1] : 0);
        const int r0 = pass ? -b.dn[0] : 0, r1 = b.M[0] + (pass ? b.up[0] : 0);
        for (int t = t0; t < t1; ++t)
            for (int s = s0; s < s1; ++s)
                for (int r = r0; r < r1; ++r) {
                    const bool ghost_cell = r < 0 || s < 0 || t < 0 || r >= b.M[0] || s >= b.M[1] || (dim == 3 && t >= b.M[2]);
                    if ((pass == 0) == ghost_cell) continue;
                    for (int k = 0; k < nsub; ++k) {
                        int pr[4], ps[4], pt[4];
                        bool touches = false;
                        for (int v = 0; v <= dim; ++v) {
                            if (dim == 3) {
                                pr[v] = r + KUHN[k][v][0];
                                ps[v] = s + KUHN[k][v][1];
                                pt[v] = t + KUHN[k][v][2];
                            } else {
                                pr[v] = r + TRIS[k][v][0];
                                ps[v] = s + TRIS[k][v][1];
                                pt[v] = 0;
                            }
                            touches = touches || (b.mode >= 2 ? in_row_box(b, pr[v], ps[v], pt[v])
                                                              : owned_pt(b, pr[v], ps[v], pt[v]));
                        }
                        if (ghost_cell && !touches) continue;
                        f(pr, ps, pt, ghost_cell);
                    }
                }
    }
}

int32_t flags_option1(int dim, const double* p, int32_t f, const double* o, const double* sz) {
    const double tol = 1.0e-12;  // MeshStructured_def.hpp:2976
    const double x = p[0], y = p[1];
    if (dim == 2) {  // :2984-2998, later tests override earlier ones
        if (x > o[0] - tol && y < o[1] + tol) f = 1;
        if (x > o[0] - tol && y > o[1] + sz[1] - tol) f = 1;
        if (x > o[0] + sz[0] - tol && y > o[1] + tol && y < o[1] + sz[1] - tol) f = 3;
        if (x < o[0] + tol) f = 2;
        return f;
    }
    const double z = p[2];  // :3136-3167
    if (x < o[0] + tol) f = 2;
    const bool in = x > o[0] + tol;
    if (in && z < o[2] + tol) f = 1;
    if (in && z > o[2] + sz[2] - tol) f = 1;
    if (in && y < o[1] + tol) f = 1;
    if (in && y > o[1] + sz[1] - tol) f = 1;
    if (x > o[0] + sz[0] - tol && y > o[1] + tol && y < o[1] + sz[1] - tol && z > o[2] + tol &&
        z < o[2] + sz[2] - tol)
        f = 3;
    return f;
}

}  // namespace

extern "C" int fedd_mesh_structured_sizes(int dim, const int* decomp, const int* cells, int rank,
                                          int with_ghost_elements, int64_t* n_elem, int64_t* n_rep,
                                          int64_t* n_uni, int64_t* n_global) {
    FEDD_CHECK(dim == 2 || dim == 3, "structured mesh: dimension must be 2 or 3");
    Block b;
    FEDD_TRY(make_block(dim, decomp, cells, rank, with_ghost_elements, b));
    int64_t ne = 0;
    for_each_element(b, [&](const int*, const int*, const int*, bool) { ++ne; });
    int64_t nrep = (int64_t)b.n1[0] * b.n1[1] * b.n1[2];
    int64_t ext = (int64_t)b.ne[0] * b.ne[1] * b.ne[2] - nrep;
    int64_t nuni = 1;
    for (int d = 0; d < dim; ++d) nuni *= b.n1[d] - b.lo_owned[d];
    if (n_elem) *n_elem = ne;
    if (n_rep) *n_rep = nrep + ext;
    if (n_uni) *n_uni = nuni;
    if (n_global) *n_global = b.P[0] * b.P[1] * b.P[2];
    return 0;
}

extern "C" int fedd_mesh_structured_build(int dim, const int* decomp, const int* cells, int rank,
                                          const double* origin, const double* size, int flags_option,
                                          int with_ghost_elements, int32_t* conn, double* xyz,
                                          int64_t* gid_rep, int32_t* flag_rep, int64_t* gid_uni,
                                          int32_t* flag_uni) {
    FEDD_CHECK(dim == 2 || dim == 3, "structured mesh: dimension must be 2 or 3");
    FEDD_CHECK(flags_option == 0 || flags_option == 1, "structured mesh: flags option %d not supported", flags_option);
    Block b;
    FEDD_TRY(make_block(dim, decomp, cells, rank, with_ghost_elements, b));
    Numbering num(b);
    double o[3] = {0, 0, 0}, sz[3] = {1, 1, 1}, h[3] = {0, 0, 0}, H[3] = {0, 0, 0};
    for (int d = 0; d < dim; ++d) {
        if (origin) o[d] = origin[d];
        if (size) sz[d] = size[d];
        h[d] = sz[d] / (b.M[d] * b.N[d]);  // :646 h = length/(M*N)
        H[d] = sz[d] / b.N[d];             // :647
    }
    const double eps = std::numeric_limits<double>::epsilon();
    const double snap = dim == 3 ? eps : 100 * eps;  // :727-734 vs :371-374
    int64_t nu = 0;
    for (int t = -b.dn[2]; t < b.n1[2] + b.up[2]; ++t)
        for (int s = -b.dn[1]; s < b.n1[1] + b.up[1]; ++s)
            for (int r = -b.dn[0]; r < b.n1[0] + b.up[0]; ++r) {
                const int32_t id = num.id(r, s, t);
                const int l[3] = {r, s, t};
                double p[3] = {0, 0, 0};
                int64_t g[3] = {0, 0, 0};
                for (int d = 0; d < dim; ++d) {
                    // a point beyond the own lattice gets the coordinate its owning block computes
                    int ll = l[d], oo = b.off[d];
                    while (ll >= b.n1[d]) {
                        ll -= b.M[d];
                        oo += 1;
                    }
                    while (ll < 0) {
                        ll += b.M[d];
                        oo -= 1;
                    }
                    double c = ll * h[d] + oo * H[d];
                    if (c < snap && c > -snap) c = 0.0;
                    p[d] = c;
                    g[d] = (int64_t)l[d] + (int64_t)b.off[d] * b.M[d];
                    xyz[(int64_t)id * dim + d] = c;
                }
                gid_rep[id] = g[0] + b.P[0] * (g[1] + b.P[1] * g[2]);  // :736-737
                int32_t f = 0;
                for (int d = 0; d < dim; ++d)  // :739-744
                    if (p[d] > o[d] + sz[d] - snap || p[d] < o[d] + snap) f = 1;
                if (flags_option == 1) f = flags_option1(dim, p, f, o, sz);
                if (flag_rep) flag_rep[id] = f;
            }
    // unique list: repeated (own-lattice) order filtered by ownership (Map_def.hpp:201-206)
    for (int t = 0; t < b.n1[2]; ++t)
        for (int s = 0; s < b.n1[1]; ++s)
            for (int r = 0; r < b.n1[0]; ++r) {
                if (!owned_pt(b, r, s, t)) continue;
                const int32_t id = num.id(r, s, t);
                gid_uni[nu] = gid_rep[id];
                if (flag_uni) {
                    int32_t f = 0;
                    double p[3] = {0, 0, 0};
                    for (int d = 0; d < dim; ++d) p[d] = xyz[(int64_t)id * dim + d];
                    for (int d = 0; d < dim; ++d)
                        if (p[d] > o[d] + sz[d] - snap || p[d] < o[d] + snap) f = 1;
                    if (flags_option == 1) f = flags_option1(dim, p, f, o, sz);
                    flag_uni[nu] = f;
                }
                ++nu;
            }
    int64_t e = 0;
    const int nen = dim + 1;
    for_each_element(b, [&](const int* pr, const int* ps, const int* pt, bool) {
        for (int v = 0; v < nen; ++v) conn[e * nen + v] = num.id(pr[v], ps[v], pt[v]);
        ++e;
    });
    return 0;
}

/* L >= 2 ghost layers: the repeated-map nodes whose matrix rows are complete on this rank although another
 * rank owns them (the ghost nodes within L - 1 layers of the owned ones): count, or with arrays their
 * global ids and boundary flags -- the arguments of fedd_mesh_set_rows. */
extern "C" int fedd_mesh_structured_row_ghosts(int dim, const int* decomp, const int* cells, int rank,
                                               int with_ghost_elements, const double* origin, const double* size,
                                               int flags_option, int64_t* n_out, int64_t* gid, int32_t* flag) {
    FEDD_CHECK(dim == 2 || dim == 3, "structured mesh: dimension must be 2 or 3");
    FEDD_CHECK(with_ghost_elements >= 2, "structured mesh: row ghosts need at least 2 ghost layers");
    Block b;
    FEDD_TRY(make_block(dim, decomp, cells, rank, with_ghost_elements, b));
    double o[3] = {0, 0, 0}, sz[3] = {1, 1, 1}, h[3] = {0, 0, 0}, H[3] = {0, 0, 0};
    for (int d = 0; d < dim; ++d) {
        if (origin) o[d] = origin[d];
        if (size) sz[d] = size[d];
        h[d] = sz[d] / (b.M[d] * b.N[d]);
        H[d] = sz[d] / b.N[d];
    }
    const double eps = std::numeric_limits<double>::epsilon();
    const double snap = dim == 3 ? eps : 100 * eps;
    int64_t n = 0;
    for (int t = -b.dn[2]; t < b.n1[2] + b.up[2]; ++t)
        for (int s = -b.dn[1]; s < b.n1[1] + b.up[1]; ++s)
            for (int r = -b.dn[0]; r < b.n1[0] + b.up[0]; ++r) {
                if (owned_pt(b, r, s, t) || !in_row_box(b, r, s, t)) continue;
                if (gid || flag) {
                    const int l[3] = {r, s, t};
                    double p[3] = {0, 0, 0};
                    int64_t g[3] = {0, 0, 0};
                    for (int d = 0; d < dim; ++d) {
                        int ll = l[d], oo = b.off[d];
                        while (ll >= b.n1[d]) {
                            ll -= b.M[d];
                            oo += 1;
                        }
                        while (ll < 0) {
                            ll += b.M[d];
                            oo -= 1;
                        }
                        double c = ll * h[d] + oo * H[d];
                        if (c < snap && c > -snap) c = 0.0;
                        p[d] = c;
                        g[d] = (int64_t)l[d] + (int64_t)b.off[d] * b.M[d];
                    }
                    if (gid) gid[n] = g[0] + b.P[0] * (g[1] + b.P[1] * g[2]);
                    if (flag) {
                        int32_t f = 0;
                        for (int d = 0; d < dim; ++d)
                            if (p[d] > o[d] + sz[d] - snap || p[d] < o[d] + snap) f = 1;
                        if (flags_option == 1) f = flags_option1(dim, p, f, o, sz);
                        flag[n] = f;
                    }
                }
                ++n;
            }
    if (n_out) *n_out = n;
    return 0;
}

// Boundary faces of the rank's structured mesh, ghost elements included: every (dim-1)-face of a local element whose
// vertices all lie on one side of the square / cube.  The reference builds no sub-elements for its structured meshes
// (MeshStructured::buildSurfaceLinesSquare, MeshStructured_def.hpp:230-238, is an empty body), so the flag rule is this
// library's: a face carries the flag setStructuredMeshFlags gives to the nodes strictly inside its side -- flags_option 0: 1
// everywhere; flags_option 1: 2 on x = origin, 3 on x = origin + size, 1 on the other sides.  Decided on lattice indices,
// not on coordinates.  Faces in element order, vertex ids (local repeated) ascending within a face.
namespace {
template <class F>
void for_each_boundary_face(const Block& b, int flags_option, F&& f) {
    const int dim = b.dim;
    const unsigned all = (1u << (dim + 1)) - 1;
    for_each_element(b, [&](const int* pr, const int* ps, const int* pt, bool) {
        for (int d = 0; d < dim; ++d) {
            // the vertices of the element on the lower / upper side in direction d, as bit masks: interior elements leave here
            unsigned on[2] = {0, 0};
            for (int v = 0; v <= dim; ++v) {
                const int64_t g = (int64_t)(d == 0 ? pr[v] : (d == 1 ? ps[v] : pt[v])) + (int64_t)b.off[d] * b.M[d];
                if (g == 0) on[0] |= 1u << v;
                if (g == b.P[d] - 1) on[1] |= 1u << v;
            }
            for (int side = 0; side < 2; ++side)
                for (int skip = 0; skip <= dim; ++skip)
                    if ((on[side] | (1u << skip)) == all) f(pr, ps, pt, skip, flags_option == 1 && d == 0 ? (side ? 3 : 2) : 1);
        }
    });
}
}  // namespace

extern "C" int fedd_mesh_structured_surfaces_sizes(int dim, const int* decomp, const int* cells, int rank,
                                                   int with_ghost_elements, int64_t* n_surf) {
    FEDD_CHECK(dim == 2 || dim == 3, "structured mesh: dimension must be 2 or 3");
    FEDD_CHECK(n_surf, "fedd_mesh_structured_surfaces_sizes: null output");
    Block b;
    FEDD_TRY(make_block(dim, decomp, cells, rank, with_ghost_elements, b));
    int64_t n = 0;
    for_each_boundary_face(b, 0, [&](const int*, const int*, const int*, int, int) { ++n; });
    *n_surf = n;
    return 0;
}

extern "C" int fedd_mesh_structured_surfaces(int dim, const int* decomp, const int* cells, int rank, int flags_option,
                                             int with_ghost_elements, int32_t* surf, int32_t* sflag) {
    FEDD_CHECK(dim == 2 || dim == 3, "structured mesh: dimension must be 2 or 3");
    FEDD_CHECK(flags_option == 0 || flags_option == 1, "structured mesh: flags option %d not supported", flags_option);
    Block b;
    FEDD_TRY(make_block(dim, decomp, cells, rank, with_ghost_elements, b));
    Numbering num(b);
    int64_t n = 0;
    for_each_boundary_face(b, flags_option, [&](const int* pr, const int* ps, const int* pt, int skip, int flag) {
        int32_t ids[3];
        int k = 0;
        for (int v = 0; v <= dim; ++v)
            if (v != skip) ids[k++] = num.id(pr[v], ps[v], pt[v]);
        for (int i = 1; i < dim; ++i)
            for (int j = i; j > 0 && ids[j - 1] > ids[j]; --j) std::swap(ids[j - 1], ids[j]);
        if (surf)
            for (int i = 0; i < dim; ++i) surf[n * dim + i] = ids[i];
        if (sflag) sflag[n] = flag;
        ++n;
    });
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Structured P2 lattice: 6-node triangles / 10-node tetrahedra on the (2M+1)^dim points of a block.
//   MeshStructured::buildMesh2D P2 branch   MeshStructured_def.hpp:468-619
//   MeshStructured::buildMesh3D P2 branch   MeshStructured_def.hpp:808-994
//   setStructuredMeshFlags(1) on P2 meshes  MeshStructured_def.hpp:2984-3011 (2D), :3137-3202 (3D)
// A lattice point (r,s,t) of the block has local id r + s*P2M + t*P2M^2, P2M = 2M+1 (:491-492, :832-834).  The vertices of
// an element are the P1 vertices at doubled indices and every mid node is the lattice point half-way between its two
// vertices; the slots the reference writes out one by one (:572-596, :906-986) are (0,1),(1,2),(0,2) in 2D and
// (0,1),(1,2),(0,2),(0,3),(1,3),(2,3) in 3D for every one of the 2 / 6 elements of a cell.
namespace {

struct BlockP2 {
    Block b;          // the P1 block of the same decomp / cells, no ghosts
    int p2m[3];       // lattice points per direction, 2M+1 (1 beyond dim)
    int64_t P2[3];    // global lattice points per direction, 2NM+1
};

int make_block_p2(int dim, const int* decomp, const int* cells, int rank, BlockP2& q) {
    if (make_block(dim, decomp, cells, rank, 0, q.b)) return 1;
    for (int d = 0; d < 3; ++d) {
        q.p2m[d] = d < dim ? 2 * (q.b.M[d] + 1) - 1 : 1;                                              // :563, :899
        q.P2[d] = d < dim ? (int64_t)q.b.N[d] * q.p2m[d] - (q.b.N[d] - 1) : 1;                        // :325, :663
    }
    return 0;
}

inline int32_t p2_id(const BlockP2& q, int r, int s, int t) {
    return (int32_t)(r + (int64_t)q.p2m[0] * (s + (int64_t)q.p2m[1] * t));
}

// (make_block sets lo_owned to 0 in the directions beyond dim, where the only index is 0)
inline bool p2_owned(const BlockP2& q, int r, int s, int t) {
    return r >= q.b.lo_owned[0] && s >= q.b.lo_owned[1] && t >= q.b.lo_owned[2];
}

const int P2_EDGE[6][2] = {{0, 1}, {1, 2}, {0, 2}, {0, 3}, {1, 3}, {2, 3}};

// the generator's own flag: 1 on the sides of the square / cube (:506-509, :852-856)
inline int32_t box_flag(int dim, const double* p, double snap) {
    for (int d = 0; d < dim; ++d)
        if (p[d] > 0.0 + 1.0 - snap || p[d] < 0.0 + snap) return 1;
    return 0;
}

}  // namespace

extern "C" int fedd_mesh_structured_p2_sizes(int dim, const int* decomp, const int* cells, int rank, int64_t* n_rep,
                                             int64_t* n_uni, int64_t* n_elem) {
    FEDD_CHECK(dim == 2 || dim == 3, "structured P2 mesh: dimension must be 2 or 3");
    BlockP2 q;
    FEDD_TRY(make_block_p2(dim, decomp, cells, rank, q));
    int64_t nrep = 1, nuni = 1, ne = dim == 3 ? 6 : 2;
    for (int d = 0; d < dim; ++d) {
        nrep *= q.p2m[d];
        nuni *= q.p2m[d] - q.b.lo_owned[d];
        ne *= q.b.M[d];
    }
    if (n_rep) *n_rep = nrep;
    if (n_uni) *n_uni = nuni;
    if (n_elem) *n_elem = ne;
    return 0;
}

extern "C" int fedd_mesh_structured_p2_build(int dim, const int* decomp, const int* cells, int rank, int flags_option,
                                             double* xyz, int64_t* gid_rep, int64_t* gid_uni, int32_t* owner,
                                             int32_t* bcflag_rep, int32_t* bcflag_uni, int32_t* conn, int32_t* eflag) {
    FEDD_CHECK(dim == 2 || dim == 3, "structured P2 mesh: dimension must be 2 or 3");
    FEDD_CHECK(flags_option == 0 || flags_option == 1, "structured P2 mesh: flags option %d not supported", flags_option);
    FEDD_CHECK(xyz && gid_rep && gid_uni && bcflag_rep && bcflag_uni && conn, "fedd_mesh_structured_p2_build: null output");
    BlockP2 q;
    FEDD_TRY(make_block_p2(dim, decomp, cells, rank, q));
    const Block& b = q.b;
    const double o[3] = {0, 0, 0}, sz[3] = {1, 1, 1};   // coorRec and length / width / height of "Square"
    double h[3] = {0, 0, 0}, H[3] = {0, 0, 0};
    for (int d = 0; d < dim; ++d) {
        h[d] = sz[d] / (b.M[d] * b.N[d]);  // :308, :648
        H[d] = sz[d] / b.N[d];             // :309, :649
    }
    const double eps = std::numeric_limits<double>::epsilon();
    const double snap = dim == 3 ? eps : 100 * eps;  // :843-847 vs :500-502
    int64_t n_uni = 1;
    for (int d = 0; d < dim; ++d) n_uni *= q.p2m[d] - b.lo_owned[d];
    // repeated points, r fastest (:491-513, :832-862)
    for (int t = 0; t < q.p2m[2]; ++t)
        for (int s = 0; s < q.p2m[1]; ++s)
            for (int r = 0; r < q.p2m[0]; ++r) {
                const int32_t id = p2_id(q, r, s, t);
                const int l[3] = {r, s, t};
                double p[3] = {0, 0, 0};
                int64_t g[3] = {0, 0, 0};
                int ob[3] = {0, 0, 0};
                for (int d = 0; d < dim; ++d) {
                    double c = l[d] * h[d] / 2.0 + b.off[d] * H[d];  // :499, :842
                    if (c < snap && c > -snap) c = 0.0;
                    p[d] = c;
                    xyz[(int64_t)id * dim + d] = c;
                    g[d] = (int64_t)l[d] + (int64_t)b.off[d] * (q.p2m[d] - 1);  // :504, :849-850
                    ob[d] = b.off[d] - (l[d] == 0 && b.off[d] > 0 ? 1 : 0);    // the lower neighbour owns the shared plane
                }
                gid_rep[id] = g[0] + q.P2[0] * (g[1] + q.P2[1] * g[2]);
                if (owner) owner[id] = ob[0] + b.N[0] * (ob[1] + b.N[1] * ob[2]);
                int32_t f = box_flag(dim, p, snap);
                // 3D: the reference's loop over the repeated points stops at the number of unique points (:3170), so the
                // repeated points beyond it keep the generator's flag
                if (flags_option == 1 && (dim == 2 || id < n_uni)) f = flags_option1(dim, p, f, o, sz);
                bcflag_rep[id] = f;
            }
    // unique list: repeated order filtered by ownership (Map_def.hpp:201-206)
    int64_t nu = 0;
    for (int t = 0; t < q.p2m[2]; ++t)
        for (int s = 0; s < q.p2m[1]; ++s)
            for (int r = 0; r < q.p2m[0]; ++r) {
                if (!p2_owned(q, r, s, t)) continue;
                const int32_t id = p2_id(q, r, s, t);
                const int64_t gid = gid_rep[id];
                gid_uni[nu] = gid;
                double p[3] = {0, 0, 0};
                if (dim == 2) {  // :541-543: the repeated point and its flag
                    p[0] = xyz[(int64_t)id * 2];
                    p[1] = xyz[(int64_t)id * 2 + 1];
                } else {  // :872-879: the unique points are computed from the global id
                    p[0] = (gid % q.P2[0]) * h[0] / 2;
                    p[1] = ((int)((gid % (q.P2[0] * q.P2[1])) / q.P2[0]) + eps) * h[1] / 2;
                    p[2] = ((int)(gid / (q.P2[0] * q.P2[1]) + eps)) * h[2] / 2;
                    for (int d = 0; d < 3; ++d)
                        if (p[d] < eps && p[d] > -eps) p[d] = 0.0;
                }
                int32_t f = box_flag(dim, p, snap);  // :543, :881-886
                if (flags_option == 1) f = flags_option1(dim, p, f, o, sz);
                bcflag_uni[nu] = f;
                ++nu;
            }
    // elements: the cells r fastest, 2 / 6 elements per cell in the P1 order (:569-609, :902-992)
    const int nv = dim + 1, nen = dim == 3 ? 10 : 6, nsub = dim == 3 ? 6 : 2;
    int64_t e = 0;
    for (int t = 0; t < (dim == 3 ? b.M[2] : 1); ++t)
        for (int s = 0; s < b.M[1]; ++s)
            for (int r = 0; r < b.M[0]; ++r)
                for (int k = 0; k < nsub; ++k, ++e) {
                    int v[4][3];
                    for (int a = 0; a < nv; ++a)
                        for (int d = 0; d < 3; ++d) {
                            const int c = d == 0 ? r : (d == 1 ? s : t);
                            v[a][d] = d < dim ? 2 * (c + (dim == 3 ? KUHN[k][a][d] : TRIS[k][a][d])) : 0;
                        }
                    int32_t* ce = conn + e * nen;
                    for (int a = 0; a < nv; ++a) ce[a] = p2_id(q, v[a][0], v[a][1], v[a][2]);
                    for (int m = 0; m < nen - nv; ++m) {
                        const int* va = v[P2_EDGE[m][0]];
                        const int* vb = v[P2_EDGE[m][1]];
                        ce[nv + m] = p2_id(q, (va[0] + vb[0]) / 2, (va[1] + vb[1]) / 2, (va[2] + vb[2]) / 2);
                    }
                    if (eflag) {
                        int32_t ef = 0;
                        if (dim == 2) {  // :580-586: the reference marks a patch of the square by the vertex centroid
                            const double x_ref = (xyz[2 * (int64_t)ce[0]] + xyz[2 * (int64_t)ce[1]] + xyz[2 * (int64_t)ce[2]]) / 3.;
                            const double y_ref = (xyz[2 * (int64_t)ce[0] + 1] + xyz[2 * (int64_t)ce[1] + 1] + xyz[2 * (int64_t)ce[2] + 1]) / 3.;
                            if (x_ref >= 0.3 && x_ref <= 0.7 && y_ref >= 0.6) ef = 1;
                        }
                        eflag[e] = ef;
                    }
                }
    return 0;
}

/* Permutation of the local repeated nodes of the structured P2 mesh that puts the P1 lattice nodes (all indices even)
 * first, in the order fedd_mesh_structured_build numbers the P1 mesh of the same decomp / cells; the other nodes follow in
 * their reference order.  perm[new] = reference local id.  The device layer takes "pressure = the first n_p1 node ids". */
extern "C" int fedd_mesh_p2_vertices_first(int dim, const int* decomp, const int* cells, int rank, int32_t* perm,
                                           int64_t* n_p1) {
    FEDD_CHECK(dim == 2 || dim == 3, "structured P2 mesh: dimension must be 2 or 3");
    BlockP2 q;
    FEDD_TRY(make_block_p2(dim, decomp, cells, rank, q));
    int64_t n = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int t = 0; t < q.p2m[2]; ++t)
            for (int s = 0; s < q.p2m[1]; ++s)
                for (int r = 0; r < q.p2m[0]; ++r) {
                    const bool p1 = r % 2 == 0 && s % 2 == 0 && t % 2 == 0;  // :494, :836
                    if ((pass == 0) != p1) continue;
                    if (perm) perm[n] = p2_id(q, r, s, t);
                    ++n;
                }
        if (pass == 0 && n_p1) *n_p1 = n;
    }
    return 0;
}
