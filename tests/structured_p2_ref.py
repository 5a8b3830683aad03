"""numpy restatement of the reference's structured P2 generator (test infrastructure), loop for loop:
  MeshStructured::buildMesh2D, P2 branch   feddlib/core/Mesh/MeshStructured_def.hpp:468-619
  MeshStructured::buildMesh3D, P2 branch   feddlib/core/Mesh/MeshStructured_def.hpp:808-994
  setStructuredMeshFlags(1)                feddlib/core/Mesh/MeshStructured_def.hpp:2984-3011 (2D), :3137-3202 (3D)
  Map::buildUniqueMap                      feddlib/core/LinearAlgebra/Map_def.hpp:184-210, with this project's
                                           lowest-rank owner (the reference leaves the winner of its INSERT import open)
as Domain::buildMesh sequences them (feddlib/core/FE/Domain_def.hpp:201-265) on the unit square / cube.
Python floats are IEEE doubles and every expression keeps the reference's operation order, so coordinates are bit-equal."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)          # Teuchos::ScalarTraits<double>::eps()
COOR_REC = (0.0, 0.0, 0.0)
LENGTH = WIDTH = HEIGHT = 1.0

# lattice offsets from (2r, 2s) of the six slots of the two triangles of cell (r, s)   (:572-578, :590-596)
TRI_SLOTS = (
    ((2, 0), (0, 0), (2, 2), (1, 0), (1, 1), (2, 1)),
    ((0, 2), (0, 0), (2, 2), (0, 1), (1, 1), (1, 2)),
)
# lattice offsets from (2r, 2s, 2t) of the ten slots of the six tetrahedra of cell (r, s, t): +1 in s is the reference's
# "+P2M", +1 in t its "+P2M*P2M"   (:906-916, :920-930, :934-944, :948-958, :962-972, :976-986; slots listed 0..9)
TET_SLOTS = (
    ((2, 0, 0), (0, 0, 0), (2, 0, 2), (2, 2, 2), (1, 0, 0), (1, 0, 1), (2, 0, 1), (2, 1, 1), (1, 1, 1), (2, 1, 2)),
    ((0, 0, 2), (0, 0, 0), (2, 0, 2), (2, 2, 2), (0, 0, 1), (1, 0, 1), (1, 0, 2), (1, 1, 2), (1, 1, 1), (2, 1, 2)),
    ((2, 0, 0), (0, 0, 0), (2, 2, 0), (2, 2, 2), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 1, 1), (1, 1, 1), (2, 2, 1)),
    ((0, 0, 0), (0, 2, 0), (2, 2, 0), (2, 2, 2), (0, 1, 0), (1, 2, 0), (1, 1, 0), (1, 1, 1), (1, 2, 1), (2, 2, 1)),
    ((0, 0, 0), (0, 2, 0), (0, 2, 2), (2, 2, 2), (0, 1, 0), (0, 2, 1), (0, 1, 1), (1, 1, 1), (1, 2, 1), (1, 2, 2)),
    ((0, 0, 0), (0, 0, 2), (0, 2, 2), (2, 2, 2), (0, 0, 1), (0, 1, 2), (0, 1, 1), (1, 1, 1), (1, 1, 2), (1, 2, 2)),
)


def _offsets(rank, N, dim):
    """:482-487, :817-827"""
    offset_x = rank % N
    offset_y = 0
    offset_z = 0
    if (rank % (N * N)) >= N:
        offset_y = (rank % (N * N)) // N
    if dim == 3 and (rank % (N * N * N)) >= N * N:
        offset_z = (rank % (N * N * N)) // (N * N)
    return offset_x, offset_y, offset_z


def _snap(c, tol):
    return 0.0 if (c < tol and c > -tol) else c


def _repeated(dim, N, M, rank):
    """points, global ids and the generator's flag of the repeated points (:491-513, :832-862)"""
    h = LENGTH / (M * N)                        # :308, :648
    H = LENGTH / N                              # :309, :649
    n1 = N * (2 * (M + 1) - 1) - (N - 1)        # nmbPoints_oneDir, :325, :663
    P2M = 2 * (M + 1) - 1
    ox, oy, oz = _offsets(rank, N, dim)
    pts, gid, flag = [], [], []
    if dim == 2:
        tol = 100 * EPS
        for s in range(P2M):
            for r in range(P2M):
                x = _snap(r * h / 2.0 + ox * H, tol)
                y = _snap(s * h / 2.0 + oy * H, tol)
                gid.append(r + s * n1 + ox * (2 * (M + 1) - 2) + oy * n1 * (2 * (M + 1) - 2))                   # :504
                f = 0
                if (x > (COOR_REC[0] + LENGTH - tol) or x < (COOR_REC[0] + tol) or
                        y > (COOR_REC[1] + HEIGHT - tol) or y < (COOR_REC[1] + tol)):                            # :506-509
                    f = 1
                pts.append((x, y))
                flag.append(f)
    else:
        tol = EPS
        for t in range(P2M):
            for s in range(P2M):
                for r in range(P2M):
                    x = _snap(r * h / 2.0 + ox * H, tol)
                    y = _snap(s * h / 2.0 + oy * H, tol)
                    z = _snap(t * h / 2.0 + oz * H, tol)
                    gid.append(r + s * n1 + t * n1 * n1 + ox * (2 * (M + 1) - 2) + oy * n1 * (2 * (M + 1) - 2)
                               + oz * n1 * n1 * (2 * (M + 1) - 2))                                                # :849-850
                    f = 0
                    if (x > (COOR_REC[0] + LENGTH - tol) or x < (COOR_REC[0] + tol) or
                            y > (COOR_REC[1] + WIDTH - tol) or y < (COOR_REC[1] + tol) or
                            z > (COOR_REC[2] + HEIGHT - tol) or z < (COOR_REC[2] + tol)):                        # :852-856
                        f = 1
                    pts.append((x, y, z))
                    flag.append(f)
    return np.array(pts, dtype=np.float64), np.array(gid, dtype=np.int64), np.array(flag, dtype=np.int32)


def _flags1_2d(p, f):
    """:2985-2996 = :2999-3010, one point"""
    tol = 1.e-12
    if p[0] > (COOR_REC[0] - tol) and p[1] < (COOR_REC[1] + tol):
        f = 1
    if p[0] > (COOR_REC[0] - tol) and p[1] > (COOR_REC[1] + HEIGHT - tol):
        f = 1
    if p[0] > (COOR_REC[0] + LENGTH - tol) and p[1] > (COOR_REC[1] + tol) and p[1] < (COOR_REC[1] + HEIGHT - tol):
        f = 3
    if p[0] < (COOR_REC[0] + tol):
        f = 2
    return f


def _flags1_3d(p, f):
    """:3138-3168 = :3171-3201, one point"""
    tol = 1.e-12
    if p[0] < (COOR_REC[0] + tol):
        f = 2
    if p[0] > (COOR_REC[0] + tol) and p[2] < (COOR_REC[2] + tol):
        f = 1
    if p[0] > (COOR_REC[0] + tol) and p[2] > (COOR_REC[2] + HEIGHT - tol):
        f = 1
    if p[0] > (COOR_REC[0] + tol) and p[1] < (COOR_REC[1] + tol):
        f = 1
    if p[0] > (COOR_REC[0] + tol) and p[1] > (COOR_REC[1] + WIDTH - tol):
        f = 1
    if (p[0] > (COOR_REC[0] + LENGTH - tol) and p[1] > (COOR_REC[1] + tol) and p[1] < (COOR_REC[1] + WIDTH - tol)
            and p[2] > (COOR_REC[2] + tol) and p[2] < (COOR_REC[2] + HEIGHT - tol)):
        f = 3
    return f


def build(dim, N, M, rank, flags_option=1):
    """The rank's mesh: dict of conn, xyz, gid_rep, gid_uni, flag_rep, flag_uni, owner, eflag."""
    assert dim in (2, 3) and M >= 1 and 0 <= rank < N ** dim and flags_option in (0, 1)
    h = LENGTH / (M * N)
    n1 = N * (2 * (M + 1) - 1) - (N - 1)
    P2M = 2 * (M + 1) - 1
    xyz, gid_rep, flag_rep = _repeated(dim, N, M, rank)
    # buildUniqueMap: a node belongs to the lowest rank whose repeated map holds it
    owner_of_gid = {}
    for q in range(N ** dim - 1, -1, -1):
        for g in _repeated(dim, N, M, q)[1]:
            owner_of_gid[int(g)] = q
    owner = np.array([owner_of_gid[int(g)] for g in gid_rep], dtype=np.int32)
    mine = np.nonzero(owner == rank)[0]                       # Map_def.hpp:201-206: repeated order, filtered
    gid_uni = gid_rep[mine]
    flag_uni = np.zeros(mine.shape[0], dtype=np.int32)
    if dim == 2:
        xyz_uni = xyz[mine].copy()                            # :536-544: the repeated point and its flag
        flag_uni[:] = flag_rep[mine]
    else:
        xyz_uni = np.zeros((mine.shape[0], 3))
        for i, g in enumerate(gid_uni):                       # :871-887: recomputed from the global id
            g = int(g)
            x = _snap((g % n1) * h / 2, EPS)
            y = _snap((int((g % (n1 * n1)) // n1) + EPS) * h / 2, EPS)
            z = _snap((int(g // (n1 * n1) + EPS)) * h / 2, EPS)
            xyz_uni[i] = (x, y, z)
            if (x > (COOR_REC[0] + LENGTH - EPS) or x < (COOR_REC[0] + EPS) or
                    y > (COOR_REC[1] + WIDTH - EPS) or y < (COOR_REC[1] + EPS) or
                    z > (COOR_REC[2] + HEIGHT - EPS) or z < (COOR_REC[2] + EPS)):
                flag_uni[i] = 1
    # elements (:569-609, :902-992)
    conn, eflag = [], []
    if dim == 2:
        for s in range(M):
            for r in range(M):
                for tri in TRI_SLOTS:
                    el = [2 * r + a + P2M * (2 * s + b) for a, b in tri]
                    x_ref = (xyz[el[0]][0] + xyz[el[1]][0] + xyz[el[2]][0]) / 3.
                    y_ref = (xyz[el[0]][1] + xyz[el[1]][1] + xyz[el[2]][1]) / 3.
                    eflag.append(1 if (x_ref >= 0.3 and x_ref <= 0.7 and y_ref >= 0.6) else 0)     # :580-586
                    conn.append(el)
    else:
        for t in range(M):
            for s in range(M):
                for r in range(M):
                    for tet in TET_SLOTS:
                        conn.append([2 * r + a + P2M * (2 * s + b) + P2M * P2M * (2 * t + c) for a, b, c in tet])
                        eflag.append(0)                                                            # :813
    # setStructuredMeshFlags (Domain_def.hpp:263)
    if flags_option == 1:
        if dim == 2:
            for i in range(xyz_uni.shape[0]):
                flag_uni[i] = _flags1_2d(xyz_uni[i], flag_uni[i])
            for i in range(xyz.shape[0]):
                flag_rep[i] = _flags1_2d(xyz[i], flag_rep[i])
        else:
            for i in range(xyz_uni.shape[0]):
                flag_uni[i] = _flags1_3d(xyz_uni[i], flag_uni[i])
            for i in range(xyz_uni.shape[0]):                 # :3170: the repeated loop runs to pointsUni_->size()
                flag_rep[i] = _flags1_3d(xyz[i], flag_rep[i])
    return dict(conn=np.array(conn, dtype=np.int32), xyz=xyz, gid_rep=gid_rep, gid_uni=gid_uni, flag_rep=flag_rep,
                flag_uni=flag_uni, owner=owner, eflag=np.array(eflag, dtype=np.int32))
