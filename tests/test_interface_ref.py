"""The numpy restatement of the interface distances, the element coefficient and the scaled element loop
(tests/interface_ref.py) has the known answers and the properties of the form.  No GPU."""
import numpy as np
import pytest

import fedd_oracle as fo
import interface_ref as ir
import stress_ref as sr

CASES = [(2, "p1", 3), (2, "p2", 3), (3, "p1", 2), (3, "p2", 2)]
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mesh(lib, dim, fe, M):
    key = (dim, fe, M)
    if key not in _cache:
        m = sr.jitter(lib.structured_mesh(dim, 1, M))
        _cache[key] = lib.p2_of_p1(m, volume_id=0) if fe == "p2" else m
    return _cache[key]


def oracle_mesh(m):
    return fo.Mesh(dim=m["dim"], fe="P1" if m["conn"].shape[1] == m["dim"] + 1 else "P2", conn=m["conn"], xyz=m["xyz"],
                   gid_rep=m["gid_rep"], flag_rep=m["flag_rep"], gid_uni=m["gid_uni"], flag_uni=m["flag_uni"], xyz_uni=None,
                   n_global=m["n_global"])


@pytest.mark.parametrize("M", [5, 7, 10])
def test_distance_to_the_side_x0_of_a_structured_square_is_x_bit_for_bit(fedd_lib, M):
    """the nearest interface point has the node's own y, so the sum of squares is fl(x * x) + 0.0, and the correctly rounded
    root of fl(x * x) is x"""
    m = fedd_lib.structured_mesh(2, 1, M)
    side = ir.interface_nodes(m, 2)
    assert side.shape[0] == M + 1 and np.all(m["xyz"][side, 0] == 0.0)
    d = ir.distances_to_flags(m, 2)
    assert np.array_equal(bits(d), bits(m["xyz"][:, 0]))
    assert np.all(d[side] == 0.0)


def test_cap_and_empty_interface(fedd_lib):
    m = fedd_lib.structured_mesh(2, 1, 3)
    n = m["xyz"].shape[0]
    assert np.array_equal(ir.distances(m["xyz"], np.zeros((0, 2))), np.full(n, 1000.0))
    assert np.array_equal(ir.distances_to_flags(m, 77), np.full(n, 1000.0))
    far = np.array([[5000.0, 0.0], [0.0, -2000.0]])
    assert np.array_equal(ir.distances(m["xyz"], far), np.full(n, 1000.0))
    # one point inside the cap, one outside: the inner one decides, the cap does not touch it
    d = ir.distances(m["xyz"], np.array([[5000.0, 0.0], [300.0, 400.0]]))
    assert np.all(d < 1000.0) and abs(d[np.argmin(np.abs(m["xyz"]).sum(axis=1))] - 500.0) < 1e-12


def test_distances_do_not_depend_on_the_order_of_the_points(fedd_lib):
    m = sr.jitter(fedd_lib.structured_mesh(3, 1, 3))
    rng = np.random.default_rng(3)
    pts = rng.uniform(-0.5, 1.5, (37, 3))
    a, b = ir.distances(m["xyz"], pts), ir.distances(m["xyz"], pts[rng.permutation(37)])
    assert np.array_equal(bits(a), bits(b))


def test_strict_less_at_mean_equal_distance(fedd_lib):
    m = fedd_lib.structured_mesh(2, 1, 2)
    dist = np.full(m["xyz"].shape[0], 0.75)                      # (0.75 + 0.75 + 0.75) / 3.0 = 0.75 exactly
    assert np.all(ir.element_means(m, dist) == 0.75)
    assert np.all(ir.coefficients(m, dist, 0.75, 50.0) == 1.0)   # mean == distance: not scaled
    assert np.all(ir.coefficients(m, dist, np.nextafter(0.75, 1.0), 50.0) == 50.0)
    assert np.all(ir.coefficients(m, dist, 0.0, 50.0) == 1.0)


@pytest.mark.parametrize("dim", [2, 3])
def test_p2_mid_edge_distances_do_not_enter(fedd_lib, dim):
    m = mesh(fedd_lib, dim, "p2", 2)
    n = m["xyz"].shape[0]
    vertex = np.zeros(n, dtype=bool)
    vertex[np.unique(m["conn"][:, :dim + 1])] = True
    assert not vertex.all()
    dist = np.where(vertex, 0.5, 1e-6)                  # the mid-edge nodes alone are close
    assert np.all(ir.coefficients(m, dist, 0.1, 9.0) == 1.0)
    dist2 = np.where(vertex, 1e-6, 0.5)
    assert np.all(ir.coefficients(m, dist2, 0.1, 9.0) == 9.0)


@pytest.mark.parametrize("dim,fe,M", CASES)
def test_matrix_symmetric_rows_sum_to_zero_and_f_one_is_the_vector_laplacian(fedd_lib, dim, fe, M):
    m = mesh(fedd_lib, dim, fe, M)
    E = m["conn"].shape[0]
    dist = ir.distances_to_flags(m, 2)
    f = ir.coefficients(m, dist, 0.4, 37.5)
    assert 0 < np.count_nonzero(f == 37.5) < E          # a mix of scaled and unscaled elements
    K = ir.assemble(m, f)
    assert abs(K - K.T).max() <= 1e-14 * abs(K).max()
    assert np.abs(K @ np.ones(K.shape[0])).max() <= 1e-13 * np.abs(K).sum(axis=1).max()
    # DIAG pattern: component a couples with component a only
    coo = K.tocoo()
    assert np.all(coo.row % dim == coo.col % dim)
    K1, L = ir.assemble(m, np.ones(E)), fo.assembly_laplace_vecfield(oracle_mesh(m))
    K1.sort_indices(); L.sort_indices()
    assert np.array_equal(K1.indptr, L.indptr) and np.array_equal(K1.indices, L.indices)
    assert abs(K1 - L).max() <= 1e-10 * abs(L).max()
    # the coefficient scales its element's contribution: K(f) - K(1) is (c - 1) x the scaled elements' part
    Kc = ir.assemble(m, np.where(f == 37.5, 1.0, 0.0))
    assert abs((K - K1) - 36.5 * Kc).max() <= 1e-12 * abs(K).max()
