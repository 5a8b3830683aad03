"""The numpy restatement of P(w) (tests/ale_ref.py) checked by itself, without a GPU and without an oracle: identities that
follow from the formula alone, on meshes with a distorted geometry."""
import numpy as np
import pytest

from ale_ref import AleRestatement, degree_P
from test_gpu_distorted import check_mesh, distorted
from test_navier_stokes_abi import degrees


def _mesh(fedd_lib, which):
    dim = 2 if which.startswith("square") else 3
    m = distorted(fedd_lib.structured_mesh(dim, 1, 3), 0.15, "all", seed=7)
    check_mesh(m)
    return fedd_lib.p2_of_p1(m, volume_id=0) if which.endswith("p2") else m


@pytest.mark.parametrize("which", ["square_p1", "cube_p1", "square_p2", "cube_p2"])
def test_restatement_of_P(fedd_lib, which):
    m = _mesh(fedd_lib, which)
    dim, x = m["dim"], m["xyz"]
    R = AleRestatement(fedd_lib, m)
    rng = np.random.default_rng(17)
    G, c0 = rng.standard_normal((dim, dim)), rng.standard_normal(dim)
    M = R.mass_vec_P()
    scale = abs(M).max()
    # affine field w = G x + c lies in the element space; div w_h = tr(G) everywhere: P = tr(G) * vector mass matrix
    w = (x @ G.T + c0[None, :]).ravel()
    P = R.P(w)
    assert np.array_equal(P.indptr, M.indptr) and np.array_equal(P.indices, M.indices)
    # rounding of div w_h: nen * dim products of |w| <= dim |G| + |c| with gradients of size <= 3 / h_min, h_min about 0.2 here:
    # 30 * 2^-53 * 15, a few 1e-14 per unit of |w|, on entries of size `scale`
    wmax = dim * np.abs(G).max() + np.abs(c0).max()
    assert np.abs(P.data - np.trace(G) * M.data).max() <= 1e-12 * wmax * scale
    # constant field: zero to rounding (the gradients of the basis sum to zero)
    wc = np.tile(c0, x.shape[0])
    assert np.abs(R.P(wc).data).max() <= 1e-12 * np.abs(c0).max() * scale
    # symmetric for any w, and on the diagonal component pairs only
    ws = np.sin(x @ G.T + c0[None, :]).ravel()
    Ps = R.P(ws)
    assert abs(Ps - Ps.T).max() <= 1e-14 * abs(Ps).max()
    rows = np.repeat(np.arange(Ps.shape[0]), np.diff(Ps.indptr))
    assert np.all(Ps.data[(rows % dim) != (Ps.indices % dim)] == 0.0)
    assert abs(Ps).max() > 0.0


@pytest.mark.parametrize("dim,nen", [(2, 3), (2, 6), (3, 4), (3, 10)])
def test_rule_of_P_is_the_rule_of_W(fedd_lib, dim, nen):
    """determineDegree(dim, FE, FE, Std, Std, determineDegree(dim, FE, Grad)): 1 + 1 + 1 for P1 (the inner degree 0 is raised
    to 1), 2 + 2 + 1 for P2 -- the rule the advection path stages for W, and a rule the library has"""
    assert degree_P(dim, nen) == degrees(dim, nen)[1] == (1 + 1 + 1 if nen == dim + 1 else 2 + 2 + 1)
    pts, w = fedd_lib.fe_quadrature(dim, degree_P(dim, nen))
    # (the tabulated weights carry 15 digits: the bound of test_quadrature_rules_are_exact_to_their_degree)
    assert pts.shape[0] == w.shape[0] > 0 and abs(w.sum() - (0.5 if dim == 2 else 1.0 / 6.0)) <= 1e-14 / (2 if dim == 2 else 6)
