"""The closed-form materials of tests/hyperelastic_ref.py (which the device kernels restate) against what the reference's
generated routines return (tests/golden/hyperelastic_materials.npz, written by tests/golden/make_hyperelastic_fixture.py), and
the properties every hyperelastic law has."""
import os

import numpy as np
import pytest

import hyperelastic_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10        # the project's parity bar
KEYS = {"nh3d": (hr.NEOHOOKE, 2), "mr3d": (hr.MOONEY_RIVLIN, 3), "stvk3d": (hr.STVK, 2), "stvk2d": (hr.STVK, 2)}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "hyperelastic_materials.npz"))


def rotation(dim, a, b=0.0):
    R = np.eye(dim)
    R[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    if dim == 3:
        R2 = np.eye(3)
        R2[1:, 1:] = [[np.cos(b), -np.sin(b)], [np.sin(b), np.cos(b)]]
        R = R2 @ R
    return R


@pytest.mark.parametrize("key", sorted(KEYS))
def test_closed_forms_match_the_generated_routines(gold, key):
    """A and P within 1e-10 of their largest entry.  At the identity and at rotations P is zero by construction and the
    routines return the rounding of terms of the size of the moduli: there, and only there, the scale is the largest entry of A
    (stress per unit strain)."""
    model, npar = KEYS[key]
    n = gold[key + "_F"].shape[0]
    assert n >= 36 and np.linalg.det(gold[key + "_F"]).min() > 0.2
    assert np.unique(gold[key + "_params"], axis=0).shape[0] == 2
    worst_p = worst_a = 0.0
    for par, F, P, A in zip(gold[key + "_params"], gold[key + "_F"], gold[key + "_P"], gold[key + "_A"]):
        P2, A2 = hr.material(model, par[:npar], F)
        worst_a = max(worst_a, np.abs(A2 - A).max() / np.abs(A).max())
        unstrained = np.abs(F.T @ F - np.eye(F.shape[0])).max() <= 1e-14          # identity, rotations: P = 0 by construction
        worst_p = max(worst_p, np.abs(P2 - P).max() / (np.abs(A).max() if unstrained else np.abs(P).max()))
    print("%s: P %.2e, A %.2e" % (key, worst_p, worst_a))
    assert worst_a <= RTOL and worst_p <= RTOL


CASES = [(hr.NEOHOOKE, (3.0e6, 0.4), 3), (hr.MOONEY_RIVLIN, (3.0e6, 0.4, 0.35), 3), (hr.STVK, hr.stvk_params(2.0e6, 0.4), 3),
         (hr.STVK, hr.stvk_params(2.0e6, 0.4), 2)]


@pytest.mark.parametrize("model,params,dim", CASES)
def test_tangent_is_major_symmetric_and_the_derivative_of_the_stress(model, params, dim):
    rng = np.random.default_rng(5)
    for _ in range(5):
        F = np.eye(dim) + 0.2 * rng.uniform(-1, 1, (dim, dim))
        P, A = hr.material(model, params, F)
        assert np.abs(A - A.transpose(2, 3, 0, 1)).max() <= 1e-14 * np.abs(A).max()
        h = 1e-6
        for k in range(dim):
            for l in range(dim):
                dF = np.zeros((dim, dim)); dF[k, l] = h
                fd = (hr.material(model, params, F + dF)[0] - hr.material(model, params, F - dF)[0]) / (2 * h)
                assert np.abs(fd - A[:, :, k, l]).max() <= 1e-7 * np.abs(A).max()


@pytest.mark.parametrize("model,params,dim", CASES)
def test_no_stress_under_rotations(model, params, dim):
    for a, b in ((0.0, 0.0), (0.7, 0.0), (2.1, 1.9), (-1.0, 0.3)):
        P, A = hr.material(model, params, rotation(dim, a, b))
        assert np.abs(P).max() <= 1e-14 * np.abs(A).max()
    P, _ = hr.material(model, params, np.eye(dim))
    assert np.all(P == 0.0)                                 # exactly: every bracket of the closed forms vanishes at the identity


@pytest.mark.parametrize("model,params,dim", [c for c in CASES if c[0] != hr.MOONEY_RIVLIN])
def test_tangent_at_the_identity_is_linear_elasticity(model, params, dim):
    lam, mu = params if model == hr.STVK else hr.lame(*params)[::-1]
    I = np.eye(dim)
    want = (lam * np.einsum("ij,kl->ijkl", I, I) + mu * (np.einsum("ik,jl->ijkl", I, I) + np.einsum("il,jk->ijkl", I, I)))
    _, A = hr.material(model, params, I)
    assert np.abs(A - want).max() <= 1e-15 * np.abs(want).max()


def test_only_saint_venant_kirchhoff_in_2d_and_no_logarithm_of_an_inverted_element():
    m = dict(dim=2, conn=np.array([[0, 1, 2]]), xyz=np.array([[0.0, 0], [1, 0], [0, 1]]), gid_rep=np.arange(3), n_global=3)
    with pytest.raises(ValueError, match="Only Saint Venant-Kirchhoff in 2D"):
        hr.assemble(m, np.zeros((3, 2)), hr.NEOHOOKE, (1.0, 0.3))
    with pytest.raises(ValueError, match="ln det F"):
        hr.material(hr.NEOHOOKE, (1.0, 0.3), -np.eye(3))


def test_element_loop_reduces_to_linear_elasticity_at_zero_displacement():
    """the restated element loop at u = 0 against the oracle's FE::assemblyLinElasXDim on the same mesh (host only)"""
    import fedd_oracle as fo
    om = fo.build_mesh_structured(3, 1, 2)
    m = dict(dim=3, conn=om.conn, xyz=om.xyz, gid_rep=om.gid_rep, gid_uni=om.gid_uni, flag_uni=om.flag_uni, n_global=om.n_global)
    lam, mu = hr.stvk_params(2.0e6, 0.4)
    K, f, minJ = hr.assemble(m, np.zeros_like(om.xyz), hr.STVK, (lam, mu))
    L = fo.assembly_linelas(om, lam, mu)
    assert minJ == 1.0 and np.all(f == 0.0)
    assert np.array_equal(K.indptr, L.indptr) and np.array_equal(K.indices, L.indices)
    assert np.abs(K.data - L.data).max() <= RTOL * np.abs(L.data).max()
