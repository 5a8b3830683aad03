"""Option "gmres_dot_own": the block Gram-Schmidt dot sweeps form W^T W from the W tile they hold in registers.

With gmres_dot_own 1 (default) k_blockdot and the second walk of k_blockfuse stream only the k final basis columns; the rows
k .. k + sa - 1 of [Q_k W]^T W come from the registers, formed for i <= j and stored to (i, j) and (j, i).  With 0 they stream
all k + sa columns, the block's own a second time.  Both forms put the same products through the same per-lane expression, the
same transpose reduction and the same order over the four waves, so they must agree in every bit: there is no tolerance in this
file.  Each comparison solves the same system with the option at 0 and at 1 and asserts np.array_equal on x and equality of the
iteration count, blocks, cut_blocks and fused_blocks.

Systems: the unpreconditioned 16^3-cell Laplace (4 913 rows: 5 row blocks of 1024, the last partial) with the assembled f = 1
plus 0.3 of its size of seeded noise, which takes 69 iterations to 1e-10 -- a cycle with k + sa >= 65 columns, the mid-loop flush
of k_blockdot<16, 2, 2> at gmres_dot_gy 1 -- under restart 100 and restart 21 (sa = min(s, room) < S, both parities of k); and one
preconditioned 12^3-cell Laplace (Schwarz target 27) with blocks of 16 (Newton shifts, odd k after the two 8-blocks)."""
import numpy as np
import pytest

import fedd_oracle as fo

pytestmark = pytest.mark.gpu

DOT_M = 16
DOT_RTOL = 1e-10
CHOL_TOL_DEFAULT = 1e-13
_SYS = {}


def _laplace(L, c, M):
    m = L.structured_mesh(3, 1, M)
    c.mesh_set_dict(m)
    c.pattern_build(1, L.BLOCK_SCALAR)
    c.assemble(L.FORM_LAPLACE)
    c.assemble_rhs([1.0])
    c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    return m


def _noisy_system(L, c):
    """assembles the 16^3-cell Laplace on c; returns the right-hand side (computed once: the oracle's f = 1 with boundary
    conditions plus 0.3 max |f| of seeded normal noise)"""
    m = _laplace(L, c, DOT_M)
    if "b" not in _SYS:
        om = fo.Mesh(dim=m["dim"], fe="P1", conn=m["conn"], xyz=m["xyz"], gid_rep=m["gid_rep"], flag_rep=m["flag_rep"],
                     gid_uni=m["gid_uni"], flag_uni=m["flag_uni"], xyz_uni=None, n_global=m["n_global"])
        rhs_bc = fo.laplace_problem(om)[1]
        b = rhs_bc + 0.3 * np.abs(rhs_bc).max() * np.random.default_rng(DOT_M).standard_normal(rhs_bc.shape[0])
        b.setflags(write=False)
        _SYS["b"] = b
    return _SYS["b"]


def _on_off(c, label, **solve):
    """solves with gmres_dot_own 0 and 1; asserts equal bits and counters; returns (iterations, info) of the option-0 run"""
    out = []
    for own in (0, 1):
        c.set_option("gmres_dot_own", own)
        x, its, rel = c.gmres(**solve)
        info = c.gmres_info()
        print("%s own %d: %d iterations, relres %.3e, %s" % (label, own, its, rel, info))
        assert info["kind"] == 2
        out.append((x, its, rel, info))
    (x0, its0, rel0, info0), (x1, its1, rel1, info1) = out
    assert its0 == its1, (label, its0, its1)
    assert info0 == info1, (label, info0, info1)
    assert rel0 == rel1, (label, rel0, rel1)
    assert np.all(np.isfinite(x0)), label
    assert np.array_equal(x0, x1), (label, int(np.count_nonzero(x0 != x1)), float(np.abs(x0 - x1).max()))
    return its0, info0


def _restore(c):
    c.set_option("gmres_dot_own", 1)
    c.set_option("gmres_chol_tol", CHOL_TOL_DEFAULT)
    c.set_option("gmres_tol_blocks", 1)
    c.set_option("gmres_dot_gy", 0)
    c.set_option("gmres_fuse", -1)
    c.set_option("gmres_s", 0)
    c.set_option("gmres_kind", 2)


@pytest.mark.parametrize("s,fuse", [(4, -1), (8, -1), (16, 0), (16, 1)])
def test_own_columns_from_registers_same_bits(fedd_lib, s, fuse):
    """k_blockdot<4, 2, 4>, <8, 2, 4>, <16, 2, 2> and k_blockfuse<16> with 1, 2, 3 workgroups per row block, restart 100 and 21,
    gmres_tol_blocks 0 (blocks of the full length at rtol 1e-10): option 0 against 1, bit for bit.  Blocks of 16 at restart 100
    must reach 64 iterations in a cycle (33 column groups: the mid-loop flush at gmres_dot_gy 1); with gmres_fuse 1 every block
    is fused.  Then the same with gmres_chol_tol 0.5: every block is cut (d_sa < sa_req) -- the columns from sa on stay zero and
    the cut columns are dropped alike; asserted: the option-0 run has cut blocks."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        b = _noisy_system(L, c)
        c.set_option("gmres_kind", 2)
        c.set_option("gmres_s", s)
        c.set_option("gmres_fuse", fuse)
        c.set_option("gmres_tol_blocks", 0)
        for chol_tol in (CHOL_TOL_DEFAULT, 0.5):
            c.set_option("gmres_chol_tol", chol_tol)
            for restart in (100, 21):
                for gy in (1, 2, 3):
                    c.set_option("gmres_dot_gy", gy)
                    its, info = _on_off(c, "s %d fuse %d chol_tol %g restart %d gy %d" % (s, fuse, chol_tol, restart, gy),
                                        b=b, rtol=DOT_RTOL, max_it=400, restart=restart, use_prec=False)
                    assert info["s"] == s
                    assert info["fused_blocks"] == (info["blocks"] if (s > 8 and fuse == 1) else 0), info
                    if chol_tol == 0.5:
                        assert info["cut_blocks"] > 0, info        # (otherwise the cut path was not run)
                    elif s > 8 and restart == 100:
                        assert its >= 64, its                      # one workgroup (gy 1) parked more than 32 column groups
    finally:
        _restore(c)
        c.close()


def test_own_columns_preconditioned_same_bits(fedd_lib):
    """12^3 cells, one-level Schwarz (target 27), blocks of 16 on the Newton basis: two monomial 8-blocks, then shifted blocks
    that start at odd k.  Option 0 against 1: x bit for bit."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        _laplace(L, c, 12)
        c.schwarz_set_target(27, 1.0)
        c.schwarz_setup(1, L.COMBINE_RESTRICTED)
        c.set_option("gmres_kind", 2)
        c.set_option("gmres_s", 16)
        c.set_option("gmres_tol_blocks", 0)
        # (to 1e-10 the solve ends inside the two 8-blocks, 15 iterations: the tolerance is the one that reaches a third block)
        its, info = _on_off(c, "preconditioned s 16", b=None, rtol=1e-13, max_it=300, restart=100, use_prec=True)
        assert info["s"] == 16 and its > 16, (its, info)           # (a block beyond the two 8-blocks ran)
    finally:
        _restore(c)
        c.close()
