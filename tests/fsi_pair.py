"""Shared set-up of the FSI GPU tests: a fluid mesh on the unit square / cube and a structure mesh shifted by +1 in x, the
interface nodes (x = 1) re-flagged to one common flag on both sides and their x set to exactly 1.0, so that the host
reference's pairing is unambiguous; and the 4 x 4-cell Stokes / linear elasticity pair with its coupled context."""
import numpy as np
import scipy.sparse as sp

import fsi_ref

FLAG = 7


def side(m, shift, flag=FLAG):
    """a copy of the mesh dict, x shifted, the nodes on x = 1 re-flagged and put on x = 1.0 exactly"""
    m = dict(m)
    m["xyz"] = np.array(m["xyz"], dtype=np.float64, copy=True)
    m["xyz"][:, 0] += shift
    on = np.abs(m["xyz"][:, 0] - 1.0) < 1e-12
    m["xyz"][on, 0] = 1.0
    m["flag_uni"] = np.array(m["flag_uni"], dtype=np.int32, copy=True)
    xu = fsi_ref.unique_coords(m)
    m["flag_uni"][xu[:, 0] == 1.0] = flag
    return m


def pair(mesh):
    return side(mesh, 0.0), side(mesh, 1.0)


def reference_table(mf, ms, flags):
    return fsi_ref.match(fsi_ref.unique_coords(mf), mf["flag_uni"], fsi_ref.unique_coords(ms), ms["flag_uni"], flags)


def csr_tuple(ctx):
    rowptr, col, val, _ = ctx.csr_get()
    return rowptr, col, val


class Pair:
    """fluid: P2 / P1 Stokes on 4 x 4 cells, parabolic inflow on x = 0 and no-slip walls (the wall rows include the two corners of
    the interface); structure: P2 linear elasticity on 4 x 4 cells, clamped on its far side x = 2; cpl: the coupled context"""
    DIM, DT = 2, 0.05

    def __init__(self, lib):
        self.lib = lib
        dim = self.DIM
        m1 = lib.structured_mesh(2, 1, 4)
        p2 = lib.p2_of_p1(m1, volume_id=0)
        self.mf, self.ms = pair(p2)
        self.n_p1 = m1["xyz"].shape[0]
        self.nv = p2["xyz"].shape[0]
        self.n_u, self.n_p, self.n_s = dim * self.nv, self.n_p1, dim * self.nv
        self.n_f = self.n_u + self.n_p
        self.fluid, self.struct, self.cpl = lib.Context(device=0), lib.Context(device=0), lib.Context(device=0)
        X = fsi_ref.unique_coords(self.mf)
        inflow = X[:, 0] < 1e-12
        wall = (X[:, 1] < 1e-12) | (X[:, 1] > 1 - 1e-12)
        self.bc_nodes = np.nonzero(inflow | wall)[0]
        self.bc_vals = np.zeros((self.bc_nodes.shape[0], dim))
        free_in = inflow[self.bc_nodes] & ~wall[self.bc_nodes]
        y = X[self.bc_nodes, 1]
        self.bc_vals[free_in, 0] = (4.0 * y * (1.0 - y))[free_in]
        self.bc_rows = (dim * self.bc_nodes[:, None] + np.arange(dim)[None, :]).ravel()
        self.far = np.nonzero(fsi_ref.unique_coords(self.ms)[:, 0] > 2.0 - 1e-12)[0]
        f = self.fluid
        f.mesh_set_dict(self.mf)
        f.pattern_build(dim, lib.BLOCK_DIAG)
        f.assemble(lib.FORM_LAPLACE_VEC)
        f.matrix_store(0)
        f.assemble_div(self.n_p1, 1, 2)
        f.matrix_scale(1, -1.0)
        f.matrix_scale(2, -1.0)
        self.fluid_system()
        self.struct.mesh_set_dict(self.ms)
        self.structure_system()
        self.n_pairs = f.interface_match(self.struct, [FLAG])
        self.i_f, self.i_s, _ = f.interface_match_table()
        self.n_l = dim * self.n_pairs

    def fluid_system(self):
        """the merged [F B^T; B 0] with its wall and inflow rows"""
        f = self.fluid
        f.block_merge(0, 2, 1, -1)
        f.rhs_set(np.zeros(self.n_f))
        f.dirichlet_rows(self.bc_rows, self.bc_vals.ravel())

    def structure_system(self):
        s, lib = self.struct, self.lib
        s.pattern_build(self.DIM, lib.BLOCK_FULL)
        s.assemble(lib.FORM_LINELAS, [1.0, 1.0])
        s.assemble_rhs([0.0, -1.0])
        s.dirichlet_nodes(self.far, np.zeros((self.far.shape[0], self.DIM)))

    def dirichlet_marks(self):
        dir_f = np.zeros(self.n_f, dtype=bool)
        dir_f[self.bc_rows] = True
        dir_s = np.zeros(self.n_s, dtype=bool)
        dir_s[(self.DIM * self.far[:, None] + np.arange(self.DIM)[None, :]).ravel()] = True
        return dir_f, dir_s

    def host_matrix(self, mask=None, dt=None):
        """(rowptr, col, val) of the coupled matrix out of the children's fedd_csr_get and the table, and the dof maps"""
        dir_f, dir_s = self.dirichlet_marks()
        fdof, sdof = fsi_ref.interface_dofs(self.i_f, self.i_s, self.DIM, mask)
        csr = fsi_ref.coupled_csr(csr_tuple(self.fluid), csr_tuple(self.struct), dir_f, dir_s, fdof, sdof, self.DT if dt is None else dt)
        return csr, fdof, sdof

    def facsi_children(self):
        """the reference's faCSIBCFactory_: homogeneous Dirichlet rows on the interface velocity dofs of the fluid, then the
        children's Schwarz setups (the fluid's is the monolithic one on the merged system)"""
        lib = self.lib
        self.fluid.dirichlet_rows((self.DIM * self.i_f[:, None].astype(np.int64) + np.arange(self.DIM)[None, :]).ravel().astype(np.int32),
                                  np.zeros(self.n_l))
        self.fluid.schwarz_setup(1, lib.COMBINE_RESTRICTED)
        self.struct.schwarz_setup(1, lib.COMBINE_RESTRICTED)

    def close(self):
        for c in (self.cpl, self.fluid, self.struct):
            c.close()


def scipy_matrix(csr):
    rowptr, col, val = csr
    n = len(rowptr) - 1
    return sp.csr_matrix((val, col, rowptr), shape=(n, n))
