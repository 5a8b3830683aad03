"""Additive against multiplicative level combination (fedd_schwarz_set_level_combination) on one GPU: iterations and ms per
solve, and the cost of one preconditioner apply, at cfg 2 (100^3-cell Laplace, bench.py's 64-node boxes, Q1 coarse level, rtol
1e-8) and cfg 5's share (94^3-cell elasticity, 8-node boxes, RGDSW with translations, rtol 1e-6).  The multiplicative solve runs
twice: with the reference's semantics (coarse pre-apply into the solution vector, then GMRES from it; rtol relative to the
residual of that start) and at the additive solve's accuracy (both stop at ||b - A x|| <= rtol ||b||).  One JSON line per
configuration.
usage: level_combination.py [cfg2|cfg5|both] [solves] [--restart-drift]
--restart-drift: 3D elasticity H/h = 16 (mu 2e6, nu 0.4), 8-node boxes, Q1 coarse level of 8 cells, restart 30, rtol 1e-12, the
three GMRES forms (the restart projection's case; --lib PATH runs a scratch build of the library instead)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from feddlib_amd import capi  # noqa: E402


def one(c, name, n, rtol, solves):
    """three solves: additive at rtol; multiplicative with the reference's semantics (pre-apply, then GMRES from it, rtol relative
    to ||b - A x_0|| of the projected start); multiplicative at the additive solve's accuracy (rtol scaled by ||b|| / ||r_0||, so
    that both stop at ||b - A x|| <= rtol ||b||)"""
    b = c.rhs_get()
    nb = float(np.linalg.norm(b))
    x0 = c.schwarz_coarse_apply(b)                    # the start the solver forms: x_0 = Pc b, refined once
    x0 = x0 + c.schwarz_coarse_apply(b - c.spmv(x0))
    r0_over_b = float(np.linalg.norm(b - c.spmv(x0))) / nb
    out = {"r0_of_the_projected_start_over_b": r0_over_b}
    runs = (("additive", capi.LEVELS_ADDITIVE, rtol, False),
            ("multiplicative_reference_semantics", capi.LEVELS_MULTIPLICATIVE, rtol, True),
            ("multiplicative_equal_accuracy", capi.LEVELS_MULTIPLICATIVE, rtol / r0_over_b, False))
    for key, comb, rt, pre in runs:
        c.schwarz_set_level_combination(comb)

        def solve():
            if pre:
                c.schwarz_coarse_apply(None)
                return c.gmres_x0(None, rtol=rt, max_it=2000, restart=100, use_prec=True)[1:]
            return c.gmres(None, rtol=rt, max_it=2000, restart=100, use_prec=True, want_x=False)[1:]
        wall, (its, rel), tm = bench.timed_passes(c, solve, solves, 1, wall_without_timers=True)
        x = c.solution_get()
        true_rel = float(np.linalg.norm(b - c.spmv(x))) / nb
        reps = 50
        c.schwarz_apply_device(5)
        c.sync()
        t0 = time.perf_counter()
        c.schwarz_apply_device(reps)
        c.sync()
        apply_ms = (time.perf_counter() - t0) / reps * 1e3
        out[key] = {"rtol": rt, "gmres_iterations": its, "ms_per_solve": round(wall, 3), "relres": rel, "true_relres_vs_b": true_rel,
                    "apply_ms_back_to_back": round(apply_ms, 4), "phases_device_ms_per_solve": bench.phases(tm, solves)}
    c.schwarz_set_level_combination(capi.LEVELS_ADDITIVE)
    a = out["additive"]
    for key in ("multiplicative_reference_semantics", "multiplicative_equal_accuracy"):
        m = out[key]
        m["iterations_ratio"] = m["gmres_iterations"] / a["gmres_iterations"]
        m["solve_time_ratio"] = m["ms_per_solve"] / a["ms_per_solve"]
        m["apply_cost_ratio"] = m["apply_ms_back_to_back"] / a["apply_ms_back_to_back"]
    print(json.dumps({"config": name, "dofs": n, **out}), flush=True)


def cfg2(solves):
    m = capi.structured_mesh(3, (1, 1, 1), [100] * 3, 0)
    c = capi.Context(device=0)
    bench.env_options(c)
    c.mesh_set_dict(m)
    c.pattern_build(1, capi.BLOCK_SCALAR)
    c.assemble(capi.FORM_LAPLACE)
    c.assemble_rhs([1.0])
    c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    c.schwarz_set_target(64, 1.0)
    c.schwarz_setup(1, capi.COMBINE_RESTRICTED, two_level=1, coarse_kind=capi.COARSE_Q1)
    one(c, "cfg 2: 100^3-cell Laplace, 64-node boxes, Q1 coarse level (%d coarse dofs), rtol 1e-8" % c.schwarz_coarse_sizes()[1],
        m["n_global"], 1e-8, solves)
    c.close()


def cfg5(solves):
    M = 94
    m = capi.structured_mesh(3, (1, 1, 1), [M] * 3, 0)
    c = capi.Context(device=0)
    bench.env_options(c)
    c.mesh_set_dict(m)
    mu, nu = 2.0e6, 0.4
    lam = 2.0 * mu * nu / (1.0 - 2.0 * nu)
    c.pattern_build(3, capi.BLOCK_FULL)
    c.assemble(capi.FORM_LINELAS, [lam, mu])
    c.assemble_rhs([0.0, 1.0, 0.0])
    c.dirichlet([2], [0.0, 0.0, 0.0])
    c.schwarz_set_target(8, 1.0)
    c.set_option("gdsw_rotations", 0)
    c.schwarz_setup(1, capi.COMBINE_RESTRICTED, two_level=1, coarse_kind=capi.COARSE_RGDSW)
    one(c, "cfg 5's share: 94^3-cell elasticity, 8-node boxes, RGDSW translations (%d coarse dofs), rtol 1e-6"
        % c.schwarz_coarse_sizes()[1], 3 * m["n_global"], 1e-6, solves)
    c.close()


def restart_drift():
    m = capi.structured_mesh(3, 1, 16)
    c = capi.Context(device=0)
    c.mesh_set_dict(m)
    c.pattern_build(3, capi.BLOCK_FULL)
    mu, nu = 2.0e6, 0.4
    c.assemble(capi.FORM_LINELAS, [2.0 * mu * nu / (1.0 - 2.0 * nu), mu])
    c.assemble_rhs([0.0, 1.0, 0.0])
    c.dirichlet([2], [0.0, 0.0, 0.0])
    c.schwarz_set_target(8, 1.0)
    c.schwarz_set_coarse(8)
    c.schwarz_setup(1, capi.COMBINE_RESTRICTED, two_level=1, coarse_kind=capi.COARSE_Q1)
    b = c.rhs_get()
    for gk, comb in ((0, 1), (1, 1), (2, 1), (2, 0)):
        c.schwarz_set_level_combination(comb)
        c.set_option("gmres_kind", gk)
        x, its, rel = c.gmres(None, rtol=1e-12, max_it=600, restart=30, use_prec=True)
        r = b - c.spmv(x)
        coarse_part = float(np.linalg.norm(c.schwarz_coarse_apply(r)) / np.linalg.norm(c.schwarz_coarse_apply(b)))
        print(json.dumps({"restart_drift": True, "scratch_library": "--lib" in sys.argv, "gmres_kind": gk, "multiplicative": comb, "its": its, "relres": rel,
                          "true_relres_vs_b": float(np.linalg.norm(r) / np.linalg.norm(b)), "coarse_part_of_final_residual": coarse_part,
                          "status": c.gmres_status()}), flush=True)
    c.close()


if __name__ == "__main__":
    if "--lib" in sys.argv:      # (a scratch build of the library, e.g. one without the restart projection)
        capi.LIB_PATH = sys.argv[sys.argv.index("--lib") + 1]
    if "--restart-drift" in sys.argv:
        restart_drift()
        sys.exit(0)
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    solves = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    if which in ("cfg2", "both"):
        cfg2(solves)
    if which in ("cfg5", "both"):
        cfg5(solves)
