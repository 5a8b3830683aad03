"""Block preconditioners against the monolithic one on cfg 4's system ("Block preconditioners";
profiles/blockprec_stokes.json).

  python tools/blockprec_profile.py [mesh]      default 6k (tests/golden/DFG3DCylinder_6k.mesh)

P2 / P1 Stokes on the DFG cylinder, nu = 1e-3, the driver's boundary conditions, GMRES(300) to 1e-6 (the tolerance bench.py
uses for cfg 4), at most 3000 iterations.  Per method -- Monolithic (one-level Schwarz on the merged system, the large-subdomain
path), Diagonal and Triangular with one-level and with two-level (Q1) children -- iterations, relative residual, setup ms and
solve ms (host clock around synchronised calls; one warm-up, median of three).  The velocity child's boxes have no overlap (a P2
box plus a graph layer exceeds the dense local solver's 256 dofs in 3D), the Schur child's overlap is 1.  Then k_bt_sub alone:
HIP-event time per launch over 200 back-to-back Triangular applies, against its byte model and the 8 TB/s HBM peak.
Monolithic needs nothing of the block layer, so the same script gives its figures on a commit without it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feddlib_amd import capi  # noqa: E402

NU, RTOL, MAX_IT, RESTART = 1.0e-3, 1e-6, 3000, 300
HBM_PEAK = 8.0e12


def median_ms(c, fn, reps=3):
    fn()
    c.sync()
    ms, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        c.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return ms[len(ms) // 2], last


def main(which):
    m1 = capi.read_mesh(os.path.join(ROOT, "tests", "golden", "DFG3DCylinder_%s.mesh" % which), 3)
    mv = capi.p2_of_p1(m1, volume_id=0)
    n_p, nv = m1["xyz"].shape[0], mv["xyz"].shape[0]
    nA, n = 3 * nv, 3 * nv + n_p
    X, flag, H = mv["xyz"], mv["flag_uni"], 0.41
    nodes = np.nonzero(np.isin(flag, (1, 2, 4)))[0]
    rows = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
    vals = np.zeros((nodes.shape[0], 3))
    inflow = flag[nodes] == 2
    vals[inflow, 0] = (16.0 * X[nodes, 1] * (H - X[nodes, 1]) * X[nodes, 2] * (H - X[nodes, 2]) / H ** 4)[inflow]

    p = capi.Context(device=0)
    p.mesh_set_dict(mv)
    p.pattern_build(3, capi.BLOCK_DIAG)
    p.assemble(capi.FORM_LAPLACE_VEC)
    p.matrix_scale(-1, NU)
    p.matrix_store(0)
    p.assemble_div(n_p, 1, 2)
    p.matrix_scale(1, -1.0)
    p.matrix_scale(2, -1.0)
    p.block_merge(0, 2, 1, -1)
    p.rhs_set(np.zeros(n))
    p.dirichlet_rows(rows, vals.ravel())
    b = p.rhs_get()

    def solve():
        return p.gmres(None, rtol=RTOL, max_it=MAX_IT, restart=RESTART, use_prec=True, want_x=False)[1:]

    def record(setup):
        setup_ms, _ = median_ms(p, setup)
        solve_ms, (its, rel) = median_ms(p, solve)
        true_rel = float(np.linalg.norm(b - p.spmv(p.solution_get())) / np.linalg.norm(b))
        return {"iterations": int(its), "relres": float(rel), "true_relres": true_rel, "converged": bool(rel <= RTOL),
                "setup_ms": setup_ms, "solve_ms": solve_ms}

    out = {"workload": "P2/P1 Stokes, DFG3DCylinder_%s.mesh, %d dofs (%d velocity, %d pressure), nu %g, GMRES(%d) rtol %g, max %d iterations"
                       % (which, n, nA, n_p, NU, RESTART, RTOL, MAX_IT),
           "timing": "host clock around synchronised calls, one warm-up, median of 3", "methods": {}}
    out["methods"]["Monolithic"] = dict(record(lambda: p.schwarz_setup(1, capi.COMBINE_RESTRICTED)),
                                        children="none: one-level Schwarz on the merged system, overlap 1", schwarz=p.schwarz_info())
    if not hasattr(p, "block_prec_attach"):     # a commit without the block layer
        return out
    v, s = capi.Context(device=0), capi.Context(device=0)
    v.mesh_set_dict(mv)
    s.mesh_set_dict(m1)
    s.pattern_build(1, capi.BLOCK_SCALAR)
    s.assemble(capi.FORM_MASS)
    s.matrix_scale(-1, 1.0 / NU)

    def children(two_level):
        def setup():
            p.sync()
            v.matrix_import(p, 0)
            v.dirichlet_nodes(nodes, vals)
            v.schwarz_setup(0, capi.COMBINE_RESTRICTED, two_level=two_level, coarse_kind=capi.COARSE_Q1 if two_level else 0)
            s.schwarz_setup(1, capi.COMBINE_RESTRICTED, two_level=two_level, coarse_kind=capi.COARSE_Q1 if two_level else 0)
            v.sync()
            s.sync()
        return setup

    for two_level in (0, 1):
        for name, kind in (("Diagonal", capi.BLOCKPREC_DIAGONAL), ("Triangular", capi.BLOCKPREC_TRIANGULAR)):
            p.block_prec_attach(kind, v, s, -1.0, 2)
            r = record(children(two_level))
            r["children"] = ("two-level (Q1)" if two_level else "one-level") + ": velocity overlap 0, Schur complement overlap 1"
            r["velocity_schwarz"], r["schur_schwarz"] = v.schwarz_info(), s.schwarz_info()
            if two_level:
                r["coarse_dofs"] = {"velocity": int(v.schwarz_coarse_sizes()[1]), "schur": int(s.schwarz_coarse_sizes()[1])}
            out["methods"]["%s, %s children" % (name, "two-level" if two_level else "one-level")] = r
            p.block_prec_detach()

    # the coupling kernel alone
    children(0)()
    p.block_prec_attach(capi.BLOCKPREC_TRIANGULAR, v, s, -1.0, 2)
    p.schwarz_apply_device(20)
    p.sync()
    p.timing_enable(True)
    p.timing_reset()
    p.schwarz_apply_device(200)
    p.sync()
    ms, launches, nbytes = p.timing_get_sampled()["blockprec_bt"]
    p.timing_enable(False)
    p.block_prec_detach()
    bt = p.matrix_get(2)
    per_launch_ms = ms / max(launches, 1)
    model = nbytes / max(launches, 1)
    out["k_bt_sub"] = {"rows": int(nA), "columns": int(n_p), "nnz": int(bt.nnz), "longest_row": int(np.diff(bt.indptr).max()),
                       "launches_timed": int(launches), "ms_per_launch": per_launch_ms, "model_bytes": model,
                       "model": "12 nnz + 4 (n_A + 1) + 4 n_A + 16 n_A + 16 n_p",
                       "model_GB_per_s": model / (per_launch_ms * 1e-3) / 1e9 if per_launch_ms > 0 else None,
                       "fraction_of_hbm_peak_8TBs": model / (per_launch_ms * 1e-3) / HBM_PEAK if per_launch_ms > 0 else None,
                       "note": "the matrix (%.1f MB) fits the caches: back-to-back launches need not read HBM" % (12e-6 * bt.nnz)}
    for c in (p, v, s):
        c.close()
    return out


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "6k"
    res = main(which)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    name = "blockprec_stokes.json" if which == "6k" else "blockprec_stokes_%s.json" % which
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
