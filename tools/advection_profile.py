"""Measurements of the advection path (profiles/advection_*).

  python tools/advection_profile.py cube [M]     N, W, N + W, N + W + A and FEDD_FORM_LAPLACE_VEC on the P2 mesh of an M^3-cell
                                                 cube (default 64, the p2_cube size of bench.py --full): two warm-up calls,
                                                 five timed ones each
  python tools/advection_profile.py newton6k     three Newton iterations of P2 / P1 Navier-Stokes on DFG3DCylinder_6k.mesh
                                                 (cfg-4 boundary conditions, viscosity 0.01, monolithic Schwarz + GMRES to 1e-8):
                                                 device ms of the parts of the LAST iteration

Per-kernel times: run either under `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/advection_profile.py ...`
and read DIR/NAME_kernel_stats.csv (k_adv_elem, k_adv_gather, k_merge_values, ...).  The JSON printed here comes from the
library's HIP-event timers (classes) and, for the merge, which has no class, from the host clock around a synchronised call."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from feddlib_amd import capi  # noqa: E402


def cube(M):
    m1 = capi.structured_mesh(3, (1, 1, 1), [M] * 3, 0)
    mv = capi.p2_of_p1(m1, volume_id=0)
    c = capi.Context(device=0)
    c.mesh_set_dict(mv)
    x = mv["xyz"]
    c.velocity_set(np.stack([np.sin(x[:, 0] + x[:, 1]), np.cos(x[:, 1] - x[:, 2]), np.sin(x[:, 2]) + 0.5], axis=1))
    c.pattern_build(3, capi.BLOCK_DIAG)
    out = {"mesh": "P2 of %d^3 cells" % M, "elements": int(mv["conn"].shape[0]), "nodes": int(x.shape[0])}

    def timed(fn, reps=5):
        fn(); fn()
        c.sync(); c.timing_enable(True); c.timing_reset()
        for _ in range(reps):
            fn()
        c.sync()
        t = c.timing_get_sampled()["assemble"]
        c.timing_enable(False)
        return {"ms_per_call": t[0] / reps, "model_bytes_per_call": t[2] / reps}

    out["laplace_vec"] = timed(lambda: c.assemble(capi.FORM_LAPLACE_VEC))
    del out["laplace_vec"]["model_bytes_per_call"]      # that path states no byte model
    c.matrix_store(0)
    for name, kind, add in (("adv_N", capi.ADV_N, -1), ("adv_W", capi.ADV_W, -1), ("adv_NEWTON", capi.ADV_NEWTON, -1),
                            ("adv_NEWTON_plus_A", capi.ADV_NEWTON, 0)):
        e = timed(lambda: c.assemble_advection(kind, 1.0, add, 4))
        e["GBs_on_model"] = e["model_bytes_per_call"] / e["ms_per_call"] / 1e6
        e["frac_hbm_8TBs"] = e["GBs_on_model"] / 8000.0
        e["vs_laplace_vec"] = e["ms_per_call"] / out["laplace_vec"]["ms_per_call"]
        out[name] = e
    c.close()
    return out


def newton6k():
    m1 = capi.read_mesh(os.path.join(ROOT, "tests", "golden", "DFG3DCylinder_6k.mesh"), 3)
    mv = capi.p2_of_p1(m1, volume_id=0)
    nv, n_p = mv["xyz"].shape[0], m1["xyz"].shape[0]
    n = 3 * nv + n_p
    X, flag, H = mv["xyz"], mv["flag_uni"], 0.41
    nodes = np.nonzero(np.isin(flag, (1, 2, 4)))[0]
    rows = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
    vals = np.zeros((nodes.shape[0], 3))
    inflow = flag[nodes] == 2
    y, z = X[nodes, 1], X[nodes, 2]
    vals[inflow, 0] = (16.0 * y * (H - y) * z * (H - z) / H ** 4)[inflow]
    vals = vals.ravel()
    c = capi.Context(device=0)
    c.mesh_set_dict(mv)
    c.pattern_build(3, capi.BLOCK_DIAG)
    c.assemble(capi.FORM_LAPLACE_VEC)
    c.matrix_scale(-1, 0.01)
    c.matrix_store(0)
    c.assemble_div(n_p, 1, 2)
    c.matrix_scale(1, -1.0)
    c.matrix_scale(2, -1.0)
    x = np.zeros(n); x[rows] = vals
    out = {"mesh": "DFG3DCylinder_6k P2/P1", "dofs": n, "iterations": []}
    for k in range(3):
        c.timing_enable(True); c.timing_reset()
        c.velocity_set(x[:3 * nv])
        c.assemble_advection(capi.ADV_N, 1.0, 0, 4)
        c.block_merge(4, 2, 1, -1)
        r = c.spmv(x)
        r[rows] = 0.0
        c.assemble_advection(capi.ADV_NEWTON, 1.0, 0, 4)
        c.sync(); t0 = time.perf_counter()
        c.block_merge(4, 2, 1, -1)
        c.sync(); merge_ms = (time.perf_counter() - t0) * 1e3
        c.rhs_set(-r)
        c.dirichlet_rows(rows, np.zeros(rows.shape[0]))
        c.schwarz_setup(overlap=1, combine=capi.COMBINE_RESTRICTED)
        dx, its, rel = c.gmres(None, rtol=1e-8, max_it=1500, restart=300, use_prec=True)
        c.sync()
        t = c.timing_get()
        c.timing_enable(False)
        x += dx
        out["iterations"].append({"residual": float(np.linalg.norm(r)), "gmres_iterations": its, "gmres_relres": rel,
                                  "advection_ms_two_calls": t["assemble"][0], "merge_ms_host_clock": merge_ms,
                                  "dirichlet_ms": t["dirichlet"][0], "symbolic_ms": t["symbolic"][0],
                                  "schwarz_setup_ms": t["schwarz_setup"][0],
                                  "gmres_ms": t["spmv"][0] + t["spmv_setup"][0] + t["schwarz_apply"][0] + t["ortho"][0]})
    c.close()
    return out


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "cube"
    res = cube(int(sys.argv[2]) if len(sys.argv) > 2 else 64) if mode == "cube" else newton6k()
    print(json.dumps(res, indent=1))
