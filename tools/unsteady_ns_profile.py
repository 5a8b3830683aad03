"""Measurement of the BDF time loop of unsteady Navier-Stokes (DESIGN.md section 4 "BDF"); writes profiles/unsteady_ns_step.json.

  python tools/unsteady_ns_profile.py [--mesh FILE] [--steps K] [--stream-cells M] [--out FILE]

Two parts, both at the ABI level, as tests/test_gpu_time_navier_stokes.py issues the calls:

  loop    P2 / P1 on the benchmark cylinder (default tests/golden/DFG3DCylinder_1k.mesh), the settings of
          tests/golden/unsteadynavierstokes_xml: viscosity 1e-3, largest inflow velocity 0.3, dt = 0.01, BDF2 with a BDF1 start,
          Newton to 1e-6 of the step's first residual, GMRES to 1e-8 with one-level Schwarz (restricted) set up again in every
          nonlinear iteration.  Per step: the history kernel (k_multistep) and the block apply from the library's HIP-event
          timers; advection assembly, merge, Schwarz setup, solve and the residual SpMV as wall time of the device-synchronised
          calls; the nonlinear and the GMRES iterations.
  stream  the history kernel alone on a system beyond the caches: the merged P1 / P1 system of an M^3-cell cube (default 128:
          8.6 million rows), one first step and five full BDF2 steps; bandwidth on the byte model (40 bytes per row for a full
          step, 24 for the first, + 8 per zeroed pressure row) against the GPU's measured read ceiling (fedd_read_bandwidth).
Not wired into bench.py."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from feddlib_amd import capi  # noqa: E402

NU, RHO, UMAX, DT, H = 1.0e-3, 1.0, 0.3, 0.01, 0.41
TOL, RTOL = 1e-6, 1e-8
SLOT_A, SLOT_B, SLOT_BT, SLOT_F, SLOT_M, SLOT_AT = 0, 1, 2, 4, 5, 6


class Clock:
    """wall time of device-synchronised sections, summed by name"""

    def __init__(self, c):
        self.c, self.ms = c, {}

    def __call__(self, name, fn, *a, **kw):
        self.c.sync()
        t0 = time.perf_counter()
        r = fn(*a, **kw)
        self.c.sync()
        self.ms[name] = self.ms.get(name, 0.0) + 1e3 * (time.perf_counter() - t0)
        return r


def timers(c):
    c.sync()
    return {k: v[0] for k, v in c.timing_get().items()}


def loop(mesh_file, steps):
    m1 = capi.read_mesh(mesh_file, 3)
    mv = capi.p2_of_p1(m1, volume_id=0)
    X, flag = mv["xyz"], mv["flag_uni"]
    nodes = np.nonzero(np.isin(flag, (1, 2, 4)))[0]
    rows = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
    vals = np.zeros((nodes.shape[0], 3))
    inflow = flag[nodes] == 2
    y, z = X[nodes, 1], X[nodes, 2]
    vals[inflow, 0] = (UMAX * 16.0 * y * (H - y) * z * (H - z) / H ** 4)[inflow]
    vals = vals.ravel()
    nv, n_p = X.shape[0], m1["xyz"].shape[0]
    n = 3 * nv + n_p
    c = capi.Context(device=0)
    c.timing_enable(1)
    c.mesh_set_dict(mv)
    c.pattern_build(3, capi.BLOCK_DIAG)
    c.assemble(capi.FORM_LAPLACE_VEC)
    c.matrix_scale(-1, RHO * NU)
    c.matrix_store(SLOT_A)
    c.assemble_div(n_p, SLOT_B, SLOT_BT)
    c.matrix_scale(SLOT_B, -1.0)
    c.matrix_scale(SLOT_BT, -1.0)
    c.pattern_build(3, capi.BLOCK_DIAG)
    c.assemble(capi.FORM_MASS_VEC)
    c.matrix_scale(-1, RHO)
    c.matrix_store(SLOT_M)

    def system(clock, kind, x):
        c.velocity_set(x[:3 * nv])
        clock("advection_assembly", c.assemble_advection, kind, RHO, SLOT_AT, SLOT_F)
        clock("merge", c.block_merge, SLOT_F, SLOT_BT, SLOT_B, -1)

    out = {"mesh": os.path.basename(mesh_file), "velocity_nodes": int(nv), "pressure_nodes": int(n_p), "rows": int(n), "steps": []}
    x = np.zeros(n)
    last, combines = None, 0
    for step in range(steps):
        clock = Clock(c)
        before = timers(c)
        cm, coeff = (1.0 / DT, [1.0 / DT]) if step == 0 else (1.5 / DT, [2.0 / DT, -0.5 / DT])
        if last != cm:
            def combine():
                if not c.matrix_combine_current(SLOT_M, cm, SLOT_A, 1.0):
                    c.matrix_combine(SLOT_M, cm, SLOT_A, 1.0)
                c.matrix_store(SLOT_AT)
            clock("combine", combine)
            last = cm
            combines += 1
        system(clock, capi.ADV_N, x)
        if step == 0:
            c.multistep_begin(2)
        c.solution_set(x)
        clock("history_and_rhs", c.multistep_advance, SLOT_M, coeff)
        b = c.rhs_get()
        hist, gmres_its = [], []
        for k in range(20):
            system(clock, capi.ADV_N, x)
            r = clock("residual_spmv", c.spmv, x) - b
            r[rows] = x[rows] - vals
            hist.append(float(np.linalg.norm(r)))
            if hist[-1] / hist[0] < TOL:
                break
            system(clock, capi.ADV_NEWTON, x)
            rhs = -r
            rhs[rows] = 0.0
            c.rhs_set(rhs)
            clock("dirichlet_rows", c.dirichlet_rows, rows, -r[rows])
            clock("schwarz_setup", c.schwarz_setup, overlap=1, combine=capi.COMBINE_RESTRICTED)
            dx, its, rel = clock("solve", c.gmres, None, rtol=RTOL, max_it=1500, restart=300, use_prec=True)
            gmres_its.append(int(its))
            x = x + dx
        after = timers(c)
        d = {k: after[k] - before[k] for k in after}
        out["steps"].append({"step": step + 1, "nonlinear_iterations": len(hist) - 1, "gmres_iterations": gmres_its,
                             "relative_residuals": [h / hist[0] for h in hist],
                             "wall_ms": clock.ms,
                             "device_ms": {k: d[k] for k in ("multistep_state", "block_apply", "assemble", "symbolic", "schwarz_setup",
                                                            "schwarz_apply", "spmv", "spmv_setup", "ortho", "dirichlet")}})
    out["combines"] = combines
    c.close()
    return out


def stream(M):
    c = capi.Context(device=0)
    c.timing_enable(1)
    m = capi.structured_mesh(3, 1, M)
    nn = m["xyz"].shape[0]
    c.mesh_set_dict(m)
    c.pattern_build(3, capi.BLOCK_DIAG)
    c.assemble(capi.FORM_MASS_VEC)
    c.matrix_store(SLOT_M)
    c.assemble(capi.FORM_LAPLACE_VEC)
    c.matrix_store(SLOT_A)
    c.assemble_div(nn, SLOT_B, SLOT_BT)
    c.block_merge(SLOT_A, SLOT_BT, SLOT_B, -1)
    n, n_m = c.csr_sizes()[0], 3 * nn
    c.solution_set(np.random.default_rng(1).standard_normal(n))
    c.multistep_begin(2)
    recs = []
    for k in range(6):
        before = timers(c)
        c.multistep_advance(SLOT_M, [1.0 / DT] if k == 0 else [2.0 / DT, -0.5 / DT])
        after = timers(c)
        nbytes = (24.0 if k == 0 else 40.0) * n + 8.0 * (n - n_m)
        ms = after["multistep_state"] - before["multistep_state"]
        recs.append({"advance": k + 1, "first_step": k == 0, "history_kernel_ms": ms, "model_bytes": nbytes,
                     "GBs_on_model": nbytes / ms / 1e6 if ms > 0 else None,
                     "block_apply_ms": after["block_apply"] - before["block_apply"]})
    full = [r["GBs_on_model"] for r in recs[1:] if r["GBs_on_model"]]
    ceiling = c.read_bandwidth(min(2 << 30, max(64 << 20, 40 * n)), 10)
    c.close()
    return {"mesh": "P1 / P1 merged, %d^3 cells" % M, "rows": int(n), "mass_rows": int(n_m), "advances": recs,
            "full_step_GBs_on_40_bytes_per_row_median": float(np.median(full)) if full else None, "read_ceiling_GBs": ceiling,
            "full_step_fraction_of_read_ceiling": float(np.median(full)) / ceiling if full and ceiling > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default=os.path.join(ROOT, "tests", "golden", "DFG3DCylinder_1k.mesh"))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--stream-cells", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unsteady_ns_step.json"))
    a = ap.parse_args()
    out = {"settings": {"viscosity": NU, "density": RHO, "max_velocity": UMAX, "dt": DT, "scheme": "BDF2, BDF1 start", "linearization": "Newton",
                        "relNonLinTol": TOL, "gmres_rtol": RTOL, "preconditioner": "one-level Schwarz, overlap 1, restricted"},
           "loop": loop(a.mesh, a.steps), "history_kernel_stream": stream(a.stream_cells)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"written": a.out, "rows": out["loop"]["rows"], "combines": out["loop"]["combines"],
                      "nonlinear_iterations": [s["nonlinear_iterations"] for s in out["loop"]["steps"]],
                      "wall_ms": [s["wall_ms"] for s in out["loop"]["steps"]],
                      "stream": {k: out["history_kernel_stream"][k] for k in ("rows", "full_step_GBs_on_40_bytes_per_row_median", "read_ceiling_GBs",
                                                                              "full_step_fraction_of_read_ceiling")}}))


if __name__ == "__main__":
    main()
