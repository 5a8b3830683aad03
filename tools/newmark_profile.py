"""Measurement of the Newmark time loop (DESIGN.md section 4 "Newmark"); writes profiles/newmark_step.json.

  python tools/newmark_profile.py [M] [steps]    3D P1 elasticity on an M^3-cell cube (default 94: 2.6 million dofs, beyond the
                                                 caches), `steps` time steps (default 10) of dt = 0.025, beta 1/4, gamma 1/2,
                                                 ramped volume load, CG to 1e-8 with one-level Schwarz (Full combine)

What it records, all from the library's HIP-event timers of a device-synchronised loop:
  - per step: state kernel (k_newmark), block apply (k_block_apply), Dirichlet values, solve (SpMV + Schwarz apply + CG sweeps),
    and the iterations, once with the previous solution as the start value (fedd_cg_x0) and once, in a second run of the same
    loop, with a zero start value (fedd_cg)
  - the state kernel's achieved bandwidth on its 56-byte-per-row model (40 in the first step) against the GPU's measured read
    ceiling (fedd_read_bandwidth): the figure DESIGN's 0.7 rule looks at; the block apply's on its 12 nnz + 20 rows model
  - the first step's extra cost: mass assembly, pattern copy + combine, Dirichlet rows, Schwarz setup, the solver's SpMV setup
Not wired into bench.py.  Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/newmark_profile.py ...`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from feddlib_amd import capi  # noqa: E402

MU, NU, RHO, FORCE = 0.5e6, 0.4, 1000.0, -7.0
DT, BETA, GAMMA, T_RAMP = 0.025, 0.25, 0.5, 0.1
RTOL = 1e-8
PER_STEP = ("newmark_state", "block_apply", "dirichlet", "spmv", "schwarz_apply", "cg_pq", "cg_xr", "cg_rz", "cg_p")
FIRST = ("symbolic", "assemble", "rhs", "dirichlet", "schwarz_setup", "spmv_setup")


def snapshot(c):
    c.sync()
    return {k: v[0] for k, v in c.timing_get().items()}


def loop(M, steps, start_from_previous):
    lam = 2.0 * MU * NU / (1.0 - 2.0 * NU)
    c = capi.Context(device=0)
    c.timing_enable(1)
    c.mesh_set_dict(capi.structured_mesh(3, 1, M))
    c.pattern_build(3, capi.BLOCK_FULL)
    c.assemble(capi.FORM_LINELAS, [lam, MU])
    c.matrix_store(1)
    c.assemble_rhs([0.0, 1.0, 0.0])
    f_unit = c.rhs_get()
    t0 = snapshot(c)
    c.pattern_build(3, capi.BLOCK_DIAG)
    c.assemble(capi.FORM_MASS_VEC)
    c.matrix_scale(-1, RHO)
    c.matrix_store(0)
    t1 = snapshot(c)
    n = c.csr_sizes()[0]
    cm = 1.0 / ((DT * DT) * BETA)
    out = {"dofs": int(n), "mass_assembly_ms": {k: t1[k] - t0[k] for k in ("symbolic", "assemble")}, "steps": []}
    for s in range(steps):
        before = snapshot(c)
        fresh = not c.matrix_combine_current(0, cm, 1, 1.0)
        if fresh:
            c.matrix_combine(0, cm, 1, 1.0)
        if s == 0:
            c.newmark_begin()
        c.newmark_advance(0, DT, BETA, GAMMA, 1.0)
        c.rhs_axpy(FORCE * min((s + 1) * DT / T_RAMP, 1.0), f_unit)
        if fresh:
            c.dirichlet([2], np.zeros(3))
            c.schwarz_setup(1, capi.COMBINE_FULL)
        else:
            c.dirichlet_rhs([2], np.zeros(3))
        if start_from_previous:
            _, its, rel = c.cg_x0(None, None, rtol=RTOL, max_it=5000, use_prec=True)
        else:
            _, its, rel = c.cg(None, rtol=RTOL, max_it=5000, use_prec=True, want_x=False)
        after = snapshot(c)
        d = {k: after[k] - before[k] for k in after}
        rec = {"step": s + 1, "iterations": int(its), "relres": float(rel), "fresh_matrix": bool(fresh),
               "ms": {k: d[k] for k in PER_STEP}, "solve_ms": sum(d[k] for k in PER_STEP[3:])}
        if fresh:
            rec["first_step_extra_ms"] = {k: d[k] for k in FIRST}
        out["steps"].append(rec)
    sampled = c.timing_get_sampled()
    for name in ("newmark_state", "block_apply"):
        ms, launches, nbytes = sampled[name]
        out[name] = {"launches": int(launches), "ms_total": ms, "model_bytes_total": nbytes,
                     "GBs_on_model": nbytes / ms / 1e6 if ms > 0 else None}
    # the steady-state launches of the state kernel alone (the first step moves 40 bytes per row)
    later = [r["ms"]["newmark_state"] for r in out["steps"][1:]]
    if later:
        out["newmark_state"]["steady_ms"] = float(np.median(later))
        out["newmark_state"]["steady_GBs_on_56_bytes_per_row"] = 56.0 * n / float(np.median(later)) / 1e6
    return c, out


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 94
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    c, prev = loop(M, steps, True)
    ceiling = c.read_bandwidth(min(2 << 30, max(64 << 20, 56 * prev["dofs"])), 10)
    c.close()
    c, zero = loop(M, steps, False)
    c.close()
    out = {"mesh": "P1, %d^3 cells" % M, "dt": DT, "beta": BETA, "gamma": GAMMA, "rtol": RTOL, "read_ceiling_GBs": ceiling,
           "start_from_previous_solution": prev, "zero_start_value": {"steps": zero["steps"]}}
    st = prev["newmark_state"].get("steady_GBs_on_56_bytes_per_row")
    if st:
        out["state_kernel_fraction_of_read_ceiling"] = st / ceiling
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "newmark_step.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    its_p = [r["iterations"] for r in prev["steps"]]
    its_z = [r["iterations"] for r in zero["steps"]]
    print(json.dumps({"written": path, "dofs": prev["dofs"], "iterations_previous": its_p, "iterations_zero": its_z,
                      "state_kernel": prev["newmark_state"], "block_apply": prev["block_apply"], "read_ceiling_GBs": ceiling,
                      "state_fraction": out.get("state_kernel_fraction_of_read_ceiling"),
                      "first_step_extra_ms": prev["steps"][0].get("first_step_extra_ms"), "step2_ms": prev["steps"][1]["ms"] if steps > 1 else None}))


if __name__ == "__main__":
    main()
