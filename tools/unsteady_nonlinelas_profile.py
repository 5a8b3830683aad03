"""Measurement of a nonlinear Newmark step (DESIGN.md section 4 "Nonlinear Newmark"); writes profiles/unsteady_nonlinelas_step.json.

  python tools/unsteady_nonlinelas_profile.py [--cells M] [--repeats R] [--out FILE]

P1 cube of M^3 cells (default 32), Neo-Hooke E = 1, nu = 0.4, density 1, volume force -0.01 in x, dt = 0.01, beta = 1/4,
gamma = 1/2, one step at the ABI level as tests/test_gpu_newton_newmark.py issues the calls: Newton to 1e-8 of the step's first
residual, GMRES to 1e-10 with one-level Schwarz (restricted) set up again in every iteration.

  step     the library's HIP-event classes over the step (assemble, dirichlet, schwarz setup / apply, spmv, orthogonalisation,
           newton_residual, newton_update, block_apply, newmark_state), the Newton and the GMRES iterations
  tangent  per repeat, at the converged displacement: the fused fedd_assemble_hyperelastic_time(TANGENT) against the unfused
           public sequence fedd_assemble_hyperelastic(TANGENT) -> fedd_matrix_store -> fedd_matrix_combine, wall time of the
           device-synchronised calls; the spread over the repeats is reported so that a difference can be told from noise
  residual k_newton_residual's device time and achieved bandwidth on its modelled bytes (fedd_timing_get_sampled), against the
           GPU's measured read ceiling (fedd_read_bandwidth)
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

E, NU, RHO, FORCE, DT, BETA, GAMMA = 1.0, 0.4, 1.0, -0.01, 0.01, 0.25, 0.5
TOL, RTOL = 1e-8, 1e-10
SLOT_M, SLOT_FREE = 0, 3


def wall(c, fn, *a, **kw):
    c.sync()
    t0 = time.perf_counter()
    fn(*a, **kw)
    c.sync()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unsteady_nonlinelas_step.json"))
    args = ap.parse_args()
    m = capi.structured_mesh(3, 1, args.cells)
    c = capi.Context(device=0)
    c.mesh_set_dict(m)
    c.pattern_build(3, capi.BLOCK_DIAG)
    c.assemble(capi.FORM_MASS_VEC)
    c.matrix_store(SLOT_M)
    c.matrix_scale(SLOT_M, RHO)
    c.pattern_build(3, capi.BLOCK_FULL)
    c.assemble_rhs([FORCE, 0.0, 0.0])
    load = c.rhs_get()
    n = load.shape[0]
    cm = 1.0 / ((DT * DT) * BETA)
    mid, p = capi.HYPER_NEOHOOKE, [E, NU]
    c.solution_set(np.zeros(n))
    c.newmark_begin()
    c.timing_enable(1)
    c.timing_reset()
    c.newmark_advance(SLOT_M, DT, BETA, GAMMA, 1.0)
    c.rhs_axpy(1.0, load)
    c.newton_begin()
    ratios, gmres_its, r0 = [], [], None
    for it in range(26):
        c.assemble_hyperelastic_time(mid, p, SLOT_M, cm)
        c.dirichlet([2])
        nr = c.newton_residual(SLOT_M, cm, [2])
        r0 = nr if r0 is None else r0
        ratios.append(nr / r0)
        if ratios[-1] < TOL:
            break
        c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
        _, its, _ = c.gmres(None, rtol=RTOL, max_it=400, restart=100, use_prec=True, want_x=False)
        gmres_its.append(its)
        c.newton_update(1.0)
    c.sync()
    classes = {k: {"ms": v[0], "launches": v[1]} for k, v in c.timing_get().items() if v[1] > 0}
    sampled = c.timing_get_sampled()["newton_residual"]
    ceiling = c.read_bandwidth(1 << 30, 10) if hasattr(c, "read_bandwidth") else None
    res_ms, res_n, res_bytes = sampled[0], sampled[1], sampled[2]
    residual = {"launches": res_n, "ms_per_launch": res_ms / max(res_n, 1), "modelled_bytes_per_launch": res_bytes / max(res_n, 1),
                "GBs_on_modelled_bytes": (res_bytes / 1e9) / (res_ms / 1e3) if res_ms > 0 else None, "read_ceiling_GBs": ceiling,
                "note": "one lane of every group of 8 / 16 loads b, f, s, u_k and stores r, and Dirichlet rows walk their mass row "
                        "although the sum is discarded: the modelled bytes are the algorithmic ones, not the sectors moved"}
    # fused against unfused, at the displacement the loop ended on (the nodal vector field holds it)
    fused, unfused = [], []
    for _ in range(args.repeats):
        fused.append(wall(c, c.assemble_hyperelastic_time, mid, p, SLOT_M, cm, what=capi.HYPER_TANGENT))

        def sequence():
            c.assemble_hyperelastic(mid, p, capi.HYPER_TANGENT)
            c.matrix_store(SLOT_FREE)
            c.matrix_combine(SLOT_M, cm, SLOT_FREE, 1.0)
        unfused.append(wall(c, sequence))
    c.newton_end()
    tangent = {"fused_ms": fused, "unfused_ms": unfused, "fused_median_ms": float(np.median(fused)),
               "unfused_median_ms": float(np.median(unfused)), "fused_spread_ms": float(max(fused) - min(fused)),
               "unfused_spread_ms": float(max(unfused) - min(unfused)),
               "note": "the first repeat of each includes what the library builds once (gather lists; the first store's allocation)"}
    out = {"mesh": {"cells": args.cells, "rows": int(n), "nnz": int(c.csr_sizes()[2])},
           "settings": {"model": "Neo-Hooke", "E": E, "nu": NU, "density": RHO, "force": FORCE, "dt": DT, "beta": BETA, "gamma": GAMMA,
                        "newton_tol": TOL, "gmres_rtol": RTOL},
           "step": {"newton_ratios": ratios, "gmres_iterations": gmres_its, "classes": classes},
           "tangent": tangent, "residual": residual}
    c.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"tangent": {k: tangent[k] for k in ("fused_median_ms", "unfused_median_ms", "fused_spread_ms", "unfused_spread_ms")},
                      "residual": residual, "newton_iterations": len(ratios) - 1}))


if __name__ == "__main__":
    main()
