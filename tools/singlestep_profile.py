"""Measurement of the single-step (Runge-Kutta) device layer (DESIGN.md section 4 "Single-step"); writes profiles/singlestep_step.json.

  python tools/singlestep_profile.py [--cells M] [--reps R] [--out FILE]

On the P2 / P1 mesh of an M^3-cell cube (default 32, the size tools/ale_profile.py uses), at the ABI level:

  rhs     fedd_stage_rhs for 1, 2 and 3 prior stages (coeff_bt = 0, "Full implicit pressure") against the same right-hand side
          composed from fedd_matrix_apply and fedd_rhs_axpy calls, next to the byte model: per nonzero of the velocity pattern
          4 B of column index once + 8 B per prior stage in the kernel, 12 B per prior stage + vector passes in the composition.
          The composition passes through host vectors (that is what those entries take), so its time contains the copies; the
          bytes-only ratio is listed beside the measured one.
  step    the device calls of a Crank-Nicolson step that are not the solve -- stage operator, push, stage system, right-hand side
          -- against those of a BDF2 step (advection pass, merge, fedd_multistep_advance, as tools/unsteady_ns_profile.py issues
          them).  The nonlinear solves are the same work in both and are left out.
  error   fedd_stage_error, both kinds.
Wall time of device-synchronised calls: one warm-up call, then the median of R repeats (default 20).  Not wired into bench.py."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from feddlib_amd import capi  # noqa: E402

SLOT_A, SLOT_B, SLOT_BT, SLOT_F, SLOT_M, SLOT_AT = 0, 1, 2, 4, 5, 6
RHO, NU, DT = 1.0, 0.01, 0.05


def median_ms(c, fn, reps):
    fn()
    c.sync()
    out = []
    for _ in range(reps):
        c.sync()
        t0 = time.perf_counter()
        fn()
        c.sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def nnz_of(c, slot):
    import ctypes as C
    a, b, z = C.c_int64(), C.c_int64(), C.c_int64()
    capi._chk(c._L.fedd_matrix_sizes(c._h, slot, C.byref(a), C.byref(b), C.byref(z)))
    return int(z.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "singlestep_step.json"))
    a = ap.parse_args()
    m1 = capi.structured_mesh(3, 1, a.cells)
    mv = capi.p2_of_p1(m1, volume_id=0)
    dim, nv, n_p = 3, mv["xyz"].shape[0], m1["xyz"].shape[0]
    nvd, n = dim * nv, dim * nv + n_p
    c = capi.Context(device=0)
    c.mesh_set_dict(mv)
    c.pattern_build(dim, capi.BLOCK_DIAG)
    c.assemble(capi.FORM_LAPLACE_VEC)
    c.matrix_scale(-1, RHO * NU)
    c.matrix_store(SLOT_A)
    c.assemble_div(n_p, SLOT_B, SLOT_BT)
    c.pattern_build(dim, capi.BLOCK_DIAG)
    c.assemble(capi.FORM_MASS_VEC)
    c.matrix_store(SLOT_M)
    rng = np.random.default_rng(0)
    U = [rng.standard_normal(n) for _ in range(3)]

    def operator(x, scale=RHO, slot_add=SLOT_A):
        c.velocity_set(x[:nvd])
        c.assemble_advection(capi.ADV_N, scale, slot_add, SLOT_F)

    c.stage_begin(4)
    for j, x in enumerate(U):
        operator(x)
        if j == 0:
            c.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)
        c.solution_set(x)
        c.stage_push(SLOT_F)
    z_f, z_m = nnz_of(c, SLOT_F), nnz_of(c, SLOT_M)
    res = {"mesh": "P2 / P1 of a %d^3-cell cube" % a.cells, "velocity_dofs": nvd, "pressure_dofs": n_p, "nnz_full_pattern": z_f,
           "nnz_mass": z_m, "bytes_per_stage": 8 * z_f + 8 * n, "reps": a.reps, "rhs": [], "timing": "wall ms of device-synchronised calls: median, min, max"}
    cf = np.array([-0.0125, -0.02, -0.03])
    Fx = [None] * 3
    for n_prior in (1, 2, 3):
        kern = median_ms(c, lambda: c.stage_rhs(SLOT_M, SLOT_BT, cf[:n_prior]), a.reps)

        def composed():
            # M u_0 through the history-free path: apply, then one axpy per term (the vectors pass through the host)
            c.rhs_set(np.zeros(n))
            t = np.zeros(n)
            t[:nvd] = c.matrix_apply(SLOT_M, U[0][:nvd])
            c.rhs_axpy(1.0, t)
            for j in range(n_prior):
                t[:nvd] = Fx[j] if Fx[j] is not None else 0.0
                c.rhs_axpy(cf[j], t)

        # the stage operators live in the store, not in slots: the composition applies the slot's current operator n_prior times
        def composed_with_applies():
            for j in range(n_prior):
                Fx[j] = c.matrix_apply(SLOT_F, U[j][:nvd])
            composed()

        comp = median_ms(c, composed_with_applies, max(3, a.reps // 4))
        model_kernel = 4.0 * z_f + 8.0 * z_f * n_prior + 12.0 * z_m + 8.0 * n
        model_comp = 12.0 * z_f * n_prior + 12.0 * z_m + 3 * 8.0 * nvd * (n_prior + 1)
        res["rhs"].append({"n_prior": n_prior, "stage_rhs_ms": kern, "composition_ms": comp,
                           "measured_ratio_composition_over_kernel": comp[0] / kern[0],
                           "model_bytes_kernel": model_kernel, "model_bytes_composition": model_comp,
                           "model_ratio": model_comp / model_kernel,
                           "kernel_gbs_on_model": model_kernel / (kern[0] * 1e-3) / 1e9})
    # ---- the calls of a step that are not the solve ----
    x = U[0]
    das = DT * 0.5

    def cn_step():
        c.stage_begin(2)
        operator(x)
        c.solution_set(x)
        c.stage_push(SLOT_F)
        operator(x, das * RHO, SLOT_AT)
        c.block_merge_scaled(SLOT_F, SLOT_BT, DT, SLOT_B, -1)
        c.stage_rhs(SLOT_M, SLOT_BT, [-das])

    c.matrix_combine(SLOT_M, 1.0, SLOT_A, das)
    c.matrix_store(SLOT_AT)
    operator(x, das * RHO, SLOT_AT)
    c.block_merge_scaled(SLOT_F, SLOT_BT, DT, SLOT_B, -1)
    res["step_crank_nicolson_ms"] = median_ms(c, cn_step, max(3, a.reps // 4))
    c.matrix_combine(SLOT_M, 1.5 / DT, SLOT_A, 1.0)
    c.matrix_store(SLOT_AT)
    operator(x, RHO, SLOT_AT)
    c.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)
    c.multistep_begin(2)
    c.solution_set(x)
    c.multistep_advance(SLOT_M, [1.0 / DT])

    def bdf2_step():
        operator(x, RHO, SLOT_AT)
        c.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)
        c.solution_set(x)
        c.multistep_advance(SLOT_M, [2.0 / DT, -0.5 / DT])

    res["step_bdf2_ms"] = median_ms(c, bdf2_step, max(3, a.reps // 4))
    res["step_ratio_cn_over_bdf2"] = res["step_crank_nicolson_ms"][0] / res["step_bdf2_ms"][0]
    # ---- error norms ----
    c.stage_begin(2)
    for xx in U[:2]:
        operator(xx)
        c.solution_set(xx)
        c.stage_push(SLOT_F)
    res["error_euclidean_ms"] = median_ms(c, lambda: c.stage_error(capi.STAGE_ERR_EUCLIDEAN, -1, 0, 1), a.reps)
    res["error_l2_ms"] = median_ms(c, lambda: c.stage_error(capi.STAGE_ERR_L2, SLOT_M, 0, 1), a.reps)
    res["error_model_bytes"] = {"euclidean": 16.0 * n, "l2": 12.0 * z_m + 16.0 * nvd}
    c.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
