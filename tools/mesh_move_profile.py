"""One step of a moving-mesh loop, measured two ways on the same build: fedd_mesh_move against fedd_mesh_set with the moved
coordinates (the only way before fedd_mesh_move; unchanged by it).  A step is: new coordinates, pattern build, assemble,
right-hand side, Dirichlet, Schwarz setup, GMRES.  Wall clock around a device synchronise, steady state (the first steps warm
up), the two variants alternating.  Also the device time and the byte-model bandwidth of k_mesh_move and k_move_check from
the library's timers.

    python tools/mesh_move_profile.py [--cells 64] [--steps 6] [--out profiles/mesh_move.json]

Case: 3D P1 Laplace on the unit cube, cells^3 cells.  (The P2 / P1 Stokes case on the 6k cylinder is not covered yet.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feddlib_amd import capi  # noqa: E402


def displacement(x, h, amp, phase):
    bubble = np.prod(np.sin(np.pi * x), axis=1)
    cols = [bubble * np.cos(2.1 * x[:, (k + 1) % 3] + 0.7 * k + phase) * np.sin(1.7 * x[:, k] + 1.1 + phase) for k in range(3)]
    d = amp * h * np.stack(cols, axis=1)
    d[np.any((x == 0.0) | (x == 1.0), axis=1)] = 0.0
    return d


def step(c, rtol):
    c.pattern_build(1, capi.BLOCK_SCALAR)
    c.assemble(capi.FORM_LAPLACE)
    c.assemble_rhs([1.0])
    c.dirichlet([1, 2, 3])
    c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
    _, its, rel = c.gmres(rtol=rtol, max_it=400, restart=100, want_x=False)
    c.sync()
    return its, rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_move.json"))
    a = ap.parse_args()
    m = capi.structured_mesh(3, 1, a.cells)
    h = 1.0 / a.cells
    disps = [displacement(m["xyz"], h, 0.2, 0.3 * k) for k in range(a.steps + 2)]
    moved = capi.Context(device=0)
    fresh = capi.Context(device=0)
    moved.mesh_set_dict(m)
    moved.timing_enable(True)
    t_move, t_set, its_move, its_set = [], [], [], []
    sym0 = None
    for k, d in enumerate(disps):
        t0 = time.perf_counter()
        moved.mesh_move(d)
        its, _ = step(moved, a.rtol)
        t1 = time.perf_counter()
        mm = dict(m)
        mm["xyz"] = m["xyz"] + d
        t2 = time.perf_counter()
        fresh.mesh_set_dict(mm)
        its2, _ = step(fresh, a.rtol)
        t3 = time.perf_counter()
        if k == 1:
            sym0 = moved.timing_get()["symbolic"][1]
        if k >= 2:      # the first two steps build the per-mesh structures and warm the code objects up
            t_move.append(1e3 * (t1 - t0))
            t_set.append(1e3 * (t3 - t2))
            its_move.append(its)
            its_set.append(its2)
    smp = moved.timing_get_sampled()
    kern = {}
    for name in ("mesh_move", "move_check"):
        ms, n, nbytes = smp[name]
        kern[name] = {"launches": n, "ms_per_launch": ms / max(n, 1), "model_bytes_per_launch": nbytes / max(n, 1),
                      "GBs_on_the_byte_model": (nbytes / 1e9) / (ms / 1e3) if ms > 0 else None}
    out = {"case": "3D P1 Laplace, unit cube, %d^3 cells, %d dofs" % (a.cells, m["xyz"].shape[0]), "steps_timed": len(t_move),
           "step": "new coordinates + pattern build + assemble + rhs + Dirichlet + Schwarz setup (one level, RAS) + GMRES(rtol %g), "
                   "host wall clock around a device synchronise" % a.rtol,
           "ms_per_step_mesh_move": {"median": float(np.median(t_move)), "all": t_move},
           "ms_per_step_mesh_set": {"median": float(np.median(t_set)), "all": t_set},
           "gmres_iterations": {"mesh_move": its_move, "mesh_set": its_set},
           "symbolic_launches_during_the_timed_steps_mesh_move": moved.timing_get()["symbolic"][1] - sym0,
           "kernels": kern, "move_info": moved.mesh_move_info(),
           "not_measured": "the P2/P1 Stokes case on the 6k cylinder"}
    moved.close()
    fresh.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
