"""The interface-distance kernel and the scaled vector Laplacian, measured on one device.

    python tools/interface_distance_profile.py [--p1-cells 64] [--p2-cells 32] [--reps 10] [--out profiles/interface_distance.json]

Cases: the P1 mesh of the unit cube with p1-cells^3 cells and the P2 mesh of the cube with p2-cells^3 cells, each with the face
x = 0 (flag 2) as interface.
  distances  device time of k_interface_distance from the library's timer (median-free: total / launches over `reps` timed calls
             after two warm-up calls), its pair rate (nodes x interface points per second) and that rate x 3 dim flops per pair
             (dim differences, dim products, dim - 1 sums and the minimum) against the f64 vector peak.  The microarchitecture
             notes this project follows list the f32 vector peak, 157.3 TFLOP/s; the f64 vector rate of the part is half of it,
             78.6 TFLOP/s (the public datasheet figure), which is the yardstick here.
  assembly   device time of fedd_assemble(FORM_LAPLACE_XDIM) next to FORM_LAPLACE_VEC on the same context, pattern and mesh
             (timer "assemble", total per call), and their ratio.  Byte model of the difference: 8 bytes per element (the
             coefficient) -- the figure the ratio is judged against in DESIGN.md section 4."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feddlib_amd import capi  # noqa: E402

F64_VECTOR_PEAK = 78.6e12


def timed(c, name, call, reps):
    for _ in range(2):
        call()
    c.sync()
    c.timing_reset()
    for _ in range(reps):
        call()
    c.sync()
    ms, n, nbytes = c.timing_get_sampled()[name]
    return ms / reps, n / reps, nbytes / reps


def case(label, m, reps):
    dim = m["dim"]
    c = capi.Context(device=0)
    try:
        c.mesh_set_dict(m)
        c.timing_enable(True)
        n_if = c.interface_distance([2])
        n_node = m["xyz"].shape[0]
        ms, _, _ = timed(c, "interface_distance", lambda: c.interface_distance([2]), reps)
        pairs = float(n_node) * float(n_if)
        rate = pairs / (ms * 1e-3)
        out = {"mesh": label, "nodes": n_node, "elements": int(m["conn"].shape[0]), "interface_points": int(n_if),
               "tile_points": c.interface_distance_info()["tile_points"],
               "distance_kernel": {"ms": ms, "pairs": pairs, "pairs_per_second": rate, "flops_per_pair": 3 * dim,
                                   "fraction_of_f64_vector_peak": rate * 3 * dim / F64_VECTOR_PEAK}}
        c.pattern_build(dim, capi.BLOCK_DIAG)
        c.set_option("asm_zero_eps", 0.0)
        ms_vec, n_vec, _ = timed(c, "assemble", lambda: c.assemble(capi.FORM_LAPLACE_VEC), reps)
        ms_x, n_x, _ = timed(c, "assemble", lambda: c.assemble(capi.FORM_LAPLACE_XDIM, [0.03, 1000.0]), reps)
        f = c.laplace_scale()
        # byte model of FORM_LAPLACE_VEC: connectivity and coordinates read, values written
        model_vec = m["conn"].size * 4.0 + n_node * dim * 8.0 + c.csr_sizes()[2] * 8.0
        out["assembly"] = {"laplace_vec_ms": ms_vec, "laplace_vec_timed_launches_per_call": n_vec, "laplace_xdim_ms": ms_x,
                           "laplace_xdim_timed_launches_per_call": n_x, "ratio_xdim_over_vec": ms_x / ms_vec,
                           "byte_model_ratio": (model_vec + 8.0 * m["conn"].shape[0]) / model_vec,
                           "scaled_elements": int(np.count_nonzero(f == 1000.0))}
        return out
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p1-cells", type=int, default=64)
    ap.add_argument("--p2-cells", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interface_distance.json"))
    a = ap.parse_args()
    p1 = capi.structured_mesh(3, 1, a.p1_cells)
    p2 = capi.structured_mesh_p2(3, 1, a.p2_cells)
    out = {"f64_vector_peak_flops": F64_VECTOR_PEAK, "reps": a.reps,
           "cases": [case("P1 cube, %d^3 cells" % a.p1_cells, p1, a.reps), case("P2 cube, %d^3 cells" % a.p2_cells, p2, a.reps)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
