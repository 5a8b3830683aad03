"""The FSI coupling entries, measured on one device.

    python tools/fsi_profile.py [--cells 64] [--cube-cells 64] [--reps 10] [--out profiles/fsi_coupled.json]

Cases
  match   fedd_interface_match of two P1 cubes with cube-cells^3 cells that share the face x = 1 ((cube-cells + 1)^2 interface
          nodes): device time of k_iface_rank + k_iface_scatter from the library's timer "fsi_match" (both sides), the
          comparisons per second against the model n^2 per side, and the wall time of the call (it also reads flags and
          coordinates back and uploads the points).
  merge   fedd_fsi_merge of a P2 / P1 Stokes fluid and a P2 linear-elasticity structure on cells^2 cells each: the cold merge
          (count / scan / fill; a changed mask forces it) and the values-only merge, timer "fsi_merge" and wall time, with the
          byte model 24 nnz + 8 n (cold fill) / 16 nnz + 8 n (values only).
  apply   one FaCSI apply on that system (fedd_schwarz_apply_device): timer "fsi_apply" (k_facsi_inject + k_facsi_rows) next
          to the children's "schwarz_apply", and the byte model of the two kernels from the library's counters."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feddlib_amd import capi  # noqa: E402

FLAG = 7


def side(m, shift):
    m = dict(m)
    m["xyz"] = np.array(m["xyz"], dtype=np.float64, copy=True)
    m["xyz"][:, 0] += shift
    on = np.abs(m["xyz"][:, 0] - 1.0) < 1e-12
    m["xyz"][on, 0] = 1.0
    pos = {int(g): i for i, g in enumerate(m["gid_rep"])}
    xu = np.array([m["xyz"][pos[int(g)], 0] for g in m["gid_uni"]])
    m["flag_uni"] = np.array(m["flag_uni"], dtype=np.int32, copy=True)
    m["flag_uni"][xu == 1.0] = FLAG
    return m, xu


def wall(call, sync):
    sync()
    t0 = time.perf_counter()
    call()
    sync()
    return (time.perf_counter() - t0) * 1e3


def match_case(cells, reps):
    m = capi.structured_mesh(3, 1, cells)
    (mf, _), (ms, _) = side(m, 0.0), side(m, 1.0)
    f, s = capi.Context(device=0), capi.Context(device=0)
    try:
        f.mesh_set_dict(mf)
        s.mesh_set_dict(ms)
        f.timing_enable(True)
        n = f.interface_match(s, [FLAG])
        f.timing_reset()
        ms_wall = [wall(lambda: f.interface_match(s, [FLAG]), f.sync) for _ in range(reps)]
        dev_ms, launches, _ = f.timing_get_sampled()["fsi_match"]
        return {"mesh": "two P1 cubes, %d^3 cells" % cells, "interface_nodes": n, "tile_points": f.interface_match_info()["tile_points"],
                "device_ms_per_match": dev_ms / reps, "timed_launches_per_match": launches / reps,
                "comparisons_per_second": 2.0 * n * n / (dev_ms / reps * 1e-3), "wall_ms_per_match": float(np.median(ms_wall))}
    finally:
        f.close()
        s.close()


def coupled_case(cells, reps):
    dim, dt = 2, 0.05
    p2 = capi.p2_of_p1(capi.structured_mesh(2, 1, cells), volume_id=0)
    n_p1 = (cells + 1) ** 2
    (mf, xf), (ms, xs) = side(p2, 0.0), side(p2, 1.0)
    f, s, c = capi.Context(device=0), capi.Context(device=0), capi.Context(device=0)
    try:
        f.mesh_set_dict(mf)
        f.pattern_build(dim, capi.BLOCK_DIAG)
        f.assemble(capi.FORM_LAPLACE_VEC)
        f.matrix_store(0)
        f.assemble_div(n_p1, 1, 2)
        f.matrix_scale(1, -1.0)
        f.matrix_scale(2, -1.0)
        f.block_merge(0, 2, 1, -1)
        yf = np.array([mf["xyz"][i, 1] for i in range(mf["xyz"].shape[0])])
        bc = np.nonzero((xf < 1e-12) | (yf < 1e-12) | (yf > 1 - 1e-12))[0]
        f.dirichlet_rows((dim * bc[:, None] + np.arange(dim)[None, :]).ravel().astype(np.int32), np.zeros(dim * bc.shape[0]))
        s.mesh_set_dict(ms)
        s.pattern_build(dim, capi.BLOCK_FULL)
        s.assemble(capi.FORM_LINELAS, [1.0, 1.0])
        far = np.nonzero(xs > 2.0 - 1e-12)[0]
        s.dirichlet_nodes(far.astype(np.int32), np.zeros((far.shape[0], dim)))
        n_pairs = f.interface_match(s, [FLAG])
        n_l = dim * n_pairs
        c.timing_enable(True)
        masks = [np.ones(n_l, dtype=np.uint8), np.ones(n_l, dtype=np.uint8)]
        masks[1][0] = 0
        c.fsi_merge(f, s, dt, masks[1])
        c.timing_reset()
        cold_wall = [wall(lambda k=k: c.fsi_merge(f, s, dt, masks[k % 2]), c.sync) for k in range(reps)]
        cold_ms, _, cold_bytes = c.timing_get_sampled()["fsi_merge"]
        c.fsi_merge(f, s, dt)
        c.timing_reset()
        val_wall = [wall(lambda: c.fsi_merge(f, s, dt), c.sync) for _ in range(reps)]
        val_ms, _, val_bytes = c.timing_get_sampled()["fsi_merge"]
        assert c.fsi_info()["last_values_only"]
        n, _, nnz = c.csr_sizes()
        i_f = f.interface_match_table()[0]
        f.dirichlet_rows((dim * i_f[:, None].astype(np.int64) + np.arange(dim)[None, :]).ravel().astype(np.int32), np.zeros(n_l))
        f.schwarz_setup(1, capi.COMBINE_RESTRICTED)
        s.schwarz_setup(1, capi.COMBINE_RESTRICTED)
        c.fsi_prec_attach(f, s)
        for ch in (f, s):
            ch.timing_enable(True)
        c.schwarz_apply_device(2)
        c.sync()
        for ch in (c, f, s):
            ch.timing_reset()
        ap_wall = wall(lambda: c.schwarz_apply_device(reps), c.sync)
        ap_ms, _, ap_bytes = c.timing_get_sampled()["fsi_apply"]
        return {"mesh": "P2 / P1 Stokes and P2 elasticity, %d^2 cells each" % cells, "rows": n, "nnz": nnz, "interface_dofs": n_l,
                "merge_cold": {"device_ms": cold_ms / reps, "wall_ms": float(np.median(cold_wall)), "model_bytes": cold_bytes / reps},
                "merge_values_only": {"device_ms": val_ms / reps, "wall_ms": float(np.median(val_wall)), "model_bytes": val_bytes / reps},
                "apply": {"fsi_kernels_ms": ap_ms / reps, "fsi_kernels_model_bytes": ap_bytes / reps,
                          "fluid_schwarz_apply_ms": f.timing_get_sampled()["schwarz_apply"][0] / reps,
                          "structure_schwarz_apply_ms": s.timing_get_sampled()["schwarz_apply"][0] / reps,
                          "wall_ms_per_apply": ap_wall / reps}}
    finally:
        for x in (c, f, s):
            x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--cube-cells", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsi_coupled.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "match": match_case(a.cube_cells, a.reps), "coupled": coupled_case(a.cells, a.reps)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
