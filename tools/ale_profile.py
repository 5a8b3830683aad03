"""Measurement of the ALE advection pass (fedd_assemble_advection_ale, DESIGN.md section 4 "ALE convection") next to the
unchanged fixed-mesh pass of the matching kind in the same process; writes profiles/ale_advection.json.

  python tools/ale_profile.py [--cells M] [--reps K] [--out FILE]

One P2 cube of M^3 cells (default 32: 196608 tetrahedra, 274625 nodes), moved once by a smooth displacement that vanishes on
the boundary, a smooth velocity and a smooth mesh velocity.  Four calls: FEDD_ADV_N, FEDD_ALE_FIXEDPOINT, FEDD_ADV_NEWTON,
FEDD_ALE_NEWTON, all with scale 1 and no slot_add into the same slot.  Two warm-up rounds (the first builds the structures),
then K rounds in which the four calls alternate, each closed by a device synchronise under a host clock, the library's
HIP-event timer of the same call beside it.  Per call: median, minimum and maximum ms, the bytes of the library's own byte
model (the one its timer records: geometry, nodal fields and connectivity once, the element blocks written and read once, the
FULL values written) and their share of the GPU's measured read ceiling and of the 8 TB/s HBM peak.  The yardstick is the
fixed-mesh call: per pair the measured ratio ALE / fixed (of the medians), the modelled ratio (of the bytes) and the
run-to-run spread of the fixed-mesh call, (max - min) / median.  Not wired into bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from feddlib_amd import capi  # noqa: E402

HBM_PEAK = 8.0e12


def timed(c, fn):
    c.sync()
    t0 = time.perf_counter()
    fn()
    c.sync()
    return 1e3 * (time.perf_counter() - t0)


def fields(x, h):
    s = x.sum(axis=1)
    bubble = np.prod(np.sin(np.pi * x), axis=1)
    d = 0.2 * h * np.stack([bubble * np.cos(2.1 * x[:, (k + 1) % 3] + 0.7 * k) for k in range(3)], axis=1)
    d[np.any((x == 0.0) | (x == 1.0), axis=1)] = 0.0
    u = np.stack([np.sin(1.3 * x[:, 0] + 0.4 * s) + 0.5, np.cos(0.9 * x[:, 1] - 0.7 * s), np.sin(1.1 * x[:, 2]) * np.cos(0.8 * s)], axis=1)
    w = np.stack([0.8 * np.cos(1.7 * x[:, 0] - 0.5 * s), np.sin(1.2 * x[:, 1] + 0.6 * s) - 0.2, 0.7 * np.sin(0.9 * x[:, 2] + 1.3 * x[:, 0])], axis=1)
    return d, u, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ale_advection.json"))
    a = ap.parse_args()
    m = capi.p2_of_p1(capi.structured_mesh(3, 1, a.cells), volume_id=0)
    n_elem, n_node = m["conn"].shape[0], m["xyz"].shape[0]
    d, u, w = fields(m["xyz"], 1.0 / a.cells)
    c = capi.Context(device=0)
    c.mesh_set_dict(m)
    c.mesh_move(d)
    c.velocity_set(u)
    c.mesh_velocity_set(w)
    calls = {"adv_n": lambda: c.assemble_advection(capi.ADV_N, 1.0, -1, 4),
             "ale_fixedpoint": lambda: c.assemble_advection_ale(capi.ALE_FIXEDPOINT, 1.0, -1, 4),
             "adv_newton": lambda: c.assemble_advection(capi.ADV_NEWTON, 1.0, -1, 4),
             "ale_newton": lambda: c.assemble_advection_ale(capi.ALE_NEWTON, 1.0, -1, 4)}
    for _ in range(2):
        for fn in calls.values():
            fn()
    ms = {k: [] for k in calls}
    ev = {k: [] for k in calls}
    nbytes = {}
    c.timing_enable(1)
    for _ in range(a.reps):
        for k, fn in calls.items():
            c.timing_reset()
            ms[k].append(timed(c, fn))
            t = c.timing_get_sampled()["assemble"]
            ev[k].append(t[0])
            nbytes[k] = t[2]
    c.timing_enable(0)
    ceiling = c.read_bandwidth() * 1e9
    info = c.mesh_move_info()
    c.close()

    def summary(k):
        med = statistics.median(ms[k])
        return dict(ms_per_call_median=med, ms_min=min(ms[k]), ms_max=max(ms[k]), event_ms_per_call=statistics.median(ev[k]),
                    modelled_bytes=nbytes[k], gbytes_per_s=nbytes[k] / med / 1e6,
                    fraction_of_read_ceiling=nbytes[k] / (med * 1e-3) / ceiling, fraction_of_hbm_peak=nbytes[k] / (med * 1e-3) / HBM_PEAK)

    def pair(ale, fixed):
        mf = statistics.median(ms[fixed])
        return dict(ale=ale, fixed=fixed, measured_ratio=statistics.median(ms[ale]) / mf,
                    measured_ratio_event_timer=statistics.median(ev[ale]) / statistics.median(ev[fixed]),
                    modelled_ratio=nbytes[ale] / nbytes[fixed], spread_of_fixed=(max(ms[fixed]) - min(ms[fixed])) / mf,
                    spread_of_ale=(max(ms[ale]) - min(ms[ale])) / statistics.median(ms[ale]))

    out = dict(mesh=dict(cells=a.cells, n_elem=int(n_elem), n_node=int(n_node), min_det_ratio=info["min_det_ratio"]), reps=a.reps,
               read_ceiling_gbytes_per_s=ceiling / 1e9, hbm_peak_gbytes_per_s=HBM_PEAK / 1e9,
               calls={k: summary(k) for k in calls},
               ratios=[pair("ale_fixedpoint", "adv_n"), pair("ale_newton", "adv_newton")])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
