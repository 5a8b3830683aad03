"""Measurement of the stress-form assembly (fedd_assemble_stress, DESIGN.md section 4 "Stress form") next to FEDD_FORM_LINELAS on
the same mesh and pattern; writes profiles/stress_assemble.json.

  python tools/stress_profile.py [--cells M] [--reps K] [--out FILE]

One P2 cube of M^3 cells (default 32: 196608 tetrahedra, 274625 nodes), the FULL pattern of fedd_pattern_build(3, FULL).  Both
forms write the same CSR values array, so FEDD_FORM_LINELAS (mu = 1, lambda = 0: the same matrix) is the comparator.  Per form:
two warm-up calls (the first builds lists and tables), then K calls each closed by a device synchronise under a host clock,
the two forms alternating; the library's HIP-event timer of the same calls beside it.  Reported per form: the median, minimum
and maximum ms per call, the modelled bytes and their share of the GPU's measured read ceiling (fedd_read_bandwidth) and of
the 8 TB/s HBM peak.  The byte model of the stress form is the one its launch states (connectivity, vertices and c once; the
packed pair blocks written and read once; the values written; the lists read); for LINELAS the compulsory traffic alone --
connectivity and vertices once, the values written -- since its kernels keep no scratch.  Also: the largest difference of the
two results relative to a row's largest magnitude.  Not wired into bench.py."""
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


def summary(ms, event_ms, nbytes, ceiling):
    med = statistics.median(ms)
    return dict(ms_per_call_median=med, ms_min=min(ms), ms_max=max(ms), event_ms_per_call=event_ms, modelled_bytes=nbytes,
                gbytes_per_s=nbytes / med / 1e6, fraction_of_read_ceiling=nbytes / (med * 1e-3) / ceiling,
                fraction_of_hbm_peak=nbytes / (med * 1e-3) / HBM_PEAK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stress_assemble.json"))
    a = ap.parse_args()
    m = capi.p2_of_p1(capi.structured_mesh(3, 1, a.cells), volume_id=0)
    n_elem, nen, n_node, dim = m["conn"].shape[0], 10, m["xyz"].shape[0], 3
    c = capi.Context(device=0)
    c.mesh_set_dict(m)
    nnz = c.pattern_build(dim, capi.BLOCK_FULL)
    nq = capi.fe_quadrature(dim, 2)[1].shape[0]
    coeff = np.random.default_rng(1).uniform(0.5, 2.0, (n_elem, nq))
    forms = {"stress": lambda: c.assemble_stress(), "stress_coeff": lambda: c.assemble_stress(coeff),
             "linelas": lambda: c.assemble(capi.FORM_LINELAS, [0.0, 1.0])}
    for fn in forms.values():
        fn(); fn()
    ms = {k: [] for k in forms}
    ev = {}
    c.timing_enable(1)
    for _ in range(a.reps):
        for k, fn in forms.items():
            c.timing_reset()
            ms[k].append(timed(c, fn))
            ev.setdefault(k, []).append(c.timing_get()["assemble"][0])
    c.timing_enable(0)
    ceiling = c.read_bandwidth() * 1e9
    npair = nen * (nen + 1) // 2
    geo = n_elem * nen * 4.0 + n_node * dim * 8.0
    stress_bytes = geo + n_elem * 2.0 * npair * dim * dim * 8.0 + nnz * 8.0 + (nnz // (dim * dim)) * 4.0
    model = {"stress": stress_bytes, "stress_coeff": stress_bytes + n_elem * nq * 8.0, "linelas": geo + nnz * 8.0}
    forms["linelas"]()
    E = c.csr_get()
    forms["stress"]()
    S = c.csr_get()
    scale = np.maximum.reduceat(np.abs(E[2]), E[0][:-1])
    diff = float((np.abs(S[2] - E[2]) / np.repeat(scale, np.diff(E[0]))).max())
    out = dict(mesh=dict(cells=a.cells, n_elem=int(n_elem), n_node=int(n_node), nnz=int(nnz), nq=int(nq)), reps=a.reps,
               read_ceiling_gbytes_per_s=ceiling / 1e9, hbm_peak_gbytes_per_s=HBM_PEAK / 1e9,
               scratch_bytes=int(n_elem * npair * dim * dim * 8),
               upload_note="stress_coeff includes the host-to-device copy of c (n_elem * nq doubles) inside the call",
               stress_vs_linelas_max_rel_diff=diff,
               forms={k: summary(ms[k], statistics.median(ev[k]), model[k], ceiling) for k in forms})
    c.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
