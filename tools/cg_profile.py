"""First numbers of preconditioned CG against the default GMRES ("CG"; profiles/cg_vs_gmres.json).

  python tools/cg_profile.py [laplace_M] [elasticity_M]     defaults 100 and 48 (cells per direction of the cube)

Per case: fedd_gmres with restricted Schwarz (the default), fedd_cg with full Schwarz one-level and with the Q1 coarse level;
one warm-up solve and three timed ones each (host clock around synchronised calls): iterations, ms per solve, ms per iteration.
Then one CG solve with the HIP-event timers on: per-launch times of k_full_park_mfma, k_full_park, k_full_gather and the four
sweeps against their byte and flop models."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feddlib_amd import capi  # noqa: E402

RTOL = 1e-8


def setup(kind, M):
    c = capi.Context(device=0)
    c.mesh_set_dict(capi.structured_mesh(3, 1, M))
    if kind == "laplace":
        c.pattern_build(1, capi.BLOCK_SCALAR)
        c.assemble(capi.FORM_LAPLACE)
        c.assemble_rhs([1.0])
        c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    else:
        c.pattern_build(3, capi.BLOCK_FULL)
        c.assemble(capi.FORM_LINELAS, [1.5, 1.0])
        c.assemble_rhs([0.0, 1.0, 0.0])
        c.dirichlet([2], [0.0, 0.0, 0.0])
    return c


def timed(c, solve):
    solve()
    c.sync()
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        _, its, rel = solve()
        c.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return {"iterations": its, "relres": rel, "ms_per_solve": ms[1], "ms_per_iteration": ms[1] / max(its, 1)}


def case(kind, M):
    c = setup(kind, M)
    n = c.csr_sizes()[0]
    out = {"problem": "%s, %d^3 cells" % (kind, M), "rows": int(n), "rtol": RTOL}
    c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
    out["gmres_restricted"] = timed(c, lambda: c.gmres(None, rtol=RTOL, max_it=1000, restart=100, use_prec=True, want_x=False))
    for name, two in (("cg_full", 0), ("cg_full_q1", 1)):
        c.schwarz_setup(1, capi.COMBINE_FULL, two_level=two, coarse_kind=capi.COARSE_Q1 if two else 0)
        out[name] = timed(c, lambda: c.cg(None, rtol=RTOL, max_it=5000, use_prec=True, want_x=False))
        if not two:
            info, full = c.schwarz_info(), c.schwarz_full_info()
            sn = info.get("sum_sizes", 0)
            c.timing_enable(True)
            c.timing_reset()
            c.cg(None, rtol=RTOL, max_it=5000, use_prec=True, want_x=False)
            c.sync()
            t = c.timing_get_sampled()
            c.timing_enable(False)
            model = {"full_park_mfma": "flops 2 sum n_i^2 of its subdomains; park 8 sum n_i", "full_park": "inverses 8 sum n_i^2 of its subdomains",
                     "full_gather": 16.0 * sn + 16.0 * n, "cg_pq": 16.0 * n, "cg_xr": 48.0 * n, "cg_rz": 16.0 * n, "cg_p": 28.0 * n}
            out["kernels"] = {k: {"ms_per_launch": t[k][0] / max(t[k][1], 1), "launches": t[k][1], "model_bytes": model[k]}
                              for k in model}
            out["subdomains"] = dict(info, **full)
    c.close()
    return out


if __name__ == "__main__":
    ml = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    me = int(sys.argv[2]) if len(sys.argv) > 2 else 48
    res = {"cases": [case("laplace", ml), case("elasticity", me)]}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "cg_vs_gmres.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
