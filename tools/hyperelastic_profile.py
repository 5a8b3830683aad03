"""Measurements of the hyperelastic assembly (profiles/hyperelastic_assembly.json).

  python tools/hyperelastic_profile.py              both meshes: the P2 mesh of the 64^3-cell cube and the P1 214^3 grid
  python tools/hyperelastic_profile.py p2 [M]       one mesh, in this process: prints its JSON entry
  python tools/hyperelastic_profile.py p1 [M]

Per mesh and material: fedd_assemble_hyperelastic (tangent + force, tangent alone, force alone) next to FEDD_FORM_LINELAS on the
same mesh and pattern in the same process, two warm-up calls and five timed ones each, from the library's HIP-event timer of
the assembly class.  Without a mesh argument every mesh runs as a child process under its own `timeout`, and the results go to
profiles/hyperelastic_assembly.json.  Per-kernel times: run a one-mesh call under `rocprofv3 --kernel-trace --stats -d DIR -o
NAME -- python tools/hyperelastic_profile.py p2` and read DIR/NAME_kernel_stats.csv (k_hyper_elem, k_hyper_gather,
k_hyper_force)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

DEFAULT_M = {"p2": 64, "p1": 214}
STEP_LIMIT_S = 420


def one(kind, M):
    from feddlib_amd import capi
    m = capi.structured_mesh(3, (1, 1, 1), [M] * 3, 0)
    if kind == "p2":
        m = capi.p2_of_p1(m, volume_id=0)
    c = capi.Context(device=0)
    c.mesh_set_dict(m)
    x = m["xyz"]
    # a smooth displacement with gradients of a few percent: det F stays near 1
    c.velocity_set(0.02 * np.stack([np.sin(x[:, 0] + x[:, 1]), np.cos(x[:, 1] - x[:, 2]), np.sin(x[:, 2])], axis=1))
    c.pattern_build(3, capi.BLOCK_FULL)
    nen = int(m["conn"].shape[1])
    out = {"mesh": "%s of %d^3 cells" % (kind.upper(), M), "elements": int(m["conn"].shape[0]), "nodes": int(x.shape[0]),
           "element_block_scratch_bytes": int(m["conn"].shape[0]) * nen * nen * 9 * 8}

    def timed(fn, reps=5):
        fn(); fn()
        c.sync(); c.timing_enable(True); c.timing_reset()
        for _ in range(reps):
            fn()
        c.sync()
        t = c.timing_get_sampled()["assemble"]
        c.timing_enable(False)
        return {"ms_per_call": t[0] / reps, "model_bytes_per_call": t[2] / reps}

    lam, mu = 0.4 / (1.4 * 0.2), 1.0 / 2.8
    out["linelas"] = timed(lambda: c.assemble(capi.FORM_LINELAS, [lam, mu]))
    del out["linelas"]["model_bytes_per_call"]      # that path states no byte model
    for name, model, params in (("neo_hooke", capi.HYPER_NEOHOOKE, [1.0, 0.4]), ("mooney_rivlin", capi.HYPER_MOONEY_RIVLIN, [1.0, 0.4, 1.0]),
                                ("stvk", capi.HYPER_STVK, [lam, mu])):
        for what_name, what in (("both", 3), ("tangent", capi.HYPER_TANGENT), ("force", capi.HYPER_FORCE)):
            e = timed(lambda: c.assemble_hyperelastic(model, params, what))
            e["GBs_on_model"] = e["model_bytes_per_call"] / e["ms_per_call"] / 1e6
            e["vs_linelas"] = e["ms_per_call"] / out["linelas"]["ms_per_call"]
            out["%s_%s" % (name, what_name)] = e
    c.close()
    return out


def main():
    if len(sys.argv) > 1:
        kind = sys.argv[1]
        print(json.dumps(one(kind, int(sys.argv[2]) if len(sys.argv) > 2 else DEFAULT_M[kind])))
        return 0
    res = {}
    for kind in ("p2", "p1"):
        # each GPU step is a process of its own under its own time limit; after a failure nothing more is started
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), kind],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print("step %s ended with status %d: stopping" % (kind, r.returncode), file=sys.stderr)
            return r.returncode
        res[kind] = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "hyperelastic_assembly.json")
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
