#!/usr/bin/env python3
"""Writes tests/golden/hyperelastic_materials.npz: what the reference's four generated material routines (nh3d, mr3d, stvk3d,
stvk2d of feddlib/core/FE/FE_def.hpp) return for a set of deformation gradients -- recorded results, data only.

Build-machine only, like make_ref_tables.py (it reads the reference tree, FEDD_REFERENCE or /root/reference; nothing at test
time does).  At run time it cuts the four routines out of FE_def.hpp into a temporary directory, compiles them there with g++
behind a flat C interface, calls them through ctypes and removes the directory.  This file holds none of their text.

Per model: two parameter sets x about 20 deformation gradients with det F > 0.2 (identity, rotations, stretches, shears and
seeded random perturbations of the identity).  Arrays, all float64:
    <key>_params [n, 3]   as the routine takes them: (E, nu, 0) | (E, nu, C) | (lambda, mu, 0)
    <key>_F      [n, d, d]
    <key>_P      [n, d, d]
    <key>_A      [n, d, d, d, d]      A[i][j][k][l] as the routine fills Amat
for key in nh3d, mr3d, stvk3d, stvk2d."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REF = os.environ.get("FEDD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROUTINES = {"nh3d": (3, 2), "mr3d": (3, 3), "stvk3d": (3, 2), "stvk2d": (2, 2)}     # name -> (dim, scalar parameters)


def cut_routine(text, name):
    """the definition `void FE<SC,LO,GO,NO>::name(...) { ... }` as a free function"""
    m = re.search(r"void\s+FE<SC,LO,GO,NO>::%s\s*\(" % name, text)
    if m is None:
        raise RuntimeError("routine %s not found" % name)
    open_brace = text.index("{", m.end())
    depth, k = 0, open_brace
    while True:
        if text[k] == "{":
            depth += 1
        elif text[k] == "}":
            depth -= 1
            if depth == 0:
                break
        k += 1
    return "static void %s(" % name + text[m.end():k + 1] + "\n"


def wrapper(name, dim, npar):
    """flat C interface: name_flat(const double* par, const double* F, double* P, double* A)"""
    args = ", ".join("&par[%d]" % i for i in range(npar))
    return """
extern "C" void %(n)s_flat(const double* par_in, const double* Fin, double* Pout, double* Aout) {
    const int d = %(d)d;
    std::vector<double> v(4096, 0.0), par(par_in, par_in + 3), Fs(Fin, Fin + d * d), Ps(d * d, 0.0), As(d * d * d * d, 0.0);
    std::vector<double*> F(d), P(d), A1(d * d * d);
    std::vector<double**> A2(d * d);
    std::vector<double***> A3(d);
    for (int i = 0; i < d; ++i) { F[i] = &Fs[i * d]; P[i] = &Ps[i * d]; }
    for (int i = 0; i < d * d * d; ++i) A1[i] = &As[i * d];
    for (int i = 0; i < d * d; ++i) A2[i] = &A1[i * d];
    for (int i = 0; i < d; ++i) A3[i] = &A2[i * d];
    %(n)s(v.data(), %(a)s, F.data(), P.data(), A3.data());
    for (int i = 0; i < d * d; ++i) Pout[i] = Ps[i];
    for (int i = 0; i < d * d * d * d; ++i) Aout[i] = As[i];
}
""" % dict(n=name, d=dim, a=args)


def gradients(dim, rng, n_random=12):
    I = np.eye(dim)
    out = [I.copy()]
    th = 0.7
    R = np.eye(dim)
    R[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    out.append(R)
    if dim == 3:
        R2 = np.eye(3)
        R2[1:, 1:] = [[np.cos(1.9), -np.sin(1.9)], [np.sin(1.9), np.cos(1.9)]]
        out.append(R2 @ R)
    out.append(np.diag([1.3, 0.8, 1.1][:dim]))
    out.append(np.diag([0.6, 0.7, 0.9][:dim]))
    S = I.copy(); S[0, 1] = 0.4
    out.append(S)
    out.append(R @ np.diag([1.2, 0.9, 1.05][:dim]))
    for amp in (0.05, 0.3):
        for _ in range(n_random // 2):
            out.append(I + amp * rng.uniform(-1.0, 1.0, (dim, dim)))
    F = np.stack(out)
    det = np.linalg.det(F)
    assert det.min() > 0.2, det.min()
    return F


def main():
    text = open(os.path.join(REF, "feddlib", "core", "FE", "FE_def.hpp")).read()
    src = "#include <cmath>\n#include <vector>\n#define Power(x, y) (std::pow((double)(x), (double)(y)))\n#define Sqrt(x) (std::sqrt((double)(x)))\n"
    for name, (dim, npar) in ROUTINES.items():
        src += cut_routine(text, name) + wrapper(name, dim, npar)
    params = {"nh3d": [(3.0e6, 0.4, 0.0), (1.0, 0.25, 0.0)],
              "mr3d": [(3.0e6, 0.4, 1.0), (2.5, 0.3, 0.35)],
              "stvk3d": [(4.0e6 / 1.4 * 0.4 / 0.2, 2.0e6 / 1.4 * 0.7, 0.0), (1.5, 0.8, 0.0)],
              "stvk2d": [(4.2857142857142857e6, 1.0714285714285714e6, 0.0), (0.7, 1.3, 0.0)]}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        cpp, so = os.path.join(tmp, "materials.cpp"), os.path.join(tmp, "materials.so")
        with open(cpp, "w") as fh:
            fh.write(src)
        subprocess.run(["g++", "-O0", "-ffp-contract=off", "-shared", "-fPIC", cpp, "-o", so], check=True)
        L = ctypes.CDLL(so)
        dp = ctypes.POINTER(ctypes.c_double)
        rng = np.random.default_rng(20240611)
        for name, (dim, npar) in ROUTINES.items():
            fn = getattr(L, name + "_flat")
            fn.argtypes = [dp, dp, dp, dp]
            fn.restype = None
            Fs = gradients(dim, rng)
            rec = {"params": [], "F": [], "P": [], "A": []}
            for par in params[name]:
                for F in Fs:
                    p = np.ascontiguousarray(par, dtype=np.float64)
                    Fc = np.ascontiguousarray(F, dtype=np.float64)
                    P = np.zeros((dim, dim)); A = np.zeros((dim,) * 4)
                    fn(p.ctypes.data_as(dp), Fc.ctypes.data_as(dp), P.ctypes.data_as(dp), A.ctypes.data_as(dp))
                    assert np.isfinite(P).all() and np.isfinite(A).all()
                    rec["params"].append(p); rec["F"].append(Fc); rec["P"].append(P); rec["A"].append(A)
            for k, v in rec.items():
                out["%s_%s" % (name, k)] = np.stack(v)
    path = os.path.join(HERE, "hyperelastic_materials.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items() if k.endswith("_F")})


if __name__ == "__main__":
    sys.exit(main())
