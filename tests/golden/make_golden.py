"""Generates tests/golden/golden_<case>.npz from the CPU oracle (oracle/).  The reference itself cannot be imported here
(gpflow 1.1.1 / TF 1.8 unavailable), so these vectors pin the ORACLE + the HIP path against each other and against
regressions; the oracle in turn is pinned relationally by tests/test_oracle_identities.py.

    python -m tests.golden.make_golden [case ...]

Run as a script it pins the BLAS code paths (REPRODUCIBLE_BLAS) before numpy / torch load them: MKL's default kernels differ between
CPU vendors (AVX-512 on Intel, AVX2 on AMD) and OpenBLAS picks its kernels by CPU model, and either changes the last bits of the
oracle's numbers.  tests/test_golden_generator.py regenerates fixtures the same way and compares them to 1e-12.
"""
import os
import sys

# MKL's vendor-independent code path and OpenBLAS's AVX-512 kernels (what it picks itself on AVX-512 hosts): the same bits on Intel
# AVX-512 hosts at any thread count; MKL on AMD hosts still differs in the last bits (5e-13 of the largest entry, multiclass case)
REPRODUCIBLE_BLAS = {"MKL_CBWR": "COMPATIBLE", "OPENBLAS_CORETYPE": "SkylakeX"}
if __name__ == "__main__":
    os.environ.update(REPRODUCIBLE_BLAS)

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "doubly-stochastic-dgp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import dgp_oracle as O  # noqa: E402
from oracle import model as OM  # noqa: E402
from tests.golden import cases, extras  # noqa: E402


def outputs(name):
    spec, state, _, X, Y, zs, c = cases.build(name)
    S = c["S"]
    Fs, Fm, Fv = OM.propagate(spec, state, X, zs, S)
    om = OM.build(O.NP, spec, state, S, c["num_data"])
    kls = np.array([float(l.KL(O.NP)) for l in om.layers])
    elbo, g = OM.elbo_and_grad(spec, state, X, Y, zs, S, num_data=c["num_data"])
    out = dict(elbo=np.array(elbo), kls=kls, source=np.array("oracle"))     # NOT the reference: see DESIGN.md section 3
    for l in range(c["L"]):
        out[f"Fmean{l}"], out[f"Fvar{l}"], out[f"F{l}"] = Fm[l], Fv[l], Fs[l]
    for k, v in g.items():
        if v.size <= 4096:
            out["grad." + k] = v
        else:                     # large q_sqrt gradients: Frobenius norm + leading 16x16 block of every output
            out["gradnorm." + k] = np.array(np.linalg.norm(v))
            out["gradblock." + k] = v[:, :16, :16].copy()
    out.update(extras.oracle_extras(spec, state, X, Y, zs, c))      # predict_y / density, full_cov, 3 Adam steps, natgrad step
    return out


def main(names=None):
    for name in names or cases.CASES:
        out = outputs(name)
        path = os.path.join(HERE, f"golden_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, "elbo", float(out["elbo"]), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
