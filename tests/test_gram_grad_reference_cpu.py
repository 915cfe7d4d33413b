"""The reference of the reverse pass of the Gram matrix (tests/gram_grad_reference.py) is itself checked here, on the CPU: against
central differences of F = sum(G * K) in long double, against torch autograd of the same F in float64, and — a condition on the
reference alone that the device tests lean on — at an offset of 1e6 the float64 sequence stays within 2^-50 mag of the long-double
truth, entry by entry (every difference is formed from the inputs; an expanded square would be off by orders of magnitude there)."""
import numpy as np
import pytest

from tests import gram_grad_cases as GC
from tests import gram_grad_reference as R

FD_CASES = ("c15", "c33", "s17", "s33", "white_s", "dup_c", "d17")
H = 1e-5


def _F(c, X, X2, variance, ls, diag_add=0.0):
    return np.sum(np.asarray(c["G"], dtype=R.LD) * R.gram(c["kind"], X, X2, variance, ls, diag_add, dtype=R.LD))


@pytest.mark.parametrize("name", FD_CASES)
def test_reference_matches_central_differences(name):
    c = GC.inputs(name)
    grad, _ = GC.truth(name)
    rng = np.random.default_rng(5)
    X, X2, ls = np.array(c["X"], dtype=R.LD), None if c["sym"] else np.array(c["X2"], dtype=R.LD), np.array(c["ls"], dtype=R.LD)

    def fd(f):
        return (f(R.LD(H)) - f(-R.LD(H))) / (2 * R.LD(H))

    def close(got, want, scale):
        # a central difference is off by h^2 / 6 |F'''| = 1.7e-11 |F'''|; at lengthscales of order one and more the third derivative of
        # an entry is within a few tens of the first ones' scale, and long double's rounding (1e-19 / h) is far below that
        assert abs(got - want) <= 1e-9 * scale, (name, float(got), float(want))

    def bump(a, idx, h):
        b = a.copy()
        b[idx] += h
        return b

    scale = float(np.max(np.abs(grad["X"]))) + 1.0
    for _ in range(3):
        i, d = rng.integers(X.shape[0]), rng.integers(X.shape[1])
        close(fd(lambda h: _F(c, bump(X, (i, d), h), X2, c["variance"], ls)), grad["X"][i, d], scale)
        if X2 is not None:
            j = rng.integers(X2.shape[0])
            close(fd(lambda h: _F(c, X, bump(X2, (j, d), h), c["variance"], ls)), grad["X2"][j, d], scale)
    close(fd(lambda h: _F(c, X, X2, c["variance"] + h, ls)), grad["variance"][0], float(abs(grad["variance"][0])) + 1.0)
    for d in range(ls.size):
        close(fd(lambda h: _F(c, X, X2, c["variance"], bump(ls, d, h))), grad["lengthscales"][d], float(np.max(np.abs(grad["lengthscales"]))) + 1.0)
    if c["sym"]:
        close(fd(lambda h: _F(c, X, None, c["variance"], ls, 0.3 + h)), grad["diag"][0], float(abs(grad["diag"][0])) + 1.0)
    else:
        assert grad["diag"][0] == 0.0


@pytest.mark.parametrize("name", ("c33", "s33", "c17", "d30s"))
def test_reference_matches_torch_autograd(name):
    import torch
    c = GC.inputs(name)
    f64 = GC.float64(name)
    X = torch.tensor(c["X"], requires_grad=True)
    X2 = None if c["sym"] else torch.tensor(c["X2"], requires_grad=True)
    ls = torch.tensor(c["ls"], requires_grad=True)
    v = torch.tensor(c["variance"], dtype=torch.float64, requires_grad=True)
    Y = X if X2 is None else X2
    u = (X[:, None, :] - Y[None, :, :]) / ls
    r2 = (u * u).sum(-1)
    if c["kind"] == R.RBF:
        K = v * torch.exp(-0.5 * r2)
    else:
        r = torch.sqrt(r2 + 1e-12)
        K = v * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r2) * torch.exp(-np.sqrt(5.0) * r)
    (torch.tensor(c["G"]) * K).sum().backward()
    pairs = [("X", X.grad), ("variance", v.grad.reshape(1)), ("lengthscales", ls.grad)] + ([] if X2 is None else [("X2", X2.grad)])
    for k, g in pairs:
        want = np.asarray(f64[k], dtype=np.float64)
        assert np.allclose(g.numpy(), want, rtol=1e-10, atol=1e-12 * (1.0 + np.max(np.abs(want)))), k


@pytest.mark.parametrize("name", GC.OFFSET)
def test_offset_cases_keep_float64_inside_the_resolution_of_the_bar(name):
    (tr, mag), f64 = GC.truth(name), GC.float64(name)
    for k in GC.KEYS:
        if tr[k] is None:
            continue
        e64 = np.abs(f64[k] - tr[k]).astype(np.float64)
        assert np.all(e64 <= 2.0 ** -50 * mag[k].astype(np.float64)), (k, float(np.max(e64 / np.maximum(mag[k].astype(np.float64), 1e-300))))


def test_far_pairs_contribute_exact_zeros():
    for name in GC.FAR:
        c, (tr, _) = GC.inputs(name), GC.truth(name)
        far = tr["X2"][4] if name == "far_c" else tr["X"][9]
        assert np.all(far == 0.0) and all(np.all(np.isfinite(tr[k])) for k in GC.KEYS if tr[k] is not None)
