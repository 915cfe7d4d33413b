"""Lloyd's k-means in numpy, the yardstick of tests/test_gpu_kmeans.py: squared distances by direct differences ((x - z)^2).sum() —
no |x|^2 + |z|^2 - 2 x.z, so nothing cancels on data far from the origin — argmin with the lowest index on ties, and a cluster
without rows keeps its centre (scipy.cluster.vq.kmeans2's missing='warn').

lloyd(X, Z0, iters) returns one record per iteration, so one run of 10 serves every smaller iteration count:
  Z        the centres after the iteration's update
  labels   the iteration's assignment (the one Z was averaged from: what kmeans2 returns), counts its cluster sizes
  inertia  sum_i min_m |x_i - z_m|^2 of that assignment
  margin   the smallest, over the rows and over this and every earlier iteration, of
             (d2_second - d2_best) / (|x_i - xbar|^2 + max_m |z_m - xbar|^2)
           — the distance between the two nearest centres in units of the magnitudes a translation-robust evaluation rounds at.  An
           evaluation correct to a few hundred ulps of those magnitudes gives the same labels whenever the margin stays above 1e-9.
  scale    sum_i (|x_i - xbar|^2 + max_m |z_m - xbar|^2) of that assignment: the magnitude the inertia's rounding error scales with

Precision.  The distances that pick the labels (and the margin) are float64, as described.  The centres between iterations and the
inertia are carried in np.longdouble (64-bit significand on x86) and rounded to float64 when recorded: a float64 centre of
X = N(0, 1) + 1e6 is only representable to 1.2e-10, and a mean summed in float64 there is off by up to 6e-10; from the second iteration
on that error enters the inertia at first order (the centres are no longer the means of the rows assigned to them).  Measured on case g
with float64 centres: the inertia off by 1.5e-9 at iteration 2 and up to 8.2e-9 later, against 2.5e-11 .. 3.3e-11 allowed to the device
— the yardstick would have been 50 to 300 times coarser than the bound it is used with.  On the cases without an offset the two
versions of the centres differ by a few 1e-16."""
import numpy as np

LD = np.longdouble

ROWS = 256      # rows per block of the (rows, M, D) difference array


def sqdist(X, Z):
    """(n, M) squared distances by direct differences"""
    out = np.empty((X.shape[0], Z.shape[0]))
    for a in range(0, X.shape[0], ROWS):
        d = X[a:a + ROWS, None, :] - Z[None, :, :]
        out[a:a + ROWS] = (d * d).sum(2)
    return out


def lloyd(X, Z0, iters, skip=()):
    """`skip`: centre indices left out of the margin (an exact duplicate of another centre ties with it on every row by construction)"""
    X = np.asarray(X, dtype=np.float64)
    Xl = X.astype(LD)
    Zl = np.array(Z0, dtype=np.float64).astype(LD)
    n, M = X.shape[0], Zl.shape[0]
    xbar = X.mean(0)
    xc2 = ((X - xbar) ** 2).sum(1)
    margin = np.inf
    hist = []
    for _ in range(int(iters)):
        Z = Zl.astype(np.float64)
        d2 = sqdist(X, Z)
        labels = np.argmin(d2, axis=1)                       # the first of equal minima
        zmax = float(((Z - xbar) ** 2).sum(1).max())
        dm = d2.copy()
        dm[:, list(skip)] = np.inf
        two = np.partition(dm, 1, axis=1)[:, :2]
        margin = min(margin, float(((two[:, 1] - two[:, 0]) / (xc2 + zmax)).min()))
        counts = np.bincount(labels, minlength=M)
        inertia = float(((Xl - Zl[labels]) ** 2).sum())
        new = Zl.copy()
        for m in np.nonzero(counts)[0]:
            new[m] = Xl[labels == m].mean(0)
        Zl = new
        hist.append(dict(Z=Zl.astype(np.float64), labels=labels.astype(np.int32), counts=counts.astype(np.int64), inertia=inertia,
                         margin=margin, scale=float((xc2 + zmax).sum())))
    return hist
