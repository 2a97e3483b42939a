"""Plain numpy fp64 references of the fidelity statistics (test infrastructure; written from the definitions in
include/scrabble_hip.h and scrabble_gan_amd/fidelity.py's docstrings, independently of the product code): moments, covariance,
polynomial-kernel Gram sums with explicit loops over tiles, the unbiased MMD^2 estimator and the Frechet distance."""
import numpy as np

U = 2.0 ** -53          # unit roundoff of fp64


def moments_ref(x):
    """x [n,D] -> (sum [D], outer [D,D], |x|^T |x| [D,D], sum |x| [D]) in fp64."""
    x = np.asarray(x).astype(np.float64)
    return x.sum(0), x.T @ x, np.abs(x).T @ np.abs(x), np.abs(x).sum(0)


def cov_ref(x):
    """numpy's two-pass mean / unbiased covariance."""
    x = np.asarray(x).astype(np.float64)
    return x.mean(0), np.cov(x, rowvar=False).reshape(x.shape[1], x.shape[1])


def poly_kernel(a, b, gamma, coef0):
    return (gamma * (a @ b.T) + coef0) ** 3


def gram_sums_ref(x, y, ix, iy, gamma, coef0, tile=7):
    """-> (sums [S,3], bound_base [S]) with sums[s] = {sum_{i!=j} k(X_i,X_j), sum_{i!=j} k(Y_i,Y_j), sum_{i,j} k(X_i,Y_j)}, X = x[ix[s]],
    Y = y[iy[s]], by double loops over tiles of the fp64 copies; bound_base[s] = sum_{i,j} (|gamma| |X_i|.|Y_j| + |coef0|)^3."""
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    S, m = ix.shape
    sums, base = np.zeros((S, 3)), np.zeros(S)
    for s in range(S):
        X, Y = x[ix[s]], y[iy[s]]
        for kind, (P, Q) in enumerate(((X, X), (Y, Y), (X, Y))):
            tot = 0.0
            for i0 in range(0, m, tile):
                for j0 in range(0, m, tile):
                    k = poly_kernel(P[i0:i0 + tile], Q[j0:j0 + tile], gamma, coef0)
                    if kind < 2 and i0 == j0:
                        k = k - np.diag(np.diag(k))
                    tot += k.sum()
            sums[s, kind] = tot
        base[s] = ((abs(gamma) * (np.abs(X) @ np.abs(Y).T) + abs(coef0)) ** 3).sum()
    return sums, base


def kid_ref(x, y, ix, iy, gamma, coef0):
    """Unbiased MMD^2 per subset, written directly from the estimator -> (mean, std, per-subset values)."""
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    vals = []
    for s in range(ix.shape[0]):
        X, Y = x[ix[s]], y[iy[s]]
        m = len(X)
        kxx, kyy, kxy = poly_kernel(X, X, gamma, coef0), poly_kernel(Y, Y, gamma, coef0), poly_kernel(X, Y, gamma, coef0)
        vals.append((kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (m * (m - 1)) - 2 * kxy.mean())
    vals = np.array(vals)
    return float(vals.mean()), float(vals.std()), vals


def frechet_samples_ref(xa, xb):
    """The same distance from the two SAMPLE sets, for few rows in many dimensions.  With A = (xa - mean) / sqrt(n_a - 1), B likewise,
    c1 = A^T A and c2 = B^T B, and the non-zero eigenvalues of c1 c2 are those of (A B^T)(A B^T)^T: tr (c1 c2)^(1/2) is the sum
    of the singular values of the small matrix A B^T.  No square root of a rounded zero eigenvalue enters (frechet_ref on singular
    moments carries sqrt(2^-53) per missing rank), so this form is good to fp64 rounding."""
    xa, xb = np.asarray(xa).astype(np.float64), np.asarray(xb).astype(np.float64)
    ma, mb = xa.mean(0), xb.mean(0)
    A, B = (xa - ma) / np.sqrt(len(xa) - 1), (xb - mb) / np.sqrt(len(xb) - 1)
    return float(np.sum((ma - mb) ** 2) + np.sum(A * A) + np.sum(B * B) - 2 * np.linalg.svd(A @ B.T, compute_uv=False).sum())


def frechet_ref(mu1, c1, mu2, c2):
    """|mu1 - mu2|^2 + tr c1 + tr c2 - 2 tr (c1 c2)^(1/2): the trace of the root as the sum of the square roots of the eigenvalues of
    c1^(1/2) c2 c1^(1/2), c1^(1/2) from the symmetric eigendecomposition, eigenvalues clamped at 0."""
    w, v = np.linalg.eigh(c1)
    r = v @ np.diag(np.sqrt(np.clip(w, 0, None))) @ v.T
    ev = np.linalg.eigvalsh(r @ c2 @ r)
    return float(np.sum((mu1 - mu2) ** 2) + np.trace(c1) + np.trace(c2) - 2 * np.sqrt(np.clip(ev, 0, None)).sum())
