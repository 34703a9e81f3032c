"""Plain-numpy references of the kernel polynomial method for the tests (nothing here is used by the product): the Chebyshev
recurrence with doubling on a dense matrix, the exact moments from an eigendecomposition, and the tolerance rule that ties the
two together."""
import numpy as np


def rescale(bounds):
    lo, hi = float(bounds[0]), float(bounds[1])
    return 0.5 * (hi - lo), 0.5 * (hi + lo)


def recurrence_moments(H, v0, num_moments, bounds):
    """mu_n = <v0|T_n(H~)|v0>, n < M, by v_{n+1} = 2 H~ v_n - v_{n-1} with mu_2n = 2 <v_n|v_n> - mu_0 and
    mu_2n+1 = 2 <v_n|v_n+1> - mu_1: M / 2 products with H.  v0: [n] or [n, K] -> [M] or [K, M]."""
    a, b = rescale(bounds)
    V = np.asarray(v0)
    single = V.ndim == 1
    V = V.reshape(len(V), -1).astype(np.result_type(H.dtype, V.dtype, np.float64))
    M = int(num_moments)
    steps = (M + 1) // 2
    mu = np.empty((V.shape[1], 2 * steps))
    dot = lambda A, B: np.einsum("ik,ik->k", A.conj(), B).real  # noqa: E731
    prev, cur = None, V
    for n in range(steps):
        if n == 0:
            nxt = (H @ cur) / a - (b / a) * cur
            mu[:, 0], mu[:, 1] = dot(cur, cur), dot(cur, nxt)
        else:
            nxt = (2.0 / a) * (H @ cur) - (2.0 * b / a) * cur - prev
            mu[:, 2 * n] = 2.0 * dot(cur, cur) - mu[:, 0]
            mu[:, 2 * n + 1] = 2.0 * dot(cur, nxt) - mu[:, 1]
        prev, cur = cur, nxt
    mu = mu[:, :M]
    return mu[0] if single else mu


def exact_moments(evals, weights, num_moments, bounds):
    """sum_j w_j T_n((E_j - b) / a), n < M: [M] (weights [J]) or [K, M] (weights [K, J])"""
    a, b = rescale(bounds)
    theta = np.arccos(np.clip((np.asarray(evals, dtype=np.float64) - b) / a, -1.0, 1.0))
    T = np.cos(np.arange(int(num_moments))[:, None] * theta[None, :])  # [M, J]
    return np.asarray(weights, dtype=np.float64) @ T.T


def eigen_weights(H, v0):
    """(E_j, |<j|v0_k>|^2 as [K, J]) of a dense Hermitian matrix"""
    evals, U = np.linalg.eigh(H)
    V = np.asarray(v0).reshape(len(H), -1)
    return evals, (np.abs(U.conj().T @ V) ** 2).T


def moment_tolerance(H, v0, num_moments, bounds, exact):
    """100 x the largest deviation of the numpy recurrence from the exact moments on the same matrix and start vectors, with a
    floor of 1e-13 mu_0: what a correct implementation with another summation order may deviate by.  -> (tolerance per start
    vector [K], the recurrence's own deviation [K])"""
    ref = np.atleast_2d(recurrence_moments(H, v0, num_moments, bounds))
    ex = np.atleast_2d(exact)
    own = np.abs(ref - ex).max(axis=1)
    return np.maximum(100.0 * own, 1e-13 * ex[:, 0]), own
