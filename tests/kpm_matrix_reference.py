"""Plain-numpy references of the matrix-valued kernel polynomial method for the tests (nothing here is used by the product): the
block Chebyshev recurrence with the matrix doubling formulas on a dense H, the exact moment matrices from an eigendecomposition, a
Gram matrix in extended precision with the forward bound of a sum, and the tolerance rule of kpm_reference.moment_tolerance
applied entry by entry."""
import numpy as np

from kpm_reference import rescale


def recurrence_blocks(H, V0, count, bounds):
    """V_n = T_n(H~) V_0 for n < count, as a list of dense blocks"""
    a, b = rescale(bounds)
    V = np.asarray(V0).astype(np.result_type(H.dtype, np.asarray(V0).dtype, np.float64))
    out = [V]
    if count > 1:
        out.append((H @ V) / a - (b / a) * V)
    for _ in range(2, count):
        out.append((2.0 / a) * (H @ out[-1]) - (2.0 * b / a) * out[-1] - out[-2])
    return out


def recurrence_moment_matrices(H, V0, num_moments, bounds):
    """mu_n = V_0^+ T_n(H~) V_0, n < M, by the recurrence with mu_2n = 2 V_n^+ V_n - mu_0 and mu_2n+1 = 2 V_n^+ V_n+1 - mu_1:
    M / 2 products with H.  -> [M, K, K] complex128, not symmetrised"""
    M = int(num_moments)
    steps = (M + 1) // 2
    V = recurrence_blocks(H, V0, steps + 1, bounds)
    K = V[0].shape[1]
    mu = np.empty((2 * steps, K, K), dtype=np.complex128)
    for n in range(steps):
        xx, xy = V[n].conj().T @ V[n], V[n].conj().T @ V[n + 1]
        if n == 0:
            mu[0], mu[1] = xx, xy
        else:
            mu[2 * n], mu[2 * n + 1] = 2.0 * xx - mu[0], 2.0 * xy - mu[1]
    return mu[:M]


def recurrence_bra_moments(H, Phi, V0, num_moments, bounds):
    """mu_n = Phi^+ T_n(H~) V_0, one order per product: [M, Ka, K] complex128"""
    V = recurrence_blocks(H, V0, int(num_moments), bounds)
    return np.stack([np.asarray(Phi).conj().T @ v for v in V]).astype(np.complex128)


def exact_moment_matrices(evals, U, Va, Vb, num_moments, bounds):
    """mu_n[a][b] = sum_j conj(<j|v_a>) <j|v_b> T_n(E~_j), n < M: [M, Ka, Kb] complex128 (Va = Vb: the moments of one block)"""
    a, b = rescale(bounds)
    theta = np.arccos(np.clip((np.asarray(evals, dtype=np.float64) - b) / a, -1.0, 1.0))
    T = np.cos(np.arange(int(num_moments))[:, None] * theta[None, :])  # [M, J]
    ca, cb = U.conj().T @ np.asarray(Va), U.conj().T @ np.asarray(Vb)  # [J, Ka], [J, Kb]
    return np.einsum("ja,mj,jb->mab", ca.conj(), T, cb).astype(np.complex128)


def entry_scale(Va, Vb):
    """sqrt(mu_0[a][a] mu_0[b][b]) = ||v_a|| ||v_b||: [Ka, Kb]"""
    return np.outer(np.linalg.norm(np.asarray(Va), axis=0), np.linalg.norm(np.asarray(Vb), axis=0))


def matrix_tolerance(reference, exact, scale):
    """the rule of kpm_reference.moment_tolerance per entry: 100 x the largest deviation (over n) of the numpy recurrence from the
    exact moments on the same matrix and start block, with a floor of 1e-13 sqrt(mu_0[a][a] mu_0[b][b]).
    -> (tolerance [Ka, Kb], the recurrence's own deviation [Ka, Kb])"""
    own = np.abs(np.asarray(reference) - np.asarray(exact)).max(axis=0)
    return np.maximum(100.0 * own, 1e-13 * scale), own


def gram_longdouble(A, B):
    """A^+ B accumulated in np.longdouble (clongdouble for complex blocks): [Ka, Kb]"""
    A, B = np.asarray(A), np.asarray(B)
    wide = np.clongdouble if np.iscomplexobj(A) or np.iscomplexobj(B) else np.longdouble
    return A.astype(wide).conj().T @ B.astype(wide)


def gram_bound(A, B):
    """4 (n + 8) 2^-53 ||A_a||_2 ||B_b||_2 per entry: the forward bound n u sum |terms| of an n-term sum in any order (with
    Cauchy-Schwarz on the sum of the magnitudes), the factor 4 for the four real products of a complex one and n + 8 for the
    roundings of the products and the folds: [Ka, Kb]"""
    n = np.asarray(A).shape[0]
    return 4.0 * (n + 8) * 2.0 ** -53 * entry_scale(A, B)
