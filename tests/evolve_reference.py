"""Plain-numpy references of Chebyshev time evolution for the tests (nothing here is used by the product): the exact propagator
from an eigendecomposition, the same Chebyshev series written naively on a dense matrix, and the tolerance rule that ties the two
together."""
import numpy as np

from distributed_matvec_amd.evolve import propagator_coefficients


def exact_propagate(H, psi, t, imaginary=False, reference_energy=0.0, eig=None):
    """e^{-iHt} psi, or e^{-t (H - E_ref)} psi, from numpy.linalg.eigh (eig: its (eigenvalues, eigenvectors) when the caller has
    them already); psi: [n] or [n, K]"""
    evals, U = np.linalg.eigh(H) if eig is None else eig
    phase = np.exp(-t * (evals - reference_energy)) if imaginary else np.exp(-1j * t * evals)
    V = np.asarray(psi)
    coef = U.conj().T @ V
    return U @ (phase.reshape((-1,) + (1,) * (V.ndim - 1)) * coef)


def series_propagate(H, psi, t, bounds, eps=1e-12, imaginary=False, reference_energy=None):
    """prefactor * sum_n c_n T_n(H~) psi on the dense matrix, every term formed and added in turn"""
    lo, hi = float(bounds[0]), float(bounds[1])
    a, b = 0.5 * (hi - lo), 0.5 * (hi + lo)
    c, pref = propagator_coefficients(t, bounds, eps, imaginary, reference_energy)
    V = np.asarray(psi)
    prev, cur = None, V.astype(np.result_type(H.dtype, V.dtype, np.float64))
    out = c[0] * cur
    for n in range(1, len(c)):
        if n == 1:
            nxt = (H @ cur) / a - (b / a) * cur
        else:
            nxt = (2.0 / a) * (H @ cur) - (2.0 * b / a) * cur - prev
        out = out + c[n] * nxt
        prev, cur = cur, nxt
    return pref * out


def propagate_tolerance(H, psi, t, bounds, eps=1e-12, imaginary=False, reference_energy=None, eig=None):
    """100 x the largest deviation of series_propagate from exact_propagate on the same matrix and vectors (per column), with a
    floor of 1e-13 |psi|: what a correct implementation with another summation order may deviate by.  -> (tolerance [K], the
    series' own deviation [K])"""
    V = np.asarray(psi).reshape(len(H), -1)
    e_ref = float(bounds[0]) if reference_energy is None else float(reference_energy)
    ex = exact_propagate(H, V, t, imaginary, e_ref, eig)
    own = np.abs(series_propagate(H, V, t, bounds, eps, imaginary, reference_energy) - ex).max(axis=0)
    return np.maximum(100.0 * own, 1e-13 * np.linalg.norm(V, axis=0)), own
