"""Kernel polynomial method (Weisse, Wellein, Alvermann, Fehske, Rev. Mod. Phys. 78, 275): density of states and dynamical
correlation functions S_A(w) = <psi|A^+ delta(w - H) A|psi> from Chebyshev moments mu_n = <v0|T_n(H~)|v0>, at any basis size the
matvec reaches.  H~ = (H - b) / a maps the spectrum into [-1, 1] (a = (hi - lo) / 2, b = (hi + lo) / 2).

The recurrence v_{n+1} = 2 H~ v_n - v_{n-1} is one call of MatvecPlan.matvec_block_axpby per step (ls_amd_matvec_block_axpby: the
update and both dot products of the step happen where the block kernels store their result), and every step yields two moments
(mu_2n = 2 <v_n|v_n> - mu_0, mu_2n+1 = 2 <v_n|v_n+1> - mu_1): M moments cost M / 2 steps and two blocks of memory.  One-partition
plans.  The Jackson-damped series is summed on the host.

Matrix-valued moments mu_n[a][b] = <v_a|T_n(H~)|v_b> of the K columns of a block come from the same recurrence with the two dots
of the step replaced by the two K x K Gram matrices X^+ X and X^+ Y (MatvecPlan.matvec_block_axpby_gram; csrc/k_gram.hip): the
doubling formulas hold for matrices, so K columns of matvecs give all K^2 entries (polarisation needs K^2 columns).  They feed the
spectral matrix S_ab(w) = <psi|A_a^+ delta(w - H) A_b|psi> (spectral_matrix, reconstruct_matrix), the retarded Green's matrix
(greens_matrix) and cross correlators <v_a|e^{-iHt}|v_b> on any time grid (cross_correlation)."""
from __future__ import annotations

import math
import time
from dataclasses import dataclass

import numpy as np

from ._lib import LsAmdError

__all__ = ["KpmResult", "KpmMatrixResult", "jackson_kernel", "reconstruct", "chebyshev_grid", "moments_from_dots", "check_guard",
           "chebyshev_moments", "delta_filter", "filter_order", "chebyshev_series", "spectral_bounds", "random_phase_block",
           "density_of_states", "spectral_function", "block_gram", "moment_matrices_from_grams", "chebyshev_moment_matrices",
           "reconstruct_matrix", "greens_matrix", "cross_correlation", "spectral_matrix"]

GUARD_EVERY = 64      # steps between two read-backs of the dots (the only host synchronisations of the recurrence)
GUARD_SLACK = 1e-6    # ||T_n(H~) v0||^2 <= (1 + slack) ||v0||^2 while the spectrum lies inside the bounds


@dataclass
class KpmResult:
    moments: np.ndarray       # [K, M] float64: mu_n of every start vector
    bounds: tuple             # (lo, hi) the spectrum was rescaled with
    matvec_columns: int       # columns that went through H (K per step)
    kernel: str               # MatvecPlan.axpby_kernel(K): "k_direct_cheb", "k_pull_gather_cheb" or "epilogue"
    seconds: float = 0.0      # wall time of the driver
    step_seconds: float = 0.0  # ... of which inside the Chebyshev steps (device time included: measured around a synchronisation)
    state: object = None      # spectral_function: the state |psi> the operator was applied to (device tensor)
    target_state: object = None  # spectral_function(target=...): v0 = A|psi> on the target basis (device tensor)

    @property
    def trace_moments(self):
        """the moments of the normalised trace, sum_k mu_n^(k) / sum_k mu_0^(k): [M]"""
        return self.moments.sum(axis=0) / self.moments[:, 0].sum()


def jackson_kernel(num_moments: int) -> np.ndarray:
    """g_n of the Jackson kernel for M moments (RMP 78, 275, eq. 71): g_0 = 1, positive, decreasing"""
    M = int(num_moments)
    n = np.arange(M, dtype=np.float64)
    q = math.pi / (M + 1)
    return ((M - n + 1) * np.cos(q * n) + np.sin(q * n) / math.tan(q)) / (M + 1)


def reconstruct(moments, bounds, energies) -> np.ndarray:
    """f(E) = 1 / (pi a sqrt(1 - x^2)) [g_0 mu_0 + 2 sum_n g_n mu_n T_n(x)],  x = (E - b) / a, zero outside the bounds:
    the Jackson-damped Chebyshev series of the moments [M] (or [..., M]: one curve per leading index) at the energies [E]."""
    mu = np.asarray(moments, dtype=np.float64)
    lo, hi = float(bounds[0]), float(bounds[1])
    a, b = 0.5 * (hi - lo), 0.5 * (hi + lo)
    M = mu.shape[-1]
    c = mu * jackson_kernel(M)
    c[..., 1:] *= 2.0
    x = (np.asarray(energies, dtype=np.float64) - b) / a
    inside = np.abs(x) < 1.0
    theta = np.arccos(np.where(inside, x, 0.0))
    out = np.zeros(mu.shape[:-1] + x.shape, dtype=np.float64)
    n = np.arange(M, dtype=np.float64)
    for e0 in range(0, x.size, 4096):  # (the cosine table in slabs: [4096, M])
        e1 = min(x.size, e0 + 4096)
        T = np.cos(theta.reshape(-1)[e0:e1, None] * n[None, :])
        out.reshape(mu.shape[:-1] + (-1,))[..., e0:e1] = (c @ T.T) / (math.pi * a * np.sin(theta.reshape(-1)[e0:e1]))
    return np.where(inside, out, 0.0)


def chebyshev_grid(bounds, points: int) -> np.ndarray:
    """E_k = b + a cos(pi (k + 1/2) / points), ascending: the abscissas the series is cheapest and best conditioned on"""
    lo, hi = float(bounds[0]), float(bounds[1])
    k = np.arange(points, dtype=np.float64)
    return 0.5 * (hi + lo) + 0.5 * (hi - lo) * np.cos(math.pi * (k + 0.5) / points)[::-1]


def moments_from_dots(dots, K: int, num_moments: int) -> np.ndarray:
    """dots [steps, 2K] (row n: <v_n|v_n> per column, then <v_n|v_n+1>) -> moments [K, M] by the doubling formulas"""
    d = np.asarray(dots, dtype=np.float64)
    steps = d.shape[0]
    mu = np.empty((K, 2 * steps), dtype=np.float64)
    mu[:, 0] = d[0, :K]
    mu[:, 1] = d[0, K:]
    for n in range(1, steps):
        mu[:, 2 * n] = 2.0 * d[n, :K] - mu[:, 0]
        mu[:, 2 * n + 1] = 2.0 * d[n, K:] - mu[:, 1]
    return mu[:, :num_moments]


def check_guard(dots, K: int, bounds, first_step: int = 0):
    """||T_n(H~) v0|| <= ||v0|| holds whenever the spectrum lies inside the bounds: raise when some <v_n|v_n> of dots [steps, 2K]
    (or a non-finite one) says it does not.  dots[0] must be the first step's row (mu_0) -- first_step only names the offset."""
    d = np.asarray(dots, dtype=np.float64)
    mu0 = d[0, :K]
    norms = d[:, :K]
    bad = ~(norms <= (1.0 + GUARD_SLACK) * mu0[None, :])
    if bad.any():
        step = int(np.argmax(bad.any(axis=1)))
        raise LsAmdError(f"kpm: the Chebyshev recurrence grows at step {first_step + step} (<v_n|v_n> / <v_0|v_0> = "
                         f"{float(np.nanmax(norms[step] / mu0)):.6g}): the spectrum is not inside the bounds ({bounds[0]!r}, {bounds[1]!r})")


def chebyshev_moments(op, start, num_moments: int, bounds) -> np.ndarray:
    """mu_n = <v0_k|T_n(H~)|v0_k> for the K columns of the (n, K) device block `start`, n < num_moments: [K, M] float64.
    op: a diagonalize.LocalOperator on one partition.  The dots of all steps land in one device array; it is read back (the
    only synchronisation) every GUARD_EVERY steps for the guard."""
    import torch

    M = int(num_moments)
    if M < 2:
        raise ValueError(f"num_moments = {num_moments!r}: at least 2")
    lo, hi = float(bounds[0]), float(bounds[1])
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"bounds = ({bounds[0]!r}, {bounds[1]!r}): need finite lo < hi")
    if len(op.sizes) != 1:
        raise LsAmdError("kpm: one-partition plans only")
    if start.dim() != 2 or start.shape[0] != op.n_local:
        raise LsAmdError(f"kpm: start {tuple(start.shape)} must be an ({op.n_local}, K) block")
    a, b = 0.5 * (hi - lo), 0.5 * (hi + lo)
    K = int(start.shape[1])
    steps = (M + 1) // 2
    X = start.to(op.dtype).contiguous().clone()
    Y = torch.empty_like(X)
    dots = torch.zeros((steps, 2 * K), dtype=torch.float64, device=X.device)
    plan = op.plan
    checked = 0
    host = np.empty((steps, 2 * K), dtype=np.float64)

    def read_back(upto):
        nonlocal checked
        host[checked:upto] = dots[checked:upto].cpu().numpy()
        plan.check()
        check_guard(np.concatenate([host[:1], host[checked:upto]]), K, (lo, hi), first_step=checked - 1)
        checked = upto

    for s in range(steps):
        if s == 0:
            plan.matvec_block_axpby(X, Y, 1.0 / a, -b / a, 0.0, dots=dots[0], check=False)
        else:
            plan.matvec_block_axpby(X, Y, 2.0 / a, -2.0 * b / a, -1.0, dots=dots[s], check=False)
        X, Y = Y, X
        op.matvecs += K
        if (s + 1) % GUARD_EVERY == 0:
            read_back(s + 1)
    if checked < steps:
        read_back(steps)
    return moments_from_dots(host, K, M)


# ---------------------------------------------------------------------------------------------
# matrix-valued moments
# ---------------------------------------------------------------------------------------------
@dataclass
class KpmMatrixResult:
    moments: np.ndarray       # [M, K, K] complex128: mu_n[a][b] = <v_a|T_n(H~)|v_b>, v_a = A_a|psi>
    bounds: tuple             # (lo, hi) the spectrum was rescaled with
    matvecs: int              # columns that went through H (K per step, M / 2 steps)
    kernel: str               # MatvecPlan.axpby_kernel(K)
    gram_kernel: str          # MatvecPlan.gram_kernel(K): "k_block_gram_mfma" or "k_block_gram"
    state: object = None      # the state |psi> the operators were applied to (device tensor)
    target_states: object = None  # the (n, K) block of the v_a on the basis the moments were computed on (device tensor)
    seconds: float = 0.0
    step_seconds: float = 0.0


def _gram_into(a, b, out, work):
    import ctypes as C

    import torch

    from . import _lib
    from .api import _stream_ptr

    _lib.check(_lib.load().ls_amd_block_gram(int(a.dtype == torch.complex128), int(a.shape[0]), int(a.shape[1]), C.c_void_p(a.data_ptr()),
                                             a.stride(0), a.stride(1), int(b.shape[1]), C.c_void_p(b.data_ptr()), b.stride(0), b.stride(1),
                                             C.c_void_p(work.data_ptr()), work.numel() * 8, C.c_void_p(out.data_ptr()), _stream_ptr()))


def _gram_work(n, Ka, Kb, dtype, device):
    import torch

    from . import _lib

    need = int(_lib.load().ls_amd_block_gram_work_bytes(int(n), int(Ka), int(Kb), int(dtype == torch.complex128)))
    if need < 0:
        _lib.check(-1)
    return torch.empty(max(1, need // 8), dtype=torch.float64, device=device)


def block_gram(a, b):
    """G = A^+ B, G[i][j] = sum_r conj(A[r, i]) B[r, j], of the (n, Ka) and (n, Kb) device tensors a and b (both float64 or both
    complex128, any strides, Ka, Kb <= 64) as a new (Ka, Kb) device tensor (ls_amd_block_gram).  Interleaved blocks (contiguous
    (n, K) tensors) of at least 8 columns run on the f64 MFMA, narrower ones and other strides on the vector ALU;
    LS_AMD_GRAM=mfma|valu overrides that.  Sums in a fixed order: two calls return equal bytes.  Allocates its own scratch."""
    import torch

    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise LsAmdError(f"block_gram: {name} must be a 2-D (n, K) tensor")
        if t.device.type != "cuda":
            raise LsAmdError(f"block_gram: {name} must be a device tensor")
        if t.dtype not in (torch.float64, torch.complex128) or t.dtype != a.dtype:
            raise LsAmdError(f"block_gram: {name} is {t.dtype}; a and b must both be float64 or both complex128")
        if not 1 <= int(t.shape[1]) <= 64:
            raise LsAmdError(f"block_gram: {name} has K = {int(t.shape[1])} columns: 1 <= K <= 64")
    if a.shape[0] != b.shape[0]:
        raise LsAmdError(f"block_gram: a {tuple(a.shape)} and b {tuple(b.shape)} must have the same number of rows")
    out = torch.empty((int(a.shape[1]), int(b.shape[1])), dtype=a.dtype, device=a.device)
    _gram_into(a, b, out, _gram_work(a.shape[0], a.shape[1], b.shape[1], a.dtype, a.device))
    return out


def moment_matrices_from_grams(grams, num_moments: int) -> np.ndarray:
    """grams [steps, 2, K, K] (row n: V_n^+ V_n, then V_n^+ V_n+1, V_n = T_n(H~) V_0) -> moments [M, K, K] complex128 by the doubling
    formulas mu_2n = 2 V_n^+ V_n - mu_0, mu_2n+1 = 2 V_n^+ V_n+1 - mu_1, each symmetrised as (mu + mu^+) / 2 (T_n(H~) is Hermitian;
    the two Gram matrices are so up to rounding)"""
    g = np.asarray(grams).astype(np.complex128)
    steps, K = g.shape[0], g.shape[-1]
    mu = np.empty((2 * steps, K, K), dtype=np.complex128)
    mu[0], mu[1] = g[0, 0], g[0, 1]
    for n in range(1, steps):
        mu[2 * n] = 2.0 * g[n, 0] - mu[0]
        mu[2 * n + 1] = 2.0 * g[n, 1] - mu[1]
    mu = mu[:int(num_moments)]
    return 0.5 * (mu + mu.conj().transpose(0, 2, 1))


def chebyshev_moment_matrices(op, start, num_moments: int, bounds, bra=None) -> np.ndarray:
    """mu_n[a][b] = <v_a|T_n(H~)|v_b> for the K columns of the (n, K) device block `start`, n < num_moments: [M, K, K] complex128
    (Hermitian; real up to rounding on a float64 operator).  op: a diagonalize.LocalOperator on one partition.  One
    MatvecPlan.matvec_block_axpby_gram per step, two moments per step; the Gram matrices of all steps land in one device array,
    read back (the only synchronisation) every GUARD_EVERY steps for the growth guard on the diagonal of X^+ X.
    bra: an (n, Ka) device block Phi -> [M, Ka, K], mu_n = Phi^+ T_n(H~) V_0 -- one order per step (the doubling needs bra = ket):
    matvec_block_axpby and one block_gram, e.g. for <phi_a|e^{-iHt}|psi_b> through cross_correlation."""
    import torch

    M = int(num_moments)
    if M < 2:
        raise ValueError(f"num_moments = {num_moments!r}: at least 2")
    lo, hi = _bounds(bounds, "chebyshev_moment_matrices")
    if len(op.sizes) != 1:
        raise LsAmdError("kpm: one-partition plans only")
    if start.dim() != 2 or start.shape[0] != op.n_local:
        raise LsAmdError(f"kpm: start {tuple(start.shape)} must be an ({op.n_local}, K) block")
    a, b = 0.5 * (hi - lo), 0.5 * (hi + lo)
    K = int(start.shape[1])
    if not 1 <= K <= 64:
        raise LsAmdError(f"kpm: K = {K} columns: 1 <= K <= 64")
    X = start.to(op.dtype).contiguous().clone()
    Y = torch.empty_like(X)
    plan = op.plan
    checked = 0
    if bra is not None:
        if bra.dim() != 2 or bra.shape[0] != op.n_local or not 1 <= int(bra.shape[1]) <= 64:
            raise LsAmdError(f"kpm: bra {tuple(bra.shape)} must be an ({op.n_local}, Ka) block, 1 <= Ka <= 64")
        phi = bra.to(op.dtype).contiguous()
        Ka = int(phi.shape[1])
        steps = M - 1
        out = torch.zeros((M, Ka, K), dtype=op.dtype, device=X.device)
        work = _gram_work(op.n_local, Ka, K, op.dtype, X.device)
        dots = torch.zeros((steps, 2 * K), dtype=torch.float64, device=X.device)
        host = np.empty((steps, 2 * K), dtype=np.float64)

        def read_back(upto):
            nonlocal checked
            host[checked:upto] = dots[checked:upto].cpu().numpy()
            plan.check()
            check_guard(np.concatenate([host[:1], host[checked:upto]]), K, (lo, hi), first_step=checked - 1)
            checked = upto

        _gram_into(phi, X, out[0], work)
        for s in range(steps):
            if s == 0:
                plan.matvec_block_axpby(X, Y, 1.0 / a, -b / a, 0.0, dots=dots[0], check=False)
            else:
                plan.matvec_block_axpby(X, Y, 2.0 / a, -2.0 * b / a, -1.0, dots=dots[s], check=False)
            X, Y = Y, X
            _gram_into(phi, X, out[s + 1], work)
            op.matvecs += K
            if (s + 1) % GUARD_EVERY == 0:
                read_back(s + 1)
        if checked < steps:
            read_back(steps)
        return out.cpu().numpy().astype(np.complex128)

    steps = (M + 1) // 2
    grams = torch.zeros((steps, 2, K, K), dtype=op.dtype, device=X.device)
    host = np.empty((steps, 2, K, K), dtype=np.complex128)

    def read_back(upto):  # noqa: F811
        nonlocal checked
        host[checked:upto] = grams[checked:upto].cpu().numpy()
        plan.check()
        norms = np.zeros((upto - checked + 1, 2 * K), dtype=np.float64)
        norms[0, :K] = np.diagonal(host[0, 0]).real
        norms[1:, :K] = np.diagonal(host[checked:upto, 0], axis1=1, axis2=2).real
        check_guard(norms, K, (lo, hi), first_step=checked - 1)
        checked = upto

    for s in range(steps):
        if s == 0:
            plan.matvec_block_axpby_gram(X, Y, 1.0 / a, -b / a, 0.0, grams[0], check=False)
        else:
            plan.matvec_block_axpby_gram(X, Y, 2.0 / a, -2.0 * b / a, -1.0, grams[s], check=False)
        X, Y = Y, X
        op.matvecs += K
        if (s + 1) % GUARD_EVERY == 0:
            read_back(s + 1)
    if checked < steps:
        read_back(steps)
    return moment_matrices_from_grams(host, M)


def _matrix_series(moments, bounds, energies, who):
    """(x inside the bounds, theta, the damped coefficients (2 - delta_n0) g_n mu_n [M, ...], a) shared by the two reconstructions"""
    mu = np.asarray(moments, dtype=np.complex128)
    if mu.ndim != 3:
        raise ValueError(f"{who}: moments {mu.shape} must be [M, Ka, Kb]")
    lo, hi = _bounds(bounds, who)
    a, b = 0.5 * (hi - lo), 0.5 * (hi + lo)
    c = mu * jackson_kernel(mu.shape[0])[:, None, None]
    c[1:] *= 2.0
    x = (np.asarray(energies, dtype=np.float64).reshape(-1) - b) / a
    inside = np.abs(x) < 1.0
    return inside, np.arccos(np.where(inside, x, 0.0)), c, a


def reconstruct_matrix(moments, bounds, energies) -> np.ndarray:
    """S_ab(E) = 1 / (pi a sqrt(1 - x^2)) [g_0 mu_0 + 2 sum_n g_n mu_n T_n(x)]_ab, x = (E - b) / a, zero outside the bounds: the
    Jackson-damped series of `reconstruct`, entry by entry, of the moments [M, Ka, Kb] at the energies [E] -> complex128
    [E, Ka, Kb].  For Hermitian moments of one block (Ka = Kb) every S(E) is Hermitian and -- the kernel being positive --
    positive semi-definite."""
    inside, theta, c, a = _matrix_series(moments, bounds, energies, "reconstruct_matrix")
    out = np.zeros((theta.size,) + c.shape[1:], dtype=np.complex128)
    n = np.arange(c.shape[0], dtype=np.float64)
    for e0 in range(0, theta.size, 4096):
        e1 = min(theta.size, e0 + 4096)
        T = np.cos(theta[e0:e1, None] * n[None, :])
        out[e0:e1] = np.tensordot(T, c, axes=(1, 0)) / (math.pi * a * np.sin(theta[e0:e1]))[:, None, None]
    out[~inside] = 0.0
    return out


def greens_matrix(moments, bounds, energies) -> np.ndarray:
    """the retarded G_ab(E + i0) = <v_a|(E + i0 - H)^-1|v_b> from the same damped series,
        G(E) = -i / (a sqrt(1 - x^2)) [g_0 mu_0 + 2 sum_n g_n mu_n e^{-i n arccos x}],
    complex128 [E, Ka, Kb], zero outside the bounds.  Its spectral part is the reconstruction: with Hermitian moments
    -(G - G^+) / (2 pi i) = reconstruct_matrix(moments, bounds, energies), and entry by entry -Im G_aa / pi = S_aa on the diagonal."""
    inside, theta, c, a = _matrix_series(moments, bounds, energies, "greens_matrix")
    out = np.zeros((theta.size,) + c.shape[1:], dtype=np.complex128)
    n = np.arange(c.shape[0], dtype=np.float64)
    for e0 in range(0, theta.size, 4096):
        e1 = min(theta.size, e0 + 4096)
        ph = np.exp(-1j * theta[e0:e1, None] * n[None, :])
        out[e0:e1] = -1j * np.tensordot(ph, c, axes=(1, 0)) / (a * np.sin(theta[e0:e1]))[:, None, None]
    out[~inside] = 0.0
    return out


def cross_correlation(moments, bounds, times, eps: float = 1e-12) -> np.ndarray:
    """C_ab(t) = <v_a|e^{-iHt}|v_b> = e^{-ibt} sum_n (2 - delta_n0) (-i)^n J_n(a t) mu_n[a][b] from the undamped moment matrices
    [M, Ka, Kb] of chebyshev_moment_matrices for the same bounds, at the times [T] -> complex128 [T, Ka, Kb].  Host only; the
    time grid is free (every time is one sum over the same moments).  ValueError when there are fewer moments than the order the
    series needs for `eps` at some time, as in evolve.autocorrelation."""
    from .evolve import propagator_coefficients

    mu = np.asarray(moments, dtype=np.complex128)
    if mu.ndim != 3:
        raise ValueError(f"cross_correlation: moments {mu.shape} must be [M, Ka, Kb]")
    lo, hi = _bounds(bounds, "cross_correlation")
    ts = np.atleast_1d(np.asarray(times, dtype=np.float64))
    M = mu.shape[0]
    out = np.empty((len(ts),) + mu.shape[1:], dtype=np.complex128)
    for j, t in enumerate(ts):
        c, pref = propagator_coefficients(float(t), (lo, hi), eps)
        if len(c) > M:
            raise ValueError(f"cross_correlation: t = {float(t)!r} needs {len(c)} moments for eps = {eps!r}, {M} were given")
        out[j] = pref * np.tensordot(c, mu[:len(c)], axes=(0, 0))
    return out


FILTER_CUT = 0.17    # filter_order: the levels wanted see p(E) >= cut p(sigma) (POLFED, PRL 125, 156601)


def _bounds(bounds, who):
    try:
        lo, hi = float(bounds[0]), float(bounds[1])
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"{who}: bounds = {bounds!r}: need finite lo < hi") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"{who}: bounds = ({bounds[0]!r}, {bounds[1]!r}): need finite lo < hi")
    return lo, hi


def _scaled_sigma(sigma, lo, hi, who):
    try:
        sigma = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: sigma = {sigma!r} is not a number") from None
    if not (math.isfinite(sigma) and lo < sigma < hi):
        raise ValueError(f"{who}: sigma = {sigma!r} is not inside the bounds ({lo!r}, {hi!r}); the levels at the edges of the spectrum: "
                         "diagonalize()")
    return (sigma - 0.5 * (hi + lo)) / (0.5 * (hi - lo))


def delta_filter(sigma: float, bounds, order: int) -> np.ndarray:
    """c[0..order] of the Jackson-damped Chebyshev expansion of delta(x - s), x = (E - b) / a, s the scaled sigma:

        p(x) = sum_n c_n T_n(x),    c_n = (2 - delta_n0) g_n cos(n arccos s) / (pi sqrt(1 - s^2)),

    g_n = jackson_kernel(order + 1), the damping of `reconstruct`.  p is positive, peaks at s (to O(1 / order^2)), is close to a
    Gaussian of width pi sqrt(1 - s^2) / order there, and its integral against the Chebyshev weight,
    int p(x) sqrt(1 - s^2) / sqrt(1 - x^2) dx = g_0, is exactly 1.  A sigma outside the bounds is refused."""
    lo, hi = _bounds(bounds, "delta_filter")
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or order < 0:
        raise ValueError(f"delta_filter: order = {order!r}: a non-negative integer")
    s = _scaled_sigma(sigma, lo, hi, "delta_filter")
    n = np.arange(int(order) + 1, dtype=np.float64)
    c = 2.0 * jackson_kernel(int(order) + 1) * np.cos(n * math.acos(s)) / (math.pi * math.sqrt(1.0 - s * s))
    c[0] *= 0.5
    return c


def _dos_at(op, sigma, bounds, num_moments=64, num_vectors=4, seed=0):
    """rho(sigma), normalised to one level, from a few moments of a few random vectors (fixed seed)"""
    start = random_phase_block(op.n_local, min(int(num_vectors), 64), op.dtype, seed, device=op.device)
    mu = chebyshev_moments(op, start, num_moments, bounds)
    return float(reconstruct(mu.sum(axis=0) / mu[:, 0].sum(), bounds, np.array([float(sigma)]))[0])


def filter_order(num_states: int, dimension: int, dos_at_sigma=None, bounds=None, cut: float = FILTER_CUT, sigma=None, op=None) -> int:
    """the order of delta_filter at which about `num_states` levels see p(E) >= cut p(sigma): the narrowest filter (the largest
    order) that keeps the window of those levels above the cut.  The `num_states` levels nearest sigma fill the window
    |E - sigma| <= num_states / (2 dimension dos_at_sigma) (dos_at_sigma: the density of states at sigma, normalised to ONE level,
    per unit of energy); near its peak p is a Gaussian of width pi sqrt(1 - s^2) / order in x = (E - b) / a, so p >= cut p(sigma)
    out to sqrt(2 ln(1 / cut)) widths: that estimate is the start, refined on the kernel's own values at the edges of the window
    (an edge beyond the bounds does not count).  sigma None: the middle of the bounds.
    dos_at_sigma None: from 64 moments of 4 random vectors of seed 0 on `op` (a diagonalize.LocalOperator).  At least 2."""
    lo, hi = _bounds(bounds, "filter_order")
    if isinstance(num_states, bool) or not isinstance(num_states, (int, np.integer)) or num_states < 1:
        raise ValueError(f"filter_order: num_states = {num_states!r}: a positive integer")
    if isinstance(dimension, bool) or not isinstance(dimension, (int, np.integer)) or dimension < 1:
        raise ValueError(f"filter_order: dimension = {dimension!r}: a positive integer")
    if not 0.0 < float(cut) < 1.0:
        raise ValueError(f"filter_order: cut = {cut!r}: 0 < cut < 1")
    s = 0.0 if sigma is None else _scaled_sigma(sigma, lo, hi, "filter_order")
    if dos_at_sigma is None:
        if op is None:
            raise ValueError("filter_order: dos_at_sigma or op is needed")
        dos_at_sigma = _dos_at(op, 0.5 * (lo + hi) if sigma is None else float(sigma), (lo, hi))
    dos = float(dos_at_sigma)
    if not (math.isfinite(dos) and dos > 0.0):
        raise ValueError(f"filter_order: dos_at_sigma = {dos_at_sigma!r}: a positive number")
    half_window = min(num_states / (2.0 * dimension * dos) / (0.5 * (hi - lo)), 2.0)  # in x; the whole band is 2 wide
    guess = max(2, int(math.ceil(math.pi * math.sqrt(1.0 - s * s) * math.sqrt(2.0 * math.log(1.0 / float(cut))) / half_window)))
    edges = np.array([x for x in (s - half_window, s + half_window) if -1.0 < x < 1.0])
    if edges.size == 0:
        return guess
    # the Jackson kernel is a Gaussian only roughly (its ratio at the Gaussian's cut is some 10 % off): the estimate is refined on
    # the kernel itself, by bisection -- the largest order at which both edges of the window still see the cut
    theta, theta_s = np.arccos(edges), math.acos(s)

    def keeps(order):
        n = np.arange(order + 1, dtype=np.float64)
        g = jackson_kernel(order + 1) * np.cos(n * theta_s)
        g[1:] *= 2.0
        peak = float(g @ np.cos(n * theta_s))
        return bool(np.all(np.cos(theta[:, None] * n[None, :]) @ g >= float(cut) * peak))

    if not keeps(2):
        return 2
    good, bad = 2, guess
    while keeps(bad):
        good, bad = bad, 2 * bad
    while bad - good > 1:
        mid = (good + bad) // 2
        if keeps(mid):
            good = mid
        else:
            bad = mid
    return good


def chebyshev_series(op, state, coefficients, bounds=None):
    """sum_n c_n T_n((H - b) / a) state as a new device tensor: a vector, or an (n, K) block of K <= 64 states with any strides
    (copied to the interleaved layout).  op: a diagonalize.LocalOperator on one partition over a Hermitian operator; bounds: (lo, hi)
    enclosing its spectrum (spectral_bounds(op) when None).  Real coefficients keep the sum in op.dtype, complex ones make it
    complex128.  One MatvecPlan.matvec_block_series: loop and growth guard run in C, one synchronisation per GUARD_EVERY orders;
    bounds that do not enclose the spectrum raise LsAmdError."""
    import torch

    K = 1 if state.dim() == 1 else (int(state.shape[1]) if state.dim() == 2 else -1)
    if K < 0:
        raise LsAmdError(f"chebyshev_series: state {tuple(state.shape)} must be a vector or an (n, K) block")
    if K > 64 or K < 1:
        raise LsAmdError(f"chebyshev_series: K = {K} columns: 1 <= K <= 64")
    if not op.plan.matrix.isHermitian:
        raise ValueError("chebyshev_series: the operator is not Hermitian (a Chebyshev series needs a real spectrum)")
    if len(op.sizes) != 1:
        raise LsAmdError("chebyshev_series: one-partition plans only")
    if state.is_complex() and op.dtype != torch.complex128:
        raise LsAmdError("chebyshev_series: the state is complex and the operator computes in float64: build the operator with "
                         "dtype=torch.complex128")
    if state.shape[0] != op.n_local:
        raise LsAmdError(f"chebyshev_series: state {tuple(state.shape)} must have {op.n_local} rows")
    c = np.asarray(coefficients).reshape(-1)
    if c.size < 1:
        raise ValueError("chebyshev_series: no coefficients")
    real = not np.iscomplexobj(c) or not np.any(c.imag != 0.0)
    c = c.real.astype(np.float64) if real else c.astype(np.complex128)
    bounds = _bounds(bounds if bounds is not None else spectral_bounds(op), "chebyshev_series")
    X = state.reshape(op.n_local, K).to(op.dtype).contiguous()
    Z = torch.empty((op.n_local, K), dtype=op.dtype if real else torch.complex128, device=X.device)
    op.plan.matvec_block_series(X, Z, c, bounds)
    op.matvecs += K * (len(c) - 1)
    return Z.reshape(-1) if state.dim() == 1 else Z


class _Negated:
    """-H through the operator interface of lanczos_smallest"""

    def __init__(self, op):
        self.op = op

    def __getattr__(self, name):
        return getattr(self.op, name)

    def matvec(self, x, y):
        self.op.matvec(x, y)
        y.neg_()

    @property
    def matvecs(self):
        return self.op.matvecs


def spectral_bounds(op, eps: float = 1e-3, widen: float = 0.01):
    """(lo, hi) enclosing the spectrum of the Hermitian operator: the extremal Ritz values of two loose Lanczos runs (on H and on
    -H), widened by `widen` of the width on each side -- Ritz values lie INSIDE the spectrum."""
    from .diagonalize import lanczos_smallest

    e_min = lanczos_smallest(op, num_evals=1, eps=eps).eigenvalues[0]
    e_max = -lanczos_smallest(_Negated(op), num_evals=1, eps=eps).eigenvalues[0]
    width = max(e_max - e_min, 1e-9 * max(1.0, abs(e_min), abs(e_max)))
    return e_min - widen * width, e_max + widen * width


def random_phase_block(n: int, K: int, dtype, seed: int, device="cuda"):
    """(n, K) start vectors for a stochastic trace, generated on the device: random signs (f64) or random phases (c128)"""
    import torch

    g = torch.Generator(device=device).manual_seed(int(seed))
    if dtype == torch.complex128:
        phi = torch.rand((n, K), dtype=torch.float64, device=device, generator=g) * (2.0 * math.pi)
        return torch.polar(torch.ones_like(phi), phi)
    return (torch.randint(0, 2, (n, K), device=device, generator=g, dtype=torch.int64) * 2 - 1).to(torch.float64)


def _load(config, observables=False):
    from . import api

    load = api.loadConfigFromYaml if isinstance(config, str) else api.loadConfigFromDict
    out = load(config, hamiltonian=True, observables=observables)
    h = out[1]
    if not h.isHermitian:
        raise ValueError("kpm: the Hamiltonian is not Hermitian (Chebyshev moments need a real spectrum)")
    return out


def density_of_states(config, num_moments: int = 256, num_vectors: int = 8, seed: int = 0, bounds=None, dtype=None, energies=None,
                      start=None):
    """rho(E) = (1 / n) sum_j delta(E - E_j) of the configured Hamiltonian (dict or YAML path) by a stochastic trace over
    `num_vectors` random-sign (c128: random-phase) vectors, or over the columns of the (n, K) device block `start`.
    -> (energies, rho, KpmResult); energies default to a Chebyshev grid of 2 M points inside the bounds (spectral_bounds(op) unless
    given)."""
    import torch

    from . import api
    from .diagonalize import LocalOperator

    t0 = time.perf_counter()
    basis, h = _load(config)
    dtype = dtype or torch.float64
    reps, _ = api.enumerateStates(basis, 1)
    op = LocalOperator(h, reps, dtype)
    if bounds is None:
        bounds = spectral_bounds(op)
    bounds = (float(bounds[0]), float(bounds[1]))
    if start is None:
        if not 1 <= int(num_vectors) <= 64:
            raise ValueError(f"num_vectors = {num_vectors!r}: 1 <= num_vectors <= 64")
        start = random_phase_block(op.n_local, int(num_vectors), dtype, seed, device=op.device)
    K = int(start.shape[1])
    before = op.matvecs
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    mu = chebyshev_moments(op, start, num_moments, bounds)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res = KpmResult(mu, bounds, op.matvecs - before, op.plan.axpby_kernel(K))
    if energies is None:
        energies = chebyshev_grid(bounds, 2 * int(num_moments))
    energies = np.asarray(energies, dtype=np.float64)
    rho = reconstruct(res.trace_moments, bounds, energies)
    res.step_seconds = t2 - t1
    res.seconds = time.perf_counter() - t0
    return energies, rho, res


def _terms_of(op):
    """the (v, m, r, x, s) terms of an api.Operator, read through the ls_hs_nonbranching_terms ABI"""
    import ctypes as C

    out = []
    for nbt in (op.payload.contents.diag_terms, op.payload.contents.off_diag_terms):
        if not nbt:
            continue
        t = nbt.contents
        n = int(t.number_terms)
        v = np.frombuffer((C.c_double * (2 * n)).from_address(t.v), dtype=np.float64).reshape(n, 2)
        m, r, x, s = (np.frombuffer((C.c_uint64 * n).from_address(q), dtype=np.uint64) for q in (t.m, t.r, t.x, t.s))
        out += [(complex(v[i, 0], v[i, 1]), int(m[i]), int(r[i]), int(x[i]), int(s[i])) for i in range(n)]
    return out


def _target_basis(target):
    """target of spectral_function: a `basis:` section, a whole config (dict), or the path of a YAML config -> api.Basis"""
    from . import api

    if isinstance(target, api.Basis):
        return target
    if isinstance(target, str):
        return api.loadConfigFromYaml(target)
    if isinstance(target, dict):
        return api.loadConfigFromDict(target if "basis" in target else {"basis": target})
    raise ValueError("target: a `basis:` section (dict), a whole config (dict or YAML path) or an api.Basis")


def _spectral_function_cross(config, operator, target, state, num_moments, energies, bounds, dtype, eps, groups="same"):
    """spectral_function for an operator that maps the config's sector into another one: psi lives in the config's own (source)
    sector, v0 = A psi goes through an api.CrossSectorPlan, and the config's Hamiltonian -- re-compiled on the target basis from
    its term tables -- supplies bounds and moments there."""
    import torch

    from . import api, config as _config
    from .diagonalize import LocalOperator, lanczos_smallest

    t0 = time.perf_counter()
    basis, h, obs = _load(config, observables=True)
    if isinstance(operator, (int, np.integer)) and not isinstance(operator, bool):
        if not 0 <= int(operator) < len(obs):
            raise ValueError(f"operator = {operator}: the config has {len(obs)} observables")
        A = obs[int(operator)]
    elif isinstance(operator, api.Operator):
        A = operator
    else:
        raise ValueError("operator: an api.Operator (on the source basis) or the index of one of the config's observables")
    dtype = dtype or torch.float64
    tbasis = _target_basis(target)
    if groups not in api.CrossSectorPlan.GROUPS:
        raise ValueError(f"groups = {groups!r} is none of 'same', 'restrict', 'project'")
    if groups != "project":  # (a projecting plan asks nothing of the operator)
        A.mapsSector(tbasis, explain=True, signs=True, subgroup=groups == "restrict")
    h_t = api.Operator.fromSpec(tbasis, _config.OperatorSpec(_terms_of(h)))
    if not h_t.isHermitian:
        raise ValueError("kpm: the Hamiltonian is not Hermitian (Chebyshev moments need a real spectrum)")
    reps, _ = api.enumerateStates(basis, 1)
    treps, _ = api.enumerateStates(tbasis, 1)
    if state is None:
        state = lanczos_smallest(LocalOperator(h, reps, dtype), num_evals=1, eps=eps).eigenvectors[0]
    state = state.to(dtype).contiguous()
    if state.dim() != 1 or state.numel() != reps[0].numel():
        raise LsAmdError(f"kpm: state {tuple(state.shape)} must be a vector of {reps[0].numel()} elements (the source basis)")
    op = LocalOperator(h_t, treps, dtype)
    if bounds is None:
        bounds = spectral_bounds(op)
    bounds = (float(bounds[0]), float(bounds[1]))
    v0 = torch.zeros(op.n_local, dtype=dtype, device=state.device)
    cross = api.CrossSectorPlan(A, reps[0], tbasis, treps[0], dtype, groups=groups)
    cross.apply(state, v0)
    cross.destroy()
    before = op.matvecs
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    mu = chebyshev_moments(op, v0.reshape(-1, 1), num_moments, bounds)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res = KpmResult(mu, bounds, op.matvecs - before, op.plan.axpby_kernel(1), state=state, target_state=v0)
    if energies is None:
        energies = chebyshev_grid(bounds, 2 * int(num_moments))
    energies = np.asarray(energies, dtype=np.float64)
    S = reconstruct(mu[0], bounds, energies)
    res.step_seconds = t2 - t1
    res.seconds = time.perf_counter() - t0
    return energies, S, res


def spectral_function(config, operator, state=None, num_moments: int = 256, energies=None, bounds=None, dtype=None,
                      eps: float = 1e-10, target=None, groups: str = "same"):
    """S_A(w) = <psi|A^+ delta(w - H) A|psi> on the absolute energy scale of H.  operator: an api.Operator on the basis of the
    config, or the index of one of the config's `observables`; it must map the basis into itself.  state: a device vector in the
    order of the representatives; None: the ground state (thick-restart Lanczos to `eps`).  -> (energies, S, KpmResult).

    target: the sector A maps INTO when that is not the config's own -- a `basis:` section (dict), a whole config whose basis it is
    (dict or YAML path), or an api.Basis -- e.g. momentum k + q for S^z_q on a ground state of momentum k.  The operator is then
    compiled on (and psi lives in) the config's own basis, the source; v0 = A psi is an api.CrossSectorPlan, and the config's
    `hamiltonian:` is re-compiled on the target basis, where the bounds and the moments are computed; KpmResult.target_state is
    v0.  Sectors with complex characters need dtype=torch.complex128.  Projected fermionic bases are sectors like any other here:
    c+_k / c_k from an N-particle ground state of momentum k0 into the N +- 1 sector of momentum k0 +- k is the photoemission
    spectrum A(k, w), n_q and S^z_q give N(q, w) and S^z(q, w).
    groups: passed to api.CrossSectorPlan -- "same" (the two bases have the same generators), "restrict" (the target group is a
    subgroup of the config's: the ground state of the sector with every symmetry, S^z_q into translations only) or "project" (any
    operator, e.g. the local sigma^z_0: v0 is the component of A psi in the target sector)."""
    import torch

    if target is not None:
        return _spectral_function_cross(config, operator, target, state, num_moments, energies, bounds, dtype, eps, groups)

    from . import api
    from .diagonalize import LocalOperator, lanczos_smallest

    t0 = time.perf_counter()
    basis, h, obs = _load(config, observables=True)
    if isinstance(operator, (int, np.integer)) and not isinstance(operator, bool):
        if not 0 <= int(operator) < len(obs):
            raise ValueError(f"operator = {operator}: the config has {len(obs)} observables")
        A = obs[int(operator)]
    elif isinstance(operator, api.Operator):
        A = operator
    else:
        raise ValueError("operator: an api.Operator or the index of one of the config's observables")
    dtype = dtype or torch.float64
    reps, _ = api.enumerateStates(basis, 1)
    op = LocalOperator(h, reps, dtype)
    if state is None:
        state = lanczos_smallest(op, num_evals=1, eps=eps).eigenvectors[0]
    state = state.to(dtype).contiguous()
    if state.dim() != 1 or state.numel() != op.n_local:
        raise LsAmdError(f"kpm: state {tuple(state.shape)} must be a vector of {op.n_local} elements")
    if bounds is None:
        bounds = spectral_bounds(op)
    bounds = (float(bounds[0]), float(bounds[1]))
    v0 = torch.zeros_like(state)
    api.MatvecPlan(A, reps, dtype).matvec([state], [v0])
    before = op.matvecs
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    mu = chebyshev_moments(op, v0.reshape(-1, 1), num_moments, bounds)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res = KpmResult(mu, bounds, op.matvecs - before, op.plan.axpby_kernel(1), state=state)
    if energies is None:
        energies = chebyshev_grid(bounds, 2 * int(num_moments))
    energies = np.asarray(energies, dtype=np.float64)
    S = reconstruct(mu[0], bounds, energies)
    res.step_seconds = t2 - t1
    res.seconds = time.perf_counter() - t0
    return energies, S, res


def _operators_of(operators, obs, who):
    from . import api

    try:
        ops = list(operators)
    except TypeError:
        raise ValueError(f"{who}: operators: a list of api.Operator or of indices of the config's observables") from None
    if not 1 <= len(ops) <= 64:
        raise ValueError(f"{who}: {len(ops)} operators: 1 <= K <= 64")
    out = []
    for k, o in enumerate(ops):
        if isinstance(o, (int, np.integer)) and not isinstance(o, bool):
            if not 0 <= int(o) < len(obs):
                raise ValueError(f"{who}: operators[{k}] = {o}: the config has {len(obs)} observables")
            out.append(obs[int(o)])
        elif isinstance(o, api.Operator):
            out.append(o)
        else:
            raise ValueError(f"{who}: operators[{k}]: an api.Operator or the index of one of the config's observables")
    return out


def spectral_matrix(config, operators, state=None, num_moments: int = 256, energies=None, bounds=None, dtype=None,
                    eps: float = 1e-10, target=None, groups: str = "same"):
    """The spectral matrix S_ab(w) = <psi|A_a^+ delta(w - H) A_b|psi> of K operators on the absolute energy scale of H
    -> (energies, S [E, K, K] complex128, KpmMatrixResult).  operators: a list of api.Operator on the basis of the config, or of
    indices of the config's `observables`.  state, bounds, energies, dtype, eps, target and groups as spectral_function: without a
    target every operator must map the basis into itself; with one, every operator must map the config's sector into that ONE
    target sector (the refusal names the operator that does not), v_a = A_a psi is one api.CrossSectorPlan per operator into one
    column of an interleaved (n, K) block, and the config's Hamiltonian is re-compiled on the target basis.  The K^2 moment
    series come from K columns of matvecs (chebyshev_moment_matrices)."""
    import torch

    from . import api, config as _config
    from .diagonalize import LocalOperator, lanczos_smallest

    who = "spectral_matrix"
    t0 = time.perf_counter()
    basis, h, obs = _load(config, observables=True)
    ops = _operators_of(operators, obs, who)
    K = len(ops)
    dtype = dtype or torch.float64
    reps, _ = api.enumerateStates(basis, 1)
    if target is not None:
        tbasis = _target_basis(target)
        if groups not in api.CrossSectorPlan.GROUPS:
            raise ValueError(f"groups = {groups!r} is none of 'same', 'restrict', 'project'")
        if groups != "project":
            for k, A in enumerate(ops):
                try:
                    A.mapsSector(tbasis, explain=True, signs=True, subgroup=groups == "restrict")
                except LsAmdError as e:
                    raise LsAmdError(f"{who}: operators[{k}] does not map the config's sector into the target sector: {e}") from None
        h_t = api.Operator.fromSpec(tbasis, _config.OperatorSpec(_terms_of(h)))
        if not h_t.isHermitian:
            raise ValueError("kpm: the Hamiltonian is not Hermitian (Chebyshev moments need a real spectrum)")
        treps, _ = api.enumerateStates(tbasis, 1)
    if state is None:
        state = lanczos_smallest(LocalOperator(h, reps, dtype), num_evals=1, eps=eps).eigenvectors[0]
    state = state.to(dtype).contiguous()
    if state.dim() != 1 or state.numel() != reps[0].numel():
        raise LsAmdError(f"kpm: state {tuple(state.shape)} must be a vector of {reps[0].numel()} elements")
    op = LocalOperator(h_t, treps, dtype) if target is not None else LocalOperator(h, reps, dtype)
    if bounds is None:
        bounds = spectral_bounds(op)
    bounds = (float(bounds[0]), float(bounds[1]))
    V0 = torch.zeros((op.n_local, K), dtype=dtype, device=state.device)
    col = torch.zeros(op.n_local, dtype=dtype, device=state.device)
    for k, A in enumerate(ops):
        col.zero_()
        if target is not None:
            cross = api.CrossSectorPlan(A, reps[0], tbasis, treps[0], dtype, groups=groups)
            cross.apply(state, col)
            cross.destroy()
        else:
            try:
                api.MatvecPlan(A, reps, dtype).matvec([state], [col])
            except LsAmdError as e:
                raise LsAmdError(f"{who}: operators[{k}] cannot be applied inside the config's sector: {e}") from None
        V0[:, k] = col
    before = op.matvecs
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    mu = chebyshev_moment_matrices(op, V0, num_moments, bounds)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res = KpmMatrixResult(mu, bounds, op.matvecs - before, op.plan.axpby_kernel(K), op.plan.gram_kernel(K), state=state, target_states=V0)
    if energies is None:
        energies = chebyshev_grid(bounds, 2 * int(num_moments))
    energies = np.asarray(energies, dtype=np.float64)
    S = reconstruct_matrix(mu, bounds, energies)
    res.step_seconds = t2 - t1
    res.seconds = time.perf_counter() - t0
    return energies, S, res
