"""Chebyshev time evolution (Tal-Ezer and Kosloff, J. Chem. Phys. 81, 3967): e^{-iHt} psi and e^{-tau H} psi at any basis size the
matvec reaches.  With H~ = (H - b) / a mapped into [-1, 1] (a = (hi - lo) / 2, b = (hi + lo) / 2),

    e^{-iHt} psi    = e^{-ibt} sum_n (2 - delta_n0) (-i)^n J_n(at) T_n(H~) psi,
    e^{-tau H} psi  = e^{-lo tau} sum_n (2 - delta_n0) (-1)^n e^{-a tau} I_n(a tau) T_n(H~) psi,

on the recurrence v_{n+1} = 2 H~ v_n - v_{n-1} of kpm.py.  One order of the series is one call of
MatvecPlan.matvec_block_axpby_acc (ls_amd_matvec_block_axpby_acc): c_{n+1} v_{n+1} is added to the running sum Z in the pass that
finishes v_{n+1} or in one streaming pass behind it, and a real recurrence feeds a complex sum without a complex
copy of it.  The
series is cut at the smallest order N whose discarded coefficients sum to at most eps (|T_n| <= 1: that sum bounds the error
relative to |psi|); N grows like a t + O((a t)^(1/3)).  One-partition plans.  The coefficients are computed on the host in numpy."""
from __future__ import annotations

import cmath
import math
import os
import time
from dataclasses import dataclass

import numpy as np

from . import kpm
from ._lib import LsAmdError

__all__ = ["bessel_series", "propagator_coefficients", "propagate", "evolve", "autocorrelation", "EvolveResult",
           "thermal_correlation", "combine_sectors", "ThermalCorrelationResult", "thermal_expectation",
           "combine_sector_expectations", "ThermalExpectationResult"]

MAX_COLUMNS = 64
_BIG = 1e250


def bessel_series(x: float, eps: float, modified: bool = False) -> np.ndarray:
    """J_n(x) -- modified: e^{-x} I_n(x), x >= 0 -- for n = 0..N, N the smallest order whose discarded tail 2 sum_{n > N} |.| is
    <= eps.  Miller's downward recurrence f_{n-1} = (2n / x) f_n -+ f_{n+1} from an order far above |x|, rescaled whenever it
    passes 1e250, normalised by J_0 + 2 sum_k J_2k = 1 (e^{-x} (I_0 + 2 sum_k I_k) = 1).  J_n(-x) = (-1)^n J_n(x)."""
    x = float(x)
    eps = float(eps)
    if not math.isfinite(x):
        raise ValueError(f"bessel_series: x = {x!r} is not finite")
    if not eps > 0.0:
        raise ValueError(f"bessel_series: eps = {eps!r} must be positive")
    if modified and x < 0.0:
        raise ValueError(f"bessel_series: x = {x!r} is negative (e^{{-x}} I_n(x) is computed for x >= 0)")
    if x == 0.0:
        return np.ones(1, dtype=np.float64)
    ax = abs(x)
    # far enough above the turning point n = |x| that f_M / f_N is below every double: the start values (0, 1) are then as good
    # as the true ones
    M = 2 * int(math.ceil(0.55 * ax + 15.0 * (ax ** (1.0 / 3.0) + 1.0) + 30.0))
    f = np.zeros(M + 2, dtype=np.float64)
    f[M] = 1.0
    hi, cur = 0.0, 1.0  # f[n + 1], f[n]
    sign = 1.0 if modified else -1.0
    for n in range(M, 0, -1):
        nxt = (2.0 * n / ax) * cur + sign * hi
        hi, cur = cur, nxt
        f[n - 1] = cur
        if abs(cur) > _BIG:
            f[n - 1:] *= 1.0 / _BIG
            hi *= 1.0 / _BIG
            cur *= 1.0 / _BIG
    if modified:
        norm = f[0] + 2.0 * f[1:].sum()
    else:
        norm = f[0] + 2.0 * f[2::2].sum()
    f /= norm
    if x < 0.0:
        f[1::2] = -f[1::2]
    tail = 2.0 * np.concatenate([np.cumsum(np.abs(f[::-1]))[::-1][1:], [0.0]])  # tail[N] = 2 sum_{n > N} |f_n|
    N = int(np.argmax(tail <= eps))
    return f[:N + 1].copy()


def _check_bounds(bounds):
    try:
        lo, hi = float(bounds[0]), float(bounds[1])
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"bounds = {bounds!r}: need finite lo < hi") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"bounds = ({bounds[0]!r}, {bounds[1]!r}): need finite lo < hi")
    return lo, hi


def propagator_coefficients(t: float, bounds, eps: float = 1e-12, imaginary: bool = False, reference_energy=None):
    """(c[0..N], prefactor) of  prefactor * sum_n c_n T_n(H~):
    real time       c_n = (2 - delta_n0) (-i)^n J_n(a t)             (complex128), prefactor e^{-i b t}; t of either sign;
    imaginary time  c_n = (2 - delta_n0) (-1)^n e^{-a t} I_n(a t)     (float64),    prefactor e^{-(lo - E_ref) t}, t >= 0:
                    e^{-t (H - E_ref)}, E_ref = reference_energy or lo -- nothing in it can overflow.
    N is the smallest order with 2 sum_{n > N} |J_n| <= eps (bessel_series)."""
    lo, hi = _check_bounds(bounds)
    t = float(t)
    if not math.isfinite(t):
        raise ValueError(f"t = {t!r} is not finite")
    a, b = 0.5 * (hi - lo), 0.5 * (hi + lo)
    if imaginary:
        if t < 0.0:
            raise ValueError(f"t = {t!r}: imaginary-time evolution needs t >= 0")
        e_ref = lo if reference_energy is None else float(reference_energy)
        f = bessel_series(a * t, eps, modified=True)
        c = 2.0 * f
        c[0] = f[0]
        c[1::2] = -c[1::2]
        return c, math.exp(-(lo - e_ref) * t)
    f = bessel_series(a * t, eps)
    c = (2.0 * f).astype(np.complex128)
    c[0] = f[0]
    c *= np.array([1.0, -1.0j, -1.0, 1.0j])[np.arange(len(f)) % 4]
    return c, cmath.exp(-1j * b * t)


def _check_operator(op):
    """what propagate asks of its operator, before anything touches the device"""
    if not op.plan.matrix.isHermitian:
        raise ValueError("evolve: the Hamiltonian is not Hermitian (the Chebyshev propagator needs a real spectrum)")
    if len(op.sizes) != 1:
        raise LsAmdError("evolve: one-partition plans only")


def propagate(op, state, t: float, bounds=None, eps: float = 1e-12, imaginary: bool = False, reference_energy=None, _info=None):
    """e^{-iHt} state (imaginary: e^{-t (H - E_ref)} state, E_ref = reference_energy or bounds[0]) as a new device tensor: a
    vector, or an (n, K) block of K <= 64 states.  op: a diagonalize.LocalOperator on one partition over a Hermitian operator;
    bounds: (lo, hi) enclosing its spectrum (kpm.spectral_bounds(op) when None).  The recurrence runs in op.dtype; the sum is
    complex128 in real time and op.dtype in imaginary time.  Three blocks of memory.  Every kpm.GUARD_EVERY orders the norms of
    the recurrence are read back (the only host synchronisation): bounds that do not enclose the spectrum raise LsAmdError."""
    import torch

    cplx_state = bool(state.is_complex())
    K = 1 if state.dim() == 1 else (int(state.shape[1]) if state.dim() == 2 else -1)
    if K < 0:
        raise LsAmdError(f"evolve: state {tuple(state.shape)} must be a vector or an (n, K) block")
    if K > MAX_COLUMNS or K < 1:
        raise LsAmdError(f"evolve: K = {K} columns: 1 <= K <= {MAX_COLUMNS}")
    _check_operator(op)
    if cplx_state and op.dtype != torch.complex128:
        raise LsAmdError("evolve: the state is complex and the operator computes in float64: build the operator with "
                         "dtype=torch.complex128")
    if state.shape[0] != op.n_local:
        raise LsAmdError(f"evolve: state {tuple(state.shape)} must have {op.n_local} rows")
    if bounds is not None:
        bounds = _check_bounds(bounds)
    else:
        bounds = _check_bounds(kpm.spectral_bounds(op))
    lo, hi = bounds
    a, b = 0.5 * (hi - lo), 0.5 * (hi + lo)
    c, prefactor = propagator_coefficients(t, bounds, eps, imaginary, reference_energy)
    N = len(c) - 1
    zdtype = op.dtype if imaginary else torch.complex128
    X = state.reshape(op.n_local, K).to(op.dtype).contiguous().clone()
    Z = (X * (float(c[0]) if imaginary else complex(c[0]))).to(zdtype)
    plan = op.plan
    if N > 0:
        Y = torch.empty_like(X)
        dots = torch.zeros((N, 2 * K), dtype=torch.float64, device=X.device)
        host = np.empty((N, 2 * K), dtype=np.float64)
        checked = 0

        def read_back(upto):
            nonlocal checked
            host[checked:upto] = dots[checked:upto].cpu().numpy()
            plan.check()
            kpm.check_guard(np.concatenate([host[:1], host[checked:upto]]), K, (lo, hi), first_step=checked - 1)
            checked = upto

        for s in range(N):
            cn = complex(c[s + 1])
            if s == 0:
                plan.matvec_block_axpby_acc(X, Y, 1.0 / a, -b / a, 0.0, Z, cn, dots=dots[0], check=False)
            else:
                plan.matvec_block_axpby_acc(X, Y, 2.0 / a, -2.0 * b / a, -1.0, Z, cn, dots=dots[s], check=False)
            X, Y = Y, X
            op.matvecs += K
            if (s + 1) % kpm.GUARD_EVERY == 0:
                read_back(s + 1)
        if checked < N:
            read_back(N)
    if prefactor != 1.0:
        Z.mul_(prefactor)
    if _info is not None:
        _info["order"] = N
        _info["bounds"] = bounds
    return Z.reshape(-1) if state.dim() == 1 else Z


@dataclass
class EvolveResult:
    times: np.ndarray         # [T] the output times
    values: np.ndarray        # [T, n_obs, K] complex128: <psi_k(t)|O|psi_k(t)> (not divided by the norm)
    norms: np.ndarray         # [T, K] float64: |psi_k(t)|
    orders: np.ndarray        # [T] int: the order N of the segment that ends at times[j]
    bounds: tuple             # (lo, hi) the spectrum was rescaled with
    matvec_columns: int       # columns that went through H in the propagation (K per order)
    kernel: str               # MatvecPlan.acc_kernel(K): "epilogue", "k_*_cheb+k_axpby_acc" (default) or "k_*_evolve" (LS_AMD_ACC=fused)
    seconds: float = 0.0      # wall time of the driver
    states: object = None     # keep_states: [T] device tensors, psi(times[j])


def _observable(ob, obs, api):
    if isinstance(ob, (int, np.integer)) and not isinstance(ob, bool):
        if obs is None:
            raise ValueError("observables: an index needs a config with an `observables:` section")
        if not 0 <= int(ob) < len(obs):
            raise ValueError(f"observable = {ob}: the config has {len(obs)} observables")
        return obs[int(ob)]
    if isinstance(ob, api.Operator):
        return ob
    raise ValueError("observables: api.Operator objects or indices into the config's observables")


def evolve(config_or_op, state, times, observables=None, keep_states: bool = False, bounds=None, eps: float = 1e-12,
           imaginary: bool = False, reference_energy=None):
    """psi(t) = e^{-iHt} state (imaginary: e^{-t (H - E_ref)} state) at the ascending `times`, segment by segment from the
    previous time, with <psi(t)|O|psi(t)> of every observable (api.Operator on the same basis, or an index into the config's
    `observables:`) and the norms at every time.  config_or_op: a config (dict or YAML path) with a `hamiltonian:`, or a
    diagonalize.LocalOperator.  state: a device vector or (n, K) block, K <= 64.  A real state under a real Hamiltonian with real
    characters runs its first segment in float64 (the sum is complex128); the complex operator of the later segments is made
    here.  -> EvolveResult."""
    import torch

    from . import api
    from .diagonalize import LocalOperator

    t0 = time.perf_counter()
    ts = np.atleast_1d(np.asarray(times, dtype=np.float64))
    if ts.ndim != 1 or ts.size == 0 or not np.isfinite(ts).all() or (np.diff(ts) < 0.0).any():
        raise ValueError("times: a non-empty ascending sequence of finite numbers")
    K = 1 if state.dim() == 1 else (int(state.shape[1]) if state.dim() == 2 else -1)
    if K < 1 or K > MAX_COLUMNS:
        raise LsAmdError(f"evolve: state {tuple(state.shape)} must be a vector or an (n, K) block, 1 <= K <= {MAX_COLUMNS}")
    if bounds is not None:
        bounds = _check_bounds(bounds)
    obs = None
    if isinstance(config_or_op, LocalOperator):
        op0 = config_or_op
        _check_operator(op0)
        h, reps = op0.plan.matrix, op0.reps
        ops = {op0.dtype: op0}
        if state.is_complex() and op0.dtype != torch.complex128:
            raise LsAmdError("evolve: the state is complex and the operator computes in float64: build the operator with "
                             "dtype=torch.complex128")
        first = op0.dtype
    else:
        from .entanglement import _complex_characters

        loaded = kpm._load(config_or_op, observables=True)
        basis, h = loaded[0], loaded[1]
        obs = loaded[2]
        reps, _ = api.enumerateStates(basis, 1)
        real = h.isReal and not _complex_characters(basis) and not state.is_complex()
        first = torch.float64 if real else torch.complex128
        ops = {}
    wanted = [_observable(ob, obs, api) for ob in (observables or [])]

    def op_of(dtype):
        if dtype not in ops:
            ops[dtype] = LocalOperator(h, reps, dtype)
        return ops[dtype]

    oplans = {}

    def expectation(j, psi):
        block = psi.reshape(psi.shape[0], K)
        out = np.empty((len(wanted), K), dtype=np.complex128)
        tmp = None
        for q, O in enumerate(wanted):
            key = (q, block.dtype)
            if key not in oplans:
                oplans[key] = LocalOperator(O, reps, block.dtype)
            tmp = torch.empty_like(block) if tmp is None else tmp
            if K == 1:
                oplans[key].matvec(block[:, 0], tmp[:, 0])
            else:
                oplans[key].matvec_block(block, tmp)
            oplans[key].check()
            out[q] = (block.conj() * tmp).sum(dim=0).cpu().numpy()
        return out

    op = op_of(first)
    if bounds is None:
        bounds = _check_bounds(kpm.spectral_bounds(op))
    psi = state.to(first)
    if psi.shape[0] != op.n_local:
        raise LsAmdError(f"evolve: state {tuple(state.shape)} must have {op.n_local} rows")
    T = len(ts)
    values = np.zeros((T, len(wanted), K), dtype=np.complex128)
    norms = np.zeros((T, K), dtype=np.float64)
    orders = np.zeros(T, dtype=np.int64)
    states = [] if keep_states else None
    columns, kernel, prev = 0, None, 0.0
    for j, tj in enumerate(ts):
        dt = float(tj) - prev
        if dt != 0.0:
            if psi.is_complex() and op.dtype != torch.complex128:
                op = op_of(torch.complex128)
            info, before = {}, op.matvecs
            psi = propagate(op, psi, dt, bounds=bounds, eps=eps, imaginary=imaginary, reference_energy=reference_energy, _info=info)
            orders[j] = info["order"]
            columns += op.matvecs - before
            kernel = kernel or op.plan.acc_kernel(K)
            prev = float(tj)
        norms[j] = torch.linalg.vector_norm(psi.reshape(psi.shape[0], K), dim=0).cpu().numpy()
        if wanted:
            values[j] = expectation(j, psi)
        if keep_states:
            states.append(psi if dt != 0.0 else psi.clone())
    res = EvolveResult(ts, values, norms, orders, bounds, columns, kernel or op.plan.acc_kernel(K), states=states)
    res.seconds = time.perf_counter() - t0
    return res


def autocorrelation(moments, bounds, times, eps: float = 1e-12) -> np.ndarray:
    """<v0|e^{-iHt}|v0> = e^{-ibt} sum_n c_n(t) mu_n from the undamped Chebyshev moments mu_n = <v0|T_n(H~)|v0> [M] (or [..., M])
    that kpm.chebyshev_moments returns for the same bounds: the Loschmidt amplitude -- with v0 = A|psi>, <psi|A^+(t) A|psi> up to
    the phase of |psi> -- at the times [T] -> complex128 [T] (or [..., T]).  Host only.  ValueError when there are fewer moments
    than the order the series needs for `eps` at some time."""
    mu = np.asarray(moments, dtype=np.float64)
    lo, hi = _check_bounds(bounds)
    ts = np.atleast_1d(np.asarray(times, dtype=np.float64))
    M = mu.shape[-1]
    out = np.empty(mu.shape[:-1] + (len(ts),), dtype=np.complex128)
    for j, t in enumerate(ts):
        c, pref = propagator_coefficients(float(t), (lo, hi), eps)
        if len(c) > M:
            raise ValueError(f"autocorrelation: t = {float(t)!r} needs {len(c)} moments for eps = {eps!r}, {M} were given")
        out[..., j] = pref * (mu[..., :len(c)] @ c)
    return out


# ---- finite temperature: C(t) = <A^+(t) A(0)>_beta by dynamical quantum typicality ----
@dataclass
class ThermalCorrelationResult:
    times: np.ndarray         # [T] the output times
    numerator: np.ndarray     # [T, K] complex128: N_k(t) = <A beta_k(t)|phi_k(t)>, |beta_k> = e^{-(beta/2)(H - E_ref)} R_k, |phi_k> = A|beta_k>
    partition: np.ndarray     # [K] float64: Z_k = <beta_k|beta_k>
    correlation: np.ndarray   # [T] complex128: sum_k N_k(t) / sum_k Z_k
    dimension: int            # D_s, the dimension of the source sector (the weight of this sector in combine_sectors)
    reference_energy: float   # E_ref of the cooling step
    bounds: tuple             # (lo, hi) both spectra were rescaled with
    orders: np.ndarray        # [T] int: the order N of the segment that ends at times[j] (the same in both sectors)
    kernel: str               # CrossSectorPlan.block_kernel(K)
    matvec_columns: int       # columns that went through H in the cooling and the propagation, both sectors
    seconds: float = 0.0      # wall time of the driver


# what thermal_correlation passes to CrossSectorPlan.apply_block for groups="project" when neither block_method nor
# LS_AMD_CROSS_PROJECT_BLOCK says otherwise: the block kernel took 0.21 x the time of the column loop on both bench shapes at K = 8
# interleaved ("Projecting block apply").  A bare plan stays on "columns".
PROJECT_BLOCK_METHOD = "kernel"


def thermal_correlation(config, operator, beta, times, num_vectors: int = 8, seed: int = 0, vectors=None, target=None,
                        groups: str = "same", bounds=None, reference_energy=None, eps: float = 1e-12, block_method=None):
    """C(t) = <A^+(t) A(0)>_beta = Tr[e^{-beta H} e^{iHt} A^+ e^{-iHt} A] / Tr e^{-beta H} inside the symmetry sector of the config,
    by dynamical quantum typicality: the trace is the average over K random vectors R_k cooled to |beta_k> = e^{-(beta/2)(H - E_ref)}
    R_k (skipped at beta = 0), and with |phi_k> = A|beta_k>

        N_k(t) = <A e^{-iHt} beta_k | e^{-iHt} phi_k>,    Z_k = <beta_k|beta_k>,    C(t) ~ sum_k N_k(t) / sum_k Z_k,

    exactly C(t) of the sector when the R_k are a whole orthonormal basis of it.  config, operator, target and groups mean what they
    mean for kpm.spectral_function: operator is an api.Operator on the config's basis (or the index of one of its `observables:`);
    target is the sector A maps INTO (None: the config's own), where the config's `hamiltonian:` is re-compiled; the left vector
    moves in the source sector, the right one in the target sector, segment by segment as evolve does, and every output time costs
    one CrossSectorPlan.apply_block and K column dots.  Everything runs in complex128.
    vectors: an (D_s, K) device block, K <= 64; None: kpm.random_phase_block(D_s, num_vectors, complex128, seed).
    bounds: ONE (lo, hi) pair that encloses the spectrum in BOTH sectors; None: the union of kpm.spectral_bounds of the two.
    reference_energy: E_ref, bounds[0] when None -- an argument so that several sectors share one (combine_sectors).
    eps: the cut of every Chebyshev series, relative to the norm of the vector that comes OUT of it: the cooling step, which
    shrinks its vector, is cut at eps times the smallest shrink factor of the block (and repeated when that was underestimated).
    block_method: the method of both CrossSectorPlan.apply_block calls, "columns" or "kernel" (it matters for groups="project" only);
    None: LS_AMD_CROSS_PROJECT_BLOCK where it is set, else PROJECT_BLOCK_METHOD for groups="project".
    -> ThermalCorrelationResult."""
    from . import api, config as _config

    t0 = time.perf_counter()
    # everything that can be refused without the device
    try:
        beta = float(beta)
    except (TypeError, ValueError):
        raise ValueError(f"beta = {beta!r}: need a finite number >= 0") from None
    if not (math.isfinite(beta) and beta >= 0.0):
        raise ValueError(f"beta = {beta!r}: need a finite number >= 0")
    ts = np.atleast_1d(np.asarray(times, dtype=np.float64))
    if ts.ndim != 1 or ts.size == 0 or not np.isfinite(ts).all() or (np.diff(ts) < 0.0).any():
        raise ValueError("times: a non-empty ascending sequence of finite numbers")
    if not float(eps) > 0.0:
        raise ValueError(f"eps = {eps!r} must be positive")
    if bounds is not None:
        bounds = _check_bounds(bounds)
    if reference_energy is not None and not math.isfinite(float(reference_energy)):
        raise ValueError(f"reference_energy = {reference_energy!r} is not finite")
    if groups not in api.CrossSectorPlan.GROUPS:
        raise ValueError(f"groups = {groups!r} is none of 'same', 'restrict', 'project'")
    if not isinstance(block_method, (str, type(None))) or block_method not in api.CrossSectorPlan.BLOCK_METHODS:
        raise ValueError(f"block_method = {block_method!r} is none of None, 'columns', 'kernel'")
    if block_method is None and groups == "project" and not os.environ.get("LS_AMD_CROSS_PROJECT_BLOCK"):
        block_method = PROJECT_BLOCK_METHOD
    if vectors is None:
        if isinstance(num_vectors, bool) or not isinstance(num_vectors, (int, np.integer)) or not 1 <= int(num_vectors) <= MAX_COLUMNS:
            raise ValueError(f"num_vectors = {num_vectors!r}: 1 <= num_vectors <= {MAX_COLUMNS}")
    else:
        if isinstance(vectors, (list, tuple)):
            raise LsAmdError("thermal_correlation: one-partition blocks only (vectors is one (D_s, K) device tensor)")
        if not hasattr(vectors, "dim") or vectors.dim() != 2 or not 1 <= int(vectors.shape[1]) <= MAX_COLUMNS:
            raise LsAmdError(f"thermal_correlation: vectors must be an (D_s, K) block, 1 <= K <= {MAX_COLUMNS}")
        if vectors.device.type != "cuda":
            raise LsAmdError("thermal_correlation: vectors must be a device tensor")
    basis, h, obs = kpm._load(config, observables=True)  # (refuses a Hamiltonian that is not Hermitian)
    if isinstance(operator, (int, np.integer)) and not isinstance(operator, bool):
        if obs is None or not 0 <= int(operator) < len(obs):
            raise ValueError(f"operator = {operator}: the config has {0 if obs is None else len(obs)} observables")
        A = obs[int(operator)]
    elif isinstance(operator, api.Operator):
        A = operator
    else:
        raise ValueError("operator: an api.Operator (on the source basis) or the index of one of the config's observables")
    tbasis = basis if target is None else kpm._target_basis(target)
    if groups != "project":  # (a projecting plan asks nothing of the operator)
        A.mapsSector(tbasis, explain=True, signs=True, subgroup=groups == "restrict")
    h_t = h if target is None else api.Operator.fromSpec(tbasis, _config.OperatorSpec(kpm._terms_of(h)))
    if not h_t.isHermitian:
        raise ValueError("thermal_correlation: the Hamiltonian is not Hermitian on the target basis")

    import torch

    from .diagonalize import LocalOperator

    c128 = torch.complex128
    reps, _ = api.enumerateStates(basis, 1)
    treps = reps if target is None else api.enumerateStates(tbasis, 1)[0]
    op_s = LocalOperator(h, reps, c128)
    op_t = op_s if target is None else LocalOperator(h_t, treps, c128)
    D_s = int(op_s.n_local)
    if vectors is None:
        R = kpm.random_phase_block(D_s, int(num_vectors), c128, seed, device=op_s.device)
    else:
        if vectors.shape[0] != D_s:
            raise LsAmdError(f"thermal_correlation: vectors {tuple(vectors.shape)} must have {D_s} rows (the source sector)")
        R = vectors.to(c128)
    K = int(R.shape[1])
    if bounds is None:
        b_s = kpm.spectral_bounds(op_s)
        b_t = b_s if op_t is op_s else kpm.spectral_bounds(op_t)
        bounds = _check_bounds((min(b_s[0], b_t[0]), max(b_s[1], b_t[1])))
    e_ref = float(bounds[0]) if reference_energy is None else float(reference_energy)
    cross = api.CrossSectorPlan(A, reps[0], tbasis, treps[0], c128, groups=groups)
    try:
        before = op_s.matvecs + (0 if op_t is op_s else op_t.matvecs)
        if beta > 0.0:
            # propagate cuts its series at eps relative to the norm of R_k, and cooling shrinks the vector -- by e^{-(beta/2)(E_0 - lo)}
            # at least, E_0 the sector's lowest level, lo the lower bound shared with the other sector -- so the cut is made at
            # eps times the smallest shrink factor s = |beta_k| / |R_k|: eps holds relative to |beta_k>.  s is known only afterwards;
            # the series falls faster than geometrically beyond order a beta / 2, so three digits in advance cost a few orders,
            # and the pass is repeated only when s turns out smaller than that.
            r_norm = torch.linalg.vector_norm(R, dim=0) * math.exp(-(bounds[0] - e_ref) * 0.5 * beta)  # (the exact prefactor is no shrinking)
            eps_c = 1e-3 * float(eps)
            for _ in range(3):
                left = propagate(op_s, R, 0.5 * beta, bounds=bounds, eps=max(eps_c, 1e-300), imaginary=True, reference_energy=e_ref)
                shrink = float((torch.linalg.vector_norm(left, dim=0) / r_norm).min())
                if not shrink > 0.0 or eps_c <= float(eps) * shrink:
                    break
                eps_c = 0.1 * float(eps) * shrink
        else:
            left = R.contiguous().clone()
        Z = (left.real ** 2 + left.imag ** 2).sum(dim=0).cpu().numpy()
        right = torch.empty((op_t.n_local, K), dtype=c128, device=left.device)
        cross.apply_block(left, right, method=block_method)
        image = torch.empty_like(right)
        T = len(ts)
        numerator = np.zeros((T, K), dtype=np.complex128)
        orders = np.zeros(T, dtype=np.int64)
        prev = 0.0
        for j, tj in enumerate(ts):
            dt = float(tj) - prev
            if dt != 0.0:
                info = {}
                left = propagate(op_s, left, dt, bounds=bounds, eps=eps, _info=info)
                right = propagate(op_t, right, dt, bounds=bounds, eps=eps)
                orders[j] = info["order"]
                prev = float(tj)
            cross.apply_block(left, image, method=block_method)
            numerator[j] = (image.conj() * right).sum(dim=0).cpu().numpy()
        columns = op_s.matvecs + (0 if op_t is op_s else op_t.matvecs) - before
        kernel = cross.block_kernel(K, block_method)
    finally:
        cross.destroy()
    res = ThermalCorrelationResult(ts, numerator, Z, numerator.sum(axis=1) / Z.sum(), D_s, e_ref, bounds, orders, kernel, int(columns))
    res.seconds = time.perf_counter() - t0
    return res


def combine_sectors(results) -> np.ndarray:
    """C(t) of the ensemble over several symmetry sectors from their thermal_correlation results (host only):

        C(t) = sum_s (D_s / K_s) sum_k N_{s,k}(t)  /  sum_s (D_s / K_s) sum_k Z_{s,k}

    -- every sector's stochastic trace estimates Tr_s with the weight D_s / K_s.  The results must share their `times` and their
    `reference_energy` (the Boltzmann weights of two sectors are comparable only on one energy scale): ValueError otherwise.
    -> complex128 [T]."""
    results = list(results)
    if not results:
        raise ValueError("combine_sectors: no results")
    first = results[0]
    num = np.zeros(len(first.times), dtype=np.complex128)
    den = 0.0
    for s, r in enumerate(results):
        if not np.array_equal(np.asarray(r.times), np.asarray(first.times)):
            raise ValueError(f"combine_sectors: result {s} has other times than result 0")
        if float(r.reference_energy) != float(first.reference_energy):
            raise ValueError(f"combine_sectors: result {s} has reference_energy {r.reference_energy!r}, result 0 {first.reference_energy!r} "
                             "(pass one reference_energy to every thermal_correlation)")
        N = np.asarray(r.numerator)
        Zk = np.asarray(r.partition)
        K = Zk.shape[0]
        if K < 1 or N.shape != (len(first.times), K) or not int(r.dimension) >= 1:
            raise ValueError(f"combine_sectors: result {s} is malformed (numerator {N.shape}, partition {Zk.shape}, dimension {r.dimension!r})")
        w = float(r.dimension) / K
        num += w * N.sum(axis=1)
        den += w * float(Zk.sum())
    return num / den


# ---- finite temperature, static: <O>_beta, E(beta), C(beta), S(beta) by canonical typicality ----
@dataclass
class ThermalExpectationResult:
    betas: np.ndarray              # [B] the inverse temperatures
    numerator: np.ndarray          # [B, n_ops, K] complex128: <beta_k|O|beta_k>, |beta_k> = e^{-(beta/2)(H - E_ref)} R_k
    partition: np.ndarray          # [B, K] float64: Z_k = <beta_k|beta_k>
    energy_numerator: np.ndarray   # [B, K] float64: <beta_k|H|beta_k>
    energy2_numerator: np.ndarray  # [B, K] float64: |H beta_k|^2
    values: np.ndarray             # [B, n_ops] complex128: sum_k numerator / sum_k partition
    energy: np.ndarray             # [B] <H>_beta
    specific_heat: np.ndarray      # [B] beta^2 (<H^2> - <H>^2)
    log_partition: np.ndarray      # [B] ln Tr e^{-beta H} = ln((D / K) sum_k Z_k) - beta E_ref
    entropy: np.ndarray            # [B] log_partition + beta energy
    dimension: int                 # D, the dimension of the sector (its weight in combine_sector_expectations)
    reference_energy: float        # E_ref of the cooling
    bounds: tuple                  # (lo, hi) the spectrum was rescaled with
    orders: np.ndarray             # [B] int: the order N of the cooling segment that ends at betas[j]
    kernel: str                    # ExpectationPlan.block_kernel(K)
    matvec_columns: int            # columns that went through H, cooling and energies
    seconds: float = 0.0           # wall time of the driver
    expectation_seconds: float = 0.0  # of which inside ExpectationPlan.values_block


def _thermal_derived(betas, num, Z, E1, E2, weight, e_ref):
    """the ensemble quantities from the sums over the columns: num [B, n_ops], Z, E1, E2 [B]; weight = D / K of the trace estimate"""
    values = num / Z[:, None]
    energy = E1 / Z
    heat = betas ** 2 * (E2 / Z - energy ** 2)
    logz = np.log(weight * Z) - betas * e_ref
    return values, energy, heat, logz, logz + betas * energy


def _cool(op, block, tau, bounds, e_ref, eps):
    """e^{-tau (H - E_ref)} block with the series cut at eps relative to the vector that comes OUT: the rule of thermal_correlation,
    for one segment -> (block, order)"""
    import torch

    r_norm = torch.linalg.vector_norm(block, dim=0) * math.exp(-(bounds[0] - e_ref) * tau)  # (the exact prefactor is no shrinking)
    eps_c = 1e-3 * float(eps)
    info = {}
    for _ in range(3):
        out = propagate(op, block, tau, bounds=bounds, eps=max(eps_c, 1e-300), imaginary=True, reference_energy=e_ref, _info=info)
        shrink = float((torch.linalg.vector_norm(out, dim=0) / r_norm).min())
        if not shrink > 0.0 or eps_c <= float(eps) * shrink:
            break
        eps_c = 0.1 * float(eps) * shrink
    return out, int(info["order"])


def thermal_expectation(config, operators, betas, num_vectors: int = 8, seed: int = 0, vectors=None, bounds=None, reference_energy=None,
                        eps: float = 1e-12, dtype=None):
    """<O>_beta = Tr[e^{-beta H} O] / Tr e^{-beta H} of every operator, the energy, the specific heat, ln Z and the entropy inside the
    symmetry sector of the config at every inverse temperature of `betas`, by canonical typicality: the trace is the average over K
    random vectors R_k cooled to |beta_k> = e^{-(beta/2)(H - E_ref)} R_k,

        <O>_beta ~ sum_k <beta_k|O|beta_k> / sum_k <beta_k|beta_k>,

    exactly the sector's when the R_k are a whole orthonormal basis of it.  The block is cooled ONCE, from each beta to the next, so
    the grid costs what its largest beta costs; at every beta one MatvecPlan.matvec_block_axpby gives <beta_k|beta_k> and
    <beta_k|H|beta_k>, a column norm |H beta_k|^2, and ONE ExpectationPlan.values_block the K values of every operator.
    operators: what ExpectationPlan accepts (Operators, OperatorSpecs, operator sections; the operators need not be invariant under
    the sector's group), or integer indices into the config's `observables:`.  betas: a non-empty ascending sequence of finite numbers
    >= 0.  vectors: an (D, K) device block, K <= 64; None: kpm.random_phase_block(D, num_vectors, dtype, seed) -- random signs in
    float64, random phases in complex128.  dtype None: float64 when the Hamiltonian is real, the characters are +-1 and `vectors` is
    real, else complex128; torch.float64 where that cannot be honoured is refused.  bounds, reference_energy, eps: as
    thermal_correlation; the cut of every cooling segment is relative to the vector that comes out of it.
    -> ThermalExpectationResult."""
    from . import api, config as _config, expectation as _expectation
    from .entanglement import _complex_characters

    t0 = time.perf_counter()
    # everything that can be refused without the device
    try:
        bs = np.atleast_1d(np.asarray(betas, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("betas: a non-empty ascending sequence of finite numbers >= 0") from None
    if bs.ndim != 1 or bs.size == 0 or not np.isfinite(bs).all() or (bs < 0.0).any() or (np.diff(bs) < 0.0).any():
        raise ValueError("betas: a non-empty ascending sequence of finite numbers >= 0")
    if not float(eps) > 0.0:
        raise ValueError(f"eps = {eps!r} must be positive")
    if bounds is not None:
        bounds = _check_bounds(bounds)
    if reference_energy is not None and not math.isfinite(float(reference_energy)):
        raise ValueError(f"reference_energy = {reference_energy!r} is not finite")
    if vectors is None:
        if isinstance(num_vectors, bool) or not isinstance(num_vectors, (int, np.integer)) or not 1 <= int(num_vectors) <= MAX_COLUMNS:
            raise ValueError(f"num_vectors = {num_vectors!r}: 1 <= num_vectors <= {MAX_COLUMNS}")
    else:
        if isinstance(vectors, (list, tuple)):
            raise LsAmdError("thermal_expectation: one-partition blocks only (vectors is one (D, K) device tensor)")
        if not hasattr(vectors, "dim") or vectors.dim() != 2 or not 1 <= int(vectors.shape[1]) <= MAX_COLUMNS:
            raise LsAmdError(f"thermal_expectation: vectors must be an (D, K) block, 1 <= K <= {MAX_COLUMNS}")
        if vectors.device.type != "cuda":
            raise LsAmdError("thermal_expectation: vectors must be a device tensor")
    basis, h, obs = kpm._load(config, observables=True)  # (refuses a Hamiltonian that is not Hermitian)
    if isinstance(operators, (dict, _config.OperatorSpec, api.Operator)) or isinstance(operators, (int, np.integer)) or not hasattr(operators, "__iter__"):
        operators = [operators]
    operators = list(operators)
    if not operators:
        raise ValueError("thermal_expectation: no operators")
    ops = []
    for k, item in enumerate(operators):
        if isinstance(item, (int, np.integer)) and not isinstance(item, bool):
            if obs is None or not 0 <= int(item) < len(obs):
                raise ValueError(f"operators[{k}] = {item}: the config has {0 if obs is None else len(obs)} observables")
            item = obs[int(item)]
        ops.append(_expectation._as_operator(basis, item, k))  # (refuses by name what ExpectationPlan refuses)

    import torch

    real = bool(h.isReal) and not _complex_characters(basis) and (vectors is None or not vectors.is_complex())
    if dtype is None:
        dtype = torch.float64 if real else torch.complex128
    if dtype not in (torch.float64, torch.complex128):
        raise ValueError(f"thermal_expectation: dtype = {dtype!r} is neither torch.float64 nor torch.complex128")
    if dtype == torch.float64 and not real:
        why = "the Hamiltonian is complex" if not h.isReal else ("the characters of the sector are complex" if _complex_characters(basis) else "vectors is complex")
        raise LsAmdError(f"thermal_expectation: dtype = torch.float64 cannot be honoured: {why} (use torch.complex128)")

    from .diagonalize import LocalOperator

    reps, _ = api.enumerateStates(basis, 1)
    if len(reps) != 1:
        raise LsAmdError("thermal_expectation: one-partition plans only")
    op = LocalOperator(h, reps, dtype)
    _check_operator(op)
    D = int(op.n_local)
    if vectors is None:
        R = kpm.random_phase_block(D, int(num_vectors), dtype, seed, device=op.device)
    else:
        if vectors.shape[0] != D:
            raise LsAmdError(f"thermal_expectation: vectors {tuple(vectors.shape)} must have {D} rows (the sector)")
        R = vectors.to(dtype)
    K = int(R.shape[1])
    if bounds is None:
        bounds = _check_bounds(kpm.spectral_bounds(op))
    e_ref = float(bounds[0]) if reference_energy is None else float(reference_energy)
    plan = _expectation.ExpectationPlan(basis, reps[0], ops)
    try:
        B, n_ops = len(bs), plan.count
        numerator = np.zeros((B, n_ops, K), dtype=np.complex128)
        Z = np.zeros((B, K)); E1 = np.zeros((B, K)); E2 = np.zeros((B, K))
        orders = np.zeros(B, dtype=np.int64)
        before = op.matvecs
        block = R.contiguous().clone()
        Y = torch.empty_like(block)
        dots = torch.zeros(2 * K, dtype=torch.float64, device=block.device)
        t_exp = 0.0
        prev = 0.0
        for j, bj in enumerate(bs):
            db = float(bj) - prev
            if db != 0.0:
                block, orders[j] = _cool(op, block, 0.5 * db, bounds, e_ref, eps)
                prev = float(bj)
            op.plan.matvec_block_axpby(block, Y, 1.0, 0.0, 0.0, dots)  # Y = H block; dots = (<X|X>, <X|Y>)
            op.matvecs += K
            d = dots.cpu().numpy()
            Z[j], E1[j] = d[:K], d[K:]
            E2[j] = (torch.linalg.vector_norm(Y, dim=0) ** 2).cpu().numpy()
            t1 = time.perf_counter()
            numerator[j] = plan.values_block(block)
            t_exp += time.perf_counter() - t1
        kernel = plan.block_kernel(K)
        columns = op.matvecs - before
    finally:
        plan.destroy()
    values, energy, heat, logz, entropy = _thermal_derived(bs, numerator.sum(axis=2), Z.sum(axis=1), E1.sum(axis=1), E2.sum(axis=1),
                                                           D / K, e_ref)
    res = ThermalExpectationResult(bs, numerator, Z, E1, E2, values, energy, heat, logz, entropy, D, e_ref, bounds, orders, kernel,
                                   int(columns))
    res.seconds = time.perf_counter() - t0
    res.expectation_seconds = t_exp
    return res


def combine_sector_expectations(results) -> ThermalExpectationResult:
    """the ensemble over several symmetry sectors from their thermal_expectation results (host only): every sector's stochastic trace
    estimates Tr_s with the weight D_s / K_s, as in combine_sectors,

        <O>_beta = sum_s (D_s / K_s) sum_k <beta_k|O|beta_k>_s  /  sum_s (D_s / K_s) sum_k Z_{s,k},

    and likewise the energy, the specific heat, ln Z and the entropy.  The results must share their `betas`, their
    `reference_energy` and their number of operators: ValueError otherwise.  -> a ThermalExpectationResult of one column per beta
    that holds the weighted sums divided by the total dimension (so that its own fields obey the same relations)."""
    results = list(results)
    if not results:
        raise ValueError("combine_sector_expectations: no results")
    first = results[0]
    betas = np.asarray(first.betas, dtype=np.float64)
    B, n_ops = len(betas), np.asarray(first.numerator).shape[1]
    num = np.zeros((B, n_ops), dtype=np.complex128)
    Z = np.zeros(B); E1 = np.zeros(B); E2 = np.zeros(B)
    dim, columns, seconds, t_exp = 0, 0, 0.0, 0.0
    for s, r in enumerate(results):
        if not np.array_equal(np.asarray(r.betas), betas):
            raise ValueError(f"combine_sector_expectations: result {s} has other betas than result 0")
        if float(r.reference_energy) != float(first.reference_energy):
            raise ValueError(f"combine_sector_expectations: result {s} has reference_energy {r.reference_energy!r}, result 0 "
                             f"{first.reference_energy!r} (pass one reference_energy to every thermal_expectation)")
        N, Zk = np.asarray(r.numerator), np.asarray(r.partition)
        if N.ndim != 3 or N.shape[1] != n_ops:
            raise ValueError(f"combine_sector_expectations: result {s} has {N.shape[1] if N.ndim == 3 else '?'} operators, result 0 {n_ops}")
        K = Zk.shape[1] if Zk.ndim == 2 else 0
        if K < 1 or N.shape != (B, n_ops, K) or not int(r.dimension) >= 1:
            raise ValueError(f"combine_sector_expectations: result {s} is malformed (numerator {N.shape}, partition {Zk.shape}, "
                             f"dimension {r.dimension!r})")
        w = float(r.dimension) / K
        num += w * N.sum(axis=2)
        Z += w * Zk.sum(axis=1)
        E1 += w * np.asarray(r.energy_numerator).sum(axis=1)
        E2 += w * np.asarray(r.energy2_numerator).sum(axis=1)
        dim += int(r.dimension); columns += int(r.matvec_columns); seconds += float(r.seconds); t_exp += float(r.expectation_seconds)
    e_ref = float(first.reference_energy)
    num, Z, E1, E2 = num / dim, Z / dim, E1 / dim, E2 / dim
    values, energy, heat, logz, entropy = _thermal_derived(betas, num, Z, E1, E2, float(dim), e_ref)
    lo = min(float(r.bounds[0]) for r in results)
    hi = max(float(r.bounds[1]) for r in results)
    kernels = sorted({r.kernel for r in results})
    return ThermalExpectationResult(betas, num[:, :, None], Z[:, None], E1[:, None], E2[:, None], values, energy, heat, logz, entropy, dim,
                                    e_ref, (lo, hi), np.max([np.asarray(r.orders) for r in results], axis=0), "+".join(kernels), columns,
                                    seconds, t_exp)
