"""Two-point correlation matrices of a sector state in one pass (include/ls_amd.h: ls_amd_corr; csrc/k_corr.hip, k_corr_fermi.hip).

For a state psi on the representatives of a symmetry sector -- an eigenvector of diagonalize(), say -- over the M bits of a state word
(the sites of a spin or spinless basis; the 2 L modes of a spinful one, mode (i, up) = i, mode (i, down) = i + L):
    densities   d[i] = <b_i>, D[i][j] = <b_i b_j>, b_i = bit i of the product state          (kernel k_corr_diag, no look-up at all)
    hoppings    G[i][j] = <B+_i B_j>, B_j clears bit j and B+_i sets bit i, G[i][i] = d[i]   (kernel k_corr_hop / k_corr_hop_fermi)
S_i.S_j or c+_i c_j are not invariant under the sector's group, but the state is: the device sums over the representatives alone,
    R[i][j] = sum_r conj(psi_r) / n(r) (O_ij psi^)(r),      psi^(s) = conj(character(s)) [sign] norm(rep s) psi[index(rep s)],
and the host averages, C[i][j] = |G|^-1 sum_g R[g(i)][g(j)] (|G| M^2 operations; an element with the global spin inversion sends
D -> 1 - d_i - d_j + D_ij and (i, j) -> (j, i) on the hoppings, which takes a normalised state).  symmetrize=False returns R itself.
On fermionic bases the hopping kernel multiplies the Jordan-Wigner sign (-1)^popcount(state & between(i, j)) in: G[i][j] =
<c+_i c_j> in the mode order of the state word, the one the c+_i c_j terms of an Operator use.  No floating-point atomics: two calls
on the same input return the same bytes.  ONE partition, one state; nothing falls back to the CPU."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import LsAmdError
from .entanglement import _complex_characters, _stream_ptr

__all__ = ["CorrelationPlan", "SpinCorrelations", "FermionCorrelations", "spin_correlations", "fermion_correlations", "structure_factor",
           "correlations"]

SpinCorrelations = collections.namedtuple("SpinCorrelations", "z zz pm ss")
FermionCorrelations = collections.namedtuple("FermionCorrelations", "n nn one_body double_occupancy")


def _f64p(a):
    return a.ctypes.data_as(_lib.c_f64p)


class CorrelationPlan:
    """ls_amd_corr: the plan of the correlation matrices of vectors on `reps` (the ascending representatives of `basis`, a 1-D int64
    device tensor, one partition).  .modes = M.  psi is taken as it is: normalise it first (the group average of a basis with
    spin inversion assumes <psi|psi> = 1)."""

    def __init__(self, basis, reps):
        import torch

        if isinstance(reps, (list, tuple)):
            if len(reps) != 1:
                raise LsAmdError(f"CorrelationPlan: one partition (the whole sector on this device), got {len(reps)} blocks of representatives")
            reps = reps[0]
        if not isinstance(reps, torch.Tensor) or reps.dim() != 1 or reps.dtype != torch.int64 or not reps.is_contiguous():
            raise LsAmdError("CorrelationPlan: reps must be a contiguous 1-D int64 device tensor (one partition)")
        _lib.require_device()
        if reps.device.type != "cuda":
            raise LsAmdError("CorrelationPlan: reps must be a device tensor")
        self.basis, self.reps = basis, reps  # borrowed by the plan: keep alive
        self.complex_characters = _complex_characters(basis)
        h = C.c_void_p()
        _lib.check(_lib.load().ls_amd_corr_create(C.byref(h), basis.payload, C.c_void_p(reps.data_ptr()), reps.numel(), _stream_ptr()))
        self.h = h
        self.modes = int(_lib.load().ls_amd_corr_modes(h))

    def destroy(self):
        if getattr(self, "h", None):
            _lib.load().ls_amd_corr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def kernel(self, which):
        """the kernel of "densities" (0) or "hoppings" (1)"""
        which = {"densities": 0, "hoppings": 1}.get(which, which)
        name = _lib.load().ls_amd_corr_kernel_name(self.h, int(which))
        if name is None:
            _lib.check(-1)
        return name.decode()

    def _psi(self, who, psi):
        import torch

        n = int(self.reps.numel())
        if self.h is None:
            raise LsAmdError(f"CorrelationPlan.{who}: the plan was destroyed")
        if not isinstance(psi, torch.Tensor) or psi.device.type != "cuda":
            raise LsAmdError(f"CorrelationPlan.{who}: psi must be a device tensor (there is no CPU path)")
        if psi.dim() != 1 or psi.numel() != n:
            raise LsAmdError(f"CorrelationPlan.{who}: psi {tuple(psi.shape)} must be ONE vector of {n} elements")
        if psi.dtype not in (torch.float64, torch.complex128):
            raise LsAmdError(f"CorrelationPlan.{who}: psi is {psi.dtype}, neither float64 nor complex128")
        if psi.dtype == torch.float64 and self.complex_characters:
            psi = psi.to(torch.complex128)
        psi = psi if psi.is_contiguous() else psi.contiguous()
        return psi, (1 if psi.dtype == torch.complex128 else 0)

    def densities(self, psi, symmetrize: bool = True):
        """-> (d, D): numpy float64 arrays of shapes (M,) and (M, M)"""
        psi, dt = self._psi("densities", psi)
        M = self.modes
        d, D = np.zeros(M), np.zeros((M, M))
        _lib.check(_lib.load().ls_amd_corr_densities(self.h, dt, C.c_void_p(psi.data_ptr()), _f64p(d), _f64p(D), int(bool(symmetrize)),
                                                     _stream_ptr()))
        return d, D

    def hoppings(self, psi, symmetrize: bool = True):
        """-> G: numpy complex128 (M, M), G[i][j] = <B+_i B_j> (fermions: <c+_i c_j>), the densities on the diagonal"""
        psi, dt = self._psi("hoppings", psi)
        M = self.modes
        G = np.zeros((M, M), dtype=np.complex128)
        _lib.check(_lib.load().ls_amd_corr_hoppings(self.h, dt, C.c_void_p(psi.data_ptr()), _f64p(G.view(np.float64)), int(bool(symmetrize)),
                                                    _stream_ptr()))
        return G


def _normalised(psi):
    import torch

    nrm = float(torch.linalg.vector_norm(psi)) if isinstance(psi, torch.Tensor) and psi.numel() else 0.0
    return psi / nrm if nrm > 0.0 else psi


def _both(basis, reps, psi):
    pl = CorrelationPlan(basis, reps)
    try:
        psi = _normalised(psi)
        d, D = pl.densities(psi)
        return d, D, pl.hoppings(psi)
    finally:
        pl.destroy()


def spin_correlations(basis, reps, psi):
    """-> SpinCorrelations(z, zz, pm, ss) of the normalised psi on a spin-1/2 basis: z[i] = <sigma^z_i>, zz[i][j] = <sigma^z_i sigma^z_j>,
    pm[i][j] = <sigma^+_i sigma^-_j>, ss[i][j] = <S_i.S_j> = zz / 4 + (pm_ij + pm_ji) / 2 off the diagonal and 3 / 4 on it.
    Bit convention (config.py): bit 1 is spin down, so sigma^+ CLEARS a bit -- pm[i][j] = G[j][i] of CorrelationPlan.hoppings for
    i != j, and pm[i][i] = 1 - d[i]."""
    if basis.particleType() != 0:
        raise LsAmdError("spin_correlations: a fermionic basis has densities and a one-body density matrix: use fermion_correlations")
    d, D, G = _both(basis, reps, psi)
    z = 1.0 - 2.0 * d
    zz = 1.0 - 2.0 * d[:, None] - 2.0 * d[None, :] + 4.0 * D
    pm = G.T.copy()
    np.fill_diagonal(pm, 1.0 - d)
    ss = 0.25 * zz + 0.5 * (pm + pm.T)
    np.fill_diagonal(ss, 0.75)
    return SpinCorrelations(z, zz, pm, ss)


def fermion_correlations(basis, reps, psi):
    """-> FermionCorrelations(n, nn, one_body, double_occupancy) of the normalised psi on a fermionic basis, over its modes (spinful:
    mode (i, up) = i, mode (i, down) = i + L): n[i] = <n_i>, nn[i][j] = <n_i n_j>, one_body[i][j] = <c+_i c_j>;
    double_occupancy[i] = nn[i][i + L] on spinful bases, None on spinless ones."""
    if basis.particleType() == 0:
        raise LsAmdError("fermion_correlations: a spin-1/2 basis has sigma^z sigma^z, sigma^+ sigma^- and S.S: use spin_correlations")
    d, D, G = _both(basis, reps, psi)
    L = int(basis.numberSites())
    docc = np.array([D[i, i + L] for i in range(L)]) if len(d) == 2 * L else None
    return FermionCorrelations(d, D, G, docc)


def structure_factor(C_ij, positions, momenta):
    """the static structure factor N^-1 sum_ij e^{i q.(r_i - r_j)} C_ij of an (N, N) correlation matrix: positions (N,) or (N, dim),
    momenta (K,) or (K, dim) -> (K,) complex128 (real for a Hermitian C).  A host Fourier sum."""
    C_ij = np.asarray(C_ij)
    r = np.asarray(positions, dtype=np.float64)
    q = np.asarray(momenta, dtype=np.float64)
    r = r.reshape(len(r), -1)
    q = q.reshape(-1, r.shape[1]) if q.ndim else q.reshape(1, 1)
    if C_ij.shape != (len(r), len(r)):
        raise ValueError(f"structure_factor: a {C_ij.shape} matrix and {len(r)} positions")
    phase = np.exp(1j * (q @ r.T))  # (K, N)
    return np.einsum("ki,ij,kj->k", phase, C_ij, phase.conj()) / len(r)


def correlations(config, state=None, dtype=None, eps: float = 1e-10):
    """the correlations of a config (dict or YAML path): SpinCorrelations or FermionCorrelations by its particle type.  state None:
    its ground state (thick-restart Lanczos to eps, as entanglement_entropy(config, ...)); else a vector on enumerateStates(basis, 1)."""
    import torch

    from . import api
    from .diagonalize import LocalOperator, lanczos_smallest

    load = api.loadConfigFromYaml if isinstance(config, str) else api.loadConfigFromDict
    basis, h = load(config, hamiltonian=True)
    reps, _ = api.enumerateStates(basis, 1)
    if state is None:
        if dtype is None:
            dtype = torch.complex128 if _complex_characters(basis) or not h.isReal else torch.float64
        state = lanczos_smallest(LocalOperator(h, reps, dtype), num_evals=1, eps=eps).eigenvectors[0]
    if basis.particleType() == 0:
        return spin_correlations(basis, reps[0], state)
    return fermion_correlations(basis, reps[0], state)
