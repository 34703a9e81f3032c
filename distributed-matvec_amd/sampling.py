"""Amplitudes of sector states on product states, and Born sampling (include/ls_amd.h: ls_amd_amp; csrc/k_amplitude_t.hpp).

A sector state lives on the orbit representatives of its basis.  With state_info(s) = (rep, character, norm) of a word s of the same
basis WITHOUT symmetries,
    <s|psi> = conj(character(s)) norm(rep) psi[index(rep)]
(the character carries the orbit sign on a projected fermionic basis; psi[index(s)] on an unprojected one) -- the entry unproject /
fermion_unproject write for s, here for a BATCH of words in any order, duplicates allowed, without the full-basis vector: the value of
the wavefunction on the configurations a Monte-Carlo sampler, a neural-network ansatz or an experiment's snapshots hand over.  A word
that is no state of the basis without symmetries (a bit above the sites, another Hamming weight or particle number, another
(N_up, N_down) split) and a word on an orbit of zero norm read 0: no error.  A representative inside the conserved numbers that is
missing from reps is an error ("not in the basis"): the array does not belong to the basis.

The inverse: sample() draws words from |<s|psi>|^2 EXACTLY.  sum_{s in orbit(r)} |<s|psi>|^2 = |psi_r|^2, and a uniform element of the
effective group (the permutation elements, each with and without the global inversion on a spin basis that has one; the up <-> down
flip of a spinful basis is among its elements) maps r uniformly onto its orbit: so a row drawn with probability |psi_r|^2 / |psi|^2
(inverse CDF: cumsum in float64 and searchsorted; torch.multinomial stops at 2^24 categories) and an element drawn uniformly give a
word with probability |<s|psi>|^2 / |psi|^2.  k_orbit_image applies the elements.

ONE partition: the whole sector is on this device."""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import LsAmdError
from .entanglement import _complex_characters, _stream_ptr

__all__ = ["SectorAmplitudes", "amplitudes", "sample_states", "snapshots"]

MAX_COLUMNS = 64


def _one_partition(who, reps):
    import torch

    if isinstance(reps, (list, tuple)):
        if len(reps) != 1:
            raise LsAmdError(f"{who}: one partition (the whole sector on this device), got {len(reps)} blocks of representatives")
        reps = reps[0]
    if not isinstance(reps, torch.Tensor) or reps.dim() != 1 or reps.dtype != torch.int64 or not reps.is_contiguous():
        raise LsAmdError(f"{who}: reps must be a contiguous 1-D int64 device tensor (one partition)")
    return reps


def _words(who, checks):
    """contiguous 1-D device tensors for (name, tensor, dtype) triples: shapes and dtypes of all of them first, then that they are on
    the device; neither refusal needs one"""
    import torch

    for name, t, dtype in checks:
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != dtype:
            raise LsAmdError(f"{who}: {name} must be a 1-D {str(dtype).replace('torch.', '')} device tensor")
    for name, t, _ in checks:
        if t.device.type != "cuda":
            raise LsAmdError(f"{who}: {name} must be a device tensor (there is no CPU path)")
    return [t.contiguous() for _, t, _ in checks]


class SectorAmplitudes:
    """ls_amd_amp: amplitudes, state_info, orbit images and Born samples of vectors on `reps` (the ascending representatives of `basis`,
    a 1-D int64 device tensor, one partition).  The plan is built at the first call that needs the device."""

    def __init__(self, basis, reps):
        self.basis, self.reps = basis, _one_partition("SectorAmplitudes", reps)  # borrowed by the plan: keep alive
        self.complex_characters = _complex_characters(basis)
        self.h = None

    def _plan(self):
        if self.h is None:
            _lib.require_device()
            if self.reps.device.type != "cuda":
                raise LsAmdError("SectorAmplitudes: reps must be a device tensor (there is no CPU path)")
            h = C.c_void_p()
            _lib.check(_lib.load().ls_amd_amp_create(C.byref(h), self.basis.payload, C.c_void_p(self.reps.data_ptr()), self.reps.numel(),
                                                     _stream_ptr()))
            self.h = h
        return self.h

    def destroy(self):
        if getattr(self, "h", None):
            _lib.load().ls_amd_amp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    @property
    def kernel(self): return _lib.load().ls_amd_amp_kernel_name(self._plan()).decode()

    @property
    def num_elements(self):
        """the order of the effective group: the elements sample() and orbit_states() number (inversion / flip included)"""
        return int(_lib.load().ls_amd_amp_num_elements(self._plan()))

    def check(self):
        _lib.check(_lib.load().ls_amd_amp_check(self._plan(), _stream_ptr()))

    def _psi(self, who, psi):
        import torch

        n = int(self.reps.numel())
        if not isinstance(psi, torch.Tensor):
            raise LsAmdError(f"{who}: psi must be a device tensor")
        if psi.dim() not in (1, 2):
            raise LsAmdError(f"{who}: psi {tuple(psi.shape)} must be a vector of {n} elements or an ({n}, K) block of columns")
        if psi.shape[0] != n:
            raise LsAmdError(f"{who}: psi has {psi.shape[0]} rows, the sector has {n} representatives")
        K = 1 if psi.dim() == 1 else int(psi.shape[1])
        if not 1 <= K <= MAX_COLUMNS:
            raise LsAmdError(f"{who}: K = {K} columns, outside [1, {MAX_COLUMNS}]; take wider blocks in slices of columns")
        if psi.dtype not in (torch.float64, torch.complex128):
            raise LsAmdError(f"{who}: psi is {psi.dtype}, neither float64 nor complex128")
        if psi.device.type != "cuda":
            raise LsAmdError(f"{who}: psi must be a device tensor (there is no CPU path)")
        return K

    def amplitudes(self, states, psi, out=None, check: bool = True):
        """-> <s|psi> (B,) for psi (n,), or (B, K) for psi (n, K), 1 <= K <= 64, for the B words `states` (a 1-D int64 device tensor,
        any order, duplicates allowed).  psi: float64 or complex128, any strides ((n, K) contiguous -- the columns interleaved -- is
        the fast layout); float64 is promoted to complex128 when the characters are complex.  out: a device tensor of exactly the
        result's shape and dtype (any strides without overlap) to write into; elements of its storage outside it are not touched."""
        import torch

        who = "SectorAmplitudes.amplitudes"
        K = self._psi(who, psi)
        states, = _words(who, [("states", states, torch.int64)])
        B = int(states.numel())
        if psi.dtype == torch.float64 and self.complex_characters:
            psi = psi.to(torch.complex128)
        dtype = psi.dtype
        shape = (B,) if psi.dim() == 1 else (B, K)
        if out is not None:
            if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != dtype or out.device.type != "cuda"
                    or any(s <= 0 for s, m in zip(out.stride(), out.shape) if m > 1)):
                raise LsAmdError(f"{who}: out must be a {dtype} device tensor of shape {shape} without overlapping elements")
        else:
            out = torch.empty(shape, dtype=dtype, device=psi.device)
        h = self._plan()
        ps, os_ = psi.stride(), out.stride()
        _lib.check(_lib.load().ls_amd_amp_amplitudes(h, 1 if dtype == torch.complex128 else 0, K, B, C.c_void_p(states.data_ptr()),
                                                     C.c_void_p(psi.data_ptr()), ps[0], ps[1] if psi.dim() == 2 else 0,
                                                     C.c_void_p(out.data_ptr()), os_[0], os_[1] if out.dim() == 2 else 0, _stream_ptr()))
        if check:
            self.check()
        return out

    def state_info(self, states, check: bool = True):
        """-> (reps, index, characters, norms) device tensors for the words `states`: the representative (int64 words), its row in
        reps (-1 for a word outside the basis or on a zero-norm orbit), the character (complex128; with the orbit sign on projected
        fermionic bases) and the norm -- ls_hs_state_info + ls_hs_state_index on device pointers.  A word outside the basis without
        symmetries reports itself with character 0 and norm 0."""
        import torch

        who = "SectorAmplitudes.state_info"
        states, = _words(who, [("states", states, torch.int64)])
        B = int(states.numel())
        rep = torch.empty(B, dtype=torch.int64, device=states.device)
        idx = torch.empty(B, dtype=torch.int64, device=states.device)
        ch = torch.empty(B, dtype=torch.complex128, device=states.device)
        nrm = torch.empty(B, dtype=torch.float64, device=states.device)
        _lib.check(_lib.load().ls_amd_amp_state_info(self._plan(), B, C.c_void_p(states.data_ptr()), C.c_void_p(rep.data_ptr()),
                                                     C.c_void_p(idx.data_ptr()), C.c_void_p(ch.data_ptr()), C.c_void_p(nrm.data_ptr()),
                                                     _stream_ptr()))
        if check:
            self.check()
        return rep, idx, ch, nrm

    def orbit_states(self, rows, elements, check: bool = True):
        """-> g_e reps[row] (int64 words) for every pair (rows[j], elements[j]): rows 1-D int64, elements 1-D int32 in
        [0, num_elements), both on the device"""
        import torch

        who = "SectorAmplitudes.orbit_states"
        rows, elements = _words(who, [("rows", rows, torch.int64), ("elements", elements, torch.int32)])
        if rows.numel() != elements.numel():
            raise LsAmdError(f"{who}: {rows.numel()} rows and {elements.numel()} elements")
        out = torch.empty(rows.numel(), dtype=torch.int64, device=rows.device)
        _lib.check(_lib.load().ls_amd_amp_orbit_states(self._plan(), rows.numel(), C.c_void_p(rows.data_ptr()), C.c_void_p(elements.data_ptr()),
                                                       C.c_void_p(out.data_ptr()), _stream_ptr()))
        if check:
            self.check()
        return out

    def sample(self, psi, num_samples, seed: int = 0, return_rows: bool = False):
        """-> num_samples words (1-D int64 device tensor) drawn independently from |<s|psi>|^2 / |psi|^2 (psi a vector on reps; it need
        not be normalised); with return_rows also the row of every word's representative.  The same seed gives the same tensor."""
        import torch

        who = "SectorAmplitudes.sample"
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 0:
            raise LsAmdError(f"{who}: num_samples must be a non-negative int, got {num_samples!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise LsAmdError(f"{who}: seed must be an int, got {seed!r}")
        if isinstance(psi, torch.Tensor) and psi.dim() != 1:
            raise LsAmdError(f"{who}: psi {tuple(psi.shape)} must be one vector on the representatives")
        self._psi(who, psi)
        rows, gen = self._rows(who, psi, num_samples, seed)
        elements = torch.randint(self.num_elements, (num_samples,), generator=gen, device=psi.device, dtype=torch.int32)
        words = self.orbit_states(rows, elements)
        return (words, rows) if return_rows else words

    def _rows(self, who, psi, num_samples, seed):
        """(rows drawn by the inverse CDF of |psi|^2, the seeded device generator)"""
        import torch

        p = (psi.real * psi.real + psi.imag * psi.imag) if psi.is_complex() else psi * psi
        cdf = torch.cumsum(p.to(torch.float64), 0)
        total = float(cdf[-1]) if cdf.numel() else 0.0
        if not (total == total and total != float("inf")) or not bool(torch.isfinite(p).all()):
            raise LsAmdError(f"{who}: psi is not finite (NaN or infinity among its elements)")
        if not total > 0.0:
            raise LsAmdError(f"{who}: psi is zero: there is no distribution to sample")
        gen = torch.Generator(device=psi.device)
        gen.manual_seed(seed)
        u = torch.rand(num_samples, generator=gen, device=psi.device, dtype=torch.float64) * total
        rows = torch.searchsorted(cdf, u, right=True)
        # u < total up to the rounding of the product: a draw that lands on the total belongs to the last row of non-zero weight
        last = int(torch.nonzero(p > 0)[-1])
        return torch.clamp(rows, max=last), gen


def amplitudes(basis, reps, psi, states):
    """one-shot SectorAmplitudes(basis, reps).amplitudes(states, psi)"""
    sa = SectorAmplitudes(basis, reps)
    try:
        return sa.amplitudes(states, psi)
    finally:
        sa.destroy()


def sample_states(basis, reps, psi, num_samples, seed: int = 0):
    """one-shot SectorAmplitudes(basis, reps).sample(psi, num_samples, seed)"""
    sa = SectorAmplitudes(basis, reps)
    try:
        return sa.sample(psi, num_samples, seed)
    finally:
        sa.destroy()


def snapshots(config, num_samples, seed: int = 0, state=None, dtype=None, eps: float = 1e-10):
    """projective-measurement snapshots of a config (dict or YAML path): -> (words, amplitudes), num_samples words drawn from
    |<s|psi>|^2 and <s|psi> of the normalised state for each of them.  state None: the ground state (thick-restart Lanczos to eps,
    as correlations.correlations(config)); else a vector on enumerateStates(basis, 1)."""
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
    nrm = float(torch.linalg.vector_norm(state)) if isinstance(state, torch.Tensor) and state.numel() else 0.0
    if nrm > 0.0:
        state = state / nrm
    sa = SectorAmplitudes(basis, reps[0])
    try:
        words = sa.sample(state, num_samples, seed)
        return words, sa.amplitudes(words, state)
    finally:
        sa.destroy()
