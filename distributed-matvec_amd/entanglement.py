"""Sector-state expansion and the entanglement of bipartitions (include/ls_amd.h: ls_amd_expand; csrc/k_expand.hip).

A state psi on the representatives of a symmetry sector -- an eigenvector of diagonalize(), a psi of kpm.spectral_function -- is
expanded to its amplitudes on product states |a>_A |b>_B: with the basis vectors P|r> / |P|r>| of the sector and
state_info(s) = (rep, character, norm),
    <s|psi> = conj(character(s)) norm(rep) psi[index(rep)]
The kernel k_expand_push scatters psi over the orbits of the representatives straight into the matrix M[a, b] = <a, b|psi> of the
bipartition, block by block in the particle number n_A of the subsystem A (a set of sites; B is the rest).  a holds the bits of a
state on the sites of A, compacted in ascending site order, b those on B.  On a fixed-weight basis block n_A has
C(|A|, n_A) x C(|B|, w - n_A) elements, row-major, row = combinadic rank of a, column = that of b (ascending integer order on both
sides); empty blocks are omitted and the blocks lie one after another in ONE buffer, ordered by n_A.  Without a fixed weight there
is a single 2^|A| x 2^|B| block (its n_A reads -1).  rho_A = M M+; its eigenvalues are the entanglement spectrum.  A = every site
is the full-basis vector: unproject().

Spin-1/2 bases, ONE partition: the whole sector is on this device.  Fermionic bases are refused (their partial trace needs
mode-ordering signs).  The scatter is HIP; the Gram products are torch.matmul on the device, the eigenvalues of the Gram blocks
torch.linalg.eigvalsh on the device (EIGVALSH_ON_DEVICE)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import LsAmdError

__all__ = ["SectorExpansion", "unproject", "reduced_density_matrix", "entanglement_spectrum", "entanglement_entropy"]

# where the eigenvalues of the Gram blocks are computed: torch.linalg.eigvalsh on the device; False copies the blocks to the host
# and calls numpy.linalg.eigvalsh
EIGVALSH_ON_DEVICE = True
DEFAULT_MAX_BYTES = 8 << 30


def _stream_ptr():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _subsystem_mask(basis, sites):
    L = basis.numberBits() if hasattr(basis, "numberBits") else int(basis.numberSites())
    if sites is None:
        return (1 << L) - 1, L
    sites = [s for s in sites]
    mask = 0
    for s in sites:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)):
            raise LsAmdError(f"SectorExpansion: sites must be integers, got {s!r}")
        s = int(s)
        if not 0 <= s < L:
            raise LsAmdError(f"SectorExpansion: site {s} is outside the {L} sites of the basis")
        if mask >> s & 1:
            raise LsAmdError(f"SectorExpansion: site {s} is listed twice")
        mask |= 1 << s
    return mask, L


def _complex_characters(basis):
    L = _lib.load()
    re, im = C.c_double(), C.c_double()
    for g in range(int(L.ls_amd_basis_group_order(basis.payload))):
        L.ls_amd_basis_group_character(basis.payload, g, C.byref(re), C.byref(im))
        if im.value != 0.0 or abs(re.value) != 1.0:
            return True
    return False


class SectorExpansion:
    """ls_amd_expand: the plan of expanding vectors on `reps` (the ascending representatives of `basis`, a 1-D int64 device tensor,
    one partition) into the blocks of the bipartition A = `sites` (None: every site -- the full-basis vector) | B = the rest.
    .blocks = [(n_a, rows, cols)] in buffer order; .total = elements of the buffer."""

    def __init__(self, basis, reps, sites=None):
        import torch

        L = _lib.load()
        self.mask, self.number_sites = _subsystem_mask(basis, sites)
        # the block table, host only: fermionic bases and bad masks are refused here, before a device is needed
        cap = 65
        na, rows, cols, offs, total = (C.c_int * cap)(), (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int64 * cap)(), C.c_int64()
        nb = L.ls_amd_test_expand_layout(basis.payload, C.c_uint64(self.mask), cap, na, rows, cols, offs, C.byref(total))
        if nb < 0:
            _lib.check(-1)
        self.blocks = [(int(na[i]), int(rows[i]), int(cols[i])) for i in range(nb)]
        self.offsets = [int(offs[i]) for i in range(nb)]
        self.total = int(total.value)
        if isinstance(reps, (list, tuple)):
            if len(reps) != 1:
                raise LsAmdError(f"SectorExpansion: one partition (the whole sector on this device), got {len(reps)} blocks of representatives")
            reps = reps[0]
        if not isinstance(reps, torch.Tensor) or reps.dim() != 1 or reps.dtype != torch.int64 or not reps.is_contiguous():
            raise LsAmdError("SectorExpansion: reps must be a contiguous 1-D int64 device tensor (one partition)")
        self.basis, self.reps = basis, reps  # borrowed by the plan: keep alive
        self.complex_characters = _complex_characters(basis)
        self.h = None

    def _plan(self):
        if self.h is None:
            _lib.require_device()
            if self.reps.device.type != "cuda":
                raise LsAmdError("SectorExpansion: reps must be a device tensor")
            h = C.c_void_p()
            _lib.check(_lib.load().ls_amd_expand_create(C.byref(h), self.basis.payload, C.c_void_p(self.reps.data_ptr()), self.reps.numel(),
                                                        C.c_uint64(self.mask), _stream_ptr()))
            self.h = h
        return self.h

    def destroy(self):
        if getattr(self, "h", None):
            _lib.load().ls_amd_expand_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    @property
    def kernel(self): return _lib.load().ls_amd_expand_kernel_name(self._plan()).decode()

    def _selection(self, blocks):
        nb = len(self.blocks)
        if blocks is None:
            return 0, nb
        if isinstance(blocks, (int, np.integer)) and not isinstance(blocks, bool):
            blocks = [int(blocks)]
        blocks = [int(b) for b in blocks]
        if not blocks or blocks != list(range(blocks[0], blocks[0] + len(blocks))) or blocks[0] < 0 or blocks[-1] >= nb:
            raise LsAmdError(f"SectorExpansion.expand: blocks = {blocks} must be a run of consecutive block indices inside [0, {nb})")
        return blocks[0], len(blocks)

    def expand(self, psi, blocks=None, out=None, max_bytes=DEFAULT_MAX_BYTES, check: bool = True):
        """-> [M_i]: 2-D views, one per block of .blocks, of ONE buffer of .total elements.  psi: a device vector on the
        representatives, float64 or complex128 (float64 is promoted to complex128 when the characters are complex).  blocks: a run of
        consecutive block indices (or one index) -- only those are cleared and written, the views of the others show whatever the
        buffer held; out: a 1-D buffer of .total elements to write into.  max_bytes guards the allocation of the selected blocks."""
        import torch

        n = int(self.reps.numel())
        if not isinstance(psi, torch.Tensor):
            raise LsAmdError("SectorExpansion.expand: psi must be a device tensor")
        if psi.dim() != 1:
            raise LsAmdError(f"SectorExpansion.expand: psi {tuple(psi.shape)} must be ONE vector of {n} elements; expand the columns of an "
                             "(n, K) block one by one")
        if psi.numel() != n:
            raise LsAmdError(f"SectorExpansion.expand: psi has {psi.numel()} elements, the basis has {n} representatives")
        if psi.dtype not in (torch.float64, torch.complex128):
            raise LsAmdError(f"SectorExpansion.expand: psi is {psi.dtype}, neither float64 nor complex128")
        first, count = self._selection(blocks)
        if psi.device.type != "cuda":
            raise LsAmdError("SectorExpansion.expand: psi must be a device tensor (there is no CPU path)")
        if psi.dtype == torch.float64 and self.complex_characters:
            psi = psi.to(torch.complex128)
        dtype = psi.dtype
        elt = 16 if dtype == torch.complex128 else 8
        selected = sum(r * c for _, r, c in self.blocks[first:first + count]) * elt
        if max_bytes is not None and selected > max_bytes:
            raise LsAmdError(f"SectorExpansion.expand: the selected blocks take {selected} bytes ({selected / 2**30:.2f} GiB), more than "
                             f"max_bytes = {max_bytes}; pass blocks= to expand them one at a time (or raise max_bytes)")
        if out is not None:
            if (not isinstance(out, torch.Tensor) or out.dim() != 1 or out.numel() != self.total or out.dtype != dtype
                    or out.device.type != "cuda" or not out.is_contiguous()):
                raise LsAmdError(f"SectorExpansion.expand: out must be a contiguous 1-D {dtype} device tensor of {self.total} elements")
        h = self._plan()
        psi = psi if psi.is_contiguous() else psi.contiguous()
        if out is None:
            if count == len(self.blocks):
                out = torch.empty(self.total, dtype=dtype, device=psi.device)
            else:
                # the selected blocks alone are backed by memory: the buffer starts at the first of them (earlier offsets are not touched)
                lo = self.offsets[first]
                hi = self.offsets[first + count - 1] + self.blocks[first + count - 1][1] * self.blocks[first + count - 1][2]
                part = torch.empty(hi - lo, dtype=dtype, device=psi.device)
                base = part.data_ptr() - lo * elt
                _lib.check(_lib.load().ls_amd_expand_apply(h, 1 if elt == 16 else 0, C.c_void_p(psi.data_ptr()), C.c_void_p(base), first, count,
                                                           _stream_ptr()))
                if check:
                    self.check()
                views = [None] * len(self.blocks)
                for i in range(first, first + count):
                    _, r, c = self.blocks[i]
                    views[i] = part[self.offsets[i] - lo:self.offsets[i] - lo + r * c].view(r, c)
                return views
        _lib.check(_lib.load().ls_amd_expand_apply(h, 1 if elt == 16 else 0, C.c_void_p(psi.data_ptr()), C.c_void_p(out.data_ptr()), first, count,
                                                   _stream_ptr()))
        if check:
            self.check()
        return [out[o:o + r * c].view(r, c) for o, (_, r, c) in zip(self.offsets, self.blocks)]

    def check(self):
        _lib.check(_lib.load().ls_amd_expand_check(self._plan(), _stream_ptr()))


def unproject(basis, reps, psi):
    """the 1-D vector of psi over the ascending states of the same basis WITHOUT symmetries (A = every site): the order
    enumerateStates gives for the plain config"""
    ex = SectorExpansion(basis, reps, None)
    try:
        (m,) = ex.expand(psi)
    finally:
        ex.destroy()
    return m.reshape(-1)


def _gram(M, smaller):
    """rho_A = M M+; with `smaller` and fewer columns than rows, rho_B = M^T M^* instead (the same non-zero spectrum)"""
    import torch

    if smaller and M.shape[1] < M.shape[0]:
        return torch.matmul(M.conj().transpose(0, 1), M).transpose(0, 1).contiguous()
    return torch.matmul(M, M.conj().transpose(0, 1))


def reduced_density_matrix(basis, reps, psi, sites, smaller: bool = False, max_bytes=DEFAULT_MAX_BYTES):
    """-> [(n_a, rho block)]: the blocks of rho_A = Tr_B |psi><psi| (block n_a: C(|A|, n_a) square, rows / columns in ascending order
    of a).  smaller=True returns, for every block with fewer columns than rows, the block of rho_B = M^T M^* instead -- M+ M
    transposed back, the same non-zero eigenvalues on the smaller side.  psi is taken as it is (normalise it first)."""
    ex = SectorExpansion(basis, reps, sites)
    try:
        out = []
        for i, (na, _r, _c) in enumerate(ex.blocks):  # one block at a time: the buffer of a block is released before the next
            M = ex.expand(psi, blocks=[i], max_bytes=max_bytes)[i]
            out.append((na, _gram(M, smaller)))
            del M
    finally:
        ex.destroy()
    return out


def _eigvalsh(rho):
    """ascending eigenvalues (numpy float64) of a Hermitian device block"""
    import torch

    if EIGVALSH_ON_DEVICE:
        return torch.linalg.eigvalsh(rho).cpu().numpy()
    return np.linalg.eigvalsh(rho.cpu().numpy())


def entanglement_spectrum(basis, reps, psi, sites, max_bytes=DEFAULT_MAX_BYTES):
    """-> (eigenvalues, n_a): the eigenvalues of rho_A over all blocks in descending order (numpy float64) and the n_a of the block
    each belongs to.  Computed on the smaller side of every block, so min(rows, cols) values per block (the others are 0).
    Eigenvalues in [-1e-13 Tr, 0) are rounding and clamped to 0; anything more negative raises."""
    blocks = reduced_density_matrix(basis, reps, psi, sites, smaller=True, max_bytes=max_bytes)
    vals, nas = [], []
    for na, rho in blocks:
        w = _eigvalsh(rho)
        vals.append(np.asarray(w, dtype=np.float64))
        nas.append(np.full(len(w), na, dtype=np.int64))
    vals = np.concatenate(vals) if vals else np.zeros(0)
    nas = np.concatenate(nas) if nas else np.zeros(0, dtype=np.int64)
    trace = float(vals.sum())
    if len(vals) and vals.min() < -1e-13 * abs(trace):
        raise LsAmdError(f"entanglement_spectrum: eigenvalue {vals.min():.3e} of a density matrix of trace {trace:.6g} is negative beyond rounding")
    vals = np.where(vals < 0.0, 0.0, vals)
    order = np.argsort(-vals, kind="stable")
    return vals[order], nas[order]


def _entropy_of(vals, renyi):
    p = vals[vals > 0.0]
    if renyi == 1.0:
        return float(-(p * np.log(p)).sum())
    if renyi <= 0.0 or math.isinf(renyi):
        raise ValueError(f"renyi = {renyi}: a positive finite order (1 = von Neumann)")
    return float(np.log((p ** renyi).sum()) / (1.0 - renyi))


def entanglement_entropy(first, *args, renyi: float = 1.0, **kwargs):
    """Entropy of the bipartition A = sites | rest: von Neumann for renyi = 1, else the Renyi entropy ln(Tr rho^q) / (1 - q).
        entanglement_entropy(basis, reps, psi, sites, renyi=1.0)          a state on the representatives of an api.Basis
        entanglement_entropy(config, sites, state=None, renyi=1.0, ...)   a config (dict or YAML path); state None: its ground state
                                                                         (thick-restart Lanczos to eps, as kpm.spectral_function)
    psi is normalised first."""
    from . import api

    if isinstance(first, api.Basis):
        return _entropy_state(first, *args, renyi=renyi, **kwargs)
    return _entropy_config(first, *args, renyi=renyi, **kwargs)


def _entropy_state(basis, reps, psi, sites, renyi=1.0, max_bytes=DEFAULT_MAX_BYTES):
    import torch

    nrm = float(torch.linalg.vector_norm(psi)) if isinstance(psi, torch.Tensor) and psi.numel() else 0.0
    if nrm > 0.0:
        psi = psi / nrm
    vals, _ = entanglement_spectrum(basis, reps, psi, sites, max_bytes=max_bytes)
    return _entropy_of(vals, float(renyi))


def _entropy_config(config, sites, state=None, renyi=1.0, dtype=None, eps: float = 1e-10, max_bytes=DEFAULT_MAX_BYTES):
    import torch

    from . import api
    from .diagonalize import LocalOperator, lanczos_smallest

    load = api.loadConfigFromYaml if isinstance(config, str) else api.loadConfigFromDict
    basis, h = load(config, hamiltonian=True)
    SectorExpansion(basis, torch.zeros(0, dtype=torch.int64), sites)  # bad sites and fermionic bases are refused before anything is enumerated
    reps, _ = api.enumerateStates(basis, 1)
    if state is None:
        if dtype is None:
            dtype = torch.complex128 if _complex_characters(basis) or not h.isReal else torch.float64
        state = lanczos_smallest(LocalOperator(h, reps, dtype), num_evals=1, eps=eps).eigenvectors[0]
    return _entropy_state(basis, reps[0], state, sites, renyi=renyi, max_bytes=max_bytes)
