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

ONE partition: the whole sector is on this device.  SectorExpansion / unproject take spin-1/2 bases and refuse fermionic ones (their
partial trace needs mode-ordering signs); FermionSectorExpansion / fermion_unproject (ls_amd_fermi_expand_create, kernel
k_expand_push_fermi, csrc/k_expand_fermi.hip) carry those signs: the image s = g r receives conj(chi(g)) sign(g, r) n(r) psi[r] with
U_g|r> = sign(g, r)|g r>, and M[a, b] = sigma(s) <s|psi> with |s> = sigma(s) |a>_A |b>_B, the modes of A carried in front of those of B
in the Fock ordering c+_{k1} ... c+_{kN}|0>, k1 < ... < kN.  rho_A = M M+ is then the fermionic reduced density matrix: Tr(rho_A O_A) =
<psi|O_A|psi> for every operator on A written by Jordan-Wigner over A's own modes.  The subsystem of a fermionic basis is given by
lattice `sites` (on a spinful basis a site brings both of its modes, i and i + L) or by `modes` directly.  The spinful (N, N_up) basis
has one block per (n_up, n_dn) of the subsystem, ordered lexicographically: rows C(|A_up|, n_up) C(|A_dn|, n_dn), columns
C(L - |A_up|, N_up - n_up) C(L - |A_dn|, N_dn - n_dn), rows and columns in ascending order of a and b (the up modes are the low ones);
every other fermionic basis has the layout above over its modes.  reduced_density_matrix, entanglement_spectrum and
entanglement_entropy dispatch on the particle type.  The scatter is HIP; the Gram products are torch.matmul on the device, the
eigenvalues of the Gram blocks torch.linalg.eigvalsh on the device (EIGVALSH_ON_DEVICE)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import LsAmdError

__all__ = ["SectorExpansion", "unproject", "FermionSectorExpansion", "fermion_unproject", "reduced_density_matrix", "entanglement_spectrum",
           "entanglement_entropy"]

# where the eigenvalues of the Gram blocks are computed: torch.linalg.eigvalsh on the device; False copies the blocks to the host
# and calls numpy.linalg.eigvalsh
EIGVALSH_ON_DEVICE = True
DEFAULT_MAX_BYTES = 8 << 30


def _stream_ptr():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bit_mask(who, what, items, L):
    """the mask of the distinct integers `items` in [0, L) (`what`: "site" or "mode", for the messages)"""
    mask = 0
    for s in [s for s in items]:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)):
            raise LsAmdError(f"{who}: {what}s must be integers, got {s!r}")
        s = int(s)
        if not 0 <= s < L:
            raise LsAmdError(f"{who}: {what} {s} is outside the {L} {what}s of the basis")
        if mask >> s & 1:
            raise LsAmdError(f"{who}: {what} {s} is listed twice")
        mask |= 1 << s
    return mask


def _subsystem_mask(basis, sites):
    L = basis.numberBits() if hasattr(basis, "numberBits") else int(basis.numberSites())
    if sites is None:
        return (1 << L) - 1, L
    return _bit_mask("SectorExpansion", "site", sites, L), L


def _mode_mask(basis, sites, modes):
    """the modes of the subsystem of a fermionic basis: `sites` (a spinful site brings its modes i and i + L) or `modes`"""
    who = "FermionSectorExpansion"
    M, L = basis.numberBits(), int(basis.numberSites())
    if sites is not None and modes is not None:
        raise LsAmdError(f"{who}: give the subsystem by sites or by modes, not both")
    if modes is not None:
        return _bit_mask(who, "mode", modes, M), M
    if sites is None:
        return (1 << M) - 1, M
    mask = _bit_mask(who, "site", sites, L)
    return (mask | mask << L if M == 2 * L else mask), M


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
        self.mask, self.number_sites = _subsystem_mask(basis, sites)
        self._setup(basis, reps)

    _create = "ls_amd_expand_create"

    def _layout(self, basis):
        """-> (.blocks, .offsets, .total): the block table, host only -- fermionic bases and bad masks are refused here, before a
        device is needed"""
        L = _lib.load()
        cap = 65
        na, rows, cols, offs, total = (C.c_int * cap)(), (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int64 * cap)(), C.c_int64()
        nb = L.ls_amd_test_expand_layout(basis.payload, C.c_uint64(self.mask), cap, na, rows, cols, offs, C.byref(total))
        if nb < 0:
            _lib.check(-1)
        return [(int(na[i]), int(rows[i]), int(cols[i])) for i in range(nb)], [int(offs[i]) for i in range(nb)], int(total.value)

    def _setup(self, basis, reps):
        import torch

        who = type(self).__name__
        self.blocks, self.offsets, self.total = self._layout(basis)
        if isinstance(reps, (list, tuple)):
            if len(reps) != 1:
                raise LsAmdError(f"{who}: one partition (the whole sector on this device), got {len(reps)} blocks of representatives")
            reps = reps[0]
        if not isinstance(reps, torch.Tensor) or reps.dim() != 1 or reps.dtype != torch.int64 or not reps.is_contiguous():
            raise LsAmdError(f"{who}: reps must be a contiguous 1-D int64 device tensor (one partition)")
        self.basis, self.reps = basis, reps  # borrowed by the plan: keep alive
        self.complex_characters = _complex_characters(basis)
        self.h = None

    def _plan(self):
        if self.h is None:
            _lib.require_device()
            if self.reps.device.type != "cuda":
                raise LsAmdError(f"{type(self).__name__}: reps must be a device tensor")
            h = C.c_void_p()
            _lib.check(getattr(_lib.load(), self._create)(C.byref(h), self.basis.payload, C.c_void_p(self.reps.data_ptr()), self.reps.numel(),
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
        nb, who = len(self.blocks), type(self).__name__
        if blocks is None:
            return 0, nb
        if isinstance(blocks, (int, np.integer)) and not isinstance(blocks, bool):
            blocks = [int(blocks)]
        blocks = [int(b) for b in blocks]
        if not blocks or blocks != list(range(blocks[0], blocks[0] + len(blocks))) or blocks[0] < 0 or blocks[-1] >= nb:
            raise LsAmdError(f"{who}.expand: blocks = {blocks} must be a run of consecutive block indices inside [0, {nb})")
        return blocks[0], len(blocks)

    def expand(self, psi, blocks=None, out=None, max_bytes=DEFAULT_MAX_BYTES, check: bool = True):
        """-> [M_i]: 2-D views, one per block of .blocks, of ONE buffer of .total elements.  psi: a device vector on the
        representatives, float64 or complex128 (float64 is promoted to complex128 when the characters are complex).  blocks: a run of
        consecutive block indices (or one index) -- only those are cleared and written, the views of the others show whatever the
        buffer held; out: a 1-D buffer of .total elements to write into.  max_bytes guards the allocation of the selected blocks."""
        import torch

        who = type(self).__name__
        n = int(self.reps.numel())
        if not isinstance(psi, torch.Tensor):
            raise LsAmdError(f"{who}.expand: psi must be a device tensor")
        if psi.dim() != 1:
            raise LsAmdError(f"{who}.expand: psi {tuple(psi.shape)} must be ONE vector of {n} elements; expand the columns of an "
                             "(n, K) block one by one")
        if psi.numel() != n:
            raise LsAmdError(f"{who}.expand: psi has {psi.numel()} elements, the basis has {n} representatives")
        if psi.dtype not in (torch.float64, torch.complex128):
            raise LsAmdError(f"{who}.expand: psi is {psi.dtype}, neither float64 nor complex128")
        first, count = self._selection(blocks)
        if psi.device.type != "cuda":
            raise LsAmdError(f"{who}.expand: psi must be a device tensor (there is no CPU path)")
        if psi.dtype == torch.float64 and self.complex_characters:
            psi = psi.to(torch.complex128)
        dtype = psi.dtype
        elt = 16 if dtype == torch.complex128 else 8
        selected = sum(r * c for _, r, c in self.blocks[first:first + count]) * elt
        if max_bytes is not None and selected > max_bytes:
            raise LsAmdError(f"{who}.expand: the selected blocks take {selected} bytes ({selected / 2**30:.2f} GiB), more than "
                             f"max_bytes = {max_bytes}; pass blocks= to expand them one at a time (or raise max_bytes)")
        if out is not None:
            if (not isinstance(out, torch.Tensor) or out.dim() != 1 or out.numel() != self.total or out.dtype != dtype
                    or out.device.type != "cuda" or not out.is_contiguous()):
                raise LsAmdError(f"{who}.expand: out must be a contiguous 1-D {dtype} device tensor of {self.total} elements")
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


class FermionSectorExpansion(SectorExpansion):
    """ls_amd_fermi_expand_create: SectorExpansion for fermionic bases (kernel k_expand_push_fermi), with the orbit sign and the sign
    of the bipartition.  The subsystem A is `sites` (lattice sites; on a spinful basis each brings both of its modes, i and i + L; on a
    spinless basis sites are modes) or `modes` (bits of the state word, one species only for example); giving both is an error, giving
    neither means every mode.  .blocks = [(label, rows, cols)]: label = n_a on spinless layouts (spinless bases, spinful ones with
    number_up unset; -1 without a fixed number), (n_up, n_dn) on the spinful (N, N_up) basis.  Spin bases are refused by name."""

    _create = "ls_amd_fermi_expand_create"

    def __init__(self, basis, reps, sites=None, modes=None):
        if basis.particleType() == 0:
            raise LsAmdError("FermionSectorExpansion: a spin-1/2 basis has no mode-ordering signs: use SectorExpansion")
        self.mask, self.number_modes = _mode_mask(basis, sites, modes)
        self.number_sites = int(basis.numberSites())
        self._setup(basis, reps)

    def _layout(self, basis):
        L = _lib.load()
        cap = 33 * 33
        nu, nd = (C.c_int * cap)(), (C.c_int * cap)()
        rows, cols, offs, total = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int64 * cap)(), C.c_int64()
        nb = L.ls_amd_test_fermi_expand_layout(basis.payload, C.c_uint64(self.mask), cap, nu, nd, rows, cols, offs, C.byref(total))
        if nb < 0:
            _lib.check(-1)
        self.spinful_layout = nb > 0 and int(nd[0]) >= 0
        label = (lambda i: (int(nu[i]), int(nd[i]))) if self.spinful_layout else (lambda i: int(nu[i]))
        return [(label(i), int(rows[i]), int(cols[i])) for i in range(nb)], [int(offs[i]) for i in range(nb)], int(total.value)


def fermion_unproject(basis, reps, psi):
    """unproject for a fermionic basis (A = every mode, where the bipartition sign is +1): the 1-D vector of psi over the ascending
    states of the same basis WITHOUT symmetries -- the order enumerateStates gives for the plain config"""
    ex = FermionSectorExpansion(basis, reps)
    try:
        (m,) = ex.expand(psi)
    finally:
        ex.destroy()
    return m.reshape(-1)


def _expansion(basis, reps, sites, modes):
    """the expansion plan of the particle type"""
    if basis.particleType() != 0:
        return FermionSectorExpansion(basis, reps, sites, modes)
    if modes is not None:
        raise LsAmdError("modes= names the modes of a fermionic basis; the subsystem of a spin-1/2 basis is given by sites")
    return SectorExpansion(basis, reps, sites)


def _gram(M, smaller):
    """rho_A = M M+; with `smaller` and fewer columns than rows, rho_B = M^T M^* instead (the same non-zero spectrum)"""
    import torch

    if smaller and M.shape[1] < M.shape[0]:
        return torch.matmul(M.conj().transpose(0, 1), M).transpose(0, 1).contiguous()
    return torch.matmul(M, M.conj().transpose(0, 1))


def reduced_density_matrix(basis, reps, psi, sites=None, smaller: bool = False, max_bytes=DEFAULT_MAX_BYTES, modes=None):
    """-> [(n_a, rho block)]: the blocks of rho_A = Tr_B |psi><psi| (block n_a: C(|A|, n_a) square, rows / columns in ascending order
    of a).  smaller=True returns, for every block with fewer columns than rows, the block of rho_B = M^T M^* instead -- M+ M
    transposed back, the same non-zero eigenvalues on the smaller side.  psi is taken as it is (normalise it first).
    Fermionic bases: the subsystem is `sites` or `modes` (FermionSectorExpansion); the label of a block of the spinful (N, N_up)
    basis is (n_up, n_dn); rho_A is the fermionic reduced density matrix over A's own modes in ascending order."""
    ex = _expansion(basis, reps, sites, modes)
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


def entanglement_spectrum(basis, reps, psi, sites=None, max_bytes=DEFAULT_MAX_BYTES, modes=None):
    """-> (eigenvalues, n_a): the eigenvalues of rho_A over all blocks in descending order (numpy float64) and the n_a of the block
    each belongs to -- an array of shape (k, 2) of (n_up, n_dn) on the spinful (N, N_up) layout.  Computed on the smaller side of
    every block, so min(rows, cols) values per block (the others are 0).
    Eigenvalues in [-1e-13 Tr, 0) are rounding and clamped to 0; anything more negative raises."""
    blocks = reduced_density_matrix(basis, reps, psi, sites, smaller=True, max_bytes=max_bytes, modes=modes)
    pairs = basis.particleType() == 1 and basis.numberUp() != -1  # the spinful product layout
    vals, nas = [], []
    for na, rho in blocks:
        w = _eigvalsh(rho)
        vals.append(np.asarray(w, dtype=np.float64))
        nas.append(np.tile(np.asarray(na, dtype=np.int64), (len(w), 1)) if pairs else np.full(len(w), na, dtype=np.int64))
    vals = np.concatenate(vals) if vals else np.zeros(0)
    nas = np.concatenate(nas) if nas else np.zeros((0, 2) if pairs else 0, dtype=np.int64)
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
    psi is normalised first.  Fermionic bases: sites, or modes= (then sites is None), as FermionSectorExpansion."""
    from . import api

    if isinstance(first, api.Basis):
        return _entropy_state(first, *args, renyi=renyi, **kwargs)
    return _entropy_config(first, *args, renyi=renyi, **kwargs)


def _entropy_state(basis, reps, psi, sites=None, renyi=1.0, max_bytes=DEFAULT_MAX_BYTES, modes=None):
    import torch

    nrm = float(torch.linalg.vector_norm(psi)) if isinstance(psi, torch.Tensor) and psi.numel() else 0.0
    if nrm > 0.0:
        psi = psi / nrm
    vals, _ = entanglement_spectrum(basis, reps, psi, sites, max_bytes=max_bytes, modes=modes)
    return _entropy_of(vals, float(renyi))


def _entropy_config(config, sites=None, state=None, renyi=1.0, dtype=None, eps: float = 1e-10, max_bytes=DEFAULT_MAX_BYTES, modes=None):
    import torch

    from . import api
    from .diagonalize import LocalOperator, lanczos_smallest

    load = api.loadConfigFromYaml if isinstance(config, str) else api.loadConfigFromDict
    basis, h = load(config, hamiltonian=True)
    _expansion(basis, torch.zeros(0, dtype=torch.int64), sites, modes)  # a bad subsystem is refused before anything is enumerated
    reps, _ = api.enumerateStates(basis, 1)
    if state is None:
        if dtype is None:
            dtype = torch.complex128 if _complex_characters(basis) or not h.isReal else torch.float64
        state = lanczos_smallest(LocalOperator(h, reps, dtype), num_evals=1, eps=eps).eigenvectors[0]
    return _entropy_state(basis, reps[0], state, sites, renyi=renyi, max_bytes=max_bytes, modes=modes)
