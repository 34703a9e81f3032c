"""Projection of full-basis vectors and product states into symmetry sectors (include/ls_amd.h: ls_amd_project; csrc/k_project_t.hpp).

The adjoint of the sector-state expansion (entanglement.unproject / fermion_unproject).  With the basis vectors |r~> = P|r> / n(r) of
the sector, P = |G|^-1 sum_g conj(chi(g)) U_g, U_g|r> = sign(g, r)|g r> (sign = 1 on spin bases), and B the matrix of their
columns over the ascending states of the same basis WITHOUT symmetries (unproject(psi) = B psi),
    project(Phi)[r] = <r~|Phi> = (B+ Phi)[r] = (|G| n(r))^-1 sum_g chi(g) sign(g, r) Phi[index(g r)]        (n(r) > 0; otherwise 0)
G includes the global spin inversion where the basis has one.  index is the layout unproject writes and enumerateStates gives for the
plain config: the word itself without a fixed weight, the combinadic rank at fixed weight or particle number, rank_dn C(L, N_up) +
rank_up on the spinful (N, N_up) basis.  B+ B = 1; B B+ is the projector on the sector, so sum over the sectors of |project(Phi)|^2 is
|Phi|^2.  The kernels k_project_pull / k_project_pull_fermi gather: one representative per lane, one plain store per (row, column), no
atomics -- two calls return the same bytes.

A single product state |s> needs no device pass: <r~|s> is non-zero for r = the representative of s alone, where it is
character(s) norm(r) with state_info(s) = (r, character, norm); product_state evaluates that on the host over the group elements.

ONE partition: the whole sector and the whole full-basis vector are on this device.  Spin-1/2 bases and every fermionic basis the
expansion takes, projected or not, the up <-> down flip of a spinful basis included."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import LsAmdError
from .entanglement import _complex_characters, _stream_ptr

__all__ = ["SectorProjection", "project", "product_state"]

MAX_COLUMNS = 64


def _full_size(basis):
    F = int(_lib.load().ls_amd_test_project_full_size(basis.payload))
    if F < 0:
        _lib.check(-1)
    return F


class SectorProjection:
    """ls_amd_project: the plan of projecting vectors over the full basis (the states of `basis` without symmetries, ascending) onto
    `reps` (the ascending representatives of `basis`, a 1-D int64 device tensor, one partition).  .full_size = F is known on the host,
    before a device is needed."""

    def __init__(self, basis, reps):
        import torch

        who = "SectorProjection"
        self.full_size = _full_size(basis)  # the refusals that need no device: 40 sites without a weight, the binomial table
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
                raise LsAmdError("SectorProjection: reps must be a device tensor")
            h = C.c_void_p()
            _lib.check(_lib.load().ls_amd_project_create(C.byref(h), self.basis.payload, C.c_void_p(self.reps.data_ptr()), self.reps.numel(),
                                                         _stream_ptr()))
            self.h = h
        return self.h

    def destroy(self):
        if getattr(self, "h", None):
            _lib.load().ls_amd_project_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    @property
    def kernel(self): return _lib.load().ls_amd_project_kernel_name(self._plan()).decode()

    def project(self, phi, out=None, check: bool = True):
        """-> psi (n,) for phi (F,), or (n, K) for phi (F, K), 1 <= K <= 64: the components of the columns of phi in the sector.
        phi: a device tensor over the full basis, float64 or complex128, any strides ((F, K) contiguous -- the columns interleaved --
        is the fast layout); float64 is promoted to complex128 when the characters are complex.  out: a device tensor of exactly the
        result's shape and dtype (any strides without overlap) to write into; elements of its storage outside it are not touched."""
        import torch

        who, n, F = "SectorProjection.project", int(self.reps.numel()), self.full_size
        if not isinstance(phi, torch.Tensor):
            raise LsAmdError(f"{who}: phi must be a device tensor")
        if phi.dim() not in (1, 2):
            raise LsAmdError(f"{who}: phi {tuple(phi.shape)} must be a vector of {F} elements or an ({F}, K) block of columns")
        if phi.shape[0] != F:
            raise LsAmdError(f"{who}: phi has {phi.shape[0]} rows, the basis without symmetries has {F} states")
        K = 1 if phi.dim() == 1 else int(phi.shape[1])
        if not 1 <= K <= MAX_COLUMNS:
            raise LsAmdError(f"{who}: K = {K} columns, outside [1, {MAX_COLUMNS}]; project wider blocks in slices of columns")
        if phi.dtype not in (torch.float64, torch.complex128):
            raise LsAmdError(f"{who}: phi is {phi.dtype}, neither float64 nor complex128")
        if phi.device.type != "cuda":
            raise LsAmdError(f"{who}: phi must be a device tensor (there is no CPU path)")
        if phi.dtype == torch.float64 and self.complex_characters:
            phi = phi.to(torch.complex128)
        dtype = phi.dtype
        shape = (n,) if phi.dim() == 1 else (n, K)
        if out is not None:
            if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != dtype or out.device.type != "cuda"
                    or any(s <= 0 for s, m in zip(out.stride(), out.shape) if m > 1)):
                raise LsAmdError(f"{who}: out must be a {dtype} device tensor of shape {shape} without overlapping elements")
        else:
            out = torch.empty(shape, dtype=dtype, device=phi.device)
        h = self._plan()
        ps, os_ = phi.stride(), out.stride()
        _lib.check(_lib.load().ls_amd_project_apply(h, 1 if dtype == torch.complex128 else 0, K, C.c_void_p(phi.data_ptr()), ps[0],
                                                    ps[1] if phi.dim() == 2 else 0, C.c_void_p(out.data_ptr()), os_[0],
                                                    os_[1] if out.dim() == 2 else 0, _stream_ptr()))
        if check:
            self.check()
        return out

    def check(self):
        _lib.check(_lib.load().ls_amd_project_check(self._plan(), _stream_ptr()))


def project(basis, reps, phi):
    """one-shot SectorProjection(basis, reps).project(phi): the adjoint of unproject / fermion_unproject"""
    pj = SectorProjection(basis, reps)
    try:
        return pj.project(phi)
    finally:
        pj.destroy()


def _orbit_overlap(basis, state):
    """(rep, <rep~|state> n(rep) |G|, n(rep)^2) on the host: rep = the orbit minimum of `state`, the sum of chi(g) sign(g, rep) over
    the elements g (permutations, and their products with the spin inversion) that carry rep onto `state`, and the stabiliser norm"""
    L = _lib.load()
    order = int(L.ls_amd_basis_group_order(basis.payload))
    inv = basis.spinInversion() if basis.particleType() == 0 else 0
    signed = basis.particleType() != 0 and basis.hasFermionSigns()
    mask = (1 << basis.numberBits()) - 1
    re, im = C.c_double(), C.c_double()
    chars = []
    for g in range(order):
        L.ls_amd_basis_group_character(basis.payload, g, C.byref(re), C.byref(im))
        chars.append(complex(re.value, im.value))

    def images(a):
        for g in range(order):
            t = int(L.ls_amd_basis_apply_group_element(basis.payload, g, C.c_uint64(a)))
            yield g, t, chars[g]
            if inv:
                yield g, t ^ mask, chars[g] * inv

    rep = min(t for _, t, _ in images(state))
    onto, stab = 0j, 0j
    for g, t, ch in images(rep):
        if t != state and t != rep:
            continue
        if signed:
            sg = int(L.ls_amd_test_fermion_sign(basis.payload, g, C.c_uint64(rep), 0))
            if sg == 0:
                raise LsAmdError(f"product_state: no permutation sign for element {g} of the group")
            ch = ch * sg
        if t == state:
            onto += ch
        if t == rep:
            stab += ch
    size = order * (2 if inv else 1)
    return rep, onto, stab.real / size, size


def _sector_text(basis):
    spec = getattr(basis, "spec", None)
    if spec is None:
        return f"this sector (a group of {basis.groupOrder()} permutations)"
    parts = [f"sectors {list(spec.sectors)} of its {len(spec.permutations)} generators"]
    if spec.spin_inversion:
        parts.append(f"spin inversion {spec.spin_inversion:+d}")
    if spec.spin_flip:
        parts.append(f"spin flip {spec.spin_flip:+d}")
    return "the sector with " + ", ".join(parts)


def product_state(basis, reps, state, dtype=None):
    """-> (psi, weight): the product state |state> (an int word of the basis) projected into the sector and normalised -- a device
    vector on `reps` with the single entry character(state) at the representative of the state -- and weight = norm(rep)^2, the
    weight of |state> in the sector (the weights of a state over all sectors of an abelian group add up to 1).  dtype: float64 when
    the entry is real and the characters are +-1, otherwise complex128.  Evaluated on the host but for placing the value."""
    import torch

    who = "product_state"
    if isinstance(state, bool) or not isinstance(state, (int, np.integer)):
        raise LsAmdError(f"{who}: state must be an int word, got {state!r}")
    state = int(state)
    if state < 0 or state >> 64:
        raise LsAmdError(f"{who}: the state {state:#x} is no 64-bit word")
    if int(_lib.load().ls_amd_test_project_state_index(basis.payload, C.c_uint64(state))) < 0:  # bits above the sites, weight, numbers
        _lib.check(-1)
    if isinstance(reps, (list, tuple)):
        if len(reps) != 1:
            raise LsAmdError(f"{who}: one partition (the whole sector on this device), got {len(reps)} blocks of representatives")
        reps = reps[0]
    if not isinstance(reps, torch.Tensor) or reps.dim() != 1 or reps.dtype != torch.int64:
        raise LsAmdError(f"{who}: reps must be a 1-D int64 tensor (one partition)")
    rep, onto, n2, size = _orbit_overlap(basis, state)
    bits = basis.numberBits()
    if not n2 > 1e-12 or abs(onto) == 0.0:
        raise LsAmdError(f"{who}: the state {state:#0{bits + 2}b} has zero weight in {_sector_text(basis)}: the orbit of its representative "
                         f"{rep:#x} has norm 0 there")
    entry = onto / abs(onto)  # <rep~|state> / n(rep) = character(state): of unit modulus
    real = entry.imag == 0.0 and not _complex_characters(basis)
    if dtype is None:
        dtype = torch.float64 if real else torch.complex128
    if dtype not in (torch.float64, torch.complex128):
        raise LsAmdError(f"{who}: dtype {dtype} is neither float64 nor complex128")
    if dtype == torch.float64 and not real:
        raise LsAmdError(f"{who}: the entry {entry} is complex (or the characters are): float64 cannot hold the state")
    signed = rep - (1 << 64) if rep >> 63 else rep  # the int64 image of the word, as reps holds it
    at = torch.nonzero(reps == signed).reshape(-1)
    if at.numel() != 1:
        raise LsAmdError(f"{who}: the representative {rep:#x} of the state {state:#x} is not among reps: the array does not belong to this basis")
    psi = torch.zeros(reps.numel(), dtype=dtype, device=reps.device)
    psi[at] = entry.real if dtype == torch.float64 else entry
    return psi, float(n2)
