"""Host-side mirror of the reference's operator interface for the matvec path.

Names, argument meaning and error behaviour follow the Chapel modules they stand in for:
    Basis, Operator, loadConfigFromYaml     /root/reference/src/ForeignTypes.chpl:8-288
    enumerateStates                          /root/reference/src/StatesEnumeration.chpl:516-585
    arrFromBlockToHashed / arrFromHashedToBlock   /root/reference/src/BlockToHashed.chpl:87,
                                             /root/reference/src/HashedToBlock.chpl:67
    matrixVectorProduct / localMatrixVector  /root/reference/src/DistributedMatrixVector.chpl:1055-1093
so that the parity tests read like test/TestMatrixVectorProduct.chpl.  Everything that computes
calls the C ABI of libls_amd.so (include/*.h); torch only provides device memory and streams.
A "BlockVector" here is simply a list with one device tensor per locale (hash partition).
uint64 arrays are held as torch.int64 tensors (bit-identical).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import config as _config
from ._lib import LsAmdError

__all__ = [
    "Basis", "Operator", "LsAmdError", "loadConfigFromYaml", "loadConfigFromDict", "enumerateStates",
    "arrFromBlockToHashed", "arrFromHashedToBlock", "matrixVectorProduct", "localMatrixVector",
    "localeIdxOf", "hash64_01", "MatvecPlan", "ReplicatedPlan", "build_library", "fillRandom",
    "Communicator", "DistMatvec", "ReplMatvec", "block_axpby_dots", "block_axpby_acc", "CrossSectorPlan",
    "CsrMatrix",
]


def build_library(verbose: bool = False):
    """hipcc --offload-arch=gfx950 build of libls_amd.so in-tree (cross-compiles without a GPU)."""
    import os
    import subprocess

    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    subprocess.check_call(["make", "-C", csrc] + ([] if verbose else ["-s"]))
    return _lib.LIB_PATH


def _torch():
    import torch

    return torch


def _stream_ptr():
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def hash64_01(x: int) -> int:
    """/root/reference/src/StatesEnumeration.chpl:122-127"""
    return int(_lib.load().ls_amd_hash64_01(C.c_uint64(x)))


def localeIdxOf(basisState: int, numLocales: int) -> int:
    """/root/reference/src/StatesEnumeration.chpl:133-136"""
    return int(_lib.load().ls_amd_locale_idx_of(C.c_uint64(basisState), numLocales))


class Basis:
    """RAII wrapper of ls_hs_basis (ForeignTypes.chpl:8-117)."""

    def __init__(self, payload, owning=True, spec=None):
        self.payload = payload
        self.owning = owning
        self.spec = spec
        self._host_reps = None  # keeps a numpy array alive for uncheckedSetRepresentatives

    @staticmethod
    def fromSpec(spec: _config.BasisSpec) -> "Basis":
        L = _lib.load()
        ng = len(spec.permutations)
        perms = (C.c_int * max(1, ng * spec.number_sites))(*[v for p in spec.permutations for v in p])
        sectors = (C.c_int * max(1, ng))(*spec.sectors)
        if spec.particle == "spinless-fermion" and ng > 0:  # with the permutation signs of the modes (parse_basis: number_up unset)
            p = L.ls_hs_create_spinless_fermion_basis(spec.number_sites, spec.number_particles, ng, perms, sectors)
        elif spec.particle == "spinful-fermion" and (ng > 0 or spec.spin_flip):  # site permutations lifted to both species, ↑↔↓ flip
            p = L.ls_hs_create_spinful_fermion_basis(spec.number_sites, spec.number_particles, spec.number_up, spec.spin_flip, ng, perms, sectors)
        elif spec.is_fermionic:  # no symmetries: the unprojected bases (closed-form index, k_hubbard)
            p = L.ls_hs_create_basis(_config.PARTICLES[spec.particle], spec.number_sites, spec.number_particles, spec.number_up)
        else:
            p = L.ls_hs_create_spin_basis(spec.number_sites, spec.hamming_weight, spec.spin_inversion, ng, perms, sectors)
        if not p:
            raise LsAmdError(L.ls_amd_last_error().decode())
        return Basis(p, True, spec)

    def __del__(self):
        try:
            if self.owning and self.payload:
                _lib.load().ls_hs_destroy_basis(self.payload)
                self.payload = None
        except Exception:
            pass

    # accessors, same names as the Chapel record ------------------------------------------------
    def numberSites(self): return int(self.payload.contents.number_sites)
    def numberBits(self): return int(_lib.load().ls_hs_basis_number_bits(self.payload))
    def numberWords(self): return int(_lib.load().ls_hs_basis_number_words(self.payload))
    def spinInversion(self): return int(self.payload.contents.spin_inversion)
    def particleType(self): return int(self.payload.contents.particle_type)  # config.PARTICLES
    def numberParticles(self): return int(self.payload.contents.number_particles)
    def numberUp(self): return int(self.payload.contents.number_up)
    def isStateIndexIdentity(self): return bool(self.payload.contents.state_index_is_identity)
    def requiresProjection(self): return bool(self.payload.contents.requires_projection)
    def isHammingWeightFixed(self): return bool(_lib.load().ls_hs_basis_has_fixed_hamming_weight(self.payload))
    def hasSpinInversionSymmetry(self): return bool(_lib.load().ls_hs_basis_has_spin_inversion_symmetry(self.payload))
    def hasPermutationSymmetries(self): return bool(_lib.load().ls_hs_basis_has_permutation_symmetries(self.payload))
    def hasFermionSigns(self): return bool(_lib.load().ls_amd_basis_fermion_signs(self.payload))  # projected fermions
    def spinFlip(self): return int(_lib.load().ls_amd_basis_spin_flip(self.payload))  # spinful fermions: ↑↔↓ character, 0 = none
    def minStateEstimate(self): return int(_lib.load().ls_hs_min_state_estimate(self.payload))
    def maxStateEstimate(self): return int(_lib.load().ls_hs_max_state_estimate(self.payload))
    def groupOrder(self): return int(_lib.load().ls_amd_basis_group_order(self.payload))

    def build(self):
        """ls_hs_basis_build (ForeignTypes.chpl:72): dispatches to the registered enumerate_states
        kernel, i.e. ls_chpl_enumerate_representatives -> the HIP enumeration."""
        _lib.require_device()
        _lib.load().ls_hs_basis_build(self.payload)
        _lib.raise_pending_halt()

    def uncheckedSetRepresentatives(self, representatives: np.ndarray):
        """ForeignTypes.chpl:74-77 (borrows host memory)."""
        arr = np.ascontiguousarray(representatives, dtype=np.uint64)
        self._host_reps = arr
        ext = _lib.ChplExternalArray(arr.ctypes.data, arr.size, None)
        _lib.load().ls_hs_unchecked_set_representatives(self.payload, C.byref(ext))

    def representatives(self) -> np.ndarray:
        """ForeignTypes.chpl:111-116; halts with "basis is not built"."""
        rs = self.payload.contents.representatives
        if not rs.elts:
            raise LsAmdError("halt: basis is not built")
        buf = (C.c_uint64 * rs.num_elts).from_address(rs.elts)
        return np.frombuffer(buf, dtype=np.uint64)


class Operator:
    """RAII wrapper of ls_hs_operator (ForeignTypes.chpl:154-259)."""

    def __init__(self, payload, owning=True):
        self.payload = payload
        self.owning = owning
        self.basis = Basis(payload.contents.basis, owning=False)
        self._plans = {}

    @staticmethod
    def fromSpec(basis: Basis, spec: _config.OperatorSpec) -> "Operator":
        L = _lib.load()
        n = len(spec.terms)
        v = np.zeros(2 * max(n, 1), dtype=np.float64)
        m = np.zeros(max(n, 1), dtype=np.uint64)
        r = np.zeros(max(n, 1), dtype=np.uint64)
        x = np.zeros(max(n, 1), dtype=np.uint64)
        s = np.zeros(max(n, 1), dtype=np.uint64)
        for i, (vv, mm, rr, xx, ss) in enumerate(spec.terms):
            v[2 * i], v[2 * i + 1] = vv.real, vv.imag
            m[i], r[i], x[i], s[i] = mm, rr, xx, ss
        p = L.ls_hs_create_operator_from_terms(
            basis.payload, n, v.ctypes.data_as(_lib.c_f64p), m.ctypes.data_as(_lib.c_u64p),
            r.ctypes.data_as(_lib.c_u64p), x.ctypes.data_as(_lib.c_u64p), s.ctypes.data_as(_lib.c_u64p))
        if not p:
            raise LsAmdError(L.ls_amd_last_error().decode())
        op = Operator(p, True)
        op.basis.spec = basis.spec
        return op

    def clear_plans(self):
        """destroy the cached matvec plans (and release the HBM they pin)"""
        for pl in list(self._plans.values()):
            pl.destroy()
        self._plans.clear()

    def __del__(self):
        try:
            self.clear_plans()
            if self.owning and self.payload:
                _lib.load().ls_hs_destroy_operator(self.payload)
                self.payload = None
        except Exception:
            pass

    def numberDiagTerms(self):
        p = self.payload.contents.diag_terms
        return int(p.contents.number_terms) if p else 0

    def numberOffDiagTerms(self):
        return int(_lib.load().ls_hs_operator_max_number_off_diag(self.payload))

    @property
    def isHermitian(self): return bool(_lib.load().ls_hs_operator_is_hermitian(self.payload))

    @property
    def isReal(self): return bool(_lib.load().ls_hs_operator_is_real(self.payload))

    def adjoint(self) -> "Operator":
        """A^+ on the same basis (ls_amd_operator_adjoint): the conjugate transpose of every term; host only"""
        L = _lib.load()
        p = L.ls_amd_operator_adjoint(self.payload)
        if not p:
            raise LsAmdError(L.ls_amd_last_error().decode())
        out = Operator(p, True)
        out.basis.spec = self.basis.spec
        return out

    def mapsSector(self, target_basis: Basis, explain: bool = False, signs: bool = False, subgroup: bool = False) -> bool:
        """whether this operator maps its own (source) sector into the sector of target_basis (ls_amd_operator_maps_sector: the
        exact covariance check U_g A U_g^-1 = chi2(g) conj(chi1(g)) A on the term tables; host only).  explain=True raises LsAmdError
        with the reason -- the offending generator, or why the two bases cannot be paired -- instead of returning False.
        signs=True runs the rule that CrossSectorPlan runs (ls_amd_operator_maps_sector_signed): the same answer for bases without
        permutation signs, and for projected fermionic bases -- which the plain rule refuses -- the covariance under
        U_g|a> = sign(g, a)|g.a>, with the Jordan-Wigner strings of the terms absorbed (c+_k, c_k, n_q, S^z_q, pair operators
        between momentum, point-group and spin-flip sectors; particle numbers are not examined).
        subgroup=True runs the rule of CrossSectorPlan(groups="restrict") instead (ls_amd_operator_maps_subgroup_sector): the two
        bases may have different generators as long as every generator of the target is an element of the source group (and a
        spin inversion / spin_flip of the target is one of the source), and the covariance is asked of the TARGET's generators
        only, with chi1 taken from the source's element -- signed where a basis is a projected fermionic one, whatever `signs`."""
        L = _lib.load()
        if subgroup:
            rule = L.ls_amd_operator_maps_subgroup_sector
        else:
            rule = L.ls_amd_operator_maps_sector_signed if signs else L.ls_amd_operator_maps_sector
        rc = rule(self.payload, target_basis.payload)
        if rc != 0 and explain:
            raise LsAmdError(L.ls_amd_last_error().decode("utf-8", "replace"))
        _lib.raise_pending_halt()
        return rc == 0

    def to_csr(self, reps, dtype=None, max_bytes: int = 8 << 30) -> "CsrMatrix":
        """the matrix of this operator on its own basis, rows and columns in the order of `reps` (its ascending representatives: a
        1-D int64 device tensor, or a list of one -- one partition), as canonical CSR on the device: a CrossSectorPlan with
        self.basis on both sides, exported (CrossSectorPlan.to_csr).  dtype None: float64 when the operator is real and every
        character of the basis is +-1, else complex128."""
        torch = _torch()
        if isinstance(reps, (list, tuple)):
            if len(reps) != 1:
                raise LsAmdError(f"Operator.to_csr: one partition (the whole sector on this device), got {len(reps)} blocks of representatives")
            reps = reps[0]
        if dtype is None:
            dtype = torch.float64 if self.isReal and not _complex_characters(self.basis) else torch.complex128
        plan = CrossSectorPlan(self, reps, self.basis, reps, dtype)
        try:
            return plan.to_csr(max_bytes=max_bytes)
        finally:
            plan.destroy()

    def to_dense(self, reps, dtype=None, max_bytes: int = 8 << 30):
        """to_csr(...).to_dense(...): the (n, n) device matrix; max_bytes bounds the export and the dense matrix alike"""
        return self.to_csr(reps, dtype=dtype, max_bytes=max_bytes).to_dense(max_bytes=max_bytes)

    # host-pointer entry points of the kernel table ----------------------------------------------
    def __matmul__(self, x: np.ndarray) -> np.ndarray:
        """kernels->matrix_vector_product (ls_chpl_matrix_vector_product, DMV:1095-1110) on host
        f64 arrays; y starts zeroed."""
        _lib.require_device()
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        _lib.load().ls_chpl_matrix_vector_product(self.payload, 1, x.ctypes.data_as(_lib.c_f64p), y.ctypes.data_as(_lib.c_f64p))
        _lib.raise_pending_halt()
        return y

    def applyDiag(self, alphas: np.ndarray) -> np.ndarray:
        """ls_chpl_operator_apply_diag (BatchedOperator.chpl:217-234)."""
        _lib.require_device()
        alphas = np.ascontiguousarray(alphas, dtype=np.uint64)
        out = _lib.ChplExternalArray()
        _lib.load().ls_chpl_operator_apply_diag(self.payload, alphas.size, alphas.ctypes.data_as(_lib.c_u64p), C.byref(out), 1)
        _lib.raise_pending_halt()
        return _take_external(out, np.float64, 1)

    def applyOffDiag(self, alphas: np.ndarray):
        """ls_chpl_operator_apply_off_diag (BatchedOperator.chpl:236-275) -> (betas, coeffs, offsets)."""
        _lib.require_device()
        alphas = np.ascontiguousarray(alphas, dtype=np.uint64)
        b, c, o = _lib.ChplExternalArray(), _lib.ChplExternalArray(), _lib.ChplExternalArray()
        _lib.load().ls_chpl_operator_apply_off_diag(self.payload, alphas.size, alphas.ctypes.data_as(_lib.c_u64p),
                                                    C.byref(b), C.byref(c), C.byref(o), 1)
        _lib.raise_pending_halt()
        offsets = _take_external(o, np.int64, 1)
        betas = _take_external(b, np.uint64, 1)
        coeffs = _take_external(c, np.complex128, 1)
        return betas, coeffs, offsets


_libc_free = None


def _take_external(arr: "_lib.ChplExternalArray", dtype, _unused):
    """copies a callee-allocated chpl_external_array into numpy and frees it through `freer`."""
    n = int(arr.num_elts)
    if not arr.elts or n == 0:
        return np.zeros(0, dtype=dtype)
    itemsize = np.dtype(dtype).itemsize
    buf = (C.c_char * (n * itemsize)).from_address(arr.elts)
    out = np.frombuffer(buf, dtype=dtype).copy()
    if arr.freer:
        C.CFUNCTYPE(None, C.c_void_p)(arr.freer)(arr.elts)
    return out


def loadConfigFromDict(cfg: dict, hamiltonian: bool = False, observables: bool = False):
    bspec = _config.parse_basis(cfg)
    basis = Basis.fromSpec(bspec)
    h = None
    if hamiltonian:
        if cfg.get("hamiltonian") is None:
            raise LsAmdError("halt: config does not contain a Hamiltonian")  # ForeignTypes.chpl:273-274
        h = Operator.fromSpec(basis, _config.parse_operator(cfg["hamiltonian"], bspec))
    obs = [Operator.fromSpec(basis, _config.parse_operator(o, bspec)) for o in (cfg.get("observables") or [])] if observables else []
    if not hamiltonian and not observables:
        return basis
    if hamiltonian and not observables:
        return basis, h
    if not hamiltonian and observables:
        return basis, obs
    return basis, h, obs


def loadConfigFromYaml(filename: str, hamiltonian: bool = False, observables: bool = False):
    """ForeignTypes.chpl:261-288, step by step: ls_hs_load_yaml_config (the C library's own loader, csrc/yaml.c) -> clone
    basis / hamiltonian / observables -> ls_hs_destroy_yaml_config."""
    L = _lib.load()
    conf = L.ls_hs_load_yaml_config(filename.encode())
    if not conf:
        raise LsAmdError(f"halt: failed to load Config from '{filename}' ({L.ls_amd_last_error().decode()})")
    try:
        c = conf.contents
        basis = Basis(L.ls_hs_clone_basis(c.basis), owning=True)
        h = None
        if hamiltonian:
            if not c.hamiltonian:
                raise LsAmdError(f"halt: '{filename}' does not contain a Hamiltonian")  # ForeignTypes.chpl:273-274
            h = Operator(L.ls_hs_clone_operator(c.hamiltonian), owning=True)
        obs = [Operator(L.ls_hs_clone_operator(c.observables[i]), owning=True) for i in range(c.number_observables)] if observables else []
    finally:
        L.ls_hs_destroy_yaml_config(conf)
    if not hamiltonian and not observables:
        return basis
    if hamiltonian and not observables:
        return basis, h
    if not hamiltonian and observables:
        return basis, obs
    return basis, h, obs


# ------------------------------------------------------------------------------------------------
# device-side pieces
# ------------------------------------------------------------------------------------------------

def _adopt(ptr: int, count: int, torch_dtype):
    """copies a library-owned device array into a torch tensor and frees the original."""
    torch = _torch()
    L = _lib.load()
    t = torch.empty(count, dtype=torch_dtype, device="cuda")
    try:
        if count > 0:
            _lib.check(L.ls_amd_memcpy_d2d(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), count * t.element_size(), _stream_ptr()))
            _lib.check(L.ls_amd_synchronize(_stream_ptr()))
    finally:
        if ptr:
            L.ls_amd_free(C.c_void_p(ptr))
    return t


def _complex_characters(basis: Basis) -> bool:
    """whether some character of the basis' group is not +-1 (host only)"""
    L = _lib.load()
    re, im = C.c_double(), C.c_double()
    for g in range(int(L.ls_amd_basis_group_order(basis.payload))):
        L.ls_amd_basis_group_character(basis.payload, g, C.byref(re), C.byref(im))
        if im.value != 0.0 or abs(re.value) != 1.0:
            return True
    return False


@dataclass
class CsrMatrix:
    """A sparse matrix in canonical CSR form (include/ls_amd.h, ls_amd_csr): shape = (rows, columns); crow_indices int64
    [rows + 1]; col_indices int64 [nnz], strictly ascending inside every row; values float64 or complex128 [nnz].  What
    CrossSectorPlan.to_csr and Operator.to_csr return (device tensors); any three tensors on one device do."""
    shape: tuple
    crow_indices: object
    col_indices: object
    values: object

    @property
    def nnz(self) -> int:
        return int(self.col_indices.numel())

    @property
    def dtype(self):
        return self.values.dtype

    def row_indices(self):
        """the row of every entry (int64 [nnz])"""
        torch = _torch()
        counts = self.crow_indices[1:] - self.crow_indices[:-1]
        return torch.repeat_interleave(torch.arange(self.shape[0], dtype=torch.int64, device=counts.device), counts, output_size=self.nnz)

    def to_dense(self, max_bytes: int = 8 << 30):
        """the (rows, columns) matrix on the device of the arrays, by an indexed store (no sparse kernels of torch)"""
        torch = _torch()
        rows, cols = int(self.shape[0]), int(self.shape[1])
        need = rows * cols * self.values.element_size()
        if need > max_bytes:
            raise LsAmdError(f"CsrMatrix.to_dense: the dense {rows} x {cols} matrix needs {need} bytes, max_bytes is {max_bytes}")
        out = torch.zeros((rows, cols), dtype=self.values.dtype, device=self.values.device)
        if self.nnz:
            out[self.row_indices(), self.col_indices] = self.values
        return out

    def to_torch(self):
        """the same arrays as a torch.sparse_csr_tensor"""
        return _torch().sparse_csr_tensor(self.crow_indices, self.col_indices, self.values, size=tuple(self.shape))


def enumerateStates(basis: Basis, numLocales: int = 1):
    """enumerateStates(basis, masks) (StatesEnumeration.chpl:580-585): returns
    (basisStates, masks) -- basisStates[p] = ascending representatives owned by locale p
    (hash64_01 % numLocales), masks = owner of every state in global ascending order."""
    _lib.require_device()
    torch = _torch()
    L = _lib.load()
    d_states, d_masks, count = C.c_void_p(), C.c_void_p(), C.c_int64()
    _lib.check(L.ls_amd_enumerate_states(basis.payload, numLocales, C.byref(d_states), C.byref(d_masks), C.byref(count), _stream_ptr()))
    states = _adopt(d_states.value, count.value, torch.int64)
    masks = _adopt(d_masks.value, count.value, torch.uint8)
    parts = [states] if numLocales == 1 else arrFromBlockToHashed(states, masks, numLocales)
    return parts, masks


def _mask_counts(masks, numLocales):
    counts = (C.c_int64 * numLocales)()
    _lib.check(_lib.load().ls_amd_mask_counts(masks.numel(), C.c_void_p(masks.data_ptr()), numLocales, counts, _stream_ptr()))
    return [int(c) for c in counts]


def arrFromBlockToHashed(arr, masks, numLocales: int):
    """BlockToHashed.chpl:87-208: stable partition of a block-order device tensor (8- or 16-byte
    elements) into one tensor per locale."""
    torch = _torch()
    _lib.require_device()
    assert arr.is_cuda and masks.is_cuda and arr.is_contiguous()
    n = arr.numel()
    assert masks.numel() == n
    counts = _mask_counts(masks, numLocales)
    parts = [torch.empty(c, dtype=arr.dtype, device=arr.device) for c in counts]
    dest = (C.c_void_p * numLocales)(*[p.data_ptr() for p in parts])
    _lib.check(_lib.load().ls_amd_block_to_hashed(n, C.c_void_p(masks.data_ptr()), numLocales, arr.element_size(),
                                                  C.c_void_p(arr.data_ptr()), dest, _stream_ptr()))
    return parts


def arrFromHashedToBlock(parts, masks):
    """HashedToBlock.chpl:67-153: inverse of arrFromBlockToHashed."""
    torch = _torch()
    _lib.require_device()
    numLocales = len(parts)
    n = masks.numel()
    out = torch.empty(n, dtype=parts[0].dtype, device=parts[0].device)
    src = (C.c_void_p * numLocales)(*[p.data_ptr() for p in parts])
    _lib.check(_lib.load().ls_amd_hashed_to_block(n, C.c_void_p(masks.data_ptr()), numLocales, parts[0].element_size(),
                                                  src, C.c_void_p(out.data_ptr()), _stream_ptr()))
    return out


def _dots_ptr(dots, K, who):
    """device pointer of the 2K float64 dots of a Chebyshev step (None: NULL)"""
    if dots is None:
        return None
    torch = _torch()
    if (not isinstance(dots, torch.Tensor) or dots.dtype != torch.float64 or dots.device.type != "cuda" or not dots.is_contiguous()
            or dots.numel() != 2 * K):
        raise _lib.LsAmdError(f"{who}: dots must be a contiguous float64 device tensor of 2K = {2 * K} elements")
    return C.c_void_p(dots.data_ptr())


def block_axpby_dots(w, x, y, alpha, beta, gamma, dots=None):
    """Y <- alpha W + beta X + gamma Y on (N, K) device tensors of one dtype (float64 or complex128), any nested strides, and the two
    dots of matvec_block_axpby (ls_amd_block_axpby_dots): the epilogue pass of the Chebyshev step on its own, no plan.  gamma == 0:
    y is not read."""
    torch = _torch()
    for name, t in (("w", w), ("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise _lib.LsAmdError(f"block_axpby_dots: {name} must be a 2-D (N, K) tensor")
        if t.dtype != x.dtype or t.dtype not in (torch.float64, torch.complex128):
            raise _lib.LsAmdError(f"block_axpby_dots: {name} is {t.dtype}; w, x and y must all be float64 or all complex128")
        if t.device.type != "cuda":
            raise _lib.LsAmdError(f"block_axpby_dots: {name} must be a device tensor")
    if tuple(w.shape) != tuple(x.shape) or tuple(y.shape) != tuple(x.shape):
        raise _lib.LsAmdError(f"block_axpby_dots: w {tuple(w.shape)}, x {tuple(x.shape)} and y {tuple(y.shape)} must have one shape")
    n, K = int(x.shape[0]), int(x.shape[1])
    _lib.check(_lib.load().ls_amd_block_axpby_dots(int(x.dtype == torch.complex128), n, K, C.c_void_p(w.data_ptr()), w.stride(0), w.stride(1),
                                                   C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), C.c_void_p(y.data_ptr()), y.stride(0),
                                                   y.stride(1), float(alpha), float(beta), float(gamma),
                                                   _dots_ptr(dots, K, "block_axpby_dots"), _stream_ptr()))


def _as_block(t):
    """a vector is a block of one column"""
    return t.unsqueeze(1) if _torch().is_tensor(t) and t.dim() == 1 else t


def _acc_args(who, blocks, z, c, want=None):
    """the checks block_axpby_acc and matvec_block_axpby_acc share -> (blocks and z as (N, K) tensors, c as a complex)"""
    torch = _torch()
    blocks = [(name, _as_block(t)) for name, t in blocks]
    z = _as_block(z)
    x = blocks[0][1]
    dtype = want if want is not None else (x.dtype if isinstance(x, torch.Tensor) else None)
    for name, t in blocks + [("z", z)]:
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise _lib.LsAmdError(f"{who}: {name} must be a 1-D (N) or 2-D (N, K) tensor")
        if t.device.type != "cuda":
            raise _lib.LsAmdError(f"{who}: {name} must be a device tensor")
    for name, t in blocks:
        if t.dtype != dtype or t.dtype not in (torch.float64, torch.complex128):
            raise _lib.LsAmdError(f"{who}: {name} is {t.dtype}" + (f", the plan computes in {want}" if want is not None else
                                                                   f"; {', '.join(n for n, _ in blocks)} must all be float64 or all complex128"))
    if z.dtype not in (torch.float64, torch.complex128):
        raise _lib.LsAmdError(f"{who}: z is {z.dtype}: float64 or complex128")
    c = complex(c)
    if dtype == torch.complex128 and z.dtype == torch.float64:
        raise _lib.LsAmdError(f"{who}: z is float64 next to complex128 vectors: the accumulator must be complex128")
    if z.dtype == torch.float64 and c.imag != 0.0:
        raise _lib.LsAmdError(f"{who}: z is float64 and c = {c!r} is not real: the accumulator must be complex128")
    for name, t in blocks[1:] + [("z", z)]:
        if tuple(t.shape) != tuple(x.shape):
            raise _lib.LsAmdError(f"{who}: {name} {tuple(t.shape)} and {blocks[0][0]} {tuple(x.shape)} must have one shape")
    return [t for _, t in blocks], z, c


def block_axpby_acc(w, x, y, alpha, beta, gamma, z, c, dots=None):
    """block_axpby_dots, and Z <- Z + c Y with the new Y in the same pass (ls_amd_block_axpby_acc): the epilogue of the accumulate
    step of Chebyshev time evolution on its own, no plan.  w, x, y: float64 or complex128; z: the same, or complex128 next to
    float64 (then c may be complex); strides of its own.  z must not overlap w, x or y."""
    torch = _torch()
    (x, w, y), z, c = _acc_args("block_axpby_acc", [("x", x), ("w", w), ("y", y)], z, c)
    n, K = int(x.shape[0]), int(x.shape[1])
    _lib.check(_lib.load().ls_amd_block_axpby_acc(int(x.dtype == torch.complex128), int(z.dtype == torch.complex128), n, K,
                                                  C.c_void_p(w.data_ptr()), w.stride(0), w.stride(1), C.c_void_p(x.data_ptr()), x.stride(0),
                                                  x.stride(1), C.c_void_p(y.data_ptr()), y.stride(0), y.stride(1), C.c_void_p(z.data_ptr()),
                                                  z.stride(0), z.stride(1), float(alpha), float(beta), float(gamma), c.real, c.imag,
                                                  _dots_ptr(dots, K, "block_axpby_acc"), _stream_ptr()))


class MatvecPlan:
    """ls_amd_plan: binds an Operator to a partition layout (include/ls_amd.h)."""

    MODES = {"auto": 0, "push": 1, "pull": 2}

    def __init__(self, matrix: Operator, representatives, dtype, my_partition: int = -1,
                 num_partitions: int | None = None, num_rounds: int = 0, mode: str = "auto"):
        torch = _torch()
        _lib.require_device()
        L = _lib.load()
        self.matrix = matrix
        reps = list(representatives) if my_partition < 0 else [representatives]
        self.reps = reps  # borrowed by the plan: keep alive
        self.P = num_partitions if num_partitions is not None else len(reps)
        self.me = my_partition
        self.cplx = dtype in (torch.complex128, "c128")
        n = len(reps)
        ptrs = (C.c_void_p * n)(*[r.data_ptr() for r in reps])
        counts = (C.c_int64 * n)(*[r.numel() for r in reps])
        h = C.c_void_p()
        _lib.check(L.ls_amd_plan_create(C.byref(h), matrix.payload, 1 if self.cplx else 0, self.P, my_partition,
                                        ptrs, counts, num_rounds, self.MODES[mode], _stream_ptr()))
        self.h = h

    def destroy(self):
        if getattr(self, "h", None):
            _lib.load().ls_amd_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    @property
    def kernel(self): return _lib.load().ls_amd_plan_kernel_name(self.h).decode()
    @property
    def num_rounds(self): return int(_lib.load().ls_amd_plan_num_rounds(self.h))
    @property
    def nnz(self): return int(_lib.load().ls_amd_plan_nnz(self.h))
    @property
    def packet_bytes(self): return int(_lib.load().ls_amd_plan_packet_bytes(self.h))
    @property
    def row_bytes(self): return int(_lib.load().ls_amd_plan_row_bytes(self.h))
    @property
    def key_bytes(self):
        """8: packets carry the state; 4: pre-indexed packets (u32 index at the destination; include/ls_amd.h)"""
        return int(_lib.load().ls_amd_plan_key_bytes(self.h))
    @property
    def packet_index_bytes(self): return int(_lib.load().ls_amd_plan_packet_index_bytes(self.h))

    def segment_bytes(self, count: int) -> int:
        """bytes of a segment of `count` packets: [key x count, padded to 8 bytes][value x count]"""
        return int(_lib.load().ls_amd_plan_segment_bytes(self.h, int(count)))

    def segment_value_offset(self, count: int) -> int:
        return int(_lib.load().ls_amd_plan_segment_value_offset(self.h, int(count)))

    def cache_slots(self, max_bytes: int = 0) -> int:
        """keep the resolved packet streams (slot of every partner, 5 B per non-zero on the Heisenberg models) across matvecs:
        the first matvec resolves them, later ones only gather -- for plans that are applied many times (eigensolvers).  Opt-in,
        not matrix-free; returns the rows cached (0: nothing, e.g. an unprojected basis or no room)."""
        rows = int(_lib.load().ls_amd_plan_cache_slots(self.h, int(max_bytes)))
        if rows < 0:
            _lib.check(-1)
        return rows

    @property
    def slot_cache(self):
        """(rows, bytes) held by the slot cache"""
        r, b = C.c_int64(0), C.c_int64(0)
        _lib.load().ls_amd_plan_slot_cache_rows(self.h, C.byref(r), C.byref(b))
        return int(r.value), int(b.value)

    def send_counts(self, rnd: int):
        c = (C.c_int64 * self.P)()
        _lib.check(_lib.load().ls_amd_plan_send_counts(self.h, rnd, c))
        return [int(v) for v in c]

    def matvec(self, x, y, check: bool = True):
        xs = (C.c_void_p * len(x))(*[t.data_ptr() for t in x])
        ys = (C.c_void_p * len(y))(*[t.data_ptr() for t in y])
        _lib.check(_lib.load().ls_amd_matvec(self.h, xs, ys, _stream_ptr()))
        if check:
            self.check()

    def matvec_block(self, x, y, check: bool = True):
        """Y[:, k] <- H X[:, k] for the K columns of the (N, K) device tensors x and y (ls_amd_matvec_block): any strides -- (K, 1)
        interleaved is the fast layout, a transposed (K, N) tensor the column-major one -- and the plan's dtype.  One-partition
        plans, 1 <= K <= 64; y is assigned.  LS_AMD_BLOCK=auto|kernel|columns picks the path (block_kernel(K) names it)."""
        torch = _torch()
        if self.P != 1 or self.me >= 0:
            raise _lib.LsAmdError(f"matvec_block: one-partition plans only (this plan has P = {self.P}, my_partition = {self.me})")
        want = torch.complex128 if self.cplx else torch.float64
        for name, t in (("x", x), ("y", y)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise _lib.LsAmdError(f"matvec_block: {name} must be a 2-D (N, K) tensor")
            if t.dtype != want:
                raise _lib.LsAmdError(f"matvec_block: {name} is {t.dtype}, the plan computes in {want}")
            if t.device.type != "cuda":
                raise _lib.LsAmdError(f"matvec_block: {name} must be a device tensor")
        n = self.reps[0].numel()
        if tuple(x.shape) != tuple(y.shape) or x.shape[0] != n:
            raise _lib.LsAmdError(f"matvec_block: x {tuple(x.shape)} and y {tuple(y.shape)} must both be ({n}, K)")
        K = int(x.shape[1])
        _lib.check(_lib.load().ls_amd_matvec_block(self.h, K, C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1),
                                                   C.c_void_p(y.data_ptr()), y.stride(0), y.stride(1), _stream_ptr()))
        if check:
            self.check()

    def block_kernel(self, K: int) -> str:
        """path a block of K columns takes on this plan: "k_direct_blk", "k_pull_gather_blk" or "columns" """
        name = _lib.load().ls_amd_plan_block_kernel_name(self.h, int(K))
        if name is None:
            _lib.check(-1)
        return name.decode()

    def matvec_block_axpby(self, x, y, alpha, beta, gamma, dots=None, check: bool = True):
        """Y[:, k] <- alpha (H X)[:, k] + beta X[:, k] + gamma Y[:, k] for the K columns of the (N, K) device tensors x and y
        (ls_amd_matvec_block_axpby; alpha, beta, gamma real): the Chebyshev / Lanczos step.  dots: None, or a contiguous float64
        device tensor of 2K elements, assigned [k] = <X_k|X_k>, [K + k] = Re <X_k|Y_k> with the new Y.  gamma == 0: y is not read.
        Tensors, strides and LS_AMD_BLOCK as matvec_block; axpby_kernel(K) names the path."""
        torch = _torch()
        if self.P != 1 or self.me >= 0:
            raise _lib.LsAmdError(f"matvec_block_axpby: one-partition plans only (this plan has P = {self.P}, my_partition = {self.me})")
        want = torch.complex128 if self.cplx else torch.float64
        for name, t in (("x", x), ("y", y)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise _lib.LsAmdError(f"matvec_block_axpby: {name} must be a 2-D (N, K) tensor")
            if t.dtype != want:
                raise _lib.LsAmdError(f"matvec_block_axpby: {name} is {t.dtype}, the plan computes in {want}")
            if t.device.type != "cuda":
                raise _lib.LsAmdError(f"matvec_block_axpby: {name} must be a device tensor")
        n = self.reps[0].numel()
        if tuple(x.shape) != tuple(y.shape) or x.shape[0] != n:
            raise _lib.LsAmdError(f"matvec_block_axpby: x {tuple(x.shape)} and y {tuple(y.shape)} must both be ({n}, K)")
        K = int(x.shape[1])
        _lib.check(_lib.load().ls_amd_matvec_block_axpby(self.h, K, C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1),
                                                         C.c_void_p(y.data_ptr()), y.stride(0), y.stride(1), float(alpha), float(beta),
                                                         float(gamma), _dots_ptr(dots, K, "matvec_block_axpby"), _stream_ptr()))
        if check:
            self.check()

    def axpby_kernel(self, K: int) -> str:
        """path matvec_block_axpby takes for K columns on this plan: "k_direct_cheb", "k_pull_gather_cheb" or "epilogue" """
        name = _lib.load().ls_amd_plan_axpby_kernel_name(self.h, int(K))
        if name is None:
            _lib.check(-1)
        return name.decode()

    def matvec_block_axpby_gram(self, x, y, alpha, beta, gamma, gram, check: bool = True):
        """matvec_block_axpby with matrix-valued dots (ls_amd_matvec_block_axpby_gram): the same step on the same path -- y is
        bit-identical to matvec_block_axpby's -- followed by one Gram launch, gram[0] = X^+ X, gram[1] = X^+ Y with the new Y.
        gram: a contiguous device tensor of 2 K K elements of the plan's dtype (e.g. shape (2, K, K)), assigned; it must not
        overlap x or y.  gram_kernel(K) names the form of the Gram launch."""
        torch = _torch()
        who = "matvec_block_axpby_gram"
        if self.P != 1 or self.me >= 0:
            raise _lib.LsAmdError(f"{who}: one-partition plans only (this plan has P = {self.P}, my_partition = {self.me})")
        want = torch.complex128 if self.cplx else torch.float64
        for name, t in (("x", x), ("y", y)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise _lib.LsAmdError(f"{who}: {name} must be a 2-D (N, K) tensor")
            if t.dtype != want:
                raise _lib.LsAmdError(f"{who}: {name} is {t.dtype}, the plan computes in {want}")
            if t.device.type != "cuda":
                raise _lib.LsAmdError(f"{who}: {name} must be a device tensor")
        n = self.reps[0].numel()
        if tuple(x.shape) != tuple(y.shape) or x.shape[0] != n:
            raise _lib.LsAmdError(f"{who}: x {tuple(x.shape)} and y {tuple(y.shape)} must both be ({n}, K)")
        K = int(x.shape[1])
        if not isinstance(gram, torch.Tensor) or gram.device.type != "cuda" or gram.dtype != want or not gram.is_contiguous() \
                or gram.numel() != 2 * K * K:
            raise _lib.LsAmdError(f"{who}: gram must be a contiguous device tensor of 2 K K = {2 * K * K} elements of {want}")
        _lib.check(_lib.load().ls_amd_matvec_block_axpby_gram(self.h, K, C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1),
                                                              C.c_void_p(y.data_ptr()), y.stride(0), y.stride(1), float(alpha), float(beta),
                                                              float(gamma), C.c_void_p(gram.data_ptr()), _stream_ptr()))
        if check:
            self.check()

    def gram_kernel(self, K: int, x=None, y=None) -> str:
        """form of the Gram launch of matvec_block_axpby_gram for K columns: "k_block_gram_mfma" for interleaved blocks (the
        layout assumed when x and y are not given) of K >= 8 columns -- of any K under LS_AMD_GRAM=mfma --, "k_block_gram" for
        narrower blocks, other strides or under LS_AMD_GRAM=valu"""
        K = int(K)
        xs = (K, 1) if x is None else (x.stride(0), x.stride(1))
        ys = (K, 1) if y is None else (y.stride(0), y.stride(1))
        name = _lib.load().ls_amd_block_gram_kernel_name(int(self.cplx), K, xs[0], xs[1], K, ys[0], ys[1])
        if name is None:
            _lib.check(-1)
        return name.decode()

    def matvec_block_axpby_acc(self, x, y, alpha, beta, gamma, z, c, dots=None, check: bool = True):
        """matvec_block_axpby, and Z[:, k] <- Z[:, k] + c Y[:, k] with the new Y where the kernel stores it
        (ls_amd_matvec_block_axpby_acc): one order of the Chebyshev series of e^{-iHt} per call.  z: an (N, K) device tensor with
        strides of its own, of the plan's dtype or complex128 (float64 only with a real c); it must not overlap x or y.  Vectors
        are blocks of one column.  acc_kernel(K) names the path."""
        torch = _torch()
        if self.P != 1 or self.me >= 0:
            raise _lib.LsAmdError(f"matvec_block_axpby_acc: one-partition plans only (this plan has P = {self.P}, my_partition = {self.me})")
        want = torch.complex128 if self.cplx else torch.float64
        (x, y), z, c = _acc_args("matvec_block_axpby_acc", [("x", x), ("y", y)], z, c, want=want)
        n = self.reps[0].numel()
        if x.shape[0] != n:
            raise _lib.LsAmdError(f"matvec_block_axpby_acc: x {tuple(x.shape)}, y and z must all be ({n}, K)")
        K = int(x.shape[1])
        _lib.check(_lib.load().ls_amd_matvec_block_axpby_acc(self.h, K, C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1),
                                                             C.c_void_p(y.data_ptr()), y.stride(0), y.stride(1), float(alpha), float(beta),
                                                             float(gamma), C.c_void_p(z.data_ptr()), z.stride(0), z.stride(1),
                                                             int(z.dtype == torch.complex128), c.real, c.imag,
                                                             _dots_ptr(dots, K, "matvec_block_axpby_acc"), _stream_ptr()))
        if check:
            self.check()

    def acc_kernel(self, K: int) -> str:
        """path matvec_block_axpby_acc takes for K columns on this plan: "epilogue", "k_direct_evolve" / "k_pull_gather_evolve"
        (LS_AMD_ACC=fused) or "k_direct_cheb+k_axpby_acc" / "k_pull_gather_cheb+k_axpby_acc" (split, the default)"""
        name = _lib.load().ls_amd_plan_acc_kernel_name(self.h, int(K))
        if name is None:
            _lib.check(-1)
        return name.decode()

    def matvec_block_series(self, x, z, coefficients, bounds, check: bool = True, work=None):
        """Z <- sum_n c_n T_n((H - b) / a) X for the K columns of the (N, K) device tensors x and z (vectors are blocks of one
        column), a = (hi - lo) / 2, b = (hi + lo) / 2 of bounds = (lo, hi) (ls_amd_matvec_block_series): one accumulate step per
        order, the loop and the growth guard in C.  x: the plan's dtype, any nested strides, left as it was.  z: the plan's dtype or
        complex128 (float64 only with real coefficients), strides of its own, assigned; it must not overlap x.  coefficients: N + 1
        numbers, real or complex.  work: None (the plan allocates two blocks and keeps them), or a contiguous device tensor of
        2 N K elements of the plan's dtype.  Bounds that do not enclose the spectrum raise LsAmdError naming them.
        series_kernel(K) names the path."""
        torch = _torch()
        import numpy as np

        who = "matvec_block_series"
        if self.P != 1 or self.me >= 0:
            raise _lib.LsAmdError(f"{who}: one-partition plans only (this plan has P = {self.P}, my_partition = {self.me})")
        want = torch.complex128 if self.cplx else torch.float64
        (x,), z, _ = _acc_args(who, [("x", x)], z, 0.0, want=want)
        n = self.reps[0].numel()
        if x.shape[0] != n:
            raise _lib.LsAmdError(f"{who}: x {tuple(x.shape)} and z must both be ({n}, K)")
        K = int(x.shape[1])
        c = np.ascontiguousarray(np.asarray(coefficients, dtype=np.complex128).reshape(-1))
        if c.size < 1:
            raise _lib.LsAmdError(f"{who}: no coefficients")
        if z.dtype == torch.float64 and np.any(c.imag != 0.0):
            raise _lib.LsAmdError(f"{who}: z is float64 and the coefficients are not real: the accumulator must be complex128")
        try:
            lo, hi = float(bounds[0]), float(bounds[1])
        except (TypeError, ValueError, IndexError):
            raise _lib.LsAmdError(f"{who}: bounds = {bounds!r}: need finite lo < hi") from None
        wp = None
        if work is not None:
            if not isinstance(work, torch.Tensor) or work.device.type != "cuda" or work.dtype != want or not work.is_contiguous() \
                    or work.numel() < 2 * n * K:
                raise _lib.LsAmdError(f"{who}: work must be a contiguous device tensor of at least {2 * n * K} elements of {want}")
            wp = C.c_void_p(work.data_ptr())
        _lib.check(_lib.load().ls_amd_matvec_block_series(self.h, K, int(c.size) - 1, c.ctypes.data_as(C.c_void_p), lo, hi,
                                                          C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), C.c_void_p(z.data_ptr()),
                                                          z.stride(0), z.stride(1), int(z.dtype == torch.complex128), wp, _stream_ptr()))
        if check:
            self.check()

    def series_kernel(self, K: int) -> str:
        """row path of every order of matvec_block_series for K columns: what axpby_kernel(K) returns"""
        name = _lib.load().ls_amd_plan_series_kernel_name(self.h, int(K))
        if name is None:
            _lib.check(-1)
        return name.decode()

    def check(self):
        _lib.check(_lib.load().ls_amd_plan_check(self.h, _stream_ptr()))

    def inject_fault(self) -> bool:
        """test hook (ls_amd_test_corrupt_plan): the row kernel skips one row from now on; False when the plan has no tile map"""
        return bool(_lib.load().ls_amd_test_corrupt_plan(self.h))

    def enable_timing(self, max_samples: int):
        _lib.check(_lib.load().ls_amd_plan_enable_timing(self.h, max_samples))

    def kernel_times_ms(self, capacity: int = 4096):
        buf = (C.c_float * capacity)()
        n = C.c_int()
        _lib.check(_lib.load().ls_amd_plan_kernel_times(self.h, buf, capacity, C.byref(n)))
        return [float(buf[i]) for i in range(n.value)]

    def enable_stage_timing(self, max_events: int = 65536):
        """the reference's kDisplayTimings (DMV:1028-1052): per-stage device time"""
        _lib.check(_lib.load().ls_amd_plan_enable_stage_timing(self.h, max_events))

    def stage_times(self):
        ms = (C.c_double * 7)()
        calls = (C.c_int64 * 7)()
        mv = C.c_int64()
        _lib.check(_lib.load().ls_amd_plan_stage_times(self.h, ms, calls, C.byref(mv)))
        names = ("localDiagonal", "hashRefresh", "rowKernel", "producers", "exchangeWait", "consumers", "resultsToOwners")
        return {n: (float(ms[i]), int(calls[i])) for i, n in enumerate(names)}, int(mv.value)

    def timing_report(self) -> str:
        buf = C.create_string_buffer(4096)
        _lib.check(_lib.load().ls_amd_plan_timing_report(self.h, buf, 4096))
        return buf.value.decode("utf-8")

    def diag(self, x, y):
        _lib.check(_lib.load().ls_amd_diag(self.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), _stream_ptr()))

    def generate(self, rnd, x, y, send):
        _lib.check(_lib.load().ls_amd_generate(self.h, rnd, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                               C.c_void_p(send.data_ptr() if send is not None else 0), _stream_ptr()))

    def scatter(self, n, betas_ptr: int, vals_ptr: int, y):
        _lib.check(_lib.load().ls_amd_scatter(self.h, n, C.c_void_p(betas_ptr), C.c_void_p(vals_ptr),
                                              C.c_void_p(y.data_ptr()), _stream_ptr()))

    def scatter_round(self, counts, offsets, recv_ptr: int, y):
        """all segments of one round's receive buffer in one launch (ls_amd_scatter_round)"""
        n = len(counts)
        _lib.check(_lib.load().ls_amd_scatter_round(self.h, n, (C.c_int64 * n)(*counts), (C.c_int64 * n)(*offsets), C.c_void_p(recv_ptr),
                                                    C.c_void_p(y.data_ptr()), _stream_ptr()))


class CrossSectorPlan:
    """ls_amd_cross: y = A x between two symmetry sectors (include/ls_amd.h).  operator: A on the SOURCE basis; source_reps /
    target_reps: the ascending representatives of the source basis / of target_basis (device tensors, one partition); x lives on
    the source rows, y on the target rows.  Creation checks that A maps the source sector into the target's (LsAmdError names the
    offending generator otherwise; the check is Operator.mapsSector(target_basis, signs=True)); float64 needs a real operator and
    +-1 characters on both bases.  Spin bases, unprojected fermionic bases, and projected fermionic bases (spinless, spinful with
    spin_flip; up to 60 modes) whose generators are the same on both sides: there the kernel is "k_cross_pull_fermi", which
    projects every image with the permutation signs (always +-1, so they never stand in the way of float64).

    groups: what the two bases' symmetry groups may be (ls_amd_cross_create_groups).
      "same" (default)  the same generator permutations in the same order; everything above.
      "restrict"        the target group is a subgroup of the source group and A is covariant under the target's generators
                        (Operator.mapsSector(target_basis, subgroup=True)): S^z_q from a ground state found with reflection and
                        spin inversion into the translations-only sector k + q.  Host work only: the same kernels, to_csr works.
                        A target without symmetries is always admitted (y = A B1 x on the plain basis).
      "project"         any two bases of one particle type and number_sites and ANY operator, no covariance check: y is the
                        component of A B1 x in the target sector, B2^+ A B1 x (sigma^z_0, c^+_0, a local quench; A = 1 moves a
                        state between the sectors of two groups).  The kernel is "k_cross_project" ("k_cross_project_fermi"); the
                        cost is |G2| times (2 |G2| with a target inversion) that of "restrict"; nnz counts the packets gathered
                        per apply; to_csr is refused."""

    GROUPS = {"same": 0, "restrict": 1, "project": 2}

    def __init__(self, operator: Operator, source_reps, target_basis: Basis, target_reps, dtype, groups: str = "same"):
        torch = _torch()
        _lib.require_device()
        for name, t in (("source_reps", source_reps), ("target_reps", target_reps)):
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.int64 or t.device.type != "cuda" or not t.is_contiguous():
                raise LsAmdError(f"CrossSectorPlan: {name} must be a contiguous 1-D int64 device tensor (one partition)")
        self.operator, self.target_basis = operator, target_basis
        self.source_reps, self.target_reps = source_reps, target_reps  # borrowed by the plan: keep alive
        self.cplx = dtype in (torch.complex128, "c128")
        if not self.cplx and dtype not in (torch.float64, "f64"):
            raise LsAmdError(f"CrossSectorPlan: dtype {dtype} is neither float64 nor complex128")
        self.dtype = torch.complex128 if self.cplx else torch.float64
        if groups not in self.GROUPS:
            raise LsAmdError(f"CrossSectorPlan: groups = {groups!r} is none of 'same', 'restrict', 'project'")
        self.groups = groups
        h = C.c_void_p()
        L = _lib.load()
        tail = (C.c_void_p(source_reps.data_ptr()), source_reps.numel(), C.c_void_p(target_reps.data_ptr()), target_reps.numel(), _stream_ptr())
        if groups == "same":
            _lib.check(L.ls_amd_cross_create(C.byref(h), operator.payload, target_basis.payload, 1 if self.cplx else 0, *tail))
        else:
            _lib.check(L.ls_amd_cross_create_groups(C.byref(h), operator.payload, target_basis.payload, 1 if self.cplx else 0,
                                                    self.GROUPS[groups], *tail))
        self.h = h

    def destroy(self):
        if getattr(self, "h", None):
            _lib.load().ls_amd_cross_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    @property
    def kernel(self): return _lib.load().ls_amd_cross_kernel_name(self.h).decode()
    @property
    def nnz(self): return int(_lib.load().ls_amd_cross_nnz(self.h))
    @property
    def n_src(self): return int(self.source_reps.numel())
    @property
    def n_dst(self): return int(self.target_reps.numel())

    def _vector(self, name, t, n):
        torch = _torch()
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise LsAmdError(f"CrossSectorPlan.apply: {name} must be a device tensor")
        if t.dtype != self.dtype:
            raise LsAmdError(f"CrossSectorPlan.apply: {name} is {t.dtype}, the plan computes in {self.dtype}")
        if t.dim() not in (1, 2) or t.shape[0] != n:
            raise LsAmdError(f"CrossSectorPlan.apply: {name} {tuple(t.shape)} must have {n} rows")

    def apply(self, x, y, check: bool = True):
        """y <- A x: x of n_src, y of n_dst elements (y is assigned); (n_src, K) and (n_dst, K) blocks are a loop over the columns"""
        self._vector("x", x, self.n_src)
        self._vector("y", y, self.n_dst)
        if x.dim() != y.dim() or (x.dim() == 2 and x.shape[1] != y.shape[1]):
            raise LsAmdError(f"CrossSectorPlan.apply: x {tuple(x.shape)} and y {tuple(y.shape)} must both be vectors or both have K columns")
        L = _lib.load()
        if x.dim() == 1:
            xc = x if x.is_contiguous() else x.contiguous()
            yc = y if y.is_contiguous() else _torch().empty_like(y, memory_format=_torch().contiguous_format)
            _lib.check(L.ls_amd_cross_apply(self.h, C.c_void_p(xc.data_ptr()), C.c_void_p(yc.data_ptr()), _stream_ptr()))
            if yc is not y:
                y.copy_(yc)
        else:
            for k in range(int(x.shape[1])):
                xc = x[:, k].contiguous()
                yc = _torch().empty(self.n_dst, dtype=self.dtype, device=y.device)
                _lib.check(L.ls_amd_cross_apply(self.h, C.c_void_p(xc.data_ptr()), C.c_void_p(yc.data_ptr()), _stream_ptr()))
                y[:, k].copy_(yc)
        if check:
            self.check()

    BLOCK_METHODS = {None: 0, "columns": 1, "kernel": 2}  # LS_AMD_CROSS_BLOCK_AUTO | _COLUMNS | _KERNEL

    @classmethod
    def _block_path(cls, who, method):
        if not isinstance(method, (str, type(None))) or method not in cls.BLOCK_METHODS:
            raise ValueError(f"CrossSectorPlan.{who}: method = {method!r} is none of None (LS_AMD_CROSS_PROJECT_BLOCK, else 'columns'), "
                             "'columns', 'kernel'")
        return cls.BLOCK_METHODS[method]

    def apply_block(self, x, y, check: bool = True, method=None):
        """Y[:, k] <- A X[:, k] for the K columns of the (n_src, K) and (n_dst, K) device tensors x and y (ls_amd_cross_apply_block):
        any strides -- (K, 1) interleaved is the fast layout, a transposed (K, n) tensor the column-major one -- and the plan's
        dtype; 1 <= K <= 64; y is assigned; x and y must not overlap.  Stages A and B1 and the look-up of the images run once per
        chunk of 8 columns instead of once per column; block_kernel(K) names the path.  method chooses the
        path of a groups="project" plan: "columns" loops apply over the columns (byte for byte K applies), "kernel" runs the block
        form k_cross_project_blk (the target's element loop once per chunk of 8 columns, a fixed order of summation), None follows
        LS_AMD_CROSS_PROJECT_BLOCK=columns|kernel (unset: columns).  The argument wins over the environment; the other plans have one
        block kernel whatever it says.  ValueError for any other value, before any device work."""
        path = self._block_path("apply_block", method)
        torch = _torch()
        for name, t in (("x", x), ("y", y)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise LsAmdError(f"apply_block: {name} must be a 2-D (n, K) tensor")
            if t.dtype != self.dtype:
                raise LsAmdError(f"apply_block: {name} is {t.dtype}, the plan computes in {self.dtype}")
            if t.device.type != "cuda":
                raise LsAmdError(f"apply_block: {name} must be a device tensor")
        if x.shape[0] != self.n_src or y.shape[0] != self.n_dst or x.shape[1] != y.shape[1]:
            raise LsAmdError(f"apply_block: x {tuple(x.shape)} must be ({self.n_src}, K) and y {tuple(y.shape)} ({self.n_dst}, K)")
        K = int(x.shape[1])
        _lib.check(_lib.load().ls_amd_cross_apply_block_path(self.h, path, K, C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1),
                                                             C.c_void_p(y.data_ptr()), y.stride(0), y.stride(1), _stream_ptr()))
        if check:
            self.check()

    def block_kernel(self, K: int, method=None) -> str:
        """path a block of K columns takes on this plan: "k_cross_pull_blk", "k_cross_pull_blk_fermi"; groups="project": "columns", or
        "k_cross_project_blk[_fermi]" with method="kernel" (None: LS_AMD_CROSS_PROJECT_BLOCK, as in apply_block)"""
        path = self._block_path("block_kernel", method)
        name = _lib.load().ls_amd_cross_block_kernel_name_path(self.h, path, int(K))
        if name is None:
            _lib.check(-1)
        return name.decode()

    def check(self):
        _lib.check(_lib.load().ls_amd_cross_check(self.h, _stream_ptr()))

    @property
    def csr_bytes(self) -> int:
        """upper bound of the peak device bytes of to_csr (ls_amd_cross_csr_bytes; host only)"""
        return int(_lib.load().ls_amd_cross_csr_bytes(self.h))

    def to_csr(self, max_bytes: int = 8 << 30) -> CsrMatrix:
        """the matrix apply multiplies by, (n_dst, n_src), as canonical CSR on the device (ls_amd_cross_csr): built in O(nnz) by the
        plan's own kernel in an emitting mode; the images of a row that meet in one source state are summed, sums that cancel are
        dropped (so nnz <= self.nnz); two exports are bitwise equal.  LsAmdError when csr_bytes exceeds max_bytes (nothing is
        allocated), or when an image lies outside the source basis (the error of check())."""
        torch = _torch()
        L = _lib.load()
        m = _lib.LsAmdCsr()
        _lib.check(L.ls_amd_cross_csr(self.h, int(max_bytes), C.byref(m), _stream_ptr()))
        try:
            # (copies; _adopt frees the library's array whatever happens)
            ptrs = [(m.d_row_ptr, m.rows + 1, torch.int64), (m.d_col, m.nnz, torch.int64), (m.d_val, m.nnz, self.dtype)]
            m.d_row_ptr = m.d_col = m.d_val = None
            out = []
            for k, (ptr, count, dt) in enumerate(ptrs):
                ptrs[k] = None
                out.append(_adopt(ptr, int(count), dt))
        finally:
            for rest in ptrs:
                if rest is not None and rest[0]:
                    L.ls_amd_free(C.c_void_p(rest[0]))
        return CsrMatrix((int(m.rows), int(m.cols)), out[0], out[1], out[2])


class _BorrowedPlan(MatvecPlan):
    """view of a plan owned by another object (ls_amd_dist): same accessors, no destroy."""

    def __init__(self, handle, owner, P, me):  # noqa: super().__init__ deliberately not called
        self.h, self.owner, self.P, self.me = handle, owner, P, me

    def destroy(self):
        self.h = None


class Communicator:
    """ls_amd_comm: RCCL communicator owned by the C host (include/ls_amd.h).  rank == locale index."""

    def __init__(self, size: int, rank: int, unique_id: bytes):
        _lib.require_device()
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _lib.check(_lib.load().ls_amd_comm_create(C.byref(h), size, rank, buf))
        self.h, self.size, self.rank = h, size, rank

    @staticmethod
    def local_group(size: int):
        """`size` loop-back communicators in this process (one per host thread): the multi-rank logic of the C host on a
        one-GPU box, where RCCL refuses more than one rank per device (test infrastructure)"""
        _lib.require_device()
        arr = (C.c_void_p * size)()
        _lib.check(_lib.load().ls_amd_comm_create_local(arr, size))
        out = []
        for r in range(size):
            c = Communicator.__new__(Communicator)
            c.h, c.size, c.rank = C.c_void_p(arr[r]), size, r
            out.append(c)
        return out

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _lib.check(_lib.load().ls_amd_comm_unique_id(buf))
        return buf.raw

    @staticmethod
    def from_torch(group=None) -> "Communicator":
        """bootstrap through an existing torch.distributed group (any backend): rank 0 creates the id,
        the group's object broadcast carries it -- the role MPI_Bcast plays for a C caller."""
        import torch.distributed as dist

        rank, size = dist.get_rank(group), dist.get_world_size(group)
        box = [Communicator.unique_id() if rank == 0 else None]
        if size > 1:
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return Communicator(size, rank, box[0])

    def wait(self, timeout_s: float = 0.0):
        """ls_amd_comm_wait: until the current stream and the exchange stream have drained; raises after timeout_s (<= 0: the
        watchdog's deadline, LS_AMD_COMM_WATCHDOG_S) instead of hanging in a synchronisation"""
        _lib.check(_lib.load().ls_amd_comm_wait(self.h, _stream_ptr(), float(timeout_s)))

    def rccl_count(self) -> int:
        """the communicator size as RCCL reports it (ncclCommCount); 0 for a loop-back group"""
        return int(_lib.load().ls_amd_comm_rccl_count(self.h))

    def set_default(self):
        """the communicator of primmeGlobalSumReal / primmeBroadcastReal / ls_chpl_primme_matvec"""
        _lib.load().ls_amd_set_default_comm(self.h)

    def allreduce_sum(self, t):
        torch = _torch()
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous()
        _lib.check(_lib.load().ls_amd_comm_allreduce_sum_f64(self.h, C.c_void_p(t.data_ptr()), t.numel(), _stream_ptr()))
        return t

    def allreduce_max(self, t):
        torch = _torch()
        assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous()
        _lib.check(_lib.load().ls_amd_comm_allreduce_max_i64(self.h, C.c_void_p(t.data_ptr()), t.numel(), _stream_ptr()))
        return t

    def broadcast(self, t, root: int = 0):
        assert t.is_cuda and t.is_contiguous()
        _lib.check(_lib.load().ls_amd_comm_broadcast(self.h, C.c_void_p(t.data_ptr()), t.numel() * t.element_size(), root,
                                                     _stream_ptr()))
        return t

    def destroy(self):
        if getattr(self, "h", None):
            L = _lib.load()
            if L.ls_amd_default_comm() == self.h.value:
                L.ls_amd_set_default_comm(None)
            L.ls_amd_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class DistMatvec:
    """ls_amd_dist: matrixVectorProduct for this rank's block, exchange inside the C host (RCCL)."""

    def __init__(self, comm: Communicator, matrix: Operator, representatives, dtype, num_rounds: int = 0):
        torch = _torch()
        _lib.require_device()
        self.comm, self.matrix, self.reps = comm, matrix, representatives  # borrowed by the C object: keep alive
        self.cplx = dtype in (torch.complex128, "c128")
        h = C.c_void_p()
        _lib.check(_lib.load().ls_amd_dist_create(C.byref(h), comm.h, matrix.payload, 1 if self.cplx else 0,
                                                  C.c_void_p(representatives.data_ptr()), representatives.numel(),
                                                  num_rounds, _stream_ptr()))
        self.h = h
        self.plan = _BorrowedPlan(C.c_void_p(_lib.load().ls_amd_dist_plan(h)), self, comm.size, comm.rank)

    @property
    def num_rounds(self): return int(_lib.load().ls_amd_dist_num_rounds(self.h))
    @property
    def exchange_bytes(self): return int(_lib.load().ls_amd_dist_exchange_bytes(self.h))

    def matvec(self, x, y, check: bool = True):
        _lib.check(_lib.load().ls_amd_dist_matvec(self.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), _stream_ptr()))
        if check:
            self.plan.check()

    def inject_fault(self) -> bool:
        """test hook (ls_amd_test_corrupt_dist): misplace one received segment; False when this rank receives none"""
        return bool(_lib.load().ls_amd_test_corrupt_dist(self.h))

    def destroy(self):
        if getattr(self, "h", None):
            self.plan.destroy()
            _lib.load().ls_amd_dist_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class ReplMatvec:
    """ls_amd_repl: matrixVectorProduct for this rank's block with the replicated-x exchange inside the C host (RCCL)."""

    def __init__(self, comm: Communicator, matrix: Operator, reps_global, masks, dtype):
        torch = _torch()
        _lib.require_device()
        self.comm, self.matrix, self.reps_global, self.masks = comm, matrix, reps_global, masks  # borrowed: keep alive
        self.cplx = dtype in (torch.complex128, "c128")
        assert masks.dtype == torch.uint8 and masks.is_cuda and masks.numel() == reps_global.numel()
        h = C.c_void_p()
        _lib.check(_lib.load().ls_amd_repl_create(C.byref(h), comm.h, matrix.payload, 1 if self.cplx else 0,
                                                  C.c_void_p(reps_global.data_ptr()), C.c_void_p(masks.data_ptr()),
                                                  reps_global.numel(), _stream_ptr()))
        self.h = h
        self.plan = _BorrowedPlan(C.c_void_p(_lib.load().ls_amd_repl_plan(h)), self, comm.size, comm.rank)

    @property
    def exchange_bytes(self): return int(_lib.load().ls_amd_repl_exchange_bytes(self.h))
    @property
    def x_in_bytes(self): return int(_lib.load().ls_amd_repl_x_in_bytes(self.h))

    def matvec(self, x, y, check: bool = True):
        _lib.check(_lib.load().ls_amd_repl_matvec(self.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), _stream_ptr()))
        if check:
            self.plan.check()

    def inject_fault(self) -> bool:
        """test hook (ls_amd_test_corrupt_repl): this rank's own rows come back one element late"""
        return bool(_lib.load().ls_amd_test_corrupt_repl(self.h))

    def destroy(self):
        if getattr(self, "h", None):
            self.plan.destroy()
            _lib.load().ls_amd_repl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def fillRandom(states, seed: int, dtype):
    """deterministic vector keyed by the basis states (same logical vector for every partitioning)."""
    torch = _torch()
    _lib.require_device()
    out = torch.empty(states.numel(), dtype=dtype, device=states.device)
    _lib.check(_lib.load().ls_amd_fill_random(states.numel(), C.c_void_p(states.data_ptr()), C.c_uint64(seed),
                                              1 if dtype == torch.complex128 else 0, C.c_void_p(out.data_ptr()), _stream_ptr()))
    return out


class ReplicatedPlan:
    """ls_amd replicated-x plan: this process owns partition `my_partition`'s rows and is handed the
    whole x in global ascending order (include/ls_amd.h)."""

    def __init__(self, matrix: "Operator", reps_local, reps_global, dtype, num_partitions: int, my_partition: int):
        torch = _torch()
        _lib.require_device()
        self.matrix, self.reps_local, self.reps_global = matrix, reps_local, reps_global
        self.cplx = dtype in (torch.complex128, "c128")
        h = C.c_void_p()
        _lib.check(_lib.load().ls_amd_plan_create_replicated(
            C.byref(h), matrix.payload, 1 if self.cplx else 0, num_partitions, my_partition,
            C.c_void_p(reps_local.data_ptr()), reps_local.numel(), C.c_void_p(reps_global.data_ptr()), reps_global.numel(),
            _stream_ptr()))
        self.h = h

    destroy = MatvecPlan.destroy
    __del__ = MatvecPlan.__del__
    kernel = MatvecPlan.kernel
    check = MatvecPlan.check
    enable_timing = MatvecPlan.enable_timing
    kernel_times_ms = MatvecPlan.kernel_times_ms
    enable_stage_timing = MatvecPlan.enable_stage_timing
    stage_times = MatvecPlan.stage_times
    timing_report = MatvecPlan.timing_report

    def matvec(self, x_global, y_local, check: bool = True):
        _lib.check(_lib.load().ls_amd_matvec_replicated(self.h, C.c_void_p(x_global.data_ptr()), C.c_void_p(y_local.data_ptr()), _stream_ptr()))
        if check:
            self.check()


def _plan_for(matrix: Operator, representatives, dtype, mode="auto"):
    key = (tuple(int(r.data_ptr()) for r in representatives), tuple(int(r.numel()) for r in representatives), str(dtype), mode)
    pl = matrix._plans.pop(key, None)
    if pl is None:
        # a plan pins its representative tensors and device tables (hash table, norms, tile map, partner-rank cache:
        # several GB for the large chains): keep only the two most recently used ones per operator
        while len(matrix._plans) >= 2:
            oldest = next(iter(matrix._plans))
            matrix._plans.pop(oldest).destroy()
        pl = MatvecPlan(matrix, representatives, dtype, mode=mode)
    matrix._plans[key] = pl  # (re)inserted last: dicts keep insertion order = LRU order
    return pl


def matrixVectorProduct(matrix: Operator, x, y, representatives, mode: str = "auto", check: bool = True):
    """matrixVectorProduct(matrix, x, y, representatives) (DMV:1072-1093) with all locales as logical
    partitions on the current device.  x, y, representatives: lists with one device tensor per
    locale (f64 or c128; representatives int64-viewed uint64).  y is overwritten by the diagonal
    pass when the operator has diagonal terms, then accumulated into."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        x, y, representatives = [x], [y], [representatives]
    if len(x) != len(representatives) or len(y) != len(representatives):
        raise LsAmdError("x, y and representatives must have one block per locale")
    for a, b, r in zip(x, y, representatives):
        if a.dtype != b.dtype or a.numel() != r.numel() or b.numel() != r.numel():
            raise LsAmdError("block shapes / dtypes do not match")
    pl = _plan_for(matrix, representatives, x[0].dtype, mode)
    pl.matvec(x, y, check=check)
    return pl


def localMatrixVector(matrix: Operator, x, y, representatives, mode: str = "auto"):
    """localMatrixVector (DMV:1055-1070): the single-locale case."""
    return matrixVectorProduct(matrix, [x], [y], [representatives], mode=mode)
