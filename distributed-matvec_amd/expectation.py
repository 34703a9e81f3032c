"""Expectation values of arbitrary operators on a sector state in one pass (include/ls_amd.h: ls_amd_expect; csrc/k_expect.hip,
k_expect_fermi.hip).

The operators need not be invariant under the sector's group and may act on any number of sites: dimer-dimer correlations
<(S_i.S_j)(S_k.S_l)>, scalar chirality S_i.(S_j x S_k), pair correlations <Delta+_i Delta_j>, four-point functions
<c+_i c+_j c_k c_l>.  With R[A] = sum_r conj(psi_r) / n(r) (A psi^)(r) over the representatives alone (psi^ as in correlations.py),
    <psi|O|psi> = |G|^-1 sum_g R[U_g O U_g^-1]
for every O and every sector.  The host conjugates every term of every operator by every group element (on projected fermionic bases
with the permutation signs of the Fock states), keeps the unique terms of the whole batch, and the device evaluates R of each of them in
one pass: the image of a row under a flip mask is projected and looked up once and shared by all terms with that mask.  An image that
leaves the conserved numbers of the basis (sigma^x on a fixed-weight basis, a lone c+) contributes exactly zero.  No floating-point
atomics: two calls on the same input return the same bytes.  ONE partition; one state per call of values, a block of up to 64 states
per call of values_block (k_expect_blk: the images are projected and looked up once per chunk of 8 columns);
nothing falls back to the CPU.

The same identity holds between two states phi, psi of ONE sector (both transform with the same character), with
R[A](phi, psi) = sum_r conj(phi_r) / n(r) (A psi^)(r): matrix_elements gives <phi_a|O_k|psi_b> for every column of a bra block and
every column of a ket block in one pass (k_expect_mat: one chunk of 8 bra x 8 ket columns shares the images),
eigenstate_matrix_elements the matrices of the operators between the eigenstates of a sector."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib, config
from ._lib import LsAmdError
from .correlations import _normalised
from .entanglement import _complex_characters, _stream_ptr

__all__ = ["ExpectationPlan", "expectation_values", "expectation_values_block", "matrix_elements", "eigenstate_matrix_elements",
           "dimer_correlations", "pair_correlations", "expectation"]

_MATRIX_METHODS = ("auto", "kernel", "polarisation")

_PARTICLE_NAMES = {v: k for k, v in config.PARTICLES.items()}


def _spec_of(basis):
    """what config.parse_operator needs to know of a basis: its particle type and its number of sites"""
    if getattr(basis, "spec", None) is not None:
        return basis.spec
    return config.BasisSpec(number_sites=basis.numberSites(), particle=_PARTICLE_NAMES[basis.particleType()])


def _as_operator(basis, item, k):
    from .api import Operator

    if isinstance(item, Operator):
        return item
    if isinstance(item, config.OperatorSpec):
        return Operator.fromSpec(basis, item)
    if isinstance(item, dict) and "terms" in item:
        return Operator.fromSpec(basis, config.parse_operator(item, _spec_of(basis)))
    raise LsAmdError(f"ExpectationPlan: operator {k} is {type(item).__name__}: neither an Operator, an OperatorSpec nor an operator "
                     "section {'terms': [{'expression': ..., 'sites': ...}]}")


class ExpectationPlan:
    """ls_amd_expect: the plan of the expectation values of `operators` -- Operators on `basis`, config.OperatorSpecs, or operator
    sections {"terms": [{"expression": ..., "sites": ...}]} in the language of the basis's particle type -- in vectors on `reps` (the
    ascending representatives of `basis`, a 1-D int64 device tensor, one partition).  psi is taken as it is."""

    def __init__(self, basis, reps, operators):
        import torch

        if isinstance(reps, (list, tuple)):
            if len(reps) != 1:
                raise LsAmdError(f"ExpectationPlan: one partition (the whole sector on this device), got {len(reps)} blocks of representatives")
            reps = reps[0]
        if not isinstance(reps, torch.Tensor) or reps.dim() != 1 or reps.dtype != torch.int64 or not reps.is_contiguous():
            raise LsAmdError("ExpectationPlan: reps must be a contiguous 1-D int64 device tensor (one partition)")
        operators = list(operators) if not isinstance(operators, (dict, config.OperatorSpec)) and hasattr(operators, "__iter__") else [operators]
        if not operators:
            raise LsAmdError("ExpectationPlan: no operators")
        ops = [_as_operator(basis, item, k) for k, item in enumerate(operators)]  # (only their term tables are read, at creation)
        _lib.require_device()
        if reps.device.type != "cuda":
            raise LsAmdError("ExpectationPlan: reps must be a device tensor")
        self.basis, self.reps = basis, reps  # borrowed by the plan: keep alive
        self.complex_characters = _complex_characters(basis)
        self.count = len(ops)
        L = _lib.load()
        arr = (type(ops[0].payload) * len(ops))(*[op.payload for op in ops])
        h = C.c_void_p()
        _lib.check(L.ls_amd_expect_create(C.byref(h), basis.payload, arr, len(ops), C.c_void_p(reps.data_ptr()), reps.numel(), _stream_ptr()))
        self.h = h
        self.num_terms = int(L.ls_amd_expect_num_terms(h))
        self.num_groups = int(L.ls_amd_expect_num_groups(h))

    def destroy(self):
        if getattr(self, "h", None):
            _lib.load().ls_amd_expect_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def kernel(self):
        name = _lib.load().ls_amd_expect_kernel_name(self.h)
        if name is None:
            _lib.check(-1)
        return name.decode()

    def _psi(self, who, psi):
        import torch

        n = int(self.reps.numel())
        if self.h is None:
            raise LsAmdError(f"ExpectationPlan.{who}: the plan was destroyed")
        if not isinstance(psi, torch.Tensor) or psi.device.type != "cuda":
            raise LsAmdError(f"ExpectationPlan.{who}: psi must be a device tensor (there is no CPU path)")
        if psi.dim() != 1 or psi.numel() != n:
            raise LsAmdError(f"ExpectationPlan.{who}: psi {tuple(psi.shape)} must be ONE vector of {n} elements")
        if psi.dtype not in (torch.float64, torch.complex128):
            raise LsAmdError(f"ExpectationPlan.{who}: psi is {psi.dtype}, neither float64 nor complex128")
        if psi.dtype == torch.float64 and self.complex_characters:
            psi = psi.to(torch.complex128)
        psi = psi if psi.is_contiguous() else psi.contiguous()
        return psi, (1 if psi.dtype == torch.complex128 else 0)

    def values(self, psi):
        """-> numpy complex128 (K,): <psi|O_k|psi> of every operator of the plan"""
        psi, dt = self._psi("values", psi)
        out = np.zeros(self.count, dtype=np.complex128)
        _lib.check(_lib.load().ls_amd_expect_values(self.h, dt, C.c_void_p(psi.data_ptr()), out.view(np.float64).ctypes.data_as(_lib.c_f64p),
                                                    _stream_ptr()))
        return out

    def block_kernel(self, K):
        """the path values_block takes for a block of K columns: "k_expect_blk", "k_expect_blk_fermi", or "columns" (the loop over
        values, LS_AMD_EXPECT_BLOCK=columns)"""
        if self.h is None:
            raise LsAmdError("ExpectationPlan.block_kernel: the plan was destroyed")
        name = _lib.load().ls_amd_expect_block_kernel_name(self.h, int(K))
        if name is None:
            _lib.check(-1)
        return name.decode()

    def values_block(self, psi):
        """-> numpy complex128 (n_ops, K): <psi_c|O_k|psi_c> of every operator of the plan for the K columns, 1 <= K <= 64, of the
        (n, K) device tensor psi (any strides, float64 or complex128) in one pass: the images, their projection and their look-up
        are shared by a chunk of 8 columns.  The columns are taken as they are."""
        import torch

        who, n = "values_block", int(self.reps.numel())
        if self.h is None:
            raise LsAmdError(f"ExpectationPlan.{who}: the plan was destroyed")
        if not isinstance(psi, torch.Tensor) or psi.device.type != "cuda":
            raise LsAmdError(f"ExpectationPlan.{who}: psi must be a device tensor (there is no CPU path)")
        if psi.dim() != 2:
            raise LsAmdError(f"ExpectationPlan.{who}: psi {tuple(psi.shape)} must be a 2-D block (n, K); one vector goes through values")
        if psi.shape[0] != n:
            raise LsAmdError(f"ExpectationPlan.{who}: psi {tuple(psi.shape)} must have {n} rows")
        K = int(psi.shape[1])
        if K < 1 or K > 64:
            raise LsAmdError(f"ExpectationPlan.{who}: K = {K} columns, outside [1, 64]")
        if psi.dtype not in (torch.float64, torch.complex128):
            raise LsAmdError(f"ExpectationPlan.{who}: psi is {psi.dtype}, neither float64 nor complex128")
        if psi.dtype == torch.float64 and self.complex_characters:
            psi = psi.to(torch.complex128)
        rs, cs = (int(s) for s in psi.stride())
        if K == 1:
            cs = 1
        if n == 1:
            rs = max(rs, K * cs)
        if rs <= 0 or cs <= 0 or not (rs >= K * cs or cs >= n * rs):  # (expanded or overlapping views)
            psi = psi.contiguous()
            rs, cs = K, 1
        out = np.zeros((self.count, K), dtype=np.complex128)
        _lib.check(_lib.load().ls_amd_expect_values_block(self.h, 1 if psi.dtype == torch.complex128 else 0, K, C.c_void_p(psi.data_ptr()), rs, cs,
                                                          out.view(np.float64).ctypes.data_as(_lib.c_f64p), _stream_ptr()))
        return out

    def _matrix_method(self, who, method):
        """the route of matrix_elements: the argument, else LS_AMD_EXPECT_MATRIX (read at every call), else auto; auto is the kernel
        ("Matrix elements between blocks")"""
        if self.h is None:
            raise LsAmdError(f"ExpectationPlan.{who}: the plan was destroyed")
        if method is None:
            method = os.environ.get("LS_AMD_EXPECT_MATRIX") or "auto"
        if method not in _MATRIX_METHODS:
            raise LsAmdError(f"ExpectationPlan.{who}: method {method!r} (argument or LS_AMD_EXPECT_MATRIX) is none of {', '.join(_MATRIX_METHODS)}")
        return "kernel" if method == "auto" else method

    def matrix_kernel(self, Ka, Kb, method=None):
        """the path matrix_elements takes for Ka bra and Kb ket columns: "k_expect_mat", "k_expect_mat_fermi", or "polarisation"
        (four values_block columns per element; method or LS_AMD_EXPECT_MATRIX=polarisation)"""
        route = self._matrix_method("matrix_kernel", method)
        name = _lib.load().ls_amd_expect_matrix_kernel_name(self.h, int(Ka), int(Kb))
        if name is None:
            _lib.check(-1)
        return "polarisation" if route == "polarisation" else name.decode()

    def _matrix_block(self, name, x):
        """a bra or ket block as matrix_elements takes it: a 1-D vector is one column; validated as values_block validates psi"""
        import torch

        who, n = "matrix_elements", int(self.reps.numel())
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise LsAmdError(f"ExpectationPlan.{who}: {name} must be a device tensor (there is no CPU path)")
        if x.dim() == 1:
            x = x.unsqueeze(1)
        if x.dim() != 2:
            raise LsAmdError(f"ExpectationPlan.{who}: {name} {tuple(x.shape)} must be a vector (n,) or a 2-D block (n, K)")
        if x.shape[0] != n:
            raise LsAmdError(f"ExpectationPlan.{who}: {name} {tuple(x.shape)} must have {n} rows")
        K = int(x.shape[1])
        if K < 1 or K > 64:
            raise LsAmdError(f"ExpectationPlan.{who}: {name} has K = {K} columns, outside [1, 64]")
        if x.dtype not in (torch.float64, torch.complex128):
            raise LsAmdError(f"ExpectationPlan.{who}: {name} is {x.dtype}, neither float64 nor complex128")
        return x

    @staticmethod
    def _strides(x):
        """(block, row stride, column stride) with the strides ls_amd takes; expanded or overlapping views are made contiguous"""
        n, K = (int(s) for s in x.shape)
        rs, cs = (int(s) for s in x.stride())
        if K == 1:
            cs = 1
        if n == 1:
            rs = max(rs, K * cs)
        if rs <= 0 or cs <= 0 or not (rs >= K * cs or cs >= n * rs):
            x = x.contiguous()
            rs, cs = K, 1
        return x, rs, cs

    def matrix_elements(self, bra, ket=None, method=None):
        """-> numpy complex128 (n_ops, Ka, Kb): <bra_a|O_k|ket_b> of every operator of the plan between the Ka columns of bra and
        the Kb columns of ket (ket None: ket = bra), 1 <= Ka, Kb <= 64 -- device tensors (n,) or (n, K) with any strides, float64 or
        complex128; both are promoted to complex128 when either is complex or the characters of the sector are.  The bra is
        conjugated, the operator acts on the ket; the columns are taken as they are.  method (else LS_AMD_EXPECT_MATRIX, else auto):
        "kernel" is k_expect_mat in one pass (the images, their projection and their look-up shared by 8 bra x 8 ket columns),
        "polarisation" four values_block columns per element (the independent check), "auto" the kernel."""
        import torch

        route = self._matrix_method("matrix_elements", method)
        same = ket is None
        bra = self._matrix_block("bra", bra)
        ket = bra if same else self._matrix_block("ket", ket)
        if self.complex_characters or bra.dtype == torch.complex128 or ket.dtype == torch.complex128:
            bra = bra.to(torch.complex128)
            ket = bra if same else ket.to(torch.complex128)
        Ka, Kb = int(bra.shape[1]), int(ket.shape[1])
        if route == "polarisation":
            return self._matrix_polarisation(bra, ket)
        bra, ars, acs = self._strides(bra)
        ket, krs, kcs = (bra, ars, acs) if same else self._strides(ket)
        out = np.zeros((self.count, Ka, Kb), dtype=np.complex128)
        _lib.check(_lib.load().ls_amd_expect_matrix_elements(self.h, 1 if bra.dtype == torch.complex128 else 0, Ka, C.c_void_p(bra.data_ptr()),
                                                             ars, acs, Kb, C.c_void_p(ket.data_ptr()), krs, kcs,
                                                             out.view(np.float64).ctypes.data_as(_lib.c_f64p), _stream_ptr()))
        return out

    def _matrix_polarisation(self, bra, ket):
        """<phi|O|psi> = (E(phi + psi) - E(phi - psi) - i E(phi + i psi) + i E(phi - i psi)) / 4 with E(chi) = <chi|O|chi> from the
        unchanged values_block: four complex128 columns per element, at most 64 columns (16 elements) per call"""
        import torch

        bra, ket = bra.to(torch.complex128), ket.to(torch.complex128)
        Ka, Kb = int(bra.shape[1]), int(ket.shape[1])
        out = np.zeros((self.count, Ka * Kb), dtype=np.complex128)
        ia = torch.arange(Ka, device=bra.device).repeat_interleave(Kb)
        ib = torch.arange(Kb, device=bra.device).repeat(Ka)
        for p0 in range(0, Ka * Kb, 16):
            phi, psi = bra[:, ia[p0:p0 + 16]], ket[:, ib[p0:p0 + 16]]
            m = int(phi.shape[1])
            E = self.values_block(torch.cat([phi + psi, phi - psi, phi + 1j * psi, phi - 1j * psi], dim=1))
            out[:, p0:p0 + m] = 0.25 * (E[:, :m] - E[:, m:2 * m] - 1j * E[:, 2 * m:3 * m] + 1j * E[:, 3 * m:])
        return out.reshape(self.count, Ka, Kb)


def _normalised_columns(x):
    import torch

    if isinstance(x, torch.Tensor) and x.dim() in (1, 2) and x.numel():
        nrm = torch.linalg.vector_norm(x, dim=0)
        x = x / torch.where(nrm > 0, nrm, torch.ones_like(nrm))
    return x


def matrix_elements(basis, reps, bra, ket, operators):
    """<bra_a|O_k|ket_b> between every normalised column of bra and every normalised column of ket (ket None: ket = bra) for every
    operator (what ExpectationPlan accepts), through one plan and one pass -> complex128 (n_ops, Ka, Kb)"""
    pl = ExpectationPlan(basis, reps, operators)
    try:
        bra = _normalised_columns(bra)
        return pl.matrix_elements(bra, None if ket is None else _normalised_columns(ket))
    finally:
        pl.destroy()


def eigenstate_matrix_elements(config_, operators, states=None, max_dim: int = 32768, max_bytes: int = 1 << 30):
    """<m|O_k|n> of every operator (what ExpectationPlan accepts) between the eigenstates of the configured Hamiltonian (dict or YAML
    path) on its sector -> (energies (m,), complex128 (n_ops, m, m)): diagonalize.full_spectrum(config, eigenvectors=True), the
    eigenvectors `states` selects (a slice or an array of indices into the ascending spectrum; None: all), and the (bra, ket) tiles
    of at most 64 x 64 columns through one plan.  ValueError, before any device work, for a result of more than max_bytes bytes
    (where the number of selected states follows from the arguments or the quantum numbers; a projected sector with an open-ended
    selection is refused once its representatives are counted, before it is diagonalised); what full_spectrum refuses is refused."""
    import torch

    from . import api
    from .diagonalize import _unprojected_dimension, full_spectrum

    who = "eigenstate_matrix_elements"
    operators = list(operators) if not isinstance(operators, (dict, config.OperatorSpec)) and hasattr(operators, "__iter__") else [operators]
    if not operators:
        raise ValueError(f"{who}: no operators")
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, int) or max_bytes < 1:
        raise ValueError(f"{who}: max_bytes = {max_bytes!r}: a positive integer")
    if states is not None and not isinstance(states, slice):
        states = np.asarray(states)
        if states.ndim != 1 or states.dtype.kind not in "iu":
            raise ValueError(f"{who}: states must be None, a slice or a 1-D array of integer indices, got {states.dtype} {states.shape}")

    def refuse(m):
        need = 16 * len(operators) * m * m
        if need > max_bytes:
            raise ValueError(f"{who}: {len(operators)} operators between {m} states are {need} bytes; max_bytes is {max_bytes} "
                             "(select fewer with states=)")

    load = api.loadConfigFromYaml if isinstance(config_, str) else api.loadConfigFromDict
    basis, _ = load(config_, hamiltonian=True)
    known = _unprojected_dimension(basis)

    def selected(n):
        if states is None:
            return n
        if isinstance(states, slice):
            return None if n is None and _open_ended(states) else len(range(*states.indices(n if n is not None else _SLICE_BOUND)))
        return int(states.size)

    m = selected(known)
    if m is not None:
        refuse(m)
    else:  # a projected sector, all of it or an open-ended slice: its size is the number of representatives
        reps, _ = api.enumerateStates(basis, 1)
        refuse(selected(int(reps[0].numel())))
    spec = full_spectrum(config_, eigenvectors=True, max_dim=max_dim)
    n = spec.dimension
    index = np.arange(n)[states if states is not None else slice(None)]
    refuse(int(index.size))
    vecs =spec.eigenvectors[:, torch.from_numpy(index).to(spec.eigenvectors.device)].contiguous()
    m = int(index.size)
    out = np.zeros((len(operators), m, m), dtype=np.complex128)
    if m:
        pl = ExpectationPlan(basis, spec.representatives, operators)
        try:
            for i0 in range(0, m, 64):
                for j0 in range(0, m, 64):
                    out[:, i0:i0 + 64, j0:j0 + 64] = pl.matrix_elements(vecs[:, i0:i0 + 64], vecs[:, j0:j0 + 64])
        finally:
            pl.destroy()
    return spec.eigenvalues[index], out


_SLICE_BOUND = 1 << 62


def _open_ended(s):
    """whether the length of range(*s.indices(n)) depends on n: a missing or negative bound"""
    step = 1 if s.step is None else s.step
    lo, hi = (s.start, s.stop) if step > 0 else (s.stop, s.start)
    return hi is None or hi < 0 or (lo is not None and lo < 0)


def expectation_values_block(basis, reps, psi, operators):
    """<O_k> of every normalised column of the (n, K) block psi for every operator (what ExpectationPlan accepts), through one plan
    and one pass -> complex128 (n_ops, K)"""
    import torch

    pl = ExpectationPlan(basis, reps, operators)
    try:
        if isinstance(psi, torch.Tensor) and psi.dim() == 2 and psi.numel():
            nrm = torch.linalg.vector_norm(psi, dim=0)
            psi = psi / torch.where(nrm > 0, nrm, torch.ones_like(nrm))
        return pl.values_block(psi)
    finally:
        pl.destroy()


def expectation_values(basis, reps, psi, operators):
    """<O_k> of the normalised psi for every operator (what ExpectationPlan accepts), through one plan -> complex128 (K,)"""
    pl = ExpectationPlan(basis, reps, operators)
    try:
        return pl.values(_normalised(psi))
    finally:
        pl.destroy()


_SUB = "₀₁₂₃"
_AXES = ("σˣ", "σʸ", "σᶻ")


def dimer_section(bond_a, bond_b, scale: float = 1.0):
    """the operator section of scale (S_i.S_j)(S_k.S_l) for the bonds (i, j) and (k, l): 9 monomials sigma^a_i sigma^a_j sigma^b_k
    sigma^b_l / 16 on the distinct sites of the two bonds (a site both bonds hold carries the composed site operator)"""
    sites = []
    for q in (*bond_a, *bond_b):
        if int(q) not in sites:
            sites.append(int(q))
    (i, j), (k, l) = [[sites.index(int(q)) for q in b] for b in (bond_a, bond_b)]
    if i == j or k == l:
        raise LsAmdError(f"dimer_correlations: a bond joins two different sites, got {tuple(bond_a)} and {tuple(bond_b)}")
    terms = [{"expression": f"{0.0625 * float(scale)!r} × {a}{_SUB[i]} {a}{_SUB[j]} {b}{_SUB[k]} {b}{_SUB[l]}", "sites": [sites]}
             for a in _AXES for b in _AXES]
    return {"terms": terms}


def dimer_correlations(basis, reps, psi, bonds):
    """-> real (B, B): C[b][b'] = Re <(S_i.S_j)(S_k.S_l)> of the normalised psi on a spin-1/2 basis, bonds b = (i, j), b' = (k, l); the
    diagonal is <(S_i.S_j)^2>.  (The real part is symmetric in the two bonds: the upper triangle is evaluated.)"""
    if basis.particleType() != 0:
        raise LsAmdError("dimer_correlations: S_i.S_j is an operator of spin-1/2 bases; a fermionic basis has pair_correlations")
    bonds = [tuple(int(q) for q in b) for b in bonds]
    B = len(bonds)
    where = [(a, b) for a in range(B) for b in range(a, B)]
    vals = expectation_values(basis, reps, psi, [dimer_section(bonds[a], bonds[b]) for a, b in where])
    out = np.zeros((B, B))
    for (a, b), v in zip(where, vals):
        out[a, b] = out[b, a] = v.real
    return out


def pair_section(i, j):
    """the operator section of Delta+_i Delta_j, Delta_i = c_{i down} c_{i up}; i == j: n_{i up} n_{i down}"""
    if i == j:
        return {"terms": [{"expression": "n₀↑ n₀↓", "sites": [[int(i)]]}]}
    return {"terms": [{"expression": "c†₀↑ c†₀↓ c₁↓ c₁↑", "sites": [[int(i), int(j)]]}]}


def pair_correlations(basis, reps, psi, sites=None):
    """-> complex (L, L): P[i][j] = <Delta+_i Delta_j> of the normalised psi on a spinful-fermion basis, Delta_i = c_{i down} c_{i up}
    (on-site singlet pairs), P[i][i] = <n_{i up} n_{i down}>; sites: a subset of the sites (default: all, in order)"""
    if basis.particleType() == 0:
        raise LsAmdError("pair_correlations: on-site pairs are operators of spinful-fermion bases; a spin-1/2 basis has dimer_correlations")
    if basis.particleType() != config.PARTICLES["spinful-fermion"]:
        raise LsAmdError("pair_correlations: on-site pairs Delta_i = c_{i down} c_{i up} need a spinful-fermion basis, not a spinless one "
                         "(its four-point functions go through expectation_values)")
    sites = list(range(basis.numberSites())) if sites is None else [int(q) for q in sites]
    n = len(sites)
    vals = expectation_values(basis, reps, psi, [pair_section(i, j) for i in sites for j in sites])
    return np.asarray(vals).reshape(n, n)


def expectation(config_, operators, state=None, dtype=None, eps: float = 1e-10):
    """<O_k> of a config (dict or YAML path) for every operator (what ExpectationPlan accepts; sections are the simplest).  state None:
    its ground state (thick-restart Lanczos to eps, as correlations.correlations(config)); else a vector on enumerateStates(basis, 1)."""
    import torch

    from . import api
    from .diagonalize import LocalOperator, lanczos_smallest

    load = api.loadConfigFromYaml if isinstance(config_, str) else api.loadConfigFromDict
    basis, h = load(config_, hamiltonian=True)
    reps, _ = api.enumerateStates(basis, 1)
    if state is None:
        if dtype is None:
            dtype = torch.complex128 if _complex_characters(basis) or not h.isReal else torch.float64
        state = lanczos_smallest(LocalOperator(h, reps, dtype), num_evals=1, eps=eps).eigenvectors[0]
    return expectation_values(basis, reps[0], state, operators)
