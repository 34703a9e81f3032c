"""The matrix of an operator on the GPU: CrossSectorPlan.to_csr / Operator.to_csr (the k_cross_pull kernels in their emitting mode,
k_csr_merge, k_csr_write) and diagonalize.full_spectrum, against reference matrices that use nothing of this library
(tests/cross_sector_reference.py, tests/fermion_cross_reference.py), against the production matvec beyond dense sizes, and the
refusals that must be loud."""
import numpy as np
import pytest

import cross_sector_reference as X
import distributed_matvec_amd as D
import fermion_cross_reference as R
import fermion_jw as J
import fermion_symm as F
from distributed_matvec_amd import CsrMatrix  # noqa: F401  (the feature under test: without it nothing here can run)
from distributed_matvec_amd import config
from distributed_matvec_amd.diagonalize import diagonalize, full_spectrum

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def _dtype(torch, name):
    return torch.complex128 if name == "c128" else torch.float64


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _structure(csr, n_rows, n_cols):
    """canonical CSR: ends of row_ptr, monotone, columns in range and strictly ascending inside every row -> (row_ptr, col)"""
    ptr, col = csr.crow_indices.cpu().numpy(), csr.col_indices.cpu().numpy()
    assert tuple(csr.shape) == (n_rows, n_cols) and ptr.dtype == np.int64 and col.dtype == np.int64
    assert ptr.shape == (n_rows + 1,) and ptr[0] == 0 and ptr[-1] == len(col) == csr.nnz == csr.values.numel()
    assert (np.diff(ptr) >= 0).all()
    if len(col):
        assert col.min() >= 0 and col.max() < n_cols
        inner = np.ones(len(col), dtype=bool)
        inner[ptr[:-1][np.diff(ptr) > 0]] = False  # the first entry of a row has no predecessor in it
        assert (np.diff(col)[inner[1:]] > 0).all()
    return ptr, col


def _against_reference(torch, csr, ref, tol, what, real):
    """element-wise to tol, and the stored pattern is {|ref| > 1e-9} (the reference has nothing between 1e-13 and 1e-9)"""
    n_rows, n_cols = ref.shape
    ptr, col = _structure(csr, n_rows, n_cols)
    dense = csr.to_dense().cpu().numpy()
    if real:
        assert np.abs(ref.imag).max() <= 1e-14
        ref = ref.real
    err = np.abs(dense - ref).max()
    mag = np.abs(ref)
    between = np.count_nonzero((mag > 1e-13) & (mag <= 1e-9))
    kept = mag > 1e-9
    print(f"sector matrix {what}: {n_rows} x {n_cols}, nnz {csr.nnz}, reference nnz {np.count_nonzero(kept)}, max error {err:.3e}, "
          f"tolerance {tol:.3e}, largest cancelled entry {mag[~kept].max() if (~kept).any() else 0.0:.3e}, smallest kept {mag[kept].min():.3e}")
    assert between == 0
    assert np.isfinite(dense).all() and err <= tol
    stored = np.zeros(ref.shape, dtype=bool)
    stored[np.repeat(np.arange(n_rows), np.diff(ptr)), col] = True
    assert np.array_equal(stored, kept)
    # the same arrays as torch's own CSR tensor
    t = csr.to_torch()
    assert t.layout == torch.sparse_csr and tuple(t.shape) == ref.shape
    assert torch.equal(t.crow_indices(), csr.crow_indices) and torch.equal(t.col_indices(), csr.col_indices)


# ---- 1. the rectangular cases of the cross-sector suite ----------------------------------------------------------------------------
def _spin_setup(src_cfg, dst_cfg, op_cfg):
    sbasis = D.loadConfigFromDict(src_cfg)
    A = D.Operator.fromSpec(sbasis, config.parse_operator(op_cfg, sbasis.spec))
    tbasis = D.loadConfigFromDict(dst_cfg)
    sreps, _ = D.enumerateStates(sbasis, 1)
    treps, _ = D.enumerateStates(tbasis, 1)
    return sbasis, A, sreps[0], tbasis, treps[0]


CANCELLED = {"L16_splus_w8_w7_k0_k5": 4, "L8_splus_w4_w3_k0_k3": 2}  # merged entries whose summands cancel


@pytest.mark.parametrize("name", sorted(X.ALL_CASES))
def test_rectangular_cases_match_the_reference_matrix(torch, name):
    src, dst, op, dt = X.ALL_CASES[name]
    ref = X.case_formula(name)
    sbasis, A, sreps, tbasis, treps = _spin_setup(src, dst, op)
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, _dtype(torch, dt))
    csr = plan.to_csr()
    assert plan.csr_bytes > 0 and csr.nnz <= plan.nnz == ref["images"]
    # an entry sums at most n_groups products of a term coefficient, a character and a norm ratio <= sqrt(|G|)
    tol = 1e-12 * X.coefficient_sum(op) * np.sqrt(max(sbasis.groupOrder(), 1))
    _against_reference(torch, csr, ref["matrix"], tol, name, dt == "f64")
    if name in CANCELLED:
        # packets that reach the source and leave no entry: merged duplicates and the cancelled sums
        merged = np.abs(ref["matrix"]) > 1e-9
        assert csr.nnz == np.count_nonzero(merged) < plan.nnz
    if name == "L8_sz_k0_k4":
        ptr = csr.crow_indices.cpu().numpy()
        assert csr.nnz == 5 and len(ptr) == 11 and np.count_nonzero(np.diff(ptr) == 0) >= 5  # empty rows
    plan.destroy()


# ---- 2. square sector Hamiltonians ---------------------------------------------------------------------------------------------------
def _heisenberg_op(L):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    return {"terms": [{"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds}, {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]}


def _heisenberg(basis_cfg, L):
    return {"basis": basis_cfg["basis"], "hamiltonian": _heisenberg_op(L)}


def _ring_no_weight(L, k):
    return {"basis": {"number_spins": L, "symmetries": [{"permutation": [(i + 1) % L for i in range(L)], "sector": k}]}}


# (basis config, sites, rows, f64?, packets > entries?)
SQUARE = {
    "ring_12_6_k5": (X.ring(12, 6, 5), 12, 75, False, True),           # zero-norm source images
    "ring_16_8_k3": (X.ring(16, 8, 3), 16, 800, False, True),          # four tiles, a ragged last one
    "ring_16_8_k0_r0_i1": (X.ring(16, 8, 0, 0, 1), 16, 257, True, True),  # f64; duplicates merged; a last tile of one row
    "ring_34_3_k5": (X.ring(34, 3, 5), 34, 176, False, True),          # 64-bit words
    "ring_10_k3": (_ring_no_weight(10, 3), 10, 99, False, False),      # no fixed weight
}


@pytest.fixture(scope="module")
def square_reference():
    cache = {}

    def get(name):
        if name not in cache:
            cfg, L = SQUARE[name][0], SQUARE[name][1]
            cache[name] = X.formula_matrix(cfg, cfg, _heisenberg_op(L))
        return cache[name]

    return get


@pytest.mark.parametrize("name", sorted(SQUARE))
def test_square_sector_hamiltonians(torch, square_reference, name):
    cfg, L, rows, real, fewer = SQUARE[name]
    ref = square_reference(name)
    basis, h = D.loadConfigFromDict(_heisenberg(cfg, L), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    assert np.array_equal(_u64(reps[0]), ref["src"]) and len(ref["src"]) == rows
    csr = h.to_csr(reps)  # a list of one partition; dtype None: f64 only for a real operator with +-1 characters
    assert csr.dtype == (torch.float64 if real else torch.complex128)
    tol = 1e-12 * 3 * L * np.sqrt(basis.groupOrder())
    _against_reference(torch, csr, ref["matrix"], tol, name, real)
    plan = D.CrossSectorPlan(h, reps[0], basis, reps[0], csr.dtype)
    assert plan.nnz == ref["images"] and csr.nnz <= plan.nnz
    print(f"{name}: images {plan.nnz} -> nnz {csr.nnz}")
    if fewer:
        assert csr.nnz < plan.nnz
    plan.destroy()
    dense = h.to_dense(reps[0])
    assert float((dense - dense.mH).abs().max()) <= tol


# ---- 3. fermions ---------------------------------------------------------------------------------------------------------------------
FERMI = {
    "tV_12_N6_k5": (R.sector(12, 6, F.translations(12), [5]), F.tv_model(J.ring(12), 1.0, 2.0)),
    "tV_34_N3_k5": (R.sector(34, 3, F.translations(34), [5]), F.tv_model(J.ring(34), 1.0, 2.0)),
    "hubbard_6_N6_up3_k1": (R.sector(6, 6, F.translations(6), [1], n_up=3), J.hubbard_model(6, J.ring(6))),
}
FERMI_ROWS = {"tV_12_N6_k5": 78, "tV_34_N3_k5": 176, "hubbard_6_N6_up3_k1": 66}


@pytest.mark.parametrize("name", sorted(FERMI))
def test_projected_fermionic_sectors(torch, name):
    sec, model = FERMI[name]
    spinful = sec["n_up"] is not None
    ref = R.reference(sec, sec, model)
    basis = D.loadConfigFromDict(R.basis_config(sec))
    h = D.Operator.fromSpec(basis, config.parse_operator(R.operator_section(model, spinful), basis.spec))
    reps, _ = D.enumerateStates(basis, 1)
    assert np.array_equal(_u64(reps[0]), ref["src"]) and len(ref["src"]) == FERMI_ROWS[name]
    plan = D.CrossSectorPlan(h, reps[0], basis, reps[0], torch.complex128)
    assert plan.kernel == "k_cross_pull_fermi" and plan.nnz == ref["images"]
    csr = plan.to_csr()
    print(f"{name}: images {plan.nnz} -> nnz {csr.nnz}")
    assert csr.nnz < plan.nnz
    tol = 1e-12 * R.coefficient_sum(model) * np.sqrt(basis.groupOrder())
    _against_reference(torch, csr, ref["matrix"], tol, name, False)
    plan.destroy()


def test_unprojected_spinful_creation_operator(torch):
    """c+_{2 up} from (N, N_up) = (6, 3) to (7, 4) on 6 sites: no group, the product index, rectangular"""
    L = 6
    model = [(1.0, [("+", 2, 0)])]
    src = {"basis": {"particle": "spinful-fermion", "number_sites": L, "number_particles": 6, "number_up": 3}}
    dst = {"basis": {"particle": "spinful-fermion", "number_sites": L, "number_particles": 7, "number_up": 4}}
    sbasis, A, sreps, tbasis, treps = _spin_setup(src, dst, {"terms": J.yaml_terms(model, True)})
    cols, rows = J.product_states(L, 3, 3), J.product_states(L, 4, 3)
    assert np.array_equal(_u64(sreps), cols) and np.array_equal(_u64(treps), rows)
    full = J.dense(model, L, True).tocsr()
    mat = np.asarray(full[rows.astype(np.int64)][:, cols.astype(np.int64)].todense())
    for dt in ("f64", "c128"):
        plan = D.CrossSectorPlan(A, sreps, tbasis, treps, _dtype(torch, dt))
        csr = plan.to_csr()
        assert csr.nnz == plan.nnz == np.count_nonzero(mat)  # one flip mask: nothing to merge
        _against_reference(torch, csr, mat.astype(complex), 1e-12, "c+_2up (6,3)->(7,4) " + dt, dt == "f64")
        plan.destroy()


# ---- 4. against the production matvec, beyond dense sizes; 5. determinism ------------------------------------------------------------
def _compare(got, want, scale, what):
    """the bound of test_gpu_cross_sector._compare: |got - want| <= max(1e-13 sum_j |c_j| max|x|, 1e-12 max(|got|, |want|))"""
    tol = np.maximum(1e-13 * scale, 1e-12 * np.maximum(np.abs(got), np.abs(want)))
    err = np.abs(got - want)
    print(f"sector matrix {what}: rows {len(want)}, max |y| {np.abs(want).max():.3e}, max error {err.max():.3e}, smallest tolerance {tol.min():.3e}")
    assert np.isfinite(got).all() and (err <= tol).all(), (what, err.max(), tol.min())


LARGE = {
    # momentum 5 is coprime to 24: one row per orbit of full period, (C(24,12) - C(12,6) - C(8,4) + C(4,2)) / 24 by Moebius inversion
    "ring_24_12_k5": (X.ring(24, 12, 5), 112632, "c128"),
    # 10 563 tiles of 256 rows: more than the resident grid, the grid-stride loop of the emitting kernel runs
    "plain_24_12": ({"basis": {"number_spins": 24, "hamming_weight": 12, "symmetries": []}}, 2704156, "f64"),
}


@pytest.mark.parametrize("name", sorted(LARGE))
def test_csr_times_x_is_the_production_matvec(torch, name):
    cfg, rows, dt = LARGE[name]
    L, dtype = 24, _dtype(torch, dt)
    basis, h = D.loadConfigFromDict(_heisenberg(cfg, L), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    assert reps[0].numel() == rows
    plan = D.CrossSectorPlan(h, reps[0], basis, reps[0], dtype)
    csr = plan.to_csr()
    _structure(csr, rows, rows)
    assert 0 < csr.nnz <= plan.nnz
    x = D.fillRandom(reps[0], 7, dtype)
    y = torch.zeros(rows, dtype=dtype, device=x.device)
    y.index_add_(0, csr.row_indices(), csr.values * x[csr.col_indices])
    y_apply = torch.full_like(y, float("nan"))
    plan.apply(x, y_apply)
    y_matvec = torch.full_like(y, float("nan"))
    D.MatvecPlan(h, reps, dtype).matvec([x], [y_matvec])
    scale = 3 * L * float(x.abs().max())
    _compare(y.cpu().numpy(), y_apply.cpu().numpy(), scale, name + " against CrossSectorPlan.apply")
    _compare(y.cpu().numpy(), y_matvec.cpu().numpy(), scale, name + " against MatvecPlan.matvec")
    if name == "ring_24_12_k5":  # two exports are the same bits
        again = plan.to_csr()
        assert torch.equal(again.crow_indices, csr.crow_indices) and torch.equal(again.col_indices, csr.col_indices)
        assert torch.equal(again.values.view(torch.float64), csr.values.view(torch.float64))
    plan.destroy()


def test_rows_longer_than_a_wave(torch):
    """12 sites without a fixed weight, sigma^x sigma^x on every pair: 66 flip masks and the diagonal, each of them active on every
    row, so every raw row has 67 entries -- more than the 64 lanes that merge and rank it (the chunked sweeps of k_csr_merge and
    k_csr_write)"""
    L = 12
    pairs = [[i, j] for i in range(L) for j in range(i + 1, L)]
    op = {"terms": [{"expression": "σˣ₀ σˣ₁", "sites": pairs}, {"expression": "0.5 σᶻ₀ σᶻ₁", "sites": pairs}]}
    cfg = _ring_no_weight(L, 0)
    ref = X.formula_matrix(cfg, cfg, op)
    basis, h = D.loadConfigFromDict({"basis": cfg["basis"], "hamiltonian": op}, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    n = reps[0].numel()
    plan = D.CrossSectorPlan(h, reps[0], basis, reps[0], torch.float64)
    csr = plan.to_csr()
    print(f"all-to-all ring of 12: {n} rows, {plan.nnz} packets ({plan.nnz / n:.1f} per row), nnz {csr.nnz}")
    assert plan.nnz == ref["images"] and plan.nnz > 64 * n  # some row is longer than a wave
    _against_reference(torch, csr, ref["matrix"], 1e-12 * 1.5 * len(pairs) * np.sqrt(basis.groupOrder()), "all-to-all ring of 12", True)
    plan.destroy()


# ---- 6. full_spectrum ---------------------------------------------------------------------------------------------------------------
def test_full_spectrum_of_a_momentum_sector(torch, square_reference):
    cfg = _heisenberg(X.ring(16, 8, 3), 16)
    H = square_reference("ring_16_8_k3")["matrix"]
    want = np.linalg.eigvalsh(H)
    res = full_spectrum(cfg)
    assert res.dimension == 800 and res.eigenvectors is None and res.eigenvalues.shape == (800,) and res.seconds > 0
    assert np.array_equal(_u64(res.representatives), square_reference("ring_16_8_k3")["src"])
    dev = np.abs(res.eigenvalues - want).max()
    print(f"full_spectrum ring(16, 8, 3): max deviation from numpy {dev:.3e}, ||H|| ~ {np.abs(want).max():.3e}")
    assert (np.diff(res.eigenvalues) >= 0).all() and dev <= 1e-10
    # the lowest level is what the iterative solver finds
    eps = 1e-10
    low = diagonalize(cfg, eps=eps, dtype=torch.complex128)
    assert abs(low.eigenvalues[0] - res.eigenvalues[0]) <= eps * np.abs(want).max() + 1e-10
    # eigenvectors: residuals through the production matvec, orthonormality
    res = full_spectrum(cfg, eigenvectors=True)
    V = res.eigenvectors
    assert V.shape == (800, 800) and V.dtype == torch.complex128 and np.abs(res.eigenvalues - want).max() <= 1e-10
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    mv = D.MatvecPlan(h, [res.representatives], torch.complex128)
    norm_h = float(np.abs(want).max())
    for k in (0, 400, 799):
        v = V[:, k].contiguous()
        hv = torch.zeros_like(v)
        mv.matvec([v], [hv])
        r = float(torch.linalg.vector_norm(hv - res.eigenvalues[k] * v))
        print(f"eigenvector {k}: residual {r:.3e}")
        assert r <= 1e-10 * norm_h
    gram = V.mH @ V
    assert float((gram - torch.eye(800, dtype=V.dtype, device=V.device)).abs().max()) <= 1e-10


def test_the_momentum_sectors_make_up_the_whole_spectrum(torch):
    """12-site ring at weight 6: the spectra of the 12 momentum sectors together are the spectrum of the plain 924-state basis"""
    L = 12
    whole = full_spectrum(_heisenberg({"basis": {"number_spins": L, "hamming_weight": 6, "symmetries": []}}, L))
    assert whole.dimension == 924
    parts = [full_spectrum(_heisenberg(X.ring(L, 6, k), L)) for k in range(L)]
    assert sum(p.dimension for p in parts) == 924
    union = np.sort(np.concatenate([p.eigenvalues for p in parts]))
    dev = np.abs(union - whole.eigenvalues).max()
    print(f"completeness over 12 momentum sectors: max deviation {dev:.3e}")
    assert dev <= 1e-10


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_an_export_above_max_bytes_is_refused_before_it_allocates(torch):
    cfg = X.ring(16, 8, 3)
    basis, h = D.loadConfigFromDict(_heisenberg(cfg, 16), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    plan = D.CrossSectorPlan(h, reps[0], basis, reps[0], torch.complex128)
    need = plan.csr_bytes
    assert need >= plan.nnz * 24 + 8 * 801
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    with pytest.raises(D.LsAmdError, match=rf"{need} bytes.*max_bytes is 1024"):
        plan.to_csr(max_bytes=1024)
    with pytest.raises(D.LsAmdError, match=rf"{need} bytes.*max_bytes is 1024"):
        h.to_csr(reps, max_bytes=1024)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= before  # nothing is left allocated
    plan.to_csr(max_bytes=need)  # the bound itself is enough
    plan.destroy()
    with pytest.raises(D.LsAmdError, match="max_bytes"):
        h.to_csr(reps).to_dense(max_bytes=1024)


def test_two_partitions_are_refused(torch):
    basis, h = D.loadConfigFromDict(_heisenberg(X.ring(12, 6, 0), 12), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 2)
    assert len(reps) == 2
    with pytest.raises(D.LsAmdError, match="one partition"):
        h.to_csr(reps)
    with pytest.raises(D.LsAmdError, match="one partition"):
        h.to_dense(reps)


def test_f64_with_complex_characters_is_refused_by_the_plan(torch):
    basis, h = D.loadConfigFromDict(_heisenberg(X.ring(12, 6, 5), 12), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    with pytest.raises(D.LsAmdError, match="c128"):
        h.to_csr(reps, dtype=torch.float64)


def test_representatives_of_another_sector_raise_from_the_export(torch):
    """the k = 0 Hamiltonian over the representatives of k = 5, which lack the orbits without norm there: images of the rows are not
    in the array, the kernel raises the plan's flag and the export reports it like check()"""
    basis, h = D.loadConfigFromDict(_heisenberg(X.ring(12, 6, 0), 12), hamiltonian=True)
    other = D.loadConfigFromDict(X.ring(12, 6, 5))
    reps, _ = D.enumerateStates(other, 1)
    own, _ = D.enumerateStates(basis, 1)
    assert reps[0].numel() == 75 < own[0].numel()
    with pytest.raises(D.LsAmdError, match="not in the source basis"):
        h.to_csr(reps)
    assert h.to_csr(own).nnz > 0  # the right representatives export
