"""Block Lanczos (diagonalize.lanczos_block_smallest, diagonalize(..., block_size=K)) on the GPU: degenerate levels come out with
their multiplicity, the spectra equal dense eigvalsh on every block-matvec path (k_pull_gather_blk, k_direct_blk, the column loop,
c128 on the torch path), residuals recomputed with single-vector matvecs agree, the fused sweeps agree with the torch products,
P = 3 with P = 1, small sectors end in an invariant subspace, block_size = 1 is lanczos_smallest, bad block sizes are refused
before any matvec, and output files keep the single-vector layout."""
import numpy as np
import pytest

from fermion_jw import dense, hubbard_model, product_states, restrict, ring, yaml_terms
from helpers import complex_translation_config, model_config, oracle_for, oracle_reps

pytestmark = pytest.mark.gpu

# heisenberg_chain_12 (free Hamming weight, 4096 states): E0 and the SU(2) triplet above it, then the next two levels
CHAIN_12 = [-21.549563669780838, -20.126173614969762, -20.126173614969762, -20.126173614969762, -19.109557334805118,
            -18.277497643221828]


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def hubbard_product():
    """a spinful Hubbard ring on the product basis with a pair hopping (not species-separable: k_direct, product index)"""
    L = 6
    model = hubbard_model(L, ring(L), U=3.0) + [(0.5, [("+", 0, 0), ("+", 0, 1), ("-", 3, 1), ("-", 3, 0)]),
                                                (0.5, [("+", 3, 0), ("+", 3, 1), ("-", 0, 1), ("-", 0, 0)])]
    cfg = {"basis": {"particle": "spinful-fermion", "number_sites": L, "number_particles": 5, "number_up": 3},
           "hamiltonian": {"terms": yaml_terms(model, True)}}
    return cfg, restrict(dense(model, L, True), product_states(L, 3, 2)).toarray()


def spin_dense(name):
    o, reps = oracle_for(name), oracle_reps(name)
    n = len(reps)
    return np.stack([o.local_matvec(reps, np.ascontiguousarray(np.eye(n)[i])) for i in range(n)], axis=1)


def operator(torch, cfg, dtype=None, P=1):
    import distributed_matvec_amd as D
    from distributed_matvec_amd.diagonalize import LocalOperator

    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, masks = D.enumerateStates(basis, P)
    return LocalOperator(h, reps, dtype or torch.float64), (basis, h, reps, masks)


def check_pairs(torch, op, r, want, tol=1e-8):
    """eigenvalues against the dense spectrum, orthonormal vectors, and residuals recomputed with single-vector matvecs"""
    assert r.converged
    assert np.abs(np.array(r.eigenvalues) - np.asarray(want)).max() < tol, (r.eigenvalues, want)
    Y = torch.stack(r.eigenvectors)
    G = Y.conj() @ Y.t()
    assert float((G - torch.eye(len(Y), dtype=Y.dtype, device=Y.device)).abs().max()) < 1e-10
    y = op.new_vector()
    for v, th, res in zip(r.eigenvectors, r.eigenvalues, r.residual_norms):
        op.matvec(v, y)
        got = float(torch.linalg.vector_norm(y - th * v))
        assert got < 1e-6 * max(1.0, abs(th)), (th, got)
        assert abs(got - res) < 1e-7 * max(1.0, abs(th)), (got, res)


def test_multiplicity_of_the_chain_12_triplet(torch):
    """the headline: a single start vector finds the triplet once; a block of 4 finds it three times"""
    from distributed_matvec_amd.diagonalize import diagonalize

    ev = np.linalg.eigvalsh(spin_dense("heisenberg_chain_12"))
    assert np.abs(ev[:6] - CHAIN_12).max() < 1e-10
    for ne in (4, 6):
        r = diagonalize(model_config("heisenberg_chain_12"), num_evals=ne, eps=1e-10, block_size=4)
        assert r.converged
        assert np.abs(np.array(r.eigenvalues) - ev[:ne]).max() < 1e-8, (ne, r.eigenvalues)
        Y = torch.stack(r.eigenvectors)
        assert float((Y @ Y.t() - torch.eye(ne, dtype=Y.dtype, device=Y.device)).abs().max()) < 1e-10


def _reference(torch, op, case):
    """the spectrum to compare with: dense eigvalsh where the sector is small, ARPACK on the single-vector matvec otherwise"""
    n = op.n_local
    if case == "chain_24_symm":  # 28968 states
        import scipy.sparse.linalg as spla

        y = op.new_vector()

        def mv(v):
            op.matvec(torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda"), y)
            return y.cpu().numpy()

        A = spla.LinearOperator((n, n), matvec=mv, dtype=np.float64)
        ev = np.sort(spla.eigsh(A, k=4, which="SA", tol=1e-13, ncv=40, v0=np.ones(n))[0])
    else:
        E = torch.eye(n, dtype=op.dtype, device="cuda")
        y = op.new_vector()
        cols = []
        for i in range(n):
            op.matvec(E[i], y)
            cols.append(y.cpu().numpy().copy())
        H = np.stack(cols, axis=1)
        ev = np.linalg.eigvalsh(0.5 * (H + H.conj().T))
    op.matvecs = 0
    return ev


CASES = {  # name -> (config, dtype, the block path)
    "chain_24_symm": (lambda: model_config("heisenberg_chain_24_symm"), "f64", "k_pull_gather_blk"),
    "kagome_12_symm": (lambda: model_config("heisenberg_kagome_12_symm"), "f64", "k_pull_gather_blk"),
    "hubbard_product": (lambda: hubbard_product()[0], "f64", "k_direct_blk"),
    "chain_12_inversion_columns": (lambda: __import__("distributed_matvec_amd.config", fromlist=["x"]).heisenberg_chain_config(12, spin_inversion=-1),
                                   "f64", "columns"),
    "momentum_12_5_c128": (lambda: complex_translation_config(12, 5), "c128", "k_pull_gather_blk"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_reference_spectrum(torch, case):
    from distributed_matvec_amd.diagonalize import lanczos_block_smallest

    make, dt, path = CASES[case]
    op, _ = operator(torch, make(), torch.complex128 if dt == "c128" else torch.float64)
    ev = _reference(torch, op, case)
    if case == "hubbard_product":  # the reference is also the independent Jordan-Wigner matrix
        assert np.abs(ev[:4] - np.linalg.eigvalsh(hubbard_product()[1])[:4]).max() < 1e-10
    for K in (2, 4, 8):
        assert op.block_kernel(K) == path
        for ne in (1, 4):
            r = lanczos_block_smallest(op, num_evals=ne, block_size=K, eps=1e-10)
            check_pairs(torch, op, r, ev[:ne])


def test_bethe_ansatz_energies(torch):
    from distributed_matvec_amd import config
    from distributed_matvec_amd.diagonalize import diagonalize
    from oracle import bethe

    for L in (24, 32):
        r = diagonalize(config.heisenberg_chain_config(L, symm=True), num_evals=1, eps=1e-10, block_size=4)
        assert r.converged and abs(r.eigenvalues[0] - bethe.ground_state_energy_sigma(L)) < 1e-8, (L, r.eigenvalues)


def test_fused_sweeps_agree_with_torch(torch, monkeypatch):
    from distributed_matvec_amd.diagonalize import lanczos_block_smallest

    op, _ = operator(torch, model_config("heisenberg_kagome_12_symm"))
    a = lanczos_block_smallest(op, num_evals=4, block_size=4, eps=1e-11)
    monkeypatch.setenv("LS_AMD_FUSED_ORTH", "0")
    b = lanczos_block_smallest(op, num_evals=4, block_size=4, eps=1e-11)
    assert a.converged and b.converged
    assert np.abs(np.array(a.eigenvalues) - np.array(b.eigenvalues)).max() < 1e-10


def test_several_partitions_agree_with_one(torch):
    from distributed_matvec_amd.diagonalize import diagonalize

    cfg = model_config("heisenberg_chain_24_symm")
    r1 = diagonalize(cfg, num_evals=4, eps=1e-10, block_size=4)
    r3 = diagonalize(cfg, num_evals=4, eps=1e-10, block_size=4, num_partitions=3)
    assert r1.converged and r3.converged
    assert np.abs(np.array(r1.eigenvalues) - np.array(r3.eigenvalues)).max() < 1e-9


@pytest.mark.parametrize("name,K,ne,basis", [("heisenberg_chain_6", 4, 4, 24), ("heisenberg_chain_8", 8, 6, 80), ("heisenberg_chain_10", 2, 2, 128),
                                             ("heisenberg_chain_4", 6, 3, 8)])
def test_small_sectors_end_in_an_invariant_subspace(torch, name, K, ne, basis):
    """fewer states than the basis holds: every block deflates in the end, and the Ritz pairs are exact, with no NaN"""
    from distributed_matvec_amd.diagonalize import lanczos_block_smallest

    H = spin_dense(name)
    n = len(H)
    op, _ = operator(torch, model_config(name))
    for fused in ("1", "0"):
        import os

        os.environ["LS_AMD_FUSED_ORTH"] = fused
        try:
            r = lanczos_block_smallest(op, num_evals=min(ne, n), block_size=min(K, n), eps=1e-10, max_basis=basis)
        finally:
            del os.environ["LS_AMD_FUSED_ORTH"]
        assert all(np.isfinite(r.eigenvalues)) and all(bool(torch.isfinite(v).all()) for v in r.eigenvectors)
        check_pairs(torch, op, r, np.linalg.eigvalsh(H)[:min(ne, n)])


def test_block_size_one_is_lanczos_smallest(torch, monkeypatch):
    from distributed_matvec_amd import diagonalize as Dg

    cfg = model_config("heisenberg_chain_12")
    r = Dg.diagonalize(cfg, num_evals=4, eps=1e-10)
    calls = []
    orig = Dg.lanczos_smallest
    monkeypatch.setattr(Dg, "lanczos_smallest", lambda *a, **k: calls.append(k) or orig(*a, **k))
    monkeypatch.setattr(Dg, "lanczos_block_smallest", lambda *a, **k: pytest.fail("block_size = 1 took the block solver"))
    r1 = Dg.diagonalize(cfg, num_evals=4, eps=1e-10, block_size=1)
    assert calls == [{"num_evals": 4, "eps": 1e-10, "max_basis": 24, "verbose": False}]
    assert np.abs(np.array(r.eigenvalues) - np.array(r1.eigenvalues)).max() < 1e-10
    # (the single start vector misses the triplet's copies: what block_size exists for)
    assert abs(r.eigenvalues[2] - CHAIN_12[2]) > 0.5


@pytest.mark.parametrize("K", [0, 17, -1])
def test_bad_block_sizes_are_refused_before_anything_runs(torch, K, monkeypatch):
    from distributed_matvec_amd import api, diagonalize as Dg

    called = []
    monkeypatch.setattr(api, "loadConfigFromDict", lambda *a, **k: called.append(1))
    with pytest.raises(ValueError, match="block_size"):
        Dg.diagonalize(model_config("heisenberg_chain_12"), num_evals=1, block_size=K)
    assert not called


def test_block_size_larger_than_the_dimension_is_refused_before_any_matvec(torch, monkeypatch):
    from distributed_matvec_amd import diagonalize as Dg

    calls = []
    for name in ("matvec", "matvec_block"):
        monkeypatch.setattr(Dg.LocalOperator, name, lambda self, *a, _n=name: calls.append(_n))
    with pytest.raises(ValueError, match="exceeds the dimension"):
        Dg.diagonalize(model_config("heisenberg_chain_4"), num_evals=1, block_size=16)  # 6 states
    assert not calls


def test_outputs_keep_the_single_vector_layout(torch, tmp_path):
    from distributed_matvec_amd import hdf5
    from distributed_matvec_amd.diagonalize import diagonalize

    cfg = model_config("heisenberg_chain_10")
    a, b = str(tmp_path / "single.npz"), str(tmp_path / "block.npz")
    ra = diagonalize(cfg, num_evals=2, eps=1e-10, output=a)
    rb = diagonalize(cfg, num_evals=2, eps=1e-10, output=b, block_size=2)
    da, db = np.load(a), np.load(b)
    assert sorted(da.files) == sorted(db.files)
    for key in da.files:
        assert da[key].shape == db[key].shape and da[key].dtype == db[key].dtype, key
    assert np.array_equal(da["basis/representatives"], db["basis/representatives"])
    assert np.abs(db["hamiltonian/eigenvalues"] - np.array(ra.eigenvalues)).max() < 1e-8
    assert abs(abs(np.dot(da["hamiltonian/eigenvectors"][0], db["hamiltonian/eigenvectors"][0])) - 1) < 1e-8
    assert rb.converged
    try:
        hdf5.lib()
    except hdf5.Hdf5Unavailable:
        return
    ha, hb = str(tmp_path / "single.h5"), str(tmp_path / "block.h5")
    diagonalize(cfg, num_evals=2, eps=1e-10, output=ha)
    diagonalize(cfg, num_evals=2, eps=1e-10, output=hb, block_size=2)
    for ds in ("/basis/representatives", "/hamiltonian/eigenvalues", "/hamiltonian/residuals", "/hamiltonian/eigenvectors"):
        x, y = hdf5.read_dataset(ha, ds), hdf5.read_dataset(hb, ds)
        assert x.shape == y.shape and x.dtype == y.dtype, ds
