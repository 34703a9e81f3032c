"""Validates tests/sector_reference.py, the reference of tests/test_gpu_projected_operators.py, without a GPU: entry by entry against
oracle.model.dense_sector_matrix (dense, state-by-state projector) on reduced copies of every operator family, its term-table branch
against its Kronecker branch, and H_sector @ x against the C oracle's local_matvec on the full-size cases of the table."""
import numpy as np
import pytest

import sector_reference
from oracle import c_oracle as CO
from oracle import model as M
from projected_cases import CASES, config_of, k4_mode_of, reduced_cases, reference_of

LEAK = 1e-12  # max |H B - B (B^+ H B)|: the operator maps the sector into itself
# entries of B^+ H B: sums of at most |G|^2 x (terms per row) products of magnitude <= max|H| ~ 10, each rounded at 2.2e-16, in two
# different orders: 1e-13 (relative to the largest entry) is several hundred roundings
ENTRY = 1e-13


@pytest.mark.parametrize("name", sorted(reduced_cases()))
def test_equals_dense_sector_matrix_entry_by_entry(name):
    cfg = reduced_cases()[name]
    reps, Hs, leak = sector_reference.sector_matrix(cfg)
    want_reps, want = M.dense_sector_matrix(cfg)
    want = np.asarray(want)
    assert len(reps) > 0 and np.array_equal(reps, want_reps)
    assert leak <= LEAK, leak
    err = np.abs(Hs.toarray() - want).max()
    assert err <= ENTRY * max(1.0, np.abs(want).max()), err
    assert np.abs(want).max() > 0.5  # (not an empty comparison)


@pytest.mark.parametrize("name", ["dimer_xxz_10", "chiral_10_k3", "chiral_8_k0_x-1", "jq_10_k0_r1", "hop_10_k3", "chiral_10_2_k1"])
def test_term_table_branch_equals_kronecker_branch(monkeypatch, name):
    """the branch of more than 16 sites (fixed-weight subspace, H from the oracle's term tables), forced at a size the first does"""
    cfg = reduced_cases()[name]
    reps, Hs, leak = sector_reference.sector_matrix(cfg)
    monkeypatch.setattr(sector_reference, "NARROW_SITES", 0)
    reps2, Hs2, leak2 = sector_reference.sector_matrix(cfg)
    assert np.array_equal(reps, reps2) and leak2 <= LEAK
    assert np.abs((Hs - Hs2).toarray()).max() <= ENTRY * max(1.0, np.abs(Hs.toarray()).max())


def test_an_operator_that_breaks_the_symmetry_leaks():
    """leak is what keeps a badly built case from passing as a kernel check: a field on one site does not commute with T"""
    cfg = reduced_cases()["tfim_8_k3"]
    cfg["hamiltonian"]["terms"].append({"expression": "σᶻ₀", "sites": [[2]]})
    assert sector_reference.sector_matrix(cfg)[2] > 1e-3


def test_weight_states():
    for L, w in ((5, 0), (6, 3), (20, 2), (36, 4)):
        s = sector_reference.weight_states(L, w)
        assert len(s) == M.binomial(L, w) and (np.diff(s.astype(np.int64)) > 0).all()
        assert all(bin(int(v)).count("1") == w for v in s[:: max(1, len(s) // 50)])


@pytest.mark.parametrize("name", sorted(CASES))
def test_full_size_cases_equal_the_c_oracle(name):
    family, args, is_real, is_hermitian, k4, _, count = CASES[name]
    cfg = config_of(name)
    model = M.model_from_config(cfg)
    reps, Hs, leak = reference_of(name)
    n = len(reps)
    assert n > 256, n  # more than one tile and window
    assert count is None or n == count, (n, count)
    assert leak <= LEAK, leak
    o = CO.COracle(model)
    assert np.array_equal(o.enumerate(), reps)
    # the row of the table: the characters ask for the K4 mode listed, the operator is as real and as Hermitian as listed
    assert k4_mode_of(model) == k4
    coefficients = np.concatenate([model.diag.v, model.offdiag.v])
    assert (np.abs(coefficients.imag).max() == 0.0) == is_real
    assert (abs(Hs - Hs.conj().T).max() <= ENTRY * abs(Hs).max()) == is_hermitian
    rs = np.random.RandomState(5)
    x = (rs.rand(n) - 0.5) + 1j * (rs.rand(n) - 0.5)
    want = o.local_matvec(reps, x)
    err = np.abs(Hs @ x - want).max()
    print(f"{name}: n = {n} nnz = {Hs.nnz} leak = {leak:.1e} max|want| = {np.abs(want).max():.2f} max|H_sector x - oracle| = {err:.1e}")
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), err
