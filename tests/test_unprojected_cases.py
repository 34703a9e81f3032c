"""Validates tests/unprojected_cases.py, the table of tests/test_gpu_unprojected_operators.py, without a GPU: every row's reference
(tests/sector_reference.py) has the states, the size, the realness and the Hermiticity the table states, and the operator families
this table adds equal plain Kronecker products of 2 x 2 Pauli matrices entry by entry -- built here, from the definition of the
family and not from its expression strings, so the strings (the `(a+bj)` prefix, sigma^y sigma^z) are pinned independently of the
oracle's expression compiler."""
import itertools

import numpy as np
import pytest

import sector_reference
from projected_cases import make_config
from unprojected_cases import CASES, reference_of

LEAK = 1e-12  # max |H B - B (B^+ H B)|: the operator maps the sector into itself
# entries are sums of at most a few dozen products of magnitude <= max|H| ~ 10, each rounded at 2.2e-16 (tests/test_sector_reference.py)
ENTRY = 1e-13


def expected_states(L, weight=None, X=None, **_):
    """what the basis says, in plain bit arithmetic: all words of L bits, or those of one weight; with the flip, the member of
    {s, ~s} with the smaller value"""
    if weight is None:
        states = np.arange(1 << L, dtype=np.uint64)
    else:
        sites = np.array(list(itertools.combinations(range(L), weight)), dtype=np.uint64)
        states = np.sort((np.uint64(1) << sites).sum(axis=1, dtype=np.uint64))
    if X is not None:
        states = states[states < (states ^ np.uint64((1 << L) - 1))]
    return states


@pytest.mark.parametrize("name", sorted(CASES))
def test_row_is_what_the_table_says(name):
    family, args, is_real, is_hermitian, n = CASES[name]
    states, H, leak = reference_of(name)
    assert len(states) == n and H.shape == (n, n)
    assert n > 1024  # several 256-row tiles, and no partition of three is trivial
    assert leak <= LEAK, leak
    want = expected_states(**args)
    assert states.dtype == np.uint64 and np.array_equal(states, want)
    if "weight" in args:
        assert all(bin(int(s)).count("1") == args["weight"] for s in states[:: max(1, n // 64)])
    scale = abs(H).max()
    assert scale > 0.5
    assert (abs(H - H.conj().T).max() <= ENTRY * scale) == is_hermitian
    assert (np.abs(H.data.imag).max() <= ENTRY * scale) == is_real
    if not is_hermitian:
        assert abs(H - H.conj().T).max() > 0.3  # (not a rounding: the smallest off-diagonal amplitude of the table is 0.4)
    if not is_real:
        assert np.abs(H.data.imag).max() > 0.3


# ---------------------------------------------------------------------------------------------
# the new families against Kronecker products
# ---------------------------------------------------------------------------------------------
PAULI = {
    "1": np.eye(2, dtype=complex),
    "x": np.array([[0, 1], [1, 0]], dtype=complex),
    "y": np.array([[0, -1j], [1j, 0]], dtype=complex),
    "z": np.array([[1, 0], [0, -1]], dtype=complex),
    "+": np.array([[0, 1], [0, 0]], dtype=complex),  # |0><1|: bit value 0 is "up"
    "-": np.array([[0, 0], [1, 0]], dtype=complex),
}


def product(L, coefficient, factors):
    """coefficient x the Kronecker product with `factors` = {site: kind}; site 0 is the least significant bit of the index"""
    out = np.array([[coefficient]], dtype=complex)
    for site in range(L):
        out = np.kron(PAULI[factors.get(site, "1")], out)
    return out


def kron_hamiltonian(family, L):
    H = np.zeros((1 << L, 1 << L), dtype=complex)
    for i in range(L):
        j = (i + 1) % L
        if family == "xyz":
            terms = [(1.0, "xx"), (0.6, "yy"), (0.8, "zz")]
        elif family == "twist":
            terms = [(1.0, "zz"), (0.4j, "yz")]
            H += product(L, 0.7, {i: "x"})
        elif family == "phase_hop":
            terms = [(0.6 + 0.8j, "+-"), (1.0, "zz")]
        elif family == "two_domain":
            J = 1.0 if i < L // 2 else 0.6
            terms = [(J, "xx"), (J, "yy"), (J, "zz")]
        for c, (a, b) in terms:
            H += product(L, c, {i: a, j: b})
    return H


def flip_sector(H, L, X, weight=None):
    """B^T H B over the columns (|r> + X |~r>) / sqrt 2, r the smaller of {r, ~r} (of one weight where given), ascending"""
    full = (1 << L) - 1
    reps = [r for r in range(1 << L) if r < (r ^ full) and (weight is None or bin(r).count("1") == weight)]
    B = np.zeros((1 << L, len(reps)))
    for k, r in enumerate(reps):
        B[r, k] = 1 / np.sqrt(2)
        B[r ^ full, k] = X / np.sqrt(2)
    return np.array(reps, dtype=np.uint64), B.T @ H @ B


# (family, arguments of the sector with the flip; phase_hop is not even under it -- sigma^+ sigma^- turns into sigma^- sigma^+ --, so it
# has none, here and in the table)
KRON = [("xyz", dict(X=1)), ("xyz", dict(X=-1)), ("twist", dict(X=-1)), ("two_domain", dict(weight=4, X=1)), ("phase_hop", None)]


@pytest.mark.parametrize("family,flip", KRON, ids=[f + ("" if a is None else "_x%d" % a["X"]) for f, a in KRON])
def test_new_families_equal_kronecker_products(family, flip):
    L = 8
    want = kron_hamiltonian(family, L)
    scale = np.abs(want).max()
    states, H, leak = sector_reference.sector_matrix(make_config(family, L))
    assert np.array_equal(states, np.arange(1 << L, dtype=np.uint64)) and leak <= LEAK
    assert np.abs(H.toarray() - want).max() <= ENTRY * scale
    assert scale >= 1.0 and np.abs(want - np.diag(np.diag(want))).max() >= 0.4  # (not an empty comparison)
    if flip is None:
        return
    reps, want_sector = flip_sector(want, L, flip["X"], flip.get("weight"))
    states, H, leak = sector_reference.sector_matrix(make_config(family, L, **flip))
    assert np.array_equal(states, reps) and leak <= LEAK
    assert np.abs(H.toarray() - want_sector).max() <= ENTRY * scale
    assert np.abs(want_sector - np.diag(np.diag(want_sector))).max() >= 0.4


def test_twist_is_a_real_matrix_that_is_not_hermitian():
    """its sigma^y sigma^z term has an imaginary coefficient: i sigma^y = [[0, 1], [-1, 0]] is real and antisymmetric"""
    H = kron_hamiltonian("twist", 8)
    assert np.abs(H.imag).max() == 0.0
    assert np.abs(H - H.T).max() == pytest.approx(0.8)  # the sigma^y sigma^z part is antisymmetric: 2 x 0.4
    ref = sector_reference.sector_matrix(make_config("twist", 8))[1].toarray()
    assert np.abs(ref.imag).max() == 0.0 and np.abs(ref - ref.T).max() == pytest.approx(0.8)
