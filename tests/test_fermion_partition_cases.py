"""Validates tests/fermion_partition_cases.py, the table of tests/test_gpu_fermion_partitions.py, without a GPU: the new 16-mode
rows against the compiled terms and against the dense Jordan-Wigner matrix, the flags and sizes the table records against the
reference matrix (fermion_jw.sector_matrix), and what the reach tests of the GPU file rely on -- which ranks leave blocks of the
vector unread and which need more than 16 intervals -- from the reference matrix alone."""
import numpy as np
import pytest

from distributed_matvec_amd import config
from fermion_jw import dense, restrict, sector_matrix, terms_matrix
from fermion_partition_cases import (ALL, COMPLEX, EXCHANGE_ONLY, FIXED_WEIGHT, HERMITIAN, NARROW, NARROW_CASES, NO_DIAGONAL,
                                     NON_HERMITIAN, PRODUCT, ROWS, WIDE, marked_blocks, reach_of, reference_of, vectors)
from fermion_wide import CASES as WIDE_CASES

ENTRY = 1e-12  # entries are sums of a few products of magnitude <= 4, each rounded at 2.2e-16


def _max(A):
    return abs(A).max() if A.nnz else 0.0


def test_the_table_has_the_rows_it_should():
    assert WIDE == ["spinless_open_33_3", "spinless_long_40_3", "spinless_long_40_3_complex", "spinless_ring_64_2",
                    "spinless_ring_36_33", "hubbard_ring_17_2_2", "hubbard_ring_17_2_2_free", "hubbard_32_1_2_pair_hop",
                    "spinful_17_n3_flips"]
    assert NARROW == ["spinless_open_16_8", "spinless_ring_16_7_peierls", "spinless_directed_16_8", "hubbard_ring_8_4_4",
                      "hubbard_8_3_4_pair_hop", "spinful_8_n5_flips"]
    assert ALL == WIDE + NARROW
    for name in WIDE:
        assert ROWS[name].case is WIDE_CASES[name]
    assert NON_HERMITIAN == ["spinless_directed_16_8"]
    assert COMPLEX == ["spinless_long_40_3_complex", "spinless_ring_16_7_peierls"]
    assert NO_DIAGONAL == ["spinless_ring_64_2", "hubbard_ring_17_2_2_free"]
    assert PRODUCT == ["hubbard_ring_17_2_2", "hubbard_ring_17_2_2_free", "hubbard_32_1_2_pair_hop", "hubbard_ring_8_4_4",
                       "hubbard_8_3_4_pair_hop"]
    assert sorted(FIXED_WEIGHT + PRODUCT) == sorted(ALL)
    assert {n: ROWS[n].n for n in NARROW} == {"spinless_open_16_8": 12870, "spinless_ring_16_7_peierls": 11440,
                                              "spinless_directed_16_8": 12870, "hubbard_ring_8_4_4": 4900,
                                              "hubbard_8_3_4_pair_hop": 3920, "spinful_8_n5_flips": 4368}


@pytest.mark.parametrize("name", ALL)
def test_row_is_what_the_table_says(name):
    row = ROWS[name]
    states, H = reference_of(name)
    assert states.dtype == np.uint64 and np.all(states[1:] > states[:-1])
    assert len(states) == row.n == H.shape[0] == H.shape[1]
    assert 1024 < row.n < 20000  # several tiles in every partition of eight, and a cheap reference
    modes = row.case.L * (2 if row.case.spinful else 1)
    assert int(states[-1]) < 1 << modes
    assert (name in NARROW) == (modes <= 32)
    assert np.all(np.bitwise_count(states) == row.case.N)
    if row.case.spinful and row.case.n_up is not None:
        assert np.all(np.bitwise_count(states & np.uint64((1 << row.case.L) - 1)) == row.case.n_up)
    scale = _max(H)
    assert scale >= 0.5
    assert (_max(H - H.getH()) <= ENTRY * scale) == row.is_hermitian
    assert (np.abs(H.data.imag).max() <= ENTRY * scale) == row.is_real == row.case.is_real
    assert (np.abs(H.diagonal()).max() > 0) == row.has_diagonal
    assert row.has_diagonal == any(all(kind == "n" for kind, _, _ in ops) for _, ops in row.case.model)
    if not row.is_hermitian:
        assert _max(H - H.getH()) >= 1.0  # (not a rounding: a hop of amplitude 1 without its conjugate)
    if not row.is_real:
        assert np.abs(H.data.imag).max() > 0.2  # sin 0.21 = 0.208, Im(0.3 + 0.4j)


@pytest.mark.parametrize("name", NARROW)
def test_new_rows_compiled_terms_and_dense_matrix(name):
    """the compiled terms (v, m, r, x, s) of the expression compiler and the Kronecker-product matrix on 2^16 words both equal the
    sector reference"""
    case = NARROW_CASES[name]
    states, want = reference_of(name)
    cfg = case.config()
    terms = config.parse_operator(cfg["hamiltonian"], config.parse_basis(cfg)).terms
    assert _max(terms_matrix(terms, states) - want) <= ENTRY, name
    assert (2 * case.L if case.spinful else case.L) == 16
    assert _max(restrict(dense(list(case.model), case.L, case.spinful), states) - want) <= ENTRY, name
    assert want.nnz > 4 * len(states)  # (not an empty comparison)


def test_signed_closing_bonds_are_there():
    """what the narrow rings are for: the closing bond crosses N - 1 other particles, so its sign depends on N -- both signs occur
    across the table's rows (N - 1 = 6 even, N - 1 = 7 odd), and inside the spinful words"""
    states, H = reference_of("spinless_ring_16_7_peierls")
    at = {int(s): i for i, s in enumerate(states)}
    a = sum(1 << b for b in (0, 2, 3, 5, 8, 9, 11))
    b = a ^ 1 ^ (1 << 15)
    t = -np.exp(0.21j)
    # t c^+_15 c_0: six occupied modes between the two ends
    assert abs(H[at[b], at[a]] - t) < 1e-15 and abs(H[at[a], at[b]] - np.conj(t)) < 1e-15
    states, H = reference_of("spinless_directed_16_8")
    at = {int(s): i for i, s in enumerate(states)}
    a = sum(1 << b for b in (0, 2, 3, 5, 8, 9, 11, 12))
    b = a ^ 1 ^ (1 << 15)
    assert H[at[b], at[a]] == 1.0 and H[at[a], at[b]] == 0.0  # -1 c^+_15 c_0 across seven particles; its conjugate is not there


def test_exchange_only_rows():
    """EXCHANGE_ONLY: every off-diagonal term joins adjacent modes (no Jordan-Wigner string) with one real amplitude both ways"""
    for name in ALL:
        case = ROWS[name].case
        if case.spinful:
            assert name not in EXCHANGE_ONLY
            continue
        hops = [ops for _, ops in case.model if any(kind != "n" for kind, _, _ in ops)]
        adjacent = all(abs(ops[0][1] - ops[1][1]) == 1 for ops in hops)
        assert (adjacent and ROWS[name].is_real and ROWS[name].is_hermitian) == (name in EXCHANGE_ONLY), name


# ---------------------------------------------------------------------------------------------
# the GPU comparisons have teeth: a broken reference moves y by far more than the 1e-12 they allow
# ---------------------------------------------------------------------------------------------
def _closing_bonds(case):
    """indices of the hops between site 0 and site L - 1 (same species): their string runs over every other mode of the species"""
    return [k for k, (_, ops) in enumerate(case.model)
            if len(ops) == 2 and {ops[0][0], ops[1][0]} == {"+", "-"} and abs(ops[0][1] - ops[1][1]) == case.L - 1]


@pytest.mark.parametrize("name", [n for n in ALL if n not in EXCHANGE_ONLY])
def test_a_flipped_closing_bond_sign_would_show(name):
    """every row but the two open chains closes a ring: with the sign of those hops flipped -- what a Jordan-Wigner string that is
    off by one mode gives at odd N - 1 -- the y of the GPU tests' own vectors moves by more than 0.01"""
    case = ROWS[name].case
    bonds = _closing_bonds(case)
    assert bonds, name
    broken = [(-coef if k in bonds else coef, ops) for k, (coef, ops) in enumerate(case.model)]
    states, H = reference_of(name)
    wrong = sector_matrix(broken, case.L, case.spinful, states)
    for cplx in (True,) + ((False,) if ROWS[name].is_real else ()):
        x, _ = vectors(name, cplx, 91)
        assert np.abs((wrong - H) @ x).max() > 0.01, name


@pytest.mark.parametrize("name", NO_DIAGONAL)
def test_an_assigned_y_would_show(name):
    for cplx in (True, False):
        x, y0 = vectors(name, cplx, 91)
        assert np.abs(y0).max() > 0.9 and np.abs(y0 - y0[0]).max() > 0.9  # H x instead of H x + y0 is off by that much
    assert [np.unique(vectors(n, True, 91)[1]).tolist() for n in ALL if ROWS[n].has_diagonal] == [[3.0]] * (len(ALL) - len(NO_DIAGONAL))


@pytest.mark.parametrize("name", HERMITIAN)
def test_every_marked_block_matters(name):
    """the reach tests send another vector first: a block of 32 entries that a rank's rows read but that did not arrive (beyond the
    rank's own rows and their halo, which the host adds whatever the matrix says) would leave that vector's values there, and
    the rank's rows of y would move by more than 1e-4 -- for EVERY block the reference matrix marks"""
    import scipy.sparse as sp

    _, H = reference_of(name)
    n, P = H.shape[0], 3
    x, _ = vectors(name, True, 23)
    other, _ = vectors(name, True, 24)
    block_of = sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) >> 5)), shape=(n, ((n - 1) >> 5) + 1))
    checked = 0
    for p in range(P):
        n0, n1 = n * p // P, n * (p + 1) // P
        marked, _ = marked_blocks(H, P, p)
        moved = abs((H[n0:n1] @ sp.diags(x - other)) @ block_of).max(axis=0).toarray().ravel()
        need = np.zeros_like(marked)
        need[np.unique(H[n0:n1].indices >> 5)] = True
        assert np.all(marked[need])
        assert np.all(moved[need] > 1e-4), (name, p, moved[need].min())
        assert np.all(moved[~marked] == 0.0)
        checked += int(need.sum())
    assert checked > 3 * 32


def _owners(name, P):
    from oracle import c_oracle as CO

    return CO.locale_idx_of(reference_of(name)[0], P)


@pytest.mark.parametrize("P", [3, 8])
@pytest.mark.parametrize("name", HERMITIAN)
def test_reach_conditions(name, P):
    """blocks of 32 rows, halo 1024, rows [n p / P, n (p + 1) / P): at least one rank leaves blocks unread (so the forced sub-range
    exchange moves fewer bytes than the whole vector), only hubbard_32_1_2_pair_hop needs more than the 16 intervals dist.c keeps"""
    _, H = reference_of(name)
    marks = [marked_blocks(H, P, p) for p in range(P)]
    shares = [float(m.mean()) for m, _ in marks]
    runs = [r for _, r in marks]
    print(f"REACH {name} P={P}: marked share {[round(s, 2) for s in shares]}, runs {runs}")
    assert min(shares) < 1.0
    assert all(s >= 0.2 for s in shares)
    if name == "hubbard_32_1_2_pair_hop":
        assert max(runs) == {3: 24, 8: 28}[P]
    elif name in WIDE:
        assert max(runs) <= 16
    want = reach_of(H, _owners(name, P), P)
    assert [r for _, _, r in want] == runs
    assert all(r <= f for r, f, _ in want) and sum(r for r, _, _ in want) < sum(f for _, f, _ in want)
    assert sum(f for _, f, _ in want) == (P - 1) * ROWS[name].n
