"""The sector reference (fermion_jw.sector_matrix) against the dense Jordan-Wigner matrix on every small model and kind of
basis, against hand-computed signs at 64 modes, and the expression compiler's terms against it on the wide cases of
fermion_wide.py (33..64 modes, where no dense matrix fits)."""
import numpy as np
import pytest

from distributed_matvec_amd import config
from fermion_jw import (dense, hubbard_model, product_states, restrict, ring, sector_matrix, spinful_states, terms_matrix,
                        weight_states)
from fermion_wide import CASES
from test_fermion_compiler import SPINFUL, SPINLESS
from test_gpu_fermions import HUBBARD


def assert_same(got, want, what):
    got, want = got.toarray(), np.asarray(want.toarray() if hasattr(want, "toarray") else want)
    assert got.shape == want.shape, what
    assert np.abs(got - want).max(initial=0.0) < 1e-12, what


@pytest.mark.parametrize("name", sorted(SPINLESS))
@pytest.mark.parametrize("N", [-1, 0, 1, 3, 8])
def test_spinless_sector_equals_dense(name, N):
    L = 8
    states = weight_states(L, N)
    assert_same(sector_matrix(SPINLESS[name], L, False, states), restrict(dense(SPINLESS[name], L, False), states), (name, N))


@pytest.mark.parametrize("name", sorted(SPINFUL))
def test_spinful_sector_equals_dense(name):
    L = 4 if name != "hubbard_ring_3" else 3
    model = SPINFUL[name]
    H = dense(model, L, True)
    bases = [product_states(L, nu, nd) for nu, nd in ((1, 1), (2, 1), (1, 3), (0, 2), (L, 1), (0, 0), (L, L))]
    bases += [spinful_states(L, N) for N in (1, 3, 2 * L)] + [np.arange(2 ** (2 * L), dtype=np.uint64)]
    for states in bases:
        assert_same(sector_matrix(model, L, True, states), restrict(H, states), (name, len(states)))


@pytest.mark.parametrize("name", sorted(HUBBARD))
def test_hubbard_sector_equals_dense(name):
    L, nu, nd, model = HUBBARD[name]
    H = dense(model, L, True)
    for states in (product_states(L, nu, nd), spinful_states(L, nu + nd)):
        assert_same(sector_matrix(model, L, True, states), restrict(H, states), (name, len(states)))


def test_signs_at_64_modes_by_hand():
    """c†_63 c_0 and c†_0 c_63 on 64 modes: the string is the 62 modes between the two ends, bit 63 included in the words"""
    model = [(1.0, [("+", 63, 0), ("-", 0, 0)]), (2.0, [("+", 0, 0), ("-", 63, 0)]), (0.5, [("n", 63, 0)])]
    w = lambda *bits: sum(1 << b for b in bits)
    states = np.array(sorted([w(0, 5, 40), w(5, 40, 63), w(0, 5, 40, 62), w(5, 40, 62, 63), w(31, 32)]), dtype=np.uint64)
    H = sector_matrix(model, 64, False, states).toarray()
    at = {int(s): i for i, s in enumerate(states)}
    assert H[at[w(5, 40, 63)], at[w(0, 5, 40)]] == 1.0  # two modes in between: even
    assert H[at[w(5, 40, 62, 63)], at[w(0, 5, 40, 62)]] == -1.0  # three: odd
    assert H[at[w(0, 5, 40)], at[w(5, 40, 63)]] == 2.0
    assert H[at[w(0, 5, 40, 62)], at[w(5, 40, 62, 63)]] == -2.0
    assert H[at[w(5, 40, 63)], at[w(5, 40, 63)]] == 0.5 and H[at[w(0, 5, 40)], at[w(0, 5, 40)]] == 0.0
    assert np.count_nonzero(H) == 6 and not H[at[w(31, 32)]].any()


def test_spinful_down_half_at_the_top_bits():
    """(i, down) is bit i + L: on L = 32, c†_31↓ c_0↑ crosses the 31 up modes above 0 and the down modes below 31"""
    L = 32
    model = [(1.0, [("+", 31, 1), ("-", 0, 0)])]
    src = (1 << 0) | (1 << 7) | (1 << 32) | (1 << 40)  # up 0, 7; down 0, 8
    dst = (1 << 7) | (1 << 32) | (1 << 40) | (1 << 63)
    states = np.array(sorted([src, dst]), dtype=np.uint64)
    H = sector_matrix(model, L, True, states).toarray()
    i, j = list(states).index(dst), list(states).index(src)
    assert H[i, j] == -1.0  # three occupied modes (7, 32, 40) below 63 after c_0 removed mode 0
    assert H[j, i] == 0.0


def _compiled(case):
    cfg = case.config()
    return config.parse_operator(cfg["hamiltonian"], config.parse_basis(cfg)).terms


@pytest.mark.parametrize("name", sorted(CASES))
def test_compiled_wide_terms_equal_sector_reference(name):
    case = CASES[name]
    states = case.states()
    want = sector_matrix(list(case.model), case.L, case.spinful, states)
    assert_same(terms_matrix(_compiled(case), states), want, name)
    assert (abs(want - want.getH()) > 1e-14).nnz == 0, name  # every wide model is Hermitian


def test_wide_cases_reach_what_they_are_for():
    """the cases touch what the GPU file needs them for: bit 63, a string across bit 32, an empty and a full species, the
    binomial table's last weight"""
    c = CASES
    assert int(c["spinless_ring_64_2"].states()[-1]) >> 63 == 1
    assert len(c["spinless_ring_36_33"].states()) == 7140 and c["spinless_ring_36_33"].N == 33
    assert len(c["hubbard_32_1_2"].states()) == 15872 and any(int(s) >> 63 for s in c["hubbard_32_1_2"].states())
    assert len(c["hubbard_32_0_2"].states()) == 496 and len(c["hubbard_20_20_1"].states()) == 20
    assert len(c["spinful_16_n3_flips"].states()) == 4960 and len(c["spinful_17_n3_flips"].states()) == 5984
    assert len(c["hubbard_ring_17_2_2"].states()) == 18496
    strings = [s for *_, s in _compiled(c["spinless_long_40_3"])]
    assert any(s >> 31 & 1 and s >> 32 & 1 for s in strings)
    assert any(s >> 62 & 1 for s in (s for *_, s in _compiled(c["spinless_ring_64_2"])))
    assert max(len(w.states()) for w in c.values()) <= 20000
