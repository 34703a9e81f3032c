"""Fermionic cases wider than 32 modes, or whose words cross bit 32, shared by the CPU check of the compiled terms
(test_fermion_sector_reference.py) and the GPU tests (test_gpu_fermions_wide.py).  Every case stays below ~20 k states so that
its reference, `fermion_jw.sector_matrix`, is cheap."""
from dataclasses import dataclass

import numpy as np

from fermion_jw import hubbard_model, product_states, ring, spinful_states, weight_states, yaml_terms


@dataclass(frozen=True)
class Wide:
    L: int
    spinful: bool
    N: int
    n_up: object  # spinful: N_up of the product basis, or None when N alone is fixed
    model: tuple

    @property
    def is_real(self):
        return all(complex(c).imag == 0 for c, _ in self.model)

    def states(self):
        if not self.spinful:
            return weight_states(self.L, self.N)
        if self.n_up is None:
            return spinful_states(self.L, self.N)
        return product_states(self.L, self.n_up, self.N - self.n_up)

    def config(self):
        basis = {"particle": "spinful-fermion" if self.spinful else "spinless-fermion", "number_sites": self.L,
                 "number_particles": self.N}
        if self.spinful:
            basis["number_up"] = self.n_up
        return {"basis": basis, "hamiltonian": {"terms": yaml_terms(list(self.model), self.spinful)}}


def hop(i, j, t, spin=0):
    """t c†_i c_j + h.c."""
    return [(t, [("+", i, spin), ("-", j, spin)]), (np.conj(t), [("+", j, spin), ("-", i, spin)])]


def spinless_chain(L, bonds, t=-1.0, V=0.0):
    model = []
    for i, j in bonds:
        model += hop(i, j, t)
        if V:
            model.append((V, [("n", i, 0), ("n", j, 0)]))
    return model


def pair_hop(i, j, g):
    """g c†_i↑ c†_i↓ c_j↓ c_j↑ + h.c.: a doubly occupied site moves from j to i"""
    return [(g, [("+", i, 0), ("+", i, 1), ("-", j, 1), ("-", j, 0)]), (g, [("+", j, 0), ("+", j, 1), ("-", i, 1), ("-", i, 0)])]


def spin_flips(L, i, j, g=0.7, h=0.4):
    """h c†_i↑ c_i↓ + h.c. (changes N_up) and the exchange g c†_i↑ c_i↓ c†_j↓ c_j↑ + h.c.: both cross the species halves"""
    return ([(h, [("+", i, 0), ("-", i, 1)]), (h, [("+", i, 1), ("-", i, 0)])]
            + [(g, [("+", i, 0), ("-", i, 1), ("+", j, 1), ("-", j, 0)]), (g, [("+", j, 0), ("-", j, 1), ("+", i, 1), ("-", i, 0)])])


def _open(L):
    return [(i, i + 1) for i in range(L - 1)]


_LONG_40 = spinless_chain(40, ring(40), V=0.7) + hop(3, 35, -0.45) + hop(30, 33, 0.55) + hop(0, 39, -0.3)
_HUB_32 = hubbard_model(32, ring(32), t=1.0, U=3.0, V=0.6, phase=0.29)

CASES = {
    # spinless: single words of 33..64 modes
    "spinless_open_33_3": Wide(33, False, 3, None, tuple(spinless_chain(33, _open(33), V=1.3))),
    "spinless_long_40_3": Wide(40, False, 3, None, tuple(_LONG_40)),
    "spinless_long_40_3_complex": Wide(40, False, 3, None, tuple(_LONG_40 + hop(31, 32, 0.3 + 0.4j))),
    "spinless_ring_64_2": Wide(64, False, 2, None, tuple(spinless_chain(64, ring(64)))),
    "spinless_ring_36_33": Wide(36, False, 33, None, tuple(spinless_chain(36, ring(36), V=0.9))),
    "spinless_ring_48_1": Wide(48, False, 1, None, tuple(spinless_chain(48, ring(48), V=0.9) + [(0.25, [("n", 47, 0)])])),
    "spinless_ring_48_0": Wide(48, False, 0, None, tuple(spinless_chain(48, ring(48), V=0.9) + [(0.25, [("n", 47, 0)])])),
    # spinful product bases: the down half at bits L..2L-1
    "hubbard_ring_17_2_2": Wide(17, True, 4, 2, tuple(hubbard_model(17, ring(17), t=1.0, U=4.0))),
    "hubbard_ring_17_2_2_free": Wide(17, True, 4, 2, tuple(hubbard_model(17, ring(17), t=1.0, U=0.0))),
    "hubbard_ring_17_2_2_peierls": Wide(17, True, 4, 2, tuple(hubbard_model(17, ring(17), t=1.0, U=4.0, phase=0.37))),
    "hubbard_32_1_2": Wide(32, True, 3, 1, tuple(_HUB_32)),
    "hubbard_32_2_1": Wide(32, True, 3, 2, tuple(_HUB_32)),
    "hubbard_32_1_2_pair_hop": Wide(32, True, 3, 1, tuple(hubbard_model(32, ring(32), t=1.0, U=2.0) + pair_hop(0, 31, 0.5))),
    "hubbard_32_0_2": Wide(32, True, 2, 0, tuple(hubbard_model(32, ring(32), t=1.0, U=2.0, V=0.4))),
    "hubbard_32_2_0": Wide(32, True, 2, 2, tuple(hubbard_model(32, ring(32), t=1.0, U=2.0, V=0.4))),
    "hubbard_20_20_1": Wide(20, True, 21, 20, tuple(hubbard_model(20, ring(20), t=1.0, U=2.5, V=0.3))),
    # spinful with N alone fixed: one word of 2 L modes, either side of 32 bits
    "spinful_16_n3_flips": Wide(16, True, 3, None, tuple(hubbard_model(16, ring(16), U=2.0) + spin_flips(16, 15, 0))),
    "spinful_17_n3_flips": Wide(17, True, 3, None, tuple(hubbard_model(17, ring(17), U=2.0) + spin_flips(17, 16, 0))),
}
