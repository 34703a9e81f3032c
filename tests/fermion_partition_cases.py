"""The fixed table of UNPROJECTED fermionic bases -- spinless at fixed N, spinful at fixed N, the spinful (N_up, N_down) product
basis -- that tests/test_gpu_fermion_partitions.py runs through the partitioned and multi-rank matvec paths (packets in one
process, replicated-x plans, the two drivers of csrc/dist.c) and tests/test_fermion_partition_cases.py validates without a GPU.
The reference of every row is fermion_jw.sector_matrix, which shares no code with the library.  What each row is there for:

  spinless_open_33_3            exchange pairs only on 64-bit words: sorted streams (u32 global-rank keys over 64-bit states), the staged
                                chain kernel on a rank's contiguous rows (chain_row0 != 0)
  spinless_long_40_3[_complex]  Jordan-Wigner strings across bit 32, real and complex coefficients
  spinless_ring_64_2            the 62-mode string of the closing bond, bit 63; no diagonal: y is accumulated into
  spinless_ring_36_33           weight 33, the last row of the binomial table: too heavy for the pre-indexed packets
  hubbard_ring_17_2_2[_free]    the product basis (no single weight: searched global index, 8-byte packet keys); _free has no diagonal
  hubbard_32_1_2_pair_hop       non-separable product basis, bit 63; a rank whose reach has more than 16 runs of blocks
  spinful_17_n3_flips           N alone fixed: one weight on 2 L = 34 modes
  spinless_open_16_8            the 32-bit twin of spinless_open_33_3
  spinless_ring_16_7_peierls    complex amplitudes, a signed closing bond, 32-bit words
  spinless_directed_16_8        directed hopping: the one non-Hermitian row (a real matrix)
  hubbard_ring_8_4_4, hubbard_8_3_4_pair_hop, spinful_8_n5_flips   the three spinful kinds on 16 modes
"""
import functools
from dataclasses import dataclass

import numpy as np

from fermion_jw import hubbard_model, ring, sector_matrix
from fermion_wide import CASES as WIDE_CASES
from fermion_wide import Wide, pair_hop, spin_flips, spinless_chain

_DIRECTED_16 = ([(-1.0, [("+", i, 0), ("-", (i + 1) % 16, 0)]) for i in range(16)]
                + [(0.5, [("n", i, 0), ("n", (i + 1) % 16, 0)]) for i in range(16)])

NARROW_CASES = {
    "spinless_open_16_8": Wide(16, False, 8, None, tuple(spinless_chain(16, [(i, i + 1) for i in range(15)], V=1.3))),
    "spinless_ring_16_7_peierls": Wide(16, False, 7, None, tuple(spinless_chain(16, ring(16), t=-np.exp(0.21j), V=0.5))),
    "spinless_directed_16_8": Wide(16, False, 8, None, tuple(_DIRECTED_16)),
    "hubbard_ring_8_4_4": Wide(8, True, 8, 4, tuple(hubbard_model(8, ring(8), t=1.0, U=4.0))),
    "hubbard_8_3_4_pair_hop": Wide(8, True, 7, 3, tuple(hubbard_model(8, ring(8), t=1.0, U=2.0) + pair_hop(0, 7, 0.5))),
    "spinful_8_n5_flips": Wide(8, True, 5, None, tuple(hubbard_model(8, ring(8), U=2.0) + spin_flips(8, 7, 0))),
}


@dataclass(frozen=True)
class Row:
    case: Wide
    is_real: bool       # the MATRIX is real
    is_hermitian: bool
    has_diagonal: bool  # any diagonal term at all (without one the matvec accumulates into y)
    n: int              # number of basis states


def _wide(name, is_real, has_diagonal, n):
    return Row(WIDE_CASES[name], is_real, True, has_diagonal, n)


ROWS = {
    "spinless_open_33_3": _wide("spinless_open_33_3", True, True, 5456),
    "spinless_long_40_3": _wide("spinless_long_40_3", True, True, 9880),
    "spinless_long_40_3_complex": _wide("spinless_long_40_3_complex", False, True, 9880),
    "spinless_ring_64_2": _wide("spinless_ring_64_2", True, False, 2016),
    "spinless_ring_36_33": _wide("spinless_ring_36_33", True, True, 7140),
    "hubbard_ring_17_2_2": _wide("hubbard_ring_17_2_2", True, True, 18496),
    "hubbard_ring_17_2_2_free": _wide("hubbard_ring_17_2_2_free", True, False, 18496),
    "hubbard_32_1_2_pair_hop": _wide("hubbard_32_1_2_pair_hop", True, True, 15872),
    "spinful_17_n3_flips": _wide("spinful_17_n3_flips", True, True, 5984),
    "spinless_open_16_8": Row(NARROW_CASES["spinless_open_16_8"], True, True, True, 12870),
    "spinless_ring_16_7_peierls": Row(NARROW_CASES["spinless_ring_16_7_peierls"], False, True, True, 11440),
    "spinless_directed_16_8": Row(NARROW_CASES["spinless_directed_16_8"], True, False, True, 12870),
    "hubbard_ring_8_4_4": Row(NARROW_CASES["hubbard_ring_8_4_4"], True, True, True, 4900),
    "hubbard_8_3_4_pair_hop": Row(NARROW_CASES["hubbard_8_3_4_pair_hop"], True, True, True, 3920),
    "spinful_8_n5_flips": Row(NARROW_CASES["spinful_8_n5_flips"], True, True, True, 4368),
}
ALL = list(ROWS)
WIDE = [name for name in ALL if name in WIDE_CASES]
NARROW = list(NARROW_CASES)
HERMITIAN = [name for name, row in ROWS.items() if row.is_hermitian]
NON_HERMITIAN = [name for name, row in ROWS.items() if not row.is_hermitian]
COMPLEX = [name for name, row in ROWS.items() if not row.is_real]
NO_DIAGONAL = [name for name, row in ROWS.items() if not row.has_diagonal]
PRODUCT = [name for name, row in ROWS.items() if row.case.spinful and row.case.n_up is not None]  # no single weight
FIXED_WEIGHT = [name for name in ALL if name not in PRODUCT]
EXCHANGE_ONLY = ["spinless_open_33_3", "spinless_open_16_8"]  # open chains: every hop joins adjacent modes, no string anywhere


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """(basis states ascending, H on them as scipy.sparse.csr) of a row, computed once per process"""
    case = ROWS[name].case
    states = case.states()
    return states, sector_matrix(list(case.model), case.L, case.spinful, states).tocsr()


def vectors(name, cplx, seed):
    """(x, y0) of a matvec of the row: x uniform in [-0.5, 0.5) (both parts when complex).  A row with a diagonal ASSIGNS y, so its
    y0 is garbage that must not survive; a row without one accumulates, so its y0 is a non-trivial vector and y = H x + y0."""
    row = ROWS[name]
    rs = np.random.RandomState(seed)
    x = rs.rand(row.n) - 0.5
    if cplx:
        x = x + 1j * (rs.rand(row.n) - 0.5)
    if row.has_diagonal:
        return x, np.full(row.n, 3.0, dtype=x.dtype)
    y0 = np.cos(0.77 * np.arange(row.n) + seed).astype(x.dtype)
    if cplx:
        y0 = y0 + 1j * np.sin(0.31 * np.arange(row.n))
    return x, y0


def marked_blocks(H, P, p, shift=5, halo=1024):
    """the blocks of 2^shift rows of the global vector that rank p of P reads in the replicated-x exchange, out of the REFERENCE matrix
    alone (csrc/dist.c setup_reach, host.c ls_amd_internal_plan_reach): rank p computes the global rows [n p / P, n (p + 1) / P) and
    reads every block that holds a column of a non-zero entry of those rows, and its own rows with `halo` = 1024 rows either side
    (REACH_HALO).  Returns (one flag per block, number of runs of marked blocks)."""
    n = H.shape[0]
    n0, n1 = n * p // P, n * (p + 1) // P
    rows = H[n0:n1]
    marked = np.zeros(((n - 1) >> shift) + 1, dtype=bool)
    marked[np.unique(rows.indices[np.abs(rows.data) > 1e-12] >> shift)] = True  # (a rounding residue is no entry)
    marked[max(0, n0 - halo) >> shift : ((min(n, n1 + halo) - 1) >> shift) + 1] = True
    runs = int((np.diff(np.concatenate([[0], marked.astype(int)])) == 1).sum())
    return marked, runs


def reach_of(H, owner, P, shift=5, halo=1024):
    """what the sub-range exchange has to deliver: rank p receives the elements of its marked blocks that other ranks own (x is owned
    by hash partition, `owner` = the owner of every state in ascending order).  Per rank: (elements received, elements of the other
    ranks in all, runs of marked blocks)"""
    n = H.shape[0]
    owner = np.asarray(owner)
    out = []
    for p in range(P):
        marked, runs = marked_blocks(H, P, p, shift, halo)
        reached = np.repeat(marked, 1 << shift)[:n]
        out.append((int((reached & (owner != p)).sum()), int((owner != p).sum()), runs))
    return out
