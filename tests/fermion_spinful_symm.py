"""Independent reference for projected spinful-fermion bases (include/ls_hs.h): a site permutation p is lifted to the 2 L modes as
p + p (mode (i, up) = bit i, mode (i, down) = bit i + L), the up <-> down flip is the half swap, the group is closed over the modes
by fermion_symm.closure, every element carries the inversion-count sign of fermion_symm.sign, and representatives, norms and the
projected matrix B+ H B are taken over fermion_jw.product_states with H = fermion_jw.sector_matrix.  Shares no code with config.py
or host.c.  `apply_v` / `sign_v` are fermion_symm.apply / sign over an array of states (the same inversion count, one pair of modes
at a time); tests/test_fermion_spinful_symm_host.py checks them against the scalar ones."""
import numpy as np
import scipy.sparse as sp

from fermion_jw import product_states, sector_matrix
from fermion_symm import closure

ONE = np.uint64(1)


def lift(p, L):
    return [int(v) for v in p] + [int(v) + L for v in p]


def swap(L):
    return [i + L for i in range(L)] + list(range(L))


def group(L, site_generators, sectors, flip=0):
    """[(permutation of the 2 L modes, character)]; flip = +1 / -1 adds the half swap with that character"""
    gens = [lift(p, L) for p in site_generators] + ([swap(L)] if flip else [])
    secs = list(sectors) + ([0 if flip > 0 else 1] if flip else [])
    return closure(2 * L, gens, secs)


def apply_v(p, a):
    out = np.zeros_like(a)
    for i, src in enumerate(p):
        out |= ((a >> np.uint64(src)) & ONE) << np.uint64(i)
    return out


def sign_v(p, a):
    """fermion_symm.sign over an array: the occupied pairs j < j' whose images q_j > q_j' are counted mode by mode"""
    M = len(p)
    q = [0] * M
    for i, src in enumerate(p):
        q[src] = i
    inv = np.zeros(len(a), dtype=np.int64)
    for j in range(M):
        above = sum(1 << jp for jp in range(j + 1, M) if q[j] > q[jp])
        if above:
            inv += ((a >> np.uint64(j)) & ONE).astype(np.int64) * np.bitwise_count(a & np.uint64(above)).astype(np.int64)
    return np.where(inv & 1, -1.0, 1.0)


def state_info_v(grp, a):
    """(orbit minima, conj(chi(g0) sign(g0, a)) of the first minimising element, norms) of an array of states"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    best = np.full(len(a), np.iinfo(np.uint64).max, dtype=np.uint64)
    ch0 = np.zeros(len(a), dtype=complex)
    stab = np.zeros(len(a), dtype=complex)
    for p, ch in grp:
        t = apply_v(p, a)
        cs = ch * sign_v(p, a)
        stab += np.where(t == a, cs, 0.0)
        less = t < best
        best = np.where(less, t, best)
        ch0 = np.where(less, np.conj(cs), ch0)
    n2 = stab.real / len(grp)
    return best, ch0, np.where(n2 > 1e-12, np.sqrt(np.maximum(n2, 0.0)), 0.0)


def representatives(L, n_up, n_dn, grp):
    """ascending orbit minima with non-zero norm among the product states, and their norms"""
    states = product_states(L, n_up, n_dn)
    rep, _, norm = state_info_v(grp, states)
    keep = (rep == states) & (norm > 0)
    return states[keep], norm[keep]


def projector_columns(L, n_up, n_dn, grp, reps):
    """B (sparse): column r = P|r> / ||P|r>||, P = |G|^-1 sum_g conj(chi(g)) U_g, U_g|a> = sign(g, a)|g.a>, on the product states"""
    states = product_states(L, n_up, n_dn)
    reps = np.ascontiguousarray(reps, dtype=np.uint64)
    rows, cols, vals = [], [], []
    for p, ch in grp:
        t = apply_v(p, reps)
        pos = np.searchsorted(states, t)
        assert np.array_equal(states[pos], t)
        rows.append(pos)
        cols.append(np.arange(len(reps)))
        vals.append(np.conj(ch) * sign_v(p, reps) / len(grp))
    B = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(states), len(reps)), dtype=complex)
    nrm = np.sqrt(np.asarray(B.multiply(B.conj()).sum(axis=0)).ravel().real)
    return states, B @ sp.diags(1.0 / nrm)


def projected_matrix(model, L, n_up, n_dn, grp, reps, dense=True):
    """B+ H B (dense, or as a scipy CSR matrix for the larger sectors)"""
    states, B = projector_columns(L, n_up, n_dn, grp, reps)
    H = sector_matrix(model, L, True, states)
    M = (B.conj().T @ H @ B).tocsr()
    return M.toarray() if dense else M


def as_spinless(model, L):
    """the same monomials written for a spinless basis on the 2 L modes: (site, spin) -> mode site + L spin"""
    return [(coef, [(kind, site + L * spin, 0) for kind, site, spin in ops]) for coef, ops in model]


def exchange_model(bonds, J=0.6):
    """J sum_<ij> (c+_i↑ c_i↓ c+_j↓ c_j↑ + h.c.): the transverse spin exchange S+_i S-_j + h.c. -- every monomial touches both
    species, so its Jordan-Wigner strings cross the halves of the word"""
    model = []
    for i, j in bonds:
        model.append((J, [("+", i, 0), ("-", i, 1), ("+", j, 1), ("-", j, 0)]))
        model.append((J, [("+", j, 0), ("-", j, 1), ("+", i, 1), ("-", i, 0)]))
    return model


def pair_hopping_model(bonds, P=0.4):
    """P sum_<ij> (c+_i↑ c+_i↓ c_j↓ c_j↑ + h.c.)"""
    model = []
    for i, j in bonds:
        model.append((P, [("+", i, 0), ("+", i, 1), ("-", j, 1), ("-", j, 0)]))
        model.append((P, [("+", j, 0), ("+", j, 1), ("-", i, 1), ("-", i, 0)]))
    return model


def free_spinful_ring_energy(L, n_up, n_dn, s, free_ring_energy):
    """lowest energy of the U = 0 ring at total momentum s: the species are independent"""
    return min(free_ring_energy(L, n_up, s1) + free_ring_energy(L, n_dn, (s - s1) % L) for s1 in range(L))
