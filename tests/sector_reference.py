"""A sparse explicit-projector reference of an operator restricted to a symmetry sector (numpy + scipy only; no line of the library,
none of the C oracle): what tests/test_gpu_projected_operators.py compares every projected spin path with.

    sector_matrix(cfg) -> (representatives uint64 ascending, H_sector scipy.sparse.csr, leak)

P = |G|^-1 sum_g conj(chi(g)) U_g over the group oracle.model.dense_sector_matrix uses (the closure of the permutations, each element
also composed with the global flip when spin_inversion != 0, characters multiplied), as a sparse matrix from the images of the WHOLE
state array (output bit i = input bit p_i, vectorised); B = the columns P|r>/||P|r>|| over the orbit minima r with norm > 1e-9;
H_sector = B^+ H B.  leak = max |H B - B H_sector| says whether H maps the sector into itself, i.e. commutes with the group: a case
whose operator does not would pass nothing on to a kernel check, so callers assert leak <= 1e-12.

  * number_spins <= 16: H on the full 2^L space is oracle.model.dense_hamiltonian_full -- Kronecker-style, straight from the
    expressions --, P lives on the full space too, so leak also sees an operator that leaves the fixed-weight subspace.
  * number_spins > 16 (fixed weight only): the same projector on the fixed-weight subspace; H there comes from the term tables of
    oracle.model (model.diag / model.offdiag, every term applied to the state array).  THIS BRANCH SHARES THE ORACLE'S EXPRESSION
    COMPILER (oracle.model.terms_from_local_matrices); tests/test_expression_compiler.py pins that compiler against Kronecker
    products, and tests/test_sector_reference.py pins this branch against the first one at sizes both can do.
"""
import functools
import itertools
import json

import numpy as np
import scipy.sparse as sp

from oracle import model as M

NARROW_SITES = 16


def group_elements(model):
    """[(permutation, flip, character)]: the elements dense_sector_matrix sums over, in its order"""
    out = []
    for p, ch in zip(model.group.perms, model.group.chars):
        out.append((p, False, complex(ch)))
        if model.spin_inversion != 0:
            out.append((p, True, complex(ch) * model.spin_inversion))
    return out


def images(perm, states):
    """g.s for the whole array: output bit i = input bit perm[i]"""
    out = np.zeros_like(states)
    for i, src in enumerate(perm):
        out |= ((states >> np.uint64(int(src))) & np.uint64(1)) << np.uint64(i)
    return out


def weight_states(L, w):
    """ascending states of L bits with w set"""
    out = np.array([sum(1 << q for q in c) for c in itertools.combinations(range(L), w)], dtype=np.uint64)
    return np.sort(out)


def hamiltonian_from_terms(model, states):
    """H on the span of `states` (ascending) out of the oracle's term tables: <s ^ x|H|s> += v (-1)^popcount(s & sign mask)
    wherever (s & m) == r.  An image outside `states` is an error: the operator leaves the subspace."""
    n = len(states)
    rows, cols, vals = [], [], []
    for terms in (model.diag, model.offdiag):
        for v, m, r, x, s in zip(terms.v, terms.m, terms.r, terms.x, terms.s):
            act = np.flatnonzero((states & m) == r)
            if len(act) == 0:
                continue
            src = states[act]
            sign = np.ones(len(act))
            sm = src & s
            par = np.zeros(len(act), dtype=np.uint64)
            while sm.any():
                par ^= sm & np.uint64(1)
                sm = sm >> np.uint64(1)
            sign[par == 1] = -1.0
            dst = src ^ x
            j = np.searchsorted(states, dst)
            j[j == n] = 0
            if not np.array_equal(states[j], dst):
                raise AssertionError("a term maps the subspace out of itself")
            rows.append(j)
            cols.append(act)
            vals.append(complex(v) * sign)
    H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    H.sum_duplicates()
    return H


@functools.lru_cache(maxsize=2)
def _full_hamiltonian(L, terms):
    """several sectors of one operator in a row share its 2^L matrix"""
    return M.dense_hamiltonian_full({"basis": {"number_spins": L}, "hamiltonian": {"terms": json.loads(terms)}}).astype(complex)


def sector_matrix(cfg):
    """(representatives, H_sector, leak) -- see the module docstring"""
    model = M.model_from_config(cfg)
    L, hw = model.number_sites, model.hamming_weight
    if L <= NARROW_SITES:
        states = np.arange(1 << L, dtype=np.uint64)
        H = _full_hamiltonian(L, json.dumps(cfg["hamiltonian"]["terms"]))
    else:
        if hw < 0:
            raise ValueError("more than 16 sites: fixed-weight bases only")
        states = weight_states(L, hw)
        H = hamiltonian_from_terms(model, states)
    n = len(states)
    elems = group_elements(model)
    full = np.uint64(model.mask)
    index = np.arange(n)
    least = states.copy()
    rows, vals = [], []
    for perm, flip, ch in elems:
        img = images(perm, states)
        if flip:
            img ^= full
        np.minimum(least, img, out=least)
        j = np.searchsorted(states, img)
        assert np.array_equal(states[j], img)  # (a permutation of the subspace)
        rows.append(j)
        vals.append(np.full(n, np.conj(ch) / len(elems)))
    P = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.tile(index, len(elems)))), shape=(n, n)).tocsc()
    P.sum_duplicates()
    cand = least == states
    if hw >= 0 and L <= NARROW_SITES:
        weight = np.zeros(n, dtype=np.int64)
        for i in range(L):
            weight += ((states >> np.uint64(i)) & np.uint64(1)).astype(np.int64)
        cand &= weight == hw
    cols = P[:, np.flatnonzero(cand)]
    norms = np.sqrt(np.asarray(cols.multiply(cols.conj()).sum(axis=0)).real.ravel())
    keep = norms > 1e-9
    reps = states[np.flatnonzero(cand)[keep]]  # ascending: states is
    B = (cols[:, np.flatnonzero(keep)] @ sp.diags(1.0 / norms[keep])).tocsc()
    HB = (H @ B).tocsc()
    Hs = (B.conj().T @ HB).tocsr()
    Hs.sum_duplicates()
    resid = (HB - B @ Hs).tocoo()
    leak = float(np.abs(resid.data).max()) if resid.nnz else 0.0
    return np.ascontiguousarray(reps, dtype=np.uint64), Hs, leak
