"""Independent Jordan-Wigner construction of fermionic operators for the fermion tests: c_k = Z x ... x Z x a x 1 x ... x 1
as Kronecker products (mode k = bit k of the occupation word; the Z string runs over the modes below k), and a model language
that produces both the YAML expression and the dense matrix from one description.  `sector_matrix` builds the same operator on a
list of occupation words instead of 2^M, so it reaches 64 modes; it shares nothing with the compiler in config.py."""
import itertools

import numpy as np
import scipy.sparse as sp

_A = sp.csr_matrix(np.array([[0.0, 1.0], [0.0, 0.0]]))  # |0><1| on one mode (basis order |0>, |1>)
_Z = sp.csr_matrix(np.diag([1.0, -1.0]))
_I = sp.identity(2, format="csr")
_SUB = "₀₁₂₃₄₅₆₇₈₉"
ARROW = {0: "↑", 1: "↓"}


def annihilator(k: int, modes: int):
    """c_k on `modes` modes; Kronecker order: the first factor is the most significant bit."""
    out = sp.identity(1, format="csr")
    for q in reversed(range(modes)):
        out = sp.kron(out, _A if q == k else (_Z if q < k else _I), format="csr")
    return out


def mode_of(site: int, spin, L: int) -> int:
    return site + (L if spin == 1 else 0)


def dense(model, L: int, spinful: bool):
    """model: [(coefficient, [(kind in '+-n', site, spin), ...])] (operators written left to right)."""
    M = 2 * L if spinful else L
    c = [annihilator(k, M) for k in range(M)]
    H = sp.csr_matrix((2 ** M, 2 ** M), dtype=complex)
    for coef, ops in model:
        term = sp.identity(2 ** M, format="csr", dtype=complex)
        for kind, site, spin in ops:
            ck = c[mode_of(site, spin, L)]
            op = ck.T if kind == "+" else (ck if kind == "-" else ck.T @ ck)
            term = term @ op
        H = H + coef * term
    return H


def yaml_terms(model, spinful: bool):
    """The same model as `expression` + `sites` terms: one term per monomial, local site k <-> the k-th distinct site."""
    out = []
    for coef, ops in model:
        sites = []
        for _, s, _ in ops:
            if s not in sites:
                sites.append(s)
        toks = []
        for kind, s, spin in ops:
            name = {"+": "c†", "-": "c", "n": "n"}[kind]
            toks.append(name + _SUB[sites.index(s)] + (ARROW[spin] if spinful else ""))
        z = complex(coef)
        scalar = repr(z.real) if z.imag == 0 else f"{z.real!r}{z.imag:+.17g}j"
        out.append({"expression": scalar + " × " + " ".join(toks), "sites": [sites]})
    return out


def product_states(L: int, n_up: int, n_dn: int):
    """The spinful (N_up, N_down) basis in ascending order (b outer, a inner), by itertools."""
    def words(w):
        return sorted(sum(1 << i for i in c) for c in itertools.combinations(range(L), w))
    return np.array([(b << L) | a for b in words(n_dn) for a in words(n_up)], dtype=np.uint64)


def weight_states(M: int, N: int):
    """all M-mode words of weight N in ascending order (every word when N < 0)"""
    if N < 0:
        return np.arange(2 ** M, dtype=np.uint64)
    return np.array(sorted(sum(1 << i for i in c) for c in itertools.combinations(range(M), N)), dtype=np.uint64)


def spinful_states(L: int, N: int):
    """The spinful basis with N alone fixed: every weight-N word of the 2 L modes, in ascending order."""
    return weight_states(2 * L, N)


def restrict(H, states):
    idx = states.astype(np.int64)
    return H[idx][:, idx]


def apply_terms(terms, states):
    """Dense matrix of compiled terms (v, m, r, x, s) on `states`, by the rule of include/ls_hs.h."""
    pos = {int(s): i for i, s in enumerate(states)}
    H = np.zeros((len(states), len(states)), dtype=complex)
    for j, a in enumerate(states):
        a = int(a)
        for v, m, r, x, s in terms:
            if (a & m) == r:
                b = a ^ x
                if b in pos:
                    H[pos[b], j] += v * (-1) ** bin(a & s).count("1")
    return H


def sector_matrix(model, L: int, spinful: bool, states):
    """<states|H|states> as a scipy CSR matrix, by acting with each monomial on the occupation words themselves: operators are
    applied right to left; c_k and c†_k need bit k set (clear), multiply by (-1)^(occupied modes below k) and flip bit k; n_k
    needs bit k set.  A result outside `states` is dropped; `states` must not be empty.  Vectorised over the states with uint64
    words, so it reaches 64 modes at the cost of the sector, not of 2^M."""
    states = np.ascontiguousarray(states, dtype=np.uint64)
    n = len(states)
    order = np.argsort(states, kind="stable")
    ordered = states[order]
    one = np.uint64(1)
    rows, cols, vals = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, complex)]
    for coef, ops in model:
        a = states.copy()
        alive = np.ones(n, dtype=bool)
        odd = np.zeros(n, dtype=bool)
        for kind, site, spin in reversed(ops):
            k = site + (L if spinful and spin == 1 else 0)
            assert 0 <= k < (2 * L if spinful else L) <= 64, (kind, site, spin)
            bit = one << np.uint64(k)
            occupied = (a & bit) != 0
            if kind == "n":
                alive &= occupied
                continue
            alive &= occupied if kind == "-" else ~occupied
            odd ^= (np.bitwise_count(a & (bit - one)) & 1).astype(bool)
            a = a ^ bit
        pos = np.minimum(np.searchsorted(ordered, a), n - 1)
        hit = alive & (ordered[pos] == a)
        rows.append(order[pos[hit]])
        cols.append(np.nonzero(hit)[0])
        vals.append(np.where(odd[hit], -1.0, 1.0) * complex(coef))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n), dtype=complex)


def terms_matrix(terms, states):
    """Sparse matrix of compiled terms (v, m, r, x, s) on `states`, by the rule of include/ls_hs.h -- `apply_terms` vectorised
    for sectors too large for a dense matrix."""
    states = np.ascontiguousarray(states, dtype=np.uint64)
    n = len(states)
    order = np.argsort(states, kind="stable")
    ordered = states[order]
    rows, cols, vals = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, complex)]
    for v, m, r, x, s in terms:
        act = (states & np.uint64(m)) == np.uint64(r)
        b = states ^ np.uint64(x)
        pos = np.minimum(np.searchsorted(ordered, b), n - 1)
        hit = act & (ordered[pos] == b)
        odd = (np.bitwise_count(states[hit] & np.uint64(s)) & 1).astype(bool)
        rows.append(order[pos[hit]])
        cols.append(np.nonzero(hit)[0])
        vals.append(np.where(odd, -1.0, 1.0) * complex(v))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n), dtype=complex)


def hubbard_model(L: int, bonds, t=1.0, U=4.0, V=0.0, phase=0.0):
    hop = -t * np.exp(1j * phase)
    model = []
    for i, j in bonds:
        for s in (0, 1):
            model.append((hop, [("+", i, s), ("-", j, s)]))
            model.append((np.conj(hop), [("+", j, s), ("-", i, s)]))
        if V:
            for s1 in (0, 1):
                for s2 in (0, 1):
                    model.append((V, [("n", i, s1), ("n", j, s2)]))
    if U:
        for i in range(L):
            model.append((U, [("n", i, 0), ("n", i, 1)]))
    return model


def ring(L):
    return [(i, (i + 1) % L) for i in range(L)]


def square(w, h):
    bonds = []
    for y in range(h):
        for x in range(w):
            s = y * w + x
            if w > 1 and (w > 2 or x == 0):
                bonds.append((s, y * w + (x + 1) % w))
            if h > 1 and (h > 2 or y == 0):
                bonds.append((s, ((y + 1) % h) * w + x))
    return bonds
