"""Independent Jordan-Wigner construction of fermionic operators for the fermion tests: c_k = Z x ... x Z x a x 1 x ... x 1
as Kronecker products (mode k = bit k of the occupation word; the Z string runs over the modes below k), and a model language
that produces both the YAML expression and the dense matrix from one description."""
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
    if N < 0:
        return np.arange(2 ** M, dtype=np.uint64)
    return np.array(sorted(sum(1 << i for i in c) for c in itertools.combinations(range(M), N)), dtype=np.uint64)


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
