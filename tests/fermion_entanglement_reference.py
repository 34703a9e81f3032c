"""Reference for the expansion and the entanglement of fermionic sector states: pure numpy / scipy on the independent references
tests/fermion_symm.py, tests/fermion_spinful_symm.py and tests/fermion_jw.py, nothing of the library.

A `Case` is a fermionic basis: spinless (L modes, N fixed or not) or the spinful (N_up, N_down) product basis (2 L modes), with site
generators, their sectors and the up <-> down flip.  Its full vector is  projector columns @ psi  over the states of the same basis
without symmetries -- column r = P|r> / |P|r>|, P = |G|^-1 sum_g conj(chi(g)) U_g, U_g|a> = sign(g, a)|g.a> -- built here for any
case from fermion_spinful_symm.apply_v / sign_v (the inversion count over an array of words); tests/test_fermion_entanglement_host.py
checks it against fermion_symm.projector_columns and fermion_spinful_symm.projector_columns.

The bipartition of a full vector: with |n> = c+_{k1} ... c+_{kN}|0>, k1 < ... < kN and |a>_A|b>_B the same product with the modes of
A in front, |n> = sigma(n)|a>|b>, sigma(n) = (-1)^#{(i, j): i in A, j in B, both occupied, j < i} -- counted pair by pair here."""
import functools

import numpy as np
import scipy.sparse as sp

import fermion_jw as JW
import fermion_spinful_symm as FS
import fermion_symm as F

ONE = np.uint64(1)


class Case:
    def __init__(self, L, N=None, up=None, gens=(), secs=(), flip=0):
        """spinless: N particles on L modes (None: every N); spinful: up = (N_up, N_down) on L sites"""
        self.L, self.N, self.up = L, N, up
        self.spinful = up is not None
        self.M = 2 * L if self.spinful else L
        self.gens, self.secs, self.flip = [list(g) for g in gens], list(secs), flip

    def basis_config(self):
        syms = [{"permutation": list(p), "sector": int(s)} for p, s in zip(self.gens, self.secs)]
        if self.spinful:
            basis = {"particle": "spinful-fermion", "number_sites": self.L, "number_particles": sum(self.up), "number_up": self.up[0],
                     "symmetries": syms}
            if self.flip:
                basis["spin_flip"] = self.flip
        else:
            basis = {"particle": "spinless-fermion", "number_sites": self.L, "symmetries": syms}
            if self.N is not None:
                basis["number_particles"] = self.N
        return basis

    def config(self, model=None):
        cfg = {"basis": self.basis_config()}
        if model is not None:
            cfg["hamiltonian"] = {"terms": JW.yaml_terms(model, self.spinful)}
        return cfg

    def plain(self):
        """the same basis without symmetries"""
        return Case(self.L, self.N, self.up)

    @functools.cached_property
    def group(self):
        if not self.gens and not self.flip:
            return [(tuple(range(self.M)), 1.0 + 0j)]
        return FS.group(self.L, self.gens, self.secs, self.flip) if self.spinful else F.closure(self.L, self.gens, self.secs)

    @functools.cached_property
    def states(self):
        s = JW.product_states(self.L, *self.up) if self.spinful else JW.weight_states(self.L, -1 if self.N is None else self.N)
        s.setflags(write=False)
        return s

    @functools.cached_property
    def _reps_norms(self):
        rep, _, norm = FS.state_info_v(self.group, self.states)
        keep = (rep == self.states) & (norm > 0)
        return self.states[keep], norm[keep]

    @property
    def reps(self): return self._reps_norms[0]

    @functools.cached_property
    def columns(self):
        """B (sparse CSR, states x reps): the projector columns, every U_g entry signed"""
        reps, grp = self.reps, self.group
        rows, cols, vals = [], [], []
        for p, ch in grp:
            t = FS.apply_v(p, reps)
            pos = np.searchsorted(self.states, t)
            assert np.array_equal(self.states[pos], t)
            rows.append(pos)
            cols.append(np.arange(len(reps)))
            vals.append(np.conj(ch) * FS.sign_v(p, reps) / len(grp))
        B = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(self.states), len(reps)), dtype=complex)
        nrm = np.sqrt(np.asarray(B.multiply(B.conj()).sum(axis=0)).ravel().real)
        assert (nrm > 1e-9).all()
        return (B @ sp.diags(1.0 / nrm)).tocsr()

    @functools.cached_property
    def live(self):
        """the states that some orbit of non-zero norm reaches"""
        out = np.zeros(len(self.states), dtype=bool)
        for p, _ in self.group:
            out[np.searchsorted(self.states, FS.apply_v(p, self.reps))] = True
        return out

    def full_vector(self, psi):
        return self.columns @ np.asarray(psi)

    def modes_of(self, sites=None, modes=None):
        """the sorted modes of a subsystem given as FermionSectorExpansion takes it"""
        assert sites is None or modes is None
        if modes is not None:
            return sorted(int(m) for m in modes)
        if sites is None:
            return list(range(self.M))
        return sorted([int(s) for s in sites] + ([int(s) + self.L for s in sites] if self.spinful else []))

    def sector_matrix(self, model):
        """B+ H B (dense) with H from fermion_jw.sector_matrix over the unprojected states"""
        H = JW.sector_matrix(model, self.L, self.spinful, self.states)
        return (self.columns.conj().T @ H @ self.columns).toarray()

    def ground_state(self, model):
        """(E0, psi) of the sector, by numpy eigh"""
        Hs = self.sector_matrix(model)
        assert np.abs(Hs - Hs.conj().T).max() < 1e-12
        w, v = np.linalg.eigh(Hs)
        return float(w[0]), v[:, 0]


def popcount(x):
    return np.bitwise_count(np.asarray(x, dtype=np.uint64)).astype(np.int64)


def compact(states, modes):
    out = np.zeros_like(states)
    for k, m in enumerate(modes):
        out |= ((states >> np.uint64(m)) & ONE) << np.uint64(k)
    return out


def sigma(states, a_modes, M):
    """(-1)^#{(i, j): i in A, j in B, both occupied, j < i}, pair by pair"""
    states = np.asarray(states, dtype=np.uint64)
    a_modes = sorted(a_modes)
    count = np.zeros(len(states), dtype=np.int64)
    for i in a_modes:
        for j in range(i):
            if j not in a_modes:
                count += (((states >> np.uint64(i)) & (states >> np.uint64(j))) & ONE).astype(np.int64)
    return np.where(count & 1, -1.0, 1.0)


def labels(case, a, a_modes):
    """the block label of every compacted word a: n_a, or (n_up, n_dn) on the spinful layout (rows of an (n, 2) array); None without a
    fixed number"""
    if case.spinful:
        au = sum(1 for m in a_modes if m < case.L)
        low = np.uint64((1 << au) - 1)
        return np.stack([popcount(a & low), popcount(a >> np.uint64(au))], axis=1)
    return None if case.N is None else popcount(a)


def bipartition(case, vec, a_modes, signed=True):
    """[(label, M)]: the blocks M[a, b] = sigma(n) <n|psi> of the full vector; rows / columns in ascending order of a / b; blocks in
    ascending (lexicographic) order of the label, empty blocks omitted; one block labelled -1 without a fixed number.
    signed=False leaves sigma out (what a spin expansion would give)."""
    a_modes = sorted(a_modes)
    b_modes = [m for m in range(case.M) if m not in a_modes]
    states = case.states
    a, b = compact(states, a_modes), compact(states, b_modes)
    v = np.asarray(vec) * (sigma(states, a_modes, case.M) if signed else 1.0)
    lab = labels(case, a, a_modes)
    if lab is None:
        m = np.zeros((1 << len(a_modes), 1 << len(b_modes)), dtype=v.dtype)
        m[a.astype(np.int64), b.astype(np.int64)] = v
        return [(-1, m)]
    keys = lab if lab.ndim == 2 else lab[:, None]
    out = []
    for key in sorted({tuple(int(x) for x in k) for k in keys}):
        sel = (keys == np.array(key)).all(axis=1)
        ua, ub = np.unique(a[sel]), np.unique(b[sel])
        assert len(ua) * len(ub) == int(sel.sum())  # the block is the full product of its row and column words
        m = np.zeros((len(ua), len(ub)), dtype=v.dtype)
        m[np.searchsorted(ua, a[sel]), np.searchsorted(ub, b[sel])] = v[sel]
        out.append((key if case.spinful else key[0], m))
    return out


def block_words(case, a_modes, label):
    """the ascending compacted words a of the block `label` (the rows of its M and of its rho_A block)"""
    na = len(a_modes)
    words = np.arange(1 << na, dtype=np.uint64)
    lab = labels(case, words, sorted(a_modes))
    if lab is None:
        return words
    return words[(lab == np.array(label)).all(axis=1)] if case.spinful else words[lab == label]


def spectrum(blocks):
    """(eigenvalues of rho_A in descending order, their labels): the squared singular values of the blocks"""
    vals, labs = [], []
    for lab, m in blocks:
        s = np.linalg.svd(m, compute_uv=False) ** 2
        vals.append(s)
        labs.extend([lab] * len(s))
    vals = np.concatenate(vals)
    order = np.argsort(-vals, kind="stable")
    return vals[order], [labs[i] for i in order]


def entropy(vals):
    p = vals[vals > 0]
    return float(-(p * np.log(p)).sum())


def peschel_entropy(hopping, N, a_sites):
    """free fermions: C = the projector on the N lowest orbitals of `hopping` (a closed shell is asserted), restricted to A;
    S = -sum [nu ln nu + (1 - nu) ln(1 - nu)] over its eigenvalues"""
    w, v = np.linalg.eigh(hopping)
    assert w[N] - w[N - 1] > 1e-6, "open shell"
    Cm = v[:, :N] @ v[:, :N].conj().T
    a = sorted(a_sites)
    nu = np.linalg.eigvalsh(Cm[np.ix_(a, a)])
    nu = nu[(nu > 1e-15) & (nu < 1 - 1e-15)]
    return float(-(nu * np.log(nu) + (1 - nu) * np.log(1 - nu)).sum())


def ring_hopping(L, t=1.0):
    h = np.zeros((L, L))
    for i in range(L):
        h[i, (i + 1) % L] -= t
        h[(i + 1) % L, i] -= t
    return h


def one_body(case, vec, i, j):
    """<psi|c+_i c_j|psi> over the unprojected states (modes i, j), by fermion_jw's action on occupation words"""
    def op(kind, m):
        return (kind, m - case.L, 1) if case.spinful and m >= case.L else (kind, m, 0)
    O = JW.sector_matrix([(1.0, [op("+", i), op("-", j)])], case.L, case.spinful, case.states)
    return complex(np.vdot(vec, O @ vec))


def torus_point_group(w, h):
    """the translations of fermion_symm.torus and the two axis reflections of a w x h torus"""
    gens = F.torus(w, h, point_group=False)
    gens.append([y * w + (w - 1 - x) for y in range(h) for x in range(w)])
    gens.append([(h - 1 - y) * w + x for y in range(h) for x in range(w)])
    return gens
