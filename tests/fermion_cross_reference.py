"""Reference matrices of an operator BETWEEN two sectors of projected fermionic bases, from tests/fermion_symm.py,
tests/fermion_spinful_symm.py and tests/fermion_jw.py alone (nothing of the library under test): B2^+ A B1 with the columns of B
from `projector_columns` (every U_g entry carries its permutation sign) and A the rectangular block <target words|A|source words>
of the Jordan-Wigner matrix -- `fermion_jw.dense` up to 12 modes, `fermion_jw.sector_matrix` on the union of the words above.
The pull form the kernel runs is counted on the same block: a (target representative, flip mask) pair with a coefficient above the
rounding residue is an image when its column state has non-zero norm in the SOURCE sector, and is dropped when that norm vanishes.
The module also holds the cases shared by tests/test_fermion_cross_host.py and tests/test_gpu_fermion_cross.py."""
import cmath
import functools
import math

import numpy as np
import scipy.sparse as sp

import fermion_jw as J
import fermion_spinful_symm as FS
import fermion_symm as F

RESIDUE = 1e-13  # a summed coefficient below RESIDUE * sum |v| is the rounding residue of terms that cancel, not an image


def phase(L, dk, j):
    """exp(-2 pi i dk j / L), exactly real where it is (so that a +-1 operator can run in f64)"""
    z = cmath.exp(-2j * math.pi * dk * j / L)
    if (2 * dk * j) % L == 0:
        z = complex(round(z.real), 0.0)
    return z


def momentum_op(L, dk, make):
    """sum_j exp(-2 pi i dk j / L) o_j: takes momentum k to k + dk under T = [(i + 1) % L]; make(j) = [(factor, ops)] of o_j"""
    return [(phase(L, dk, j) * f, ops) for j in range(L) for f, ops in make(j)]


def c_dag(L, dk, spin=0):
    return momentum_op(L, dk, lambda j: [(1.0, [("+", j, spin)])])


def c_ann(L, dk, spin=0):
    return momentum_op(L, dk, lambda j: [(1.0, [("-", j, spin)])])


def n_q(L, dk, spinful=False):
    return momentum_op(L, dk, lambda j: [(1.0, [("n", j, s)]) for s in ((0, 1) if spinful else (0,))])


def sz_q(L, dk):
    return momentum_op(L, dk, lambda j: [(0.5, [("n", j, 0)]), (-0.5, [("n", j, 1)])])


def sector(L, N, gens, secs, n_up=None, flip=0):
    """a sector as a plain dict; spinless when n_up is None, else (N_up, N_down) = (n_up, N - n_up)"""
    return {"L": L, "N": N, "gens": [list(g) for g in gens], "secs": [int(s) for s in secs], "n_up": n_up, "flip": flip}


def basis_config(sec):
    sym = [{"permutation": list(p), "sector": int(s)} for p, s in zip(sec["gens"], sec["secs"])]
    if sec["n_up"] is None:
        return {"basis": {"particle": "spinless-fermion", "number_sites": sec["L"], "number_particles": sec["N"], "symmetries": sym}}
    b = {"particle": "spinful-fermion", "number_sites": sec["L"], "number_particles": sec["N"], "number_up": sec["n_up"], "symmetries": sym}
    if sec["flip"]:
        b["spin_flip"] = sec["flip"]
    return {"basis": b}


def operator_section(model, spinful):
    return {"terms": J.yaml_terms(model, spinful)}


def coefficient_sum(model):
    return float(sum(abs(complex(c)) for c, _ in model))


def _sector_tables(sec):
    """(group, words of the particle-number sector, representatives, B as CSR, norm of every word)"""
    L = sec["L"]
    if sec["n_up"] is None:
        grp = F.closure(L, sec["gens"], sec["secs"])
        # (state_info_v is fermion_symm.state_info over an array of words, for ANY group of mode permutations: it gives the norm
        # of every word; the representatives come from the scalar loop of fermion_symm up to 16 modes -- above, it takes seconds)
        rep, _, norms = FS.state_info_v(grp, J.weight_states(L, sec["N"]))
        if L <= 16:
            reps, _ = F.representatives(L, sec["N"], grp)
        else:
            reps = J.weight_states(L, sec["N"])[(rep == J.weight_states(L, sec["N"])) & (norms > 0)]
        words, B = F.projector_columns(L, sec["N"], grp, reps)
        return grp, words, reps, sp.csr_matrix(B), norms
    nu, nd = sec["n_up"], sec["N"] - sec["n_up"]
    grp = FS.group(L, sec["gens"], sec["secs"], sec["flip"])
    reps, _ = FS.representatives(L, nu, nd, grp)
    words, B = FS.projector_columns(L, nu, nd, grp, reps)
    return grp, words, reps, sp.csr_matrix(B), FS.state_info_v(grp, words)[2]


def rectangular_block(model, L, spinful, rows, cols):
    """<rows|A|cols> as CSR: the block of the dense Jordan-Wigner matrix up to 12 modes, of sector_matrix on the union above"""
    modes = 2 * L if spinful else L
    if modes <= 12:
        full = J.dense(model, L, spinful).tocsr()
        return full[rows.astype(np.int64)][:, cols.astype(np.int64)].tocsr()
    words = np.unique(np.concatenate([rows, cols]))
    full = J.sector_matrix(model, L, spinful, words).tocsr()
    return full[np.searchsorted(words, rows)][:, np.searchsorted(words, cols)].tocsr()


def reference(src, dst, model):
    """{"src", "dst" (ascending representatives), "matrix" = B2^+ A B1 [n_dst, n_src], "leak" = ||A B1 - B2 B2^+ A B1|| (what leaves
    the target sector), "norm" = ||A B1||, "images", "pull_dropped" (the pull form: see the module docstring)}"""
    spinful = src["n_up"] is not None
    _, w1, r1, B1, norm1 = _sector_tables(src)
    _, w2, r2, B2, _ = _sector_tables(dst)
    A = rectangular_block(model, src["L"], spinful, w2, w1)
    AB = A @ B1
    mat = (B2.conj().T @ AB).toarray()
    leak = float(abs(AB - B2 @ sp.csr_matrix(mat)).power(2).sum() ** 0.5)
    tiny = RESIDUE * coefficient_sum(model)
    rows = A[np.searchsorted(w2, r2)].tocoo()  # <r'|A|a>: one entry per (target representative, flip mask r' ^ a)
    live = np.abs(rows.data) > tiny
    has_norm = norm1[rows.col] > 0
    return {"src": r1, "dst": r2, "matrix": mat, "leak": leak, "norm": float(abs(AB).power(2).sum() ** 0.5),
            "images": int(np.count_nonzero(live & has_norm)), "pull_dropped": int(np.count_nonzero(live & ~has_norm))}


def _T(L):
    return F.translations(L)


# name -> (source sector, target sector, model, dk of the operator, dtypes, (source rows, target rows, zero-norm pull images or None))
CASES = {
    "L8_cdag_q3": (sector(8, 3, _T(8), [0]), sector(8, 4, _T(8), [3]), c_dag(8, 3), 3, ("c128",), (7, 8, 0)),
    "L8_cdag_q2": (sector(8, 4, _T(8), [1]), sector(8, 5, _T(8), [3]), c_dag(8, 2), 2, ("c128",), (8, 7, 3)),
    "L8_cdag_q4": (sector(8, 2, _T(8), [4]), sector(8, 3, _T(8), [0]), c_dag(8, 4), 4, ("c128",), (3, 7, 3)),
    "L8_n_q3": (sector(8, 4, _T(8), [1]), sector(8, 4, _T(8), [4]), n_q(8, 3), 3, ("c128",), (8, 9, None)),
    "L8_dihedral_cdag_q0": (sector(8, 3, F.dihedral(8), [0, 0]), sector(8, 4, F.dihedral(8), [0, 0]), c_dag(8, 0), 0, ("f64", "c128"), (2, 6, 8)),
    "L12_cdag_q5": (sector(12, 6, _T(12), [0]), sector(12, 7, _T(12), [5]), c_dag(12, 5), 5, ("c128",), (76, 66, 10)),
    "L34_cdag_q5": (sector(34, 2, _T(34), [0]), sector(34, 3, _T(34), [5]), c_dag(34, 5), 5, ("c128",), (16, 176, 16)),
    "spinful_L4_cdag_q1_up": (sector(4, 4, _T(4), [0], n_up=2), sector(4, 5, _T(4), [1], n_up=3), c_dag(4, 1, 0), 1, ("c128",), (10, 6, 0)),
    "spinful_L4_c_q3_dn": (sector(4, 4, _T(4), [2], n_up=2), sector(4, 3, _T(4), [1], n_up=2), c_ann(4, 3, 1), 3, ("c128",), (10, 6, 0)),
    "spinful_L6_cdag_q2_up": (sector(6, 6, _T(6), [1], n_up=3), sector(6, 7, _T(6), [3], n_up=4), c_dag(6, 2, 0), 2, ("c128",), (66, 50, "> 0")),
    "spinful_L6_sz_q2": (sector(6, 6, _T(6), [0], n_up=3, flip=1), sector(6, 6, _T(6), [2], n_up=3, flip=-1), sz_q(6, 2), 2, ("c128",), (30, 36, None)),
    "spinful_L6_dihedral_n_q3": (sector(6, 6, F.dihedral(6), [0, 0], n_up=3, flip=1), sector(6, 6, F.dihedral(6), [3, 1], n_up=3, flip=1),
                                 n_q(6, 3, True), 3, ("f64", "c128"), (12, 19, None)),
}


def is_spinful(name):
    return CASES[name][0]["n_up"] is not None


def wrong_dk_model(name):
    """the operator of the case with dk + 1 in place of dk: maps the source sector into the NEXT momentum sector, not the target"""
    src, _, model, dk, _, _ = CASES[name]
    L = src["L"]
    return [(phase(L, dk + 1, ops[0][1]) * (complex(c) / phase(L, dk, ops[0][1])), ops) for c, ops in model]


@functools.lru_cache(maxsize=None)
def case_reference(name):
    src, dst, model, _, _, _ = CASES[name]
    return reference(src, dst, model)
