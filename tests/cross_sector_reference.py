"""Reference matrices of an operator BETWEEN two symmetry sectors, from plain numpy and oracle.model alone (nothing of the library
under test): projector_matrix is B2^+ A B1 on the full 2^L space, formula_matrix the push form of the matrix elements with
oracle.model.state_info,
    <r'|_2 A |r>_1 = sum_{j : rep(b_j) = r'} c_j conj(chi2(g0j)) n2(r') / n1(r),     A|r> = sum_j c_j |b_j>,  g0j b_j = r'.
A basis is given as a config {"basis": ...}, the operator as a `hamiltonian:`-style section {"terms": [{expression, sites}]}.
The module also holds the cases shared by tests/test_cross_sector_host.py and tests/test_gpu_cross_sector.py."""
import cmath
import functools
import math

import numpy as np

from oracle import model as M

RESIDUE = 1e-13  # a summed coefficient below RESIDUE * sum |v| is the rounding residue of terms that cancel, not an image


def _model(basis_cfg, op_cfg=None):
    cfg = {"basis": basis_cfg["basis"]}
    if op_cfg is not None:
        cfg["hamiltonian"] = op_cfg
    return M.model_from_config(cfg)


def isometry(basis_cfg):
    """(reps, B): the columns of B [2^L, n] are P|r> / ||P|r>|| for the ascending representatives r of non-zero norm,
    P = |G|^-1 sum_g conj(chi(g)) U_g (the convention of oracle.model.dense_sector_matrix), on the FULL 2^L space"""
    model = _model(basis_cfg)
    L, hw = model.number_sites, model.hamming_weight
    assert L <= 12
    dim = 1 << L
    elems = []
    for p, ch in zip(model.group.perms, model.group.chars):
        elems.append((p, False, ch))
        if model.spin_inversion != 0:
            elems.append((p, True, ch * model.spin_inversion))
    reps, cols, seen = [], [], set()
    for s in range(dim):
        if (hw >= 0 and bin(s).count("1") != hw) or s in seen:
            continue
        orbit = set()
        for p, flip, _ in elems:
            t = M.apply_perm(p, s)
            orbit.add(t ^ model.mask if flip else t)
        seen |= orbit
        r = min(orbit)
        vec = np.zeros(dim, dtype=complex)
        for p, flip, ch in elems:
            t = M.apply_perm(p, r)
            vec[t ^ model.mask if flip else t] += np.conj(ch) / len(elems)
        nrm = np.linalg.norm(vec)
        if nrm > 1e-9:
            reps.append(r)
            cols.append(vec / nrm)
    order = np.argsort(reps)
    return np.array(reps, dtype=np.uint64)[order], np.array(cols)[order].T


def full_matrix(basis_cfg, op_cfg):
    """A on the full 2^L space, straight from the expressions (oracle.model.dense_hamiltonian_full)"""
    return M.dense_hamiltonian_full({"basis": basis_cfg["basis"], "hamiltonian": op_cfg})


def projector_matrix(src_cfg, dst_cfg, op_cfg):
    """(source reps, target reps, B2^+ A B1 [n_dst, n_src]) and the part of A B1 that leaves the target sector (Frobenius norm)"""
    r1, B1 = isometry(src_cfg)
    r2, B2 = isometry(dst_cfg)
    AB = full_matrix(src_cfg, op_cfg) @ B1
    mat = B2.conj().T @ AB
    leak = float(np.linalg.norm(AB - B2 @ mat))
    return r1, r2, np.asarray(mat), leak


def _groups(terms):
    """the terms of an oracle.model.Terms by flip mask: {x: [(v, m, r, s)]}"""
    out = {}
    for v, m, r, x, s in zip(terms.v, terms.m, terms.r, terms.x, terms.s):
        out.setdefault(int(x), []).append((complex(v), int(m), int(r), int(s)))
    return out


def _coefficient(group, alpha):
    c = 0j
    for v, m, r, s in group:
        if (alpha & m) == r:
            c += -v if bin(alpha & s).count("1") & 1 else v
    return c


def _active(group, alpha):
    return any((alpha & m) == r for _, m, r, _ in group)


def formula_matrix(src_cfg, dst_cfg, op_cfg):
    """the push formula, with counts: {"src", "dst" (reps), "matrix" [n_dst, n_src], "dropped" (images -- a source representative
    and a flip mask with an active term -- whose orbit has zero norm in the target sector: covariance makes their contribution
    vanish, whatever the coefficient), "images" (the (target row, flip mask) pairs that contribute in the PULL form: a coefficient
    <r'|A|r' ^ x> above the rounding residue whose column state r' ^ x has non-zero norm in the source sector), "pull_dropped"
    (such coefficients whose column state has ZERO norm in the source sector: what the pull kernel must discard), "row_sums"
    (sum_j |c_j| n1 / n2 per target row in the pull form)}"""
    m1, m2 = _model(src_cfg, op_cfg), _model(dst_cfg)
    r1 = [int(s) for s in M.enumerate_representatives(m1)]
    r2 = [int(s) for s in M.enumerate_representatives(m2)]
    idx2 = {s: i for i, s in enumerate(r2)}
    groups = {}
    for part in (m1.diag, m1.offdiag):
        for x, g in _groups(part).items():
            groups.setdefault(x, []).extend(g)
    tiny = RESIDUE * sum(abs(v) for g in groups.values() for v, _, _, _ in g)
    mat = np.zeros((len(r2), len(r1)), dtype=complex)
    dropped = 0
    for i, r in enumerate(r1):
        n1 = M.state_info(m1, r)[2] if m1.requires_projection else 1.0
        for x, g in groups.items():
            if not _active(g, r):
                continue
            rep, ch, nb = M.state_info(m2, r ^ x) if m2.requires_projection else (r ^ x, 1.0, 1.0)
            if nb == 0.0:
                dropped += 1
                continue
            c = _coefficient(g, r)
            if abs(c) <= tiny:
                continue
            mat[idx2[rep], i] += c * ch * nb / n1  # KeyError: the operator leaves the target basis
    images = pull_dropped = 0
    row_sums = np.zeros(len(r2))
    for j, rp in enumerate(r2):
        n2 = M.state_info(m2, rp)[2] if m2.requires_projection else 1.0
        for x, g in groups.items():
            c = _coefficient(g, rp ^ x)  # <r'|A|r' ^ x>
            if abs(c) <= tiny:
                continue
            n1 = M.state_info(m1, rp ^ x)[2] if m1.requires_projection else 1.0
            if n1 == 0.0:
                pull_dropped += 1
                continue
            images += 1
            row_sums[j] += abs(c) * n1 / n2
    return {"src": np.array(r1, dtype=np.uint64), "dst": np.array(r2, dtype=np.uint64), "matrix": mat, "dropped": dropped,
            "images": images, "pull_dropped": pull_dropped, "row_sums": row_sums}


# ---- the shared cases ------------------------------------------------------------------------------------------------------------
def ring(L, hw, k=None, reflection=None, inversion=None):
    """basis config of a ring: translation T = [(i + 1) % L] in sector k, reflection [L - 1 - i] in its sector, spin inversion"""
    b = {"number_spins": L, "hamming_weight": hw, "symmetries": []}
    if k is not None:
        b["symmetries"].append({"permutation": [(i + 1) % L for i in range(L)], "sector": int(k)})
    if reflection is not None:
        b["symmetries"].append({"permutation": [L - 1 - i for i in range(L)], "sector": int(reflection)})
    if inversion is not None:
        b["spin_inversion"] = int(inversion)
    return {"basis": b}


def _c(z):
    z = complex(z)
    return repr(z.real) if z.imag == 0 else "(" + repr(z.real) + ("+" if z.imag >= 0 else "-") + repr(abs(z.imag)) + "j)"


def sz_q(L, dk):
    """sum_j exp(-2 pi i dk j / L) sigma^z_j: covariant for k -> k + dk with T = [(i + 1) % L] and the character exp(-2 pi i k / n)"""
    return {"terms": [{"expression": _c(cmath.exp(-2j * math.pi * dk * j / L)) + " σᶻ₀", "sites": [[j]]} for j in range(L)]}


def sz_q_projectors(L, dk):
    """the same operator written with projector terms: sigma^z = sigma^+ sigma^- - sigma^- sigma^+"""
    terms = []
    for j in range(L):
        ph = cmath.exp(-2j * math.pi * dk * j / L)
        terms.append({"expression": _c(ph) + " σ⁺₀ σ⁻₀", "sites": [[j]]})
        terms.append({"expression": _c(-ph) + " σ⁻₀ σ⁺₀", "sites": [[j]]})
    return {"terms": terms}


def splus_q(L, dk):
    return {"terms": [{"expression": _c(cmath.exp(-2j * math.pi * dk * j / L)) + " σ⁺₀", "sites": [[j]]} for j in range(L)]}


def staggered_z(L):
    return {"terms": [{"expression": _c((-1.0) ** j) + " σᶻ₀", "sites": [[j]]} for j in range(L)]}


def coefficient_sum(op_cfg):
    """sum_j |c_j| over the monomials of the operator"""
    return sum(abs(M.parse_expression(t["expression"])[0]) * len(t["sites"]) for t in op_cfg["terms"])


# name -> (source config, target config, operator section, dtype); the representative counts in the comments are checked by the tests
CASES = {
    "L8_sz_k0_k3": (ring(8, 4, 0), ring(8, 4, 3), sz_q(8, 3), "c128"),            # 10 -> 8 rows, 2 images dropped for zero norm
    "L8_sz_k2_k7": (ring(8, 4, 2), ring(8, 4, 7), sz_q(8, 5), "c128"),
    "L8_sz_k0_k4": (ring(8, 4, 0), ring(8, 4, 4), sz_q(8, 4), "c128"),
    "L8_splus_w4_w3_k0_k3": (ring(8, 4, 0), ring(8, 3, 3), splus_q(8, 3), "c128"),
    "L8_dihedral_staggered": (ring(8, 4, 0, 0, 1), ring(8, 4, 4, 1, -1), staggered_z(8), "f64"),  # 7 -> 4 rows, 3 dropped
    # a source sector in which periodic states have zero norm: the PULL form meets images with a coefficient and no source state
    "L8_splus_w4_w3_k1_k4": (ring(8, 4, 1), ring(8, 3, 4), splus_q(8, 3), "c128"),
}


@functools.lru_cache(maxsize=None)
def case_formula(name):
    src, dst, op, _ = ALL_CASES[name]
    return formula_matrix(src, dst, op)


def _plain(L, hw):
    b = {"number_spins": L, "symmetries": []}
    if hw is not None:
        b["hamming_weight"] = hw
    return {"basis": b}


GPU_ONLY_CASES = {
    "L12_w6_w5_f64": (_plain(12, 6), _plain(12, 5), {"terms": [{"expression": "σ⁺₀", "sites": [[0]]}, {"expression": "0.5 σ⁺₀", "sites": [[3]]}]}, "f64"),
    "L12_w6_w5_c128": (_plain(12, 6), _plain(12, 5), {"terms": [{"expression": "σ⁺₀", "sites": [[0]]}, {"expression": "0.5 σ⁺₀", "sites": [[3]]}]}, "c128"),
    "L12_identity_index": (_plain(12, None), _plain(12, None), {"terms": [{"expression": "σˣ₀ σᶻ₁", "sites": [[0, 1]]}]}, "f64"),
    "L16_sz_k0_k5": (ring(16, 8, 0), ring(16, 8, 5), sz_q(16, 5), "c128"),
    "L16_splus_w8_w7_k0_k5": (ring(16, 8, 0), ring(16, 7, 5), splus_q(16, 5), "c128"),
}
ALL_CASES = {**CASES, **GPU_ONLY_CASES}
