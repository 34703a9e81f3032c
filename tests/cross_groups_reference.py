"""References and the tolerance of the cross-sector tests between bases with DIFFERENT symmetry groups (tests/test_cross_groups_host.py,
tests/test_gpu_cross_groups.py).  Nothing here is the code under test:

  * up to 12 sites or modes the matrix is the dense B2^+ A B1 of tests/cross_sector_reference.py (spins) and
    tests/fermion_cross_reference.py (fermions), which build each side's isometry from its own group;
  * the covariance rule of groups="restrict" is checked against dense conjugation, U_g A U_g^+ - chi2(g) conj(chi1(g)) A on the full
    2^L space, with chi1 looked up in the closure oracle.model builds of the SOURCE's generators.

The tolerance is derived, not measured.  A row of y is a sum of at most S summands coefficient * x[column] -- S = (elements of the
target group, the inversion doubling included) x (monomials of the operator) for a projecting plan, the monomials alone for a
restricted one -- added in LDS in no fixed order, so
    |got - want| <= max((S + 2) 2^-53 scale, 1e-12 max(|got|, |want|)),      scale = (the row's sum of |coefficient|) max|x|:
S - 1 roundings of the additions in any order and the roundings of a summand itself, each relative to the sum of the absolute
summands; the second term is the reference's own error (a dense product over up to 4096 states).  The row's sum of |coefficient| is
bounded by (sum of |c_j| over the monomials) / n2(r'): the element weights |chi2(g)| / (|G2| n2(r')) of a projecting plan add up to
1 / n2(r'), a restricted plan has the one weight 1 / n2(r'), and the source norms n1 are at most 1."""
import functools
import json

import numpy as np

import cross_sector_reference as X
from oracle import model as M

U = 2.0 ** -53


def ring(L, hw=None, k=None, reflection=None, inversion=None):
    """cross_sector_reference.ring, and hw=None for every Hamming weight"""
    cfg = X.ring(L, hw if hw is not None else 0, k, reflection, inversion)
    if hw is None:
        del cfg["basis"]["hamming_weight"]
    return cfg


def with_generators(L, hw, gens, inversion=None):
    """a spin basis with arbitrary generators: gens = [(permutation, sector)]"""
    b = {"number_spins": L, "symmetries": [{"permutation": list(p), "sector": int(s)} for p, s in gens]}
    if hw is not None:
        b["hamming_weight"] = hw
    if inversion is not None:
        b["spin_inversion"] = int(inversion)
    return {"basis": b}


def translation(L, step=1):
    return [(i + step) % L for i in range(L)]


def reflection(L):
    return [L - 1 - i for i in range(L)]


def compose(p, q):
    """the permutation of applying q, then p, to a state: (p.(q.a))[i] = (q.a)[p[i]] = a[q[p[i]]]"""
    return [q[p[i]] for i in range(len(p))]


# ---- operators ---------------------------------------------------------------------------------------------------------------------
def sz_site(j=0):
    return {"terms": [{"expression": "σᶻ₀", "sites": [[j]]}]}


def identity(L):
    """1 = sum_j (sigma^+_j sigma^-_j + sigma^-_j sigma^+_j) / L: one diagonal group whose coefficient is 1 on every state"""
    c = repr(1.0 / L)
    return {"terms": [{"expression": c + " σ⁺₀ σ⁻₀", "sites": [[j] for j in range(L)]}, {"expression": c + " σ⁻₀ σ⁺₀", "sites": [[j] for j in range(L)]}]}


def hop_q_plus_sz0(L, q):
    """sum_j e^{-2 pi i q j / L} sigma^+_j sigma^-_{j+1} + sigma^z_0: L flip masks and a diagonal group, complex coefficients,
    covariant under nothing"""
    terms = [{"expression": X._c(np.exp(-2j * np.pi * q * j / L)) + " σ⁺₀ σ⁻₁", "sites": [[j, (j + 1) % L]]} for j in range(L)]
    return {"terms": terms + sz_site(0)["terms"]}


def monomials(op_cfg):
    return sum(len(t["sites"]) for t in op_cfg["terms"])


# ---- dense spin references ---------------------------------------------------------------------------------------------------------
def _key(cfg):
    return json.dumps(cfg, sort_keys=True, ensure_ascii=False)


@functools.lru_cache(maxsize=None)
def _isometry(key):
    return X.isometry(json.loads(key))


@functools.lru_cache(maxsize=4)
def _image(src_key, op_key):
    """A B1 on the full space"""
    src = json.loads(src_key)
    return np.asarray(X.full_matrix(src, json.loads(op_key)) @ _isometry(src_key)[1])


def group_order(cfg):
    """|G| with the inversion doubling"""
    model = X._model(cfg)
    return len(model.group.perms) * (2 if model.spin_inversion != 0 else 1)


@functools.lru_cache(maxsize=None)
def _dense(src_key, dst_key, op_key):
    r1, _ = _isometry(src_key)
    r2, B2 = _isometry(dst_key)
    AB = _image(src_key, op_key)
    mat = B2.conj().T @ AB
    # B2[r', column of r'] = n2(r')^2 / n2(r'): the norm of every target row
    n2 = np.abs(B2[r2.astype(np.int64), np.arange(len(r2))])
    return {"src": r1, "dst": r2, "matrix": np.asarray(mat), "leak": float(np.linalg.norm(AB - B2 @ mat)), "norm": float(np.linalg.norm(AB)),
            "n2": n2, "image": AB}


def dense(src_cfg, dst_cfg, op_cfg):
    """{"src", "dst": ascending representatives; "matrix": B2^+ A B1 (the arithmetic of cross_sector_reference.projector_matrix, its
    isometries and its full matrix, cached); "leak": ||A B1 - B2 B2^+ A B1||_F; "norm": ||A B1||_F; "n2": the norm of every target row;
    "image": A B1}"""
    return _dense(_key(src_cfg), _key(dst_cfg), _key(op_cfg))


# ---- the tolerance -----------------------------------------------------------------------------------------------------------------
def compare(got, want, summands, scale, what):
    """the module docstring's bound; summands = S, scale = per row (array) or one number.  Prints the worst ratio error / tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    tol = np.maximum((summands + 2) * U * np.broadcast_to(scale, want.shape), 1e-12 * np.maximum(np.abs(got), np.abs(want)))
    err = np.abs(got - want)
    finite = np.isfinite(got).all()
    ratio = float((err / np.maximum(tol, 1e-300)).max()) if finite and len(want) else 0.0
    print(f"cross-groups {what}: rows {len(want)}, S {summands}, max |y| {np.abs(want).max() if len(want) else 0.0:.3e}, "
          f"max error {err.max() if len(want) else 0.0:.3e}, worst error / tolerance {ratio:.3g}")
    assert finite and (err <= tol).all(), (what, float(err.max()), ratio)
    return ratio


def row_scale(coefficient_sum, n2, xmax):
    return coefficient_sum * float(xmax) / np.asarray(n2)


# ---- the covariance rule of groups="restrict" by dense conjugation -------------------------------------------------------------
def _perm_matrix(p, L):
    """U_g on the full space: U_g|a> = |g.a>, g.a = oracle.model.apply_perm(p, a)"""
    dim = 1 << L
    Umat = np.zeros((dim, dim))
    for a in range(dim):
        Umat[M.apply_perm(p, a), a] = 1.0
    return Umat


def subgroup_defects(src_cfg, dst_cfg, op_cfg):
    """None when the target group is no subgroup of the source group (a generator of the target is no element of the source's closure,
    or the target has the spin inversion and the source has not); else [(name, defect)] -- name = "generator g" or "spin inversion",
    defect = max |U A U^+ - chi2 conj(chi1) A| over the entries, for every generator of the TARGET and its inversion"""
    m1, m2 = X._model(src_cfg), X._model(dst_cfg)
    L = m1.number_sites
    assert L <= 8 and m2.number_sites == L
    if m2.spin_inversion != 0 and m1.spin_inversion == 0:
        return None
    A = X.full_matrix(src_cfg, op_cfg)
    A = np.asarray(A.todense() if hasattr(A, "todense") else A)
    closure = {tuple(int(v) for v in p): complex(ch) for p, ch in zip(m1.group.perms, m1.group.chars)}
    out = []
    for g, sym in enumerate(dst_cfg["basis"]["symmetries"]):
        p = tuple(int(v) for v in sym["permutation"])
        if p not in closure:
            return None
        order, q = 1, p
        while list(q) != list(range(L)):
            q, order = tuple(compose(list(p), list(q))), order + 1
        chi2 = np.exp(-2j * np.pi * int(sym["sector"]) / order)
        Umat = _perm_matrix(list(p), L)
        out.append((f"generator {g}", float(np.abs(Umat @ A @ Umat.T - chi2 * np.conj(closure[p]) * A).max())))
    if m2.spin_inversion != 0:
        F = np.zeros((1 << L, 1 << L))
        for a in range(1 << L):
            F[a ^ m1.mask, a] = 1.0
        out.append(("spin inversion", float(np.abs(F @ A @ F.T - m1.spin_inversion * m2.spin_inversion * A).max())))
    return out
