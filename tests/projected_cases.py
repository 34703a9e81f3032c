"""The fixed table of physical operators on projected spin bases that tests/test_gpu_projected_operators.py runs through every
pull / push / cached / block path, and tests/test_sector_reference.py validates the reference on.  All are rings; T is the
translation by one site, T2 by two, R the reflection i -> L-1-i, X the global spin flip.  Each row names the dispatch kind of
pull_kinds() (csrc/k_pull_t.hpp) it is there for: the K4 mode follows from the characters (all +1 and X >= 0: TRIVIAL; all +-1:
PM1; else GENERAL), the coefficient kind from the operator (complex coefficients: CPLX; real ones: REAL, or UNI when every group is
one exchange pair of one amplitude; GENERAL carries CPLX whatever the operator)."""
import functools

PAULI = {"x": "σˣ", "y": "σʸ", "z": "σᶻ", "+": "σ⁺", "-": "σ⁻"}
SUB = "₀₁₂₃₄₅₆₇₈₉"


def monomial(coefficient, kinds):
    body = " ".join(PAULI[k] + SUB[i] for i, k in enumerate(kinds))
    return body if coefficient == 1 else f"{coefficient!r} {body}"


def ring_tuples(L, k, step=1, start=0):
    return [[(i + q) % L for q in range(k)] for i in range(start, L, step)]


def heisenberg(sites, J=1):
    return [{"expression": monomial(J, a + a), "sites": sites} for a in "xyz"]


def tfim_terms(L):
    return [{"expression": monomial(1, "zz"), "sites": ring_tuples(L, 2)}, {"expression": monomial(0.7, "x"), "sites": ring_tuples(L, 1)}]


def dimer_terms(L):
    """Heisenberg, J = 1 on the even bonds and 0.6 on the odd ones: exchange pairs, but not one amplitude"""
    return heisenberg(ring_tuples(L, 2, 2, 0)) + heisenberg(ring_tuples(L, 2, 2, 1), 0.6)


def chiral_terms(L):
    """Heisenberg + 0.3 sum_i sigma_i . (sigma_{i+1} x sigma_{i+2}), the triple product as its six monomials: Hermitian, purely
    imaginary off-diagonal part, even under X, conserves the weight only as a sum"""
    eps = [("xyz", 0.3), ("yzx", 0.3), ("zxy", 0.3), ("xzy", -0.3), ("yxz", -0.3), ("zyx", -0.3)]
    return heisenberg(ring_tuples(L, 2)) + [{"expression": monomial(c, k), "sites": ring_tuples(L, 3)} for k, c in eps]


def jq_terms(L):
    """Heisenberg - 0.5 sum_i (sigma_i . sigma_{i+1}) (sigma_{i+2} . sigma_{i+3}): four-bit flip masks, many terms per group"""
    return heisenberg(ring_tuples(L, 2)) + [{"expression": monomial(-0.5, a + a + b + b), "sites": ring_tuples(L, 4)} for a in "xyz" for b in "xyz"]


def hop_terms(L):
    """directed hopping: real, NOT Hermitian -- only the push kernel can apply it on a projected basis"""
    return [{"expression": monomial(1, "+-"), "sites": ring_tuples(L, 2)}, {"expression": monomial(1, "zz"), "sites": ring_tuples(L, 2)}]


def xyz_terms(L):
    """XYZ ring, Jx = 1, Jy = 0.6, Jz = 0.8: real, Hermitian, even under X, NO weight conservation -- the two-bit flip of a bond carries
    Jx - Jy on an aligned pair and Jx + Jy on an anti-aligned one, i.e. a coefficient that depends on the partner's bits"""
    return [{"expression": monomial(J, a + a), "sites": ring_tuples(L, 2)} for a, J in (("x", 1.0), ("y", 0.6), ("z", 0.8))]


def twist_terms(L):
    """tfim + 0.4i sigma^y_i sigma^z_{i+1}: a complex COEFFICIENT but a real matrix (i sigma^y is real), not Hermitian, even under X;
    one-bit flip masks whose coefficient depends on the flipped bit and on its neighbour"""
    return tfim_terms(L) + [{"expression": "(0.0+0.4j) " + monomial(1, "yz"), "sites": ring_tuples(L, 2)}]


def phase_hop_terms(L):
    """directed hopping of one complex amplitude: not Hermitian, conserves the weight, not even under X"""
    return [{"expression": monomial(0.6 + 0.8j, "+-"), "sites": ring_tuples(L, 2)}, {"expression": monomial(1, "zz"), "sites": ring_tuples(L, 2)}]


def two_domain_terms(L):
    """Heisenberg ring, J = 1 on the bonds (i, i + 1) with i < L / 2 and 0.6 on the others (the closing bond too): two exchange runs
    of different amplitude"""
    bonds = ring_tuples(L, 2)
    return heisenberg(bonds[: L // 2]) + heisenberg(bonds[L // 2 :], 0.6)


FAMILIES = {"tfim": tfim_terms, "dimer_xxz": dimer_terms, "chiral": chiral_terms, "jq": jq_terms, "hop": hop_terms,
            "xyz": xyz_terms, "twist": twist_terms, "phase_hop": phase_hop_terms, "two_domain": two_domain_terms}


def make_config(family, L, weight=None, T=None, T2=None, R=None, X=None):
    basis = {"number_spins": L, "symmetries": []}
    if weight is not None:
        basis["hamming_weight"] = weight
    if X is not None:
        basis["spin_inversion"] = X
    if T is not None:
        basis["symmetries"].append({"permutation": [(i + 1) % L for i in range(L)], "sector": T})
    if T2 is not None:
        basis["symmetries"].append({"permutation": [(i + 2) % L for i in range(L)], "sector": T2})
    if R is not None:
        basis["symmetries"].append({"permutation": [L - 1 - i for i in range(L)], "sector": R})
    return {"basis": basis, "hamiltonian": {"name": family, "terms": FAMILIES[family](L)}}


# name -> (family, basis arguments, isReal, isHermitian, K4 mode, bytes per cached packet (5 UNI / 13 REAL / 21 CPLX; None: no pull
# plan), number of representatives where the table states it)
CASES = {
    "tfim_14_k0_r0_x1": ("tfim", dict(L=14, T=0, R=0, X=1), True, True, "TRIVIAL", 13, 362),
    "tfim_14_k7": ("tfim", dict(L=14, T=7), True, True, "PM1", 13, None),
    "tfim_14_k0_x-1": ("tfim", dict(L=14, T=0, X=-1), True, True, "PM1", 13, None),
    "tfim_14_k3": ("tfim", dict(L=14, T=3), True, True, "GENERAL", 21, 1161),
    "dimer_xxz_16": ("dimer_xxz", dict(L=16, weight=8, T2=0), True, True, "TRIVIAL", 13, 1620),
    "chiral_16_k0": ("chiral", dict(L=16, weight=8, T=0), False, True, "TRIVIAL", 21, 810),
    "chiral_16_k8": ("chiral", dict(L=16, weight=8, T=8), False, True, "PM1", 21, 810),
    "chiral_16_k0_x-1": ("chiral", dict(L=16, weight=8, T=0, X=-1), False, True, "PM1", 21, None),
    "chiral_16_k3": ("chiral", dict(L=16, weight=8, T=3), False, True, "GENERAL", 21, 800),
    "chiral_16_k3_x-1": ("chiral", dict(L=16, weight=8, T=3, X=-1), False, True, "GENERAL", 21, 408),
    "jq_16_k0_r1": ("jq", dict(L=16, weight=8, T=0, R=1), True, True, "PM1", 13, None),
    "chiral_36_4_k5": ("chiral", dict(L=36, weight=4, T=5), False, True, "GENERAL", 21, None),
    "tfim_zz_36_4_k0": ("dimer_xxz", dict(L=36, weight=4, T2=0), True, True, "TRIVIAL", 13, None),
    "hop_16_k0": ("hop", dict(L=16, weight=8, T=0), True, False, "TRIVIAL", None, None),
    "hop_16_k3": ("hop", dict(L=16, weight=8, T=3), True, False, "GENERAL", None, None),
}
HERMITIAN = [name for name, row in CASES.items() if row[3]]
NON_HERMITIAN = [name for name, row in CASES.items() if not row[3]]


def config_of(name):
    family, args = CASES[name][:2]
    return make_config(family, **args)


def k4_mode_of(model):
    """the K4 mode the characters of a basis ask for (host.c basis_device: `trivial`, chars_pm1)"""
    chars = [complex(c) for c in model.group.chars]
    if all(c == 1 for c in chars) and model.spin_inversion >= 0:
        return "TRIVIAL"
    return "PM1" if all(c.imag == 0 and abs(c.real) == 1 for c in chars) else "GENERAL"


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """(representatives, H_sector, leak) of a case, computed once per process"""
    from sector_reference import sector_matrix

    return sector_matrix(config_of(name))


# reduced copies of every family for the entry-by-entry comparison with oracle.model.dense_sector_matrix: one sector of each character
# type (trivial, -1, complex, and with the flip in the group where the operator is even under it)
def reduced_cases():
    out = {}
    for L in (8, 10):
        w = L // 2
        out[f"tfim_{L}_k0_r0_x1"] = make_config("tfim", L, T=0, R=0, X=1)
        out[f"tfim_{L}_k{L // 2}"] = make_config("tfim", L, T=L // 2)
        out[f"tfim_{L}_k0_x-1"] = make_config("tfim", L, T=0, X=-1)
        out[f"tfim_{L}_k3"] = make_config("tfim", L, T=3)
        out[f"dimer_xxz_{L}"] = make_config("dimer_xxz", L, weight=w, T2=0)
        out[f"dimer_xxz_{L}_k1"] = make_config("dimer_xxz", L, weight=w, T2=1)
        out[f"chiral_{L}_k0"] = make_config("chiral", L, weight=w, T=0)
        out[f"chiral_{L}_k{L // 2}"] = make_config("chiral", L, weight=w, T=L // 2)
        out[f"chiral_{L}_k0_x-1"] = make_config("chiral", L, weight=w, T=0, X=-1)
        out[f"chiral_{L}_k3"] = make_config("chiral", L, weight=w, T=3)
        out[f"chiral_{L}_k3_x-1"] = make_config("chiral", L, weight=w, T=3, X=-1)
        out[f"jq_{L}_k0_r1"] = make_config("jq", L, weight=w, T=0, R=1)
        out[f"jq_{L}_k3"] = make_config("jq", L, weight=w, T=3)
        out[f"hop_{L}_k0"] = make_config("hop", L, weight=w, T=0)
        out[f"hop_{L}_k3"] = make_config("hop", L, weight=w, T=3)
        out[f"chiral_{L}_2_k1"] = make_config("chiral", L, weight=2, T=1)  # (a dilute sector, as the 36-site cases are)
    return out
