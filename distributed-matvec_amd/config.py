"""Host mirror of ``ls_hs_load_yaml_config`` (/root/reference/src/ForeignTypes.chpl:261-288,
/root/reference/src/FFI.chpl:205): YAML -> basis description + non-branching terms.

The reference delegates this to lattice-symmetries-haskell; here the (new-schema) YAML subset of
/root/reference/data/*.yaml is compiled symbolically: every expression is a
monomial of single-site operators, each of which maps a basis state to at most one basis state, so a
monomial applied to a site tuple yields a handful of terms
    coefficient v, projector (m, r), flip mask x, sign mask s
(include/ls_hs.h).  Merging / cancellation / grouping by flip mask happens in C
(ls_hs_create_operator_from_terms).  No numerics on the hot path happen here.

Conventions: site i <-> bit i; bit 0 = spin up (sigma^z = +1); S^a = sigma^a / 2.

Fermions (``particle: spinless-fermion | spinful-fermion``): one bit per mode -- mode i = bit i for spinless fermions, mode
(i, up) = bit i and mode (i, down) = bit i + L for spinful ones -- and the Jordan-Wigner order is the bit order:
    c+_k |n> = (-1)^{sum_{k' < k} n_k'} |n + e_k>
(include/ls_hs.h).  Operators ``c†ᵢσ``, ``cᵢσ``, ``nᵢσ`` with σ in {↑, ↓} (no σ for spinless fermions); a monomial compiles to
one term per occupation pattern of the modes it touches, its sign mask the XOR of the "modes below k" masks of its c / c†
factors without those modes (their occupations are fixed by the pattern and folded into v).
"""
from __future__ import annotations

import cmath
import itertools
from dataclasses import dataclass, field

_SUPER = {"ˣ": "x", "ʸ": "y", "ᶻ": "z", "⁺": "+", "⁻": "-"}
_SUB = {chr(0x2080 + d): d for d in range(10)}

# single-site operators as {input bit: (output bit, coefficient)}
_SITE_OPS = {
    "x": {0: (1, 1.0 + 0j), 1: (0, 1.0 + 0j)},
    "y": {0: (1, 1j), 1: (0, -1j)},
    "z": {0: (0, 1.0 + 0j), 1: (1, -1.0 + 0j)},
    "+": {1: (0, 1.0 + 0j)},  # |up><down|
    "-": {0: (1, 1.0 + 0j)},
    "I": {0: (0, 1.0 + 0j), 1: (1, 1.0 + 0j)},
}


def parse_expression(expr: str):
    """'0.8 × σˣ₀ σˣ₁' -> (0.8+0j, [('x', 0, 1.0), ('x', 1, 1.0)])."""
    scalar = 1.0 + 0j
    factors = []
    for tok in expr.replace("×", " ").replace("*", " ").split():
        if tok[0] in ("σ", "S"):
            pref = 1.0 if tok[0] == "σ" else 0.5
            if len(tok) < 3 or tok[1] not in _SUPER:
                raise ValueError(f"cannot parse operator {tok!r} in {expr!r}")
            idx = 0
            for ch in tok[2:]:
                if ch not in _SUB:
                    raise ValueError(f"cannot parse site index in {tok!r}")
                idx = idx * 10 + _SUB[ch]
            factors.append((_SUPER[tok[1]], idx, pref))
        else:
            scalar *= complex(tok)
    if not factors:
        raise ValueError(f"expression {expr!r} has no operators")
    return scalar, factors


_SPIN_ARROW = {"↑": 0, "↓": 1}


def parse_fermion_expression(expr: str, spinful: bool):
    """'-1 × c†₀↑ c₁↑' -> (-1+0j, [('+', 0, 0), ('-', 1, 0)]): kind in {'+', '-', 'n'}, local site, spin (0 up, 1 down)."""
    scalar = 1.0 + 0j
    factors = []
    for tok in expr.replace("×", " ").replace("*", " ").split():
        if tok[0] in ("c", "n"):
            rest = tok[1:]
            if tok[0] == "c" and rest.startswith("†"):
                kind, rest = "+", rest[1:]
            else:
                kind = "-" if tok[0] == "c" else "n"
            spin = None
            if rest and rest[-1] in _SPIN_ARROW:
                spin, rest = _SPIN_ARROW[rest[-1]], rest[:-1]
            if not rest or any(ch not in _SUB for ch in rest):
                raise ValueError(f"cannot parse site index in {tok!r}")
            idx = 0
            for ch in rest:
                idx = idx * 10 + _SUB[ch]
            if spinful and spin is None:
                raise ValueError(f"spinful-fermion operator {tok!r} needs a spin index (↑ or ↓)")
            if not spinful and spin is not None:
                raise ValueError(f"spinless-fermion operator {tok!r} takes no spin index")
            factors.append((kind, idx, spin or 0))
        elif tok[0] in ("σ", "S"):
            raise ValueError(f"spin operator {tok!r} in a fermionic expression {expr!r}")
        else:
            scalar *= complex(tok)
    if not factors:
        raise ValueError(f"expression {expr!r} has no operators")
    return scalar, factors


def fermion_monomial_terms(expr: str, sites, spinful: bool, number_sites: int):
    """Terms (v, m, r, x, s) of one fermionic monomial on one tuple of global sites (sign convention: module docstring)."""
    scalar, factors = parse_fermion_expression(expr, spinful)
    k = 1 + max(f[1] for f in factors)
    if len(sites) != k:
        raise ValueError(f"expression {expr!r} needs {k} sites, got {sites}")
    if len(set(sites)) != len(sites):
        raise ValueError(f"repeated site in {sites}")
    modes = [int(sites[i]) + (number_sites if s else 0) for _, i, s in factors]
    touched = sorted(set(modes))
    M = 0
    for q in touched:
        M |= 1 << q
    s_mask = 0
    for (kind, _, _), q in zip(factors, modes):
        if kind != "n":
            s_mask ^= (1 << q) - 1
    s_mask &= ~M
    terms = []
    for pat in range(1 << len(touched)):
        r = 0
        for j, q in enumerate(touched):
            if (pat >> j) & 1:
                r |= 1 << q
        occ, v = r, scalar
        for (kind, _, _), q in reversed(list(zip(factors, modes))):  # written left-to-right, acting right-to-left
            bit = 1 << q
            if kind == "n":
                if not occ & bit:
                    v = 0
                    break
                continue
            if (kind == "+") == bool(occ & bit):
                v = 0
                break
            if bin(occ & M & (bit - 1)).count("1") & 1:
                v = -v
            occ ^= bit
        if v != 0:
            terms.append((complex(v), M, r, r ^ occ, s_mask))
    return terms


def _compose(first, second):
    """site operator `second` applied after `first`."""
    out = {}
    for b, (a, c) in first.items():
        if a in second:
            a2, c2 = second[a]
            out[b] = (a2, c * c2)
    return out


def _site_alternatives(op):
    """A single-site non-branching operator as mutually exclusive alternatives
    (needs_projector, r_bit, flip, sign, coeff): Pauli-like operators need no projector."""
    if 0 in op and 1 in op:
        (a0, c0), (a1, c1) = op[0], op[1]
        flip0, flip1 = a0 != 0, a1 != 1
        if flip0 == flip1 and c1 == c0:
            return [(False, 0, flip0, False, c0)]
        if flip0 == flip1 and c1 == -c0:
            return [(False, 0, flip0, True, c0)]
    alts = []
    for b, (a, c) in op.items():
        alts.append((True, b, a != b, False, c))
    return alts


def monomial_terms(expr: str, sites):
    """Terms (v, m, r, x, s) of one monomial on one tuple of global site indices."""
    scalar, factors = parse_expression(expr)
    per_site = {}
    order = []
    # operators written left-to-right act right-to-left on a ket
    for kind, idx, pref in reversed(factors):
        op = {b: (a, c * pref) for b, (a, c) in _SITE_OPS[kind].items()}
        if idx in per_site:
            per_site[idx] = _compose(per_site[idx], op)
        else:
            per_site[idx] = op
            order.append(idx)
    k = 1 + max(per_site)
    if len(sites) != k:
        raise ValueError(f"expression {expr!r} needs {k} sites, got {sites}")
    if len(set(sites)) != len(sites):
        raise ValueError(f"repeated site in {sites}")
    alts_per_site = [(idx, _site_alternatives(per_site[idx])) for idx in order]
    terms = []
    for combo in itertools.product(*[alts for _, alts in alts_per_site]):
        v = scalar
        m = r = x = s = 0
        for (idx, _), (need, rbit, flip, sign, c) in zip(alts_per_site, combo):
            bit = 1 << int(sites[idx])
            v *= c
            if need:
                m |= bit
                if rbit:
                    r |= bit
            if flip:
                x |= bit
            if sign:
                s |= bit
        if v != 0:
            terms.append((complex(v), m, r, x, s))
    return terms


PARTICLES = {"spin-1/2": 0, "spinful-fermion": 1, "spinless-fermion": 2}  # ls_hs_particle_type


@dataclass
class BasisSpec:
    number_sites: int
    hamming_weight: int = -1  # -1: unrestricted
    spin_inversion: int = 0
    permutations: list = field(default_factory=list)
    sectors: list = field(default_factory=list)
    particle: str = "spin-1/2"
    number_particles: int = -1  # fermions: -1 unrestricted
    number_up: int = -1  # spinful fermions: -1 = only number_particles fixed
    spin_flip: int = 0  # spinful fermions with number_up: the up <-> down flip's character (+1 / -1), 0 = none

    @property
    def is_fermionic(self) -> bool:
        return self.particle != "spin-1/2"


@dataclass
class OperatorSpec:
    terms: list  # [(v complex, m, r, x, s)]


def parse_basis(cfg: dict) -> BasisSpec:
    b = cfg["basis"]
    hw = b.get("hamming_weight", None)
    inv = b.get("spin_inversion", None)
    syms = b.get("symmetries", None) or []
    particle = b.get("particle") or "spin-1/2"
    if particle not in PARTICLES:
        raise ValueError(f"unknown particle {particle!r} (spin-1/2, spinful-fermion or spinless-fermion)")
    if particle != "spin-1/2":
        if "number_spins" in b:
            raise ValueError(f"number_spins is a key of spin-1/2 bases, not of particle {particle!r} (use number_sites)")
        # symmetries: spinless fermions (mode permutations), and the spinful (N, N_up) product basis (site permutations lifted to both
        # species, spin_flip); the N-only spinful basis with symmetries is a spinless one on 2 L modes and stays refused
        lifted = particle == "spinful-fermion" and b.get("number_up", None) is not None
        for key in ("hamming_weight", "spin_inversion", "symmetries"):
            if b.get(key) and not (key == "symmetries" and (particle == "spinless-fermion" or lifted)):
                raise ValueError(f"{key} is not supported for particle {particle!r}" + (" without number_up" if key == "symmetries" else ""))
        flip = b.get("spin_flip", None) or 0
        if flip and not lifted:
            raise ValueError(f"spin_flip is a key of spinful-fermion bases with number_up, not of particle {particle!r}"
                             + (" without number_up" if particle == "spinful-fermion" else ""))
        if flip not in (0, 1, -1):
            raise ValueError("spin_flip must be 1 or -1")
        if "number_sites" not in b:
            raise ValueError(f"particle {particle!r} needs number_sites")
        npart, nup = b.get("number_particles", None), b.get("number_up", None)
        if particle == "spinless-fermion" and nup is not None:
            raise ValueError("number_up is a key of spinful-fermion bases")
        if nup is not None and npart is None:
            raise ValueError("a fixed number_up needs a fixed number_particles")
        L = int(b["number_sites"])
        perms, sectors = _parse_symmetries(syms, L)
        if flip and 2 * int(nup) != int(npart):
            raise ValueError("spin_flip requires number_up == number_particles - number_up")
        return BasisSpec(number_sites=L, particle=particle, permutations=perms, sectors=sectors, spin_flip=int(flip),
                         number_particles=-1 if npart is None else int(npart), number_up=-1 if nup is None else int(nup))
    return BasisSpec(
        number_sites=int(b["number_spins"]),
        hamming_weight=-1 if hw is None else int(hw),
        spin_inversion=0 if inv is None else int(inv),
        permutations=[[int(v) for v in s["permutation"]] for s in syms],
        sectors=[int(s["sector"]) for s in syms],
    )


def _parse_symmetries(syms, L):
    """`symmetries:` of a fermionic basis: permutations of the number_sites modes (spinless) or sites (spinful); csrc/yaml.c checks
    the same"""
    perms, sectors = [], []
    for g, s in enumerate(syms):
        p = s.get("permutation") if isinstance(s, dict) else None
        if not isinstance(p, list) or len(p) != L or "sector" not in s:
            raise ValueError(f"basis.symmetries[{g}]: expected {{permutation: [{L} sites], sector: int}}")
        perms.append([int(v) for v in p])
        sectors.append(int(s["sector"]))
    return perms, sectors


def parse_operator(section: dict, basis: BasisSpec = None) -> OperatorSpec:
    """`basis` decides the operator language: σ / S for spin-1/2 (or None), c† / c / n for fermionic bases."""
    fermionic = basis is not None and basis.is_fermionic
    terms = []
    for t in section["terms"]:
        if "expression" not in t:
            raise ValueError("only the `expression:` schema is supported (data/*.yaml); "
                             "old-schema `matrix:` files are inputs of input_for_matvec.py only")
        for sites in t["sites"]:
            if fermionic:
                terms.extend(fermion_monomial_terms(t["expression"], [int(q) for q in sites],
                                                    basis.particle == "spinful-fermion", basis.number_sites))
            else:
                terms.extend(monomial_terms(t["expression"], [int(q) for q in sites]))
    return OperatorSpec(terms)


def heisenberg_chain_config(L: int, symm: bool = False, spin_inversion=None) -> dict:
    """The reference's chain inputs, generated: identical content to
    /root/reference/data/heisenberg_chain_{L}[_symm].yaml (checked in tests when the reference is
    mounted).  Needed because nothing may read /root/reference at run time on the GPU box."""
    basis = {"number_spins": L, "hamming_weight": L // 2}
    if symm:
        basis["spin_inversion"] = 1
        basis["symmetries"] = [
            {"permutation": [(i + 1) % L for i in range(L)], "sector": 0},
            {"permutation": [L - 1 - i for i in range(L)], "sector": 0},
        ]
    else:
        if spin_inversion is not None:
            basis["spin_inversion"] = spin_inversion
        basis["symmetries"] = []
    lattice = [[i, (i + 1) % L] for i in range(L)]
    terms = [{"expression": e, "sites": lattice} for e in ("σˣ₀ σˣ₁", "σʸ₀ σʸ₁", "σᶻ₀ σᶻ₁")]
    return {"basis": basis, "hamiltonian": {"name": "Heisenberg Hamiltonian", "terms": terms}}


def hubbard_config(sites: int, bonds, t=1.0, U=4.0, number_up=None, number_down=None, V=0.0, peierls=0.0, symmetries=None,
                   spin_flip=None) -> dict:
    """Spinful Hubbard model -t sum_<ij>,s (e^{i phi} c+_is c_js + h.c.) + U sum_i n_i↑ n_i↓ + V sum_<ij> n_i n_j over `bonds`
    (pairs (i, j)); half filling with N↑ = N↓ by default.  `symmetries` ([{permutation: sites, sector}]) and `spin_flip` (±1) go into
    the basis section as they are: the sector of the (N↑, N↓) basis the model is projected on."""
    nu = sites // 2 if number_up is None else number_up
    nd = sites // 2 if number_down is None else number_down
    bonds = [[int(i), int(j)] for i, j in bonds]
    fwd = complex(-t) * cmath.exp(1j * peierls)
    terms = []
    for s in ("↑", "↓"):
        terms.append({"expression": f"{_c(fwd)} × c†₀{s} c₁{s}", "sites": bonds})
        terms.append({"expression": f"{_c(fwd.conjugate())} × c†₁{s} c₀{s}", "sites": bonds})
    if U:
        terms.append({"expression": f"{U!r} × n₀↑ n₀↓", "sites": [[i] for i in range(sites)]})
    if V:
        for s1 in ("↑", "↓"):
            for s2 in ("↑", "↓"):
                terms.append({"expression": f"{V!r} × n₀{s1} n₁{s2}", "sites": bonds})
    basis = {"particle": "spinful-fermion", "number_sites": sites, "number_particles": nu + nd, "number_up": nu}
    if symmetries:
        basis["symmetries"] = [{"permutation": [int(v) for v in s["permutation"]], "sector": int(s["sector"])} for s in symmetries]
    if spin_flip:
        basis["spin_flip"] = int(spin_flip)
    return {"basis": basis, "hamiltonian": {"name": "Hubbard", "terms": terms}}


def _c(z: complex) -> str:
    return repr(z.real) if z.imag == 0 else f"{z.real!r}{z.imag:+.17g}j"
