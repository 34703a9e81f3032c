"""Reference for the sector-state expansion and the entanglement of bipartitions: pure numpy on oracle.model, nothing of the library.

The convention is the isometry of oracle.model.dense_sector_matrix -- basis vector P|r> / |P|r>| with
P = |G|^-1 sum_g conj(chi(g)) U_g -- for which, with state_info(s) = (rep, character, norm),
    <s|psi> = conj(character(s)) norm(rep) psi[index(rep)]
state_info_all is oracle.model.state_info over an array of states at once (the per-state Python loop takes minutes on the 12 870
states of the 4 x 4 lattice with its 256 group elements); tests/test_entanglement_host.py checks it against the oracle's own."""
import functools
import json

import numpy as np

from oracle import model as M


def _key(cfg):
    return json.dumps(cfg["basis"], sort_keys=True)


def ring(L, weight, sectors=None, inv=None, reflect=None):
    """basis config of an L-site ring: translation in sector `sectors` (None: no translation), reflection in sector `reflect`
    (None: none), spin inversion `inv`"""
    syms = []
    if sectors is not None:
        syms.append({"permutation": [(i + 1) % L for i in range(L)], "sector": int(sectors)})
    if reflect is not None:
        syms.append({"permutation": [L - 1 - i for i in range(L)], "sector": int(reflect)})
    basis = {"number_spins": L, "hamming_weight": weight, "symmetries": syms}
    if inv is not None:
        basis["spin_inversion"] = inv
    return {"basis": basis}


def full_states(model):
    """the ascending states of the same basis without symmetries"""
    L, w = model.number_sites, model.hamming_weight
    if w < 0:
        return np.arange(1 << L, dtype=np.uint64)
    out = []
    v = (1 << w) - 1
    top = v << (L - w)
    while True:
        out.append(v)
        if v == top or w == 0:
            break
        v = M.next_state_fixed_hamming(v)
    return np.array(out, dtype=np.uint64)


def apply_perm_all(p, states):
    out = np.zeros_like(states)
    for i, src in enumerate(p):
        out |= ((states >> np.uint64(int(src))) & np.uint64(1)) << np.uint64(i)
    return out


def _elements(model):
    """[(permutation, flip, character)] of the full group (permutations x optional spin flip), in the order of state_info"""
    out = []
    for p, ch in zip(model.group.perms, model.group.chars):
        out.append((p, False, complex(ch)))
        if model.spin_inversion != 0:
            out.append((p, True, complex(ch) * model.spin_inversion))
    return out


def state_info_all(model, states):
    """(representatives, characters, norms) of oracle.model.state_info for every state of the array"""
    states = np.asarray(states, dtype=np.uint64)
    mask = np.uint64(model.mask)
    elems = _elements(model)
    best = np.full(len(states), np.iinfo(np.uint64).max, dtype=np.uint64)
    best_ch = np.zeros(len(states), dtype=complex)
    stab = np.zeros(len(states), dtype=complex)
    for p, flip, ch in elems:
        t = apply_perm_all(p, states)
        if flip:
            t = t ^ mask
        stab += np.where(t == states, ch, 0.0)
        less = t < best  # strict: the first minimising element, as the oracle
        best = np.where(less, t, best)
        best_ch = np.where(less, ch, best_ch)
    assert np.abs(stab.imag).max(initial=0.0) < 1e-9
    n2 = stab.real / len(elems)
    norms = np.where(n2 > 1e-12, np.sqrt(np.maximum(n2, 0.0)), 0.0)
    return best, np.conj(best_ch), norms


@functools.lru_cache(maxsize=None)
def _tables_cached(key):
    cfg = {"basis": json.loads(key)}
    model = M.model_from_config(cfg)
    full = full_states(model)
    rep, ch, nrm = state_info_all(model, full)
    reps = np.unique(rep[(rep == full) & (nrm > 0)])
    idx = np.searchsorted(reps, rep)
    idx = np.where(idx < len(reps), idx, 0)
    live = (nrm > 0) & (reps[idx] == rep) if len(reps) else np.zeros(len(full), dtype=bool)
    coef = np.where(live, np.conj(ch) * nrm, 0.0)
    for a in (full, reps, idx, coef, live):
        a.setflags(write=False)
    return model, full, reps, idx, coef, live


def tables(cfg):
    """(model, full states, representatives, index of rep(s), conj(character(s)) norm(rep(s)) or 0, s has non-zero norm):
    computed once per basis and shared (read-only)"""
    return _tables_cached(_key(cfg))


def expand_full(cfg, psi):
    """the full-basis vector <s|psi> over full_states, by the formula above"""
    _model, _full, reps, idx, coef, _live = tables(cfg)
    psi = np.asarray(psi)
    assert psi.shape == (len(reps),)
    return coef * psi[idx]


def split_states(states, L, sites):
    """(a, b): the bits of every state on `sites` / on the other sites, compacted in ascending site order"""
    sites = sorted(int(s) for s in sites)
    rest = [s for s in range(L) if s not in sites]
    a = np.zeros_like(states)
    b = np.zeros_like(states)
    for k, s in enumerate(sites):
        a |= ((states >> np.uint64(s)) & np.uint64(1)) << np.uint64(k)
    for k, s in enumerate(rest):
        b |= ((states >> np.uint64(s)) & np.uint64(1)) << np.uint64(k)
    return a, b


def _popcount(x):
    return np.array([bin(int(v)).count("1") for v in x], dtype=np.int64)


def bipartition(cfg, vec, sites):
    """[(n_a, M)]: the blocks M[a, b] = <a, b|psi> of the full-basis vector `vec`, ordered by n_a (one block with n_a = -1 without a
    fixed weight); rows and columns in ascending order of a and b; empty blocks omitted"""
    model, full = tables(cfg)[0], tables(cfg)[1]
    L, w = model.number_sites, model.hamming_weight
    sites = list(range(L)) if sites is None else list(sites)
    a, b = split_states(full, L, sites)
    if w < 0:
        m = np.zeros((1 << len(sites), 1 << (L - len(sites))), dtype=vec.dtype)
        m[a.astype(np.int64), b.astype(np.int64)] = vec
        return [(-1, m)]
    na = _popcount(a)
    out = []
    for n in range(0, len(sites) + 1):
        sel = na == n
        if not sel.any():
            continue
        ua, ub = np.unique(a[sel]), np.unique(b[sel])
        assert len(ua) == M.binomial(len(sites), n) and len(ub) == M.binomial(L - len(sites), w - n)
        m = np.zeros((len(ua), len(ub)), dtype=vec.dtype)
        m[np.searchsorted(ua, a[sel]), np.searchsorted(ub, b[sel])] = vec[sel]
        out.append((n, m))
    return out


def spectrum(blocks):
    """(eigenvalues of rho_A in descending order, their n_a): the squared singular values of the blocks"""
    vals, nas = [], []
    for n, m in blocks:
        s = np.linalg.svd(m, compute_uv=False) ** 2
        vals.append(s)
        nas.append(np.full(len(s), n))
    vals, nas = np.concatenate(vals), np.concatenate(nas)
    order = np.argsort(-vals, kind="stable")
    return vals[order], nas[order]


def entropy(vals, renyi=1.0):
    p = vals[vals > 0]
    if renyi == 1.0:
        return float(-(p * np.log(p)).sum())
    return float(np.log((p ** renyi).sum()) / (1.0 - renyi))


def projector_columns(cfg):
    """(representatives, B): the columns P|r> / |P|r>| over full_states, by the explicit projector sum of
    oracle.model.dense_sector_matrix (no state_info, no characters of minimising elements)"""
    model, full, reps = tables(cfg)[0], tables(cfg)[1], tables(cfg)[2]
    elems = _elements(model)
    B = np.zeros((len(full), len(reps)), dtype=complex)
    cols = np.arange(len(reps))
    for p, flip, ch in elems:
        t = apply_perm_all(p, reps)
        if flip:
            t = t ^ np.uint64(model.mask)
        np.add.at(B, (np.searchsorted(full, t), cols), np.conj(ch) / len(elems))
    nrm = np.linalg.norm(B, axis=0)
    assert (nrm > 1e-9).all()
    return reps, B / nrm
