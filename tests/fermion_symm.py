"""Independent reference for projected spinless-fermion bases (include/ls_hs.h): group closure, the permutation sign of a Fock state
by explicit inversion counting, orbit minima, norms n(r)^2 = |G|^-1 sum_{g in Stab(r)} chi(g) sign(g, r), and the projected matrix
B+ H B with H from fermion_jw.sector_matrix and the columns of B built as in oracle/model.py's projector, each U_g entry signed.
Shares no code with config.py or host.c."""
import itertools
import math

import numpy as np

from fermion_jw import sector_matrix, weight_states


def closure(L, generators, sectors):
    """{permutation tuple: character}; a permutation p maps a state a to (g.a)[i] = a[p[i]], and (g after h)[i] = h[g[i]]"""
    gens = []
    for p, k in zip(generators, sectors):
        p = tuple(int(v) for v in p)
        n, q = 1, p
        while q != tuple(range(L)):
            q = tuple(q[i] for i in p)
            n += 1
        gens.append((p, np.exp(-2j * np.pi * (k % n) / n)))
    elems = {tuple(range(L)): 1.0 + 0j}
    todo = [tuple(range(L))]
    while todo:
        e = todo.pop()
        for p, ch in gens:
            c = tuple(e[i] for i in p)
            if c not in elems:
                elems[c] = elems[e] * ch
                todo.append(c)
            elif abs(elems[c] - elems[e] * ch) > 1e-9:
                raise ValueError("sectors are incompatible with the group")
    return list(elems.items())


def apply(p, a):
    return sum(((a >> src) & 1) << i for i, src in enumerate(p))


def sign(p, a):
    """U_g c+_j U_g+ = c+_{q_j}, q = p^-1: the occupied modes, written in ascending order, move to q_j; the sign is the parity of
    the permutation that sorts them again -- counted pair by pair"""
    q = [0] * len(p)
    for i, src in enumerate(p):
        q[src] = i
    occ = [j for j in range(len(p)) if (a >> j) & 1]
    inv = sum(1 for x, y in itertools.combinations(occ, 2) if q[x] > q[y])
    return -1 if inv % 2 else 1


def state_info(group, a):
    """(orbit minimum, conj(chi(g0) sign(g0, a)) of a minimising g0, norm)"""
    best, ch0 = None, None
    stab = 0j
    for p, ch in group:
        t = apply(p, a)
        s = sign(p, a)
        if t == a:
            stab += ch * s
        if best is None or t < best:
            best, ch0 = t, np.conj(ch * s)
    n2 = stab.real / len(group)
    return best, ch0, (math.sqrt(n2) if n2 > 1e-12 else 0.0)


def representatives(L, N, group):
    """ascending orbit minima with non-zero norm, and their norms"""
    reps, norms = [], []
    for a in weight_states(L, N):
        r, _, n = state_info(group, int(a))
        if r == int(a) and n > 0:
            reps.append(r)
            norms.append(n)
    return np.array(reps, dtype=np.uint64), np.array(norms)


def projector_columns(L, N, group, reps):
    """B: column r = P|r> / ||P|r>||, P = |G|^-1 sum_g conj(chi(g)) U_g, U_g|a> = sign(g, a)|g.a>, on the weight-N words"""
    states = weight_states(L, N)
    pos = {int(s): i for i, s in enumerate(states)}
    B = np.zeros((len(states), len(reps)), dtype=complex)
    for c, r in enumerate(reps):
        r = int(r)
        for p, ch in group:
            B[pos[apply(p, r)], c] += np.conj(ch) * sign(p, r) / len(group)
        B[:, c] /= np.linalg.norm(B[:, c])
    return states, B


def projected_matrix(model, L, N, group, reps):
    states, B = projector_columns(L, N, group, reps)
    H = sector_matrix(model, L, False, states).toarray()
    return B.conj().T @ H @ B


def translations(L):
    return [[(i + 1) % L for i in range(L)]]


def dihedral(L):
    return [[(i + 1) % L for i in range(L)], [L - 1 - i for i in range(L)]]


def torus(w, h, point_group=True):
    """translations of a w x h torus (site = y w + x); on a square one also the rotation by 90 degrees and a reflection (D4)"""
    tx = [y * w + (x + 1) % w for y in range(h) for x in range(w)]
    ty = [((y + 1) % h) * w + x for y in range(h) for x in range(w)]
    gens = [tx, ty]
    if point_group and w == h:
        gens.append([(w - 1 - x) * w + y for y in range(h) for x in range(w)])  # rotation
        gens.append([y * w + (w - 1 - x) for y in range(h) for x in range(w)])  # reflection x -> -x
    return gens


def tv_model(bonds, t=1.0, V=0.0, phase=0.0):
    """-t e^{i phase} c+_i c_j + h.c. + V n_i n_j on every bond"""
    hop = -t * np.exp(1j * phase)
    model = []
    for i, j in bonds:
        model.append((hop, [("+", i, 0), ("-", j, 0)]))
        model.append((np.conj(hop), [("+", j, 0), ("-", i, 0)]))
        if V:
            model.append((V, [("n", i, 0), ("n", j, 0)]))
    return model


def free_ring_energy(L, N, s, t=1.0):
    """lowest energy of -t sum (c+_i c_{i+1} + h.c.) on an L-site ring with N particles and total momentum s (mod L): a subset S
    of N distinct momenta with sum S = s mod L, minimising sum -2 t cos(2 pi m / L) -- a DP over (momentum, count, sum mod L)"""
    INF = float("inf")
    best = [[INF] * L for _ in range(N + 1)]
    best[0][0] = 0.0
    for m in range(L):
        e = -2.0 * t * math.cos(2.0 * math.pi * m / L)
        for c in range(min(N, m + 1), 0, -1):
            prev, cur = best[c - 1], best[c]
            for r in range(L):
                if prev[r] < INF:
                    v = prev[r] + e
                    rr = (r + m) % L
                    if v < cur[rr]:
                        cur[rr] = v
    return best[N][s % L]
