"""Finite-temperature static observables on the GPU (evolve.thermal_expectation, evolve.combine_sector_expectations) against
eigendecompositions of the sector matrices in numpy: B^+ H B and B^+ O B from the isometries of tests/cross_sector_reference.py with
operators built here as Kronecker products (spins), and from the signed projector columns of tests/fermion_entanglement_reference.py
with the Jordan-Wigner matrices of tests/fermion_jw.py (fermions).

Bounds (not tuned; the constants of the thermal_correlation tests): at most 3 cooling segments enter a value, each good to
eps = 1e-12 relative to its outgoing vector, and they enter bilinearly; the expectation kernel adds 2e-11 max(1, sum |v|) per unit
of <beta_k|beta_k> (tests/test_gpu_expectation.py).  Per column, with Z_k = <beta_k|beta_k> and 2-norms of the dense matrices:
    |partition - exact|          <= 1e-11 Z_k
    |numerator - exact|          <= (1e-10 ||O|| + 2e-11 max(1, sum |v|)) Z_k
    |energy_numerator - exact|   <= 1e-10 ||H|| Z_k
    |energy2_numerator - exact|  <= 1e-10 ||H||^2 Z_k
and for the ensemble quantities the same without Z_k, the specific heat within beta^2 3e-10 ||H||^2 (two second moments and a
product of first ones) and the entropy within 1e-10 (1 + beta ||H||)."""
import numpy as np
import pytest

import cross_sector_reference as X
import distributed_matvec_amd as D
import fermion_entanglement_reference as R
import fermion_jw as JW
import fermion_symm as F
from distributed_matvec_amd import config, expectation
from distributed_matvec_amd.evolve import combine_sector_expectations, thermal_expectation

pytestmark = pytest.mark.gpu
L = 8
BETAS = [0.0, 0.7, 3.0]
ATOL = 2e-11


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


# ---- dense spin operators on the full 2^L space: site i is bit i of the state index ------------------------------------------------
_S = {"x": np.array([[0, 1], [1, 0]], dtype=complex), "y": np.array([[0, -1j], [1j, 0]], dtype=complex), "z": np.diag([1.0 + 0j, -1.0])}


def _site(op, i):
    return np.kron(np.kron(np.eye(1 << (L - 1 - i)), op), np.eye(1 << i))


def _dot(i, j):
    return sum(_site(_S[a], i) @ _site(_S[a], j) for a in "xyz")


def _heisenberg_section():
    bonds = [[i, (i + 1) % L] for i in range(L)]
    return {"name": "Heisenberg", "terms": [{"expression": e, "sites": bonds} for e in ("σˣ₀ σˣ₁", "σʸ₀ σʸ₁", "σᶻ₀ σᶻ₁")]}


def _operators():
    """(sections, dense matrices on 2^L): sigma^z_0 sigma^z_j for j = 1..4 and the dimer-dimer operator (S_0.S_1)(S_2.S_3); none of
    them is invariant under the translations"""
    secs = [{"terms": [{"expression": "σᶻ₀ σᶻ₁", "sites": [[0, j]]}]} for j in range(1, 5)]
    dense = [_site(_S["z"], 0) @ _site(_S["z"], j) for j in range(1, 5)]
    secs.append(expectation.dimer_section((0, 1), (2, 3)))
    dense.append(_dot(0, 1) @ _dot(2, 3) / 16.0)
    return secs, dense


_cache = {}


def _full_space():
    if "full" not in _cache:
        secs, dense = _operators()
        H = sum(_dot(i, (i + 1) % L) for i in range(L))
        _cache["full"] = (secs, dense, H)
    return _cache["full"]


def _sector(k):
    """{"H", "O": sector matrices; "E", "U"; "norm_h", "norm_o", "sum_v"; "bounds"} of the ring at weight 4 and momentum k"""
    if k not in _cache:
        secs, dense, H = _full_space()
        cfg = X.ring(L, 4, k)
        reps, B = X.isometry(cfg)
        Hs = B.conj().T @ H @ B
        assert np.abs(Hs - Hs.conj().T).max() <= 1e-12
        Hs = 0.5 * (Hs + Hs.conj().T)
        E, U = np.linalg.eigh(Hs)
        Os = [B.conj().T @ O @ B for O in dense]
        basis = D.loadConfigFromDict({"basis": cfg["basis"]})
        sum_v = [sum(abs(t[0]) for t in config.parse_operator(sec, basis.spec).terms) for sec in secs]
        w = E[-1] - E[0]
        _cache[k] = {"cfg": {"basis": cfg["basis"], "hamiltonian": _heisenberg_section()}, "H": Hs, "O": Os, "E": E, "U": U, "n": len(reps),
                     "norm_h": float(np.linalg.norm(Hs, 2)), "norm_o": [float(np.linalg.norm(O, 2)) for O in Os], "sum_v": sum_v,
                     "bounds": (float(E[0] - 0.01 * w), float(E[-1] + 0.01 * w)), "secs": secs}
    return _cache[k]


def _o_bound(norm_o, sum_v):
    return 1e-10 * norm_o + ATOL * max(1.0, sum_v)


def _trace_reference(E, U, Os, H, betas):
    """Tr[e^{-beta H} .] / Z of every operator, <H>, the specific heat, ln Z and the entropy from an eigendecomposition"""
    vals, en, heat, logz, ent = [], [], [], [], []
    for beta in betas:
        p = np.exp(-beta * (E - E[0]))
        Z = p.sum()
        vals.append([((U.conj().T @ O @ U).diagonal() * p).sum() / Z for O in Os])
        e1, e2 = (E * p).sum() / Z, (E * E * p).sum() / Z
        en.append(e1); heat.append(beta ** 2 * (e2 - e1 ** 2))
        lz = np.log(Z) - beta * E[0]
        logz.append(lz); ent.append(lz + beta * e1)
    return np.array(vals), np.array(en), np.array(heat), np.array(logz), np.array(ent)


def test_explicit_vectors_match_the_eigendecomposition(torch):
    """the 10 states of the ring at weight 4, k = 0; K = 3 columns; every recorded quantity per column"""
    d = _sector(0)
    assert d["n"] == 10
    basis = D.loadConfigFromDict({"basis": d["cfg"]["basis"]})
    reps, _ = D.enumerateStates(basis, 1)
    K = 3
    Rv = torch.stack([D.fillRandom(reps[0], 21 + k, torch.float64) for k in range(K)], dim=1)
    res = thermal_expectation(d["cfg"], d["secs"], BETAS, vectors=Rv, bounds=d["bounds"])
    assert res.kernel == "k_expect_blk" and res.dimension == 10 and res.bounds == d["bounds"] and res.reference_energy == d["bounds"][0]
    assert res.numerator.shape == (3, 5, K) and res.partition.shape == (3, K) and res.values.shape == (3, 5)
    assert res.energy_numerator.shape == (3, K) and res.energy2_numerator.shape == (3, K)
    assert res.orders.shape == (3,) and res.orders[0] == 0 and (res.orders[1:] > 0).all()
    assert res.matvec_columns >= K * (int(res.orders.sum()) + 3)  # every order and one energy pass per beta move K columns
    E, U, H, e_ref = d["E"], d["U"], d["H"], res.reference_energy
    Rn = Rv.cpu().numpy()
    worst = {"partition": 0.0, "numerator": 0.0, "energy": 0.0, "energy2": 0.0}
    for j, beta in enumerate(BETAS):
        b = U @ (np.exp(-0.5 * beta * (E - e_ref))[:, None] * (U.conj().T @ Rn))
        Z = (np.abs(b) ** 2).sum(axis=0)
        assert Z.min() > 1e-6
        worst["partition"] = max(worst["partition"], float((np.abs(res.partition[j] - Z) / (1e-11 * Z)).max()))
        for o, O in enumerate(d["O"]):
            want = ((b.conj()) * (O @ b)).sum(axis=0)
            r = np.abs(res.numerator[j, o] - want) / (_o_bound(d["norm_o"][o], d["sum_v"][o]) * Z)
            worst["numerator"] = max(worst["numerator"], float(r.max()))
        Hb = H @ b
        e1 = (b.conj() * Hb).sum(axis=0).real
        e2 = (np.abs(Hb) ** 2).sum(axis=0)
        worst["energy"] = max(worst["energy"], float((np.abs(res.energy_numerator[j] - e1) / (1e-10 * d["norm_h"] * Z)).max()))
        worst["energy2"] = max(worst["energy2"], float((np.abs(res.energy2_numerator[j] - e2) / (1e-10 * d["norm_h"] ** 2 * Z)).max()))
    print("thermal_expectation, explicit vectors: worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + f"; orders {res.orders.tolist()}")
    assert all(v <= 1.0 for v in worst.values()), worst
    # the derived quantities are what their definitions say
    Zs = res.partition.sum(axis=1)
    assert np.abs(res.values - res.numerator.sum(axis=2) / Zs[:, None]).max() <= 1e-14
    assert np.abs(res.energy - res.energy_numerator.sum(axis=1) / Zs).max() <= 1e-13 * d["norm_h"]
    assert np.abs(res.log_partition - (np.log(10 / K * Zs) - np.array(BETAS) * e_ref)).max() <= 1e-13
    assert np.abs(res.entropy - (res.log_partition + np.array(BETAS) * res.energy)).max() <= 1e-12


def _check_ensemble(res, ref, betas, norm_h, o_bounds, label):
    vals, en, heat, logz, ent = ref
    betas = np.asarray(betas)
    ratios = {"values": float((np.abs(res.values - vals) / np.asarray(o_bounds)[None, :]).max()),
              "energy": float((np.abs(res.energy - en) / (1e-10 * norm_h)).max()),
              "entropy": float((np.abs(res.entropy - ent) / (1e-10 * (1.0 + betas * norm_h))).max()),
              "log_partition": float((np.abs(res.log_partition - logz) / (1e-10 * (1.0 + betas * norm_h))).max())}
    hot = betas > 0
    if hot.any():
        ratios["specific_heat"] = float((np.abs(res.specific_heat - heat)[hot] / (betas[hot] ** 2 * 3e-10 * norm_h ** 2)).max())
    assert res.specific_heat[~hot].tolist() == [0.0] * int((~hot).sum())
    print(f"thermal_expectation, {label}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (label, ratios)


def test_a_whole_basis_is_the_exact_trace(torch):
    """vectors = the 10 x 10 identity: the typicality average IS the trace over the sector"""
    d = _sector(0)
    eye = torch.eye(10, dtype=torch.float64, device="cuda")
    res = thermal_expectation(d["cfg"], d["secs"], BETAS, vectors=eye, bounds=d["bounds"])
    assert res.kernel == "k_expect_blk" and res.numerator.shape == (3, 5, 10)
    ref = _trace_reference(d["E"], d["U"], d["O"], d["H"], BETAS)
    _check_ensemble(res, ref, BETAS, d["norm_h"], [_o_bound(n, s) for n, s in zip(d["norm_o"], d["sum_v"])], "identity vectors, k = 0")
    # beta = 0: the plain trace and ln D
    for o, O in enumerate(d["O"]):
        assert abs(res.values[0, o] - np.trace(O) / 10) <= _o_bound(d["norm_o"][o], d["sum_v"][o])
    assert abs(res.entropy[0] - np.log(10)) <= 1e-10
    assert np.abs(ref[0]).max() > 1e-2 and np.abs(ref[0][2] - ref[0][0]).max() > 1e-2  # (the values move with beta)
    # complex128 on request gives the same numbers
    res_c = thermal_expectation(d["cfg"], d["secs"], BETAS, vectors=eye, bounds=d["bounds"], dtype=torch.complex128)
    _check_ensemble(res_c, ref, BETAS, d["norm_h"], [_o_bound(n, s) for n, s in zip(d["norm_o"], d["sum_v"])], "identity vectors, k = 0, c128")


def test_canonical_ensemble_over_all_momentum_sectors(torch):
    """the eight momentum sectors with identity vectors, one E_ref and one pair of bounds, combined by combine_sector_expectations,
    against the dense trace over the 70 states of the weight sector: the operators are not translation-invariant one by one"""
    secs, dense, H = _full_space()
    states = np.array([s for s in range(1 << L) if bin(s).count("1") == 4])
    assert len(states) == 70
    H70 = H[np.ix_(states, states)]
    O70 = [O[np.ix_(states, states)] for O in dense]
    E, U = np.linalg.eigh(0.5 * (H70 + H70.conj().T))
    w = E[-1] - E[0]
    bounds = (float(E[0] - 0.01 * w), float(E[-1] + 0.01 * w))
    norm_h = float(np.linalg.norm(H70, 2))
    results, dims = [], []
    for k in range(L):
        d = _sector(k)
        eye = torch.eye(d["n"], dtype=torch.float64, device="cuda")
        results.append(thermal_expectation(d["cfg"], secs, BETAS, vectors=eye, bounds=bounds, reference_energy=bounds[0]))
        dims.append(results[-1].dimension)
        assert results[-1].reference_energy == bounds[0] and results[-1].kernel == "k_expect_blk"
    assert dims == [10, 8, 9, 8, 10, 8, 9, 8]
    got = combine_sector_expectations(results)
    assert got.dimension == 70 and got.values.shape == (3, 5)
    ref = _trace_reference(E, U, O70, H70, BETAS)
    o_bounds = [_o_bound(float(np.linalg.norm(O, 2)), s) for O, s in zip(O70, _sector(0)["sum_v"])]
    _check_ensemble(got, ref, BETAS, norm_h, o_bounds, "all momentum sectors")
    one = _trace_reference(_sector(0)["E"], _sector(0)["U"], _sector(0)["O"], _sector(0)["H"], BETAS)
    assert np.abs(one[0] - ref[0]).max() > 1e-3  # (one sector alone is another ensemble)


def test_random_vectors_are_reproducible_and_typical(torch):
    """vectors=None: random signs in float64 from the seed; the same call twice gives the same numbers, and the numbers are those of
    the dense typicality average over these very vectors"""
    from distributed_matvec_amd import kpm

    d = _sector(0)
    a = thermal_expectation(d["cfg"], d["secs"][:2], [0.0, 1.0], num_vectors=4, seed=5, bounds=d["bounds"])
    b = thermal_expectation(d["cfg"], d["secs"][:2], [0.0, 1.0], num_vectors=4, seed=5, bounds=d["bounds"])
    assert a.numerator.tobytes() == b.numerator.tobytes() and a.partition.tobytes() == b.partition.tobytes()
    Rn = kpm.random_phase_block(10, 4, torch.float64, 5).cpu().numpy()
    assert set(np.unique(Rn)) == {-1.0, 1.0}
    E, U = d["E"], d["U"]
    bvec = U @ (np.exp(-0.5 * (E - a.reference_energy))[:, None] * (U.conj().T @ Rn))
    Z = (np.abs(bvec) ** 2).sum(axis=0)
    assert (np.abs(a.partition[1] - Z) <= 1e-11 * Z).all() and (np.abs(a.partition[0] - 10.0) <= 1e-13).all()
    for o in range(2):
        want = (bvec.conj() * (d["O"][o] @ bvec)).sum(axis=0)
        assert (np.abs(a.numerator[1, o] - want) <= _o_bound(d["norm_o"][o], d["sum_v"][o]) * Z).all()
    with pytest.raises(D.LsAmdError, match="cannot be honoured"):
        thermal_expectation(_sector(1)["cfg"], d["secs"][:1], [0.5], num_vectors=2, dtype=torch.float64)  # complex characters


def test_fermions_on_the_spinful_hubbard_ring(torch):
    """6 sites at (3, 3), k = 0, flip +1: double occupancy and Delta+_0 Delta_1 with identity vectors against the dense trace in the
    sector -- float64 through k_expect_blk_fermi"""
    case = R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0], flip=1)
    model = JW.hubbard_model(6, JW.ring(6), U=4.0)
    Hs = case.sector_matrix(model)
    assert np.abs(Hs - Hs.conj().T).max() <= 1e-12
    Hs = 0.5 * (Hs + Hs.conj().T)
    E, U = np.linalg.eigh(Hs)
    op_models = [[(1.0, [("n", 0, 0), ("n", 0, 1)])], [(1.0, [("+", 0, 0), ("+", 0, 1), ("-", 1, 1), ("-", 1, 0)])]]
    Os = [case.sector_matrix(m) for m in op_models]
    secs = [{"terms": JW.yaml_terms(m, True)} for m in op_models]
    n = len(case.reps)
    w = E[-1] - E[0]
    bounds = (float(E[0] - 0.01 * w), float(E[-1] + 0.01 * w))
    cfg = case.config(model)
    betas = [0.0, 1.0]
    assert n == 30
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    res = thermal_expectation(cfg, secs, betas, vectors=eye, bounds=bounds)
    assert res.kernel == "k_expect_blk_fermi" and res.dimension == n and res.numerator.shape == (2, 2, n)
    norm_h = float(np.linalg.norm(Hs, 2))
    ref = _trace_reference(E, U, Os, Hs, betas)
    _check_ensemble(res, ref, betas, norm_h, [_o_bound(float(np.linalg.norm(O, 2)), 1.0) for O in Os], "spinful Hubbard ring, identity vectors")
    assert abs(ref[0][1, 0]) > 1e-3 and abs(ref[0][1, 1]) > 1e-3
