"""Fermionic bases on the GPU: product-basis enumeration bit-exact against itertools, the product state index, and y element by
element against the dense Jordan-Wigner matrix (tests/fermion_jw.py) -- the species-split row kernel where it must run, the
generic kernels (with their signs) everywhere else."""
import os

import numpy as np
import pytest

import distributed_matvec_amd as D
from distributed_matvec_amd import config
from fermion_jw import (dense, hubbard_model, product_states, restrict, ring, square, weight_states, yaml_terms)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def spinful_cfg(model, L, N, Nup):
    return {"basis": {"particle": "spinful-fermion", "number_sites": L, "number_particles": N, "number_up": Nup},
            "hamiltonian": {"terms": yaml_terms(model, True)}}


def spinless_cfg(model, L, N):
    return {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": N},
            "hamiltonian": {"terms": yaml_terms(model, False)}}


def check_matvec(torch, cfg, H, states, modes=("pull", "push"), parts=(1, 3), kernel=None):
    rs = np.random.RandomState(11)
    x = rs.rand(len(states)) - 0.5
    xc = x + 1j * (rs.rand(len(states)) - 0.5)
    is_real = np.abs(H.imag).max() == 0 if H.size else True
    for P in parts:
        basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
        reps, masks = D.enumerateStates(basis, P)
        got_reps = D.arrFromHashedToBlock(reps, masks).cpu().numpy().view(np.uint64)
        assert np.array_equal(got_reps, states)
        for vec in ((x, xc) if is_real else (xc,)):
            for mode in (modes if P == 1 else ("auto",)):
                xb = torch.from_numpy(np.ascontiguousarray(vec)).cuda()
                xs = D.arrFromBlockToHashed(xb, masks, P)
                ys = [torch.zeros_like(v) for v in xs]
                pl = D.matrixVectorProduct(h, xs, ys, reps, mode=mode)
                got = D.arrFromHashedToBlock(ys, masks).cpu().numpy()
                want = H @ vec
                assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (P, mode, vec.dtype, pl.kernel)
                if kernel is not None and P == 1 and mode == "pull":
                    assert (pl.kernel == "direct-pull+hubbard") == kernel, pl.kernel


@pytest.mark.parametrize("L,nu,nd", [(4, 2, 2), (5, 3, 1), (5, 0, 2), (4, 4, 1), (6, 0, 0), (3, 3, 3), (7, 2, 5)])
def test_product_enumeration_is_bit_exact(torch, L, nu, nd):
    basis = D.Basis.fromSpec(config.BasisSpec(number_sites=L, particle="spinful-fermion", number_particles=nu + nd, number_up=nu))
    for P in (1, 3):
        reps, masks = D.enumerateStates(basis, P)
        got = D.arrFromHashedToBlock(reps, masks).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, product_states(L, nu, nd)), (L, nu, nd, P)


HUBBARD = {
    "ring_6": (6, 3, 3, hubbard_model(6, ring(6), t=1.0, U=4.0)),
    "lattice_2x3": (6, 3, 2, hubbard_model(6, square(3, 2), t=1.0, U=2.0)),
    "ring_8": (8, 4, 4, hubbard_model(8, ring(8), t=1.0, U=4.0)),
    "lattice_2x4": (8, 3, 4, hubbard_model(8, square(4, 2), t=0.7, U=3.0)),
    "extended_ring_6": (6, 2, 3, hubbard_model(6, ring(6), t=1.0, U=4.0, V=0.8)),
    "peierls_ring_6": (6, 3, 3, hubbard_model(6, ring(6), t=1.0, U=2.0, phase=0.37)),
    "next_nearest_ring_7": (7, 3, 3, hubbard_model(7, ring(7) + [(i, (i + 2) % 7) for i in range(7)], t=0.6, U=1.5)),
}


@pytest.mark.parametrize("name", sorted(HUBBARD))
def test_hubbard_matches_dense_jordan_wigner(torch, name):
    L, nu, nd, model = HUBBARD[name]
    states = product_states(L, nu, nd)
    H = restrict(dense(model, L, True), states).toarray()
    check_matvec(torch, spinful_cfg(model, L, nu + nd, nu), H, states, kernel=True)


def test_density_assisted_hop_takes_the_species_kernel(torch):
    L = 6
    model = hubbard_model(L, ring(L), U=3.0) + [(0.4, [("n", 2, 0), ("+", 0, 0), ("-", 4, 0)]), (0.4, [("n", 2, 0), ("+", 4, 0), ("-", 0, 0)])]
    states = product_states(L, 3, 2)
    H = restrict(dense(model, L, True), states).toarray()
    check_matvec(torch, spinful_cfg(model, L, 5, 3), H, states, kernel=True)


@pytest.mark.parametrize("extra", ["pair_hopping", "spin_exchange"])
def test_non_separable_operator_takes_the_generic_kernel(torch, extra):
    L = 6
    model = hubbard_model(L, ring(L), U=2.0)
    if extra == "pair_hopping":
        model += [(0.5, [("+", 0, 0), ("+", 0, 1), ("-", 3, 1), ("-", 3, 0)]), (0.5, [("+", 3, 0), ("+", 3, 1), ("-", 0, 1), ("-", 0, 0)])]
    else:
        model += [(0.7, [("+", 1, 0), ("-", 1, 1), ("+", 4, 1), ("-", 4, 0)]), (0.7, [("+", 4, 0), ("-", 4, 1), ("+", 1, 1), ("-", 1, 0)])]
    states = product_states(L, 3, 3)
    H = restrict(dense(model, L, True), states).toarray()
    check_matvec(torch, spinful_cfg(model, L, 6, 3), H, states, kernel=False)


def test_non_hermitian_hop(torch):
    L = 6
    model = hubbard_model(L, ring(L), U=1.0) + [(0.3, [("+", 0, 0), ("-", 2, 0)])]
    states = product_states(L, 3, 2)
    H = restrict(dense(model, L, True), states).toarray()
    check_matvec(torch, spinful_cfg(model, L, 5, 3), H, states, kernel=False)


def test_spinful_fixed_n_only(torch):
    L = 5
    model = hubbard_model(L, ring(L), U=2.0) + [(0.7, [("+", 1, 0), ("-", 1, 1)]), (0.7, [("+", 1, 1), ("-", 1, 0)])]
    states = weight_states(2 * L, 5)
    H = restrict(dense(model, L, True), states).toarray()
    check_matvec(torch, {"basis": {"particle": "spinful-fermion", "number_sites": L, "number_particles": 5},
                         "hamiltonian": {"terms": yaml_terms(model, True)}}, H, states, kernel=False)


def spinless_ring(L, t=1.0, V=0.0, phase=0.0):
    hop = -t * np.exp(1j * phase)
    model = []
    for i, j in ring(L):
        model.append((hop, [("+", i, 0), ("-", j, 0)]))
        model.append((np.conj(hop), [("+", j, 0), ("-", i, 0)]))
        if V:
            model.append((V, [("n", i, 0), ("n", j, 0)]))
    return model


@pytest.mark.parametrize("L,N,V,phase", [(8, 3, 0.0, 0.0), (8, 4, 1.3, 0.0), (9, 4, 0.5, 0.21), (10, -1, 0.0, 0.0)])
def test_spinless_ring_with_signed_closing_bond(torch, L, N, V, phase):
    model = spinless_ring(L, V=V, phase=phase)
    states = weight_states(L, N)
    H = restrict(dense(model, L, False), states).toarray()
    check_matvec(torch, spinless_cfg(model, L, N), H, states, kernel=False)


def open_spinless_chain(L, t=1.0, V=1.3):
    model = []
    for i in range(L - 1):
        model += [(-t, [("+", i, 0), ("-", i + 1, 0)]), (-t, [("+", i + 1, 0), ("-", i, 0)]), (V, [("n", i, 0), ("n", i + 1, 0)])]
    return model


# (model, LS_AMD_ROW_KERNEL) -> the kernel the plan must report.  Adjacent hops carry no string (s = 0) and are plain exchange
# pairs: the open chain is one exchange run and takes the staged chain kernel; the ring's closing bond carries the string of the
# L - 2 modes between its sites, so the classifier keeps it generic and the whole operator stays on k_direct.  The pair kernels
# take only zz diagonals, which density terms are not: under `pairs` both fall back to k_direct.
SWITCH_KERNELS = {
    ("open", "auto"): "direct-pull+staged", ("open", "generic"): "direct-pull", ("open", "pairs"): "direct-pull",
    ("ring", "auto"): "direct-pull", ("ring", "generic"): "direct-pull", ("ring", "pairs"): "direct-pull",
}


@pytest.mark.parametrize("row_kernel", ["auto", "generic", "pairs"])
@pytest.mark.parametrize("shape", ["open", "ring"])
def test_spinless_chain_under_every_row_kernel_switch(torch, row_kernel, shape, monkeypatch):
    monkeypatch.setenv("LS_AMD_ROW_KERNEL", row_kernel)
    L, N = 12, 5
    model = open_spinless_chain(L) if shape == "open" else spinless_ring(L, V=1.3)
    states = weight_states(L, N)
    H = restrict(dense(model, L, False), states).toarray().real
    basis, h = D.loadConfigFromDict(spinless_cfg(model, L, N), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    assert np.array_equal(reps[0].cpu().numpy().view(np.uint64), states)
    x = np.random.RandomState(2).rand(len(states)) - 0.5
    y = torch.zeros(len(states), dtype=torch.float64, device="cuda")
    pl = D.matrixVectorProduct(h, [torch.from_numpy(x).cuda()], [y], reps, mode="pull")
    assert pl.kernel == SWITCH_KERNELS[(shape, row_kernel)], pl.kernel
    want = H @ x
    assert np.abs(y.cpu().numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_generic_switch_keeps_k_direct(torch, monkeypatch):
    monkeypatch.setenv("LS_AMD_ROW_KERNEL", "generic")
    L, nu, nd, model = HUBBARD["ring_6"]
    states = product_states(L, nu, nd)
    H = restrict(dense(model, L, True), states).toarray()
    check_matvec(torch, spinful_cfg(model, L, nu + nd, nu), H, states, modes=("pull",), parts=(1,), kernel=False)


def test_hubbard_chain_16_state_index_and_edge_rows(torch):
    """Full-size hubbard_chain_16: count, order, index round trip, and > 1e5 rows at strip / tile seams against a numpy row
    evaluator of the same Hamiltonian."""
    import ctypes as C
    from math import comb

    from distributed_matvec_amd import _lib

    L, nu = 16, 8
    nA = comb(L, nu)
    cfg = config.hubbard_config(L, ring(L), t=1.0, U=4.0)
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, masks = D.enumerateStates(basis, 1)
    n = reps[0].numel()
    assert n == nA * nA
    r = reps[0]
    assert bool((r[1:] > r[:-1]).all())
    rs = np.random.RandomState(3)
    rows = np.unique(np.concatenate([
        np.arange(0, 4096), n - 1 - np.arange(4096),
        (np.arange(1, nA)[:, None] * nA + np.array([-2, -1, 0, 1])[None, :]).ravel(),  # strip seams
        (rs.randint(0, n // 256, 40000) * 256)[:, None].ravel() + rs.randint(-1, 1, 40000),  # tile seams
        rs.randint(0, n, 20000)]))
    rows = rows[(rows >= 0) & (rows < n)]
    assert len(rows) >= 100000
    states = r[torch.from_numpy(rows).cuda()].cpu().numpy().view(np.uint64)
    basis.uncheckedSetRepresentatives(r.cpu().numpy().view(np.uint64))  # what ls_hs_state_index searches (host array, borrowed)
    idx = np.full(len(rows), -7, dtype=np.int64)
    L_ = _lib.load()
    st = np.ascontiguousarray(states)
    L_.ls_hs_state_index(basis.payload, len(st), st.ctypes.data_as(_lib.c_u64p), 1, idx.ctypes.data_as(C.POINTER(C.c_ssize_t)), 1)
    _lib.raise_pending_halt()
    assert np.array_equal(idx, rows)
    # wrong weight in one half; right weights with a stray bit at or above 2 L (0xff | 0xff << 32)
    bad = np.array([int(states[0]) ^ 1, int(states[0]) | (1 << 24), 0xFF | (0xFF << 32)], dtype=np.uint64)
    bidx = np.zeros(3, dtype=np.int64)
    L_.ls_hs_state_index(basis.payload, 3, bad.ctypes.data_as(_lib.c_u64p), 1, bidx.ctypes.data_as(C.POINTER(C.c_ssize_t)), 1)
    assert (bidx < 0).all()
    x = torch.from_numpy(np.sin(0.37 * np.arange(n, dtype=np.float64)) * 0.5).cuda()
    y = torch.zeros_like(x)
    pl = D.matrixVectorProduct(h, [x], [y], reps, mode="pull")
    assert pl.kernel == "direct-pull+hubbard"
    got = y.cpu().numpy()[rows]
    xs = x.cpu().numpy()
    terms = config.parse_operator(cfg["hamiltonian"], config.parse_basis(cfg)).terms

    def index_of(s):
        lo, hi = s & 0xffff, s >> 16
        return np.array([_rank(int(v)) for v in hi]) * nA + np.array([_rank(int(v)) for v in lo])

    want = np.zeros(len(rows))
    a = states.astype(np.uint64)
    for v, m, rr, xx, s in terms:  # pull: y[i] = sum over terms acting on partner beta = i ^ x that land on i
        beta = a ^ np.uint64(xx)
        act = (beta & np.uint64(m)) == np.uint64(rr)
        if xx == 0:
            sign = 1 - 2 * (np.vectorize(lambda q: bin(int(q)).count("1") & 1)(beta & np.uint64(s)))
            want += np.where(act, v.real * sign * xs[rows], 0.0)
            continue
        ok = act & (np.vectorize(lambda q: bin(int(q & 0xffff)).count("1") == 8 and bin(int(q >> 16)).count("1") == 8)(beta))
        if not ok.any():
            continue
        sign = 1 - 2 * (np.vectorize(lambda q: bin(int(q)).count("1") & 1)(beta[ok] & np.uint64(s)))
        want[ok] += v.real * sign * xs[index_of(beta[ok])]
    assert np.abs(got - want).max() <= 1e-11


_RANK = {}


def _rank(w):
    if w not in _RANK:
        from math import comb
        k, r = 0, 0
        for p in range(64):
            if (w >> p) & 1:
                k += 1
                r += comb(p, k)
        _RANK[w] = r
    return _RANK[w]


def test_free_fermion_ground_state_energy(torch):
    """U = 0 on a 14-site ring, 7 up 7 down (11.8 M states): the closed-shell free-fermion energy."""
    from distributed_matvec_amd.diagonalize import diagonalize

    L = 14
    want = 2 * sum(-2 * np.cos(2 * np.pi * k / L) for k in range(-3, 4))
    assert abs(want - (-17.975836829739738)) < 1e-12
    r = diagonalize(config.hubbard_config(L, ring(L), t=1.0, U=0.0), num_evals=1, eps=1e-12)
    assert abs(float(r.eigenvalues[0]) - want) < 1e-8, r.eigenvalues


def test_small_interacting_spectrum(torch):
    L, nu, nd, model = HUBBARD["lattice_2x3"]
    states = product_states(L, nu, nd)
    Hd = restrict(dense(model, L, True), states).toarray()
    basis, h = D.loadConfigFromDict(spinful_cfg(model, L, nu + nd, nu), hamiltonian=True)
    reps, masks = D.enumerateStates(basis, 1)
    n = len(states)
    X = torch.eye(n, dtype=torch.float64, device="cuda")
    cols = []
    for j in range(n):
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        D.matrixVectorProduct(h, [X[j].contiguous()], [y], reps, mode="pull")
        cols.append(y.cpu().numpy())
    M = np.stack(cols, axis=1)
    assert np.allclose(np.linalg.eigvalsh(M), np.linalg.eigvalsh(Hd.real), atol=1e-10)


def test_adopted_foreign_spinful_basis(torch):
    """A prefix-only spinful basis and operator (nothing of ours behind the prefix), adopted and applied through the
    ls_chpl_kernels table entry (ls_chpl_matrix_vector_product)."""
    import ctypes as C

    from distributed_matvec_amd import _lib
    from test_host_tables import _ForeignBasis, _ForeignOperator

    lib = _lib.load()
    L, nu, nd, model = HUBBARD["ring_6"]
    states = product_states(L, nu, nd)
    H = restrict(dense(model, L, True), states).toarray().real
    basis, h = D.loadConfigFromDict(spinful_cfg(model, L, nu + nd, nu), hamiltonian=True)
    src = basis.payload.contents
    fb = _ForeignBasis()
    for f, _ in _lib.LsHsBasis._fields_:
        setattr(fb, f, getattr(src, f))
    fb.kernels = None
    fb.representatives = _lib.ChplExternalArray(None, 0, None)
    fo = _ForeignOperator()
    fo.basis = C.pointer(fb)
    fo.off_diag_terms = h.payload.contents.off_diag_terms
    fo.diag_terms = h.payload.contents.diag_terms
    bp = C.cast(C.pointer(fb), C.POINTER(_lib.LsHsBasis))
    op = C.cast(C.pointer(fo), C.POINTER(_lib.LsHsOperator))
    no_perm = (C.c_int * 1)(0)
    assert lib.ls_amd_adopt_basis(bp, 0, no_perm, no_perm) == 0, lib.ls_amd_last_error()
    assert lib.ls_amd_adopt_operator(op) == 0, lib.ls_amd_last_error()
    try:
        assert lib.ls_hs_basis_number_bits(bp) == 2 * L and not lib.ls_hs_basis_has_fixed_hamming_weight(bp)
        reps = np.ascontiguousarray(states)
        fb.representatives = _lib.ChplExternalArray(reps.ctypes.data, reps.size, None)
        x = np.random.RandomState(5).rand(len(states)) - 0.5
        y = np.full(len(states), 7.0)
        lib.ls_chpl_matrix_vector_product(op, 1, x.ctypes.data_as(_lib.c_f64p), y.ctypes.data_as(_lib.c_f64p))
        _lib.raise_pending_halt()
        want = H @ x
        assert np.abs(y - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    finally:
        fb.representatives = _lib.ChplExternalArray(None, 0, None)
        lib.ls_amd_release(C.cast(op, C.c_void_p))
        lib.ls_amd_release(C.cast(bp, C.c_void_p))
