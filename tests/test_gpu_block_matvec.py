"""Block matvec on the GPU (MatvecPlan.matvec_block, ls_amd_matvec_block): Y = H X for K columns at once.  The block result equals
K single-vector matvecs on every path (k_direct_blk, resolve + k_pull_gather_blk, the column loop), in every layout, and one case
per path equals an independent reference (the C oracle for spins, the dense Jordan-Wigner matrix for fermions).  Y is assigned,
X is left alone, the plan's single-vector state does not change, and argument errors are refused before anything runs."""
import numpy as np
import pytest

import distributed_matvec_amd as D
from distributed_matvec_amd import config
from fermion_jw import dense, hubbard_model, product_states, restrict, ring, weight_states, yaml_terms
from helpers import complex_translation_config, model_config

pytestmark = pytest.mark.gpu

KS = [1, 3, 8, 13, 64]
LAYOUTS = ["interleaved", "colmajor", "colmajor_ld"]


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def hop_chain_config(L):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    return {"basis": {"number_spins": L, "hamming_weight": L // 2, "symmetries": []},
            "hamiltonian": {"terms": [{"expression": "σ⁺₀ σ⁻₁", "sites": bonds}, {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]}}


def hubbard_nonseparable():
    L = 6
    model = hubbard_model(L, ring(L), U=2.0) + [(0.5, [("+", 0, 0), ("+", 0, 1), ("-", 3, 1), ("-", 3, 0)]),
                                                (0.5, [("+", 3, 0), ("+", 3, 1), ("-", 0, 1), ("-", 0, 0)])]
    cfg = {"basis": {"particle": "spinful-fermion", "number_sites": L, "number_particles": 6, "number_up": 3},
           "hamiltonian": {"terms": yaml_terms(model, True)}}
    states = product_states(L, 3, 3)
    return cfg, restrict(dense(model, L, True), states).toarray(), states


def spinless_ring(L, N):
    model = []
    for i, j in ring(L):
        model += [(-1.0, [("+", i, 0), ("-", j, 0)]), (-1.0, [("+", j, 0), ("-", i, 0)]), (0.7, [("n", i, 0), ("n", j, 0)])]
    cfg = {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": N}, "hamiltonian": {"terms": yaml_terms(model, False)}}
    states = weight_states(L, N)
    return cfg, restrict(dense(model, L, False), states).toarray(), states


# name -> (config, dtype, the block path `auto` takes for K >= 2)
def model_table():
    return {
        "heisenberg_chain_10/f64": (lambda: model_config("heisenberg_chain_10"), "f64", "columns"),  # (a spin-inversion sector)
        "heisenberg_chain_16/c128": (lambda: model_config("heisenberg_chain_16"), "c128", "columns"),
        "heisenberg_chain_24_symm/f64": (lambda: model_config("heisenberg_chain_24_symm"), "f64", "k_pull_gather_blk"),
        "heisenberg_kagome_12_symm/f64": (lambda: model_config("heisenberg_kagome_12_symm"), "f64", "k_pull_gather_blk"),
        "heisenberg_kagome_12_symm/c128": (lambda: model_config("heisenberg_kagome_12_symm"), "c128", "k_pull_gather_blk"),
        "heisenberg_square_4x4/f64": (lambda: model_config("heisenberg_square_4x4"), "f64", "k_pull_gather_blk"),
        "momentum_12_5/c128": (lambda: complex_translation_config(12, 5), "c128", "k_pull_gather_blk"),
        "hop_chain_12/f64": (lambda: hop_chain_config(12), "f64", "k_direct_blk"),
        "hop_chain_12/c128": (lambda: hop_chain_config(12), "c128", "k_direct_blk"),
        "hubbard_pair_hop_6/c128": (lambda: hubbard_nonseparable()[0], "c128", "k_direct_blk"),
        "spinless_ring_9_4/f64": (lambda: spinless_ring(9, 4)[0], "f64", "k_direct_blk"),
        "spinless_ring_8_all/f64": (lambda: spinless_ring(8, -1)[0], "f64", "k_direct_blk"),
        "chain_12_inversion/f64": (lambda: config.heisenberg_chain_config(12, spin_inversion=-1), "f64", "columns"),
    }


_plans = {}


def plan_of(torch, name):
    if name not in _plans:
        make, dt, _ = model_table()[name]
        basis, h = D.loadConfigFromDict(make(), hamiltonian=True)
        reps, _ = D.enumerateStates(basis, 1)
        dtype = torch.complex128 if dt == "c128" else torch.float64
        _plans[name] = (D.MatvecPlan(h, reps, dtype), reps, dtype, h)
    return _plans[name]


def random_block(torch, n, K, dtype, seed):
    rs = np.random.RandomState(seed)
    X = rs.rand(n, K) - 0.5
    if dtype == torch.complex128:
        X = X + 1j * (rs.rand(n, K) - 0.5)
    return X


def device_block(torch, X, layout, dtype, fill=None):
    """(N, K) device tensor holding X (or `fill` everywhere) in the given layout"""
    n, K = X.shape
    src = torch.from_numpy(np.ascontiguousarray(X)).to(dtype)
    if layout == "interleaved":
        t = torch.empty((n, K), dtype=dtype, device="cuda")
    elif layout == "colmajor":
        t = torch.empty((K, n), dtype=dtype, device="cuda").t()
    else:
        t = torch.empty((K, n + 5), dtype=dtype, device="cuda")[:, :n].t()
    if fill is None:
        t.copy_(src.cuda())
    else:
        t.fill_(fill)
    return t


def columns_reference(torch, pl, X, dtype):
    cols = []
    for k in range(X.shape[1]):
        xk = torch.from_numpy(np.ascontiguousarray(X[:, k])).to(dtype).cuda()
        yk = torch.zeros_like(xk)
        pl.matvec([xk], [yk])
        cols.append(yk.cpu().numpy())
    return np.stack(cols, axis=1)


def assert_block_close(got, want, what):
    err = np.abs(got - want).max()
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), (what, err)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", sorted(model_table()))
def test_block_equals_single_vector_matvecs(torch, monkeypatch, name, K, layout):
    pl, reps, dtype, _ = plan_of(torch, name)
    n = reps[0].numel()
    X = random_block(torch, n, K, dtype, 7 + K)
    want = columns_reference(torch, pl, X, dtype)
    for mode in ("auto", "kernel", "columns"):
        monkeypatch.setenv("LS_AMD_BLOCK", mode)
        x = device_block(torch, X, layout, dtype)
        x0 = x.clone()
        y = device_block(torch, X, layout, dtype, fill=float("nan"))
        pl.matvec_block(x, y)
        got = y.cpu().numpy()
        assert np.isfinite(got).all(), (name, mode)  # Y is assigned
        assert torch.equal(x, x0)  # X is left alone
        assert_block_close(got, want, (name, K, layout, mode, pl.block_kernel(K)))


def test_block_kernel_choice(torch, monkeypatch):
    for name, (_, _, want) in model_table().items():
        pl = plan_of(torch, name)[0]
        monkeypatch.delenv("LS_AMD_BLOCK", raising=False)
        assert pl.block_kernel(8) == want, (name, pl.kernel)
        assert pl.block_kernel(1) == "columns", name
        monkeypatch.setenv("LS_AMD_BLOCK", "columns")
        assert pl.block_kernel(8) == "columns"
        monkeypatch.setenv("LS_AMD_BLOCK", "kernel")
        forced = pl.block_kernel(8)
        if want != "columns":
            assert forced == want and pl.block_kernel(1) == want, name
    # the staged chain kernel keeps the column loop under auto; `kernel` forces k_direct_blk
    pl = plan_of(torch, "heisenberg_chain_16/c128")[0]
    assert pl.kernel == "direct-pull+staged"
    assert pl.block_kernel(8) == "k_direct_blk"
    # inversion sectors (heisenberg_chain_10 is one) have no block kernel
    for name in ("chain_12_inversion/f64", "heisenberg_chain_10/f64"):
        assert plan_of(torch, name)[0].block_kernel(8) == "columns", name


def test_block_matches_independent_reference(torch, monkeypatch):
    from oracle import c_oracle as CO
    from oracle import model as M

    monkeypatch.setenv("LS_AMD_BLOCK", "kernel")
    K = 5
    # spins: the C oracle, one model per path
    for name in ("heisenberg_chain_24_symm/f64", "momentum_12_5/c128", "hop_chain_12/f64", "chain_12_inversion/f64",
                 "heisenberg_chain_16/c128"):
        make, _, _ = model_table()[name]
        pl, reps, dtype, _ = plan_of(torch, name)
        o = CO.COracle(M.model_from_config(make()))
        want_reps = o.enumerate()
        assert np.array_equal(reps[0].cpu().numpy().view(np.uint64), want_reps)
        X = random_block(torch, len(want_reps), K, dtype, 3)
        want = np.stack([o.local_matvec(want_reps, X[:, k]) for k in range(K)], axis=1)
        x = device_block(torch, X, "interleaved", dtype)
        y = torch.empty_like(x)
        pl.matvec_block(x, y)
        assert_block_close(y.cpu().numpy(), want, name)
    # fermions: the dense Jordan-Wigner matrices
    for name, (cfg_H_states) in (("hubbard_pair_hop_6/c128", hubbard_nonseparable()), ("spinless_ring_9_4/f64", spinless_ring(9, 4))):
        _, H, states = cfg_H_states
        pl, reps, dtype, _ = plan_of(torch, name)
        assert np.array_equal(reps[0].cpu().numpy().view(np.uint64), states)
        X = random_block(torch, len(states), K, dtype, 4)
        x = device_block(torch, X, "colmajor", dtype)
        y = device_block(torch, X, "colmajor", dtype, fill=float("nan"))
        pl.matvec_block(x, y)
        assert_block_close(y.cpu().numpy(), H @ X, name)


@pytest.mark.parametrize("name", ["heisenberg_chain_24_symm/f64", "heisenberg_kagome_12_symm/c128", "hop_chain_12/f64"])
def test_no_state_leak(torch, name):
    make, dt, _ = model_table()[name]
    basis, h = D.loadConfigFromDict(make(), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    dtype = torch.complex128 if dt == "c128" else torch.float64
    n = reps[0].numel()
    X = random_block(torch, n, 8, dtype, 5)
    xb = torch.from_numpy(X).to(dtype).cuda()
    x1 = xb[:, 2].contiguous()

    def single(pl):
        y = torch.zeros_like(x1)
        pl.matvec([x1], [y])
        return y

    results = []
    for cached in (False, True):
        pl = D.MatvecPlan(h, reps, dtype)
        if cached:
            rows = pl.cache_slots()
            assert rows == (n if name != "hop_chain_12/f64" else 0)
        before = single(pl)
        kernel, cache = pl.kernel, pl.slot_cache
        y = torch.empty_like(xb)
        pl.matvec_block(xb, y)
        results.append(y.cpu().numpy())
        after = single(pl)
        assert torch.equal(before, after), (name, cached)
        assert pl.kernel == kernel and pl.slot_cache == cache
    assert_block_close(results[1], results[0], name)


def test_errors_are_refused(torch):
    pl, reps, dtype, h = plan_of(torch, "heisenberg_chain_24_symm/f64")
    n = reps[0].numel()
    x = torch.zeros((n, 65), dtype=dtype, device="cuda")
    with pytest.raises(D.LsAmdError, match=r"K = 65"):
        pl.matvec_block(x, torch.zeros_like(x))
    x = torch.zeros((n, 4), dtype=dtype, device="cuda")
    with pytest.raises(D.LsAmdError, match="computes in"):
        pl.matvec_block(x.to(torch.complex128), torch.zeros_like(x).to(torch.complex128))
    with pytest.raises(D.LsAmdError, match="2-D"):
        pl.matvec_block(x[:, 0], x[:, 1])
    with pytest.raises(D.LsAmdError, match="overlap"):
        pl.matvec_block(x, x)
    big = torch.zeros((n, 8), dtype=dtype, device="cuda")
    with pytest.raises(D.LsAmdError, match="overlap"):
        pl.matvec_block(big[:, :4], big[:, 4:])  # interleaved rows of one buffer: the ranges overlap
    # two partitions: refused by the block entry
    basis, h2 = D.loadConfigFromDict(model_config("heisenberg_chain_16"), hamiltonian=True)
    reps2, _ = D.enumerateStates(basis, 2)
    pl2 = D.MatvecPlan(h2, reps2, torch.float64)
    x2 = torch.zeros((reps2[0].numel(), 2), dtype=torch.float64, device="cuda")
    with pytest.raises(D.LsAmdError, match="one-partition"):
        pl2.matvec_block(x2, torch.zeros_like(x2))
    # ... and by the C entry itself, whatever the wrapper checks
    from distributed_matvec_amd import _lib
    import ctypes as C

    y2 = torch.zeros_like(x2)
    assert _lib.load().ls_amd_matvec_block(pl2.h, 2, C.c_void_p(x2.data_ptr()), 2, 1, C.c_void_p(y2.data_ptr()), 2, 1, None) == -1
    assert "one-partition" in _lib.load().ls_amd_last_error().decode()
    # strides that put two elements on one: refused by the C entry
    y = torch.zeros((n, 4), dtype=dtype, device="cuda")
    rc = _lib.load().ls_amd_matvec_block(pl.h, 4, C.c_void_p(x.data_ptr()), 1, 1, C.c_void_p(y.data_ptr()), 4, 1, None)
    assert rc == -1 and "share" in _lib.load().ls_amd_last_error().decode()
    # a non-Hermitian operator that maps the basis out of itself is still refused when the plan is made
    cfg = config.heisenberg_chain_config(8)
    cfg["hamiltonian"]["terms"].append({"expression": "σ⁺₀", "sites": [[3]]})
    basis3, h3 = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps3, _ = D.enumerateStates(basis3, 1)
    with pytest.raises(D.LsAmdError, match="invalid index"):
        pl3 = D.MatvecPlan(h3, reps3, torch.float64)
        x3 = torch.ones((reps3[0].numel(), 2), dtype=torch.float64, device="cuda")
        pl3.matvec_block(x3, torch.zeros_like(x3))


def _sampled_rows_check(torch, pl, reps, K, seed):
    n = reps[0].numel()
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((n, K), dtype=torch.float64, device="cuda", generator=g) - 0.5
    y = torch.empty_like(x)
    pl.matvec_block(x, y)
    rows = torch.from_numpy(np.random.RandomState(seed).choice(n, 4000, replace=False)).cuda()
    got = y[rows].cpu().numpy()
    del y
    want = np.empty_like(got)
    for k in range(K):
        xk = x[:, k].contiguous()
        yk = torch.zeros_like(xk)
        pl.matvec([xk], [yk])
        want[:, k] = yk[rows].cpu().numpy()
    assert_block_close(got, want, (pl.kernel, K))


def test_larger_cases(torch, monkeypatch):
    """multi-tile persistent grids (chain_28, k_direct_blk forced) and the chunked resolve of chain_36_symm under a small packet
    buffer (LS_AMD_BLOCK_RESOLVE_BYTES = 64 MiB: many chunks)"""
    monkeypatch.setenv("LS_AMD_BLOCK", "kernel")
    basis, h = D.loadConfigFromDict(model_config("heisenberg_chain_28"), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    pl = D.MatvecPlan(h, reps, torch.float64)
    assert pl.block_kernel(8) == "k_direct_blk"
    _sampled_rows_check(torch, pl, reps, 8, 1)
    del pl, reps, basis, h
    torch.cuda.empty_cache()
    monkeypatch.setenv("LS_AMD_BLOCK_RESOLVE_BYTES", str(64 << 20))
    basis, h = D.loadConfigFromDict(model_config("heisenberg_chain_36_symm"), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    pl = D.MatvecPlan(h, reps, torch.float64)
    assert pl.block_kernel(4) == "k_pull_gather_blk"
    _sampled_rows_check(torch, pl, reps, 4, 2)
