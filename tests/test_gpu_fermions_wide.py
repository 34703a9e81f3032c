"""Fermionic bases wider than 32 modes, or whose down half crosses bit 32, on the GPU: enumeration bit-exact against itertools and
y against the sector Jordan-Wigner reference (fermion_jw.sector_matrix), on every kernel such a basis reaches -- k_chain_t and
k_direct on 64-bit words (both REAL instantiations), k_direct with the product index, all three k_hubbard instantiations,
push, hash partitions, k_direct_blk.  Every plan names the kernel it must take, so a silent re-route fails."""
import numpy as np
import pytest

import distributed_matvec_amd as D
from fermion_jw import sector_matrix
from fermion_wide import CASES

pytestmark = pytest.mark.gpu

# name -> the kernel each plan reports: pull and push at P = 1, `auto` at P = 3.  What each case is there for:
#   spinless_open_33_3          k_chain_t on 64-bit words (one exchange run, no strings); the only P = 3 case on sorted streams
#   spinless_long_40_3[_complex] k_direct<uint64_t> with strings across bit 32 (REAL = true; the complex hop 31-32: REAL = false)
#   spinless_ring_64_2          the closing bond's 62-mode string, bit 63; no diagonal: y is accumulated into
#   spinless_ring_36_33         weight 33, the last row of the binomial table (LSK_BINOM_K = 34)
#   spinless_ring_48_{1,0}      one particle; the one-row sector
#   hubbard_ring_17_2_2[_free|_peierls]  k_hubbard<false, false>, <true, false> (f64, c128), <true, true>: the down half crosses
#                               bit 32 (row state (uint64_t)dn << 17, species tables with hmask at bits 17..33); _free has no diagonal
#   hubbard_32_{1_2,2_1}        k_hubbard with bit 63 reachable, V and a Peierls phase
#   hubbard_32_1_2_pair_hop     non-separable: k_direct with the product index (prod_sites = 32), push with atomics
#   hubbard_32_{0_2,2_0}, hubbard_20_20_1  an empty species (n_b = 1) and a full one (no partner in that half)
#   spinful_{16,17}_n3_flips    N alone fixed: 32-bit and 64-bit words either side of the switch in launch_direct1
# Push on the single-word bases takes the staged push; every case under LS_AMD_ROW_KERNEL=generic is plain k_direct.
_SINGLE_WORD = {"pull": "direct-pull", "push": "direct-push+staged", "auto3": "tile"}
_HUBBARD = {"pull": "direct-pull+hubbard", "push": "direct-push", "auto3": "tile"}
KERNELS = {
    "spinless_open_33_3": {"pull": "direct-pull+staged", "push": "direct-push+staged", "auto3": "tile+streams"},
    "spinless_long_40_3": _SINGLE_WORD,
    "spinless_long_40_3_complex": {"pull": "direct-pull", "push": "direct-push", "auto3": "tile"},
    "spinless_ring_64_2": _SINGLE_WORD,
    "spinless_ring_36_33": _SINGLE_WORD,
    "spinless_ring_48_1": _SINGLE_WORD,
    "spinless_ring_48_0": _SINGLE_WORD,
    "hubbard_ring_17_2_2": _HUBBARD,
    "hubbard_ring_17_2_2_free": _HUBBARD,
    "hubbard_ring_17_2_2_peierls": _HUBBARD,
    "hubbard_32_1_2": _HUBBARD,
    "hubbard_32_2_1": _HUBBARD,
    "hubbard_32_1_2_pair_hop": {"pull": "direct-pull", "push": "direct-push", "auto3": "tile"},
    "hubbard_32_0_2": _HUBBARD,
    "hubbard_32_2_0": _HUBBARD,
    "hubbard_20_20_1": _HUBBARD,
    "spinful_16_n3_flips": _SINGLE_WORD,
    "spinful_17_n3_flips": _SINGLE_WORD,
}


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


_refs = {}


def reference(name):
    if name not in _refs:
        case = CASES[name]
        states = case.states()
        _refs[name] = (states, sector_matrix(list(case.model), case.L, case.spinful, states))
    return _refs[name]


def vectors(n, real):
    rs = np.random.RandomState(11)
    x = rs.rand(n) - 0.5
    xc = x + 1j * (rs.rand(n) - 0.5)
    return (x, xc) if real else (xc,)


def assert_close(got, want, what):
    err = np.abs(got - want).max()
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), (what, err)


def apply(torch, h, reps, masks, P, x, y0, mode):
    """y (block order) after matrixVectorProduct from y0, and the plan's kernel"""
    xs = D.arrFromBlockToHashed(torch.from_numpy(np.ascontiguousarray(x)).cuda(), masks, P)
    ys = D.arrFromBlockToHashed(torch.from_numpy(np.ascontiguousarray(y0)).cuda(), masks, P)
    pl = D.matrixVectorProduct(h, xs, ys, reps, mode=mode)
    return D.arrFromHashedToBlock(ys, masks).cpu().numpy(), pl.kernel


@pytest.mark.parametrize("name", sorted(CASES))
def test_wide_matvec_equals_sector_reference(torch, monkeypatch, name):
    """pull and push at P = 1, `auto` over three hash partitions; y is assigned when the operator has a diagonal (y starts as
    garbage) and accumulated into when it has none (y starts as a random vector)"""
    monkeypatch.delenv("LS_AMD_ROW_KERNEL", raising=False)
    case = CASES[name]
    states, H = reference(name)
    for P, modes in ((1, ("pull", "push")), (3, ("auto",))):
        basis, h = D.loadConfigFromDict(case.config(), hamiltonian=True)
        reps, masks = D.enumerateStates(basis, P)
        assert np.array_equal(D.arrFromHashedToBlock(reps, masks).cpu().numpy().view(np.uint64), states), (name, P)
        assert h.isReal == case.is_real
        diagonal = h.numberDiagTerms() > 0
        for x in vectors(len(states), case.is_real):
            y0 = np.full(len(states), 123.0, dtype=x.dtype) if diagonal else np.cos(np.arange(len(states)) * 0.77).astype(x.dtype)
            want = H @ x + (0 if diagonal else y0)
            for mode in modes:
                got, kernel = apply(torch, h, reps, masks, P, x, y0, mode)
                assert kernel == KERNELS[name][mode if P == 1 else "auto3"], (name, P, mode, kernel)
                assert_close(got, want, (name, P, mode, x.dtype, kernel))


@pytest.mark.parametrize("name", sorted(CASES))
def test_wide_generic_row_kernel(torch, monkeypatch, name):
    """LS_AMD_ROW_KERNEL=generic: the staged chain, staged push and species kernels give way to k_direct on the same basis"""
    monkeypatch.setenv("LS_AMD_ROW_KERNEL", "generic")
    case = CASES[name]
    states, H = reference(name)
    basis, h = D.loadConfigFromDict(case.config(), hamiltonian=True)
    reps, masks = D.enumerateStates(basis, 1)
    diagonal = h.numberDiagTerms() > 0
    for x in vectors(len(states), case.is_real):
        y0 = np.full(len(states), 123.0, dtype=x.dtype) if diagonal else np.ones(len(states), dtype=x.dtype)
        for mode in ("pull", "push"):
            got, kernel = apply(torch, h, reps, masks, 1, x, y0, mode)
            assert kernel == "direct-" + mode, (name, mode, kernel)
            assert_close(got, H @ x + (0 if diagonal else y0), (name, mode, x.dtype))


@pytest.mark.parametrize("name,dt", [("spinless_long_40_3", "f64"), ("spinless_long_40_3_complex", "c128"),
                                     ("hubbard_ring_17_2_2", "f64"), ("hubbard_32_1_2", "c128"),
                                     ("hubbard_32_1_2_pair_hop", "c128")])
def test_wide_block_matvec(torch, monkeypatch, name, dt):
    """K = 5 columns in both layouts through k_direct_blk and the column loop; Y starts as NaN because the block call assigns"""
    monkeypatch.delenv("LS_AMD_ROW_KERNEL", raising=False)
    case = CASES[name]
    states, H = reference(name)
    dtype = torch.complex128 if dt == "c128" else torch.float64
    basis, h = D.loadConfigFromDict(case.config(), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    pl = D.MatvecPlan(h, reps, dtype)
    assert pl.kernel == KERNELS[name]["pull"], pl.kernel
    K, n = 5, len(states)
    rs = np.random.RandomState(5)
    X = rs.rand(n, K) - 0.5
    if dt == "c128":
        X = X + 1j * (rs.rand(n, K) - 0.5)
    want = H @ X
    for block in ("kernel", "columns"):
        monkeypatch.setenv("LS_AMD_BLOCK", block)
        assert pl.block_kernel(K) == ("k_direct_blk" if block == "kernel" else "columns"), (name, block)
        for layout in ("interleaved", "colmajor"):
            if layout == "interleaved":
                x, y = (torch.empty((n, K), dtype=dtype, device="cuda") for _ in range(2))
            else:
                x, y = (torch.empty((K, n), dtype=dtype, device="cuda").t() for _ in range(2))
            x.copy_(torch.from_numpy(X).to(dtype).cuda())
            y.fill_(float("nan"))
            pl.matvec_block(x, y)
            got = y.cpu().numpy()
            assert np.isfinite(got).all(), (name, block, layout)
            assert_close(got, want, (name, block, layout))
