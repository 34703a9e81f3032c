"""Wave headers of the staged row kernel (k_chain_t on fused records): a wave-row whose 64 rows share their bits >= 12 reads an
8-byte header and a word table instead of 64 8-byte records.  Every shape is run three times -- default plan, the same plan under
LS_AMD_CHAIN_RECORDS=1 (records everywhere) and the generic row kernel (k_direct, which shares no code with either) -- in f64
(fused records) and c128 (4-byte state + 4-byte cache entry per row; the same headers)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def _config(L, weight, kind, jz=1.0):
    from distributed_matvec_amd import config

    cfg = config.heisenberg_chain_config(L)
    cfg["basis"]["hamming_weight"] = weight
    lattice = [[i, i + 1] for i in range(L - 1)] if kind == "open" else [[i, (i + 1) % L] for i in range(L)]
    for t in cfg["hamiltonian"]["terms"]:
        t["sites"] = lattice
        if jz != 1.0 and "σᶻ" in t["expression"]:
            t["expression"] = f"{jz} × " + t["expression"]
    return cfg


# name: (sites, weight, ring / open, Jz, wave headers in use, headers save bytes)
SHAPES = {
    "ring13-w6": (13, 6, "ring", 1.0, True, True),       # the high part is one bit, the ring bond's own
    "ring14-w7": (14, 7, "ring", 1.0, True, True),
    "ring16-w8": (16, 8, "ring", 1.0, True, True),       # 12 870 rows: several blocks, a partial last tile
    "ring20-w10": (20, 10, "ring", 1.0, True, True),     # 184 756 rows, many tiles
    "ring20-w3": (20, 3, "ring", 1.0, True, False),      # blocks of a handful of rows: nearly every wave-row on its records
    "ring20-w17": (20, 17, "ring", 1.0, True, False),
    "ring24-w12": (24, 12, "ring", 1.0, True, True),     # headed wave-rows dominate, as on chain_32
    "open20-w10": (20, 10, "open", 1.0, True, True),     # no cached pair
    "ring12-w6": (12, 6, "ring", 1.0, False, False),     # < 13 sites: records only
    "xxz16-w8": (16, 8, "ring", 0.35, True, True),       # Jz != J: another diagonal
}


def _matvec(torch, cfg, x):
    import distributed_matvec_amd as D

    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, masks = D.enumerateStates(basis, 1)
    xs = D.arrFromBlockToHashed(torch.from_numpy(np.ascontiguousarray(x)).cuda(), masks, 1)
    ys = [torch.zeros_like(v) for v in xs]
    pl = D.matrixVectorProduct(h, xs, ys, reps, mode="pull")
    y = D.arrFromHashedToBlock(ys, masks).cpu().numpy()
    return y, pl.kernel, pl.row_bytes, reps[0].cpu().numpy().view(np.uint64)


def _header_row_bytes(states, rec):
    """ceil((8 wave-rows + 64 rec wave-rows without a header) / rows), rec = bytes of a row's records (f64: 8, i.e. 512 per
    wave-row): a wave-row has a header when it is full and its rows share every bit >= 12"""
    n = len(states)
    n_wave = -(-n // 64)
    full = n // 64
    first, last = states[0:64 * full:64], states[63:64 * full:64]
    headed = int(np.count_nonzero(((first ^ last) >> np.uint64(12)) == 0))
    return -(-(8 * n_wave + 64 * rec * (n_wave - headed)) // n), headed, n_wave


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_headers_match_records_and_generic_kernel(torch, monkeypatch, shape, dtype):
    L, weight, kind, jz, uses_headers, saves = SHAPES[shape]
    for k in ("LS_AMD_CHAIN_RECORDS", "LS_AMD_ROW_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    cfg = _config(L, weight, kind, jz)
    from math import comb

    n = comb(L, weight)
    rs = np.random.RandomState(1000 * L + weight)
    x = rs.rand(n) - 0.5
    if dtype == "c128":
        x = x + 1j * (rs.rand(n) - 0.5)
    y, kernel, row_bytes, states = _matvec(torch, cfg, x)
    assert len(states) == n
    assert kernel == "direct-pull+staged", kernel

    monkeypatch.setenv("LS_AMD_CHAIN_RECORDS", "1")
    y_rec, kernel_rec, row_bytes_rec, _ = _matvec(torch, cfg, x)
    monkeypatch.delenv("LS_AMD_CHAIN_RECORDS")
    assert kernel_rec == "direct-pull+staged", kernel_rec
    assert y.tobytes() == y_rec.tobytes(), (shape, dtype, np.abs(y - y_rec).max())

    monkeypatch.setenv("LS_AMD_ROW_KERNEL", "generic")
    y_gen, kernel_gen, _, _ = _matvec(torch, cfg, x)
    monkeypatch.delenv("LS_AMD_ROW_KERNEL")
    assert kernel_gen == "direct-pull", kernel_gen
    err = np.abs(y - y_gen).max()
    print(f"{shape} {dtype}: max|y - y_generic| = {err:.3e}, max|y| = {np.abs(y_gen).max():.3e}, row_bytes {row_bytes} / {row_bytes_rec}")
    assert err <= 1e-12 * np.abs(y_gen).max(), (shape, dtype, err)

    # per-row records: f64 the fused 8 bytes, c128 the low state word + one cached partner rank per cached pair
    rec = 8 if dtype == "f64" else 4 + 4 * (0 if kind == "open" else 1)
    assert row_bytes_rec == rec
    if not uses_headers:
        assert row_bytes == rec
        return
    want, headed, n_wave = _header_row_bytes(states, rec)
    assert row_bytes == want, (row_bytes, want, headed, n_wave)
    if saves:
        assert row_bytes < rec and row_bytes <= 2 and headed > n_wave // 2, (row_bytes, headed, n_wave)
    else:  # nearly every wave-row runs on its records (3 resp. 2 of 18 have a header): f64 7 resp. 8 bytes per row by the formula
        assert rec - 1 <= row_bytes <= rec and headed <= n_wave // 4, (row_bytes, headed, n_wave)
