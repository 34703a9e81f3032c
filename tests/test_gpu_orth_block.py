"""ls_amd_orth_block_pass and ls_amd_block_rotate (csrc/orth_block.hip), the block Gram-Schmidt sweep and the in-place rotation of
the block eigensolver, against plain PyTorch f64: every basis size class (none, one row, a partial 16-row tile, full tiles, the
limit), K from 1 to 16, odd lengths, lengths shorter than one tile, row strides larger than the length, unaligned starts, with and
without the update; the rotation with fewer output rows and with a triangular K x K matrix; and the solver-level property
(orthogonal to rounding after two sweeps)."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


@pytest.fixture(scope="module")
def lib():
    from distributed_matvec_amd import _lib

    return _lib.load()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _sweep(torch, lib, V, W, H):
    m, K, n = V.shape[0], W.shape[0], W.shape[1]
    out = torch.full((m * K + K * K,), 7.0, dtype=torch.float64, device="cuda")
    rc = lib.ls_amd_orth_block_pass(m, K, n, _ptr(V) if m else None, V.stride(0) if m else n, _ptr(W), W.stride(0), _ptr(H), _ptr(out), None)
    assert rc == 0, lib.ls_amd_last_error()
    torch.cuda.synchronize()
    return out[: m * K].reshape(m, K), out[m * K:].reshape(K, K)


def _rows(torch, g, rows, n, pad, shift):
    """`rows` rows of length n at row stride n + pad, starting `shift` elements into the allocation"""
    store = torch.randn(rows * (n + pad) + shift + 1, dtype=torch.float64, device="cuda", generator=g)
    return store[shift: shift + rows * (n + pad)].view(rows, n + pad)[:, :n]


CASES = [  # (m, K, n, pad, shift)
    (0, 1, 1000, 0, 0), (0, 16, 4097, 3, 1), (1, 1, 100001, 0, 0), (1, 2, 33, 0, 1), (7, 8, 12345, 5, 0), (7, 16, 10, 0, 0),
    (32, 2, 300007, 2, 0), (32, 16, 65536, 0, 0), (128, 1, 20001, 1, 1), (128, 8, 1 << 17, 0, 0), (128, 16, 40003, 0, 0),
    (17, 4, 5, 0, 0), (64, 8, 250, 6, 3), (7, 2, 1, 0, 0), (33, 16, 16, 0, 0),
]


@pytest.mark.parametrize("m,K,n,pad,shift", CASES)
def test_orth_block_pass_matches_torch(torch, lib, m, K, n, pad, shift):
    g = torch.Generator(device="cuda").manual_seed(1000 * m + 10 * K + pad)
    V = _rows(torch, g, m, n, pad, shift) if m else torch.empty((0, n), dtype=torch.float64, device="cuda")
    W0 = _rows(torch, g, K, n, pad + 1, shift)
    Wt = W0.clone()
    # sweep without update: overlaps and Gram matrix, W untouched
    W = _rows(torch, g, K, n, pad + 1, shift)
    W.copy_(W0)
    O, G = _sweep(torch, lib, V, W, None)
    assert torch.equal(W, Wt)
    want_o, want_g = V @ W0.t(), W0 @ W0.t()
    scale = float(want_g.abs().max())
    assert float((G - want_g).abs().max()) <= 1e-12 * scale
    if m == 0:
        return
    assert float((O - want_o).abs().max()) <= 1e-12 * scale
    # with update: W <- W - H^T V, then the overlaps and the Gram matrix of the updated W
    H = torch.randn((m, K), dtype=torch.float64, device="cuda", generator=g).contiguous()
    W.copy_(W0)
    O, G = _sweep(torch, lib, V, W, H)
    want_w = W0 - H.t() @ V
    assert float((W - want_w).abs().max()) <= 1e-12 * float(want_w.abs().max()) * max(1.0, m ** 0.5)
    want_o, want_g = V @ want_w.t(), want_w @ want_w.t()
    scale = float(want_g.abs().max())
    assert float((O - want_o).abs().max()) <= 1e-12 * scale * max(1.0, m ** 0.5)
    assert float((G - want_g).abs().max()) <= 1e-12 * scale * max(1.0, m ** 0.5)


def test_exact_integer_products_place_every_output(torch, lib):
    """small integers are exact in f64: a transposed or misplaced output of the matrix units shows as an exact mismatch"""
    m, K, n = 37, 11, 999
    g = torch.Generator(device="cuda").manual_seed(3)
    V = torch.randint(-3, 4, (m, n), device="cuda", generator=g).double()
    W = torch.randint(-3, 4, (K, n), device="cuda", generator=g).double()
    H = torch.randint(-2, 3, (m, K), device="cuda", generator=g).double()
    W0 = W.clone()
    O, G = _sweep(torch, lib, V, W, H)
    want_w = W0 - H.t() @ V
    assert torch.equal(W, want_w)
    assert torch.equal(O, V @ want_w.t()) and torch.equal(G, want_w @ want_w.t())
    S = torch.randint(-2, 3, (m, 13), device="cuda", generator=g).double().contiguous()
    Vr = V.clone()
    assert lib.ls_amd_block_rotate(m, 13, n, _ptr(Vr), Vr.stride(0), _ptr(S), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(Vr[:13], S.t() @ V) and torch.equal(Vr[13:], V[13:])


@pytest.mark.parametrize("m_in,m_out,n,pad,shift", [(1, 1, 1000, 0, 0), (12, 8, 100003, 2, 0), (64, 30, 65537, 0, 1),
                                                     (128, 128, 20000, 0, 0), (128, 7, 999, 3, 0), (16, 16, 15, 0, 0)])
def test_block_rotate_matches_torch(torch, lib, m_in, m_out, n, pad, shift):
    g = torch.Generator(device="cuda").manual_seed(m_in * 1000 + m_out)
    V = _rows(torch, g, m_in, n, pad, shift)
    V0 = V.clone()
    S = torch.randn((m_in, m_out), dtype=torch.float64, device="cuda", generator=g).contiguous()
    assert lib.ls_amd_block_rotate(m_in, m_out, n, _ptr(V), V.stride(0), _ptr(S), None) == 0
    torch.cuda.synchronize()
    want = S.t() @ V0
    assert float((V[:m_out] - want).abs().max()) <= 1e-12 * float(want.abs().max()) * max(1.0, m_in ** 0.5)
    assert torch.equal(V[m_out:], V0[m_out:])  # rows past m_out are left as they are


def test_block_rotate_triangular_normalisation(torch, lib):
    """the Cholesky-QR step of the solver: W <- W R^-1 with R^T R = Gram(W) gives orthonormal rows"""
    import numpy as np

    K, n = 8, 300001
    g = torch.Generator(device="cuda").manual_seed(11)
    W = torch.randn((K, n), dtype=torch.float64, device="cuda", generator=g)
    W[3] += 5 * W[1]  # not orthogonal to start with
    _, G = _sweep(torch, lib, torch.empty((0, n), dtype=torch.float64, device="cuda"), W, None)
    R = np.linalg.cholesky(G.cpu().numpy()).T  # upper, R^T R = G
    Rinv = torch.as_tensor(np.linalg.inv(R), device="cuda").contiguous()
    assert float(Rinv.tril(-1).abs().max()) == 0.0
    W0 = W.clone()
    assert lib.ls_amd_block_rotate(K, K, n, _ptr(W), W.stride(0), _ptr(Rinv), None) == 0
    torch.cuda.synchronize()
    assert float((W - Rinv.t() @ W0).abs().max()) <= 1e-12 * float(W.abs().max()) * 10
    assert float((W @ W.t() - torch.eye(K, dtype=torch.float64, device="cuda")).abs().max()) <= 1e-12


def test_two_sweeps_orthogonalise_to_rounding(torch, lib):
    """what lanczos_block_smallest relies on: against an orthonormal basis, sweep 1 + sweep 2 leave ||V^T W|| at rounding level,
    and the second sweep reports what is left and the Gram matrix of the result"""
    m, K, n = 48, 8, 1 << 18
    g = torch.Generator(device="cuda").manual_seed(5)
    Q, _ = torch.linalg.qr(torch.randn((n, m), dtype=torch.float64, device="cuda", generator=g))
    V = Q.t().contiguous()
    W = torch.randn((K, n), dtype=torch.float64, device="cuda", generator=g) + 50.0 * V[3:3 + K]
    O1, _ = _sweep(torch, lib, V, W, None)
    O2, G = _sweep(torch, lib, V, W, O1.contiguous())
    norms = torch.sqrt(torch.diagonal(G))
    assert float(O2.abs().max()) <= 1e-12 * float(norms.min()) * 60
    assert float((G - W @ W.t()).abs().max()) <= 1e-12 * float(G.abs().max())
    assert float((V @ W.t()).abs().max()) <= 1e-12 * float(norms.min()) * 60
