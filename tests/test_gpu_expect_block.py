"""Block expectation values on the GPU (ExpectationPlan.values_block / k_expect_blk, k_expect_blk_fermi; expectation_values_block)
against the references tests/test_gpu_expectation.py owns -- the CPU expansion of every column followed by numpy bit arithmetic with
the raw terms -- and against ExpectationPlan.values column by column (the single-state kernel, untouched by the block form): the
chunks of 8 columns and their tails, the layouts, the launches of a batch with more than 4096 unique terms, the promotion of float64,
bitwise reproducibility, the column loop behind LS_AMD_EXPECT_BLOCK, the error flag and the refusals.

Tolerance: that of tests/test_gpu_expectation.py, per operator and per column: ATOL_k = 2e-11 max(1, sum_t |v_t|) for a normalised
column (a column of another norm scales it by |psi_c|^2: every summand is bilinear in the column).  The block kernel forms the same
products as k_expect and adds them in another order, so the derivation there holds word for word."""
import ctypes as C
import functools

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
from distributed_matvec_amd import config, expectation_values_block  # noqa: F401  (the feature under test)
from distributed_matvec_amd._lib import LsAmdError
from test_gpu_expectation import CASES, _atol, _coef, _setup, _u64, raw_expectation

pytestmark = pytest.mark.gpu
BIG = "ring16_k3_c128_more_than_4096_terms"


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    assert hasattr(D.ExpectationPlan, "values_block") and hasattr(D.ExpectationPlan, "block_kernel")
    return t


def _columns(torch, reps, dtype, seeds, normalise=True):
    cols = [D.fillRandom(reps, s, dtype) for s in seeds]
    if normalise:
        cols = [c / torch.linalg.vector_norm(c) for c in cols]
    return torch.stack(cols, dim=1).contiguous()


def _family(name, basis):
    fermi = not isinstance(CASES[name][0](), dict) and basis.hasFermionSigns()
    return "k_expect_blk_fermi" if fermi else "k_expect_blk"


@functools.lru_cache(maxsize=None)
def _case(name):
    """(basis, reps, block of 3 normalised columns, specs, sections, dense values (3, n_ops)): computed once per case, read-only"""
    import torch

    basis, reps, psi, states, _vec, sections = _setup(torch, name)
    what = CASES[name][0]()
    specs = [config.parse_operator(sec, basis.spec) for sec in sections]
    keep = [k for k, s in enumerate(specs) if s.terms]  # (a monomial that vanishes identically has no terms)
    block = _columns(torch, reps, psi.dtype, (11, 12, 13))
    want = []
    for c in range(3):
        col = block[:, c].cpu().numpy()
        vec = E.expand_full(what, col) if isinstance(what, dict) else what.full_vector(col)
        assert abs(np.vdot(vec, vec).real - 1.0) < 1e-12
        want.append([raw_expectation(states, vec, specs[k].terms) for k in keep])
    return basis, reps, block, [specs[k] for k in keep], [sections[k] for k in keep], np.array(want)


@pytest.mark.parametrize("blocks", [None, 2])
@pytest.mark.parametrize("name", sorted(n for n in CASES if n != BIG))
def test_every_column_matches_the_expansion(torch, name, blocks, monkeypatch):
    """K = 3 columns of every case against the dense reference, with the default grid and with LS_AMD_CORR_BLOCKS=2 (the 16-site rings
    have 800 rows, four tiles: a block accumulates its partial sums across two)"""
    if blocks:
        monkeypatch.setenv("LS_AMD_CORR_BLOCKS", str(blocks))
    basis, reps, block, specs, sections, want = _case(name)
    assert len(specs) >= 10
    pl = D.ExpectationPlan(basis, reps, specs)
    assert pl.block_kernel(3) == _family(name, basis)
    if name == "ring16_k3_c128":
        assert pl.num_groups > 8 and int(reps.numel()) == 800
    got = pl.values_block(block)
    assert got.shape == (len(specs), 3) and got.dtype == np.complex128 and np.isfinite(got).all()
    worst = 0.0
    for k, spec in enumerate(specs):
        tol = _atol(spec.terms)
        for c in range(3):
            err = abs(got[k, c] - want[c, k])
            worst = max(worst, err / tol)
            assert err <= tol, (name, blocks, sections[k], c, got[k, c], want[c, k], err, tol)
    print(f"values_block {name} (blocks {blocks}): {len(specs)} operators x 3 columns, {pl.num_terms} device terms in {pl.num_groups} groups, "
          f"worst error / tolerance {worst:.2e}")
    assert (np.abs(want[0]) > 1e-3).sum() >= 3  # (the batch does not vanish)
    pl.destroy()


def _against_values(pl, specs, block, got, label):
    """got (n_ops, K) against K calls of values, per operator and column within ATOL_k |psi_c|^2 -> the worst error / tolerance"""
    K = block.shape[1]
    worst = 0.0
    for c in range(K):
        col = block[:, c].contiguous()
        one = pl.values(col)
        n2 = float((col.abs() ** 2).sum())
        for k, spec in enumerate(specs):
            err, tol = abs(got[k, c] - one[k]), _atol(spec.terms) * n2
            worst = max(worst, err / tol)
            assert err <= tol, (label, k, c, got[k, c], one[k], err, tol)
    return worst


@pytest.mark.parametrize("name", ["ring16_k3_c128", "spinful6_k0_flip_plus_f64"])
def test_chunks_of_columns_and_their_tails(torch, name):
    """K = 1, 8, 11 (a full chunk and a tail of 3) and 64 (8 chunks) against values column by column; the columns are not normalised"""
    basis, reps, block3, specs, _sections, _want = _case(name)
    pl = D.ExpectationPlan(basis, reps, specs)
    wide = _columns(torch, reps, block3.dtype, range(100, 164), normalise=False)
    single = np.stack([pl.values(wide[:, c].contiguous()) for c in range(64)], axis=1)
    norms2 = (wide.abs() ** 2).sum(dim=0).cpu().numpy()
    tol = np.array([_atol(s.terms) for s in specs])[:, None] * norms2[None, :]
    for K in (1, 8, 11, 64):
        assert pl.block_kernel(K) == _family(name, basis)
        got = pl.values_block(wide[:, :K].contiguous())
        assert got.shape == (len(specs), K)
        ratio = np.abs(got - single[:, :K]) / tol[:, :K]
        print(f"values_block {name} K = {K}: worst error / tolerance against values {ratio.max():.2e}")
        assert ratio.max() <= 1.0, (name, K, np.unravel_index(ratio.argmax(), ratio.shape))
    assert np.abs(single).max() > 1e-3
    pl.destroy()


def test_layouts_agree_and_unused_columns_do_not_leak(torch):
    basis, reps, _block3, specs, _sections, _want = _case("ring16_k3_c128")
    pl = D.ExpectationPlan(basis, reps, specs)
    inter = _columns(torch, reps, torch.complex128, range(40, 45))
    colmajor = inter.t().contiguous().t()
    assert colmajor.stride() == (1, inter.shape[0]) and inter.stride() == (5, 1)
    wide = torch.full((inter.shape[0], 10), float("nan"), dtype=torch.complex128, device=inter.device)
    wide[:, 1::2] = inter
    view = wide[:, 1::2]
    assert view.stride() == (10, 2)
    a, b, c = pl.values_block(inter), pl.values_block(colmajor), pl.values_block(view)
    assert np.isfinite(c).all()
    tol = np.array([_atol(s.terms) for s in specs])[:, None]
    assert (np.abs(a - b) <= tol).all() and (np.abs(a - c) <= tol).all()
    assert _against_values(pl, specs, inter, a, "layouts") <= 1.0
    pl.destroy()


def test_more_than_4096_terms(torch):
    """more unique device terms than one launch of the single-state kernel takes: the block launches split by terms"""
    basis, reps, psi, _states, _vec, sections = _setup(torch, BIG)
    specs = [s for s in (config.parse_operator(sec, basis.spec) for sec in sections) if s.terms]
    pl = D.ExpectationPlan(basis, reps, specs)
    assert pl.num_terms > 4096
    block = _columns(torch, reps, psi.dtype, (11, 12, 13))
    worst = _against_values(pl, specs, block, pl.values_block(block), BIG)
    print(f"values_block {BIG}: {pl.num_terms} device terms, worst error / tolerance against values {worst:.2e}")
    # and 64 columns: more (term, column) pairs than one launch takes -- the launches split by columns too
    wide = _columns(torch, reps, psi.dtype, range(200, 264))
    got = pl.values_block(wide)
    for c in (0, 7, 8, 37, 63):
        one = pl.values(wide[:, c].contiguous())
        assert all(abs(got[k, c] - one[k]) <= _atol(s.terms) for k, s in enumerate(specs)), c
    pl.destroy()


def test_float64_blocks_are_promoted_where_the_characters_are_complex(torch):
    basis, reps, _block3, specs, _sections, _want = _case("ring16_k3_c128")  # complex characters
    pl = D.ExpectationPlan(basis, reps, specs)
    real = _columns(torch, reps, torch.float64, (5, 6, 7, 8))
    a, b = pl.values_block(real), pl.values_block(real.to(torch.complex128))
    assert a.tobytes() == b.tobytes() and np.abs(a).max() > 1e-3
    pl.destroy()
    basis, reps, _block3, specs, _sections, _want = _case("ring16_k8_reflection_inversion_minus_f64")  # +-1 characters
    pl = D.ExpectationPlan(basis, reps, specs)
    real = _columns(torch, reps, torch.float64, (5, 6, 7, 8))
    a, b = pl.values_block(real), pl.values_block(real.to(torch.complex128))
    tol = np.array([_atol(s.terms) for s in specs])[:, None]
    assert (np.abs(a - b) <= tol).all() and np.abs(a).max() > 1e-3
    pl.destroy()


def test_two_calls_and_two_plans_are_bitwise_equal(torch):
    for name in ("ring16_k3_c128", "spinless12_dihedral_reflection_odd_f64", "ring16_k8_reflection_inversion_minus_f64"):
        basis, reps, block3, specs, _sections, _want = _case(name)
        block = _columns(torch, reps, block3.dtype, range(20, 31))
        pl = D.ExpectationPlan(basis, reps, specs)
        a, b = pl.values_block(block), pl.values_block(block)
        assert a.tobytes() == b.tobytes()
        pl2 = D.ExpectationPlan(basis, reps, specs)
        assert pl2.values_block(block).tobytes() == a.tobytes()
        pl2.destroy()
        pl.destroy()


def test_the_column_loop_behind_the_environment_knob(torch, monkeypatch):
    basis, reps, _block3, specs, _sections, _want = _case("ring16_k3_c128")
    pl = D.ExpectationPlan(basis, reps, specs)
    block = _columns(torch, reps, torch.complex128, range(50, 55))
    kernel = pl.values_block(block)
    tol = np.array([_atol(s.terms) for s in specs])[:, None]
    monkeypatch.setenv("LS_AMD_EXPECT_BLOCK", "columns")
    assert pl.block_kernel(5) == "columns" and pl.block_kernel(1) == "columns"
    for b in (block, block.t().contiguous().t()):  # (strided rows go through the plan's scratch column; contiguous columns directly)
        loop = pl.values_block(b)
        assert (np.abs(loop - kernel) <= tol).all()
    assert np.array_equal(pl.values_block(block)[:, 2], pl.values(block[:, 2].contiguous()))
    monkeypatch.setenv("LS_AMD_EXPECT_BLOCK", "kernel")
    assert pl.block_kernel(5) == "k_expect_blk"
    assert pl.values_block(block).tobytes() == kernel.tobytes()
    monkeypatch.setenv("LS_AMD_EXPECT_BLOCK", "auto")
    assert pl.block_kernel(5) == "k_expect_blk"
    pl.destroy()


def test_representatives_that_are_not_the_sector_raise_the_error_flag(torch):
    """the lower half of the representatives (tests/test_gpu_expectation.py): sigma^+_11 sends each of them to a word inside the weight
    sector that is not in the array.  The flag is cleared by the call that reports it: the plan keeps refusing that batch, and a plan
    over the whole sector answers afterwards."""
    sec = {"terms": [{"expression": "σ⁻₀ σ⁺₁ σᶻ₂", "sites": [[0, 11, 7]]}]}
    for cfg in (E.ring(12, 6, 0), E.ring(12, 6, None)):  # the static index table, and the searched index of an incomplete array
        basis = D.loadConfigFromDict(cfg)
        reps = D.enumerateStates(basis, 1)[0][0]
        cut = reps[: reps.numel() // 2].contiguous()
        pl = D.ExpectationPlan(basis, cut, [sec])
        block = _columns(torch, cut, torch.float64, (1, 2, 3))
        for _ in range(2):
            with pytest.raises(LsAmdError, match="not in the basis"):
                pl.values_block(block)
        assert pl.block_kernel(3) == "k_expect_blk"
        pl.destroy()
        whole = D.ExpectationPlan(basis, reps, [sec])
        block = _columns(torch, reps, torch.float64, (1, 2, 3))
        got = whole.values_block(block)
        assert _against_values(whole, [config.parse_operator(sec, basis.spec)], block, got, "after the flag") <= 1.0
        whole.destroy()


def test_refusals_come_back_by_name(torch):
    from distributed_matvec_amd import _lib

    L = _lib.load()
    basis = D.loadConfigFromDict(E.ring(12, 6, 5))  # complex characters
    reps = D.enumerateStates(basis, 1)[0][0]
    n = int(reps.numel())
    sec = {"terms": [{"expression": "σ⁺₀ σ⁻₁ σᶻ₂", "sites": [[0, 5, 7]]}]}
    pl = D.ExpectationPlan(basis, reps, [sec])
    block = _columns(torch, reps, torch.complex128, (1, 2))
    out = np.zeros(2 * 2)
    f64p = C.POINTER(C.c_double)
    ptr, outp = C.c_void_p(block.data_ptr()), out.ctypes.data_as(f64p)
    err = lambda: L.ls_amd_last_error().decode()  # noqa: E731
    assert L.ls_amd_expect_values_block(pl.h, 1, 0, ptr, 2, 1, outp, None) == -1 and "ls_amd_expect_values_block: K = 0 is outside [1, 64]" in err()
    assert L.ls_amd_expect_values_block(pl.h, 1, 65, ptr, 65, 1, outp, None) == -1 and "K = 65 is outside [1, 64]" in err()
    assert L.ls_amd_expect_values_block(pl.h, 1, 2, None, 2, 1, outp, None) == -1 and "NULL block" in err()
    assert L.ls_amd_expect_values_block(None, 1, 2, ptr, 2, 1, outp, None) == -1 and "NULL plan" in err()
    assert L.ls_amd_expect_values_block(pl.h, 1, 2, ptr, 2, 1, None, None) == -1 and "NULL output" in err()
    assert L.ls_amd_expect_values_block(pl.h, 7, 2, ptr, 2, 1, outp, None) == -1 and "unknown dtype 7" in err()
    assert L.ls_amd_expect_values_block(pl.h, 0, 2, ptr, 2, 1, outp, None) == -1
    assert "ls_amd_expect_values_block: f64 needs +-1 characters (complex characters: use c128)" in err()
    assert L.ls_amd_expect_values_block(pl.h, 1, 2, ptr, 0, 1, outp, None) == -1 and "must be positive" in err()
    assert L.ls_amd_expect_values_block(pl.h, 1, 2, ptr, 2, 0, outp, None) == -1 and "must be positive" in err()
    assert L.ls_amd_expect_values_block(pl.h, 1, 2, ptr, 1, 1, outp, None) == -1 and "share storage" in err()
    assert L.ls_amd_expect_block_kernel_name(pl.h, 65) is None and "outside [1, 64]" in err()
    assert L.ls_amd_expect_values_block(pl.h, 1, 2, ptr, 2, 1, outp, None) == 0  # (and the good call goes through)
    assert np.array_equal(out.view(np.complex128), pl.values_block(block)[0])
    with pytest.raises(LsAmdError, match=r"must be a 2-D block \(n, K\)"):
        pl.values_block(block[:, 0])
    with pytest.raises(LsAmdError, match=r"K = 65 columns, outside \[1, 64\]"):
        pl.values_block(torch.zeros((n, 65), dtype=torch.complex128, device=block.device))
    with pytest.raises(LsAmdError, match=f"must have {n} rows"):
        pl.values_block(block[:-1])
    with pytest.raises(LsAmdError, match="device tensor"):
        pl.values_block(block.cpu())
    with pytest.raises(LsAmdError, match="neither float64 nor complex128"):
        pl.values_block(block.to(torch.complex64))
    pl.destroy()
    with pytest.raises(LsAmdError, match="destroyed"):
        pl.values_block(block)
    with pytest.raises(LsAmdError, match="destroyed"):
        pl.block_kernel(2)


def test_64_bit_words(torch):
    """36 sites at weight 3, translations in sector k = 5 (the basis of test_64_bit_words_against_unproject_and_matvec): images above
    2^32, K = 2, against values per column"""
    basis = D.loadConfigFromDict(E.ring(36, 3, 5))
    reps = D.enumerateStates(basis, 1)[0][0]
    assert basis.numberBits() == 36 and reps.numel() < 256
    rs = np.random.RandomState(36)
    sections = []
    for expr, k in (("σ⁺₀ σ⁻₁ σᶻ₂", 3), ("σ⁺₀ σ⁺₁ σ⁻₂ σ⁻₃", 4), ("σᶻ₀ σᶻ₁ σᶻ₂", 3), ("σ⁻₀ σᶻ₁ σ⁺₂ σᶻ₃", 4)):
        for _ in range(3):
            near = int(rs.randint(36))
            sites = [(near + int(d)) % 36 for d in rs.choice(6, size=k, replace=False)]
            sections.append({"terms": [{"expression": f"{_coef(rs)} × {expr}", "sites": [sites]}]})
    sections.append({"terms": [{"expression": "σ⁺₀ σ⁻₁", "sites": [[35, 33]]}, {"expression": "0.5 × σᶻ₀ σᶻ₁", "sites": [[34, 35], [31, 32]]}]})
    specs = [config.parse_operator(sec, basis.spec) for sec in sections]
    pl = D.ExpectationPlan(basis, reps, specs)
    block = _columns(torch, reps, torch.complex128, (11, 12))
    got = pl.values_block(block)
    worst = _against_values(pl, specs, block, got, "ring36")
    print(f"values_block ring36 weight 3 k = 5 (64-bit words): {len(specs)} operators x 2 columns, worst error / tolerance {worst:.2e}")
    assert np.abs(got).max() > 1e-3
    pl.destroy()


def test_expectation_values_block_normalises_every_column(torch):
    basis, reps, _block3, specs, _sections, _want = _case("torus_4x3_f64")
    block = _columns(torch, reps, torch.float64, (3, 4, 5), normalise=False)
    got = expectation_values_block(basis, reps, block, specs)
    tol = np.array([_atol(s.terms) for s in specs])
    for c in range(3):
        assert (np.abs(got[:, c] - D.expectation_values(basis, reps, block[:, c].contiguous(), specs)) <= tol).all()
    assert _u64(reps).size == block.shape[0]
