"""Amplitudes of sector states on product states and Born sampling on the GPU (SectorAmplitudes / k_amplitude_pull, k_amplitude_pull_fermi,
k_orbit_image; amplitudes, sample_states, sampling.snapshots) against the dense isometry B of tests/entanglement_reference.py and
tests/fermion_entanglement_reference.py -- <s|psi> = (B psi)[position of s] -- over the 21 sectors of the projection tests, against the
shipped expansion kernels, in blocks of columns of every layout, over batch sizes on both sides of a tile and of the grid, state_info
and orbit images against the host, the failures that must be loud, and sampling: exact conditions, Pearson's chi^2 against |B psi|^2,
and a Monte-Carlo estimate of a ground-state correlation from snapshots alone.

Tolerance (derived, not measured): the stabiliser sum of at most |G| unit characters, a square root and one complex product:
    |got - want| <= 2 (|G| + 4) 2^-53 max|psi|
The chi^2 condition is the mean plus six standard deviations of the chi^2 law, chi^2 < dof + 6 sqrt(2 dof), over the bins of expected
count >= 5 and one merged bin of the rest (dropped when its own expectation is below 5)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
from distributed_matvec_amd import SectorAmplitudes  # noqa: F401  (the feature under test: without it nothing here can run)
from test_gpu_projection import ADJOINT, FERMI, SPIN, sector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(torch, words):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(words, dtype=np.uint64)).view(np.int64).copy()).cuda()


def bound(order, scale):
    return 2.0 * (order + 4) * 2.0 ** -53 * scale


def _is_cplx(name):
    return (SPIN.get(name) or FERMI[name])[1] == "c128"


def _bits(s):
    return s.model.number_sites if name_is_spin(s) else s.case.M


def name_is_spin(s):
    return hasattr(s, "cfg")


def _live(s):
    return np.asarray(E.tables(s.cfg)[5] if name_is_spin(s) else s.case.live)


def _expand(s, psi):
    """B psi over s.full (numpy, (F,) or (F, K))"""
    return s.B @ psi if name_is_spin(s) else s.case.columns @ psi


def random_psi(torch, n, K, cplx, seed):
    rs = np.random.RandomState(seed)
    a = rs.rand(n, K) - 0.5
    if cplx:
        a = a + 1j * (rs.rand(n, K) - 0.5)
    return a, torch.from_numpy(a).cuda()


def outside_words(s):
    """words that are no states of the basis without symmetries: one bit above the sites; at a fixed weight / particle number one
    particle more and one less; on the spinful layout (N_up + 1, N_down - 1) -- the right total in the wrong split"""
    M = _bits(s)
    first = int(s.full[len(s.full) // 2])
    out = []
    if M < 64:
        out.append(first | 1 << M)
    if name_is_spin(s):
        fixed = s.model.hamming_weight >= 0
    else:
        fixed = s.case.spinful or s.case.N is not None
    if fixed:
        free = [i for i in range(M) if not first >> i & 1]
        used = [i for i in range(M) if first >> i & 1]
        out += [first | 1 << free[0], first & ~(1 << used[0])]
    if not name_is_spin(s) and s.case.spinful:
        L = s.case.L
        up_free = [i for i in range(L) if not first >> i & 1]
        dn_used = [i for i in range(L, 2 * L) if first >> i & 1]
        out.append((first | 1 << up_free[0]) & ~(1 << dn_used[0]))
    have = set(int(x) for x in s.full)
    assert out and not any(w in have for w in out)
    return out


def query_batch(s, seed=5):
    """(words, position in s.full or -1): every state, 50 duplicates and the outside words, shuffled"""
    rs = np.random.RandomState(seed)
    dup = rs.randint(0, s.F, size=50)
    out = outside_words(s)
    words = np.concatenate([s.full, s.full[dup], np.array(out, dtype=np.uint64)])
    pos = np.concatenate([np.arange(s.F), dup, np.full(len(out), -1)])
    order = rs.permutation(len(words))
    return words[order], pos[order]


@pytest.mark.parametrize("name", sorted(SPIN) + sorted(FERMI))
def test_amplitudes_match_the_dense_isometry(torch, name):
    s = sector(name)
    cplx = _is_cplx(name)
    psi_np, psi = random_psi(torch, s.n, 1, cplx, 7)
    psi_np, psi = psi_np[:, 0], psi[:, 0].contiguous()
    words, pos = query_batch(s)
    sa = D.SectorAmplitudes(s.basis, s.reps)
    got_t = sa.amplitudes(_dev(torch, words), psi)
    signed = not name_is_spin(s) and s.basis.hasFermionSigns()  # a projected fermionic basis
    assert sa.kernel == ("k_amplitude_pull_fermi" if signed else "k_amplitude_pull")
    assert got_t.shape == (len(words),)
    assert got_t.dtype == (torch.complex128 if cplx or sa.complex_characters else torch.float64)
    if name == "ring12_k3_promoted_f64":
        assert got_t.dtype == torch.complex128 and psi.dtype == torch.float64
    got = got_t.cpu().numpy()
    full = _expand(s, psi_np)
    want = np.where(pos >= 0, full[np.maximum(pos, 0)], 0.0)
    tol = bound(s.order, float(np.abs(psi_np).max()))
    worst = float(np.abs(got - want).max())
    print(f"amplitudes {name}: {len(words)} words on {s.n} rows, |G| = {s.order}, max error {worst:.2e}, bound {tol:.2e}, ratio {worst / tol:.3f}")
    assert np.isfinite(got).all() and worst <= tol, (name, worst, tol)
    assert (got[pos < 0] == 0).all()  # outside the conserved numbers: exactly 0, and no error
    dead = (pos >= 0) & ~_live(s)[np.maximum(pos, 0)]
    assert (got[dead] == 0).all()  # orbits of zero norm: exactly 0
    if name == "ring12_k6_reflection_inversion_minus_zero_norms":
        assert dead.sum() > 100
    if name == "ring10_weight5_unprojected_identity":
        inside = pos >= 0
        assert np.array_equal(got[inside], psi_np[pos[inside]])  # B = 1: psi permuted
    # the one-shot form is the same call
    assert torch.equal(D.amplitudes(s.basis, s.reps, psi, _dev(torch, words)), got_t)
    sa.destroy()


@pytest.mark.parametrize("name", ADJOINT)
def test_amplitudes_of_every_state_are_the_expansion(torch, name):
    s = sector(name)
    dtype = torch.complex128 if _is_cplx(name) else torch.float64
    psi = D.fillRandom(s.reps, 5, dtype)
    want = s.unproject(psi)
    got = D.amplitudes(s.basis, s.reps, psi, _dev(torch, s.full))
    tol = bound(s.order, float(psi.abs().max()))
    dev = float((got - want).abs().max())
    print(f"expansion {name}: max |amplitudes - unproject| = {dev:.2e}, bound {tol:.2e}")
    assert got.shape == want.shape and dev <= tol and float(got.abs().max()) > 1e-3


BLOCKS = ["ring12_k3_complex_characters_c128", "spinful6_k0_flip_plus", "ring16_k0_810_rows"]


@pytest.mark.parametrize("name", BLOCKS)
@pytest.mark.parametrize("K", [1, 3, 8, 9, 64])
def test_blocks_of_columns_in_every_layout(torch, name, K):
    s = sector(name)
    _, psi = random_psi(torch, s.n, K, _is_cplx(name), 100 + K)
    words, _ = query_batch(s)
    states = _dev(torch, words)
    B = len(words)
    sa = D.SectorAmplitudes(s.basis, s.reps)
    single = torch.stack([sa.amplitudes(states, psi[:, c].contiguous()) for c in range(K)], dim=1)
    transposed = psi.T.contiguous().T  # column-major
    wide = torch.zeros(s.n, 2 * K + 1, dtype=psi.dtype, device=psi.device)
    wide[:, 1::2] = psi
    layouts = {"interleaved": psi, "transposed": transposed, "strided view": wide[:, 1::2]}
    assert transposed.stride() == (1, s.n) or K == 1
    assert layouts["strided view"].stride() == (2 * K + 1, 2)
    for what, block in layouts.items():
        got = sa.amplitudes(states, block)
        assert got.shape == (B, K) and got.is_contiguous()
        assert torch.equal(got, single), (name, K, what)  # every column bit for bit the single-vector call
    # out= with strides is honoured, and nothing outside it is touched
    sentinel = 12345.0
    big = torch.full((B + 2, 2 * K), sentinel, dtype=single.dtype, device=psi.device)
    out = big[1:-1, 1::2]
    ret = sa.amplitudes(states, psi, out=out)
    assert ret.data_ptr() == out.data_ptr() and torch.equal(out, single)
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[1:-1, 1::2] = False
    assert bool((big[keep] == sentinel).all())
    colmajor = torch.empty(K, B, dtype=single.dtype, device=psi.device).T
    assert torch.equal(sa.amplitudes(states, psi, out=colmajor), single)
    sa.destroy()


def test_batch_sizes_and_a_second_trip_of_the_grid(torch):
    s = sector("ring16_k0_810_rows")
    psi_np, psi = random_psi(torch, s.n, 8, False, 3)
    words, _ = query_batch(s)
    states = _dev(torch, words)
    sa = D.SectorAmplitudes(s.basis, s.reps)
    whole1, whole8 = sa.amplitudes(states, psi[:, 0].contiguous()), sa.amplitudes(states, psi)
    for B in (0, 1, 63, 257):
        got = sa.amplitudes(states[:B].contiguous(), psi)
        assert got.shape == (B, 8) and torch.equal(got, whole8[:B])
        rep, idx, ch, nrm = sa.state_info(states[:B].contiguous())
        assert rep.shape == idx.shape == ch.shape == nrm.shape == (B,)
        assert sa.orbit_states(idx[:0], idx[:0].to(torch.int32)).shape == (0,)
    assert len(words) > 2 * 2 * 256  # two blocks of 256 lanes take more than two trips each
    assert "LS_AMD_AMP_BLOCKS" not in os.environ
    os.environ["LS_AMD_AMP_BLOCKS"] = "2"
    try:
        capped1, capped8 = sa.amplitudes(states, psi[:, 0].contiguous()), sa.amplitudes(states, psi)
        info = sa.state_info(states)
    finally:
        del os.environ["LS_AMD_AMP_BLOCKS"]
    assert torch.equal(capped1, whole1) and torch.equal(capped8, whole8)
    for a, b in zip(info, sa.state_info(states)):
        assert torch.equal(a, b)
    sa.destroy()


@pytest.mark.parametrize("name", ["ring12_k3_complex_characters_c128", "ring12_k6_reflection_inversion_minus_zero_norms"])
def test_state_info_on_the_device(torch, name):
    from distributed_matvec_amd import _lib

    s = sector(name)
    words, pos = query_batch(s)
    inside = pos >= 0
    sa = D.SectorAmplitudes(s.basis, s.reps)
    rep, idx, ch, nrm = (t.cpu().numpy() for t in sa.state_info(_dev(torch, words)))
    rep = rep.view(np.uint64)
    w_rep, w_ch, w_nrm = E.state_info_all(s.model, words[inside])
    assert np.array_equal(rep[inside], w_rep)
    assert np.abs(nrm[inside] - w_nrm).max() <= 4 * 2.0 ** -53
    alive = w_nrm > 0
    if name.endswith("zero_norms"):
        assert (~alive).sum() > 100
    # (the character of a minimising element is unique up to stabiliser elements: it is defined where the norm is not 0)
    assert np.abs(ch[inside][alive] - w_ch[alive]).max() <= 4 * 2.0 ** -53
    w_idx = np.where(alive, np.searchsorted(s.want_reps, w_rep), -1)
    assert np.array_equal(idx[inside], w_idx)
    # outside the basis: the word itself, no row, character and norm 0
    assert np.array_equal(rep[~inside], words[~inside]) and (idx[~inside] == -1).all()
    assert (ch[~inside] == 0).all() and (nrm[~inside] == 0).all()
    # the host-pointer entry point agrees
    lib = _lib.load()
    q = np.ascontiguousarray(words[inside])
    betas, chars, norms = np.zeros(len(q), dtype=np.uint64), np.zeros(2 * len(q)), np.zeros(len(q))
    lib.ls_hs_state_info(s.basis.payload, len(q), q.ctypes.data_as(_lib.c_u64p), 1, betas.ctypes.data_as(_lib.c_u64p), 1,
                         chars.ctypes.data_as(_lib.c_f64p), norms.ctypes.data_as(_lib.c_f64p))
    _lib.raise_pending_halt()
    assert np.array_equal(betas, rep[inside]) and np.array_equal(norms, nrm[inside])
    host_ch = chars[0::2] + 1j * chars[1::2]
    assert np.array_equal(host_ch[alive], ch[inside][alive])
    sa.destroy()


@pytest.mark.parametrize("K", [1, 8])
def test_two_calls_return_the_same_bytes(torch, K):
    for name in ("ring16_k0_810_rows", "spinful6_k1_flip_minus"):
        s = sector(name)
        _, psi = random_psi(torch, s.n, K, _is_cplx(name), 9)
        block = psi[:, 0].contiguous() if K == 1 else psi
        states = _dev(torch, query_batch(s)[0])
        sa = D.SectorAmplitudes(s.basis, s.reps)
        a, b = sa.amplitudes(states, block), sa.amplitudes(states, block)
        assert a.data_ptr() != b.data_ptr()
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        sa.destroy()


def test_errors_are_flags_and_messages(torch):
    from distributed_matvec_amd import _lib

    L = _lib.load()
    s = sector("ring12_k3_complex_characters_c128")
    states = _dev(torch, s.full)
    _, psi = random_psi(torch, s.n, 8, True, 2)
    # one row removed: its orbit is inside the conserved numbers, has a norm, and is not in the array
    short = s.reps[1:].contiguous()
    sa = D.SectorAmplitudes(s.basis, short)
    with pytest.raises(D.LsAmdError, match="not in the basis"):
        sa.amplitudes(states, psi[1:, 0].contiguous())
    out = sa.amplitudes(states, psi[1:].contiguous(), check=False)
    with pytest.raises(D.LsAmdError, match="not in the basis"):
        sa.check()
    sa.check()  # the flag is cleared once reported
    missing = np.asarray(E.tables(s.cfg)[3]) == 0
    assert bool((out[torch.from_numpy(missing & _live(s)).cuda()] == 0).all())
    sa.destroy()
    # the C level names a wrong dtype, K = 65, an out that shares storage and an out that overlaps psi
    sa = D.SectorAmplitudes(s.basis, s.reps)
    h, B = sa._plan(), states.numel()
    real = torch.zeros(s.n, dtype=torch.float64, device="cuda")
    out = torch.zeros(B, 65, dtype=torch.complex128, device="cuda")
    err = lambda: L.ls_amd_last_error().decode()  # noqa: E731
    sp, pp, op = C.c_void_p(states.data_ptr()), C.c_void_p(psi.data_ptr()), C.c_void_p(out.data_ptr())
    assert L.ls_amd_amp_amplitudes(h, 7, 1, B, sp, pp, 8, 1, op, 65, 1, None) == -1 and "unknown dtype 7" in err()
    assert L.ls_amd_amp_amplitudes(h, 0, 1, B, sp, C.c_void_p(real.data_ptr()), 1, 0, op, 65, 1, None) == -1
    assert "f64 needs +-1 characters" in err()
    for K in (0, 65):
        assert L.ls_amd_amp_amplitudes(h, 1, K, B, sp, pp, 8, 1, op, 65, 1, None) == -1 and f"K = {K} columns, outside [1, 64]" in err()
    assert L.ls_amd_amp_amplitudes(h, 1, 8, B, sp, pp, 8, 1, op, 4, 1, None) == -1 and "share storage" in err()
    assert L.ls_amd_amp_amplitudes(h, 1, 8, B, sp, pp, 8, 1, pp, 8, 1, None) == -1 and "out overlaps psi" in err()
    assert L.ls_amd_amp_amplitudes(h, 1, 8, -1, sp, pp, 8, 1, op, 65, 1, None) == -1 and "negative count" in err()
    assert L.ls_amd_amp_amplitudes(h, 1, 8, B, None, pp, 8, 1, op, 65, 1, None) == -1 and "NULL states" in err()
    assert L.ls_amd_amp_amplitudes(h, 1, 8, 0, None, None, 8, 1, None, 65, 1, None) == 0  # B = 0 is a no-op
    with pytest.raises(D.LsAmdError, match="out must be"):
        sa.amplitudes(states, psi, out=torch.empty(B, 1, dtype=torch.complex128, device="cuda").expand(B, 8))
    assert sa.kernel == "k_amplitude_pull" and sa.num_elements == 12
    # orbit_states: a row or an element out of range is a flag and a message
    rows = torch.tensor([0, s.n], dtype=torch.int64, device="cuda")
    with pytest.raises(D.LsAmdError, match=rf"a row outside \[0, {s.n}\) or an element outside \[0, 12\)"):
        sa.orbit_states(rows, torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(D.LsAmdError, match="an element outside"):
        sa.orbit_states(rows[:1], torch.full((1,), 12, dtype=torch.int32, device="cuda"))
    sa.check()
    # sampling refuses what is no distribution
    with pytest.raises(D.LsAmdError, match="psi is zero"):
        sa.sample(torch.zeros(s.n, dtype=torch.complex128, device="cuda"), 10)
    bad = psi[:, 0].clone()
    bad[3] = float("nan")
    with pytest.raises(D.LsAmdError, match="not finite"):
        sa.sample(bad, 10)
    sa.destroy()
    assert D.SectorAmplitudes(sector("spinful6_k1_flip_minus").basis, sector("spinful6_k1_flip_minus").reps).kernel == "k_amplitude_pull_fermi"


@pytest.mark.parametrize("name", ["ring12_k6_reflection_inversion_minus_zero_norms", "spinful6_k1_flip_minus"])
def test_orbit_states_of_every_row_and_element(torch, name):
    from distributed_matvec_amd import _lib

    L = _lib.load()
    s = sector(name)
    sa = D.SectorAmplitudes(s.basis, s.reps)
    n_el = sa.num_elements
    assert n_el == s.order
    rows = torch.arange(s.n, dtype=torch.int64, device="cuda").repeat_interleave(n_el)
    elements = torch.arange(n_el, dtype=torch.int32, device="cuda").repeat(s.n)
    got = _u64(sa.orbit_states(rows, elements))
    ok = C.c_int(0)
    reps = _u64(s.reps)
    want = np.array([L.ls_amd_test_orbit_state(s.basis.payload, C.c_uint64(int(reps[r])), e, C.byref(ok))
                     for r in range(s.n) for e in range(n_el)], dtype=np.uint64)
    assert ok.value == 1 and np.array_equal(got, want)
    assert len(np.unique(got)) > s.n  # the orbits, not the representatives alone
    rep, idx, _, _ = sa.state_info(_dev(torch, got))
    assert torch.equal(rep, s.reps[rows]) and torch.equal(idx, rows)
    sa.destroy()


def chi_square(words, full, p):
    """(Pearson's chi^2, dof) of the sampled words against the probabilities p over full"""
    at = np.searchsorted(full, words)
    assert (at < len(full)).all() and np.array_equal(full[at], words)  # every sampled word is a state of the basis
    counts = np.bincount(at, minlength=len(full)).astype(np.float64)
    assert (p[counts > 0] > 0).all()  # no sampled word has probability 0
    expected = len(words) * p
    big = expected >= 5
    chi2 = float(((counts[big] - expected[big]) ** 2 / expected[big]).sum())
    bins = int(big.sum())
    rest = float(expected[~big].sum())
    if rest >= 5:
        chi2 += (float(counts[~big].sum()) - rest) ** 2 / rest
        bins += 1
    return chi2, bins - 1


@pytest.mark.parametrize("name", ["ring12_k0_inversion_plus_stabilisers_f64", "ring8_k1_c128", "ring12_k6_reflection_inversion_minus_zero_norms"])
def test_samples_follow_the_born_distribution(torch, name):
    s = sector(name)
    psi_np, psi = random_psi(torch, s.n, 1, _is_cplx(name), 31)
    psi_np, psi = psi_np[:, 0], psi[:, 0].contiguous()
    p = np.abs(_expand(s, psi_np)) ** 2
    p = p / p.sum()
    N = 200_000
    sa = D.SectorAmplitudes(s.basis, s.reps)
    words_t, rows = sa.sample(psi, N, seed=1234, return_rows=True)
    assert words_t.shape == (N,) and words_t.dtype == torch.int64 and rows.shape == (N,)
    # exact conditions
    assert torch.equal(sa.sample(psi, N, seed=1234), words_t)
    assert not torch.equal(sa.sample(psi, N, seed=1235), words_t)
    assert torch.equal(D.sample_states(s.basis, s.reps, psi, N, seed=1234), words_t)
    rep, idx, _, _ = sa.state_info(words_t)
    assert torch.equal(idx, rows) and torch.equal(rep, s.reps[rows])
    chi2, dof = chi_square(_u64(words_t), s.full, p)
    limit = dof + 6.0 * math.sqrt(2.0 * dof)
    print(f"sampling {name}: {N} samples over {s.F} states, chi^2 = {chi2:.1f} at dof {dof}, limit {limit:.1f}")
    assert dof > 20 and chi2 < limit, (name, chi2, dof, limit)
    assert sa.sample(psi, 0).shape == (0,)
    sa.destroy()


def test_snapshots_of_a_ground_state_estimate_a_correlation(torch):
    from distributed_matvec_amd import _lib, config, sampling
    from distributed_matvec_amd.diagonalize import LocalOperator, lanczos_smallest

    L = _lib.load()
    cfg = config.heisenberg_chain_config(24, symm=True)
    N = 100_000
    words_t, amps = sampling.snapshots(cfg, N, seed=7)
    assert words_t.shape == (N,) and amps.shape == (N,)
    w = _u64(words_t)
    z0, z1 = 1.0 - 2.0 * (w & np.uint64(1)).astype(np.float64), 1.0 - 2.0 * ((w >> np.uint64(1)) & np.uint64(1)).astype(np.float64)
    est = float((z0 * z1).mean())
    stderr = float((z0 * z1).std(ddof=1) / math.sqrt(N))
    want = float(D.correlations.correlations(cfg).zz[0][1])
    print(f"snapshots: <sz_0 sz_1> = {est:.5f} +- {stderr:.5f} from {N} words, {want:.5f} from spin_correlations "
          f"({abs(est - want) / stderr:.2f} standard errors)")
    assert stderr > 0 and abs(est - want) <= 6.0 * stderr
    assert -0.9 < want < -0.3  # an antiferromagnet: the comparison is not of constants
    # the amplitudes beside the words: |amp|^2 is the reference probability of each word, from the expansion kernel on the same state
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    dtype = amps.dtype
    psi = lanczos_smallest(LocalOperator(h, reps, dtype), num_evals=1, eps=1e-10).eigenvectors[0]
    psi = psi / float(torch.linalg.vector_norm(psi))
    words2, amps2 = sampling.snapshots(cfg, 2000, seed=8, state=psi)
    full = D.unproject(basis, reps[0], psi)
    at = np.array([L.ls_amd_test_project_state_index(basis.payload, C.c_uint64(int(x))) for x in _u64(words2)], dtype=np.int64)
    assert (at >= 0).all()
    ref = full[torch.from_numpy(at).cuda()]
    order = int(L.ls_amd_basis_group_order(basis.payload)) * (2 if basis.spinInversion() else 1)
    tol = bound(order, float(psi.abs().max()))
    dev = float((amps2 - ref).abs().max())
    print(f"snapshots: max |amplitude - unproject| over 2000 words = {dev:.2e}, bound {tol:.2e}")
    assert dev <= tol and float((amps2.abs() ** 2 - ref.abs() ** 2).abs().max()) <= 2.0 * tol * float(ref.abs().max())
    assert float((amps2.abs() ** 2).min()) > 0.0  # a sampled word has a probability
