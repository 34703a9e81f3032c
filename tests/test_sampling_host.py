"""Amplitudes on product states and Born sampling, the parts that need no device (SectorAmplitudes, amplitudes, sample_states, snapshots;
ls_amd_amp): the ABI and the build, the element numbering of orbit_states / sample -- ls_amd_test_orbit_state evaluates it from the
compiled host tables -- against entanglement_reference.apply_perm_all, and the refusals of the Python layer that are raised before a
device is asked for.

The numbering: the library keeps its permutation elements in the order of its own group closure (not the sorted order of the oracle),
so element p is identified by its action on the one-hot words (ls_amd_basis_apply_group_element) and by its character; what is pinned
is that element 2 p of a basis with the global inversion is that permutation, element 2 p + 1 the same followed by ^ mask (p itself
without an inversion), applied to EVERY state as apply_perm_all applies it, and that the list as a whole is the reference's element list,
characters included."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
import fermion_entanglement_reference as R
import fermion_symm as F
from distributed_matvec_amd import SectorAmplitudes  # noqa: F401  (the feature under test: without it nothing here can run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_amd_amp_create", "ls_amd_amp_num_elements", "ls_amd_amp_amplitudes", "ls_amd_amp_state_info", "ls_amd_amp_orbit_states",
         "ls_amd_amp_check", "ls_amd_amp_kernel_name", "ls_amd_amp_destroy", "ls_amd_test_orbit_state")


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def _reps(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy())


def test_abi_makefile_and_python_names():
    header = open(os.path.join(ROOT, "include", "ls_amd.h"), encoding="utf-8").read()
    L = _lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
    assert "typedef struct ls_amd_amp ls_amd_amp;" in header
    make = open(os.path.join(ROOT, "distributed-matvec_amd", "csrc", "Makefile"), encoding="utf-8").read()
    ksrc = re.search(r"^KSRC := (.*)$", make, re.M).group(1).split()
    assert "k_amplitude.hip" in ksrc and "k_amplitude_fermi.hip" in ksrc
    assert re.search(r"^k_amplitude\.o k_amplitude_fermi\.o.*: k_amplitude_t\.hpp k_cross_t\.hpp k_project_t\.hpp lsk_fermi\.hpp$", make, re.M)
    lsk = open(os.path.join(ROOT, "distributed-matvec_amd", "csrc", "lsk.h"), encoding="utf-8").read()
    for name in ("lsk_amplitude_pull", "lsk_amplitude_pull_fermi", "lsk_amplitude_info", "lsk_amplitude_info_fermi", "lsk_orbit_image",
                 "lsk_orbit_image_fermi"):
        assert re.search(r"\b%s\(" % name, lsk), name
    # the new units are not fingerprinted: the fingerprints of the existing kernels stay what they were
    isa = open(os.path.join(ROOT, "scripts", "kernel_isa_sha.py"), encoding="utf-8").read()
    assert "k_amplitude" not in isa
    for name in ("SectorAmplitudes", "amplitudes", "sample_states", "snapshots"):
        assert name in D.__all__ and getattr(D, name) is getattr(D.sampling, name), name
    assert D.sampling.__name__.endswith(".sampling")  # the module keeps its name


def _spin(cfg):
    model, full, reps = E.tables(cfg)[:3]
    elems = [(np.asarray(p), flip, ch) for p, flip, ch in E._elements(model)]
    return D.loadConfigFromDict(cfg), full, reps, elems, int(model.mask), model.spin_inversion != 0


def _fermi(case):
    elems = [(np.asarray(p), False, complex(ch)) for p, ch in case.group]
    return D.loadConfigFromDict({"basis": case.basis_config()}), case.states, case.reps, elems, (1 << case.M) - 1, False


SECTORS = {
    "ring12_k0_inversion_plus": lambda: _spin(E.ring(12, 6, 0, inv=1)),
    "ring12_k6_reflection_inversion_minus": lambda: _spin(E.ring(12, 6, 6, inv=-1, reflect=1)),
    "spinless10_dihedral": lambda: _fermi(R.Case(10, 5, gens=F.dihedral(10), secs=[0, 1])),
    "spinful6_k1_flip_minus": lambda: _fermi(R.Case(6, up=(3, 3), gens=F.translations(6), secs=[1], flip=-1)),
}


def _orbit(L, basis, states, element):
    ok = C.c_int(0)
    out = np.empty(len(states), dtype=np.uint64)
    for i, s in enumerate(states):
        out[i] = L.ls_amd_test_orbit_state(basis.payload, C.c_uint64(int(s)), element, C.byref(ok))
        assert ok.value == 1
    return out


@pytest.mark.parametrize("name", sorted(SECTORS))
def test_element_numbering_against_apply_perm_all(name):
    L = _lib()
    basis, full, reps, elems, mask, inv = SECTORS[name]()
    M = int(mask).bit_length()
    order = int(L.ls_amd_basis_group_order(basis.payload))
    n_el = order * (2 if inv else 1)
    assert n_el == len(elems)
    re_, im_ = C.c_double(), C.c_double()
    seen = collections.Counter()
    for e in range(n_el):
        g, flip = (e >> 1, bool(e & 1)) if inv else (e, False)
        # the permutation of element g by its action on the one-hot words: bit i of the image is bit perm[i] of the word
        perm = np.empty(M, dtype=np.int64)
        for src in range(M):
            perm[int(L.ls_amd_basis_apply_group_element(basis.payload, g, C.c_uint64(1 << src))).bit_length() - 1] = src
        want = E.apply_perm_all(perm, full)
        if flip:
            want = want ^ np.uint64(mask)
        assert np.array_equal(_orbit(L, basis, full, e), want), (name, e)
        L.ls_amd_basis_group_character(basis.payload, g, C.byref(re_), C.byref(im_))
        ch = complex(re_.value, im_.value)
        seen[(tuple(perm), flip, round(ch.real, 9), round(ch.imag, 9))] += 1
    # as a whole: the reference's element list, every element once, with its character (times the inversion's on the flipped half)
    sign = 1.0
    if inv:
        sign = [c for p, f, c in elems if f and tuple(p) == tuple(range(M))][0].real
    want = collections.Counter((tuple(int(x) for x in p), f, round((c * (sign if f else 1.0)).real, 9), round((c * (sign if f else 1.0)).imag, 9))
                               for p, f, c in elems)
    assert seen == want
    # out of range: refused by name, *ok cleared
    ok = C.c_int(1)
    assert L.ls_amd_test_orbit_state(basis.payload, C.c_uint64(int(full[0])), n_el, C.byref(ok)) == 0 and ok.value == 0
    assert f"outside [0, {n_el})" in L.ls_amd_last_error().decode()
    ok = C.c_int(1)
    assert L.ls_amd_test_orbit_state(basis.payload, C.c_uint64(1 << M), 0, C.byref(ok)) == 0 and ok.value == 0
    assert "bits above" in L.ls_amd_last_error().decode()


@pytest.mark.parametrize("name", sorted(SECTORS))
def test_the_elements_cover_an_orbit_with_equal_multiplicity(name):
    L = _lib()
    basis, full, reps, elems, mask, inv = SECTORS[name]()
    n_el = len(elems)
    sizes = set()
    for r in reps:
        images = np.array([_orbit(L, basis, [r], e)[0] for e in range(n_el)], dtype=np.uint64)
        orbit, counts = np.unique(images, return_counts=True)
        assert orbit[0] == r  # the representative is the orbit minimum
        assert n_el % len(orbit) == 0 and (counts == n_el // len(orbit)).all(), (name, hex(int(r)))
        sizes.add(len(orbit))
    print(f"{name}: orbit sizes {sorted(sizes)} under {n_el} elements")
    if name.startswith("ring12"):
        assert len(sizes) > 1  # orbits with and without stabilisers


def test_c_refusals_that_need_no_device():
    L = _lib()
    err = lambda: L.ls_amd_last_error().decode()  # noqa: E731
    h = C.c_void_p()
    reps = (C.c_uint64 * 4)()
    spin = D.loadConfigFromDict(E.ring(8, 4, 0))
    assert L.ls_amd_amp_create(None, spin.payload, reps, 4, None) == -1 and "NULL" in err()
    assert L.ls_amd_amp_create(C.byref(h), None, reps, 4, None) == -1 and "NULL" in err()
    assert L.ls_amd_amp_create(C.byref(h), spin.payload, None, 4, None) == -1 and "NULL" in err()
    assert L.ls_amd_amp_create(C.byref(h), spin.payload, reps, -1, None) == -1 and "negative count" in err()
    assert L.ls_amd_amp_create(C.byref(h), spin.payload, reps, 0xffffffff, None) == -1 and "2^32 - 1" in err()
    assert h.value is None
    assert L.ls_amd_amp_amplitudes(None, 0, 1, 1, reps, reps, 1, 0, reps, 1, 0, None) == -1 and "NULL" in err()
    assert L.ls_amd_amp_state_info(None, 1, reps, None, None, None, None, None) == -1 and "NULL" in err()
    assert L.ls_amd_amp_orbit_states(None, 1, reps, reps, reps, None) == -1 and "NULL" in err()
    assert L.ls_amd_amp_check(None, None) == -1 and L.ls_amd_amp_num_elements(None) == -1
    assert L.ls_amd_amp_kernel_name(None) is None
    L.ls_amd_amp_destroy(None)


def test_python_refusals_that_need_no_device():
    import torch

    cfg = E.ring(12, 6, 3)
    basis = D.loadConfigFromDict(cfg)
    reps = _reps(E.tables(cfg)[2])
    n = reps.numel()
    states = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(D.LsAmdError, match="one partition"):
        D.SectorAmplitudes(basis, [reps, reps])
    with pytest.raises(D.LsAmdError, match="one partition"):
        D.amplitudes(basis, [reps, reps], torch.zeros(n, dtype=torch.complex128), states)
    with pytest.raises(D.LsAmdError, match="one partition"):
        D.sample_states(basis, [reps, reps], torch.zeros(n, dtype=torch.complex128), 10)
    with pytest.raises(D.LsAmdError, match="int64"):
        D.SectorAmplitudes(basis, reps.double())
    sa = D.SectorAmplitudes(basis, [reps])
    assert sa.complex_characters
    with pytest.raises(D.LsAmdError, match=f"{n - 1} rows, the sector has {n} representatives"):
        sa.amplitudes(states, torch.zeros(n - 1, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match=f"{n - 1} rows"):
        sa.amplitudes(states, torch.zeros(n - 1, 2, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match=f"vector of {n} elements or an"):
        sa.amplitudes(states, torch.zeros(n, 2, 2, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match=r"K = 65 columns, outside \[1, 64\]"):
        sa.amplitudes(states, torch.zeros(n, 65, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match=r"K = 0 columns"):
        sa.amplitudes(states, torch.zeros(n, 0, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match="neither float64 nor complex128"):
        sa.amplitudes(states, torch.zeros(n, dtype=torch.float32))
    with pytest.raises(D.LsAmdError, match="there is no CPU path"):
        sa.amplitudes(states, torch.zeros(n, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match="device tensor"):
        sa.amplitudes(states, np.zeros(n))
    # the words: a 1-D int64 tensor (checked after psi, before any device work)
    for bad, what in ((states.to(torch.int32), "int64"), (states.reshape(5, 1), "1-D"), ([1, 2, 3], "int64")):
        with pytest.raises(D.LsAmdError, match=what):
            sa.state_info(bad)
    with pytest.raises(D.LsAmdError, match="there is no CPU path"):
        sa.state_info(states)
    with pytest.raises(D.LsAmdError, match="elements must be a 1-D int32"):
        sa.orbit_states(states, states)
    with pytest.raises(D.LsAmdError, match="there is no CPU path"):
        sa.orbit_states(states, states.to(torch.int32))
    # sampling
    with pytest.raises(D.LsAmdError, match="non-negative int"):
        sa.sample(torch.zeros(n, dtype=torch.complex128), -1)
    with pytest.raises(D.LsAmdError, match="non-negative int"):
        sa.sample(torch.zeros(n, dtype=torch.complex128), 2.5)
    with pytest.raises(D.LsAmdError, match="seed must be an int"):
        sa.sample(torch.zeros(n, dtype=torch.complex128), 4, seed="x")
    with pytest.raises(D.LsAmdError, match="one vector"):
        sa.sample(torch.zeros(n, 2, dtype=torch.complex128), 4)
    with pytest.raises(D.LsAmdError, match="there is no CPU path"):
        sa.sample(torch.zeros(n, dtype=torch.complex128), 4)
    assert sa.h is None  # nothing above asked for a device
    sa.destroy()

