"""Block cross-sector apply and finite-temperature correlations, the parts that need no device (ls_amd_cross_apply_block,
CrossSectorPlan.apply_block, evolve.thermal_correlation, evolve.combine_sectors): the ABI and the build, combine_sectors on
fabricated results -- its weights D_s / K_s and its refusals -- and the arguments thermal_correlation refuses before it asks for a
device."""
import os
import re

import numpy as np
import pytest

import cross_sector_reference as X
import distributed_matvec_amd as D
from distributed_matvec_amd import evolve
from distributed_matvec_amd.evolve import ThermalCorrelationResult, combine_sectors, thermal_correlation  # noqa: F401  (the feature under test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_makefile_and_python_names():
    from distributed_matvec_amd import _lib

    header = open(os.path.join(ROOT, "include", "ls_amd.h"), encoding="utf-8").read()
    L = _lib.load()
    for name in ("ls_amd_cross_apply_block", "ls_amd_cross_block_kernel_name"):
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
    make = open(os.path.join(ROOT, "distributed-matvec_amd", "csrc", "Makefile"), encoding="utf-8").read()
    ksrc = re.search(r"^KSRC := (.*)$", make, re.M).group(1).split()
    assert "k_cross_blk.hip" in ksrc and "k_cross_blk_fermi.hip" in ksrc
    assert re.search(r"^k_cross_blk\.o k_cross_blk_fermi\.o.*: k_cross_blk_t\.hpp k_cross_t\.hpp lsk_fermi\.hpp$", make, re.M)
    # the new units are not fingerprinted: the fingerprints of the existing kernels stay what they were
    isa = open(os.path.join(ROOT, "scripts", "kernel_isa_sha.py"), encoding="utf-8").read()
    assert "k_cross_blk" not in isa
    assert hasattr(D.CrossSectorPlan, "apply_block") and hasattr(D.CrossSectorPlan, "block_kernel")
    for name in ("thermal_correlation", "combine_sectors", "ThermalCorrelationResult"):
        assert name in evolve.__all__ and name in D.__all__ and getattr(D, name) is getattr(evolve, name), name


def test_null_plan_is_refused_by_the_library():
    """the entry points answer a NULL plan with a message (no device is touched)"""
    from distributed_matvec_amd import _lib

    L = _lib.load()
    assert L.ls_amd_cross_apply_block(None, 1, None, 1, 0, None, 1, 0, None) == -1
    assert b"NULL plan" in L.ls_amd_last_error()
    assert L.ls_amd_cross_block_kernel_name(None, 1) is None
    assert b"NULL plan" in L.ls_amd_last_error()


def _result(times, numerator, partition, dimension, e_ref=-3.0):
    numerator = np.asarray(numerator, dtype=np.complex128)
    partition = np.asarray(partition, dtype=np.float64)
    return ThermalCorrelationResult(np.asarray(times, dtype=np.float64), numerator, partition, numerator.sum(axis=1) / partition.sum(),
                                    dimension, e_ref, (-3.0, 2.0), np.zeros(len(times), dtype=np.int64), "k_cross_pull_blk", 0)


def test_combine_sectors_weights_every_sector_by_dimension_over_vectors():
    times = [0.0, 1.0]
    a = _result(times, [[1.0 + 2.0j, 3.0], [0.5j, -1.0]], [2.0, 4.0], 10)           # K = 2: weight 5
    b = _result(times, [[2.0], [1.0 - 1.0j]], [0.5], 7)                               # K = 1: weight 7
    c = _result(times, [[1.0, 1.0, 1.0j, 0.0], [0.0, 2.0, 0.0, 0.0]], [1.0, 1.0, 2.0, 4.0], 6)  # K = 4: weight 1.5
    den = 5.0 * 6.0 + 7.0 * 0.5 + 1.5 * 8.0
    want = np.array([5.0 * (4.0 + 2.0j) + 7.0 * 2.0 + 1.5 * (2.0 + 1.0j), 5.0 * (-1.0 + 0.5j) + 7.0 * (1.0 - 1.0j) + 1.5 * 2.0]) / den
    got = combine_sectors([a, b, c])
    assert got.dtype == np.complex128 and got.shape == (2,)
    assert np.abs(got - want).max() <= 4 * np.finfo(float).eps * np.abs(want).max()
    # one sector: its own correlation
    assert np.abs(combine_sectors([a]) - a.correlation).max() <= 4 * np.finfo(float).eps * np.abs(a.correlation).max()
    # a whole basis in every sector (K = D): the plain sum of numerators over the plain sum of partitions
    d = _result(times, [[1.0, 2.0], [3.0, 4.0]], [1.0, 3.0], 2)
    e = _result(times, [[5.0], [6.0]], [2.0], 1)
    assert np.allclose(combine_sectors([d, e]), np.array([8.0, 13.0]) / 6.0, rtol=1e-15, atol=0)


def test_combine_sectors_refusals():
    a = _result([0.0, 1.0], [[1.0], [1.0]], [1.0], 3)
    with pytest.raises(ValueError, match="other times"):
        combine_sectors([a, _result([0.0, 1.5], [[1.0], [1.0]], [1.0], 3)])
    with pytest.raises(ValueError, match="other times"):
        combine_sectors([a, _result([0.0], [[1.0]], [1.0], 3)])
    with pytest.raises(ValueError, match="reference_energy"):
        combine_sectors([a, _result([0.0, 1.0], [[1.0], [1.0]], [1.0], 3, e_ref=-2.5)])
    with pytest.raises(ValueError, match="no results"):
        combine_sectors([])


def _heisenberg(basis_cfg, L, hermitian=True):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    terms = [{"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds}, {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]
    if not hermitian:
        terms = [{"expression": "σ⁺₀ σ⁻₁", "sites": bonds}]
    return {"basis": basis_cfg["basis"], "hamiltonian": {"name": "H", "terms": terms}}


def test_thermal_correlation_refuses_bad_arguments_before_any_device_work():
    """this machine may have no device at all: every refusal below is raised before one is asked for"""
    src, dst, op = X.ring(8, 4, 0), X.ring(8, 4, 3), X.sz_q(8, 3)
    cfg = _heisenberg(src, 8)
    cfg["observables"] = [op]
    ok = dict(beta=0.5, times=[0.0, 1.0], target=dst)
    for beta in (-0.1, float("nan"), float("inf"), "cold"):
        with pytest.raises(ValueError, match="beta"):
            thermal_correlation(cfg, 0, **{**ok, "beta": beta})
    for times in ([1.0, 0.5], [], [0.0, float("inf")], [[0.0, 1.0]]):
        with pytest.raises(ValueError, match="times"):
            thermal_correlation(cfg, 0, **{**ok, "times": times})
    for nv in (0, 65, 2.5):
        with pytest.raises(ValueError, match="num_vectors"):
            thermal_correlation(cfg, 0, num_vectors=nv, **ok)
    with pytest.raises(ValueError, match="bounds"):
        thermal_correlation(cfg, 0, bounds=(1.0, 1.0), **ok)
    with pytest.raises(ValueError, match="eps"):
        thermal_correlation(cfg, 0, eps=0.0, **ok)
    with pytest.raises(ValueError, match="reference_energy"):
        thermal_correlation(cfg, 0, reference_energy=float("nan"), **ok)
    with pytest.raises(ValueError, match="none of 'same', 'restrict', 'project'"):
        thermal_correlation(cfg, 0, groups="subgroup", **ok)
    with pytest.raises(ValueError, match="the config has 1 observables"):
        thermal_correlation(cfg, 1, **ok)
    with pytest.raises(ValueError, match="api.Operator"):
        thermal_correlation(cfg, "S^z_q", **ok)
    with pytest.raises(D.LsAmdError, match="one-partition"):
        thermal_correlation(cfg, 0, vectors=[np.zeros((10, 2))], **ok)
    import torch

    with pytest.raises(D.LsAmdError, match=r"\(D_s, K\) block"):
        thermal_correlation(cfg, 0, vectors=torch.zeros(10, dtype=torch.complex128), **ok)
    with pytest.raises(D.LsAmdError, match=r"\(D_s, K\) block"):
        thermal_correlation(cfg, 0, vectors=torch.zeros((10, 65), dtype=torch.complex128), **ok)
    with pytest.raises(D.LsAmdError, match="device tensor"):
        thermal_correlation(cfg, 0, vectors=torch.zeros((10, 2), dtype=torch.complex128), **ok)
    bad = _heisenberg(src, 8, hermitian=False)
    bad["observables"] = [op]
    with pytest.raises(ValueError, match="not Hermitian"):
        thermal_correlation(bad, 0, **ok)
    # an operator that does not map the source sector into the target's: the covariance check names the generator
    with pytest.raises(D.LsAmdError, match="generator 0"):
        thermal_correlation(cfg, 0, **{**ok, "target": X.ring(8, 4, 2)})
