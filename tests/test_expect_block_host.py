"""Block expectation values and finite-temperature static observables, the parts that need no device
(ls_amd_expect_values_block, ExpectationPlan.values_block, evolve.thermal_expectation, evolve.combine_sector_expectations): the ABI
and the build, combine_sector_expectations on fabricated results -- its weights D_s / K_s and its refusals -- and the arguments
thermal_expectation refuses before it asks for a device."""
import os
import re

import numpy as np
import pytest

import cross_sector_reference as X
import distributed_matvec_amd as D
from distributed_matvec_amd import evolve, expectation
from distributed_matvec_amd.evolve import ThermalExpectationResult, combine_sector_expectations, thermal_expectation  # noqa: F401  (the feature under test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-matvec_amd", "csrc")


def test_abi_makefile_and_python_names():
    from distributed_matvec_amd import _lib

    header = open(os.path.join(ROOT, "include", "ls_amd.h"), encoding="utf-8").read()
    L = _lib.load()
    for name in ("ls_amd_expect_values_block", "ls_amd_expect_block_kernel_name"):
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
    make = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    ksrc = re.search(r"^KSRC := (.*)$", make, re.M).group(1).split()
    assert "k_expect_blk.hip" in ksrc and "k_expect_blk_fermi.hip" in ksrc
    assert re.search(r"^k_expect_blk\.o k_expect_blk_fermi\.o k_expect_blk_ablate\.o k_expect_blk_fermi_ablate\.o: "
                     r"k_expect_blk_t\.hpp k_expect_t\.hpp k_corr_t\.hpp k_cross_t\.hpp lsk_fermi\.hpp$", make, re.M)
    # the new units are not fingerprinted: the fingerprints of the existing kernels stay what they were
    isa = open(os.path.join(ROOT, "scripts", "kernel_isa_sha.py"), encoding="utf-8").read()
    assert "k_expect" not in isa
    for name in ("values_block", "block_kernel"):
        assert hasattr(D.ExpectationPlan, name), name
    assert "expectation_values_block" in expectation.__all__ and D.expectation_values_block is expectation.expectation_values_block
    for name in ("thermal_expectation", "combine_sector_expectations", "ThermalExpectationResult"):
        assert name in evolve.__all__ and name in D.__all__ and getattr(D, name) is getattr(evolve, name), name


def test_the_block_kernel_has_no_floating_point_atomics_and_one_chunk_width():
    """the bitwise guarantee of k_expect carries over: the template adds in a fixed order, in registers and plain LDS stores"""
    def code_of(header):
        src = open(os.path.join(CSRC, header), encoding="utf-8").read()
        return "\n".join(line.split("//")[0] for line in src.splitlines())

    code = code_of("k_expect_blk_t.hpp")
    # ... and the headers it takes its stages and constants from
    for header in ("k_expect_blk_t.hpp", "k_expect_t.hpp", "k_corr_t.hpp"):
        assert "atomicAdd" not in code_of(header) and "unsafeAtomicAdd" not in code_of(header), header
    assert re.search(r"constexpr int kExpKC = 8;", code)
    assert "corr_grid(n)" in code and "lsk_corr_sum(" in code
    for unit, fermi in (("k_expect_blk.hip", False), ("k_expect_blk_fermi.hip", True)):
        text = open(os.path.join(CSRC, unit), encoding="utf-8").read()
        assert ("expect_blk_launch<true>" in text) == fermi and ("expect_blk_launch<false>" in text) == (not fermi)
        assert ('"k_expect_blk_fermi"' in text) == fermi


def test_null_plan_is_refused_by_the_library():
    """the entry points answer a NULL plan with a message (no device is touched)"""
    from distributed_matvec_amd import _lib

    L = _lib.load()
    assert L.ls_amd_expect_values_block(None, 1, 2, None, 2, 1, None, None) == -1
    assert b"ls_amd_expect_values_block: NULL plan" in L.ls_amd_last_error()
    assert L.ls_amd_expect_block_kernel_name(None, 1) is None
    assert b"NULL plan" in L.ls_amd_last_error()


def _result(betas, numerator, partition, e1, e2, dimension, e_ref=-3.0):
    betas = np.asarray(betas, dtype=np.float64)
    numerator = np.asarray(numerator, dtype=np.complex128)
    partition, e1, e2 = (np.asarray(a, dtype=np.float64) for a in (partition, e1, e2))
    K = partition.shape[1]
    values, energy, heat, logz, ent = evolve._thermal_derived(betas, numerator.sum(axis=2), partition.sum(axis=1), e1.sum(axis=1), e2.sum(axis=1),
                                                              dimension / K, e_ref)
    return ThermalExpectationResult(betas, numerator, partition, e1, e2, values, energy, heat, logz, ent, dimension, e_ref, (-3.0, 2.0),
                                    np.zeros(len(betas), dtype=np.int64), "k_expect_blk", 0)


def test_combine_sector_expectations_weights_every_sector_by_dimension_over_vectors():
    betas = [0.0, 2.0]
    # one operator; K = 2 (weight 5), K = 1 (weight 7)
    a = _result(betas, [[[1.0 + 2.0j, 3.0]], [[0.5j, -1.0]]], [[2.0, 4.0], [1.0, 0.5]], [[-2.0, -4.0], [-1.5, -0.5]], [[3.0, 5.0], [2.5, 1.0]], 10)
    b = _result(betas, [[[2.0]], [[1.0 - 1.0j]]], [[0.5], [0.25]], [[-0.25], [-0.5]], [[1.0], [1.5]], 7)
    got = combine_sector_expectations([a, b])
    Z = np.array([5.0 * 6.0 + 7.0 * 0.5, 5.0 * 1.5 + 7.0 * 0.25])
    num = np.array([5.0 * (4.0 + 2.0j) + 7.0 * 2.0, 5.0 * (-1.0 + 0.5j) + 7.0 * (1.0 - 1.0j)])
    e1 = np.array([5.0 * -6.0 + 7.0 * -0.25, 5.0 * -2.0 + 7.0 * -0.5])
    e2 = np.array([5.0 * 8.0 + 7.0 * 1.0, 5.0 * 3.5 + 7.0 * 1.5])
    bs = np.array(betas)
    eps = 8 * np.finfo(float).eps
    assert got.values.shape == (2, 1) and np.abs(got.values[:, 0] - num / Z).max() <= eps * np.abs(num / Z).max()
    assert np.abs(got.energy - e1 / Z).max() <= eps * np.abs(e1 / Z).max()
    heat = bs ** 2 * (e2 / Z - (e1 / Z) ** 2)
    assert np.abs(got.specific_heat - heat).max() <= 64 * eps * max(1.0, np.abs(heat).max())
    logz = np.log(Z) - bs * -3.0
    assert np.abs(got.log_partition - logz).max() <= 8 * eps * np.abs(logz).max()
    assert np.abs(got.entropy - (logz + bs * e1 / Z)).max() <= 16 * eps * np.abs(logz).max()
    assert got.dimension == 17 and got.reference_energy == -3.0 and np.array_equal(got.betas, bs)
    # one sector: its own ensemble
    one = combine_sector_expectations([a])
    for name in ("values", "energy", "specific_heat", "log_partition", "entropy"):
        assert np.abs(getattr(one, name) - getattr(a, name)).max() <= 64 * eps * max(1.0, np.abs(getattr(a, name)).max()), name
    # and a combined result combines further, with its dimension as its weight
    again = combine_sector_expectations([combine_sector_expectations([a]), b])
    assert np.abs(again.values - got.values).max() <= 8 * eps * np.abs(got.values).max()
    assert np.abs(again.log_partition - got.log_partition).max() <= 8 * eps * np.abs(got.log_partition).max()


def test_combine_sector_expectations_refusals():
    a = _result([0.0, 1.0], [[[1.0]], [[1.0]]], [[1.0], [1.0]], [[1.0], [1.0]], [[1.0], [1.0]], 3)
    with pytest.raises(ValueError, match="other betas"):
        combine_sector_expectations([a, _result([0.0, 1.5], [[[1.0]], [[1.0]]], [[1.0], [1.0]], [[1.0], [1.0]], [[1.0], [1.0]], 3)])
    with pytest.raises(ValueError, match="other betas"):
        combine_sector_expectations([a, _result([0.0], [[[1.0]]], [[1.0]], [[1.0]], [[1.0]], 3)])
    with pytest.raises(ValueError, match="reference_energy"):
        combine_sector_expectations([a, _result([0.0, 1.0], [[[1.0]], [[1.0]]], [[1.0], [1.0]], [[1.0], [1.0]], [[1.0], [1.0]], 3, e_ref=-2.5)])
    with pytest.raises(ValueError, match="2 operators, result 0 1"):
        combine_sector_expectations([a, _result([0.0, 1.0], [[[1.0], [2.0]], [[1.0], [2.0]]], [[1.0], [1.0]], [[1.0], [1.0]], [[1.0], [1.0]], 3)])
    with pytest.raises(ValueError, match="no results"):
        combine_sector_expectations([])


def _heisenberg(basis_cfg, L, hermitian=True):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    terms = [{"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds}, {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]
    if not hermitian:
        terms = [{"expression": "σ⁺₀ σ⁻₁", "sites": bonds}]
    return {"basis": basis_cfg["basis"], "hamiltonian": {"name": "H", "terms": terms}}


def test_thermal_expectation_refuses_bad_arguments_before_any_device_work():
    """this machine may have no device at all: every refusal below is raised before one is asked for"""
    import torch

    cfg = _heisenberg(X.ring(8, 4, 0), 8)
    zz = {"terms": [{"expression": "σᶻ₀ σᶻ₁", "sites": [[0, 1]]}]}
    cfg["observables"] = [zz]
    for betas in ([-0.1], [float("nan")], [0.0, float("inf")], [1.0, 0.5], [], [[0.0, 1.0]], "cold"):
        with pytest.raises(ValueError, match="betas"):
            thermal_expectation(cfg, [zz], betas)
    for nv in (0, 65, 2.5):
        with pytest.raises(ValueError, match="num_vectors"):
            thermal_expectation(cfg, [zz], [0.5], num_vectors=nv)
    with pytest.raises(ValueError, match="bounds"):
        thermal_expectation(cfg, [zz], [0.5], bounds=(1.0, 1.0))
    with pytest.raises(ValueError, match="eps"):
        thermal_expectation(cfg, [zz], [0.5], eps=0.0)
    with pytest.raises(ValueError, match="reference_energy"):
        thermal_expectation(cfg, [zz], [0.5], reference_energy=float("nan"))
    with pytest.raises(ValueError, match="the config has 1 observables"):
        thermal_expectation(cfg, [0, 1], [0.5])
    with pytest.raises(D.LsAmdError, match="neither an Operator"):
        thermal_expectation(cfg, ["σᶻ₀ σᶻ₁"], [0.5])
    with pytest.raises(ValueError, match="no operators"):
        thermal_expectation(cfg, [], [0.5])
    with pytest.raises(D.LsAmdError, match="one-partition"):
        thermal_expectation(cfg, [zz], [0.5], vectors=[np.zeros((10, 2))])
    with pytest.raises(D.LsAmdError, match=r"\(D, K\) block"):
        thermal_expectation(cfg, [zz], [0.5], vectors=torch.zeros(10, dtype=torch.float64))
    with pytest.raises(D.LsAmdError, match=r"\(D, K\) block"):
        thermal_expectation(cfg, [zz], [0.5], vectors=torch.zeros((10, 65), dtype=torch.float64))
    with pytest.raises(D.LsAmdError, match="device tensor"):
        thermal_expectation(cfg, [zz], [0.5], vectors=torch.zeros((10, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="not Hermitian"):
        thermal_expectation(_heisenberg(X.ring(8, 4, 0), 8, hermitian=False), [zz], [0.5])
    # float64 on request where the sector has complex characters
    with pytest.raises(D.LsAmdError, match="torch.float64 cannot be honoured: the characters of the sector are complex"):
        thermal_expectation(_heisenberg(X.ring(8, 4, 3), 8), [zz], [0.5], dtype=torch.float64)
    with pytest.raises(ValueError, match="neither torch.float64 nor torch.complex128"):
        thermal_expectation(cfg, [zz], [0.5], dtype=torch.float32)
