"""The fermionic cross-sector kernels in the compiler's resource report: csrc/k_cross_fermi.hip holds exactly the 10 instantiations
of k_cross_pull with the FERMI switch on (the family the plans call k_cross_pull_fermi) and nothing else, none spills, and each one
costs no more LDS and no occupancy next to its twin without permutation signs in csrc/k_cross.hip (the same template,
csrc/k_cross_t.hpp, with the switch off)."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-matvec_amd", "csrc")


@pytest.fixture(scope="module")
def stats():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    return kernel_resources.resources(source="k_cross_fermi.hip"), kernel_resources.resources(source="k_cross.hip")


PREFIX = "_Z12k_cross_pullI"  # k_cross_pull<W, PM1, CPLX, REAL, FERMI>: W = j (uint32_t) / m (uint64_t), then four bools


def _kinds(stats, fermi):
    """{(W, PM1, CPLX, REAL): resources} of the k_cross_pull instantiations with FERMI == fermi"""
    out = {}
    for name, v in stats.items():
        m = re.match(re.escape(PREFIX) + r"([jm])Lb([01])ELb([01])ELb([01])ELb([01])EE", name)
        if m and int(m.group(5)) == fermi:
            out[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))] = v
    return out


# {32-, 64-bit words} x {f64 | c128 x {+-1, complex characters} x {real, complex terms}}
KINDS = {(w, *k) for w in "jm" for k in ((1, 0, 1), (1, 1, 1), (1, 1, 0), (0, 1, 1), (0, 1, 0))}


def test_the_unit_holds_the_ten_kernels_and_nothing_else(stats):
    fermi, spin = stats
    assert len(fermi) == 10, sorted(fermi)
    assert set(_kinds(fermi, 1)) == KINDS and not _kinds(fermi, 0), sorted(fermi)
    # ... and the unit without permutation signs holds none of them
    assert len(spin) == 10 and set(_kinds(spin, 0)) == KINDS and not _kinds(spin, 1), sorted(spin)


def test_no_scratch_and_the_twins_lds_and_occupancy(stats):
    fermi, spin = stats
    f, s = _kinds(fermi, 1), _kinds(spin, 0)
    assert set(f) == set(s) == KINDS
    for kind, v in sorted(f.items()):
        twin = s[kind]
        print(f"k_cross_pull<{kind}, FERMI>: {v}   twin: {twin}")
        assert v["scratch"] == 0, (kind, v)
        assert v["lds"] == twin["lds"], (kind, v, twin)
        assert v["occ"] >= twin["occ"], (kind, v, twin)
        # the admitted-blocks rule of test_cross_kernels_in_the_resource_report: the SGPR file must not admit fewer blocks than LDS
        # and VGPRs
        by_sgpr = 800 // (-(-v["sgpr"] // 16) * 16 + 16)
        by_lds = (160 * 1024) // v["lds"] if v["lds"] else 8
        assert by_sgpr >= min(by_lds, v["occ"], 8), (kind, v)


def test_the_units_keep_their_kernels_apart():
    """the signed instantiations live in their own unit: k_cross.hip routes a fermionic source there instead of refusing it,
    k_fermi.hip knows nothing of the cross kernel, and the Makefile builds the new unit with its header dependencies"""
    cross = open(os.path.join(CSRC, "k_cross.hip")).read()
    assert "if (src.fermi) return lsk_cross_fermi_pull(" in cross and "REAL, true>" not in cross
    assert "k_cross" not in open(os.path.join(CSRC, "k_fermi.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^KSRC :=.*\bk_cross_fermi\.hip\b", mk, flags=re.M)
    assert re.search(r"^k_cross\.o k_cross_fermi\.o.*: k_cross_t\.hpp lsk_fermi\.hpp$", mk, flags=re.M)
