"""The fermionic K4 kernels (csrc/k_fermi.hip) against the spin instantiations they mirror: no spills, the same LDS, no lower
occupancy.  (The hot units' device-function cap is test_host_tables.py's: the fermionic k_pull_t lives in a unit of its own.)"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fermionic_kernels_match_the_spin_resources():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    fermi = kernel_resources.resources(source="k_fermi.hip")
    spin = kernel_resources.resources(source="k_pull.hip")
    pulls = {k: v for k, v in fermi.items() if k.startswith("_Z8k_pull_tI")}
    # fused: {u32, u64} x {PM1 real, PM1 complex, general} on c128 + PM1 real on f64; resolve: {u32, u64} x the three kinds
    assert len(pulls) == 14 and len(fermi) == 16, sorted(fermi)
    for name, v in fermi.items():
        assert v["scratch"] == 0, (name, v)
    for name, v in pulls.items():
        # the spin twin: K4 kind FERMI_PM1 (3) -> PM1 (1), FERMI (4) -> GENERAL (2); the rest of the mangled name is the same
        twin = re.sub(r"^(_Z8k_pull_tI[jm])Li([34])E", lambda m: m.group(1) + "Li" + {"3": "1", "4": "2"}[m.group(2)] + "E", name)
        assert twin != name and twin in spin, name
        assert v["lds"] == spin[twin]["lds"] and v["occ"] >= spin[twin]["occ"], (name, v, spin[twin])
