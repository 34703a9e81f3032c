#!/usr/bin/env python3
"""The cost of the fermionic permutation sign in the indexed pull kernel (k_pull_t): a spinless t-V ring of L modes at N = L / 2
(t = 1, V = 1, closing bond included) in the dihedral trivial sector, against the same ring as a spin chain -- heisenberg_chain_L_symm
WITHOUT spin_inversion, whose exchange terms connect the same states as the hopping.  Both run the element loop of K4 mode 0 over
the 2 L dihedral elements (LS_AMD_K4=general for the spins; projected fermionic bases always take it), so they share the sector,
the partners and the loop, and only the sign differs.  The spin chain in its default K4 mode (3: run-pruned orbit minimum) is
measured for context.  One JSON line per case: ms per matvec (HIP events inside the library, f64, fused path, one partition);
the fermion line carries its ratio to the spin chain under `general` (estimate: <= 1.3)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import config  # noqa: E402


def spin_chain(L):
    cfg = config.heisenberg_chain_config(L, symm=True)
    del cfg["basis"]["spin_inversion"]
    return cfg


def tv_ring(L, N, t=1.0, V=1.0):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    dihedral = [{"permutation": [(i + 1) % L for i in range(L)], "sector": 0}, {"permutation": [L - 1 - i for i in range(L)], "sector": 0}]
    terms = [{"expression": f"{-t!r} × c†₀ c₁", "sites": bonds}, {"expression": f"{-t!r} × c†₁ c₀", "sites": bonds},
             {"expression": f"{V!r} × n₀ n₁", "sites": bonds}]
    return {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": N, "symmetries": dihedral},
            "hamiltonian": {"terms": terms}}


def measure(cfg, k4, steps, warmup):
    """(states, kernel, ms per matvec, y) with LS_AMD_K4 = k4 (None: the default mode) for enumeration and plan"""
    if k4:
        os.environ["LS_AMD_K4"] = k4
    else:
        os.environ.pop("LS_AMD_K4", None)
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    n = int(reps[0].numel())
    x = [D.fillRandom(reps[0], 42, torch.float64)]
    y = [torch.zeros_like(x[0])]
    pl = D.MatvecPlan(h, reps, torch.float64)
    kernel = pl.kernel
    pl.enable_timing(256)
    for _ in range(warmup):
        pl.matvec(x, y)
    pl.kernel_times_ms()
    for _ in range(steps):
        pl.matvec(x, y, check=False)
    pl.check()
    ks = pl.kernel_times_ms()
    ms = sum(ks) / len(ks)
    out = y[0].cpu()
    pl.destroy()
    del x, y, reps, basis, h
    torch.cuda.empty_cache()
    os.environ.pop("LS_AMD_K4", None)
    return n, kernel, ms, out


ap = argparse.ArgumentParser()
ap.add_argument("--sites", type=int, default=36)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
L, N = args.sites, args.sites // 2
if not torch.cuda.is_available():
    raise SystemExit("fermion_symm_bench.py measures on a GPU; none is visible")
torch.cuda.set_device(0)

n_s, k_s, ms_s, y_s = measure(spin_chain(L), "general", args.steps, args.warmup)
print(json.dumps({"case": f"xxz_chain_{L}_symm_no_inversion", "k4": "general (mode 0)", "states": n_s, "kernel": k_s,
                  "ms_per_matvec": ms_s}), flush=True)
n_3, k_3, ms_3, y_3 = measure(spin_chain(L), None, args.steps, args.warmup)
diff = float((y_3 - y_s).abs().max() / y_s.abs().max())
print(json.dumps({"case": f"xxz_chain_{L}_symm_no_inversion", "k4": "default (mode 3)", "states": n_3, "kernel": k_3,
                  "ms_per_matvec": ms_3, "ratio_to_general": ms_3 / ms_s, "max_rel_diff_vs_general": diff}), flush=True)
n_f, k_f, ms_f, _ = measure(tv_ring(L, N), "general", args.steps, args.warmup)
print(json.dumps({"case": f"tV_ring_{L}_N{N}_dihedral_k0", "k4": "fermionic (mode 0, signed)", "states": n_f, "kernel": k_f,
                  "ms_per_matvec": ms_f, "ratio_to_spin_general": ms_f / ms_s, "target_ratio": 1.3,
                  "meets_target": ms_f / ms_s <= 1.3}), flush=True)
