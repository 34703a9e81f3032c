#!/usr/bin/env python3
"""The cost of the fermionic permutation sign in the indexed pull kernel (k_pull_t): a spinless t-V ring of L modes at N = L / 2
(t = 1, V = 1, closing bond included) in the dihedral trivial sector, against the same ring as a spin chain -- heisenberg_chain_L_symm
WITHOUT spin_inversion, whose exchange terms connect the same states as the hopping.  Both run the element loop of K4 mode 0 over
the 2 L dihedral elements (LS_AMD_K4=general for the spins; projected fermionic bases always take it), so they share the sector,
the partners and the loop, and only the sign differs.  The spin chain in its default K4 mode (3: run-pruned orbit minimum) is
measured for context.  One JSON line per case: ms per matvec (HIP events inside the library, f64, fused path, one partition);
the fermion line carries its ratio to the spin chain under `general` (estimate: <= 1.3).

--spinful L measures the lifted ring elements of a projected spinful basis instead: the Hubbard ring of L sites at half filling in
the dihedral trivial sector (no flip), (a) as the spinless basis on the 2 L modes with the lifted generators and the same terms --
every element a network with one sign-table load per particle, what the library did before spinful sectors existed -- (b) as the
(L/2, L/2) spinful basis, whose lifted rotations and reflections have closed forms, and (c) as (b) with LS_AMD_FERMI_LIFT=0, which
keeps the network + table form on the spinful basis.  The sectors differ in size, so the figure is ns per matvec and ROW; every case
is built and measured --repeats times (each: warm-up, then --steps timed matvecs) and reports median, min and max.  With
--enumerate L2 the enumeration of the (L2/2, L2/2) sector with dihedral x flip is timed as well."""
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


def lifted_dihedral(L):
    rot, rev = [(i + 1) % L for i in range(L)], [L - 1 - i for i in range(L)]
    return [{"permutation": p + [v + L for v in p], "sector": 0} for p in (rot, rev)]


def hubbard_on_modes(L, t=1.0, U=4.0):
    """config.hubbard_config's ring written for a spinless basis on 2 L modes (mode i = (i, up), mode i + L = (i, down)): the same
    compiled terms, since the Jordan-Wigner order of the modes is the same"""
    bonds = [[i + o, (i + 1) % L + o] for o in (0, L) for i in range(L)]
    terms = [{"expression": f"{-t!r} × c†₀ c₁", "sites": bonds}, {"expression": f"{-t!r} × c†₁ c₀", "sites": bonds},
             {"expression": f"{U!r} × n₀ n₁", "sites": [[i, i + L] for i in range(L)]}]
    return {"basis": {"particle": "spinless-fermion", "number_sites": 2 * L, "number_particles": 2 * (L // 2), "symmetries": lifted_dihedral(L)},
            "hamiltonian": {"terms": terms}}


def hubbard_spinful(L, flip=None):
    syms = [{"permutation": [(i + 1) % L for i in range(L)], "sector": 0}, {"permutation": [L - 1 - i for i in range(L)], "sector": 0}]
    return config.hubbard_config(L, [[i, (i + 1) % L] for i in range(L)], symmetries=syms, spin_flip=flip)


def timed_enumeration(cfg):
    import time

    basis, _ = D.loadConfigFromDict(cfg, hamiltonian=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps, _ = D.enumerateStates(basis, 1)
    torch.cuda.synchronize()
    return int(reps[0].numel()), (time.perf_counter() - t0) * 1e3


def spinful_cases(L, steps, warmup, repeats, enum_sites):
    import statistics

    rows = {}
    for case, cfg, lift in ((f"hubbard_ring_{L}_as_spinless_{2 * L}_modes_dihedral_k0", hubbard_on_modes(L), None),
                            (f"hubbard_ring_{L}_spinful_{L // 2}_{L // 2}_dihedral_k0", hubbard_spinful(L), None),
                            (f"hubbard_ring_{L}_spinful_{L // 2}_{L // 2}_dihedral_k0", hubbard_spinful(L), "0")):
        if lift is not None:
            os.environ["LS_AMD_FERMI_LIFT"] = lift
        runs = [measure(cfg, None, steps, warmup) for _ in range(repeats)]
        n_rows, enum_ms = timed_enumeration(cfg)
        os.environ.pop("LS_AMD_FERMI_LIFT", None)
        ms = [r[2] for r in runs]
        k4 = "network + sign table" if (lift == "0" or "spinless" in case) else "lifted closed forms"
        rows[(case, k4)] = statistics.median(ms) * 1e6 / n_rows
        print(json.dumps({"case": case, "k4": k4, "states": n_rows, "kernel": runs[0][1], "repeats": repeats, "steps": steps,
                          "ms_per_matvec_median": statistics.median(ms), "ms_per_matvec_min": min(ms), "ms_per_matvec_max": max(ms),
                          "ns_per_row_median": statistics.median(ms) * 1e6 / n_rows, "ns_per_row_min": min(ms) * 1e6 / n_rows,
                          "ns_per_row_max": max(ms) * 1e6 / n_rows, "enumeration_ms": enum_ms}), flush=True)
    a, b, c = rows.values()  # (insertion order: spinless modes, spinful closed forms, spinful table)
    print(json.dumps({"case": f"hubbard_ring_{L}_dihedral_k0_per_row_ratios", "spinful_closed_over_spinless_modes": b / a,
                      "spinful_closed_over_spinful_table": b / c}), flush=True)
    if enum_sites:
        n, ms = timed_enumeration(hubbard_spinful(enum_sites, flip=1))
        print(json.dumps({"case": f"hubbard_ring_{enum_sites}_spinful_{enum_sites // 2}_{enum_sites // 2}_dihedral_k0_flip_p",
                          "states": n, "enumeration_ms": ms}), flush=True)


ap = argparse.ArgumentParser()
ap.add_argument("--sites", type=int, default=36)
ap.add_argument("--spinful", type=int, default=0, help="sites of the Hubbard ring of the spinful comparison (0: the spinless t-V measurement)")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--enumerate", type=int, default=0, help="with --spinful: also time the enumeration of this many sites at half filling")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
L, N = args.sites, args.sites // 2
if not torch.cuda.is_available():
    raise SystemExit("fermion_symm_bench.py measures on a GPU; none is visible")
torch.cuda.set_device(0)
if args.spinful:
    spinful_cases(args.spinful, args.steps, args.warmup, args.repeats, args.enumerate)
    raise SystemExit(0)

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
