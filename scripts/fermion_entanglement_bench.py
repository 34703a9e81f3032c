#!/usr/bin/env python3
"""What one fermionic sector-state expansion costs, and what the two signs add to the spin kernel: a vector on the representatives
of a translation sector (k = 0) expanded by FermionSectorExpansion (k_expand_push_fermi) for
    tv        the t-V ring of --modes modes (28) at half filling -- the spinless layout, closed-form rotation signs,
    hubbard   the Hubbard ring of --modes / 2 sites at (N/2 up, N/2 down) -- the product layout, lifted rotations,
and by SectorExpansion (k_expand_push) for
    spin      the Heisenberg ring of --modes sites at half filling: as many output elements as tv, the same group order,
each for A = the low half of the sites, A = every other site (the bipartition sign is constant per block on the first and varies on
the second) and A = everything (unproject).  Next to each expansion: a hipMemsetAsync over the same buffer (the write floor; the
expansion clears its blocks with one, so its own time contains it) and one matrix-free matvec of H in the same sector.  Everything
alternates inside one process after a warm-up and is timed by device events; medians over --steps.  One JSON line per
(model, dtype, A), appended to --out; `over_spin` is the ratio of the expansion's time per output element to the spin kernel's for
the same dtype and kind of subsystem.
usage: fermion_entanglement_bench.py [--modes 28] [--steps 5] [--warmup 1] [--dtypes f64,c128] [--out profiles/fermion_entanglement_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import _lib, config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--modes", type=int, default=28)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--dtypes", default="f64,c128")
ap.add_argument("--out", default=None)
args = ap.parse_args()
M = args.modes
assert M % 4 == 0, "--modes: a multiple of 4 (half filling of the ring and of both species of the Hubbard ring)"
torch.cuda.set_device(0)
lib = _lib.load()


def translation(L):
    return [{"permutation": [(i + 1) % L for i in range(L)], "sector": 0}]


def tv_config(L, V=1.0):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    terms = [{"expression": "-1.0 × c†₀ c₁", "sites": bonds}, {"expression": "-1.0 × c†₁ c₀", "sites": bonds},
             {"expression": f"{V!r} × n₀ n₁", "sites": bonds}]
    return {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": L // 2, "symmetries": translation(L)},
            "hamiltonian": {"name": "t-V", "terms": terms}}


def spin_config(L):
    cfg = config.heisenberg_chain_config(L)
    cfg["basis"]["symmetries"] = translation(L)
    return cfg


MODELS = [
    ("spin", f"heisenberg_chain_{M}", spin_config(M), M),
    ("tv", f"tv_ring_{M}", tv_config(M), M),
    ("hubbard", f"hubbard_ring_{M // 2}", config.hubbard_config(M // 2, [(i, (i + 1) % (M // 2)) for i in range(M // 2)],
                                                               symmetries=translation(M // 2)), M // 2),
]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
spin_ns_per_element = {}

for kind, model, cfg, sites_n in MODELS:
    t0 = time.perf_counter()
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    n = int(reps[0].numel())
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    for dt in args.dtypes.split(","):
        dtype = torch.complex128 if dt == "c128" else torch.float64
        elt = 16 if dt == "c128" else 8
        psi = D.fillRandom(reps[0], 1, dtype)
        plan = D.MatvecPlan(h, reps, dtype)
        y = torch.zeros_like(psi)
        for name, sites in (("half", list(range(sites_n // 2))), ("alternate", list(range(0, sites_n, 2))), ("all", None)):
            ex = D.SectorExpansion(basis, reps[0], sites) if kind == "spin" else D.FermionSectorExpansion(basis, reps[0], sites=sites)
            out = torch.empty(ex.total, dtype=dtype, device="cuda")
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def do_expand():
                ex.expand(psi, out=out, max_bytes=None, check=False)

            def do_memset():
                _lib.check(lib.ls_amd_memset(C.c_void_p(out.data_ptr()), 0, ex.total * elt, stream))

            def do_matvec():
                plan.matvec([psi], [y], check=False)

            for _ in range(args.warmup):
                do_expand()
                do_memset()
                do_matvec()
            ex.check()
            plan.check()
            te, tz, tm = [], [], []
            for _ in range(args.steps):  # alternating
                te.append(timed(do_expand))
                tz.append(timed(do_memset))
                tm.append(timed(do_matvec))
            ex.check()
            plan.check()
            do_expand()
            norm_out, norm_psi = float(torch.linalg.vector_norm(out)), float(torch.linalg.vector_norm(psi))
            ms = med(te)
            per_element = ms * 1e6 / ex.total
            if kind == "spin":
                spin_ns_per_element[(dt, name)] = per_element
            rec = {"model": model, "symmetries": "translation", "sector": 0, "dtype": dt, "subsystem": name, "n_representatives": n,
                   "elements": ex.total, "blocks": len(ex.blocks), "group_order": basis.groupOrder(), "kernel": ex.kernel,
                   "steps": args.steps, "warmup": args.warmup, "expand_ms_median": round(ms, 4), "expand_ms_min": round(min(te), 4),
                   "expand_ms_max": round(max(te), 4), "elements_per_s": round(ex.total / (ms * 1e-3), 1),
                   "bytes_written_per_s": round(ex.total * elt / (ms * 1e-3), 1), "ns_per_element": round(per_element, 5),
                   "over_spin": round(per_element / spin_ns_per_element[(dt, name)], 4), "memset_ms_median": round(med(tz), 4),
                   "scatter_ms_median_minus_memset": round(ms - med(tz), 4), "matvec_kernel": plan.kernel,
                   "matvec_ms_median": round(med(tm), 4), "expand_over_matvec": round(ms / med(tm), 4),
                   "norm_defect": abs(norm_out - norm_psi) / norm_psi, "setup_seconds": round(setup_s, 2)}
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            ex.destroy()
            del out
        plan.destroy()
        del psi, y
        torch.cuda.empty_cache()
    del reps, basis, h
