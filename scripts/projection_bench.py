#!/usr/bin/env python3
"""What projecting a full-basis vector into a symmetry sector costs, next to the expansion of the same sector: SectorProjection
(k_project_pull / k_project_pull_fermi, a gathered load per image) against SectorExpansion / FermionSectorExpansion with A =
everything (k_expand_push / k_expand_push_fermi, a scattered store per image; its time contains the clear of the buffer) -- the same
element applications and ranks on both sides.  Sectors (translation, k = 0):
    spin   the Heisenberg ring of --sites sites at half filling (32: 18.8 M representatives, F = 601 M),
    tv     the t-V ring of --modes modes at half filling (28: 1.43 M representatives, F = 40.1 M).
For f64 and c128: one vector (K = 1), and K = 8 columns as an interleaved (F, 8) block, as a column-major block and as 8 single
columns one after another.  Timed by device events after --warmup runs; min, median and max of --steps runs.  A configuration whose
blocks would not fit --max-gib of device memory is recorded as skipped, not measured.  One JSON line per (model, dtype), appended
to --out.
usage: projection_bench.py [--sites 32] [--modes 28] [--steps 3] [--warmup 1] [--dtypes f64,c128] [--models spin,tv] [--max-gib 160]
                           [--out profiles/projection_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sites", type=int, default=32)
ap.add_argument("--modes", type=int, default=28)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--dtypes", default="f64,c128")
ap.add_argument("--models", default="spin,tv")
ap.add_argument("--max-gib", type=float, default=160.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.cuda.set_device(0)
K = 8


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


MODELS = {"spin": (f"heisenberg_chain_{args.sites}", lambda: spin_config(args.sites)), "tv": (f"tv_ring_{args.modes}", lambda: tv_config(args.modes))}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(fn, check):
    for _ in range(args.warmup):
        fn()
    check()
    t = sorted(timed(fn) for _ in range(args.steps))
    check()
    return {"min": round(t[0], 4), "median": round(t[len(t) // 2], 4), "max": round(t[-1], 4)}


def fill(t, seed):
    """seeded uniform values in [-0.5, 0.5) in place (real and imaginary part alike)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    v = torch.view_as_real(t) if t.is_complex() else t
    v.uniform_(-0.5, 0.5, generator=g)
    return t


for kind in args.models.split(","):
    model, make = MODELS[kind]
    t0 = time.perf_counter()
    basis = D.loadConfigFromDict({"basis": make()["basis"]})
    reps = D.enumerateStates(basis, 1)[0][0]
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    n = int(reps.numel())
    pj = D.SectorProjection(basis, reps)
    ex = D.SectorExpansion(basis, reps, None) if kind == "spin" else D.FermionSectorExpansion(basis, reps)
    F = pj.full_size
    assert ex.total == F
    for dt in args.dtypes.split(","):
        dtype = torch.complex128 if dt == "c128" else torch.float64
        elt = 16 if dt == "c128" else 8
        rec = {"model": model, "symmetries": "translation", "sector": 0, "dtype": dt, "n_representatives": n, "full_size": F,
               "group_order": basis.groupOrder(), "kernel": pj.kernel, "expand_kernel": ex.kernel, "steps": args.steps, "warmup": args.warmup,
               "setup_seconds": round(setup_s, 2)}
        # one vector: project next to expand (A = everything) of the same sector
        phi = fill(torch.empty(F, dtype=dtype, device="cuda"), 1)
        psi = torch.empty(n, dtype=dtype, device="cuda")
        rec["project_K1_ms"] = measure(lambda: pj.project(phi, out=psi, check=False), pj.check)
        full = torch.empty(F, dtype=dtype, device="cuda")
        rec["expand_ms"] = measure(lambda: ex.expand(psi, out=full, max_bytes=None, check=False), ex.check)
        # B B+ is a projector: expanding the projection and projecting again returns the same vector
        again = pj.project(full)
        rec["projector_defect"] = float(torch.linalg.vector_norm(again - psi) / torch.linalg.vector_norm(psi))
        rec["project_over_expand"] = round(rec["project_K1_ms"]["median"] / rec["expand_ms"]["median"], 4)
        rec["images_per_s_project"] = round(n * basis.groupOrder() / (rec["project_K1_ms"]["median"] * 1e-3), 1)
        del phi, full, again
        torch.cuda.empty_cache()
        # K = 8 columns
        if F * K * elt / 2 ** 30 > args.max_gib:
            rec["K8"] = f"not measured: the block takes {F * K * elt / 2 ** 30:.1f} GiB, more than --max-gib {args.max_gib}"
        else:
            out = torch.empty(n, K, dtype=dtype, device="cuda")
            block = fill(torch.empty(F, K, dtype=dtype, device="cuda"), 2)
            rec["project_K8_interleaved_ms"] = measure(lambda: pj.project(block, out=out, check=False), pj.check)
            del block
            torch.cuda.empty_cache()
            rows = fill(torch.empty(K, F, dtype=dtype, device="cuda"), 3)
            rec["project_K8_column_major_ms"] = measure(lambda: pj.project(rows.T, out=out, check=False), pj.check)

            def one_by_one():
                for c in range(K):
                    pj.project(rows[c], out=psi, check=False)

            rec["project_K8_single_columns_ms"] = measure(one_by_one, pj.check)
            rec["interleaved_over_single_columns"] = round(rec["project_K8_interleaved_ms"]["median"] / rec["project_K8_single_columns_ms"]["median"], 4)
            del rows, out
            torch.cuda.empty_cache()
        del psi
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    pj.destroy()
    ex.destroy()
    del reps, basis
    torch.cuda.empty_cache()
