#!/usr/bin/env python3
"""Block matvec (MatvecPlan.matvec_block) against the single-vector plan on the same vectors.  One JSON line per
(model, dtype, layout, K, path): ms per block call and per column (torch events around the call, median of --steps), the
single-vector ms per column on the same plan, and their ratio.  Paths: `auto` (the documented rule), `kernel` (the block kernel
forced, where one applies) and `columns`.  Models:
  chain_36_symm, chain_40_symm   projected (resolve + k_pull_gather_blk); chain_40_symm at f64, K <= 8, if the HBM has room
  hop_30                          non-Hermitian sigma+ sigma- ring + zz, 30 sites at weight 15 (k_direct)
  hubbard_chain_16_pairhop        hubbard_chain_16 + a pair hopping 0 <-> 8: not species-separable (k_direct, product index)
  chain_32_generic, chain_32      LS_AMD_ROW_KERNEL=generic (k_direct) and the staged k_chain_t
usage: block_bench.py [--models a,b] [--ks 1,2,4,8,16] [--layouts interleaved,colmajor] [--dtypes f64,c128] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import config  # noqa: E402


def model(name):
    if name in ("chain_36_symm", "chain_40_symm"):
        return config.heisenberg_chain_config(int(name[6:8]), symm=True), {}
    if name == "hop_30":
        bonds = [[i, (i + 1) % 30] for i in range(30)]
        return {"basis": {"number_spins": 30, "hamming_weight": 15, "symmetries": []},
                "hamiltonian": {"terms": [{"expression": "σ⁺₀ σ⁻₁", "sites": bonds}, {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]}}, {}
    if name == "hubbard_chain_16_pairhop":
        cfg = config.hubbard_config(16, [(i, (i + 1) % 16) for i in range(16)], t=1.0, U=4.0)
        cfg["hamiltonian"]["terms"] += [{"expression": "0.5 × c†₀↑ c†₀↓ c₁↓ c₁↑", "sites": [[0, 8]]},
                                        {"expression": "0.5 × c†₁↑ c†₁↓ c₀↓ c₀↑", "sites": [[0, 8]]}]
        return cfg, {}
    if name == "chain_32_generic":
        return config.heisenberg_chain_config(32), {"LS_AMD_ROW_KERNEL": "generic"}
    if name == "chain_32":
        return config.heisenberg_chain_config(32), {}
    raise SystemExit(f"unknown model {name}")


def timed(fn, steps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def block(n, K, dtype, layout):
    if layout == "interleaved":
        return torch.empty((n, K), dtype=dtype, device="cuda")
    return torch.empty((K, n), dtype=dtype, device="cuda").t()


ap = argparse.ArgumentParser()
ap.add_argument("--models", default="chain_36_symm,hop_30,hubbard_chain_16_pairhop,chain_32_generic,chain_32,chain_40_symm")
ap.add_argument("--ks", default="1,2,4,8,16")
ap.add_argument("--layouts", default="interleaved,colmajor")
ap.add_argument("--dtypes", default="f64,c128")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--out", default=None, help="append the JSON lines here as well")
args = ap.parse_args()
torch.cuda.set_device(0)
out = open(args.out, "a") if args.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


for name in args.models.split(","):
    cfg, env = model(name)
    for k, v in env.items():
        os.environ[k] = v
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    n = reps[0].numel()
    for dt in args.dtypes.split(","):
        dtype = torch.complex128 if dt == "c128" else torch.float64
        big = name == "chain_40_symm" or n > 400_000_000
        if big and dt == "c128":
            continue
        pl = D.MatvecPlan(h, reps, dtype)
        x1 = torch.rand(n, dtype=dtype, device="cuda") - 0.5
        y1 = torch.empty_like(x1)
        single = timed(lambda: pl.matvec([x1], [y1], check=False), args.steps)
        pl.check()
        del x1, y1
        for layout in args.layouts.split(","):
            for K in [int(k) for k in args.ks.split(",")]:
                if big and (K > 8 or layout != "interleaved"):
                    continue
                free, _ = torch.cuda.mem_get_info()
                need = 2 * n * K * (16 if dt == "c128" else 8)
                if need > 0.8 * free:
                    emit({"model": name, "dtype": dt, "layout": layout, "K": K, "skipped": f"needs {need / 1e9:.1f} GB, {free / 1e9:.1f} GB free"})
                    continue
                x = block(n, K, dtype, layout)
                x.copy_(torch.rand((n, K), dtype=torch.float64, device="cuda").to(dtype) - 0.5)
                y = block(n, K, dtype, layout)
                for mode in ("auto", "kernel", "columns"):
                    os.environ["LS_AMD_BLOCK"] = mode
                    path = pl.block_kernel(K)
                    if mode == "kernel" and path == "columns":
                        continue
                    ms = timed(lambda: pl.matvec_block(x, y, check=False), args.steps)
                    pl.check()
                    emit({"model": name, "N": n, "kernel": pl.kernel, "dtype": dt, "layout": layout, "K": K, "mode": mode, "path": path,
                          "ms_block": round(ms, 3), "ms_per_column": round(ms / K, 3), "ms_single": round(single, 3),
                          "per_column_vs_single": round(ms / K / single, 3)})
                os.environ.pop("LS_AMD_BLOCK", None)
                del x, y
        pl.destroy()
        torch.cuda.empty_cache()
    for k in env:
        os.environ.pop(k, None)
