#!/usr/bin/env python3
"""What amplitudes on product states and Born sampling cost: SectorAmplitudes (k_amplitude_pull, k_orbit_image) on the Heisenberg ring
of --sites sites at half filling with translations, sectors k = 0 (f64) and k = 3 (c128) -- at 32 sites 18.8 M representatives.
    sample      --samples words drawn from |<s|psi>|^2 of a uniform random psi, and its two parts: the rows (cumsum of |psi|^2,
                uniforms, searchsorted) and the images (randint, k_orbit_image);
    amplitudes  of those sampled words, K = 1 and K = 8 as an interleaved (n, 8) block;
and for scale beside them, in the same sector: SectorProjection.project of a full-basis vector (the same element loop per row, a
closed-form rank where the amplitude kernel probes the index table) and one matvec of the Hamiltonian.  Timed by device events after
--warmup runs; min, median and max of --steps runs.  One JSON line per sector, appended to --out.
usage: amplitude_bench.py [--sites 32] [--samples 16777216] [--steps 3] [--warmup 1] [--sectors 0,3] [--no-scale]
                          [--out profiles/amplitude_bench.jsonl]"""
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
ap.add_argument("--samples", type=int, default=1 << 24)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sectors", default="0,3")
ap.add_argument("--no-scale", action="store_true", help="leave out project and the matvec")
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.cuda.set_device(0)
K = 8


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(fn, check=None):
    for _ in range(args.warmup):
        fn()
    if check:
        check()
    t = sorted(timed(fn) for _ in range(args.steps))
    if check:
        check()
    return {"min": round(t[0], 4), "median": round(t[len(t) // 2], 4), "max": round(t[-1], 4)}


def fill(t, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    v = torch.view_as_real(t) if t.is_complex() else t
    v.uniform_(-0.5, 0.5, generator=g)
    return t


for k in (int(x) for x in args.sectors.split(",")):
    L = args.sites
    cfg = config.heisenberg_chain_config(L)
    cfg["basis"]["symmetries"] = [{"permutation": [(i + 1) % L for i in range(L)], "sector": k}]
    t0 = time.perf_counter()
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps_list, _ = D.enumerateStates(basis, 1)
    reps = reps_list[0]
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    n, B = int(reps.numel()), args.samples
    sa = D.SectorAmplitudes(basis, reps)
    dtype = torch.complex128 if sa.complex_characters else torch.float64
    rec = {"model": f"heisenberg_chain_{L}", "symmetries": "translation", "sector": k, "dtype": "c128" if sa.complex_characters else "f64",
           "n_representatives": n, "samples": B, "num_elements": sa.num_elements, "kernel": sa.kernel, "steps": args.steps,
           "warmup": args.warmup, "setup_seconds": round(setup_s, 2)}
    psi = fill(torch.empty(n, dtype=dtype, device="cuda"), 1)
    # sampling, whole and in its two parts
    rec["sample_ms"] = measure(lambda: sa.sample(psi, B, seed=1), sa.check)
    rows, gen = sa._rows("amplitude_bench", psi, B, 1)
    rec["sample_rows_cumsum_searchsorted_ms"] = measure(lambda: sa._rows("amplitude_bench", psi, B, 1))
    elements = torch.randint(sa.num_elements, (B,), generator=gen, device="cuda", dtype=torch.int32)
    rec["orbit_image_ms"] = measure(lambda: sa.orbit_states(rows, elements, check=False), sa.check)
    words = sa.orbit_states(rows, elements)
    del rows, elements
    # amplitudes of the sampled words
    out1 = torch.empty(B, dtype=dtype, device="cuda")
    rec["amplitudes_K1_ms"] = measure(lambda: sa.amplitudes(words, psi, out=out1, check=False), sa.check)
    rec["states_per_s_K1"] = round(B / (rec["amplitudes_K1_ms"]["median"] * 1e-3), 1)
    del out1
    block = fill(torch.empty(n, K, dtype=dtype, device="cuda"), 2)
    out8 = torch.empty(B, K, dtype=dtype, device="cuda")
    rec["amplitudes_K8_interleaved_ms"] = measure(lambda: sa.amplitudes(words, block, out=out8, check=False), sa.check)
    del block, out8, words
    torch.cuda.empty_cache()
    if not args.no_scale:
        pj = D.SectorProjection(basis, reps)
        phi = fill(torch.empty(pj.full_size, dtype=dtype, device="cuda"), 3)
        low = torch.empty(n, dtype=dtype, device="cuda")
        rec["project_K1_ms"] = measure(lambda: pj.project(phi, out=low, check=False), pj.check)
        rec["rows_per_s_project"] = round(n / (rec["project_K1_ms"]["median"] * 1e-3), 1)
        rec["full_size"] = pj.full_size
        del phi, low
        pj.destroy()
        torch.cuda.empty_cache()
        y = torch.zeros_like(psi)
        plan = D.MatvecPlan(h, reps_list, dtype)
        rec["matvec_ms"] = measure(lambda: plan.matvec([psi], [y]))
        rec["matvec_kernel"] = plan.kernel
        plan.destroy()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    sa.destroy()
    del psi, reps, reps_list, basis, h
    torch.cuda.empty_cache()
