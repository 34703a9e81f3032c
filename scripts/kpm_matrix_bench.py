#!/usr/bin/env python3
"""What the matrix-valued Chebyshev moments cost ("Matrix moments"), on the two sectors the block benchmarks use:
  spin      heisenberg_chain_32 with translations, k = 3
  fermion   the 28-mode t-V ring (V = 1) with translations, N = 14, k = 3
c128, K = 8, interleaved blocks, device events, 1 warm-up and 3 timed runs of each, alternating in one process; min-max.
  step      one order of MatvecPlan.matvec_block_axpby_gram against one order of MatvecPlan.matvec_block_axpby (with its dots): the
            difference is the Gram launch in place, X^+ [X | Y] with X read once
  gram      the two products X^+ X and X^+ Y alone, as two kpm.block_gram calls under LS_AMD_GRAM=mfma and =valu and as two
            torch.matmul(X.conj().T, .); the measured streaming read rate of the device (ls_amd_stream_read over X) and the ratio of
            the in-place Gram launch to 2 n K 16 B at that rate
  moments   kpm.chebyshev_moment_matrices (K columns) against the polarisation route through the unchanged kpm.chebyshev_moments
            (K^2 columns: v_a, v_a + v_b, v_a + i v_b), and the largest difference of the two sets of moments
  forms     --forms: k_block_gram_mfma against k_block_gram and torch.matmul on synthetic interleaved blocks of 2^29 bytes, f64 and
            c128, K in 1, 2, 4, 8, 16, 32, 64: the table behind the `auto` rule of LS_AMD_GRAM
One JSON line per record, appended to --out.
usage: kpm_matrix_bench.py [--which spin|fermion|both|none] [--forms] [--sites 32] [--modes 28] [--k 3] [--K 8] [--moments 16]
                           [--steps 3] [--warmup 1] [--out profiles/kpm_matrix_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import _lib, config, kpm  # noqa: E402
from distributed_matvec_amd.diagonalize import LocalOperator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--which", default="both", choices=["spin", "fermion", "both", "none"])
ap.add_argument("--forms", action="store_true")
ap.add_argument("--sites", type=int, default=32)
ap.add_argument("--modes", type=int, default=28)
ap.add_argument("--k", type=int, default=3)
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--moments", type=int, default=16)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
K = args.K
dtype = torch.complex128
torch.cuda.set_device(0)


def translation(L, k):
    return [{"permutation": [(i + 1) % L for i in range(L)], "sector": k}]


def spin_ring(L, k):
    cfg = config.heisenberg_chain_config(L)
    cfg["basis"]["symmetries"] = translation(L, k)
    return cfg


def tv_ring(L, N, k, t=1.0, V=1.0):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    terms = [{"expression": f"{-t!r} × c†₀ c₁", "sites": bonds}, {"expression": f"{-t!r} × c†₁ c₀", "sites": bonds},
             {"expression": f"{V!r} × n₀ n₁", "sites": bonds}]
    return {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": N, "symmetries": translation(L, k)},
            "hamiltonian": {"terms": terms}}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternating(fns):
    """{name: sorted ms of args.steps runs} after args.warmup runs of each, the candidates taking turns"""
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(args.steps):
        for name, fn in fns.items():
            out[name].append(timed(fn))
    return {name: sorted(v) for name, v in out.items()}


def span(ms):
    return {"min": round(ms[0], 4), "max": round(ms[-1], 4)}


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def with_form(form, fn):
    def run():
        os.environ["LS_AMD_GRAM"] = form  # (read at every call)
        try:
            fn()
        finally:
            os.environ.pop("LS_AMD_GRAM", None)
    return run


def read_rate(x):
    """GB/s of a streaming read of x (ls_amd_stream_read, 4 loads of 16 bytes in flight per lane)"""
    L = _lib.load()
    sink = torch.zeros(4, dtype=torch.int32, device="cuda")
    nb = x.numel() * x.element_size()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = alternating({"read": lambda: _lib.check(L.ls_amd_stream_read(C.c_void_p(x.data_ptr()), nb, 4, C.c_void_p(sink.data_ptr()), st))})["read"]
    return nb / (ms[0] * 1e-3) / 1e9


def sector(head, cfg, bounds):
    t0 = time.perf_counter()
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    op = LocalOperator(h, reps, dtype)
    plan = op.plan
    n = int(reps[0].numel())
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    X = kpm.random_phase_block(n, K, dtype, 1)
    Y = torch.zeros_like(X)
    dots = torch.zeros(2 * K, dtype=torch.float64, device="cuda")
    gram = torch.zeros((2, K, K), dtype=dtype, device="cuda")
    head = {**head, "dtype": "c128", "K": K, "layout": "interleaved", "n": n, "steps": args.steps, "warmup": args.warmup,
            "kernel": plan.axpby_kernel(K), "gram_kernel": plan.gram_kernel(K), "setup_seconds": round(setup_s, 2)}

    # one order of the recurrence, with dots and with Gram matrices (gamma = 0: Y is assigned, every run does the same work)
    step = alternating({"axpby": lambda: plan.matvec_block_axpby(X, Y, 1.0 / a, -b / a, 0.0, dots=dots, check=False),
                        "axpby_gram": lambda: plan.matvec_block_axpby_gram(X, Y, 1.0 / a, -b / a, 0.0, gram, check=False)})
    plan.check()
    in_place = step["axpby_gram"][0] - step["axpby"][0]
    d = dots.cpu().numpy()
    g = gram.cpu().numpy()
    diag = np.arange(K)
    emit({**head, "record": "step", "axpby_ms": span(step["axpby"]), "axpby_gram_ms": span(step["axpby_gram"]),
          "gram_over_axpby_min": round(step["axpby_gram"][0] / step["axpby"][-1], 4), "gram_over_axpby_max": round(step["axpby_gram"][-1] / step["axpby"][0], 4),
          "gram_in_place_ms": round(in_place, 4),
          "max_abs_diagonal_minus_dots": float(max(np.abs(g[0][diag, diag].real - d[:K]).max(), np.abs(g[1][diag, diag].real - d[K:]).max())),
          "max_abs_dots": float(np.abs(d).max())})

    # the two products alone
    outs = {}

    def pair(name):
        def run():
            outs[name] = (kpm.block_gram(X, X), kpm.block_gram(X, Y))
        return run

    def matmuls():
        outs["torch"] = (torch.matmul(X.conj().T, X), torch.matmul(X.conj().T, Y))

    alone = alternating({"mfma": with_form("mfma", pair("mfma")), "valu": with_form("valu", pair("valu")), "torch": matmuls})
    rate = read_rate(X)
    floor_ms = 2.0 * n * K * 16 / (rate * 1e9) * 1e3
    scale = float(outs["torch"][0].abs().max())
    emit({**head, "record": "gram", "two_block_gram_mfma_ms": span(alone["mfma"]), "two_block_gram_valu_ms": span(alone["valu"]),
          "two_torch_matmul_ms": span(alone["torch"]), "stream_read_GBps": round(rate, 1), "bytes_X_and_Y": 2 * n * K * 16,
          "read_X_and_Y_ms": round(floor_ms, 4), "gram_in_place_ms": round(in_place, 4),
          "gram_in_place_over_read": round(in_place / floor_ms, 3), "two_block_gram_mfma_over_read_of_3_blocks": round(alone["mfma"][0] / (1.5 * floor_ms), 3),
          "max_abs_mfma_minus_valu": float(max((p - q).abs().max() for p, q in zip(outs["mfma"], outs["valu"]))),
          "max_abs_mfma_minus_torch": float(max((p - q).abs().max() for p, q in zip(outs["mfma"], outs["torch"]))), "max_abs_gram": scale})
    del outs, Y

    # K x K moment matrices: K columns with Gram matrices against K^2 columns with dots
    M = args.moments
    pairs = [(i, j) for i in range(K) for j in range(i + 1, K)]
    P = torch.empty((n, K * K), dtype=dtype, device="cuda")
    P[:, :K] = X
    for c, (i, j) in enumerate(pairs):
        P[:, K + 2 * c] = X[:, i] + X[:, j]
        P[:, K + 2 * c + 1] = X[:, i] + 1j * X[:, j]
    res = {}

    def matrices():
        res["gram"] = kpm.chebyshev_moment_matrices(op, X, M, bounds)

    def polarisation():
        res["pol"] = np.concatenate([kpm.chebyshev_moments(op, P[:, c0:c0 + 64], M, bounds) for c0 in range(0, K * K, 64)])

    ms = alternating({"matrices": matrices, "polarisation": polarisation})
    mu = np.zeros((M, K, K), dtype=np.complex128)
    pol = res["pol"]
    mu[:, diag, diag] = pol[:K].T
    for c, (i, j) in enumerate(pairs):  # <a + b|T|a + b> = aa + bb + 2 Re ab;  <a + i b|T|a + i b> = aa + bb - 2 Im ab
        re = 0.5 * (pol[K + 2 * c] - pol[i] - pol[j])
        im = -0.5 * (pol[K + 2 * c + 1] - pol[i] - pol[j])
        mu[:, i, j] = re + 1j * im
        mu[:, j, i] = re - 1j * im
    emit({**head, "record": "moments", "num_moments": M, "matvec_columns_matrices": K * ((M + 1) // 2), "matvec_columns_polarisation": K * K * ((M + 1) // 2),
          "moment_matrices_ms": span(ms["matrices"]), "polarisation_ms": span(ms["polarisation"]),
          "matrices_over_polarisation_min": round(ms["matrices"][0] / ms["polarisation"][-1], 4),
          "matrices_over_polarisation_max": round(ms["matrices"][-1] / ms["polarisation"][0], 4),
          "max_abs_difference": float(np.abs(mu - res["gram"]).max()), "max_abs_moment": float(np.abs(res["gram"]).max())})


def forms():
    """single products A^+ B on synthetic interleaved blocks of 2^29 bytes: the table behind LS_AMD_GRAM=auto"""
    for dt, name in ((torch.float64, "f64"), (torch.complex128, "c128")):
        w = 16 if dt == torch.complex128 else 8
        for k in (1, 2, 4, 8, 16, 32, 64):
            n = (1 << 29) // (k * w)
            A = kpm.random_phase_block(n, k, dt, 3)
            B = kpm.random_phase_block(n, k, dt, 4)
            outs = {}

            def one(tag):
                def run():
                    outs[tag] = kpm.block_gram(A, B)
                return run

            def matmul():
                outs["torch"] = torch.matmul(A.conj().T if dt == torch.complex128 else A.T, B)

            ms = alternating({"mfma": with_form("mfma", one("mfma")), "valu": with_form("valu", one("valu")), "torch": matmul})
            rate_ms = 2.0 * (1 << 29) / 1e9  # ms per GB/s: the two blocks, once each
            emit({"record": "forms", "dtype": name, "K": k, "layout": "interleaved", "n": n, "steps": args.steps, "warmup": args.warmup,
                  "mfma_ms": span(ms["mfma"]), "valu_ms": span(ms["valu"]), "torch_matmul_ms": span(ms["torch"]),
                  "mfma_GBps": round(rate_ms / ms["mfma"][0] * 1e3, 1), "valu_GBps": round(rate_ms / ms["valu"][0] * 1e3, 1),
                  "torch_GBps": round(rate_ms / ms["torch"][0] * 1e3, 1), "mfma_is_slower_than_valu": bool(ms["mfma"][0] > ms["valu"][-1]),
                  "max_abs_mfma_minus_valu": float((outs["mfma"] - outs["valu"]).abs().max()),
                  "max_abs_mfma_minus_torch": float((outs["mfma"] - outs["torch"]).abs().max()), "max_abs_gram": float(outs["torch"].abs().max())})
            del A, B, outs


if args.forms:
    forms()
if args.which in ("spin", "both"):
    L = args.sites
    sector({"model": f"heisenberg_chain_{L}", "symmetries": "translation", "sector": args.k % L}, spin_ring(L, args.k % L), (-3.0 * L - 0.5, L + 0.5))
if args.which in ("fermion", "both"):
    L = args.modes
    sector({"model": f"tV_ring_{L}", "symmetries": "translation", "particles": L // 2, "sector": args.k % L}, tv_ring(L, L // 2, args.k % L),
           (-2.0 * L - 0.5, 3.0 * L + 0.5))
