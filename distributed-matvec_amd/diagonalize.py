"""Eigensolver driver: the caller of the matvec path in BASELINE config 5
(`/root/reference/src/Diagonalize.chpl:258-332`: load YAML -> basis states -> PRIMME `dprimme` with
`ls_chpl_primme_matvec` -> eigenpairs).

libprimme is not available here (headers only, `/root/reference/primme_headers/`), so the PRIMME-ABI
callbacks stay exported from the C library for a real PRIMME (include/ls_chpl.h) and
this module ships a small restarted Lanczos that keeps every vector in HBM — PRIMME hands host
pointers to its matvec callback, which costs a PCIe round trip of x and y per call,
so a device-resident solver is the MI355X-first way to drive this path.

The solver only needs three things from its operator: `matvec(x, y)`, a global dot product and the
local vector length — provided both by a single-process plan (all partitions on one GPU) and by
`DistributedOperator` (one partition per rank; dots = all_reduce = PRIMME's globalSumReal,
`/root/reference/src/PRIMME.chpl:267-311`).
"""
from __future__ import annotations

import math
import os
import time
from dataclasses import dataclass, field


class LocalOperator:
    """H on one device: P logical partitions concatenated into flat per-partition vectors."""

    def __init__(self, matrix, representatives, dtype, mode="auto", slot_cache_bytes=0):
        import torch

        from .api import MatvecPlan

        self.torch = torch
        self.reps = list(representatives)
        self.plan = MatvecPlan(matrix, self.reps, dtype, mode=mode)
        # an eigensolver applies ONE plan hundreds of times: keep the resolved packet streams of a projected basis in HBM
        # when the caller has room for them (ls_amd_plan_cache_slots; 0 rows = the plan stays matrix-free)
        self.cached_rows = self.plan.cache_slots(slot_cache_bytes) if slot_cache_bytes > 0 and len(self.reps) == 1 else 0
        self.dtype = dtype
        self.sizes = [int(r.numel()) for r in self.reps]
        self.n_local = sum(self.sizes)
        self.device = self.reps[0].device
        self.matvecs = 0

    def _split(self, v):
        return list(v.split(self.sizes)) if len(self.sizes) > 1 else [v]

    def matvec(self, x, y):
        y.zero_()
        self.plan.matvec(self._split(x), self._split(y), check=False)
        self.matvecs += 1

    def check(self):
        self.plan.check()

    def dot(self, a, b):
        return self.torch.vdot(a, b) if a.is_complex() else self.torch.dot(a, b)

    def new_vector(self):
        return self.torch.zeros(self.n_local, dtype=self.dtype, device=self.device)

    def random_vector(self, seed):
        from .api import fillRandom

        return self.torch.cat([fillRandom(r, seed, self.dtype) for r in self.reps])

    def matvec_block(self, x, y):
        """Y[:, c] <- H X[:, c] for the K columns of the (n, K) views x and y (column-major views `V[s:s+K].T` of basis rows are
        the layout of the block solver).  One-partition plans take ls_amd_matvec_block; with P > 1 the columns go through the
        single-vector plan one by one."""
        K = int(x.shape[1])
        if len(self.sizes) == 1:
            self.plan.matvec_block(x, y, check=False)
        else:
            for c in range(K):
                yc = y[:, c] if y[:, c].is_contiguous() else self.new_vector()
                yc.zero_()
                self.plan.matvec(self._split(x[:, c].contiguous()), self._split(yc), check=False)
                if yc.data_ptr() != y[:, c].data_ptr():
                    y[:, c] = yc
        self.matvecs += K

    def block_kernel(self, K):
        """path a block of K columns takes (\"columns\" for plans with P > 1: the loop of matvec_block)"""
        return self.plan.block_kernel(K) if len(self.sizes) == 1 else "columns"


class RankOperator:
    """H with one partition per process (wraps distributed.DistributedOperator)."""

    def __init__(self, dist_op, representatives, dtype):
        import torch

        self.torch = torch
        self.op = dist_op
        self.reps = representatives
        self.dtype = dtype
        self.n_local = int(representatives.numel())
        self.device = representatives.device
        self.matvecs = 0

    def matvec(self, x, y):
        y.zero_()
        self.op.matvec(x, y, check=False)
        self.matvecs += 1

    def check(self):
        self.op.engine.check()

    def dot(self, a, b):
        return self.op.dot(a, b)

    def global_sum(self, t):
        if t.is_complex():
            r = self.torch.view_as_real(t).contiguous()
            self.op.global_sum(r)
            return self.torch.view_as_complex(r)
        return self.op.global_sum(t)

    def new_vector(self):
        return self.torch.zeros(self.n_local, dtype=self.dtype, device=self.device)

    def random_vector(self, seed):
        from .api import fillRandom

        return fillRandom(self.reps, seed, self.dtype)


@dataclass
class EigenResult:
    eigenvalues: list
    eigenvectors: list
    residual_norms: list
    matvecs: int
    restarts: int
    converged: bool
    seconds: float
    history: list = field(default_factory=list)


def lanczos_smallest(op, num_evals: int = 1, eps: float = 1e-6, max_basis: int = 24, max_restarts: int = 500,
                     seed: int = 1234, verbose: bool = False) -> EigenResult:
    """Smallest `num_evals` eigenpairs of the Hermitian operator `op` (target = primme_smallest, eps as
    in `/root/reference/src/Diagonalize.chpl:164-172,205`): thick-restart Lanczos (Wu & Simon) with
    full re-orthogonalisation (classical Gram-Schmidt twice, one GEMV per pass) inside a window of
    `max_basis` device vectors.  Residuals come from the Lanczos relation
    ||H y_i - theta_i y_i|| = |beta_m s_{m,i}|, so a step costs exactly one matvec.
    Converged when every wanted residual <= eps * ||H|| (estimated by the largest |Ritz value|)."""
    import numpy as np
    import torch

    t0 = time.perf_counter()
    k = num_evals
    m = max(max_basis, 2 * k + 4)
    v = op.random_vector(seed)
    n = v.numel()
    cplx = v.is_complex()
    V = torch.empty((m + 1, n), dtype=v.dtype, device=v.device)
    T = np.zeros((m + 1, m), dtype=complex if cplx else float)

    def gsum(t):
        return op.global_sum(t) if hasattr(op, "global_sum") else t

    def norm(u):
        # (no full-size temporaries: the vectors of chain_40_symm are 6.9 GB each and the HBM next to them belongs to the slot cache)
        return math.sqrt(float(gsum((torch.linalg.vector_norm(u) ** 2).reshape(1))[0]))

    torch.div(v, norm(v), out=V[0])
    del v
    w = op.new_vector()
    # fused orthogonalisation sweeps (real f64 vectors on the device; the partial sums of a rank go through the operator's global sum)
    fused, fused_rows = None, 0
    if not cplx and V.is_cuda and V.dtype == torch.float64 and os.environ.get("LS_AMD_FUSED_ORTH", "1") != "0":
        import ctypes as C

        from . import _lib
        from .api import _stream_ptr

        lib = _lib.load()
        fused_rows = int(lib.ls_amd_orth_max_rows())
        obuf = torch.zeros(fused_rows + 1, dtype=torch.float64, device=V.device)

        def fused(rows, Vb, wv, hin):
            _lib.check(lib.ls_amd_orth_pass(rows, n, C.c_void_p(Vb.data_ptr()), Vb.stride(0), C.c_void_p(wv.data_ptr()),
                                            C.c_void_p(hin.data_ptr()) if hin is not None else None, C.c_void_p(obuf.data_ptr()), _stream_ptr()))
            return gsum(obuf[: rows + 1].clone())
    j0 = 0  # number of locked (restarted) vectors at the front of V
    restarts = 0
    history = []
    prof = {"orth": 0.0, "normalise": 0.0, "restart": 0.0} if os.environ.get("LS_AMD_LANCZOS_PROFILE") else None

    def tick():
        if prof is None:
            return 0.0
        torch.cuda.synchronize()
        return time.perf_counter()

    while True:
        for j in range(j0, m):
            op.matvec(V[j], w)
            Vj = V[: j + 1]
            t_a = tick()
            if fused is not None and j + 1 <= fused_rows:
                # classical Gram-Schmidt with the fused sweeps of csrc/orth.hip: pass 1 -> h and ||w||^2; pass 2 applies h and returns
                # the overlaps that are left and the new norm in the same sweep.  A third sweep only when orthogonality was
                # really lost (the left-over overlaps are not at rounding level relative to what remains of w)
                out = fused(j + 1, Vj, w, None)
                h = out[: j + 1].clone()
                out = fused(j + 1, Vj, w, h)
                o2 = out.cpu().numpy()
                h2n, n1 = float(np.sqrt((o2[: j + 1] ** 2).sum())), math.sqrt(max(float(o2[j + 1]), 0.0))
                if h2n > 1e-11 * n1:
                    h2 = out[: j + 1].clone()
                    out = fused(j + 1, Vj, w, h2)
                    h = h + h2
                    n1 = math.sqrt(max(float(out[j + 1].item()), 0.0))
                h = h.cpu().numpy()
                beta = n1
            else:
                h = gsum(torch.mv(Vj.conj() if cplx else Vj, w))
                w -= torch.mv(Vj.t(), h)
                h2 = gsum(torch.mv(Vj.conj() if cplx else Vj, w))
                w -= torch.mv(Vj.t(), h2)
                h = (h + h2).cpu().numpy()
                beta = norm(w)
            if prof is not None:
                prof["orth"] += tick() - t_a
            T[: j + 1, j] = h
            T[j + 1, j] = beta
            if beta < 1e-14 * max(1.0, float(np.abs(h).max())):
                m_eff = j + 1
                break
            t_a = tick()
            torch.div(w, beta, out=V[j + 1])
            if prof is not None:
                prof["normalise"] += tick() - t_a
        else:
            m_eff = m
        Tm = T[:m_eff, :m_eff]
        Tm = 0.5 * (Tm + Tm.conj().T)
        theta, S = np.linalg.eigh(Tm)
        beta_m = T[m_eff, m_eff - 1].real if m_eff == m else 0.0
        kk = min(k, m_eff)
        res = [abs(beta_m * S[m_eff - 1, i]) for i in range(kk)]
        scale = max(float(np.abs(theta).max()), 1e-300)
        history.append((op.matvecs, [float(t) for t in theta[:kk]], res))
        if verbose:
            print(f"[lanczos] restart {restarts}: matvecs={op.matvecs} theta={theta[:kk]} res={res}", flush=True)
        done = all(r <= eps * scale for r in res) or m_eff < m
        if done or restarts >= max_restarts:
            St = torch.as_tensor(S[:, :kk], dtype=V.dtype, device=V.device)
            Y = torch.mm(St.t(), V[:m_eff])  # Ritz vectors, [kk, n]
            vecs = [Y[i].clone() for i in range(kk)]
            op.check()
            return EigenResult([float(t) for t in theta[:kk]], vecs, [float(r) for r in res], op.matvecs, restarts, bool(done),
                               time.perf_counter() - t0, history)
        # thick restart: keep `keep` Ritz vectors, then the next Lanczos vector
        t_a = tick()
        keep = min(m_eff - 2, kk + max(2, (m_eff - kk) // 3))
        St = torch.as_tensor(S[:, :keep], dtype=V.dtype, device=V.device)
        if fused is not None and m_eff <= fused_rows:
            # V[:keep] <- S^T V[:m_eff] in place, one read of m_eff and one write of keep vectors (csrc/orth.hip)
            Sc = St.contiguous()
            _lib.check(lib.ls_amd_basis_rotate(m_eff, keep, n, C.c_void_p(V.data_ptr()), V.stride(0), C.c_void_p(Sc.data_ptr()), _stream_ptr()))
        else:
            # ... in column blocks: the product of whole rows would be a temporary of `keep` vectors
            step = 1 << 24
            for c0 in range(0, n, step):
                c1 = min(n, c0 + step)
                V[:keep, c0:c1] = torch.mm(St.t(), V[:m_eff, c0:c1])
        V[keep] = V[m_eff]
        T[:, :] = 0
        for i in range(keep):
            T[i, i] = theta[i]
            T[keep, i] = beta_m * S[m_eff - 1, i]  # coupling of the kept Ritz vectors to the next vector
            T[i, keep] = np.conj(T[keep, i])
        j0 = keep
        restarts += 1
        if prof is not None:
            prof["restart"] += tick() - t_a
            print(f"[lanczos] profile after restart {restarts}: " + ", ".join(f"{k} {v:.2f} s" for k, v in prof.items()), flush=True)


def _block_orth_ops(op, V, K):
    """(sweep, rotate, fused) for lanczos_block_smallest on the basis array V [rows, n].
    sweep(p, s, h): classical Gram-Schmidt sweep of the block V[s:s+K] against V[:p] -- if h (p x K) is given, first
    V[s+c] -= sum_k h[k][c] V[k] -- returning (overlaps (p x K) = <V_k, W_c> and the Gram matrix (K x K) = <W_c, W_c'>) of the
    updated block as host arrays.  rotate(m_in, m_out, S, r0): V[r0:r0+m_out] <- S^T V[r0:r0+m_in] in place.
    Fused (real f64 on the device, LS_AMD_FUSED_ORTH != 0): ls_amd_orth_block_pass / ls_amd_block_rotate (csrc/orth_block.hip),
    one read of V[:p] per sweep.  Otherwise torch products in column chunks: no temporary larger than one block."""
    import numpy as np
    import torch

    n = V.shape[1]

    def gsum(t):
        return op.global_sum(t) if hasattr(op, "global_sum") else t

    if V.is_cuda and V.dtype == torch.float64 and os.environ.get("LS_AMD_FUSED_ORTH", "1") != "0":
        import ctypes as C

        from . import _lib
        from .api import _stream_ptr

        lib = _lib.load()
        rows = int(lib.ls_amd_orth_block_max_rows())
        obuf = torch.zeros(rows * K + K * K, dtype=torch.float64, device=V.device)
        ld = V.stride(0)

        def sweep(p, s, h):
            hd = torch.as_tensor(np.ascontiguousarray(h), dtype=torch.float64, device=V.device) if h is not None else None
            _lib.check(lib.ls_amd_orth_block_pass(p, K, n, C.c_void_p(V.data_ptr()), ld, C.c_void_p(V[s].data_ptr()), ld,
                                                  C.c_void_p(hd.data_ptr()) if hd is not None else None, C.c_void_p(obuf.data_ptr()),
                                                  _stream_ptr()))
            o = gsum(obuf[: p * K + K * K].clone()).cpu().numpy()
            return o[: p * K].reshape(p, K), o[p * K:].reshape(K, K)

        def rotate(m_in, m_out, S, r0=0):
            Sd = torch.as_tensor(np.ascontiguousarray(S), dtype=torch.float64, device=V.device)
            _lib.check(lib.ls_amd_block_rotate(m_in, m_out, n, C.c_void_p(V[r0].data_ptr()), ld, C.c_void_p(Sd.data_ptr()), _stream_ptr()))

        return sweep, rotate, rows

    cplx = V.is_complex()
    step = max(1, (1 << 24) // max(K, 1))

    def sweep(p, s, h):
        W = V[s:s + K]
        if h is not None:
            Ht = torch.as_tensor(np.ascontiguousarray(h), dtype=V.dtype, device=V.device).t()  # K x p
            for c0 in range(0, n, step):
                c1 = min(n, c0 + step)
                W[:, c0:c1] -= torch.mm(Ht, V[:p, c0:c1])
        o = torch.zeros((p, K), dtype=V.dtype, device=V.device)
        g = torch.zeros((K, K), dtype=V.dtype, device=V.device)
        for c0 in range(0, n, step):
            c1 = min(n, c0 + step)
            Wc = W[:, c0:c1]
            if p:
                o += torch.mm(V[:p, c0:c1].conj() if cplx else V[:p, c0:c1], Wc.t())
            g += torch.mm(Wc.conj() if cplx else Wc, Wc.t())
        return gsum(o).cpu().numpy(), gsum(g).cpu().numpy()

    def rotate(m_in, m_out, S, r0=0):
        St = torch.as_tensor(np.ascontiguousarray(S), dtype=V.dtype, device=V.device).t()
        for c0 in range(0, n, step):
            c1 = min(n, c0 + step)
            V[r0:r0 + m_out, c0:c1] = torch.mm(St, V[r0:r0 + m_in, c0:c1])

    return sweep, rotate, None


def lanczos_block_smallest(op, num_evals: int = 1, block_size: int = 4, eps: float = 1e-6, max_basis: int | None = None,
                           max_restarts: int = 500, seed: int = 1234, verbose: bool = False) -> EigenResult:
    """Smallest `num_evals` eigenpairs of the Hermitian operator `op` by block thick-restart Lanczos (block Krylov-Schur, Zhou &
    Saad 2008) with blocks of K = `block_size` vectors -- the reference's kMaxBlockSize, handed to PRIMME as maxBlockSize
    (Diagonalize.chpl:172,192).  A Krylov space grown from one vector holds one vector per eigenspace; a block of K start vectors
    finds a degenerate level with its multiplicity (up to K).
    Step: W = H V_j (op.matvec_block, one pass over the plan for K columns); classical Gram-Schmidt of W against the basis twice
    (one sweep of the basis each, csrc/orth_block.hip), a third sweep only when the overlaps left exceed 1e-11 of the remaining
    norm (lanczos_smallest's rule); Cholesky-QR from the Gram matrix of the last sweep, repeated once when ||Q^T Q - I|| > 1e-12.
    A column whose norm falls below 1e-10 of its norm before the orthogonalisation (or that makes the Gram matrix singular) is
    deflated: replaced by a fresh random vector orthogonalised against the basis, with zero coupling in T; when even that has
    nothing left, the basis spans an invariant subspace and the Ritz pairs are exact.
    The basis holds max(max_basis, 2 num_evals + 3 K) vectors (<= 128 on the fused path) plus one block.  Residuals,
    convergence test, `history` and EigenResult fields as lanczos_smallest; `matvecs` counts columns."""
    import numpy as np
    import torch

    t0 = time.perf_counter()
    K = int(block_size)
    k = num_evals
    if not 1 <= K <= 16:
        raise ValueError(f"block_size = {K}: the block solver takes 1 <= block_size <= 16")
    if op.n_local < K and not hasattr(op, "global_sum"):
        raise ValueError(f"block_size = {K} exceeds the dimension {op.n_local}")
    mb = max(max_basis if max_basis is not None else 0, 2 * k + 3 * K)
    x0 = op.random_vector(seed)
    n, dt, dev = x0.numel(), x0.dtype, x0.device
    cplx = x0.is_complex()
    # the basis: mb vectors and one block (the next block W = H V_j is computed into the rows after the basis it joins)
    V = torch.empty((mb + K, n), dtype=dt, device=dev)
    sweep, rotate, fused_rows = _block_orth_ops(op, V, K)
    if fused_rows is not None and mb > fused_rows:
        raise ValueError(f"lanczos_block_smallest: a basis of {mb} vectors exceeds the {fused_rows} rows of the fused "
                         f"orthogonalisation (ls_amd_orth_block_max_rows); lower max_basis, num_evals or block_size")
    T = np.zeros((mb + K, mb + K), dtype=complex if cplx else float)
    restarts = 0
    history = []
    rng_seed = [seed + K]
    prof = {"matvec": 0.0, "orth": 0.0, "restart": 0.0} if os.environ.get("LS_AMD_LANCZOS_PROFILE") else None

    def tick():
        if prof is None:
            return 0.0
        torch.cuda.synchronize()
        return time.perf_counter()

    def orthogonalise(p, s):
        """CGS twice (three times when needed) of V[s:s+K] against V[:p]: (coefficients p x K, Gram of the result, Gram before)"""
        h, G = sweep(p, s, None)
        G0 = G
        if p == 0:
            return np.zeros((0, K), dtype=T.dtype), G, G0
        h2, G = sweep(p, s, h)
        left = np.sqrt((np.abs(h2) ** 2).sum(axis=0))
        if np.any(left > 1e-11 * np.sqrt(np.maximum(np.diag(G).real, 0.0))):
            _, G = sweep(p, s, h2)
            h = h + h2
        return h, G, G0

    def cholesky_deflate(G, G0):
        """upper R with R^H R = G over the columns that keep a norm; the deflated columns are returned separately: norm below
        1e-10 of the norm before, or a pivot that is not positive at the precision a Gram matrix resolves (below 1e-12 of the
        column's squared norm: the cancellation in G[c, c] - sum R[:, c]^2 is 1e-16 of it, so dependence inside the block shows
        there, not at 1e-20)"""
        G = 0.5 * (G + G.conj().T)
        R = np.zeros((K, K), dtype=T.dtype)
        dead = []
        for c in range(K):
            d = G[c, c].real - float(np.sum(np.abs(R[:c, c]) ** 2))
            before = max(G0[c, c].real, 0.0)
            if not d > (1e-10) ** 2 * before or not d > 1e-12 * G[c, c].real:
                dead.append(c)
                continue
            R[c, c] = math.sqrt(d)
            for c2 in range(c + 1, K):
                R[c, c2] = (G[c, c2] - np.dot(R[:c, c].conj(), R[:c, c2])) / R[c, c]
        return R, dead

    def normalise(s, G, G0):
        """Cholesky-QR of V[s:s+K] in place: returns (R, None), R the coupling (W = Q R).  Deflated columns are replaced by random
        vectors orthogonalised against V[:s] and the block, which the coupling does not reach.  When such a vector has nothing left, V[:s] and
        the block's live columns span the whole space: returns (R over all columns, the live columns), nothing normalised."""
        R, dead = cholesky_deflate(G, G0)
        if dead:
            # what is left of a deflated column is a combination W_live x of the live ones (x = 0 when its norm vanished): its
            # coupling is carried by them, and the column itself is free for a new direction
            live = [c for c in range(K) if c not in dead]
            X = np.linalg.solve(R[np.ix_(live, live)], R[np.ix_(live, dead)]) if live else None
            for c in dead:
                V[s + c] = op.random_vector(rng_seed[0])
                rng_seed[0] += 1
            # the surviving columns are orthogonal to V[:s] already: the new ones go through the same sweeps (whole block)
            _, G1, G10 = orthogonalise(s, s)
            R_all, dead_n = cholesky_deflate(G1, G10)
            R = R_all.copy()
            R[:, dead] = R_all[:, live] @ X if live else 0.0
            if dead_n:
                return R, ([c for c in range(K) if c not in dead_n], R_all)
        else:
            R_all = R
        rotate(K, K, np.linalg.inv(R_all), s)
        # ||Q^T Q - I|| by one m = 0 sweep; one more Cholesky-QR when it is not at rounding level
        _, Gq = sweep(0, s, None)
        if np.abs(Gq - np.eye(K)).max() > 1e-12:
            R2 = np.linalg.cholesky(0.5 * (Gq + Gq.conj().T)).conj().T
            rotate(K, K, np.linalg.inv(R2), s)
            R = R2 @ R
        return R, None

    def complete(p, q, live, R, R_all):
        """the space is exhausted at V[:p] + the live columns of V[p:p+K]: orthonormalise those (R_all over them is their Cholesky
        factor), apply H to them (the whole dimension is at most the basis size here) and fill T: V[:p + len(live)] spans an
        invariant subspace.  Returns its size."""
        s_ = len(live)
        if s_ == 0:
            return p
        Rl = R_all[np.ix_(live, live)]
        Wl = V[p:p + K][live].clone()
        V[p:p + s_] = torch.as_tensor(np.linalg.inv(Rl), dtype=V.dtype, device=V.device).t() @ Wl
        T[p:p + s_, q:q + K] = R[live, :]
        Y = torch.empty((s_, n), dtype=V.dtype, device=V.device)
        op.matvec_block(V[p:p + s_].t(), Y.t())
        T[:p + s_, p:p + s_] = (V[:p + s_].conj() @ Y.t()).cpu().numpy()
        return p + s_

    # start block: K random vectors, orthonormalised
    for c in range(K):
        V[c] = x0 if c == 0 else op.random_vector(seed + c)
    del x0
    _, G = sweep(0, 0, None)
    _, exhausted = normalise(0, G, G)
    if exhausted is not None:
        raise ValueError(f"lanczos_block_smallest: no {K} independent start vectors (dimension {n})")
    q, p = 0, K  # T columns [0, q) are known; V[q:p] is the block to be multiplied next
    while True:
        invariant = False
        while p + K <= mb + K:
            t_a = tick()
            op.matvec_block(V[q:p].t(), V[p:p + K].t())
            t_b = tick()
            h, G, G0 = orthogonalise(p, p)
            T[:p, q:p] = h
            R, exhausted = normalise(p, G, G0)
            if prof is not None:
                prof["matvec"] += t_b - t_a
                prof["orth"] += tick() - t_b
            if exhausted is not None:
                q = complete(p, q, exhausted[0], R, exhausted[1])
                invariant = True
                break
            q = p
            T[p:p + K, q - K:q] = R
            p += K
        # the projected matrix: block tridiagonal (arrow-shaped after a restart); the residual block is R_last = T[q:q+K, q-K:q]
        m_eff = q
        Tm = T[:m_eff, :m_eff]
        Tm = 0.5 * (Tm + Tm.conj().T)
        theta, S = np.linalg.eigh(Tm)
        Rl = np.zeros((K, K), dtype=T.dtype) if invariant else T[q:q + K, q - K:q]
        kk = min(k, m_eff)
        coup = Rl @ S[m_eff - K:m_eff, :]  # K x m_eff: residual of Ritz pair i = ||coup[:, i]||
        res = [float(np.linalg.norm(coup[:, i])) for i in range(kk)]
        scale = max(float(np.abs(theta).max()), 1e-300)
        history.append((op.matvecs, [float(t) for t in theta[:kk]], res))
        if verbose:
            print(f"[lanczos-block K={K}] restart {restarts}: matvecs={op.matvecs} theta={theta[:kk]} res={res}", flush=True)
        done = all(r <= eps * scale for r in res) or invariant
        if done or restarts >= max_restarts:
            St = torch.as_tensor(S[:, :kk], dtype=V.dtype, device=V.device)
            Y = torch.mm(St.t(), V[:m_eff])  # Ritz vectors, [kk, n]
            vecs = [Y[i].clone() for i in range(kk)]
            op.check()
            if prof is not None:
                print(f"[lanczos-block] profile: " + ", ".join(f"{a} {b:.2f} s" for a, b in prof.items()), flush=True)
            return EigenResult([float(t) for t in theta[:kk]], vecs, res, op.matvecs, restarts, bool(done),
                               time.perf_counter() - t0, history)
        # thick restart: the `keep` lowest Ritz vectors, then the residual block
        t_a = tick()
        keep = min(m_eff - 2 * K, kk + max(K, (m_eff - kk) // 3))
        rotate(m_eff, keep, S[:, :keep])
        V[keep:keep + K] = V[q:q + K]
        T[:, :] = 0
        for i in range(keep):
            T[i, i] = theta[i]
        T[keep:keep + K, :keep] = coup[:, :keep]
        T[:keep, keep:keep + K] = coup[:, :keep].conj().T
        q, p = keep, keep + K
        restarts += 1
        if prof is not None:
            prof["restart"] += tick() - t_a


class FilteredOperator:
    """-p(H) = -sum_n c_n T_n((H - b) / a) through the operator interface lanczos_block_smallest uses (matvec_block, matvec,
    random_vector, new_vector, matvecs, check, dtype, n_local, sizes, device, block_kernel): with the coefficients of
    kpm.delta_filter the levels of H nearest sigma are its SMALLEST.  op: a LocalOperator on one partition; every application is
    one MatvecPlan.matvec_block_series.  matvecs counts columns x orders of H (they are added to op.matvecs as well),
    applications the filter calls."""

    def __init__(self, op, coefficients, bounds):
        import numpy as np

        if len(op.sizes) != 1:
            raise ValueError("FilteredOperator: one-partition plans only")
        c = np.asarray(coefficients, dtype=np.float64).reshape(-1)
        if c.size < 1 or not np.isfinite(c).all():
            raise ValueError("FilteredOperator: coefficients: a non-empty sequence of finite real numbers")
        lo, hi = float(bounds[0]), float(bounds[1])
        if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
            raise ValueError(f"FilteredOperator: bounds = ({bounds[0]!r}, {bounds[1]!r}): need finite lo < hi")
        self.op = op
        self.coefficients = c
        self._negated = -c
        self.bounds = (lo, hi)
        self.order = int(c.size) - 1
        self.dtype = op.dtype
        self.n_local = op.n_local
        self.sizes = list(op.sizes)
        self.device = op.device
        self.matvecs = 0
        self.applications = 0
        self.seconds = 0.0  # wall time inside the filter calls

    def matvec_block(self, x, y):
        """Y <- -p(H) X for the K <= 64 columns of the (n, K) views x and y (any nested strides; x is left as it was)"""
        K = int(x.shape[1])
        t0 = time.perf_counter()
        self.op.plan.matvec_block_series(x, y, self._negated, self.bounds, check=False)  # (returns after its last guard read-back)
        self.seconds += time.perf_counter() - t0
        self.matvecs += K * self.order
        self.op.matvecs += K * self.order
        self.applications += 1

    def matvec(self, x, y):
        self.matvec_block(x.reshape(-1, 1), y.reshape(-1, 1))

    def check(self):
        self.op.check()

    def dot(self, a, b):
        return self.op.dot(a, b)

    def new_vector(self):
        return self.op.new_vector()

    def random_vector(self, seed):
        return self.op.random_vector(seed)

    def block_kernel(self, K):
        return self.op.plan.series_kernel(K)


@dataclass
class InteriorResult:
    eigenvalues: list         # the num_evals levels nearest sigma, ascending
    eigenvectors: list        # device vectors, one per level
    residual_norms: list      # ||H y - theta y||, computed from H y itself
    sigma: float
    order: int                # of the filter polynomial
    bounds: tuple             # (lo, hi) the spectrum was rescaled with
    applications: int         # filter calls (each one `order` block steps)
    matvecs: int              # columns that went through H: the filter's columns x orders, and the Rayleigh-Ritz steps
    polish_rounds: int
    converged: bool           # every residual <= eps max(|lo|, |hi|)
    seconds: float
    filter_seconds: float = 0.0   # ... of which inside the filter calls (Lanczos run and polish rounds)
    orth_seconds: float = 0.0     # ... of which in the Lanczos run outside the filter: orthogonalisation, restarts, the small problems
    ritz_seconds: float = 0.0     # ... of which inside the Rayleigh-Ritz steps (orthonormalisation, H Q, rotation, residuals)
    lanczos_restarts: int = 0
    kernel: str = ""          # MatvecPlan.series_kernel(block_size)


INTERIOR_MAX_RESTARTS = 30    # of the Lanczos run on p(H); what is left is the polish rounds' to finish


def _interior_window(num_evals, guard, block_size, max_basis):
    """the basis window lanczos_block_smallest opens for num_evals + guard pairs, and the rows its fused orthogonalisation holds"""
    return max(max_basis if max_basis is not None else 0, 2 * (num_evals + guard) + 3 * block_size), 128


def interior_eigenpairs(config_or_op, sigma, num_evals: int = 8, eps: float = 1e-6, block_size: int = 8, order=None, guard=None,
                        bounds=None, max_basis=None, max_polish: int = 3, seed: int = 1234, dtype=None, cut=None,
                        verbose: bool = False) -> InteriorResult:
    """The `num_evals` eigenpairs of a Hermitian operator nearest the energy `sigma`, at any basis size the matvec reaches on one
    partition: polynomially filtered block Lanczos (POLFED: Sierant, Lewenstein, Zakrzewski, PRL 125, 156601).
    config_or_op: a config (dict or YAML path) with a `hamiltonian:`, or a LocalOperator.
    1. bounds (kpm.spectral_bounds when None) and the order of the filter (kpm.filter_order for num_evals + guard levels, guard =
       max(block_size, num_evals // 4), from a density of states of 64 moments when None); p = kpm.delta_filter(sigma, bounds, order).
    2. lanczos_block_smallest on FilteredOperator(-p(H)) for num_evals + guard pairs, to eps / 4 of p's scale.
    3. Rayleigh-Ritz against H itself on the vectors it returns: p is flat at its peak, so p's own Ritz vectors do not separate
       neighbouring levels of H -- only the space they span is accurate.  The block is orthonormalised (Cholesky-QR twice), H Q is
       formed in blocks of <= 64 columns, the small problem solved on the host, and ||H y - theta y|| computed from H y.
    4. The num_evals pairs nearest sigma are kept; converged when each residual <= eps max(|lo|, |hi|).
    5. Otherwise up to max_polish rounds of subspace iteration: one more filter application on the whole Ritz block, then 3 and 4.
       What is still not converged after them is returned with converged=False.
    Refused before any device work: an operator that is not Hermitian, more than one partition, num_evals + guard beyond the basis
    window of lanczos_block_smallest, a sigma outside given bounds, order < 2.  -> InteriorResult."""
    import numpy as np
    import torch

    from . import api, kpm

    t0 = time.perf_counter()
    who = "interior_eigenpairs"
    for name, v, least in (("num_evals", num_evals, 1), ("block_size", block_size, 1), ("max_polish", max_polish, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
            raise ValueError(f"{who}: {name} = {v!r}: an integer >= {least}")
    if block_size > 16:
        raise ValueError(f"{who}: block_size = {block_size}: the block solver takes 1 <= block_size <= 16")
    if guard is None:
        guard = max(int(block_size), int(num_evals) // 4)
    if isinstance(guard, bool) or not isinstance(guard, (int, np.integer)) or guard < 0:
        raise ValueError(f"{who}: guard = {guard!r}: an integer >= 0")
    if order is not None and (isinstance(order, bool) or not isinstance(order, (int, np.integer)) or order < 2):
        raise ValueError(f"{who}: order = {order!r}: the filter needs an order >= 2")
    if not float(eps) > 0.0:
        raise ValueError(f"{who}: eps = {eps!r} must be positive")
    cut = kpm.FILTER_CUT if cut is None else float(cut)
    want = int(num_evals) + int(guard)
    window, rows = _interior_window(int(num_evals), int(guard), int(block_size), max_basis)
    if window > rows:
        raise ValueError(f"{who}: num_evals + guard = {want} with block_size = {block_size} needs a basis of {window} vectors; "
                         f"lanczos_block_smallest holds {rows} (2 (num_evals + guard) + 3 block_size <= {rows}, and max_basis <= {rows})")
    if bounds is not None:
        bounds = kpm._bounds(bounds, who)
        kpm._scaled_sigma(sigma, bounds[0], bounds[1], who)
    elif not math.isfinite(float(sigma)):
        raise ValueError(f"{who}: sigma = {sigma!r} is not finite")
    if isinstance(config_or_op, LocalOperator) or hasattr(config_or_op, "plan"):
        op = config_or_op
        if not op.plan.matrix.isHermitian:
            raise ValueError(f"{who}: the operator is not Hermitian (the filter needs a real spectrum)")
        if len(op.sizes) != 1:
            raise api.LsAmdError(f"{who}: one-partition plans only (this operator has {len(op.sizes)} partitions)")
    else:
        load = api.loadConfigFromYaml if isinstance(config_or_op, str) else api.loadConfigFromDict
        basis, h = load(config_or_op, hamiltonian=True)
        if not h.isHermitian:
            raise ValueError(f"{who}: the Hamiltonian is not Hermitian (the filter needs a real spectrum)")
        if dtype is None:
            dtype = torch.float64 if h.isReal and not api._complex_characters(basis) else torch.complex128
        reps, _ = api.enumerateStates(basis, 1)
        op = LocalOperator(h, reps, dtype)
    n = int(op.n_local)
    if want > n:
        raise ValueError(f"{who}: num_evals + guard = {want} exceeds the dimension {n} of the basis")
    if bounds is None:
        bounds = kpm._bounds(kpm.spectral_bounds(op), who)
        kpm._scaled_sigma(sigma, bounds[0], bounds[1], who)
    lo, hi = bounds
    sigma = float(sigma)
    before = op.matvecs
    if order is None:
        order = kpm.filter_order(want, n, None, bounds, cut=cut, sigma=sigma, op=op)
    order = int(order)
    fop = FilteredOperator(op, kpm.delta_filter(sigma, bounds, order), bounds)
    h_norm = max(abs(lo), abs(hi))
    t_ritz = 0.0

    def clock():
        if op.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    t1 = clock()
    inner = lanczos_block_smallest(fop, num_evals=want, block_size=int(block_size), eps=0.25 * float(eps), max_basis=max_basis,
                                   max_restarts=INTERIOR_MAX_RESTARTS, seed=seed, verbose=verbose)
    t_orth = clock() - t1 - fop.seconds
    m = len(inner.eigenvectors)
    Q = torch.stack(inner.eigenvectors)  # [m, n]: rows are vectors, as the solvers keep them
    del inner.eigenvectors[:]
    W = torch.empty_like(Q)
    cplx = Q.is_complex()

    def orthonormalise():
        for _ in range(2):
            G = (Q.conj() @ Q.t() if cplx else Q @ Q.t()).cpu().numpy()  # G[i, j] = <q_i|q_j>
            R = np.linalg.cholesky(0.5 * (G + G.conj().T)).conj().T      # G = R^H R
            Q.copy_(torch.as_tensor(np.linalg.inv(R).T, dtype=Q.dtype, device=Q.device) @ Q)

    def rayleigh_ritz():
        """Q <- the Ritz vectors of H in span Q (orthonormal rows), W <- H Q; -> (theta ascending, explicit residual norms)"""
        for s in range(0, m, 64):
            e = min(m, s + 64)
            op.matvec_block(Q[s:e].t(), W[s:e].t())
        Hs = (Q.conj() @ W.t() if cplx else Q @ W.t()).cpu().numpy()   # Hs[i, j] = <q_i|H q_j>
        theta, S = np.linalg.eigh(0.5 * (Hs + Hs.conj().T))
        St = torch.as_tensor(S.T, dtype=Q.dtype, device=Q.device)      # y_i = sum_j S[j, i] q_j
        Q.copy_(St @ Q)
        W.copy_(St @ W)
        res = torch.empty(m, dtype=torch.float64, device=Q.device)
        for i in range(m):
            res[i] = torch.linalg.vector_norm(W[i] - float(theta[i]) * Q[i])
        return theta, res.cpu().numpy()

    polish = 0
    while True:
        t1 = clock()
        orthonormalise()
        theta, res = rayleigh_ritz()
        op.check()
        t_ritz += clock() - t1
        near = np.sort(np.argsort(np.abs(theta - sigma), kind="stable")[:int(num_evals)])
        done = bool(np.all(res[near] <= float(eps) * h_norm))
        if verbose:
            print(f"[interior] order {order}, polish {polish}: theta = {theta[near]}, residuals = {res[near]}", flush=True)
        if done or polish >= int(max_polish):
            break
        for s in range(0, m, 64):
            e = min(m, s + 64)
            fop.matvec_block(Q[s:e].t(), W[s:e].t())
        Q, W = W, Q
        polish += 1
    vecs = [Q[int(i)].clone() for i in near]
    return InteriorResult([float(theta[i]) for i in near], vecs, [float(res[i]) for i in near], sigma, order, (lo, hi), fop.applications,
                          int(op.matvecs - before), polish, done, time.perf_counter() - t0, fop.seconds, t_orth, t_ritz,
                          int(inner.restarts),
                          fop.block_kernel(int(block_size)))


def diagonalize(config, num_evals: int = 1, eps: float = 1e-6, num_partitions: int = 1, dtype=None, output: str | None = None,
                max_basis: int = 24, verbose: bool = False, block_size: int = 1, sigma=None):
    """`Diagonalize.main` (Diagonalize.chpl:258-332) on one device: config (dict or YAML path) ->
    representatives (enumerated on the GPU; an existing HDF5 `output` that already holds basis/representatives is
    reused and extended, like makeBasisStates :227-246) ->
    eigenpairs; `output` (.npz) receives what the reference writes to its HDF5 groups:
    basis/representatives, hamiltonian/eigenvalues, hamiltonian/eigenvectors, hamiltonian/residuals.
    block_size (the reference's kMaxBlockSize, Diagonalize.chpl:172,192): 1 = lanczos_smallest; 2..16 = lanczos_block_smallest,
    which finds degenerate levels with their multiplicity (up to block_size).
    sigma: None, or a target energy: the num_evals levels NEAREST sigma (interior_eigenpairs with this block_size; one partition;
    -> InteriorResult), written to the same datasets."""
    import os

    import numpy as np
    import torch

    from . import api

    if isinstance(block_size, bool) or not isinstance(block_size, int) or not 1 <= block_size <= 16:
        raise ValueError(f"block_size = {block_size!r}: 1 <= block_size <= 16")
    if sigma is not None and num_partitions != 1:
        raise ValueError(f"diagonalize: sigma = {sigma!r} with num_partitions = {num_partitions}: interior eigenpairs "
                         "(interior_eigenpairs) run on one partition")
    if isinstance(config, str):
        basis, h = api.loadConfigFromYaml(config, hamiltonian=True)
    else:
        basis, h = api.loadConfigFromDict(config, hamiltonian=True)
    if sigma is not None and not h.isHermitian:
        raise ValueError("diagonalize: the Hamiltonian is not Hermitian (sigma: the interior solver needs a real spectrum)")
    dtype = dtype or torch.float64
    reps = None
    if output and output.endswith((".h5", ".hdf5")) and num_partitions == 1:
        # makeBasisStates (Diagonalize.chpl:227-246): representatives already stored in the output file are reused
        from . import hdf5

        if hdf5.has_dataset(output, "/basis/representatives"):
            stored = hdf5.read_dataset(output, "/basis/representatives").astype(np.uint64)
            # a stale file (another model, another sector, another Hamming weight, a truncated dataset) must not be
            # diagonalised silently.  The reference reuses stored representatives to skip an enumeration that takes its CPU path
            # hours; here the enumeration is a few seconds of GPU time even for chain_40_symm, so the stored array is simply
            # required to EQUAL what this basis enumerates to -- order, count and every state.
            fresh, _ = api.enumerateStates(basis, 1)
            ok = len(stored) == int(fresh[0].numel())
            if ok:
                ok = bool(torch.equal(torch.from_numpy(stored.view(np.int64)).cuda(), fresh[0]))
            del fresh
            if not ok:
                raise api.LsAmdError(f"halt: /basis/representatives of '{output}' does not belong to the configured basis "
                                     "(stale output file?); remove the dataset or the file")
            reps = [torch.from_numpy(stored.view(np.int64).copy()).cuda()]
            masks = torch.zeros(len(stored), dtype=torch.uint8, device="cuda")
    if reps is None:
        reps, masks = api.enumerateStates(basis, num_partitions)
    # one plan, hundreds of matvecs: what is left of HBM after the Krylov basis may hold the resolved packet streams
    # (ls_amd_plan_cache_slots; LS_AMD_SLOT_CACHE=0 keeps the solver matrix-free)
    n_total = sum(int(r_.numel()) for r_ in reps)
    if block_size > n_total:
        raise ValueError(f"block_size = {block_size} exceeds the dimension {n_total} of the basis")
    cache_bytes = 0
    # (LS_AMD_SLOT_CACHE has one meaning everywhere: bytes; 0 = off; set = the C plan applies it at creation, nothing to add here)
    if sigma is not None:
        pass  # (the interior solver keeps three blocks of num_evals + guard vectors next to the Lanczos basis: it stays matrix-free)
    elif num_partitions == 1 and os.environ.get("LS_AMD_SLOT_CACHE") is None:
        n_states = int(reps[0].numel())
        free, _total = torch.cuda.mem_get_info()
        if block_size == 1:
            reserve = (max_basis + 6) * n_states * (16 if dtype == torch.complex128 else 8) + (4 << 30)
        else:
            # the block basis (max(max_basis, 2 num_evals + 3 K) vectors), its extra block and one block of slack, the margin of the
            # single-vector solver, and the packet buffer of the block matvec (used for the rows the cache leaves out)
            mb = max(max_basis, 2 * num_evals + 3 * block_size)
            resolve = int(os.environ.get("LS_AMD_BLOCK_RESOLVE_BYTES", "0") or 0)
            resolve = resolve if resolve > 0 else (1 << 30)
            reserve = (mb + 2 * block_size + 6) * n_states * (16 if dtype == torch.complex128 else 8) + (4 << 30) + resolve
        cache_bytes = max(0, int(free) - reserve)
    op = LocalOperator(h, reps, dtype, slot_cache_bytes=cache_bytes)
    if verbose and op.cached_rows:
        print(f"[diagonalize] slot cache: {op.cached_rows} rows, {op.plan.slot_cache[1] / 1e9:.2f} GB", flush=True)
    if sigma is not None:
        r = interior_eigenpairs(op, sigma, num_evals=num_evals, eps=eps, block_size=block_size, max_basis=max_basis, verbose=verbose)
    elif block_size == 1:
        r = lanczos_smallest(op, num_evals=num_evals, eps=eps, max_basis=max_basis, verbose=verbose)
    else:
        r = lanczos_block_smallest(op, num_evals=num_evals, block_size=block_size, eps=eps, max_basis=max_basis, verbose=verbose)
    if output and output.endswith((".h5", ".hdf5")):
        # same groups/datasets as the reference's output file (Diagonalize.chpl:241,248-256)
        from . import hdf5

        to_block = lambda v: api.arrFromHashedToBlock(list(v.split(op.sizes)), masks) if num_partitions > 1 else v  # noqa: E731
        if any(v.is_complex() for v in r.eigenvectors):
            raise NotImplementedError("HDF5 output is implemented for real eigenvectors (the reference's eltType is real(64))")
        hdf5.write_datasets(output, append=True, datasets={
            "/basis/representatives": (api.arrFromHashedToBlock(reps, masks) if num_partitions > 1 else reps[0]).cpu().numpy().view(np.uint64),
            "/hamiltonian/eigenvalues": np.array(r.eigenvalues),
            "/hamiltonian/residuals": np.array(r.residual_norms),
        })
        # the eigenvectors go out block by block (writeDatasetAsBlocks, MyHDF5.chpl:303-333: every locale its own hyperslab of
        # the last dimension): the host holds one block at a time -- chain_40_symm vectors are 6.9 GB each
        n_states = int(sum(op.sizes)) if num_partitions > 1 else int(reps[0].numel())
        num_blocks = max(num_partitions, -(-n_states // (1 << 27)))
        hdf5.create_dataset(output, "/hamiltonian/eigenvectors", (len(r.eigenvectors), n_states), np.float64)
        for row, v in enumerate(r.eigenvectors):
            vb = to_block(v)
            for b in range(num_blocks):
                lo, hi = hdf5.block_range(n_states, num_blocks, b)
                hdf5.write_dataset_chunk(output, "/hamiltonian/eigenvectors", (row, lo), vb[lo:hi].cpu().numpy()[None, :])
    elif output:
        parts_to_block = lambda v: api.arrFromHashedToBlock(list(v.split(op.sizes)), masks) if num_partitions > 1 else v  # noqa: E731
        np.savez(
            output,
            **{
                "basis/representatives": (api.arrFromHashedToBlock(reps, masks) if num_partitions > 1 else reps[0]).cpu().numpy().view(np.uint64),
                "hamiltonian/eigenvalues": np.array(r.eigenvalues),
                "hamiltonian/residuals": np.array(r.residual_norms),
                "hamiltonian/eigenvectors": np.stack([parts_to_block(v).cpu().numpy() for v in r.eigenvectors]),
            },
        )
    return r


@dataclass
class SpectrumResult:
    """full_spectrum: every eigenvalue of one sector (ascending, numpy); the eigenvectors as the columns of a device (n, n) tensor
    over the representatives, or None; the representatives (device int64); n; wall seconds of the whole call"""
    eigenvalues: object
    eigenvectors: object
    representatives: object
    dimension: int
    seconds: float = 0.0


def _unprojected_dimension(basis):
    """the number of states of a basis without symmetries, from its quantum numbers alone (host only); None for a projected basis,
    whose dimension is known once its representatives are enumerated"""
    if basis.requiresProjection():
        return None
    L, n, up, kind = basis.numberSites(), basis.numberParticles(), basis.numberUp(), basis.particleType()
    if kind == 1:  # spinful fermions: (N, N_up) product basis, N alone over the 2 L modes, or everything
        if up >= 0 and n >= 0:
            return math.comb(L, up) * math.comb(L, n - up)
        return math.comb(2 * L, n) if n >= 0 else 4 ** L
    fixed = n if kind == 2 else up  # spinless fermions: particles; spins: the Hamming weight
    return math.comb(L, fixed) if fixed >= 0 else 2 ** L


def _refuse_dimension(n, max_dim, itemsize):
    if n > max_dim:
        raise ValueError(f"full_spectrum: the sector has {n} states, the dense matrix {n * n * itemsize} bytes; max_dim is {max_dim} "
                         "(the few lowest levels of a larger sector: diagonalize())")


def full_spectrum(config, eigenvectors: bool = False, dtype=None, max_dim: int = 32768):
    """Every eigenvalue (eigenvectors=True: and eigenvector) of the configured Hamiltonian (dict or YAML path) on its sector: the
    representatives are enumerated, the sector matrix is exported in O(nnz) (Operator.to_csr), made dense and handed to
    torch.linalg.eigvalsh / eigh on the device.  dtype None: float64 for a real operator and +-1 characters, else complex128.
    ValueError before anything is allocated for a Hamiltonian that is not Hermitian and for a sector of more than max_dim states
    (an unprojected basis is refused from its quantum numbers, before a device is asked for; a projected one once its
    representatives are counted); LsAmdError when the exported matrix is not Hermitian to 1e-12 max|H|."""
    import numpy as np
    import torch

    from . import api

    t0 = time.perf_counter()
    load = api.loadConfigFromYaml if isinstance(config, str) else api.loadConfigFromDict
    basis, h = load(config, hamiltonian=True)
    if not h.isHermitian:
        raise ValueError("full_spectrum: the Hamiltonian is not Hermitian (a dense Hermitian solver is used)")
    if isinstance(max_dim, bool) or not isinstance(max_dim, int) or max_dim < 1:
        raise ValueError(f"max_dim = {max_dim!r}: a positive integer")
    if dtype is None:
        dtype = torch.float64 if h.isReal and not api._complex_characters(basis) else torch.complex128
    itemsize = 16 if dtype in (torch.complex128, "c128") else 8
    known = _unprojected_dimension(basis)
    if known is not None:
        _refuse_dimension(known, max_dim, itemsize)
    reps, _ = api.enumerateStates(basis, 1)
    n = int(reps[0].numel())
    _refuse_dimension(n, max_dim, itemsize)
    H = h.to_dense(reps, dtype=dtype, max_bytes=max(8 << 30, 2 * n * n * itemsize))
    scale = float(H.abs().max()) if n else 0.0
    defect = float((H - H.mH).abs().max()) if n else 0.0
    if defect > 1e-12 * scale:
        raise api.LsAmdError(f"full_spectrum: the sector matrix is not Hermitian: max|H - H^+| = {defect:.3e}, max|H| = {scale:.3e}")
    if eigenvectors:
        vals, vecs = torch.linalg.eigh(H)
    else:
        vals, vecs = torch.linalg.eigvalsh(H), None
    vals = vals.cpu().numpy().astype(np.float64)
    return SpectrumResult(vals, vecs, reps[0], n, time.perf_counter() - t0)


def diagonalize_distributed(config, group=None, num_evals: int = 1, eps: float = 1e-6, dtype=None, output: str | None = None,
                            exchange: str = "auto", max_basis: int = 24, verbose: bool = False):
    """`Diagonalize.main` (Diagonalize.chpl:258-332) with one process per GPU: every rank enumerates the basis on its device,
    keeps its hash partition of the states and of the Lanczos vectors, the matvec goes through the C host's exchange
    (replicated-x for Hermitian operators, packets otherwise / on request), the reductions through RCCL, and the output file
    (HDF5, visible to every rank) is written block-distributed: /basis/representatives and /hamiltonian/eigenvectors [k, N]
    in global ascending order, every rank its own hyperslab, all ranks writing at once (MyHDF5.chpl:303-333;
    distributed.write_block_dataset), eigenvalues and residuals by rank 0.  An `output` that already holds
    /basis/representatives (an earlier run of this driver, or of the reference: makeBasisStates, Diagonalize.chpl:227-246) is
    extended, not truncated: every rank reads its block of the stored states (readDatasetAsBlocks), they must equal what
    the configured basis enumerates to, and the dataset is left as it is.
    Must be called by every rank of `group` (torch.distributed, backend "nccl")."""
    import numpy as np
    import torch
    import torch.distributed as dist

    from . import api, hdf5
    from .distributed import RcclDistributedOperator, RcclReplicatedOperator, hashed_to_block, write_block_dataset, write_hashed_vectors

    rank, world = dist.get_rank(group), dist.get_world_size(group)
    if isinstance(config, str):
        basis, h = api.loadConfigFromYaml(config, hamiltonian=True)
    else:
        basis, h = api.loadConfigFromDict(config, hamiltonian=True)
    dtype = dtype or torch.float64
    if output and not output.endswith((".h5", ".hdf5")):
        raise ValueError("diagonalize_distributed writes HDF5 (the block-distributed format of the reference)")
    parts, masks = api.enumerateStates(basis, world)
    my_reps = parts[rank]
    stored_basis = False
    if output:
        from .distributed import _broadcast_int

        # rank 0 looks (one decision for all ranks); -1 = no such dataset
        n_stored = _broadcast_int(hdf5.dataset_shape(output, "/basis/representatives")[-1]
                                  if rank == 0 and hdf5.has_dataset(output, "/basis/representatives") else None, group)
        if n_stored is not None:
            # the reference trusts the stored states to skip an enumeration that costs its CPU path hours; the enumeration
            # above is seconds of GPU time, so here they are CHECKED instead (like diagonalize()): a stale file -- another
            # model, sector or Hamming weight, a truncated dataset -- must not be extended silently.  Every rank compares
            # its own block, read by itself, with its block of the fresh enumeration.
            n = int(masks.numel())
            fresh = hashed_to_block(my_reps, masks, group)
            ok = n_stored == n
            if ok:
                mine = hdf5.read_dataset_block(output, "/basis/representatives", world, rank, np.uint64)
                ok = bool(torch.equal(torch.from_numpy(mine.view(np.int64)), fresh.cpu()))
            del fresh
            flag = torch.tensor([1 if ok else 0], dtype=torch.int64, device=my_reps.device if dist.get_backend(group) == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
            if not int(flag.item()):
                raise api.LsAmdError(f"halt: /basis/representatives of '{output}' does not belong to the configured basis "
                                     "(stale output file?); remove the dataset or the file")
            stored_basis = True
            if verbose and rank == 0:
                print(f"[diagonalize_distributed] /basis/representatives of '{output}': {n} states, verified, kept", flush=True)
    if exchange == "auto":
        # replicated x is the fast exchange, but its tables are O(N) on EVERY rank; the packets are the O(N / P) strategy and the
        # fallback when those tables do not fit next to the Krylov basis (exchange_memory_estimate; LS_AMD_EXCHANGE_HBM_CEILING)
        from .distributed import choose_exchange, exchange_memory_estimate

        free, _total = torch.cuda.mem_get_info() if my_reps.is_cuda else (1 << 62, 0)
        est = exchange_memory_estimate(int(masks.numel()), int(my_reps.numel()), world, 16 if dtype == torch.complex128 else 8,
                                       basis.requiresProjection(), h.numberOffDiagTerms(), krylov_vectors=max_basis + 4)
        exchange = choose_exchange(bool(h.isHermitian), est, int(free))
        if world > 1:  # one decision for all ranks: any rank without room for the replicated tables pulls everybody to the packets
            flag = torch.tensor([1 if exchange == "packets" else 0], dtype=torch.int64, device=my_reps.device if dist.get_backend(group) == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
            exchange = "packets" if int(flag.item()) else "replicated"
        if verbose and rank == 0:
            print(f"[diagonalize_distributed] exchange = {exchange} (per-rank HBM estimate: replicated {est['replicated'] / 1e9:.2f} GB, "
                  f"packets {est['packets'] / 1e9:.2f} GB, free {free / 1e9:.1f} GB)", flush=True)
    if exchange == "replicated":
        reps_global = api.arrFromHashedToBlock(parts, masks) if world > 1 else parts[0]
        op = RcclReplicatedOperator(h, reps_global, masks, dtype, group=group)
        del reps_global
        # one plan, hundreds of matvecs: this rank's rows keep their resolved packet streams in the HBM the Krylov basis leaves
        # (ls_amd_plan_cache_slots -- a local decision, no collective; rows that do not fit stay matrix-free; LS_AMD_SLOT_CACHE=0: off)
        plan = getattr(getattr(op, "engine", None), "plan", None)
        # (LS_AMD_SLOT_CACHE set: bytes, applied by ls_amd_repl_create itself -- 0 = off; unset: sized here)
        if plan is not None and hasattr(plan, "cache_slots") and my_reps.is_cuda and os.environ.get("LS_AMD_SLOT_CACHE") is None:
            free, _total = torch.cuda.mem_get_info()
            budget = int(free) - (max_basis + 6) * int(my_reps.numel()) * (16 if dtype == torch.complex128 else 8) - (4 << 30)
            if budget > 0:
                rows = plan.cache_slots(budget)
                if verbose and rows:
                    print(f"[diagonalize_distributed] rank {rank}: slot cache for {rows} rows, {plan.slot_cache[1] / 1e9:.2f} GB", flush=True)
    else:
        op = RcclDistributedOperator(h, my_reps, dtype, group=group)
    del parts
    r = lanczos_smallest(RankOperator(op, my_reps, dtype), num_evals=num_evals, eps=eps, max_basis=max_basis, verbose=verbose)
    if output:
        if rank == 0:
            # append: whatever else the file holds stays; hamiltonian/* of an earlier run is replaced (Diagonalize.chpl:248-256)
            hdf5.write_datasets(output, {"/hamiltonian/eigenvalues": np.array(r.eigenvalues),
                                         "/hamiltonian/residuals": np.array(r.residual_norms)}, append=os.path.exists(output))
        dist.barrier(group)
        if not stored_basis:
            write_block_dataset(output, "/basis/representatives", (int(masks.numel()),), np.uint64,
                                (hashed_to_block(my_reps, masks, group).cpu().numpy().view(np.uint64) for _ in range(1)), group)
        write_hashed_vectors(output, "/hamiltonian/eigenvectors", list(r.eigenvectors), masks, group)
    return r
