// k_cross_blk_t.hpp -- the block form of the cross-sector pull kernel: Y[:, k] = A X[:, k] for the K columns of
// an (n_src, K) block, k_cross_pull_blk.  k_cross_blk.hip instantiates it for the bases without permutation signs (FERMI = false),
// k_cross_blk_fermi.hip for the projected fermionic ones (FERMI = true; "k_cross_pull_blk_fermi").  The formulation is that of
// k_cross_pull (k_cross_t.hpp), whose stages A, B1 and the look-up of B2 are repeated here -- they do not depend on x -- with the slot
// allocation of A and the core of B1 as the same functions (cross_wave_slot, sector_project) and the look-up word for word:
// one target row per thread, the adjoint's flip-mask groups expanded into the LDS packet list kGCCross groups per pass, every packet
// projected into the source basis and resolved to (source index, coefficient) ONCE.  Only the tail of B2 differs: a resolved packet
// gathers a chunk of kCrossKC columns of X -- with interleaved columns (strides (K, 1)) 64 B (f64) or 128 B (c128) of consecutive
// memory -- and adds coef * X[idx, c] to the kCrossKC accumulators of its row.  A block handles the columns
// [kCrossKC blockIdx.y, kCrossKC blockIdx.y + kCrossKC), as k_project_pull does: a block wider than one chunk repeats the stages per
// chunk of 8, not per column.  Y is assigned, one plain store per (row, column); no global atomics.
// The accumulators live in LDS as kCrossKC (x 2 for c128) planes of kBlock doubles, plane p of row r at s_acc[p * kBlock + r]: the
// packets of one group took consecutive slots for consecutive rows in stage A, so the lanes of a wave mostly add to consecutive
// doubles of one plane (no bank conflict beyond the two passes a 64 x 8 B access takes anyway); the r * KC + c pattern would put
// consecutive rows 64 / 128 B apart, on two of the banks (measured 20-31 % slower).  c128: 8 K packets'
// states + 16 K coefficients + 2 K rows + 32 K accumulators = 58 KB of static LDS, two workgroups per CU.
#pragma once
#include <cstdlib>

#include "k_cross_t.hpp"

constexpr int kCrossKC = 8; // columns per block: accumulators per row, and loads in flight per packet

// X[idx, c0 + c] for the columns of the chunk into v, then coef * v into the row's accumulators (FULL: all kCrossKC columns, no
// column predicate)
template <bool CPLX, bool FULL>
__device__ __forceinline__ void cross_blk_load(double const *__restrict__ x, int64_t at, int64_t x_col, int kc, double (&vr)[kCrossKC],
                                               double (&vi)[kCrossKC]) {
#pragma unroll
    for (int c = 0; c < kCrossKC; ++c) {
        vr[c] = 0.0; vi[c] = 0.0;
        if (FULL || c < kc) {
            if (CPLX) { const double2 v = reinterpret_cast<double2 const *>(x)[at + (int64_t)c * x_col]; vr[c] = v.x; vi[c] = v.y; }
            else vr[c] = x[at + (int64_t)c * x_col];
        }
    }
}
template <bool CPLX, bool FULL>
__device__ __forceinline__ void cross_blk_add(double *acc, int kc, double hr, double hi, double const (&vr)[kCrossKC],
                                              double const (&vi)[kCrossKC]) {
#pragma unroll
    for (int c = 0; c < kCrossKC; ++c) {
        if (!(FULL || c < kc)) continue;
        if (CPLX) {
            atomicAdd(&acc[(2 * c) * kBlock], hr * vr[c] - hi * vi[c]);
            atomicAdd(&acc[(2 * c + 1) * kBlock], hr * vi[c] + hi * vr[c]);
        } else atomicAdd(&acc[c * kBlock], hr * vr[c]);
    }
}

template <typename W, bool PM1, bool CPLX, bool REAL, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_cross_pull_blk(int n_groups, lsk_group const *__restrict__ groups,
                                                           lsk_term const *__restrict__ terms, lsk_basis sbs,
                                                           lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                           int64_t n_dst, uint64_t const *__restrict__ dst_reps,
                                                           double const *__restrict__ dst_norms, int K, double const *__restrict__ x,
                                                           int64_t x_row, int64_t x_col, double *__restrict__ y, int64_t y_row,
                                                           int64_t y_col, double tiny, int *err) {
    constexpr bool RC = REAL && PM1; // the coefficient stays real: real terms and +-1 source characters
    constexpr int NP = kCrossKC * (CPLX ? 2 : 1); // accumulator planes
    __shared__ uint64_t s_beta[kCapCross];
    __shared__ double s_coef[kCapCross * (RC ? 1 : 2)];
    __shared__ uint16_t s_row[kCapCross];
    __shared__ double s_acc[NP * kBlock];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const bool project = sbs.proj != LSK_PROJ_NONE;
    const bool table = gt.entries != nullptr;
    const int c0 = (int)blockIdx.y * kCrossKC;
    const int kc = K - c0 < kCrossKC ? K - c0 : kCrossKC;
    if (kc <= 0) return;
    const bool full = kc == kCrossKC;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n_dst; t0 += (int64_t)gridDim.x * kBlock) {
        const int64_t i = t0 + tid;
        const bool valid = i < n_dst;
        uint64_t a = 0;
        double inv_na = 0.0;
        if (valid) {
            a = dst_reps[i];
            const double na = dst_norms[i];
            inv_na = na > 0.0 ? 1.0 / na : 0.0;
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) s_acc[p * kBlock + tid] = 0.0; // (the stores of the tile before are behind its closing barrier)
        for (int g0 = 0; g0 < n_groups; g0 += kGCCross) {
            if (tid == 0) s_n = 0;
            __syncthreads();
            // ---- stage A: the adjoint's groups of every row -> packets (state, conj(c) / n2(r'), row) ------------------
            const int g1 = min(g0 + kGCCross, n_groups);
            for (int g = g0; g < g1; ++g) {
                lsk_group const G = groups[g];
                double cr = 0.0, ci = 0.0;
                if (valid) term_sum<REAL>(terms, G.begin, G.end, a, cr, ci);
                const bool act = valid && (fabs(cr) > tiny || (!REAL && fabs(ci) > tiny));
                const int slot = cross_wave_slot(act, lane, &s_n);
                if (act) {
                    s_beta[slot] = a ^ G.x;
                    s_row[slot] = (uint16_t)tid;
                    if (RC) s_coef[slot] = cr * inv_na;
                    else { s_coef[2 * slot] = cr * inv_na; s_coef[2 * slot + 1] = -ci * inv_na; }
                }
            }
            __syncthreads();
            const int n = s_n;
            // ---- stage B1: project every packet into the SOURCE basis (general K4: minimum, character, stabiliser norm) --
            if (project) {
                for (int e = tid; e < n; e += kBlock) {
                    W rep; double chr, chi, nb;
                    if (!sector_project<W, PM1, FERMI>(sbs, elems, (W)s_beta[e], rep, chr, chi, nb)) { s_row[e] = 0xffff; continue; }
                    s_beta[e] = (uint64_t)rep;
                    if (RC) s_coef[e] = s_coef[e] * chr * nb;
                    else { // times chi1(g0) = conj(chr, chi), times n1(rep)
                        const double hr = s_coef[2 * e], hi = s_coef[2 * e + 1];
                        s_coef[2 * e] = (hr * chr + hi * chi) * nb;
                        s_coef[2 * e + 1] = (hi * chr - hr * chi) * nb;
                    }
                }
            }
            // ---- stage B2: representative -> source index, once per packet; then the chunk of X (a thread's loads issued before
            // any is used) into the accumulators of the packet's row ---------------------------------------------------------
            {
                uint64_t key[kGCCross], bucket[kGCCross];
                uint32_t tag[kGCCross];
                ulonglong2 first[kGCCross];
                int64_t idx[kGCCross];
                bool live[kGCCross];
#pragma unroll
                for (int k = 0; k < kGCCross; ++k) {
                    const int e = tid + k * kBlock;
                    live[k] = e < n && s_row[e] != 0xffff;
                    key[k] = live[k] ? s_beta[e] : 0;
                    idx[k] = -1;
                    bucket[k] = 0; tag[k] = 0;
                    first[k] = make_ulonglong2(kGtEmpty, kGtEmpty);
                    if (live[k] && table && !(gt.L < 64 && (key[k] >> gt.L) != 0)) {
                        gt_split(gt, key[k], bucket[k], tag[k]);
                        first[k] = *(ulonglong2 const *)(gt.entries + 2 * bucket[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < kGCCross; ++k) {
                    if (!live[k]) continue;
                    if (table) {
                        const uint32_t pay = gt_resolve(gt, gt.entries, bucket[k], tag[k], first[k]);
                        idx[k] = pay == 0xffffffffu ? -1 : (int64_t)pay;
                    } else idx[k] = cross_index(six, key[k]);
                    if (idx[k] < 0 || idx[k] >= six.count) { idx[k] = -1; atomicExch(err, 1); } // an image that is not in the source basis
                }
                double vr[kGCCross][kCrossKC], vi[kGCCross][kCrossKC];
#pragma unroll
                for (int k = 0; k < kGCCross; ++k) {
                    if (idx[k] < 0) continue;
                    const int64_t at = idx[k] * x_row + (int64_t)c0 * x_col;
                    if (full) cross_blk_load<CPLX, true>(x, at, x_col, kc, vr[k], vi[k]);
                    else cross_blk_load<CPLX, false>(x, at, x_col, kc, vr[k], vi[k]);
                }
#pragma unroll
                for (int k = 0; k < kGCCross; ++k) {
                    if (idx[k] < 0) continue;
                    const int e = tid + k * kBlock;
                    double hr, hi = 0.0;
                    if (RC) hr = s_coef[e]; else { hr = s_coef[2 * e]; hi = s_coef[2 * e + 1]; }
                    double *const acc = &s_acc[s_row[e]];
                    if (full) cross_blk_add<CPLX, true>(acc, kc, hr, hi, vr[k], vi[k]);
                    else cross_blk_add<CPLX, false>(acc, kc, hr, hi, vr[k], vi[k]);
                }
            }
            __syncthreads();
        }
        if (valid) {
            const int64_t at = i * y_row + (int64_t)c0 * y_col;
#pragma unroll
            for (int c = 0; c < kCrossKC; ++c) {
                if (c >= kc) break;
                if (CPLX) reinterpret_cast<double2 *>(y)[at + (int64_t)c * y_col] = make_double2(s_acc[(2 * c) * kBlock + tid], s_acc[(2 * c + 1) * kBlock + tid]);
                else y[at + (int64_t)c * y_col] = s_acc[c * kBlock + tid];
            }
        }
        __syncthreads();
    }
}

// row blocks of a launch: what is co-resident, shared among the column chunks; LS_AMD_CROSS_BLOCKS=<k>, read at every launch, lowers
// the ceiling (tests: several tiles per block at sizes a dense reference reaches)
template <typename Kern>
static int cross_blk_grid(Kern kernel, int64_t work_blocks, int chunks) {
    int64_t g = resident_grid(kernel, work_blocks * chunks) / chunks;
    if (char const *e = getenv("LS_AMD_CROSS_BLOCKS")) { const long k = atol(e); if (k >= 1 && k < g) g = k; }
    if (g > work_blocks) g = work_blocks;
    return (int)(g < 1 ? 1 : g);
}

// the launch of both units: the instantiation matrix of k_cross_pull, {32, 64-bit words} x {f64 (real terms, +-1 characters) |
// c128 x {+-1, complex characters} x {real, complex terms}}: 10 kernels per unit
template <bool FERMI>
static int cross_blk_launch(char const *who, int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src,
                            lsk_index six, lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, int K,
                            void const *x, int64_t x_row, int64_t x_col, void *y, int64_t y_row, int64_t y_col, double tiny, int *d_err,
                            void *stream) {
    if (K < 1 || K > 64) { snprintf(g_err, sizeof(g_err), "%s: K = %d columns, outside [1, 64]", who, K); return -1; }
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (!cplx && !(is_real && src.chars_pm1)) { snprintf(g_err, sizeof(g_err), "%s: f64 needs a real operator and +-1 characters", who); return -1; }
    const int64_t work_blocks = (n_dst + kBlock - 1) / kBlock;
    const int chunks = (K + kCrossKC - 1) / kCrossKC;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(1, (unsigned)chunks), b(kBlock);
#define LSK_CXB_ONE(W, PM1, CPLX, REAL)                                                                                                  \
    do {                                                                                                                                 \
        g.x = (unsigned)cross_blk_grid(k_cross_pull_blk<W, PM1, CPLX, REAL, FERMI>, work_blocks, chunks);                                \
        hipLaunchKernelGGL((k_cross_pull_blk<W, PM1, CPLX, REAL, FERMI>), g, b, 0, s, n_groups, groups, terms, src, src.elems, six, gt,  \
                           n_dst, dst_reps, dst_norms, K, (double const *)x, x_row, x_col, (double *)y, y_row, y_col, tiny, d_err);      \
    } while (0)
#define LSK_CXB_LAUNCH(W)                                                                                                                \
    do {                                                                                                                                 \
        if (!cplx) LSK_CXB_ONE(W, true, false, true);                                                                                    \
        else if (src.chars_pm1) { if (is_real) LSK_CXB_ONE(W, true, true, true); else LSK_CXB_ONE(W, true, true, false); }               \
        else { if (is_real) LSK_CXB_ONE(W, false, true, true); else LSK_CXB_ONE(W, false, true, false); }                                \
    } while (0)
    if (src.number_sites <= 32) LSK_CXB_LAUNCH(uint32_t); else LSK_CXB_LAUNCH(uint64_t);
#undef LSK_CXB_LAUNCH
#undef LSK_CXB_ONE
    LSK_LAUNCH_CHECK();
    return 0;
}
