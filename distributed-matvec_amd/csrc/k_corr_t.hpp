// k_corr_t.hpp -- the hopping kernel k_corr_hop of the two-point correlation matrices as a template header:
// k_corr.hip instantiates it for the bases without permutation signs (FERMI = false), k_corr_fermi.hip for the projected fermionic
// ones (FERMI = true; the plans call that family "k_corr_hop_fermi").
//     R[i][j] = sum over the rows r with bit i set and bit j clear of  conj(psi_r) / n(r) * <s|psi>,   s = r ^ 1 << i ^ 1 << j
// with <s|psi> = chi(g0) [sign(g0, s)] n(rep s) psi[index(rep s)], g0 s = rep s: the matrix element k_cross_pull computes in its
// stages B1 / B2, with source = target (B1 through the same function, sector_project of k_cross_t.hpp).  It is the row loop of
// k_cross_pull; a few ordered pairs (i, j) per pass, uniform across the block, take the place of the flip-mask groups.  What
// differs from there:
//   - the packet list is compacted in a FIXED order (pair, then wave, then lane: the counts of every (pair, wave) go through LDS
//     and every thread takes its offsets from their prefix sums), so the packets of a pair lie one after another and a packet
//     does not depend on the order in which the waves arrive;
//   - a packet's product is not added to its row but written back to its slot, and one wave per pair sums the slots of the pair in
//     ascending order (lane-strided, then a butterfly over the lanes): one value per (tile, pair), added to the block's partial
//     by the one lane that owns the pair -- no atomics anywhere, equal inputs give equal bytes.
// On fermionic bases (jw != 0, projected or not) a packet carries the Jordan-Wigner sign (-1)^popcount(r & between(i, j)), so
// that the pair is c+_i c_j in the mode order of the state word.
#pragma once
#include <cstdlib>

#include "k_cross_t.hpp" // sector_project, cross_index, and through it lsk_dev.hpp / lsk_fermi.hpp

constexpr int kCorrPP = 8;                   // ordered pairs per pass
constexpr int kCorrCap = kBlock * kCorrPP;   // packets a pass of one tile can generate
constexpr int kCorrWaves = kBlock / 64;
constexpr int kCorrMaxBlocks = 1024;         // blocks of either kernel = rows of the partial sums

// blocks of a launch over n rows: one per tile of kBlock rows up to kCorrMaxBlocks, grid-stride beyond -- every block has a tile, so it
// writes its partials.  LS_AMD_CORR_BLOCKS=<k> lowers the ceiling (tests: several tiles per block at sizes a dense reference reaches).
static int corr_grid(int64_t n) {
    int64_t cap = kCorrMaxBlocks;
    if (char const *e = getenv("LS_AMD_CORR_BLOCKS")) { const long k = atol(e); if (k >= 1 && k < cap) cap = k; }
    const int64_t tiles = (n + kBlock - 1) / kBlock;
    return (int)(tiles < 1 ? 1 : (tiles > cap ? cap : tiles));
}

template <typename W, bool PM1, bool CPLX, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_corr_hop(lsk_basis bs, lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                     int jw, int n_pairs, uint16_t const *__restrict__ pairs, int64_t n,
                                                     uint64_t const *__restrict__ reps, double const *__restrict__ norms,
                                                     double const *__restrict__ psi, double *__restrict__ partial, int *err) {
    constexpr int NC = CPLX ? 2 : 1; // doubles of a value (complex characters come with c128 vectors only)
    __shared__ W s_beta[kCorrCap];
    __shared__ double s_val[kCorrCap * NC];  // B1: chi(g0) n(rep), one double when the characters are +-1; B2: the packet's product
    __shared__ uint16_t s_row[kCorrCap];     // row of the tile | Jordan-Wigner parity << 8; 0xffff: zero norm
    __shared__ double s_rc[kBlock * NC];     // conj(psi_r) / n(r) of the tile's rows
    __shared__ int s_cnt[kCorrPP * kCorrWaves];
    __shared__ int s_off[kCorrPP + 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const bool project = bs.proj != LSK_PROJ_NONE;
    const bool table = gt.entries != nullptr;
    double *const mine = partial + (size_t)blockIdx.x * n_pairs * NC;
    bool first = true;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n; t0 += (int64_t)gridDim.x * kBlock, first = false) {
        const int64_t i = t0 + tid;
        const bool valid = i < n;
        W a = 0;
        {
            double cr = 0.0, ci = 0.0;
            if (valid) {
                a = (W)reps[i];
                const double na = norms[i];
                const double inv_na = na > 0.0 ? 1.0 / na : 0.0;
                if (CPLX) { cr = psi[2 * i] * inv_na; ci = -psi[2 * i + 1] * inv_na; } else cr = psi[i] * inv_na;
            }
            if (CPLX) { s_rc[2 * tid] = cr; s_rc[2 * tid + 1] = ci; } else s_rc[tid] = cr;
        }
        for (int p0 = 0; p0 < n_pairs; p0 += kCorrPP) {
            // the block's partial of the two pairs this wave will sum: asked for now, used after the pass
            double old[2][NC];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int p = p0 + wave + h * kCorrWaves;
#pragma unroll
                for (int c = 0; c < NC; ++c) old[h][c] = (!first && lane == 0 && p < n_pairs) ? mine[(size_t)p * NC + c] : 0.0;
            }
            // ---- stage A: the active rows of every pair, counted per (pair, wave) ... ---------------------------------------
            uint32_t act = 0;
#pragma unroll
            for (int q = 0; q < kCorrPP; ++q) {
                bool on = false;
                if (p0 + q < n_pairs) {
                    const uint32_t pr = pairs[p0 + q];
                    on = valid && ((a >> (pr & 0xff)) & 1) != 0 && ((a >> (pr >> 8)) & 1) == 0;
                }
                const unsigned long long ball = __ballot(on);
                if (lane == 0) s_cnt[q * kCorrWaves + wave] = __popcll(ball);
                act |= (uint32_t)on << q;
            }
            __syncthreads();
            // ---- ... and written at the prefix sums of the counts: packets (image, row | parity) in (pair, wave, lane) order ---
            int run = 0;
#pragma unroll
            for (int q = 0; q < kCorrPP; ++q) {
                if (tid == 0) s_off[q] = run;
                int base = 0;
#pragma unroll
                for (int w = 0; w < kCorrWaves; ++w) {
                    if (w == wave) base = run;
                    run += s_cnt[q * kCorrWaves + w];
                }
                const bool on = (act >> q) & 1;
                const unsigned long long ball = __ballot(on);
                if (on) {
                    const uint32_t pr = pairs[p0 + q];
                    const int bi = pr & 0xff, bj = pr >> 8;
                    const int slot = base + __popcll(ball & ((1ULL << lane) - 1));
                    int par = 0;
                    if (jw) {
                        const int lo = min(bi, bj), hi = max(bi, bj);
                        const W between = (W)((((W)1 << hi) - 1) & ~((((W)1 << lo) << 1) - 1));
                        par = fermi_popc<W>((W)(a & between)) & 1;
                    }
                    s_beta[slot] = (W)(a ^ ((W)1 << bi) ^ ((W)1 << bj));
                    s_row[slot] = (uint16_t)(tid | (par << 8));
                }
            }
            if (tid == 0) s_off[kCorrPP] = run;
            __syncthreads();
            const int np = run; // (every thread summed the same counts)
            // ---- stage B1: project every packet (sector_project, k_cross_t.hpp) ---------------------------------------------------
            if (project) {
                for (int e = tid; e < np; e += kBlock) {
                    W rep; double chr, chi, nb;
                    if (!sector_project<W, PM1, FERMI>(bs, elems, s_beta[e], rep, chr, chi, nb)) { s_row[e] = 0xffff; continue; }
                    s_beta[e] = rep;
                    if (PM1) s_val[NC * e] = chr * nb;
                    else { s_val[2 * e] = chr * nb; s_val[2 * e + 1] = -chi * nb; } // chi(g0) = conj(chr, chi), times n(rep)
                }
            }
            // ---- stage B2: representative -> index, the gathers, and the packet's product back into its slot -------------------
            // (slot e is read and written by thread e % kBlock alone, in B1 and here)
            for (int e0 = 0; e0 < np; e0 += 4 * kBlock) {
                uint64_t key[4], bucket[4];
                uint32_t tag[4];
                ulonglong2 head[4];
                int64_t idx[4];
                bool live[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = e0 + tid + k * kBlock;
                    live[k] = e < np && s_row[e] != 0xffff;
                    key[k] = live[k] ? (uint64_t)s_beta[e] : 0;
                    idx[k] = -1;
                    bucket[k] = 0; tag[k] = 0;
                    head[k] = make_ulonglong2(kGtEmpty, kGtEmpty);
                    if (live[k] && table && !(gt.L < 64 && (key[k] >> gt.L) != 0)) {
                        gt_split(gt, key[k], bucket[k], tag[k]);
                        head[k] = *(ulonglong2 const *)(gt.entries + 2 * bucket[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!live[k]) continue;
                    if (table) {
                        const uint32_t pay = gt_resolve(gt, gt.entries, bucket[k], tag[k], head[k]);
                        idx[k] = pay == 0xffffffffu ? -1 : (int64_t)pay;
                    } else idx[k] = cross_index(six, key[k]);
                    if (idx[k] < 0 || idx[k] >= n) { idx[k] = -1; atomicExch(err, 1); } // an image that is not among the representatives
                }
                double xr[4], xi[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    xr[k] = 0.0; xi[k] = 0.0;
                    if (idx[k] >= 0) {
                        if (CPLX) { xr[k] = psi[2 * idx[k]]; xi[k] = psi[2 * idx[k] + 1]; } else xr[k] = psi[idx[k]];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = e0 + tid + k * kBlock;
                    if (e >= np) continue;
                    double vr = 0.0, vi = 0.0;
                    if (idx[k] >= 0) {
                        const int r = s_row[e] & 0xff;
                        double fr = 1.0, fi = 0.0;
                        if (project) { fr = s_val[NC * e]; if (!PM1) fi = s_val[2 * e + 1]; }
                        if (s_row[e] & 0x100) { fr = -fr; fi = -fi; }
                        if (CPLX) {
                            const double cr = s_rc[2 * r], ci = s_rc[2 * r + 1];
                            const double gr = PM1 ? cr * fr : cr * fr - ci * fi, gi = PM1 ? ci * fr : cr * fi + ci * fr;
                            vr = gr * xr[k] - gi * xi[k];
                            vi = gr * xi[k] + gi * xr[k];
                        } else vr = s_rc[r] * fr * xr[k];
                    }
                    if (CPLX) { s_val[2 * e] = vr; s_val[2 * e + 1] = vi; } else s_val[e] = vr;
                }
            }
            __syncthreads();
            // ---- the sum of every pair's slots, in a fixed order; one lane adds it to the block's partial ------------------------
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = wave + h * kCorrWaves;
                const int p = p0 + q;
                if (p >= n_pairs) continue; // (uniform across the wave)
                const int b = s_off[q], e1 = s_off[q + 1];
                double sr = 0.0, si = 0.0;
                for (int e = b + lane; e < e1; e += 64) {
                    if (CPLX) { sr += s_val[2 * e]; si += s_val[2 * e + 1]; } else sr += s_val[e];
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    sr += __shfl_xor(sr, d);
                    if (CPLX) si += __shfl_xor(si, d);
                }
                if (lane == 0) {
                    mine[(size_t)p * NC] = old[h][0] + sr;
                    if (CPLX) mine[(size_t)p * NC + 1] = old[h][NC - 1] + si;
                }
            }
            __syncthreads();
        }
    }
}

template <bool FERMI>
static int corr_hop_launch(lsk_basis bs, lsk_index six, lsk_gtab gt, int jw, int n_pairs, uint16_t const *pairs, int cplx, int64_t n,
                           uint64_t const *reps, double const *norms, void const *psi, double *partial, double *out, int *d_err,
                           void *stream) {
    if (n <= 0 || n_pairs <= 0) return 0;
    if (!cplx && !bs.chars_pm1) { snprintf(g_err, sizeof(g_err), "%s: f64 needs +-1 characters", __func__); return -1; }
    if (bs.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected basis is looked up by its index", __func__); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int blocks = corr_grid(n);
    dim3 g(blocks), b(kBlock);
    // (no more blocks than are resident at once -- 2 to 5 per CU by the LDS of the kind: a surplus block would run behind the others)
#define LSK_CH_ONE(W, PM1, CPLX)                                                                                                         \
    do {                                                                                                                                 \
        g.x = resident_grid(k_corr_hop<W, PM1, CPLX, FERMI>, blocks);                                                                    \
        hipLaunchKernelGGL((k_corr_hop<W, PM1, CPLX, FERMI>), g, b, 0, s, bs, bs.elems, six, gt, jw, n_pairs, pairs, n, reps, norms,     \
                           (double const *)psi, partial, d_err);                                                                         \
    } while (0)
    // {32, 64-bit words} x {f64 (+-1 characters) | c128 x {+-1, complex characters}}: 6 kernels per family
#define LSK_CH_LAUNCH(W)                                                                                                                 \
    do {                                                                                                                                 \
        if (!cplx) LSK_CH_ONE(W, true, false);                                                                                           \
        else if (bs.chars_pm1) LSK_CH_ONE(W, true, true);                                                                                \
        else LSK_CH_ONE(W, false, true);                                                                                                 \
    } while (0)
    if (bs.number_sites <= 32) LSK_CH_LAUNCH(uint32_t); else LSK_CH_LAUNCH(uint64_t);
#undef LSK_CH_LAUNCH
#undef LSK_CH_ONE
    LSK_LAUNCH_CHECK();
    return lsk_corr_sum((int)g.x, n_pairs * (cplx ? 2 : 1), partial, out, stream);
}
