// k_expect_t.hpp -- the row kernel k_expect of the expectation values of arbitrary operators on a sector state
// as a template header: k_expect.hip instantiates it for the bases without permutation signs (FERMI = false), k_expect_fermi.hip for
// the projected fermionic ones (FERMI = true; the plans call that family "k_expect_fermi").
//     R[u] = sum over the rows r with r & m_u == r_u of  (-1)^popcount(r & s_u) conj(psi_r) / n(r) * <r ^ x_u|psi>
// for every unique device term u = (m, r, x, s) of the batch (row-wise orientation, coefficient 1: the host holds the coefficients).
// It is k_corr_hop (k_corr_t.hpp) with "item = any term" in the place of "item = ordered pair": the same tiles, the same stages B1 / B2
// (projection of an image by sector_project, look-up, four look-ups in flight), the same error flag, one partial per (block, item) and the sum over the
// blocks in block order by lsk_corr_sum.  What differs from there:
//   - a PACKET belongs to a flip-mask group, not to a term: the image r ^ x is projected and looked up once, and its product
//     conj(psi_r) / n(r) <r ^ x|psi> serves every term of the group.  The row's factor travels in the packet's slot from stage A on,
//     so the tile keeps its words in LDS where k_corr_hop keeps that factor, and the residency stays what k_corr_hop has.  A row
//     emits the packet of a group when it passes the group's common projector (the mask bits all of its terms agree on) and the
//     image keeps the conserved numbers of the basis (Hamming weight / particle number, the numbers of both species on the
//     (N, N_up) basis); an image that leaves them contributes exactly zero and raises no error;
//   - the group x = 0 is neither projected nor looked up: its product is |psi_r|^2;
//   - after B2 one wave per term sums the slots of the term's group in ascending slot order (lane-strided, then the butterfly); a
//     slot counts when the row's word -- the tile's words stay in LDS -- passes the term's own (m, r), with the sign
//     (-1)^popcount(word & s).  No atomics anywhere: equal inputs give equal bytes.
// Every Jordan-Wigner and permutation sign of a fermionic term is inside s and the host's coefficient already, so FERMI switches the
// signed projection of B1 and nothing else.
#pragma once
#include "k_corr_t.hpp" // kCorrPP, kCorrCap, kCorrWaves, corr_grid; through it k_cross_t.hpp: sector_project, cross_index

template <typename W, bool PM1, bool CPLX, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_expect(lsk_basis bs, lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                   lsk_expect_cons cons, int n_groups, lsk_expect_group const *__restrict__ groups,
                                                   lsk_expect_term const *__restrict__ terms, int term0, int64_t n,
                                                   uint64_t const *__restrict__ reps, double const *__restrict__ norms,
                                                   double const *__restrict__ psi, double *__restrict__ partial, int n_partial, int *err) {
    constexpr int NC = CPLX ? 2 : 1;
    constexpr uint16_t kDead = 0xffff;  // zero norm: contributes nothing
    constexpr uint16_t kDiag = 0x0200;  // packet of the group x = 0: s_val holds |psi_r|^2 since stage A
    __shared__ W s_beta[kCorrCap];
    __shared__ double s_val[kCorrCap * NC];  // A: conj(psi_r) / n(r) of the packet's row; B1: times chi(g0) n(rep); B2: the product
    __shared__ uint16_t s_row[kCorrCap];     // row of the tile | kDiag; kDead
    __shared__ W s_word[kBlock];             // the tile's words, for the per-term tests
    __shared__ int s_cnt[kCorrPP * kCorrWaves];
    __shared__ int s_off[kCorrPP + 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const bool project = bs.proj != LSK_PROJ_NONE;
    const bool table = gt.entries != nullptr;
    double *const mine = partial + (size_t)blockIdx.x * n_partial * NC;
    const W low = cons.half > 0 ? (W)((((W)1 << (cons.half - 1)) << 1) - 1) : (W)0;
    bool first = true;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n; t0 += (int64_t)gridDim.x * kBlock, first = false) {
        const int64_t i = t0 + tid;
        const bool valid = i < n;
        W a = 0;
        double p2 = 0.0, cr = 0.0, ci = 0.0; // |psi_r|^2; conj(psi_r) / n(r)
        {
            if (valid) {
                a = (W)reps[i];
                const double na = norms[i];
                const double inv_na = na > 0.0 ? 1.0 / na : 0.0;
                if (CPLX) {
                    const double re = psi[2 * i], im = psi[2 * i + 1];
                    cr = re * inv_na; ci = -im * inv_na; p2 = re * re + im * im;
                } else { const double re = psi[i]; cr = re * inv_na; p2 = re * re; }
            }
            s_word[tid] = a;
        }
        for (int g0 = 0; g0 < n_groups; g0 += kCorrPP) {
            // ---- stage A: the rows that emit a packet for every group of the pass, counted per (group, wave) ... -----------------
            uint32_t act = 0;
#pragma unroll
            for (int q = 0; q < kCorrPP; ++q) {
                bool on = false;
                if (g0 + q < n_groups) {
                    lsk_expect_group const G = groups[g0 + q];
                    const W b = (W)(a ^ (W)G.x);
                    on = valid && (W)(a & (W)G.cm) == (W)G.cr;
                    if (cons.weight >= 0) on = on && fermi_popc<W>(b) == cons.weight;
                    if (cons.half > 0) on = on && fermi_popc<W>((W)(b & low)) == cons.n_up && fermi_popc<W>((W)(b & ~low)) == cons.n_dn;
                }
                const unsigned long long ball = __ballot(on);
                if (lane == 0) s_cnt[q * kCorrWaves + wave] = __popcll(ball);
                act |= (uint32_t)on << q;
            }
            __syncthreads();
            // ---- ... and written at the prefix sums of the counts: packets (image, row) in (group, wave, lane) order -------------
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
                    const W x = (W)groups[g0 + q].x;
                    const int slot = base + __popcll(ball & ((1ULL << lane) - 1));
                    s_beta[slot] = (W)(a ^ x);
                    s_row[slot] = (uint16_t)(x == 0 ? tid | kDiag : tid);
                    s_val[NC * slot] = x == 0 ? p2 : cr;
                    if (CPLX) s_val[2 * slot + 1] = x == 0 ? 0.0 : ci;
                }
            }
            if (tid == 0) s_off[kCorrPP] = run;
            __syncthreads();
            const int np = run; // (every thread summed the same counts)
            // ---- stage B1: project every packet (sector_project, k_cross_t.hpp) ---------------------------------------------------
            if (project) {
                for (int e = tid; e < np; e += kBlock) {
                    if (s_row[e] & kDiag) continue;
                    W rep; double chr, chi, nb;
                    if (!sector_project<W, PM1, FERMI>(bs, elems, s_beta[e], rep, chr, chi, nb)) { s_row[e] = kDead; continue; }
                    s_beta[e] = rep;
                    const double fr = chr * nb, fi = -chi * nb; // chi(g0) = conj(chr, chi), times n(rep)
                    if (PM1) {
                        s_val[NC * e] *= fr;
                        if (CPLX) s_val[2 * e + 1] *= fr;
                    } else {
                        const double hr = s_val[2 * e], hi = s_val[2 * e + 1];
                        s_val[2 * e] = hr * fr - hi * fi;
                        s_val[2 * e + 1] = hr * fi + hi * fr;
                    }
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
                    live[k] = e < np && (s_row[e] & kDiag) == 0; // (kDead has the bit of kDiag set)
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
                    const uint16_t row = s_row[e];
                    if (row != kDead && (row & kDiag)) continue; // |psi_r|^2 is in its slot already
                    double vr = 0.0, vi = 0.0;
                    if (idx[k] >= 0) {
                        if (CPLX) {
                            const double gr = s_val[2 * e], gi = s_val[2 * e + 1];
                            vr = gr * xr[k] - gi * xi[k];
                            vi = gr * xi[k] + gi * xr[k];
                        } else vr = s_val[e] * xr[k];
                    }
                    if (CPLX) { s_val[2 * e] = vr; s_val[2 * e + 1] = vi; } else s_val[e] = vr;
                }
            }
            __syncthreads();
            // ---- the terms of the pass, one wave each: the slots of the term's group in ascending order, under the term's own ------
            // (m, r) and sign mask; one lane adds the sum to the block's partial of the term
            const int g1 = min(g0 + kCorrPP, n_groups);
            for (int q = 0; q < g1 - g0; ++q) {
                const int tb = groups[g0 + q].begin, te = groups[g0 + q].end;
                const int b = s_off[q], e1 = s_off[q + 1];
                for (int t = tb + wave; t < te; t += kCorrWaves) { // (uniform across the wave)
                    lsk_expect_term const T = terms[t];
                    const W tm = (W)T.m, tr = (W)T.r, ts = (W)T.s;
                    double sr = 0.0, si = 0.0;
                    for (int e = b + lane; e < e1; e += 64) {
                        const uint16_t row = s_row[e];
                        if (row == kDead) continue;
                        const W w = s_word[row & 0xff];
                        if ((W)(w & tm) != tr) continue;
                        const bool neg = fermi_popc<W>((W)(w & ts)) & 1;
                        if (CPLX) {
                            sr += neg ? -s_val[2 * e] : s_val[2 * e];
                            si += neg ? -s_val[2 * e + 1] : s_val[2 * e + 1];
                        } else sr += neg ? -s_val[e] : s_val[e];
                    }
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        sr += __shfl_xor(sr, d);
                        if (CPLX) si += __shfl_xor(si, d);
                    }
                    if (lane == 0) {
                        const size_t at = (size_t)(t - term0) * NC;
                        mine[at] = (first ? 0.0 : mine[at]) + sr;
                        if (CPLX) mine[at + 1] = (first ? 0.0 : mine[at + 1]) + si;
                    }
                }
            }
            __syncthreads(); // (and s_word of the next tile after the last pass)
        }
    }
}

// one chunk: the groups [0, n_groups) of `groups`, whose terms are terms[term0, term0 + n_terms) -- out[0, n_terms * NC)
template <bool FERMI>
static int expect_launch(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups, lsk_expect_group const *groups,
                         lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n, uint64_t const *reps,
                         double const *norms, void const *psi, double *partial, double *out, int *d_err, void *stream) {
    if (n <= 0 || n_groups <= 0 || n_terms <= 0) return 0;
    if (!cplx && !bs.chars_pm1) { snprintf(g_err, sizeof(g_err), "%s: f64 needs +-1 characters", __func__); return -1; }
    if (bs.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected basis is looked up by its index", __func__); return -1; }
    if (n_terms > LSK_EXPECT_CHUNK) { snprintf(g_err, sizeof(g_err), "%s: %d terms in a chunk, at most %d", __func__, n_terms, LSK_EXPECT_CHUNK); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int blocks = corr_grid(n);
    dim3 g(blocks), b(kBlock);
#define LSK_EX_ONE(W, PM1, CPLX)                                                                                                         \
    do {                                                                                                                                 \
        g.x = resident_grid(k_expect<W, PM1, CPLX, FERMI>, blocks);                                                                      \
        hipLaunchKernelGGL((k_expect<W, PM1, CPLX, FERMI>), g, b, 0, s, bs, bs.elems, six, gt, cons, n_groups, groups, terms, term0, n,  \
                           reps, norms, (double const *)psi, partial, n_terms, d_err);                                                   \
    } while (0)
    // {32, 64-bit words} x {f64 (+-1 characters) | c128 x {+-1, complex characters}}: 6 kernels per family
#define LSK_EX_LAUNCH(W)                                                                                                                 \
    do {                                                                                                                                 \
        if (!cplx) LSK_EX_ONE(W, true, false);                                                                                           \
        else if (bs.chars_pm1) LSK_EX_ONE(W, true, true);                                                                                \
        else LSK_EX_ONE(W, false, true);                                                                                                 \
    } while (0)
    if (bs.number_sites <= 32) LSK_EX_LAUNCH(uint32_t); else LSK_EX_LAUNCH(uint64_t);
#undef LSK_EX_LAUNCH
#undef LSK_EX_ONE
    LSK_LAUNCH_CHECK();
    return lsk_corr_sum((int)g.x, n_terms * (cplx ? 2 : 1), partial, out, stream);
}
