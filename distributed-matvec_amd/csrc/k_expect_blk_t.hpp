// k_expect_blk_t.hpp -- the block form of the expectation-value kernel: k_expect (k_expect_t.hpp) for the K
// columns of an (n, K) block Psi with element strides (row, column),
//     R[u][c] = sum over the rows r with r & m_u == r_u of  (-1)^popcount(r & s_u) conj(Psi[r, c]) / n(r) * <r ^ x_u|Psi[:, c]>
// for every unique device term u = (m, r, x, s) and every column c.  k_expect_blk.hip instantiates it for the bases without
// permutation signs (FERMI = false), k_expect_blk_fermi.hip for the projected fermionic ones (FERMI = true; "k_expect_blk_fermi").
// A block handles the columns [kExpKC blockIdx.y, kExpKC blockIdx.y + kExpKC), as k_cross_pull_blk does.  Everything that does not
// depend on the state runs once per chunk of columns, on the tiles and in the stages of k_expect:
//   - stage A (the packets of every flip-mask group of the pass, compacted in (group, wave, lane) order), stage B1 (the projection
//     of every image) and the look-up of stage B2 work on 4 (c128) or 8 (f64) groups at a time with every lane busy; a packet's slot carries
//     the column-independent factor chi(g0) n(rep) / n(r) and, after B2, the INDEX of its representative in place of the image;
//   - the products are then formed group by group, by the thread that owns the packet's ROW: it kept Psi[r, c0 .. c0 + kExpKC) in
//     registers since the tile's one coalesced read, issues the kExpKC gathers of Psi[idx, c0 ..) -- with interleaved columns 64 B
//     (f64) or 128 B (c128) of consecutive memory -- before it uses any, and writes conj(Psi[r, c]) factor Psi[idx, c] to the
//     group's product planes in LDS (plane p of the group's j-th packet at s_prod[p * kBlock + j]: a wave writes and reads
//     consecutive doubles of a plane).  One group's products are 16 KB (f64) or 32 KB (c128), whatever the pass holds;
//   - one wave per term sums the group's slots in ascending order under the term's own (m, r) and sign mask: the test and the sign
//     are evaluated once per (slot, term) and applied to the 8 (16) planes; the lanes' sums are then folded by a transposing
//     butterfly (three exchange steps halve the columns a lane holds, three more finish the one that is left: 10 shuffles per
//     plane set instead of 48), after which lane 8 c holds column c.  One partial per (block, term, column), accumulated from tile
//     to tile and summed over the blocks in block order by lsk_corr_sum.  No floating-point atomics, neither global nor in LDS:
//     equal inputs give equal bytes.
// The group x = 0 is neither projected nor looked up: its product is |Psi[r, c]|^2.
#pragma once
#include "k_expect_t.hpp" // through it k_corr_t.hpp (kCorrWaves, corr_grid) and k_cross_t.hpp (sector_project, cross_index)

constexpr int kExpKC = 8;                        // columns per block: products per packet, and loads in flight per packet
constexpr int kExpBlkPP = 4;                     // flip-mask groups per pass of the c128 kinds (60 KB of static LDS; 8 do not fit in 64 KB)
constexpr int kExpBlkPPReal = 8;                 // and of the f64 kinds (53 KB; measured 5-9 % faster than 4)

// v[c][.] of every lane, kExpKC columns -> the sum over the 64 lanes of column (lane >> 3) in v[0][.] (of every lane)
template <int NC>
__device__ __forceinline__ void expect_blk_fold(double (&v)[kExpKC][NC], int lane) {
#pragma unroll
    for (int half = kExpKC / 2, d = 32; half >= 1; half >>= 1, d >>= 1) {
        const bool hi = (lane & d) != 0;
#pragma unroll
        for (int c = 0; c < half; ++c) {
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const double keep = hi ? v[c + half][k] : v[c][k], send = hi ? v[c][k] : v[c + half][k];
                v[c][k] = keep + __shfl_xor(send, d);
            }
        }
    }
#pragma unroll
    for (int d = 4; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < NC; ++k) v[0][k] += __shfl_xor(v[0][k], d);
    }
}

template <typename W, bool PM1, bool CPLX, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_expect_blk(lsk_basis bs, lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                       lsk_expect_cons cons, int n_groups, lsk_expect_group const *__restrict__ groups,
                                                       lsk_expect_term const *__restrict__ terms, int term0, int64_t n,
                                                       uint64_t const *__restrict__ reps, double const *__restrict__ norms, int K,
                                                       double const *__restrict__ psi, int64_t p_row, int64_t p_col,
                                                       double *__restrict__ partial, int n_partial, int *err) {
    static_assert(kExpKC == 8, "expect_blk_fold puts column c on lane 8 c");
    constexpr int NC = CPLX ? 2 : 1;
    constexpr int PP = CPLX ? kExpBlkPP : kExpBlkPPReal, CAP = kBlock * PP; // groups, and packets, per pass of one tile
    constexpr int NF = PM1 ? 1 : 2;     // doubles of a packet's factor
    constexpr int NP = kExpKC * NC;     // product planes
    constexpr uint16_t kDead = 0xffff;  // zero norm, or not among the representatives: contributes nothing
    constexpr uint16_t kDiag = 0x0200;  // packet of the group x = 0: |Psi[r, c]|^2, no look-up
    __shared__ W s_beta[CAP];          // A: the image; B1: its representative; B2: the representative's index
    __shared__ double s_fac[CAP * NF]; // A: 1 / n(r) of the packet's row; B1: times chi(g0) n(rep)
    __shared__ uint16_t s_row[CAP];    // row of the tile | kDiag; kDead
    __shared__ W s_word[kBlock];              // the tile's words, for the per-term tests
    __shared__ double s_prod[NP * kBlock];    // the products of ONE group: plane p of its j-th packet at [p * kBlock + j]
    __shared__ int s_cnt[PP * kCorrWaves];
    __shared__ int s_off[PP + 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const bool project = bs.proj != LSK_PROJ_NONE;
    const bool table = gt.entries != nullptr;
    const int c0 = (int)blockIdx.y * kExpKC;
    const int kc = K - c0 < kExpKC ? K - c0 : kExpKC;
    if (kc <= 0) return;
    double *const mine = partial + (size_t)blockIdx.x * n_partial * K * NC;
    const W low = cons.half > 0 ? (W)((((W)1 << (cons.half - 1)) << 1) - 1) : (W)0;
    bool first = true;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n; t0 += (int64_t)gridDim.x * kBlock, first = false) {
        const int64_t i = t0 + tid;
        const bool valid = i < n;
        W a = 0;
        double inv_na = 0.0;
        double own_r[kExpKC], own_i[kExpKC]; // Psi[r, c0 + c]
#pragma unroll
        for (int c = 0; c < kExpKC; ++c) { own_r[c] = 0.0; own_i[c] = 0.0; }
        if (valid) {
            a = (W)reps[i];
            const double na = norms[i];
            inv_na = na > 0.0 ? 1.0 / na : 0.0;
            const int64_t at = i * p_row + (int64_t)c0 * p_col;
#pragma unroll
            for (int c = 0; c < kExpKC; ++c) {
                if (c >= kc) continue;
                if (CPLX) { const double2 v = reinterpret_cast<double2 const *>(psi)[at + (int64_t)c * p_col]; own_r[c] = v.x; own_i[c] = v.y; }
                else own_r[c] = psi[at + (int64_t)c * p_col];
            }
        }
        s_word[tid] = a;
        for (int g0 = 0; g0 < n_groups; g0 += PP) {
            // ---- stage A: the rows that emit a packet for every group of the pass, counted per (group, wave) ... -----------------
            uint32_t act = 0;
#pragma unroll
            for (int q = 0; q < PP; ++q) {
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
            // ---- ... and written at the prefix sums of the counts: packets (image, row, 1 / n(r)) in (group, wave, lane) order; a
            // row remembers the slot of its packet in every group of the pass ---------------------------------------------------
            int my[PP];
            int run = 0;
#pragma unroll
            for (int q = 0; q < PP; ++q) {
                if (tid == 0) s_off[q] = run;
                int base = 0;
#pragma unroll
                for (int w = 0; w < kCorrWaves; ++w) {
                    if (w == wave) base = run;
                    run += s_cnt[q * kCorrWaves + w];
                }
                const bool on = (act >> q) & 1;
                const unsigned long long ball = __ballot(on);
                my[q] = -1;
                if (on) {
                    const W x = (W)groups[g0 + q].x;
                    const int slot = base + __popcll(ball & ((1ULL << lane) - 1));
                    my[q] = slot;
                    s_beta[slot] = (W)(a ^ x);
                    s_row[slot] = (uint16_t)(x == 0 ? tid | kDiag : tid);
                    s_fac[NF * slot] = inv_na;
                    if (!PM1) s_fac[2 * slot + 1] = 0.0;
                }
            }
            if (tid == 0) s_off[PP] = run;
            __syncthreads();
            const int np = run; // (every thread summed the same counts)
            // ---- stage B1: project every packet (sector_project, k_cross_t.hpp), once per chunk --------------------------------------
            if (project) {
                for (int e = tid; e < np; e += kBlock) {
                    if (s_row[e] & kDiag) continue;
                    W rep; double chr, chi, nb;
                    if (!sector_project<W, PM1, FERMI>(bs, elems, s_beta[e], rep, chr, chi, nb)) { s_row[e] = kDead; continue; }
                    s_beta[e] = rep;
                    if (PM1) s_fac[e] *= chr * nb;
                    else { // chi(g0) = conj(chr, chi), times n(rep) / n(r)
                        const double h = s_fac[2 * e];
                        s_fac[2 * e] = h * (chr * nb);
                        s_fac[2 * e + 1] = h * (-chi * nb);
                    }
                }
            }
            // ---- stage B2, the shared part: representative -> index, four look-ups in flight; the index takes the image's place --
            // (slot e is read and written by thread e % kBlock alone, in B1 and here)
            for (int e0 = 0; e0 < np; e0 += 4 * kBlock) {
                uint64_t key[4], bucket[4];
                uint32_t tag[4];
                ulonglong2 head[4];
                bool live[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = e0 + tid + k * kBlock;
                    live[k] = e < np && (s_row[e] & kDiag) == 0; // (kDead has the bit of kDiag set)
                    key[k] = live[k] ? (uint64_t)s_beta[e] : 0;
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
                    const int e = e0 + tid + k * kBlock;
                    int64_t idx;
                    if (table) {
                        const uint32_t pay = gt_resolve(gt, gt.entries, bucket[k], tag[k], head[k]);
                        idx = pay == 0xffffffffu ? -1 : (int64_t)pay;
                    } else idx = cross_index(six, key[k]);
                    if (idx < 0 || idx >= n) { s_row[e] = kDead; atomicExch(err, 1); } // an image that is not among the representatives
                    else s_beta[e] = (W)idx; // (n < 2^32 - 1)
                }
            }
            __syncthreads();
            // ---- group by group: the products of the group's packets, by the threads of their rows; then the group's terms ---------
#pragma unroll
            for (int q = 0; q < PP; ++q) {
                if (g0 + q >= n_groups) break; // (uniform across the block)
                const int b = s_off[q], e1 = s_off[q + 1];
                if (my[q] >= 0) {
                    const int e = my[q];
                    const uint16_t row = s_row[e];
                    if (row != kDead) {
                        double vr[kExpKC], vi[kExpKC];
                        if (row & kDiag) {
#pragma unroll
                            for (int c = 0; c < kExpKC; ++c) { vr[c] = own_r[c] * own_r[c] + own_i[c] * own_i[c]; vi[c] = 0.0; }
                        } else {
                            const int64_t at = (int64_t)s_beta[e] * p_row + (int64_t)c0 * p_col;
                            double xr[kExpKC], xi[kExpKC];
#pragma unroll
                            for (int c = 0; c < kExpKC; ++c) {
                                xr[c] = 0.0; xi[c] = 0.0;
                                if (c >= kc) continue;
                                if (CPLX) { const double2 v = reinterpret_cast<double2 const *>(psi)[at + (int64_t)c * p_col]; xr[c] = v.x; xi[c] = v.y; }
                                else xr[c] = psi[at + (int64_t)c * p_col];
                            }
                            const double fr = s_fac[NF * e], fi = PM1 ? 0.0 : s_fac[NF * e + NF - 1];
#pragma unroll
                            for (int c = 0; c < kExpKC; ++c) {
                                if (CPLX) { // conj(Psi[r, c]) * factor * Psi[idx, c]
                                    const double gr = PM1 ? own_r[c] * fr : own_r[c] * fr + own_i[c] * fi;
                                    const double gi = PM1 ? -own_i[c] * fr : own_r[c] * fi - own_i[c] * fr;
                                    vr[c] = gr * xr[c] - gi * xi[c];
                                    vi[c] = gr * xi[c] + gi * xr[c];
                                } else { vr[c] = own_r[c] * fr * xr[c]; vi[c] = 0.0; }
                            }
                        }
                        double *const at = &s_prod[e - b];
#pragma unroll
                        for (int c = 0; c < kExpKC; ++c) {
                            at[(NC * c) * kBlock] = vr[c];
                            if (CPLX) at[(2 * c + 1) * kBlock] = vi[c];
                        }
                    }
                }
                __syncthreads();
                const int tb = groups[g0 + q].begin, te = groups[g0 + q].end;
                for (int t = tb + wave; t < te; t += kCorrWaves) { // (uniform across the wave)
                    lsk_expect_term const T = terms[t];
                    const W tm = (W)T.m, tr = (W)T.r, ts = (W)T.s;
                    double sum[kExpKC][NC];
#pragma unroll
                    for (int c = 0; c < kExpKC; ++c) {
#pragma unroll
                        for (int k = 0; k < NC; ++k) sum[c][k] = 0.0;
                    }
                    for (int e = b + lane; e < e1; e += 64) {
                        const uint16_t row = s_row[e];
                        if (row == kDead) continue;
                        const W w = s_word[row & 0xff];
                        if ((W)(w & tm) != tr) continue;
                        const bool neg = fermi_popc<W>((W)(w & ts)) & 1;
                        double const *const at = &s_prod[e - b];
#pragma unroll
                        for (int c = 0; c < kExpKC; ++c) {
#pragma unroll
                            for (int k = 0; k < NC; ++k) {
                                const double v = at[(NC * c + k) * kBlock];
                                sum[c][k] += neg ? -v : v;
                            }
                        }
                    }
                    expect_blk_fold<NC>(sum, lane);
                    const int col = lane >> 3;
                    if ((lane & 7) == 0 && col < kc) {
                        const size_t at = ((size_t)(t - term0) * K + (size_t)(c0 + col)) * NC;
#pragma unroll
                        for (int k = 0; k < NC; ++k) mine[at + k] = (first ? 0.0 : mine[at + k]) + sum[0][k];
                    }
                }
                __syncthreads(); // (s_prod of the next group; the packets of the next pass; s_word of the next tile)
            }
        }
    }
}

// one chunk of terms: the groups [0, n_groups) of `groups`, whose terms are terms[term0, term0 + n_terms) -- out[(u K + c) NC ...),
// term-major.  `partial` holds corr_grid(n) * n_terms * K values.
template <bool FERMI>
static int expect_blk_launch(char const *who, lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups,
                             lsk_expect_group const *groups, lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n,
                             uint64_t const *reps, double const *norms, int K, void const *psi, int64_t p_row, int64_t p_col,
                             double *partial, double *out, int *d_err, void *stream) {
    if (K < 1 || K > 64) { snprintf(g_err, sizeof(g_err), "%s: K = %d columns, outside [1, 64]", who, K); return -1; }
    if (n <= 0 || n_groups <= 0 || n_terms <= 0) return 0;
    if (!cplx && !bs.chars_pm1) { snprintf(g_err, sizeof(g_err), "%s: f64 needs +-1 characters", who); return -1; }
    if (bs.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected basis is looked up by its index", who); return -1; }
    if (n >= 0xffffffffLL) { snprintf(g_err, sizeof(g_err), "%s: %lld rows, at most 2^32 - 2", who, (long long)n); return -1; }
    if ((int64_t)n_terms * K > (int64_t)LSK_EXPECT_CHUNK * kExpKC) {
        snprintf(g_err, sizeof(g_err), "%s: %d terms x %d columns in a launch, at most %d values", who, n_terms, K, LSK_EXPECT_CHUNK * kExpKC);
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    const int blocks = corr_grid(n);
    const int chunks = (K + kExpKC - 1) / kExpKC;
    dim3 g(1, (unsigned)chunks), b(kBlock);
    // (no more blocks than are resident at once, shared among the column chunks)
#define LSK_EXB_ONE(W, PM1, CPLX)                                                                                                        \
    do {                                                                                                                                 \
        int rows = resident_grid(k_expect_blk<W, PM1, CPLX, FERMI>, (int64_t)blocks * chunks) / chunks;                                  \
        rows = rows > blocks ? blocks : rows;                                                                                            \
        g.x = (unsigned)(rows < 1 ? 1 : rows);                                                                                           \
        hipLaunchKernelGGL((k_expect_blk<W, PM1, CPLX, FERMI>), g, b, 0, s, bs, bs.elems, six, gt, cons, n_groups, groups, terms, term0, \
                           n, reps, norms, K, (double const *)psi, p_row, p_col, partial, n_terms, d_err);                               \
    } while (0)
    // {32, 64-bit words} x {f64 (+-1 characters) | c128 x {+-1, complex characters}}: 6 kernels per family
#define LSK_EXB_LAUNCH(W)                                                                                                                \
    do {                                                                                                                                 \
        if (!cplx) LSK_EXB_ONE(W, true, false);                                                                                          \
        else if (bs.chars_pm1) LSK_EXB_ONE(W, true, true);                                                                               \
        else LSK_EXB_ONE(W, false, true);                                                                                                \
    } while (0)
    if (bs.number_sites <= 32) LSK_EXB_LAUNCH(uint32_t); else LSK_EXB_LAUNCH(uint64_t);
#undef LSK_EXB_LAUNCH
#undef LSK_EXB_ONE
    LSK_LAUNCH_CHECK();
    return lsk_corr_sum((int)g.x, n_terms * K * (cplx ? 2 : 1), partial, out, stream);
}
