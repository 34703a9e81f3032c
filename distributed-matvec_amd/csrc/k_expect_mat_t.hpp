// k_expect_mat_t.hpp -- matrix elements between the columns of two blocks of sector states: k_expect_blk
// (k_expect_blk_t.hpp) with a bra block Phi (n, Ka) and a ket block Psi (n, Kb), each with its own element strides,
//     R[u][a][b] = sum over the rows r with r & m_u == r_u of  (-1)^popcount(r & s_u) conj(Phi[r, a]) / n(r) * <r ^ x_u|Psi[:, b]>
// for every unique device term u = (m, r, x, s), every bra column a and every ket column b.  k_expect_mat.hip instantiates it for
// the bases without permutation signs (FERMI = false), k_expect_mat_fermi.hip for the projected fermionic ones ("k_expect_mat_fermi").
// A block handles kExpMatKA bra columns x kExpKC ket columns; blockIdx.y enumerates the pairs of chunks, the ket chunk fastest.
//   - stages A, B1 and B2 are those of k_expect_blk, word for word: they depend on neither block and run once per (tile, pass,
//     pair of chunks);
//   - the thread that owns a packet's ROW kept Phi[r, a0 .. a0 + kExpMatKA) in registers since the tile's one coalesced read.  Per
//     group it gathers the kExpKC values Psi[idx, b0 ..) of its packet once, then for every bra column in turn (a loop that is
//     uniform across the block) writes the kExpKC products conj(Phi[r, a]) factor Psi[idx, b] to the one-group product planes of
//     k_expect_blk; the per-term waves sum and fold them exactly as there, into the partial of (term, a, b).  The bra value of
//     the turn is picked out of the registers by a chain of selects on the uniform a: no indexed register array, no scratch;
//   - the group x = 0 is neither projected nor looked up: its packet gathers the row's own Psi[r, b0 ..) (a reload, instead of a
//     second register block next to Phi's) with factor 1, and writes conj(Phi[r, a]) Psi[r, b].
// One partial per (block, term, a, b), accumulated from tile to tile and summed over the blocks in block order by lsk_corr_sum.  No
// floating-point atomics, neither global nor in LDS: equal inputs give equal bytes.
#pragma once
#include "k_expect_blk_t.hpp" // kExpKC, kExpBlkPP(Real), expect_blk_fold; through it k_expect_t.hpp, k_corr_t.hpp, k_cross_t.hpp

constexpr int kExpMatKA = 8; // bra columns per block: Phi[r, .] in registers (scratch 0 in every instantiation)

template <typename W, bool PM1, bool CPLX, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_expect_mat(lsk_basis bs, lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                       lsk_expect_cons cons, int n_groups, lsk_expect_group const *__restrict__ groups,
                                                       lsk_expect_term const *__restrict__ terms, int term0, int64_t n,
                                                       uint64_t const *__restrict__ reps, double const *__restrict__ norms, int Ka,
                                                       double const *__restrict__ phi, int64_t a_row, int64_t a_col, int Kb,
                                                       double const *__restrict__ psi, int64_t k_row, int64_t k_col,
                                                       double *__restrict__ partial, int n_partial, int *err) {
    static_assert(kExpKC == 8, "expect_blk_fold puts column c on lane 8 c");
    constexpr int NC = CPLX ? 2 : 1;
    constexpr int PP = CPLX ? kExpBlkPP : kExpBlkPPReal, CAP = kBlock * PP; // groups, and packets, per pass of one tile
    constexpr int NF = PM1 ? 1 : 2;     // doubles of a packet's factor
    constexpr int NP = kExpKC * NC;     // product planes
    constexpr uint16_t kDead = 0xffff;  // zero norm, or not among the representatives: contributes nothing
    constexpr uint16_t kDiag = 0x0200;  // packet of the group x = 0: conj(Phi[r, a]) Psi[r, b], no look-up
    __shared__ W s_beta[CAP];          // A: the image; B1: its representative; B2: the representative's index
    __shared__ double s_fac[CAP * NF]; // A: 1 / n(r) of the packet's row; B1: times chi(g0) n(rep)
    __shared__ uint16_t s_row[CAP];    // row of the tile | kDiag; kDead
    __shared__ W s_word[kBlock];              // the tile's words, for the per-term tests
    __shared__ double s_prod[NP * kBlock];    // the products of ONE group and ONE bra column: plane p of its j-th packet at [p * kBlock + j]
    __shared__ int s_cnt[PP * kCorrWaves];
    __shared__ int s_off[PP + 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const bool project = bs.proj != LSK_PROJ_NONE;
    const bool table = gt.entries != nullptr;
    const int chunks_b = (Kb + kExpKC - 1) / kExpKC;
    const int a0 = (int)(blockIdx.y / (unsigned)chunks_b) * kExpMatKA, b0 = (int)(blockIdx.y % (unsigned)chunks_b) * kExpKC;
    const int ka = Ka - a0 < kExpMatKA ? Ka - a0 : kExpMatKA;
    const int kb = Kb - b0 < kExpKC ? Kb - b0 : kExpKC;
    if (ka <= 0 || kb <= 0) return;
    double *const mine = partial + (size_t)blockIdx.x * n_partial * Ka * Kb * NC;
    const W low = cons.half > 0 ? (W)((((W)1 << (cons.half - 1)) << 1) - 1) : (W)0;
    bool first = true;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n; t0 += (int64_t)gridDim.x * kBlock, first = false) {
        const int64_t i = t0 + tid;
        const bool valid = i < n;
        W a = 0;
        double inv_na = 0.0;
        double own_r[kExpMatKA], own_i[kExpMatKA]; // Phi[r, a0 + c]
#pragma unroll
        for (int c = 0; c < kExpMatKA; ++c) { own_r[c] = 0.0; own_i[c] = 0.0; }
        if (valid) {
            a = (W)reps[i];
            const double na = norms[i];
            inv_na = na > 0.0 ? 1.0 / na : 0.0;
            const int64_t at = i * a_row + (int64_t)a0 * a_col;
#pragma unroll
            for (int c = 0; c < kExpMatKA; ++c) {
                if (c >= ka) continue;
                if (CPLX) { const double2 v = reinterpret_cast<double2 const *>(phi)[at + (int64_t)c * a_col]; own_r[c] = v.x; own_i[c] = v.y; }
                else own_r[c] = phi[at + (int64_t)c * a_col];
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
            // ---- stage B1: project every packet (sector_project, k_cross_t.hpp), once per pair ---------------------------------------
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
            // ---- group by group: the ket values of the group's packets, gathered once by the threads of their rows; then bra column
            // by bra column the products, and the group's terms ----------------------------------------------------------------------
#pragma unroll 1
            for (int q = 0; q < PP; ++q) {
                if (g0 + q >= n_groups) break; // (uniform across the block)
                const int b = s_off[q], e1 = s_off[q + 1];
                int slot = -1;
#pragma unroll
                for (int p = 0; p < PP; ++p) slot = p == q ? my[p] : slot; // (q is uniform: selects, not an indexed array)
                double xr[kExpKC], xi[kExpKC]; // Psi[idx, b0 + c]
                double fr = 0.0, fi = 0.0;
#pragma unroll
                for (int c = 0; c < kExpKC; ++c) { xr[c] = 0.0; xi[c] = 0.0; }
                bool live = false;
                if (slot >= 0) {
                    const uint16_t row = s_row[slot];
                    if (row != kDead) {
                        live = true;
                        const bool diag = (row & kDiag) != 0;
                        // (a packet of x = 0 reads the row's own ket values, with factor n(r) / n(r))
                        const int64_t at = (diag ? i : (int64_t)s_beta[slot]) * k_row + (int64_t)b0 * k_col;
#pragma unroll
                        for (int c = 0; c < kExpKC; ++c) {
                            if (c >= kb) continue;
                            if (CPLX) { const double2 v = reinterpret_cast<double2 const *>(psi)[at + (int64_t)c * k_col]; xr[c] = v.x; xi[c] = v.y; }
                            else xr[c] = psi[at + (int64_t)c * k_col];
                        }
                        fr = diag ? 1.0 : s_fac[NF * slot];
                        fi = PM1 || diag ? 0.0 : s_fac[NF * slot + NF - 1];
                    }
                }
                const int tb = groups[g0 + q].begin, te = groups[g0 + q].end;
#pragma unroll 1
                for (int ca = 0; ca < ka; ++ca) { // (uniform across the block)
                    if (live) {
                        double pr = 0.0, pi = 0.0; // Phi[r, a0 + ca]
#pragma unroll
                        for (int c = 0; c < kExpMatKA; ++c) {
                            pr = c == ca ? own_r[c] : pr;
                            if (CPLX) pi = c == ca ? own_i[c] : pi;
                        }
                        // conj(Phi[r, a]) * factor
                        const double gr = !CPLX || PM1 ? pr * fr : pr * fr + pi * fi;
                        const double gi = !CPLX ? 0.0 : PM1 ? -pi * fr : pr * fi - pi * fr;
                        double *const at = &s_prod[slot - b];
#pragma unroll
                        for (int c = 0; c < kExpKC; ++c) {
                            if (CPLX) {
                                at[(2 * c) * kBlock] = gr * xr[c] - gi * xi[c];
                                at[(2 * c + 1) * kBlock] = gr * xi[c] + gi * xr[c];
                            } else at[c * kBlock] = gr * xr[c];
                        }
                    }
                    __syncthreads();
                    for (int t = tb + wave; t < te; t += kCorrWaves) { // (uniform across the wave)
                        lsk_expect_term const T = terms[t];
                        const W tm = (W)T.m, tr = (W)T.r, ts = (W)T.s;
                        double sum[kExpKC][NC];
#pragma unroll
                        for (int c = 0; c < kExpKC; ++c) {
#pragma unroll
                            for (int k = 0; k < NC; ++k) sum[c][k] = 0.0;
                        }
                        // the block's partial of (term, a, b), read by the lane that will add to it BEFORE the slots are summed: all
                        // blocks' partials together exceed the caches, and the sum and the fold hide the round trip
                        const int col = lane >> 3;
                        const bool writer = (lane & 7) == 0 && col < kb;
                        const size_t mat = (((size_t)(t - term0) * Ka + (size_t)(a0 + ca)) * Kb + (size_t)(b0 + col)) * NC;
                        double prev[NC];
#pragma unroll
                        for (int k = 0; k < NC; ++k) prev[k] = writer && !first ? mine[mat + k] : 0.0;
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
                        if (writer) {
#pragma unroll
                            for (int k = 0; k < NC; ++k) mine[mat + k] = prev[k] + sum[0][k];
                        }
                    }
                    __syncthreads(); // (s_prod of the next bra column and group; the packets of the next pass; s_word of the next tile)
                }
            }
        }
    }
}

// one chunk of terms: the groups [0, n_groups) of `groups`, whose terms are terms[term0, term0 + n_terms) --
// out[((u Ka + a) Kb + b) NC ...), term-major.  `partial` holds corr_grid(n) * n_terms * Ka * Kb values.
template <bool FERMI>
static int expect_mat_launch(char const *who, lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups,
                             lsk_expect_group const *groups, lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n,
                             uint64_t const *reps, double const *norms, int Ka, void const *phi, int64_t a_row, int64_t a_col, int Kb,
                             void const *psi, int64_t k_row, int64_t k_col, double *partial, double *out, int *d_err, void *stream) {
    if (Ka < 1 || Ka > 64 || Kb < 1 || Kb > 64) {
        snprintf(g_err, sizeof(g_err), "%s: Ka = %d bra and Kb = %d ket columns, outside [1, 64]", who, Ka, Kb);
        return -1;
    }
    if (n <= 0 || n_groups <= 0 || n_terms <= 0) return 0;
    if (!cplx && !bs.chars_pm1) { snprintf(g_err, sizeof(g_err), "%s: f64 needs +-1 characters", who); return -1; }
    if (bs.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected basis is looked up by its index", who); return -1; }
    if (n >= 0xffffffffLL) { snprintf(g_err, sizeof(g_err), "%s: %lld rows, at most 2^32 - 2", who, (long long)n); return -1; }
    if ((int64_t)n_terms * Ka * Kb > (int64_t)LSK_EXPECT_CHUNK * kExpKC) {
        snprintf(g_err, sizeof(g_err), "%s: %d terms x %d x %d columns in a launch, at most %d values", who, n_terms, Ka, Kb,
                 LSK_EXPECT_CHUNK * kExpKC);
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    const int blocks = corr_grid(n);
    const int chunks = ((Ka + kExpMatKA - 1) / kExpMatKA) * ((Kb + kExpKC - 1) / kExpKC);
    dim3 g(1, (unsigned)chunks), b(kBlock);
    // (no more blocks than are resident at once, shared among the pairs of chunks)
#define LSK_EXM_ONE(W, PM1, CPLX)                                                                                                        \
    do {                                                                                                                                 \
        int rows = resident_grid(k_expect_mat<W, PM1, CPLX, FERMI>, (int64_t)blocks * chunks) / chunks;                                  \
        rows = rows > blocks ? blocks : rows;                                                                                            \
        g.x = (unsigned)(rows < 1 ? 1 : rows);                                                                                           \
        hipLaunchKernelGGL((k_expect_mat<W, PM1, CPLX, FERMI>), g, b, 0, s, bs, bs.elems, six, gt, cons, n_groups, groups, terms, term0, \
                           n, reps, norms, Ka, (double const *)phi, a_row, a_col, Kb, (double const *)psi, k_row, k_col, partial,        \
                           n_terms, d_err);                                                                                              \
    } while (0)
    // {32, 64-bit words} x {f64 (+-1 characters) | c128 x {+-1, complex characters}}: 6 kernels per family
#define LSK_EXM_LAUNCH(W)                                                                                                                \
    do {                                                                                                                                 \
        if (!cplx) LSK_EXM_ONE(W, true, false);                                                                                          \
        else if (bs.chars_pm1) LSK_EXM_ONE(W, true, true);                                                                               \
        else LSK_EXM_ONE(W, false, true);                                                                                                \
    } while (0)
    if (bs.number_sites <= 32) LSK_EXM_LAUNCH(uint32_t); else LSK_EXM_LAUNCH(uint64_t);
#undef LSK_EXM_LAUNCH
#undef LSK_EXM_ONE
    LSK_LAUNCH_CHECK();
    return lsk_corr_sum((int)g.x, n_terms * Ka * Kb * (cplx ? 2 : 1), partial, out, stream);
}
