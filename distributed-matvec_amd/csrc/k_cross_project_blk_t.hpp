// k_cross_project_blk_t.hpp -- the block form of the PROJECTING cross-sector kernel (DESIGN.md sections 6b, 6h): Y[:, k] = B2+ A B1 X[:, k]
// for the K columns of an (n_src, K) block, k_cross_project_blk.  k_cross_project_blk.hip instantiates it without permutation signs
// (FERMI = false), k_cross_project_blk_fermi.hip with a projected fermionic basis on either side ("k_cross_project_blk_fermi").
// The formulation is that of k_cross_project (k_cross_project_t.hpp): the loop over the TARGET's elements outermost with a wave-uniform
// element descriptor, the inversion image as the n_img loop, stage A on the image with w = chi2(g) sign / (|G2| n2) folded into the
// coefficient, B1 through sector_project, the look-up of B2 word for word.  None of that depends on x, so a chunk of kCrossKC columns
// shares it -- blockIdx.y is the chunk, as in k_cross_pull_blk (k_cross_blk_t.hpp), whose strides, grid and FULL / tail split this
// kernel takes over.  What changes is where a row's sum is taken: product slots for 8 columns would need kCapCross x 8 x 16 B = 128 KB
// of LDS, so B2 leaves the SOURCE INDEX of every packet in the packet's slot (s_beta; -1: the packet reached no source row) next to
// the coefficient that B1 finished (s_coef), and after the pass's barrier the row's own lane -- which dealt the slots in stage A and
// kept them -- walks its packets in ascending group order, gathers X[idx, c0 .. c0 + 7] (128 B consecutive in c128 on interleaved
// blocks) and adds coef * X to kCrossKC REGISTER accumulators (16 doubles in c128) that live across all elements and images.  They are
// cleared at the head of every tile and stored once at its end, one plain store per (row, column).  No floating-point atomics, in LDS
// or global; the order of a (row, column)'s sum is (element, image, group), whatever the grid: two calls return the same bytes.  LDS
// is that of the single-vector kernel (c128: 8 K states / indices + 16 K coefficients + 1 K flags).  No counting and no emitting mode;
// the error flag keeps its meaning.
#pragma once
#include "k_cross_blk_t.hpp"     // kCrossKC, cross_blk_load, cross_blk_grid
#include "k_cross_project_t.hpp" // cxp_args_ok

// coef * v into the row's register accumulators (FULL: all kCrossKC columns, no column predicate)
template <bool CPLX, bool FULL>
__device__ __forceinline__ void cross_project_blk_add(double (&ar)[kCrossKC], double (&ai)[kCrossKC], int kc, double hr, double hi,
                                                      double const (&vr)[kCrossKC], double const (&vi)[kCrossKC]) {
#pragma unroll
    for (int c = 0; c < kCrossKC; ++c) {
        if (!(FULL || c < kc)) continue;
        if (CPLX) {
            ar[c] += hr * vr[c] - hi * vi[c];
            ai[c] += hr * vi[c] + hi * vr[c];
        } else ar[c] += hr * vr[c];
    }
}

template <typename W, bool PM1, bool CPLX, bool REAL, bool TPM1, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_cross_project_blk(int n_groups, lsk_group const *__restrict__ groups,
                                                              lsk_term const *__restrict__ terms, lsk_basis sbs,
                                                              lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                              lsk_basis dbs, lsk_group_elem const *__restrict__ delems, int64_t n_dst,
                                                              uint64_t const *__restrict__ dst_reps, double const *__restrict__ dst_norms,
                                                              int K, double const *__restrict__ x, int64_t x_row, int64_t x_col,
                                                              double *__restrict__ y, int64_t y_row, int64_t y_col, double tiny, int *err) {
    constexpr bool RC = REAL && PM1 && TPM1;
    static_assert(CPLX || RC, "f64 needs a real coefficient");
    __shared__ uint64_t s_beta[kCapCross]; // the packet's state, then its representative, then (B2) its source index or -1
    constexpr int CW = RC ? 1 : 2;         // doubles of a slot: the coefficient
    __shared__ double s_coef[kCapCross * CW];
    __shared__ uint8_t s_live[kCapCross];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const bool project = sbs.proj != LSK_PROJ_NONE;
    const bool table = gt.entries != nullptr;
    const int L = dbs.number_sites;
    const W mask = (W)dbs.site_mask;
    const int inv = FERMI ? 0 : dbs.spin_inversion;
    const bool dsigns = FERMI && dbs.fermi != 0; // a projected fermionic target: every element carries sign(g, r')
    const int n_img = inv != 0 ? 2 : 1;
    const int c0 = (int)blockIdx.y * kCrossKC;
    const int kc = K - c0 < kCrossKC ? K - c0 : kCrossKC;
    if (kc <= 0) return;
    const bool full = kc == kCrossKC;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n_dst; t0 += (int64_t)gridDim.x * kBlock) {
        const int64_t i = t0 + tid;
        const bool valid = i < n_dst;
        W r = 0;
        double scale = 0.0;
        bool row = false;
        if (valid) {
            const uint64_t r64 = dst_reps[i];
            const double na = dst_norms[i];
            // a zero-norm orbit is no basis vector (the row reads 0); a word outside the sites is no state of the target
            row = na > 0.0 && (r64 & ~dbs.site_mask) == 0;
            r = (W)r64;
            if (row) scale = dbs.inv_order / na;
        }
        double acc_r[kCrossKC], acc_i[kCrossKC]; // the row's sums of this tile: cleared here, stored once at its end
#pragma unroll
        for (int c = 0; c < kCrossKC; ++c) { acc_r[c] = 0.0; acc_i[c] = 0.0; }
        for (int ge = 0; ge < dbs.n_elems; ++ge) {
            lsk_group_elem const &E = delems[ge];
            W img = 0;
            double wr = 0.0, wi = 0.0;
            if (row) {
                img = FERMI ? fermi_apply_elem_w<W>(E, r, L, mask) : apply_elem_w<W>(E, r, L, mask);
                wr = E.ch_re * scale;
                wi = TPM1 ? 0.0 : E.ch_im * scale;
                if (dsigns && fermi_parity<W>(E, dbs.fsign + (size_t)ge * L, r, L, false)) { wr = -wr; wi = -wi; }
            }
            for (int f = 0; f < n_img; ++f) {
                if (f) { img = (W)(img ^ mask); wr *= (double)inv; wi *= (double)inv; }
                const uint64_t a = (uint64_t)img;
                for (int g0 = 0; g0 < n_groups; g0 += kGCCross) {
                    if (tid == 0) s_n = 0;
                    __syncthreads();
                    // ---- stage A: the adjoint's groups on the image -> packets (state, conj(c) w, row) -------------------------
                    int mine[kGCCross]; // the slots of this row's packets, in group order (-1: none)
#pragma unroll
                    for (int k = 0; k < kGCCross; ++k) mine[k] = -1;
#pragma unroll
                    for (int k = 0; k < kGCCross; ++k) {
                        const int g = g0 + k;
                        if (g >= n_groups) break; // (uniform over the block)
                        lsk_group const G = groups[g];
                        double cr = 0.0, ci = 0.0;
                        if (row) term_sum<REAL>(terms, G.begin, G.end, a, cr, ci);
                        const bool act = row && (fabs(cr) > tiny || (!REAL && fabs(ci) > tiny));
                        const int slot = cross_wave_slot(act, lane, &s_n); // < kCapCross: <= kGCCross packets per row
                        if (act) {
                            mine[k] = slot;
                            s_beta[slot] = a ^ G.x;
                            s_live[slot] = 1;
                            if (RC) s_coef[slot] = cr * wr;
                            else { // conj(c) w
                                s_coef[2 * slot] = cr * wr + ci * wi;
                                s_coef[2 * slot + 1] = cr * wi - ci * wr;
                            }
                        }
                    }
                    __syncthreads();
                    const int n = s_n;
                    // ---- stage B1: project every packet into the SOURCE basis (minimum, character, stabiliser norm) -------------
                    if (project) {
                        for (int e = tid; e < n; e += kBlock) {
                            W rep; double chr, chi, nb; // (signed characters where the SOURCE is the fermionic basis)
                            if (!sector_project<W, PM1, FERMI>(sbs, elems, (W)s_beta[e], rep, chr, chi, nb, sbs.fermi != 0)) { s_live[e] = 0; continue; }
                            s_beta[e] = (uint64_t)rep;
                            if (RC) s_coef[e] = s_coef[e] * chr * nb;
                            else { // times chi1(g0) = conj(chr, chi), times n1(rep)
                                const double hr = s_coef[2 * e], hi = s_coef[2 * e + 1];
                                s_coef[2 * e] = (hr * chr + hi * chi) * nb;
                                s_coef[2 * e + 1] = (hi * chr - hr * chi) * nb;
                            }
                        }
                    }
                    // ---- stage B2: representative -> source index, once per packet; the index takes the packet's slot ----------
                    {
                        uint64_t key[kGCCross], bucket[kGCCross];
                        uint32_t tag[kGCCross];
                        ulonglong2 first[kGCCross];
                        int64_t idx[kGCCross];
                        bool live[kGCCross];
#pragma unroll
                        for (int k = 0; k < kGCCross; ++k) {
                            const int e = tid + k * kBlock;
                            live[k] = e < n && s_live[e] != 0;
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
                        // every slot of the pass receives its index (-1 for a packet that reached no source row): plain stores
#pragma unroll
                        for (int k = 0; k < kGCCross; ++k) {
                            const int e = tid + k * kBlock;
                            if (e < n) s_beta[e] = (uint64_t)idx[k];
                        }
                    }
                    __syncthreads();
                    // the row's own packets, in group order: the chunk of X at the packet's source row, times its coefficient (the
                    // next pass writes its slots behind its opening barrier)
#pragma unroll
                    for (int k = 0; k < kGCCross; ++k) {
                        if (mine[k] < 0) continue;
                        const int64_t src = (int64_t)s_beta[mine[k]];
                        if (src < 0) continue;
                        double hr, hi = 0.0;
                        if (RC) hr = s_coef[mine[k]]; else { hr = s_coef[2 * mine[k]]; hi = s_coef[2 * mine[k] + 1]; }
                        double vr[kCrossKC], vi[kCrossKC];
                        const int64_t at = src * x_row + (int64_t)c0 * x_col;
                        if (full) {
                            cross_blk_load<CPLX, true>(x, at, x_col, kc, vr, vi);
                            cross_project_blk_add<CPLX, true>(acc_r, acc_i, kc, hr, hi, vr, vi);
                        } else {
                            cross_blk_load<CPLX, false>(x, at, x_col, kc, vr, vi);
                            cross_project_blk_add<CPLX, false>(acc_r, acc_i, kc, hr, hi, vr, vi);
                        }
                    }
                }
            }
        }
        if (valid) {
            const int64_t at = i * y_row + (int64_t)c0 * y_col;
#pragma unroll
            for (int c = 0; c < kCrossKC; ++c) {
                if (c >= kc) break;
                if (CPLX) reinterpret_cast<double2 *>(y)[at + (int64_t)c * y_col] = make_double2(acc_r[c], acc_i[c]);
                else y[at + (int64_t)c * y_col] = acc_r[c];
            }
        }
    }
}

// the launch shared by both units: the instantiation matrix of LSK_CXP_LAUNCH, {32, 64-bit words} x {f64 | c128 x {real coefficient |
// +-1 source characters, complex coefficient | complex source characters}}: 8 kernels per unit; the grid is cross_blk_grid's
// (LS_AMD_CROSS_BLOCKS caps the row blocks here too)
template <bool FERMI>
static int cross_project_blk_launch(char const *who, int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real,
                                    lsk_basis src, lsk_index six, lsk_gtab gt, lsk_basis dst, int cplx, int64_t n_dst,
                                    uint64_t const *dst_reps, double const *dst_norms, int K, void const *x, int64_t x_row, int64_t x_col,
                                    void *y, int64_t y_row, int64_t y_col, double tiny, int *d_err, void *stream) {
    if (K < 1 || K > 64) { snprintf(g_err, sizeof(g_err), "%s: K = %d columns, outside [1, 64]", who, K); return -1; }
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (!cxp_args_ok(who, is_real, src, gt, dst, cplx)) return -1;
    const bool real_coef = is_real && src.chars_pm1 && dst.chars_pm1;
    const int64_t work_blocks = (n_dst + kBlock - 1) / kBlock;
    const int chunks = (K + kCrossKC - 1) / kCrossKC;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(1, (unsigned)chunks), b(kBlock);
#define LSK_CXPB_ONE(W, PM1, CPLX, REAL, TPM1)                                                                                           \
    do {                                                                                                                                 \
        g.x = (unsigned)cross_blk_grid(k_cross_project_blk<W, PM1, CPLX, REAL, TPM1, FERMI>, work_blocks, chunks);                       \
        hipLaunchKernelGGL((k_cross_project_blk<W, PM1, CPLX, REAL, TPM1, FERMI>), g, b, 0, s, n_groups, groups, terms, src, src.elems,  \
                           six, gt, dst, dst.elems, n_dst, dst_reps, dst_norms, K, (double const *)x, x_row, x_col, (double *)y, y_row,  \
                           y_col, tiny, d_err);                                                                                          \
    } while (0)
#define LSK_CXPB_LAUNCH(W)                                                                                                               \
    do {                                                                                                                                 \
        if (!cplx) LSK_CXPB_ONE(W, true, false, true, true);                                                                             \
        else if (real_coef) LSK_CXPB_ONE(W, true, true, true, true);                                                                     \
        else if (src.chars_pm1) LSK_CXPB_ONE(W, true, true, false, false);                                                               \
        else LSK_CXPB_ONE(W, false, true, false, false);                                                                                 \
    } while (0)
    if (src.number_sites <= 32) LSK_CXPB_LAUNCH(uint32_t); else LSK_CXPB_LAUNCH(uint64_t);
#undef LSK_CXPB_LAUNCH
#undef LSK_CXPB_ONE
    LSK_LAUNCH_CHECK();
    return 0;
}
