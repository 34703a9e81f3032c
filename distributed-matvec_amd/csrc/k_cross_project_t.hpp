// k_cross_project_t.hpp -- the PROJECTING cross-sector kernel k_cross_project (groups = "project"): any
// operator A between the sectors of two DIFFERENT groups, no covariance assumed.  With Phi = A B1 x on the full basis (never formed),
//     y[r'] = (|G2| n2(r'))^-1 sum_{g in G2} chi2(g) [sign(g, r')] Phi(g r')            (n2(r') > 0; otherwise 0)
// the projection formula of k_project_t.hpp (on a spin target with the global inversion every element also contributes g r' ^ mask with
// chi2(g) inv), and Phi(s) is what stages A, B1, B2 of k_cross_pull (k_cross_t.hpp) evaluate for a target row s with n2 = 1:
//     Phi(s) = sum_j conj(c+_j(s)) chi1(g0j) n1(r) x[idx1(r)],    r = rep1(s ^ x_j),  g0j (s ^ x_j) = r.
// So: the loop over the TARGET's elements is outermost; the element descriptor (network masks, character) is wave-uniform and stays in
// scalar registers, as in pj_rows; every lane applies the element to its row's representative; stage A expands the adjoint's groups on
// that image with the coefficient times w = chi2(g) sign / (|G2| n2); stages B1 and B2 run against the source basis as they do in
// k_cross_pull.  The sum of a row differs from k_cross_pull's: stage B2 leaves coefficient * x of every packet in the packet's LDS
// slot, and after the pass's barrier the row's own lane -- which dealt the slots in stage A and kept them -- adds its packets in
// ascending group order to a REGISTER accumulator that lives across all elements; y is stored once, at the end.  No atomics on y
// and no floating-point atomics at all, a fixed order of the sum: two applies return the same bytes (LDS adds in order of arrival
// would not, with |G2| times as many summands per row as a restricted plan has).  The error flag keeps its meaning: an image with
// non-zero source norm that is not in the source basis.
// The slot allocation of stage A and the core of B1 are the functions of k_cross_t.hpp that k_cross_pull runs on (cross_wave_slot,
// sector_project); the look-up of B2 is restated (see there), and this kernel has no emitting mode.
// PM1: the SOURCE's characters are +-1 (integer stabiliser sums in stage B1); TPM1: the TARGET's are (w is real); REAL: real terms.
// The coefficient of a packet stays real exactly when all three hold (RC), the only form f64 admits.  FERMI: either basis is a
// projected fermionic one -- the target's elements then carry sign(g, r') (where the target has a sign table) and stage B1 projects
// with the signed characters (where the source is projected).
#pragma once
#include "k_cross_t.hpp"

template <typename W, bool PM1, bool CPLX, bool REAL, bool TPM1, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_cross_project(int n_groups, lsk_group const *__restrict__ groups,
                                                          lsk_term const *__restrict__ terms, lsk_basis sbs,
                                                          lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                          lsk_basis dbs, lsk_group_elem const *__restrict__ delems, int64_t n_dst,
                                                          uint64_t const *__restrict__ dst_reps, double const *__restrict__ dst_norms,
                                                          double const *__restrict__ x, double *__restrict__ y, double tiny,
                                                          unsigned long long *count, int *err) {
    constexpr bool RC = REAL && PM1 && TPM1;
    static_assert(CPLX || RC, "f64 needs a real coefficient");
    __shared__ uint64_t s_beta[kCapCross];
    constexpr int CW = CPLX ? 2 : 1; // doubles of a slot: the coefficient (1 when RC), then the product coefficient * x
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
        double acc_r = 0.0, acc_i = 0.0;
        unsigned long long found = 0;
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
                            if (RC) s_coef[CW * slot] = cr * wr;
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
                            if (RC) s_coef[CW * e] = s_coef[CW * e] * chr * nb;
                            else { // times chi1(g0) = conj(chr, chi), times n1(rep)
                                const double hr = s_coef[2 * e], hi = s_coef[2 * e + 1];
                                s_coef[2 * e] = (hr * chr + hi * chi) * nb;
                                s_coef[2 * e + 1] = (hi * chr - hr * chi) * nb;
                            }
                        }
                    }
                    // ---- stage B2: representative -> source index, then the gathers (a thread's loads issued before any is used) --
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
                            else ++found;
                        }
                        if (!count) {
                            double xr[kGCCross], xi[kGCCross];
#pragma unroll
                            for (int k = 0; k < kGCCross; ++k) {
                                xr[k] = 0.0; xi[k] = 0.0;
                                if (idx[k] >= 0) {
                                    if (CPLX) { xr[k] = x[2 * idx[k]]; xi[k] = x[2 * idx[k] + 1]; } else xr[k] = x[idx[k]];
                                }
                            }
                            // every slot of the pass receives its product (0 for a packet that reached no source row): plain stores
#pragma unroll
                            for (int k = 0; k < kGCCross; ++k) {
                                const int e = tid + k * kBlock;
                                if (e >= n) continue;
                                double hr = 0.0, hi = 0.0;
                                if (idx[k] >= 0) { if (RC) hr = s_coef[CW * e]; else { hr = s_coef[2 * e]; hi = s_coef[2 * e + 1]; } }
                                if (CPLX) {
                                    s_coef[2 * e] = hr * xr[k] - hi * xi[k];
                                    s_coef[2 * e + 1] = hr * xi[k] + hi * xr[k];
                                } else s_coef[e] = hr * xr[k];
                            }
                        }
                    }
                    __syncthreads();
                    // the row's own packets, in group order (the next pass writes its slots behind its opening barrier)
                    if (!count) {
#pragma unroll
                        for (int k = 0; k < kGCCross; ++k) {
                            if (mine[k] < 0) continue;
                            acc_r += s_coef[CW * mine[k]];
                            if (CPLX) acc_i += s_coef[2 * mine[k] + 1];
                        }
                    }
                }
            }
        }
        if (count) { if (found) atomicAdd(count, found); }
        else if (valid) {
            if (CPLX) { y[2 * i] = acc_r; y[2 * i + 1] = acc_i; } else y[i] = acc_r;
        }
    }
}

// the launch shared by both units: {32, 64-bit words} x {f64 | c128 x {real coefficient | +-1 source characters, complex coefficient
// | complex source characters}}: 8 kernels.  The last two take complex terms and complex target characters whether or not both occur.
#define LSK_CXP_ARGS n_groups, groups, terms, src, src.elems, six, gt, dst, dst.elems, n_dst, dst_reps, dst_norms, (double const *)x, (double *)y, tiny, d_count, d_err
#define LSK_CXP_ONE(W, PM1, CPLX, REAL, TPM1, FERMI)                                                                                     \
    do {                                                                                                                                 \
        g.x = resident_grid(k_cross_project<W, PM1, CPLX, REAL, TPM1, FERMI>, work_blocks);                                              \
        hipLaunchKernelGGL((k_cross_project<W, PM1, CPLX, REAL, TPM1, FERMI>), g, b, 0, s, LSK_CXP_ARGS);                                \
    } while (0)
#define LSK_CXP_LAUNCH(W, FERMI)                                                                                                         \
    do {                                                                                                                                 \
        if (!cplx) LSK_CXP_ONE(W, true, false, true, true, FERMI);                                                                       \
        else if (real_coef) LSK_CXP_ONE(W, true, true, true, true, FERMI);                                                               \
        else if (src.chars_pm1) LSK_CXP_ONE(W, true, true, false, false, FERMI);                                                         \
        else LSK_CXP_ONE(W, false, true, false, false, FERMI);                                                                           \
    } while (0)

// what both launchers refuse; 1 when the arguments are fine
static inline int cxp_args_ok(char const *who, int is_real, lsk_basis const &src, lsk_gtab const &gt, lsk_basis const &dst, int cplx) {
    if (src.number_sites != dst.number_sites || src.number_sites < 1 || src.number_sites > 64) {
        snprintf(g_err, sizeof(g_err), "%s: the bases have %d and %d bits", who, src.number_sites, dst.number_sites);
        return 0;
    }
    if (!cplx && !(is_real && src.chars_pm1 && dst.chars_pm1)) {
        snprintf(g_err, sizeof(g_err), "%s: f64 needs a real operator and +-1 characters on both bases", who);
        return 0;
    }
    if (src.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected source is looked up by its index", who); return 0; }
    if (dst.n_elems < 1 || !dst.elems) { snprintf(g_err, sizeof(g_err), "%s: the target basis has no group elements (the identity is one)", who); return 0; }
    return 1;
}
