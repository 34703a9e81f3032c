// k_project_t.hpp -- projection of full-basis vectors into a symmetry sector (ls_amd_project, host.c): the
// adjoint B+ of the sector-state expansion B of k_expand.hip / k_expand_fermi.hip.  With |r~> = P|r> / n(r),
//     psi[r] = <r~|Phi> = (|G| n(r))^-1 sum_{g in G} chi(g) [sign(g, r)] Phi[index(g r)]          (n(r) > 0; otherwise 0)
// where index is the position among the ascending states of the same basis WITHOUT symmetries (the layout unproject writes) and, on a
// spin basis with the global inversion, every permutation element g contributes its image t with chi(g) and t ^ mask with chi(g) inv.
// Pull form: one ROW (representative) per lane, the element loop outside -- the element descriptor (network masks, character) is
// wave-uniform and stays in scalar registers, as in k_expand_push; every lane applies the element, ranks the image, gathers Phi and
// accumulates in registers; ONE plain store per (row, column).  No atomics on the output, no floating-point atomics at all, a fixed
// order of the sum: two calls return the same bytes.  A row is never dealt to several blocks (that would need a reduction).
// Blocks of columns: Phi is (F, K) with arbitrary element strides; a block handles the columns [KT blockIdx.y, KT blockIdx.y + KT)
// with KT accumulators per lane (KT = 1 for one vector, 8 otherwise: 8 complex accumulators and the 8 loads in flight are 64 VGPRs,
// 64 complex accumulators alone would be 256), so the image and its rank are computed once per (row, element) for up to 8 columns.
// Bounds: an image (or a representative) that is not a state of the basis raises *err and is skipped before it is ranked; the rank of
// a state is below F by construction, and is compared with F once more before the load.
// This header holds everything but the __global__ entry points: k_project_pull (k_project.hip; spin bases, with the inversion) and
// k_project_pull_fermi (k_project_fermi.hip; the orbit sign of lsk_fermi.hpp and the product-basis ranking).
#pragma once
#include "lsk_dev.hpp"
#include "lsk_fermi.hpp"

enum { PJ_ALL = LSK_PROJECT_ALL, PJ_FIXED = LSK_PROJECT_FIXED, PJ_PRODUCT = LSK_PROJECT_PRODUCT };
constexpr int kProjectCols = LSK_PROJECT_COLS; // columns per block of the K > 1 kernels

__device__ __forceinline__ uint64_t pj_low_bits(int n) { return n >= 64 ? ~0ULL : ((1ULL << n) - 1); }
__device__ __forceinline__ uint64_t pj_shr(uint64_t s, int n) { return n >= 64 ? 0ULL : (s >> n); }

// is the word a state of the basis?  ALL: no bit above the sites; FIXED: and the weight; PRODUCT: and both halves' particle numbers
template <typename W, int KIND> __device__ __forceinline__ bool pj_is_state(W t, W mask, int weight, lsk_project const &pj) {
    if ((W)(t & (W)~mask) != 0) return false;
    if (KIND == PJ_FIXED) return WordTraits<W>::popc(t) == weight;
    if (KIND == PJ_PRODUCT) {
        const uint64_t s = (uint64_t)t;
        return __popcll(s & pj_low_bits(pj.half)) == pj.n_up && __popcll(pj_shr(s, pj.half)) == pj.n_dn;
    }
    return true;
}
// the position of a STATE among the ascending states of the basis without symmetries: < 2^L, < C(L, w), < C(h, N_up) C(h, N_dn)
template <typename W, int KIND> __device__ __forceinline__ int64_t pj_rank(W t, lsk_project const &pj, uint64_t const *s_binom) {
    if (KIND == PJ_FIXED) return rank_combinadic_w<W, uint64_t>(t, s_binom);
    if (KIND == PJ_PRODUCT) {
        const uint64_t s = (uint64_t)t;
        return rank_combinadic(pj_shr(s, pj.half), s_binom) * pj.n_low + rank_combinadic(s & pj_low_bits(pj.half), s_binom);
    }
    return (int64_t)t;
}

// one image: acc[c] += (cr + i ci) Phi[index(t), c0 + c] for the kc columns of this block.  FULL: kc == KT, no column predicate
template <typename W, bool PM1, bool CPLX, int KIND, int KT, bool FULL>
__device__ __forceinline__ void pj_gather(W t, double cr, double ci, lsk_project const &pj, int weight, W mask, uint64_t const *s_binom,
                                          double const *__restrict__ phi, int c0, int kc, double (&ar)[KT], double (&ai)[KT], int *err) {
    if (!pj_is_state<W, KIND>(t, mask, weight, pj)) { atomicExch(err, 1); return; }
    const int64_t idx = pj_rank<W, KIND>(t, pj, s_binom);
    if ((uint64_t)idx >= (uint64_t)pj.full) { atomicExch(err, 1); return; } // (never: the rank of a state is below F)
    const int64_t base = idx * pj.phi_s0 + (int64_t)c0 * pj.phi_s1;
#pragma unroll
    for (int c = 0; c < KT; ++c) {
        if (!FULL && c >= kc) break;
        const int64_t at = base + (int64_t)c * pj.phi_s1;
        if (CPLX) {
            const double2 v = reinterpret_cast<double2 const *>(phi)[at];
            if (PM1) { ar[c] += cr * v.x; ai[c] += cr * v.y; }
            else { ar[c] += cr * v.x - ci * v.y; ai[c] += cr * v.y + ci * v.x; }
        } else ar[c] += cr * phi[at];
    }
}

template <typename W, bool PM1, bool CPLX, int KIND, bool FERMI, int KT, bool FULL>
__device__ __forceinline__ void pj_rows(lsk_basis const &bs, lsk_group_elem const *__restrict__ elems, lsk_project const &pj,
                                        uint64_t const *s_binom, int64_t n, uint64_t const *__restrict__ reps,
                                        double const *__restrict__ norms, double const *__restrict__ phi, double *__restrict__ out,
                                        int c0, int kc, int *err) {
    const int L = bs.number_sites, weight = bs.hamming_weight, inv = FERMI ? 0 : bs.spin_inversion;
    const W mask = (W)bs.site_mask;
    const bool signs = FERMI && bs.fermi != 0; // a projected fermionic basis: every element carries sign(g, r) (the table is NULL otherwise)
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n; t0 += (int64_t)gridDim.x * kBlock) {
        const int64_t i = t0 + threadIdx.x;
        bool live = i < n;
        W r = 0;
        double scale = 0.0;
        if (live) {
            const uint64_t r64 = reps[i];
            const double nr = norms[i];
            r = (W)r64;
            if ((r64 & ~bs.site_mask) != 0 || !pj_is_state<W, KIND>(r, mask, weight, pj)) { // not a state of this basis
                if (blockIdx.y == 0) atomicExch(err, 1);
                live = false;
            }
            if (!(nr > 0.0)) live = false; // a zero-norm orbit is no basis vector: the row reads 0
            if (live) scale = bs.inv_order / nr;
        }
        double ar[KT], ai[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c) { ar[c] = 0.0; ai[c] = 0.0; }
        for (int g = 0; g < bs.n_elems; ++g) {
            lsk_group_elem const &e = elems[g];
            if (!live) continue;
            const W t = FERMI ? fermi_apply_elem_w<W>(e, r, L, mask) : apply_elem_w<W>(e, r, L, mask);
            double cr = e.ch_re, ci = PM1 ? 0.0 : e.ch_im;
            if (signs && fermi_parity<W>(e, bs.fsign + (size_t)g * L, r, L, false)) { cr = -cr; ci = -ci; }
            pj_gather<W, PM1, CPLX, KIND, KT, FULL>(t, cr, ci, pj, weight, mask, s_binom, phi, c0, kc, ar, ai, err);
            if (inv != 0)
                pj_gather<W, PM1, CPLX, KIND, KT, FULL>((W)(t ^ mask), cr * (double)inv, ci * (double)inv, pj, weight, mask, s_binom, phi,
                                                        c0, kc, ar, ai, err);
        }
        if (i >= n) continue;
        const int64_t base = i * pj.out_s0 + (int64_t)c0 * pj.out_s1;
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            if (!FULL && c >= kc) break;
            const int64_t at = base + (int64_t)c * pj.out_s1;
            if (CPLX) reinterpret_cast<double2 *>(out)[at] = make_double2(scale * ar[c], scale * ai[c]);
            else out[at] = scale * ar[c];
        }
    }
}

// the body of both entry points: the columns of this block, then the rows
template <typename W, bool PM1, bool CPLX, int KIND, bool FERMI, int KT>
__device__ __forceinline__ void pj_block(lsk_basis const &bs, lsk_group_elem const *__restrict__ elems, lsk_project const &pj,
                                         uint64_t const *s_binom, int64_t n, uint64_t const *__restrict__ reps,
                                         double const *__restrict__ norms, double const *__restrict__ phi, double *__restrict__ out, int *err) {
    const int c0 = (int)blockIdx.y * KT;
    const int kc = pj.K - c0 < KT ? pj.K - c0 : KT;
    if (kc <= 0) return;
    if (kc == KT) pj_rows<W, PM1, CPLX, KIND, FERMI, KT, true>(bs, elems, pj, s_binom, n, reps, norms, phi, out, c0, kc, err);
    else pj_rows<W, PM1, CPLX, KIND, FERMI, KT, false>(bs, elems, pj, s_binom, n, reps, norms, phi, out, c0, kc, err);
}

// launch geometry shared by both units: row tiles x column chunks
static inline dim3 pj_grid(int64_t n, int K, int KT) {
    const int64_t tiles = (n + kBlock - 1) / kBlock;
    return dim3((unsigned)(tiles < ((int64_t)1 << 22) ? tiles : ((int64_t)1 << 22)), (unsigned)((K + KT - 1) / KT));
}
static inline int pj_args_ok(char const *who, lsk_basis const &bs, lsk_project const &pj, int cplx) {
    if (pj.K < 1 || pj.K > LSK_PROJECT_MAX_K) { snprintf(g_err, sizeof(g_err), "%s: K = %d columns, outside [1, %d]", who, pj.K, LSK_PROJECT_MAX_K); return 0; }
    if (!cplx && !bs.chars_pm1) { snprintf(g_err, sizeof(g_err), "%s: f64 needs +-1 characters", who); return 0; }
    if (pj.full < 1 || bs.number_sites < 1 || bs.number_sites > 64) { snprintf(g_err, sizeof(g_err), "%s: the layout does not belong to the basis", who); return 0; }
    return 1;
}
