// k_expand_fermi.hip -- sector-state expansion of fermionic bases (ls_amd_fermi_expand_create, host.c): the push
// scatter of k_expand.hip with the two signs of fermions.  The image s = g r of representative r under group element g receives
//     <a, b|psi> = sigma(s) conj(chi(g)) sign(g, r) n(r) psi[r]
//   sign(g, r): U_g |r> = sign(g, r) |g r> (fermi_parity, lsk_fermi.hpp; a basis without a group has the identity alone and no table);
//   sigma(s):   |s> = sigma(s) |a>_A |b>_B, the modes of A carried in front of those of B (fermi_split_parity, lsk_fermi.hpp).
// Several g reach the same s when r has a stabiliser; they store the same value (n(r) > 0 forces chi(g) sign(g, r) = 1 on the
// stabiliser, and U is a representation), so plain stores are enough.  No spin inversion: fermionic bases have none.
// Lane mapping of k_expand_push: one ROW per lane, the element loop outside, the element descriptor wave-uniform; blockIdx.y deals
// the elements to several blocks when there are few row tiles.
// Block layouts (KIND): ALL -- no fixed particle number, one 2^|A| x 2^|B| block; FIXED -- one block per n_A, as the spin kernel;
// PRODUCT -- the spinful (N_up, N_down) basis, one block per (n_A_up, n_A_down): with a = a_dn << |A_up| | a_up (the up modes of A
// are its low modes) and b alike, row = rank(a_dn) C(|A_up|, n_up) + rank(a_up), column = rank(b_dn) C(L - |A_up|, N_up - n_up) +
// rank(b_up): ascending integer order of a and b, and for A = every mode the order of lsk_enumerate_product.
#include "lsk_dev.hpp"
#include "lsk_fermi.hpp"

extern "C" char const *lsk_expand_fermi_kernel_name(void) { return "k_expand_push_fermi"; }
// host run of the bipartition sign (ls_amd_test_fermi_split_parity): the code the kernel runs, on 64-bit words
extern "C" int lsk_test_fermi_split_parity(uint64_t n, uint64_t mask_a, uint64_t mask_b) {
    return fermi_split_parity<uint64_t>(n, mask_a, mask_b);
}

enum { KIND_ALL = LSK_EXPAND_FERMI_ALL, KIND_FIXED = LSK_EXPAND_FERMI_FIXED, KIND_PRODUCT = LSK_EXPAND_FERMI_PRODUCT };

__device__ __forceinline__ uint64_t fx_low_bits(int n) { return n >= 64 ? ~0ULL : ((1ULL << n) - 1); }
__device__ __forceinline__ uint64_t fx_shr(uint64_t s, int n) { return n >= 64 ? 0ULL : (s >> n); }
// the bits of s on the modes of m, compacted in ascending mode order (m is wave-uniform: so is the trip count)
__device__ __forceinline__ uint64_t fx_gather_bits(uint64_t s, uint64_t m) {
    uint64_t out = 0;
    int k = 0;
    while (m) {
        const int p = __ffsll((unsigned long long)m) - 1;
        out |= ((s >> p) & 1ULL) << k;
        ++k;
        m &= m - 1;
    }
    return out;
}

// is the word a state of the basis?  ALL: no bit above the modes; FIXED: and the particle number; PRODUCT: and both halves' numbers
template <typename W, int KIND> __device__ __forceinline__ bool fx_is_state(W t, W mask, int weight, lsk_expand_fermi const &ex) {
    if ((W)(t & (W)~mask) != 0) return false;
    if (KIND == KIND_FIXED) return WordTraits<W>::popc(t) == weight;
    if (KIND == KIND_PRODUCT) {
        const uint64_t s = (uint64_t)t;
        return __popcll(s & fx_low_bits(ex.half)) == ex.n_up && __popcll(fx_shr(s, ex.half)) == ex.n_dn;
    }
    return true;
}

// one image: sign of the split, split by the subsystem, rank both sides, store.  An image that is not a state of the basis raises
// *err and is dropped; every index below is then inside its block (ranks of sub-words of a state with the block's particle numbers;
// a < 2^n_a, b < 2^n_b without a fixed number)
template <typename W, bool CPLX, int KIND>
__device__ __forceinline__ void expand_store_fermi(W t, double wr, double wi, lsk_expand_fermi const &ex, int weight, W mask,
                                                   uint64_t const *s_binom, int64_t const *s_tab, double *__restrict__ out, int *err) {
    if (!fx_is_state<W, KIND>(t, mask, weight, ex)) { atomicExch(err, 1); return; }
    const uint64_t s = (uint64_t)t;
    uint64_t a, b;
    if (ex.split == LSK_SPLIT_LOW) { a = s & fx_low_bits(ex.n_a); b = fx_shr(s, ex.n_a); }
    else if (ex.split == LSK_SPLIT_HIGH) { b = s & fx_low_bits(ex.n_b); a = fx_shr(s, ex.n_b); }
    else { a = fx_gather_bits(s, ex.mask_a); b = fx_gather_bits(s, ex.mask_b); }
    int64_t idx;
    if (KIND == KIND_FIXED) {
        const int na = __popcll(a);
        if (na < ex.lo || na > ex.hi) return; // a block that was not asked for
        const int64_t off = s_tab[na];
        if (off < 0) { atomicExch(err, 1); return; }
        idx = off + rank_combinadic(a, s_binom) * s_tab[LSK_EXPAND_MAX_NA + na] + rank_combinadic(b, s_binom);
    } else if (KIND == KIND_PRODUCT) {
        const int bu = ex.half - ex.au, bd = ex.half - ex.ad; // modes of B per species
        const uint64_t a_up = a & fx_low_bits(ex.au), a_dn = fx_shr(a, ex.au), b_up = b & fx_low_bits(bu), b_dn = fx_shr(b, bu);
        const int nu = __popcll(a_up), nd = __popcll(a_dn); // <= N_up, N_down: t is a state
        const int key = nu * (ex.ad + 1) + nd;
        if (key < ex.lo || key > ex.hi) return;
        const int64_t off = s_tab[key];
        if (off < 0) { atomicExch(err, 1); return; }
        const int64_t ru = (int64_t)s_binom[ex.au * LSK_BINOM_K + nu];
        const int64_t cu = (int64_t)s_binom[bu * LSK_BINOM_K + (ex.n_up - nu)], cd = (int64_t)s_binom[bd * LSK_BINOM_K + (ex.n_dn - nd)];
        const int64_t row = rank_combinadic(a_dn, s_binom) * ru + rank_combinadic(a_up, s_binom);
        const int64_t col = rank_combinadic(b_dn, s_binom) * cu + rank_combinadic(b_up, s_binom);
        idx = off + row * (cu * cd) + col;
    } else idx = (int64_t)a * ex.cols + (int64_t)b;
    if (fermi_split_parity<W>(t, (W)ex.mask_a, (W)ex.mask_b)) { wr = -wr; wi = -wi; }
    if (CPLX) reinterpret_cast<double2 *>(out)[idx] = make_double2(wr, wi);
    else out[idx] = wr;
}

template <typename W, bool PM1, bool CPLX, int KIND>
__global__ __launch_bounds__(kBlock) void k_expand_push_fermi(lsk_basis bs, lsk_group_elem const *__restrict__ elems, lsk_expand_fermi ex,
                                                              uint64_t const *__restrict__ g_binom, int64_t n,
                                                              uint64_t const *__restrict__ reps, double const *__restrict__ norms,
                                                              double const *__restrict__ psi, double *__restrict__ out, int *err) {
    __shared__ uint64_t s_binom[KIND != KIND_ALL ? 64 * LSK_BINOM_K : 1];
    __shared__ int64_t s_tab[KIND == KIND_PRODUCT ? LSK_EXPAND_FERMI_TAB : (KIND == KIND_FIXED ? 2 * LSK_EXPAND_MAX_NA : 1)];
    if (KIND != KIND_ALL) {
        const int n_tab = KIND == KIND_PRODUCT ? (ex.au + 1) * (ex.ad + 1) : 2 * LSK_EXPAND_MAX_NA; // PRODUCT: <= 33 x 33
        for (int i = threadIdx.x; i < n_tab; i += blockDim.x) s_tab[i] = ex.tab[i];
        load_binom(s_binom, g_binom); // (synchronises the block)
    }
    const int L = bs.number_sites, weight = bs.hamming_weight;
    const W mask = (W)bs.site_mask;
    const bool signs = bs.fermi != 0; // a projected basis: every element carries sign(g, r) (the table is NULL otherwise)
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n; t0 += (int64_t)gridDim.x * kBlock) {
        const int64_t i = t0 + threadIdx.x;
        bool valid = i < n;
        W r = 0;
        double vr = 0.0, vi = 0.0;
        if (valid) {
            const uint64_t r64 = reps[i];
            const double nr = norms[i];
            r = (W)r64;
            if ((r64 & ~bs.site_mask) != 0 || !fx_is_state<W, KIND>(r, mask, weight, ex)) { // not a state of this basis
                if (blockIdx.y == 0) atomicExch(err, 1);
                valid = false;
            }
            if (!(nr > 0.0)) valid = false; // a zero-norm orbit is no basis vector: nothing to scatter
            if (CPLX) { vr = nr * psi[2 * i]; vi = nr * psi[2 * i + 1]; } else vr = nr * psi[i];
        }
        for (int g = blockIdx.y; g < bs.n_elems; g += gridDim.y) {
            lsk_group_elem const &e = elems[g];
            if (!valid) continue;
            const W t = fermi_apply_elem_w<W>(e, r, L, mask);
            double cr = e.ch_re, ci = PM1 ? 0.0 : e.ch_im;
            if (signs && fermi_parity<W>(e, bs.fsign + (size_t)g * L, r, L, false)) { cr = -cr; ci = -ci; }
            // conj(chi sign) v
            const double wr = CPLX ? cr * vr + ci * vi : cr * vr, wi = CPLX ? cr * vi - ci * vr : 0.0;
            expand_store_fermi<W, CPLX, KIND>(t, wr, wi, ex, weight, mask, s_binom, s_tab, out, err);
        }
    }
}

extern "C" int lsk_expand_fermi_push(lsk_basis bs, lsk_expand_fermi ex, uint64_t const *d_binom, int cplx, int64_t n, uint64_t const *reps,
                                     double const *norms, void const *psi, void *out, int *d_err, void *stream) {
    if (n <= 0) return 0;
    if (bs.spin_inversion != 0 || (bs.fermi && !bs.fsign) || (!bs.fermi && bs.n_elems != 1) || bs.number_sites < 1 || bs.number_sites > 64) {
        snprintf(g_err, sizeof(g_err), "%s: not a fermionic basis (a group without its sign table, or a spin inversion)", __func__);
        return -1;
    }
    if (!cplx && !bs.chars_pm1) { snprintf(g_err, sizeof(g_err), "%s: f64 needs +-1 characters", __func__); return -1; }
    const int M = bs.number_sites;
    bool ok = ex.n_a >= 0 && ex.n_b >= 0 && ex.n_a + ex.n_b == M && (ex.mask_a & ex.mask_b) == 0 && (ex.mask_a | ex.mask_b) == bs.site_mask;
    if (ex.kind == KIND_FIXED) ok = ok && ex.tab && bs.hamming_weight >= 0 && bs.hamming_weight < LSK_BINOM_K;
    else if (ex.kind == KIND_PRODUCT)
        ok = ok && ex.tab && bs.hamming_weight < 0 && M == 2 * ex.half && ex.half >= 1 && ex.half <= 32 && ex.au >= 0 && ex.au <= ex.half &&
             ex.ad >= 0 && ex.ad <= ex.half && ex.au + ex.ad == ex.n_a && ex.n_up >= 0 && ex.n_up <= ex.half && ex.n_dn >= 0 &&
             ex.n_dn <= ex.half && (ex.au + 1) * (ex.ad + 1) <= LSK_EXPAND_FERMI_TAB;
    else ok = ok && ex.kind == KIND_ALL && bs.hamming_weight < 0 && M <= 40 && ex.cols == ((int64_t)1 << ex.n_b);
    if (!ok) { snprintf(g_err, sizeof(g_err), "%s: the block layout does not belong to the basis", __func__); return -1; }
    // rows x elements: with few row tiles the elements are dealt to blockIdx.y, so that small sectors with large groups fill the device too
    const int64_t tiles = (n + kBlock - 1) / kBlock;
    int64_t gy = (kMaxGrid + tiles - 1) / tiles;
    if (gy > bs.n_elems) gy = bs.n_elems;
    if (gy > 1024) gy = 1024;
    if (gy < 1) gy = 1;
    const dim3 g((unsigned)(tiles < ((int64_t)1 << 22) ? tiles : ((int64_t)1 << 22)), (unsigned)gy), b(kBlock);
    hipStream_t s = (hipStream_t)stream;
#define LSK_FX_ARGS bs, bs.elems, ex, d_binom, n, reps, norms, (double const *)psi, (double *)out, d_err
#define LSK_FX_ONE(W, PM1, CPLX)                                                                                                          \
    do {                                                                                                                                  \
        if (ex.kind == KIND_FIXED) hipLaunchKernelGGL((k_expand_push_fermi<W, PM1, CPLX, KIND_FIXED>), g, b, 0, s, LSK_FX_ARGS);          \
        else if (ex.kind == KIND_PRODUCT) hipLaunchKernelGGL((k_expand_push_fermi<W, PM1, CPLX, KIND_PRODUCT>), g, b, 0, s, LSK_FX_ARGS); \
        else hipLaunchKernelGGL((k_expand_push_fermi<W, PM1, CPLX, KIND_ALL>), g, b, 0, s, LSK_FX_ARGS);                                  \
    } while (0)
    // {32, 64-bit words} x {f64 (+-1 characters) | c128 x {+-1, complex characters}} x {all states, fixed number, product}: 18 kernels
#define LSK_FX_LAUNCH(W)                                                                                                                  \
    do {                                                                                                                                  \
        if (!cplx) LSK_FX_ONE(W, true, false);                                                                                            \
        else if (bs.chars_pm1) LSK_FX_ONE(W, true, true);                                                                                 \
        else LSK_FX_ONE(W, false, true);                                                                                                  \
    } while (0)
    if (M <= 32) LSK_FX_LAUNCH(uint32_t); else LSK_FX_LAUNCH(uint64_t);
#undef LSK_FX_LAUNCH
#undef LSK_FX_ONE
#undef LSK_FX_ARGS
    LSK_LAUNCH_CHECK();
    return 0;
}
