// k_expand.hip -- sector-state expansion (ls_amd_expand, host.c): a vector psi on the representatives of a
// symmetry sector, scattered over the orbits of its representatives into the matrix M[a, b] = <a, b|psi> of a bipartition.
// Push form: the image s = g r of representative r under group element g receives
//     <s|psi> = conj(chi(g)) n(r) psi[r]          (flipped image under the spin inversion: character chi(g) inv)
// -- |reps| |G| ~ |full basis| element applications; the pull form (one thread per full state, orbit minimum and look-up) costs
// |G| times more.  Several g reach the same s when r has a stabiliser; they store the same value (n(r) > 0 forces chi = 1 on the
// stabiliser), so plain stores are enough.  States of zero-norm orbits receive nothing: the host clears the blocks first.
// Lane mapping: one ROW per lane, the element loop outside -- the element descriptor (network masks, character) is wave-uniform and
// stays in scalar registers, as in state_info_w; blockIdx.y deals the elements to several blocks when there are few row tiles.
// Spin-1/2 bases; the fermionic variant with the orbit sign and the sign of the bipartition is k_expand_push_fermi (k_expand_fermi.hip).
#include "lsk_dev.hpp"

extern "C" char const *lsk_expand_kernel_name(void) { return "k_expand_push"; }

__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ULL : ((1ULL << n) - 1); }
__device__ __forceinline__ uint64_t shr_sites(uint64_t s, int n) { return n >= 64 ? 0ULL : (s >> n); }
// the bits of s on the sites of m, compacted in ascending site order (m is wave-uniform: so is the trip count)
__device__ __forceinline__ uint64_t gather_bits(uint64_t s, uint64_t m) {
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

// one image: split by the subsystem, rank both halves, store.  An image that is not a state of the basis raises *err and is dropped;
// every index below is then inside its block: rank(a) < C(n_a, n_A), rank(b) < C(n_b, w - n_A) (a < 2^n_a, b < 2^n_b without a weight)
template <typename W, bool CPLX, bool FIXED>
__device__ __forceinline__ void expand_store(W t, double cr, double ci, double vr, double vi, lsk_expand const &ex, int weight, W mask,
                                             uint64_t const *s_binom, int64_t const *s_tab, double *__restrict__ out, int *err) {
    if ((W)(t & (W)~mask) != 0 || (FIXED && WordTraits<W>::popc(t) != weight)) { atomicExch(err, 1); return; }
    const uint64_t s = (uint64_t)t;
    uint64_t a, b;
    if (ex.split == LSK_SPLIT_LOW) { a = s & low_bits(ex.n_a); b = shr_sites(s, ex.n_a); }
    else if (ex.split == LSK_SPLIT_HIGH) { b = s & low_bits(ex.n_b); a = shr_sites(s, ex.n_b); }
    else { a = gather_bits(s, ex.mask_a); b = gather_bits(s, (uint64_t)mask & ~ex.mask_a); }
    int64_t idx;
    if (FIXED) {
        const int na = __popcll(a);
        if (na < ex.na_lo || na > ex.na_hi) return; // a block that was not asked for
        const int64_t off = s_tab[na];
        if (off < 0) { atomicExch(err, 1); return; }
        idx = off + rank_combinadic(a, s_binom) * s_tab[LSK_EXPAND_MAX_NA + na] + rank_combinadic(b, s_binom);
    } else idx = (int64_t)a * ex.cols + (int64_t)b;
    if (CPLX) reinterpret_cast<double2 *>(out)[idx] = make_double2(cr * vr + ci * vi, cr * vi - ci * vr); // conj(chi) v
    else out[idx] = cr * vr;
}

template <typename W, bool PM1, bool CPLX, bool FIXED>
__global__ __launch_bounds__(kBlock) void k_expand_push(lsk_basis bs, lsk_group_elem const *__restrict__ elems, lsk_expand ex,
                                                        uint64_t const *__restrict__ g_binom, int64_t n,
                                                        uint64_t const *__restrict__ reps, double const *__restrict__ norms,
                                                        double const *__restrict__ psi, double *__restrict__ out, int *err) {
    __shared__ uint64_t s_binom[FIXED ? 64 * LSK_BINOM_K : 1];
    __shared__ int64_t s_tab[FIXED ? 2 * LSK_EXPAND_MAX_NA : 1];
    if (FIXED) {
        for (int i = threadIdx.x; i < 2 * LSK_EXPAND_MAX_NA; i += blockDim.x) s_tab[i] = ex.tab[i];
        load_binom(s_binom, g_binom); // (synchronises the block)
    }
    const int L = bs.number_sites, weight = bs.hamming_weight, inv = bs.spin_inversion;
    const W mask = (W)bs.site_mask;
#ifdef LSK_EXPAND_PAIR_LANES
    // A/B builds: one (row, element) PAIR per lane, elements fastest -- a wave stores every image of 64 / |G|
    // consecutive rows; the element descriptor is a per-lane load.  Never the product build: what it measured is in DESIGN.md section 5.
    for (int64_t w0 = (int64_t)blockIdx.x * kBlock; w0 < n * bs.n_elems; w0 += (int64_t)gridDim.x * kBlock) {
        const int64_t w = w0 + threadIdx.x;
        if (w >= n * bs.n_elems || blockIdx.y != 0) continue;
        const int64_t i = w / bs.n_elems;
        const int g = (int)(w - i * bs.n_elems);
        const uint64_t r64 = reps[i];
        const double nr = norms[i];
        if ((r64 & ~bs.site_mask) != 0 || (FIXED && __popcll(r64) != weight)) { atomicExch(err, 1); continue; }
        if (!(nr > 0.0)) continue;
        double vr, vi = 0.0;
        if (CPLX) { vr = nr * psi[2 * i]; vi = nr * psi[2 * i + 1]; } else vr = nr * psi[i];
        lsk_group_elem const &e = elems[g];
        const W t = apply_elem_w<W>(e, (W)r64, L, mask);
        const double cr = e.ch_re, ci = PM1 ? 0.0 : e.ch_im;
        expand_store<W, CPLX, FIXED>(t, cr, ci, vr, vi, ex, weight, mask, s_binom, s_tab, out, err);
        if (inv != 0) expand_store<W, CPLX, FIXED>((W)(t ^ mask), cr * (double)inv, ci * (double)inv, vr, vi, ex, weight, mask, s_binom, s_tab, out, err);
    }
    return;
#endif
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n; t0 += (int64_t)gridDim.x * kBlock) {
        const int64_t i = t0 + threadIdx.x;
        bool valid = i < n;
        W r = 0;
        double vr = 0.0, vi = 0.0;
        if (valid) {
            const uint64_t r64 = reps[i];
            const double nr = norms[i];
            if ((r64 & ~bs.site_mask) != 0 || (FIXED && __popcll(r64) != weight)) { // not a state of this basis
                if (blockIdx.y == 0) atomicExch(err, 1);
                valid = false;
            }
            if (!(nr > 0.0)) valid = false; // a zero-norm orbit is no basis vector: nothing to scatter
            r = (W)r64;
            if (CPLX) { vr = nr * psi[2 * i]; vi = nr * psi[2 * i + 1]; } else vr = nr * psi[i];
        }
        for (int g = blockIdx.y; g < bs.n_elems; g += gridDim.y) {
            lsk_group_elem const &e = elems[g];
            if (!valid) continue;
            const W t = apply_elem_w<W>(e, r, L, mask);
            const double cr = e.ch_re, ci = PM1 ? 0.0 : e.ch_im;
            expand_store<W, CPLX, FIXED>(t, cr, ci, vr, vi, ex, weight, mask, s_binom, s_tab, out, err);
            if (inv != 0) expand_store<W, CPLX, FIXED>((W)(t ^ mask), cr * (double)inv, ci * (double)inv, vr, vi, ex, weight, mask, s_binom, s_tab, out, err);
        }
    }
}

extern "C" int lsk_expand_push(lsk_basis bs, lsk_expand ex, uint64_t const *d_binom, int cplx, int64_t n, uint64_t const *reps,
                               double const *norms, void const *psi, void *out, int *d_err, void *stream) {
    if (n <= 0) return 0;
    if (bs.fermi) { snprintf(g_err, sizeof(g_err), "%s: fermionic bases are not expanded here (mode-ordering signs: lsk_expand_fermi_push)", __func__); return -1; }
    if (!cplx && !bs.chars_pm1) { snprintf(g_err, sizeof(g_err), "%s: f64 needs +-1 characters", __func__); return -1; }
    const bool fixed = bs.hamming_weight >= 0;
    if (fixed && (!ex.tab || bs.hamming_weight >= LSK_BINOM_K)) { snprintf(g_err, sizeof(g_err), "%s: no block table, or a weight beyond the binomial table", __func__); return -1; }
    // rows x elements: with few row tiles the elements are dealt to blockIdx.y, so that small sectors with large groups fill the device too
    const int64_t tiles = (n + kBlock - 1) / kBlock;
    int64_t gy = (kMaxGrid + tiles - 1) / tiles;
    if (gy > bs.n_elems) gy = bs.n_elems;
    if (gy > 1024) gy = 1024;
    if (gy < 1) gy = 1;
#ifdef LSK_EXPAND_PAIR_LANES
    const int64_t pair_tiles = (n * bs.n_elems + kBlock - 1) / kBlock;
    const dim3 g((unsigned)(pair_tiles < ((int64_t)1 << 24) ? pair_tiles : ((int64_t)1 << 24)), 1u), b(kBlock);
#else
    const dim3 g((unsigned)(tiles < ((int64_t)1 << 22) ? tiles : ((int64_t)1 << 22)), (unsigned)gy), b(kBlock);
#endif
    hipStream_t s = (hipStream_t)stream;
#define LSK_EX_ARGS bs, bs.elems, ex, d_binom, n, reps, norms, (double const *)psi, (double *)out, d_err
#define LSK_EX_ONE(W, PM1, CPLX)                                                                                                          \
    do {                                                                                                                                  \
        if (fixed) hipLaunchKernelGGL((k_expand_push<W, PM1, CPLX, true>), g, b, 0, s, LSK_EX_ARGS);                                      \
        else hipLaunchKernelGGL((k_expand_push<W, PM1, CPLX, false>), g, b, 0, s, LSK_EX_ARGS);                                           \
    } while (0)
    // {32, 64-bit words} x {f64 (+-1 characters) | c128 x {+-1, complex characters}} x {fixed weight, all states}: 12 kernels
#define LSK_EX_LAUNCH(W)                                                                                                                  \
    do {                                                                                                                                  \
        if (!cplx) LSK_EX_ONE(W, true, false);                                                                                            \
        else if (bs.chars_pm1) LSK_EX_ONE(W, true, true);                                                                                 \
        else LSK_EX_ONE(W, false, true);                                                                                                  \
    } while (0)
    if (bs.number_sites <= 32) LSK_EX_LAUNCH(uint32_t); else LSK_EX_LAUNCH(uint64_t);
#undef LSK_EX_LAUNCH
#undef LSK_EX_ONE
#undef LSK_EX_ARGS
    LSK_LAUNCH_CHECK();
    return 0;
}
