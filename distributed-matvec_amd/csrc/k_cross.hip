// k_cross.hip -- cross-sector operators: y2 = A x1 with x1 indexed by the representatives of a SOURCE basis and y2 by those of a
// TARGET basis (ls_amd_cross, host.c).  Pull form, modelled on k_tile_pull (k_pull.hip): one target row per thread, the adjoint's
// flip-mask groups expanded into an LDS packet list, every packet projected into the source basis and gathered from x1
//     y[r'] = sum_j conj(c+_j) chi1(g0j) n1(r) / n2(r') x[idx1(r)],    r = rep1(r' ^ x_j),  g0j (r' ^ x_j) = r
// (c+_j: coefficient of the adjoint's group j on r').  Only the norms and the look-up differ from the
// projection formula of section 6: they come from two bases.  Groups with flip mask 0 go through the same path -- row i of the
// target is not column i of the source.  No global atomics on y, y is assigned once per row.
// The kernel is the template of k_cross_t.hpp; this unit holds its 10 instantiations without permutation signs (FERMI = false),
// and lsk_cross_pull hands a projected fermionic source to the signed ones of k_cross_fermi.hip.
#include "k_cross_t.hpp" // the k_cross_pull template, shared with k_cross_fermi.hip

extern "C" char const *lsk_cross_kernel_name(void) { return "k_cross_pull"; }

// d_count != NULL: nothing is read from x or written to y; the packets that reach a source row are added to *d_count
extern "C" int lsk_cross_pull(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                              lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, void const *x,
                              void *y, double tiny, unsigned long long *d_count, int *d_err, void *stream) {
    if (src.fermi) return lsk_cross_fermi_pull(n_groups, groups, terms, is_real, src, six, gt, cplx, n_dst, dst_reps, dst_norms, x, y, tiny, d_count, d_err, stream);
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (!cplx && !(is_real && src.chars_pm1)) { snprintf(g_err, sizeof(g_err), "%s: f64 needs a real operator and +-1 characters", __func__); return -1; }
    if (src.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected source is looked up by its index", __func__); return -1; }
    const int64_t work_blocks = (n_dst + kBlock - 1) / kBlock;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(1), b(kBlock);
#define LSK_CX_ARGS n_groups, groups, terms, src, src.elems, six, gt, n_dst, dst_reps, dst_norms, (double const *)x, (double *)y, tiny, d_count, d_err
#define LSK_CX_ONE(W, PM1, CPLX, REAL)                                                                                                   \
    do { g.x = resident_grid(k_cross_pull<W, PM1, CPLX, REAL, false>, work_blocks); hipLaunchKernelGGL((k_cross_pull<W, PM1, CPLX, REAL, false>), g, b, 0, s, LSK_CX_ARGS); } while (0)
    // {32, 64-bit words} x {f64 (real terms, +-1 characters) | c128 x {+-1, complex characters} x {real, complex terms}}: 10 kernels
#define LSK_CX_LAUNCH(W)                                                                                                                 \
    do {                                                                                                                                 \
        if (!cplx) LSK_CX_ONE(W, true, false, true);                                                                                     \
        else if (src.chars_pm1) { if (is_real) LSK_CX_ONE(W, true, true, true); else LSK_CX_ONE(W, true, true, false); }                 \
        else { if (is_real) LSK_CX_ONE(W, false, true, true); else LSK_CX_ONE(W, false, true, false); }                                  \
    } while (0)
    if (src.number_sites <= 32) LSK_CX_LAUNCH(uint32_t); else LSK_CX_LAUNCH(uint64_t);
#undef LSK_CX_LAUNCH
#undef LSK_CX_ONE
#undef LSK_CX_ARGS
    LSK_LAUNCH_CHECK();
    return 0;
}
