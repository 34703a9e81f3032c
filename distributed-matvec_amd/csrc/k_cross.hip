// k_cross.hip -- cross-sector operators: y2 = A x1 with x1 indexed by the representatives of a SOURCE basis and y2 by those of a
// TARGET basis (ls_amd_cross, host.c).  Pull form, modelled on k_tile_pull (k_pull.hip): one target row per thread, the adjoint's
// flip-mask groups expanded into an LDS packet list, every packet projected into the source basis and gathered from x1
//     y[r'] = sum_j conj(c+_j) chi1(g0j) n1(r) / n2(r') x[idx1(r)],    r = rep1(r' ^ x_j),  g0j (r' ^ x_j) = r
// (c+_j: coefficient of the adjoint's group j on r').  Only the norms and the look-up differ from the
// projection formula of section 6: they come from two bases.  Groups with flip mask 0 go through the same path -- row i of the
// target is not column i of the source.  No global atomics on y, y is assigned once per row.
// The kernel is the template of k_cross_t.hpp; this unit holds its 10 instantiations without permutation signs (FERMI = false),
// and lsk_cross_pull hands a projected fermionic source to the signed ones of k_cross_fermi.hip.
#include "k_cross_t.hpp" // the k_cross_pull template and its launcher cross_pull_launch, shared with k_cross_fermi.hip

extern "C" char const *lsk_cross_kernel_name(void) { return "k_cross_pull"; }

// d_count != NULL: nothing is read from x or written to y; the packets that reach a source row are added to *d_count
extern "C" int lsk_cross_pull(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                              lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, void const *x,
                              void *y, double tiny, unsigned long long *d_count, int *d_err, void *stream) {
    if (src.fermi) return lsk_cross_fermi_pull(n_groups, groups, terms, is_real, src, six, gt, cplx, n_dst, dst_reps, dst_norms, x, y, tiny, d_count, d_err, stream);
    return cross_pull_launch<false>(__func__, n_groups, groups, terms, is_real, src, six, gt, cplx, n_dst, dst_reps, dst_norms, x, y, tiny, d_count, d_err, stream);
}
