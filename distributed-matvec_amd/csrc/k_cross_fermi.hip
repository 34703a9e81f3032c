// k_cross_fermi.hip -- cross-sector operators between projected FERMIONIC bases (spinless; spinful over their 2 L modes): the
// k_cross_pull template of k_cross_t.hpp with its FERMI switch on, so that stage B1 projects every packet into the source basis with the
// signed characters chi(g) sign(g, a) of lsk_fermi.hpp.  c+_k, c_k, n_q, S^z_q between the (momentum, point-group, flip) sectors of
// a t-V or Hubbard model: the Jordan-Wigner signs of the operator are in the terms' sign masks, the permutation signs of the
// projection are here.  The same 10 kinds as k_cross.hip; a translation unit of its own so that k_cross.hip and k_fermi.hip keep
// their kernel counts (tests pin both).  DESIGN.md section 6b.
#include "k_cross_t.hpp"

// the name of the family in plans and reports: k_cross_pull<W, PM1, CPLX, REAL, FERMI = true>
extern "C" char const *lsk_cross_fermi_kernel_name(void) { return "k_cross_pull_fermi"; }

// lsk_cross_pull for src.fermi (same arguments; reached through it).  The source is always projected, so always looked up in its
// static index table: the sign table and the table's key width bound every shift and load of the kernel.
extern "C" int lsk_cross_fermi_pull(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                                    lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, void const *x,
                                    void *y, double tiny, unsigned long long *d_count, int *d_err, void *stream) {
    if (!src.fermi || !src.fsign || src.spin_inversion != 0 || src.k4_mode != 0 || src.proj != LSK_PROJ_FULL) {
        snprintf(g_err, sizeof(g_err), "%s: not a projected fermionic basis in K4 mode 0", __func__);
        return -1;
    }
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (!gt.entries || gt.L != src.number_sites) { snprintf(g_err, sizeof(g_err), "%s: a projected fermionic source is looked up in its static index table", __func__); return -1; }
    if (!cplx && !(is_real && src.chars_pm1)) { snprintf(g_err, sizeof(g_err), "%s: f64 needs a real operator and +-1 characters", __func__); return -1; }
    const int64_t work_blocks = (n_dst + kBlock - 1) / kBlock;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(1), b(kBlock);
#define LSK_CXF_ARGS n_groups, groups, terms, src, src.elems, six, gt, n_dst, dst_reps, dst_norms, (double const *)x, (double *)y, tiny, d_count, d_err
#define LSK_CXF_ONE(W, PM1, CPLX, REAL)                                                                                                  \
    do { g.x = resident_grid(k_cross_pull<W, PM1, CPLX, REAL, true>, work_blocks); hipLaunchKernelGGL((k_cross_pull<W, PM1, CPLX, REAL, true>), g, b, 0, s, LSK_CXF_ARGS); } while (0)
    // {32, 64-bit words} x {f64 (real terms, +-1 characters) | c128 x {+-1, complex characters} x {real, complex terms}}: 10 kernels
#define LSK_CXF_LAUNCH(W)                                                                                                                \
    do {                                                                                                                                 \
        if (!cplx) LSK_CXF_ONE(W, true, false, true);                                                                                    \
        else if (src.chars_pm1) { if (is_real) LSK_CXF_ONE(W, true, true, true); else LSK_CXF_ONE(W, true, true, false); }               \
        else { if (is_real) LSK_CXF_ONE(W, false, true, true); else LSK_CXF_ONE(W, false, true, false); }                                \
    } while (0)
    if (src.number_sites <= 32) LSK_CXF_LAUNCH(uint32_t); else LSK_CXF_LAUNCH(uint64_t);
#undef LSK_CXF_LAUNCH
#undef LSK_CXF_ONE
#undef LSK_CXF_ARGS
    LSK_LAUNCH_CHECK();
    return 0;
}
