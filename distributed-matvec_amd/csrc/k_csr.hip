// k_csr.hip -- the matrix of a cross-sector plan written out as canonical CSR (ls_amd_cross_csr, host.c).
//   k_cross_pull   the template of k_cross_t.hpp in its emitting mode (word type cross_emit_w<W>): stages A, B1, B2 as in the apply
//                  kernels, and every packet that reached a source row stored as (source index, coefficient) in the raw slot
//                  off[row] + (its rank among the row's packets in ascending group order).  Run twice: a counting pass (off == NULL)
//                  whose per-row counts are scanned into off, then the fill.  Plain stores, each slot written once.
//   k_csr_merge    one wave per row: entries of one column are summed into the first of them in ascending slot order (= ascending
//                  group), the others and the sums that cancel (|sum| <= 1e-12 sum |s|) are marked; counts what is left
//   k_csr_write    one wave per row: rank of every entry left among the row's columns -> its place in the final arrays
// Nothing depends on the order in which threads or waves arrive, so two exports of one plan are the same bits.  The 20 emitting
// kinds ({32, 64-bit words} x {f64 | c128 x {+-1, complex characters} x {real, complex terms}} x {FERMI off, on}) live
// here so that k_cross.hip and k_cross_fermi.hip keep their ten kernels each.
#include "k_cross_t.hpp"

extern "C" int lsk_cross_emit(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                              lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, double tiny,
                              int64_t const *off, int64_t *cnt, int64_t *col, void *val, int *d_err, void *stream) {
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (!cplx && !(is_real && src.chars_pm1)) { snprintf(g_err, sizeof(g_err), "%s: f64 needs a real operator and +-1 characters", __func__); return -1; }
    if (src.fermi) { // the preconditions of lsk_cross_fermi_pull
        if (!src.fsign || src.spin_inversion != 0 || src.k4_mode != 0 || src.proj != LSK_PROJ_FULL) {
            snprintf(g_err, sizeof(g_err), "%s: not a projected fermionic basis in K4 mode 0", __func__);
            return -1;
        }
        if (!gt.entries || gt.L != src.number_sites) { snprintf(g_err, sizeof(g_err), "%s: a projected fermionic source is looked up in its static index table", __func__); return -1; }
    } else if (src.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected source is looked up by its index", __func__); return -1; }
    if (off ? (!col || !val) : !cnt) { snprintf(g_err, sizeof(g_err), "%s: NULL output", __func__); return -1; }
    const int64_t work_blocks = (n_dst + kBlock - 1) / kBlock;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(1), b(kBlock);
    // (the emitting mode's reading of the kernel's parameter list: k_cross_t.hpp)
    double const *const e_x = (double const *)off;
    double *const e_y = (double *)val;
    unsigned long long *const e_count = (unsigned long long *)(off ? col : cnt);
#define LSK_CE_ONE(W, PM1, CPLX, REAL, FERMI)                                                                                            \
    do {                                                                                                                                 \
        g.x = resident_grid(k_cross_pull<cross_emit_w<W>, PM1, CPLX, REAL, FERMI>, work_blocks);                                         \
        hipLaunchKernelGGL((k_cross_pull<cross_emit_w<W>, PM1, CPLX, REAL, FERMI>), g, b, 0, s, n_groups, groups, terms, src, src.elems, \
                           six, gt, n_dst, dst_reps, dst_norms, e_x, e_y, tiny, e_count, d_err);                                         \
    } while (0)
#define LSK_CE_LAUNCH(W, FERMI)                                                                                                          \
    do {                                                                                                                                 \
        if (!cplx) LSK_CE_ONE(W, true, false, true, FERMI);                                                                              \
        else if (src.chars_pm1) { if (is_real) LSK_CE_ONE(W, true, true, true, FERMI); else LSK_CE_ONE(W, true, true, false, FERMI); }   \
        else { if (is_real) LSK_CE_ONE(W, false, true, true, FERMI); else LSK_CE_ONE(W, false, true, false, FERMI); }                    \
    } while (0)
    if (src.fermi) { if (src.number_sites <= 32) LSK_CE_LAUNCH(uint32_t, true); else LSK_CE_LAUNCH(uint64_t, true); }
    else { if (src.number_sites <= 32) LSK_CE_LAUNCH(uint32_t, false); else LSK_CE_LAUNCH(uint64_t, false); }
#undef LSK_CE_LAUNCH
#undef LSK_CE_ONE
    LSK_LAUNCH_CHECK();
    return 0;
}

// ---- canonicalisation: one wave per row (blocks of one wave, so that a block barrier orders the wave's LDS and global traffic) ----
constexpr int kCsrWave = 64;
constexpr int kCsrMaxGrid = 256 * 32; // 256 CUs x 32 resident waves: grid-stride beyond this
constexpr double kCsrCancel = 1e-12;  // a merged entry with |sum| <= kCsrCancel sum |s| is a cancellation, not an entry

static int csr_grid(int64_t n_rows) { return (int)(n_rows < 1 ? 1 : (n_rows < kCsrMaxGrid ? n_rows : kCsrMaxGrid)); }

// a raw column as the merge pass may have marked it (-2 - col: merged away or cancelled)
__device__ __forceinline__ int64_t csr_unmark(int64_t c) { return c < 0 ? -2 - c : c; }

// Lane l owns entry j = jc + l of the row, 64 at a time; for each of them the whole row goes by in LDS chunks of 64.  An entry is
// the head of its column when no earlier entry has the column; the head's sum runs over the row in ascending slot order.  Marks
// are written after an entry's sweep and are reversible, so that later chunks still see every column; a head's sum replaces its own
// value, which only the head reads.  A row longer than 64 costs (m / 64)^2 chunk sweeps: rows are as long as the operator has
// flip masks.
template <bool CPLX>
__global__ __launch_bounds__(kCsrWave) void k_csr_merge(int64_t n_rows, int64_t const *__restrict__ off, int64_t *col, double *val,
                                                        int64_t *__restrict__ cnt) {
    __shared__ int64_t s_col[kCsrWave];
    __shared__ double s_val[kCsrWave * (CPLX ? 2 : 1)];
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int64_t b = off[row], m = off[row + 1] - b;
        int64_t left = 0;
        for (int64_t jc = 0; jc < m; jc += kCsrWave) {
            const int64_t j = jc + lane;
            const bool have = j < m;
            const int64_t cj = have ? csr_unmark(col[b + j]) : -1;
            bool head = have;
            double sr = 0.0, si = 0.0, sabs = 0.0;
            for (int64_t qc = 0; qc < m; qc += kCsrWave) {
                __syncthreads(); // the chunk before is read, the marks and sums of the sweep before are stored
                const int64_t q = qc + lane;
                s_col[lane] = q < m ? csr_unmark(col[b + q]) : -1;
                if (CPLX) { s_val[2 * lane] = q < m ? val[2 * (b + q)] : 0.0; s_val[2 * lane + 1] = q < m ? val[2 * (b + q) + 1] : 0.0; }
                else s_val[lane] = q < m ? val[b + q] : 0.0;
                __syncthreads();
                const int len = (int)(m - qc < kCsrWave ? m - qc : kCsrWave);
                for (int k = 0; k < len; ++k) {
                    if (s_col[k] != cj) continue;
                    if (qc + k < j) head = false;
                    if (CPLX) { const double vr = s_val[2 * k], vi = s_val[2 * k + 1]; sr += vr; si += vi; sabs += sqrt(vr * vr + vi * vi); }
                    else { const double vr = s_val[k]; sr += vr; sabs += fabs(vr); }
                }
            }
            const bool keep = head && (CPLX ? sqrt(sr * sr + si * si) : fabs(sr)) > kCsrCancel * sabs;
            if (have) {
                if (!keep) col[b + j] = -2 - cj;
                else if (CPLX) { val[2 * (b + j)] = sr; val[2 * (b + j) + 1] = si; }
                else val[b + j] = sr;
            }
            left += __popcll(__ballot(keep));
        }
        if (lane == 0) cnt[row] = left;
        __syncthreads();
    }
}

template <bool CPLX>
__global__ __launch_bounds__(kCsrWave) void k_csr_write(int64_t n_rows, int64_t const *__restrict__ off, int64_t const *__restrict__ col,
                                                        double const *__restrict__ val, int64_t const *__restrict__ row_ptr,
                                                        int64_t *__restrict__ out_col, double *__restrict__ out_val) {
    __shared__ int64_t s_col[kCsrWave];
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int64_t b = off[row], m = off[row + 1] - b, o = row_ptr[row], left = row_ptr[row + 1] - o;
        for (int64_t jc = 0; jc < m; jc += kCsrWave) {
            const int64_t j = jc + lane;
            const int64_t cj = j < m ? col[b + j] : -1; // (a marked entry is negative)
            int64_t rank = 0;
            for (int64_t qc = 0; qc < m; qc += kCsrWave) {
                __syncthreads();
                s_col[lane] = qc + lane < m ? col[b + qc + lane] : -1;
                __syncthreads();
                const int len = (int)(m - qc < kCsrWave ? m - qc : kCsrWave);
                for (int k = 0; k < len; ++k) rank += (s_col[k] >= 0 && s_col[k] < cj) ? 1 : 0;
            }
            if (cj >= 0 && rank < left) { // (rank < left always: the merge pass counted the same entries)
                out_col[o + rank] = cj;
                if (CPLX) { out_val[2 * (o + rank)] = val[2 * (b + j)]; out_val[2 * (o + rank) + 1] = val[2 * (b + j) + 1]; }
                else out_val[o + rank] = val[b + j];
            }
        }
        __syncthreads();
    }
}

extern "C" int lsk_csr_merge(int cplx, int64_t n_rows, int64_t const *off, int64_t *col, void *val, int64_t *cnt, void *stream) {
    if (n_rows <= 0) return 0;
    if (!off || !cnt) { snprintf(g_err, sizeof(g_err), "%s: NULL argument", __func__); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (cplx) hipLaunchKernelGGL(k_csr_merge<true>, dim3(csr_grid(n_rows)), dim3(kCsrWave), 0, s, n_rows, off, col, (double *)val, cnt);
    else hipLaunchKernelGGL(k_csr_merge<false>, dim3(csr_grid(n_rows)), dim3(kCsrWave), 0, s, n_rows, off, col, (double *)val, cnt);
    LSK_LAUNCH_CHECK();
    return 0;
}

extern "C" int lsk_csr_write(int cplx, int64_t n_rows, int64_t const *off, int64_t const *col, void const *val, int64_t const *row_ptr,
                             int64_t *out_col, void *out_val, void *stream) {
    if (n_rows <= 0) return 0;
    if (!off || !row_ptr) { snprintf(g_err, sizeof(g_err), "%s: NULL argument", __func__); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (cplx) hipLaunchKernelGGL(k_csr_write<true>, dim3(csr_grid(n_rows)), dim3(kCsrWave), 0, s, n_rows, off, col, (double const *)val, row_ptr, out_col, (double *)out_val);
    else hipLaunchKernelGGL(k_csr_write<false>, dim3(csr_grid(n_rows)), dim3(kCsrWave), 0, s, n_rows, off, col, (double const *)val, row_ptr, out_col, (double *)out_val);
    LSK_LAUNCH_CHECK();
    return 0;
}
