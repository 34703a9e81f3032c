// k_corr.hip -- two-point correlation matrices of a sector state (ls_amd_corr, host.c): sums over the
// representatives alone, which the host averages over the group.
//   k_corr_diag  the densities: the weighted Gram matrix of the bit strings, D[i][j] = sum_r |psi_r|^2 b_i(r) b_j(r), i <= j.  No
//                look-up, no character, no sign.  A tile of (representative, |psi_r|^2) is staged in LDS; every thread owns KPT of
//                the M (M + 1) / 2 pairs and walks the tile's rows: one broadcast LDS read, a mask test and an add per pair.
//   k_corr_hop   the hoppings (k_corr_t.hpp); this unit holds the 6 instantiations without permutation signs, and lsk_corr_hop
//                hands a projected fermionic basis to the signed ones of k_corr_fermi.hip.
//   k_corr_sum   the partial sums of the blocks, added in ascending block order: no floating-point atomics in either kernel.
#include "k_corr_t.hpp"

extern "C" char const *lsk_corr_diag_kernel_name(void) { return "k_corr_diag"; }
extern "C" char const *lsk_corr_hop_kernel_name(void) { return "k_corr_hop"; }

// the most blocks a launch over n rows has (corr_grid, k_corr_t.hpp): the rows of `partial` the caller provides
extern "C" int lsk_corr_blocks(int64_t n) {
    const int64_t tiles = (n + kBlock - 1) / kBlock;
    return (int)(tiles < 1 ? 1 : (tiles > kCorrMaxBlocks ? kCorrMaxBlocks : tiles));
}

__global__ __launch_bounds__(kBlock) void k_corr_sum(int blocks, int m, double const *__restrict__ partial, double *__restrict__ out) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= m) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partial[(size_t)b * m + q];
    out[q] = s;
}

extern "C" int lsk_corr_sum(int blocks, int m, double const *partial, double *out, void *stream) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_corr_sum, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, blocks, m, partial, out);
    LSK_LAUNCH_CHECK();
    return 0;
}

template <typename W, bool CPLX, int KPT>
__global__ __launch_bounds__(kBlock) void k_corr_diag(int n_pairs, uint16_t const *__restrict__ pairs, int64_t n,
                                                      uint64_t const *__restrict__ reps, double const *__restrict__ psi,
                                                      double *__restrict__ partial) {
    __shared__ W s_rep[kBlock];
    __shared__ double s_w[kBlock];
    const int tid = threadIdx.x;
    W mask[KPT];
    double acc[KPT];
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        const int q = tid + k * kBlock;
        mask[k] = 0; // (a slot beyond the pairs: it matches every row, and is never stored)
        if (q < n_pairs) { const uint32_t pr = pairs[q]; mask[k] = (W)(((W)1 << (pr & 0xff)) | ((W)1 << (pr >> 8))); }
        acc[k] = 0.0;
    }
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n; t0 += (int64_t)gridDim.x * kBlock) {
        const int64_t i = t0 + tid;
        W a = 0;
        double w = 0.0; // (rows beyond n weigh nothing)
        if (i < n) {
            a = (W)reps[i];
            if (CPLX) { const double re = psi[2 * i], im = psi[2 * i + 1]; w = re * re + im * im; } else w = psi[i] * psi[i];
        }
        s_rep[tid] = a;
        s_w[tid] = w;
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < kBlock; ++r) {
            const W b = s_rep[r];
            const double wr = s_w[r];
#pragma unroll
            for (int k = 0; k < KPT; ++k) acc[k] += (b & mask[k]) == mask[k] ? wr : 0.0;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        const int q = tid + k * kBlock;
        if (q < n_pairs) partial[(size_t)blockIdx.x * n_pairs + q] = acc[k];
    }
}

extern "C" int lsk_corr_diag(int modes, int n_pairs, uint16_t const *pairs, int cplx, int64_t n, uint64_t const *reps, void const *psi,
                             double *partial, double *out, void *stream) {
    if (n <= 0 || n_pairs <= 0) return 0;
    if (n_pairs > 9 * kBlock) { snprintf(g_err, sizeof(g_err), "%s: %d pairs, at most %d (64 modes)", __func__, n_pairs, 9 * kBlock); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int blocks = corr_grid(n);
    dim3 g(blocks), b(kBlock);
#define LSK_CD_ONE(W, CPLX, KPT) hipLaunchKernelGGL((k_corr_diag<W, CPLX, KPT>), g, b, 0, s, n_pairs, pairs, n, reps, (double const *)psi, partial)
    // pairs per thread: 1, 2, 3 (32 modes: 528 pairs) -- all that 32-bit words need --, 5, 9 (64 modes: 2080 pairs)
#define LSK_CD_NARROW(CPLX)                                                                                                              \
    do {                                                                                                                                 \
        if (n_pairs <= kBlock) LSK_CD_ONE(uint32_t, CPLX, 1);                                                                            \
        else if (n_pairs <= 2 * kBlock) LSK_CD_ONE(uint32_t, CPLX, 2);                                                                   \
        else LSK_CD_ONE(uint32_t, CPLX, 3);                                                                                              \
    } while (0)
#define LSK_CD_WIDE(CPLX)                                                                                                                \
    do {                                                                                                                                 \
        if (n_pairs <= 3 * kBlock) LSK_CD_ONE(uint64_t, CPLX, 3);                                                                        \
        else if (n_pairs <= 5 * kBlock) LSK_CD_ONE(uint64_t, CPLX, 5);                                                                   \
        else LSK_CD_ONE(uint64_t, CPLX, 9);                                                                                              \
    } while (0)
    if (modes <= 32) { if (cplx) LSK_CD_NARROW(true); else LSK_CD_NARROW(false); }
    else { if (cplx) LSK_CD_WIDE(true); else LSK_CD_WIDE(false); }
#undef LSK_CD_WIDE
#undef LSK_CD_NARROW
#undef LSK_CD_ONE
    LSK_LAUNCH_CHECK();
    return lsk_corr_sum(blocks, n_pairs, partial, out, stream);
}

extern "C" int lsk_corr_hop(lsk_basis bs, lsk_index six, lsk_gtab gt, int jw, int n_pairs, uint16_t const *pairs, int cplx, int64_t n,
                            uint64_t const *reps, double const *norms, void const *psi, double *partial, double *out, int *d_err,
                            void *stream) {
    if (bs.fermi) return lsk_corr_hop_fermi(bs, six, gt, jw, n_pairs, pairs, cplx, n, reps, norms, psi, partial, out, d_err, stream);
    return corr_hop_launch<false>(bs, six, gt, jw, n_pairs, pairs, cplx, n, reps, norms, psi, partial, out, d_err, stream);
}
