// k_cheb.hip -- the Chebyshev / Lanczos step of the kernel polynomial method (ls_amd_matvec_block_axpby), one partition:
//     Y[:, k] <- alpha (H X)[:, k] + beta X[:, k] + gamma Y[:, k],   dots[k] = <X_k|X_k>,   dots[K + k] = Re <X_k|Y_k> (new Y)
// for K columns, alpha, beta, gamma real.  Three kernels, in a translation unit of their own (the four hot units keep their
// device-function budget, tests/test_block_matvec_abi.py):
//   k_axpby_dots        the epilogue pass after a matvec into W: reads W, X (and Y unless gamma == 0), writes Y -- 4 words per
//                       element next to the 2 of the matvec;
//   k_direct_cheb       the row loop of k_direct_blk (k_rows.hip) with the store of Y replaced by the update and the two partial
//                       sums: own x, y read, y written -- 3 words;
//   k_pull_gather_cheb  the row loop of k_pull_gather_blk (k_pull.hip), likewise.
// The two row loops are COPIES of the block kernels' loops, not shared with them: with the loop moved into a device function
// template (epilogue policy as a parameter, by value or by reference, with and without __restrict__ on the parameters) the
// compiler allocates the registers of all eight k_direct_blk instantiations differently, and their measured machine code
// (kernel_isa.json) must stay what it is.  A change to one of the loops has to be made in all three places
// (k_evolve.hip holds a third copy of each, with the accumulate of the time-evolution step).
// gamma == 0: Y is not read (it may hold NaN).  The dots are ADDED to d_dots by atomics: the caller clears them.
#include <hip/hip_runtime.h>
#include "k_pull_t.hpp" // pull_kinds, COEF_*, kNoSlot, pull_xcd_chunk (and lsk_dev.hpp)

template <bool CPLX> struct ChebCols { static constexpr int KB = CPLX ? 4 : 8; };
constexpr int kChebMaxCols = 64;

// The update of one element and its two summands.  Each column's summands go through a wave reduction (six cross-lane steps
// each) straight away -- held per lane until the end of the chunk, the 2 KB partial sums cost k_direct_cheb its eighth resident
// workgroup -- into the workgroup's LDS array s_dots[2][K], which the kernel sends out once, after its persistent loop: one
// atomic per (dot, column) and workgroup.  A wave whose lanes are not all in the chunk (the last tile of a list) adds lane by
// lane: cross-lane reads of idle lanes are not defined.  gamma == 0: Y is not read.
template <typename X> struct BlkCheb {
    double alpha, beta, gamma;
    double *s_dots; // LDS [2][K]; nullptr: no dots wanted
    int K;
    __device__ __forceinline__ void init(double a, double b, double g, double *lds, int K_, bool want) {
        alpha = a; beta = b; gamma = g; K = K_;
        s_dots = want ? lds : nullptr;
    }
    // Y[i, col] <- alpha h + beta xo + gamma Y[i, col]; sxx, sxy: this lane's summands of <X|X> and Re <X|Y>
    __device__ __forceinline__ void update(X xo, X *__restrict__ yp, X h, double &sxx, double &sxy) const {
        if constexpr (std::is_same<X, double2>::value) {
            double2 yn = make_double2(alpha * h.x + beta * xo.x, alpha * h.y + beta * xo.y);
            if (gamma != 0.0) { const double2 yo = *yp; yn.x += gamma * yo.x; yn.y += gamma * yo.y; }
            *yp = yn;
            sxx = xo.x * xo.x + xo.y * xo.y;
            sxy = xo.x * yn.x + xo.y * yn.y;
        } else {
            double yn = alpha * h + beta * xo;
            if (gamma != 0.0) yn += gamma * *yp;
            *yp = yn;
            sxx = xo * xo;
            sxy = xo * yn;
        }
    }
    // by every lane that is in the chunk (`full`: all 64 are), with zeros where a lane has no row
    __device__ __forceinline__ void reduce(int col, bool full, double a, double b) const {
        if (!s_dots) return; // (workgroup-uniform)
        if (full) {
            for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); }
            if ((threadIdx.x & 63) == 0) { atomicAdd(s_dots + col, a); atomicAdd(s_dots + K + col, b); }
        } else { atomicAdd(s_dots + col, a); atomicAdd(s_dots + K + col, b); }
    }
};

// the workgroup's sums: cleared before the persistent loop, sent out after it (one atomic per dot, column and workgroup)
__device__ __forceinline__ void cheb_dots_begin(double *s_dots, int K) {
    if (threadIdx.x < 2 * K) s_dots[threadIdx.x] = 0.0;
    __syncthreads();
}
__device__ __forceinline__ void cheb_dots_end(double const *s_dots, int K, double *__restrict__ dots) {
    __syncthreads();
    if (dots && threadIdx.x < 2 * K) unsafeAtomicAdd(dots + threadIdx.x, s_dots[threadIdx.x]);
}

// (<= 80 SGPRs, as k_direct_blk: the persistent grid is sized by the occupancy API, which over-reports the resident blocks from 81 on)
template <bool CPLX, int INDEX>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(80))) void k_direct_cheb(lsk_runs runs, int n_groups, lsk_group const *__restrict__ groups,
                                                       lsk_term const *__restrict__ off, int n_diag, lsk_term const *__restrict__ diag,
                                                       lsk_index ix, int weight, uint64_t const *__restrict__ tilemap,
                                                       int64_t slots_per_xcd, uint64_t const *__restrict__ reps, int K, double const *__restrict__ x,
                                                       int64_t xr, int64_t xc, double *__restrict__ y, int64_t yr, int64_t yc, double alpha,
                                                       double beta_, double gamma, double *__restrict__ dots, int *err) {
    __shared__ double s_dots[2 * kChebMaxCols];
    cheb_dots_begin(s_dots, K);
    BlkCheb<typename ChainX<CPLX>::type> ep;
    ep.init(alpha, beta_, gamma, s_dots, K, dots != nullptr);
    typedef typename ChainX<CPLX>::type X;
    constexpr bool REAL = !CPLX; // (f64 vectors only ever meet real operators: the plan refuses the other combination)
    constexpr int KB = ChebCols<CPLX>::KB;
    constexpr bool BINOM = INDEX == LSK_INDEX_COMBINADIC || INDEX == LSK_INDEX_PRODUCT;
    __shared__ uint64_t s_binom[BINOM ? 64 * LSK_BINOM_K : 1];
    if (BINOM) {
        for (int k = threadIdx.x; k < 64 * LSK_BINOM_K; k += blockDim.x) s_binom[k] = ix.binom[k];
        __syncthreads();
    }
    X const *__restrict__ xv = (X const *)x;
    X *__restrict__ yv = (X *)y;
    const int xcd = blockIdx.x & 7;
    const int64_t blocks_per_xcd = gridDim.x >> 3; // grid is a multiple of 8
    tilemap += (int64_t)xcd * slots_per_xcd;
    for (int64_t t = blockIdx.x >> 3; t < slots_per_xcd; t += blocks_per_xcd) {
        const uint64_t slot = tilemap[t]; // (first row, number of rows <= kBlock)
        if ((uint64_t)threadIdx.x >= (slot >> 48)) continue;
        const int64_t i = (int64_t)(slot & 0xffffffffffffULL) + threadIdx.x;
        const uint64_t a = __builtin_nontemporal_load(reps + i);
        double dr = 0.0, di = 0.0;
        if (n_diag > 0) diag_coeff<uint64_t, REAL>(runs, n_diag, diag, a, dr, di);
        for (int c0 = 0; c0 < K; c0 += KB) {
            const int kb = min(KB, K - c0); // wave-uniform
            X acc[KB];
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                acc[k] = cx_zero<X>();
                if (k < kb) {
                    const X xo = xv[i * xr + (int64_t)(c0 + k) * xc];
                    if constexpr (CPLX) acc[k] = make_double2(dr * xo.x - di * xo.y, dr * xo.y + di * xo.x);
                    else acc[k] = dr * xo;
                }
            }
            for (int g = 0; g < n_groups; ++g) {
                lsk_group const G = groups[g];
                double cr, ci;
                // <i|H_g|i ^ x_g>: the coefficient of the PARTNER's row expansion (any operator, as k_direct's pull form)
                const uint64_t beta = a ^ G.x;
                group_coeff<REAL>(G, off, beta, cr, ci);
                if (cr == 0.0 && (REAL || ci == 0.0)) continue;
                int64_t idx;
                if (INDEX == LSK_INDEX_IDENTITY) idx = (int64_t)beta;
                else if (INDEX == LSK_INDEX_COMBINADIC) {
                    if (__popcll(beta) != weight) { atomicExch(err, 1); continue; }
                    idx = rank_combinadic_w<uint64_t, uint64_t>(beta, s_binom);
                } else if constexpr (INDEX == LSK_INDEX_PRODUCT) idx = product_index(ix, beta, s_binom);
                else idx = search_index(ix, beta);
                if (idx < 0) { atomicExch(err, 1); continue; } // DMV:115-118
                X v[KB];
                X const *__restrict__ xp = xv + idx * xr;
#pragma unroll
                for (int k = 0; k < KB; ++k) v[k] = k < kb ? xp[(int64_t)(c0 + k) * xc] : cx_zero<X>();
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    if constexpr (CPLX) {
                        acc[k].x += cr * v[k].x - ci * v[k].y;
                        acc[k].y += cr * v[k].y + ci * v[k].x;
                    } else acc[k] = fma(cr, v[k], acc[k]);
                }
            }
            const bool full = __ballot(1) == ~0ULL; // (lanes past the end of the tile are not here)
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (k < kb) {
                    // (the row's own x again: the line was read at the top of the chunk -- a cache hit, and KB registers fewer across
                    // the gathers than keeping it)
                    const X xo = xv[i * xr + (int64_t)(c0 + k) * xc];
                    double sxx, sxy;
                    ep.update(xo, yv + (i * yr + (int64_t)(c0 + k) * yc), acc[k], sxx, sxy);
                    ep.reduce(c0 + k, full, sxx, sxy);
                }
        }
    }
    cheb_dots_end(s_dots, K, dots);
}
template <bool CPLX, int INDEX>
static int launch_direct_cheb(lsk_operator const &op, lsk_index ix, int weight, lsk_tilemap tm, uint64_t const *reps, int K, void const *x, int64_t xr,
                              int64_t xc, void *y, int64_t yr, int64_t yc, double alpha, double beta, double gamma, double *dots, int *d_err,
                              hipStream_t s) {
    int64_t gb = tm.slots_per_xcd * 8;
    int64_t cap = resident_grid(k_direct_cheb<CPLX, INDEX>, gb) & ~(int64_t)7; // persistent, a multiple of 8 (XCD dealing)
    if (cap < 8) cap = 8;
    if (gb > cap) gb = cap;
    hipLaunchKernelGGL((k_direct_cheb<CPLX, INDEX>), dim3((unsigned)gb), dim3(kBlock), 0, s, op.runs, op.n_groups, op.groups, op.off, op.n_diag,
                       op.diag, ix, weight, tm.entries, tm.slots_per_xcd, reps, K, (double const *)x, xr, xc, (double *)y, yr, yc, alpha, beta,
                       gamma, dots, d_err);
    LSK_LAUNCH_CHECK();
    return 0;
}
extern "C" int lsk_direct_cheb(lsk_operator op, lsk_basis bs, lsk_index ix, int cplx, lsk_tilemap tm, uint64_t const *reps, int K,
                               void const *x, int64_t xr, int64_t xc, void *y, int64_t yr, int64_t yc, double alpha, double beta,
                               double gamma, double *d_dots, int *d_err, void *stream) {
    if (tm.slots_per_xcd == 0 || K <= 0) return 0;
    if (K > kChebMaxCols) { snprintf(g_err, sizeof(g_err), "lsk_direct_cheb: at most %d columns", kChebMaxCols); return -1; }
    if (!tm.entries) { snprintf(g_err, sizeof(g_err), "lsk_direct_cheb: no tile map"); return -1; }
    if (bs.proj != LSK_PROJ_NONE) { snprintf(g_err, sizeof(g_err), "lsk_direct_cheb: unprojected bases only"); return -1; }
    if (!cplx && !op.is_real) { snprintf(g_err, sizeof(g_err), "lsk_direct_cheb: complex operators need c128 vectors"); return -1; }
    hipStream_t s = (hipStream_t)stream;
#define LSK_DC(IDX) (cplx ? launch_direct_cheb<true, IDX>(op, ix, bs.hamming_weight, tm, reps, K, x, xr, xc, y, yr, yc, alpha, beta, gamma, d_dots, d_err, s) \
                          : launch_direct_cheb<false, IDX>(op, ix, bs.hamming_weight, tm, reps, K, x, xr, xc, y, yr, yc, alpha, beta, gamma, d_dots, d_err, s))
    switch (ix.kind) {
    case LSK_INDEX_IDENTITY: return LSK_DC(LSK_INDEX_IDENTITY);
    case LSK_INDEX_COMBINADIC: return LSK_DC(LSK_INDEX_COMBINADIC);
    case LSK_INDEX_PRODUCT: return LSK_DC(LSK_INDEX_PRODUCT);
    default: return LSK_DC(LSK_INDEX_SEARCH);
    }
#undef LSK_DC
}

// the packet gather of k_pull_gather_blk (one wave per 64 rows, LDS accumulators [column][row], K4-prescaling norms and the
// diagonal fused), with the update in place of the store.
template <bool CPLX>
__global__ __launch_bounds__(kBlock) void k_pull_gather_cheb(lsk_runs runs, int n_diag, lsk_term const *__restrict__ diag, int k4_mode,
                                                             int coef, int64_t row0, int64_t row1, uint64_t const *__restrict__ reps,
                                                             double const *__restrict__ norms, double uni_v, lsk_pullbuf buf, int K,
                                                             double const *__restrict__ x, int64_t xr, int64_t xc, double *__restrict__ y,
                                                             int64_t yr, int64_t yc, double alpha, double beta_, double gamma,
                                                             double *__restrict__ dots, int xcd_chunk) {
    typedef typename ChainX<CPLX>::type X;
    constexpr int KB = ChebCols<CPLX>::KB;
    constexpr int GU = 2;
    X const *__restrict__ xv = (X const *)x;
    X *__restrict__ yv = (X *)y;
    __shared__ X s_acc[KB * kBlock];
    __shared__ double s_dots[2 * kChebMaxCols];
    cheb_dots_begin(s_dots, K);
    BlkCheb<X> ep;
    ep.init(alpha, beta_, gamma, s_dots, K, dots != nullptr);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int64_t n_tiles = (row1 - row0 + kBlock - 1) / kBlock;
    for (int64_t tb = blockIdx.x; tb < n_tiles; tb += gridDim.x) {
        const int64_t t0 = row0 + pull_tile_of_block(tb, n_tiles, gridDim.x >= n_tiles ? xcd_chunk : 0) * kBlock;
        if ((t0 + (wave << 6)) >= row1) continue; // wave-uniform
        const int64_t i = t0 + tid;
        const bool valid = i < row1;
        const int64_t wg = ((t0 - buf.row0) >> 6) + wave;
        const int64_t sbase = buf.offs ? buf.offs[wg] : wg * buf.cap;
        const int n = (int)buf.counts[wg];
        double inv_na = 0.0, dr = 0.0, di = 0.0;
        if (valid) {
            const double na = norms[i];
            inv_na = na > 0.0 ? 1.0 / na : 0.0;
            if (n_diag > 0) diag_coeff<uint64_t, !CPLX>(runs, n_diag, diag, reps[i], dr, di);
        }
        const double sc = coef == COEF_UNI ? uni_v * inv_na : 1.0;
        for (int c0 = 0; c0 < K; c0 += KB) {
            const int kb = min(KB, K - c0); // wave-uniform
#pragma unroll
            for (int k = 0; k < KB; ++k) s_acc[k * kBlock + tid] = cx_zero<X>();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int c = 0; c < n; c += 64 * GU) {
                uint32_t slot[GU];
                int r[GU];
                double hr[GU], hi[GU], nb[GU];
#pragma unroll
                for (int u = 0; u < GU; ++u) {
                    const int p = c + 64 * u + lane;
                    slot[u] = kNoSlot; r[u] = 0; hr[u] = 1.0; hi[u] = 0.0; nb[u] = 1.0;
                    if (p < n) {
                        const int64_t o = sbase + p;
                        slot[u] = buf.slots[o];
                        r[u] = (int)buf.rows[o];
                        if (coef == COEF_REAL) hr[u] = buf.coefs[o];
                        else if (coef == COEF_CPLX) { hr[u] = buf.coefs[2 * o]; hi[u] = buf.coefs[2 * o + 1]; }
                    }
                    if (slot[u] != kNoSlot && k4_mode != 0) nb[u] = norms[slot[u]];
                }
                X v[GU][KB];
#pragma unroll
                for (int u = 0; u < GU; ++u) {
                    X const *__restrict__ xp = xv + (int64_t)(slot[u] != kNoSlot ? slot[u] : 0) * xr + (int64_t)c0 * xc;
#pragma unroll
                    for (int k = 0; k < KB; ++k) v[u][k] = (slot[u] != kNoSlot && k < kb) ? xp[(int64_t)k * xc] : cx_zero<X>();
                }
#pragma unroll
                for (int u = 0; u < GU; ++u) {
                    if (slot[u] == kNoSlot) continue;
                    const int ra = (wave << 6) + r[u];
                    const double cr = hr[u] * nb[u], ci = hi[u] * nb[u];
#pragma unroll
                    for (int k = 0; k < KB; ++k) {
                        if (k >= kb) continue;
                        double *const acc = (double *)&s_acc[k * kBlock + ra];
                        if constexpr (CPLX) {
                            atomicAdd(acc, cr * v[u][k].x - ci * v[u][k].y);
                            atomicAdd(acc + 1, cr * v[u][k].y + ci * v[u][k].x);
                        } else atomicAdd(acc, cr * v[u][k]);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                if (k >= kb) continue;
                double sxx = 0.0, sxy = 0.0;
                if (valid) {
                    const X xo = xv[i * xr + (int64_t)(c0 + k) * xc];
                    const X s = s_acc[k * kBlock + tid];
                    X h;
                    if constexpr (CPLX) h = make_double2(dr * xo.x - di * xo.y + sc * s.x, dr * xo.y + di * xo.x + sc * s.y);
                    else h = dr * xo + sc * s;
                    ep.update(xo, yv + (i * yr + (int64_t)(c0 + k) * yc), h, sxx, sxy);
                }
                ep.reduce(c0 + k, true, sxx, sxy); // (the whole wave is here: lanes past row1 carry zeros)
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // this wave's accumulators are free again
            __builtin_amdgcn_wave_barrier();
        }
    }
    cheb_dots_end(s_dots, K, dots);
}
extern "C" int lsk_pull_gather_cheb(lsk_operator op, lsk_basis bs, int cplx, int64_t row0, int64_t row1, uint64_t const *reps,
                                    double const *norms, lsk_pullbuf buf, int K, void const *x, int64_t xr, int64_t xc, void *y,
                                    int64_t yr, int64_t yc, double alpha, double beta, double gamma, double *d_dots, void *stream) {
    if (row1 <= row0 || K <= 0) return 0;
    if (K > kChebMaxCols) { snprintf(g_err, sizeof(g_err), "lsk_pull_gather_cheb: at most %d columns", kChebMaxCols); return -1; }
    int k4m, coef;
    pull_kinds(op, bs, k4m, coef);
    if (coef == COEF_CPLX && !cplx) { snprintf(g_err, sizeof(g_err), "lsk_pull_gather_cheb: complex coefficients need c128 vectors"); return -1; }
    const int64_t work_blocks = (row1 - row0 + kBlock - 1) / kBlock;
    hipStream_t s = (hipStream_t)stream;
    if (cplx)
        hipLaunchKernelGGL(k_pull_gather_cheb<true>, dim3((unsigned)tile_grid(k_pull_gather_cheb<true>, work_blocks)), dim3(kBlock), 0, s, op.runs,
                           op.n_diag, op.diag, bs.k4_mode, coef, row0, row1, reps, norms, op.uni_v, buf, K, (double const *)x, xr, xc,
                           (double *)y, yr, yc, alpha, beta, gamma, d_dots, pull_xcd_chunk());
    else
        hipLaunchKernelGGL(k_pull_gather_cheb<false>, dim3((unsigned)tile_grid(k_pull_gather_cheb<false>, work_blocks)), dim3(kBlock), 0, s, op.runs,
                           op.n_diag, op.diag, bs.k4_mode, coef, row0, row1, reps, norms, op.uni_v, buf, K, (double const *)x, xr, xc,
                           (double *)y, yr, yc, alpha, beta, gamma, d_dots, pull_xcd_chunk());
    LSK_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Epilogue pass (k_axpby_dots): Y <- alpha W + beta X + gamma Y and the two dots, K columns of n rows.  All strides are in
// DOUBLES here (the launcher doubles those of c128).  Streaming and grid-strided; a thread moves 16 bytes per array and step where
// the layout allows (TWO): one c128 element; or, for f64, VEC = two columns of a row (column stride 1, K even) or two rows of a
// column (row stride 1), everything 16-byte aligned.  COLS = false: a thread keeps ONE column (pair) and walks rows -- consecutive
// threads take consecutive columns of a row, then the next row: the order of an interleaved block.  COLS = true: column after
// column, consecutive threads on consecutive rows.  Reduction: __shfl_xor across the lanes that hold the same column, then LDS,
// then one f64 atomic per workgroup and output (as k_orth_pass).
// ---------------------------------------------------------------------------------------------
constexpr int kAxBlock = 256;
template <bool TWO>
__device__ __forceinline__ void ax_update(double const *__restrict__ wp, double const *__restrict__ xp, double *__restrict__ yp, double alpha,
                                          double beta, double gamma, double2 &xo, double2 &yn) {
    if constexpr (TWO) {
        const double2 wv = *reinterpret_cast<double2 const *>(wp);
        xo = *reinterpret_cast<double2 const *>(xp);
        yn = make_double2(alpha * wv.x + beta * xo.x, alpha * wv.y + beta * xo.y);
        if (gamma != 0.0) {
            const double2 yo = *reinterpret_cast<double2 const *>(yp);
            yn.x += gamma * yo.x;
            yn.y += gamma * yo.y;
        }
        *reinterpret_cast<double2 *>(yp) = yn;
    } else {
        xo = make_double2(*xp, 0.0);
        yn = make_double2(alpha * *wp + beta * xo.x, 0.0);
        if (gamma != 0.0) yn.x += gamma * *yp;
        *yp = yn.x;
    }
}
template <bool CPLX, bool VEC, bool COLS>
__global__ __launch_bounds__(kAxBlock) void k_axpby_dots(int64_t n, int K, double const *__restrict__ w, int64_t wr, int64_t wc,
                                                         double const *__restrict__ x, int64_t xr, int64_t xc, double *__restrict__ y, int64_t yr,
                                                         int64_t yc, double alpha, double beta, double gamma, double *__restrict__ d_xx,
                                                         double *__restrict__ d_xy) {
    constexpr bool TWO = CPLX || VEC;
    __shared__ double s_dots[2 * kChebMaxCols];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 2 * kChebMaxCols) s_dots[tid] = 0.0;
    __syncthreads();
    double2 xo, yn;
    if constexpr (!COLS) {
        const int CG = VEC ? K >> 1 : K; // column groups: <= 64
        const int rpb = kAxBlock / CG;   // rows of a workgroup per step; threads past rpb * CG idle
        const int cg = tid % CG, r = tid / CG;
        const int64_t kcol = VEC ? 2 * cg : cg;
        double a0 = 0.0, b0 = 0.0, a1 = 0.0, b1 = 0.0;
        if (r < rpb)
            for (int64_t i = (int64_t)blockIdx.x * rpb + r; i < n; i += (int64_t)gridDim.x * rpb) {
                ax_update<TWO>(w + i * wr + kcol * wc, x + i * xr + kcol * xc, y + i * yr + kcol * yc, alpha, beta, gamma, xo, yn);
                if constexpr (VEC) { a0 += xo.x * xo.x; b0 += xo.x * yn.x; a1 += xo.y * xo.y; b1 += xo.y * yn.y; }
                else { a0 += xo.x * xo.x + xo.y * xo.y; b0 += xo.x * yn.x + xo.y * yn.y; }
            }
        const int c0 = (int)kcol;
        if (64 % CG == 0) { // (workgroup-uniform) lanes l, l + CG, ... hold the same column and every thread has rows
            for (int d = 32; d >= CG; d >>= 1) {
                a0 += __shfl_xor(a0, d); b0 += __shfl_xor(b0, d);
                if constexpr (VEC) { a1 += __shfl_xor(a1, d); b1 += __shfl_xor(b1, d); }
            }
            if (lane < CG) {
                atomicAdd(s_dots + c0, a0); atomicAdd(s_dots + kChebMaxCols + c0, b0);
                if constexpr (VEC) { atomicAdd(s_dots + c0 + 1, a1); atomicAdd(s_dots + kChebMaxCols + c0 + 1, b1); }
            }
        } else if (r < rpb) {
            atomicAdd(s_dots + c0, a0); atomicAdd(s_dots + kChebMaxCols + c0, b0);
            if constexpr (VEC) { atomicAdd(s_dots + c0 + 1, a1); atomicAdd(s_dots + kChebMaxCols + c0 + 1, b1); }
        }
    } else {
        const int64_t units = VEC ? n >> 1 : n;
        for (int k = 0; k < K; ++k) {
            double a = 0.0, b = 0.0;
            for (int64_t p = (int64_t)blockIdx.x * kAxBlock + tid; p < units; p += (int64_t)gridDim.x * kAxBlock) {
                const int64_t i = VEC ? 2 * p : p;
                ax_update<TWO>(w + i * wr + k * wc, x + i * xr + k * xc, y + i * yr + k * yc, alpha, beta, gamma, xo, yn);
                a += xo.x * xo.x + xo.y * xo.y;
                b += xo.x * yn.x + xo.y * yn.y;
            }
            if (VEC && (n & 1) && blockIdx.x == 0 && tid == 0) { // the odd last row
                const int64_t i = n - 1;
                ax_update<false>(w + i * wr + k * wc, x + i * xr + k * xc, y + i * yr + k * yc, alpha, beta, gamma, xo, yn);
                a += xo.x * xo.x;
                b += xo.x * yn.x;
            }
            for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); }
            if (lane == 0) { atomicAdd(s_dots + k, a); atomicAdd(s_dots + kChebMaxCols + k, b); }
        }
    }
    __syncthreads();
    if (tid < K) {
        if (d_xx) unsafeAtomicAdd(d_xx + tid, s_dots[tid]);
        if (d_xy) unsafeAtomicAdd(d_xy + tid, s_dots[kChebMaxCols + tid]);
    }
}
// strides in ELEMENTS (doubles, or double pairs for c128); d_xx / d_xy: K doubles each (or NULL), added to
extern "C" int lsk_axpby_dots(int cplx, int64_t n, int K, void const *w, int64_t wr, int64_t wc, void const *x, int64_t xr, int64_t xc,
                              void *y, int64_t yr, int64_t yc, double alpha, double beta, double gamma, double *d_xx, double *d_xy,
                              void *stream) {
    if (n <= 0 || K <= 0) return 0;
    if (K > kChebMaxCols) { snprintf(g_err, sizeof(g_err), "lsk_axpby_dots: at most %d columns", kChebMaxCols); return -1; }
    if (K == 1) { wc = 0; xc = 0; yc = 0; }
    if (cplx) { wr *= 2; wc *= 2; xr *= 2; xc *= 2; yr *= 2; yc *= 2; }
    const bool cols = K == 1 || xr < xc;
    const bool al = ((uintptr_t)w % 16 == 0) && ((uintptr_t)x % 16 == 0) && ((uintptr_t)y % 16 == 0);
    bool vec = false;
    if (!cplx && al) {
        if (cols) vec = wr == 1 && xr == 1 && yr == 1 && wc % 2 == 0 && xc % 2 == 0 && yc % 2 == 0 && n >= 2;
        else vec = wc == 1 && xc == 1 && yc == 1 && K % 2 == 0 && wr % 2 == 0 && xr % 2 == 0 && yr % 2 == 0;
    }
    int64_t work; // threads that have something to do
    if (cols) work = vec ? n >> 1 : n;
    else { const int cg = vec ? K >> 1 : K; work = (n + kAxBlock / cg - 1) / (kAxBlock / cg) * kAxBlock; }
    int64_t blocks = (work + kAxBlock - 1) / kAxBlock;
    if (blocks < 1) blocks = 1;
    if (blocks > kMaxGrid) blocks = kMaxGrid; // 8 workgroups per CU, grid-stride: few atomics, long streams
    hipStream_t s = (hipStream_t)stream;
    dim3 g((unsigned)blocks), b(kAxBlock);
#define LSK_AX(C, V, CO) hipLaunchKernelGGL((k_axpby_dots<C, V, CO>), g, b, 0, s, n, K, (double const *)w, wr, wc, (double const *)x, xr, xc, \
                                            (double *)y, yr, yc, alpha, beta, gamma, d_xx, d_xy)
    if (cplx) { if (cols) LSK_AX(true, false, true); else LSK_AX(true, false, false); }
    else if (vec) { if (cols) LSK_AX(false, true, true); else LSK_AX(false, true, false); }
    else { if (cols) LSK_AX(false, false, true); else LSK_AX(false, false, false); }
#undef LSK_AX
    LSK_LAUNCH_CHECK();
    return 0;
}
