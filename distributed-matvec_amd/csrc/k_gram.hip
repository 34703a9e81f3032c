// k_gram.hip -- the Gram matrices of blocks of vectors (ls_amd_block_gram, ls_amd_matvec_block_axpby_gram, host.c; DESIGN.md
// section 5, "Matrix moments"): G[a][b] = sum_r conj(A[r][a]) B[r][b] for a bra block A (n x Ka) and one or two ket blocks B1, B2
// (n x Kb), f64 or c128, Ka, Kb <= 64.  The matrix-valued Chebyshev moments are two of them per step (X^+ X and X^+ Y).
//
//   k_block_gram_mfma   blocks with column stride 1 and row stride K (the interleaved layout of the block kernels).  A c128 block is
//                       a real n x 2K array, an f64 block n x K; it is cut into chunks of 16 real columns.  v_mfma_f64_16x16x4_f64
//                       takes 4 rows per instruction: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], which
//                       for a chunk is the double at (row0 + (l >> 4)) * width + 16 chunk + (l & 15) -- the memory layout IS the
//                       operand layout (one coalesced 512-byte wave load per operand when the width is 16): no LDS staging, no
//                       shuffles.  Result register r of lane l is D[(l >> 4) + 4 r][l & 15] (the f64 map, not the f32 one).
//                       Columns past the width and rows past n enter as zeros and are never read.  A job (blockIdx.y) is one bra
//                       chunk and up to kGramTiles = 8 ket chunks: the wave holds the bra operand and streams the kets, 8 tiles of
//                       4 f64 per lane = 64 accumulator registers.  The operands of the next 2 to 4 row groups are loaded before
//                       the MFMAs of the current ones are issued (70 / 99 / 103 / 189 VGPRs with 1 / 2 / 4 / 8 tiles: the widest
//                       form runs 2 waves per SIMD, where the product is compute-bound anyway).  A ket chunk that is the bra chunk
//                       (X^+ X) reuses the bra register.
//                       Complex entries are folded from the real tile when the workgroup writes its partial:
//                       G[a][b] = (R[2a][2b] + R[2a+1][2b+1]) + i (R[2a][2b+1] - R[2a+1][2b]).
//   k_block_gram        any strides, on the vector ALU: a thread owns a 4 x 4 tile of outputs and every 64th row of its wave's
//                       range; the lanes are summed by a butterfly.  The fallback, and the in-library check of the form above.
//
// The reduction is the same in both: the 4-row groups of n are dealt to (workgroup, wave) in contiguous ranges by gram_range(), a
// fixed function of n and the launch; the waves of a workgroup are summed in LDS in wave order; a workgroup writes one partial; the
// partials are added in block order by lsk_corr_sum (k_corr.hip).  No floating-point atomics: two calls return equal bytes.
#include "lsk_dev.hpp"

constexpr int kGramBlock = 512;                 // 8 waves
constexpr int kGramWaves = kGramBlock / 64;
constexpr int kGramTiles = 8;                   // accumulator tiles of a wave of k_block_gram_mfma
constexpr int kGramMaxBlocks = 512;             // workgroups of a launch over all jobs of the MFMA form (two per CU)
constexpr int kGramVT = 4;                      // k_block_gram: outputs per thread, kGramVT x kGramVT

typedef double gram_d4 __attribute__((ext_vector_type(4)));

// one block of vectors: element (r, k) at base + (r * row + k * col) * (CPLX ? 2 : 1) doubles
struct gram_blk { double const *p; int64_t row, col; };

// the 4-row groups [g0, g1) of this wave: contiguous, ascending in (workgroup, wave)
__device__ __forceinline__ void gram_range(int64_t n, int wave, int64_t &g0, int64_t &g1) {
    const int64_t groups = (n + 3) >> 2;
    const int64_t per = (groups + (int64_t)gridDim.x * kGramWaves - 1) / ((int64_t)gridDim.x * kGramWaves);
    const int64_t idx = (int64_t)blockIdx.x * kGramWaves + wave;
    g0 = idx * per < groups ? idx * per : groups;
    g1 = g0 + per < groups ? g0 + per : groups;
}

// NT: accumulator tiles kept (1, 2, 4, 8); U: row groups whose loads are issued before their MFMAs
template <bool CPLX, int NT, int U>
__global__ __launch_bounds__(kGramBlock) void k_block_gram_mfma(int64_t n, int Ka, int Kb, int nket, double const *__restrict__ A,
                                                                double const *__restrict__ B1, double const *__restrict__ B2,
                                                                int same0, double *__restrict__ partial) {
    __shared__ double s_w[kGramWaves][256]; // a tile of every wave, [row][column] of D
    __shared__ double s_r[256];             // their sum
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lo = lane & 15, hi = lane >> 4;
    constexpr int E = CPLX ? 2 : 1;
    const int Wa = Ka * E, Wb = Kb * E;                 // real widths
    const int CB = (Wb + 15) >> 4;                      // ket chunks per ket block
    const int tiles = nket * CB;                        // ket tiles in all: tile t = ket (t / CB), chunk (t % CB)
    const int groups_of_tiles = (tiles + NT - 1) / NT;
    const int ca = blockIdx.y / groups_of_tiles;        // the job: bra chunk ca, ket tiles [t0, t0 + NT)
    const int t0 = (blockIdx.y % groups_of_tiles) * NT;

    const int col_a = 16 * ca + lo;
    const bool in_a = col_a < Wa;
    double const *pb[NT];
    bool in_b[NT], same[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int tt = t0 + t < tiles ? t0 + t : tiles - 1; // (a tile past the end repeats the last one and is not written)
        const int ket = tt / CB, cb = tt % CB;
        pb[t] = (ket == 0 ? B1 : B2) + 16 * cb + lo;
        in_b[t] = 16 * cb + lo < Wb;
        same[t] = same0 && ket == 0 && cb == ca;
    }

    gram_d4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = gram_d4{0.0, 0.0, 0.0, 0.0};

    int64_t g0, g1;
    gram_range(n, wave, g0, g1);
    // the operands of U row groups from g on; the next batch is loaded before the MFMAs of this one are issued
    auto load = [&](int64_t g, double (&a)[U], double (&b)[NT][U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = 4 * (g + u) + hi;
            const bool ok = g + u < g1 && row < n;
            a[u] = ok && in_a ? A[row * Wa + col_a] : 0.0;
#pragma unroll
            for (int t = 0; t < NT; ++t) b[t][u] = same[t] ? a[u] : (ok && in_b[t] ? pb[t][row * Wb] : 0.0);
        }
    };
    double a[U], b[NT][U], an[U], bn[NT][U];
    if (g0 < g1) load(g0, a, b);
    for (int64_t g = g0; g < g1; g += U) {
        load(g + U, an, bn); // (past g1: zeros, nothing is read)
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[t][u], acc[t], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            a[u] = an[u];
#pragma unroll
            for (int t = 0; t < NT; ++t) b[t][u] = bn[t][u];
        }
    }

    // tile by tile: the waves' tiles summed in wave order, folded, written to this workgroup's partial
    const int64_t m = (int64_t)nket * Ka * Kb * E;
    double *const out = partial + (int64_t)blockIdx.x * m;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t0 + t >= tiles) break;
        const int ket = (t0 + t) / CB, cb = (t0 + t) % CB;
#pragma unroll
        for (int r = 0; r < 4; ++r) s_w[wave][(hi + 4 * r) * 16 + lo] = acc[t][r];
        __syncthreads();
        if (threadIdx.x < 256) {
            double s = s_w[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < kGramWaves; ++w) s += s_w[w][threadIdx.x];
            s_r[threadIdx.x] = s;
        }
        __syncthreads();
        if (CPLX) {
            if (threadIdx.x < 128) {
                const int e = threadIdx.x >> 1, im = threadIdx.x & 1;
                const int al = e >> 3, bl = e & 7, ga = 8 * ca + al, gb = 8 * cb + bl;
                if (ga < Ka && gb < Kb) {
                    const double v = im ? s_r[(2 * al) * 16 + 2 * bl + 1] - s_r[(2 * al + 1) * 16 + 2 * bl]
                                        : s_r[(2 * al) * 16 + 2 * bl] + s_r[(2 * al + 1) * 16 + 2 * bl + 1];
                    out[(((int64_t)ket * Ka + ga) * Kb + gb) * 2 + im] = v;
                }
            }
        } else if (threadIdx.x < 256) {
            const int ga = 16 * ca + (threadIdx.x >> 4), gb = 16 * cb + (threadIdx.x & 15);
            if (ga < Ka && gb < Kb) out[((int64_t)ket * Ka + ga) * Kb + gb] = s_r[threadIdx.x];
        }
        // (the next tile's writes of s_w follow the second barrier, behind every read of it; those of s_r follow its first one)
    }
}

// a job (blockIdx.y) is one ket block and one kGramVT x kGramVT tile of its Ka x Kb outputs
template <bool CPLX>
__global__ __launch_bounds__(kGramBlock) void k_block_gram(int64_t n, int Ka, int Kb, gram_blk A, gram_blk B1, gram_blk B2,
                                                           double *__restrict__ partial) {
    constexpr int E = CPLX ? 2 : 1, V = kGramVT, NV = V * V * E;
    __shared__ double s_w[kGramWaves][NV];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int TA = (Ka + V - 1) / V, TB = (Kb + V - 1) / V;
    const int ket = blockIdx.y / (TA * TB), ta = (blockIdx.y / TB) % TA, tb = blockIdx.y % TB;
    const gram_blk B = ket == 0 ? B1 : B2;

    double acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0;

    int64_t g0, g1;
    gram_range(n, wave, g0, g1);
    const int64_t r1 = 4 * g1 < n ? 4 * g1 : n;
    for (int64_t r = 4 * g0 + lane; r < r1; r += 64) {
        double a[V][E], b[V][E];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int ka = V * ta + i, kb = V * tb + i;
#pragma unroll
            for (int c = 0; c < E; ++c) {
                a[i][c] = ka < Ka ? A.p[(r * A.row + ka * A.col) * E + c] : 0.0;
                b[i][c] = kb < Kb ? B.p[(r * B.row + kb * B.col) * E + c] : 0.0;
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (CPLX) { // conj(a) b
                    acc[(i * V + j) * 2] += a[i][0] * b[j][0] + a[i][E - 1] * b[j][E - 1];
                    acc[(i * V + j) * 2 + 1] += a[i][0] * b[j][E - 1] - a[i][E - 1] * b[j][0];
                } else {
                    acc[i * V + j] += a[i][0] * b[j][0];
                }
            }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double v = acc[i];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if (lane == 0) s_w[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = s_w[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kGramWaves; ++w) s += s_w[w][threadIdx.x];
        const int e = threadIdx.x / E, c = threadIdx.x % E;
        const int ga = V * ta + e / V, gb = V * tb + e % V;
        const int64_t m = (int64_t)gridDim.y / (TA * TB) * Ka * Kb * E; // (gridDim.y = nket TA TB)
        if (ga < Ka && gb < Kb) partial[(int64_t)blockIdx.x * m + (((int64_t)ket * Ka + ga) * Kb + gb) * E + c] = s;
    }
}

extern "C" char const *lsk_block_gram_kernel_name(int mfma) { return mfma ? "k_block_gram_mfma" : "k_block_gram"; }

// workgroups (= partials) of a launch over n rows: at least 256 rows each, and with the jobs of the MFMA form -- one per chunk
// of 16 real bra columns -- about two workgroups per CU in all, so that the whole grid is resident (measured: a grid of 1024
// workgroups of 99 VGPRs ran 1.5 x slower than one of 512)
extern "C" int lsk_block_gram_blocks(int64_t n, int Ka, int Kb, int cplx) {
    const int64_t want = (n + 255) / 256;
    const int cap = kGramMaxBlocks / ((Ka * (cplx ? 2 : 1) + 15) / 16);
    return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

template <bool CPLX>
static int gram_mfma_launch(int64_t n, int Ka, int Kb, int nket, double const *A, double const *B1, double const *B2, int same0,
                            int blocks, double *partial, hipStream_t s) {
    const int E = CPLX ? 2 : 1;
    const int CA = (Ka * E + 15) / 16, tiles = nket * ((Kb * E + 15) / 16);
    const int nt = tiles >= kGramTiles ? kGramTiles : (tiles > 2 ? 4 : tiles);
    const dim3 grid(blocks, CA * ((tiles + nt - 1) / nt)), block(kGramBlock);
    switch (nt) {
    case 1: hipLaunchKernelGGL((k_block_gram_mfma<CPLX, 1, 4>), grid, block, 0, s, n, Ka, Kb, nket, A, B1, B2, same0, partial); break;
    case 2: hipLaunchKernelGGL((k_block_gram_mfma<CPLX, 2, 4>), grid, block, 0, s, n, Ka, Kb, nket, A, B1, B2, same0, partial); break;
    case 4: hipLaunchKernelGGL((k_block_gram_mfma<CPLX, 4, 2>), grid, block, 0, s, n, Ka, Kb, nket, A, B1, B2, same0, partial); break;
    default: hipLaunchKernelGGL((k_block_gram_mfma<CPLX, kGramTiles, 2>), grid, block, 0, s, n, Ka, Kb, nket, A, B1, B2, same0, partial); break;
    }
    LSK_LAUNCH_CHECK();
    return 0;
}

// out[(ket Ka + a) Kb + b] = sum_r conj(A[r][a]) B_ket[r][b], ket < nket (1 or 2; b2 is not read when nket == 1), ASSIGNED, in
// elements of the vector type.  Strides in elements.  mfma != 0: k_block_gram_mfma -- the caller has checked that every block has
// column stride 1 (or one column) and row stride equal to its width.  partial: lsk_block_gram_blocks(n, Ka, Kb, cplx) x nket Ka Kb elements.
extern "C" int lsk_block_gram(int cplx, int64_t n, int Ka, void const *a, int64_t a_row, int64_t a_col, int Kb, int nket, void const *b1,
                              int64_t b1_row, int64_t b1_col, void const *b2, int64_t b2_row, int64_t b2_col, int mfma, double *partial,
                              double *out, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const int E = cplx ? 2 : 1;
    const int64_t m = (int64_t)nket * Ka * Kb * E;
    if (n <= 0) {
        LSK_CHECK(hipMemsetAsync(out, 0, sizeof(double) * (size_t)m, s));
        return 0;
    }
    const int blocks = lsk_block_gram_blocks(n, Ka, Kb, cplx);
    double const *A = (double const *)a, *B1 = (double const *)b1, *B2 = (double const *)(nket > 1 ? b2 : b1);
    if (mfma) {
        const int same0 = a == b1 && Ka == Kb;
        if (cplx) { if (gram_mfma_launch<true>(n, Ka, Kb, nket, A, B1, B2, same0, blocks, partial, s) != 0) return -1; }
        else if (gram_mfma_launch<false>(n, Ka, Kb, nket, A, B1, B2, same0, blocks, partial, s) != 0) return -1;
    } else {
        const gram_blk ga = { A, a_row, a_col }, gb1 = { B1, b1_row, b1_col }, gb2 = { B2, nket > 1 ? b2_row : b1_row, nket > 1 ? b2_col : b1_col };
        const int TA = (Ka + kGramVT - 1) / kGramVT, TB = (Kb + kGramVT - 1) / kGramVT;
        const dim3 grid(blocks, nket * TA * TB), block(kGramBlock);
        if (cplx) hipLaunchKernelGGL(k_block_gram<true>, grid, block, 0, s, n, Ka, Kb, ga, gb1, gb2, partial);
        else hipLaunchKernelGGL(k_block_gram<false>, grid, block, 0, s, n, Ka, Kb, ga, gb1, gb2, partial);
        LSK_LAUNCH_CHECK();
    }
    return lsk_corr_sum(blocks, (int)m, partial, out, stream);
}
