// orth_block.hip -- the vector algebra of a BLOCK eigensolver (block Lanczos, diagonalize.py: lanczos_block_smallest): classical
// Gram-Schmidt of K new vectors against a basis of m vectors, and the in-place rotation of the thick restart and of the
// Cholesky-QR normalisation.  orth.hip sweeps the basis once per new vector; a block of K would read it K times.  Here one launch
// reads V once and W once (plus W's write-back when updating), whatever K is.
//
// ls_amd_orth_block_pass(m, K, n, V, ldv, W, ldw, H_in, out):
//     if H_in:  W_c <- W_c - sum_k H_in[k][c] V_k              (H_in: m x K, row-major)
//     out[k*K + c]           = <V_k, W_c>   over the UPDATED W  (k < m, c < K)
//     out[m*K + c*K + c']    = <W_c, W_c'>                       (the Gram matrix of the updated W)
// Both products are split-K tall-skinny GEMMs over n.  Every workgroup walks ONE contiguous range of n (a grid-stride loop cost
// k_orth_pass 3.9 against 5.4 TB/s) in tiles of 16 columns: the tile of V (m x 16) and of W (K x 16) is staged in LDS (the next
// tile's global loads are in flight in registers meanwhile), and the products run on the f64 MFMA 16x16x4 -- the update as
// (K x m) . (m x 16) split over the waves by k-steps and reduced in LDS in a fixed order, the overlaps as (16-row tile of V) . W^T
// with the 16-row tiles (and the Gram tile W . W^T) owned by the waves.  An output is owned by one lane of one wave of a
// workgroup: one atomic per workgroup and output, no shuffles.
//
// ls_amd_block_rotate(m_in, m_out, n, V, ldv, S): V[:m_out] <- S^T V[:m_in] in place (S: m_in x m_out, row-major) -- the thick
// restart (S = kept Ritz coefficients) and W <- W R^-1 (m_in = m_out = K).  The tile of V[:m_in] is in LDS before any of its
// columns is written back, so m_in rows are read once and m_out rows written once, with no temporary in HBM.
//
// f64 MFMA operand maps (gfx950, v_mfma_f64_16x16x4_f64): lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register r
// of lane l is D[(l >> 4) + 4 r][l & 15].
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int kObBlock = 256;    // 4 waves
constexpr int kObMaxRows = 128;  // m, m_in
constexpr int kObMaxCols = 16;   // K
constexpr int kObTile = 16;      // columns per tile
constexpr int kObLd = kObTile + 1; // LDS row stride in doubles (spreads the column reads of the MFMA A operand over the banks)

typedef double ob_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ ob_d4 ob_mfma(double a, double b, ob_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// One tile (rows [0, rows) x columns [i0, i0 + 16) of a row-strided array, clipped at column i1) in registers: thread t owns the
// column pair 2 (t & 7) of rows (t >> 3) + 32 q.  Pairs are 16-byte loads when ALIGNED and both columns are in range.
template <bool ALIGNED, int Q>
struct ObStage {
    double2 v[Q];
    __device__ __forceinline__ void load(double const *__restrict__ A, int64_t ld, int rows, int64_t i0, int64_t i1) {
        const int r0 = threadIdx.x >> 3;
        const int64_t i = i0 + 2 * (threadIdx.x & 7);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int r = r0 + 32 * q;
            double2 x = make_double2(0.0, 0.0);
            if (r < rows) {
                double const *p = A + (int64_t)r * ld + i;
                if (ALIGNED && i + 1 < i1) x = *reinterpret_cast<double2 const *>(p);
                else {
                    if (i < i1) x.x = p[0];
                    if (i + 1 < i1) x.y = p[1];
                }
            }
            v[q] = x;
        }
    }
    __device__ __forceinline__ void store(double (*s)[kObLd], int rows) const {
        const int r0 = threadIdx.x >> 3, j = 2 * (threadIdx.x & 7);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int r = r0 + 32 * q;
            if (r < rows) { s[r][j] = v[q].x; s[r][j + 1] = v[q].y; }
        }
    }
};

template <bool UPDATE, bool ALIGNED>
__global__ __launch_bounds__(kObBlock) void k_orth_block_pass(int m, int K, int64_t n, double const *__restrict__ V, int64_t ldv,
                                                              double *__restrict__ W, int64_t ldw, double const *__restrict__ H,
                                                              double *__restrict__ out) {
    __shared__ double s_V[kObMaxRows][kObLd];
    __shared__ double s_W[kObMaxCols][kObLd];
    __shared__ double s_U[UPDATE ? 4 : 1][kObMaxCols][kObTile]; // the waves' partial V.H of a tile, summed in wave order
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lo = lane & 15, hi = lane >> 4;
    const int steps = (m + 3) >> 2;            // k-steps of the update (4 rows of V each)
    const int vtiles = (m + 15) >> 4;          // 16-row tiles of V; tile `vtiles` is the Gram tile W.W^T
    const int upd_waves = steps < 4 ? steps : 4;

    ob_d4 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t] = ob_d4{0.0, 0.0, 0.0, 0.0};

    const int64_t tiles = (n + kObTile - 1) / kObTile;
    const int64_t per_block = (tiles + gridDim.x - 1) / gridDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * per_block, t1 = t0 + per_block < tiles ? t0 + per_block : tiles;

    ObStage<ALIGNED, 4> sv;
    ObStage<ALIGNED, 1> sw;
    if (t0 < t1) {
        const int64_t i0 = t0 * kObTile, i1 = i0 + kObTile < n ? i0 + kObTile : n;
        sv.load(V, ldv, m, i0, i1);
        sw.load(W, ldw, K, i0, i1);
    }
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t i0 = t * kObTile, i1 = i0 + kObTile < n ? i0 + kObTile : n;
        __syncthreads(); // the previous tile's LDS reads are done
        sv.store(s_V, m);
        sw.store(s_W, K);
        __syncthreads();
        if (t + 1 < t1) { // the next tile's loads fly while this one is computed
            const int64_t n0 = i0 + kObTile, n1 = n0 + kObTile < n ? n0 + kObTile : n;
            sv.load(V, ldv, m, n0, n1);
            sw.load(W, ldw, K, n0, n1);
        }
        if (UPDATE) {
            // U[c][j] = sum_k H[k][c] V[k][j]: A[c][k] = H[k][c] (read through the cache: m x K <= 2048 doubles, the same for
            // every tile), B[k][j] = V[k][j]; wave w takes the k-steps w, w + 4, ...
            if (wave < upd_waves) {
                ob_d4 u = ob_d4{0.0, 0.0, 0.0, 0.0};
                for (int st = wave; st < steps; st += 4) {
                    const int k = 4 * st + hi;
                    u = ob_mfma(k < m && lo < K ? H[(int64_t)k * K + lo] : 0.0, k < m ? s_V[k][lo] : 0.0, u);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) s_U[UPDATE ? wave : 0][hi + 4 * r][lo] = u[r];
            }
            __syncthreads();
            // W' = W - U, summed over the waves in a fixed order; written back to W
            const int c = threadIdx.x >> 4, j = threadIdx.x & 15;
            if (c < K) {
                double u = 0.0;
                for (int q = 0; q < upd_waves; ++q) u += s_U[UPDATE ? q : 0][c][j];
                const double w = s_W[c][j] - u;
                s_W[c][j] = w;
                if (i0 + j < i1) W[(int64_t)c * ldw + i0 + j] = w;
            }
            __syncthreads();
        }
        // B[j][c] = W'[c][j] for the 4 k-steps of the tile (the same for every row tile; also the A operand of the Gram tile)
        double b[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) b[s] = lo < K ? s_W[lo][4 * s + hi] : 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int vt = wave + 4 * q;
            if (vt < vtiles) {
                const int k = 16 * vt + lo;
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[q] = ob_mfma(k < m ? s_V[k][4 * s + hi] : 0.0, b[s], acc[q]);
            } else if (vt == vtiles) {
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[q] = ob_mfma(b[s], b[s], acc[q]);
            }
        }
    }
    // lane l, register r holds D[(l >> 4) + 4 r][l & 15]: row k (or c') of the tile, column c
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int vt = wave + 4 * q;
        if (vt > vtiles || lo >= K) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = hi + 4 * r;
            if (vt < vtiles) {
                const int k = 16 * vt + row;
                if (k < m) unsafeAtomicAdd(out + (int64_t)k * K + lo, acc[q][r]);
            } else if (row < K) {
                unsafeAtomicAdd(out + (int64_t)m * K + row * K + lo, acc[q][r]);
            }
        }
    }
}

// V[:m_out] <- S^T V[:m_in] on 16-column tiles: Y[o][j] = sum_k S[k][o] V[k][j] with A[o][k] = S[k][o] (read through the cache:
// m_in x m_out <= 128 x 128 doubles), B = the LDS tile of V.  Wave w computes the 16-row output tiles w, w + 4.
template <bool ALIGNED>
__global__ __launch_bounds__(kObBlock) void k_block_rotate(int m_in, int m_out, int64_t n, double *__restrict__ V, int64_t ldv,
                                                           double const *__restrict__ S) {
    __shared__ double s_V[kObMaxRows][kObLd];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lo = lane & 15, hi = lane >> 4;
    const int steps = (m_in + 3) >> 2, otiles = (m_out + 15) >> 4;

    const int64_t tiles = (n + kObTile - 1) / kObTile;
    const int64_t per_block = (tiles + gridDim.x - 1) / gridDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * per_block, t1 = t0 + per_block < tiles ? t0 + per_block : tiles;

    ObStage<ALIGNED, 4> sv;
    if (t0 < t1) {
        const int64_t i0 = t0 * kObTile;
        sv.load(V, ldv, m_in, i0, i0 + kObTile < n ? i0 + kObTile : n);
    }
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t i0 = t * kObTile, i1 = i0 + kObTile < n ? i0 + kObTile : n;
        __syncthreads();
        sv.store(s_V, m_in);
        __syncthreads();
        // every row of this tile is in LDS: the rows written below are not read again for these columns
        if (t + 1 < t1) {
            const int64_t n0 = i0 + kObTile;
            sv.load(V, ldv, m_in, n0, n0 + kObTile < n ? n0 + kObTile : n);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ot = wave + 4 * q;
            if (ot >= otiles) continue;
            const int o = 16 * ot + lo;
            ob_d4 y = ob_d4{0.0, 0.0, 0.0, 0.0};
            for (int st = 0; st < steps; ++st) {
                const int k = 4 * st + hi;
                const double a = (k < m_in && o < m_out) ? S[(int64_t)k * m_out + o] : 0.0;
                y = ob_mfma(a, k < m_in ? s_V[k][lo] : 0.0, y);
            }
            // lane l, register r: output row 16 ot + (l >> 4) + 4 r, column l & 15 of the tile
            if (i0 + lo < i1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * ot + hi + 4 * r;
                    if (row < m_out) V[(int64_t)row * ldv + i0 + lo] = y[r];
                }
            }
        }
    }
}

extern "C" int ls_amd_internal_error(char const *fmt, ...); // host.c: formats into ls_amd_last_error(), returns -1
extern "C" int ls_amd_orth_block_max_rows(void) { return kObMaxRows; }

// one resident grid (4 workgroups per CU: the occupancy both kernels keep), each workgroup a contiguous range of whole tiles
static unsigned ob_grid(int64_t n) {
    int64_t tiles = (n + kObTile - 1) / kObTile;
    if (tiles > 256 * 4) tiles = 256 * 4;
    return (unsigned)(tiles < 1 ? 1 : tiles);
}

extern "C" int ls_amd_orth_block_pass(int m, int K, int64_t n, double const *d_V, int64_t ldv, double *d_W, int64_t ldw,
                                      double const *d_H_in, double *d_out, void *stream) {
    if (m < 0 || m > kObMaxRows || K < 1 || K > kObMaxCols || n < 0 || (m > 0 && ldv < n) || ldw < n || !d_W || !d_out ||
        (m > 0 && !d_V))
        return ls_amd_internal_error("ls_amd_orth_block_pass: bad arguments (m = %d of at most %d rows, K = %d of at most %d, n = %lld, "
                                     "ldv = %lld, ldw = %lld)", m, kObMaxRows, K, kObMaxCols, (long long)n, (long long)ldv, (long long)ldw);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_out, 0, sizeof(double) * (size_t)(m * K + K * K), s);
    if (e != hipSuccess) return ls_amd_internal_error("ls_amd_orth_block_pass: hipMemsetAsync: %s", hipGetErrorString(e));
    if (n == 0) return 0;
    const bool update = d_H_in != nullptr && m > 0;
    const bool aligned = ((uintptr_t)d_V % 16 == 0) && ((uintptr_t)d_W % 16 == 0) && (ldv % 2 == 0) && (ldw % 2 == 0);
    const dim3 grid(ob_grid(n)), block(kObBlock);
    if (update) {
        if (aligned) hipLaunchKernelGGL((k_orth_block_pass<true, true>), grid, block, 0, s, m, K, n, d_V, ldv, d_W, ldw, d_H_in, d_out);
        else hipLaunchKernelGGL((k_orth_block_pass<true, false>), grid, block, 0, s, m, K, n, d_V, ldv, d_W, ldw, d_H_in, d_out);
    } else {
        if (aligned) hipLaunchKernelGGL((k_orth_block_pass<false, true>), grid, block, 0, s, m, K, n, d_V, ldv, d_W, ldw, nullptr, d_out);
        else hipLaunchKernelGGL((k_orth_block_pass<false, false>), grid, block, 0, s, m, K, n, d_V, ldv, d_W, ldw, nullptr, d_out);
    }
    e = hipGetLastError();
    return e == hipSuccess ? 0 : ls_amd_internal_error("ls_amd_orth_block_pass: launch (m = %d, K = %d, n = %lld): %s", m, K, (long long)n, hipGetErrorString(e));
}

extern "C" int ls_amd_block_rotate(int m_in, int m_out, int64_t n, double *d_V, int64_t ldv, double const *d_S, void *stream) {
    if (m_in < 1 || m_in > kObMaxRows || m_out < 1 || m_out > m_in || n < 0 || ldv < n || !d_V || !d_S)
        return ls_amd_internal_error("ls_amd_block_rotate: bad arguments (m_in = %d, m_out = %d, at most %d rows, n = %lld, ldv = %lld)",
                                     m_in, m_out, kObMaxRows, (long long)n, (long long)ldv);
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool aligned = ((uintptr_t)d_V % 16 == 0) && (ldv % 2 == 0);
    if (aligned) hipLaunchKernelGGL(k_block_rotate<true>, dim3(ob_grid(n)), dim3(kObBlock), 0, s, m_in, m_out, n, d_V, ldv, d_S);
    else hipLaunchKernelGGL(k_block_rotate<false>, dim3(ob_grid(n)), dim3(kObBlock), 0, s, m_in, m_out, n, d_V, ldv, d_S);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ls_amd_internal_error("ls_amd_block_rotate: launch (m_in = %d, m_out = %d, n = %lld): %s", m_in, m_out, (long long)n, hipGetErrorString(e));
}
