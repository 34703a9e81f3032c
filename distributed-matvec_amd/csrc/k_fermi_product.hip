// k_fermi_product.hip -- enumeration of a projected spinful-fermion basis with fixed (N_up, N_down): the signed representative test
// of k_fermi_enum_flags (k_fermi.hip, lsk_fermi.hpp) over the PRODUCT candidate set instead of one fixed-weight set.  A unit of its
// own: k_fermi.hip keeps exactly the kernels whose resources are compared with their spin twins.
#include "lsk_dev.hpp"
#include "lsk_fermi.hpp"

// The candidates of a spinful (N_up, N_down) basis: candidate c = b n_a + a is unrank(b, N_down) << L | unrank(a, N_up)
// (the order of k_enum_product, ascending in the word).  A thread unranks its first candidate with two combinadic unranks and then
// steps the up word, carrying into the down word.  WRITE: the second pass walks the same candidates and writes the flagged ones
// at offsets[t] (the exclusive scan of the first pass's counts).
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void k_fermi_enum_product(lsk_basis bs, lsk_group_elem const *__restrict__ elems, int n_up, int n_dn,
                                                               int64_t n_a, uint64_t const *__restrict__ g_binom, int64_t n_cand,
                                                               int64_t n_threads, uint64_t *__restrict__ flags, int64_t *__restrict__ counts,
                                                               int64_t const *__restrict__ offsets, uint64_t *__restrict__ out) {
    __shared__ uint64_t s_binom[64 * LSK_BINOM_K];
    load_binom(s_binom, g_binom);
    const int L = bs.number_sites >> 1;
    const uint64_t a_first = n_up ? (1ULL << n_up) - 1 : 0; // (n_up <= L <= 32)
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n_threads; t += (int64_t)gridDim.x * kBlock) {
        const int64_t c0 = t * 64;
        const int64_t c1 = c0 + 64 < n_cand ? c0 + 64 : n_cand;
        uint64_t m = WRITE ? flags[t] : 0;
        if (WRITE && !m) continue;
        int64_t rb = c0 / n_a, ra = c0 - rb * n_a;
        uint64_t b = unrank_combinadic(rb, n_dn, s_binom), a = unrank_combinadic(ra, n_up, s_binom);
        int64_t o = WRITE ? offsets[t] : 0;
        for (int64_t c = c0; c < c1; ++c) {
            const uint64_t s = (b << L) | a;
            if (WRITE) { if ((m >> (c - c0)) & 1) out[o++] = s; }
            else if (fermi_is_representative(bs, elems, s)) m |= 1ULL << (c - c0);
            if (c + 1 < c1) { // (a successor exists: Gosper's step is never taken on an empty or an exhausted word)
                if (++ra == n_a) { ra = 0; a = a_first; b = next_fixed_hamming(b); }
                else a = next_fixed_hamming(a);
            }
        }
        if (!WRITE) { flags[t] = m; counts[t] = __popcll(m); }
    }
}
extern "C" int lsk_fermi_enumerate_product(lsk_basis bs, int n_up, int n_dn, uint64_t const *d_binom, uint64_t **d_states, int64_t *count,
                                           void *stream) {
    hipStream_t s = (hipStream_t)stream;
    *d_states = nullptr;
    *count = 0;
    const int L = bs.number_sites >> 1;
    if (!bs.fermi || !bs.fsign || bs.spin_inversion != 0 || (bs.number_sites & 1) || L < 1 || L > 32 || n_up < 0 || n_up > L || n_dn < 0 || n_dn > L) {
        snprintf(g_err, sizeof(g_err), "lsk_fermi_enumerate_product: not a projected spinful-fermion basis");
        return -1;
    }
    uint64_t h_binom[2];
    LSK_CHECK(hipMemcpy(&h_binom[0], d_binom + (size_t)L * LSK_BINOM_K + n_up, 8, hipMemcpyDeviceToHost));
    LSK_CHECK(hipMemcpy(&h_binom[1], d_binom + (size_t)L * LSK_BINOM_K + n_dn, 8, hipMemcpyDeviceToHost));
    const int64_t n_a = (int64_t)h_binom[0], n_cand = n_a * (int64_t)h_binom[1]; // >= 1
    const int64_t n_threads = (n_cand + 63) / 64;
    uint64_t *flags = nullptr;
    int64_t *counts = nullptr, *offsets = nullptr;
    LSK_CHECK(hipMalloc((void **)&flags, 8 * n_threads));
    LSK_CHECK(hipMalloc((void **)&counts, 8 * n_threads));
    LSK_CHECK(hipMalloc((void **)&offsets, 8 * n_threads));
    int rc = -1;
    int64_t total = 0;
    do {
        hipLaunchKernelGGL(k_fermi_enum_product<false>, dim3(grid_for(n_threads)), dim3(kBlock), 0, s, bs, bs.elems, n_up, n_dn, n_a, d_binom,
                           n_cand, n_threads, flags, counts, nullptr, nullptr);
        if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "lsk_fermi_enumerate_product: launch failed"); break; }
        if (lsk_internal_exclusive_scan_i64(n_threads, counts, offsets, s) != 0) break;
        int64_t last_off = 0, last_cnt = 0;
        if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(&last_off, offsets + (n_threads - 1), 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(&last_cnt, counts + (n_threads - 1), 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMalloc((void **)d_states, (total = last_off + last_cnt) > 0 ? 8 * total : 8) != hipSuccess) {
            snprintf(g_err, sizeof(g_err), "lsk_fermi_enumerate_product: %s", hipGetErrorString(hipGetLastError()));
            break;
        }
        hipLaunchKernelGGL(k_fermi_enum_product<true>, dim3(grid_for(n_threads)), dim3(kBlock), 0, s, bs, bs.elems, n_up, n_dn, n_a, d_binom,
                           n_cand, n_threads, flags, nullptr, offsets, *d_states);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            snprintf(g_err, sizeof(g_err), "lsk_fermi_enumerate_product: the write pass failed");
            break;
        }
        rc = 0;
    } while (0);
    (void)hipFree(flags); (void)hipFree(counts); (void)hipFree(offsets);
    if (rc != 0) { if (*d_states) (void)hipFree(*d_states); *d_states = nullptr; return -1; }
    *count = total;
    return 0;
}
