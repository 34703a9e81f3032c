// lsk_fermi.hpp -- K4 of projected fermionic bases (spinless, and spinful over their 2 L modes): the permutation sign of a Fock
// state (convention: include/ls_hs.h).
//
// An element g with (g.a)[i] = a[p_i] acts as U_g c+_j U_g+ = c+_{p^-1(j)}, so U_g |a> = sign(g, a) |g.a> with
// sign = (-1)^(number of occupied pairs j < j' with p^-1(j) > p^-1(j')).  U is a representation (U_g U_h = U_gh), so
//   - sign(g0 s, a) = sign(g0, a) sign(s, a) for s in Stab(a): every element that maps a onto its orbit minimum carries the
//     effective character chi(g) sign(g, a) = chi(g0) sign(g0, a) * chi(s) sign(s, a), and the tie accumulation of state_info_w
//     still yields the stabiliser sum  sum_{s in Stab(a)} chi(s) sign(s, a)  once multiplied by conj(chi(g0) sign(g0, a));
//   - that sum may vanish in any sector (4-site ring, N = 2: T^2 fixes 0101 with sign -1), so the fermionic K4 never skips the
//     norm: these bases always run K4 mode 0.
// The sign is written over MODES (the bits of the state word).  A spinful basis lifts its site permutations to both species on the
// host (p + p over the 2 L modes, and the half swap for the up <-> down flip): nothing here changes for them, but a lifted ring
// rotation / reflection has a closed form per half (the LSK_ELEM_LIFT kinds of lsk.h) instead of a network and one table load per
// particle.
// Everything here is a template or __host__ __device__: k_fermi.hip uses it, k_pull_t.hpp compiles it into the fermionic
// k_pull_t instantiations, and lsk_test_fermi_parity runs the same code on the host.  k_expand_fermi.hip takes the element signs
// and the sign of a bipartition (fermi_split_parity, below) from here; lsk_test_fermi_split_parity is its host run.
#pragma once
#include "lsk.h"

template <typename W> __host__ __device__ __forceinline__ int fermi_popc(W v) {
    return sizeof(W) == 4 ? __builtin_popcount((uint32_t)v) : __builtin_popcountll((uint64_t)v);
}
template <typename W> __host__ __device__ __forceinline__ int fermi_ctz(W v) {
    return sizeof(W) == 4 ? __builtin_ctz((uint32_t)v) : __builtin_ctzll((uint64_t)v);
}
// parity of sign(g, a) for the element e; tab = its row of the sign table (lsk_basis.fsign + g * L).  Closed forms:
//   ROT k (output bit i = input bit (i + k) mod L): the pairs with one mode below k and one at or above it swap order,
//     (-1)^(n_low n_high);
//   REVROT k (reverse first, then rotate, as apply_elem): (-1)^(N (N - 1) / 2) for the reversal times the rotation's sign on
//     the reversed word;
//   BENES (any permutation): the GF(2) quadratic form  parity(a & XOR_{i in occ(a)} tab[i]),  tab[i] = the modes j < i that
//     the permutation puts above i -- one table load per particle.
//   LIFT kinds (word of 2 h modes, h = L / 2; u = up half, d = down half): the site element acts inside each half, and no pair
//     with one mode in each half changes its order, so the sign is the product of the two halves' ROT / REVROT signs over h
//     modes.  The reversed word is not formed: its low k bits are the top k bits of the half.  With SWAP every (up, down) pair
//     changes its order as well: (-1)^(N_up N_down).
// table != 0 takes the table form for every kind (the host mirror's check of the closed forms).
template <typename W>
__host__ __device__ __forceinline__ int fermi_parity(lsk_group_elem const &e, uint64_t const *__restrict__ tab, W a, int L, bool table) {
    if (table || e.kind == LSK_ELEM_BENES) {
        W x = 0;
        for (W m = a; m != 0; m &= m - 1) x ^= (W)tab[fermi_ctz<W>(m)];
        return fermi_popc<W>(a & x) & 1;
    }
    if (e.kind & LSK_ELEM_LIFT) {
        const int h = L >> 1, k = e.k; // 0 <= k < h, 2 h <= 8 sizeof(W)
        const W hm = (W)(((W)1 << h) - 1);
        const W u = a & hm, d = (W)(a >> h);
        const bool rev = (e.kind & LSK_ELEM_LIFT_REV) != 0;
        const W mk = rev ? (W)(hm & ~(hm >> k)) : (W)(((W)1 << k) - 1); // the k modes that the rotation carries past the others
        const int nu = fermi_popc<W>(u), nd = fermi_popc<W>(d);
        const int au = fermi_popc<W>(u & mk), ad = fermi_popc<W>(d & mk);
        int par = (au & (nu - au)) ^ (ad & (nd - ad));
        if (rev) par ^= (nu >> 1) ^ (nd >> 1); // (-1)^(n (n - 1) / 2) per half
        if (e.kind & LSK_ELEM_LIFT_SWAP) par ^= nu & nd;
        return par & 1;
    }
    int par = 0;
    W w = a;
    if (e.kind == LSK_ELEM_REVROT) {
        const int n = fermi_popc<W>(a);
        par = (n * (n - 1) / 2) & 1;
        W r = 0;
        if (sizeof(W) == 4) r = (W)(__builtin_bitreverse32((uint32_t)a) >> (32 - L));
        else r = (W)(__builtin_bitreverse64((uint64_t)a) >> (64 - L));
        w = r;
    }
    const int k = e.k; // 0 <= k < L <= 8 sizeof(W)
    const int lo = k ? fermi_popc<W>(w & (W)(((W)1 << k) - 1)) : 0;
    const int hi = fermi_popc<W>(w) - lo;
    return par ^ (lo & hi & 1);
}

// The sign of a bipartition (k_expand_fermi.hip).  |n> = c+_{k1} ... c+_{kN} |0>, k1 < ... < kN, and
// |a>_A |b>_B := (prod_{k in A, ascending} c+_k) (prod_{k in B, ascending} c+_k) |0> -- the modes of A in front -- differ by
//   sigma(n) = (-1)^#{(i, j): i in A, j in B, both occupied, j < i}:
// every occupied mode of B that stands in front of an occupied mode of A is carried past it.  With prefix(y) = the word whose bit i
// is the parity of the bits of y below i (log2(width) shift-xor steps), the exponent is popcount(n & mask_a & prefix(n & mask_b)).
template <typename W> __host__ __device__ __forceinline__ W fermi_prefix_parity(W y) {
    y = (W)(y << 1); // exclusive: bit i collects the bits strictly below i
    y ^= (W)(y << 1);
    y ^= (W)(y << 2);
    y ^= (W)(y << 4);
    y ^= (W)(y << 8);
    y ^= (W)(y << 16);
    if (sizeof(W) == 8) y ^= (W)((uint64_t)y << 32);
    return y;
}
template <typename W> __host__ __device__ __forceinline__ int fermi_split_parity(W n, W mask_a, W mask_b) {
    return fermi_popc<W>(n & mask_a & fermi_prefix_parity<W>(n & mask_b)) & 1;
}

// apply_elem_w with the LIFT kinds: rotate / reverse both h-bit halves in registers, optionally exchange them.  Reversing the
// whole 2 h-bit word reverses each half AND exchanges them, so REV costs one bit reversal and REV + SWAP no exchange at all.
template <typename W> __host__ __device__ __forceinline__ W fermi_apply_lift(lsk_group_elem const &e, W x, int L, W mask) {
    const int h = L >> 1, k = e.k;
    bool swap = (e.kind & LSK_ELEM_LIFT_SWAP) != 0;
    if (e.kind & LSK_ELEM_LIFT_REV) {
        if (sizeof(W) == 4) x = (W)(__builtin_bitreverse32((uint32_t)x) >> (32 - L));
        else x = (W)(__builtin_bitreverse64((uint64_t)x) >> (64 - L));
        swap = !swap;
    }
    if (k) {
        const W hm = (W)(((W)1 << h) - 1);
        const W m1 = (W)((hm >> k) | ((W)(hm >> k) << h)); // where x >> k stays inside its half
        x = (W)(((x >> k) & m1) | ((W)(x << (h - k)) & mask & ~m1));
    }
    if (swap) x = (W)(((x >> h) | (W)(x << h)) & mask);
    return x;
}
#ifdef __HIPCC__
template <typename W> __device__ __forceinline__ W fermi_apply_elem_w(lsk_group_elem const &e, W x, int L, W mask) {
    if (e.kind & LSK_ELEM_LIFT) return fermi_apply_lift<W>(e, x, L, mask);
    return apply_elem_w<W>(e, x, L, mask);
}
// state_info_w (lsk_dev.hpp) with the signed characters chi(g) sign(g, a): orbit minimum, conj(chi(g0) sign(g0, a)) of the first
// minimising element, stabiliser sum.  No spin inversion (fermionic bases have none).  PM1: every character is +-1.
template <typename W, bool PM1>
__device__ __forceinline__ void fermi_state_info_w(lsk_basis const &bs, lsk_group_elem const *__restrict__ elems, W a, W &rep,
                                                   double &chr, double &chi, double &stab) {
    W best = ~(W)0;
    int g0 = 0, s0 = 0, si = 0;
    double sr = 0.0, sim = 0.0;
    const int L = bs.number_sites;
    const W mask = (W)bs.site_mask;
    for (int g = 0; g < bs.n_elems; ++g) {
        lsk_group_elem const &e = elems[g];
        const W t = fermi_apply_elem_w<W>(e, a, L, mask);
        const int par = fermi_parity<W>(e, bs.fsign + (size_t)g * L, a, L, false);
        const bool less = t < best, eq = t == best;
        if (PM1) {
            int ch = (int)e.ch_re;
            ch = par ? -ch : ch;
            si = less ? ch : (eq ? si + ch : si);
        } else {
            const double cr = par ? -e.ch_re : e.ch_re, ci = par ? -e.ch_im : e.ch_im;
            sr = less ? cr : (eq ? sr + cr : sr);
            sim = less ? ci : (eq ? sim + ci : sim);
        }
        best = less ? t : best;
        g0 = less ? g : g0;
        s0 = less ? par : s0;
    }
    rep = best;
    double c0r = elems[g0].ch_re, c0i = elems[g0].ch_im;
    if (s0) { c0r = -c0r; c0i = -c0i; }
    chr = c0r;
    chi = -c0i;
    if (PM1) stab = c0r * (double)si;
    else stab = c0r * sr + c0i * sim; // Re(conj(chi0 sign0) * S)
}
// is_representative (lsk_dev.hpp) with signs: false as soon as some element maps below a, else the signed stabiliser sum decides
__device__ __forceinline__ bool fermi_is_representative(lsk_basis const &bs, lsk_group_elem const *__restrict__ elems, uint64_t a) {
    double st = 0.0;
    for (int g = 0; g < bs.n_elems; ++g) {
        lsk_group_elem const &e = elems[g];
        const uint64_t t = fermi_apply_elem_w<uint64_t>(e, a, bs.number_sites, bs.site_mask);
        if (t < a) return false;
        if (t == a) st += fermi_parity<uint64_t>(e, bs.fsign + (size_t)g * bs.number_sites, a, bs.number_sites, false) ? -e.ch_re : e.ch_re;
    }
    return st * bs.inv_order > 1e-12;
}
#endif
