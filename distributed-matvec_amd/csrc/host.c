/* host.c -- C host side of the MI355X-native matvec: the ls_hs_* ABI subset, plans, and the
 * ls_chpl_* exports of the reference's shared library.  Plain C11; every device action goes through
 * the extern-"C" shim in the k_*.hip translation units (lsk.h).  No compute on the CPU: the functions here build
 * tables (symmetry-group closure, Benes networks, term grouping), size buffers and launch kernels.
 *
 * Reference behaviour mirrored (see include/ls_chpl.h, include/ls_amd.h for per-symbol citations):
 *   localMatrixVector / matrixVectorProduct   /root/reference/src/DistributedMatrixVector.chpl:1055-1110
 *   localOffDiagonalNoQueue (sizing, rounds)  /root/reference/src/DistributedMatrixVector.chpl:856-1053
 *   enumerateStates                           /root/reference/src/StatesEnumeration.chpl:516-603
 *   Diagonalize's PRIMME callback             /root/reference/src/Diagonalize.chpl:134-162
 */
#define _GNU_SOURCE
#include <math.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ls_amd.h"
#include "../../include/ls_chpl.h"
#include "../../include/ls_hs.h"
#include "lsk.h"

/* ============================================================================================ */
/* errors                                                                                       */
/* ============================================================================================ */
static __thread char g_last_error[1024] = "";
static ls_amd_error_handler g_handler = NULL;

static int set_error(char const *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
    return -1;
}
static int dev_error(void) { return set_error("%s", lsk_last_error()); }
/* for the other host files (dist.c): same buffer, same -1 */
int ls_amd_internal_error(char const *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
    return -1;
}
#define DEV(expr) do { if ((expr) != 0) return dev_error(); } while (0)
/* a constructor that succeeded leaves no message behind (a failed attempt before it must not read as this call's error) */
void ls_amd_internal_clear_error(void) { g_last_error[0] = 0; }

char const *ls_amd_last_error(void) { return g_last_error; }
void ls_amd_set_error_handler(ls_amd_error_handler handler) { g_handler = handler; }

/* the reference's `halt(...)` */
static void halt_with(char const *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    snprintf(g_last_error, sizeof(g_last_error), "%s", buf);
    if (g_handler) { g_handler(buf); return; }
    fprintf(stderr, "[Error]   halt: %s\n", buf);
    abort();
}

/* ============================================================================================ */
/* device helpers re-exported                                                                   */
/* ============================================================================================ */
/* object registry                                                                              */
/* ============================================================================================ */
/* Everything this library knows about a basis / an operator beyond the struct prefix the reference declares
 * (/root/reference/src/FFI.chpl:94-119) lives in a side table keyed by the object's address -- NOT in a trailing struct
 * field: an ls_hs_operator built by the real lattice-symmetries-haskell has "other stuff" of unknown layout behind the
 * prefix, and reading a field of ours there would be out of bounds.  Objects created here are registered by their
 * constructors; foreign ones by ls_amd_adopt_basis / ls_amd_adopt_operator. */
typedef struct { void const *key; void *val; int kind; } reg_slot;
enum { REG_BASIS = 1, REG_OPERATOR = 2 };
static reg_slot *g_reg = NULL;
static size_t g_reg_cap = 0, g_reg_used = 0; /* used counts live entries and tombstones */
static pthread_mutex_t g_reg_lock = PTHREAD_MUTEX_INITIALIZER;
static void const *const REG_TOMB = (void const *)(uintptr_t)1;

static size_t reg_hash(void const *k, size_t cap) { return (size_t)(((uintptr_t)k >> 4) * 0x9E3779B97F4A7C15ULL) & (cap - 1); }
static void reg_put_nolock(void const *key, void *val, int kind);
static void reg_grow(void) {
    reg_slot *old = g_reg;
    size_t const oc = g_reg_cap;
    g_reg_cap = oc ? 2 * oc : 64;
    g_reg = (reg_slot *)calloc(g_reg_cap, sizeof(reg_slot));
    g_reg_used = 0;
    for (size_t i = 0; i < oc; ++i)
        if (old[i].key && old[i].key != REG_TOMB) reg_put_nolock(old[i].key, old[i].val, old[i].kind);
    free(old);
}
static void reg_put_nolock(void const *key, void *val, int kind) {
    if (2 * (g_reg_used + 1) > g_reg_cap) reg_grow();
    size_t i = reg_hash(key, g_reg_cap);
    while (g_reg[i].key && g_reg[i].key != REG_TOMB && g_reg[i].key != key) i = (i + 1) & (g_reg_cap - 1);
    if (!g_reg[i].key) ++g_reg_used;
    g_reg[i].key = key;
    g_reg[i].val = val;
    g_reg[i].kind = kind;
}
static void reg_put(void const *key, void *val, int kind) {
    pthread_mutex_lock(&g_reg_lock);
    reg_put_nolock(key, val, kind);
    pthread_mutex_unlock(&g_reg_lock);
}
static void *reg_find(void const *key, int *kind) {
    void *v = NULL;
    pthread_mutex_lock(&g_reg_lock);
    if (g_reg_cap) {
        size_t i = reg_hash(key, g_reg_cap);
        while (g_reg[i].key) {
            if (g_reg[i].key == key) { v = g_reg[i].val; if (kind) *kind = g_reg[i].kind; break; }
            i = (i + 1) & (g_reg_cap - 1);
        }
    }
    pthread_mutex_unlock(&g_reg_lock);
    return v;
}
static void *reg_get(void const *key) { return reg_find(key, NULL); }
static void reg_del(void const *key) {
    pthread_mutex_lock(&g_reg_lock);
    if (g_reg_cap) {
        size_t i = reg_hash(key, g_reg_cap);
        while (g_reg[i].key) {
            if (g_reg[i].key == key) { g_reg[i].key = REG_TOMB; g_reg[i].val = NULL; break; }
            i = (i + 1) & (g_reg_cap - 1);
        }
    }
    pthread_mutex_unlock(&g_reg_lock);
}
static void halt_with(char const *fmt, ...);
struct ls_amd_basis_ext;
struct ls_amd_operator_ext;
static struct ls_amd_basis_ext *basis_ext_of(ls_hs_basis const *b);
static struct ls_amd_operator_ext *operator_ext_of(ls_hs_operator const *op);
#define BEXT(b) basis_ext_of(b)
#define NBITS(b) (BEXT(b)->nbits) /* width of a basis state: number_sites counts sites, not modes */
#define OEXT(op) operator_ext_of(op)

/* ============================================================================================ */
int ls_amd_device_count(void) { return lsk_device_count(); }
int ls_amd_set_device(int device) { DEV(lsk_set_device(device)); return 0; }
int ls_amd_malloc(void **d_ptr, size_t bytes) { DEV(lsk_malloc(d_ptr, bytes)); return 0; }
int ls_amd_free(void *d_ptr) { DEV(lsk_free(d_ptr)); return 0; }
int ls_amd_memcpy_h2d(void *d, void const *h, size_t bytes) { DEV(lsk_h2d(d, h, bytes)); return 0; }
int ls_amd_memcpy_d2h(void *h, void const *d, size_t bytes) { DEV(lsk_d2h(h, d, bytes)); return 0; }
int ls_amd_memcpy_d2d(void *d, void const *s, size_t bytes, void *stream) { DEV(lsk_d2d_async(d, s, bytes, stream)); return 0; }
int ls_amd_memset(void *d, int value, size_t bytes, void *stream) { DEV(lsk_memset_async(d, value, bytes, stream)); return 0; }
int ls_amd_synchronize(void *stream) { DEV(lsk_sync(stream)); return 0; }

uint64_t ls_amd_hash64_01(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    x = x ^ (x >> 31);
    return x;
}
int ls_amd_locale_idx_of(uint64_t basis_state, int num_locales) {
    return (int)(ls_amd_hash64_01(basis_state) % (uint64_t)num_locales);
}

/* ============================================================================================ */
/* binomials                                                                                    */
/* ============================================================================================ */
static uint64_t g_binom[64 * LSK_BINOM_K];
static int g_binom_ready = 0;
static uint64_t *g_d_binom = NULL;

static void binom_fill(void) {
    for (int n = 0; n < 64; ++n)
        for (int k = 0; k < LSK_BINOM_K; ++k) {
            uint64_t v;
            if (k == 0) v = 1;
            else if (n == 0) v = 0;
            else v = g_binom[(n - 1) * LSK_BINOM_K + (k - 1)] + g_binom[(n - 1) * LSK_BINOM_K + k];
            g_binom[n * LSK_BINOM_K + k] = v;
        }
    g_binom_ready = 1;
}
static pthread_once_t g_binom_once = PTHREAD_ONCE_INIT;
static void binom_init(void) { pthread_once(&g_binom_once, binom_fill); } /* (first use may come from several host threads at once) */
static uint64_t binom(int n, int k) {
    binom_init();
    if (k < 0 || n < 0 || k > n) return 0;
    if (n - k < k) k = n - k;
    if (n < 64 && k < LSK_BINOM_K) return g_binom[n * LSK_BINOM_K + k];
    /* n == 64 or beyond table: compute directly (only used for sizes) */
    long double r = 1;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
    return (uint64_t)(r + 0.5L);
}
static pthread_mutex_t g_binom_lock = PTHREAD_MUTEX_INITIALIZER;
static int device_binom_unlocked(uint64_t const **out);
static int device_binom(uint64_t const **out) { /* first use may come from several host threads at once */
    pthread_mutex_lock(&g_binom_lock);
    int const rc = device_binom_unlocked(out);
    pthread_mutex_unlock(&g_binom_lock);
    return rc;
}
static int device_binom_unlocked(uint64_t const **out) {
    binom_init();
    if (!g_d_binom) {
        void *p;
        DEV(lsk_malloc(&p, sizeof(g_binom)));
        DEV(lsk_h2d(p, g_binom, sizeof(g_binom)));
        g_d_binom = (uint64_t *)p;
    }
    *out = g_d_binom;
    return 0;
}

ptrdiff_t ls_hs_fixed_hamming_state_to_index(uint64_t s) {
    binom_init();
    ptrdiff_t idx = 0;
    int k = 1;
    while (s) {
        int p = __builtin_ctzll(s);
        idx += (ptrdiff_t)binom(p, k);
        ++k;
        s &= s - 1;
    }
    return idx;
}
uint64_t ls_hs_fixed_hamming_index_to_state(ptrdiff_t idx, int hamming_weight) {
    uint64_t s = 0;
    int p = 63;
    for (int k = hamming_weight; k >= 1; --k) {
        while (p > k - 1 && (ptrdiff_t)binom(p, k) > idx) --p;
        s |= 1ULL << p;
        idx -= (ptrdiff_t)binom(p, k);
        --p;
    }
    return s;
}

/* ============================================================================================ */
/* basis                                                                                        */
/* ============================================================================================ */
struct ls_amd_basis_ext {
    int hamming_weight; /* -1 unrestricted (and for the spinful product basis: two weights, see below) */
    int nbits;          /* bits of a basis state: number_sites, or 2 number_sites for spinful fermions */
    /* spinful fermions with fixed (N_up, N_down): the product of the weight-N_up words of the low half (mode (i, up) = bit i)
     * and the weight-N_down words of the high half (mode (i, down) = bit i + L) -- index kind LSK_INDEX_PRODUCT */
    int product, prod_up, prod_dn;
    int n_generators;
    int *gen_perms;     /* [n_generators][L] */
    int *gen_sectors;
    int order;          /* permutation group order (>= 1, identity first) */
    int *perms;         /* [order][L] */
    lsk_group_elem *elems; /* [order] host copy (characters, networks) */
    lsk_group_elem *d_elems;
    /* K4 mode 4 (lsk_basis in lsk.h): the group contains every translation of a tw x (L / tw) torus; coset_ids = one element
     * of every right coset T g (indices into elems), found once per basis.  tw == 0: not looked for yet, -1: no such subgroup */
    int tw, n_cosets;
    int *coset_ids;
    lsk_group_elem *d_cosets;
    uint32_t *d_trow;    /* mode 4, tw <= 8: the row table of torus_min on the device */
    int d4_mask;         /* mode 5: which of 1, r, o, r o (bits 0-3) and of their products with the transpose (bits 4-7) the cosets are;
                          * 0 = not examined, -1 = the cosets are not of that form */
    lsk_group_elem d4_transpose; /* the transpose network (the only compiled network of mode 5) */
    lsk_group_elem *d_d4_net;
    uint64_t *d_trow2;   /* mode 5: row table with the reversed row's fields in the high half */
    /* projected spinless-fermion basis: the permutation sign of every element (lsk_fermi.hpp) -- fsign[g][i] = the modes j < i that
     * element g puts above mode i -- and its device copy (lsk_basis.fsign) */
    int fermi;
    uint64_t *fsign, *d_fsign;
    /* projected spinful-fermion basis (ls_hs_create_spinful_fermion_basis): gen_perms holds the generators LIFTED to the 2 L modes
     * (the n_generators - 1 site generators, then the half swap, when spin_flip != 0) */
    int spin_flip;
    int owns_representatives;
    uint64_t *d_reps_cache; /* device copy of `representatives` for the host-pointer entry points */
    uint64_t d_reps_count;
    /* plans cached by the host-pointer entry points (ls_chpl_matrix_vector_product, ls_chpl_primme_matvec), keyed by the
     * OPERATOR and the communicator they were built for: several operators share one basis (H and an observable,
     * ls_hs_clone_operator), and each needs its own device term tables */
    struct host_plan_slot {
        ls_hs_operator const *op;
        void *comm;    /* ls_amd_comm* (NULL: single process) */
        void *plan;    /* ls_amd_plan* when comm == NULL */
        void *dist;    /* ls_amd_dist* otherwise */
        uint64_t stamp;
        /* persistent device copies of the caller's host vectors (allocated on first use, kept with the plan; the second pair
         * only for blocks of columns: the upload of column k + 1 overlaps kernel and download of column k) */
        void *d_x[2], *d_y[2];
        int64_t stage_n;
    } host_plans[4];
    uint64_t host_plan_clock;
    uint32_t *d_index_table; /* search table over d_reps_cache (ls_hs_state_index) */
    int index_kind, index_shift;
    int refcount;           /* the creator's reference + one per operator built on the basis */
    int adopted;            /* the struct belongs to somebody else (ls_amd_adopt_basis): never freed here */
};

static struct ls_amd_basis_ext g_dummy_basis_ext;
static struct ls_amd_basis_ext *basis_ext_of(ls_hs_basis const *b) {
    struct ls_amd_basis_ext *e = (struct ls_amd_basis_ext *)reg_get(b);
    if (!e) {
        halt_with("ls_hs_basis %p was not created by this library: register it with ls_amd_adopt_basis first", (void const *)b);
        g_dummy_basis_ext.hamming_weight = -1;
        return &g_dummy_basis_ext;
    }
    return e;
}

void ls_hs_init(void) {}
void ls_hs_exit(void) {}

static int perm_order(int const *p, int L) {
    int *q = (int *)malloc(sizeof(int) * L), *t = (int *)malloc(sizeof(int) * L);
    memcpy(q, p, sizeof(int) * L);
    int n = 1;
    for (;;) {
        int ident = 1;
        for (int i = 0; i < L; ++i) if (q[i] != i) { ident = 0; break; }
        if (ident) break;
        for (int i = 0; i < L; ++i) t[i] = q[p[i]]; /* compose(p, q)[i] = q[p[i]] */
        memcpy(q, t, sizeof(int) * L);
        ++n;
    }
    free(q); free(t);
    return n;
}

/* Benes network for y[i] = x[src[i]], i < 64.  masks[level] = input stage of recursion level
 * `level` (distance 32 >> level), masks[10 - level] = its output stage, masks[5] = the middle. */
static void benes_route(int base, int n, int const *src, int level, uint64_t *masks) {
    if (n == 2) {
        if (src[0] == 1) masks[5] |= 1ULL << base;
        return;
    }
    int const h = n / 2;
    int inv[64], incolor[64], outcolor[64], lower[32], upper[32];
    for (int i = 0; i < n; ++i) { inv[src[i]] = i; incolor[i] = -1; outcolor[i] = -1; }
    for (int o = 0; o < n; ++o) {
        if (outcolor[o] != -1) continue;
        int cur = o, c = 0;
        while (outcolor[cur] == -1) {
            outcolor[cur] = c;
            int s = src[cur];
            incolor[s] = c;
            int sp = s ^ h;
            incolor[sp] = 1 - c;
            int o2 = inv[sp];
            outcolor[o2] = 1 - c;
            cur = o2 ^ h;
        }
    }
    for (int j = 0; j < h; ++j) {
        if (incolor[j] == 1) masks[level] |= 1ULL << (base + j);
        if (outcolor[j] == 1) masks[10 - level] |= 1ULL << (base + j);
    }
    for (int i = 0; i < h; ++i) {
        int fo_l = (outcolor[i] == 0) ? i : i + h;
        int fo_u = (outcolor[i] == 1) ? i : i + h;
        lower[i] = src[fo_l] & (h - 1);
        upper[i] = src[fo_u] & (h - 1);
    }
    benes_route(base, h, lower, level + 1, masks);
    benes_route(base + h, h, upper, level + 1, masks);
}

static void compile_elem(int const *perm, int L, double ch_re, double ch_im, lsk_group_elem *e) {
    memset(e, 0, sizeof(*e));
    e->ch_re = ch_re;
    e->ch_im = ch_im;
    /* rotation: perm[i] = (i + k) mod L  -> y = rotr_L(x, k) */
    int k = perm[0];
    int is_rot = 1;
    for (int i = 0; i < L; ++i) if (perm[i] != (i + k) % L) { is_rot = 0; break; }
    if (is_rot) { e->kind = LSK_ELEM_ROT; e->k = k; return; }
    /* reflection + rotation: perm[i] = (k' - i) mod L -> y = rotr_L(rev_L(x), (L - 1 - k') mod L) */
    int kp = perm[0];
    int is_rev = 1;
    for (int i = 0; i < L; ++i) if (perm[i] != ((kp - i) % L + L) % L) { is_rev = 0; break; }
    if (is_rev) { e->kind = LSK_ELEM_REVROT; e->k = ((L - 1 - kp) % L + L) % L; return; }
    int src[64];
    for (int i = 0; i < 64; ++i) src[i] = i < L ? perm[i] : i;
    e->kind = LSK_ELEM_BENES;
    benes_route(0, 64, src, 0, e->masks);
}

static uint64_t host_delta_swap(uint64_t x, uint64_t m, int d) {
    uint64_t t = ((x >> d) ^ x) & m;
    return x ^ t ^ (t << d);
}
/* CPU mirror of apply_elem in lsk_dev.hpp -- used by the test hooks and table checks only */
static uint64_t host_apply_elem(lsk_group_elem const *e, uint64_t x, int L) {
    static int const dist[LSK_BENES_STAGES] = {32, 16, 8, 4, 2, 1, 2, 4, 8, 16, 32};
    uint64_t const mask = L >= 64 ? ~0ULL : ((1ULL << L) - 1);
    if (e->kind & LSK_ELEM_LIFT) return lsk_test_fermi_apply_lift(*e, x, L); /* the fermionic kinds: the device code's own host mirror */
    if (e->kind == LSK_ELEM_BENES) {
        for (int s = 0; s < LSK_BENES_STAGES; ++s)
            if (e->masks[s]) x = host_delta_swap(x, e->masks[s], dist[s]);
        return x;
    }
    if (e->kind == LSK_ELEM_REVROT) {
        uint64_t r = 0;
        for (int i = 0; i < L; ++i) r |= ((x >> i) & 1ULL) << (L - 1 - i);
        x = r;
    }
    if (e->k == 0) return x;
    return ((x >> e->k) | (x << (L - e->k))) & mask;
}

/* The kernels loop over the group elements of a projected basis per candidate state; the largest groups of the reference's inputs
 * have 288 elements (heisenberg_square_6x6), the automorphisms of a 64-site lattice a few thousand */
enum { LS_AMD_MAX_GROUP_ORDER = 1 << 20 }; /* closure is linear in the order (hash-table membership): a million elements take milliseconds */
static uint64_t perm_hash(int const *p, int L) {
    uint64_t h = 0x9e3779b97f4a7c15ULL;
    for (int i = 0; i < L; ++i) { h ^= (uint64_t)(p[i] + 1); h *= 0xff51afd7ed558ccdULL; h ^= h >> 29; }
    return h;
}
static int close_group(struct ls_amd_basis_ext *ext, int L) {
    int const ng = ext->n_generators;
    int cap = 64, order = 1;
    int *perms = (int *)malloc(sizeof(int) * cap * L);
    double *chars = (double *)malloc(sizeof(double) * 2 * cap);
    double *gch = (double *)malloc(sizeof(double) * 2 * (ng > 0 ? ng : 1));
    for (int i = 0; i < L; ++i) perms[i] = i;
    chars[0] = 1.0; chars[1] = 0.0;
    for (int g = 0; g < ng; ++g) {
        int const *p = ext->gen_perms + g * L;
        int n = perm_order(p, L);
        int k = ((ext->gen_sectors[g] % n) + n) % n;
        double ang = -2.0 * M_PI * (double)k / (double)n;
        double re = cos(ang), im = sin(ang);
        /* snap the exact values so real sectors stay exactly real */
        if (fabs(re) < 1e-15) re = 0.0;
        if (fabs(im) < 1e-15) im = 0.0;
        if (fabs(fabs(re) - 1.0) < 1e-15) re = re > 0 ? 1.0 : -1.0;
        if (fabs(fabs(im) - 1.0) < 1e-15) im = im > 0 ? 1.0 : -1.0;
        gch[2 * g] = re; gch[2 * g + 1] = im;
    }
    int *cand = (int *)malloc(sizeof(int) * L);
    /* membership by an open-addressing table of element numbers keyed by a hash of the permutation: the closure is linear in
     * the group order (a linear scan per candidate made generators of a huge group -- a typo in one permutation of a YAML file
     * is enough: two random permutations generate S_L -- run ~2^40 comparisons before the size limit below was reached) */
    size_t tcap = 256;
    int32_t *table = (int32_t *)malloc(sizeof(int32_t) * tcap);
    for (size_t i = 0; i < tcap; ++i) table[i] = -1;
    table[perm_hash(perms, L) & (tcap - 1)] = 0;
    for (int head = 0; head < order; ++head) { /* BFS: `order` grows while we scan */
        for (int g = 0; g < ng; ++g) {
            int const *p = ext->gen_perms + g * L;
            int const *e = perms + (size_t)head * L;
            for (int i = 0; i < L; ++i) cand[i] = e[p[i]]; /* compose(g, e) */
            double cre = chars[2 * head] * gch[2 * g] - chars[2 * head + 1] * gch[2 * g + 1];
            double cim = chars[2 * head] * gch[2 * g + 1] + chars[2 * head + 1] * gch[2 * g];
            int found = -1;
            size_t slot = perm_hash(cand, L) & (tcap - 1);
            for (; table[slot] >= 0; slot = (slot + 1) & (tcap - 1))
                if (memcmp(perms + (size_t)table[slot] * L, cand, sizeof(int) * L) == 0) { found = table[slot]; break; }
            if (found >= 0) {
                if (fabs(chars[2 * found] - cre) > 1e-9 || fabs(chars[2 * found + 1] - cim) > 1e-9) {
                    free(perms); free(chars); free(gch); free(cand); free(table);
                    return set_error("symmetry sectors are incompatible with the group structure");
                }
                continue;
            }
            if (order >= LS_AMD_MAX_GROUP_ORDER) {
                free(perms); free(chars); free(gch); free(cand); free(table);
                return set_error("symmetry group too large (more than %d elements; note: one wrong entry in a permutation makes the generators span nearly S_L)", LS_AMD_MAX_GROUP_ORDER);
            }
            if (order == cap) {
                cap *= 2;
                perms = (int *)realloc(perms, sizeof(int) * cap * L);
                chars = (double *)realloc(chars, sizeof(double) * 2 * cap);
            }
            memcpy(perms + (size_t)order * L, cand, sizeof(int) * L);
            chars[2 * order] = cre; chars[2 * order + 1] = cim;
            table[slot] = order;
            ++order;
            if ((size_t)order * 2 > tcap) { /* keep the table at most half full */
                tcap *= 2;
                table = (int32_t *)realloc(table, sizeof(int32_t) * tcap);
                for (size_t i = 0; i < tcap; ++i) table[i] = -1;
                for (int j = 0; j < order; ++j) {
                    size_t s2 = perm_hash(perms + (size_t)j * L, L) & (tcap - 1);
                    while (table[s2] >= 0) s2 = (s2 + 1) & (tcap - 1);
                    table[s2] = j;
                }
            }
        }
    }
    free(table);
    ext->order = order;
    ext->perms = perms;
    ext->elems = (lsk_group_elem *)malloc(sizeof(lsk_group_elem) * order);
    for (int j = 0; j < order; ++j) {
        double re = chars[2 * j], im = chars[2 * j + 1];
        if (fabs(im) < 1e-14) im = 0.0;
        if (fabs(re) < 1e-14) re = 0.0;
        compile_elem(perms + (size_t)j * L, L, re, im, ext->elems + j);
    }
    free(chars); free(gch); free(cand);
    return 0;
}

ls_hs_basis *ls_hs_create_spin_basis(int number_sites, int hamming_weight, int spin_inversion,
                                     int number_generators, int const *permutations,
                                     int const *sectors) {
    if (number_sites < 1 || number_sites > 64) { set_error("number_sites must be in [1, 64] (number_words == 1)"); return NULL; }
    if (hamming_weight > number_sites) { set_error("hamming_weight > number_sites"); return NULL; }
    if (hamming_weight >= LSK_BINOM_K) { set_error("hamming_weight too large for the binomial table"); return NULL; }
    if (spin_inversion != 0 && spin_inversion != 1 && spin_inversion != -1) { set_error("spin_inversion must be 0, 1 or -1"); return NULL; }
    if (spin_inversion != 0 && hamming_weight >= 0 && 2 * hamming_weight != number_sites) {
        set_error("spin inversion requires hamming_weight == number_sites / 2"); return NULL;
    }
    for (int g = 0; g < number_generators; ++g) {
        uint64_t seen = 0;
        for (int i = 0; i < number_sites; ++i) {
            int v = permutations[g * number_sites + i];
            if (v < 0 || v >= number_sites || ((seen >> v) & 1)) { set_error("generator %d is not a permutation", g); return NULL; }
            seen |= 1ULL << v;
        }
    }
    ls_hs_basis *b = (ls_hs_basis *)calloc(1, sizeof(ls_hs_basis));
    struct ls_amd_basis_ext *ext = (struct ls_amd_basis_ext *)calloc(1, sizeof(*ext));
    reg_put(b, ext, REG_BASIS);
    ext->refcount = 1;
    b->number_sites = number_sites;
    b->number_particles = -1;
    b->number_up = hamming_weight >= 0 ? hamming_weight : -1;
    b->particle_type = LS_HS_SPIN;
    b->spin_inversion = spin_inversion;
    b->kernels = NULL;
    ext->hamming_weight = hamming_weight < 0 ? -1 : hamming_weight;
    ext->nbits = number_sites;
    ext->n_generators = number_generators;
    ext->gen_perms = (int *)malloc(sizeof(int) * (size_t)(number_generators > 0 ? number_generators : 1) * number_sites);
    ext->gen_sectors = (int *)malloc(sizeof(int) * (size_t)(number_generators > 0 ? number_generators : 1));
    if (number_generators > 0) {
        memcpy(ext->gen_perms, permutations, sizeof(int) * (size_t)number_generators * number_sites);
        memcpy(ext->gen_sectors, sectors, sizeof(int) * (size_t)number_generators);
    }
    if (close_group(ext, number_sites) != 0) { ls_hs_destroy_basis(b); return NULL; }
    b->requires_projection = ext->order > 1 || spin_inversion != 0;
    b->state_index_is_identity = ext->hamming_weight < 0 && !b->requires_projection;
    return b;
}

/* FFI.chpl:143-144 (declared, commented out, in the reference).  Fermionic bases are unprojected: a basis state is a word of
 * occupation numbers, one bit per mode -- L modes for spinless fermions, 2 L for spinful ones (mode (i, up) = bit i, mode
 * (i, down) = bit i + L, as the reference's x = (xB << numberSites) | xA, StatesEnumeration.chpl:248-252).  Internally they are
 * spin bases over that many bits, except the spinful (N, N_up) basis, which is the product of two fixed-weight halves. */
ls_hs_basis *ls_hs_create_basis(ls_hs_particle_type particle_type, int number_sites, int number_particles, int number_up) {
    if (particle_type == LS_HS_SPIN) return ls_hs_create_spin_basis(number_sites, number_up, 0, 0, NULL, NULL);
    if (particle_type == LS_HS_SPINLESS_FERMION) {
        if (number_sites < 1 || number_sites > 64) { set_error("spinless fermions: number_sites must be in [1, 64]"); return NULL; }
        if (number_particles < -1 || number_particles > number_sites) { set_error("spinless fermions: number_particles must be in [0, number_sites] or -1"); return NULL; }
        if (number_up != -1) { set_error("spinless fermions have no number_up (pass -1)"); return NULL; }
        ls_hs_basis *b = ls_hs_create_spin_basis(number_sites, number_particles, 0, 0, NULL, NULL);
        if (!b) return NULL;
        b->particle_type = LS_HS_SPINLESS_FERMION;
        b->number_particles = number_particles;
        b->number_up = -1;
        return b;
    }
    if (particle_type != LS_HS_SPINFUL_FERMION) { set_error("unknown particle type %d", particle_type); return NULL; }
    if (number_sites < 1 || number_sites > 32) { set_error("spinful fermions: number_sites must be in [1, 32] (2 number_sites modes in one word)"); return NULL; }
    if (number_particles < -1 || number_particles > 2 * number_sites) { set_error("spinful fermions: number_particles must be in [0, 2 number_sites] or -1"); return NULL; }
    if (number_up != -1) {
        if (number_particles < 0) { set_error("spinful fermions: a fixed number_up needs a fixed number_particles"); return NULL; }
        if (number_up < 0 || number_up > number_sites || number_particles - number_up < 0 || number_particles - number_up > number_sites) {
            set_error("spinful fermions: need 0 <= number_up <= number_sites and 0 <= number_particles - number_up <= number_sites"); return NULL;
        }
    }
    ls_hs_basis *b = ls_hs_create_spin_basis(2 * number_sites, number_up == -1 ? number_particles : -1, 0, 0, NULL, NULL);
    if (!b) return NULL;
    struct ls_amd_basis_ext *e = BEXT(b);
    b->number_sites = number_sites;
    b->particle_type = LS_HS_SPINFUL_FERMION;
    b->number_particles = number_particles;
    b->number_up = number_up;
    if (number_up != -1) {
        e->product = 1;
        e->prod_up = number_up;
        e->prod_dn = number_particles - number_up;
        b->state_index_is_identity = false;
    }
    return b;
}

/* The sign table of a projected spinless-fermion basis: with q = p^-1 (q[j] = the position mode j goes to, (g.a)[i] = a[p_i]),
 * fsign[g][i] = { j < i : q[j] > q[i] }, so that sign(g, a) = parity(a & XOR_{i in occ(a)} fsign[g][i]) (include/ls_hs.h) */
static void fermi_sign_table(struct ls_amd_basis_ext *e, int L) {
    e->fsign = (uint64_t *)calloc((size_t)e->order * (size_t)L, sizeof(uint64_t));
    int q[64];
    for (int g = 0; g < e->order; ++g) {
        int const *p = e->perms + (size_t)g * L;
        for (int i = 0; i < L; ++i) q[p[i]] = i;
        for (int i = 0; i < L; ++i)
            for (int j = 0; j < i; ++j)
                if (q[j] > q[i]) e->fsign[(size_t)g * L + i] |= 1ULL << j;
    }
    e->fermi = 1;
}

ls_hs_basis *ls_hs_create_spinless_fermion_basis(int number_sites, int number_particles, int number_generators, int const *permutations,
                                                 int const *sectors) {
    if (number_sites < 1 || number_sites > 64) { set_error("spinless fermions: number_sites must be in [1, 64]"); return NULL; }
    if (number_particles < -1 || number_particles > number_sites) { set_error("spinless fermions: number_particles must be in [0, number_sites] or -1"); return NULL; }
    ls_hs_basis *b = ls_hs_create_spin_basis(number_sites, number_particles, 0, number_generators, permutations, sectors);
    if (!b) return NULL;
    b->particle_type = LS_HS_SPINLESS_FERMION;
    b->number_particles = number_particles;
    b->number_up = -1;
    struct ls_amd_basis_ext *e = BEXT(b);
    if (e->order > 1) fermi_sign_table(e, number_sites);
    return b;
}

/* A lifted ring element of a spinful basis gets its closed-form kind (LSK_ELEM_LIFT, lsk.h): p over 2 L modes is s + s, or s + s
 * followed by the half swap, with s a rotation or reflection of the L sites.  Everything else (tori, other lattices) keeps the
 * network that compile_elem built; so does every element under LS_AMD_FERMI_LIFT=0 (A/B of the closed forms against the table). */
static void classify_lifted_elem(int const *p, int L, lsk_group_elem *e) {
    int s[32];
    int const swap = p[0] >= L;
    for (int i = 0; i < L; ++i) {
        s[i] = p[i] - (swap ? L : 0);
        if (s[i] < 0 || s[i] >= L || p[i + L] != s[i] + (swap ? 0 : L)) return;
    }
    lsk_group_elem site;
    compile_elem(s, L, 0.0, 0.0, &site);
    if (site.kind != LSK_ELEM_ROT && site.kind != LSK_ELEM_REVROT) return;
    e->kind = LSK_ELEM_LIFT | (site.kind == LSK_ELEM_REVROT ? LSK_ELEM_LIFT_REV : 0) | (swap ? LSK_ELEM_LIFT_SWAP : 0);
    e->k = site.k;
}

/* Spinful fermions with fixed (N_up, N_down) and site permutations (include/ls_hs.h): the product basis of ls_hs_create_basis with
 * the group closed over the 2 L modes -- every site generator lifted as p + p, the up <-> down flip as the half swap i <-> i + L --
 * and the sign table of those mode permutations.  The prefix keeps spin_inversion == 0 (that field means the bit complement). */
ls_hs_basis *ls_hs_create_spinful_fermion_basis(int number_sites, int number_particles, int number_up, int spin_flip, int number_generators,
                                                int const *permutations, int const *sectors) {
    if (number_up == -1) { set_error("spinful fermions with symmetries need a fixed number_up (the (N, N_up) product basis)"); return NULL; }
    if (spin_flip != 0 && spin_flip != 1 && spin_flip != -1) { set_error("spin_flip must be 0, 1 or -1"); return NULL; }
    if (number_generators < 0 || (number_generators > 0 && (!permutations || !sectors))) { set_error("spinful fermions: bad generators"); return NULL; }
    if (number_sites >= 1 && number_sites <= 32)
        for (int g = 0; g < number_generators; ++g) {
            uint64_t seen = 0;
            for (int i = 0; i < number_sites; ++i) {
                int v = permutations[g * number_sites + i];
                if (v < 0 || v >= number_sites || ((seen >> v) & 1)) { set_error("generator %d is not a permutation", g); return NULL; }
                seen |= 1ULL << v;
            }
        }
    ls_hs_basis *b = ls_hs_create_basis(LS_HS_SPINFUL_FERMION, number_sites, number_particles, number_up);
    if (!b) return NULL;
    if (spin_flip != 0 && 2 * number_up != number_particles) {
        ls_hs_destroy_basis(b);
        set_error("spin_flip requires number_up == number_particles - number_up");
        return NULL;
    }
    struct ls_amd_basis_ext *e = BEXT(b);
    int const L = number_sites, M = 2 * L, ng = number_generators + (spin_flip != 0 ? 1 : 0);
    e->spin_flip = spin_flip;
    if (ng == 0) return b;
    free(e->gen_perms); free(e->gen_sectors); free(e->perms); free(e->elems);
    e->perms = NULL; e->elems = NULL;
    e->n_generators = ng;
    e->gen_perms = (int *)malloc(sizeof(int) * (size_t)ng * M);
    e->gen_sectors = (int *)malloc(sizeof(int) * (size_t)ng);
    for (int g = 0; g < number_generators; ++g) {
        for (int i = 0; i < L; ++i) {
            e->gen_perms[(size_t)g * M + i] = permutations[g * L + i];
            e->gen_perms[(size_t)g * M + L + i] = permutations[g * L + i] + L;
        }
        e->gen_sectors[g] = sectors[g];
    }
    if (spin_flip != 0) {
        for (int i = 0; i < L; ++i) { e->gen_perms[(size_t)(ng - 1) * M + i] = i + L; e->gen_perms[(size_t)(ng - 1) * M + L + i] = i; }
        e->gen_sectors[ng - 1] = spin_flip > 0 ? 0 : 1; /* an element of order 2: sector 0 = character +1, 1 = -1 */
    }
    if (close_group(e, M) != 0) { ls_hs_destroy_basis(b); return NULL; }
    b->requires_projection = e->order > 1;
    if (e->order > 1) {
        char const *env = getenv("LS_AMD_FERMI_LIFT");
        if (!(env && atoi(env) == 0))
            for (int g = 0; g < e->order; ++g) classify_lifted_elem(e->perms + (size_t)g * M, L, e->elems + g);
        fermi_sign_table(e, M);
    }
    return b;
}
/* the site generators of such a basis, read back off the lifted ones (clone) */
static ls_hs_basis *clone_spinful_projected(ls_hs_basis const *basis) {
    struct ls_amd_basis_ext const *e = BEXT(basis);
    int const L = basis->number_sites, ng = e->n_generators - (e->spin_flip != 0 ? 1 : 0);
    int *perms = (int *)malloc(sizeof(int) * (size_t)(ng > 0 ? ng : 1) * L);
    for (int g = 0; g < ng; ++g)
        for (int i = 0; i < L; ++i) perms[g * L + i] = e->gen_perms[(size_t)g * 2 * L + i];
    ls_hs_basis *b = ls_hs_create_spinful_fermion_basis(L, basis->number_particles, basis->number_up, e->spin_flip, ng, perms, e->gen_sectors);
    free(perms);
    return b;
}

ls_hs_basis *ls_hs_clone_basis(ls_hs_basis const *basis) {
    struct ls_amd_basis_ext const *e = BEXT(basis);
    ls_hs_basis *b = basis->particle_type == LS_HS_SPINFUL_FERMION && (e->n_generators > 0 || e->spin_flip != 0)
                         ? clone_spinful_projected(basis)
                     : basis->particle_type == LS_HS_SPINLESS_FERMION
                         ? ls_hs_create_spinless_fermion_basis(basis->number_sites, basis->number_particles, e->n_generators, e->gen_perms,
                                                               e->gen_sectors)
                     : basis->particle_type != LS_HS_SPIN
                         ? ls_hs_create_basis(basis->particle_type, basis->number_sites, basis->number_particles, basis->number_up)
                         : ls_hs_create_spin_basis(basis->number_sites, e->hamming_weight, basis->spin_inversion,
                                                   e->n_generators, e->gen_perms, e->gen_sectors);
    if (!b) return NULL;
    if (basis->representatives.elts) { /* deep copy, like upstream's clone keeps the built states */
        size_t bytes = 8 * basis->representatives.num_elts;
        b->representatives.elts = malloc(bytes ? bytes : 8);
        memcpy(b->representatives.elts, basis->representatives.elts, bytes);
        b->representatives.num_elts = basis->representatives.num_elts;
        b->representatives.freer = (void *)free;
        BEXT(b)->owns_representatives = 1;
    }
    return b;
}

#define HOST_PLAN_SLOTS ((int)(sizeof(((struct ls_amd_basis_ext *)0)->host_plans) / sizeof(struct host_plan_slot)))
static void host_plan_slot_drop(struct host_plan_slot *sl) {
    if (sl->plan) ls_amd_plan_destroy((ls_amd_plan *)sl->plan);
    if (sl->dist) ls_amd_dist_destroy((ls_amd_dist *)sl->dist);
    for (int i = 0; i < 2; ++i) { if (sl->d_x[i]) lsk_free(sl->d_x[i]); if (sl->d_y[i]) lsk_free(sl->d_y[i]); }
    memset(sl, 0, sizeof(*sl));
}
/* Forget the cached plans of one operator (op != NULL), of one communicator (comm != NULL), or all of them.  The slots are
 * DETACHED under the registry lock -- a basis cannot disappear, and no second thread can pick the same slot, while they are
 * read -- and destroyed after it is released (destroying a plan takes that lock again). */
static int detach_host_plans_locked(struct ls_amd_basis_ext *e, ls_hs_operator const *op, void const *comm,
                                    struct host_plan_slot *out, int n, int cap) {
    for (int i = 0; i < HOST_PLAN_SLOTS && n < cap; ++i) {
        struct host_plan_slot *sl = &e->host_plans[i];
        if (!sl->op) continue;
        if ((op && sl->op != op) || (comm && sl->comm != comm)) continue;
        out[n++] = *sl;
        memset(sl, 0, sizeof(*sl));
    }
    return n;
}
static void basis_drop_host_plans(struct ls_amd_basis_ext *e, ls_hs_operator const *op, void const *comm) {
    struct host_plan_slot dropped[HOST_PLAN_SLOTS];
    pthread_mutex_lock(&g_reg_lock);
    int const n = detach_host_plans_locked(e, op, comm, dropped, 0, HOST_PLAN_SLOTS);
    pthread_mutex_unlock(&g_reg_lock);
    for (int i = 0; i < n; ++i) host_plan_slot_drop(&dropped[i]);
}
/* a communicator is going away (ls_amd_comm_destroy, dist.c): no cached ls_amd_dist may keep pointing at it */
void ls_amd_internal_forget_comm(void const *comm) {
    pthread_mutex_lock(&g_reg_lock);
    size_t bases = 0;
    for (size_t i = 0; i < g_reg_cap; ++i)
        if (g_reg[i].key && g_reg[i].key != REG_TOMB && g_reg[i].kind == REG_BASIS) ++bases;
    int const cap = (int)(bases ? bases : 1) * HOST_PLAN_SLOTS;
    struct host_plan_slot *dropped = (struct host_plan_slot *)calloc((size_t)cap, sizeof(*dropped));
    int n = 0;
    for (size_t i = 0; i < g_reg_cap; ++i)
        if (g_reg[i].key && g_reg[i].key != REG_TOMB && g_reg[i].kind == REG_BASIS)
            n = detach_host_plans_locked((struct ls_amd_basis_ext *)g_reg[i].val, NULL, comm, dropped, n, cap);
    pthread_mutex_unlock(&g_reg_lock);
    for (int i = 0; i < n; ++i) host_plan_slot_drop(&dropped[i]);
    free(dropped);
}

static void basis_drop_device_caches(ls_hs_basis *b) {
    struct ls_amd_basis_ext *e = BEXT(b);
    basis_drop_host_plans(e, NULL, NULL);
    if (e->d_reps_cache) { lsk_free(e->d_reps_cache); e->d_reps_cache = NULL; e->d_reps_count = 0; }
    if (e->d_index_table) { lsk_free(e->d_index_table); e->d_index_table = NULL; }
    e->index_kind = -1;
}

void ls_hs_destroy_basis(ls_hs_basis *b) {
    if (!b) return;
    struct ls_amd_basis_ext *e = (struct ls_amd_basis_ext *)reg_get(b);
    if (!e) return; /* not ours (or already gone): leave the struct alone */
    /* (atomic: threads that clone / destroy operators of one basis -- the reference's tasks do -- must not lose a count) */
    if (__atomic_sub_fetch(&e->refcount, 1, __ATOMIC_ACQ_REL) > 0) return; /* operators built on this basis still share it */
    basis_drop_device_caches(b);
    if (e->d_elems) lsk_free(e->d_elems);
    if (e->d_cosets) lsk_free(e->d_cosets);
    if (e->d_trow) lsk_free(e->d_trow);
    if (e->d_d4_net) lsk_free(e->d_d4_net);
    if (e->d_trow2) lsk_free(e->d_trow2);
    if (e->d_fsign) lsk_free(e->d_fsign);
    if (e->owns_representatives && b->representatives.elts) free(b->representatives.elts);
    free(e->gen_perms); free(e->gen_sectors); free(e->perms); free(e->elems); free(e->coset_ids); free(e->fsign);
    reg_del(b);
    int const adopted = e->adopted;
    free(e);
    if (!adopted) free(b);
}

uint64_t ls_hs_min_state_estimate(ls_hs_basis const *b) {
    struct ls_amd_basis_ext const *e = BEXT(b);
    if (e->product) return (((1ULL << e->prod_dn) - 1) << b->number_sites) | ((1ULL << e->prod_up) - 1);
    int h = e->hamming_weight;
    return h > 0 ? ((1ULL << h) - 1) : 0;
}
/* with spin inversion the highest admissible state has the top site bit clear (see oracle notes) */
uint64_t ls_hs_max_state_estimate(ls_hs_basis const *b) {
    struct ls_amd_basis_ext const *e = BEXT(b);
    if (e->product) { /* (weights <= L <= 32; an empty half contributes nothing and is not shifted: 2 L - 0 may be 64) */
        int const L = b->number_sites;
        uint64_t const dn = e->prod_dn ? ((1ULL << e->prod_dn) - 1) << (2 * L - e->prod_dn) : 0;
        uint64_t const up = e->prod_up ? ((1ULL << e->prod_up) - 1) << (L - e->prod_up) : 0;
        return dn | up;
    }
    int const L = NBITS(b) - (b->spin_inversion != 0 ? 1 : 0);
    int h = e->hamming_weight;
    if (h >= 0) return h == 0 ? 0 : ((1ULL << h) - 1) << (L - h);
    return L >= 64 ? ~0ULL : ((1ULL << L) - 1);
}
/* 2 number_sites for spinful fermions; read off the prefix alone, like the reference, for structs nobody registered */
int ls_hs_basis_number_bits(ls_hs_basis const *b) { return b->number_sites * (b->particle_type == LS_HS_SPINFUL_FERMION ? 2 : 1); }
int ls_hs_basis_number_words(ls_hs_basis const *b) { return (ls_hs_basis_number_bits(b) + 63) / 64; }
bool ls_hs_basis_has_fixed_hamming_weight(ls_hs_basis const *b) { return BEXT(b)->hamming_weight >= 0; }
bool ls_hs_basis_has_spin_inversion_symmetry(ls_hs_basis const *b) { return b->spin_inversion != 0; }
bool ls_hs_basis_has_permutation_symmetries(ls_hs_basis const *b) { return BEXT(b)->order > 1; }
bool ls_hs_basis_requires_projection(ls_hs_basis const *b) { return b->requires_projection; }

void ls_hs_unchecked_set_representatives(ls_hs_basis *b, chpl_external_array const *states) {
    basis_drop_device_caches(b);
    if (BEXT(b)->owns_representatives && b->representatives.elts) free(b->representatives.elts);
    b->representatives = *states;
    BEXT(b)->owns_representatives = 0;
}

int ls_amd_basis_group_order(ls_hs_basis const *b) { return BEXT(b)->order; }
int ls_amd_basis_fermion_signs(ls_hs_basis const *b) { return BEXT(b)->fermi; }
int ls_amd_basis_spin_flip(ls_hs_basis const *b) { return BEXT(b)->spin_flip; }
/* test hook: how element `element` was compiled (LSK_ELEM_* of lsk.h: 0 network, 1 rotation, 2 reflection, 4-7 lifted ring elements) */
int ls_amd_test_group_element_kind(ls_hs_basis const *b, int element) {
    struct ls_amd_basis_ext const *e = BEXT(b);
    return element < 0 || element >= e->order ? -1 : e->elems[element].kind;
}
/* test hook (no device): sign(g, state) of group element `element` of a projected fermionic basis by the device code's host
 * mirror -- closed form for rotations and reflections, or (table != 0) the sign table for every element; 0 on bad arguments */
int ls_amd_test_fermion_sign(ls_hs_basis const *b, int element, uint64_t state, int table) {
    struct ls_amd_basis_ext const *e = BEXT(b);
    if (!e->fermi || element < 0 || element >= e->order) return 0;
    return lsk_test_fermi_parity(e->elems[element], e->fsign + (size_t)element * NBITS(b), state, NBITS(b), table) ? -1 : 1;
}
uint64_t ls_amd_basis_apply_group_element(ls_hs_basis const *b, int element, uint64_t state) {
    return host_apply_elem(BEXT(b)->elems + element, state, NBITS(b));
}
int ls_amd_basis_group_character(ls_hs_basis const *b, int element, double *re, double *im) {
    if (element < 0 || element >= BEXT(b)->order) return set_error("element out of range");
    *re = BEXT(b)->elems[element].ch_re;
    *im = BEXT(b)->elems[element].ch_im;
    return 0;
}

static pthread_mutex_t g_device_tables_lock = PTHREAD_MUTEX_INITIALIZER;
/* Looks for the translation subgroup of a lattice group (K4 mode 4).  Every element is taken by its ACTION on the one-hot
 * states (img[g][s] = position of the bit of g(1 << s)), so no convention about permutation arrays enters: t is a translation
 * of the w x h torus (s = y w + x) when img_t[s] = ((y + dy) % h) w + (x + dx) % w; the subgroup qualifies when all w h of them
 * are in the group.  Then one element of every right coset T g is kept (t o g covers the coset: img_{t o g}[s] = img_t[img_g[s]]).
 * Sets e->tw (-1: none), e->n_cosets, e->coset_ids. */
static void find_translation_cosets(struct ls_amd_basis_ext *e, int L) {
    e->tw = -1;
    int const order = e->order;
    if (order < 4 || order > 8192 || L < 4) return;
    unsigned char *img = (unsigned char *)malloc((size_t)order * (size_t)L);
    for (int g = 0; g < order; ++g)
        for (int s = 0; s < L; ++s) img[(size_t)g * L + s] = (unsigned char)__builtin_ctzll(host_apply_elem(&e->elems[g], 1ULL << s, L));
    /* index of an action among the group's (open addressing over an FNV hash) */
    int cap = 1;
    while (cap < 4 * order) cap *= 2;
    int *table = (int *)malloc(sizeof(int) * (size_t)cap);
    for (int i = 0; i < cap; ++i) table[i] = -1;
#define IMG_HASH(ptr, out_h) do { uint64_t h_ = 1469598103934665603ULL; for (int s_ = 0; s_ < L; ++s_) { h_ ^= (ptr)[s_]; h_ *= 1099511628211ULL; } (out_h) = (int)(h_ & (uint64_t)(cap - 1)); } while (0)
    for (int g = 0; g < order; ++g) {
        int h;
        IMG_HASH(img + (size_t)g * L, h);
        while (table[h] >= 0) h = (h + 1) & (cap - 1);
        table[h] = g;
    }
    unsigned char *cand = (unsigned char *)malloc((size_t)L);
    int *trans = (int *)malloc(sizeof(int) * (size_t)L);
    int best_w = -1;
    for (int w = 2; w <= L / 2 && best_w < 0; ++w) {
        if (L % w) continue;
        int const hgt = L / w;
        int found = 0;
        for (int dy = 0; dy < hgt; ++dy)
            for (int dx = 0; dx < w; ++dx) {
                for (int s = 0; s < L; ++s) cand[s] = (unsigned char)((((s / w) + dy) % hgt) * w + ((s % w) + dx) % w);
                int h, id = -1;
                IMG_HASH(cand, h);
                while (table[h] >= 0) {
                    if (memcmp(img + (size_t)table[h] * L, cand, (size_t)L) == 0) { id = table[h]; break; }
                    h = (h + 1) & (cap - 1);
                }
                if (id >= 0) trans[found++] = id;
            }
        if (found == L) best_w = w;
    }
    if (best_w > 0) {
        unsigned char *covered = (unsigned char *)calloc((size_t)order, 1);
        int *ids = (int *)malloc(sizeof(int) * (size_t)order);
        int nc = 0, ok = 1;
        for (int g = 0; g < order && ok; ++g) {
            if (covered[g]) continue;
            ids[nc++] = g;
            for (int t = 0; t < L && ok; ++t) {
                unsigned char const *it = img + (size_t)trans[t] * L, *ig = img + (size_t)g * L;
                for (int s = 0; s < L; ++s) cand[s] = it[ig[s]];
                int h, id = -1;
                IMG_HASH(cand, h);
                while (table[h] >= 0) {
                    if (memcmp(img + (size_t)table[h] * L, cand, (size_t)L) == 0) { id = table[h]; break; }
                    h = (h + 1) & (cap - 1);
                }
                if (id < 0) ok = 0; /* not closed: cannot happen for a group; be safe */
                else covered[id] = 1;
            }
        }
        if (ok && nc * L == order) {
            e->tw = best_w;
            e->n_cosets = nc;
            e->coset_ids = (int *)malloc(sizeof(int) * (size_t)nc);
            memcpy(e->coset_ids, ids, sizeof(int) * (size_t)nc);
        }
        free(covered); free(ids);
    }
#undef IMG_HASH
    free(img); free(table); free(cand); free(trans);
}

/* K4 mode 5: are the cosets T g found above the point group of the torus itself?  Canonical images of a site (y, x): r = (y, tw-1-x),
 * o = (th-1-y, x), and on a square torus the transpose (x, y) applied first; a coset matches the canonical element c when
 * img_g = img_t o img_c for some translation t.  Every coset must match a different c.  Sets e->d4_mask (> 0, or -1). */
static void classify_d4_cosets(struct ls_amd_basis_ext *e, int L) {
    e->d4_mask = -1;
    int const tw = e->tw;
    if (tw <= 0 || tw > 8 || L % tw || e->n_cosets < 1 || e->n_cosets > 8) return;
    int const th = L / tw;
    int mask = 0;
    for (int r = 0; r < e->n_cosets; ++r) {
        unsigned char ig[64];
        for (int s = 0; s < L; ++s) ig[s] = (unsigned char)__builtin_ctzll(host_apply_elem(&e->elems[e->coset_ids[r]], 1ULL << s, L));
        int found = -1;
        for (int c = 0; c < 8 && found < 0; ++c) {
            if ((c & 4) && tw != th) continue;
            for (int dy = 0; dy < th && found < 0; ++dy)
                for (int dx = 0; dx < tw && found < 0; ++dx) {
                    int ok = 1;
                    for (int s = 0; s < L && ok; ++s) {
                        int y = s / tw, x = s % tw;
                        if (c & 4) { int const t = y; y = x; x = t; } /* transpose first */
                        if (c & 1) x = tw - 1 - x;                     /* r */
                        if (c & 2) y = th - 1 - y;                     /* o */
                        ok = ig[s] == ((y + dy) % th) * tw + (x + dx) % tw;
                    }
                    if (ok) found = c;
                }
        }
        if (found < 0 || (mask >> found) & 1) return;
        mask |= 1 << found;
    }
    if (!(mask & 1)) return; /* (the coset of the identity is always there) */
    if (mask >> 4) { /* the transpose as a compiled network: y[i] = x[perm[i]], an involution */
        int perm[64];
        for (int s = 0; s < L; ++s) perm[s] = (s % tw) * tw + s / tw;
        compile_elem(perm, L, 1.0, 0.0, &e->d4_transpose);
    }
    e->d4_mask = mask;
}
int ls_amd_test_d4_mask(ls_hs_basis const *b) {
    struct ls_amd_basis_ext *e = BEXT(b);
    if (ls_amd_test_translation_cosets(b, NULL) <= 0) return 0;
    pthread_mutex_lock(&g_device_tables_lock);
    if (e->d4_mask == 0) classify_d4_cosets(e, NBITS(b));
    pthread_mutex_unlock(&g_device_tables_lock);
    return e->d4_mask > 0 ? e->d4_mask : 0;
}

/* host-only test hooks of K4 mode 4: the shape found for a basis (returns tw, or -1), and the orbit minimum of `state` computed
 * the way the kernels do it (coset networks + row / word rotations; the global spin flip folded in by canonicalising to "top
 * site clear" when the basis has one) */
int ls_amd_test_translation_cosets(ls_hs_basis const *b, int *n_cosets) {
    struct ls_amd_basis_ext *e = BEXT(b);
    pthread_mutex_lock(&g_device_tables_lock);
    if (e->tw == 0) find_translation_cosets(e, NBITS(b));
    pthread_mutex_unlock(&g_device_tables_lock);
    if (n_cosets) *n_cosets = e->tw > 0 ? e->n_cosets : 0;
    return e->tw;
}
uint64_t ls_amd_test_rep_by_cosets(ls_hs_basis const *b, uint64_t a) {
    struct ls_amd_basis_ext *e = BEXT(b);
    int const L = NBITS(b);
    if (ls_amd_test_translation_cosets(b, NULL) <= 0) return ~0ULL;
    uint64_t const mask = L >= 64 ? ~0ULL : ((1ULL << L) - 1);
    int const tw = e->tw, th = L / tw;
    uint64_t col0 = 0, best = ~0ULL;
    for (int y = 0; y < th; ++y) col0 |= 1ULL << (y * tw);
    char const *k4env = getenv("LS_AMD_K4");
    int const d4 = (k4env && strcmp(k4env, "cosets") == 0) ? 0 : ls_amd_test_d4_mask(b);
    if (d4 > 0) { /* what the kernels run (mode 5): one transpose network, the rest factorised */
        uint64_t rowtab2[256];
        lsk_torus_rowtab2(tw, rowtab2);
        best = lsk_test_torus_min_d2(a, L, tw, b->spin_inversion != 0, d4 & 15, rowtab2, best);
        if (d4 >> 4) best = lsk_test_torus_min_d2(host_apply_elem(&e->d4_transpose, a, L), L, tw, b->spin_inversion != 0, d4 >> 4, rowtab2, best);
        return best;
    }
    if (tw <= 8) { /* mode 4: the row table picks the translations that can be minimal */
        uint32_t rowtab[256];
        lsk_torus_rowtab(tw, rowtab);
        for (int r = 0; r < e->n_cosets; ++r)
            best = lsk_test_torus_min(host_apply_elem(&e->elems[e->coset_ids[r]], a, L), L, tw, b->spin_inversion != 0, rowtab, best);
        return best;
    }
    for (int r = 0; r < e->n_cosets; ++r) {
        uint64_t v = host_apply_elem(&e->elems[e->coset_ids[r]], a, L);
        for (int j = 0; j < th; ++j) {
            for (int i = 0; i < tw; ++i) {
                uint64_t c = v;
                if (b->spin_inversion != 0 && ((v >> (L - 1)) & 1)) c = v ^ mask;
                if (c < best) best = c;
                v = ((v << 1) & ~col0 & mask) | ((v >> (tw - 1)) & col0);
            }
            v = ((v << tw) | (v >> (L - tw))) & mask;
        }
    }
    return best;
}

static int basis_device_unlocked(ls_hs_basis const *b, lsk_basis *out) {
    struct ls_amd_basis_ext *e = BEXT(b);
    if (!e->d_elems) {
        void *p;
        DEV(lsk_malloc(&p, sizeof(lsk_group_elem) * e->order));
        DEV(lsk_h2d(p, e->elems, sizeof(lsk_group_elem) * e->order));
        e->d_elems = (lsk_group_elem *)p;
    }
    out->number_sites = NBITS(b);
    out->hamming_weight = e->hamming_weight;
    out->spin_inversion = b->spin_inversion;
    out->n_elems = e->order;
    out->proj = e->order > 1 ? LSK_PROJ_FULL : (b->spin_inversion != 0 ? LSK_PROJ_INVERSION : LSK_PROJ_NONE);
    out->site_mask = NBITS(b) >= 64 ? ~0ULL : ((1ULL << NBITS(b)) - 1);
    out->inv_order = 1.0 / ((double)e->order * (b->spin_inversion != 0 ? 2.0 : 1.0));
    out->elems = e->d_elems;
    out->chars_pm1 = 1;
    int trivial = b->spin_inversion >= 0;
    for (int g = 0; g < e->order; ++g) {
        if (e->elems[g].ch_im != 0.0 || fabs(e->elems[g].ch_re) != 1.0) out->chars_pm1 = 0;
        if (e->elems[g].ch_im != 0.0 || e->elems[g].ch_re != 1.0) trivial = 0;
    }
    out->k4_mode = 0;
    out->reflect = 0;
    out->debug_ablate = lsk_ablate_mask(); /* 0 in the shipped library; LS_AMD_ABLATE in profiling builds (make ablate) */
    out->tw = out->n_cosets = 0;
    out->tcol0 = 0;
    out->cosets = NULL;
    out->trow = NULL;
    out->d4_mask = 0;
    out->trow2 = NULL;
    out->fermi = e->fermi;
    if (e->fermi) {
        /* signed characters: the norm of an orbit can vanish in any sector, so never a mode that assumes it does not (modes 1-5 only
         * deliver the orbit minimum) -- the element loop of mode 0, with the sign table in place of mode 5's row table */
        if (!e->d_fsign) {
            size_t const bytes = sizeof(uint64_t) * (size_t)e->order * (size_t)NBITS(b);
            void *p = NULL;
            if (lsk_malloc(&p, bytes) != 0 || lsk_h2d(p, e->fsign, bytes) != 0) { if (p) lsk_free(p); return dev_error(); }
            e->d_fsign = (uint64_t *)p;
        }
        out->fsign = e->d_fsign;
        return 0;
    }
    /* LS_AMD_K4 (test hook): general = the element loop with characters and norms even in trivial sectors; brute = trivial
     * sectors by the plain loop over every element (no run pruning, no translation cosets) */
    char const *k4env = getenv("LS_AMD_K4");
    int const k4_general = k4env && strcmp(k4env, "general") == 0, k4_brute = k4env && strcmp(k4env, "brute") == 0;
    int const k4_cosets = k4env && strcmp(k4env, "cosets") == 0; /* keep mode 4 (one network per coset) where mode 5 applies: A/B */
    if (trivial && e->order > 1 && !k4_general) {
        out->k4_mode = 1;
        /* full cyclic group of the ring (every rotation k = 0..L-1), optionally with all reflections? */
        int const L = NBITS(b);
        uint64_t rot = 0, rev = 0;
        int other = 0;
        for (int g = 0; g < e->order; ++g) {
            if (e->elems[g].kind == LSK_ELEM_ROT) rot |= 1ULL << e->elems[g].k;
            else if (e->elems[g].kind == LSK_ELEM_REVROT) rev |= 1ULL << e->elems[g].k;
            else other = 1;
        }
        uint64_t const full = L >= 64 ? ~0ULL : ((1ULL << L) - 1);
        if (!other && rot == full && (rev == 0 || rev == full) && e->order == L * (rev ? 2 : 1) && L >= 3) {
            out->k4_mode = k4_brute ? 2 : 3; /* 3: longest-zero-run candidate pruning */
            out->reflect = rev ? 1 : 0;
        } else if (!k4_brute) {
            /* a lattice group: its translation subgroup is walked with cheap bit operations, only the coset representatives
             * (the point group) go through compiled networks */
            if (e->tw == 0) find_translation_cosets(e, L);
            if (e->tw > 0) {
                if (!e->d_cosets) {
                    lsk_group_elem *tmp = (lsk_group_elem *)malloc(sizeof(lsk_group_elem) * (size_t)e->n_cosets);
                    for (int r = 0; r < e->n_cosets; ++r) tmp[r] = e->elems[e->coset_ids[r]];
                    void *p = NULL;
                    int const bad = lsk_malloc(&p, sizeof(lsk_group_elem) * (size_t)e->n_cosets) != 0 ||
                                    lsk_h2d(p, tmp, sizeof(lsk_group_elem) * (size_t)e->n_cosets) != 0;
                    free(tmp);
                    if (bad) { if (p) lsk_free(p); return dev_error(); }
                    e->d_cosets = (lsk_group_elem *)p;
                }
                if (!e->d_trow && e->tw <= 8) {
                    uint32_t rowtab[256];
                    void *p = NULL;
                    lsk_torus_rowtab(e->tw, rowtab);
                    if (lsk_malloc(&p, sizeof(rowtab)) != 0 || lsk_h2d(p, rowtab, sizeof(uint32_t) << e->tw) != 0) { if (p) lsk_free(p); return dev_error(); }
                    e->d_trow = (uint32_t *)p;
                }
                out->trow = e->d_trow;
                out->k4_mode = 4;
                out->tw = e->tw;
                out->n_cosets = e->n_cosets;
                out->cosets = e->d_cosets;
                for (int y = 0; y < L / e->tw; ++y) out->tcol0 |= 1ULL << (y * e->tw);
                /* mode 5: the cosets are the point group of the torus -- one network (the transpose) instead of n_cosets */
                if (e->d4_mask == 0) classify_d4_cosets(e, L);
                if (e->d4_mask > 0 && !k4_cosets) {
                    if (!e->d_trow2) {
                        uint64_t rowtab2[256];
                        void *p = NULL;
                        lsk_torus_rowtab2(e->tw, rowtab2);
                        if (lsk_malloc(&p, sizeof(rowtab2)) != 0 || lsk_h2d(p, rowtab2, sizeof(uint64_t) << e->tw) != 0) { if (p) lsk_free(p); return dev_error(); }
                        e->d_trow2 = (uint64_t *)p;
                    }
                    if ((e->d4_mask >> 4) && !e->d_d4_net) {
                        void *p = NULL;
                        if (lsk_malloc(&p, sizeof(lsk_group_elem)) != 0 || lsk_h2d(p, &e->d4_transpose, sizeof(lsk_group_elem)) != 0) { if (p) lsk_free(p); return dev_error(); }
                        e->d_d4_net = (lsk_group_elem *)p;
                    }
                    out->k4_mode = 5;
                    out->d4_mask = e->d4_mask;
                    out->trow2 = e->d_trow2;
                    out->cosets = e->d_d4_net; /* NULL when no image involves the transpose */
                    out->n_cosets = e->d_d4_net ? 1 : 0;
                }
            }
        }
    }
    return 0;
}

/* ============================================================================================ */
/* operator                                                                                     */
/* ============================================================================================ */
struct ls_amd_operator_ext {
    int n_groups;
    lsk_group *groups; /* host */
    lsk_term *off;     /* host, grouped */
    lsk_term *diag;    /* host */
    int n_off, n_diag;
    int is_real, is_hermitian;
    lsk_runs runs;
    /* device mirrors */
    lsk_group *d_groups;
    lsk_term *d_off, *d_diag;
    int adopted; /* foreign struct (ls_amd_adopt_operator): only the side tables are ours */
};

static struct ls_amd_operator_ext g_dummy_operator_ext;
static struct ls_amd_operator_ext *operator_ext_of(ls_hs_operator const *op) {
    struct ls_amd_operator_ext *e = (struct ls_amd_operator_ext *)reg_get(op);
    if (!e) {
        halt_with("ls_hs_operator %p was not created by this library: register it with ls_amd_adopt_operator first", (void const *)op);
        return &g_dummy_operator_ext;
    }
    return e;
}

typedef struct { double re, im; uint64_t m, r, x, s; } raw_term;

static int raw_cmp(void const *pa, void const *pb) {
    raw_term const *a = (raw_term const *)pa, *b = (raw_term const *)pb;
    if (a->x != b->x) return a->x < b->x ? -1 : 1;
    if (a->m != b->m) return a->m < b->m ? -1 : 1;
    if (a->r != b->r) return a->r < b->r ? -1 : 1;
    if (a->s != b->s) return a->s < b->s ? -1 : 1;
    return 0;
}

static void eval_terms(lsk_term const *t, int b, int e, uint64_t a, double *re, double *im) {
    double cr = 0, ci = 0;
    for (int k = b; k < e; ++k)
        if ((a & t[k].m) == t[k].r) {
            int neg = __builtin_popcountll(a & t[k].s) & 1;
            cr += neg ? -t[k].v_re : t[k].v_re;
            ci += neg ? -t[k].v_im : t[k].v_im;
        }
    *re = cr; *im = ci;
}

static uint64_t deposit_bits(uint64_t pattern, uint64_t support) { /* software pdep */
    uint64_t out = 0;
    for (int i = 0; support; ++i) {
        uint64_t low = support & -support;
        if ((pattern >> i) & 1) out |= low;
        support ^= low;
    }
    return out;
}

static void classify_groups(struct ls_amd_operator_ext *ext) {
    ext->is_hermitian = 1;
    /* diagonal must be real for a Hermitian operator */
    for (int k = 0; k < ext->n_diag; ++k) if (ext->diag[k].v_im != 0.0) ext->is_hermitian = 0;
    for (int g = 0; g < ext->n_groups; ++g) {
        lsk_group *G = &ext->groups[g];
        uint64_t support = G->x;
        for (int k = G->begin; k < G->end; ++k) support |= ext->off[k].m | ext->off[k].s;
        int nb = __builtin_popcountll(support);
        G->adj = -1;
        if (__builtin_popcountll(G->x) == 2) {
            int lo = __builtin_ctzll(G->x);
            if (G->x == (3ULL << lo)) G->adj = lo;
        }
        G->fast = LSK_GROUP_GENERIC;
        G->v_re = G->v_im = 0.0;
        if (nb <= 16) {
            /* exact truth table over the support */
            int herm = 1;
            for (uint64_t pat = 0; pat < (1ULL << nb); ++pat) {
                uint64_t a = deposit_bits(pat, support);
                double fr, fi, gr, gi;
                eval_terms(ext->off, G->begin, G->end, a, &fr, &fi);
                eval_terms(ext->off, G->begin, G->end, a ^ G->x, &gr, &gi);
                if (fabs(gr - fr) > 1e-12 * (1 + fabs(fr)) || fabs(gi + fi) > 1e-12 * (1 + fabs(fi))) herm = 0;
            }
            if (!herm) ext->is_hermitian = 0;
            if (nb == 2 && support == G->x) {
                uint64_t b0 = G->x & -G->x, b1 = G->x ^ b0;
                double f00r, f00i, f01r, f01i, f10r, f10i, f11r, f11i;
                eval_terms(ext->off, G->begin, G->end, 0, &f00r, &f00i);
                eval_terms(ext->off, G->begin, G->end, b0, &f01r, &f01i);
                eval_terms(ext->off, G->begin, G->end, b1, &f10r, &f10i);
                eval_terms(ext->off, G->begin, G->end, b0 | b1, &f11r, &f11i);
                if (f00r == 0 && f00i == 0 && f11r == 0 && f11i == 0 && f01r == f10r && f01i == f10i) {
                    G->fast = LSK_GROUP_EXCHANGE;
                    G->v_re = f01r;
                    G->v_im = f01i;
                } else if (f00r == 0 && f00i == 0 && f11r == 0 && f11i == 0 && ((f01r == 0 && f01i == 0) != (f10r == 0 && f10i == 0))) {
                    /* a directed pair (sigma^+ sigma^-): one of the two patterns alone is a source */
                    int const lo_src = !(f01r == 0 && f01i == 0); /* alpha = the pair's lower site alone has a coefficient */
                    G->fast = lo_src ? LSK_GROUP_HOP_LO : LSK_GROUP_HOP_HI;
                    G->v_re = lo_src ? f01r : f10r;
                    G->v_im = lo_src ? f01i : f10i;
                }
            }
        } else {
            /* sampled check (fixed seed) */
            uint64_t z = 0x9e3779b97f4a7c15ULL;
            for (int it = 0; it < 4096; ++it) {
                z = ls_amd_hash64_01(z + 0x9e3779b97f4a7c15ULL * (uint64_t)(it + 1));
                double fr, fi, gr, gi;
                eval_terms(ext->off, G->begin, G->end, z, &fr, &fi);
                eval_terms(ext->off, G->begin, G->end, z ^ G->x, &gr, &gi);
                if (fabs(gr - fr) > 1e-12 * (1 + fabs(fr)) || fabs(gi + fi) > 1e-12 * (1 + fabs(fi))) { ext->is_hermitian = 0; break; }
            }
        }
    }
}

typedef struct { int lo; int index; double re, im; int kind; } run_item;
static int run_item_cmp(void const *pa, void const *pb) {
    run_item const *a = (run_item const *)pa, *b = (run_item const *)pb;
    return a->lo < b->lo ? -1 : (a->lo > b->lo ? 1 : 0);
}

/* Recognise exchange runs among the groups and zz runs among the diagonal terms (lsk.h) and move
 * them to the front of their arrays.  `number_sites`/`inversion`: runs must not touch the top site
 * of a spin-inversion basis, where the image state may need the global flip. */
static void detect_runs(struct ls_amd_operator_ext *ext, int number_sites, int inversion) {
    lsk_runs *R = &ext->runs;
    memset(R, 0, sizeof(*R));
    /* ---- off-diagonal exchange runs ---- */
    int ng = ext->n_groups;
    run_item *items = (run_item *)malloc(sizeof(run_item) * (ng > 0 ? ng : 1));
    int ni = 0;
    for (int g = 0; g < ng; ++g) {
        lsk_group const *G = &ext->groups[g];
        if (G->fast == LSK_GROUP_GENERIC || G->adj < 0) continue; /* exchange pairs and directed pairs (HOP_*) on adjacent sites */
        if (inversion && G->fast != LSK_GROUP_EXCHANGE) continue;  /* (directed runs: unprojected bases only -- k_direct's DIRECTED instantiation) */
        if (inversion && G->adj + 1 >= number_sites - 1) continue;
        run_item it = {G->adj, g, G->v_re, G->v_im, G->fast};
        items[ni++] = it;
    }
    qsort(items, ni, sizeof(run_item), run_item_cmp);
    char *taken = (char *)calloc(ng > 0 ? ng : 1, 1);
    lsk_group *reordered = (lsk_group *)malloc(sizeof(lsk_group) * (ng > 0 ? ng : 1));
    int w = 0;
    for (int i = 0; i < ni && R->n_runs < LSK_MAX_RUNS;) {
        int j = i + 1;
        while (j < ni && items[j].lo == items[j - 1].lo + 1 && items[j].re == items[i].re && items[j].im == items[i].im && items[j].kind == items[i].kind) ++j;
        if (j - i >= 2) {
            int r = R->n_runs++;
            int const dir = items[i].kind == LSK_GROUP_HOP_LO ? 1 : (items[i].kind == LSK_GROUP_HOP_HI ? 2 : 0);
            R->lo0[r] = items[i].lo; R->cnt[r] = (j - i) | (dir << 16); R->v_re[r] = items[i].re; R->v_im[r] = items[i].im;
            for (int k = i; k < j; ++k) { reordered[w++] = ext->groups[items[k].index]; taken[items[k].index] = 1; }
        }
        i = j;
    }
    R->n_run_groups = w;
    for (int g = 0; g < ng; ++g) if (!taken[g]) reordered[w++] = ext->groups[g];
    memcpy(ext->groups, reordered, sizeof(lsk_group) * ng);
    free(items); free(taken); free(reordered);
    /* ---- diagonal zz runs ---- */
    int nd = ext->n_diag;
    items = (run_item *)malloc(sizeof(run_item) * (nd > 0 ? nd : 1));
    ni = 0;
    for (int t = 0; t < nd; ++t) {
        lsk_term const *T = &ext->diag[t];
        if (T->m != 0 || T->r != 0 || T->v_im != 0.0 || __builtin_popcountll(T->s) != 2) continue;
        int lo = __builtin_ctzll(T->s);
        if (T->s != (3ULL << lo)) continue;
        run_item it = {lo, t, T->v_re, 0.0, 0};
        items[ni++] = it;
    }
    qsort(items, ni, sizeof(run_item), run_item_cmp);
    taken = (char *)calloc(nd > 0 ? nd : 1, 1);
    lsk_term *dre = (lsk_term *)malloc(sizeof(lsk_term) * (nd > 0 ? nd : 1));
    w = 0;
    for (int i = 0; i < ni && R->n_zz < LSK_MAX_RUNS;) {
        int j = i + 1;
        while (j < ni && items[j].lo == items[j - 1].lo + 1 && items[j].re == items[i].re) ++j;
        if (j - i >= 2) {
            int r = R->n_zz++;
            R->zz_lo0[r] = items[i].lo; R->zz_cnt[r] = j - i; R->zz_v[r] = items[i].re;
            for (int k = i; k < j; ++k) { dre[w++] = ext->diag[items[k].index]; taken[items[k].index] = 1; }
        }
        i = j;
    }
    R->n_zz_terms = w;
    for (int t = 0; t < nd; ++t) if (!taken[t]) dre[w++] = ext->diag[t];
    memcpy(ext->diag, dre, sizeof(lsk_term) * nd);
    free(items); free(taken); free(dre);
}

static ls_hs_nonbranching_terms *make_nbt(lsk_term const *t, uint64_t const *xs, int n, int nbits) {
    if (n == 0) return NULL; /* the reference tests `p == nil` (ForeignTypes.chpl:219-222) */
    ls_hs_nonbranching_terms *nb = (ls_hs_nonbranching_terms *)calloc(1, sizeof(*nb));
    ls_hs_scalar *v = (ls_hs_scalar *)malloc(sizeof(ls_hs_scalar) * n);
    uint64_t *m = (uint64_t *)malloc(8 * n), *l = (uint64_t *)malloc(8 * n), *r = (uint64_t *)malloc(8 * n),
             *x = (uint64_t *)malloc(8 * n), *s = (uint64_t *)malloc(8 * n);
    for (int i = 0; i < n; ++i) {
        v[i].re = t[i].v_re; v[i].im = t[i].v_im;
        m[i] = t[i].m; r[i] = t[i].r; x[i] = xs ? xs[i] : 0; s[i] = t[i].s;
        l[i] = t[i].r ^ (x[i] & t[i].m);
    }
    nb->number_terms = n; nb->number_bits = nbits;
    nb->v = v; nb->m = m; nb->l = l; nb->r = r; nb->x = x; nb->s = s;
    return nb;
}
static void free_nbt(ls_hs_nonbranching_terms *nb) {
    if (!nb) return;
    free((void *)nb->v); free((void *)nb->m); free((void *)nb->l); free((void *)nb->r);
    free((void *)nb->x); free((void *)nb->s); free(nb);
}

/* term tables of an operator: filter / normalise / merge the raw terms, split them into diagonal and off-diagonal ones,
 * group the latter by flip mask, classify.  *offx_out (malloc'ed, n_off entries): flip mask of every off-diagonal term. */
static struct ls_amd_operator_ext *build_operator_ext(int number_sites, int has_inversion, int number_terms, double const *v,
                                                      uint64_t const *m, uint64_t const *r, uint64_t const *x,
                                                      uint64_t const *s, uint64_t **offx_out) {
    uint64_t const site_mask = number_sites >= 64 ? ~0ULL : ((1ULL << number_sites) - 1);
    raw_term *raw = (raw_term *)malloc(sizeof(raw_term) * (number_terms > 0 ? number_terms : 1));
    int n = 0;
    double vmax = 0;
    for (int i = 0; i < number_terms; ++i) {
        if ((m[i] | r[i] | x[i] | s[i]) & ~site_mask) { free(raw); set_error("term %d touches sites outside the basis", i); return NULL; }
        if (r[i] & ~m[i]) continue; /* can never be active */
        raw_term t = {v[2 * i], v[2 * i + 1], m[i], r[i], x[i], s[i]};
        /* sign bits inside the projector have a fixed value when the term is active */
        if (__builtin_popcountll(t.r & t.s) & 1) { t.re = -t.re; t.im = -t.im; }
        t.s &= ~t.m;
        raw[n++] = t;
        double a = fabs(t.re) + fabs(t.im);
        if (a > vmax) vmax = a;
    }
    qsort(raw, n, sizeof(raw_term), raw_cmp);
    /* merge equal keys */
    int w = 0;
    for (int i = 0; i < n;) {
        raw_term acc = raw[i];
        int j = i + 1;
        while (j < n && raw_cmp(&raw[i], &raw[j]) == 0) { acc.re += raw[j].re; acc.im += raw[j].im; ++j; }
        if (fabs(acc.re) + fabs(acc.im) > 1e-15 * vmax) raw[w++] = acc;
        i = j;
    }
    n = w;
    struct ls_amd_operator_ext *ext = (struct ls_amd_operator_ext *)calloc(1, sizeof(*ext));
    int nd = 0;
    while (nd < n && raw[nd].x == 0) ++nd; /* sorted by x: the diagonal terms come first */
    ext->n_diag = nd;
    ext->n_off = n - nd;
    ext->diag = (lsk_term *)malloc(sizeof(lsk_term) * (nd > 0 ? nd : 1));
    ext->off = (lsk_term *)malloc(sizeof(lsk_term) * (ext->n_off > 0 ? ext->n_off : 1));
    uint64_t *offx = (uint64_t *)malloc(8 * (ext->n_off > 0 ? ext->n_off : 1));
    ext->is_real = 1;
    for (int i = 0; i < n; ++i) {
        lsk_term t = {raw[i].re, raw[i].im, raw[i].m, raw[i].r, raw[i].s};
        if (raw[i].im != 0.0) ext->is_real = 0;
        if (i < nd) ext->diag[i] = t; else { ext->off[i - nd] = t; offx[i - nd] = raw[i].x; }
    }
    ext->groups = (lsk_group *)malloc(sizeof(lsk_group) * (ext->n_off > 0 ? ext->n_off : 1));
    ext->n_groups = 0;
    for (int i = 0; i < ext->n_off; ++i) {
        if (i == 0 || offx[i] != offx[i - 1]) {
            lsk_group G;
            memset(&G, 0, sizeof(G));
            G.x = offx[i];
            G.begin = i;
            ext->groups[ext->n_groups++] = G;
        }
        ext->groups[ext->n_groups - 1].end = i + 1;
    }
    classify_groups(ext);
    detect_runs(ext, number_sites, has_inversion);
    free(raw);
    if (offx_out) *offx_out = offx; else free(offx);
    return ext;
}

/* The operator SHARES its basis (one more reference), as upstream's ls_hs_operator does: representatives set or built
 * on the basis after the operator exists are seen by the operator, and nothing is duplicated (the representatives of
 * heisenberg_chain_32 are 4.8 GB of host memory). */
ls_hs_operator *ls_hs_create_operator_from_terms(ls_hs_basis const *basis, int number_terms,
                                                 double const *v, uint64_t const *m, uint64_t const *r,
                                                 uint64_t const *x, uint64_t const *s) {
    struct ls_amd_basis_ext *be = (struct ls_amd_basis_ext *)reg_get(basis);
    if (!be) { set_error("unknown basis: create it with ls_hs_create_spin_basis or register it with ls_amd_adopt_basis"); return NULL; }
    uint64_t *offx = NULL;
    struct ls_amd_operator_ext *ext = build_operator_ext(NBITS(basis), basis->spin_inversion != 0, number_terms, v, m, r,
                                                         x, s, &offx);
    if (!ext) return NULL;
    ls_hs_operator *op = (ls_hs_operator *)calloc(1, sizeof(*op));
    reg_put(op, ext, REG_OPERATOR);
    op->basis = (ls_hs_basis *)basis;
    __atomic_add_fetch(&be->refcount, 1, __ATOMIC_RELAXED);
    op->diag_terms = make_nbt(ext->diag, NULL, ext->n_diag, NBITS(basis));
    op->off_diag_terms = make_nbt(ext->off, offx, ext->n_off, NBITS(basis));
    free(offx);
    return op;
}

/* ---- foreign objects ------------------------------------------------------------------------ */
/* A basis struct somebody else owns (e.g. built by lattice-symmetries-haskell): only the reference's prefix is read
 * (number_sites, number_up = Hamming weight or -1, spin_inversion, representatives; FFI.chpl:94-105).  The symmetry
 * group is not part of that prefix, so the caller passes the generators it built the basis from (the YAML's
 * `symmetries`), in the convention of ls_hs_create_spin_basis. */
static int adopt_basis(ls_hs_basis const *basis, int spin_flip, int number_generators, int const *permutations, int const *sectors) {
    if (!basis) return set_error("null basis");
    if (reg_get(basis)) return set_error("basis %p is already registered", (void const *)basis);
    ls_hs_basis *tmp;
    if (basis->particle_type == LS_HS_SPINLESS_FERMION) {
        /* spinless-fermion prefix: number_sites, number_particles, particle_type; site permutations with their signs on the modes */
        if (basis->spin_inversion != 0 || basis->number_up != -1) return set_error("spinless-fermion bases have no spin inversion and no number_up");
        tmp = ls_hs_create_spinless_fermion_basis(basis->number_sites, basis->number_particles, number_generators, permutations, sectors);
    } else if (basis->particle_type == LS_HS_SPINFUL_FERMION && basis->number_up != -1 && (number_generators != 0 || spin_flip != 0)) {
        /* spinful (N, N_up) prefix: SITE generators, lifted to both species, and the up <-> down flip */
        if (basis->spin_inversion != 0) return set_error("spinful-fermion bases have no spin inversion (the up <-> down flip is spin_flip)");
        tmp = ls_hs_create_spinful_fermion_basis(basis->number_sites, basis->number_particles, basis->number_up, spin_flip, number_generators,
                                                 permutations, sectors);
    } else if (basis->particle_type != LS_HS_SPIN) {
        /* other fermionic prefixes: number_sites, number_particles, number_up, particle_type; no symmetries (on the N-only spinful
         * basis they are not supported: it is a spinless basis on 2 L modes) */
        if (number_generators != 0 || spin_flip != 0 || basis->spin_inversion != 0 || basis->requires_projection)
            return set_error("fermionic bases with symmetries are not supported");
        tmp = ls_hs_create_basis(basis->particle_type, basis->number_sites, basis->number_particles, basis->number_up);
    } else
        tmp = ls_hs_create_spin_basis(basis->number_sites, basis->number_up >= 0 ? basis->number_up : -1, basis->spin_inversion,
                                      number_generators, permutations, sectors);
    if (!tmp) return -1;
    if (tmp->requires_projection != basis->requires_projection) {
        ls_hs_destroy_basis(tmp);
        return set_error("generators do not reproduce the basis: requires_projection differs");
    }
    /* move the private part over to the foreign address */
    struct ls_amd_basis_ext *e = (struct ls_amd_basis_ext *)reg_get(tmp);
    reg_del(tmp);
    free(tmp);
    e->adopted = 1;
    e->owns_representatives = 0;
    reg_put(basis, e, REG_BASIS);
    return 0;
}
int ls_amd_adopt_basis(ls_hs_basis const *basis, int number_generators, int const *permutations, int const *sectors) {
    return adopt_basis(basis, 0, number_generators, permutations, sectors);
}
int ls_amd_adopt_spinful_fermion_basis(ls_hs_basis const *basis, int spin_flip, int number_generators, int const *permutations,
                                       int const *sectors) {
    if (basis && basis->particle_type != LS_HS_SPINFUL_FERMION) return set_error("ls_amd_adopt_spinful_fermion_basis: not a spinful-fermion basis");
    return adopt_basis(basis, spin_flip, number_generators, permutations, sectors);
}
/* An operator struct somebody else owns: the term tables are rebuilt from its off_diag_terms / diag_terms
 * (ls_hs_nonbranching_terms, number_words == 1) and kept in the side table. */
int ls_amd_adopt_operator(ls_hs_operator const *op) {
    if (!op || !op->basis) return set_error("null operator");
    if (reg_get(op)) return set_error("operator %p is already registered", (void const *)op);
    if (!reg_get(op->basis)) return set_error("the operator's basis is unknown: ls_amd_adopt_basis first");
    ls_hs_nonbranching_terms const *parts[2] = {op->diag_terms, op->off_diag_terms};
    int n = 0;
    for (int k = 0; k < 2; ++k)
        if (parts[k]) {
            if (parts[k]->number_bits > 64) return set_error("bases with more than 64 bits are not yet implemented"); /* DMV:1099 */
            n += parts[k]->number_terms;
        }
    double *v = (double *)malloc(16 * (size_t)(n > 0 ? n : 1));
    uint64_t *m = (uint64_t *)malloc(8 * (size_t)(n > 0 ? n : 1)), *r = (uint64_t *)malloc(8 * (size_t)(n > 0 ? n : 1)),
             *x = (uint64_t *)malloc(8 * (size_t)(n > 0 ? n : 1)), *s = (uint64_t *)malloc(8 * (size_t)(n > 0 ? n : 1));
    int k = 0;
    for (int q = 0; q < 2; ++q)
        for (int i = 0; parts[q] && i < parts[q]->number_terms; ++i, ++k) {
            v[2 * k] = parts[q]->v[i].re; v[2 * k + 1] = parts[q]->v[i].im;
            m[k] = parts[q]->m[i]; r[k] = parts[q]->r[i]; x[k] = parts[q]->x[i]; s[k] = parts[q]->s[i];
        }
    struct ls_amd_operator_ext *ext = build_operator_ext(NBITS(op->basis), op->basis->spin_inversion != 0, n, v, m, r, x, s, NULL);
    free(v); free(m); free(r); free(x); free(s);
    if (!ext) return -1;
    ext->adopted = 1;
    reg_put(op, ext, REG_OPERATOR);
    __atomic_add_fetch(&BEXT(op->basis)->refcount, 1, __ATOMIC_RELAXED);
    return 0;
}
/* forget an adopted basis / operator (device tables are released; the foreign struct is not touched) */
void ls_amd_release(void const *object) {
    int kind = 0;
    if (!reg_find(object, &kind)) return;
    if (kind == REG_BASIS) ls_hs_destroy_basis((ls_hs_basis *)object);
    else ls_hs_destroy_operator((ls_hs_operator *)object);
}

ls_hs_operator *ls_hs_clone_operator(ls_hs_operator const *op) {
    struct ls_amd_operator_ext const *e = OEXT(op);
    int n = e->n_diag + e->n_off;
    double *v = (double *)malloc(16 * (n > 0 ? n : 1));
    uint64_t *m = (uint64_t *)malloc(8 * (n > 0 ? n : 1)), *r = (uint64_t *)malloc(8 * (n > 0 ? n : 1)),
             *x = (uint64_t *)malloc(8 * (n > 0 ? n : 1)), *s = (uint64_t *)malloc(8 * (n > 0 ? n : 1));
    int k = 0;
    for (int i = 0; i < e->n_diag; ++i, ++k) {
        v[2 * k] = e->diag[i].v_re; v[2 * k + 1] = e->diag[i].v_im;
        m[k] = e->diag[i].m; r[k] = e->diag[i].r; x[k] = 0; s[k] = e->diag[i].s;
    }
    for (int g = 0; g < e->n_groups; ++g)
        for (int i = e->groups[g].begin; i < e->groups[g].end; ++i, ++k) {
            v[2 * k] = e->off[i].v_re; v[2 * k + 1] = e->off[i].v_im;
            m[k] = e->off[i].m; r[k] = e->off[i].r; x[k] = e->groups[g].x; s[k] = e->off[i].s;
        }
    ls_hs_operator *c = ls_hs_create_operator_from_terms(op->basis, n, v, m, r, x, s);
    free(v); free(m); free(r); free(x); free(s);
    return c;
}

void ls_hs_destroy_operator(ls_hs_operator *op) {
    if (!op) return;
    struct ls_amd_operator_ext *e = (struct ls_amd_operator_ext *)reg_get(op);
    if (!e) return;
    { /* plans cached for this operator hold its device tables (and its address may be reused by the next operator) */
        struct ls_amd_basis_ext *be = op->basis ? (struct ls_amd_basis_ext *)reg_get(op->basis) : NULL;
        if (be) basis_drop_host_plans(be, op, NULL);
    }
    if (e->d_groups) lsk_free(e->d_groups);
    if (e->d_off) lsk_free(e->d_off);
    if (e->d_diag) lsk_free(e->d_diag);
    free(e->groups); free(e->off); free(e->diag);
    reg_del(op);
    int const adopted = e->adopted;
    free(e);
    ls_hs_destroy_basis(op->basis); /* drops the operator's reference */
    if (adopted) return;
    free_nbt(op->diag_terms);
    free_nbt(op->off_diag_terms);
    free(op);
}

int ls_hs_operator_max_number_off_diag(ls_hs_operator const *op) { return OEXT(op)->n_groups; }
bool ls_hs_operator_is_hermitian(ls_hs_operator const *op) { return OEXT(op)->is_hermitian != 0; }
bool ls_hs_operator_is_real(ls_hs_operator const *op) { return OEXT(op)->is_real != 0; }

static int operator_device_unlocked(ls_hs_operator const *op, lsk_operator *out) {
    struct ls_amd_operator_ext *e = OEXT(op);
    if (!e->d_groups) {
        void *p;
        DEV(lsk_malloc(&p, sizeof(lsk_group) * (e->n_groups > 0 ? e->n_groups : 1)));
        DEV(lsk_h2d(p, e->groups, sizeof(lsk_group) * e->n_groups));
        e->d_groups = (lsk_group *)p;
        DEV(lsk_malloc(&p, sizeof(lsk_term) * (e->n_off > 0 ? e->n_off : 1)));
        DEV(lsk_h2d(p, e->off, sizeof(lsk_term) * e->n_off));
        e->d_off = (lsk_term *)p;
        DEV(lsk_malloc(&p, sizeof(lsk_term) * (e->n_diag > 0 ? e->n_diag : 1)));
        DEV(lsk_h2d(p, e->diag, sizeof(lsk_term) * e->n_diag));
        e->d_diag = (lsk_term *)p;
    }
    out->n_diag = e->n_diag;
    out->n_off = e->n_off;
    out->n_groups = e->n_groups;
    out->is_real = e->is_real;
    out->diag = e->d_diag;
    out->off = e->d_off;
    out->groups = e->d_groups;
    out->runs = e->runs;
    /* one real amplitude on every off-diagonal group, all of them exchange pairs: the projected pull kernels then carry no
     * coefficient per packet */
    out->uni = e->is_real && e->n_groups > 0;
    out->uni_v = e->n_groups > 0 ? e->groups[0].v_re : 0.0;
    for (int g = 0; g < e->n_groups && out->uni; ++g)
        if (e->groups[g].fast != LSK_GROUP_EXCHANGE || e->groups[g].v_im != 0.0 || e->groups[g].v_re != out->uni_v ||
            __builtin_popcountll(e->groups[g].x) != 2)
            out->uni = 0;
    return 0;
}

/* the device mirrors of a basis / an operator are uploaded on first use; several host threads may create plans on the same
 * objects at once (one communicator per thread) */
static int operator_device(ls_hs_operator const *op, lsk_operator *out) {
    pthread_mutex_lock(&g_device_tables_lock);
    int const rc = operator_device_unlocked(op, out);
    pthread_mutex_unlock(&g_device_tables_lock);
    return rc;
}
static int basis_device(ls_hs_basis const *b, lsk_basis *out) {
    pthread_mutex_lock(&g_device_tables_lock);
    int const rc = basis_device_unlocked(b, out);
    pthread_mutex_unlock(&g_device_tables_lock);
    return rc;
}

/* ============================================================================================ */
/* kernel table                                                                                 */
/* ============================================================================================ */
static ls_chpl_kernels g_kernels;
void ls_hs_internal_set_chpl_kernels(ls_chpl_kernels const *kernels) { g_kernels = *kernels; }
ls_chpl_kernels const *ls_hs_internal_get_chpl_kernels(void) { return &g_kernels; }

void ls_chpl_init_kernels(void) {
    ls_chpl_kernels k;
    k.enumerate_states = (void *)ls_chpl_enumerate_representatives;
    k.operator_apply_off_diag = (void *)ls_chpl_operator_apply_off_diag;
    k.operator_apply_diag = (void *)ls_chpl_operator_apply_diag;
    k.matrix_vector_product = (void *)ls_chpl_matrix_vector_product;
    ls_hs_internal_set_chpl_kernels(&k);
}

static int g_initialised = 0;
void ls_chpl_init(void) {
    if (g_initialised) return;
    if (lsk_device_count() < 1) { halt_with("ls_chpl_init: no HIP device available"); return; }
    char const *dev = getenv("LS_AMD_DEVICE");
    if (dev && lsk_set_device(atoi(dev)) != 0) { halt_with("ls_chpl_init: %s", lsk_last_error()); return; }
    ls_chpl_init_kernels();
    g_initialised = 1;
}
void ls_chpl_finalize(void) {
    if (g_d_binom) { lsk_free(g_d_binom); g_d_binom = NULL; }
    g_initialised = 0;
}

void ls_hs_basis_build(ls_hs_basis *basis) {
    if (basis->representatives.elts) return;
    typedef void (*enum_fn)(ls_hs_basis *, uint64_t, uint64_t, chpl_external_array *);
    enum_fn f = (enum_fn)g_kernels.enumerate_states;
    if (!f) { ls_chpl_init_kernels(); f = (enum_fn)g_kernels.enumerate_states; }
    chpl_external_array arr = {NULL, 0, NULL};
    f(basis, ls_hs_min_state_estimate(basis), ls_hs_max_state_estimate(basis), &arr);
    if (!arr.elts) return;
    basis_drop_device_caches(basis);
    basis->representatives = arr;
    BEXT(basis)->owns_representatives = 1;
}

/* ============================================================================================ */
/* plans                                                                                        */
/* ============================================================================================ */
typedef struct part_state {
    int64_t count;
    uint64_t const *d_reps; /* borrowed */
    lsk_index index;
    uint32_t *d_table;      /* owned */
    lsk_rankdir *d_dir;     /* owned: rank directory (hash partitions of unprojected fixed-weight bases), else NULL */
    double *d_norms;        /* owned (FULL projection) */
    int rounds;
    int64_t *send_counts;   /* [rounds][P] host */
    lsk_round_layout *d_layouts; /* [rounds] device */
    int64_t max_send_bytes;
    int64_t *h_beta_off, *h_val_off; /* [rounds][P] host copies of the layout */
    /* packet producer with per-wave rings (lsk_tile_wv, P <= 64): position of every (wave of 64 rows, destination) inside the
     * round's send segments, fixed by the plan's count pass -- [sum over rounds of waves][P] u32 */
    uint32_t *d_wtab;     /* owned */
    int64_t *wtab_first;  /* [rounds] first wave of the round in d_wtab */
    /* sorted packet streams (lsk_tile_st / lsk_window): position of every (tile, destination, stream) inside the destination's
     * segment -- [sum over rounds of tiles][P * S] u32 -- and the stream starts of every segment, [rounds][P][S + 1] */
    uint32_t *d_ttab;     /* owned */
    int64_t *ttab_first;  /* [rounds + 1] first tile of the round in d_ttab */
    uint32_t *d_soff;     /* owned */
    uint32_t *h_soff;     /* owned: host copy (dist.c exchanges it at set-up) */
    struct ls_amd_gtab *scatter_gt; /* shared (refcount): {representative -> index} for the consumers of state-carrying packets, or NULL */
} part_state;

#ifndef LS_AMD_PULL_VALUES_DEFAULT
#define LS_AMD_PULL_VALUES_DEFAULT 0 /* flipped to 1 where the value table measures faster INCLUDING its refresh */
#endif
enum { FAMILY_DIRECT_PUSH = 0, FAMILY_DIRECT_PULL = 1, FAMILY_TILE = 2, FAMILY_TILE_PULL = 3,
       FAMILY_REPL_DIRECT = 4, FAMILY_REPL_TILE = 5 };

struct ls_amd_plan {
    ls_hs_operator const *op;
    lsk_operator dop;
    lsk_basis dbs;
    int cplx, P, me, n_local;
    int family;
    part_state *parts; /* [n_local] */
    void *d_send;      /* local mode: staging for one round */
    int64_t send_capacity;
    unsigned long long *d_cursors; /* [P] */
    unsigned long long *d_counts;  /* [P] */
    int *d_err;
    int64_t nnz;
    /* pre-indexed packets (packet plans over unprojected fixed-weight bases): all-destinations rank directory; the producer
     * writes (u32 index at the destination, value) and the consumers are search-free (lsk_gdir, lsk.h) */
    lsk_gdir gd;
    lsk_rankdir *d_gdir; /* owned */
    lsk_part_ctx *d_part_ctx; /* owned: all partitions in this process -- index / norms of every destination for the fused consumer */
    int part_ctx_any;         /* a partition whose index carries a rank directory (else 0) */
    int key_bytes;       /* 4: pre-indexed packets, 8: packets carry the state */
    /* sorted packet streams (all partitions in this process; unprojected fixed-weight bases, exchange operators): every source
     * partition keeps its round in its own buffer and ONE consumer launch per round adds windows of every y in LDS -- no atomics */
    int streams, st_S, st_tile_rows, st_wpb, st_rounds;
    int stream_gkeys;        /* the keys of the streams are global colex ranks; every partition then carries its own rank directory */
    void **d_send_parts;     /* [P] owned */
    lsk_wsrc *d_wsrcs;       /* owned: device [rounds][P destinations][P sources] */
    /* replicated-x mode: index / norms of the GLOBAL basis, global index of every local row */
    lsk_index gindex;
    uint32_t *d_gtable;
    int64_t *d_row_gidx;
    double *d_norms_global;
    /* tile map of the row kernels (lsk_tilemap in lsk.h) */
    lsk_tilemap tilemap;
    void *d_tilemap;
    int has_pairs; /* staged row kernel for arbitrary exchange pairs (lsk_pairs): non-ring lattices */
    int has_push_staged; /* staged push kernel (lsk_push_staged): LDS window of y per tile; y is cleared, not assigned by k_diag */
    int one_rank_full_basis; /* FAMILY_TILE with one rank that owns the full fixed-weight basis (plan_setup_part) */
    lsk_pairplan pairs;
    void *d_pair_recs, *d_rank_low, *d_pair_binom, *d_states32, *d_pair_rows, *d_pair_sites;
    int global_index;  /* a temporary plan that only builds the index of the GLOBAL basis (replicated-x plans): no product index */
    int has_hubbard;   /* species-split row kernel (lsk_hubbard_apply): spinful product basis, separable operator */
    lsk_hubbard hubbard;
    void *d_hub[6];    /* words / ranks / amplitudes of the two species tables */
    int has_chain; /* staged row kernel (lsk_chain) */
    int chain_cached;      /* leading non-adjacent exchange groups whose partner ranks are cached */
    void *d_chain_cache;   /* [chain_cached][count] u32, or u64 when chain_wide */
    int chain_wide;        /* 64-bit ranks (>= 2^32 - 1 states) */
    uint64_t *d_chain_rec; /* fused records (lsk_chain_pack) replacing reps + the first cached pair */
    void *d_chain_wave;    /* 32-bit states and ranks: word table + one 8-byte header per 64 rows (setup_chain_headers); headed wave-rows do not read their records */
    int chain_row_bytes;   /* plan bytes per row the kernel streams with the headers, rounded up */
    int chain_headed;      /* the wave headers are in use (not all ones) */
    int chain_headers_apply; /* ... or would be without LS_AMD_CHAIN_RECORDS=1 */
    /* paired tiles (setup_chain_pairs, lsk_chain_paired): tile map of the paired launch, headers of its second segments, rows between
     * the two segments of a tile, first paired row; d_tilemap then covers the other rows only */
    int chain_paired, chain_pair_levels; /* (the deepest level that holds a range) */
    void *d_tilemap_pair, *d_chain_hdr_b; /* (two words per slot; the headers of every range's second segments) */
    lsk_tilemap tilemap_pair;
    int64_t chain_pair_rows[8]; /* rows paired at level 1, 2, ... ([0] unused) */
    double chain_v[2];
    int64_t chain_row0; /* global rank of the first local row (replicated-x plans) */
    void *d_htab;        /* hash table {rep -> x * norm(rep)} of the tile-pull families */
    uint32_t *d_slot_of; /* slot of every (global) representative */
    int htab_bits;
    void *d_xs;          /* x * norm in index order (K4 modes that prescale x): values of the near window; else x itself */
    int pull_halo;       /* near window of the staged pull kernel (entries either side of a tile), 0 = off */
    /* indexed mode of the staged pull kernel (lsk_tile_pull_idx): static {rep -> slot} table shared by every plan over the
     * same global basis and partition layout; nothing is refreshed per matvec */
    int idx_mode;
    struct ls_amd_gtab *gtab;
    uint64_t *d_vtab;    /* owned: value table over the same buckets (f64, one partition, matrix-free), else NULL */
    int64_t row_g0;      /* global index of the first local row (replicated-x plans over a contiguous block) */
    /* split matvec of the indexed mode (lsk_tile_pull_resolve | lsk_tile_pull_gather): packet streams of the first
     * split_rows rows (a multiple of 256, or all of them); 0 = the fused kernel only */
    lsk_pullbuf pbuf;
    int64_t split_rows;
    int64_t split_active; /* rows [0, split_active) are resolved ahead this matvec (<= split_rows, whole 256-row tiles or all of
                           * them; 0 = follow split_rows): the replicated-x driver resolves only as many rows as hide its exchange */
    /* slot cache (ls_amd_plan_cache_slots): the packet streams of the split form are plan data -- they depend on the operator,
     * the basis and the partition layout only -- so a plan that is applied many times (an eigensolver) resolves them ONCE and
     * every later matvec is the gather kernel alone.  Opt-in: the path is then no longer matrix-free (5 bytes per non-zero of
     * HBM for one-amplitude operators, 13 / 21 with real / complex coefficients). */
    int slot_cache, slot_cache_valid;
    int64_t slot_cache_bytes;
    /* block matvec (ls_amd_matvec_block): its own packet buffer of the projected path (chunks of blk_rows rows, allocated on first
     * use), its own 256-row tile map for k_direct_blk when the plan's row kernel tiles otherwise, one column of x and of y for the
     * strided columns of the `columns` path -- none of it touches the single-vector state above */
    lsk_pullbuf blk_pbuf;
    int64_t blk_rows;
    lsk_tilemap blk_tilemap;
    void *d_blk_tilemap;
    void *d_blk_cols; /* [2][count] elements */
    void *d_gram_work;        /* ls_amd_matvec_block_axpby_gram: the partials of the Gram launch, gram_work_bytes of them */
    size_t gram_work_bytes;
    void *d_series_work;      /* ls_amd_matvec_block_series without caller's work: two blocks of count x series_cols elements */
    int series_cols;
    double *d_series_dots;    /* [64][2 * 64]: the dots of 64 orders */
    void const *y_checked[2]; /* y pointers whose memory kind was looked at (push plans: ls_amd_internal_check_y) */
    int leaves_basis;         /* pull plan over a non-Hermitian operator whose row expansion leaves the basis (found at plan time) */
    /* kernel timing ring */
    int t_capacity, t_count;
    void **t_start, **t_stop;
    /* stage timers (the reference's kDisplayTimings tree, DMV:1028-1052): event pairs tagged with a stage */
    int st_capacity, st_count;
    void **st_start, **st_stop;
    unsigned char *st_stage;
    double st_ms[8];
    int64_t st_calls[8];
    int64_t st_matvecs;
};

/* ---- static index tables (lsk_gtab) ---------------------------------------------------------------------------------
 * One table per (global basis, partition layout), shared by reference: every plan of a process over the same device array
 * of representatives and the same masks gets the same table and the same global-row -> slot permutation (the loop-back
 * ranks of the tests and of scripts/loopback_bench.py are threads of one process: eight private copies of a 17 GB table
 * would not fit one device; separate processes each build their own). */
typedef struct ls_amd_gtab {
    uint64_t const *reps; /* key: device array of the global representatives (borrowed) */
    uint8_t const *masks; /* key: owner of every global row (NULL: one partition, slot = global index) */
    int64_t n;
    int P, L;
    lsk_gtab tab;
    uint64_t *d_entries;
    uint32_t *d_perm;     /* [n] global row -> slot owner * max_count + local index (NULL when masks == NULL) */
    int64_t counts[LSK_MAX_PARTS], max_count;
    uint64_t finger[8];   /* key, part two: the representatives at eight sampled positions -- a caller that frees the array and
                           * gets the same address back for another basis of the same size (caching allocators do that) must not
                           * be handed the old table */
    int refs;
    struct ls_amd_gtab *next;
} ls_amd_gtab;
static ls_amd_gtab *g_gtabs = NULL;
static lsk_gtab no_gtab(void) { lsk_gtab t; memset(&t, 0, sizeof(t)); return t; }
static pthread_mutex_t g_gtab_lock = PTHREAD_MUTEX_INITIALIZER;

static void gtab_free(ls_amd_gtab *t) {
    if (t->d_entries) lsk_free(t->d_entries);
    if (t->d_perm) lsk_free(t->d_perm);
    free(t);
}
void ls_amd_internal_gtab_release(ls_amd_gtab *t) {
    if (!t) return;
    pthread_mutex_lock(&g_gtab_lock);
    if (--t->refs == 0) {
        for (ls_amd_gtab **q = &g_gtabs; *q; q = &(*q)->next)
            if (*q == t) { *q = t->next; break; }
        gtab_free(t);
    }
    pthread_mutex_unlock(&g_gtab_lock);
}
static int gtab_build(ls_amd_gtab *t, void *stream) {
    int64_t const n = t->n;
    int const P = t->P;
    if (t->masks) {
        /* slot of every global row: the hashed -> block merge of the slot numbers (arrFromHashedToBlock, HashedToBlock.chpl:67-153) */
        DEV(lsk_mask_counts(n, t->masks, P, t->counts, stream));
        for (int p = 0; p < P; ++p) if (t->counts[p] > t->max_count) t->max_count = t->counts[p];
        if ((int64_t)P * t->max_count >= 0xffffffffLL) return set_error("indexed pull: more than 2^32 - 1 slots");
        void *pos[LSK_MAX_PARTS];
        memset(pos, 0, sizeof(pos));
        void *perm64 = NULL, *perm32 = NULL;
        int rc = lsk_malloc(&perm64, 8 * (size_t)(n > 0 ? n : 1));
        for (int p = 0; p < P && rc == 0; ++p) {
            rc = lsk_malloc(&pos[p], 8 * (size_t)(t->counts[p] > 0 ? t->counts[p] : 1));
            if (rc == 0) rc = lsk_iota_i64(t->counts[p], (int64_t)p * t->max_count, (int64_t *)pos[p], stream);
        }
        if (rc == 0) rc = lsk_hashed_to_block(n, t->masks, P, 8, (void const *const *)pos, perm64, stream);
        if (rc == 0) rc = lsk_malloc(&perm32, 4 * (size_t)(n > 0 ? n : 1));
        if (rc == 0) rc = lsk_narrow_i32(n, (int64_t const *)perm64, (int32_t *)perm32, stream);
        if (rc == 0) rc = lsk_sync(stream);
        for (int p = 0; p < P; ++p) if (pos[p]) lsk_free(pos[p]);
        if (perm64) lsk_free(perm64);
        if (rc != 0) { if (perm32) lsk_free(perm32); return dev_error(); }
        t->d_perm = (uint32_t *)perm32;
    } else {
        t->counts[0] = n;
        t->max_count = n;
    }
    int64_t const max_bytes = (int64_t)1 << 40;
    int const bb = lsk_gtab_bits(t->L, n, max_bytes);
    if (bb < 0) return set_error("indexed pull: no admissible index-table size for %lld keys of %d bits", (long long)n, t->L);
    t->tab.L = t->L; t->tab.bbits = bb; t->tab.tbits = t->L - bb;
    void *p, *flag;
    DEV(lsk_malloc(&p, (size_t)16 << bb));
    t->d_entries = (uint64_t *)p;
    t->tab.entries = t->d_entries;
    DEV(lsk_malloc(&flag, sizeof(int)));
    int zero = 0, bad = 0;
    int rc = lsk_h2d(flag, &zero, sizeof(int)) || lsk_gtab_build(t->tab, t->d_entries, n, t->reps, t->d_perm, (int *)flag, stream) ||
             lsk_sync(stream) || lsk_d2h(&bad, flag, sizeof(int));
    lsk_free(flag);
    if (rc) return dev_error();
    if (bad) return set_error("indexed pull: a key could not be placed within 255 buckets of its home");
    return 0;
}
/* the table of (d_reps, n, d_masks, P), built on first use.  Holds g_gtab_lock while building: the other ranks of a
 * loop-back group wait for the one that got there first. */
static int gtab_fingerprint(uint64_t const *d_reps, int64_t n, void *stream, uint64_t *f) {
    memset(f, 0, 8 * sizeof(uint64_t));
    if (n <= 0) return 0;
    DEV(lsk_sync(stream));
    for (int k = 0; k < 8; ++k) DEV(lsk_d2h(&f[k], d_reps + (n - 1) * k / 7, sizeof(uint64_t)));
    return 0;
}
int ls_amd_internal_gtab_acquire(ls_amd_gtab **out, int L, uint64_t const *d_reps, int64_t n, uint8_t const *d_masks, int P,
                                 void *stream) {
    *out = NULL;
    uint64_t finger[8];
    if (gtab_fingerprint(d_reps, n, stream, finger) != 0) return -1;
    pthread_mutex_lock(&g_gtab_lock);
    for (ls_amd_gtab *t = g_gtabs; t; t = t->next)
        if (t->reps == d_reps && t->n == n && t->masks == d_masks && t->P == P && t->L == L && memcmp(t->finger, finger, sizeof(finger)) == 0) {
            ++t->refs;
            pthread_mutex_unlock(&g_gtab_lock);
            *out = t;
            return 0;
        }
    ls_amd_gtab *t = (ls_amd_gtab *)calloc(1, sizeof(*t));
    t->reps = d_reps; t->n = n; t->masks = d_masks; t->P = P; t->L = L;
    memcpy(t->finger, finger, sizeof(finger));
    if (gtab_build(t, stream) != 0) {
        gtab_free(t);
        pthread_mutex_unlock(&g_gtab_lock);
        return -1;
    }
    t->refs = 1;
    t->next = g_gtabs;
    g_gtabs = t;
    pthread_mutex_unlock(&g_gtab_lock);
    *out = t;
    return 0;
}
uint32_t const *ls_amd_internal_gtab_perm(ls_amd_gtab const *t) { return t->d_perm; }
int64_t ls_amd_internal_gtab_max_count(ls_amd_gtab const *t) { return t->max_count; }
int64_t const *ls_amd_internal_gtab_counts(ls_amd_gtab const *t) { return t->counts; }
int64_t ls_amd_internal_gtab_bytes(ls_amd_gtab const *t) { return (int64_t)16 << t->tab.bbits; }

static int timing_begin(ls_amd_plan *pl, void *stream) {
    if (pl->t_count >= pl->t_capacity) return -1;
    if (lsk_event_record(pl->t_start[pl->t_count], stream) != 0) return -1;
    return pl->t_count;
}
static void timing_end(ls_amd_plan *pl, int slot, void *stream) {
    if (slot < 0) return;
    if (lsk_event_record(pl->t_stop[slot], stream) == 0) pl->t_count = slot + 1;
}

/* ---- stage timers ----------------------------------------------------------------------------- */
enum { ST_DIAG = 0, ST_REFRESH = 1, ST_ROWS = 2, ST_GENERATE = 3, ST_EXCHANGE = 4, ST_SCATTER = 5, ST_RETURN = 6, ST_COUNT = 7 };
static int stage_begin(ls_amd_plan *pl, int stage, void *stream) {
    if (pl->st_count >= pl->st_capacity) return -1;
    if (lsk_event_record(pl->st_start[pl->st_count], stream) != 0) return -1;
    pl->st_stage[pl->st_count] = (unsigned char)stage;
    return pl->st_count;
}
static void stage_end(ls_amd_plan *pl, int slot, void *stream) {
    if (slot < 0) return;
    if (lsk_event_record(pl->st_stop[slot], stream) == 0) pl->st_count = slot + 1;
}
int ls_amd_internal_stage_begin(ls_amd_plan *pl, int stage, void *stream) { return stage_begin(pl, stage, stream); }
void ls_amd_internal_stage_end(ls_amd_plan *pl, int slot, void *stream) { stage_end(pl, slot, stream); }
void ls_amd_internal_count_matvec(ls_amd_plan *pl) { if (pl->st_capacity) ++pl->st_matvecs; }
/* Plans that accumulate into the caller's y with hardware f64 atomics (push: k_direct, the packet consumers) need y in
 * coarse-grained memory (hipMalloc): on fine-grained memory -- hipMallocManaged unless advised otherwise -- the unsafe-fp-atomics
 * `global_atomic_add_f64` may lose updates silently ("Atomics").  A managed y is refused here instead;
 * the host-pointer boundary (ls_chpl_matrix_vector_product) stages managed memory and never gets here with it.
 * LS_AMD_ALLOW_MANAGED_Y=1: the caller vouches for hipMemAdvise(..., hipMemAdviseSetCoarseGrain, ...). */
int ls_amd_internal_check_y(ls_amd_plan *pl, void const *y) {
    if (pl->family != FAMILY_DIRECT_PUSH && pl->family != FAMILY_TILE) return 0;
    if (!y || y == pl->y_checked[0] || y == pl->y_checked[1]) return 0;
    if (lsk_pointer_kind(y) == LSK_PTR_MANAGED) {
        char const *e = getenv("LS_AMD_ALLOW_MANAGED_Y");
        if (!e || atoi(e) == 0)
            return set_error("y is managed (hipMallocManaged) memory: this plan accumulates with hardware f64 atomics, which need "
                             "coarse-grained memory -- pass hipMalloc memory, go through ls_chpl_matrix_vector_product (which stages it), "
                             "or advise the range coarse-grained and set LS_AMD_ALLOW_MANAGED_Y=1");
    }
    pl->y_checked[1] = pl->y_checked[0];
    pl->y_checked[0] = y;
    return 0;
}
/* folds the recorded event pairs into the per-stage totals (synchronises on the events) */
static int stage_collect(ls_amd_plan *pl) {
    for (int i = 0; i < pl->st_count; ++i) {
        float ms = 0;
        DEV(lsk_event_elapsed_ms(pl->st_start[i], pl->st_stop[i], &ms));
        pl->st_ms[pl->st_stage[i]] += ms;
        pl->st_calls[pl->st_stage[i]] += 1;
    }
    pl->st_count = 0;
    return 0;
}
int ls_amd_plan_enable_stage_timing(ls_amd_plan *pl, int max_events) {
    for (int i = 0; i < pl->st_capacity; ++i) { lsk_event_destroy(pl->st_start[i]); lsk_event_destroy(pl->st_stop[i]); }
    free(pl->st_start); free(pl->st_stop); free(pl->st_stage);
    pl->st_start = pl->st_stop = NULL; pl->st_stage = NULL;
    pl->st_capacity = pl->st_count = 0;
    memset(pl->st_ms, 0, sizeof(pl->st_ms)); memset(pl->st_calls, 0, sizeof(pl->st_calls));
    pl->st_matvecs = 0;
    if (max_events <= 0) return 0;
    pl->st_start = (void **)calloc(max_events, sizeof(void *));
    pl->st_stop = (void **)calloc(max_events, sizeof(void *));
    pl->st_stage = (unsigned char *)calloc(max_events, 1);
    for (int i = 0; i < max_events; ++i) {
        DEV(lsk_event_create(&pl->st_start[i]));
        DEV(lsk_event_create(&pl->st_stop[i]));
        pl->st_capacity = i + 1;
    }
    return 0;
}
int ls_amd_plan_stage_times(ls_amd_plan *pl, double *ms, int64_t *calls, int64_t *matvecs) {
    if (stage_collect(pl) != 0) return -1;
    for (int k = 0; k < ST_COUNT; ++k) { ms[k] = pl->st_ms[k]; calls[k] = pl->st_calls[k]; }
    if (matvecs) *matvecs = pl->st_matvecs;
    return 0;
}
/* the reference prints this tree when kDisplayTimings is set (DMV:1028-1052); stages are mapped to what replaced them */
int ls_amd_plan_timing_report(ls_amd_plan *pl, char *buf, size_t cap) {
    if (stage_collect(pl) != 0) return -1;
    double total = 0;
    for (int k = 0; k < ST_COUNT; ++k) total += pl->st_ms[k];
    int64_t const m = pl->st_matvecs > 0 ? pl->st_matvecs : 1;
#define PER(k) (pl->st_ms[k] / (double)m), (long long)pl->st_calls[k]
    snprintf(buf, cap,
             "matrixVectorProduct [%s]: %.3f ms per matvec over %lld matvecs (device time of the stages, HIP events)\n"
             " \xe2\x94\x9c\xe2\x94\x80 localDiagonal (k_diag):                         %9.3f ms  (%lld launches)\n"
             " \xe2\x94\x9c\xe2\x94\x80 x preparation (table refresh | x n(rep) | permutation): %1.3f ms  (%lld launches)\n"
             " \xe2\x94\x9c\xe2\x94\x80 row kernel (fused computeOffDiag + localProcess): %7.3f ms  (%lld launches)\n"
             " \xe2\x94\x9c\xe2\x94\x80 producers (k_tile: computeOffDiag, stateInfo,\n"
             " \xe2\x94\x82   localeIdxOf, radixOneStep, own localProcess):    %9.3f ms  (%lld launches)\n"
             " \xe2\x94\x9c\xe2\x94\x80 exchange wait on the compute stream (all-to-all-v): %5.3f ms  (%lld waits)\n"
             " \xe2\x94\x9c\xe2\x94\x80 consumers (k_scatter: indexing + accessing):    %9.3f ms  (%lld launches)\n"
             " \xe2\x94\x94\xe2\x94\x80 replicated-x: y rows grouped by owner + returned: %8.3f ms  (%lld passes)\n",
             ls_amd_plan_kernel_name(pl), total / (double)m, (long long)pl->st_matvecs, PER(ST_DIAG), PER(ST_REFRESH), PER(ST_ROWS),
             PER(ST_GENERATE), PER(ST_EXCHANGE), PER(ST_SCATTER), PER(ST_RETURN));
#undef PER
    return 0;
}

int ls_amd_plan_enable_timing(ls_amd_plan *pl, int max_samples) {
    for (int i = 0; i < pl->t_capacity; ++i) { lsk_event_destroy(pl->t_start[i]); lsk_event_destroy(pl->t_stop[i]); }
    free(pl->t_start); free(pl->t_stop);
    pl->t_start = pl->t_stop = NULL;
    pl->t_capacity = pl->t_count = 0;
    if (max_samples <= 0) return 0;
    pl->t_start = (void **)calloc(max_samples, sizeof(void *));
    pl->t_stop = (void **)calloc(max_samples, sizeof(void *));
    for (int i = 0; i < max_samples; ++i) {
        DEV(lsk_event_create(&pl->t_start[i]));
        DEV(lsk_event_create(&pl->t_stop[i]));
        pl->t_capacity = i + 1;
    }
    return 0;
}
int ls_amd_plan_kernel_times(ls_amd_plan *pl, float *ms, int capacity, int *count) {
    int n = pl->t_count < capacity ? pl->t_count : capacity;
    for (int i = 0; i < n; ++i) DEV(lsk_event_elapsed_ms(pl->t_start[i], pl->t_stop[i], &ms[i]));
    *count = n;
    pl->t_count = 0;
    return 0;
}
int ls_amd_fill_random(int64_t n, uint64_t const *d_states, uint64_t seed, ls_amd_dtype dtype, void *d_out,
                       void *stream) {
    DEV(lsk_fill_random(n, d_states, seed, dtype == LS_AMD_C128, d_out, stream));
    return 0;
}

static int prescaled_x(ls_amd_plan *pl, int64_t n, uint64_t const *d_reps, void const *d_x, double const *d_norms,
                       void const **out, void *stream);

/* near window of the staged pull kernels: entries either side of a 256-row tile that are resolved in LDS (LS_AMD_PULL_HALO;
 * 0 = every partner through the table).  The indexed kernels hold the window as a hash set of <= 1024 entries and measure
 * alike from 64 to 512 (profiles/r3_indexed_ab_*): 256; the value-table kernel keeps its sorted window of +-512. */
static int pull_halo_setting(int indexed) {
    int const mx = indexed ? lsk_pull_max_halo() : 512;
    char const *e = getenv("LS_AMD_PULL_HALO");
    int h = e ? atoi(e) : (indexed ? 256 : 512);
    if (h < 0) h = 0;
    if (h > mx) h = mx;
    return h;
}

/* ---- split matvec: packet streams ------------------------------------------------------------------------------------- */
static void split_free(ls_amd_plan *pl) {
    if (pl->pbuf.offs) lsk_free((void *)pl->pbuf.offs);
    if (pl->pbuf.slots) lsk_free(pl->pbuf.slots);
    if (pl->pbuf.rows) lsk_free(pl->pbuf.rows);
    if (pl->pbuf.coefs) lsk_free(pl->pbuf.coefs);
    if (pl->pbuf.counts) lsk_free(pl->pbuf.counts);
    memset(&pl->pbuf, 0, sizeof(pl->pbuf));
    pl->split_rows = 0;
    pl->slot_cache = pl->slot_cache_valid = 0;
}
static void block_free(ls_amd_plan *pl) {
    if (pl->blk_pbuf.slots) lsk_free(pl->blk_pbuf.slots);
    if (pl->blk_pbuf.rows) lsk_free(pl->blk_pbuf.rows);
    if (pl->blk_pbuf.coefs) lsk_free(pl->blk_pbuf.coefs);
    if (pl->blk_pbuf.counts) lsk_free(pl->blk_pbuf.counts);
    memset(&pl->blk_pbuf, 0, sizeof(pl->blk_pbuf));
    pl->blk_rows = 0;
    if (pl->d_blk_tilemap) lsk_free(pl->d_blk_tilemap);
    pl->d_blk_tilemap = NULL;
    memset(&pl->blk_tilemap, 0, sizeof(pl->blk_tilemap));
    if (pl->d_blk_cols) lsk_free(pl->d_blk_cols);
    pl->d_blk_cols = NULL;
    if (pl->d_gram_work) lsk_free(pl->d_gram_work);
    pl->d_gram_work = NULL;
    pl->gram_work_bytes = 0;
    if (pl->d_series_work) lsk_free(pl->d_series_work);
    pl->d_series_work = NULL;
    pl->series_cols = 0;
    if (pl->d_series_dots) lsk_free(pl->d_series_dots);
    pl->d_series_dots = NULL;
}
/* room for the packet streams of as many of the plan's rows as `max_bytes` allow (all of them if it can); returns the number
 * of rows covered (0: none -- the plan keeps the fused kernel) */
int64_t ls_amd_internal_plan_split_enable(ls_amd_plan *pl, int64_t max_bytes) {
    split_free(pl);
    if (!pl->idx_mode || pl->dbs.proj != LSK_PROJ_FULL || pl->parts[0].count <= 0) return 0;
    int64_t const cap = lsk_pullbuf_cap(pl->dop);
    int const nc = lsk_pullbuf_coef_doubles(pl->dop, pl->dbs);
    int64_t const per_stream = cap * (4 + 1 + 8 * nc) + 4; /* 64 rows */
    int64_t streams = (pl->parts[0].count + 63) / 64;
    streams = (streams + 3) & ~(int64_t)3; /* whole 256-row tiles */
    if (max_bytes > 0 && streams * per_stream > max_bytes) streams = (max_bytes / per_stream) & ~(int64_t)3;
    while (streams >= 4) {
        void *a = NULL, *b = NULL, *c = NULL, *d = NULL;
        if (lsk_malloc(&a, (size_t)(streams * cap * 4)) == 0 && lsk_malloc(&b, (size_t)(streams * cap)) == 0 &&
            (nc == 0 || lsk_malloc(&c, (size_t)(streams * cap * 8 * nc)) == 0) && lsk_malloc(&d, (size_t)(streams * 4)) == 0) {
            pl->pbuf.slots = (uint32_t *)a; pl->pbuf.rows = (uint8_t *)b; pl->pbuf.coefs = (double *)c; pl->pbuf.counts = (uint32_t *)d;
            pl->pbuf.cap = cap;
            pl->pbuf.row0 = 0;
            pl->split_rows = streams * 64 < pl->parts[0].count ? streams * 64 : pl->parts[0].count;
            return pl->split_rows;
        }
        if (a) lsk_free(a);
        if (b) lsk_free(b);
        if (c) lsk_free(c);
        if (d) lsk_free(d);
        streams = (streams / 2) & ~(int64_t)3; /* no room: half as many rows */
    }
    return 0;
}
int64_t ls_amd_internal_plan_split_rows(ls_amd_plan const *pl) { return pl->split_rows; }
/* rows resolved ahead by the NEXT ls_amd_internal_repl_split_begin: a prefix of the rows the packet buffer covers (rounded down
 * to whole 256-row tiles; <= 0 or >= split_rows: all of them).  A cached plan keeps all its rows. */
static int64_t split_rows_now(ls_amd_plan const *pl) {
    if (pl->slot_cache || pl->split_active <= 0 || pl->split_active >= pl->split_rows) return pl->split_rows;
    return pl->split_active;
}
void ls_amd_internal_plan_split_set_active(ls_amd_plan *pl, int64_t rows) {
    pl->split_active = rows <= 0 ? 0 : (rows & ~(int64_t)255);
    if (rows > 0 && pl->split_active < 256) pl->split_active = 256;
}
int64_t ls_amd_internal_plan_split_active(ls_amd_plan const *pl) { return split_rows_now(pl); }
int ls_amd_internal_plan_slot_cached(ls_amd_plan const *pl) { return pl->slot_cache != 0; }
/* Streams laid out back to back at their exact lengths (a count pass of stage A + a scan): about half of what the worst-case
 * stride of the split form reserves.  Covers every row if `max_bytes` (<= 0: no ceiling) and the device allow, else the longest
 * prefix of whole 256-row tiles that fits -- the rows behind it keep the fused kernel.  Returns the rows covered (0: none, nothing
 * is left allocated), -1 on a device error. */
static int64_t split_enable_exact(ls_amd_plan *pl, int64_t max_bytes) {
    split_free(pl);
    part_state *ps = &pl->parts[0];
    int64_t const streams_all = (ps->count + 63) / 64;
    int const nc = lsk_pullbuf_coef_doubles(pl->dop, pl->dbs);
    int64_t const per_packet = 4 + 1 + 8 * nc;
    void *offs = NULL;
    /* (offsets and counts for WHOLE tiles of four streams: every wave of the last tile reads its offset and stores its count) */
    if (lsk_malloc(&offs, 8 * (size_t)(((streams_all + 3) & ~(int64_t)3) + 1)) != 0) return 0;
    if (lsk_tile_pull_stream_offsets(pl->dop, pl->dbs, 0, ps->count, ps->d_reps, (int64_t *)offs, NULL) != 0) { lsk_free(offs); return -1; }
    int64_t streams = streams_all;
    for (;;) {
        /* largest number of streams (whole tiles, or all of them) whose packets fit the ceiling: offs is ascending */
        int64_t total = 0;
        if (lsk_d2h(&total, (char *)offs + 8 * (size_t)streams, 8) != 0) { lsk_free(offs); return -1; }
        if (max_bytes > 0 && total * per_packet + 12 * streams + 8 > max_bytes) {
            int64_t lo = 0, hi = streams / 4; /* in tiles: lo fits, hi does not */
            while (hi - lo > 1) {
                int64_t const mid = lo + (hi - lo) / 2;
                int64_t t = 0;
                if (lsk_d2h(&t, (char *)offs + 8 * (size_t)(4 * mid), 8) != 0) { lsk_free(offs); return -1; }
                if (t * per_packet + 12 * 4 * mid + 8 <= max_bytes) lo = mid; else hi = mid;
            }
            streams = 4 * lo;
            if (streams <= 0) { lsk_free(offs); return 0; }
            if (lsk_d2h(&total, (char *)offs + 8 * (size_t)streams, 8) != 0) { lsk_free(offs); return -1; }
        }
        if (total >= ((int64_t)1 << 40)) { lsk_free(offs); return 0; }
        void *a = NULL, *b = NULL, *c = NULL, *d = NULL;
        if (lsk_malloc(&a, (size_t)(4 * total + 4)) == 0 && lsk_malloc(&b, (size_t)(total + 4)) == 0 &&
            (nc == 0 || lsk_malloc(&c, (size_t)(8 * nc * total + 8)) == 0) && lsk_malloc(&d, (size_t)(4 * ((streams + 3) & ~(int64_t)3))) == 0) {
            pl->pbuf.slots = (uint32_t *)a; pl->pbuf.rows = (uint8_t *)b; pl->pbuf.coefs = (double *)c; pl->pbuf.counts = (uint32_t *)d;
            pl->pbuf.offs = (int64_t const *)offs;
            pl->pbuf.cap = lsk_pullbuf_cap(pl->dop);
            pl->pbuf.row0 = 0;
            pl->split_rows = streams * 64 < ps->count ? streams * 64 : ps->count;
            pl->slot_cache_bytes = total * per_packet + 12 * streams + 8;
            return pl->split_rows;
        }
        if (a) lsk_free(a);
        if (b) lsk_free(b);
        if (c) lsk_free(c);
        if (d) lsk_free(d);
        /* the device has no room for this many: three quarters of it, in whole tiles */
        max_bytes = (total * per_packet + 12 * streams + 8) / 4 * 3;
        if (max_bytes < ((int64_t)1 << 20)) { lsk_free(offs); return 0; }
    }
}
/* Keep the resolved packet streams across matvecs (see slot_cache above; include/ls_amd.h).  Returns the number of rows whose
 * streams are cached: all of them, or the prefix that fits `max_bytes` / the device -- the rest runs the fused kernel. */
int64_t ls_amd_plan_cache_slots(ls_amd_plan *pl, int64_t max_bytes) {
    if (!pl || !pl->idx_mode || pl->dbs.proj != LSK_PROJ_FULL || pl->parts[0].count <= 0 ||
        (pl->family != FAMILY_TILE_PULL && pl->family != FAMILY_REPL_TILE)) return 0;
    int64_t const rows = split_enable_exact(pl, max_bytes);
    if (rows < 0) return dev_error();
    if (rows == 0) return 0;
    pl->slot_cache = 1;
    pl->slot_cache_valid = 0;
    return rows;
}
int ls_amd_plan_slot_cache_rows(ls_amd_plan const *pl, int64_t *rows, int64_t *bytes) {
    if (rows) *rows = pl->slot_cache ? pl->split_rows : 0;
    if (bytes) *bytes = pl->slot_cache ? pl->slot_cache_bytes : 0;
    return 0;
}

/* LS_AMD_PACKETS=block keeps the block-wide packet lists of k_tile (cursor atomics); default: per-wave rings (k_tile_wv) */
static int packets_wave_rings(void) {
    char const *e = getenv("LS_AMD_PACKETS");
    return !(e && strcmp(e, "block") == 0);
}
static int64_t rows_per_round_default(void) {
    char const *e = getenv("LS_AMD_ROWS_PER_ROUND");
    if (e) { long long v = atoll(e); if (v > 0) return (int64_t)v; }
    return (int64_t)1 << 24;
}

static int build_search_index(part_state *ps, int number_sites, void *stream) {
    if (ps->count >= 0xffffffffLL) return set_error("partitions with >= 2^32 states are not supported");
    int bits = 0;
    while ((1LL << (bits + 1)) <= ps->count) ++bits; /* floor(log2(count)) */
    bits -= 3;
    if (bits < 1) bits = 1;
    if (bits > 26) bits = 26;
    if (bits > number_sites) bits = number_sites;
    int shift = number_sites - bits;
    int64_t nbuckets = (int64_t)1 << bits;
    void *p;
    DEV(lsk_malloc(&p, 4 * (size_t)(nbuckets + 2)));
    ps->d_table = (uint32_t *)p;
    DEV(lsk_build_table(ps->count, ps->d_reps, shift, nbuckets, ps->d_table, stream));
    ps->index.kind = LSK_INDEX_SEARCH;
    ps->index.shift = shift;
    ps->index.table = ps->d_table;
    return 0;
}

static int upload(void **slot, void const *host, size_t bytes) {
    DEV(lsk_malloc(slot, bytes ? bytes : 8));
    DEV(lsk_h2d(*slot, host, bytes));
    return 0;
}

/* Tile map of the row kernels (lsk_tilemap in lsk.h): the traversal order is data, not code.
 *   chunk == 0: XCD k gets the k-th contiguous eighth of the row tiles;
 *   chunk  > 0: chunks of `chunk` consecutive tiles are dealt to the XCDs round-robin, so all XCDs advance through the
 *               same region of the vector together (the shared Infinity Cache sees one moving front) while each keeps
 *               runs of consecutive tiles for its own L2.
 * Orders that were measured and removed (r2, chain_32 f64, gpurun_out/r2/order_sweep.log): sets closed under the flips of
 * the top t site bits, per XCD or chip-wide (t = 6..12, 0.26 - 8 M rows per set): 10.97 - 11.67 ms against 11.09 ms
 * contiguous and 10.60 ms chunked -- the far-pair gathers are bound by the L2-miss request rate, which no order of
 * 1024-row tiles changes (a set small enough for one 4 MiB L2 is 70 tiles; 224 tiles are in flight per XCD). */
typedef struct { uint64_t *e; int64_t n, cap; } tile_list;
static void tile_push(tile_list *l, int64_t row, int64_t cnt) {
    if (l->n == l->cap) { l->cap = l->cap ? 2 * l->cap : 1024; l->e = (uint64_t *)realloc(l->e, sizeof(uint64_t) * (size_t)l->cap); }
    l->e[l->n++] = (uint64_t)row | ((uint64_t)cnt << 48);
}
static int tilemap_host(int64_t n, int TILE, int64_t chunk, uint64_t **out, int64_t *slots_out) {
    tile_list lists[8];
    memset(lists, 0, sizeof(lists));
    int64_t const tiles = (n + TILE - 1) / TILE;
    if (chunk > 0) {
        for (int64_t q = 0; q < tiles; ++q)
            tile_push(&lists[(q / chunk) % 8], q * TILE, n - q * TILE < TILE ? n - q * TILE : TILE);
    } else
        for (int k = 0; k < 8; ++k) /* XCD k: the k-th contiguous eighth of the tiles */
            for (int64_t q = tiles * k / 8; q < tiles * (k + 1) / 8; ++q)
                tile_push(&lists[k], q * TILE, n - q * TILE < TILE ? n - q * TILE : TILE);
    int64_t slots = 0, total = 0;
    for (int k = 0; k < 8; ++k) if (lists[k].n > slots) slots = lists[k].n;
    uint64_t *flat = (uint64_t *)calloc((size_t)(8 * slots > 0 ? 8 * slots : 1), sizeof(uint64_t));
    for (int k = 0; k < 8; ++k) {
        for (int64_t q = 0; q < lists[k].n; ++q) { flat[k * slots + q] = lists[k].e[q]; total += (int64_t)(lists[k].e[q] >> 48); }
        free(lists[k].e);
    }
    if (total != n) {
        free(flat);
        return set_error("internal error: tile map covers %lld of %lld rows", (long long)total, (long long)n);
    }
    *out = flat;
    *slots_out = slots;
    return 0;
}
/* Paired tiles of the chain kernel (k_chain_pair_t, lsk_chain_paired).  Read the top site bits as disjoint pairs (L-1, L-2), (L-3, L-4),
 * ...: levels 1, 2, ...  A row belongs to the first level, from the top, whose two bits differ; flipping them (bond b = L - 2 level)
 * keeps it there, so no row is claimed twice.  Fix a pattern h of the level - 1 higher pairs (each 00 or 11) and let m = k - popc(h) - 1
 * be the set bits below b: in the combinadic order of the weight-k words the rows with pair bits 01 are
 * base(h) + [C(b, m + 1), C(b + 1, m + 1)), those with 10 the next d = C(b, m) rows, and rows R01 + j and R01 + d + j differ in those two
 * bits only (base(h) = the rank terms of the set bits of h; level 1: R01 = [C(L-2, k), C(L-1, k))).  A range = the whole 512-row
 * segments [a0, a1) of one R01; hdr0 = where the wave headers of its second segments start, in headers, all ranges in one array.
 * Levels go on while b >= 12 (a far pair) and bond b lies in `bonds` (bit b: inside an exchange run), `levels` at most; ranges come in
 * (level, h ascending) order.  Returns their number, at most CHAIN_MAX_RANGES = 2^6 - 1 (six levels). */
#define CHAIN_MAX_PAIR_LEVELS 6
#define CHAIN_PAIR_LEVELS_DEFAULT 2 /* LS_AMD_CHAIN_PAIR_LEVELS; chain_32: 3, 4 and 6 measure 0.01-0.03 ms below 2, under 3 x the run-to-run spread (profiles/chain_pair_levels_ab.txt) */
#define CHAIN_MAX_RANGES 63
typedef struct { int level, bond; int64_t a0, a1, d, hdr0; } chain_range;
static int chain_pair_ranges(int L, int k, int levels, uint64_t bonds, chain_range *out) {
    if (L < 14 || L > 32 || k < 1 || k > L - 1) return 0;
    uint64_t C[33][33];
    memset(C, 0, sizeof(C));
    for (int n = 0; n <= 32; ++n) { C[n][0] = 1; for (int j = 1; j <= n; ++j) C[n][j] = C[n - 1][j - 1] + (j <= n - 1 ? C[n - 1][j] : 0); }
    if (levels > CHAIN_MAX_PAIR_LEVELS) levels = CHAIN_MAX_PAIR_LEVELS;
    int nr = 0;
    int64_t hdr = 0;
    for (int lv = 1; lv <= levels; ++lv) {
        int const b = L - 2 * lv;
        if (b < 12 || !((bonds >> b) & 1)) break;
        for (int h = 0; h < (1 << (lv - 1)); ++h) { /* bit t of h: the pair (b + 2 t + 3, b + 2 t + 2) is 11 */
            int const m = k - 2 * __builtin_popcount((unsigned)h) - 1;
            if (m < 0 || m > b) continue;
            int64_t base = 0;
            int idx = m + 1; /* set bits at or below the pair of this level */
            for (int t = 0; t < lv - 1; ++t)
                if ((h >> t) & 1) { base += (int64_t)C[b + 2 * t + 2][idx + 1] + (int64_t)C[b + 2 * t + 3][idx + 2]; idx += 2; }
            int64_t const r01 = base + (int64_t)C[b][m + 1], r10 = base + (int64_t)C[b + 1][m + 1];
            chain_range r = {lv, b, (r01 + 511) & ~(int64_t)511, r10 & ~(int64_t)511, r10 - r01, hdr};
            if (r.a1 <= r.a0) continue;
            hdr += (r.a1 - r.a0) / 64;
            out[nr++] = r;
        }
    }
    return nr;
}
#define CHAIN_TILE_PLAIN 0x8000 /* bit 63 of a tile-map entry (k_chain_t on fused records): this tile runs on its records, not on wave headers */
static int tilemap_deal(tile_list const *all, int64_t chunk, uint64_t **out, int64_t *slots_out) {
    int64_t const tiles = all->n;
    int64_t per[8] = {0, 0, 0, 0, 0, 0, 0, 0}, slots = 0;
    if (chunk > 0) for (int64_t q = 0; q < tiles; ++q) ++per[(q / chunk) % 8];
    else for (int k = 0; k < 8; ++k) per[k] = tiles * (k + 1) / 8 - tiles * k / 8; /* XCD k: the k-th contiguous eighth */
    for (int k = 0; k < 8; ++k) if (per[k] > slots) slots = per[k];
    uint64_t *flat = (uint64_t *)calloc((size_t)(8 * slots > 0 ? 8 * slots : 1), sizeof(uint64_t));
    if (!flat) return set_error("out of memory");
    int64_t fill[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int k0 = 0;
    for (int64_t q = 0; q < tiles; ++q) {
        int k;
        if (chunk > 0) k = (int)((q / chunk) % 8);
        else { while (q >= tiles * (k0 + 1) / 8) ++k0; k = k0; }
        flat[k * slots + fill[k]++] = all->e[q];
    }
    *out = flat;
    *slots_out = slots;
    return 0;
}
/* The two tile maps of a paired plan: `pairs` = one entry per paired tile (first row of its first segment | the id of its range << 32,
 * 1024 rows), in ascending row order over all ranges; `rest` = tiles of at most TILE rows over the rows outside every range's segments
 * [a0, a1) and [a0 + d, a1 + d), cut at the multiples of TILE; a tile that starts or ends off the 64-row grid of the wave headers (the
 * second segments do) is flagged CHAIN_TILE_PLAIN, and one that starts off it ends at the next multiple of 64.  Both are dealt like
 * tilemap_host does, `pairs` in chunks of pair_chunk.  Every row lies in exactly one tile of the two maps. */
typedef struct { int64_t lo, hi; int id; } chain_span;
static int chain_span_cmp(void const *pa, void const *pb) {
    int64_t const a = ((chain_span const *)pa)->lo, b = ((chain_span const *)pb)->lo;
    return a < b ? -1 : a > b;
}
static int tilemap_paired_host(int64_t n, int TILE, int64_t chunk, int64_t pair_chunk, chain_range const *rg, int nr, uint64_t **rest,
                               int64_t *rest_slots, uint64_t **pairs, int64_t *pair_slots) {
    tile_list all[2];
    memset(all, 0, sizeof(all));
    chain_span sp[2 * CHAIN_MAX_RANGES];
    *rest = *pairs = NULL;
    if (nr < 1 || nr > CHAIN_MAX_RANGES) return set_error("internal error: %d paired ranges", nr);
    for (int r = 0; r < nr; ++r) {
        sp[2 * r] = (chain_span){rg[r].a0, rg[r].a1, r};
        sp[2 * r + 1] = (chain_span){rg[r].a0 + rg[r].d, rg[r].a1 + rg[r].d, -1};
    }
    qsort(sp, (size_t)(2 * nr), sizeof(chain_span), chain_span_cmp);
    int64_t total = 0, from = 0;
    int rc = 0;
    for (int q = 0; q <= 2 * nr && !rc; ++q) {
        int64_t const to = q < 2 * nr ? sp[q].lo : n;
        if (to < from || (q < 2 * nr && sp[q].hi > n)) { rc = set_error("internal error: paired ranges overlap"); break; }
        for (int64_t pos = from; pos < to;) {
            int64_t end = (pos / TILE + 1) * TILE;
            if (pos & 63) end = (pos | 63) + 1;
            if (end > to) end = to;
            int const plain = (pos & 63) != 0 || ((end & 63) != 0 && end != n);
            tile_push(&all[0], pos, (end - pos) | (plain ? CHAIN_TILE_PLAIN : 0));
            total += end - pos;
            pos = end;
        }
        if (q == 2 * nr) break;
        if (sp[q].id >= 0)
            for (int64_t i0 = sp[q].lo; i0 < sp[q].hi; i0 += 512) { tile_push(&all[1], i0 | ((int64_t)sp[q].id << 32), 1024); total += 1024; }
        from = sp[q].hi;
    }
    if (!rc && total != n) rc = set_error("internal error: paired tile maps cover %lld of %lld rows", (long long)total, (long long)n);
    if (!rc) rc = tilemap_deal(&all[0], chunk, rest, rest_slots);
    if (!rc) rc = tilemap_deal(&all[1], pair_chunk, pairs, pair_slots);
    if (rc) { free(*rest); free(*pairs); *rest = *pairs = NULL; }
    free(all[0].e);
    free(all[1].e);
    return rc;
}
static int build_tilemap(ls_amd_plan *pl, int64_t n, int TILE) {
    uint64_t *flat = NULL;
    int64_t slots = 0;
    /* Default for the staged kernel: chunks of 256 tiles -- measured on chain_32 with one block per tile
     * (gpurun_out/r2: 9.35 ms contiguous eighths, 8.98 / 8.56 / 8.47 / 8.47 / 8.49 / 8.53 / 8.85 / 9.83 ms at
     * 4 / 32 / 128 / 256 / 512 / 1024 / 4096 / 16384) */
    char const *e = getenv("LS_AMD_TILE_CHUNK");
    int64_t const chunk = e ? atoll(e) : (TILE >= 512 ? 256 : 0);
    if (tilemap_host(n, TILE, chunk > 0 ? chunk : 0, &flat, &slots) < 0) return -1;
    int const up = upload(&pl->d_tilemap, flat, sizeof(uint64_t) * (size_t)(8 * slots > 0 ? 8 * slots : 1));
    free(flat);
    if (up) return -1;
    pl->tilemap.entries = (uint64_t const *)pl->d_tilemap;
    pl->tilemap.slots_per_xcd = slots;
    return 0;
}
/* test hook (ls_amd.h): the row kernel of a one-process plan skips ONE row -- the first tile of XCD 0's list loses its last row, so
 * that row's y is never written (pull) or its contributions never leave (push).  Memory-safe: a shorter tile reads nothing new.
 * Returns 1 when plan data was corrupted, 0 when the plan has neither a tile map nor per-row norms (packet plans). */
int ls_amd_test_corrupt_plan(ls_amd_plan *pl) {
    if (!pl) return 0;
    if (pl->family == FAMILY_TILE_PULL && pl->n_local == 1 && pl->parts[0].d_norms && pl->parts[0].count > 0) {
        /* projected pull plans walk their tiles by arithmetic, not through the map: ONE per-row norm is doubled instead -- that
         * row's y and the contributions it makes to its partners come out wrong (plan data the kernel reads; memory-safe) */
        double v = 0;
        double *p = pl->parts[0].d_norms + pl->parts[0].count / 2;
        if (lsk_device_sync() != 0 || lsk_d2h(&v, p, sizeof(v)) != 0) return 0;
        v *= 2.0;
        return lsk_h2d(p, &v, sizeof(v)) == 0;
    }
    if (!pl->d_tilemap || pl->tilemap.slots_per_xcd <= 0) return 0;
    uint64_t e = 0;
    if (lsk_device_sync() != 0 || lsk_d2h(&e, pl->d_tilemap, sizeof(e)) != 0) return 0;
    uint64_t const rows = e >> 48;
    if (rows < 2) return 0;
    e = (e & 0xffffffffffffULL) | ((rows - 1) << 48);
    if (lsk_h2d(pl->d_tilemap, &e, sizeof(e)) != 0) return 0;
    return 1;
}
/* test hook (host only): the tile map of n rows.  Returns slots per XCD (< 0 on error); *entries is malloc'ed, free
 * with ls_amd_test_free. */
int ls_amd_test_window_find(uint64_t const *reps, int n, uint64_t key) { return lsk_test_window_find(reps, n, key); }
int ls_amd_test_nw_find(uint64_t const *reps, int n, uint64_t key) { return lsk_test_nw_find(reps, n, key); }
int ls_amd_test_chain_near_table(int elem, int ldsp, int16_t *out) { return lsk_test_chain_near_table(elem, ldsp, out); }
uint64_t ls_amd_test_rep_trivial_dihedral(uint64_t a, int L, int inv, int reflect) { return lsk_test_rep_trivial_dihedral(a, L, inv, reflect); }
int ls_amd_bench_k4(int L, int inv, int reflect, int variant, int64_t n, uint64_t const *d_reps, uint64_t *d_out, void *stream) {
    if (lsk_bench_k4(L, inv, reflect, variant, n, d_reps, d_out, stream) != 0) { set_error("%s", lsk_last_error()); return -1; }
    return 0;
}
int64_t ls_amd_test_tilemap(int64_t n, int tile_rows, int64_t chunk, uint64_t **entries) {
    int64_t slots = 0;
    *entries = NULL;
    if (tilemap_host(n, tile_rows, chunk, entries, &slots) < 0) return -1;
    return slots;
}
/* test hook (host only): the two tile maps of the paired chain plan of the weight-`weight` words of L sites.  Returns 1 and fills
 * everything, 0 when that basis has no whole paired segment (nothing is filled), < 0 on error.  out[0..4] = n, a0, a1, d, then the
 * slots per XCD of `rest` and `pairs` in out[4], out[5]. */
int ls_amd_test_tilemap_paired(int L, int weight, int tile_rows, int64_t chunk, uint64_t **rest, uint64_t **pairs, int64_t *out) {
    int64_t n = 1;
    chain_range r[CHAIN_MAX_RANGES];
    *rest = *pairs = NULL;
    if (chain_pair_ranges(L, weight, 1, ~0ULL, r) != 1) return 0;
    for (int j = 1; j <= weight; ++j) n = n * (L - weight + j) / j;
    if (tilemap_paired_host(n, tile_rows, chunk, chunk, r, 1, rest, &out[4], pairs, &out[5]) != 0) return -1;
    out[0] = n; out[1] = r[0].a0; out[2] = r[0].a1; out[3] = r[0].d;
    return 1;
}
/* test hook (host only): the same for up to `levels` levels of a ring (every bond inside a run), with the table of ranges.  Returns
 * the number of ranges (0: no whole paired segment, nothing is filled), < 0 on error.  out[0..3] = n, slots per XCD of `rest` and of
 * `pairs`, levels in use; *ranges = six int64 per range, in table order (a tile of `pairs` names its range in bits 32..47): level,
 * bond, a0, a1, d, first header of its second segments.  Free the three arrays with ls_amd_test_free. */
int ls_amd_test_tilemap_pair_levels(int L, int weight, int tile_rows, int64_t chunk, int64_t pair_chunk, int levels, uint64_t **rest,
                                    uint64_t **pairs, int64_t **ranges, int64_t *out) {
    int64_t n = 1;
    chain_range r[CHAIN_MAX_RANGES];
    *rest = *pairs = NULL;
    *ranges = NULL;
    int const nr = levels >= 1 ? chain_pair_ranges(L, weight, levels, ~0ULL, r) : 0;
    if (nr == 0) return 0;
    for (int j = 1; j <= weight; ++j) n = n * (L - weight + j) / j;
    int64_t *t = (int64_t *)malloc(sizeof(int64_t) * 6 * (size_t)nr);
    if (!t) return set_error("out of memory");
    if (tilemap_paired_host(n, tile_rows, chunk, pair_chunk, r, nr, rest, &out[1], pairs, &out[2]) != 0) { free(t); return -1; }
    for (int q = 0; q < nr; ++q) {
        int64_t const row[6] = {r[q].level, r[q].bond, r[q].a0, r[q].a1, r[q].d, r[q].hdr0};
        memcpy(t + 6 * q, row, sizeof(row));
    }
    out[0] = n; out[3] = r[nr - 1].level;
    *ranges = t;
    return nr;
}
void ls_amd_test_free(void *p) { free(p); }
/* host-only test hooks of the static index table (lsk_gtab): shape for n keys of L bits, sequential build into a malloc'ed
 * array of 2 << bbits entries (*entries, ls_amd_test_free), lookup */
int ls_amd_test_gtab_bits(int L, int64_t n) { return lsk_gtab_bits(L, n, (int64_t)1 << 40); }
int ls_amd_test_gtab_build(int L, int bbits, int64_t n, uint64_t const *reps, uint32_t const *payload, uint64_t **entries) {
    lsk_gtab t;
    t.entries = NULL; t.L = L; t.bbits = bbits; t.tbits = L - bbits;
    *entries = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)2 << bbits));
    if (lsk_test_gtab_build_host(t, *entries, n, reps, payload) != 0) { free(*entries); *entries = NULL; return -1; }
    return 0;
}
int64_t ls_amd_test_gtab_find(int L, int bbits, uint64_t const *entries, uint64_t key) {
    lsk_gtab t;
    t.entries = NULL; t.L = L; t.bbits = bbits; t.tbits = L - bbits;
    return lsk_test_gtab_find(t, entries, key);
}

/* Staged row kernel (k_chain_t, lsk.h): pull, f64 or c128 vectors, <= 64 sites, the full fixed-weight basis without
 * symmetries, a real operator made of exchange runs plus at most two other exchange pairs.  LS_AMD_ROW_KERNEL=generic keeps k_direct. */
/* Staged push (k_push_t, lsk.h): the full fixed-weight basis without symmetries, a real operator with at least one undirected
 * exchange run (what gives the near targets an LDS window is worth having for).  LS_AMD_ROW_KERNEL=generic keeps k_direct. */
static int push_staged_eligible(ls_amd_plan const *pl) {
    ls_hs_operator const *op = pl->op;
    struct ls_amd_operator_ext const *ext = OEXT(op);
    char const *e = getenv("LS_AMD_ROW_KERNEL");
    if (e && strcmp(e, "generic") == 0) return 0;
    if (NBITS(op->basis) > 64 || op->basis->spin_inversion != 0 || pl->dbs.proj != LSK_PROJ_NONE || !ext->is_real ||
        ext->runs.n_runs <= 0 || BEXT(op->basis)->hamming_weight < 0)
        return 0;
    for (int q = 0; q < ext->runs.n_runs; ++q) if (ext->runs.cnt[q] >> 16) return 0; /* directed runs: k_direct's DIRECTED instantiation */
    return 1;
}
static int chain_eligible(ls_amd_plan const *pl) {
    ls_hs_operator const *op = pl->op;
    struct ls_amd_operator_ext const *ext = OEXT(op);
    char const *e = getenv("LS_AMD_ROW_KERNEL"); /* auto (default) | generic: k_direct | pairs: k_pairs_t where it applies | pairrows / pairsites: k_pairs_row / k_pairs_site where they apply */
    if (e && (strcmp(e, "generic") == 0 || strcmp(e, "pairs") == 0 || strcmp(e, "pairrows") == 0 || strcmp(e, "pairsites") == 0)) return 0;
    int const L = NBITS(op->basis);
    int const inv = op->basis->spin_inversion != 0;
    /* Inversion sectors WITHOUT permutations (round 6; BASELINE config 1's sector, BatchedOperator.chpl:119-161): at half filling the
     * canonical state of {sigma, ~sigma} is the one with the top site clear, so the basis is the full set of weight-L/2 words of
     * L - 1 sites in the same colex order (index kind COMBINADIC with Leff = L - 1), every pair below the top site acts as in the
     * plain sector, and a pair that touches the top site ALWAYS lands on a flipped state: partner = rank(~beta), amplitude
     * s v -- a cached pair.  The ring then is a run of L - 2 bonds + two cached pairs, exactly what k_chain_t already takes. */
    if (inv && (pl->dbs.proj != LSK_PROJ_INVERSION || pl->family != FAMILY_DIRECT_PULL || (L & 1) || BEXT(op->basis)->hamming_weight != L / 2)) return 0;
    if (L > 64 || (!inv && pl->dbs.proj != LSK_PROJ_NONE) ||
        !ext->is_real || !ext->is_hermitian || ext->runs.n_runs <= 0 || ext->n_diag <= 0)
        return 0;
    int extra = 0; /* the run bond (L - 2, L - 1) leaves its run and joins the cached pairs */
    if (inv) for (int q = 0; q < ext->runs.n_runs; ++q) if (ext->runs.lo0[q] + ext->runs.cnt[q] - 1 == L - 2) extra = 1;
    if (ext->n_groups - ext->runs.n_run_groups + extra > 2) return 0;
    for (int g = ext->runs.n_run_groups; g < ext->n_groups; ++g) {
        lsk_group const *G = &ext->groups[g];
        if (G->fast != LSK_GROUP_EXCHANGE || G->v_im != 0.0 || __builtin_popcountll(G->x) != 2) return 0;
    }
    return 1;
}
/* Word tables of the wave headers (k_chain_t, lsk_chain_headers), bits 0..11 of a state being its low word:
 *   U[class_off[k] + r] = the r-th 12-bit word of weight k in ascending order (class_off[13] = 4096),
 *   Rg[w] = rank of w ^ (1 << low_site) inside its own weight class (low_site < 0: 0).
 * The 64 rows of a wave that share their bits >= 12 hold 64 consecutive entries of U, and the cached pair (low_site, a site >= 12)
 * sends row `high | w` to row Rg[w] of ONE block of rows (the header holds its start). */
static void chain_wave_tables(int low_site, uint16_t *U, uint16_t *Rg, int *class_off) {
    int pos[13];
    uint16_t rank_in[4096];
    memset(class_off, 0, sizeof(int) * 14);
    for (int w = 0; w < 4096; ++w) ++class_off[__builtin_popcount(w) + 1];
    for (int k = 0; k < 13; ++k) { class_off[k + 1] += class_off[k]; pos[k] = class_off[k]; }
    for (int w = 0; w < 4096; ++w) {
        int const k = __builtin_popcount(w);
        rank_in[w] = (uint16_t)(pos[k] - class_off[k]);
        U[pos[k]++] = (uint16_t)w;
    }
    for (int w = 0; w < 4096; ++w) Rg[w] = low_site >= 0 ? rank_in[w ^ (1 << low_site)] : 0;
}
int ls_amd_test_chain_wave_tables(int low_site, uint16_t *U, uint16_t *Rg, int *class_off) {
    if (low_site >= 12) return set_error("ls_amd_test_chain_wave_tables: the low site lies below bit 12");
    chain_wave_tables(low_site, U, Rg, class_off);
    return 0;
}
/* Wave headers of the plans with 32-bit states and ranks (k_chain_t: f64 on fused records, c128 on states + cache).  One partition, 13..32 sites, at most one cached pair, which has one site
 * below bit 12 and one at or above it (the bond that closes a ring; an open chain has none): a wave-row whose 64 rows share their
 * bits >= 12 reads an 8-byte header and 64 entries of a 16 KB table (U, Rg and the low site's bit interleaved: one 4-byte hit per
 * lane) instead of 64 8-byte records; the other wave-rows keep the records.  Every other such plan, and every plan under
 * LS_AMD_CHAIN_RECORDS=1 (A/B runs, tests), gets headers that say "records" everywhere -- the kernel reads them unconditionally.
 * Returns 1 when there is no room for them. */
static int setup_chain_headers(ls_amd_plan *pl, lsk_index index, int64_t n, uint64_t const *d_reps, int nc, uint64_t xmask, void *stream) {
    int const L = NBITS(pl->op->basis);
    char const *e = getenv("LS_AMD_CHAIN_RECORDS");
    int headed = L >= 13 && L <= 32 && pl->dbs.proj == LSK_PROJ_NONE && pl->chain_row0 == 0 &&
                 pl->family == FAMILY_DIRECT_PULL && pl->dbs.hamming_weight >= 0 && nc <= 1;
    int lo = -1, hi = -1;
    if (headed && nc == 1) {
        lo = __builtin_ctzll(xmask);
        hi = 63 - __builtin_clzll(xmask);
        if (lo >= 12 || hi < 12) { headed = 0; lo = hi = -1; }
    }
    /* (the records switch leaves the shape of the plan alone: the tiles of a plan the headers serve are paired with or without them,
     * setup_chain_pairs, so the two give the same y to the bit) */
    pl->chain_headers_apply = headed;
    if (e && atoi(e) != 0) { headed = 0; lo = hi = -1; }
    int const words = lsk_chain_words();
    int64_t const n_hdr = (n + 63) / 64;
    uint16_t U[4096], Rg[4096];
    int class_off[14];
    uint32_t *tab = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)words);
    if (!tab) return set_error("out of memory");
    chain_wave_tables(headed ? lo : -1, U, Rg, class_off);
    for (int t = 0; t < words; ++t) tab[t] = (uint32_t)U[t] | ((uint32_t)Rg[U[t]] << 16) | (lo >= 0 ? (((uint32_t)U[t] >> lo) & 1u) << 31 : 0u);
    /* [word table][headers][counter of the wave-rows without a header] */
    size_t const tab_bytes = sizeof(uint32_t) * (size_t)words, hdr_bytes = 8 * (size_t)n_hdr;
    void *q;
    if (lsk_malloc(&q, tab_bytes + hdr_bytes + 8) != 0) { free(tab); return 1; }
    unsigned long long plain = 0;
    unsigned long long *d_plain = (unsigned long long *)((char *)q + tab_bytes + hdr_bytes);
    int const rc = lsk_h2d(q, tab, tab_bytes) || lsk_h2d(d_plain, &plain, 8) ||
                   lsk_chain_headers(pl->dbs, index, n, d_reps, headed, hi, (char *)q + tab_bytes, d_plain, stream) || lsk_sync(stream) ||
                   lsk_d2h(&plain, d_plain, 8);
    free(tab);
    if (rc) { lsk_free(q); return dev_error(); }
    pl->d_chain_wave = q;
    pl->chain_headed = headed;
    /* plan bytes per row: 8 per wave-row + 64 rows of records (f64: 8 bytes; c128: the 4-byte state + 4 per cached pair) per
     * wave-row still on them, rounded up; all on records: theirs */
    int const rec = pl->cplx ? 4 + 4 * nc : 8;
    pl->chain_row_bytes = headed ? (int)((8 * (uint64_t)n_hdr + 64 * (uint64_t)rec * (uint64_t)plain + (uint64_t)n - 1) / (uint64_t)n) : rec;
    return 0;
}
/* Paired tiles (k_chain_pair_t; chain_pair_ranges, tilemap_paired_host): f64 plans on fused records that the wave headers serve (in use,
 * or all ones under LS_AMD_CHAIN_RECORDS=1: the second segments' headers follow; so: 13..32 sites, 32-bit ranks, one partition that starts at row 0, at most one cached pair) of >= 14 sites whose operator has bond
 * L - 2 inside a run and whose basis holds a whole 512-row segment of some range, down to level LS_AMD_CHAIN_PAIR_LEVELS (at 1: the top
 * bond alone) and to the first level whose bond is in no run.  The plan's tile map is rebuilt without the paired rows, which get a tile
 * map (dealt in chunks of LS_AMD_PAIR_TILE_CHUNK, default: as the other map) and a launch of their own; the second segments get headers
 * of their own (they lie off the 64-row grid), and every tile of that launch carries its range's d and bond next to its entry.
 * Every other plan, and every plan under LS_AMD_CHAIN_PAIRED=0 (A/B runs, tests), is left as it is.  hi = the cached pair's site
 * >= 12 (< 0: none).  No room for the extra arrays: the plan stays unpaired. */
static int setup_chain_pairs(ls_amd_plan *pl, lsk_index index, int64_t n, uint64_t const *d_reps, int hi, void *stream) {
    char const *e = getenv("LS_AMD_CHAIN_PAIRED");
    int const L = NBITS(pl->op->basis);
    if ((e && atoi(e) == 0) || !pl->chain_headers_apply || pl->cplx || !pl->d_chain_rec || pl->chain_cached > 1 || pl->chain_row0 != 0 ||
        pl->n_local != 1 || pl->family != FAMILY_DIRECT_PULL)
        return 0;
    uint64_t bonds = 0; /* bit b: bond (b, b + 1) lies inside an exchange run */
    for (int q = 0; q < pl->dop.runs.n_runs; ++q)
        for (int b = pl->dop.runs.lo0[q]; b < pl->dop.runs.lo0[q] + (pl->dop.runs.cnt[q] & 0xffff) && b < 64; ++b) bonds |= 1ULL << b;
    char const *le = getenv("LS_AMD_CHAIN_PAIR_LEVELS");
    int levels = le ? atoi(le) : CHAIN_PAIR_LEVELS_DEFAULT;
    if (levels < 1) levels = 1;
    chain_range rg[CHAIN_MAX_RANGES];
    int const nr = chain_pair_ranges(L, pl->dbs.hamming_weight, levels, bonds, rg);
    if (nr == 0) return 0;
    for (int r = 0; r < nr; ++r) if (rg[r].a1 + rg[r].d > n || rg[r].d < 512) return 0;
    uint64_t *rest = NULL, *pairs = NULL;
    int64_t rest_slots = 0, pair_slots = 0;
    char const *ce = getenv("LS_AMD_TILE_CHUNK"), *pe = getenv("LS_AMD_PAIR_TILE_CHUNK");
    int64_t const chunk = ce ? atoll(ce) : 256; /* (build_tilemap's default for these tiles) */
    int64_t const pair_chunk = pe ? atoll(pe) : chunk;
    if (tilemap_paired_host(n, lsk_chain_tile_rows(0), chunk > 0 ? chunk : 0, pair_chunk > 0 ? pair_chunk : 0, rg, nr, &rest, &rest_slots, &pairs,
                            &pair_slots) != 0)
        return -1;
    /* the paired map as the kernel reads it: two words per slot, the entry and d | header of the tile's second segment << 32 |
     * bond << 59 (lsk_chain_paired) */
    int64_t const n_hdr = rg[nr - 1].hdr0 + (rg[nr - 1].a1 - rg[nr - 1].a0) / 64;
    size_t const pair_words = 2 * (size_t)(8 * pair_slots);
    uint64_t *wide = (uint64_t *)calloc(pair_words, sizeof(uint64_t));
    if (!wide || n_hdr >= (1LL << 27)) { free(wide); free(rest); free(pairs); return wide ? 0 : set_error("out of memory"); }
    for (size_t q = 0; q < pair_words / 2; ++q) {
        uint64_t const en = pairs[q];
        if (!(en >> 48)) continue;
        chain_range const *r = &rg[(en >> 32) & 0xffff];
        int64_t const i0 = (int64_t)(en & 0xffffffffULL);
        wide[2 * q] = en;
        wide[2 * q + 1] = (uint64_t)r->d | (uint64_t)(r->hdr0 + (i0 - r->a0) / 64) << 32 | (uint64_t)r->bond << 59;
    }
    free(pairs);
    pairs = wide;
    void *d_rest = NULL, *d_pairs = NULL, *d_hdr = NULL;
    unsigned long long plain = 0;
    int rc = lsk_malloc(&d_rest, sizeof(uint64_t) * (size_t)(8 * rest_slots > 0 ? 8 * rest_slots : 1)) ||
             lsk_malloc(&d_pairs, sizeof(uint64_t) * pair_words) || lsk_malloc(&d_hdr, 8 * (size_t)n_hdr + 8);
    if (!rc) {
        unsigned long long *d_plain = (unsigned long long *)((char *)d_hdr + 8 * (size_t)n_hdr);
        rc = lsk_h2d(d_rest, rest, sizeof(uint64_t) * (size_t)(8 * rest_slots)) || lsk_h2d(d_pairs, pairs, sizeof(uint64_t) * pair_words) ||
             lsk_h2d(d_plain, &plain, 8);
        for (int r = 0; r < nr && !rc; ++r) /* rows of the range's second segments: [a0 + d, a1 + d) */
            rc = lsk_chain_headers(pl->dbs, index, rg[r].a1 - rg[r].a0, d_reps + rg[r].a0 + rg[r].d, pl->chain_headed, hi,
                                   (char *)d_hdr + 8 * (size_t)rg[r].hdr0, d_plain, stream);
        if (!rc) rc = lsk_sync(stream);
        if (rc) { free(rest); free(pairs); lsk_free(d_rest); lsk_free(d_pairs); lsk_free(d_hdr); return dev_error(); }
    }
    free(rest);
    free(pairs);
    if (rc) { /* no room */
        if (d_rest) lsk_free(d_rest);
        if (d_pairs) lsk_free(d_pairs);
        if (d_hdr) lsk_free(d_hdr);
        return 0;
    }
    lsk_free(pl->d_tilemap);
    pl->d_tilemap = d_rest;
    pl->tilemap.entries = (uint64_t const *)d_rest;
    pl->tilemap.slots_per_xcd = rest_slots;
    pl->d_tilemap_pair = d_pairs;
    pl->tilemap_pair.entries = (uint64_t const *)d_pairs;
    pl->tilemap_pair.slots_per_xcd = pair_slots;
    pl->d_chain_hdr_b = d_hdr;
    memset(pl->chain_pair_rows, 0, sizeof(pl->chain_pair_rows));
    for (int r = 0; r < nr; ++r) pl->chain_pair_rows[rg[r].level] += 2 * (rg[r].a1 - rg[r].a0);
    pl->chain_pair_levels = rg[nr - 1].level;
    pl->chain_paired = 1;
    return 0;
}
/* tile map with 1024-row tiles + the cache of partner ranks of the exchange pairs outside the runs (for a ring: the
 * bond that closes it) -- 4 bytes per row instead of a ranking loop of `weight` steps per row and matvec.
 * Leaves pl->has_chain == 0 (and no tile map) when a partner leaves the basis: k_direct reports that at run time,
 * as the reference does. */
static int setup_chain(ls_amd_plan *pl, lsk_index index, int64_t n, uint64_t const *d_reps, void *stream) {
    struct ls_amd_operator_ext const *ext = OEXT(pl->op);
    int nc = ext->n_groups - ext->runs.n_run_groups;
    /* the cached pairs: flip mask + amplitude.  Inversion sectors (chain_eligible): the run bond that touches the top site becomes
     * a cached pair, pairs that touch the top site carry the sector's sign, and THIS plan's copy of the run table loses that bond */
    int const Ls = NBITS(pl->op->basis);
    int const inv = pl->dbs.proj == LSK_PROJ_INVERSION;
    uint64_t const top = 1ULL << (Ls - 1);
    uint64_t cx[3];
    double cv[3];
    int k = 0;
    if (inv)
        for (int q = 0; q < pl->dop.runs.n_runs; ++q)
            if (pl->dop.runs.lo0[q] + pl->dop.runs.cnt[q] - 1 == Ls - 2) {
                cx[k] = 3ULL << (Ls - 2);
                cv[k++] = pl->dop.runs.v_re[q] * (double)pl->op->basis->spin_inversion;
                if (--pl->dop.runs.cnt[q] == 0) { /* (a run of that one bond: gone) */
                    for (int r = q; r + 1 < pl->dop.runs.n_runs; ++r) {
                        pl->dop.runs.lo0[r] = pl->dop.runs.lo0[r + 1]; pl->dop.runs.cnt[r] = pl->dop.runs.cnt[r + 1];
                        pl->dop.runs.v_re[r] = pl->dop.runs.v_re[r + 1]; pl->dop.runs.v_im[r] = pl->dop.runs.v_im[r + 1];
                    }
                    --pl->dop.runs.n_runs;
                }
                break;
            }
    for (int g = ext->runs.n_run_groups; g < ext->n_groups && k < 3; ++g) {
        cx[k] = ext->groups[g].x;
        cv[k++] = ext->groups[g].v_re * ((inv && (ext->groups[g].x & top)) ? (double)pl->op->basis->spin_inversion : 1.0);
    }
    nc = k;
    if (nc > 2) return 0;
    /* ranks are 32-bit while the whole basis (index.count states: x is indexed by global rank) has < 2^32 - 1 states;
     * LS_AMD_CHAIN_WIDE=1 forces the 64-bit instantiation (test hook: no in-tree config is that large) */
    char const *ew = getenv("LS_AMD_CHAIN_WIDE");
    pl->chain_wide = index.count >= 0xffffffffLL || (ew && atoi(ew) != 0 && NBITS(pl->op->basis) > 32);
    size_t const es = pl->chain_wide ? sizeof(uint64_t) : sizeof(uint32_t);
    if (nc > 0 && n > 0) {
        void *q;
        if (lsk_malloc(&q, es * (size_t)nc * (size_t)n) != 0) return 0; /* no room for the cache: k_direct */
        pl->d_chain_cache = q;
        int zero = 0, flag = 0;
        DEV(lsk_h2d(pl->d_err, &zero, sizeof(int)));
        for (int c = 0; c < nc; ++c)
            DEV(lsk_chain_cache(pl->dbs, index, n, d_reps, cx[c],
                                (char *)pl->d_chain_cache + es * (size_t)c * (size_t)n, pl->chain_wide, pl->d_err, stream));
        DEV(lsk_sync(stream));
        DEV(lsk_d2h(&flag, pl->d_err, sizeof(int)));
        DEV(lsk_h2d(pl->d_err, &zero, sizeof(int)));
        if (flag) {
            lsk_free(pl->d_chain_cache);
            pl->d_chain_cache = NULL;
            return 0;
        }
        pl->chain_cached = nc;
        pl->chain_v[0] = cv[0];
        pl->chain_v[1] = nc > 1 ? cv[1] : 0.0;
    }
    if (build_tilemap(pl, n, lsk_chain_tile_rows(pl->cplx)) != 0) return -1;
    /* 32-bit states and ranks, f64 vectors: state and partner rank of the first cached pair are fused into one 8-byte
     * record per row (8 instead of 8 + 4 bytes per row from HBM, one load instead of two: measured on chain_32
     * 8.59 -> 8.41 ms; c128: 15.40 -> 15.70 ms, so complex vectors keep the two arrays).  This shape has no unfused
     * instantiation (it sat at 98 SGPRs, one resident block per CU short); a second cached pair stays in the cache
     * array, whose layout [pair][row] is what the kernel indexes.  No room for the records: the generic row kernel. */
    if (!pl->cplx && NBITS(pl->op->basis) <= 32 && !pl->chain_wide && n > 0) {
        void *q;
        if (lsk_malloc(&q, sizeof(uint64_t) * (size_t)n) != 0) {
            if (pl->d_chain_cache) { lsk_free(pl->d_chain_cache); pl->d_chain_cache = NULL; }
            if (pl->d_tilemap) { lsk_free(pl->d_tilemap); pl->d_tilemap = NULL; memset(&pl->tilemap, 0, sizeof(pl->tilemap)); }
            pl->chain_cached = 0;
            return 0;
        }
        pl->d_chain_rec = (uint64_t *)q;
        DEV(lsk_chain_pack(n, d_reps, pl->chain_cached ? pl->d_chain_cache : NULL, (uint64_t *)q, stream));
        DEV(lsk_sync(stream));
        if (pl->chain_cached <= 1 && pl->d_chain_cache) { lsk_free(pl->d_chain_cache); pl->d_chain_cache = NULL; }
    }
    if (NBITS(pl->op->basis) <= 32 && !pl->chain_wide && n > 0) { /* (f64 on the records, c128 on its two arrays) */
        int const rc = setup_chain_headers(pl, index, n, d_reps, pl->chain_cached, pl->chain_cached > 0 ? cx[0] : 0, stream);
        if (rc < 0) return -1;
        if (rc > 0) { /* no room: the generic row kernel */
            if (pl->d_chain_rec) { lsk_free(pl->d_chain_rec); pl->d_chain_rec = NULL; }
            if (pl->d_chain_cache) { lsk_free(pl->d_chain_cache); pl->d_chain_cache = NULL; }
            if (pl->d_tilemap) { lsk_free(pl->d_tilemap); pl->d_tilemap = NULL; memset(&pl->tilemap, 0, sizeof(pl->tilemap)); }
            pl->chain_cached = 0;
            return 0;
        }
        if (setup_chain_pairs(pl, index, n, d_reps, pl->chain_cached > 0 ? 63 - __builtin_clzll(cx[0]) : -1, stream) != 0) return -1;
    }
    pl->has_chain = 1;
    return 0;
}

/* Staged row kernel for arbitrary exchange pairs (k_pairs_t, lsk.h): pull, the full fixed-weight basis of <= 32 sites without
 * symmetries, a real Hermitian operator whose off-diagonal groups are all exchange pairs (any two sites, any real amplitude)
 * and whose diagonal terms are zz terms on those same pairs -- Heisenberg / XXZ on any lattice.  Rings and open chains keep
 * k_chain_t.  LS_AMD_ROW_KERNEL=generic keeps the generic row kernel (k_direct), =pairs sends rings here too. */
static int pair_cmp(void const *pa, void const *pb) {
    lsk_pair const *a = (lsk_pair const *)pa, *b = (lsk_pair const *)pb;
    int const ca = a->j < 11 ? 0 : (a->i < 11 ? 1 : 2), cb = b->j < 11 ? 0 : (b->i < 11 ? 1 : 2);
    if (ca != cb) return ca - cb;
    if (a->i != b->i) return (int)a->i - (int)b->i;
    return (int)a->j - (int)b->j;
}
static int setup_pairs(ls_amd_plan *pl, int64_t n, uint64_t const *d_reps, void *stream) {
    ls_hs_operator const *op = pl->op;
    struct ls_amd_operator_ext const *ext = OEXT(op);
    int const L = NBITS(op->basis), hw = BEXT(op->basis)->hamming_weight;
    char const *e = getenv("LS_AMD_ROW_KERNEL");
    if (e && strcmp(e, "generic") == 0) return 0;
    int const wide = L > 32; /* 33..64 sites (round 6): the kernel streams the 8-byte representatives themselves */
    if (L > 64 || hw < 0 || hw + 2 > LSK_PAIR_KC || op->basis->spin_inversion != 0 || pl->dbs.proj != LSK_PROJ_NONE || !ext->is_real ||
        !ext->is_hermitian || ext->n_groups < 1 || ext->n_groups > LSK_MAX_PAIRS || n <= 0 || n >= 0xffffffffLL ||
        ext->n_diag <= 0) /* (no diagonal terms: y is accumulated into, DMV:1062-1063 -- left to the generic kernel) */
        return 0;
    /* The kernel walks the basis in blocks "all 11-bit low words of weight kl under one high part": C(11, kl) rows, kl ~ 11 hw / L on
     * average.  Far from half filling the blocks are a handful of rows, a wave spans many of them and prices its HIGH / STRADDLE pairs
     * once per block: measured on a 36-site square lattice (profiles/r6_widen_bench.txt) weight 6 -- kl ~ 1.8 -- 1.09 ms against 0.25 ms
     * of the generic row kernel, weight 9 -- kl ~ 2.75 -- 15.3 against 14.3 ms.  Such bases keep k_direct (LS_AMD_ROW_KERNEL=pairs forces
     * the staged kernel: tests). */
    /* Round 6: those bases take the one-row-per-lane variant of the same plan instead (k_pairs_row: O(1) rank shifts out of per-row
     * prefix arrays in LDS), which leaves the generic kernel behind at any filling; LS_AMD_ROW_KERNEL=pairrows forces it everywhere. */
    int const force_sites = e && strcmp(e, "pairsites") == 0;
    int const by_row = force_sites || (e && strcmp(e, "pairrows") == 0) || (!(e && strcmp(e, "pairs") == 0) && (11 * hw < 4 * L || 11 * (L - hw) < 4 * L));
    lsk_pair recs[LSK_MAX_PAIRS];
    memset(recs, 0, sizeof(recs));
    for (int g = 0; g < ext->n_groups; ++g) {
        lsk_group const *G = &ext->groups[g];
        if (G->fast != LSK_GROUP_EXCHANGE || G->v_im != 0.0 || __builtin_popcountll(G->x) != 2) return 0;
        recs[g].i = (uint8_t)__builtin_ctzll(G->x);
        recs[g].j = (uint8_t)(63 - __builtin_clzll(G->x));
        recs[g].v = G->v_re;
    }
    double dsum = 0.0;
    for (int t = 0; t < ext->n_diag; ++t) { /* every diagonal term must be a zz term on one of the pairs */
        lsk_term const *T = &ext->diag[t];
        if (T->m != 0 || T->r != 0 || T->v_im != 0.0) return 0;
        int g = 0;
        while (g < ext->n_groups && ext->groups[g].x != T->s) ++g;
        if (g == ext->n_groups) return 0;
        recs[g].vz += T->v_re;
        dsum += T->v_re;
    }
    qsort(recs, (size_t)ext->n_groups, sizeof(lsk_pair), pair_cmp);
    lsk_pairplan pp;
    memset(&pp, 0, sizeof(pp));
    for (int g = 0; g < ext->n_groups; ++g) {
        if (recs[g].j < 11) ++pp.n_near; else if (recs[g].i < 11) ++pp.n_str; else ++pp.n_high;
    }
    pp.dsum = dsum;
    uint16_t rank_low[2048];
    for (int w = 0; w < 2048; ++w) {
        uint64_t r = 0;
        int k = 0;
        for (int b = 0; b < 11; ++b) if ((w >> b) & 1) r += binom(b, ++k);
        rank_low[w] = (uint16_t)r;
    }
    int const nbits = wide ? 64 : 32;
    uint32_t bin[64 * LSK_PAIR_KC]; /* (entries no valid state of a basis with < 2^32 states can touch are truncated: never read for a live lane) */
    for (int a = 0; a < nbits; ++a) for (int k = 0; k < LSK_PAIR_KC; ++k) bin[a * LSK_PAIR_KC + k] = (uint32_t)binom(a, k);
    void *q = NULL;
    if (!wide) {
        if (lsk_malloc(&q, 4 * (size_t)n) != 0) return 0; /* no room for the 4-byte states: the generic kernel */
        pl->d_states32 = q;
    }
    if (upload(&pl->d_pair_recs, recs, sizeof(lsk_pair) * (size_t)ext->n_groups) != 0 || upload(&pl->d_rank_low, rank_low, sizeof(rank_low)) != 0 ||
        upload(&pl->d_pair_binom, bin, sizeof(uint32_t) * (size_t)nbits * LSK_PAIR_KC) != 0)
        return -1;
    if (!wide) DEV(lsk_narrow_states(n, d_reps, (uint32_t *)pl->d_states32, stream));
    if (by_row) {
        lsk_pair_row rr[LSK_MAX_PAIRS];
        memset(rr, 0, sizeof(rr));
        for (int g = 0; g < ext->n_groups; ++g) {
            int const i = recs[g].i, j = recs[g].j;
            rr[g].i = i;
            rr[g].j = j;
            rr[g].between = ((1ULL << j) - 1) & ~((2ULL << i) - 1);
            rr[g].v = recs[g].v;
            rr[g].vz = recs[g].vz;
        }
        if (upload(&pl->d_pair_rows, rr, sizeof(lsk_pair_row) * (size_t)ext->n_groups) != 0) return -1;
        pp.rows = (lsk_pair_row const *)pl->d_pair_rows;
        /* ... or walking the particles of the row: weight x degree candidates instead of all pairs (k_pairs_site is bound by VALU
         * issue, ~30 instructions per candidate against ~47 per pair of k_pairs_row).  LS_AMD_ROW_KERNEL=pairsites forces it while
         * the degree fits the table, =pairrows keeps the pair loop. */
        int deg[64] = {0}, dmax = 0;
        for (int g = 0; g < ext->n_groups; ++g) { ++deg[recs[g].i]; ++deg[recs[g].j]; }
        for (int q = 0; q < L; ++q) if (deg[q] > dmax) dmax = deg[q];
        int const D = dmax <= 4 ? 4 : 8;
        if (dmax <= LSK_PAIR_SITE_MAX_DEGREE && !(e && strcmp(e, "pairrows") == 0) && (force_sites || 2 * hw * D <= 3 * ext->n_groups)) {
            /* amplitude classes: distinct (v, vz) */
            double cv[LSK_PAIR_SITE_MAX_CLASSES], cz[LSK_PAIR_SITE_MAX_CLASSES];
            uint8_t cls_of[LSK_MAX_PAIRS];
            int n_cls = 0, ok = 1;
            for (int g = 0; g < ext->n_groups && ok; ++g) {
                int c = 0;
                while (c < n_cls && !(cv[c] == recs[g].v && cz[c] == recs[g].vz)) ++c;
                if (c == n_cls) {
                    if (n_cls == LSK_PAIR_SITE_MAX_CLASSES) { ok = 0; break; }
                    cv[c] = recs[g].v;
                    cz[c] = recs[g].vz;
                    ++n_cls;
                }
                cls_of[g] = (uint8_t)c;
            }
            if (ok) {
                int const DW = D / 4, amp_at = (2 * L * DW + 3) & ~3, words = amp_at + 4 * n_cls;
                uint32_t *tab = (uint32_t *)calloc((size_t)words, sizeof(uint32_t));
                if (!tab) return -1;
                uint8_t *nb = (uint8_t *)tab, *cl = (uint8_t *)(tab + L * DW);
                for (int q = 0; q < L; ++q) for (int d = 0; d < D; ++d) nb[q * D + d] = (uint8_t)q; /* padding: the site itself */
                int fill[64] = {0};
                for (int g = 0; g < ext->n_groups; ++g) {
                    int const ends[2] = {recs[g].i, recs[g].j};
                    for (int side = 0; side < 2; ++side) {
                        int const p = ends[side], d = fill[p]++;
                        nb[p * D + d] = (uint8_t)ends[1 - side];
                        cl[p * D + d] = cls_of[g];
                    }
                }
                double *amp = (double *)(tab + amp_at);
                for (int c = 0; c < n_cls; ++c) { amp[2 * c] = cv[c]; amp[2 * c + 1] = cz[c]; }
                int const up = upload(&pl->d_pair_sites, tab, sizeof(uint32_t) * (size_t)words);
                free(tab);
                if (up != 0) return -1;
                pp.sites = (uint32_t const *)pl->d_pair_sites;
                pp.n_classes = n_cls;
                pp.site_words = words;
                pp.n_sites = L;
                pp.degree = D;
            }
        }
    }
    pp.pairs = (lsk_pair const *)pl->d_pair_recs;
    pp.rank_low = (uint16_t const *)pl->d_rank_low;
    pp.binom = (uint32_t const *)pl->d_pair_binom;
    pp.states = wide ? (void const *)d_reps : (void const *)pl->d_states32;
    pp.wide = wide;
    if (build_tilemap(pl, n, by_row ? 256 : lsk_pairs_tile_rows(pl->cplx)) != 0) return -1;
    pl->pairs = pp;
    pl->has_pairs = 1;
    return 0;
}

/* Pre-indexed packets: for a hash partition of an UNPROJECTED fixed-weight basis every rank can
 * derive, alone, where any state sits inside its owner's block -- global colex rank (closed form) -> entry [rank / 64][owner] of the
 * all-destinations directory -> prefix + popcount.  The producer then sends (u32 index, value) = 12 bytes (20 for c128) instead
 * of (u64 state, value) = 16 (24), the exchange shrinks by a quarter (a sixth), and the consumer is one streaming read + one
 * atomic per packet.  Costs P / 4 bytes of HBM per basis state on every rank (chain_32 at 8 ranks: 1.2 GB; the per-rank data of the
 * packet strategy stays O(N / P) otherwise), so it is taken only while it fits LS_AMD_PACKET_INDEX_MAX bytes (default: a quarter
 * of the free HBM); LS_AMD_PACKET_INDEX=0 keeps the state-carrying packets (also the path of every projected basis, whose
 * representatives no closed form ranks), =1 takes the indexed ones also for logical partitions inside one process. */
static int packets_wave_rings(void);
/* dist.c: the packet layout is one decision of all ranks -- a rank whose peers could not build the directory re-creates its plan
 * with state-carrying packets (thread-local: loop-back ranks are threads) */
static __thread int g_no_packet_index = 0;
void ls_amd_internal_set_no_packet_index(int v) { g_no_packet_index = v; }
/* bytes of the key array (states or indices) of a segment of c packets: the values behind it stay 8-byte aligned */
static int64_t segment_key_bytes(ls_amd_plan const *pl, int64_t c) { return pl->key_bytes == 4 ? ((4 * c + 7) & ~(int64_t)7) : 8 * c; }
/* Sorted packet streams (k_packets.hip, k_tile_st / k_window) for the partitions of ONE process: every off-diagonal group must be an
 * exchange pair -- a packet exists iff alpha is anti-aligned on the pair, and beta - alpha is then one of two constants -- on an
 * unprojected fixed-weight basis (the conditions of the pre-indexed packets, which setup_packet_index checks).
 * LS_AMD_PACKET_STREAMS=0: the atomics of lsk_scatter_parts / lsk_scatter_idx instead (A/B). */
/* A plan that owns ONE partition is driven by generate / exchange / scatter: only a driver that knows the streams (dist.c: the
 * stream offsets of every source are exchanged at set-up, the own segment is consumed out of the send buffer) asks for them */
static __thread int g_want_streams = 0;
void ls_amd_internal_set_want_streams(int v) { g_want_streams = v; }
/* the static part of the conditions (operator and basis): dist.c sizes its rounds by it before the plan exists */
int ls_amd_internal_streams_eligible(ls_hs_operator const *op, int P) {
    char const *e = getenv("LS_AMD_PACKET_STREAMS");
    if (e && atoi(e) == 0) return 0;
    e = getenv("LS_AMD_PACKET_INDEX"); /* (the streams are made of pre-indexed packets: switched off with them) */
    if (e && atoi(e) == 0) return 0;
    ls_hs_basis const *b = op->basis;
    /* (P == 1: every packet is an own-partition packet, whose atomics in the producer meet ~8 packets per line of y -- measured on
     * chain_32 with one rank: 97 ms with them against 148 ms through 2 x 119 GB of streams) */
    if (BEXT(b)->order > 1 || b->spin_inversion != 0 || BEXT(b)->hamming_weight < 0 || P < 2 || P > LSK_MAX_SEGS) return 0;
    struct ls_amd_operator_ext const *oe = OEXT(op);
    if (oe->n_groups < 1 || oe->n_groups > 128 || P * 2 * oe->n_groups > lsk_tile_st_max_classes()) return 0;
    for (int g = 0; g < oe->n_groups; ++g)
        if (oe->groups[g].fast != LSK_GROUP_EXCHANGE || __builtin_popcountll(oe->groups[g].x) != 2) return 0;
    return 1;
}
static __thread int g_no_streams = 0; /* set while a plan whose stream buffers did not fit is created again with the atomic consumers */
static int streams_wanted(ls_amd_plan const *pl) {
    if (g_no_streams || (pl->me >= 0 && !g_want_streams) || pl->family != FAMILY_TILE || pl->dbs.proj != LSK_PROJ_NONE) return 0;
    return ls_amd_internal_streams_eligible(pl->op, pl->P);
}
static int setup_packet_index(ls_amd_plan *pl, uint64_t const *const *d_reps, int64_t const *counts, void *stream) {
    ls_hs_basis const *b = pl->op->basis;
    int const L = NBITS(b), h = BEXT(b)->hamming_weight, P = pl->P;
    char const *e = getenv("LS_AMD_PACKET_INDEX");
    int const for_streams = streams_wanted(pl); /* the streams need every packet's index at its destination */
    if ((e && atoi(e) == 0) || g_no_packet_index) return 0;
    /* Default: only where packets cross a wire (one partition per process).  With all partitions in one process the "exchange" is a
     * pointer hand-off, and on one device the directory costs the producers more than it saves the consumers (chain_28 x 8: 23.5
     * against 22.6 ms, chain_30 x 8: 97.7 against 92.2 -- profiles/r5_packets_preindexed_ab.txt: the consumers are bound by their
     * atomics, not by the rank directory look-up they lose).  LS_AMD_PACKET_INDEX=1 forces it there too (tests, A/B). */
    if (pl->me < 0 && !(e && atoi(e) == 1) && !for_streams) return 0;
    if (pl->dbs.proj == LSK_PROJ_FULL || h < 0 || h >= LSK_BINOM_K - 1 || L > 64 || P > lsk_tile_wv_max_parts() || P > LSK_MAX_SEGS ||
        !packets_wave_rings()) return 0;
    for (int i = 0; i < pl->n_local; ++i) if (counts[i] >= 0xffffffffLL) return 0;
    int const sites = L - (b->spin_inversion != 0 ? 1 : 0); /* inversion sectors: the canonical states have the top site bit clear */
    uint64_t const n_ranks = binom(sites, h);
    if (n_ranks == 0 || n_ranks >= ((uint64_t)1 << 40)) return 0;
    int64_t const words = (int64_t)((n_ranks + 63) / 64);
    size_t const bytes = sizeof(lsk_rankdir) * (size_t)words * (size_t)P;
    size_t fr = 0, tot = 0, ceiling;
    if (lsk_mem_info(&fr, &tot) != 0) return 0;
    e = getenv("LS_AMD_PACKET_INDEX_MAX");
    ceiling = e && atoll(e) > 0 ? (size_t)atoll(e) : fr / 4;
    uint64_t const *d_binom;
    if (device_binom(&d_binom) != 0) return -1;
    /* Sorted streams with GLOBAL-RANK keys (round 6): the key of a packet is the colex rank of beta among all states of
     * the weight -- the producer needs NO directory (the rank is alpha's +- one binomial on adjacent pairs, a rank sum otherwise) and
     * the consumer translates rank -> row through its OWN partition's rank directory (lsk_rankdir, built with the partition's index:
     * 1 / 4 byte per global state whatever P).  The all-destinations directory -- P / 4 bytes per global state on EVERY rank, 1.2 GB
     * for chain_32 at 8 ranks -- is then not built at all.  Needs < 2^32 global ranks (u32 keys); LS_AMD_STREAM_KEYS=index keeps the
     * round-5 form (index at the destination out of the all-destinations directory). */
    e = getenv("LS_AMD_STREAM_KEYS");
    if (for_streams && n_ranks < 0xffffffffULL && !(e && strcmp(e, "index") == 0)) {
        memset(&pl->gd, 0, sizeof(pl->gd));
        pl->gd.entries = NULL; pl->gd.P = P; pl->gd.sites = L; pl->gd.weight = h; pl->gd.n_ranks = (int64_t)n_ranks;
        pl->key_bytes = 4;
        pl->stream_gkeys = 1;
        pl->streams = 1;
        pl->st_S = 2 * OEXT(pl->op)->n_groups;
        pl->st_tile_rows = 256;
        return 0;
    }
    if (bytes > ceiling) return 0; /* does not fit: the packets carry the state and the consumers rank it (O(N / P) memory) */
    void *p = NULL;
    if (lsk_malloc(&p, bytes) != 0) return 0;
    lsk_gdir gd;
    memset(&gd, 0, sizeof(gd));
    gd.entries = (lsk_rankdir const *)p; gd.P = P; gd.sites = L; gd.weight = h; gd.n_ranks = (int64_t)n_ranks;
    int zero = 0, flag = 1;
    int ok = lsk_h2d(pl->d_err, &zero, sizeof(int)) == 0 && lsk_gdir_build(gd, (lsk_rankdir *)p, d_binom, stream) == 0;
    /* self-check: every state this process owns must come back as (its partition, its position) */
    for (int i = 0; ok && i < pl->n_local; ++i)
        ok = lsk_gdir_check(gd, pl->me < 0 ? i : pl->me, counts[i], d_reps[i], d_binom, pl->d_err, stream) == 0;
    ok = ok && lsk_sync(stream) == 0 && lsk_d2h(&flag, pl->d_err, sizeof(int)) == 0 && flag == 0;
    (void)lsk_h2d(pl->d_err, &zero, sizeof(int));
    if (!ok) { lsk_free(p); return 0; } /* not the full fixed-weight basis (or no room for the scans): state-carrying packets */
    pl->gd = gd;
    pl->d_gdir = (lsk_rankdir *)p;
    pl->key_bytes = 4;
    if (for_streams) {
        pl->streams = 1;
        pl->st_S = 2 * OEXT(pl->op)->n_groups;
        pl->st_tile_rows = 256;
    }
    return 0;
}

/* Species-split row kernel (k_hubbard, lsk.h): one process, pull, a Hermitian operator on the spinful product basis whose every
 * off-diagonal group lives inside one species half (support of x, m and s) -- Hubbard hopping of any range and phase, one-species
 * density-assisted terms; the diagonal is arbitrary.  The tables hold <row word|H|partner word> for every word of a species and
 * every group of that species whose partner has the species' weight: O(C(L, N_up) + C(L, N_down)) entries, never O(nnz).
 * LS_AMD_ROW_KERNEL=generic keeps k_direct. */
static int hubbard_species(ls_amd_plan *pl, int half, int weight, lsk_species *sp, void **d_words, void **d_rank, void **d_coef,
                           int64_t *nnz_words) {
    struct ls_amd_operator_ext const *ext = OEXT(pl->op);
    int const L = pl->op->basis->number_sites, shift = half ? L : 0;
    uint64_t const hmask = ((1ULL << L) - 1) << shift;
    int64_t const n = (int64_t)binom(L, weight);
    int const cc = pl->hubbard.cplx_coef;
    int *gs = (int *)malloc(sizeof(int) * (ext->n_groups > 0 ? ext->n_groups : 1));
    int ng = 0;
    if (gs) for (int g = 0; g < ext->n_groups; ++g) if ((ext->groups[g].x & hmask) != 0) gs[ng++] = g;
    uint32_t *words = (uint32_t *)malloc(4 * (size_t)n);
    int *cnt = (int *)calloc((size_t)n, sizeof(int));
    int deg = 0;
    uint32_t *rank = (uint32_t *)malloc(4 * (size_t)n * (ng > 0 ? ng : 1));
    double *coef = (double *)malloc(8 * (size_t)(cc ? 2 : 1) * n * (ng > 0 ? ng : 1));
    if (!gs || !words || !cnt || !rank || !coef) {
        free(gs); free(words); free(cnt); free(rank); free(coef);
        return set_error("species tables: out of host memory");
    }
    for (int64_t a = 0; a < n; ++a) words[a] = (uint32_t)ls_hs_fixed_hamming_index_to_state((ptrdiff_t)a, weight);
    for (int64_t a = 0; a < n; ++a) {
        int k = 0;
        for (int q = 0; q < ng; ++q) {
            lsk_group const *G = &ext->groups[gs[q]];
            uint64_t const partner = ((uint64_t)words[a] << shift) ^ G->x;
            if (__builtin_popcountll(partner) != weight) continue;
            double re, im;
            eval_terms(ext->off, G->begin, G->end, partner, &re, &im); /* the partner's expansion reaches this row with <row|H|partner> */
            if (re == 0.0 && im == 0.0) continue;
            int64_t const r = (int64_t)ls_hs_fixed_hamming_state_to_index(partner >> shift);
            int64_t const e = (int64_t)k * n + a; /* [slot][word]: filled below in the final layout once deg is known */
            rank[e] = (uint32_t)r;
            if (cc) { coef[2 * e] = re; coef[2 * e + 1] = im; } else coef[e] = re;
            ++k;
        }
        cnt[a] = k;
        if (k > deg) deg = k;
    }
    /* the slots were written with stride n for slot k, i.e. already [slot][word]; pad every word to deg with (self, 0) */
    int64_t active = 0;
    for (int64_t a = 0; a < n; ++a) {
        active += cnt[a];
        for (int k = cnt[a]; k < deg; ++k) {
            int64_t const e = (int64_t)k * n + a;
            rank[e] = (uint32_t)a;
            if (cc) { coef[2 * e] = 0.0; coef[2 * e + 1] = 0.0; } else coef[e] = 0.0;
        }
    }
    int rc = upload(d_words, words, 4 * (size_t)n) || upload(d_rank, rank, 4 * (size_t)n * (deg > 0 ? deg : 1)) ||
             upload(d_coef, coef, 8 * (size_t)(cc ? 2 : 1) * n * (deg > 0 ? deg : 1));
    free(gs); free(words); free(cnt); free(rank); free(coef);
    if (rc) return -1;
    sp->n = n;
    sp->deg = deg;
    sp->words = (uint32_t const *)*d_words;
    sp->rank = (uint32_t const *)*d_rank;
    sp->coef = (double const *)*d_coef;
    *nnz_words = active;
    return 0;
}
static int setup_hubbard(ls_amd_plan *pl, part_state const *ps, void *stream) {
    ls_hs_basis const *b = pl->op->basis;
    struct ls_amd_basis_ext const *be = BEXT(b);
    struct ls_amd_operator_ext const *ext = OEXT(pl->op);
    char const *env = getenv("LS_AMD_ROW_KERNEL");
    if (env && strcmp(env, "generic") == 0) return 0;
    if (!be->product || pl->P != 1 || pl->n_local != 1 || pl->family != FAMILY_DIRECT_PULL || !ext->is_hermitian) return 0;
    int const L = b->number_sites;
    uint64_t const lo = (1ULL << L) - 1, hi = lo << L;
    for (int g = 0; g < ext->n_groups; ++g) { /* separable: every group inside one species half */
        lsk_group const *G = &ext->groups[g];
        uint64_t support = G->x;
        for (int k = G->begin; k < G->end; ++k) support |= ext->off[k].m | ext->off[k].s;
        if ((support & lo) && (support & hi)) return 0;
    }
    int64_t const na = (int64_t)binom(L, be->prod_up), nb = (int64_t)binom(L, be->prod_dn);
    /* the rows must be the product basis in its own order (plan_setup_part verified it: the plan's index is then PRODUCT) */
    if (ps->index.kind != LSK_INDEX_PRODUCT || ps->count != na * nb || na > ((int64_t)1 << 26) || nb > ((int64_t)1 << 26)) return 0;
    memset(&pl->hubbard, 0, sizeof(pl->hubbard));
    pl->hubbard.L = L;
    pl->hubbard.cplx_coef = !ext->is_real;
    int64_t act_up = 0, act_dn = 0;
    if (hubbard_species(pl, 0, be->prod_up, &pl->hubbard.up, &pl->d_hub[0], &pl->d_hub[1], &pl->d_hub[2], &act_up) != 0 ||
        hubbard_species(pl, 1, be->prod_dn, &pl->hubbard.dn, &pl->d_hub[3], &pl->d_hub[4], &pl->d_hub[5], &act_dn) != 0)
        return -1;
    if (build_tilemap(pl, ps->count, 256) != 0) return -1;
    pl->nnz = act_up * nb + act_dn * na; /* off-diagonal non-zeros */
    pl->has_hubbard = 1;
    return 0;
}

static int plan_setup_part(ls_amd_plan *pl, part_state *ps, int part_id, int num_rounds, void *stream) {
    ls_hs_basis const *b = pl->op->basis;
    int const L = NBITS(b);
    int const h = BEXT(b)->hamming_weight;
    uint64_t const *d_binom;
    if (device_binom(&d_binom) != 0) return -1;
    ps->index.count = ps->count;
    ps->index.reps = ps->d_reps;
    ps->index.binom = d_binom;
    ps->index.table = NULL;
    ps->index.shift = 0;
    ps->index.kind = LSK_INDEX_SEARCH;
    int closed_form = 0;
    if (pl->P == 1 && pl->dbs.proj != LSK_PROJ_FULL && pl->family != FAMILY_TILE) {
        int const Leff = L - (b->spin_inversion != 0 ? 1 : 0);
        if (h < 0) {
            if (Leff < 63 && ps->count == ((int64_t)1 << Leff)) { ps->index.kind = LSK_INDEX_IDENTITY; closed_form = 1; }
        } else if ((uint64_t)ps->count == binom(Leff, h) && ps->count > 0) {
            /* the basis should be the full fixed-Hamming prefix: verify on the device */
            int zero = 0, flag = 0;
            DEV(lsk_h2d(pl->d_err, &zero, sizeof(int)));
            DEV(lsk_check_combinadic(ps->index, h, ps->count, ps->d_reps, pl->d_err, stream));
            DEV(lsk_sync(stream));
            DEV(lsk_d2h(&flag, pl->d_err, sizeof(int)));
            DEV(lsk_h2d(pl->d_err, &zero, sizeof(int)));
            if (!flag) { ps->index.kind = LSK_INDEX_COMBINADIC; closed_form = 1; }
        }
    }
    if (!closed_form && pl->P == 1 && !pl->global_index && (pl->family == FAMILY_DIRECT_PULL || pl->family == FAMILY_DIRECT_PUSH) &&
        BEXT(b)->product && !BEXT(b)->fermi && ps->count > 0) {
        /* the spinful product basis in its own order: two closed-form ranks (LSK_INDEX_PRODUCT), verified on the device */
        lsk_index pix = ps->index;
        pix.kind = LSK_INDEX_PRODUCT;
        pix.prod_sites = b->number_sites; pix.prod_up = BEXT(b)->prod_up; pix.prod_dn = BEXT(b)->prod_dn;
        pix.prod_na = (int64_t)binom(b->number_sites, BEXT(b)->prod_up);
        if (ps->count == pix.prod_na * (int64_t)binom(b->number_sites, BEXT(b)->prod_dn)) {
            int zero = 0, flag = 0;
            DEV(lsk_h2d(pl->d_err, &zero, sizeof(int)));
            DEV(lsk_check_product(pix, ps->count, ps->d_reps, pl->d_err, stream));
            DEV(lsk_sync(stream));
            DEV(lsk_d2h(&flag, pl->d_err, sizeof(int)));
            DEV(lsk_h2d(pl->d_err, &zero, sizeof(int)));
            if (!flag) { ps->index = pix; closed_form = 1; }
        }
    }
    if (pl->P == 1 && pl->family == FAMILY_TILE && pl->dbs.proj == LSK_PROJ_NONE && b->spin_inversion == 0 && h >= 0 &&
        (uint64_t)ps->count == binom(L, h) && ps->count > 0) {
        /* ONE rank drives this plan through generate / exchange / scatter (dist.c) and owns the whole basis: every packet is its own.
         * When the basis is the full fixed-weight set the producer can be the staged push kernel (k_push_t), which scatters them
         * itself -- verified here, decided at the end of the set-up (ls_amd_plan_create). */
        int zero = 0, flag = 0;
        lsk_index cix = ps->index;
        cix.kind = LSK_INDEX_COMBINADIC;
        DEV(lsk_h2d(pl->d_err, &zero, sizeof(int)));
        DEV(lsk_check_combinadic(cix, h, ps->count, ps->d_reps, pl->d_err, stream));
        DEV(lsk_sync(stream));
        DEV(lsk_d2h(&flag, pl->d_err, sizeof(int)));
        DEV(lsk_h2d(pl->d_err, &zero, sizeof(int)));
        pl->one_rank_full_basis = !flag;
    }
    if (!closed_form && ps->count > 0) {
        if (build_search_index(ps, L, stream) != 0) return -1;
    }
    /* Packet plans over a hash partition of an unprojected fixed-weight basis: the global rank of a state is closed-form, the
     * local index is a popcount away (lsk_rankdir) -- one 16-byte load per packet in k_scatter / k_tile_wv instead of the prefix
     * table and the 3-4 dependent probes of the binary search.  C(L, h) / 4 bytes per partition; the search index stays as the
     * fallback (no room, a state of another weight) and for every other caller.  chain_28 x 8 partitions 23.7 -> 22.3 ms, x 2
     * partitions 12.0 -> 10.2 ms, chain_30 x 8 98.0 -> 91.7 ms (profiles/r4_packets_rank_directory_ab.txt).  (Inversion sectors qualify: the canonical
     * state of a pair has the same weight at half filling, which is the only filling they exist at.) */
    if (pl->family == FAMILY_TILE && !pl->d_gdir /* pre-indexed packets need no per-partition directory */ &&
        pl->dbs.proj != LSK_PROJ_FULL && h >= 0 && h < LSK_BINOM_K - 1 && L <= 64 && ps->count > 0 &&
        ps->count < 0xffffffffLL && ps->index.kind == LSK_INDEX_SEARCH) {
        uint64_t const n_global = binom(L, h);
        if (n_global > 0 && n_global < ((uint64_t)1 << 40)) {
            int64_t const entries = (int64_t)((n_global + 63) / 64);
            void *p = NULL;
            if (lsk_malloc(&p, sizeof(lsk_rankdir) * (size_t)entries) == 0) {
                int zero = 0, flag = 1;
                if (lsk_h2d(pl->d_err, &zero, sizeof(int)) == 0 &&
                    lsk_rankdir_build(ps->count, ps->d_reps, L, h, d_binom, entries, (lsk_rankdir *)p, pl->d_err, stream) == 0 &&
                    lsk_d2h(&flag, pl->d_err, sizeof(int)) == 0 && flag == 0) {
                    ps->d_dir = (lsk_rankdir *)p;
                    ps->index.dir = ps->d_dir;
                    ps->index.dir_sites = L;
                    ps->index.dir_weight = h;
                } else lsk_free(p);
                (void)lsk_h2d(pl->d_err, &zero, sizeof(int));
            }
        }
    }
    if (pl->family == FAMILY_TILE_PULL) {
        void *p;
        DEV(lsk_malloc(&p, 8 * (size_t)(ps->count > 0 ? ps->count : 1)));
        ps->d_norms = (double *)p;
        DEV(lsk_norms(pl->dbs, ps->count, ps->d_reps, ps->d_norms, stream));
        ps->rounds = 1;
        return 0;
    }
    if (pl->family != FAMILY_TILE) return 0;

    if (pl->dbs.proj == LSK_PROJ_FULL) {
        void *p;
        DEV(lsk_malloc(&p, 8 * (size_t)(ps->count > 0 ? ps->count : 1)));
        ps->d_norms = (double *)p;
        DEV(lsk_norms(pl->dbs, ps->count, ps->d_reps, ps->d_norms, stream));
    }
    int rounds = num_rounds;
    if (rounds <= 0) {
        int64_t rpr = rows_per_round_default();
        rounds = (int)((ps->count + rpr - 1) / rpr);
        if (rounds < 1) rounds = 1;
    }
    ps->rounds = rounds;
    int const P = pl->P;
    ps->send_counts = (int64_t *)calloc((size_t)rounds * P, sizeof(int64_t));
    ps->h_beta_off = (int64_t *)calloc((size_t)rounds * P, sizeof(int64_t));
    ps->h_val_off = (int64_t *)calloc((size_t)rounds * P, sizeof(int64_t));
    lsk_round_layout *layouts = (lsk_round_layout *)calloc(rounds, sizeof(lsk_round_layout));
    int const w = pl->cplx ? 16 : 8;
    unsigned long long hc[LSK_MAX_PARTS];
    /* the per-wave producer (deterministic send layout) whenever lane d of a wave can stand for destination d */
    int const wave_rings = !pl->streams && P <= lsk_tile_wv_max_parts() && packets_wave_rings();
    uint32_t *h_wtab = NULL;
    int64_t n_waves = 0;
    /* sorted streams: count pass per (tile, destination, stream); the host turns the counts into positions inside the destination's
     * segment, streams one after the other, tiles in row order inside a stream */
    uint32_t *h_ttab = NULL, *h_soff = NULL, *sbase = NULL;
    uint64_t *running = NULL;
    int const S = pl->st_S, C = P * S, TR = pl->st_tile_rows;
    int64_t n_tiles = 0;
    if (pl->streams) {
        uint64_t const *d_binom;
        if (device_binom(&d_binom) != 0) { free(layouts); return -1; }
        ps->ttab_first = (int64_t *)calloc((size_t)rounds + 1, sizeof(int64_t));
        for (int r = 0; r < rounds; ++r) {
            int64_t row0 = ps->count * r / rounds, row1 = ps->count * (r + 1) / rounds;
            ps->ttab_first[r] = n_tiles;
            n_tiles += (row1 - row0 + TR - 1) / TR;
        }
        ps->ttab_first[rounds] = n_tiles;
        void *pt;
        size_t const bytes = sizeof(uint32_t) * (size_t)(n_tiles > 0 ? n_tiles : 1) * (size_t)C;
        if (lsk_malloc(&pt, bytes) != 0) { free(layouts); return dev_error(); }
        ps->d_ttab = (uint32_t *)pt;
        if (lsk_memset_async(pt, 0, bytes, stream) != 0) { free(layouts); return dev_error(); }
        for (int r = 0; r < rounds; ++r) {
            int64_t row0 = ps->count * r / rounds, row1 = ps->count * (r + 1) / rounds;
            if (lsk_tile_st(pl->dop, pl->gd, d_binom, pl->cplx, 1, P, S, TR, row0, row1, ps->d_reps, NULL,
                            ps->d_ttab + (size_t)ps->ttab_first[r] * C, NULL, NULL, pl->d_err, stream) != 0) { free(layouts); return dev_error(); }
        }
        h_ttab = (uint32_t *)malloc(bytes);
        h_soff = (uint32_t *)calloc((size_t)rounds * P * (S + 1), sizeof(uint32_t));
        sbase = (uint32_t *)calloc((size_t)C, sizeof(uint32_t));
        running = (uint64_t *)calloc((size_t)C, sizeof(uint64_t));
        if (!h_ttab || !h_soff || !sbase || !running || lsk_sync(stream) != 0 || lsk_d2h(h_ttab, pt, bytes) != 0) {
            free(h_ttab); free(h_soff); free(sbase); free(running); free(layouts);
            return dev_error();
        }
    }
    if (wave_rings) {
        ps->wtab_first = (int64_t *)calloc((size_t)rounds + 1, sizeof(int64_t));
        for (int r = 0; r < rounds; ++r) {
            int64_t row0 = ps->count * r / rounds, row1 = ps->count * (r + 1) / rounds;
            ps->wtab_first[r] = n_waves;
            n_waves += (row1 - row0 + 63) / 64;
        }
        ps->wtab_first[rounds] = n_waves;
        void *pw;
        size_t const bytes = sizeof(uint32_t) * (size_t)(n_waves > 0 ? n_waves : 1) * (size_t)P;
        if (lsk_malloc(&pw, bytes) != 0) { free(layouts); return dev_error(); }
        ps->d_wtab = (uint32_t *)pw;
        if (lsk_memset_async(pw, 0, bytes, stream) != 0) { free(layouts); return dev_error(); }
        for (int r = 0; r < rounds; ++r) {
            int64_t row0 = ps->count * r / rounds, row1 = ps->count * (r + 1) / rounds;
            if (lsk_tile_wv(pl->dop, pl->dbs, ps->index, pl->gd, pl->cplx, 1, P, part_id, row0, row1, ps->d_reps, ps->d_norms, NULL, NULL,
                            ps->d_wtab + (size_t)ps->wtab_first[r] * P, NULL, NULL, pl->d_err, no_gtab(), stream) != 0) { free(layouts); return dev_error(); }
        }
        h_wtab = (uint32_t *)malloc(bytes);
        if (!h_wtab || lsk_sync(stream) != 0 || lsk_d2h(h_wtab, pw, bytes) != 0) { free(h_wtab); free(layouts); return dev_error(); }
    }
    for (int r = 0; r < rounds; ++r) {
        int64_t row0 = ps->count * r / rounds, row1 = ps->count * (r + 1) / rounds;
        if (pl->streams) {
            memset(running, 0, sizeof(uint64_t) * (size_t)C);
            for (int64_t t = ps->ttab_first[r]; t < ps->ttab_first[r + 1]; ++t) { /* exclusive prefix over the tiles, class by class */
                uint32_t *row = h_ttab + (size_t)t * C;
                for (int c = 0; c < C; ++c) { uint32_t const k = row[c]; row[c] = (uint32_t)running[c]; running[c] += k; }
            }
            int too_many = 0;
            for (int d = 0; d < P; ++d) { /* the streams of a segment one after the other */
                uint64_t base = 0;
                uint32_t *so = h_soff + ((size_t)r * P + d) * (S + 1);
                for (int q = 0; q < S; ++q) {
                    so[q] = (uint32_t)base;
                    sbase[d * S + q] = (uint32_t)base;
                    base += running[d * S + q];
                    if (base > 0xffffffffULL) too_many = 1;
                }
                so[S] = (uint32_t)base;
                hc[d] = base;
            }
            if (too_many) {
                free(h_ttab); free(h_soff); free(sbase); free(running); free(layouts);
                return set_error("more than 2^32 packets for one destination in one round: raise the number of rounds");
            }
            for (int64_t t = ps->ttab_first[r]; t < ps->ttab_first[r + 1]; ++t) {
                uint32_t *row = h_ttab + (size_t)t * C;
                for (int c = 0; c < C; ++c) row[c] += sbase[c];
            }
        } else if (wave_rings) {
            /* counts -> exclusive offsets along the waves of the round, destination by destination; the own partition's
             * packets never enter the send buffer */
            for (int d = 0; d < P; ++d) hc[d] = 0;
            for (int64_t wv = ps->wtab_first[r]; wv < ps->wtab_first[r + 1]; ++wv) {
                uint32_t *row = h_wtab + (size_t)wv * P;
                for (int d = 0; d < P; ++d) {
                    uint32_t const c = row[d];
                    if (d != part_id && hc[d] + c > 0xffffffffULL) { free(h_wtab); free(layouts); return set_error("more than 2^32 packets for one destination in one round: raise the number of rounds"); }
                    row[d] = (uint32_t)hc[d];
                    hc[d] += c;
                }
            }
        } else {
            if (lsk_memset_async(pl->d_counts, 0, 8 * LSK_MAX_PARTS, stream) != 0 ||
                lsk_tile(pl->dop, pl->dbs, ps->index, pl->cplx, 1, P, part_id, row0, row1, ps->d_reps, ps->d_norms,
                         NULL, NULL, pl->d_cursors, NULL, NULL, pl->d_counts, pl->d_err, stream) != 0 ||
                lsk_sync(stream) != 0 || lsk_d2h(hc, pl->d_counts, 8 * (size_t)P) != 0) { free(layouts); return dev_error(); }
        }
        int64_t off = 0;
        for (int d = 0; d < P; ++d) {
            pl->nnz += (int64_t)hc[d];
            int64_t c = (d == part_id && !pl->streams) ? 0 : (int64_t)hc[d]; /* (sorted streams: the own partition's packets take the buffer too) */
            ps->send_counts[(size_t)r * P + d] = c;
            int64_t const keys = segment_key_bytes(pl, c); /* u64 states, or u32 indices padded to 8 bytes */
            layouts[r].beta_off[d] = off;
            layouts[r].val_off[d] = off + keys;
            ps->h_beta_off[(size_t)r * P + d] = off;
            ps->h_val_off[(size_t)r * P + d] = off + keys;
            off += keys + w * c;
        }
        if (off > ps->max_send_bytes) ps->max_send_bytes = off;
    }
    if (wave_rings) {
        int const rcw = lsk_h2d(ps->d_wtab, h_wtab, sizeof(uint32_t) * (size_t)(n_waves > 0 ? n_waves : 1) * (size_t)P);
        free(h_wtab);
        if (rcw != 0) { free(layouts); return dev_error(); }
    }
    if (pl->streams) {
        void *po = NULL;
        size_t const sob = sizeof(uint32_t) * (size_t)rounds * (size_t)P * (size_t)(S + 1);
        int const rcs = lsk_h2d(ps->d_ttab, h_ttab, sizeof(uint32_t) * (size_t)(n_tiles > 0 ? n_tiles : 1) * (size_t)C) != 0 ||
                        lsk_malloc(&po, sob) != 0 || lsk_h2d(po, h_soff, sob) != 0;
        ps->d_soff = (uint32_t *)po; /* owned by the plan from here on */
        ps->h_soff = h_soff;
        free(h_ttab); free(sbase); free(running);
        if (rcs != 0) { free(layouts); return dev_error(); }
    }
    void *p;
    if (lsk_malloc(&p, sizeof(lsk_round_layout) * (size_t)rounds) != 0) { free(layouts); return dev_error(); }
    ps->d_layouts = (lsk_round_layout *)p; /* owned by the plan from here on */
    int const rc = lsk_h2d(p, layouts, sizeof(lsk_round_layout) * (size_t)rounds);
    free(layouts);
    return rc != 0 ? dev_error() : 0;
}

/* windows of y per consumer block: the end of one window's run is the start of the next one's (one binary search saved per
 * stream), as long as >= 8192 blocks keep the 2048 block slots busy without a long tail.  (Measured on chain_28 x 8: 1 / 4 / 8
 * windows per block 2.96 / 2.86 / 3.06 ms -- no knob; the test hook forces the carry path on small bases.) */
static __thread int g_test_stream_wpb = 0;
void ls_amd_test_set_stream_windows_per_block(int n) { g_test_stream_wpb = n; }
static int stream_windows_per_block(int64_t windows) {
    if (g_test_stream_wpb > 0) return g_test_stream_wpb;
    int64_t const w = windows / 8192;
    return w < 1 ? 1 : (w > 8 ? 8 : (int)w);
}
/* sorted streams, all partitions in this process: one send buffer per source partition (a round of all sources is consumed by
 * ONE launch, so y is read and written once per round) and the consumer's view of every (round, destination, source) segment */
static __thread int g_test_fail_stream_buffers = 0;
void ls_amd_test_fail_stream_buffers(int on) { g_test_fail_stream_buffers = on; }
static int setup_streams(ls_amd_plan *pl, int rounds) {
    int const P = pl->P, S = pl->st_S;
    if (g_test_fail_stream_buffers) return set_error("test hook: no room for the stream buffers");
    pl->st_rounds = rounds;
    pl->d_send_parts = (void **)calloc((size_t)P, sizeof(void *));
    for (int p = 0; p < P; ++p) {
        if (pl->parts[p].rounds != rounds) return set_error("internal error: partitions disagree on the number of rounds");
        if (lsk_malloc(&pl->d_send_parts[p], (size_t)(pl->parts[p].max_send_bytes > 0 ? pl->parts[p].max_send_bytes : 8)) != 0) return dev_error();
    }
    size_t const n = (size_t)rounds * (size_t)P * (size_t)P;
    lsk_wsrc *h = (lsk_wsrc *)calloc(n, sizeof(lsk_wsrc));
    for (int r = 0; r < rounds; ++r)
        for (int d = 0; d < P; ++d)
            for (int q = 0; q < P; ++q) {
                part_state const *src = &pl->parts[q];
                lsk_wsrc *w = h + ((size_t)r * P + d) * P + q;
                w->keys = (uint32_t const *)((char const *)pl->d_send_parts[q] + src->h_beta_off[(size_t)r * P + d]);
                w->vals = (double const *)((char const *)pl->d_send_parts[q] + src->h_val_off[(size_t)r * P + d]);
                w->soff = src->d_soff + ((size_t)r * P + d) * (size_t)(S + 1);
            }
    void *pw = NULL;
    int const bad = lsk_malloc(&pw, sizeof(lsk_wsrc) * n) != 0 || lsk_h2d(pw, h, sizeof(lsk_wsrc) * n) != 0;
    free(h);
    pl->d_wsrcs = (lsk_wsrc *)pw;
    if (bad) return dev_error();
    /* windows per block: the end of one window's run is the start of the next one's (one binary search saved per stream) as long
     * as the launch still has several blocks per CU */
    int64_t windows = 0;
    int const W = lsk_window_rows(pl->cplx);
    for (int d = 0; d < P; ++d) windows += (pl->parts[d].count + W - 1) / W;
    pl->st_wpb = stream_windows_per_block(windows);
    return 0;
}

int ls_amd_plan_create(ls_amd_plan **out, ls_hs_operator const *op, ls_amd_dtype dtype,
                       int num_partitions, int my_partition, uint64_t const *const *d_reps,
                       int64_t const *counts, int num_rounds, ls_amd_mode mode, void *stream) {
    *out = NULL;
    if (!op || !op->basis) return set_error("null operator");
    if (ls_hs_basis_number_words(op->basis) != 1) return set_error("bases with more than 64 bits are not yet implemented"); /* DMV:1099 */
    if (num_partitions < 1 || num_partitions > LSK_MAX_PARTS) return set_error("num_partitions must be in [1, %d]", LSK_MAX_PARTS);
    if (my_partition >= num_partitions) return set_error("my_partition out of range");
    if (dtype == LS_AMD_F64 && !OEXT(op)->is_real) return set_error("an operator with complex coefficients needs dtype c128");
    ls_amd_plan *pl = (ls_amd_plan *)calloc(1, sizeof(*pl));
    pl->op = op;
    pl->cplx = dtype == LS_AMD_C128;
    pl->P = num_partitions;
    pl->me = my_partition;
    pl->n_local = my_partition < 0 ? num_partitions : 1;
    if (operator_device(op, &pl->dop) != 0 || basis_device(op->basis, &pl->dbs) != 0) { free(pl); return -1; }
    if (pl->dbs.fermi) {
        /* projected fermions: the signed K4 exists in the indexed pull kernel of one partition (fused, or resolve + gather) and
         * nowhere else -- every other path would run without the signs, so it is refused here, before anything launches */
        char const *why = NULL, *ev = getenv("LS_AMD_PULL_VALUES"), *ei = getenv("LS_AMD_PULL_INDEXED"), *em = getenv("LS_AMD_MODE");
        if (my_partition >= 0) why = "one partition per process";
        else if (num_partitions != 1) why = "more than one partition";
        else if (mode == LS_AMD_MODE_PUSH || (mode == LS_AMD_MODE_AUTO && em && strcmp(em, "push") == 0)) why = "push mode";
        else if (!OEXT(op)->is_hermitian) why = "a non-Hermitian operator";
        else if (ev && atoi(ev) != 0) why = "LS_AMD_PULL_VALUES=1";
        else if (ei && atoi(ei) == 0) why = "LS_AMD_PULL_INDEXED=0";
        if (why) { free(pl); return set_error("projected fermionic bases run the indexed pull kernel of one partition only: %s is not supported", why); }
    }
    if (dtype == LS_AMD_F64) {
        /* f64 vectors: characters must be real as well (the reference casts c128 -> f64, DMV:91,109) */
        for (int g = 0; g < BEXT(op->basis)->order; ++g)
            if (BEXT(op->basis)->elems[g].ch_im != 0.0) { free(pl); return set_error("complex characters need dtype c128"); }
    }
    /* kernel family */
    /* a plan that owns ONE partition is driven by generate / exchange / scatter (one locale per process): always the
     * packet kernels, also when numLocales == 1 (the reference's matrixVectorProduct works there too, DMV:1072-1093) */
    int const force_tile = my_partition >= 0;
    if (force_tile) pl->family = FAMILY_TILE;
    else if (num_partitions == 1 && pl->dbs.proj != LSK_PROJ_FULL) {
        ls_amd_mode m = mode;
        if (m == LS_AMD_MODE_AUTO) {
            char const *e = getenv("LS_AMD_MODE");
            if (e && strcmp(e, "pull") == 0) m = LS_AMD_MODE_PULL;
            else if (e && strcmp(e, "push") == 0) m = LS_AMD_MODE_PUSH;
            /* measured: pull is 2.6x push on chain_32.  Round 6: on an unprojected basis ANY operator can be pulled -- row i takes
             * <i|H_g|i ^ x_g> from the partner's row expansion (k_direct, k_rows.hip) -- so non-Hermitian operators leave the
             * atomics too; only the inversion sectors still pull through the Hermiticity of the projected matrix */
            else m = (OEXT(op)->is_hermitian || pl->dbs.proj == LSK_PROJ_NONE) ? LS_AMD_MODE_PULL : LS_AMD_MODE_PUSH;
        }
        if (m == LS_AMD_MODE_PULL && !OEXT(op)->is_hermitian && pl->dbs.proj != LSK_PROJ_NONE) {
            if (mode == LS_AMD_MODE_PULL) { free(pl); return set_error("pull mode needs a Hermitian operator (or an unprojected basis)"); }
            m = LS_AMD_MODE_PUSH;
        }
        pl->family = m == LS_AMD_MODE_PULL ? FAMILY_DIRECT_PULL : FAMILY_DIRECT_PUSH;
    } else if (num_partitions == 1 && pl->dbs.proj == LSK_PROJ_FULL) {
        /* projected basis on one device: staged pull (no global atomics) when H is Hermitian */
        ls_amd_mode m = mode;
        if (m == LS_AMD_MODE_AUTO) {
            char const *e = getenv("LS_AMD_MODE");
            if (e && strcmp(e, "push") == 0) m = LS_AMD_MODE_PUSH;
            else m = LS_AMD_MODE_PULL;
        }
        if (m == LS_AMD_MODE_PULL && !OEXT(op)->is_hermitian) {
            if (mode == LS_AMD_MODE_PULL) { free(pl); return set_error("pull mode needs a Hermitian operator"); }
            m = LS_AMD_MODE_PUSH;
        }
        pl->family = m == LS_AMD_MODE_PULL ? FAMILY_TILE_PULL : FAMILY_TILE;
        if (pl->family == FAMILY_TILE_PULL) {
            /* Default: the INDEXED mode -- static {rep -> index} table + x[index] (two dependent requests per far partner,
             * nothing rewritten per matvec).  Measured r3 (profiles/r3_indexed_ab_*): chain_36_symm 24.8 -> 20.4 ms,
             * chain_40_symm 373.5 -> 323.0 ms per matvec against the {rep -> x n(rep)} value table (one request per far
             * partner, but N random 16-byte writes per matvec: 2.8 / 42.5 ms), which stays as LS_AMD_PULL_INDEXED=0 and
             * as the fallback for bases whose keys do not fit the 8-byte entries (lsk_gtab_bits). */
            char const *e = getenv("LS_AMD_PULL_INDEXED");
            pl->idx_mode = e ? atoi(e) != 0 : 1;
            if (pl->idx_mode && (counts[0] >= 0xffffffffLL || lsk_gtab_bits(NBITS(op->basis), counts[0], (int64_t)1 << 40) < 0)) pl->idx_mode = 0;
        }
    } else pl->family = FAMILY_TILE;

    void *p;
    if (lsk_malloc(&p, 8 * LSK_MAX_PARTS) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
    pl->d_cursors = (unsigned long long *)p;
    if (lsk_malloc(&p, 8 * LSK_MAX_PARTS) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
    pl->d_counts = (unsigned long long *)p;
    if (lsk_malloc(&p, 2 * sizeof(int)) != 0) { ls_amd_plan_destroy(pl); return dev_error(); } /* [0]: the error flag; [1]: a word nobody reads (lsk_direct) */
    pl->d_err = (int *)p;
    int zero = 0;
    int const zero2[2] = {0, 0};
    if (lsk_h2d(pl->d_err, zero2, sizeof(zero2)) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }

    pl->key_bytes = 8;
    if (pl->family == FAMILY_TILE && setup_packet_index(pl, d_reps, counts, stream) != 0) { ls_amd_plan_destroy(pl); return -1; }
    pl->parts = (part_state *)calloc(pl->n_local, sizeof(part_state));
    int const num_rounds_arg = num_rounds;
    if (pl->streams && num_rounds <= 0) { /* one consumer launch per round over all sources: every partition runs the same rounds */
        int64_t mx = 0, rpr = rows_per_round_default();
        for (int i = 0; i < pl->n_local; ++i) if (counts[i] > mx) mx = counts[i];
        num_rounds = (int)((mx + rpr - 1) / rpr);
        if (num_rounds < 1) num_rounds = 1;
    }
    for (int i = 0; i < pl->n_local; ++i) {
        part_state *ps = &pl->parts[i];
        ps->count = counts[i];
        ps->d_reps = d_reps[i];
        int pid = my_partition < 0 ? i : my_partition;
        if (plan_setup_part(pl, ps, pid, num_rounds, stream) != 0) { ls_amd_plan_destroy(pl); return -1; }
        if (ps->max_send_bytes > pl->send_capacity) pl->send_capacity = ps->max_send_bytes;
    }
    int gkeys_ok = 1;
    if (pl->stream_gkeys) for (int i = 0; i < pl->n_local; ++i) if (pl->parts[i].count > 0 && !pl->parts[i].index.dir) gkeys_ok = 0;
    if (pl->streams && !gkeys_ok) {
        /* a partition without its rank directory (not the hash partition of the full fixed-weight basis, or no room): the same plan with
         * the atomic consumers */
        ls_amd_plan_destroy(pl);
        if (g_no_streams) return -1;
        g_no_streams = 1;
        int const rc = ls_amd_plan_create(out, op, dtype, num_partitions, my_partition, d_reps, counts, num_rounds_arg, mode, stream);
        g_no_streams = 0;
        return rc;
    }
    if (pl->streams && my_partition < 0 && setup_streams(pl, num_rounds) != 0) {
        /* one buffer per source partition did not fit (or a table could not be uploaded): the same plan with ONE shared buffer and
         * the atomic consumers -- the O(N / P) form must not fail where it used to work */
        ls_amd_plan_destroy(pl);
        if (g_no_streams) return -1;
        g_no_streams = 1;
        int const rc = ls_amd_plan_create(out, op, dtype, num_partitions, my_partition, d_reps, counts, num_rounds_arg, mode, stream);
        g_no_streams = 0;
        return rc;
    }
    if (pl->streams && my_partition >= 0) { /* one partition per process: the driver owns the buffers (dist.c) */
        pl->st_rounds = pl->parts[0].rounds;
        pl->st_wpb = stream_windows_per_block((pl->parts[0].count + lsk_window_rows(pl->cplx) - 1) / lsk_window_rows(pl->cplx));
    }
    if (pl->family == FAMILY_DIRECT_PULL || pl->family == FAMILY_DIRECT_PUSH) {
        int const combinadic = pl->parts[0].index.kind == LSK_INDEX_COMBINADIC;
        part_state *ps0 = &pl->parts[0];
        if (pl->family == FAMILY_DIRECT_PULL && combinadic && chain_eligible(pl) &&
            setup_chain(pl, ps0->index, ps0->count, ps0->d_reps, stream) != 0) { ls_amd_plan_destroy(pl); return -1; }
        if (!pl->has_chain && pl->family == FAMILY_DIRECT_PULL && combinadic && setup_pairs(pl, ps0->count, ps0->d_reps, stream) != 0) {
            ls_amd_plan_destroy(pl);
            return -1;
        }
        if (!pl->has_chain && !pl->has_pairs && setup_hubbard(pl, ps0, stream) != 0) { ls_amd_plan_destroy(pl); return -1; }
        if (pl->family == FAMILY_DIRECT_PUSH && combinadic && push_staged_eligible(pl)) {
            if (build_tilemap(pl, ps0->count, lsk_push_tile_rows(pl->cplx)) != 0) { ls_amd_plan_destroy(pl); return -1; }
            pl->has_push_staged = 1;
        }
        if (!pl->has_chain && !pl->has_pairs && !pl->has_push_staged && !pl->has_hubbard && build_tilemap(pl, ps0->count, 256) != 0) { ls_amd_plan_destroy(pl); return -1; }
        if (pl->family == FAMILY_DIRECT_PULL && !OEXT(op)->is_hermitian) {
            /* a gather never sees a state that is mapped OUT of the basis (the reference's halt, DMV:115-118): checked once, here;
             * ls_amd_plan_check reports it after every matvec like the push kernels' error flag */
            int flag = 0;
            if (lsk_direct_validate(pl->dop, pl->dbs, ps0->index, ps0->count, ps0->d_reps, pl->d_err, stream) != 0 || lsk_sync(stream) != 0 ||
                lsk_d2h(&flag, pl->d_err, sizeof(int)) != 0 || lsk_h2d(pl->d_err, &zero, sizeof(int)) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
            pl->leaves_basis = flag != 0;
        }
    }
    if (pl->family == FAMILY_TILE && my_partition < 0 && pl->send_capacity > 0 && !pl->streams) {
        if (lsk_malloc(&pl->d_send, (size_t)pl->send_capacity) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
    }
    if (pl->family == FAMILY_TILE && pl->P == 1 && my_partition >= 0 && pl->one_rank_full_basis && pl->parts[0].rounds == 1 &&
        push_staged_eligible(pl)) {
        /* one rank, every packet its own: the producer of the only round is the staged push kernel (round 6: chain_32 through the
         * C host's packet driver 87.6 -> see profiles/r6_staged_push_ab.txt) */
        if (build_tilemap(pl, pl->parts[0].count, lsk_push_tile_rows(pl->cplx)) != 0) { ls_amd_plan_destroy(pl); return -1; }
        pl->has_push_staged = 1;
    }
    if (pl->family == FAMILY_TILE && pl->key_bytes == 8 && pl->P > 1) {
        /* State-carrying packets into a SEARCHED index (projected bases): the consumer's look-up is one 16-byte probe of a static
         * {representative -> index} table per partition instead of the prefix table + binary search (4-6 dependent loads per packet;
         * round 6: chain_36_symm x 8 consumers 40.0 -> see profiles/r6_projected_packets_hash_index_ab.txt).  16-32 bytes per state,
         * O(N / P); a table that cannot be built leaves the search in place.  LS_AMD_SCATTER_HASH=0: off (A/B). */
        char const *he = getenv("LS_AMD_SCATTER_HASH");
        if (!(he && atoi(he) == 0))
            for (int p = 0; p < pl->n_local; ++p) {
                part_state *ps = &pl->parts[p];
                if (ps->index.kind != LSK_INDEX_SEARCH || ps->index.dir || ps->count <= 0 || ps->count >= 0xffffffffLL) continue;
                if (ls_amd_internal_gtab_acquire(&ps->scatter_gt, NBITS(op->basis), ps->d_reps, ps->count, NULL, 1, stream) != 0) {
                    ps->scatter_gt = NULL; /* (the error text stays readable through ls_amd_last_error; the plan works without the table) */
                }
            }
    }
    if (pl->family == FAMILY_TILE && my_partition < 0 && pl->P > 1 && pl->key_bytes == 8) {
        /* the destinations' indexes as a device array: all segments a producer's round leaves are consumed by ONE launch */
        lsk_part_ctx *h = (lsk_part_ctx *)calloc((size_t)pl->P, sizeof(lsk_part_ctx));
        for (int d = 0; d < pl->P; ++d) {
            h[d].ix = pl->parts[d].index;
            h[d].norms = pl->dbs.k4_mode ? pl->parts[d].d_norms : NULL;
            if (pl->parts[d].scatter_gt) h[d].gt = pl->parts[d].scatter_gt->tab;
            if (!pl->parts[pl->part_ctx_any].index.dir && pl->parts[d].index.dir) pl->part_ctx_any = d;
        }
        void *pc = NULL;
        int const bad = lsk_malloc(&pc, sizeof(lsk_part_ctx) * (size_t)pl->P) != 0 || lsk_h2d(pc, h, sizeof(lsk_part_ctx) * (size_t)pl->P) != 0;
        free(h);
        if (bad) { if (pc) lsk_free(pc); ls_amd_plan_destroy(pl); return dev_error(); }
        pl->d_part_ctx = (lsk_part_ctx *)pc;
    }
    if (pl->family == FAMILY_TILE_PULL && pl->idx_mode) {
        /* static index table + room for x * norm(rep), acquired here: a table that cannot be built (no memory, a key that
         * finds no place within 255 buckets) puts the plan on the value-table path instead of failing the first matvec */
        part_state *ps = &pl->parts[0];
        int ok = ls_amd_internal_gtab_acquire(&pl->gtab, NBITS(op->basis), ps->d_reps, ps->count, NULL, 1, stream) == 0;
        if (ok && pl->dbs.k4_mode != 0 &&
            lsk_malloc(&pl->d_xs, (size_t)(pl->cplx ? 16 : 8) * (size_t)(ps->count > 0 ? ps->count : 1)) != 0) {
            ls_amd_internal_gtab_release(pl->gtab);
            pl->gtab = NULL;
            pl->d_xs = NULL;
            ok = 0;
        }
        if (!ok) pl->idx_mode = 0;
        else {
            pl->pull_halo = pull_halo_setting(1);
            char const *e = getenv("LS_AMD_PULL_SPLIT"); /* bytes of packet buffer; measurement of the two-kernel form */
            if (e && atoll(e) > 0) ls_amd_internal_plan_split_enable(pl, atoll(e));
            /* LS_AMD_SLOT_CACHE = bytes: ls_amd_plan_cache_slots for callers that cannot reach the plan -- the host-pointer entry
             * points under Diagonalize / PRIMME (ls_chpl_matrix_vector_product, ls_chpl_primme_matvec) keep one plan per
             * operator, which then resolves its packet streams on the first matvec only */
            e = getenv("LS_AMD_SLOT_CACHE");
            if (e && atoll(e) > 0 && ls_amd_plan_cache_slots(pl, atoll(e)) < 0) { ls_amd_plan_destroy(pl); return -1; }
            /* Value table (round 6; k_pull.hip, lsk_vtab_*): f64 vectors of one partition, matrix-free plans --
             * the far partners' values travel with their table bucket (one fabric request instead of two dependent ones) and
             * are refreshed once per matvec in table order.  32 bytes per bucket next to the shared index table's 16; taken while
             * it fits a third of the free HBM.  LS_AMD_PULL_VALUES=0 keeps the index table + x[slot] gather (always the path of
             * c128 vectors, of the replicated-x exchange -- no rank may do O(N) work per matvec there -- and of the slot cache). */
            e = getenv("LS_AMD_PULL_VALUES");
            int const want_values = e ? atoi(e) != 0 : LS_AMD_PULL_VALUES_DEFAULT;
            if (want_values && !pl->cplx && !pl->slot_cache && pl->split_rows == 0 && !pl->dbs.fermi) { /* (no signs in the value-table kernel) */
                size_t fr = 0, tot = 0;
                size_t const need = (size_t)32 << pl->gtab->tab.bbits;
                void *vt = NULL;
                if (lsk_mem_info(&fr, &tot) == 0 && need <= fr / 3 && lsk_malloc(&vt, need) == 0) {
                    if (lsk_vtab_build(pl->gtab->tab, (uint64_t *)vt, stream) != 0) { lsk_free(vt); ls_amd_plan_destroy(pl); return dev_error(); }
                    pl->d_vtab = (uint64_t *)vt;
                }
            }
        }
    }
    if (pl->dbs.fermi && (!pl->idx_mode || pl->d_vtab)) {
        ls_amd_plan_destroy(pl);
        return set_error("projected fermionic bases run the indexed pull kernel of one partition only: no static index table for this basis");
    }
    if (lsk_sync(stream) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
    *out = pl;
    ls_amd_internal_clear_error(); /* (internal fallbacks -- a table that did not fit, a layout that does not apply -- leave no message) */
    return 0;
}

void ls_amd_plan_destroy(ls_amd_plan *pl) {
    if (!pl) return;
    if (pl->d_vtab) lsk_free(pl->d_vtab);
    if (pl->d_gdir) lsk_free(pl->d_gdir);
    if (pl->d_part_ctx) lsk_free(pl->d_part_ctx);
    if (pl->d_send_parts) {
        for (int p = 0; p < pl->P; ++p) if (pl->d_send_parts[p]) lsk_free(pl->d_send_parts[p]);
        free(pl->d_send_parts);
    }
    if (pl->d_wsrcs) lsk_free(pl->d_wsrcs);
    if (pl->parts) {
        for (int i = 0; i < pl->n_local; ++i) {
            part_state *ps = &pl->parts[i];
            if (ps->d_table) lsk_free(ps->d_table);
            if (ps->d_dir) lsk_free(ps->d_dir);
            if (ps->d_norms) lsk_free(ps->d_norms);
            if (ps->d_layouts) lsk_free(ps->d_layouts);
            if (ps->d_wtab) lsk_free(ps->d_wtab);
            free(ps->wtab_first);
            if (ps->d_ttab) lsk_free(ps->d_ttab);
            if (ps->d_soff) lsk_free(ps->d_soff);
            if (ps->scatter_gt) ls_amd_internal_gtab_release(ps->scatter_gt);
            free(ps->h_soff);
            free(ps->ttab_first);
            free(ps->send_counts); free(ps->h_beta_off); free(ps->h_val_off);
        }
        free(pl->parts);
    }
    if (pl->d_gtable) lsk_free(pl->d_gtable);
    if (pl->d_row_gidx) lsk_free(pl->d_row_gidx);
    if (pl->d_norms_global) lsk_free(pl->d_norms_global);
    if (pl->d_tilemap) lsk_free(pl->d_tilemap);
    if (pl->d_chain_cache) lsk_free(pl->d_chain_cache);
    if (pl->d_chain_rec) lsk_free(pl->d_chain_rec);
    if (pl->d_chain_wave) lsk_free(pl->d_chain_wave);
    if (pl->d_tilemap_pair) lsk_free(pl->d_tilemap_pair);
    if (pl->d_chain_hdr_b) lsk_free(pl->d_chain_hdr_b);
    if (pl->d_pair_recs) lsk_free(pl->d_pair_recs);
    for (int k = 0; k < 6; ++k) if (pl->d_hub[k]) lsk_free(pl->d_hub[k]);
    if (pl->d_pair_rows) lsk_free(pl->d_pair_rows);
    if (pl->d_pair_sites) lsk_free(pl->d_pair_sites);
    if (pl->d_rank_low) lsk_free(pl->d_rank_low);
    if (pl->d_pair_binom) lsk_free(pl->d_pair_binom);
    if (pl->d_states32) lsk_free(pl->d_states32);
    if (pl->d_htab) lsk_free(pl->d_htab);
    if (pl->d_slot_of) lsk_free(pl->d_slot_of);
    if (pl->d_xs) lsk_free(pl->d_xs);
    if (pl->gtab) ls_amd_internal_gtab_release(pl->gtab);
    split_free(pl);
    block_free(pl);
    if (pl->d_send) lsk_free(pl->d_send);
    if (pl->d_cursors) lsk_free(pl->d_cursors);
    if (pl->d_counts) lsk_free(pl->d_counts);
    if (pl->d_err) lsk_free(pl->d_err);
    ls_amd_plan_enable_timing(pl, 0);
    ls_amd_plan_enable_stage_timing(pl, 0);
    free(pl);
}

int ls_amd_plan_num_rounds(ls_amd_plan const *pl) { return pl->family == FAMILY_TILE ? pl->parts[0].rounds : 1; }

/* -------------------------------------------------------------------------------------------- */
/* replicated-x plans                                                                            */
/* -------------------------------------------------------------------------------------------- */
static int plan_create_replicated_impl(ls_amd_plan **out, ls_hs_operator const *op, ls_amd_dtype dtype,
                                       int num_partitions, int my_partition, uint64_t const *d_reps_local,
                                       int64_t count_local, uint64_t const *d_reps_global, int64_t count_global,
                                       ls_amd_gtab *gt, void *stream);
int ls_amd_plan_create_replicated(ls_amd_plan **out, ls_hs_operator const *op, ls_amd_dtype dtype,
                                  int num_partitions, int my_partition, uint64_t const *d_reps_local,
                                  int64_t count_local, uint64_t const *d_reps_global, int64_t count_global,
                                  void *stream) {
    return plan_create_replicated_impl(out, op, dtype, num_partitions, my_partition, d_reps_local, count_local, d_reps_global,
                                       count_global, NULL, stream);
}
/* the replicated-x plan of the indexed exchange (dist.c): x arrives as the owners' blocks (slot order of `gt`), the rows are
 * the contiguous global rows d_reps_local = d_reps_global + row0.  Projected bases only. */
int ls_amd_internal_plan_create_replicated_indexed(ls_amd_plan **out, ls_hs_operator const *op, ls_amd_dtype dtype,
                                                   int num_partitions, int my_partition, uint64_t const *d_reps_local,
                                                   int64_t count_local, uint64_t const *d_reps_global, int64_t count_global,
                                                   ls_amd_gtab *gt, void *stream) {
    return plan_create_replicated_impl(out, op, dtype, num_partitions, my_partition, d_reps_local, count_local, d_reps_global,
                                       count_global, gt, stream);
}
static int plan_create_replicated_impl(ls_amd_plan **out, ls_hs_operator const *op, ls_amd_dtype dtype,
                                       int num_partitions, int my_partition, uint64_t const *d_reps_local,
                                       int64_t count_local, uint64_t const *d_reps_global, int64_t count_global,
                                       ls_amd_gtab *gt, void *stream) {
    *out = NULL;
    if (!op || !op->basis) return set_error("null operator");
    if (ls_hs_basis_number_words(op->basis) != 1) return set_error("bases with more than 64 bits are not yet implemented");
    if (!OEXT(op)->is_hermitian) return set_error("replicated-x (pull) plans need a Hermitian operator");
    if (BEXT(op->basis)->fermi) return set_error("projected fermionic bases: replicated-x plans are not supported (one partition only)");
    if (num_partitions < 1 || num_partitions > LSK_MAX_PARTS || my_partition < 0 || my_partition >= num_partitions)
        return set_error("bad partition arguments");
    if (dtype == LS_AMD_F64 && !OEXT(op)->is_real) return set_error("an operator with complex coefficients needs dtype c128");
    ls_amd_plan *pl = (ls_amd_plan *)calloc(1, sizeof(*pl));
    pl->op = op;
    pl->cplx = dtype == LS_AMD_C128;
    pl->P = num_partitions;
    pl->me = my_partition;
    pl->n_local = 1;
    if (operator_device(op, &pl->dop) != 0 || basis_device(op->basis, &pl->dbs) != 0) { free(pl); return -1; }
    if (dtype == LS_AMD_F64)
        for (int g = 0; g < BEXT(op->basis)->order; ++g)
            if (BEXT(op->basis)->elems[g].ch_im != 0.0) { free(pl); return set_error("complex characters need dtype c128"); }
    pl->family = pl->dbs.proj == LSK_PROJ_FULL ? FAMILY_REPL_TILE : FAMILY_REPL_DIRECT;
    void *p;
    if (lsk_malloc(&p, sizeof(int)) != 0) { free(pl); return dev_error(); }
    pl->d_err = (int *)p;
    int zero = 0;
    lsk_h2d(pl->d_err, &zero, sizeof(int));
    pl->parts = (part_state *)calloc(1, sizeof(part_state));
    part_state *ps = &pl->parts[0];
    ps->count = count_local;
    ps->d_reps = d_reps_local;
    ps->rounds = 1;
    if (gt) {
        /* indexed mode: the static table replaces every other index of the global basis */
        if (pl->family != FAMILY_REPL_TILE) { ls_amd_plan_destroy(pl); return set_error("indexed replicated-x plans are for projected bases"); }
        if (!(d_reps_local >= d_reps_global && d_reps_local + count_local <= d_reps_global + count_global)) {
            ls_amd_plan_destroy(pl);
            return set_error("indexed replicated-x plans need a contiguous block of the global rows");
        }
        pthread_mutex_lock(&g_gtab_lock);
        ++gt->refs;
        pthread_mutex_unlock(&g_gtab_lock);
        pl->gtab = gt;
        pl->idx_mode = 1;
        pl->row_g0 = (int64_t)(d_reps_local - d_reps_global);
        pl->gindex.kind = LSK_INDEX_SEARCH;
        pl->gindex.count = count_global;
        pl->gindex.reps = d_reps_global;
        pl->pull_halo = pull_halo_setting(1);
        if (lsk_malloc(&p, 8 * (size_t)(count_local > 0 ? count_local : 1)) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
        ps->d_norms = (double *)p;
        if (lsk_norms(pl->dbs, count_local, d_reps_local, ps->d_norms, stream) != 0 || lsk_sync(stream) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
        *out = pl;
        return 0;
    }
    /* index of the GLOBAL basis: reuse the single-partition logic on a temporary part */
    {
        ls_amd_plan tmp = *pl;
        part_state gps;
        memset(&gps, 0, sizeof(gps));
        gps.count = count_global;
        gps.d_reps = d_reps_global;
        tmp.P = 1;
        tmp.family = FAMILY_DIRECT_PULL; /* no tile-side tables */
        tmp.global_index = 1;
        if (pl->dbs.proj == LSK_PROJ_FULL) {
            uint64_t const *d_binom;
            if (device_binom(&d_binom) != 0) { ls_amd_plan_destroy(pl); return -1; }
            gps.index.count = count_global; gps.index.reps = d_reps_global; gps.index.binom = d_binom;
            if (count_global > 0 && build_search_index(&gps, NBITS(op->basis), stream) != 0) { ls_amd_plan_destroy(pl); return -1; }
        } else if (plan_setup_part(&tmp, &gps, 0, 1, stream) != 0) { ls_amd_plan_destroy(pl); return -1; }
        pl->gindex = gps.index;
        pl->d_gtable = gps.d_table;
    }
    if (pl->family == FAMILY_REPL_DIRECT) {
        /* rows that are a contiguous block [row0, row0 + count_local) of the global basis (what ReplicatedOperator
         * hands over: a slice of the global array) can take the staged kernel */
        int const contiguous = d_reps_local >= d_reps_global && d_reps_local + count_local <= d_reps_global + count_global;
        if (contiguous && pl->gindex.kind == LSK_INDEX_COMBINADIC && chain_eligible(pl)) {
            pl->chain_row0 = (int64_t)(d_reps_local - d_reps_global);
            if (setup_chain(pl, pl->gindex, count_local, d_reps_local, stream) != 0) { ls_amd_plan_destroy(pl); return -1; }
        }
        if (!pl->has_chain && build_tilemap(pl, count_local, 256) != 0) { ls_amd_plan_destroy(pl); return -1; }
    }
    if (pl->gindex.kind == LSK_INDEX_SEARCH && count_local > 0) {
        if (lsk_malloc(&p, 8 * (size_t)count_local) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
        pl->d_row_gidx = (int64_t *)p;
        if (lsk_state_index(pl->gindex, count_local, d_reps_local, pl->d_row_gidx, stream) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
    }
    if (pl->family == FAMILY_REPL_TILE) {
        if (lsk_malloc(&p, 8 * (size_t)(count_local > 0 ? count_local : 1)) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
        ps->d_norms = (double *)p;
        if (lsk_norms(pl->dbs, count_local, d_reps_local, ps->d_norms, stream) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
        if (pl->dbs.k4_mode != 0) {
            if (lsk_malloc(&p, 8 * (size_t)(count_global > 0 ? count_global : 1)) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
            pl->d_norms_global = (double *)p;
            if (lsk_norms(pl->dbs, count_global, d_reps_global, pl->d_norms_global, stream) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
        }
    }
    if (lsk_sync(stream) != 0) { ls_amd_plan_destroy(pl); return dev_error(); }
    *out = pl;
    return 0;
}

int ls_amd_internal_basis_is_projected(ls_hs_basis const *b) { return BEXT(b)->order > 1; }
/* does the plan's K4 mode read x * norm(rep)?  (then the owners prescale their blocks in the indexed exchange) */
int ls_amd_internal_plan_prescales(ls_amd_plan const *pl) { return pl->dbs.k4_mode != 0; }
/* norm(rep) of the `count` representatives a rank owns, in its own order (freshly allocated; the caller lsk_free's it):
 * the rows are pulled out of the global array through the slot permutation, then K4's stabiliser sum */
int ls_amd_internal_owner_norms(ls_hs_operator const *op, ls_amd_gtab const *gt, int me, double **d_norms, void *stream) {
    lsk_basis dbs;
    *d_norms = NULL;
    if (basis_device(op->basis, &dbs) != 0) return -1;
    int64_t const cnt = gt->counts[me];
    void *reps = NULL, *nrm = NULL;
    if (lsk_malloc(&reps, 8 * (size_t)(cnt > 0 ? cnt : 1)) != 0) return dev_error();
    if (lsk_malloc(&nrm, 8 * (size_t)(cnt > 0 ? cnt : 1)) != 0) { lsk_free(reps); return dev_error(); }
    int const rc = lsk_scatter_owned(gt->n, gt->d_perm, (int64_t)me * gt->max_count, cnt, gt->reps, (uint64_t *)reps, stream) ||
                   lsk_norms(dbs, cnt, (uint64_t const *)reps, (double *)nrm, stream) || lsk_sync(stream);
    lsk_free(reps);
    if (rc) { lsk_free(nrm); return dev_error(); }
    *d_norms = (double *)nrm;
    return 0;
}

int ls_amd_matvec_replicated(ls_amd_plan *pl, void const *d_x_global, void *d_y_local, void *stream) {
    part_state *ps = &pl->parts[0];
    int slot;
    ls_amd_internal_count_matvec(pl);
    if (pl->family == FAMILY_REPL_DIRECT) {
        int const st = stage_begin(pl, ST_ROWS, stream);
        slot = timing_begin(pl, stream);
        if (pl->has_chain)
            DEV(lsk_chain(pl->dop, pl->dbs, pl->gindex, pl->cplx, pl->chain_wide, pl->d_chain_rec != NULL, pl->tilemap, ps->count,
                          pl->d_chain_rec ? pl->d_chain_rec : ps->d_reps, pl->chain_row0, pl->gindex.count, d_x_global, d_y_local,
                          pl->chain_cached, pl->d_chain_cache, pl->chain_v[0], pl->chain_v[1], pl->d_chain_wave, stream));
        else
            DEV(lsk_direct_gx(pl->dop, pl->dbs, pl->gindex, pl->cplx, pl->tilemap, ps->d_reps, pl->d_row_gidx, d_x_global,
                          d_y_local, pl->d_err, stream));
        timing_end(pl, slot, stream);
        stage_end(pl, st, stream);
        return 0;
    }
    if (pl->family == FAMILY_REPL_TILE && pl->idx_mode) {
        /* d_x_global = the owners' blocks in slot order, already multiplied by norm(rep) where the K4 mode prescales */
        lsk_pullidx ix;
        ix.tab = pl->gtab->tab;
        ix.perm = pl->gtab->d_perm;
        ix.row_g0 = pl->row_g0;
        ix.vtab = NULL;
        int const st = stage_begin(pl, ST_ROWS, stream);
        slot = timing_begin(pl, stream);
        DEV(lsk_tile_pull_idx(pl->dop, pl->dbs, pl->cplx, 0, ps->count, ps->d_reps, ps->d_norms, ix, pl->gindex.reps,
                              pl->gindex.count, d_x_global, pl->pull_halo, d_y_local, pl->d_err, stream));
        timing_end(pl, slot, stream);
        stage_end(pl, st, stream);
        return 0;
    }
    if (pl->family == FAMILY_REPL_TILE) {
        void const *xg;
        if (prescaled_x(pl, pl->gindex.count, pl->gindex.reps, d_x_global, pl->d_norms_global, &xg, stream) != 0) return -1;
        int const st = stage_begin(pl, ST_ROWS, stream);
        slot = timing_begin(pl, stream);
        DEV(lsk_tile_pull(pl->dop, pl->dbs, pl->gindex, pl->cplx, 0, ps->count, ps->d_reps, ps->d_norms,
                          pl->d_norms_global, pl->d_row_gidx, xg, pl->htab_bits, pl->gindex.reps, pl->gindex.count,
                          pl->d_xs ? pl->d_xs : d_x_global, pl->pull_halo, d_x_global, d_y_local, pl->d_err, stream));
        timing_end(pl, slot, stream);
        stage_end(pl, st, stream);
        return 0;
    }
    return set_error("ls_amd_matvec_replicated: not a replicated-x plan");
}
/* Plan time (dist.c, replicated-x exchange of an unprojected basis): the blocks of 2^shift rows of the global vector that this
 * plan's rows read -- every off-diagonal partner, plus the rows themselves with `halo` rows either side (the LDS windows of the
 * staged kernels; row0 = global index of the plan's first row).  h_bitmap[nwords] is overwritten.  Returns 0, 1 when the question does not apply (projected bases read x
 * through the index table; inversion sectors canonicalise the partner first: they keep the whole vector), -1 on a device error. */
int ls_amd_internal_plan_reach(ls_amd_plan *pl, int shift, int64_t row0, int64_t halo, int64_t nwords, uint32_t *h_bitmap, void *stream) {
    if (pl->family != FAMILY_REPL_DIRECT || pl->dbs.proj != LSK_PROJ_NONE) return 1;
    part_state *ps = &pl->parts[0];
    int64_t const n_global = pl->gindex.count;
    if (((n_global - 1) >> shift) / 32 >= nwords) return set_error("internal error: reach bitmap too small");
    memset(h_bitmap, 0, 4 * (size_t)nwords);
    if (ps->count <= 0) return 0;
    void *d = NULL;
    DEV(lsk_malloc(&d, 4 * (size_t)nwords));
    if (lsk_memset_async(d, 0, 4 * (size_t)nwords, stream) != 0 ||
        lsk_reach_blocks(pl->dop, pl->gindex, ps->count, ps->d_reps, shift, (uint32_t *)d, stream) != 0 || lsk_sync(stream) != 0 ||
        lsk_d2h(h_bitmap, d, 4 * (size_t)nwords) != 0) { lsk_free(d); return dev_error(); }
    lsk_free(d);
    /* own rows [row0, row0 + count) +- halo */
    int64_t g0 = row0, g1 = g0 + ps->count;
    g0 = g0 > halo ? g0 - halo : 0;
    g1 = g1 + halo < n_global ? g1 + halo : n_global;
    for (int64_t b = g0 >> shift; b <= (g1 - 1) >> shift; ++b) h_bitmap[b >> 5] |= 1u << (b & 31);
    return 0;
}

/* The indexed replicated-x matvec in two steps (dist.c): BEGIN resolves the packets of the first split_rows rows -- stage A,
 * K4 and every slot look-up, nothing of x -- and is enqueued while the blocks of x travel; FINISH gathers them from the
 * received x and runs the fused kernel on whatever rows the packet buffer did not cover. */
int ls_amd_internal_repl_split_begin(ls_amd_plan *pl, void *stream) {
    if (pl->family != FAMILY_REPL_TILE || !pl->idx_mode || pl->split_rows <= 0) return 0;
    if (pl->slot_cache && pl->slot_cache_valid) return 0; /* the streams of an earlier matvec are still good */
    part_state *ps = &pl->parts[0];
    lsk_pullidx ix;
    ix.tab = pl->gtab->tab;
    ix.perm = pl->gtab->d_perm;
    ix.row_g0 = pl->row_g0;
    ix.vtab = NULL;
    int const st = stage_begin(pl, ST_GENERATE, stream);
    int const slot = timing_begin(pl, stream);
    DEV(lsk_tile_pull_resolve(pl->dop, pl->dbs, 0, split_rows_now(pl), ps->d_reps, ps->d_norms, ix, pl->gindex.reps, pl->gindex.count,
                              pl->pull_halo, pl->pbuf, pl->d_err, stream));
    pl->slot_cache_valid = pl->slot_cache; /* only once the resolve launch went through: a failed one leaves nothing to reuse */
    timing_end(pl, slot, stream);
    stage_end(pl, st, stream);
    return 0;
}
/* rows [row0, row1) of the split matvec (row0 a multiple of 256): what was resolved ahead is gathered, the rest takes the fused
 * kernel.  The chunked return of the replicated-x driver calls it once per chunk of rows; count = 1: this call opens the matvec. */
int ls_amd_internal_repl_split_rows(ls_amd_plan *pl, void const *d_x_global, void *d_y_local, int64_t row0, int64_t row1, int count, void *stream) {
    if (pl->family != FAMILY_REPL_TILE || !pl->idx_mode || pl->split_rows <= 0) return set_error("internal error: not a split plan");
    part_state *ps = &pl->parts[0];
    if (row1 > ps->count) row1 = ps->count;
    if (row0 < 0 || (row0 & 255) != 0 || row0 > row1) return set_error("internal error: bad row range of the split matvec");
    if (count) ls_amd_internal_count_matvec(pl);
    lsk_pullidx ix;
    ix.tab = pl->gtab->tab;
    ix.perm = pl->gtab->d_perm;
    ix.row_g0 = pl->row_g0;
    ix.vtab = NULL;
    int64_t const S = split_rows_now(pl);
    int const st = stage_begin(pl, ST_ROWS, stream);
    if (row0 < S) {
        int const slot = pl->slot_cache ? timing_begin(pl, stream) : -1; /* cached: the gather kernel is the dominant (only) one */
        DEV(lsk_tile_pull_gather(pl->dop, pl->dbs, pl->cplx, row0, row1 < S ? row1 : S, ps->d_reps, ps->d_norms, ix, d_x_global, pl->pbuf, d_y_local,
                                 stream));
        if (slot >= 0) timing_end(pl, slot, stream);
    }
    if (row1 > S)
        DEV(lsk_tile_pull_idx(pl->dop, pl->dbs, pl->cplx, row0 > S ? row0 : S, row1, ps->d_reps, ps->d_norms, ix, pl->gindex.reps,
                              pl->gindex.count, d_x_global, pl->pull_halo, d_y_local, pl->d_err, stream));
    stage_end(pl, st, stream);
    return 0;
}
int ls_amd_internal_repl_split_finish(ls_amd_plan *pl, void const *d_x_global, void *d_y_local, void *stream) {
    if (pl->family != FAMILY_REPL_TILE || !pl->idx_mode || pl->split_rows <= 0) return ls_amd_matvec_replicated(pl, d_x_global, d_y_local, stream);
    return ls_amd_internal_repl_split_rows(pl, d_x_global, d_y_local, 0, pl->parts[0].count, 1, stream);
}
char const *ls_amd_plan_kernel_name(ls_amd_plan const *pl) {
    switch (pl->family) {
    case FAMILY_DIRECT_PUSH: return pl->has_push_staged ? "direct-push+staged" : "direct-push";
    case FAMILY_DIRECT_PULL:
        if (pl->has_hubbard) return "direct-pull+hubbard";
        return pl->has_chain ? "direct-pull+staged" : pl->has_pairs ? (pl->pairs.sites ? "direct-pull+pairsites" : pl->pairs.rows ? "direct-pull+pairrows" : "direct-pull+pairs") : "direct-pull";
    case FAMILY_TILE_PULL: return pl->idx_mode ? (pl->slot_cache ? "tile-pull+indexed+cached" : (pl->d_vtab ? "tile-pull+values" : "tile-pull+indexed")) : "tile-pull";
    case FAMILY_REPL_DIRECT:
        return pl->has_chain ? "replicated-direct-pull+staged" : "replicated-direct-pull";
    case FAMILY_REPL_TILE: return pl->idx_mode ? (pl->slot_cache ? "replicated-tile-pull+indexed+cached" : "replicated-tile-pull+indexed") : "replicated-tile-pull";
    default: return pl->streams ? "tile+streams" : (pl->has_push_staged ? "tile(one rank: push+staged)" : "tile");
    }
}
/* nominal bytes per packet (a segment of c packets takes ls_amd_plan_segment_bytes(c): pre-indexed keys are padded to 8 bytes) */
int ls_amd_plan_packet_bytes(ls_amd_plan const *pl) { return pl->key_bytes + (pl->cplx ? 16 : 8); }
/* bytes of per-row plan / basis data the plan's dominant kernel streams from HBM next to x and y (the roofline's
 * compulsory traffic is rows * (this + 2 w)): the staged row kernel reads the fused 8-byte record, or the low state word(s)
 * plus one cached partner rank per cached pair -- with wave headers (setup_chain_headers) 8 bytes per wave-row and those records
 * only for the wave-rows without one, rounded up; the generic row kernels read the 8-byte state; the projected pull kernel
 * the state and norm(alpha) */
int ls_amd_plan_row_bytes(ls_amd_plan const *pl) {
    if (pl->has_hubbard) return 0; /* the species tables are O(sqrt N) and cache-resident: x and y are the whole stream */
    if (pl->has_pairs) return pl->pairs.wide ? 8 : 4; /* the plan's 4-byte copy of the states, or (33..64 sites) the 8-byte representatives */
    if (pl->has_chain) {
        if (pl->d_chain_wave) return pl->chain_row_bytes; /* the records' bytes, or with wave headers what they and the remaining records come to */
        int const narrow = NBITS(pl->op->basis) <= 32 && !pl->chain_wide;
        return (narrow ? 4 : 8) + pl->chain_cached * (pl->chain_wide ? 8 : 4);
    }
    if (pl->family == FAMILY_TILE_PULL || pl->family == FAMILY_REPL_TILE) return 16;
    return 8;
}
/* rows that the plan's paired launch computes (k_chain_pair_t, setup_chain_pairs); 0: the plan runs on k_chain_t alone, or not on it */
int64_t ls_amd_plan_chain_paired_rows(ls_amd_plan const *pl) {
    return pl->has_chain && pl->chain_paired ? pl->chain_pair_rows[1] : 0;
}
/* ... across the bond of `level` (1: bond L - 2, 2: L - 4, ...), and the deepest level at which the plan pairs rows (0: unpaired) */
int64_t ls_amd_plan_chain_paired_rows_at(ls_amd_plan const *pl, int level) {
    return pl->has_chain && pl->chain_paired && level >= 1 && level <= CHAIN_MAX_PAIR_LEVELS ? pl->chain_pair_rows[level] : 0;
}
int ls_amd_plan_chain_pair_levels(ls_amd_plan const *pl) { return pl->has_chain && pl->chain_paired ? pl->chain_pair_levels : 0; }
int64_t ls_amd_plan_nnz(ls_amd_plan const *pl) { return pl->nnz; }
int ls_amd_plan_send_counts(ls_amd_plan const *pl, int round, int64_t *counts) {
    if (pl->family != FAMILY_TILE) { for (int d = 0; d < pl->P; ++d) counts[d] = 0; return 0; }
    part_state const *ps = &pl->parts[0];
    if (round < 0 || round >= ps->rounds) return set_error("round out of range");
    memcpy(counts, ps->send_counts + (size_t)round * pl->P, sizeof(int64_t) * pl->P);
    return 0;
}

/* hash table over `n` (global) representatives: built on first use, values refreshed per matvec */
static int prescaled_x(ls_amd_plan *pl, int64_t n, uint64_t const *d_reps, void const *d_x, double const *d_norms,
                       void const **out, void *stream) {
    if (!pl->d_htab) {
        int bits = 4;
        while (((int64_t)1 << bits) < 2 * n) ++bits; /* load factor <= 0.5 */
        if (bits > 32) return set_error("hash index: more than 2^31 representatives per table are not supported");
        pl->htab_bits = bits;
        DEV(lsk_malloc(&pl->d_htab, (size_t)(pl->cplx ? 32 : 16) << bits));
        void *p;
        DEV(lsk_malloc(&p, 4 * (size_t)(n > 0 ? n : 1)));
        pl->d_slot_of = (uint32_t *)p;
        DEV(lsk_hash_build(pl->cplx, n, d_reps, bits, pl->d_htab, pl->d_slot_of, stream));
        /* near window (LS_AMD_PULL_HALO entries either side of a tile, default 512, 0 = every partner through the table) */
        pl->pull_halo = pull_halo_setting(0);
        if (pl->pull_halo > 0 && pl->dbs.k4_mode != 0) DEV(lsk_malloc(&pl->d_xs, (size_t)(pl->cplx ? 16 : 8) * (size_t)(n > 0 ? n : 1)));
    }
    int const st = stage_begin(pl, ST_REFRESH, stream);
    DEV(lsk_hash_fill(pl->cplx, n, pl->d_slot_of, d_x, pl->dbs.k4_mode != 0 ? d_norms : NULL, pl->d_htab, pl->d_xs, stream));
    stage_end(pl, st, stream);
    *out = pl->d_htab;
    return 0;
}

int ls_amd_diag(ls_amd_plan *pl, void const *d_x, void *d_y, void *stream) {
    part_state *ps = &pl->parts[0];
    int const st = stage_begin(pl, ST_DIAG, stream);
    if (pl->has_push_staged) { /* the staged push kernel adds the diagonal part itself: y is cleared (no diagonal terms: accumulated into) */
        if (pl->dop.n_diag > 0) DEV(lsk_memset_async(d_y, 0, (size_t)ps->count * (pl->cplx ? 16 : 8), stream));
    } else
    DEV(lsk_diag(pl->dop, pl->cplx, ps->count, ps->d_reps, d_x, d_y, stream));
    stage_end(pl, st, stream);
    return 0;
}

static int generate_round(ls_amd_plan *pl, part_state *ps, int pid, int round, void const *d_x, void *d_y,
                          void *d_send, void *stream) {
    int64_t row0 = ps->count * round / ps->rounds, row1 = ps->count * (round + 1) / ps->rounds;
    if (pl->P > 1 && !ps->d_wtab) DEV(lsk_memset_async(pl->d_cursors, 0, 8 * (size_t)pl->P, stream));
    int const st = stage_begin(pl, ST_GENERATE, stream);
    int slot = timing_begin(pl, stream);
    if (pl->has_push_staged) { /* (FAMILY_TILE, one rank, one round: every packet is this partition's own) */
        lsk_index cix = ps->index;
        cix.kind = LSK_INDEX_COMBINADIC;
        DEV(lsk_push_staged(pl->dop, pl->dbs, cix, pl->cplx, pl->tilemap, ps->count, ps->d_reps, d_x, d_y, pl->d_err, stream));
    } else if (pl->streams) {
        uint64_t const *d_binom;
        if (device_binom(&d_binom) != 0) return -1;
        DEV(lsk_tile_st(pl->dop, pl->gd, d_binom, pl->cplx, 0, pl->P, pl->st_S, pl->st_tile_rows, row0, row1, ps->d_reps, d_x,
                        ps->d_ttab + (size_t)ps->ttab_first[round] * (size_t)(pl->P * pl->st_S), ps->d_layouts + round, d_send, pl->d_err, stream));
    } else if (ps->d_wtab)
        DEV(lsk_tile_wv(pl->dop, pl->dbs, ps->index, pl->gd, pl->cplx, 0, pl->P, pid, row0, row1, ps->d_reps, ps->d_norms, d_x, d_y,
                        ps->d_wtab + (size_t)ps->wtab_first[round] * pl->P, ps->d_layouts + round, d_send, pl->d_err,
                        ps->scatter_gt ? ps->scatter_gt->tab : no_gtab(), stream));
    else
        DEV(lsk_tile(pl->dop, pl->dbs, ps->index, pl->cplx, 0, pl->P, pid, row0, row1, ps->d_reps, ps->d_norms, d_x,
                     d_y, pl->d_cursors, ps->d_layouts + round, d_send, pl->d_counts, pl->d_err, stream));
    timing_end(pl, slot, stream);
    stage_end(pl, st, stream);
    return 0;
}

int ls_amd_generate(ls_amd_plan *pl, int round, void const *d_x, void *d_y, void *d_send, void *stream) {
    if (pl->family != FAMILY_TILE) return set_error("ls_amd_generate: the plan uses a direct kernel (P == 1)");
    if (pl->me < 0) return set_error("ls_amd_generate: plan owns all partitions; use ls_amd_matvec");
    part_state *ps = &pl->parts[0];
    if (round < 0 || round >= ps->rounds) return set_error("round out of range");
    return generate_round(pl, ps, pl->me, round, d_x, d_y, d_send, stream);
}

int ls_amd_scatter(ls_amd_plan *pl, int64_t n, uint64_t const *d_betas, void const *d_values, void *d_y,
                   void *stream) {
    part_state *ps = &pl->parts[0];
    if (pl->streams) return set_error("ls_amd_scatter: the plan writes sorted streams (consumed by windows, dist.c)");
    if (ps->index.kind == LSK_INDEX_COMBINADIC || ps->index.kind == LSK_INDEX_PRODUCT) return set_error("ls_amd_scatter: plan has no search index");
    int const st = stage_begin(pl, ST_SCATTER, stream);
    if (pl->key_bytes == 4) { /* pre-indexed packets: d_betas is the segment's u32 index array */
        lsk_segs sg;
        memset(&sg, 0, sizeof(sg));
        sg.n = 1; sg.start[0] = 0; sg.start[1] = n; sg.key_off[0] = 0;
        sg.val_off[0] = (int64_t)((char const *)d_values - (char const *)d_betas);
        sg.y[0] = d_y;
        DEV(lsk_scatter_idx(pl->cplx, &sg, d_betas, stream));
    } else
        DEV(lsk_scatter(ps->index, pl->cplx, n, d_betas, d_values, d_y, pl->dbs.k4_mode ? ps->d_norms : NULL, pl->d_err,
                        stream));
    stage_end(pl, st, stream);
    return 0;
}
/* All segments of one round's receive buffer in ONE launch (consumer side of a rank): segment s holds counts[s] packets at
 * d_recv + offsets[s], laid out as ls_amd_plan_segment_bytes describes.  (The per-segment form above cost 56 launches per
 * matvec on chain_28 x 8.) */
int ls_amd_scatter_round(ls_amd_plan *pl, int num_segments, int64_t const *counts, int64_t const *offsets, void const *d_recv,
                         void *d_y, void *stream) {
    part_state *ps = &pl->parts[0];
    if (pl->streams) return set_error("ls_amd_scatter_round: the plan writes sorted streams (consumed by windows, dist.c)");
    if (ps->index.kind == LSK_INDEX_COMBINADIC || ps->index.kind == LSK_INDEX_PRODUCT) return set_error("ls_amd_scatter_round: plan has no search index");
    int const st = stage_begin(pl, ST_SCATTER, stream);
    int s = 0;
    while (s < num_segments) {
        lsk_segs sg;
        memset(&sg, 0, sizeof(sg));
        int64_t total = 0;
        for (; s < num_segments && sg.n < LSK_MAX_SEGS; ++s) {
            if (counts[s] <= 0) continue;
            sg.start[sg.n] = total;
            sg.key_off[sg.n] = offsets[s];
            sg.val_off[sg.n] = offsets[s] + segment_key_bytes(pl, counts[s]);
            sg.y[sg.n] = d_y;
            total += counts[s];
            ++sg.n;
        }
        if (sg.n == 0) break;
        sg.start[sg.n] = total;
        if (pl->key_bytes == 4) DEV(lsk_scatter_idx(pl->cplx, &sg, d_recv, stream));
        else {
            DEV(lsk_scatter_segs(ps->index, ps->scatter_gt ? ps->scatter_gt->tab : no_gtab(), pl->cplx, &sg, d_recv, pl->dbs.k4_mode ? ps->d_norms : NULL, pl->d_err, stream));
        }
    }
    stage_end(pl, st, stream);
    return 0;
}
/* sorted streams of a plan that owns one partition (dist.c): S streams per segment; offsets[rounds][P][S + 1] = where the streams
 * of the segment for destination d start in round r (packets); the consumer of one round over n_src source segments */
int ls_amd_internal_plan_streams(ls_amd_plan const *pl) { return pl->streams ? pl->st_S : 0; }
uint32_t const *ls_amd_internal_plan_stream_offsets(ls_amd_plan const *pl) { return pl->streams ? pl->parts[0].h_soff : NULL; }
int ls_amd_internal_window_round(ls_amd_plan *pl, lsk_wsrc const *d_srcs, int n_src, void *d_y, void *stream) {
    if (!pl->streams || pl->me < 0) return set_error("ls_amd_internal_window_round: not a streams plan of one partition");
    lsk_wdests wd;
    memset(&wd, 0, sizeof(wd));
    int const W = lsk_window_rows(pl->cplx);
    int64_t const windows = (pl->parts[0].count + W - 1) / W;
    wd.n = 1;
    wd.count[0] = pl->parts[0].count;
    wd.y[0] = d_y;
    wd.first_block[1] = (windows + pl->st_wpb - 1) / pl->st_wpb;
    if (pl->stream_gkeys) {
        uint64_t const *d_binom;
        if (device_binom(&d_binom) != 0) return -1;
        wd.dir[0] = pl->parts[0].index.dir; wd.reps[0] = pl->parts[0].d_reps;
        wd.binom = d_binom; wd.n_ranks = pl->gd.n_ranks; wd.weight = pl->gd.weight; wd.err = pl->d_err;
    }
    int const st = stage_begin(pl, ST_SCATTER, stream);
    DEV(lsk_window(pl->cplx, &wd, d_srcs, n_src, pl->st_S, pl->st_wpb, stream));
    stage_end(pl, st, stream);
    return 0;
}
int ls_amd_plan_key_bytes(ls_amd_plan const *pl) { return pl->key_bytes; }
int64_t ls_amd_plan_segment_bytes(ls_amd_plan const *pl, int64_t count) { return segment_key_bytes(pl, count) + (pl->cplx ? 16 : 8) * count; }
int64_t ls_amd_plan_segment_value_offset(ls_amd_plan const *pl, int64_t count) { return segment_key_bytes(pl, count); }
int64_t ls_amd_plan_packet_index_bytes(ls_amd_plan const *pl) {
    return pl->d_gdir ? (int64_t)sizeof(lsk_rankdir) * ((pl->gd.n_ranks + 63) / 64) * pl->gd.P : 0;
}

int ls_amd_matvec(ls_amd_plan *pl, void const *const *d_x, void *const *d_y, void *stream) {
    if (pl->me >= 0) return set_error("ls_amd_matvec: plan owns one partition; drive it with generate/scatter");
    for (int p = 0; p < pl->n_local; ++p) if (ls_amd_internal_check_y(pl, d_y[p]) != 0) return -1;
    ls_amd_internal_count_matvec(pl);
    if (pl->family == FAMILY_TILE_PULL && pl->idx_mode) {
        /* indexed mode on one device: slot = index; the only per-matvec preparation is x * norm(rep), a streaming pass
         * (the value table of the other mode costs N random 16-byte writes) */
        part_state *ps = &pl->parts[0];
        void const *xs = d_x[0];
        if (pl->dbs.k4_mode != 0) {
            int const sr = stage_begin(pl, ST_REFRESH, stream);
            DEV(lsk_scale(pl->cplx, ps->count, d_x[0], ps->d_norms, pl->d_xs, stream));
            stage_end(pl, sr, stream);
            xs = pl->d_xs;
        }
        lsk_pullidx ix;
        ix.tab = pl->gtab->tab;
        ix.perm = NULL;
        ix.row_g0 = 0;
        ix.vtab = NULL;
        if (pl->d_vtab && (pl->slot_cache || pl->split_rows > 0)) { lsk_free(pl->d_vtab); pl->d_vtab = NULL; } /* a cache enabled later takes over */
        if (pl->split_rows > 0 && pl->slot_cache) {
            /* slot cache: the streams of rows [0, split_rows) are resolved by the first matvec and kept; later matvecs gather.
             * Rows the cache has no room for take the fused kernel */
            lsk_pullbuf const pb = pl->pbuf;
            int st, slot;
            if (!pl->slot_cache_valid) {
                st = stage_begin(pl, ST_GENERATE, stream);
                slot = timing_begin(pl, stream);
                DEV(lsk_tile_pull_resolve(pl->dop, pl->dbs, 0, pl->split_rows, ps->d_reps, ps->d_norms, ix, ps->d_reps, ps->count, pl->pull_halo, pb,
                                          pl->d_err, stream));
                timing_end(pl, slot, stream);
                stage_end(pl, st, stream);
                pl->slot_cache_valid = 1;
            }
            st = stage_begin(pl, ST_ROWS, stream);
            slot = timing_begin(pl, stream); /* the gather kernel is the dominant one of a cached plan */
            DEV(lsk_tile_pull_gather(pl->dop, pl->dbs, pl->cplx, 0, pl->split_rows, ps->d_reps, ps->d_norms, ix, xs, pb, d_y[0], stream));
            timing_end(pl, slot, stream);
            if (pl->split_rows < ps->count) {
                slot = timing_begin(pl, stream);
                DEV(lsk_tile_pull_idx(pl->dop, pl->dbs, pl->cplx, pl->split_rows, ps->count, ps->d_reps, ps->d_norms, ix, ps->d_reps, ps->count, xs,
                                      pl->pull_halo, d_y[0], pl->d_err, stream));
                timing_end(pl, slot, stream);
            }
            stage_end(pl, st, stream);
            return 0;
        }
        if (pl->split_rows > 0) {
            /* the split form on one device (LS_AMD_PULL_SPLIT: measurement of what the replicated-x exchange runs, dist.c):
             * rounds of resolve | gather over the rows the packet buffer holds */
            for (int64_t r0 = 0; r0 < ps->count; r0 += pl->split_rows) {
                int64_t const r1 = r0 + pl->split_rows < ps->count ? r0 + pl->split_rows : ps->count;
                lsk_pullbuf pb = pl->pbuf;
                pb.row0 = r0;
                int st = stage_begin(pl, ST_GENERATE, stream);
                int const slot = timing_begin(pl, stream);
                DEV(lsk_tile_pull_resolve(pl->dop, pl->dbs, r0, r1, ps->d_reps, ps->d_norms, ix, ps->d_reps, ps->count, pl->pull_halo, pb,
                                          pl->d_err, stream));
                timing_end(pl, slot, stream);
                stage_end(pl, st, stream);
                st = stage_begin(pl, ST_ROWS, stream);
                DEV(lsk_tile_pull_gather(pl->dop, pl->dbs, pl->cplx, r0, r1, ps->d_reps, ps->d_norms, ix, xs, pb, d_y[0], stream));
                stage_end(pl, st, stream);
            }
            return 0;
        }
        if (pl->d_vtab) { /* the values of this matvec's x (x n(rep) in the prescaling K4 modes) into their buckets: table order */
            int const sr = stage_begin(pl, ST_REFRESH, stream);
            DEV(lsk_vtab_refresh(pl->gtab->tab, pl->d_vtab, xs, stream));
            stage_end(pl, sr, stream);
            ix.vtab = pl->d_vtab;
        }
        int const st = stage_begin(pl, ST_ROWS, stream);
        int slot = timing_begin(pl, stream);
        DEV(lsk_tile_pull_idx(pl->dop, pl->dbs, pl->cplx, 0, ps->count, ps->d_reps, ps->d_norms, ix, ps->d_reps, ps->count, xs,
                              pl->pull_halo, d_y[0], pl->d_err, stream));
        timing_end(pl, slot, stream);
        stage_end(pl, st, stream);
        return 0;
    }
    if (pl->family == FAMILY_TILE_PULL) {
        part_state *ps = &pl->parts[0];
        void const *xg;
        if (prescaled_x(pl, ps->count, ps->d_reps, d_x[0], ps->d_norms, &xg, stream) != 0) return -1;
        int const st = stage_begin(pl, ST_ROWS, stream);
        int slot = timing_begin(pl, stream);
        DEV(lsk_tile_pull(pl->dop, pl->dbs, ps->index, pl->cplx, 0, ps->count, ps->d_reps, ps->d_norms, ps->d_norms,
                          NULL, xg, pl->htab_bits, ps->d_reps, ps->count, pl->d_xs ? pl->d_xs : d_x[0], pl->pull_halo, d_x[0],
                          d_y[0], pl->d_err, stream));
        timing_end(pl, slot, stream);
        stage_end(pl, st, stream);
        return 0;
    }
    /* localDiagonal on every partition first: y is assigned (DMV:1062-1063) */
    if (pl->has_push_staged) { /* the staged push kernel adds the diagonal part itself: y is cleared (n_diag == 0: accumulated into, DMV:1062-1063) */
        if (pl->dop.n_diag > 0) {
            int const st = stage_begin(pl, ST_DIAG, stream);
            DEV(lsk_memset_async(d_y[0], 0, (size_t)pl->parts[0].count * (pl->cplx ? 16 : 8), stream));
            stage_end(pl, st, stream);
        }
    } else if (pl->family != FAMILY_DIRECT_PULL) {
        int const st = stage_begin(pl, ST_DIAG, stream);
        for (int p = 0; p < pl->n_local; ++p)
            DEV(lsk_diag(pl->dop, pl->cplx, pl->parts[p].count, pl->parts[p].d_reps, d_x[p], d_y[p], stream));
        stage_end(pl, st, stream);
    }
    if (pl->dop.n_groups == 0 && pl->family != FAMILY_DIRECT_PULL) return 0;
    if (pl->family != FAMILY_TILE) {
        part_state *ps = &pl->parts[0];
        int const st = stage_begin(pl, ST_ROWS, stream);
        int slot = timing_begin(pl, stream);
        if (pl->has_chain) {
            DEV(lsk_chain(pl->dop, pl->dbs, ps->index, pl->cplx, pl->chain_wide, pl->d_chain_rec != NULL, pl->tilemap, ps->count,
                          pl->d_chain_rec ? pl->d_chain_rec : ps->d_reps, 0, ps->count, d_x[0], d_y[0], pl->chain_cached,
                          pl->d_chain_cache, pl->chain_v[0], pl->chain_v[1], pl->d_chain_wave, stream));
            if (pl->chain_paired) /* the rows that tile map leaves out (setup_chain_pairs) */
                DEV(lsk_chain_paired(pl->dop, pl->dbs, pl->tilemap_pair, ps->count, pl->d_chain_rec, d_x[0], d_y[0], pl->chain_cached, pl->chain_v[0],
                                     pl->d_chain_wave, pl->d_chain_hdr_b, stream));
        } else if (pl->has_pairs)
            DEV(lsk_pairs(pl->pairs, pl->dbs.hamming_weight, pl->cplx, pl->tilemap, ps->count, d_x[0], d_y[0], stream));
        else if (pl->has_hubbard)
            DEV(lsk_hubbard_apply(pl->hubbard, pl->dop, pl->cplx, pl->tilemap, d_x[0], d_y[0], stream));
        else if (pl->has_push_staged)
            DEV(lsk_push_staged(pl->dop, pl->dbs, ps->index, pl->cplx, pl->tilemap, ps->count, ps->d_reps, d_x[0], d_y[0], pl->d_err, stream));
        else
            DEV(lsk_direct(pl->dop, pl->dbs, ps->index, pl->cplx, pl->family == FAMILY_DIRECT_PULL ? (OEXT(pl->op)->is_hermitian ? 1 : 2) : 0, pl->tilemap, ps->d_reps,
                           d_x[0], d_y[0], pl->d_err, stream));
        timing_end(pl, slot, stream);
        stage_end(pl, st, stream);
        return 0;
    }
    int const P = pl->P;
    if (pl->streams) {
        /* sorted streams: every source writes its round into its own buffer, then ONE launch adds windows of every y in LDS */
        uint64_t const *d_binom;
        if (device_binom(&d_binom) != 0) return -1;
        int const W = lsk_window_rows(pl->cplx);
        lsk_wdests wd;
        memset(&wd, 0, sizeof(wd));
        wd.n = P;
        for (int d = 0; d < P; ++d) {
            int64_t const windows = (pl->parts[d].count + W - 1) / W;
            wd.count[d] = pl->parts[d].count;
            wd.y[d] = d_y[d];
            wd.first_block[d + 1] = wd.first_block[d] + (windows + pl->st_wpb - 1) / pl->st_wpb;
            if (pl->stream_gkeys) { wd.dir[d] = pl->parts[d].index.dir; wd.reps[d] = pl->parts[d].d_reps; }
        }
        if (pl->stream_gkeys) { wd.binom = d_binom; wd.n_ranks = pl->gd.n_ranks; wd.weight = pl->gd.weight; wd.err = pl->d_err; }
        for (int r = 0; r < pl->st_rounds; ++r) {
            int st = stage_begin(pl, ST_GENERATE, stream);
            for (int p = 0; p < P; ++p) {
                part_state *ps = &pl->parts[p];
                int64_t row0 = ps->count * r / ps->rounds, row1 = ps->count * (r + 1) / ps->rounds;
                int const slot = timing_begin(pl, stream);
                DEV(lsk_tile_st(pl->dop, pl->gd, d_binom, pl->cplx, 0, P, pl->st_S, pl->st_tile_rows, row0, row1, ps->d_reps, d_x[p],
                                ps->d_ttab + (size_t)ps->ttab_first[r] * (size_t)(P * pl->st_S), ps->d_layouts + r, pl->d_send_parts[p],
                                pl->d_err, stream));
                timing_end(pl, slot, stream);
            }
            stage_end(pl, st, stream);
            st = stage_begin(pl, ST_SCATTER, stream);
            DEV(lsk_window(pl->cplx, &wd, pl->d_wsrcs + (size_t)r * P * P, P, pl->st_S, pl->st_wpb, stream));
            stage_end(pl, st, stream);
        }
        return 0;
    }
    for (int p = 0; p < P; ++p) {
        part_state *ps = &pl->parts[p];
        for (int r = 0; r < ps->rounds; ++r) {
            if (generate_round(pl, ps, p, r, d_x[p], d_y[p], pl->d_send, stream) != 0) return -1;
            /* the "exchange": every destination consumes its segment straight from the send buffer */
            if (pl->key_bytes == 4) { /* pre-indexed packets: all destinations in one launch, each segment with its own y */
                for (int d0 = 0; d0 < P; d0 += LSK_MAX_SEGS) {
                    lsk_segs sg;
                    memset(&sg, 0, sizeof(sg));
                    int64_t total = 0;
                    for (int d = d0; d < P && d < d0 + LSK_MAX_SEGS; ++d) {
                        int64_t const c = ps->send_counts[(size_t)r * P + d];
                        if (d == p || c == 0) continue;
                        sg.start[sg.n] = total;
                        sg.key_off[sg.n] = ps->h_beta_off[(size_t)r * P + d];
                        sg.val_off[sg.n] = ps->h_val_off[(size_t)r * P + d];
                        sg.y[sg.n] = d_y[d];
                        total += c;
                        ++sg.n;
                    }
                    if (sg.n == 0) continue;
                    sg.start[sg.n] = total;
                    int const st = stage_begin(pl, ST_SCATTER, stream);
                    DEV(lsk_scatter_idx(pl->cplx, &sg, pl->d_send, stream));
                    stage_end(pl, st, stream);
                }
                continue;
            }
            if (pl->d_part_ctx) { /* state-carrying packets: one launch too, index and norms of a segment's destination from the context array */
                /* (a partition whose rank directory is missing while others have one keeps the per-segment form below) */
                int mixed = 0;
                for (int d = 0; d < P; ++d) if ((pl->parts[d].index.dir != NULL) != (pl->parts[pl->part_ctx_any].index.dir != NULL) && pl->parts[d].count > 0) mixed = 1;
                if (!mixed) {
                    for (int d0 = 0; d0 < P; d0 += LSK_MAX_SEGS) {
                        lsk_segs sg;
                        memset(&sg, 0, sizeof(sg));
                        int64_t total = 0;
                        for (int d = d0; d < P && d < d0 + LSK_MAX_SEGS; ++d) {
                            int64_t const c = ps->send_counts[(size_t)r * P + d];
                            if (d == p || c == 0) continue;
                            sg.start[sg.n] = total;
                            sg.key_off[sg.n] = ps->h_beta_off[(size_t)r * P + d];
                            sg.val_off[sg.n] = ps->h_val_off[(size_t)r * P + d];
                            sg.y[sg.n] = d_y[d];
                            sg.part[sg.n] = (uint8_t)d;
                            total += c;
                            ++sg.n;
                        }
                        if (sg.n == 0) continue;
                        sg.start[sg.n] = total;
                        int const st = stage_begin(pl, ST_SCATTER, stream);
                        DEV(lsk_scatter_parts(pl->d_part_ctx, pl->parts[pl->part_ctx_any].index, pl->cplx, &sg, pl->d_send, pl->d_err, stream));
                        stage_end(pl, st, stream);
                    }
                    continue;
                }
            }
            for (int d = 0; d < P; ++d) {
                int64_t c = ps->send_counts[(size_t)r * P + d];
                if (d == p || c == 0) continue;
                uint64_t const *betas = (uint64_t const *)((char *)pl->d_send + ps->h_beta_off[(size_t)r * P + d]);
                void const *vals = (char *)pl->d_send + ps->h_val_off[(size_t)r * P + d];
                int const st = stage_begin(pl, ST_SCATTER, stream);
                DEV(lsk_scatter(pl->parts[d].index, pl->cplx, c, betas, vals, d_y[d],
                                pl->dbs.k4_mode ? pl->parts[d].d_norms : NULL, pl->d_err, stream));
                stage_end(pl, st, stream);
            }
        }
    }
    return 0;
}

/* ============================================================================================ */
/* block matvec (ls_amd_matvec_block)                                                           */
/* ============================================================================================ */
enum { BLK_COLUMNS = 0, BLK_DIRECT = 1, BLK_PULL = 2 };
static char const *const g_blk_names[3] = { "columns", "k_direct_blk", "k_pull_gather_blk" };
/* the block kernel that can serve this plan, else BLK_COLUMNS: projected indexed pull plans (resolve + k_pull_gather_blk) and
 * unprojected pull plans (k_direct_blk); push plans, inversion sectors, value-table projected plans and packet plans loop columns */
static int block_kernel_of(ls_amd_plan const *pl) {
    if (pl->P != 1 || pl->me >= 0 || pl->n_local != 1) return BLK_COLUMNS;
    if (pl->family == FAMILY_TILE_PULL && pl->idx_mode && pl->dbs.proj == LSK_PROJ_FULL)
        return (!pl->cplx && lsk_pullbuf_coef_doubles(pl->dop, pl->dbs) == 2) ? BLK_COLUMNS : BLK_PULL;
    if (pl->family == FAMILY_DIRECT_PULL && pl->dbs.proj == LSK_PROJ_NONE && !pl->has_push_staged) return BLK_DIRECT;
    return BLK_COLUMNS;
}
/* LS_AMD_BLOCK: `columns`, `kernel`, anything else (`auto`) the fixed rule below ("Block matvec"):
 *   projected indexed pull: k_pull_gather_blk from K = 2 on;
 *   unprojected pull whose single-vector kernel is k_direct: k_direct_blk from K = 2 on;
 *   unprojected pull on a staged row kernel (k_chain_t, k_pairs_*, k_hubbard): columns.
 * K = 1 keeps the single-vector kernels. */
static int block_path(ls_amd_plan const *pl, int K) {
    int const kern = block_kernel_of(pl);
    char const *e = getenv("LS_AMD_BLOCK");
    if (kern == BLK_COLUMNS || (e && strcmp(e, "columns") == 0)) return BLK_COLUMNS;
    if (e && strcmp(e, "kernel") == 0) return kern;
    if (K < 2) return BLK_COLUMNS;
    if (kern == BLK_DIRECT && (pl->has_chain || pl->has_pairs || pl->has_hubbard)) return BLK_COLUMNS;
    return kern;
}
char const *ls_amd_plan_block_kernel_name(ls_amd_plan const *pl, int K) {
    if (!pl) { set_error("ls_amd_plan_block_kernel_name: plan is NULL"); return NULL; }
    if (K < 1 || K > 64) { set_error("ls_amd_plan_block_kernel_name: K = %d is outside [1, 64]", K); return NULL; }
    return g_blk_names[block_path(pl, K)];
}

/* what every entry point asks of an n x K block (element (i, k) at i * r + k * c): no two (i, k) on one element -- non-negative
 * strides, one of the two nested in the other */
static int block_strides(char const *who, int64_t n, int K, int64_t r, int64_t c, char const *name) {
    int ok = r >= 0 && c >= 0;
    if (ok && K > 1 && n > 1) ok = (c >= 1 && r >= c * K) || (r >= 1 && c >= r * n);
    else if (ok && K > 1) ok = c >= 1;
    else if (ok && n > 1) ok = r >= 1;
    if (!ok)
        return set_error("%s: strides (row %lld, column %lld) of %s make two elements of the %lld x %d block share "
                         "storage (need non-negative strides with row >= K * column, or column >= N * row)", who, (long long)r,
                         (long long)c, name, (long long)n, K);
    return 0;
}
/* whether the address ranges of two blocks of K columns meet; each block has its element width (the accumulator of the
 * time-evolution step is c128 next to f64 vectors) and its number of rows (the two sectors of a cross-sector plan) */
static int block_overlap(size_t wa, int64_t na, void const *a, int64_t ar, int64_t ac, size_t wb, int64_t nb, void const *b, int64_t br,
                         int64_t bc, int K) {
    uintptr_t const a0 = (uintptr_t)a, a1 = a0 + wa * (size_t)((na - 1) * ar + (int64_t)(K - 1) * ac + 1);
    uintptr_t const b0 = (uintptr_t)b, b1 = b0 + wb * (size_t)((nb - 1) * br + (int64_t)(K - 1) * bc + 1);
    return a0 < b1 && b0 < a1;
}

/* packet buffer of the projected block path: whole 256-row tiles, as many rows as LS_AMD_BLOCK_RESOLVE_BYTES (default 1 GiB) allow
 * -- at least one tile -- and no more than the plan has */
static int block_pbuf(ls_amd_plan *pl) {
    if (pl->blk_rows > 0) return 0;
    int64_t const cap = lsk_pullbuf_cap(pl->dop);
    int const nc = lsk_pullbuf_coef_doubles(pl->dop, pl->dbs);
    int64_t const per_stream = cap * (4 + 1 + 8 * nc) + 4;
    char const *e = getenv("LS_AMD_BLOCK_RESOLVE_BYTES");
    int64_t max_bytes = e ? atoll(e) : ((int64_t)1 << 30);
    if (max_bytes <= 0) max_bytes = (int64_t)1 << 30;
    int64_t streams = (pl->parts[0].count + 63) / 64;
    streams = (streams + 3) & ~(int64_t)3;
    if (streams * per_stream > max_bytes) streams = (max_bytes / per_stream) & ~(int64_t)3;
    if (streams < 4) streams = 4;
    for (;;) {
        void *a = NULL, *b = NULL, *c = NULL, *d = NULL;
        if (lsk_malloc(&a, (size_t)(streams * cap * 4)) == 0 && lsk_malloc(&b, (size_t)(streams * cap)) == 0 &&
            (nc == 0 || lsk_malloc(&c, (size_t)(streams * cap * 8 * nc)) == 0) && lsk_malloc(&d, (size_t)(streams * 4)) == 0) {
            pl->blk_pbuf.slots = (uint32_t *)a; pl->blk_pbuf.rows = (uint8_t *)b; pl->blk_pbuf.coefs = (double *)c;
            pl->blk_pbuf.counts = (uint32_t *)d;
            pl->blk_pbuf.cap = cap;
            pl->blk_pbuf.offs = NULL;
            pl->blk_rows = streams * 64;
            return 0;
        }
        if (a) lsk_free(a);
        if (b) lsk_free(b);
        if (c) lsk_free(c);
        if (d) lsk_free(d);
        if (streams <= 4) return dev_error();
        streams = (streams / 2 + 3) & ~(int64_t)3; /* no room: half as many rows */
    }
}

/* the tile map k_direct_blk / k_direct_cheb walk: the plan's own, or -- chain and pair plans tile by 512 / 1024 rows -- a 256-row
 * map of the block path's own, made on first use */
static int block_tilemap(ls_amd_plan *pl, lsk_tilemap *tm) {
    *tm = pl->tilemap;
    if (!(pl->has_chain || pl->has_pairs)) return 0;
    if (!pl->d_blk_tilemap) {
        uint64_t *flat = NULL;
        int64_t slots = 0;
        if (tilemap_host(pl->parts[0].count, 256, 0, &flat, &slots) < 0) return -1;
        int const up = upload(&pl->d_blk_tilemap, flat, sizeof(uint64_t) * (size_t)(8 * slots > 0 ? 8 * slots : 1));
        free(flat);
        if (up) return -1;
        pl->blk_tilemap.entries = (uint64_t const *)pl->d_blk_tilemap;
        pl->blk_tilemap.slots_per_xcd = slots;
    }
    *tm = pl->blk_tilemap;
    return 0;
}

/* ---- one driver for the three block steps on a matvec plan ----
 * ls_amd_matvec_block (STEP_PLAIN: Y <- H X), ls_amd_matvec_block_axpby (STEP_CHEB: Y <- alpha H X + beta X + gamma Y and two dots)
 * and ls_amd_matvec_block_axpby_acc (STEP_ACC: that, and Z += c Y) walk a plan the same way; they differ in the launcher of each
 * path, picked by step_direct / step_gather / step_column_tail below */
enum { STEP_PLAIN = 0, STEP_CHEB = 1, STEP_ACC = 2 };
typedef struct block_step {
    int kind;
    double alpha, beta, gamma;  /* STEP_CHEB, STEP_ACC */
    double *d_dots;             /* [2K] or NULL */
    char *z;                    /* STEP_ACC: the accumulator, its strides (in its own elements) and c */
    int64_t z_row, z_col;
    int z_cplx;
    double c_re, c_im;
} block_step;
/* the X and Y of a call: K columns, strides in elements of the plan's dtype */
typedef struct block_xy { int K; char const *x; int64_t xr, xc; char *y; int64_t yr, yc; } block_xy;

/* the head of every block entry on a matvec plan: the number of rows, 0 where there are none (the dots, if any, cleared), -1 on error */
static int64_t block_step_rows(char const *who, ls_amd_plan const *pl, int K, double *d_dots, void *stream) {
    if (!pl) return set_error("%s: plan is NULL", who);
    if (K < 1 || K > 64) return set_error("%s: K = %d is outside [1, 64]", who, K);
    if (pl->P != 1 || pl->me >= 0 || pl->n_local != 1)
        return set_error("%s: one-partition plans only (this plan has P = %d, my_partition = %d)", who, pl->P, pl->me);
    int64_t const n = pl->parts[0].count;
    if (n <= 0 && d_dots) DEV(lsk_memset_async(d_dots, 0, sizeof(double) * 2 * (size_t)K, stream));
    return n > 0 ? n : 0;
}
static int block_xy_check(char const *who, ls_amd_plan const *pl, block_xy const *b) {
    int64_t const n = pl->parts[0].count;
    size_t const w = pl->cplx ? 16 : 8;
    if (block_strides(who, n, b->K, b->xr, b->xc, "X") != 0 || block_strides(who, n, b->K, b->yr, b->yc, "Y") != 0) return -1;
    if (block_overlap(w, n, b->x, b->xr, b->xc, w, n, b->y, b->yr, b->yc, b->K)) return set_error("%s: X and Y overlap", who);
    return 0;
}

static int step_direct(ls_amd_plan *pl, lsk_tilemap tm, block_xy const *b, block_step const *s, void *stream) {
    part_state const *ps = &pl->parts[0];
    /* (a non-Hermitian operator's partners outside the basis go to the word nobody reads, as in lsk_direct) */
    int *const d_err = OEXT(pl->op)->is_hermitian ? pl->d_err : pl->d_err + 1;
    switch (s->kind) {
    case STEP_PLAIN:
        return lsk_direct_blk(pl->dop, pl->dbs, ps->index, pl->cplx, tm, ps->d_reps, b->K, b->x, b->xr, b->xc, b->y, b->yr, b->yc, d_err, stream);
    case STEP_CHEB:
        return lsk_direct_cheb(pl->dop, pl->dbs, ps->index, pl->cplx, tm, ps->d_reps, b->K, b->x, b->xr, b->xc, b->y, b->yr, b->yc, s->alpha,
                               s->beta, s->gamma, s->d_dots, d_err, stream);
    default:
        return lsk_direct_evolve(pl->dop, pl->dbs, ps->index, pl->cplx, tm, ps->d_reps, b->K, b->x, b->xr, b->xc, b->y, b->yr, b->yc, s->alpha,
                                 s->beta, s->gamma, s->z, s->z_row, s->z_col, s->z_cplx, s->c_re, s->c_im, s->d_dots, d_err, stream);
    }
}
/* rows [r0, r1) from the packet streams of pb; a STEP_CHEB / STEP_ACC launch adds its rows' share to the dots (and updates its
 * own rows of Z) */
static int step_gather(ls_amd_plan *pl, int64_t r0, int64_t r1, lsk_pullbuf pb, block_xy const *b, block_step const *s, void *stream) {
    part_state const *ps = &pl->parts[0];
    switch (s->kind) {
    case STEP_PLAIN:
        return lsk_pull_gather_blk(pl->dop, pl->dbs, pl->cplx, r0, r1, ps->d_reps, ps->d_norms, pb, b->K, b->x, b->xr, b->xc, b->y, b->yr, b->yc,
                                   stream);
    case STEP_CHEB:
        return lsk_pull_gather_cheb(pl->dop, pl->dbs, pl->cplx, r0, r1, ps->d_reps, ps->d_norms, pb, b->K, b->x, b->xr, b->xc, b->y, b->yr, b->yc,
                                    s->alpha, s->beta, s->gamma, s->d_dots, stream);
    default:
        return lsk_pull_gather_evolve(pl->dop, pl->dbs, pl->cplx, r0, r1, ps->d_reps, ps->d_norms, pb, b->K, b->x, b->xr, b->xc, b->y, b->yr, b->yc,
                                      s->alpha, s->beta, s->gamma, s->z, s->z_row, s->z_col, s->z_cplx, s->c_re, s->c_im, s->d_dots, stream);
    }
}
/* column k of the column loop, after ls_amd_matvec left H X_k in col_w: STEP_PLAIN has Y_k there already (copied out where the rows
 * of Y are strided); the fused steps finish Y_k (and Z_k) from it with the epilogue kernel, k_axpby_dots / k_axpby_acc */
static int step_column_tail(ls_amd_plan *pl, int k, void const *col_w, block_xy const *b, block_step const *s, void *stream) {
    int64_t const n = pl->parts[0].count;
    size_t const w = pl->cplx ? 16 : 8;
    void const *xk = b->x + (size_t)k * (size_t)b->xc * w;
    void *yk = b->y + (size_t)k * (size_t)b->yc * w;
    double *const xx = s->d_dots ? s->d_dots + k : NULL, *const xy = s->d_dots ? s->d_dots + b->K + k : NULL;
    switch (s->kind) {
    case STEP_PLAIN:
        return b->yr != 1 ? lsk_copy_strided(n, (int)w, col_w, 1, yk, b->yr, stream) : 0;
    case STEP_CHEB:
        return lsk_axpby_dots(pl->cplx, n, 1, col_w, 1, 0, xk, b->xr, 0, yk, b->yr, 0, s->alpha, s->beta, s->gamma, xx, xy, stream);
    default:
        return lsk_axpby_acc(pl->cplx, n, 1, col_w, 1, 0, xk, b->xr, 0, yk, b->yr, 0, s->alpha, s->beta, s->gamma,
                             s->z + (size_t)k * (size_t)s->z_col * (s->z_cplx ? 16 : 8), s->z_row, 0, s->z_cplx, s->c_re, s->c_im, xx, xy, stream);
    }
}

/* the path of every plan without a block kernel (and of K = 1 under `auto`): K columns, one ls_amd_matvec each (it counts and
 * times itself).  A strided column of X is gathered into one of the plan's two scratch columns; H X_k goes to the other, cleared
 * first (the single-vector paths accumulate when the operator has no diagonal) -- or, in STEP_PLAIN with contiguous rows of Y,
 * straight into Y_k, and then the scratch is only allocated where a row stride asks for it */
static int block_step_columns(ls_amd_plan *pl, block_xy const *b, block_step const *s, void *stream) {
    int64_t const n = pl->parts[0].count;
    size_t const w = pl->cplx ? 16 : 8;
    int const in_place = s->kind == STEP_PLAIN && b->yr == 1;
    if ((s->kind != STEP_PLAIN || b->xr != 1 || b->yr != 1) && !pl->d_blk_cols && lsk_malloc(&pl->d_blk_cols, 2 * w * (size_t)n) != 0)
        return dev_error();
    char *const col_x = (char *)pl->d_blk_cols, *const col_w = col_x ? col_x + w * (size_t)n : NULL;
    for (int k = 0; k < b->K; ++k) {
        void const *xin = b->x + (size_t)k * (size_t)b->xc * w;
        void *wout = in_place ? b->y + (size_t)k * (size_t)b->yc * w : col_w;
        if (b->xr != 1) {
            DEV(lsk_copy_strided(n, (int)w, xin, b->xr, col_x, 1, stream));
            xin = col_x;
        }
        DEV(lsk_memset_async(wout, 0, w * (size_t)n, stream));
        if (ls_amd_matvec(pl, &xin, &wout, stream) != 0) return -1;
        DEV(step_column_tail(pl, k, col_w, b, s, stream));
    }
    return 0;
}

/* one step on the path block_path() chose, after the entry point's own checks */
static int block_step_run(ls_amd_plan *pl, int path, block_xy const *b, block_step const *s, void *stream) {
    if (path == BLK_COLUMNS) return block_step_columns(pl, b, s, stream);
    part_state *ps = &pl->parts[0];
    int64_t const n = ps->count;
    ls_amd_internal_count_matvec(pl);
    if (path == BLK_DIRECT) {
        lsk_tilemap tm;
        if (block_tilemap(pl, &tm) != 0) return -1;
        int const st = stage_begin(pl, ST_ROWS, stream);
        int const slot = timing_begin(pl, stream);
        DEV(step_direct(pl, tm, b, s, stream));
        timing_end(pl, slot, stream);
        stage_end(pl, st, stream);
        return 0;
    }
    /* projected, indexed: rows a valid slot cache covers gather from it; the others are resolved chunk by chunk into the block's
     * own buffer (never the plan's split / cache buffer) and gathered K columns at a time */
    lsk_pullidx ix;
    memset(&ix, 0, sizeof(ix));
    ix.tab = pl->gtab->tab;
    int64_t const cached = pl->slot_cache && pl->slot_cache_valid ? pl->split_rows : 0;
    int const slot = timing_begin(pl, stream);
    if (cached > 0) {
        int const st = stage_begin(pl, ST_ROWS, stream);
        DEV(step_gather(pl, 0, cached, pl->pbuf, b, s, stream));
        stage_end(pl, st, stream);
    }
    if (cached < n && block_pbuf(pl) != 0) return -1;
    for (int64_t r0 = cached; r0 < n; r0 += pl->blk_rows) {
        int64_t const r1 = r0 + pl->blk_rows < n ? r0 + pl->blk_rows : n;
        lsk_pullbuf pb = pl->blk_pbuf;
        pb.row0 = r0;
        int st = stage_begin(pl, ST_GENERATE, stream);
        DEV(lsk_tile_pull_resolve(pl->dop, pl->dbs, r0, r1, ps->d_reps, ps->d_norms, ix, ps->d_reps, ps->count, pl->pull_halo, pb, pl->d_err,
                                  stream));
        stage_end(pl, st, stream);
        st = stage_begin(pl, ST_ROWS, stream);
        DEV(step_gather(pl, r0, r1, pb, b, s, stream));
        stage_end(pl, st, stream);
    }
    timing_end(pl, slot, stream);
    return 0;
}

int ls_amd_matvec_block(ls_amd_plan *pl, int K, void const *d_x, int64_t x_row, int64_t x_col, void *d_y, int64_t y_row, int64_t y_col,
                        void *stream) {
    char const *const who = "ls_amd_matvec_block";
    int64_t const n = block_step_rows(who, pl, K, NULL, stream);
    if (n <= 0) return (int)n;
    if (!d_x || !d_y) return set_error("%s: X or Y is NULL", who);
    if (K == 1) { x_col = 0; y_col = 0; }
    block_xy const b = { K, (char const *)d_x, x_row, x_col, (char *)d_y, y_row, y_col };
    if (block_xy_check(who, pl, &b) != 0) return -1;
    if (ls_amd_internal_check_y(pl, d_y) != 0) return -1;
    block_step const s = { .kind = STEP_PLAIN };
    return block_step_run(pl, block_path(pl, K), &b, &s, stream);
}

/* ============================================================================================ */
/* Chebyshev step (ls_amd_matvec_block_axpby): Y <- alpha H X + beta X + gamma Y and two dots    */
/* ============================================================================================ */
static char const *const g_axpby_names[3] = { "epilogue", "k_direct_cheb", "k_pull_gather_cheb" };
char const *ls_amd_plan_axpby_kernel_name(ls_amd_plan const *pl, int K) {
    if (!pl) { set_error("ls_amd_plan_axpby_kernel_name: plan is NULL"); return NULL; }
    if (K < 1 || K > 64) { set_error("ls_amd_plan_axpby_kernel_name: K = %d is outside [1, 64]", K); return NULL; }
    return g_axpby_names[block_path(pl, K)];
}

int ls_amd_block_axpby_dots(int cplx, int64_t n, int K, void const *d_w, int64_t w_row, int64_t w_col, void const *d_x, int64_t x_row,
                            int64_t x_col, void *d_y, int64_t y_row, int64_t y_col, double alpha, double beta, double gamma,
                            double *d_dots, void *stream) {
    char const *const who = "ls_amd_block_axpby_dots";
    if (K < 1 || K > 64) return set_error("%s: K = %d is outside [1, 64]", who, K);
    if (n < 0) return set_error("%s: n = %lld is negative", who, (long long)n);
    if (n == 0) {
        if (d_dots) DEV(lsk_memset_async(d_dots, 0, sizeof(double) * 2 * (size_t)K, stream));
        return 0;
    }
    if (!d_w || !d_x || !d_y) return set_error("%s: W, X or Y is NULL", who);
    if (K == 1) { w_col = 0; x_col = 0; y_col = 0; }
    if (block_strides(who, n, K, w_row, w_col, "W") != 0 || block_strides(who, n, K, x_row, x_col, "X") != 0 ||
        block_strides(who, n, K, y_row, y_col, "Y") != 0)
        return -1;
    size_t const w = cplx ? 16 : 8;
    if (block_overlap(w, n, d_x, x_row, x_col, w, n, d_y, y_row, y_col, K)) return set_error("%s: X and Y overlap", who);
    if (block_overlap(w, n, d_w, w_row, w_col, w, n, d_y, y_row, y_col, K)) return set_error("%s: W and Y overlap", who);
    if (d_dots) DEV(lsk_memset_async(d_dots, 0, sizeof(double) * 2 * (size_t)K, stream));
    DEV(lsk_axpby_dots(cplx != 0, n, K, d_w, w_row, w_col, d_x, x_row, x_col, d_y, y_row, y_col, alpha, beta, gamma, d_dots,
                       d_dots ? d_dots + K : NULL, stream));
    return 0;
}

int ls_amd_matvec_block_axpby(ls_amd_plan *pl, int K, void const *d_x, int64_t x_row, int64_t x_col, void *d_y, int64_t y_row,
                              int64_t y_col, double alpha, double beta, double gamma, double *d_dots, void *stream) {
    char const *const who = "ls_amd_matvec_block_axpby";
    int64_t const n = block_step_rows(who, pl, K, d_dots, stream);
    if (n <= 0) return (int)n;
    if (!d_x || !d_y) return set_error("%s: X or Y is NULL", who);
    if (K == 1) { x_col = 0; y_col = 0; }
    block_xy const b = { K, (char const *)d_x, x_row, x_col, (char *)d_y, y_row, y_col };
    if (block_xy_check(who, pl, &b) != 0) return -1;
    if (ls_amd_internal_check_y(pl, d_y) != 0) return -1;
    if (d_dots) DEV(lsk_memset_async(d_dots, 0, sizeof(double) * 2 * (size_t)K, stream));
    block_step const s = { .kind = STEP_CHEB, .alpha = alpha, .beta = beta, .gamma = gamma, .d_dots = d_dots };
    return block_step_run(pl, block_path(pl, K), &b, &s, stream);
}

/* ============================================================================================ */
/* Gram matrices of blocks (k_gram.hip): ls_amd_block_gram, and the Chebyshev step followed by   */
/* X^+ X and X^+ Y (ls_amd_matvec_block_axpby_gram) -- the matrix-valued moments of kpm.py       */
/* ============================================================================================ */
/* a block the MFMA form reads as it lies: column stride 1 (or one column) and a row stride equal to its width */
static int gram_interleaved(int K, int64_t row, int64_t col) { return row == K && (K == 1 || col == 1); }
/* LS_AMD_GRAM=auto|mfma|valu, read at every call: `valu` takes k_block_gram everywhere; `mfma` forces k_block_gram_mfma where it
 * applies (every block interleaved); anything else is the rule the measurements decided ("Matrix moments"):
 * the MFMA form from 8 columns on -- below that most of its 16 operand columns are padding and k_block_gram is faster */
enum { GRAM_MFMA_MIN_COLS = 8 };
static int gram_use_mfma(int all_interleaved, int Ka, int Kb) {
    char const *e = getenv("LS_AMD_GRAM");
    if (e && strcmp(e, "valu") == 0) return 0;
    if (e && strcmp(e, "mfma") == 0) return all_interleaved;
    return all_interleaved && Ka >= GRAM_MFMA_MIN_COLS && Kb >= GRAM_MFMA_MIN_COLS;
}
int64_t ls_amd_block_gram_work_bytes(int64_t n, int Ka, int Kb, int cplx) {
    if (n < 0 || Ka < 1 || Ka > 64 || Kb < 1 || Kb > 64) {
        set_error("ls_amd_block_gram_work_bytes: n = %lld, Ka = %d, Kb = %d: need n >= 0 and 1 <= Ka, Kb <= 64", (long long)n, Ka, Kb);
        return -1;
    }
    /* (room for two ket blocks, whatever the call has) */
    return (int64_t)lsk_block_gram_blocks(n, Ka, Kb, cplx != 0) * 2 * Ka * Kb * (cplx ? 16 : 8);
}
char const *ls_amd_block_gram_kernel_name(int cplx, int Ka, int64_t a_row, int64_t a_col, int Kb, int64_t b_row, int64_t b_col) {
    if (Ka < 1 || Ka > 64 || Kb < 1 || Kb > 64) {
        set_error("ls_amd_block_gram_kernel_name: Ka = %d, Kb = %d: each is outside [1, 64]", Ka, Kb);
        return NULL;
    }
    return lsk_block_gram_kernel_name(gram_use_mfma(gram_interleaved(Ka, a_row, a_col) && gram_interleaved(Kb, b_row, b_col), Ka, Kb));
}
/* [p, p + bytes) against an n x K block of elements of w bytes */
static int range_overlaps_block(void const *p, size_t bytes, size_t w, int64_t n, void const *b, int64_t br, int64_t bc, int K) {
    uintptr_t const p0 = (uintptr_t)p, p1 = p0 + bytes;
    uintptr_t const b0 = (uintptr_t)b, b1 = b0 + w * (size_t)((n - 1) * br + (int64_t)(K - 1) * bc + 1);
    return p0 < b1 && b0 < p1;
}
int ls_amd_block_gram(int cplx, int64_t n, int Ka, void const *d_a, int64_t a_row, int64_t a_col, int Kb, void const *d_b, int64_t b_row,
                      int64_t b_col, void *d_work, int64_t work_bytes, void *d_out, void *stream) {
    char const *const who = "ls_amd_block_gram";
    if (Ka < 1 || Ka > 64) return set_error("%s: Ka = %d is outside [1, 64]", who, Ka);
    if (Kb < 1 || Kb > 64) return set_error("%s: Kb = %d is outside [1, 64]", who, Kb);
    if (n < 0) return set_error("%s: n = %lld is negative", who, (long long)n);
    if (!d_out) return set_error("%s: the output is NULL", who);
    size_t const w = cplx ? 16 : 8;
    if (n == 0) {
        DEV(lsk_memset_async(d_out, 0, w * (size_t)Ka * (size_t)Kb, stream));
        return 0;
    }
    if (!d_a || !d_b) return set_error("%s: A or B is NULL", who);
    if (!d_work) return set_error("%s: the work buffer is NULL", who);
    if (Ka == 1) a_col = 0;
    if (Kb == 1) b_col = 0;
    if (block_strides(who, n, Ka, a_row, a_col, "A") != 0 || block_strides(who, n, Kb, b_row, b_col, "B") != 0) return -1;
    int64_t const need = ls_amd_block_gram_work_bytes(n, Ka, Kb, cplx) / 2; /* (one ket block) */
    if (work_bytes < need) return set_error("%s: work_bytes = %lld, this call needs %lld (ls_amd_block_gram_work_bytes)", who, (long long)work_bytes, (long long)need);
    if (range_overlaps_block(d_out, w * (size_t)Ka * (size_t)Kb, w, n, d_a, a_row, a_col, Ka) ||
        range_overlaps_block(d_out, w * (size_t)Ka * (size_t)Kb, w, n, d_b, b_row, b_col, Kb))
        return set_error("%s: the output overlaps A or B", who);
    if (range_overlaps_block(d_work, (size_t)need, w, n, d_a, a_row, a_col, Ka) || range_overlaps_block(d_work, (size_t)need, w, n, d_b, b_row, b_col, Kb))
        return set_error("%s: the work buffer overlaps A or B", who);
    int const mfma = gram_use_mfma(gram_interleaved(Ka, a_row, a_col) && gram_interleaved(Kb, b_row, b_col), Ka, Kb);
    DEV(lsk_block_gram(cplx != 0, n, Ka, d_a, a_row, a_col, Kb, 1, d_b, b_row, b_col, NULL, 0, 0, mfma, (double *)d_work, (double *)d_out, stream));
    return 0;
}
int ls_amd_matvec_block_axpby_gram(ls_amd_plan *pl, int K, void const *d_x, int64_t x_row, int64_t x_col, void *d_y, int64_t y_row,
                                   int64_t y_col, double alpha, double beta, double gamma, void *d_gram, void *stream) {
    char const *const who = "ls_amd_matvec_block_axpby_gram";
    int64_t const n = block_step_rows(who, pl, K, NULL, stream);
    if (n < 0) return -1;
    if (!d_gram) return set_error("%s: the Gram output is NULL", who);
    size_t const w = pl->cplx ? 16 : 8, gram_bytes = 2 * w * (size_t)K * (size_t)K;
    if (n == 0) {
        DEV(lsk_memset_async(d_gram, 0, gram_bytes, stream));
        return 0;
    }
    if (!d_x || !d_y) return set_error("%s: X or Y is NULL", who);
    if (K == 1) { x_col = 0; y_col = 0; }
    block_xy const b = { K, (char const *)d_x, x_row, x_col, (char *)d_y, y_row, y_col };
    if (block_xy_check(who, pl, &b) != 0) return -1;
    if (range_overlaps_block(d_gram, gram_bytes, w, n, d_x, x_row, x_col, K) || range_overlaps_block(d_gram, gram_bytes, w, n, d_y, y_row, y_col, K))
        return set_error("%s: the Gram output overlaps X or Y", who);
    size_t const need = (size_t)ls_amd_block_gram_work_bytes(n, K, K, pl->cplx);
    if (pl->gram_work_bytes < need) {
        if (pl->d_gram_work) lsk_free(pl->d_gram_work);
        pl->d_gram_work = NULL;
        pl->gram_work_bytes = 0;
        if (lsk_malloc(&pl->d_gram_work, need) != 0) return dev_error();
        pl->gram_work_bytes = need;
    }
    if (ls_amd_matvec_block_axpby(pl, K, d_x, x_row, x_col, d_y, y_row, y_col, alpha, beta, gamma, NULL, stream) != 0) return -1;
    int const mfma = gram_use_mfma(gram_interleaved(K, x_row, x_col) && gram_interleaved(K, y_row, y_col), K, K);
    DEV(lsk_block_gram(pl->cplx, n, K, d_x, x_row, x_col, K, 2, d_x, x_row, x_col, d_y, y_row, y_col, mfma, (double *)pl->d_gram_work,
                       (double *)d_gram, stream));
    return 0;
}

/* ============================================================================================ */
/* accumulate step of Chebyshev time evolution (ls_amd_matvec_block_axpby_acc): the step above   */
/* and Z += c Y with the new Y (k_evolve.hip)                                                    */
/* ============================================================================================ */
static char const *const g_acc_names[3] = { "epilogue", "k_direct_evolve", "k_pull_gather_evolve" };
static char const *const g_acc_split_names[3] = { "epilogue", "k_direct_cheb+k_axpby_acc", "k_pull_gather_cheb+k_axpby_acc" };
/* LS_AMD_ACC=fused|split, read at every call: on the two row-kernel paths, whether Z is accumulated inside the row kernel
 * (k_direct_evolve / k_pull_gather_evolve) or by one streaming pass of k_axpby_acc behind the Chebyshev kernel of that path.
 * Anything else: the default of DESIGN.md section 5, "Accumulate step" (ACC_SPLIT_DEFAULT per path, decided by measurement). */
static int const ACC_SPLIT_DEFAULT[3] = { 0, 1, 1 };
static int acc_split(int path) {
    if (path == BLK_COLUMNS) return 0;
    char const *e = getenv("LS_AMD_ACC");
    if (e && strcmp(e, "fused") == 0) return 0;
    if (e && strcmp(e, "split") == 0) return 1;
    return ACC_SPLIT_DEFAULT[path];
}
char const *ls_amd_plan_acc_kernel_name(ls_amd_plan const *pl, int K) {
    if (!pl) { set_error("ls_amd_plan_acc_kernel_name: plan is NULL"); return NULL; }
    if (K < 1 || K > 64) { set_error("ls_amd_plan_acc_kernel_name: K = %d is outside [1, 64]", K); return NULL; }
    int const path = block_path(pl, K);
    return acc_split(path) ? g_acc_split_names[path] : g_acc_names[path];
}

/* what both entry points ask of Z and c (after K and n were checked and the column strides of K = 1 cleared) */
static int acc_check_z(char const *who, int cplx, int z_cplx, int64_t n, int K, void const *d_z, int64_t z_row, int64_t z_col, double c_im) {
    if (!d_z) return set_error("%s: Z is NULL", who);
    if (cplx && !z_cplx) return set_error("%s: z_cplx = 0 with c128 vectors: Z must be c128 (an f64 accumulator cannot hold c Y)", who);
    if (!z_cplx && c_im != 0.0) return set_error("%s: z_cplx = 0 with c_im = %g: an f64 Z needs a real c", who, c_im);
    return block_strides(who, n, K, z_row, z_col, "Z");
}

int ls_amd_block_axpby_acc(int cplx, int z_cplx, int64_t n, int K, void const *d_w, int64_t w_row, int64_t w_col, void const *d_x,
                           int64_t x_row, int64_t x_col, void *d_y, int64_t y_row, int64_t y_col, void *d_z, int64_t z_row, int64_t z_col,
                           double alpha, double beta, double gamma, double c_re, double c_im, double *d_dots, void *stream) {
    char const *const who = "ls_amd_block_axpby_acc";
    if (K < 1 || K > 64) return set_error("%s: K = %d is outside [1, 64]", who, K);
    if (n < 0) return set_error("%s: n = %lld is negative", who, (long long)n);
    if (n == 0) {
        if (d_dots) DEV(lsk_memset_async(d_dots, 0, sizeof(double) * 2 * (size_t)K, stream));
        return 0;
    }
    if (!d_w || !d_x || !d_y) return set_error("%s: W, X or Y is NULL", who);
    if (K == 1) { w_col = 0; x_col = 0; y_col = 0; z_col = 0; }
    if (acc_check_z(who, cplx != 0, z_cplx != 0, n, K, d_z, z_row, z_col, c_im) != 0) return -1;
    if (block_strides(who, n, K, w_row, w_col, "W") != 0 || block_strides(who, n, K, x_row, x_col, "X") != 0 ||
        block_strides(who, n, K, y_row, y_col, "Y") != 0)
        return -1;
    size_t const w = cplx ? 16 : 8, wz = z_cplx ? 16 : 8;
    if (block_overlap(w, n, d_x, x_row, x_col, w, n, d_y, y_row, y_col, K)) return set_error("%s: X and Y overlap", who);
    if (block_overlap(w, n, d_w, w_row, w_col, w, n, d_y, y_row, y_col, K)) return set_error("%s: W and Y overlap", who);
    if (block_overlap(wz, n, d_z, z_row, z_col, w, n, d_y, y_row, y_col, K)) return set_error("%s: Z and Y overlap", who);
    if (block_overlap(wz, n, d_z, z_row, z_col, w, n, d_x, x_row, x_col, K)) return set_error("%s: Z and X overlap", who);
    if (block_overlap(wz, n, d_z, z_row, z_col, w, n, d_w, w_row, w_col, K)) return set_error("%s: Z and W overlap", who);
    if (d_dots) DEV(lsk_memset_async(d_dots, 0, sizeof(double) * 2 * (size_t)K, stream));
    DEV(lsk_axpby_acc(cplx != 0, n, K, d_w, w_row, w_col, d_x, x_row, x_col, d_y, y_row, y_col, alpha, beta, gamma, d_z, z_row, z_col,
                      z_cplx != 0, c_re, c_im, d_dots, d_dots ? d_dots + K : NULL, stream));
    return 0;
}

int ls_amd_matvec_block_axpby_acc(ls_amd_plan *pl, int K, void const *d_x, int64_t x_row, int64_t x_col, void *d_y, int64_t y_row,
                                  int64_t y_col, double alpha, double beta, double gamma, void *d_z, int64_t z_row, int64_t z_col,
                                  int z_cplx, double c_re, double c_im, double *d_dots, void *stream) {
    char const *const who = "ls_amd_matvec_block_axpby_acc";
    int64_t const n = block_step_rows(who, pl, K, d_dots, stream);
    if (n <= 0) return (int)n;
    if (!d_x || !d_y) return set_error("%s: X or Y is NULL", who);
    if (K == 1) { x_col = 0; y_col = 0; z_col = 0; }
    z_cplx = z_cplx != 0;
    if (acc_check_z(who, pl->cplx, z_cplx, n, K, d_z, z_row, z_col, c_im) != 0) return -1;
    block_xy const b = { K, (char const *)d_x, x_row, x_col, (char *)d_y, y_row, y_col };
    if (block_xy_check(who, pl, &b) != 0) return -1;
    size_t const w = pl->cplx ? 16 : 8, wz = z_cplx ? 16 : 8;
    if (block_overlap(wz, n, d_z, z_row, z_col, w, n, d_y, y_row, y_col, K)) return set_error("%s: Z and Y overlap", who);
    if (block_overlap(wz, n, d_z, z_row, z_col, w, n, d_x, x_row, x_col, K)) return set_error("%s: Z and X overlap", who);
    if (ls_amd_internal_check_y(pl, d_y) != 0) return -1;
    if (d_dots) DEV(lsk_memset_async(d_dots, 0, sizeof(double) * 2 * (size_t)K, stream));
    int const path = block_path(pl, K);
    if (acc_split(path)) {
        /* the Chebyshev kernel of the path, then Z += c Y in one streaming pass over the finished Y */
        if (ls_amd_matvec_block_axpby(pl, K, d_x, x_row, x_col, d_y, y_row, y_col, alpha, beta, gamma, d_dots, stream) != 0) return -1;
        DEV(lsk_axpby_acc(pl->cplx, n, K, NULL, 0, 0, NULL, 0, 0, d_y, y_row, y_col, 0.0, 0.0, 1.0, d_z, z_row, z_col, z_cplx, c_re, c_im, NULL,
                          NULL, stream));
        return 0;
    }
    block_step const s = { .kind = STEP_ACC, .alpha = alpha, .beta = beta, .gamma = gamma, .d_dots = d_dots, .z = (char *)d_z, .z_row = z_row,
                           .z_col = z_col, .z_cplx = z_cplx, .c_re = c_re, .c_im = c_im };
    return block_step_run(pl, path, &b, &s, stream);
}

/* ============================================================================================ */
/* a whole Chebyshev series on a block (ls_amd_matvec_block_series): the accumulate step above,  */
/* once per order, between two work blocks; no kernel of its own                                 */
/* ============================================================================================ */
#define SERIES_GUARD_EVERY 64   /* orders between two read-backs of the dots (kpm.GUARD_EVERY) */
#define SERIES_GUARD_SLACK 1e-6 /* kpm.GUARD_SLACK */
char const *ls_amd_plan_series_kernel_name(ls_amd_plan const *pl, int K) {
    if (!pl) { set_error("ls_amd_plan_series_kernel_name: plan is NULL"); return NULL; }
    if (K < 1 || K > 64) { set_error("ls_amd_plan_series_kernel_name: K = %d is outside [1, 64]", K); return NULL; }
    return g_axpby_names[block_path(pl, K)];
}

/* Z <- 0 for any strides block_strides lets through: one memset where the block is dense, else column by column (in slabs of rows)
 * out of `zeros`, zero_bytes of cleared device memory */
static int series_clear(char *z, size_t wz, int64_t n, int K, int64_t zr, int64_t zc, void const *zeros, size_t zero_bytes, void *stream) {
    if ((n - 1) * zr + (int64_t)(K - 1) * zc + 1 == n * (int64_t)K) {
        DEV(lsk_memset_async(z, 0, wz * (size_t)n * (size_t)K, stream));
        return 0;
    }
    int64_t const slab = (int64_t)(zero_bytes / wz);
    if (slab < 1) return set_error("ls_amd_matvec_block_series: no room to clear Z from");
    for (int k = 0; k < K; ++k)
        for (int64_t r0 = 0; r0 < n; r0 += slab) {
            int64_t const rows = r0 + slab < n ? slab : n - r0;
            DEV(lsk_copy_strided(rows, (int)wz, zeros, 1, z + ((size_t)k * (size_t)zc + (size_t)r0 * (size_t)zr) * wz, zr, stream));
        }
    return 0;
}

int ls_amd_matvec_block_series(ls_amd_plan *pl, int K, int N, double const *coeffs, double lo, double hi, void const *d_x, int64_t x_row,
                               int64_t x_col, void *d_z, int64_t z_row, int64_t z_col, int z_cplx, void *d_work, void *stream) {
    char const *const who = "ls_amd_matvec_block_series";
    int64_t const n = block_step_rows(who, pl, K, NULL, stream);
    if (n < 0) return -1;
    if (N < 0) return set_error("%s: N = %d is negative", who, N);
    if (!coeffs) return set_error("%s: coeffs is NULL", who);
    if (!(isfinite(lo) && isfinite(hi) && lo < hi)) return set_error("%s: bounds (%.17g, %.17g): need finite lo < hi", who, lo, hi);
    z_cplx = z_cplx != 0;
    for (int i = 0; i <= N; ++i) {
        if (!(isfinite(coeffs[2 * i]) && isfinite(coeffs[2 * i + 1])))
            return set_error("%s: coeffs[%d] = (%g, %g) is not finite", who, i, coeffs[2 * i], coeffs[2 * i + 1]);
        if (!z_cplx && coeffs[2 * i + 1] != 0.0)
            return set_error("%s: z_cplx = 0 with Im coeffs[%d] = %g: an f64 Z needs real coefficients", who, i, coeffs[2 * i + 1]);
    }
    if (n == 0) return 0;
    if (!d_x) return set_error("%s: X is NULL", who);
    if (K == 1) { x_col = 0; z_col = 0; }
    if (acc_check_z(who, pl->cplx, z_cplx, n, K, d_z, z_row, z_col, 0.0) != 0) return -1;
    if (block_strides(who, n, K, x_row, x_col, "X") != 0) return -1;
    size_t const w = pl->cplx ? 16 : 8, wz = z_cplx ? 16 : 8;
    size_t const block = w * (size_t)n * (size_t)K;
    if (block_overlap(wz, n, d_z, z_row, z_col, w, n, d_x, x_row, x_col, K)) return set_error("%s: Z and X overlap", who);
    char *work = (char *)d_work;
    if (!work) {
        if (pl->d_series_work && pl->series_cols < K) {
            DEV(lsk_sync(stream));
            lsk_free(pl->d_series_work);
            pl->d_series_work = NULL;
            pl->series_cols = 0;
        }
        if (!pl->d_series_work) {
            if (lsk_malloc(&pl->d_series_work, 2 * block) != 0) return dev_error();
            pl->series_cols = K;
        }
        work = (char *)pl->d_series_work;
    }
    /* (the work buffer: its two interleaved blocks as one of 2 n rows) */
    if (block_overlap(w, 2 * n, work, K, 1, w, n, d_x, x_row, x_col, K)) return set_error("%s: work and X overlap", who);
    if (block_overlap(w, 2 * n, work, K, 1, wz, n, d_z, z_row, z_col, K)) return set_error("%s: work and Z overlap", who);
    if (!pl->d_series_dots && lsk_malloc((void **)&pl->d_series_dots, sizeof(double) * SERIES_GUARD_EVERY * 128) != 0) return dev_error();
    double const a = 0.5 * (hi - lo), b = 0.5 * (hi + lo);
    /* the two work blocks in the interleaved layout (row stride K, column stride 1): cur = v_n, oth = v_{n-1}, overwritten by v_{n+1} */
    char *cur = work, *oth = work + block;
    /* Z <- c_0 X: Z cleared (oth, cleared, is where a padded Z copies its zeros from), then the accumulate alone over X */
    DEV(lsk_memset_async(oth, 0, block, stream));
    if (series_clear((char *)d_z, wz, n, K, z_row, z_col, oth, block, stream) != 0) return -1;
    DEV(lsk_axpby_acc(pl->cplx, n, K, NULL, 0, 0, NULL, 0, 0, (void *)(uintptr_t)d_x, x_row, x_col, 0.0, 0.0, 1.0, d_z, z_row, z_col, z_cplx,
                      coeffs[0], coeffs[1], NULL, NULL, stream));
    if (N == 0) return 0;
    for (int k = 0; k < K; ++k)
        DEV(lsk_copy_strided(n, (int)w, (char const *)d_x + (size_t)k * (size_t)x_col * w, x_row, cur + (size_t)k * w, K, stream));
    double mu0[64], host[SERIES_GUARD_EVERY * 128];
    for (int s = 0, checked = 0; s < N; ++s) {
        double *const dots = pl->d_series_dots + (size_t)(s - checked) * 2 * (size_t)K;
        double const al = (s == 0 ? 1.0 : 2.0) / a, be = (s == 0 ? -1.0 : -2.0) * b / a, ga = s == 0 ? 0.0 : -1.0;
        if (ls_amd_matvec_block_axpby_acc(pl, K, cur, K, 1, oth, K, 1, al, be, ga, d_z, z_row, z_col, z_cplx, coeffs[2 * (s + 1)],
                                          coeffs[2 * (s + 1) + 1], dots, stream) != 0)
            return -1;
        char *const t = cur; cur = oth; oth = t;
        if (s + 1 - checked == SERIES_GUARD_EVERY || s + 1 == N) {
            int const rows = s + 1 - checked;
            DEV(lsk_sync(stream));
            DEV(lsk_d2h(host, pl->d_series_dots, sizeof(double) * (size_t)rows * 2 * (size_t)K));
            if (checked == 0) memcpy(mu0, host, sizeof(double) * (size_t)K);
            for (int r = 0; r < rows; ++r)
                for (int k = 0; k < K; ++k) {
                    double const vv = host[(size_t)r * 2 * (size_t)K + k];
                    if (!(vv <= (1.0 + SERIES_GUARD_SLACK) * mu0[k]))
                        return set_error("%s: the Chebyshev recurrence grows at order %d (<v_n|v_n> / <v_0|v_0> = %.6g in column %d): the "
                                         "spectrum is not inside the bounds (%.17g, %.17g)", who, checked + r, vv / mu0[k], k, lo, hi);
                }
            checked = s + 1;
        }
    }
    return 0;
}

int ls_amd_plan_check(ls_amd_plan *pl, void *stream) {
    int flag = 0, zero = 0;
    DEV(lsk_sync(stream));
    DEV(lsk_d2h(&flag, pl->d_err, sizeof(int)));
    if (flag || pl->leaves_basis) {
        DEV(lsk_h2d(pl->d_err, &zero, sizeof(int)));
        return set_error("invalid index: the operator generated a state outside the basis "
                         "(it does not respect the basis symmetries)"); /* DMV:115-118 */
    }
    return 0;
}

/* ============================================================================================ */
/* enumeration and layout converters                                                            */
/* ============================================================================================ */
static int64_t candidate_count(ls_hs_basis const *b) {
    int const Leff = NBITS(b) - (b->spin_inversion != 0 ? 1 : 0);
    int const h = BEXT(b)->hamming_weight;
    if (h >= 0) return (int64_t)binom(Leff, h);
    if (Leff >= 62) return -1;
    return (int64_t)1 << Leff;
}

int ls_amd_enumerate_states(ls_hs_basis const *basis, int num_locales, uint64_t **d_states, uint8_t **d_masks,
                            int64_t *count, void *stream) {
    lsk_basis dbs;
    uint64_t const *d_binom;
    if (basis_device(basis, &dbs) != 0 || device_binom(&d_binom) != 0) return -1;
    struct ls_amd_basis_ext const *e = BEXT(basis);
    if (e->product && e->fermi) { /* projected: the product candidates through the signed representative test */
        DEV(lsk_fermi_enumerate_product(dbs, e->prod_up, e->prod_dn, d_binom, d_states, count, stream));
    } else if (e->product) {
        DEV(lsk_enumerate_product(basis->number_sites, e->prod_up, e->prod_dn, d_binom, d_states, count, stream));
    } else {
        int64_t ncand = candidate_count(basis);
        if (ncand < 0) return set_error("basis too large to enumerate");
        DEV(lsk_enumerate(dbs, d_binom, ncand, d_states, count, stream));
    }
    if (d_masks) {
        void *p;
        DEV(lsk_malloc(&p, (size_t)(*count > 0 ? *count : 1)));
        *d_masks = (uint8_t *)p;
        DEV(lsk_masks(*count, *d_states, num_locales < 1 ? 1 : num_locales, *d_masks, stream));
        DEV(lsk_sync(stream));
    }
    return 0;
}
int ls_amd_gather(int64_t n, void const *d_perm, int perm_is_64, int elt_size, void const *d_src, void *d_out, void *stream) {
    DEV(lsk_gather_perm(n, d_perm, perm_is_64, elt_size, d_src, d_out, stream));
    return 0;
}
int ls_amd_mask_counts(int64_t n, uint8_t const *d_masks, int num_locales, int64_t *counts, void *stream) {
    DEV(lsk_mask_counts(n, d_masks, num_locales, counts, stream));
    return 0;
}
int ls_amd_block_to_hashed(int64_t n, uint8_t const *d_masks, int num_locales, int elt_size, void const *d_src,
                           void *const *d_dest, void *stream) {
    DEV(lsk_block_to_hashed(n, d_masks, num_locales, elt_size, d_src, d_dest, stream));
    return 0;
}
int ls_amd_hashed_to_block(int64_t n, uint8_t const *d_masks, int num_locales, int elt_size,
                           void const *const *d_src, void *d_dest, void *stream) {
    DEV(lsk_hashed_to_block(n, d_masks, num_locales, elt_size, d_src, d_dest, stream));
    return 0;
}

/* ============================================================================================ */
/* ls_chpl_* exports (host pointers; stage through HBM)                                          */
/* ============================================================================================ */
void ls_chpl_enumerate_representatives(ls_hs_basis *basisPtr, uint64_t lower, uint64_t upper,
                                       chpl_external_array *dest) {
    (void)lower; (void)upper; /* ignored exactly as in the reference (StatesEnumeration.chpl:596) */
    uint64_t *d_states = NULL;
    int64_t count = 0;
    if (ls_amd_enumerate_states(basisPtr, 1, &d_states, NULL, &count, NULL) != 0) {
        halt_with("ls_chpl_enumerate_representatives: %s", g_last_error);
        return;
    }
    uint64_t *h = (uint64_t *)malloc(8 * (size_t)(count > 0 ? count : 1));
    if (lsk_d2h(h, d_states, 8 * (size_t)count) != 0) { free(h); lsk_free(d_states); halt_with("%s", lsk_last_error()); return; }
    lsk_free(d_states);
    dest->elts = h;
    dest->num_elts = (uint64_t)count;
    dest->freer = (void *)free;
}

static int ensure_device_reps(ls_hs_basis *b) {
    struct ls_amd_basis_ext *e = BEXT(b);
    if (!b->representatives.elts) return set_error("basis is not built"); /* ForeignTypes.chpl:113-114 */
    if (e->d_reps_cache && e->d_reps_count == b->representatives.num_elts) return 0;
    basis_drop_device_caches(b);
    void *p;
    DEV(lsk_malloc(&p, 8 * (size_t)b->representatives.num_elts));
    DEV(lsk_h2d(p, b->representatives.elts, 8 * (size_t)b->representatives.num_elts));
    e->d_reps_cache = (uint64_t *)p;
    e->d_reps_count = b->representatives.num_elts;
    return 0;
}

/* ---- the host-pointer boundary (DMV:1095-1110, Diagonalize.chpl:134-162) -------------------------------------------------
 * The reference's callers hand over `double *`.  What that costs here is decided by where the memory lives (stage.cpp):
 *   device memory (hipMalloc, torch)      used in place, zero copies
 *   pinned / registered host memory       one DMA per direction (ls_amd_host_register: once per workspace, PRIMME reuses its)
 *   pageable host memory                  double-buffered pinned bounce chunks, upload and download at the same time
 * x and y have persistent device copies in the cached plan slot (no hipMalloc / hipFree per call); y is uploaded only when the
 * operator has no diagonal terms (else it is assigned, DMV:1062-1063); the columns of a block go through one pipeline.
 * LS_AMD_STAGE=0 restores plain synchronous hipMemcpy (A/B in bench.py's boundary_host_ptr). */
static lsk_stager *g_stager = NULL;
static pthread_mutex_t g_stager_lock = PTHREAD_MUTEX_INITIALIZER;
static struct ls_amd_boundary_stats g_bstats;
void ls_amd_boundary_stats_get(struct ls_amd_boundary_stats *out, int reset) {
    *out = g_bstats;
    if (reset) memset(&g_bstats, 0, sizeof(g_bstats));
}
int ls_amd_host_register(void *p, size_t bytes) {
    if (lsk_host_register(p, bytes) != 0) return set_error("%s", lsk_stage_last_error());
    return 0;
}
int ls_amd_host_unregister(void *p) {
    if (lsk_host_unregister(p) != 0) return set_error("%s", lsk_stage_last_error());
    return 0;
}
int ls_amd_pointer_kind(void const *p) { return lsk_pointer_kind(p); }
/* LS_AMD_STAGE: 1 (default) = pinned bounce pipeline (pageable memory; registered memory: one DMA per direction), 0 = the runtime's own
 * copies one after the other (what a single vector costs either way: 179 vs 182 ms on chain_32; a block of four columns: 716 vs 555 ms) */
static int staging_mode(void) { char const *e = getenv("LS_AMD_STAGE"); return e ? atoi(e) : 1; }
/* (caller holds g_stager_lock -- and keeps it while it uses the stager: a change of the chunk knob destroys and recreates it) */
static lsk_stager *stager_locked(void) {
    char const *e = getenv("LS_AMD_STAGE_CHUNK_KB"), *t = getenv("LS_AMD_STAGE_THREADS");
    size_t const chunk = (e && atoi(e) > 0 ? (size_t)atoi(e) : (size_t)32768) << 10;
    if (g_stager && lsk_stager_chunk(g_stager) != (chunk < 4096 ? 4096 : chunk & ~(size_t)4095)) { lsk_stager_destroy(g_stager); g_stager = NULL; }
    if (!g_stager && lsk_stager_create(&g_stager, chunk, t ? atoi(t) : 0) != 0) { g_stager = NULL; set_error("%s", lsk_stage_last_error()); }
    return g_stager;
}
/* up: host -> device, down: device -> host, at the same time; kinds from lsk_pointer_kind (never LSK_PTR_DEVICE here) */
static int transfer(void *d_up, void const *h_up, size_t up_bytes, int up_kind, void *h_down, void const *d_down, size_t down_bytes,
                    int down_kind) {
    if (!up_bytes && !down_bytes) return 0;
    __atomic_fetch_add(&g_bstats.bytes_h2d, (int64_t)up_bytes, __ATOMIC_RELAXED); /* loop-back ranks call this from several threads */
    __atomic_fetch_add(&g_bstats.bytes_d2h, (int64_t)down_bytes, __ATOMIC_RELAXED);
    int const mode = staging_mode();
    if (mode == 0 && up_kind != LSK_PTR_MANAGED && down_kind != LSK_PTR_MANAGED) {
        if (up_bytes) DEV(lsk_h2d(d_up, h_up, up_bytes));
        if (down_bytes) DEV(lsk_d2h(h_down, d_down, down_bytes));
        return 0;
    }

    pthread_mutex_lock(&g_stager_lock);
    lsk_stager *st = stager_locked();
    int rc = st ? 0 : -1;
    if (st && lsk_stage_run(st, d_up, h_up, up_bytes, up_kind, h_down, d_down, down_bytes, down_kind) != 0) rc = set_error("%s", lsk_stage_last_error());
    pthread_mutex_unlock(&g_stager_lock);
    return rc;
}

/* localMatrixVector on `ncols` host (or device) vectors: column k at x + k ldx, y + k ldy.  The memory kind is looked up ONCE,
 * at x and at y: all columns of a block must live in one kind of memory (one PRIMME workspace does). */
static int host_matvec_block(ls_hs_operator *op, int64_t n, int ncols, double const *x, int64_t ldx, double *y, int64_t ldy,
                             ls_amd_comm *cm) {
    ls_hs_basis *b = op->basis;
    struct ls_amd_basis_ext *e = BEXT(b);
    if (ensure_device_reps(b) != 0) return -1;
    if ((uint64_t)n != e->d_reps_count) return set_error("vector length does not match the number of representatives");
    if (ncols < 1) return 0;
    if (!cm) cm = ls_amd_default_comm();
    if (cm && ls_amd_comm_size(cm) <= 1) cm = NULL;
    /* the cached plan of THIS operator on THIS communicator (least recently used slot is recycled) */
    struct host_plan_slot *sl = NULL, *victim = &e->host_plans[0];
    for (int i = 0; i < HOST_PLAN_SLOTS; ++i) {
        struct host_plan_slot *c = &e->host_plans[i];
        if (c->op == op && c->comm == (void *)cm) { sl = c; break; }
        if (!c->op) { if (victim->op) victim = c; }
        else if (victim->op && c->stamp < victim->stamp) victim = c;
    }
    if (!sl) {
        host_plan_slot_drop(victim);
        if (cm) {
            /* one locale per process: `representatives` is this locale's block of the hashed basis and x, y are the
             * matching blocks (Diagonalize.chpl:134-162 runs the callback on every locale in lock-step) */
            ls_amd_dist *dd;
            if (ls_amd_dist_create(&dd, cm, op, LS_AMD_F64, e->d_reps_cache, n, 0, NULL) != 0) return -1;
            victim->dist = dd;
        } else {
            ls_amd_plan *pl;
            uint64_t const *reps[1] = {e->d_reps_cache};
            int64_t counts[1] = {n};
            if (ls_amd_plan_create(&pl, op, LS_AMD_F64, 1, -1, reps, counts, 0, LS_AMD_MODE_AUTO, NULL) != 0) return -1;
            victim->plan = pl;
        }
        victim->op = op;
        victim->comm = cm;
        sl = victim;
    }
    sl->stamp = ++e->host_plan_clock;
    ls_amd_plan *plan = cm ? ls_amd_dist_plan((ls_amd_dist *)sl->dist) : (ls_amd_plan *)sl->plan;
    size_t const bytes = 8 * (size_t)n;
    int const xk = lsk_pointer_kind(x), yk = lsk_pointer_kind(y);
    int const upload_y = !op->diag_terms || op->diag_terms->number_terms == 0; /* y += H x: the caller's y matters */
    int const nbuf = ncols > 1 ? 2 : 1;
    for (int i = 0; i < nbuf; ++i) {
        if (xk != LSK_PTR_DEVICE && !sl->d_x[i]) DEV(lsk_malloc(&sl->d_x[i], bytes));
        if (yk != LSK_PTR_DEVICE && !sl->d_y[i]) DEV(lsk_malloc(&sl->d_y[i], bytes));
    }
    sl->stage_n = n;
    __atomic_fetch_add(&g_bstats.calls, 1, __ATOMIC_RELAXED);
    __atomic_fetch_add(&g_bstats.columns, ncols, __ATOMIC_RELAXED);
    if (xk == LSK_PTR_DEVICE) __atomic_fetch_add(&g_bstats.device_x, ncols, __ATOMIC_RELAXED);
    if (yk == LSK_PTR_DEVICE) __atomic_fetch_add(&g_bstats.device_y, ncols, __ATOMIC_RELAXED);
    /* pipeline over the columns: [upload x_0 (+ y_0)] ; for k: launch matvec_k | upload x_{k+1} (+ y_{k+1}) and download y_{k-1}
     * while it runs | check ; [download y_last] */
#define XDEV(k) (xk == LSK_PTR_DEVICE ? (void *)(x + (int64_t)(k) * ldx) : sl->d_x[(k) & (nbuf - 1)])
#define YDEV(k) (yk == LSK_PTR_DEVICE ? (void *)(y + (int64_t)(k) * ldy) : sl->d_y[(k) & (nbuf - 1)])
    if (xk != LSK_PTR_DEVICE && transfer(XDEV(0), x, bytes, xk, NULL, NULL, 0, 0) != 0) return -1;
    if (yk != LSK_PTR_DEVICE && upload_y && transfer(YDEV(0), y, bytes, yk, NULL, NULL, 0, 0) != 0) return -1;
    for (int k = 0; k < ncols; ++k) {
        int rc;
        if (cm) rc = ls_amd_dist_matvec((ls_amd_dist *)sl->dist, XDEV(k), YDEV(k), NULL);
        else {
            void const *xs[1] = {XDEV(k)};
            void *ys[1] = {YDEV(k)};
            rc = ls_amd_matvec(plan, xs, ys, NULL);
        }
        /* (error exits after a launch wait for the device: the slot's persistent d_x / d_y must not be overwritten by the next call
         * while a kernel of this one still reads them -- ADVICE r5) */
#define FAIL_AFTER_LAUNCH do { (void)lsk_device_sync(); return -1; } while (0)
        if (rc != 0) FAIL_AFTER_LAUNCH;
        /* while the kernel runs: the next column goes up, the previous result comes down (different buffers) */
        int const up = k + 1 < ncols && xk != LSK_PTR_DEVICE, down = k >= 1 && yk != LSK_PTR_DEVICE;
        if ((up || down) && transfer(up ? XDEV(k + 1) : NULL, up ? x + (int64_t)(k + 1) * ldx : NULL, up ? bytes : 0, xk,
                                     down ? y + (int64_t)(k - 1) * ldy : NULL, down ? YDEV(k - 1) : NULL, down ? bytes : 0, yk) != 0) FAIL_AFTER_LAUNCH;
        /* (y += H x: the next column's y goes up only now -- its buffer held the result that has just come down) */
        if (k + 1 < ncols && yk != LSK_PTR_DEVICE && upload_y &&
            transfer(YDEV(k + 1), y + (int64_t)(k + 1) * ldy, bytes, yk, NULL, NULL, 0, 0) != 0) FAIL_AFTER_LAUNCH;
        if (ls_amd_plan_check(plan, NULL) != 0) FAIL_AFTER_LAUNCH; /* synchronises the launch stream; halts on an invalid index */
#undef FAIL_AFTER_LAUNCH
    }
    if (yk != LSK_PTR_DEVICE &&
        transfer(NULL, NULL, 0, 0, y + (int64_t)(ncols - 1) * ldy, YDEV(ncols - 1), bytes, yk) != 0) return -1;
#undef XDEV
#undef YDEV
    return 0;
}

void ls_chpl_matrix_vector_product(ls_hs_operator *matrixPtr, int numVectors, double *xPtr, double *yPtr) {
    if (ls_hs_basis_number_words(matrixPtr->basis) != 1) { halt_with("bases with more than 64 bits are not yet implemented"); return; }
    if (numVectors != 1) { halt_with("applying the Operator to more than 1 vector is not yet implemented"); return; }
    if (!matrixPtr->basis->representatives.elts) { halt_with("basis is not built"); return; }
    int64_t n = (int64_t)matrixPtr->basis->representatives.num_elts;
    if (host_matvec_block(matrixPtr, n, 1, xPtr, n, yPtr, n, NULL) != 0) halt_with("%s", g_last_error);
}

void ls_chpl_primme_matvec(void *x, int64_t *ldx, void *y, int64_t *ldy, int *blockSize, void *primme,
                           int *ierr) {
    ls_primme_params_view *pp = (ls_primme_params_view *)primme;
    ls_hs_operator *op = (ls_hs_operator *)pp->matrix;
    int64_t n = pp->nLocal;
    *ierr = 0;
    if (*ldx < n || *ldy < n) { *ierr = -1; return; }
    /* all blockSize columns through ONE pipeline (x_{k+1} up and y_{k-1} down while column k computes) */
    if (host_matvec_block(op, n, *blockSize, (double const *)x, *ldx, (double *)y, *ldy, (ls_amd_comm *)pp->commInfo) != 0) {
        halt_with("%s", g_last_error);
        *ierr = -1;
    }
}
/* primmeGlobalSumReal / primmeBroadcastReal: dist.c (collective over the communicator) */

static void free_array(void *p) { free(p); }

void ls_chpl_operator_apply_diag(ls_hs_operator *matrixPtr, int64_t count, uint64_t *alphas,
                                 chpl_external_array *coeffs, int64_t numTasks) {
    (void)numTasks;
    if (ls_hs_basis_number_words(matrixPtr->basis) != 1) { halt_with("bases with more than 64 bits are not yet implemented"); return; }
    if (matrixPtr->basis->requires_projection) { halt_with("bases that require projection are not yet supported"); return; }
    lsk_operator dop;
    if (operator_device(matrixPtr, &dop) != 0) { halt_with("%s", g_last_error); return; }
    double *h = (double *)malloc(8 * (size_t)(count > 0 ? count : 1));
    void *da = NULL, *dy = NULL;
    int rc = lsk_malloc(&da, 8 * (size_t)count) || lsk_malloc(&dy, 8 * (size_t)count) ||
             lsk_h2d(da, alphas, 8 * (size_t)count) ||
             lsk_diag_coeffs(dop, count, (uint64_t const *)da, (double *)dy, NULL, NULL) || lsk_sync(NULL) ||
             lsk_d2h(h, dy, 8 * (size_t)count);
    lsk_free(da); lsk_free(dy);
    if (rc) { free(h); halt_with("%s", lsk_last_error()); return; }
    coeffs->elts = h;
    coeffs->num_elts = (uint64_t)count;
    coeffs->freer = (void *)free_array;
}

void ls_chpl_operator_apply_off_diag(ls_hs_operator *matrixPtr, int64_t count, uint64_t *alphas,
                                     chpl_external_array *betas, chpl_external_array *coeffs,
                                     chpl_external_array *offsets, int64_t numTasks) {
    (void)numTasks;
    if (ls_hs_basis_number_words(matrixPtr->basis) != 1) { halt_with("bases with more than 64 bits are not yet implemented"); return; }
    if (matrixPtr->basis->requires_projection) { halt_with("bases that require projection are not yet supported"); return; }
    int const T = OEXT(matrixPtr)->n_groups;
    int64_t *h_off = (int64_t *)calloc((size_t)count + 1, sizeof(int64_t));
    if (T == 0) {
        betas->elts = NULL; betas->num_elts = 0; betas->freer = NULL;
        coeffs->elts = NULL; coeffs->num_elts = 0; coeffs->freer = NULL;
        offsets->elts = h_off; offsets->num_elts = (uint64_t)count + 1; offsets->freer = (void *)free_array;
        return;
    }
    lsk_operator dop;
    if (operator_device(matrixPtr, &dop) != 0) { free(h_off); halt_with("%s", g_last_error); return; }
    size_t cap = (size_t)count * (size_t)T;
    uint64_t *h_b = (uint64_t *)calloc(cap ? cap : 1, 8);
    double *h_c = (double *)calloc(cap ? cap : 1, 16);
    void *da = NULL, *dcnt = NULL, *doff = NULL, *db = NULL, *dc = NULL;
    int rc = lsk_malloc(&da, 8 * (size_t)count) || lsk_malloc(&dcnt, 8 * ((size_t)count + 1)) ||
             lsk_malloc(&doff, 8 * ((size_t)count + 1)) || lsk_malloc(&db, 8 * cap) || lsk_malloc(&dc, 16 * cap) ||
             lsk_h2d(da, alphas, 8 * (size_t)count) || lsk_memset_async(dcnt, 0, 8 * ((size_t)count + 1), NULL) ||
             lsk_offdiag_counts(dop, count, (uint64_t const *)da, (int64_t *)dcnt, NULL) ||
             lsk_exclusive_scan_i64(count + 1, (int64_t const *)dcnt, (int64_t *)doff, NULL) ||
             lsk_offdiag_fill(dop, count, (uint64_t const *)da, (int64_t const *)doff, (uint64_t *)db, (double *)dc, NULL, NULL) ||
             lsk_sync(NULL) || lsk_d2h(h_off, doff, 8 * ((size_t)count + 1));
    if (!rc) {
        size_t total = (size_t)h_off[count];
        rc = lsk_d2h(h_b, db, 8 * total) || lsk_d2h(h_c, dc, 16 * total);
    }
    lsk_free(da); lsk_free(dcnt); lsk_free(doff); lsk_free(db); lsk_free(dc);
    if (rc) { free(h_off); free(h_b); free(h_c); halt_with("%s", lsk_last_error()); return; }
    betas->elts = h_b; betas->num_elts = cap; betas->freer = (void *)free_array;
    coeffs->elts = h_c; coeffs->num_elts = cap; coeffs->freer = (void *)free_array;
    offsets->elts = h_off; offsets->num_elts = (uint64_t)count + 1; offsets->freer = (void *)free_array;
}

/* ============================================================================================ */
/* batched externs with the reference's signatures (host arrays, device kernels)                 */
/* ============================================================================================ */
static uint64_t *gather_u64(uint64_t const *src, ptrdiff_t n, ptrdiff_t stride) {
    uint64_t *t = (uint64_t *)malloc(8 * (size_t)(n > 0 ? n : 1));
    for (ptrdiff_t i = 0; i < n; ++i) t[i] = src[i * stride];
    return t;
}

void ls_hs_state_index(ls_hs_basis const *basis_c, ptrdiff_t n, uint64_t const *spins, ptrdiff_t sstride,
                       ptrdiff_t *indices, ptrdiff_t istride) {
    ls_hs_basis *b = (ls_hs_basis *)basis_c;
    struct ls_amd_basis_ext *e = BEXT(b);
    if (n <= 0) return;
    if (ensure_device_reps(b) != 0) { halt_with("%s", g_last_error); return; }
    uint64_t const *d_binom;
    if (device_binom(&d_binom) != 0) { halt_with("%s", g_last_error); return; }
    lsk_index ix;
    memset(&ix, 0, sizeof(ix));
    ix.count = (int64_t)e->d_reps_count;
    ix.reps = e->d_reps_cache;
    ix.binom = d_binom;
    if (b->state_index_is_identity) ix.kind = LSK_INDEX_IDENTITY;
    if (e->product && !e->fermi && e->index_kind != LSK_INDEX_SEARCH) {
        /* the spinful product basis: two closed-form ranks, once the representatives are known to be the whole basis in order */
        ix.prod_sites = b->number_sites; ix.prod_up = e->prod_up; ix.prod_dn = e->prod_dn;
        ix.prod_na = (int64_t)binom(b->number_sites, e->prod_up);
        if (e->index_kind != LSK_INDEX_PRODUCT) {
            int flag = 1;
            void *df = NULL;
            ix.kind = LSK_INDEX_PRODUCT;
            if (ix.count == ix.prod_na * (int64_t)binom(b->number_sites, e->prod_dn) && lsk_malloc(&df, sizeof(int)) == 0) {
                flag = 0;
                if (lsk_h2d(df, &flag, sizeof(int)) != 0 || lsk_check_product(ix, ix.count, ix.reps, (int *)df, NULL) != 0 ||
                    lsk_sync(NULL) != 0 || lsk_d2h(&flag, df, sizeof(int)) != 0) flag = 1;
                lsk_free(df);
            }
            e->index_kind = flag ? LSK_INDEX_SEARCH : LSK_INDEX_PRODUCT;
        }
        ix.kind = e->index_kind;
    }
    if (!b->state_index_is_identity && ix.kind != LSK_INDEX_PRODUCT) {
        if (!e->d_index_table) {
            part_state ps;
            memset(&ps, 0, sizeof(ps));
            ps.count = ix.count;
            ps.d_reps = ix.reps;
            if (build_search_index(&ps, NBITS(b), NULL) != 0 || lsk_sync(NULL) != 0) { halt_with("%s", g_last_error); return; }
            e->d_index_table = ps.d_table;
            e->index_shift = ps.index.shift;
        }
        ix.kind = LSK_INDEX_SEARCH;
        ix.table = e->d_index_table;
        ix.shift = e->index_shift;
    }
    uint64_t *h = gather_u64(spins, n, sstride);
    int64_t *hi = (int64_t *)malloc(8 * (size_t)n);
    void *ds = NULL, *di = NULL;
    int rc = lsk_malloc(&ds, 8 * (size_t)n) || lsk_malloc(&di, 8 * (size_t)n) || lsk_h2d(ds, h, 8 * (size_t)n) ||
             lsk_state_index(ix, n, (uint64_t const *)ds, (int64_t *)di, NULL) || lsk_sync(NULL) ||
             lsk_d2h(hi, di, 8 * (size_t)n);
    lsk_free(ds); lsk_free(di);
    if (!rc) for (ptrdiff_t i = 0; i < n; ++i) indices[i * istride] = (ptrdiff_t)hi[i];
    free(h); free(hi);
    if (rc) halt_with("%s", lsk_last_error());
}

static int state_info_host(ls_hs_basis const *b, ptrdiff_t n, uint64_t const *alphas, ptrdiff_t astride,
                           uint64_t *betas, double *chars, double *norms) {
    lsk_basis dbs;
    if (basis_device(b, &dbs) != 0) return -1;
    uint64_t *h = gather_u64(alphas, n, astride);
    void *da = NULL, *db = NULL, *dc = NULL, *dn = NULL;
    int rc = lsk_malloc(&da, 8 * (size_t)n) || lsk_malloc(&db, 8 * (size_t)n) || lsk_malloc(&dc, 16 * (size_t)n) ||
             lsk_malloc(&dn, 8 * (size_t)n) || lsk_h2d(da, h, 8 * (size_t)n) ||
             lsk_state_info(dbs, n, (uint64_t const *)da, (uint64_t *)db, (double *)dc, (double *)dn, NULL) ||
             lsk_sync(NULL) || lsk_d2h(betas, db, 8 * (size_t)n) || lsk_d2h(chars, dc, 16 * (size_t)n) ||
             lsk_d2h(norms, dn, 8 * (size_t)n);
    lsk_free(da); lsk_free(db); lsk_free(dc); lsk_free(dn);
    free(h);
    return rc ? dev_error() : 0;
}

void ls_hs_state_info(ls_hs_basis const *basis, ptrdiff_t n, uint64_t const *alphas, ptrdiff_t astride,
                      uint64_t *betas, ptrdiff_t bstride, ls_hs_scalar *characters, double *norms) {
    if (n <= 0) return;
    uint64_t *hb = (uint64_t *)malloc(8 * (size_t)n);
    if (state_info_host(basis, n, alphas, astride, hb, (double *)characters, norms) != 0) { free(hb); halt_with("%s", g_last_error); return; }
    for (ptrdiff_t i = 0; i < n; ++i) betas[i * bstride] = hb[i];
    free(hb);
}

void ls_hs_is_representative(ls_hs_basis const *basis, ptrdiff_t n, uint64_t const *alphas, ptrdiff_t astride,
                             uint8_t *are_representatives, double *norms) {
    if (n <= 0) return;
    uint64_t *hb = (uint64_t *)malloc(8 * (size_t)n);
    double *hc = (double *)malloc(16 * (size_t)n);
    if (state_info_host(basis, n, alphas, astride, hb, hc, norms) != 0) { free(hb); free(hc); halt_with("%s", g_last_error); return; }
    for (ptrdiff_t i = 0; i < n; ++i) are_representatives[i] = hb[i] == alphas[i * astride];
    free(hb); free(hc);
}

void ls_internal_operator_apply_diag_x1(ls_hs_operator const *op, ptrdiff_t n, uint64_t const *alphas, double *ys,
                                        double const *xs) {
    if (n <= 0) return;
    lsk_operator dop;
    if (operator_device(op, &dop) != 0) { halt_with("%s", g_last_error); return; }
    void *da = NULL, *dy = NULL, *dx = NULL;
    int rc = lsk_malloc(&da, 8 * (size_t)n) || lsk_malloc(&dy, 8 * (size_t)n) || lsk_h2d(da, alphas, 8 * (size_t)n);
    if (!rc && xs) rc = lsk_malloc(&dx, 8 * (size_t)n) || lsk_h2d(dx, xs, 8 * (size_t)n);
    if (!rc) rc = lsk_diag_coeffs(dop, n, (uint64_t const *)da, (double *)dy, (double const *)dx, NULL) || lsk_sync(NULL) ||
                  lsk_d2h(ys, dy, 8 * (size_t)n);
    lsk_free(da); lsk_free(dy); lsk_free(dx);
    if (rc) halt_with("%s", lsk_last_error());
}

void ls_internal_operator_apply_off_diag_x1(ls_hs_operator const *op, ptrdiff_t n, uint64_t const *alphas,
                                            uint64_t *betas, ls_hs_scalar *coeffs, ptrdiff_t *offsets,
                                            double const *xs) {
    offsets[0] = 0;
    if (n <= 0) return;
    int const T = OEXT(op)->n_groups;
    if (T == 0) { for (ptrdiff_t i = 0; i <= n; ++i) offsets[i] = 0; return; }
    lsk_operator dop;
    if (operator_device(op, &dop) != 0) { halt_with("%s", g_last_error); return; }
    size_t cap = (size_t)n * (size_t)T;
    int64_t *h_off = (int64_t *)malloc(8 * ((size_t)n + 1));
    void *da = NULL, *dcnt = NULL, *doff = NULL, *db = NULL, *dc = NULL, *dx = NULL;
    int rc = lsk_malloc(&da, 8 * (size_t)n) || lsk_malloc(&dcnt, 8 * ((size_t)n + 1)) ||
             lsk_malloc(&doff, 8 * ((size_t)n + 1)) || lsk_malloc(&db, 8 * cap) || lsk_malloc(&dc, 16 * cap) ||
             lsk_h2d(da, alphas, 8 * (size_t)n) || lsk_memset_async(dcnt, 0, 8 * ((size_t)n + 1), NULL);
    if (!rc && xs) rc = lsk_malloc(&dx, 8 * (size_t)n) || lsk_h2d(dx, xs, 8 * (size_t)n);
    if (!rc) rc = lsk_offdiag_counts(dop, n, (uint64_t const *)da, (int64_t *)dcnt, NULL) ||
                  lsk_exclusive_scan_i64(n + 1, (int64_t const *)dcnt, (int64_t *)doff, NULL) ||
                  lsk_offdiag_fill(dop, n, (uint64_t const *)da, (int64_t const *)doff, (uint64_t *)db, (double *)dc,
                                   (double const *)dx, NULL) ||
                  lsk_sync(NULL) || lsk_d2h(h_off, doff, 8 * ((size_t)n + 1));
    if (!rc) {
        size_t total = (size_t)h_off[n];
        rc = lsk_d2h(betas, db, 8 * total) || lsk_d2h(coeffs, dc, 16 * total);
        for (ptrdiff_t i = 0; i <= n; ++i) offsets[i] = (ptrdiff_t)h_off[i];
    }
    lsk_free(da); lsk_free(dcnt); lsk_free(doff); lsk_free(db); lsk_free(dc); lsk_free(dx);
    free(h_off);
    if (rc) halt_with("%s", lsk_last_error());
}

/* ============================================================================================ */
/* cross-sector operators (include/ls_amd.h: ls_amd_operator_adjoint, ls_amd_operator_maps_sector, ls_amd_cross) */
/* ============================================================================================ */
/* every term of an operator as (v, m, r, x, s): the diagonal ones (x = 0), then the groups */
static int operator_raw_terms(ls_hs_operator const *op, raw_term **out) {
    struct ls_amd_operator_ext const *e = OEXT(op);
    int const n = e->n_diag + e->n_off;
    raw_term *t = (raw_term *)malloc(sizeof(raw_term) * (size_t)(n > 0 ? n : 1));
    int k = 0;
    for (int i = 0; i < e->n_diag; ++i, ++k) { raw_term r = {e->diag[i].v_re, e->diag[i].v_im, e->diag[i].m, e->diag[i].r, 0, e->diag[i].s}; t[k] = r; }
    for (int g = 0; g < e->n_groups; ++g)
        for (int i = e->groups[g].begin; i < e->groups[g].end; ++i, ++k) {
            raw_term r = {e->off[i].v_re, e->off[i].v_im, e->off[i].m, e->off[i].r, e->groups[g].x, e->off[i].s};
            t[k] = r;
        }
    *out = t;
    return n;
}

/* A|a> = v [a & m == r] (-1)^popcount(a & s) |a ^ x>, so <b|A|a> lives at b = a ^ x and
 *   A+|b> = conj(v) [(b ^ x) & m == r] (-1)^popcount((b ^ x) & s) |b ^ x>
 *         = conj(v) (-1)^popcount(x & s) [b & m == r ^ (x & m)] (-1)^popcount(b & s) |b ^ x>
 * (the parity of (b ^ x) & s is the sum of the parities of b & s and x & s) */
ls_hs_operator *ls_amd_operator_adjoint(ls_hs_operator const *op) {
    if (!op) { set_error("ls_amd_operator_adjoint: NULL operator"); return NULL; }
    if (!reg_get(op)) { set_error("ls_amd_operator_adjoint: unknown operator (ls_amd_adopt_operator first)"); return NULL; }
    raw_term *t = NULL;
    int const n = operator_raw_terms(op, &t);
    size_t const cap = (size_t)(n > 0 ? n : 1);
    double *v = (double *)malloc(16 * cap);
    uint64_t *m = (uint64_t *)malloc(8 * cap), *r = (uint64_t *)malloc(8 * cap), *x = (uint64_t *)malloc(8 * cap), *s = (uint64_t *)malloc(8 * cap);
    for (int k = 0; k < n; ++k) {
        double const sg = (__builtin_popcountll(t[k].x & t[k].s) & 1) ? -1.0 : 1.0;
        v[2 * k] = sg * t[k].re; v[2 * k + 1] = -sg * t[k].im;
        m[k] = t[k].m; r[k] = t[k].r ^ (t[k].x & t[k].m); x[k] = t[k].x; s[k] = t[k].s;
    }
    ls_hs_operator *adj = ls_hs_create_operator_from_terms(op->basis, n, v, m, r, x, s);
    free(t); free(v); free(m); free(r); free(x); free(s);
    return adj;
}

/* ---- the covariance check: U_g A U_g^-1 == chi2(g) conj(chi1(g)) A for every generator and the spin inversion ----
 * A term is first written out on its full support u = m | x | s as 2^|u \ m| pure projector terms (u, pattern, x) with the sign
 * folded into the coefficient: sigma^z given as a sign mask and as two projector terms then are the same two entries.  A
 * permutation relabels the sites of such an entry, (g.w)[i] = w[g[i]] for w = u, pattern, x; the inversion complements the
 * pattern inside u.  Two operators are compared entry by entry after sorting and merging. */
typedef struct { uint64_t u, r, x; double re, im; } canon_term;
static int canon_cmp(void const *pa, void const *pb) {
    canon_term const *a = (canon_term const *)pa, *b = (canon_term const *)pb;
    if (a->x != b->x) return a->x < b->x ? -1 : 1;
    if (a->u != b->u) return a->u < b->u ? -1 : 1;
    if (a->r != b->r) return a->r < b->r ? -1 : 1;
    return 0;
}
#define CANON_MAX_FREE 12 /* sites of a term's support outside its projector mask (spin operators: 0-2) */
static int64_t canon_expand(ls_hs_operator const *op, canon_term **out) {
    raw_term *t = NULL;
    int const n = operator_raw_terms(op, &t);
    int64_t total = 0;
    for (int k = 0; k < n; ++k) {
        int const nf = __builtin_popcountll((t[k].x | t[k].s) & ~t[k].m);
        if (nf > CANON_MAX_FREE) { free(t); *out = NULL; return -1; }
        total += (int64_t)1 << nf;
    }
    canon_term *c = (canon_term *)malloc(sizeof(canon_term) * (size_t)(total > 0 ? total : 1));
    int64_t w = 0;
    for (int k = 0; k < n; ++k) {
        uint64_t const fr = (t[k].x | t[k].s) & ~t[k].m;
        int const nf = __builtin_popcountll(fr);
        for (uint64_t pat = 0; pat < (1ULL << nf); ++pat) {
            uint64_t const a = t[k].r | deposit_bits(pat, fr);
            double const sg = (__builtin_popcountll(a & t[k].s) & 1) ? -1.0 : 1.0;
            canon_term e = {t[k].m | fr, a, t[k].x, sg * t[k].re, sg * t[k].im};
            c[w++] = e;
        }
    }
    free(t);
    *out = c;
    return total;
}
static int64_t canon_merge(canon_term *c, int64_t n) {
    qsort(c, (size_t)n, sizeof(canon_term), canon_cmp);
    int64_t w = 0;
    for (int64_t i = 0; i < n;) {
        canon_term acc = c[i];
        int64_t j = i + 1;
        while (j < n && canon_cmp(&c[i], &c[j]) == 0) { acc.re += c[j].re; acc.im += c[j].im; ++j; }
        c[w++] = acc;
        i = j;
    }
    return w;
}
static uint64_t permute_mask(int const *p, int L, uint64_t w) { /* (g.w)[i] = w[p[i]] */
    uint64_t out = 0;
    for (int i = 0; i < L; ++i) out |= ((w >> p[i]) & 1ULL) << i;
    return out;
}
/* largest |g.A - f A| over the entries (c: the merged entries of A, n of them; p == NULL: the inversion) */
static double canon_defect(canon_term const *c, int64_t n, int const *p, int L, double f_re, double f_im) {
    canon_term *both = (canon_term *)malloc(sizeof(canon_term) * (size_t)(2 * n > 0 ? 2 * n : 1));
    for (int64_t i = 0; i < n; ++i) {
        canon_term e = c[i];
        if (p) { e.u = permute_mask(p, L, e.u); e.r = permute_mask(p, L, e.r); e.x = permute_mask(p, L, e.x); }
        else e.r ^= e.u; /* (no sign mask is left after the expansion: the factor (-1)^popcount(s) of the inversion is 1) */
        both[i] = e;
        canon_term m = c[i];
        m.re = -(f_re * c[i].re - f_im * c[i].im);
        m.im = -(f_re * c[i].im + f_im * c[i].re);
        both[n + i] = m;
    }
    int64_t const k = canon_merge(both, 2 * n);
    double worst = 0.0;
    for (int64_t i = 0; i < k; ++i) {
        double const d = fabs(both[i].re) > fabs(both[i].im) ? fabs(both[i].re) : fabs(both[i].im);
        if (d > worst) worst = d;
    }
    free(both);
    return worst;
}

/* signs != 0: projected fermionic bases are admitted (the caller runs the signed covariance rule) */
static int cross_preconditions(ls_hs_basis const *a, ls_hs_basis const *b, int signs) {
    struct ls_amd_basis_ext const *ea = (struct ls_amd_basis_ext const *)reg_get(a), *eb = (struct ls_amd_basis_ext const *)reg_get(b);
    if (!ea || !eb) return set_error("cross-sector: unknown basis (ls_amd_adopt_basis first)");
    if (a->particle_type != b->particle_type) return set_error("cross-sector: the bases have different particle types (%d and %d)", a->particle_type, b->particle_type);
    if (!signs && (ea->fermi || eb->fermi))
        return set_error("cross-sector: projected fermionic bases are not supported (permutation signs in the projection; follow-up: a "
                         "sign-aware cross kernel next to k_fermi) -- use the unprojected (N, N_up) bases");
    if (a->number_sites != b->number_sites || ea->nbits != eb->nbits)
        return set_error("cross-sector: the bases have different number_sites (%d and %d)", a->number_sites, b->number_sites);
    if (ea->nbits > 64) return set_error("cross-sector: more than 64 sites are not supported (number_words == 1)");
    if ((a->spin_inversion != 0) != (b->spin_inversion != 0))
        return set_error("cross-sector: spin inversion is present on one basis only (source %d, target %d)", a->spin_inversion, b->spin_inversion);
    if (ea->n_generators != eb->n_generators ||
        (ea->n_generators > 0 && memcmp(ea->gen_perms, eb->gen_perms, sizeof(int) * (size_t)ea->n_generators * (size_t)ea->nbits) != 0))
        return set_error("cross-sector: the bases have different generators (same permutations in the same order are required; only the "
                         "sectors may differ)");
    return 0;
}

int ls_amd_operator_maps_sector(ls_hs_operator const *op, ls_hs_basis const *target) {
    if (!op || !target) return set_error("ls_amd_operator_maps_sector: NULL %s", !op ? "operator" : "target basis");
    if (!reg_get(op)) return set_error("ls_amd_operator_maps_sector: unknown operator (ls_amd_adopt_operator first)");
    ls_hs_basis const *src = op->basis;
    if (cross_preconditions(src, target, 0) != 0) return -1;
    struct ls_amd_basis_ext const *es = BEXT(src), *et = BEXT(target);
    int const L = es->nbits;
    if (es->n_generators == 0 && src->spin_inversion == 0) return 0; /* no group: nothing to be covariant under */
    canon_term *c = NULL;
    int64_t n = canon_expand(op, &c);
    if (n < 0) return set_error("ls_amd_operator_maps_sector: a term's support exceeds its projector mask by more than %d sites", CANON_MAX_FREE);
    n = canon_merge(c, n);
    double vmax = 0.0;
    for (int64_t i = 0; i < n; ++i) { double const a = fabs(c[i].re) > fabs(c[i].im) ? fabs(c[i].re) : fabs(c[i].im); if (a > vmax) vmax = a; }
    double const tol = 1e-12 * vmax;
    int rc = 0;
    for (int g = 0; g < es->n_generators && rc == 0; ++g) {
        int const *p = es->gen_perms + (size_t)g * L;
        int const ord = perm_order(p, L);
        /* chi(g) = exp(-2 pi i sector / order): chi2 conj(chi1) = exp(-2 pi i (sector2 - sector1) / order) */
        double const phi = -2.0 * M_PI * (double)(et->gen_sectors[g] - es->gen_sectors[g]) / (double)ord;
        double const defect = canon_defect(c, n, p, L, cos(phi), sin(phi));
        if (defect > tol)
            rc = set_error("the operator does not map the source sector into the target sector: under generator %d (sector %d -> %d of "
                           "order %d) it must pick up the factor exp(-2 pi i %d / %d), and misses that by %.3g",
                           g, es->gen_sectors[g], et->gen_sectors[g], ord, et->gen_sectors[g] - es->gen_sectors[g], ord, defect);
    }
    if (rc == 0 && src->spin_inversion != 0) {
        double const f = (double)(src->spin_inversion * target->spin_inversion);
        double const defect = canon_defect(c, n, NULL, L, f, 0.0);
        if (defect > tol)
            rc = set_error("the operator does not map the source sector into the target sector: under the spin inversion (character %d -> "
                           "%d) it must pick up the factor %d, and misses that by %.3g", src->spin_inversion, target->spin_inversion, (int)f, defect);
    }
    free(c);
    return rc;
}

/* ---- the signed covariance rule: projected fermionic bases, U_g|a> = sign(g, a)|g.a> ----
 * sign(g, a) = (-1)^Q(a), Q(a) = the occupied pairs j < i with j in tab[i] (tab: the sign table of g, as fermi_sign_table builds
 * it): a GF(2) quadratic form.  For a raw term (v, m, r, x, s) with x inside m, sign(g, a) sign(g, a ^ x) is affine in the bits of a
 * outside x -- a pair with exactly one mode i in x contributes the other mode's bit: the sign mask lin = XOR_{i in x} nb(i) & ~x,
 * nb(i) = tab[i] | {k > i : i in tab[k]} -- and constant on the bits inside, which r fixes: a pair inside x contributes
 * r'_i r'_j + r_i r_j with r' = r ^ x.  So conjugation stays inside the term format,
 *     U_g A_t U_g^-1 = ((-1)^c v, g.m, g.r, g.x, g.(s ^ lin)).
 * A fermionic term drags a Jordan-Wigner string over up to 63 modes outside m, which canon_expand cannot write out; but the string
 * of a flip mask x is J(x) = XOR_{j in x} ((1 << j) - 1) whatever the monomial, so only free = (s ^ J(x)) & ~m is expanded --
 * entries (u = m | free, pattern, x), the sign of the pattern folded into the coefficient -- and the residual sign
 * (-1)^popcount(a & J(x) & ~u) is a function of the key (u, x): two entries with one key are the same operator. */
static void perm_sign_table(int const *p, int L, uint64_t *tab, uint64_t *nb) {
    int q[64];
    for (int i = 0; i < L; ++i) q[p[i]] = i;
    for (int i = 0; i < L; ++i) {
        tab[i] = 0;
        for (int j = 0; j < i; ++j)
            if (q[j] > q[i]) tab[i] |= 1ULL << j;
    }
    for (int i = 0; i < L; ++i) {
        nb[i] = tab[i];
        for (int k = i + 1; k < L; ++k)
            if ((tab[k] >> i) & 1ULL) nb[i] |= 1ULL << k;
    }
}
static uint64_t jw_string(uint64_t x) { /* bit k: the parity of the modes of x above k */
    uint64_t out = 0;
    for (uint64_t w = x; w != 0; w &= w - 1) out ^= (1ULL << __builtin_ctzll(w)) - 1;
    return out;
}
/* U_g t U_g^-1 of one raw term with t.x inside t.m */
static raw_term signed_conjugate(raw_term t, int const *p, int L, uint64_t const *tab, uint64_t const *nb) {
    uint64_t lin = 0;
    uint64_t const r0 = t.r & t.x, r1 = r0 ^ t.x;
    int c = 0;
    for (uint64_t w = t.x; w != 0; w &= w - 1) {
        int const i = __builtin_ctzll(w);
        lin ^= nb[i] & ~t.x;
        if ((r0 >> i) & 1ULL) c ^= __builtin_popcountll(tab[i] & r0) & 1;
        if ((r1 >> i) & 1ULL) c ^= __builtin_popcountll(tab[i] & r1) & 1;
    }
    raw_term out = t;
    if (c) { out.re = -out.re; out.im = -out.im; }
    out.m = permute_mask(p, L, t.m); out.r = permute_mask(p, L, t.r); out.x = permute_mask(p, L, t.x);
    out.s = permute_mask(p, L, t.s ^ lin);
    return out;
}
/* the canonical entries of n raw terms; -1 - k when term k keeps more than CANON_MAX_FREE sign bits beside its Jordan-Wigner string */
static int64_t signed_expand(raw_term const *t, int n, canon_term **out) {
    int64_t total = 0;
    *out = NULL;
    for (int k = 0; k < n; ++k) {
        int const nf = __builtin_popcountll((t[k].s ^ jw_string(t[k].x)) & ~t[k].m);
        if (nf > CANON_MAX_FREE) return -1 - (int64_t)k;
        total += (int64_t)1 << nf;
    }
    canon_term *c = (canon_term *)malloc(sizeof(canon_term) * (size_t)(total > 0 ? total : 1));
    int64_t w = 0;
    for (int k = 0; k < n; ++k) {
        uint64_t const fr = (t[k].s ^ jw_string(t[k].x)) & ~t[k].m;
        int const nf = __builtin_popcountll(fr);
        for (uint64_t pat = 0; pat < (1ULL << nf); ++pat) {
            uint64_t const a = t[k].r | deposit_bits(pat, fr);
            double const sg = (__builtin_popcountll(a & t[k].s) & 1) ? -1.0 : 1.0;
            canon_term e = {t[k].m | fr, a, t[k].x, sg * t[k].re, sg * t[k].im};
            c[w++] = e;
        }
    }
    *out = c;
    return total;
}
static int not_fermionic(raw_term const *t) {
    return set_error("ls_amd_operator_maps_sector_signed: a term is not a fermionic operator: beside the Jordan-Wigner string of its "
                     "flip mask (x = 0x%llx) its sign mask (s = 0x%llx) holds more than %d modes outside its projector mask (m = 0x%llx)",
                     (unsigned long long)t->x, (unsigned long long)t->s, CANON_MAX_FREE, (unsigned long long)t->m);
}

/* the signed rule for one permutation p: *defect = the largest |U_p A U_p^-1 - f A| over the canonical entries (t: the n raw terms of
 * A, c: their nc merged entries; tg: room for n terms; *both: scratch that grows, freed by the caller).  -1 when the image of a
 * term is no fermionic operator (the message names the term as it was given). */
static int signed_defect(raw_term const *t, int n, canon_term const *c, int64_t nc, int const *p, int L, double f_re, double f_im,
                         raw_term *tg, canon_term **both, double *defect) {
    uint64_t tab[64], nb[64];
    perm_sign_table(p, L, tab, nb);
    for (int k = 0; k < n; ++k) tg[k] = signed_conjugate(t[k], p, L, tab, nb);
    canon_term *cg = NULL;
    int64_t const ng = signed_expand(tg, n, &cg);
    if (ng < 0) return not_fermionic(&t[-1 - ng]); /* (shown by the image only: the term as it was given) */
    *both = (canon_term *)realloc(*both, sizeof(canon_term) * (size_t)(ng + nc > 0 ? ng + nc : 1));
    memcpy(*both, cg, sizeof(canon_term) * (size_t)ng);
    free(cg);
    for (int64_t i = 0; i < nc; ++i) {
        canon_term m = c[i];
        m.re = -(f_re * c[i].re - f_im * c[i].im);
        m.im = -(f_re * c[i].im + f_im * c[i].re);
        (*both)[ng + i] = m;
    }
    int64_t const k = canon_merge(*both, ng + nc);
    *defect = 0.0;
    for (int64_t i = 0; i < k; ++i) {
        double const d = fabs((*both)[i].re) > fabs((*both)[i].im) ? fabs((*both)[i].re) : fabs((*both)[i].im);
        if (d > *defect) *defect = d;
    }
    return 0;
}

int ls_amd_operator_maps_sector_signed(ls_hs_operator const *op, ls_hs_basis const *target) {
    if (!op || !target) return set_error("ls_amd_operator_maps_sector_signed: NULL %s", !op ? "operator" : "target basis");
    if (!reg_get(op)) return set_error("ls_amd_operator_maps_sector_signed: unknown operator (ls_amd_adopt_operator first)");
    ls_hs_basis const *src = op->basis;
    struct ls_amd_basis_ext const *es = (struct ls_amd_basis_ext const *)reg_get(src), *et = (struct ls_amd_basis_ext const *)reg_get(target);
    if (!es || !et || !(es->fermi || et->fermi)) return ls_amd_operator_maps_sector(op, target); /* no permutation signs: the plain rule */
    if (cross_preconditions(src, target, 1) != 0) return -1;
    int const L = es->nbits;
    raw_term *t = NULL, *tg = NULL;
    canon_term *c = NULL, *both = NULL;
    int const n = operator_raw_terms(op, &t);
    int rc = 0;
    for (int k = 0; k < n && rc == 0; ++k)
        if (t[k].x & ~t[k].m)
            rc = set_error("ls_amd_operator_maps_sector_signed: a term flips modes outside its projector mask (x = 0x%llx is not inside "
                           "m = 0x%llx): not a product of creation and annihilation operators", (unsigned long long)t[k].x, (unsigned long long)t[k].m);
    int64_t nc = 0;
    if (rc == 0 && (nc = signed_expand(t, n, &c)) < 0) rc = not_fermionic(&t[-1 - nc]);
    if (rc == 0) {
        nc = canon_merge(c, nc);
        double vmax = 0.0;
        for (int64_t i = 0; i < nc; ++i) { double const a = fabs(c[i].re) > fabs(c[i].im) ? fabs(c[i].re) : fabs(c[i].im); if (a > vmax) vmax = a; }
        double const tol = 1e-12 * vmax;
        tg = (raw_term *)malloc(sizeof(raw_term) * (size_t)(n > 0 ? n : 1));
        for (int g = 0; g < es->n_generators && rc == 0; ++g) {
            int const *p = es->gen_perms + (size_t)g * L;
            int const ord = perm_order(p, L);
            /* g.A - f A, f = chi2(g) conj(chi1(g)) = exp(-2 pi i (sector2 - sector1) / order) */
            double const phi = -2.0 * M_PI * (double)(et->gen_sectors[g] - es->gen_sectors[g]) / (double)ord;
            double defect = 0.0;
            if (signed_defect(t, n, c, nc, p, L, cos(phi), sin(phi), tg, &both, &defect) != 0) { rc = -1; break; }
            if (defect > tol)
                rc = set_error("the operator does not map the source sector into the target sector: under generator %d (sector %d -> %d of "
                               "order %d) it must pick up the factor exp(-2 pi i %d / %d), and misses that by %.3g",
                               g, es->gen_sectors[g], et->gen_sectors[g], ord, et->gen_sectors[g] - es->gen_sectors[g], ord, defect);
        }
    }
    free(t); free(tg); free(c); free(both);
    return rc;
}

/* ---- bases with DIFFERENT groups (include/ls_amd.h: ls_amd_cross_create_groups) ---- */
/* what both new modes need of a pair of bases: one particle type, one number of sites, one word */
static int cross_groups_preconditions(ls_hs_basis const *a, ls_hs_basis const *b) {
    struct ls_amd_basis_ext const *ea = (struct ls_amd_basis_ext const *)reg_get(a), *eb = (struct ls_amd_basis_ext const *)reg_get(b);
    if (!ea || !eb) return set_error("cross-sector: unknown basis (ls_amd_adopt_basis first)");
    if (a->particle_type != b->particle_type) return set_error("cross-sector: the bases have different particle types (%d and %d)", a->particle_type, b->particle_type);
    if (a->number_sites != b->number_sites || ea->nbits != eb->nbits)
        return set_error("cross-sector: the bases have different number_sites (%d and %d)", a->number_sites, b->number_sites);
    if (ea->nbits > 64) return set_error("cross-sector: more than 64 sites are not supported (number_words == 1)");
    return 0;
}

/* the element of the basis' group (the closure its extension holds; spinful bases: over the lifted permutations) that is the
 * permutation p, or -1 */
static int group_element_of(struct ls_amd_basis_ext const *e, int const *p, int L) {
    for (int g = 0; g < e->order; ++g)
        if (memcmp(e->perms + (size_t)g * L, p, sizeof(int) * (size_t)L) == 0) return g;
    return -1;
}

int ls_amd_operator_maps_subgroup_sector(ls_hs_operator const *op, ls_hs_basis const *target) {
    if (!op || !target) return set_error("ls_amd_operator_maps_subgroup_sector: NULL %s", !op ? "operator" : "target basis");
    if (!reg_get(op)) return set_error("ls_amd_operator_maps_subgroup_sector: unknown operator (ls_amd_adopt_operator first)");
    ls_hs_basis const *src = op->basis;
    if (cross_groups_preconditions(src, target) != 0) return -1;
    struct ls_amd_basis_ext const *es = BEXT(src), *et = BEXT(target);
    int const L = es->nbits;
    if (target->spin_inversion != 0 && src->spin_inversion == 0)
        return set_error("cross-sector: the target basis has the spin inversion and the source basis has not: the target group is no "
                         "subgroup of the source group (groups=\"project\" takes any two groups)");
    if (et->spin_flip != 0 && es->spin_flip == 0)
        return set_error("cross-sector: the target basis has spin_flip and the source basis has not: the target group is no subgroup "
                         "of the source group (groups=\"project\" takes any two groups)");
    /* every target generator h as an element of the source group: chi1(h) is that element's character */
    int *at = (int *)malloc(sizeof(int) * (size_t)(et->n_generators > 0 ? et->n_generators : 1));
    for (int g = 0; g < et->n_generators; ++g) {
        at[g] = group_element_of(es, et->gen_perms + (size_t)g * L, L);
        if (at[g] < 0) {
            free(at);
            return set_error("cross-sector: generator %d of the target basis is not an element of the source group (%d elements): the "
                             "target group is no subgroup of the source group (groups=\"project\" takes any two groups)", g, es->order);
        }
    }
    if (et->n_generators == 0 && target->spin_inversion == 0) { free(at); return 0; } /* no target group: always a subgroup, nothing to check */
    int const fermi = es->fermi || et->fermi;
    raw_term *t = NULL, *tg = NULL;
    canon_term *c = NULL, *both = NULL;
    int const n = operator_raw_terms(op, &t);
    int64_t nc = 0;
    int rc = 0;
    if (fermi) {
        for (int k = 0; k < n && rc == 0; ++k)
            if (t[k].x & ~t[k].m)
                rc = set_error("ls_amd_operator_maps_subgroup_sector: a term flips modes outside its projector mask (x = 0x%llx is not "
                               "inside m = 0x%llx): not a product of creation and annihilation operators",
                               (unsigned long long)t[k].x, (unsigned long long)t[k].m);
        if (rc == 0 && (nc = signed_expand(t, n, &c)) < 0) rc = not_fermionic(&t[-1 - nc]);
        tg = (raw_term *)malloc(sizeof(raw_term) * (size_t)(n > 0 ? n : 1));
    } else if ((nc = canon_expand(op, &c)) < 0)
        rc = set_error("ls_amd_operator_maps_subgroup_sector: a term's support exceeds its projector mask by more than %d sites", CANON_MAX_FREE);
    if (rc == 0) {
        nc = canon_merge(c, nc);
        double vmax = 0.0;
        for (int64_t i = 0; i < nc; ++i) { double const a = fabs(c[i].re) > fabs(c[i].im) ? fabs(c[i].re) : fabs(c[i].im); if (a > vmax) vmax = a; }
        double const tol = 1e-12 * vmax;
        for (int g = 0; g < et->n_generators && rc == 0; ++g) {
            int const *p = et->gen_perms + (size_t)g * L;
            int const ord = perm_order(p, L);
            /* f = chi2(h) conj(chi1(h)): chi2 from the target's sector, chi1 from the source's element */
            double const phi = -2.0 * M_PI * (double)et->gen_sectors[g] / (double)ord;
            double const c1r = es->elems[at[g]].ch_re, c1i = es->elems[at[g]].ch_im;
            double const f_re = cos(phi) * c1r + sin(phi) * c1i, f_im = sin(phi) * c1r - cos(phi) * c1i;
            double defect = 0.0;
            if (fermi) { if (signed_defect(t, n, c, nc, p, L, f_re, f_im, tg, &both, &defect) != 0) { rc = -1; break; } }
            else defect = canon_defect(c, nc, p, L, f_re, f_im);
            if (defect > tol)
                rc = set_error("the operator does not map the source sector into the target sector: under generator %d of the target "
                               "(sector %d of order %d there; element %d of the source group, character %.6g%+.6gi) it must pick up the "
                               "factor %.6g%+.6gi, and misses that by %.3g", g, et->gen_sectors[g], ord, at[g], c1r, c1i, f_re, f_im, defect);
        }
        if (rc == 0 && target->spin_inversion != 0) {
            double const f = (double)(src->spin_inversion * target->spin_inversion);
            double const defect = canon_defect(c, nc, NULL, L, f, 0.0);
            if (defect > tol)
                rc = set_error("the operator does not map the source sector into the target sector: under the spin inversion (character %d -> "
                               "%d) it must pick up the factor %d, and misses that by %.3g", src->spin_inversion, target->spin_inversion, (int)f, defect);
        }
    }
    free(at); free(t); free(tg); free(c); free(both);
    return rc;
}

struct ls_amd_cross {
    ls_hs_operator *adj;      /* owned: the adjoint, on the source basis' struct (only its term tables are used) */
    lsk_group *d_groups;      /* owned: the adjoint's groups, x = 0 first when it has diagonal terms */
    lsk_term *d_terms;        /* owned */
    int n_groups, is_real, cplx;
    double tiny;              /* 1e-13 sum |v| over the adjoint's terms: a smaller summed coefficient is rounding residue, not a packet */
    lsk_basis src;            /* device tables owned by the source basis */
    lsk_index six;
    uint32_t *d_table;        /* owned: prefix table of a searched (unprojected, incomplete) source */
    ls_amd_gtab *gtab;        /* shared: static index table of a projected source */
    double *d_norms;          /* owned: n2(r') of every target row */
    uint64_t const *d_src_reps, *d_dst_reps; /* borrowed */
    int64_t n_src, n_dst, nnz;
    int *d_err;               /* owned; d_err + 2: the packet counter of the counting pass (8 bytes) */
    int mode;                 /* LS_AMD_CROSS_SAME | _RESTRICT (both: k_cross_pull) | _PROJECT (k_cross_project, which sums over dst's elements) */
    lsk_basis dst;            /* device tables owned by the target basis */
    void *d_blk_cols;         /* owned: two contiguous scratch columns (source, target) of the column loop of ls_amd_cross_apply_block */
};

/* one apply, or the counting pass (d_count != NULL), by the kernel of the plan's mode */
static int cross_launch(ls_amd_cross *cx, void const *d_x, void *d_y, unsigned long long *d_count, void *stream) {
    lsk_gtab const gt = cx->gtab ? cx->gtab->tab : no_gtab();
    if (cx->mode == LS_AMD_CROSS_PROJECT)
        return lsk_cross_project(cx->n_groups, cx->d_groups, cx->d_terms, cx->is_real, cx->src, cx->six, gt, cx->dst, cx->cplx, cx->n_dst,
                                 cx->d_dst_reps, cx->d_norms, d_x, d_y, cx->tiny, d_count, cx->d_err, stream);
    return lsk_cross_pull(cx->n_groups, cx->d_groups, cx->d_terms, cx->is_real, cx->src, cx->six, gt, cx->cplx, cx->n_dst, cx->d_dst_reps,
                          cx->d_norms, d_x, d_y, cx->tiny, d_count, cx->d_err, stream);
}

void ls_amd_cross_destroy(ls_amd_cross *cx) {
    if (!cx) return;
    if (cx->d_groups) lsk_free(cx->d_groups);
    if (cx->d_terms) lsk_free(cx->d_terms);
    if (cx->d_table) lsk_free(cx->d_table);
    if (cx->d_norms) lsk_free(cx->d_norms);
    if (cx->d_err) lsk_free(cx->d_err);
    if (cx->d_blk_cols) lsk_free(cx->d_blk_cols);
    if (cx->gtab) ls_amd_internal_gtab_release(cx->gtab);
    if (cx->adj) ls_hs_destroy_operator(cx->adj);
    free(cx);
}

static int cross_every_char_pm1(ls_hs_basis const *b) {
    struct ls_amd_basis_ext const *e = BEXT(b);
    for (int g = 0; g < e->order; ++g)
        if (e->elems[g].ch_im != 0.0 || fabs(e->elems[g].ch_re) != 1.0) return 0;
    return 1;
}

/* how the images of a kernel are looked up among the n ascending states d_reps of `basis` (device form: dev): a projected basis
 * through the static index table of the array (shared with the matvec plans over it), an unprojected one through a closed form where
 * the array is the whole identity / fixed-weight / product basis in order, else through a prefix table and a search (*d_table, owned
 * by the caller).  d_err: a device flag that is clear on entry and on return.  `who` words the refusals. */
static int sector_lookup(char const *who, ls_hs_basis const *basis, lsk_basis const *dev, uint64_t const *d_reps, int64_t n, int *d_err,
                         lsk_index *six, uint32_t **d_table, ls_amd_gtab **gtab, void *stream) {
    struct ls_amd_basis_ext const *es = BEXT(basis);
    int const L = es->nbits;
    uint64_t const *d_binom;
    if (device_binom(&d_binom) != 0) return -1;
    memset(six, 0, sizeof(*six));
    six->kind = LSK_INDEX_SEARCH;
    six->count = n;
    six->reps = d_reps;
    six->binom = d_binom;
    six->dir_sites = L;
    six->dir_weight = es->hamming_weight;
    if (n >= 0xffffffffLL) return set_error("%s: source bases with >= 2^32 - 1 states are not supported", who);
    if (dev->fermi && L > 60)
        return set_error("%s: projected fermionic bases of more than 60 modes are not supported (%d modes: the static index table "
                         "of the source does not fit, as for their matvec plans)", who, L);
    if (dev->proj != LSK_PROJ_NONE) {
        if (n > 0 && ls_amd_internal_gtab_acquire(gtab, L, d_reps, n, NULL, 1, stream) != 0) return -1;
    } else if (n > 0) {
        int const h = es->hamming_weight;
        int closed = 0, zero = 0, flag = 0;
        if (h < 0 && L < 63 && n == ((int64_t)1 << L)) { six->kind = LSK_INDEX_IDENTITY; closed = 1; }
        else if (h >= 0 && (uint64_t)n == binom(L, h)) {
            DEV(lsk_check_combinadic(*six, h, n, d_reps, d_err, stream));
            DEV(lsk_sync(stream));
            DEV(lsk_d2h(&flag, d_err, sizeof(int)));
            DEV(lsk_h2d(d_err, &zero, sizeof(int)));
            if (!flag) { six->kind = LSK_INDEX_COMBINADIC; closed = 1; }
        } else if (es->product) {
            lsk_index pix = *six;
            pix.kind = LSK_INDEX_PRODUCT;
            pix.prod_sites = basis->number_sites; pix.prod_up = es->prod_up; pix.prod_dn = es->prod_dn;
            pix.prod_na = (int64_t)binom(basis->number_sites, es->prod_up);
            if (n == pix.prod_na * (int64_t)binom(basis->number_sites, es->prod_dn)) {
                DEV(lsk_check_product(pix, n, d_reps, d_err, stream));
                DEV(lsk_sync(stream));
                DEV(lsk_d2h(&flag, d_err, sizeof(int)));
                DEV(lsk_h2d(d_err, &zero, sizeof(int)));
                if (!flag) { *six = pix; closed = 1; }
            }
        }
        if (!closed) {
            part_state ps;
            memset(&ps, 0, sizeof(ps));
            ps.count = n;
            ps.d_reps = (uint64_t *)d_reps;
            if (build_search_index(&ps, L, stream) != 0) return -1;
            *d_table = ps.d_table;
            six->shift = ps.index.shift;
            six->table = ps.index.table;
        }
    }
    return 0;
}

static int cross_setup(ls_amd_cross *cx, ls_hs_operator const *op, ls_hs_basis const *target, void *stream) {
    ls_hs_basis const *src = op->basis;
    if (basis_device(src, &cx->src) != 0 || basis_device(target, &cx->dst) != 0) return -1;
    lsk_basis const dst = cx->dst;
    /* the adjoint's device groups: the diagonal terms are the group with flip mask 0 (row i of the target is not column i of the
     * source, so they take the projected path like every other group) */
    struct ls_amd_operator_ext const *ae = OEXT(cx->adj);
    int const nt = ae->n_diag + ae->n_off;
    cx->n_groups = ae->n_groups + (ae->n_diag > 0 ? 1 : 0);
    cx->is_real = ae->is_real;
    for (int k = 0; k < ae->n_diag; ++k) cx->tiny += hypot(ae->diag[k].v_re, ae->diag[k].v_im);
    for (int k = 0; k < ae->n_off; ++k) cx->tiny += hypot(ae->off[k].v_re, ae->off[k].v_im);
    cx->tiny *= 1e-13;
    if (cx->n_groups > 0) {
        lsk_term *terms = (lsk_term *)malloc(sizeof(lsk_term) * (size_t)nt);
        lsk_group *groups = (lsk_group *)calloc((size_t)cx->n_groups, sizeof(lsk_group));
        int w = 0;
        if (ae->n_diag > 0) {
            memcpy(terms, ae->diag, sizeof(lsk_term) * (size_t)ae->n_diag);
            groups[w].x = 0; groups[w].begin = 0; groups[w].end = ae->n_diag; groups[w].adj = -1; groups[w].fast = LSK_GROUP_GENERIC;
            ++w;
        }
        if (ae->n_off > 0) memcpy(terms + ae->n_diag, ae->off, sizeof(lsk_term) * (size_t)ae->n_off);
        for (int g = 0; g < ae->n_groups; ++g, ++w) {
            groups[w] = ae->groups[g];
            groups[w].begin += ae->n_diag; groups[w].end += ae->n_diag;
            groups[w].fast = LSK_GROUP_GENERIC; /* the kernel sums the terms of every group */
        }
        void *p = NULL, *q = NULL;
        int const bad = upload(&p, terms, sizeof(lsk_term) * (size_t)nt) != 0 || upload(&q, groups, sizeof(lsk_group) * (size_t)cx->n_groups) != 0;
        cx->d_terms = (lsk_term *)p; cx->d_groups = (lsk_group *)q;
        free(terms); free(groups);
        if (bad) return -1;
    }
    void *p = NULL;
    DEV(lsk_malloc(&p, 4 * sizeof(int)));
    cx->d_err = (int *)p;
    DEV(lsk_memset_async(cx->d_err, 0, 4 * sizeof(int), stream));
    DEV(lsk_malloc(&p, 8 * (size_t)(cx->n_dst > 0 ? cx->n_dst : 1)));
    cx->d_norms = (double *)p;
    DEV(lsk_norms(dst, cx->n_dst, cx->d_dst_reps, cx->d_norms, stream));
    /* the source look-up */
    if (sector_lookup("cross-sector", src, &cx->src, cx->d_src_reps, cx->n_src, cx->d_err, &cx->six, &cx->d_table, &cx->gtab, stream) != 0) return -1;
    /* counting pass: the packets that reach a source row (ls_amd_cross_nnz); whether some do not is left to the first apply */
    unsigned long long count = 0;
    if (cx->n_groups > 0 && cx->n_dst > 0 && cx->n_src > 0) {
        int zero = 0;
        DEV(cross_launch(cx, NULL, NULL, (unsigned long long *)(cx->d_err + 2), stream));
        DEV(lsk_sync(stream));
        DEV(lsk_d2h(&count, cx->d_err + 2, sizeof(count)));
        DEV(lsk_h2d(cx->d_err, &zero, sizeof(int)));
    }
    cx->nnz = (int64_t)count;
    return 0;
}

/* the body of both constructors (who: the name in the messages).  mode decides the rule that admits the pair of bases -- SAME: the
 * same generators, the operator covariant under them; RESTRICT: the target group inside the source group, covariant under the
 * target's generators; PROJECT: no rule, the kernel projects -- and, for PROJECT, the kernel. */
static int cross_create(char const *who, ls_amd_cross **out, ls_hs_operator const *op, ls_hs_basis const *target, ls_amd_dtype dtype, int mode,
                        uint64_t const *d_src_reps, int64_t n_src, uint64_t const *d_dst_reps, int64_t n_dst, void *stream) {
    if (out) *out = NULL;
    if (!out || !op || !target) return set_error("%s: NULL %s", who, !out ? "handle" : (!op ? "operator" : "target basis"));
    if (n_src < 0 || n_dst < 0 || (n_src > 0 && !d_src_reps) || (n_dst > 0 && !d_dst_reps))
        return set_error("%s: NULL representatives or a negative count", who);
    if (dtype != LS_AMD_F64 && dtype != LS_AMD_C128) return set_error("%s: unknown dtype %d", who, (int)dtype);
    if (mode == LS_AMD_CROSS_SAME) {
        if (ls_amd_operator_maps_sector_signed(op, target) != 0) return -1; /* (the plain rule where no basis has permutation signs) */
    } else if (mode == LS_AMD_CROSS_RESTRICT) {
        if (ls_amd_operator_maps_subgroup_sector(op, target) != 0) return -1;
    } else if (mode == LS_AMD_CROSS_PROJECT) {
        if (!reg_get(op)) return set_error("%s: unknown operator (ls_amd_adopt_operator first)", who);
        if (cross_groups_preconditions(op->basis, target) != 0) return -1;
    } else return set_error("%s: unknown mode %d (LS_AMD_CROSS_SAME, LS_AMD_CROSS_RESTRICT or LS_AMD_CROSS_PROJECT)", who, mode);
    ls_hs_operator *adj = ls_amd_operator_adjoint(op);
    if (!adj) return -1;
    if (dtype == LS_AMD_F64 && !(OEXT(adj)->is_real && cross_every_char_pm1(op->basis) && cross_every_char_pm1(target))) {
        ls_hs_destroy_operator(adj);
        return set_error("%s: f64 needs a real operator and +-1 characters on both bases (complex characters or "
                         "coefficients: use c128)", who);
    }
    ls_amd_cross *cx = (ls_amd_cross *)calloc(1, sizeof(*cx));
    cx->adj = adj;
    cx->mode = mode;
    cx->cplx = dtype == LS_AMD_C128;
    cx->d_src_reps = d_src_reps; cx->n_src = n_src;
    cx->d_dst_reps = d_dst_reps; cx->n_dst = n_dst;
    if (cross_setup(cx, op, target, stream) != 0) { ls_amd_cross_destroy(cx); return -1; }
    *out = cx;
    return 0;
}

int ls_amd_cross_create(ls_amd_cross **out, ls_hs_operator const *op, ls_hs_basis const *target, ls_amd_dtype dtype,
                        uint64_t const *d_src_reps, int64_t n_src, uint64_t const *d_dst_reps, int64_t n_dst, void *stream) {
    return cross_create("ls_amd_cross_create", out, op, target, dtype, LS_AMD_CROSS_SAME, d_src_reps, n_src, d_dst_reps, n_dst, stream);
}
int ls_amd_cross_create_groups(ls_amd_cross **out, ls_hs_operator const *op, ls_hs_basis const *target, ls_amd_dtype dtype, int mode,
                               uint64_t const *d_src_reps, int64_t n_src, uint64_t const *d_dst_reps, int64_t n_dst, void *stream) {
    return cross_create("ls_amd_cross_create_groups", out, op, target, dtype, mode, d_src_reps, n_src, d_dst_reps, n_dst, stream);
}

int ls_amd_cross_apply(ls_amd_cross *cx, void const *d_x, void *d_y, void *stream) {
    if (!cx || !d_y || (!d_x && cx && cx->n_src > 0)) return set_error("ls_amd_cross_apply: NULL %s", !cx ? "plan" : (!d_y ? "y" : "x"));
    if (cx->n_dst == 0) return 0;
    if (cx->n_groups == 0 || cx->n_src == 0) { /* A = 0, or nothing to read: y = 0 */
        DEV(lsk_memset_async(d_y, 0, (size_t)cx->n_dst * (cx->cplx ? 16 : 8), stream));
        return 0;
    }
    DEV(cross_launch(cx, d_x, d_y, NULL, stream));
    return 0;
}

/* ---- blocks of vectors (include/ls_amd.h: ls_amd_cross_apply_block; csrc/k_cross_blk.hip) ---- */
/* SAME and RESTRICT plans have one block kernel, k_cross_pull_blk.  A projecting plan has two paths: the column loop over
 * ls_amd_cross_apply (the default) and the block kernel k_cross_project_blk.  path: LS_AMD_CROSS_BLOCK_AUTO follows
 * LS_AMD_CROSS_PROJECT_BLOCK=columns|kernel, read at every call (unset: columns).  1: the column loop, 0: a block kernel, -1 with a
 * message: an unknown path or value */
static int cross_block_path_ok(char const *who, int path) {
    if (path != LS_AMD_CROSS_BLOCK_AUTO && path != LS_AMD_CROSS_BLOCK_COLUMNS && path != LS_AMD_CROSS_BLOCK_KERNEL)
        return set_error("%s: unknown path %d (LS_AMD_CROSS_BLOCK_AUTO, LS_AMD_CROSS_BLOCK_COLUMNS or LS_AMD_CROSS_BLOCK_KERNEL)", who, path);
    return 0;
}
static int cross_block_columns(char const *who, ls_amd_cross const *cx, int path) {
    if (cross_block_path_ok(who, path) != 0) return -1;
    if (cx->mode != LS_AMD_CROSS_PROJECT) return 0;
    if (path == LS_AMD_CROSS_BLOCK_AUTO) {
        char const *e = getenv("LS_AMD_CROSS_PROJECT_BLOCK");
        if (!e || !*e || strcmp(e, "columns") == 0) return 1;
        if (strcmp(e, "kernel") == 0) return 0;
        return set_error("%s: LS_AMD_CROSS_PROJECT_BLOCK=%s (columns or kernel)", who, e);
    }
    return path == LS_AMD_CROSS_BLOCK_COLUMNS;
}

char const *ls_amd_cross_block_kernel_name_path(ls_amd_cross const *cx, int path, int K) {
    char const *const who = "ls_amd_cross_block_kernel_name";
    if (cross_block_path_ok(who, path) != 0) return NULL; /* (the path and K before the plan: refusals that need no plan) */
    if (K < 1 || K > 64) { set_error("%s: K = %d is outside [1, 64]", who, K); return NULL; }
    if (!cx) { set_error("%s: NULL plan", who); return NULL; }
    int const columns = cross_block_columns(who, cx, path);
    if (columns < 0) return NULL;
    if (columns) return "columns";
    if (cx->mode == LS_AMD_CROSS_PROJECT)
        return cx->src.fermi || cx->dst.fermi ? lsk_cross_project_blk_fermi_kernel_name() : lsk_cross_project_blk_kernel_name();
    return cx->src.fermi ? lsk_cross_blk_fermi_kernel_name() : lsk_cross_blk_kernel_name();
}
char const *ls_amd_cross_block_kernel_name(ls_amd_cross const *cx, int K) {
    return ls_amd_cross_block_kernel_name_path(cx, LS_AMD_CROSS_BLOCK_AUTO, K);
}

int ls_amd_cross_apply_block(ls_amd_cross *cx, int K, void const *d_x, int64_t x_row, int64_t x_col, void *d_y, int64_t y_row, int64_t y_col,
                             void *stream) {
    return ls_amd_cross_apply_block_path(cx, LS_AMD_CROSS_BLOCK_AUTO, K, d_x, x_row, x_col, d_y, y_row, y_col, stream);
}

int ls_amd_cross_apply_block_path(ls_amd_cross *cx, int path, int K, void const *d_x, int64_t x_row, int64_t x_col, void *d_y, int64_t y_row,
                                  int64_t y_col, void *stream) {
    char const *const who = "ls_amd_cross_apply_block";
    if (cross_block_path_ok(who, path) != 0) return -1; /* (the path and K before the plan: refusals that need no plan) */
    if (K < 1 || K > 64) return set_error("%s: K = %d is outside [1, 64]", who, K);
    if (!cx) return set_error("%s: NULL plan", who);
    int const columns = cross_block_columns(who, cx, path);
    if (columns < 0) return -1;
    int64_t const ns = cx->n_src, nd = cx->n_dst;
    if (nd == 0) return 0;
    if (!d_y || (!d_x && ns > 0)) return set_error("%s: NULL %s", who, !d_y ? "Y" : "X");
    if (K == 1) { x_col = 0; y_col = 0; }
    if (block_strides(who, ns, K, x_row, x_col, "X") != 0 || block_strides(who, nd, K, y_row, y_col, "Y") != 0) return -1;
    size_t const w = cx->cplx ? 16 : 8;
    if (ns > 0 && block_overlap(w, ns, d_x, x_row, x_col, w, nd, d_y, y_row, y_col, K)) return set_error("%s: X and Y overlap", who);
    char *const y = (char *)d_y;
    if (cx->n_groups == 0 || ns == 0) { /* A = 0, or nothing to read: Y = 0 */
        if (y_col == 1 && y_row == K) { DEV(lsk_memset_async(y, 0, w * (size_t)nd * (size_t)K, stream)); return 0; }
        if (!cx->d_blk_cols) DEV(lsk_malloc(&cx->d_blk_cols, w * (size_t)(ns + nd)));
        char *const zero = (char *)cx->d_blk_cols + w * (size_t)ns; /* (the target scratch column, cleared, to copy from) */
        DEV(lsk_memset_async(zero, 0, w * (size_t)nd, stream));
        for (int k = 0; k < K; ++k) DEV(lsk_copy_strided(nd, (int)w, zero, 1, y + (size_t)k * (size_t)y_col * w, y_row, stream));
        return 0;
    }
    if (!columns) {
        lsk_gtab const gt = cx->gtab ? cx->gtab->tab : no_gtab();
        if (cx->mode == LS_AMD_CROSS_PROJECT) {
            DEV(lsk_cross_project_blk(cx->n_groups, cx->d_groups, cx->d_terms, cx->is_real, cx->src, cx->six, gt, cx->dst, cx->cplx, nd,
                                      cx->d_dst_reps, cx->d_norms, K, d_x, x_row, x_col, d_y, y_row, y_col, cx->tiny, cx->d_err, stream));
            return 0;
        }
        DEV(lsk_cross_pull_blk(cx->n_groups, cx->d_groups, cx->d_terms, cx->is_real, cx->src, cx->six, gt, cx->cplx, nd, cx->d_dst_reps,
                               cx->d_norms, K, d_x, x_row, x_col, d_y, y_row, y_col, cx->tiny, cx->d_err, stream));
        return 0;
    }
    /* the column loop: ls_amd_cross_apply through contiguous scratch columns that the plan owns */
    if ((x_row != 1 || y_row != 1) && !cx->d_blk_cols) DEV(lsk_malloc(&cx->d_blk_cols, w * (size_t)(ns + nd)));
    char *const col_x = (char *)cx->d_blk_cols, *const col_y = col_x ? col_x + w * (size_t)ns : NULL;
    for (int k = 0; k < K; ++k) {
        void const *xin = (char const *)d_x + (size_t)k * (size_t)x_col * w;
        void *const yk = y + (size_t)k * (size_t)y_col * w;
        void *const yout = y_row == 1 ? yk : (void *)col_y;
        if (x_row != 1) {
            DEV(lsk_copy_strided(ns, (int)w, xin, x_row, col_x, 1, stream));
            xin = col_x;
        }
        DEV(cross_launch(cx, xin, yout, NULL, stream));
        if (y_row != 1) DEV(lsk_copy_strided(nd, (int)w, col_y, 1, yk, y_row, stream));
    }
    return 0;
}

int ls_amd_cross_check(ls_amd_cross *cx, void *stream) {
    if (!cx) return set_error("ls_amd_cross_check: NULL plan");
    int flag = 0, zero = 0;
    DEV(lsk_sync(stream));
    DEV(lsk_d2h(&flag, cx->d_err, sizeof(int)));
    if (flag) {
        DEV(lsk_h2d(cx->d_err, &zero, sizeof(int)));
        return set_error("cross-sector: the adjoint of the operator generated a state with non-zero norm that is not in the source basis "
                         "(the operator does not map the source basis into the target basis, e.g. it changes the Hamming weight otherwise)");
    }
    return 0;
}

char const *ls_amd_cross_kernel_name(ls_amd_cross const *cx) {
    if (!cx) { set_error("ls_amd_cross_kernel_name: NULL plan"); return NULL; }
    if (cx->mode == LS_AMD_CROSS_PROJECT) return cx->src.fermi || cx->dst.fermi ? lsk_cross_project_fermi_kernel_name() : lsk_cross_project_kernel_name();
    return cx->src.fermi ? lsk_cross_fermi_kernel_name() : lsk_cross_kernel_name();
}
int64_t ls_amd_cross_nnz(ls_amd_cross const *cx) {
    if (!cx) { set_error("ls_amd_cross_nnz: NULL plan"); return -1; }
    return cx->nnz;
}

/* ---- the matrix of a plan as canonical CSR (include/ls_amd.h: ls_amd_cross_csr; csrc/k_csr.hip) ---- */
/* peak device bytes of an export: the raw and the final (column, value) arrays -- the final ones are no longer than the raw ones,
 * which hold ls_amd_cross_nnz entries -- three arrays of n_dst + 1 offsets, and the scratch of the scans (one partial sum per
 * 1024 elements at the least; bounded by 1 / 64 of the scanned array plus a page) */
int64_t ls_amd_cross_csr_bytes(ls_amd_cross const *cx) {
    if (!cx) { set_error("ls_amd_cross_csr_bytes: NULL plan"); return -1; }
    int64_t const entry = 8 + (cx->cplx ? 16 : 8), rows = 8 * (cx->n_dst + 1);
    return 2 * cx->nnz * entry + 3 * rows + rows / 64 + 4096;
}

void ls_amd_csr_free(ls_amd_csr *m) {
    if (!m) return;
    if (m->d_row_ptr) lsk_free(m->d_row_ptr);
    if (m->d_col) lsk_free(m->d_col);
    if (m->d_val) lsk_free(m->d_val);
    memset(m, 0, sizeof(*m));
}

static int cross_csr_run(ls_amd_cross *cx, ls_amd_csr *out, void **tmp, void *stream) {
    /* tmp[0] cnt, tmp[1] off (n_dst + 1 each), tmp[2] raw columns, tmp[3] raw values: freed by the caller */
    int64_t const n = cx->n_dst;
    size_t const vb = cx->cplx ? 16 : 8;
    int64_t raw = 0, nnz = 0;
    lsk_gtab const gt = cx->gtab ? cx->gtab->tab : no_gtab();
    int const empty = cx->n_groups == 0 || cx->n_src == 0 || n == 0;
    void *p = NULL;
    DEV(lsk_malloc(&p, 8 * (size_t)(n + 1)));
    out->d_row_ptr = (int64_t *)p;
    if (empty) { DEV(lsk_memset_async(out->d_row_ptr, 0, 8 * (size_t)(n + 1), stream)); }
    else {
        DEV(lsk_malloc(&tmp[0], 8 * (size_t)(n + 1)));
        DEV(lsk_malloc(&tmp[1], 8 * (size_t)(n + 1)));
        DEV(lsk_memset_async(tmp[0], 0, 8 * (size_t)(n + 1), stream)); /* (element n stays 0: the scan's last element is the sum) */
        DEV(lsk_cross_emit(cx->n_groups, cx->d_groups, cx->d_terms, cx->is_real, cx->src, cx->six, gt, cx->cplx, n, cx->d_dst_reps,
                           cx->d_norms, cx->tiny, NULL, (int64_t *)tmp[0], NULL, NULL, cx->d_err, stream));
        DEV(lsk_exclusive_scan_i64(n + 1, (int64_t const *)tmp[0], (int64_t *)tmp[1], stream));
        DEV(lsk_sync(stream));
        DEV(lsk_d2h(&raw, (int64_t *)tmp[1] + n, sizeof(raw)));
        if (raw != cx->nnz) return set_error("ls_amd_cross_csr: the counting pass found %lld packets, the plan %lld", (long long)raw, (long long)cx->nnz);
    }
    if (raw > 0) {
        DEV(lsk_malloc(&tmp[2], 8 * (size_t)raw));
        DEV(lsk_malloc(&tmp[3], vb * (size_t)raw));
        DEV(lsk_cross_emit(cx->n_groups, cx->d_groups, cx->d_terms, cx->is_real, cx->src, cx->six, gt, cx->cplx, n, cx->d_dst_reps,
                           cx->d_norms, cx->tiny, (int64_t const *)tmp[1], NULL, (int64_t *)tmp[2], tmp[3], cx->d_err, stream));
        DEV(lsk_csr_merge(cx->cplx, n, (int64_t const *)tmp[1], (int64_t *)tmp[2], tmp[3], (int64_t *)tmp[0], stream));
        DEV(lsk_exclusive_scan_i64(n + 1, (int64_t const *)tmp[0], out->d_row_ptr, stream));
        DEV(lsk_sync(stream));
        DEV(lsk_d2h(&nnz, out->d_row_ptr + n, sizeof(nnz)));
        if (nnz < 0 || nnz > raw) return set_error("ls_amd_cross_csr: %lld entries out of %lld packets", (long long)nnz, (long long)raw);
    } else if (!empty) DEV(lsk_memset_async(out->d_row_ptr, 0, 8 * (size_t)(n + 1), stream));
    /* (never NULL, so that a matrix without entries still has three arrays) */
    DEV(lsk_malloc(&p, 8 * (size_t)(nnz > 0 ? nnz : 1)));
    out->d_col = (int64_t *)p;
    DEV(lsk_malloc(&p, vb * (size_t)(nnz > 0 ? nnz : 1)));
    out->d_val = p;
    if (nnz > 0)
        DEV(lsk_csr_write(cx->cplx, n, (int64_t const *)tmp[1], (int64_t const *)tmp[2], tmp[3], out->d_row_ptr, out->d_col, out->d_val, stream));
    out->nnz = nnz;
    /* an image outside the source basis: the matrix is not the operator's (synchronises) */
    return ls_amd_cross_check(cx, stream);
}

int ls_amd_cross_csr(ls_amd_cross *cx, int64_t max_bytes, ls_amd_csr *out, void *stream) {
    if (out) memset(out, 0, sizeof(*out));
    if (!cx || !out) return set_error("ls_amd_cross_csr: NULL %s", !cx ? "plan" : "output");
    if (cx->mode == LS_AMD_CROSS_PROJECT)
        return set_error("ls_amd_cross_csr: a projecting plan (LS_AMD_CROSS_PROJECT, groups=\"project\") has no CSR export: the emitting "
                         "mode numbers a row's packets per flip group, and this plan sums them over the target group's elements as well");
    int64_t const need = ls_amd_cross_csr_bytes(cx);
    if (need > max_bytes)
        return set_error("ls_amd_cross_csr: the export needs up to %lld bytes of device memory (%lld rows, %lld packets), max_bytes is %lld",
                         (long long)need, (long long)cx->n_dst, (long long)cx->nnz, (long long)max_bytes);
    out->rows = cx->n_dst; out->cols = cx->n_src;
    out->dtype = cx->cplx ? LS_AMD_C128 : LS_AMD_F64;
    void *tmp[4] = {NULL, NULL, NULL, NULL};
    int const rc = cross_csr_run(cx, out, tmp, stream);
    if (rc != 0) (void)lsk_sync(stream); /* nothing in flight may still write what is freed now */
    for (int k = 0; k < 4; ++k) if (tmp[k]) lsk_free(tmp[k]);
    if (rc != 0) ls_amd_csr_free(out);
    return rc;
}

/* ============================================================================================ */
/* sector-state expansion (include/ls_amd.h: ls_amd_expand; csrc/k_expand.hip)     */
/* ============================================================================================ */
#define EXPAND_MAX_BLOCKS LSK_EXPAND_FERMI_TAB /* fixed weight: n_A = 0 .. 64; the spinful product basis: (n_up, n_dn), 0 .. 32 each */
typedef struct expand_layout {
    int L, weight, n_a, n_b, split, nb;
    int kind, half, au, ad, n_up, n_dn; /* fermionic plans: LSK_EXPAND_FERMI_*; PRODUCT: L, the up / down modes of A, (N_up, N_down) */
    int na[EXPAND_MAX_BLOCKS];          /* n_A of the block (PRODUCT: n_up + n_dn; -1 without a fixed number) */
    int nd[EXPAND_MAX_BLOCKS];          /* PRODUCT: n_dn of the block; -1 on every other layout of a fermionic plan */
    int64_t rows[EXPAND_MAX_BLOCKS], cols[EXPAND_MAX_BLOCKS], off[EXPAND_MAX_BLOCKS], total;
} expand_layout;

/* the layout of a basis of L-bit words with Hamming weight w (-1: every word): one block per n_A, or one 2^|A| x 2^|B| block.
 * `who` / `noun` word the refusals of the spin entry points ("sites") and of the fermionic ones ("modes"). */
static int expand_layout_weight(expand_layout *lay, char const *who, char const *noun, int L, int w, uint64_t mask_a) {
    uint64_t const sites = L >= 64 ? ~0ULL : ((1ULL << L) - 1);
    if (mask_a & ~sites) return set_error("%s: the subsystem mask 0x%llx has bits outside the %d %s", who, (unsigned long long)mask_a, L, noun);
    if (w >= LSK_BINOM_K) return set_error("%s: Hamming weight %d is beyond the binomial table (%d)", who, w, LSK_BINOM_K - 1);
    memset(lay, 0, sizeof(*lay));
    lay->L = L; lay->weight = w;
    lay->n_a = __builtin_popcountll(mask_a);
    lay->n_b = L - lay->n_a;
    if (mask_a == (lay->n_a >= 64 ? ~0ULL : ((1ULL << lay->n_a) - 1))) lay->split = LSK_SPLIT_LOW;       /* (the empty A too) */
    else if (mask_a == (sites & ~((1ULL << lay->n_b) - 1))) lay->split = LSK_SPLIT_HIGH;
    else lay->split = LSK_SPLIT_GATHER;
    if (w < 0) {
        if (L > 40) return set_error("%s: %d %s without a fixed Hamming weight expand to 2^%d elements", who, L, noun, L);
        lay->kind = LSK_EXPAND_FERMI_ALL;
        lay->nb = 1;
        lay->na[0] = -1; lay->nd[0] = -1;
        lay->rows[0] = (int64_t)1 << lay->n_a; lay->cols[0] = (int64_t)1 << lay->n_b;
        lay->total = (int64_t)1 << L;
        return 0;
    }
    lay->kind = LSK_EXPAND_FERMI_FIXED;
    for (int na = 0; na <= lay->n_a && na <= w; ++na) {
        uint64_t const r = binom(lay->n_a, na), c = binom(lay->n_b, w - na);
        if (r == 0 || c == 0) continue; /* empty blocks are omitted */
        long double const sz = (long double)r * (long double)c;
        if (sz + (long double)lay->total > 4.0e18L) return set_error("%s: the expansion has more than 2^62 elements", who);
        int const i = lay->nb++;
        lay->na[i] = na; lay->nd[i] = -1; lay->rows[i] = (int64_t)r; lay->cols[i] = (int64_t)c; lay->off[i] = lay->total;
        lay->total += (int64_t)(r * c);
    }
    return 0;
}

/* the block table of a bipartition: host only.  The refusals of ls_amd_expand_create that need no device live here. */
static int expand_layout_of(ls_hs_basis const *basis, uint64_t mask_a, expand_layout *lay) {
    if (!basis) return set_error("ls_amd_expand: NULL basis");
    if (basis->particle_type != LS_HS_SPIN)
        return set_error("ls_amd_expand: fermionic bases are not supported here -- the partial trace of fermions needs the mode-ordering signs of "
                         "moving the modes of the subsystem in front of the others, which ls_amd_fermi_expand_create carries");
    struct ls_amd_basis_ext const *e = BEXT(basis);
    return expand_layout_weight(lay, "ls_amd_expand", "sites", e->nbits, e->hamming_weight, mask_a);
}

/* ... of a fermionic basis (ls_amd_fermi_expand_create).  Spinless bases, and spinful ones with number_up unset (spinless over their
 * 2 L modes), take the layout above over their modes; the spinful (N, N_up) product basis one block per (n_up, n_dn) of the up and
 * down modes of A, ordered lexicographically: rows C(|A_up|, n_up) C(|A_dn|, n_dn), columns C(L - |A_up|, N_up - n_up)
 * C(L - |A_dn|, N_dn - n_dn) (include/ls_amd.h). */
static int fermi_expand_layout_of(ls_hs_basis const *basis, uint64_t mask_a, expand_layout *lay) {
    char const *who = "ls_amd_fermi_expand";
    if (!basis) return set_error("%s: NULL basis", who);
    if (basis->particle_type == LS_HS_SPIN)
        return set_error("%s: a spin-1/2 basis has no mode-ordering signs: it is expanded by ls_amd_expand_create (SectorExpansion)", who);
    struct ls_amd_basis_ext const *e = BEXT(basis);
    if (basis->spin_inversion != 0) return set_error("%s: a fermionic basis has no spin inversion", who);
    if (!e->product) return expand_layout_weight(lay, who, "modes", e->nbits, e->hamming_weight, mask_a);
    int const L = basis->number_sites, M = 2 * L; /* L <= 32 */
    uint64_t const modes = M >= 64 ? ~0ULL : ((1ULL << M) - 1), low = (1ULL << L) - 1;
    if (mask_a & ~modes) return set_error("%s: the subsystem mask 0x%llx has bits outside the %d modes", who, (unsigned long long)mask_a, M);
    memset(lay, 0, sizeof(*lay));
    lay->L = M; lay->weight = -1;
    lay->kind = LSK_EXPAND_FERMI_PRODUCT;
    lay->half = L; lay->n_up = e->prod_up; lay->n_dn = e->prod_dn;
    lay->n_a = __builtin_popcountll(mask_a);
    lay->n_b = M - lay->n_a;
    lay->au = __builtin_popcountll(mask_a & low); lay->ad = lay->n_a - lay->au;
    if (mask_a == (lay->n_a >= 64 ? ~0ULL : ((1ULL << lay->n_a) - 1))) lay->split = LSK_SPLIT_LOW;
    else if (mask_a == (modes & ~((1ULL << lay->n_b) - 1))) lay->split = LSK_SPLIT_HIGH;
    else lay->split = LSK_SPLIT_GATHER;
    for (int nu = 0; nu <= lay->au && nu <= lay->n_up; ++nu)
        for (int nd = 0; nd <= lay->ad && nd <= lay->n_dn; ++nd) {
            long double const r = (long double)binom(lay->au, nu) * (long double)binom(lay->ad, nd);
            long double const c = (long double)binom(L - lay->au, lay->n_up - nu) * (long double)binom(L - lay->ad, lay->n_dn - nd);
            if (r == 0 || c == 0) continue; /* empty blocks are omitted */
            if (r * c + (long double)lay->total > 4.0e18L) return set_error("%s: the expansion has more than 2^62 elements", who);
            int const i = lay->nb++;
            lay->na[i] = nu + nd; lay->nd[i] = nd; lay->rows[i] = (int64_t)r; lay->cols[i] = (int64_t)c; lay->off[i] = lay->total;
            lay->total += (int64_t)r * (int64_t)c;
        }
    return 0;
}

int ls_amd_test_expand_layout(ls_hs_basis const *basis, uint64_t subsystem_mask, int capacity, int *n_a, int64_t *rows, int64_t *cols,
                              int64_t *offsets, int64_t *total) {
    expand_layout lay;
    if (expand_layout_of(basis, subsystem_mask, &lay) != 0) return -1;
    for (int i = 0; i < lay.nb && i < capacity; ++i) {
        if (n_a) n_a[i] = lay.na[i];
        if (rows) rows[i] = lay.rows[i];
        if (cols) cols[i] = lay.cols[i];
        if (offsets) offsets[i] = lay.off[i];
    }
    if (total) *total = lay.total;
    return lay.nb;
}

int ls_amd_test_fermi_expand_layout(ls_hs_basis const *basis, uint64_t mode_mask, int capacity, int *n_up, int *n_dn, int64_t *rows,
                                    int64_t *cols, int64_t *offsets, int64_t *total) {
    expand_layout lay;
    if (fermi_expand_layout_of(basis, mode_mask, &lay) != 0) return -1;
    for (int i = 0; i < lay.nb && i < capacity; ++i) {
        if (n_up) n_up[i] = lay.nd[i] < 0 ? lay.na[i] : lay.na[i] - lay.nd[i];
        if (n_dn) n_dn[i] = lay.nd[i];
        if (rows) rows[i] = lay.rows[i];
        if (cols) cols[i] = lay.cols[i];
        if (offsets) offsets[i] = lay.off[i];
    }
    if (total) *total = lay.total;
    return lay.nb;
}

/* test hook (no device): sigma(state) = +-1 of the bipartition A = mode_mask_a | the other modes of a word of `modes` modes, by the
 * device code's host run (fermi_split_parity, lsk_fermi.hpp); 0 on bad arguments */
int ls_amd_test_fermi_split_parity(uint64_t mode_mask_a, int modes, uint64_t state) {
    if (modes < 1 || modes > 64) return 0;
    uint64_t const all = modes >= 64 ? ~0ULL : ((1ULL << modes) - 1);
    if ((mode_mask_a & ~all) || (state & ~all)) return 0;
    return lsk_test_fermi_split_parity(state, mode_mask_a, all & ~mode_mask_a) ? -1 : 1;
}

struct ls_amd_expand {
    lsk_basis bs;             /* device tables owned by the basis */
    expand_layout lay;
    uint64_t mask_a;
    int pm1;                  /* every character is +-1: f64 allowed */
    int fermi;                /* a plan of ls_amd_fermi_expand_create: k_expand_push_fermi */
    double *d_norms;          /* owned: n(r) of every row */
    int64_t *d_tab;           /* owned: the block table by n_A (lsk_expand.tab) or by (n_up, n_dn) (lsk_expand_fermi.tab); NULL without a fixed weight */
    int *d_err;               /* owned */
    uint64_t const *d_reps;   /* borrowed */
    uint64_t const *d_binom;
    int64_t n;
};

void ls_amd_expand_destroy(ls_amd_expand *ex) {
    if (!ex) return;
    if (ex->d_norms) lsk_free(ex->d_norms);
    if (ex->d_tab) lsk_free(ex->d_tab);
    if (ex->d_err) lsk_free(ex->d_err);
    free(ex);
}

static int expand_setup(ls_amd_expand *ex, ls_hs_basis const *basis, void *stream) {
    if (basis_device(basis, &ex->bs) != 0) return -1;
    ex->pm1 = cross_every_char_pm1(basis);
    if (device_binom(&ex->d_binom) != 0) return -1;
    void *p = NULL;
    DEV(lsk_malloc(&p, 4 * sizeof(int)));
    ex->d_err = (int *)p;
    DEV(lsk_memset_async(ex->d_err, 0, 4 * sizeof(int), stream));
    DEV(lsk_malloc(&p, 8 * (size_t)(ex->n > 0 ? ex->n : 1)));
    ex->d_norms = (double *)p;
    /* the stabiliser norms, by the routine the matvec and cross-sector plans use (an unprojected basis: the identity alone, n = 1) */
    DEV(lsk_norms(ex->bs, ex->n, ex->d_reps, ex->d_norms, stream));
    if (ex->fermi && ex->lay.kind == LSK_EXPAND_FERMI_PRODUCT) {
        int64_t tab[LSK_EXPAND_FERMI_TAB];
        for (int i = 0; i < LSK_EXPAND_FERMI_TAB; ++i) tab[i] = -1;
        for (int i = 0; i < ex->lay.nb; ++i) tab[(ex->lay.na[i] - ex->lay.nd[i]) * (ex->lay.ad + 1) + ex->lay.nd[i]] = ex->lay.off[i];
        if (upload(&p, tab, sizeof(tab)) != 0) return -1;
        ex->d_tab = (int64_t *)p;
    } else if (ex->lay.weight >= 0) {
        int64_t tab[2 * LSK_EXPAND_MAX_NA];
        for (int i = 0; i < LSK_EXPAND_MAX_NA; ++i) { tab[i] = -1; tab[LSK_EXPAND_MAX_NA + i] = 0; }
        for (int i = 0; i < ex->lay.nb; ++i) { tab[ex->lay.na[i]] = ex->lay.off[i]; tab[LSK_EXPAND_MAX_NA + ex->lay.na[i]] = ex->lay.cols[i]; }
        if (upload(&p, tab, sizeof(tab)) != 0) return -1;
        ex->d_tab = (int64_t *)p;
    }
    DEV(lsk_sync(stream));
    return 0;
}

int ls_amd_expand_create(ls_amd_expand **out, ls_hs_basis const *basis, uint64_t const *d_reps, int64_t n, uint64_t subsystem_mask,
                         void *stream) {
    if (out) *out = NULL;
    if (!out || !basis) return set_error("ls_amd_expand_create: NULL %s", !out ? "handle" : "basis");
    if (n < 0 || (n > 0 && !d_reps)) return set_error("ls_amd_expand_create: NULL representatives or a negative count");
    expand_layout lay;
    if (expand_layout_of(basis, subsystem_mask, &lay) != 0) return -1;
    ls_amd_expand *ex = (ls_amd_expand *)calloc(1, sizeof(*ex));
    ex->lay = lay;
    ex->mask_a = subsystem_mask;
    ex->d_reps = d_reps; ex->n = n;
    if (expand_setup(ex, basis, stream) != 0) { ls_amd_expand_destroy(ex); return -1; }
    *out = ex;
    return 0;
}

int ls_amd_fermi_expand_create(ls_amd_expand **out, ls_hs_basis const *basis, uint64_t const *d_reps, int64_t n, uint64_t mode_mask,
                               void *stream) {
    if (out) *out = NULL;
    if (!out || !basis) return set_error("ls_amd_fermi_expand_create: NULL %s", !out ? "handle" : "basis");
    if (n < 0 || (n > 0 && !d_reps)) return set_error("ls_amd_fermi_expand_create: NULL representatives or a negative count");
    ls_amd_expand *ex = (ls_amd_expand *)calloc(1, sizeof(*ex));
    if (fermi_expand_layout_of(basis, mode_mask, &ex->lay) != 0) { free(ex); return -1; }
    ex->fermi = 1;
    ex->mask_a = mode_mask;
    ex->d_reps = d_reps; ex->n = n;
    if (expand_setup(ex, basis, stream) != 0) { ls_amd_expand_destroy(ex); return -1; }
    *out = ex;
    return 0;
}

int ls_amd_expand_num_blocks(ls_amd_expand const *ex) {
    if (!ex) return set_error("ls_amd_expand_num_blocks: NULL plan");
    return ex->lay.nb;
}
int ls_amd_expand_block(ls_amd_expand const *ex, int i, int *n_a, int64_t *rows, int64_t *cols, int64_t *offset) {
    if (!ex) return set_error("ls_amd_expand_block: NULL plan");
    if (i < 0 || i >= ex->lay.nb) return set_error("ls_amd_expand_block: block %d of %d", i, ex->lay.nb);
    if (n_a) *n_a = ex->lay.na[i];
    if (rows) *rows = ex->lay.rows[i];
    if (cols) *cols = ex->lay.cols[i];
    if (offset) *offset = ex->lay.off[i];
    return 0;
}
int ls_amd_fermi_expand_block(ls_amd_expand const *ex, int i, int *n_up, int *n_dn, int64_t *rows, int64_t *cols, int64_t *offset) {
    if (!ex) return set_error("ls_amd_fermi_expand_block: NULL plan");
    if (!ex->fermi) return set_error("ls_amd_fermi_expand_block: the plan of a spin basis (ls_amd_expand_block)");
    if (i < 0 || i >= ex->lay.nb) return set_error("ls_amd_fermi_expand_block: block %d of %d", i, ex->lay.nb);
    if (n_up) *n_up = ex->lay.nd[i] < 0 ? ex->lay.na[i] : ex->lay.na[i] - ex->lay.nd[i];
    if (n_dn) *n_dn = ex->lay.nd[i];
    if (rows) *rows = ex->lay.rows[i];
    if (cols) *cols = ex->lay.cols[i];
    if (offset) *offset = ex->lay.off[i];
    return 0;
}
int64_t ls_amd_expand_total(ls_amd_expand const *ex) {
    if (!ex) { set_error("ls_amd_expand_total: NULL plan"); return -1; }
    return ex->lay.total;
}

int ls_amd_expand_apply(ls_amd_expand *ex, ls_amd_dtype dtype, void const *d_psi, void *d_out, int first_block, int num_blocks, void *stream) {
    if (!ex || !d_out || (!d_psi && ex && ex->n > 0)) return set_error("ls_amd_expand_apply: NULL %s", !ex ? "plan" : (!d_out ? "out" : "psi"));
    if (dtype != LS_AMD_F64 && dtype != LS_AMD_C128) return set_error("ls_amd_expand_apply: unknown dtype %d", (int)dtype);
    if (dtype == LS_AMD_F64 && !ex->pm1)
        return set_error("ls_amd_expand_apply: f64 needs +-1 characters (complex characters: use c128)");
    if (first_block < 0 || num_blocks < 0 || first_block + num_blocks > ex->lay.nb)
        return set_error("ls_amd_expand_apply: blocks [%d, %d) of %d", first_block, first_block + num_blocks, ex->lay.nb);
    if (num_blocks == 0) return 0;
    int const cplx = dtype == LS_AMD_C128, last = first_block + num_blocks - 1;
    size_t const elt = cplx ? 16 : 8;
    int64_t const begin = ex->lay.off[first_block], end = ex->lay.off[last] + ex->lay.rows[last] * ex->lay.cols[last];
    /* the selected blocks lie one after another: one clear, then the scatter assigns what the orbits reach */
    DEV(lsk_memset_async((char *)d_out + (size_t)begin * elt, 0, (size_t)(end - begin) * elt, stream));
    if (ex->n == 0) return 0;
    if (ex->fermi) {
        expand_layout const *lay = &ex->lay;
        lsk_expand_fermi f;
        memset(&f, 0, sizeof(f));
        f.mask_a = ex->mask_a; f.mask_b = ex->bs.site_mask & ~ex->mask_a;
        f.n_a = lay->n_a; f.n_b = lay->n_b;
        f.split = lay->split;
        f.kind = lay->kind;
        f.half = lay->half; f.au = lay->au; f.ad = lay->ad; f.n_up = lay->n_up; f.n_dn = lay->n_dn;
        if (lay->kind == LSK_EXPAND_FERMI_PRODUCT) { /* lexicographic in (n_up, n_dn) = ascending in the key */
            f.lo = (lay->na[first_block] - lay->nd[first_block]) * (lay->ad + 1) + lay->nd[first_block];
            f.hi = (lay->na[last] - lay->nd[last]) * (lay->ad + 1) + lay->nd[last];
        } else { f.lo = lay->na[first_block]; f.hi = lay->na[last]; }
        f.tab = ex->d_tab;
        f.cols = lay->cols[0];
        DEV(lsk_expand_fermi_push(ex->bs, f, ex->d_binom, cplx, ex->n, ex->d_reps, ex->d_norms, d_psi, d_out, ex->d_err, stream));
        return 0;
    }
    lsk_expand k;
    memset(&k, 0, sizeof(k));
    k.mask_a = ex->mask_a;
    k.n_a = ex->lay.n_a; k.n_b = ex->lay.n_b;
    k.split = ex->lay.split;
    k.na_lo = ex->lay.na[first_block]; k.na_hi = ex->lay.na[last];
    k.tab = ex->d_tab;
    k.cols = ex->lay.cols[0];
    DEV(lsk_expand_push(ex->bs, k, ex->d_binom, cplx, ex->n, ex->d_reps, ex->d_norms, d_psi, d_out, ex->d_err, stream));
    return 0;
}

int ls_amd_expand_check(ls_amd_expand *ex, void *stream) {
    if (!ex) return set_error("ls_amd_expand_check: NULL plan");
    int flag = 0, zero = 0;
    DEV(lsk_sync(stream));
    DEV(lsk_d2h(&flag, ex->d_err, sizeof(int)));
    if (flag) {
        DEV(lsk_h2d(ex->d_err, &zero, sizeof(int)));
        if (ex->fermi)
            return set_error("sector expansion: a representative or one of its images is not a state of the basis (another particle number "
                             "of the word or of a species, or bits above the %d modes): the array does not belong to this basis", ex->lay.L);
        return set_error("sector expansion: a representative or one of its images is not a state of the basis (another Hamming weight, "
                         "or bits above the %d sites): the array does not belong to this basis", ex->lay.L);
    }
    return 0;
}

char const *ls_amd_expand_kernel_name(ls_amd_expand const *ex) {
    if (!ex) { set_error("ls_amd_expand_kernel_name: NULL plan"); return NULL; }
    return ex->fermi ? lsk_expand_fermi_kernel_name() : lsk_expand_kernel_name();
}

/* ============================================================================================ */
/* projection into a sector (include/ls_amd.h: ls_amd_project; csrc/k_project_t.hpp) */
/* ============================================================================================ */
/* the layout of the full-basis vector -- the one block of the expansion with A = every site / mode -- and F; host only: the refusals
 * of ls_amd_project_create that need no device live here */
static int project_layout_of(ls_hs_basis const *basis, lsk_project *pj) {
    char const *who = "ls_amd_project";
    if (!basis) return set_error("%s: NULL basis", who);
    struct ls_amd_basis_ext const *e = BEXT(basis);
    int const spin = basis->particle_type == LS_HS_SPIN;
    if (!spin && basis->spin_inversion != 0) return set_error("%s: a fermionic basis has no spin inversion", who);
    memset(pj, 0, sizeof(*pj));
    if (!spin && e->product) {
        int const L = basis->number_sites; /* L <= 32 */
        long double const f = (long double)binom(L, e->prod_up) * (long double)binom(L, e->prod_dn);
        if (f > 4.0e18L) return set_error("%s: the full basis has more than 2^62 states", who);
        pj->kind = LSK_PROJECT_PRODUCT;
        pj->half = L; pj->n_up = e->prod_up; pj->n_dn = e->prod_dn;
        pj->n_low = (int64_t)binom(L, e->prod_up);
        pj->full = pj->n_low * (int64_t)binom(L, e->prod_dn);
        return 0;
    }
    expand_layout lay; /* every site in A: one block of one column, F rows */
    uint64_t const all = e->nbits >= 64 ? ~0ULL : ((1ULL << e->nbits) - 1);
    if (expand_layout_weight(&lay, who, spin ? "sites" : "modes", e->nbits, e->hamming_weight, all) != 0) return -1;
    pj->kind = e->hamming_weight < 0 ? LSK_PROJECT_ALL : LSK_PROJECT_FIXED;
    pj->full = lay.total;
    return 0;
}

int64_t ls_amd_test_project_full_size(ls_hs_basis const *basis) {
    lsk_project pj;
    if (project_layout_of(basis, &pj) != 0) return -1;
    return pj.full;
}

static int64_t project_host_rank(uint64_t s) { /* combinadic rank among the words of equal popcount (positions < 64, k < LSK_BINOM_K) */
    int64_t idx = 0;
    for (int k = 1; s; ++k, s &= s - 1) idx += (int64_t)binom(__builtin_ctzll(s), k);
    return idx;
}

/* host only: index(state) of the kernels -- the position of `state` among the ascending states of the basis without symmetries --
 * or -1 with a message that names why the word is no state of the basis */
int64_t ls_amd_test_project_state_index(ls_hs_basis const *basis, uint64_t state) {
    lsk_project pj;
    if (project_layout_of(basis, &pj) != 0) return -1;
    struct ls_amd_basis_ext const *e = BEXT(basis);
    int const spin = basis->particle_type == LS_HS_SPIN;
    uint64_t const all = e->nbits >= 64 ? ~0ULL : ((1ULL << e->nbits) - 1);
    if (state & ~all) {
        set_error("ls_amd_project: the state 0x%llx has bits above the %d %s of the basis", (unsigned long long)state, e->nbits, spin ? "sites" : "modes");
        return -1;
    }
    if (pj.kind == LSK_PROJECT_PRODUCT) {
        uint64_t const lo = state & ((1ULL << pj.half) - 1), hi = state >> pj.half;
        int const nu = __builtin_popcountll(lo), nd = __builtin_popcountll(hi);
        if (nu != pj.n_up || nd != pj.n_dn) {
            set_error("ls_amd_project: the state 0x%llx has the particle numbers (%d up, %d down), the basis (%d up, %d down)",
                      (unsigned long long)state, nu, nd, pj.n_up, pj.n_dn);
            return -1;
        }
        return project_host_rank(hi) * pj.n_low + project_host_rank(lo);
    }
    if (pj.kind == LSK_PROJECT_FIXED) {
        int const w = __builtin_popcountll(state);
        if (w != e->hamming_weight) {
            set_error("ls_amd_project: the state 0x%llx has %s %d, the basis %d", (unsigned long long)state,
                      spin ? "Hamming weight" : "particle number", w, e->hamming_weight);
            return -1;
        }
        return project_host_rank(state);
    }
    return (int64_t)state;
}

struct ls_amd_project {
    lsk_basis bs;             /* device tables owned by the basis */
    lsk_project pj;
    int pm1;                  /* every character is +-1: f64 allowed */
    int fermi;                /* a fermionic basis: k_project_pull_fermi */
    int modes;
    double *d_norms;          /* owned: n(r) of every row */
    int *d_err;               /* owned */
    uint64_t const *d_reps;   /* borrowed */
    uint64_t const *d_binom;
    int64_t n;
};

void ls_amd_project_destroy(ls_amd_project *p) {
    if (!p) return;
    if (p->d_norms) lsk_free(p->d_norms);
    if (p->d_err) lsk_free(p->d_err);
    free(p);
}

static int project_setup(ls_amd_project *p, ls_hs_basis const *basis, void *stream) {
    if (basis_device(basis, &p->bs) != 0) return -1;
    p->pm1 = cross_every_char_pm1(basis);
    if (device_binom(&p->d_binom) != 0) return -1;
    void *q = NULL;
    DEV(lsk_malloc(&q, 4 * sizeof(int)));
    p->d_err = (int *)q;
    DEV(lsk_memset_async(p->d_err, 0, 4 * sizeof(int), stream));
    DEV(lsk_malloc(&q, 8 * (size_t)(p->n > 0 ? p->n : 1)));
    p->d_norms = (double *)q;
    /* the stabiliser norms, by the routine the expansion and the cross-sector plans use */
    DEV(lsk_norms(p->bs, p->n, p->d_reps, p->d_norms, stream));
    DEV(lsk_sync(stream));
    return 0;
}

int ls_amd_project_create(ls_amd_project **out, ls_hs_basis const *basis, uint64_t const *d_reps, int64_t n, void *stream) {
    if (out) *out = NULL;
    if (!out || !basis) return set_error("ls_amd_project_create: NULL %s", !out ? "handle" : "basis");
    if (n < 0 || (n > 0 && !d_reps)) return set_error("ls_amd_project_create: NULL representatives or a negative count");
    lsk_project pj;
    if (project_layout_of(basis, &pj) != 0) return -1;
    ls_amd_project *p = (ls_amd_project *)calloc(1, sizeof(*p));
    if (!p) return set_error("ls_amd_project_create: out of host memory");
    p->pj = pj;
    p->fermi = basis->particle_type != LS_HS_SPIN;
    p->modes = BEXT(basis)->nbits;
    p->d_reps = d_reps; p->n = n;
    if (project_setup(p, basis, stream) != 0) { ls_amd_project_destroy(p); return -1; }
    *out = p;
    return 0;
}

int64_t ls_amd_project_full_size(ls_amd_project const *p) {
    if (!p) { set_error("ls_amd_project_full_size: NULL plan"); return -1; }
    return p->pj.full;
}

int ls_amd_project_apply(ls_amd_project *p, ls_amd_dtype dtype, int K, void const *d_phi, int64_t phi_s0, int64_t phi_s1, void *d_out,
                         int64_t out_s0, int64_t out_s1, void *stream) {
    if (!p || !d_phi || (!d_out && p && p->n > 0)) return set_error("ls_amd_project_apply: NULL %s", !p ? "plan" : (!d_phi ? "phi" : "out"));
    if (dtype != LS_AMD_F64 && dtype != LS_AMD_C128) return set_error("ls_amd_project_apply: unknown dtype %d", (int)dtype);
    if (dtype == LS_AMD_F64 && !p->pm1)
        return set_error("ls_amd_project_apply: f64 needs +-1 characters (complex characters: use c128)");
    if (K < 1 || K > LSK_PROJECT_MAX_K) return set_error("ls_amd_project_apply: K = %d columns, outside [1, %d]", K, LSK_PROJECT_MAX_K);
    if (phi_s0 < 0 || phi_s1 < 0 || out_s0 < 0 || out_s1 < 0) return set_error("ls_amd_project_apply: negative strides");
    if (p->n == 0) return 0;
    lsk_project pj = p->pj;
    pj.K = K;
    pj.phi_s0 = phi_s0; pj.phi_s1 = phi_s1; pj.out_s0 = out_s0; pj.out_s1 = out_s1;
    int const cplx = dtype == LS_AMD_C128;
    if (p->fermi) DEV(lsk_project_pull_fermi(p->bs, pj, p->d_binom, cplx, p->n, p->d_reps, p->d_norms, d_phi, d_out, p->d_err, stream));
    else DEV(lsk_project_pull(p->bs, pj, p->d_binom, cplx, p->n, p->d_reps, p->d_norms, d_phi, d_out, p->d_err, stream));
    return 0;
}

int ls_amd_project_check(ls_amd_project *p, void *stream) {
    if (!p) return set_error("ls_amd_project_check: NULL plan");
    int flag = 0, zero = 0;
    DEV(lsk_sync(stream));
    DEV(lsk_d2h(&flag, p->d_err, sizeof(int)));
    if (flag) {
        DEV(lsk_h2d(p->d_err, &zero, sizeof(int)));
        if (p->fermi)
            return set_error("sector projection: a representative or one of its images is not in the basis (another particle number of the "
                             "word or of a species, or bits above the %d modes): the array does not belong to this basis", p->modes);
        return set_error("sector projection: a representative or one of its images is not in the basis (another Hamming weight, or bits "
                         "above the %d sites): the array does not belong to this basis", p->modes);
    }
    return 0;
}

char const *ls_amd_project_kernel_name(ls_amd_project const *p) {
    if (!p) { set_error("ls_amd_project_kernel_name: NULL plan"); return NULL; }
    return p->fermi ? lsk_project_fermi_kernel_name() : lsk_project_kernel_name();
}

/* ============================================================================================ */
/* amplitudes on product states and orbit images (include/ls_amd.h: ls_amd_amp; csrc/k_amplitude_t.hpp) */
/* ============================================================================================ */
/* which words are states of the basis without symmetries (the membership of lsk_project: no layout, so none of its size limits);
 * host only: the refusals of ls_amd_amp_create that need no device live here */
static int amp_membership_of(char const *who, ls_hs_basis const *basis, lsk_project *pj) {
    if (!basis) return set_error("%s: NULL basis", who);
    if (!reg_get(basis)) return set_error("%s: the basis is not built by this library (ls_amd_adopt_basis first)", who);
    struct ls_amd_basis_ext const *e = BEXT(basis);
    int const spin = basis->particle_type == LS_HS_SPIN;
    if (!spin && basis->spin_inversion != 0) return set_error("%s: a fermionic basis has no spin inversion", who);
    if (e->fermi && e->nbits > 60)
        return set_error("%s: projected fermionic bases of more than 60 modes are not supported (%d modes: the static index table does "
                         "not fit, as for their matvec and cross-sector plans)", who, e->nbits);
    memset(pj, 0, sizeof(*pj));
    if (!spin && e->product) {
        pj->kind = LSK_PROJECT_PRODUCT;
        pj->half = basis->number_sites; pj->n_up = e->prod_up; pj->n_dn = e->prod_dn;
    } else pj->kind = e->hamming_weight < 0 ? LSK_PROJECT_ALL : LSK_PROJECT_FIXED;
    return 0;
}

/* the effective group: the permutation elements, each followed by its product with the global inversion on a spin basis that has one
 * (element 2 p = permutation p, 2 p + 1 = permutation p then ^ site_mask: the order of k_orbit_image) */
static int amp_num_elements(ls_hs_basis const *basis) {
    return BEXT(basis)->order * (basis->particle_type == LS_HS_SPIN && basis->spin_inversion != 0 ? 2 : 1);
}

uint64_t ls_amd_test_orbit_state(ls_hs_basis const *basis, uint64_t state, int element, int *ok) {
    lsk_project pj;
    if (ok) *ok = 0;
    if (amp_membership_of("ls_amd_test_orbit_state", basis, &pj) != 0) return 0;
    struct ls_amd_basis_ext const *e = BEXT(basis);
    int const inv = basis->particle_type == LS_HS_SPIN && basis->spin_inversion != 0;
    uint64_t const all = e->nbits >= 64 ? ~0ULL : ((1ULL << e->nbits) - 1);
    if (element < 0 || element >= amp_num_elements(basis)) {
        set_error("ls_amd_test_orbit_state: element %d is outside [0, %d)", element, amp_num_elements(basis));
        return 0;
    }
    if (state & ~all) { set_error("ls_amd_test_orbit_state: the state 0x%llx has bits above the %d sites", (unsigned long long)state, e->nbits); return 0; }
    uint64_t t = host_apply_elem(&e->elems[inv ? element >> 1 : element], state, e->nbits);
    if (inv && (element & 1)) t ^= all;
    if (ok) *ok = 1;
    return t;
}

struct ls_amd_amp {
    lsk_basis bs;             /* device tables owned by the basis */
    lsk_project pj;           /* the membership kind and its numbers */
    lsk_index six;
    uint32_t *d_table;        /* owned: prefix table of a searched index */
    ls_amd_gtab *gtab;        /* shared static index table {representative -> row} (projected bases) */
    int pm1;                  /* every character is +-1: f64 allowed */
    int fermi;                /* a projected fermionic basis: k_amplitude_pull_fermi */
    int modes, n_elements;
    int *d_err;               /* owned: [0] a representative that is missing, [1] a row or element out of range */
    uint64_t const *d_reps;   /* borrowed */
    int64_t n;
};

void ls_amd_amp_destroy(ls_amd_amp *p) {
    if (!p) return;
    if (p->d_table) lsk_free(p->d_table);
    if (p->d_err) lsk_free(p->d_err);
    if (p->gtab) ls_amd_internal_gtab_release(p->gtab);
    free(p);
}

static int amp_setup(ls_amd_amp *p, ls_hs_basis const *basis, void *stream) {
    if (basis_device(basis, &p->bs) != 0) return -1;
    p->pm1 = cross_every_char_pm1(basis);
    void *q = NULL;
    DEV(lsk_malloc(&q, 4 * sizeof(int)));
    p->d_err = (int *)q;
    DEV(lsk_memset_async(p->d_err, 0, 4 * sizeof(int), stream));
    DEV(lsk_sync(stream));
    if (sector_lookup("ls_amd_amp_create", basis, &p->bs, p->d_reps, p->n, p->d_err, &p->six, &p->d_table, &p->gtab, stream) != 0) return -1;
    DEV(lsk_sync(stream));
    return 0;
}

int ls_amd_amp_create(ls_amd_amp **out, ls_hs_basis const *basis, uint64_t const *d_reps, int64_t n, void *stream) {
    if (out) *out = NULL;
    if (!out || !basis) return set_error("ls_amd_amp_create: NULL %s", !out ? "handle" : "basis");
    if (n < 0 || (n > 0 && !d_reps)) return set_error("ls_amd_amp_create: NULL representatives or a negative count");
    lsk_project pj;
    if (amp_membership_of("ls_amd_amp_create", basis, &pj) != 0) return -1;
    if (n >= 0xffffffffLL) return set_error("ls_amd_amp_create: source bases with >= 2^32 - 1 states are not supported");
    ls_amd_amp *p = (ls_amd_amp *)calloc(1, sizeof(*p));
    if (!p) return set_error("ls_amd_amp_create: out of host memory");
    p->pj = pj;
    p->fermi = BEXT(basis)->fermi != 0;
    p->modes = BEXT(basis)->nbits;
    p->n_elements = amp_num_elements(basis);
    p->d_reps = d_reps; p->n = n;
    if (amp_setup(p, basis, stream) != 0) { ls_amd_amp_destroy(p); return -1; }
    *out = p;
    return 0;
}

int ls_amd_amp_num_elements(ls_amd_amp const *p) {
    if (!p) return set_error("ls_amd_amp_num_elements: NULL plan");
    return p->n_elements;
}

int ls_amd_amp_amplitudes(ls_amd_amp *p, ls_amd_dtype dtype, int K, int64_t B, uint64_t const *d_states, void const *d_psi, int64_t psi_row,
                          int64_t psi_col, void *d_out, int64_t out_row, int64_t out_col, void *stream) {
    char const *const who = "ls_amd_amp_amplitudes";
    if (!p) return set_error("%s: NULL plan", who);
    if (dtype != LS_AMD_F64 && dtype != LS_AMD_C128) return set_error("%s: unknown dtype %d", who, (int)dtype);
    if (dtype == LS_AMD_F64 && !p->pm1) return set_error("%s: f64 needs +-1 characters (complex characters: use c128)", who);
    if (K < 1 || K > LSK_PROJECT_MAX_K) return set_error("%s: K = %d columns, outside [1, %d]", who, K, LSK_PROJECT_MAX_K);
    if (B < 0) return set_error("%s: a negative count of states (%lld)", who, (long long)B);
    if (B == 0) return 0;
    if (!d_states || !d_out || (!d_psi && p->n > 0)) return set_error("%s: NULL %s", who, !d_states ? "states" : (!d_out ? "out" : "psi"));
    if (K == 1) { psi_col = 0; out_col = 0; }
    if (psi_row < 0 || psi_col < 0) return set_error("%s: negative strides of psi", who);
    if (block_strides(who, B, K, out_row, out_col, "out") != 0) return -1;
    size_t const w = dtype == LS_AMD_C128 ? 16 : 8;
    if (p->n > 0 && block_overlap(w, p->n, d_psi, psi_row, psi_col, w, B, d_out, out_row, out_col, K)) return set_error("%s: out overlaps psi", who);
    lsk_project pj = p->pj;
    pj.K = K;
    pj.phi_s0 = psi_row; pj.phi_s1 = psi_col; pj.out_s0 = out_row; pj.out_s1 = out_col;
    lsk_gtab const gt = p->gtab ? p->gtab->tab : no_gtab();
    int const cplx = dtype == LS_AMD_C128;
    if (p->fermi) DEV(lsk_amplitude_pull_fermi(p->bs, p->six, gt, pj, cplx, B, d_states, d_psi, d_out, p->d_err, stream));
    else DEV(lsk_amplitude_pull(p->bs, p->six, gt, pj, cplx, B, d_states, d_psi, d_out, p->d_err, stream));
    return 0;
}

int ls_amd_amp_state_info(ls_amd_amp *p, int64_t B, uint64_t const *d_states, uint64_t *d_reps_out, int64_t *d_index, double *d_characters,
                          double *d_norms, void *stream) {
    char const *const who = "ls_amd_amp_state_info";
    if (!p) return set_error("%s: NULL plan", who);
    if (B < 0) return set_error("%s: a negative count of states (%lld)", who, (long long)B);
    if (B == 0) return 0;
    if (!d_states) return set_error("%s: NULL states", who);
    lsk_gtab const gt = p->gtab ? p->gtab->tab : no_gtab();
    if (p->fermi) DEV(lsk_amplitude_info_fermi(p->bs, p->six, gt, p->pj, B, d_states, d_reps_out, d_index, d_characters, d_norms, p->d_err, stream));
    else DEV(lsk_amplitude_info(p->bs, p->six, gt, p->pj, B, d_states, d_reps_out, d_index, d_characters, d_norms, p->d_err, stream));
    return 0;
}

int ls_amd_amp_orbit_states(ls_amd_amp *p, int64_t B, int64_t const *d_rows, int32_t const *d_elements, uint64_t *d_out, void *stream) {
    char const *const who = "ls_amd_amp_orbit_states";
    if (!p) return set_error("%s: NULL plan", who);
    if (B < 0) return set_error("%s: a negative count of pairs (%lld)", who, (long long)B);
    if (B == 0) return 0;
    if (!d_rows || !d_elements || !d_out) return set_error("%s: NULL %s", who, !d_rows ? "rows" : (!d_elements ? "elements" : "out"));
    if (p->fermi) DEV(lsk_orbit_image_fermi(p->bs, p->n, p->d_reps, B, d_rows, d_elements, d_out, p->d_err, stream));
    else DEV(lsk_orbit_image(p->bs, p->n, p->d_reps, B, d_rows, d_elements, d_out, p->d_err, stream));
    return 0;
}

int ls_amd_amp_check(ls_amd_amp *p, void *stream) {
    if (!p) return set_error("ls_amd_amp_check: NULL plan");
    int flag[2] = {0, 0}, zero[2] = {0, 0};
    DEV(lsk_sync(stream));
    DEV(lsk_d2h(flag, p->d_err, sizeof(flag)));
    if (flag[0] || flag[1]) DEV(lsk_h2d(p->d_err, zero, sizeof(zero)));
    if (flag[0])
        return set_error("sector amplitudes: the representative of a queried state has non-zero norm and is not in the basis (the array of "
                         "representatives does not belong to this basis or is not the whole sector)");
    if (flag[1])
        return set_error("orbit states: a row outside [0, %lld) or an element outside [0, %d)", (long long)p->n, p->n_elements);
    return 0;
}

char const *ls_amd_amp_kernel_name(ls_amd_amp const *p) {
    if (!p) { set_error("ls_amd_amp_kernel_name: NULL plan"); return NULL; }
    return p->fermi ? lsk_amplitude_fermi_kernel_name() : lsk_amplitude_kernel_name();
}

/* ============================================================================================ */
/* two-point correlation matrices (include/ls_amd.h: ls_amd_corr; csrc/k_corr.hip) */
/* ============================================================================================ */
/* The device sums over the representatives alone (the RAW matrices); C[i][j] = |G|^-1 sum_g R[g(i)][g(j)] over the whole group is
 * this host pass of |G| M^2 operations.  g(i) = the position of the bit of g(1 << i).  The elements that contain the global spin
 * inversion send bit b -> 1 - b: on the densities D -> 1 - d_i - d_j + D_ij (d -> 1 - d; a normalised state), on the hoppings
 * (i, j) -> (j, i) (and the diagonal, which holds the densities, -> 1 - d).
 * kind 0: raw / out = the one-point row d[M], then D[M][M];  kind 1: G[M][M] as (re, im) pairs. */
static int corr_symmetrize(ls_hs_basis const *basis, int kind, double const *raw, double *out) {
    struct ls_amd_basis_ext const *e = BEXT(basis);
    int const M = e->nbits, order = e->order, inv = basis->spin_inversion != 0;
    size_t const len = kind == 0 ? (size_t)M + (size_t)M * M : 2 * (size_t)M * M;
    int *img = (int *)malloc(sizeof(int) * (size_t)M);
    double *acc = (double *)calloc(len, sizeof(double));
    if (!img || !acc) { free(img); free(acc); return set_error("ls_amd_corr: out of host memory"); }
    for (int g = 0; g < order; ++g) {
        for (int s = 0; s < M; ++s) img[s] = __builtin_ctzll(host_apply_elem(&e->elems[g], 1ULL << s, M));
        if (kind == 0) {
            double const *d = raw, *D = raw + M;
            for (int i = 0; i < M; ++i) acc[i] += inv ? 1.0 : d[img[i]]; /* d + (1 - d) */
            for (int i = 0; i < M; ++i)
                for (int j = 0; j < M; ++j) {
                    double const v = D[(size_t)img[i] * M + img[j]];
                    acc[M + (size_t)i * M + j] += inv ? 1.0 - d[img[i]] - d[img[j]] + 2.0 * v : v;
                }
        } else {
            for (int i = 0; i < M; ++i)
                for (int j = 0; j < M; ++j) {
                    double const *a = raw + 2 * ((size_t)img[i] * M + img[j]), *b = raw + 2 * ((size_t)img[j] * M + img[i]);
                    double *o = acc + 2 * ((size_t)i * M + j);
                    if (!inv) { o[0] += a[0]; o[1] += a[1]; }
                    else if (i == j) { o[0] += 1.0; } /* G_ii + (1 - G_ii) */
                    else { o[0] += a[0] + b[0]; o[1] += a[1] + b[1]; }
                }
        }
    }
    double const scale = 1.0 / ((double)order * (inv ? 2.0 : 1.0));
    for (size_t k = 0; k < len; ++k) out[k] = acc[k] * scale;
    free(img); free(acc);
    return 0;
}

/* the refusals of ls_amd_corr_create that need no device */
static int corr_preconditions(char const *who, ls_hs_basis const *basis) {
    if (!basis) return set_error("%s: NULL basis", who);
    if (!reg_get(basis)) return set_error("%s: the basis is not built by this library (ls_amd_adopt_basis first)", who);
    struct ls_amd_basis_ext const *e = BEXT(basis);
    if (e->fermi && e->nbits > 60)
        return set_error("%s: projected fermionic bases of more than 60 modes are not supported (%d modes: the static index table does "
                         "not fit, as for their matvec and cross-sector plans)", who, e->nbits);
    return 0;
}

int ls_amd_test_corr_symmetrize(ls_hs_basis const *basis, int kind, double const *raw, double *out) {
    if (corr_preconditions("ls_amd_test_corr_symmetrize", basis) != 0) return -1;
    if (kind != 0 && kind != 1) return set_error("ls_amd_test_corr_symmetrize: kind %d is neither 0 (densities) nor 1 (hoppings)", kind);
    if (!raw || !out) return set_error("ls_amd_test_corr_symmetrize: NULL %s", !raw ? "raw matrix" : "output");
    return corr_symmetrize(basis, kind, raw, out);
}

struct ls_amd_corr {
    ls_hs_basis const *basis; /* borrowed */
    lsk_basis bs;             /* device tables owned by the basis */
    lsk_index six;
    uint32_t *d_table;        /* owned: prefix table of a searched (unprojected, incomplete) array */
    ls_amd_gtab *gtab;        /* shared: static index table of a projected basis */
    double *d_norms;          /* owned: n(r) of every row */
    int *d_err;               /* owned */
    uint64_t const *d_reps;   /* borrowed */
    int64_t n;
    int M, pm1, jw;           /* modes; every character is +-1: f64 allowed; fermionic: the hoppings carry the Jordan-Wigner sign */
    int n_dpairs, n_hpairs;   /* i <= j; ordered i != j (inside one species on the spinful product basis) */
    uint16_t *h_dpairs, *h_hpairs, *d_dpairs, *d_hpairs; /* owned: i | j << 8 */
    double *d_partial, *d_out, *h_out; /* owned: the partial sums of the blocks, the sums, and their host copy */
};

void ls_amd_corr_destroy(ls_amd_corr *pl) {
    if (!pl) return;
    if (pl->d_table) lsk_free(pl->d_table);
    if (pl->d_norms) lsk_free(pl->d_norms);
    if (pl->d_err) lsk_free(pl->d_err);
    if (pl->d_dpairs) lsk_free(pl->d_dpairs);
    if (pl->d_hpairs) lsk_free(pl->d_hpairs);
    if (pl->d_partial) lsk_free(pl->d_partial);
    if (pl->d_out) lsk_free(pl->d_out);
    if (pl->gtab) ls_amd_internal_gtab_release(pl->gtab);
    free(pl->h_dpairs); free(pl->h_hpairs); free(pl->h_out);
    free(pl);
}

static int corr_setup(ls_amd_corr *pl, void *stream) {
    struct ls_amd_basis_ext const *e = BEXT(pl->basis);
    int const M = pl->M;
    if (basis_device(pl->basis, &pl->bs) != 0) return -1;
    pl->pm1 = cross_every_char_pm1(pl->basis);
    pl->jw = pl->basis->particle_type != LS_HS_SPIN;
    /* the pairs: densities i <= j; hoppings every ordered i != j -- on the spinful (N, N_up) product basis inside one species only
     * (the others change N_up: exactly zero, and their images are no states of the basis) */
    pl->h_dpairs = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)(M * (M + 1) / 2));
    pl->h_hpairs = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)(M * M));
    int const half = pl->basis->number_sites;
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < M; ++j) {
            if (i <= j) pl->h_dpairs[pl->n_dpairs++] = (uint16_t)(i | j << 8);
            if (i != j && !(e->product && (i < half) != (j < half))) pl->h_hpairs[pl->n_hpairs++] = (uint16_t)(i | j << 8);
        }
    void *p = NULL;
    if (upload(&p, pl->h_dpairs, sizeof(uint16_t) * (size_t)pl->n_dpairs) != 0) return -1;
    pl->d_dpairs = (uint16_t *)p;
    if (pl->n_hpairs > 0) {
        if (upload(&p, pl->h_hpairs, sizeof(uint16_t) * (size_t)pl->n_hpairs) != 0) return -1;
        pl->d_hpairs = (uint16_t *)p;
    }
    size_t const vals = (size_t)(pl->n_dpairs > 2 * pl->n_hpairs ? pl->n_dpairs : 2 * pl->n_hpairs);
    pl->h_out = (double *)malloc(8 * vals);
    DEV(lsk_malloc(&p, 8 * vals * (size_t)lsk_corr_blocks(pl->n)));
    pl->d_partial = (double *)p;
    DEV(lsk_malloc(&p, 8 * vals));
    pl->d_out = (double *)p;
    DEV(lsk_malloc(&p, 4 * sizeof(int)));
    pl->d_err = (int *)p;
    DEV(lsk_memset_async(pl->d_err, 0, 4 * sizeof(int), stream));
    DEV(lsk_malloc(&p, 8 * (size_t)pl->n));
    pl->d_norms = (double *)p;
    /* the stabiliser norms, by the routine the matvec, cross-sector and expansion plans use */
    DEV(lsk_norms(pl->bs, pl->n, pl->d_reps, pl->d_norms, stream));
    DEV(lsk_sync(stream));
    return sector_lookup("ls_amd_corr_create", pl->basis, &pl->bs, pl->d_reps, pl->n, pl->d_err, &pl->six, &pl->d_table, &pl->gtab, stream);
}

int ls_amd_corr_create(ls_amd_corr **out, ls_hs_basis const *basis, uint64_t const *d_reps, int64_t n, void *stream) {
    if (out) *out = NULL;
    if (!out) return set_error("ls_amd_corr_create: NULL handle");
    if (corr_preconditions("ls_amd_corr_create", basis) != 0) return -1;
    if (n <= 0 || !d_reps) return set_error("ls_amd_corr_create: NULL representatives or no rows (n = %lld)", (long long)n);
    if (n >= 0xffffffffLL) return set_error("ls_amd_corr_create: bases with >= 2^32 - 1 states are not supported");
    ls_amd_corr *pl = (ls_amd_corr *)calloc(1, sizeof(*pl));
    pl->basis = basis;
    pl->M = NBITS(basis);
    pl->d_reps = d_reps; pl->n = n;
    if (corr_setup(pl, stream) != 0) { ls_amd_corr_destroy(pl); return -1; }
    *out = pl;
    return 0;
}

int ls_amd_corr_modes(ls_amd_corr const *pl) {
    if (!pl) return set_error("ls_amd_corr_modes: NULL plan");
    return pl->M;
}

static int corr_dtype(char const *who, ls_amd_corr const *pl, ls_amd_dtype dtype, void const *d_psi) {
    if (!pl || !d_psi) return set_error("%s: NULL %s", who, !pl ? "plan" : "psi");
    if (dtype != LS_AMD_F64 && dtype != LS_AMD_C128) return set_error("%s: unknown dtype %d", who, (int)dtype);
    if (dtype == LS_AMD_F64 && !pl->pm1) return set_error("%s: f64 needs +-1 characters (complex characters: use c128)", who);
    return 0;
}

/* the raw densities into raw[M + M * M] (the one-point row, then the symmetric D); synchronises the stream */
static int corr_raw_densities(ls_amd_corr *pl, int cplx, void const *d_psi, double *raw, void *stream) {
    int const M = pl->M;
    DEV(lsk_corr_diag(M, pl->n_dpairs, pl->d_dpairs, cplx, pl->n, pl->d_reps, d_psi, pl->d_partial, pl->d_out, stream));
    DEV(lsk_sync(stream));
    DEV(lsk_d2h(pl->h_out, pl->d_out, 8 * (size_t)pl->n_dpairs));
    for (int k = 0; k < pl->n_dpairs; ++k) {
        int const i = pl->h_dpairs[k] & 0xff, j = pl->h_dpairs[k] >> 8;
        raw[M + (size_t)i * M + j] = raw[M + (size_t)j * M + i] = pl->h_out[k];
        if (i == j) raw[i] = pl->h_out[k];
    }
    return 0;
}

int ls_amd_corr_densities(ls_amd_corr *pl, ls_amd_dtype dtype, void const *d_psi, double *h_d, double *h_dd, int symmetrize, void *stream) {
    if (corr_dtype("ls_amd_corr_densities", pl, dtype, d_psi) != 0) return -1;
    int const M = pl->M;
    size_t const len = (size_t)M + (size_t)M * M;
    double *raw = (double *)malloc(8 * 2 * len), *res = raw + len;
    int rc = corr_raw_densities(pl, dtype == LS_AMD_C128, d_psi, raw, stream);
    if (rc == 0 && symmetrize) rc = corr_symmetrize(pl->basis, 0, raw, res);
    else res = raw;
    if (rc == 0) {
        if (h_d) memcpy(h_d, res, 8 * (size_t)M);
        if (h_dd) memcpy(h_dd, res + M, 8 * (size_t)M * M);
    }
    free(raw);
    return rc;
}

int ls_amd_corr_hoppings(ls_amd_corr *pl, ls_amd_dtype dtype, void const *d_psi, double *h_g, int symmetrize, void *stream) {
    if (corr_dtype("ls_amd_corr_hoppings", pl, dtype, d_psi) != 0) return -1;
    if (!h_g) return set_error("ls_amd_corr_hoppings: NULL output");
    int const M = pl->M, cplx = dtype == LS_AMD_C128;
    size_t const len = 2 * (size_t)M * M;
    double *dens = (double *)malloc(8 * ((size_t)M + (size_t)M * M)), *raw = (double *)calloc(len, 8);
    int rc = corr_raw_densities(pl, cplx, d_psi, dens, stream);
    if (rc == 0 && pl->n_hpairs > 0) {
        rc = lsk_corr_hop(pl->bs, pl->six, pl->gtab ? pl->gtab->tab : no_gtab(), pl->jw, pl->n_hpairs, pl->d_hpairs, cplx, pl->n, pl->d_reps,
                          pl->d_norms, d_psi, pl->d_partial, pl->d_out, pl->d_err, stream) != 0 ? dev_error() : 0;
        int flag = 0, zero = 0;
        if (rc == 0 && (lsk_sync(stream) != 0 || lsk_d2h(&flag, pl->d_err, sizeof(int)) != 0)) rc = dev_error();
        if (rc == 0 && flag) {
            if (lsk_h2d(pl->d_err, &zero, sizeof(int)) != 0) rc = dev_error();
            else rc = set_error("correlations: the image of a representative under a hopping has non-zero norm and is not in the basis (the "
                                "array of representatives does not belong to this basis or is not the whole sector: another Hamming weight, "
                                "a truncated array)");
        }
        if (rc == 0 && lsk_d2h(pl->h_out, pl->d_out, 8 * (size_t)pl->n_hpairs * (cplx ? 2 : 1)) != 0) rc = dev_error();
    }
    if (rc == 0) {
        for (int k = 0; k < pl->n_hpairs; ++k) {
            size_t const at = 2 * ((size_t)(pl->h_hpairs[k] & 0xff) * M + (pl->h_hpairs[k] >> 8));
            raw[at] = cplx ? pl->h_out[2 * k] : pl->h_out[k];
            raw[at + 1] = cplx ? pl->h_out[2 * k + 1] : 0.0;
        }
        for (int i = 0; i < M; ++i) raw[2 * ((size_t)i * M + i)] = dens[i];
        if (symmetrize) rc = corr_symmetrize(pl->basis, 1, raw, h_g);
        else memcpy(h_g, raw, 8 * len);
    }
    free(dens); free(raw);
    return rc;
}

char const *ls_amd_corr_kernel_name(ls_amd_corr const *pl, int which) {
    if (!pl) { set_error("ls_amd_corr_kernel_name: NULL plan"); return NULL; }
    if (which == 0) return lsk_corr_diag_kernel_name();
    if (which == 1) return pl->bs.fermi ? lsk_corr_hop_fermi_kernel_name() : lsk_corr_hop_kernel_name();
    set_error("ls_amd_corr_kernel_name: kernel %d is neither 0 (densities) nor 1 (hoppings)", which);
    return NULL;
}

/* ============================================================================================ */
/* expectation values of arbitrary operators (include/ls_amd.h: ls_amd_expect; csrc/k_expect.hip) */
/* ============================================================================================ */
/* <psi|O|psi> = |G|^-1 sum_g R[U_g O U_g^-1], R[A] = sum_r conj(psi_r) / n(r) (A psi^)(r) over the representatives alone.  The host
 * conjugates every term by every element of the group -- inside the term format -- and the device evaluates R of the unique results.
 * One entry = one conjugated term of operator k, scaled by |G|^-1, in canonical form: r inside m, the sign bits inside m (where the
 * state is fixed) folded into the coefficient. */
typedef struct { uint64_t x, m, r, s; int k; double re, im; } expect_entry;
static int expect_key_cmp(expect_entry const *a, expect_entry const *b) {
    if (a->x != b->x) return a->x < b->x ? -1 : 1;
    if (a->m != b->m) return a->m < b->m ? -1 : 1;
    if (a->r != b->r) return a->r < b->r ? -1 : 1;
    if (a->s != b->s) return a->s < b->s ? -1 : 1;
    return 0;
}
static int expect_entry_cmp(void const *pa, void const *pb) {
    expect_entry const *a = (expect_entry const *)pa, *b = (expect_entry const *)pb;
    int const c = expect_key_cmp(a, b);
    return c != 0 ? c : (a->k > b->k) - (a->k < b->k);
}
/* adjoint != 0: the row-wise orientation of ls_amd_operator_adjoint without the conjugation of v -- <b|A|b ^ x> is tested on the row b */
static expect_entry expect_canonical(raw_term t, int k, int adjoint, double scale) {
    t.r &= t.m;
    if (adjoint) {
        if (__builtin_popcountll(t.x & t.s) & 1) { t.re = -t.re; t.im = -t.im; }
        t.r ^= t.x & t.m;
    }
    if (__builtin_popcountll(t.r & t.s) & 1) { t.re = -t.re; t.im = -t.im; }
    expect_entry e = {t.x, t.m, t.r, t.s & ~t.m, k, t.re * scale, t.im * scale};
    return e;
}
/* appends the |G| conjugates U_g t U_g^-1 / |G| of the n raw terms t (|G| counts the inversion doubling) to *buf */
static int expect_conjugates(char const *who, ls_hs_basis const *basis, raw_term const *t, int n, int k, int adjoint, expect_entry **buf,
                             size_t *len, size_t *cap) {
    struct ls_amd_basis_ext const *e = BEXT(basis);
    int const L = e->nbits, order = e->order > 0 ? e->order : 1, inv = basis->spin_inversion != 0;
    double const scale = 1.0 / ((double)order * (inv ? 2.0 : 1.0));
    if (e->fermi)
        for (int i = 0; i < n; ++i)
            if (t[i].x & ~t[i].m)
                return set_error("%s: a term flips modes outside its projector mask (x = 0x%llx is not inside m = 0x%llx): not a product "
                                 "of creation and annihilation operators", who, (unsigned long long)t[i].x, (unsigned long long)t[i].m);
    size_t const need = *len + (size_t)order * (inv ? 2 : 1) * (size_t)n;
    if (need > *cap) {
        size_t const c = need > 2 * *cap ? need : 2 * *cap;
        expect_entry *nb = (expect_entry *)realloc(*buf, sizeof(expect_entry) * (c > 0 ? c : 1));
        if (!nb) return set_error("%s: out of host memory", who);
        *buf = nb; *cap = c;
    }
    int p[64];
    uint64_t tab[64], nbr[64];
    for (int g = 0; g < order; ++g) {
        int ident = 1;
        if (e->elems && e->order > 0) { /* p[i] = the bit that element g carries to position i: (g.w)[i] = w[p[i]] */
            for (int s = 0; s < L; ++s) p[__builtin_ctzll(host_apply_elem(&e->elems[g], 1ULL << s, L))] = s;
        } else for (int s = 0; s < L; ++s) p[s] = s;
        for (int s = 0; s < L; ++s) ident &= p[s] == s;
        if (e->fermi && !ident) perm_sign_table(p, L, tab, nbr);
        for (int i = 0; i < n; ++i) {
            raw_term c = t[i];
            c.r &= c.m;
            if (!ident) {
                if (e->fermi) c = signed_conjugate(c, p, L, tab, nbr);
                else { c.m = permute_mask(p, L, c.m); c.r = permute_mask(p, L, c.r); c.x = permute_mask(p, L, c.x); c.s = permute_mask(p, L, c.s); }
            }
            (*buf)[(*len)++] = expect_canonical(c, k, adjoint, scale);
            if (inv) { /* the same element with the global flip: ((-1)^popcount(s) v, m, r ^ m, x, s) */
                raw_term f = c;
                if (__builtin_popcountll(f.s) & 1) { f.re = -f.re; f.im = -f.im; }
                f.r ^= f.m;
                (*buf)[(*len)++] = expect_canonical(f, k, adjoint, scale);
            }
        }
    }
    return 0;
}
/* sorts by (key, k), adds the coefficients of equal (key, k) in that order and drops what cancels (|w| <= 1e-15 vmax[k]: the rounding
 * residue of at most |G| summands of modulus vmax / |G|); returns the entries left */
static size_t expect_merge(expect_entry *buf, size_t len, double const *vmax) {
    qsort(buf, len, sizeof(expect_entry), expect_entry_cmp);
    size_t w = 0;
    for (size_t i = 0; i < len;) {
        expect_entry acc = buf[i];
        size_t j = i + 1;
        while (j < len && expect_entry_cmp(&buf[i], &buf[j]) == 0) { acc.re += buf[j].re; acc.im += buf[j].im; ++j; }
        if (hypot(acc.re, acc.im) > 1e-15 * vmax[acc.k]) buf[w++] = acc;
        i = j;
    }
    return w;
}
static double raw_vmax(raw_term const *t, int n) {
    double v = 0.0;
    for (int i = 0; i < n; ++i) { double const a = hypot(t[i].re, t[i].im); if (a > v) v = a; }
    return v;
}
static int expect_operator_check(char const *who, ls_hs_basis const *basis, ls_hs_operator const *op, int k) {
    if (!op) return set_error("%s: operator %d is NULL", who, k);
    if (!reg_get(op)) return set_error("%s: operator %d is unknown (ls_amd_adopt_operator first)", who, k);
    if (op->basis != basis) return set_error("%s: operator %d is an operator of another basis (build it on the basis of the plan)", who, k);
    return 0;
}

int64_t ls_amd_test_expect_average(ls_hs_basis const *basis, ls_hs_operator const *op, int64_t cap, double *v, uint64_t *m, uint64_t *r,
                                   uint64_t *x, uint64_t *s) {
    char const *who = "ls_amd_test_expect_average";
    if (corr_preconditions(who, basis) != 0) return -1;
    if (expect_operator_check(who, basis, op, 0) != 0) return -1;
    if (cap > 0 && (!v || !m || !r || !x || !s)) return set_error("%s: NULL output", who);
    raw_term *t = NULL;
    int const n = operator_raw_terms(op, &t);
    double const vmax = raw_vmax(t, n);
    expect_entry *buf = NULL;
    size_t len = 0, room = 0;
    int const rc = expect_conjugates(who, basis, t, n, 0, 0, &buf, &len, &room);
    free(t);
    if (rc != 0) { free(buf); return -1; }
    len = expect_merge(buf, len, &vmax);
    for (size_t i = 0; i < len && (int64_t)i < cap; ++i) {
        v[2 * i] = buf[i].re; v[2 * i + 1] = buf[i].im;
        m[i] = buf[i].m; r[i] = buf[i].r; x[i] = buf[i].x; s[i] = buf[i].s;
    }
    free(buf);
    return (int64_t)len;
}

struct ls_amd_expect {
    ls_hs_basis const *basis; /* borrowed */
    lsk_basis bs;             /* device tables owned by the basis */
    lsk_index six;
    uint32_t *d_table;        /* owned: prefix table of a searched (unprojected, incomplete) array */
    ls_amd_gtab *gtab;        /* shared: static index table of a projected basis */
    double *d_norms;          /* owned: n(r) of every row */
    int *d_err;               /* owned */
    uint64_t const *d_reps;   /* borrowed */
    int64_t n;
    int pm1, n_ops, n_terms, n_groups, n_chunks;
    lsk_expect_cons cons;
    lsk_expect_group *h_groups, *d_groups; /* owned: sorted by flip mask, at most LSK_EXPECT_CHUNK terms each */
    lsk_expect_term *d_terms;              /* owned: the unique device terms, in group order */
    int *chunk_first;                      /* owned [n_chunks + 1]: the groups of every launch */
    size_t n_comb;                         /* value[k] = sum over the entries with comb_k == k of comb_w * R[comb_u] */
    int *comb_k, *comb_u;
    double *comb_w;                        /* (re, im) */
    double *d_partial, *d_out, *h_out;     /* owned: the partial sums of the blocks of one chunk; R of every term, and its host copy */
    /* ls_amd_expect_values_block, all owned and allocated at the first call that needs them (grown by later ones): */
    double *d_blk_partial;                 /* the partial sums of the blocks of one block launch, blk_partial_vals x 16 bytes */
    double *d_blk_out, *h_blk_out;         /* R of every (term, column), blk_out_vals x 16 bytes, and its host copy */
    size_t blk_partial_vals, blk_out_vals;
    void *d_blk_col;                       /* a contiguous scratch column of the column loop */
    double *h_col;                         /* the values of one column of the column loop */
    /* ls_amd_expect_matrix_elements, owned and allocated at the first call (grown by later ones): */
    double *d_mat_partial;                 /* the partial sums of the blocks of one matrix launch, mat_partial_vals x 16 bytes */
    double *d_mat_out, *h_mat_out;         /* R of every (term, bra, ket), mat_out_vals x 16 bytes, and its host copy */
    size_t mat_partial_vals, mat_out_vals;
};

void ls_amd_expect_destroy(ls_amd_expect *pl) {
    if (!pl) return;
    if (pl->d_table) lsk_free(pl->d_table);
    if (pl->d_norms) lsk_free(pl->d_norms);
    if (pl->d_err) lsk_free(pl->d_err);
    if (pl->d_groups) lsk_free(pl->d_groups);
    if (pl->d_terms) lsk_free(pl->d_terms);
    if (pl->d_partial) lsk_free(pl->d_partial);
    if (pl->d_out) lsk_free(pl->d_out);
    if (pl->d_blk_partial) lsk_free(pl->d_blk_partial);
    if (pl->d_blk_out) lsk_free(pl->d_blk_out);
    if (pl->d_blk_col) lsk_free(pl->d_blk_col);
    if (pl->d_mat_partial) lsk_free(pl->d_mat_partial);
    if (pl->d_mat_out) lsk_free(pl->d_mat_out);
    if (pl->gtab) ls_amd_internal_gtab_release(pl->gtab);
    free(pl->h_groups); free(pl->chunk_first); free(pl->comb_k); free(pl->comb_u); free(pl->comb_w); free(pl->h_out);
    free(pl->h_blk_out); free(pl->h_col); free(pl->h_mat_out);
    free(pl);
}

/* the batch: unique device terms in flip-mask groups, the launches, and the sparse combination (host only) */
static int expect_compile(ls_amd_expect *pl, ls_hs_operator const *const *ops, lsk_expect_term **h_terms) {
    char const *who = "ls_amd_expect_create";
    expect_entry *buf = NULL;
    size_t len = 0, room = 0;
    double *vmax = (double *)calloc((size_t)pl->n_ops, sizeof(double));
    int rc = 0;
    for (int k = 0; k < pl->n_ops && rc == 0; ++k) {
        raw_term *t = NULL;
        int const n = operator_raw_terms(ops[k], &t);
        vmax[k] = raw_vmax(t, n);
        rc = expect_conjugates(who, pl->basis, t, n, k, 1, &buf, &len, &room);
        free(t);
    }
    if (rc != 0) { free(buf); free(vmax); return -1; }
    len = expect_merge(buf, len, vmax);
    free(vmax);
    if (len >= (size_t)INT32_MAX) { free(buf); return set_error("%s: %zu conjugated terms in the batch, at most 2^31 - 1", who, len); }
    /* the entries are sorted by key: one device term per key, one group per flip mask (split at LSK_EXPECT_CHUNK terms) */
    size_t const cap = len > 0 ? len : 1;
    *h_terms = (lsk_expect_term *)malloc(sizeof(lsk_expect_term) * cap);
    pl->h_groups = (lsk_expect_group *)malloc(sizeof(lsk_expect_group) * cap);
    pl->comb_k = (int *)malloc(sizeof(int) * cap); pl->comb_u = (int *)malloc(sizeof(int) * cap);
    pl->comb_w = (double *)malloc(16 * cap);
    if (!*h_terms || !pl->h_groups || !pl->comb_k || !pl->comb_u || !pl->comb_w) { free(buf); return set_error("%s: out of host memory", who); }
    int nt = 0, ng = 0;
    for (size_t i = 0; i < len; ++i) {
        int const fresh = i == 0 || expect_key_cmp(&buf[i - 1], &buf[i]) != 0;
        if (fresh) {
            if (ng == 0 || pl->h_groups[ng - 1].x != buf[i].x || nt - pl->h_groups[ng - 1].begin >= LSK_EXPECT_CHUNK) {
                lsk_expect_group g = {buf[i].x, buf[i].m, buf[i].r, nt, nt};
                pl->h_groups[ng++] = g;
            }
            lsk_expect_group *g = &pl->h_groups[ng - 1];
            /* the common projector: the mask bits every term of the group has, with one value */
            g->cm &= buf[i].m & ~(g->cr ^ buf[i].r);
            g->cr &= g->cm;
            lsk_expect_term t = {buf[i].m, buf[i].r, buf[i].s};
            (*h_terms)[nt++] = t;
            g->end = nt;
        }
        pl->comb_k[i] = buf[i].k; pl->comb_u[i] = nt - 1;
        pl->comb_w[2 * i] = buf[i].re; pl->comb_w[2 * i + 1] = buf[i].im;
    }
    free(buf);
    pl->n_comb = len; pl->n_terms = nt; pl->n_groups = ng;
    /* launches: consecutive groups of at most LSK_EXPECT_CHUNK terms together */
    pl->chunk_first = (int *)malloc(sizeof(int) * ((size_t)ng + 2));
    pl->n_chunks = 0;
    for (int g = 0; g < ng;) {
        pl->chunk_first[pl->n_chunks++] = g;
        int const t0 = pl->h_groups[g].begin;
        int h = g + 1;
        while (h < ng && pl->h_groups[h].end - t0 <= LSK_EXPECT_CHUNK) ++h;
        g = h;
    }
    pl->chunk_first[pl->n_chunks] = ng;
    return 0;
}

static int expect_setup(ls_amd_expect *pl, lsk_expect_term const *h_terms, void *stream) {
    struct ls_amd_basis_ext const *e = BEXT(pl->basis);
    if (basis_device(pl->basis, &pl->bs) != 0) return -1;
    pl->pm1 = cross_every_char_pm1(pl->basis);
    pl->cons.weight = e->product ? -1 : e->hamming_weight;
    if (e->product) { pl->cons.half = pl->basis->number_sites; pl->cons.n_up = e->prod_up; pl->cons.n_dn = e->prod_dn; }
    void *p = NULL;
    if (pl->n_terms > 0) {
        if (upload(&p, h_terms, sizeof(lsk_expect_term) * (size_t)pl->n_terms) != 0) return -1;
        pl->d_terms = (lsk_expect_term *)p;
        if (upload(&p, pl->h_groups, sizeof(lsk_expect_group) * (size_t)pl->n_groups) != 0) return -1;
        pl->d_groups = (lsk_expect_group *)p;
    }
    size_t const chunk = (size_t)(pl->n_terms < LSK_EXPECT_CHUNK ? (pl->n_terms > 0 ? pl->n_terms : 1) : LSK_EXPECT_CHUNK);
    size_t const vals = 2 * (size_t)(pl->n_terms > 0 ? pl->n_terms : 1);
    pl->h_out = (double *)malloc(8 * vals);
    DEV(lsk_malloc(&p, 16 * chunk * (size_t)lsk_corr_blocks(pl->n)));
    pl->d_partial = (double *)p;
    DEV(lsk_malloc(&p, 8 * vals));
    pl->d_out = (double *)p;
    DEV(lsk_malloc(&p, 4 * sizeof(int)));
    pl->d_err = (int *)p;
    DEV(lsk_memset_async(pl->d_err, 0, 4 * sizeof(int), stream));
    DEV(lsk_malloc(&p, 8 * (size_t)pl->n));
    pl->d_norms = (double *)p;
    /* the stabiliser norms and the look-up, as ls_amd_corr_create builds them */
    DEV(lsk_norms(pl->bs, pl->n, pl->d_reps, pl->d_norms, stream));
    DEV(lsk_sync(stream));
    return sector_lookup("ls_amd_expect_create", pl->basis, &pl->bs, pl->d_reps, pl->n, pl->d_err, &pl->six, &pl->d_table, &pl->gtab, stream);
}

int ls_amd_expect_create(ls_amd_expect **out, ls_hs_basis const *basis, ls_hs_operator const *const *ops, int n_ops,
                         uint64_t const *d_reps, int64_t n, void *stream) {
    char const *who = "ls_amd_expect_create";
    if (out) *out = NULL;
    if (!out) return set_error("%s: NULL handle", who);
    if (corr_preconditions(who, basis) != 0) return -1;
    if (n_ops <= 0 || !ops) return set_error("%s: no operators (n_ops = %d%s)", who, n_ops, ops ? "" : ", NULL array");
    for (int k = 0; k < n_ops; ++k)
        if (expect_operator_check(who, basis, ops[k], k) != 0) return -1;
    if (n <= 0 || !d_reps) return set_error("%s: NULL representatives or no rows (n = %lld)", who, (long long)n);
    if (n >= 0xffffffffLL) return set_error("%s: bases with >= 2^32 - 1 states are not supported", who);
    ls_amd_expect *pl = (ls_amd_expect *)calloc(1, sizeof(*pl));
    pl->basis = basis;
    pl->n_ops = n_ops;
    pl->d_reps = d_reps; pl->n = n;
    lsk_expect_term *h_terms = NULL;
    int rc = expect_compile(pl, ops, &h_terms);
    if (rc == 0) rc = expect_setup(pl, h_terms, stream);
    free(h_terms);
    if (rc != 0) { ls_amd_expect_destroy(pl); return -1; }
    *out = pl;
    return 0;
}

int ls_amd_expect_num_terms(ls_amd_expect const *pl) {
    if (!pl) return set_error("ls_amd_expect_num_terms: NULL plan");
    return pl->n_terms;
}

int ls_amd_expect_num_groups(ls_amd_expect const *pl) {
    if (!pl) return set_error("ls_amd_expect_num_groups: NULL plan");
    return pl->n_groups;
}

char const *ls_amd_expect_kernel_name(ls_amd_expect const *pl) {
    if (!pl) { set_error("ls_amd_expect_kernel_name: NULL plan"); return NULL; }
    return pl->bs.fermi ? lsk_expect_fermi_kernel_name() : lsk_expect_kernel_name();
}

/* ---- what ls_amd_expect_values, ls_amd_expect_values_block and ls_amd_expect_matrix_elements share ---- */
/* a block of states handed to an entry point, as its messages name it */
typedef struct expect_block { char const *name; int K; int64_t row, col; } expect_block;
/* the checks behind the plan, the pointers and the numbers of columns: dtype, characters, output, then the strides of the nb blocks
 * (all positive, then no two elements on one) */
static int expect_check_args(char const *who, ls_amd_expect const *pl, ls_amd_dtype dtype, double const *h_out, expect_block const *blk,
                             int nb) {
    if (dtype != LS_AMD_F64 && dtype != LS_AMD_C128) return set_error("%s: unknown dtype %d", who, (int)dtype);
    if (dtype == LS_AMD_F64 && !pl->pm1) return set_error("%s: f64 needs +-1 characters (complex characters: use c128)", who);
    if (!h_out) return set_error("%s: NULL output", who);
    for (int i = 0; i < nb; ++i)
        if (blk[i].row <= 0 || blk[i].col <= 0)
            return set_error("%s: strides (row %lld, column %lld) of %s must be positive", who, (long long)blk[i].row, (long long)blk[i].col,
                             blk[i].name);
    for (int i = 0; i < nb; ++i)
        if (block_strides(who, pl->n, blk[i].K, blk[i].row, blk[i].col, blk[i].name) != 0) return -1;
    return 0;
}
/* launch c of a plan: the groups [g0, g1) and their terms [t0, t0 + nt) */
typedef struct expect_chunk { int g0, g1, t0, nt; } expect_chunk;
static expect_chunk expect_chunk_of(ls_amd_expect const *pl, int c) {
    int const g0 = pl->chunk_first[c], g1 = pl->chunk_first[c + 1], t0 = pl->h_groups[g0].begin;
    return (expect_chunk){ g0, g1, t0, pl->h_groups[g1 - 1].end - t0 };
}
/* a device buffer of at least `vals` 16-byte values and, where h is given, its host copy: freed and allocated anew by a call that
 * needs more (*have: what they hold, 0 after a failure) */
static int expect_grow(char const *who, double **d, double **h, size_t *have, size_t vals) {
    if (vals <= *have) return 0;
    if (*d) { lsk_free(*d); *d = NULL; }
    if (h) { free(*h); *h = NULL; }
    *have = 0;
    void *p = NULL;
    DEV(lsk_malloc(&p, 16 * vals));
    *d = (double *)p;
    if (h && !(*h = (double *)malloc(16 * vals))) return set_error("%s: out of host memory", who);
    *have = vals;
    return 0;
}
/* behind the launches of a call: wait for them and read the flag they raise (cleared again for the next call) */
static int expect_finish_launches(ls_amd_expect *pl, void *stream) {
    int flag = 0, zero = 0;
    DEV(lsk_sync(stream));
    DEV(lsk_d2h(&flag, pl->d_err, sizeof(int)));
    if (flag) {
        DEV(lsk_h2d(pl->d_err, &zero, sizeof(int)));
        return set_error("expectation values: the image of a representative under a term keeps the conserved numbers, has non-zero norm "
                         "and is not in the basis (the array of representatives does not belong to this basis or is not the whole "
                         "sector: another Hamming weight, a truncated array)");
    }
    return 0;
}

int ls_amd_expect_values(ls_amd_expect *pl, ls_amd_dtype dtype, void const *d_psi, double *h_out, void *stream) {
    char const *who = "ls_amd_expect_values";
    if (!pl || !d_psi) return set_error("%s: NULL %s", who, !pl ? "plan" : "psi");
    if (expect_check_args(who, pl, dtype, h_out, NULL, 0) != 0) return -1;
    int const cplx = dtype == LS_AMD_C128, nc = cplx ? 2 : 1;
    for (int c = 0; c < pl->n_chunks; ++c) {
        expect_chunk const ck = expect_chunk_of(pl, c);
        DEV(lsk_expect(pl->bs, pl->six, pl->gtab ? pl->gtab->tab : no_gtab(), pl->cons, ck.g1 - ck.g0, pl->d_groups + ck.g0, pl->d_terms, ck.t0,
                       ck.nt, cplx, pl->n, pl->d_reps, pl->d_norms, d_psi, pl->d_partial, pl->d_out + (size_t)ck.t0 * nc, pl->d_err, stream));
    }
    if (expect_finish_launches(pl, stream) != 0) return -1;
    if (pl->n_terms > 0) DEV(lsk_d2h(pl->h_out, pl->d_out, 8 * (size_t)pl->n_terms * nc));
    for (int k = 0; k < 2 * pl->n_ops; ++k) h_out[k] = 0.0;
    for (size_t i = 0; i < pl->n_comb; ++i) {
        int const u = pl->comb_u[i];
        double const rr = cplx ? pl->h_out[2 * u] : pl->h_out[u], ri = cplx ? pl->h_out[2 * u + 1] : 0.0;
        double const wr = pl->comb_w[2 * i], wi = pl->comb_w[2 * i + 1];
        h_out[2 * pl->comb_k[i]] += wr * rr - wi * ri;
        h_out[2 * pl->comb_k[i] + 1] += wr * ri + wi * rr;
    }
    return 0;
}

/* ---- blocks of states (include/ls_amd.h: ls_amd_expect_values_block; csrc/k_expect_blk.hip) ---- */
/* LS_AMD_EXPECT_BLOCK, read at every call: `columns` loops ls_amd_expect_values over the columns; `kernel` and anything else
 * (`auto`) take k_expect_blk for every K ("Block expectation values") */
static int expect_block_columns(void) {
    char const *e = getenv("LS_AMD_EXPECT_BLOCK");
    return e && strcmp(e, "columns") == 0;
}

char const *ls_amd_expect_block_kernel_name(ls_amd_expect const *pl, int K) {
    if (!pl) { set_error("ls_amd_expect_block_kernel_name: NULL plan"); return NULL; }
    if (K < 1 || K > 64) { set_error("ls_amd_expect_block_kernel_name: K = %d is outside [1, 64]", K); return NULL; }
    if (expect_block_columns()) return "columns";
    return pl->bs.fermi ? lsk_expect_blk_fermi_kernel_name() : lsk_expect_blk_kernel_name();
}

/* columns of one block launch over a chunk of nt <= LSK_EXPECT_CHUNK terms: all K while nt * K stays within 8 LSK_EXPECT_CHUNK
 * partial sums per block, else the most whole chunks of 8 columns that do (at least one) */
static int expect_block_cols(int nt, int K) {
    if ((int64_t)nt * K <= 8 * (int64_t)LSK_EXPECT_CHUNK) return K;
    return 8 * LSK_EXPECT_CHUNK / nt / 8 * 8;
}

static int expect_block_kernel(ls_amd_expect *pl, int cplx, int K, char const *psi, int64_t p_row, int64_t p_col, double *h_out, void *stream) {
    char const *who = "ls_amd_expect_values_block";
    int const nc = cplx ? 2 : 1;
    size_t const w = 8 * (size_t)nc;
    /* the buffers of the block calls: allocated here, at the first call that needs them, and grown by a call with more columns */
    size_t part = 1;
    for (int c = 0; c < pl->n_chunks; ++c) {
        size_t const nt = (size_t)expect_chunk_of(pl, c).nt;
        size_t const v = nt * (size_t)expect_block_cols((int)nt, K);
        if (v > part) part = v;
    }
    part *= (size_t)lsk_corr_blocks(pl->n);
    if (expect_grow(who, &pl->d_blk_partial, NULL, &pl->blk_partial_vals, part) != 0) return -1;
    size_t const vals = (size_t)(pl->n_terms > 0 ? pl->n_terms : 1) * (size_t)K;
    if (expect_grow(who, &pl->d_blk_out, &pl->h_blk_out, &pl->blk_out_vals, vals) != 0) return -1;
    /* the launches: per chunk of terms, per range of columns; a launch writes R[(u - t0) kl + (c - k0)] of its nt terms and kl
     * columns at (t0 K + nt k0) of d_blk_out */
    for (int c = 0; c < pl->n_chunks; ++c) {
        expect_chunk const ck = expect_chunk_of(pl, c);
        int const t0 = ck.t0, nt = ck.nt;
        int const cols = expect_block_cols(nt, K);
        for (int k0 = 0; k0 < K; k0 += cols) {
            int const kl = K - k0 < cols ? K - k0 : cols;
            DEV(lsk_expect_blk(pl->bs, pl->six, pl->gtab ? pl->gtab->tab : no_gtab(), pl->cons, ck.g1 - ck.g0, pl->d_groups + ck.g0, pl->d_terms,
                               t0, nt, cplx, pl->n, pl->d_reps, pl->d_norms, kl, psi + (size_t)k0 * (size_t)p_col * w, p_row, p_col,
                               pl->d_blk_partial, pl->d_blk_out + ((size_t)t0 * (size_t)K + (size_t)nt * (size_t)k0) * nc, pl->d_err, stream));
        }
    }
    if (expect_finish_launches(pl, stream) != 0) return -1;
    if (pl->n_terms > 0) DEV(lsk_d2h(pl->h_blk_out, pl->d_blk_out, w * (size_t)pl->n_terms * (size_t)K));
    for (int k = 0; k < 2 * pl->n_ops * K; ++k) h_out[k] = 0.0;
    /* value[k][c] = sum_u w[k][u] R[u][c]: the loop of ls_amd_expect_values per column (comb_u ascends: the chunk follows it) */
    int ch = 0;
    for (size_t i = 0; i < pl->n_comb; ++i) {
        int const u = pl->comb_u[i];
        while (u >= pl->h_groups[pl->chunk_first[ch + 1] - 1].end) ++ch;
        int const t0 = expect_chunk_of(pl, ch).t0, nt = expect_chunk_of(pl, ch).nt;
        int const cols = expect_block_cols(nt, K);
        double const wr = pl->comb_w[2 * i], wi = pl->comb_w[2 * i + 1];
        double *const o = h_out + 2 * (size_t)pl->comb_k[i] * (size_t)K;
        for (int col = 0; col < K; ++col) {
            int const k0 = col / cols * cols, kl = K - k0 < cols ? K - k0 : cols;
            size_t const at = (size_t)t0 * (size_t)K + (size_t)nt * (size_t)k0 + (size_t)(u - t0) * (size_t)kl + (size_t)(col - k0);
            double const rr = cplx ? pl->h_blk_out[2 * at] : pl->h_blk_out[at], ri = cplx ? pl->h_blk_out[2 * at + 1] : 0.0;
            o[2 * col] += wr * rr - wi * ri;
            o[2 * col + 1] += wr * ri + wi * rr;
        }
    }
    return 0;
}

int ls_amd_expect_values_block(ls_amd_expect *pl, ls_amd_dtype dtype, int K, void const *d_psi, int64_t row_stride, int64_t col_stride,
                               double *h_out, void *stream) {
    char const *who = "ls_amd_expect_values_block";
    if (!pl || !d_psi) return set_error("%s: NULL %s", who, !pl ? "plan" : "block");
    if (K < 1 || K > 64) return set_error("%s: K = %d is outside [1, 64]", who, K);
    expect_block const blk = { "the block", K, row_stride, col_stride };
    if (expect_check_args(who, pl, dtype, h_out, &blk, 1) != 0) return -1;
    int const cplx = dtype == LS_AMD_C128;
    size_t const w = cplx ? 16 : 8;
    char const *const psi = (char const *)d_psi;
    if (!expect_block_columns()) return expect_block_kernel(pl, cplx, K, psi, row_stride, col_stride, h_out, stream);
    /* the column loop: ls_amd_expect_values, through a contiguous scratch column that the plan owns where the rows are strided */
    if (!pl->h_col && !(pl->h_col = (double *)malloc(16 * (size_t)pl->n_ops))) return set_error("%s: out of host memory", who);
    if (row_stride != 1 && !pl->d_blk_col) DEV(lsk_malloc(&pl->d_blk_col, 16 * (size_t)pl->n));
    for (int c = 0; c < K; ++c) {
        void const *col = psi + (size_t)c * (size_t)col_stride * w;
        if (row_stride != 1) {
            DEV(lsk_copy_strided(pl->n, (int)w, col, row_stride, pl->d_blk_col, 1, stream));
            col = pl->d_blk_col;
        }
        if (ls_amd_expect_values(pl, dtype, col, pl->h_col, stream) != 0) return -1;
        for (int k = 0; k < pl->n_ops; ++k) {
            h_out[2 * ((size_t)k * (size_t)K + (size_t)c)] = pl->h_col[2 * k];
            h_out[2 * ((size_t)k * (size_t)K + (size_t)c) + 1] = pl->h_col[2 * k + 1];
        }
    }
    return 0;
}

/* ---- matrix elements between two blocks (include/ls_amd.h: ls_amd_expect_matrix_elements; csrc/k_expect_mat.hip) ---- */
char const *ls_amd_expect_matrix_kernel_name(ls_amd_expect const *pl, int Ka, int Kb) {
    if (!pl) { set_error("ls_amd_expect_matrix_kernel_name: NULL plan"); return NULL; }
    if (Ka < 1 || Ka > 64 || Kb < 1 || Kb > 64) {
        set_error("ls_amd_expect_matrix_kernel_name: Ka = %d, Kb = %d: each must be within [1, 64]", Ka, Kb);
        return NULL;
    }
    return pl->bs.fermi ? lsk_expect_mat_fermi_kernel_name() : lsk_expect_mat_kernel_name();
}

/* (bra, ket) columns of one matrix launch over a chunk of nt <= LSK_EXPECT_CHUNK terms: all of them while nt * Ka * Kb stays within
 * 8 LSK_EXPECT_CHUNK partial sums per block; else the ket columns are cut first, to the most whole chunks of 8 that fit (at least
 * one, as nt <= LSK_EXPECT_CHUNK), and then the bra columns, to the most that fit beside them (whole chunks of 8 where 8 fit) */
static void expect_matrix_cols(int nt, int Ka, int Kb, int *kal, int *kbl) {
    int64_t const cap = 8 * (int64_t)LSK_EXPECT_CHUNK / nt; /* >= 8 */
    if ((int64_t)Ka * Kb <= cap) { *kal = Ka; *kbl = Kb; return; }
    int64_t b = cap / 8 * 8;
    if (b > Kb) b = Kb;
    int64_t a = cap / b;
    if (a >= 8) a = a / 8 * 8;
    if (a > Ka) a = Ka;
    *kal = (int)a; *kbl = (int)b;
}

/* where launch (chunk of terms [t0, t0 + nt); bra columns from a0, kla of them; ket columns from b0) writes in d_mat_out: the chunks
 * of terms follow each other, within one the ranges of bra columns, within those the ranges of ket columns */
static size_t expect_matrix_at(int t0, int nt, int Ka, int Kb, int a0, int kla, int b0) {
    return (size_t)t0 * (size_t)Ka * (size_t)Kb + (size_t)nt * ((size_t)a0 * (size_t)Kb + (size_t)kla * (size_t)b0);
}

int ls_amd_expect_matrix_elements(ls_amd_expect *pl, ls_amd_dtype dtype, int Ka, void const *d_bra, int64_t bra_row, int64_t bra_col, int Kb,
                                  void const *d_ket, int64_t ket_row, int64_t ket_col, double *h_out, void *stream) {
    char const *who = "ls_amd_expect_matrix_elements";
    if (!pl || !d_bra || !d_ket) return set_error("%s: NULL %s", who, !pl ? "plan" : !d_bra ? "bra block" : "ket block");
    if (Ka < 1 || Ka > 64) return set_error("%s: Ka = %d is outside [1, 64]", who, Ka);
    if (Kb < 1 || Kb > 64) return set_error("%s: Kb = %d is outside [1, 64]", who, Kb);
    expect_block const blk[2] = { { "the bra block", Ka, bra_row, bra_col }, { "the ket block", Kb, ket_row, ket_col } };
    if (expect_check_args(who, pl, dtype, h_out, blk, 2) != 0) return -1;
    int const cplx = dtype == LS_AMD_C128, nc = cplx ? 2 : 1;
    size_t const w = 8 * (size_t)nc;
    char const *const bra = (char const *)d_bra, *const ket = (char const *)d_ket;
    /* the buffers of the matrix calls: allocated here, at the first call, and grown by a call with more pairs of columns */
    size_t part = 1;
    for (int c = 0; c < pl->n_chunks; ++c) {
        int const nt = expect_chunk_of(pl, c).nt;
        int kal, kbl;
        expect_matrix_cols(nt, Ka, Kb, &kal, &kbl);
        size_t const v = (size_t)nt * (size_t)kal * (size_t)kbl;
        if (v > part) part = v;
    }
    part *= (size_t)lsk_corr_blocks(pl->n);
    if (expect_grow(who, &pl->d_mat_partial, NULL, &pl->mat_partial_vals, part) != 0) return -1;
    size_t const pairs = (size_t)Ka * (size_t)Kb;
    size_t const vals = (size_t)(pl->n_terms > 0 ? pl->n_terms : 1) * pairs;
    if (expect_grow(who, &pl->d_mat_out, &pl->h_mat_out, &pl->mat_out_vals, vals) != 0) return -1;
    /* the launches: per chunk of terms, per range of bra columns, per range of ket columns; a launch writes
     * R[((u - t0) kla + (a - a0)) klb + (b - b0)] of its nt terms at expect_matrix_at() of d_mat_out */
    for (int c = 0; c < pl->n_chunks; ++c) {
        expect_chunk const ck = expect_chunk_of(pl, c);
        int const g0 = ck.g0, g1 = ck.g1, t0 = ck.t0, nt = ck.nt;
        int kal, kbl;
        expect_matrix_cols(nt, Ka, Kb, &kal, &kbl);
        for (int a0 = 0; a0 < Ka; a0 += kal) {
            int const kla = Ka - a0 < kal ? Ka - a0 : kal;
            for (int b0 = 0; b0 < Kb; b0 += kbl) {
                int const klb = Kb - b0 < kbl ? Kb - b0 : kbl;
                DEV(lsk_expect_mat(pl->bs, pl->six, pl->gtab ? pl->gtab->tab : no_gtab(), pl->cons, g1 - g0, pl->d_groups + g0, pl->d_terms, t0,
                                   nt, cplx, pl->n, pl->d_reps, pl->d_norms, kla, bra + (size_t)a0 * (size_t)bra_col * w, bra_row, bra_col, klb,
                                   ket + (size_t)b0 * (size_t)ket_col * w, ket_row, ket_col, pl->d_mat_partial,
                                   pl->d_mat_out + expect_matrix_at(t0, nt, Ka, Kb, a0, kla, b0) * nc, pl->d_err, stream));
            }
        }
    }
    if (expect_finish_launches(pl, stream) != 0) return -1;
    if (pl->n_terms > 0) DEV(lsk_d2h(pl->h_mat_out, pl->d_mat_out, w * (size_t)pl->n_terms * pairs));
    for (size_t k = 0; k < 2 * (size_t)pl->n_ops * pairs; ++k) h_out[k] = 0.0;
    /* value[k][a][b] = sum_u w[k][u] R[u][a][b]: the loop of ls_amd_expect_values per pair (comb_u ascends: the chunk follows it) */
    int ch = 0;
    for (size_t i = 0; i < pl->n_comb; ++i) {
        int const u = pl->comb_u[i];
        while (u >= pl->h_groups[pl->chunk_first[ch + 1] - 1].end) ++ch;
        int const t0 = expect_chunk_of(pl, ch).t0, nt = expect_chunk_of(pl, ch).nt;
        int kal, kbl;
        expect_matrix_cols(nt, Ka, Kb, &kal, &kbl);
        double const wr = pl->comb_w[2 * i], wi = pl->comb_w[2 * i + 1];
        double *const o = h_out + 2 * (size_t)pl->comb_k[i] * pairs;
        for (int a = 0; a < Ka; ++a) {
            int const a0 = a / kal * kal, kla = Ka - a0 < kal ? Ka - a0 : kal;
            for (int b = 0; b < Kb; ++b) {
                int const b0 = b / kbl * kbl, klb = Kb - b0 < kbl ? Kb - b0 : kbl;
                size_t const at = expect_matrix_at(t0, nt, Ka, Kb, a0, kla, b0) + ((size_t)(u - t0) * (size_t)kla + (size_t)(a - a0)) * (size_t)klb
                                  + (size_t)(b - b0);
                double const rr = cplx ? pl->h_mat_out[2 * at] : pl->h_mat_out[at], ri = cplx ? pl->h_mat_out[2 * at + 1] : 0.0;
                double *const v = o + 2 * ((size_t)a * (size_t)Kb + (size_t)b);
                v[0] += wr * rr - wi * ri;
                v[1] += wr * ri + wi * rr;
            }
        }
    }
    return 0;
}
