/*
 * band_order.c -- reverse Cuthill-McKee on the pattern of Q + A'A, and the configuration of the band solver's variable order
 * (band_order.h; contracts: include/qpdo_amd_ext.h).  Pure host code, no HIP.
 *
 * The graph: variables i, j are adjacent when Q stores (i, j) or (j, i) -- on the stored triangle for stype != 0, as the setup
 * reads Q -- or when a row of A stores both.  Explicit zeros count (band_detect counts them too).  A'A is never formed: the
 * breadth-first search walks Q's neighbour lists and, through the columns of A, the ROWS that hold a vertex; a row is expanded
 * once per search, the first time one of its columns is reached (everything it holds is visited then, so a second expansion
 * could add nothing).  One search is O(nnz); a component gets at most 8 + 3 of them.
 *
 * Degrees are EXACT (the number of distinct neighbours: the union of a vertex's Q-neighbours and of the columns of its rows), not the
 * O(nnz) bound Q-neighbours + sum of (row length - 1), which counts a pair of columns once per row that holds both.  The union costs
 * sum over the rows of (row length)^2, at most 1024 nnz(A) behind the early out below and a small multiple of nnz on chain QPs, whose
 * rows are short.  It buys the order's quality: on the test family the exact degrees reproduce scipy's reverse_cuthill_mckee
 * bandwidths (18 / 41 / 83 / 190); the bound gave 21 / 47-48 / 94 / 204 (tests/test_band_order_cpu.py).
 *
 * A row of A with more than 1024 entries forces a half-bandwidth above 1023 under every order: the identity comes back at once
 * (early_out), before anything is built -- which also bounds the work on matrices with dense rows.
 *
 * Per connected component, components in order of their smallest index:
 *   root   the vertex of smallest (degree, index); then George-Liu: re-root at the smallest (degree, index) of the last level of
 *          the rooted level structure while that makes the structure deeper, at most 8 rounds;
 *   order  breadth-first from the root; the unvisited neighbours of a parent are appended in ascending (degree, index).
 * The concatenation is reversed.  No hashing, no address-dependent order, no threads: the same pattern gives the same newold.
 */
#include "band_order.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define BAND_ORDER_MAX_ROW 1024          /* a longer row of A forces a half-bandwidth above 1023 under every order */
#define BAND_ORDER_GL_ROUNDS 8

static inline int64_t bo_idx(const void *a, int itype, int64_t k) {
    return itype == 0 ? (int64_t)((const int32_t *)a)[k] : (int64_t)((const int64_t *)a)[k];
}
/* is the stored entry (i, j) of Q one the setup reads?  (stype -1: the lower triangle, +1: the upper, 0: all) */
static inline int bo_q_entry(int stype, int64_t i, int64_t j) { return stype == 0 || (stype < 0 ? i >= j : i <= j); }

long band_order_bandwidth(const cholmod_sparse *Q, const cholmod_sparse *A, const int32_t *oldnew) {
    const int64_t n = (int64_t)Q->ncol, m = A ? (int64_t)A->nrow : 0;
    int64_t b = 0;
    for (int64_t j = 0; j < n; j++) {
        const int64_t pj = oldnew ? oldnew[j] : j;
        for (int64_t k = bo_idx(Q->p, Q->itype, j); k < bo_idx(Q->p, Q->itype, j + 1); k++) {
            const int64_t i = bo_idx(Q->i, Q->itype, k);
            if (!bo_q_entry(Q->stype, i, j)) continue;
            const int64_t pi = oldnew ? oldnew[i] : i, s = pi > pj ? pi - pj : pj - pi;
            if (s > b) b = s;
        }
    }
    if (m > 0) {
        int32_t *lo = malloc((size_t)m * sizeof(int32_t)), *hi = malloc((size_t)m * sizeof(int32_t));
        if (!lo || !hi) { free(lo); free(hi); return -1; }
        for (int64_t r = 0; r < m; r++) { lo[r] = INT32_MAX; hi[r] = -1; }
        for (int64_t j = 0; j < n; j++) {
            const int32_t pj = (int32_t)(oldnew ? oldnew[j] : j);
            for (int64_t k = bo_idx(A->p, A->itype, j); k < bo_idx(A->p, A->itype, j + 1); k++) {
                const int64_t r = bo_idx(A->i, A->itype, k);
                if (pj < lo[r]) lo[r] = pj;
                if (pj > hi[r]) hi[r] = pj;
            }
        }
        for (int64_t r = 0; r < m; r++) if (hi[r] >= 0 && hi[r] - lo[r] > b) b = hi[r] - lo[r];
        free(lo); free(hi);
    }
    return (long)b;
}

/* the graph in the form the search walks: Q's neighbour lists (symmetric, no duplicates, no loops), CSR of A's pattern; the
 * columns of A are the caller's own arrays */
typedef struct {
    int32_t n, m;
    int64_t *qp; int32_t *qi;            /* neighbour lists of Q */
    int64_t *rp; int32_t *rc;            /* rows of A: their columns */
    const cholmod_sparse *A;
    int32_t *deg;                        /* exact degrees */
    int32_t *vmark, *rmark; int32_t stamp;      /* visited vertex / expanded row in the search that carries this stamp */
    int32_t *level_end;                  /* scratch of bo_bfs: see there */
    uint64_t *keys;                      /* scratch of bo_bfs: (degree, index) of one parent's new vertices */
} BoGraph;

static void bo_free(BoGraph *g) {
    free(g->qp); free(g->qi); free(g->rp); free(g->rc); free(g->deg); free(g->vmark); free(g->rmark); free(g->level_end); free(g->keys);
}
static int bo_key_cmp(const void *a, const void *b) {
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}
static int bo_build(BoGraph *g, const cholmod_sparse *Q, const cholmod_sparse *A) {
    const int32_t n = (int32_t)Q->ncol, m = A ? (int32_t)A->nrow : 0;
    memset(g, 0, sizeof(*g));
    g->n = n; g->m = m; g->A = A;
    const int64_t qnnz = bo_idx(Q->p, Q->itype, n), annz = m ? bo_idx(A->p, A->itype, n) : 0;
    g->qp = calloc((size_t)n + 2, sizeof(int64_t));
    g->qi = malloc((size_t)(2 * qnnz + 1) * sizeof(int32_t));
    g->rp = calloc((size_t)m + 2, sizeof(int64_t));
    g->rc = malloc((size_t)(annz + 1) * sizeof(int32_t));
    g->deg = malloc(((size_t)n + 1) * sizeof(int32_t));
    g->vmark = calloc((size_t)n + 1, sizeof(int32_t));
    g->rmark = calloc((size_t)m + 1, sizeof(int32_t));
    g->level_end = malloc(((size_t)n + 2) * sizeof(int32_t));
    g->keys = malloc(((size_t)n + 1) * sizeof(uint64_t));
    if (!g->qp || !g->qi || !g->rp || !g->rc || !g->deg || !g->vmark || !g->rmark || !g->level_end || !g->keys) return -1;
    /* Q: both directions of every stored off-diagonal entry (counting pass, fill pass), then duplicates out, list by list */
    int64_t *qp = g->qp;
    for (int pass = 0; pass < 2; pass++) {
        for (int32_t j = 0; j < n; j++)
            for (int64_t k = bo_idx(Q->p, Q->itype, j); k < bo_idx(Q->p, Q->itype, (int64_t)j + 1); k++) {
                const int64_t i = bo_idx(Q->i, Q->itype, k);
                if (i == j || !bo_q_entry(Q->stype, i, j)) continue;
                if (pass == 0) { qp[i + 2]++; qp[j + 2]++; }
                else { g->qi[qp[i + 1]++] = j; g->qi[qp[j + 1]++] = (int32_t)i; }
            }
        if (pass == 0) for (int32_t v = 0; v < n; v++) qp[v + 2] += qp[v + 1];      /* qp[v + 1] = start of list v: the fill pass moves it to its end */
    }
    {   /* now qp[v + 1] = end of list v, qp[0] = 0 = start of list 0: compact in place; vmark[w] = v + 1 marks "w seen in list v" */
        int64_t out = 0, beg = 0;
        for (int32_t v = 0; v < n; v++) {
            const int64_t end = qp[v + 1];
            qp[v] = out;
            for (int64_t k = beg; k < end; k++) { const int32_t w = g->qi[k]; if (g->vmark[w] != v + 1) { g->vmark[w] = v + 1; g->qi[out++] = w; } }
            beg = end;
        }
        qp[n] = out;
        memset(g->vmark, 0, ((size_t)n + 1) * sizeof(int32_t));
    }
    /* rows of A */
    int64_t *rp = g->rp;
    if (m) {
        for (int64_t k = 0; k < annz; k++) rp[bo_idx(A->i, A->itype, k) + 2]++;
        for (int32_t r = 0; r < m; r++) rp[r + 2] += rp[r + 1];
        for (int32_t j = 0; j < n; j++)
            for (int64_t k = bo_idx(A->p, A->itype, j); k < bo_idx(A->p, A->itype, (int64_t)j + 1); k++) g->rc[rp[bo_idx(A->i, A->itype, k) + 1]++] = j;
    }
    /* (rp[r] = start of row r, rp[r + 1] = its end, as qp) */
    /* exact degrees: the union of v's Q-neighbours and of the columns of its rows; vmark[w] = v + 1 marks "w counted for v" */
    for (int32_t v = 0; v < n; v++) {
        int32_t dg = 0;
        g->vmark[v] = v + 1;
        for (int64_t k = qp[v]; k < qp[v + 1]; k++) { const int32_t w = g->qi[k]; if (g->vmark[w] != v + 1) { g->vmark[w] = v + 1; dg++; } }
        if (m) for (int64_t k = bo_idx(A->p, A->itype, v); k < bo_idx(A->p, A->itype, (int64_t)v + 1); k++) {
            const int64_t r = bo_idx(A->i, A->itype, k);
            for (int64_t e = rp[r]; e < rp[r + 1]; e++) { const int32_t w = g->rc[e]; if (g->vmark[w] != v + 1) { g->vmark[w] = v + 1; dg++; } }
        }
        g->deg[v] = dg;
    }
    memset(g->vmark, 0, ((size_t)n + 1) * sizeof(int32_t));
    return 0;
}
/* Breadth-first search from root over its component, Cuthill-McKee's visiting order, into out[0 .. count).  Returns count;
 * *nlevels = the depth of the rooted level structure, g->level_end[l] = the end in out of level l. */
static int32_t bo_bfs(BoGraph *g, int32_t root, int32_t *out, int32_t *nlevels) {
    const cholmod_sparse *A = g->A;
    const int32_t st = ++g->stamp;
    int32_t head = 0, tail = 0, lev = 0, lev_end = 1;
    out[tail++] = root; g->vmark[root] = st;
    while (head < tail) {
        if (head == lev_end) { g->level_end[lev++] = lev_end; lev_end = tail; }
        const int32_t v = out[head++];
        int32_t cnt = 0;
        for (int64_t k = g->qp[v]; k < g->qp[v + 1]; k++) {
            const int32_t w = g->qi[k];
            if (g->vmark[w] != st) { g->vmark[w] = st; g->keys[cnt++] = (uint64_t)(uint32_t)g->deg[w] << 32 | (uint32_t)w; }
        }
        if (g->m) for (int64_t k = bo_idx(A->p, A->itype, v); k < bo_idx(A->p, A->itype, (int64_t)v + 1); k++) {
            const int64_t r = bo_idx(A->i, A->itype, k);
            if (g->rmark[r] == st) continue;
            g->rmark[r] = st;
            for (int64_t e = g->rp[r]; e < g->rp[r + 1]; e++) {
                const int32_t w = g->rc[e];
                if (g->vmark[w] != st) { g->vmark[w] = st; g->keys[cnt++] = (uint64_t)(uint32_t)g->deg[w] << 32 | (uint32_t)w; }
            }
        }
        if (cnt > 1) qsort(g->keys, (size_t)cnt, sizeof(uint64_t), bo_key_cmp);
        for (int32_t c = 0; c < cnt; c++) out[tail++] = (int32_t)(uint32_t)g->keys[c];
    }
    g->level_end[lev++] = tail;
    *nlevels = lev;
    return tail;
}
static int32_t bo_min_deg(const BoGraph *g, const int32_t *v, int32_t beg, int32_t end) {
    int32_t best = v[beg];
    for (int32_t k = beg + 1; k < end; k++)
        if (g->deg[v[k]] < g->deg[best] || (g->deg[v[k]] == g->deg[best] && v[k] < best)) best = v[k];
    return best;
}

int qpdo_amd_band_order(const cholmod_sparse *Q, const cholmod_sparse *A, long *newold, long *info4) {
    if (!Q || !Q->p || !newold || (Q->itype != 0 && Q->itype != 2) || Q->nrow != Q->ncol || Q->ncol >= (size_t)INT32_MAX) return -1;
    if (A && (!A->p || (A->itype != 0 && A->itype != 2) || A->ncol != Q->ncol || A->nrow >= (size_t)INT32_MAX)) return -1;
    if (A && A->nrow == 0) A = NULL;
    const int32_t n = (int32_t)Q->ncol;
    long info[4] = {0, 0, 0, 0};
    for (int32_t k = 0; k < n; k++) newold[k] = k;
    const long bnat = band_order_bandwidth(Q, A, NULL);
    if (bnat < 0) return -1;
    info[0] = info[1] = bnat;
    BoGraph g;
    int32_t *order = NULL, *oldnew = NULL, *done = NULL;
    int rc = -1;
    memset(&g, 0, sizeof(g));
    if (n == 0) { rc = 0; goto out; }
    if (A) {                                                               /* the early out: before anything is built */
        const int64_t m = (int64_t)A->nrow, annz = bo_idx(A->p, A->itype, n);
        int32_t *len = calloc((size_t)m, sizeof(int32_t));
        if (!len) goto out;
        int over = 0;
        for (int64_t k = 0; k < annz; k++) over |= ++len[bo_idx(A->i, A->itype, k)] > BAND_ORDER_MAX_ROW;
        free(len);
        if (over) { info[3] = 1; rc = 0; goto out; }
    }
    if (bo_build(&g, Q, A)) goto out;
    order = malloc((size_t)n * sizeof(int32_t)); oldnew = malloc((size_t)n * sizeof(int32_t)); done = calloc((size_t)n, sizeof(int32_t));
    if (!order || !oldnew || !done) goto out;
    int32_t filled = 0;
    for (int32_t s = 0; s < n; s++) {
        if (done[s]) continue;
        int32_t *seg = order + filled, nlev = 0, nl2 = 0;
        int32_t cnt = bo_bfs(&g, s, seg, &nlev);                           /* the component, to find its smallest degree */
        int32_t root = bo_min_deg(&g, seg, 0, cnt);
        if (root != s) cnt = bo_bfs(&g, root, seg, &nlev);
        for (int round = 0; round < BAND_ORDER_GL_ROUNDS && nlev > 1; round++) {
            const int32_t cand = bo_min_deg(&g, seg, g.level_end[nlev - 2], cnt);
            bo_bfs(&g, cand, seg, &nl2);
            if (nl2 > nlev) { root = cand; nlev = nl2; }
            else { bo_bfs(&g, root, seg, &nlev); break; }                  /* (seg holds the root's order again) */
        }
        /* (all rounds used: seg holds the order of the last accepted root -- the search just run) */
        for (int32_t k = 0; k < cnt; k++) done[seg[k]] = 1;
        filled += cnt;
        info[2]++;
    }
    for (int32_t k = 0; k < n; k++) { newold[k] = order[n - 1 - k]; oldnew[order[n - 1 - k]] = k; }
    info[1] = band_order_bandwidth(Q, A, oldnew);
    rc = info[1] < 0 ? -1 : 0;
out:
    if (info4) memcpy(info4, info, sizeof(info));
    bo_free(&g);
    free(order); free(oldnew); free(done);
    return rc;
}

/* ---- configuration (qpdo_amd_band_order_config; read once per qpdo_setup through band_order_snapshot) -------------------------------- */
static pthread_mutex_t g_bo_mu = PTHREAD_MUTEX_INITIALIZER;
static int g_bo_mode = QPDO_AMD_BAND_ORDER_ENV;
static int32_t *g_bo_newold = NULL;
static long g_bo_n = 0;

int qpdo_amd_band_order_config(int mode, const long *newold, long n) {
    int32_t *copy = NULL;
    if (mode < QPDO_AMD_BAND_ORDER_ENV || mode > QPDO_AMD_BAND_ORDER_GIVEN) {
        printf("ERROR in %s: unknown mode %d\n", __func__, mode); fflush(stdout); return -1;
    }
    if (mode == QPDO_AMD_BAND_ORDER_GIVEN) {
        const char *why = NULL;
        if (!newold || n < 0 || n >= (long)INT32_MAX) why = "a given order needs newold and 0 <= n < 2^31 - 1";
        unsigned char *seen = why ? NULL : calloc((size_t)n + 1, 1);
        copy = why ? NULL : malloc(((size_t)n + 1) * sizeof(int32_t));
        if (!why && (!seen || !copy)) why = "out of memory";
        for (long k = 0; !why && k < n; k++) {
            if (newold[k] < 0 || newold[k] >= n || seen[newold[k]]) why = "newold is not a permutation of 0 .. n-1";
            else { seen[newold[k]] = 1; copy[k] = (int32_t)newold[k]; }
        }
        free(seen);
        if (why) { free(copy); printf("ERROR in %s: %s\n", __func__, why); fflush(stdout); return -1; }
    }
    pthread_mutex_lock(&g_bo_mu);
    free(g_bo_newold);
    g_bo_mode = mode; g_bo_newold = copy; g_bo_n = copy ? n : 0;
    pthread_mutex_unlock(&g_bo_mu);
    return 0;
}
int band_order_snapshot(long n, int *mode, int32_t **newold, char *msg, size_t msg_len) {
    int rc = 0;
    *newold = NULL;
    pthread_mutex_lock(&g_bo_mu);
    *mode = g_bo_mode;
    if (g_bo_mode == QPDO_AMD_BAND_ORDER_GIVEN) {
        if (g_bo_n != n) { snprintf(msg, msg_len, "the order given to qpdo_amd_band_order_config has %ld entries, the workspace %ld variables", g_bo_n, n); rc = -1; }
        else {
            *newold = malloc(((size_t)n + 1) * sizeof(int32_t));
            if (!*newold) { snprintf(msg, msg_len, "band order: out of memory"); rc = -1; }
            else if (n) memcpy(*newold, g_bo_newold, (size_t)n * sizeof(int32_t));
        }
    }
    pthread_mutex_unlock(&g_bo_mu);
    if (!rc && *mode == QPDO_AMD_BAND_ORDER_ENV) {
        const char *e = getenv("QPDO_BAND_ORDER");
        if (!e || !*e || !strcmp(e, "0")) *mode = QPDO_AMD_BAND_ORDER_NATURAL;
        else if (!strcmp(e, "rcm")) *mode = QPDO_AMD_BAND_ORDER_RCM;
        else { snprintf(msg, msg_len, "QPDO_BAND_ORDER=%s: expected \"rcm\" (unset, \"\" or \"0\": the caller's order)", e); rc = -1; }
    }
    return rc;
}
