// linesearch.inc -- part of qpdo_dev.hip (one translation unit; included in order): exact linesearch: radix sort, scans, search
// ------------------------------------------------------------------------------------------------
// Exact linesearch (linesearch.c:74-158): stable LSD radix sort of the 2m breakpoints on the
// 64-bit pattern of t (positive doubles order as unsigned integers; non-candidates carry a
// sentinel key and sort last; ties keep index order like glibc's merge-sort qsort; the sorting
// pass is scan_sort.inc's), then an exclusive scan of the slope/intercept increments and a
// first-crossing search.
// ------------------------------------------------------------------------------------------------
static const int RS_ITEMS = 8;                       // keys per thread per tile of the sort
static const int RS_TILE = BLK * RS_ITEMS;           // 2048

static const int LS_ITEMS = 4;
static const int LS_TILE = BLK * LS_ITEMS;           // 1024 breakpoints per block
// per-block exclusive scan of (da, db) over the sorted breakpoints; block totals to bt
__global__ __launch_bounds__(256) void k_ls_scan1(const Ctrl *__restrict__ ctrl, const u32 *__restrict__ idx,
                                                  const double *__restrict__ delta, const double *__restrict__ alpha,
                                                  double *__restrict__ pa, double *__restrict__ pb, double *__restrict__ bt, int nblk) {
    __shared__ double sa[256], sb[256];
    const int nL = ctrl->cnt[C_NL];
    const int base = blockIdx.x * LS_TILE + threadIdx.x * LS_ITEMS;
    double da[LS_ITEMS], db[LS_ITEMS], ta = 0.0, tb = 0.0;
#pragma unroll
    for (int j = 0; j < LS_ITEMS; j++) {
        const int k = base + j;
        da[j] = 0.0; db[j] = 0.0;
        if (k < nL) {
            const u32 iz = idx[k];
            const double dl = delta[iz], al = alpha[iz];
            if (dl > 0) { da[j] = dl * dl; db[j] = -(dl * al); }      // linesearch.c:135-137
            else        { da[j] = -(dl * dl); db[j] = dl * al; }      // linesearch.c:138-140
        }
        ta += da[j]; tb += db[j];
    }
    sa[threadIdx.x] = ta; sb[threadIdx.x] = tb;
    __syncthreads();
    if (threadIdx.x == 0) {
        double ra = 0.0, rb = 0.0;
        for (int i = 0; i < 256; i++) { double t1 = sa[i], t2 = sb[i]; sa[i] = ra; sb[i] = rb; ra += t1; rb += t2; }
        bt[blockIdx.x] = ra; bt[nblk + blockIdx.x] = rb;
    }
    __syncthreads();
    double ra = sa[threadIdx.x], rb = sb[threadIdx.x];
#pragma unroll
    for (int j = 0; j < LS_ITEMS; j++) {
        const int k = base + j;
        if (k < nL) { pa[k] = ra; pb[k] = rb; }
        ra += da[j]; rb += db[j];
    }
}
// one block: a0, b0 from the partial sums (linesearch.c:19-25,119-120), exclusive scan of block totals
__global__ __launch_bounds__(256) void k_ls_scan2(Ctrl *ctrl, const double *__restrict__ part, int pm, int pn, double *__restrict__ bt, int nblk) {
    __shared__ double sm[32];
    const double eta_m = reduce_partials(part + P_ETA_M * PGRID, pm, sm);
    const double beta_m = reduce_partials(part + P_BETA_M * PGRID, pm, sm + 16);
    const double ja = reduce_partials(part + P_A0 * PGRID, pm, sm);
    const double jb = reduce_partials(part + P_B0 * PGRID, pm, sm + 16);
    const double dxQdx = reduce_partials(part + P_DXQDX * PGRID, pn, sm);
    const double dxdf = reduce_partials(part + P_DXDF * PGRID, pn, sm + 16);
    if (threadIdx.x == 0) {
        double eta = eta_m; eta += dxQdx; eta *= 0.5;
        double beta = beta_m; beta += dxdf; beta *= 0.5;
        ctrl->val[V_A0] = eta + ja;
        ctrl->val[V_B0] = beta - jb;
        ctrl->cnt[C_KSTAR] = 0x7fffffff;
        const int nL = ctrl->cnt[C_NL];
        const int used = (nL + LS_TILE - 1) / LS_TILE;
        double ra = 0.0, rb = 0.0;
        for (int i = 0; i < used; i++) {
            double t1 = bt[i], t2 = bt[nblk + i];
            bt[i] = ra; bt[nblk + i] = rb; ra += t1; rb += t2;
        }
        bt[2 * nblk] = ra; bt[2 * nblk + 1] = rb;     // grand totals
    }
}
__global__ __launch_bounds__(256) void k_ls_search(Ctrl *ctrl, const u64 *__restrict__ key, const double *__restrict__ pa,
                                                   const double *__restrict__ pb, const double *__restrict__ bt, int nblk) {
    const int nL = ctrl->cnt[C_NL];
    const double a0 = ctrl->val[V_A0], b0 = ctrl->val[V_B0];
    int best = 0x7fffffff;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nL; k += gridDim.x * blockDim.x) {
        const int blk = k / LS_TILE;
        const double a = a0 + (bt[blk] + pa[k]), b = b0 + (bt[nblk + blk] + pb[k]);
        const double t = __longlong_as_double((long long)key[k]);
        if (b + a * t > 0) { best = k; break; }       // ascending k per thread: first hit is its minimum
    }
    if (best != 0x7fffffff) atomicMin(&ctrl->cnt[C_KSTAR], best);
}
__global__ void k_ls_final(Ctrl *ctrl, const double *__restrict__ pa, const double *__restrict__ pb, const double *__restrict__ bt, int nblk) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int nL = ctrl->cnt[C_NL];
    const double a0 = ctrl->val[V_A0], b0 = ctrl->val[V_B0];
    const int ks = ctrl->cnt[C_KSTAR];
    double a, b;
    if (nL == 0) { a = a0; b = b0; }
    else if (ks >= nL) { a = a0 + bt[2 * nblk]; b = b0 + bt[2 * nblk + 1]; }
    else { const int blk = ks / LS_TILE; a = a0 + (bt[blk] + pa[ks]); b = b0 + (bt[nblk + blk] + pb[ks]); }
    ctrl->val[V_TAU] = -b / a;
}
// ---- the whole breakpoint search in ONE launch for 2m <= LS_SMALL_MAX (small problems: 28 launches -> 1) ----------------
// One 1024-thread workgroup: bitonic sort of the (key, index) pairs in LDS -- indices are distinct and start in ascending
// order, so the lexicographic order IS the stable order by key that the radix path produces -- then the same two-level
// exclusive scan as k_ls_scan1 / k_ls_scan2 (4 consecutive items per thread, 256 threads per sub-block, sub-block totals
// chained in order: identical operations in identical order, so tau carries the same bits as the multi-launch path), the
// first-crossing search and the final division.
// lane ^ J for every in-wave distance without the LDS crossbar: J = 1, 2, 4, 8 by DPP moves (quad permutes; xor 4 = row_half_mirror then the reversed quad, xor 8 =
// row_mirror then row_half_mirror).  The sixteen waves of k_ls_small share one crossbar, and 34 of the 55 stages of a 1024-element bitonic
// network have these distances: with ds_bpermute for all of them the network was bound by that pipe (12.5 us; tools/lab/ls_lab.hip).
template <int J> __device__ __forceinline__ u32 dpp_xor32(u32 v) {
    static_assert(J == 1 || J == 2 || J == 4 || J == 8 || J == 16 || J == 32, "in-wave distances");
    // distances 16 and 32: the gfx950 row swaps (v_permlane16_swap / v_permlane32_swap exchange the odd rows / the upper half of one
    // operand with the even rows / the lower half of the other; with both operands = v each lane finds its partner's value in one of the
    // two results -- checked against __shfl_xor in tools/lab/permlane_lab.hip)
    if constexpr (J == 32) { const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false); return (threadIdx.x & 32) ? r[0] : r[1]; }
    else if constexpr (J == 16) { const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false); return (threadIdx.x & 16) ? r[0] : r[1]; }
    else if constexpr (J == 1) return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
    else if constexpr (J == 2) return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);
    else if constexpr (J == 4) { const int t = __builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true); return (u32)__builtin_amdgcn_update_dpp(0, t, 0x1B, 0xF, 0xF, true); }
    else { const int t = __builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true); return (u32)__builtin_amdgcn_update_dpp(0, t, 0x141, 0xF, 0xF, true); }
}
template <int J> __device__ __forceinline__ void ls_stage_dpp(u64 &key, u32 &idx, int tid, int kk) {
    const u32 lo = dpp_xor32<J>((u32)key), hi = dpp_xor32<J>((u32)(key >> 32));
    const u64 pk = ((u64)hi << 32) | lo; const u32 pi = dpp_xor32<J>(idx);
    const bool mine_gt = (key > pk) || (key == pk && idx > pi);
    const bool up = ((tid & kk) == 0), lower = ((tid & J) == 0);
    const bool swap = lower ? (mine_gt == up) : (mine_gt != up);      // pair (i, i^j), i the lower position: exchanged iff (element i > element i^j) == up
    if (swap) { key = pk; idx = pi; }
}
// More than 1024 candidates (up to 8192): C = ceil(ncand / 1024) chunks of 1024 are sorted SIDE BY SIDE by the 1024-element bitonic network
// (thread t holds element t of every chunk: 55 stages, 45 of them in-wave, 10 through LDS), then every element finds its final position by
// counting, with a binary search per other chunk, the elements that sort before it -- (key, index) pairs are distinct, so the ranks are a
// permutation and the result is the one sorted order.  A 4096-element network (78 stages x 4 elements per thread; bound by the
// compare-exchange instructions of one CU) took 40 us for 2058 candidates; this takes 55 x 3 + the searches (tools/lab/ls_lab.hip).
// in: sk / si = the compacted candidates, sentinels up to 1024 C.  out: the sorted candidates in place (ranks are formed in registers while
// sk / si are only read; a barrier later every element goes to its slot).
static const int LS_CHUNKS = 8;
__device__ __forceinline__ void ls_sort_chunks(int ncand, u64 *sk, u32 *si, int tid) {
    const int C = (ncand + 1023) >> 10;                               // 2 .. 8
    u64 key[LS_CHUNKS]; u32 idx[LS_CHUNKS];
#pragma unroll
    for (int r = 0; r < LS_CHUNKS; r++) if (r < C) { key[r] = sk[1024 * r + tid]; idx[r] = si[1024 * r + tid]; }
    for (int kk = 2; kk <= 1024; kk <<= 1) {
        for (int j = kk >> 1; j >= 64; j >>= 1) {
            u64 pk[LS_CHUNKS]; u32 pi[LS_CHUNKS];
            {
                __syncthreads();                                      // the initial loads / the previous exchange have been read
#pragma unroll
                for (int r = 0; r < LS_CHUNKS; r++) if (r < C) { sk[1024 * r + tid] = key[r]; si[1024 * r + tid] = idx[r]; }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < LS_CHUNKS; r++) if (r < C) { pk[r] = sk[1024 * r + (tid ^ j)]; pi[r] = si[1024 * r + (tid ^ j)]; }
            }
            const bool up = ((tid & kk) == 0), lower = ((tid & j) == 0);
#pragma unroll
            for (int r = 0; r < LS_CHUNKS; r++) if (r < C) {
                const bool mine_gt = (key[r] > pk[r]) || (key[r] == pk[r] && idx[r] > pi[r]);
                const bool swap = lower ? (mine_gt == up) : (mine_gt != up);
                if (swap) { key[r] = pk[r]; idx[r] = pi[r]; }
            }
        }
#pragma unroll
        for (int r = 0; r < LS_CHUNKS; r++) if (r < C) {
            if (kk >= 64) ls_stage_dpp<32>(key[r], idx[r], tid, kk);
            if (kk >= 32) ls_stage_dpp<16>(key[r], idx[r], tid, kk);
            if (kk >= 16) ls_stage_dpp<8>(key[r], idx[r], tid, kk);
            if (kk >= 8) ls_stage_dpp<4>(key[r], idx[r], tid, kk);
            if (kk >= 4) ls_stage_dpp<2>(key[r], idx[r], tid, kk);
            ls_stage_dpp<1>(key[r], idx[r], tid, kk);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LS_CHUNKS; r++) if (r < C) { sk[1024 * r + tid] = key[r]; si[1024 * r + tid] = idx[r]; }
    __syncthreads();
    // ranks: own position + for every other chunk the number of its (real) elements below this one
    int rank[LS_CHUNKS];
#pragma unroll
    for (int r = 0; r < LS_CHUNKS; r++) {
        rank[r] = -1;
        if (r < C && tid < ncand - 1024 * r) {                        // a real element of chunk r (the sentinels sort behind them)
            int rk = tid;
#pragma unroll 1
            for (int q = 0; q < C; q++) {
                if (q == r) continue;
                int lo = 0, hi = ncand - 1024 * q; if (hi > 1024) hi = 1024;
                while (lo < hi) {                                     // first position of chunk q whose element is not below (key, idx)
                    const int mid = (lo + hi) >> 1;
                    const u64 mk = sk[1024 * q + mid];
                    const bool below = (mk < key[r]) || (mk == key[r] && si[1024 * q + mid] < idx[r]);
                    if (below) lo = mid + 1; else hi = mid;
                }
                rk += lo;
            }
            rank[r] = rk;
        }
    }
    __syncthreads();                                                  // every search has read the sorted chunks
#pragma unroll
    for (int r = 0; r < LS_CHUNKS; r++) if (rank[r] >= 0) { sk[rank[r]] = key[r]; si[rank[r]] = idx[r]; }
    __syncthreads();
}
static const int LS_SMALL_MAX = 8192;
#ifdef LS_TIMING
__device__ long long g_ls_t[16];
#define LS_T(k) do { if (threadIdx.x == 0) g_ls_t[k] = wall_clock64(); } while (0)
#else
#define LS_T(k) do { } while (0)
#endif
struct LsProd { int tpr, nrows; const int *rp, *ci; const double *val, *x; double *y; };
__global__ __launch_bounds__(1024) void k_ls_small(Ctrl *ctrl, const double *__restrict__ part, int pm, int pn, const u64 *__restrict__ key_in,
                                                   const double *__restrict__ delta, const double *__restrict__ alpha, int M2, int spec = 0,
                                                   LsProd lp = LsProd{}) {
    if (spec && ctrl->cnt[C_SPEC_SKIP]) return;                        // launch-ahead (vector.inc SpecArgs): this pass is not a Newton step
    if (blockIdx.x > 0) {
        // launch-ahead route: A'dy of this step (needed by the iterate update only, not by the search) as extra workgroups of this launch;
        // spmv_rows, the row loop of k_spmv: the same bits
        EpiStore e{lp.y};
        spmv_rows((int)blockIdx.x - 1, (int)gridDim.x - 1, lp.tpr, lp.nrows, lp.rp, lp.ci, lp.val, lp.x, e, 1024);
        return;
    }
    constexpr int NSUB = LS_SMALL_MAX / LS_TILE;                       // 8 sub-blocks of 1024 items = two "virtual threads" per thread
    constexpr int NVT = NSUB / 4;
    __shared__ __attribute__((aligned(16))) u64 sk[LS_SMALL_MAX];
    __shared__ u32 si[LS_SMALL_MAX];
    __shared__ double sa[NSUB * 256], sb[NSUB * 256];
    __shared__ double bta[NSUB + 1], btb[NSUB + 1];
    __shared__ double sm6[96];
    __shared__ int kstar;
    __shared__ double sdl[1024], sal[1024];
    const int tid = threadIdx.x;
    LS_T(0);
    if (tid == 0) kstar = 0x7fffffff;
    // everything this launch reads from global memory that does not depend on the sorted order is requested here, in front of the sort,
    // so that the sort hides the round trips (each ~1-2 us on a chain of dependent phases): the number of breakpoints, the partial sums of
    // the two products (thread sums in the order of the loops they replace), and -- up to 1024 candidates -- delta and alpha themselves,
    // gathered from LDS afterwards
    const int nL = ctrl->cnt[C_NL];
    double eta_m = 0.0, beta_m = 0.0, ja = 0.0, jb = 0.0, dxQdx = 0.0, dxdf = 0.0;
    for (int i = tid; i < pm; i += 1024) { eta_m += part[P_ETA_M * PGRID + i]; beta_m += part[P_BETA_M * PGRID + i]; ja += part[P_A0 * PGRID + i]; jb += part[P_B0 * PGRID + i]; }
    for (int i = tid; i < pn; i += 1024) { dxQdx += part[P_DXQDX * PGRID + i]; dxdf += part[P_DXDF * PGRID + i]; }
    const bool lds_gather = M2 <= 1024;
    if (lds_gather) { sdl[tid] = tid < M2 ? delta[tid] : 0.0; sal[tid] = tid < M2 ? alpha[tid] : 0.0; }
    // Only the nL candidates with a positive ratio are breakpoints; the others carry the sentinel key, sort behind them and are never
    // looked at.  They are dropped BEFORE the sort -- compacted in index order, which is the order the index tie-break wants -- so the
    // network sorts the candidates that matter (typically half of the 2m: a bitonic network on one CU is bound by its compare-exchange
    // instructions).  Slab r = the candidates 1024 r .. 1024 r + 1023, one per thread.
    __shared__ int wcnt[LS_CHUNKS * 16], wbase[LS_CHUNKS * 16], s_total;
    {
        u64 k_in[LS_CHUNKS]; bool real[LS_CHUNKS]; int inw[LS_CHUNKS];
        const int w = tid >> 6, l = tid & 63;
        const u64 lt = (1ull << l) - 1ull;
#pragma unroll
        for (int r = 0; r < LS_CHUNKS; r++) {
            real[r] = false; inw[r] = 0;
            if (1024 * r < M2) {
                const int e = tid + 1024 * r;
                k_in[r] = e < M2 ? key_in[e] : KEY_SENTINEL;
                real[r] = k_in[r] != KEY_SENTINEL;
                const u64 mk = __ballot(real[r]);
                inw[r] = __popcll(mk & lt);
                if (l == 0) wcnt[r * 16 + w] = __popcll(mk);
            } else if (l == 0) wcnt[r * 16 + w] = 0;
        }
        __syncthreads();
        if (w == 0) {                                                  // exclusive prefix of the 128 (slab, wave) counts, two per lane
            const int c0 = wcnt[l], c1 = wcnt[64 + l];
            int i0 = c0, i1 = c1;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t0 = __shfl_up(i0, o, 64), t1 = __shfl_up(i1, o, 64); if (l >= o) { i0 += t0; i1 += t1; } }
            const int tot0 = __shfl(i0, 63, 64);
            wbase[l] = i0 - c0; wbase[64 + l] = tot0 + i1 - c1;
            if (l == 63) s_total = tot0 + i1;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < LS_CHUNKS; r++) if (real[r]) { const int pos = wbase[r * 16 + w] + inw[r]; sk[pos] = k_in[r]; si[pos] = (u32)(tid + 1024 * r); }
    }
    const int ncand = s_total;
    LS_T(1);
    int np2c = 1; while (np2c < ncand) np2c <<= 1;
    {
        const int fill_to = ncand <= 1024 ? 1024 : 1024 * ((ncand + 1023) >> 10);
        for (int e = ncand + tid; e < fill_to; e += 1024) { sk[e] = KEY_SENTINEL; si[e] = 0xFFFFFFFFu; }
    }
    __syncthreads();
    if (ncand <= 1024) {
        // One element per thread, held in registers.  Compare-exchange stages at in-wave distances are DPP moves / row swaps; those with
        // distance >= 64 exchange through LDS (two buffers, one barrier each).
        u64 key = sk[tid];
        u32 idx = si[tid];
        u64 *xk = sk + 1024;                        // exchange buffers: 2 x 1024 keys in the unused upper part of sk, indices in si
        u32 *xi = si + 1024;
        int buf = 0;
        for (int kk = 2; kk <= np2c; kk <<= 1) {
            for (int j = kk >> 1; j >= 64; j >>= 1) {
                u64 pk; u32 pi;
                {
                    xk[buf * 1024 + tid] = key; xi[buf * 1024 + tid] = idx;
                    __syncthreads();
                    pk = xk[buf * 1024 + (tid ^ j)]; pi = xi[buf * 1024 + (tid ^ j)];
                    buf ^= 1;
                }
                const bool mine_gt = (key > pk) || (key == pk && idx > pi);
                const bool up = ((tid & kk) == 0), lower = ((tid & j) == 0);
                // pair (i, i^j), i the lower position: exchanged iff (element i > element i^j) == up
                const bool swap = lower ? (mine_gt == up) : (mine_gt != up);
                if (swap) { key = pk; idx = pi; }
            }
            if ((tid & ~63) < np2c) {             // in-wave distances: row swaps and DPP moves (a wave of sentinels only has nothing to exchange)
                if (kk >= 64) ls_stage_dpp<32>(key, idx, tid, kk);
                if (kk >= 32) ls_stage_dpp<16>(key, idx, tid, kk);
                if (kk >= 16) ls_stage_dpp<8>(key, idx, tid, kk);
                if (kk >= 8) ls_stage_dpp<4>(key, idx, tid, kk);
                if (kk >= 4) ls_stage_dpp<2>(key, idx, tid, kk);
                ls_stage_dpp<1>(key, idx, tid, kk);
            }
        }
        __syncthreads();                          // (every thread has read its element of sk / si)
        sk[tid] = key; si[tid] = idx;
        __syncthreads();
    } else ls_sort_chunks(ncand, sk, si, tid);
    LS_T(2);
    // a0, b0 (k_ls_scan2)
    // the six block sums of k_ls_scan2 with one pair of barriers (per value the operations of reduce_partials: strided thread sums,
    // wave sums, the wave totals added in order -- the same bits)
    {
        const int w = tid >> 6, l = tid & 63;
        // (waves beyond the partials carry +0.0 in all six: their wave sums are +0.0 without the 72 shuffles)
        if (w < (((pm > pn ? pm : pn) + 63) >> 6)) { eta_m = wave_sum(eta_m); beta_m = wave_sum(beta_m); ja = wave_sum(ja); jb = wave_sum(jb); dxQdx = wave_sum(dxQdx); dxdf = wave_sum(dxdf); }
        if (l == 0) { sm6[w] = eta_m; sm6[16 + w] = beta_m; sm6[32 + w] = ja; sm6[48 + w] = jb; sm6[64 + w] = dxQdx; sm6[80 + w] = dxdf; }
        __syncthreads();
        double t0 = sm6[0], t1 = sm6[16], t2 = sm6[32], t3 = sm6[48], t4 = sm6[64], t5 = sm6[80];
#pragma nounroll
        for (int i = 1; i < 16; i++) { t0 += sm6[i]; t1 += sm6[16 + i]; t2 += sm6[32 + i]; t3 += sm6[48 + i]; t4 += sm6[64 + i]; t5 += sm6[80 + i]; }
        eta_m = t0; beta_m = t1; ja = t2; jb = t3; dxQdx = t4; dxdf = t5;
    }
    double eta = eta_m; eta += dxQdx; eta *= 0.5;
    double beta = beta_m; beta += dxdf; beta *= 0.5;
    const double a0 = eta + ja, b0 = beta - jb;
    LS_T(3);
    // per-thread items and totals (k_ls_scan1: thread t of block q owns items q*1024 + t*4 .. +3).  A thread plays the virtual threads
    // vt = tid + 1024 h: sub-block q = vt / 256, thread tl = vt % 256 of it; the second one only beyond 4096 breakpoints.
    const int nvt = nL > 4 * LS_TILE ? NVT : 1;
    double da[NVT][LS_ITEMS], db[NVT][LS_ITEMS];
#pragma unroll
    for (int h = 0; h < NVT; h++) {
        if (h < nvt) {
            const int vt = tid + 1024 * h, base = vt * LS_ITEMS;
            double ta = 0.0, tb = 0.0;
#pragma unroll
            for (int j = 0; j < LS_ITEMS; j++) {
                const int k = base + j;
                da[h][j] = 0.0; db[h][j] = 0.0;
                if (k < nL) {
                    const u32 iz = si[k];
                    const double dl = lds_gather ? sdl[iz] : delta[iz], al = lds_gather ? sal[iz] : alpha[iz];
                    if (dl > 0) { da[h][j] = dl * dl; db[h][j] = -(dl * al); }
                    else        { da[h][j] = -(dl * dl); db[h][j] = dl * al; }
                }
                ta += da[h][j]; tb += db[h][j];
            }
            sa[vt] = ta; sb[vt] = tb;
        }
    }
    __syncthreads();
    LS_T(4);
    const int used_sub = (nL + LS_TILE - 1) / LS_TILE;
    if ((tid & 127) == 0 && (tid >> 7) < used_sub) {   // one lane per used sub-block (eight different waves): sequential exclusive scan of its
        // 256 thread totals (the order of k_ls_scan1), eight at a time: the loads of a group are issued before its dependent additions
        const int q = tid >> 7;
        double ra = 0.0, rb = 0.0;
        double *pa = sa + q * 256, *pb = sb + q * 256;
        // (only the threads that own items: the totals behind them are +0.0, and adding +0.0 leaves a running sum that started at +0.0
        // unchanged bit for bit -- with 2m = 200 the scan is 7 groups instead of 32)
        const int used_thr = (((nL - q * LS_TILE < LS_TILE ? nL - q * LS_TILE : LS_TILE) + LS_ITEMS - 1) / LS_ITEMS + 7) & ~7;
#pragma nounroll
        for (int i = 0; i < used_thr; i += 8) {     // (left to itself the compiler unrolls all 32 trips and spills 128 VGPRs to scratch)
            double va[8], vb[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { va[u] = pa[i + u]; vb[u] = pb[i + u]; }
#pragma unroll
            for (int u = 0; u < 8; u++) { const double t1 = va[u], t2 = vb[u]; va[u] = ra; vb[u] = rb; ra += t1; rb += t2; }
#pragma unroll
            for (int u = 0; u < 8; u++) { pa[i + u] = va[u]; pb[i + u] = vb[u]; }
        }
        bta[q] = ra; btb[q] = rb;
    }
    __syncthreads();
    if (tid == 0) {         // k_ls_scan2: sub-block totals chained in order over the used sub-blocks
        double ra = 0.0, rb = 0.0;
        for (int i = 0; i < used_sub; i++) { const double t1 = bta[i], t2 = btb[i]; bta[i] = ra; btb[i] = rb; ra += t1; rb += t2; }
        bta[NSUB] = ra; btb[NSUB] = rb;
    }
    __syncthreads();
    LS_T(5);
    // first crossing (k_ls_search): prefix of item k = sub-block base + (thread prefix + running sum inside the thread)
    int best = 0x7fffffff; double abest = 0.0, bbest = 0.0;
#pragma unroll
    for (int h = 0; h < NVT; h++) {
        if (h < nvt) {
            const int vt = tid + 1024 * h, base = vt * LS_ITEMS, q = vt >> 8;
            double ra = sa[vt], rb = sb[vt];
#pragma unroll
            for (int j = 0; j < LS_ITEMS; j++) {
                const int k = base + j;
                if (k < nL && best == 0x7fffffff) {
                    const double a = a0 + (bta[q] + ra), b = b0 + (btb[q] + rb);
                    const double t = __longlong_as_double((long long)sk[k]);
                    if (b + a * t > 0) { best = k; abest = a; bbest = b; }
                }
                ra += da[h][j]; rb += db[h][j];
            }
        }
    }
    if (best != 0x7fffffff) atomicMin(&kstar, best);
    __syncthreads();
    const int ks = kstar;
    LS_T(6);
    if (nL == 0 || ks >= nL) {
        if (tid == 0) {
            const double a = nL == 0 ? a0 : a0 + bta[NSUB], b = nL == 0 ? b0 : b0 + btb[NSUB];
            ctrl->val[V_A0] = a0; ctrl->val[V_B0] = b0; ctrl->cnt[C_KSTAR] = ks;
            ctrl->val[V_TAU] = -b / a;
        }
    } else if (best == ks) {       // exactly one thread found the minimum index
        ctrl->val[V_A0] = a0; ctrl->val[V_B0] = b0; ctrl->cnt[C_KSTAR] = ks;
        ctrl->val[V_TAU] = -bbest / abest;
    }
}
// standalone prep for the linesearch parity entry point (caller supplies eta, beta, delta, alpha)
__global__ __launch_bounds__(256) void k_ls_prep_raw(int M2, const double *__restrict__ delta, const double *__restrict__ alpha,
                                                     u64 *__restrict__ key, u32 *__restrict__ idx, double *__restrict__ p_a0,
                                                     double *__restrict__ p_b0, Ctrl *ctrl) {
    __shared__ double sm[32];
    double a0 = 0.0, b0 = 0.0; int nL = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M2; i += gridDim.x * blockDim.x) {
        const double dl = delta[i], al = alpha[i], t = al / dl;
        const bool L = t > 0, P = dl > 0;
        key[i] = L ? (u64)__double_as_longlong(t) : KEY_SENTINEL;
        idx[i] = (u32)i;
        if (L) nL++;
        if (L != P) { a0 += dl * dl; b0 += dl * al; }
    }
    double t3 = block_sum(a0, sm), t4 = block_sum(b0, sm + 16);
    int tn = block_sum_int(nL, (int *)sm);
    if (threadIdx.x == 0) { p_a0[blockIdx.x] = t3; p_b0[blockIdx.x] = t4; if (tn) atomicAdd(&ctrl->cnt[C_NL], tn); }
}
__global__ void k_set_partial(double *p, double v) { if (threadIdx.x == 0 && blockIdx.x == 0) p[0] = v; }
__global__ void k_ctrl_set_int(Ctrl *c, int slot, int v) { if (threadIdx.x == 0 && blockIdx.x == 0) c->cnt[slot] = v; }
__global__ void k_ctrl_set_nrm0(Ctrl *c, int slot) { if (threadIdx.x == 0 && blockIdx.x == 0) c->nrm[slot] = 0ull; }
// read-back without the copy engine: one wave writes the control block into the host's pinned copy and then, system-scope released, the
// sequence word the host is spinning on (host_core.inc read_ctrl_block)
__global__ __launch_bounds__(64) void k_ctrl_publish(const Ctrl *__restrict__ c, Ctrl *host, u64 *hseq, u64 seq) {
    const u64 *src = (const u64 *)c; u64 *dst = (u64 *)host;
    if (threadIdx.x < sizeof(Ctrl) / 8) dst[threadIdx.x] = src[threadIdx.x];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(hseq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}


