// scan_sort.inc -- part of qpdo_dev.hip (one translation unit; included in order): the backend's exclusive integer scan and its stable radix pass
// ------------------------------------------------------------------------------------------------
// Every integer scan of the backend (flag words, row pointers of the per-pass copies, of the set-up's transposition and symmetric
// expansion, radix histograms) is k_scn_sums + k_scn_apply; every sorting pass (the linesearch's breakpoints, the transposition's entry
// positions) is k_radix_hist + k_radix_scatter.  Host wrappers: host_core.inc dev_scan, radix_pass.  Integers: any association gives
// the same result.
// ------------------------------------------------------------------------------------------------
// The scan runs on many workgroups, none of which waits for another: tile sums in one launch; in the next every workgroup adds up the sums
// of the tiles in front of its own and scans its tile (one tile: that launch alone).
// cnt and out may be the same array (every thread holds its items in registers before it stores); total (or null) receives the grand total.
// n may be anything up to INT_MAX: positions are 64-bit, the sums of a tile are not.  Every tile re-adds the sums in front of it, which is
// quadratic in the number of tiles: about 100 at the largest per-pass scan, 3052 at the set-up histogram of a matrix of 2e8 entries
// (18 MB of L2-resident reads in all), 32768 at the longest histogram the transposition can have (nnz < 2^31).
static const int SCN_ITEMS = 8;
static const int SCN_TILE = BLK * SCN_ITEMS;         // 2048
__global__ __launch_bounds__(256) void k_scn_sums(const int *__restrict__ cnt, int n, int *__restrict__ tsum) {
    __shared__ int ws[BLK / 64];
    const long long base = (long long)blockIdx.x * SCN_TILE + threadIdx.x * SCN_ITEMS;
    int s = 0;
#pragma unroll
    for (int u = 0; u < SCN_ITEMS; u++) if (base + u < n) s += cnt[base + u];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < BLK / 64; w++) t += ws[w]; tsum[blockIdx.x] = t; }
}
__global__ __launch_bounds__(256) void k_scn_apply(const int *cnt, int n, const int *__restrict__ tsum, int *out, int *__restrict__ total) {
    __shared__ int woff[BLK / 64], wtot[BLK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int off = 0;                                              // the tiles in front of this one
    for (int i = threadIdx.x; i < (int)blockIdx.x; i += BLK) off += tsum[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) off += __shfl_down(off, o, 64);
    const long long base = (long long)blockIdx.x * SCN_TILE + threadIdx.x * SCN_ITEMS;
    int v[SCN_ITEMS], s = 0;
#pragma unroll
    for (int u = 0; u < SCN_ITEMS; u++) { v[u] = base + u < n ? cnt[base + u] : 0; s += v[u]; }
    int inc = s;                                              // inclusive scan of the thread sums over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 0) woff[wave] = off;
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int run = inc - s;
    for (int w = 0; w < BLK / 64; w++) { run += woff[w]; if (w < wave) run += wtot[w]; }
#pragma unroll
    for (int u = 0; u < SCN_ITEMS; u++) { if (base + u < n) out[base + u] = run; run += v[u]; }
    if (total && blockIdx.x == gridDim.x - 1 && threadIdx.x == BLK - 1) *total = run;      // (items behind n count zero)
}
// ---- one pass of a stable LSD radix sort on the 8-bit digit at `shift` -----------------------------------------------------------
// K: key type; ITEMS: keys per thread (a block owns BLK * ITEMS consecutive keys); I: the type that counts keys.  The histogram is
// digit-major, hist[digit * nblocks + block]; scanned, it holds the first slot of every (digit, block).
template <class K, int ITEMS, class I>
__global__ __launch_bounds__(256) void k_radix_hist(const K *__restrict__ keys, I N, int shift, int nblocks, int *__restrict__ hist) {
    __shared__ int lh[256];
    lh[threadIdx.x] = 0;
    __syncthreads();
    const I base = (I)blockIdx.x * (BLK * ITEMS);
    for (int r = 0; r < ITEMS; r++) {
        const I i = base + (I)r * BLK + threadIdx.x;
        if (i < N) atomicAdd(&lh[(int)((keys[i] >> shift) & (K)255)], 1);
    }
    __syncthreads();
    hist[(I)threadIdx.x * nblocks + blockIdx.x] = lh[threadIdx.x];
}
// (key, payload) pairs of block b go to the slots their digit owns, in their order: ballot ranking inside a wave, the waves of a block one
// after the other.  vin == NULL: the position is the payload.
template <class K, int ITEMS, class I>
__global__ __launch_bounds__(256) void k_radix_scatter(const K *__restrict__ kin, const u32 *__restrict__ vin, K *__restrict__ kout,
                                                       u32 *__restrict__ vout, I N, int shift, int nblocks, const int *__restrict__ hist) {
    __shared__ int base[256];
    __shared__ int cnt[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    base[tid] = hist[(I)tid * nblocks + blockIdx.x];
    const I tile = (I)blockIdx.x * (BLK * ITEMS);
    for (int r = 0; r < ITEMS; r++) {
        for (int w = 0; w < 4; w++) cnt[w][tid] = 0;
        __syncthreads();
        const I i = tile + (I)r * BLK + tid;
        const bool valid = i < N;
        K key = 0; u32 val = 0; int dig = 0;
        if (valid) { key = kin[i]; val = vin ? vin[i] : (u32)i; dig = (int)((key >> shift) & (K)255); }
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const u64 bal = __ballot(valid && ((dig >> b) & 1));
            peers &= ((dig >> b) & 1) ? bal : ~bal;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) cnt[wave][dig] = __popcll(peers);
        __syncthreads();
        if (valid) {
            int off = base[dig] + rank;
            for (int w = 0; w < wave; w++) off += cnt[w][dig];
            kout[off] = key; vout[off] = val;
        }
        __syncthreads();
        base[tid] += cnt[0][tid] + cnt[1][tid] + cnt[2][tid] + cnt[3][tid];
        __syncthreads();
    }
}
