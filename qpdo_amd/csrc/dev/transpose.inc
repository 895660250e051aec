// transpose.inc -- part of qpdo_dev.hip (one translation unit; included in order): qpdo_setup's matrix conversions ON THE DEVICE.
// ------------------------------------------------------------------------------------------------
// The caller hands over CSC arrays (cholmod_sparse: reference include/types.h:84-85, read by qpdo_setup at src/qpdo.c:100-109).  They
// ARE the CSR arrays of the transpose, so CSR(A') is the upload itself; CSR(A) and the full symmetric CSR(Q) used to be built by OpenMP
// loops on the host (0.7 s of a 1.9 s setup at n = 1e5, m = 2e5, 1 % fill, plus 3 GB more to upload).  Here:
//   * transposition = a STABLE LSD radix sort of the entry positions by their minor index (8-bit digits, ballot ranking inside a wave,
//     per-(digit, block) offsets from a scanned histogram): entries of one output row keep their source order, i.e. ascending major
//     index -- the rows come out column-sorted, exactly the arrays the host's counting pass produced (duplicates keep their order too);
//   * the symmetric expansion merges, per row, the kept part of the transposed triangle with the mirrored stored column (the rule of
//     qpdo_api.c sym_to_full_csr).
// Integer work only; the arrays are bit-for-bit those of the host path (tests: test_device_setup_matches_host_setup).
// ------------------------------------------------------------------------------------------------
static const int RT_ITEMS = 32;                      // keys per thread per block
static const int RT_TILE = BLK * RT_ITEMS;           // 8192 keys per block

__global__ void k_narrow_i64(long long n, const long long *__restrict__ in, int *__restrict__ out) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) out[k] = (int)in[k];
}
__global__ void k_tr_count(long long N, const int *__restrict__ key, int *__restrict__ cnt) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += (long long)gridDim.x * blockDim.x) atomicAdd(&cnt[key[k]], 1);
}
// major index of every entry position (row r of the source owns positions rp[r] .. rp[r+1]): one wave per row
__global__ __launch_bounds__(256) void k_expand_rows(int nrows, const int *__restrict__ rp, u32 *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * BLK + threadIdx.x) >> 6, nwaves = gridDim.x * (BLK / 64);
    for (int r = wave; r < nrows; r += nwaves)
        for (int k = rp[r] + lane; k < rp[r + 1]; k += 64) out[k] = (u32)r;
}
__global__ __launch_bounds__(256) void k_rt_hist(const u32 *__restrict__ keys, long long N, int shift, int nblocks, int *__restrict__ hist) {
    __shared__ int lh[256];
    lh[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * RT_TILE;
    for (int r = 0; r < RT_ITEMS; r++) {
        const long long i = base + (long long)r * BLK + threadIdx.x;
        if (i < N) atomicAdd(&lh[(int)((keys[i] >> shift) & 255u)], 1);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = lh[threadIdx.x];
}
// exclusive scan of a long integer array in three launches (tile sums, scan of the tile sums by one block, rescan with offsets);
// integers: any association gives the same result
static const int SC_TILE = 1024 * 64;
__global__ __launch_bounds__(1024) void k_sc_tile_sums(const int *__restrict__ a, long long total, int *__restrict__ tsum) {
    __shared__ int ws[16];
    const long long beg = (long long)blockIdx.x * SC_TILE;
    int s = 0;
    for (int q = 0; q < 64; q++) { const long long i = beg + (long long)q * 1024 + threadIdx.x; if (i < total) s += a[i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < 16; w++) t += ws[w]; tsum[blockIdx.x] = t; }
}
__global__ __launch_bounds__(1024) void k_sc_tile_scan(int *__restrict__ a, long long total, const int *__restrict__ toff) {
    // tile = 64 rows of 1024 consecutive elements; row q is scanned across the block with wave shuffles, rows one after the other
    __shared__ int wtot[16]; __shared__ int carry;
    const long long beg = (long long)blockIdx.x * SC_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = toff[blockIdx.x];
    __syncthreads();
    for (int q = 0; q < 64; q++) {
        const long long i = beg + (long long)q * 1024 + threadIdx.x;
        const int v = i < total ? a[i] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int run = carry + inc - v;
        for (int w = 0; w < wave; w++) run += wtot[w];
        if (i < total) a[i] = run;
        __syncthreads();
        if (threadIdx.x == 1023) carry = run + v;
        __syncthreads();
    }
}
// one pass of the stable sort: (key, pos) pairs of block b go to the slots their digit owns; pos_in == NULL: the position is the index
__global__ __launch_bounds__(256) void k_rt_scatter(const u32 *__restrict__ kin, const u32 *__restrict__ vin, u32 *__restrict__ kout,
                                                    u32 *__restrict__ vout, long long N, int shift, int nblocks, const int *__restrict__ hist) {
    __shared__ int base[256];
    __shared__ int cnt[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    base[tid] = hist[(size_t)tid * nblocks + blockIdx.x];
    const long long tile = (long long)blockIdx.x * RT_TILE;
    for (int r = 0; r < RT_ITEMS; r++) {
        for (int w = 0; w < 4; w++) cnt[w][tid] = 0;
        __syncthreads();
        const long long i = tile + (long long)r * BLK + tid;
        const bool valid = i < N;
        u32 key = 0, val = 0; int dig = 0;
        if (valid) { key = kin[i]; val = vin ? vin[i] : (u32)i; dig = (int)((key >> shift) & 255u); }
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
__global__ void k_tr_gather(long long N, const u32 *__restrict__ perm, const u32 *__restrict__ major, const double *__restrict__ vsrc,
                            int *__restrict__ ci, double *__restrict__ val) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += (long long)gridDim.x * blockDim.x) {
        const u32 p = perm[k];
        ci[k] = (int)major[p]; if (vsrc) val[k] = vsrc[p];      // (vsrc == nullptr: a pattern-only transposition)
    }
}
__global__ void k_max_row_len(int nrows, const int *__restrict__ rp, int *__restrict__ out) {
    int mx = 0;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) { const int l = rp[r + 1] - rp[r]; mx = l > mx ? l : mx; }
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_down(mx, o, 64); mx = t > mx ? t : mx; }
    if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(out, mx);
}
// ---- full symmetric CSR from one stored triangle -----------------------------------------------------------------------------------
// S = the stored arrays read as CSR (row j = stored column j, entries = stored row indices), R = its transpose (CSR of the stored
// matrix).  st < 0 (lower stored): row i = R row i with columns <= i, then S row i with indices > i (the mirrored column below the
// diagonal); st > 0: S row i with indices < i, then R row i with columns >= i.  Entries on the wrong side are ignored, as CHOLMOD does.
__global__ void k_sym_count(int n, int st, const int *__restrict__ Rrp, const int *__restrict__ Rci, const int *__restrict__ Srp,
                            const int *__restrict__ Sci, int *__restrict__ cnt) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int c = 0;
        for (int k = Rrp[i]; k < Rrp[i + 1]; k++) { const int j = Rci[k]; c += (st < 0) ? (j <= i) : (j >= i); }
        for (int k = Srp[i]; k < Srp[i + 1]; k++) { const int r = Sci[k]; c += (st < 0) ? (r > i) : (r < i); }
        cnt[i] = c;
    }
}
// (V = double: the values; V = u32: index payloads -- qpdo_amd_update_matrices's map from the full storage back to the caller's entries)
template <class V>
__global__ __launch_bounds__(256) void k_sym_fill(int n, int st, const int *__restrict__ Rrp, const int *__restrict__ Rci, const V *__restrict__ Rval,
                                                  const int *__restrict__ Srp, const int *__restrict__ Sci, const V *__restrict__ Sval,
                                                  const int *__restrict__ orp, int *__restrict__ oci, V *__restrict__ oval) {
    // one wave per row: the two kept parts are contiguous runs of their (index-sorted or not) source rows, compacted in order by ballot
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * BLK + threadIdx.x) >> 6, nwaves = gridDim.x * (BLK / 64);
    for (int i = wave; i < n; i += nwaves) {
        int s = orp[i];
        for (int part = 0; part < 2; part++) {
            const bool fromR = (st < 0) ? (part == 0) : (part == 1);
            const int b = fromR ? Rrp[i] : Srp[i], e = fromR ? Rrp[i + 1] : Srp[i + 1];
            for (int k0 = b; k0 < e; k0 += 64) {
                const int k = k0 + lane;
                int idx = 0; V v = V(0); bool keep = false;
                if (k < e) {
                    idx = fromR ? Rci[k] : Sci[k]; v = fromR ? Rval[k] : Sval[k];
                    keep = fromR ? ((st < 0) ? (idx <= i) : (idx >= i)) : ((st < 0) ? (idx > i) : (idx < i));
                }
                const u64 mask = __ballot(keep);
                if (keep) { const int pos = s + __popcll(mask & ((1ull << lane) - 1ull)); oci[pos] = idx; oval[pos] = v; }
                s += __popcll(mask);
            }
        }
    }
}
