// transpose.inc -- part of qpdo_dev.hip (one translation unit; included in order): qpdo_setup's matrix conversions ON THE DEVICE.
// ------------------------------------------------------------------------------------------------
// The caller hands over CSC arrays (cholmod_sparse: reference include/types.h:84-85, read by qpdo_setup at src/qpdo.c:100-109).  They
// ARE the CSR arrays of the transpose, so CSR(A') is the upload itself; CSR(A) and the full symmetric CSR(Q) used to be built by OpenMP
// loops on the host (0.7 s of a 1.9 s setup at n = 1e5, m = 2e5, 1 % fill, plus 3 GB more to upload).  Here:
//   * transposition = a STABLE LSD radix sort of the entry positions by their minor index (8-bit digits, ballot ranking inside a wave,
//     per-(digit, block) offsets from a scanned histogram): entries of one output row keep their source order, i.e. ascending major
//     index -- the rows come out column-sorted, exactly the arrays the host's counting pass produced (duplicates keep their order too);
//   * the symmetric expansion merges, per row, the kept part of the transposed triangle with the mirrored stored column (the rule
//     written down in csc_convert.h, which csc_convert.c sym_to_full_csr implements on the host).
// Integer work only; the arrays are bit-for-bit those of the host path (tests: test_device_setup_matches_host_setup).
// ------------------------------------------------------------------------------------------------
static const int RT_ITEMS = 32;                      // keys per thread per block of the sort (scan_sort.inc)
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
