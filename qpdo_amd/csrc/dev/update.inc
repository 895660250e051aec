// update.inc -- part of qpdo_dev.hip (one translation unit; included in order): kernels of qpdo_amd_update_matrices (host side:
// host_update.inc).  New values of Q and A in the pattern given at setup land in the workspace's three stored matrices in ONE launch.
// ------------------------------------------------------------------------------------------------
// srcA: the caller's A values in CSC order (the workspace's raw copy, or At.val itself when the workspace keeps none);
// Tval != nullptr: CSR(A') = CSC(A) gets a plain copy of srcA; Aval != nullptr: CSR(A) gathers through mapA (the final payload of setup's
// stable radix transposition: the same permutation k_tr_gather applied).  Q: qsrc != nullptr gathers the caller's stored triangle through
// mapQ into the full storage (and into the raw copy qraw when the workspace keeps one); qsrc == nullptr, qraw != nullptr copies the raw
// full storage.  Two grid-stride ranges in one launch; every store is a plain copy, so the values are those setup wrote, bit for bit.
__global__ __launch_bounds__(256) void k_update_values(long long nA, const double *__restrict__ srcA, double *__restrict__ Tval, const u32 *__restrict__ mapA,
                                                       double *__restrict__ Aval, long long nQ, const double *__restrict__ qsrc, const u32 *__restrict__ mapQ,
                                                       double *__restrict__ qraw, double *__restrict__ Qval) {
    const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (Tval || Aval)
        for (long long k = t0; k < nA; k += stride) {
            if (Tval) Tval[k] = srcA[k];
            if (Aval) Aval[k] = srcA[mapA[k]];
        }
    if (qsrc || qraw)
        for (long long k = t0; k < nQ; k += stride) {
            const double v = qsrc ? qsrc[mapQ[k]] : qraw[k];
            if (qsrc && qraw) qraw[k] = v;
            Qval[k] = v;
        }
}
// flag = 1 where two integer arrays differ (the pattern check: every thread that sees a difference writes the same word)
__global__ void k_cmp_int(long long n, const int *__restrict__ a, const int *__restrict__ b, int *__restrict__ flag) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x)
        if (a[k] != b[k]) *flag = 1;
}
__global__ void k_iota_u32(long long n, u32 *__restrict__ out) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) out[k] = (u32)k;
}
