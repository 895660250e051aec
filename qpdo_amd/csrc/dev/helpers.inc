// helpers.inc -- part of qpdo_dev.hip (one translation unit; included in order): device reduction helpers
// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// sum over the block; result valid in every thread.  sm: >= 4 doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double *sm) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sm[w] = v;
    __syncthreads();
    double t = sm[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); i++) t += sm[i];
    return t;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { double t = __shfl_down(v, o, 64); v = t > v ? t : v; }
    return v;
}
// max over block of non-negative values then one atomicMax on the bit pattern (exact).
__device__ __forceinline__ void block_max_to(double v, u64 *dst, double *sm) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sm[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sm[0];
        for (int i = 1; i < (int)(blockDim.x >> 6); i++) t = sm[i] > t ? sm[i] : t;
        if (t > 0.0) atomicMax(dst, (u64)__double_as_longlong(t));
    }
}
// max over the block of non-negative values; result valid in every thread.  sm: >= blockDim.x / 64 doubles that no thread still reads.
__device__ __forceinline__ double block_max(double v, double *sm) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sm[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); i++) t = sm[i] > t ? sm[i] : t;
    return t;
}
// reference c_absval / '>' semantics: a NaN never replaces the running maximum (lin_alg.c:107-140)
__device__ __forceinline__ double absmax_acc(double mx, double a) {
    double s = a < 0 ? -a : a;
    return s > mx ? s : mx;
}
__device__ __forceinline__ double mid3(double a, double lo, double hi) {   // lin_alg.c:163-168
    double t = a < hi ? a : hi;
    return lo > t ? lo : t;
}
// every block re-reduces `cnt` per-block partial sums in a fixed order (deterministic)
__device__ __forceinline__ double reduce_partials(const double *p, int cnt, double *sm) {
    double s = 0.0;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) s += p[i];
    return block_sum(s, sm);
}
// Four sums at once over the first 256 threads of a block of 256 or more (the others pass zeros and get the sums too): one pair of
// barriers instead of four; per value the wave sums, four LDS slots and the order of additions of block_sum in a 256-thread block.
// sm: >= 16 doubles.
__device__ __forceinline__ void block_sum4_256(double &a, double &b, double &c, double &e, double *sm) {
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c); e = wave_sum(e);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0 && w < 4) { sm[w] = a; sm[4 + w] = b; sm[8 + w] = c; sm[12 + w] = e; }
    __syncthreads();
    double ta = sm[0], tb = sm[4], tc = sm[8], te = sm[12];
    for (int i = 1; i < 4; i++) { ta += sm[i]; tb += sm[4 + i]; tc += sm[8 + i]; te += sm[12 + i]; }
    a = ta; b = tb; c = tc; e = te;
}
__device__ __forceinline__ int block_sum_int(int v, int *sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sm[w] = v;
    __syncthreads();
    int t = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) t += sm[i];
    return t;
}

static inline int vgrid(long long len) {
    long long g = (len + BLK - 1) / BLK;
    if (g < 1) g = 1;
    if (g > PGRID) g = PGRID;
    return (int)g;
}

