// updown.inc -- part of qpdo_dev.hip (one translation unit; included in order): in-place up/downdate of the kept dense LDL' factor, one changed row of A at a time
// ================================================================================================
// K' = K + delta a a'  (a = one row of A, delta = d_new - d_fact) changes the kept factor K = L D L' in place
// (QPDO_DENSE_UPDOWN; the reference: newton.c:21-30 -> cholmod_updown).  Method C1 of Gill, Golub, Murray and
// Saunders (Math. Comp. 28, 1974) with its running quantity written as a prefix sum:
//   p = L^-1 a                                   the chained forward solve that exists (k_ldl_chain<true>: p and q = p / D)
//   t_0 = 1 / delta,  t_{j+1} = t_j + p_j q_j    k_ud_prep, workgroup "scan"
//   D'_j = D_j t_{j+1} / t_j,  beta_j = q_j / t_{j+1}
//   row r of L, s = a_r, for j < r in order:  s -= p_j L_rj,  L'_rj = L_rj + beta_j s        k_ud_apply
// p is known before L is touched, so a 64 x 64 tile (I, J) needs only its entry state a_I - sum_{J' < J} L(I, J') p_J': the tile
// products g(I, J') = L(I, J') p_J' come from the other workgroups of k_ud_prep, and k_ud_apply subtracts them in ascending J'.
// Three launches per changed row, nothing waits on another workgroup inside a launch, every sum has a fixed order: the same bits
// from the same sequence.  A scan that meets a D' that is not a positive finite number latches C_UD_REJECT before anything is
// overwritten; k_ud_apply (of this row and of the rows behind it) then leaves at once, L and D stay a valid factor, and the host
// refactors when it reads the latch with the solve's residual (host_dense.inc dense_solve_updown).
// ================================================================================================
static const int UD_DEFAULT_CAP = 1;       // QPDO_DENSE_UPDOWN=1: one row, the smallest cap, until the route's cost has been measured (docs/LAB_NOTES.md)
static const int UD_CAP_MAX = 64;          // rows one pass may send through the up/downdate (the scratch columns a, p, q)

// the rows whose weight differs from the factored one, in row order: rows[0 .. min(cnt, cap)), cnt[0] = how many differ
__global__ __launch_bounds__(1024) void k_ud_select(int m, const double *__restrict__ dw, const double *__restrict__ dfact, int cap,
                                                    int *__restrict__ rows, int *__restrict__ cnt) {
    __shared__ int sums[1024];
    const int chunk = (m + 1023) / 1024;
    const int beg = min((int)threadIdx.x * chunk, m), end = min(beg + chunk, m);
    int c = 0;
    for (int i = beg; i < end; i++) c += (dw[i] != dfact[i]);
    sums[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) { int run = 0; for (int i = 0; i < 1024; i++) { const int t = sums[i]; sums[i] = run; run += t; } cnt[0] = run; }
    __syncthreads();
    int pos = sums[threadIdx.x];
    for (int i = beg; i < end; i++)
        if (dw[i] != dfact[i]) { if (pos < cap) rows[pos] = i; pos++; }
}
// column b of the scratch: a = row rows[b] of A as a dense vector (zero padded to ld); p and q get the sentinel of the chained solve
__global__ __launch_bounds__(256) void k_ud_load(int ld, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci,
                                                 const double *__restrict__ aval, double *__restrict__ A, double *__restrict__ P, double *__restrict__ Q) {
    double *a = A + (size_t)blockIdx.x * ld;
    unsigned long long *p = reinterpret_cast<unsigned long long *>(P + (size_t)blockIdx.x * ld), *q = reinterpret_cast<unsigned long long *>(Q + (size_t)blockIdx.x * ld);
    for (int i = threadIdx.x; i < ld; i += blockDim.x) { a[i] = 0.0; p[i] = CH_SENT; q[i] = CH_SENT; }
    __syncthreads();
    const int r = rows[blockIdx.x];
    for (int e = arp[r] + threadIdx.x; e < arp[r + 1]; e += blockDim.x) a[aci[e]] = aval[e];
}
// grid (nb, nb + 1), the scan first.  Workgroup (I, J + 1), J < I: g(I, J) = L(I, J) p_J (64 values; each wave sums 16 columns in order, the four partial
// sums are added pairwise) into G[J ld + 64 I ..].  Workgroup (0, 0), the scan (the serial part: dispatched in front of the tile products): D' and beta of every column from p, q = p / D and D;
// the prefix sum is cut into 256 runs of consecutive columns -- the run totals are added in order by one thread, then every thread
// walks its run again -- so its order is fixed.
__global__ __launch_bounds__(256) void k_ud_prep(const double *__restrict__ K, int ld, int nb, const double *__restrict__ Dg, const double *__restrict__ p,
                                                 const double *__restrict__ q, const int *__restrict__ rows, int k, const double *__restrict__ dw,
                                                 const double *__restrict__ dfact, double *__restrict__ G, double *__restrict__ Dn,
                                                 double *__restrict__ beta, Ctrl *ctrl) {
    __shared__ double part[4][DNB];
    __shared__ double runs[256];
    const int tid = threadIdx.x;
    if (blockIdx.y == 0) {
        if (blockIdx.x != 0) return;
        const int r = rows[k];
        const double t0 = 1.0 / (dw[r] - dfact[r]);
        const int chunk = (ld + 255) / 256;
        const int beg = min(tid * chunk, ld), end = min(beg + chunk, ld);
        double sacc = 0.0;
        for (int i = beg; i < end; i++) sacc += p[i] * q[i];
        runs[tid] = sacc;
        __syncthreads();
        if (tid == 0) { double run = t0; for (int i = 0; i < 256; i++) { const double t = runs[i]; runs[i] = run; run += t; } }
        __syncthreads();
        double t = runs[tid];
        bool bad = false;
        for (int i = beg; i < end; i++) {
            const double tn = t + p[i] * q[i];
            const double dn = Dg[i] * (tn / t), b = q[i] / tn;
            if (!(dn > 0.0) || !(dn <= 1.7976931348623157e308) || !(fabs(b) <= 1.7976931348623157e308)) bad = true;
            Dn[i] = dn; beta[i] = b;
            t = tn;
        }
        if (bad) atomicOr(&ctrl->cnt[C_UD_REJECT], 1);
        return;
    }
    const int I = blockIdx.x, J = (int)blockIdx.y - 1;
    if (J >= I) return;
    const int w = tid >> 6, l = tid & 63;
    const double *t = K + (size_t)I * DNB + l + ((size_t)J * DNB + (size_t)w * 16) * ld;
    double v[16];
#pragma unroll
    for (int c = 0; c < 16; c++) v[c] = t[(size_t)c * ld];
    const double *pj = p + (size_t)J * DNB + w * 16;
    double sacc = 0.0;
#pragma unroll
    for (int c = 0; c < 16; c++) sacc += v[c] * pj[c];
    part[w][l] = sacc;
    __syncthreads();
    if (w == 0) G[(size_t)J * ld + (size_t)I * DNB + l] = (part[0][l] + part[1][l]) + (part[2][l] + part[3][l]);
}
// grid (nb, nb), workgroup (I, J), J <= I: the recurrence on tile (I, J) of L.  Thread (w, r) = row r of the tile, columns 16 w .. 16 w + 15:
// its state is the tile's entry state minus the columns of the waves before it (read from the LDS image of the OLD tile, in column
// order -- the same operations as one thread walking the 64 columns).  The new tile goes to L and, for J < I, transposed into the
// upper triangle (the copy the backward solve reads); a diagonal tile (strictly lower part only) also gets the inverse of its
// unit-lower block rebuilt (the 16 x 16 scheme of the factorization: tri16_inv_wave, inv_block_wave), Linv and LinvT from the same
// values, and commits D' of its 64 columns; workgroup (0, 0) sets d_fact of the row.
__global__ __launch_bounds__(256) void k_ud_apply(double *__restrict__ K, int ld, int nb, double *__restrict__ Dg, double *__restrict__ Linv,
                                                  double *__restrict__ LinvT, const double *__restrict__ a, const double *__restrict__ p,
                                                  const double *__restrict__ G, const double *__restrict__ Dn, const double *__restrict__ beta,
                                                  const int *__restrict__ rows, int k, const double *__restrict__ dw, double *__restrict__ dfact,
                                                  const Ctrl *ctrl) {
    constexpr int TS = DG_TS;
    __shared__ double T[DNB * TS];
    __shared__ double Ic[10 * 256];
    __shared__ double ps[DNB], bs[DNB];
    if (ctrl->cnt[C_UD_REJECT]) return;                             // a scan rejected this row or one before it: the factor stays as it is
    const int I = blockIdx.x, J = blockIdx.y;
    if (J > I) return;
    const int tid = threadIdx.x, w = tid >> 6, r = tid & 63;
    const bool diag = I == J;
    const size_t row = (size_t)I * DNB + r;
    double *t = K + row + ((size_t)J * DNB + (size_t)w * 16) * ld;
    double v[16];
#pragma unroll
    for (int c = 0; c < 16; c++) v[c] = (!diag || w * 16 + c < r) ? t[(size_t)c * ld] : 0.0;
    if (tid < DNB) { ps[tid] = p[(size_t)J * DNB + tid]; bs[tid] = beta[(size_t)J * DNB + tid]; }
    double s = a[row];
    for (int j = 0; j < J; j++) s -= G[(size_t)j * ld + row];
#pragma unroll
    for (int c = 0; c < 16; c++) T[r * TS + w * 16 + c] = v[c];
    __syncthreads();
    for (int j = 0; j < w * 16; j++) s -= ps[j] * T[r * TS + j];
    __syncthreads();                                                // every wave has read the old columns before any is overwritten
#pragma unroll
    for (int c = 0; c < 16; c++) {
        const int j = w * 16 + c;
        s -= ps[j] * v[c];
        const double ln = v[c] + bs[j] * s;
        if (!diag || j < r) { t[(size_t)c * ld] = ln; T[r * TS + j] = ln; }
    }
    __syncthreads();
    if (!diag) {
        // transposed copy: K(64 J + j, 64 I + i) = L'(i, j), lanes along j
        double *u = K + (size_t)J * DNB + r + ((size_t)I * DNB + (size_t)w * 16) * ld;
#pragma unroll
        for (int c = 0; c < 16; c++) u[(size_t)c * ld] = T[(w * 16 + c) * TS + r];
        return;
    }
    const int li = r & 15, lk = r >> 4;
    tri16_inv_wave<1, 0>(T, Ic, w, r);
    __syncthreads();
#pragma unroll 1
    for (int dgl = 1; dgl < 4; dgl++) {
        const int bi = dgl + w, bj = w;
        if (bi < 4) inv_block_wave(T, Ic, bi, bj, li, lk);
        __syncthreads();
    }
    double *o1 = Linv + (size_t)I * DNB * DNB, *o2 = LinvT + (size_t)I * DNB * DNB;
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) {
        const int c = w + 4 * e;
        o1[(size_t)c * DNB + r] = diag64_inv(Ic, r, c);
        o2[(size_t)c * DNB + r] = diag64_inv(Ic, c, r);
    }
    if (tid < DNB) Dg[(size_t)I * DNB + tid] = Dn[(size_t)I * DNB + tid];
    if (I == 0 && tid == 0) { const int ar = rows[k]; dfact[ar] = dw[ar]; }
}
