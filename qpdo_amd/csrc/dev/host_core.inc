// host_core.inc -- part of qpdo_dev.hip (one translation unit; included in order): host side: allocation, upload, slab set-up, collectives
// ================================================================================================
// host side of the backend
// ================================================================================================
template <class T>
static int dev_alloc(QpdoDev *d, T **p, size_t count) {
    void *q = nullptr;
    size_t bytes = (count ? count : 1) * sizeof(T);
    HIPCHK(hipMalloc(&q, bytes));
    HIPCHK(hipMemsetAsync(q, 0, bytes, d->stream));
    d->allocs.push_back(q);
    *p = (T *)q;
    return 0;
}
static int pick_tpr(const DevCsr &M) {
    const double avg = M.nrows ? (double)M.nnz / (double)M.nrows : 0.0;
    if (avg > 48) return 64;
    if (avg > 24) return 32;
    if (avg > 12) return 16;
    if (avg > 6) return 8;
    return 4;
}
// Host -> device copy of a large pageable array: chunks are copied by a few host threads into two pinned staging buffers
// and sent with asynchronous copies, so the host memcpy of chunk c+1 overlaps the DMA of chunk c (a plain hipMemcpy from
// pageable memory ran at ~7-10 GB/s here: ~0.9 s of the 1.9 s C4 setup).
static void h2d_staging_release(QpdoDev *d) {
    for (int i = 0; i < 2; i++) {
        if (d->pin_ev[i]) { (void)hipEventSynchronize(d->pin_ev[i]); (void)hipEventDestroy(d->pin_ev[i]); d->pin_ev[i] = nullptr; }
        if (d->pin[i]) { (void)hipHostFree(d->pin[i]); d->pin[i] = nullptr; }
        d->pin_used[i] = false;
    }
}
static int h2d_staged(QpdoDev *d, void *dst, const void *src, size_t bytes) {
    const size_t CH = (size_t)64 << 20;
    if (bytes < 2 * CH || d->pin_failed) { HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->stream)); return 0; }
    // the two staging buffers and their events belong to the workspace (device and stream of THIS workspace; freed by
    // h2d_staging_release at the end of qdev_create_dist or by qdev_destroy)
    for (int i = 0; i < 2; i++) if (!d->pin[i]) {
        if (hipHostMalloc((void **)&d->pin[i], CH, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); d->pin[i] = nullptr; d->pin_failed = true; }
        else if (hipEventCreateWithFlags(&d->pin_ev[i], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); d->pin_ev[i] = nullptr; d->pin_failed = true; }
        if (d->pin_failed) {      // no pinned memory: release whatever half of the pair exists and copy plainly
            h2d_staging_release(d);
            HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->stream)); return 0;
        }
    }
    const int T = 4;
    size_t off = 0; int b = 0;
    while (off < bytes) {
        const size_t len = bytes - off < CH ? bytes - off : CH;
        if (d->pin_used[b]) HIPCHK(hipEventSynchronize(d->pin_ev[b]));     // the DMA that read this buffer last has finished
        std::thread th[T];
        char *pb = d->pin[b];
        const char *sb = (const char *)src + off;
        const size_t part = (len + T - 1) / T;
        for (int t = 0; t < T; t++) {
            const size_t o = (size_t)t * part; if (o >= len) break;
            const size_t l2 = len - o < part ? len - o : part;
            th[t] = std::thread([pb, sb, o, l2]() { memcpy(pb + o, sb + o, l2); });
        }
        for (int t = 0; t < T; t++) if (th[t].joinable()) th[t].join();
        HIPCHK(hipMemcpyAsync((char *)dst + off, d->pin[b], len, hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipEventRecord(d->pin_ev[b], d->stream));
        d->pin_used[b] = true; b ^= 1; off += len;
    }
    return 0;
}
static int upload_csr(QpdoDev *d, DevCsr *M, const QdevCsr *h) {
    M->nrows = h->nrows; M->ncols = h->ncols; M->nnz = h->nnz;
    int rc;
    if ((rc = dev_alloc(d, &M->rp, (size_t)h->nrows + 1))) return rc;
    if ((rc = dev_alloc(d, &M->ci, (size_t)h->nnz))) return rc;
    if ((rc = dev_alloc(d, &M->val, (size_t)h->nnz))) return rc;
    HIPCHK(hipMemcpyAsync(M->rp, h->rp, ((size_t)h->nrows + 1) * sizeof(int), hipMemcpyHostToDevice, d->stream));
    if (h->nnz) {
        if ((rc = h2d_staged(d, M->ci, h->ci, (size_t)h->nnz * sizeof(int)))) return rc;
        if ((rc = h2d_staged(d, M->val, h->val, (size_t)h->nnz * sizeof(double)))) return rc;
    }
    M->tpr = pick_tpr(*M);
    return 0;
}
static int read_ctrl(QpdoDev *d);
// decide whether M streams from HBM (then use the LDS-staged kernel) and build its slab pointers
// arrays of the slab-major image (two padding entries: the 16-byte loads may touch one element past a segment)
// with_p16: the pair-local index words of an image that will be in pair order.  They are 16 bits wide because a pair's 2 W floats share
// the LDS with the row sums: W < SLAB_LDS_BYTES / 8 whatever the pass.
static_assert(2 * (SLAB_LDS_BYTES / 8) <= 65536, "pair-local indices are 16 bits wide");
static int slab_major_alloc(QpdoDev *d, DevCsr *M, size_t nnz_cap, size_t nseg, bool with_f32 = false, bool with_h16 = false, bool with_p16 = false) {
    // the vector loads start at a multiple of their entry count (2, 4; 8 for the half-precision stream, which reads eight values and eight
    // 16-bit indices per load) below the segment's end: up to seven elements past it
    const size_t PAD = 8;
    int rc = dev_alloc(d, &M->vsm, nnz_cap + PAD);
    if (!rc) rc = M->ci16 ? dev_alloc(d, &M->i16sm, nnz_cap + PAD) : dev_alloc(d, &M->cism, nnz_cap + PAD);
    if (!rc && with_f32 && M->ci16) rc = dev_alloc(d, &M->vsm32, nnz_cap + PAD);
    if (!rc && with_h16 && M->vsm32) rc = dev_alloc(d, &M->vsm16, nnz_cap + PAD);
    if (!rc && with_p16 && M->vsm32) rc = dev_alloc(d, &M->p16sm, nnz_cap + PAD);      // (zeroed, its padding too)
    if (!rc) rc = dev_alloc(d, &M->seg, nseg > 0 ? nseg : 1);
    if (!rc) {
        hipError_t e = hipMemsetAsync(M->vsm + nnz_cap, 0, PAD * sizeof(double), d->stream);
        if (e == hipSuccess) e = M->i16sm ? hipMemsetAsync(M->i16sm + nnz_cap, 0, PAD * sizeof(unsigned short), d->stream) : hipMemsetAsync(M->cism + nnz_cap, 0, PAD * sizeof(int), d->stream);
        if (e == hipSuccess && M->vsm32) e = hipMemsetAsync(M->vsm32 + nnz_cap, 0, PAD * sizeof(float), d->stream);
        if (e == hipSuccess && M->vsm16) e = hipMemsetAsync(M->vsm16 + nnz_cap, 0, PAD * sizeof(_Float16), d->stream);
        if (e != hipSuccess) rc = set_err(e, "hipMemsetAsync", __LINE__);
    }
    M->sm_dirty = 1;
    return rc;
}
// QPDO_SLAB_MAX_W=<columns, a multiple of 64>: caps the slab width wherever one is computed (here, and for the per-pass compact matrices in
// create_tail and build_compact), so that small problems reach several slabs (tests).  Unset: the LDS decides alone.
static long long slab_cap_w(long long lds_doubles) {
    const char *mw = getenv("QPDO_SLAB_MAX_W");
    const long long cap = (mw && *mw) ? atoll(mw) : 0;
    return (cap > 0 && cap % 64 == 0 && cap < lds_doubles) ? cap : lds_doubles;
}
static int setup_slabs(QpdoDev *d, DevCsr *M) {
    { const char *ov = getenv("QPDO_SLAB_OVERLAP"); M->slab_ovl = !(ov && *ov && atoi(ov) == 0); }
    { const char *nt = getenv("QPDO_SLAB_NT"); M->slab_nt = (nt && atoi(nt) != 0) ? 1 : 0; }
    const char *force = getenv("QPDO_SPMV");            // "slab" | "plain" | unset (auto)
    const double bytes = 12.0 * (double)M->nnz;
    bool want = bytes >= 192.0 * 1024 * 1024 && M->nrows >= 4096;   // beyond what L2 + Infinity Cache keep resident
    if (force && !strcmp(force, "slab")) want = M->nrows >= 256;
    if (force && !strcmp(force, "plain")) want = false;
    M->use_slab = 0;
    if (!want) return 0;
    const int NWG = 256;                                 // one workgroup per CU
    M->rows_per_wg = (M->nrows + NWG - 1) / NWG;
    M->slab_grid = (M->nrows + M->rows_per_wg - 1) / M->rows_per_wg;
    const long long lds_room = (160 * 1024 - 1024) / 8 - M->rows_per_wg;
    if (lds_room < 1024) return 0;
    const long long lds_doubles = slab_cap_w(lds_room);
    int nslabs = (int)((M->ncols + lds_doubles - 1) / lds_doubles);
    if (nslabs < 1) nslabs = 1;
    int W = (M->ncols + nslabs - 1) / nslabs;
    W = (W + 63) & ~63;
    if (W > lds_doubles) { nslabs++; W = ((M->ncols + nslabs - 1) / nslabs + 63) & ~63; }
    M->nslabs = nslabs; M->W = W;
    int rc = dev_alloc(d, &M->sp, (size_t)M->nrows * (nslabs + 1));
    if (rc) return rc;
    hipLaunchKernelGGL(k_ctrl_set_int, dim3(1), dim3(1), 0, d->stream, d->ctrl, C_VIOL, 0);
    hipLaunchKernelGGL(k_build_slab_ptr, dim3(vgrid(M->nrows)), dim3(BLK), 0, d->stream, M->nrows, M->rp, M->ci, nslabs, W, M->sp, &d->ctrl->cnt[C_VIOL]);
    rc = read_ctrl(d); if (rc) return rc;
    M->use_slab = d->hctrl->cnt[C_VIOL] ? 0 : 1;          // unsorted rows: keep the plain kernel
    const char *i16 = getenv("QPDO_IDX16");
    if (M->use_slab && W < 65536 && !(i16 && !strcmp(i16, "0"))) {
        rc = dev_alloc(d, &M->ci16, (size_t)M->nnz);
        if (rc) return rc;
        hipLaunchKernelGGL(k_fill_ci16, dim3(2048), dim3(BLK), 0, d->stream, M->nnz, M->ci, W, M->ci16);
    }
    if (M->use_slab) { rc = slab_major_alloc(d, M, (size_t)M->nnz, (size_t)M->nrows * nslabs); if (rc) return rc; }
    return 0;
}
// where the builders of M's image write its half-precision values: nowhere while the workspace has no scale (h16_refresh_scale)
static inline _Float16 *h16_dst(const QpdoDev *d, const DevCsr &M) { return d->h16_set ? M.vsm16 : (_Float16 *)nullptr; }
static void slab_major_build(QpdoDev *d, const DevCsr &M) {
    hipLaunchKernelGGL(k_slab_seg, dim3(M.slab_grid), dim3(1024), 0, d->stream, M.nrows, M.nslabs, M.rows_per_wg, (const int *)M.sp, M.seg, M.seg_pairs);
    hipLaunchKernelGGL(k_slab_permute, dim3(2048), dim3(256), 0, d->stream, M.nrows, M.nslabs, M.W, (const int *)M.sp, (const int2 *)M.seg,
                       (const int *)M.ci, (const unsigned short *)M.ci16, (const double *)M.val, M.vsm, M.i16sm, M.cism, M.vsm32,
                       h16_dst(d, M), d->h16_scale, M.p16sm);
    M.sm_dirty = 0;
}
// Read-back of a control block.  A pass of the multi-kernel routes makes 1-3 of these and, at mid-size orders, they are a tenth of its time:
// hipMemcpyAsync into pinned memory + hipStreamSynchronize is ~15.7 us per round trip, a one-wave kernel that writes the block and a
// sequence word into coherent pinned memory while the host spins on that word ~10 us (tools/lab/sync_lab.hip, profiles/r05_sync_lab.txt).
// The spin is bounded: after CTRL_SPIN_US it hands over to hipStreamSynchronize (long kernels -- a PCG batch, a large factorization -- are
// waited for there, not by burning a core; a faulted kernel surfaces there as its HIP error).  QPDO_CTRL_PUBLISH=0: the copy path.
static const size_t CTRL_SEQ_OFF = 256;
static const long long CTRL_SPIN_US = 150;
static int ctrl_wait(QpdoDev *d, u64 *hseq, u64 seq) {
    volatile u64 *vs = hseq;
    struct timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
    for (unsigned spins = 0; *vs != seq; spins++) {
        if ((spins & 63u) == 63u) {
            struct timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) * 1000000LL + (t1.tv_nsec - t0.tv_nsec) / 1000 > CTRL_SPIN_US) {
                HIPCHK(hipStreamSynchronize(d->stream));
                if (*vs != seq) return set_err(hipErrorUnknown, "control block publication did not arrive although the stream has drained", __LINE__);
                break;
            }
        }
        __builtin_ia32_pause();
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return 0;
}
static int read_ctrl_block(QpdoDev *d, const Ctrl *dev, Ctrl *host, u64 *hseq) {
    if (!d->ctrl_publish) {
        HIPCHK(hipMemcpyAsync(host, dev, sizeof(Ctrl), hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        return 0;
    }
    const u64 seq = ++d->pub_seq;
    hipLaunchKernelGGL(k_ctrl_publish, dim3(1), dim3(64), 0, d->stream, dev, host, hseq, seq);
    return ctrl_wait(d, hseq, seq);
}
static int read_ctrl(QpdoDev *d) {
    { int rc = read_ctrl_block(d, d->ctrl, d->hctrl, d->hseq); if (rc) return rc; }
    // every host-visible decision of a pass goes through here: a launch that was refused (bad configuration, missing code
    // object) since the last read-back surfaces now instead of as a silently stale control block
    HIPCHK(hipGetLastError());
    return 0;
}
static inline double nrm_of(const Ctrl *c, int slot) {
    double v; u64 b = c->nrm[slot]; memcpy(&v, &b, 8); return v;
}
#define LAUNCH(kernel, grid, ...) hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLK), 0, d->stream, __VA_ARGS__)
// The scale of the half-precision images: 2^e with max |a_ij| 2^e in [2^14, 2^15), the maximum over A as the workspace holds it (the compact
// rows are a subset of its rows; A' has the same entries).  Called where A's values are set; one read of A and one host read.  A maximum
// of 0, inf or NaN leaves the coarse sweeps off.  No-op for a workspace without half-precision images.
static int h16_refresh_scale(QpdoDev *d) {
    d->h16_set = 0; d->h16_e = 0; d->h16_scale = 0.0;
    if (!d->Arc.vsm16 || !d->Atc.vsm16 || d->Ar.nnz <= 0 || d->Ar.nnz > 0x7fffffffLL) return 0;
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    LAUNCH(k_absmax_mul, 2048, (int)d->Ar.nnz, (const double *)d->Ar.val, (const double *)nullptr, d->ctrl, N_A);
    int rc = read_ctrl(d); if (rc) return rc;
    const double amax = nrm_of(d->hctrl, N_A);
    if (!(amax > 0.0) || !(amax <= 1.7976931348623157e308)) return 0;
    int ex = 0; (void)frexp(amax, &ex);               // amax = f 2^ex, f in [0.5, 1): amax 2^(15 - ex) in [2^14, 2^15)
    d->h16_e = 15 - ex; d->h16_scale = ldexp(1.0, d->h16_e); d->h16_set = 1;
    d->Arc.sm_dirty = d->Atc.sm_dirty = 1;
    return 0;
}
// ---- the integer scan and the sorting pass (dev/scan_sort.inc) ----------------------------------------------------------------------
// exclusive scan of cnt[0 .. n) into out[0 .. n) (cnt == out: in place), the total into *total (or nowhere): tile sums, then every tile's
// own scan behind the sums in front of it.  tsum: scratch of scan_tiles(n) ints (a pass: d->scan_tsum; the set-up: its TempAllocs)
static inline int scan_tiles(int n) { return n > 0 ? (int)(((long long)n + SCN_TILE - 1) / SCN_TILE) : 1; }
static void dev_scan(QpdoDev *d, const int *cnt, int n, int *out, int *total, int *tsum) {
    const int nt = scan_tiles(n);
    if (nt > 1) LAUNCH(k_scn_sums, nt, cnt, n, tsum);
    LAUNCH(k_scn_apply, nt, cnt, n, (const int *)tsum, out, total);
}
// one pass of the stable sort of N (key, payload) pairs by the keys' 8-bit digit at `shift`: histogram of the nblocks = ceil(N / (BLK ITEMS))
// tiles, its scan in place, scatter.  hist: 256 nblocks ints; vin == NULL: the payload is the position
template <class K, int ITEMS, class I>
static void radix_pass(QpdoDev *d, const K *kin, const u32 *vin, K *kout, u32 *vout, I N, int shift, int nblocks, int *hist, int *tsum) {
    LAUNCH((k_radix_hist<K, ITEMS, I>), nblocks, kin, N, shift, nblocks, hist);
    dev_scan(d, hist, 256 * nblocks, hist, (int *)nullptr, tsum);
    LAUNCH((k_radix_scatter<K, ITEMS, I>), nblocks, kin, vin, kout, vout, N, shift, nblocks, (const int *)hist);
}

// ---- collectives ----------------------------------------------------------------------------------------
static int comm_allreduce(QpdoDev *d, double *dev, size_t cnt, int op /*0 sum, 1 max*/) {
    Comm &c = d->comm;
    if (!c.active || cnt == 0) return 0;
    d->st.collectives++;
    if (c.mode == 2) {
        ncclResult_t r = ncclAllReduce(dev, dev, cnt, ncclDouble, op ? ncclMax : ncclSum, c.nccl, d->stream);
        if (r != ncclSuccess) { snprintf(g_err, sizeof(g_err), "ncclAllReduce: %s", ncclGetErrorString(r)); return -1; }
        return 0;
    }
    if (c.mode == 1) {
        if (cnt > c.hcap) { snprintf(g_err, sizeof(g_err), "allreduce staging too small"); return -1; }
        HIPCHK(hipMemcpyAsync(c.hbuf, dev, cnt * 8, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        c.fn(c.ctx, c.hbuf, (long)cnt, op);
        HIPCHK(hipMemcpyAsync(dev, c.hbuf, cnt * 8, hipMemcpyHostToDevice, d->stream));
        return 0;
    }
    snprintf(g_err, sizeof(g_err), "distributed workspace without a communicator");
    return -1;
}
// row epilogue applied after the exchange: the same functors the fused single-GPU products use
template <class Epi>
__global__ __launch_bounds__(256) void k_epi_apply(int nrows, const double *__restrict__ sums, Epi epi) {
    __shared__ double sm[32];
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) epi.row(r, sums[r]);
    epi.finish(sm);
}
// y = A x with epilogue (global row space m); world > 1: local rows, sum all-reduce, then the epilogue
template <class Epi>
static int spmv_A(QpdoDev *d, const double *x, Epi epi, bool partials) {
    if (!d->comm.active) { launch_spmv(d, d->Ar, x, epi, partials); return 0; }
    HIPCHK(hipMemsetAsync(d->dist_tmp, 0, (size_t)d->m * 8, d->stream));
    launch_spmv(d, d->Ar, x, EpiStore{d->dist_tmp + d->m0}, false);
    int rc = comm_allreduce(d, d->dist_tmp, (size_t)d->m, 0); if (rc) return rc;
    hipLaunchKernelGGL((k_epi_apply<Epi>), dim3(vgrid(d->m)), dim3(BLK), 0, d->stream, d->m, (const double *)d->dist_tmp, epi);
    return 0;
}
static inline int pgrid_A(QpdoDev *d) { return !d->comm.active ? spmv_pgrid(d->Ar) : vgrid(d->m); }
// y = A' x with epilogue (x is a global m-vector); world > 1: local columns, sum all-reduce, then the epilogue
template <class Epi>
static int spmv_At(QpdoDev *d, const double *x, Epi epi, bool partials) {
    if (!d->comm.active) { launch_spmv(d, d->At, x, epi, partials); return 0; }
    launch_spmv(d, d->At, x + d->m0, EpiStore{d->dist_tmp}, false);
    int rc = comm_allreduce(d, d->dist_tmp, (size_t)d->n, 0); if (rc) return rc;
    hipLaunchKernelGGL((k_epi_apply<Epi>), dim3(vgrid(d->n)), dim3(BLK), 0, d->stream, d->n, (const double *)d->dist_tmp, epi);
    return 0;
}
// PCG pieces of the distributed operator
__global__ void k_pcg_dist_finish(int n, const int *__restrict__ done, const double *__restrict__ part, const double *__restrict__ p,
                                  double sigma_f, double *__restrict__ Kp, double *__restrict__ p_pKp) {
    __shared__ double sm[32];
    if (*done) return;
    double acc = 0.0;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const double v = part[j] + sigma_f * p[j];
        Kp[j] = v; acc += p[j] * v;
    }
    double t = block_sum(acc, sm);
    if (threadIdx.x == 0) p_pKp[blockIdx.x] = t;
}
struct EpiAddTo {                          // out[r + off] += s   (partial operator rows)
    double *out; int off;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { out[r + off] += s; }
    __device__ void finish(double *) {}
};
__global__ void k_add3(int n, const double *__restrict__ a, const double *__restrict__ b, double c, double *__restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = a[i] + b[i] + c;
}


// ---- matrix conversions on the device (dev/transpose.inc) -------------------------------------------------------------------------
struct TempAllocs {                       // device scratch of the setup conversions: released when the conversions are done
    std::vector<void *> v;
    template <class T> int get(T **p, size_t count) { void *q = nullptr; if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return -1; } v.push_back(q); *p = (T *)q; return 0; }
    void release(hipStream_t st) { if (!v.empty()) (void)hipStreamSynchronize(st); for (void *q : v) (void)hipFree(q); v.clear(); }
};
// dst = transpose of src as CSR, rows sorted by (source) major index: stable LSD radix sort of the entry positions by minor index
// perm_out != nullptr (N entries): also the final payload of the sort, perm_out[k] = the source position of entry k of dst
static int dev_transpose(QpdoDev *d, TempAllocs &tmp, const DevCsr &src, DevCsr *dst, bool temp_dst, u32 *perm_out = nullptr) {
    const long long N = src.nnz; const int T = src.ncols;
    dst->nrows = src.ncols; dst->ncols = src.nrows; dst->nnz = N;
    int rc;
    if (temp_dst) {
        if (tmp.get(&dst->rp, (size_t)T + 1) || tmp.get(&dst->ci, (size_t)N) || tmp.get(&dst->val, (size_t)N)) return set_err(hipErrorOutOfMemory, "setup scratch", __LINE__);
        HIPCHK(hipMemsetAsync(dst->rp, 0, ((size_t)T + 1) * sizeof(int), d->stream));
    } else {
        if ((rc = dev_alloc(d, &dst->rp, (size_t)T + 1))) return rc;          // (zero-filled)
        if ((rc = dev_alloc(d, &dst->ci, (size_t)N))) return rc;
        if ((rc = dev_alloc(d, &dst->val, (size_t)N))) return rc;
    }
    dst->tpr = pick_tpr(*dst);
    if (N == 0 || T == 0) return 0;
    int bits = 1; while (bits < 31 && (1ll << bits) < (long long)T) bits++;
    const int passes = (bits + 7) / 8;
    const int nblocks = (int)((N + RT_TILE - 1) / RT_TILE);
    const int tiles = scan_tiles(T) > scan_tiles(256 * nblocks) ? scan_tiles(T) : scan_tiles(256 * nblocks);
    u32 *kb[2] = {nullptr, nullptr}, *pb[2] = {nullptr, nullptr}, *major = nullptr; int *hist = nullptr, *tsum = nullptr;
    if (tmp.get(&pb[0], (size_t)N) || tmp.get(&pb[1], (size_t)N) || tmp.get(&major, (size_t)N) || tmp.get(&hist, (size_t)256 * nblocks) ||
        tmp.get(&tsum, (size_t)tiles) || (passes > 1 && (tmp.get(&kb[0], (size_t)N) || tmp.get(&kb[1], (size_t)N))))
        return set_err(hipErrorOutOfMemory, "setup scratch (transposition)", __LINE__);
    hipLaunchKernelGGL(k_tr_count, dim3(2048), dim3(BLK), 0, d->stream, N, (const int *)src.ci, dst->rp);
    dev_scan(d, dst->rp, T, dst->rp, dst->rp + T, tsum);            // (the total is N: every entry was counted)
    hipLaunchKernelGGL(k_expand_rows, dim3(2048), dim3(BLK), 0, d->stream, src.nrows, (const int *)src.rp, major);
    const u32 *kin = (const u32 *)src.ci, *vin = nullptr;
    int cur = 0;
    for (int p = 0; p < passes; p++) {
        u32 *kout = passes > 1 ? kb[cur] : pb[cur ^ 1];                // (a single pass: the keys go nowhere useful; reuse the spare payload buffer)
        radix_pass<u32, RT_ITEMS, long long>(d, kin, vin, kout, pb[cur], N, 8 * p, nblocks, hist, tsum);
        kin = kout; vin = pb[cur]; cur ^= 1;
    }
    hipLaunchKernelGGL(k_tr_gather, dim3(2048), dim3(BLK), 0, d->stream, N, vin, (const u32 *)major, (const double *)src.val, dst->ci, dst->val);
    if (perm_out) HIPCHK(hipMemcpyAsync(perm_out, vin, (size_t)N * sizeof(u32), hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipGetLastError());
    return 0;
}
// uploads the caller's CSC arrays of an r x c matrix as the CSR arrays of its c x r transpose (index narrowing on the device)
// (with_values = false: the pattern only -- M->val stays unallocated; the pattern check of qpdo_amd_update_matrices)
static int upload_csc_as_csr_of_transpose(QpdoDev *d, TempAllocs &tmp, DevCsr *M, const QdevCsc *h, bool temp_arrays, bool with_values = true) {
    M->nrows = h->ncols; M->ncols = h->nrows; M->nnz = h->nnz;
    int rc = 0;
    if (temp_arrays) { if (tmp.get(&M->rp, (size_t)M->nrows + 1) || tmp.get(&M->ci, (size_t)M->nnz) || (with_values && tmp.get(&M->val, (size_t)M->nnz))) return set_err(hipErrorOutOfMemory, "setup scratch", __LINE__); }
    else { if ((rc = dev_alloc(d, &M->rp, (size_t)M->nrows + 1)) || (rc = dev_alloc(d, &M->ci, (size_t)M->nnz)) || (rc = dev_alloc(d, &M->val, (size_t)M->nnz))) return rc; }
    if (h->itype == 0) {
        HIPCHK(hipMemcpyAsync(M->rp, h->p, ((size_t)M->nrows + 1) * sizeof(int), hipMemcpyHostToDevice, d->stream));
        if (M->nnz && (rc = h2d_staged(d, M->ci, h->i, (size_t)M->nnz * sizeof(int)))) return rc;
    } else {
        long long *w = nullptr;
        const size_t wn = (size_t)(M->nnz > M->nrows + 1 ? M->nnz : M->nrows + 1);
        if (tmp.get(&w, wn)) return set_err(hipErrorOutOfMemory, "setup scratch", __LINE__);
        HIPCHK(hipMemcpyAsync(w, h->p, ((size_t)M->nrows + 1) * 8, hipMemcpyHostToDevice, d->stream));
        hipLaunchKernelGGL(k_narrow_i64, dim3(vgrid(M->nrows + 1)), dim3(BLK), 0, d->stream, (long long)M->nrows + 1, (const long long *)w, M->rp);
        if (M->nnz) {
            if ((rc = h2d_staged(d, w, h->i, (size_t)M->nnz * 8))) return rc;
            hipLaunchKernelGGL(k_narrow_i64, dim3(2048), dim3(BLK), 0, d->stream, (long long)M->nnz, (const long long *)w, M->ci);
        }
    }
    if (with_values && M->nnz && (rc = h2d_staged(d, M->val, h->x, (size_t)M->nnz * sizeof(double)))) return rc;
    M->tpr = pick_tpr(*M);
    return 0;
}
