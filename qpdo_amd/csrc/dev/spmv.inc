// spmv.inc -- part of qpdo_dev.hip (one translation unit; included in order): SpMV kernels (plain and LDS-staged slab), epilogue functors, launchers, per-pass compaction
// ------------------------------------------------------------------------------------------------
// SpMV: y = M x, CSR, TPR lanes cooperate on a row, shuffle reduction inside the lane group.
// The epilogue functor receives the row sum in lane 0 of the group and may fuse the vector work
// that follows the product in the reference (S1/S2 + V1, N5, L1 of SURVEY section 8).
// ------------------------------------------------------------------------------------------------
template <int TPR>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = TPR / 2; o > 0; o >>= 1) v += __shfl_down(v, o, TPR);
    return v;
}

// The CSR row loop of every plain product (k_spmv, and the products folded into k_spmv_pair, k_ls_small and k_dense_assemble):
// block `bid` of `nblk` blocks of `bs` threads, lane groups of `tpr` lanes, two partial sums, the tail added to s0, the shuffle
// tree, epi.row in lane 0.  tpr is a std::integral_constant (k_spmv<TPR>) or a run-time int (the folded products: one
// instantiation serves every matrix); the operations and their order are the same either way, so every caller gets the same bits.
template <class Tpr, class Epi>
__device__ __forceinline__ void spmv_rows(int bid, int nblk, Tpr tpr, int nrows, const int *__restrict__ rp, const int *__restrict__ ci,
                                          const double *__restrict__ val, const double *__restrict__ x, Epi &epi, int bs = BLK) {
    const int lane = threadIdx.x & (tpr - 1);
    const int group = (bid * bs + threadIdx.x) / tpr;
    const int ngroups = nblk * (bs / tpr);
    for (int row = group; row < nrows; row += ngroups) {
        double s = 0.0;
        if (!epi.skip(row)) {
            const int beg = rp[row], end = rp[row + 1];
            double s0 = 0.0, s1 = 0.0;
            int k = beg + lane;
            for (; k + tpr < end; k += 2 * tpr) {
                const double v0 = val[k], v1 = val[k + tpr];
                const int c0 = ci[k], c1 = ci[k + tpr];
                s0 += v0 * x[c0];
                s1 += v1 * x[c1];
            }
            if (k < end) s0 += val[k] * x[ci[k]];
            s = s0 + s1;
            for (int o = tpr / 2; o > 0; o >>= 1) s += __shfl_down(s, o, tpr);
        }
        if (lane == 0) epi.row(row, s);
    }
}
// Optional hook of an epilogue functor: bool prologue(double *sm), called by every thread at the top of the product kernels (k_spmv,
// k_spmv_slab) with the kernel's 32 doubles of LDS; false (uniform over the launch's running workgroups) ends the workgroup.
template <class Epi>
__device__ __forceinline__ auto epi_prologue(Epi &epi, double *sm, int) -> decltype(epi.prologue(sm)) { return epi.prologue(sm); }
template <class Epi>
__device__ __forceinline__ bool epi_prologue(Epi &, double *, long) { return true; }
// done: the PCG's latch (every thread leaves at once when the solver has converged), or nullptr
template <int TPR, class Epi>
__global__ __launch_bounds__(256) void k_spmv(const int *__restrict__ done, int nrows, const int *__restrict__ rp, const int *__restrict__ ci,
                                              const double *__restrict__ val, const double *__restrict__ x, Epi epi) {
    __shared__ double sm[32];
    if (done && *done) return;
    if (!epi_prologue(epi, sm, 0)) return;
    spmv_rows(blockIdx.x, gridDim.x, std::integral_constant<int, TPR>(), nrows, rp, ci, val, x, epi);
    epi.finish(sm);
}


// ------------------------------------------------------------------------------------------------
// LDS-staged SpMV for matrices that stream from HBM (BASELINE north star: "coalesced CSR row loads
// staged in LDS with wavefront __shfl reductions").  One 1024-thread workgroup per CU owns a block of
// consecutive rows and walks the column slabs; for each slab the x-slice (W doubles, up to ~150 KB)
// is copied once into LDS with coalesced loads, then 16-lane groups stream their rows' sub-ranges
// (contiguous val / col-index runs) and gather x from LDS instead of from L2.  Row sums accumulate
// in LDS across slabs in a fixed order, so results are reproducible.
// ------------------------------------------------------------------------------------------------
static const int SLAB_THREADS = 1024;
static constexpr int SLAB_LDS_BYTES = 160 * 1024 - 512;      // dynamic LDS a launch may ask for: the x slice (pair) and the row sums
#define SLAB_UNR 8               // 16-byte loads in flight per lane
static constexpr int SLAB_TPR = 16;     // lanes per row segment (16 x 16-byte loads measured best at C4; 8 and 32: tools/lab/slab_lab.hip)
// OVL (the default; QPDO_SLAB_OVERLAP=0 keeps the old schedule): the slab boundaries are hidden behind matrix loads already in flight.
// Without it, every CU's HBM queue drains at each boundary -- the last segments, two barriers, the x-slice copy from L2 and one
// HBM miss before the new slab's first data.  With it, each lane group issues the value and index loads of ITS first row of the
// next slab (fixed assignment: group g takes row g; the LDS counter then starts at the number of groups) before it goes into the
// barrier, and the same before the staging of slab 0.  The loads do not depend on x.  They land in the registers of the streaming
// loop, and the trip is computed from them after the copy exactly as the loop would have: the arithmetic of a row does not change.
// The x slice is copied with 16-byte global_load_lds (dst = wave base + 16 * lane), so the copy costs one L2 round trip, not one
// per 16 KB.  (Lab, tools/lab/slab_lab.hip LAB_OVL=1, round 6: the early loads alone do not pay at the compact shapes -- the
// register copy waits for them in order; with the async copy: -4 % at k = 66 000, -3.5 % at 73 000, -1 % on the full matrix.)
// NT (opt-in, QPDO_SLAB_NT=1): the values are read once per launch, so their 16-byte loads are non-temporal -- 8 of the 10 streamed
// bytes per nonzero no longer push the x vector and the seg table, which every workgroup re-reads, out of L2.  The index words, x
// staging, seg, acc and the epilogue's vectors keep the default policy.  (Lab, tools/lab/slab_lab.hip LAB_NT=1, round 7: values
// alone -6 % per launch at the compact shapes, non-temporal index words +10 %, alone or together with the values.  The C4 solve does
// not show the lab's gain -- back-to-back launches re-read nothing of the matrix from L2 either way -- and is 0.5 % slower with it:
// off by default, docs/LAB_NOTES.md R7.)
// VT (the value type of the stream): double reads vsm, 10 bytes per nonzero with 16-bit indices; float reads the fp32 copy vsm32 (16-bit
// indices only), 6 bytes per nonzero: one lane trip is then a 16-byte load of FOUR values plus an 8-byte load of four indices, SLAB_UNR32
// of them in flight -- 256 entries per trip of a lane group, so a C4 segment is still one trip.  Products and sums are in double for
// both; everything else of the schedule (early loads, global_load_lds copy, prologue hook, dynamic rows, fixed-order row sums) is shared.
typedef double slab_d2 __attribute__((ext_vector_type(2)));
typedef float slab_f4 __attribute__((ext_vector_type(4)));
// XT (the type of the staged operand): double as above; float (only with VT = float, and only on an image in pair order, k_slab_seg)
// reads an fp32 copy of x, so the LDS that holds W doubles holds the slices of TWO column slabs and the kernel walks slab PAIRS: a row's
// two segments of a pair are adjacent in the image and are streamed as one segment, [beg, mid) of slab 2S and [mid, end) of slab 2S + 1
// (a last single slab is a pair with an empty second half); an entry at or behind mid gathers xs[W + its slab-local index]: these
// instances read the image's PAIR-LOCAL index words (DevCsr::p16sm, passed as `i16sm`), which carry that W already.  Half the
// row hand-outs, seg loads and shuffle trees, half the slab boundaries and half the staging traffic of the slab-by-slab instance, and
// no other matrix byte.  A float times a float is exact in double, so the product's own rounding is that of the sums alone, as before.
#define SLAB_UNR32 4             // fp32 stream: 16-byte value loads in flight per lane
#define SLAB_UNR32X 4            // fp32 stream with the fp32 operand: a C4 pair segment (330-400 entries) is two trips of 256 (measured on the C4 solve: 2, 6 and 8 in flight are 4-8 % slower, docs/LAB_NOTES.md)
// VT = _Float16 (with XT = float, pair order): the half-precision copy vsm16 of the values, scaled by a power of two (QpdoDev::h16_e) that
// the finished row sums undo -- 4 bytes per nonzero.  One lane trip is a 16-byte load of EIGHT values plus a 16-byte load of eight indices,
// a start aligned to eight entries.  half -> float -> double, products and sums in double: an 11-bit value times a 24-bit operand is exact
// there, so the row sums stay the only rounding.  Four loads in flight per lane and EIGHT lanes per row segment: a trip of 256 entries, so
// a C4 pair segment (330-400 entries) is two trips, with 128 bytes per lane in flight.  Measured on the C4 solve against (loads, lanes) =
// (2, 16), (4, 16), (3, 16), (2, 8), (3, 8): docs/LAB_NOTES.md.  (The macros exist for such builds.)
#ifndef SLAB_UNR16
#define SLAB_UNR16 4
#endif
#ifndef SLAB_TPR16
#define SLAB_TPR16 8
#endif
// SLAB_GB16: loads of a trip whose operands are gathered before their products (SLAB_UNR16: the whole trip; SLAB_UNR16 / 2: half trips).
// SLAB_SKIP16: a load behind the first that no lane of the wave needs is neither gathered nor multiplied.  (Measured on the C4 solve,
// docs/LAB_NOTES.md, "fused exact products".)
#ifndef SLAB_GB16
#define SLAB_GB16 (SLAB_UNR16 / 2)
#endif
#ifndef SLAB_SKIP16
#define SLAB_SKIP16 1
#endif
typedef _Float16 slab_h8 __attribute__((ext_vector_type(8)));
template <class VT, class XT> struct SlabStream;
// EPL: entries per lane and load; NSA: partial sums per lane (entry EPL u + e of a trip goes to sum (EPL u + e) mod NSA); TPR: lanes per row segment
template <> struct SlabStream<double, double> { static constexpr int EPL = 2, UNR = SLAB_UNR, NSA = EPL * UNR, TPR = SLAB_TPR; using Vec = double2; };
template <> struct SlabStream<float, double>  { static constexpr int EPL = 4, UNR = SLAB_UNR32, NSA = EPL * UNR, TPR = SLAB_TPR; using Vec = float4; };
template <> struct SlabStream<float, float>   { static constexpr int EPL = 4, UNR = SLAB_UNR32X, NSA = 8, TPR = SLAB_TPR; using Vec = float4; };     // (one sum per entry spills from 8 loads on)
template <> struct SlabStream<_Float16, float> { static constexpr int EPL = 8, UNR = SLAB_UNR16, NSA = 8, TPR = SLAB_TPR16; using Vec = slab_h8; };
template <class VT, class XT>
static int slab_trip_shape(int *shape) {                // {EPL, UNR, NSA, TPR} for the host (qdev_slab_trip_shape)
    using S = SlabStream<VT, XT>;
    shape[0] = S::EPL; shape[1] = S::UNR; shape[2] = S::NSA; shape[3] = S::TPR;
    return 0;
}
template <class VT, class XT, class Epi, bool I16, bool OVL, bool NT>
__global__ __launch_bounds__(1024) void k_spmv_slab(const int *__restrict__ done, int nrows, int ncols, int nslabs, int W,
                                                    int rows_per_wg, const int2 *__restrict__ seg, const int *__restrict__ cism,
                                                    const unsigned short *__restrict__ i16sm,
                                                    const VT *__restrict__ vsm, const XT *__restrict__ x, Epi epi, double rscale) {
    constexpr int TPR = SlabStream<VT, XT>::TPR;
    // NARROW: a copy of the values narrower than double (float, half); rscale: what undoes the scale of the half-precision copy (H16 only)
    constexpr bool F32 = std::is_same<VT, float>::value, H16 = std::is_same<VT, _Float16>::value, NARROW = F32 || H16, X32 = std::is_same<XT, float>::value;
    static_assert(!NARROW || I16, "the narrow streams have 16-bit indices only");
    static_assert(!X32 || NARROW, "the fp32 operand goes with the narrow streams only");
    static_assert(!H16 || X32, "the half-precision stream is pair-wide only");
    constexpr int EPL = SlabStream<VT, XT>::EPL, UNR = SlabStream<VT, XT>::UNR, NSA = SlabStream<VT, XT>::NSA;
    static_assert((EPL * UNR) % NSA == 0 && NSA % 2 == 0, "the partial sums take the entries of a trip in turn");
    using Vec = typename SlabStream<VT, XT>::Vec;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double sm[32];
    __shared__ int next_row;
    if (done && *done) return;
    XT *xs = reinterpret_cast<XT *>(lds);               // W doubles, or the 2 W floats of a slab pair
    double *acc = lds + W;
    const int nsteps = X32 ? (nslabs + 1) >> 1 : nslabs, CW = X32 ? 2 * W : W;      // slabs, or slab pairs, and their columns
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * rows_per_wg;
    const int R = min(rows_per_wg, nrows - row0);
    for (int r = tid; r < R; r += SLAB_THREADS) acc[r] = 0.0;
    const int lane = tid & (TPR - 1);
    constexpr int NG = SLAB_THREADS / TPR;              // lane groups per workgroup
    constexpr int STEP = EPL * UNR * TPR;               // entries per trip of a lane group
    // 16-byte value loads and the matching index loads from a start aligned to EPL entries (the elements before an unaligned
    // `beg` and those after the end are masked): one instruction covers EPL*TPR consecutive entries and UNR of them are in flight
    // per lane -- a C4 segment of one slab (~170 entries) is a single trip of the slab-by-slab instances, a C4 pair segment (330-400) two
    // trips of 256 of the pair-wide ones.  EPL is 2 (double), 4 (float) or 8 (half: both loads of a lane are 16 bytes, starts aligned to
    // eight entries, hence eight entries of padding behind every image array).  No scalar tail loop: slots past the end re-read the
    // first load and contribute exact zeros.  (Lab, tools/lab/slab_lab.hip, C4 shape: 8-byte loads x4: 5.8 TB/s; 16-byte x4: 6.2; x8: 6.9
    // with the slab-major image, 6.2 without.)
    // index words: EPL 16-bit slab-local indices, or a pair of 32-bit ones; unpacked at the use, so that nothing waits for a
    // load in flight before the row's first trip is computed
    using IdxW = typename std::conditional<H16, uint4, typename std::conditional<F32, uint2, typename std::conditional<I16, unsigned, int2>::type>::type>::type;
    auto load_trip = [&](Vec *v, IdxW *w, int k, int kb, int end) {
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            const int kk = k + u * EPL * TPR;
            const int kc = kk < end ? kk : kb;
            if constexpr (H16) {
                if constexpr (NT) v[u] = __builtin_nontemporal_load(reinterpret_cast<const slab_h8 *>(vsm + kc));
                else v[u] = *reinterpret_cast<const slab_h8 *>(vsm + kc);
                w[u] = *reinterpret_cast<const uint4 *>(i16sm + kc);
            } else if constexpr (F32) {
                if constexpr (NT) {
                    const slab_f4 t = __builtin_nontemporal_load(reinterpret_cast<const slab_f4 *>(vsm + kc));
                    v[u] = make_float4(t.x, t.y, t.z, t.w);
                } else v[u] = *reinterpret_cast<const float4 *>(vsm + kc);
                w[u] = *reinterpret_cast<const uint2 *>(i16sm + kc);
            } else {
                if constexpr (NT) {
                    const slab_d2 t = __builtin_nontemporal_load(reinterpret_cast<const slab_d2 *>(vsm + kc));
                    v[u] = make_double2(t.x, t.y);
                } else v[u] = *reinterpret_cast<const double2 *>(vsm + kc);
                if constexpr (I16) w[u] = *reinterpret_cast<const unsigned *>(i16sm + kc);
                else               w[u] = *reinterpret_cast<const int2 *>(cism + kc);
            }
        }
    };
    // OVL: the first trip of the group's prefetched row (pv, pw: written on every pass of the prefetch, so that they are live
    // only from there to the row's first trip -- the register allocator then gives them the registers of the streaming loop)
    Vec pv[UNR]; IdxW pw[UNR];
    int pr = -1, pbeg = 0, pend = 0;
    // segment [beg, end) of `row` in step s: that of slab s, or the two adjacent ones of pair s (which entries are the second slab's is in
    // the pair-local index words)
    auto seg_of = [&](int row, int s, int &beg, int &end) {
        if constexpr (X32) {
            const int2 a = seg[(size_t)row * nslabs + 2 * s];
            const int lb = 2 * s + 1 < nslabs ? seg[(size_t)row * nslabs + 2 * s + 1].y : 0;
            beg = a.x; end = a.x + a.y + lb;
        } else {
            const int2 a = seg[(size_t)row * nslabs + s];
            beg = a.x; end = a.x + a.y;
        }
    };
    // row r's segment [beg, end) of the staged slab (pair), added to acc[r]; PRE: the loads of the first trip are in pv / pw
    auto row_seg = [&](int r, int beg, int end, auto pre) {
        constexpr bool PRE = decltype(pre)::value;
        const int kb = beg & ~(EPL - 1);
        double sa[NSA];
#pragma unroll
        for (int u = 0; u < NSA; u++) sa[u] = 0.0;
        // A trip in straight-line code, GB loads at a time.  Gathers: the operand of EVERY entry slot is read from LDS, whatever the slot's
        // position -- an index word of a load is an index of the image into xs (slab-local; pair-local, [0, 2 W), in the pair-wide
        // instances, whose index words are DevCsr::p16sm) or its zero padding, so the address is inside xs; only behind the last entry of a
        // per-pass image that an earlier, larger pass wrote may a slot hold an index of that pass's wider slab (pair: below 2 W_old),
        // and an LDS read past the workgroup's allocation returns zero, is a read, and feeds a slot that does not count -- and the reads
        // do not depend on each other: they are issued together and waited for together, not one LDS round trip per entry.
        // Products: the slot at position p of the image counts when beg <= p < end.  Only the first load of a lane's trip can lie before
        // beg (kb > beg - EPL), and there the test is one unsigned compare, p - beg < end - beg; every other load compares the entry's
        // number with end - kk.  A slot that does not count adds a zero whatever was gathered for it, so a NaN or an Inf of a column that
        // the row does not touch, or of LDS that the last slab did not stage, never reaches a sum.  fp32 and fp64 values (which may be
        // Inf): the select is on the product, +0.0 for a masked slot.  Half-precision values (finite by construction, h16_round): the
        // select is on the OPERAND, xm = in ? x : 0, and the slot is one fma(v, xm, s) -- v xm is exact in double (11 x 24 bits, exponents
        // far inside the range), so the fma rounds once where s + v x rounded; a masked slot adds v (+0) = +-0 to a sum that began as
        // +0.0 and, to nearest, never becomes -0.0, so s stays s.  No `&&` or `||` in here: the compiler makes a branch per entry of
        // their short circuit and sinks the gather under it.
        // SKIP (half-precision instance): load u >= 1 of a trip is neither gathered nor multiplied when no lane of the wave has an entry in
        // it (kk >= end for all 64; one uniform branch per load) -- every slot of it would have added +-0, and which sum a slot goes to
        // does not depend on it.
        constexpr int GB = H16 ? SLAB_GB16 : X32 ? UNR : UNR / 2;    // (a double operand is two registers per gather: half a trip keeps every instance within 128)
        constexpr bool SKIP = H16 && SLAB_SKIP16 != 0;
        static_assert(UNR % GB == 0, "whole gather batches");
        const unsigned len = (unsigned)(end - beg);
        auto fma_trip = [&](const Vec *v, const IdxW *w, int k) {
#pragma unroll
            for (int u0 = 0; u0 < UNR; u0 += GB) {
                XT xg[GB][EPL];
                bool live[GB];
#pragma unroll
                for (int g = 0; g < GB; g++) {
                    const int u = u0 + g;
                    live[g] = true;
                    if constexpr (SKIP) { if (u > 0) live[g] = __builtin_amdgcn_ballot_w64(k + u * EPL * TPR < end) != 0; }
                    if (!live[g]) continue;
                    int ax[EPL];
                    if constexpr (H16) {
                        const unsigned wd[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
                        for (int e = 0; e < EPL; e++) ax[e] = (int)((e & 1) ? wd[e >> 1] >> 16 : wd[e >> 1] & 0xffffu);
                    } else if constexpr (F32) {
                        ax[0] = (int)(w[u].x & 0xffffu); ax[1] = (int)(w[u].x >> 16); ax[2] = (int)(w[u].y & 0xffffu); ax[3] = (int)(w[u].y >> 16);
                    } else {
                        if constexpr (I16) { ax[0] = (int)(w[u] & 0xffffu); ax[1] = (int)(w[u] >> 16); }
                        else               { ax[0] = w[u].x; ax[1] = w[u].y; }
                    }
#pragma unroll
                    for (int e = 0; e < EPL; e++) xg[g][e] = xs[ax[e]];
                }
#pragma unroll
                for (int g = 0; g < GB; g++) {
                    if (!live[g]) continue;
                    const int u = u0 + g, kk = k + u * EPL * TPR;
                    double vv[EPL];
                    if constexpr (H16) {
#pragma unroll
                        for (int e = 0; e < EPL; e++) vv[e] = (double)(float)v[u][e];
                    } else if constexpr (F32) {
                        vv[0] = (double)v[u].x; vv[1] = (double)v[u].y; vv[2] = (double)v[u].z; vv[3] = (double)v[u].w;
                    } else {
                        vv[0] = v[u].x; vv[1] = v[u].y;
                    }
                    const unsigned t = (unsigned)(kk - beg);
                    const int hi = end - kk;
#pragma unroll
                    for (int e = 0; e < EPL; e++) {
                        const bool in = u == 0 ? t + (unsigned)e < len : e < hi;
                        if constexpr (H16) {
                            const float xm = in ? xg[g][e] : 0.0f;
                            sa[(EPL * u + e) % NSA] = __builtin_fma(vv[e], (double)xm, sa[(EPL * u + e) % NSA]);
                        } else {
                            const double pe = vv[e] * (double)xg[g][e];
                            sa[(EPL * u + e) % NSA] += in ? pe : 0.0;
                        }
                    }
                }
                // (a build without SKIP: the scheduler otherwise hoists the next batch's gathers and conversions over this one's products, 128 VGPRs
                // and 12-24 bytes of scratch; with SKIP the uniform branches keep the batches apart and this line changes no instruction)
                if constexpr (H16 && !SKIP) __builtin_amdgcn_sched_barrier(0);
            }
        };
        int k = kb + EPL * lane;
        if (PRE && k < end) { fma_trip(pv, pw, k); k += STEP; }
        for (; k < end; k += STEP) {
            Vec v[UNR]; IdxW w[UNR];
            load_trip(v, w, k, kb, end);
            fma_trip(v, w, k);
        }
        double t = 0.0;
#pragma unroll
        for (int u = 0; u < NSA / 2; u++) t += sa[2 * u] + sa[2 * u + 1];
#pragma unroll
        for (int o = TPR / 2; o > 0; o >>= 1) t += __shfl_down(t, o, TPR);
        if (lane == 0) acc[r] += t;
    };
    // OVL: the first row batch of slab s is group g -> row g; its first trip's loads are issued here, before the barrier.  Called
    // with s == nslabs too (no loads then): pv / pw are defined on every path around the slab loop.
    auto prefetch = [&](int s) {
#pragma unroll
        for (int u = 0; u < UNR; u++) { pv[u] = Vec{}; pw[u] = IdxW{}; }
        pr = -1;
        const int g = tid / TPR;
        if (s < nsteps && g < R && !epi.skip(row0 + g)) {
            seg_of(row0 + g, s, pbeg, pend);
            pr = g;
            const int kb = pbeg & ~(EPL - 1);
            if (kb + EPL * lane < pend) load_trip(pv, pw, kb + EPL * lane, kb, pend);
        }
    };
    if (OVL) prefetch(0);
    // (behind the first matrix loads: the hook's few KB from L2 and its barriers run while those are in flight)
    if (!epi_prologue(epi, sm, 0)) return;
    for (int s = 0; s < nsteps; s++) {
        const int c0 = s * CW;
        const int cw = min(CW, ncols - c0);
        __syncthreads();
        {   // stage x[c0 .. c0+cw) : 16-byte loads, then the tail (one double, or up to three floats)
            using V16 = typename std::conditional<X32, float4, double2>::type;
            constexpr int E16 = 16 / (int)sizeof(XT);
            const int vecs = cw / E16;
            const V16 *src = reinterpret_cast<const V16 *>(x + c0);
            V16 *dst = reinterpret_cast<V16 *>(xs);
            if (OVL) {      // global -> LDS without VGPRs: every copy of a lane in flight at once, not one L2 round trip each
                for (int i = tid; i < vecs; i += SLAB_THREADS)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + i),
                                                     (__attribute__((address_space(3))) void *)(dst + (i & ~63)), 16, 0, 0);
            } else {
                for (int i = tid; i < vecs; i += SLAB_THREADS) dst[i] = src[i];
            }
            if (tid < (cw & (E16 - 1))) { const int i = (cw & ~(E16 - 1)) + tid; xs[i] = x[c0 + i]; }
            if (tid == 0) next_row = OVL ? NG : 0;
            if (OVL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the copies have landed in LDS
        }
        __syncthreads();
        if (OVL && pr >= 0) row_seg(pr, pbeg, pend, std::true_type());
        // Rows are handed out dynamically (LDS counter): with only a few row segments per lane group and slab a
        // static split leaves groups idle at the end-of-slab barrier.  One lane per WAVE grabs a batch of 64/TPR
        // rows and broadcasts it wave-wide, so the loop exit is wave-uniform (no divergent break around the
        // shuffles).  Which group takes a row does not change the row's arithmetic: results stay reproducible.
        const int gw = (tid & 63) / TPR;                 // group index inside the wave
        for (;;) {
            int base = 0;
            if ((tid & 63) == 0) base = atomicAdd(&next_row, 64 / TPR);
            base = __shfl(base, 0, 64);
            if (base >= R) break;
            const int r = base + gw;
            if (r >= R) continue;
            const int row = row0 + r;
            if (epi.skip(row)) continue;
            int beg, end;
            seg_of(row, s, beg, end);
            row_seg(r, beg, end, std::false_type());
        }
        if (OVL) prefetch(s + 1);
    }
    __syncthreads();
    for (int r = tid; r < R; r += SLAB_THREADS) epi.row(row0 + r, H16 ? acc[r] * rscale : acc[r]);      // (a power of two: exact)
    epi.finish(sm);
}
// slab pointers by binary search in each (column-sorted) row; with `unsorted` given, also flags unsorted rows (a walk over the whole row)
__global__ void k_build_slab_ptr(int nrows, const int *__restrict__ rp, const int *__restrict__ ci, int nslabs, int W,
                                 int *__restrict__ sp, int *__restrict__ unsorted) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
        const int b = rp[r], e = rp[r + 1];
        if (unsorted) {                              // (skipped for the per-pass copies: compaction keeps the checked order)
            int bad = 0;
            for (int k = b + 1; k < e; k++) bad |= (ci[k] < ci[k - 1]);
            if (bad) atomicOr(unsorted, 1);
        }
        int *o = sp + (size_t)r * (nslabs + 1);
        for (int s = 0; s < nslabs; s++) {
            const int target = s * W;
            int lo = b, hi = e;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (ci[mid] < target) lo = mid + 1; else hi = mid; }
            o[s] = lo;
        }
        o[nslabs] = e;
    }
}

// the same pointers for the per-pass copy of the listed rows, searched in the SOURCE rows (the copy has the same columns in the same order):
// sp[j] = rp2[j] + the offset inside row rowlist[j]; the copy itself has not been written yet
__global__ void k_build_slab_ptr_rows(int k, const int *__restrict__ rowlist, const int *__restrict__ rp, const int *__restrict__ ci,
                                      const int *__restrict__ rp2, int nslabs, int W, int *__restrict__ sp) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < k; j += gridDim.x * blockDim.x) {
        const int r = rowlist[j];
        const int b = rp[r], e = rp[r + 1], d0 = rp2[j] - b;
        int *o = sp + (size_t)j * (nslabs + 1);
        for (int s = 0; s < nslabs; s++) {
            const int target = s * W;
            int lo = b, hi = e;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (ci[mid] < target) lo = mid + 1; else hi = mid; }
            o[s] = lo + d0;
        }
        o[nslabs] = e + d0;
    }
}

// slab-major order of the segments of one workgroup's rows: t = s*R + r; exclusive scan of the lengths.  pairs (DevCsr::seg_pairs: the
// compact matrices whose fp32 copy is streamed with fp32 operands): pair-major, (pair S = s / 2, row r, parity s & 1), so that the two segments of a row in a slab pair are
// adjacent -- seg[row][2S+1].x == seg[row][2S].x + seg[row][2S].y -- and the pair-wide product (k_spmv_slab, XT = float) streams them
// as one; an odd last slab follows in (r) order.  The slab-by-slab products read seg[row][s] and take either order.
__global__ __launch_bounds__(1024) void k_slab_seg(int nrows, int nslabs, int rows_per_wg, const int *__restrict__ sp, int2 *__restrict__ seg, int pairs) {
    __shared__ int sums[1024];
    const int row0 = blockIdx.x * rows_per_wg;
    const int R = min(rows_per_wg, nrows - row0);
    if (R <= 0) return;
    const int T = R * nslabs, chunk = (T + 1023) / 1024;
    const int t0 = min((int)threadIdx.x * chunk, T), t1 = min(t0 + chunk, T);
    const int TP = 2 * R * (nslabs >> 1);               // pairs: the segments of the whole pairs come first
    auto at = [&](int t, int &sl, int &r) {             // position t of the order -> (slab, row)
        if (!pairs) { sl = t / R; r = t - sl * R; }
        else if (t < TP) { const int S = t / (2 * R), u = t - 2 * R * S; r = u >> 1; sl = 2 * S + (u & 1); }
        else { r = t - TP; sl = nslabs - 1; }
    };
    int c = 0;
    for (int t = t0; t < t1; t++) { int sl, r; at(t, sl, r); const int *q = sp + (size_t)(row0 + r) * (nslabs + 1) + sl; c += q[1] - q[0]; }
    sums[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) { int run = 0; for (int i = 0; i < 1024; i++) { const int v = sums[i]; sums[i] = run; run += v; } }
    __syncthreads();
    int pos = sp[(size_t)row0 * (nslabs + 1)] + sums[threadIdx.x];
    for (int t = t0; t < t1; t++) {
        int sl, r; at(t, sl, r); const int *q = sp + (size_t)(row0 + r) * (nslabs + 1) + sl;
        const int len = q[1] - q[0];
        seg[(size_t)(row0 + r) * nslabs + sl] = make_int2(pos, len);
        pos += len;
    }
}
// One entry of the half-precision image (DevCsr::vsm16): v scaled by the workspace's power of two h16s = 2^e (exact), rounded to float and
// then to half, each step to nearest even; what lands in the subnormal range of half stays a subnormal.
// INVARIANT: every value of the half-precision image is finite.  h16_refresh_scale keeps max |a| 2^e in [2^14, 2^15), below half's largest
// finite 65504, and sets no scale (no image, no coarse sweeps) for an A whose largest magnitude is not finite; the allocation is zeroed,
// its padding included.  k_spmv_slab's half-precision instance relies on it: it masks the operand of a slot that does not count, not the
// product, and v (+0) is a zero only for a finite v.
__device__ __forceinline__ _Float16 h16_round(double v, double h16s) { return (_Float16)(float)(v * h16s); }
// One entry of the pair-local index image (DevCsr::p16sm): the slab-local index c16 of an entry of slab sl, plus W in the odd slab of a
// pair -- where the pair-wide product finds its operand among the 2 W floats of the staged pair.  (A last single slab is even.)
__device__ __forceinline__ unsigned short pair_local(unsigned short c16, int sl, int W) { return (unsigned short)(c16 + ((sl & 1) ? W : 0)); }
// copy values and slab-local indices of every (row, slab) segment to its slab-major place; 16 lanes per row
__global__ __launch_bounds__(256) void k_slab_permute(int nrows, int nslabs, int W, const int *__restrict__ sp, const int2 *__restrict__ seg,
                                                      const int *__restrict__ ci, const unsigned short *__restrict__ ci16,
                                                      const double *__restrict__ val, double *__restrict__ vsm,
                                                      unsigned short *__restrict__ i16sm, int *__restrict__ cism, float *__restrict__ vsm32,
                                                      _Float16 *__restrict__ vsm16, double h16s, unsigned short *__restrict__ p16sm) {
    const int lane = threadIdx.x & 15;
    const int ngroups = gridDim.x * (blockDim.x >> 4);
    for (int row = blockIdx.x * (blockDim.x >> 4) + (threadIdx.x >> 4); row < nrows; row += ngroups)
        for (int sl = 0; sl < nslabs; sl++) {
            const int src = sp[(size_t)row * (nslabs + 1) + sl];
            const int2 sg = seg[(size_t)row * nslabs + sl];
            for (int e = lane; e < sg.y; e += 16) {
                const double v = val[src + e];
                vsm[sg.x + e] = v;
                if (vsm32) vsm32[sg.x + e] = (float)v;
                if (vsm16) vsm16[sg.x + e] = h16_round(v, h16s);
                if (i16sm) i16sm[sg.x + e] = ci16[src + e]; else cism[sg.x + e] = ci[src + e] - sl * W;
                if (p16sm) p16sm[sg.x + e] = pair_local(ci16[src + e], sl, W);
            }
        }
}

struct EpiStore {                          // y = M x
    double *y;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { y[r] = s; }
    __device__ void finish(double *) {}
};
struct EpiRhs {                            // newton.c:42-45: Atdy = A' t ; rhs = -res_dual_in - Atdy
    const double *rdi; double *atdy, *rhs;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { atdy[r] = s; rhs[r] = -rdi[r] - s; }
    __device__ void finish(double *) {}
};
struct EpiRhsX {                           // EpiRhs inside the assembly launch (k_dense_assemble): also the padded right-hand side of the one-launch factorization
    const double *rdi; double *atdy, *rhs, *rx;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { atdy[r] = s; const double v = -rdi[r] - s; rhs[r] = v; rx[r] = v; }
};
struct EpiQdx {                            // newton.c:52-55 + the two n-dots of linesearch.c:19-25
    const double *dx, *df; double sigma; int prox; double *Qdx, *p_dxQdx, *p_dxdf;
    double a1 = 0.0, a2 = 0.0;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) {
        double v = prox ? s + sigma * dx[r] : s;
        Qdx[r] = v; a1 += dx[r] * v; a2 += dx[r] * df[r];
    }
    __device__ void finish(double *sm) {
        double t1 = block_sum(a1, sm), t2 = block_sum(a2, sm + 16);
        if (threadIdx.x == 0) { p_dxQdx[blockIdx.x] = t1; p_dxdf[blockIdx.x] = t2; }
    }
};
struct EpiQpure {                          // qpdo.c:385: Qdx = Q dx (no sigma), warm start Qx
    const double *xv; double sigma; int prox; double *out;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { out[r] = prox ? s + sigma * xv[r] : s; }
    __device__ void finish(double *) {}
};
// A*dx with the m-side of newton.c:57-63 and linesearch.c:13-40,82-120 fused behind it
struct EpiAdxLs {
    int m;
    const double *mu, *isq, *w, *l, *u, *y; const int *active; int *active_old;
    double *Adx, *dy, *delta, *alpha; u64 *key; u32 *idx;
    double *p_eta, *p_beta, *p_a0, *p_b0; Ctrl *ctrl;
    double e = 0.0, b = 0.0, a0 = 0.0, b0 = 0.0; int nL = 0;
    __device__ bool skip(int) const { return false; }
    __device__ void cand(int i, double dl, double al) {
        delta[i] = dl; alpha[i] = al;
        const double t = al / dl;
        const bool L = t > 0, P = dl > 0;
        key[i] = L ? (u64)__double_as_longlong(t) : KEY_SENTINEL;
        idx[i] = (u32)i;
        if (L) nL++;
        if (L != P) { a0 += dl * dl; b0 += dl * al; }
    }
    __device__ void row(int r, double s) {
        Adx[r] = s;
        const int act = active[r];
        double dyr = dy[r];
        if (act) dyr += s / mu[r];
        dy[r] = dyr;
        active_old[r] = act;                       // newton.c:69
        double sv = dyr * mu[r]; sv = sv * 0.5;    // linesearch.c:14-15
        e += dyr * sv; b += y[r] * sv;
        double c0 = s - sv; c0 = c0 * isq[r];      // linesearch.c:27-28
        const double dlo = c0 * -1.0;
        const double alo = (w[r] - l[r]) * isq[r];
        const double ahi = (u[r] - w[r]) * isq[r];
        cand(r, dlo, alo);
        cand(r + m, c0, ahi);
    }
    __device__ void finish(double *sm) {
        double t1 = block_sum(e, sm), t2 = block_sum(b, sm + 16);
        double t3 = block_sum(a0, sm), t4 = block_sum(b0, sm + 16);
        int tn = block_sum_int(nL, (int *)sm);
        if (threadIdx.x == 0) {
            p_eta[blockIdx.x] = t1; p_beta[blockIdx.x] = t2; p_a0[blockIdx.x] = t3; p_b0[blockIdx.x] = t4;
            if (tn) atomicAdd(&ctrl->cnt[C_NL], tn);
        }
    }
};
struct EpiPcgA {                           // t = d_c .* (A_c p) in the compact row space of the pass
    const double *d; double *t; const int *done;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { t[r] = d[r] * s; }
    __device__ void finish(double *) {}
};
struct EpiPcgQ {                           // Kp = Q p + sigma_f p
    const double *p; double sigma_f; double *Kp;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { Kp[r] = s + sigma_f * p[r]; }
    __device__ void finish(double *) {}
};
struct EpiPcgQdot {                        // no weighted rows: Kp = Q p + sigma_f p and the p.Kp partials in one go
    const double *p; double sigma_f; double *Kp, *p_pKp; double acc = 0.0;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { const double v = s + sigma_f * p[r]; Kp[r] = v; acc += p[r] * v; }
    __device__ void finish(double *sm) {
        double t = block_sum(acc, sm);
        if (threadIdx.x == 0) p_pKp[blockIdx.x] = t;
    }
};
struct EpiPcgAt {                          // Kp += A' t ; partial p.Kp
    const double *p; double *Kp, *p_pKp; double acc = 0.0;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { double v = Kp[r] + s; Kp[r] = v; acc += p[r] * v; }
    __device__ void finish(double *sm) {
        double t = block_sum(acc, sm);
        if (threadIdx.x == 0) p_pKp[blockIdx.x] = t;
    }
};
struct EpiDivDot {                         // t = (M x) ./ w ; partial sum of (M x) .* t   (product 1 of the single-reduction inner CG)
    const double *w; double *out, *p_f; double acc = 0.0;
    float *out32 = nullptr;                // the fp32 copy of t for the pair-wide fp32 product that follows (three-launch schedule), or null
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { const double t = s / w[r]; out[r] = t; if (out32) out32[r] = (float)t; acc += s * t; }
    __device__ void finish(double *sm) {
        double t = block_sum(acc, sm);
        if (threadIdx.x == 0) p_f[blockIdx.x] = t;
    }
};
struct EpiSchurW {                         // w = u ./ d + A_c t   (product 2: S' u without the dot)
    const double *dc, *u; double *w;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int r, double s) { w[r] = u[r] / dc[r] + s; }
    __device__ void finish(double *) {}
};
struct EpiResid {                          // r = rhs - (Kp + A' t), ||r||inf -> ctrl->nrm[slot] (inf if any NaN)
    const double *rhs, *Kp; double *r; Ctrl *ctrl; int slot; double mx = 0.0;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int j, double s) {
        const double v = rhs[j] - (Kp[j] + s);
        r[j] = v;
        const double a = fabs(v);
        mx = (v != v) ? __longlong_as_double(0x7FF0000000000000LL) : (a > mx ? a : mx);
    }
    __device__ void finish(double *sm) { block_max_to(mx, &ctrl->nrm[slot], sm); }
};

static inline int spmv_grid(const DevCsr &M, bool partials) {
    if (M.use_slab) return M.slab_grid;
    long long groups_per_block = BLK / M.tpr;
    long long g = (M.nrows + groups_per_block - 1) / groups_per_block;
    long long cap = partials ? PGRID : 4096;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}
// number of blocks a partial-emitting spmv launch uses (consumers need it)
static inline int spmv_pgrid(const DevCsr &M) { return spmv_grid(M, true); }
// grid of the row-loop kernels (TPR lanes per row, no partial sums: the diagonals and the per-pass counts) over a matrix laid out like M
static inline int rowloop_grid(const DevCsr &M) { return M.use_slab ? 2048 : spmv_grid(M, false); }
// KERNEL<M.tpr> on GRID blocks of BLK threads with LDS bytes of dynamic LDS (further template arguments, such as k_spmv's Epi, are
// deduced from the arguments)
#define DISPATCH_TPR_LDS(M, KERNEL, GRID, LDS, ...)                                                             \
    switch ((M).tpr) {                                                                                          \
        case 4:  hipLaunchKernelGGL((KERNEL<4>),  dim3(GRID), dim3(BLK), (LDS), d->stream, __VA_ARGS__); break; \
        case 8:  hipLaunchKernelGGL((KERNEL<8>),  dim3(GRID), dim3(BLK), (LDS), d->stream, __VA_ARGS__); break; \
        case 16: hipLaunchKernelGGL((KERNEL<16>), dim3(GRID), dim3(BLK), (LDS), d->stream, __VA_ARGS__); break; \
        case 32: hipLaunchKernelGGL((KERNEL<32>), dim3(GRID), dim3(BLK), (LDS), d->stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((KERNEL<64>), dim3(GRID), dim3(BLK), (LDS), d->stream, __VA_ARGS__); break; \
    }
#define DISPATCH_TPR(M, KERNEL, GRID, ...) DISPATCH_TPR_LDS(M, KERNEL, GRID, 0, __VA_ARGS__)
// (re)build the slab-major image of M from its row-major arrays and slab pointers
static void slab_major_build(QpdoDev *d, const DevCsr &M);
// One launch of the slab kernel K with what every such launch needs: the kernel's LDS limit (set once per kernel and host thread),
// the slab-major image rebuilt when the row-major arrays have changed, LDS for the x slice and the row sums, the statistics.
template <auto K, class... Args>
static void launch_slab(QpdoDev *d, const DevCsr &M, Args... args) {
    static thread_local bool attr_set = false;   // per kernel
    if (!attr_set) { (void)hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, SLAB_LDS_BYTES); attr_set = true; }
    if (M.sm_dirty) slab_major_build(d, M);
    const size_t lds = ((size_t)M.W + (size_t)M.rows_per_wg) * sizeof(double);
    hipLaunchKernelGGL(K, dim3(M.slab_grid), dim3(SLAB_THREADS), lds, d->stream, args...);
    d->st.spmv_calls++;
    d->st.spmv_bytes += (int64_t)M.alg_bytes();
}
// f32: the product streams the fp32 copy of the values (M.vsm32 and M.i16sm must exist: the callers check, schur_f32_ready)
template <class Epi>
static void launch_spmv_slab(QpdoDev *d, const DevCsr &M, const double *x, Epi epi, const int *done, bool f32 = false) {
#define SLAB_GO(VT, VSM, I16, OVL, NT) launch_slab<k_spmv_slab<VT, double, Epi, I16, OVL, NT>>(d, M, done, M.nrows, M.ncols, M.nslabs, M.W, M.rows_per_wg, M.seg, M.cism, M.i16sm, VSM, x, epi, 1.0)
#define SLAB_GO_NT(VT, VSM, I16, OVL) do { if (M.slab_nt) SLAB_GO(VT, VSM, I16, OVL, true); else SLAB_GO(VT, VSM, I16, OVL, false); } while (0)
    if (f32) {
        if (M.slab_ovl) SLAB_GO_NT(float, (const float *)M.vsm32, true, true); else SLAB_GO_NT(float, (const float *)M.vsm32, true, false);
        d->st.spmv_bytes -= (int64_t)(4.0 * (double)M.nnz);        // (launch_slab counted the fp64 stream)
        return;
    }
    if (M.slab_ovl) { if (M.i16sm) SLAB_GO_NT(double, (const double *)M.vsm, true, true); else SLAB_GO_NT(double, (const double *)M.vsm, false, true); }
    else            { if (M.i16sm) SLAB_GO_NT(double, (const double *)M.vsm, true, false); else SLAB_GO_NT(double, (const double *)M.vsm, false, false); }
#undef SLAB_GO_NT
#undef SLAB_GO
}
// The pair-wide products: a narrow copy `vals` of the values -- fp32 (vsm32), or half precision (vsm16, whose scale rscale = 2^-e undoes)
// -- and the fp32 copy x32 of the operand.  M takes the slab kernel, carries that copy and i16sm (schur_f32_ready, schur_h16_ready) and
// its image is in pair order (DevCsr::seg_pairs, k_slab_seg), which comes with the pair-local index words p16sm that these instances stream.
template <class VT, class Epi>
static void launch_spmv_x32(QpdoDev *d, const DevCsr &M, const VT *vals, double rscale, const float *x32, Epi epi, const int *done) {
#define SLAB_GO(OVL, NT) launch_slab<k_spmv_slab<VT, float, Epi, true, OVL, NT>>(d, M, done, M.nrows, M.ncols, M.nslabs, M.W, M.rows_per_wg, M.seg, M.cism, M.p16sm, vals, x32, epi, rscale)
    if (M.slab_ovl) { if (M.slab_nt) SLAB_GO(true, true); else SLAB_GO(true, false); }
    else            { if (M.slab_nt) SLAB_GO(false, true); else SLAB_GO(false, false); }
#undef SLAB_GO
    d->st.spmv_bytes -= (int64_t)((12.0 - 4.0 - (double)sizeof(VT)) * (double)M.nnz);      // (launch_slab counted the fp64 stream)
}
// y = M x with the kernel M was set up for; done: the PCG's latch (the product is skipped once it is set), or nullptr
template <class Epi>
static void launch_spmv(QpdoDev *d, const DevCsr &M, const double *x, Epi epi, bool partials, const int *done = nullptr, bool f32 = false) {
    if (M.use_slab) { launch_spmv_slab(d, M, x, epi, done, f32); return; }
    const int g = spmv_grid(M, partials);
    DISPATCH_TPR(M, k_spmv, g, done, M.nrows, M.rp, M.ci, M.val, x, epi);
    d->st.spmv_calls++;
    d->st.spmv_bytes += (int64_t)M.alg_bytes();
}
// ---- the multi-vector product of the group path (dev/adjoint.inc adj_sweeps_group; qpdo_amd_spmv_group) -----------------------------------
// y_g = M x_g for the vectors g of `live` (a kernel argument: every branch on it is uniform over the launch), at most G of them.  The row
// loop is spmv_rows' with ONE read of rp / ci / val per entry and a gather per live vector; every vector keeps its own s0, s1, tail,
// s0 + s1 and shuffle tree, so its bits are k_spmv's with that vector alone.  Operands and results are right-hand-side major: vector g's
// result at y + g ys; its operand at x + g xs, or, compact, at x + (the number of live vectors below g) xs -- where the group's solves
// left their columns.  A vector outside the mask is neither read nor written.  Plain store (the EpiStore of k_spmv).
// Registers: G x 2 partial sums of doubles are 32 VGPRs at G = 8, the gathers in flight and the addresses beside them: the compiler's
// count is 70 VGPRs (72 at TPR = 64), no scratch, 7 waves per SIMD at every TPR -- the vector bases are uniform and stay in SGPRs.
static const int SPMV_GROUP_MAX = 8;
template <int TPR, int G>
__global__ __launch_bounds__(256) void k_spmv_group(int nrows, const int *__restrict__ rp, const int *__restrict__ ci, const double *__restrict__ val,
                                                    const double *__restrict__ x, long long xs, int compact, double *__restrict__ y, long long ys, unsigned live) {
    const int lane = threadIdx.x & (TPR - 1);
    const int group = (blockIdx.x * BLK + threadIdx.x) / TPR;
    const int ngroups = gridDim.x * (BLK / TPR);
    const double *xg[G];
    {
        int slot = 0;
#pragma unroll
        for (int g = 0; g < G; g++) { xg[g] = x + (long long)(compact ? slot : g) * xs; slot += (live >> g) & 1u; }
    }
    for (int row = group; row < nrows; row += ngroups) {
        const int beg = rp[row], end = rp[row + 1];
        double s0[G], s1[G];
#pragma unroll
        for (int g = 0; g < G; g++) { s0[g] = 0.0; s1[g] = 0.0; }
        int k = beg + lane;
        for (; k + TPR < end; k += 2 * TPR) {
            const double v0 = val[k], v1 = val[k + TPR];
            const int c0 = ci[k], c1 = ci[k + TPR];
#pragma unroll
            for (int g = 0; g < G; g++)
                if ((live >> g) & 1u) {
                    s0[g] += v0 * xg[g][c0];
                    s1[g] += v1 * xg[g][c1];
                }
        }
        if (k < end) {
            const double v0 = val[k]; const int c0 = ci[k];
#pragma unroll
            for (int g = 0; g < G; g++) if ((live >> g) & 1u) s0[g] += v0 * xg[g][c0];
        }
#pragma unroll
        for (int g = 0; g < G; g++)
            if ((live >> g) & 1u) {
                double s = s0[g] + s1[g];
                for (int o = TPR / 2; o > 0; o >>= 1) s += __shfl_down(s, o, TPR);
                if (lane == 0) y[(long long)g * ys + row] = s;
            }
    }
}
// M takes the plain kernel (the callers check: a slab multi-vector product does not exist); the grid is launch_spmv's
static void launch_spmv_group(QpdoDev *d, const DevCsr &M, const double *x, long long xs, bool compact, double *y, long long ys, unsigned live) {
    const int g = spmv_grid(M, false);
#define SPMV_GROUP_GO(T) hipLaunchKernelGGL((k_spmv_group<T, SPMV_GROUP_MAX>), dim3(g), dim3(BLK), 0, d->stream, M.nrows, (const int *)M.rp, (const int *)M.ci, (const double *)M.val, x, xs, compact ? 1 : 0, y, ys, live)
    switch (M.tpr) {
        case 4:  SPMV_GROUP_GO(4); break;
        case 8:  SPMV_GROUP_GO(8); break;
        case 16: SPMV_GROUP_GO(16); break;
        case 32: SPMV_GROUP_GO(32); break;
        default: SPMV_GROUP_GO(64); break;
    }
#undef SPMV_GROUP_GO
    d->st.spmv_calls++;
    d->st.spmv_bytes += (int64_t)(M.alg_bytes() + (double)(__builtin_popcount(live) - 1) * 8.0 * (M.nrows + M.ncols));
}
// The width of the matrix stream of one product of the Schur mode's inner solve: the fp64 values, their fp32 copy, their half-precision copy
enum StreamWidth { STREAM_F64 = 0, STREAM_F32, STREAM_H16 };
// One product of the Schur mode's inner CG.  STREAM_F32: pair-wide with the fp32 copy x32 of x where there is one, otherwise slab by slab
// with x.  STREAM_H16: pair-wide only (x32 and M.vsm16 must exist: schur_h16_ready); the row sums are multiplied by 2^-e of the workspace.
template <class Epi>
static void launch_spmv_inner(QpdoDev *d, const DevCsr &M, const double *x, const float *x32, Epi epi, bool partials, const int *done, StreamWidth width) {
    if (width == STREAM_H16) launch_spmv_x32(d, M, (const _Float16 *)M.vsm16, ldexp(1.0, -d->h16_e), x32, epi, done);
    else if (width == STREAM_F32 && x32) launch_spmv_x32(d, M, (const float *)M.vsm32, 1.0, x32, epi, done);
    else launch_spmv(d, M, x, epi, partials, done, width == STREAM_F32);
}

// Two independent products in ONE launch (small problems: a launch is ~4-5 us whatever it computes, and Q dx and A dx of a Newton step
// depend on nothing of each other): blocks [0, gA) take the first with its own grid, the rest the second.  Lanes per row are run-time
// values here (spmv_rows with an int width), so one instantiation serves every pair of matrices.  The second epilogue indexes its block
// partials by blockIdx.x: the host passes those pointers shifted back by gA.
template <class EpiA, class EpiB>
__global__ __launch_bounds__(256) void k_spmv_pair(int gA, int tprA, int nrowsA, const int *__restrict__ rpA, const int *__restrict__ ciA,
                                                   const double *__restrict__ valA, const double *__restrict__ xA, EpiA epiA, int tprB, int nrowsB,
                                                   const int *__restrict__ rpB, const int *__restrict__ ciB, const double *__restrict__ valB,
                                                   const double *__restrict__ xB, EpiB epiB, const int *__restrict__ skip = nullptr) {
    __shared__ double sm[32];
    if (skip && *skip) return;                                      // launch-ahead (vector.inc SpecArgs): this pass is not a Newton step
    if ((int)blockIdx.x < gA) { spmv_rows(blockIdx.x, gA, tprA, nrowsA, rpA, ciA, valA, xA, epiA); epiA.finish(sm); }
    else { spmv_rows(blockIdx.x - gA, gridDim.x - gA, tprB, nrowsB, rpB, ciB, valB, xB, epiB); epiB.finish(sm); }
}

// row-wise max |a_ij| (Ruiz norms, cholmod_interface.c:162-199) -- one lane group per row
template <int TPR>
__global__ __launch_bounds__(256) void k_row_absmax(int nrows, const int *__restrict__ rp, const double *__restrict__ val,
                                                    double *__restrict__ out) {
    const int lane = threadIdx.x % TPR;
    const int group = (blockIdx.x * BLK + threadIdx.x) / TPR;
    const int ngroups = gridDim.x * (BLK / TPR);
    for (int row = group; row < nrows; row += ngroups) {
        double mx = 0.0;
        for (int k = rp[row] + lane; k < rp[row + 1]; k += TPR) mx = absmax_acc(mx, val[k]);
#pragma unroll
        for (int o = TPR / 2; o > 0; o >>= 1) { double t = __shfl_down(mx, o, TPR); mx = t > mx ? t : mx; }
        if (lane == 0) out[row] = mx;
    }
}
// val[k] = (val[k] * rs[row or col]) * cs[...]: ROW scale then COL scale (scaling.c:56-57)
template <int TPR>
__global__ __launch_bounds__(256) void k_scale_rows_cols(int nrows, const int *__restrict__ rp, const int *__restrict__ ci,
                                                         double *__restrict__ val, const double *__restrict__ first_by_row,
                                                         const double *__restrict__ first_by_col,
                                                         const double *__restrict__ second_by_row,
                                                         const double *__restrict__ second_by_col) {
    const int lane = threadIdx.x % TPR;
    const int group = (blockIdx.x * BLK + threadIdx.x) / TPR;
    const int ngroups = gridDim.x * (BLK / TPR);
    for (int row = group; row < nrows; row += ngroups) {
        for (int k = rp[row] + lane; k < rp[row + 1]; k += TPR) {
            double v = val[k];
            v = v * (first_by_row ? first_by_row[row] : first_by_col[ci[k]]);
            v = v * (second_by_row ? second_by_row[row] : second_by_col[ci[k]]);
            val[k] = v;
        }
    }
}
// Q <- D Q D: val *= (D[col] * D[row]) for a stored lower entry (row i, col j): t = s[j]; x *= t*s[i]
template <int TPR>
__global__ __launch_bounds__(256) void k_scale_sym(int nrows, const int *__restrict__ rp, const int *__restrict__ ci,
                                                   double *__restrict__ val, const double *__restrict__ D) {
    const int lane = threadIdx.x % TPR;
    const int group = (blockIdx.x * BLK + threadIdx.x) / TPR;
    const int ngroups = gridDim.x * (BLK / TPR);
    for (int row = group; row < nrows; row += ngroups) {
        for (int k = rp[row] + lane; k < rp[row + 1]; k += TPR) {
            const int c = ci[k];
            // lower entry (i>=j) is stored as (row=i,col=j): t = D[j] * D[i]; its mirror computes the same product
            const double t = row >= c ? D[c] * D[row] : D[row] * D[c];
            val[k] *= t;
        }
    }
}
__global__ void k_scale_sym_rows(int nrows, int row0, const int *__restrict__ rp, const int *__restrict__ ci, double *__restrict__ val,
                                 const double *__restrict__ D) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
        const int row = r + row0;
        for (int k = rp[r]; k < rp[r + 1]; k++) { const int c = ci[k]; val[k] *= (row >= c ? D[c] * D[row] : D[row] * D[c]); }
    }
}
__global__ void k_scale_vals(long long nnz, double *__restrict__ val, double f) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (long long)gridDim.x * blockDim.x) val[k] *= f;
}
// Jacobi diagonal: diag_j = Q_jj + sigma_f + sum_i A_ij^2 d_i  (row j of CSR(A'))
template <int TPR>
__global__ __launch_bounds__(256) void k_jacobi_diag(int n, const int *__restrict__ rp, const int *__restrict__ ci,
                                                     const double *__restrict__ val, const double *__restrict__ dw,
                                                     const double *__restrict__ qdiag, double sigma_f, double *__restrict__ out) {
    const int lane = threadIdx.x % TPR;
    const int group = (blockIdx.x * BLK + threadIdx.x) / TPR;
    const int ngroups = gridDim.x * (BLK / TPR);
    for (int row = group; row < n; row += ngroups) {
        double s = 0.0;
        for (int k = rp[row] + lane; k < rp[row + 1]; k += TPR) { double v = val[k]; s += v * v * dw[ci[k]]; }
        s = group_sum<TPR>(s);
        if (lane == 0) out[row] = qdiag[row] + sigma_f + s;
    }
}
// deflated variant: P_j = max(remainder_j, 1e-6 * full_j).  The floor bounds the cancellation in the Woodbury
// form u - P^-1 A_h' S^-1 A_h u to six digits; M = P + A_h' D_h A_h stays SPD, which is all PCG requires.
template <int TPR>
__global__ __launch_bounds__(256) void k_jacobi_diag2(int n, const int *__restrict__ rp, const int *__restrict__ ci,
                                                      const double *__restrict__ val, const double *__restrict__ dlight,
                                                      const double *__restrict__ dfull, const double *__restrict__ qdiag,
                                                      double sigma_f, double *__restrict__ out) {
    const int lane = threadIdx.x % TPR;
    const int group = (blockIdx.x * BLK + threadIdx.x) / TPR;
    const int ngroups = gridDim.x * (BLK / TPR);
    for (int row = group; row < n; row += ngroups) {
        double s = 0.0, f = 0.0;
        for (int k = rp[row] + lane; k < rp[row + 1]; k += TPR) { const double v = val[k]; const int c = ci[k]; s += v * v * dlight[c]; f += v * v * dfull[c]; }
        s = group_sum<TPR>(s); f = group_sum<TPR>(f);
        if (lane == 0) {
            const double rem = qdiag[row] + sigma_f + s, full = qdiag[row] + sigma_f + f;
            out[row] = rem > 1e-6 * full ? rem : 1e-6 * full;
        }
    }
}
// diagonal of the inner system of the Schur mode: Sd_i = 1/d_i + sum_j A_ij^2 / Dq_j  (row i of the compact A_c)
template <int TPR>
__global__ __launch_bounds__(256) void k_schur_diag(int k, const int *__restrict__ rp, const int *__restrict__ ci, const double *__restrict__ val,
                                                    const double *__restrict__ Dq, const double *__restrict__ dc, double *__restrict__ out) {
    const int lane = threadIdx.x % TPR;
    const int group = (blockIdx.x * BLK + threadIdx.x) / TPR;
    const int ngroups = gridDim.x * (BLK / TPR);
    for (int row = group; row < k; row += ngroups) {
        double s = 0.0;
        for (int e = rp[row] + lane; e < rp[row + 1]; e += TPR) { const double v = val[e]; s += v * v / Dq[ci[e]]; }
        s = group_sum<TPR>(s);
        if (lane == 0) out[row] = 1.0 / dc[row] + s;
    }
}
__global__ void k_extract_diag(int n, const int *__restrict__ rp, const int *__restrict__ ci, const double *__restrict__ val,
                               double *__restrict__ out) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        double dg = 0.0;
        for (int k = rp[r]; k < rp[r + 1]; k++) if (ci[k] == r) dg += val[k];
        out[r] = dg;
    }
}

__global__ void k_gather_rowinfo(int k, const int *__restrict__ rowlist, const int *__restrict__ rp, const double *__restrict__ dw,
                                 int *__restrict__ cnt, double *__restrict__ dc) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < k; j += gridDim.x * blockDim.x) {
        const int r = rowlist[j];
        cnt[j] = rp[r + 1] - rp[r]; dc[j] = dw[r];
    }
}
// copy the listed rows of a CSR matrix into a contiguous CSR (one wave per row)
__global__ __launch_bounds__(256) void k_copy_rows(int k, const int *__restrict__ rowlist, const int *__restrict__ rp, const int *__restrict__ ci,
                                                   const unsigned short *__restrict__ ci16, const double *__restrict__ val,
                                                   const int *__restrict__ rp2, int *__restrict__ ci2, unsigned short *__restrict__ ci16_2,
                                                   double *__restrict__ val2, int W16) {
    // W16 > 0: the copy has its own slab width (fewer rows per workgroup leave more LDS for the x slice), so the
    // slab-local 16-bit indices are recomputed instead of copied
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * BLK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (BLK >> 6);
    for (int j = wave; j < k; j += nwaves) {
        const int r = rowlist[j];
        const int src = rp[r], len = rp[r + 1] - src, dst = rp2[j];
        for (int e = lane; e < len; e += 64) {
            const int c = ci[src + e];
            ci2[dst + e] = c; val2[dst + e] = val[src + e];
            if (ci16_2) ci16_2[dst + e] = W16 > 0 ? (unsigned short)(c % W16) : ci16[src + e];
        }
    }
}
// ---- per-pass compact matrices with their slab image from ONE read ----------------------------------------------------------------
// An entry's place in the image is its CSR position plus a per-(row, slab) shift, seg.x - sp; a row's slab starts and shifts are loaded once
// per row (wave-uniform) and an entry finds its slab by counting the starts at or below its position (empty segments included: the
// starts are monotone).  Up to PASS_SLABS_MAX slabs; the host keeps the former kernels beyond that.  The loops issue the loads of PASS_U
// 64-entry steps before the first dependent instruction (the walk's base depends on the ballots, its loads do not).
static const int PASS_SLABS_MAX = 8, PASS_U = 8;
// Their grid.  The row loops split the rows statically over the grid, so workgroups beyond those resident at once run after the rest.  The
// per-row tables cost scalar registers, which leave 7 waves per SIMD: 7 x 256 workgroups of 4 waves are resident for the copy on 256 CUs,
// 2048 were not.  The compaction's LDS tables (37.5 KB at m = 2e5) allow it only 4 workgroups per CU; it runs in two rounds with either
// grid and was measured faster with this one as well (C4, with the deeper prefetch: 0.88 -> 0.76 ms); its own optimum was not searched.
static const int PASS_GRID = 7 * 256;
struct RowSlabs {
    int ob[PASS_SLABS_MAX], dl[PASS_SLABS_MAX];
    __device__ __forceinline__ void load(const int *__restrict__ o, const int2 *__restrict__ sg, int nslabs) {
#pragma unroll
        for (int t = 0; t < PASS_SLABS_MAX; t++) {
            ob[t] = t < nslabs ? o[t] : 0x7fffffff;
            dl[t] = t < nslabs ? sg[t].x - o[t] : 0;
        }
    }
    // slab of CSR position p and the shift to its place in the image
    __device__ __forceinline__ int slab(int p, int &shift) const {
        int sl = 0; shift = dl[0];
#pragma unroll
        for (int t = 1; t < PASS_SLABS_MAX; t++) { const bool in = p >= ob[t]; sl += in ? 1 : 0; shift = in ? dl[t] : shift; }
        return sl;
    }
};
// k_copy_rows for a copy that takes the slab kernel: the CSR copy as k_copy_rows writes it, every entry at its slab-major place as well (where
// k_slab_permute would put it: sp and seg of the copy are built first, from the source rows), and with DIAG the row's diagonal of the
// Schur mode's inner system in k_schur_diag<64>'s order (lane L adds entries L, L + 64, ... ascending, group_sum<64>, 1 / dc + s;
// Dq_j = qdiag_j + sigma_f, the one addition of k_axpy_const): the same bits as the three kernels.  (W16 > 0 is the copy's own W: the
// slab-local index c mod W is c - slab W.)
template <bool DIAG>
__global__ __launch_bounds__(256) void k_copy_rows_slab(int k, const int *__restrict__ rowlist, const int *__restrict__ rp, const int *__restrict__ ci,
                                                        const unsigned short *__restrict__ ci16, const double *__restrict__ val,
                                                        const int *__restrict__ rp2, int *__restrict__ ci2, unsigned short *__restrict__ ci16_2,
                                                        double *__restrict__ val2, int W16, int nslabs, int W, const int *__restrict__ sp,
                                                        const int2 *__restrict__ seg, double *__restrict__ vsm, unsigned short *__restrict__ i16sm,
                                                        int *__restrict__ cism, float *__restrict__ vsm32, _Float16 *__restrict__ vsm16, double h16s,
                                                        const double *__restrict__ qdiag, double sigma_f, const double *__restrict__ dc,
                                                        double *__restrict__ sdiag, unsigned short *__restrict__ p16sm) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * BLK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (BLK >> 6);
    for (int jw = wave; jw < k; jw += nwaves) {
        const int j = __builtin_amdgcn_readfirstlane(jw);
        const int r = rowlist[j];
        const int src = rp[r], len = rp[r + 1] - src, dst = rp2[j];
        RowSlabs rs; rs.load(sp + (size_t)j * (nslabs + 1), seg + (size_t)j * nslabs, nslabs);
        double s = 0.0;
        for (int e0 = 0; e0 < len; e0 += 64 * PASS_U) {
            int c[PASS_U]; double v[PASS_U]; unsigned short h[PASS_U];
#pragma unroll
            for (int u = 0; u < PASS_U; u++) {
                const int e = e0 + 64 * u + lane;
                c[u] = 0; v[u] = 0.0; h[u] = 0;
                if (e < len) { c[u] = ci[src + e]; v[u] = val[src + e]; if (ci16_2 && W16 <= 0) h[u] = ci16[src + e]; }
            }
#pragma unroll
            for (int u = 0; u < PASS_U; u++) {
                const int e = e0 + 64 * u + lane;
                if (e < len) {
                    const int p = dst + e;
                    int shift; const int sl = rs.slab(p, shift);
                    const int cl = c[u] - sl * W;
                    const unsigned short c16 = W16 > 0 ? (unsigned short)cl : h[u];
                    ci2[p] = c[u]; val2[p] = v[u];
                    if (ci16_2) ci16_2[p] = c16;
                    const int q = p + shift;
                    vsm[q] = v[u];
                    if (vsm32) vsm32[q] = (float)v[u];
                    if (vsm16) vsm16[q] = h16_round(v[u], h16s);
                    if (i16sm) i16sm[q] = c16; else cism[q] = cl;
                    if (p16sm) p16sm[q] = pair_local(c16, sl, W);
                    if (DIAG) s += v[u] * v[u] / (qdiag[c[u]] + sigma_f);
                }
            }
        }
        if (DIAG) {
            s = group_sum<64>(s);
            if (lane == 0) sdiag[j] = 1.0 / dc[j] + s;
        }
    }
}
__global__ void k_fill_ci16(long long nnz, const int *__restrict__ ci, int W, unsigned short *__restrict__ ci16) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (long long)gridDim.x * blockDim.x)
        ci16[k] = (unsigned short)(ci[k] % W);
}
// ---- per-pass compaction of CSR(A') to the columns (constraints) that carry weight ------------------
// Rows of A with d_i == 0 contribute exact zeros to A' (d .* (A p)); dropping those entries from the
// n x m CSR once per Newton pass removes their HBM traffic from every PCG iteration.  Order inside a
// row is preserved (stable ballot compaction), so the product stays reproducible.
template <int TPR>
__global__ __launch_bounds__(256) void k_count_flagged(int nrows, const int *__restrict__ rp, const int *__restrict__ ci,
                                                       const double *__restrict__ dw, int *__restrict__ cnt) {
    const int lane = threadIdx.x % TPR;
    const int group = (blockIdx.x * BLK + threadIdx.x) / TPR;
    const int ngroups = gridDim.x * (BLK / TPR);
    for (int row = group; row < nrows; row += ngroups) {
        int c = 0;
        for (int k = rp[row] + lane; k < rp[row + 1]; k += TPR) c += (dw[ci[k]] != 0.0);
#pragma unroll
        for (int o = TPR / 2; o > 0; o >>= 1) c += __shfl_down(c, o, TPR);
        if (lane == 0) cnt[row] = c;
    }
}
// The same count with the flags as a bit mask staged in LDS (25 KB at m = 2e5): the per-entry gather dw[ci[k]] -- 2e8 random 8-byte
// reads per pass at C4 -- becomes an LDS lookup and the kernel streams the index array only.
template <int TPR>
__global__ __launch_bounds__(256) void k_count_flagged_bits(int nrows, const int *__restrict__ rp, const int *__restrict__ ci,
                                                            const u64 *__restrict__ bits, int words, int *__restrict__ cnt) {
    extern __shared__ u64 sbits_cnt[];
    for (int i = threadIdx.x; i < words; i += BLK) sbits_cnt[i] = bits[i];
    __syncthreads();
    const int lane = threadIdx.x % TPR;
    const int group = (blockIdx.x * BLK + threadIdx.x) / TPR;
    const int ngroups = gridDim.x * (BLK / TPR);
    for (int row = group; row < nrows; row += ngroups) {
        int c = 0;
        for (int k = rp[row] + lane; k < rp[row + 1]; k += TPR) { const int col = ci[k]; c += (int)((sbits_cnt[col >> 6] >> (col & 63)) & 1ull); }
#pragma unroll
        for (int o = TPR / 2; o > 0; o >>= 1) c += __shfl_down(c, o, TPR);
        if (lane == 0) cnt[row] = c;
    }
}
// compact index space of a Newton pass: cidx[i] = number of weighted rows before i, rowlist = their ids; also the flags as a bit mask
// (bits[w] bit b = row 64 w + b carries weight) and wprefix[w] = cidx[64 w].  Three steps over the 64-row words: the flags of a word as
// its bit mask and their number; a scan of the numbers (dev_scan: wprefix); cidx and rowlist from the masks and the prefix.
__global__ __launch_bounds__(256) void k_flag_words(int m, const double *__restrict__ dw, u64 *__restrict__ bits, int *__restrict__ wcnt) {
    const int lane = threadIdx.x & 63;
    const int words = (m + 63) >> 6, nwaves = gridDim.x * (BLK >> 6);
    for (int w = (blockIdx.x * BLK + threadIdx.x) >> 6; w < words; w += nwaves) {
        const int i = w * 64 + lane;
        const u64 b = __ballot(i < m && dw[i] != 0.0);
        if (lane == 0) { bits[w] = b; wcnt[w] = __popcll(b); }
    }
}
__global__ __launch_bounds__(256) void k_flag_apply(int m, const u64 *__restrict__ bits, const int *__restrict__ wprefix, int *__restrict__ cidx,
                                                    int *__restrict__ rowlist) {
    const int lane = threadIdx.x & 63;
    const int words = (m + 63) >> 6, nwaves = gridDim.x * (BLK >> 6);
    for (int w = (blockIdx.x * BLK + threadIdx.x) >> 6; w < words; w += nwaves) {
        const int i = w * 64 + lane;
        const u64 b = bits[w];
        const int pos = wprefix[w] + __popcll(b & ((1ull << lane) - 1ull));
        if (i < m) { cidx[i] = pos; if ((b >> lane) & 1ull) rowlist[pos] = i; }
    }
}
// one wave per row: stable compaction of (ci, val) pairs whose column weight is nonzero; kept columns are
// renumbered through `remap` (monotone, so rows stay column-sorted) and, if W16 > 0, their slab-local
// 16-bit index is produced as well
__global__ __launch_bounds__(256) void k_compact_rows(int nrows, const int *__restrict__ rp, const int *__restrict__ ci,
                                                      const double *__restrict__ val, const double *__restrict__ dw,
                                                      const int *__restrict__ rp2, int *__restrict__ ci2, double *__restrict__ val2,
                                                      const int *__restrict__ remap, int W16, unsigned short *__restrict__ ci16) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * BLK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (BLK >> 6);
    for (int row = wave; row < nrows; row += nwaves) {
        const int beg = rp[row], end = rp[row + 1];
        int base = rp2[row];
        for (int k0 = beg; k0 < end; k0 += 64) {
            const int k = k0 + lane;
            int c = 0; double v = 0.0; bool keep = false;
            if (k < end) { c = ci[k]; v = val[k]; keep = dw[c] != 0.0; }
            const u64 bal = __ballot(keep);
            if (keep) {
                const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
                const int cn = remap ? remap[c] : c;
                ci2[pos] = cn; val2[pos] = v;
                if (W16 > 0) ci16[pos] = (unsigned short)(cn % W16);
            }
            base += __popcll(bal);
        }
    }
}

// k_compact_rows with the flags and the renumbering as LDS tables: keep = bit, new column = wprefix[word] + popcount of the lower bits
// (= cidx[c]); the same (ci, val) pairs land in the same places.
__global__ __launch_bounds__(256) void k_compact_rows_bits(int nrows, const int *__restrict__ rp, const int *__restrict__ ci,
                                                           const double *__restrict__ val, const u64 *__restrict__ bits, const int *__restrict__ wprefix,
                                                           int words, const int *__restrict__ rp2, int *__restrict__ ci2, double *__restrict__ val2,
                                                           int W16, unsigned short *__restrict__ ci16) {
    extern __shared__ u64 sbits_cmp[];
    int *spre = reinterpret_cast<int *>(sbits_cmp + words);
    for (int i = threadIdx.x; i < words; i += BLK) { sbits_cmp[i] = bits[i]; spre[i] = wprefix[i]; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * BLK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (BLK >> 6);
    for (int row = wave; row < nrows; row += nwaves) {
        const int beg = rp[row], end = rp[row + 1];
        int base = rp2[row];
        for (int k0 = beg; k0 < end; k0 += 64) {
            const int k = k0 + lane;
            int c = 0; double v = 0.0; bool keep = false; u64 wbits = 0;
            if (k < end) { c = ci[k]; v = val[k]; wbits = sbits_cmp[c >> 6]; keep = (wbits >> (c & 63)) & 1ull; }
            const u64 bal = __ballot(keep);
            if (keep) {
                const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
                const int cn = spre[c >> 6] + __popcll(wbits & ((1ull << (c & 63)) - 1ull));
                ci2[pos] = cn; val2[pos] = v;
                if (W16 > 0) ci16[pos] = (unsigned short)(cn % W16);
            }
            base += __popcll(bal);
        }
    }
}

// k_count_flagged_bits, one wave per row, that also delivers the row's slab pointers: the renumbering is monotone, so a kept entry of
// original column c lies in slab t or beyond exactly when c >= rowlist[t W] (thr; no entry when t W >= k).  sp (or null: no slab kernel
// for this matrix) receives the pointers RELATIVE to the row's start: [0, kept below slab 1, ..., all kept]; k_sp_add_rp adds the
// row pointers once they are scanned.  The same counts as k_count_flagged_bits.
__global__ __launch_bounds__(256) void k_count_flagged_slabs(int nrows, const int *__restrict__ rp, const int *__restrict__ ci,
                                                             const u64 *__restrict__ bits, int words, const int *__restrict__ rowlist, int k,
                                                             int nslabs, int W, int *__restrict__ cnt, int *__restrict__ sp) {
    extern __shared__ u64 sbits_cs[];
    for (int i = threadIdx.x; i < words; i += BLK) sbits_cs[i] = bits[i];
    int thr[PASS_SLABS_MAX];
#pragma unroll
    for (int t = 0; t < PASS_SLABS_MAX; t++) thr[t] = (sp && t >= 1 && t < nslabs && (long long)t * W < k) ? rowlist[t * W] : 0x7fffffff;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * BLK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (BLK >> 6);
    for (int row = wave; row < nrows; row += nwaves) {
        const int beg = rp[row], end = rp[row + 1];
        int tot = 0, ge[PASS_SLABS_MAX];
#pragma unroll
        for (int t = 0; t < PASS_SLABS_MAX; t++) ge[t] = 0;
        for (int k0 = beg; k0 < end; k0 += 64 * PASS_U) {
            int col[PASS_U];
#pragma unroll
            for (int u = 0; u < PASS_U; u++) { const int e = k0 + 64 * u + lane; col[u] = e < end ? ci[e] : -1; }
#pragma unroll
            for (int u = 0; u < PASS_U; u++) {
                const bool keep = col[u] >= 0 && ((sbits_cs[col[u] >> 6] >> (col[u] & 63)) & 1ull);
                tot += __popcll(__ballot(keep));
                if (sp) {
#pragma unroll
                    for (int t = 1; t < PASS_SLABS_MAX; t++) if (t < nslabs) ge[t] += __popcll(__ballot(keep && col[u] >= thr[t]));
                }
            }
        }
        if (lane == 0) {
            cnt[row] = tot;
            if (sp) {
                int *o = sp + (size_t)row * (nslabs + 1);
                o[0] = 0; o[nslabs] = tot;
#pragma unroll
                for (int t = 1; t < PASS_SLABS_MAX; t++) if (t < nslabs) o[t] = tot - ge[t];
            }
        }
    }
}
__global__ void k_sp_add_rp(int nrows, int nslabs, const int *__restrict__ rp, int *__restrict__ sp) {
    const long long total = (long long)nrows * (nslabs + 1);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) sp[i] += rp[i / (nslabs + 1)];
}
// k_compact_rows_bits that also writes every kept (index, value) pair at its slab-major place (sp, seg of the compact matrix are built
// first; sp == null: no image).  The same pairs in the same places of the CSR; with an image W16 is its W and cn mod W is cn - slab W.
__global__ __launch_bounds__(256) void k_compact_rows_bits_slab(int nrows, const int *__restrict__ rp, const int *__restrict__ ci,
                                                                const double *__restrict__ val, const u64 *__restrict__ bits,
                                                                const int *__restrict__ wprefix, int words, const int *__restrict__ rp2,
                                                                int *__restrict__ ci2, double *__restrict__ val2, int W16,
                                                                unsigned short *__restrict__ ci16, int nslabs, int W, const int *__restrict__ sp,
                                                                const int2 *__restrict__ seg, double *__restrict__ vsm,
                                                                unsigned short *__restrict__ i16sm, int *__restrict__ cism, float *__restrict__ vsm32,
                                                                _Float16 *__restrict__ vsm16, double h16s, unsigned short *__restrict__ p16sm) {
    extern __shared__ u64 sbits_cmps[];
    int *spre = reinterpret_cast<int *>(sbits_cmps + words);
    for (int i = threadIdx.x; i < words; i += BLK) { sbits_cmps[i] = bits[i]; spre[i] = wprefix[i]; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const u64 lt = (1ull << lane) - 1ull;
    const int wave = (blockIdx.x * BLK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (BLK >> 6);
    for (int roww = wave; roww < nrows; roww += nwaves) {
        const int row = __builtin_amdgcn_readfirstlane(roww);
        const int beg = rp[row], end = rp[row + 1];
        int base = rp2[row];
        RowSlabs rs;
        if (sp) rs.load(sp + (size_t)row * (nslabs + 1), seg + (size_t)row * nslabs, nslabs);
        for (int k0 = beg; k0 < end; k0 += 64 * PASS_U) {
            int c[PASS_U]; double v[PASS_U];
#pragma unroll
            for (int u = 0; u < PASS_U; u++) {
                const int e = k0 + 64 * u + lane;
                c[u] = -1; v[u] = 0.0;
                if (e < end) { c[u] = ci[e]; v[u] = val[e]; }
            }
#pragma unroll
            for (int u = 0; u < PASS_U; u++) {
                u64 wbits = 0; bool keep = false;
                if (c[u] >= 0) { wbits = sbits_cmps[c[u] >> 6]; keep = (wbits >> (c[u] & 63)) & 1ull; }
                const u64 bal = __ballot(keep);
                if (keep) {
                    const int pos = base + __popcll(bal & lt);
                    const int cn = spre[c[u] >> 6] + __popcll(wbits & ((1ull << (c[u] & 63)) - 1ull));
                    ci2[pos] = cn; val2[pos] = v[u];
                    if (sp) {
                        int shift; const int sl = rs.slab(pos, shift);
                        const int cl = cn - sl * W, q = pos + shift;
                        if (W16 > 0) ci16[pos] = (unsigned short)cl;
                        vsm[q] = v[u];
                        if (vsm32) vsm32[q] = (float)v[u];
                        if (vsm16) vsm16[q] = h16_round(v[u], h16s);
                        if (i16sm) i16sm[q] = (unsigned short)cl; else cism[q] = cl;
                        if (p16sm) p16sm[q] = pair_local((unsigned short)cl, sl, W);
                    } else if (W16 > 0) ci16[pos] = (unsigned short)(cn % W16);
                }
                base += __popcll(bal);
            }
        }
    }
}
