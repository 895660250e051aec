// mid_kernels.inc -- part of qpdo_dev.hip (one translation unit; included in order): the dense LDL' of the Newton matrix and the
// forward solve in ONE launch of tile-owning workgroups (written for mid-size orders, measured faster at every order up to 12288)
// ================================================================================================
// Round 5.  Below n ~ 1500 the blocked factorization of dense_kernels.inc is a string of 3 nb + 3 dependent launches (diagonal block,
// panel, update per block column, then the chained solves), each ~10 us whatever it computes: 219 us per Newton pass at n = 200, where
// the factorization itself is 2.7 Mflop (profiles/r04_mid_size_latency.txt).  Here the whole factorization is one launch of
// nb (nb + 1) / 2 workgroups, ONE PER 64 x 64 TILE of the lower triangle, that stay resident and talk through flags:
//   tile (i, j) accumulates  P = sum_{k < j} [L(i, k) D_k] L(j, k)'  on the matrix cores as the tiles of its row and of row j are
//   published (left-looking per tile, accumulators in registers), forms C = K(i, j) - P, and then
//     i == j:  factors the block (diag64_lds_v2), publishes D_j, L_jj^-1;
//     i >  j:  waits for those, L(i, j) = C L_jj^-T / D_j on the matrix cores, publishes it (K's own storage is the mailbox; the
//              transposed copy for the backward solve goes to the upper triangle as in k_ldl_panel).
// The right-hand side rides along as one more block row (nb more workgroups): row block j of the forward solve
//   z_j = L_jj^-1 (b_j - sum_{k<j} L(j, k) z_k),  y_j = z_j / D_j
// is ready one hand-off after the last diagonal block.  The backward solve stays a launch of its own (k_ldl_chain<false>): its
// dependencies run against the dispatch order.
// Hand-off protocol (MI355X_MICROARCH.md, inter-workgroup visibility): the producer stores the bytes with 16-byte sc1 (write-through)
// buffer stores, every storing wave drains them (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, one lane stores the flag (sc1);
// the consumer polls the flag with one lane (sc1 loads, s_sleep), meets at a barrier and reads EVERY handed-off byte with sc1 buffer
// loads (8-byte agent-scope accesses took 4-4.6 us per 32 KB tile against 2 us of matrix-core work: tools/lab/mid_lab.hip).  What no
// workgroup of the same launch reads -- the transposed copies for the backward solve, L of a diagonal tile -- is stored after the flag.  Flags
// carry the launch's epoch, so nothing is reset between launches.  Workgroups are numbered column by column, diagonal tile first: a
// workgroup waits only for workgroups with a smaller index, so the grid drains under in-order dispatch whatever its residency; a
// bounded spin turns a lost producer into C_CHAIN_ERR and the host refactors with the separate kernels (as for k_ldl_chain).
// Order of the arithmetic: per tile the k-sum is accumulated first and subtracted once -- not the right-looking order of the
// multi-launch path, so the factor differs from it in the last bits; the dense path's parity bar is a tolerance.
// ================================================================================================
static const int MID_MAX_NB = 640;                // every order the dense solver accepts (DENSE_LIMIT_N = 40000 -> 625 block columns)
static const int MID_SPIN_MAX = 1 << 22;
// LDS: 63 KB, so that TWO workgroups share a CU (the staging of one overlaps the matrix-core phase of the other: a product runs as two
// 32-deep halves through two 20 KB operand images).  Layout: R0 = S[0 .. 5120) -- the two half images of a product, later the [k][row]
// image of C (64 x 80) or the diagonal block T (64 x 65); R1 = S[5120 .. 7872) -- a 32-deep chunk of L_jj^-1 for the panel product, or
// (with the tail of R0) the inverse blocks / scratch of the diagonal factorization.
static const int MID_LDS_DOUBLES = DNB * DG_TS + 10 * 256 + 64 + DNB * 17;       // = DG_LDS = 7872
#ifdef MID_TIMING
__device__ long long g_mid_t[512][16];
#define MID_T(k) do { if (threadIdx.x == 0) g_mid_t[blockIdx.x][k] = wall_clock64(); } while (0)
#else
#define MID_T(k) do { } while (0)
#endif

// one lane polls up to two flags, the workgroup meets at a barrier; true: a producer was lost
__device__ __forceinline__ bool mid_wait2(const unsigned int *f0, const unsigned int *f1, unsigned int epoch, int tid, int *s_lost) {
    if (tid == 0) {
        int spins = 0;
        while (__hip_atomic_load(f0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
            if (++spins > MID_SPIN_MAX) { *s_lost = 1; break; }
            __builtin_amdgcn_s_sleep(2);
        }
        if (f1) {
            while (!*s_lost && __hip_atomic_load(f1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
                if (++spins > MID_SPIN_MAX) { *s_lost = 1; break; }
                __builtin_amdgcn_s_sleep(2);
            }
        }
    }
    __syncthreads();
    return *s_lost != 0;
}
__device__ __forceinline__ void mid_publish(unsigned int *flag, unsigned int epoch, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 64 x 64 x 32 product on the matrix cores for one workgroup of 4 waves: wave w owns the 32x32 quadrant (w>>1, w&1) as 2x2 tiles of
// v_mfma_f64_16x16x4_f64; As / Bs are [k][row] / [k][col] images, [32][80] (the two k-rows a half-wave reads land on disjoint banks).
// A/B lane map: lane l holds A[l&15][k = l>>4], B[k = l>>4][l&15]; C/D: row = (l>>4) + 4*reg, col = l&15.
__device__ __forceinline__ void mfma_64x64x32(const double (*As)[80], const double (*Bs)[80], dvec4 acc[2][2], int wr, int wc, int li, int lk) {
    // operands of k-step s + 1 are read from LDS before the four products of k-step s are issued (explicit register double buffer:
    // the matrix pipe does not wait for an LDS round trip at the head of every k-step)
    double a0 = As[lk][wr + li], a1 = As[lk][wr + 16 + li], b0 = Bs[lk][wc + li], b1 = Bs[lk][wc + 16 + li];
#pragma unroll
    for (int k0 = 0; k0 < 32; k0 += 4) {
        const int kn = (k0 + 4 < 32) ? k0 + 4 : k0;
        const double na0 = As[kn + lk][wr + li], na1 = As[kn + lk][wr + 16 + li];
        const double nb0 = Bs[kn + lk][wc + li], nb1 = Bs[kn + lk][wc + 16 + li];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
    }
}
// acc += X diag(dv) X' for a 64 x 64 X given as its [k][row] image: ONE image serves both operands, the scaling is applied to the A operand
// on its way from LDS to the matrix cores
__device__ __forceinline__ void mfma_64x64x64_xdx(const double (*Xs)[80], const double *dv, dvec4 acc[2][2], int wr, int wc, int li, int lk) {
    double d = dv[lk];
    double a0 = Xs[lk][wr + li] * d, a1 = Xs[lk][wr + 16 + li] * d, b0 = Xs[lk][wc + li], b1 = Xs[lk][wc + 16 + li];
#pragma unroll
    for (int k0 = 0; k0 < 64; k0 += 4) {
        const int kn = (k0 + 4 < 64) ? k0 + 4 : k0;
        const double nd = dv[kn + lk];
        const double na0 = Xs[kn + lk][wr + li], na1 = Xs[kn + lk][wr + 16 + li];
        const double nb0 = Xs[kn + lk][wc + li], nb1 = Xs[kn + lk][wc + 16 + li];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        a0 = na0 * nd; a1 = na1 * nd; b0 = nb0; b1 = nb1;
    }
}
typedef unsigned int mid_u4 __attribute__((ext_vector_type(4)));
typedef double mid_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mid_rsrc(const double *p, size_t doubles) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(p), 0, (int)(doubles * 8), 0x00020000);
}
__device__ __forceinline__ mid_d2 mid_ld16(__amdgpu_buffer_rsrc_t r, size_t idx) {          // two doubles at element idx (even), sc1
    const mid_u4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(idx * 8), 0, 16);
    mid_d2 o;
    o.x = __hiloint2double((int)v.y, (int)v.x); o.y = __hiloint2double((int)v.w, (int)v.z);
    return o;
}
__device__ __forceinline__ double mid_ld8(__amdgpu_buffer_rsrc_t r, size_t idx) {
    typedef unsigned int u2 __attribute__((ext_vector_type(2)));
    const u2 v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)(idx * 8), 0, 16);
    return __hiloint2double((int)v.y, (int)v.x);
}
__device__ __forceinline__ void mid_st16(__amdgpu_buffer_rsrc_t r, size_t idx, double a, double b) {
    mid_u4 v;
    v.x = (unsigned)__double2loint(a); v.y = (unsigned)__double2hiint(a); v.z = (unsigned)__double2loint(b); v.w = (unsigned)__double2hiint(b);
    __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)(idx * 8), 0, 16);
}
__global__ __launch_bounds__(256) void k_mid_factor(double *__restrict__ K, int n, int ld, int nb, double *__restrict__ Dg, double *__restrict__ Linv,
                                                    double *__restrict__ LinvT, const double *__restrict__ rhs, double *zpub, double *__restrict__ yout,
                                                    unsigned int *flags, unsigned int epoch, Ctrl *ctrl, double *__restrict__ Cpub, double *__restrict__ Dinvg,
                                                    int spec = 0) {
    extern __shared__ __attribute__((aligned(16))) double S[];
    __shared__ int s_lost, s_known;
    __shared__ double dks[DNB];
    const int tid = threadIdx.x;
    if (spec && ctrl->cnt[C_SPEC_SKIP]) return;                     // launch-ahead (vector.inc SpecArgs): this pass is not a Newton step
    // (i, j) of this workgroup: column by column, rows j .. nb-1 and then, with a right-hand side, the extra row nb
    const int nrhs = rhs ? 1 : 0;
    int j = 0, rem = (int)blockIdx.x;
    while (j < nb && rem >= nb - j + nrhs) { rem -= nb - j + nrhs; j++; }
    if (j >= nb) return;
    const int i = j + rem;                                            // i == nb: the right-hand side's block row
    if (tid == 0) s_lost = 0;
    MID_T(0);
    __syncthreads();
    const int wave = tid >> 6, l = tid & 63;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int li = l & 15, lk = l >> 4;
    const int lr = tid & 63, c0 = tid >> 6;
    const int r2 = 2 * (tid & 31), cq = tid >> 5;                     // 16-byte accesses: rows r2, r2 + 1 of columns cq + 8 e
    auto flag_of = [&](int r, int c) { return flags + (size_t)r * nb + c; };
    const __amdgpu_buffer_rsrc_t rL = mid_rsrc(Linv, (size_t)nb * DNB * DNB);
    bool lost = false;
    if (i == nb) {
        // ---- right-hand side, block row j ----------------------------------------------------------------------------------------
        double *zs = S, *part = S + DNB;                              // z_k (64), partial sums [4][64]
        double acc = 0.0;
        for (int k = 0; k < j && !lost; k++) {
            lost = mid_wait2(flag_of(j, k), nullptr, epoch, tid, &s_lost);
            if (lost) break;
            if (tid < DNB) {                                          // z_k: polled like the chained solves (sentinel = not yet written)
                const unsigned long long *src = reinterpret_cast<const unsigned long long *>(zpub) + (size_t)k * DNB + tid;
                unsigned long long bits = CH_SENT; int spins = 0;
                for (;;) {
                    bits = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (bits != CH_SENT) break;
                    if (++spins > MID_SPIN_MAX) { s_lost = 1; bits = 0x7FF8000000000000ULL; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                zs[tid] = __longlong_as_double((long long)bits);
            }
            __syncthreads();
            if (s_lost) { lost = true; break; }
            const double *t = K + (size_t)j * DNB + lr + ((size_t)k * DNB + (size_t)c0 * 16) * ld;
#pragma unroll 4
            for (int q = 0; q < 16; q++) acc += ld_agent(t + (size_t)q * ld) * zs[c0 * 16 + q];
            __syncthreads();                                          // (zs is rewritten by the next k)
        }
        if (!lost) lost = mid_wait2(flag_of(j, j), nullptr, epoch, tid, &s_lost);
        if (!lost) {
            part[c0 * DNB + lr] = acc;
            __syncthreads();
            if (tid < DNB) zs[tid] = rhs[(size_t)j * DNB + tid] - ((part[tid] + part[DNB + tid]) + (part[2 * DNB + tid] + part[3 * DNB + tid]));
            __syncthreads();
            const double *Li = Linv + (size_t)j * DNB * DNB;
            double s = 0.0;
#pragma unroll 4
            for (int q = 0; q < 16; q++) s += ld_agent(&Li[(size_t)(c0 * 16 + q) * DNB + lr]) * zs[c0 * 16 + q];
            __syncthreads();
            part[c0 * DNB + lr] = s;
            __syncthreads();
            if (tid < DNB) {
                const double r = (part[tid] + part[DNB + tid]) + (part[2 * DNB + tid] + part[3 * DNB + tid]);
                unsigned long long rb = (unsigned long long)__double_as_longlong(r);
                if (rb == CH_SENT) rb = 0x7FF8000000000000ULL;
                yout[(size_t)j * DNB + tid] = r / ld_agent(&Dg[(size_t)j * DNB + tid]);
                __hip_atomic_store(reinterpret_cast<unsigned long long *>(zpub) + (size_t)j * DNB + tid, rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (lost && tid == 0) atomicOr(&ctrl->cnt[C_CHAIN_ERR], 1);
        return;
    }
    // ---- tile (i, j): P = sum_{k<j} [L(i,k) D_k] L(j,k)' ----------------------------------------------------------------------------
    double (*As)[80] = reinterpret_cast<double (*)[80]>(S);                       // 64-deep [k][row] image of C (the panel product's A operand)
    double (*Ah)[80] = reinterpret_cast<double (*)[80]>(S);                       // a product's 32-deep halves: A in R0[0 .. 2560), B in R0[2560 .. 5120)
    double (*Bh)[80] = reinterpret_cast<double (*)[80]>(S + 32 * 80);
    double (*Lh)[80] = reinterpret_cast<double (*)[80]>(S + DNB * 80);            // R1: a 32-deep chunk of L_jj^-1
    const size_t base = (size_t)i * DNB + (size_t)j * DNB * ld;
    const __amdgpu_buffer_rsrc_t rT = mid_rsrc(K + base, (size_t)DNB * ld);          // this tile: element (r, c) at r + c ld
    // this tile of the assembled matrix (written by the launch before this one: plain loads), in flight while the products run
    mid_d2 kt[8];
#pragma unroll
    for (int e = 0; e < 8; e++) kt[e] = *reinterpret_cast<const mid_d2 *>(&K[base + r2 + (size_t)(cq + 8 * e) * ld]);
    dvec4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = (dvec4){0.0, 0.0, 0.0, 0.0};
    // `known`: the tiles of both rows are published for every column below it.  mid_ensure(k) blocks until column k is, and looks (without
    // blocking: 64 flag loads in flight at once) up to 31 columns further, so that far from the factorization's front -- where the tiles
    // of old columns have long been there -- the loads of product k + 1 are issued BEFORE product k runs on the matrix cores.
    int known = 0;
    // A diagonal workgroup (j > 0) stops one column short: the tile to its left, L(j, j-1), is the last thing the column before it produces,
    // and waiting for its owner to publish it put two hand-offs on the factorization's critical path (diagonal j-1 -> tile (j, j-1) ->
    // diagonal j: 9.5 of the 21.9 us per block column, tools/lab/mid_lab.hip -DMID_TIMING).  Instead the owner of (j, j-1) publishes its
    // C = K(j, j-1) - P early (it is complete long before diagonal j-1 is), and this workgroup forms X = C L^-T itself when diagonal j-1
    // arrives and applies X D^-1 X' -- one hand-off.
    const bool self_last = (i == j) && j > 0;
    const int kend = self_last ? j - 1 : j;
    auto mid_ensure = [&](int k) -> bool {
        if (wave == 0) {
            // lanes 0-31: row i, columns k .. k + 31; lanes 32-63: row j, the same columns
            const int t = l & 31, kk = k + t;
            const unsigned int *f = (l < 32) ? flag_of(i, kk < kend ? kk : k) : flag_of(j, kk < kend ? kk : k);
            int spins = 0, lead = 0;
            for (;;) {
                bool ok = true;
                if (kk >= kend) ok = false;
                else if (l < 32 || i != j) ok = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch;
                const unsigned long long m = __ballot(ok);
                const unsigned int both = (unsigned int)(m & 0xFFFFFFFFull) & (unsigned int)(m >> 32);
                lead = (both == 0xFFFFFFFFu) ? 32 : __builtin_ctz(~both);          // leading run of published columns from k on
                if (lead >= 1) break;
                if (++spins > MID_SPIN_MAX) { if (l == 0) s_lost = 1; break; }
                __builtin_amdgcn_s_sleep(2);
            }
            if (l == 0) s_known = k + lead;
        }
        __syncthreads();
        known = s_known;
        return s_lost != 0;
    };
    const __amdgpu_buffer_rsrc_t rD = mid_rsrc(Dg, (size_t)ld);
    mid_d2 ra[8], rb[8]; double dk[8];
    auto mid_issue = [&](int k) {
        const __amdgpu_buffer_rsrc_t rA = mid_rsrc(K + (size_t)i * DNB + (size_t)k * DNB * ld, (size_t)DNB * ld);
#pragma unroll
        for (int e = 0; e < 8; e++) ra[e] = mid_ld16(rA, r2 + (size_t)(cq + 8 * e) * ld);
        if (i != j) {
            const __amdgpu_buffer_rsrc_t rB = mid_rsrc(K + (size_t)j * DNB + (size_t)k * DNB * ld, (size_t)DNB * ld);
#pragma unroll
            for (int e = 0; e < 8; e++) rb[e] = mid_ld16(rB, r2 + (size_t)(cq + 8 * e) * ld);
        }
#pragma unroll
        for (int e = 0; e < 8; e++) dk[e] = mid_ld8(rD, (size_t)k * DNB + cq + 8 * e);
    };
    if (kend > 0) { lost = mid_ensure(0); if (!lost) mid_issue(0); }
    for (int k = 0; k < kend && !lost; k++) {
        MID_T(1);
        const bool pre = k + 1 < kend && k + 1 < known;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            __syncthreads();                                          // the previous half product is done with the images
#pragma unroll
            for (int e4 = 0; e4 < 4; e4++) {
                const int e = 4 * h + e4, kh = cq + 8 * e4;           // column kk = cq + 8 e of the tile = row kh of half h (kk = 32 h + kh)
                *reinterpret_cast<mid_d2 *>(&Ah[kh][r2]) = (mid_d2){ra[e].x * dk[e], ra[e].y * dk[e]};
                *reinterpret_cast<mid_d2 *>(&Bh[kh][r2]) = (i != j) ? rb[e] : ra[e];
            }
            __syncthreads();
            if (h == 1) {
                MID_T(2);
#ifndef MID_LAB_NO_LOAD
                if (pre) mid_issue(k + 1);                            // (the registers are free: both halves are in LDS or consumed)
#endif
            }
#ifndef MID_LAB_NO_MFMA
            mfma_64x64x32(Ah, Bh, acc, wr, wc, li, lk);
#endif
        }
        MID_T(3);
#ifndef MID_LAB_NO_LOAD
        if (k + 1 < kend && !pre) { lost = mid_ensure(k + 1); if (!lost) mid_issue(k + 1); }
#else
        if (k + 1 < kend && !pre) lost = mid_ensure(k + 1);
#endif
    }
    if (lost) { if (tid == 0) atomicOr(&ctrl->cnt[C_CHAIN_ERR], 1); return; }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rC = mid_rsrc(Cpub, (size_t)nb * DNB * DNB);
    if (self_last) {
        // ---- the last column's term, made here: X = C(j, j-1) L_{j-1,j-1}^-T, acc += [X D^-1] X' -----------------------------------------
        lost = mid_wait2(flag_of(j - 1, j), nullptr, epoch, tid, &s_lost);          // (the unused upper-triangle slot: "C of (j, j-1) is out")
        if (lost) { if (tid == 0) atomicOr(&ctrl->cnt[C_CHAIN_ERR], 1); return; }
        {
            const size_t co = (size_t)j * DNB * DNB;
            mid_d2 cl[8];
#pragma unroll
            for (int e = 0; e < 8; e++) cl[e] = mid_ld16(rC, co + (size_t)(cq + 8 * e) * DNB + r2);
#pragma unroll
            for (int e = 0; e < 8; e++) *reinterpret_cast<mid_d2 *>(&As[cq + 8 * e][r2]) = cl[e];
        }
        MID_T(13);
        lost = mid_wait2(flag_of(j - 1, j - 1), nullptr, epoch, tid, &s_lost);      // (its barrier also publishes the image)
        if (lost) { if (tid == 0) atomicOr(&ctrl->cnt[C_CHAIN_ERR], 1); return; }
        MID_T(1);
        dvec4 ax[2][2];
        {
            const size_t lo = (size_t)(j - 1) * DNB * DNB;
            mid_d2 lb[8];
#pragma unroll
            for (int e = 0; e < 8; e++) lb[e] = mid_ld16(rL, lo + (size_t)(cq + 8 * e) * DNB + r2);
            if (tid < DNB) dks[tid] = ld_agent(&Dinvg[(size_t)(j - 1) * DNB + tid]);
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) ax[a][b] = (dvec4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (h) __syncthreads();
#pragma unroll
                for (int e4 = 0; e4 < 4; e4++) *reinterpret_cast<mid_d2 *>(&Lh[cq + 8 * e4][r2]) = lb[4 * h + e4];
                __syncthreads();
                // (operands swapped against the panel product below: the accumulators hold X' -- element (c, row), c = wr + 16 a + lk + 4 v,
                // row = wc + 16 b + li -- so that the [k = c][row] operand images of the update are written along rows, without the 8-way
                // bank conflicts of a transposing write: 5.6 us for this step before, tools/lab/mid_lab.hip -DMID_TIMING)
                mfma_64x64x32(Lh, reinterpret_cast<const double (*)[80]>(S + (size_t)h * 32 * 80), ax, wr, wc, li, lk);
            }
        }
        MID_T(2);
        // X' as ONE [k = c][row] image in R0 (every wave writes the sixteen values it holds, along rows); the update scales its A operand
        __syncthreads();                                              // the X product is done with R0
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int v = 0; v < 4; v++)
#pragma unroll
                for (int b = 0; b < 2; b++) As[wr + a * 16 + lk + 4 * v][wc + b * 16 + li] = ax[a][b][v];
        __syncthreads();
        mfma_64x64x64_xdx(As, dks, acc, wr, wc, li, lk);
        MID_T(3);
        __syncthreads();
    }
    if (i == j) {
        // ---- diagonal tile: T = K(j,j) - P, factor, publish D, L^-1 -----------------------------------------------------------------
        double *T = S, *Ic = S + DNB * DG_TS, *cbuf = Ic + 10 * 256, *Xs = cbuf + 64;
#pragma unroll
        for (int e = 0; e < 8; e++) { const int c = cq + 8 * e; T[r2 * DG_TS + c] = kt[e].x; T[(r2 + 1) * DG_TS + c] = kt[e].y; }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int v = 0; v < 4; v++) { double *t = &T[(wr + a * 16 + lk + 4 * v) * DG_TS + wc + b * 16 + li]; *t = *t - acc[a][b][v]; }
        __syncthreads();
        MID_T(4);
        const int ncol = n - j * DNB;
        diag64_lds_v2(T, Ic, Xs, tid, ncol >= DNB ? 4 : (ncol + 15) / 16);
        MID_T(5);
        const size_t lo = (size_t)j * DNB * DNB;
#pragma unroll
        for (int e = 0; e < 8; e++) { const int c = cq + 8 * e; mid_st16(rL, lo + (size_t)c * DNB + r2, diag64_inv(Ic, r2, c), diag64_inv(Ic, r2 + 1, c)); }
        if (tid < DNB) { const double dd = T[tid * DG_TS + tid]; st_agent(&Dg[(size_t)j * DNB + tid], dd); st_agent(&Dinvg[(size_t)j * DNB + tid], 1.0 / dd); }
        mid_publish(flag_of(j, j), epoch, tid);
        MID_T(6);
        // for the launches that follow (the chained solves): L of this tile, the transposed inverse
        double *o2 = LinvT + lo;
#pragma unroll 4
        for (int e = 0; e < DNB / 4; e++) {
            const int c = c0 + 4 * e;
            if (lr > c) K[base + lr + (size_t)c * ld] = T[lr * DG_TS + c];
            o2[(size_t)c * DNB + lr] = diag64_inv(Ic, c, lr);
        }
        return;
    }
    // ---- tile below the diagonal: C = K(i,j) - P as the [k][row] operand image, X = C L_jj^-T, L = X / D ---------------------------
#pragma unroll
    for (int e = 0; e < 8; e++) *reinterpret_cast<mid_d2 *>(&As[cq + 8 * e][r2]) = kt[e];
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int v = 0; v < 4; v++) { double *t = &As[wc + b * 16 + li][wr + a * 16 + lk + 4 * v]; *t = *t - acc[a][b][v]; }
    MID_T(7);
    if (i == j + 1) {
        // the tile left of a diagonal: C goes out for that diagonal's workgroup (see self_last), as the [column][row] image it is here
        __syncthreads();
        const size_t co = (size_t)i * DNB * DNB;
#pragma unroll
        for (int e = 0; e < 8; e++) { const mid_d2 cv = *reinterpret_cast<const mid_d2 *>(&As[cq + 8 * e][r2]); mid_st16(rC, co + (size_t)(cq + 8 * e) * DNB + r2, cv.x, cv.y); }
        mid_publish(flag_of(j, i), epoch, tid);
    }
    lost = mid_wait2(flag_of(j, j), nullptr, epoch, tid, &s_lost);      // (its barrier also publishes the image)
    if (lost) { if (tid == 0) atomicOr(&ctrl->cnt[C_CHAIN_ERR], 1); return; }
    MID_T(8);
    {
        const size_t lo = (size_t)j * DNB * DNB;
        mid_d2 lb[8];
#pragma unroll
        for (int e = 0; e < 8; e++) lb[e] = mid_ld16(rL, lo + (size_t)(cq + 8 * e) * DNB + r2);                  // B[k][c] = (L^-1)[c][k]
        if (tid < DNB) dks[tid] = ld_agent(&Dinvg[(size_t)j * DNB + tid]);                // 1 / D_j (sixteen IEEE divisions per lane were ~0.8 us of this hand-off)
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) acc[a][b] = (dvec4){0.0, 0.0, 0.0, 0.0};
        MID_T(9);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (h) __syncthreads();                                   // the first half product is done with R1
#pragma unroll
            for (int e4 = 0; e4 < 4; e4++) *reinterpret_cast<mid_d2 *>(&Lh[cq + 8 * e4][r2]) = lb[4 * h + e4];
            __syncthreads();
            mfma_64x64x32(reinterpret_cast<const double (*)[80]>(S + (size_t)h * 32 * 80), Lh, acc, wr, wc, li, lk);
        }
    }
    __syncthreads();
    MID_T(10);
    // X as a [col][row] image (row stride 65), then L along contiguous rows; L' for the upper triangle after the flag
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int v = 0; v < 4; v++) S[(wc + b * 16 + li) * (DNB + 1) + wr + a * 16 + lk + 4 * v] = acc[a][b][v];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int col = cq + 8 * e; const double dk = dks[col];
        mid_st16(rT, r2 + (size_t)col * ld, S[col * (DNB + 1) + r2] * dk, S[col * (DNB + 1) + r2 + 1] * dk);
    }
    MID_T(11);
    mid_publish(flag_of(i, j), epoch, tid);
    MID_T(12);
    const double dl = dks[lr];
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) {
        const int row = c0 + 4 * e;
        K[(size_t)j * DNB + lr + ((size_t)i * DNB + row) * ld] = S[lr * (DNB + 1) + row] * dl;
    }
}
