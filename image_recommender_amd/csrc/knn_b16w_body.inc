// knn_b16w_body.inc — the body of the 256 x 256 candidate kernels, included once in each of
// knn_b16w_tile_kernel (B16W_I8T 0) and knn_b16w_tile_kernel_i8t (B16W_I8T 1) in knn_b16w.hip: the
// two share every line of geometry, LDS ring, swizzle, DMA pieces, barrier placement, epilogue,
// shared bound and list fold, and each kernel holds its code directly.  What the int8 tail adds or
// does differently stands under `#if B16W_I8T`, so with B16W_I8T 0 the compiler sees the bf16
// kernel's text token for token (a shared inlined function, or the same text behind `if constexpr`,
// changed the bf16 instances' register allocation and cost them 1 %).  The including kernel
// defines smem, the kernel's parameters, B16W_I8T, `constexpr bool I8T` and `const I8TailArgs ta`.
#if B16W_I8T
#else

#endif
    // XCD-aware bijective block -> (query block, row split) map: the G query blocks of one row
    // split run on one XCD and share its L2 for the corpus tiles
#ifdef IMGREC_B16_STAMPS
    const int wg = blockIdx.x;
    if (threadIdx.x == 0 && wg < 1024) g_b16w_wg[2 * wg] = __builtin_amdgcn_s_memrealtime();
    // stage-loop sums of this wave (B16W_LOOP_BEGIN / _END): [0] int8 tail stages, [1] bf16 stages
    unsigned long long lp_cyc[2] = {0, 0}, lp_rt[2] = {0, 0}, lp_n[2] = {0, 0};
#endif
    const int wgid = xcd_wgid();
    constexpr int kG = 4;
    const int G = (nqb % kG == 0) ? kG : nqb;
    const int qbg = wgid / (nsplit * G), rem = wgid - qbg * (nsplit * G);
    const int split = rem / G;
    const int qb = qbg * G + rem % G;
    // this split's rows (header): cnt groups, global group split + m * nsplit for m < cnt; trow =
    // stored row of tile row tr of tile t (groups past the split's end: the tile's first group)
    const int ngroups = (nrows + kRPP - 1) / kRPP;
    const int cnt = split < ngroups ? (ngroups - split + nsplit - 1) / nsplit : 0;
    const int t0 = 0, t1 = (cnt + kGPT - 1) / kGPT;
    auto trow = [&](int t, int tr) {
        const int m = t * kGPT + tr / kRPP;
        return (split + (m < cnt ? m : t * kGPT) * nsplit) * kRPP + tr % kRPP;
    };

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lc = lane & 15, lq = lane >> 4;
    int qcol[2];
    qcol[0] = qb * kBQ + wave * kQW + lc;
    qcol[1] = qcol[0] + 16;
#if B16W_I8T
    // (I8T has no register to spare — the bf16 instances sit at 256 — so there the query columns,
    // and the 64-bit addresses the compiler derives from them, are worked out again at every use
    // from the lane's column, which the empty asm keeps the compiler from hoisting)
    auto qcol_of = [&](int h) __attribute__((always_inline)) {
        if constexpr (!I8T) return qcol[h];
        int l = lc;
        asm volatile("" : "+v"(l));
        return qb * kBQ + wave * kQW + l + 16 * h;
    };
#endif
    float qn[2] = {0.f, 0.f};
#if B16W_I8T
    if constexpr (!I8T) {
        if (L2) { qn[0] = qnorm[qcol[0]]; qn[1] = qnorm[qcol[1]]; }
        asm volatile("" : "+v"(qn[0]), "+v"(qn[1]));
    }
    // I8T: the wave's queries' tail scales wait in LDS for the fold (the kernel has no register to
    // spare: the bf16 instances sit at 256)
    float* const lsq = reinterpret_cast<float*>(smem + (I8T ? kQScaleOff : 0)) + wave * kQW;
    float* const lqn = reinterpret_cast<float*>(smem + (I8T ? kQNormOff : 0)) + wave * kQW;
    if constexpr (I8T)
        if (lane < kQW) {
            lsq[lane] = ta.qts[qb * kBQ + wave * kQW + lane];
            lqn[lane] = L2 ? qnorm[qb * kBQ + wave * kQW + lane] : 0.f;
        }
#else
    if (L2) { qn[0] = qnorm[qcol[0]]; qn[1] = qnorm[qcol[1]]; }
    asm volatile("" : "+v"(qn[0]), "+v"(qn[1]));
#endif

    // ---- DMA (header): waves 0-3 move the corpus tile, 4-7 the query tile; lane -> (row prow of
    // the piece, chunk pchk), source chunk pre-swizzled
    const bool isA = wave < 4;
    if (!isA) __builtin_amdgcn_s_setprio(1);
    const int pbase = (isA ? wave : wave - 4) * kLPW;
    const int prow = lane / kCPR, pchk = lane % kCPR;
    static_assert(kRPP == 8 && kRPB == 2 && kLPW % 2 == 0, "piece offset form");
    // (I8T: xh, qh and dw are the joint rows — tail codes, then the bf16 head — so one stride serves
    // every stage and the offsets are the bf16 kernel's)
    uint32_t vpar[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int P = pbase + e, r = P * kRPP + prow;
        const int srow = isA ? P * nsplit * kRPP + prow : r;
        vpar[e] = (uint32_t)srow * (uint32_t)(dw * 4) + 16u * (uint32_t)(pchk ^ ((r / kRPB) % kCPR));
    }
    const uint32_t kPS = (uint32_t)((isA ? nsplit : 1) * kRPP * dw * 4);
    auto voff_of = [&](int j) {
        return vpar[j & 1] + (uint32_t)(j & ~1) * kPS - 1024u * (uint32_t)(j & 3);
    };
    const uint32_t smem0 = lds_u32(smem);
    const uint32_t pdst = (uint32_t)((isA ? 0 : kSA) + pbase * 1024);

    // fragment read offsets: k-step c of lane quarter lq = logical chunk 4c + lq of row lc of a
    // 16-row block (the swizzle of row lc is the same in every block: (lc >> 1) & 7)
    const int fsw = (lc / kRPB) % kCPR;
    int aoff[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) aoff[c] = lc * kRowB + 16 * ((4 * c + lq) ^ fsw);
    const int boff = kSA + wave * kQW * kRowB;

    float kd[2][KM];
    int ki[2][KM];
    uint32_t kp[2][KM];
    const uint32_t lowm = PACK ? (1u << ib) - 1u : 0u;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int p = 0; p < KM; ++p) {
            if constexpr (PACK) kp[h][p] = ~0u;
            else { kd[h][p] = INFINITY; ki[h][p] = -1; }
        }

    // Shared screen bound (TileArgs::sbound, DESIGN.md "Shared screen bound").  For a tile (see
    // rec_due) the wave copies the records of its kQW queries (2 KiB, contiguous) into LDS with two
    // agent-scope LDS-DMA loads issued one stage before the tile's last, so they land under the
    // stage loop's own wait and no register or memory wait is spent on them; the epilogue reads, per query,
    // the slots (lane quarter lq: words 4 lq .. 4 lq + 3) and the limit coefficients.  U = the
    // largest slot bounds the query's KM-th best approximate key over the whole corpus from above
    // (the slots hold keys of rows of KM distinct row splits); +inf while a slot is empty.
    // lu = the smallest L(U) seen so far and the value last published live per query in LDS
    // (written by the query's lane of quarter 0, read by its four lanes: one wave, in order).
    const bool sb_on = sbound != nullptr;
    uint32_t* const wrec = sbound + (size_t)(qb * kBQ + wave * kQW) * kSBWords;    // wave-uniform
    const uint32_t* const lrec = reinterpret_cast<const uint32_t*>(smem + kRecOff) + wave * (kQW * kSBWords);
    uint2* const lst = reinterpret_cast<uint2*>(smem + kLuOff) + wave * kQW;
    if (sb_on && lq == 0) {
        lst[lc] = make_uint2(__float_as_uint(INFINITY), ~0u);
        lst[lc + 16] = make_uint2(__float_as_uint(INFINITY), ~0u);
    }
    auto rec_dma = [&]() __attribute__((always_inline)) {
        dma2_agent(wrec, smem0 + (uint32_t)(kRecOff + wave * (kQW * kSBWords * 4)), (uint32_t)lane * 16u);
    };

    // stages per tile (I8T: a joint row's first nst_t stages are its tail codes, the rest its head)
    const int nst = dw / kBKW;
#if B16W_I8T
    const int nst_t = ta.nst_t;
#endif
    const int total = (t1 - t0) * nst;
    const uint32_t* qblk = qh + (size_t)qb * kBQ * dw;

    int c_it = t0, c_is = 0;
    const uint32_t* c_tile = isA ? xh + (size_t)trow(t0, 0) * dw : qblk;
    int c_ng = (isA && t0 == t1 - 1) ? cnt - t0 * kGPT : kGPT;
    auto issue = [&](int g) __attribute__((always_inline)) {
#if B16W_I8T
        // (the unpacked I8T instances have no registers for the eight hoisted piece offsets — KM = 10,
        // L2 spilled one — so theirs are added up from the two pinned bases at every issue: nine
        // vector adds, no division or multiply; the packed instances hoist them as the bf16 kernel does)
        uint32_t vp[2] = {vpar[0], vpar[1]};
        if constexpr (!PACK) asm volatile("" : "+v"(vp[0]), "+v"(vp[1]));
        auto voff_of = [&](int j) {
            return vp[j & 1] + (uint32_t)(j & ~1) * kPS - 1024u * (uint32_t)(j & 3);
        };
#endif
        const uint32_t* src = c_tile + c_is * kBKW;
        const uint32_t dst = smem0 + (uint32_t)((g & (kNS - 1)) * kStage) + pdst;
        if (pbase + kLPW <= c_ng || !isA) {
#pragma unroll
            for (int h = 0; h < kLPW / 4; ++h)
                dma4x(src, dst + 4096u * h, voff_of(4 * h), voff_of(4 * h + 1), voff_of(4 * h + 2),
                      voff_of(4 * h + 3));
        } else {
            // the split's last, partial tile: pieces past its groups are skipped
#pragma unroll
            for (int j = 0; j < kLPW; ++j)
                if (pbase + j < c_ng) {
                    const uint32_t d = dst + 4096u * (j / 4);
                    switch (j & 3) {
                        case 0: dma1<0>(src, d, voff_of(j)); break;
                        case 1: dma1<1024>(src, d, voff_of(j)); break;
                        case 2: dma1<2048>(src, d, voff_of(j)); break;
                        default: dma1<3072>(src, d, voff_of(j)); break;
                    }
                }
        }
        if (c_is == 0 && wave < 4)
            dma4_norm(xnorm + trow(c_it, wave * 64 + lane),
                      smem0 + (uint32_t)(kNormOff + ((c_it - t0) & (kNormSlots - 1)) * kBM * 4 + wave * 256));
#if B16W_I8T
        if constexpr (I8T)
            if (c_is == 0 && wave < 4)
                dma4_norm(ta.xts + trow(c_it, wave * 64 + lane),
                          smem0 + (uint32_t)(kScaleOff + ((c_it - t0) & (kNormSlots - 1)) * kBM * 4 + wave * 256));
#endif
        if (++c_is == nst) {
            c_is = 0;
            ++c_it;
            if (isA) {
                c_tile = xh + (size_t)trow(c_it, 0) * dw;
                c_ng = c_it == t1 - 1 ? cnt - c_it * kGPT : kGPT;
            }
        }
    };
    static_assert(kNS == 2 && kNormSlots == 4, "power-of-two ring slots");

    constexpr int kJ = (KM + 3) / 4;
    constexpr float kLo = 1.0f / 1048576.f;

    // quad q of a stage: k-step q >> 2, row blocks 4 (q & 3) .. + 3
    auto read_a = [&](const char* sb, int q, u32x4 (&fa)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            fa[j] = *reinterpret_cast<const u32x4*>(sb + aoff[q >> 2] + (4 * (q & 3) + j) * 16 * kRowB);
    };
    auto read_b = [&](const char* sb, int c, u32x4 (&fb)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) fb[h] = *reinterpret_cast<const u32x4*>(sb + aoff[c] + boff + h * 16 * kRowB);
    };
#if B16W_I8T
    // (tl_tag: a tail stage — the int8 MFMA on the same registers, read and written as int32)
    auto mfma_quad = [&](auto tl_tag, f32x4 (&acc)[kRB][2], const u32x4 (&fa)[4], const u32x4 (&fb)[2], int q) __attribute__((always_inline)) {
#else
    auto mfma_quad = [&](f32x4 (&acc)[kRB][2], const u32x4 (&fa)[4], const u32x4 (&fb)[2], int q) __attribute__((always_inline)) {
#endif
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
#if B16W_I8T
            for (int h = 0; h < 2; ++h) {
                if constexpr (decltype(tl_tag)::value)
                    acc[4 * (q & 3) + j][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x64_i8(
                        __builtin_bit_cast(i32x4, fa[j]), __builtin_bit_cast(i32x4, fb[h]),
                        __builtin_bit_cast(i32x4, acc[4 * (q & 3) + j][h]), 0, 0, 0));
                else
                    acc[4 * (q & 3) + j][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        __builtin_bit_cast(bf16x8, fa[j]), __builtin_bit_cast(bf16x8, fb[h]), acc[4 * (q & 3) + j][h], 0, 0, 0);
            }
#else
            for (int h = 0; h < 2; ++h)
                acc[4 * (q & 3) + j][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    __builtin_bit_cast(bf16x8, fa[j]), __builtin_bit_cast(bf16x8, fb[h]), acc[4 * (q & 3) + j][h], 0, 0, 0);
#endif
    };

    u32x4 fa[2][4], fb[2][2];
    int g = 0;
    int pend = -1;
    if (total > 0) {
        issue(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        barrier_lds();
        if (total > 1) issue(1);
        read_a(smem, 0, fa[0]);
        read_b(smem, 0, fb[0]);
    }
    for (int t = t0; t < t1; ++t) {
#ifdef IMGREC_B16_STAMPS
        const bool stamp_on = blockIdx.x == 100 && t - t0 < 120;
        int nit = 0;
        unsigned long long ins_cyc = 0;      // cycles inside the insertion blocks of this tile
#endif
        f32x4 acc[kRB][2];
#pragma unroll
        for (int rb = 0; rb < kRB; ++rb)
#pragma unroll
            for (int h = 0; h < 2; ++h) acc[rb][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // the records are fetched for a split's first four tiles, then for every fourth: U falls
        // like 1 / tiles done, and the corpus stream evicts the records from L2 between tiles, so
        // each fetch is HBM traffic (a tile without one screens with the image it has)
        const bool rec_due = sb_on && (t - t0 < 4 || ((t - t0) & 3) == 0);
        // live quad rows (64 tile rows each) of this tile: a split's partial last tile runs the
        // MFMAs, fragment reads and screens of its live row blocks only
        const int nlive = (t + 1) * kGPT <= cnt ? 4 : (((cnt - t * kGPT) * kRPP + 63) >> 6);
        // one tile's stages with NR live quad rows: per stage 2 k-steps x NR quads, quad i =
        // (k-step i / NR, quad row i % NR); the next quad's fragments are read under the current
        // one's MFMAs (the second k-step's B fragments under the first k-step's last quad); the
        // barrier sits before the last quad, after which the next stage's first fragments are
        // read and the corpus-tile waves issue the DMA of the stage after it
#if B16W_I8T
        // (ns stages, the tile's stages s0 .. s0 + ns - 1; more: a stage of this tile follows them)
        auto stage_loop = [&](auto nr_tag, auto tl_tag, int ns, int s0, bool more) __attribute__((always_inline)) {
#else
        auto stage_loop = [&](auto nr_tag) __attribute__((always_inline)) {
#endif
            constexpr int NR = decltype(nr_tag)::value, L = 2 * NR;
#if B16W_I8T
            for (int s = 0; s < ns; ++s, ++g) {
#else
            for (int s = 0; s < nst; ++s, ++g) {
#endif
                const char* sb = smem + (g & 1) * kStage;
#pragma unroll
                for (int i = 0; i + 1 < L; ++i) {
                    read_a(sb, 4 * ((i + 1) / NR) + (i + 1) % NR, fa[(i + 1) & 1]);
                    if (i == NR - 1) read_b(sb, 1, fb[1]);
#if B16W_I8T
                    mfma_quad(tl_tag, acc, fa[i & 1], fb[i / NR], 4 * (i / NR) + i % NR);
#else
                    mfma_quad(acc, fa[i & 1], fb[i / NR], 4 * (i / NR) + i % NR);
#endif
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
                    }
                    if (i == NR - 1) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                    } else {
                        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (i == (kDeferQ < L - 2 ? kDeferQ : L - 2) && pend >= 0) {
                        __builtin_amdgcn_sched_barrier(0);
                        issue(pend);
                        pend = -1;
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                barrier_lds();
                __builtin_amdgcn_sched_barrier(0);
#if B16W_I8T
                if (s + 1 < ns || more) {
#else
                if (s + 1 < nst) {
#endif
                    const char* nb = smem + ((g + 1) & 1) * kStage;
                    read_a(nb, 0, fa[0]);
                    read_b(nb, 0, fb[0]);
                }
                if (g + 2 < total) {
                    if (isA) issue(g + 2);
                    else pend = g + 2;
                }
#if B16W_I8T
                if (rec_due && s0 + s + 2 == nst) rec_dma();
                mfma_quad(tl_tag, acc, fa[1], fb[1], 4 + NR - 1);
            }
        };
        // a tile with NR live quad rows.  I8T: its tail stages, the fold, its head stages — the fold
        // turns the int32 dots of the codes into the fp32 inner products of the tails, in place, for
        // the live row blocks (the scales of the tile's rows came with its first stage, in a ring like
        // the norms'; the wave's queries' scales wait in LDS)
        auto tile_stages = [&](auto nr_tag) __attribute__((always_inline)) {
            if constexpr (I8T) {
                constexpr int NR = decltype(nr_tag)::value;
                { B16W_LOOP_BEGIN(); stage_loop(nr_tag, std::true_type{}, nst_t, 0, nst > nst_t); B16W_LOOP_END(0, nst_t); }
                const float* scl = reinterpret_cast<const float*>(smem + kScaleOff + ((t - t0) % kNormSlots) * kBM * 4);
                const float sq[2] = {lsq[lc], lsq[lc + 16]};
#pragma unroll
                for (int rb = 0; rb < (IMGREC_B16W_EPI_EXP == 3 ? 0 : 4 * NR); ++rb) {
                    const float4 s4 = *reinterpret_cast<const float4*>(scl + rb * 16 + 4 * lq);
                    const float sr[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const i32x4 ai = __builtin_bit_cast(i32x4, acc[rb][h]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[rb][h][i] = (float)ai[i] * sr[i] * sq[h];
                    }
                    // (pinned: left alone, the compiler moves the arithmetic away from the loads and
                    // keeps every row block's scales in registers at once)
                    asm volatile("" : "+v"(acc[rb][0]), "+v"(acc[rb][1]));
                }
                { B16W_LOOP_BEGIN(); stage_loop(nr_tag, std::false_type{}, nst - nst_t, nst_t, false); B16W_LOOP_END(1, nst - nst_t); }
            } else {
                stage_loop(nr_tag, std::false_type{}, nst, 0, false);
#else
                if (rec_due && s + 2 == nst) rec_dma();
                mfma_quad(acc, fa[1], fb[1], 4 + NR - 1);
#endif
            }
        };
        if (rec_due && nst < 2) rec_dma();           // a one-stage tile: before its only wait
#if B16W_I8T
        if (nlive >= 4) tile_stages(std::integral_constant<int, 4>{});
        else if (nlive == 3) tile_stages(std::integral_constant<int, 3>{});
        else if (nlive == 2) tile_stages(std::integral_constant<int, 2>{});
        else tile_stages(std::integral_constant<int, 1>{});
#else
#ifdef IMGREC_B16_STAMPS
        B16W_LOOP_BEGIN();
#endif
        if (nlive >= 4) stage_loop(std::integral_constant<int, 4>{});
        else if (nlive == 3) stage_loop(std::integral_constant<int, 3>{});
        else if (nlive == 2) stage_loop(std::integral_constant<int, 2>{});
        else stage_loop(std::integral_constant<int, 1>{});
#ifdef IMGREC_B16_STAMPS
        B16W_LOOP_END(1, nst);
#endif
#endif

        // ---- top-k epilogue of tile t.  Screen: a row matters only if its key beats T = min(the
        // K-th of any of the query's four lane lists, max over them of their J-th best) — four
        // lists holding J >= KM/4 entries each at or below that max give the union KM better
        // entries, and a dropped row ranks behind the folded list's last entry (merge floor).
        // The test runs on the accumulator, so a row that fails costs no key: d = (|x|^2 (1/2 -
        // 2^-20) + c) - acc with c = (|q|^2 - T)/2 - 2^-20 (|q|^2 + |T|) is negative iff the row
        // passes (the 2^-20 terms keep fp32 rounding from rejecting a row the exact key would
        // keep); two packed adds per pair of rows and one v_alignbit per row shift the sign bits
        // into a 16-bit lane mask per 64-row group.  A lane's passing rows are then visited one
        // per round, keyed and inserted.
        B16W_STAMP(2 * (t - t0));
#if IMGREC_B16W_EPI_EXP != 0
#pragma unroll
        for (int rb = 0; rb < kRB; ++rb)
#pragma unroll
            for (int h = 0; h < 2; ++h) asm volatile("" :: "v"(acc[rb][h]));
#endif
        const float* nrm = reinterpret_cast<const float*>(smem + kNormOff + ((t - t0) % kNormSlots) * kBM * 4);
        const bool full = (t + 1) * kGPT <= cnt && trow(t, kBM - 1) < nrows;
        auto row_ok = [&](int tr) { return t * kGPT + tr / kRPP < cnt && trow(t, tr) < nrows; };
#if B16W_I8T
        // (I8T: the queries' norms come from LDS for the epilogue's duration)
        if constexpr (I8T && L2 != 0) { qn[0] = lqn[lc]; qn[1] = lqn[lc + 16]; }
#endif
        float lu[2] = {INFINITY, INFINITY};
        if (sb_on) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                // U and L(U) = U + (A + B |U|) >= prefix_limit(a) for every a <= U (the prep kernel
                // inflated A, B: QueryBounds::limit_coefs); an empty slot (~0u), +inf or a NaN: no
                // bound.  Words KM .. 11 of a record are 0; quarter 3 holds (A, B, floor, 0).
                const uint4 c = *reinterpret_cast<const uint4*>(lrec + (lc + 16 * h) * kSBWords + 4 * lq);
                const uint32_t ub = quarter_max_u(lq < 3 ? max(max(c.x, c.y), max(c.z, c.w)) : 0u);
                const float cA = __uint_as_float(quarter_max_u(lq == 3 ? c.x : 0u));
                const float cB = __uint_as_float(quarter_max_u(lq == 3 ? c.y : 0u));
                const float U = ord_float(ub);
                const float L = ub >= 0xff800000u ? INFINITY : U + fmaf(cB, fabsf(U), cA);
                lu[h] = fminf(__uint_as_float(lst[lc + 16 * h].x), L);
            }
        }
        float cth[2];
        auto screen = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float T;
                if constexpr (PACK) T = bucket_end(min(quarter_min_u(kp[h][KM - 1]), quarter_max_u(kp[h][kJ - 1])), lowm);
                else T = fminf(quarter_min(kd[h][KM - 1]), quarter_max(kd[h][kJ - 1]));
                T = fminf(T, lu[h]);
                const float c = L2 ? 0.5f * (qn[h] - T) - kLo * (qn[h] + fabsf(T)) : -T;
#if B16W_I8T
                cth[h] = qcol_of(h) < nq ? c : INFINITY;
#else
                cth[h] = qcol[h] < nq ? c : INFINITY;
#endif
            }
        };
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            if (rg >= nlive || IMGREC_B16W_EPI_EXP == 1) break;
            // row group rg = row blocks 4 rg .. 4 rg + 3; bit 4 j + i of a mask = accumulator
            // register i of row block 4 rg + j = tile row (4 rg + j) * 16 + 4 lq + i
            screen();
            unsigned live = 0xffffu;
            if (!full) {
                live = 0;
#if B16W_I8T
                // (a partial tile's path: its lane constants are worked out here, not kept for the launch)
                int lq_c = lq;
                asm volatile("" : "+v"(lq_c));
#pragma unroll
                for (int b = 0; b < 16; ++b) live |= (unsigned)row_ok((4 * rg + (b >> 2)) * 16 + 4 * lq_c + (b & 3)) << b;
#else
#pragma unroll
                for (int b = 0; b < 16; ++b) live |= (unsigned)row_ok((4 * rg + (b >> 2)) * 16 + 4 * lq + (b & 3)) << b;
#endif
            }
            unsigned msk[2] = {0u, 0u};
            float4 nr4[4];                                      // the group's row norms
#pragma unroll
            for (int j = 3; j >= 0; --j) {                      // high bits first
                const int rb = 4 * rg + j;
                float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (L2) n4 = *reinterpret_cast<const float4*>(nrm + rb * 16 + 4 * lq);
                nr4[j] = n4;
                const f32x2 half2 = (f32x2){0.5f - kLo, 0.5f - kLo};
                const f32x2 hlo = (f32x2){n4.x, n4.y} * half2, hhi = (f32x2){n4.z, n4.w} * half2;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f32x2 c2 = (f32x2){cth[h], cth[h]};
                    const f32x2 dhi = (L2 ? hhi + c2 : c2) - (f32x2){acc[rb][h][2], acc[rb][h][3]};
                    const f32x2 dlo = (L2 ? hlo + c2 : c2) - (f32x2){acc[rb][h][0], acc[rb][h][1]};
                    msk[h] = __builtin_amdgcn_alignbit(msk[h], __float_as_uint(dhi.y), 31);
                    msk[h] = __builtin_amdgcn_alignbit(msk[h], __float_as_uint(dhi.x), 31);
                    msk[h] = __builtin_amdgcn_alignbit(msk[h], __float_as_uint(dlo.y), 31);
                    msk[h] = __builtin_amdgcn_alignbit(msk[h], __float_as_uint(dlo.x), 31);
                }
            }
#ifdef IMGREC_B16_STAMPS
            const unsigned long long ins0 = __builtin_amdgcn_s_memtime();
#endif
#if IMGREC_B16W_EPI_EXP == 2
            asm volatile("" :: "v"(msk[0] & live), "v"(msk[1] & live));   // the screen, no insertion
            continue;
#endif
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned m = msk[h] & live;
                if (!__any(m != 0)) continue;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {                // row blocks 4 rg + 2 hf, + 1
                    unsigned mh = (m >> (8 * hf)) & 0xffu;
                    if (!__any(mh != 0)) continue;
                    const int rb0 = 4 * rg + 2 * hf;
                    while (__any(mh != 0)) {
#ifdef IMGREC_B16_STAMPS
                        ++nit;
#endif
                        const bool act = mh != 0u;
                        const int r8 = act ? __builtin_ctz(mh) : 0;
                        mh &= mh - 1u;
                        const int tr = (rb0 + (r8 >> 2)) * 16 + 4 * lq + (r8 & 3);
                        const float a = sel8(r8, acc[rb0][h][0], acc[rb0][h][1], acc[rb0][h][2], acc[rb0][h][3],
                                             acc[rb0 + 1][h][0], acc[rb0 + 1][h][1], acc[rb0 + 1][h][2],
                                             acc[rb0 + 1][h][3]);
                        const float4 na = nr4[2 * hf], nb = nr4[2 * hf + 1];
                        const float xn = L2 ? sel8(r8, na.x, na.y, na.z, na.w, nb.x, nb.y, nb.z, nb.w) : 0.f;
                        float kv = L2 ? fmaf(-2.f, a, qn[h] + xn) : -a;
                        if constexpr (PACK) {
                            // L2: the clamp at 0 and the order map in two integer ops — a key
                            // with the sign bit set (negative or -0) maps to ord(+0) = 2^31, a
                            // non-negative one to its bits | 2^31
                            const uint32_t ob = L2 ? ((uint32_t)max((int)__float_as_uint(kv), 0) | 0x80000000u)
                                                   : ord_bits(kv);
                            const uint32_t u = (ob & ~lowm) | (uint32_t)(t * kBM + tr);
                            insert_packed<KM>(kp[h], __builtin_unpredictable(act) ? u : ~0u);
                        } else {
                            if (L2) kv = kv < 0.f ? 0.f : kv;
                            kv = __builtin_unpredictable(act && kv < kd[h][KM - 1]) ? kv : INFINITY;
                            insert_mono<KM>(kd[h], ki[h], kv, trow(t, tr));
                        }
                    }
                }
            }
#ifdef IMGREC_B16_STAMPS
            ins_cyc += __builtin_amdgcn_s_memtime() - ins0;
#endif
        }
        if (sb_on) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                // publish the best key of the query's four lists when it improved on the value
                // last published: an upper bound of that row's approximate key (PACK: the end of
                // its bucket), into the slot of this row split's residue class; one lane per
                // query, pad queries never, an empty list (PACK: the increment wraps to 0) neither
                const uint32_t best = quarter_min_u(PACK ? kp[h][0] : ord_bits(kd[h][0]));
                uint32_t pubd = lst[lc + 16 * h].y;
                const uint32_t pub = PACK ? (best | lowm) + 1u : best;
                if (lq == 0) {
#if B16W_I8T
                    const int qc = qcol_of(h);
                    if (qc < nq && pub != 0u && pub < 0xff800000u && pub < pubd) {
                        __hip_atomic_fetch_min(sbound + (size_t)qc * kSBWords + split % KM, pub,
#else
                    if (qcol[h] < nq && pub != 0u && pub < 0xff800000u && pub < pubd) {
                        __hip_atomic_fetch_min(sbound + (size_t)qcol[h] * kSBWords + split % KM, pub,
#endif
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        pubd = pub;
                    }
                    lst[lc + 16 * h] = make_uint2(__float_as_uint(lu[h]), pubd);
                }
            }
        }
        B16W_STAMP(2 * (t - t0) + 1);
#ifdef IMGREC_B16_STAMPS
        if (stamp_on && lane == 0) g_b16w_stamps[wave * 256 + 128 + (t - t0)] = (unsigned long long)nit;
        if (stamp_on && lane == 0 && t - t0 < 64) g_b16w_stamps[wave * 256 + 192 + (t - t0)] = ins_cyc;
#endif
        if (g < total) {
            read_a(smem + (g & 1) * kStage, 0, fa[0]);
            read_b(smem + (g & 1) * kStage, 0, fb[0]);
        }
    }

#ifdef IMGREC_B16_STAMPS
    if (threadIdx.x == 0 && wg < 1024) g_b16w_wg[2 * wg + 1] = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && wg < 1024)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            g_b16w_loop[6 * wg + 3 * i] = lp_cyc[i];
            g_b16w_loop[6 * wg + 3 * i + 1] = lp_rt[i];
            g_b16w_loop[6 * wg + 3 * i + 2] = lp_n[i];
        }
#endif
    // ---- one list per (query, row split): fold lane quarters 2, 3 into 0, 1 (lane ^ 32), then
    // quarter 1 into 0 (lane ^ 16).  Entries a fold drops rank behind the folded list's last
    // entry, which the merge floor covers.
#pragma unroll
    for (int x = 32; x >= 16; x >>= 1) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (PACK) {
                // every lane merges its partner's list as it was before the fold (both lists
                // change in this step; a list must not take an entry it already holds)
                uint32_t o[KM];
#pragma unroll
                for (int p = 0; p < KM; ++p) o[p] = (uint32_t)__shfl_xor((int)kp[h][p], x, 64);
#pragma unroll
                for (int p = 0; p < KM; ++p) insert_packed<KM>(kp[h], o[p]);
                continue;
            }
#pragma unroll
            for (int p = 0; p < KM; ++p) {
                const float od = __shfl_xor(kd[h][p], x, 64);
                const int oi = __shfl_xor(ki[h][p], x, 64);
                if (lq < x / 16 && oi >= 0 && rank_lt(od, oi, kd[h][KM - 1], ki[h][KM - 1]))
                    insert_any<KM>(kd[h], ki[h], od, oi);
            }
        }
    }
    if (lq != 0) return;
    const float lu[2] = {sb_on ? __uint_as_float(lst[lc].x) : INFINITY, sb_on ? __uint_as_float(lst[lc + 16].x) : INFINITY};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#if B16W_I8T
        const int qc = qcol_of(h);
        if (qc >= nq) continue;
#else
        if (qcol[h] >= nq) continue;
#endif
        // the screen floor: lu only ever decreased, so its last value bounds from below every row
        // this workgroup dropped by it (the rerank and the second chance fold it into their taus)
        if (sb_on && lu[h] != INFINITY)
#if B16W_I8T
            __hip_atomic_fetch_min(sbound + (size_t)qc * kSBWords + kSBFloor, ord_bits(lu[h]),
#else
            __hip_atomic_fetch_min(sbound + (size_t)qcol[h] * kSBWords + kSBFloor, ord_bits(lu[h]),
#endif
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#if B16W_I8T
        const size_t base = (size_t)qc * ncand + (size_t)split * KM;
#else
        const size_t base = (size_t)qcol[h] * ncand + (size_t)split * KM;
#endif
#pragma unroll
        for (int p = 0; p < KM; ++p) {
            if constexpr (PACK) {
                // key truncated toward -inf (a lower bound of the approximate key: the rerank
                // adds the truncation to its bounds, RerankArgs::c_trunc); split-local row ->
                // stored row
                const uint32_t u = kp[h][p];
                const int j = (int)(u & lowm);
                cand_d[base + p] = u == ~0u ? INFINITY : ord_float(u & ~lowm);
                cand_i[base + p] = u == ~0u ? (int64_t)-1
                                            : (int64_t)((split + (j >> 3) * nsplit) * kRPP + (j & 7)) + id_offset;
            } else {
                cand_d[base + p] = kd[h][p];
                cand_i[base + p] = ki[h][p] < 0 ? (int64_t)-1 : (int64_t)ki[h][p] + id_offset;
            }
        }
    }
