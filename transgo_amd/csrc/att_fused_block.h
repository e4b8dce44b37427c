// The body of the fused Self_Attention kernels, INCLUDED TWICE by net.hip (which describes it): with TG_ATT_SPLIT 1 it defines
// k_attention_x3, with TG_ATT_SPLIT 0 k_attention_h.  Textual, not a __device__ function that both kernels call: these kernels sit on
// the register limit, and a body that is optimised on its own before it is inlined into its kernel comes out with another register
// allocation (k_attention_x3: 17 spilled registers for 12, k_attention_h: 238 registers for 216; profiles/att_fused_refactor.txt).
// Everything the two precisions do differently is an `if constexpr (SPLIT)` below.
template <int S, int F, bool PRO>
#if TG_ATT_SPLIT
__global__ __launch_bounds__(256, 1) void k_attention_x3(const float* __restrict__ xin, float* __restrict__ out, _Float16* __restrict__ out2,
                                                         const _Float16* __restrict__ wimg, const float* __restrict__ qb,
                                                         const float* __restrict__ wsc_p, const float* __restrict__ gamma,
                                                         const float* __restrict__ bs, const float* __restrict__ bt,
                                                         const float* __restrict__ ps, const float* __restrict__ pt,
                                                         const float* __restrict__ s2, const float* __restrict__ t2, int rows,
                                                         unsigned* __restrict__ ovf) {
#else
__global__ __launch_bounds__(256, 1) void k_attention_h(const float* __restrict__ xin, float* __restrict__ out, _Float16* __restrict__ out2,
                                                        const _Float16* __restrict__ wimg, const float* __restrict__ qb,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ bs, const float* __restrict__ bt,
                                                        const float* __restrict__ ps, const float* __restrict__ pt,
                                                        const float* __restrict__ s2, const float* __restrict__ t2, int rows,
                                                        unsigned* __restrict__ ovf) {
#endif
    constexpr bool SPLIT = TG_ATT_SPLIT;
    // a channel group = the GC real channels of one K = 32 step; a lane's two 16-B loads of a row lie G2 bytes apart; a group's
    // v projection takes KPG K steps (SPLIT: the hi, then the lo weight fragments); a channel tile's fp16 output fills PL chunk planes
    constexpr int GC = SPLIT ? 16 : 32, G2 = SPLIT ? 16 : 64, KPG = SPLIT ? 2 : 1, PL = SPLIT ? 4 : 2;
    constexpr int P = S * S, FQ = F / 4, W = 2 * FQ + F, NT = (P + 15) / 16, CT = F / 16, NG = F / GC, NSUB = FQ / 16;
    static_assert(P <= 96 && FQ % 16 == 0 && NG % 2 == 0, "attention tile geometry");
    static_assert(SPLIT || NG * W * 64 + (W + 6 * F) * 4 + 4096 <= 65536, "attention tile geometry");   // (SPLIT asks for more than 64 KB: lds3)
    extern __shared__ __attribute__((aligned(16))) unsigned char att_smem[];
    _Float16* const wl = reinterpret_cast<_Float16*>(att_smem);                       // [NG][W][32]
    for (int i = threadIdx.x; i < NG * W * 4; i += 256) reinterpret_cast<f32x4*>(wl)[i] = reinterpret_cast<const f32x4*>(wimg)[i];
    // per-channel parameters behind the image: q|k|v bias [W], then bn scale / shift, next block's bn1 scale / shift, prologue scale /
    // shift [F each].  Read from LDS, they neither pin registers across the board loop nor queue behind the epilogue's stores (vector
    // memory loads and stores share the in-order vmcnt)
    float* const prm = reinterpret_cast<float*>(att_smem + (size_t)NG * W * 64);
    for (int i = threadIdx.x; i < W; i += 256) prm[i] = qb[i];
    for (int i = threadIdx.x; i < F; i += 256) {
        prm[W + i] = bs[i]; prm[W + F + i] = bt[i];
        prm[W + 2 * F + i] = out2 ? s2[i] : 1.f; prm[W + 3 * F + i] = out2 ? t2[i] : 0.f;
        prm[W + 4 * F + i] = PRO ? ps[i] : 1.f; prm[W + 5 * F + i] = PRO ? pt[i] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: board pointers stay in SGPRs
    const int j = lane & 15, kq = lane >> 4;
    const float lo_neg = kq >> 1 ? -1.f : -0.f;                                      // SPLIT, -1: this lane carries the lo halves of x
    const unsigned chx = (kq & 1) * 8;                                               // SPLIT: this lane's column within a group's loads (!SPLIT: kq*4)
    // this lane's 16-B chunk of weight row j: SPLIT the hi and the lo halves of its 8 channels, else its K slots kq*8 .. +7
    const int wq = SPLIT ? kq & 1 : kq;
    const int whi = j * 32 + ((wq ^ swz64(j)) << 3), wlo = j * 32 + (((2 + wq) ^ swz64(j)) << 3);
    // ds_read offsets are 16-bit: SPLIT, the image's upper half gets its own (opaque) base so that no address needs a register of
    // its own (!SPLIT: the whole image is within the offset)
    int upper = NG / 2 * W * 32;
    if constexpr (SPLIT) asm volatile("" : "+v"(upper));
    const _Float16* const wl1 = wl + upper;
    auto wgroup = [&](int g) -> const _Float16* {
        if constexpr (SPLIT) return g < NG / 2 ? wl + g * W * 32 : wl1 + (g - NG / 2) * W * 32;
        else return wl + g * W * 32;
    };
#if TG_ATT_SPLIT
    const float wsc = wsc_p[0];
#else
    constexpr float wsc = 1.f;                                                       // (no weight scale)
#endif
    const int M = rows * P;
    // Addresses: tile t of a board starts 16 rows = 16*F floats further (a scalar add on the board pointer); within the tile lane j
    // takes row j -- except in the last tile, where rows past the board clamp to its last row.  Three per-lane byte offsets serve
    // every access: {first five tiles, last tile} x the column of the projection reads, and the 4-channel column of the D tiles
    // (!SPLIT: the same column, + g*128 B, + 64 B for the reads and + ct*64 B for the D tiles)
    constexpr int LASTR = P - 1 - (NT - 1) * 16;                                     // last valid row of the last tile
    const unsigned rowA = (unsigned)j * F * 4u, rowB = (unsigned)(j <= LASTR ? j : LASTR) * F * 4u;
    const unsigned xoA = rowA + (SPLIT ? chx * 4u : kq * 16u), xoB = rowB + (SPLIT ? chx * 4u : kq * 16u), eoA = rowA + kq * 16u;
    const unsigned hoA = ((unsigned)(kq >> 1) * M + j) * 16u + (kq & 1) * 8u;        // chunk-major fp16 output, + t*256 per tile
    auto tile = [](const float* board, int t) { return board + t * 16 * F; };
    auto ld16 = [](const float* base, unsigned byte_off) { return *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + byte_off); };
    // 8 channels of one row -> this lane's fragment (SPLIT: its half of the split fragment)
    const float* l_ps = nullptr; const float* l_pt = nullptr;                          // set per board (LDS parameter block)
    struct Pro { f32x4 sc[2], sh[2]; };                                               // prologue scale / shift of this lane's 8 channels of a group
    auto pro_of = [&](int g) {
        Pro p{};
        if constexpr (PRO) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if constexpr (SPLIT) { p.sc[h] = *reinterpret_cast<const f32x4*>(l_ps + g * 16 + chx + 4 * h); p.sh[h] = *reinterpret_cast<const f32x4*>(l_pt + g * 16 + chx + 4 * h); }
                else { p.sc[h] = *reinterpret_cast<const f32x4*>(l_ps + g * 32 + h * 16 + kq * 4); p.sh[h] = *reinterpret_cast<const f32x4*>(l_pt + g * 32 + h * 16 + kq * 4); }
            }
        }
        return p;
    };
    // range guard (see conv_epilogue_h8): the largest |x| this wave converted in phase A (phase B converts the same values again) and
    // the largest value the epilogue rounds to fp16; checked once per board.  As in the conv epilogue, fmaxf drops a NaN operand: what
    // is counted is a value beyond +-65504 (inf included), the event that first produces NaNs downstream -- a NaN that arrives is not
    float amax = 0.f;
    auto frag8 = [&](const f32x4 (&src)[2], const Pro& pr, bool track = false) -> h8 {
        h8 xf;
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            f32x2 v = {src[e >> 2][e & 3], src[e >> 2][(e & 3) + 1]};
            if constexpr (PRO) {
#pragma unroll
                for (int q = 0; q < 2; ++q) { const float w = v[q] * pr.sc[e >> 2][(e & 3) + q] + pr.sh[e >> 2][(e & 3) + q]; v[q] = w > 0.f ? w : 0.f; }
            }
            if (track) amax = __builtin_fmaxf(amax, __builtin_fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])));
            h2 o = __builtin_convertvector(v, h2);                                   // !SPLIT: one rounding
            if constexpr (SPLIT) {
                const f32x2 hi = __builtin_convertvector(o, f32x2);
                // hi lanes (lo_neg = -0): half(v); lo lanes (lo_neg = -1): half(v - hi), the product is exact either way
                const f32x2 d = {__builtin_fmaf(lo_neg, hi[0], v[0]), __builtin_fmaf(lo_neg, hi[1], v[1])};
                o = __builtin_convertvector(d, h2);
            }
            xf[e] = o[0]; xf[e + 1] = o[1];
        }
        return xf;
    };
    f32x4 rawA[NT][2], rawB[NT][2];                                                  // phase A stream: one group of all six tiles each
    h8 xfA[NT], xfB[NT];
    // (the lane offsets are made opaque where they are used: hoisted out of the board loop in their 64-bit form they are spilled, and the
    // loads then take full VGPR addresses reloaded from scratch -- behind whatever the wave has in flight)
    auto issue = [&](const float* xb, int g, f32x4 (&dst)[NT][2]) {
        unsigned oa = xoA, ob = xoB;
        asm volatile("" : "+v"(oa), "+v"(ob));
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            dst[t][0] = ld16(tile(xb, t), (t + 1 < NT ? oa : ob) + g * (GC * 4));
            dst[t][1] = ld16(tile(xb, t), (t + 1 < NT ? oa : ob) + g * (GC * 4) + G2);
        }
    };
    auto frag_group = [&](const f32x4 (&src)[NT][2], int g, h8 (&xf)[NT]) {
        const Pro pr = pro_of(g);
#pragma unroll
        for (int t = 0; t < NT; ++t) xf[t] = frag8(src[t], pr, true);
    };
    int b = blockIdx.x * 4 + wave;
    if (b >= rows) return;
    { const float* xb0 = xin + (size_t)b * P * F; issue(xb0, 0, rawB); issue(xb0, 1, rawA); }
    int nboard = 0;
    for (; b < rows; b += gridDim.x * 4, ++nboard) {
        const float* xb = xin + (size_t)b * P * F;
        // opaque per board: LDS is read-only from here on, so every parameter read would otherwise be hoisted out of the board loop
        // (and pin, then spill, ~150 registers)
        unsigned popq = 0;
        asm volatile("" : "+v"(popq));                                                // (an opaque OFFSET: the pointer keeps its LDS address space)
        const float* const l_qb = prm + popq;
        const float* const l_bs = l_qb + W; const float* const l_bt = l_bs + F;
        const float* const l_s2 = l_bt + F; const float* const l_t2 = l_s2 + F; l_ps = l_t2 + F; l_pt = l_ps + F;
        TG_ASTAMP(0);
        // ---- phase A: q^T and k^T, [c][pos] tiles (!SPLIT: the f32 bias in the accumulator) ----
        f32x4 qk[2 * NSUB][NT];
#pragma unroll
        for (int ct = 0; ct < 2 * NSUB; ++ct) {
            f32x4 q0 = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (!SPLIT) q0 = *reinterpret_cast<const f32x4*>(l_qb + ct * 16 + kq * 4);
#pragma unroll
            for (int t = 0; t < NT; ++t) qk[ct][t] = q0;
        }
        auto mfma_qk = [&](int g, const h8 (&xf)[NT]) {
#pragma unroll
            for (int ct = 0; ct < 2 * NSUB; ++ct) {
                const _Float16* wr = wgroup(g) + ct * 16 * 32;
                const h8 ah = *reinterpret_cast<const h8*>(wr + whi);
                h8 al = ah;
                if constexpr (SPLIT) al = *reinterpret_cast<const h8*>(wr + wlo);       // (both requested before the first MFMA)
#pragma unroll
                for (int t = 0; t < NT; ++t) qk[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, xf[t], qk[ct][t], 0, 0, 0);
                if constexpr (SPLIT) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) qk[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, xf[t], qk[ct][t], 0, 0, 0);
                }
            }
        };
        constexpr int NMA = 2 * NSUB * NT * KPG, KVA = SPLIT ? 3 : 4;                  // MFMAs of a group, VALU instructions behind each
        frag_group(rawB, 0, xfA);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < NG; g += 2) {
            if (g + 2 < NG) issue(xb, g + 2, rawB);
            mfma_qk(g, xfA);
            frag_group(rawA, g + 1, xfB);
            TG_ATT_SCHED(NMA, KVA);
            if (g + 3 < NG) issue(xb, g + 3, rawA);
            mfma_qk(g + 1, xfB);
            if (g + 2 < NG) frag_group(rawB, g + 2, xfA);
            TG_ATT_SCHED(NMA, KVA);
            if (g == 0) TG_ASTAMP(29);
        }
        TG_ASTAMP(1);
        // ---- phase B, block tm = rows i in [16 tm, 16 tm + 16) ----
        f32x4 rv[NG][2];                                                             // the block's x rows, all groups
        auto issue_rows = [&](int tm) {
            unsigned o = tm + 1 < NT ? xoA : xoB;
            asm volatile("" : "+v"(o));
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                rv[g][0] = ld16(tile(xb, tm), o + g * (GC * 4));
                rv[g][1] = ld16(tile(xb, tm), o + g * (GC * 4) + G2);
            }
        };
        issue_rows(0);
        if constexpr (SPLIT) {
#pragma unroll
            for (int ct = 0; ct < 2 * NSUB; ++ct) {
                const f32x4 bq = *reinterpret_cast<const f32x4*>(l_qb + ct * 16 + kq * 4);
#pragma unroll
                for (int t = 0; t < NT; ++t) qk[ct][t] = qk[ct][t] * wsc + bq;
            }
        }
        // The residual x (PRO: relu(x*ps + pt)) is ADDED INTO the output accumulators, column tile tn in row block tm = tn, and v
        // carries the factor gamma, so that they end as gamma * out + x and the epilogue has no loads at all: a load queued behind
        // the epilogue's stores would wait for their acknowledgements (vmcnt is in order), and did -- 30 % of a board's time in the
        // first version.  Taken in block tn, the residual rows are the lines that block's own row loads have just brought in (read
        // up front for all tiles they were a third trip to HBM: 2.17 GB of reads per launch against 0.67 GB of x).
        const float gam = gamma[0];
        f32x4 acc[CT][NT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int tn = 0; tn < NT; ++tn) acc[ct][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
        // next board's rows towards L2 now (one dword per 128-B line, results unused): phase A is the first touch of a board's x and
        // its loads run only one group ahead of their use -- from HBM that was 17 % of a board's time
        const int bnx = b + gridDim.x * 4;
        const float* const xnext = xin + (size_t)(bnx < rows ? bnx : b) * P * F;
        // as LDS-DMA into a scratch KB of this wave: no destination registers, nothing ever waits for them
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const unsigned lo = (unsigned)(lane + 64 * i) * 128u, off = lo < (unsigned)(P * F * 4 - 16) ? lo : (unsigned)(P * F * 4 - 16);
            tg_dma_global(xnext, (int)off, (tg_lds_void*)(&att_smem[(size_t)NG * W * 64 + (W + 6 * F) * 4 + wave * 1024]));
        }
        __builtin_amdgcn_sched_barrier(0);
        TG_ASTAMP(27);
#pragma unroll
        for (int tm = 0; tm < NT; ++tm) {
            // v for the block: D[pos][c], all channel tiles (!SPLIT: the bias in the accumulator)
            f32x4 va[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                float bv = 0.f;
                if constexpr (!SPLIT) bv = l_qb[2 * FQ + ct * 16 + j];
                va[ct] = f32x4{bv, bv, bv, bv};
            }
            // weight fragments: eight in flight, each slot refilled (for the next K step) right behind the MFMA that used it; the
            // fences and group barriers keep that distance (left alone, the scheduler sinks every read next to its MFMA and the wave
            // sits on LDS latency 128 times per block)
            h8 wf[CT];
            auto wslot = [&](int ks, int ct) {                                       // K step ks = KPG*g (+ 1, SPLIT: the lo fragment)
                return *reinterpret_cast<const h8*>(wgroup(ks / KPG) + (2 * FQ + ct * 16) * 32 + (ks % KPG ? wlo : whi));
            };
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) wf[ct] = wslot(0, ct);
            h8 xf = frag8(rv[0], pro_of(0)), xfn = xf;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < KPG * NG; ++ks) {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    va[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf, wf[ct], va[ct], 0, 0, 0);
                    if (ks + 1 < KPG * NG) wf[ct] = wslot(ks + 1, ct);
                }
                if (ks % KPG == 0 && ks / KPG + 1 < NG) xfn = frag8(rv[ks / KPG + 1], pro_of(ks / KPG + 1));   // next group's fragment, in the MFMA shadow
#pragma unroll
                for (int i_ = 0; i_ < CT; ++i_) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (ks % KPG == KPG - 1) xf = xfn;
            }
            TG_ASTAMP(2 + 4 * tm);
            if constexpr (SPLIT) __builtin_amdgcn_sched_barrier(0);
            // the residual rows of column tile tm, D layout (row = channel ct*16 + kq*4 + r, column = position tm*16 + j), from the
            // block's ROW registers.  !SPLIT: D tile ct = 2g + h is this lane's own rv[g][h].  SPLIT: they hold exactly these values
            // in the projection layout -- lane (j, kq') has channels g*16 + (kq' & 1)*8 .. +7 of row j, the lane pairs kq' and kq' + 2
            // hold the same eight -- so lanes kq' < 2 offer their first four, lanes kq' >= 2 their last four, and destination
            // (j, kq) pulls from (j, (kq >> 1) + 2*(kq & 1)): one ds_bpermute per register, no memory access at all.  (Round 3
            // read them from memory again: meant to be cache hits on the lines the row loads had just fetched, they were the third
            // trip to HBM -- the XCD's L2 turns over within a row block, profiles/r3_pmc_attention_x3.json: 2.19 GB fetched.)
            f32x4 xa[CT];
            if constexpr (SPLIT) {
                const int src = ((((kq >> 1) + 2 * (kq & 1)) << 4) + j) << 2;          // byte address of the source lane
                const bool hi_half = kq >= 2;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    // (scalar copies: a bit_cast of a vector ELEMENT sends the whole vector through scratch)
                    const float s0 = hi_half ? rv[ct][1][0] : rv[ct][0][0], s1 = hi_half ? rv[ct][1][1] : rv[ct][0][1];
                    const float s2 = hi_half ? rv[ct][1][2] : rv[ct][0][2], s3 = hi_half ? rv[ct][1][3] : rv[ct][0][3];
                    xa[ct] = f32x4{__int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(s0))), __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(s1))),
                                   __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(s2))), __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(s3)))};
                }
            } else {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) xa[ct] = rv[ct >> 1][ct & 1];
            }
            // !SPLIT: added now, before the next block's rows overwrite the registers; SPLIT (whose xa are copies): behind the output GEMM
            if constexpr (!SPLIT) {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    f32x4 xv = xa[ct];
                    if constexpr (PRO) {
                        const f32x4 vps = *reinterpret_cast<const f32x4*>(l_ps + ct * 16 + kq * 4), vpt = *reinterpret_cast<const f32x4*>(l_pt + ct * 16 + kq * 4);
#pragma unroll
                        for (int q = 0; q < 4; ++q) { const float w = xv[q] * vps[q] + vpt[q]; xv[q] = w > 0.f ? w : 0.f; }
                    }
                    acc[ct][tm] = acc[ct][tm] + xv;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (tm + 1 < NT) issue_rows(tm + 1);                                      // lands during the block's energy / output GEMMs
            __builtin_amdgcn_sched_barrier(0);                                       // (kept here: sunk to the block's end they are waited for at once)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                if constexpr (SPLIT) va[ct] = va[ct] * wsc + l_qb[2 * FQ + ct * 16 + j];
                va[ct] = va[ct] * gam;
            }
            // energies of the block (exact f32): e[tn] = q[tm] . k[tn]
            f32x4 e[NT];
#pragma unroll
            for (int tn = 0; tn < NT; ++tn) e[tn] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                    for (int tn = 0; tn < NT; ++tn)
                        e[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(qk[sub][tm][s4], qk[NSUB + sub][tn][s4], e[tn], 0, 0, 0);
            TG_ASTAMP(3 + 4 * tm);
            // softmax over j (columns) for the rows i = tm*16 + kq*4 + r
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float mx = -INFINITY;
#pragma unroll
                for (int tn = 0; tn < NT; ++tn) if (tn * 16 + j < P) mx = e[tn][r] > mx ? e[tn][r] : mx;
#pragma unroll
                for (int o = 0; o < 4; ++o) { const float t = row16_step(mx, o); mx = t > mx ? t : mx; }
                float sum = 0.f;
#pragma unroll
                for (int tn = 0; tn < NT; ++tn) {
                    const float v = tn * 16 + j < P ? __expf(e[tn][r] - mx) : 0.f;        // v_exp_f32: ~1e-7 relative, tolerance is 1e-3
                    e[tn][r] = v; sum += v;
                }
#pragma unroll
                for (int o = 0; o < 4; ++o) sum += row16_step(sum, o);
                const float inv = (tm * 16 + kq * 4 + r < P) ? 1.f / sum : 0.f;     // rows past the board contribute nothing below
#pragma unroll
                for (int tn = 0; tn < NT; ++tn) e[tn][r] *= inv;
            }
            TG_ASTAMP(4 + 4 * tm);
            // out[c][j] += v[i][c] attention[i][j]: k-step r covers rows i = tm*16 + kq*4 + r; of the last block only the steps that
            // touch a row < P exist
            constexpr int LASTS = P - (NT - 1) * 16, NS_LAST = LASTS < 4 ? LASTS : 4;
            const int ns = tm + 1 < NT ? 4 : NS_LAST;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (r >= ns) continue;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int tn = 0; tn < NT; ++tn)
                        acc[ct][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[ct][r], e[tn][r], acc[ct][tn], 0, 0, 0);
            }
            if constexpr (SPLIT) {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    f32x4 xv = xa[ct];
                    if constexpr (PRO) {
                        const f32x4 vps = *reinterpret_cast<const f32x4*>(l_ps + ct * 16 + kq * 4), vpt = *reinterpret_cast<const f32x4*>(l_pt + ct * 16 + kq * 4);
#pragma unroll
                        for (int q = 0; q < 4; ++q) { const float w = xv[q] * vps[q] + vpt[q]; xv[q] = w > 0.f ? w : 0.f; }
                    }
                    acc[ct][tm] = acc[ct][tm] + xv;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            TG_ASTAMP(5 + 4 * tm);
        }
        // ---- epilogue.  D tile: row = channel ct*16 + kq*4 + r, column = position tn*16 + j ----
        // every address = a per-board scalar base + one of six per-lane byte offsets + a compile-time constant.  Loads are kept
        // AHEAD of the stores in issue order (a load queued behind stores waits for their acknowledgements): the next board's first
        // two groups go out before the first store, and the residual is already inside the accumulators.
        {
            issue(xnext, 0, rawB); issue(xnext, 1, rawA);                             // unconditional (last board: its own rows again)
        }
        char* const yb = reinterpret_cast<char*>(out + (size_t)b * P * F);
        // opaque per board: hoisted out of the board loop, the 64-bit forms of these offsets would be spilled -- and a spill reload in
        // here queues behind the stores
        unsigned eoE = eoA, hoE = hoA;
        asm volatile("" : "+v"(eoE), "+v"(hoE));
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int c = ct * 16 + kq * 4;
            const f32x4 vbs = *reinterpret_cast<const f32x4*>(l_bs + c), vbt = *reinterpret_cast<const f32x4*>(l_bt + c);
            const f32x4 vs2 = *reinterpret_cast<const f32x4*>(l_s2 + c), vt2 = *reinterpret_cast<const f32x4*>(l_t2 + c);
            // fp16 output, chunk-major: the channel tile starts at chunk plane ct*PL, this lane's four channels lie in plane + (kq >> 1),
            // half (kq & 1)*4 of row m.  SPLIT: element (m, x2_index(c)), the lo plane 2 further; !SPLIT: element (m, c), h16_index
            const size_t hplane = ((size_t)ct * PL * M + (size_t)b * P) * 16;
            char* hb = nullptr; char* lb = nullptr;                                  // SPLIT: the hi and lo plane pointers, formed up here
            if constexpr (SPLIT) { hb = reinterpret_cast<char*>(out2) + hplane; lb = hb + (size_t)2 * M * 16; }
#pragma unroll
            for (int tn = 0; tn < NT; ++tn) {
                if (tn * 16 + j >= P) continue;
                f32x4 y, u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float w = acc[ct][tn][q] * vbs[q] + vbt[q];
                    y[q] = w > 0.f ? w : 0.f;
                    const float z = y[q] * vs2[q] + vt2[q];
                    u[q] = z > 0.f ? z : 0.f;
                }
                *reinterpret_cast<f32x4*>(yb + tn * 16 * F * 4 + (eoE + ct * 64)) = y;
                if (out2) {
                    h4 hi, lo;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        hi[q] = (_Float16)u[q];
                        if constexpr (SPLIT) lo[q] = (_Float16)(u[q] - (float)hi[q]);
                        amax = __builtin_fmaxf(amax, u[q]);
                    }
                    if constexpr (SPLIT) {
                        *reinterpret_cast<h4*>(hb + (hoE + tn * 256)) = hi;
                        *reinterpret_cast<h4*>(lb + (hoE + tn * 256)) = lo;
                    } else {
                        *reinterpret_cast<h4*>(reinterpret_cast<char*>(out2) + hplane + (hoE + tn * 256)) = hi;
                    }
                }
            }
            if (ct == 3) TG_ASTAMP(28);
        }
        TG_ASTAMP(26);
        if (__builtin_amdgcn_ballot_w64(!(amax <= 65504.f)) != 0) { if (lane == 0) atomicAdd(ovf, 1u); amax = 0.f; }
    }
    TG_VMCNT(0);                                                                     // the last board's touches and stores
}
