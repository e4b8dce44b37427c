// net.hip -- policy/value/ownership network forward for gfx950 (replaces TransGoNetwork.main_prediction,
// model.py:17-20 -> MainNetwork.forward, model.py:79-114, built from CNNBlock model.py:317-324 and the pre-activation
// ResidualBlock model.py:238-248; inference only, BatchNorm in eval mode).
//
// Tower: stem conv3x3(C->F)+BN+ReLU, N x [BN,ReLU,conv3x3,BN,ReLU,conv3x3,+x], BN+ReLU, then the two heads of
// model.py:65-76 / :97-111 (value/ownership: conv3x3(F->2)+BN+ReLU, FC(2P->64)+ReLU, FC(64->1) tanh, FC(64->P) tanh;
// policy: conv3x3(F->4)+BN+ReLU, FC(4P->P+1), softmax).
//
// The 3x3 convolutions are the one dense contraction of the whole engine and run on the matrix cores as an implicit
// GEMM in exact fp32 (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain, so results stay within 1e-3 of torch fp32):
//   D[cout][position] += W[tap][cout][cin] * X[position + tap][cin]
// Activations are position-major / channel-minor (NHWC flattened over the batch: row m = leaf*P + point), so a tile of
// 128 consecutive rows plus a halo of S+1 rows on each side contains every 3x3 neighbour of its rows regardless of
// where leaf boundaries fall; taps that leave the board are zeroed in registers from a 9-bit per-row mask instead
// of materialising padded boards.  BatchNorm is folded on the host (transgo_amd/model.py): BN that follows a conv goes
// into its weights/bias, BN that precedes one (pre-activation) is applied with ReLU while the tile is staged into LDS.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "conv_rows.h"
#include "engine.h"

using namespace tg;

namespace tg {

struct ConvW { const float* w; const float* b; };
struct BlockW { const float* s1; const float* t1; ConvW c1; ConvW c2; const float* g1; const float* g2;
                const _Float16* h1; const _Float16* h2; };   // g1/g2: stage-ordered f32, h1/h2: stage-ordered fp16 copies of c1.w / c2.w
struct AttW { ConvW qkv; const float* gamma; const float* s; const float* t;          // Self_Attention, model.py:288-315
              const _Float16* x3w = nullptr; const float* x3sc = nullptr; };          // q|k|v weights as the LDS image of k_attention_x3 (split, + 2^-s) / k_attention_h (fp16)
struct Layer { int kind; int ridx; AttW a; };                                         // kind 0: residual block blocks[ridx]; 1: attention

// Which forward runs, decided once at load (net_path) and read by the buffer allocation, the weight restaging and forward_t.
//   CHAIN_F32   general f32 chain: k_conv3x3 everywhere (F = 32 / 64, TG_DMA_CONV=0, and the DMA
//               chain's batches of 2 GiB or more per activation buffer)
//   CHAIN_DMA   f32 tower of 128 / 256 filters on the DMA-fed k_conv3x3_sg.  Between two conv layers (stem or residual block ->
//               residual block) the residual stream is ONE f32 tensor, slice-major in the conv's row order (conv_rows.h): the producer
//               writes nothing else, the block's first conv applies relu(bn1(.)) to its B fragments as they land, its second conv
//               starts its accumulators from the stream.  Towards an attention layer or the head the stream is row-major, and an
//               attention layer also writes relu(bn1_next(.)) slice-major (bufAct) for a residual block that follows it.
//               No launch of this chain uses the second output (`out2`) of k_conv3x3 / k_conv3x3_sg any more: it served the
//               two-tensor chain this replaced and stays in the kernels only until its removal is measured
//   CHAIN_F16   fp16 storage, f32 accumulate (k_conv3x3_h2; stem and head conv too); the residual stream stays f32 unless r16
//   CHAIN_SPLIT split precision ("f32x3"): every conv operand as fp16 hi + lo, three of the four products on the fp16 MFMA; the
//               residual stream, the dense heads and (beyond the fused k_attention_x3) attention stay f32
enum Chain { CHAIN_F32 = 0, CHAIN_DMA, CHAIN_F16, CHAIN_SPLIT };
struct NetPath {
    Chain chain = CHAIN_F32;
    bool r16 = false;          // CHAIN_F16: fp16 residual stream too (net_precision 2)
    bool att_x3 = false;       // CHAIN_SPLIT: attention blocks on the fused k_attention_x3 (9x9, F = 128)
    bool att_h = false;        // CHAIN_F16, f32 residual stream: attention blocks on the fused k_attention_h (9x9, F = 128)
    bool head_x2 = false;      // CHAIN_SPLIT: the head conv on k_head_gemm_x2 (F = 128, the trunk ends in a residual block)
    size_t att_lds = 0;        // k_attention's dynamic LDS in bytes; 0: no attention, or its image does not fit
};

struct Net {
    int F = 0, NB = 0, C = 0, S = 0, P = 0, A = 0;
    float* blob = nullptr; size_t blob_floats = 0;
    float* wstage = nullptr; // [2*NB][F/16*9][F][16] stage-ordered F->F conv weights (k_conv3x3_sg)
    ConvW stem; std::vector<BlockW> blocks; std::vector<Layer> layers; const float* s_end = nullptr; const float* t_end = nullptr;
    bool pol_att = false; AttW patt; ConvW head_a; std::string arch;
    float* bufQ = nullptr; float* hca = nullptr;   // q|k|v projections [rows][P][1.5F]; policy head conv output
    float* bufAct = nullptr;                       // DMA chain with an attention layer in front of a residual block ("AR"): relu(bn1(.)) from that layer for the block's first conv
    int prec = 0;                                  // cfg.net_precision: 0 = f32, 1 = fp16 storage + f32 accumulate (k_conv3x3_h2), 2 = 1 + fp16 residual stream,
                                                   // 3 = split precision ("f32x3"): every operand as fp16 hi + lo, three of the four products on the fp16 MFMA, f32 accumulate
    const float* head_g = nullptr; const float* head_ag = nullptr;   // [64][F] head conv weights for k_head_gemm (tap*6 + cout rows)
    const _Float16* head_x2 = nullptr; const float* head_x2sc = nullptr;   // prec 3, F = 128: the value/policy head conv's split weights (k_head_gemm_x2) + 2^-s
    float* wsc = nullptr;                          // prec 3: [2*NB + 1] power-of-two factor 2^-s each conv's weights were scaled by before splitting (stem last)
    _Float16* stem_h = nullptr; _Float16* head_h = nullptr; _Float16* x0h = nullptr;   // fp16 path: stem [2*9][F][32] (16 planes padded to 64), head [F/32*9][16][32], input [rows][P][64]
    _Float16* wh = nullptr; _Float16* act16 = nullptr; _Float16* h16 = nullptr;   // fp16 path: weights [2*NB][F/32*9][F][32], activations [rows][P][F]
    NetPath path;
    ConvW head; const float* w_vo = nullptr; const float* b_vo = nullptr; const float* w_v = nullptr; const float* b_v = nullptr;
    const float* w_o = nullptr; const float* b_o = nullptr; const float* w_a = nullptr; const float* b_a = nullptr;
    // engine batches arrive bit-packed and sparse (engine.h: obs_bits through row_slot); tg_net_predict hands float planes
    const uint32_t* in_bits = nullptr; const int32_t* in_slot = nullptr; int in_words = 0;
    float* x0 = nullptr;   // [rows][P][16] input planes, channel-minor
    float* bufA = nullptr; float* bufB = nullptr; float* bufH = nullptr;   // [rows][P][F]
    float* hc = nullptr;   // [rows][P][16] head conv output
    float* own = nullptr;  // [rows][P]
    int rows_cap = 0;
    // range guard: [0] sticky count of epilogue tiles (conv) / boards (attention) that rounded a value beyond +-65504 to fp16 since
    // the network was created (fp16-carrying precisions only); [1 + k] bit pattern of max |w| over weight set k's BN-folded blob
    unsigned* range = nullptr;
    // Two complete weight sets (f2, "double-buffered so search never stalls"): the forward pass reads set `active` (the pointer
    // fields above are bound to it); a refresh fills the other one -- tg_net_load_async on a side stream while searches keep
    // running -- and the next forward that finds it complete rebinds.  `swapped` orders a later refill of the retired set behind
    // every kernel that may still read it.
    struct WeightSet { float* blob = nullptr; float* wstage = nullptr; _Float16* wh = nullptr; _Float16* stem_h = nullptr; _Float16* head_h = nullptr;
                       float* wsc = nullptr; float* head_g = nullptr; float* head_ag = nullptr;
                       _Float16* att_h = nullptr; float* att_sc = nullptr;
                       _Float16* head_x2 = nullptr; float* head_x2sc = nullptr; };                          // att_h / att_sc: per attention layer, k_attention_x3's split weight image + scale, or k_attention_h's fp16 image (no scale)   // head_g / head_ag: k_head_gemm copies of head / head_a
    WeightSet sets[2]; int active = 0; bool pending = false;
    hipStream_t side = nullptr; hipEvent_t loaded = nullptr, swapped = nullptr; float* pinned = nullptr;
    // profiling of the dominant kernel (3x3 conv F->F) with HIP events on the launch stream
    bool prof = false; std::vector<hipEvent_t> ev; size_t ev_used = 0; double conv_ms = 0; long conv_launches = 0; double conv_flops = 0;
    long conv_skipped = 0;                         // launches that found the event pool full (drain it with tg_prof_read between steps)
};

}  // namespace tg

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using h2 = __attribute__((ext_vector_type(2))) _Float16;
using h8 = __attribute__((ext_vector_type(8))) _Float16;
using h4 = __attribute__((ext_vector_type(4))) _Float16;
__device__ __forceinline__ int tid0() { return (int)threadIdx.x; }



template <int S>
__global__ __launch_bounds__(256) void k_obs_to_rows(const float* __restrict__ obs, float* __restrict__ x0, int rows, int C) {
    constexpr int P = S * S;
    const size_t total = (size_t)rows * P * 16;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i & 15);
        const size_t m = i >> 4;
        const int p = (int)(m % P);
        const size_t r = m / P;
        x0[i] = c < C ? obs[(r * C + c) * P + p] : 0.f;
    }
}


// The same from the engine's evaluation batch: row r = entry row_slot[r] of the bit-packed batch (bit c*P + p of its W words).
template <int S>
__global__ __launch_bounds__(256) void k_bits_to_rows(const uint32_t* __restrict__ bits, const int32_t* __restrict__ row_slot,
                                                      float* __restrict__ x0, int rows, int C, int W) {
    constexpr int P = S * S;
    const size_t total = (size_t)rows * P * 16;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i & 15);
        const size_t m = i >> 4;
        const int p = (int)(m % P), k = c * P + p;
        const size_t r = m / P;
        x0[i] = c < C ? (float)((bits[(size_t)row_slot[r] * W + (k >> 5)] >> (k & 31)) & 1u) : 0.f;
    }
}

// Conv epilogue shared by the conv kernels.  acc[ct][t] holds couts ct*16 + kq*4 .. +3 of row mrow[t].
// Loads and stores retire through ONE in-order counter (vmcnt), so a load issued after stores waits for all of them: per-cout
// parameters therefore come from LDS (par = bias | s2 | t2, COUT floats each), and the residual is fetched one 4-tile chunk
// ahead of the stores of the previous chunk, which turns ~CT*NPT serialized memory round trips into counted, overlapped ones.
// EPI 0: relu(acc + bias)   EPI 1: acc + bias + res   EPI 2: acc + bias;   out2 (optional) = relu(v * s2 + t2).
// SM / SM2: `out` / `out2` is a SLICE-MAJOR f32 tensor [COUT/16][Msm][16] (f32_sm_index) -- the layout the DMA-fed kernel reads its
// inputs in, with BOARD-GROUPED rows (conv_rows.h): srow[t] = conv_sg_row(board, position) of natural row mrow[t], Msm =
// conv_sg_rows(boards) the padded row count.  A B fragment of k_conv3x3_sg (one position, 16 boards, 64 B of one slice) is then one
// contiguous KB.  The rows of the absent boards of the last group of 16 are never written (stale or uninitialised, NaN included):
// they only ever feed MFMA columns of those same absent boards, which are never stored.
__device__ __forceinline__ size_t f32_sm_index(int srow, int c, int Msm) { return ((size_t)(c >> 4) * Msm + srow) * 16 + (c & 15); }
// relu(bn(v)) of a pre-activation residual block's input: the ONE expression behind `out2` and behind k_conv3x3_sg's activation on
// load, so both give the same bits
__device__ __forceinline__ float bn_relu(float v, float s, float t) { const float w = v * s + t; return w > 0.f ? w : 0.f; }
// bn_relu beside MFMAs: the same two roundings (this library is built without contraction), spelled as single v_mul_f32 / v_add_f32
// because the compiler SLP-packs neighbouring elements into v_pk_mul_f32 / v_pk_add_f32, which cost the MFMA pipe issue cycles
// (MI355X_MICROARCH.md, constants table: packed f32 VALU beside MFMAs)
__device__ __forceinline__ float bn_relu_unpacked(float v, float s, float t) {
    float w;
    asm("v_mul_f32 %0, %1, %2" : "=v"(w) : "v"(v), "v"(s));
    asm("v_add_f32 %0, %1, %2" : "=v"(w) : "v"(w), "v"(t));
    return w > 0.f ? w : 0.f;
}

template <int COUT, int CT, int NPT, int EPI, bool SM = false, bool SM2 = false>
__device__ __forceinline__ void conv_epilogue(f32x4 (&acc)[CT][NPT], const int (&mrow)[NPT], int M, int co_base, int kq,
                                              float* __restrict__ out, const float* __restrict__ res, float* __restrict__ out2,
                                              const float* par, const int (&srow)[NPT], int Msm) {
    constexpr int CH = CT % 4 == 0 ? 4 : CT % 3 == 0 ? 3 : CT % 2 == 0 ? 2 : 1;   // cout tiles per chunk
    constexpr int NCH = (CT / CH) * NPT;
    static_assert(CT % CH == 0, "chunking");
    f32x4 r[2][CH];
    auto load_res = [&](int c, f32x4* dst) {
        const int t = c / (CT / CH), h = c % (CT / CH);
        if (mrow[t] < M) {
#pragma unroll
            for (int i = 0; i < CH; ++i)
                dst[i] = *reinterpret_cast<const f32x4*>(res + (size_t)mrow[t] * COUT + co_base + (h * CH + i) * 16 + kq * 4);
        }
    };
    if (EPI == 1) load_res(0, r[0]);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int t = c / (CT / CH), h = c % (CT / CH);
        if (EPI == 1 && c + 1 < NCH) load_res(c + 1, r[(c + 1) & 1]);
        if (mrow[t] < M) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int ct = h * CH + i;
                const int col = ct * 16 + kq * 4;      // column within this kernel's cout range
                f32x4 v = acc[ct][t] + *reinterpret_cast<const f32x4*>(par + col);
                if (EPI == 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
                } else if (EPI == 1) {
                    v = v + r[c & 1][i];
                }
                *reinterpret_cast<f32x4*>(out + (SM ? f32_sm_index(srow[t], co_base + col, Msm) : (size_t)mrow[t] * COUT + co_base + col)) = v;
                if (out2) {
                    const f32x4 sc = *reinterpret_cast<const f32x4*>(par + COUT + col);
                    const f32x4 sh = *reinterpret_cast<const f32x4*>(par + 2 * COUT + col);
                    f32x4 u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) u[e] = bn_relu(v[e], sc[e], sh[e]);
                    *reinterpret_cast<f32x4*>(out2 + (SM2 ? f32_sm_index(srow[t], co_base + col, Msm) : (size_t)mrow[t] * COUT + co_base + col)) = u;
                }
            }
        }
    }
}

// EPI 0: out = relu(acc + bias)      EPI 1: out = acc + bias + res      EPI 2: out = acc + bias
// NTAP 9: 3x3 convolution with zero padding; NTAP 1: 1x1 convolution (the q/k/v projections of Self_Attention, model.py:294-296)
// SM2 / SM1: `out2` / `out` slice-major in the conv's row order (the DMA chain's stem; see conv_epilogue)
template <int S, int CIN, int COUT, bool PRO, int EPI, int NTAP = 9, int NPT = 2, bool SM2 = false, bool SM1 = false>
// NPT = 3 only pays with two waves per SIMD (<= 256 registers, a handful of spills): measured 132 vs 118 TFLOP/s at one
__global__ __launch_bounds__(256, (NPT > 2 ? 2 : 1)) void k_conv3x3(const float* __restrict__ in, float* __restrict__ out,
                                                 const float* __restrict__ res, const float* __restrict__ Wt,
                                                 const float* __restrict__ bias, const float* __restrict__ ps,
                                                 const float* __restrict__ pt, int M, float* __restrict__ out2 = nullptr,
                                                 const float* __restrict__ s2 = nullptr, const float* __restrict__ t2 = nullptr) {
    constexpr int P = S * S, HALO = NTAP == 9 ? S + 1 : 0;
    constexpr int TM = 64 * NPT;                    // output rows per workgroup: 4 waves x NPT position tiles x 16
    constexpr int CC = CIN < 32 ? CIN : 32;         // input channels staged per pass
    constexpr int RS = CC + 4;                      // LDS row stride (floats)
    constexpr int NROW = TM + 2 * HALO;
    constexpr int CT = COUT / 16;                   // cout tiles, all held by every wave
    constexpr int C4 = CC / 4;
    __shared__ float xs[NROW * RS];
    __shared__ __attribute__((aligned(16))) float par[3 * COUT];            // bias | s2 | t2 for the epilogue
    for (int i = tid0(); i < COUT; i += 256) { par[i] = bias[i]; par[COUT + i] = out2 ? s2[i] : 0.f; par[2 * COUT + i] = out2 ? t2[i] : 0.f; }
    // WALL: a narrow output (the 16-wide head conv) is latency-bound, not MFMA-bound -- stage all NTAP weight tiles of a channel
    // slice at once (2 barriers per slice instead of 2 per tap; 480 -> ~ us per forward at 16384 leaves)
    constexpr bool WALL = COUT <= 16 && NTAP == 9;
    constexpr int WT = WALL ? NTAP : 1;             // weight tiles resident in LDS
    __shared__ float ws[WT * COUT * RS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 15, kq = lane >> 4;
    const int m0 = blockIdx.x * TM;

    unsigned vmask[NPT];
#pragma unroll
    for (int t = 0; t < NPT; ++t) {
        const int m = m0 + (wave * NPT + t) * 16 + j;
        unsigned mk = 0;
        if (m < M) {
            const int p = m % P, x = p % S, y = p / S;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                if (yy >= 0 && yy < S && xx >= 0 && xx < S) mk |= 1u << tap;
            }
            if (NTAP == 1) mk = 1u;
        }
        vmask[t] = mk;
    }
    f32x4 acc[CT][NPT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int t = 0; t < NPT; ++t) acc[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Software pipeline: the global loads of stage s+1 (one tap's weights; every 9th stage also the next 32-channel
    // slice of the activation tile) are issued before the MFMA block of stage s and land in registers while it runs;
    // they are written to LDS after the barrier that ends it.
    constexpr int WL = (WT * COUT * C4 + 255) / 256;
    constexpr int XL = (NROW * C4 + 255) / 256;
    f32x4 wreg[WL], xreg[XL];
    auto load_w = [&](int cc, int tap) {
#pragma unroll
        for (int i = 0; i < WL; ++i) {
            const int idx = tid + i * 256;
            if (idx < WT * COUT * C4) {                                   // WALL: idx also runs over the taps (tap argument = 0)
                const int co = idx / C4, c4 = idx % C4;
                wreg[i] = *reinterpret_cast<const f32x4*>(Wt + ((size_t)tap * COUT + co) * CIN + cc + c4 * 4);
            }
        }
    };
    auto store_w = [&]() {
#pragma unroll
        for (int i = 0; i < WL; ++i) {
            const int idx = tid + i * 256;
            if (idx < WT * COUT * C4) { const int co = idx / C4, c4 = idx % C4; *reinterpret_cast<f32x4*>(&ws[co * RS + c4 * 4]) = wreg[i]; }
        }
    };
    auto load_x = [&](int cc) {
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int idx = tid + i * 256;
            xreg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (idx < NROW * C4) {
                const int r = idx / C4, c4 = idx % C4;
                const int m = m0 - HALO + r;
                if (m >= 0 && m < M) xreg[i] = *reinterpret_cast<const f32x4*>(in + (size_t)m * CIN + cc + c4 * 4);
            }
        }
    };
    auto store_x = [&](int cc) {
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int idx = tid + i * 256;
            if (idx < NROW * C4) {
                const int r = idx / C4, c4 = idx % C4;
                f32x4 v = xreg[i];
                if (PRO) {
                    const int m = m0 - HALO + r;
                    if (m >= 0 && m < M) {             // the zero rows outside the batch stay zero (padding is post-activation)
                        const f32x4 sc = *reinterpret_cast<const f32x4*>(ps + cc + c4 * 4);
                        const f32x4 sh = *reinterpret_cast<const f32x4*>(pt + cc + c4 * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { float u = v[e] * sc[e] + sh[e]; v[e] = u > 0.f ? u : 0.f; }
                    }
                }
                *reinterpret_cast<f32x4*>(&xs[r * RS + c4 * 4]) = v;
            }
        }
    };
    load_x(0);
    load_w(0, 0);
    for (int cc = 0; cc < CIN; cc += CC) {
        for (int tap = 0; tap < NTAP; ++tap) {
            if (!WALL || tap == 0) {
                __syncthreads();
                if (tap == 0) store_x(cc);
                store_w();
                __syncthreads();
                if (!WALL && tap < NTAP - 1) load_w(cc, tap + 1);
                else if (cc + CC < CIN) { load_w(cc + CC, 0); load_x(cc + CC); }
            }
            const int toff = NTAP == 9 ? (tap / 3 - 1) * S + (tap % 3 - 1) : 0;
#pragma unroll
            for (int sub = 0; sub < CC / 16; ++sub) {
                f32x4 b[NPT];
#pragma unroll
                for (int t = 0; t < NPT; ++t) {
                    const int r = (wave * NPT + t) * 16 + j + HALO + toff;
                    b[t] = *reinterpret_cast<const f32x4*>(&xs[r * RS + sub * 16 + kq * 4]);
                    if (!((vmask[t] >> tap) & 1)) b[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(&ws[((WALL ? tap * COUT : 0) + ct * 16 + j) * RS + sub * 16 + kq * 4]);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int t = 0; t < NPT; ++t)
                            acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[t][s], acc[ct][t], 0, 0, 0);
                }
            }
        }
    }
    // D tile: row (lane>>4)*4 + r = cout, column lane&15 = position
    int mrow[NPT], srow[NPT];
#pragma unroll
    for (int t = 0; t < NPT; ++t) {
        mrow[t] = m0 + (wave * NPT + t) * 16 + j;
        srow[t] = SM2 || SM1 ? conv_sg_row(mrow[t] / P, mrow[t] % P, P) : mrow[t];
    }
    conv_epilogue<COUT, CT, NPT, EPI, SM1, SM2>(acc, mrow, M, 0, kq, out, res, out2, par, srow, conv_sg_rows(M / P, P));
}

// LDS pointer type of the LDS-DMA builtins; counted wait on the in-order vector-memory counter (loads, stores and LDS-DMA share it)
typedef __attribute__((address_space(3))) void tg_lds_void;
#define TG_VMCNT(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory")
// raw s_barrier fenced for the COMPILER on both sides: the LDS-DMA writes are invisible to it (inline assembly, see below), so
// nothing else stops it from scheduling a fragment read of the next stage above the barrier that publishes that stage
#define TG_BARRIER() do { asm volatile("" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)

// LDS-DMA pieces (64 lanes x 16 B -> 1 KB of LDS at `lds`, lane-linear) issued as INLINE ASSEMBLY on purpose.  Through the
// builtins hipcc knows that LDS is being written asynchronously, cannot see that the kernels' own counted s_waitcnt + s_barrier
// already order every fragment read behind the pieces it needs, and inserts `s_waitcnt vmcnt(0)` in front of the next ds_read --
// which makes every wave wait for the pieces it has JUST issued (two stages of landing slack thrown away, once per stage).
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
__device__ __forceinline__ u32x4 tg_rsrc(const void* base, unsigned bytes) {       // raw buffer: stride 0, bounds check on the byte offset
    const unsigned long long a = (unsigned long long)base;
    return u32x4{(unsigned)a, (unsigned)(a >> 32) & 0xffffu, bytes, 0x00020000u};
}
__device__ __forceinline__ void tg_dma_global(const void* sbase /*wave-uniform*/, int voff_bytes, tg_lds_void* lds) {
    const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)lds);     // wave-uniform by construction; makes it an SGPR
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(la), "v"(voff_bytes), "s"(sbase) : "memory");
}
__device__ __forceinline__ void tg_dma_buffer(u32x4 rsrc, int voff_bytes, tg_lds_void* lds) {    // out-of-range offsets write zeros
    const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(la), "v"(voff_bytes), "s"(rsrc) : "memory");
}

// XOR swizzle of the 16-B chunk index for LDS images with 64-byte rows read as MFMA fragments by ds_read_b128 (lane = (j, kq):
// row base + j, chunk kq).  The instruction is served in four 16-lane groups, each holding all 16 values of j with kq = q0 for
// j in {0-3, 12-15} and q0^1 for j in {4-11} (MI355X_MICROARCH.md, LDS table); the 16-B slot of a lane is (row%4)*4 + chunk, so the
// four rows of one residue class, which use chunks (q0, q0^1, q0^1, q0) in row order, must land on four distinct chunks for every
// alignment of the base row: chunk ^ 2*((row>>2)&1) does that ({c, c^3, c^1, c^2}), the obvious chunk ^ ((row>>2)&3) is 2-way
// conflicted on every read (measured: SQ_LDS_BANK_CONFLICT = 49 % of SQ_LDS_IDX_ACTIVE).
__device__ __forceinline__ int swz64(int row) { return ((row >> 2) & 1) << 1; }

// ---- F->F 3x3 conv of the f32 tower (F = 128 / 256) ------------------------------------------------------------------------------
// SIN: the kernel's stream-side input is the residual stream in the conv's row order (slice-major, board-grouped).  EPI 0: `in` is
// that stream and s2 / t2 its BN: b = relu(s2 * b + t2) is applied to every B fragment in registers when it is handed over to the
// next stage (a stage after its load; s2 / t2 of the lane's 4 channels come from `par`, re-read when the slice changes) -- no tap
// that is walked lies off the board, so there is no zero padding the activation could spoil, and each value is bit for bit the one
// the producer's epilogue would have stored (bn_relu).  Without SIN `in` is already activated (bufAct).  EPI 1: `res` is the stream,
// and the accumulators start from it with one 16-B load per lane and (ct, t), a contiguous KB per wave (row-major `res`: sixteen
// 64-B pieces 81 * 4F bytes apart).  SOUT (EPI 1): `out` is written in the same order, else row-major for an attention layer or
// the head.
// Implicit GEMM on v_mfma_f32_16x16x4_f32: D[cout][board] += W[tap][cout][cin] * X[board][pos + tap][cin].
// Workgroup = ONE board position x 128 boards x all F couts: 4 waves x NPT = 2 tiles, a tile = that position on one group of 16
// boards (the 16 columns of an MFMA; conv_rows.h has the row order that makes such a tile one contiguous KB per slice).  Which of
// the nine taps fall on the board is therefore the same for the whole workgroup, and it walks ONLY those: 9 taps at the (S-2)^2
// interior positions, 6 on an edge, 4 in a corner -- (3S-2)^2 of the 9*S*S (position, tap) pairs, 625 of 729 at 9x9 and 3025 of
// 3249 at 19x19.  A tap off the board costs no weight DMA, no barrier, no fragment read and no MFMA (the row-ordered kernel this
// replaced loaded zeros for it and multiplied by them: 14.3 % of its MFMAs at 9x9).  Every output element still accumulates its
// on-board (slice, tap, k) terms in the same order, so results are those of the full walk (x + w*0 = x).
// Stage k = (16-channel slice k / nt, the (k % nt)-th on-board tap), nt = 4 / 6 / 9, so F/16 * nt stages -- always an even count.
// A (weights): the stage's tile arrives by LDS-DMA from a stage-ordered copy of the weights ([slice*9+tap][cout][16]) into a
// 4-slot ring (slot = k % 4), two stages per barrier, the next pair landing while this one is used (the prologue: stages 0 and 1
// in front of the first barrier, 2 and 3 behind it -- see "the fixed part" below); the LDS image is XOR-swizzled
// at the source (swz64) so ds_read_b128 fragments are conflict-free.  Stages per barrier at F = 128, measured on the row-ordered
// kernel: 2: 138.5, 3: 131.6, 4: 127.1 TFLOP/s.  B (activations): every wave loads its own B fragments straight from L2 into
// registers, a stage ahead; a tap is the wave-uniform shift of (dy*S + dx)*16 rows inside the board group.  Everything is at least
// a stage old when it is waited for, so each stage simply ends with s_waitcnt vmcnt(0).
// Boards past the batch: a wave none of whose groups exists skips its loads and MFMAs (it still feeds the weight ring and meets
// the barriers); absent boards next to present ones are computed on whatever their never-written rows hold and never stored -- an
// MFMA column depends on its own B column only.  The buffer resource ends with the padded tensor, so nothing is read past it.
// Workgroups are numbered per XCD (workgroup b runs on XCD b % 8 and is the (b >> 3)-th of its list, conv_launch_wg in conv_rows.h):
// an XCD takes whole board ranges, range-major and inside a range longest walk first (conv_pos_of), so the 81 (361) workgroups that
// share one range's input are neighbours on one L2 -- but its last K ranges and its share of the nrange % 8 leftover ranges are
// spent CLASS-major, every interior position, then every edge, then every corner: each XCD ends on its shortest walks, so fewer slots
// stand empty while the last workgroups finish (the order changes nothing that a workgroup computes).
// F = 128: 98 VGPRs (106 with the activation on load, 110 with a row-major residual) and 34 KB of LDS, four workgroups per CU;
// F = 256: 162 VGPRs (170 / 206) and 67 KB, two per CU.  Three tiles per wave
// (192 boards, three workgroups per CU at F = 128), the better shape of the row-ordered kernel on full rounds, measured 4-7 %
// slower here at 9x9 and 19x19: the walks differ in length, and four shorter waves per SIMD fill each other's gaps better.
// The fixed part of a workgroup, what it pays before its first MFMA:
//  * bias | s2 | t2 are fetched into registers FIRST and written to `par` behind everything the prologue issues, so their round
//    trip runs beside the weight DMAs instead of in front of them (the first barrier publishes `par`);
//  * the first barrier waits for the weight stages 0 and 1 only.  vmcnt retires in order, so what the first MFMA needs is issued
//    first: stages 0 and 1, the B fragments of stage 0, then (EPI 1) the residual in the order of use, ct-major.  Stages 2 and 3
//    go out behind the barrier and behind the first consumer of those loads (act_b, or an empty asm: the compiler waits for them
//    there with vmcnt(0), the accumulators being live into a loop, and that wait must not include two more weight stages), and land
//    during stage 0.  The stage-end vmcnt(0) covers them before the second barrier.  (In today's ISA the write of `par` still
//    carries a compiler vmcnt(0), so the first barrier also sees the wave's B fragments and residual landed: DESIGN.md 8.8);
//  * without the activation on load the hand-over b_cur = b_next goes through an empty asm at the END of the stage, as act_b does
//    with VALU: the compiler cannot fold the copy into the next stage's MFMA operands, so its own vmcnt(0) for the fragments
//    lands there, a stage after their load, and not in front of the next stage's first MFMA, a few instructions after the next load.
// The tail of a workgroup: the last pair of stages is peeled off the loop and closed by no barrier, and the last stage carries the
// epilogue between its MFMAs, a cout tile behind them (see there): a wave ends two stores after its last MFMA.
// -DTG_CONV_STAMP (diagnostic build only, scripts/stamp_conv.py): phase stamps of wave 0 of six workgroups at 9x9 / F = 128.
// It also records how a launch DRAINS (stamp_conv.py --drain): lane 0 of wave 0 of EVERY workgroup of the last conv1 /
// stream-to-stream conv2 launch leaves its entry and its end (every store issued) on the cycle counter and on the device-wide 100 MHz
// clock, its (range, p) and the XCD / CU it ran on, indexed by blockIdx.x.
#ifdef TG_CONV_STAMP
__device__ unsigned long long g_conv_stamp[2 * 6 * 8];                  // [EPI][interior, edge, corner of range 0 | of range 7][phase]
constexpr int TG_DRAIN_CAP = 16384, TG_DRAIN_REC = 6;                   // workgroups of a launch that are recorded, words per record
__device__ unsigned long long g_conv_drain[2 * TG_DRAIN_CAP * TG_DRAIN_REC];   // [EPI][blockIdx.x][entry, end, entry rt, end rt, range | p, xcc | hw_id]
#define TG_CSTAMP(i) do { __builtin_amdgcn_sched_barrier(0); if (cslot >= 0 && lane == 0) g_conv_stamp[cslot * 8 + (i)] = __builtin_readcyclecounter(); \
                          __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define TG_CSTAMP(i) do { } while (0)
#endif
// K of conv_launch_wg: the ranges per XCD that are spent class-major, from {1, 2, 4} (the runs that decided it: DESIGN.md 8.12).
// It lives here and not in conv_rows.h so that the source hash the committed traffic counters are keyed on covers it.
constexpr int conv_drain_k(int S, int F) { return S == 9 && (F == 128 || F == 256) ? 4 : 1; }
template <int S, int F, int EPI, bool SIN = false, bool SOUT = false>
__global__ __launch_bounds__(256, (F == 128 ? 4 : 2)) void k_conv3x3_sg(const float* __restrict__ in, float* __restrict__ out,
                                                                       const float* __restrict__ res, const float* __restrict__ Ws,
                                                                       const float* __restrict__ bias, float* __restrict__ out2,
                                                                       const float* __restrict__ s2, const float* __restrict__ t2, int rows) {
    constexpr int P = S * S, CT = F / 16, CC = 16;
    constexpr int NPT = 2, TB = 64 * NPT;                               // tiles per wave, boards per workgroup
    constexpr int WPW = CT / 4;
    constexpr int NSL = F / CC, D = 4;                                  // two stages per barrier, two pairs resident
    static_assert((F == 128 || F == 256) && NSL % 2 == 0, "tile geometry");
    static_assert(conv_drain_k(S, F) == 1 || conv_drain_k(S, F) == 2 || conv_drain_k(S, F) == 4, "the K that tests/test_conv_launch_order.py checks");
    __shared__ __attribute__((aligned(16))) float ws[D][F * CC];
    __shared__ __attribute__((aligned(16))) float par[3 * F];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, kq = lane >> 4;
#ifdef TG_CONV_STAMP
    const unsigned long long t_entry = __builtin_readcyclecounter(), rt_entry = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long* const drec = (EPI == 0 || SOUT) && tid == 0 && (int)blockIdx.x < TG_DRAIN_CAP
                                         ? g_conv_drain + ((size_t)(EPI == 1 ? TG_DRAIN_CAP : 0) + blockIdx.x) * TG_DRAIN_REC : nullptr;
#endif
    // XCD-aware, drain-aware order: workgroup b runs on XCD b % 8 and is the (b >> 3)-th of that XCD's list (conv_launch_wg) --
    // whole board ranges first, whose workgroups share one L2, and the short walks of its last ranges at the very end
    const int nrange = (rows + TB - 1) / TB;
    const conv_wg wg = conv_launch_wg((int)blockIdx.x & 7, (int)blockIdx.x >> 3, nrange, S, conv_drain_k(S, F));
#ifdef TG_CONV_STAMP
    if (drec && wg.range < 0) { drec[0] = drec[1] = t_entry; drec[2] = drec[3] = rt_entry; drec[4] = ~0ull; }
#endif
    if (wg.range < 0) return;                                           // the grid is 8 x the longest list
    const int range = wg.range, p = wg.p;
    const int M = rows * P, Msm = conv_sg_rows(rows, P);
    constexpr bool ACT = EPI == 0 && SIN;                               // s2 / t2 are then the BN of `in`, applied as its fragments land
#ifdef TG_CONV_STAMP
    // range 0 runs in the first round of XCD 0, range 7 in the middle of its run of 15; conv_pos_of: interior, edge, corner positions
    int cslot = -1;
    if (S == 9 && F == 128 && (EPI == 0 || SOUT) && wave == 0 && (range == 0 || range == 7)) {
        const int cls = p == conv_pos_of(conv_class_first(0, S), S) ? 0 : p == conv_pos_of(conv_class_first(1, S), S) ? 1
                        : p == conv_pos_of(conv_class_first(2, S), S) ? 2 : -1;   // the first position of each class
        if (cls >= 0) cslot = (EPI == 1 ? 6 : 0) + (range == 0 ? 0 : 3) + cls;
    }
    if (cslot >= 0 && lane == 0) g_conv_stamp[cslot * 8] = t_entry;
    if (drec) {                                                          // HW_REG_XCC_ID [3:0] and HW_REG_HW_ID (cu_id, sh_id, se_id in [15:8])
        drec[0] = t_entry; drec[2] = rt_entry; drec[4] = (unsigned long long)range << 32 | (unsigned)p;
        drec[5] = (unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32 | __builtin_amdgcn_s_getreg((31 << 11) | 4);
    }
#endif
    static_assert(F <= 256, "one parameter triple per thread");
    const bool bn = out2 || ACT;                                         // s2 / t2 are in use
    // this thread's element of bias | s2 | t2, in flight; no branch around the loads (see TG_PAR_LANDED)
    float pbias = bias[tid & (F - 1)], ps2 = (bn ? s2 : bias)[tid & (F - 1)], pt2 = (bn ? t2 : bias)[tid & (F - 1)];
    __builtin_amdgcn_sched_barrier(0);                                   // issued here, ahead of the weight DMAs
    TG_CSTAMP(1);

    // the workgroup's walk: nt on-board taps, packed 4 bits each; k / nt by a multiplication that is exact far beyond NSL * 9
    const unsigned mask = conv_tap_mask(p, S);
    const int nt = conv_tap_count(mask), nst = NSL * nt;
    const unsigned long long taps = conv_tap_list(mask);
    const int inv = nt == 9 ? 7282 : nt == 6 ? 10923 : 16384;           // ceil(65536 / nt)
    auto stage = [&](int k, int* sl, int* tap) {
        *sl = (k * inv) >> 16;
        *tap = (int)(taps >> (4 * (k - *sl * nt))) & 15;
    };

    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in), 0, Msm * F * 4, 0x00020000);
    const int prow = lane >> 2, pchunk = (lane & 3) ^ swz64(lane >> 2);
    auto dma_w = [&](int k) {
        int sl, tap;
        stage(k, &sl, &tap);
        const float* src = Ws + (size_t)(sl * 9 + tap) * (F * CC);
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            const int pc = wave * WPW + i;
            tg_dma_global(src + pc * 16 * CC, (prow * CC + pchunk * 4) * 4, (tg_lds_void*)(&ws[k & (D - 1)][pc * 256]));
        }
    };
    const int aoff = j * CC + ((kq ^ swz64(j)) << 2);
    const int grp0 = (range * 4 + wave) * NPT;                          // the wave's first board group
    const bool active = grp0 * 16 < rows;                               // wave-uniform
    const int boff = ((conv_sg_row(grp0 * 16 + j, p, P)) * CC + kq * 4) * 4;   // byte offset of this lane's 16 B inside slice 0, tile 0
    f32x4 acc[CT][NPT], b_cur[NPT], b_next[NPT];
    int sl_b = 0, sl_p = -1;                                             // slice of the fragments last loaded / of bsc, bsh (scalars)
    f32x4 bsc, bsh;                                                      // ACT: s1 / t1 of the lane's 4 channels (slice, kq)
    auto load_b = [&](f32x4* b, int k) {
        int sl, tap;
        stage(k, &sl, &tap);
        sl_b = sl;
        const int ty = (tap * 11) >> 5;                                  // tap / 3
        const int soff = (sl * Msm + ((ty - 1) * S + (tap - 3 * ty - 1)) * 16) * (CC * 4);   // wave-uniform: slice base + tap shift
#pragma unroll
        for (int t = 0; t < NPT; ++t)                                    // the offset carries everything: the range check is on it
            b[t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rin, (int)((unsigned)boff + (unsigned)soff + (unsigned)(t * (P * 16 * CC * 4))), 0, 0));
    };
    // b = relu(s1 * b + t1) on the fragments of the stage loaded last; s1 / t1 are re-read from `par` when the slice changes
    auto act_b = [&](f32x4* dst, const f32x4* b) {
        if (sl_b != sl_p) {
            sl_p = sl_b;
            bsc = *reinterpret_cast<const f32x4*>(par + F + sl_b * CC + kq * 4);
            bsh = *reinterpret_cast<const f32x4*>(par + 2 * F + sl_b * CC + kq * 4);
        }
#pragma unroll
        for (int t = 0; t < NPT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[t][e] = bn_relu_unpacked(b[t][e], bsc[e], bsh[e]);
    };
    constexpr int NRES = EPI == 1 ? CT * NPT : 0;                        // residual loads per lane
    // The triple is older than the DMAs just waited for.  It is taken over by an asm that differs between the two paths, so that
    // the compiler's wait for it stands on each path with that path's count (behind a merged tail it is vmcnt(0), and the barrier
    // would wait for the residual too)
#define TG_PAR_LANDED(PATH) asm volatile("; bias, s2, t2 landed: " PATH : "+v"(pbias), "+v"(ps2), "+v"(pt2))
    dma_w(0); dma_w(1);
    TG_CSTAMP(2);
    if (active) {
        load_b(b_cur, 0);
        __builtin_amdgcn_sched_barrier(0);                               // ahead of the residual: the first MFMA needs them first
#pragma unroll
        for (int i = 0; i < CT * NPT; ++i) {                             // EPI 1: start from the residual (no loads behind the epilogue's stores)
            const int ct = i / NPT, t = i % NPT;                         // in the order of use
            const int b = (grp0 + t) * 16 + j;
            [[maybe_unused]] const int m = b < rows ? b * P + p : M - 1;
            {
                acc[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                // always issued (they are never stored for boards past the batch): the wait below counts them
                if constexpr (EPI == 1 && SIN) {
                    // the stream in the conv's row order: a (ct, t) is one contiguous KB per wave.  Absent boards of a present group read
                    // their own never-written rows; a group past the padded tensor reads another slice or, past the end, zeros
                    const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(res), 0, Msm * F * 4, 0x00020000);
                    acc[ct][t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rres, (int)((unsigned)boff + (unsigned)(ct * Msm * (CC * 4)) + (unsigned)(t * (P * 16 * CC * 4))), 0, 0));
                } else if constexpr (EPI == 1) {
                    acc[ct][t] = *reinterpret_cast<const f32x4*>(res + (size_t)m * F + ct * 16 + kq * 4);   // row-major: the last row instead
                }
            }
        }
        // The barrier must see the weight DMAs of the first stages landed; the operations issued after them -- CT*NPT residual
        // loads, NPT B fragments -- are the wave's youngest and are waited for by the compiler, one by one, in front of the MFMA
        // that first needs each.
        TG_VMCNT(NRES + NPT);
        TG_PAR_LANDED("wave with boards");
    } else {
        TG_VMCNT(0);
        TG_PAR_LANDED("wave without boards");
    }
#undef TG_PAR_LANDED
    if (tid < F) { par[tid] = pbias; par[F + tid] = bn ? ps2 : 0.f; par[2 * F + tid] = bn ? pt2 : 0.f; }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    TG_BARRIER();
    TG_CSTAMP(3);
    if constexpr (ACT) {                                                 // `par` is published by the barrier above
        if (active) act_b(b_cur, b_cur);
        else {                                                           // written on both paths: the loop then waits for no load of b_cur
#pragma unroll
            for (int t = 0; t < NPT; ++t) b_cur[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    // Stages 2 and 3 go out behind the first consumer of everything loaded above: the compiler waits for those loads with
    // vmcnt(0) (the accumulators are live into a loop), which must not include two more weight stages.
    if (active) {
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
            if constexpr (!ACT) asm volatile("" : "+v"(b_cur[t]));
            if constexpr (EPI == 1) {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) asm volatile("" : "+v"(acc[ct][t]));
            }
        }
    }
    dma_w(2); dma_w(3);

    // One stage of the walk but the last: stage k's MFMAs under the loads of stage k + 1's fragments.
    auto walk_stage = [&](int k) {
        const float* wcur = ws[k & (D - 1)];
        load_b(b_next, k + 1);
        __builtin_amdgcn_sched_barrier(0);                               // keep the loads HERE: hipcc sinks them to their use, a stage later
        f32x4 a_cur = *reinterpret_cast<const f32x4*>(wcur + aoff);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            f32x4 a_next = a_cur;
            if (ct + 1 < CT) a_next = *reinterpret_cast<const f32x4*>(wcur + (ct + 1) * 256 + aoff);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int t = 0; t < NPT; ++t)
                    acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[s4], b_cur[t][s4], acc[ct][t], 0, 0, 0);
            a_cur = a_next;
#ifdef TG_CONV_STAMP
            if (ct == 0 && k == 0) TG_CSTAMP(4);                         // the first MFMAs have issued: their operands had landed
#endif
        }
        if constexpr (ACT) {
            __builtin_amdgcn_sched_barrier(0);                           // behind the stage's MFMAs: the fragments are a stage old here
            act_b(b_cur, b_next);
        } else {
            __builtin_amdgcn_sched_barrier(0);                           // the same place for the fragments' wait
#pragma unroll
            for (int t = 0; t < NPT; ++t) {
                asm volatile("" : "+v"(b_next[t]));
                b_cur[t] = b_next[t];
            }
        }
    };
#pragma unroll 1
    for (int k0 = 0; k0 < nst - 2; k0 += 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (active) walk_stage(k0 + h);
            TG_VMCNT(0);                                                 // B fragments of stage k+1 (and any weight pieces): a stage old
        }
        TG_BARRIER();                                                    // the next pair has landed for everybody; this pair's slots are free
        if (k0 + 4 < nst) { dma_w(k0 + 4); dma_w(k0 + 5); }
    }
    // The last pair (nst is even) is peeled.  It landed before the barrier above, no DMA follows and nobody writes the ring or `par`
    // again, so no barrier closes it: a wave goes from its last MFMAs to its stores and ends without waiting for the slowest one.
    if (!active) return;
    walk_stage(nst - 2);
    TG_VMCNT(0);
    // The last stage with the epilogue inside it.  acc[ct][.] is final once cout tile ct's 4 * NPT MFMAs have issued: bias (ReLU for
    // EPI 0; EPI 1 started from the residual) and the 16-B store of tile ct go out behind the first NPT MFMAs of tile ct + 1, whose
    // issue covers the results' latency, and only the last tile's NPT stores stand behind the last MFMA.  Per element the same terms
    // in the same order as a walk followed by conv_epilogue, and the same expressions behind them.  Buffer stores: the whole address
    // is a 32-bit byte offset (the lane's row + the cout tile), and a board past the batch carries an offset past the tensor, which
    // the range check drops -- no branch between the MFMAs.  `out2` is always null on this kernel and is left out here.
    constexpr bool SM = EPI == 0 || SOUT;                                // `out` slice-major in the conv's row order, else row-major
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out, 0, (SM ? Msm : M) * F * 4, 0x00020000);
    const unsigned ostep = SM ? (unsigned)Msm * (CC * 4) : CC * 4;       // bytes from one cout tile to the next
    unsigned ooff[NPT];
#pragma unroll
    for (int t = 0; t < NPT; ++t) {
        const int b = (grp0 + t) * 16 + j;
        ooff[t] = b >= rows ? 0x80000000u : SM ? (unsigned)(conv_sg_row(b, p, P) * CC + kq * 4) * 4 : (unsigned)((b * P + p) * F + kq * 4) * 4;
    }
    auto store_tile = [&](int ct, f32x4 bv) {
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
            f32x4 v = acc[ct][t] + bv;
            if constexpr (EPI == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rout, (int)(ooff[t] + (unsigned)ct * ostep), 0, 0);
        }
    };
    {
        const float* wcur = ws[(nst - 1) & (D - 1)];
        const float* pb = par + kq * 4;
        __builtin_amdgcn_sched_barrier(0);                               // the offsets above are computed in front of the stage
        f32x4 a_cur = *reinterpret_cast<const f32x4*>(wcur + aoff);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            f32x4 a_next = a_cur, bv = a_cur;
            if (ct + 1 < CT) a_next = *reinterpret_cast<const f32x4*>(wcur + (ct + 1) * 256 + aoff);
            if (ct > 0) bv = *reinterpret_cast<const f32x4*>(pb + (ct - 1) * 16);   // read here, used two MFMAs on
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
#pragma unroll
                for (int t = 0; t < NPT; ++t)
                    acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[s4], b_cur[t][s4], acc[ct][t], 0, 0, 0);
                if (s4 == 0 && ct > 0) {                                 // hipcc sinks stores to the end: keep tile ct - 1's HERE
                    __builtin_amdgcn_sched_barrier(0);
                    store_tile(ct - 1, bv);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            a_cur = a_next;
        }
        TG_CSTAMP(5);                                                    // the last MFMA has issued
        __builtin_amdgcn_sched_barrier(0);
        store_tile(CT - 1, *reinterpret_cast<const f32x4*>(pb + (CT - 1) * 16));
    }
#ifdef TG_CONV_STAMP
    TG_CSTAMP(6);                                                        // every store issued
    if (drec) { drec[1] = __builtin_readcyclecounter(); drec[3] = __builtin_amdgcn_s_memrealtime(); }
    TG_VMCNT(0);
    TG_CSTAMP(7);                                                        // and written: the wave can end
#endif
}

// fp16 activation tensors are CHUNK-MAJOR: [channels/32 slices][4 chunks of 8 channels][M rows][8 halfs].  A slab DMA piece (64 rows
// x 16 B of one chunk plane) is one contiguous KB in memory (a row-major piece is 16 half-used lines 2F bytes apart and costs the
// texture-address path ~3x as much), and the LDS image it builds -- plane after plane, rows 16 B apart -- is read by ds_read_b128
// MFMA fragments without bank conflicts and WITHOUT a swizzle: lane (row j, chunk kq) reads plane kq at row R + j, the 16-lane
// service groups of the instruction (MI355X_MICROARCH.md, LDS table) then cover 64 distinct banks as long as a plane is a multiple
// of 16 rows, so a tap is a constant byte offset (round 1 kept rows of 64 B and XOR-swizzled the chunk index by the row, which cost
// ~8 vector instructions of address arithmetic per fragment).  Element (row m, channel c):
__device__ __forceinline__ size_t h16_index(int m, int c, int M) { return (((size_t)(c >> 5) * 4 + ((c >> 3) & 3)) * M + m) * 8 + (c & 7); }

// s_waitcnt vmcnt(n) for a wave-uniform n in [0, N]: the instruction takes an immediate
template <int N>
__device__ __forceinline__ void vmcnt_uniform(int n) {
    if (n >= N) TG_VMCNT(N);
    else if constexpr (N > 0) vmcnt_uniform<N - 1>(n);
}

// Epilogue of k_conv3x3_h2 in the PAIRED cout mapping: the weights are restaged (k_restage_half, pair8) so that row i of A tile ct
// is physical cout (ct >> 1) * 32 + (i >> 2) * 8 + (ct & 1) * 4 + (i & 3); lane kq then holds, across the tile pair (2u, 2u + 1),
// the 8 CONSECUTIVE couts u * 32 + kq * 8 .. + 7 of its row -- one whole 16-B chunk of the chunk-major fp16 tensors.  Every fp16
// access of the epilogue (and the fp16 residual read that starts the accumulators) is one 16-B access per lane instead of two
// 8-B ones: half the memory instructions on the path that the DMA pieces already load.
// X2 (split precision, net_precision 3): the accumulators hold the conv of weights scaled by 2^s (wsc = 2^-s undoes it, exactly),
// and every fp16 output is written as TWO chunks -- hi = half(v), lo = half(v - hi) -- at the [16 hi | 16 lo] positions of the
// channel group (x2_index), which is what the next conv's K = 32 MFMA step consumes.
__device__ __forceinline__ int x2_index(int c) { return ((c >> 4) << 5) + (c & 15); }       // hi position of real channel c; lo = + 16
template <int F, int CT, int NPT, int EPI, bool R16, bool X2 = false>
__device__ __forceinline__ void conv_epilogue_h8(f32x4 (&acc)[CT][NPT], const int (&mrow)[NPT], int M, int co_base, int kq,
                                                 float* __restrict__ out32, _Float16* __restrict__ out16, const float* par, int pstride,
                                                 float wsc, float& amax) {
    // amax: largest |value| this lane rounded to fp16 (range guard: above 65504 the fp16 copy is inf and the next layer computes
    // NaN; the caller raises the network's sticky overflow counter, tg_net_range)
    static_assert(CT % 2 == 0, "tile pairs");
    static_assert(!(X2 && R16), "split precision keeps the f32 residual stream");
#pragma unroll
    for (int t = 0; t < NPT; ++t) {
        if (mrow[t] >= M) continue;
#pragma unroll
        for (int u = 0; u < CT / 2; ++u) {
            const int lc = u * 32 + kq * 8, col = co_base + lc;
            f32x4 v[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) v[h] = (X2 ? acc[2 * u + h][t] * wsc : acc[2 * u + h][t]) + *reinterpret_cast<const f32x4*>(par + lc + 4 * h);
            h8 o;
            if constexpr (X2) {
                auto store_split = [&](const f32x4 (&w)[2]) {
                    h8 hi, lo;
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float x = w[e >> 2][e & 3]; hi[e] = (_Float16)x; lo[e] = (_Float16)(x - (float)hi[e]); }
#pragma unroll
                    for (int e = 0; e < 8; e += 2) amax = __builtin_fmaxf(amax, __builtin_fmaxf(__builtin_fabsf(w[e >> 2][e & 3]), __builtin_fabsf(w[e >> 2][(e & 3) + 1])));
                    const int c2 = x2_index(col);
                    *reinterpret_cast<h8*>(out16 + h16_index(mrow[t], c2, M)) = hi;
                    *reinterpret_cast<h8*>(out16 + h16_index(mrow[t], c2 + 16, M)) = lo;
                };
                if (EPI == 0 || EPI == 4) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[h][e] = v[h][e] > 0.f ? v[h][e] : 0.f;
                }
                if (EPI == 0) { store_split(v); continue; }
                if (out32) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) *reinterpret_cast<f32x4*>(out32 + (size_t)mrow[t] * F + col + 4 * h) = v[h];
                }
                if (out16) {
                    f32x4 w[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f32x4 sc = *reinterpret_cast<const f32x4*>(par + pstride + lc + 4 * h);
                        const f32x4 sh = *reinterpret_cast<const f32x4*>(par + 2 * pstride + lc + 4 * h);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const float y = v[h][e] * sc[e] + sh[e]; w[h][e] = y > 0.f ? y : 0.f; }
                    }
                    store_split(w);
                }
                continue;
            }
            if (EPI == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float w = v[e >> 2][e & 3]; o[e] = (_Float16)(w > 0.f ? w : 0.f); amax = __builtin_fmaxf(amax, w); }
                *reinterpret_cast<h8*>(out16 + h16_index(mrow[t], col, M)) = o;
            } else {
                if (EPI == 4) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[h][e] = v[h][e] > 0.f ? v[h][e] : 0.f;
                }
                if (out32) {                                             // null: the last block (only its activation feeds the head)
                    if (R16) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) { o[e] = (_Float16)v[e >> 2][e & 3]; amax = __builtin_fmaxf(amax, __builtin_fabsf(v[e >> 2][e & 3])); }
                        *reinterpret_cast<h8*>(reinterpret_cast<_Float16*>(out32) + h16_index(mrow[t], col, M)) = o;
                    } else {
#pragma unroll
                        for (int h = 0; h < 2; ++h) *reinterpret_cast<f32x4*>(out32 + (size_t)mrow[t] * F + col + 4 * h) = v[h];
                    }
                }
                if (out16) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f32x4 sc = *reinterpret_cast<const f32x4*>(par + pstride + lc + 4 * h);
                        const f32x4 sh = *reinterpret_cast<const f32x4*>(par + 2 * pstride + lc + 4 * h);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const float w = v[h][e] * sc[e] + sh[e]; o[4 * h + e] = (_Float16)(w > 0.f ? w : 0.f); amax = __builtin_fmaxf(amax, w); }
                    }
                    *reinterpret_cast<h8*>(out16 + h16_index(mrow[t], col, M)) = o;
                }
            }
        }
    }
}

// Workgroup = 4 waves = 256 rows x 128 couts (the block index picks the cout half at F=256; wave tile 128 couts x 64 rows = 8x4
// accumulator tiles, 12 ds_read_b128 per 32 MFMAs).  Stage = (32-channel slice, tap); stages are handled in PAIRS per barrier:
// 4-slot weight ring (8 KB per slot, global_load_lds one pair ahead), two 32-channel slab buffers (rows + halo, buffer_load..lds,
// bounds check = zero fill) -- 70 KB of LDS and <= 256 VGPRs, so TWO workgroups share a CU and one computes while the other sits
// in its barrier, its slab wait or its epilogue.  The kernel can walk a (row tile, cout half) list with the next tile's first
// DMAs issued before the current tile's stores (gridDim.x a multiple of 16), but is launched with one block per tile.  Weight traffic: 1.18 MB per 256 rows (~4 TB/s of L2
// reads chip-wide at 1 PFLOP/s).  Measured shares of a 0.88-ms launch (8192 boards, F=256; ablation builds): MFMA loop alone
// 0.44, DMA issue + traffic 0.17, epilogue 0.22, B-fragment addressing + reads 0.09, barriers 0.03, A reads 0.03.
// An 8-wave 256x256 tile with one workgroup per CU (64-channel stages) measured 827 vs 888 TFLOP/s for this shape.
// X2 = split precision (net_precision 3, "f32x3"): the tensors hold every real channel as fp16 hi + lo, a 32-wide channel group
// being [16 real channels hi | the same 16 lo] in activations and weights alike (CIN counts those positions: 2 x the real input
// channels).  One K = 32 MFMA step with the B fragment [a_hi | a_lo] against the A fragment [w_hi | w_hi] gives w_hi*(a_hi + a_lo),
// a second one against [w_lo | w_lo] gives w_lo*(a_hi + a_lo): all four products of (w_hi + w_lo)(a_hi + a_lo) in f32
// accumulation from ONE read of the activations and two reads of the SAME weight tile (lane (j, kq) takes 16-B chunk kq & 1 of
// row j for the hi fragment, 2 + (kq & 1) for the lo one -- no duplicate storage, the swizzle and its conflict-freedom carry
// over).  4 x the MFMA work of the plain fp16 conv at ~22 significand bits per operand, against 16 x for the exact-f32 MFMA.
// Only THREE of the four products are formed -- w_lo*a_lo is dropped and the two lo-weight products of a pair of stages share one
// K = 32 step (see the stage loop): 3 x the MFMA work of the plain fp16 conv.
template <int S, int CIN, int F, int EPI, bool R16 = false, bool X2 = false>
__global__ __launch_bounds__(256, 2) void k_conv3x3_h2(const _Float16* __restrict__ in, float* __restrict__ out32,
                                                       _Float16* __restrict__ out16, const float* __restrict__ res,
                                                       const _Float16* __restrict__ Ws, const float* __restrict__ bias,
                                                       const float* __restrict__ s2, const float* __restrict__ t2, int M, int nblk,
                                                       const float* __restrict__ wsc_p, unsigned* __restrict__ ovf) {
    constexpr int P = S * S, HALO = S + 1, KC = 32, NW = 4, NPT = 4, TM = 64 * NW, NCO = 128, CT = NCO / 16, COS = F / NCO;
    constexpr int NCHK = KC / 8, RPP = 64 / NCHK;                       // 4 chunks per 64-B row, 16 rows per 1-KB DMA piece
    constexpr int NSL = CIN / KC, NST = NSL * 9, NPAIR = NST / 2, NSLOT = 4;        // CIN input channels (row stride), F output channels
    constexpr int NROW = TM + 2 * HALO;
    constexpr int PLR = (NROW + 63) / 64 * 64;                          // rows of one chunk plane of the slab image (whole 1-KB pieces)
    constexpr int NXP = NCHK * (PLR / 64);                              // slab pieces: 4 planes x PLR/64
    constexpr int NXQ = (NXP + NW - 1) / NW;
    constexpr int WPW = NCO / RPP / NW;                                 // weight pieces per wave per stage (2)
    static_assert(NST % 2 == 0 && CIN % KC == 0 && F % NCO == 0 && NCO % (RPP * NW) == 0, "tile geometry");
    __shared__ __attribute__((aligned(16))) _Float16 xs[2][NCHK * PLR * 8];
    __shared__ __attribute__((aligned(16))) _Float16 ws[NSLOT][NCO * KC];
    __shared__ __attribute__((aligned(16))) float par[3 * NCO];
    __shared__ __attribute__((aligned(16))) float zrow[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, kq = lane >> 4;
    // the COS cout parts of one row tile are blocks b and b+8: same XCD (b % 8), dispatched together, so the slab's second read hits L2
    // Persistent: this workgroup takes blocks bid, bid + gridDim.x, ... (gridDim.x is a multiple of 8*COS, so the cout part co0
    // never changes); blocks whose rows lie past M (the block count is rounded up) are skipped.
    auto tile_m0 = [&](int b) {
        (void)nblk;                                                     // captured: keeps the tile walk's code as measured
        return (COS == 1 ? b : (b / (8 * COS)) * 8 + b % 8) * TM;
    };
    int bid = blockIdx.x;
    const int co0 = COS == 1 ? 0 : ((bid / 8) % COS) * NCO;
    while (bid < nblk && tile_m0(bid) >= M) bid += gridDim.x;
    if (bid >= nblk) return;
    int m0 = tile_m0(bid);
    if (tid < 4) zrow[tid] = 0.f;
    for (int i = tid; i < NCO; i += 256) {
        par[i] = bias[co0 + i]; par[NCO + i] = out16 && s2 ? s2[co0 + i] : 0.f; par[2 * NCO + i] = out16 && t2 ? t2[co0 + i] : 0.f;
    }
    const u32x4 rin = tg_rsrc(in, (unsigned)M * CIN * 2);
    // weight pieces: 16 rows (couts) x 64 B; lane -> row prow, physical chunk pchk, which holds logical chunk pchk ^ swz64(row)
    const int prow = lane / NCHK, pchk = lane % NCHK;
    const int lane_w = prow * KC + (pchk ^ swz64(prow)) * 8;              // halfs, stage-tile rows are KC halfs apart
    // slab pieces: 64 rows x 16 B of one chunk plane, contiguous in memory and in LDS (lane = row)
    auto dma_x = [&](int sl) {
#pragma unroll
        for (int i = 0; i < NXQ; ++i) {
            const int q = wave * NXQ + i;
            if (q < NXP) {                                               // wave-uniform
                const int plane = q / (PLR / 64), rg = q % (PLR / 64);
                // the whole offset must travel in voffset: soffset is not range-checked, and rows outside the tensor must read 0
                // (before its first plane / past its last one: bounds check).  Rows m < 0 or >= M of an inner plane read the
                // neighbouring plane's rows instead -- finite values that only masked taps could ever select
                const int voff = (((sl * NCHK + plane) * M + m0 - HALO + rg * 64) * 8) * 2 + lane * 16;
                tg_dma_buffer(rin, voff, (tg_lds_void*)(&xs[sl & 1][(plane * PLR + rg * 64) * 8]));
            }
        }
    };
    auto dma_w = [&](int g) {
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            const int pc = wave * WPW + i;
            const _Float16* wb = Ws + ((size_t)g * F + co0 + pc * RPP) * KC;                       // wave-uniform
            tg_dma_global(wb, lane_w * 2, (tg_lds_void*)(&ws[g % NSLOT][pc * 512]));
        }
    };
    auto prologue = [&]() {                                              // order matters for the counted wait below
        dma_x(0); dma_w(0); dma_w(1);
        if (NSL > 1) dma_x(1);
        dma_w(2); dma_w(3);
    };
    prologue();
    bool first = true;
    const int aoff = j * KC + (((X2 ? (kq & 1) : kq) ^ swz64(j)) << 3);   // A fragment of cout tile ct: + ct*16*KC (X2: the hi half)
    const int aoff_lo = j * KC + (((2 + (kq & 1)) ^ swz64(j)) << 3);      // X2: the lo half of the same rows
    const float wsc = X2 ? wsc_p[0] : 1.f, wsc_inv = X2 ? 1.f / wsc : 1.f;   // powers of two: both exact
    for (;;) {
        unsigned vmask[NPT]; int vrow[NPT];
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
            const int m = m0 + (wave * NPT + t) * 16 + j;
            unsigned mk = 0;
            if (m < M) {
                const int p = m % P, x = p % S, y = p / S;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                    if (yy >= 0 && yy < S && xx >= 0 && xx < S) mk |= 1u << tap;
                }
            }
            vmask[t] = mk; vrow[t] = (wave * NPT + t) * 16 + j + HALO;
        }
        auto read_b = [&](f32x4* b, int g) {
            const int sl = g / 9, tap = g % 9;
            const int toff = (tap / 3 - 1) * S + (tap % 3 - 1);
            const _Float16* base = xs[sl & 1];
#pragma unroll
            for (int t = 0; t < NPT; ++t) {
                const int R = vrow[t] + toff;
                const _Float16* src = ((vmask[t] >> tap) & 1) ? base + ((kq * PLR + R) << 3)
                                                              : reinterpret_cast<const _Float16*>(zrow);
                b[t] = *reinterpret_cast<const f32x4*>(src);
            }
        };
        // EPI 1: the accumulators START from the residual (32 loads per wave that fly while the first DMAs land), so the epilogue
        // has no load in it -- a load issued after stores waits for them (one in-order counter): 8 serial round trips per tile
        f32x4 acc[CT][NPT];
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
            const int m = m0 + (wave * NPT + t) * 16 + j;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                if (!(EPI == 1 && R16 && ct % 2 == 1)) acc[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};   // (set by its pair's load)
                if (EPI == 1) {
                    // always issued (rows past the batch re-read the last row and are never stored): the number of residual loads in
                    // flight must be the same for every wave, because the wait below counts them.  Paired cout mapping (see
                    // conv_epilogue_h8): one 16-B load covers this lane's 8 couts of the tile pair.
                    const int mc = m < M ? m : M - 1;
                    if (R16) {
                        if (ct % 2 == 0) {
                            const h8 rh = *reinterpret_cast<const h8*>(reinterpret_cast<const _Float16*>(res) + h16_index(mc, co0 + (ct >> 1) * 32 + kq * 8, M));
#pragma unroll
                            for (int e = 0; e < 4; ++e) { acc[ct][t][e] = (float)rh[e]; acc[ct + 1][t][e] = (float)rh[4 + e]; }
                        }
                    } else {
                        acc[ct][t] = *reinterpret_cast<const f32x4*>(res + (size_t)mc * F + co0 + (ct >> 1) * 32 + kq * 8 + (ct & 1) * 4);
                        if (X2) acc[ct][t] = acc[ct][t] * wsc_inv;              // the accumulators run in the scaled-weight domain
                    }
                }
            }
        }
        // first tile of a residual-free launch: only the prologue DMAs are in flight, so the wait can leave X(1), W(2), W(3) out.
        // Residual variant: the CT*NPT residual loads are the YOUNGEST operations of the wave (the prologue DMAs and, in a persistent
        // walk, the previous tile's stores are older), so waiting until only they are outstanding releases the first barrier as soon
        // as the DMAs have landed; each accumulator's own load is then waited for by the compiler, in order, right before its first
        // MFMA -- the 0.34-0.68 GB residual read no longer sits in front of the whole tile.
        if (EPI != 1 && first && NSL > 1) vmcnt_uniform<NXQ + 2 * WPW>((NXP - wave * NXQ < 0 ? 0 : NXP - wave * NXQ > NXQ ? NXQ : NXP - wave * NXQ) + 2 * WPW);
        else if (EPI != 1 && first) TG_VMCNT(2 * WPW);
        else if (EPI == 1) TG_VMCNT(R16 ? CT / 2 * NPT : CT * NPT);
        else TG_VMCNT(0);
        first = false;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        TG_BARRIER();
        f32x4 b_cur[NPT], b_next[NPT];
        read_b(b_cur, 0);

#pragma unroll 1                                                         // unrolled, hipcc keeps 4 pairs of address state live and spills
        for (int pp = 0; pp < NPAIR; ++pp) {
          const int g0 = 2 * pp;
          if constexpr (X2) {
            // THREE partial products per pair of stages instead of four: w_lo * a_lo (2^-22 of a product, below the f32 rounding of the
            // sum) is dropped.  Steps of a pair (s0, s1 = its two stages, same or neighbouring slice, both tiles in the ring):
            //   CT steps  [w_hi(s0) | w_hi(s0)] x [a_hi(s0) | a_lo(s0)]      (as before)
            //   CT steps  [w_hi(s1) | w_hi(s1)] x [a_hi(s1) | a_lo(s1)]      (as before)
            //   CT steps  [w_lo(s0) | w_lo(s1)] x [a_hi(s0) | a_hi(s1)]      -- both lo-weight products in ONE K = 32 step: the B operand is
            //             made in place from the two stages' fragments by v_permlane32_swap (the hi halves live in lanes 0-31), the A
            //             operand takes its lo chunks from tile s0 in lanes 0-31 and from tile s1 in lanes 32-63.
            // 3/4 of the MFMA steps and of the weight-fragment reads; b_cur holds s0's fragments, b_next s1's, and after the swap
            // b_next is free for the next pair's first stage.
            constexpr int NU = 3 * CT, DA = 4;
            const _Float16* const wmix = ws[(g0 + (kq >> 1)) % NSLOT] + aoff_lo;
            auto a_addr = [&](int un) -> const _Float16* {
                const int kind = un / CT, ct = un % CT;
                return kind == 2 ? wmix + ct * 16 * KC : ws[(g0 + kind) % NSLOT] + ct * 16 * KC + aoff;
            };
            f32x4 a[DA];
#pragma unroll
            for (int u = 0; u < DA - 1; ++u) a[u] = *reinterpret_cast<const f32x4*>(a_addr(u));
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                if (u + DA - 1 < NU) a[(u + DA - 1) % DA] = *reinterpret_cast<const f32x4*>(a_addr(u + DA - 1));
                if (u == CT / 2) read_b(b_next, g0 + 1);                                  // s1's fragments, needed from step CT on
                if (u == 2 * CT) {                                                        // b_cur <- [a_hi(s0) | a_hi(s1)]
#pragma unroll
                    for (int t = 0; t < NPT; ++t)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float fc = b_cur[t][e], fn = b_next[t][e];     // (scalar copies: a bit_cast of a vector ELEMENT miscompiles)
                            const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(fc), __float_as_uint(fn), false, false);
                            b_cur[t][e] = __uint_as_float(r[0]);
                        }
                }
                if (u == 2 * CT + CT / 2 && g0 + 2 < NST) read_b(b_next, g0 + 2);         // the next pair's first stage (its slab is visible)
                const int ct = u % CT;
#pragma unroll
                for (int t = 0; t < NPT; ++t)
                    acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a[u % DA]), __builtin_bit_cast(h8, u / CT == 1 ? b_next[t] : b_cur[t]),
                                                                        acc[ct][t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int t = 0; t < NPT; ++t) b_cur[t] = b_next[t];
          } else {
            constexpr int SPS = CT;                                      // MFMA steps per stage
            constexpr int NU = 2 * SPS, DA = 4;
            // A fragments run DA-1 steps ahead of their MFMAs (a step = 4 MFMAs = 64 cycles; an LDS read under load takes longer)
            auto a_addr = [&](int un) -> const _Float16* { return ws[(g0 + un / SPS) % NSLOT] + (un % SPS) * 16 * KC + aoff; };
            f32x4 a[DA];
#pragma unroll
            for (int u = 0; u < DA - 1; ++u) a[u] = *reinterpret_cast<const f32x4*>(a_addr(u));
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                if (u + DA - 1 < NU) a[(u + DA - 1) % DA] = *reinterpret_cast<const f32x4*>(a_addr(u + DA - 1));
                if (u % SPS == SPS / 2 && g0 + u / SPS + 1 < NST) read_b(b_next, g0 + u / SPS + 1);   // that stage's slab is visible (see below)
                const int ct = u % SPS;
#pragma unroll
                for (int t = 0; t < NPT; ++t)
                    acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a[u % DA]), __builtin_bit_cast(h8, b_cur[t]),
                                                                        acc[ct][t], 0, 0, 0);
                if (u % SPS == SPS - 1) {
#pragma unroll
                    for (int t = 0; t < NPT; ++t) b_cur[t] = b_next[t];
                }
                __builtin_amdgcn_sched_barrier(0);                      // keep each step's reads where they were issued (hipcc sinks them to their use)
            }
          }
            // every DMA of this wave was issued at least one pair ago: wait for all of them, then meet the other waves.  After the
            // barrier the two slots of this pair are free, and so is the slab buffer of slice sl-1 once stage 9*sl-1 is behind us.
            TG_VMCNT(0);
            TG_BARRIER();
            const int gdone = g0 + 1;                                    // last finished stage
            // the slab of slice sl+1 goes into the buffer slice sl-1 used: issue it right after the pair that finished stage 9*sl-1
            // (it is fenced by the NEXT pair's barrier, i.e. before stage 9*sl+3; first read by the prefetch in stage 9*sl+8)
            {
                const int sl = (gdone + 1) / 9;
                if (sl >= 1 && sl + 1 < NSL && (gdone == 9 * sl - 1 || gdone == 9 * sl)) dma_x(sl + 1);
            }
            if (g0 + 4 < NST) { dma_w(g0 + 4); dma_w(g0 + 5); }
        }
        int mrow[NPT];
#pragma unroll
        for (int t = 0; t < NPT; ++t) mrow[t] = m0 + (wave * NPT + t) * 16 + j;
        if constexpr (X2) {
            // opaque here: computed before the stage loop, the epilogue's 64-bit addresses are spilled across it and reloaded BEHIND the
            // epilogue's stores (scratch reloads queue on the same in-order counter)
            static_assert(NPT == 4, "four row tiles per wave");
            asm volatile("" : "+v"(mrow[0]), "+v"(mrow[1]), "+v"(mrow[2]), "+v"(mrow[3]));
        }
        int Me = M, kqe = kq;                                             // likewise the row count and the lane's chunk index the plane offsets are made of
        if constexpr (X2) { asm volatile("" : "+s"(Me)); asm volatile("" : "+v"(kqe)); }
        // every wave is past the last barrier: ring and slab buffers are free, so the next tile's first loads go out before this
        // tile's results do and land while the epilogue runs
        int nb = bid + gridDim.x;
        while (nb < nblk && tile_m0(nb) >= M) nb += gridDim.x;
        const bool have_next = nb < nblk;
        if (have_next) { bid = nb; m0 = tile_m0(nb); prologue(); }
        float amax = 0.f;
        conv_epilogue_h8<F, CT, NPT, (EPI == 1 ? 2 : EPI), R16, X2>(acc, mrow, Me, co0, kqe, out32, out16, par, NCO, wsc, amax);   // EPI 4: the stem
        // range guard: one compare + ballot per tile and wave, an atomic only when a value left the fp16 range (sticky counter)
        if (__builtin_amdgcn_ballot_w64(!(amax <= 65504.f)) != 0 && lane == 0) atomicAdd(ovf, 1u);
        if (!have_next) break;
    }
}

// stage-ordered fp16 copy of a conv: dst[(slice*9 + tap)][cout][KC] = half(w[tap][cout][slice*KC + c]) for c < cin_src, else 0
// (w is [9][COUT][cin_src]; the destination covers cin_dst >= cin_src channels: the stem pads its 16 input planes to 64)
__global__ __launch_bounds__(256) void k_restage_half(const float* __restrict__ w, _Float16* __restrict__ dst, int COUT, int cin_src,
                                                      int cin_dst, int KC, int pair8) {
    const size_t total = (size_t)9 * COUT * cin_dst;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % KC);
        const size_t r = i / KC;
        int co = (int)(r % COUT);
        const int st = (int)(r / COUT);
        const int sl = st / 9, tap = st % 9;
        const int ci = sl * KC + c;
        // pair8 (k_conv3x3_h2): destination row r of a 32-row group holds physical cout ((r & 15) >> 2) * 8 + ((r >> 4) & 1) * 4 + (r & 3)
        if (pair8) co = (co & ~31) | ((((co & 15) >> 2) << 3) + (((co >> 4) & 1) << 2) + (co & 3));
        dst[i] = ci < cin_src ? (_Float16)w[((size_t)tap * COUT + co) * cin_src + ci] : (_Float16)0.f;
    }
}

// Split precision (net_precision 3).  k_absmax: largest |w| of one conv as float bits (non-negative floats order like unsigned ints).
__global__ __launch_bounds__(256) void k_absmax(const float* __restrict__ w, size_t n, unsigned* __restrict__ out) {
    unsigned m = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned b = __float_as_uint(w[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(m, o); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
// stage-ordered split copy: dst[(slice*9 + tap)][cout][32] = [16 channels hi | the same 16 lo] of w * 2^s, slice = 16 real input
// channels (zero beyond cin_src), hi = half(v), lo = half(v - hi); s puts the conv's largest weight in [2^14, 2^15), so that the
// lo halves of all but negligible weights are normal fp16 numbers; wsc_out = 2^-s for the epilogue.  pair8 as in k_restage_half.
__global__ __launch_bounds__(256) void k_restage_split(const float* __restrict__ w, _Float16* __restrict__ dst, float* __restrict__ wsc_out,
                                                       const unsigned* __restrict__ maxbits, int COUT, int cin_src, int nsl_dst, int pair8) {
    const unsigned mb = maxbits[0];
    int sh = mb ? 14 - ((int)((mb >> 23) & 0xffu) - 127) : 0;
    sh = sh < -60 ? -60 : sh > 60 ? 60 : sh;
    const float scale = ldexpf(1.f, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) wsc_out[0] = ldexpf(1.f, -sh);
    const size_t total = (size_t)nsl_dst * 9 * COUT * 32;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int k = (int)(i & 31);
        const size_t r = i >> 5;
        int co = (int)(r % COUT);
        const int st = (int)(r / COUT);
        const int sl = st / 9, tap = st % 9;
        const int ci = sl * 16 + (k & 15);
        if (pair8) co = (co & ~31) | ((((co & 15) >> 2) << 3) + (((co >> 4) & 1) << 2) + (co & 3));
        const float v = ci < cin_src ? w[((size_t)tap * COUT + co) * cin_src + ci] * scale : 0.f;
        const _Float16 hi = (_Float16)v;
        dst[i] = (k & 16) ? (_Float16)(v - (float)hi) : hi;
    }
}

// stage-ordered f32 copy of an F->F conv for k_conv3x3_sg: dst[(slice*9 + tap)][cout][16] = w[tap][cout][slice*16 + c]
__global__ __launch_bounds__(256) void k_restage_f32(const float* __restrict__ w, float* __restrict__ dst, int F) {
    const size_t total = (size_t)9 * F * F;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i & 15);
        const size_t r = i >> 4;
        const int co = (int)(r % F);
        const int st = (int)(r / F);
        dst[i] = w[((size_t)(st % 9) * F + co) * F + (st / 9) * 16 + c];
    }
}

// network input for the fp16 stem: obs f32 [rows][C][P] (planes of 0/1, exact in fp16) -> x0h, 64 channels, chunk-major (h16_index)
template <int S>
__global__ __launch_bounds__(256) void k_obs_to_rows_h(const float* __restrict__ obs, _Float16* __restrict__ x0, int rows, int C) {
    constexpr int P = S * S;
    const size_t total = (size_t)rows * P * 64;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i & 63);
        const size_t m = i >> 6;
        const int p = (int)(m % P);
        const size_t r = m / P;
        x0[h16_index((int)m, c, rows * P)] = c < C ? (_Float16)obs[(r * C + c) * P + p] : (_Float16)0.f;
    }
}

template <int S>
__global__ __launch_bounds__(256) void k_bits_to_rows_h(const uint32_t* __restrict__ bits, const int32_t* __restrict__ row_slot,
                                                        _Float16* __restrict__ x0, int rows, int C, int W) {
    // one thread = one 16-B chunk (8 channels of one row) of the chunk-major tensor; consecutive threads walk a chunk plane, so the
    // stores are contiguous (round 2 wrote 2-B elements scattered over the planes: 97 us per 16 k leaves, now ~25)
    constexpr int P = S * S;
    const size_t M = (size_t)rows * P, total = M * 8;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int cp = (int)(i / M);
        const size_t m = i - (size_t)cp * M;
        h8 o = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
        if (cp * 8 < C) {
            const size_t r = m / P;
            const int p = (int)(m - r * P);
            const uint32_t* base = bits + (size_t)row_slot[r] * W;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = cp * 8 + e, k = c * P + p;
                if (c < C) o[e] = (_Float16)(float)((base[k >> 5] >> (k & 31)) & 1u);
            }
        }
        *reinterpret_cast<h8*>(x0 + (i << 3)) = o;                       // h16_index(m, cp * 8, M) = (cp * M + m) * 8
    }
}

// fp16 head conv (F -> 16 couts: value/ownership and policy convs with their BNs folded, model.py:65-76): out[m][16] = relu(acc +
// bias) in f32 for k_heads.  One 16-cout tile makes this an LDS-read-bound kernel (one B fragment per MFMA), not an MFMA-bound
// one: the 9 A fragments of a 32-channel slice live in registers, slabs and the slice's 9-KB weight block are double-buffered
// LDS-DMA targets, one barrier per slice.  Same slab image, swizzle and masking as k_conv3x3_h2.
template <int S, int F>
__global__ __launch_bounds__(256, 2) void k_head_h(const _Float16* __restrict__ in, float* __restrict__ out,
                                                   const _Float16* __restrict__ Wh, const float* __restrict__ bias, int M) {
    constexpr int P = S * S, HALO = S + 1, KC = 32, NW = 4, NPT = 4, TM = 64 * NW, NCHK = 4, RPP = 16;
    constexpr int NSL = F / KC, NROW = TM + 2 * HALO, PLR = (NROW + 63) / 64 * 64, NXP = NCHK * (PLR / 64), NXQ = (NXP + NW - 1) / NW;
    static_assert(RPP == 16, "weight pieces are 16 couts x 64 B");
    __shared__ __attribute__((aligned(16))) _Float16 xs[2][NCHK * PLR * 8];      // chunk-major slab image (see h16_index)
    __shared__ __attribute__((aligned(16))) _Float16 wsl[2][9 * 16 * KC];
    __shared__ __attribute__((aligned(16))) float zrow[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, kq = lane >> 4;
    const int m0 = blockIdx.x * TM;
    if (tid < 4) zrow[tid] = 0.f;
    const u32x4 rin = tg_rsrc(in, (unsigned)M * F * 2);
    const int prow = lane / NCHK, pchk = lane % NCHK;
    const int lane_w = prow * KC + (pchk ^ swz64(prow)) * 8;
    auto dma = [&](int sl) {                                              // slab and weight block of slice sl
#pragma unroll
        for (int i = 0; i < NXQ; ++i) {
            const int q = wave * NXQ + i;
            if (q < NXP) {                                               // wave-uniform: a piece = 64 rows x 16 B of one chunk plane
                const int plane = q / (PLR / 64), rg = q % (PLR / 64);
                const int voff = (((sl * NCHK + plane) * M + m0 - HALO + rg * 64) * 8) * 2 + lane * 16;
                tg_dma_buffer(rin, voff, (tg_lds_void*)(&xs[sl & 1][(plane * PLR + rg * 64) * 8]));
            }
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
            if (tap % NW == wave)                                        // one 1-KB piece per tap: 16 couts x 32 channels
                tg_dma_global(Wh + ((size_t)sl * 9 + tap) * 16 * KC, lane_w * 2, (tg_lds_void*)(&wsl[sl & 1][tap * 512]));
    };
    unsigned vmask[NPT]; int vrow[NPT];
#pragma unroll
    for (int t = 0; t < NPT; ++t) {
        const int m = m0 + (wave * NPT + t) * 16 + j;
        unsigned mk = 0;
        if (m < M) {
            const int p = m % P, x = p % S, y = p / S;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                if (yy >= 0 && yy < S && xx >= 0 && xx < S) mk |= 1u << tap;
            }
        }
        vmask[t] = mk; vrow[t] = (wave * NPT + t) * 16 + j + HALO;
    }
    const int aoff = j * KC + ((kq ^ swz64(j)) << 3);
    const int nx_mine = NXP - wave * NXQ < 0 ? 0 : NXP - wave * NXQ > NXQ ? NXQ : NXP - wave * NXQ;
    const int cnt_mine = nx_mine + (wave == 0 ? 3 : 2);                  // DMA instructions this wave issues per slice (taps w, w+4, w+8 < 9)
    f32x4 acc[NPT];
#pragma unroll
    for (int t = 0; t < NPT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    dma(0);
    if (NSL > 1) dma(1);
#pragma unroll 1
    for (int sl = 0; sl < NSL; ++sl) {
        // slice sl must have landed; the only younger DMAs of this wave are its pieces of slice sl+1
        if (sl + 1 < NSL) vmcnt_uniform<NXQ + 3>(cnt_mine); else TG_VMCNT(0);
        TG_BARRIER();
        f32x4 a[9];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) a[tap] = *reinterpret_cast<const f32x4*>(wsl[sl & 1] + tap * 512 + aoff);
        const _Float16* base = xs[sl & 1];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int toff = (tap / 3 - 1) * S + (tap % 3 - 1);
#pragma unroll
            for (int t = 0; t < NPT; ++t) {
                const int R = vrow[t] + toff;
                const _Float16* src = ((vmask[t] >> tap) & 1) ? base + ((kq * PLR + R) << 3) : reinterpret_cast<const _Float16*>(zrow);
                const f32x4 b = *reinterpret_cast<const f32x4*>(src);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a[tap]), __builtin_bit_cast(h8, b), acc[t], 0, 0, 0);
            }
        }
        TG_BARRIER();                                     // every wave is done with buffers sl & 1
        if (sl + 2 < NSL) dma(sl + 2);
    }
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + kq * 4);
#pragma unroll
    for (int t = 0; t < NPT; ++t) {
        const int m = m0 + (wave * NPT + t) * 16 + j;
        if (m < M) {
            f32x4 v = acc[t] + bv;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
            *reinterpret_cast<f32x4*>(out + (size_t)m * 16 + kq * 4) = v;
        }
    }
}

// ---- head conv (F -> the 6 real couts of the 16-wide head tensor: value/ownership conv 2 + policy conv 4, model.py:65-76) --------
// As an implicit GEMM a 6-cout conv fills 6 of the 16 columns of an MFMA tile: 0.44 ms per 16 k leaves at 9x9 / F = 128, a third of
// it useful.  Here it is "GEMM, then col2im": every INPUT row m is multiplied once by all 9 taps' weights,
//     D[m][tap*6 + co] = sum_c act(x[m][c]) * W[tap][co][c]          (54 useful of 64 columns = 4 MFMA N-tiles),
// and an output is out[p][co] = relu(bias[co] + sum_tap D[p + off(tap)][tap*6 + co]) over the taps that stay on the board.  MFMAs
// per output row: 4 N-tiles x F/4 steps x (1 + halo share) instead of 9 taps x F/4 -- 10.7 vs 18 per row at 9x9 / F = 128.
// No LDS operand staging and no barrier in the GEMM phase: a wave keeps its B fragments (the whole 64 x F weight matrix at F <= 128,
// two N-tiles per pass above) in registers and streams A fragments (16 rows x 64 B of the row-major stream) straight from L2, the
// next row tile's in flight while this one computes; D goes to LDS (row stride 68 floats: the four 16-lane groups of a store hit
// disjoint banks) for the col2im pass.  Workgroups walk the tile list (at F <= 128 the weights are fetched once per wave).  PRO: the
// input is the residual stream and relu(bn_end(.)) is applied to the A fragments in registers (rows outside the batch stay zero).
template <int S, int F, bool PRO>
__global__ __launch_bounds__(256, 2) void k_head_gemm(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ W2,
                                                      const float* __restrict__ bias, const float* __restrict__ ps,
                                                      const float* __restrict__ pt, int M, int ntiles) {
    constexpr int P = S * S, HALO = S + 1, NTW = S == 9 ? 3 : 4, NROW = 64 * NTW, TM = NROW - 2 * HALO, LDW = 68, NK = F / 16;
    constexpr int NTP = F <= 128 ? 4 : 2, NPASS = 4 / NTP;               // N-tiles whose B fragments a wave holds at once
    constexpr bool DBUF = F <= 128;                                     // room to keep the next row tile's A fragments in flight
    __shared__ __attribute__((aligned(16))) float dl[NROW * LDW];
    __shared__ __attribute__((aligned(16))) float pro[PRO ? 2 * F : 4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, kq = lane >> 4;
    if (PRO) for (int i = tid; i < F; i += 256) { pro[i] = ps[i]; pro[F + i] = pt[i]; }
    __syncthreads();
    auto load_a = [&](f32x4* a, int row) {                              // A fragments of one row tile: x[row][k16*16 + kq*4 .. +3]
        const bool ok = row >= 0 && row < M;
        const float* src = in + (size_t)(ok ? row : 0) * F + kq * 4;
#pragma unroll
        for (int k = 0; k < NK; ++k) a[k] = ok ? *reinterpret_cast<const f32x4*>(src + k * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    f32x4 bw[NTP][NK];                                                  // B fragments: W2[n = nt*16 + j][k16*16 + kq*4 .. +3]
    auto load_b = [&](int pass) {
#pragma unroll
        for (int nt = 0; nt < NTP; ++nt)
#pragma unroll
            for (int k = 0; k < NK; ++k)
                bw[nt][k] = *reinterpret_cast<const f32x4*>(W2 + (size_t)((pass * NTP + nt) * 16 + j) * F + k * 16 + kq * 4);
    };
    if (NPASS == 1) load_b(0);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int m0 = tile * TM, r0 = m0 - HALO;
#pragma unroll 1
        for (int pass = 0; pass < NPASS; ++pass) {
            if (NPASS > 1) load_b(pass);
            f32x4 a[DBUF ? 2 : 1][NK];
            load_a(a[0], r0 + (wave * NTW) * 16 + j);
#pragma unroll
            for (int i = 0; i < NTW; ++i) {
                const int rt = wave * NTW + i, row = r0 + rt * 16 + j;
                f32x4* cur = a[DBUF ? (i & 1) : 0];
                if (DBUF && i + 1 < NTW) load_a(a[(i + 1) & 1], row + 16);
                const bool ok = row >= 0 && row < M;
                f32x4 acc[NTP];
#pragma unroll
                for (int nt = 0; nt < NTP; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
                int po = kq * 4;                                        // opaque per row tile: the scale / shift reads stay inside the loop
                asm volatile("" : "+v"(po));                            // (hoisted they are 2 * F / 4 registers per lane: spills at F = 256)
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    f32x4 v = cur[k];
                    if (PRO) {
                        const f32x4 sc = *reinterpret_cast<const f32x4*>(pro + k * 16 + po), sh = *reinterpret_cast<const f32x4*>(pro + F + k * 16 + po);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { float u = v[e] * sc[e] + sh[e]; u = u > 0.f ? u : 0.f; v[e] = ok ? u : 0.f; }
                    }
#pragma unroll
                    for (int nt = 0; nt < NTP; ++nt)
#pragma unroll
                        for (int s4 = 0; s4 < 4; ++s4) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[s4], bw[nt][k][s4], acc[nt], 0, 0, 0);
                }
                // D tile: row = A's M index = kq*4 + r, column = B's N index = j
#pragma unroll
                for (int nt = 0; nt < NTP; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dl[(rt * 16 + kq * 4 + r) * LDW + (pass * NTP + nt) * 16 + j] = acc[nt][r];
                if (!DBUF && i + 1 < NTW) load_a(a[0], row + 16);
            }
        }
        __syncthreads();
        for (int idx = tid; idx < TM * 8; idx += 256) {
            const int o = idx >> 3, co = idx & 7, m = m0 + o;
            if (m >= M) continue;
            float v = 0.f;
            if (co < 6) {
                const int p = m % P, x = p % S, y = p / S;
                v = bias[co];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
                    if (y + dy >= 0 && y + dy < S && x + dx >= 0 && x + dx < S) v += dl[(o + HALO + dy * S + dx) * LDW + tap * 6 + co];
                }
                v = v > 0.f ? v : 0.f;
            }
            out[(size_t)m * 16 + co] = v;
        }
        __syncthreads();
    }
}

// the head conv's weights for k_head_gemm: dst[n = tap*6 + co][c] = w[tap][co][c] for co < 6 (w is [9][16][F]), rows 54..63 zero
__global__ __launch_bounds__(256) void k_restage_head(const float* __restrict__ w, float* __restrict__ dst, int F) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 64 * F; i += gridDim.x * 256) {
        const int n = i / F, c = i % F;
        dst[i] = n < 54 ? w[((size_t)(n / 6) * 16 + n % 6) * F + c] : 0.f;
    }
}

// The same head conv for the split-precision chain (net_precision 3, F = 128): the GEMM runs on v_mfma_f32_16x16x32_f16 with the
// activation rows taken from the split chunk-major conv input the last residual block wrote (relu(bn_end(x)) as fp16 hi | lo:
// a lane's A fragment of a 16-channel group is ONE 16-B load, chunk plane g*4 + kq) and the weights as [w_hi | w_hi] and
// [w_lo | w_lo] fragments in registers (dst of k_restage_head_split, scaled by a power of two): two K = 32 steps per (group,
// N-tile) give all four partial products of (w_hi + w_lo)(a_hi + a_lo) -- a quarter of the f32 kernel's MFMA time, so the kernel
// is bound by the 512 B per row it reads.  A wave holds the B fragments of two N-tiles (128 registers) for the whole kernel;
// D through LDS and col2im as in k_head_gemm, the power-of-two scale undone there (exact).
template <int S, int F>
__global__ __launch_bounds__(256, 2) void k_head_gemm_x2(const _Float16* __restrict__ in, float* __restrict__ out, const _Float16* __restrict__ W2,
                                                         const float* __restrict__ wsc_p, const float* __restrict__ bias, int M, int ntiles) {
    constexpr int P = S * S, HALO = S + 1, NTW = S == 9 ? 3 : 4, NROW = 64 * NTW, TM = NROW - 2 * HALO, LDW = 68, NG = F / 16;
    constexpr int NTP = 2;                                                
    __shared__ __attribute__((aligned(16))) float dl[NROW * LDW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, kq = lane >> 4;
    const float wsc = wsc_p[0];
    auto load_a = [&](f32x4* a, int row) {                              // group g: 8 halfs = chunk plane g*4 + kq of row `row`
        const bool ok = row >= 0 && row < M;
        const _Float16* src = in + ((size_t)kq * M + (ok ? row : 0)) * 8;
#pragma unroll
        for (int g = 0; g < NG; ++g) a[g] = ok ? *reinterpret_cast<const f32x4*>(src + (size_t)g * 4 * M * 8) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    f32x4 bh[NTP][NG], bl[NTP][NG];                                     // B fragments of column n = nt*16 + j: hi and lo halves
    auto load_b = [&](int pass) {
#pragma unroll
        for (int nt = 0; nt < NTP; ++nt)
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const _Float16* w = W2 + ((size_t)((pass * NTP + nt) * 16 + j) * NG + g) * 32;
                bh[nt][g] = *reinterpret_cast<const f32x4*>(w + (kq & 1) * 8);
                bl[nt][g] = *reinterpret_cast<const f32x4*>(w + 16 + (kq & 1) * 8);
            }
    };
    // waves 0, 1 take N-tiles {0, 1}, waves 2, 3 take {2, 3}: a wave's B fragments are loaded ONCE per kernel; the two waves of a
    // pair split the row tiles of a tile between them (every row tile is read by one wave of each pair)
    const int nh = wave >> 1, wr = wave & 1;
    load_b(nh);
    constexpr int RTW = 2 * NTW;                                        // row tiles per wave
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int m0 = tile * TM, r0 = m0 - HALO;
        {
            const int pass = nh;
            f32x4 cur[NG];                                              // one buffer: the next row tile is requested right behind this one's
            load_a(cur, r0 + (wr * RTW) * 16 + j);                      // MFMAs and lands while its D tile goes to LDS (128 registers are
#pragma unroll 1                                                         // the weights': a second A buffer spills)
            for (int i = 0; i < RTW; ++i) {
                const int rt = wr * RTW + i, row = r0 + rt * 16 + j;
                f32x4 acc[NTP];
#pragma unroll
                for (int nt = 0; nt < NTP; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int nt = 0; nt < NTP; ++nt) {
                        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, cur[g]), __builtin_bit_cast(h8, bh[nt][g]), acc[nt], 0, 0, 0);
                        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, cur[g]), __builtin_bit_cast(h8, bl[nt][g]), acc[nt], 0, 0, 0);
                    }
                __builtin_amdgcn_sched_barrier(0);
                if (i + 1 < RTW) load_a(cur, row + 16);
                // D tile: row = A's M index = kq*4 + r, column = B's N index = j
#pragma unroll
                for (int nt = 0; nt < NTP; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dl[(rt * 16 + kq * 4 + r) * LDW + (pass * NTP + nt) * 16 + j] = acc[nt][r];
            }
        }
        __syncthreads();
        for (int idx = tid; idx < TM * 8; idx += 256) {
            const int o = idx >> 3, co = idx & 7, m = m0 + o;
            if (m >= M) continue;
            float v = 0.f;
            if (co < 6) {
                const int p = m % P, x = p % S, y = p / S;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
                    if (y + dy >= 0 && y + dy < S && x + dx >= 0 && x + dx < S) v += dl[(o + HALO + dy * S + dx) * LDW + tap * 6 + co];
                }
                v = v * wsc + bias[co];
                v = v > 0.f ? v : 0.f;
            }
            out[(size_t)m * 16 + co] = v;
        }
        __syncthreads();
    }
}

// its weights: dst[n = tap*6 + co][group of 16 channels][w_hi 16 | w_lo 16] of w * 2^s (w is [9][16][F]; rows 54..63 zero; s puts the
// largest weight in [2^14, 2^15) like k_restage_split); wsc_out = 2^-s
__global__ __launch_bounds__(256) void k_restage_head_split(const float* __restrict__ w, _Float16* __restrict__ dst, float* __restrict__ wsc_out,
                                                            const unsigned* __restrict__ maxbits, int F) {
    const unsigned mb = maxbits[0];
    int sh = mb ? 14 - ((int)((mb >> 23) & 0xffu) - 127) : 0;
    sh = sh < -60 ? -60 : sh > 60 ? 60 : sh;
    const float scale = ldexpf(1.f, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) wsc_out[0] = ldexpf(1.f, -sh);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 64 * F; i += gridDim.x * 256) {
        const int n = i / F, c = i % F, g = c >> 4, e = c & 15;
        const float v = n < 54 ? w[((size_t)(n / 6) * 16 + n % 6) * F + c] * scale : 0.f;
        const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
        _Float16* d = dst + ((size_t)n * (F / 16) + g) * 32;
        d[e] = hi; d[16 + e] = lo;
    }
}

// Self_Attention core (model.py:301-315) for one board per workgroup, after the fused q/k/v 1x1 projection:
//   energy[i][j] = q_i . k_j ; attention = softmax_j(energy) ; out[:, j] = sum_i v[:, i] * attention[i][j]   (note: summed over
//   the softmaxed ROW index i, exactly as torch.bmm(proj_value, attention) does)
//   y = relu(bn(gamma * out + x))            -- x optionally pre-activated with relu(x*ps+pt) (policy head, model.py:94,106)
template <int S, int F>
__global__ __launch_bounds__(256) void k_attention(const float* __restrict__ qkv, const float* __restrict__ xin,
                                                   float* __restrict__ out, const float* __restrict__ gamma,
                                                   const float* __restrict__ bs, const float* __restrict__ bt,
                                                   const float* __restrict__ ps, const float* __restrict__ pt) {
    constexpr int P = S * S, FQ = F / 4, W = 2 * FQ + F;
    extern __shared__ float sm[];
    float* q = sm;                    // [P][W] rows: q | k | v
    float* at = sm + P * W;           // [P][P+1]
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* src = qkv + (size_t)b * P * W;
    for (int i = tid; i < P * W / 4; i += 256) reinterpret_cast<f32x4*>(q)[i] = reinterpret_cast<const f32x4*>(src)[i];
    __syncthreads();
    for (int e = tid; e < P * P; e += 256) {
        const int i = e / P, j = e % P;
        const float* qi = q + i * W; const float* kj = q + j * W + FQ;
        float a = 0.f;
        for (int c = 0; c < FQ; ++c) a = fmaf(qi[c], kj[c], a);
        at[i * (P + 1) + j] = a;
    }
    __syncthreads();
    for (int i = tid; i < P; i += 256) {
        float* r = at + i * (P + 1);
        float mx = r[0];
        for (int j = 1; j < P; ++j) mx = r[j] > mx ? r[j] : mx;
        float sum = 0.f;
        for (int j = 0; j < P; ++j) { float e = expf(r[j] - mx); r[j] = e; sum += e; }
        const float inv = 1.f / sum;
        for (int j = 0; j < P; ++j) r[j] *= inv;
    }
    __syncthreads();
    const float g = gamma[0];
    for (int e = tid; e < P * F; e += 256) {
        const int j = e / F, c = e % F;
        float a = 0.f;
        for (int i = 0; i < P; ++i) a = fmaf(q[i * W + 2 * FQ + c], at[i * (P + 1) + j], a);
        float x = xin[((size_t)b * P + j) * F + c];
        if (ps) { x = x * ps[c] + pt[c]; x = x > 0.f ? x : 0.f; }
        float y = (g * a + x) * bs[c] + bt[c];
        out[((size_t)b * P + j) * F + c] = y > 0.f ? y : 0.f;
    }
}

// one butterfly step of a reduction over the 16 lanes of a DPP row (= the 16 columns j of one lane group kq), without LDS traffic:
// steps 0, 1 exchange within quads (lane ^ 1, lane ^ 2); steps 2, 3 mirror the half row / the row, which pairs quad with quad and
// half with half -- the values are uniform within those by then, so the result equals the xor butterfly's, in the same order
__device__ __forceinline__ float row16_step(float v, int step) {
    const int x = __builtin_bit_cast(int, v);
    int r;
    switch (step) {
        case 0: r = __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false); break;      // quad_perm [1,0,3,2]
        case 1: r = __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xf, 0xf, false); break;      // quad_perm [2,3,0,1]
        case 2: r = __builtin_amdgcn_update_dpp(x, x, 0x141, 0xf, 0xf, false); break;     // row_half_mirror
        default: r = __builtin_amdgcn_update_dpp(x, x, 0x140, 0xf, 0xf, false); break;    // row_mirror
    }
    return __builtin_bit_cast(float, r);
}
// The same Self_Attention core on the matrix cores (F = 64, 128, 256 at 9x9): ONE WAVE PER BOARD, everything between the q/k/v
// projection and the block's output stays in registers.
//   GEMM 1  energy[i][j] = sum_c q[i][c] k[j][c]        (P x P x F/4; 6 x 6 tiles of 16 x 16, P = 81 padded to 96)
//   softmax over j, row by row, on the accumulator tiles themselves (a row lives in 16 lanes x 6 tiles: in-register max/sum
//           + 4 xor-shuffles); padded columns are excluded, padded rows zeroed
//   GEMM 2  out[c][j] = sum_i v[i][c] attention[i][j]   (F x P x P).  The D layout of a 16x16x4 MFMA tile (column = lane & 15,
//           row = 4*(lane >> 4) + r) IS the B-operand layout with k = 4*(lane >> 4) + s, so the softmaxed tiles feed GEMM 2
//           without leaving their registers; only v is loaded (each element once, 64-B runs).  i = 81 needs 21 k-steps, not 24.
//   y = relu(bn(gamma * out + x)), written row-major (the residual stream) and, when the next layer is a residual block of the
//   DMA-fed chain, also as its pre-activated slice-major input relu(bn1_next(y)) (out2).
// MFMA work per board: 288 + 1008 instructions of 16x16x4 (F = 128) = 1.3 % of an F->F conv's; the scalar-FMA kernel above took
// 8.3 ms per 16384 boards (3 x an F->F conv), this one is bounded by its 97 KB of q/k/v/x/y traffic per board.
// X2O: out2 is the split-precision chain's conv input instead -- fp16 hi + lo of relu(bn1_next(y)), chunk-major (x2_index).
template <int S, int F, int CP, bool X2O = false>
__global__ __launch_bounds__(256, 1) void k_attention_mfma(const float* __restrict__ qkv, const float* __restrict__ xin,
                                                        float* __restrict__ out, float* __restrict__ out2,
                                                        const float* __restrict__ gamma, const float* __restrict__ bs,
                                                        const float* __restrict__ bt, const float* __restrict__ ps,
                                                        const float* __restrict__ pt, const float* __restrict__ s2,
                                                        const float* __restrict__ t2, int rows, unsigned* __restrict__ ovf = nullptr) {
    constexpr int P = S * S, FQ = F / 4, W = 2 * FQ + F, NT = (P + 15) / 16, CT = F / 16, NSUB = FQ / 16;
    static_assert(P <= 96 && FQ % 16 == 0 && CT % CP == 0, "attention tile geometry");
    float amax = 0.f;                                                                // X2O: range guard of the fp16 copies (see conv_epilogue_h8)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    if (b >= rows) return;
    const int j = lane & 15, kq = lane >> 4;
    const float* base = qkv + (size_t)b * P * W;
    const int M = rows * P;
    // ---- GEMM 1 ----
    f32x4 e[NT][NT];
#pragma unroll
    for (int tm = 0; tm < NT; ++tm)
#pragma unroll
        for (int tn = 0; tn < NT; ++tn) e[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
        // padded rows (>= P) repeat the last one; their columns / rows are masked below.  k fragments of the slice stay resident,
        // q fragments stream through one register quad (one ahead), so the 36 energy tiles dominate the register budget
        auto row_of = [&](int t) { return t * 16 + j < P ? t * 16 + j : P - 1; };
        f32x4 kb[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) kb[t] = *reinterpret_cast<const f32x4*>(base + (size_t)row_of(t) * W + FQ + sub * 16 + kq * 4);
        f32x4 qa = *reinterpret_cast<const f32x4*>(base + (size_t)row_of(0) * W + sub * 16 + kq * 4);
#pragma unroll
        for (int tm = 0; tm < NT; ++tm) {
            f32x4 qn = qa;
            if (tm + 1 < NT) qn = *reinterpret_cast<const f32x4*>(base + (size_t)row_of(tm + 1) * W + sub * 16 + kq * 4);
#pragma unroll
            for (int tn = 0; tn < NT; ++tn)
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4)
                    e[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[s4], kb[tn][s4], e[tm][tn], 0, 0, 0);
            qa = qn;
        }
    }
    // ---- softmax over j (columns) for every row i = tm*16 + kq*4 + r ----
#pragma unroll
    for (int tm = 0; tm < NT; ++tm) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mx = -INFINITY;
#pragma unroll
            for (int tn = 0; tn < NT; ++tn) if (tn * 16 + j < P) mx = e[tm][tn][r] > mx ? e[tm][tn][r] : mx;
#pragma unroll
            for (int o = 0; o < 4; ++o) { const float t = row16_step(mx, o); mx = t > mx ? t : mx; }   // DPP: no LDS round trips
            float sum = 0.f;
#pragma unroll
            for (int tn = 0; tn < NT; ++tn) {
                const float v = tn * 16 + j < P ? __expf(e[tm][tn][r] - mx) : 0.f;        // v_exp_f32: ~1e-7 relative, tolerance is 1e-3
                e[tm][tn][r] = v; sum += v;
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) sum += row16_step(sum, o);
            const float inv = (tm * 16 + kq * 4 + r < P) ? 1.f / sum : 0.f;     // rows past the board contribute nothing to GEMM 2
#pragma unroll
            for (int tn = 0; tn < NT; ++tn) e[tm][tn][r] *= inv;
        }
    }
    // ---- GEMM 2 + epilogue, CP channel tiles per pass ----
    // One wave per SIMD (the 36 energy tiles alone are 144 registers), so latency is hidden inside the wave: ALL v operands of a
    // pass (NK k-steps x CP tiles, 4 B each) are requested while the previous pass computes -- with one step of lead the kernel
    // sat on load latency (84 dependent round trips per board, 1.14 ms per 16384 boards).
    const float g = gamma[0];
    const float* vb = base + 2 * FQ;
    constexpr int LASTS = P - (NT - 1) * 16, NS_LAST = LASTS < 4 ? LASTS : 4, NK = (NT - 1) * 4 + NS_LAST, NPASS = CT / CP;
    // k-step kk covers rows i = (kk/4)*16 + kq*4 + kk%4; of the last 16-row block only the steps that touch a row < P exist
    float av[2][NK][CP];
    auto load_pass = [&](int pass, float (*dst)[CP]) {
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) {
            const int i = (kk >> 2) * 16 + kq * 4 + (kk & 3);
            const int ic = i < P ? i : P - 1;                                         // the matching attention rows are zero
#pragma unroll
            for (int cp = 0; cp < CP; ++cp) dst[kk][cp] = vb[(size_t)ic * W + (pass * CP + cp) * 16 + j];
        }
    };
    load_pass(0, av[0]);
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
        const int c0 = pass * CP;
        if (pass + 1 < NPASS) load_pass(pass + 1, av[(pass + 1) & 1]);
        f32x4 acc[CP][NT];
#pragma unroll
        for (int cp = 0; cp < CP; ++cp)
#pragma unroll
            for (int tn = 0; tn < NT; ++tn) acc[cp][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the pass's residual rows are requested BEFORE its MFMAs: they queue behind the previous pass's stores (vmcnt is in order)
        // and have the whole output GEMM to get past them; requested in the epilogue they were waited for at once
        f32x4 x[CP][NT];
#pragma unroll
        for (int cp = 0; cp < CP; ++cp)
#pragma unroll
            for (int tn = 0; tn < NT; ++tn) {
                const int p = tn * 16 + j < P ? tn * 16 + j : P - 1;
                x[cp][tn] = *reinterpret_cast<const f32x4*>(xin + (size_t)(b * P + p) * F + (c0 + cp) * 16 + kq * 4);
            }
        // ... and so are the pass's per-channel parameters (at F = 256 the split-output variant has no registers left for that:
        // there the parameters are fetched behind the MFMAs, as before)
        constexpr bool PARAMS_EARLY = !(X2O && F > 128);
        f32x4 vbs[CP], vbt[CP], vps[CP], vpt[CP], vs2[CP], vt2[CP];
        auto load_params = [&]() {
#pragma unroll
        for (int cp = 0; cp < CP; ++cp) {
            const int c = (c0 + cp) * 16 + kq * 4;
            vbs[cp] = *reinterpret_cast<const f32x4*>(bs + c); vbt[cp] = *reinterpret_cast<const f32x4*>(bt + c);
            vps[cp] = f32x4{1.f, 1.f, 1.f, 1.f}; vpt[cp] = f32x4{0.f, 0.f, 0.f, 0.f}; vs2[cp] = vps[cp]; vt2[cp] = vpt[cp];
            if (ps) { vps[cp] = *reinterpret_cast<const f32x4*>(ps + c); vpt[cp] = *reinterpret_cast<const f32x4*>(pt + c); }
            if (out2) { vs2[cp] = *reinterpret_cast<const f32x4*>(s2 + c); vt2[cp] = *reinterpret_cast<const f32x4*>(t2 + c); }
        }
        };
        if constexpr (PARAMS_EARLY) load_params();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < NK; ++kk)
#pragma unroll
            for (int cp = 0; cp < CP; ++cp)
#pragma unroll
                for (int tn = 0; tn < NT; ++tn)
                    acc[cp][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[pass & 1][kk][cp], e[kk >> 2][tn][kk & 3], acc[cp][tn], 0, 0, 0);
        // D tile: row = channel (c0+cp)*16 + kq*4 + r, column = position tn*16 + j
        if constexpr (!PARAMS_EARLY) load_params();
#pragma unroll
        for (int cp = 0; cp < CP; ++cp) {
            const int c = (c0 + cp) * 16 + kq * 4;
#pragma unroll
            for (int tn = 0; tn < NT; ++tn) {
                const int p = tn * 16 + j;
                if (p >= P) continue;
                const int m = b * P + p;
                f32x4 y, u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float xv = x[cp][tn][q];
                    if (ps) { xv = xv * vps[cp][q] + vpt[cp][q]; xv = xv > 0.f ? xv : 0.f; }
                    const float w = (g * acc[cp][tn][q] + xv) * vbs[cp][q] + vbt[cp][q];
                    y[q] = w > 0.f ? w : 0.f;
                    const float z = y[q] * vs2[cp][q] + vt2[cp][q];
                    u[q] = z > 0.f ? z : 0.f;
                }
                *reinterpret_cast<f32x4*>(out + (size_t)m * F + c) = y;
                if constexpr (X2O) {
                    if (out2) {
                        h4 hi, lo;
#pragma unroll
                        for (int q = 0; q < 4; ++q) { hi[q] = (_Float16)u[q]; lo[q] = (_Float16)(u[q] - (float)hi[q]); amax = __builtin_fmaxf(amax, u[q]); }
                        _Float16* const o16 = reinterpret_cast<_Float16*>(out2);
                        const int c2 = x2_index(c);
                        *reinterpret_cast<h4*>(o16 + h16_index(m, c2, M)) = hi;
                        *reinterpret_cast<h4*>(o16 + h16_index(m, c2 + 16, M)) = lo;
                    }
                } else {
                    if (out2) *reinterpret_cast<f32x4*>(out2 + f32_sm_index(conv_sg_row(b, p, P), c, conv_sg_rows(rows, P))) = u;
                }
            }
        }
    }
    if constexpr (X2O) {
        if (__builtin_amdgcn_ballot_w64(!(amax <= 65504.f)) != 0 && lane == 0) atomicAdd(ovf, 1u);
    }
}

// The Self_Attention core TILED, for 19x19 (P = 361 = 22 tiles of 16 + 9 positions; F = 128, 256), exact f32 on the 16x16x4 MFMA:
// ONE WORKGROUP (4 waves) PER BOARD.  The P x P energy matrix (521 KB) never exists; because the softmax normalises the index that
// GEMM 2 SUMS over (see k_attention), no online rescaling is needed, but the row statistics must be complete before the first
// output column is formed -- two passes over the energies:
//   stage    k of the board into LDS, in B-fragment order [j tile][16-channel slice][lane] (one conflict-free 16-B read per lane and
//            slice; rows >= P zero).  q is read from memory as A fragments (an i tile's are FQ/4 registers), v is streamed.
//   pass 1   wave w takes the i tiles w, w+4, ..: the 23 energy tiles of the tile row in registers, m_i = max_j e_ij and
//            1 / sum_j exp(e_ij - m_i) over the columns j < P (in-register + DPP row reduction, as k_attention_mfma), two floats per
//            row into LDS; rows >= P get 1/l = 0.
//   pass 2   for each i tile: the four waves recompute a quarter of the tile row each (bit-identical energies: same MFMA order),
//            p_ij = exp(e_ij - m_i) / l_i (0 in padded rows and columns), and park the tiles in LDS AS THEY LIE in the D layout,
//            which is the B-operand layout of GEMM 2 -- 16 B per lane, written and read back without conflicts (two buffers of
//            23 KB, one barrier per i tile).  Every wave then feeds all 23 tiles to out[c][j] += v[i][c] p_ij for ITS 32 channels
//            (2 channel tiles x 23 j tiles = 184 accumulator registers; the channels are split over the waves and, at F = 256,
//            over two such sweeps, the second of which recomputes the probabilities).  v: 4 B per lane and k-step, 64-B runs, each
//            element read once per board, requested one i tile ahead.
//   epilogue y = relu(bn(gamma * out + x)) row-major and, for a residual block of the DMA-fed chain that follows, relu(bn1_next(y))
//            slice-major in board-grouped rows (out2), exactly as k_attention_mfma<.., false> writes them.
// MFMA instructions per board: F = 128 4232 (pass 1) + 4232 + 16928 (pass 2); F = 256 8464 + 2 x (8464 + 16928).
// Resources (gfx950, scratch 0, one wave per SIMD): F = 128 234 VGPRs + 188 AGPRs, 97 152 B of dynamic LDS (k 47 104, tiles 47 104,
// statistics 2 944); F = 256 256 VGPRs + 254 AGPRs, 144 256 B (k 94 208).
template <int S, int F> constexpr int att_t_lds() {
    constexpr int NT = (S * S + 15) / 16;
    return (int)sizeof(float) * (4 * 64 * (NT * (F / 64) + 2 * NT) + 2 * NT * 16);
}
template <int S, int F>
__global__ __launch_bounds__(256, 1) void k_attention_t(const float* __restrict__ qkv, const float* __restrict__ xin,
                                                     float* __restrict__ out, float* __restrict__ out2,
                                                     const float* __restrict__ gamma, const float* __restrict__ bs,
                                                     const float* __restrict__ bt, const float* __restrict__ ps,
                                                     const float* __restrict__ pt, const float* __restrict__ s2,
                                                     const float* __restrict__ t2, int rows) {
    constexpr int P = S * S, FQ = F / 4, W = 2 * FQ + F, NT = (P + 15) / 16, NSUB = FQ / 16, CT = F / 16, CPW = 2, NPASS = CT / (4 * CPW);
    static_assert(FQ % 16 == 0 && CT % (4 * CPW) == 0, "attention tile geometry");
    extern __shared__ float sm[];
    f32x4* const kl = reinterpret_cast<f32x4*>(sm);                 // [NT][NSUB][64 lanes]: k as B fragments
    f32x4* const pl = kl + NT * NSUB * 64;                          // [2][NT][64 lanes]: the probability tiles of one i tile
    float* const rm = reinterpret_cast<float*>(pl + 2 * NT * 64);   // [NT * 16] row maxima
    float* const ri = rm + NT * 16;                                 // [NT * 16] 1 / row sums, 0 in the padded rows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x;
    if (b >= rows) return;
    const float* base = qkv + (size_t)b * P * W;
    for (int e = threadIdx.x; e < NT * 16 * (FQ / 4); e += 256) {
        const int p = e / (FQ / 4), c4 = e % (FQ / 4);              // position, quad of channels: slice c4 >> 2, k group c4 & 3
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p < P) v = *reinterpret_cast<const f32x4*>(base + (size_t)p * W + FQ + c4 * 4);
        kl[((p >> 4) * NSUB + (c4 >> 2)) * 64 + (c4 & 3) * 16 + (p & 15)] = v;
    }
    __syncthreads();
    // A fragments of q for the i tile `it` (padded rows repeat the last one; their probabilities are zeroed), and one energy tile
    auto load_q = [&](int it, f32x4 (&qa)[NSUB]) {
        const int row = it * 16 + j < P ? it * 16 + j : P - 1;
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) qa[sub] = *reinterpret_cast<const f32x4*>(base + (size_t)row * W + sub * 16 + kq * 4);
    };
    auto energy = [&](const f32x4 (&qa)[NSUB], int jt) {
        f32x4 e = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const f32x4 kb = kl[(jt * NSUB + sub) * 64 + lane];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) e = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[sub][s4], kb[s4], e, 0, 0, 0);
        }
        return e;
    };
    // ---- pass 1: row statistics.  Lane (j, kq) holds rows it*16 + kq*4 + r, columns jt*16 + j of the tile row ----
#pragma unroll 1
    for (int it = wave; it < NT; it += 4) {
        f32x4 qa[NSUB];
        load_q(it, qa);
        f32x4 e[NT];
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) e[jt] = energy(qa, jt);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mx = -INFINITY;
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) if (jt * 16 + j < P) mx = e[jt][r] > mx ? e[jt][r] : mx;
#pragma unroll
            for (int o = 0; o < 4; ++o) { const float t = row16_step(mx, o); mx = t > mx ? t : mx; }
            float sum = 0.f;
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) sum += jt * 16 + j < P ? __expf(e[jt][r] - mx) : 0.f;
#pragma unroll
            for (int o = 0; o < 4; ++o) sum += row16_step(sum, o);
            const int i = it * 16 + kq * 4 + r;
            if (j == 0) { rm[i] = i < P ? mx : 0.f; ri[i] = i < P ? 1.f / sum : 0.f; }
        }
    }
    __syncthreads();
    // ---- pass 2: probabilities by i tile through LDS, GEMM 2 on this wave's channels, epilogue ----
    const float g = gamma[0];
    const float* vb = base + 2 * FQ;
#pragma unroll 1
    for (int pass = 0; pass < NPASS; ++pass) {
        const int c0 = (pass * 4 + wave) * CPW;                      // first of this wave's channel tiles
        // k-step kk of i tile `it` covers row i = it*16 + kq*4 + kk (the D row of the probability tile's register kk)
        auto load_v = [&](int it, float (&dst)[CPW][4]) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int i = it * 16 + kq * 4 + kk;
                const int ic = i < P ? i : P - 1;                        // the matching probabilities are zero
#pragma unroll
                for (int cp = 0; cp < CPW; ++cp) dst[cp][kk] = vb[(size_t)ic * W + (c0 + cp) * 16 + j];
            }
        };
        f32x4 acc[CPW][NT];
#pragma unroll
        for (int cp = 0; cp < CPW; ++cp)
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) acc[cp][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
        float av[CPW][4], an[CPW][4];
        load_v(0, av);
#pragma unroll 1
        for (int it = 0; it < NT; ++it) {
            f32x4 qa[NSUB];
            load_q(it, qa);
            const f32x4 m4 = *reinterpret_cast<const f32x4*>(rm + it * 16 + kq * 4);
            const f32x4 i4 = *reinterpret_cast<const f32x4*>(ri + it * 16 + kq * 4);
            f32x4* const pb = pl + (it & 1) * NT * 64;
#pragma unroll 1
            for (int jt = wave; jt < NT; jt += 4) {
                f32x4 e = energy(qa, jt);
                const bool col = jt * 16 + j < P;
#pragma unroll
                for (int r = 0; r < 4; ++r) e[r] = col && it * 16 + kq * 4 + r < P ? __expf(e[r] - m4[r]) * i4[r] : 0.f;
                pb[jt * 64 + lane] = e;
            }
#pragma unroll
            for (int cp = 0; cp < CPW; ++cp)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) an[cp][kk] = av[cp][kk];
            if (it + 1 < NT) load_v(it + 1, an);
            // one barrier per i tile: the tiles written next go to the other buffer, which every wave finished reading before it
            // arrived here
            __syncthreads();
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) {
                const f32x4 pr = pb[jt * 64 + lane];
#pragma unroll
                for (int cp = 0; cp < CPW; ++cp)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
                        acc[cp][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[cp][kk], pr[kk], acc[cp][jt], 0, 0, 0);
            }
#pragma unroll
            for (int cp = 0; cp < CPW; ++cp)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) av[cp][kk] = an[cp][kk];
        }
        // D tile: row = channel (c0+cp)*16 + kq*4 + r, column = position jt*16 + j
#pragma unroll
        for (int cp = 0; cp < CPW; ++cp) {
            const int c = (c0 + cp) * 16 + kq * 4;
            const f32x4 one = f32x4{1.f, 1.f, 1.f, 1.f}, zero = f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4 vbs = *reinterpret_cast<const f32x4*>(bs + c), vbt = *reinterpret_cast<const f32x4*>(bt + c);
            const f32x4 vps = ps ? *reinterpret_cast<const f32x4*>(ps + c) : one, vpt = ps ? *reinterpret_cast<const f32x4*>(pt + c) : zero;
            const f32x4 vs2 = out2 ? *reinterpret_cast<const f32x4*>(s2 + c) : one, vt2 = out2 ? *reinterpret_cast<const f32x4*>(t2 + c) : zero;
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) {
                const int p = jt * 16 + j;
                if (p >= P) continue;
                const size_t m = (size_t)b * P + p;
                const f32x4 x = *reinterpret_cast<const f32x4*>(xin + m * F + c);
                f32x4 y, u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float xv = x[q];
                    if (ps) { xv = xv * vps[q] + vpt[q]; xv = xv > 0.f ? xv : 0.f; }
                    const float w = (g * acc[cp][jt][q] + xv) * vbs[q] + vbt[q];
                    y[q] = w > 0.f ? w : 0.f;
                    const float z = y[q] * vs2[q] + vt2[q];
                    u[q] = z > 0.f ? z : 0.f;
                }
                *reinterpret_cast<f32x4*>(out + m * F + c) = y;
                if (out2) *reinterpret_cast<f32x4*>(out2 + f32_sm_index(conv_sg_row(b, p, P), c, conv_sg_rows(rows, P))) = u;
            }
        }
        if (pass + 1 < NPASS) __syncthreads();                       // the next sweep starts in the buffer the last i tile used
    }
}

// Self_Attention as ONE kernel (F = 128, 9x9), one body (att_fused_block.h, included below once per precision and again behind
// k_restage_att_split) for two precisions of the q/k/v 1x1 projection: the projection is computed
// inside the per-board core on the fp16 matrix cores and never goes through memory (the two-kernel form moves 62 KB of q|k|v per
// board out and back in: at 16 k boards the pair took 0.61 + 0.70 ms, 23 % of a MainNetwork wave).
//   SPLIT   (k_attention_x3, net_precision 3) split precision: x and the weights as fp16 hi + lo, three of the four products;
//   !SPLIT  (k_attention_h, net_precision 1)  a single fp16 product: what rounds to fp16 is the projection's input (x, under PRO
//           relu(x*ps + pt)) and its weights.
// The biases, q, k, v, the energy GEMM, the softmax, the output GEMM, gamma, the residual and the block's BN are f32 in both.
//   * the layer's weights sit in LDS for the life of a persistent workgroup (one workgroup of 4 waves per CU), [NG groups][W couts]
//     [32 halfs], the 64-B rows XOR-swizzled like the conv's stage tiles; one K = 32 step of v_mfma_f32_16x16x32_f16 covers a group.
//     SPLIT: groups of 16 channels as [hi 16 | lo 16], scaled by 2^s (k_restage_att_split), 96 KB.  !SPLIT: groups of 32 channels
//     of plain fp16 (k_restage_att_half; no scale), 48 KB -- two images (57 KB each with parameters and touch scratch) would fit
//     the LDS, but the output accumulators (192 registers) and q^T / k^T (96) alone are more than the 256 registers a second wave
//     per SIMD would leave;
//   * one wave per board, as in k_attention_mfma.  x fragments are built from the f32 residual stream on the fly, from two 16-B loads
//     per lane (j, kq) of row j.  SPLIT: 8 adjacent channels of the group, of which the lane keeps the fp16 hi (kq < 2) or lo
//     (kq >= 2) halves -- the [a_hi | a_lo] operand of a K = 32 step.  !SPLIT: channels g*32 + kq*4 .. +3 and g*32 + 16 + kq*4 .. +3,
//     rounded once; the lane's K slots kq*8 + e hold those eight in that order and the image's rows are stored in the same order.
//     With that order the lane's two loads ARE its elements of the two D tiles ct = 2g, 2g + 1 of column j (row = channel
//     ct*16 + kq*4 + r): the residual goes from the row registers into the output accumulators with no shuffle (SPLIT needs 32
//     ds_bpermute per row block);
//   * phase A: q^T and k^T for the whole board, as D[c][pos] tiles -- which ARE the A / B operand layouts of the energy GEMM's f32
//     16x16x4 steps (k index = 4*(lane >> 4) + r).  A three-stage stream over the channel groups: group g on the matrix cores,
//     group g+1 being converted (VALU work in the shadow of the MFMAs), group g+2's loads in flight.  The f32 biases start the
//     accumulators (SPLIT: added behind the GEMM, with the weight scale);
//   * phase B, per block of 16 rows i (tm): v for those rows and all channels as D[pos][c] tiles -- the A operand layout of the
//     output GEMM -- from the block's x rows (second pass over x; measured, it comes from HBM again: a board's 41 KB do not survive
//     in an L2 shared by 128 boards in flight); the block's 16 x 96 energies; softmax on the accumulator tiles with DPP row
//     reductions (a row is complete within the block); out[c][j] += (gamma v)[i][c] attention[i][j] into accumulators that cover all
//     channels and also take the residual x of column tile tm in block tm (from the lines the block's row loads just fetched).
//     Nothing but those accumulators outlives a block, so the 36 energy tiles of k_attention_mfma never exist at once and x is
//     converted twice per board, not once per channel pass.
//   * epilogue: y = relu(bn(acc)) row-major and the next residual block's fp16 input (SPLIT: hi and lo planes, x2_index; !SPLIT: one
//     plane, h16_index) -- stores only (a load in here would queue behind the stores: vmcnt is in order); the next board's first two
//     groups are requested before the first store, its lines were touched towards L2 (LDS-DMA into a scratch KB) at the start of
//     phase B.
// Per board, SPLIT: 1152 K=32 fp16 steps (projection) + 1296 f32 16x16x4 steps (exact-f32 energy and output GEMMs) = 59 k cycles of
// MFMA; measured 130 k cycles per board (0.98 ms per 16 k boards; MFMA pipe 40 % busy).  !SPLIT: 288 K=32 steps (96 for q^T / k^T,
// 6 x 32 for v) + the same 1296.  PRO: x is relu(x*ps + pt) first (attention in the policy head, model.py:94,106).
// Diagnostics: -DTG_ATT_STAMP (phase stamps of the SPLIT kernel, scripts/stamp_att.py).
// NM MFMAs with KV VALU instructions (the conversion of the next group) in the shadow of each
#define TG_ATT_SCHED(NM, KV) do { _Pragma("unroll") for (int i_ = 0; i_ < (NM); ++i_) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); \
                                  __builtin_amdgcn_sched_group_barrier(0x002, (KV), 0); } __builtin_amdgcn_sched_barrier(0); } while (0)
#ifdef TG_ATT_STAMP
// diagnostic build: phase stamps (s_memtime, 100 MHz) of the third board of wave 0 of workgroup 0, SPLIT, PRO = false launches
__device__ unsigned long long g_att_stamp[32];
#define TG_ASTAMP(i) do { if constexpr (SPLIT) { __builtin_amdgcn_sched_barrier(0); if (!PRO && blockIdx.x == 0 && wave == 0 && nboard == 2 && lane == 0) g_att_stamp[i] = __builtin_readcyclecounter(); \
                          __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define TG_ASTAMP(i) do { } while (0)
#endif
#define TG_ATT_SPLIT 1
#include "att_fused_block.h"   // k_attention_x3<S, F, PRO>
#undef TG_ATT_SPLIT

// the LDS image of k_attention_x3: dst[g][cout][32] = [hi of channels g*16..+15 | lo of the same] of w[cout][F] * 2^s, the four
// 16-B chunks of a row XOR-swizzled by swz64(cout) (the fragment reads of the kernel undo it); wsc_out = 2^-s
__global__ __launch_bounds__(256) void k_restage_att_split(const float* __restrict__ w, _Float16* __restrict__ dst, float* __restrict__ wsc_out,
                                                           const unsigned* __restrict__ maxbits, int W, int F) {
    const unsigned mb = maxbits[0];
    int sh = mb ? 14 - ((int)((mb >> 23) & 0xffu) - 127) : 0;
    sh = sh < -60 ? -60 : sh > 60 ? 60 : sh;
    const float scale = ldexpf(1.f, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) wsc_out[0] = ldexpf(1.f, -sh);
    const int total = F / 16 * W * 32;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int k = i & 31, r = (i >> 5) % W, g = (i >> 5) / W;
        const int kk = (((k >> 3) ^ swz64(r)) << 3) + (k & 7);                       // logical position of this physical slot
        const float v = w[(size_t)r * F + g * 16 + (kk & 15)] * scale;
        const _Float16 hi = (_Float16)v;
        dst[i] = (kk & 16) ? (_Float16)(v - (float)hi) : hi;
    }
}

#define TG_ATT_SPLIT 0
#include "att_fused_block.h"   // k_attention_h<S, F, PRO>
#undef TG_ATT_SPLIT

// the LDS image of k_attention_h: dst[g][cout][32] = half(w[cout][g*32 + ch(kk)]), kk the logical K slot of the physical position (the
// four 16-B chunks of a row XOR-swizzled by swz64(cout)), ch(kk) = (kk >> 2 & 1)*16 + (kk >> 3)*4 + (kk & 3): lane kq's slots
// kq*8 .. +7 are the channels its two 16-B loads of x bring (kq*4 .. +3 and 16 + kq*4 .. +3)
__global__ __launch_bounds__(256) void k_restage_att_half(const float* __restrict__ w, _Float16* __restrict__ dst, int W, int F) {
    const int total = F / 32 * W * 32;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int k = i & 31, r = (i >> 5) % W, g = (i >> 5) / W;
        const int kk = (((k >> 3) ^ swz64(r)) << 3) + (k & 7);
        dst[i] = (_Float16)w[(size_t)r * F + g * 32 + ((kk >> 2) & 1) * 16 + (kk >> 3) * 4 + (kk & 3)];
    }
}

// Heads after the 3x3 head convs (hc[row][p][16]: channels 0-1 value/own, 2-5 policy; BN+ReLU already applied).
// HR rows per workgroup (8 at 9x9, 2 at 19x19): the dense weights (fc_act alone is 4P x A floats = 106 KB at 9x9) are read once per workgroup and used
// for all its rows -- with one row per workgroup the kernel moved 1.7 GB of L2 -> CU traffic per 16384 rows.  Every output is the
// same k-ordered fmaf chain as before, whatever the batching, so a row's results do not depend on which rows share its workgroup.
template <int S> struct HeadRows { static constexpr int N = S == 9 ? 8 : 2; };      // LDS: 6P + A + 64 floats per row
template <int S>
__global__ __launch_bounds__(256) void k_heads(const float* __restrict__ hc, const float* __restrict__ hca, const float* __restrict__ w_vo,
                                               const float* __restrict__ b_vo, const float* __restrict__ w_v,
                                               const float* __restrict__ b_v, const float* __restrict__ w_o,
                                               const float* __restrict__ b_o, const float* __restrict__ w_a,
                                               const float* __restrict__ b_a, float* __restrict__ policy,
                                               float* __restrict__ value, float* __restrict__ own, int rows) {
    constexpr int P = S * S, A = P + 1, HR = HeadRows<S>::N;
    __shared__ float hin[HR][6 * P];
    __shared__ float hid[HR][64];
    __shared__ float logit[HR][A];
    __shared__ float red[HR][2];
    const int row0 = blockIdx.x * HR, tid = threadIdx.x;
    const int nr = rows - row0 < HR ? rows - row0 : HR;
    for (int i = tid; i < HR * 6 * P; i += 256) {      // channels 0-1 from the value conv, 2-5 from the policy conv
        const int r = i / (6 * P), k = i % (6 * P), c = k / P, p = k % P;
        hin[r][k] = r < nr ? (c < 2 ? hc : hca)[((size_t)(row0 + r) * P + p) * 16 + c] : 0.f;
    }
    __syncthreads();
    // (spreading the rows of the workgroup over all 256 threads -- two / four row groups, each thread half / a quarter of the rows,
    // the same fmaf chains -- was measured: 135 us per launch against 92; the loops are bound by their weight loads, whose number per
    // thread stays the same and whose total doubles.  Splitting the input range instead would change the summation order.)
    if (tid < 64) {                                                   // fc_val_own + ReLU (model.py:99)
        float a[HR];
#pragma unroll
        for (int r = 0; r < HR; ++r) a[r] = b_vo[tid];
        for (int i = 0; i < 2 * P; ++i) {
            const float w = w_vo[i * 64 + tid];
#pragma unroll
            for (int r = 0; r < HR; ++r) a[r] = fmaf(hin[r][i], w, a[r]);
        }
#pragma unroll
        for (int r = 0; r < HR; ++r) hid[r][tid] = a[r] > 0.f ? a[r] : 0.f;
    }
    for (int o = tid; o < A; o += 256) {                              // fc_act (model.py:110)
        float a[HR];
#pragma unroll
        for (int r = 0; r < HR; ++r) a[r] = b_a[o];
        for (int i = 0; i < 4 * P; ++i) {
            const float w = w_a[(size_t)i * A + o];
#pragma unroll
            for (int r = 0; r < HR; ++r) a[r] = fmaf(hin[r][2 * P + i], w, a[r]);
        }
#pragma unroll
        for (int r = 0; r < HR; ++r) logit[r][o] = a[r];
    }
    __syncthreads();
    if (tid < nr) {
        const int r = tid;
        float a = b_v[0];
        for (int k = 0; k < 64; ++k) a = fmaf(hid[r][k], w_v[k], a);
        value[row0 + r] = tanhf(a);                                   // model.py:101
        float mx = logit[r][0];
        for (int o = 1; o < A; ++o) mx = logit[r][o] > mx ? logit[r][o] : mx;
        red[r][0] = mx;
    }
    if (own)
        for (int o = tid; o < P; o += 256) {                          // fc_own (model.py:102)
            float a[HR];
#pragma unroll
            for (int r = 0; r < HR; ++r) a[r] = b_o[o];
            for (int k = 0; k < 64; ++k) {
                const float w = w_o[k * P + o];
#pragma unroll
                for (int r = 0; r < HR; ++r) a[r] = fmaf(hid[r][k], w, a[r]);
            }
#pragma unroll
            for (int r = 0; r < HR; ++r) if (r < nr) own[(size_t)(row0 + r) * P + o] = tanhf(a[r]);
        }
    __syncthreads();
    for (int i = tid; i < HR * A; i += 256) { const int r = i / A, o = i % A; logit[r][o] = expf(logit[r][o] - red[r][0]); }
    __syncthreads();
    if (tid < nr) { float s2 = 0.f; for (int o = 0; o < A; ++o) s2 += logit[tid][o]; red[tid][1] = s2; }
    __syncthreads();
    for (int i = tid; i < nr * A; i += 256) {                          // softmax, model.py:111
        const int r = i / A, o = i % A;
        policy[(size_t)(row0 + r) * A + o] = logit[r][o] * (1.f / red[r][1]);
    }
}

struct ProfScope {
    Net* n; hipStream_t st; bool on;
    ProfScope(Net* net, hipStream_t s, double flops) : n(net), st(s), on(net->prof && net->ev_used + 2 <= net->ev.size()) {
        if (on) { (void)hipEventRecord(n->ev[n->ev_used], st); n->conv_flops += flops; n->conv_launches++; }
        else if (net->prof) n->conv_skipped++;
    }
    ~ProfScope() { if (on) { (void)hipEventRecord(n->ev[n->ev_used + 1], st); n->ev_used += 2; } }
};

template <int S, int F>
int forward_t(tg_ctx* ctx, Net* n, const float* obs, int rows, float* policy, float* value, float* own) {
    constexpr int P = S * S;
    constexpr bool WIDE = F == 128 || F == 256;       // the DMA, fp16 and split chains exist at these widths only
    hipStream_t st = ctx->stream;
    const int M = rows * P;
    const int grid = (M + 127) / 128;                 // stem / head / 1x1 convs: 128 rows per workgroup
    // position tiles per wave in the F->F convs (workgroup = 64*NPT rows): 3 while the accumulators (F/16*NPT*4 registers)
    // still leave room for two waves per SIMD, else 2.  Measured at F=128: 128.0 -> 132.3 TFLOP/s.
    constexpr int NPT = F <= 128 ? 3 : 2;
    const int grid_f = (M + 64 * NPT - 1) / (64 * NPT);
    // k_conv3x3_h2: (256-row tile, 128-cout part) blocks, one workgroup each -- the kernel can walk a tile list, but the hardware
    // dispatcher balances better than a static list (512 persistent workgroups measured 0.6-2 % slower)
    const int grid_h = (M + 255) / 256;
    constexpr int COS = F / 128;
    const int nblk_h2 = COS == 1 ? grid_h : (grid_h + 7) / 8 * 8 * COS;
    const double conv_flops = 2.0 * 9.0 * (double)F * (double)F * (double)M;
    constexpr int WQ = F / 4 + F / 4 + F;             // q|k|v projection width
    const bool big = (long long)M * F * 4 >= (1ll << 31);
    Chain chain = n->path.chain;
    // the DMA chain's slice-major tensors hold whole groups of 16 boards (conv_rows.h) and are addressed by 32-bit byte offsets
    if (chain == CHAIN_DMA && (long long)conv_sg_rows(rows, P) * F * 4 >= (1ll << 31)) chain = CHAIN_F32;
    if (chain == CHAIN_SPLIT && big) TG_FAIL(ctx, TG_ERR_ARG, "split-precision path: rows * P * F * 4 bytes must stay below 2 GiB per activation buffer");
    if (chain == CHAIN_F16 && (long long)M * F * 2 >= (1ll << 31)) TG_FAIL(ctx, TG_ERR_ARG, "fp16 path: rows * P * F * 2 bytes must stay below 2 GiB per activation buffer");
    const bool h16 = chain == CHAIN_F16 || chain == CHAIN_SPLIT, x2 = chain == CHAIN_SPLIT;
    // the fp16 chain's head conv, and the split one's with head_x2, read the conv input act16 that the last layer writes
    const bool head16 = chain == CHAIN_F16 || (x2 && n->path.head_x2);
    auto wsc = [&](size_t conv) { return x2 ? n->wsc + conv : nullptr; };    // split: 2^-s of conv `conv` (stem last)
    const size_t nl = n->layers.size(), nb = n->blocks.size();
    // next_bn(j): the BN that layer j (j == nl: the head conv) wants applied by the layer before it.  Every chain but the general f32
    // one hands a residual block, and the fp16 / split head conv, its input relu(bn(.)) that way.
    auto next_bn = [&](size_t j, const float** sn, const float** tn) -> bool {
        *sn = nullptr; *tn = nullptr;
        if (chain == CHAIN_F32) return false;
        if (j < nl && n->layers[j].kind == 0) { const BlockW& b = n->blocks[n->layers[j].ridx]; *sn = b.s1; *tn = b.t1; return true; }
        if (j == nl && head16) { *sn = n->s_end; *tn = n->t_end; return true; }
        return false;
    };

    // ---- what differs between the chains: stem, residual block, attention block, head conv ----
    float* x = n->bufA; float* y = n->bufB;
    // The DMA chain's residual stream between two conv layers (stem or residual block -> residual block) is ONE tensor, slice-major
    // in the conv's row order (conv_rows.h): the producer writes only it (`sout`), the consumer's conv1 activates it on load and its
    // conv2 starts its accumulators from it (`sin`).  Towards an attention layer or the head the stream is row-major as before, and an
    // attention layer hands a residual block relu(bn1(.)) in bufAct (`act`, `sn` / `tn`: the attention, fp16 and split kernels take
    // them; the f32 conv kernels get no second output).  `chain` is this forward's: a batch that fell back to CHAIN_F32 above has no
    // such stream.
    const bool one = chain == CHAIN_DMA;
    auto conv_layer = [&](size_t j) { return j < nl && n->layers[j].kind == 0; };
    auto stem = [&](bool act, const float* sn, const float* tn, bool sout) {   // conv 16 -> F into the residual stream x
        if constexpr (WIDE) {
            if (h16) {   // input planes are 0/1, exact in fp16; 16 planes padded to 64 channels = 18 stages
                auto* k = x2 ? &k_conv3x3_h2<S, 64, F, 4, false, true> : n->path.r16 ? &k_conv3x3_h2<S, 64, F, 4, true> : &k_conv3x3_h2<S, 64, F, 4>;
                hipLaunchKernelGGL(k, dim3(nblk_h2), dim3(256), 0, st, n->x0h, x, act ? n->act16 : nullptr, nullptr, n->stem_h, n->stem.b,
                                   sn, tn, M, nblk_h2, wsc(2 * nb), n->range);
                return;
            }
            if (chain == CHAIN_DMA) {
                auto* k = sout ? &k_conv3x3<S, 16, F, false, 0, 9, 2, true, true> : &k_conv3x3<S, 16, F, false, 0, 9, 2, true>;
                hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, st, n->x0, x, nullptr, n->stem.w,
                                   n->stem.b, nullptr, nullptr, M, nullptr, nullptr, nullptr);
                return;
            }
        }
        hipLaunchKernelGGL((k_conv3x3<S, 16, F, false, 0>), dim3(grid), dim3(256), 0, st, n->x0, x, nullptr, n->stem.w, n->stem.b, nullptr, nullptr, M);
    };
    auto block = [&](const BlockW& b, int ridx, float* out, bool act, const float* sn, const float* tn, bool sin, bool sout) {   // y = x + conv(conv(x))
        if constexpr (WIDE) {
            if (h16) {
                auto* k1 = x2 ? &k_conv3x3_h2<S, 2 * F, F, 0, false, true> : &k_conv3x3_h2<S, F, F, 0>;
                auto* k2 = x2 ? &k_conv3x3_h2<S, 2 * F, F, 1, false, true> : n->path.r16 ? &k_conv3x3_h2<S, F, F, 1, true> : &k_conv3x3_h2<S, F, F, 1>;
                { ProfScope ps(n, st, conv_flops);
                  hipLaunchKernelGGL(k1, dim3(nblk_h2), dim3(256), 0, st, n->act16, nullptr, n->h16, nullptr, b.h1, b.c1.b, nullptr, nullptr,
                                     M, nblk_h2, wsc(2 * ridx), n->range); }
                { ProfScope ps(n, st, conv_flops);
                  hipLaunchKernelGGL(k2, dim3(nblk_h2), dim3(256), 0, st, n->h16, out, act ? n->act16 : nullptr, x, b.h2, b.c2.b, sn, tn,
                                     M, nblk_h2, wsc(2 * ridx + 1), n->range); }
                return;
            }
            if (chain == CHAIN_DMA) {
                // one workgroup per (range of 128 boards, position): 8 x the longest XCD list of the launch order (conv_rows.h)
                const int grid_sd = conv_launch_grid((rows + 127) / 128, S);
                // conv1 activates the stream on load (sin), or reads the copy that an attention layer left activated in bufAct; conv2
                // (EPI 1) never reads s2 / t2
                auto* k1 = sin ? &k_conv3x3_sg<S, F, 0, true> : &k_conv3x3_sg<S, F, 0>;
                auto* k2 = sin ? (sout ? &k_conv3x3_sg<S, F, 1, true, true> : &k_conv3x3_sg<S, F, 1, true>)
                               : (sout ? &k_conv3x3_sg<S, F, 1, false, true> : &k_conv3x3_sg<S, F, 1>);
                { ProfScope ps(n, st, conv_flops);
                  hipLaunchKernelGGL(k1, dim3(grid_sd), dim3(256), 0, st, sin ? x : n->bufAct, n->bufH, nullptr, b.g1, b.c1.b, nullptr,
                                     sin ? b.s1 : nullptr, sin ? b.t1 : nullptr, rows); }
                { ProfScope ps(n, st, conv_flops);
                  hipLaunchKernelGGL(k2, dim3(grid_sd), dim3(256), 0, st, n->bufH, out, x, b.g2, b.c2.b, nullptr, nullptr, nullptr, rows); }
                return;
            }
        }
        { ProfScope ps(n, st, conv_flops);
          hipLaunchKernelGGL((k_conv3x3<S, F, F, true, 0, 9, NPT>), dim3(grid_f), dim3(256), 0, st, x, n->bufH, nullptr, b.c1.w, b.c1.b, b.s1, b.t1, M); }
        { ProfScope ps(n, st, conv_flops);
          hipLaunchKernelGGL((k_conv3x3<S, F, F, false, 1, 9, NPT>), dim3(grid_f), dim3(256), 0, st, n->bufH, out, x, b.c2.w, b.c2.b, nullptr, nullptr, M); }
    };
    // Self_Attention block (model.py:301-315) xin -> xout; ps/pt: the policy head's relu(bn_end(.)) first.  Non-zero: no kernel fits.
    auto attention = [&](const AttW& a, const float* xin, float* xout, const float* ps, const float* pt, bool act, const float* sn, const float* tn) -> int {
        if constexpr (S == 9 && F == 128) {
            if (x2) {   // one kernel per block: q/k/v projected inside the core, in split precision
                constexpr int lds3 = (int)(sizeof(_Float16) * F / 16 * WQ * 32 + sizeof(float) * (WQ + 6 * F) + 4096);   // image, parameters, touch scratch
                const int nwg = (rows + 3) / 4 < 256 ? (rows + 3) / 4 : 256;
                auto* k = ps ? &k_attention_x3<S, F, true> : &k_attention_x3<S, F, false>;
                hipLaunchKernelGGL(k, dim3(nwg), dim3(256), lds3, st, xin, xout, act ? n->act16 : nullptr, a.x3w, a.qkv.b, a.x3sc,
                                   a.gamma, a.s, a.t, ps, pt, sn, tn, rows, n->range);
                return 0;
            }
            if (chain == CHAIN_F16 && n->path.att_h) {   // the same block with one fp16 product in the projection
                constexpr int ldsh = (int)(sizeof(_Float16) * F / 32 * WQ * 32 + sizeof(float) * (WQ + 6 * F) + 4096);
                const int nwg = (rows + 3) / 4 < 256 ? (rows + 3) / 4 : 256;
                auto* k = ps ? &k_attention_h<S, F, true> : &k_attention_h<S, F, false>;
                hipLaunchKernelGGL(k, dim3(nwg), dim3(256), ldsh, st, xin, xout, act ? n->act16 : nullptr, a.x3w, a.qkv.b,
                                   a.gamma, a.s, a.t, ps, pt, sn, tn, rows, n->range);
                return 0;
            }
        }
        if (chain == CHAIN_F16) return -1;               // (tg_net_load_arch admits fp16 attention only where k_attention_h is built)
        if (S != 19 && chain == CHAIN_F32 && !n->path.att_lds) return -1;
        // the fused q|k|v 1x1 projection on the matrix cores, then the per-board core
        auto* kq = ps ? &k_conv3x3<S, F, WQ, true, 2, 1> : &k_conv3x3<S, F, WQ, false, 2, 1>;
        hipLaunchKernelGGL(kq, dim3(grid), dim3(256), 0, st, xin, n->bufQ, nullptr, a.qkv.w, a.qkv.b, ps, pt, M, nullptr, nullptr, nullptr);
        // 19x19 (f32, both f32 chains): the tiled core, one workgroup per board; `act` is set in the DMA chain only
        if constexpr (S == 19) {
            if (x2) return -1;
            constexpr int ldst = att_t_lds<S, F>();
            hipLaunchKernelGGL((k_attention_t<S, F>), dim3(rows), dim3(256), ldst, st, n->bufQ, xin, xout,
                               act ? n->bufAct : nullptr, a.gamma, a.s, a.t, ps, pt, sn, tn, rows);
            return 0;
        } else {
        // the MFMA core, one wave per board, writes the next residual block's input too (split: as hi + lo)
        if constexpr (S == 9 && F == 256) {
            if (x2) {
                hipLaunchKernelGGL((k_attention_mfma<S, F, 2, true>), dim3((rows + 3) / 4), dim3(256), 0, st, n->bufQ, xin, xout,
                                   reinterpret_cast<float*>(act ? n->act16 : nullptr), a.gamma, a.s, a.t, ps, pt, sn, tn, rows, n->range);
                return 0;
            }
        }
        if constexpr (S == 9 && WIDE) {
            if (chain == CHAIN_DMA) {
                hipLaunchKernelGGL((k_attention_mfma<S, F, 2>), dim3((rows + 3) / 4), dim3(256), 0, st, n->bufQ, xin, xout,
                                   act ? n->bufAct : nullptr, a.gamma, a.s, a.t, ps, pt, sn, tn, rows);
                return 0;
            }
        }
        hipLaunchKernelGGL((k_attention<S, F>), dim3(rows), dim3(256), n->path.att_lds, st, n->bufQ, xin, xout, a.gamma, a.s, a.t, ps, pt);
        return 0;
        }
    };
    // head conv F -> 16 (6 real couts) on relu(bn(in)) (ps/pt) or on in: GEMM + col2im (k_head_gemm); TG_HEAD_GEMM=0 selects the
    // implicit-GEMM kernel it replaced
    auto head_conv = [&](const float* in, float* outp, const float* Wg, const ConvW& cw, const float* ps, const float* pt) {
        const char* hg = getenv("TG_HEAD_GEMM");
        if (hg && atoi(hg) == 0) {
            auto* k = ps ? &k_conv3x3<S, F, 16, true, 0> : &k_conv3x3<S, F, 16, false, 0>;
            hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, st, in, outp, nullptr, cw.w, cw.b, ps, pt, M, nullptr, nullptr, nullptr);
            return;
        }
        constexpr int TMH = 64 * (S == 9 ? 3 : 4) - 2 * (S + 1);
        const int nt = (M + TMH - 1) / TMH, g = nt < 512 ? nt : 512;      // two workgroups per CU walk the tile list
        auto* k = ps ? &k_head_gemm<S, F, true> : &k_head_gemm<S, F, false>;
        hipLaunchKernelGGL(k, dim3(g), dim3(256), 0, st, in, outp, Wg, cw.b, ps, pt, M, nt);
    };

    // ---- the forward: input planes, stem, layers, head convs, dense heads ----
    if (h16) {
        int g0h = (int)(((size_t)M * 8 + 255) / 256); if (g0h > 65535) g0h = 65535;
        if (n->in_bits) hipLaunchKernelGGL((k_bits_to_rows_h<S>), dim3(g0h), dim3(256), 0, st, n->in_bits, n->in_slot, n->x0h, rows, n->C, n->in_words);
        else hipLaunchKernelGGL((k_obs_to_rows_h<S>), dim3(g0h), dim3(256), 0, st, obs, n->x0h, rows, n->C);
    } else {
        int g0 = (int)(((size_t)M * 16 + 255) / 256); if (g0 > 65535) g0 = 65535;
        if (n->in_bits) hipLaunchKernelGGL((k_bits_to_rows<S>), dim3(g0), dim3(256), 0, st, n->in_bits, n->in_slot, n->x0, rows, n->C, n->in_words);
        else hipLaunchKernelGGL((k_obs_to_rows<S>), dim3(g0), dim3(256), 0, st, obs, n->x0, rows, n->C);
    }
    const float* sn; const float* tn;
    bool sm = one && conv_layer(0);                    // x is slice-major in the conv's row order
    { const bool act = next_bn(0, &sn, &tn); stem(act, sn, tn, sm); }
    for (size_t i = 0; i < nl; ++i) {
        const Layer& L = n->layers[i];
        const bool act = next_bn(i + 1, &sn, &tn);
        const bool sin = sm;
        sm = one && L.kind == 0 && conv_layer(i + 1);
        if (L.kind == 1) {
            if (attention(L.a, x, y, nullptr, nullptr, act, sn, tn)) TG_FAIL(ctx, TG_ERR_ARG, "attention blocks: no kernel for this shape and precision (built: f32 at 9x9 with 32 / 64 / 128 / 256 filters and at 19x19 with 128 / 256, f16 at 9x9 with 128, f32x3 at 9x9 with 128 / 256)");
        } else {
            // nothing reads the last block's f32 stream when the head conv takes act16 and no policy attention follows
            block(n->blocks[L.ridx], L.ridx, i + 1 == nl && head16 && !n->pol_att ? nullptr : y, act, sn, tn, sin, sm);
        }
        float* t = x; x = y; y = t;
    }
    // heads: value/ownership conv reads relu(bn_end(x)) (model.py:94,97); the policy conv reads the same tensor, or its
    // Self_Attention when the architecture has attention_act (model.py:72,106-107)
    if (!head16) {
        head_conv(x, n->hc, n->head_g, n->head, n->s_end, n->t_end);
    } else if constexpr (WIDE) {
        if (!x2) {
            hipLaunchKernelGGL((k_head_h<S, F>), dim3(grid_h), dim3(256), 0, st, n->act16, n->hc, n->head_h, n->head.b, M);
        } else if constexpr (F == 128) {
            constexpr int TMH = 64 * (S == 9 ? 3 : 4) - 2 * (S + 1);
            const int nt = (M + TMH - 1) / TMH, g = nt < 512 ? nt : 512;
            hipLaunchKernelGGL((k_head_gemm_x2<S, F>), dim3(g), dim3(256), 0, st, n->act16, n->hc, n->head_x2, n->head_x2sc, n->head.b, M, nt);
        }
    }
    const float* hca = n->hc;
    if (n->pol_att) {
        // the f32 head conv reads the attention's f32 output in the split chain too (the policy head conv on the split MFMA was
        // measured: what it saves the attention block's extra split write of its output costs -- 723.3 vs 723.2 k sims/s)
        if (attention(n->patt, x, y, n->s_end, n->t_end, false, nullptr, nullptr)) TG_FAIL(ctx, TG_ERR_ARG, "attention policy head: no kernel for this shape and precision (built: f32 at 9x9 with 32 / 64 / 128 / 256 filters and at 19x19 with 128 / 256, f16 at 9x9 with 128, f32x3 at 9x9 with 128 / 256)");
        head_conv(y, n->hca, n->head_ag, n->head_a, nullptr, nullptr);
        hca = n->hca;
    }
    hipLaunchKernelGGL((k_heads<S>), dim3((rows + HeadRows<S>::N - 1) / HeadRows<S>::N), dim3(256), 0, st, n->hc, hca, n->w_vo, n->b_vo, n->w_v, n->b_v,
                       n->w_o, n->b_o, n->w_a, n->b_a, policy, value, own, rows);
    TG_HIP(ctx, hipGetLastError());
    return TG_OK;
}

int adopt_pending(tg_ctx* ctx, Net* n, bool wait);

// A finished background refresh takes over only where the CALLER is at a boundary: tg_net_predict (every call stands alone) and
// tg_sp_begin_move (tg_net_adopt_ready) -- never in the middle of a move's search, so one search tree and one recorded pi never
// mix evaluations of two weight sets and the switch point does not depend on upload timing within a move.
int forward(tg_ctx* ctx, Net* n, const float* obs, int rows, float* policy, float* value, float* own) {
    if (rows <= 0) return TG_OK;
    if (rows > n->rows_cap) TG_FAIL(ctx, TG_ERR_ARG, "network batch larger than the allocated activation buffers");
#define TG_NET_CASE(SZ, FF) if (n->S == SZ && n->F == FF) return forward_t<SZ, FF>(ctx, n, obs, rows, policy, value, own)
    TG_NET_CASE(9, 32); TG_NET_CASE(9, 64); TG_NET_CASE(9, 128); TG_NET_CASE(9, 256);
    TG_NET_CASE(19, 128); TG_NET_CASE(19, 256);
#undef TG_NET_CASE
    TG_FAIL(ctx, TG_ERR_ARG, "unsupported (board_size, net_filters): built are 9x{32,64,128,256}, 19x{128,256}");
}

// forward() under the context's symmetry mode (tg_net_set_symmetry; symmetry.hip) -- the one place tg_net_forward (bit input
// through the engine's slot table) and tg_net_predict (float planes) reach the network.  Mode 0 is forward() itself: nothing else
// is launched or allocated.  Otherwise the rows are transformed into a dense staging batch, the unchanged forward reads it through
// in_bits / in_slot and writes to staging, and the back-map kernel puts the outputs into policy / value / own in the original
// orientation; mean8 does that for s = 0..7 in order, accumulating in the destination.  No weight refresh is adopted in here
// (adopt_pending is the callers'), so the eight passes of one mean8 evaluation see one weight set.
int forward_sym(tg_ctx* ctx, Net* n, const float* obs, int rows, float* policy, float* value, float* own) {
    SymState& y = ctx->sym;
    if (y.mode == SYM_NONE) return forward(ctx, n, obs, rows, policy, value, own);
    if (rows <= 0) return TG_OK;
    if (rows > n->rows_cap) TG_FAIL(ctx, TG_ERR_ARG, "network batch larger than the allocated activation buffers");
    const int W = (n->C * n->P + 31) / 32;
    const bool from_planes = n->in_bits == nullptr;
    { int rc = sym_reserve(ctx, n->rows_cap, W, n->A, n->P, from_planes); if (rc) return rc; }
    const uint32_t* src = n->in_bits; const int32_t* slot = n->in_slot;
    if (from_planes) {
        int rc = sym_pack(ctx, obs, rows, n->C, n->P, W); if (rc) return rc;
        src = (const uint32_t*)y.packed.p; slot = nullptr;
    }
    const uint32_t* keep_bits = n->in_bits; const int32_t* keep_slot = n->in_slot; const int keep_words = n->in_words;
    const int passes = y.mode == SYM_MEAN8 ? 8 : 1;
    int rc = TG_OK;
    for (int k = 0; k < passes && rc == TG_OK; ++k) {
        rc = y.mode == SYM_MEAN8 ? sym_transform(ctx, src, slot, rows, n->S, n->C, W, SYM_FIXED, (uint32_t)k)
                                 : sym_transform(ctx, src, slot, rows, n->S, n->C, W, y.mode, y.arg);
        if (rc) break;
        n->in_bits = (const uint32_t*)y.bits.p; n->in_slot = (const int32_t*)y.ident.p; n->in_words = W;
        rc = forward(ctx, n, nullptr, rows, (float*)y.pol.p, (float*)y.val.p, own ? (float*)y.own.p : nullptr);
        n->in_bits = keep_bits; n->in_slot = keep_slot; n->in_words = keep_words;
        if (rc) break;
        rc = sym_backmap(ctx, policy, value, own, rows, n->S, passes == 1 ? 0 : k == 0 ? 0 : k == 7 ? 2 : 1);
    }
    return rc;
}

// arch: one letter per trunk layer, 'R' residual block / 'A' Self_Attention block, optional "+P" = attention in the policy
// head.  The reference MainNetwork (model.py:49-76) is "RARRRARRRRAR+P"; BASELINE's N-block tower is N x 'R'.
bool parse_arch(const std::string& arch, std::string* trunk, bool* pol) {
    *pol = false; *trunk = arch;
    const size_t plus = arch.find('+');
    if (plus != std::string::npos) {
        if (arch.substr(plus) != "+P") return false;
        *pol = true; *trunk = arch.substr(0, plus);
    }
    for (char c : *trunk) if (c != 'R' && c != 'A') return false;
    return true;
}

size_t expected_floats(int S, int C, int F, const std::string& arch) {
    const size_t P = (size_t)S * S, A = P + 1, Wq = (size_t)F / 4 * 2 + F;
    (void)C;
    std::string trunk; bool pol;
    if (!parse_arch(arch, &trunk, &pol)) return 0;
    const size_t att = Wq * F + Wq + 1 + 2 * (size_t)F;
    size_t n = 9 * (size_t)F * 16 + F;
    for (char c : trunk) n += (c == 'R') ? (2 * (size_t)F + 2 * (9 * (size_t)F * F + F)) : att;
    n += 2 * (size_t)F;
    if (pol) n += att + 9 * 16 * (size_t)F + 16;
    n += 9 * 16 * (size_t)F + 16;
    n += 2 * P * 64 + 64 + 64 + 1 + 64 * P + P + 4 * P * A + A;
    return n;
}

// Bind the pointer fields of `n` to weight set `k` (blob sections in the order transgo_amd/model.py:pack_weights writes them).
void bind_weights(Net* n, int k) {
    const int F = n->F; const size_t P = n->P, A = n->A, Wq = (size_t)F / 4 * 2 + F;
    const Net::WeightSet& w = n->sets[k];
    n->blob = w.blob; n->wstage = w.wstage; n->wh = w.wh; n->stem_h = w.stem_h; n->head_h = w.head_h; n->wsc = w.wsc; n->head_g = w.head_g; n->head_ag = w.head_ag;
    n->head_x2 = w.head_x2; n->head_x2sc = w.head_x2sc;
    std::string trunk; bool pol = false;
    parse_arch(n->arch, &trunk, &pol);
    const float* p = w.blob;
    auto take = [&](size_t c) { const float* q = p; p += c; return q; };
    auto take_att = [&](AttW& a) { a.qkv.w = take(Wq * F); a.qkv.b = take(Wq); a.gamma = take(1); a.s = take(F); a.t = take(F); };
    n->stem.w = take(9 * (size_t)F * 16); n->stem.b = take(F);
    n->blocks.assign(n->NB, BlockW{});
    n->layers.clear();
    const size_t per = 9 * (size_t)F * F;
    int ri = 0, ai = 0;
    // halfs per attention layer: k_attention_x3's LDS image (hi | lo per 16 channels), or k_attention_h's (plain fp16)
    const size_t att_img = (size_t)F / (n->path.att_h ? 32 : 16) * Wq * 32;
    auto bind_x3 = [&](AttW& a) { if (w.att_h) { a.x3w = w.att_h + (size_t)ai * att_img; if (w.att_sc) a.x3sc = w.att_sc + ai; } ++ai; };
    for (char c : trunk) {
        Layer L; L.kind = c == 'A'; L.ridx = -1; L.a = AttW{};
        if (c == 'R') {
            BlockW& b = n->blocks[ri];
            b.s1 = take(F); b.t1 = take(F);
            b.c1.w = take(per); b.c1.b = take(F);
            b.c2.w = take(per); b.c2.b = take(F);
            b.g1 = w.wstage ? w.wstage + (size_t)(2 * ri) * per : nullptr; b.g2 = w.wstage ? w.wstage + (size_t)(2 * ri + 1) * per : nullptr;
            const size_t perh = n->path.chain == CHAIN_SPLIT ? 2 * per : per;   // split precision: hi + lo halves of every weight
            b.h1 = w.wh ? w.wh + (size_t)(2 * ri) * perh : nullptr; b.h2 = w.wh ? w.wh + (size_t)(2 * ri + 1) * perh : nullptr;
            L.ridx = ri++;
        } else {
            take_att(L.a); bind_x3(L.a);
        }
        n->layers.push_back(L);
    }
    n->s_end = take(F); n->t_end = take(F);
    if (pol) { take_att(n->patt); bind_x3(n->patt); n->head_a.w = take(9 * 16 * (size_t)F); n->head_a.b = take(16); }
    n->head.w = take(9 * 16 * (size_t)F); n->head.b = take(16);
    n->w_vo = take(2 * P * 64); n->b_vo = take(64); n->w_v = take(64); n->b_v = take(1);
    n->w_o = take(64 * P); n->b_o = take(P); n->w_a = take(4 * P * A); n->b_a = take(A);
}

// Upload `blob` into weight set k and rebuild its stage-ordered copies, everything on `st` (no synchronisation here).
int fill_weight_set(tg_ctx* ctx, Net* n, int k, const float* blob, hipStream_t st, bool blob_on_device = false) {
    const int F = n->F;
    TG_HIP(ctx, hipMemcpyAsync(n->sets[k].blob, blob, sizeof(float) * n->blob_floats,
                               blob_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (blob_on_device) {
        // the library keeps no caller pointer after a call returns: the copy out of the caller's buffer is over before the
        // (asynchronous) restaging starts
        TG_HIP(ctx, hipStreamSynchronize(st));
    }
    TG_HIP(ctx, hipMemsetAsync(n->range + 1 + k, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_absmax, dim3(256), dim3(256), 0, st, (const float*)n->sets[k].blob, n->blob_floats, n->range + 1 + k);
    Net view = *n;                                        // pointer fields of set k without disturbing the live binding
    bind_weights(&view, k);
    hipLaunchKernelGGL(k_restage_head, dim3(64), dim3(256), 0, st, view.head.w, n->sets[k].head_g, F);
    if (n->pol_att) hipLaunchKernelGGL(k_restage_head, dim3(64), dim3(256), 0, st, view.head_a.w, n->sets[k].head_ag, F);
    const NetPath& p = n->path;
    if (p.chain == CHAIN_SPLIT) {
        // split copies (hi | lo of w * 2^s per conv), made on the device from the blob just uploaded; the scale words double as the
        // scratch of the abs-max reduction (bit patterns), overwritten with 2^-s by the restaging kernel that follows in order
        const size_t nconv = 2 * view.blocks.size() + 1;
        unsigned* mx = reinterpret_cast<unsigned*>(n->sets[k].wsc) + nconv;          // second half of the allocation
        TG_HIP(ctx, hipMemsetAsync(mx, 0, sizeof(unsigned) * nconv, st));
        size_t ci = 0;
        for (const BlockW& b : view.blocks) {
            for (int h = 0; h < 2; ++h) {
                const float* w = h ? b.c2.w : b.c1.w;
                hipLaunchKernelGGL(k_absmax, dim3(256), dim3(256), 0, st, w, (size_t)9 * F * F, mx + ci);
                hipLaunchKernelGGL(k_restage_split, dim3(1024), dim3(256), 0, st, w, const_cast<_Float16*>(h ? b.h2 : b.h1), n->sets[k].wsc + ci,
                                   (const unsigned*)(mx + ci), F, F, F / 16, 1);
                ++ci;
            }
        }
        if (p.att_x3) {                                                               // fused attention layers: split q|k|v weights
            std::vector<const AttW*> atts;
            for (const Layer& L : view.layers) if (L.kind == 1) atts.push_back(&L.a);
            if (n->pol_att) atts.push_back(&view.patt);
            const int Wq = F / 4 * 2 + F;
            unsigned* amx = reinterpret_cast<unsigned*>(n->sets[k].att_sc) + atts.size();
            TG_HIP(ctx, hipMemsetAsync(amx, 0, sizeof(unsigned) * atts.size(), st));
            for (size_t a = 0; a < atts.size(); ++a) {
                hipLaunchKernelGGL(k_absmax, dim3(64), dim3(256), 0, st, atts[a]->qkv.w, (size_t)Wq * F, amx + a);
                hipLaunchKernelGGL(k_restage_att_split, dim3(256), dim3(256), 0, st, atts[a]->qkv.w, const_cast<_Float16*>(atts[a]->x3w),
                                   const_cast<float*>(atts[a]->x3sc), (const unsigned*)(amx + a), Wq, F);
            }
        }
        hipLaunchKernelGGL(k_absmax, dim3(64), dim3(256), 0, st, view.stem.w, (size_t)9 * F * 16, mx + ci);
        hipLaunchKernelGGL(k_restage_split, dim3(256), dim3(256), 0, st, view.stem.w, view.stem_h, n->sets[k].wsc + ci, (const unsigned*)(mx + ci),
                           F, 16, 2, 1);                                              // 16 planes = one group, padded to two (an even stage count)
        if (p.head_x2) {
            unsigned* hmx = reinterpret_cast<unsigned*>(n->sets[k].head_x2sc) + 1;
            TG_HIP(ctx, hipMemsetAsync(hmx, 0, sizeof(unsigned), st));
            hipLaunchKernelGGL(k_absmax, dim3(16), dim3(256), 0, st, view.head.w, (size_t)9 * 16 * F, hmx);
            hipLaunchKernelGGL(k_restage_head_split, dim3(32), dim3(256), 0, st, view.head.w, n->sets[k].head_x2, n->sets[k].head_x2sc, (const unsigned*)hmx, F);
        }
        TG_HIP(ctx, hipGetLastError());
    } else if (p.chain == CHAIN_F16) {
        // stage-ordered fp16 copies, converted on the device from the blob just uploaded (round to nearest even)
        for (const BlockW& b : view.blocks) {
            hipLaunchKernelGGL(k_restage_half, dim3(1024), dim3(256), 0, st, b.c1.w, const_cast<_Float16*>(b.h1), F, F, F, 32, 1);   // k_conv3x3_h2: 32-channel stages, paired couts
            hipLaunchKernelGGL(k_restage_half, dim3(1024), dim3(256), 0, st, b.c2.w, const_cast<_Float16*>(b.h2), F, F, F, 32, 1);
        }
        hipLaunchKernelGGL(k_restage_half, dim3(256), dim3(256), 0, st, view.stem.w, view.stem_h, F, 16, 64, 32, 1);
        hipLaunchKernelGGL(k_restage_half, dim3(256), dim3(256), 0, st, view.head.w, view.head_h, 16, F, F, 32, 0);
        if (p.att_h) {                                                                // fused attention layers: the fp16 q|k|v image, trunk and +P
            for (const Layer& L : view.layers)
                if (L.kind == 1) hipLaunchKernelGGL(k_restage_att_half, dim3(96), dim3(256), 0, st, L.a.qkv.w, const_cast<_Float16*>(L.a.x3w), F / 4 * 2 + F, F);
            if (n->pol_att) hipLaunchKernelGGL(k_restage_att_half, dim3(96), dim3(256), 0, st, view.patt.qkv.w, const_cast<_Float16*>(view.patt.x3w), F / 4 * 2 + F, F);
        }
        TG_HIP(ctx, hipGetLastError());
    } else if (p.chain == CHAIN_DMA) {
        // stage-ordered copy for k_conv3x3_sg, [slice*9 + tap][cout][16 channels of the slice], made on the device
        for (const BlockW& b : view.blocks) {
            hipLaunchKernelGGL(k_restage_f32, dim3(1024), dim3(256), 0, st, b.c1.w, const_cast<float*>(b.g1), F);
            hipLaunchKernelGGL(k_restage_f32, dim3(1024), dim3(256), 0, st, b.c2.w, const_cast<float*>(b.g2), F);
        }
        TG_HIP(ctx, hipGetLastError());
    }
    return TG_OK;
}

// A completed asynchronous refresh becomes the live set.  Called at boundaries only -- tg_sp_begin_move (tg_net_adopt_ready), every
// stand-alone tg_net_predict, tg_net_load_poll, and at the top of every load -- never from forward(): a host that drives
// tg_sp_collect / tg_net_forward / tg_sp_absorb itself adopts a refresh through tg_net_load_poll (include/transgo_hip.h).
int adopt_pending(tg_ctx* ctx, Net* n, bool wait) {
    if (!n->pending) return TG_OK;
    if (wait) TG_HIP(ctx, hipEventSynchronize(n->loaded));
    else if (hipEventQuery(n->loaded) != hipSuccess) return TG_OK;     // still in flight: keep searching on the old weights
    n->active ^= 1;
    bind_weights(n, n->active);
    n->pending = false;
    tg::eval_cache_invalidate(ctx);                                     // another weight set: cached outputs are the old one's
    TG_HIP(ctx, hipEventRecord(n->swapped, ctx->stream));               // kernels already queued may still read the retired set
    return TG_OK;
}

// The forward's path for a network of this shape and precision (tg_net_load_arch has rejected the unsupported combinations).
NetPath net_path(int S, int F, int prec, const std::string& trunk, bool pol) {
    const size_t P = (size_t)S * S, Wq = (size_t)F / 4 * 2 + F;
    const bool any_att = pol || trunk.find('A') != std::string::npos;
    NetPath p;
    if (prec == 3) p.chain = CHAIN_SPLIT;
    else if (prec >= 1) p.chain = CHAIN_F16;
    else if (F == 128 || F == 256) {                                    // attention layers: k_attention_mfma (9x9), k_attention_t (19x19)
        const char* dma = getenv("TG_DMA_CONV");
        p.chain = dma && atoi(dma) == 0 ? CHAIN_F32 : CHAIN_DMA;
    }
    p.r16 = prec == 2;
    p.att_x3 = prec == 3 && any_att && F == 128 && S == 9;
    p.att_h = prec == 1 && any_att && F == 128 && S == 9;
    p.head_x2 = prec == 3 && F == 128 && !trunk.empty() && trunk.back() == 'R';
    const size_t lds = sizeof(float) * (P * Wq + P * (P + 1));
    p.att_lds = any_att && lds <= 160 * 1024 ? lds : 0;
    return p;
}

}  // namespace

extern "C" {

size_t tg_net_blob_floats(int board_size, int encode_dim, int filters, int blocks) {
    return expected_floats(board_size, encode_dim, filters, std::string((size_t)(blocks > 0 ? blocks : 0), 'R'));
}

size_t tg_net_blob_floats_arch(int board_size, int encode_dim, int filters, const char* arch) {
    return arch ? expected_floats(board_size, encode_dim, filters, arch) : 0;
}

int tg_net_load(tg_ctx* ctx, const float* blob, size_t n_floats, int rows_cap) {
    if (!ctx) return TG_ERR_ARG;
    const std::string arch((size_t)(ctx->cfg.net_blocks > 0 ? ctx->cfg.net_blocks : 0), 'R');
    return tg_net_load_arch(ctx, arch.c_str(), blob, n_floats, rows_cap);
}

int tg_net_load_arch(tg_ctx* ctx, const char* arch_c, const float* blob, size_t n_floats, int rows_cap) {
    if (!ctx || !blob || !arch_c) return TG_ERR_ARG;
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const int S = ctx->S, C = ctx->cfg.encode_dim, F = ctx->cfg.net_filters;
    const std::string arch(arch_c);
    std::string trunk; bool pol = false;
    if (!parse_arch(arch, &trunk, &pol)) TG_FAIL(ctx, TG_ERR_ARG, "bad architecture string (letters R/A, optional +P)");
    if (C > 16) TG_FAIL(ctx, TG_ERR_ARG, "encode_dim > 16 not supported by the stem kernel");
    if (F % 32 != 0) TG_FAIL(ctx, TG_ERR_ARG, "net_filters must be a multiple of 32");
    if (n_floats != expected_floats(S, C, F, arch)) TG_FAIL(ctx, TG_ERR_ARG, "weight blob size does not match (board_size, filters, architecture)");
    if (!ctx->eng) { ctx->eng = new Engine(); }          // rules-only context + network: a bare evaluator
    Engine* e = ctx->eng;
    if (rows_cap <= 0) rows_cap = e->rows_cap > 0 ? e->rows_cap : 256;
    if (e->rows_cap > rows_cap) rows_cap = e->rows_cap;
    Net* n = e->net;
    const int prec = ctx->cfg.net_precision;
    if (prec < 0 || prec > 3) TG_FAIL(ctx, TG_ERR_ARG, "net_precision: 0 (f32), 1 (fp16 storage, f32 accumulate, f32 residual stream), 2 (fp16 residual stream too) or 3 (split precision: fp16 hi + lo operands, f32 accumulate)");
    if (n && (n->rows_cap < rows_cap || n->arch != arch || n->prec != prec)) { tg_net_destroy(ctx); n = nullptr; }
    const size_t P = (size_t)S * S, A = P + 1, Wq = (size_t)F / 4 * 2 + F;
    const bool any_att = pol || trunk.find('A') != std::string::npos;
    int NB = 0; for (char c : trunk) NB += c == 'R';
    if (prec >= 1 && ((any_att && !(prec == 3 && S == 9) && !(prec == 1 && S == 9 && F == 128)) || (F != 128 && F != 256)))
        TG_FAIL(ctx, TG_ERR_ARG, "net_precision 1 / 2 (fp16 matrix cores) is built for towers with 128 or 256 filters; attention layers are built for 1 (fp16 storage, f32 residual stream) at 9x9 with 128 filters and for 3 (split precision) at 9x9, not for 2, nor for 1 at 19x19 or with 256 filters");
    if (prec == 0 && any_att && S == 19 && F != 128 && F != 256)
        TG_FAIL(ctx, TG_ERR_ARG, "attention layers at 19x19 are built for net_precision 0 (f32) with 128 or 256 filters (k_attention_t); at 9x9 for every filter count of the f32 path");
    if (!n) {
        n = new Net();
        e->net = n;
        n->S = S; n->P = (int)P; n->A = (int)A; n->C = C; n->F = F; n->NB = NB; n->rows_cap = rows_cap; n->arch = arch; n->pol_att = pol;
        n->blob_floats = n_floats; n->prec = prec;
        const NetPath& p = n->path = net_path(S, F, prec, trunk, pol);
        const bool h16 = p.chain == CHAIN_F16 || p.chain == CHAIN_SPLIT, x2 = p.chain == CHAIN_SPLIT;
        const size_t act = sizeof(float) * (size_t)rows_cap * P * F;
        // bufH and bufAct are slice-major in the DMA chain: whole groups of 16 boards (conv_rows.h), the padding never written; so is
        // the residual stream between two conv layers there (bufA / bufB hold it in either layout)
        const size_t act_sm = sizeof(float) * (size_t)conv_sg_rows(rows_cap, (int)P) * F;
        TG_HIP(ctx, hipMalloc((void**)&n->bufA, p.chain == CHAIN_DMA ? act_sm : act));
        TG_HIP(ctx, hipMalloc((void**)&n->bufB, p.chain == CHAIN_DMA ? act_sm : act));
        TG_HIP(ctx, hipMalloc((void**)&n->bufH, act_sm));
        TG_HIP(ctx, hipMalloc((void**)&n->x0, sizeof(float) * (size_t)rows_cap * P * 16));
        TG_HIP(ctx, hipMalloc((void**)&n->hc, sizeof(float) * (size_t)rows_cap * P * 16));
        TG_HIP(ctx, hipMalloc((void**)&n->own, sizeof(float) * (size_t)rows_cap * P));
        TG_HIP(ctx, hipMalloc((void**)&n->range, sizeof(unsigned) * 4));
        TG_HIP(ctx, hipMemset(n->range, 0, sizeof(unsigned) * 4));

        if (any_att && !p.att_h) TG_HIP(ctx, hipMalloc((void**)&n->bufQ, sizeof(float) * (size_t)rows_cap * P * Wq));
        if (pol) TG_HIP(ctx, hipMalloc((void**)&n->hca, sizeof(float) * (size_t)rows_cap * P * 16));
        const size_t wcopy = (size_t)(NB > 0 ? 2 * NB : 1) * 9 * F * F;
        // relu(bn1(.)) beside the stream: only an attention layer hands it to a residual block ("AR"), the conv layers share one stream
        if (p.chain == CHAIN_DMA && trunk.find("AR") != std::string::npos) TG_HIP(ctx, hipMalloc((void**)&n->bufAct, act_sm));
        for (Net::WeightSet& w : n->sets) {
            TG_HIP(ctx, hipMalloc((void**)&w.blob, sizeof(float) * n_floats));
            TG_HIP(ctx, hipMalloc((void**)&w.head_g, sizeof(float) * 64 * (size_t)F));
            if (pol) TG_HIP(ctx, hipMalloc((void**)&w.head_ag, sizeof(float) * 64 * (size_t)F));
            if (p.chain == CHAIN_DMA) TG_HIP(ctx, hipMalloc((void**)&w.wstage, sizeof(float) * wcopy));
            if (h16) {
                TG_HIP(ctx, hipMalloc((void**)&w.wh, sizeof(_Float16) * wcopy * (x2 ? 2 : 1)));
                TG_HIP(ctx, hipMalloc((void**)&w.stem_h, sizeof(_Float16) * 9 * (size_t)F * 64));
            }
            if (p.chain == CHAIN_F16) TG_HIP(ctx, hipMalloc((void**)&w.head_h, sizeof(_Float16) * 9 * 16 * (size_t)F));
            if (x2) TG_HIP(ctx, hipMalloc((void**)&w.wsc, sizeof(float) * 2 * (size_t)(2 * NB + 1)));
            if (p.head_x2) {
                TG_HIP(ctx, hipMalloc((void**)&w.head_x2, sizeof(_Float16) * 64 * (size_t)F * 2));
                TG_HIP(ctx, hipMalloc((void**)&w.head_x2sc, sizeof(float) * 2));
            }
            if (p.att_x3) {                                                      // its weight image must fit LDS
                size_t n_att = pol ? 1 : 0; for (char c : trunk) n_att += c == 'A';
                TG_HIP(ctx, hipMalloc((void**)&w.att_h, sizeof(_Float16) * n_att * ((size_t)F / 16 * Wq * 32)));
                TG_HIP(ctx, hipMalloc((void**)&w.att_sc, sizeof(float) * 2 * n_att));
            }
            if (p.att_h) {                                                       // k_attention_h: plain fp16, 48 KB per layer
                size_t n_att = pol ? 1 : 0; for (char c : trunk) n_att += c == 'A';
                TG_HIP(ctx, hipMalloc((void**)&w.att_h, sizeof(_Float16) * n_att * ((size_t)F / 32 * Wq * 32)));
            }
        }
        if (h16) {
            TG_HIP(ctx, hipMalloc((void**)&n->act16, x2 ? act : act / 2));     // split precision: hi + lo per element
            TG_HIP(ctx, hipMalloc((void**)&n->h16, x2 ? act : act / 2));
            TG_HIP(ctx, hipMalloc((void**)&n->x0h, sizeof(_Float16) * (size_t)rows_cap * P * 64));
        }
        TG_HIP(ctx, hipStreamCreateWithFlags(&n->side, hipStreamNonBlocking));
        TG_HIP(ctx, hipEventCreateWithFlags(&n->loaded, hipEventDisableTiming));
        TG_HIP(ctx, hipEventCreateWithFlags(&n->swapped, hipEventDisableTiming));
        TG_HIP(ctx, hipEventRecord(n->swapped, ctx->stream));
        TG_HIP(ctx, hipHostMalloc((void**)&n->pinned, sizeof(float) * n_floats, hipHostMallocDefault));
        n->active = 1;                                    // the load below fills set 0 and makes it the live one
        if (p.att_x3) {
            const int lds3 = (int)(sizeof(_Float16) * (size_t)F / 16 * Wq * 32 + sizeof(float) * (Wq + 6 * (size_t)F) + 4096);
            TG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_x3<9, 128, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds3));
            TG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_x3<9, 128, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds3));
        }
        if (p.att_h) {
            const int ldsh = (int)(sizeof(_Float16) * (size_t)F / 32 * Wq * 32 + sizeof(float) * (Wq + 6 * (size_t)F) + 4096);
            TG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_h<9, 128, false>), hipFuncAttributeMaxDynamicSharedMemorySize, ldsh));
            TG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_h<9, 128, true>), hipFuncAttributeMaxDynamicSharedMemorySize, ldsh));
        }
        if (any_att && prec == 0 && S == 19) {            // k_attention_t: k fragments, two probability tile rows, row statistics
            hipError_t er = hipSuccess;
            if (F == 128) er = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_t<19, 128>), hipFuncAttributeMaxDynamicSharedMemorySize, att_t_lds<19, 128>());
            if (F == 256) er = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_t<19, 256>), hipFuncAttributeMaxDynamicSharedMemorySize, att_t_lds<19, 256>());
            TG_HIP(ctx, er);
        }
        if (p.att_lds) {
            hipError_t er = hipSuccess;
#define TG_ATT_ATTR(SZ, FF) if (S == SZ && F == FF) er = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention<SZ, FF>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.att_lds)
            TG_ATT_ATTR(9, 32); TG_ATT_ATTR(9, 64); TG_ATT_ATTR(9, 128); TG_ATT_ATTR(9, 256);
#undef TG_ATT_ATTR
            TG_HIP(ctx, er);
        }
    }
    // Synchronous refresh (trainer.py:76-79 -> self_play.py:913): an asynchronous one still in flight is adopted first, then the
    // retired set is filled on the context's own stream (in order behind every kernel that reads it) and becomes the live set.
    { int rc = adopt_pending(ctx, n, /*wait=*/true); if (rc) return rc; }
    const int k = n->active ^ 1;
    { int rc = fill_weight_set(ctx, n, k, blob, ctx->stream); if (rc) return rc; }
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    n->active = k;
    bind_weights(n, k);
    tg::eval_cache_invalidate(ctx);
    return TG_OK;
}

// The refresh that never stalls a search: the blob is copied to pinned memory, uploaded and re-staged into the
// retired weight set on a side stream while the context's stream keeps searching on the live set; the switch happens at the next
// move boundary (tg_sp_begin_move), stand-alone tg_net_predict or tg_net_load_poll that finds the upload complete -- never inside a
// search.  Needs a network already loaded with the same architecture (else: synchronous).
int tg_net_load_async(tg_ctx* ctx, const char* arch_c, const float* blob, size_t n_floats) {
    if (!ctx || !blob || !arch_c) return TG_ERR_ARG;
    Net* n = ctx->eng ? ctx->eng->net : nullptr;
    if (!n || n->arch != arch_c || n->blob_floats != n_floats || n->prec != ctx->cfg.net_precision)
        return tg_net_load_arch(ctx, arch_c, blob, n_floats, 0);
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    { int rc = adopt_pending(ctx, n, /*wait=*/true); if (rc) return rc; }     // at most one refresh in flight
    memcpy(n->pinned, blob, sizeof(float) * n_floats);
    TG_HIP(ctx, hipStreamWaitEvent(n->side, n->swapped, 0));                 // nothing queued before the last switch reads this set now
    { int rc = fill_weight_set(ctx, n, n->active ^ 1, n->pinned, n->side); if (rc) return rc; }
    TG_HIP(ctx, hipEventRecord(n->loaded, n->side));
    n->pending = true;
    return TG_OK;
}

// The same with the blob already in THIS GPU's memory (what an RCCL broadcast delivered): device -> device into the retired set,
// no host bounce.  The contents of d_blob must be complete when the call is made (synchronise the producing stream first); the
// buffer may be reused as soon as the call returns.
int tg_net_load_async_dev(tg_ctx* ctx, const char* arch_c, const float* d_blob, size_t n_floats) {
    if (!ctx || !d_blob || !arch_c) return TG_ERR_ARG;
    Net* n = ctx->eng ? ctx->eng->net : nullptr;
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if (!n || n->arch != arch_c || n->blob_floats != n_floats || n->prec != ctx->cfg.net_precision) {
        // nothing to refresh yet (first weights of this context, or another architecture): the synchronous load, through the host
        std::vector<float> host(n_floats);
        TG_HIP(ctx, hipMemcpy(host.data(), d_blob, sizeof(float) * n_floats, hipMemcpyDeviceToHost));
        return tg_net_load_arch(ctx, arch_c, host.data(), n_floats, 0);
    }
    { int rc = adopt_pending(ctx, n, /*wait=*/true); if (rc) return rc; }
    TG_HIP(ctx, hipStreamWaitEvent(n->side, n->swapped, 0));
    { int rc = fill_weight_set(ctx, n, n->active ^ 1, d_blob, n->side, /*blob_on_device=*/true); if (rc) return rc; }
    TG_HIP(ctx, hipEventRecord(n->loaded, n->side));
    n->pending = true;
    return TG_OK;
}

// pending = 1 while an asynchronous refresh has not been adopted yet; wait != 0 blocks until it is (and adopts it).
int tg_net_load_poll(tg_ctx* ctx, int wait, int* pending) {
    if (!ctx || !ctx->eng || !ctx->eng->net) return TG_ERR_STATE;
    Net* n = ctx->eng->net;
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = adopt_pending(ctx, n, wait != 0);
    if (pending) *pending = n->pending ? 1 : 0;
    return rc;
}

#ifdef TG_CONV_STAMP
int tg_debug_conv_stamps(unsigned long long* out, int n) {
    if (n > 96) n = 96;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_conv_stamp), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -1;
}
// the drain records of one conv (epi 0 / 1): `n` workgroups x 6 words
int tg_debug_conv_drain(unsigned long long* out, int epi, int n) {
    if (n > TG_DRAIN_CAP) n = TG_DRAIN_CAP;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_conv_drain), sizeof(unsigned long long) * TG_DRAIN_REC * n,
                               sizeof(unsigned long long) * TG_DRAIN_REC * TG_DRAIN_CAP * (epi ? 1 : 0)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef TG_ATT_STAMP
int tg_debug_att_stamps(unsigned long long* out, int n) {
    if (n > 32) n = 32;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_att_stamp), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -1;
}
#endif

void tg_net_destroy(tg_ctx* ctx) {
    if (!ctx || !ctx->eng || !ctx->eng->net) return;
    Net* n = ctx->eng->net;
    if (n->pending) (void)hipEventSynchronize(n->loaded);
    void* ptrs[] = {n->bufA, n->bufB, n->bufH, n->x0, n->hc, n->own, n->bufQ, n->hca, n->bufAct, n->act16, n->h16, n->x0h, n->range};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (Net::WeightSet& w : n->sets) { void* q[] = {w.blob, w.wstage, w.wh, w.stem_h, w.head_h, w.wsc, w.head_g, w.head_ag, w.att_h, w.att_sc, w.head_x2, w.head_x2sc}; for (void* p : q) if (p) (void)hipFree(p); }
    if (n->side) (void)hipStreamDestroy(n->side);
    if (n->loaded) (void)hipEventDestroy(n->loaded);
    if (n->swapped) (void)hipEventDestroy(n->swapped);
    if (n->pinned) (void)hipHostFree(n->pinned);
    for (hipEvent_t ev : n->ev) (void)hipEventDestroy(ev);
    delete n;
    ctx->eng->net = nullptr;
}

// Move boundary of the engine (tg_sp_begin_move): a completed background refresh becomes the live set here, and only here.
int tg_net_adopt_ready(tg_ctx* ctx) {
    if (!ctx || !ctx->eng || !ctx->eng->net) return TG_OK;
    return adopt_pending(ctx, ctx->eng->net, /*wait=*/false);
}

int tg_net_forward(tg_ctx* ctx, int rows) {
    Engine* e = ctx->eng;
    if (!e || !e->net) TG_FAIL(ctx, TG_ERR_STATE, "no network weights loaded (tg_net_load)");
    return tg_net_forward_rows(ctx, rows, e->dev.row_slot, e->dev.policy, e->dev.value);
}

int tg_net_forward_rows(tg_ctx* ctx, int rows, const int32_t* slot, float* policy, float* value) {
    return tg_net_forward_rows_own(ctx, rows, slot, policy, value, nullptr);
}

// own == nullptr: the ownership head is not written (k_heads skips it), as the search has always run it
int tg_net_forward_rows_own(tg_ctx* ctx, int rows, const int32_t* slot, float* policy, float* value, float* own) {
    Engine* e = ctx->eng;
    if (!e || !e->net) TG_FAIL(ctx, TG_ERR_STATE, "no network weights loaded (tg_net_load)");
    Net* n = e->net;
    n->in_bits = e->dev.obs_bits; n->in_slot = slot; n->in_words = e->dev.obs_words;
    const int rc = forward_sym(ctx, n, nullptr, rows, policy, value, own);
    n->in_bits = nullptr; n->in_slot = nullptr;
    return rc;
}

// main_prediction on host buffers (model.py:17-20): obs f32[n][C][S][S] -> policy f32[n][A], value f32[n], own f32[n][P]
int tg_net_predict(tg_ctx* ctx, const float* obs, int n_rows, float* policy, float* value, float* own) {
    if (!ctx || !ctx->eng || !ctx->eng->net) { if (ctx) ctx->err = "no network weights loaded (tg_net_load)"; return TG_ERR_STATE; }
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    Net* n = ctx->eng->net;
    { int rc = adopt_pending(ctx, n, /*wait=*/false); if (rc) return rc; }      // a finished background refresh takes over between calls
    const size_t P = n->P, A = n->A, C = n->C;
    int done = 0;
    tg::DevBuf& din = ctx->env_f32; tg::DevBuf& dout = ctx->env_in;
    while (done < n_rows) {
        const int k = (n_rows - done) < n->rows_cap ? (n_rows - done) : n->rows_cap;
        if (din.reserve(sizeof(float) * k * C * P) || dout.reserve(sizeof(float) * k * (A + 1)))
            TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed (predict scratch)");
        float* d_pol = (float*)dout.p; float* d_val = d_pol + (size_t)k * A;
        TG_HIP(ctx, hipMemcpyAsync(din.p, obs + (size_t)done * C * P, sizeof(float) * k * C * P, hipMemcpyHostToDevice, ctx->stream));
        int rc = forward_sym(ctx, n, (const float*)din.p, k, d_pol, d_val, own ? n->own : nullptr);
        if (rc) return rc;
        TG_HIP(ctx, hipMemcpyAsync(policy + (size_t)done * A, d_pol, sizeof(float) * k * A, hipMemcpyDeviceToHost, ctx->stream));
        TG_HIP(ctx, hipMemcpyAsync(value + done, d_val, sizeof(float) * k, hipMemcpyDeviceToHost, ctx->stream));
        if (own) TG_HIP(ctx, hipMemcpyAsync(own + (size_t)done * P, n->own, sizeof(float) * k * P, hipMemcpyDeviceToHost, ctx->stream));
        TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        done += k;
    }
    return TG_OK;
}


// Range report (the reference runs f32 end to end, model.py:79-114, and hands over arbitrary trained checkpoints, model.py:23-27;
// the fp16-carrying precisions do not have f32's range).  fp16_overflows: sticky count, since the network was created, of epilogue
// tiles (convs) / boards (attention) in which a value beyond +-65504 was rounded to fp16 -- from there on the network computes
// inf / NaN; 0 = every forward pass so far stayed in range.  Always 0 with net_precision 0.  weight_absmax: largest |w| of the
// live weight set's BN-folded blob (inf / NaN if the blob holds one).  A non-zero count also leaves a message in tg_last_error.
int tg_net_stream_layout(tg_ctx* ctx, int* one_stream, int* act_copy) {
    if (!ctx || !ctx->eng || !ctx->eng->net) return TG_ERR_STATE;
    const Net* n = ctx->eng->net;
    if (one_stream) *one_stream = n->path.chain == CHAIN_DMA;
    if (act_copy) *act_copy = n->bufAct != nullptr;
    return TG_OK;
}

int tg_net_range(tg_ctx* ctx, uint64_t* fp16_overflows, float* weight_absmax) {
    if (!ctx || !ctx->eng || !ctx->eng->net) return TG_ERR_STATE;
    Net* n = ctx->eng->net;
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    unsigned host[4] = {0, 0, 0, 0};
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    TG_HIP(ctx, hipMemcpy(host, n->range, sizeof(host), hipMemcpyDeviceToHost));
    if (fp16_overflows) *fp16_overflows = host[0];
    if (weight_absmax) { float f; memcpy(&f, &host[1 + n->active], sizeof(f)); *weight_absmax = f; }
    if (host[0])
        ctx->err = "fp16 overflow: " + std::to_string(host[0]) + " epilogue tiles rounded a value beyond +-65504 to fp16 (net_precision " +
                   std::to_string(n->prec) + "); outputs since then may be inf/NaN -- use net_precision 0 for these weights";
    return TG_OK;
}

// HIP-event timing of the dominant kernel (3x3 conv F->F), measured on the stream the kernels are launched on.
int tg_prof_enable(tg_ctx* ctx, int on, int max_launches) {
    if (!ctx || !ctx->eng || !ctx->eng->net) return TG_ERR_STATE;
    Net* n = ctx->eng->net;
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if (on) {
        const size_t want = 2 * (size_t)(max_launches > 0 ? max_launches : 4096);
        while (n->ev.size() < want) { hipEvent_t ev; TG_HIP(ctx, hipEventCreate(&ev)); n->ev.push_back(ev); }
        n->ev_used = 0; n->conv_ms = 0; n->conv_launches = 0; n->conv_flops = 0; n->conv_skipped = 0;
    }
    n->prof = on != 0;
    return TG_OK;
}

int tg_prof_read(tg_ctx* ctx, double* conv_ms, int64_t* conv_launches, double* conv_flops) {
    if (!ctx || !ctx->eng || !ctx->eng->net) return TG_ERR_STATE;
    Net* n = ctx->eng->net;
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double ms = 0;
    for (size_t i = 0; i + 1 < n->ev_used; i += 2) {
        float t = 0; TG_HIP(ctx, hipEventElapsedTime(&t, n->ev[i], n->ev[i + 1])); ms += t;
    }
    n->conv_ms += ms; n->ev_used = 0;
    if (conv_ms) *conv_ms = n->conv_ms;
    if (conv_launches) *conv_launches = n->conv_launches;
    if (conv_flops) *conv_flops = n->conv_flops;
    return TG_OK;
}

// Launches of the dominant kernel that were NOT timed since tg_prof_enable(ctx, 1, n) because the event pool was full
// (tg_prof_read drains the pool into the running totals; 0 here = the totals cover every launch).
int tg_prof_skipped(tg_ctx* ctx, int64_t* launches) {
    if (!ctx || !ctx->eng || !ctx->eng->net) return TG_ERR_STATE;
    if (launches) *launches = ctx->eng->net->conv_skipped;
    return TG_OK;
}

}  // extern "C"
