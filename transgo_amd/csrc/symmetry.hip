// symmetry.hip -- dihedral transforms around the network forward (tg_net_set_symmetry; DESIGN.md "Symmetry-aware evaluation").
//
// The network is trained on all eight dihedral images of every position (self_play.py:943-965; k_sample in replay.hip), so it
// may be asked about a position in any of them.  Evaluating row x under symmetry s: T_s on each of its C planes, the unchanged
// forward on the result, and the outputs mapped back -- p[sym_src(s, dst)] = p'[dst] for every board point, pass and value
// unchanged, ownership like the board part of p -- so the tree code sees the original orientation only.  Two kernels stand
// beside the forward:
//   k_sym_transform  rows of bit-packed planes (gathered through the batch's slot table) -> a dense staging batch under a per-row
//                    s, which the forward reads through its usual in_bits / in_slot / in_words binding; the engine's own
//                    obs_bits are only read (records and tg_sp_batch_obs read them too)
//   k_sym_backmap    the forward's policy / value / ownership from staging -> the destination through the inverse permutation,
//                    stored (fixed, position) or accumulated in f32 in the fixed order s = 0..7 (mean8)
// Both are plain HIP C++: they move a few MB beside a forward that takes milliseconds.
#include "engine.h"
#include "sym_dev.h"

namespace {

using tg::sym_src;

constexpr int kSymThreads = 128;
constexpr int kSymMaxWords = (13 * 361 + 31) / 32;     // the largest row: 13 planes of 19x19 = 4693 bits = 147 words
constexpr int kSymMaxP = 361;

// sym_of(seed, words): FNV-1a style mix over the row's words, murmur3's fmix32 to finish, top three bits.  uint32 arithmetic.
__device__ __forceinline__ int sym_of(uint32_t seed, const uint32_t* words, int W) {
    uint32_t h = seed ^ 0x9E3779B9u;
    for (int i = 0; i < W; ++i) h = (h ^ words[i]) * 0x01000193u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return (int)(h >> 29);
}

// One workgroup per row.  The row's W source words are staged in LDS (the unused high bits of the last word masked off, so the
// hash never depends on them), the row's s is chosen, and every lane assembles whole output words: output bit k = (plane ch,
// point d) is source bit (ch, sym_src(s, d)).  Planes are not word-aligned (81 and 361 are odd), so a word's 32 bits walk (ch, d)
// across plane boundaries; the source-point table of the row's s is built once per workgroup.
__global__ __launch_bounds__(kSymThreads) void k_sym_transform(const uint32_t* __restrict__ bits, const int32_t* __restrict__ slot,
                                                               uint32_t* __restrict__ out, int32_t* __restrict__ sym_of_row, int rows,
                                                               int S, int C, int W, int sel, uint32_t arg) {
    __shared__ uint32_t src[kSymMaxWords];
    __shared__ uint16_t perm[kSymMaxP];
    __shared__ int s_row;
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= rows) return;
    const int P = S * S, nbits = C * P;
    const uint32_t* in = bits + (size_t)(slot ? slot[row] : row) * W;
    for (int w = tid; w < W; w += kSymThreads) {
        uint32_t v = in[w];
        if (w == W - 1 && (nbits & 31)) v &= (1u << (nbits & 31)) - 1u;
        src[w] = v;
    }
    __syncthreads();
    if (tid == 0) {
        const int s = sel == tg::SYM_POSITION ? sym_of(arg, src, W) : (int)(arg & 7u);
        s_row = s;
        sym_of_row[row] = s;
    }
    __syncthreads();
    const int s = s_row;
    for (int d = tid; d < P; d += kSymThreads) perm[d] = (uint16_t)sym_src(s, d / S, d % S, S);
    __syncthreads();
    for (int w = tid; w < W; w += kSymThreads) {
        const int k0 = w * 32;
        int ch = k0 / P, d = k0 - ch * P;
        uint32_t word = 0;
        for (int b = 0; b < 32 && k0 + b < nbits; ++b) {
            const int sb = ch * P + perm[d];
            word |= ((src[sb >> 5] >> (sb & 31)) & 1u) << b;
            if (++d == P) { d = 0; ++ch; }
        }
        out[(size_t)row * W + w] = word;
    }
}

// tg_net_predict's float planes [rows][C*P] -> bit-packed rows of the same layout (bit i = plane-major flat index i), a bit set
// where the plane value is nonzero.  One lane per output word.
__global__ __launch_bounds__(256) void k_sym_pack(const float* __restrict__ obs, uint32_t* __restrict__ out, int rows, int nbits, int W) {
    const size_t total = (size_t)rows * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / W;
        const int k0 = (int)(i - row * W) * 32;
        uint32_t word = 0;
        for (int b = 0; b < 32 && k0 + b < nbits; ++b) word |= (obs[row * nbits + k0 + b] != 0.f ? 1u : 0u) << b;
        out[i] = word;
    }
}

__global__ __launch_bounds__(256) void k_sym_iota(int32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = i;
}

// acc 0: store; 1: add; 2: add, then * 0.125f (the eighth pass of mean8).  Two roundings, never contracted (-ffp-contract=off).
__device__ __forceinline__ void sym_put(float* dst, float v, int acc) {
    if (acc == 0) *dst = v;
    else if (acc == 1) *dst = *dst + v;
    else *dst = (*dst + v) * 0.125f;
}

// One workgroup per row: staging (transformed orientation) -> destination (original orientation), out of place.  sym_src(s, .)
// is a permutation of the board, so every destination element is touched by exactly one lane.
__global__ __launch_bounds__(kSymThreads) void k_sym_backmap(const float* __restrict__ pol_s, const float* __restrict__ val_s,
                                                             const float* __restrict__ own_s, const int32_t* __restrict__ sym_of_row,
                                                             float* __restrict__ pol, float* __restrict__ val, float* __restrict__ own,
                                                             int rows, int S, int acc) {
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= rows) return;
    const int P = S * S, A = P + 1;
    const int s = sym_of_row[row];
    for (int d = tid; d < P; d += kSymThreads) {
        const int j = sym_src(s, d / S, d % S, S);
        sym_put(pol + (size_t)row * A + j, pol_s[(size_t)row * A + d], acc);
        if (own) sym_put(own + (size_t)row * P + j, own_s[(size_t)row * P + d], acc);
    }
    if (tid == 0) {
        sym_put(pol + (size_t)row * A + P, pol_s[(size_t)row * A + P], acc);
        sym_put(val + row, val_s[row], acc);
    }
}

// HIP-event pair around one launch of either kernel (kind 0: transform, 1: back-map) while tg_prof_enable_symmetry is on
struct SymProfScope {
    tg::SymState& y; hipStream_t st; bool on;
    SymProfScope(tg_ctx* ctx, int kind) : y(ctx->sym), st(ctx->stream), on(false) {
        if (y.prof && y.ev_used + 2 <= y.ev.size()) {
            on = true; y.ev_kind[y.ev_used / 2] = (char)kind;
            (void)hipEventRecord(y.ev[y.ev_used], st);
        }
    }
    ~SymProfScope() { if (on) { (void)hipEventRecord(y.ev[y.ev_used + 1], st); y.ev_used += 2; } }
};

}  // namespace

namespace tg {

int sym_reserve(tg_ctx* ctx, int rows, int words, int A, int P, bool want_packed) {
    SymState& y = ctx->sym;
    if (words > kSymMaxWords || P > kSymMaxP) TG_FAIL(ctx, TG_ERR_ARG, "symmetry: rows of more than 147 words (13 planes of 19x19) are not supported");
    if (y.bits.reserve(sizeof(uint32_t) * (size_t)rows * words) || y.ident.reserve(sizeof(int32_t) * (size_t)rows) ||
        y.sym_of_row.reserve(sizeof(int32_t) * (size_t)rows) || y.pol.reserve(sizeof(float) * (size_t)rows * A) ||
        y.val.reserve(sizeof(float) * (size_t)rows) || y.own.reserve(sizeof(float) * (size_t)rows * P) ||
        (want_packed && y.packed.reserve(sizeof(uint32_t) * (size_t)rows * words)))
        TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed (symmetry staging)");
    if (y.ident_rows < rows) {                           // a grown table is a new allocation: fill all of it
        hipLaunchKernelGGL(k_sym_iota, dim3((rows + 255) / 256), dim3(256), 0, ctx->stream, (int32_t*)y.ident.p, rows);
        TG_HIP(ctx, hipGetLastError());
        y.ident_rows = rows;
    }
    return TG_OK;
}

int sym_pack(tg_ctx* ctx, const float* obs, int rows, int C, int P, int words) {
    int grid = (int)(((size_t)rows * words + 255) / 256); if (grid > 65535) grid = 65535;
    hipLaunchKernelGGL(k_sym_pack, dim3(grid), dim3(256), 0, ctx->stream, obs, (uint32_t*)ctx->sym.packed.p, rows, C * P, words);
    TG_HIP(ctx, hipGetLastError());
    return TG_OK;
}

int sym_transform(tg_ctx* ctx, const uint32_t* src, const int32_t* slot, int rows, int S, int C, int words, int sel, uint32_t arg) {
    SymState& y = ctx->sym;
    {
        SymProfScope ps(ctx, 0);
        hipLaunchKernelGGL(k_sym_transform, dim3(rows), dim3(kSymThreads), 0, ctx->stream, src, slot, (uint32_t*)y.bits.p,
                           (int32_t*)y.sym_of_row.p, rows, S, C, words, sel, arg);
    }
    TG_HIP(ctx, hipGetLastError());
    return TG_OK;
}

int sym_backmap(tg_ctx* ctx, float* policy, float* value, float* own, int rows, int S, int acc) {
    SymState& y = ctx->sym;
    {
        SymProfScope ps(ctx, 1);
        hipLaunchKernelGGL(k_sym_backmap, dim3(rows), dim3(kSymThreads), 0, ctx->stream, (const float*)y.pol.p, (const float*)y.val.p,
                           (const float*)y.own.p, (const int32_t*)y.sym_of_row.p, policy, value, own, rows, S, acc);
    }
    TG_HIP(ctx, hipGetLastError());
    return TG_OK;
}

}  // namespace tg

extern "C" {

int tg_net_set_symmetry(tg_ctx* ctx, int mode, uint32_t arg) {
    if (!ctx) return TG_ERR_ARG;
    if (mode < tg::SYM_NONE || mode > tg::SYM_MEAN8)
        TG_FAIL(ctx, TG_ERR_ARG, "tg_net_set_symmetry: mode must be 0 (none), 1 (fixed), 2 (position) or 3 (mean8), got " + std::to_string(mode));
    if (mode == tg::SYM_FIXED && arg > 7)
        TG_FAIL(ctx, TG_ERR_ARG, "tg_net_set_symmetry: a fixed symmetry is 0..7, got " + std::to_string(arg));
    if (ctx->eng && ctx->eng->batch_kind != tg::BATCH_NONE)
        TG_FAIL(ctx, TG_ERR_STATE, "tg_net_set_symmetry: the evaluator changes at a move boundary only (an evaluation batch is pending)");
    const uint32_t new_arg = (mode == tg::SYM_FIXED || mode == tg::SYM_POSITION) ? arg : 0u;
    if (mode != ctx->sym.mode || new_arg != ctx->sym.arg) tg::eval_cache_invalidate(ctx);
    ctx->sym.mode = mode;
    ctx->sym.arg = new_arg;
    return TG_OK;
}

int tg_net_get_symmetry(tg_ctx* ctx, int* mode, uint32_t* arg) {
    if (!ctx) return TG_ERR_ARG;
    if (mode) *mode = ctx->sym.mode;
    if (arg) *arg = ctx->sym.arg;
    return TG_OK;
}

int tg_net_symmetry_staging(tg_ctx* ctx, uint64_t* bytes) {
    if (!ctx || !bytes) return TG_ERR_ARG;
    *bytes = (uint64_t)ctx->sym.bytes();
    return TG_OK;
}

int tg_prof_enable_symmetry(tg_ctx* ctx, int on, int max_launches) {
    if (!ctx) return TG_ERR_ARG;
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    tg::SymState& y = ctx->sym;
    if (on) {
        const size_t want = 2 * (size_t)(max_launches > 0 ? max_launches : 1024);
        while (y.ev.size() < want) { hipEvent_t ev; TG_HIP(ctx, hipEventCreate(&ev)); y.ev.push_back(ev); }
        y.ev_kind.assign(y.ev.size() / 2, 0);
        y.ev_used = 0; y.transform_ms = 0; y.backmap_ms = 0; y.launches = 0;
    }
    y.prof = on != 0;
    return TG_OK;
}

int tg_prof_read_symmetry(tg_ctx* ctx, double* transform_ms, double* backmap_ms, int64_t* launches) {
    if (!ctx) return TG_ERR_ARG;
    tg::SymState& y = ctx->sym;
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i + 1 < y.ev_used; i += 2) {
        float t = 0; TG_HIP(ctx, hipEventElapsedTime(&t, y.ev[i], y.ev[i + 1]));
        (y.ev_kind[i / 2] ? y.backmap_ms : y.transform_ms) += t;
        y.launches++;
    }
    y.ev_used = 0;
    if (transform_ms) *transform_ms = y.transform_ms;
    if (backmap_ms) *backmap_ms = y.backmap_ms;
    if (launches) *launches = y.launches;
    return TG_OK;
}

}  // extern "C"
