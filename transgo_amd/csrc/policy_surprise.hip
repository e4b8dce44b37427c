// policy_surprise.hip -- policy surprise weighting (transgo_amd/policy_surprise.py holds the rule): the positions of
// the finished games are resampled on the device before they leave the harvest.  A position whose search target differs much from
// the raw network policy is written more often, an unsurprising one less often or not at all; a game keeps its weight T.
//
//   prior     one forward of the loaded network over the harvested positions, read from their bit-packed observations in chunks of
//             at most rows_cap rows, identity orientation, past the evaluation cache, into rows of its own (or the caller's rows)
//   k_psw_surprise   one wavefront per position: counts 1 -> 0, n, KL(pi || prior) in f64
//   k_psw_plan       one workgroup: per game sum of the surprises (sequential), weights, the counter-hash draw, copies; then the
//                    exclusive scan of the copies over the batch -> per-game n_moves, output offsets, source row of every output row
//   k_psw_gather     one wavefront per OUTPUT row: obs words, counts row, z, ownership row, player from its source row
//
// Nothing here is launched while the weight is 0, and no kernel of the other translation units changes.
#include <float.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "engine.h"

namespace tg {

struct PolicySurprise {
    double weight = 0.0;             // lambda; 0 = off
    uint32_t seed = 0;
    // the current plan: valid for the finished games of the tg_sp_play that made Engine::fin_seq what plan_seq says
    bool planned = false;
    uint64_t plan_seq = 0;
    int n_in = 0, n_out = 0, n_games = 0;
    DevBuf obs, cnt, z, own, pl;     // the plain harvest of those games, in HBM
    DevBuf prior;                    // [n_in][A] f32
    DevBuf ident, val;               // [rows_cap] identity slot table of the forward's input, its value outputs (not used)
    int ident_rows = 0;
    DevBuf game;                     // T i32[g] | off i32[g] | seed u32[g] | out_moves i32[g] | out_base i32[g + 1]
    DevBuf work;                     // surprise f64[n] | weight f64[n] | copies i32[n]
    DevBuf src;                      // [2 n + 1] source row of every output row
    DevBuf o_obs, o_cnt, o_z, o_own, o_pl;   // the gathered batch on its way to host arrays
    std::vector<int32_t> h_slot, h_moves, h_winner, h_game;
    std::vector<float> h_score;
    std::vector<int8_t> h_terr;
    uint64_t st_in = 0, st_out = 0, st_games = 0, st_rows = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double prior_ms = 0, plan_ms = 0, gather_ms = 0; long plans = 0;
    void release() {
        for (DevBuf* b : {&obs, &cnt, &z, &own, &pl, &prior, &ident, &val, &game, &work, &src, &o_obs, &o_cnt, &o_z, &o_own, &o_pl}) b->release();
        for (hipEvent_t& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    }
};

namespace {

constexpr uint32_t kPswDomain = 0x50535731u;           // "PSW1": xored into the seed, keeps these draws apart from the playout cap's
constexpr int kPlanThreads = 1024;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the splitmix64 finaliser and the 24-bit draw of rng_host.cpp (tg_host_cap_draw), on the device
__device__ __forceinline__ uint64_t psw_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint32_t psw_draw(uint32_t seed, int32_t t, uint32_t dseed) {
    return (uint32_t)(psw_mix(psw_mix(((uint64_t)dseed << 32) | seed) ^ (uint64_t)(uint32_t)t) >> 40);
}

// One wavefront per position.  A = 82 or 362: lanes stride the row by 64, the last stripe is partial.
__global__ __launch_bounds__(64) void k_psw_surprise(const int32_t* __restrict__ counts, const float* __restrict__ prior, int A, int n,
                                                     double* __restrict__ s_out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= n) return;
    const int32_t* c = counts + (size_t)r * A;
    const float* p = prior + (size_t)r * A;
    long long tot = 0;
    for (int a = lane; a < A; a += 64) { const int v = c[a]; tot += v == 1 ? 0 : v; }
    tot = wave_sum(tot);
    double acc = 0.0;
    if (tot != 0) {
        const double dn = (double)tot;
        for (int a = lane; a < A; a += 64) {
            const int v = c[a];
            if (v > 1) {                                               // c' > 0
                const double pi = (double)v / dn;
                double pa = (double)p[a];
                pa = pa > (double)FLT_MIN ? pa : (double)FLT_MIN;
                acc += pi * (log(pi) - log(pa));
            }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) s_out[r] = acc > 0.0 ? acc : 0.0;
}

// One workgroup of 1024 threads for the whole batch; thread i owns the games i, i + 1024, ...  Pass 1: the game's sum of surprises
// in recorded order, weights, draws, copies, and the game's total.  Pass 2: exclusive scan of the totals over the games (64-lane
// shuffle scan, the 16 wave totals through LDS, a carry from one block of 1024 games to the next).  Pass 3: the source row of every
// output row.  A game is a few hundred positions at the most and a harvest a few thousand rows, so one thread per game is enough.
__global__ __launch_bounds__(kPlanThreads) void k_psw_plan(const double* __restrict__ s, const int32_t* __restrict__ T,
                                                           const int32_t* __restrict__ off, const uint32_t* __restrict__ gseed, int ng,
                                                           double lam, uint32_t dseed, double* __restrict__ w_out,
                                                           int32_t* __restrict__ copies, int32_t* __restrict__ out_moves,
                                                           int32_t* __restrict__ out_base, int32_t* __restrict__ src, int src_cap) {
    __shared__ int wave_tot[kPlanThreads / 64];
    __shared__ int carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int g = tid; g < ng; g += kPlanThreads) {
        const int n = T[g], o = off[g];
        double tot = 0.0;
        for (int t = 0; t < n; ++t) tot = tot + s[o + t];
        const uint32_t gs = gseed[g];
        int total = 0;
        for (int t = 0; t < n; ++t) {
            const double w = tot > 0.0 ? (1.0 - lam) + lam * (double)n * s[o + t] / tot : 1.0;
            const double u = (double)psw_draw(gs, t, dseed) / 16777216.0;
            int k = (int)floor(w + u);
            if (k < 0) k = 0;
            w_out[o + t] = w; copies[o + t] = k; total += k;
        }
        out_moves[g] = total;
    }
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int g0 = 0; g0 < ng; g0 += kPlanThreads) {
        const int g = g0 + tid;
        const int own = g < ng ? out_moves[g] : 0;
        int v = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
        if (lane == 63) wave_tot[wv] = v;
        __syncthreads();
        int before = carry_s;
        for (int k = 0; k < wv; ++k) before += wave_tot[k];
        if (g < ng) out_base[g] = before + v - own;
        __syncthreads();
        if (tid == kPlanThreads - 1) carry_s = before + v;
        __syncthreads();
    }
    if (tid == 0) out_base[ng] = carry_s;
    for (int g = tid; g < ng; g += kPlanThreads) {
        const int n = T[g], o = off[g];
        int j = out_base[g];
        for (int t = 0; t < n; ++t)
            for (int k = copies[o + t]; k > 0; --k, ++j)
                if (j < src_cap) src[j] = o + t;
    }
}

// One wavefront per output row.
__global__ __launch_bounds__(64) void k_psw_gather(const int32_t* __restrict__ src, int n_out, int W, int A, int P,
                                                   const uint32_t* __restrict__ i_obs, const int32_t* __restrict__ i_cnt,
                                                   const float* __restrict__ i_z, const int8_t* __restrict__ i_own,
                                                   const uint8_t* __restrict__ i_pl, uint32_t* __restrict__ o_obs,
                                                   int32_t* __restrict__ o_cnt, float* __restrict__ o_z, int8_t* __restrict__ o_own,
                                                   uint8_t* __restrict__ o_pl) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= n_out) return;
    const size_t q = (size_t)src[r], d = (size_t)r;
    for (int i = lane; i < W; i += 64) o_obs[d * W + i] = i_obs[q * W + i];
    for (int i = lane; i < A; i += 64) o_cnt[d * A + i] = i_cnt[q * A + i];
    for (int i = lane; i < P; i += 64) o_own[d * P + i] = i_own[q * P + i];
    if (lane == 0) { o_z[d] = i_z[q]; if (o_pl) o_pl[d] = i_pl[q]; }
}

// k_psw_surprise + k_psw_plan on device arrays; everything on ctx->stream
int launch_plan(tg_ctx* ctx, const int32_t* d_cnt, const float* d_prior, int n, int ng, const int32_t* d_T, const int32_t* d_off,
                const uint32_t* d_seed, double lam, uint32_t seed, double* d_s, double* d_w, int32_t* d_copies, int32_t* d_moves,
                int32_t* d_base, int32_t* d_src, int src_cap) {
    if (n > 0) hipLaunchKernelGGL(k_psw_surprise, dim3(n), dim3(64), 0, ctx->stream, d_cnt, d_prior, ctx->A, n, d_s);
    hipLaunchKernelGGL(k_psw_plan, dim3(1), dim3(kPlanThreads), 0, ctx->stream, (const double*)d_s, d_T, d_off, d_seed, ng, lam,
                       seed ^ kPswDomain, d_w, d_copies, d_moves, d_base, d_src, src_cap);
    TG_HIP(ctx, hipGetLastError());
    return TG_OK;
}

size_t up8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

void psw_destroy(tg_ctx* ctx) {
    Engine* e = ctx->eng;
    if (!e || !e->psw) return;
    e->psw->release();
    delete e->psw;
    e->psw = nullptr;
}

}  // namespace tg

using namespace tg;

extern "C" {

#define NEED_ENGINE(ctx) do { if (!(ctx) || !(ctx)->eng || (ctx)->eng->G <= 0) return TG_ERR_ARG; TG_HIP(ctx, hipSetDevice((ctx)->cfg.device)); } while (0)

int tg_sp_policy_surprise(tg_ctx* ctx, double weight, uint32_t seed) {
    NEED_ENGINE(ctx);
    Engine* e = ctx->eng;
    if (!(weight >= 0.0 && weight <= 1.0))
        TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_policy_surprise: the weight must lie in [0, 1] (0 = off), got " + std::to_string(weight));
    if (weight > 0.0 && !e->dev.hist_obs)
        TG_FAIL(ctx, TG_ERR_STATE, "tg_sp_policy_surprise: the context was created with record_games = 0, there is nothing to resample");
    if (!e->psw) {
        if (weight == 0.0) return TG_OK;                               // off and never on: nothing is allocated
        e->psw = new PolicySurprise();
    }
    e->psw->weight = weight; e->psw->seed = seed;
    e->psw->planned = false;                                           // a plan made under other parameters is not current
    return TG_OK;
}

int tg_sp_policy_surprise_get(tg_ctx* ctx, double* weight, uint32_t* seed) {
    NEED_ENGINE(ctx);
    const PolicySurprise* s = ctx->eng->psw;
    if (weight) *weight = s ? s->weight : 0.0;
    if (seed) *seed = s ? s->seed : 0u;
    return TG_OK;
}

int tg_sp_policy_surprise_plan(tg_ctx* ctx, const float* prior, const uint32_t* game_seed, int32_t* n_out, double* surprise,
                               double* weight, int32_t* copies, float* prior_out) {
    NEED_ENGINE(ctx);
    Engine* e = ctx->eng;
    PolicySurprise* s = e->psw;
    if (!s || !(s->weight > 0.0))
        TG_FAIL(ctx, TG_ERR_STATE, "tg_sp_policy_surprise_plan: policy surprise weighting is off (tg_sp_policy_surprise with a weight above 0 first)");
    if (!game_seed) TG_FAIL(ctx, TG_ERR_ARG, "tg_sp_policy_surprise_plan: game_seed must not be NULL (the seed of the game in every slot)");
    if (!prior && !e->net)
        TG_FAIL(ctx, TG_ERR_STATE, "tg_sp_policy_surprise_plan: prior is NULL and no network weights are loaded (tg_net_load), "
                                   "pass the prior rows of the harvested positions instead");
    s->planned = false;
    const int nf = (int)e->fin_slot.size(), np = e->fin_positions, A = ctx->A, P = ctx->P, W = e->dev.obs_words;
    s->n_games = nf; s->n_in = np; s->n_out = 0;
    if (nf == 0) {
        s->planned = true; s->plan_seq = e->fin_seq;
        if (n_out) *n_out = 0;
        return TG_OK;
    }
    for (int i = 0; i < 4; ++i) if (!s->ev[i]) TG_HIP(ctx, hipEventCreate(&s->ev[i]));
    // 1. the plain harvest of the finished games, kept in HBM; its per-game tables on the host for the harvest call
    const size_t npa = np > 0 ? (size_t)np : 1;
    if (s->obs.reserve(sizeof(uint32_t) * npa * W) || s->cnt.reserve(sizeof(int32_t) * npa * A) || s->z.reserve(sizeof(float) * npa) ||
        s->own.reserve(npa * P) || s->pl.reserve(npa) || s->prior.reserve(sizeof(float) * npa * A) ||
        s->work.reserve(up8(npa * 20)) || s->src.reserve(sizeof(int32_t) * (2 * npa + 1)) || s->game.reserve(sizeof(int32_t) * (5 * (size_t)nf + 1)))
        TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed (policy surprise staging)");
    s->h_slot.resize(nf); s->h_moves.resize(nf); s->h_winner.resize(nf); s->h_score.resize(nf); s->h_terr.resize((size_t)nf * P);
    {
        int rc = tg_sp_harvest(ctx, (uint32_t*)s->obs.p, (int32_t*)s->cnt.p, (float*)s->z.p, (int8_t*)s->own.p, (uint8_t*)s->pl.p, 1,
                               s->h_slot.data(), s->h_moves.data(), s->h_winner.data(), s->h_score.data(), s->h_terr.data());
        if (rc) return rc;
    }
    // 2. the prior rows
    TG_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    float* d_prior = (float*)s->prior.p;
    if (prior) {
        if (np > 0) TG_HIP(ctx, hipMemcpyAsync(d_prior, prior, sizeof(float) * (size_t)np * A, hipMemcpyHostToDevice, ctx->stream));
    } else {
        const int cap = e->rows_cap;
        if (s->ident_rows < cap) {
            if (s->ident.reserve(sizeof(int32_t) * (size_t)cap) || s->val.reserve(sizeof(float) * (size_t)cap))
                TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed (policy surprise staging)");
            std::vector<int32_t> id(cap);
            for (int i = 0; i < cap; ++i) id[i] = i;
            TG_HIP(ctx, hipMemcpy(s->ident.p, id.data(), sizeof(int32_t) * (size_t)cap, hipMemcpyHostToDevice));
            s->ident_rows = cap;
        }
        // tg_net_forward_rows reads the rows it is given out of dev.obs_bits and goes through the context's symmetry mode.  For
        // the length of each call the engine's view of its batch buffer is pointed at the harvested observations and the mode is
        // set to none: the forward then runs on these rows in identity orientation, into prior rows of its own.  Only the host-side
        // pointer moves -- the buffer that holds a pending root batch, its slot table and its output rows are not touched -- and
        // the evaluation cache (eval_cache_run) is not on this path at all.  net.hip stays as it is.
        uint32_t* keep_bits = e->dev.obs_bits;
        const int keep_mode = ctx->sym.mode;
        int rc = TG_OK;
        for (int done = 0; done < np && rc == TG_OK; done += cap) {
            const int k = np - done < cap ? np - done : cap;
            e->dev.obs_bits = (uint32_t*)s->obs.p + (size_t)done * W;
            ctx->sym.mode = SYM_NONE;
            rc = tg_net_forward_rows(ctx, k, (const int32_t*)s->ident.p, d_prior + (size_t)done * A, (float*)s->val.p);
            e->dev.obs_bits = keep_bits;
            ctx->sym.mode = keep_mode;
            if (rc == TG_OK) s->st_rows += (uint64_t)k;
        }
        if (rc) return rc;
    }
    TG_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    // 3. surprise, weights, copies, offsets
    s->h_game.assign(3 * (size_t)nf, 0);
    for (int i = 0, o = 0; i < nf; ++i) {
        s->h_game[i] = s->h_moves[i]; s->h_game[nf + i] = o; o += s->h_moves[i];
        const uint32_t gs = game_seed[s->h_slot[i]];
        memcpy(&s->h_game[2 * (size_t)nf + i], &gs, sizeof(gs));
    }
    int32_t* d_T = (int32_t*)s->game.p; int32_t* d_off = d_T + nf; uint32_t* d_seed = (uint32_t*)(d_off + nf);
    int32_t* d_moves = (int32_t*)(d_seed + nf); int32_t* d_base = d_moves + nf;
    double* d_s = (double*)s->work.p; double* d_w = d_s + npa; int32_t* d_copies = (int32_t*)(d_w + npa);
    TG_HIP(ctx, hipMemcpyAsync(d_T, s->h_game.data(), sizeof(int32_t) * 3 * (size_t)nf, hipMemcpyHostToDevice, ctx->stream));
    const int src_cap = 2 * np + 1;
    {
        int rc = launch_plan(ctx, (const int32_t*)s->cnt.p, d_prior, np, nf, d_T, d_off, d_seed, s->weight, s->seed, d_s, d_w, d_copies,
                             d_moves, d_base, (int32_t*)s->src.p, src_cap);
        if (rc) return rc;
    }
    TG_HIP(ctx, hipEventRecord(s->ev[2], ctx->stream));
    int32_t total = 0;
    TG_HIP(ctx, hipMemcpyAsync(s->h_moves.data(), d_moves, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, ctx->stream));
    TG_HIP(ctx, hipMemcpyAsync(&total, d_base + nf, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (np > 0) {
        if (surprise) TG_HIP(ctx, hipMemcpyAsync(surprise, d_s, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
        if (weight) TG_HIP(ctx, hipMemcpyAsync(weight, d_w, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
        if (copies) TG_HIP(ctx, hipMemcpyAsync(copies, d_copies, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
        if (prior_out) TG_HIP(ctx, hipMemcpyAsync(prior_out, d_prior, sizeof(float) * (size_t)np * A, hipMemcpyDeviceToHost, ctx->stream));
    }
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (total < 0 || total >= src_cap) TG_FAIL(ctx, TG_ERR_STATE, "tg_sp_policy_surprise_plan: the copies do not add up (a weight outside what the rule allows)");
    float ms = 0;
    TG_HIP(ctx, hipEventElapsedTime(&ms, s->ev[0], s->ev[1])); s->prior_ms += ms;
    TG_HIP(ctx, hipEventElapsedTime(&ms, s->ev[1], s->ev[2])); s->plan_ms += ms;
    s->plans += 1;
    s->n_out = total;
    s->st_in += (uint64_t)np; s->st_out += (uint64_t)total; s->st_games += (uint64_t)nf;
    s->planned = true; s->plan_seq = e->fin_seq;
    if (n_out) *n_out = total;
    return TG_OK;
}

int tg_sp_policy_surprise_harvest(tg_ctx* ctx, uint32_t* obs_bits, int32_t* counts, float* z, int8_t* own, uint8_t* player,
                                  int device_out, int32_t* slot, int32_t* n_moves, int32_t* winner, float* score, int8_t* terr) {
    NEED_ENGINE(ctx);
    Engine* e = ctx->eng;
    PolicySurprise* s = e->psw;
    if (!s || !s->planned || s->plan_seq != e->fin_seq)
        TG_FAIL(ctx, TG_ERR_STATE, "tg_sp_policy_surprise_harvest: no plan is current for the games the last tg_sp_play finished "
                                   "(call tg_sp_policy_surprise_plan first)");
    const int nf = s->n_games, no = s->n_out, A = ctx->A, P = ctx->P, W = e->dev.obs_words;
    if (nf == 0) return TG_OK;
    if (no > 0) {
        if (!obs_bits || !counts || !z || !own) return TG_ERR_ARG;
        uint32_t* d_obs = obs_bits; int32_t* d_cnt = counts; float* d_z = z; int8_t* d_own = own; uint8_t* d_pl = player;
        if (!device_out) {
            if (s->o_obs.reserve(sizeof(uint32_t) * (size_t)no * W) || s->o_cnt.reserve(sizeof(int32_t) * (size_t)no * A) ||
                s->o_z.reserve(sizeof(float) * (size_t)no) || s->o_own.reserve((size_t)no * P) || s->o_pl.reserve((size_t)no))
                TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed (policy surprise staging)");
            d_obs = (uint32_t*)s->o_obs.p; d_cnt = (int32_t*)s->o_cnt.p; d_z = (float*)s->o_z.p; d_own = (int8_t*)s->o_own.p;
            d_pl = player ? (uint8_t*)s->o_pl.p : nullptr;
        }
        TG_HIP(ctx, hipEventRecord(s->ev[2], ctx->stream));
        hipLaunchKernelGGL(k_psw_gather, dim3(no), dim3(64), 0, ctx->stream, (const int32_t*)s->src.p, no, W, A, P,
                           (const uint32_t*)s->obs.p, (const int32_t*)s->cnt.p, (const float*)s->z.p, (const int8_t*)s->own.p,
                           (const uint8_t*)s->pl.p, d_obs, d_cnt, d_z, d_own, d_pl);
        TG_HIP(ctx, hipGetLastError());
        TG_HIP(ctx, hipEventRecord(s->ev[3], ctx->stream));
        if (!device_out) {
            TG_HIP(ctx, hipMemcpyAsync(obs_bits, d_obs, sizeof(uint32_t) * (size_t)no * W, hipMemcpyDeviceToHost, ctx->stream));
            TG_HIP(ctx, hipMemcpyAsync(counts, d_cnt, sizeof(int32_t) * (size_t)no * A, hipMemcpyDeviceToHost, ctx->stream));
            TG_HIP(ctx, hipMemcpyAsync(z, d_z, sizeof(float) * (size_t)no, hipMemcpyDeviceToHost, ctx->stream));
            TG_HIP(ctx, hipMemcpyAsync(own, d_own, (size_t)no * P, hipMemcpyDeviceToHost, ctx->stream));
            if (player) TG_HIP(ctx, hipMemcpyAsync(player, d_pl, (size_t)no, hipMemcpyDeviceToHost, ctx->stream));
        }
        TG_HIP(ctx, hipStreamSynchronize(ctx->stream));                // device outputs are complete on return as well
        float ms = 0;
        TG_HIP(ctx, hipEventElapsedTime(&ms, s->ev[2], s->ev[3])); s->gather_ms += ms;
    }
    for (int i = 0; i < nf; ++i) {
        if (slot) slot[i] = s->h_slot[i];
        if (n_moves) n_moves[i] = s->h_moves[i];
        if (winner) winner[i] = s->h_winner[i];
        if (score) score[i] = s->h_score[i];
    }
    if (terr) memcpy(terr, s->h_terr.data(), (size_t)nf * P);
    return TG_OK;
}

int tg_sp_policy_surprise_stats(tg_ctx* ctx, uint64_t* positions_in, uint64_t* positions_out, uint64_t* games, uint64_t* rows_forwarded) {
    NEED_ENGINE(ctx);
    const PolicySurprise* s = ctx->eng->psw;
    if (positions_in) *positions_in = s ? s->st_in : 0;
    if (positions_out) *positions_out = s ? s->st_out : 0;
    if (games) *games = s ? s->st_games : 0;
    if (rows_forwarded) *rows_forwarded = s ? s->st_rows : 0;
    return TG_OK;
}

int tg_prof_read_policy_surprise(tg_ctx* ctx, double* prior_ms, double* plan_ms, double* gather_ms, int64_t* plans) {
    NEED_ENGINE(ctx);
    const PolicySurprise* s = ctx->eng->psw;
    if (prior_ms) *prior_ms = s ? s->prior_ms : 0.0;
    if (plan_ms) *plan_ms = s ? s->plan_ms : 0.0;
    if (gather_ms) *gather_ms = s ? s->gather_ms : 0.0;
    if (plans) *plans = s ? s->plans : 0;
    return TG_OK;
}

int tg_policy_surprise_plan_arrays(tg_ctx* ctx, int n_games, const int32_t* n_moves, const uint32_t* game_seed, const int32_t* counts,
                                   const float* prior, double weight, uint32_t seed, int32_t* n_out, int32_t* n_moves_out,
                                   double* surprise, double* weight_out, int32_t* copies, int32_t* src, int src_cap) {
    if (!ctx) return TG_ERR_ARG;
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if (!(weight >= 0.0 && weight <= 1.0))
        TG_FAIL(ctx, TG_ERR_ARG, "tg_policy_surprise_plan_arrays: the weight must lie in [0, 1], got " + std::to_string(weight));
    if (n_games < 0 || (n_games > 0 && (!n_moves || !game_seed))) return TG_ERR_ARG;
    long long n64 = 0;
    for (int i = 0; i < n_games; ++i) { if (n_moves[i] < 0) return TG_ERR_ARG; n64 += n_moves[i]; }
    if (n64 > 0x3fffffffLL) TG_FAIL(ctx, TG_ERR_ARG, "tg_policy_surprise_plan_arrays: more than 2^30 positions");
    const int n = (int)n64, A = ctx->A, ng = n_games;
    if (n > 0 && (!counts || !prior)) return TG_ERR_ARG;
    const size_t npa = n > 0 ? (size_t)n : 1, nga = ng > 0 ? (size_t)ng : 1;
    const int cap = 2 * n + 1;
    DevBuf b_cnt, b_prior, b_game, b_work, b_src;
    auto done = [&](int rc) { b_cnt.release(); b_prior.release(); b_game.release(); b_work.release(); b_src.release(); return rc; };
    if (b_cnt.reserve(sizeof(int32_t) * npa * A) || b_prior.reserve(sizeof(float) * npa * A) || b_game.reserve(sizeof(int32_t) * (5 * nga + 1)) ||
        b_work.reserve(up8(npa * 20)) || b_src.reserve(sizeof(int32_t) * (size_t)cap)) {
        ctx->err = "hipMalloc failed (policy surprise staging)";
        return done(TG_ERR_HIP);
    }
    std::vector<int32_t> hg(3 * nga, 0);
    for (int i = 0, o = 0; i < ng; ++i) { hg[i] = n_moves[i]; hg[nga + i] = o; o += n_moves[i]; memcpy(&hg[2 * nga + i], &game_seed[i], 4); }
    int32_t* d_T = (int32_t*)b_game.p; int32_t* d_off = d_T + nga; uint32_t* d_seed = (uint32_t*)(d_off + nga);
    int32_t* d_moves = (int32_t*)(d_seed + nga); int32_t* d_base = d_moves + nga;
    double* d_s = (double*)b_work.p; double* d_w = d_s + npa; int32_t* d_copies = (int32_t*)(d_w + npa);
    hipError_t he = hipMemcpyAsync(d_T, hg.data(), sizeof(int32_t) * 3 * nga, hipMemcpyHostToDevice, ctx->stream);
    if (he == hipSuccess && n > 0) he = hipMemcpyAsync(b_cnt.p, counts, sizeof(int32_t) * (size_t)n * A, hipMemcpyHostToDevice, ctx->stream);
    if (he == hipSuccess && n > 0) he = hipMemcpyAsync(b_prior.p, prior, sizeof(float) * (size_t)n * A, hipMemcpyHostToDevice, ctx->stream);
    if (he != hipSuccess) { ctx->err = std::string("tg_policy_surprise_plan_arrays: ") + hipGetErrorString(he); return done(TG_ERR_HIP); }
    int rc = launch_plan(ctx, (const int32_t*)b_cnt.p, (const float*)b_prior.p, n, ng, d_T, d_off, d_seed, weight, seed, d_s, d_w, d_copies,
                         d_moves, d_base, (int32_t*)b_src.p, cap);
    if (rc) return done(rc);
    int32_t total = 0;
    he = hipMemcpyAsync(&total, d_base + ng, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess && n_moves_out && ng > 0) he = hipMemcpyAsync(n_moves_out, d_moves, sizeof(int32_t) * (size_t)ng, hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess && surprise && n > 0) he = hipMemcpyAsync(surprise, d_s, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess && weight_out && n > 0) he = hipMemcpyAsync(weight_out, d_w, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess && copies && n > 0) he = hipMemcpyAsync(copies, d_copies, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
    if (he == hipSuccess && src && total > 0 && total < cap) {
        const int m = total < src_cap ? total : src_cap;
        if (m > 0) he = hipMemcpy(src, b_src.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost);
    }
    if (he != hipSuccess) { ctx->err = std::string("tg_policy_surprise_plan_arrays: ") + hipGetErrorString(he); return done(TG_ERR_HIP); }
    if (n_out) *n_out = total;
    return done(TG_OK);
}

}  // extern "C"
