// pass_alive.hip -- pass-alive analysis on the device: tg_env_pass_alive over caller states, the read-out of the
// games' roots, and the settled-game end of self-play (tg_sp_pass_alive): the kernels that run behind k_play / k_reset while the
// mode is on, and the harvest / final kernels that score with the pass-alive-aware area.  Everything here is launched only through
// these entry points or while the mode is on; no other translation unit's device code knows about it.
#include "engine.h"
#include "pass_alive_dev.h"

using namespace tg;

namespace {

constexpr int kMaxPlies = 512;                      // plies of one game's record (hist_T <= max_step <= 510, checked at engine create)

template <int S> __device__ __forceinline__ BlockHdr<S>* root_hdr(const EngineDev& d, int g) {
    NodeRec* arena = d.arena;
    return reinterpret_cast<BlockHdr<S>*>(arena + arena[d.ctl[g].root].block);
}

// status / settled / score / owner of one state, written with plain per-lane stores
template <int S>
__device__ __forceinline__ void pa_write(BoardWave<S>& bw, PaLds<S>* T, const BoardState<S>& st, float komi, size_t g, int8_t* status,
                                         uint8_t* settled, float* score, int8_t* owner) {
    using G = Geo<S>;
    int8_t s8[G::NW];
    uint8_t own[G::NW];
    bool is_settled;
    const float raw = pass_alive_area<S>(bw, T, st, s8, own, &is_settled);
#pragma unroll
    for (int k = 0; k < G::NW; ++k) {
        if (bw.pt[k] >= G::P) continue;
        if (status) status[g * G::P + bw.pt[k]] = s8[k];
        if (owner) owner[g * G::P + bw.pt[k]] = own[k] == 1 ? 1 : own[k] == 2 ? -1 : 0;
    }
    if (bw.lane == 0) {
        if (settled) settled[g] = is_settled ? 1 : 0;
        if (score) score[g] = raw - komi;
    }
}

template <int S>
__global__ __launch_bounds__(64) void k_env_pass_alive(const BoardState<S>* sts, int n, float komi, int8_t* status, uint8_t* settled,
                                                       float* score, int8_t* owner) {
    __shared__ WaveLds<S> lds;
    __shared__ PaLds<S> tab;
    const int g = blockIdx.x;
    if (g >= n) return;
    BoardWave<S> bw; bw.init(&lds);
    const BoardState<S> st = sts[g];
    pa_write<S>(bw, &tab, st, komi, (size_t)g, status, settled, score, owner);
}

template <int S>
__global__ __launch_bounds__(64) void k_root_pass_alive(EngineDev d, int8_t* status, uint8_t* settled) {
    __shared__ WaveLds<S> lds;
    __shared__ PaLds<S> tab;
    const int g = blockIdx.x;
    BoardWave<S> bw; bw.init(&lds);
    BoardState<S> st;
    if (d.arena[d.ctl[g].root].block >= 0) st = root_hdr<S>(d, g)->st; else state_reset(st);     // (a game parked without a root block)
    pa_write<S>(bw, &tab, st, d.rules.komi, (size_t)g, status, settled, nullptr, nullptr);
}

// Behind k_play (done_out / rec_out = its outputs) or k_reset (both nullptr; mask = the restarted games), before k_compact: a game
// that is still running and whose root is settled ends here -- the root state is terminated, the game finished, the evaluation of
// the root that k_play / k_reset asked for is withdrawn, and the recorded plies are counted as play_body counts them.
template <int S>
__global__ __launch_bounds__(64) void k_pa_end(EngineDev d, const uint8_t* mask, uint8_t* done_out, int32_t* rec_out, unsigned long long* stat) {
    using G = Geo<S>;
    __shared__ WaveLds<S> lds;
    __shared__ PaLds<S> tab;
    const int g = blockIdx.x, lane = lane_id();
    if (mask && !mask[g]) return;
    GameCtl* c = &d.ctl[g];
    if (c->finished || c->error) return;
    BoardWave<S> bw; bw.init(&lds);
    BlockHdr<S>* h = root_hdr<S>(d, g);
    const BoardState<S> st = h->st;
    if (st.terminated) return;
    int8_t s8[G::NW];
    pass_alive<S>(bw, &tab, st, s8);
    int nz = 0;
#pragma unroll
    for (int k = 0; k < G::NW; ++k) nz += __popcll(ballot64(bw.pt[k] < G::P && s8[k] == 0));
    if (nz) return;
    int rec = 0;
    const int t = c->moves;
    if (rec_out && d.hist_obs) {
        const int n = t < d.hist_T ? t : d.hist_T;
        const uint8_t* h_pl = d.hist_pl + (size_t)g * d.hist_T;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            rec += __popcll(ballot64(i < n && !(h_pl[i] & kPlySkip)));
        }
    }
    if (lane == 0) {
        h->st.terminated = 1;
        c->finished = 1; c->need_eval = 0; c->searching = 0; c->active = 0;
        d.game_nslot[g] = 0;
        if (done_out) done_out[g] = 1;
        if (rec_out) rec_out[g] = rec;
        atomicAdd(&stat[0], 1ull);
        atomicAdd(&stat[1], (unsigned long long)t);
    }
}

// k_harvest (engine.hip) with the final position scored by the pass-alive-aware area: same arrays, same order of positions.
template <int S>
__global__ __launch_bounds__(64) void k_harvest_pa(EngineDev d, const int32_t* slot, const int32_t* off, uint32_t* o_obs,
                                                   int32_t* o_cnt, float* o_z, int8_t* o_own, uint8_t* o_pl, int32_t* o_winner,
                                                   float* o_score, int8_t* o_terr) {
    using G = Geo<S>;
    __shared__ WaveLds<S> lds;
    __shared__ PaLds<S> tab;
    __shared__ int8_t terr_s[G::PPAD];
    __shared__ int16_t src_s[kMaxPlies];
    const int f = blockIdx.x, lane = lane_id();
    const int g = slot[f];
    const size_t base = (size_t)off[f];
    GameCtl* c = &d.ctl[g];
    int n = c->moves < d.hist_T ? c->moves : d.hist_T;
    n = n < kMaxPlies ? n : kMaxPlies;
    BoardWave<S> bw; bw.init(&lds);
    const BoardState<S> st = root_hdr<S>(d, g)->st;
    int8_t s8[G::NW];
    uint8_t owner[G::NW];
    bool is_settled;
    const float raw = pass_alive_area<S>(bw, &tab, st, s8, owner, &is_settled);
    const float sc = raw - d.rules.komi;
    const int winner = sc > 0.f ? kBlack : kWhite;
#pragma unroll
    for (int k = 0; k < G::NW; ++k) {
        const int8_t tv = owner[k] == 1 ? 1 : owner[k] == 2 ? -1 : 0;
        terr_s[bw.pt[k]] = tv;
        if (o_terr && bw.pt[k] < G::P) o_terr[(size_t)f * G::P + bw.pt[k]] = tv;
    }
    if (lane == 0) { if (o_winner) o_winner[f] = winner; if (o_score) o_score[f] = sc; }
    __syncthreads();
    const uint32_t* h_obs = d.hist_obs + (size_t)g * d.hist_T * d.obs_words;
    const int32_t* h_cnt = d.hist_cnt + (size_t)g * d.hist_T * G::A;
    const uint8_t* h_pl = d.hist_pl + (size_t)g * d.hist_T;
    int m = 0;                                                          // the plies without the kPlySkip mark, dense, in ply order
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool keep = i < n && !(h_pl[i] & kPlySkip);
        const uint64_t b = ballot64(keep);
        if (keep) src_s[m + __popcll(b & ((1ull << lane) - 1ull))] = (int16_t)i;
        m += __popcll(b);
    }
    __syncthreads();
    const int W = d.obs_words;
    for (int i = lane; i < m * W; i += 64) { const int tt = i / W, w = i - tt * W; o_obs[base * W + i] = h_obs[(size_t)src_s[tt] * W + w]; }
    for (int i = lane; i < m * G::A; i += 64) { const int tt = i / G::A, a = i - tt * G::A; o_cnt[base * G::A + i] = h_cnt[(size_t)src_s[tt] * G::A + a]; }
    for (int i = lane; i < m; i += 64) {
        const int pl = h_pl[src_s[i]] & ~kPlySkip;
        o_z[base + i] = pl == winner ? 1.f : -1.f;
        if (o_pl) o_pl[base + i] = (uint8_t)pl;
    }
    for (int i = lane; i < m * G::P; i += 64) {
        const int tt = i / G::P, p = i - tt * G::P;
        o_own[base * G::P + i] = (h_pl[src_s[tt]] & ~kPlySkip) == kBlack ? terr_s[p] : (int8_t)-terr_s[p];
    }
}

template <int S>
__global__ __launch_bounds__(64) void k_final_pa(EngineDev d, float* score, float* terr, int32_t* winner) {
    using G = Geo<S>;
    __shared__ WaveLds<S> lds;
    __shared__ PaLds<S> tab;
    const int g = blockIdx.x, lane = lane_id();
    BoardWave<S> bw; bw.init(&lds);
    const BoardState<S> st = root_hdr<S>(d, g)->st;
    int8_t s8[G::NW];
    uint8_t owner[G::NW];
    bool is_settled;
    const float sc = pass_alive_area<S>(bw, &tab, st, s8, owner, &is_settled) - d.rules.komi;
    if (lane == 0) { if (score) score[g] = sc; if (winner) winner[g] = sc > 0.f ? kBlack : kWhite; }
    if (terr)
#pragma unroll
        for (int k = 0; k < G::NW; ++k)
            if (bw.pt[k] < G::P) terr[(size_t)g * G::P + bw.pt[k]] = owner[k] == 1 ? 1.f : owner[k] == 2 ? -1.f : 0.f;
}

#define PA_LAUNCH(ctx, kern, grid, ...)                                                                            \
    do {                                                                                                           \
        if ((ctx)->S == 9) hipLaunchKernelGGL(kern<9>, dim3(grid), dim3(64), 0, (ctx)->stream, __VA_ARGS__);       \
        else hipLaunchKernelGGL(kern<19>, dim3(grid), dim3(64), 0, (ctx)->stream, __VA_ARGS__);                    \
        TG_HIP(ctx, hipGetLastError());                                                                            \
    } while (0)

}  // namespace

namespace tg {

int pa_end_games(tg_ctx* ctx, const uint8_t* d_mask, uint8_t* d_done, int32_t* d_rec) {
    Engine* e = ctx->eng;
    if (!e->pa_on) return TG_OK;
    PA_LAUNCH(ctx, k_pa_end, e->G, e->dev, d_mask, d_done, d_rec, e->d_pa_stat);
    return TG_OK;
}

int pa_harvest(tg_ctx* ctx, int nf, const int32_t* slot, const int32_t* off, uint32_t* o_obs, int32_t* o_cnt, float* o_z, int8_t* o_own,
               uint8_t* o_pl, int32_t* o_winner, float* o_score, int8_t* o_terr) {
    if (ctx->eng->dev.hist_T > kMaxPlies) TG_FAIL(ctx, TG_ERR_STATE, "pass-alive harvest: the game record is longer than 512 plies");
    PA_LAUNCH(ctx, k_harvest_pa, nf, ctx->eng->dev, slot, off, o_obs, o_cnt, o_z, o_own, o_pl, o_winner, o_score, o_terr);
    return TG_OK;
}

int pa_final(tg_ctx* ctx, float* d_score, float* d_terr, int32_t* d_winner) {
    PA_LAUNCH(ctx, k_final_pa, ctx->eng->G, ctx->eng->dev, d_score, d_terr, d_winner);
    return TG_OK;
}

void pa_destroy(tg_ctx* ctx) {
    Engine* e = ctx->eng;
    if (!e) return;
    if (e->d_pa_stat) (void)hipFree(e->d_pa_stat);
    e->d_pa_stat = nullptr; e->pa_on = false;
    e->pa_buf.release();
}

}  // namespace tg

extern "C" {

int tg_env_pass_alive(tg_ctx* ctx, const void* states, int n, int8_t* status, uint8_t* settled, float* score, int8_t* owner) {
    if (!ctx || !states || !status || n < 0) return TG_ERR_ARG;
    if (n == 0) return TG_OK;
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t P = ctx->P, bytes = (size_t)n * ctx->state_bytes;
    // device layout: u8 = [status n*P][owner n*P][settled n]; f32 = [score n]
    if (ctx->env_in.reserve(bytes) || ctx->env_u8.reserve(n * (2 * P + 1)) || ctx->env_f32.reserve(sizeof(float) * n))
        TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed (env scratch)");
    int8_t* d_status = (int8_t*)ctx->env_u8.p; int8_t* d_owner = d_status + n * P; uint8_t* d_settled = (uint8_t*)(d_owner + n * P);
    float* d_score = (float*)ctx->env_f32.p;
    TG_HIP(ctx, hipMemcpyAsync(ctx->env_in.p, states, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (ctx->S == 9)
        hipLaunchKernelGGL(k_env_pass_alive<9>, dim3(n), dim3(64), 0, ctx->stream, (const BoardState<9>*)ctx->env_in.p, n, ctx->rules.komi,
                           d_status, settled ? d_settled : nullptr, score ? d_score : nullptr, owner ? d_owner : nullptr);
    else
        hipLaunchKernelGGL(k_env_pass_alive<19>, dim3(n), dim3(64), 0, ctx->stream, (const BoardState<19>*)ctx->env_in.p, n, ctx->rules.komi,
                           d_status, settled ? d_settled : nullptr, score ? d_score : nullptr, owner ? d_owner : nullptr);
    TG_HIP(ctx, hipGetLastError());
    TG_HIP(ctx, hipMemcpyAsync(status, d_status, n * P, hipMemcpyDeviceToHost, ctx->stream));
    if (owner) TG_HIP(ctx, hipMemcpyAsync(owner, d_owner, n * P, hipMemcpyDeviceToHost, ctx->stream));
    if (settled) TG_HIP(ctx, hipMemcpyAsync(settled, d_settled, n, hipMemcpyDeviceToHost, ctx->stream));
    if (score) TG_HIP(ctx, hipMemcpyAsync(score, d_score, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TG_OK;
}

#define PA_NEED_ENGINE(ctx) do { if (!(ctx) || !(ctx)->eng || (ctx)->eng->G <= 0) return TG_ERR_ARG; TG_HIP(ctx, hipSetDevice((ctx)->cfg.device)); } while (0)

int tg_sp_pass_alive(tg_ctx* ctx, int on) {
    PA_NEED_ENGINE(ctx);
    Engine* e = ctx->eng;
    if (e->batch_kind == BATCH_LEAVES) TG_FAIL(ctx, TG_ERR_STATE, "tg_sp_pass_alive: a leaf batch is pending");
    if (on && !e->d_pa_stat) {
        TG_HIP(ctx, hipMalloc((void**)&e->d_pa_stat, 2 * sizeof(unsigned long long)));
        TG_HIP(ctx, hipMemsetAsync(e->d_pa_stat, 0, 2 * sizeof(unsigned long long), ctx->stream));
        TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    e->pa_on = on != 0;
    return TG_OK;
}

int tg_sp_pass_alive_get(tg_ctx* ctx, int* on) {
    PA_NEED_ENGINE(ctx);
    if (on) *on = ctx->eng->pa_on ? 1 : 0;
    return TG_OK;
}

int tg_sp_pass_alive_stats(tg_ctx* ctx, uint64_t* games_settled, uint64_t* plies_at_settlement_sum) {
    PA_NEED_ENGINE(ctx);
    Engine* e = ctx->eng;
    unsigned long long h[2] = {0, 0};
    if (e->d_pa_stat) {
        TG_HIP(ctx, hipMemcpyAsync(h, e->d_pa_stat, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (games_settled) *games_settled = h[0];
    if (plies_at_settlement_sum) *plies_at_settlement_sum = h[1];
    return TG_OK;
}

int tg_sp_root_pass_alive(tg_ctx* ctx, int8_t* status, uint8_t* settled) {
    PA_NEED_ENGINE(ctx);
    Engine* e = ctx->eng;
    if (!e->all_reset) TG_FAIL(ctx, TG_ERR_STATE, "tg_sp_root_pass_alive: no game has a root yet (tg_sp_reset first)");
    const size_t G = e->G, P = ctx->P;
    if (e->pa_buf.reserve(G * (P + 1))) TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed");
    int8_t* d_status = (int8_t*)e->pa_buf.p; uint8_t* d_settled = (uint8_t*)(d_status + G * P);
    PA_LAUNCH(ctx, k_root_pass_alive, e->G, e->dev, d_status, d_settled);
    if (status) TG_HIP(ctx, hipMemcpyAsync(status, d_status, G * P, hipMemcpyDeviceToHost, ctx->stream));
    if (settled) TG_HIP(ctx, hipMemcpyAsync(settled, d_settled, G, hipMemcpyDeviceToHost, ctx->stream));
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TG_OK;
}

}  // extern "C"
