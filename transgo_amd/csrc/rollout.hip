// rollout.hip -- tg_env_rollout: uniformly random playouts of a batch of boards to the end of the game, one launch per call.
// One 64-lane workgroup per board, like k_env_step / k_env_query (env.hip); the board code is board_dev.h, the stream is the
// NumPy-legacy MT19937 of tree_dev.h (WaveRng), so a playout equals the loop
//     while not terminated and plies < budget:  pts = candidates(state);  a = S*S if not pts else rs.choice(pts);  step(a)
// over the reference's GoEnv and a np.random.RandomState bit for bit (a one-element choice makes no draw).
#include <climits>

#include "ctx.h"
#include "tree_dev.h"

using namespace tg;

namespace {

// The state stays in registers for the whole game; WaveLds + the twist scratch are the only LDS.  Every helper below is
// __forceinline__ (board_dev.h, tree_dev.h): at 19x19 an out-of-line call with a BoardWave<19> in a scratch frame is what
// DESIGN.md 8.4 describes, and tests/test_cabi_symbols.py keeps calls out of the code object.
template <int S>
__global__ __launch_bounds__(64) void k_env_rollout(const BoardState<S>* in, BoardState<S>* out, int n, RulesCfg cfg,
                                                    tg_mt19937* rng, const int32_t* max_plies, int policy, int32_t* plies,
                                                    uint8_t* done, int32_t* moves, int moves_cap) {
    using G = Geo<S>;
    __shared__ WaveLds<S> lds;
    __shared__ uint32_t mt_scratch[1248];
    const int g = blockIdx.x;
    if (g >= n) return;
    const int lane = lane_id();
    BoardWave<S> bw;
    bw.init(&lds);
    BoardState<S> st = in[g];
    WaveRng r; r.key = rng[g].key; r.pos = __builtin_amdgcn_readfirstlane(rng[g].pos); r.scratch = mt_scratch; r.draws = 0;
    // step_count grows by one per ply and the game ends when it passes max_step, so max_step + 1 plies always suffice: the bound
    // never cuts a game, it only makes the trip count finite whatever bytes arrive as a state
    int budget = max_plies ? max_plies[g] : INT_MAX;
    const int hard = cfg.max_step < 65535 ? cfg.max_step + 1 : 65536;
    budget = __builtin_amdgcn_readfirstlane(budget < hard ? budget : hard);
    int32_t* mv = moves ? moves + (size_t)g * moves_cap : nullptr;
    int np = 0;
    while (!st.terminated && np < budget) {
        const int player = st.next_player;
        bw.load_colors(st.bb[0], st.bb[1]);
        bw.analyze();
        uint64_t cand[G::NW];
        int k = 0;
#pragma unroll
        for (int w = 0; w < G::NW; ++w) {
            bool c = bw.pt[w] < G::P && bw.legal(w, st, player);                        // board.cc:467-489
            if (policy == TG_ROLLOUT_NOEYE) c = c && !bw.true_eye(w, player);           // go_env.cc:171-181
            cand[w] = ballot64(c);
            k += __popcll(cand[w]);
        }
        int a = G::P;                                                                   // pass only when no point is left
        if (k > 0) {
            const int idx = r.choice_index(k);
            int acc = 0;
            bool found = false;
#pragma unroll
            for (int w = 0; w < G::NW; ++w) {                                           // idx-th candidate in ascending point order
                const int c = __popcll(cand[w]);
                if (!found && idx < acc + c) { a = w * 64 + nth_set_bit(cand[w], idx - acc); found = true; }
                acc += c;
            }
        }
        bool ok;
        state_step(bw, st, a, cfg, /*check=*/false, &ok);
        if (mv && lane == 0 && np < moves_cap) mv[np] = a;
        ++np;
    }
    if (mv)
        for (int i = np + lane; i < moves_cap; i += 64) mv[i] = -1;
    if (lane == 0) {
        out[g] = st;
        rng[g].pos = r.pos;
        plies[g] = np;
        done[g] = st.terminated ? 1 : 0;
    }
}

}  // namespace

extern "C" int tg_env_rollout(tg_ctx* ctx, const void* in, void* out, int n, tg_mt19937* rng, const int32_t* max_plies, int policy,
                              int32_t* plies, uint8_t* done, int32_t* moves, int moves_cap) {
    if (!ctx || !in || !out || !rng || !plies || !done || n < 0) return TG_ERR_ARG;
    if (policy != TG_ROLLOUT_NOEYE && policy != TG_ROLLOUT_LEGAL) TG_FAIL(ctx, TG_ERR_ARG, "tg_env_rollout: unknown policy");
    int most = ctx->rules.max_step;
    if (max_plies) {
        most = 0;
        for (int i = 0; i < n; ++i) {
            if (max_plies[i] < 0) TG_FAIL(ctx, TG_ERR_ARG, "tg_env_rollout: negative ply budget");
            if (max_plies[i] > most) most = max_plies[i];
        }
    }
    for (int i = 0; i < n; ++i)                                                         // the kernel reads key[pos]
        if (rng[i].pos < 0 || rng[i].pos > 624) TG_FAIL(ctx, TG_ERR_ARG, "tg_env_rollout: stream position outside 0..624");
    if (moves && moves_cap < most)
        TG_FAIL(ctx, TG_ERR_ARG, max_plies ? "tg_env_rollout: moves_cap is smaller than the largest ply budget"
                                           : "tg_env_rollout: moves_cap is smaller than max_step");
    if (n == 0) return TG_OK;
    TG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t bytes = (size_t)n * ctx->state_bytes, rbytes = (size_t)n * sizeof(tg_mt19937);
    const size_t mbytes = moves ? (size_t)n * moves_cap * sizeof(int32_t) : 0;
    if (ctx->env_in.reserve(bytes) || ctx->env_out.reserve(bytes) || ctx->env_act.reserve((size_t)n * 4) ||
        ctx->env_i32.reserve((size_t)n * 4) || ctx->env_flags.reserve((size_t)n) || ctx->env_rng.reserve(rbytes) ||
        (mbytes && ctx->env_moves.reserve(mbytes)))
        TG_FAIL(ctx, TG_ERR_HIP, "hipMalloc failed (env scratch)");
    TG_HIP(ctx, hipMemcpyAsync(ctx->env_in.p, in, bytes, hipMemcpyHostToDevice, ctx->stream));
    TG_HIP(ctx, hipMemcpyAsync(ctx->env_rng.p, rng, rbytes, hipMemcpyHostToDevice, ctx->stream));
    if (max_plies) TG_HIP(ctx, hipMemcpyAsync(ctx->env_act.p, max_plies, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
#define TG_R(SZ)                                                                                                         \
    hipLaunchKernelGGL(k_env_rollout<SZ>, dim3(n), dim3(64), 0, ctx->stream, (const BoardState<SZ>*)ctx->env_in.p,       \
                       (BoardState<SZ>*)ctx->env_out.p, n, ctx->rules, (tg_mt19937*)ctx->env_rng.p,                      \
                       max_plies ? (const int32_t*)ctx->env_act.p : nullptr, policy, (int32_t*)ctx->env_i32.p,           \
                       (uint8_t*)ctx->env_flags.p, moves ? (int32_t*)ctx->env_moves.p : nullptr, moves_cap)
    if (ctx->S == 9) TG_R(9); else TG_R(19);
#undef TG_R
    TG_HIP(ctx, hipGetLastError());
    TG_HIP(ctx, hipMemcpyAsync(out, ctx->env_out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    TG_HIP(ctx, hipMemcpyAsync(rng, ctx->env_rng.p, rbytes, hipMemcpyDeviceToHost, ctx->stream));
    TG_HIP(ctx, hipMemcpyAsync(plies, ctx->env_i32.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    TG_HIP(ctx, hipMemcpyAsync(done, ctx->env_flags.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (moves) TG_HIP(ctx, hipMemcpyAsync(moves, ctx->env_moves.p, mbytes, hipMemcpyDeviceToHost, ctx->stream));
    TG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TG_OK;
}
