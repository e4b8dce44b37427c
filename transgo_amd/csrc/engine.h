// engine.h -- host-side engine state shared by engine.hip (tree) and net.hip (network)
#pragma once
#include <vector>

#include "ctx.h"
#include "tree_dev.h"

namespace tg {

enum { CNT_ROWS = 0, CNT_ACTIVE = 1, CNT_ERRORS = 2, CNT_N = 8 };
enum BatchKind { BATCH_NONE = 0, BATCH_ROOTS = 1, BATCH_LEAVES = 2 };

// Everything the tree kernels need, passed by value.
struct EngineDev {
    NodeRec* arena = nullptr;       // the chunk pool: [pool_chunks][chunk_slots] (tree_dev.h)
    int32_t* ring = nullptr;        // [pool_chunks] free ring of chunk ids
    PoolCtl* pool = nullptr;        // its counters
    int32_t* chunk_ids = nullptr;   // [G][2][max_chunks] chunk-id lists of the games' trees
    GameCtl* ctl = nullptr;         // [G]
    tg_mt19937* rng = nullptr;      // [G]  NumPy-legacy MT19937 stream per game
    int32_t* path_nodes = nullptr;  // [G][R][maxd]
    int32_t* path_len = nullptr;    // [G][R]
    int32_t* path_row = nullptr;    // [G][R]  slot (0..R-1) of the game's evaluation-batch entry that serves the path
    // Evaluation batch.  Game g writes the positions it wants evaluated into ITS OWN slots g*R + 0.. (env.encode bit-packed,
    // obs_words u32 each) and their number into game_nslot[g]; k_compact then turns the counts into dense rows: game_off[g] =
    // first row of game g, row_slot[row] = slot.  Rows are therefore ordered by game (deterministic), nothing is allocated with
    // atomics (round 1: ~16 k increments of one counter per wave cost a fifth of the tree stage), and the batch costs 104 B per
    // position instead of 3240 B of float planes; the network's input kernel gathers through row_slot.
    uint32_t* obs_bits = nullptr;   // [rows_cap = G*R][obs_words]
    int32_t* game_nslot = nullptr;  // [G]
    int32_t* game_off = nullptr;    // [G]
    int32_t* row_slot = nullptr;    // [rows_cap]
    uint8_t* game_act = nullptr;    // [G]  game was below its visit target when the wave started
    float* policy = nullptr;        // [rows_cap][A]
    float* value = nullptr;         // [rows_cap]
    int32_t* counters = nullptr;    // [CNT_N]
    // per-game record of the moves played so far (the observation/pi/player lists of self_play.py:917-926), ply-major per game
    uint32_t* hist_obs = nullptr;   // [G][hist_T][obs_words]  env.encode(root) bit-packed (bit i = plane-major flat index i)
    int32_t* hist_cnt = nullptr;    // [G][hist_T][A]          raw root visit counts
    uint8_t* hist_pl = nullptr;     // [G][hist_T]             side to move (1 / 2); bit 0x80 (kPlySkip): the ply is not a training position
    uint8_t* ply_skip = nullptr;    // [G]  != 0: the ply the next k_play plays is kept out of the harvest (tg_sp_begin_move_games sets it,
                                    //      k_play consumes it; every reset and restore clears it)
    int hist_T = 0, obs_words = 0, G = 0;
    SearchCfg sc;
    RulesCfg rules;
};

struct Net;                          // net.hip
struct EvalCache;                    // eval_cache.hip
struct PolicySurprise;               // policy_surprise.hip

struct Engine {
    int G = 0, R = 0, rows_cap = 0;
    EngineDev dev;
    BatchKind batch_kind = BATCH_NONE;
    bool batch_ready = false;
    bool all_reset = false;
    int last_rows = 0;
    int n_errors = 0;                // games parked in error as of the last counter read
    size_t arena_bytes = 0;
    double* d_noise = nullptr;
    int32_t* d_i32 = nullptr;
    float* d_f32 = nullptr;
    uint8_t* d_u8 = nullptr;
    tg_mt19937* h_rng = nullptr;     // pinned host mirror of dev.rng; authoritative while rng_on_host (the host-side draws of a
    bool rng_on_host = false;        // move -- choice(A, p) then the next Dirichlet -- share one round trip)
    std::vector<int32_t> h_moves;    // moves played per game, as of the last tg_sp_play
    std::vector<int32_t> fin_slot, fin_off;   // games finished by the last tg_sp_play (ascending slot) and their position offsets
    int fin_positions = 0;
    int32_t* d_fin = nullptr;        // [2][G] device copy of fin_slot / fin_off
    uint64_t fin_seq = 0;            // bumped whenever the list of finished games is replaced (play, reset, restore): a resampling plan
                                     // (policy_surprise.hip) is current only for the list it was made from
    DevBuf hv_obs, hv_cnt, hv_z, hv_own, hv_pl, hv_game;   // harvest staging when the caller wants host arrays
    DevBuf obs_f32;                  // float planes of the pending batch, only materialised for tg_sp_batch_obs (tests, host evaluators)
    DevBuf readout;                  // staging of tg_sp_root_children / tg_sp_pv, allocated by the first such call
    DevBuf snap_tab, snap_stage;     // snapshot.hip: scan offsets, and the packed snapshot on its way to / from a host buffer
    std::vector<double> h_noise;
    std::vector<int32_t> h_nchild;
    std::vector<int32_t> h_sims, h_rec;       // tg_sp_begin_move_games: the per-game budgets; tg_sp_play: recorded plies of the games it finished
    std::vector<uint8_t> h_flags;             // tg_sp_begin_move_games: noise switch [G] | skip switch [G]
    // forced playouts: k is context state (0 = off: only then are k_collect_forced / k_play_forced launched); the
    // per-game flag of a move in progress is set by k_begin, ended by k_play, cleared by every reset and restore
    double forced_k = 0.0;
    uint8_t* d_forced = nullptr;     // [G]  the move in progress began with root noise while k > 0
    unsigned long long* d_forced_stat = nullptr;   // [2]  root selections of forced games, those that met a forced child
    // Gumbel root search: m, c_visit, c_scale are context state (m = 0: off, no *_gumbel kernel is launched).  The
    // per-game flag has the forced flag's lifetime; the tables of a move are allocated when m is first set above 0.  The gl table
    // itself travels through d_noise / h_noise, which a Gumbel move leaves idle.
    int gumbel_m = 0;
    double gumbel_c_visit = 50.0, gumbel_c_scale = 1.0;
    uint8_t* d_gumbel = nullptr;     // [G]  the move in progress is a Gumbel move
    unsigned long long* d_gumbel_stat = nullptr;   // [2]  root selections of Gumbel games, those that fell back to the smallest effort
    int32_t* d_gumbel_n0 = nullptr;  // [G][A] by child index: c.n at the start of the move
    int32_t* d_gumbel_N0 = nullptr;  // [G]    root.n at the start of the move
    int32_t* d_gumbel_target = nullptr;   // [G][A] by action: the counts staged by tg_sp_gumbel_target
    uint8_t* d_gumbel_staged = nullptr;   // [G]    ... and for which games
    std::vector<double> h_gumbel;    // [G][A] the variates of one move (host)
    // Search ownership: context state, off by default -- only while it is on do these buffers exist, is k_absorb_own
    // launched in k_absorb's place and does the forward write its ownership head for the pending batch.  The accumulators are
    // cleared by every begin_move, reset and restore; they are not part of a snapshot.
    bool own_on = false;
    float* d_own = nullptr;          // [rows_cap][P] ownership rows of the pending batch (side to move's point of view)
    float* d_own_sum = nullptr;      // [G][P] sum over the move's absorbed simulations, Black's point of view
    int32_t* d_own_n = nullptr;      // [G]    how many simulations the sum holds
    Net* net = nullptr;
    EvalCache* cache = nullptr;      // tg_sp_eval_cache: nullptr = every pending row goes through the network (nothing else is launched)
    PolicySurprise* psw = nullptr;   // tg_sp_policy_surprise: nullptr until the weight is first set above 0
    // Pass-alive end: context state, off by default -- only while it is on is k_pa_end launched behind k_play / k_reset
    // and do tg_sp_harvest / tg_sp_final score with the pass-alive-aware area (pass_alive.hip).  Not part of a snapshot.
    bool pa_on = false;
    unsigned long long* d_pa_stat = nullptr;   // [2]  games ended by settlement, sum of their plies (allocated when the mode is first set)
    DevBuf pa_buf;                   // staging of tg_sp_root_pass_alive
    // HIP-event timing of the tree stage (k_collect, k_absorb) on the engine's stream, switched by tg_prof_enable
    bool tprof = false; std::vector<hipEvent_t> tev; size_t tev_used = 0; double collect_ms = 0, absorb_ms = 0; long tree_waves = 0;
    std::vector<char> tev_kind;
};

// eval_cache.hip -- the exact evaluation cache around tg_net_forward
int eval_cache_run(tg_ctx* ctx, int rows);      // the pending batch: probe, in-batch duplicates, forward on the rest, scatter + insert
void eval_cache_invalidate(tg_ctx* ctx);        // the evaluator changed (weights, precision, symmetry): no entry made so far may hit again
void eval_cache_destroy(tg_ctx* ctx);

// policy_surprise.hip -- policy surprise weighting
void psw_destroy(tg_ctx* ctx);

// pass_alive.hip -- pass-alive end.  pa_end_games: nothing is launched while the mode is off; d_mask = the games to look
// at (nullptr = every game), d_done / d_rec = k_play's outputs (nullptr behind a reset).  pa_harvest / pa_final: k_harvest / k_final
// with the pass-alive-aware area, same arguments.  All on ctx->stream.
int pa_end_games(tg_ctx* ctx, const uint8_t* d_mask, uint8_t* d_done, int32_t* d_rec);
int pa_harvest(tg_ctx* ctx, int nf, const int32_t* slot, const int32_t* off, uint32_t* o_obs, int32_t* o_cnt, float* o_z, int8_t* o_own,
               uint8_t* o_pl, int32_t* o_winner, float* o_score, int8_t* o_terr);
int pa_final(tg_ctx* ctx, float* d_score, float* d_terr, int32_t* d_winner);
void pa_destroy(tg_ctx* ctx);

// engine.hip -- search ownership: the accumulators of the games with d_mask[g] != 0 (nullptr = every game) := 0, on
// ctx->stream; nothing is launched while the mode is off
int own_clear(tg_ctx* ctx, const uint8_t* d_mask);

}  // namespace tg

extern "C" int tg_net_forward(tg_ctx* ctx, int rows);   // pending batch (obs_bits through row_slot) -> policy[rows], value[rows] on ctx->stream
// the same for `rows` rows listed in `slot` (entries of obs_bits), outputs row-indexed into the caller's buffers of >= rows rows
extern "C" int tg_net_forward_rows(tg_ctx* ctx, int rows, const int32_t* slot, float* policy, float* value);
// ... and with the ownership head written too: own[rows][P], the side to move's point of view (search ownership)
extern "C" int tg_net_forward_rows_own(tg_ctx* ctx, int rows, const int32_t* slot, float* policy, float* value, float* own);
extern "C" void tg_net_destroy(tg_ctx* ctx);
extern "C" int tg_net_adopt_ready(tg_ctx* ctx);         // tg_sp_begin_move: a completed background weight refresh becomes the live set
extern "C" int tg_net_load_arch(tg_ctx* ctx, const char* arch, const float* blob, size_t n_floats, int rows_cap);
