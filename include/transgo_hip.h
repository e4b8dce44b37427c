/*
 * transgo_hip.h -- C ABI of libtransgo_hip.so, the MI355X-native drop-in for Transgo's self-play hot path.
 *
 * Plain C, plain pointers and sizes, no torch types.  Every entry point names the reference interface it replaces
 * (file:line under /root/reference).  Unless a parameter says "device", pointers are HOST memory owned by the caller;
 * the library never keeps a caller pointer after a call returns.  All functions return 0 on success or a negative
 * tg_status; tg_last_error() gives the message.  A context is single-owner (one host thread, one GPU).
 *
 * Four groups (the fourth = the reference's own 15 names, for binding-compatibility):
 *   1. tg_env_*   batched form of the 15 extern "C" functions of GoEnv/cpp_src/go_env.h:24-70 over opaque state blobs
 *                 (what GoEnv/environment.py:42-90 binds through ctypes today).
 *   2. tg_sp_*    the batched self-play engine: G concurrent games, WP_MCTS (self_play.py:575-875) as HIP tree
 *                 kernels + the policy/value network forward (model.py:79-114) on MFMA.
 *   3. tg_host_*  host-only helpers that must be bit-identical to NumPy's legacy MT19937 stream
 *                 (np.random.dirichlet / choice used at self_play.py:93, :709, :683).
 */
#ifndef TRANSGO_HIP_H_
#define TRANSGO_HIP_H_

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tg_ctx tg_ctx;

typedef enum tg_status {
    TG_OK = 0,
    TG_ERR_ARG = -1,        /* bad argument / unsupported configuration */
    TG_ERR_HIP = -2,        /* HIP runtime error (message has the HIP error string) */
    TG_ERR_NO_DEVICE = -3,  /* no usable GPU: the library has no CPU fallback */
    TG_ERR_ARENA = -4,      /* a game's tree hit its cap (cfg.arena_slots) or found the shared pool empty (results of that game are invalid) */
    TG_ERR_STATE = -5       /* call sequence violated (e.g. absorb without collect) */
} tg_status;

/* Replaces: compile-time BOARD_SIZE (go_comm.h:20), Init(history_dim, encode_dim, max_step, komi) (go_env.h:30,
 * environment.py:43-45) and the search fields of configure.py:9-37.  Zero-initialise, then set what you need;
 * tg_config_default() fills the reference defaults. */
typedef struct tg_config {
    int32_t board_size;         /* 9 or 19 */
    int32_t encode_dim;         /* 9, 10 or 13 feature planes (environment.py:36; go_env.cc:96-115) */
    int32_t max_step;           /* environment.py:37 (120) */
    float komi;                 /* environment.py:38 (7.5) */
    int32_t n_games;            /* concurrent boards G; 0 = rules-only context */
    int32_t num_simulation;     /* configure.py:29 */
    int32_t parallel_readouts;  /* configure.py:33 (4); 1..8 */
    int32_t wu_loss;            /* configure.py:32 (2) */
    double c_puct1;             /* configure.py:26 (3) */
    double c_puct2;             /* configure.py:27 (0.05) */
    int32_t arena_slots;        /* most 32-byte tree slots ONE game's tree may hold (per-game cap); 0 = (4*num_simulation + 256) blocks of
                                   the largest size.  Memory is set by pool_slots below, not by this */
    int32_t net_blocks;         /* residual blocks of the tower (BASELINE.json "N-block x F-filter") */
    int32_t net_filters;        /* channels F (multiple of 32) */
    int32_t device;             /* HIP device ordinal */
    int32_t net_precision;      /* 0 = f32 network (default); 1 = fp16 weights/activations, f32 accumulate (BASELINE config 5), f32
                                   residual stream; 2 = as 1 with the residual stream stored in fp16 too (a quarter less HBM traffic);
                                   3 = split precision, opt-in: every conv operand as fp16 hi + lo, three of the four partial products (lo*lo dropped) on the
                                   fp16 matrix cores, f32 accumulate and residual stream (fp32-level accuracy at 2.4-3.1x the
                                   simulations/s).  1 and 2 take towers of 128 / 256 filters; attention layers (the reference's
                                   MainNetwork) are taken by 0 at 9x9 (every width) and at 19x19 with 128 / 256 filters (k_attention_t), by 1 at
                                   9x9 with 128 filters and by 3 at 9x9, never by 2, and by neither 1 nor 3 at 19x19; anything else is
                                   refused by tg_net_load */
    int32_t record_games;       /* 1 (default): every game's move record -- env.encode(root) bit-packed, raw visit counts, side to
                                   move; the three Python lists of self_play.py:917-926 -- is kept in HBM for tg_sp_harvest */
    int32_t pool_slots;         /* tree memory: 32-byte slots provisioned PER GAME ON AVERAGE in the pool all games of the context share
                                   (pool = n_games x this; a game takes chunks from it as its tree grows and returns them when it is
                                   re-rooted or restarted); 0 = (2*num_simulation + 128) blocks of the largest size.  tg_sp_pool_stats
                                   reports the fill; a game that finds the pool empty is parked like one that hits its cap */
    int32_t reserved[5];
} tg_config;

void tg_config_default(tg_config* cfg);

/* Lifetime.  tg_create fails with TG_ERR_NO_DEVICE when no GPU is present (there is no CPU path). */
int tg_create(const tg_config* cfg, tg_ctx** out);
void tg_destroy(tg_ctx* ctx);
const char* tg_last_error(const tg_ctx* ctx);       /* ctx may be NULL: last creation error */
int tg_sync(tg_ctx* ctx);                            /* wait for the context's stream */
int tg_version(void);

/* ---- 1. rules engine over caller-owned opaque states ---------------------------------------------------------------
 * A state is tg_state_size() bytes (48 at 9x9, 112 at 19x19); the reference's is a 1188-byte GoState
 * (go_env.h:15-18) that Python also treats as opaque (environment.py:93-103).  `states` arrays are n contiguous
 * blobs. */
int tg_state_size(const tg_ctx* ctx);

/* Reset (go_env.h:33, go_env.cc:34-41). */
int tg_env_reset(tg_ctx* ctx, void* states, int n);

/* Step (go_env.h:37, go_env.cc:44-80): out[i] = in[i] advanced by actions[i]; action S*S (or -1) is pass.
 * done[i] = game over (double pass or step_count > max_step).  An illegal action leaves the state unchanged with
 * done=0 and ok[i]=0 (the reference prints a message, go_env.cc:75-79); stepping a finished state returns done=1
 * unchanged (go_env.cc:52-55).  in may equal out (Step_, go_env.h:38).  ok may be NULL. */
int tg_env_step(tg_ctx* ctx, const void* in, void* out, const int32_t* actions, int n, uint8_t* done, uint8_t* ok);

/* One pass computing any subset of the read-only queries; NULL outputs are skipped.
 *   legal  u8[n][A]   getLegalAction (go_env.h:57, go_env.cc:154-164): 1 for every legal point, legal[A-1] (pass)
 *                     always 1 -- the pass filter of environment.py:121-129 is the caller's, as in the reference.
 *   noeye  u8[n][A]   getLegalNoEye (go_env.h:60, go_env.cc:171-181).
 *   obs    f32[n][C][S][S]  Encode (go_env.h:48, board_feature.cc:213-253).
 *   score  f32[n]     getScore = Tromp-Taylor - komi (go_env.h:51, go_env.cc:126-130).
 *   terr   f32[n][S*S] getTerritory: +1 black, 0 dame, -1 white (go_env.h:54, go_env.cc:136-149).
 *   player i32[n], step i32[n], terminated u8[n]: getPlayer / getStep / isTerminated (go_env.h:66,69,45). */
int tg_env_query(tg_ctx* ctx, const void* states, int n, uint8_t* legal, uint8_t* noeye, float* obs, float* score,
                 float* terr, int32_t* player, int32_t* step, uint8_t* terminated);

/* Pass-alive groups and territory (Benson's algorithm; transgo_amd/pass_alive.py is the definition).  Per state:
 *   status  i8[n][S*S]  +2 pass-alive Black stone, +1 Black pass-alive territory (an empty point or a dead White stone), -2 / -1
 *                       White likewise, 0 everything else.
 *   settled u8[n]       1 if no point has status 0.
 *   owner   i8[n][S*S]  the pass-alive-aware area: the status' colour where it is not 0, Tromp-Taylor elsewhere (+1 / -1 / 0 dame).
 *   score   f32[n]      #Black - #White of owner, minus komi; Black wins iff score > 0.
 * settled, score and owner may be NULL.  States, outputs and errors follow tg_env_query. */
int tg_env_pass_alive(tg_ctx* ctx, const void* states, int n, int8_t* status /*[n][S*S]*/, uint8_t* settled /*[n] or NULL*/,
                      float* score /*[n] or NULL*/, int8_t* owner /*[n][S*S] or NULL*/);

/* Show (go_env.h:63): prints the board of one state to stdout. */
int tg_env_show(tg_ctx* ctx, const void* state);


/* NumPy legacy RandomState stream: key/pos are get_state()[1] / get_state()[2]. */
typedef struct tg_mt19937 {
    uint32_t key[624];
    int32_t pos;
} tg_mt19937;

/* Uniformly random playouts, the whole game in ONE kernel launch (the reference plays them ply by ply on the host:
 * test_trans.py:14-23 RandomBot, :60-95 evaluate2, over getLegalAction / getLegalNoEye, environment.py:121-129, :161-164).
 * Candidate policies: */
#define TG_ROLLOUT_NOEYE 0      /* getLegalNoEye without its trailing pass (go_env.cc:171-181): own true eyes are never filled */
#define TG_ROLLOUT_LEGAL 1      /* the pass-filtered getLegalAction of environment.py:121-129: what RandomBot draws from */
/* Per board i, with rs = np.random.RandomState at rng[i] (NumPy's legacy stream, not Python's `random`):
 *     plies = 0
 *     while not terminated(state) and plies < max_plies[i]:
 *         pts = candidates(state)                     # ascending points, pass excluded
 *         a = S*S if len(pts) == 0 else rs.choice(pts)    # a one-element choice makes NO draw
 *         state, done = Step(state, a);  moves[i][plies] = a;  plies += 1
 * out[i] = the last state, rng[i] = the stream behind the last draw, plies[i], done[i] = terminated (double pass or step_count >
 * max_step, as tg_env_step reports it); moves i32[n][moves_cap] (may be NULL) holds -1 behind the last ply.  max_plies NULL = play
 * every game to its end.  A board that arrives terminated, or whose budget is 0, comes back unchanged with plies 0 and its stream
 * untouched.  TG_ERR_ARG: unknown policy, a negative budget, a stream position outside 0..624, `moves` with moves_cap smaller than
 * the largest budget (or than max_step when max_plies is NULL).  in may equal out. */
int tg_env_rollout(tg_ctx* ctx, const void* in, void* out, int n, tg_mt19937* rng /*[n], in and out*/,
                   const int32_t* max_plies /*[n] or NULL*/, int policy, int32_t* plies /*[n]*/, uint8_t* done /*[n]*/,
                   int32_t* moves /*[n][moves_cap] or NULL*/, int moves_cap);

/* ---- 2. batched self-play engine (needs cfg.n_games > 0) -----------------------------------------------------------------
 * G games advance in lock step.  One move of every game is:
 *     tg_sp_begin_move -> { tg_sp_collect -> evaluate -> tg_sp_absorb } until no game is active
 *                      -> tg_sp_root_info (visit counts) -> host picks moves -> tg_sp_play -> evaluate -> tg_sp_expand_roots
 * "evaluate" is tg_sp_eval (network forward on the GPU) or, for parity tests with a stand-in evaluator,
 * tg_sp_batch_obs + tg_sp_set_eval.  tg_sp_search runs the whole inner loop with the network.
 * An evaluation batch is a compact array of rows; rows belong either to fresh roots or to the leaves of one wave. */

/* WP_MCTS.reset_root (self_play.py:595-605) for every game (mask NULL) or the games with mask[g] != 0:
 * empty board, np.random.seed(seeds[g]) for the game's stream.  Leaves a root batch pending. */
int tg_sp_reset(tg_ctx* ctx, const uint32_t* seeds, const uint8_t* mask);

/* WP_MCTS.select_action prologue (self_play.py:689-700): a fresh root at the given position for every game with
 * mask[g] != 0 (mask NULL = all); unmasked slots are parked and take no part in searches.  `states` = G blobs of
 * tg_state_size() bytes.  RNG streams are left as they are.  Leaves a root batch pending. */
int tg_sp_reset_from(tg_ctx* ctx, const void* states, const uint8_t* mask);
/* Current root position of every game (G blobs), e.g. to hand a game from one engine to another. */
int tg_sp_root_states(tg_ctx* ctx, void* states);

int tg_sp_batch_rows(tg_ctx* ctx, int32_t* n_rows);                        /* rows of the pending batch */
int tg_sp_batch_obs(tg_ctx* ctx, float* obs /*[n_rows][C][S][S]*/, int32_t n_rows);   /* env.encode of each row (self_play.py:798) */
int tg_sp_set_eval(tg_ctx* ctx, const float* policy /*[n_rows][A]*/, const float* value /*[n_rows]*/, int32_t n_rows);
int tg_sp_eval(tg_ctx* ctx);                                               /* model.main_prediction on the pending batch (self_play.py:777-786) */
int tg_sp_expand_roots(tg_ctx* ctx);                                       /* root.expand with raw priors (self_play.py:603-605, :867-870) */

/* get_action_probs prologue (self_play.py:659-663): Dirichlet(0.03) root noise when selfplay != 0, and the visit
 * target N0 + num_simulation (<= 0: cfg.num_simulation). */
int tg_sp_begin_move(tg_ctx* ctx, int selfplay, int num_simulation);
/* The same prologue with a per-game noise switch, visit budget and record switch (playout cap randomization):
 * noise u8[G] (NULL = no game is noised): Dirichlet root noise for the games with noise[g] != 0 only -- the MT19937 stream of
 * any other game is not advanced; num_simulation i32[G]: the game's target is N0 + num_simulation[g] (<= 0: cfg.num_simulation);
 * record u8[G] (NULL = every game records): with record[g] == 0 the ply the next tg_sp_play plays is kept out of the training
 * positions -- the game's record still holds it, marked, and tg_sp_finished / tg_sp_harvest skip it.  The switch lives until
 * that tg_sp_play; tg_sp_reset, tg_sp_reset_from and tg_sp_restore put it back to "record".  tg_sp_begin_move(ctx, selfplay, n)
 * is this call with noise = selfplay for every game, the same n and record = NULL. */
int tg_sp_begin_move_games(tg_ctx* ctx, const uint8_t* noise, const int32_t* num_simulation, const uint8_t* record);

/* Front half of WP_MCTS.run (self_play.py:616-646) for every active game.  n_active = games still below their
 * target before this wave; n_rows = leaves awaiting evaluation. */
int tg_sp_collect(tg_ctx* ctx, int32_t* n_active, int32_t* n_rows);
/* Back half (self_play.py:651-654, :727-774). */
int tg_sp_absorb(tg_ctx* ctx);
/* while root.N < N0 + sims: run()  (self_play.py:662-664) with the network as evaluator. */
int tg_sp_search(tg_ctx* ctx, int32_t* n_waves);

/* visit counts per action (self_play.py:666-667), root visit total, side to move, ply counter, env.encode(root)
 * (self_play.py:685).  Any pointer may be NULL. */
int tg_sp_root_info(tg_ctx* ctx, int32_t* visits /*[G][A]*/, int32_t* root_n, int32_t* player, int32_t* step,
                    float* obs /*[G][C][S][S]*/);
/* ---- search tree read-out (analysis, play against a person, debugging a weight set) ------------------------------------------
 * Both calls only READ the trees: they are legal at any point between engine calls, also between tg_sp_collect and
 * tg_sp_absorb (pending counters are then reported as they stand), and leave the search, the RNG streams and a pending batch
 * untouched.  Every tree reference they follow is range-checked first, so a damaged tree yields a status, never a bad address. */

/* bits of tg_sp_root_children's flags[g][a] */
#define TG_CHILD_PRESENT 0x01u  /* the root has a child for action a, i.e. a is legal at the root (self_play.py:603) */
#define TG_CHILD_OPEN    0x02u  /* real_expanded (self_play.py:62): the child was evaluated and has children of its own */
#define TG_CHILD_PRIOR32 0x04u  /* prior[g][a] is a float32 value widened (a network prior); clear: float64 (after root noise) */
#define TG_CHILD_WIN     0x08u  /* the move ends the game and the cached result (self_play.py:638-642) is +1 for the side to move there */
#define TG_CHILD_LOSS    0x10u  /* ... or -1 */
/* tg_sp_root_children's status[g] */
enum {
    TG_ROOT_OK = 0,
    TG_ROOT_PARKED = 1,         /* slot left out by tg_sp_reset_from's mask: rows and root values are all zero */
    TG_ROOT_UNEVALUATED = 2,    /* the root awaits evaluation (tg_sp_expand_roots not called yet): no children yet */
    TG_ROOT_TERMINAL = 3,       /* the root position is the end of the game: no children */
    TG_ROOT_ERROR = 4           /* the game is parked in error (tg_sp_game_errors), or its tree failed a range check: all zero */
};
/* The root's children as dense per-action tables -- the fields of Node_V (self_play.py:51-63) of every entry of
 * root.children (self_play.py:70-77): n = total_visit_count (:55), pending = ons (:56, the WU-UCT counter of :767-774),
 * w = value_sum (:57) and var = value_var (:59) as stored in float32, prior (:54; after root noise, :90-95, a float64),
 * flags = the TG_CHILD_* bits.  The value of move a from the mover's side is -(w / (n + 1)) in float32, the value_score term of
 * ucb_score (:67-68, :716-725).  Per game: the root record's own n / pending / w / var (w / (n + 1) = the root's value from the
 * side to move) and status = TG_ROOT_*.  Every one of the A entries of a game is written: absent actions, and all
 * rows of a game whose status is not TG_ROOT_OK, are 0.  Any pointer may be NULL: it is then neither computed nor copied. */
int tg_sp_root_children(tg_ctx* ctx, int32_t* n /*[G][A]*/, int32_t* pending /*[G][A]*/, float* w /*[G][A]*/,
                        float* var /*[G][A]*/, double* prior /*[G][A]*/, uint8_t* flags /*[G][A]*/, int32_t* root_n /*[G]*/,
                        int32_t* root_pending /*[G]*/, float* root_w /*[G]*/, float* root_var /*[G]*/, uint8_t* status /*[G]*/);
/* Principal variation: from the root, the child with the most visits (ties: the lowest action, i.e. the first in the order of
 * the `children` dict, self_play.py:603 -- ascending action, pass last), down to `depth` levels (1 .. the path capacity,
 * max_step + 2 rounded up to 64; anything else is TG_ERR_ARG).  The walk ends early at a node that has no children, that is only
 * pseudo-expanded (self_play.py:634-636: evaluation pending) or whose best child was never visited.  action i32[G][depth]
 * (padding -1), n i32[G][depth] and w f32[G][depth] (the chosen child's total_visit_count / value_sum; padding 0), len i32[G] =
 * levels found; 0 for a parked, finished or errored slot, -1 when the walk met a reference that failed its range check (the row
 * is then all padding).  Any output pointer may be NULL. */
int tg_sp_pv(tg_ctx* ctx, int depth, int32_t* action /*[G][depth]*/, int32_t* n /*[G][depth]*/, float* w /*[G][depth]*/,
             int32_t* len /*[G]*/);

/* ---- forced playouts and policy target pruning (KataGo section 3.2; DESIGN.md 12, transgo_amd/forced_playouts.py) ------------
 * k >= 0 (0 = off, the default; KataGo uses 2): while k > 0, a move that begins with root noise (tg_sp_begin_move with
 * selfplay != 0, tg_sp_begin_move_games for the games with noise[g] != 0) is a *forced* move until its tg_sp_play: at the root a
 * child with n >= 1 and n + pending < sqrt(k * prior * (root.n + root.pending)) is selected before any other, and the counts
 * tg_sp_play records for the game are pruned -- every child but the most visited gives back up to floor(sqrt(k * prior * root.n))
 * visits while its score, recomputed with the reduced count, stays below the most visited child's.  The tree keeps its statistics
 * as searched.  Moves without noise, and everything with k = 0, are untouched.  k is context state: it is not part of a snapshot
 * (set it again after tg_sp_restore); TG_ERR_ARG for k < 0 or not finite, TG_ERR_STATE while a leaf batch is pending.  The flag of
 * a forced move ends with the game's tg_sp_play, however that call leaves the game; tg_sp_reset ends it for the slots it restarts
 * (the other slots keep theirs), tg_sp_reset_from and tg_sp_restore for every slot. */
int tg_sp_forced_playouts(tg_ctx* ctx, double k);
int tg_sp_forced_playouts_get(tg_ctx* ctx, double* k);
/* The root visit counts per action with the pruning applied for the games whose move in progress is a forced one (pruned_game[g]
 * = 1), raw for every other game; all 0 for a game whose tg_sp_root_children status is not TG_ROOT_OK.  Meant for a search that
 * is over (pending counters count as 0).  counts == 1 -> 0 (self_play.py:669) is the caller's step, as for tg_sp_root_info.
 * A read-out like tg_sp_root_children: nothing changes.  Either pointer may be NULL: it is then neither computed nor copied. */
int tg_sp_root_visits_pruned(tg_ctx* ctx, int32_t* visits /*[G][A] or NULL*/, uint8_t* pruned_game /*[G] or NULL*/);
/* Cumulative since tg_create: root selections made in forced moves, and how many of them met at least one forced child. */
int tg_sp_forced_playouts_stats(tg_ctx* ctx, uint64_t* root_selections, uint64_t* forced_selections);

/* ---- Gumbel root search (Danihelka et al., ICLR 2022; DESIGN.md 13, transgo_amd/gumbel.py) -------------------------------------
 * m >= 0 considered actions (0 = off, the default), c_visit, c_scale (the paper: 50, 1).  While m > 0, a move that would begin
 * with root noise (tg_sp_begin_move with selfplay != 0, tg_sp_begin_move_games for the games with noise[g] != 0) is a *Gumbel
 * move* until its tg_sp_play, and gets NO Dirichlet noise.  At its start the host takes one random_sample() u per root child
 * (ascending action, pass last) from the game's stream: g = -log(-log(u)), gl = g + log((double)prior); the m_eff = min(m, nchild)
 * children with the largest gl (ties: the lower action) are considered, every other child's gl is -inf.  The device stores
 * n0[c] = c.n and N0 = root.n.  With wu the WU-UCT loss, e(c) = (c.n - n0[c]) + c.pending / wu and
 * t = (root.n - N0) + root.pending / wu.  Root selection (depth 0 only): the considered children with e(c) == v(t), v the
 * sequential-halving schedule for (m_eff, budget = n_target - N0) at step min(t, budget - 1) (gumbel.considered_visit); if none,
 * the considered children with the smallest e(c) (counted as a fallback).  score(c) = gl[c] + (c_visit + maxN) * c_scale * qhat(c)
 * in float64, maxN = the largest c.n over all root children, qhat(c) = (double)(-(c.w / (c.n + 1))) in float32; the maximum, the
 * tie list in ascending action order and the one choice over it are the plain search's.  Moves without noise, and everything with
 * m = 0, are untouched.  The parameters are context state: not part of a snapshot (set them again after tg_sp_restore).
 * TG_ERR_ARG for m < 0, constants that are not finite, or m > 0 while forced playouts are on (tg_sp_forced_playouts refuses
 * k > 0 while m > 0 in turn); TG_ERR_STATE while a leaf batch is pending.  The flag of a Gumbel move ends like a forced move's. */
int tg_sp_gumbel(tg_ctx* ctx, int m, double c_visit, double c_scale);
int tg_sp_gumbel_get(tg_ctx* ctx, int* m, double* c_visit, double* c_scale);
/* The move of every game inside a Gumbel move whose search is over: argmax score(c) over the considered children with the largest
 * e(c) (pending counts as 0), ties to the lower action; no draw.  action[g] = -1 and gumbel_game[g] = 0 for every other game (and
 * for a game whose tg_sp_root_children status is not TG_ROOT_OK).  A read-out: nothing changes.  Either pointer may be NULL. */
int tg_sp_gumbel_move(tg_ctx* ctx, int32_t* action /*[G] or NULL*/, uint8_t* gumbel_game /*[G] or NULL*/);
/* The gl table of the moves in progress as uploaded, row g indexed by CHILD (ascending action order, nchild entries); rows of games
 * that are not in a Gumbel move are unspecified.  TG_ERR_STATE while m = 0. */
int tg_sp_gumbel_table(tg_ctx* ctx, double* gl /*[G][A]*/);
/* Stages the counts tg_sp_play records for the games in a Gumbel move with mask[g] != 0 (NULL: all of them) in place of the visit
 * counts: the improved policy as round_half_up(pi' * 2^24) (gumbel.improved_policy / fixed_point).  Every call replaces the
 * staging of every game; a Gumbel game without staged counts records its raw visits.  TG_ERR_STATE while m = 0. */
int tg_sp_gumbel_target(tg_ctx* ctx, const int32_t* counts /*[G][A]*/, const uint8_t* mask /*[G] or NULL*/);
/* Cumulative since tg_create: root selections made in Gumbel moves, and how many of them found no child at v(t). */
int tg_sp_gumbel_stats(tg_ctx* ctx, uint64_t* root_selections, uint64_t* fallback_selections);

/* ---- search ownership (KataGo's ownership map) -------------------------------------------------------------------
 * on != 0 (off is the default): every simulation tg_sp_absorb backs up also adds the ownership head's row of its leaf, turned to
 * Black's point of view, to a per-game accumulator: own_sum[g][p] = f32(own_sum[g][p] + s * own[row][p]), s = +1 when Black is to
 * move at the leaf (the root's side to move flipped by the parity of the path's moves), else -1; paths in the order tg_sp_absorb
 * handles them, wave after wave.  own_n[g] counts them.  What contributes is exactly what tg_sp_absorb backs up: not the duplicate
 * leaf of a wave (dropped, self_play.py:732-734), not a simulation that ends the game (backed up in tg_sp_collect without a
 * network row), not the root's own evaluation (tg_sp_expand_roots), not evaluations inherited with a reused sub-tree.  Both are
 * cleared by tg_sp_begin_move / tg_sp_begin_move_games (the mean is over ONE move's search), by tg_sp_reset (the slots it restarts),
 * tg_sp_reset_from and tg_sp_restore; they are not part of a snapshot, and neither is the switch.  The mode does not steer the
 * search: visits, moves and RNG streams are those of the same search with the mode off.  Turning it on allocates the accumulators
 * and [n_games * parallel_readouts][S*S] floats for the pending batch's ownership rows (once; they stay with the context when the
 * mode is turned off again); while it is on tg_sp_eval / tg_sp_search
 * make the forward write its ownership head (mapped back under the symmetry modes), and a host evaluator delivers through
 * tg_sp_set_eval_own -- plain tg_sp_set_eval is TG_ERR_STATE.  TG_ERR_STATE while an evaluation batch (leaves or roots) is pending, and while an evaluation
 * cache is attached: the cache stores policy and value only, so a hit has no ownership to give (tg_sp_eval_cache with entries > 0
 * is refused in turn while the mode is on). */
int tg_sp_search_ownership(tg_ctx* ctx, int on);
int tg_sp_search_ownership_get(tg_ctx* ctx, int* on);
/* tg_sp_set_eval with the ownership rows of the batch, each from the point of view of the side to move in that row's position
 * (what model.main_prediction returns).  TG_ERR_STATE while the mode is off. */
int tg_sp_set_eval_own(tg_ctx* ctx, const float* policy /*[n_rows][A]*/, const float* value /*[n_rows]*/,
                       const float* own /*[n_rows][S*S]*/, int32_t n_rows);
/* mean[g][p] = own_sum[g][p] / (float)own_n[g] (one float32 division; +1 Black ... -1 White; all 0 while own_n[g] == 0),
 * n[g] = own_n[g], score_lead[g] = (mean[g][0] + mean[g][1] + ..., sequential float32 in point order) - komi: Black's lead, the
 * sign of tg_sp_final's score.  A read-out like tg_sp_root_children: nothing changes, legal at any move boundary.  TG_ERR_STATE
 * before the first tg_sp_reset and while the mode is off.  Any pointer may be NULL. */
int tg_sp_root_ownership(tg_ctx* ctx, float* mean /*[G][S*S] or NULL*/, int32_t* n /*[G] or NULL*/, float* score_lead /*[G] or NULL*/);

/* Pass-alive end.  Context state, off by default.  While it is on:
 *   - after tg_sp_play has advanced the games, every game that is still running and whose new root is settled (tg_env_pass_alive)
 *     ends there: its root state is terminated, no evaluation of that root is requested, done[g] = 1 and the game is listed by
 *     tg_sp_finished with its recorded plies, exactly like a game that ended by double pass;
 *   - tg_sp_reset_from treats a settled state like a terminated one;
 *   - tg_sp_harvest (z, ownership target, winner, score, territory) and tg_sp_final score with the pass-alive-aware area, for every
 *     game, however it ended.
 * The search inside the tree is unchanged (leaves keep the plain rules), so visits and moves up to the ply of settlement are those
 * of the mode off.  While it is off nothing of this is launched.  Neither the switch nor the counters are part of a snapshot: set
 * the mode before tg_sp_restore.  TG_ERR_STATE while a leaf batch is pending. */
int tg_sp_pass_alive(tg_ctx* ctx, int on);
int tg_sp_pass_alive_get(tg_ctx* ctx, int* on);
/* Since the mode was first turned on: games ended by settlement, and the sum of the plies they had played. */
int tg_sp_pass_alive_stats(tg_ctx* ctx, uint64_t* games_settled, uint64_t* plies_at_settlement_sum);
/* tg_env_pass_alive's status and settled for the games' current roots.  A read-out like tg_sp_root_children: nothing changes, the
 * mode need not be on.  TG_ERR_STATE before the first tg_sp_reset.  Either pointer may be NULL.  A game parked in error without a root
 * block (tg_sp_game_errors) reads as an empty board: status 0 everywhere, not settled. */
int tg_sp_root_pass_alive(tg_ctx* ctx, int8_t* status /*[G][S*S] or NULL*/, uint8_t* settled /*[G] or NULL*/);

/* One random_sample() from each game's stream: the draw inside np.random.choice(A, p=) (self_play.py:683). */
int tg_sp_draw_uniform(tg_ctx* ctx, double* u /*[G]*/, const uint8_t* mask);
int tg_sp_rng_state(tg_ctx* ctx, int game, tg_mt19937* out);
/* All G streams at once, and the way back (mask NULL = all): lets a game's stream move between contexts -- in policy_evaluate
 * (self_play.py:986-1040) the two agents of a game draw from ONE global stream, so it follows the game from the engine holding
 * the train model to the one holding the evaluation model and back, ply by ply. */
int tg_sp_rng_get(tg_ctx* ctx, tg_mt19937* out /*[G]*/);
int tg_sp_rng_set(tg_ctx* ctx, const tg_mt19937* in /*[G]*/, const uint8_t* mask /*[G] or NULL*/);
/* update_with_action (self_play.py:857-872) for every unfinished game; done[g] = 1 game over, 2 the game is parked in
 * error (tree cap reached / pool empty; see tg_sp_game_errors), 0 otherwise.  With cfg.record_games the move's record entry is
 * written first (self_play.py:917-926).  Leaves a root batch pending for the games whose new root was not yet expanded. */
int tg_sp_play(tg_ctx* ctx, const int32_t* actions /*[G]*/, uint8_t* done /*[G]*/);
/* A game whose tree outgrows its cap (cfg.arena_slots), or that finds the shared pool (cfg.pool_slots) empty, is parked: it takes no
 * further part in searches (its chunks stay its own until its slot is reset), tg_sp_play reports
 * 2 for it, every other game is unaffected, and tg_sp_reset with its mask bit starts a new game in the slot.  n_errors = games
 * parked right now (as of the last collect/play; no device round trip when err is NULL); err[g] = 0 or a bit set (1 arena,
 * 2 path depth, 4 action not among the root's children). */
int tg_sp_game_errors(tg_ctx* ctx, int32_t* n_errors, int32_t* err /*[G] or NULL*/);
/* The reference keeps the searched tree in unbounded Python memory (tree reuse, self_play.py:860); here a re-rooted tree may
 * keep at most arena_slots minus the room of one full search.  When the kept sub-tree is larger (very peaked policies, many
 * moves in a row) its deepest blocks are dropped: those nodes keep their statistics and become unexpanded leaves again.
 * blocks = how many were dropped so far over all games (0 = every search so far equals the reference's). */
int tg_sp_tree_truncations(tg_ctx* ctx, uint64_t* blocks);

/* Tree memory.  The reference keeps every tree in unbounded Python memory (Node_V objects, self_play.py:51-95); here all games of
 * a context share ONE pool of cfg.pool_slots x n_games slots.  pool_slots = its size; high_water_slots = the most that was in use
 * at once since creation; in_use_slots = now; exhausted = how often a game found no chunk left (that game is then parked in error
 * 1, tg_sp_game_errors, or its kept sub-tree truncated, tg_sp_tree_truncations -- 0 = never).  Any pointer may be NULL. */
int tg_sp_pool_stats(tg_ctx* ctx, uint64_t* pool_slots, uint64_t* high_water_slots, uint64_t* in_use_slots, uint64_t* exhausted);

/* ---- finished games -> training positions, on the device (self_play.py:929-967) ------------------------------------------
 * Games the LAST tg_sp_play finished, in ascending slot order, and the number of recorded positions they hold (= their moves,
 * unless tg_sp_begin_move_games kept plies out of the record: those are not counted, not harvested, and a game may contribute
 * no position at all -- tg_sp_harvest then lists it with n_moves = 0). */
int tg_sp_finished(tg_ctx* ctx, int32_t* n_games, int32_t* n_positions);
/* Their positions as one position-major batch, game after game in that order, plies ascending -- the arrays
 * tg_replay_append(_dev) takes: obs_bits u32[n_positions][ceil(C*S*S/32)] (env.encode bit-packed, bit i = plane-major flat
 * index i), counts i32[n_positions][A] (raw visit counts; pi = counts with 1 -> 0, / sum, self_play.py:666-671), z
 * f32[n_positions] (+1 mover == winner else -1, :931-934), own i8[n_positions][S*S] (territory from the mover's side,
 * :938-940), player u8[n_positions] (may be NULL).  device_out != 0: those five are pointers into this GPU's memory (e.g. the
 * payload tensors of an RCCL gather) and nothing bulky crosses PCIe.  Per-game tables are host arrays and may be NULL:
 * slot / n_moves / winner (1 black, 2 white, environment.py:118-119) / score (getScore, go_env.cc:126-130) [n_games], terr
 * i8[n_games][S*S] (getTerritory, +1 black / 0 / -1 white).  Call before tg_sp_reset restarts the slots.  The 8-fold
 * augmentation (self_play.py:943-965) is applied by the consumer (tg_replay_sample; transgo_amd.self_play.game_targets). */
int tg_sp_harvest(tg_ctx* ctx, uint32_t* obs_bits, int32_t* counts, float* z, int8_t* own, uint8_t* player, int device_out,
                  int32_t* slot, int32_t* n_moves, int32_t* winner, float* score, int8_t* terr);
/* ---- policy surprise weighting (KataGo's policySurpriseDataWeight; DESIGN.md 15, transgo_amd/policy_surprise.py) -----------------
 * How often a position of a finished game is written to the training data.  weight = lambda in [0, 1] (0 = off, the default; KataGo
 * uses 0.5; anything else is TG_ERR_ARG), seed = the seed of the copy draws.  For a harvested position with recorded counts c and the
 * network's float32 policy row p for it (all in float64): c' = c with 1 -> 0, n = sum c', pi = c' / n,
 * s = max(0, sum over c'_a > 0 of pi_a * (log pi_a - log max(p_a, FLT_MIN))), s = 0 when n == 0; for a game with T harvested
 * positions t = 0..T-1 (plies kept out of the record do not count) and S = s_0 + s_1 + ... in that order:
 * w_t = (1 - lambda) + lambda * T * s_t / S (1 when S == 0), k_t = floor(w_t + tg_host_cap_draw(game seed, t, seed ^ 0x50535731)
 * / 2^24).  The resampled batch holds position t k_t times in a row (possibly 0 times); games and plies keep their order, the
 * per-game n_moves are the sums of the k_t, every other per-game table is tg_sp_harvest's.  No part of the search changes, no
 * game's MT19937 stream is touched, and while the weight is 0 nothing of this is launched or allocated.  The setting is context
 * state like tg_sp_forced_playouts': not part of a snapshot (set it again after tg_sp_restore; a plan holds no state beyond the
 * finished games, so games restored finished-but-unharvested resample identically). */
int tg_sp_policy_surprise(tg_ctx* ctx, double weight, uint32_t seed);
int tg_sp_policy_surprise_get(tg_ctx* ctx, double* weight, uint32_t* seed);
/* The two-call pattern of tg_sp_finished / tg_sp_harvest.  The PLAN call works on the games the last tg_sp_play finished (it runs
 * their plain harvest into HBM of its own) and returns n_out, the positions of the resampled batch.  prior = host rows
 * f32[n_positions][A] in tg_sp_harvest's order, or NULL: the loaded network then runs over the harvested positions, straight from
 * their bit-packed observations, in chunks of at most the engine's row capacity (n_games * parallel_readouts), in identity
 * orientation whatever tg_net_set_symmetry says, past the evaluation cache (no lookup, no insert, no counter moves), into rows of
 * its own -- a root batch tg_sp_play left pending is not disturbed, and tg_sp_stats' evals does not count these rows
 * (tg_sp_policy_surprise_stats does).  game_seed u32[cfg.n_games]: the seed of the game in every SLOT (the finished games pick
 * theirs).  Optional read-outs for tests and analysis, each may be NULL: surprise f64[n_positions], weight f64[n_positions], copies
 * i32[n_positions], prior_out f32[n_positions][A] = the prior rows used.  TG_ERR_STATE while the weight is 0, and with prior ==
 * NULL while no network is loaded; the message says which. */
int tg_sp_policy_surprise_plan(tg_ctx* ctx, const float* prior, const uint32_t* game_seed, int32_t* n_out, double* surprise,
                               double* weight, int32_t* copies, float* prior_out);
/* tg_sp_harvest's argument list with the position arrays sized for n_out: the resampled batch, to host arrays or (device_out != 0)
 * into this GPU's memory.  TG_ERR_STATE when no plan is current for the games the last tg_sp_play finished (tg_sp_play, tg_sp_reset,
 * tg_sp_reset_from, tg_sp_restore and tg_sp_policy_surprise each end a plan). */
int tg_sp_policy_surprise_harvest(tg_ctx* ctx, uint32_t* obs_bits, int32_t* counts, float* z, int8_t* own, uint8_t* player,
                                  int device_out, int32_t* slot, int32_t* n_moves, int32_t* winner, float* score, int8_t* terr);
/* Cumulative since tg_create: positions that went into plans, positions the plans put out, games planned, rows the prior forward
 * ran (0 while every plan was given host priors).  Any pointer may be NULL. */
int tg_sp_policy_surprise_stats(tg_ctx* ctx, uint64_t* positions_in, uint64_t* positions_out, uint64_t* games, uint64_t* rows_forwarded);
/* HIP-event times on the context's stream, cumulative: the prior (forward, or the upload of host rows), k_psw_surprise + k_psw_plan,
 * k_psw_gather; and the number of plans. */
int tg_prof_read_policy_surprise(tg_ctx* ctx, double* prior_ms, double* plan_ms, double* gather_ms, int64_t* plans);
/* k_psw_surprise and k_psw_plan on caller arrays, for any context (kernel tests, analysis of stored games): n_games games of
 * n_moves[g] positions each, game after game; counts i32[n][A], prior f32[n][A], game_seed u32[n_games] (by game).  Outputs, each may
 * be NULL: n_out, n_moves_out i32[n_games], surprise / weight_out f64[n], copies i32[n], src i32[min(n_out, src_cap)] = the source
 * row of every output row. */
int tg_policy_surprise_plan_arrays(tg_ctx* ctx, int n_games, const int32_t* n_moves, const uint32_t* game_seed, const int32_t* counts,
                                   const float* prior, double weight, uint32_t seed, int32_t* n_out, int32_t* n_moves_out,
                                   double* surprise, double* weight_out, int32_t* copies, int32_t* src, int src_cap);

/* getScoreAndTerritory / getWinner of the current root position (self_play.py:932-937). */
int tg_sp_final(tg_ctx* ctx, float* score /*[G]*/, float* terr /*[G][S*S]*/, int32_t* winner /*[G]*/);
/* Aggregate counters: completed simulations, evaluated leaves, summed selection depth, RNG words drawn by tie
 * breaks, games in error, and max_slots = the most slots any single game's tree has held (whole chunks; the pool's own fill is
 * tg_sp_pool_stats). */
int tg_sp_stats(tg_ctx* ctx, uint64_t* sims, uint64_t* evals, uint64_t* depth_sum, uint64_t* tie_draws, int32_t* errors,
                int32_t* max_slots);

/* ---- evaluation cache: positions already evaluated skip the network ---------------------------------------------------------------
 * Opt-in, per context, exact.  The network's output for a row of the evaluation batch is a pure function of the row's bit-packed
 * planes, the live weight set and the symmetry mode, and the forward computes identical bits for identical rows wherever they stand
 * in a batch; so a table keyed by the full bits (a hash only picks the bucket, every word is compared before a hit) changes no
 * visit count, move or float in the tree -- it only takes rows out of the forward.  With a cache configured tg_sp_eval and
 * tg_sp_search probe the table, fold the rows of one batch that hold the same position into one, run the forward on the rest (one
 * 4-byte read-back per batch gives the host their number), and insert what was evaluated.  tg_sp_set_eval (a host evaluator is not
 * known to be pure) and tg_net_predict never touch it.
 *
 * tg_sp_eval_cache: entries == 0 frees the cache (the context is the uncached engine again: nothing else is launched or
 * allocated); otherwise a 4-way set-associative table of `entries` rounded up to whole buckets plus staging for one batch,
 * 16 + 4 * obs_words + 4 * (A + 1) bytes per entry (452 B at 9x9, 1920 B at 19x19 with 10 planes).  An existing cache is replaced
 * (contents and counters start again).  TG_ERR_STATE while an evaluation batch is pending, TG_ERR_HIP (the message names the
 * bytes asked for) when the allocation fails, TG_ERR_ARG for a context without games or more than 2^31 entries.
 * Invalidation is a generation number, nothing is swept: every change of the evaluator -- tg_net_load / tg_net_load_arch, an
 * asynchronous refresh at the moment it is adopted, tg_net_set_symmetry with another mode or argument -- and
 * tg_sp_eval_cache_clear make every entry written so far a miss.  Snapshots do not hold the cache and tg_sp_restore leaves it
 * alone (entries are keyed by position and generation, not by game).
 * tg_sp_eval_cache_stats: cumulative since the cache was created; lookups = hits + batch_duplicates + evaluated, rows requested /
 * served from the table / served by another row of the same batch / sent through the network; inserts, and dropped_inserts = an
 * evaluated row that lost the claim on its way of the table to another row of the same batch (harmless: it is evaluated again next
 * time).  Which of two keys wins a contested way may differ from run to run, so may the counters; results never do.  Any pointer
 * may be NULL; without a cache everything is 0.  tg_sp_stats keeps counting the rows requested as evals. */
int tg_sp_eval_cache(tg_ctx* ctx, uint64_t entries);
int tg_sp_eval_cache_clear(tg_ctx* ctx);
int tg_sp_eval_cache_stats(tg_ctx* ctx, uint64_t* lookups, uint64_t* hits, uint64_t* batch_duplicates, uint64_t* evaluated,
                           uint64_t* inserts, uint64_t* dropped_inserts, uint64_t* entries, uint64_t* bytes);

/* ---- checkpoint and resume: the whole engine as one flat byte buffer ------------------------------------------------------------
 * The reference checkpoints its replay buffer (replay_buffer.py:49-87, transgo.py:225-250); its games in flight are lost with the
 * process.  Here the population itself can be put down and picked up again, or forked (one snapshot restored into two contexts).
 * A snapshot is legal at a MOVE BOUNDARY only: no evaluation batch pending and no game inside a search -- between tg_sp_play +
 * tg_sp_expand_roots (or tg_sp_reset + tg_sp_expand_roots) and the next tg_sp_begin_move; anywhere else TG_ERR_STATE.  It holds
 * every game's control record, tree, RNG stream, move record and counters, the tree pool's ring and statistics, and the
 * finished games tg_sp_harvest has not taken yet; the tree pool is PACKED (the chunks trees own, not the provisioned pool), so a
 * snapshot costs what is in use.  Network weights are not part of it (load them as before; a restore into a context without
 * weights succeeds and the next search reports "no network weights loaded"), nor is a pending background refresh.
 * device_mem != 0: the buffer is in this GPU's memory (16-byte aligned; fork / migrate without a host bounce).  With a HOST buffer
 * the snapshot is packed in (or scattered from) a staging buffer of its size in HBM, which the context then keeps for the next
 * checkpoint until tg_destroy (371 MiB at 4096 boards / 400 simulations); the device path allocates nothing of that size.
 * tg_sp_snapshot_size: the bytes tg_sp_snapshot would write now.  tg_sp_snapshot: cap = room in `out`, written = bytes used.
 * tg_sp_restore takes a snapshot into a context created with the same board_size, encode_dim, n_games, parallel_readouts,
 * max_step, komi, wu_loss, c_puct1/2, record_games, arena_slots and pool_slots (num_simulation, device and the network may
 * differ); a mismatch is refused with a message that names the field and both values.  A truncated buffer, a wrong magic or
 * version, a section past the end, a chunk id outside the pool or listed twice are refused too -- all BEFORE anything in the
 * context is overwritten: a refused restore leaves the context as it was. */
int tg_sp_snapshot_size(tg_ctx* ctx, uint64_t* bytes);
int tg_sp_snapshot(tg_ctx* ctx, void* out, uint64_t cap, int device_mem, uint64_t* written);
int tg_sp_restore(tg_ctx* ctx, const void* in, uint64_t bytes, int device_mem);

/* ---- network -------------------------------------------------------------------------------------------------------------
 * Replaces TransGoNetwork.set_weights / main_prediction (model.py:17-27).  The blob is the BatchNorm-folded, kernel-layout
 * packing of the model's state_dict produced by transgo_amd/model.py:pack_weights (layout documented there and in
 * DESIGN.md); tg_net_blob_floats gives its exact length.  Loading again later is the weight refresh of
 * self_play.py:913.  rows_cap: largest batch tg_net_predict will be asked for (engine contexts size it themselves). */
size_t tg_net_blob_floats(int board_size, int encode_dim, int filters, int blocks);
int tg_net_load(tg_ctx* ctx, const float* blob, size_t n_floats, int rows_cap);
/* Same with an explicit layer program: one letter per trunk layer, 'R' = pre-activation ResidualBlock (model.py:238-248),
 * 'A' = Self_Attention (model.py:288-315), optional "+P" = attention in the policy head (model.py:72,106).  The shipped
 * MainNetwork (model.py:49-76) is "RARRRARRRRAR+P"; tg_net_load uses cfg.net_blocks x 'R'.  Attention is built at 9x9, and in f32 (net_precision 0) at 19x19 with 128 or 256
 * filters; the fp16 and split-precision modes with attention at 19x19 are refused at the load. */
size_t tg_net_blob_floats_arch(int board_size, int encode_dim, int filters, const char* arch);
int tg_net_load_arch(tg_ctx* ctx, const char* arch, const float* blob, size_t n_floats, int rows_cap);
/* Weight refresh that never stalls a search (the hand-off of trainer.py:76-79 -> self_play.py:913): there are two complete
 * weight sets; this call copies the blob to pinned memory and uploads + re-stages it into the idle set on a side stream, then
 * returns.  Searches keep running on the live set; the switch happens at a boundary only: the next tg_sp_begin_move (so one
 * move's search, and its recorded pi, never mixes two weight sets) or the next tg_net_predict that finds the upload complete.
 * tg_sp_eval / tg_sp_collect / tg_sp_absorb never switch: a host that drives those itself and never calls tg_sp_begin_move must
 * call tg_net_load_poll(ctx, 0, &pending) where it wants a finished refresh to take over.
 * Falls back to the synchronous load when no network of this architecture is loaded yet.  One refresh in flight at a time (a
 * second call first waits for the previous one).  tg_net_load_poll: pending = 1 while a refresh is not adopted yet; wait != 0
 * blocks until it is. */
int tg_net_load_async(tg_ctx* ctx, const char* arch, const float* blob, size_t n_floats);
/* The same with the blob in THIS GPU's memory (e.g. the buffer an RCCL broadcast filled): copied device -> device, no host
 * bounce.  Its contents must be complete when the call is made; the buffer is free again when the call returns.  Without a
 * network of this architecture loaded yet it falls back to the synchronous load (one copy through the host). */
int tg_net_load_async_dev(tg_ctx* ctx, const char* arch, const float* d_blob /*device*/, size_t n_floats);
int tg_net_load_poll(tg_ctx* ctx, int wait, int* pending);
/* main_prediction (model.py:17-20) on host buffers: obs f32[n][C][S][S] -> policy f32[n][A] (softmax), value f32[n]
 * (tanh), own f32[n][S*S] (tanh; may be NULL). */
int tg_net_predict(tg_ctx* ctx, const float* obs, int n_rows, float* policy, float* value, float* own);
/* Symmetry-aware evaluation.  The network is trained on all eight dihedral images of every position (self_play.py:943-965), so it
 * may be asked about a position in any of them.  Symmetry s = 0..7 is the augmentation index of that loop, s = 2*(i-1) + f:
 * T_s(m) = np.rot90(m, i) for i = 1..4, then np.fliplr if f == 1; s = 6 is the identity.  Evaluating a row under s: T_s on each of
 * its planes, the unchanged forward, and the outputs mapped back to the original orientation (board part of the policy and the
 * ownership through the inverse permutation, pass entry and value as they are).  Every evaluation of the context -- tg_sp_eval,
 * tg_sp_search, tg_net_predict -- goes through the mode, in every net_precision:
 *   TG_SYM_NONE      the plain forward: nothing more is launched or allocated, results are bit-identical to a context that never
 *                    made this call
 *   TG_SYM_FIXED     every row under s = arg (tests, diagnostics)
 *   TG_SYM_POSITION  row r under s = sym_of(arg = seed, the row's bit-packed planes), a pure function of seed and position -- the
 *                    same position gets the same orientation in whatever batch it appears, so duplicate leaves, a snapshot +
 *                    restore and a host restatement all agree.  sym_of in uint32 arithmetic over the row's ceil(C*S*S/32) words
 *                    (bit i = plane-major flat index i, unused high bits of the last word zero): h = seed ^ 0x9E3779B9; per word
 *                    h = (h ^ w) * 0x01000193; then h ^= h>>16, h *= 0x85EBCA6B, h ^= h>>13, h *= 0xC2B2AE35, h ^= h>>16;
 *                    s = h >> 29.  No game's MT19937 stream is touched.
 *   TG_SYM_MEAN8     eight forwards, s = 0..7 in that order; the mapped-back policy, value and ownership accumulate in float32
 *                    as ((((o0 + o1) + o2) + ...) + o7) * 0.125f.  A background weight refresh is never adopted between the
 *                    eight passes.
 * The reference's self-play evaluates in one orientation only (self_play.py:777-786): TG_SYM_NONE alone keeps bit parity with it.
 * TG_ERR_ARG for an unknown mode or s > 7; TG_ERR_STATE while an evaluation batch is pending (the evaluator changes at a move
 * boundary only); a refused call leaves the setting as it was.  Legal before or after weights are loaded; the setting is context
 * state like the weights -- no part of a snapshot or of tg_config.  The staging buffers (the transformed rows and the forward's
 * outputs, sized by the network's rows_cap) are allocated by the first evaluation under a mode other than TG_SYM_NONE;
 * tg_net_symmetry_staging reports their bytes (0 until then). */
#define TG_SYM_NONE 0
#define TG_SYM_FIXED 1
#define TG_SYM_POSITION 2
#define TG_SYM_MEAN8 3
int tg_net_set_symmetry(tg_ctx* ctx, int mode, uint32_t arg);   /* mode 0..3; arg = s for mode 1, seed for mode 2, else 0 */
int tg_net_get_symmetry(tg_ctx* ctx, int* mode, uint32_t* arg);
int tg_net_symmetry_staging(tg_ctx* ctx, uint64_t* bytes);
/* HIP-event timing of the two symmetry kernels (bit-plane transform, output back-map) on the context's stream: enable, run, read
 * the totals since the enable; launches that found the event pool full are left out. */
int tg_prof_enable_symmetry(tg_ctx* ctx, int on, int max_launches);
int tg_prof_read_symmetry(tg_ctx* ctx, double* transform_ms, double* backmap_ms, int64_t* launches);
/* How the loaded network carries its f32 residual stream: one_stream = 1 for the DMA-fed f32 chain, which keeps ONE slice-major
 * stream between conv layers and activates it on load, 0 for every other chain; act_copy = 1 while the buffer of the pre-activated
 * copy is allocated (the DMA-fed chain with an attention layer in front of a residual block).  Either may be NULL. */
int tg_net_stream_layout(tg_ctx* ctx, int* one_stream, int* act_copy);
/* Range report.  The reference network is f32 end to end (model.py:79-114) and accepts any trained checkpoint (model.py:23-27);
 * net_precision 1 / 2 / 3 carry activations as fp16 (3: as fp16 hi + lo) and lose f32's range: beyond +-65504 the fp16 copy is
 * inf and the layers behind it compute NaN.  Every kernel that rounds to fp16 checks what it rounds; fp16_overflows = sticky
 * count, since the network was created, of output tiles (convs) / boards (attention) that held such a value (0 = all forward
 * passes so far stayed in range; always 0 with net_precision 0); a non-zero count also leaves a message in tg_last_error.
 * weight_absmax = largest |w| of the live weight set's BatchNorm-folded blob (inf / NaN if it holds one).  Either may be NULL. */
int tg_net_range(tg_ctx* ctx, uint64_t* fp16_overflows, float* weight_absmax);
/* HIP-event timing of the dominant kernel (3x3 conv F->F) on the launch stream: enable, run, read totals. */
int tg_prof_enable(tg_ctx* ctx, int on, int max_launches);
int tg_prof_read(tg_ctx* ctx, double* conv_ms, int64_t* conv_launches, double* conv_flops);
/* tg_prof_read drains the event pool into running totals (call it between steps); launches that found the pool full are not in
 * the totals and are counted here (0 = the totals cover every launch since tg_prof_enable). */
int tg_prof_skipped(tg_ctx* ctx, int64_t* launches);
/* The same for the tree stage (k_collect = selection + leaf step + pseudo-expansion + feature planes, self_play.py:607-650;
 * k_absorb = complete_update + backup, :651-654, :727-764): event time per kind, number of waves, and the number of children
 * scored by PUCT summed over all selection levels since the last reset (mean fan-out = children_scored / depth_sum). */
int tg_prof_enable_tree(tg_ctx* ctx, int on, int max_waves);
int tg_prof_read_tree(tg_ctx* ctx, double* collect_ms, double* absorb_ms, int64_t* waves, uint64_t* children_scored);
/* The same for a context with an evaluation cache (TG_ERR_STATE without one), per cached batch: probe_ms = probe, in-batch
 * duplicates and the dense list; readback_ms = the stream's idle gap while the host reads the number of rows left; net_ms = the
 * forward on those rows; insert_ms = scatter and insert.  Batches that found the event pool full are not in the totals. */
int tg_prof_enable_eval_cache(tg_ctx* ctx, int on, int max_batches);
int tg_prof_read_eval_cache(tg_ctx* ctx, double* probe_ms, double* readback_ms, double* net_ms, double* insert_ms, int64_t* batches);

/* ---- device-resident replay store + batch sampler (replaces replay_buffer.py:30-47 + the stacking of trainer.py:46-54) ----
 * Positions are stored once, un-augmented and compact; entry e of the reference's ring of augmented tuples is
 * (position e/8, symmetry e%8) in the reference's append order (self_play.py:943-965: for i in 1..4: rot90(i), fliplr of
 * that).  tg_replay_sample materialises entries as the four float32 arrays the trainer feeds the network. */
typedef struct tg_replay tg_replay;
int tg_replay_create(tg_ctx* ctx, int capacity_positions, tg_replay** out);
void tg_replay_destroy(tg_replay* rp);
int tg_replay_append(tg_replay* rp, const uint32_t* obs_bits /*[n][ceil(C*S*S/32)]*/, const int32_t* counts /*[n][A]*/,
                     const float* z /*[n]*/, const int8_t* own /*[n][S*S]*/, int n);
/* The same with the four arrays in this GPU's memory (tg_sp_harvest with device_out, or what an RCCL gather delivered). */
int tg_replay_append_dev(tg_replay* rp, const uint32_t* obs_bits, const int32_t* counts, const float* z, const int8_t* own, int n);
int tg_replay_info(const tg_replay* rp, long long* entries, long long* index, int* full);
int tg_replay_sample(tg_replay* rp, const long long* entry /*[B]*/, int B, float* state /*[B][C][S][S]*/, float* pi /*[B][A]*/,
                     float* z /*[B]*/, float* own /*[B][S*S]*/, int device_out);
/* Checkpoint of the store (save / load of replay_buffer.py:49-87).  tg_replay_export copies the slots first_position ..
 * first_position + n - 1 out in STORAGE order (slot p holds the position appended p-th modulo the capacity), to host arrays of
 * tg_replay_append's layouts; first_position + n may not exceed the positions held (entries / 8).  tg_replay_import writes slots
 * 0 .. n_held - 1 verbatim and sets the append counter, so the ring position and the mapping from entry e to (position,
 * symmetry) are those of the exported store.  Only appended mod capacity and whether appended >= capacity are observable
 * (tg_replay_info), so a saver may pass the counter normalised to capacity + ring position for a full store; refused (TG_ERR_ARG) when n_held exceeds the capacity or differs from
 * min(appended, capacity). */
int tg_replay_export(tg_replay* rp, long long first_position, int n, uint32_t* obs_bits, int32_t* counts, float* z, int8_t* own);
int tg_replay_import(tg_replay* rp, const uint32_t* obs_bits, const int32_t* counts, const float* z, const int8_t* own, int n_held,
                     long long appended);

/* ---- 3. host-only NumPy-legacy MT19937 helpers ------------------------------------------------------------------------
 * Same stream as np.random.RandomState: key/pos are get_state()[1] / get_state()[2].  No GPU needed. */

void tg_host_mt_seed(tg_mt19937* s, uint32_t seed);                 /* np.random.seed(seed) */
uint32_t tg_host_mt_next32(tg_mt19937* s);
double tg_host_mt_random_sample(tg_mt19937* s);                     /* random_sample(): the draw inside choice(A, p=) (self_play.py:683) */
int32_t tg_host_mt_choice_index(tg_mt19937* s, int32_t k);          /* index drawn by choice(list of k) (self_play.py:709) */
int tg_host_mt_dirichlet(tg_mt19937* s, double alpha, int32_t n, double* out);   /* dirichlet([alpha]*n) (self_play.py:93) */
void tg_host_mt_gumbel(tg_mt19937* s, int32_t n, double* out);   /* n draws of -log(-log(random_sample())), libm's log */
/* Playout cap randomization: the 24-bit draw that decides whether ply `ply` of the game seeded `seed` is searched in full --
 * mix(mix(cap_seed << 32 | seed) ^ ply) >> 40 with mix = the splitmix64 finaliser; full when draw < floor(p_full * 2^24).  A
 * pure function of its arguments: no game's MT19937 stream is touched (transgo_amd/playout_cap.py is the same in NumPy). */
uint32_t tg_host_cap_draw(uint32_t seed, int32_t ply, uint32_t cap_seed);
/* getSubEncode (go_env.h:70, board.cc:1166-1271) with the board size as an argument: crops channels x S x S 32-bit planes into
 * cut_num (<= 5) channels x s x s windows -- the four corners, then the centre.  Host arrays; no GPU needed. */
void tg_host_sub_encode(int board_size, const void* encode, void* sub_encode, int sub_board_size, int channels, int cut_num);


/* ---- 4. the reference engine's own 15 entry points (GoEnv/cpp_src/go_env.h:24-70), same names and signatures -------------
 * One process-wide context (the reference keeps its configuration in file-static variables, go_env.cc:9-12); every call is
 * the batched GPU entry point with n = 1.  `State` is any caller buffer of at least tg_state_size() bytes -- the
 * reference's 1188-byte GoState / Python's 1196-byte c_GoState (environment.py:17-29) qualify, so GoEnv/environment.py binds
 * this library unchanged.  Board size: 9, or 19 with TRANSGO_BOARD_SIZE=19 in the environment (go_comm.h:20 is compile-time
 * in the reference).  Coord = int16_t, Stone = uint8_t (go_comm.h:13-15). */
#ifndef TRANSGO_NO_GOENV_NAMES
bool Init(int history_dim, int encode_dim, int max_step, float komi);        /* go_env.h:30 */
bool Reset(void* state);                                                      /* go_env.h:33 */
bool Step(const void* state, void* next_state, int16_t action);              /* go_env.h:37 */
bool Step_(void* state, int16_t action);                                      /* go_env.h:38 */
bool checkAction(const void* state, int16_t action);                          /* go_env.h:42 */
bool isTerminated(const void* state);                                         /* go_env.h:45 */
bool Encode(const void* state, float* encode_state);                          /* go_env.h:48 */
float getScore(const void* state);                                            /* go_env.h:51 */
float getTerritory(const void* state, float* territory);                      /* go_env.h:54 */
int getLegalAction(const void* state, int* actions);                          /* go_env.h:57 */
int getLegalNoEye(const void* state, int* actions);                           /* go_env.h:60 */
void Show(const void* state);                                                 /* go_env.h:63 */
uint8_t getPlayer(const void* state);                                         /* go_env.h:66 */
int getStep(const void* state);                                               /* go_env.h:69 */
void getSubEncode(int* encode_state, int* sub_encode_state, int sub_board_size, int encode_state_channels, int cut_num);  /* go_env.h:70 */
#endif

#ifdef __cplusplus
}
#endif
#endif /* TRANSGO_HIP_H_ */
