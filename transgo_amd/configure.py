"""Config -- the hot-path parameters of the reference's configure.py:5-103 (same attribute names and defaults), plus the
tower size and the number of concurrent boards of the batched engine."""
import math


class Config:
    def __init__(self, **over):
        self.board_size = 9                      # configure.py:9
        self.encode_state_channels = 10          # configure.py:11
        self.komi = 7.5                          # configure.py:13
        self.black, self.white = 1, 2
        self.max_step = 120                      # configure.py:16
        self.buffer_size = 1500000               # configure.py:19
        self.game_total_num = 1e8                # configure.py:24
        self.c_puct1 = 3                         # configure.py:26
        self.c_puct2 = 0.05                      # configure.py:27
        self.num_simulation = 210                # configure.py:29
        self.wu_loss = 2                         # configure.py:32
        self.parallel_readouts = 4               # configure.py:33
        self.input_dim = self.encode_state_channels
        self.num_features = 128                  # configure.py:37
        self.num_blocks = 6                      # tower depth (BASELINE.json "N-block x F-filter")
        self.network = "tower"                   # "tower" | "transgo" (the shipped MainNetwork with attention, model.py:49-76; at
                                                 # board_size 19 in inference_dtype "f32" with 128 or 256 filters)
        self.concurrent_games = 4096             # boards resident on one GPU
        self.game_groups = 1                     # K > 1: the boards of a GPU as K independent groups on their own HIP streams (GroupedSelfPlay)
        self.stagger_games = 0                   # T > 1: slot g starts its first game at step g mod T (BatchedSelfPlay.start): games end
                                                 # spread over T steps instead of all on one; 0 = all slots start together
        self.inference_dtype = "f32"             # "f16": fp16 weights/activations, f32 accumulate (BASELINE config 5; towers of 128/256
                                                 # filters, and network = "transgo" at 9x9 with 128 filters, not at 19x19); "f16r" (attention-free
                                                 # towers only): the residual stream in fp16 as well (+4-6 %, error < 4e-4 over 40 blocks);
                                                 # "f32x3": split precision -- conv operands as fp16 hi + lo, f32 accumulate, ~1e-6 of f32
        self.eval_symmetry = "none"              # "position": every evaluation in one orientation chosen from (symmetry_seed, position);
                                                 # "mean8": the mean over all eight (match play, analysis); transgo_amd/symmetry.py.
        self.symmetry_seed = 0                   # Only "none" keeps bit parity with the reference's self-play
        self.eval_cache_entries = 0              # > 0: exact evaluation cache of that many positions per engine (452 B each at 9x9, 1920 B
                                                 # at 19x19): rows already evaluated skip the network, results stay bit-identical
        self.playout_cap_p_full = 1.0            # < 1: playout cap randomization (transgo_amd/playout_cap.py) -- every self-play move is a
                                                 # full search (num_simulation, root noise, recorded) with this probability, else a fast one
        self.playout_cap_fast = 0                # simulations of a fast search (no root noise, not a training position); needed when p_full < 1
        self.playout_cap_seed = 0                # seed of the full / fast draws (a hash of game seed, ply and this; no game's RNG stream is used)
        self.playout_cap_fast_noise = False      # True: fast searches get root noise too.  Only p_full = 1.0 keeps parity with the reference
        self.forced_playouts_k = 0.0             # > 0 (KataGo: 2.0): forced playouts and policy target pruning (transgo_amd/forced_playouts.py)
                                                 # in every search that begins with root noise.  Only 0.0 keeps parity with the reference
        self.gumbel_m = 0                        # > 0: Gumbel root search (transgo_amd/gumbel.py) with this many considered actions in
                                                 # every search that would begin with root noise: sequential halving at the root, the
                                                 # improved policy as the target.  Only 0 keeps parity with the reference
        self.gumbel_c_visit = 50.0               # sigma(q) = (c_visit + max visits) * c_scale * q
        self.gumbel_c_scale = 1.0
        self.search_ownership = False            # True: every search also averages the ownership head over the positions it evaluates
                                                 # (SelfPlayEngine.root_ownership; analysis).  The search itself is unchanged; refused
                                                 # together with eval_cache_entries > 0.  policy_evaluate ignores it
        self.policy_surprise_weight = 0.0        # > 0 (KataGo: 0.5): policy surprise weighting (transgo_amd/policy_surprise.py) -- finished
                                                 # games are resampled on the device before they leave the harvest: a position is
                                                 # written floor(w) or floor(w) + 1 times, w = (1 - weight) + weight * T * KL(search
                                                 # target || raw policy) / the game's sum of those.  The search is unchanged
        self.policy_surprise_seed = 0            # seed of the copy draws (a hash of game seed, position index and this)
        self.pass_alive_end = False              # True: a self-play game ends as soon as every point of its board is a pass-alive stone or
                                                 # pass-alive territory (Benson's algorithm, transgo_amd/pass_alive.py), and finished
                                                 # games are scored with the pass-alive-aware area.  The search is unchanged; only False
                                                 # keeps parity with the reference
        self.batch_size = 2048
        self.train_play_ratio = 7500 / 100000    # configure.py:61
        self.adjust_train_play_ratio = True
        self.adjust_lr = True
        self.learn_rate = 6.5e-5
        for k, v in over.items():
            setattr(self, k, v)
        from .playout_cap import check_config
        check_config(self)
        from .forced_playouts import check_k
        check_k(self.forced_playouts_k)
        from .gumbel import check_params
        check_params(self.gumbel_m, self.gumbel_c_visit, self.gumbel_c_scale)
        from .policy_surprise import check_config as check_policy_surprise
        check_policy_surprise(self)
        if self.gumbel_m > 0 and self.forced_playouts_k > 0:
            raise ValueError("gumbel_m > 0 and forced_playouts_k > 0: both are rules for the same root, choose one")
        if self.search_ownership and self.eval_cache_entries:
            raise ValueError("search_ownership and eval_cache_entries > 0: the evaluation cache stores policy and value only, so a hit "
                             "has no ownership to give; choose one")

    def epsilon_by_frame(self, game_step):       # configure.py:75-79
        return 0.65 + (1.0 - 0.65) * math.exp(-1. * game_step / 10)

    def ad_lr(self, now_play_games, current_lr):                      # configure.py:90-93
        if (now_play_games + 1) % 1500 == 0 and now_play_games < 3100 and current_lr > 0.5 * 0.5 * 6.5e-5:
            return current_lr * 0.5
        return current_lr

    def ad_train_play_ratio(self, now_play_steps, current):           # configure.py:97-103
        if (now_play_steps + 1) % 6 == 0 and current < 2.6 / 10:
            return (current * 100000 + 1) / 100000
        return current
