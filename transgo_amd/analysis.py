"""Position analysis on top of the tree read-out (tg_sp_root_children, tg_sp_pv): what a person looking at a position, a GTP
front end or somebody debugging a weight set asks a search for -- per candidate move its visits, value and prior, the root's own
value and the line the search expects.  The reference has no such interface of its own; its consumers of these numbers are
human_play.py and elo.py, which read them off the Node_V objects (self_play.py:51-95) directly.
"""
import numpy as np

_COLUMNS = "ABCDEFGHJKLMNOPQRST"           # GTP column letters: no I


def vertex(action, board_size):
    """GTP vertex of an action: column letter (I skipped) + row number counted from the bottom, so row index 0 of the action
    grid (action // board_size) is row `board_size`; board_size**2 is "pass"."""
    action, S = int(action), int(board_size)
    if action == S * S:
        return "pass"
    if not 0 <= action < S * S:
        raise ValueError(f"action {action} is not on a {S}x{S} board")
    return f"{_COLUMNS[action % S]}{S - action // S}"


def analyse(engine, states, num_simulation=0, depth=16, symmetry=None, eval_cache_entries=None, ownership=False, pass_alive=False):
    """Search every position of `states` ([N, state_size] uint8 blobs of transgo_amd.environment.GoEnv) in evaluation mode -- a
    fresh root, no root noise, as select_action's prologue (self_play.py:689-700) -- and read the trees out.  The engine's games
    are re-rooted (`reset_from`), so whatever they held is gone; the engine must have been `reset` once before (that seeds the
    streams the tie breaks draw from).  More positions than the engine has games go in successive chunks.  num_simulation 0 =
    the engine's own.  One dict per position:
      visits  int32[A]    visit count of each move           prior  float64[A]  its prior (0 where the move is illegal)
      q       float32[A]  value of the move from the mover's side, -(w / (n + 1)) in float32 -- the value_score term of
                          ucb_score (self_play.py:67-68, :716-725); NaN where the move is illegal or was never visited
      legal   bool[A]     the move is a child of the root    status  ROOT_* of SelfPlayEngine (0 = searched)
      root_value  float   w / (n + 1) of the root, from the side to move (NaN unless status is 0)
      pv      list of actions, most-visited child at each level (ties: lowest action), at most `depth`; pv_visits their visits
    symmetry: "none" | "position" | "mean8" | an int s (transgo_amd.symmetry) evaluates under that mode for this call only; the
    engine's own mode is put back afterwards, also when the search raises.  None = the engine's own.
    eval_cache_entries: an int gives the engine an exact evaluation cache of that many entries first (SelfPlayEngine.set_eval_cache;
    0 frees it) and leaves it in place for later calls -- the same results, fewer network rows when positions repeat within or
    across the searched trees.  None = the engine as it is.
    ownership: True searches with search ownership on (SelfPlayEngine.set_search_ownership) for this call -- the engine's own switch
    is put back afterwards -- and every record gains
      ownership        float32[S, S]  mean of the ownership head over the evaluations the search backed up, +1 black ... -1 white
      ownership_evals  int            how many evaluations that mean rests on (0: the map is all zero)
      score_lead       float          float32 sum of the map in point order - komi: black's lead as the search sees it
    The engine must then have no evaluation cache (it stores no ownership): asking for both raises ValueError.
    pass_alive: True adds what is settled by proof and not by opinion (tg_env_pass_alive; transgo_amd/pass_alive.py) to every record:
      pass_alive        int8[S, S]  +2 / -2 pass-alive black / white stone, +1 / -1 pass-alive territory, 0 everything else
      settled           bool        no point has status 0
      pass_alive_score  float       the pass-alive-aware area (status where it is not 0, Tromp-Taylor elsewhere) - komi
    """
    if pass_alive:
        recs = analyse(engine, states, num_simulation, depth, symmetry, eval_cache_entries, ownership)
        st = np.ascontiguousarray(states, np.uint8)
        N, S = st.shape[0], engine.S
        status = np.zeros((N, S * S), np.int8); settled = np.zeros(N, np.uint8); score = np.zeros(N, np.float32)
        if N:
            engine.ctx.call("tg_env_pass_alive", st.ctypes.data, N, status.ctypes.data, settled.ctypes.data, score.ctypes.data, None)
        for i, r in enumerate(recs):
            r.update(pass_alive=status[i].reshape(S, S).copy(), settled=bool(settled[i]), pass_alive_score=float(score[i]))
        return recs
    states = np.ascontiguousarray(states, np.uint8)
    if states.ndim != 2:
        raise ValueError("states must be [N, state_size]")
    if ownership and eval_cache_entries:
        raise ValueError("analyse: ownership=True and eval_cache_entries > 0: the evaluation cache stores policy and value only, so a "
                         "position it serves has no ownership to add to the mean")
    if eval_cache_entries is not None:
        engine.set_eval_cache(eval_cache_entries)
    if symmetry is not None:
        old = engine.get_symmetry()
        engine.set_symmetry(symmetry, old[1] if symmetry == "position" and old[0] == 2 else 0)
        try:
            return analyse(engine, states, num_simulation, depth, ownership=ownership)
        finally:
            engine.set_symmetry(("none", "fixed", "position", "mean8")[old[0]], old[1])
    if ownership and not engine.get_search_ownership():
        engine.set_search_ownership(True)                  # (an attached evaluation cache makes the library refuse, with the reason)
        try:
            return analyse(engine, states, num_simulation, depth, ownership=True)
        finally:
            engine.set_search_ownership(False)
    G, N = engine.G, states.shape[0]
    out = []
    for lo in range(0, N, G):
        k = min(G, N - lo)
        batch = np.repeat(states[lo:lo + 1], G, axis=0)              # slots past the chunk hold a copy and are masked out (parked)
        batch[:k] = states[lo:lo + k]
        mask = np.zeros(G, np.uint8); mask[:k] = 1
        engine.reset_from(batch, None if k == G else mask)
        engine.search(selfplay=False, num_simulation=num_simulation)
        rc = engine.root_children()
        act, vis, _, ln = engine.principal_variation(depth)
        so = engine.root_ownership() if ownership else None
        for g in range(k):
            present = (rc["flags"][g] & engine.CHILD_PRESENT) != 0
            n, w = rc["n"][g], rc["w"][g]
            q = np.full(engine.A, np.nan, np.float32)
            seen = present & (n > 0)
            q[seen] = -(w[seen] / (n[seen] + 1).astype(np.float32))
            ok = rc["status"][g] == engine.ROOT_OK
            root_value = float(rc["root_w"][g] / np.float32(rc["root_n"][g] + 1)) if ok else float("nan")
            m = max(int(ln[g]), 0)
            out.append(dict(visits=n.copy(), prior=rc["prior"][g].copy(), q=q, legal=present, status=int(rc["status"][g]),
                            root_value=root_value, pv=[int(a) for a in act[g, :m]], pv_visits=[int(v) for v in vis[g, :m]]))
            if so is not None:
                out[-1].update(ownership=so["mean"][g].copy(), ownership_evals=int(so["n"][g]), score_lead=float(so["score_lead"][g]))
    return out


def symmetry_spread(net, states):
    """How far a weight set is from equivariance: every position of `states` ([N, state_size] blobs) evaluated by `net` (a
    transgo_amd.model.HipNetwork of the same board size and planes) under each of the eight symmetries (mode "fixed", s = 0..7),
    outputs mapped back to the position's own orientation.  One dict per position: "policy" / "value" = the largest absolute
    difference between any two of the eight policies / values (0 = the network gives one answer in every orientation).  The
    network's own mode is put back afterwards."""
    import ctypes
    states = np.ascontiguousarray(states, np.uint8)
    if states.ndim != 2:
        raise ValueError("states must be [N, state_size]")
    N = states.shape[0]
    if N == 0:
        return []
    obs = np.zeros((N, net.C, net.S, net.S), np.float32)
    net.ctx.call("tg_env_query", states.ctypes.data_as(ctypes.c_void_p), N, None, None, obs.ctypes.data_as(ctypes.c_void_p),
                 None, None, None, None, None)
    old = net.get_symmetry()
    try:
        pols, vals = [], []
        for s in range(8):
            net.set_symmetry(s)
            p, v, _ = net.main_prediction(obs)
            pols.append(p); vals.append(v.reshape(N))
    finally:
        net.set_symmetry(("none", "fixed", "position", "mean8")[old[0]], old[1])
    pols, vals = np.stack(pols), np.stack(vals)
    return [dict(policy=float((pols[:, i].max(0) - pols[:, i].min(0)).max()), value=float(vals[:, i].max() - vals[:, i].min()))
            for i in range(N)]


def playout_ownership(env, states, playouts=64, seed=0):
    """The network-free Monte-Carlo estimate of every position of `states` ([N, state_size] blobs of `env`, a
    transgo_amd.environment.GoEnv): `playouts` uniformly random no-eye games per position, all N * playouts of them in ONE
    kernel launch (GoEnv.rollout_batch; game k of position i is seeded seed + i * playouts + k), each scored by Tromp-Taylor.
    One dict per position:
      territory  float64[P]  mean owner of each point over the games, +1 black / -1 white (an integer sum / playouts)
      score      float       mean of getScore (Tromp-Taylor - komi) over the games
      black_win  float       share of the games black wins (score > 0, environment.py:118-119)
      playouts   int"""
    states = np.ascontiguousarray(states, np.uint8)
    if states.ndim != 2:
        raise ValueError("states must be [N, state_size]")
    N, K = states.shape[0], int(playouts)
    if K <= 0:
        raise ValueError("playouts must be positive")
    if N == 0:
        return []
    seeds = (int(seed) + np.arange(N * K, dtype=np.int64)) % (2 ** 32)
    end = env.rollout_batch(np.repeat(states, K, axis=0), seeds=seeds)["states"]
    q = env.query_batch(end, score=True, terr=True)
    terr = q["terr"].astype(np.int64).reshape(N, K, -1)               # exactly -1 / 0 / +1
    score = q["score"].astype(np.float64).reshape(N, K)
    return [dict(territory=terr[i].sum(0) / K, score=float(score[i].sum() / K), black_win=float((score[i] > 0).sum() / K),
                 playouts=K) for i in range(N)]


def format_ownership(record, board_size):
    """The territory map of one `playout_ownership` record as a board of percentages (+100 black ... -100 white), with the mean
    score and black's win rate on top.  An `analyse(..., ownership=True)` record prints the same board from its search ownership,
    under the number of evaluations and the score lead."""
    S = int(board_size)
    if "territory" in record:
        t = np.asarray(record["territory"]).reshape(S, S)
        head = f"playouts {int(record['playouts'])}   mean score {record['score']:+.2f}   black wins {100 * record['black_win']:.1f}%"
    else:
        t = np.asarray(record["ownership"]).reshape(S, S)
        head = f"search ownership over {int(record['ownership_evals'])} evaluations   score lead {record['score_lead']:+.2f}"
    lines = [head, "    " + " ".join(f"{c:>4}" for c in _COLUMNS[:S])]
    for y in range(S):
        lines.append(f"{S - y:>3} " + " ".join(f"{int(round(100 * v)):>+4d}" for v in t[y]))
    return "\n".join(lines)


def format_analysis(record, board_size, top=5, ownership=None):
    """A table of the `top` candidate moves of one `analyse` record: one line per candidate in descending visits (ties: ascending
    action) with its vertex, visits, q, prior and its line -- the principal variation for the move that heads it, the move alone
    for the others.  A q that is NaN (never visited) prints as '-'.  `ownership`: a `playout_ownership` record of the same
    position, printed underneath (format_ownership).  A record that carries its own search ownership (analyse(..., ownership=True))
    prints that board too.  A record with a pass-alive status (analyse(..., pass_alive=True)) gains a column `pa` -- the status of
    the candidate's point: B / W a pass-alive stone, b / w pass-alive territory, . unsettled -- and a line with the settled flag and
    the pass-alive-aware score."""
    status = np.asarray(record["pass_alive"]).reshape(-1) if "pass_alive" in record else None
    mark = lambda a: "" if status is None else f"{'-' if a >= len(status) else {2: 'B', 1: 'b', 0: '.', -1: 'w', -2: 'W'}[int(status[a])]:>4}"
    visits, prior, q = np.asarray(record["visits"]), np.asarray(record["prior"]), np.asarray(record["q"])
    legal = np.asarray(record["legal"]) if "legal" in record else (visits > 0) | (prior > 0)
    cand = sorted(np.flatnonzero(legal), key=lambda a: (-int(visits[a]), int(a)))[:max(int(top), 0)]
    pv = list(record.get("pv", []))
    rv = record.get("root_value", float("nan"))
    lines = [f"root value {'-' if np.isnan(rv) else format(rv, '+.3f')}   visits {int(visits.sum())}",
             f"{'move':<5}{'visits':>8}{'q':>8}{'prior':>8}{'' if status is None else '  pa'}  pv"]
    for a in cand:
        qs = "-" if np.isnan(q[a]) else format(float(q[a]), "+.3f")
        line = pv if pv and pv[0] == a else [a]
        lines.append(f"{vertex(a, board_size):<5}{int(visits[a]):>8}{qs:>8}{float(prior[a]):>8.4f}{mark(a)}  "
                     + " ".join(vertex(m, board_size) for m in line))
    if status is not None:
        lines.append(f"pass-alive: {'settled' if record['settled'] else 'not settled'}, {int((status != 0).sum())} of {len(status)} points decided, "
                     f"score {record['pass_alive_score']:+.1f}")
    if "ownership" in record:
        lines.append(format_ownership(record, board_size))
    if ownership is not None:
        lines.append(format_ownership(ownership, board_size))
    return "\n".join(lines)
