"""Forced playouts and policy target pruning on the device (tg_sp_forced_playouts, k_collect_forced, pruned_counts in k_play_forced
and tg_sp_root_visits_pruned) against the oracle search with the same rule (tests/forced_playouts_ref.py, written with the
definition in transgo_amd/forced_playouts.py), on the same seeds: everything compared is bit-identical.

The oracle games and the engine runs are computed once and shared.  tests/test_forced_playouts_host.py holds the condition on
the inputs (k = 2 really changes the search for these evaluators and seeds) on the CPU."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import evaluators
from transgo_amd import forced_playouts as fp

K, R = 2.0, 4
CASES = {                                   # name -> (evaluator, board, games, simulations, moves, max_step, first seed)
    "sharp9": ("sharp", 9, 8, 64, 6, 6, 500),         # max_step = 6: the games end with their sixth move and are harvested
    "flat9": ("flat", 9, 8, 64, 6, 6, 500),
    "sharp19": ("sharp", 19, 2, 32, 2, 450, 700),     # 362 children: the multi-pass child loops
}


def _seeds(case):
    _, _, G, _, _, _, s0 = CASES[case]
    return np.arange(s0, s0 + G).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(case, k=K, noised=None):
    """Per game the list of its moves (tests/forced_playouts_ref.play_moves); noised: per-game tuple of switches (default all)."""
    from tests.forced_playouts_ref import play_moves
    name, S, G, sims, moves, max_step, _ = CASES[case]
    games, sel, hit = [], 0, 0
    for g, s in enumerate(_seeds(case)):
        mv, o = play_moves(evaluators.BY_NAME[name], int(s), k, moves, sims, board_size=S, max_step=max_step, readouts=R,
                           selfplay=True if noised is None else bool(noised[g]))
        games.append(mv); sel += o.root_selections; hit += o.forced_selections
    return dict(games=games, stats=dict(root_selections=sel, forced_selections=hit))


def _engine(case, **kw):
    from transgo_amd.engine import SelfPlayEngine
    name, S, G, sims, _, max_step, _ = CASES[case]
    return SelfPlayEngine(G, board_size=S, num_simulation=sims, parallel_readouts=R, max_step=max_step, evaluator=evaluators.BY_NAME[name], **kw)


def _move(eng, search):
    """One searched move of every game; `search` issues the search.  Returns what the move looked like, the move played."""
    live = ~eng.finished
    search()
    raw, _, _, st, _ = eng.root_info(obs=False)
    pruned, st2 = eng.root_visits(pruned=True)
    assert np.array_equal(st, st2)
    pg = eng.pruned_games()
    tables = eng.root_children()
    acts, pis = eng.choose_moves(pruned, st)
    done = eng.play(acts)
    ch = eng.root_children()
    return dict(live=live, raw=raw, pruned=pruned, pg=pg, acts=acts, pis=pis, done=done, new_root_n=ch["root_n"], status=ch["status"], tables=tables,
                pos=np.array([eng.rng_state(g)[1] for g in range(eng.G)]))


@functools.lru_cache(maxsize=None)
def _run(case):
    """The engine's side of a case with k = 2: every move, the harvests, the record as a snapshot holds it, the counters."""
    from transgo_amd import snapshot
    _, S, G, _, moves, _, _ = CASES[case]
    eng = _engine(case, forced_playouts_k=K)
    assert eng.get_forced_playouts() == K
    eng.reset(_seeds(case))
    out, harvests = [], []
    for _ in range(moves):
        if eng.finished.all():
            break
        mv = _move(eng, lambda: eng.search(True))
        out.append(mv)
        if (mv["done"] & mv["live"]).any():
            harvests.append(eng.harvest(device=False, seeds=_seeds(case)))
    snap = eng.snapshot()
    hdr = snapshot.parse_header(snap)
    hist = snapshot.section(snap, hdr, "hist_cnt", np.int32).reshape(-1, S * S + 1).copy()
    stats, errors = eng.forced_playouts_stats(), eng.stats()["errors"]
    eng.close()
    return dict(moves=out, harvests=harvests, hist=hist, stats=stats, errors=errors)


def _compare(run, games, noised=None):
    """Every way the engine's moves differ from the oracle's games (empty = equal)."""
    bad = []
    for m, mv in enumerate(run["moves"]):
        for g in np.flatnonzero(mv["live"]):
            if m >= len(games[g]):
                bad.append((g, m, "the oracle's game is over")); continue
            om = games[g][m]
            forced = noised is None or bool(noised[g])
            for what, a, b in (("raw root visits", mv["raw"][g], om["raw"]), ("pruned visits", mv["pruned"][g], om["pruned"]),
                               ("pi", mv["pis"][g], om["pi"])):
                if not np.array_equal(a, b):
                    bad.append((g, m, what))
            if int(mv["acts"][g]) != om["action"]:
                bad.append((g, m, "action"))
            if int(mv["pos"][g]) != om["pos"]:
                bad.append((g, m, "MT19937 stream position"))
            if bool(mv["pg"][g]) != forced:
                bad.append((g, m, "pruned_game flag"))
        # the read-out kernel against the definition's array form fed with the tree as tg_sp_root_children shows it
        if not np.array_equal(fp.prune_tables(K, 3, 0.05, mv["tables"], mv["pg"]), mv["pruned"]):
            bad.append((-1, m, "prune_tables(root_children()) != tg_sp_root_visits_pruned"))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sharp9", "flat9"])
def test_forced_search_against_the_oracle_9x9(case):
    """1. 8 games, 64 simulations, 6 moves, k = 2: raw root visits, pruned visits, pi, chosen moves and the stream position of every
    game and move are the oracle's; pruning happened; the harvested counts are the pruned ones; the counters of forced root
    selections are the oracle's."""
    run, games = _run(case), _oracle(case)["games"]
    A = 82
    assert run["errors"] == 0 and len(run["moves"]) == 6
    assert _compare(run, games) == []
    assert any((mv["raw"] != mv["pruned"]).any() for mv in run["moves"])
    seen = set()
    for h in run["harvests"]:
        cnt, nm = h.view("counts").reshape(-1, A), h.view("n_moves")
        o = 0
        for i, g in enumerate(h.view("slot")):
            want = np.array([m["pruned"] for m in games[int(g)]], np.int32)
            assert int(nm[i]) == len(want) and np.array_equal(cnt[o:o + len(want)], want), int(g)
            o += len(want); seen.add(int(g))
    assert seen == set(range(8))
    want = _oracle(case)["stats"]
    assert run["stats"] == want and 0 < want["forced_selections"] < want["root_selections"]


@pytest.mark.gpu
def test_forced_search_against_the_oracle_19x19():
    """2. 19x19, 2 games, 32 simulations, 2 moves: the same comparisons through the multi-pass child loops; the counts k_play_forced
    recorded (read from a snapshot's hist_cnt section: the games are still running) are the pruned ones."""
    run, games = _run("sharp19"), _oracle("sharp19")["games"]
    assert run["errors"] == 0 and len(run["moves"]) == 2
    assert _compare(run, games) == []
    assert any((mv["raw"] != mv["pruned"]).any() for mv in run["moves"])
    want = np.array([m["pruned"] for g in games for m in g], np.int32)
    assert np.array_equal(run["hist"], want)


@pytest.mark.gpu
def test_mixed_batch_full_and_fast_games():
    """3. tg_sp_begin_move_games with half the games noised (full) and half not: the games without noise are bit-identical to the
    same games in an engine with k = 0, the noised ones match the oracle twin."""
    case = "sharp9"
    _, S, G, sims, _, _, _ = CASES[case]
    noised = tuple(g % 2 == 0 for g in range(G))
    nz = np.array(noised)
    budget = np.where(nz, sims, 24)

    def run(k, moves=3):
        eng = _engine(case, forced_playouts_k=k)
        eng.reset(_seeds(case))
        out = [_move(eng, lambda: eng.search(True, budget, noise=nz, record=nz)) for _ in range(moves)]
        eng.close()
        return out
    forced, plain = run(K), run(0.0)
    fast = ~nz
    for a, b in zip(forced, plain):
        assert not b["pg"].any() and np.array_equal(a["pg"], nz & a["live"])
        for key in ("raw", "pruned", "acts", "pis", "pos", "new_root_n"):
            assert np.array_equal(a[key][fast], b[key][fast]), key
        assert np.array_equal(a["raw"][fast], a["pruned"][fast])
    assert any(not np.array_equal(a["raw"][nz], b["raw"][nz]) for a, b in zip(forced, plain))
    # the oracle twin of the noised games: the same budget every move, noise every move (the fast games' twins are not needed)
    twins = _oracle(case)["games"]
    for m, mv in enumerate(forced):
        for g in np.flatnonzero(nz):
            om = twins[g][m]
            assert np.array_equal(mv["raw"][g], om["raw"]) and np.array_equal(mv["pruned"][g], om["pruned"]), (g, m)
            assert int(mv["acts"][g]) == om["action"] and int(mv["pos"][g]) == om["pos"], (g, m)


@pytest.mark.gpu
def test_off_is_off():
    """4. k = 0 set, the call never made, and k = 2 set and put back to 0: identical visits, moves, streams and records over 4 moves."""
    from transgo_amd import snapshot
    case = "sharp9"

    def run(prepare):
        eng = _engine(case)
        prepare(eng)
        eng.reset(_seeds(case))
        out = []
        for _ in range(4):
            eng.search(True)
            vis, st = eng.root_visits()
            pr, _ = eng.root_visits(pruned=True)
            assert np.array_equal(vis, pr) and not eng.pruned_games().any()
            acts, pis = eng.choose_moves(vis, st)
            eng.play(acts)
            out.append((vis.tobytes(), acts.tobytes(), pis.tobytes(), eng.rng_streams().tobytes()))
        snap = eng.snapshot()
        out.append(snapshot.section(snap, snapshot.parse_header(snap), "hist_cnt").tobytes())
        out.append(eng.forced_playouts_stats())
        eng.close()
        return out
    a = run(lambda e: e.set_forced_playouts(0.0))
    b = run(lambda e: None)
    c = run(lambda e: (e.set_forced_playouts(2.0), e.set_forced_playouts(0.0)))
    assert a == b == c and a[-1] == dict(root_selections=0, forced_selections=0)


@pytest.mark.gpu
def test_argument_checks():
    """5. Negative k is refused; the call is refused while a leaf batch is pending; tg_sp_root_visits_pruned before a reset names
    tg_sp_reset."""
    from transgo_amd import _lib
    eng = _engine("sharp9")
    vis = np.zeros((eng.G, eng.A), np.int32)
    with pytest.raises(_lib.TransgoError, match="tg_sp_reset"):
        eng.ctx.call("tg_sp_root_visits_pruned", vis.ctypes.data_as(ctypes.c_void_p), None)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.TransgoError, match="tg_sp_forced_playouts"):
            eng.ctx.call("tg_sp_forced_playouts", ctypes.c_double(bad))
    with pytest.raises(ValueError, match="forced_playouts_k"):
        eng.set_forced_playouts(-2.0)
    eng.set_forced_playouts(1e305)                                    # finite: accepted on both sides
    assert eng.get_forced_playouts() == 1e305
    eng.set_forced_playouts(1.5)
    assert eng.get_forced_playouts() == 1.5
    eng.reset(_seeds("sharp9"))
    eng.ctx.call("tg_sp_begin_move", 1, 0)
    act, rows = ctypes.c_int32(), ctypes.c_int32()
    eng.ctx.call("tg_sp_collect", ctypes.byref(act), ctypes.byref(rows))
    assert rows.value > 0
    with pytest.raises(_lib.TransgoError, match="batch is pending"):
        eng.ctx.call("tg_sp_forced_playouts", ctypes.c_double(2.0))
    assert eng.get_forced_playouts() == 1.5
    eng._evaluate(rows.value)
    eng.ctx.call("tg_sp_absorb")
    eng.set_forced_playouts(0.0)
    assert eng.get_forced_playouts() == 0.0
    eng.close()


@pytest.mark.gpu
def test_tree_reuse_sees_the_unpruned_statistics():
    """6. After a forced move is played the new root's n (tg_sp_root_children) is the chosen child's unpruned n, also where the
    pruning took visits from that child."""
    run, games = _run("sharp9"), _oracle("sharp9")["games"]
    checked = cut = 0
    for m, mv in enumerate(run["moves"]):
        for g in np.flatnonzero(mv["live"]):
            a = int(mv["acts"][g])
            assert int(mv["new_root_n"][g]) == int(mv["raw"][g, a]) == games[g][m]["child_n"] == games[g][m]["new_root_n"], (g, m)
            checked += 1
            cut += int(mv["pruned"][g, a] < mv["raw"][g, a])
    assert checked == 8 * 6 and cut > 0


@pytest.mark.gpu
def test_batched_self_play_forces_the_full_plies_only():
    """BatchedSelfPlay with the playout cap on and k = 2: at move selection exactly the live games on a full ply are pruned games,
    the others choose from raw counts; a restored worker gets k back from its Config."""
    from transgo_amd import playout_cap
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    cfg = Config(num_simulation=48, max_step=8, playout_cap_p_full=0.5, playout_cap_fast=16, playout_cap_seed=0, forced_playouts_k=K)
    sp = BatchedSelfPlay(cfg, 8, evaluator=evaluators.sharp)
    sp.start()
    eng, seen = sp.engine, []
    choose = eng.choose_moves

    def spy(vis, steps, selfplay=True):
        seen.append((eng.pruned_games(), vis.copy(), eng.root_info(obs=False)[0]))
        return choose(vis, steps, selfplay)
    eng.choose_moves = spy
    assert eng.get_forced_playouts() == K
    harvested = cut = 0
    for _ in range(10):
        full = playout_cap.schedule(sp.seeds, eng.root_plies(), 0.5, 0) & ~eng.finished
        h = sp.advance()
        pg, vis, raw = seen[-1]
        assert np.array_equal(pg, full)
        assert np.array_equal(vis[~pg], raw[~pg]) and (vis <= raw).all()
        cut += int((vis[pg] < raw[pg]).sum())
        harvested += 0 if h is None else h.n_positions
    assert cut > 0 and harvested > 0 and 0 < sp.full_moves < sp.moves_played and eng.stats()["errors"] == 0
    state, snap = sp.checkpoint_state(), eng.snapshot()
    eng.set_forced_playouts(0.0)
    sp._restore_part(state, snap)
    assert eng.get_forced_playouts() == K
    eng.close()


@pytest.mark.gpu
def test_masked_reset_ends_the_forced_move_of_the_restarted_slots_only():
    """A reset of some slots between a forced search's end and the move: the restarted slots are no forced games any more, the
    others still are and still report their pruned counts."""
    case = "sharp9"
    eng = _engine(case, forced_playouts_k=K)
    eng.reset(_seeds(case))
    eng.search(True)
    before, _ = eng.root_visits(pruned=True)
    assert eng.pruned_games().all()
    mask = np.zeros(eng.G, bool); mask[[0, 3]] = True
    eng.reset(_seeds(case), mask)
    assert np.array_equal(eng.pruned_games(), ~mask)
    after, _ = eng.root_visits(pruned=True)
    assert np.array_equal(after[~mask], before[~mask]) and not after[mask].any()
    eng.close()


@pytest.mark.gpu
def test_wp_mcts_returns_the_pruned_pi():
    """The reference-shaped single-tree object with Config.forced_playouts_k = 2: get_action_probs' action and pi are the oracle
    twin's (from pruned counts), and the counts update_with_action recorded are the pruned ones -- pi and record agree."""
    from transgo_amd.configure import Config
    from transgo_amd.self_play import WP_MCTS
    name, S, G, sims, moves, max_step, s0 = CASES["sharp9"]
    game = _oracle("sharp9")["games"][0]
    mcts = WP_MCTS(Config(num_simulation=sims, max_step=max_step, forced_playouts_k=K), seed=s0, evaluator=evaluators.BY_NAME[name])
    done = False
    for m, om in enumerate(game):
        a, pi, _ = mcts.get_action_probs()
        assert a == om["action"] and np.array_equal(pi, om["pi"]), m
        done = mcts.update_with_action(a)
    assert done
    h = mcts.engine.harvest(device=False)
    want = np.array([om["pruned"] for om in game], np.int32)
    assert np.array_equal(h.view("counts").reshape(-1, 82), want)
    assert any((om["raw"] != om["pruned"]).any() for om in game)
    mcts.close()
