"""Checkpoint and resume (tg_sp_snapshot / tg_sp_restore, BatchedSelfPlay.save_checkpoint, DeviceReplayMemory.save): a population
restored into a fresh context continues BIT-IDENTICALLY to the one that was never stopped, and taking a snapshot changes nothing.

All searches but one use the host evaluators of oracle/evaluators.py, so every run is deterministic and needs no network."""
import ctypes

import numpy as np
import pytest

from oracle import evaluators

pytestmark = pytest.mark.gpu

# The sections of a snapshot that two runs of the same games must agree on byte for byte.  WHICH chunk of the pool a tree gets is
# decided by the order in which the games' workgroups draw their tickets on the ring, so chunk ids -- and with them the slot
# indices in GameCtl (root, free_slot, spare), the ring's order and the tree section -- may differ between two runs that play
# identically; everything else may not.
EXACT_SECTIONS = ("game_ctl", "pool_ctl", "counters", "moves", "finished", "rng", "hist_obs", "hist_cnt", "hist_pl")


def _worker(G=24, sims=48, max_step=12, S=9, **kw):
    from transgo_amd.configure import Config
    from transgo_amd.self_play import BatchedSelfPlay
    cfg = Config(num_simulation=sims, max_step=max_step, board_size=S, stagger_games=kw.pop("stagger", 0))
    sp = BatchedSelfPlay(cfg, G, evaluator=kw.pop("evaluator", evaluators.sharp), **kw)
    sp.log = {"visits": [], "actions": []}
    eng = sp.engine
    rv, cm = eng.root_visits, eng.choose_moves

    def root_visits():
        out = rv(); sp.log["visits"].append(out[0].tobytes()); return out

    def choose_moves(*a, **k):
        out = cm(*a, **k); sp.log["actions"].append(out[0].tobytes()); return out
    eng.root_visits, eng.choose_moves = root_visits, choose_moves
    return sp


def _advance(sp, n):
    """n moves; per move everything observable: root visit tables, chosen actions, the harvest's bytes, RNG streams, counters."""
    out = []
    for _ in range(n):
        nv = len(sp.log["visits"])
        h = sp.advance()
        eng = sp.engine
        out.append({"visits": sp.log["visits"][nv:], "actions": sp.log["actions"][nv:],
                    "harvest": None if h is None else h.to_host().buf.tobytes(),
                    "rng": eng.rng_streams().tobytes(), "stats": sorted(eng.stats().items()), "pool": sorted(eng.pool_stats().items()),
                    "worker": (sp.games_started.tobytes(), sp.seeds.tobytes(), sp.moves_played, sp.games_finished, sp.games_dropped,
                               sp.last_live, eng.finished.tobytes(), eng.errored.tobytes())})
    return out


def _same(a, b, what=""):
    assert len(a) == len(b)
    for m, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert x[k] == y[k], f"{what}move {m}: {k} differs"


def _exact_sections(eng):
    from transgo_amd import snapshot
    buf = eng.snapshot()
    hdr = snapshot.parse_header(buf)
    out = {k: snapshot.section(buf, hdr, k).tobytes() for k in EXACT_SECTIONS}
    ctl = snapshot.section(buf, hdr, "game_ctl", snapshot.GAME_CTL).copy()
    ctl["spare"] = ctl["spare"] >= 0
    ctl["root"] = 0; ctl["free_slot"] %= hdr["chunk_slots"]          # where in its chunk the tree ends, not which chunk that is
    out["game_ctl"] = ctl.tobytes()                                   # per-game counters, high-water marks, chunk counts, flags
    return out, hdr


def _twin(tmp_path, before, after, at_snapshot=None, **kw):
    """Run A: `before` moves, checkpoint, `after` moves.  Run B: a fresh worker loads the checkpoint and plays `after` moves.
    Run C: never snapshotted.  B == A's continuation, C == A.  at_snapshot(worker) looks at A when the checkpoint is taken and
    at B right after it was loaded."""
    path = str(tmp_path / "ckpt.bin")
    a = _worker(**kw)
    log_a = _advance(a, before)
    if at_snapshot:
        at_snapshot(a)
    a.save_checkpoint(path)
    log_a += _advance(a, after)
    b = _worker(**kw)
    b.load_checkpoint(path)
    if at_snapshot:
        at_snapshot(b)
    log_b = _advance(b, after)
    _same(log_a[before:], log_b, "restored run, ")
    c = _worker(**kw)
    log_c = _advance(c, before + after)
    _same(log_a, log_c, "undisturbed run, ")
    sa, hdr = _exact_sections(a.engine)
    sb, _ = _exact_sections(b.engine)
    sc, _ = _exact_sections(c.engine)
    for k in EXACT_SECTIONS:
        assert sa[k] == sb[k], f"final state: section {k} differs after a restore"
        assert sa[k] == sc[k], f"final state: section {k} differs from the undisturbed run"
    for w in (a, b, c):
        w.engine.close()
    return log_a, hdr, np.frombuffer(sa["pool_ctl"], np.uint64)


def test_twin_continuation_9x9(tmp_path):
    log, hdr, pool = _twin(tmp_path, 7, 9)
    # the run is the one the issue asks for: games ended and restarted inside it, trees span several chunks, the ring was pushed and popped
    assert sum(m["harvest"] is not None for m in log) >= 1 and log[-1]["worker"][3] >= 24
    assert hdr["tree_chunks"] > hdr["n_games"]
    assert pool[0] > hdr["n_games"] and pool[1] > hdr["pool_chunks"]     # PoolCtl head / tail: chunks were popped, and pushed back past the ring's end


def test_twin_continuation_19x19(tmp_path):
    _, hdr, _ = _twin(tmp_path, 3, 3, G=4, sims=32, max_step=120, S=19)
    assert hdr["board_size"] == 19 and hdr["chunk_slots"] == 4096


def test_twin_with_staggered_start(tmp_path):
    def still_parked(w):                                             # after 2 steps slots g mod 4 >= 2 wait for their first move
        assert w._parked.tolist() == [g % 4 >= 2 for g in range(12)]
    log, _, _ = _twin(tmp_path, 2, 4, at_snapshot=still_parked, G=12, sims=24, stagger=4)
    assert log[-1]["worker"][5] == 12                                # last_live: every slot plays by the end


def _engine(G, sims, **kw):
    from transgo_amd.engine import SelfPlayEngine
    return SelfPlayEngine(G, num_simulation=sims, evaluator=kw.pop("evaluator", evaluators.sharp), net_blocks=2, net_filters=32, **kw)


def _move(eng, num_simulation=0):
    eng.search(True, num_simulation)
    vis, st = eng.root_visits()
    acts, _ = eng.choose_moves(vis, st)
    done = eng.play(acts)
    return (vis.tobytes(), acts.tobytes(), done.tobytes(), eng.errored.tobytes(), eng.rng_streams().tobytes(), sorted(eng.stats().items()),
            eng.game_errors().tobytes())


def _move_and_restart(eng, k):
    """_move, then what BatchedSelfPlay.advance does at a game's end: harvest, and restart the slots that are over or in error."""
    out = _move(eng)
    h = eng.harvest()
    restart = np.frombuffer(out[2], bool) | eng.errored
    if restart.any():
        eng.reset(1000 * (k + 1) + np.arange(eng.G), restart)
    return out + (None if h is None else h.buf.tobytes(), eng.rng_streams().tobytes(), eng.finished.tobytes())


def test_twin_with_a_game_parked_in_error():
    # a per-game cap of four chunks holds 48 blocks of a young game: the root's and 47 leaves'.  A 46-simulation search runs 12 waves
    # of 4 paths, so it overflows the cap in the games where no two paths of a wave met in the same leaf, and fits in the others
    kw = dict(arena_slots=3000)
    a = _engine(16, 46, **kw)
    a.reset(np.arange(16))
    log_a = [_move(a) for _ in range(2)]
    err = a.game_errors()
    print("games parked in error:", int((err != 0).sum()), "of 16")
    assert a.errored.any() and not a.errored.all(), "the case needs games parked in error next to games that play on"
    snap = a.snapshot()
    b = _engine(16, 46, **kw)
    b.restore(snap)
    assert (b.game_errors() == err).all() and (b.errored == a.errored).all() and (b.finished == a.finished).all()
    assert (b.errored == (err != 0)).all()                           # done == 2: parked, neither over nor playable
    for m in range(4):
        log_a.append(_move(a))
        assert log_a[-1] == _move(b), m
    c = _engine(16, 46, **kw)                                        # the undisturbed run: the snapshot only read
    c.reset(np.arange(16))
    for m in range(6):
        assert _move(c) == log_a[m], m
    for e in (a, b, c):
        e.close()


def test_twin_with_unharvested_games():
    """Snapshot after play() and BEFORE harvest(), in a mixed population: slots 4-7 have just played their last ply, slots 0-3 were
    restarted two moves ago and are in mid-game.  The harvest taken after the restore equals the original's, and both contexts then
    restart the finished slots and play on identically (more games end and restart inside those moves)."""
    def upto_snapshot(e):
        e.reset(np.arange(8))
        log = [_move(e) for _ in range(2)]
        e.reset(100 + np.arange(8), np.arange(8) < 4)                # slots 0-3 start new games: they are two plies behind from here on
        return log + [_move(e) for _ in range(2)]

    def harvest_and_restart(e):
        h = e.harvest()
        e.reset(200 + np.arange(8), e.finished.copy())
        return h.buf.tobytes(), h.n_games
    kw = dict(max_step=4)
    a = _engine(8, 12, **kw)
    log_a = upto_snapshot(a)
    assert a.finished.tolist() == [False] * 4 + [True] * 4
    snap = a.snapshot()                                              # fin_slot / fin_off / fin_positions are not empty here
    b = _engine(8, 12, **kw)
    b.restore(snap)
    assert (b.finished == a.finished).all()
    ha, hb = harvest_and_restart(a), harvest_and_restart(b)
    assert ha == hb and ha[1] == 4
    for m in range(4):
        log_a.append(_move_and_restart(a, m))
        assert log_a[-1] == _move_and_restart(b, m), m
    assert sum(x[-3] is not None for x in log_a[4:]) >= 2            # both halves of the population finished games after the restore
    c = _engine(8, 12, **kw)                                         # the undisturbed run
    assert upto_snapshot(c) == log_a[:4]
    assert harvest_and_restart(c) == ha
    for m in range(4):
        assert _move_and_restart(c, m) == log_a[4 + m], m
    for e in (a, b, c):
        e.close()


def test_packed_not_dumped():
    from transgo_amd import snapshot
    G = 8
    eng = _engine(G, 32, pool_slots=65536)
    eng.reset(np.arange(G))
    for _ in range(3):
        _move(eng)
    n = ctypes.c_uint64(); w = ctypes.c_uint64()
    eng.ctx.call("tg_sp_snapshot_size", ctypes.byref(n))
    buf = np.empty(n.value + 64, np.uint8)
    eng.ctx.call("tg_sp_snapshot", buf.ctypes.data_as(ctypes.c_void_p), buf.size, 0, ctypes.byref(w))
    assert w.value == n.value
    hdr = snapshot.parse_header(buf[:w.value])
    ctl = snapshot.section(buf, hdr, "game_ctl", snapshot.GAME_CTL)
    owned = int(ctl["n_chunks"].sum() + (ctl["spare"] >= 0).sum())
    assert hdr["tree_chunks"] == owned
    assert hdr["sections"]["tree"][1] == owned * hdr["chunk_slots"] * 32
    pool = eng.pool_stats()
    assert hdr["sections"]["tree"][1] == pool["pool_in_use"] * 32    # what tg_sp_pool_stats calls in use
    assert pool["pool_slots"] >= 8 * pool["pool_in_use"]             # the pool is provisioned 8x beyond what the run uses ...
    assert w.value < pool["pool_slots"] * 32 // 4                    # ... and the snapshot does not pay for it
    ids = snapshot.section(buf, hdr, "chunk_ids", np.int32)
    assert len(set(ids.tolist())) == owned and ids.min() >= 0 and ids.max() < hdr["pool_chunks"]
    eng.close()


def test_device_round_trip_and_fork():
    import torch
    a = _engine(8, 32)
    a.reset(np.arange(100, 108))
    for _ in range(3):
        _move(a)
    snap = a.snapshot(device=True)
    assert isinstance(snap, torch.Tensor) and snap.is_cuda and snap.dtype == torch.uint8
    b = _engine(8, 32)
    b.restore(snap)                                                  # HBM -> HBM, same GPU, no host copy of the buffer
    first_b = _move(b)
    assert _move(a) == first_b
    assert _move(a) == _move(b)
    a.restore(snap)                                                  # the fork: the same position continued differently
    first_a = _move(a, num_simulation=16)
    assert first_a[0] != first_b[0]                                  # negative control: the comparison can fail
    a.restore(snap)
    assert _move(a) == first_b                                       # and a third continuation equals the first again
    a.close(); b.close()


def test_with_the_network():
    from transgo_amd import _lib, model
    from transgo_amd.engine import SelfPlayEngine
    sd = model.random_weights(9, 10, 32, 2, seed=11)

    def mk(load=True):
        e = SelfPlayEngine(8, num_simulation=16, net_blocks=2, net_filters=32)
        if load:
            model.load_into(e.ctx, sd, 9, 10, 32, 2)
        return e
    a = mk()
    a.reset(np.arange(8))
    for _ in range(2):
        _move(a)
    snap = a.snapshot()
    b = mk()
    b.restore(snap)
    for m in range(3):
        assert _move(a) == _move(b), m
    c = mk(load=False)
    c.restore(snap)                                                  # weights are not part of a snapshot: this succeeds ...
    with pytest.raises(_lib.TransgoError, match="no network weights loaded"):
        c.search()                                                   # ... and the next search says what is missing
    for e in (a, b, c):
        e.close()


def test_snapshot_inside_a_search_is_refused():
    from transgo_amd import _lib
    eng = _engine(4, 16)
    eng.reset(np.arange(4))
    eng.ctx.call("tg_sp_begin_move", 1, 0)
    act, rows = ctypes.c_int32(), ctypes.c_int32()
    eng.ctx.call("tg_sp_collect", ctypes.byref(act), ctypes.byref(rows))
    with pytest.raises(_lib.TransgoError, match=r"error -5: .*move boundary"):
        eng.snapshot()                                               # between tg_sp_collect and tg_sp_absorb
    eng._evaluate(rows.value)
    eng.ctx.call("tg_sp_absorb")
    with pytest.raises(_lib.TransgoError, match=r"error -5: .*move boundary"):
        eng.snapshot()                                               # between two waves of a search
    eng.close()


def test_restore_refuses_mismatch_and_damage():
    from transgo_amd import _lib, snapshot
    base = dict(pool_slots=20000)
    a = _engine(4, 16, **base)
    a.reset(np.arange(4))
    for _ in range(2):
        _move(a)
    snap = a.snapshot()
    for field, kw, G in (("n_games", base, 5), ("board_size", dict(base, board_size=19), 4), ("pool_chunks", dict(pool_slots=40000), 4),
                         ("record_games", dict(base, record_games=False), 4)):
        other = _engine(G, 16, **kw)
        with pytest.raises(_lib.TransgoError, match=field):
            other.restore(snap)
        other.close()
    hdr = snapshot.parse_header(snap)
    cut = snap[:len(snap) // 2].copy()
    magic = snap.copy(); magic[3] ^= 0x40
    chunk = snap.copy()
    snapshot.section(chunk, hdr, "chunk_ids", np.int32)[0] = hdr["pool_chunks"] + 5
    twice = snap.copy()
    ids = snapshot.section(twice, hdr, "chunk_ids", np.int32); ids[1] = ids[0]
    b = _engine(4, 16, **base)
    b.reset(np.arange(50, 54))
    _move(b)
    for bad, what in ((cut, "truncated"), (magic, "magic"), (chunk, "outside the pool"), (twice, "listed twice")):
        before = b.rng_streams().tobytes(), sorted(b.stats().items()), b.root_visits()[0].tobytes()
        with pytest.raises(_lib.TransgoError, match=what):
            b.restore(bad)
        assert before == (b.rng_streams().tobytes(), sorted(b.stats().items()), b.root_visits()[0].tobytes())      # nothing was overwritten
        b.reset(np.arange(60, 64))                                   # and the context is as usable as before
        vis = np.frombuffer(_move(b)[0], np.int32).reshape(4, 82)
        assert (vis.sum(1) >= 15).all()
    b.restore(snap)                                                  # the undamaged buffer is still taken
    assert _move(a) == _move(b)
    a.close(); b.close()


def test_replay_store_save_load(tmp_path):
    from transgo_amd.configure import Config
    from transgo_amd.replay_buffer import DeviceReplayMemory
    sp = _worker(G=4, sims=8, max_step=5)
    cfg = Config()
    mem = DeviceReplayMemory(cfg, capacity_positions=64)
    mem.SAVE_PIECE = 24                                              # several pieces, the last one short
    total, last = 0, None
    for _ in range(25):
        h = sp.advance()
        if h is not None:
            mem.append_harvest(h); total += h.n_positions; last = h
    assert total == 100                                              # 64 slots: the ring has wrapped
    path = str(tmp_path / "store.bin")
    mem.save(path)
    mem2 = DeviceReplayMemory(cfg, capacity_positions=64)
    mem2.load(path)
    assert mem.info() == mem2.info() and mem.info()["full"] and mem.info()["index"] == (100 % 64) * 8
    every = np.arange(mem.info()["entries"])
    for x, y in zip(mem.sample_entries(every), mem2.sample_entries(every)):
        assert x.tobytes() == y.tobytes()
    mem.append_harvest(last); mem2.append_harvest(last)              # one more append lands in the same slots in both
    assert mem.info() == mem2.info()
    for x, y in zip(mem.sample_entries(every), mem2.sample_entries(every)):
        assert x.tobytes() == y.tobytes()
    # tg_replay_import refuses more positions than the capacity, and a counter that does not match
    z = np.zeros(65 * 82, np.int32); p = z.ctypes.data_as(ctypes.c_void_p)
    assert mem2.ctx.lib.tg_replay_import(mem2.h, p, p, p, p, 65, 65) != 0
    assert mem2.ctx.lib.tg_replay_import(mem2.h, p, p, p, p, 10, 64) != 0
    assert mem.info() == mem2.info()
    small = DeviceReplayMemory(cfg, capacity_positions=32)
    with pytest.raises(ValueError):
        small.load(path)
    for m in (mem, mem2, small):
        m.close()
    sp.engine.close()


def test_grouped_checkpoint_has_one_section_per_group(tmp_path):
    from transgo_amd import model, snapshot
    from transgo_amd.configure import Config
    from transgo_amd.self_play import GroupedSelfPlay
    cfg = Config(num_simulation=12, max_step=4, num_features=32, num_blocks=2)
    sd = model.random_weights(9, 10, 32, 2, seed=3)

    def mk(groups=2):
        w = GroupedSelfPlay(cfg, 8, groups=groups)
        w.set_weights(sd)
        return w

    def run(w, n):
        out = []
        for _ in range(n):
            hs = w.advance()
            out.append(([None if h is None else h.to_host().buf.tobytes() for h in hs], sorted(w.stats().items()), w.games_finished,
                        [p.engine.rng_streams().tobytes() for p in w.parts]))
        return out
    a = mk()
    run(a, 3)
    path = str(tmp_path / "grouped.ckpt")
    a.save_checkpoint(path)
    parts = snapshot.read_checkpoint(path)
    assert len(parts) == 2 and [st["n_games"] for st, _ in parts] == [4, 4]
    after = run(a, 3)                                                # games end (4 plies) and restart inside these moves
    b = mk()
    bad = str(tmp_path / "bad.ckpt")                                 # group 1's section damaged: refused before group 0 is touched
    broken = parts[1][1].copy(); broken[2] ^= 0x20
    snapshot.write_checkpoint(bad, [parts[0], (parts[1][0], broken)])
    with pytest.raises(ValueError, match="magic"):
        b.load_checkpoint(bad)
    assert b.parts[0].moves_played == 0 and not b.parts[0]._started
    b.load_checkpoint(path)
    assert run(b, 3) == after
    c = mk(groups=1)
    with pytest.raises(ValueError, match="groups"):
        c.load_checkpoint(path)
    for w in (a, b, c):
        for p in w.parts:
            p.engine.close()
        w.close()
