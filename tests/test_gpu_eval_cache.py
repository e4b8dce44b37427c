"""The evaluation cache (tg_sp_eval_cache, csrc/eval_cache.hip) is exact: a cached engine and an uncached one with the same seeds
and weights play the same games down to the float bits of the tree, and the cache's counters account for every row.  Every
comparison is of bytes; no test depends on hit counts beyond the bounds the design guarantees (which of two keys wins a contested
way of the table may differ from run to run)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = dict(S=9, F=32, NB=2, G=48, R=4, sims=32, max_step=12, prec="f32", arch=None)
LARGE = dict(S=19, F=128, NB=1, G=8, R=4, sims=16, max_step=6, prec="f32", arch=None)      # obs_words = 113: two words per lane + tail
CASES = {
    "small": SMALL,
    "large": LARGE,
    "f16": dict(SMALL, F=128, prec="f16"),
    "f32x3": dict(SMALL, F=128, prec="f32x3"),
    "attention": dict(SMALL, F=128, G=16, arch="RARRRARRRRAR+P"),
}
TABLE = 65536


def _weights(c, seed):
    from transgo_amd import model
    if c["arch"]:
        return model.random_transgo_weights(c["S"], 10, c["F"], seed=seed)
    return model.random_weights(c["S"], 10, c["F"], c["NB"], seed=seed)


def _load(eng, c, sd):
    from transgo_amd import model
    model.load_into(eng.ctx, sd, c["S"], 10, c["F"], c["NB"], arch=model.transgo_arch() if c["arch"] else None)


def _engine(c, entries=0, sd=None, **kw):
    from transgo_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine(c["G"], board_size=c["S"], num_simulation=c["sims"], parallel_readouts=c["R"], max_step=c["max_step"],
                         net_blocks=c["NB"], net_filters=c["F"], net_precision=c["prec"], eval_cache_entries=entries, **kw)
    if sd is not None:
        _load(eng, c, sd)
    return eng


def _move(eng, log):
    """One move of every game; what the tree held before it, the move, and the records of the games it finished, as bytes."""
    eng.search()
    vis, st = eng.root_visits()
    rc = eng.root_children()
    acts, _ = eng.choose_moves(vis, st)
    eng.play(acts)
    h = eng.harvest()
    log.append(dict(visits=vis.tobytes(), actions=acts.tobytes(), records=b"" if h is None else np.asarray(h.buf).tobytes(),
                    **{"rc_" + k: v.tobytes() for k, v in rc.items()}))


def _play(eng, moves=None):
    log = []
    while (moves is None and not eng.finished.all()) or (moves is not None and len(log) < moves):
        _move(eng, log)
        assert len(log) <= 64
    return log


def _same(a, b, what=""):
    assert len(a) == len(b), (what, len(a), len(b))
    for m, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert x[k] == y[k], f"{what}: {k} differs at move {m}"


def _accounted(s):
    assert s["lookups"] == s["hits"] + s["batch_duplicates"] + s["evaluated"], s


@pytest.fixture(scope="module")
def uncached():
    """The uncached engine's game at each shape: played once, compared against by every test that needs it."""
    memo = {}

    def get(name):
        if name not in memo:
            c = CASES[name]
            eng = _engine(c, 0, _weights(c, 23))
            eng.reset(np.arange(c["G"]) + 100)
            log = _play(eng)
            st = eng.stats()
            assert eng.eval_cache_stats() == dict.fromkeys(eng.EVAL_CACHE_STATS, 0)
            eng.close()
            memo[name] = (log, st)
        return memo[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_transparency(name, uncached):
    c = CASES[name]
    want, want_stats = uncached(name)
    eng = _engine(c, TABLE, _weights(c, 23))
    eng.reset(np.arange(c["G"]) + 100)
    first = eng.eval_cache_stats()
    # every root is the empty board and nothing is in the table: one row through the network, the others follow it
    assert (first["lookups"], first["hits"], first["batch_duplicates"], first["evaluated"]) == (c["G"], 0, c["G"] - 1, 1), first
    assert first["inserts"] == 1 and first["dropped_inserts"] == 0
    got = _play(eng)
    _same(got, want, name)
    st, s = eng.stats(), eng.eval_cache_stats()
    assert (st["sims"], st["evals"]) == (want_stats["sims"], want_stats["evals"])
    _accounted(s)
    print(name, s)
    assert s["evaluated"] < s["lookups"]
    assert s["entries"] == TABLE and s["bytes"] >= TABLE * (16 + 4 * ((10 * c["S"] ** 2 + 31) // 32) + 4 * (c["S"] ** 2 + 2))
    eng.close()


def test_tiny_table(uncached):
    c = SMALL
    want, _ = uncached("small")
    eng = _engine(c, 16, _weights(c, 23))
    eng.reset(np.arange(c["G"]) + 100)
    _same(_play(eng), want, "16 entries")
    s = eng.eval_cache_stats()
    _accounted(s)
    assert s["entries"] == 16
    # no generation change in this run: more inserts than entries means live entries were overwritten
    assert s["dropped_inserts"] > 0 or s["inserts"] > s["entries"], s
    eng.close()


def _unique_rows(eng):
    obs = eng.root_info()[4]
    return len(np.unique(obs.reshape(len(obs), -1), axis=0))


def test_second_pass_hits():
    c = SMALL
    G = c["G"]
    eng = _engine(c, TABLE, _weights(c, 23))
    seeds = np.arange(G) + 100
    eng.reset(seeds)
    a = eng.eval_cache_stats()
    eng.reset(seeds)                                      # the same roots again: one unique position, inserted without a race
    b = eng.eval_cache_stats()
    assert b["hits"] - a["hits"] == G and b["evaluated"] == a["evaluated"] == 1
    # a root batch of different positions: a few moves in, the same states evaluated twice as fresh roots
    _play(eng, 3)
    states = eng.root_states()
    eng.clear_eval_cache()
    s0 = eng.eval_cache_stats()
    eng.reset_from(states)
    unique = _unique_rows(eng)
    s1 = eng.eval_cache_stats()
    assert s1["hits"] == s0["hits"] and s1["evaluated"] - s0["evaluated"] >= unique      # cleared: every position went through
    dropped = s1["dropped_inserts"] - s0["dropped_inserts"]
    eng.reset_from(states)
    s2 = eng.eval_cache_stats()
    assert s2["lookups"] - s1["lookups"] == G
    assert s2["hits"] - s1["hits"] >= unique - dropped
    if dropped == 0:
        assert s2["evaluated"] == s1["evaluated"] and s2["hits"] - s1["hits"] == G
    _accounted(s2)
    eng.close()


def _first_batch_then_search(eng):
    """A move's search with its first leaf batch evaluated by hand, so that the cache counters can be read around it."""
    eng.ctx.call("tg_sp_begin_move", 1, 0)
    act, rows = ctypes.c_int32(), ctypes.c_int32()
    eng.ctx.call("tg_sp_collect", ctypes.byref(act), ctypes.byref(rows))
    before = eng.eval_cache_stats()
    eng.ctx.call("tg_sp_eval")
    after = eng.eval_cache_stats()
    eng.ctx.call("tg_sp_absorb")
    w = ctypes.c_int32()
    eng.ctx.call("tg_sp_search", ctypes.byref(w))
    return rows.value, {k: after[k] - before[k] for k in ("lookups", "hits")}


def _finish_move(eng, log):
    vis, st = eng.root_visits()
    rc = eng.root_children()
    acts, _ = eng.choose_moves(vis, st)
    eng.play(acts)
    log.append(dict(visits=vis.tobytes(), actions=acts.tobytes(), **{"rc_" + k: v.tobytes() for k, v in rc.items()}))


@pytest.mark.parametrize("how", ["set_weights", "async"])
def test_invalidation_by_weights(how):
    import torch
    from transgo_amd import model
    c = SMALL
    sd1, sd2 = _weights(c, 23), _weights(c, 24)
    logs = []
    for entries in (TABLE, 0):
        eng = _engine(c, entries, sd1)
        eng.reset(np.arange(c["G"]) + 100)
        log = _play(eng, 2)
        if how == "set_weights":
            _load(eng, c, sd2)
        else:
            blob = model.pack_weights(sd2, c["S"], 10, c["F"], arch=model.tower_arch(c["NB"]))
            eng.ctx.call("tg_net_load_async", model.tower_arch(c["NB"]).code.encode(), blob.ctypes.data_as(ctypes.c_void_p), blob.size)
            torch.cuda.synchronize(eng.device)            # the upload is complete: the coming tg_sp_begin_move adopts it
        rows, d = _first_batch_then_search(eng)
        if entries:
            assert rows > 0 and d == dict(lookups=rows, hits=0), (how, rows, d)
        _finish_move(eng, log)
        log += _play(eng, 2)
        if entries:
            _accounted(eng.eval_cache_stats())
        logs.append(log)
        eng.close()
    _same(logs[0], logs[1], how)


def test_invalidation_by_symmetry():
    c = SMALL
    sd = _weights(c, 23)
    logs = []
    for entries in (TABLE, 0):
        eng = _engine(c, entries, sd)
        eng.reset(np.arange(c["G"]) + 100)
        log = _play(eng, 2)
        for mode in ("position", "none"):                 # back to "none": the entries of the first two moves stay dead
            eng.set_symmetry(mode, 7)
            rows, d = _first_batch_then_search(eng)
            if entries:
                assert rows > 0 and d == dict(lookups=rows, hits=0), (mode, rows, d)
            _finish_move(eng, log)
            log += _play(eng, 1)
        logs.append(log)
        eng.close()
    _same(logs[0], logs[1], "symmetry")


def test_off_is_off(uncached):
    from transgo_amd._lib import TransgoError
    c = SMALL
    want, want_stats = uncached("small")
    zero = None
    for make_first in (False, True):
        eng = _engine(c, 0, _weights(c, 23))
        zero = dict.fromkeys(eng.EVAL_CACHE_STATS, 0)
        if make_first:
            eng.set_eval_cache(TABLE)
            assert eng.eval_cache_stats()["entries"] == TABLE
            eng.set_eval_cache(0)
        eng.reset(np.arange(c["G"]) + 100)
        _same(_play(eng), want, f"off (created first: {make_first})")
        assert eng.eval_cache_stats() == zero
        st = eng.stats()
        assert (st["sims"], st["evals"]) == (want_stats["sims"], want_stats["evals"])
        eng.close()
    eng = _engine(c, 0, _weights(c, 23))
    eng.ctx.call("tg_sp_reset", (np.arange(c["G"], dtype=np.uint32) + 100).ctypes.data_as(ctypes.c_void_p), None)
    with pytest.raises(TransgoError, match="pending"):    # refused while a batch is pending
        eng.set_eval_cache(TABLE)
    eng.close()


def test_host_evaluator_bypasses_the_cache():
    from transgo_amd import model
    c = SMALL
    hn = model.HipNetwork(9, 10, c["F"], c["NB"], rows_cap=c["G"] * c["R"])
    hn.set_weights(_weights(c, 23))
    eng = _engine(c, TABLE, evaluator=lambda o: hn.main_prediction(o)[:2])
    eng.reset(np.arange(c["G"]) + 100)
    _play(eng, 2)
    s = eng.eval_cache_stats()
    assert s["entries"] == TABLE and all(s[k] == 0 for k in s if k not in ("entries", "bytes")), s
    eng.close(); hn.ctx.close()
