"""Playout cap randomization, the host side: the full / fast draw in C (tg_host_cap_draw) and in NumPy (transgo_amd.playout_cap),
the schedule built from it, and the Config refusals.  No GPU."""
import ctypes

import numpy as np
import pytest

from transgo_amd import _lib, playout_cap
from transgo_amd.configure import Config

PINNED = [((0, 0, 0), 0xa706dd), ((0, 1, 0), 0x08b4fd), ((0, 2, 0), 0xd7cc96), ((7, 5, 3), 0x5d2bbb)]


def _c_draw():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.tg_host_cap_draw.restype = ctypes.c_uint32
    lib.tg_host_cap_draw.argtypes = [ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint32]
    return lib.tg_host_cap_draw


def test_pinned_draws_in_c_and_in_python():
    c = _c_draw()
    for (seed, ply, cap), want in PINNED:
        assert c(seed, ply, cap) == want, (seed, ply, cap, hex(c(seed, ply, cap)))
        assert int(playout_cap.draw(seed, ply, cap)) == want, (seed, ply, cap)
        assert int(playout_cap.draw(np.array([seed], np.uint32), np.array([ply], np.int32), cap)[0]) == want


def test_c_and_python_agree_on_random_triples():
    c = _c_draw()
    rs = np.random.RandomState(11)
    seeds = rs.randint(0, 2 ** 32, 10000, dtype=np.uint64).astype(np.uint32)
    plies = rs.randint(0, 1000, 10000).astype(np.int32)
    caps = rs.randint(0, 2 ** 32, 10000, dtype=np.uint64).astype(np.uint32)
    caps[:5000] = caps[0]                                             # half of them through the vectorised form with one cap seed
    vec = playout_cap.draw(seeds[:5000], plies[:5000], int(caps[0]))
    assert vec.dtype == np.uint32 and vec.max() < 2 ** 24
    for i in range(10000):
        want = c(int(seeds[i]), int(plies[i]), int(caps[i]))
        got = int(vec[i]) if i < 5000 else int(playout_cap.draw(seeds[i], plies[i], int(caps[i])))
        assert got == want, (i, seeds[i], plies[i], caps[i])


@pytest.mark.parametrize("p,band", [(0.25, 0.0055), (0.5, 0.0063)])
def test_share_of_full_moves(p, band):
    """Seeds 0..999 x plies 0..99: 100 000 draws, sigma = sqrt(p (1 - p) / 1e5); the band is 4 sigma."""
    seeds = np.repeat(np.arange(1000, dtype=np.uint32), 100)
    plies = np.tile(np.arange(100, dtype=np.int32), 1000)
    for cap_seed in (0, 1, 12345):
        share = playout_cap.schedule(seeds, plies, p, cap_seed).mean()
        print(f"p_full {p} cap seed {cap_seed}: share of full moves {share:.4f}")
        assert abs(share - p) <= band, (p, cap_seed, share)


def test_schedule_with_p_one_is_all_true_and_shaped_like_the_games():
    seeds = np.arange(50, dtype=np.uint32)
    for cap_seed in (0, 9):
        full = playout_cap.schedule(seeds, np.arange(50), 1.0, cap_seed)
        assert full.dtype == bool and full.shape == (50,) and full.all()
    a = playout_cap.schedule(seeds, np.full(50, 3), 0.5, 4)
    assert a.shape == (50,) and 0 < a.sum() < 50
    assert np.array_equal(a, [playout_cap.schedule(int(s), 3, 0.5, 4) for s in seeds])
    assert not np.array_equal(a, playout_cap.schedule(seeds, np.full(50, 3), 0.5, 5))     # the cap seed matters


def test_a_harvest_without_positions_is_legal_on_the_host():
    """A game whose moves were all fast contributes no position: records.Harvest, its read-outs, game_targets and the
    single-process gather take a batch of n games and zero positions, and a batch where only some games are empty."""
    from transgo_amd import distributed, records
    from transgo_amd.self_play import GameRecord, game_targets
    S, C, P = 9, 10, 81
    empty = GameRecord(5); empty.winner, empty.territory, empty.score = 1, np.ones(P, np.float32), 2.5
    full = GameRecord(6); full.winner, full.territory, full.score = 2, -np.ones(P, np.float32), -1.5
    rs = np.random.RandomState(0)
    for _ in range(2):
        full.observations.append((rs.rand(C, S, S) < 0.3).astype(np.float32))
        v = rs.randint(0, 9, P + 1).astype(np.int32); v[0] = 7
        full.visits.append(v); full.players.append(1 + len(full.players) % 2)
    h0 = records.from_records([empty, empty], S, C)
    assert (h0.n_games, h0.n_positions) == (2, 0) and h0.nbytes == records.header_bytes(S, C, 2)
    assert h0.targets() == [] and h0.observations().shape == (0, C, S, S) and h0.pis().shape == (0, P + 1)
    r0 = h0.records()
    assert len(r0) == 2 and r0[0].players == [] and r0[0].winner == 1 and r0[0].seed == 5
    assert game_targets([], [], [], 1, np.ones(P), S) == []
    assert distributed.gather_harvest(h0, S, C, live=3) == ([h0], 3)
    h1 = records.from_records([empty, full, empty], S, C)
    assert list(h1.view("n_moves")) == [0, 2, 0] and h1.n_positions == 2 and len(h1.targets()) == 16
    r1 = h1.records()
    assert [len(r.players) for r in r1] == [0, 2, 0] and np.array_equal(r1[1].visits[1], full.visits[1])
    # same bytes after a trip through the records and back
    assert np.array_equal(records.from_records(r1, S, C).buf, h1.buf)


def test_config_defaults_and_refusals():
    c = Config()
    assert (c.playout_cap_p_full, c.playout_cap_fast, c.playout_cap_seed, c.playout_cap_fast_noise) == (1.0, 0, 0, False)
    assert not playout_cap.enabled(c)
    ok = Config(playout_cap_p_full=0.25, playout_cap_fast=64)
    assert playout_cap.enabled(ok)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="playout_cap_p_full"):
            Config(playout_cap_p_full=bad, playout_cap_fast=32)
    for fast in (0, -3):
        with pytest.raises(ValueError, match="playout_cap_fast"):
            Config(playout_cap_p_full=0.5, playout_cap_fast=fast)
    # attributes set after construction are checked where they are used
    late = Config()
    late.playout_cap_p_full = 0.5
    with pytest.raises(ValueError, match="playout_cap_fast"):
        playout_cap.check_config(late)
