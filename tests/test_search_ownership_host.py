"""Search ownership on the CPU: the restatement of tests/search_ownership_ref.py against a brute-force recomputation
from a trace of the same search, the conditions the GPU cases (tests/test_gpu_search_ownership.py) rest on, the binding, the config
attribute and the formatter's shim.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

from tests import search_ownership_ref as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@functools.lru_cache(maxsize=None)
def _case(case, own="tenths", rule="plain", invert=False):
    kw = {"forced": dict(forced_k=2.0), "gumbel": dict(gumbel_m=8)}.get(rule, {})
    return so.play_case(case, own=own, rule=rule, invert_sign=invert, trace=True, **kw)


def _brute_force(trace, own_fn, S, komi=7.5):
    """Per searched move of a trace: (mean, n, score_lead) recomputed from the absorbed leaves' states alone -- every state
    re-encoded, its ownership recomputed, the sign from the state's own side to move, summed in trace order in float32 scalars."""
    from oracle.go_oracle import OracleGoEnv
    env = OracleGoEnv(board_size=S)
    out, acc, n = [], None, 0
    for kind, payload in trace:
        if kind == "move":
            acc, n = [F32(0)] * (S * S), 0
        elif kind == "absorb":
            own = own_fn(np.array([env.encode(payload)], dtype="float32"))[0]
            sgn = F32(1) if env.getPlayer(payload) == 1 else F32(-1)
            acc = [F32(a + sgn * o) for a, o in zip(acc, own)]
            n += 1
        elif kind == "played":
            mean = np.array([a / F32(n) for a in acc], F32) if n else np.zeros(S * S, F32)
            s = mean[0]
            for p in range(1, S * S):
                s = F32(s + mean[p])
            out.append((mean, n, F32(s - F32(komi))))
    return out


@pytest.mark.parametrize("own", ["tenths", "exact"])
def test_restatement_equals_the_brute_force_sum_over_the_trace(own):
    games = _case("flat9", own)
    for mv, o, tr in games[:3]:
        want = _brute_force(tr, so.OWN_BY_NAME[own], 9)
        assert len(want) == len(mv)
        for m, (mean, n, lead) in zip(mv, want):
            assert m["n"] == n
            assert np.array_equal(m["mean"], mean) and m["mean"].dtype == np.float32
            assert m["score_lead"] == lead


def test_exact_stand_in_sums_without_rounding():
    """own_exact's partial sums are exact in float32: the float32 accumulator equals the float64 sum of the same rows."""
    from oracle.go_oracle import OracleGoEnv
    env = OracleGoEnv(board_size=9)
    mv, o, tr = _case("flat9", "exact")[0]
    acc64, k = np.zeros(81), 0
    for kind, payload in tr:
        if kind == "move":
            acc64[:] = 0
        elif kind == "absorb":
            own = so.own_exact(np.array([env.encode(payload)], dtype="float32"))[0]
            acc64 += (1 if env.getPlayer(payload) == 1 else -1) * own.astype(np.float64)
        elif kind == "played":
            n = mv[k]["n"]
            if n:
                assert np.array_equal(mv[k]["mean"], (acc64.astype(F32) / F32(n))) and np.array_equal(acc64.astype(F32).astype(np.float64), acc64)
            k += 1
    assert np.abs(so.own_exact(np.array([env.encode(env.reset()[0])], dtype="float32"))).max() <= 1
    assert np.abs(so.own_tenths(np.array([env.encode(env.reset()[0])], dtype="float32"))).max() <= 1


def test_the_9x9_case_holds_what_the_gpu_test_needs():
    """flat9: dropped duplicate leaves, terminal simulations, roots of both colours, moves that begin on a reused sub-tree, and a
    game whose search completes only terminal simulations (n = 0) -- asserted here so that a later edit of the case cannot hollow
    the GPU comparison out."""
    games = _case("flat9")
    moves = [m for mv, _, _ in games for m in mv]
    assert len(games) == 6 and all(len(mv) == 5 for mv, _, _ in games)
    assert sum(m["dropped"] for m in moves) >= 1
    assert sum(m["terminal"] for m in moves) >= 1
    assert {m["root_player"] for m in moves} == {1, 2}
    assert any(m["root_n0"] > 0 for m in moves)
    zero = [m for m in moves if m["n"] == 0]
    assert zero and all(not m["mean"].any() and m["score_lead"] == F32(-7.5) and m["terminal"] > 0 for m in zero)
    # a dropped path and a terminal simulation add nothing: n counts the absorbed paths only
    for mv, o, tr in games:
        per_move, k = [0] * len(mv), 0
        for kind, _ in tr:
            if kind == "absorb":
                per_move[k] += 1
            elif kind == "played":
                k += 1
        assert per_move == [m["n"] for m in mv]
    # the means are not trivially symmetric: both signs occur, and a search of Black's and one of White's are both non-zero
    assert any(m["mean"].any() for m in moves if m["root_player"] == 1) and any(m["mean"].any() for m in moves if m["root_player"] == 2)


def test_the_mode_does_not_steer_the_restatement():
    """The mixin only listens: visits, moves and stream positions are those of the plain oracle search."""
    from oracle import evaluators
    from oracle.go_oracle import OracleGoEnv
    from oracle.wp_mcts import OracleSearch
    name, S, G, sims, moves, max_step, _ = so.CASES["flat9"]
    mv, _, _ = _case("flat9")[1]
    rng = np.random.RandomState(int(so.case_seeds("flat9")[1]))
    o = OracleSearch(OracleGoEnv(board_size=S, max_step=max_step), evaluators.BY_NAME[name], rng, num_simulation=sims, parallel_readouts=so.R,
                     board_size=S)
    for m in mv:
        a, pi, _, _ = o.search_move(True)
        raw = np.array([o.root.kids[i].n if i in o.root.kids else 0 for i in range(o.A)])
        assert a == m["action"] and np.array_equal(raw, m["raw"]) and np.array_equal(pi, m["pi"])
        o.advance(a)
        assert int(rng.get_state()[2]) == m["pos"]


def test_inverted_sign_is_a_different_answer():
    """The negative control of the GPU file: the same search with contributions from the leaf mover's own side differs."""
    a, b = _case("flat9"), _case("flat9", invert=True)
    diff = 0
    for (mv, _, _), (mw, _, _) in zip(a, b):
        for m, w in zip(mv, mw):
            assert np.array_equal(m["raw"], w["raw"]) and m["n"] == w["n"]
            diff += not np.array_equal(m["mean"], w["mean"])
    assert diff >= 6


@pytest.mark.parametrize("rule", ["forced", "gumbel"])
def test_rule_cases_absorb_and_drop(rule):
    """The forced-playout and Gumbel restatements run with the mixin and their case still holds dropped and terminal paths."""
    games = _case("rule9", "tenths", rule)
    moves = [m for mv, _, _ in games for m in mv]
    assert sum(m["n"] for m in moves) > 0 and sum(m["terminal"] for m in moves) >= 1 and sum(m["dropped"] for m in moves) >= 1
    plain = [m for mv, _, _ in _case("rule9") for m in mv]
    assert any(not np.array_equal(m["raw"], p["raw"]) for m, p in zip(moves, plain))       # the rule really changes the search


def _declarations():
    src = open(os.path.join(ROOT, "include", "transgo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(tg_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_symbols_in_header_and_binding():
    from transgo_amd import _lib
    decl = _declarations()
    for name, nargs in (("tg_sp_search_ownership", 2), ("tg_sp_search_ownership_get", 2), ("tg_sp_root_ownership", 4),
                        ("tg_sp_set_eval_own", 5)):
        assert name in decl, name
        assert len(decl[name].split(",")) == nargs, (name, decl[name])
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in ("tg_sp_search_ownership", "tg_sp_search_ownership_get", "tg_sp_root_ownership", "tg_sp_set_eval_own"))


def test_config_attribute():
    from transgo_amd.configure import Config
    assert Config().search_ownership is False
    assert Config(search_ownership=True).search_ownership is True
    with pytest.raises(ValueError, match="eval_cache_entries"):
        Config(search_ownership=True, eval_cache_entries=1024)


def test_analyse_refuses_ownership_with_a_cache_before_it_touches_the_engine():
    from transgo_amd import analysis
    with pytest.raises(ValueError, match="evaluation cache"):
        analysis.analyse(None, np.zeros((1, 48), np.uint8), ownership=True, eval_cache_entries=1024)


def test_format_ownership_takes_both_kinds_of_record():
    from transgo_amd import analysis
    mean = ((np.arange(81) % 17 - 8) / 8).astype(np.float32).reshape(9, 9)         # eighths: 100 * v is the same in float32 and float64
    rec = dict(ownership=mean, ownership_evals=37, score_lead=-7.5)
    txt = analysis.format_ownership(rec, 9)
    lines = txt.split("\n")
    assert "37 evaluations" in lines[0] and "-7.50" in lines[0] and len(lines) == 11
    assert lines[2].split()[1] == "-100" and lines[2].split()[-1] == "+0" and lines[-1].split()[-1] == "+50"
    play = dict(territory=mean.astype(np.float64).reshape(-1), score=1.5, black_win=0.5, playouts=8)
    assert analysis.format_ownership(play, 9).split("\n")[2:] == lines[2:]
    full = dict(visits=np.zeros(82, np.int32), prior=np.zeros(82), q=np.full(82, np.nan, np.float32), legal=np.zeros(82, bool), **rec)
    assert analysis.format_analysis(full, 9).endswith(txt)
