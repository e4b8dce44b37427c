"""The evaluation cache's public surface without a GPU: the C ABI is declared and bound, the Python options exist and default to
off, and asking for statistics without an engine context is the project's own error."""
import ctypes
import inspect
import os
import re

import pytest

from transgo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARGS = {"tg_sp_eval_cache": 2, "tg_sp_eval_cache_clear": 1, "tg_sp_eval_cache_stats": 9}


def _declarations():
    src = open(os.path.join(ROOT, "include", "transgo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(tg_sp_eval_cache\w*)\s*\(([^)]*)\)\s*;", src)}


def test_symbols_declared_bound_and_exported():
    decl = _declarations()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in ARGS.items():
        assert name in decl, name
        assert len(decl[name].split(",")) == n, (name, decl[name])
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n, name
        assert hasattr(lib, name), name
    assert _lib.SIGNATURES["tg_sp_eval_cache"][1][1] is ctypes.c_uint64
    assert all(a == ctypes.POINTER(ctypes.c_uint64) for a in _lib.SIGNATURES["tg_sp_eval_cache_stats"][1][1:])


def test_python_options_default_to_off():
    from transgo_amd import analysis
    from transgo_amd.configure import Config
    from transgo_amd.engine import SelfPlayEngine
    from transgo_amd.self_play import BatchedSelfPlay
    assert Config().eval_cache_entries == 0
    assert inspect.signature(SelfPlayEngine.__init__).parameters["eval_cache_entries"].default == 0
    assert inspect.signature(BatchedSelfPlay.__init__).parameters["eval_cache_entries"].default is None      # None = the Config's
    assert inspect.signature(analysis.analyse).parameters["eval_cache_entries"].default is None              # None = leave the engine alone
    for m in ("set_eval_cache", "clear_eval_cache", "eval_cache_stats"):
        assert callable(getattr(SelfPlayEngine, m)), m
    assert SelfPlayEngine.EVAL_CACHE_STATS == ("lookups", "hits", "batch_duplicates", "evaluated", "inserts", "dropped_inserts",
                                               "entries", "bytes")


def test_stats_without_an_engine_context_is_a_transgo_error():
    from transgo_amd.engine import SelfPlayEngine, eval_cache_stats
    eng = SelfPlayEngine.__new__(SelfPlayEngine)          # an engine whose context was never created (no GPU here)
    with pytest.raises(_lib.TransgoError):
        eng.eval_cache_stats()
    with pytest.raises(_lib.TransgoError):
        eval_cache_stats(object())
