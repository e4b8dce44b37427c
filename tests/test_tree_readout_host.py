"""Host side of the tree read-out: GTP vertices, the analysis table, and the ctypes signatures of the two new entry points."""
import os
import re

import numpy as np
import pytest

from transgo_amd import _lib, analysis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vertex_is_gtp_style_at_both_sizes():
    v = analysis.vertex
    # row index 0 of the action grid is the top row = row S; columns skip the letter I
    assert (v(0, 9), v(8, 9), v(72, 9), v(80, 9)) == ("A9", "J9", "A1", "J1")
    assert (v(7, 9), v(8, 9)) == ("H9", "J9")
    assert v(81, 9) == "pass"
    assert (v(0, 19), v(18, 19), v(342, 19), v(360, 19)) == ("A19", "T19", "A1", "T1")
    assert (v(7, 19), v(8, 19), v(19 + 7, 19), v(19 + 8, 19)) == ("H19", "J19", "H18", "J18")
    assert v(361, 19) == "pass"
    assert all("I" not in v(a, 19) for a in range(361))
    for bad in (-1, 82):
        with pytest.raises(ValueError):
            v(bad, 9)


def _record():
    A = 82
    visits = np.zeros(A, np.int32); prior = np.zeros(A, np.float64); q = np.full(A, np.nan, np.float32)
    legal = np.zeros(A, bool)
    # action: (visits, q, prior) -- 40 and 3 tie on visits, 70 was never visited
    for a, (n, qq, p) in {40: (7, 0.25, 0.125), 3: (7, -0.5, 0.25), 81: (20, 0.0625, 0.5), 70: (0, np.nan, 0.0625), 10: (2, -1.0, 0.03125),
                          11: (1, 0.5, 0.015625)}.items():
        visits[a], q[a], prior[a], legal[a] = n, qq, p, True
    return dict(visits=visits, prior=prior, q=q, legal=legal, status=0, root_value=-0.125, pv=[81, 40, 3], pv_visits=[20, 9, 4])


def test_format_analysis_orders_cuts_and_prints_nan():
    txt = analysis.format_analysis(_record(), 9, top=6)
    lines = txt.split("\n")
    assert "root value -0.125" in lines[0] and "visits 37" in lines[0]
    rows = [l.split() for l in lines[2:]]
    # descending visits, the 7-7 tie by ascending action (D9 = 3 before E5 = 40), the unvisited move last
    assert [r[0] for r in rows] == ["pass", "D9", "E5", "B8", "C8", "H2"]
    assert [int(r[1]) for r in rows] == [20, 7, 7, 2, 1, 0]
    assert [r[2] for r in rows] == ["+0.062", "-0.500", "+0.250", "-1.000", "+0.500", "-"]      # NaN prints as '-'
    assert [float(r[3]) for r in rows] == [0.5, 0.25, 0.125, 0.0312, 0.0156, 0.0625]
    assert rows[0][4:] == ["pass", "E5", "D9"]                         # the principal variation on the move that heads it
    assert rows[1][4:] == ["D9"] and rows[5][4:] == ["H2"]
    assert "nan" not in txt.lower()
    # the cut
    assert len(analysis.format_analysis(_record(), 9).split("\n")) == 2 + 5
    top2 = analysis.format_analysis(_record(), 9, top=2).split("\n")
    assert len(top2) == 4 and top2[2].split()[0] == "pass" and top2[3].split()[0] == "D9"
    assert len(analysis.format_analysis(_record(), 9, top=0).split("\n")) == 2
    # a record of a slot that was not searched
    r = _record(); r["root_value"] = float("nan"); r["pv"] = []; r["visits"][:] = 0; r["q"][:] = np.nan
    txt = analysis.format_analysis(r, 9, top=3)
    assert "root value -" in txt and "nan" not in txt.lower()


def test_new_symbols_are_bound_with_the_argument_counts_the_header_declares():
    src = open(os.path.join(ROOT, "include", "transgo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("tg_sp_root_children", "tg_sp_pv"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name + " is not declared in the header"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n_args, (name, len(args), n_args)
    assert len(_lib.SIGNATURES["tg_sp_root_children"][1]) == 12 and len(_lib.SIGNATURES["tg_sp_pv"][1]) == 6

