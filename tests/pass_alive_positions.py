"""Hand-built positions for the pass-alive tests, with the expected status written out.  TEST INFRASTRUCTURE ONLY.

Diagrams: X black, O white, . empty.  Expected: B +2 (pass-alive black stone), b +1 (black territory), W -2, w -1, . 0.
Rows that are left out are empty (expected: 0)."""
import numpy as np

_ST = {"B": 2, "b": 1, "W": -2, "w": -1, ".": 0}


def _grid(rows, S, table):
    g = np.zeros((S, S), np.int8)
    for y, row in enumerate(rows):
        cells = row.split()
        assert len(cells) == S, (row, S)
        for x, c in enumerate(cells):
            g[y, x] = table[c]
    return g


def position(rows, expected, S=9):
    """-> (black bool[P], white bool[P], expected status int8[P])"""
    g = _grid(rows, S, {"X": 1, "O": 2, ".": 0})
    e = _grid(expected, S, _ST)
    return (g == 1).reshape(-1), (g == 2).reshape(-1), e.reshape(-1)


E9 = ". . . . . . . . ."

HAND_9 = {
    # one black chain in the corner with the one-point eyes (0,0) and (0,2)
    "corner_two_eyes": position(
        [". X . X . . . . .",
         "X X X X . . . . ."],
        ["b B b B . . . . .",
         "B B B B . . . . ."]),
    # the same without the stone at (1,1): three chains, the eye at (0,0) belongs to two single stones and nothing lives
    "corner_false_eye": position(
        [". X . X . . . . .",
         "X . X X . . . . ."],
        [E9]),
    # Benson's classic: two chains, both next to both one-point eyes (0,1) and (1,2)
    "two_chains_share_two_eyes": position(
        ["X . X X . . . . .",
         "X X . X . . . . .",
         ". X X . . . . . ."],
        ["B b B B . . . . .",
         "B B b B . . . . .",
         ". B B . . . . . ."]),
    # the right-hand chain has the eye (0,4) and the two-point region (0,0)-(0,1), whose corner point is no liberty of it: that
    # region is vital to the left-hand chain only, every chain has one vital region, nothing lives
    "second_eye_not_vital": position(
        [". . X X . X . . .",
         "X X . X X X . . ."],
        [E9]),
    # a live wall (eyes (0,3), (0,5)) around the corner region (0,0),(0,1),(1,0),(1,1): only (0,0) has no black neighbour, so the
    # region is black territory, the dead white stone at (1,1) included
    "territory_one_interior": position(
        [". . X . X . X . .",
         ". O X X X X X . .",
         "X X X . . . . . ."],
        ["b b B b B b B . .",
         "b b B B B B B . .",
         "B B B . . . . . ."]),
    # the same wall one column further out: (0,0) and (0,1) have no black neighbour, the region stays unassigned
    "territory_two_interior": position(
        [". . . X . X . X .",
         ". O . X X X X X .",
         "X X X X . . . . ."],
        [". . . B b B b B .",
         ". . . B B B B B .",
         "B B B B . . . . ."]),
    # every point is a stone of a two-eyed chain or one of its eyes
    "settled": position(
        [". X X X O O O O .",
         "X X X X O O O O O",
         ". X X X O O O O ."] + ["X X X X O O O O O"] * 6,
        ["b B B B W W W W w",
         "B B B B W W W W W",
         "b B B B W W W W w"] + ["B B B B W W W W W"] * 6),
    "empty": position([E9] * 9, [E9] * 9),
}


def _blocks_19():
    """Free-standing two-eyed 3x5 blocks whose middle rows straddle the lane-word boundaries 63|64 ... 319|320 of a 19x19 board, and a
    two-eyed group on row 18."""
    S = 19
    col = np.zeros((S, S), np.int8)
    exp = np.zeros((S, S), np.int8)
    for (r, c, colour) in ((2, 5, 1), (5, 12, 2), (9, 0, 1), (12, 7, 2), (15, 14, 1)):
        s = 2 if colour == 1 else -2
        col[r:r + 3, c:c + 5] = colour
        exp[r:r + 3, c:c + 5] = s
        for e in (c + 1, c + 3):
            col[r + 1, e] = 0
            exp[r + 1, e] = s // 2
    for p in (63, 127, 191, 255, 319):                                 # the first eye of each block is the last point of a lane word
        assert col.reshape(-1)[p] == 0 and exp.reshape(-1)[p] != 0 and col.reshape(-1)[p + 1] != 0
    col[17, 0:5] = 2; col[18, 0:5] = 2; exp[17, 0:5] = -2; exp[18, 0:5] = -2
    for e in (1, 3):
        col[18, e] = 0; exp[18, e] = -1
    return (col == 1).reshape(-1), (col == 2).reshape(-1), exp.reshape(-1)


def _settled_19():
    S = 19
    col = np.zeros((S, S), np.int8)
    col[:, :9] = 1; col[:, 9:] = 2
    exp = np.where(col == 1, 2, -2).astype(np.int8)
    for (y, x) in ((0, 0), (2, 0), (16, 0), (18, 0)):
        col[y, x] = 0; exp[y, x] = 1
    for (y, x) in ((0, 18), (2, 18), (18, 18)):
        col[y, x] = 0; exp[y, x] = -1
    return (col == 1).reshape(-1), (col == 2).reshape(-1), exp.reshape(-1)


def _corner_19(name):
    b, w, e = HAND_9[name]
    S = 19
    out = []
    for a in (b, w, e):
        g = np.zeros((S, S), a.dtype)
        g[:3, :9] = a.reshape(9, 9)[:3]
        out.append(g.reshape(-1))
    return tuple(out)


HAND_19 = {
    "blocks_on_word_boundaries": _blocks_19(),
    "settled": _settled_19(),
    "territory_one_interior": _corner_19("territory_one_interior"),
    "territory_two_interior": _corner_19("territory_two_interior"),
    "two_chains_share_two_eyes": _corner_19("two_chains_share_two_eyes"),
    "empty": (np.zeros(361, bool), np.zeros(361, bool), np.zeros(361, np.int8)),
}


def states_of(black, white, ssz, board_size, next_player=1):
    """State blobs uint8[n][ssz] for stone sets bool[n][P]: the two bitboards, step_count 1, no ko, `next_player` to move."""
    black = np.atleast_2d(np.asarray(black, bool)); white = np.atleast_2d(np.asarray(white, bool))
    n, P = black.shape
    nw = (P + 63) // 64
    st = np.zeros((n, ssz), np.uint8)
    for i, stones in enumerate((black, white)):
        bits = np.zeros((n, nw * 64), np.uint8)
        bits[:, :P] = stones
        st[:, i * nw * 8:(i + 1) * nw * 8] = np.packbits(bits, axis=1, bitorder="little")
    tail = np.zeros(n, np.dtype([("lm1", "<i2"), ("lm2", "<i2"), ("ko", "<i2"), ("ko_age", "<i2"), ("step", "<u2"), ("ko_color", "u1"),
                                 ("player", "u1"), ("term", "u1"), ("pad", "u1", 3)]))
    tail["lm1"] = tail["lm2"] = tail["ko"] = -3
    tail["step"] = 1
    tail["player"] = next_player
    st[:, 2 * nw * 8:2 * nw * 8 + 16] = tail.view(np.uint8).reshape(n, 16)
    return st


def near_settled_19(dames):
    """A 19x19 position one filling move per point of `dames` away from settled: Black holds columns 0-8 with the eyes (0,0), (2,0)
    and a corner region (17,0),(18,0),(18,1) around a dead white stone at (17,1) (one interior point: black territory, which
    Tromp-Taylor scores otherwise); White holds columns 9-18 with three eyes; `dames` are empty points on the border between them,
    given as (row, column) in columns 8 or 9.  -> (black bool[P], white bool[P])."""
    S = 19
    col = np.zeros((S, S), np.int8)
    col[:, :9] = 1; col[:, 9:] = 2
    for (y, x) in ((0, 0), (2, 0), (17, 0), (18, 0), (18, 1), (0, 18), (2, 18), (18, 18)) + tuple(dames):
        col[y, x] = 0
    col[17, 1] = 2
    return (col == 1).reshape(-1), (col == 2).reshape(-1)


def move_sequence(black, white, S):
    """A legal sequence of plies from the empty board to the position: the stones of each colour in row-major order, Black first, a
    pass (action S*S) where a colour has none left -- never two passes in a row, no capture on the way for the positions here."""
    bp, wp = [int(p) for p in np.flatnonzero(black)], [int(p) for p in np.flatnonzero(white)]
    out = []
    for i in range(max(len(bp), len(wp))):
        out.append(bp[i] if i < len(bp) else S * S)
        if i < len(wp) or i + 1 < len(bp):
            out.append(wp[i] if i < len(wp) else S * S)
    return out
