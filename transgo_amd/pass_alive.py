"""Pass-alive groups and territory (Benson's algorithm): the NumPy restatement of csrc/pass_alive_dev.h.

For each colour X: chains are X's groups; regions are the maximal 4-connected sets of points without an X stone (empty points
and the opponent's stones together).  A region is vital to a chain if it has an empty point and every one of its empty points
is a liberty of the chain.  All chains and regions start live; a chain with fewer than two live vital regions dies, a region
that touches a dead chain dies, until nothing changes.  The surviving chains are pass-alive: they cannot be captured even if X
passes for ever.  A surviving region is X's pass-alive territory if at most one of its points (empty or not) has no X stone
next to it: the opponent can then never make two eyes inside.

status int8[P]: +2 pass-alive Black stone, +1 Black pass-alive territory (empty point or dead White stone), -2 / -1 White
likewise, 0 everything else.  A position is settled if no point has status 0.  The pass-alive-aware area gives a point to the
colour of its status, and to Tromp-Taylor where the status is 0.

This module is the definition the kernels are tested against; it is plain Python and slow on purpose.
"""
import numpy as np

BLACK, WHITE = 1, 2


def _size(n):
    S = int(round(np.sqrt(n)))
    if S * S != n:
        raise ValueError("a board has S*S points")
    return S


def _neighbours(S):
    nb = []
    for p in range(S * S):
        y, x = divmod(p, S)
        nb.append([q for ok, q in ((x > 0, p - 1), (y > 0, p - S), (x < S - 1, p + 1), (y < S - 1, p + S)) if ok])
    return nb


_NB = {}


def neighbours(S):
    if S not in _NB:
        _NB[S] = _neighbours(S)
    return _NB[S]


def components(member, nb):
    """Labels of the 4-connected components of the points with member[p] (label = lowest point), -1 elsewhere."""
    lab = np.full(len(member), -1, np.int32)
    for p in range(len(member)):
        if not member[p] or lab[p] >= 0:
            continue
        lab[p] = p
        stack = [p]
        while stack:
            q = stack.pop()
            for r in nb[q]:
                if member[r] and lab[r] < 0:
                    lab[r] = p
                    stack.append(r)
    return lab


def _one_colour(x, emp, nb):
    """-> (alive[P]: pass-alive stones of the colour with stones x, terr[P]: its pass-alive territory)."""
    P = len(x)
    chain = components(x, nb)
    region = components(~x, nb)
    chains = sorted(set(chain[chain >= 0].tolist()))
    regions = sorted(set(region[region >= 0].tolist()))
    libs = {c: set() for c in chains}                 # empty points next to the chain
    touch = {r: set() for r in regions}               # chains with a stone next to a point of the region
    for p in range(P):
        if x[p]:
            for q in nb[p]:
                if emp[q]:
                    libs[chain[p]].add(q)
                if not x[q]:
                    touch[region[q]].add(chain[p])
    vital = {c: [] for c in chains}
    for r in regions:
        e = [p for p in range(P) if region[p] == r and emp[p]]
        if not e:
            continue
        for c in touch[r]:
            if all(p in libs[c] for p in e):
                vital[c].append(r)
    live_c = {c: True for c in chains}
    live_r = {r: True for r in regions}
    for _ in range(len(chains) + 1):                  # every round but the last kills a chain
        changed = False
        for c in chains:
            if live_c[c] and sum(live_r[r] for r in vital[c]) < 2:
                live_c[c] = False
                changed = True
        for r in regions:
            if live_r[r] and any(not live_c[c] for c in touch[r]):
                live_r[r] = False
        if not changed:
            break
    else:
        raise AssertionError("pass_alive: no fixed point")
    alive = np.array([bool(x[p]) and live_c[chain[p]] for p in range(P)])
    interior = np.array([not x[p] and not any(x[q] for q in nb[p]) for p in range(P)])
    terr = np.zeros(P, bool)
    for r in regions:
        if live_r[r] and int(interior[region == r].sum()) <= 1:
            terr |= region == r
    return alive, terr


def pass_alive(black, white):
    """black, white: bool[P] (or [S][S]) stones of a position -> status int8[P]."""
    b = np.asarray(black, bool).reshape(-1)
    w = np.asarray(white, bool).reshape(-1)
    if b.shape != w.shape or (b & w).any():
        raise ValueError("pass_alive: two stone sets of one board")
    nb = neighbours(_size(len(b)))
    emp = ~(b | w)
    ab, tb = _one_colour(b, emp, nb)
    aw, tw = _one_colour(w, emp, nb)
    assert not ((ab | tb) & (aw | tw)).any(), "pass_alive: a point claimed by both colours"
    return (2 * ab.astype(np.int8) + tb.astype(np.int8) - 2 * aw.astype(np.int8) - tw.astype(np.int8)).astype(np.int8)


def settled(status):
    return bool((np.asarray(status) != 0).all())


def tromp_taylor_owner(black, white):
    """+1 / -1 / 0 per point: stones to their colour, an empty region to the only colour it touches (board.cc:822-958)."""
    b = np.asarray(black, bool).reshape(-1)
    w = np.asarray(white, bool).reshape(-1)
    nb = neighbours(_size(len(b)))
    emp = ~(b | w)
    lab = components(emp, nb)
    own = b.astype(np.int8) - w.astype(np.int8)
    for r in set(lab[lab >= 0].tolist()):
        pts = np.flatnonzero(lab == r)
        tb = any(b[q] for p in pts for q in nb[p])
        tw = any(w[q] for p in pts for q in nb[p])
        own[pts] = 1 if (tb and not tw) else -1 if (tw and not tb) else 0
    return own


def area_score(black, white, komi, status=None):
    """The pass-alive-aware area -> (score float32 = #Black - #White - komi, owner int8[P]); Black wins iff score > 0."""
    st = pass_alive(black, white) if status is None else np.asarray(status, np.int8).reshape(-1)
    own = tromp_taylor_owner(black, white)
    own = np.where(st != 0, np.sign(st), own).astype(np.int8)
    score = np.float32(int((own == 1).sum()) - int((own == -1).sum())) - np.float32(komi)
    return np.float32(score), own


def stones_of_states(states, board_size):
    """State blobs uint8[n][state_bytes] (two bitboards first, tg_state_size) -> (black, white) bool[n][P]."""
    st = np.ascontiguousarray(states, np.uint8)
    st = st.reshape(1, -1) if st.ndim == 1 else st
    P = board_size * board_size
    nw = (P + 63) // 64
    bits = np.unpackbits(st[:, : 16 * nw], axis=1, bitorder="little").reshape(len(st), 2, nw * 64)[:, :, :P].astype(bool)
    return bits[:, 0], bits[:, 1]
