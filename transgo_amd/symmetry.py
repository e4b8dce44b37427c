"""Symmetry-aware evaluation, restated in NumPy: the definition the device path (tg_net_set_symmetry, csrc/symmetry.hip) is
tested against, and the same feature for evaluators that run on the host.

Symmetry s = 0..7 is the augmentation index of the reference's loop (self_play.py:943-965), s = 2*(i-1) + f:
T_s(m) = np.rot90(m, i) for i = 1..4, then np.fliplr if f == 1; s = 6 is the identity.  Evaluating a position x under s is
T_s on each plane of x, the unchanged evaluator on the result, and the outputs mapped back to x's orientation: the board part of
the policy and the ownership through the inverse of T_s, the pass entry and the value as they are.

Modes: "none" (the evaluator itself), an int s (every row under s), "position" (row r under position_symmetry(seed, its
bit-packed planes): a pure function of the position, so the same position gets the same orientation in whatever batch it
appears) and "mean8" (all eight, accumulated in float32 in the order s = 0..7, then * 0.125).
"""
import numpy as np

IDENTITY = 6
MODES = {"none": 0, "fixed": 1, "position": 2, "mean8": 3}


def parse_mode(mode, arg=0):
    """("none" | "position" | "mean8" | "fixed" | int s, arg) -> (mode number 0..3, arg) as tg_net_set_symmetry takes them."""
    if mode is None:
        mode = "none"
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"symmetry mode {mode!r}: one of 'none', 'position', 'mean8' or an int 0..7")
        m = MODES[mode]
    else:
        m, arg = 1, int(mode)
    arg = int(arg)
    if m == 1 and not 0 <= arg <= 7:
        raise ValueError(f"a fixed symmetry is 0..7, got {arg}")
    if m in (0, 3):
        arg = 0
    return m, arg & 0xFFFFFFFF


def _t(m, s):
    """T_s on the last two axes of m."""
    i, f = (s >> 1) + 1, s & 1
    y = np.rot90(m, i, axes=(-2, -1))
    return y[..., ::-1] if f else y


def _t_inv(m, s):
    """The inverse of T_s on the last two axes of m."""
    i, f = (s >> 1) + 1, s & 1
    y = m[..., ::-1] if f else m
    return np.rot90(y, -i, axes=(-2, -1))


def _check(s):
    s = int(s)
    if not 0 <= s <= 7:
        raise ValueError(f"symmetry {s} is not in 0..7")
    return s


def transform_planes(x, s):
    """T_s on every plane of x ([..., S, S]; one position [C, S, S] or a batch [N, C, S, S])."""
    return np.ascontiguousarray(_t(np.asarray(x), _check(s)))


def untransform_board(o, s, S):
    """A board-shaped output o' ([..., S*S]) of the transformed position, back in the original orientation."""
    o = np.asarray(o)
    return np.ascontiguousarray(_t_inv(o.reshape(o.shape[:-1] + (S, S)), _check(s))).reshape(o.shape)


def untransform_policy(p, s, S):
    """A policy p' ([..., S*S + 1]) of the transformed position, back in the original orientation; the pass entry stays."""
    p = np.asarray(p)
    out = np.empty_like(p)
    out[..., :S * S] = untransform_board(p[..., :S * S], s, S)
    out[..., S * S] = p[..., S * S]
    return out


def transform_policy(p, s, S):
    """The policy of the original orientation as the transformed position sees it (the inverse of untransform_policy)."""
    p = np.asarray(p)
    out = np.empty_like(p)
    b = p[..., :S * S]
    out[..., :S * S] = np.ascontiguousarray(_t(b.reshape(b.shape[:-1] + (S, S)), _check(s))).reshape(b.shape)
    out[..., S * S] = p[..., S * S]
    return out


def pack_planes(x):
    """Planes [N, C, S, S] (or one position [C, S, S]) -> uint32 [N, ceil(C*S*S/32)] (or [W]): bit i of a row is plane-major flat
    index i, set where the plane value is nonzero; the unused high bits of the last word are zero.  The layout of the engine's
    evaluation batch and of tg_sp_harvest's obs_bits."""
    x = np.asarray(x)
    one = x.ndim == 3
    flat = (x.reshape(1 if one else x.shape[0], -1) != 0)
    n, nbits = flat.shape
    W = (nbits + 31) // 32
    padded = np.zeros((n, W * 32), np.uint8)
    padded[:, :nbits] = flat
    words = np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(n, W)
    return words[0] if one else words


def position_symmetry(seed, packed_words):
    """sym_of(seed, words): the orientation mode "position" gives a row.  uint32 arithmetic: h = seed ^ 0x9E3779B9; per word in
    order h = (h ^ w) * 0x01000193; murmur3's fmix32; s = h >> 29.  packed_words: uint32 [W] -> int, or [N, W] -> int array [N]."""
    w = np.asarray(packed_words, np.uint32)
    one = w.ndim == 1
    w = w.reshape(1, -1) if one else w
    h = np.full(w.shape[0], (int(seed) & 0xFFFFFFFF) ^ 0x9E3779B9, np.uint32)
    with np.errstate(over="ignore"):
        for j in range(w.shape[1]):
            h = (h ^ w[:, j]) * np.uint32(0x01000193)
        h ^= h >> np.uint32(16); h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13); h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    s = (h >> np.uint32(29)).astype(np.int64)
    return int(s[0]) if one else s


def _call(fn, x, S):
    """fn(x) -> (policy [N, A], value [N], own [N, P] or None), as float32."""
    out = fn(x)
    pol = np.asarray(out[0], np.float32)
    val = np.asarray(out[1], np.float32)
    own = np.asarray(out[2], np.float32) if len(out) > 2 and out[2] is not None else None
    return pol, val, own


def _under(fn, obs, s_rows, S):
    """Every row r of obs under s_rows[r], in ONE call of fn on the batch in its own row order; outputs mapped back."""
    x = np.empty_like(obs)
    for s in np.unique(s_rows):
        m = s_rows == s
        x[m] = transform_planes(obs[m], s)
    pol, val, own = _call(fn, x, S)
    p = np.empty_like(pol)
    o = None if own is None else np.empty_like(own)
    for s in np.unique(s_rows):
        m = s_rows == s
        p[m] = untransform_policy(pol[m], s, S)
        if o is not None:
            o[m] = untransform_board(own[m], s, S)
    return p, val, o


def evaluate_with_symmetry(fn, obs, mode="none", arg=0):
    """fn(obs [N, C, S, S] float32) -> (policy [N, S*S+1], value [N] or [N, 1][, own [N, S*S]]) evaluated under a symmetry mode
    ("none" | "position" | "mean8" | "fixed" | int s; arg = s for "fixed", the seed for "position").  Returns what fn returns, in
    the original orientation.  fn is called on whole batches in obs's row order (once; eight times for "mean8", s = 0..7), so an fn
    whose result for a row depends on the row's place in the batch sees the places the device path uses."""
    m, arg = parse_mode(mode, arg)
    if m == 0:
        return fn(obs)
    obs = np.ascontiguousarray(obs, np.float32)
    N, S = obs.shape[0], obs.shape[-1]
    ret = lambda p, v, o: (p, v) if o is None else (p, v, o)
    if m == 1:
        return ret(*_under(fn, obs, np.full(N, arg, np.int64), S))
    if m == 2:
        return ret(*_under(fn, obs, position_symmetry(arg, pack_planes(obs)), S))
    acc = None
    for s in range(8):
        cur = _under(fn, obs, np.full(N, s, np.int64), S)
        acc = cur if acc is None else tuple(None if a is None else a + c for a, c in zip(acc, cur))      # float32 + float32
    return ret(*[None if a is None else a * np.float32(0.125) for a in acc])
