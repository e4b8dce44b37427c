"""transgo_amd.symmetry, the NumPy restatement of symmetry-aware evaluation: the numbering is the reference's augmentation order,
the back-map inverts the transform, the position hash is the literal per-bit definition, and the modes are what they say.  No GPU."""
import os

import numpy as np
import pytest

from transgo_amd import symmetry


def encoded_positions(S, C, k, seed):
    """k distinct encoded positions [k, C, S, S] from random play (oracle rules engine)."""
    from oracle.go_oracle import OracleGoEnv
    env = OracleGoEnv(board_size=S, max_step=S * S, encode_dim=C)
    rng = np.random.RandomState(seed)
    obs, seen = [], set()
    while len(obs) < k:
        s, done = env.reset()
        while not done and len(obs) < k:
            la = env.getLegalAction(s)
            s, done = env.step(s, int(la[rng.randint(len(la))]))
            e = env.encode(s)
            if e.tobytes() not in seen:
                seen.add(e.tobytes())
                obs.append(e)
    return np.stack(obs)


def test_transform_planes_is_the_reference_augmentation_order(golden_dir):
    with np.load(os.path.join(golden_dir, "targets_game.npz")) as z:
        obs = z["obs"]
    n = len(obs) // 8
    assert n >= 4
    for i in range(n):
        x = obs[8 * i + 6]                                # rot90 by 4 quarter turns, no flip: the position itself
        assert np.array_equal(symmetry.transform_planes(x, symmetry.IDENTITY), x)
        for s in range(8):
            assert np.array_equal(symmetry.transform_planes(x, s), obs[8 * i + s]), (i, s)
    batch = obs[6::8]
    for s in range(8):
        assert np.array_equal(symmetry.transform_planes(batch, s), obs[s::8])


@pytest.mark.parametrize("S", [9, 19])
def test_untransform_inverts_transform(S):
    rng = np.random.RandomState(S)
    P = S * S
    pi = rng.rand(3, P + 1).astype(np.float32)
    pi[:, P] = [7.0, 8.0, 9.0]                            # a pass entry no board entry equals
    own = rng.rand(3, P).astype(np.float32)
    for s in range(8):
        t = symmetry.transform_policy(pi, s, S)
        assert np.array_equal(t[:, :P].reshape(3, S, S), symmetry.transform_planes(pi[:, :P].reshape(3, S, S), s))
        assert np.array_equal(t[:, P], pi[:, P])
        assert np.array_equal(symmetry.untransform_policy(t, s, S), pi)
        to = symmetry.transform_planes(own.reshape(3, S, S), s).reshape(3, P)
        assert np.array_equal(symmetry.untransform_board(to, s, S), own)
        if s != symmetry.IDENTITY:
            assert not np.array_equal(t, pi)
    with pytest.raises(ValueError):
        symmetry.transform_planes(pi[:, :P].reshape(3, S, S), 8)


def literal_sym_of(seed, x):
    """The definition, bit by bit: pack plane-major flat index i into bit i of the words, then hash in Python integers."""
    flat = x.reshape(-1)
    words = [0] * ((len(flat) + 31) // 32)
    for i, v in enumerate(flat):
        if v != 0:
            words[i >> 5] |= 1 << (i & 31)
    M = 0xFFFFFFFF
    h = (seed ^ 0x9E3779B9) & M
    for w in words:
        h = ((h ^ w) * 0x01000193) & M
    h ^= h >> 16; h = (h * 0x85EBCA6B) & M
    h ^= h >> 13; h = (h * 0xC2B2AE35) & M
    h ^= h >> 16
    return h >> 29, words


@pytest.mark.parametrize("S,C,k", [(9, 10, 200), (9, 13, 200), (19, 10, 200)])
def test_position_symmetry_is_the_literal_definition(S, C, k):
    x = encoded_positions(S, C, k, seed=S + C)
    packed = symmetry.pack_planes(x)
    assert packed.dtype == np.uint32 and packed.shape == (k, (C * S * S + 31) // 32)
    lit = [literal_sym_of(0, x[i]) for i in range(k)]
    assert np.array_equal(packed, np.array([w for _, w in lit], np.uint64).astype(np.uint32))
    assert np.array_equal(symmetry.pack_planes(x[3]), packed[3])
    tail = (C * S * S) & 31
    assert tail and (packed[:, -1] >> np.uint32(tail)).max() == 0          # unused high bits of the last word are zero
    for seed in (0, 1, 0xFFFFFFFF):
        want = np.array([literal_sym_of(seed, x[i])[0] for i in range(k)])
        got = symmetry.position_symmetry(seed, packed)
        assert np.array_equal(got, want), seed
        assert symmetry.position_symmetry(seed, packed[5]) == want[5]
        assert set(want.tolist()) == set(range(8)), (seed, np.bincount(want, minlength=8))    # a condition on the inputs: every s occurs


def skewed_fn(S, C, seed=0):
    """A deliberately non-equivariant evaluator: every output depends on WHERE on the board a plane bit sits."""
    rng = np.random.RandomState(seed)
    P = S * S
    w_pol = rng.randn(C, P).astype(np.float32)
    w_own = rng.randn(C, P).astype(np.float32)
    w_val = rng.randn(C * P).astype(np.float32)
    ramp = np.linspace(-1, 1, P + 1, dtype=np.float32)

    def fn(obs):
        o = np.asarray(obs, np.float32).reshape(len(obs), C, P)
        logit = np.concatenate([(o * w_pol).sum(1), np.full((len(o), 1), 0.25, np.float32)], axis=1) + ramp
        e = np.exp(logit - logit.max(1, keepdims=True))
        pol = (e / e.sum(1, keepdims=True)).astype(np.float32)
        val = np.tanh((o.reshape(len(o), -1) * w_val).sum(1) * np.float32(0.1)).astype(np.float32)
        own = np.tanh((o * w_own).sum(1)).astype(np.float32)
        return pol, val, own
    return fn


def test_mean8_is_the_float32_loop_in_order():
    S, C = 9, 10
    x = encoded_positions(S, C, 12, seed=4)
    fn = skewed_fn(S, C)
    acc = None
    for s in range(8):
        i, f = s // 2 + 1, s % 2
        t = np.rot90(x, i, axes=(2, 3))
        t = np.ascontiguousarray(t[..., ::-1] if f else t)
        p, v, o = fn(t)
        back = lambda b: np.rot90(b[..., ::-1] if f else b, -i, axes=(1, 2)).reshape(len(x), S * S)
        p0 = np.concatenate([back(p[:, :S * S].reshape(-1, S, S)), p[:, S * S:]], axis=1)
        cur = [p0, v, back(o.reshape(-1, S, S))]
        assert all(c.dtype == np.float32 for c in cur)
        acc = cur if acc is None else [a + c for a, c in zip(acc, cur)]
    want = [a * np.float32(0.125) for a in acc]
    got = symmetry.evaluate_with_symmetry(fn, x, "mean8")
    assert len(got) == 3 and all(g.dtype == np.float32 and np.array_equal(g, w) for g, w in zip(got, want))
    plain = fn(x)
    assert not np.array_equal(got[0], plain[0])                               # the evaluator really is orientation-dependent
    fixed = symmetry.evaluate_with_symmetry(fn, x, 3)
    assert not np.array_equal(fixed[0], plain[0]) and abs(float(fixed[0].sum(1).max()) - 1) < 1e-5
    assert all(np.array_equal(a, b) for a, b in zip(symmetry.evaluate_with_symmetry(fn, x, symmetry.IDENTITY), plain))
    # "position": each row under its own s, whatever batch it is part of
    s_rows = symmetry.position_symmetry(9, symmetry.pack_planes(x))
    pos = symmetry.evaluate_with_symmetry(fn, x, "position", 9)
    for r in range(len(x)):
        one = symmetry.evaluate_with_symmetry(fn, x[r:r + 1], int(s_rows[r]))
        assert all(np.array_equal(a[r:r + 1], b) for a, b in zip(pos, one)), r
    # a two-output evaluator (policy, value) comes back as two outputs
    two = symmetry.evaluate_with_symmetry(lambda o: fn(o)[:2], x, "mean8")
    assert len(two) == 2 and np.array_equal(two[0], want[0]) and np.array_equal(two[1], want[1])


def test_empty_board_every_mode_equals_none_for_an_equivariant_fn():
    """fn sees the position through an isotropic 3x3 sum only, so it is equivariant by construction; its outputs are quantised to
    multiples of 2^-12, which leaves the three spare mantissa bits that make the sum of eight EQUAL float32 values exact (the
    mean of eight equal values is then that value, bit for bit)."""
    from oracle.go_oracle import OracleGoEnv
    S, C, P = 9, 10, 81
    env = OracleGoEnv(board_size=S, encode_dim=C)
    s0, _ = env.reset()
    x = env.encode(s0)[None]
    assert all(np.array_equal(symmetry.transform_planes(x, s), x) for s in range(8))
    gain = np.linspace(0.5, 1.5, C, dtype=np.float32)[None, :, None, None]

    def fn(obs):
        o = (np.asarray(obs, np.float32) + 1) * gain      # + 1: the empty board's planes are all zero; the zero border shows
        pad = np.pad(o, ((0, 0), (0, 0), (1, 1), (1, 1)))
        box = sum(pad[:, :, 1 + dy:1 + dy + S, 1 + dx:1 + dx + S] for dy in (-1, 0, 1) for dx in (-1, 0, 1)).sum(1)    # [N, S, S]
        q = lambda a: (np.round(a * 4096) / 4096).astype(np.float32)
        pol = q(np.concatenate([box.reshape(-1, P) / 64, np.full((len(o), 1), 0.125, np.float32)], axis=1))
        return pol, q(np.tanh(box.reshape(-1, P).sum(1) / 100)), q(np.tanh(box.reshape(-1, P) / 8))

    want = fn(x)
    assert len(np.unique(want[0])) > 3                    # corners, edges and the middle differ: not a constant map
    for mode, arg in [("none", 0), ("position", 0), ("position", 12345), ("mean8", 0)] + [(s, 0) for s in range(8)]:
        got = symmetry.evaluate_with_symmetry(fn, x, mode, arg)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), mode


def test_parse_mode():
    assert symmetry.parse_mode("none") == (0, 0) and symmetry.parse_mode(None) == (0, 0)
    assert symmetry.parse_mode(5) == (1, 5) and symmetry.parse_mode("position", 77) == (2, 77) and symmetry.parse_mode("mean8", 3) == (3, 0)
    for bad in (8, -1, "all"):
        with pytest.raises(ValueError):
            symmetry.parse_mode(bad)
