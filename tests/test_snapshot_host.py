"""Host side of checkpoint and resume (transgo_amd/snapshot.py): the file parsers refuse damaged input with ValueError, and a
failed write leaves nothing under the final name.  No GPU."""
import ctypes
import json
import os
import re
import shutil

import numpy as np
import pytest

from transgo_amd import _lib, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parts(k=2):
    rng = np.random.RandomState(3)
    return [({"n_games": 4, "board_size": 9, "seeds": [1, 2, 3, 4 + i], "_parked": None}, rng.randint(0, 256, 100 + 7 * i).astype(np.uint8))
            for i in range(k)]


def test_checkpoint_round_trip(tmp_path):
    path = str(tmp_path / "c.bin")
    parts = _parts()
    snapshot.write_checkpoint(path, parts)
    back = snapshot.read_checkpoint(path)
    assert [s for s, _ in back] == [s for s, _ in parts]
    assert all((a == b).all() for (_, a), (_, b) in zip(back, parts))
    assert os.listdir(tmp_path) == ["c.bin"]                          # the temporary file is gone


def test_checkpoint_parser_rejects_damage(tmp_path):
    path = str(tmp_path / "c.bin")
    snapshot.write_checkpoint(path, _parts())
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw[8:16], np.uint64)[0])
    head = json.loads(raw[16:16 + n])
    overrun = dict(head, parts=[dict(head["parts"][0], snapshot_bytes=10 ** 9), head["parts"][1]])
    oj = json.dumps(overrun).encode()
    cases = {
        "empty": b"", "magic only": raw[:8], "cut in the length": raw[:12], "cut in the JSON": raw[:16 + n // 2],
        "cut in the data": raw[:-5], "trailing bytes": raw + b"xx", "wrong magic": b"X" + raw[1:],
        "JSON length overruns": raw[:8] + np.uint64(10 ** 12).tobytes() + raw[16:],
        "sizes overrun": raw[:8] + np.uint64(len(oj)).tobytes() + oj + raw[16 + n:],
        "not JSON": raw[:16] + b"\xff" * n + raw[16 + n:],
        "JSON of another shape": raw[:8] + np.uint64(2).tobytes() + b"[]" + raw[16 + n:],
    }
    for what, data in cases.items():
        bad = str(tmp_path / "bad.bin")
        with open(bad, "wb") as f:
            f.write(data)
        with pytest.raises(ValueError):
            snapshot.read_checkpoint(bad)
            pytest.fail(what + " was accepted")


def test_failed_write_leaves_no_partial_file(tmp_path):
    d = tmp_path / "ckpt"
    d.mkdir()
    path = str(d / "c.bin")
    snapshot.write_checkpoint(path, _parts())
    good = open(path, "rb").read()

    def parts_then_trouble():
        yield _parts()[0]
        raise OSError("disk went away")
    with pytest.raises(OSError):
        snapshot.write_checkpoint(path, parts_then_trouble())
    assert os.listdir(d) == ["c.bin"] and open(path, "rb").read() == good        # the old checkpoint stands, no temporary file is left

    # the directory disappears while the checkpoint is written: nothing appears under the final name
    class Vanishing:
        def __array__(self, dtype=None, copy=None):
            shutil.rmtree(d)
            return np.zeros(64, np.uint8)
    with pytest.raises(OSError):
        snapshot.write_checkpoint(path, [({"n_games": 1}, Vanishing())])
    assert not os.path.exists(path) and not os.path.exists(d)


def _header(**over):
    h = snapshot.SnapHdr()
    h.magic = snapshot.SNAP_MAGIC
    h.version, h.header_bytes = snapshot.SNAP_VERSION, snapshot.HEADER_BYTES
    h.n_games, h.board_size = 4, 9
    off = snapshot.HEADER_BYTES
    for i in range(len(snapshot.SECTIONS)):
        h.sec[i].off, h.sec[i].bytes = off, 32
        off += 32
    h.total_bytes = off
    for k, v in over.items():
        setattr(h, k, v)
    return bytes(h) + b"\0" * (off - snapshot.HEADER_BYTES)


def test_engine_snapshot_header_parser():
    buf = _header()
    hdr = snapshot.parse_header(buf)
    assert hdr["n_games"] == 4 and hdr["sections"]["tree"] == (snapshot.HEADER_BYTES + 8 * 32, 32)
    snapshot.check_length(hdr, len(buf))
    with pytest.raises(ValueError, match="truncated"):
        snapshot.parse_header(buf[:100])
    with pytest.raises(ValueError, match="magic"):
        snapshot.parse_header(b"Q" + buf[1:])
    with pytest.raises(ValueError, match="version"):
        snapshot.parse_header(_header(version=99))
    with pytest.raises(ValueError, match="truncated"):
        snapshot.check_length(hdr, len(buf) // 2)
    with pytest.raises(ValueError, match="truncated"):
        snapshot.section(np.frombuffer(buf[:len(buf) // 2], np.uint8), hdr, "hist_pl")


def test_header_mirror_matches_the_library_source():
    """SnapHdr and the GameCtl dtype are hand-written mirrors of csrc/snapshot.hip and csrc/tree_dev.h: same fields, same order."""
    src = open(os.path.join(ROOT, "transgo_amd", "csrc", "snapshot.hip")).read()
    body = src[src.index("struct SnapHdr {"):src.index("static_assert(sizeof(SnapHdr)")]
    body = re.sub(r"//[^\n]*", "", body[body.index("{") + 1:body.rindex("}")])
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in snapshot.SnapHdr._fields_]
    assert f"sizeof(SnapHdr) == {snapshot.HEADER_BYTES}" in src and f"sizeof(GameCtl) == {snapshot.GAME_CTL.itemsize}" in src
    names_sec = re.search(r"kSecName\[SEC_N\] = \{(.*?)\};", src, re.S).group(1)
    assert tuple(re.findall(r'"(\w+)"', names_sec)) == snapshot.SECTIONS
    tree = open(os.path.join(ROOT, "transgo_amd", "csrc", "tree_dev.h")).read()
    ctl = tree[tree.index("struct GameCtl {"):]
    ctl = re.sub(r"//[^\n]*", "", ctl[:ctl.index("};")])
    fields = re.findall(r"(?:int32_t|unsigned long long)\s+(\w+);", ctl)
    assert fields == [n for n in snapshot.GAME_CTL.names if n != "_pad"]


def test_replay_file_parser_rejects_damage(tmp_path):
    S, C, cap, appended = 9, 10, 64, 100
    sec, total = snapshot.replay_layout(S, C, 64)
    good = snapshot.REPLAY_MAGIC + np.array([S, C, cap, appended], np.int64).tobytes() + b"\0" * (total - 40)
    path = str(tmp_path / "r.bin")
    open(path, "wb").write(good)
    assert snapshot.read_replay_header(path)[:5] == (S, C, cap, appended, 64)
    hdr = lambda *v: snapshot.REPLAY_MAGIC + np.array(v, np.int64).tobytes()
    for what, data in {"empty": b"", "cut in the header": good[:20], "cut in the data": good[:-1], "trailing": good + b"x",
                       "wrong magic": b"Z" + good[1:], "sizes overrun": hdr(S, C, 10 ** 12, 10 ** 12) + good[40:],
                       "negative": hdr(S, C, cap, -1) + good[40:], "board": hdr(7, C, cap, appended) + good[40:]}.items():
        open(path, "wb").write(data)
        with pytest.raises(ValueError):
            snapshot.read_replay_header(path)
            pytest.fail(what + " was accepted")


def test_new_symbols_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "transgo_hip.h")).read()
    for name in ("tg_sp_snapshot_size", "tg_sp_snapshot", "tg_sp_restore", "tg_replay_export", "tg_replay_import"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
