"""Host side of checkpoint and resume: the header of an engine snapshot (tg_sp_snapshot, csrc/snapshot.hip) and the checkpoint
file BatchedSelfPlay / GroupedSelfPlay write.  Nothing here needs a GPU; every parser raises ValueError on damaged input.

Checkpoint file:   b"TGCKPT1\\0" | u64 length of the JSON header | JSON header (UTF-8) | the engine snapshots, back to back
The JSON header is {"format": 1, "parts": [{"state": {...}, "snapshot_bytes": n}, ...]}: one part per engine (BatchedSelfPlay
writes one, GroupedSelfPlay one per group), `state` = the worker's own counters (see BatchedSelfPlay.save_checkpoint).  A
checkpoint holds data only -- no pickle, nothing executable; network weights are not part of it."""
import ctypes
import json
import os

import numpy as np

SNAP_MAGIC = b"TGSNAP\0\0"
SNAP_VERSION = 1
SECTIONS = ("game_ctl", "pool_ctl", "ring", "chunk_ids", "counters", "moves", "finished",
            "rng", "tree", "hist_obs", "hist_cnt", "hist_pl")
ECHO_FIELDS = ("board_size", "encode_dim", "n_games", "parallel_readouts", "chunk_slots", "pool_chunks", "max_chunks", "arena_slots",
               "keep_slots", "maxd", "hist_T", "record_games", "max_step", "wu_loss", "komi", "c_puct1", "c_puct2")


class SnapSec(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


class SnapHdr(ctypes.Structure):                       # mirrors csrc/snapshot.hip:SnapHdr
    _fields_ = [("magic", ctypes.c_char * 8), ("version", ctypes.c_uint32), ("header_bytes", ctypes.c_uint32)] + \
               [(n, ctypes.c_int32) for n in ECHO_FIELDS[:14]] + \
               [("komi", ctypes.c_float), ("pad0", ctypes.c_int32), ("c_puct1", ctypes.c_double), ("c_puct2", ctypes.c_double),
                ("all_reset", ctypes.c_int32), ("n_errors", ctypes.c_int32), ("fin_positions", ctypes.c_int32), ("n_fin", ctypes.c_int32),
                ("tree_chunks", ctypes.c_uint64), ("hist_plies", ctypes.c_uint64), ("tables_bytes", ctypes.c_uint64),
                ("total_bytes", ctypes.c_uint64), ("sec", SnapSec * len(SECTIONS))]


HEADER_BYTES = ctypes.sizeof(SnapHdr)

# GameCtl (csrc/tree_dev.h), 112 bytes
GAME_CTL = np.dtype([(n, "<i4") for n in ("cur", "free_slot", "n_chunks", "root", "spare", "n_target", "active", "n_paths", "need_eval",
                                          "root_row", "finished", "error", "searching", "moves", "hw_slot", "_pad")] +
                    [(n, "<u8") for n in ("sims", "evals", "depth_sum", "tie_draws", "child_sum", "truncs")])
assert GAME_CTL.itemsize == 112


def parse_header(buf):
    """The header of an engine snapshot as a dict (echo fields, counts, "sections": name -> (offset, bytes)).  `buf`: bytes or a
    uint8 array holding at least the header; `len(buf)` is taken as the snapshot's length when it holds more."""
    raw = bytes(memoryview(buf)[:HEADER_BYTES])
    if len(raw) < HEADER_BYTES:
        raise ValueError("truncated engine snapshot (shorter than its header)")
    h = SnapHdr.from_buffer_copy(raw)
    if raw[:8] != SNAP_MAGIC:
        raise ValueError("not an engine snapshot (wrong magic)")
    if h.version != SNAP_VERSION or h.header_bytes != HEADER_BYTES:
        raise ValueError(f"engine snapshot format version {h.version} (this package reads version {SNAP_VERSION})")
    out = {n: getattr(h, n) for n in ECHO_FIELDS + ("all_reset", "n_errors", "fin_positions", "n_fin", "tree_chunks", "hist_plies",
                                                    "tables_bytes", "total_bytes")}
    out["sections"] = {n: (int(h.sec[i].off), int(h.sec[i].bytes)) for i, n in enumerate(SECTIONS)}
    return out


def check_length(hdr, n_bytes):
    """ValueError unless every section of the parsed header lies inside a buffer of n_bytes."""
    for name, (off, size) in hdr["sections"].items():
        if off + size > n_bytes:
            raise ValueError(f"truncated engine snapshot (section {name} ends at byte {off + size}, the buffer holds {n_bytes})")
    if hdr["total_bytes"] > n_bytes:
        raise ValueError("truncated engine snapshot")


def section(buf, hdr, name, dtype=np.uint8):
    """NumPy view of one section of a host snapshot."""
    off, size = hdr["sections"][name]
    if off + size > len(buf):
        raise ValueError(f"truncated engine snapshot (section {name})")
    return np.asarray(buf)[off:off + size].view(dtype)


def game_flags(ctl):
    """(finished, errored) as SelfPlayEngine keeps them, from the GameCtl records: a slot takes no part in the next search when its
    game is over, parked or in error."""
    return (ctl["finished"] != 0) | (ctl["error"] != 0), ctl["error"] != 0


# ---- checkpoint file -------------------------------------------------------------------------------------------------------------
CKPT_MAGIC = b"TGCKPT1\0"


def write_checkpoint(path, parts):
    """parts: iterable of (state dict, snapshot as a uint8 array).  Written to a temporary name next to `path` and moved into place
    with os.replace, so `path` never holds a partial file; a failure removes the temporary file and is re-raised."""
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        parts = [(st, np.ascontiguousarray(np.asarray(sn), np.uint8)) for st, sn in parts]
        head = json.dumps({"format": 1, "parts": [{"state": st, "snapshot_bytes": int(sn.size)} for st, sn in parts]}).encode()
        with open(tmp, "wb") as f:
            f.write(CKPT_MAGIC)
            f.write(np.uint64(len(head)).tobytes())
            f.write(head)
            for _, sn in parts:
                f.write(memoryview(sn))
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def read_checkpoint(path):
    """-> list of (state dict, snapshot uint8 array).  ValueError on a truncated file, a wrong magic or a header whose sizes do not
    match the file."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        if f.read(8) != CKPT_MAGIC:
            raise ValueError("not a self-play checkpoint (wrong magic)")
        raw = f.read(8)
        if len(raw) < 8:
            raise ValueError("truncated checkpoint")
        n = int(np.frombuffer(raw, np.uint64)[0])
        if n > size - 16:
            raise ValueError("truncated checkpoint (the JSON header overruns the file)")
        head = json.loads(f.read(n).decode("utf-8", "strict"))          # JSONDecodeError and UnicodeDecodeError are ValueErrors
        if not isinstance(head, dict) or head.get("format") != 1 or not isinstance(head.get("parts"), list):
            raise ValueError("unknown checkpoint header")
        sizes = []
        for p in head["parts"]:
            if not isinstance(p, dict) or not isinstance(p.get("state"), dict) or not isinstance(p.get("snapshot_bytes"), int) \
                    or p["snapshot_bytes"] < 0:
                raise ValueError("damaged checkpoint header")
            sizes.append(p["snapshot_bytes"])
        if sum(sizes) != size - 16 - n:
            raise ValueError(f"checkpoint header describes {sum(sizes)} snapshot bytes, the file holds {size - 16 - n}")
        out = []
        for p, k in zip(head["parts"], sizes):
            sn = np.fromfile(f, np.uint8, k)
            if sn.size != k:
                raise ValueError("truncated checkpoint")
            out.append((p["state"], sn))
    return out


# ---- replay store file -------------------------------------------------------------------------------------------------------------
REPLAY_MAGIC = b"TGRSTOR1"


def replay_layout(S, C, n_held):
    """Byte offsets of the four arrays behind the 40-byte header of a DeviceReplayMemory file, and the file's length."""
    P, A, W = S * S, S * S + 1, (C * S * S + 31) // 32
    o, sec = 40, {}
    for name, dt, shape in (("obs_bits", np.uint32, (n_held, W)), ("counts", np.int32, (n_held, A)), ("z", np.float32, (n_held,)),
                            ("own", np.int8, (n_held, P))):
        sec[name] = (o, np.dtype(dt), shape)
        o += int(np.prod(shape)) * np.dtype(dt).itemsize
    return sec, o


def read_replay_header(path):
    """-> (S, C, capacity, appended, n_held, sections).  ValueError on a wrong magic, a damaged header or a file whose length does not
    match it."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        raw = f.read(40)
    if raw[:8] != REPLAY_MAGIC:
        raise ValueError("not a replay store file (wrong magic)")
    if len(raw) < 40:
        raise ValueError("truncated replay store file")
    S, C, cap, appended = (int(x) for x in np.frombuffer(raw[8:], np.int64))
    if S not in (9, 19) or not 1 <= C <= 64 or cap <= 0 or appended < 0:
        raise ValueError("damaged replay store header")
    n_held = min(cap, appended)
    sec, total = replay_layout(S, C, n_held)
    if total != size:
        raise ValueError(f"replay store file holds {size} bytes, its header describes {total}")
    return S, C, cap, appended, n_held, sec
