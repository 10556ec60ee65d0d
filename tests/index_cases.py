"""Model and key builders of the Object index tests (tests/test_index_cases_cpu.py,
tests/test_object_index_gpu.py).

The index (spacedrive_amd/csrc/object_index.hip) is an open-addressing table with linear probing
from home(key) = mix64(key) >> (64 - log2 slots).  mix64 is a bijection, so a test places keys:
`keys_with_home` inverts it to build any probe chain it wants.  `Model` is the dict the table must
agree with.  Numpy only: no torch, no library.
"""
import numpy as np

# mirrored from spacedrive_amd/csrc/sd_mix.h, sd_object_index.h and sd_object_index_plan.h:
MIX_C1 = 0xBF58476D1CE4E5B9        # mix64's two multipliers
MIX_C2 = 0x94D049BB133111EB
KEY_EMPTY = (1 << 64) - 1          # INDEX_EMPTY: the key word of a free slot
KEY_TOMB = (1 << 64) - 2           # INDEX_TOMB: the key word of an erased slot
MIN_SLOTS = 1024                   # INDEX_MIN_SLOTS
NONE = 0xFFFFFFFF                  # SD_CAS_NO_OBJECT
ID_LIMIT = 1 << 31                 # ids are below this

_M64 = (1 << 64) - 1
_INV_C1 = pow(MIX_C1, -1, 1 << 64)
_INV_C2 = pow(MIX_C2, -1, 1 << 64)


def mix64(z: int) -> int:
    """sd_mix.h mix64 (the splitmix64 finalizer)."""
    z &= _M64
    z = ((z ^ (z >> 30)) * MIX_C1) & _M64
    z = ((z ^ (z >> 27)) * MIX_C2) & _M64
    return z ^ (z >> 31)


def inv_mix64(h: int) -> int:
    """The key whose mix64 is h."""
    h &= _M64
    h ^= (h >> 31) ^ (h >> 62)
    h = (h * _INV_C2) & _M64
    h ^= (h >> 27) ^ (h >> 54)
    h = (h * _INV_C1) & _M64
    return h ^ (h >> 30) ^ (h >> 60)


def home(key: int, log2_slots: int) -> int:
    return mix64(key) >> (64 - log2_slots)


def keys_with_home(slot: int, log2_slots: int, count: int, first: int = 0) -> np.ndarray:
    """`count` distinct keys whose home in a table of 2^log2_slots slots is `slot`: the
    pre-images of (slot, first), (slot, first + 1), ... — never one of the two reserved words."""
    assert 0 <= slot < (1 << log2_slots) and first + count <= 1 << (64 - log2_slots)
    out = [inv_mix64((slot << (64 - log2_slots)) | (first + j)) for j in range(count)]
    assert KEY_EMPTY not in out and KEY_TOMB not in out
    return np.array(out, dtype=np.uint64)


def special_keys() -> np.ndarray:
    """0, 1, 2^64 - 1 (and 2^64 - 2: the other word the table reserves), and the keys that mix64
    sends to 0, 1 and 2^64 - 1."""
    return np.array([0, 1, KEY_EMPTY, KEY_TOMB, inv_mix64(0), inv_mix64(1), inv_mix64(_M64)], dtype=np.uint64)


class Model(dict):
    """key -> smallest id inserted for it since it was last erased."""

    def insert(self, keys, ids) -> None:
        ids = [int(i) for i in ids]
        if any(i < 0 or i >= ID_LIMIT for i in ids):
            raise ValueError("an id >= 2^31 refuses the whole batch")
        for k, i in zip((int(k) for k in keys), ids):
            self[k] = min(self.get(k, i), i)

    def erase(self, keys) -> None:
        for k in keys:
            self.pop(int(k), None)

    def lookup(self, keys) -> np.ndarray:
        return np.array([self.get(int(k), NONE) for k in keys], dtype=np.uint32)

    def pairs(self) -> set:
        return set(self.items())


def reidentify(model: Model, rows: dict, path, new_key=None) -> None:
    """The caller's rule when file_path `path` is deleted (new_key None) or re-identified: erase
    its old cas key and re-insert the (key, id) pairs that remain for it.  rows: path -> (key,
    Object id), the DB's file_path table."""
    old_key, obj = rows.pop(path)
    if new_key is not None:
        rows[path] = (new_key, obj)
    model.erase([old_key])
    left = [(k, o) for k, o in rows.values() if k == old_key]
    model.insert([k for k, _ in left], [o for _, o in left])
    if new_key is not None:
        model.insert([new_key], [obj])
