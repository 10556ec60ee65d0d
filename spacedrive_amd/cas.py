"""Host-side mirror of the reference's content-identification interface, over the C ABI.

Reference (annihilatorrrr/spacedrive, Rust) → here:

* ``generate_cas_id(path, size) -> String``        core/src/object/cas.rs:23-62
  → :func:`generate_cas_id` (a one-file batch) and :meth:`CasEngine.generate_cas_ids`
  (the batched drop-in the north star asks for: ``generate_cas_ids(&[(buf, size)])``).
* ``file_checksum(path) -> String``                  core/src/object/validation/hash.rs:11-25
  → :func:`file_checksum`.
* ``FileMetadata::new`` + ``identifier_job_step``    core/src/object/file_identifier/mod.rs:55-350
  → :func:`identifier_job_step` (cas_ids, Object links, ``(total_created, total_linked)``).

Errors follow the reference: an I/O failure on one file is an ``OSError`` for the
single-file call (``io::Error`` in Rust) and a per-file drop in the batch
(mod.rs:125-141); a GPU failure is a batch-level :class:`CasError`.

Device arrays are torch tensors used as plain HBM buffers (u64 values are stored in
int64 tensors bit-for-bit); all computation happens in libsd_hip_cas.so.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _native
from ._native import CasError

# core/src/object/cas.rs:10-15 and file_identifier/mod.rs:34
SAMPLE_COUNT = 4
SAMPLE_SIZE = 1024 * 10
HEADER_OR_FOOTER_SIZE = 1024 * 8
MINIMUM_FILE_SIZE = 1024 * 100
SAMPLED_CONTENT_LEN = 2 * HEADER_OR_FOOTER_SIZE + SAMPLE_COUNT * SAMPLE_SIZE  # 57,344
CHUNK_SIZE = 100
MAX_PACKED_CONTENT_LEN = 104 * 1024 - 8
THRESHOLD_DEFAULT = (1 << 64) - 1  # SD_CAS_THRESHOLD_DEFAULT
NO_OBJECT = NO_STEP = 0xFFFFFFFF   # SD_CAS_NO_OBJECT / SD_CAS_NO_STEP
# SD_CAS_STAT_* in index order (the keys of the totals dicts), SD_CAS_TOP_MAX, and the tile of
# the top list's stable compaction (object_stats.hip: TOP_THREADS x TOP_ITEMS rows)
STAT_NAMES = ("rows", "objects", "total_bytes", "unique_bytes", "duplicate_sets", "max_copies",
              "size_mismatch_rows", "bad_rows")
TOP_MAX = 65536
TOP_TILE = 16384
EXACT_AUTO, EXACT_WORDS = 0, 1  # SD_CAS_EXACT_*
EXACT_COMPARE_ROUNDS_DEFAULT = 3  # SD_CAS_EXACT_COMPARE_ROUNDS_DEFAULT


def key_to_cas_id(key: int) -> str:
    """cas.rs:61 ``hasher.finalize().to_hex()[..16]`` from the big-endian u64 key."""
    return f"{int(key) & 0xFFFFFFFFFFFFFFFF:016x}"


def cas_id_to_key(cas_id: str) -> int:
    return int(cas_id, 16)


def digest_from_hex(hex_digest: str) -> bytes:
    """sd_cas_digest_from_hex: the 32 bytes of a checksum string (file_checksum's result,
    Hash::to_hex of hash.rs:24) — exactly 64 hex digits of either case, else ValueError."""
    raw = hex_digest.encode() if isinstance(hex_digest, str) else bytes(hex_digest)
    out = ctypes.create_string_buffer(32)
    if b"\0" in raw or _native.lib().sd_cas_digest_from_hex(raw, ctypes.addressof(out)) != 0:
        raise ValueError(f"not a 64-hex-digit checksum: {hex_digest!r}")
    return out.raw


def digest_to_hex(digest: bytes) -> str:
    """sd_cas_digest_to_hex: 64 lowercase hex digits of a 32-byte digest."""
    d = bytes(digest)
    if len(d) != 32:
        raise ValueError(f"a digest has 32 bytes, got {len(d)}")
    src, out = ctypes.create_string_buffer(d, 32), ctypes.create_string_buffer(65)
    _native.lib().sd_cas_digest_to_hex(ctypes.addressof(src), out)
    return out.value.decode()


def _ptr(t) -> int:
    return int(t.data_ptr())


def _stream(stream: Optional[int]) -> int:
    """Device calls default to torch's current stream so they order with tensor ops."""
    if stream is not None:
        return stream
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def _np_ptr(a: np.ndarray) -> int:
    return int(a.ctypes.data)


def _sizes_u64(sizes, what: str = "sizes") -> np.ndarray:
    """File sizes (fs::metadata lengths) as the u64 column of the ABI.  A signed array is
    checked first: a negative size (e.g. a -1 'stat failed' marker) would otherwise wrap to
    2^64 - 1 and be hashed as a huge sampled file."""
    a = np.asarray(sizes) if isinstance(sizes, np.ndarray) else np.array([int(x) for x in sizes])
    if a.size and a.dtype.kind == "i" and int(a.min()) < 0:
        raise ValueError(f"{what}: negative size {int(a.min())}")
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"{what}: integer sizes expected, got {a.dtype}")
    return np.ascontiguousarray(a, dtype=np.uint64)


def _check_dev(t, dtypes, n: int, what: str) -> None:
    """A device tensor handed to a *_dev call: one of `dtypes`, n elements, contiguous, on a
    GPU — checked before the library reads it as raw memory."""
    if t.dtype not in dtypes or t.numel() != n or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{what}: expected a contiguous CUDA tensor of {n} x "
                         f"{'/'.join(str(d) for d in dtypes)}, got {tuple(t.shape)} {t.dtype} "
                         f"on {t.device}")


def _object_ids(ids, what: str, none_ok: bool) -> np.ndarray:
    """Object ids as the u32 column of the link emission: each in [0, 2^31) (the seeded
    grouping's row tag is bit 31); none_ok: -1 / None / 0xFFFFFFFF = no Object."""
    a = np.asarray([NO_OBJECT if x is None else x for x in ids] if not isinstance(ids, np.ndarray)
                   else ids)
    if a.size == 0:
        return np.zeros(0, dtype=np.uint32)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what}: integer Object ids expected, got {a.dtype}")
    a = a.astype(np.int64)
    none = (a == -1) | (a == NO_OBJECT)
    bad = ~none & ((a < 0) | (a >= 1 << 31)) if none_ok else (a < 0) | (a >= 1 << 31)
    if bad.any():
        raise ValueError(f"{what}: Object id {int(a[bad][0])} outside [0, 2^31)")
    return np.ascontiguousarray(np.where(none, NO_OBJECT, a).astype(np.uint32))


def _path_array(paths: Sequence) -> tuple[object, int]:
    """The `const char* const* paths` argument of the batch path calls: (keep-alive, address).
    ASCII str paths (the common case) are encoded in one join and their pointers computed
    by numpy: ~20 us per 100 paths instead of ~90 us for one bytes object and one
    c_char_p each, which was a third of a 100-file job step's Python overhead.  Anything
    else (bytes, PathLike, non-ASCII names) takes the per-path encoding."""
    n = len(paths)
    if n and all(type(p) is str for p in paths):
        joined = "\0".join(paths) + "\0"
        buf = os.fsencode(joined)
        if len(buf) == len(joined) and joined.count("\0") == n:  # ASCII, no embedded NUL
            lens = np.fromiter(map(len, paths), dtype=np.uint64, count=n) + np.uint64(1)
            ptrs = np.empty(n, dtype=np.uint64)
            ptrs[0] = 0
            np.cumsum(lens[:-1], out=ptrs[1:])
            cbuf = ctypes.c_char_p(buf)
            ptrs += np.uint64(ctypes.cast(cbuf, ctypes.c_void_p).value)
            return (buf, cbuf, ptrs), _np_ptr(ptrs)
    parr = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
    return parr, ctypes.cast(parr, ctypes.c_void_p).value


@dataclass
class DuplicateReport:
    """sd_cas_duplicate_report: rep / copies per row in the caller's numbering (NO_OBJECT / 0
    on rows that are not hashed), the totals keyed by STAT_NAMES, and the top list (k entries,
    (NO_OBJECT, 0) past the sets found)."""
    rep: np.ndarray
    copies: np.ndarray
    totals: dict
    top_heads: np.ndarray
    top_waste: np.ndarray


@dataclass
class ExactDuplicateReport:
    """sd_cas_duplicate_report_exact: rep / totals exactly as duplicate_report gives them (sets
    of one cas_id); rep_exact / copies_exact / totals_exact / the top list over the sets whose
    whole-content checksums agree as well (NO_OBJECT / 0 on rows that are not hashed or have no
    checksum); unconfirmed = hashed rows without a checksum."""
    rep: np.ndarray
    rep_exact: np.ndarray
    copies_exact: np.ndarray
    totals: dict
    totals_exact: dict
    unconfirmed: int
    top_heads: np.ndarray
    top_waste: np.ndarray


@dataclass
class ComparedDuplicateReport(ExactDuplicateReport):
    """CasEngine.exact_duplicates_compared: ExactDuplicateReport's fields, the exact ones found
    by comparing the members of each sampled set with each other (unconfirmed = candidates
    whose read failed or whose length changed since the stat), plus what the route read:
    candidate_rows / candidate_bytes = the hashed rows with a sampled copy and their sizes (no
    other file's whole content is opened), compared_rows = the rows that went through
    group_exact_contents, checksum_rows = the rows of sets too large for one arena, which took
    file_checksums and the digest split."""
    candidate_rows: int = 0
    candidate_bytes: int = 0
    compared_rows: int = 0
    checksum_rows: int = 0


class CasEngine:
    """One context on one gfx950 device (one per thread/device, like the C ABI)."""

    def __init__(self, device: int = 0):
        self.L = _native.lib()
        h = ctypes.c_void_p()
        rc = self.L.sd_cas_ctx_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise CasError(rc, f"sd_cas_ctx_create(device={device}) failed "
                               "(needs a gfx950 / MI355X device)")
        self.h = h
        self.device = device

    def close(self) -> None:
        if getattr(self, "h", None):
            self.L.sd_cas_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- helpers --------------------------------------------------------------------
    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            msg = self.L.sd_cas_last_error(self.h)
            raise CasError(rc, f"{what}: {msg.decode() if msg else ''}")

    @property
    def stream(self) -> int:
        return int(self.L.sd_cas_ctx_stream(self.h) or 0)

    def synchronize(self) -> None:
        self._check(self.L.sd_cas_synchronize(self.h), "synchronize")

    @property
    def batch_quantum(self) -> int:
        return int(self.L.sd_cas_batch_quantum(self.h))

    def set_latency_threshold(self, sampled: Optional[int] = None, packed: Optional[int] = None) -> None:
        """Batches below these sizes hash chunk-parallel (K1L); 0 = always one file per lane,
        None = the measured default crossover."""
        d = THRESHOLD_DEFAULT
        self.L.sd_cas_set_latency_threshold(self.h, d if sampled is None else int(sampled),
                                            d if packed is None else int(packed))

    def set_chunkpar_split(self, sampled: Optional[int] = None, packed: Optional[int] = None) -> None:
        """K1L batches of at least this many files pack 4 files per wave (16-lane segments);
        smaller ones use a wave per file.  0 = always 4 per wave, None = measured default."""
        d = THRESHOLD_DEFAULT
        self.L.sd_cas_set_chunkpar_split(self.h, d if sampled is None else int(sampled),
                                         d if packed is None else int(packed))

    GROUP_AUTO, GROUP_HASH, GROUP_SORT = 0, 1, 2

    def set_group_method(self, method: int = 0, bucket_target: int = 0) -> None:
        """Grouping method (GROUP_AUTO / GROUP_HASH / GROUP_SORT) and the hash grouping's
        mean keys per bucket (0 = tuned default); identical results for every setting."""
        self._check(self.L.sd_cas_set_group_method(self.h, int(method), int(bucket_target)),
                    "set_group_method")

    # ---- host batches (blocking) -------------------------------------------------------
    def generate_cas_keys(self, items: Sequence[tuple[bytes, int]]) -> np.ndarray:
        """Batched ``generate_cas_id`` over already-gathered content: items = (buf, size)."""
        n = len(items)
        if n == 0:
            return np.zeros(0, dtype=np.uint64)
        bufs = [bytes(b) for b, _ in items]
        ptrs = (ctypes.c_char_p * n)(*bufs)
        lens = np.array([len(b) for b in bufs], dtype=np.uint64)
        sizes = np.array([int(s) for _, s in items], dtype=np.uint64)
        keys = np.zeros(n, dtype=np.uint64)
        rc = self.L.sd_cas_generate_cas_ids(self.h, ctypes.cast(ptrs, ctypes.c_void_p),
                                            _np_ptr(lens), _np_ptr(sizes), n, _np_ptr(keys))
        self._check(rc, "generate_cas_ids")
        return keys

    def generate_cas_ids(self, items: Sequence[tuple[bytes, int]]) -> list[str]:
        return [key_to_cas_id(k) for k in self.generate_cas_keys(items)]

    def generate_cas_keys_from_paths(self, paths: Sequence[str], sizes: Optional[Sequence[int]] = None):
        """The cas part of FileMetadata::new (file_identifier/mod.rs:55-95) over a batch:
        gather (pread at the cas.rs:27-58 offsets) + hash.  sizes = fs::metadata lengths, or
        None to let the library take the metadata (stat).  Returns (keys, status): status 0 =
        hashed, STATUS_NO_CAS = length 0 (no cas_id, key 0), -errno = error (EISDIR for a
        directory)."""
        n = len(paths)
        keep, parr = _path_array(paths)
        sz = None
        if sizes is not None:
            sz = _sizes_u64(sizes)
            if sz.shape != (n,):
                raise ValueError(f"sizes has shape {sz.shape}, expected ({n},)")
        keys = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        if n:
            rc = self.L.sd_cas_generate_cas_ids_from_paths(
                self.h, parr, None if sz is None else _np_ptr(sz), n,
                _np_ptr(keys), _np_ptr(status))
            self._check(rc, "generate_cas_ids_from_paths")
        return keys, status

    def file_metadata_from_paths(self, paths: Sequence[str]):
        """FileMetadata::new over a batch (mod.rs:55-95), metadata taken by the library:
        (keys, status, sizes) — sizes = the fs::metadata length each row was decided from
        (sd_cas_file_metadata_from_paths: one stat per path)."""
        n = len(paths)
        keep, parr = _path_array(paths)
        keys = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        sizes = np.zeros(n, dtype=np.uint64)
        if n:
            self._check(self.L.sd_cas_file_metadata_from_paths(
                self.h, parr, n, _np_ptr(keys), _np_ptr(status),
                _np_ptr(sizes)), "file_metadata_from_paths")
        return keys, status, sizes

    def alloc_pinned(self, nbytes: int) -> np.ndarray:
        """Page-locked host buffer (uint8 numpy view); free with free_pinned."""
        p = ctypes.c_void_p()
        self._check(self.L.sd_cas_alloc_pinned(self.h, int(nbytes), ctypes.byref(p)), "alloc_pinned")
        buf = (ctypes.c_uint8 * int(nbytes)).from_address(p.value)
        return np.frombuffer(buf, dtype=np.uint8)

    def free_pinned(self, arr: np.ndarray) -> None:
        self._check(self.L.sd_cas_free_pinned(self.h, int(arr.ctypes.data)), "free_pinned")

    def hash_sampled_host(self, content: np.ndarray, sizes: np.ndarray, stride: int = SAMPLED_CONTENT_LEN,
                          batch_files: int = 0) -> np.ndarray:
        """End-to-end K1 from host memory (H2D pipelined with hashing)."""
        n = len(sizes)
        sz = _sizes_u64(sizes)
        keys = np.zeros(n, dtype=np.uint64)
        self._check(self.L.sd_cas_hash_sampled_host(self.h, int(content.ctypes.data), int(stride),
                                                    _np_ptr(sz), n, _np_ptr(keys), int(batch_files)),
                    "hash_sampled_host")
        return keys

    def hash_sampled_host_ring(self, ring_ptr: int, ring_files: int, sizes: np.ndarray,
                               stride: int = SAMPLED_CONTENT_LEN, batch_files: int = 0) -> np.ndarray:
        """End-to-end K1 over len(sizes) files whose contents cycle through a host ring of
        ring_files x stride bytes at ring_ptr (every file is copied host -> device)."""
        n = len(sizes)
        sz = _sizes_u64(sizes)
        keys = np.zeros(n, dtype=np.uint64)
        self._check(self.L.sd_cas_hash_sampled_host_ring(self.h, int(ring_ptr), int(stride),
                                                         int(ring_files), _np_ptr(sz), n,
                                                         _np_ptr(keys), int(batch_files)),
                    "hash_sampled_host_ring")
        return keys

    def file_checksum(self, path: str) -> str:
        out = ctypes.create_string_buffer(65)
        err = ctypes.c_int(0)
        rc = self.L.sd_cas_file_checksum(self.h, os.fsencode(path), out, ctypes.byref(err))
        if rc == -3 and err.value:
            raise OSError(err.value, os.strerror(err.value), path)
        self._check(rc, "file_checksum")
        return out.value.decode()

    def file_checksums(self, paths: Sequence[str]) -> tuple[list[Optional[str]], np.ndarray]:
        """The validator job over many files (validator_job.rs:107-172, one file_checksum
        per step, hash.rs:11-25) in one call: returns (64-hex digest or None per path, errno
        array — 0, or the errno of the failed open/stat/read)."""
        n = len(paths)
        keep, parr = _path_array(paths)
        out = ctypes.create_string_buffer(65 * max(n, 1))
        status = np.zeros(n, dtype=np.int32)
        if n:
            self._check(self.L.sd_cas_file_checksums(self.h, parr, n,
                                                     out, _np_ptr(status)), "file_checksums")
        # one numpy conversion of the fixed 65-byte records (64 hex + NUL): ~2x faster than a
        # slice + decode per path, which cost ~10 ms per 20,000 paths
        digests = np.frombuffer(out, dtype="S65", count=n).astype("U64").tolist() if n else []
        for i in np.flatnonzero(status).tolist():
            digests[i] = None
        return digests, -status

    def identify_validate(self, paths: Sequence[str]):
        """Both columns of a file_path row from one read (and one stat) per file
        (sd_cas_identify_validate_paths): returns (keys, cas_status, sizes, digests, errnos) —
        the first three exactly as file_metadata_from_paths, the last two as file_checksums."""
        n = len(paths)
        keep, parr = _path_array(paths)
        keys = np.zeros(n, dtype=np.uint64)
        cas_status = np.zeros(n, dtype=np.int32)
        sizes = np.zeros(n, dtype=np.uint64)
        out = ctypes.create_string_buffer(65 * max(n, 1))
        status = np.zeros(n, dtype=np.int32)
        if n:
            self._check(self.L.sd_cas_identify_validate_paths(
                self.h, parr, n, _np_ptr(keys), _np_ptr(cas_status), _np_ptr(sizes), out,
                _np_ptr(status)), "identify_validate_paths")
        digests = np.frombuffer(out, dtype="S65", count=n).astype("U64").tolist() if n else []
        for i in np.flatnonzero(status).tolist():
            digests[i] = None
        return keys, cas_status, sizes, digests, -status

    # ---- device-resident (torch tensors as HBM buffers) ----------------------------------
    def hash_sampled(self, content, sizes, keys, stride: Optional[int] = None,
                     n: Optional[int] = None, stream: Optional[int] = None) -> None:
        """K1: content uint8 [n, stride] (or flat), sizes/keys int64 [n]."""
        n = int(sizes.numel()) if n is None else n
        stride = int(content.shape[-1]) if stride is None and content.dim() == 2 else stride
        self._check(self.L.sd_cas_hash_sampled_dev(self.h, _ptr(content), int(stride), _ptr(sizes),
                                                   n, _ptr(keys), _stream(stream)), "hash_sampled")

    def hash_packed(self, arena, offs, lens, sizes, keys, stream: Optional[int] = None) -> None:
        n = int(sizes.numel())
        self._check(self.L.sd_cas_hash_packed_dev(self.h, _ptr(arena), _ptr(offs), _ptr(lens),
                                                  _ptr(sizes), n, _ptr(keys), _stream(stream)),
                    "hash_packed")

    def group(self, keys, rep, stream: Optional[int] = None, want_objects: bool = True) -> Optional[int]:
        n = int(keys.numel())
        obj = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_group_dev(self.h, _ptr(keys), n, _ptr(rep),
                                            ctypes.byref(obj) if want_objects else None, _stream(stream)),
                    "group")
        return int(obj.value) if want_objects else None

    def hash_group_sampled(self, content, sizes, keys, rep, overflow, stream: Optional[int] = None,
                           want_objects: bool = True) -> Optional[int]:
        """K1 with the grouping partition fused into its epilogue + one bucket-table launch
        (sd_cas_hash_group_sampled_dev): keys as hash_sampled, rep as group.  overflow: int32
        [1] device tensor, zeroed by the caller — set if a coarse bucket outgrew its region
        (the result is exact either way: that region is regrouped on the device from the
        whole key array); want_objects blocks and returns the Object count."""
        n = int(sizes.numel())
        stride = int(content.shape[-1]) if content.dim() == 2 else SAMPLED_CONTENT_LEN
        obj = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_hash_group_sampled_dev(
            self.h, _ptr(content), stride, _ptr(sizes), n, _ptr(keys), _ptr(rep), _ptr(overflow),
            ctypes.byref(obj) if want_objects else None, _stream(stream)), "hash_group_sampled")
        return int(obj.value) if want_objects else None

    def hash_regions_sampled(self, content, sizes, keys, rep, overflow,
                             stream: Optional[int] = None) -> None:
        """The first half of hash_group_sampled: K1G into the next region set (async)."""
        n = int(sizes.numel())
        stride = int(content.shape[-1]) if content.dim() == 2 else SAMPLED_CONTENT_LEN
        self._check(self.L.sd_cas_hash_regions_sampled_dev(
            self.h, _ptr(content), stride, _ptr(sizes), n, _ptr(keys), _ptr(rep), _ptr(overflow),
            _stream(stream)), "hash_regions_sampled")

    def group_regions(self, n: int, rep, stream: Optional[int] = None,
                      want_objects: bool = True) -> Optional[int]:
        """The second half: the bucket tables over the last hash_regions batch."""
        obj = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_group_regions_dev(self.h, int(n), _ptr(rep),
                                                    ctypes.byref(obj) if want_objects else None,
                                                    _stream(stream)), "group_regions")
        return int(obj.value) if want_objects else None

    def set_dup_verify(self, on: bool = True) -> None:
        """The fused chain compares a duplicate candidate's 57,344 bytes with the earlier file's
        instead of hashing them (default on; identical results either way, off = plain K1G)."""
        self._check(self.L.sd_cas_set_dup_verify(self.h, 1 if on else 0), "set_dup_verify")

    def dup_verify_counters(self) -> tuple[int, int, int]:
        """(candidates, verified, rehashed) of the last hash_regions_sampled /
        hash_group_sampled call (blocks; zeros when that call did not verify duplicates)."""
        c, v, r = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.L.sd_cas_dup_verify_counters(self.h, ctypes.byref(c), ctypes.byref(v),
                                                      ctypes.byref(r)), "dup_verify_counters")
        return int(c.value), int(v.value), int(r.value)

    def dup_verify_rows(self) -> tuple[int, int, int]:
        """(groups, tasks, references) of the same call: the comparison read every candidate's
        row once and an earlier file's row `references` times (blocks; zeros as above)."""
        g, t, r = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.L.sd_cas_dup_verify_rows(self.h, ctypes.byref(g), ctypes.byref(t),
                                                  ctypes.byref(r)), "dup_verify_rows")
        return int(g.value), int(t.value), int(r.value)

    def group_min(self, keys, vals, out, stream: Optional[int] = None,
                  want_objects: bool = True) -> Optional[int]:
        """out[i] = min{ vals[j] : keys[j] == keys[i] } (vals None = identity)."""
        n = int(keys.numel())
        obj = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_group_min_dev(
            self.h, _ptr(keys), _ptr(vals) if vals is not None else None, n, _ptr(out),
            ctypes.byref(obj) if want_objects else None, _stream(stream)), "group_min")
        return int(obj.value) if want_objects else None

    def exchange_pack(self, keys, pos, file0: int, rows, stream: Optional[int] = None) -> None:
        """rows int32 [n, 3] = (key lo, key hi, u32(file0 + pos)) for the RCCL exchange."""
        self._check(self.L.sd_cas_exchange_pack_dev(self.h, _ptr(keys), _ptr(pos), int(keys.numel()),
                                                    int(file0), _ptr(rows), _stream(stream)),
                    "exchange_pack")

    def exchange_split(self, rows, keys, vals, stream: Optional[int] = None) -> None:
        self._check(self.L.sd_cas_exchange_split_dev(self.h, _ptr(rows), int(keys.numel()), _ptr(keys),
                                                     _ptr(vals), _stream(stream)), "exchange_split")

    def exchange_unpack(self, back, pos, rep, stream: Optional[int] = None) -> None:
        self._check(self.L.sd_cas_exchange_unpack_dev(self.h, _ptr(back), _ptr(pos), int(back.numel()),
                                                      _ptr(rep), _stream(stream)), "exchange_unpack")

    def partition(self, keys, parts: int, keys_out, pos_out, counts, stream: Optional[int] = None) -> None:
        """Key-range partition part(k) = floor(k * parts / 2^64), part-contiguous output."""
        n = int(keys.numel())
        self._check(self.L.sd_cas_partition_dev(self.h, _ptr(keys), n, int(parts), _ptr(keys_out),
                                                _ptr(pos_out), _ptr(counts), _stream(stream)),
                    "partition")

    def group_sorted(self, skeys, svals, rep, stream: Optional[int] = None) -> int:
        n = int(skeys.numel())
        obj = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_group_sorted_dev(self.h, _ptr(skeys), _ptr(svals), n, _ptr(rep),
                                                   ctypes.byref(obj), _stream(stream)), "group_sorted")
        return int(obj.value)

    def group_chunked(self, rep, rep_chunked, chunk: int = CHUNK_SIZE,
                      stream: Optional[int] = None) -> tuple[int, int]:
        n = int(rep.numel())
        c = ctypes.c_uint64(0)
        ln = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_group_chunked_dev(self.h, _ptr(rep), n, int(chunk),
                                                     _ptr(rep_chunked), ctypes.byref(c),
                                                     ctypes.byref(ln), _stream(stream)), "group_chunked")
        return int(c.value), int(ln.value)

    def identifier_links(self, keys, state=None, chunk: int = CHUNK_SIZE,
                         stream: Optional[int] = None, existing=None, pre_objects=None, out=None,
                         index: Optional["ObjectIndex"] = None):
        """Object-link emission of one file-identifier job over the rows (ascending
        file_path.id) — sd_cas_identifier_links_ex_dev: returns (step, object, action)
        device tensors (int32, int32, uint8) and the per-step (created, linked) counts as an
        int64 numpy array [steps, 2].  state: uint8 ROW_* per row (None = all hashed).
        existing: None (a fresh library) or (seed_keys int64/uint64, seed_objects int32)
        device tensors — the Objects the library holds before the job, as (cas key, Object id)
        pairs (mod.rs:180-198); a row whose key one carries links to the smallest such id
        (action LINK_EXISTING).  pre_objects: None or an int32 device tensor, per row the
        Object its file_path already holds (object_id set, cas_id NULL:
        file_identifier_job.rs:258-261) or -1 (= SD_CAS_NO_OBJECT) — see
        sd_cas_identifier_links_ex_dev.  Ids must be < 2^31 (checked by the library).
        index: an ObjectIndex of this engine in place of `existing` (not both): the library's
        Objects are read from it — sd_cas_identifier_links_indexed_dev, the same decisions as
        existing = index.export() at a cost independent of the library's size.
        out: None or the caller's (step, object, action) tensors to write into."""
        import torch
        if index is not None and existing is not None:
            raise ValueError("identifier_links: existing= and index= exclude each other")
        n = int(keys.numel())
        _check_dev(keys, (torch.int64, torch.uint64), n, "keys")
        if state is not None:
            _check_dev(state, (torch.uint8,), n, "state")
        dev = keys.device
        if out is not None:
            step, obj, act = out
            _check_dev(step, (torch.int32, torch.uint32), n, "out step")
            _check_dev(obj, (torch.int32, torch.uint32), n, "out object")
            _check_dev(act, (torch.uint8,), n, "out action")
        else:
            step = torch.empty(n, dtype=torch.int32, device=dev)
            obj = torch.empty(n, dtype=torch.int32, device=dev)
            act = torch.empty(n, dtype=torch.uint8, device=dev)
        ms = int(self.L.sd_cas_identifier_max_steps(n, int(chunk)))
        counts = np.zeros(2 * max(ms, 1), dtype=np.uint64)
        steps = ctypes.c_uint64(0)
        sk, so = existing if existing is not None else (None, None)
        ns = 0 if sk is None else int(sk.numel())
        if ns:
            _check_dev(sk, (torch.int64, torch.uint64), ns, "existing keys")
            _check_dev(so, (torch.int32, torch.uint32), ns, "existing Object ids")
        if pre_objects is not None:
            _check_dev(pre_objects, (torch.int32, torch.uint32), n, "pre_objects")
        if index is not None:
            self._check(self.L.sd_cas_identifier_links_indexed_dev(
                self.h, _ptr(keys), _ptr(state) if state is not None else None, n, int(chunk),
                index._handle(self), _ptr(pre_objects) if pre_objects is not None else None,
                _ptr(step), _ptr(obj), _ptr(act), _np_ptr(counts), ms, ctypes.byref(steps),
                _stream(stream)), "identifier_links")
            k = int(steps.value)
            return step, obj, act, counts[:2 * k].reshape(k, 2).astype(np.int64)
        self._check(self.L.sd_cas_identifier_links_ex_dev(
            self.h, _ptr(keys), _ptr(state) if state is not None else None, n, int(chunk),
            _ptr(sk) if ns else None, _ptr(so) if ns else None, ns,
            _ptr(pre_objects) if pre_objects is not None else None,
            _ptr(step), _ptr(obj), _ptr(act), _np_ptr(counts), ms, ctypes.byref(steps),
            _stream(stream)), "identifier_links")
        k = int(steps.value)
        return step, obj, act, counts[:2 * k].reshape(k, 2).astype(np.int64)

    def identifier_links_host(self, keys: np.ndarray, state: Optional[np.ndarray] = None,
                              chunk: int = CHUNK_SIZE, existing=None, pre_objects=None,
                              index: Optional["ObjectIndex"] = None):
        """sd_cas_identifier_links_ex (host arrays): (step u32, object u32, action u8,
        counts int64 [steps, 2]) — the DB layer's view of the same emission.  existing: None
        or (seed_keys, seed_objects) numpy arrays; pre_objects: None or per-row Object ids
        (NO_OBJECT / -1 = none); index: an ObjectIndex in place of `existing` (not both,
        sd_cas_identifier_links_indexed) — see identifier_links."""
        if index is not None and existing is not None:
            raise ValueError("identifier_links_host: existing= and index= exclude each other")
        n = len(keys)
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        st = None if state is None else np.ascontiguousarray(state, dtype=np.uint8)
        step = np.zeros(n, dtype=np.uint32)
        obj = np.zeros(n, dtype=np.uint32)
        act = np.zeros(n, dtype=np.uint8)
        ms = int(self.L.sd_cas_identifier_max_steps(n, int(chunk)))
        counts = np.zeros(2 * max(ms, 1), dtype=np.uint64)
        steps = ctypes.c_uint64(0)
        if existing is not None:
            sk = np.ascontiguousarray(existing[0], dtype=np.uint64)
            so = _object_ids(existing[1], "existing Object ids", none_ok=False)
            if len(sk) != len(so):
                raise ValueError("existing: as many Object ids as cas keys")
        else:
            sk = so = np.zeros(0, dtype=np.uint64)
        ns = len(sk)
        po = None
        if pre_objects is not None:
            po = _object_ids(pre_objects, "pre_objects", none_ok=True)
            if po.shape != (n,):
                raise ValueError(f"pre_objects has shape {po.shape}, expected ({n},)")
        if index is not None:
            self._check(self.L.sd_cas_identifier_links_indexed(
                self.h, _np_ptr(k), _np_ptr(st) if st is not None else None, n, int(chunk),
                index._handle(self), _np_ptr(po) if po is not None else None,
                _np_ptr(step), _np_ptr(obj), _np_ptr(act), _np_ptr(counts), ms, ctypes.byref(steps)),
                "identifier_links")
            s = int(steps.value)
            return step, obj, act, counts[:2 * s].reshape(s, 2).astype(np.int64)
        self._check(self.L.sd_cas_identifier_links_ex(
            self.h, _np_ptr(k), _np_ptr(st) if st is not None else None, n, int(chunk),
            _np_ptr(sk) if ns else None, _np_ptr(so) if ns else None, ns,
            _np_ptr(po) if po is not None else None,
            _np_ptr(step), _np_ptr(obj), _np_ptr(act), _np_ptr(counts), ms, ctypes.byref(steps)),
            "identifier_links")
        s = int(steps.value)
        return step, obj, act, counts[:2 * s].reshape(s, 2).astype(np.int64)

    def object_index(self, expected: int = 0) -> "ObjectIndex":
        """A library-resident Object index of this engine (sd_cas_index_create): the library's
        (cas key -> smallest Object id) relation kept in HBM between calls.  expected: the
        entries to size the table for (0 = the minimum; it grows by itself)."""
        return ObjectIndex(self, expected)

    def object_stats(self, rep, sizes, copies, totals=None, stream: Optional[int] = None,
                     want_totals: bool = True) -> Optional[dict]:
        """sd_cas_object_stats_dev: copies[i] (int32 device tensor, accumulator and output) =
        the rows of row i's Object, and the eight totals of a grouping `rep` (as group) with
        the rows' sizes — total_object_count and total_unique_bytes of the reference's
        `statistics` row (statistics.rs:42,46) among them.  totals: None or an int64 [8]
        device tensor.  want_totals blocks and returns the totals keyed by STAT_NAMES (raises
        EINVAL if rep holds bad rows); otherwise the call is asynchronous and returns None."""
        import torch
        n = int(rep.numel())
        _check_dev(rep, (torch.int32, torch.uint32), n, "rep")
        _check_dev(sizes, (torch.int64, torch.uint64), n, "sizes")
        _check_dev(copies, (torch.int32, torch.uint32), n, "copies")
        if totals is not None:
            _check_dev(totals, (torch.int64, torch.uint64), len(STAT_NAMES), "totals")
        out = np.zeros(len(STAT_NAMES), dtype=np.uint64)
        self._check(self.L.sd_cas_object_stats_dev(
            self.h, _ptr(rep), _ptr(sizes), n, _ptr(copies),
            _ptr(totals) if totals is not None else None,
            _np_ptr(out) if want_totals else None, _stream(stream)), "object_stats")
        return {k: int(v) for k, v in zip(STAT_NAMES, out)} if want_totals else None

    def top_duplicates(self, rep, sizes, copies, k: int, heads, waste,
                       stream: Optional[int] = None) -> int:
        """sd_cas_top_duplicates_dev: the min(k, duplicate sets) heads with copies >= 2 by
        waste = (copies - 1) * size descending, ties by head ascending, into heads (int32 [k])
        / waste (int64 [k]) device tensors; the rest is (NO_OBJECT, 0).  Returns the number
        found.  copies as object_stats left it.  Blocking; k <= TOP_MAX."""
        import torch
        n = int(rep.numel())
        k = int(k)
        _check_dev(rep, (torch.int32, torch.uint32), n, "rep")
        _check_dev(sizes, (torch.int64, torch.uint64), n, "sizes")
        _check_dev(copies, (torch.int32, torch.uint32), n, "copies")
        if k <= TOP_MAX:  # a larger k is the library's EINVAL, whatever the arrays hold
            _check_dev(heads, (torch.int32, torch.uint32), k, "heads")
            _check_dev(waste, (torch.int64, torch.uint64), k, "waste")
        found = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_top_duplicates_dev(
            self.h, _ptr(rep), _ptr(sizes), _ptr(copies), n, k, _ptr(heads), _ptr(waste),
            ctypes.byref(found), _stream(stream)), "top_duplicates")
        return int(found.value)

    def duplicate_report(self, keys, sizes, state=None, k: int = 0) -> DuplicateReport:
        """sd_cas_duplicate_report (host arrays, the DB layer's side): grouping, copies,
        totals and the top-k duplicate sets of the HASHED rows (state: ROW_* per row, None =
        all hashed), everything in the caller's row numbering."""
        n = len(keys)
        kk = np.ascontiguousarray(keys, dtype=np.uint64)
        sz = _sizes_u64(sizes)
        if sz.shape != (n,):
            raise ValueError(f"sizes has shape {sz.shape}, expected ({n},)")
        st = None if state is None else np.ascontiguousarray(state, dtype=np.uint8)
        if st is not None and st.shape != (n,):
            raise ValueError(f"state has shape {st.shape}, expected ({n},)")
        k = int(k)
        rep = np.zeros(n, dtype=np.uint32)
        copies = np.zeros(n, dtype=np.uint32)
        totals = np.zeros(len(STAT_NAMES), dtype=np.uint64)
        heads = np.zeros(max(k, 1), dtype=np.uint32)
        waste = np.zeros(max(k, 1), dtype=np.uint64)
        found = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_duplicate_report(
            self.h, _np_ptr(kk), _np_ptr(sz), _np_ptr(st) if st is not None else None, n,
            _np_ptr(rep), _np_ptr(copies), _np_ptr(totals), k, _np_ptr(heads), _np_ptr(waste),
            ctypes.byref(found)), "duplicate_report")
        return DuplicateReport(rep, copies, {q: int(v) for q, v in zip(STAT_NAMES, totals)},
                               heads[:k], waste[:k])

    EXACT_AUTO, EXACT_WORDS = EXACT_AUTO, EXACT_WORDS

    def set_exact_method(self, method: int = EXACT_AUTO) -> None:
        """group_exact's path: EXACT_AUTO = fast key + verify, the word-wise path only on a
        mismatch; EXACT_WORDS = always the word-wise path.  Identical results either way."""
        self._check(self.L.sd_cas_set_exact_method(self.h, int(method)), "set_exact_method")

    def group_exact(self, rep, digests, rep_exact, stream: Optional[int] = None) -> int:
        """sd_cas_group_exact_dev: rep_exact[i] = the first row with row i's rep AND 32-byte
        digest (rep None: the digests alone).  rep / rep_exact int32 [n] device tensors (rep is
        read as a value only), digests uint8 [32 n] (or [n, 32]), 16-B aligned.  Blocking;
        returns the number of distinct (rep, digest) pairs."""
        import torch
        n = int(rep_exact.numel())
        _check_dev(rep_exact, (torch.int32, torch.uint32), n, "rep_exact")
        _check_dev(digests, (torch.uint8,), 32 * n, "digests")
        if rep is not None:
            _check_dev(rep, (torch.int32, torch.uint32), n, "rep")
        obj = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_group_exact_dev(
            self.h, _ptr(rep) if rep is not None else None, _ptr(digests), n, _ptr(rep_exact),
            ctypes.byref(obj), _stream(stream)), "group_exact")
        return int(obj.value)

    def group_exact_counters(self) -> tuple[int, int]:
        """(mismatched_rows, fallbacks) of the last group_exact call: the rows whose fast-path
        head did not match them, and 1 if the word-wise path ran."""
        m, f = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.L.sd_cas_group_exact_counters(self.h, ctypes.byref(m), ctypes.byref(f)),
                    "group_exact_counters")
        return int(m.value), int(f.value)

    def duplicate_report_exact(self, keys, sizes, digests, state=None, k: int = 0) -> ExactDuplicateReport:
        """sd_cas_duplicate_report_exact (host arrays): duplicate_report plus the same over the
        exact sets.  digests: per row the 64-hex checksum string identify_validate /
        file_checksums return, None (or "") = no checksum."""
        n = len(keys)
        kk = np.ascontiguousarray(keys, dtype=np.uint64)
        sz = _sizes_u64(sizes)
        if sz.shape != (n,):
            raise ValueError(f"sizes has shape {sz.shape}, expected ({n},)")
        if len(digests) != n:
            raise ValueError(f"{len(digests)} digests for {n} rows")
        st = None if state is None else np.ascontiguousarray(state, dtype=np.uint8)
        if st is not None and st.shape != (n,):
            raise ValueError(f"state has shape {st.shape}, expected ({n},)")
        hexes = np.zeros(max(n, 1), dtype="S65")
        for i, d in enumerate(digests):
            if d:
                b = d.encode() if isinstance(d, str) else bytes(d)
                if len(b) > 64 or b"\0" in b:  # (a shorter or non-hex one is the library's EINVAL)
                    raise ValueError(f"digests[{i}]: not a 64-hex-digit checksum")
                hexes[i] = b
        k = int(k)
        rep = np.zeros(n, dtype=np.uint32)
        rep_exact = np.zeros(n, dtype=np.uint32)
        copies = np.zeros(n, dtype=np.uint32)
        totals = np.zeros(len(STAT_NAMES), dtype=np.uint64)
        totals_exact = np.zeros(len(STAT_NAMES), dtype=np.uint64)
        heads = np.zeros(max(k, 1), dtype=np.uint32)
        waste = np.zeros(max(k, 1), dtype=np.uint64)
        found, unconfirmed = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.L.sd_cas_duplicate_report_exact(
            self.h, _np_ptr(kk), _np_ptr(sz), _np_ptr(hexes), _np_ptr(st) if st is not None else None, n,
            _np_ptr(rep), _np_ptr(rep_exact), _np_ptr(copies), _np_ptr(totals), _np_ptr(totals_exact),
            ctypes.byref(unconfirmed), k, _np_ptr(heads), _np_ptr(waste), ctypes.byref(found)),
            "duplicate_report_exact")
        return ExactDuplicateReport(rep, rep_exact, copies,
                                    {q: int(v) for q, v in zip(STAT_NAMES, totals)},
                                    {q: int(v) for q, v in zip(STAT_NAMES, totals_exact)},
                                    int(unconfirmed.value), heads[:k], waste[:k])

    def exact_duplicates(self, paths: Sequence[str], k: int = 0) -> ExactDuplicateReport:
        """identify_validate over the paths (one read per file for cas_id and checksum), then
        duplicate_report_exact: a row is HASHED when its cas_id was computed, NO_CAS when the
        file is empty, ERROR otherwise; a hashed row whose checksum failed is unconfirmed."""
        keys, cas_status, sizes, digests, _ = self.identify_validate(paths)
        state = np.where(cas_status == 0, 0, np.where(cas_status == STATUS_NO_CAS, 1, 2)).astype(np.uint8)
        return self.duplicate_report_exact(keys, sizes, digests, state, k)

    def set_exact_compare_rounds(self, max_rounds: Optional[int] = None) -> None:
        """group_exact_contents' round cap: after max_rounds compare rounds the rows still
        unresolved are finished by checksums_dev + group_exact (0 = no cap, None = the library's
        default).  Identical results for every value."""
        if max_rounds is None:
            max_rounds = EXACT_COMPARE_ROUNDS_DEFAULT
        if not 0 <= int(max_rounds) < 1 << 32:
            raise ValueError(f"max_rounds {max_rounds} outside [0, 2^32)")
        self._check(self.L.sd_cas_set_exact_compare_rounds(self.h, int(max_rounds)), "set_exact_compare_rounds")

    def group_exact_contents(self, rep, arena, offs, lens, rep_exact, arena_bytes: Optional[int] = None,
                             stream: Optional[int] = None) -> int:
        """sd_cas_group_exact_contents_dev: rep_exact[i] = the first row with row i's rep (a
        value), length AND bytes, found by comparing contents, not by hashing them.  Content i =
        arena[offs[i] : offs[i] + lens[i]] as for checksums_dev (int64 tensors, 16-B aligned
        offsets, readable to the 16-B round-up); rep / rep_exact int32 [n] device tensors.
        Blocking; returns the number of rows with rep_exact[i] == i.  Raises CasError (EINVAL)
        when a content breaks the bounds; rep_exact is then untouched."""
        import torch
        n = int(rep_exact.numel())
        _check_dev(rep_exact, (torch.int32, torch.uint32), n, "rep_exact")
        _check_dev(rep, (torch.int32, torch.uint32), n, "rep")
        _check_dev(offs, (torch.int64, torch.uint64), n, "offs")
        _check_dev(lens, (torch.int64, torch.uint64), n, "lens")
        if not arena.is_cuda or not arena.is_contiguous():
            raise ValueError("arena: expected a contiguous CUDA tensor")
        ab = int(arena.numel() * arena.element_size()) if arena_bytes is None else int(arena_bytes)
        obj = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_group_exact_contents_dev(
            self.h, _ptr(rep), _ptr(arena), ab, _ptr(offs), _ptr(lens), n, _ptr(rep_exact),
            ctypes.byref(obj), _stream(stream)), "group_exact_contents")
        return int(obj.value)

    def exact_compare_counters(self) -> tuple[int, int, int, int]:
        """(rounds, compares, unequal, digest_rows) of the last group_exact_contents call."""
        v = [ctypes.c_uint64(0) for _ in range(4)]
        self._check(self.L.sd_cas_exact_compare_counters(self.h, *[ctypes.byref(x) for x in v]),
                    "exact_compare_counters")
        return tuple(int(x.value) for x in v)

    def exact_duplicates_compared(self, paths: Sequence[str], k: int = 0,
                                  arena_bytes: Optional[int] = None) -> ComparedDuplicateReport:
        """exact_duplicates without reading what cannot be a duplicate and without digests:
        size, then the sampled cas_id (at most 57,344 B of a file over 100 KiB), then the whole
        content of the CANDIDATES only, the hashed rows whose sampled set has two members, which
        are compared with each other on the device (group_exact_contents).  Every other hashed
        row is its own exact Object and is not opened again.  Whole sets are packed in ascending
        row order into a device arena of at most arena_bytes (default: half of the free device
        memory torch reports at the call, a choice); a set that does not fit takes file_checksums
        and the digest split.  On files that do not change, every field shared with
        exact_duplicates(paths, k) equals that call's."""
        import torch
        from concurrent.futures import ThreadPoolExecutor
        n, k = len(paths), int(k)
        keys, cas_status, sizes = self.file_metadata_from_paths(paths)
        state = np.where(cas_status == 0, 0, np.where(cas_status == STATUS_NO_CAS, 1, 2)).astype(np.uint8)
        sampled = self.duplicate_report(keys, sizes, state, k=0)
        hashed = state == 0
        rows_all = np.arange(n, dtype=np.uint32)
        rep_exact = np.where(hashed, rows_all, np.uint32(NO_OBJECT)).astype(np.uint32)
        unconfirmed = np.zeros(n, dtype=bool)
        cand = np.flatnonzero(hashed & (sampled.copies >= 2))
        if arena_bytes is None:
            arena_bytes = int(torch.cuda.mem_get_info()[0]) // 2 if len(cand) else 0
        arena_bytes = int(arena_bytes)
        room = (sizes.astype(np.int64) + 15) & ~np.int64(15)  # a content's room in the arena
        # the sampled sets in ascending order of their first row; a set's rows ascend as well
        by_set = cand[np.argsort(sampled.rep[cand], kind="stable")]
        cuts = np.flatnonzero(np.diff(sampled.rep[by_set])) + 1
        batches, batch, used, big = [], [], 0, []
        for members in np.split(by_set, cuts) if len(by_set) else []:
            need = int(room[members].sum())
            if need > arena_bytes:
                big.append(members)
                continue
            if used + need > arena_bytes:
                batches.append(batch)
                batch, used = [], 0
            batch.append(members)
            used += need
        if batch:
            batches.append(batch)
        compared_rows = checksum_rows = 0

        def split_on_device(rows, fn):
            """rows ascending; fn(rep, out) runs a grouping over them: back to the caller's numbering"""
            rep_t = torch.from_numpy(sampled.rep[rows].view(np.int32)).cuda()
            out = torch.empty(len(rows), dtype=torch.int32, device="cuda")
            fn(rep_t, out)
            rep_exact[rows] = rows[out.cpu().numpy().view(np.uint32)]

        if batches:
            cap = max(sum(int(room[m].sum()) for m in b) for b in batches)
            staging = self.alloc_pinned(max(cap, 16))
            try:
                with ThreadPoolExecutor(max_workers=16) as pool:  # (never sized by the machine's CPUs)
                    for b in batches:
                        rows = np.sort(np.concatenate(b)).astype(np.uint32)
                        offs = np.concatenate([[0], np.cumsum(room[rows])[:-1]]).astype(np.int64)

                        def read(j):
                            want, at = int(sizes[rows[j]]), int(offs[j])
                            try:
                                with open(paths[rows[j]], "rb", buffering=0) as fh:
                                    got, view = 0, memoryview(staging)[at:at + want]
                                    while got < want:
                                        r = fh.readinto(view[got:])
                                        if not r:
                                            return False
                                        got += r
                                    return fh.read(1) == b""  # still sizes[i] bytes long
                            except OSError:
                                return False
                        ok = np.fromiter(pool.map(read, range(len(rows))), dtype=bool, count=len(rows))
                        unconfirmed[rows[~ok]] = True
                        total = int(room[rows].sum())
                        arena = torch.empty(max(total, 16), dtype=torch.uint8, device="cuda")
                        arena[:total].copy_(torch.from_numpy(staging[:total]))
                        rows, offs = rows[ok], offs[ok]
                        if len(rows):
                            d_offs = torch.from_numpy(offs).cuda()
                            d_lens = torch.from_numpy(sizes[rows].astype(np.int64)).cuda()
                            split_on_device(rows, lambda r, o: self.group_exact_contents(
                                r, arena, d_offs, d_lens, o, arena_bytes=total))
                            compared_rows += len(rows)
                        del arena
            finally:
                self.free_pinned(staging)
        for members in big:  # the route exact_duplicates takes, for these rows alone
            rows = np.sort(members).astype(np.uint32)
            checksum_rows += len(rows)
            digests, _ = self.file_checksums([paths[i] for i in rows])
            ok = np.array([d is not None for d in digests], dtype=bool)
            unconfirmed[rows[~ok]] = True
            rows = rows[ok]
            if len(rows):
                raw = np.frombuffer(b"".join(bytes.fromhex(d) for d in digests if d is not None), dtype=np.uint8)
                d_dig = torch.from_numpy(raw.copy()).cuda()
                split_on_device(rows, lambda r, o: self.group_exact(r, d_dig, o))
        rep_exact[unconfirmed] = NO_OBJECT
        # copies, totals and the top list over the eligible rows, compacted and scattered back
        elig = np.flatnonzero(hashed & ~unconfirmed).astype(np.uint32)
        copies = np.zeros(n, dtype=np.uint32)
        totals_exact = {q: 0 for q in STAT_NAMES}
        heads = np.full(k, NO_OBJECT, dtype=np.uint32)
        waste = np.zeros(k, dtype=np.uint64)
        if len(elig):
            rep_c = torch.from_numpy(np.searchsorted(elig, rep_exact[elig]).astype(np.int32)).cuda()
            sizes_c = torch.from_numpy(sizes[elig].astype(np.int64)).cuda()
            copies_c = torch.zeros(len(elig), dtype=torch.int32, device="cuda")
            totals_exact = self.object_stats(rep_c, sizes_c, copies_c)
            copies[elig] = copies_c.cpu().numpy().view(np.uint32)
            if k:
                d_heads = torch.empty(k, dtype=torch.int32, device="cuda")
                d_waste = torch.empty(k, dtype=torch.int64, device="cuda")
                found = self.top_duplicates(rep_c, sizes_c, copies_c, k, d_heads, d_waste)
                heads[:found] = elig[d_heads.cpu().numpy().view(np.uint32)[:found]]
                waste[:found] = d_waste.cpu().numpy().view(np.uint64)[:found]
        return ComparedDuplicateReport(
            sampled.rep, rep_exact, copies, sampled.totals, totals_exact, int(unconfirmed.sum()), heads, waste,
            candidate_rows=len(cand), candidate_bytes=int(sizes[cand].sum()), compared_rows=compared_rows,
            checksum_rows=checksum_rows)

    def keys_to_hex(self, keys, out, stream: Optional[int] = None) -> None:
        """The cas_id column of a device batch: out (uint8, 16 per key, 16-B aligned)."""
        self._check(self.L.sd_cas_keys_to_hex_dev(self.h, _ptr(keys), keys.numel(), _ptr(out),
                                                  _stream(stream)), "keys_to_hex_dev")

    def thumbnail_paths(self, keys, prefix: str, stride: int, out, stream: Optional[int] = None) -> None:
        """Thumbnail path records of a device batch: out[i*stride ..] = prefix + shard + '/' +
        cas_id + '.webp', NUL-padded (prefix from :func:`thumbnail_dir`)."""
        self._check(self.L.sd_cas_thumbnail_paths_dev(self.h, _ptr(keys), keys.numel(),
                                                      os.fsencode(prefix), stride, _ptr(out),
                                                      _stream(stream)), "thumbnail_paths_dev")

    def sort_pairs(self, keys_in, vals_in, keys_out, vals_out, begin_bit: int = 0,
                   end_bit: int = 64, stream: Optional[int] = None) -> None:
        n = int(keys_in.numel())
        self._check(self.L.sd_cas_sort_pairs_dev(
            self.h, _ptr(keys_in), _ptr(vals_in) if vals_in is not None else None, n,
            _ptr(keys_out), _ptr(vals_out), begin_bit, end_bit, _stream(stream)), "sort_pairs")

    def checksum_dev(self, data, length: Optional[int] = None, stream: Optional[int] = None) -> str:
        length = int(data.numel() * data.element_size()) if length is None else length
        out = ctypes.create_string_buffer(32)
        self._check(self.L.sd_cas_checksum_dev(self.h, _ptr(data), int(length), out, _stream(stream)),
                    "checksum")
        return out.raw.hex()

    def checksums_dev(self, arena, offs, lens, out, arena_bytes: Optional[int] = None,
                      stream: Optional[int] = None) -> None:
        """Digests of many device buffers in one launch chain (sd_cas_checksums_dev): buffer
        i = arena[offs[i] : offs[i] + lens[i]] (int64 tensors, 16-B aligned offsets), out
        uint8 [n, 32]."""
        n = int(offs.numel())
        ab = int(arena.numel() * arena.element_size()) if arena_bytes is None else int(arena_bytes)
        self._check(self.L.sd_cas_checksums_dev(self.h, _ptr(arena), ab, _ptr(offs), _ptr(lens), n,
                                                _ptr(out), _stream(stream)), "checksums_dev")

    def hash_contents(self, arena, offs, lens, keys, arena_bytes: Optional[int] = None,
                      stream: Optional[int] = None) -> None:
        """cas keys of whole file contents where they lie in HBM (sd_cas_hash_contents_dev):
        content i = arena[offs[i] : offs[i] + lens[i]] as for checksums_dev, lens[i] = the
        file's size; files over 100 KiB are hashed straight from their header, samples and
        footer.  keys int64 [n].  Raises CasError (EINVAL) when a buffer breaks the bounds;
        keys is then untouched."""
        n = int(offs.numel())
        ab = int(arena.numel() * arena.element_size()) if arena_bytes is None else int(arena_bytes)
        self._check(self.L.sd_cas_hash_contents_dev(self.h, _ptr(arena), ab, _ptr(offs), _ptr(lens), n,
                                                    _ptr(keys), _stream(stream)), "hash_contents")

    def identify_validate_dev(self, arena, offs, lens, keys, digests,
                              arena_bytes: Optional[int] = None, stream: Optional[int] = None) -> None:
        """hash_contents + checksums_dev over the same buffers with one bounds check: keys
        int64 [n], digests uint8 [n, 32]."""
        n = int(offs.numel())
        ab = int(arena.numel() * arena.element_size()) if arena_bytes is None else int(arena_bytes)
        self._check(self.L.sd_cas_identify_validate_dev(self.h, _ptr(arena), ab, _ptr(offs), _ptr(lens),
                                                        n, _ptr(keys), _ptr(digests), _stream(stream)),
                    "identify_validate_dev")

    def synth_sampled(self, seed: int, file0: int, n: int, content, sizes, stride: int,
                      dup_permille: int = 0, stream: Optional[int] = None) -> None:
        self._check(self.L.sd_cas_synth_sampled_dev(self.h, seed, file0, n, dup_permille,
                                                    _ptr(content), stride, _ptr(sizes), _stream(stream)),
                    "synth_sampled")

    def synth_small(self, seed: int, file0: int, n: int, sizes, lens, offs, arena=None,
                    dup_permille: int = 0, stream: Optional[int] = None) -> int:
        out = ctypes.c_uint64(0)
        self._check(self.L.sd_cas_synth_small_dev(self.h, seed, file0, n, dup_permille,
                                                  _ptr(sizes), _ptr(lens), _ptr(offs),
                                                  _ptr(arena) if arena is not None else None,
                                                  ctypes.byref(out), _stream(stream)), "synth_small")
        return int(out.value)

    def synth_small_content(self, seed: int, file0: int, n: int, offs, lens, arena,
                            dup_permille: int = 0, stream: Optional[int] = None) -> None:
        """Whole-file content at caller-chosen (16-B aligned) offsets."""
        self._check(self.L.sd_cas_synth_small_content_dev(self.h, seed, file0, n, dup_permille,
                                                          _ptr(offs), _ptr(lens), _ptr(arena),
                                                          _stream(stream)), "synth_small_content")

    def synth_stream(self, seed: int, file: int, byte_off: int, length: int, out,
                     stream: Optional[int] = None) -> None:
        """Bytes [byte_off, byte_off + length) of synthetic file `file`'s content stream."""
        self._check(self.L.sd_cas_synth_stream_dev(self.h, seed, file, byte_off, length, _ptr(out),
                                                   _stream(stream)), "synth_stream")

    def synth_roots(self, seed: int, file0: int, n: int, roots, dup_permille: int = 0,
                    stream: Optional[int] = None) -> None:
        self._check(self.L.sd_cas_synth_roots_dev(self.h, seed, file0, n, dup_permille,
                                                  _ptr(roots), _stream(stream)), "synth_roots")


_DEFAULT: dict[int, CasEngine] = {}


INDEX_MAX = 64  # SD_CAS_INDEX_MAX
INDEX_STAT_NAMES = ("entries", "slots", "tombstones", "rehashes", "last_max_probe")  # SD_CAS_INDEX_STAT_*


class ObjectIndex:
    """sd_cas_index_*: the (cas key -> smallest Object id) relation of a library, resident in HBM
    and owned by its CasEngine — the reference's SQLite index on cas_id (find_many by cas_id,
    file_identifier/mod.rs:181-188; the watcher's find_first, watcher/utils.rs:249-257).

    Keys and ids are device tensors (int64/uint64 keys, int32/uint32 ids: the *_dev calls,
    asynchronous on `stream`) or numpy arrays / sequences (the blocking host forms).  The index
    keeps the MINIMUM id per key only: when a file_path is deleted or re-identified, erase its
    key and insert the pairs the DB still holds for that cas_id."""

    def __init__(self, eng: CasEngine, expected: int = 0):
        h = ctypes.c_uint32(0)
        eng._check(eng.L.sd_cas_index_create(eng.h, int(expected), ctypes.byref(h)), "index_create")
        self.eng = eng
        self.handle: Optional[int] = int(h.value)

    def _handle(self, eng: Optional[CasEngine] = None) -> int:
        if self.handle is None:
            raise ValueError("this ObjectIndex is closed")
        if eng is not None and eng is not self.eng:
            raise ValueError("an ObjectIndex belongs to the CasEngine that made it")
        return self.handle

    def close(self) -> None:
        if self.handle is not None and getattr(self.eng, "h", None):
            self.eng._check(self.eng.L.sd_cas_index_destroy(self.eng.h, self.handle), "index_destroy")
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def _is_dev(a) -> bool:
        return hasattr(a, "data_ptr")

    @staticmethod
    def _host_keys(keys) -> np.ndarray:
        if isinstance(keys, np.ndarray) and keys.dtype == np.int64:
            keys = keys.view(np.uint64)
        return np.ascontiguousarray(keys, dtype=np.uint64)

    def insert(self, keys, objects, stream: Optional[int] = None) -> None:
        """index[key] = min(what it held, every id given for key here).  An id outside
        [0, 2^31) refuses the whole batch (CasError EINVAL / ValueError) and inserts nothing."""
        e, L = self.eng, self.eng.L
        if self._is_dev(keys):
            import torch
            n = int(keys.numel())
            _check_dev(keys, (torch.int64, torch.uint64), n, "keys")
            _check_dev(objects, (torch.int32, torch.uint32), n, "objects")
            e._check(L.sd_cas_index_insert_dev(e.h, self._handle(), _ptr(keys) if n else None,
                                               _ptr(objects) if n else None, n, _stream(stream)),
                     "index_insert")
            return
        k = self._host_keys(keys)
        o = _object_ids(objects, "objects", none_ok=False)
        if len(k) != len(o):
            raise ValueError("insert: as many Object ids as keys")
        e._check(L.sd_cas_index_insert(e.h, self._handle(), _np_ptr(k) if len(k) else None,
                                       _np_ptr(o) if len(k) else None, len(k)), "index_insert")

    def lookup(self, keys, out=None, stream: Optional[int] = None):
        """The id of every key, NO_OBJECT where the index has none: an int32 device tensor for
        device keys (`out` to write into one of the caller's), a uint32 numpy array otherwise."""
        e, L = self.eng, self.eng.L
        if self._is_dev(keys):
            import torch
            n = int(keys.numel())
            _check_dev(keys, (torch.int64, torch.uint64), n, "keys")
            if out is None:
                out = torch.empty(n, dtype=torch.int32, device=keys.device)
            _check_dev(out, (torch.int32, torch.uint32), n, "out")
            e._check(L.sd_cas_index_lookup_dev(e.h, self._handle(), _ptr(keys) if n else None, n,
                                               _ptr(out) if n else None, _stream(stream)), "index_lookup")
            return out
        k = self._host_keys(keys)
        o = np.full(len(k), NO_OBJECT, dtype=np.uint32)
        e._check(L.sd_cas_index_lookup(e.h, self._handle(), _np_ptr(k) if len(k) else None, len(k),
                                       _np_ptr(o) if len(k) else None), "index_lookup")
        return o

    def erase(self, keys, stream: Optional[int] = None) -> None:
        """Remove the keys whatever id they hold (absent and repeated keys are fine)."""
        e, L = self.eng, self.eng.L
        if self._is_dev(keys):
            import torch
            n = int(keys.numel())
            _check_dev(keys, (torch.int64, torch.uint64), n, "keys")
            e._check(L.sd_cas_index_erase_dev(e.h, self._handle(), _ptr(keys) if n else None, n,
                                              _stream(stream)), "index_erase")
            return
        k = self._host_keys(keys)
        e._check(L.sd_cas_index_erase(e.h, self._handle(), _np_ptr(k) if len(k) else None, len(k)),
                 "index_erase")

    def clear(self, stream: Optional[int] = None) -> None:
        e = self.eng
        e._check(e.L.sd_cas_index_clear(e.h, self._handle(), _stream(stream)), "index_clear")

    def stats(self) -> dict:
        """SD_CAS_INDEX_STAT_* keyed by INDEX_STAT_NAMES (blocks)."""
        e = self.eng
        st = np.zeros(8, dtype=np.uint64)
        e._check(e.L.sd_cas_index_stats(e.h, self._handle(), _np_ptr(st)), "index_stats")
        return {name: int(st[i]) for i, name in enumerate(INDEX_STAT_NAMES)}

    def __len__(self) -> int:
        return self.stats()["entries"]

    def export(self, device=None, stream: Optional[int] = None):
        """The live pairs in unspecified order as device tensors (keys int64, ids int32) — what
        `existing=` of identifier_links takes (blocks)."""
        import torch
        e = self.eng
        dev = device if device is not None else f"cuda:{e.device}"
        n = len(self)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        ids = torch.empty(n, dtype=torch.int32, device=dev)
        got = ctypes.c_uint64(0)
        e._check(e.L.sd_cas_index_export_dev(e.h, self._handle(), _ptr(keys) if n else None,
                                             _ptr(ids) if n else None, n, ctypes.byref(got),
                                             _stream(stream)), "index_export")
        return keys[:int(got.value)], ids[:int(got.value)]


def engine(device: int = 0) -> CasEngine:
    if device not in _DEFAULT:
        _DEFAULT[device] = CasEngine(device)
    return _DEFAULT[device]


# ---- reference-shaped free functions -----------------------------------------------------
def generate_cas_id(path: str, size: int) -> str:
    """``generate_cas_id(path, size)`` (cas.rs:23): a one-file batch on the GPU.
    Raises OSError like the reference's io::Error.  (size 0 is what FileMetadata::new never
    passes — the batch ABI answers it with no cas_id — so the one-file drop-in hashes
    le64(0) || the file as cas.rs:29 would.)"""
    if size == 0:
        with open(path, "rb") as fh:
            return engine().generate_cas_ids([(fh.read(), 0)])[0]
    keys, status = engine().generate_cas_keys_from_paths([path], [size])
    if status[0] < 0:
        raise OSError(int(-status[0]), os.strerror(int(-status[0])), path)
    return key_to_cas_id(keys[0])


def generate_cas_ids(items: Sequence[tuple[bytes, int]]) -> list[str]:
    """North-star drop-in: ``generate_cas_ids(&[(buf, size)]) -> Vec<CasId>``."""
    return engine().generate_cas_ids(items)


def file_checksum(path: str) -> str:
    """``file_checksum(path)`` (validation/hash.rs:11): full 64-hex BLAKE3 digest."""
    return engine().file_checksum(path)


@dataclass
class FileMetadata:
    """file_identifier/mod.rs:48-53 (kind is out of scope: sd-file-ext)."""
    cas_id: Optional[str]
    size: int


ROW_HASHED, ROW_NO_CAS, ROW_ERROR = 0, 1, 2                          # SD_CAS_ROW_*
STATUS_NO_CAS = 1                                                    # SD_CAS_STATUS_NO_CAS
LINK_CREATED, LINK_LINKED, LINK_DROPPED, LINK_NOT_REACHED, LINK_EXISTING = 0, 1, 2, 3, 4  # SD_CAS_LINK_*


@dataclass
class StepBatch:
    """One job step's DB batches as identifier_job_step issues them (mod.rs:157-347)."""
    step: int
    creates: list = field(default_factory=list)   # rows getting a new Object (create_many)
    links: list = field(default_factory=list)     # (row, row owning the existing Object)
    links_existing: list = field(default_factory=list)  # (row, id of an Object older than the job)
    total_created: int = 0                        # mod.rs:349 (total_created, total_linked)
    total_linked: int = 0


@dataclass
class StepResult:
    """What one file-identifier job (file_identifier_job.rs:180-236 over identifier_job_step,
    mod.rs:98-350) decides for its orphan file_paths."""
    metadata: dict = field(default_factory=dict)   # idx -> FileMetadata (errors dropped)
    object_of: dict = field(default_factory=dict)  # idx -> idx of the file owning its Object
    existing_of: dict = field(default_factory=dict)  # idx -> id of the pre-job Object it links to
    total_created: int = 0
    total_linked: int = 0
    errors: dict = field(default_factory=dict)     # idx -> errno (logged + dropped, :125-141)
    steps: list = field(default_factory=list)      # StepBatch per executed step
    not_reached: list = field(default_factory=list)  # rows past the job's last step


def identifier_job_step(paths: Sequence[str], chunk: int = CHUNK_SIZE,
                        eng: Optional[CasEngine] = None, existing=None,
                        pre_objects=None, index: Optional[ObjectIndex] = None) -> StepResult:
    """Run the file identifier over ``paths`` (ascending file_path.id order: the rows the
    job's orphan query returns — object/cas NULL and indexed size != 0, orphan_path_filters,
    file_identifier_job.rs:251-277) as file_identifier_job.rs:180-236 / mod.rs:98-350 would:
    fs::metadata per row (mod.rs:63), cas_ids from the GPU (len 0 -> no cas_id, mod.rs:78-86;
    an I/O error drops the row, :125-141), and the Object decisions of every step from the
    GPU link emission (sd_cas_identifier_links: grouping + the cursor walk, a last row that
    stays orphan is queried again by the next step).  existing: None for a fresh library,
    else (cas_ids or keys, Object ids) of the Objects the library already holds
    (mod.rs:180-238: a row whose cas_id one carries links to the lowest such id).
    pre_objects: None, or per row the Object id its file_path already holds (a file the
    watcher gave an Object while it was empty, then written: object_id set, cas_id NULL,
    watcher/utils.rs:236-293,473-490) or None / -1 — such rows and the rows of their step
    with the same cas_id link to the smallest Object carrying it (sd_cas_identifier_links_ex).
    index: an ObjectIndex of `eng` in place of `existing` (not both): the library's Objects are
    read from it; the Objects the DB then creates are the caller's to insert.
    Returns the per-file decisions, the per-step batches and the summed (created, linked)."""
    if index is not None and existing is not None:
        raise ValueError("identifier_job_step: existing= and index= exclude each other")
    eng = eng or (index.eng if index is not None else engine())
    res = StepResult()
    n = len(paths)
    if n == 0:
        return res
    # FileMetadata::new per row, behind the ABI: fs::metadata (mod.rs:63), a directory or an
    # error drops the row, length 0 -> no cas_id (mod.rs:78-86), else generate_cas_id; the
    # metadata length each row was decided from comes back with it (one stat per path)
    all_keys, status, sizes = eng.file_metadata_from_paths(paths)
    state = np.full(n, ROW_HASHED, dtype=np.uint8)
    for i in range(n):
        if status[i] == STATUS_NO_CAS:
            state[i] = ROW_NO_CAS
        elif status[i] < 0:
            res.errors[i] = int(-status[i])
            state[i] = ROW_ERROR
    seed = None
    if existing is not None:
        ek, eo = existing
        ek = np.array([cas_id_to_key(x) if isinstance(x, str) else int(x) for x in ek], dtype=np.uint64)
        seed = (ek, np.asarray(eo, dtype=np.uint32))
    step, obj, act, counts = eng.identifier_links_host(all_keys, state, chunk, existing=seed,
                                                       pre_objects=pre_objects, index=index)
    res.steps = [StepBatch(k, total_created=int(c), total_linked=int(ln))
                 for k, (c, ln) in enumerate(counts)]
    for i in range(n):
        a = int(act[i])
        if a == LINK_NOT_REACHED:
            res.not_reached.append(i)
            continue
        if a == LINK_DROPPED:
            continue
        res.metadata[i] = FileMetadata(key_to_cas_id(all_keys[i]) if state[i] == ROW_HASHED else None,
                                       int(sizes[i]))
        b = res.steps[int(step[i])]
        if a == LINK_EXISTING:
            res.existing_of[i] = int(obj[i])
            b.links_existing.append((i, int(obj[i])))
            continue
        res.object_of[i] = int(obj[i])
        if a == LINK_CREATED:
            b.creates.append(i)
        else:
            b.links.append((i, int(obj[i])))
    # a NO_CAS row ending a chunk stays orphan and is queried again by the next step: it
    # gets an Object in each step (mod.rs:277-283, 401-405), `step` names its last one — the
    # row missing from step k's creates is step k+1's first (cursor) row
    first = 0
    for k, b in enumerate(res.steps):
        if b.total_created > len(b.creates):
            while first < n and (int(step[first]) == 0xFFFFFFFF or int(step[first]) <= k):
                first += 1
            if first < n:
                b.creates.append(first)
    res.total_created = int(counts[:, 0].sum()) if len(counts) else 0
    res.total_linked = int(counts[:, 1].sum()) if len(counts) else 0
    return res


# ---- cas_id string consumers: thumbnails (core/src/object/media/thumbnail/) ---------------

def _key_of(cas_id: str) -> int:
    if len(cas_id) != 16:
        raise ValueError(f"a cas_id is 16 hex chars (cas.rs:61), got {cas_id!r}")
    return cas_id_to_key(cas_id)


def get_shard_hex(cas_id: str) -> str:
    """Thumbnail shard directory of a cas_id: its first three hex chars
    (thumbnail/shard.rs:10-13), 4,096 shards 000..fff — sd_cas_shard_hex."""
    out = ctypes.create_string_buffer(4)
    _native.lib().sd_cas_shard_hex(_key_of(cas_id), out)
    return out.value.decode()


def _thumbnail_path(data_dir: str, cas_id: str, library_id: Optional[str]) -> str:
    L = _native.lib()
    dd = os.fsencode(data_dir)
    lib = None if library_id is None else str(library_id).encode()
    need = L.sd_cas_thumbnail_path(dd, lib, _key_of(cas_id), None, 0)
    if need < 0:
        raise CasError(int(need), "sd_cas_thumbnail_path")
    out = ctypes.create_string_buffer(need + 1)
    L.sd_cas_thumbnail_path(dd, lib, _key_of(cas_id), out, need + 1)
    return os.fsdecode(out.value)


def get_indexed_thumbnail_path(data_dir: str, cas_id: str, library_id: str) -> str:
    """get_indexed_thumbnail_path (thumbnail/mod.rs:62-64): data_dir / "thumbnails" /
    library_id / shard / cas_id.webp (``node.config.data_directory()`` given as data_dir)."""
    return _thumbnail_path(data_dir, cas_id, library_id)


def get_ephemeral_thumbnail_path(data_dir: str, cas_id: str) -> str:
    """get_thumbnail_path(.., ThumbnailKind::Ephemeral) (thumbnail/mod.rs:67-82)."""
    return _thumbnail_path(data_dir, cas_id, None)


def _thumb_key(cas_id: str, library_id: Optional[str]) -> list[str]:
    L = _native.lib()
    lib = None if library_id is None else str(library_id).encode()
    need = L.sd_cas_thumb_key(lib, _key_of(cas_id), None, 0)
    out = ctypes.create_string_buffer(need)
    L.sd_cas_thumb_key(lib, _key_of(cas_id), out, need)
    return [x.decode() for x in out.raw[:need].split(b"\0")[:3]]


def get_indexed_thumb_key(cas_id: str, library_id: str) -> list[str]:
    """get_indexed_thumb_key (thumbnail/mod.rs:84-86): [library_id, shard, cas_id]."""
    return _thumb_key(cas_id, library_id)


def get_ephemeral_thumb_key(cas_id: str) -> list[str]:
    """get_ephemeral_thumb_key (thumbnail/mod.rs:88-90, 94-103): ["ephemeral", shard, cas_id]."""
    return _thumb_key(cas_id, None)


def thumbnail_dir(data_dir: str, library_id: Optional[str] = None) -> str:
    """The batch prefix of sd_cas_thumbnail_paths_dev: one kind's thumbnail directory with
    its trailing '/' (the thumbnail path minus "<shard>/<cas_id>.webp")."""
    return _thumbnail_path(data_dir, "0" * 16, library_id)[:-25]
