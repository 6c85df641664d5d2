"""ctypes binding of libpykmer_hip.so (include/pykmer_hip.h).

The engine has no CPU fallback: if the shared library is missing or a call fails, this raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
from ._rt import LIB_PATH, open_library

PK_OK, PK_ERR_ARG, PK_ERR_HIP, PK_ERR_RECS_CAP, PK_ERR_STATE, PK_ERR_FORMAT = 0, -1, -2, -3, -4, -5
PK_FORMAT_FASTA, PK_FORMAT_FASTQ = 0, 1
FORMATS = {"fasta": PK_FORMAT_FASTA, "fastq": PK_FORMAT_FASTQ}
MASK_HARD, MASK_INVERT = 1, 2                                # the mode bits of pk_query_set_mask

RECORD_DTYPE = np.dtype([("name_off", "<u8"), ("name_len", "<u8"), ("seq_len", "<u8"), ("n_valid_kmers", "<u8")])

_u64p = ctypes.POINTER(ctypes.c_uint64)
_SIGNATURES = {
    "pk_version": (ctypes.c_int, []),
    "pk_last_error": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]),
    "pk_device_count": (ctypes.c_int, []),
    "pk_warm": (ctypes.c_int, [ctypes.c_int]),
    "pk_dev_alloc": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint64, ctypes.c_int]),
    "pk_dev_free": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pk_dev_upload": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]),
    "pk_dev_download": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]),
    "pk_dev_mem_info": (ctypes.c_int, [_u64p, _u64p, ctypes.c_int]),
    "pk_count_fasta": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, _u64p, _u64p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u64p, ctypes.c_int]),
    "pk_count_release": (ctypes.c_int, []),
    "pk_indexer_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int]),
    "pk_indexer_create_slice": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "pk_indexer_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "pk_indexer_set_format": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pk_indexer_fastq_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_indexer_set_min_qual": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pk_indexer_fastq_masked": (ctypes.c_int, [ctypes.c_void_p, _u64p]),
    "pk_indexer_feed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_indexer_feed_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_indexer_finish": (ctypes.c_int, [ctypes.c_void_p, _u64p, _u64p, ctypes.c_void_p, _u64p]),
    "pk_indexer_records": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_indexer_table_to_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_indexer_table_slice_to_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "pk_indexer_table_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "pk_indexer_table_slice_to_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "pk_indexer_timings": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_indexer_destroy": (None, [ctypes.c_void_p]),
    "pk_query_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int]),
    "pk_query_set_tables": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "pk_query_results": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_query_set_bins": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "pk_query_bin_count": (ctypes.c_int, [ctypes.c_void_p, _u64p]),
    "pk_query_bin_results": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "pk_query_set_coords": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pk_query_bin_coords": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_query_set_spectrum": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pk_query_spectrum": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_query_set_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pk_query_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_query_set_cover": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pk_query_cover": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u64p]),
    "pk_query_set_mask": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]),
    "pk_query_mask_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u64p]),
    "pk_query_mask_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u64p]),
    "pk_query_set_intervals": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pk_query_interval_count": (ctypes.c_int, [ctypes.c_void_p, _u64p, ctypes.POINTER(ctypes.c_double)]),
    "pk_query_intervals": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_table_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]),
    "pk_gram": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "pk_gram_device_partial": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_double)]),
    "pk_gram_device_accumulate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "pk_gram_device_accumulate_windows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                          ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "pk_gram_expand": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "pk_spectrum_device_accumulate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                                      ctypes.POINTER(ctypes.c_double)]),
    "pk_occgram_device_accumulate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                                     ctypes.POINTER(ctypes.c_double)]),
    "pk_patterns_device_accumulate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "pk_extract_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u64p, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_double)]),
    "pk_extract_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]),
    "pk_extract_table_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_double)]),
    "pk_select_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    "pk_select_set_records": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_select_feed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, _u64p]),
    "pk_select_feed_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, _u64p]),
    "pk_select_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_select_timings": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_select_destroy": (None, [ctypes.c_void_p]),
    "pk_trim_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    "pk_trim_set_cover": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]),
    "pk_trim_feed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "pk_trim_feed_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "pk_trim_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_trim_timings": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_trim_destroy": (None, [ctypes.c_void_p]),
    "pk_correct_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int]),
    "pk_correct_set_tables": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "pk_correct_set_cover": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]),
    "pk_correct_feed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                        ctypes.c_void_p]),
    "pk_correct_feed_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "pk_correct_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_correct_timings": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_correct_destroy": (None, [ctypes.c_void_p]),
    "pk_unitig_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int]),
    "pk_unitig_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]),
    "pk_unitig_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_unitig_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "pk_unitig_timings": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_unitig_graph": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_unitig_edges": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pk_unitig_gfa_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "pk_unitig_graph_timings": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pk_unitig_destroy": (None, [ctypes.c_void_p]),
    "pk_bgzf_scan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _u64p]),
    "pk_bgzf_inflate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                        ctypes.c_int]),
    "pk_bgzf_deflate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.c_void_p, _u64p, ctypes.c_int]),
    "pk_diag_occupancy": (ctypes.c_int, [ctypes.c_int]),
    "pk_diag_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]),
    "pk_diag_settled_chunks": (ctypes.c_int, [ctypes.c_void_p, _u64p]),
    "pk_diag_plan_slice": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]),
    "pk_diag_level2_order": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)

_lib = None


class PkError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libpykmer_hip error {code}: {message}")
        self.code = code


def load():
    """Loads the library (building nothing: run pykmer_amd.build or __graft_entry__.build first)."""
    global _lib
    if _lib is None:
        lib = open_library()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _check(rc):
    if rc != PK_OK:
        buf = ctypes.create_string_buffer(512)
        load().pk_last_error(buf, 512)
        msg = buf.value.decode("utf-8", "replace")
        if rc == PK_ERR_ARG:
            raise ValueError(msg)
        raise PkError(rc, msg)


def _as_u8(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(data, dtype=np.uint8)


def device_count() -> int:
    return load().pk_device_count()


def warm(device: int = 0) -> None:
    """pk_warm: HIP start-up and kernel load on `device` (the CLIs call this from a thread while they set up)."""
    _check(load().pk_warm(device))


def mem_info(device: int = 0):
    """(free, total) bytes of HBM on `device`."""
    f, t = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(load().pk_dev_mem_info(ctypes.byref(f), ctypes.byref(t), device))
    return int(f.value), int(t.value)


def _hist_out():
    return np.zeros(256, dtype=np.uint64)


def _ptr_array(dev_ptrs):
    """A C array of the device pointers (of one element at least: ctypes gives an empty array no address to pass)."""
    return (ctypes.c_void_p * max(1, len(dev_ptrs)))(*dev_ptrs)


class DeviceBuffer:
    """n bytes of HBM on one device (pk_dev_*)."""

    def __init__(self, n_bytes: int, device: int = 0):
        self.n, self.device = int(n_bytes), device
        p = ctypes.c_void_p()
        _check(load().pk_dev_alloc(ctypes.byref(p), self.n, device))
        self.ptr = p.value

    def zero(self):
        self.upload(np.zeros(self.n, dtype=np.uint8))

    def upload(self, data, offset: int = 0):
        buf = _as_u8(data)
        assert offset + buf.size <= self.n
        _check(load().pk_dev_upload(ctypes.c_void_p(self.ptr + offset), buf.ctypes.data, buf.size, self.device))

    def download(self, n_bytes: int = None, offset: int = 0) -> np.ndarray:
        n = self.n - offset if n_bytes is None else n_bytes
        out = np.empty(n, dtype=np.uint8)
        _check(load().pk_dev_download(out.ctypes.data, ctypes.c_void_p(self.ptr + offset), n, self.device))
        return out

    def download_into(self, out: np.ndarray, offset: int = 0) -> None:
        """Bytes [offset, offset + out.size) into `out`, a writable contiguous uint8 array (e.g. a slice of a memmap)."""
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable and offset + out.size <= self.n
        _check(load().pk_dev_download(out.ctypes.data, ctypes.c_void_p(self.ptr + offset), out.size, self.device))

    def free(self):
        if getattr(self, "ptr", None):
            load().pk_dev_free(ctypes.c_void_p(self.ptr), self.device)
            self.ptr = None

    __del__ = free


class Indexer:
    """One 4^k count table resident in HBM on one device (pk_indexer_*).  fmt: what the feeds hold, "fasta" or "fastq"
    (pk_indexer_set_format; it stays across resets).  min_qual_byte: FASTQ only, the threshold byte Q + offset below which a
    base counts as N (pk_indexer_set_min_qual; 0 = off; it stays across resets too)."""

    TIMINGS = ("scan_s", "squeeze_s", "finalize_s", "zero_s", "feeds", "partition_s", "bucket_s", "walk_sort_s", "relayouts",
               "buckets_recounted")
    COUNTERS = ("feeds", "relayouts", "buckets_recounted")   # of TIMINGS: integers, not seconds

    def __init__(self, k: int, device: int = 0, slice_index: int = 0, n_slices: int = 1, fmt: str = "fasta", min_qual_byte: int = 0):
        if fmt not in FORMATS:
            raise ValueError(f"unknown input format {fmt!r}: expected one of {sorted(FORMATS)}")
        if min_qual_byte and fmt != "fastq":
            raise ValueError("min_qual_byte needs fmt=\"fastq\": only FASTQ records carry base qualities")
        self._h = ctypes.c_void_p()
        self.k, self.device, self.slice_index, self.n_slices, self.fmt = k, device, slice_index, n_slices, fmt
        self.table_bytes = 4 ** k // n_slices
        self._create()
        if fmt != "fasta":
            _check(load().pk_indexer_set_format(self._h, FORMATS[fmt]))
        if min_qual_byte:
            _check(load().pk_indexer_set_min_qual(self._h, int(min_qual_byte)))

    def _create(self):
        _check(load().pk_indexer_create_slice(ctypes.byref(self._h), self.k, self.device, self.slice_index, self.n_slices))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            load().pk_indexer_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        _check(load().pk_indexer_reset(self._h))

    def feed(self, data):
        buf = _as_u8(data)                                   # bytes, bytearray, mmap, numpy: no copy for any of them
        _check(load().pk_indexer_feed(self._h, buf.ctypes.data, buf.size))

    def feed_device(self, dev_ptr: int, n_bytes: int):
        _check(load().pk_indexer_feed_device(self._h, ctypes.c_void_p(dev_ptr), n_bytes))

    def finish(self):
        nk, bp, nr = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        hist = _hist_out()
        _check(load().pk_indexer_finish(self._h, ctypes.byref(nk), ctypes.byref(bp), hist.ctypes.data, ctypes.byref(nr)))
        return {"num_kmers": int(nk.value), "total_bp": int(bp.value), "hist256": hist, "n_records": int(nr.value)}

    def records(self, n_records: int) -> np.ndarray:
        recs = np.zeros(max(n_records, 1), dtype=RECORD_DTYPE)
        _check(load().pk_indexer_records(self._h, recs.ctypes.data, recs.size))
        return recs[:n_records]

    def table_to_host(self, out: np.ndarray = None) -> np.ndarray:
        if out is None:
            out = np.empty(self.table_bytes, dtype=np.uint8)
        assert out.dtype == np.uint8 and out.size == self.table_bytes and out.flags.c_contiguous
        _check(load().pk_indexer_table_to_host(self._h, out.ctypes.data))
        return out

    def table_slice_to_host(self, out: np.ndarray, offset: int):
        """Table bytes [offset, offset + out.size) into `out` (a contiguous uint8 array, e.g. a slice of a memmap)."""
        assert out.dtype == np.uint8 and out.flags.c_contiguous
        _check(load().pk_indexer_table_slice_to_host(self._h, out.ctypes.data, offset, out.size))

    def table_device_ptr(self) -> int:
        p = ctypes.c_void_p()
        _check(load().pk_indexer_table_device(self._h, ctypes.byref(p)))
        return p.value

    def table_slice_to_device(self, dev_dst: int, offset: int, n_bytes: int):
        _check(load().pk_indexer_table_slice_to_device(self._h, ctypes.c_void_p(dev_dst), offset, n_bytes))

    def fastq_stats(self) -> dict:
        """pk_indexer_fastq_stats of a FASTQ indexer: records, lines, FASTQ bytes fed, FASTA bytes emitted."""
        out = np.zeros(4, dtype=np.uint64)
        _check(load().pk_indexer_fastq_stats(self._h, out.ctypes.data))
        return {"records": int(out[0]), "lines": int(out[1]), "bytes_fed": int(out[2]), "bytes_emitted": int(out[3])}

    def fastq_masked(self) -> int:
        """pk_indexer_fastq_masked of a FASTQ indexer: the line-2 bytes replaced by N so far (0 with min_qual_byte = 0)."""
        n = ctypes.c_uint64(0)
        _check(load().pk_indexer_fastq_masked(self._h, ctypes.byref(n)))
        return int(n.value)

    def settled_chunks(self) -> int:
        """pk_diag_settled_chunks: the 16 KiB chunks of the last feed that the structure pass squeezed itself (full chunks of
        plain sequence text not entered inside a header line); 0 for a query indexer."""
        n = ctypes.c_uint64(0)
        _check(load().pk_diag_settled_chunks(self._h, ctypes.byref(n)))
        return int(n.value)

    def _timings_raw(self) -> np.ndarray:
        t = np.zeros(10, dtype=np.float64)
        _check(load().pk_indexer_timings(self._h, t.ctypes.data))
        return t

    def timings(self) -> dict:
        """pk_indexer_timings: the first doubles of the library's ten, under the names of this class's TIMINGS."""
        return {name: int(v) if name in self.COUNTERS else v for name, v in zip(self.TIMINGS, self._timings_raw())}


class QueryIndexer(Indexer):
    """An indexer in query mode (pk_query_*): it parses its feeds like an Indexer, holds no table, and tallies per record how
    many windows hit each of N device-resident 4^k-byte tables.  feed / feed_device / finish / records / reset as Indexer."""

    TIMINGS = ("scan_s", "squeeze_s", "finalize_s", "zero_s", "feeds", "lookup_s", "coords_s", "mask_s")

    def __init__(self, k: int, device: int = 0, fmt: str = "fasta", min_qual_byte: int = 0):
        self.n_tables = 0
        super().__init__(k, device, fmt=fmt, min_qual_byte=min_qual_byte)

    def _create(self):
        _check(load().pk_query_create(ctypes.byref(self._h), self.k, self.device))

    def set_tables(self, dev_ptrs, min_count: int = 1, max_count: int = 255):
        """pk_query_set_tables: device pointers of the 4^k-byte tables (the caller keeps them alive through the feeds)."""
        _check(load().pk_query_set_tables(self._h, _ptr_array(dev_ptrs), len(dev_ptrs), int(min_count), int(max_count)))
        self.n_tables = len(dev_ptrs)

    @staticmethod
    def _room(*shape):
        """(array, view): uint64 zeros with room for `shape` and no empty dimension, so that the library always gets a
        pointer, and the `shape` corner of them that the getter hands back."""
        full = np.zeros([max(int(n), 1) for n in shape], dtype=np.uint64)
        return full, full[tuple(slice(0, int(n)) for n in shape)]

    def results(self, n_records: int):
        """pk_query_results after finish(): (hits, depth), each (n_records, N) uint64."""
        (hits, h), (depth, d) = self._room(n_records, self.n_tables), self._room(n_records, self.n_tables)
        _check(load().pk_query_results(self._h, hits.ctypes.data, depth.ctypes.data, n_records))
        return h, d

    def set_bins(self, bin_windows: int):
        """pk_query_set_bins, after set_tables and before the first feed: tally in bins of `bin_windows` valid windows
        along each record (0: per record, the default a reset restores)."""
        if not 0 <= int(bin_windows) < 2 ** 64:
            raise ValueError(f"bin_windows must be an unsigned 64-bit integer, got {bin_windows}")
        _check(load().pk_query_set_bins(self._h, int(bin_windows)))

    def _bin_count(self) -> int:
        nb = ctypes.c_uint64(0)
        _check(load().pk_query_bin_count(self._h, ctypes.byref(nb)))
        return int(nb.value)

    def bin_results(self, n_records: int):
        """pk_query_bin_results after finish(): (hits, depth, bin_first); hits and depth (B, N) uint64, one row per bin,
        bin_first (n_records + 1,) uint64 with bin_first[-1] = B."""
        B = self._bin_count()
        (hits, h), (depth, d) = self._room(B, self.n_tables), self._room(B, self.n_tables)
        bin_first = np.zeros(n_records + 1, dtype=np.uint64)
        _check(load().pk_query_bin_results(self._h, hits.ctypes.data, depth.ctypes.data, bin_first.ctypes.data, B, n_records))
        return h, d, bin_first

    def set_coords(self, on: bool = True):
        """pk_query_set_coords, after set_bins with W > 0 and before the first feed: also keep every row's base coordinates
        (off by default; a reset clears the setting with the bins)."""
        _check(load().pk_query_set_coords(self._h, 1 if on else 0))

    def bin_coords(self):
        """pk_query_bin_coords after finish(): (bin_start, bin_end), each (B,) uint64 in row order: the position of the first
        base of the row's first window and one past the last base of its last."""
        B = self._bin_count()
        (start, s), (end, e) = self._room(B), self._room(B)
        _check(load().pk_query_bin_coords(self._h, start.ctypes.data, end.ctypes.data, B))
        return s, e

    def set_spectrum(self, on: bool = True):
        """pk_query_set_spectrum, after set_tables and before the first feed (before or after set_bins): also tally the
        table count of every valid window per row and table (off by default; a reset clears the setting)."""
        _check(load().pk_query_set_spectrum(self._h, 1 if on else 0))

    def spectrum(self, n_rows: int):
        """pk_query_spectrum after finish(): (n_rows, N, 256) uint64, spectrum[row][t][c] = the windows of the row whose count
        in table t is c; the rows are the records, or the bins (n_rows = bin_first[-1]) when bins are on."""
        out, view = self._room(n_rows, self.n_tables, 256)
        _check(load().pk_query_spectrum(self._h, out.ctypes.data, n_rows))
        return view

    def set_pairs(self, on: bool = True):
        """pk_query_set_pairs, after set_tables (at most 16) and before the first feed (before or after set_bins): also tally,
        per row and pair of tables, the windows valid in both (off by default; a reset clears the setting)."""
        _check(load().pk_query_set_pairs(self._h, 1 if on else 0))

    def pairs(self, n_rows: int):
        """pk_query_pairs after finish(): (n_rows, P) uint64, P = N (N - 1) / 2, shared[row][p] = the windows of the row valid
        in both tables of pair p (spectrum.pair_list(N)[p]); the rows are the records, or the bins when bins are on."""
        out, view = self._room(n_rows, self.n_tables * (self.n_tables - 1) // 2)
        _check(load().pk_query_pairs(self._h, out.ctypes.data, n_rows))
        return view

    def set_cover(self, on: bool = True):
        """pk_query_set_cover, after set_tables and before the first feed: keep one bit per valid base of the stream, set iff
        the base lies in a valid window that matches at least one table; the feeds then run no lookup (hits stay zero).  Off by
        default; a reset clears the setting."""
        _check(load().pk_query_set_cover(self._h, 1 if on else 0))

    def cover(self, n_bits_cap: int):
        """pk_query_cover after finish(): (cover, n_bases), the packed bits (ceil(n_bases / 8),) uint8, bit g of the stream at
        byte g // 8, bit g % 8 (np.unpackbits(bitorder="little")).  n_bits_cap: an upper bound of n_bases, the bytes fed for one."""
        out = np.zeros((int(n_bits_cap) + 7) // 8 + 1, dtype=np.uint8)
        n = ctypes.c_uint64(0)
        _check(load().pk_query_cover(self._h, out.ctypes.data, int(n_bits_cap), ctypes.byref(n)))
        return out[:(int(n.value) + 7) // 8], int(n.value)

    def set_mask(self, cover, n_bases: int, hard: bool = False, invert: bool = False):
        """pk_query_set_mask, before the first feed and without tables: every feed then leaves its text with the selected valid
        bases marked (mask_text) -- those whose bit in `cover` (packed as cover() returns it, for n_bases bases) is set, with
        `invert` the others; lower case, with `hard` N.  A reset ends the mode."""
        bits = np.ascontiguousarray(cover, dtype=np.uint8)
        if bits.ndim != 1 or bits.size != (int(n_bases) + 7) // 8:
            raise ValueError(f"{int(n_bases)} bases take {(int(n_bases) + 7) // 8} bytes of cover bits, got an array of shape {bits.shape}")
        mode = (MASK_HARD if hard else 0) | (MASK_INVERT if invert else 0)
        _check(load().pk_query_set_mask(self._h, bits.ctypes.data if bits.size else None, int(n_bases), mode))

    def mask_text(self, out: np.ndarray) -> np.ndarray:
        """pk_query_mask_text: the last feed's patched bytes into `out` (uint8, at least as long as the feed); returns the view of them."""
        assert out.dtype == np.uint8 and out.flags.c_contiguous
        n = ctypes.c_uint64(0)
        _check(load().pk_query_mask_text(self._h, out.ctypes.data if out.size else None, out.size, ctypes.byref(n)))
        return out[:int(n.value)]

    def mask_counts(self, n_records: int):
        """pk_query_mask_counts after finish(): (masked (n_records,) uint64, n_bases_seen); PkError if the stream's valid bases do
        not number what the mask was made for."""
        masked, view = self._room(n_records)
        n = ctypes.c_uint64(0)
        _check(load().pk_query_mask_counts(self._h, masked.ctypes.data, n_records, ctypes.byref(n)))
        return view, int(n.value)

    def set_intervals(self, on: bool = True):
        """pk_query_set_intervals, after set_mask and before the first feed: also keep the maximal runs of selected bases as
        intervals of positions (off by default; a reset clears the setting)."""
        _check(load().pk_query_set_intervals(self._h, 1 if on else 0))

    def _interval_count(self):
        n, seconds = ctypes.c_uint64(0), ctypes.c_double(0)
        _check(load().pk_query_interval_count(self._h, ctypes.byref(n), ctypes.byref(seconds)))
        return int(n.value), float(seconds.value)

    def intervals(self):
        """pk_query_intervals after finish(): (iv_record, iv_start, iv_end), each (M,) uint64 in stream order; interval j is the
        positions iv_start[j] .. iv_end[j] - 1 of record iv_record[j]."""
        M = self._interval_count()[0]
        (rec, r), (start, s), (end, e) = self._room(M), self._room(M), self._room(M)
        _check(load().pk_query_intervals(self._h, rec.ctypes.data, start.ctypes.data, end.ctypes.data, M))
        return r, s, e

    def interval_seconds(self) -> float:
        """The HIP-event seconds of the interval kernels (not part of mask_s), after finish()."""
        return self._interval_count()[1]


class Selector:
    """The bytes of a chosen subset of the records of a byte stream (pk_select_*): set_records once, then feed the stream in
    consecutive pieces cut anywhere; every feed hands back the bytes of its piece that lie in kept records.  Creating one
    touches no device; set_records with at least one record brings it up."""

    def __init__(self, device: int = 0):
        self._h = ctypes.c_void_p()
        self.device = device
        _check(load().pk_select_create(ctypes.byref(self._h), device))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            load().pk_select_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_records(self, starts, keep):
        """pk_select_set_records: `starts` (R + 1,) non-decreasing stream offsets, `keep` (R,) flags (non-zero keeps record r,
        the bytes [starts[r], starts[r + 1])).  Both are copied.  ValueError for a decreasing list or lengths that differ."""
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        keep = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        if starts.ndim != 1 or keep.ndim != 1 or starts.size != keep.size + 1:
            raise ValueError(f"{keep.size} records need {keep.size + 1} offsets, got {starts.size}")
        _check(load().pk_select_set_records(self._h, starts.ctypes.data, keep.ctypes.data if keep.size else None, keep.size))

    def _fed(self, rc, n_out):
        if rc == PK_ERR_RECS_CAP:
            exc = PkError(rc, f"the feed keeps {int(n_out.value)} bytes: the output is too small")
            exc.needed = int(n_out.value)
            raise exc
        _check(rc)
        return int(n_out.value)

    def feed(self, data, out: np.ndarray = None) -> np.ndarray:
        """pk_select_feed: the next piece of the stream (anything with the buffer protocol) -> its kept bytes, a uint8 array
        (a view of `out`, a writable contiguous uint8 array, when one is given; a PkError with `.needed` and the code
        PK_ERR_RECS_CAP if it is too small -- nothing was written and the same piece may be fed again)."""
        buf = _as_u8(data)
        if out is None:
            out = np.empty(buf.size, dtype=np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable
        n_out = ctypes.c_uint64(0)
        rc = load().pk_select_feed(self._h, buf.ctypes.data if buf.size else None, buf.size, out.ctypes.data if out.size else None, out.size,
                                   ctypes.byref(n_out))
        return out[:self._fed(rc, n_out)]

    def feed_device(self, dev_ptr: int, n_bytes: int, dev_out: int, out_cap: int) -> int:
        """pk_select_feed_device: the next n_bytes of the stream at dev_ptr (HBM, 16-byte aligned) -> the number of kept bytes
        written to dev_out (HBM, any alignment, out_cap bytes of room); PkError with `.needed` as feed."""
        n_out = ctypes.c_uint64(0)
        rc = load().pk_select_feed_device(self._h, ctypes.c_void_p(dev_ptr) if dev_ptr else None, int(n_bytes),
                                          ctypes.c_void_p(dev_out) if dev_out else None, int(out_cap), ctypes.byref(n_out))
        return self._fed(rc, n_out)

    def finish(self) -> dict:
        """pk_select_finish: bytes_fed, bytes_kept, records_kept (kept records whose first byte was fed)."""
        out = np.zeros(3, dtype=np.uint64)
        _check(load().pk_select_finish(self._h, out.ctypes.data))
        return {"bytes_fed": int(out[0]), "bytes_kept": int(out[1]), "records_kept": int(out[2])}

    def timings(self) -> dict:
        """pk_select_timings: the HIP-event seconds of the select kernels so far, and the feeds."""
        out = np.zeros(2, dtype=np.float64)
        _check(load().pk_select_timings(self._h, out.ctypes.data))
        return {"select_s": float(out[0]), "feeds": int(out[1])}


TRIM_FIELDS = ("pos2", "pos4", "end2", "end4", "seq_len", "trim_start", "trim_end", "covered", "lead")   # PK_TRIM_POS2 .. PK_TRIM_LEAD


class Trimmer:
    """The longest covered stretch of every read of a FASTQ stream (pk_trim_*): set_cover once, then feed the stream in
    consecutive pieces of whole records; every feed hands back the nine TRIM_FIELDS of its records.  Creating one touches no
    device; set_cover brings it up."""

    def __init__(self, device: int = 0):
        self._h = ctypes.c_void_p()
        self.device = device
        _check(load().pk_trim_create(ctypes.byref(self._h), device))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            load().pk_trim_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_cover(self, cover, n_bases: int, min_qual_byte: int = 0):
        """pk_trim_set_cover: `cover` packed as QueryIndexer.cover returns it, for n_bases bases (copied); min_qual_byte: the
        threshold byte Q + offset below which a base is no valid base (0 = off).  ValueError for bits of another length."""
        bits = np.ascontiguousarray(cover, dtype=np.uint8)
        if bits.ndim != 1 or bits.size != (int(n_bases) + 7) // 8:
            raise ValueError(f"{int(n_bases)} bases take {(int(n_bases) + 7) // 8} bytes of cover bits, got an array of shape {bits.shape}")
        _check(load().pk_trim_set_cover(self._h, bits.ctypes.data if bits.size else None, int(n_bases), int(min_qual_byte)))

    @staticmethod
    def _offsets(starts):
        """(the offsets as the library takes them, room for the fields of their records)"""
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        if starts.ndim != 1 or starts.size < 1:
            raise ValueError(f"R records need R + 1 offsets, got an array of shape {starts.shape}")
        return starts, np.zeros((len(TRIM_FIELDS), max(1, starts.size - 1)), dtype=np.uint64)

    @staticmethod
    def _fields(out, n_records: int) -> dict:
        flat = out.reshape(-1)[:len(TRIM_FIELDS) * n_records].reshape(len(TRIM_FIELDS), n_records)
        return {name: flat[f].copy() for f, name in enumerate(TRIM_FIELDS)}

    def feed(self, data, starts) -> dict:
        """pk_trim_feed: the next piece of the stream (anything with the buffer protocol), whole records cut by `starts`
        (R + 1,) offsets relative to the piece with starts[R] = its length -> dict of the TRIM_FIELDS, (R,) uint64 each."""
        buf = _as_u8(data)
        starts, out = self._offsets(starts)
        _check(load().pk_trim_feed(self._h, buf.ctypes.data if buf.size else None, buf.size, starts.ctypes.data, starts.size - 1, out.ctypes.data))
        return self._fields(out, starts.size - 1)

    def feed_device(self, dev_ptr: int, n_bytes: int, starts) -> dict:
        """pk_trim_feed_device: the same with the next n_bytes of the stream at dev_ptr (HBM, any alignment)."""
        starts, out = self._offsets(starts)
        _check(load().pk_trim_feed_device(self._h, ctypes.c_void_p(dev_ptr) if dev_ptr else None, int(n_bytes), starts.ctypes.data, starts.size - 1,
                                          out.ctypes.data))
        return self._fields(out, starts.size - 1)

    def finish(self) -> dict:
        """pk_trim_finish: n_records, n_bases (the valid bases seen) and n_covered; PkError (PK_ERR_STATE) if the stream does not
        hold the valid bases the cover bits were made for."""
        out = np.zeros(3, dtype=np.uint64)
        _check(load().pk_trim_finish(self._h, out.ctypes.data))
        return {"n_records": int(out[0]), "n_bases": int(out[1]), "n_covered": int(out[2])}

    def timings(self) -> dict:
        """pk_trim_timings: the HIP-event seconds of the trim kernels so far, and the feeds."""
        out = np.zeros(2, dtype=np.float64)
        _check(load().pk_trim_timings(self._h, out.ctypes.data))
        return {"trim_s": float(out[0]), "feeds": int(out[1])}


CORR_FIELDS = ("pos2", "seq_len", "candidates", "untried", "corrected", "ambiguous")   # PK_CORR_POS2 .. PK_CORR_AMBIGUOUS


class Corrector:
    """Single-base corrections of the reads of a FASTQ stream (pk_correct_*): set_tables, set_cover, then feed the stream in
    consecutive pieces of whole records; every feed hands back the six CORR_FIELDS of its records and the piece with the
    corrected bytes patched in.  Creating one touches no device; set_tables brings it up."""

    def __init__(self, kmer_len: int, device: int = 0):
        self._h = ctypes.c_void_p()
        self.kmer_len, self.device = int(kmer_len), device
        _check(load().pk_correct_create(ctypes.byref(self._h), int(kmer_len), device))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            load().pk_correct_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_tables(self, dev_ptrs, min_count: int = 1, max_count: int = 255):
        """pk_correct_set_tables: device pointers of 4^k-byte tables (at most 16), owned by the caller until the last feed."""
        _check(load().pk_correct_set_tables(self._h, _ptr_array(dev_ptrs), len(dev_ptrs), int(min_count), int(max_count)))

    def set_cover(self, cover, n_bases: int, min_qual_byte: int = 0, min_windows: int = None):
        """pk_correct_set_cover: `cover` packed as QueryIndexer.cover returns it, for n_bases bases (copied); min_qual_byte as for
        Trimmer.set_cover; min_windows: None = (kmer_len + 1) // 2.  ValueError for bits of another length."""
        bits = np.ascontiguousarray(cover, dtype=np.uint8)
        if bits.ndim != 1 or bits.size != (int(n_bases) + 7) // 8:
            raise ValueError(f"{int(n_bases)} bases take {(int(n_bases) + 7) // 8} bytes of cover bits, got an array of shape {bits.shape}")
        M = (self.kmer_len + 1) // 2 if min_windows is None else int(min_windows)
        _check(load().pk_correct_set_cover(self._h, bits.ctypes.data if bits.size else None, int(n_bases), int(min_qual_byte), M))

    @staticmethod
    def _offsets(starts):
        """(the offsets as the library takes them, room for the fields of their records)"""
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        if starts.ndim != 1 or starts.size < 1:
            raise ValueError(f"R records need R + 1 offsets, got an array of shape {starts.shape}")
        return starts, np.zeros((len(CORR_FIELDS), max(1, starts.size - 1)), dtype=np.uint64)

    @staticmethod
    def _fields(out, n_records: int) -> dict:
        flat = out.reshape(-1)[:len(CORR_FIELDS) * n_records].reshape(len(CORR_FIELDS), n_records)
        return {name: flat[f].copy() for f, name in enumerate(CORR_FIELDS)}

    def feed(self, data, starts):
        """pk_correct_feed: the next piece of the stream, whole records cut by `starts` (R + 1,) offsets relative to the piece
        with starts[R] = its length -> (dict of the CORR_FIELDS, (R,) uint64 each; the corrected piece, (n_bytes,) uint8)."""
        buf = _as_u8(data)
        starts, out = self._offsets(starts)
        text_out = np.empty(max(1, buf.size), dtype=np.uint8)
        _check(load().pk_correct_feed(self._h, buf.ctypes.data if buf.size else None, buf.size, starts.ctypes.data, starts.size - 1,
                                      text_out.ctypes.data, out.ctypes.data))
        return self._fields(out, starts.size - 1), text_out[:buf.size]

    def feed_device(self, dev_ptr: int, n_bytes: int, starts, dev_out_ptr: int) -> dict:
        """pk_correct_feed_device: the same with the next n_bytes of the stream at dev_ptr and the corrected piece written to
        dev_out_ptr (HBM, any alignment, not overlapping) -> dict of the CORR_FIELDS."""
        starts, out = self._offsets(starts)
        _check(load().pk_correct_feed_device(self._h, ctypes.c_void_p(dev_ptr) if dev_ptr else None, int(n_bytes), starts.ctypes.data, starts.size - 1,
                                             ctypes.c_void_p(dev_out_ptr) if dev_out_ptr else None, out.ctypes.data))
        return self._fields(out, starts.size - 1)

    def finish(self) -> dict:
        """pk_correct_finish: n_records, n_bases (the valid bases seen) and the four totals; PkError (PK_ERR_STATE) if the stream
        does not hold the valid bases the cover bits were made for."""
        out = np.zeros(6, dtype=np.uint64)
        _check(load().pk_correct_finish(self._h, out.ctypes.data))
        return {"n_records": int(out[0]), "n_bases": int(out[1]), "n_candidates": int(out[2]), "n_untried": int(out[3]), "n_corrected": int(out[4]),
                "n_ambiguous": int(out[5])}

    def timings(self) -> dict:
        """pk_correct_timings: the HIP-event seconds of the correct kernels so far, and the feeds."""
        out = np.zeros(2, dtype=np.float64)
        _check(load().pk_correct_timings(self._h, out.ctypes.data))
        return {"correct_s": float(out[0]), "feeds": int(out[1])}


UNITIG_TOTALS = ("n_nodes", "n_branching", "n_linear", "n_circular", "n_short", "nodes_short", "bytes", "longest_kmers")
UNITIG_GRAPH_TOTALS = ("n_edges", "edges_dropped", "n_dead_ends", "gfa_bytes")


class Unitigs:
    """The unitigs of one table in HBM (pk_unitig_*): build once per table and window, then read the rows and any slice of
    the FASTA text.  Creating one touches no device; ValueError for an even kmer_len or one above 17."""

    def __init__(self, kmer_len: int, device: int = 0):
        self._h = ctypes.c_void_p()
        self.k, self.device = int(kmer_len), device
        self.graph_totals = dict.fromkeys(UNITIG_GRAPH_TOTALS, 0)            # before graph(): the library refuses edges() and gfa_text()
        _check(load().pk_unitig_create(ctypes.byref(self._h), int(kmer_len), device))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            load().pk_unitig_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def build(self, dev_table: int, min_count: int = 1, max_count: int = 255, min_kmers: int = 1) -> dict:
        """pk_unitig_build on the 4^k bytes at dev_table: the UNITIG_TOTALS.  PkError (PK_ERR_STATE) if a walk met its step
        bound, (PK_ERR_RECS_CAP) if the rows or the text do not fit the device."""
        if int(min_kmers) < 1:
            raise ValueError(f"min_kmers must be at least 1, got {min_kmers}")
        out = np.zeros(8, dtype=np.uint64)
        _check(load().pk_unitig_build(self._h, ctypes.c_void_p(dev_table), int(min_count), int(max_count), int(min_kmers), out.ctypes.data))
        self.totals = {name: int(v) for name, v in zip(UNITIG_TOTALS, out)}
        return dict(self.totals)

    def rows(self) -> dict:
        """pk_unitig_rows: first_addr, n_kmers, depth (U,) uint64 and circular (U,) uint8, linear rows first."""
        U = self.totals["n_linear"] + self.totals["n_circular"]
        out = {"first_addr": np.zeros(U, dtype=np.uint64), "n_kmers": np.zeros(U, dtype=np.uint64), "depth": np.zeros(U, dtype=np.uint64),
               "circular": np.zeros(U, dtype=np.uint8)}
        _check(load().pk_unitig_rows(self._h, *(out[key].ctypes.data if U else None for key in ("first_addr", "n_kmers", "depth", "circular")), U))
        return out

    def text(self, offset: int = 0, n_bytes: int = None) -> np.ndarray:
        """pk_unitig_text: bytes [offset, offset + n_bytes) of the FASTA text (to its end by default), uint8."""
        n = self.totals["bytes"] - int(offset) if n_bytes is None else int(n_bytes)
        out = np.empty(max(0, n), dtype=np.uint8)
        _check(load().pk_unitig_text(self._h, out.ctypes.data if out.size else None, int(offset), n))
        return out

    def timings(self) -> dict:
        """pk_unitig_timings: the HIP-event seconds of the link pass, the linear and the circular phase, and the builds."""
        out = np.zeros(4, dtype=np.float64)
        _check(load().pk_unitig_timings(self._h, out.ctypes.data))
        return {"links_s": float(out[0]), "paths_s": float(out[1]), "cycles_s": float(out[2]), "builds": int(out[3])}

    def graph(self) -> dict:
        """pk_unitig_graph on the last build: the UNITIG_GRAPH_TOTALS.  PkError (PK_ERR_STATE) before a build,
        (PK_ERR_RECS_CAP) if the edges or the GFA text do not fit the device."""
        out = np.zeros(4, dtype=np.uint64)
        _check(load().pk_unitig_graph(self._h, out.ctypes.data))
        self.graph_totals = {name: int(v) for name, v in zip(UNITIG_GRAPH_TOTALS, out)}
        return dict(self.graph_totals)

    def edges(self) -> dict:
        """pk_unitig_edges: edge_from, edge_to (E,) uint64 and edge_orient (E,) uint8 (bit 0: from is -, bit 1: to is -)."""
        E = self.graph_totals["n_edges"]
        out = {"edge_from": np.zeros(E, dtype=np.uint64), "edge_to": np.zeros(E, dtype=np.uint64), "edge_orient": np.zeros(E, dtype=np.uint8)}
        _check(load().pk_unitig_edges(self._h, *(out[key].ctypes.data if E else None for key in ("edge_from", "edge_to", "edge_orient")), E))
        return out

    def gfa_text(self, offset: int = 0, n_bytes: int = None) -> np.ndarray:
        """pk_unitig_gfa_text: bytes [offset, offset + n_bytes) of the GFA text (to its end by default), uint8."""
        n = self.graph_totals["gfa_bytes"] - int(offset) if n_bytes is None else int(n_bytes)
        out = np.empty(max(0, n), dtype=np.uint8)
        _check(load().pk_unitig_gfa_text(self._h, out.ctypes.data if out.size else None, int(offset), n))
        return out

    def graph_timings(self) -> dict:
        """pk_unitig_graph_timings: the HIP-event seconds of the edge passes and of the GFA passes of the last graph()."""
        out = np.zeros(2, dtype=np.float64)
        _check(load().pk_unitig_graph_timings(self._h, out.ctypes.data))
        return {"edges_s": float(out[0]), "gfa_s": float(out[1])}


def count_fasta(data, k: int, device: int = 0, table_out: np.ndarray = None):
    """pk_count_fasta: host FASTA text -> dict(table, num_kmers, total_bp, hist256, records)."""
    buf = _as_u8(data)
    if k <= 0 or k % 2 == 0 or k > 17:                      # let the library word the error (tools.py:165-167)
        _check(load().pk_count_fasta(None, 0, k, None, None, None, None, None, 0, None, device))
    table = table_out if table_out is not None else np.empty(4 ** k, dtype=np.uint8)
    nk, bp, nr = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    hist = _hist_out()
    cap = 4096
    while True:
        recs = np.zeros(cap, dtype=RECORD_DTYPE)
        rc = load().pk_count_fasta(buf.ctypes.data, buf.size, k, table.ctypes.data, ctypes.byref(nk), ctypes.byref(bp),
                                   hist.ctypes.data, recs.ctypes.data, cap, ctypes.byref(nr), device)
        if rc == PK_ERR_RECS_CAP and nr.value > cap:
            cap = int(nr.value)
            continue
        _check(rc)
        break
    return {"table": table, "num_kmers": int(nk.value), "total_bp": int(bp.value), "hist256": hist,
            "records": recs[: nr.value].copy()}


def table_stats(table: np.ndarray, device: int = 0) -> np.ndarray:
    """pk_table_stats: 256-bin histogram of a host u8 table."""
    t = _as_u8(table)
    hist = _hist_out()
    _check(load().pk_table_stats(t.ctypes.data, t.size, hist.ctypes.data, device))
    return hist


def gram(tables, min_count: int = 1, max_count: int = 255, devices=(0,)) -> np.ndarray:
    """pk_gram on host tables -> (N,N,3) uint64 matrix (merger.py:136,175-176; zero diagonal)."""
    ts = [_as_u8(t) for t in tables]
    n = ts[0].size
    if any(t.size != n for t in ts):
        raise AssertionError("tables differ in size (tools.py:444)")
    N = len(ts)
    ptrs = (ctypes.c_void_p * N)(*[t.ctypes.data for t in ts])
    devs = (ctypes.c_int * len(devices))(*devices)
    m = np.zeros((N, N, 3), dtype=np.uint64)
    _check(load().pk_gram(ptrs, N, n, min_count, max_count, m.ctypes.data, devs, len(devices)))
    return m


def gram_device_partial(dev_ptrs, n_slice: int, min_count: int = 1, max_count: int = 255, device: int = 0,
                        dev_pair_out: int = None):
    """pk_gram_device_partial on device-resident slices -> (pair[N,N] uint64, kernel_seconds)."""
    N = len(dev_ptrs)
    ptrs = _ptr_array(dev_ptrs)
    pair = np.zeros((N, N), dtype=np.uint64)
    secs = ctypes.c_double(0)
    _check(load().pk_gram_device_partial(ptrs, N, n_slice, min_count, max_count, pair.ctypes.data,
                                         ctypes.c_void_p(dev_pair_out) if dev_pair_out else None, device,
                                         ctypes.byref(secs)))
    return pair, secs.value


def gram_device_accumulate(dev_ptrs, n_slice: int, dev_pair_accum: int, min_count: int = 1, max_count: int = 255,
                           device: int = 0) -> float:
    """pk_gram_device_accumulate: adds one slice's tallies to an N x N u64 accumulator in HBM; returns kernel seconds."""
    N = len(dev_ptrs)
    ptrs = _ptr_array(dev_ptrs)
    secs = ctypes.c_double(0)
    _check(load().pk_gram_device_accumulate(ptrs, N, n_slice, min_count, max_count, ctypes.c_void_p(dev_pair_accum), device,
                                            ctypes.byref(secs)))
    return secs.value


def gram_device_accumulate_windows(dev_ptrs, n_slice: int, dev_pair_accum: int, windows, device: int = 0) -> float:
    """pk_gram_device_accumulate_windows: adds one slice's tallies for every (min_count, max_count) of `windows` to a
    W x N x N u64 accumulator in HBM -- one pass over the slices per group of windows; returns kernel seconds."""
    N, W = len(dev_ptrs), len(windows)
    ptrs = _ptr_array(dev_ptrs)
    mins = (ctypes.c_int * W)(*[int(w[0]) for w in windows])
    maxs = (ctypes.c_int * W)(*[int(w[1]) for w in windows])
    secs = ctypes.c_double(0)
    _check(load().pk_gram_device_accumulate_windows(ptrs, N, n_slice, mins, maxs, W, ctypes.c_void_p(dev_pair_accum), device,
                                                    ctypes.byref(secs)))
    return secs.value


def spectrum_words(N: int) -> int:
    """u64 words of a spectrum accumulator for N tables: N x 256 histograms, then N(N-1)/2 x 255 x 255 joint bins."""
    return N * 256 + N * (N - 1) // 2 * 255 * 255


def spectrum_device_accumulate(dev_ptrs, n_slice: int, dev_accum: int, device: int = 0) -> float:
    """pk_spectrum_device_accumulate: adds the value histograms and joint count spectra of N device-resident slices to a
    spectrum_words(N) u64 accumulator in HBM; returns kernel seconds."""
    N = len(dev_ptrs)
    ptrs = _ptr_array(dev_ptrs)
    secs = ctypes.c_double(0)
    _check(load().pk_spectrum_device_accumulate(ptrs, N, n_slice, ctypes.c_void_p(dev_accum), device, ctypes.byref(secs)))
    return secs.value


def occgram_words(N: int) -> int:
    """u64 words of an occgram accumulator for N tables: occ_hist (N+1), lin (N x N), gram (N x N(N+1)/2)."""
    return (N + 1) + N * N + N * (N * (N + 1) // 2)


def occgram_device_accumulate(dev_ptrs, n_slice: int, dev_accum: int, device: int = 0) -> float:
    """pk_occgram_device_accumulate: adds the occupancy-stratified Gram products of N device-resident slices to an
    occgram_words(N) u64 accumulator in HBM; returns kernel seconds."""
    N = len(dev_ptrs)
    ptrs = _ptr_array(dev_ptrs)
    secs = ctypes.c_double(0)
    _check(load().pk_occgram_device_accumulate(ptrs, N, n_slice, ctypes.c_void_p(dev_accum), device, ctypes.byref(secs)))
    return secs.value


def patterns_words(N: int) -> int:
    """u64 words of a presence-pattern accumulator for N tables: one bin per subset of them."""
    return 1 << N


def patterns_device_accumulate(dev_ptrs, n_slice: int, dev_accum: int, min_count: int = 1, max_count: int = 255, device: int = 0) -> float:
    """pk_patterns_device_accumulate: adds the presence-pattern histogram of N <= 16 device-resident slices under one count
    window to a patterns_words(N) u64 accumulator in HBM; returns kernel seconds."""
    N = len(dev_ptrs)
    ptrs = _ptr_array(dev_ptrs)
    secs = ctypes.c_double(0)
    _check(load().pk_patterns_device_accumulate(ptrs, N, int(n_slice), int(min_count), int(max_count),
                                                ctypes.c_void_p(dev_accum) if dev_accum else None, device, ctypes.byref(secs)))
    return secs.value


def extract_device(dev_ptrs, n_present: int, n_slice: int, first_addr: int, min_count: int, max_count: int, min_present: int,
                   max_absent: int, dev_addr_out: int = None, dev_counts_out: int = None, cap: int = 0, device: int = 0):
    """pk_extract_device on device-resident slices (`n_present` present tables first, then the absent ones) ->
    (n_selected, fits, kernel_seconds).  `fits`: the addresses and count rows were written to the two device arrays
    (n_selected <= cap); with cap = 0 and no arrays the call only counts and `fits` is False unless nothing is selected."""
    N = len(dev_ptrs)
    ptrs = _ptr_array(dev_ptrs)
    count, secs = ctypes.c_uint64(0), ctypes.c_double(0)
    rc = load().pk_extract_device(ptrs, int(n_present), N - int(n_present), int(n_slice), int(first_addr), int(min_count), int(max_count),
                                  int(min_present), int(max_absent), ctypes.c_void_p(dev_addr_out) if dev_addr_out else None,
                                  ctypes.c_void_p(dev_counts_out) if dev_counts_out else None, int(cap), ctypes.byref(count), device,
                                  ctypes.byref(secs))
    if rc != PK_ERR_RECS_CAP:
        _check(rc)
    return int(count.value), rc == PK_OK and int(count.value) <= int(cap), secs.value


TABLE_OPS = ("sum", "min", "max", "count")                  # PK_TABLE_SUM .. PK_TABLE_COUNT


def extract_table_device(dev_ptrs, n_present: int, n_slice: int, min_count: int, max_count: int, min_present: int, max_absent: int, op,
                         dev_table_out: int, dev_hist_accum: int, device: int = 0) -> float:
    """pk_extract_table_device on device-resident slices (`n_present` present tables first, then the absent ones): the
    selection as n_slice bytes at dev_table_out, reduced by `op` (a name of TABLE_OPS, or its number), and the counts of
    the values 1..255 among them added to the 256 u64 at dev_hist_accum; returns kernel seconds."""
    N = len(dev_ptrs)
    ptrs = _ptr_array(dev_ptrs)
    secs = ctypes.c_double(0)
    _check(load().pk_extract_table_device(ptrs, int(n_present), N - int(n_present), int(n_slice), int(min_count), int(max_count), int(min_present),
                                          int(max_absent), TABLE_OPS.index(op) if isinstance(op, str) else int(op),
                                          ctypes.c_void_p(dev_table_out) if dev_table_out else None,
                                          ctypes.c_void_p(dev_hist_accum) if dev_hist_accum else None, device, ctypes.byref(secs)))
    return secs.value


def extract_text(dev_addr: int, m: int, k: int, dev_text_out: int, device: int = 0) -> None:
    """pk_extract_text: m u64 addresses in HBM -> m lines of k letters + newline in HBM."""
    _check(load().pk_extract_text(ctypes.c_void_p(dev_addr) if dev_addr else None, int(m), int(k),
                                  ctypes.c_void_p(dev_text_out) if dev_text_out else None, device))


def bgzf_scan(buf: np.ndarray):
    """pk_bgzf_scan: (offsets, sizes, isizes) of every BGZF block in a u8 array (int64 arrays); ValueError if not BGZF."""
    cap = max(16, buf.size // 4096)
    while True:
        c_off, c_size, isize = (np.zeros(cap, dtype=np.uint64) for _ in range(3))
        n = ctypes.c_uint64(0)
        rc = load().pk_bgzf_scan(buf.ctypes.data, buf.size, cap, c_off.ctypes.data, c_size.ctypes.data, isize.ctypes.data, ctypes.byref(n))
        if rc == PK_ERR_RECS_CAP:
            cap = int(n.value)
            continue
        _check(rc)
        k = int(n.value)
        return c_off[:k].astype(np.int64), c_size[:k].astype(np.int64), isize[:k].astype(np.int64)


def bgzf_inflate(buf: np.ndarray, c_off, c_size, u_off, out: np.ndarray, threads: int) -> None:
    """pk_bgzf_inflate: blocks (c_off[i], c_size[i]) of `buf` -> out[u_off[i] - u_off[0] : u_off[i + 1] - u_off[0]]."""
    n = len(c_off)
    co = np.ascontiguousarray(c_off, dtype=np.uint64)
    cs = np.ascontiguousarray(c_size, dtype=np.uint64)
    uo = np.ascontiguousarray(np.asarray(u_off, dtype=np.int64) - int(u_off[0]), dtype=np.uint64)
    assert uo.size == n + 1 and out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= int(uo[-1])
    _check(load().pk_bgzf_inflate(buf.ctypes.data, buf.size, co.ctypes.data, cs.ctypes.data, uo.ctypes.data, n, out.ctypes.data, int(threads)))


def bgzf_deflate(data: np.ndarray, level: int, block_input: int, threads: int):
    """pk_bgzf_deflate: (compressed blocks back to back as a u8 array, per-block compressed sizes)."""
    n_blocks = (data.size + block_input - 1) // block_input
    dst = np.empty(max(1, n_blocks) * 65536, dtype=np.uint8)
    sizes = np.zeros(max(1, n_blocks), dtype=np.uint64)
    total = ctypes.c_uint64(0)
    _check(load().pk_bgzf_deflate(data.ctypes.data, data.size, level, block_input, dst.ctypes.data, dst.size, sizes.ctypes.data,
                                  ctypes.byref(total), int(threads)))
    return dst[: total.value], sizes[:n_blocks].astype(np.int64)


def diag_plan(k: int, n_bytes: int = 0) -> dict:
    """pk_diag_plan: the partition plan of one feed (n_bytes = 0: the largest piece a feed is cut into)."""
    out = np.zeros(8, dtype=np.uint64)
    _check(load().pk_diag_plan(k, n_bytes, out.ctypes.data))
    names = ("feed_max", "capacity1", "capacity2", "B1", "B2", "fb_bits", "n_chunks", "fits_u32")
    return {n: int(v) for n, v in zip(names, out)}


WS_VARIANTS = ("narrow", "narrow_sliced", "k15", "k17", "wide_sliced", "deep", "wide")
COUNT_KERNELS = ("whole", "bytes", "half")


def diag_plan_slice(k: int, n_slices: int = 1, n_bytes: int = 0) -> dict:
    """pk_diag_plan_slice: the partition plan of one feed into one of n_slices address slices and what the launchers
    choose from it (no GPU is touched).  ValueError for what Indexer(k, n_slices=...) refuses."""
    out = np.zeros(16, dtype=np.uint64)
    _check(load().pk_diag_plan_slice(k, n_slices, n_bytes, out.ctypes.data))
    names = ("addr_bits", "fb_bits", "b1", "b2", "sample_stride", "n_tally", "sample2", "n_chunks", "variant", "count_kernel",
             "split", "B1", "B2", "capacity1", "capacity2", "fits_u32")
    d = {n: int(v) for n, v in zip(names, out)}
    d["variant"] = WS_VARIANTS[d["variant"]]
    d["count_kernel"] = COUNT_KERNELS[d["count_kernel"]]
    return d


def diag_level2_order(sizes) -> np.ndarray:
    """pk_diag_level2_order: the order in which level 2 walks level-1 buckets of these sizes, position class * (B1 / 8) +
    round (no GPU is touched).  ValueError unless B1 is a multiple of 8 from 8 to 512."""
    s = np.ascontiguousarray(sizes, dtype=np.uint32)
    out = np.zeros(max(1, s.size), dtype=np.uint32)
    _check(load().pk_diag_level2_order(s.ctypes.data, s.size, out.ctypes.data))
    return out[:s.size]


def gram_expand(pair: np.ndarray) -> np.ndarray:
    p = np.ascontiguousarray(pair, dtype=np.uint64)
    N = p.shape[0]
    m = np.zeros((N, N, 3), dtype=np.uint64)
    _check(load().pk_gram_expand(p.ctypes.data, N, m.ctypes.data))
    return m
