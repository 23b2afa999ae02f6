"""Batch entry points: many independent streams per launch (the hot path of this package).

``compress_batch`` / ``decompress_batch`` take either host data (bytes-likes / numpy) or data already
resident in HBM (torch CUDA tensors); torch is used only as a device-memory container -- pointers go
straight into the C ABI (include/tamp_amd.h).  CSR contract: stream ``i`` is
``data[in_off[i] : in_off[i] + in_len[i]]``; results land in ``out[out_off[i] : out_off[i] + out_len[i]]``.
"""
from __future__ import annotations

import ctypes as C
import numbers
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import TampAmdConf


def compress_bound(n: int, literal: int = 8, dictionary_reset: bool = False) -> int:
    """Worst-case ``.tamp`` size of an ``n``-byte stream (every byte a literal)."""
    return 1 + int(bool(dictionary_reset)) + (n * (literal + 1) + 7) // 8


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def compress_resets_bound(n, reset_interval: int, literal: int = 8):
    """Not part of the package's surface: how ``compress_batch(..., reset_interval=N, out_cap=None)`` sizes its slabs -- the
    arithmetic of ``tamp_amd_compress_resets_bound`` (tests pin the two together) for whole tables at once, on the device for CUDA
    tensors, where a C call per stream would take a copy and a sync.  Worst-case size of an ``n``-byte stream: per segment
    the 2-byte lead and every byte a literal, a FLUSH token behind every segment but the last.  ``n``: an int, or per-stream lengths
    as a numpy array or torch tensor (-> uint64 array / int64 tensor)."""
    if _is_torch(n):
        import torch

        n = n.to(torch.int64) & 0xFFFFFFFF  # (lengths are uint32 values, whatever the storage)
        closed = (torch.clamp(n, min=1) - 1) // reset_interval
    elif isinstance(n, np.ndarray):
        n = n.astype(np.uint64)
        closed = (np.maximum(n, np.uint64(1)) - np.uint64(1)) // np.uint64(reset_interval)
        reset_interval, literal = np.uint64(reset_interval), np.uint64(literal)
        return (closed * (np.uint64(2) + (reset_interval * (literal + np.uint64(1)) + np.uint64(16)) // np.uint64(8)) + np.uint64(2)
                + ((n - closed * reset_interval) * (literal + np.uint64(1)) + np.uint64(7)) // np.uint64(8))
    else:
        closed = (max(n, 1) - 1) // reset_interval
    return closed * (2 + (reset_interval * (literal + 1) + 16) // 8) + 2 + ((n - closed * reset_interval) * (literal + 1) + 7) // 8


@dataclass
class ResetIndex:
    """Where the dictionary resets of a batch lie (``compress_batch(..., reset_index=True)`` makes one, ``decompress_batch(...,
    reset_index=...)`` takes one as a hint): ``first`` has one entry per stream and one more, stream ``i``'s entries are
    ``off[first[i]:first[i + 1]]``, each the offset, in the stream's compressed bytes, of the byte behind a reset.  numpy arrays
    (uint64, uint32) or CUDA tensors (int64, int32), like the other tables.  ``interval``: the decoded bytes per segment the
    streams were compressed with, which ``read_ranges`` needs (``compress_batch`` fills it)."""
    first: object
    off: object
    interval: Optional[int] = None


@dataclass
class BatchResult:
    out: object          # uint8 buffer (numpy array or torch tensor) holding every stream's slab
    out_off: object      # uint64/int64 [n]
    out_len: object      # uint32/int32 [n]
    status: object       # int8 [n] -- tamp_res per stream
    in_consumed: object = None
    kernel_ms: float = -1.0
    _keep: object = None  # device tensors the asynchronous launch still reads (converted tables, the dictionary)
    _ws_key: object = None  # (streams, capacity, device) when the slab may serve as the next call's workspace (``reuse=``)
    reset_index: Optional[ResetIndex] = None  # compress_batch(..., reset_index=True)

    def stream(self, i: int) -> bytes:
        o, n = int(self.out_off[i]), int(self.out_len[i])
        chunk = self.out[o : o + n]
        return bytes(chunk.cpu().numpy()) if _is_torch(chunk) else chunk.tobytes()

    def streams(self):
        return [self.stream(i) for i in range(len(self.out_len))]

    def packed(self, align: int = 1, out=None, stream=None) -> "PackedBatch":
        """The batch's streams back to back instead of in their slabs: ``pack_batch(self.out, self.out_off, self.out_len, ...)``."""
        return pack_batch(self.out, self.out_off, self.out_len, align=align, out=out, stream=stream)


def _conf(window, literal, extended, dictionary, dictionary_reset=False, lazy_matching=False, run_aware=None) -> TampAmdConf:
    # run_aware: None = TAMP_AMD_HINT_AUTO (by stream length), False = PLAIN, True = RUNS
    hint = 0 if run_aware is None else (2 if run_aware else 1)
    return TampAmdConf(window, literal, int(dictionary is not None), int(bool(extended)), int(bool(dictionary_reset)),
                       int(bool(lazy_matching)), hint)


def _np_u8(x) -> np.ndarray:
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x.reshape(-1), dtype=np.uint8)
    return np.frombuffer(bytes(x), dtype=np.uint8)


def _is_int(x) -> bool:
    """A plain integer capacity: Python or numpy integer scalars, not bool (numpy scalars are not ``int`` instances)."""
    return isinstance(x, numbers.Integral) and not isinstance(x, bool)


def _ptr(a):
    if a is None:
        return None
    if _is_torch(a):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


class DictionaryTable:
    """K custom dictionaries of D bytes each and a per-stream selector: what ``dictionaries=`` + ``dictionary_index=`` of
    ``compress_batch`` / ``decompress_batch`` stand for, and what ``dictionary=`` of the three batch calls takes as well
    (``decoded_size_batch`` in this form only).

    ``dictionaries``: K bytes objects of equal length, or a uint8 array / CUDA tensor of shape ``(K, D)``; D a multiple of 16.
    ``index``: an integer array or CUDA tensor, one entry per stream, each in ``[0, K)`` -- checked here for host arrays; a CUDA
    tensor is not looked at (that would take a sync): an entry outside the table makes its stream fail, alone, with status -21
    (compress) / -3 (decode).  Every check raises ``ValueError`` before anything is loaded or launched.

    Device calls: dictionaries given as bytes or a host array are uploaded on the first call to a device (a synchronous copy
    of K x D bytes) and the tensor is kept on this object -- build the table once and pass it as ``dictionary=`` to every
    call, or pass a CUDA tensor; ``dictionaries=`` makes a new object, and a new upload, per call.
    """

    def __init__(self, dictionaries, index):
        if index is None:
            raise ValueError("dictionaries needs a dictionary_index.")
        if _is_torch(dictionaries) or isinstance(dictionaries, np.ndarray):
            if dictionaries.ndim != 2 or "uint8" not in str(dictionaries.dtype):
                raise ValueError("dictionaries: a uint8 array of shape (K, D) expected.")
            k, d = int(dictionaries.shape[0]), int(dictionaries.shape[1])
            if _is_torch(dictionaries) and not dictionaries.is_cuda:
                dictionaries = dictionaries.numpy()
            buf = dictionaries.contiguous().reshape(-1) if _is_torch(dictionaries) else np.ascontiguousarray(dictionaries).reshape(-1)
        else:
            rows = [bytes(x) for x in dictionaries]
            k, d = len(rows), (len(rows[0]) if rows else 0)
            if any(len(r) != d for r in rows):
                raise ValueError("dictionaries: K dictionaries of equal length expected.")
            buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
        if k == 0 or d == 0 or d % 16:
            raise ValueError("Dictionary size must be a non-zero multiple of 16.")
        if not (_is_torch(index) and index.is_cuda):
            index = np.asarray(index)
            if index.ndim != 1 or index.dtype.kind not in "iu":
                raise ValueError("dictionary_index: a 1-D integer array expected.")
            if index.size and (int(index.min()) < 0 or int(index.max()) >= k):
                raise ValueError("dictionary_index out of range.")
        elif index.ndim != 1 or index.is_floating_point():
            raise ValueError("dictionary_index: a 1-D integer array expected.")
        self.buffer, self.count, self.size, self.index = buf, k, d, index  # (flat uint8 buffer, K, D, selector)
        self._uploaded = {}  # device -> the buffer there

    def __len__(self):
        return self.count * self.size

    def on_device(self, n, dev, with_bytes=True):
        """-> (buffer tensor or None, dict_off int64 tensor) on ``dev``; the offsets are formed there, without a sync."""
        import torch

        if int(self.index.shape[0]) != n:
            raise ValueError("one dictionary_index per stream expected")
        buf = self.buffer
        buf_t = None
        if with_bytes:
            buf_t = self._uploaded.get(str(dev))
            if buf_t is None:
                buf_t = self._uploaded[str(dev)] = buf.to(dev) if _is_torch(buf) else torch.from_numpy(np.array(buf)).to(dev)
        idx = self.index
        idx_t = idx.to(device=dev, dtype=torch.int64) if _is_torch(idx) else torch.from_numpy(idx.astype(np.int64)).to(dev)
        return buf_t, idx_t * self.size

    def on_host(self, n, with_bytes=True):
        """-> (buffer array or None, dict_off uint64 array) in host memory."""
        buf, index = self.buffer, self.index
        if _is_torch(index):
            index = index.cpu().numpy()
            if index.size and (int(index.min()) < 0 or int(index.max()) >= self.count):
                raise ValueError("dictionary_index out of range.")
        if len(index) != n:
            raise ValueError("one dictionary_index per stream expected")
        if with_bytes and _is_torch(buf):
            buf = buf.cpu().numpy()
        return (buf if with_bytes else None), np.ascontiguousarray(index.astype(np.uint64) * np.uint64(self.size))


def _dict_table(dictionary, dictionaries, dictionary_index, window=None):
    """The dictionary arguments of a batch call -> ``(dictionary, table)``, one of them None at least: ``dictionaries=`` +
    ``dictionary_index=`` or ``dictionary=DictionaryTable(...)`` give the table.  ``window``: compress calls, where D must be
    the window itself.  Raises ``ValueError`` before anything is loaded or launched."""
    table = None
    if isinstance(dictionary, DictionaryTable):
        dictionary, table = None, dictionary
        if dictionaries is not None or dictionary_index is not None:
            raise ValueError("dictionary and dictionaries exclude each other.")
    elif dictionaries is None:
        if dictionary_index is not None:
            raise ValueError("dictionary_index needs dictionaries.")
    else:
        if dictionary is not None:
            raise ValueError("dictionary and dictionaries exclude each other.")
        table = DictionaryTable(dictionaries, dictionary_index)
    if table is not None and window is not None and table.size != (1 << window):
        raise ValueError("Dictionary-window size mismatch.")  # (as for one dictionary)
    return dictionary, table


def pack_streams(streams: Sequence[bytes]):
    """list of bytes -> (flat uint8 array, in_off uint64[n], in_len uint32[n])."""
    lens = np.fromiter((len(s) for s in streams), dtype=np.uint32, count=len(streams))
    offs = np.zeros(len(streams), dtype=np.uint64)
    if len(streams):
        offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
    flat = np.frombuffer(b"".join(bytes(s) for s in streams), dtype=np.uint8) if len(streams) else np.zeros(0, np.uint8)
    return flat, offs, lens


def _slab_offsets(caps: np.ndarray):
    offs = np.zeros(len(caps), dtype=np.uint64)
    if len(caps):
        offs[1:] = np.cumsum(caps.astype(np.uint64))[:-1]
    return offs, int(caps.astype(np.uint64).sum())


def trim(device: int = 0) -> int:
    """Release the device scratch the library keeps between calls on ``device`` (decoder window slabs, the split decoder's
    record slab); returns the bytes released.  ``tamp_amd_trim`` of the C ABI."""
    freed = int(_lib.load().tamp_amd_trim(device))
    if freed < 0:
        _lib.check_launch(freed)
    return freed


def compress_batch(data, in_off=None, in_len=None, *, window: int = 10, literal: int = 8, extended: bool = True,
                   dictionary=None, dictionary_reset: bool = False, lazy_matching: bool = False, out_cap=None,
                   max_in_len: int = 0, device: int = 0, stream=None, timing: bool = False,
                   run_aware=None, reuse=None, dictionaries=None, dictionary_index=None, reset_interval=None,
                   reset_index: bool = False) -> BatchResult:
    """Compress many independent streams in one launch.

    ``data`` is a list of bytes-likes (host), a flat numpy uint8 array + ``in_off``/``in_len`` (host), or a flat
    torch CUDA uint8 tensor + CUDA ``in_off`` (int64) / ``in_len`` (int32) tensors (device, zero-copy).
    Stream ``i``'s output equals ``tamp.compress(stream_i, window=..., literal=..., dictionary=..., extended=...)``
    of the reference.  ``status[i]`` holds the reference's ``tamp_res`` code for that stream.
    ``run_aware`` picks the kernel build for batches of SHORT messages (same bytes either way): True = the run-aware
    build (long runs listed once, most extended matches settled without a search), False = the lean one-wavefront build
    (faster for short messages), None = the lean build.  Streams of 1 KiB and more (``max_in_len`` >= 1024, or unknown)
    always take the run-aware build since round 3 -- it was the faster one on every text measured -- and the argument
    (like ``$TAMP_AMD_RUNS``) is ignored for them.
    ``reuse`` (device batches with an integer ``out_cap``): the result of an earlier call with the same stream count and
    capacity on the same device; its output slab and tables are overwritten instead of allocating new ones.
    ``dictionaries`` + ``dictionary_index``: one custom dictionary PER STREAM in one launch (``tamp_batch_compress_dicts``).
    ``dictionaries`` is K bytes objects of ``1 << window`` bytes each, or a uint8 array / CUDA tensor of shape
    ``(K, 1 << window)``; stream ``i`` is compressed as ``dictionary=dictionaries[dictionary_index[i]]`` would compress it
    (``dictionary=DictionaryTable(dictionaries, dictionary_index)`` says the same).
    ``reset_interval`` (with ``dictionary_reset=True``; not in the reference): every stream is cut every ``reset_interval`` bytes
    and the segments of ALL streams are the units of work (``tamp_batch_compress_resets``), so a ragged batch does
    not wait for its longest stream.  Stream ``i`` is ``tamp_amd.compress(stream_i, dictionary_reset=True, reset_interval=...)``;
    ``out_cap=None`` sizes the slabs with the bound of ``tamp_amd_compress_resets_bound``.  ``max_in_len`` stays a hint, as without resets.  Not with a dictionary of any form, nor with ``reuse``.
    ``reset_index=True`` (with ``reset_interval``): the result's ``reset_index`` says where every reset of every stream lies
    (``ResetIndex``, ``tamp_batch_compress_resets_index``) -- the same bytes, and what ``decompress_batch(..., reset_index=...)``
    reads the batch back with.  Device tensors: one more sync, for the number of entries.
    """
    if reset_index and reset_interval is None:
        raise ValueError("reset_index needs reset_interval")
    if reset_interval is not None:  # (the rules and wording of codec._compress_resets; all decided before the library is looked for)
        if isinstance(reset_interval, bool) or not isinstance(reset_interval, int) or reset_interval < 1:
            raise ValueError("reset_interval must be a positive integer")
        if not dictionary_reset:
            raise ValueError("reset_interval needs dictionary_reset=True")
        if dictionary is not None or dictionaries is not None or dictionary_index is not None:
            raise ValueError("reset_interval excludes dictionaries: a reset restores the seeded window")
        if reuse is not None:
            raise ValueError("reset_interval excludes reuse")
        if reset_interval > 0xFFFFFFFF:
            raise ValueError("reset_interval must fit 32 bits")
        if not 8 <= window <= 15:
            raise ValueError(f"window must be in 8..15, not {window!r}")
        if not 5 <= literal <= 8:
            raise ValueError(f"literal must be in 5..8, not {literal!r}")
    dictionary, table = _dict_table(dictionary, dictionaries, dictionary_index, window)
    if stream is not None and _is_torch(data):
        # The call makes its tables (capacities, offsets) and its output slab with torch: they have to come into being on the
        # stream the kernels are enqueued on, or the launch races the fill kernels of torch's current stream (and the caching
        # allocator hands the slab's memory on while the launch still writes it).
        import torch

        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
            return compress_batch(data, in_off, in_len, window=window, literal=literal, extended=extended,
                                  dictionary=dictionary if table is None else table,
                                  dictionary_reset=dictionary_reset, lazy_matching=lazy_matching, out_cap=out_cap,
                                  max_in_len=max_in_len, device=device, stream=None, timing=timing, run_aware=run_aware, reuse=reuse,
                                  reset_interval=reset_interval, reset_index=reset_index)
    lib = _lib.load()
    conf = _conf(window, literal, extended, dictionary if table is None else table, dictionary_reset, lazy_matching, run_aware)
    if dictionary is not None and not _is_torch(dictionary) and len(dictionary) != (1 << window):
        raise ValueError("Dictionary-window size mismatch.")  # tamp/_c_compressor.pyx:43-46
    lib.tamp_amd_set_timing(1 if timing else 0)

    if _is_torch(data):
        import torch

        n = int(in_len.numel())
        dev = data.device
        ws = None
        if reuse is not None and out_cap is not None and _is_int(out_cap) and reuse._ws_key == (n, int(out_cap), str(dev)):
            # steady-state callers (one launch per step on the same shapes): the output slab and its tables of the
            # previous call are written again -- no allocation, no fill kernels, nothing on the host but the launch
            ws = reuse
            out, out_off_t, out_len_t, status_t, out_cap_t = ws.out, ws.out_off, ws.out_len, ws.status, ws._keep[3]
        elif out_cap is None and reset_interval is not None:
            cap64 = compress_resets_bound(in_len, reset_interval, literal)
            total, largest = (int(x) for x in torch.stack((cap64.sum(), cap64.max())).tolist()) if n else (0, 0)
            if largest > 0xFFFFFFFF:
                raise ValueError("a stream's bound does not fit 32 bits: pass out_cap")
            out_cap_t = cap64.to(torch.int32)  # (the low 32 bits: what the library reads as uint32)
            out_off_t = torch.cumsum(cap64, 0) - cap64
        elif out_cap is None or _is_int(out_cap):
            if _is_int(out_cap):
                cap1 = int(out_cap)  # one capacity for every stream: no device round trip to lay the slabs out
                # (max_in_len stays as given: 0 = unknown, which AUTO reads as "long streams" -> the run-aware build;
                # pass max_in_len for batches of short messages)
            else:
                if not max_in_len:
                    max_in_len = int(in_len.max().item()) if n else 0
                cap1 = compress_bound(max_in_len, literal, dictionary_reset)
            out_cap_t = torch.full((n,), cap1, dtype=torch.int32, device=dev)
            out_off_t = torch.arange(n, dtype=torch.int64, device=dev) * cap1
            total = n * cap1
        else:
            out_cap_t = out_cap.to(device=dev, dtype=torch.int32)
            out_off_t = torch.cumsum(out_cap_t.to(torch.int64), 0) - out_cap_t.to(torch.int64)
            total = int(out_cap_t.to(torch.int64).sum().item())
        if ws is None:
            out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
            out_len_t = torch.empty(n, dtype=torch.int32, device=dev)
            status_t = torch.empty(n, dtype=torch.int8, device=dev)
        dict_t = None
        if dictionary is not None:
            dict_t = dictionary if _is_torch(dictionary) else torch.frombuffer(bytearray(dictionary), dtype=torch.uint8).to(dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        # the launch is asynchronous: converted copies of the tables must outlive it (they ride on the result)
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)
        dict_off_t = None
        if table is not None:
            dict_t, dict_off_t = table.on_device(n, dev)
            rc = lib.tamp_batch_compress_dicts(C.byref(conf), _ptr(dict_t), int(dict_t.numel()), _ptr(dict_off_t), _ptr(data),
                                               _ptr(in_off_t), _ptr(in_len_t), _ptr(out), _ptr(out_off_t), _ptr(out_cap_t),
                                               _ptr(out_len_t), _ptr(status_t), n, int(max_in_len), _lib.MEM_DEVICE,
                                               dev.index or 0, C.c_void_p(st))
        elif reset_index:
            # (the entries: the `closed` of compress_resets_bound, summed on the device; one sync for the total)
            closed = (torch.clamp(in_len_t.to(torch.int64) & 0xFFFFFFFF, min=1) - 1) // reset_interval
            entries = int(closed.sum().item()) if n else 0
            index = ResetIndex(torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(max(entries, 1), dtype=torch.int32, device=dev)[:entries],
                               int(reset_interval))
            rc = lib.tamp_batch_compress_resets_index(C.byref(conf), _ptr(data), _ptr(in_off_t), _ptr(in_len_t), reset_interval, _ptr(out),
                                                      _ptr(out_off_t), _ptr(out_cap_t), _ptr(out_len_t), _ptr(status_t), n, int(max_in_len),
                                                      _lib.MEM_DEVICE, dev.index or 0, C.c_void_p(st), _ptr(index.first),
                                                      _ptr(index.off) if entries else None, entries)
        elif reset_interval is not None:
            rc = lib.tamp_batch_compress_resets(C.byref(conf), _ptr(data), _ptr(in_off_t), _ptr(in_len_t), reset_interval, _ptr(out),
                                                _ptr(out_off_t), _ptr(out_cap_t), _ptr(out_len_t), _ptr(status_t), n, int(max_in_len),
                                                _lib.MEM_DEVICE, dev.index or 0, C.c_void_p(st))
        else:
            rc = lib.tamp_batch_compress(C.byref(conf), _ptr(dict_t), _ptr(data), _ptr(in_off_t),
                                         _ptr(in_len_t), _ptr(out), _ptr(out_off_t), _ptr(out_cap_t),
                                         _ptr(out_len_t), _ptr(status_t), n, int(max_in_len), _lib.MEM_DEVICE,
                                         dev.index or 0, C.c_void_p(st))
        _lib.check_launch(rc)
        ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
        res = BatchResult(out, out_off_t, out_len_t, status_t, None, ms, (data, in_off_t, in_len_t, out_cap_t, dict_t, dict_off_t))
        res._ws_key = (n, int(out_cap), str(dev)) if (out_cap is not None and _is_int(out_cap)) else None
        res.reset_index = index if reset_index else None
        return res

    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    n = len(in_len)
    if out_cap is None and reset_interval is not None:
        out_cap = compress_resets_bound(in_len, reset_interval, literal)
        if n and int(out_cap.max()) > 0xFFFFFFFF:
            raise ValueError("a stream's bound does not fit 32 bits: pass out_cap")
    elif out_cap is None:
        out_cap = np.array([compress_bound(int(x), literal, dictionary_reset) for x in in_len], dtype=np.uint32)
    elif _is_int(out_cap):
        out_cap = np.full(n, int(out_cap), dtype=np.uint32)
    out_cap = np.ascontiguousarray(out_cap, dtype=np.uint32)
    out_off, total = _slab_offsets(out_cap)
    out = np.zeros(total + 1, dtype=np.uint8)
    out_len = np.zeros(n, dtype=np.uint32)
    status = np.zeros(n, dtype=np.int8)
    d = _np_u8(dictionary) if dictionary is not None else None
    if table is not None:
        d, dict_off = table.on_host(n)
        rc = lib.tamp_batch_compress_dicts(C.byref(conf), _ptr(d), d.size, _ptr(dict_off),
                                           _ptr(flat if flat.size else np.zeros(1, np.uint8)), _ptr(in_off), _ptr(in_len), _ptr(out),
                                           _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status), n, int(max_in_len),
                                           _lib.MEM_HOST, device, C.c_void_p(stream) if stream else None)
    elif reset_index:
        entries = int(((np.maximum(in_len.astype(np.uint64), np.uint64(1)) - np.uint64(1)) // np.uint64(reset_interval)).sum())
        index = ResetIndex(np.zeros(n + 1, dtype=np.uint64), np.zeros(entries, dtype=np.uint32), int(reset_interval))
        rc = lib.tamp_batch_compress_resets_index(C.byref(conf), _ptr(flat if flat.size else np.zeros(1, np.uint8)), _ptr(in_off),
                                                  _ptr(in_len), reset_interval, _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len),
                                                  _ptr(status), n, int(max_in_len), _lib.MEM_HOST, device,
                                                  C.c_void_p(stream) if stream else None, _ptr(index.first),
                                                  _ptr(index.off) if entries else None, entries)
    elif reset_interval is not None:
        rc = lib.tamp_batch_compress_resets(C.byref(conf), _ptr(flat if flat.size else np.zeros(1, np.uint8)), _ptr(in_off), _ptr(in_len),
                                            reset_interval, _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status), n,
                                            int(max_in_len), _lib.MEM_HOST, device, C.c_void_p(stream) if stream else None)
    else:
        rc = lib.tamp_batch_compress(C.byref(conf), _ptr(d), _ptr(flat if flat.size else np.zeros(1, np.uint8)),
                                     _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len),
                                     _ptr(status), n, int(max_in_len), _lib.MEM_HOST, device,
                                     C.c_void_p(stream) if stream else None)
    _lib.check_launch(rc)
    ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
    return BatchResult(out, out_off, out_len, status, None, ms, reset_index=index if reset_index else None)


@dataclass
class DecodedSizes:
    size: object         # uint32/int32 [n] -- bytes stream i decodes to (``limit[i]`` at most)
    status: object       # int8 [n] -- what decoding into ``limit[i]`` bytes of room would report
    in_consumed: object  # uint32/int32 [n]
    kernel_ms: float = -1.0
    _keep: object = None  # device tensors the asynchronous launch still reads


def decoded_size_batch(data, in_off=None, in_len=None, *, limit=None, dictionary=None, max_window_bits: int = 15,
                       device: int = 0, stream=None, timing: bool = False) -> DecodedSizes:
    """How many bytes each ``.tamp`` stream of a batch decodes to, without decoding it (``tamp_batch_decoded_size``).

    Per stream exactly the size, status and consumed count that ``decompress_batch`` reports with ``out_cap = limit``
    (``None``: no limit below 2^32 - 1): status 2 and the full size for a stream that ends normally, status 1 and
    ``size == limit`` for one that would outgrow ``limit`` (an int or a per-stream array), -4 / -3 for malformed input.
    ``data`` takes the three forms of ``decompress_batch``; with torch CUDA tensors the call is one asynchronous kernel on
    torch's current stream (or ``stream``).  Of ``dictionary`` only the length is used; a ``DictionaryTable`` (one dictionary
    per stream, see ``decompress_batch``) is passed as ``dictionary=`` too, and only its shape and selector are used.
    """
    dictionary, table = _dict_table(dictionary, None, None)
    if stream is not None and _is_torch(data):
        import torch  # (tables on the launch stream: see compress_batch)

        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
            return decoded_size_batch(data, in_off, in_len, limit=limit, dictionary=dictionary if table is None else table,
                                      max_window_bits=max_window_bits, device=device, stream=None, timing=timing)
    lib = _lib.load()
    lib.tamp_amd_set_timing(1 if timing else 0)
    dict_len = 0
    if dictionary is not None:
        dict_len = int(dictionary.numel()) if _is_torch(dictionary) else len(dictionary)
    if _is_torch(data):
        import torch

        n = int(in_len.numel())
        dev = data.device
        limit_t = None
        if limit is not None and _is_int(limit):
            if not 0 <= int(limit) <= 0xFFFFFFFF:
                raise ValueError("limit must fit 32 bits")
            if int(limit) != 0xFFFFFFFF:  # (the table holds uint32 values in int32 storage)
                limit_t = torch.full((n,), int(limit) - (1 << 32) if int(limit) >= 1 << 31 else int(limit), dtype=torch.int32, device=dev)
        elif limit is not None:
            limit_t = (limit if _is_torch(limit) else torch.as_tensor(np.asarray(limit, dtype=np.uint32).view(np.int32))).to(device=dev, dtype=torch.int32)
        size_t = torch.empty(n, dtype=torch.int32, device=dev)
        status_t = torch.empty(n, dtype=torch.int8, device=dev)
        consumed_t = torch.empty(n, dtype=torch.int32, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)  # kept alive on the result (async launch)
        dict_off_t = None
        if table is not None:
            _, dict_off_t = table.on_device(n, dev, with_bytes=False)
            rc = lib.tamp_batch_decoded_size_dicts(len(table), _ptr(dict_off_t), max_window_bits, _ptr(data), _ptr(in_off_t),
                                                   _ptr(in_len_t), _ptr(limit_t), _ptr(size_t), _ptr(status_t), _ptr(consumed_t), n,
                                                   _lib.MEM_DEVICE, dev.index or 0, C.c_void_p(st))
        else:
            rc = lib.tamp_batch_decoded_size(dict_len, max_window_bits, _ptr(data), _ptr(in_off_t), _ptr(in_len_t), _ptr(limit_t),
                                             _ptr(size_t), _ptr(status_t), _ptr(consumed_t), n, _lib.MEM_DEVICE, dev.index or 0,
                                             C.c_void_p(st))
        _lib.check_launch(rc)
        ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
        return DecodedSizes(size_t, status_t, consumed_t, ms, (data, in_off_t, in_len_t, limit_t, dict_off_t))

    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    n = len(in_len)
    if limit is not None and _is_int(limit):
        if not 0 <= int(limit) <= 0xFFFFFFFF:
            raise ValueError("limit must fit 32 bits")
        limit = None if int(limit) == 0xFFFFFFFF else np.full(n, int(limit), dtype=np.uint32)
    elif limit is not None:
        limit = np.ascontiguousarray(limit, dtype=np.uint32)
        if len(limit) != n:
            raise ValueError("one limit per stream expected")
    size = np.zeros(n, dtype=np.uint32)
    status = np.zeros(n, dtype=np.int8)
    consumed = np.zeros(n, dtype=np.uint32)
    if table is not None:
        _, dict_off = table.on_host(n, with_bytes=False)
        rc = lib.tamp_batch_decoded_size_dicts(len(table), _ptr(dict_off), max_window_bits,
                                               _ptr(flat if flat.size else np.zeros(1, np.uint8)), _ptr(in_off), _ptr(in_len),
                                               _ptr(limit), _ptr(size), _ptr(status), _ptr(consumed), n, _lib.MEM_HOST, device,
                                               C.c_void_p(stream) if stream else None)
    else:
        rc = lib.tamp_batch_decoded_size(dict_len, max_window_bits, _ptr(flat if flat.size else np.zeros(1, np.uint8)), _ptr(in_off),
                                         _ptr(in_len), _ptr(limit), _ptr(size), _ptr(status), _ptr(consumed), n, _lib.MEM_HOST,
                                         device, C.c_void_p(stream) if stream else None)
    _lib.check_launch(rc)
    ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
    return DecodedSizes(size, status, consumed, ms)


def decompress_batch(data, in_off=None, in_len=None, *, out_cap=None, max_out: int = 0xFFFFFFFF, dictionary=None,
                     max_window_bits: int = 15, scan_headers: bool = True, device: int = 0, stream=None,
                     timing: bool = False, dictionaries=None, dictionary_index=None, reset_index=None) -> BatchResult:
    """Decompress many independent ``.tamp`` streams in one launch (configuration read from each header).

    ``out_cap=None``: the sizes are not known.  ``decoded_size_batch(limit=max_out)`` finds them and stream ``i`` is decoded
    into ``min(size[i] + 1, max_out)`` bytes of room -- per stream exactly the status, bytes and consumed count of
    ``out_cap=max_out``, in slabs of ``size + 1`` bytes instead of ``max_out`` (the extra byte is what lets a stream that
    fits report its end status 2: room used up exactly is status 1 in the reference while padding bits remain).  Host data
    crosses the link twice this way; device data costs one device-to-host sync for the slab total.

    ``max_window_bits`` is the reference's limit (larger headers -> TAMP_INVALID_CONF).  With ``scan_headers`` the
    library first looks at the batch's headers to size its on-chip windows for the largest one present (one tiny
    kernel + a 4-byte copy that waits for the stream); pass ``scan_headers=False`` to stay fully asynchronous.

    ``out_cap`` (int or per-stream array) bounds each stream's output.  ``status[i]`` is the reference's code:
    2 (INPUT_EXHAUSTED) on normal completion, 1 (OUTPUT_FULL) if ``out_cap[i]`` was reached with work left,
    -4 / -3 for malformed input.

    ``dictionaries`` + ``dictionary_index``: one custom dictionary PER STREAM in one launch (``tamp_batch_decompress_dicts``).
    ``dictionaries`` is K bytes objects of equal length D, or a uint8 array / CUDA tensor of shape ``(K, D)``, D a multiple of
    16; a stream whose header has the custom bit is decoded as ``dictionary=dictionaries[dictionary_index[i]]`` would decode
    it, one without the bit ignores its selector (``dictionary=DictionaryTable(dictionaries, dictionary_index)`` says the same).

    ``reset_index`` (the ``ResetIndex`` of ``compress_batch(..., reset_interval=N, reset_index=True)``; not in the reference): the
    segments between the resets of ALL streams are the units of work (``tamp_batch_decompress_resets``), so a ragged
    batch does not wait for its longest stream.  The index is a hint that the library verifies on the device: status, bytes and
    consumed count of every stream are those of the call without it, whatever the index holds.  Not with a dictionary of any form.
    """
    if reset_index is not None:  # (all decided before the library is looked for)
        if dictionary is not None or dictionaries is not None or dictionary_index is not None:
            raise ValueError("reset_index excludes dictionaries: a reset restores the seeded window")
        if not isinstance(reset_index, ResetIndex):
            raise ValueError("reset_index: a ResetIndex expected")
        n_streams = len(data) if in_off is None and not _is_torch(data) else len(in_len)
        if len(reset_index.first) != n_streams + 1:
            raise ValueError("reset_index.first: one entry per stream and one more expected")
    dictionary, table = _dict_table(dictionary, dictionaries, dictionary_index)
    dict_arg = dictionary if table is None else table  # (what the calls below pass on)
    if stream is not None and _is_torch(data):
        import torch  # (tables and output slab on the launch stream: see compress_batch)

        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
            return decompress_batch(data, in_off, in_len, out_cap=out_cap, max_out=max_out, dictionary=dict_arg,
                                    max_window_bits=max_window_bits, scan_headers=scan_headers, device=device, stream=None, timing=timing,
                                    reset_index=reset_index)
    if reset_index is not None:
        return _decompress_batch_resets(data, in_off, in_len, reset_index, out_cap, max_out, max_window_bits, scan_headers, device, stream,
                                        timing)
    if out_cap is None:
        if not 0 <= int(max_out) <= 0xFFFFFFFF:
            raise ValueError("max_out must fit 32 bits")
        if not _is_torch(data) and in_off is None:
            data, in_off, in_len = pack_streams(data)  # (packed once for both calls)
        q = decoded_size_batch(data, in_off, in_len, limit=int(max_out), dictionary=dict_arg, max_window_bits=max_window_bits,
                               device=device, stream=stream)
        if _is_torch(data):
            import torch

            out_cap = torch.clamp((q.size.to(torch.int64) & 0xFFFFFFFF) + 1, max=int(max_out))  # (int64: sizes are uint32 values)
        else:
            out_cap = np.minimum(q.size.astype(np.uint64) + 1, np.uint64(int(max_out))).astype(np.uint32)
        return decompress_batch(data, in_off, in_len, out_cap=out_cap, dictionary=dict_arg, max_window_bits=max_window_bits,
                                scan_headers=scan_headers, device=device, stream=stream, timing=timing)
    lib = _lib.load()
    lib.tamp_amd_set_timing(1 if timing else 0)
    if not scan_headers:
        max_window_bits |= _lib.WINDOW_BITS_EXACT
    if _is_torch(data):
        import torch

        n = int(in_len.numel())
        dev = data.device
        if _is_int(out_cap):
            out_cap = int(out_cap)
            out_cap_t = torch.full((n,), out_cap, dtype=torch.int32, device=dev)
            out_off_t = torch.arange(n, dtype=torch.int64, device=dev) * out_cap
            total = n * out_cap
        else:
            cap64 = out_cap.to(device=dev, dtype=torch.int64)
            out_cap_t = cap64.to(torch.int32)  # (the low 32 bits: what the library reads as uint32)
            out_off_t = torch.cumsum(cap64, 0) - cap64
            total = int(cap64.sum().item())
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        out_len_t = torch.empty(n, dtype=torch.int32, device=dev)
        status_t = torch.empty(n, dtype=torch.int8, device=dev)
        consumed_t = torch.empty(n, dtype=torch.int32, device=dev)
        dict_t, dict_len = None, 0
        if dictionary is not None:
            dict_t = dictionary if _is_torch(dictionary) else torch.frombuffer(bytearray(dictionary), dtype=torch.uint8).to(dev)
            dict_len = int(dict_t.numel())
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)  # kept alive on the result (async launch)
        dict_off_t = None
        if table is not None:
            dict_t, dict_off_t = table.on_device(n, dev)
            rc = lib.tamp_batch_decompress_dicts(_ptr(dict_t), int(dict_t.numel()), _ptr(dict_off_t), max_window_bits, _ptr(data),
                                                 _ptr(in_off_t), _ptr(in_len_t), _ptr(out), _ptr(out_off_t), _ptr(out_cap_t),
                                                 _ptr(out_len_t), _ptr(status_t), _ptr(consumed_t), n, _lib.MEM_DEVICE,
                                                 dev.index or 0, C.c_void_p(st))
        else:
            rc = lib.tamp_batch_decompress(_ptr(dict_t), dict_len, max_window_bits, _ptr(data), _ptr(in_off_t),
                                           _ptr(in_len_t), _ptr(out), _ptr(out_off_t), _ptr(out_cap_t),
                                           _ptr(out_len_t), _ptr(status_t), _ptr(consumed_t), n, _lib.MEM_DEVICE,
                                           dev.index or 0, C.c_void_p(st))
        _lib.check_launch(rc)
        ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
        return BatchResult(out, out_off_t, out_len_t, status_t, consumed_t, ms,
                           (data, in_off_t, in_len_t, out_cap_t, dict_t, dict_off_t))

    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    n = len(in_len)
    if _is_int(out_cap):
        out_cap = np.full(n, int(out_cap), dtype=np.uint32)
    out_cap = np.ascontiguousarray(out_cap, dtype=np.uint32)
    out_off, total = _slab_offsets(out_cap)
    out = np.zeros(total + 1, dtype=np.uint8)
    out_len = np.zeros(n, dtype=np.uint32)
    status = np.zeros(n, dtype=np.int8)
    consumed = np.zeros(n, dtype=np.uint32)
    d = _np_u8(dictionary) if dictionary is not None else None
    if table is not None:
        d, dict_off = table.on_host(n)
        rc = lib.tamp_batch_decompress_dicts(_ptr(d), d.size, _ptr(dict_off), max_window_bits,
                                             _ptr(flat if flat.size else np.zeros(1, np.uint8)), _ptr(in_off), _ptr(in_len),
                                             _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                             _ptr(consumed), n, _lib.MEM_HOST, device, C.c_void_p(stream) if stream else None)
    else:
        rc = lib.tamp_batch_decompress(_ptr(d), len(d) if d is not None else 0, max_window_bits,
                                       _ptr(flat if flat.size else np.zeros(1, np.uint8)), _ptr(in_off), _ptr(in_len),
                                       _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                       _ptr(consumed), n, _lib.MEM_HOST, device, C.c_void_p(stream) if stream else None)
    _lib.check_launch(rc)
    ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
    return BatchResult(out, out_off, out_len, status, consumed, ms)


def _decompress_batch_resets(data, in_off, in_len, index, out_cap, max_out, max_window_bits, scan_headers, device, stream, timing):
    """``decompress_batch(..., reset_index=index)`` behind its checks: with ``out_cap=None`` the call is made twice, first for the
    sizes (no output buffer, ``max_out`` as every stream's limit), then into ``min(size + 1, max_out)`` bytes per stream."""
    if out_cap is None and not 0 <= int(max_out) <= 0xFFFFFFFF:
        raise ValueError("max_out must fit 32 bits")
    lib = _lib.load()
    lib.tamp_amd_set_timing(1 if timing else 0)
    if not scan_headers:
        max_window_bits |= _lib.WINDOW_BITS_EXACT
    if _is_torch(data):
        import torch

        n = int(in_len.numel())
        dev = data.device
        as_t = lambda x, dt: (x if _is_torch(x) else torch.from_numpy(np.asarray(x).astype(np.int64))).to(device=dev, dtype=dt)  # noqa: E731
        first_t, off_t = as_t(index.first, torch.int64), as_t(index.off, torch.int32)
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)  # kept alive on the result (async launch)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream

        def call(out, out_off_t, out_cap_t):
            out_len_t = torch.empty(n, dtype=torch.int32, device=dev)
            status_t = torch.empty(n, dtype=torch.int8, device=dev)
            consumed_t = torch.empty(n, dtype=torch.int32, device=dev)
            _lib.check_launch(lib.tamp_batch_decompress_resets(
                max_window_bits, _ptr(data), _ptr(in_off_t), _ptr(in_len_t), _ptr(first_t), _ptr(off_t) if off_t.numel() else None,
                _ptr(out), _ptr(out_off_t), _ptr(out_cap_t), _ptr(out_len_t), _ptr(status_t), _ptr(consumed_t), n, _lib.MEM_DEVICE,
                dev.index or 0, C.c_void_p(st)))
            return out_len_t, status_t, consumed_t

        if out_cap is None:
            limit = int(max_out)  # (the table holds uint32 values in int32 storage)
            limit_t = torch.full((n,), limit - (1 << 32) if limit >= 1 << 31 else limit, dtype=torch.int32, device=dev)
            size_t, _, _ = call(None, None, limit_t)
            out_cap = torch.clamp((size_t.to(torch.int64) & 0xFFFFFFFF) + 1, max=limit)  # (int64: sizes are uint32 values)
        if _is_int(out_cap):
            out_cap = int(out_cap)
            out_cap_t = torch.full((n,), out_cap, dtype=torch.int32, device=dev)
            out_off_t = torch.arange(n, dtype=torch.int64, device=dev) * out_cap
            total = n * out_cap
        else:
            cap64 = out_cap.to(device=dev, dtype=torch.int64)
            out_cap_t = cap64.to(torch.int32)  # (the low 32 bits: what the library reads as uint32)
            out_off_t = torch.cumsum(cap64, 0) - cap64
            total = int(cap64.sum().item())
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        out_len_t, status_t, consumed_t = call(out, out_off_t, out_cap_t)
        ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
        return BatchResult(out, out_off_t, out_len_t, status_t, consumed_t, ms, (data, in_off_t, in_len_t, out_cap_t, first_t, off_t))

    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    n = len(in_len)
    to_np = lambda x, dt: np.ascontiguousarray((x.cpu().numpy() if _is_torch(x) else np.asarray(x)).astype(dt))  # noqa: E731
    first, off = to_np(index.first, np.uint64), to_np(index.off, np.uint32)
    if not flat.size:
        flat = np.zeros(1, np.uint8)

    def call(out, out_off, out_cap):
        out_len, status, consumed = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.uint32)
        _lib.check_launch(lib.tamp_batch_decompress_resets(
            max_window_bits, _ptr(flat), _ptr(in_off), _ptr(in_len), _ptr(first), _ptr(off) if off.size else None, _ptr(out),
            _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status), _ptr(consumed), n, _lib.MEM_HOST, device,
            C.c_void_p(stream) if stream else None))
        return out_len, status, consumed

    if out_cap is None:
        size, _, _ = call(None, None, np.full(n, int(max_out), dtype=np.uint32))
        out_cap = np.minimum(size.astype(np.uint64) + 1, np.uint64(int(max_out))).astype(np.uint32)
    if _is_int(out_cap):
        out_cap = np.full(n, int(out_cap), dtype=np.uint32)
    out_cap = np.ascontiguousarray(out_cap, dtype=np.uint32)
    out_off, total = _slab_offsets(out_cap)
    out = np.zeros(total + 1, dtype=np.uint8)
    out_len, status, consumed = call(out, out_off, out_cap)
    ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
    return BatchResult(out, out_off, out_len, status, consumed, ms)


@dataclass
class RangeResult:
    out: object          # uint8 buffer (numpy array or torch tensor): the ranges back to back
    out_off: object      # uint64/int64 [n_ranges] -- the running sum of ``length``
    out_len: object      # uint32/int32 [n_ranges] -- bytes delivered
    status: object       # int8 [n_ranges] -- per range (include/tamp_amd.h, tamp_batch_read_ranges)
    kernel_ms: float = -1.0
    _keep: object = None  # device tensors the asynchronous launch still reads

    def range(self, q: int) -> bytes:
        o, n = int(self.out_off[q]), int(self.out_len[q]) & 0xFFFFFFFF
        chunk = self.out[o : o + n]
        return bytes(chunk.cpu().numpy()) if _is_torch(chunk) else chunk.tobytes()

    def ranges(self):
        return [self.range(q) for q in range(len(self.out_len))]


def read_ranges(data, in_off=None, in_len=None, *, reset_index, stream_index, begin, length, reset_interval=None, segment_ends=None,
                max_window_bits: int = 15, device: int = 0, stream=None, timing: bool = False) -> RangeResult:
    """Byte ranges of reset-segmented streams, without decoding the rest (``tamp_batch_read_ranges``; not in the
    reference).  ``data`` as for ``decompress_batch``: the streams of ``compress_batch(..., reset_interval=N, reset_index=True)``,
    ``reset_index`` their index.  Range ``q`` is ``decompress(stream stream_index[q])[begin[q] : begin[q] + length[q]]``; only the
    segments it touches are staged and decoded.  The three range tables are sequences, numpy arrays or CUDA tensors.  The output is
    the ranges back to back; ``status[q]`` is 0 when all of range ``q`` was delivered, 2 when the stream ended first (``out_len[q]``
    bytes are there), negative otherwise -- -22 when the index does not hold up on the touched segments.  The index is trusted
    for position: pass the compressor's own.  ``reset_interval`` defaults to ``reset_index.interval``.

    ``segment_ends=``: the table of segment ends (``ResetScan.segment_ends()``, ``tamp_batch_read_ranges_grid``) for streams whose
    segments differ in size -- reference-made streams with resets of their own, append-mode logs, batches compressed with different
    intervals.  With it no interval is needed, and one that is given is ignored; the table is trusted for position like the index
    and verified on the segments a range touches (status -22 where it does not hold up).  It lives where ``data`` lives."""
    if not isinstance(reset_index, ResetIndex):  # (all decided before the library is looked for)
        raise ValueError("reset_index: a ResetIndex expected")
    n_streams = len(data) if in_off is None and not _is_torch(data) else len(in_len)
    if len(reset_index.first) != n_streams + 1:
        raise ValueError("reset_index.first: one entry per stream and one more expected")
    if not len(stream_index) == len(begin) == len(length):
        raise ValueError("stream_index, begin and length: one entry per range each")
    if segment_ends is not None:
        interval = 0
        if not (_is_torch(segment_ends) or isinstance(segment_ends, np.ndarray)):
            segment_ends = np.array([int(x) for x in segment_ends] or [0], dtype=object)[: len(segment_ends)]
        if _is_torch(segment_ends):  # (torch dtypes have no kind: integers are what is neither floating, complex nor bool)
            dt = segment_ends.dtype
            kind = "f" if dt.is_floating_point or dt.is_complex or "bool" in str(dt) else "i"
        else:
            kind = segment_ends.dtype.kind
        if segment_ends.ndim != 1 or kind not in "iuO":
            raise ValueError("segment_ends: a 1-D table of integers expected")
        if len(segment_ends) != len(reset_index.off) + n_streams:  # (the tables' lengths: nothing is read back)
            raise ValueError("segment_ends: one entry per segment expected, len(reset_index.off) + the number of streams")
        if (_is_torch(segment_ends) and segment_ends.is_cuda) != (_is_torch(data) and data.is_cuda):
            raise ValueError("segment_ends: on another memory kind than the data")
        if _is_torch(segment_ends) and not segment_ends.is_cuda:  # (int64 storage holds uint64 values, as in the other tables)
            segment_ends = segment_ends.long().numpy().view(np.uint64)
        if not _is_torch(segment_ends):
            if len(segment_ends) and (int(segment_ends.min()) < 0 or int(segment_ends.max()) > (1 << 64) - 1):
                raise ValueError("segment_ends: does not fit 64 bits")
            segment_ends = np.ascontiguousarray(segment_ends.astype(np.uint64))
    else:
        interval = reset_interval if reset_interval is not None else reset_index.interval
        if interval is None:
            raise ValueError("reset_interval: not given and not in the index")
        if not _is_int(interval) or not 1 <= int(interval) <= 0xFFFFFFFF:
            raise ValueError("reset_interval: a positive integer that fits 32 bits expected")
        interval = int(interval)
    n_ranges = len(stream_index)
    on_device = _is_torch(data)
    tables = (stream_index, begin, length)
    if not (on_device and all(_is_torch(t) for t in tables)):  # (CUDA tables of a CUDA call are checked by nobody: no sync)
        def host_table(t, what, most, dt):  # -> numpy array of dt; a sequence goes through Python integers (2^64 - 1 is one)
            a = t.cpu().numpy() if _is_torch(t) else (t if isinstance(t, np.ndarray) else np.array([int(x) for x in t] or [0], dtype=object)[: len(t)])
            if a.dtype.kind not in "iuO":
                raise ValueError(what + ": integers expected")
            if len(a) and int(a.min()) < 0 and what == "begin":
                raise ValueError(what + ": negative")
            if len(a) and (int(a.min()) < 0 or int(a.max()) > most):
                raise ValueError(what + ": does not fit %d bits" % most.bit_length())
            return np.ascontiguousarray(a.astype(dt))

        h_stream = host_table(stream_index, "stream_index", 0xFFFFFFFF, np.uint32)
        h_begin = host_table(begin, "begin", (1 << 64) - 1, np.uint64)
        h_length = host_table(length, "length", 0xFFFFFFFF, np.uint32)
        if on_device:
            stream_index, begin, length = h_stream, h_begin, h_length
    if stream is not None and on_device:
        import torch  # (tables and output on the launch stream: see compress_batch)

        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
            return read_ranges(data, in_off, in_len, reset_index=reset_index, stream_index=stream_index, begin=begin, length=length,
                               reset_interval=interval or None, segment_ends=segment_ends, max_window_bits=max_window_bits, device=device,
                               stream=None, timing=timing)
    lib = _lib.load()
    lib.tamp_amd_set_timing(1 if timing else 0)

    def call(*a):  # (the two entries differ in ONE argument: the interval, or the table)
        if segment_ends is None:
            return lib.tamp_batch_read_ranges(*a)
        return lib.tamp_batch_read_ranges_grid(*a[:6], _ptr(ends), *a[7:])
    if on_device:
        import torch

        dev = data.device
        as_t = lambda x, dt: (x if _is_torch(x) else torch.from_numpy(np.asarray(x).astype(np.uint64).view(np.int64))).to(device=dev, dtype=dt)  # noqa: E731
        first_t, off_t = as_t(reset_index.first, torch.int64), as_t(reset_index.off, torch.int32)
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)  # kept alive on the result (async launch)
        stream_t, begin_t, length_t = as_t(stream_index, torch.int32), as_t(begin, torch.int64), as_t(length, torch.int32)
        len64 = length_t.to(torch.int64) & 0xFFFFFFFF  # (lengths are uint32 values, whatever the storage)
        out_off_t = torch.cumsum(len64, 0) - len64
        total = int(len64.sum().item()) if n_ranges else 0
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        out_len_t = torch.empty(n_ranges, dtype=torch.int32, device=dev)
        status_t = torch.empty(n_ranges, dtype=torch.int8, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        # (an empty table still needs an address: the call refuses a null one)
        ends = None if segment_ends is None else (segment_ends.to(device=dev, dtype=torch.int64).contiguous() if segment_ends.numel()
                                                  else torch.zeros(1, dtype=torch.int64, device=dev))
        _lib.check_launch(call(
            max_window_bits, _ptr(data), _ptr(in_off_t), _ptr(in_len_t), _ptr(first_t), _ptr(off_t) if off_t.numel() else None, interval,
            _ptr(stream_t), _ptr(begin_t), _ptr(length_t), _ptr(out), _ptr(out_off_t), _ptr(out_len_t), _ptr(status_t), n_streams,
            n_ranges, _lib.MEM_DEVICE, dev.index or 0, C.c_void_p(st)))
        ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
        return RangeResult(out, out_off_t, out_len_t, status_t, ms,
                           (data, in_off_t, in_len_t, first_t, off_t, stream_t, begin_t, length_t, ends))
    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    to_np = lambda x, dt: np.ascontiguousarray((x.cpu().numpy() if _is_torch(x) else np.asarray(x)).astype(dt))  # noqa: E731
    first, off = to_np(reset_index.first, np.uint64), to_np(reset_index.off, np.uint32)
    range_stream, range_begin, range_len = h_stream, h_begin, h_length
    if not flat.size:
        flat = np.zeros(1, np.uint8)
    out_off, total = _slab_offsets(range_len)
    out = np.zeros(total + 1, dtype=np.uint8)
    out_len, status = np.zeros(n_ranges, dtype=np.uint32), np.zeros(n_ranges, dtype=np.int8)
    ends = None if segment_ends is None else (segment_ends if segment_ends.size else np.zeros(1, np.uint64))
    _lib.check_launch(call(
        max_window_bits, _ptr(flat), _ptr(in_off), _ptr(in_len), _ptr(first), _ptr(off) if off.size else None, interval, _ptr(range_stream),
        _ptr(range_begin), _ptr(range_len), _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(status), n_streams, n_ranges, _lib.MEM_HOST,
        device, C.c_void_p(stream) if stream else None))
    ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
    return RangeResult(out, out_off, out_len, status, ms)


def _aligned_rows(rows: int, stride: int) -> np.ndarray:
    """uint8 [rows, stride] on a 16-byte boundary (the row stores are 16 bytes wide)."""
    raw = np.zeros(rows * stride + 16, dtype=np.uint8)
    at = (-raw.ctypes.data) & 15
    return raw[at : at + rows * stride].reshape(rows, stride)


@dataclass
class SeekIndex:
    """Checkpoints of a batch's streams every ``interval`` decoded bytes (``build_seek_index`` makes one, ``read_ranges_seek`` reads
    through it; ``tamp_batch_seek_index`` of the C ABI says what a checkpoint is).  Stream ``i``'s rows are
    ``first[i]:first[i + 1]`` of ``in_pos`` (input bytes consumed) and ``state`` (16 bytes of decoder state, then the window; rows
    sized for ``window_bits``); row ``r`` of a stream is its decoder after ``(r + 1) * interval`` decoded bytes.  ``size`` and
    ``status`` per stream: what it decodes to, and what decoding it reports.  numpy arrays (uint64, uint32, uint8, uint64, int8) or
    CUDA tensors (int64, int32, uint8, int64, int8), like the other tables."""
    first: object
    in_pos: object
    state: object
    interval: int
    window_bits: int
    size: object
    status: object
    _keep: object = None  # device tensors the asynchronous launch still reads

    @property
    def nbytes(self) -> int:
        """Bytes the index occupies."""
        return sum(int(t.numel()) * t.element_size() if _is_torch(t) else int(t.nbytes)
                   for t in (self.first, self.in_pos, self.state, self.size, self.status))

    def to(self, device) -> "SeekIndex":
        """The index in host memory (``"cpu"``: numpy arrays) or on a CUDA device (tensors)."""
        if str(device) == "cpu":
            host = lambda t, dt: np.ascontiguousarray(t.cpu().numpy().view(dt) if _is_torch(t) else np.asarray(t, dtype=dt))  # noqa: E731
            state = host(self.state, np.uint8)
            rows = _aligned_rows(*state.shape) if state.ndim == 2 else state
            rows[...] = state
            return SeekIndex(host(self.first, np.uint64), host(self.in_pos, np.uint32), rows, self.interval, self.window_bits,
                             host(self.size, np.uint64), host(self.status, np.int8))
        import torch

        dev = lambda t, dt, st: (t if _is_torch(t) else torch.from_numpy(np.ascontiguousarray(t).view(dt))).to(device=device, dtype=st)  # noqa: E731
        return SeekIndex(dev(self.first, np.int64, torch.int64), dev(self.in_pos, np.int32, torch.int32),
                         dev(self.state, np.uint8, torch.uint8).contiguous(), self.interval, self.window_bits,
                         dev(self.size, np.int64, torch.int64), dev(self.status, np.int8, torch.int8))

    def extend(self, data, in_off=None, in_len=None, **kwargs) -> "SeekIndex":
        """``extend_seek_index(data, in_off, in_len, seek_index=self, ...)``: a new index for the grown batch; this one stays."""
        return extend_seek_index(data, in_off, in_len, seek_index=self, **kwargs)

    def save(self, path) -> None:
        """One ``.npz`` file at exactly ``path``, with host arrays."""
        h = self.to("cpu")
        with open(path, "wb") as f:
            np.savez(f, first=h.first, in_pos=h.in_pos, state=h.state, interval=np.uint64(h.interval),
                     window_bits=np.uint64(h.window_bits), size=h.size, status=h.status)

    @staticmethod
    def load(path) -> "SeekIndex":
        with np.load(path) as z:
            state = z["state"]
            rows = _aligned_rows(*state.shape)
            rows[...] = state
            return SeekIndex(z["first"].astype(np.uint64), z["in_pos"].astype(np.uint32), rows, int(z["interval"]),
                             int(z["window_bits"]), z["size"].astype(np.uint64), z["status"].astype(np.int8))


def _seek_interval(interval, window_bits: int) -> int:
    if interval is None:
        return 16 << window_bits
    if not _is_int(interval) or not 1 <= int(interval) <= 0xFFFFFFFF:
        raise ValueError("interval: a positive integer that fits 32 bits expected")
    return int(interval)


def build_seek_index(data, in_off=None, in_len=None, *, interval=None, dictionary=None, max_window_bits: int = 15, device: int = 0,
                     stream=None) -> SeekIndex:
    """Checkpoints for reading byte ranges of streams that have NO dictionary resets (``tamp_batch_seek_index``, DESIGN.md 3.13;
    not in the reference): the streams of plain ``compress`` / ``compress_batch``, of a ``CompressorBatch``, of a reference
    ``Compressor``.  ``data`` as for ``decompress_batch``.  Every stream is decoded once, without its bytes being written anywhere,
    and its decoder is kept every ``interval`` decoded bytes (default ``16 << max_window_bits``: an index of about 1/16 of the
    decoded size).  The rows are sized by ``decoded_size_batch`` first; for host data ``max_window_bits`` becomes the largest
    window a header of the batch asks for (``max_window_bits`` at most)."""
    if not _is_int(max_window_bits) or not 8 <= int(max_window_bits) <= 15:
        raise ValueError("max_window_bits: 8 .. 15 expected")
    if interval is not None:
        _seek_interval(interval, 8)
    if _is_torch(data):
        if in_off is None or in_len is None or not (_is_torch(in_off) and _is_torch(in_len)):
            raise ValueError("in_off, in_len: CUDA tensors expected with CUDA data")
        import torch

        w = int(max_window_bits)
        N = _seek_interval(interval, w)
        if stream is not None:
            with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
                return build_seek_index(data, in_off, in_len, interval=N, dictionary=dictionary, max_window_bits=w, device=device)
        lib = _lib.load()
        dev = data.device
        n = int(in_len.numel())
        sizes = decoded_size_batch(data, in_off, in_len, dictionary=dictionary, max_window_bits=w)
        S = sizes.size.to(torch.int64) & 0xFFFFFFFF
        rows = torch.clamp(S - 1, min=0) // N
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)
        dict_t = None if dictionary is None else (dictionary if _is_torch(dictionary) else torch.from_numpy(_np_u8(dictionary).copy())).to(dev)
        stride = 16 + (1 << w)
        st = torch.cuda.current_stream(dev).cuda_stream
        for _ in range(2):  # (a stream of 2^32 bytes or more: the size query stops there, the index says the rest)
            first_t = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            first_t[1:] = torch.cumsum(rows, 0)
            total = int(first_t[-1].item())
            in_pos_t = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
            state_t = torch.zeros((max(total, 1), stride), dtype=torch.uint8, device=dev)
            size_t = torch.zeros(n, dtype=torch.int64, device=dev)
            status_t = torch.zeros(n, dtype=torch.int8, device=dev)
            _lib.check_launch(lib.tamp_batch_seek_index(
                _ptr(dict_t), 0 if dict_t is None else int(dict_t.numel()), w, _ptr(data), _ptr(in_off_t), _ptr(in_len_t), N, _ptr(first_t),
                _ptr(in_pos_t), _ptr(state_t), stride, _ptr(size_t), _ptr(status_t), n, _lib.MEM_DEVICE, dev.index or 0, C.c_void_p(st)))
            if not bool((S >= 0xFFFFFFFF).any().item()):
                break
            S, rows = size_t, torch.clamp(size_t - 1, min=0) // N
        return SeekIndex(first_t, in_pos_t[:total], state_t[:total], N, w, size_t, status_t,
                         (data, in_off_t, in_len_t, dict_t, in_pos_t, state_t))
    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    n = len(in_len)
    live = in_len > 0
    if live.any() and int((in_off[live].astype(np.uint64) + in_len[live]).max()) > flat.size:
        raise ValueError("in_off, in_len: a stream lies outside the data")
    heads = flat[in_off[live].astype(np.int64)] if live.any() else np.zeros(0, np.uint8)
    w = min(int(max_window_bits), int(((heads >> 5) & 7).max()) + 8 if len(heads) else 8)
    N = _seek_interval(interval, w)
    lib = _lib.load()
    sizes = decoded_size_batch(flat, in_off, in_len, dictionary=dictionary, max_window_bits=w, device=device)
    S = sizes.size.astype(np.uint64)
    dict_a = None if dictionary is None else _np_u8(dictionary)
    stride = 16 + (1 << w)
    if not flat.size:
        flat = np.zeros(1, np.uint8)
    for _ in range(2):  # (as above)
        rows = np.where(S > 0, (np.maximum(S, np.uint64(1)) - np.uint64(1)) // np.uint64(N), np.uint64(0)).astype(np.uint64)
        first = np.zeros(n + 1, dtype=np.uint64)
        first[1:] = np.cumsum(rows)
        total = int(first[-1])
        in_pos = np.zeros(max(total, 1), dtype=np.uint32)
        state = _aligned_rows(max(total, 1), stride)
        size = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int8)
        _lib.check_launch(lib.tamp_batch_seek_index(
            _ptr(dict_a), 0 if dict_a is None else len(dict_a), w, _ptr(flat), _ptr(in_off), _ptr(in_len), N, _ptr(first), _ptr(in_pos),
            _ptr(state), stride, _ptr(size), _ptr(status), n, _lib.MEM_HOST, device, None))
        if not (S >= 0xFFFFFFFF).any():
            break
        S = size
    return SeekIndex(first, in_pos[:total], state[:total], N, w, size, status)


def extend_seek_index(data, in_off=None, in_len=None, *, seek_index, dictionary=None, device: int = 0, stream=None) -> SeekIndex:
    """``seek_index`` brought up to date with streams that have GROWN since it was made, without decoding what it already covers
    (``tamp_batch_seek_index_extend``; not in the reference).  ``data`` is the grown batch, in the forms
    ``build_seek_index`` takes: every stream's old bytes are a prefix of its bytes now, and streams behind the index's last one
    are new and indexed from their headers.  The result equals ``build_seek_index`` of the grown batch at the index's own
    ``interval`` and ``window_bits``; the old index is not modified (its rows are copied to their new places).  Decoding resumes
    at each stream's restart row -- the last row whose ``in_pos`` lies below the last row's -- and not at its last row: the rows
    made at the old end of the input are decoded again.  Two calls: one with the rows the index has, for the sizes, and one that
    writes the new rows."""
    if not isinstance(seek_index, SeekIndex):  # (all decided before the library is looked for)
        raise ValueError("seek_index: a SeekIndex expected")
    on_device = _is_torch(data)
    if on_device and (in_off is None or in_len is None or not (_is_torch(in_off) and _is_torch(in_len))):
        raise ValueError("in_off, in_len: CUDA tensors expected with CUDA data")
    n = len(data) if in_off is None and not on_device else len(in_len)
    n_old = len(seek_index.first) - 1
    if n_old < 0 or n < n_old:
        raise ValueError("seek_index: it holds more streams than the data")
    if seek_index.interval is None:
        raise ValueError("seek_index.interval: the index's own interval expected")
    N = _seek_interval(seek_index.interval, 8)
    w = seek_index.window_bits
    if not _is_int(w) or not 8 <= int(w) <= 15:
        raise ValueError("seek_index.window_bits: 8 .. 15 expected")
    w = int(w)
    for t in (seek_index.first, seek_index.in_pos, seek_index.state):
        if _is_torch(t) != on_device or (on_device and not t.is_cuda):
            raise ValueError("seek_index: on another memory kind than the data (SeekIndex.to)")
    stride = 16 + (1 << w)
    if len(seek_index.state.shape) != 2 or int(seek_index.state.shape[1]) != stride or len(seek_index.state) != len(seek_index.in_pos):
        raise ValueError("seek_index.state: one row of 16 + (1 << window_bits) bytes per entry of in_pos expected")
    if on_device:
        import torch

        if stream is not None:
            with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
                return extend_seek_index(data, in_off, in_len, seek_index=seek_index, dictionary=dictionary, device=device)
        lib = _lib.load()
        dev = data.device
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)
        dict_t = None if dictionary is None else (dictionary if _is_torch(dictionary) else torch.from_numpy(_np_u8(dictionary).copy())).to(dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        old_first = seek_index.first.to(device=dev, dtype=torch.int64)
        old_rows = int(seek_index.in_pos.numel())
        h_first = old_first.cpu().numpy()  # (one small read-back: a first that is no running sum cannot place the rows)
        if int(h_first[0]) != 0 or (np.diff(h_first) < 0).any() or int(h_first[-1]) != old_rows:
            raise ValueError("seek_index.first: a running sum from 0 to the number of rows expected")
        have = torch.zeros(n, dtype=torch.int64, device=dev)
        have[:n_old] = old_first[1:] - old_first[:-1]
        have_t = have.to(torch.int32)
        size_t = torch.zeros(n, dtype=torch.int64, device=dev)
        status_t = torch.zeros(n, dtype=torch.int8, device=dev)

        def call(first_t, in_pos_t, state_t):
            _lib.check_launch(lib.tamp_batch_seek_index_extend(
                _ptr(dict_t), 0 if dict_t is None else int(dict_t.numel()), w, _ptr(data), _ptr(in_off_t), _ptr(in_len_t), N, _ptr(first_t),
                _ptr(have_t), _ptr(in_pos_t), _ptr(state_t), stride, _ptr(size_t), _ptr(status_t), n, _lib.MEM_DEVICE, dev.index or 0,
                C.c_void_p(st)))

        # 1. the sizes: room = have, on a copy of the rows (the call writes the rows behind each restart row again)
        first1 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        first1[1:] = torch.cumsum(have, 0)
        in_pos1 = torch.zeros(old_rows + 1, dtype=torch.int32, device=dev)
        state1 = torch.zeros((old_rows + 1, stride), dtype=torch.uint8, device=dev)
        in_pos1[:old_rows] = seek_index.in_pos.to(torch.int32)
        state1[:old_rows] = seek_index.state
        call(first1, in_pos1, state1)
        # 2. the new layout; 3. the old rows to their places (a row its stream has no room for any more goes to the spare row)
        rows = torch.clamp(size_t - 1, min=0) // N
        first_t = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        first_t[1:] = torch.cumsum(rows, 0)
        total = int(first_t[-1].item())
        in_pos_t = torch.zeros(total + 1, dtype=torch.int32, device=dev)
        state_t = torch.zeros((total + 1, stride), dtype=torch.uint8, device=dev)
        if old_rows:
            owner = torch.repeat_interleave(torch.arange(n, device=dev), have, output_size=old_rows)
            r = torch.arange(old_rows, device=dev) - first1[owner]
            dst = torch.where(r < rows[owner], first_t[owner] + r, torch.full_like(r, total))
            in_pos_t.index_copy_(0, dst, in_pos1[:old_rows])
            state_t.index_copy_(0, dst, state1[:old_rows])
        # 4. the new rows
        call(first_t, in_pos_t, state_t)
        return SeekIndex(first_t, in_pos_t[:total], state_t[:total], N, w, size_t, status_t,
                         (data, in_off_t, in_len_t, dict_t, have_t, in_pos_t, state_t))
    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    live = in_len > 0
    if live.any() and int((in_off[live].astype(np.uint64) + in_len[live]).max()) > flat.size:
        raise ValueError("in_off, in_len: a stream lies outside the data")
    old_first = np.ascontiguousarray(seek_index.first, dtype=np.uint64)
    if int(old_first[0]) != 0 or (np.diff(old_first.astype(np.int64)) < 0).any() or int(old_first[-1]) != len(seek_index.in_pos):
        raise ValueError("seek_index.first: a running sum from 0 to the number of rows expected")
    lib = _lib.load()
    dict_a = None if dictionary is None else _np_u8(dictionary)
    if not flat.size:
        flat = np.zeros(1, np.uint8)
    old_rows = len(seek_index.in_pos)
    have = np.zeros(n, dtype=np.uint32)
    have[:n_old] = np.diff(old_first.astype(np.int64)).astype(np.uint32)
    size = np.zeros(n, dtype=np.uint64)
    status = np.zeros(n, dtype=np.int8)

    def call(first, in_pos, state):
        _lib.check_launch(lib.tamp_batch_seek_index_extend(
            _ptr(dict_a), 0 if dict_a is None else len(dict_a), w, _ptr(flat), _ptr(in_off), _ptr(in_len), N, _ptr(first), _ptr(have),
            _ptr(in_pos), _ptr(state), stride, _ptr(size), _ptr(status), n, _lib.MEM_HOST, device, None))

    # 1. the sizes: room = have, on a copy of the rows (the call writes the rows behind each restart row again)
    first1 = np.zeros(n + 1, dtype=np.uint64)
    first1[1:] = np.cumsum(have.astype(np.uint64))
    in_pos1 = np.zeros(max(old_rows, 1), dtype=np.uint32)
    in_pos1[:old_rows] = seek_index.in_pos
    state1 = _aligned_rows(max(old_rows, 1), stride)
    state1[:old_rows] = seek_index.state
    call(first1, in_pos1, state1)
    # 2. the new layout; 3. the old rows to their places
    rows = np.where(size > 0, (np.maximum(size, np.uint64(1)) - np.uint64(1)) // np.uint64(N), np.uint64(0)).astype(np.uint64)
    first = np.zeros(n + 1, dtype=np.uint64)
    first[1:] = np.cumsum(rows)
    total = int(first[-1])
    in_pos = np.zeros(max(total, 1), dtype=np.uint32)
    state = _aligned_rows(max(total, 1), stride)
    for i in np.flatnonzero(have[:n_old]):
        k = min(int(have[i]), int(rows[i]))
        a, b = int(first1[i]), int(first[i])
        in_pos[b : b + k] = in_pos1[a : a + k]
        state[b : b + k] = state1[a : a + k]
    # 4. the new rows
    call(first, in_pos, state)
    return SeekIndex(first, in_pos[:total], state[:total], N, w, size, status)


def read_ranges_seek(data, in_off=None, in_len=None, *, seek_index, stream_index, begin, length, dictionary=None, device: int = 0,
                     stream=None) -> RangeResult:
    """Byte ranges of streams WITHOUT dictionary resets, through a ``SeekIndex`` (``tamp_batch_read_ranges_seek``, DESIGN.md 3.13;
    not in the reference).  Range ``q`` is ``decompress(stream stream_index[q])[begin[q] : begin[q] + length[q]]``: decoding starts
    at the checkpoint in front of ``begin[q]``, a range that crosses checkpoints is decoded by one wavefront per interval, and the
    bytes go straight to their place in the output.  Tables, output and statuses as for ``read_ranges`` (-22: a row of the index
    does not hold up; -4 comes with the bytes in front of the offending token).  The index is trusted for position and lives where
    ``data`` lives (``SeekIndex.to``)."""
    if not isinstance(seek_index, SeekIndex):  # (all decided before the library is looked for)
        raise ValueError("seek_index: a SeekIndex expected")
    on_device = _is_torch(data)
    if on_device and (in_off is None or in_len is None):
        raise ValueError("in_off, in_len: expected with CUDA data")
    n_streams = len(data) if in_off is None and not on_device else len(in_len)
    if len(seek_index.first) != n_streams + 1:
        raise ValueError("seek_index.first: one entry per stream and one more expected")
    N = _seek_interval(seek_index.interval, 8)
    w = seek_index.window_bits
    if not _is_int(w) or not 8 <= int(w) <= 15:
        raise ValueError("seek_index.window_bits: 8 .. 15 expected")
    w = int(w)
    for t in (seek_index.first, seek_index.in_pos, seek_index.state):
        if _is_torch(t) != on_device or (on_device and not t.is_cuda):
            raise ValueError("seek_index: on another memory kind than the data (SeekIndex.to)")
    stride = 16 + (1 << w)
    if len(seek_index.state.shape) != 2 or int(seek_index.state.shape[1]) != stride or len(seek_index.state) != len(seek_index.in_pos):
        raise ValueError("seek_index.state: one row of 16 + (1 << window_bits) bytes per entry of in_pos expected")
    if not len(stream_index) == len(begin) == len(length):
        raise ValueError("stream_index, begin and length: one entry per range each")
    n_ranges = len(stream_index)
    tables = (stream_index, begin, length)
    if not (on_device and all(_is_torch(t) for t in tables)):  # (CUDA tables of a CUDA call are checked by nobody: no sync)
        def host_table(t, what, most, dt):  # -> numpy array of dt; a sequence goes through Python integers (2^64 - 1 is one)
            a = t.cpu().numpy() if _is_torch(t) else (t if isinstance(t, np.ndarray) else np.array([int(x) for x in t] or [0], dtype=object)[: len(t)])
            if a.dtype.kind not in "iuO":
                raise ValueError(what + ": integers expected")
            if len(a) and int(a.min()) < 0 and what == "begin":
                raise ValueError(what + ": negative")
            if len(a) and (int(a.min()) < 0 or int(a.max()) > most):
                raise ValueError(what + ": does not fit %d bits" % most.bit_length())
            return np.ascontiguousarray(a.astype(dt))

        h_stream = host_table(stream_index, "stream_index", 0xFFFFFFFF, np.uint32)
        h_begin = host_table(begin, "begin", (1 << 64) - 1, np.uint64)
        h_length = host_table(length, "length", 0xFFFFFFFF, np.uint32)
        if on_device:
            stream_index, begin, length = h_stream, h_begin, h_length
    if not on_device:
        first = np.ascontiguousarray(seek_index.first, dtype=np.uint64)
        if len(first) and (int(first[0]) != 0 or (np.diff(first.astype(np.int64)) < 0).any() or int(first[-1]) != len(seek_index.in_pos)):
            raise ValueError("seek_index.first: a running sum from 0 to the number of rows expected")
    if stream is not None and on_device:
        import torch  # (tables and output on the launch stream: see compress_batch)

        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
            return read_ranges_seek(data, in_off, in_len, seek_index=seek_index, stream_index=stream_index, begin=begin, length=length,
                                    dictionary=dictionary, device=device, stream=None)
    lib = _lib.load()
    if on_device:
        import torch

        dev = data.device
        as_t = lambda x, dt: (x if _is_torch(x) else torch.from_numpy(np.asarray(x).astype(np.uint64).view(np.int64))).to(device=dev, dtype=dt)  # noqa: E731
        first_t, in_pos_t = seek_index.first.to(device=dev, dtype=torch.int64), seek_index.in_pos.to(device=dev, dtype=torch.int32).contiguous()
        state_t = seek_index.state.to(device=dev).contiguous()
        if state_t.numel() and state_t.data_ptr() & 15:
            state_t = torch.cat([state_t.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])[: state_t.numel()].reshape(state_t.shape)
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)  # kept alive on the result (async launch)
        stream_t, begin_t, length_t = as_t(stream_index, torch.int32), as_t(begin, torch.int64), as_t(length, torch.int32)
        len64 = length_t.to(torch.int64) & 0xFFFFFFFF  # (lengths are uint32 values, whatever the storage)
        out_off_t = torch.cumsum(len64, 0) - len64
        total = int(len64.sum().item()) if n_ranges else 0
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        out_len_t = torch.empty(n_ranges, dtype=torch.int32, device=dev)
        status_t = torch.empty(n_ranges, dtype=torch.int8, device=dev)
        dict_t = None if dictionary is None else (dictionary if _is_torch(dictionary) else torch.from_numpy(_np_u8(dictionary).copy())).to(dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check_launch(lib.tamp_batch_read_ranges_seek(
            _ptr(dict_t), 0 if dict_t is None else int(dict_t.numel()), w, _ptr(data), _ptr(in_off_t), _ptr(in_len_t), N, _ptr(first_t),
            _ptr(in_pos_t) if in_pos_t.numel() else None, _ptr(state_t) if state_t.numel() else None, stride, _ptr(stream_t), _ptr(begin_t),
            _ptr(length_t), _ptr(out), _ptr(out_off_t), _ptr(out_len_t), _ptr(status_t), n_streams, n_ranges, _lib.MEM_DEVICE,
            dev.index or 0, C.c_void_p(st)))
        return RangeResult(out, out_off_t, out_len_t, status_t, -1.0,
                           (data, in_off_t, in_len_t, first_t, in_pos_t, state_t, stream_t, begin_t, length_t, dict_t, seek_index))
    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    if not flat.size:
        flat = np.zeros(1, np.uint8)
    in_pos = np.ascontiguousarray(seek_index.in_pos, dtype=np.uint32)
    state = np.ascontiguousarray(seek_index.state, dtype=np.uint8)
    if state.size and state.ctypes.data & 15:
        rows = _aligned_rows(*state.shape)
        rows[...] = state
        state = rows
    dict_a = None if dictionary is None else _np_u8(dictionary)
    out_off, total = _slab_offsets(h_length)
    out = np.zeros(total + 1, dtype=np.uint8)
    out_len, status = np.zeros(n_ranges, dtype=np.uint32), np.zeros(n_ranges, dtype=np.int8)
    _lib.check_launch(lib.tamp_batch_read_ranges_seek(
        _ptr(dict_a), 0 if dict_a is None else len(dict_a), w, _ptr(flat), _ptr(in_off), _ptr(in_len), N, _ptr(first),
        _ptr(in_pos) if in_pos.size else None, _ptr(state) if state.size else None, stride, _ptr(h_stream), _ptr(h_begin), _ptr(h_length),
        _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(status), n_streams, n_ranges, _lib.MEM_HOST, device, None))
    return RangeResult(out, out_off, out_len, status)


def _write_tables(stream_index, begin, length, source_off, n_streams):
    """Not part of the package's surface: the host tables of ``write_ranges`` as the C call takes them -- checked, then sorted stably
    by (stream, begin), writes of no bytes first among equals.  -> (stream uint32, begin uint64, length uint32, source_off uint64); ValueError on negative values, values
    that do not fit, a stream index out of range, and writes of one stream that overlap."""
    def table(t, what, most, dt):  # (a sequence goes through Python integers: 2^64 - 1 is one)
        a = t.cpu().numpy() if _is_torch(t) else (t if isinstance(t, np.ndarray) else np.array([int(x) for x in t] or [0], dtype=object)[: len(t)])
        if a.dtype.kind not in "iuO":
            raise ValueError(what + ": integers expected")
        if len(a) and int(a.min()) < 0:
            raise ValueError(what + ": negative")
        if len(a) and int(a.max()) > most:
            raise ValueError(what + ": does not fit %d bits" % most.bit_length())
        return np.ascontiguousarray(a.astype(dt))

    w_stream = table(stream_index, "stream_index", 0xFFFFFFFF, np.uint32)
    w_begin = table(begin, "begin", (1 << 64) - 1, np.uint64)
    w_len = table(length, "length", 0xFFFFFFFF, np.uint32)
    w_src = table(source_off, "source_off", (1 << 64) - 1, np.uint64)
    if len(w_stream) and int(w_stream.max()) >= n_streams:
        raise ValueError("stream_index: out of range")
    # (stable: writes with the same stream and begin keep their order, but one of no bytes goes in front of one that begins where it
    # stands -- behind it, it would stand inside its predecessor)
    order = np.lexsort((w_len != 0, w_begin, w_stream))
    w_stream, w_begin, w_len, w_src = (np.ascontiguousarray(a[order]) for a in (w_stream, w_begin, w_len, w_src))
    if len(w_stream) > 1:
        end = w_begin[:-1] + w_len[:-1].astype(np.uint64)  # (a sum 64 bits do not hold wraps: behind everything)
        same = w_stream[1:] == w_stream[:-1]
        if bool((same & ((w_begin[1:] < end) | (end < w_begin[:-1]))).any()):
            raise ValueError("writes of one stream overlap")
    return w_stream, w_begin, w_len, w_src


def _write_bound(entries, interval: int, literal: int):
    """``compress_resets_bound((E + 1) * interval, interval, literal)`` per stream of ``E`` entries, without the 32-bit mask that
    function puts on lengths: ``E`` closed segments and one more full one.  ``entries``: a uint64 array or an int64 tensor."""
    closed, last = 2 + (interval * (literal + 1) + 16) // 8, 2 + (interval * (literal + 1) + 7) // 8
    if _is_torch(entries):
        return entries * closed + last
    return entries * np.uint64(closed) + np.uint64(last)


def write_ranges(data, in_off=None, in_len=None, *, reset_index, stream_index, begin, source, source_off=None, length=None,
                 reset_interval=None, lazy_matching: bool = False, out_cap=None, max_window_bits: int = 15, device: int = 0, stream=None,
                 timing: bool = False, window=None, literal=None, extended=None) -> BatchResult:
    """Write byte ranges into reset-segmented streams without compressing the rest again (``tamp_batch_write_ranges``, DESIGN.md 3.13;
    not in the reference).  ``data``, ``reset_index`` and ``reset_interval`` as for ``read_ranges``.  Write ``q`` replaces the decoded
    bytes ``[begin[q], begin[q] + length[q])`` of stream ``stream_index[q]``.  ``source``: a sequence of bytes-likes, one per write
    (``source_off`` and ``length`` are then derived), or one flat uint8 buffer (numpy array or CUDA tensor) with ``source_off`` and
    ``length``.  Only the touched segments are decoded, patched and compressed again; the others keep their bytes.  A stream's size
    never changes: a write beyond its end fails the stream with status 2.  The result holds the new streams in slabs, and
    ``res.reset_index`` their index.  For streams ``compress_batch(..., reset_interval=N, reset_index=True)`` made, the result is byte
    for byte what that call makes of the patched data.  ``window``, ``literal``, ``extended``: how the touched segments are compressed;
    they must be the streams' own -- read from the first stream's header for host data, required with CUDA tensors (no sync is hidden).
    Host tables may come in any order (they are sorted by stream and begin; overlapping writes raise ``ValueError``, and so does a write of no bytes INSIDE another); CUDA tables of a
    CUDA call are passed as they are and must be sorted already -- a stream whose writes are not gets status -21.
    ``out_cap=None`` sizes the slabs from the index: no stream of ``E`` entries can take more than ``E + 1`` full segments do."""
    if not isinstance(reset_index, ResetIndex):  # (all decided before the library is looked for)
        raise ValueError("reset_index: a ResetIndex expected")
    on_device = _is_torch(data)
    n_streams = len(data) if in_off is None and not on_device else len(in_len)
    if len(reset_index.first) != n_streams + 1:
        raise ValueError("reset_index.first: one entry per stream and one more expected")
    interval = reset_interval if reset_interval is not None else reset_index.interval
    if interval is None:
        raise ValueError("reset_interval: not given and not in the index")
    if not _is_int(interval) or not 1 <= int(interval) <= 0xFFFFFFFF:
        raise ValueError("reset_interval: a positive integer that fits 32 bits expected")
    interval = int(interval)
    pieces = not _is_torch(source) and not isinstance(source, np.ndarray)
    if pieces:
        if isinstance(source, (bytes, bytearray, memoryview)):
            raise ValueError("source: a sequence of bytes-likes, one per write, or a flat uint8 buffer with source_off and length")
        if source_off is not None or length is not None:
            raise ValueError("source_off and length are derived from a sequence of sources")
        parts = [_np_u8(x) for x in source]
        length = np.array([p.size for p in parts], dtype=np.uint64)
        source_off = np.cumsum(length) - length
        source = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    elif source_off is None or length is None:
        raise ValueError("a flat source needs source_off and length")
    if not len(stream_index) == len(begin) == len(length) == len(source_off):
        raise ValueError("stream_index, begin, length and the sources: one entry per write each")
    if on_device != _is_torch(source) and not (on_device and pieces):
        raise ValueError("source: where the data is (a CUDA tensor with CUDA data)")
    if on_device and (window is None or literal is None or extended is None):
        raise ValueError("window, literal and extended are required with CUDA tensors")
    for name, v, lo, hi in (("window", window, 8, 15), ("literal", literal, 5, 8)):
        if v is not None and (not _is_int(v) or not lo <= int(v) <= hi):
            raise ValueError(f"{name} must be in {lo}..{hi}, not {v!r}")
    if out_cap is not None and not _is_int(out_cap) and len(out_cap) != n_streams:
        raise ValueError("out_cap: one entry per stream expected")
    if _is_int(out_cap) and not 0 <= int(out_cap) <= 0xFFFFFFFF:
        raise ValueError("out_cap: does not fit 32 bits")
    n_writes = len(stream_index)
    tables = (stream_index, begin, length, source_off)
    if not (on_device and all(_is_torch(t) for t in tables)):  # (CUDA tables of a CUDA call: the device check answers for them)
        stream_index, begin, length, source_off = _write_tables(stream_index, begin, length, source_off, n_streams)
    if stream is not None and on_device:
        import torch  # (tables and output on the launch stream: see compress_batch)

        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
            return write_ranges(data, in_off, in_len, reset_index=reset_index, stream_index=stream_index, begin=begin,
                                source=source if _is_torch(source) else torch.from_numpy(source).to(data.device), source_off=source_off,
                                length=length, reset_interval=interval, lazy_matching=lazy_matching, out_cap=out_cap,
                                max_window_bits=max_window_bits, device=device, stream=None, timing=timing, window=window, literal=literal,
                                extended=extended)
    lib = _lib.load()
    lib.tamp_amd_set_timing(1 if timing else 0)
    if on_device:
        import torch

        dev = data.device
        as_t = lambda x, dt: (x if _is_torch(x) else torch.from_numpy(np.asarray(x).astype(np.uint64).view(np.int64))).to(device=dev, dtype=dt)  # noqa: E731
        conf = _conf(int(window), int(literal), extended, None, True, lazy_matching)
        first_t, off_t = as_t(reset_index.first, torch.int64), as_t(reset_index.off, torch.int32)
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)  # kept alive on the result (async launch)
        stream_t, begin_t, length_t = as_t(stream_index, torch.int32), as_t(begin, torch.int64), as_t(length, torch.int32)
        src_off_t = as_t(source_off, torch.int64)
        src_t = source if _is_torch(source) else torch.from_numpy(source).to(dev)
        if out_cap is None:
            cap64 = _write_bound(first_t[1:] - first_t[:-1], interval, int(literal))
            cap64 = torch.maximum(cap64, in_len_t.to(torch.int64) & 0xFFFFFFFF)  # (a stream no write touches is copied as it stands)
            if n_streams and int(cap64.max().item()) > 0xFFFFFFFF:
                raise ValueError("a stream's bound does not fit 32 bits: pass out_cap")
        elif _is_int(out_cap):
            cap64 = torch.full((n_streams,), int(out_cap), dtype=torch.int64, device=dev)
        else:
            cap64 = as_t(out_cap, torch.int64) & 0xFFFFFFFF
        out_cap_t = cap64.to(torch.int32)  # (the low 32 bits: what the library reads as uint32)
        out_off_t = torch.cumsum(cap64, 0) - cap64
        total = int(cap64.sum().item()) if n_streams else 0
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        out_len_t = torch.zeros(n_streams, dtype=torch.int32, device=dev)
        status_t = torch.zeros(n_streams, dtype=torch.int8, device=dev)
        new_off_t = torch.zeros(max(int(off_t.numel()), 1), dtype=torch.int32, device=dev)[: int(off_t.numel())]
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        _lib.check_launch(lib.tamp_batch_write_ranges(
            C.byref(conf), max_window_bits, _ptr(data), _ptr(in_off_t), _ptr(in_len_t), _ptr(first_t), _ptr(off_t) if off_t.numel() else None,
            interval, _ptr(stream_t), _ptr(begin_t), _ptr(length_t), _ptr(src_t if src_t.numel() else torch.zeros(1, dtype=torch.uint8, device=dev)),
            _ptr(src_off_t), _ptr(out), _ptr(out_off_t), _ptr(out_cap_t), _ptr(out_len_t), _ptr(status_t),
            _ptr(new_off_t) if new_off_t.numel() else None, n_streams, n_writes, _lib.MEM_DEVICE, dev.index or 0, C.c_void_p(st)))
        ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
        return BatchResult(out, out_off_t, out_len_t, status_t, None, ms,
                           (data, in_off_t, in_len_t, first_t, off_t, stream_t, begin_t, length_t, src_t, src_off_t, out_cap_t),
                           reset_index=ResetIndex(first_t, new_off_t, interval))
    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    if n_streams and int(in_len[0]) and (window is None or literal is None or extended is None):
        h0 = int(flat[int(in_off[0])])  # (the first stream's header: what every written stream must have)
        window = (h0 >> 5) + 8 if window is None else window
        literal = ((h0 >> 3) & 3) + 5 if literal is None else literal
        extended = bool((h0 >> 1) & 1) if extended is None else extended
    conf = _conf(int(window) if window is not None else 10, int(literal) if literal is not None else 8,
                 True if extended is None else extended, None, True, lazy_matching)
    to_np = lambda x, dt: np.ascontiguousarray((x.cpu().numpy() if _is_torch(x) else np.asarray(x)).astype(dt))  # noqa: E731
    first, off = to_np(reset_index.first, np.uint64), to_np(reset_index.off, np.uint32)
    if not flat.size:
        flat = np.zeros(1, np.uint8)
    src = _np_u8(source)
    if not src.size:
        src = np.zeros(1, np.uint8)
    if out_cap is None:
        out_cap = np.maximum(_write_bound(first[1:] - first[:-1], interval, int(conf.literal)), in_len.astype(np.uint64))
        if n_streams and int(out_cap.max()) > 0xFFFFFFFF:
            raise ValueError("a stream's bound does not fit 32 bits: pass out_cap")
    elif _is_int(out_cap):
        out_cap = np.full(n_streams, int(out_cap), dtype=np.uint32)
    out_cap = np.ascontiguousarray(out_cap, dtype=np.uint32)
    out_off, total = _slab_offsets(out_cap)
    out = np.zeros(total + 1, dtype=np.uint8)
    out_len, status = np.zeros(n_streams, dtype=np.uint32), np.zeros(n_streams, dtype=np.int8)
    new_off = np.zeros(off.size, dtype=np.uint32)
    _lib.check_launch(lib.tamp_batch_write_ranges(
        C.byref(conf), max_window_bits, _ptr(flat), _ptr(in_off), _ptr(in_len), _ptr(first), _ptr(off) if off.size else None, interval,
        _ptr(stream_index), _ptr(begin), _ptr(length), _ptr(src), _ptr(source_off), _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len),
        _ptr(status), _ptr(new_off) if off.size else None, n_streams, n_writes, _lib.MEM_HOST, device,
        C.c_void_p(stream) if stream else None))
    ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
    return BatchResult(out, out_off, out_len, status, None, ms, reset_index=ResetIndex(first, new_off, interval))


def _append_tables(source, source_off, length, stream_index, n_streams, on_device):
    """Not part of the package's surface: the per-stream source tables of ``append_batch`` from what the caller gave.
    -> (source, source_off, length): a flat uint8 buffer and one row per STREAM; host arrays (uint64, uint32) unless all three came
    as CUDA tensors with no ``stream_index``, which are passed as they are.  ValueError on anything that does not fit."""
    pieces = not _is_torch(source) and not isinstance(source, np.ndarray)
    if pieces:
        if isinstance(source, (bytes, bytearray, memoryview)):
            raise ValueError("source: a sequence of bytes-likes, one per stream, or a flat uint8 buffer with source_off and length")
        if source_off is not None or length is not None:
            raise ValueError("source_off and length are derived from a sequence of sources")
        parts = [_np_u8(b"" if x is None else x) for x in source]
        length = np.array([p.size for p in parts], dtype=np.uint64)
        source_off = np.cumsum(length) - length if len(parts) else np.zeros(0, np.uint64)
        source = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    elif source_off is None or length is None:
        raise ValueError("a flat source needs source_off and length")
    if on_device != _is_torch(source) and not (on_device and pieces):
        raise ValueError("source: where the data is (a CUDA tensor with CUDA data)")
    rows = n_streams if stream_index is None else len(stream_index)
    if not len(source_off) == len(length) == rows:
        raise ValueError("the sources: one per stream, or one per entry of stream_index")
    if stream_index is None and on_device and _is_torch(source_off) and _is_torch(length):
        return source, source_off, length  # (CUDA tables of a CUDA call: nobody looks at them, no sync)

    def table(t, what, most, dt):  # (a sequence goes through Python integers: 2^64 - 1 is one)
        a = t.cpu().numpy() if _is_torch(t) else (t if isinstance(t, np.ndarray) else np.array([int(x) for x in t] or [0], dtype=object)[: len(t)])
        if a.dtype.kind not in "iuO":
            raise ValueError(what + ": integers expected")
        if len(a) and int(a.min()) < 0:
            raise ValueError(what + ": negative")
        if len(a) and int(a.max()) > most:
            raise ValueError(what + ": does not fit %d bits" % most.bit_length())
        return np.ascontiguousarray(a.astype(dt))

    h_off, h_len = table(source_off, "source_off", (1 << 64) - 1, np.uint64), table(length, "length", 0xFFFFFFFF, np.uint32)
    if stream_index is None:
        return source, h_off, h_len
    idx = table(stream_index, "stream_index", 0xFFFFFFFF, np.uint32).astype(np.int64)
    if len(idx) and int(idx.max()) >= n_streams:
        raise ValueError("stream_index: out of range")
    if len(np.unique(idx)) != len(idx):
        raise ValueError("stream_index: a stream is named twice")
    full_off, full_len = np.zeros(n_streams, np.uint64), np.zeros(n_streams, np.uint32)
    full_off[idx], full_len[idx] = h_off, h_len
    return source, full_off, full_len


def append_batch(data, in_off=None, in_len=None, *, reset_index, source, source_off=None, length=None, stream_index=None,
                 reset_interval=None, lazy_matching: bool = False, out_cap=None, max_window_bits: int = 15, device: int = 0, stream=None,
                 timing: bool = False, window=None, literal=None, extended=None) -> BatchResult:
    """Append bytes to reset-segmented streams so that they stay seekable (``tamp_batch_append``; not in the reference,
    whose append mode opens with a reset wherever the stream ended).  ``data``, ``reset_index`` and ``reset_interval`` as for
    ``read_ranges``.  ``source``: one bytes-like per stream, ``b""`` or ``None`` for none -- with ``stream_index=[...]`` one per named
    stream (a stream named twice or out of range raises ``ValueError``) -- or one flat uint8 buffer (numpy array or CUDA tensor) with
    per-stream ``source_off`` and ``length``.  Only a stream's open segment is decoded; its bytes and the new ones are cut at every
    ``reset_interval`` bytes and compressed, and every byte in front of the open segment keeps its place.  For streams
    ``compress_batch(..., reset_interval=N, reset_index=True)`` made, streams and index are byte for byte what that call makes of
    old data + appended.  ``window``, ``literal``, ``extended``: the streams' own -- read from the first stream's header for host
    data, required with CUDA tensors.  ``out_cap=None``: a stream's length plus ``ceil(L / N) + 1`` full closed segments.  The result's
    ``reset_index`` is the new index; with CUDA tensors its ``off`` is sized by the bound ``entries + sum(ceil(L / N))`` and may have
    spare entries behind ``first[n]``: every call that takes an index takes it as it stands."""
    if not isinstance(reset_index, ResetIndex):  # (all decided before the library is looked for)
        raise ValueError("reset_index: a ResetIndex expected")
    on_device = _is_torch(data)
    n_streams = len(data) if in_off is None and not on_device else len(in_len)
    if len(reset_index.first) != n_streams + 1:
        raise ValueError("reset_index.first: one entry per stream and one more expected")
    interval = reset_interval if reset_interval is not None else reset_index.interval
    if interval is None:
        raise ValueError("reset_interval: not given and not in the index")
    if not _is_int(interval) or not 1 <= int(interval) <= 0xFFFFFFFF:
        raise ValueError("reset_interval: a positive integer that fits 32 bits expected")
    interval = int(interval)
    source, source_off, length = _append_tables(source, source_off, length, stream_index, n_streams, on_device)
    if on_device and (window is None or literal is None or extended is None):
        raise ValueError("window, literal and extended are required with CUDA tensors")
    for name, v, lo, hi in (("window", window, 8, 15), ("literal", literal, 5, 8)):
        if v is not None and (not _is_int(v) or not lo <= int(v) <= hi):
            raise ValueError(f"{name} must be in {lo}..{hi}, not {v!r}")
    if out_cap is not None and not _is_int(out_cap) and len(out_cap) != n_streams:
        raise ValueError("out_cap: one entry per stream expected")
    if _is_int(out_cap) and not 0 <= int(out_cap) <= 0xFFFFFFFF:
        raise ValueError("out_cap: does not fit 32 bits")
    if stream is not None and on_device:
        import torch  # (tables and output on the launch stream: see compress_batch)

        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
            return append_batch(data, in_off, in_len, reset_index=reset_index,
                                source=source if _is_torch(source) else torch.from_numpy(source).to(data.device), source_off=source_off,
                                length=length, reset_interval=interval, lazy_matching=lazy_matching, out_cap=out_cap,
                                max_window_bits=max_window_bits, device=device, stream=None, timing=timing, window=window, literal=literal,
                                extended=extended)
    if on_device:
        import torch

        dev = data.device
        as_t = lambda x, dt: (x if _is_torch(x) else torch.from_numpy(np.asarray(x).astype(np.uint64).view(np.int64))).to(device=dev, dtype=dt)  # noqa: E731
        conf = _conf(int(window), int(literal), extended, None, True, lazy_matching)
        first_t, off_t = as_t(reset_index.first, torch.int64), as_t(reset_index.off, torch.int32)
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)  # kept alive on the result (async launch)
        src_off_t, src_len_t = as_t(source_off, torch.int64), as_t(length, torch.int32)
        src_t = source if _is_torch(source) else torch.from_numpy(source).to(dev)
        if not src_t.numel():
            src_t = torch.zeros(1, dtype=torch.uint8, device=dev)
        more = ((src_len_t.to(torch.int64) & 0xFFFFFFFF) + (interval - 1)) // interval  # (lengths are uint32 values, whatever the storage)
        if out_cap is None:
            cap64 = (in_len_t.to(torch.int64) & 0xFFFFFFFF) + (more + 1) * _append_closed_bound(interval, int(literal))
        elif _is_int(out_cap):
            cap64 = torch.full((n_streams,), int(out_cap), dtype=torch.int64, device=dev)
        else:
            cap64 = as_t(out_cap, torch.int64) & 0xFFFFFFFF
        # (one look at the device for what sizes the buffers: the slabs' total, their largest, the bound of the new entries)
        total, most, fresh = (int(v) for v in torch.stack([cap64.sum(), cap64.max(), more.sum()]).tolist()) if n_streams else (0, 0, 0)
        if out_cap is None and most > 0xFFFFFFFF:
            raise ValueError("a stream's bound does not fit 32 bits: pass out_cap")
        out_cap_t = cap64.to(torch.int32)  # (the low 32 bits: what the library reads as uint32)
        out_off_t = torch.cumsum(cap64, 0) - cap64
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        out_len_t = torch.zeros(n_streams, dtype=torch.int32, device=dev)
        status_t = torch.zeros(n_streams, dtype=torch.int8, device=dev)
        new_cap = int(off_t.numel()) + fresh  # (reset_first[n] <= the entries the old table has room for)
        new_first_t = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
        new_off_t = torch.zeros(max(new_cap, 1), dtype=torch.int32, device=dev)[:new_cap]
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        lib = _lib.load()
        lib.tamp_amd_set_timing(1 if timing else 0)
        _lib.check_launch(lib.tamp_batch_append(
            C.byref(conf), max_window_bits, _ptr(data), _ptr(in_off_t), _ptr(in_len_t), _ptr(first_t), _ptr(off_t) if off_t.numel() else None,
            interval, _ptr(src_t), _ptr(src_off_t), _ptr(src_len_t), _ptr(out), _ptr(out_off_t), _ptr(out_cap_t), _ptr(out_len_t),
            _ptr(status_t), _ptr(new_first_t), _ptr(new_off_t) if new_cap else None, new_cap, n_streams, _lib.MEM_DEVICE, dev.index or 0,
            C.c_void_p(st)))
        ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
        return BatchResult(out, out_off_t, out_len_t, status_t, None, ms,
                           (data, in_off_t, in_len_t, first_t, off_t, src_t, src_off_t, src_len_t, out_cap_t),
                           reset_index=ResetIndex(new_first_t, new_off_t, interval))
    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    if n_streams and int(in_len[0]) and (window is None or literal is None or extended is None):
        h0 = int(flat[int(in_off[0])])  # (the first stream's header: what every stream that is appended to must have)
        window = (h0 >> 5) + 8 if window is None else window
        literal = ((h0 >> 3) & 3) + 5 if literal is None else literal
        extended = bool((h0 >> 1) & 1) if extended is None else extended
    conf = _conf(int(window) if window is not None else 10, int(literal) if literal is not None else 8,
                 True if extended is None else extended, None, True, lazy_matching)
    to_np = lambda x, dt: np.ascontiguousarray((x.cpu().numpy() if _is_torch(x) else np.asarray(x)).astype(dt))  # noqa: E731
    first, off = to_np(reset_index.first, np.uint64), to_np(reset_index.off, np.uint32)
    if not flat.size:
        flat = np.zeros(1, np.uint8)
    src = _np_u8(source)
    if not src.size:
        src = np.zeros(1, np.uint8)
    more = (length.astype(np.uint64) + np.uint64(interval - 1)) // np.uint64(interval)
    if out_cap is None:
        out_cap = in_len.astype(np.uint64) + (more + np.uint64(1)) * np.uint64(_append_closed_bound(interval, int(conf.literal)))
        if n_streams and int(out_cap.max()) > 0xFFFFFFFF:
            raise ValueError("a stream's bound does not fit 32 bits: pass out_cap")
    elif _is_int(out_cap):
        out_cap = np.full(n_streams, int(out_cap), dtype=np.uint32)
    out_cap = np.ascontiguousarray(out_cap, dtype=np.uint32)
    out_off, total = _slab_offsets(out_cap)
    out = np.zeros(total + 1, dtype=np.uint8)
    out_len, status = np.zeros(n_streams, dtype=np.uint32), np.zeros(n_streams, dtype=np.int8)
    new_cap = (int(first[n_streams]) if n_streams else 0) + int(more.sum())
    new_first, new_off = np.zeros(n_streams + 1, dtype=np.uint64), np.zeros(max(new_cap, 1), dtype=np.uint32)
    lib = _lib.load()
    lib.tamp_amd_set_timing(1 if timing else 0)
    _lib.check_launch(lib.tamp_batch_append(
        C.byref(conf), max_window_bits, _ptr(flat), _ptr(in_off), _ptr(in_len), _ptr(first), _ptr(off) if off.size else None, interval,
        _ptr(src), _ptr(source_off), _ptr(length), _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status), _ptr(new_first),
        _ptr(new_off) if new_cap else None, new_cap, n_streams, _lib.MEM_HOST, device, C.c_void_p(stream) if stream else None))
    ms = lib.tamp_amd_last_kernel_ms() if timing else -1.0
    return BatchResult(out, out_off, out_len, status, None, ms,
                       reset_index=ResetIndex(new_first, new_off[: int(new_first[n_streams])].copy(), interval))


def _append_closed_bound(interval: int, literal: int) -> int:
    """Bytes a closed segment of ``interval`` bytes can take at most (reset_segment_bound with the FLUSH token)."""
    return 2 + (interval * (literal + 1) + 16) // 8


@dataclass
class ResetScan:
    """What ``index_resets`` found: the batch's ``ResetIndex`` and, from the token grammar alone, the decoded sizes."""
    index: ResetIndex
    status: object       # int8 [n] -- per stream (include/tamp_amd.h, tamp_batch_index_resets)
    closed_size: object  # uint32/int32 [entries] -- decoded bytes of the segment each reset closes (0xFFFFFFFF: 2^32 - 1 or more)
    open_size: object    # uint32/int32 [n] -- decoded bytes of each stream's last (open) segment
    kernel_ms: float = -1.0
    _keep: object = None  # device tensors the asynchronous launch still reads

    def size(self, i: int) -> int:
        """Decoded bytes of stream ``i``: its closed segments and its open one."""
        a, b = int(self.index.first[i]), int(self.index.first[i + 1])
        closed = self.closed_size[a:b]
        closed = closed.cpu().numpy() if _is_torch(closed) else np.asarray(closed)
        return int((closed.astype(np.int64) & 0xFFFFFFFF).sum()) + (int(self.open_size[i]) & 0xFFFFFFFF)

    def segment_ends(self, *, device: int = 0, stream=None):
        """The table of segment ends of the scanned batch, for ``read_ranges(..., segment_ends=)``: see ``segment_ends``.  Made once,
        where the scan's tables live, and kept on the object."""
        if self._segment_ends is None:
            self._segment_ends = segment_ends(self.index.first, self.closed_size, self.open_size, device=device, stream=stream)
        return self._segment_ends

    _segment_ends = None  # (a class attribute until the first call: no field, so the dataclass is what it was)


def segment_ends(first, closed_size, open_size, *, device: int = 0, stream=None):
    """The table of segment ends (``tamp_batch_segment_ends``; not in the reference) from an index's ``first`` and the
    sizes ``index_resets`` found: one uint64 entry per SEGMENT, stream ``i``'s at ``[first[i] + i, first[i + 1] + i + 1)``, entry ``k``
    the decoded size of its segments ``0 .. k`` -- the last one the stream's decoded size.  numpy tables give a numpy table, computed
    on the host; CUDA tensors give an int64 tensor, computed on the device with no read-back and no wait."""
    n = len(first) - 1
    if n < 0 or len(open_size) != n:
        raise ValueError("first: one entry per stream and one more expected, open_size: one per stream")
    on_device = _is_torch(first) and first.is_cuda
    if any((_is_torch(t) and t.is_cuda) != on_device for t in (closed_size, open_size)):
        raise ValueError("first, closed_size and open_size: on one memory kind expected")
    lib = _lib.load()
    if on_device:
        import torch

        dev = first.device
        first_t, open_t = first.to(torch.int64).contiguous(), open_size.to(torch.int32).contiguous()
        closed_t = closed_size.to(torch.int32).contiguous() if closed_size.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        if stream is not None:
            with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=dev)):
                ends = torch.empty(max(len(closed_size) + n, 1), dtype=torch.int64, device=dev)
        else:
            ends = torch.empty(max(len(closed_size) + n, 1), dtype=torch.int64, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        _lib.check_launch(lib.tamp_batch_segment_ends(_ptr(first_t), _ptr(closed_t), _ptr(open_t), _ptr(ends), n, _lib.MEM_DEVICE,
                                                      dev.index or 0, C.c_void_p(st)))
        ends = ends[: len(closed_size) + n]
        ends._tamp_keep = (first_t, closed_t, open_t)  # (the asynchronous launch still reads them)
        return ends
    to_np = lambda x, dt: np.ascontiguousarray((x.numpy() if _is_torch(x) else np.asarray(x)).astype(dt))  # noqa: E731
    first, closed, open_size = to_np(first, np.uint64), to_np(closed_size, np.uint32), to_np(open_size, np.uint32)
    if int(first[n]) != len(closed):
        raise ValueError("closed_size: first[-1] entries expected")
    ends = np.zeros(max(len(closed) + n, 1), dtype=np.uint64)
    _lib.check_launch(lib.tamp_batch_segment_ends(_ptr(first), _ptr(closed) if closed.size else None, _ptr(open_size), _ptr(ends), n,
                                                  _lib.MEM_HOST, device, None))
    return ends[: len(closed) + n]


def _detect_interval(first, closed, open_size, status):
    """``ResetIndex.interval`` of a found index (numpy tables): the one size of all closed segments of the ``TAMP_OK`` streams,
    when there is a closed segment and no open segment is larger -- else ``None``."""
    counts = np.diff(first.astype(np.int64))
    ok = np.repeat(status == 0, counts)
    sizes = closed[ok]
    if not sizes.size or int(sizes.min()) != int(sizes.max()):
        return None
    return int(sizes[0]) if not open_size.size or int(open_size.max()) <= int(sizes[0]) else None


def index_resets(data, in_off=None, in_len=None, *, max_window_bits: int = 15, device: int = 0, stream=None,
                 timing: bool = False) -> ResetScan:
    """The reset index of streams that came without one (``tamp_batch_index_resets``; not in the reference): a blob
    of ``compress(..., dictionary_reset=True, reset_interval=N)``, a file, a batch whose index was not kept, anything a reference
    ``Compressor(dictionary_reset=True)`` wrote with ``reset_dictionary()`` calls of its own.  ``data`` as for ``decompress_batch``:
    a list of bytes, numpy tables or CUDA tensors.  The resets are found on the device, from the token grammar alone; nothing is
    decoded.  ``status[i]`` is 0, 2 (shorter than its header), -3 (header), -4 (an offset out of the window: entries and sizes still
    as the grammar says) or -21 (too long); a refused stream has no entries.  ``index`` goes to ``read_ranges`` and
    ``decompress_batch(..., reset_index=)`` as it stands: they verify what they use.  ``index.interval`` is filled when the batch has
    a closed segment, all closed segments of the status-0 streams decode to the same number of bytes and no open segment is larger.
    The first call has room for ``max(n, total_bytes >> 12)`` entries; when there are more, the library says how many and ONE more
    call is made with exactly that room.  CUDA tensors: the entry count and the interval check are the only waits beyond the
    library's own (one per round of its start search)."""
    if not _is_int(max_window_bits) or not 8 <= int(max_window_bits) <= 15:  # (all decided before the library is looked for)
        raise ValueError("max_window_bits: 8 .. 15 expected")
    if (in_off is None) != (in_len is None):
        raise ValueError("in_off and in_len: both or neither")
    if in_off is not None and len(in_off) != len(in_len):
        raise ValueError("in_off and in_len: one entry per stream each")
    on_device = _is_torch(data)
    if on_device and in_off is None:
        raise ValueError("a CUDA buffer needs in_off and in_len")
    if stream is not None and on_device:
        import torch  # (tables and output on the launch stream: see compress_batch)

        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
            return index_resets(data, in_off, in_len, max_window_bits=max_window_bits, device=device, stream=None, timing=timing)
    lib = _lib.load()
    lib.tamp_amd_set_timing(1 if timing else 0)
    total_ms = 0.0

    def call(args, first_n, cap, make):  # -> (reset_off, closed_size), the retry included
        nonlocal total_ms
        for attempt in (0, 1):
            off, closed = make(cap)
            rc = lib.tamp_batch_index_resets(*args(off if cap else None, closed if cap else None, cap))
            total_ms += lib.tamp_amd_last_kernel_ms() if timing else 0.0
            if rc != 1 or attempt:
                break
            cap = first_n()
        if rc == 1:
            raise RuntimeError("tamp_amd: the entry count changed between two calls")
        _lib.check_launch(rc)
        return off, closed

    if on_device:
        import torch

        dev = data.device
        n = len(in_len)
        in_off_t, in_len_t = in_off.to(torch.int64), in_len.to(torch.int32)  # kept alive on the result (async launch)
        first_t = torch.empty(n + 1, dtype=torch.int64, device=dev)
        open_t = torch.empty(n, dtype=torch.int32, device=dev)
        status_t = torch.empty(n, dtype=torch.int8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        off_t, closed_t = call(
            lambda off, closed, cap: (max_window_bits, _ptr(data), _ptr(in_off_t), _ptr(in_len_t), _ptr(first_t), _ptr(off), _ptr(closed),
                                      _ptr(open_t), cap, _ptr(status_t), n, _lib.MEM_DEVICE, dev.index or 0, C.c_void_p(st)),
            lambda: int(first_t[n].item()), max(n, data.numel() >> 12),
            lambda cap: (torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)))
        entries = int(first_t[n].item())
        off_t, closed_t = off_t[:entries], closed_t[:entries]
        interval = None
        if entries:
            ok = torch.repeat_interleave(status_t == 0, first_t[1:] - first_t[:-1], output_size=entries)
            sizes = closed_t.to(torch.int64) & 0xFFFFFFFF  # (masked without a compaction: that would be one more wait)
            lo, hi = torch.where(ok, sizes, 1 << 32).min(), torch.where(ok, sizes, -1).max()
            found = torch.where((lo == hi) & ((open_t.to(torch.int64) & 0xFFFFFFFF).max() <= lo), lo, -1)
            found = int(found.item())
            interval = found if found >= 0 else None
        return ResetScan(ResetIndex(first_t, off_t, interval), status_t, closed_t, open_t, total_ms if timing else -1.0,
                         (data, in_off_t, in_len_t))
    if in_off is None:
        flat, in_off, in_len = pack_streams(data)
    else:
        flat = _np_u8(data)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    n = len(in_len)
    if not flat.size:
        flat = np.zeros(1, np.uint8)
    first = np.zeros(n + 1, dtype=np.uint64)
    open_size, status = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int8)
    off, closed = call(
        lambda off, closed, cap: (max_window_bits, _ptr(flat), _ptr(in_off), _ptr(in_len), _ptr(first), _ptr(off), _ptr(closed),
                                  _ptr(open_size), cap, _ptr(status), n, _lib.MEM_HOST, device, C.c_void_p(stream) if stream else None),
        lambda: int(first[n]), max(n, int(in_len.sum(dtype=np.uint64)) >> 12),
        lambda cap: (np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)))
    entries = int(first[n])
    off, closed = off[:entries], closed[:entries]
    return ResetScan(ResetIndex(first, off, _detect_interval(first, closed, open_size, status)), status, closed, open_size,
                     total_ms if timing else -1.0)


@dataclass
class PackedBatch:
    """A batch's streams back to back in one buffer (``pack_batch``, ``BatchResult.packed``): stream ``i`` is
    ``data[off[i] : off[i] + len[i]]``, and ``off[-1]`` is the packed size.  numpy arrays (uint8, uint64, uint32) or CUDA tensors
    (uint8, int64, int32), like the other tables.  With ``out=`` the caller compares ``off[-1]`` with ``out.numel()``: a batch that
    did not fit left ``data`` untouched."""
    data: object  # uint8
    off: object   # n + 1 entries
    len: object   # n entries
    _keep: object = None  # device tensors the asynchronous launch still reads (the source, converted tables)

    def stream(self, i: int) -> bytes:
        o, n = int(self.off[i]), int(self.len[i])
        chunk = self.data[o : o + n]
        return bytes(chunk.cpu().numpy()) if _is_torch(chunk) else chunk.tobytes()

    def streams(self):
        """Every stream's bytes: ONE device-to-host copy of the packed bytes (and one of each table), sliced on the host."""
        h = self.cpu()
        flat = h.data.tobytes()
        return [flat[o : o + n] for o, n in zip(h.off[:-1].tolist(), h.len.tolist())]

    def triple(self):
        """``(data, in_off, in_len)``: what ``decompress_batch`` / ``decoded_size_batch`` take positionally."""
        return self.data, self.off[:-1], self.len

    def cpu(self) -> "PackedBatch":
        """The same batch in numpy arrays (itself when it is there already)."""
        if not _is_torch(self.data):
            return self
        off = self.off.cpu().numpy().astype(np.uint64)
        data = self.data[: min(int(off[-1]), int(self.data.numel()))].cpu().numpy()
        return PackedBatch(data, off, self.len.cpu().numpy().view(np.uint32))


def pack_batch(data, off, length, *, align: int = 1, out=None, device: int = 0, stream=None) -> PackedBatch:
    """Streams ``data[off[i] : off[i] + length[i]]``, in any order and with any gaps, copied back to back (``tamp_batch_pack``).

    Stream ``i`` lands at ``result.off[i]``, the running sum of the lengths rounded up to ``align`` (a power of two in 1..4096);
    the bytes between its end and ``result.off[i + 1]`` are zero.  No codec work: the result's ``triple()`` decodes like the slabs.
    With CUDA tensors (``off`` int64, ``length`` int32) the copy is a kernel on torch's current stream (or ``stream``): the sizes
    are found first, ONE ``.item()`` reads the total, exactly that is allocated and then filled.  ``out=`` (a CUDA uint8 tensor)
    takes the place of the allocation: one asynchronous call and no sync, and the caller compares ``result.off[-1]`` with
    ``out.numel()`` -- a batch that does not fit leaves ``out`` untouched.  ``data`` and ``out`` must not overlap.
    With numpy arrays the streams are packed on the host, by numpy.
    """
    if isinstance(align, bool) or not isinstance(align, numbers.Integral) or not 1 <= align <= 4096 or align & (align - 1):
        raise ValueError(f"align must be a power of two in 1..4096, not {align!r}")
    align = int(align)
    if len(off) != len(length):
        raise ValueError("one offset and one length per stream expected")
    if not _is_torch(data):
        if out is not None:
            raise ValueError("out= needs CUDA tensors: host arrays are packed into a new array")
        flat = _np_u8(data)
        src_off = np.ascontiguousarray(off, dtype=np.uint64)
        src_len = np.ascontiguousarray(length, dtype=np.uint32)
        if len(src_len) and int((src_off + src_len.astype(np.uint64)).max()) > flat.size:
            raise ValueError("a stream ends behind the data")
        dst_off = np.zeros(len(src_len) + 1, dtype=np.uint64)
        np.cumsum((src_len.astype(np.uint64) + np.uint64(align - 1)) & ~np.uint64(align - 1), out=dst_off[1:])
        packed = np.zeros(int(dst_off[-1]), dtype=np.uint8)
        for o, s, n in zip(dst_off[:-1].tolist(), src_off.tolist(), src_len.tolist()):
            packed[o : o + n] = flat[s : s + n]
        return PackedBatch(packed, dst_off, src_len)
    if not data.is_cuda:
        raise ValueError("data: a CUDA tensor or a host array expected")
    if out is not None and not (_is_torch(out) and out.is_cuda and "uint8" in str(out.dtype) and out.dim() == 1 and out.is_contiguous()):
        raise ValueError("out: a contiguous 1-D CUDA uint8 tensor expected")
    import torch

    if stream is not None:  # (tables and the packed buffer on the launch stream: see compress_batch)
        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=data.device)):
            return pack_batch(data, off, length, align=align, out=out, device=device, stream=None)
    lib = _lib.load()
    dev = data.device
    n = int(length.numel())
    src = data.contiguous().reshape(-1)
    if not src.numel():
        src = torch.zeros(1, dtype=torch.uint8, device=dev)  # (a batch of empty streams: a byte to point at)
    src_off_t = off.to(device=dev, dtype=torch.int64).contiguous()
    src_len_t = length.to(device=dev, dtype=torch.int32).contiguous()
    dst_off_t = torch.empty(n + 1, dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    # (no streams: the tables are empty tensors without an address, and the call refuses null tables)
    tables = (_ptr(src_off_t), _ptr(src_len_t)) if n else (_ptr(dst_off_t), _ptr(dst_off_t))

    def call(dst, cap):
        _lib.check_launch(lib.tamp_batch_pack(_ptr(src), *tables, _ptr(dst) if cap else None, cap, _ptr(dst_off_t), n, align,
                                              dev.index or 0, st))

    if out is None:
        call(None, 0)
        out = torch.empty(int(dst_off_t[-1].item()), dtype=torch.uint8, device=dev)
    call(out, int(out.numel()))
    # the launch is asynchronous: the source and the converted tables must outlive it (they ride on the result)
    return PackedBatch(out, dst_off_t, src_len_t, (src, src_off_t, src_len_t))


class DecoderBatch:
    """``n`` resumable decoder objects advanced together, one launch per step (``tamp_batch_decompress_resume``).

    Each object is what the reference's ``TampDecompressor`` is (tamp/_c_src/tamp/decompressor.h:13-57): its state and
    window survive between steps, so a stream may arrive in pieces of any size and be decoded into output buffers of
    any size -- e.g. many network connections decoded as their packets come in.  ``step(chunks, out_caps)`` offers
    object ``i`` the bytes ``chunks[i]`` and ``out_caps[i]`` bytes of room and returns per object the reference's
    status code (1 output full, 2 input exhausted, negative = error), the bytes produced and the number of input bytes
    consumed; what was not consumed must be offered again.  ``conf`` = None reads the header from each stream;
    a ``dictionary`` is placed in every object's window (used by streams whose header has the custom bit).
    """

    def __init__(self, n: int, *, window_bits: int = 15, conf: Optional[TampAmdConf] = None, dictionary=None,
                 device: int = 0):
        lib = _lib.load()
        self.n, self.window_bits, self.device = n, window_bits, device
        self.stride = (lib.tamp_amd_decoder_state_size(window_bits) + 15) & ~15
        if conf is not None and conf.use_custom_dictionary and dictionary is None:
            raise ValueError("custom dictionary expected")
        one = np.zeros(self.stride, dtype=np.uint8)
        if dictionary is not None:  # the window buffer holds the dictionary, as with the reference's object
            d = _np_u8(dictionary)[: 1 << window_bits]
            one[16 : 16 + len(d)] = d
        res = lib.tamp_amd_decoder_state_init(_ptr(one), C.byref(conf) if conf is not None else None, window_bits)
        if res != _lib.OK:
            raise ValueError(f"tamp_amd_decoder_state_init -> {res}")
        self.states = np.tile(one, (n, 1))

    def step(self, chunks: Sequence, out_caps):
        lib = _lib.load()
        flat, in_off, in_len = pack_streams(chunks)
        # one call looks at 2^28 bytes per object at most (32-bit bit counters) and reports what it consumed
        in_len = np.minimum(in_len, np.uint32(1 << 28))
        out_cap = np.ascontiguousarray(np.broadcast_to(np.asarray(out_caps, dtype=np.uint32), (self.n,)))
        out_off, total = _slab_offsets(out_cap)
        out = np.zeros(total + 1, dtype=np.uint8)
        out_len = np.zeros(self.n, dtype=np.uint32)
        status = np.zeros(self.n, dtype=np.int8)
        consumed = np.zeros(self.n, dtype=np.uint32)
        rc = lib.tamp_batch_decompress_resume(_ptr(self.states), self.stride, self.window_bits,
                                              _ptr(flat if flat.size else np.zeros(1, np.uint8)), _ptr(in_off),
                                              _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len),
                                              _ptr(status), _ptr(consumed), self.n, _lib.MEM_HOST, self.device, None)
        _lib.check_launch(rc)
        outs = [out[int(out_off[i]) : int(out_off[i]) + int(out_len[i])].tobytes() for i in range(self.n)]
        return status, outs, consumed


class EncoderBatch:
    """``n`` compressor objects below flush granularity, advanced together (``tamp_batch_compress_resume``).

    Each object is the reference's ``TampCompressor`` (tamp/_c_src/tamp/compressor.h:13-66): the 16-byte input ring,
    a growing RLE run / extended match, pending output bits and the window all survive between calls, so input may
    arrive in pieces of any size and output buffers may be as small as the reference allows.  Every method runs the
    reference's call of the same name on all objects in one launch and returns per object
    ``(status, bytes, consumed)``.  Whole segments belong to ``compress_batch`` / ``Compressor``.
    """

    def __init__(self, n: int, *, window: int = 10, literal: int = 8, extended: bool = True, dictionary=None,
                 dictionary_reset: bool = False, append: bool = False, lazy_matching: bool = False, device: int = 0):
        lib = _lib.load()
        conf = _conf(window, literal, extended, dictionary, dictionary_reset, lazy_matching)
        self.n, self.window_bits, self.device = n, window, device
        self.stride = (lib.tamp_amd_encoder_state_size(window) + 15) & ~15
        one = np.zeros(self.stride, dtype=np.uint8)
        if dictionary is not None:
            if len(dictionary) != (1 << window):
                raise ValueError("Dictionary-window size mismatch.")
            one[40 : 40 + (1 << window)] = _np_u8(dictionary)
        res = lib.tamp_amd_encoder_state_init(_ptr(one), C.byref(conf), int(append), window)
        if res != _lib.OK:
            raise ValueError(f"tamp_amd_encoder_state_init -> {res}")
        self.states = np.tile(one, (n, 1))

    def _run(self, op: int, chunks, out_caps, write_token: bool = False):
        lib = _lib.load()
        if chunks is None:
            chunks = [b""] * self.n
        flat, in_off, in_len = pack_streams(chunks)
        out_cap = np.ascontiguousarray(np.broadcast_to(np.asarray(out_caps, dtype=np.uint32), (self.n,)))
        out_off, total = _slab_offsets(out_cap)
        out = np.zeros(total + 1, dtype=np.uint8)
        out_len = np.zeros(self.n, dtype=np.uint32)
        status = np.zeros(self.n, dtype=np.int8)
        consumed = np.zeros(self.n, dtype=np.uint32)
        rc = lib.tamp_batch_compress_resume(_ptr(self.states), self.stride, self.window_bits, op, int(write_token),
                                            _ptr(flat if flat.size else np.zeros(1, np.uint8)), _ptr(in_off), _ptr(in_len),
                                            _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                            _ptr(consumed), self.n, _lib.MEM_HOST, self.device, None)
        _lib.check_launch(rc)
        outs = [out[int(out_off[i]) : int(out_off[i]) + int(out_len[i])].tobytes() for i in range(self.n)]
        return status, outs, consumed

    def poll(self, out_caps):
        return self._run(_lib.OP_POLL, None, out_caps)

    def compress(self, chunks: Sequence, out_caps):
        return self._run(_lib.OP_COMPRESS, chunks, out_caps)

    def flush(self, out_caps, write_token: bool = True):
        return self._run(_lib.OP_FLUSH, None, out_caps, write_token)

    def compress_and_flush(self, chunks: Sequence, out_caps, write_token: bool = False):
        return self._run(_lib.OP_COMPRESS_AND_FLUSH, chunks, out_caps, write_token)

    def sink(self, chunks: Sequence):
        """tamp_compressor_sink (compressor.c:665-679): bytes into the rings, host side (a buffer copy, no codec work)."""
        taken = np.zeros(self.n, dtype=np.uint32)
        for i, ch in enumerate(chunks):
            st = self.states[i]
            size, pos = int(st[7]), int(st[8])
            k = min(16 - size, len(ch))
            for j in range(k):
                st[12 + ((pos + size + j) & 15)] = ch[j]
            st[7] = size + k
            taken[i] = k
        return taken

    def full(self):
        return self.states[:, 7] == 16


class CompressorBatch:
    """``n`` streaming compressors on the device, advanced together: ``tamp_amd.Compressor`` for thousands of open streams.

    Stream ``i`` is ONE reference ``Compressor`` with the same keywords: the concatenation of everything the calls below have
    returned for it is, byte for byte, what that object writes for the same sequence of ``write`` / ``flush`` /
    ``reset_dictionary`` / ``close`` calls (per call the boundaries may differ by the up to 31 bits the reference's object holds
    back).  Message ``k`` of a stream therefore matches against its messages ``0..k-1``, which independent streams
    (``compress_batch``) cannot.  Every call is ONE ``tamp_batch_compress_pieces`` launch sequence over all streams
    (include/tamp_amd.h): there is no gather threshold, a ``write`` sends every non-empty chunk as an unfinished piece at once.

    The objects (48 bytes + window each) live in one CUDA uint8 tensor ``objects`` of shape ``(n, stride)`` and never leave the
    device; the per-stream bookkeeping of ``codec.Compressor`` (header sent, window carried, data since the last flush point,
    last token was a FLUSH) is numpy arrays on the host.  Each method returns a ``BatchResult`` whose slabs are sized with
    ``compress_bound(len + 271, ...)``; streams that took no part have ``out_len == 0`` and ``status == 0``.  With ``literal``
    below 8 a stream can fail with ``TAMP_EXCESS_BITS``: its object and bookkeeping stay as the failed piece found them, and
    whatever else the call held for that stream (the rest of a ``write`` above ``PIECE_MAX``) is not sent; the statuses are then
    read back after every library call, one sync each.
    """

    def __init__(self, n: int, *, window: int = 10, literal: int = 8, extended: bool = True, dictionary=None,
                 lazy_matching: bool = False, dictionary_reset: bool = False, append: bool = False, device: int = 0, stream=None):
        if dictionary is not None and len(dictionary) != (1 << window):
            raise ValueError("Dictionary-window size mismatch.")
        if not (8 <= window <= 15 and 5 <= literal <= 8):
            raise ValueError("window must be in 8..15 and literal in 5..8")
        if append and (not dictionary_reset or dictionary is not None):
            raise ValueError("append needs dictionary_reset=True and no dictionary")  # compressor.c:209
        if isinstance(n, bool) or not _is_int(n) or n < 0:
            raise ValueError("n must be a non-negative integer")
        from .codec import Compressor

        self.n, self.window_bits, self.literal = int(n), window, literal
        self._lit_seed = literal if extended else 8  # compressor.c:224-225
        self._conf = _conf(window, literal, extended, dictionary, dictionary_reset, lazy_matching)
        self._dictionary = None if dictionary is None else _np_u8(dictionary).copy()
        self._dictionary_reset, self._append = bool(dictionary_reset), bool(append)
        self._piece_max = Compressor.PIECE_MAX
        self._stream, self._device = stream, device
        self.stride = 48 + (1 << window)
        self._objects = self._nothing_t = self._dev_t = None  # (made by the first call: constructing needs neither library nor device)
        self._seed_t = None
        self._opened = np.zeros(self.n, dtype=bool)           # header / append marker already sent
        self._resume = np.zeros(self.n, dtype=bool)           # the object holds a carried window (else: fresh stream)
        self._dirty = np.zeros(self.n, dtype=bool)            # data was handed over since the last flush point (compressor.c:548)
        self._last_was_flush = np.full(self.n, self._append)  # compressor.c:234

    @property
    def _dev(self):
        if self._dev_t is None:
            import torch

            self._dev_t = torch.device("cuda", self._device)
        return self._dev_t

    @property
    def objects(self):
        """The objects: a CUDA uint8 tensor of shape ``(n, stride)``, each row 48 bytes of ``TampAmdPieceObject`` and the window."""
        if self._objects is None:
            import torch

            _lib.load()  # fail loudly if the native library is missing
            with self._on_stream():
                self._objects = torch.zeros((self.n, self.stride), dtype=torch.uint8, device=self._dev)
                if self._dictionary is not None:
                    self._objects[:, 48:] = torch.from_numpy(self._dictionary).to(self._dev)
        return self._objects

    @property
    def _nothing(self):
        if self._nothing_t is None:
            import torch

            with self._on_stream():
                self._nothing_t = torch.zeros(16, dtype=torch.uint8, device=self._dev)
        return self._nothing_t

    def _on_stream(self):
        import contextlib

        import torch

        if self._stream is None:
            return contextlib.nullcontext()
        return torch.cuda.stream(torch.cuda.ExternalStream(int(self._stream), device=self._dev))

    def _which(self, which) -> np.ndarray:
        mask = np.zeros(self.n, dtype=bool)
        if which is None:
            mask[:] = True
            return mask
        idx = [int(i) for i in which]
        if any(i < 0 or i >= self.n for i in idx):
            raise ValueError(f"which: stream indices must be in 0..{self.n - 1}")
        mask[idx] = True
        return mask

    def _leads(self, live: np.ndarray) -> np.ndarray:
        """The op bits that say how the piece opens, for the streams of ``live``; the others get SKIP."""
        lead = np.where(self._opened, 0, _lib.PIECE_APPEND_MARKER if self._append else _lib.PIECE_HEADER)
        ops = lead | np.where(self._resume, _lib.PIECE_RESUME, 0)
        return np.where(live, ops, _lib.PIECE_SKIP).astype(np.uint8)

    def _run(self, rounds, data, in_off):
        """``rounds``: a list of (ops uint8[n], in_len uint32[n], input shift) on the host.  One library call per round, every
        round's bytes behind the previous round's in the stream's slab.  A stream whose piece fails (``TAMP_EXCESS_BITS``, which
        needs ``literal`` below 8: only then are the statuses read back, one sync per round) takes no part in the later rounds:
        its object stays where the failed piece found it, and its status is that failure.
        -> (BatchResult, streams that completed a piece, streams that failed one)"""
        import torch

        lib = _lib.load()
        n, dev = self.n, self._dev
        caps = [np.where(ops & _lib.PIECE_SKIP, 0, compress_bound(ln.astype(np.int64) + 271, self.literal, self._dictionary_reset))
                for ops, ln, _ in rounds]
        advanced, failed = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        cap = np.sum(caps, axis=0, dtype=np.int64) if rounds else np.zeros(n, dtype=np.int64)
        off = np.cumsum(cap) - cap
        with self._on_stream():
            st = self._stream if self._stream is not None else torch.cuda.current_stream(dev).cuda_stream
            out = torch.empty(max(int(cap.sum()), 1), dtype=torch.uint8, device=dev)
            out_off = torch.from_numpy(off).to(dev)
            out_len = torch.zeros(n, dtype=torch.int32, device=dev)
            status = torch.zeros(n, dtype=torch.int8, device=dev)
            keep = [data, in_off]
            for k, (ops, ln, shift) in enumerate(rounds):
                ops = np.where(failed, _lib.PIECE_SKIP, ops).astype(np.uint8)
                live = (ops & _lib.PIECE_SKIP) == 0
                ops_t = torch.from_numpy(ops).to(dev)
                len_t = torch.from_numpy(ln.astype(np.int32)).to(dev)
                cap_t = torch.from_numpy(caps[k].astype(np.int32)).to(dev)
                off_t = in_off + shift if shift else in_off
                first = k == 0
                o_off = out_off if first else out_off + out_len.to(torch.int64)
                o_len = out_len if first else torch.zeros(n, dtype=torch.int32, device=dev)
                o_status = status if first else torch.zeros(n, dtype=torch.int8, device=dev)
                rc = lib.tamp_batch_compress_pieces(C.byref(self._conf), _ptr(self.objects), self.stride, _ptr(ops_t), _ptr(data),
                                                    _ptr(off_t), _ptr(len_t), _ptr(out), _ptr(o_off), _ptr(cap_t), _ptr(o_len),
                                                    _ptr(o_status), n, int(ln.max()) if n else 0, _lib.MEM_DEVICE, dev.index or 0,
                                                    C.c_void_p(st))
                _lib.check_launch(rc)
                if not first:
                    out_len += o_len
                    status = torch.where(status == 0, o_status, status)
                keep += [ops_t, len_t, cap_t, off_t, o_off, o_len, o_status]
                # (at literal 8 a piece with room for its worst case cannot fail: no read-back)
                bad = live & (o_status.cpu().numpy() != _lib.OK) if self.literal < 8 and n else np.zeros(n, dtype=bool)
                advanced |= live & ~bad
                failed |= bad
        return BatchResult(out, out_off, out_len, status, None, -1.0, tuple(keep)), advanced, failed

    def write(self, chunks, in_off=None, in_len=None):
        """One bytes-like or ``None`` per stream, or a flat CUDA uint8 tensor with CUDA ``in_off`` / ``in_len`` tables (the
        lengths are read back: the bookkeeping is the host's).  Every non-empty chunk goes to its stream as an unfinished
        piece, cut at ``Compressor.PIECE_MAX``."""
        import torch

        if _is_torch(chunks):
            if in_off is None or in_len is None or int(in_len.numel()) != self.n or int(in_off.numel()) != self.n:
                raise ValueError(f"write: in_off and in_len need {self.n} entries")
            lens = in_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            with self._on_stream():
                data, off_t = chunks, in_off.to(torch.int64)
        else:
            chunks = list(chunks)
            if len(chunks) != self.n:
                raise ValueError(f"write: {len(chunks)} chunks for {self.n} streams")
            flat, offs, lens32 = pack_streams([b"" if c is None else c for c in chunks])
            lens = lens32.astype(np.int64)
            with self._on_stream():
                data = torch.from_numpy(flat.copy()).to(self._dev) if flat.size else self._nothing
                off_t = torch.from_numpy(offs.astype(np.int64)).to(self._dev)
        rounds = []
        shift = 0
        while True:
            ln = np.clip(lens - shift, 0, self._piece_max)
            live = ln > 0
            if not live.any():
                break
            # (a stream's second piece of one write: its first has opened it)
            ops = self._leads(live) if not shift else np.where(live, _lib.PIECE_RESUME, _lib.PIECE_SKIP).astype(np.uint8)
            rounds.append((ops, ln.astype(np.uint32), shift))
            shift += self._piece_max
        res, done, _ = self._run(rounds, data, off_t)
        self._opened |= done
        self._resume |= done
        self._dirty |= done
        return res

    def flush(self, write_token: bool = True, which=None):
        """``Compressor.flush`` on the streams of ``which`` (all of them by default)."""
        return self._flush(self._which(which), bool(write_token))

    def _flush(self, sel: np.ndarray, write_token: bool):
        self._last_was_flush &= ~(sel & self._dirty)  # compressor.c:548
        want = sel & write_token & ~self._last_was_flush  # compressor.c:784
        # byte aligned, nothing handed over: the reference's flush writes nothing either
        live = sel & (self._dirty | ~self._opened | (want & self._dictionary_reset))
        ops = self._leads(live) | np.where(live, _lib.PIECE_FINISH, 0).astype(np.uint8) \
            | np.where(live & want, _lib.PIECE_FLUSH_TOKEN, 0).astype(np.uint8)
        with self._on_stream():
            import torch

            zeros = torch.zeros(self.n, dtype=torch.int64, device=self._dev)
        res, done, _ = self._run([(ops, np.zeros(self.n, dtype=np.uint32), 0)] if live.any() else [], self._nothing, zeros)
        self._opened |= done
        self._resume |= done
        self._dirty &= ~done
        asked = done & want
        if asked.any():
            # compressor.c:784-794: the token is written when bits are pending or the stream allows dictionary resets
            token = asked if self._dictionary_reset else asked & (self.objects[:, 34].cpu().numpy() != 0)
            self._last_was_flush |= token
        return res

    def reset_dictionary(self, which=None):
        """``tamp_compressor_reset_dictionary`` (compressor.c:845-881) on the streams of ``which``: the double FLUSH, then a fresh
        seeded window."""
        if not self._dictionary_reset:
            raise ValueError("reset_dictionary needs dictionary_reset=True")  # TAMP_INVALID_CONF
        import torch

        sel = self._which(which)
        # both flushes write their token (the stream allows resets), so both rounds are known now
        first = self._leads(sel) | np.where(sel, _lib.PIECE_FINISH | _lib.PIECE_FLUSH_TOKEN, 0).astype(np.uint8)
        second = np.where(sel, _lib.PIECE_RESUME | _lib.PIECE_FINISH | _lib.PIECE_FLUSH_TOKEN, _lib.PIECE_SKIP).astype(np.uint8)
        none = np.zeros(self.n, dtype=np.uint32)
        with self._on_stream():
            zeros = torch.zeros(self.n, dtype=torch.int64, device=self._dev)
        res, advanced, failed = self._run([(first, none, 0), (second, none, 0)] if sel.any() else [], self._nothing, zeros)
        done = advanced & ~failed
        self._resume |= advanced & failed  # (the first flush went through, the second did not: opened, and no reset)
        self._opened |= advanced
        if done.any():
            with self._on_stream():
                idx = torch.from_numpy(np.flatnonzero(done)).to(self._dev)
                self.objects[idx, :48] = 0  # a fresh object; the next segment starts from the seeded window, never the custom one
                if self._conf.use_custom_dictionary:
                    if self._seed_t is None:
                        seed = np.zeros(1 << self.window_bits, dtype=np.uint8)
                        _lib.load().tamp_initialize_dictionary(_ptr(seed), seed.size, self._lit_seed)
                        self._seed_t = torch.from_numpy(seed).to(self._dev)
                    self.objects[idx, 48:] = self._seed_t
        self._opened |= done
        self._resume &= ~done
        self._dirty &= ~done
        self._last_was_flush = np.where(done, self._append, self._last_was_flush)
        return res

    def close(self):
        """``Compressor.close``: the final flush of every stream (with a FLUSH token where the stream allows resets)."""
        return self._flush(np.ones(self.n, dtype=bool), self._dictionary_reset)


def _read_participants(chunks, which_mask: np.ndarray) -> np.ndarray:
    """Which streams take part in a ``DecompressorBatch.read`` of host chunks: every chunk that is not ``None`` -- ``b""`` takes part
    with no input, which drains a token an earlier ``TAMP_OUTPUT_FULL`` cut short -- and every stream ``which`` names."""
    return np.fromiter((c is not None for c in chunks), dtype=bool, count=len(chunks)) | which_mask


def _read_which(which, n: int) -> np.ndarray:
    """``which`` of ``DecompressorBatch.read`` as a mask; an index out of range or named twice is refused (two rows advancing one
    object in the same launch would leave it undefined)."""
    mask = np.zeros(n, dtype=bool)
    if which is None:
        return mask
    idx = [int(i) for i in which]
    if any(i < 0 or i >= n for i in idx):
        raise ValueError(f"which: stream indices must be in 0..{n - 1}")
    if len(set(idx)) != len(idx):
        raise ValueError("which: a stream is named twice")
    mask[idx] = True
    return mask


def _read_slabs(size, max_out: int):
    """The slabs of a ``read`` whose sizes the query found: stream ``i`` gets ``min(size[i] + 1, max_out)`` bytes of room at the running
    sum of the rooms in front of it (``decompress_batch`` sizes its slabs the same way; the spare byte lets a piece that ends in
    bits too short for a token report ``TAMP_INPUT_EXHAUSTED``, not ``TAMP_OUTPUT_FULL``).  ``size``: uint32 values as a numpy array or
    a torch tensor (int32 storage included) -> (cap, off) in 64 bits, the same kind."""
    if _is_torch(size):
        import torch

        cap = torch.clamp((size.to(torch.int64) & 0xFFFFFFFF) + 1, max=int(max_out))
        return cap, torch.cumsum(cap, 0) - cap
    cap = np.minimum((np.asarray(size).astype(np.int64) & 0xFFFFFFFF) + 1, int(max_out))
    return cap, np.cumsum(cap) - cap


class DecompressorBatch:
    """``n`` streaming decoders on the device, advanced together: the receiving side of ``CompressorBatch``.

    Stream ``i`` is one reference ``TampDecompressor`` (tamp/_c_src/tamp/decompressor.h:13-57), as with ``DecoderBatch`` and with
    the same arguments -- ``conf=None`` reads each stream's header, a ``dictionary`` sits in every object's window -- but the
    objects (16 bytes of state + the window each) live in one CUDA uint8 tensor ``objects`` of shape ``(n, stride)`` and never
    leave the device, input and output are CUDA tensors, and a round touches only the objects of the streams that take part.

    ``read(chunks)`` offers stream ``i`` the bytes ``chunks[i]`` and returns a ``BatchResult`` of ``n`` rows: the decoded bytes, the
    reference's status (2 input exhausted, 1 output full, negative = error) and ``in_consumed`` per stream.  What was not consumed
    must be offered again.
    """

    def __init__(self, n: int, *, window_bits: int = 15, conf: Optional[TampAmdConf] = None, dictionary=None, device: int = 0,
                 stream=None):
        if isinstance(n, bool) or not _is_int(n) or n < 0:
            raise ValueError("n must be a non-negative integer")
        if not 8 <= window_bits <= 15:
            raise ValueError("window_bits must be in 8..15")
        if conf is not None and conf.use_custom_dictionary and dictionary is None:
            raise ValueError("custom dictionary expected")
        if conf is not None and dictionary is not None and not conf.use_custom_dictionary:
            raise ValueError("a dictionary needs conf.use_custom_dictionary")
        self.n, self.window_bits = int(n), window_bits
        self.stride = (16 + (1 << window_bits) + 15) & ~15  # tamp_amd_decoder_state_size, in whole 16 bytes
        self._conf = conf
        self._dictionary = None if dictionary is None else _np_u8(dictionary)[: 1 << window_bits].copy()
        self._stream, self._device = stream, device
        self._objects = self._dev_t = None  # (made by the first call: constructing needs neither library nor device)

    _dev = CompressorBatch._dev
    _on_stream = CompressorBatch._on_stream

    @property
    def objects(self):
        """The objects: a CUDA uint8 tensor of shape ``(n, stride)``, each row a ``TampAmdDecoderState`` and the window."""
        if self._objects is None:
            import torch

            lib = _lib.load()
            one = np.zeros(self.stride, dtype=np.uint8)
            if self._dictionary is not None:  # the window buffer holds the dictionary, as with the reference's object
                one[16 : 16 + len(self._dictionary)] = self._dictionary
            res = lib.tamp_amd_decoder_state_init(_ptr(one), C.byref(self._conf) if self._conf is not None else None, self.window_bits)
            if res != _lib.OK:
                raise ValueError(f"tamp_amd_decoder_state_init -> {res}")
            with self._on_stream():
                self._objects = torch.from_numpy(one).to(self._dev).unsqueeze(0).repeat(self.n, 1)
        return self._objects

    def read(self, chunks, in_off=None, in_len=None, *, out_cap=None, max_out=None, which=None) -> BatchResult:
        """One bytes-like or ``None`` per stream, or a flat CUDA uint8 tensor with CUDA ``in_off`` / ``in_len`` tables -- ``out``,
        ``out_off``, ``out_len`` of a ``CompressorBatch`` result go in as they are.

        A ``None`` chunk (tensors: ``in_len == 0``) means the stream takes no part: its object is untouched and its rows of the result
        are 0.  ``b""`` (tensors: a stream named in ``which``) takes part with no input, which drains a token an earlier
        ``TAMP_OUTPUT_FULL`` cut short.

        ``out_cap=None``: ``tamp_batch_decoded_size_pieces`` finds what each piece decodes to from where its object stands, and stream
        ``i`` is decoded into ``min(size + 1, max_out)`` bytes at the running sum (one device-to-host sync for the total).  A stream
        above ``max_out`` comes back with ``TAMP_OUTPUT_FULL``, ``max_out`` bytes and its ``in_consumed``, and a later ``read``
        continues it; a stream whose piece is in error is decoded all the same and reports that error.
        ``out_cap`` = an int or one value per stream: one decode launch into that much room, no query."""
        import torch

        n = self.n
        max_out = 0xFFFFFFFF if max_out is None else int(max_out)
        if not 0 <= max_out <= 0xFFFFFFFF:
            raise ValueError("max_out must fit 32 bits")
        which_mask = _read_which(which, n)
        on_device = _is_torch(chunks)
        if on_device:
            if in_off is None or in_len is None or int(in_len.numel()) != n or int(in_off.numel()) != n:
                raise ValueError(f"read: in_off and in_len need {n} entries")
        else:
            chunks = list(chunks)
            if len(chunks) != n:
                raise ValueError(f"read: {len(chunks)} chunks for {n} streams")
        cap_all = None
        if out_cap is not None:
            if _is_int(out_cap):
                cap_all = np.full(n, int(out_cap), dtype=np.int64)
            else:
                cap_all = np.asarray(out_cap.cpu() if _is_torch(out_cap) else out_cap).astype(np.int64).reshape(-1)
                if cap_all.size != n:
                    raise ValueError(f"read: out_cap needs {n} entries")
            if n and (cap_all.min() < 0 or cap_all.max() > 0xFFFFFFFF):
                raise ValueError("out_cap must fit 32 bits")

        lib = _lib.load()
        dev = self._dev
        with self._on_stream():
            st = self._stream if self._stream is not None else torch.cuda.current_stream(dev).cuda_stream
            # ---- the rows: one per stream that takes part, in stream order ----
            if on_device:
                data = chunks
                part = (in_len != 0) | torch.from_numpy(which_mask).to(dev) if which_mask.any() else in_len != 0
                idx = torch.nonzero(part).flatten()  # (reads the count back: the rows are sized on the host)
                m = int(idx.numel())
                off_t, len_t = in_off.to(torch.int64), in_len.to(torch.int32)
                if m != n:
                    off_t, len_t = off_t[idx], len_t[idx]
            else:
                idx_np = np.flatnonzero(_read_participants(chunks, which_mask))
                m = int(idx_np.size)
                flat, offs, lens = pack_streams([chunks[i] if chunks[i] is not None else b"" for i in idx_np])
                data = torch.from_numpy(flat.copy()).to(dev) if flat.size else torch.zeros(16, dtype=torch.uint8, device=dev)
                off_t = torch.from_numpy(offs.astype(np.int64)).to(dev)
                len_t = torch.from_numpy(lens.astype(np.int32)).to(dev)
                idx = torch.from_numpy(idx_np).to(dev)
            if m == 0:
                zeros = torch.zeros(n, dtype=torch.int32, device=dev)
                return BatchResult(torch.zeros(1, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int64, device=dev), zeros,
                                   torch.zeros(n, dtype=torch.int8, device=dev), zeros.clone())
            obj_t = idx.to(torch.int32) if m != n else None  # (every stream, in order: the identity needs no table)
            objects = self.objects
            out_len = torch.empty(m, dtype=torch.int32, device=dev)
            status = torch.empty(m, dtype=torch.int8, device=dev)
            consumed = torch.empty(m, dtype=torch.int32, device=dev)
            keep = [data, off_t, len_t, obj_t]
            # ---- room ----
            if cap_all is None:
                limit_t = None  # (no limit below 2^32 - 1: no table)
                if max_out != 0xFFFFFFFF:
                    limit_t = torch.full((m,), max_out - (1 << 32) if max_out >= 1 << 31 else max_out, dtype=torch.int32, device=dev)
                rc = lib.tamp_batch_decoded_size_pieces(_ptr(objects), self.stride, self.window_bits, _ptr(obj_t), _ptr(data), _ptr(off_t),
                                                        _ptr(len_t), _ptr(limit_t), _ptr(out_len), _ptr(status), _ptr(consumed), m,
                                                        dev.index or 0, C.c_void_p(st))
                _lib.check_launch(rc)
                cap64, o_off = _read_slabs(out_len, max_out)
                total = int(cap64.sum().item())  # (the one value read back: it sizes the output tensor)
                keep.append(limit_t)
            else:
                sel = cap_all if m == n else cap_all[idx.cpu().numpy()]
                total = int(sel.sum())
                cap64 = torch.from_numpy(sel).to(dev)
                o_off = torch.cumsum(cap64, 0) - cap64
            cap_t = cap64.to(torch.int32)  # (the low 32 bits: what the library reads as uint32)
            out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
            rc = lib.tamp_batch_decompress_pieces(_ptr(objects), self.stride, self.window_bits, _ptr(obj_t), _ptr(data), _ptr(off_t),
                                                  _ptr(len_t), _ptr(out), _ptr(o_off), _ptr(cap_t), _ptr(out_len), _ptr(status),
                                                  _ptr(consumed), m, dev.index or 0, C.c_void_p(st))
            _lib.check_launch(rc)
            keep += [cap_t, o_off, out_len, status, consumed]
            if m != n:  # the rows back to their streams; the others are 0
                def spread(rows, dtype):
                    full = torch.zeros(n, dtype=dtype, device=dev)
                    full[idx] = rows
                    return full
                o_off, out_len = spread(o_off, torch.int64), spread(out_len, torch.int32)
                status, consumed = spread(status, torch.int8), spread(consumed, torch.int32)
        return BatchResult(out, o_off, out_len, status, consumed, -1.0, tuple(keep))
