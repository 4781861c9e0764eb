"""Host-side mirror of the reference's block interface for the RX hot path, over the C-ABI.

Same block names, setting names, defaults and error behaviour as the reference's
gr::Block<T> classes (cited per class; paths relative to
/root/reference/blocks/include/gnuradio-4.0/packet-modem/).  `start()` mirrors
gr::Block::start(), `process_bulk()` mirrors processBulk(); samples are torch tensors
resident in HBM (torch is only plumbing: device memory + the current HIP stream), tags are
numpy records (TAG_DTYPE) with explicit indices instead of the runtime's chunk-head tags.
The C++ gr::Block wrappers in host/ are the drop-in for the reference's flowgraphs; this
module is what the parity tests and bench.py drive."""
import ctypes as C
import fractions
import math
import os

import numpy as np

from . import _abi
from ._abi import PACKET_TAG_DTYPE, TAG_DTYPE, TAG_OTHER, TAG_SYNCWORD, Gr4pmError, check, lib

CONSTELLATIONS = {"PILOT": 0, "BPSK": 1, "QPSK": 2}  # constellation.hpp:6


def _torch():
    import torch
    return torch


def _stream_handle():
    torch = _torch()
    if not torch.cuda.is_available():
        raise Gr4pmError("no HIP device: the gr4pm blocks have no CPU fallback")
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _release(name, h):
    """destroy a C handle; silent when the interpreter is already tearing the module down"""
    try:
        getattr(lib(), name)(h)
    except Exception:
        pass


def _dev_c64(x, what="in"):
    torch = _torch()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.complex64 and x.is_contiguous()):
        raise TypeError(f"{what} must be a contiguous complex64 CUDA tensor")
    return x


def _inputs_ready(x):
    """The receivers inside the library run on streams of their own (non-blocking: they do not order themselves against
    torch's streams).  An input that a torch kernel is still writing on the caller's current stream would be read too
    early: wait for that stream (a few microseconds when it is idle)."""
    _torch().cuda.current_stream(x.device).synchronize()


def _dev_c64_rows(x, what="in"):
    """[channels, n] with contiguous rows; the row stride is free (a window of a wider ring)"""
    torch = _torch()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.complex64 and x.dim() == 2 and
            (x.shape[1] <= 1 or x.stride(1) == 1) and x.stride(0) >= x.shape[1]):
        raise TypeError(f"{what} must be a [channels, n] complex64 CUDA tensor with contiguous rows")
    return x


def _tags_array(tags):
    if tags is None:
        return np.zeros(0, dtype=TAG_DTYPE)
    return np.ascontiguousarray(tags, dtype=TAG_DTYPE)


def _ptags_array(tags):
    if tags is None:
        return np.zeros(0, dtype=PACKET_TAG_DTYPE)
    return np.ascontiguousarray(tags, dtype=PACKET_TAG_DTYPE)


def _header_msgs(headers):
    """parsed_header messages: packet_length, or None for an "invalid_header" message; returns
    (HEADER_MSG_DTYPE array with at least one slot, number of messages)"""
    if isinstance(headers, np.ndarray) and headers.dtype == _abi.HEADER_MSG_DTYPE:
        return (headers if headers.size else np.zeros(1, dtype=_abi.HEADER_MSG_DTYPE)), headers.size
    n = len(headers)
    msgs = np.zeros(max(n, 1), dtype=_abi.HEADER_MSG_DTYPE)
    if isinstance(headers, np.ndarray):  # all valid
        msgs["packet_length"][:n] = headers
        return msgs, n
    for i, h in enumerate(headers):
        if h is None:
            msgs[i]["invalid_header"] = 1
        else:
            msgs[i]["packet_length"] = int(h)
    return msgs, n


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def sincosf(x):
    """sinf / cosf as the CostasLoop kernels evaluate them (glibc's algorithm on the device), for the parity suite"""
    torch = _torch()
    xd = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    s, c = torch.empty_like(xd), torch.empty_like(xd)
    check(lib().gr4pm_sincosf(xd.data_ptr(), xd.numel(), s.data_ptr(), c.data_ptr()), "sincosf")
    return s.cpu().numpy(), c.cpu().numpy()


def logf(x):
    """glibc's logf as the NoiseSource kernels evaluate it (csrc/noise_source.hip), for the parity suite.  x: a CUDA
    float32 tensor (returns one) or anything numpy takes (returns a numpy array)"""
    torch = _torch()
    on_dev = isinstance(x, torch.Tensor) and x.is_cuda
    xd = x.contiguous() if on_dev else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    if xd.dtype != torch.float32:
        raise TypeError("logf: float32 input")
    out = torch.empty_like(xd)
    check(lib().gr4pm_logf(xd.data_ptr(), xd.numel(), out.data_ptr()), "logf")
    return out if on_dev else out.cpu().numpy()


def costas_phase_wrap(x):
    """the phase wrap of a CostasLoop iteration (costas_loop.hpp:141-145) as the kernels evaluate it, for the parity suite"""
    torch = _torch()
    xd = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    out = torch.empty_like(xd)
    check(lib().gr4pm_costas_phase_wrap(xd.data_ptr(), xd.numel(), out.data_ptr()), "costas_phase_wrap")
    return out.cpu().numpy()


def packet_transmitter_rrc_taps(samples_per_symbol):
    """packet_transmitter_rrc_taps.hpp:8-28: the transmitter's RRC (root_raised_cosine(1, sps, 1, 0.35, 11 sps))
    scaled so that the largest polyphase |tap| sum is 0.9 (DAC head-room), in the reference's float32 arithmetic
    and summation order"""
    sps = int(samples_per_symbol)
    taps = root_raised_cosine(1.0, float(sps), 1.0, 0.35, sps * 11)
    worst = np.float32(0.0)
    for j in range(sps):
        acc = np.float32(0.0)
        for k in range(j, taps.size, sps):
            acc = np.float32(acc + np.abs(taps[k]))
        worst = max(worst, acc)
    return (taps * np.float32(np.float32(0.9) / worst)).astype(np.float32)


def root_raised_cosine(gain, sampling_freq, symbol_rate, alpha, ntaps):
    """firdes::root_raised_cosine<float>, firdes.hpp:29-76"""
    out = np.zeros(ntaps | 1, dtype=np.float32)
    n = lib().gr4pm_firdes_root_raised_cosine(gain, sampling_freq, symbol_rate, alpha, ntaps, _np_ptr(out))
    return out[:n]


class SyncwordDetection:
    """syncword_detection.hpp:32-357.  Settings :133-141 keep their names and defaults."""

    def __init__(self, rrc_taps, syncword, constellation, min_freq_bin=0, max_freq_bin=0, fft_size=2048,
                 samples_per_symbol=4, time_threshold=768, power_threshold=9.5, n_channels=1,
                 max_items=1 << 22):
        self.fft_size = fft_size
        self.samples_per_symbol = samples_per_symbol
        self.rrc_taps = np.ascontiguousarray(rrc_taps, dtype=np.float32)
        self.syncword = np.ascontiguousarray(syncword, dtype=np.uint8)
        self.constellation = np.ascontiguousarray(constellation, dtype=np.complex64)
        self.min_freq_bin = min_freq_bin
        self.max_freq_bin = max_freq_bin
        self.time_threshold = time_threshold
        self.power_threshold = power_threshold
        self.n_channels = n_channels
        self.max_items = max_items
        self._h = None
        self.start()

    def start(self):
        """start(), :143-202; raises Gr4pmError where the reference throws gr::exception"""
        self._destroy()
        p = _abi.SyncwordDetectionParams(
            self.fft_size, self.samples_per_symbol, _np_ptr(self.rrc_taps), self.rrc_taps.size,
            _np_ptr(self.syncword), self.syncword.size, _np_ptr(self.constellation), self.constellation.size,
            self.min_freq_bin, self.max_freq_bin, self.time_threshold, self.power_threshold, self.n_channels,
            self.max_items, _stream_handle())
        h = C.c_void_p()
        check(lib().gr4pm_syncword_detection_create(C.byref(p), C.byref(h)), "SyncwordDetection.start")
        self._h = h
        self._syncword_samples_size = lib().gr4pm_syncword_detection_syncword_samples_size(h)
        self._syncword_self_corr = lib().gr4pm_syncword_detection_self_corr(h)

    @property
    def _items_consumed(self):
        return lib().gr4pm_syncword_detection_items_consumed(self._h)

    def scan_counts(self, channel=0):
        """(candidates the scan visited, of which tested by the separate pass over the powers) in the last call"""
        v, m = C.c_uint64(0), C.c_uint64(0)
        lib().gr4pm_syncword_detection_scan_counts(self._h, channel, C.byref(v), C.byref(m))
        return v.value, m.value

    def reset(self):
        """back to the state right after start() without rebuilding the templates"""
        check(lib().gr4pm_syncword_detection_reset(self._h), "SyncwordDetection.reset")

    def announce(self, x):
        """look-ahead: names the input of a later call (after the ones already announced, at most
        two calls ahead); everything of that call that does not depend on the scan state runs on
        other streams behind the calls before it.  The caller keeps x alive and unchanged."""
        x = _dev_c64(x)
        x2 = x.reshape(1, -1) if x.dim() == 1 else x
        assert x2.shape[0] == self.n_channels
        check(lib().gr4pm_syncword_detection_announce(self._h, x2.data_ptr(), x2.stride(0), x2.shape[1]),
              "SyncwordDetection.announce")

    def process_bulk(self, x, want_output=True, tags_cap=1024, next_x=None):
        """processBulk(), :204-356.  x: [n] or [n_channels, n] complex64 on the GPU.
        Returns (status, out, tags): out holds the n_done published items (delayed input),
        tags a list (one per channel) of TAG_DTYPE records, index relative to out[0].
        next_x (optional look-ahead): the tensor the NEXT call will be given; its correlator
        then runs on a second stream behind this call's.  The caller keeps next_x alive and
        unchanged until that call (a device ring does)."""
        torch = _torch()
        x = _dev_c64(x)
        x2 = x.reshape(1, -1) if x.dim() == 1 else x
        assert x2.shape[0] == self.n_channels
        n_in = x2.shape[1]
        if next_x is not None:
            nx = _dev_c64(next_x)
            nx2 = nx.reshape(1, -1) if nx.dim() == 1 else nx
            assert nx2.shape[0] == self.n_channels
            check(lib().gr4pm_syncword_detection_hint_next(self._h, nx2.data_ptr(), nx2.stride(0), nx2.shape[1]),
                  "SyncwordDetection.hint_next")
        out = torch.empty_like(x2) if want_output else None
        n_done = C.c_size_t(0)
        tags = np.zeros((self.n_channels, tags_cap), dtype=TAG_DTYPE)
        n_tags = (C.c_size_t * self.n_channels)()
        st = lib().gr4pm_syncword_detection_process(
            self._h, x2.data_ptr(), x2.stride(0), n_in, out.data_ptr() if want_output else None,
            out.stride(0) if want_output else 0, C.byref(n_done), _np_ptr(tags), tags_cap, n_tags)
        check(st, "SyncwordDetection.processBulk")
        n = n_done.value
        tag_list = [tags[c, : n_tags[c]].copy() for c in range(self.n_channels)]
        if want_output:
            out = out[:, :n]
            if x.dim() == 1:
                out = out[0]
        if x.dim() == 1:
            tag_list = tag_list[0]
        return st, out, tag_list, n

    def correlate_only(self, x):
        """measurement hook: only the overlap-save correlator kernel (bench.py roofline leg)"""
        x2 = x.reshape(1, -1) if x.dim() == 1 else x
        check(lib().gr4pm_syncword_detection_correlate_only(self._h, x2.data_ptr(), x2.stride(0), x2.shape[1]),
              "correlate_only")

    def last_zpow(self, n_done):
        torch = _torch()
        z = torch.empty((self.n_channels, n_done), dtype=torch.float32, device="cuda")
        check(lib().gr4pm_syncword_detection_last_zpow(self._h, z.data_ptr(), z.stride(0)), "last_zpow")
        return z

    def _destroy(self):
        if getattr(self, "_h", None):
            _release("gr4pm_syncword_detection_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass


class SyncwordDetectionFilter:
    """syncword_detection_filter.hpp:10-211"""

    def __init__(self, samples_per_symbol=4, syncword_size=64, header_size=128):
        self.samples_per_symbol, self.syncword_size, self.header_size = samples_per_symbol, syncword_size, header_size
        p = _abi.SdfParams(samples_per_symbol, syncword_size, header_size, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_syncword_detection_filter_create(C.byref(p), C.byref(self._h)), "SyncwordDetectionFilter")

    def start(self):
        check(lib().gr4pm_syncword_detection_filter_reset(self._h), "start")

    def process_bulk(self, x, out, head_tag_flags=0, headers=(), n_ignored=0):
        """one processBulk (:54-210). headers: sequence of packet_length or None (invalid_header).
        Returns (consumed, headers_consumed, ignored_consumed, tag_out_flags)."""
        x = _dev_c64(x)
        msgs = (_abi.HeaderMsg * max(len(headers), 1))()
        for i, hm in enumerate(headers):
            msgs[i].packet_length = 0 if hm is None else hm
            msgs[i].invalid_header = 1 if hm is None else 0
        c, hc, ic, tf = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        check(lib().gr4pm_syncword_detection_filter_process(
            self._h, x.data_ptr(), x.numel(), out.data_ptr(), out.numel(), head_tag_flags, msgs, len(headers),
            n_ignored, C.byref(c), C.byref(hc), C.byref(ic), C.byref(tf)), "SyncwordDetectionFilter.processBulk")
        return c.value, hc.value, ic.value, tf.value

    def gate(self, tag_index, headers=(), per_tag=False):
        """tag gate without the copy (device-resident chains): which syncword tags pass.
        headers[k] answers the k-th accepted tag (per_tag: tag k if accepted): packet_length, or
        None for invalid_header."""
        idx = np.ascontiguousarray(tag_index, dtype=np.uint64)
        msgs = np.zeros(max(len(headers), 1), dtype=_abi.HEADER_MSG_DTYPE)
        if isinstance(headers, np.ndarray) and headers.dtype == _abi.HEADER_MSG_DTYPE:
            msgs = _header_msgs(headers)[0]
        elif len(headers):
            if isinstance(headers, np.ndarray) and headers.dtype.kind in "iu":
                msgs["packet_length"][: len(headers)] = headers
            else:
                inval = np.fromiter((h is None for h in headers), dtype=bool, count=len(headers))
                msgs["invalid_header"][: len(headers)] = inval
                msgs["packet_length"][: len(headers)] = np.fromiter((0 if h is None else h for h in headers),
                                                                    dtype=np.uint64, count=len(headers))
        acc = np.zeros(max(idx.size, 1), dtype=np.uint8)
        used = C.c_size_t(0)
        check(lib().gr4pm_syncword_detection_filter_gate(self._h, _np_ptr(idx), idx.size, _np_ptr(msgs), len(headers),
                                                         1 if per_tag else 0, _np_ptr(acc), C.byref(used)),
              "SyncwordDetectionFilter.gate")
        return acc[: idx.size].astype(bool), used.value

    def gate_resolve(self, msg):
        """deliver the message of the packet the gate left open with a pending header"""
        m = np.ascontiguousarray(msg, dtype=_abi.HEADER_MSG_DTYPE).reshape(1)
        check(lib().gr4pm_syncword_detection_filter_gate_resolve(self._h, _np_ptr(m)), "SyncwordDetectionFilter.gate")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_syncword_detection_filter_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class _RotatorBase:
    def _create(self, mode, phase_incr, delay, n_channels):
        p = _abi.RotatorParams(mode, phase_incr, delay, n_channels, _stream_handle())
        self._h = C.c_void_p()
        self.n_channels = n_channels
        check(lib().gr4pm_rotator_create(C.byref(p), C.byref(self._h)), type(self).__name__)

    def start(self):
        check(lib().gr4pm_rotator_reset(self._h), "start")

    def process_bulk(self, x, tags=None, tag_channel=None):
        torch = _torch()
        x = _dev_c64(x)
        x2 = x.reshape(1, -1) if x.dim() == 1 else x
        out = torch.empty_like(x2)
        t = _tags_array(tags)
        tc = None if tag_channel is None else np.ascontiguousarray(tag_channel, dtype=np.uint32)
        check(lib().gr4pm_rotator_process(self._h, x2.data_ptr(), x2.stride(0), x2.shape[1], out.data_ptr(),
                                          _np_ptr(t), None if tc is None else _np_ptr(tc), t.size),
              type(self).__name__ + ".processBulk")
        return out.reshape(x.shape)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_rotator_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class Rotator(_RotatorBase):
    """rotator.hpp:20-65"""

    def __init__(self, phase_incr=0.0, n_channels=1):
        self.phase_incr = np.float32(phase_incr)
        self._create(0, float(self.phase_incr), 0, n_channels)


class CoarseFrequencyCorrection(_RotatorBase):
    """coarse_frequency_correction.hpp:20-99"""

    def __init__(self, delay=0, n_channels=1):
        self.delay = delay
        self._create(1, 0.0, delay, n_channels)


class CostasLoop:
    """costas_loop.hpp:15-149"""

    def __init__(self, loop_bandwidth=0.01, constellation="BPSK", n_channels=1):
        self.loop_bandwidth = loop_bandwidth
        self.constellation = constellation
        if constellation.upper() not in CONSTELLATIONS:
            raise Gr4pmError(f"unknown constellation {constellation}")  # enum_cast(...).value() throws
        p = _abi.CostasParams(loop_bandwidth, CONSTELLATIONS[constellation.upper()], n_channels, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_costas_loop_create(C.byref(p), C.byref(self._h)), "CostasLoop")

    @property
    def coeffs(self):
        k1, k2 = C.c_float(0), C.c_float(0)
        lib().gr4pm_costas_loop_coeffs(self._h, C.byref(k1), C.byref(k2))
        return k1.value, k2.value

    def settings_changed(self, loop_bandwidth=None, constellation=None):
        """settingsChanged(), :52-88"""
        if loop_bandwidth is not None:
            self.loop_bandwidth = loop_bandwidth
        if constellation is not None:
            self.constellation = constellation
        check(lib().gr4pm_costas_loop_set(self._h, self.loop_bandwidth, CONSTELLATIONS[self.constellation.upper()]),
              "settingsChanged")

    def process_bulk(self, x, tags=None, tag_channel=None):
        torch = _torch()
        x = _dev_c64(x)
        x2 = x.reshape(1, -1) if x.dim() == 1 else x
        out = torch.empty_like(x2)
        t = _tags_array(tags)
        tc = None if tag_channel is None else np.ascontiguousarray(tag_channel, dtype=np.uint32)
        check(lib().gr4pm_costas_loop_process(self._h, x2.data_ptr(), x2.stride(0), x2.shape[1], out.data_ptr(),
                                              _np_ptr(t), None if tc is None else _np_ptr(tc), t.size),
              "CostasLoop.processBulk")
        return out.reshape(x.shape)

    def process_packets(self, x, tags):
        """processBulk() behind PayloadMetadataInsert: tags are PACKET_TAG_DTYPE records whose
        "constellation" / "loop_bandwidth" keys update the settings (:52-88) from the tagged item
        on and whose syncword_phase sets the phase (:101-106)"""
        torch = _torch()
        x = _dev_c64(x)
        out = torch.empty_like(x)
        t = _ptags_array(tags)
        check(lib().gr4pm_costas_loop_process_packets(self._h, x.data_ptr(), x.numel(), out.data_ptr(), _np_ptr(t),
                                                      t.size), "CostasLoop.processBulk")
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_costas_loop_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class SyncwordWipeoff:
    """syncword_wipeoff.hpp:12-91"""

    def __init__(self, syncword):
        self.syncword = np.ascontiguousarray(syncword, dtype=np.float32)
        p = _abi.WipeoffParams(_np_ptr(self.syncword), self.syncword.size, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_syncword_wipeoff_create(C.byref(p), C.byref(self._h)), "SyncwordWipeoff")

    def process_bulk(self, x, tags=None, in_place=False):
        """in_place: the syncword items of x itself are multiplied, nothing is copied (x is returned)"""
        torch = _torch()
        x = _dev_c64(x)
        out = x if in_place else torch.empty_like(x)
        t = _tags_array(tags)
        check(lib().gr4pm_syncword_wipeoff_process(self._h, x.data_ptr(), x.numel(), out.data_ptr(), _np_ptr(t),
                                                   t.size), "SyncwordWipeoff.processBulk")
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_syncword_wipeoff_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class PayloadMetadataInsert:
    """payload_metadata_insert.hpp:12-324"""

    def __init__(self, syncword_size=64, header_size=128, syncword_costas_loop_bandwidth=0.02,
                 header_costas_loop_bandwidth=0.01, payload_costas_loop_bandwidth=0.005):
        self.syncword_size, self.header_size = syncword_size, header_size
        p = _abi.PmiParams(syncword_size, header_size, syncword_costas_loop_bandwidth, header_costas_loop_bandwidth,
                           payload_costas_loop_bandwidth, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_payload_metadata_insert_create(C.byref(p), C.byref(self._h)), "PayloadMetadataInsert")

    def start(self):
        check(lib().gr4pm_payload_metadata_insert_reset(self._h), "PayloadMetadataInsert.start")

    def resolve(self, msg):
        """per_tag mode: the message of the packet that was opened with a pending header"""
        m = np.ascontiguousarray(msg, dtype=_abi.HEADER_MSG_DTYPE).reshape(1)
        check(lib().gr4pm_payload_metadata_insert_resolve(self._h, _np_ptr(m)), "PayloadMetadataInsert.resolve")

    def process_bulk(self, x, tags=None, headers=(), out_cap=None, tags_cap=None, per_tag=False):
        """x: symbols with syncword tags (TAG_DTYPE); headers: the pending parsed_header messages
        (packet_length, None = invalid header), or with per_tag one message per tag.  Returns
        dict(out, tags, consumed, headers_used, ignored): consumed < len(x) where the block waits
        for a header message."""
        torch = _torch()
        x = _dev_c64(x)
        t = _tags_array(tags)
        out_cap = x.numel() if out_cap is None else out_cap
        out = torch.empty(max(out_cap, 1), dtype=x.dtype, device=x.device)
        tags_cap = 3 * t.size + 8 if tags_cap is None else tags_cap
        tout = np.empty(tags_cap, dtype=PACKET_TAG_DTYPE)  # the first n_tags records are written whole
        msgs, n_msgs = _header_msgs(headers)
        v = [C.c_size_t(0) for _ in range(5)]
        check(lib().gr4pm_payload_metadata_insert_process(
            self._h, x.data_ptr(), x.numel(), out.data_ptr(), out_cap, _np_ptr(t), t.size, _np_ptr(msgs),
            n_msgs, 1 if per_tag else 0, _np_ptr(tout), tags_cap, *[C.byref(c) for c in v]),
            "PayloadMetadataInsert.processBulk")
        n_tags, consumed, produced, used, ignored = [c.value for c in v]
        return {"out": out[:produced], "tags": tout[:n_tags], "consumed": consumed, "headers_used": used,
                "ignored": ignored}

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_payload_metadata_insert_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class SyncwordRemove:
    """syncword_remove.hpp:11-112"""

    def __init__(self, syncword_size=64):
        self.syncword_size = syncword_size
        p = _abi.SyncwordRemoveParams(syncword_size, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_syncword_remove_create(C.byref(p), C.byref(self._h)), "SyncwordRemove")

    def process_bulk(self, x, tags=None):
        torch = _torch()
        x = _dev_c64(x)
        t = _ptags_array(tags)
        out = torch.empty(max(x.numel(), 1), dtype=x.dtype, device=x.device)
        tout = np.empty(t.size + 1, dtype=PACKET_TAG_DTYPE)
        nt, produced = C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4pm_syncword_remove_process(self._h, x.data_ptr(), x.numel(), out.data_ptr(), _np_ptr(t),
                                                  t.size, _np_ptr(tout), tout.size, C.byref(nt), C.byref(produced)),
              "SyncwordRemove.processBulk")
        return out[: produced.value], tout[: nt.value]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_syncword_remove_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class ConstellationLLRDecoder:
    """constellation_llr_decoder.hpp:13-142"""

    def __init__(self, noise_sigma=1.0, constellation="BPSK"):
        self.noise_sigma, self.constellation = noise_sigma, constellation
        if constellation.upper() not in CONSTELLATIONS:
            raise Gr4pmError(f"unknown constellation {constellation}")
        p = _abi.LlrParams(noise_sigma, CONSTELLATIONS[constellation.upper()], _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_constellation_llr_decoder_create(C.byref(p), C.byref(self._h)),
              "ConstellationLLRDecoder")  # PILOT: "constellation not supported", :72-74

    def process_bulk(self, x, tags=None):
        """returns (llr float32 tensor, tags re-indexed to LLR positions)"""
        torch = _torch()
        x = _dev_c64(x)
        t = _ptags_array(tags)
        out = torch.empty(max(2 * x.numel(), 1), dtype=torch.float32, device=x.device)
        tout = np.empty(t.size + 1, dtype=PACKET_TAG_DTYPE)
        nt, produced = C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4pm_constellation_llr_decoder_process(
            self._h, x.data_ptr(), x.numel(), out.data_ptr(), out.numel(), _np_ptr(t), t.size, _np_ptr(tout),
            tout.size, C.byref(nt), C.byref(produced)), "ConstellationLLRDecoder.processBulk")
        return out[: produced.value], tout[: nt.value]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_constellation_llr_decoder_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class AdditiveScrambler:
    """additive_scrambler.hpp:24-100 on float32 soft symbols or uint8 hard symbols (by the
    dtype of the first tensor it is given, or `dtype=`)"""

    def __init__(self, mask=0x8A, seed=0x7F, length=7, count=0, dtype="float32"):
        self.mask, self.seed, self.length, self.count = mask, seed, length, count
        kind = {"float32": 1, "uint8": 2}[str(dtype).replace("torch.", "")]
        p = _abi.ScramblerParams(mask, seed, length, count, kind, _stream_handle())
        self._kind = kind
        self._h = C.c_void_p()
        check(lib().gr4pm_additive_scrambler_create(C.byref(p), C.byref(self._h)), "AdditiveScrambler")

    def start(self):
        check(lib().gr4pm_additive_scrambler_reset(self._h), "AdditiveScrambler.start")

    def process_bulk(self, x, reset_index=()):
        """reset_index: items that carry the reset_tag_key (:78-80)"""
        torch = _torch()
        want = torch.float32 if self._kind == 1 else torch.uint8
        if not x.is_cuda or x.dtype != want:
            raise Gr4pmError(f"AdditiveScrambler expects a CUDA {want} tensor")
        x = x.contiguous()
        out = torch.empty_like(x)
        ri = np.ascontiguousarray(reset_index, dtype=np.uint64)
        check(lib().gr4pm_additive_scrambler_process(self._h, x.data_ptr(), x.numel(), out.data_ptr(), _np_ptr(ri),
                                                     ri.size), "AdditiveScrambler.processBulk")
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_additive_scrambler_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class HeaderPayloadSplit:
    """header_payload_split.hpp:9-147 on float32 items (the header loop, packet_receiver.hpp:136-137) or complex64
    items (the symbol tap of zmq_output, :159-162: header_size 128, the payload tags carry payload_symbols)"""

    def __init__(self, header_size=256):
        self.header_size = header_size
        p = _abi.HeaderPayloadSplitParams(header_size, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_header_payload_split_create(C.byref(p), C.byref(self._h)), "HeaderPayloadSplit")

    def process_bulk(self, x, tags=None):
        """returns (header items, payload items, header tags, payload tags)"""
        torch = _torch()
        x = x.contiguous()
        assert x.is_cuda and x.dtype in (torch.float32, torch.complex64)
        t = _ptags_array(tags)
        hdr, pay = torch.empty(max(x.numel(), 1), dtype=x.dtype, device=x.device), torch.empty(
            max(x.numel(), 1), dtype=x.dtype, device=x.device)
        ht, pt = np.empty(t.size + 1, dtype=PACKET_TAG_DTYPE), np.empty(t.size + 1, dtype=PACKET_TAG_DTYPE)
        v = [C.c_size_t(0) for _ in range(4)]
        fn = (lib().gr4pm_header_payload_split_process if x.dtype == torch.float32
              else lib().gr4pm_header_payload_split_process_c64)
        check(fn(
            self._h, x.data_ptr(), x.numel(), hdr.data_ptr(), C.byref(v[0]), pay.data_ptr(), C.byref(v[1]),
            _np_ptr(t), t.size, _np_ptr(ht), C.byref(v[2]), _np_ptr(pt), C.byref(v[3]), t.size + 1),
            "HeaderPayloadSplit.processBulk")
        return hdr[: v[0].value], pay[: v[1].value], ht[: v[2].value], pt[: v[3].value]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_header_payload_split_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


def header_ldpc_alist():
    """the (128, 32) parity-check matrix of the header code in alist form
    (header_fec_decoder.hpp:31-258), shipped as data/header_ldpc_128_32.alist"""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    return open(os.path.join(here, "data", "header_ldpc_128_32.alist")).read()


class HeaderFecDecoder:
    """header_fec_decoder.hpp:13-359: 256 LLRs -> 4 header bytes, or invalid.  With another `alist` (an (n, m) code the
    decoder accepts, include/gr4pm_hip.h): llrs_per_codeword = 2 n LLRs -> header_bytes = (n - m) / 8 bytes"""

    def __init__(self, alist=None, max_iterations=25, arithmetic=0):
        """arithmetic: 0 float32 messages (default), 1 8-bit messages (include/gr4pm_hip.h)"""
        self._alist = (alist or header_ldpc_alist()).encode()
        p = _abi.HeaderFecDecoderParams(self._alist, max_iterations, _stream_handle(), arithmetic)
        self._h = C.c_void_p()
        check(lib().gr4pm_header_fec_decoder_create(C.byref(p), C.byref(self._h)), "HeaderFecDecoder.start")
        n_llrs, n_bytes = C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4pm_header_fec_decoder_dims(self._h, C.byref(n_llrs), C.byref(n_bytes)), "HeaderFecDecoder.start")
        self.llrs_per_codeword, self.header_bytes = n_llrs.value, n_bytes.value

    def process_bulk(self, llrs):
        """llrs: CUDA float32, llrs_per_codeword (256) per codeword.
        Returns (headers [n, header_bytes (4)] uint8, invalid [n] bool)"""
        torch = _torch()
        llrs = llrs.contiguous()
        assert llrs.is_cuda and llrs.dtype == torch.float32
        n = llrs.numel() // self.llrs_per_codeword
        out = np.empty((max(n, 1), self.header_bytes), dtype=np.uint8)
        inval = np.empty(max(n, 1), dtype=np.uint8)
        check(lib().gr4pm_header_fec_decoder_process(self._h, llrs.data_ptr(), n, _np_ptr(out), _np_ptr(inval)),
              "HeaderFecDecoder.processBulk")
        return out[:n], inval[:n].astype(bool)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_header_fec_decoder_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


def header_parse(headers, invalid=None):
    """HeaderParser, header_parser.hpp:46-95: [n, 4] bytes (+ the decoder's verdicts) -> the
    parsed_header messages as a HEADER_MSG_DTYPE array, and the packet types (-1 invalid)"""
    hd = np.ascontiguousarray(headers, dtype=np.uint8).reshape(-1, 4)
    inv = np.zeros(hd.shape[0], dtype=np.uint8) if invalid is None else np.ascontiguousarray(invalid, dtype=np.uint8)
    msgs = np.zeros(max(hd.shape[0], 1), dtype=_abi.HEADER_MSG_DTYPE)
    ptype = np.zeros(max(hd.shape[0], 1), dtype=np.int32)
    lib().gr4pm_header_parse(_np_ptr(hd), _np_ptr(inv), hd.shape[0], _np_ptr(msgs), _np_ptr(ptype))
    return msgs[: hd.shape[0]], ptype[: hd.shape[0]]


def _item_kind(x):
    torch = _torch()
    if x.dtype == torch.complex64:
        return 0
    if x.dtype == torch.float32:
        return 1
    raise TypeError("items must be complex64 or float32")


class InterpolatingFirFilter:
    """interpolating_fir_filter.hpp:14-103 (TIn = TOut in {c64, float}, TTaps = float)"""

    def __init__(self, interpolation, taps, item_dtype="complex64"):
        self.interpolation = interpolation
        self.taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.item_kind = 0 if item_dtype == "complex64" else 1
        p = _abi.InterpFirParams(interpolation, _np_ptr(self.taps), self.taps.size, self.item_kind, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_interp_fir_create(C.byref(p), C.byref(self._h)), "InterpolatingFirFilter")

    def process_bulk(self, x):
        torch = _torch()
        assert x.is_cuda and x.is_contiguous() and _item_kind(x) == self.item_kind
        out = torch.empty(x.numel() * self.interpolation, dtype=x.dtype, device=x.device)
        check(lib().gr4pm_interp_fir_process(self._h, x.data_ptr(), x.numel(), out.data_ptr()),
              "InterpolatingFirFilter.processBulk")
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_interp_fir_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class SymbolFilter:
    """symbol_filter.hpp:13-253"""

    def __init__(self, taps, num_arms, samples_per_symbol, delay=0, item_dtype="complex64"):
        self.taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.num_arms, self.samples_per_symbol, self.delay = num_arms, samples_per_symbol, delay
        self.item_kind = 0 if item_dtype == "complex64" else 1
        p = _abi.SymbolFilterParams(samples_per_symbol, _np_ptr(self.taps), self.taps.size, num_arms, delay,
                                    self.item_kind, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_symbol_filter_create(C.byref(p), C.byref(self._h)), "SymbolFilter")

    def start(self):
        check(lib().gr4pm_symbol_filter_reset(self._h), "start")

    def process_bulk(self, x, tags=None, out_cap=None):
        """returns (symbols, tags_out, consumed)"""
        torch = _torch()
        assert x.is_cuda and x.is_contiguous() and _item_kind(x) == self.item_kind
        t = _tags_array(tags)
        if out_cap is None:
            out_cap = x.numel() // self.samples_per_symbol + t.size + 2
        out = torch.empty(max(out_cap, 1), dtype=x.dtype, device=x.device)
        tout = np.zeros(t.size + 64, dtype=TAG_DTYPE)
        nto, cons, prod = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4pm_symbol_filter_process(self._h, x.data_ptr(), x.numel(), out.data_ptr(), out_cap, _np_ptr(t),
                                                t.size, _np_ptr(tout), tout.size, C.byref(nto), C.byref(cons),
                                                C.byref(prod)), "SymbolFilter.processBulk")
        return out[: prod.value], tout[: nto.value].copy(), cons.value

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_symbol_filter_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


def cfc_symbol_filter(cfc, symf, x, tags=None, out_cap=None):
    """CoarseFrequencyCorrection -> SymbolFilter in one pass (gr4pm_cfc_symbol_filter_process):
    identical results and state updates, the rotated stream is not materialised.
    Returns (symbols, tags_out, consumed)."""
    torch = _torch()
    x = _dev_c64(x)
    t = _tags_array(tags)
    if out_cap is None:
        out_cap = x.numel() // symf.samples_per_symbol + t.size + 2
    out = torch.empty(max(out_cap, 1), dtype=x.dtype, device=x.device)
    tout = np.zeros(t.size + 64, dtype=TAG_DTYPE)
    nto, cons, prod = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    check(lib().gr4pm_cfc_symbol_filter_process(cfc._h, symf._h, x.data_ptr(), x.numel(), out.data_ptr(), out_cap,
                                                _np_ptr(t), t.size, _np_ptr(tout), tout.size, C.byref(nto),
                                                C.byref(cons), C.byref(prod)), "cfc_symbol_filter")
    return out[: prod.value], tout[: nto.value].copy(), cons.value


def cfc_symbol_filter_plan(cfc, n_in, tags=None):
    """first half of cfc_symbol_filter (gr4pm_cfc_symbol_filter_plan): the CFC's tag handling and the
    phasor checkpoints of a call of n_in items; returns the plan id for cfc_symbol_filter_run"""
    t = _tags_array(tags)
    plan = C.c_int(-1)
    check(lib().gr4pm_cfc_symbol_filter_plan(cfc._h, n_in, _np_ptr(t), t.size, C.byref(plan)), "cfc_symbol_filter_plan")
    return plan.value


def cfc_symbol_filter_run(cfc, plan, symf, x, tags=None, out_cap=None):
    """second half (gr4pm_cfc_symbol_filter_run): the filter itself, on the SymbolFilter's stream;
    the caller makes sure the plan has completed.  Returns (symbols, tags_out, consumed)."""
    torch = _torch()
    x = _dev_c64(x)
    t = _tags_array(tags)
    if out_cap is None:
        out_cap = x.numel() // symf.samples_per_symbol + t.size + 2
    out = torch.empty(max(out_cap, 1), dtype=x.dtype, device=x.device)
    tout = np.zeros(t.size + 64, dtype=TAG_DTYPE)
    nto, cons, prod = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    check(lib().gr4pm_cfc_symbol_filter_run(cfc._h, plan, symf._h, x.data_ptr(), x.numel(), out.data_ptr(), out_cap,
                                            _np_ptr(t), t.size, _np_ptr(tout), tout.size, C.byref(nto),
                                            C.byref(cons), C.byref(prod)), "cfc_symbol_filter_run")
    return out[: prod.value], tout[: nto.value].copy(), cons.value


class PfbArbResampler:
    """pfb_arb_resampler.hpp:23-183 (<c64, c64, float, TRate>)"""

    def __init__(self, rate=1.0, taps=None, filter_size=32, rate_dtype="float32"):
        if taps is None:
            from . import default_pfb_arb_taps
            taps = default_pfb_arb_taps()
        self.rate, self.filter_size = rate, filter_size
        self.taps = np.ascontiguousarray(taps, dtype=np.float32)
        p = _abi.PfbArbParams(rate, 1 if rate_dtype == "float64" else 0, _np_ptr(self.taps), self.taps.size,
                              filter_size, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_pfb_arb_resampler_create(C.byref(p), C.byref(self._h)), "PfbArbResampler")

    def process_bulk(self, x, out_cap=None):
        """returns (out, consumed)"""
        torch = _torch()
        x = _dev_c64(x)
        if out_cap is None:
            out_cap = int(x.numel() * self.rate) + 64
        out = torch.empty(out_cap, dtype=x.dtype, device=x.device)
        cons, prod = C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4pm_pfb_arb_resampler_process(self._h, x.data_ptr(), x.numel(), out.data_ptr(), out_cap,
                                                    C.byref(cons), C.byref(prod)), "PfbArbResampler.processBulk")
        return out[: prod.value], cons.value

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_pfb_arb_resampler_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


# CCSDS syncword of the modem, packet_receiver.hpp:45-59
SYNCWORD = np.array(
    [0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1,
     0, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0],
    dtype=np.uint8)


def binary_slicer(x, invert=False):
    """BinarySlicer<invert>, binary_slicer.hpp:10-35: float32 soft symbols -> uint8 hard symbols"""
    torch = _torch()
    x = x.contiguous()
    assert x.is_cuda and x.dtype == torch.float32
    out = torch.empty(x.numel(), dtype=torch.uint8, device=x.device)
    check(lib().gr4pm_binary_slicer_process(x.data_ptr(), x.numel(), out.data_ptr(), 1 if invert else 0,
                                            _stream_handle()), "BinarySlicer")
    return out


def pack_bits(x, inputs_per_output=8, bits_per_input=1, msb_first=True):
    """PackBits<MSB|LSB, uint8_t, uint8_t>, pack_bits.hpp"""
    torch = _torch()
    x = x.contiguous()
    assert x.is_cuda and x.dtype == torch.uint8
    if x.numel() % inputs_per_output:
        raise Gr4pmError("input size not divisible by inputs_per_output")
    n_out = x.numel() // inputs_per_output
    out = torch.empty(n_out, dtype=torch.uint8, device=x.device)
    check(lib().gr4pm_pack_bits_process(x.data_ptr(), n_out, out.data_ptr(), inputs_per_output, bits_per_input,
                                        1 if msb_first else 0, _stream_handle()), "PackBits")
    return out


def slice_pack(llr):
    """BinarySlicer<true> + PackBits<>(8, 1) in one kernel (packet_receiver.hpp:140-144)"""
    torch = _torch()
    llr = llr.contiguous()
    assert llr.is_cuda and llr.dtype == torch.float32 and llr.numel() % 8 == 0
    out = torch.empty(llr.numel() // 8, dtype=torch.uint8, device=llr.device)
    check(lib().gr4pm_slice_pack_process(llr.data_ptr(), out.numel(), out.data_ptr(), _stream_handle()), "slice_pack")
    return out


class CrcCheck:
    """crc_check.hpp:22-239 (defaults = CRC-32, :61-66)"""

    def __init__(self, num_bits=32, poly=0x4C11DB7, initial_value=0xFFFFFFFF, final_xor=0xFFFFFFFF,
                 input_reflected=True, result_reflected=True, swap_endianness=False, discard_crc=False,
                 skip_header_bytes=0):
        p = _abi.CrcCheckParams(num_bits, poly, initial_value, final_xor, int(input_reflected), int(result_reflected),
                                int(swap_endianness), int(discard_crc), skip_header_bytes, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_crc_check_create(C.byref(p), C.byref(self._h)), "CrcCheck")

    def compute(self, data):
        d = np.ascontiguousarray(data, dtype=np.uint8)
        return int(lib().gr4pm_crc_check_compute(self._h, _np_ptr(d), d.size))

    def process_bulk(self, x, packet_len, packet_offset=None):
        """x: CUDA uint8 packets ("packet_len" tags = packet_len[], laid back to back unless
        packet_offset is given).  Returns (bytes of the packets that pass, out_len per packet)"""
        torch = _torch()
        x = x.contiguous()
        assert x.is_cuda and x.dtype == torch.uint8
        pl = np.ascontiguousarray(packet_len, dtype=np.uint64)
        po = (np.concatenate([[0], np.cumsum(pl)[:-1]]).astype(np.uint64) if packet_offset is None
              else np.ascontiguousarray(packet_offset, dtype=np.uint64))
        out = torch.empty(max(x.numel(), 1), dtype=torch.uint8, device=x.device)
        ol = np.zeros(max(pl.size, 1), dtype=np.uint64)
        n = C.c_size_t(0)
        check(lib().gr4pm_crc_check_process(self._h, x.data_ptr(), _np_ptr(po), _np_ptr(pl), pl.size, out.data_ptr(),
                                            _np_ptr(ol), C.byref(n)), "CrcCheck.processBulk")
        return out[: n.value], ol[: pl.size]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_crc_check_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class HeaderDecoder:
    """The header decode loop of packet_receiver.hpp:131-139 as one unit: AdditiveScrambler<float>
    (CCSDS 131.0-B-5 polynomial, reset at every "header_start") -> HeaderPayloadSplit ->
    HeaderFecDecoder -> HeaderParser.  Fed with the LLR stream and its tags
    (ConstellationLLRDecoder output); a header whose 256 LLRs end in a later call is finished
    there."""

    def __init__(self):
        self.descrambler = AdditiveScrambler(0x4001, 0x18E38, 16)  # :131-135
        self.header_payload_split = HeaderPayloadSplit(256)        # :136-137
        self.header_fec_decoder = HeaderFecDecoder()               # :138
        self._partial = None

    def process_bulk(self, llr, llr_tags):
        """returns dict(messages: HEADER_MSG_DTYPE per finished header, packet_type, header_bytes,
        invalid, payload_llr: descrambled payload LLRs, payload_tags)"""
        torch = _torch()
        t = _ptags_array(llr_tags)
        resets = t["index"][t["kind"] == _abi.PKT_HEADER_START]
        d = self.descrambler.process_bulk(llr, resets)
        hdr, pay, _, pay_tags = self.header_payload_split.process_bulk(d, t)
        if self._partial is not None:
            hdr = torch.cat([self._partial, hdr])
        n = hdr.numel() // 256
        self._partial = hdr[n * 256:].clone() if hdr.numel() % 256 else None
        hb, inval = self.header_fec_decoder.process_bulk(hdr[: n * 256])
        msgs, ptype = header_parse(hb, inval)
        return {"messages": msgs, "packet_type": ptype, "header_bytes": hb, "invalid": inval, "payload_llr": pay,
                "payload_tags": pay_tags}


class PacketReceiver:
    """The sample-rate / symbol-rate front half of gr::packet_modem::PacketReceiver
    (packet_receiver.hpp:34-127,191-232): SyncwordDetection -> SyncwordDetectionFilter ->
    CoarseFrequencyCorrection -> SymbolFilter -> SyncwordWipeoff -> CostasLoop, with every
    constant the reference constructor fixes.  Everything after CostasLoop (header decode,
    LDPC, CRC) is outside the hot path; the `parsed_header` feedback that the filter waits for
    is supplied by the caller (`header_fn(tag) -> packet_length | None`, or a constant).

    pipelined=True runs the chain as the reference's multi-threaded scheduler does (one worker
    per block, benchmarks/README.md:8-26), here as three stages on three HIP streams --
    detector | frequency correction + symbol filter + wipe-off | Costas loop -- so that the
    per-packet serial kernels (phasor checkpoints, PLL), which occupy only a few CUs, overlap
    the detector of the following batches.  process_bulk() then returns the result of an
    EARLIER batch (None while the pipeline fills); flush() drains it.

    soft_bits=True continues as packet_receiver.hpp:123-131 does: SyncwordWipeoff ->
    PayloadMetadataInsert (drops everything between packets, marks syncword / header / payload
    with "constellation" and "loop_bandwidth" tags) -> CostasLoop (those tags drive its settings)
    -> SyncwordRemove -> ConstellationLLRDecoder (noise_sigma 0.7, QPSK): the result then also
    carries "llr" (float32, two per symbol) and "llr_tags".

    decode_headers=True (implies soft_bits) closes the header feedback loop of
    packet_receiver.hpp:131-139,233-247 on the device instead of asking the caller for
    `header_fn`: descrambler -> HeaderPayloadSplit -> HeaderFecDecoder -> HeaderParser supply the
    parsed_header messages.  The reference resolves that loop packet by packet; a batch resolves
    it in two passes: (A) every detection is taken through a second set of the same blocks up to
    its header LLRs (its payload is dropped by answering "invalid_header"), which yields every
    candidate's header; (B) the real
    chain runs with those messages, and the headers it decodes itself are compared with the ones
    it was given (`header_mismatches` in the result; its payload LLRs leave descrambled as
    "payload_llr" / "payload_tags").  Pass A runs on a compact stream of one 228-symbol window
    per detection, so it costs a few percent of the real pass.  A header whose symbols continue in
    the next batch stays pending until then.  The payload tail follows (:140-147): BinarySlicer<true>,
    PackBits, CrcCheck(discard_crc) -- "packets" holds the bytes of the packets whose CRC-32 matches,
    "packet_lengths" their lengths (0 = dropped)."""

    def __init__(self, samples_per_symbol=4, syncword_freq_bins=4, syncword_threshold=9.5,
                 costas_constellation="QPSK", max_items=1 << 22, pipelined=False, fused=True,
                 soft_bits=False, decode_headers=False, detector=True):
        """detector=False: only the blocks behind SyncwordDetection are created (the caller feeds
        _stage1 / _stage2 from a detector of its own: MultiChannelPacketReceiver)"""
        torch = _torch()
        self.fused = fused  # CFC applied while the symbol filter stages its input
        self.decode_headers = decode_headers
        soft_bits = soft_bits or decode_headers
        self.soft_bits = soft_bits
        sps = samples_per_symbol
        self.samples_per_symbol = sps
        if decode_headers and sps < 4:  # as gr4pm_packet_receiver_create (see there)
            raise Gr4pmError(f"decode_headers needs at least 4 samples per symbol ({sps} given): below that the reference's "
                             "symbol filter loses the symbol clock at a detection and no header decodes")
        rrc = root_raised_cosine(1.0, float(sps), 1.0, 0.35, sps * 11)            # :60-65
        norm = np.float32(0.0)
        for v in rrc:                                                            # :67-74 (float accumulate)
            norm = np.float32(norm + np.float32(v * v))
        norm = np.float32(np.sqrt(norm))
        self.rrc_taps = (rrc / norm).astype(np.float32)
        bpsk = np.array([1, -1], dtype=np.complex64)
        self.pipelined = pipelined
        cur = torch.cuda.current_stream()
        self._streams = [torch.cuda.Stream() for _ in range(3)] if pipelined else [cur, cur, cur]
        self.syncword_detection = None
        if detector:
            with torch.cuda.stream(self._streams[0]):
                self.syncword_detection = SyncwordDetection(                      # :76-83
                    self.rrc_taps, SYNCWORD, bpsk, -syncword_freq_bins, syncword_freq_bins,
                    samples_per_symbol=sps, power_threshold=syncword_threshold, max_items=max_items)
        with torch.cuda.stream(self._streams[1]):
            self.syncword_detection_filter = SyncwordDetectionFilter(sps)         # :84-85
            self.freq_correction = CoarseFrequencyCorrection((self.rrc_taps.size - 1) // 2 + sps)  # :94-95
            arms = 32                                                             # :96
            pfb = root_raised_cosine(float(arms) / float(norm), float(arms * sps), 1.0, 0.35, arms * sps * 11)[:-1]  # :100-110
            self.symbol_filter = SymbolFilter(pfb, arms, sps, self.rrc_taps.size - 1)  # :111-115
            self.syncword_wipeoff = SyncwordWipeoff(np.where(SYNCWORD == 1, -1.0, 1.0).astype(np.float32))  # :117-122
            if decode_headers:  # pass A: the same blocks again, up to the header LLRs
                self._spec = {
                    "cfc": CoarseFrequencyCorrection((self.rrc_taps.size - 1) // 2 + sps),
                    "symf": SymbolFilter(pfb, arms, sps, self.rrc_taps.size - 1),
                    "wipeoff": SyncwordWipeoff(np.where(SYNCWORD == 1, -1.0, 1.0).astype(np.float32)),
                    "pmi": PayloadMetadataInsert(),
                    "costas": CostasLoop(),
                    "remove": SyncwordRemove(),
                    "llr": ConstellationLLRDecoder(0.7, "QPSK"),
                    "headers": HeaderDecoder(),
                }
                self._awaiting = np.zeros(0, dtype=np.uint64)   # detections whose window continues next batch
                self._awaiting_tags = np.zeros(0, dtype=TAG_DTYPE)
                self._spec_order = np.zeros(0, dtype=np.uint64)  # detections in pass A, header not out yet
                self._spec_fifo = np.zeros(0, dtype=_abi.HEADER_MSG_DTYPE)
                # pass A's window, in items: 64 and 912 at 4 samples per symbol (see _predecode)
                self._spec_pre, self._spec_w = self._SPEC_PRE_SYMBOLS * sps, self._SPEC_W_SYMBOLS * sps
                self._tail = torch.zeros(self._spec_w + self._spec_pre, dtype=torch.complex64, device="cuda")
                self._known_idx = np.zeros(0, dtype=np.uint64)  # candidates with a decoded header ...
                self._known_msg = np.zeros(0, dtype=_abi.HEADER_MSG_DTYPE)  # ... and the message
                self._pending_real = None                       # accepted packet waiting for its header
        with torch.cuda.stream(self._streams[2]):
            self.costas_loop = CostasLoop(0.01, costas_constellation)             # :125
            if soft_bits:
                self.payload_metadata_insert = PayloadMetadataInsert()            # :123-124
                self.costas_loop = CostasLoop()                                   # :125 (BPSK until the first tag)
                self.syncword_remove = SyncwordRemove()                           # :126
                self.constellation_decoder = ConstellationLLRDecoder(0.7, "QPSK")  # :129-130
            if decode_headers:
                self.header_decoder = HeaderDecoder()                             # :131-139
                self.payload_crc_check = CrcCheck(discard_crc=True)               # :145-147
                self._payload_carry = None   # soft bits of a payload that continues in the next batch
                self._payload_lens = np.zeros(0, dtype=np.uint64)  # bits of the payloads not finished yet
                self._used_msgs = np.zeros(0, dtype=_abi.HEADER_MSG_DTYPE)        # given to pass B, not yet verified
        # messages of accepted tags on their way to PayloadMetadataInsert: the symbol filter can
        # hold a tag of the last few samples back until the next call (symbol_filter.hpp:204-228)
        self._hdr_fifo = np.zeros(0, dtype=_abi.HEADER_MSG_DTYPE)
        self._workers = None
        self._inflight = []
        if pipelined:
            import concurrent.futures
            # the current device is a per-thread setting (torch and HIP alike): the workers take the creator's
            dev = _torch().cuda.current_device()
            self._workers = [concurrent.futures.ThreadPoolExecutor(max_workers=1, initializer=_torch().cuda.set_device,
                                                                   initargs=(dev,)) for _ in range(2)]

    # ---- the three stages
    def _stage0(self, x, tags_cap, history, next_x=None):
        torch = _torch()
        with torch.cuda.stream(self._streams[0]):
            st, y, det_tags, n = self.syncword_detection.process_bulk(x, want_output=history is None,
                                                                      tags_cap=tags_cap, next_x=next_x)
        if history is not None:
            # device-ring input: the delayed stream (hpp:318-319: out[i] = in[i - (2T+1)]) is read in
            # place from the ring instead of being copied
            d = 2 * self.syncword_detection.time_threshold + 1
            assert history.numel() >= d and history.data_ptr() + history.numel() * 8 == x.data_ptr(), \
                "history must be the ring contents that directly precede x"
            # as_strided takes the offset inside the STORAGE, not inside the view
            y = torch.as_strided(history, (n,), (1,), history.storage_offset() + history.numel() - d)
        base = self.syncword_detection._items_consumed - n        # absolute index of y[0]
        return st, y, det_tags, n, base

    def _stage1(self, st, y, det_tags, n, base, header_fn):
        torch = _torch()
        if st != 0:
            return {"status": st, "consumed": 0, "symbols": None, "tags": det_tags, "detector_tags": det_tags}
        if self.decode_headers:
            return self._stage1_decode(y, det_tags, n, base)
        with torch.cuda.stream(self._streams[1]):
            # SyncwordDetectionFilter: gate the tags; the samples pass unchanged
            if callable(header_fn):
                headers = [header_fn(t) for t in det_tags]
            elif header_fn is None:  # every header invalid
                headers = [None] * det_tags.size
            else:  # a constant packet_length
                headers = np.full(det_tags.size, int(header_fn), dtype=np.uint64)
            acc, _ = self.syncword_detection_filter.gate(base + det_tags["index"], headers, per_tag=True)
            tags = det_tags[acc]
            if self.fused:
                sym, sym_tags, consumed = cfc_symbol_filter(self.freq_correction, self.symbol_filter, y, tags)
            else:
                z = self.freq_correction.process_bulk(y, tags)
                sym, sym_tags, consumed = self.symbol_filter.process_bulk(z, tags)
            w = self.syncword_wipeoff.process_bulk(sym, sym_tags)
            self._hdr_fifo = np.concatenate([self._hdr_fifo, _header_msgs(headers)[0][: det_tags.size][acc]])
            hdrs, self._hdr_fifo = self._hdr_fifo[: sym_tags.size], self._hdr_fifo[sym_tags.size:]
        return {"status": 0, "consumed": n, "symbols": w, "tags": sym_tags, "detector_tags": det_tags,
                "accepted": acc, "headers": hdrs}

    # pass A works on a compact stream: one window of _SPEC_W_SYMBOLS symbols per detection, starting
    # _SPEC_PRE_SYMBOLS symbols before the tagged sample (room for the matched filter's history) and long
    # enough for syncword + header behind the filter delay: 16 + 11 + 192 < 228 symbols.  In items
    # (self._spec_pre, self._spec_w) that is samples_per_symbol times as much, as in the native receiver.
    _SPEC_PRE_SYMBOLS = 16
    _SPEC_W_SYMBOLS = 228

    def _predecode(self, y, det_tags, idx_abs, base):
        """pass A: the header of every detection (see the class docstring); updates the table of
        known headers.  A detection whose window runs past the end of this batch waits in
        self._awaiting and is decoded with the next batch (its first samples come from the saved
        tail of this one)."""
        torch = _torch()
        sp = self._spec
        n, W, pre = y.numel(), self._spec_w, self._spec_pre
        # window starts relative to y[0]: waiting detections of the last batch first (negative)
        old = self._awaiting.astype(np.int64) - np.int64(base) - pre
        new = det_tags["index"].astype(np.int64) - pre
        fits = new + W <= n
        starts = np.concatenate([old, new[fits]])
        tags = np.concatenate([self._awaiting_tags, det_tags[fits]])
        self._awaiting, self._awaiting_tags = idx_abs[~fits], det_tags[~fits].copy()
        k = starts.size
        if k:
            st = torch.from_numpy(starts).to(y.device)
            ar = torch.arange(W, device=y.device)
            inside = st >= 0
            compact = torch.empty((k, W), dtype=y.dtype, device=y.device)
            if bool(inside.all()):
                compact = y[st[:, None] + ar]
            else:  # a few windows begin in the previous batch: read them from [saved tail | head of y]
                head = torch.cat([self._tail, y[: W]])
                compact[inside] = y[st[inside][:, None] + ar]
                compact[~inside] = head[(st[~inside] + self._tail.numel())[:, None] + ar]
            ctags = tags.copy()
            ctags["index"] = np.arange(k, dtype=np.uint64) * np.uint64(W) + np.uint64(pre)
            inv = np.zeros(k, dtype=_abi.HEADER_MSG_DTYPE)
            inv["invalid_header"] = 1
            sym, sym_tags, _ = cfc_symbol_filter(sp["cfc"], sp["symf"], compact.reshape(-1), ctags)
            w = sp["wipeoff"].process_bulk(sym, sym_tags)
            self._spec_fifo = np.concatenate([self._spec_fifo, inv])
            hdrs, self._spec_fifo = self._spec_fifo[: sym_tags.size], self._spec_fifo[sym_tags.size:]
            pm = sp["pmi"].process_bulk(w, sym_tags, hdrs, per_tag=True)
            z = sp["costas"].process_packets(pm["out"], pm["tags"])
            d, dt = sp["remove"].process_bulk(z, pm["tags"])
            llr, lt = sp["llr"].process_bulk(d, dt)
            done = sp["headers"].process_bulk(llr, lt)["messages"]
            self._spec_order = np.concatenate([self._spec_order, np.concatenate([
                (old + np.int64(base) + pre).astype(np.uint64), idx_abs[fits]])])
            m = done.size
            self._known_idx = np.concatenate([self._known_idx, self._spec_order[:m]])
            self._known_msg = np.concatenate([self._known_msg, done])
            self._spec_order = self._spec_order[m:]
            order = np.argsort(self._known_idx, kind="stable")
            self._known_idx, self._known_msg = self._known_idx[order], self._known_msg[order]
        self._tail = y[-(W + pre):].clone()

    def _stage1_decode(self, y, det_tags, n, base):
        torch = _torch()
        with torch.cuda.stream(self._streams[1]):
            idx_abs = (base + det_tags["index"]).astype(np.uint64)
            self._predecode(y, det_tags, idx_abs, base)
            resolve = None
            if self._pending_real is not None:
                j = np.searchsorted(self._known_idx, self._pending_real)
                if j < self._known_idx.size and self._known_idx[j] == self._pending_real:
                    resolve = self._known_msg[j].copy()
                    self.syncword_detection_filter.gate_resolve(resolve)
                    self._pending_real = None
                    waiting = np.nonzero(self._hdr_fifo["invalid_header"] == 2)[0]
                    if waiting.size:  # its tag has not even reached PayloadMetadataInsert yet
                        self._hdr_fifo[waiting[0]] = resolve
                        resolve = None
            # per-tag messages: decoded / still on its way (2) / never decoded (1)
            msgs = np.zeros(det_tags.size, dtype=_abi.HEADER_MSG_DTYPE)
            msgs["invalid_header"] = 1
            j = np.searchsorted(self._known_idx, idx_abs)
            jc = np.minimum(j, max(self._known_idx.size - 1, 0))
            hit = (j < self._known_idx.size) & (self._known_idx[jc] == idx_abs) if self._known_idx.size else \
                np.zeros(det_tags.size, dtype=bool)
            msgs[hit] = self._known_msg[jc[hit]]
            msgs["invalid_header"][np.isin(idx_abs, self._awaiting) | np.isin(idx_abs, self._spec_order)] = 2
            acc, _ = self.syncword_detection_filter.gate(idx_abs, msgs, per_tag=True)
            tags, headers = det_tags[acc], msgs[acc]
            if headers.size and headers["invalid_header"][-1] == 2:
                self._pending_real = idx_abs[acc][-1]
            keep = self._known_idx + np.uint64(1 << 22) >= np.uint64(base)  # forget old entries
            self._known_idx, self._known_msg = self._known_idx[keep], self._known_msg[keep]
            sym, sym_tags, consumed = cfc_symbol_filter(self.freq_correction, self.symbol_filter, y, tags)
            w = self.syncword_wipeoff.process_bulk(sym, sym_tags)
            self._hdr_fifo = np.concatenate([self._hdr_fifo, headers])
            hdrs, self._hdr_fifo = self._hdr_fifo[: sym_tags.size], self._hdr_fifo[sym_tags.size:]
        return {"status": 0, "consumed": n, "symbols": w, "tags": sym_tags, "detector_tags": det_tags,
                "accepted": acc, "headers": hdrs, "resolve": resolve}

    def _stage2(self, res):
        torch = _torch()
        if res["status"] != 0:
            return res
        with torch.cuda.stream(self._streams[2]):
            if not self.soft_bits:
                res["symbols"] = self.costas_loop.process_bulk(res["symbols"], res["tags"])
                return res
            early_mismatch = 0
            if res.get("resolve") is not None:
                self.payload_metadata_insert.resolve(res["resolve"])
                if self.decode_headers:
                    waiting = np.nonzero(self._used_msgs["invalid_header"] == 2)[0]
                    early = getattr(self, "_early_hdrs", [])
                    if waiting.size:
                        self._used_msgs[waiting[0]] = res["resolve"]
                    elif early:  # the chain's own decode of that header came first: checked now
                        got0, r = early.pop(0), res["resolve"]
                        if not (r["invalid_header"] == got0["invalid_header"] and
                                (got0["invalid_header"] == 1 or r["packet_length"] == got0["packet_length"])):
                            early_mismatch = 1
            sym_in, tags_in, hdrs_in = res["symbols"], res["tags"], res["headers"]
            carry = getattr(self, "_pm_carry", None)
            if carry is not None:  # symbols PayloadMetadataInsert could not take in the batch before (below)
                csym, ctags, chdrs = carry
                tags_in = tags_in.copy()
                tags_in["index"] += csym.numel()
                sym_in = torch.cat([csym, sym_in])
                tags_in = np.concatenate([ctags, tags_in])
                hdrs_in = np.concatenate([chdrs, hdrs_in])
                self._pm_carry = None
            pm = self.payload_metadata_insert.process_bulk(sym_in, tags_in, hdrs_in, per_tag=True)
            if pm["consumed"] != sym_in.numel():
                # the block waits for a header that pass A delivers with the next batch (a batch that ends 204 .. 212 symbols
                # behind a syncword, payload_metadata_insert.hpp:243-247): the rest is carried, as in the native receiver
                rest = sym_in.numel() - pm["consumed"]
                if rest > 1024:
                    raise Gr4pmError(f"PayloadMetadataInsert stalled at symbol {pm['consumed']} of {sym_in.numel()}: "
                                     "a header message is missing")
                keep = tags_in["index"] >= pm["consumed"]
                ctags = tags_in[keep].copy()
                ctags["index"] -= pm["consumed"]
                self._pm_carry = (sym_in[pm["consumed"]:].clone(), ctags, hdrs_in[keep].copy())
            res["tags"], res["headers"] = tags_in, hdrs_in  # (what the bookkeeping below refers to)
            z = self.costas_loop.process_packets(pm["out"], pm["tags"])
            data, data_tags = self.syncword_remove.process_bulk(z, pm["tags"])
            llr, llr_tags = self.constellation_decoder.process_bulk(data, data_tags)
            res.update(symbols=z, packet_tags=pm["tags"], llr=llr, llr_tags=llr_tags,
                       ignored_syncwords=pm["ignored"])
            if self.decode_headers:
                # the chain's own header decode (packet_receiver.hpp:131-139): descrambled payload
                # LLRs for the consumers behind, and the check that pass A told the truth
                hd = self.header_decoder.process_bulk(llr, llr_tags)
                # messages of the packets PayloadMetadataInsert opened (it ignores syncwords inside a packet)
                opened_at = pm["tags"]["syncword"]["index"][pm["tags"]["kind"] == _abi.PKT_SYNCWORD]
                opened = res["headers"][np.isin(res["tags"]["index"], opened_at)]
                self._used_msgs = np.concatenate([self._used_msgs, opened])
                k = hd["messages"].size
                given, self._used_msgs = self._used_msgs[:k], self._used_msgs[k:]
                got = hd["messages"]
                same = (given["invalid_header"] == got["invalid_header"]) & \
                    ((given["packet_length"] == got["packet_length"]) | (got["invalid_header"] == 1))
                pending = given["invalid_header"] == 2  # pass A's message not there yet: checked when it arrives
                if pending.any():
                    self._early_hdrs = getattr(self, "_early_hdrs", []) + [got[i] for i in np.nonzero(pending)[0]]
                res.update(header_messages=got, header_bytes=hd["header_bytes"], packet_type=hd["packet_type"],
                           payload_llr=hd["payload_llr"], payload_tags=hd["payload_tags"],
                           header_mismatches=int(np.sum(~same & ~pending)) + early_mismatch)
                # payload tail, packet_receiver.hpp:140-147: BinarySlicer<true> -> PackBits -> CrcCheck
                # (which needs whole packets: an unfinished one waits for the next batch)
                soft = hd["payload_llr"] if self._payload_carry is None else torch.cat([self._payload_carry,
                                                                                       hd["payload_llr"]])
                lens = np.concatenate([self._payload_lens, hd["payload_tags"]["payload_bits"].astype(np.uint64)])
                ends = np.cumsum(lens)
                whole = int(np.searchsorted(ends, soft.numel(), side="right"))
                used = int(ends[whole - 1]) if whole else 0
                packed = slice_pack(soft[:used])
                data, out_len = self.payload_crc_check.process_bulk(packed, lens[:whole] // 8)
                self._payload_carry = soft[used:].clone() if used < soft.numel() else None
                self._payload_lens = lens[whole:]
                res.update(packets=data, packet_lengths=out_len, crc_ok=out_len > 0)
        return res

    def _stage12(self, fut1):
        return self._stage2(fut1.result())

    def announce(self, x):
        """the detector's look-ahead (SyncwordDetection.announce)"""
        self.syncword_detection.announce(x)

    def process_bulk(self, x, header_fn=None, tags_cap=4096, history=None, next_x=None):
        """x: complex64 CUDA tensor.  Returns dict(consumed, symbols, tags, detector_tags):
        symbols = CostasLoop output (one per symbol), tags = symbol-rate tags.  With
        pipelined=True the dict belongs to an earlier batch (None while the pipeline fills).
        history: when x is a window of a device ring buffer, the view of the >= 2T+1 items that
        precede x in the ring; the chain then reads the delayed stream in place (no copy).
        next_x: the window the next call will present (SyncwordDetection look-ahead)."""
        front = self._stage0(x, tags_cap, history, next_x)
        if not self.pipelined:
            return self._stage2(self._stage1(*front, header_fn))
        f1 = self._workers[0].submit(self._stage1, *front, header_fn)
        f2 = self._workers[1].submit(self._stage12, f1)
        self._inflight.append(f2)
        if len(self._inflight) > 2:  # keep at most two batches behind the detector
            return self._inflight.pop(0).result()
        return None

    def flush(self):
        """pipelined mode: results of the batches still in flight (oldest first)"""
        out = [f.result() for f in self._inflight]
        self._inflight = []
        return out


def mapper(x, map_values):
    """Mapper<uint8_t, c64 | float>, mapper.hpp:13-51: out[i] = map[x[i] & (len(map) - 1)]"""
    torch = _torch()
    x = x.contiguous()
    assert x.is_cuda and x.dtype == torch.uint8
    m = np.ascontiguousarray(map_values)
    kind = 0 if np.iscomplexobj(m) else 1
    m = m.astype(np.complex64 if kind == 0 else np.float32)
    out = torch.empty(x.numel(), dtype=torch.complex64 if kind == 0 else torch.float32, device=x.device)
    check(lib().gr4pm_mapper_process(x.data_ptr(), x.numel(), out.data_ptr(), _np_ptr(m), m.size, kind,
                                     _stream_handle()), "Mapper")
    return out


def burst_shaper(x, leading_shape, trailing_shape, packet_len, packet_offset=None):
    """BurstShaper, burst_shaper.hpp:47-126 over whole packets ("packet_len" tags = packet_len[],
    back to back unless packet_offset is given)"""
    torch = _torch()
    x = x.contiguous()
    assert x.is_cuda and x.dtype in (torch.complex64, torch.float32)
    lead = np.ascontiguousarray(leading_shape, dtype=np.float32)
    trail = np.ascontiguousarray(trailing_shape, dtype=np.float32)
    pl = np.ascontiguousarray(packet_len, dtype=np.uint64)
    po = (np.concatenate([[0], np.cumsum(pl)[:-1]]).astype(np.uint64) if packet_offset is None
          else np.ascontiguousarray(packet_offset, dtype=np.uint64))
    out = torch.empty_like(x)
    check(lib().gr4pm_burst_shaper_process(x.data_ptr(), x.numel(), out.data_ptr(), 0 if x.dtype == torch.complex64 else 1,
                                           _np_ptr(lead), lead.size, _np_ptr(trail), trail.size, _np_ptr(po), _np_ptr(pl),
                                           pl.size, _stream_handle()), "BurstShaper")
    return out


class BurstGenerator:
    """The burst path of PacketTransmitterPdu (packet_transmitter_pdu.hpp:84-337, stream_mode = false)
    plus the channel of apps/packet_transceiver.cpp:48-78, on the device, as a test-signal source:

        payload bytes + CRC-32  ->  [header (formatter, (128,32) LDPC + repetition) | payload] bits
        -> AdditiveScrambler (CCSDS 131.0-B-5, restarted per packet) -> PackBits(2) -> Mapper(QPSK)
        -> [syncword (BPSK) | header | payload | 9 ramp-down symbols | 11 zero symbols]
        -> InterpolatingFirFilter (4 samples/symbol, the transmitter's RRC) -> BurstShaper (sine ramps)
        -> gaps, Rotator (carrier offset), AWGN.

    Header formatting and its FEC encoding (32 bits per packet) and the CRC run on the host."""

    RAMP_DOWN, FLUSH = 9, 11   # :213-216, :209

    def __init__(self, samples_per_symbol=4, generator=None):
        import os
        self.sps = samples_per_symbol
        here = os.path.dirname(os.path.abspath(__file__))
        self.generator = np.fromfile(os.path.join(here, "data", "header_ldpc_generator.u32"), dtype="<u4") \
            if generator is None else np.ascontiguousarray(generator, dtype=np.uint32)
        taps = packet_transmitter_rrc_taps(samples_per_symbol)  # computed here, not shipped as data
        self.rrc_taps = taps
        self.fir = InterpolatingFirFilter(samples_per_symbol, taps)
        self.scrambler = AdditiveScrambler(0x4001, 0x18E38, 16, dtype="uint8")   # :118-122
        a = np.float32(np.sqrt(np.float32(2.0)) / np.float32(2.0))
        self.qpsk = np.array([a + 1j * a, a - 1j * a, -a + 1j * a, -a - 1j * a], dtype=np.complex64)  # :131-134
        ramp, offset = 4 * samples_per_symbol, 4 * samples_per_symbol                              # :296-300
        n_lead = offset + ramp
        self.leading = np.sin((np.arange(n_lead) + 1.0) / n_lead * 0.5 * np.pi).astype(np.float32)  # :301-306
        n_trail = self.FLUSH * samples_per_symbol - offset + ramp
        self.trailing = np.sin((np.arange(n_trail)[::-1] + 1.0) / n_trail * 0.5 * np.pi).astype(np.float32)  # :307-313

    def header_bits(self, packet_length, packet_type=0):
        """header_formatter.hpp:104-107 + header_fec_encoder.hpp:60-107 -> 256 bits"""
        info = ((packet_length >> 8) & 0xFF) << 24 | (packet_length & 0xFF) << 16 | (packet_type & 0xFF) << 8 | 0x55
        bits = [(info >> (31 - i)) & 1 for i in range(32)]
        bits += [bin(info & int(g)).count("1") & 1 for g in self.generator]
        return np.array(bits + bits, dtype=np.uint8)

    def symbols(self, payloads, packet_types=None):
        """packet symbols (device complex64) back to back, and the length of each packet in symbols"""
        import zlib
        torch = _torch()
        bits, resets, n_syms, pos = [], [], [], 0
        for k, data in enumerate(payloads):
            data = bytes(data)
            crc = zlib.crc32(data)
            body = np.frombuffer(data + crc.to_bytes(4, "big"), dtype=np.uint8)   # crc_append, :60-69
            b = np.concatenate([self.header_bits(len(data), 0 if packet_types is None else packet_types[k]),
                                np.unpackbits(body)])
            resets.append(pos)
            bits.append(b)
            pos += b.size
            n_syms.append(64 + b.size // 2 + self.RAMP_DOWN + self.FLUSH)
        allbits = torch.from_numpy(np.concatenate(bits)).cuda()
        scr = self.scrambler.process_bulk(allbits, np.array(resets, dtype=np.uint64))
        sym = mapper(pack_bits(scr, 2, 1), self.qpsk)                                           # :135-147
        sw = torch.from_numpy(np.where(SYNCWORD == 1, -1.0, 1.0).astype(np.complex64)).cuda()   # :158-181
        rng = np.random.default_rng(12345)
        parts, at = [], 0
        for k, b in enumerate(bits):
            n = b.size // 2
            ramp = torch.from_numpy(self.qpsk[rng.integers(0, 4, self.RAMP_DOWN)]).cuda()        # :211-247 (any data)
            parts += [sw, sym[at:at + n], ramp, torch.zeros(self.FLUSH, dtype=torch.complex64, device="cuda")]
            at += n
        return torch.cat(parts), np.array(n_syms, dtype=np.uint64)

    def bursts(self, payloads, packet_types=None):
        """shaped bursts back to back (device complex64) and their lengths in samples"""
        sym, n_syms = self.symbols(payloads, packet_types)
        self.fir = InterpolatingFirFilter(self.sps, self.rrc_taps)  # every call starts from a silent filter
        x = self.fir.process_bulk(sym)                                                           # :286-288
        lens = n_syms * np.uint64(self.sps)
        return burst_shaper(x, self.leading, self.trailing, lens), lens                         # :314-316

    def stream(self, payloads, gaps, freq_error=0.0, esn0_db=None, seed=1, tail=4000, packet_types=None,
               sfo_ppm=None, carrier="rotator"):
        """bursts separated by `gaps` (samples of silence before each burst) through the channel model of
        apps/packet_transceiver.cpp:48-78: PfbArbResampler<c64, c64, float> at rate 1 + 1e-6 sfo_ppm (sampling
        frequency offset; sfo_ppm=None leaves the block out), Rotator at freq_error rad/sample, AWGN for the
        given Es/N0 (tx power 0.32).  carrier="rotator" is the reference's Rotator (phasor recurrence, one serial
        lane for an untagged stream: 50 Msamples/s); carrier="closed_form" multiplies by exp(j freq_error n) from
        a double-precision phase instead -- a generator-only mode, not the reference's rounding, at HBM speed."""
        torch = _torch()
        x, lens = self.bursts(payloads, packet_types)
        total = int(np.sum(lens)) + int(np.sum(gaps)) + tail
        out = torch.zeros(total, dtype=torch.complex64, device="cuda")
        src = dst = 0
        for n, g in zip(lens, gaps):
            dst += int(g)
            out[dst:dst + int(n)] = x[src:src + int(n)]
            src += int(n)
            dst += int(n)
        if sfo_ppm is not None:                                                                  # :69-71
            rate = float(np.float32(1.0) + np.float32(1e-6) * np.float32(sfo_ppm))
            out, _ = PfbArbResampler(rate, rate_dtype="float32").process_bulk(out)
            total = out.numel()
        if freq_error and carrier == "closed_form":
            k = torch.arange(total, device="cuda", dtype=torch.float64)
            ph = torch.remainder(k * float(np.float32(freq_error)), 2.0 * np.pi)
            out = (out * torch.polar(torch.ones_like(ph), ph).to(torch.complex64)).contiguous()
        elif freq_error:
            out = Rotator(np.float32(freq_error)).process_bulk(out)                              # :72-73
        if esn0_db is not None:
            n0 = 0.32 * self.sps * 10.0 ** (-0.1 * esn0_db)                                      # :48-52
            g = torch.Generator(device="cuda")
            g.manual_seed(seed)
            # NoiseSource "amplitude" = sqrt(n0) is the standard deviation of the complex noise
            noise = torch.complex(torch.randn(total, generator=g, device="cuda"),
                                  torch.randn(total, generator=g, device="cuda")) * np.float32(np.sqrt(n0 / 2.0))
            out = (out + noise).to(torch.complex64)
        return out


class PacketTransmitter:
    """gr4pm_packet_transmitter: PacketTransmitterPdu (packet_transmitter_pdu.hpp:40-355) on the device.

    Burst mode: one shaped burst of samples_per_symbol * (4 L + 228) samples per packet (L payload bytes), with
    optional gaps of zeros in front; the ramp-down GLFSR runs on across bursts and calls until reset().  Stream mode:
    the packets back to back through one filter whose history carries over to the next call.  max_packets and
    max_payload_bytes bound one process_bulk() call."""

    USER_DATA, IDLE = 0, 1

    def __init__(self, stream_mode=False, samples_per_symbol=4, max_packets=1 << 14, max_payload_bytes=1 << 25):
        import os
        here = os.path.dirname(os.path.abspath(__file__))
        self._generator = np.fromfile(os.path.join(here, "data", "header_ldpc_generator.u32"), dtype="<u4")
        self.stream_mode, self.samples_per_symbol = bool(stream_mode), samples_per_symbol
        p = _abi.PacketTransmitterParams(samples_per_symbol, 1 if stream_mode else 0, max_packets, max_payload_bytes,
                                         _np_ptr(self._generator), _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_packet_transmitter_create(C.byref(p), C.byref(self._h)), "PacketTransmitter")

    def reset(self):
        check(lib().gr4pm_packet_transmitter_reset(self._h), "PacketTransmitter.reset")

    @staticmethod
    def _host_args(n, lengths, packet_types, gaps):
        lens = np.ascontiguousarray(lengths, dtype=np.uint64)
        if lens.size != n:
            raise Gr4pmError(f"PacketTransmitter: {lens.size} lengths for {n} packets")
        types = None
        if packet_types is not None:
            types = np.ascontiguousarray([{"USER_DATA": 0, "IDLE": 1}.get(t, t) if isinstance(t, str) else t
                                          for t in packet_types], dtype=np.int64)
            if types.size != n or types.min(initial=0) < 0 or types.max(initial=0) > 255:
                raise Gr4pmError("PacketTransmitter: one packet type per packet, 0 USER_DATA or 1 IDLE")
            types = types.astype(np.uint8)
        g = None if gaps is None else np.ascontiguousarray(gaps, dtype=np.uint64)
        if g is not None and g.size != n:
            raise Gr4pmError(f"PacketTransmitter: {g.size} gaps for {n} packets")
        return lens, types, g

    def output_items(self, lengths, packet_types=None, gaps=None):
        """samples process_bulk() makes for packets of these lengths"""
        lens, types, g = self._host_args(len(lengths), lengths, packet_types, gaps)
        n = C.c_size_t(0)
        check(lib().gr4pm_packet_transmitter_output_items(self._h, _np_ptr(lens), None if types is None else _np_ptr(types),
                                                          None if g is None else _np_ptr(g), lens.size, C.byref(n)),
              "PacketTransmitter.output_items")
        return n.value

    def process_bulk(self, payloads, packet_types=None, gaps=None, lengths=None, out=None):
        """payloads: a list of bytes, or a CUDA uint8 tensor of the packets back to back with `lengths`.
        packet_types: per packet 0 / "USER_DATA" or 1 / "IDLE" (None: all USER_DATA); gaps: samples of silence in
        front of each burst (burst mode).  out: an optional CUDA complex64 tensor to write into.
        Returns (samples, burst_offsets, burst_lengths)."""
        torch = _torch()
        if isinstance(payloads, torch.Tensor):
            if lengths is None:
                raise Gr4pmError("PacketTransmitter: a payload tensor needs `lengths`")
            if not payloads.is_cuda or payloads.dtype != torch.uint8:
                raise Gr4pmError("PacketTransmitter expects a CUDA uint8 tensor")
            data = payloads.contiguous()
        else:
            payloads = [bytes(b) for b in payloads]
            lengths = [len(b) for b in payloads]
            joined = np.frombuffer(b"".join(payloads), dtype=np.uint8)
            data = torch.from_numpy(joined.copy()).cuda() if joined.size else torch.empty(1, dtype=torch.uint8, device="cuda")
        _inputs_ready(data)
        n = len(lengths)
        lens, types, g = self._host_args(n, lengths, packet_types, gaps)
        if out is None:
            out = torch.empty(max(self.output_items(lens, types, g), 1), dtype=torch.complex64, device=data.device)
        elif not out.is_cuda or out.dtype != torch.complex64 or not out.is_contiguous():
            raise Gr4pmError("PacketTransmitter: out must be a contiguous CUDA complex64 tensor")
        offsets = np.zeros(max(n, 1), dtype=np.uint64)
        blens = np.zeros(max(n, 1), dtype=np.uint64)
        n_out = C.c_size_t(0)
        check(lib().gr4pm_packet_transmitter_process(self._h, data.data_ptr(), _np_ptr(lens),
                                                     None if types is None else _np_ptr(types),
                                                     None if g is None else _np_ptr(g), n, out.data_ptr(), out.numel(),
                                                     _np_ptr(offsets), _np_ptr(blens), C.byref(n_out)),
              "PacketTransmitter.processBulk")
        return out[: n_out.value], offsets[:n], blens[:n]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_packet_transmitter_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


def _hip_memcpy_d2d(dst, src, nbytes):
    """device-to-device copy through the HIP runtime the library is linked against"""
    import ctypes.util
    global _hiprt
    try:
        _hiprt
    except NameError:
        _hiprt = C.CDLL("libamdhip64.so")
        _hiprt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return 0 if _hiprt.hipMemcpy(dst, src, nbytes, 3) == 0 else -3


NOISE_TYPES = {"UNIFORM": 0, "GAUSSIAN": 1, "LAPLACIAN": 2, "IMPULSE": 3}


class NoiseSource:
    """gr4pm_noise_source: NoiseSource<T> (noise_source.hpp:45-110) on the device, bit-exact with the reference's
    sequential stream (ROCm clang++ against libstdc++) for any call size and chain of calls.  item: "c64" (UNIFORM,
    GAUSSIAN) or "float" (all four types).  The stream position stays on the device; reset() returns to start()."""

    def __init__(self, noise_type="gaussian", amplitude=1.0, seed=0, item="c64", max_items=1 << 24):
        t = NOISE_TYPES.get(str(noise_type).upper())
        if t is None:
            raise Gr4pmError(f"NoiseSource: unknown noise_type {noise_type}")  # enum_cast(...).value() throws
        if item not in ("c64", "float"):
            raise Gr4pmError(f"NoiseSource: item must be 'c64' or 'float', not {item!r}")
        self.noise_type, self.item, self.seed, self.max_items = str(noise_type).upper(), item, int(seed), max_items
        self._amplitude = float(np.float32(amplitude))
        p = _abi.NoiseSourceParams(0 if item == "c64" else 1, t, self._amplitude, self.seed, max_items, _stream_handle())
        self._h = C.c_void_p()
        check(lib().gr4pm_noise_source_create(C.byref(p), C.byref(self._h)), "NoiseSource")

    @property
    def amplitude(self):
        return self._amplitude

    @amplitude.setter
    def amplitude(self, value):
        """settingsChanged(): later items take the new amplitude, the stream position is kept"""
        self._amplitude = float(np.float32(value))
        check(lib().gr4pm_noise_source_set_amplitude(self._h, self._amplitude), "NoiseSource.amplitude")

    def reset(self):
        check(lib().gr4pm_noise_source_reset(self._h), "NoiseSource.reset")

    start = reset

    def process_bulk(self, n, add_to=None, out=None):
        """the next n items; add_to (a CUDA tensor of n items of the handle's kind): returns add_to + noise (Add's
        processOne(signal, noise)).  out: optional CUDA tensor to write into (may be add_to)."""
        torch = _torch()
        dt = torch.complex64 if self.item == "c64" else torch.float32
        if add_to is not None:
            if not add_to.is_cuda or add_to.dtype != dt or add_to.numel() != n:
                raise Gr4pmError(f"NoiseSource: add_to must be a CUDA {dt} tensor of {n} items")
            add_to = add_to.contiguous()
        if out is None:
            out = torch.empty(n, dtype=dt, device="cuda")
        elif not out.is_cuda or out.dtype != dt or out.numel() != n or not out.is_contiguous():
            raise Gr4pmError(f"NoiseSource: out must be a contiguous CUDA {dt} tensor of {n} items")
        check(lib().gr4pm_noise_source_process(self._h, None if add_to is None else add_to.data_ptr(), out.data_ptr(), n),
              "NoiseSource.processBulk")
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_noise_source_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class Channel:
    """The channel of apps/packet_transceiver.cpp:48-78: PfbArbResampler (SFO) -> Rotator (CFO) -> Add with a
    Gaussian NoiseSource<c64> (AWGN at Es/N0 for the transmitter's measured power of 0.32).  n0 = 0.32 sps
    10^(-esn0/10) in double, amplitude float(sqrt(n0)), resampling rate 1.0f + 1e-6f sfo_ppm in float.  Input the
    resampler leaves unconsumed is carried into the next call."""

    TX_POWER = 0.32

    def __init__(self, samples_per_symbol=4, esn0_db=20.0, cfo=0.0, sfo_ppm=0.0, seed=0, max_items=1 << 24):
        import math
        self.samples_per_symbol, self.esn0_db = samples_per_symbol, float(esn0_db)
        self.n0 = self.TX_POWER * float(samples_per_symbol) * math.pow(10.0, -0.1 * self.esn0_db)
        self.noise_amplitude = float(np.float32(math.sqrt(self.n0)))
        self.rate = float(np.float32(1.0) + np.float32(1e-6) * np.float32(sfo_ppm))
        self.resampler = PfbArbResampler(rate=self.rate)
        self.rotator = Rotator(cfo)
        self.noise = NoiseSource("gaussian", self.noise_amplitude, seed, "c64", max_items)
        self._carry = None

    def process_bulk(self, x):
        torch = _torch()
        x = _dev_c64(x)
        if self._carry is not None and self._carry.numel():
            x = torch.cat([self._carry, x])
        y, consumed = self.resampler.process_bulk(x)
        self._carry = x[consumed:].clone()
        y = self.rotator.process_bulk(y.contiguous())
        return self.noise.process_bulk(y.numel(), add_to=y, out=y)


IQ_FORMATS = {"sc16": _abi.IQ_SC16, "sc8": _abi.IQ_SC8, "cu8": _abi.IQ_CU8}


def _iq_dtypes():
    torch = _torch()
    return {torch.int16: _abi.IQ_SC16, torch.int8: _abi.IQ_SC8, torch.uint8: _abi.IQ_CU8}


def _dev_iq(x, what="x"):
    """integer IQ: a CUDA tensor of dtype int16 (sc16), int8 (sc8) or uint8 (cu8), [n, 2] or [rows, n, 2] with (I, Q)
    adjacent and the items of a row contiguous; the row stride is free.  Returns (format, rows, n, row stride in items)."""
    torch = _torch()
    fmt = _iq_dtypes().get(x.dtype) if isinstance(x, torch.Tensor) else None
    if fmt is None or not x.is_cuda or x.dim() not in (2, 3) or x.shape[-1] != 2:
        raise TypeError(f"{what} must be a CUDA int16 / int8 / uint8 tensor of shape [n, 2] or [rows, n, 2]")
    n = x.shape[-2]
    if x.numel() and (x.stride(-1) != 1 or (n > 1 and x.stride(-2) != 2)):
        raise TypeError(f"{what}: the items of a row must be contiguous")
    if x.dim() == 2:
        return fmt, 1, n, n
    if x.shape[0] > 1 and (x.stride(0) % 2 or x.stride(0) < 2 * n):
        raise TypeError(f"{what}: a row stride of {x.stride(0)} components for rows of {n} items")
    return fmt, x.shape[0], n, (x.stride(0) // 2 if x.shape[0] > 1 else n)


def _dev_c64_iq(x, what):
    """the complex64 side of a conversion: [n], or [rows, n] with contiguous rows.  Returns (rows, n, row stride)"""
    torch = _torch()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.complex64 and x.dim() in (1, 2)):
        raise TypeError(f"{what} must be a CUDA complex64 tensor of shape [n] or [rows, n]")
    if x.dim() == 1:
        if x.numel() > 1 and x.stride(0) != 1:
            raise TypeError(f"{what} must be contiguous")
        return 1, x.shape[0], x.shape[0]
    x = _dev_c64_rows(x, what)
    return x.shape[0], x.shape[1], (x.stride(0) if x.shape[0] > 1 else x.shape[1])


def iq_unpack(x, scale=None, out=None):
    """gr4pm_iq_unpack: integer IQ (see _dev_iq: the format follows from the dtype) to complex64 on the device, on the
    current stream.  Per component float(v) * scale, cu8: (float(v) - 127.5) * scale; scale None: 2^-15 (sc16) or 2^-7.
    Returns complex64 [n] or [rows, n]; out: an optional tensor of that shape (rows contiguous, any row stride)."""
    torch = _torch()
    fmt, rows, n, stride = _dev_iq(x)
    shape = (n,) if x.dim() == 2 else (rows, n)
    if out is None:
        out = torch.empty(shape, dtype=torch.complex64, device=x.device)
    orows, on, ostride = _dev_c64_iq(out, "out")
    if tuple(out.shape) != shape:
        raise Gr4pmError(f"iq_unpack: out is {tuple(out.shape)}, the call makes {shape}")
    check(lib().gr4pm_iq_unpack(x.data_ptr(), stride, fmt, 0.0 if scale is None else float(scale), rows, n, out.data_ptr(),
                                ostride, _stream_handle()), "iq_unpack")
    return out


def iq_pack(x, fmt, gain=None, out=None, clipped=None):
    """gr4pm_iq_pack: complex64 [n] or [rows, n] to integer IQ [n, 2] or [rows, n, 2] on the device, on the current
    stream.  fmt: "sc16", "sc8" or "cu8".  Per component rint(x * gain) (cu8: rint(x * gain + 127.5)), ties to even,
    clamped to the type's range, NaN: 0 (cu8: 128); gain None: 2^15 (sc16) or 2^7.  clipped: an optional one-element
    int64 CUDA tensor the call adds the number of clamped or NaN components to.  out: an optional tensor to write into."""
    torch = _torch()
    f = IQ_FORMATS.get(str(fmt).lower())
    if f is None:
        raise Gr4pmError(f"iq_pack: unknown format {fmt!r} (sc16, sc8 or cu8)")
    dtype = {v: k for k, v in _iq_dtypes().items()}[f]
    rows, n, stride = _dev_c64_iq(x, "x")
    shape = (n, 2) if x.dim() == 1 else (rows, n, 2)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=x.device)
    ofmt, orows, on, ostride = _dev_iq(out, "out")
    if ofmt != f or tuple(out.shape) != shape:
        raise Gr4pmError(f"iq_pack: out is {out.dtype} {tuple(out.shape)}, the call makes {dtype} {shape}")
    if clipped is not None and not (isinstance(clipped, torch.Tensor) and clipped.is_cuda and clipped.dtype == torch.int64
                                    and clipped.numel() == 1):
        raise TypeError("clipped must be a one-element int64 CUDA tensor")
    check(lib().gr4pm_iq_pack(x.data_ptr(), stride, rows, n, f, 0.0 if gain is None else float(gain), out.data_ptr(), ostride,
                              None if clipped is None else clipped.data_ptr(), _stream_handle()), "iq_pack")
    return out


def _iq_out(what, fmt, samples, out, clipped, device):
    """the integer side of a transmit bank's process_bulk(format=...): the format's number, the tensor [>= samples, 2]
    of iq_pack's dtype that the call writes (out, or a new one) and the counter's address or None"""
    torch = _torch()
    f = IQ_FORMATS.get(str(fmt).lower())
    if f is None:
        raise Gr4pmError(f"{what}: unknown format {fmt!r} (sc16, sc8 or cu8)")
    dtype = {v: k for k, v in _iq_dtypes().items()}[f]
    if out is None:
        out = torch.empty((samples, 2), dtype=dtype, device=device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dtype and out.dim() == 2 and out.shape[1] == 2
              and out.is_contiguous()):
        raise Gr4pmError(f"{what}: out must be a contiguous CUDA {dtype} tensor [n, 2] for format {fmt!r}")
    elif out.shape[0] < samples:
        raise Gr4pmError(f"{what}: out is {tuple(out.shape)}, the call makes [{samples}, 2]")
    if clipped is not None and not (isinstance(clipped, torch.Tensor) and clipped.is_cuda and clipped.dtype == torch.int64
                                    and clipped.numel() == 1):
        raise TypeError("clipped must be a one-element int64 CUDA tensor")
    return f, out, (None if clipped is None else clipped.data_ptr())


def _design_taps(entry, ratio, per, passband, stopband, what):
    """a gr4pm_*_taps entry: the design of per * ratio float32 taps"""
    n = int(ratio) * int(per)
    out = np.zeros(max(n, 1), dtype=np.float32)
    check(getattr(lib(), entry)(int(ratio), int(per), float(passband), float(stopband), _np_ptr(out)), what)
    return out[:n]


def _stream_input(x, scale, stream):
    """What a front-end block's process_bulk() takes: a contiguous complex64 CUDA tensor [n], or integer IQ [n, 2] (see
    _dev_iq) with an optional scale; handed over to the handle's stream.  Returns (x, n, the format or None for complex64,
    the scale as the C entry takes it)."""
    torch = _torch()
    fmt = None
    if isinstance(x, torch.Tensor) and x.dtype in _iq_dtypes():
        fmt, _, n_in, _ = _dev_iq(x)
        if x.dim() != 2:
            raise TypeError("x must be [n, 2]")
    else:
        if scale is not None:
            raise TypeError("scale applies to integer IQ only")
        x = _dev_c64(x, "x")
        if x.dim() != 1:
            raise TypeError("x must be one-dimensional")
        n_in = x.numel()
    if torch.cuda.current_stream(x.device).cuda_stream != stream:
        _inputs_ready(x)  # made on another stream than the handle's
    return x, n_in, fmt, 0.0 if scale is None else float(scale)


def _rows_output(out, rows, frames, device, what):
    """the [rows, frames] complex64 result: a new tensor, or the caller's [rows, >= frames] with contiguous rows"""
    if out is None:
        return _torch().empty((rows, frames), dtype=_torch().complex64, device=device)
    out = _dev_c64_rows(out, "out")
    if out.shape[0] != rows or out.shape[1] < frames:
        raise Gr4pmError(f"{what}: out is {tuple(out.shape)}, the call makes [{rows}, {frames}]")
    return out


def _xlate_settings(what, frequencies, ratio, taps, taps_per_phase, start_index, design):
    """the settings Ddc and Duc share: (frequencies as float64, float32 taps, start_index)"""
    f = np.ascontiguousarray(np.atleast_1d(np.asarray(frequencies, dtype=np.float64)))
    if f.ndim != 1:
        raise Gr4pmError(f"{what}: frequencies must be a list of numbers")
    if taps is not None:
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        if not taps.size:
            raise Gr4pmError(f"{what}: the prototype has 1 .. 8192 taps, not 0")
    else:
        taps = design(ratio, taps_per_phase)
    start_index = int(start_index)
    if not 0 <= start_index < 1 << 64:
        raise Gr4pmError(f"{what}: start_index must fit 64 unsigned bits")
    return f, taps, start_index


def _destroy(self, entry):
    """a __del__: the handle goes once; silent at interpreter shutdown"""
    try:
        if getattr(self, "_h", None):
            _release(entry, self._h)
            self._h = None
    except Exception:
        pass


def channelizer_taps(n_channels, taps_per_branch=12, passband=0.25, stopband=0.75):
    """gr4pm_channelizer_taps: the Channelizer's prototype low-pass, a Kaiser-windowed sinc of taps_per_branch *
    n_channels float32 taps with DC gain 1 (host only: works without a GPU).  passband / stopband: the band edges in
    units of the channel spacing.  The defaults suit the transmitter's RRC at 4 samples per symbol (occupied to 0.169
    of the spacing; the neighbour's band starts at 0.831)."""
    return _design_taps("gr4pm_channelizer_taps", n_channels, taps_per_branch, passband, stopband, "channelizer_taps")


class Channelizer:
    """gr4pm_channelizer: critically sampled polyphase analysis bank.  One wideband complex64 stream at fs becomes
    n_channels (a power of two, 2 .. 1024) channels at fs / n_channels: row k is the band at +k fs / n_channels
    (k > n_channels / 2: negative frequencies, as an FFT orders them), so that
    NativeMultiChannelReceiver.submit(Channelizer(...).process_bulk(x)) is a wideband receiver.
    taps: taps_per_branch * n_channels float32 prototype taps (None: channelizer_taps(n_channels, taps_per_branch)).
    select: channel numbers to deliver, in this order (None: all).  process_bulk() takes any number of samples; the
    filter history and the samples of an incomplete frame stay on the device.  The handle works on the stream that is
    current when it is made."""

    def __init__(self, n_channels, taps=None, taps_per_branch=12, select=None, max_frames=1 << 22):
        self.n_channels = int(n_channels)
        if taps is not None:
            self.taps = np.ascontiguousarray(taps, dtype=np.float32)
            if self.n_channels < 1 or self.taps.size % self.n_channels or not self.taps.size:
                raise Gr4pmError(f"Channelizer: {self.taps.size} taps are not a multiple of {self.n_channels} channels")
            taps_per_branch = self.taps.size // self.n_channels
        else:
            self.taps = channelizer_taps(self.n_channels, taps_per_branch)
        self.taps_per_branch = int(taps_per_branch)
        self.select = None if select is None else [int(k) for k in select]
        if self.select is not None and (not self.select or min(self.select) < 0):
            raise Gr4pmError("Channelizer: select must be a non-empty list of channel numbers")
        sel = np.ascontiguousarray(self.select if self.select is not None else [], dtype=np.uint32)
        self.n_rows = sel.size if self.select is not None else self.n_channels
        self.max_frames = int(max_frames)
        stream = _stream_handle()
        self._stream = stream.value
        p = _abi.ChannelizerParams(self.n_channels, self.taps_per_branch, _np_ptr(self.taps), sel.size,
                                   _np_ptr(sel) if sel.size else None, self.max_frames, stream)
        self._h = C.c_void_p()
        check(lib().gr4pm_channelizer_create(C.byref(p), C.byref(self._h)), "Channelizer")

    def output_items(self, n_in):
        """frames (items per row) the next process_bulk() of n_in samples produces"""
        n = C.c_size_t(0)
        check(lib().gr4pm_channelizer_output_items(self._h, int(n_in), C.byref(n)), "Channelizer.output_items")
        return n.value

    def reset(self):
        """back to the fresh stream: zero history, no carried samples"""
        check(lib().gr4pm_channelizer_reset(self._h), "Channelizer.reset")

    def process_bulk(self, x, out=None, scale=None):
        """x: a contiguous CUDA complex64 tensor of any length (all of it is consumed), or integer IQ: an int16 (sc16),
        int8 (sc8) or uint8 (cu8) CUDA tensor [n, 2], converted as iq_unpack(x, scale) does where the kernel loads it
        (gr4pm_channelizer_process_iq: the same result bit for bit; calls of any format mix on one handle).  Returns
        y[n_rows, frames]; out: an optional CUDA complex64 [n_rows, >= frames] tensor with contiguous rows and any row
        stride (a window of a receiver's ring) to write into."""
        x, n_in, fmt, scale = _stream_input(x, scale, self._stream)
        out = _rows_output(out, self.n_rows, self.output_items(n_in), x.device, "Channelizer")
        n = C.c_size_t(0)
        if fmt is None:
            check(lib().gr4pm_channelizer_process(self._h, x.data_ptr(), n_in, out.data_ptr(), out.stride(0),
                                                  out.shape[1], C.byref(n)), "Channelizer.process")
        else:
            check(lib().gr4pm_channelizer_process_iq(self._h, x.data_ptr(), fmt, scale, n_in, out.data_ptr(), out.stride(0),
                                                     out.shape[1], C.byref(n)), "Channelizer.process_iq")
        return out[:, : n.value]

    def __del__(self):
        _destroy(self, "gr4pm_channelizer_destroy")


def ddc_taps(decimation, taps_per_phase=12, passband=0.25, stopband=0.75):
    """gr4pm_ddc_taps: the Ddc's prototype low-pass, the Kaiser design of channelizer_taps with taps_per_phase *
    decimation float32 taps for any integer decimation, DC gain 1 (host only: works without a GPU).  passband /
    stopband: the band edges in units of the output rate.  For a power-of-two decimation the floats are those of
    channelizer_taps."""
    return _design_taps("gr4pm_ddc_taps", decimation, taps_per_phase, passband, stopband, "ddc_taps")


def ddc_rational_taps(interpolation, decimation, taps_per_phase=12, passband=0.25, stopband=0.75):
    """gr4pm_ddc_rational_taps: the prototype low-pass of a Ddc that resamples by interpolation / decimation, at the
    rate interpolation * fs: the Kaiser design of ddc_taps with taps_per_phase * decimation float32 taps and DC gain
    `interpolation`, scaled in double before the one rounding to float32 (host only: works without a GPU).  passband /
    stopband: the band edges in units of the output rate; a cutoff beyond half of the lower of the input and the output
    rate (passband + stopband > min(1, decimation / interpolation)) is refused.  With interpolation = 1 the floats are
    those of ddc_taps."""
    n = int(decimation) * int(taps_per_phase)
    out = np.zeros(max(n, 1), dtype=np.float32)
    check(lib().gr4pm_ddc_rational_taps(int(interpolation), int(decimation), int(taps_per_phase), float(passband),
                                        float(stopband), _np_ptr(out)), "ddc_rational_taps")
    return out[:n]


def ddc_burst_span(start_sample, end_sample, decimation, n_taps, start_index=0, margin_frames=0):
    """hostlogic/extract_plan.hpp's burst_span in Python integers (host only: works without a GPU): (first_frame,
    n_frames) of the frames of a Ddc(decimation, n_taps taps, start_index) that see the samples [start_sample,
    end_sample), widened by margin_frames on either side.  From max(0, floor((start_sample - start_index) / decimation)
    - margin_frames), the first frame whose newest sample is at or after start_sample, to ceil((end_sample - start_index
    + n_taps - 1) / decimation) + margin_frames, a frame whose oldest sample is at or after end_sample; both clamped to
    the frames whose sample indices fit 64 bits.  An empty burst gives (0, 0)."""
    start, end, D, L, s0, m = (int(v) for v in (start_sample, end_sample, decimation, n_taps, start_index, margin_frames))
    if D < 1 or L < 1 or m < 0 or min(start, end, s0) < 0 or max(start, end, s0) >= 1 << 64:
        raise Gr4pmError("ddc_burst_span: decimation and n_taps from 1, no negative margin, indices of 64 unsigned bits")
    most = (1 << 64) - 2 - max(s0, L - 1)
    if end <= start or most // D < 1:
        return 0, 0
    first = max(0, (start - s0) // D - m) if start > s0 else 0
    last = min(-(-max(0, end - s0 + L - 1) // D) + m, most // D - 1)
    first = min(first, last)
    if last - first + 1 >= 1 << 32:
        raise Gr4pmError(f"ddc_burst_span: {last - first + 1} frames do not fit a span's 32 bits")
    return first, last - first + 1


class Ddc:
    """gr4pm_ddc: tunable down-converter.  One wideband complex64 stream at fs becomes len(frequencies) channels at
    fs / decimation: row k is the band centred on frequencies[k] (cycles per input sample, any real value, quantised to
    fs / 2^32: .frequencies holds the values in use, folded to [-0.5, 0.5)), mixed to 0, low-pass filtered and
    decimated by any integer 1 .. 1024, so that NativeMultiChannelReceiver.submit(Ddc(...).process_bulk(x)) receives
    carriers that sit on no grid.  taps: 1 .. 8192 float32 prototype taps of any length (None: ddc_taps(decimation,
    taps_per_phase)).  start_index: the absolute index of the first sample (the phase of a channel follows from the
    absolute index in integer arithmetic, exactly, at any stream position).  process_bulk() takes any number of
    samples; the filter history and the samples of an incomplete frame stay on the device.  Frequencies are fixed: make
    another Ddc to retune.  The handle works on the stream that is current when it is made.

    interpolation = I > 1 (at most 64) resamples by I / decimation in the same pass (gr4pm_ddc_create_rational): the
    output rate is fs I / decimation (.rate, a Fraction), N samples make floor(N I / decimation) items per row, and
    the prototype (None: ddc_rational_taps(I, decimation, taps_per_phase)) runs at I fs.  Without taps the pair is
    reduced to lowest terms (.interpolation and .decimation hold the reduced values); with taps a pair that is not in
    lowest terms is refused, since the taps belong to one rate.  max_frames bounds the items of one call."""

    def __init__(self, frequencies, decimation, interpolation=1, taps=None, taps_per_phase=12, start_index=0,
                 max_frames=1 << 22):
        self.decimation, self.interpolation = int(decimation), int(interpolation)
        if self.interpolation > 1 and self.decimation >= 1:
            g = math.gcd(self.interpolation, self.decimation)
            if g > 1 and taps is not None:
                raise Gr4pmError(f"Ddc: {self.interpolation} / {self.decimation} is not in lowest terms, and the taps "
                                 f"belong to one rate: use {self.interpolation // g} / {self.decimation // g}")
            if g > 1:
                self.decimation, self.interpolation = self.decimation // g, self.interpolation // g
        if self.interpolation == 1:
            design = ddc_taps
        else:
            design = lambda d, per: ddc_rational_taps(self.interpolation, d, per)
        f, self.taps, self.start_index = _xlate_settings("Ddc", frequencies, self.decimation, taps, taps_per_phase,
                                                         start_index, design)
        self.rate = fractions.Fraction(self.interpolation, self.decimation) if self.decimation > 0 else None
        self.n_channels = self.n_rows = int(f.size)
        self.max_frames = int(max_frames)
        stream = _stream_handle()
        self._stream = stream.value
        self._h = C.c_void_p()
        if self.interpolation == 1:
            p = _abi.DdcParams(self.n_channels, self.decimation, _np_ptr(f) if f.size else None, _np_ptr(self.taps),
                               self.taps.size, self.max_frames, self.start_index, stream)
            check(lib().gr4pm_ddc_create(C.byref(p), C.byref(self._h)), "Ddc")
        else:
            p = _abi.DdcRationalParams(self.n_channels, self.decimation, _np_ptr(f) if f.size else None,
                                       _np_ptr(self.taps), self.taps.size, self.max_frames, self.start_index, stream,
                                       self.interpolation)
            check(lib().gr4pm_ddc_create_rational(C.byref(p), C.byref(self._h)), "Ddc")
        q = np.zeros(self.n_channels, dtype=np.float64)
        check(lib().gr4pm_ddc_frequencies(self._h, _np_ptr(q)), "Ddc.frequencies")
        self.frequencies = q

    def output_items(self, n_in):
        """items per row the next process_bulk() of n_in samples produces"""
        n = C.c_size_t(0)
        check(lib().gr4pm_ddc_output_items(self._h, int(n_in), C.byref(n)), "Ddc.output_items")
        return n.value

    def reset(self):
        """back to start_index: zero history, no carried samples"""
        check(lib().gr4pm_ddc_reset(self._h), "Ddc.reset")

    def process_bulk(self, x, out=None, scale=None):
        """x: a contiguous CUDA complex64 tensor of any length (all of it is consumed), or integer IQ: an int16 (sc16),
        int8 (sc8) or uint8 (cu8) CUDA tensor [n, 2], converted as iq_unpack(x, scale) does where the kernel loads it
        (gr4pm_ddc_process_iq: the same result bit for bit; calls of any format mix on one handle).  Returns
        y[n_channels, frames]; out: an optional CUDA complex64 [n_channels, >= frames] tensor with contiguous rows and
        any row stride (a window of a receiver's ring) to write into."""
        x, n_in, fmt, scale = _stream_input(x, scale, self._stream)
        out = _rows_output(out, self.n_channels, self.output_items(n_in), x.device, "Ddc")
        n = C.c_size_t(0)
        stride = out.stride(0) if self.n_channels > 1 else out.shape[1]
        if fmt is None:
            check(lib().gr4pm_ddc_process(self._h, x.data_ptr(), n_in, out.data_ptr(), stride, out.shape[1], C.byref(n)),
                  "Ddc.process")
        else:
            check(lib().gr4pm_ddc_process_iq(self._h, x.data_ptr(), fmt, scale, n_in, out.data_ptr(), stride, out.shape[1],
                                             C.byref(n)), "Ddc.process_iq")
        return out[:, : n.value]

    SPAN_DTYPE = np.dtype([("channel", np.uint32), ("n_frames", np.uint32), ("first_frame", np.uint64)])  # gr4pm_ddc_span
    SPANS_PER_CALL = 64

    def _spans(self, spans):
        """spans as a contiguous SPAN_DTYPE array: from one, or from a sequence of (channel, first_frame, n_frames)"""
        if isinstance(spans, np.ndarray) and spans.dtype.names:
            if set(spans.dtype.names) != set(self.SPAN_DTYPE.names):
                raise Gr4pmError(f"Ddc.extract: a structured spans array has the fields {self.SPAN_DTYPE.names}")
            rec = np.zeros(spans.shape, dtype=self.SPAN_DTYPE)
            for name in self.SPAN_DTYPE.names:
                rec[name] = spans[name]
            return np.ascontiguousarray(rec.reshape(-1))
        rec = np.zeros(len(spans), dtype=self.SPAN_DTYPE)
        for b, (channel, first_frame, n_frames) in enumerate(spans):
            channel, first_frame, n_frames = int(channel), int(first_frame), int(n_frames)
            if not (0 <= channel < 1 << 32 and 0 <= first_frame < 1 << 64 and 0 <= n_frames < 1 << 32):
                raise Gr4pmError(f"Ddc.extract: spans[{b}] = ({channel}, {first_frame}, {n_frames}) does not fit "
                                 "(uint32 channel, uint64 first_frame, uint32 n_frames)")
            rec[b] = (channel, n_frames, first_frame)
        return rec

    def extract(self, x, spans, n_cols=None, x_index=None, out=None, scale=None):
        """gr4pm_ddc_extract: spans of the handle's output, computed from a recording on their own.  x: the recording (or
        a window of it), complex64 or integer IQ exactly as in process_bulk; x_index: the absolute index of x[0] (None:
        the handle's start_index).  The stream is x inside [x_index, x_index + len(x)) and zero elsewhere, and before
        start_index.  spans: a sequence of (channel, first_frame, n_frames), or a structured array of SPAN_DTYPE; frames
        are numbered from start_index as process_bulk numbers them from a fresh handle.  Returns (rows, lengths): rows
        is CUDA complex64 [len(spans), n_cols] (n_cols None: the longest span) with rows[b, :n_frames] the bits of
        process_bulk's [channel, first_frame : first_frame + n_frames] and +0 behind them -- the layout
        NativeMultiChannelReceiver.submit takes; lengths is the spans' n_frames (numpy, int64).  out: an optional CUDA
        complex64 [len(spans), >= n_cols] tensor with contiguous rows.  The handle's stream is not touched: a later
        process_bulk gives what it would have given.  Any number of spans: 64 go into one launch.  A handle with
        interpolation > 1 is refused."""
        rec = self._spans(spans)
        x, n_in, fmt, scale = _stream_input(x, scale, self._stream)
        if n_cols is None:
            n_cols = int(rec["n_frames"].max()) if rec.size else 0
        n_cols = int(n_cols)
        if n_cols < 0:
            raise Gr4pmError("Ddc.extract: n_cols must not be negative")
        x_index = self.start_index if x_index is None else int(x_index)
        if not 0 <= x_index < 1 << 64:
            raise Gr4pmError("Ddc.extract: x_index must fit 64 unsigned bits")
        out = _rows_output(out, rec.size, n_cols, x.device, "Ddc.extract")
        for lo in range(0, max(rec.size, 1), self.SPANS_PER_CALL):  # no span: one call, which refuses what it refuses
            part = rec[lo:lo + self.SPANS_PER_CALL]
            rows = out[lo:lo + part.size]
            stride = rows.stride(0) if part.size > 1 else max(rows.shape[1], n_cols)
            if fmt is None:
                check(lib().gr4pm_ddc_extract(self._h, x.data_ptr(), n_in, x_index, _np_ptr(part), part.size, rows.data_ptr(),
                                              stride, n_cols), "Ddc.extract")
            else:
                check(lib().gr4pm_ddc_extract_iq(self._h, x.data_ptr(), fmt, scale, n_in, x_index, _np_ptr(part), part.size,
                                                 rows.data_ptr(), stride, n_cols), "Ddc.extract_iq")
        return out[:, :n_cols], rec["n_frames"].astype(np.int64)

    def burst_spans(self, bursts, channel, margin_frames=0):
        """the spans of `channel` that see the bursts Spectrogram.bursts() found: per record the frames from
        max(0, floor((start_sample - start_index) / decimation) - margin_frames), the first whose newest sample is at or
        after start_sample, to ceil((end_sample - start_index + len(taps) - 1) / decimation) + margin_frames, one whose
        oldest sample is at or after end_sample (host only).  Returns a list of (channel, first_frame, n_frames) for
        extract()."""
        if self.interpolation > 1:
            raise Gr4pmError("Ddc.burst_spans: needs a handle with interpolation 1")
        return [(int(channel),) + ddc_burst_span(int(b["start_sample"]), int(b["end_sample"]), self.decimation,
                                                 int(self.taps.size), self.start_index, margin_frames) for b in bursts]

    def __del__(self):
        _destroy(self, "gr4pm_ddc_destroy")


def fft_ddc_taps(decimation, taps_per_phase=12):
    """gr4pm_fft_ddc_taps: the FftDdc's default prototype, ddc_taps(decimation, taps_per_phase) for a power-of-two
    decimation in 4 .. 64 (host only: works without a GPU)."""
    n = int(decimation) * int(taps_per_phase)
    out = np.zeros(max(n, 1), dtype=np.float32)
    check(lib().gr4pm_fft_ddc_taps(int(decimation), int(taps_per_phase), _np_ptr(out)), "fft_ddc_taps")
    return out[:n]


class FftDdc:
    """gr4pm_fft_ddc: the Ddc for many channels and a power-of-two decimation (4 .. 64), as a fast-convolution filter
    bank: one forward 2048-point transform of the wideband stream per segment, shared by all len(frequencies) <= 64
    channels; per channel a product over `images` * 2048 / decimation bins around the channel's nearest bin, a fold and
    an inverse transform of 2048 / decimation points.  Row k is the band centred on frequencies[k]
    on the Ddc's own frame grid; with images = decimation it is the Ddc's result up to float32 rounding, with fewer
    images it differs by the prototype's response outside +-images / (2 decimation) cycles per sample (images = 1 cuts
    inside the default design's transition band).  taps: float32 prototype taps (None: fft_ddc_taps(decimation,
    taps_per_phase)); overlap: a multiple of decimation with len(taps) - 1 <= overlap <= 1984 (None: the smallest
    multiple of 256 that is >= len(taps) - 1); .hop = 2048 - overlap.  process_bulk() takes any number of samples and
    delivers whole segments, hop / decimation frames each; the rest stays on the device, and any cutting of the stream
    into calls gives the same bits.  Frequencies are fixed.  The handle works on the stream that is current when it is
    made."""

    def __init__(self, frequencies, decimation, taps=None, taps_per_phase=12, overlap=None, images=2, start_index=0):
        self.decimation, self.images = int(decimation), int(images)
        f, self.taps, self.start_index = _xlate_settings("FftDdc", frequencies, self.decimation, taps, taps_per_phase,
                                                         start_index, fft_ddc_taps)
        if self.images < 0 or (overlap is not None and not 0 <= int(overlap) < 1 << 62):
            raise Gr4pmError("FftDdc: images and overlap must not be negative")
        self.n_channels = self.n_rows = int(f.size)
        stream = _stream_handle()
        self._stream = stream.value
        self._h = C.c_void_p()
        p = _abi.FftDdcParams(self.n_channels, self.decimation, _np_ptr(f) if f.size else None, _np_ptr(self.taps),
                              self.taps.size, int(taps_per_phase), -1 if overlap is None else int(overlap), self.images,
                              self.start_index, stream)
        check(lib().gr4pm_fft_ddc_create(C.byref(p), C.byref(self._h)), "FftDdc")
        q = np.zeros(self.n_channels, dtype=np.float64)
        check(lib().gr4pm_fft_ddc_frequencies(self._h, _np_ptr(q)), "FftDdc.frequencies")
        self.frequencies = q
        v, hop = C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4pm_fft_ddc_sizes(self._h, C.byref(v), C.byref(hop)), "FftDdc.sizes")
        self.overlap, self.hop = v.value, hop.value

    def frames_for(self, n_in):
        """frames per row the next process_bulk() of n_in samples delivers"""
        n = C.c_size_t(0)
        check(lib().gr4pm_fft_ddc_frames_for(self._h, int(n_in), C.byref(n)), "FftDdc.frames_for")
        return n.value

    def reset(self):
        """back to start_index: zero prehistory, no carried samples"""
        check(lib().gr4pm_fft_ddc_reset(self._h), "FftDdc.reset")

    def process_bulk(self, x, out=None, scale=None):
        """x: a contiguous CUDA complex64 tensor of any length (all of it is consumed), or integer IQ: an int16 (sc16),
        int8 (sc8) or uint8 (cu8) CUDA tensor [n, 2], converted as iq_unpack(x, scale) does where the kernel loads it
        (gr4pm_fft_ddc_process_iq: the same result bit for bit; calls of any format mix on one handle).  Returns
        y[n_channels, frames], the array NativeMultiChannelReceiver.submit() takes; out: an optional CUDA complex64
        [n_channels, >= frames] tensor with contiguous rows and any row stride to write into."""
        x, n_in, fmt, scale = _stream_input(x, scale, self._stream)
        out = _rows_output(out, self.n_channels, self.frames_for(n_in), x.device, "FftDdc")
        n = C.c_size_t(0)
        stride = out.stride(0) if self.n_channels > 1 else out.shape[1]
        if fmt is None:
            check(lib().gr4pm_fft_ddc_process(self._h, x.data_ptr(), n_in, out.data_ptr(), stride, out.shape[1], C.byref(n)),
                  "FftDdc.process")
        else:
            check(lib().gr4pm_fft_ddc_process_iq(self._h, x.data_ptr(), fmt, scale, n_in, out.data_ptr(), stride, out.shape[1],
                                                 C.byref(n)), "FftDdc.process_iq")
        return out[:, : n.value]

    def __del__(self):
        _destroy(self, "gr4pm_fft_ddc_destroy")


def fft_ddc_decimation(bandwidth):
    """the decimation the MixedFftDdc gives a carrier of `bandwidth` cycles per wideband sample (find_carriers' field):
    the largest power of two <= provisional_decimation(bandwidth), at most 64 (host only).  The row then holds the
    carrier at 4 to 8 samples per symbol or more, which RowResampler brings to 4.  Below 4 (a carrier wider than 0.1 of
    the band) raises Gr4pmError: that carrier is the Ddc's."""
    d = provisional_decimation(bandwidth)
    if d < 4:
        raise Gr4pmError(f"fft_ddc_decimation: a bandwidth of {float(bandwidth)} gives a decimation of {d}, below 4")
    return min(64, 1 << (d.bit_length() - 1))


class MixedFftDdc:
    """gr4pm_fft_ddc_mixed: the FftDdc with a decimation per channel: carriers of different symbol rates from one pass
    over the stream and one forward transform per segment.  decimations[k] is a power of two in
    4 .. 64; row k is the band centred on frequencies[k] on the Ddc's frame grid at decimations[k], as
    FftDdc([frequencies[k]], decimations[k]) would give it, and with all decimations equal the block is the FftDdc bit
    for bit.  taps: a list of one float32 prototype per channel (None: fft_ddc_taps(decimations[k], taps_per_phase)
    each); images: an int or one per channel; overlap: one for the handle, a multiple of max(decimations) with
    max(decimations) - decimations[k] + len(taps[k]) - 1 <= overlap <= 1984 for every k (None: the smallest multiple of
    256 that takes all of them); .hop = 2048 - overlap.  process_bulk() takes any number of samples and delivers whole
    segments, hop / decimations[k] frames of row k each; the rest stays on the device, and any cutting of the stream
    into calls gives the same bits.  The handle works on the stream that is current when it is made."""

    def __init__(self, frequencies, decimations, taps=None, taps_per_phase=12, overlap=None, images=2, start_index=0):
        f = np.ascontiguousarray(np.atleast_1d(np.asarray(frequencies, dtype=np.float64)))
        if f.ndim != 1:
            raise Gr4pmError("MixedFftDdc: frequencies must be a list of numbers")
        K = int(f.size)
        dec = [int(d) for d in np.atleast_1d(decimations)]
        img = [int(images)] * K if np.ndim(images) == 0 else [int(r) for r in images]
        if len(dec) != K or len(img) != K or (taps is not None and len(taps) != K):
            raise Gr4pmError(f"MixedFftDdc: {K} frequencies need {K} decimations, {K} images (or one) and {K} prototypes (or None)")
        if min(dec + img + [0]) < 0 or (overlap is not None and not 0 <= int(overlap) < 1 << 62):
            raise Gr4pmError("MixedFftDdc: decimations, images and overlap must not be negative")
        self.start_index = int(start_index)
        if not 0 <= self.start_index < 1 << 64:
            raise Gr4pmError("MixedFftDdc: start_index must fit 64 unsigned bits")
        if taps is not None:
            self.taps = [np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t in taps]
        else:
            self.taps = [fft_ddc_taps(d, taps_per_phase) for d in dec]
        self.decimations, self.images = np.array(dec, dtype=np.int64), np.array(img, dtype=np.int64)
        self.n_channels = self.n_rows = K
        d_arr, r_arr = np.array(dec, dtype=np.uintp), np.array(img, dtype=np.uintp)
        l_arr = np.array([t.size for t in self.taps], dtype=np.uintp)
        all_taps = np.ascontiguousarray(np.concatenate(self.taps + [np.zeros(1, dtype=np.float32)]))
        stream = _stream_handle()
        self._stream = stream.value
        self._h = C.c_void_p()
        p = _abi.FftDdcMixedParams(K, _np_ptr(d_arr), _np_ptr(f) if K else None, _np_ptr(all_taps), _np_ptr(l_arr), int(taps_per_phase),
                                   _np_ptr(r_arr), -1 if overlap is None else int(overlap), self.start_index, stream)
        check(lib().gr4pm_fft_ddc_mixed_create(C.byref(p), C.byref(self._h)), "MixedFftDdc")
        q = np.zeros(K, dtype=np.float64)
        check(lib().gr4pm_fft_ddc_mixed_frequencies(self._h, _np_ptr(q)), "MixedFftDdc.frequencies")
        self.frequencies = q
        v, hop = C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4pm_fft_ddc_mixed_sizes(self._h, C.byref(v), C.byref(hop)), "MixedFftDdc.sizes")
        self.overlap, self.hop = v.value, hop.value

    def frames_for(self, n_in):
        """frames of each row the next process_bulk() of n_in samples delivers (numpy, int64, one per channel)"""
        n = np.zeros(self.n_channels, dtype=np.uintp)
        check(lib().gr4pm_fft_ddc_mixed_frames_for(self._h, int(n_in), _np_ptr(n)), "MixedFftDdc.frames_for")
        return n.astype(np.int64)

    def reset(self):
        """back to start_index: zero prehistory, no carried samples"""
        check(lib().gr4pm_fft_ddc_mixed_reset(self._h), "MixedFftDdc.reset")

    def process_bulk(self, x, out=None, scale=None):
        """x: a contiguous CUDA complex64 tensor of any length (all of it is consumed), or integer IQ [n, 2] as
        FftDdc.process_bulk takes it (the same result bit for bit).  Returns (rows, lengths): rows is CUDA complex64
        [n_channels, max(lengths)] with rows[k, :lengths[k]] the frames of channel k and +0 behind them, the layout of
        Ddc.extract and RowResampler; lengths is numpy int64.  out: an optional CUDA complex64 [n_channels, >=
        max(lengths)] tensor with contiguous rows and any row stride to write into."""
        x, n_in, fmt, scale = _stream_input(x, scale, self._stream)
        longest = int(self.frames_for(n_in).max())
        out = _rows_output(out, self.n_channels, longest, x.device, "MixedFftDdc")
        n = np.zeros(self.n_channels, dtype=np.uintp)
        stride = out.stride(0) if self.n_channels > 1 else out.shape[1]
        if fmt is None:
            check(lib().gr4pm_fft_ddc_mixed_process(self._h, x.data_ptr(), n_in, out.data_ptr(), stride, out.shape[1], _np_ptr(n)),
                  "MixedFftDdc.process")
        else:
            check(lib().gr4pm_fft_ddc_mixed_process_iq(self._h, x.data_ptr(), fmt, scale, n_in, out.data_ptr(), stride, out.shape[1],
                                                       _np_ptr(n)), "MixedFftDdc.process_iq")
        return out[:, :longest], n.astype(np.int64)

    def __del__(self):
        _destroy(self, "gr4pm_fft_ddc_mixed_destroy")


def duc_taps(interpolation, taps_per_phase=12, passband=0.25, stopband=0.75):
    """gr4pm_duc_taps: the Duc's prototype low-pass, the Kaiser design of ddc_taps with taps_per_phase * interpolation
    float32 taps and DC gain `interpolation`, scaled in double before the one rounding to float32 (host only: works
    without a GPU).  passband / stopband: the band edges in units of the input rate."""
    return _design_taps("gr4pm_duc_taps", interpolation, taps_per_phase, passband, stopband, "duc_taps")


def duc_rational_taps(interpolation, decimation, taps_per_phase=12, passband=0.25, stopband=0.75):
    """gr4pm_duc_rational_taps: the prototype low-pass of a Duc that resamples by interpolation / decimation, at the
    rate interpolation * the input rate: the Kaiser design of duc_taps with taps_per_phase * interpolation float32 taps
    and DC gain `interpolation`, scaled in double before the one rounding to float32 (host only: works without a GPU).
    passband / stopband: the band edges in units of the input rate; a cutoff beyond half of the lower of the input and
    the output rate (passband + stopband > min(1, interpolation / decimation)) is refused.  With decimation = 1 the
    floats are those of duc_taps."""
    n = int(interpolation) * int(taps_per_phase)
    out = np.zeros(max(n, 1), dtype=np.float32)
    check(lib().gr4pm_duc_rational_taps(int(interpolation), int(decimation), int(taps_per_phase), float(passband),
                                        float(stopband), _np_ptr(out)), "duc_rational_taps")
    return out[:n]


class Duc:
    """gr4pm_duc: tunable up-converter, the mirror of Ddc.  len(frequencies) complex64 rows at fs / interpolation become
    one wideband stream at fs: row k is interpolated by any integer 1 .. 1024 through the prototype, scaled by gains[k]
    (None: 1) and mixed to frequencies[k] (cycles per output sample, any real value, quantised to fs / 2^32:
    .frequencies holds the values in use, folded to [-0.5, 0.5)); the rows are summed.  taps: 1 .. 8192 float32
    prototype taps of any length (None: duc_taps(interpolation, taps_per_phase)).  start_index: the absolute index of
    the first output sample (a row's phase follows from the absolute index in integer arithmetic, exactly, at any
    stream position), so Ddc(frequencies, interpolation, start_index=...) on the result returns the rows.
    process_bulk() takes any number of items per row; the filter history stays on the device.  Frequencies and gains
    are fixed: make another Duc to retune.  The handle works on the stream that is current when it is made.

    decimation = D > 1 (at most 64) resamples by interpolation / D in the same pass (gr4pm_duc_create_rational): the
    output rate is the rows' rate times interpolation / D (.rate, a Fraction), N items per row make ceil(N
    interpolation / D) samples, and the prototype (None: duc_rational_taps(interpolation, D, taps_per_phase), which
    exists for interpolation >= D only) runs at interpolation times the rows' rate.  Without taps the pair is reduced
    to lowest terms (.interpolation and .decimation hold the reduced values); with taps a pair that is not in lowest
    terms is refused, since the taps belong to one rate.  Ddc(frequencies, interpolation, interpolation=D,
    start_index=...) on the result returns the rows."""

    def __init__(self, frequencies, interpolation, decimation=1, gains=None, taps=None, taps_per_phase=12, start_index=0,
                 max_items=1 << 22):
        self.interpolation, self.decimation = int(interpolation), int(decimation)
        if self.decimation > 1 and self.interpolation >= 1:
            g = math.gcd(self.interpolation, self.decimation)
            if g > 1 and taps is not None:
                raise Gr4pmError(f"Duc: {self.interpolation} / {self.decimation} is not in lowest terms, and the taps "
                                 f"belong to one rate: use {self.interpolation // g} / {self.decimation // g}")
            if g > 1:
                self.interpolation, self.decimation = self.interpolation // g, self.decimation // g
        if self.decimation == 1:
            design = duc_taps
        else:
            design = lambda i, per: duc_rational_taps(i, self.decimation, per)
        f, self.taps, self.start_index = _xlate_settings("Duc", frequencies, self.interpolation, taps, taps_per_phase,
                                                         start_index, design)
        self.rate = fractions.Fraction(self.interpolation, self.decimation) if self.decimation > 0 else None
        self.n_channels = int(f.size)
        a = None
        if gains is not None:
            a = np.ascontiguousarray(np.atleast_1d(np.asarray(gains, dtype=np.float64)))
            if a.shape != f.shape:
                raise Gr4pmError("Duc: one gain per frequency")
        self.gains = np.ones(f.size) if a is None else a
        self.max_items = int(max_items)
        stream = _stream_handle()
        self._stream = stream.value
        args = (self.n_channels, self.interpolation, _np_ptr(f) if f.size else None,
                _np_ptr(a) if a is not None and a.size else None, _np_ptr(self.taps), self.taps.size, self.max_items,
                self.start_index, stream)
        self._h = C.c_void_p()
        if self.decimation == 1:
            p = _abi.DucParams(*args)
            check(lib().gr4pm_duc_create(C.byref(p), C.byref(self._h)), "Duc")
        else:
            p = _abi.DucRationalParams(*args, self.decimation)
            check(lib().gr4pm_duc_create_rational(C.byref(p), C.byref(self._h)), "Duc")
        q = np.zeros(self.n_channels, dtype=np.float64)
        check(lib().gr4pm_duc_frequencies(self._h, _np_ptr(q)), "Duc.frequencies")
        self.frequencies = q

    def output_items(self, n_in):
        """samples the next process_bulk() of n_in items per row produces.  With decimation = 1 that is n_in *
        interpolation; a handle that resamples by interpolation / decimation makes ceil(N interpolation / decimation)
        samples from N items in all, so the count of one call depends on where the handle stands in its stream: ask
        before each call (the state is unchanged by asking)"""
        n = C.c_size_t(0)
        check(lib().gr4pm_duc_output_items(self._h, int(n_in), C.byref(n)), "Duc.output_items")
        return n.value

    def reset(self):
        """back to start_index: zero history"""
        check(lib().gr4pm_duc_reset(self._h), "Duc.reset")

    @property
    def tile_items(self):
        """consecutive output samples that one workgroup of the handle's kernel owns; no result depends on it"""
        n = C.c_size_t(0)
        check(lib().gr4pm_duc_tile_items(self._h, C.byref(n)), "Duc.tile_items")
        return n.value

    def process_bulk(self, v, out=None, format=None, gain=None, clipped=None):
        """v: a CUDA complex64 tensor [n_channels, n] with contiguous rows and any row stride (a window of a wider
        tensor), or a contiguous 1-D tensor when there is one channel.  Returns x[output_items(n)] (n * interpolation
        samples with decimation = 1); out: an optional contiguous CUDA complex64 tensor of at least that many samples to
        write into.
        format "sc16", "sc8" or "cu8" (gr4pm_duc_process_iq): the kernel writes integer IQ itself, and
        the call returns iq_pack(process_bulk(v), format, gain, clipped=clipped) byte for byte, [samples, 2] of iq_pack's
        dtype, without the complex64 band in between; out is then a contiguous tensor [>= samples, 2] of that dtype,
        gain None the format's default, clipped iq_pack's one-element int64 CUDA tensor.  Calls of any format mix on
        one handle."""
        torch = _torch()
        if isinstance(v, torch.Tensor) and self.n_channels == 1 and (v.dim() == 1 or (v.dim() == 2 and v.shape[0] == 1)):
            v = _dev_c64(v.reshape(-1) if v.dim() == 2 else v, "v")  # one row: its stride means nothing
            n_in, stride = v.numel(), v.numel()
        else:
            v = _dev_c64_rows(v, "v")
            if v.shape[0] != self.n_channels:
                raise Gr4pmError(f"Duc: v is {tuple(v.shape)}, the handle has {self.n_channels} rows")
            n_in, stride = v.shape[1], (v.stride(0) if self.n_channels > 1 else v.shape[1])
        if torch.cuda.current_stream(v.device).cuda_stream != self._stream:
            _inputs_ready(v)  # made on another stream than the handle's
        samples = self.output_items(n_in)
        n = C.c_size_t(0)
        if format is not None:
            f, out, counter = _iq_out("Duc", format, samples, out, clipped, v.device)
            check(lib().gr4pm_duc_process_iq(self._h, v.data_ptr(), stride, n_in, out.data_ptr(), f, 0.0 if gain is None else float(gain),
                                             out.shape[0], C.byref(n), counter), "Duc.process_iq")
            return out[: n.value]
        if out is None:
            out = torch.empty(samples, dtype=torch.complex64, device=v.device)
        else:
            out = _dev_c64(out, "out")
            if out.dim() != 1 or out.numel() < samples:
                raise Gr4pmError(f"Duc: out is {tuple(out.shape)}, the call makes [{samples}]")
        check(lib().gr4pm_duc_process(self._h, v.data_ptr(), stride, n_in, out.data_ptr(), out.numel(), C.byref(n)),
              "Duc.process")
        return out[: n.value]

    def __del__(self):
        _destroy(self, "gr4pm_duc_destroy")


def fft_duc_taps(interpolation, taps_per_phase=12):
    """gr4pm_fft_duc_taps: the FftDuc's default prototype, duc_taps(interpolation, taps_per_phase) for a power-of-two
    interpolation in 4 .. 64 (host only: works without a GPU)."""
    n = int(interpolation) * int(taps_per_phase)
    out = np.zeros(max(n, 1), dtype=np.float32)
    check(lib().gr4pm_fft_duc_taps(int(interpolation), int(taps_per_phase), _np_ptr(out)), "fft_duc_taps")
    return out[:n]


class FftDuc:
    """gr4pm_fft_duc: the Duc for many channels and a power-of-two interpolation (4 .. 64), as a fast-convolution
    synthesis bank, the mirror of FftDdc: per channel the Duc's rotator and a forward transform of 2048 / interpolation
    points, a product over `images` * 2048 / interpolation bins around the channel's nearest bin summed into one
    2048-bin spectrum, and one inverse 2048-point transform per segment shared by all len(frequencies) <= 64 channels
    (DESIGN section 27).  Row k is interpolated through the prototype, scaled by gains[k] (None: 1) and centred on
    frequencies[k] (cycles per output sample; .frequencies holds the values in use); with images = interpolation the
    result is the Duc's up to float32 rounding, with fewer images it differs by the prototype's response outside
    +-images / (2 interpolation) cycles per sample.  taps: float32 prototype taps (None: fft_duc_taps(interpolation,
    taps_per_phase)); overlap: a multiple of interpolation with len(taps) - 1 <= overlap <= 1984 (None: the smallest
    multiple of 256 that is >= len(taps) - 1); .hop = 2048 - overlap.  process_bulk() takes any number of items per row
    and delivers whole segments, hop samples for every hop / interpolation items; the rest stays on the device
    (.pending items per row), and any cutting of the rows into calls gives the same bits.  flush() brings out what the
    items so far still owe.  Frequencies and gains are fixed.  The handle works on the stream that is current when it
    is made."""

    def __init__(self, frequencies, interpolation, gains=None, taps=None, taps_per_phase=12, overlap=None, images=2,
                 start_index=0):
        self.interpolation, self.images = int(interpolation), int(images)
        f, self.taps, self.start_index = _xlate_settings("FftDuc", frequencies, self.interpolation, taps, taps_per_phase,
                                                         start_index, fft_duc_taps)
        if self.images < 0 or (overlap is not None and not 0 <= int(overlap) < 1 << 62):
            raise Gr4pmError("FftDuc: images and overlap must not be negative")
        self.n_channels = int(f.size)
        a = None
        if gains is not None:
            a = np.ascontiguousarray(np.atleast_1d(np.asarray(gains, dtype=np.float64)))
            if a.shape != f.shape:
                raise Gr4pmError("FftDuc: one gain per frequency")
        self.gains = np.ones(f.size) if a is None else a
        stream = _stream_handle()
        self._stream = stream.value
        self._h = C.c_void_p()
        p = _abi.FftDucParams(self.n_channels, self.interpolation, _np_ptr(f) if f.size else None,
                              _np_ptr(a) if a is not None and a.size else None, _np_ptr(self.taps), self.taps.size,
                              int(taps_per_phase), -1 if overlap is None else int(overlap), self.images, self.start_index,
                              stream)
        check(lib().gr4pm_fft_duc_create(C.byref(p), C.byref(self._h)), "FftDuc")
        q = np.zeros(self.n_channels, dtype=np.float64)
        check(lib().gr4pm_fft_duc_frequencies(self._h, _np_ptr(q)), "FftDuc.frequencies")
        self.frequencies = q
        v, hop = C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4pm_fft_duc_sizes(self._h, C.byref(v), C.byref(hop)), "FftDuc.sizes")
        self.overlap, self.hop = v.value, hop.value
        self._taken = 0  # items per row since create or reset

    @property
    def pending(self):
        """items per row taken but not yet in a delivered segment"""
        n = C.c_size_t(0)
        check(lib().gr4pm_fft_duc_pending(self._h, C.byref(n)), "FftDuc.pending")
        return n.value

    def output_items(self, n_in):
        """samples the next process_bulk() of n_in items per row delivers: whole segments of .hop samples, so the count
        depends on where the handle stands in its stream (the state is unchanged by asking)"""
        n = C.c_size_t(0)
        check(lib().gr4pm_fft_duc_output_items(self._h, int(n_in), C.byref(n)), "FftDuc.output_items")
        return n.value

    def reset(self):
        """back to start_index: zero prehistory, no carried items"""
        check(lib().gr4pm_fft_duc_reset(self._h), "FftDuc.reset")
        self._taken = 0

    def process_bulk(self, v, out=None, format=None, gain=None, clipped=None):
        """v: a CUDA complex64 tensor [n_channels, n] with contiguous rows and any row stride (a window of a wider
        tensor), or a contiguous 1-D tensor when there is one channel.  Returns x[output_items(n)]; out: an optional
        contiguous CUDA complex64 tensor of at least that many samples to write into.
        format, gain, clipped: as Duc.process_bulk's (gr4pm_fft_duc_process_iq): integer IQ [samples, 2] from the kernel,
        iq_pack's bytes and count."""
        torch = _torch()
        if isinstance(v, torch.Tensor) and self.n_channels == 1 and (v.dim() == 1 or (v.dim() == 2 and v.shape[0] == 1)):
            v = _dev_c64(v.reshape(-1) if v.dim() == 2 else v, "v")  # one row: its stride means nothing
            n_in, stride = v.numel(), v.numel()
        else:
            v = _dev_c64_rows(v, "v")
            if v.shape[0] != self.n_channels:
                raise Gr4pmError(f"FftDuc: v is {tuple(v.shape)}, the handle has {self.n_channels} rows")
            n_in, stride = v.shape[1], (v.stride(0) if self.n_channels > 1 else v.shape[1])
        if torch.cuda.current_stream(v.device).cuda_stream != self._stream:
            _inputs_ready(v)  # made on another stream than the handle's
        samples = self.output_items(n_in)
        n = C.c_size_t(0)
        if format is not None:
            f, out, counter = _iq_out("FftDuc", format, samples, out, clipped, v.device)
            check(lib().gr4pm_fft_duc_process_iq(self._h, v.data_ptr(), stride, n_in, out.data_ptr(), f,
                                                 0.0 if gain is None else float(gain), out.shape[0], C.byref(n), counter),
                  "FftDuc.process_iq")
            self._taken += n_in
            return out[: n.value]
        if out is None:
            out = torch.empty(samples, dtype=torch.complex64, device=v.device)
        else:
            out = _dev_c64(out, "out")
            if out.dim() != 1 or out.numel() < samples:
                raise Gr4pmError(f"FftDuc: out is {tuple(out.shape)}, the call makes [{samples}]")
        check(lib().gr4pm_fft_duc_process(self._h, v.data_ptr(), stride, n_in, out.data_ptr(), out.numel(), C.byref(n)),
              "FftDuc.process")
        self._taken += n_in
        return out[: n.value]

    def flush_items(self):
        """zero items per row that flush() feeds: the fewest after which every sample the items so far influence is out.
        The last of T items reaches the samples up to (T - 1) interpolation + len(taps) - 1, and T' items deliver
        floor(T' interpolation / hop) hop samples."""
        if self._taken == 0:
            return 0
        need = (self._taken - 1) * self.interpolation + self.taps.size
        segments = -(-need // self.hop)
        return max(segments * (self.hop // self.interpolation) - self._taken, 0)

    def flush(self, format=None, gain=None, clipped=None):
        """feeds flush_items() zero items per row and returns the samples that come out: with them every sample
        influenced by the items so far is delivered, the prototype's len(taps) - 1 samples of tail included.  The result
        is bit-equal to process_bulk() of that many zeros, and the stream goes on behind it.  format, gain, clipped:
        process_bulk's."""
        torch = _torch()
        n = self.flush_items()
        return self.process_bulk(torch.zeros((self.n_channels, n), dtype=torch.complex64, device="cuda"), format=format, gain=gain,
                                 clipped=clipped)

    def __del__(self):
        _destroy(self, "gr4pm_fft_duc_destroy")


class MixedFftDuc:
    """gr4pm_fft_duc_mixed: the FftDuc with an interpolation per row: carriers of different symbol rates onto one stream
    from one assembling pass and one inverse transform per segment.  interpolations[k] is a power of
    two in 4 .. 64; row k's item m sits at output sample m * interpolations[k], all rows start at output sample 0, and the
    result is the sum of what FftDuc([frequencies[k]], interpolations[k], gains=[gains[k]]) makes of each row; with all
    interpolations equal the block is the FftDuc bit for bit.  taps: a list of one float32 prototype per row (None:
    fft_duc_taps(interpolations[k], taps_per_phase) each); images: an int or one per row; overlap: one for the handle, a
    multiple of max(interpolations) with len(taps[k]) - 1 <= overlap <= 1984 for every k (None: the smallest multiple of
    256 that takes all of them); .hop = 2048 - overlap.  The handle counts in slots of .slot = max(interpolations) output
    samples: a call of u slots takes u * slot / interpolations[k] items of row k (items_for) and delivers the whole
    segments they complete; the rest stays on the device (.pending slots), and any cutting into calls gives the same
    bits.  flush() brings out what the items so far still owe.  The handle works on the stream that is current when it is
    made."""

    def __init__(self, frequencies, interpolations, gains=None, taps=None, taps_per_phase=12, overlap=None, images=2,
                 start_index=0):
        f = np.ascontiguousarray(np.atleast_1d(np.asarray(frequencies, dtype=np.float64)))
        if f.ndim != 1:
            raise Gr4pmError("MixedFftDuc: frequencies must be a list of numbers")
        K = int(f.size)
        itp = [int(i) for i in np.atleast_1d(interpolations)]
        img = [int(images)] * K if np.ndim(images) == 0 else [int(r) for r in images]
        if len(itp) != K or len(img) != K or (taps is not None and len(taps) != K):
            raise Gr4pmError(f"MixedFftDuc: {K} frequencies need {K} interpolations, {K} images (or one) and {K} prototypes (or None)")
        if min(itp + img + [0]) < 0 or (overlap is not None and not 0 <= int(overlap) < 1 << 62):
            raise Gr4pmError("MixedFftDuc: interpolations, images and overlap must not be negative")
        self.start_index = int(start_index)
        if not 0 <= self.start_index < 1 << 64:
            raise Gr4pmError("MixedFftDuc: start_index must fit 64 unsigned bits")
        a = None
        if gains is not None:
            a = np.ascontiguousarray(np.atleast_1d(np.asarray(gains, dtype=np.float64)))
            if a.shape != f.shape:
                raise Gr4pmError("MixedFftDuc: one gain per frequency")
        self.gains = np.ones(K) if a is None else a
        if taps is not None:
            self.taps = [np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t in taps]
        else:
            self.taps = [fft_duc_taps(i, taps_per_phase) for i in itp]
        self.interpolations, self.images = np.array(itp, dtype=np.int64), np.array(img, dtype=np.int64)
        self.n_channels = self.n_rows = K
        self.slot = max(itp + [0])
        i_arr, r_arr = np.array(itp, dtype=np.uintp), np.array(img, dtype=np.uintp)
        l_arr = np.array([t.size for t in self.taps], dtype=np.uintp)
        all_taps = np.ascontiguousarray(np.concatenate(self.taps + [np.zeros(1, dtype=np.float32)]))
        stream = _stream_handle()
        self._stream = stream.value
        self._h = C.c_void_p()
        p = _abi.FftDucMixedParams(K, _np_ptr(i_arr), _np_ptr(f) if K else None, _np_ptr(a) if a is not None and a.size else None,
                                   _np_ptr(all_taps), _np_ptr(l_arr), int(taps_per_phase), _np_ptr(r_arr),
                                   -1 if overlap is None else int(overlap), self.start_index, stream)
        check(lib().gr4pm_fft_duc_mixed_create(C.byref(p), C.byref(self._h)), "MixedFftDuc")
        q = np.zeros(K, dtype=np.float64)
        check(lib().gr4pm_fft_duc_mixed_frequencies(self._h, _np_ptr(q)), "MixedFftDuc.frequencies")
        self.frequencies = q
        v, hop = C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4pm_fft_duc_mixed_sizes(self._h, C.byref(v), C.byref(hop)), "MixedFftDuc.sizes")
        self.overlap, self.hop = v.value, hop.value
        self._taken = 0  # slots since create or reset

    @property
    def pending(self):
        """slots taken but not yet in a delivered segment"""
        n = C.c_size_t(0)
        check(lib().gr4pm_fft_duc_mixed_pending(self._h, C.byref(n)), "MixedFftDuc.pending")
        return n.value

    def items_for(self, slots):
        """items of each row a process_bulk() of `slots` slots takes (numpy, int64, one per row)"""
        n = np.zeros(self.n_channels, dtype=np.uintp)
        check(lib().gr4pm_fft_duc_mixed_items_for(self._h, int(slots), _np_ptr(n)), "MixedFftDuc.items_for")
        return n.astype(np.int64)

    def output_items(self, slots):
        """samples the next process_bulk() of `slots` slots delivers: whole segments of .hop samples, so the count depends
        on where the handle stands in its stream (the state is unchanged by asking)"""
        n = C.c_size_t(0)
        check(lib().gr4pm_fft_duc_mixed_output_items(self._h, int(slots), C.byref(n)), "MixedFftDuc.output_items")
        return n.value

    def reset(self):
        """back to start_index: zero prehistory, nothing carried"""
        check(lib().gr4pm_fft_duc_mixed_reset(self._h), "MixedFftDuc.reset")
        self._taken = 0

    def process_bulk(self, v, slots=None, out=None, format=None, gain=None, clipped=None):
        """v: a CUDA complex64 tensor [n_channels, n_cols] with contiguous rows and any row stride; row k's first
        items_for(slots)[k] items are used.  slots: None for the most that n_cols covers for every row, n_cols *
        min(interpolations) // slot.  Returns x[output_items(slots)]; out: an optional contiguous CUDA complex64 tensor of
        at least that many samples to write into.
        format, gain, clipped: as Duc.process_bulk's (gr4pm_fft_duc_mixed_process_iq): integer IQ [samples, 2] from the
        kernel, iq_pack's bytes and count."""
        torch = _torch()
        if isinstance(v, torch.Tensor) and self.n_channels == 1 and v.dim() == 1:
            v = v.reshape(1, -1)
        v = _dev_c64_rows(v, "v")
        if v.shape[0] != self.n_channels:
            raise Gr4pmError(f"MixedFftDuc: v is {tuple(v.shape)}, the handle has {self.n_channels} rows")
        most = v.shape[1] * int(self.interpolations.min()) // self.slot
        slots = most if slots is None else int(slots)
        if not 0 <= slots <= most:
            raise Gr4pmError(f"MixedFftDuc: {slots} slots, the {v.shape[1]} columns of v cover {most}")
        stride = v.stride(0) if self.n_channels > 1 else v.shape[1]
        if torch.cuda.current_stream(v.device).cuda_stream != self._stream:
            _inputs_ready(v)  # made on another stream than the handle's
        samples = self.output_items(slots)
        n = C.c_size_t(0)
        if format is not None:
            f, out, counter = _iq_out("MixedFftDuc", format, samples, out, clipped, v.device)
            check(lib().gr4pm_fft_duc_mixed_process_iq(self._h, v.data_ptr(), stride, slots, out.data_ptr(), f,
                                                       0.0 if gain is None else float(gain), out.shape[0], C.byref(n), counter),
                  "MixedFftDuc.process_iq")
            self._taken += slots
            return out[: n.value]
        if out is None:
            out = torch.empty(samples, dtype=torch.complex64, device=v.device)
        else:
            out = _dev_c64(out, "out")
            if out.dim() != 1 or out.numel() < samples:
                raise Gr4pmError(f"MixedFftDuc: out is {tuple(out.shape)}, the call makes [{samples}]")
        check(lib().gr4pm_fft_duc_mixed_process(self._h, v.data_ptr(), stride, slots, out.data_ptr(), out.numel(), C.byref(n)),
              "MixedFftDuc.process")
        self._taken += slots
        return out[: n.value]

    def flush_items(self):
        """zero slots that flush() feeds: the fewest after which every sample the items so far influence is out.  The last
        of row k's T_k = taken * slot / interpolations[k] items reaches the samples up to (T_k - 1) interpolations[k] +
        len(taps[k]) - 1, and T slots deliver floor(T slot / hop) hop samples."""
        if self._taken == 0:
            return 0
        need = max((self._taken * self.slot // int(i) - 1) * int(i) + t.size for i, t in zip(self.interpolations, self.taps))
        segments = -(-need // self.hop)
        return max(segments * (self.hop // self.slot) - self._taken, 0)

    def flush(self, format=None, gain=None, clipped=None):
        """feeds flush_items() zero slots and returns the samples that come out: with them every sample influenced by the
        items so far is delivered, the prototypes' tails included.  The result is bit-equal to process_bulk() of that
        many slots of zeros, and the stream goes on behind it.  format, gain, clipped: process_bulk's."""
        torch = _torch()
        n = self.flush_items()
        cols = n * self.slot // int(self.interpolations.min()) if self.n_channels else 0
        return self.process_bulk(torch.zeros((self.n_channels, cols), dtype=torch.complex64, device="cuda"), slots=n, format=format,
                                 gain=gain, clipped=clipped)

    def pack(self, rows):
        """rows: a list of n_channels one-dimensional CUDA complex64 tensors, bursts of different lengths at the rows' own
        rates.  Returns (v, slots): v is [n_channels, n_cols] with row k the burst and zeros behind it, and `slots` the
        fewest slots that take all of every burst (row k is padded to a whole number of slots); process_bulk(v, slots)
        takes it."""
        torch = _torch()
        if len(rows) != self.n_channels:
            raise Gr4pmError(f"MixedFftDuc: {len(rows)} rows, the handle has {self.n_channels}")
        rows = [_dev_c64(r, "rows") for r in rows]
        if any(r.dim() != 1 for r in rows):
            raise Gr4pmError("MixedFftDuc: pack() takes one-dimensional rows")
        per_slot = [self.slot // int(i) for i in self.interpolations]
        slots = max(-(-r.numel() // p) for r, p in zip(rows, per_slot))
        v = torch.zeros((self.n_channels, slots * max(per_slot)), dtype=torch.complex64, device=rows[0].device)
        for k, r in enumerate(rows):
            v[k, :r.numel()] = r
        return v, slots

    def __del__(self):
        _destroy(self, "gr4pm_fft_duc_mixed_destroy")


def spectrum_window(n):
    """gr4pm_spectrum_window: the periodic Hann window 0.5 - 0.5 cos(2 pi i / n) of the Spectrum block, computed in double
    and rounded to float32 once (host only: works without a GPU)."""
    out = np.zeros(max(int(n), 1), dtype=np.float32)
    check(lib().gr4pm_spectrum_window(int(n), _np_ptr(out)), "spectrum_window")
    return out[: int(n)]


def find_carriers(psd, threshold_db=6.0, max_gap_bins=2, min_width_bins=4, cap=None):
    """gr4pm_find_carriers: the carriers in a power spectrum of n bins in FFT order (host only: works without a GPU).
    floor: the lower median of the bins; a bin is occupied above floor * 10^(threshold_db / 10); runs of occupied bins on
    the circle of n bins, merged across at most max_gap_bins free bins, dropped below min_width_bins.  Returns a structured
    array (frequency: the centroid above the floor in cycles per sample, folded to [-0.5, 0.5); bandwidth; power: the sum
    above the floor; snr_db: peak over floor; first_bin; n_bins) in ascending frequency.  cap: at most so many rows, the
    lowest frequencies (None: all; count_carriers() tells how many there are)."""
    psd = np.ascontiguousarray(psd, dtype=np.float64).reshape(-1)
    p = _abi.CarrierParams(float(threshold_db), int(max_gap_bins), int(min_width_bins))
    n = C.c_size_t(0)
    room = psd.size if cap is None else int(cap)
    out = np.zeros(max(room, 1), dtype=_abi.CARRIER_DTYPE)
    check(lib().gr4pm_find_carriers(_np_ptr(psd), psd.size, C.byref(p), _np_ptr(out), room, C.byref(n)), "find_carriers")
    return out[: min(room, n.value)]


def count_carriers(psd, threshold_db=6.0, max_gap_bins=2, min_width_bins=4):
    """how many carriers find_carriers() finds, whatever its cap (gr4pm_find_carriers with room for none)"""
    psd = np.ascontiguousarray(psd, dtype=np.float64).reshape(-1)
    p = _abi.CarrierParams(float(threshold_db), int(max_gap_bins), int(min_width_bins))
    n = C.c_size_t(0)
    check(lib().gr4pm_find_carriers(_np_ptr(psd), psd.size, C.byref(p), None, 0, C.byref(n)), "find_carriers")
    return n.value


class Spectrum:
    """gr4pm_spectrum: Welch power spectral density of one wideband stream on the device.  Segment s is x[s hop .. s hop +
    2048) of all samples since the handle was made or reset (no zero prehistory); every segment is multiplied by the
    window (2048 float32; None: spectrum_window(2048), periodic Hann), transformed (forward sign, FFT bin order:
    .frequencies holds the bin centres in cycles per sample, folded to [-0.5, 0.5)) and its powers are summed and
    maximised per bin.  process_bulk() takes any number of samples; the samples of the incomplete segment stay on the
    device.  read() gives mean (white noise of power sigma^2 reads sigma^2 in every bin) and max_hold (for bursts: an
    average over a mostly silent recording dilutes them).  The handle works on the stream that is current when it is
    made."""

    fft_size = 2048

    def __init__(self, hop=1024, window=None, fft_size=2048):
        self.hop, self.fft_size = int(hop), int(fft_size)
        if window is not None:
            window = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
            if window.size != self.fft_size:
                raise Gr4pmError(f"Spectrum: a window of {window.size} floats for {self.fft_size} points")
        self.window = window if window is not None else spectrum_window(self.fft_size)
        if not (0 <= self.hop < 1 << 32 and 0 <= self.fft_size < 1 << 32):
            raise Gr4pmError("Spectrum: hop and fft_size must fit 32 unsigned bits")
        k = np.arange(self.fft_size, dtype=np.float64) / max(self.fft_size, 1)
        self.frequencies = k - np.floor(k + 0.5)
        stream = _stream_handle()
        self._stream = stream.value
        p = _abi.SpectrumParams(self.fft_size, self.hop, _np_ptr(self.window) if window is not None else None, stream)
        self._h = C.c_void_p()
        check(lib().gr4pm_spectrum_create(C.byref(p), C.byref(self._h)), "Spectrum")

    def reset(self):
        """back to the fresh stream: no segments, no carried samples"""
        check(lib().gr4pm_spectrum_reset(self._h), "Spectrum.reset")

    def process_bulk(self, x, scale=None):
        """x: a contiguous CUDA complex64 tensor of any length (all of it is consumed), or integer IQ: an int16 (sc16),
        int8 (sc8) or uint8 (cu8) CUDA tensor [n, 2], converted as iq_unpack(x, scale) does where the kernel loads it
        (gr4pm_spectrum_process_iq: the same result bit for bit; calls of any format mix on one handle).  Returns self."""
        x, n_in, fmt, scale = _stream_input(x, scale, self._stream)
        if fmt is None:
            check(lib().gr4pm_spectrum_process(self._h, x.data_ptr(), n_in), "Spectrum.process")
        else:
            check(lib().gr4pm_spectrum_process_iq(self._h, x.data_ptr(), fmt, scale, n_in), "Spectrum.process_iq")
        self._last = x  # the call does not wait: the input lives until the next call or read()
        return self

    def read(self):
        """dict(mean: float64[2048], max_hold: float32[2048], segments); waits for the handle's stream"""
        mean = np.zeros(self.fft_size, dtype=np.float64)
        max_hold = np.zeros(self.fft_size, dtype=np.float32)
        n = C.c_uint64(0)
        check(lib().gr4pm_spectrum_read(self._h, _np_ptr(mean), _np_ptr(max_hold), C.byref(n)), "Spectrum.read")
        self._last = None
        return dict(mean=mean, max_hold=max_hold, segments=n.value)

    def carriers(self, which="max_hold", threshold_db=6.0, max_gap_bins=2, min_width_bins=4):
        """find_carriers() on read()[which] (which: "max_hold" or "mean")"""
        if which not in ("max_hold", "mean"):
            raise Gr4pmError(f"Spectrum.carriers: which is {which!r}, not 'max_hold' or 'mean'")
        return find_carriers(self.read()[which], threshold_db, max_gap_bins, min_width_bins)

    def __del__(self):
        _destroy(self, "gr4pm_spectrum_destroy")


BAND_MODES = {"stop": 0, "pass": 1}


def band_filter_taps(bands, mode="stop", n_taps=1025, attenuation_db=60.0):
    """gr4pm_band_filter_taps: complex64 taps that stop or pass the given bands of a complex stream (host only: works
    without a GPU).  bands: (centre, width) pairs in cycles per sample; a band may wrap across +-0.5, and bands that
    overlap or touch are merged on the circle.  n_taps odd: a Kaiser-windowed design (beta from attenuation_db) that delays
    by (n_taps - 1) / 2 samples, with a transition width of (attenuation_db - 7.95) / (14.36 (n_taps - 1))."""
    if mode not in BAND_MODES:
        raise Gr4pmError(f"band_filter_taps: mode is {mode!r}, not 'stop' or 'pass'")
    b = np.ascontiguousarray(np.asarray(bands, dtype=np.float64).reshape(-1, 2))
    n = int(n_taps)
    if not 0 <= n < 1 << 24:
        raise Gr4pmError("band_filter_taps: n_taps out of range")
    out = np.zeros(max(n, 1), dtype=np.complex64)
    check(lib().gr4pm_band_filter_taps(_np_ptr(b) if b.size else None, b.shape[0], BAND_MODES[mode], n, float(attenuation_db),
                                       _np_ptr(out)), "band_filter_taps")
    return out[:n]


def notch_taps(carriers, widen=1.5, min_width=None, **kw):
    """band_filter_taps() for find_carriers()' records: one band per carrier at its `frequency`, `bandwidth` * widen wide and
    not below min_width (None: the design's transition width, (attenuation_db - 7.95) / (14.36 (n_taps - 1))).  kw:
    band_filter_taps' mode, n_taps, attenuation_db."""
    n_taps, a = int(kw.get("n_taps", 1025)), float(kw.get("attenuation_db", 60.0))
    if min_width is None:
        min_width = (a - 7.95) / (14.36 * max(n_taps - 1, 1))
    carriers = np.atleast_1d(carriers)
    bands = [(float(c["frequency"]), max(float(c["bandwidth"]) * float(widen), float(min_width))) for c in carriers]
    return band_filter_taps(bands, **kw)


class FftFilter:
    """gr4pm_fft_filter: any complex FIR of up to 1985 taps on one wideband stream, by fast convolution on the device
    (DESIGN section 32): out[n] = sum_t taps[t] x[n - t], output sample n beside input sample n, x[i] = 0 before the
    stream.  Segments of 2048 samples that overlap by `overlap` (len(taps) - 1 <= overlap <= 1984; None: len(taps) - 1
    rounded up to a multiple of 256) are transformed, multiplied by the taps' response and transformed back; .hop = 2048 -
    overlap samples of each are kept.  process_bulk() takes any number of samples and delivers whole segments; the rest
    stays on the device (.pending samples), and any cutting of the stream into calls gives the same bits.  flush() brings
    out what is still owed.  The handle works on the stream that is current when it is made."""

    def __init__(self, taps, overlap=None):
        self.taps = self._taps(taps)
        if overlap is not None and not 0 <= int(overlap) < 1 << 62:
            raise Gr4pmError("FftFilter: overlap must not be negative")
        if overlap is not None and int(overlap) == 0 and self.taps.size > 1:
            raise Gr4pmError(f"FftFilter: overlap 0 is below len(taps) - 1 = {self.taps.size - 1}")
        stream = _stream_handle()
        self._stream = stream.value
        self._h = C.c_void_p()
        p = _abi.FftFilterParams(_np_ptr(self.taps) if self.taps.size else None, self.taps.size,
                                 0 if overlap is None else int(overlap), stream)
        check(lib().gr4pm_fft_filter_create(C.byref(p), C.byref(self._h)), "FftFilter")
        v, hop, n = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4pm_fft_filter_sizes(self._h, C.byref(v), C.byref(hop), C.byref(n)), "FftFilter.sizes")
        self.overlap, self.hop = v.value, hop.value

    @staticmethod
    def _taps(taps):
        return np.ascontiguousarray(np.asarray(taps, dtype=np.complex64).reshape(-1))

    @property
    def pending(self):
        """samples taken whose outputs are still owed"""
        n = C.c_size_t(0)
        check(lib().gr4pm_fft_filter_pending(self._h, C.byref(n)), "FftFilter.pending")
        return n.value

    def output_items(self, n):
        """samples the next process_bulk() of n samples delivers: whole segments of .hop samples, so the count depends on
        where the handle stands in its stream (the state is unchanged by asking)"""
        out = C.c_size_t(0)
        check(lib().gr4pm_fft_filter_output_items(self._h, int(n), C.byref(out)), "FftFilter.output_items")
        return out.value

    def reset(self):
        """back to the fresh stream: zero prehistory, nothing pending"""
        check(lib().gr4pm_fft_filter_reset(self._h), "FftFilter.reset")

    def set_taps(self, taps):
        """other taps from the next segment delivered on (len(taps) - 1 <= .overlap); the carried samples stay"""
        taps = self._taps(taps)
        check(lib().gr4pm_fft_filter_set_taps(self._h, _np_ptr(taps) if taps.size else None, taps.size), "FftFilter.set_taps")
        self.taps = taps

    def _out(self, out, samples, device):
        torch = _torch()
        if out is None:
            return torch.empty(samples, dtype=torch.complex64, device=device)
        out = _dev_c64(out, "out")
        if out.dim() != 1:
            raise TypeError("out must be one-dimensional")
        return out

    def process_bulk(self, x, scale=None, out=None):
        """x: a contiguous CUDA complex64 tensor of any length, or integer IQ: an int16 (sc16), int8 (sc8) or uint8 (cu8)
        CUDA tensor [n, 2], converted as iq_unpack(x, scale) does where the kernel loads it (the same result bit for bit;
        calls of any format mix on one handle).  Returns the output_items(n) filtered samples, complex64; out: an optional
        contiguous CUDA complex64 tensor with room for them to write into."""
        x, n_in, fmt, scale = _stream_input(x, scale, self._stream)
        out = self._out(out, self.output_items(n_in), x.device)
        n = C.c_size_t(0)
        if fmt is None:
            check(lib().gr4pm_fft_filter_process(self._h, x.data_ptr(), n_in, out.data_ptr(), out.numel(), C.byref(n)),
                  "FftFilter.process")
        else:
            check(lib().gr4pm_fft_filter_process_iq(self._h, x.data_ptr(), fmt, scale, n_in, out.data_ptr(), out.numel(),
                                                    C.byref(n)), "FftFilter.process_iq")
        self._last = x  # the call does not wait: the input lives until the next call
        return out[: n.value]

    def flush(self, out=None):
        """the .pending samples still owed (the last segment run over zeros); leaves the handle as reset() does, so the
        samples out equal the samples in"""
        out = self._out(out, self.pending, "cuda")
        n = C.c_size_t(0)
        check(lib().gr4pm_fft_filter_flush(self._h, out.data_ptr(), out.numel(), C.byref(n)), "FftFilter.flush")
        return out[: n.value]

    def __del__(self):
        _destroy(self, "gr4pm_fft_filter_destroy")


def find_bursts(power, threshold_db=6.0, max_gap_rows=1, min_rows=2, floor=None, cap=None):
    """gr4pm_find_bursts: the bursts in a band's power over time, rows in time order (host only: works without a GPU).
    floor: the noise level of a row (None: the lower median of the rows, which holds while the band is silent in more
    than half of them); a row is active above floor * 10^(threshold_db / 10); runs of active rows, merged across at most
    max_gap_rows inactive rows, dropped below min_rows.  Returns a structured array (first_row, n_rows, peak_row; power:
    the mean above the floor; snr_db: peak over floor) in ascending time.  cap: at most so many (None: all)."""
    power = np.ascontiguousarray(power, dtype=np.float64).reshape(-1)
    p = _abi.BurstParams(float(threshold_db), 0.0 if floor is None else float(floor), int(max_gap_rows), int(min_rows))
    n = C.c_size_t(0)
    room = power.size if cap is None else int(cap)
    out = np.zeros(max(room, 1), dtype=_abi.BURST_DTYPE)
    check(lib().gr4pm_find_bursts(_np_ptr(power), power.size, C.byref(p), _np_ptr(out), room, C.byref(n)), "find_bursts")
    return out[: min(room, n.value)]


class Spectrogram:
    """gr4pm_spectrogram: PSD rows over time of one wideband stream on the device.  The segments are the Spectrum's
    (segment s is x[s hop .. s hop + 2048) of all samples since the handle was made or reset, windowed and transformed);
    row t is the mean (detector "mean") or the maximum ("max") per bin of the powers of the `average` = R segments
    t R .. t R + R - 1, divided by the window's power, so white noise of power sigma^2 reads sigma^2 in every bin of a
    mean row.  Row t covers the samples [t row_advance, t row_advance + row_span).  process_bulk() takes any number of
    samples and returns the rows they complete; the samples of the incomplete segment and the sums of the incomplete row
    stay on the device, and the rows do not depend on how the stream is cut into calls, bit for bit.  The handle works
    on the stream that is current when it is made."""

    fft_size = 2048

    def __init__(self, hop=1024, average=1, detector="mean", window=None, fft_size=2048):
        self.hop, self.average, self.fft_size = int(hop), int(average), int(fft_size)
        if detector not in _abi.SPECTROGRAM_DETECTORS:
            raise Gr4pmError(f"Spectrogram: detector is {detector!r}, not 'mean' or 'max'")
        self.detector = detector
        if window is not None:
            window = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
            if window.size != self.fft_size:
                raise Gr4pmError(f"Spectrogram: a window of {window.size} floats for {self.fft_size} points")
        self.window = window if window is not None else spectrum_window(self.fft_size)
        if not all(0 <= v < 1 << 32 for v in (self.hop, self.average, self.fft_size)):
            raise Gr4pmError("Spectrogram: hop, average and fft_size must fit 32 unsigned bits")
        k = np.arange(self.fft_size, dtype=np.float64) / max(self.fft_size, 1)
        self.frequencies = k - np.floor(k + 0.5)
        self.row_advance = self.average * self.hop
        self.row_span = (self.average - 1) * self.hop + self.fft_size
        self.rows_done = 0
        stream = _stream_handle()
        self._stream = stream.value
        p = _abi.SpectrogramParams(self.fft_size, self.hop, self.average, _abi.SPECTROGRAM_DETECTORS[detector],
                                   _np_ptr(self.window) if window is not None else None, stream)
        self._h = C.c_void_p()
        check(lib().gr4pm_spectrogram_create(C.byref(p), C.byref(self._h)), "Spectrogram")

    def reset(self):
        """back to the fresh stream: no segments, no carried samples, no carried row"""
        check(lib().gr4pm_spectrogram_reset(self._h), "Spectrogram.reset")
        self.rows_done = 0

    def rows(self, n):
        """gr4pm_spectrogram_rows: the rows a call of n samples would complete now"""
        r = C.c_size_t(0)
        check(lib().gr4pm_spectrogram_rows(self._h, int(n), C.byref(r)), "Spectrogram.rows")
        return r.value

    def process_bulk(self, x, scale=None):
        """x: a contiguous CUDA complex64 tensor of any length (all of it is consumed), or integer IQ: an int16 (sc16),
        int8 (sc8) or uint8 (cu8) CUDA tensor [n, 2], converted as iq_unpack(x, scale) does where the kernel loads it
        (the same rows bit for bit; calls of any format mix on one handle).  Returns the rows the call completes, a CUDA
        float32 tensor [rows, 2048] in FFT bin order (zero rows for a call that completes none).  Does not wait."""
        torch = _torch()
        x, n_in, fmt, scale = _stream_input(x, scale, self._stream)
        want = self.rows(n_in)
        out = torch.empty((want, self.fft_size), dtype=torch.float32, device=x.device)
        got = C.c_size_t(0)
        if fmt is None:
            check(lib().gr4pm_spectrogram_process(self._h, x.data_ptr(), n_in, out.data_ptr(), want, C.byref(got)),
                  "Spectrogram.process")
        else:
            check(lib().gr4pm_spectrogram_process_iq(self._h, x.data_ptr(), fmt, scale, n_in, out.data_ptr(), want, C.byref(got)),
                  "Spectrogram.process_iq")
        if got.value != want:
            raise Gr4pmError(f"Spectrogram: the call made {got.value} rows, gr4pm_spectrogram_rows said {want}")
        self._last = x  # the call does not wait: the input lives until the next call
        self.rows_done += want
        return out

    def band_power(self, rows, bands):
        """gr4pm_spectrogram_band_power: rows: a CUDA float32 tensor [n, 2048] (process_bulk's, or several of them
        joined); bands: find_carriers' structured array (its first_bin and n_bins) or a list of (first_bin, n_bins), at
        most 64, the bins first_bin .. first_bin + n_bins - 1 mod 2048.  Returns a CUDA float64 tensor [K, n]: the sum of
        each band's bins of each row, added in double in a fixed order (the same call gives the same bits)."""
        torch = _torch()
        if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2
                and rows.shape[1] == self.fft_size and rows.is_contiguous()):
            raise TypeError(f"rows must be a contiguous CUDA float32 tensor [n, {self.fft_size}]")
        if isinstance(bands, np.ndarray) and bands.dtype.names and {"first_bin", "n_bins"} <= set(bands.dtype.names):
            pairs = [(int(b["first_bin"]), int(b["n_bins"])) for b in bands.reshape(-1)]
        else:
            pairs = [(int(a), int(b)) for a, b in bands]
        if not all(0 <= a < 1 << 32 and 0 <= b < 1 << 32 for a, b in pairs):
            raise Gr4pmError("Spectrogram.band_power: first_bin and n_bins must fit 32 unsigned bits")
        b = np.array(pairs, dtype=_abi.BAND_DTYPE).reshape(-1)
        if torch.cuda.current_stream(rows.device).cuda_stream != self._stream:
            _inputs_ready(rows)
        out = torch.empty((len(pairs), rows.shape[0]), dtype=torch.float64, device=rows.device)
        check(lib().gr4pm_spectrogram_band_power(self._h, rows.data_ptr(), rows.shape[0], _np_ptr(b) if len(pairs) else None,
                                                 len(pairs), out.data_ptr()), "Spectrogram.band_power")
        return out

    def bursts(self, power_row, first_row=0, **kw):
        """find_bursts(power_row, **kw) for one row of band_power() (a tensor or an array; row 0 of it is the stream's row
        first_row), with the samples each burst covers: a structured array of find_bursts' fields plus start_sample =
        (first_row + burst first_row) row_advance and end_sample = (first_row + burst first_row + n_rows - 1)
        row_advance + row_span (exclusive)."""
        if hasattr(power_row, "cpu"):
            power_row = power_row.cpu().numpy()
        found = find_bursts(power_row, **kw)
        out = np.zeros(len(found), dtype=np.dtype(_abi.BURST_DTYPE.descr + [("start_sample", "<u8"), ("end_sample", "<u8")]))
        for f in _abi.BURST_DTYPE.names:
            out[f] = found[f]
        first = int(first_row) + found["first_row"].astype(np.uint64)
        out["start_sample"] = first * np.uint64(self.row_advance)
        out["end_sample"] = (first + found["n_rows"] - np.uint64(1)) * np.uint64(self.row_advance) + np.uint64(self.row_span)
        return out

    def __del__(self):
        _destroy(self, "gr4pm_spectrogram_destroy")


def find_line(spectrum, first_bin=0, n_bins=None, guard_bins=2):
    """gr4pm_find_line: the line of a spectrum of n bins in FFT order (host only: works without a GPU).  The search
    window is the n_bins bins (first_bin + i) mod n (None: all n), 2 guard_bins + 3 <= n_bins <= n.  Returns one record
    of LINE_DTYPE: bin (the first maximum in window order), peak, floor (the window's lower median), snr_db = 10 log10(peak
    / floor), margin_db = 10 log10(peak / the largest window bin farther than guard_bins from the peak on the circle):
    the confidence measure, near 0 dB for noise whatever the number of segments; frequency = (bin + d) / n folded to
    [-0.5, 0.5), d from the parabola through the logarithms of the peak and its two circular neighbours, clamped to
    +-0.5 (0 when one of them is <= 0 or the curvature is not negative); found = peak > 0."""
    spectrum = np.ascontiguousarray(spectrum, dtype=np.float64).reshape(-1)
    n_bins = spectrum.size if n_bins is None else int(n_bins)
    first_bin, guard_bins = int(first_bin), int(guard_bins)
    if not all(0 <= v < 1 << 64 for v in (first_bin, n_bins, guard_bins)):
        raise Gr4pmError("find_line: first_bin, n_bins and guard_bins must fit 64 unsigned bits")
    p = _abi.LineParams(first_bin, n_bins, guard_bins)
    out = np.zeros(1, dtype=_abi.LINE_DTYPE)
    check(lib().gr4pm_find_line(_np_ptr(spectrum), spectrum.size, C.byref(p), _np_ptr(out)), "find_line")
    return out[0]


def simplest_ratio(value, rel_tol, max_num, max_den):
    """gr4pm_simplest_ratio: (num, den), the fraction with the smallest denominator (of several: the smallest numerator)
    inside [value (1 - rel_tol), value (1 + rel_tol)] with num <= max_num and den <= max_den, in lowest terms (host
    only).  Gr4pmError when there is none or the arguments are not finite and positive."""
    max_num, max_den = int(max_num), int(max_den)
    if not (0 <= max_num < 1 << 32 and 0 <= max_den < 1 << 32):
        raise Gr4pmError("simplest_ratio: max_num and max_den must fit 32 unsigned bits")
    num, den = C.c_uint32(0), C.c_uint32(0)
    check(lib().gr4pm_simplest_ratio(float(value), float(rel_tol), max_num, max_den, C.byref(num), C.byref(den)),
          "simplest_ratio")
    return num.value, den.value


def resample_ratio(symbols_per_wide_sample, samples_per_symbol=4, rel_tol=2e-3, max_interpolation=64, max_decimation=1024):
    """(I, D) for Ddc(frequencies, D, interpolation=I): the simplest I / D within rel_tol of samples_per_symbol *
    symbols_per_wide_sample, so that the rows have samples_per_symbol items per symbol.  A rate rho symbols per item
    measured on the rows of a handle with ratio I0 / D0 (LineSpectrum.symbol_rate) is rho I0 / D0 symbols per wideband
    sample.  rel_tol: the rate estimate is good to 2e-4 with at least three segments at high SNR;
    2e-3 leaves a factor of ten, and around 4 / 25 no simpler fraction lies inside it."""
    return simplest_ratio(float(samples_per_symbol) * float(symbols_per_wide_sample), rel_tol, max_interpolation, max_decimation)


def provisional_decimation(bandwidth):
    """max(1, floor(0.4 / bandwidth)): the decimation at which a carrier of `bandwidth` cycles per wideband sample
    (find_carriers' field) is looked at before its symbol rate is known.  It then occupies at most +-0.2 of the row rate:
    inside the default taps' 0.25 passband, band edges included, which the envelope line needs, and its symbol rate stays
    below 0.5 cycles per item."""
    bandwidth = float(bandwidth)
    if not (bandwidth > 0.0 and math.isfinite(bandwidth)):
        raise Gr4pmError(f"provisional_decimation: bandwidth is {bandwidth}, need a positive number")
    return max(1, int(math.floor(0.4 / bandwidth)))


class LineSpectrum:
    """gr4pm_line_spectrum: per row of channel items (Ddc.process_bulk's or Ddc.extract's [rows, n]) the Welch spectrum
    of a memoryless nonlinearity, whose spectral line gives what a blind receiver lacks: "fourth" ((g x)^4: a line at
    four times the residual carrier offset of a QPSK burst), "square" ((g x)^2: twice the offset, BPSK) and "envelope"
    (|g x|^2: a line at the symbol rate).  Row r has lengths[r] items; behind them the row counts as zero and is never
    read.  Segment s is y[s hop .. s hop + 2048), the last one zero-filled, so a short burst still has one;
    out[r] = sum_s |FFT(w y_s)|^2 / (S_r sum w^2) in FFT bin order (.frequencies: the bin centres in cycles per item), a
    CUDA float64 tensor.  A row's result depends on that row alone, bit for bit.  The handle works on the stream that is
    current when it is made.

    Frequency bookkeeping: a row offset of delta cycles per item of a handle with ratio I / D (Ddc(f, D,
    interpolation=I)) is delta I / D cycles per wideband sample, to be ADDED to that channel's frequency; a rate of rho
    symbols per item is rho I / D symbols per wideband sample (resample_ratio takes that)."""

    fft_size = 2048
    ROWS_PER_CALL = 64

    def __init__(self, hop=1024, window=None, fft_size=2048):
        self.hop, self.fft_size = int(hop), int(fft_size)
        if window is not None:
            window = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
            if window.size != self.fft_size:
                raise Gr4pmError(f"LineSpectrum: a window of {window.size} floats for {self.fft_size} points")
        self.window = window if window is not None else spectrum_window(self.fft_size)
        if not (0 <= self.hop < 1 << 32 and 0 <= self.fft_size < 1 << 32):
            raise Gr4pmError("LineSpectrum: hop and fft_size must fit 32 unsigned bits")
        k = np.arange(self.fft_size, dtype=np.float64) / max(self.fft_size, 1)
        self.frequencies = k - np.floor(k + 0.5)
        stream = _stream_handle()
        self._stream = stream.value
        p = _abi.LineSpectrumParams(self.fft_size, self.hop, _np_ptr(self.window) if window is not None else None, stream)
        self._h = C.c_void_p()
        check(lib().gr4pm_line_spectrum_create(C.byref(p), C.byref(self._h)), "LineSpectrum")

    def _lengths(self, x, lengths):
        if lengths is None:
            return np.full(x.shape[0], x.shape[1], dtype=np.uint64)
        lengths = np.asarray(lengths).reshape(-1)
        if lengths.size != x.shape[0]:
            raise Gr4pmError(f"LineSpectrum: {lengths.size} lengths for {x.shape[0]} rows")
        if lengths.size and (int(lengths.min()) < 0 or int(lengths.max()) >= 1 << 64):
            raise Gr4pmError("LineSpectrum: lengths must fit 64 unsigned bits")
        return np.ascontiguousarray(lengths.astype(np.uint64))

    def process_rows(self, x, lengths=None, statistic="fourth", normalize=True):
        """gr4pm_line_spectrum_process: x: a CUDA complex64 tensor [R, n] with contiguous rows (any row stride >= n);
        lengths: R item counts <= n (None: n each).  statistic: "fourth", "square" or "envelope".  normalize: the row's
        gain is 1 / sqrt(mean |x|^2 over the row's length), computed with torch on the device without a readback (False:
        1; the fourth power leaves float32's range for |x| outside about 1e-4 .. 1e4).  Any number of rows: 64 go into
        one call.  Returns a CUDA float64 tensor [R, 2048]; does not wait."""
        torch = _torch()
        if statistic not in _abi.LINE_STATISTICS:
            raise Gr4pmError(f"LineSpectrum: statistic is {statistic!r}, not 'envelope', 'square' or 'fourth'")
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.complex64 and x.dim() == 2 and
                (x.shape[1] <= 1 or x.stride(1) == 1) and (x.shape[0] <= 1 or x.stride(0) >= x.shape[1])):
            raise TypeError("x must be a [rows, n] complex64 CUDA tensor with contiguous rows")
        n_rows, n_cols = x.shape
        lengths = self._lengths(x, lengths)
        if lengths.size and int(lengths.max()) > n_cols:
            raise Gr4pmError(f"LineSpectrum: a length of {int(lengths.max())} items, the rows have {n_cols}")
        if torch.cuda.current_stream(x.device).cuda_stream != self._stream:
            _inputs_ready(x)  # made on another stream than the handle's
        gains = None
        if normalize and n_rows and n_cols:
            ln = torch.as_tensor(lengths.astype(np.int64), device=x.device)
            live = torch.arange(n_cols, device=x.device)[None, :] < ln[:, None]
            xr = torch.view_as_real(x)
            power = torch.where(live, xr[..., 0] * xr[..., 0] + xr[..., 1] * xr[..., 1], 0.0).sum(dim=1, dtype=torch.float64)
            mean = power / ln.clamp(min=1).to(torch.float64)
            gains = torch.where(mean > 0, mean.rsqrt(), 1.0).to(torch.float32).contiguous()
            if torch.cuda.current_stream(x.device).cuda_stream != self._stream:
                _inputs_ready(gains)
        out = torch.empty((n_rows, self.fft_size), dtype=torch.float64, device=x.device)
        stat = _abi.LINE_STATISTICS[statistic]
        for lo in range(0, n_rows, self.ROWS_PER_CALL):
            rows, part = x[lo:lo + self.ROWS_PER_CALL], lengths[lo:lo + self.ROWS_PER_CALL]
            stride = rows.stride(0) if rows.shape[0] > 1 else max(n_cols, 1)
            check(lib().gr4pm_line_spectrum_process(
                self._h, rows.data_ptr(), stride, n_cols, _np_ptr(part), part.size,
                gains[lo:lo + self.ROWS_PER_CALL].data_ptr() if gains is not None else None, stat,
                out[lo:lo + self.ROWS_PER_CALL].data_ptr()), "LineSpectrum.process_rows")
        self._last = (x, gains)  # the calls do not wait: the inputs live until the next call
        return out

    def _lines(self, spectra, first_bin, n_bins, scale, field):
        spectra = spectra.cpu().numpy()
        out = np.zeros(spectra.shape[0], dtype=np.dtype([(field, "<f8"), ("snr_db", "<f8"), ("margin_db", "<f8")]))
        for r, row in enumerate(spectra):
            line = find_line(row, first_bin, n_bins)
            out[r] = (line["frequency"] * scale, line["snr_db"], line["margin_db"])
        return out

    def carrier_offset(self, x, lengths=None, order=4, max_offset=0.1):
        """the residual carrier offset of every row: the line of the "fourth" (order 4: QPSK) or "square" (order 2:
        BPSK) spectrum inside |order f| <= order max_offset, divided by `order`.  max_offset < 0.5 / order: beyond it
        the line aliases.  Returns a structured array per row: offset (cycles per item; with a handle of ratio I / D add
        offset I / D to the channel's frequency), snr_db, margin_db (find_line's; trust a row with margin_db >= 6).
        Waits for the result."""
        if order not in (2, 4):
            raise Gr4pmError(f"LineSpectrum.carrier_offset: order is {order!r}, not 2 or 4")
        if not 0.0 < float(max_offset) < 0.5 / order:
            raise Gr4pmError(f"LineSpectrum.carrier_offset: max_offset is {max_offset}, need 0 < max_offset < {0.5 / order}")
        half = min(int(math.floor(order * float(max_offset) * self.fft_size)), self.fft_size // 2 - 1)
        half = max(half, 3)
        spectra = self.process_rows(x, lengths, "fourth" if order == 4 else "square")
        return self._lines(spectra, (self.fft_size - half) % self.fft_size, 2 * half + 1, 1.0 / order, "offset")

    def symbol_rate(self, x, lengths=None, min_rate=0.05, max_rate=0.45):
        """the symbol rate of every row: the line of the "envelope" spectrum inside [min_rate, max_rate] cycles per item
        (0 < min_rate < max_rate < 0.5; the spectrum is symmetric, the positive half is searched).  Returns a structured
        array per row: rate (symbols per item; with a handle of ratio I / D that is rate I / D symbols per wideband
        sample), snr_db, margin_db.  Waits for the result."""
        min_rate, max_rate = float(min_rate), float(max_rate)
        if not 0.0 < min_rate < max_rate < 0.5:
            raise Gr4pmError(f"LineSpectrum.symbol_rate: need 0 < min_rate < max_rate < 0.5, not {min_rate}, {max_rate}")
        first = int(math.ceil(min_rate * self.fft_size))
        last = int(math.floor(max_rate * self.fft_size))
        if last - first + 1 < 7:
            raise Gr4pmError("LineSpectrum.symbol_rate: the range holds fewer than 7 bins")
        spectra = self.process_rows(x, lengths, "envelope")
        return self._lines(spectra, first, last - first + 1, 1.0, "rate")

    def __del__(self):
        _destroy(self, "gr4pm_line_spectrum_destroy")


def row_resampler_taps(phases=32, taps_per_phase=12, max_step=1.0, passband=0.25, stopband=0.75):
    """gr4pm_row_resampler_taps: the RowResampler's prototype at the virtual rate `phases` per input item, the Kaiser
    design of ddc_taps with DC gain `phases` (host only: works without a GPU).  passband / stopband: the band edges in
    units of the lower of the input rate and the output rate at max_step input items per output item: they are divided
    by max(1, max_step), and there are ceil(taps_per_phase * max(1, max_step)) taps per phase, so a decimating handle
    keeps the design's span in output items.  Returns phases * that many float32 taps."""
    phases, per, max_step = int(phases), int(taps_per_phase), float(max_step)
    if not (0 <= phases < 1 << 32 and 0 <= per < 1 << 32):
        raise Gr4pmError("row_resampler_taps: phases and taps_per_phase must fit 32 unsigned bits")
    span = int(math.ceil(per * max(1.0, max_step))) if math.isfinite(max_step) else 0
    n = phases * span
    out = np.zeros(n if 0 < n <= 4096 else 1, dtype=np.float32)  # beyond 4096 taps the design is refused before it writes
    check(lib().gr4pm_row_resampler_taps(phases, per, max_step, float(passband), float(stopband), _np_ptr(out)),
          "row_resampler_taps")
    return out[:n]


def _check_rows_input(x, n_rows=None):
    """x is a [rows, n] complex64 CUDA tensor with contiguous rows (any row stride >= n), of n_rows rows where given"""
    torch = _torch()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.complex64 and x.dim() == 2 and
            (n_rows is None or x.shape[0] == n_rows) and (x.shape[1] <= 1 or x.stride(1) == 1) and
            (x.shape[0] <= 1 or x.stride(0) >= x.shape[1])):
        raise TypeError(f"x must be a [{'rows' if n_rows is None else n_rows}, n] complex64 CUDA tensor with contiguous rows")


def _row_freq_word(offset):
    """round(offset 2^32) in Python integers: the frequency word of an offset in cycles per item"""
    return int(round(fractions.Fraction(float(offset)) * (1 << 32)))


class RowResampler:
    """gr4pm_row_resampler: rows of channel items (Ddc.extract's [rows, n]) to any real rate with the residual carrier
    removed, every row with a step and a frequency word of its own: what acts on LineSpectrum's per-row symbol rate and
    carrier offset on the rows themselves, so the wideband recording is read once.  phases: Q, a power of two 2 .. 256;
    taps: Q * P float32 prototype taps at the virtual rate Q per input item (None: row_resampler_taps(phases,
    taps_per_phase, max_step)); Q * P <= 4096.  Output item m of row r sits at pos = phase0 + m * step input items (Q32.32
    integers, exact), takes the P input items up to floor(pos) through coefficients interpolated linearly between the
    two nearest of the Q phases, and is then turned by exp(-2 pi j floor(freq * pos / 2^32) / 2^32): the mix comes after
    the filter, so the block is for residual offsets well inside the prototype's passband.  A row's result depends on
    that row alone, bit for bit, and not on where a call begins in it.  .delay_items: a tone appears (Q P - 1) / (2 Q)
    input items late.  The handle is made on first use, on the stream that is current then; output_lengths, delay_items
    and tile_items work without a GPU."""

    ROWS_PER_CALL = 64
    COLUMN_GRAIN = 2048

    def __init__(self, phases=32, taps_per_phase=12, taps=None, max_step=1.0):
        self.phases = int(phases)
        if taps is None:
            taps = row_resampler_taps(self.phases, taps_per_phase, max_step)
        self.taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        if not (2 <= self.phases <= 256 and self.phases & (self.phases - 1) == 0):
            raise Gr4pmError(f"RowResampler: {self.phases} phases, need a power of two in [2, 256]")
        if not self.taps.size or self.taps.size % self.phases or self.taps.size > 4096:
            raise Gr4pmError(f"RowResampler: {self.taps.size} taps for {self.phases} phases: need a multiple of the phases, "
                             "1 .. 4096 in all")
        if not np.all(np.isfinite(self.taps)):
            raise Gr4pmError("RowResampler: a tap is not finite")
        self.taps_per_phase = self.taps.size // self.phases
        self.delay_items = fractions.Fraction(self.taps.size - 1, 2 * self.phases)
        self._h = None
        self._stream = None

    def _handle(self):
        if not self._h:
            stream = _stream_handle()
            self._stream = stream.value
            p = _abi.RowResamplerParams(self.phases, self.taps_per_phase, _np_ptr(self.taps), stream)
            h = C.c_void_p()
            check(lib().gr4pm_row_resampler_create(C.byref(p), C.byref(h)), "RowResampler")
            self._h = h
        return self._h

    def _records(self, n_rows, steps, phase0, freqs):
        def column(values, what, lo, hi, default):
            if values is None:
                values = [default] * n_rows
            values = [int(v) for v in (values.tolist() if isinstance(values, np.ndarray) else values)]
            if len(values) != n_rows:
                raise Gr4pmError(f"RowResampler: {len(values)} {what} for {n_rows} rows")
            if any(not lo <= v < hi for v in values):
                raise Gr4pmError(f"RowResampler: {what} must lie in [{lo}, {hi})")
            return values
        rec = np.zeros(n_rows, dtype=_abi.ROW_RECORD_DTYPE)
        rec["step"] = np.array(column(steps, "steps", 0, 1 << 64, 1 << 32), dtype=np.uint64)
        rec["phase0"] = np.array(column(phase0, "phase0", 0, 1 << 64, 0), dtype=np.uint64)
        rec["freq"] = np.array(column(freqs, "freqs", -(1 << 31), 1 << 31, 0), dtype=np.int32)
        return rec

    @staticmethod
    def _row_lengths(n_rows, n_cols, lengths):
        if lengths is None:
            return np.full(n_rows, n_cols, dtype=np.uint64)
        lengths = np.asarray(lengths).reshape(-1)
        if lengths.size != n_rows:
            raise Gr4pmError(f"RowResampler: {lengths.size} lengths for {n_rows} rows")
        if lengths.size and (int(lengths.min()) < 0 or int(lengths.max()) >= 1 << 64):
            raise Gr4pmError("RowResampler: lengths must fit 64 unsigned bits")
        return np.ascontiguousarray(lengths.astype(np.uint64))

    def output_lengths(self, lengths, steps, phase0=None, n_cols=None):
        """M_r per row (numpy int64; host only): the output items m whose newest input item floor(phase0 + m step) is at
        most lengths[r] + P - 2, so the filter runs out over the row's end; cut at n_cols where given."""
        lengths = self._row_lengths(len(lengths), 1 << 63, lengths)
        rec = self._records(lengths.size, steps, phase0, None)
        out = np.zeros(lengths.size, dtype=np.uint64)
        cap = 1 << 31 if n_cols is None else int(n_cols)
        for lo in range(0, lengths.size, self.ROWS_PER_CALL):
            part, rows = lengths[lo:lo + self.ROWS_PER_CALL], rec[lo:lo + self.ROWS_PER_CALL]
            check(lib().gr4pm_row_resampler_output_lengths(self.taps_per_phase, int(part.max()), _np_ptr(part), _np_ptr(rows),
                                                           part.size, cap, _np_ptr(out[lo:lo + self.ROWS_PER_CALL])),
                  "RowResampler.output_lengths")
        return out.astype(np.int64)

    def tile_items(self, steps):
        """the output items of one tile of a call with these steps (host only): nothing but the time depends on it"""
        return int(lib().gr4pm_row_resampler_tile_items(self.taps_per_phase, max(int(s) for s in steps)))

    def process_rows(self, x, lengths, steps, phase0=None, freqs=None, n_cols=None, out=None):
        """gr4pm_row_resampler_process: x: a CUDA complex64 tensor [R, n] with contiguous rows (any row stride >= n);
        lengths: R item counts <= n (None: n each); steps, phase0 (None: 0): R Python or numpy integers in Q32.32, input
        items per output item and the position of output item 0; freqs (None: 0): R signed frequency words, cycles per
        input item times 2^32.  Returns (rows, out_lengths): rows is CUDA complex64 [R, n_cols] (None: the smallest
        multiple of 2048 that holds the longest row) with rows[r, :out_lengths[r]] the resampled row and +0 behind it,
        the layout NativeMultiChannelReceiver.submit takes; out_lengths is numpy int64.  out: an optional CUDA complex64
        [R, >= n_cols] tensor with contiguous rows.  Any number of rows: 64 go into one call.  Does not wait."""
        torch = _torch()
        _check_rows_input(x)
        n_rows, n_in = x.shape
        lengths = self._row_lengths(n_rows, n_in, lengths)
        rec = self._records(n_rows, steps, phase0, freqs)
        if n_cols is None:
            longest = int(self.output_lengths(lengths, rec["step"], rec["phase0"]).max()) if n_rows else 0
            n_cols = -(-longest // self.COLUMN_GRAIN) * self.COLUMN_GRAIN
        n_cols = int(n_cols)
        if n_cols < 0:
            raise Gr4pmError("RowResampler: n_cols must not be negative")
        h = self._handle()
        if torch.cuda.current_stream(x.device).cuda_stream != self._stream:
            _inputs_ready(x)  # made on another stream than the handle's
        out = _rows_output(out, n_rows, n_cols, x.device, "RowResampler")
        out_lengths = np.zeros(n_rows, dtype=np.uint64)
        for lo in range(0, n_rows, self.ROWS_PER_CALL):
            rows, part, dst = x[lo:lo + self.ROWS_PER_CALL], lengths[lo:lo + self.ROWS_PER_CALL], out[lo:lo + self.ROWS_PER_CALL]
            stride = rows.stride(0) if rows.shape[0] > 1 else max(n_in, 1)
            out_stride = dst.stride(0) if dst.shape[0] > 1 else max(dst.shape[1], n_cols)
            check(lib().gr4pm_row_resampler_process(
                h, rows.data_ptr(), stride, n_in, _np_ptr(part), _np_ptr(rec[lo:lo + self.ROWS_PER_CALL]), part.size,
                dst.data_ptr(), out_stride, n_cols, _np_ptr(out_lengths[lo:lo + self.ROWS_PER_CALL])), "RowResampler.process_rows")
        self._last = x  # the calls do not wait: the input lives until the next call
        return out[:, :n_cols], out_lengths.astype(np.int64)

    @staticmethod
    def steps_for(rates, samples_per_symbol=4):
        """round(2^32 / (samples_per_symbol * rho_r)) per row, in Python integers: the Q32.32 step that puts
        samples_per_symbol output items on a symbol of a row with rho_r symbols per item"""
        den = [fractions.Fraction(float(r)) * int(samples_per_symbol) for r in rates]
        if any(d <= 0 for d in den):
            raise Gr4pmError("RowResampler: a symbol rate must be positive")
        return [int(round(fractions.Fraction(1 << 32) / d)) for d in den]

    def to_samples_per_symbol(self, x, lengths, rates, offsets=None, samples_per_symbol=4, n_cols=None):
        """process_rows with step_r = round(2^32 / (samples_per_symbol rates[r])) and freq_r = round(offsets[r] 2^32):
        rates in symbols per item and offsets in cycles per item, as LineSpectrum.symbol_rate and .carrier_offset give
        them.  Returns (rows, out_lengths) with samples_per_symbol items per symbol and the offsets removed."""
        steps = self.steps_for(rates, samples_per_symbol)
        freqs = None if offsets is None else [_row_freq_word(d) for d in offsets]
        return self.process_rows(x, lengths, steps, None, freqs, n_cols)

    def __del__(self):
        _destroy(self, "gr4pm_row_resampler_destroy")


class StreamRowResampler:
    """gr4pm_row_stream: the RowResampler as a stream block.  Every row's position, history and phase
    are carried from call to call, so cutting the rows into calls changes no bit of what comes out, and the rows of
    MixedFftDdc.process_bulk go to exactly 4 samples per symbol call after call.  steps: one Q32.32 step per row (1 .. 64
    rows); freqs (None: 0): signed frequency words; phase0 (None: 0): the position of output item 0, below 2^63;
    start_index (None: 0): the absolute index of the first item each row is given (items in front of it are +0, and
    output begins with the first item at or behind it).  phases, taps_per_phase, taps, max_step: RowResampler's.  The
    handle is made at construction and is host only until the first process_rows or flush, which run on the stream that
    was current at construction: items_for, set_row, set_rate, state and reset work without a GPU."""

    COLUMN_GRAIN = 2048

    def __init__(self, steps, freqs=None, phase0=None, start_index=None, phases=32, taps_per_phase=12, taps=None, max_step=1.0):
        shape = RowResampler(phases, taps_per_phase, taps, max_step)  # the sizes' and the taps' checks, and the design
        self.phases, self.taps, self.taps_per_phase, self.delay_items = shape.phases, shape.taps, shape.taps_per_phase, shape.delay_items
        steps = [int(s) for s in (steps.tolist() if isinstance(steps, np.ndarray) else steps)]
        self.n_rows = len(steps)
        if not 1 <= self.n_rows <= 64:
            raise Gr4pmError(f"StreamRowResampler: {self.n_rows} rows, a handle has 1 .. 64")
        rec = shape._records(self.n_rows, steps, phase0, freqs)
        if start_index is None:
            start_index = [0] * self.n_rows
        start = [int(v) for v in (start_index.tolist() if isinstance(start_index, np.ndarray) else start_index)]
        if len(start) != self.n_rows or any(not 0 <= v < 1 << 64 for v in start):
            raise Gr4pmError(f"StreamRowResampler: start_index holds {self.n_rows} values that fit 64 unsigned bits")
        self.start_index = np.array(start, dtype=np.uint64)
        self._steps, self._freqs = [int(v) for v in rec["step"]], [int(v) for v in rec["freq"]]
        try:
            stream = _stream_handle()
        except Gr4pmError:  # no GPU: the host-only calls still work, process_rows and flush report the missing device
            stream = C.c_void_p()
        self._stream = stream.value
        p = _abi.RowStreamParams(self.phases, self.taps_per_phase, _np_ptr(self.taps), self.n_rows, _np_ptr(rec),
                                 _np_ptr(self.start_index), stream)
        self._h = C.c_void_p()
        check(lib().gr4pm_row_stream_create(C.byref(p), C.byref(self._h)), "StreamRowResampler")

    @classmethod
    def for_rates(cls, rates, offsets=None, samples_per_symbol=4, **kw):
        """a handle whose row r has rates[r] symbols per item and offsets[r] (None: 0) cycles per item of residual
        carrier: step_r = round(2^32 / (samples_per_symbol rates[r])), freq_r = round(offsets[r] 2^32)"""
        steps = RowResampler.steps_for(rates, samples_per_symbol)
        freqs = None if offsets is None else [_row_freq_word(d) for d in offsets]
        return cls(steps, freqs, **kw)

    _freq_word = staticmethod(_row_freq_word)

    def _lengths(self, lengths, n_cols=None):
        if lengths is None and n_cols is not None:
            return np.full(self.n_rows, n_cols, dtype=np.uint64)
        if lengths is None:
            raise Gr4pmError("StreamRowResampler: no lengths")
        lengths = RowResampler._row_lengths(self.n_rows, 0, lengths)
        if lengths.size != self.n_rows:
            raise Gr4pmError(f"StreamRowResampler: {lengths.size} lengths for {self.n_rows} rows")
        return lengths

    def items_for(self, lengths):
        """what the next process_rows with these lengths would report (numpy int64; host only, changes no state)"""
        lengths = self._lengths(lengths)
        out = np.zeros(self.n_rows, dtype=np.uint64)
        check(lib().gr4pm_row_stream_items_for(self._h, _np_ptr(lengths), _np_ptr(out)), "StreamRowResampler.items_for")
        return out.astype(np.int64)

    def _columns(self, counts):
        longest = int(counts.max())
        return -(-longest // self.COLUMN_GRAIN) * self.COLUMN_GRAIN

    def process_rows(self, x, lengths=None, out=None):
        """x: a CUDA complex64 tensor [R, n] with contiguous rows (any row stride >= n), the next lengths[r] <= n items of
        every row (None: n each), the layout MixedFftDdc.process_bulk returns.  Returns (rows, out_lengths): rows is CUDA
        complex64 [R, columns] with rows[r, :out_lengths[r]] the items row r made in this call and +0 behind them;
        columns is the smallest multiple of 2048 that holds the longest count, or out's (an optional CUDA complex64
        [R, columns] tensor with contiguous rows; one that is too short for a row's count is refused, nothing is cut).
        out_lengths is numpy int64.  Does not wait."""
        torch = _torch()
        _check_rows_input(x, self.n_rows)
        n_in = x.shape[1]
        lengths = self._lengths(lengths, n_in)
        if out is None:
            out = _rows_output(None, self.n_rows, self._columns(self.items_for(lengths)), x.device, "StreamRowResampler")
        else:
            out = _rows_output(out, self.n_rows, 0, x.device, "StreamRowResampler")
        if torch.cuda.current_stream(x.device).cuda_stream != self._stream:
            _inputs_ready(x)  # made on another stream than the handle's
        n_cols = out.shape[1]
        stride = x.stride(0) if self.n_rows > 1 else max(n_in, 1)
        out_stride = out.stride(0) if self.n_rows > 1 else max(n_cols, 1)
        out_lengths = np.zeros(self.n_rows, dtype=np.uint64)
        check(lib().gr4pm_row_stream_process(self._h, x.data_ptr() if n_in else None, stride, n_in, _np_ptr(lengths),
                                             out.data_ptr() if n_cols else None, out_stride, n_cols, _np_ptr(out_lengths)),
              "StreamRowResampler.process_rows")
        self._last = x  # the call does not wait: the input lives until the next call
        return out, out_lengths.astype(np.int64)

    def flush_lengths(self):
        """the items flush() will make per row (numpy int64; host only): P - 1 items of +0 behind the last one"""
        return self.items_for(np.full(self.n_rows, self.taps_per_phase - 1, dtype=np.uint64))

    def flush(self, out=None):
        """the items whose windows run out over +0 behind the rows' last items, as the one-shot block's M_r counts them;
        then every row is back in its created state with its current step and freq.  Returns (rows, out_lengths) as
        process_rows does; without out the tensor lives on the current device."""
        torch = _torch()
        if out is None:
            out = torch.empty((self.n_rows, self._columns(self.flush_lengths())), dtype=torch.complex64, device="cuda")
        else:
            out = _rows_output(out, self.n_rows, 0, out.device, "StreamRowResampler")
        n_cols = out.shape[1]
        out_stride = out.stride(0) if self.n_rows > 1 else max(n_cols, 1)
        out_lengths = np.zeros(self.n_rows, dtype=np.uint64)
        check(lib().gr4pm_row_stream_flush(self._h, out.data_ptr() if n_cols else None, out_stride, n_cols, _np_ptr(out_lengths)),
              "StreamRowResampler.flush")
        return out, out_lengths.astype(np.int64)

    def reset(self):
        """every row back to its created state, with its current step and freq; no output"""
        check(lib().gr4pm_row_stream_reset(self._h), "StreamRowResampler.reset")

    def set_row(self, r, step=None, freq=None):
        """a new step and / or frequency word for row r from its next output item on: that item's position stays, later
        ones follow it at the new step, and the phase is continuous there"""
        r = int(r)
        if not 0 <= r < self.n_rows:
            raise Gr4pmError(f"StreamRowResampler: row {r} of {self.n_rows}")
        step = self._steps[r] if step is None else int(step)
        freq = self._freqs[r] if freq is None else int(freq)
        if not (0 <= step < 1 << 64 and -(1 << 31) <= freq < 1 << 31):
            raise Gr4pmError("StreamRowResampler: step must fit 64 unsigned bits and freq 32 signed bits")
        check(lib().gr4pm_row_stream_set_row(self._h, r, step, freq), "StreamRowResampler.set_row")
        self._steps[r], self._freqs[r] = step, freq

    def set_rate(self, r, rate, offset=None, samples_per_symbol=4):
        """set_row from a symbol rate in symbols per item and (None: unchanged) an offset in cycles per item"""
        self.set_row(r, RowResampler.steps_for([rate], samples_per_symbol)[0], None if offset is None else _row_freq_word(offset))

    def state(self, r):
        """(items_in, items_out) of row r: the absolute index of its next input item and the index of its next output item"""
        a, m = C.c_uint64(0), C.c_uint64(0)
        check(lib().gr4pm_row_stream_state(self._h, int(r), C.byref(a), C.byref(m)), "StreamRowResampler.state")
        return a.value, m.value

    def __del__(self):
        _destroy(self, "gr4pm_row_stream_destroy")


class RowBurstGate:
    """gr4pm_row_gate: a power squelch on rows that carries its state from call to call.  Fed with
    MixedFftDdc.process_bulk's ragged rows call after call, it delivers every burst of every row once, as a zero-padded row
    of the [bursts, n_cols] layout that LineSpectrum, RowResampler and the receivers take; cutting the rows into calls
    changes no byte of a row's records and burst rows.  block: B, a power of two 16 .. 1024; a block whose power sum
    reaches the row's open_sum opens a burst, hold_blocks + 1 blocks in a row below its close_sum close it, bursts of
    fewer than min_blocks blocks are dropped, pre_blocks and post_blocks (<= hold_blocks + 1) blocks of margin go with a
    burst, and the block that completes max_blocks (None: n_cols // block) ends one that is still open (its record has
    TRUNCATED).  The gate is shut until set_thresholds or set_floor.  The handle is made at construction and is host only
    until the first process_rows, flush or block_power, which run on the stream that was current at construction."""

    TRUNCATED, AT_END = _abi.ROW_GATE_TRUNCATED, _abi.ROW_GATE_AT_END

    def __init__(self, n_rows, n_cols=4096, block=64, hold_blocks=3, min_blocks=2, pre_blocks=4, post_blocks=4, max_blocks=None):
        self.n_rows, self.n_cols, self.block = int(n_rows), int(n_cols), int(block)
        values = [self.n_rows, self.n_cols, self.block, int(hold_blocks), int(min_blocks), int(pre_blocks), int(post_blocks),
                  0 if max_blocks is None else int(max_blocks)]
        if any(not 0 <= v < 1 << 32 for v in values):
            raise Gr4pmError("RowBurstGate: the sizes must fit 32 unsigned bits")
        if max_blocks is not None and values[7] == 0:
            raise Gr4pmError("RowBurstGate: max_blocks is 1 or more")
        try:
            stream = _stream_handle()
        except Gr4pmError:  # no GPU: the host-only calls still work, the others report the missing device
            stream = C.c_void_p()
        self._stream = stream.value
        p = _abi.RowGateParams(*values, 0.0, 0.0, stream)
        self._h = C.c_void_p()
        check(lib().gr4pm_row_gate_create(C.byref(p), C.byref(self._h)), "RowBurstGate")
        b, m, n = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
        check(lib().gr4pm_row_gate_sizes(self._h, C.byref(b), C.byref(m), C.byref(n)), "RowBurstGate")
        self.max_blocks = m.value

    def _rows(self, x):
        torch = _torch()
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.complex64 and x.dim() == 2 and
                x.shape[0] == self.n_rows and (x.shape[1] <= 1 or x.stride(1) == 1) and
                (x.shape[0] <= 1 or x.stride(0) >= x.shape[1])):
            raise TypeError(f"rows must be a [{self.n_rows}, n] complex64 CUDA tensor with contiguous rows")
        if torch.cuda.current_stream(x.device).cuda_stream != self._stream:
            _inputs_ready(x)  # made on another stream than the handle's
        return x.shape[1], (x.stride(0) if self.n_rows > 1 else max(x.shape[1], 1))

    def _lengths(self, lengths, n_in):
        if lengths is None:
            return np.full(self.n_rows, n_in, dtype=np.uint64)
        lengths = RowResampler._row_lengths(self.n_rows, 0, lengths)
        if lengths.size != self.n_rows:
            raise Gr4pmError(f"RowBurstGate: {lengths.size} lengths for {self.n_rows} rows")
        return lengths

    def _emit(self, what, call, cap, out, device):
        """runs call(out_ptr, out_stride, cap, records_ptr, count_ptr); with cap None a capacity refusal is followed by one
        more call with the count the library reports"""
        torch = _torch()
        given, want = cap is not None or out is not None, (4 * self.n_rows + 12 if cap is None else int(cap))
        if out is not None:
            out = _rows_output(out, out.shape[0], self.n_cols, device, "RowBurstGate")
            want = out.shape[0] if cap is None else min(want, out.shape[0])
        count = C.c_size_t(0)
        for attempt in range(2):
            rows = out if out is not None else torch.empty((want, self.n_cols), dtype=torch.complex64, device=device)
            records = np.zeros(max(want, 1), dtype=_abi.ROW_GATE_RECORD_DTYPE)
            stride = rows.stride(0) if rows.shape[0] > 1 else self.n_cols
            status = call(rows.data_ptr() if want else None, stride, want, _np_ptr(records), C.byref(count))
            if status == -5 and count.value > want and not given and attempt == 0:  # GR4PM_ERR_OVERFLOW: the capacity
                want = count.value
                continue
            check(status, what)
            break
        n = count.value
        records = records[:n].copy()
        return rows[:n], records["n_items"].astype(np.int64), records

    def process_rows(self, rows, lengths=None, cap=None, out=None):
        """rows: a CUDA complex64 tensor [n_rows, n] with contiguous rows, the next lengths[r] <= n items of every row
        (None: n each).  Returns (burst_rows, burst_lengths, records): burst_rows is CUDA complex64 [bursts, n_cols] with
        the span's items and +0 behind them, in the order (row, time); burst_lengths numpy int64; records a structured
        array (row, first_item, n_items, first_active_item, active_items, flags, peak, power).  cap: the most bursts the
        call may emit (None: a guess, and a second call with the library's count if it was too small; nothing is ever
        lost); a call that would emit more raises and changes nothing.  out: an optional CUDA complex64 [cap, >= n_cols]
        tensor.  Waits for the block sums; the copies into burst_rows are enqueued, not waited for."""
        n_in, stride = self._rows(rows)
        lengths = self._lengths(lengths, n_in)
        res = self._emit("RowBurstGate.process_rows", lambda o, os_, c, rec, cnt: lib().gr4pm_row_gate_process(
            self._h, rows.data_ptr() if n_in else None, stride, _np_ptr(lengths), o, os_, c, rec, cnt), cap, out, rows.device)
        self._last = rows  # the copies do not wait: the input lives until the next call
        return res

    def flush(self, cap=None, out=None):
        """the end of the rows: an incomplete block is decided with +0 behind it, open bursts close (AT_END) with their
        margins clipped to the items that exist; then every row is in its created state, thresholds kept.  Returns what
        process_rows returns."""
        device = out.device if out is not None else _torch().device("cuda", _torch().cuda.current_device())
        return self._emit("RowBurstGate.flush", lambda o, os_, c, rec, cnt: lib().gr4pm_row_gate_flush(self._h, o, os_, c, rec, cnt),
                          cap, out, device)

    def reset(self):
        """every row back to its created state without output; the thresholds stay"""
        check(lib().gr4pm_row_gate_reset(self._h), "RowBurstGate.reset")

    def state(self, row):
        """dict(items, blocks, open, emitted, dropped, truncated) of a row (host only)"""
        s = _abi.RowGateState()
        check(lib().gr4pm_row_gate_state(self._h, int(row), C.byref(s)), "RowBurstGate.state")
        return dict(items=s.items, blocks=s.blocks, open=bool(s.open), emitted=s.emitted, dropped=s.dropped, truncated=s.truncated)

    def set_thresholds(self, row, open_sum, close_sum):
        """the block sums (float32) that open and keep open a burst of this row, from the next block decided:
        0 < close_sum <= open_sum"""
        check(lib().gr4pm_row_gate_set_thresholds(self._h, int(row), float(np.float32(open_sum)), float(np.float32(close_sum))),
              "RowBurstGate.set_thresholds")

    def set_floor(self, floors, open_db=10.0, close_db=6.0):
        """set_thresholds for every row from its noise floor in power per item: floor * block * 10^(dB / 10), rounded to
        float32 once"""
        floors = np.asarray(floors, dtype=np.float64).reshape(-1)
        if floors.size != self.n_rows:
            raise Gr4pmError(f"RowBurstGate: {floors.size} floors for {self.n_rows} rows")
        for r, f in enumerate(floors):
            self.set_thresholds(r, np.float32(f * self.block * 10.0 ** (open_db / 10.0)),
                                np.float32(f * self.block * 10.0 ** (close_db / 10.0)))

    def block_power(self, rows, lengths=None):
        """the block sums of rows that begin at item 0, by the gate's kernel and in its order; changes no state.  Returns a
        list of numpy float32 arrays, lengths[r] // block sums each.  Waits."""
        torch = _torch()
        n_in, stride = self._rows(rows)
        lengths = self._lengths(lengths, n_in)
        cols = max(n_in // self.block, 1)
        out = torch.empty((self.n_rows, cols), dtype=torch.float32, device=rows.device)
        check(lib().gr4pm_row_gate_block_power(self._h, rows.data_ptr() if n_in else None, stride, _np_ptr(lengths), out.data_ptr(), cols),
              "RowBurstGate.block_power")
        torch.cuda.synchronize(rows.device)  # the handle's stream need not be torch's current one
        sums = out.cpu().numpy()
        return [sums[r, :int(lengths[r]) // self.block].copy() for r in range(self.n_rows)]

    def measure_floor(self, rows, lengths=None, quantile=0.1):
        """per row the `quantile` order statistic (the sorted block powers' item floor(quantile * count)) of its block
        powers per item, 0 for a row without a complete block: a low quantile, because a band may be on the air most of
        the time"""
        out = np.zeros(self.n_rows, dtype=np.float64)
        for r, s in enumerate(self.block_power(rows, lengths)):
            if s.size:
                out[r] = float(np.sort(s)[min(int(quantile * s.size), s.size - 1)]) / self.block
        return out

    def __del__(self):
        _destroy(self, "gr4pm_row_gate_destroy")


class RowPacketReceivers:
    """one NativePacketReceiver(decode_headers=True, packets_only=True) per row behind a StreamRowResampler: host
    composition of existing blocks, for rows that grow by different lengths per call.  Each row keeps the items its
    receiver has not consumed yet and presents them again in front of the next ones; nothing is submitted below the
    receiver's smallest batch of 3072 items.  max_items: the most items one batch holds.  receiver_kw: samples_per_symbol,
    syncword_freq_bins, syncword_threshold, costas_constellation of the receivers."""

    MIN_BATCH = 3072  # one header window and one FFT block
    TAIL = 12288      # zeros flush() appends: the receiver delivers a packet once the stream goes on well behind it

    def __init__(self, n_rows, max_items=1 << 20, **receiver_kw):
        self.n_rows, self.max_items = int(n_rows), int(max_items)
        if self.n_rows < 1 or self.max_items < self.MIN_BATCH:
            raise Gr4pmError(f"RowPacketReceivers: need at least one row and batches of {self.MIN_BATCH} items or more")
        self._rx = [NativePacketReceiver(max_items=self.max_items + 4096, tags_cap=self.max_items // 768 + 64,
                                         decode_headers=True, packets_only=True, **receiver_kw) for _ in range(self.n_rows)]
        self._left = [None] * self.n_rows
        self.stats = [{"items": 0, "headers": 0, "invalid_headers": 0, "crc_failures": 0} for _ in range(self.n_rows)]

    def _run(self, r, new):
        """row r's receiver over what it has left and `new`; returns the packets"""
        torch = _torch()
        left = self._left[r]
        work = new if left is None or not left.numel() else (torch.cat([left, new]) if new.numel() else left)
        packets, stats = [], self.stats[r]
        while work.numel() >= self.MIN_BATCH:
            n = min(work.numel(), self.max_items)
            res = self._rx[r].process_bulk(work[:n].contiguous())
            if res.get("status", 0):
                raise Gr4pmError(f"RowPacketReceivers: row {r}: the receiver lost a batch: {res.get('error')}")
            m, lens = res["header_messages"], res["packet_lengths"]
            stats["headers"] += int(m.size)
            stats["invalid_headers"] += int(np.sum(m["invalid_header"] != 0))
            stats["crc_failures"] += int(np.sum(lens == 0))
            data, pos = res["packets"].cpu().numpy(), 0
            for k in lens[lens > 0]:
                packets.append(data[pos:pos + int(k)].tobytes())
                pos += int(k)
            c = int(res["consumed"])
            stats["items"] += c
            work = work[c:]
            if c == 0 or (n < self.max_items and work.numel() < self.MIN_BATCH):
                break
        self._left[r] = work.clone()
        return packets

    def process_rows(self, rows, lengths):
        """rows: CUDA complex64 [n_rows, columns]; lengths: the items of each row in this call.  Returns a list per row of
        the packets (bytes) its receiver delivered."""
        if rows.shape[0] != self.n_rows or len(lengths) != self.n_rows:
            raise Gr4pmError(f"RowPacketReceivers: {rows.shape[0]} rows and {len(lengths)} lengths for {self.n_rows} receivers")
        return [self._run(r, rows[r, :int(lengths[r])]) for r in range(self.n_rows)]

    def flush(self):
        """appends the zeros a last packet needs behind it to every row and returns the packets that come out; what a
        receiver still has not consumed is dropped"""
        torch = _torch()
        out = []
        for r in range(self.n_rows):
            out.append(self._run(r, torch.zeros(self.TAIL, dtype=torch.complex64, device="cuda")))
            self._left[r] = None
        return out


class MultiChannelPacketReceiver:
    """BASELINE config 3: `n_channels` independent receive chains on one GPU
    (packet_receiver.hpp:191-265 couples nothing across receivers).  The detector is ONE batched
    SyncwordDetection handle (every launch covers all channels, blockIdx.y = channel); behind
    it every channel has its own SyncwordDetectionFilter / CoarseFrequencyCorrection /
    SymbolFilter / SyncwordWipeoff / CostasLoop with their carried state, and the channels'
    chains are spread over `workers` host threads, each with a HIP stream of its own, whose
    process() calls queue up without waiting in between (gr4pm_set_deferred_sync).
    process_bulk(x[n_channels, n]) returns one PacketReceiver-style result per channel."""

    def __init__(self, n_channels, samples_per_symbol=4, syncword_freq_bins=4, syncword_threshold=9.5,
                 costas_constellation="QPSK", max_items=1 << 22, workers=8, soft_bits=False):
        import concurrent.futures
        torch = _torch()
        self.n_channels = n_channels
        workers = max(1, min(workers, n_channels))
        self._streams = [torch.cuda.Stream() for _ in range(workers)]
        self.chains = []
        for c in range(n_channels):
            with torch.cuda.stream(self._streams[c % workers]):
                self.chains.append(PacketReceiver(samples_per_symbol, syncword_freq_bins, syncword_threshold,
                                                  costas_constellation, soft_bits=soft_bits, detector=False))
        bpsk = np.array([1, -1], dtype=np.complex64)
        self.syncword_detection = SyncwordDetection(
            self.chains[0].rrc_taps, SYNCWORD, bpsk, -syncword_freq_bins, syncword_freq_bins,
            samples_per_symbol=samples_per_symbol, power_threshold=syncword_threshold, n_channels=n_channels,
            max_items=max_items)
        self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=workers, initializer=torch.cuda.set_device,
                                                           initargs=(torch.cuda.current_device(),))

    def announce(self, x):
        self.syncword_detection.announce(x)

    def _run_worker(self, w, y, det_tags, n, base, header_fn):
        torch = _torch()
        lib().gr4pm_set_deferred_sync(1)  # per thread: the calls below only queue their kernels
        out = {}
        try:
            with torch.cuda.stream(self._streams[w]):
                for c in range(w, self.n_channels, len(self._streams)):
                    chain = self.chains[c]
                    out[c] = chain._stage2(chain._stage1(0, y[c], det_tags[c], n, base, header_fn))
            self._streams[w].synchronize()
        finally:
            lib().gr4pm_set_deferred_sync(0)
        return out

    def process_bulk(self, x, header_fn=None, tags_cap=4096):
        """x: [n_channels, n] complex64 on the GPU.  Returns a list (one per channel) of
        dict(consumed, symbols, tags, detector_tags, ...) as PacketReceiver.process_bulk does."""
        st, y, det_tags, n = self.syncword_detection.process_bulk(x, want_output=True, tags_cap=tags_cap)
        if st != 0:
            return [{"status": st, "consumed": 0, "symbols": None, "tags": t, "detector_tags": t} for t in det_tags]
        base = self.syncword_detection._items_consumed - n
        _torch().cuda.current_stream().synchronize()  # y is read on the workers' streams
        futs = [self._pool.submit(self._run_worker, w, y, det_tags, n, base, header_fn)
                for w in range(len(self._streams))]
        res = {}
        for f in futs:
            res.update(f.result())
        return [res[c] for c in range(self.n_channels)]


class NativeMultiChannelReceiver:
    """gr4pm_multichannel_receiver: what MultiChannelPacketReceiver composes in Python, inside the
    library (one batched detector, every channel's own chain on worker threads with a stream each).
    process_bulk(x[n_channels, n], packet_length) -> one dict per channel."""

    def __init__(self, n_channels, samples_per_symbol=4, syncword_freq_bins=4, syncword_threshold=9.5,
                 costas_constellation="QPSK", max_items=1 << 22, tags_cap=4096, workers=12, output_ring=False):
        self.n_channels = n_channels
        # output_ring (streaming callers, bench.py): submit() takes its symbol buffer from a ring of 6 (more than the
        # batches in flight) instead of allocating one per batch -- a device allocation in the middle of a stream stalls
        # every stage; a result's "symbols" then stay valid until five further batches have been submitted
        self.output_ring = output_ring
        self._ring, self._ring_next = [], 0
        self.samples_per_symbol = samples_per_symbol
        self.tags_cap = max(int(tags_cap), 64)
        p = _abi.MultiChannelReceiverParams(n_channels, samples_per_symbol, syncword_freq_bins, syncword_threshold,
                                            {"PILOT": 0, "BPSK": 1, "QPSK": 2}[costas_constellation], max_items,
                                            self.tags_cap, workers)
        self._h = C.c_void_p()
        self._pending = []
        check(lib().gr4pm_multichannel_receiver_create(C.byref(p), C.byref(self._h)), "MultiChannelReceiver")

    def announce(self, x):
        x = _dev_c64_rows(x)
        assert x.dim() == 2 and x.shape[0] == self.n_channels
        _inputs_ready(x)
        check(lib().gr4pm_multichannel_receiver_announce(self._h, x.data_ptr(), x.stride(0), x.shape[1]),
              "MultiChannelReceiver.announce")

    def submit(self, x, packet_length=None):
        """pipelined form: returns the items consumed per channel as soon as the detector has taken the batch;
        the stages behind it keep working on up to four batches.  Results come from collect(), in order."""
        torch = _torch()
        x = _dev_c64_rows(x)
        assert x.dim() == 2 and x.shape[0] == self.n_channels
        _inputs_ready(x)
        Cn, n = self.n_channels, x.shape[1]
        stride = n // self.samples_per_symbol + self.tags_cap + 64
        if self.output_ring:
            if not self._ring or self._ring[0].shape[1] < stride:
                self._ring = [torch.empty((Cn, stride), dtype=torch.complex64, device=x.device) for _ in range(6)]
            sym = self._ring[self._ring_next][:, :stride]
            stride = self._ring[self._ring_next].stride(0)
            self._ring_next = (self._ring_next + 1) % 6
        else:
            sym = torch.empty((Cn, stride), dtype=torch.complex64, device=x.device)
        consumed = C.c_size_t(0)
        check(lib().gr4pm_multichannel_receiver_submit(
            self._h, x.data_ptr(), x.stride(0), n, 0 if packet_length is None else int(packet_length),
            sym.data_ptr(), stride, C.byref(consumed)), "MultiChannelReceiver.submit")
        self._pending.append((sym, x))  # keep the buffers alive until collected
        return consumed.value

    def in_flight(self):
        return int(lib().gr4pm_multichannel_receiver_in_flight(self._h))

    def set_input_in_place(self, on=True):
        """the caller keeps every submitted input unchanged until it has been collected (a device ring): the receiver
        reads the detector's delayed stream in place instead of writing a delayed copy per batch.  Same results."""
        check(lib().gr4pm_multichannel_receiver_set_input_in_place(self._h, 1 if on else 0),
              "MultiChannelReceiver.set_input_in_place")

    def collect(self):
        Cn = self.n_channels
        sym, _x = self._pending.pop(0)
        consumed = C.c_size_t(0)
        n_sym, n_tags, n_det = (C.c_size_t * Cn)(), (C.c_size_t * Cn)(), (C.c_size_t * Cn)()
        tags = np.zeros((Cn, self.tags_cap), dtype=TAG_DTYPE)
        det = np.zeros((Cn, self.tags_cap), dtype=TAG_DTYPE)
        check(lib().gr4pm_multichannel_receiver_collect(self._h, C.byref(consumed), n_sym, _np_ptr(tags), n_tags,
                                                        _np_ptr(det), n_det), "MultiChannelReceiver.collect")
        return [{"status": 0, "consumed": consumed.value, "symbols": sym[c, : n_sym[c]],
                 "tags": tags[c, : n_tags[c]].copy(), "detector_tags": det[c, : n_det[c]].copy()} for c in range(Cn)]

    def process_bulk(self, x, packet_length=None):
        torch = _torch()
        x = _dev_c64_rows(x)
        assert x.dim() == 2 and x.shape[0] == self.n_channels
        _inputs_ready(x)
        Cn, n = self.n_channels, x.shape[1]
        stride = n // self.samples_per_symbol + self.tags_cap + 64
        sym = torch.empty((Cn, stride), dtype=torch.complex64, device=x.device)
        consumed = C.c_size_t(0)
        n_sym, n_tags, n_det = (C.c_size_t * Cn)(), (C.c_size_t * Cn)(), (C.c_size_t * Cn)()
        tags = np.zeros((Cn, self.tags_cap), dtype=TAG_DTYPE)
        det = np.zeros((Cn, self.tags_cap), dtype=TAG_DTYPE)
        check(lib().gr4pm_multichannel_receiver_process(
            self._h, x.data_ptr(), x.stride(0), n, 0 if packet_length is None else int(packet_length),
            sym.data_ptr(), stride, C.byref(consumed), n_sym, _np_ptr(tags), n_tags, _np_ptr(det), n_det),
            "MultiChannelReceiver.process")
        return [{"status": 0, "consumed": consumed.value, "symbols": sym[c, : n_sym[c]],
                 "tags": tags[c, : n_tags[c]].copy(), "detector_tags": det[c, : n_det[c]].copy()} for c in range(Cn)]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_multichannel_receiver_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class NativePacketReceiver:
    """gr4pm_packet_receiver: the same chain as PacketReceiver (front end, or soft_bits up to the
    LLR decoder) composed and pipelined in the C++ library -- stage threads, streams and
    intermediate buffers live there, so no Python runs between the kernels of a batch.
    Identical outputs (tests compare bit for bit).  parsed_header feedback: a constant
    packet_length per call (None: every header invalid)."""

    def __init__(self, samples_per_symbol=4, syncword_freq_bins=4, syncword_threshold=9.5,
                 costas_constellation="QPSK", max_items=1 << 22, tags_cap=4096, pipelined=False, soft_bits=False,
                 decode_headers=False, output_ring=False, packets_only=False, result_fields="all", packets_cap=None):
        """result_fields="packets" (decode_headers): collect() marshals only what a packet sink needs -- consumed, the accepted
        detections' tags, header messages, packet lengths and bytes -- and leaves the per-symbol tag lists (tens of thousands
        of 96-byte records per batch on a packet-dense stream) in the library; "all": everything the C result holds.
        packets_only (a form of decode_headers; include/gr4pm_hip.h): IQ in, CRC-checked packets out, the stream between
        the Costas loop and the packer never written to memory -- the same packets / header messages / tags; the result
        has no "llr", "payload_llr" and "pdu_symbols" arrays (None)"""
        soft_bits = soft_bits or decode_headers
        self.packets_only = bool(packets_only)
        assert result_fields in ("all", "packets")
        self.result_fields = result_fields
        self._packets_cap = packets_cap  # (tests: a packet output buffer that is too small for a batch)
        self.output_ring = output_ring
        self.samples_per_symbol, self.pipelined, self.soft_bits = samples_per_symbol, pipelined, soft_bits
        self.decode_headers = decode_headers
        self.time_threshold = 768
        self._alist = header_ldpc_alist().encode() if decode_headers else None
        p = _abi.PacketReceiverParams(samples_per_symbol, syncword_freq_bins, syncword_threshold,
                                      CONSTELLATIONS[costas_constellation.upper()], max_items, tags_cap,
                                      1 if pipelined else 0, 1 if soft_bits else 0, 1 if decode_headers else 0,
                                      self._alist, 1 if packets_only else 0)
        self._h = C.c_void_p()
        check(lib().gr4pm_packet_receiver_create(C.byref(p), C.byref(self._h)), "PacketReceiver")
        self._keep = []  # (input tensors, output tensors) of the batches in flight

    def announce(self, x):
        """names the input of a later submit (after the ones already announced): the detector's
        look-ahead, up to two batches ahead.  The caller keeps x alive and unchanged until then."""
        x = _dev_c64(x)
        _inputs_ready(x)
        check(lib().gr4pm_packet_receiver_announce(self._h, x.data_ptr(), x.numel()), "PacketReceiver.announce")

    # output buffers.  output_ring=True (streaming callers, bench.py): a ring of _out_ring_sets() sets, one more than
    # the batches the library accepts in flight (gr4pm_packet_receiver_max_inflight), allocated at the first submit and
    # whenever a bigger batch arrives -- not once per call: a device allocation in the middle of a stream stalls every
    # stage.  No two batches in flight share a set, and a result's "symbols" / "llr" / "packets" stay valid until
    # max_inflight further batches have been submitted (a refused submit takes no set).
    @staticmethod
    def _out_ring_sets():
        return int(lib().gr4pm_packet_receiver_max_inflight()) + 1

    def _new_outputs(self, n, device):
        torch = _torch()
        sps = self.samples_per_symbol
        n_sym = n // sps + 4160
        # packets: a QPSK stream carries at most n / (4 sps) payload bytes -- n // 16 at 4 samples per symbol, the lowest
        # rate decode_headers takes, and never less above it; 65536 for the packet that a batch finishes for the one before
        return (torch.empty(n_sym, dtype=torch.complex64, device=device),
                torch.empty(2 * n_sym if self.soft_bits and not self.packets_only else 1, dtype=torch.float32, device=device),
                torch.empty((self._packets_cap or n // (4 * min(sps, 4)) + 65536) if self.decode_headers else 1,
                            dtype=torch.uint8, device=device))

    def _outputs(self, n, device):
        """the output set of the next submit; _out_next moves on only once the library has taken the batch"""
        if not self.output_ring:  # fresh buffers for every batch: results stay valid as long as they are referenced
            return self._new_outputs(n, device)
        if getattr(self, "_out_n", -1) < n:
            self._out_ring = [self._new_outputs(n, device) for _ in range(self._out_ring_sets())]
            self._out_n, self._out_next = n, 0
        return self._out_ring[self._out_next]

    def submit(self, x, packet_length=None, history=None, next_x=None):
        x = _dev_c64(x)
        _inputs_ready(x)
        n = x.numel()
        sym, llr, pk = self._outputs(n, x.device)
        delayed = None
        if history is not None:
            d = 2 * self.time_threshold + 1
            assert history.numel() >= d and history.data_ptr() + history.numel() * 8 == x.data_ptr(), \
                "history must be the ring contents that directly precede x"
            delayed = x.data_ptr() - 8 * d
        nx = None if next_x is None else _dev_c64(next_x)
        check(lib().gr4pm_packet_receiver_submit(
            self._h, x.data_ptr(), n, delayed, None if nx is None else nx.data_ptr(), 0 if nx is None else nx.numel(),
            0 if packet_length is None else int(packet_length), sym.data_ptr(), sym.numel(),
            llr.data_ptr() if self.soft_bits and not self.packets_only else None, llr.numel(),
            pk.data_ptr() if self.decode_headers else None, pk.numel()), "PacketReceiver.submit")
        if self.output_ring:
            self._out_next = (self._out_next + 1) % len(self._out_ring)
        self._keep.append((x, history, nx, sym, llr, pk))

    def collect(self):
        r = _abi.PacketReceiverResult()
        st = lib().gr4pm_packet_receiver_collect(self._h, C.byref(r))
        x, history, nx, sym, llr, pk = self._keep.pop(0)
        check(st, "PacketReceiver")
        if st > 0:  # a gr::work::Status the batch ended with (INSUFFICIENT_OUTPUT_ITEMS ...): the batch is lost, the receiver goes on
            return {"status": int(st), "error": lib().gr4pm_last_error().decode(), "consumed": r.consumed}

        def records(ptr, n, dtype):
            if not n:
                return np.zeros(0, dtype=dtype)
            buf = (C.c_char * (n * dtype.itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype, count=n).copy()

        if self.result_fields == "packets" and self.decode_headers:
            res = {"status": 0, "consumed": r.consumed, "symbols": sym[: r.n_symbols], "tags": records(r.tags, r.n_tags, TAG_DTYPE),
                   "n_detector_tags": int(r.n_detector_tags), "n_packet_tags": int(r.n_packet_tags),
                   "header_messages": records(r.header_messages, r.n_header_messages, _abi.HEADER_MSG_DTYPE),
                   "header_mismatches": r.header_mismatches, "packets": pk[: r.n_packet_bytes],
                   "packet_lengths": records(r.packet_lengths, r.n_packets, np.dtype(np.uint64))}
            res["crc_ok"] = res["packet_lengths"] > 0
            return res
        res = {"status": 0, "consumed": r.consumed, "symbols": sym[: r.n_symbols],
               "tags": records(r.tags, r.n_tags, TAG_DTYPE),
               "detector_tags": records(r.detector_tags, r.n_detector_tags, TAG_DTYPE),
               "accepted": records(r.accepted, r.n_detector_tags, np.dtype(np.uint8)).astype(bool)}
        if self.soft_bits:
            torch = _torch()
            pdu_sym = None
            if not self.packets_only:
                pdu_sym = torch.empty(r.n_pdu_symbols, dtype=torch.complex64, device=sym.device)
                if r.n_pdu_symbols:  # the library's buffer is recycled: take a copy
                    check(_hip_memcpy_d2d(pdu_sym.data_ptr(), r.pdu_symbols, 8 * r.n_pdu_symbols), "pdu_symbols")
            res.update(pdu_symbols=pdu_sym, symbol_pdus=records(r.symbol_pdus, r.n_symbol_pdus, _abi.SYMBOL_PDU_DTYPE))
            res.update(llr=None if self.packets_only else llr[: r.n_llr], n_llr=int(r.n_llr),
                       llr_tags=records(r.llr_tags, r.n_llr_tags, PACKET_TAG_DTYPE),
                       packet_tags=records(r.packet_tags, r.n_packet_tags, PACKET_TAG_DTYPE),
                       ignored_syncwords=r.ignored_syncwords)
        if self.decode_headers:
            torch = _torch()
            pay = None
            if not self.packets_only:
                pay = torch.empty(r.n_payload_llr, dtype=torch.float32, device=llr.device)
                if r.n_payload_llr:  # the library's buffer is recycled at the next collect(): take a copy
                    check(_hip_memcpy_d2d(pay.data_ptr(), r.payload_llr, 4 * r.n_payload_llr), "payload_llr")
            res.update(header_messages=records(r.header_messages, r.n_header_messages, _abi.HEADER_MSG_DTYPE),
                       packet_type=records(r.packet_type, r.n_header_messages, np.dtype(np.int32)),
                       header_mismatches=r.header_mismatches, payload_llr=pay, n_payload_llr=int(r.n_payload_llr),
                       payload_tags=records(r.payload_tags, r.n_payload_tags, PACKET_TAG_DTYPE),
                       packets=pk[: r.n_packet_bytes],
                       packet_lengths=records(r.packet_lengths, r.n_packets, np.dtype(np.uint64)))
            res["crc_ok"] = res["packet_lengths"] > 0
        return res

    def set_symbol_pdu_callback(self, fn):
        """the symbol PDU tap (packet_receiver.hpp:159-189): fn(kind, symbols) is called from collect() once per
        complete header (kind 0, 128 symbols) / payload (kind 1) PDU with a numpy copy of its symbols; None removes it"""
        if fn is None:
            self._pdu_cb = None
            check(lib().gr4pm_packet_receiver_set_symbol_pdu_callback(self._h, None, None), "set_symbol_pdu_callback")
            return

        def tramp(user, kind, ptr, n):
            buf = (C.c_char * (8 * n)).from_address(ptr)
            fn(int(kind), np.frombuffer(buf, dtype=np.complex64, count=n).copy())
        self._pdu_cb = _abi.SYMBOL_PDU_FN(tramp)  # keep the trampoline alive
        check(lib().gr4pm_packet_receiver_set_symbol_pdu_callback(self._h, self._pdu_cb, None), "set_symbol_pdu_callback")

    def publish_symbol_pdus(self, header_endpoint="tcp://*:5000", payload_endpoint="tcp://*:5001"):
        """`zmq_output` of packet_receiver.hpp:159-189: collect() publishes every complete header PDU (128 symbols) on
        header_endpoint and every payload PDU on payload_endpoint, one ZeroMQ message of raw complex64 each
        (zmq_pdu_pub_sink.hpp:31-41; the library speaks ZMTP 3.0 itself).  Returns the two bound TCP ports;
        (None, None) stops publishing."""
        self._pdu_cb = None
        ports = (C.c_int * 2)(0, 0)
        enc = lambda e: None if e is None else e.encode()
        check(lib().gr4pm_packet_receiver_publish_symbol_pdus(self._h, enc(header_endpoint), enc(payload_endpoint), ports),
              "publish_symbol_pdus")
        return int(ports[0]), int(ports[1])

    def process_bulk(self, x, header_fn=None, tags_cap=None, history=None, next_x=None):
        """same calling convention as PacketReceiver.process_bulk (header_fn: None or a constant
        packet_length); pipelined: returns the result of an earlier batch, None while filling"""
        self.submit(x, header_fn, history, next_x)
        depth = 5 if self.decode_headers else (4 if self.soft_bits else 3)  # stages behind the detector
        if not self.pipelined or lib().gr4pm_packet_receiver_inflight(self._h) > depth:
            return self.collect()
        return None

    def flush(self):
        out = []
        while lib().gr4pm_packet_receiver_inflight(self._h):
            out.append(self.collect())
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release("gr4pm_packet_receiver_destroy", self._h)
                self._h = None
        except Exception:  # interpreter shutdown
            pass


class ZmqPduPubSink:
    """zmq_pdu_pub_sink.hpp:11-44: a ZeroMQ PUB socket bound to `endpoint`, one message per PDU holding its raw items
    (gr4pm_zmq_pub_*: ZMTP 3.0 in the library, no libzmq; host only -- works without a GPU)"""

    def __init__(self, endpoint="tcp://*:5555"):
        h = C.c_void_p()
        check(lib().gr4pm_zmq_pub_create(endpoint.encode(), C.byref(h)), "ZmqPduPubSink")
        self._h = h

    @property
    def port(self):
        return int(lib().gr4pm_zmq_pub_port(self._h))

    @property
    def subscribers(self):
        return int(lib().gr4pm_zmq_pub_subscribers(self._h))

    @property
    def dropped(self):
        return int(lib().gr4pm_zmq_pub_dropped(self._h))

    def process_one(self, data):
        """data: the PDU's items (any contiguous numpy array or bytes)"""
        buf = np.ascontiguousarray(data) if not isinstance(data, (bytes, bytearray)) else np.frombuffer(bytes(data), dtype=np.uint8)
        check(lib().gr4pm_zmq_pub_send(self._h, buf.ctypes.data_as(C.c_void_p), buf.nbytes), "ZmqPduPubSink.process_one")

    def close(self):
        if getattr(self, "_h", None):
            lib().gr4pm_zmq_pub_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass
