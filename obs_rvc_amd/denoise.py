"""Streaming spectral-gate noise reduction on host buffers (`rvc_denoiser_*`, csrc/denoise.hip.h; DESIGN.md "Spectral-gate noise reduction"): causal,
10 ms delay, per-stream strength (0 = off: the stream passes undelayed, bit for bit) and threshold."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native
from .rvc_common import RvcInferError


class Denoiser:
    def __init__(self, engine, sample_rate: int, n_streams: int = 1):
        self._L = _native.lib()
        self._engine = engine                      # keeps the engine (device, stream) alive
        h = C.c_void_p()
        self._chk(self._L.rvc_denoiser_create(engine._h, int(sample_rate), int(n_streams), C.byref(h)))
        self._h, self.n_streams, self.sample_rate = h, int(n_streams), int(sample_rate)

    def _chk(self, rc) -> None:
        if int(rc) != 0:
            raise RvcInferError(int(rc), (self._L.rvc_last_error_message(self._engine._h) or b"").decode())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self._engine, "_h", None):
            self._L.rvc_denoiser_destroy(h)

    @property
    def latency(self) -> int:
        """samples of delay of a stream whose strength is > 0 (sample_rate / 100)"""
        return int(self._L.rvc_denoiser_latency(self._h))

    def set(self, strength: float, threshold: float = 2.0, stream: int = None) -> None:
        """strength in [0, 1] (0 = off), threshold in [0, 16]; every stream, or one"""
        self._chk(self._L.rvc_denoiser_set(self._h, -1 if stream is None else int(stream), float(strength), float(threshold)))

    def reset(self) -> None:
        self._L.rvc_denoiser_reset(self._h)

    def process(self, wave_in) -> np.ndarray:
        """(n,) for one stream or (n_streams, n); n a positive multiple of sample_rate / 100 -> the same shape"""
        x = np.ascontiguousarray(wave_in, dtype=np.float32)
        single = x.ndim == 1
        x = x.reshape(1, -1) if single else x
        if x.ndim != 2 or x.shape[0] != self.n_streams:
            raise RvcInferError(5, "expected %d stream(s)" % self.n_streams)
        out = np.empty_like(x)
        fp = C.POINTER(C.c_float)
        self._chk(self._L.rvc_denoiser_process(self._h, x.ctypes.data_as(fp), x.shape[1], out.ctypes.data_as(fp)))
        return out[0] if single else out
