"""Python mirror of the reference's `rvc` crate API (rvc/src/lib.rs:5, rvc/src/rvc.rs:18-220) on top of
the C ABI (include/rvc_mi355x.h).  Same method names, argument meaning and error behaviour as
`rvc::RvcInfer`; numpy arrays stand in for ndarray views.  All compute happens in the HIP library."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native
from .rvc_common import (CREPE_ARGMAX, CREPE_VITERBI, CROSSFADE_LINEAR, CROSSFADE_PHASE_VOCODER, F0_CREPE, F0_CREPE_TINY, F0_FCPE, F0_HYBRID, F0_PM, F0_RMVPE, F0_YIN, HYBRID_MAX_MEMBERS, HYBRID_MEDIAN, HYBRID_VOTE, SCALE_C_MAJOR, SCALE_CHROMATIC, PitchAlgorithm,  # noqa: F401
                         RvcInferError, RvcModelVersion, parse_f0_hybrid, scale_mask)

_FP = C.POINTER(C.c_float)


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(_FP)


class RvcInfer:
    def __init__(self, data_path, device: int = -1):
        """RvcInfer::new (rvc.rs:30-44)."""
        self._L = _native.lib()
        h = C.c_void_p()
        rc = self._L.rvc_create(os.fspath(data_path).encode(), int(device), C.byref(h))
        if rc != 0:
            raise RvcInferError(rc, "rvc_create failed (no HIP device?)")
        self._h = h
        self.n_streams = 1

    # -- lifetime -----------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.rvc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RvcInferError(rc, (self._L.rvc_last_error_message(self._h) or b"").decode())

    # -- loading (rvc.rs:46-79) -------------------------------------------------------------
    def load_contentvec(self, model_version=RvcModelVersion.V2):
        self._chk(self._L.rvc_load_contentvec(self._h, int(RvcModelVersion.from_value(model_version))))

    def load_model(self, model_path):
        self._chk(self._L.rvc_load_model(self._h, os.fspath(model_path).encode()))

    def load_f0(self, pitch_algorithm=PitchAlgorithm.Rmvpe):
        self._chk(self._L.rvc_load_f0(self._h, int(PitchAlgorithm.from_value(pitch_algorithm))))

    _F0_NAMES = {"rmvpe": F0_RMVPE, "yin": F0_YIN, "crepe": F0_CREPE, "crepe-full": F0_CREPE, "crepe-tiny": F0_CREPE_TINY, "fcpe": F0_FCPE, "pm": F0_PM}

    def load_f0_method(self, method):
        """The engine's f0 method: "rmvpe" / F0_RMVPE (loads <data>/f0/rmvpe.rvcw, as load_f0), "yin" / F0_YIN (needs no file), "crepe" = "crepe-full" / F0_CREPE
        (<data>/f0/crepe-full.rvcw), "crepe-tiny" / F0_CREPE_TINY (<data>/f0/crepe-tiny.rvcw) or "fcpe" / F0_FCPE (<data>/f0/fcpe.rvcw), or "pm" / F0_PM (Praat's autocorrelation
        tracker, weight-free as YIN)."""
        if isinstance(method, str):
            members = parse_f0_hybrid(method, self._F0_NAMES)      # "hybrid[rmvpe+fcpe]", the forks' form, under the default mode (load_f0_hybrid)
            if members is not None:
                return self.load_f0_hybrid(members)
            if method.lower() not in self._F0_NAMES:
                raise ValueError("f0 method: 'rmvpe', 'yin', 'crepe' (= 'crepe-full'), 'crepe-tiny', 'fcpe' or 'pm', not %r" % method)
            method = self._F0_NAMES[method.lower()]
        self._chk(self._L.rvc_load_f0_method(self._h, int(method)))

    @property
    def f0_method(self) -> int:
        """0 = none loaded, F0_RMVPE, F0_YIN, F0_CREPE, F0_CREPE_TINY, F0_FCPE, F0_PM, F0_HYBRID"""
        return int(self._L.rvc_f0_method(self._h))

    _HYBRID_MODES = {"vote": HYBRID_VOTE, "median": HYBRID_MEDIAN}

    @classmethod
    def _hybrid_args(cls, methods, mode):
        """load_f0_hybrid's arguments as the C call takes them, checked here first (no device needed): -> ([method ids], mode id)"""
        if isinstance(methods, (str, bytes)) or not 1 <= len(methods) <= HYBRID_MAX_MEMBERS:
            raise ValueError("f0 hybrid: a list of 1 to %d members" % HYBRID_MAX_MEMBERS)
        ids = []
        for m in methods:
            if isinstance(m, str):
                if m.lower() not in cls._F0_NAMES:
                    raise ValueError("f0 hybrid member: 'rmvpe', 'yin', 'crepe' (= 'crepe-full'), 'crepe-tiny', 'fcpe' or 'pm', not %r" % m)
                m = cls._F0_NAMES[m.lower()]
            if int(m) not in cls._F0_NAMES.values():
                raise ValueError("f0 hybrid member: %r is no single f0 method" % (m,))
            ids.append(int(m))
        if len(set(ids)) != len(ids):
            raise ValueError("f0 hybrid: a member is named twice")
        if isinstance(mode, str):
            if mode.lower() not in cls._HYBRID_MODES:
                raise ValueError("f0 hybrid mode: 'vote' or 'median', not %r" % mode)
            mode = cls._HYBRID_MODES[mode.lower()]
        if int(mode) not in (HYBRID_VOTE, HYBRID_MEDIAN):
            raise ValueError("f0 hybrid mode: HYBRID_VOTE or HYBRID_MEDIAN, not %r" % (mode,))
        return ids, int(mode)

    def load_f0_hybrid(self, methods, mode="vote"):
        """Hybrid f0: 1 to 4 distinct members (names or F0_* values; the first is the lead) run on the same audio and combined per frame.  mode "vote" /
        HYBRID_VOTE (the default): a frame is voiced iff most members say so (the lead breaks a tie) and takes the median of the voiced values; "median" /
        HYBRID_MEDIAN: the forks' plain median with unvoiced members entering as 0, which halves f0 where two members disagree on voicing.  Loads every member's
        weights as load_f0_method would; all or nothing."""
        ids, mode = self._hybrid_args(methods, mode)
        self._chk(self._L.rvc_load_f0_hybrid(self._h, (C.c_int * len(ids))(*ids), len(ids), mode))

    def f0_hybrid(self):
        """The hybrid in force as ([F0_* of the members, the lead first], mode), None when the f0 method is no hybrid"""
        m, mode = (C.c_int * HYBRID_MAX_MEMBERS)(), C.c_int()
        n = int(self._L.rvc_f0_hybrid(self._h, m, HYBRID_MAX_MEMBERS, C.byref(mode)))
        return ([int(m[i]) for i in range(n)], int(mode.value)) if n else None

    def set_crepe_decoder(self, decoder):
        """CREPE's decoder: "viterbi" / CREPE_VITERBI (the default) or "argmax" / CREPE_ARGMAX; engine-wide"""
        if isinstance(decoder, str):
            if decoder.lower() not in ("viterbi", "argmax"):
                raise ValueError("crepe decoder: 'viterbi' or 'argmax', not %r" % decoder)
            decoder = {"viterbi": CREPE_VITERBI, "argmax": CREPE_ARGMAX}[decoder.lower()]
        self._chk(self._L.rvc_set_crepe_decoder(self._h, int(decoder)))

    @property
    def crepe_decoder(self) -> int:
        return int(self._L.rvc_crepe_decoder(self._h))

    def set_fcpe_threshold(self, threshold: float):
        """FCPE's voicing threshold in [0, 1): f0 = 0 where a frame's largest posterior is at or below it (default 0.006); engine-wide"""
        self._chk(self._L.rvc_set_fcpe_threshold(self._h, float(threshold)))

    @property
    def fcpe_threshold(self) -> float:
        return float(self._L.rvc_fcpe_threshold(self._h))

    def unload_model(self):
        self._L.rvc_unload_model(self._h)

    def model_has_f0(self):
        """True: the loaded model was trained with pitch guidance; False: without (no f0 method is needed or run, pitch_shift may be None everywhere, the pitch
        controls and protect are ignored); None: no model loaded (rvc_model_has_f0)"""
        v = int(self._L.rvc_model_has_f0(self._h))
        return None if v < 0 else bool(v)

    # -- speakers of a multi-speaker model (rvc_set_speaker*): engine-wide, may change between any two chunks ----
    def speakers(self) -> int:
        """rows of the loaded model's speaker table; 1 for a model without one (its baked speaker, id 0); 0: no model loaded"""
        return int(self._L.rvc_model_speakers(self._h))

    def set_speaker(self, sid: int):
        self._chk(self._L.rvc_set_speaker(self._h, int(sid)))

    def set_speaker_mix(self, mix):
        """{sid: weight, ...} over 1 to 8 speakers: the blend sum_i w_i emb_g[sid_i], weights >= 0 and normalised to sum 1"""
        items = list(dict(mix).items())
        ids = (C.c_int32 * max(len(items), 1))(*[int(k) for k, _ in items])
        ws = (C.c_double * max(len(items), 1))(*[float(v) for _, v in items])
        self._chk(self._L.rvc_set_speaker_mix(self._h, ids, ws, len(items)))

    def speaker_mix(self) -> dict:
        """the mix in force, {sid: normalised weight}"""
        ids, ws, n = (C.c_int32 * 8)(), (C.c_double * 8)(), C.c_size_t()
        self._chk(self._L.rvc_speaker_mix(self._h, ids, ws, 8, C.byref(n)))
        return {int(ids[i]): float(ws[i]) for i in range(n.value)}

    # -- per-chunk API (rvc.rs:81-220) ----------------------------------------------------
    def hubert(self, input):
        """-> (1, C, T) float32 (rvc.rs:81-97)."""
        x, xp = _f32(input)
        dims = (C.c_size_t * 3)()
        cap = 1024 * (len(x) // 320 + 8)
        out = np.empty(cap, np.float32)
        self._chk(self._L.rvc_hubert(self._h, xp, len(x), out.ctypes.data_as(_FP), cap, dims))
        return out[: dims[0] * dims[1] * dims[2]].reshape(dims[0], dims[1], dims[2]).copy()

    def extract_feature(self, input):
        """-> (1, 2T+1, C) float32 (rvc.rs:99-109)."""
        x, xp = _f32(input)
        dims = (C.c_size_t * 3)()
        cap = 1024 * (2 * (len(x) // 320) + 16)
        out = np.empty(cap, np.float32)
        self._chk(self._L.rvc_extract_feature(self._h, xp, len(x), out.ctypes.data_as(_FP), cap, dims))
        return out[: dims[0] * dims[1] * dims[2]].reshape(dims[0], dims[1], dims[2]).copy()

    def pitch(self, input, pitch_shift: int, sample_frame_16k_size: int):
        """-> f0 in Hz, one value per RMVPE frame (rvc.rs:111-131)."""
        x, xp = _f32(input)
        n = C.c_size_t()
        out = np.empty(4096, np.float32)
        self._chk(self._L.rvc_pitch(self._h, xp, len(x), int(pitch_shift), int(sample_frame_16k_size), out.ctypes.data_as(_FP), 4096, C.byref(n)))
        return out[: n.value].copy()

    def infer(self, input, sample_frame_16k_size: int, pitch_shift, skip_head: int, return_length: int):
        """-> float PCM at the model rate (rvc.rs:133-220).  pitch_shift=None mirrors Option::None."""
        x, xp = _f32(input)
        n = C.c_size_t()
        cap = int(return_length) * 1024 + 16
        out = np.empty(cap, np.float32)
        self._chk(self._L.rvc_infer(self._h, xp, len(x), int(sample_frame_16k_size), 0 if pitch_shift is None else 1, int(pitch_shift or 0),
                                    int(skip_head), int(return_length), out.ctypes.data_as(_FP), cap, C.byref(n)))
        return out[: n.value].copy()

    # -- extensions ---------------------------------------------------------------------
    def load_index(self, vectors, nprobe=None, train=False, k=None):
        """`vectors`: an (n, dim) float32 array, or the path of a Faiss `.index` file (IndexFlat / IndexIVFFlat: the stored
        vectors are reconstructed in id order, obs_rvc_amd.faiss_index) or of a `.npy` matrix (upstream's total_fea.npy).
        `nprobe`: None = the flat search over every row; an integer >= 1 = keep an IndexIVFFlat file's structure and search it as upstream
        does, that many nearest lists per query (rvc_set_index_ivf + rvc_set_index_nprobe); "file" = the nprobe the file stores.  A source
        without an IVF structure (an array, a .npy matrix, a flat file) with nprobe >= 1 or "file" raises the RVC_SHAPE error (NdarrayShapeError)
        before anything is loaded: the engine keeps the index it had.
        `train`: True, or a dict of train_index_ivf's arguments (nlist, iters, init_rows, seed): with `nprobe` given, a source without a structure is trained
        on the device after loading (k-means, rvc_train_index_ivf) instead of refused; "file" then means 1, upstream's stored value.  A file's own structure is
        kept as it is.  False (the default): everything above.
        `k`: neighbours blended per query.  None leaves the engine's value (4 unless set_index_k changed it); 4 or 8; "upstream" = 8, what upstream's
        pipelines search with.  Set before the load, so an index of fewer than k rows is refused and the engine keeps the index it had (and its k)."""
        if k is not None:
            if isinstance(k, str) and k != "upstream":
                raise ValueError('k is 4, 8 or "upstream"')
            k = 8 if k == "upstream" else int(k)
            if k not in (4, 8):
                raise RvcInferError(5, "k must be 4 or 8")
        centroids = assign = None
        stored = 0
        if isinstance(vectors, (str, os.PathLike)):
            path = os.fspath(vectors)
            if path.endswith(".npy"):
                vectors = np.load(path)
            elif nprobe is None:
                from .faiss_index import read_index
                vectors = read_index(path)
            else:
                from .faiss_index import read_index_ivf
                vectors, centroids, assign, stored = read_index_ivf(path, with_nprobe=True)
        if nprobe is not None:
            # decided before anything is loaded, so that a refused call leaves the engine's index as it was: a source without an IVF structure (an array,
            # a .npy matrix, a flat file) has no lists to probe and no stored value -- the engine's own RVC_SHAPE error for nprobe >= 1 without a structure
            if isinstance(nprobe, str) and nprobe != "file":
                raise ValueError('nprobe is an integer or "file"')
            if centroids is None and not train and (nprobe == "file" or int(nprobe) >= 1):
                raise RvcInferError(5, "nprobe >= 1 needs an IVF structure: the index source has none")
            if centroids is None and train and nprobe == "file":
                stored = 1
            nprobe = int(stored) if nprobe == "file" else int(nprobe)
            if not 0 <= nprobe <= 64:
                raise RvcInferError(5, "nprobe must be in [0, 64]")
        v, vp = _f32(vectors)
        if k is not None and v.shape[0] < k:
            raise RvcInferError(5, "index needs at least %d vectors" % k)
        if k is not None and k < self.index_k():
            self.set_index_k(k)          # (lowering never fails; raising waits for the new index, which has the rows for it)
        self._chk(self._L.rvc_load_index(self._h, vp, v.shape[0], v.shape[1]))
        self._index_shape = (int(v.shape[0]), int(v.shape[1]))
        if k is not None:
            self.set_index_k(k)
        if nprobe is not None:
            if centroids is not None:
                self.set_index_ivf(centroids, assign)
            elif train and nprobe >= 1:
                self.train_index_ivf(**(train if isinstance(train, dict) else {}))
            self.set_index_nprobe(nprobe)

    def set_index_ivf(self, centroids, assign):
        """rvc_set_index_ivf: attach an IVF structure to the loaded index: `centroids` (nlist, dim) float32, `assign` (n,) the list of every row."""
        c, cp = _f32(centroids)
        a = np.ascontiguousarray(assign, np.int32)
        self._chk(self._L.rvc_set_index_ivf(self._h, cp, c.shape[0], c.shape[1], a.ctypes.data_as(C.POINTER(C.c_int32)), a.shape[0]))

    def set_index_nprobe(self, k: int):
        """rvc_set_index_nprobe: 0 = flat search, 1..64 = probe that many lists of the attached IVF structure (clamped to its nlist)."""
        self._chk(self._L.rvc_set_index_nprobe(self._h, int(k)))

    def index_nprobe(self) -> int:
        return int(self._L.rvc_index_nprobe(self._h))

    def set_index_k(self, k: int):
        """rvc_set_index_k: neighbours blended per query, 4 (the default) or 8 (upstream's).  Engine-wide; kept across index loads."""
        self._chk(self._L.rvc_set_index_k(self._h, int(k)))

    def index_k(self) -> int:
        return int(self._L.rvc_index_k(self._h))

    def index_ivf_info(self):
        """(nlist, rows of the longest list, empty lists) of the attached IVF structure"""
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._chk(self._L.rvc_index_ivf_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def train_index_ivf(self, nlist=None, iters: int = 10, init_rows=None, seed: int = 0, nprobe=None) -> dict:
        """rvc_train_index_ivf: k-means over the loaded index on the device, the result attached as set_index_ivf would.  nlist None = upstream's rule
        min(floor(16 sqrt(n)), n // 39); init_rows None = the seeded sample.  nprobe given: set after training (training itself returns it to 0).
        -> {nlist, longest_list, empty_lists, iters_run, moved_last, objective: [...], ms_assign, ms_update, ms_total}"""
        rows = None if init_rows is None else np.ascontiguousarray(init_rows, np.int32)
        if rows is not None and (rows.ndim != 1 or nlist not in (None, 0, rows.shape[0])):
            raise RvcInferError(5, "init_rows: one row number per list")
        self._chk(self._L.rvc_train_index_ivf(self._h, int(nlist or 0) if rows is None else rows.shape[0], int(iters),
                                              None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_int32)), int(seed) & 0xffffffff))
        if nprobe is not None:
            self.set_index_nprobe(nprobe)
        return self.index_ivf_train_info()

    def index_ivf_train_info(self) -> dict:
        """rvc_index_ivf_train_info + rvc_index_ivf_info of the last training on this engine"""
        it, moved, n_obj = C.c_int(), C.c_size_t(), C.c_size_t()
        obj, ms = (C.c_double * 101)(), (C.c_double * 3)()
        self._chk(self._L.rvc_index_ivf_train_info(self._h, C.byref(it), C.byref(moved), obj, 101, C.byref(n_obj), ms))
        nl, longest, empty = self.index_ivf_info()
        return {"nlist": nl, "longest_list": longest, "empty_lists": empty, "iters_run": it.value, "moved_last": moved.value,
                "objective": [obj[i] for i in range(n_obj.value)], "ms_assign": ms[0], "ms_update": ms[1], "ms_total": ms[2]}

    def _index_dims(self):
        """(n, dim) of the loaded index: noted by load_index / index_broadcast, checked against the bytes the engine holds"""
        shape = getattr(self, "_index_shape", None)
        _, nbytes = self.index_device_ptr()
        if not shape or shape[0] * shape[1] * 4 != nbytes:
            raise RvcInferError(5, "the shape of the loaded index is not known to this object (load it with load_index, or broadcast with vectors / expect)")
        return shape

    def index_ivf(self):
        """rvc_get_index_ivf: the attached structure, trained or set -> (centroids (nlist, dim) float32, assign (n,) int32)"""
        n, dim = self._index_dims()
        nlist = self.index_ivf_info()[0]
        cent, assign = np.empty((nlist, dim), np.float32), np.empty(n, np.int32)
        self._chk(self._L.rvc_get_index_ivf(self._h, cent.ctypes.data_as(_FP), cent.size, assign.ctypes.data_as(C.POINTER(C.c_int32)), n))
        return cent, assign

    def index_vectors(self) -> np.ndarray:
        """the loaded index (n, dim) copied back from the device (export: save_index)"""
        n, dim = self._index_dims()
        p, nbytes = self.index_device_ptr()
        out = np.empty((n, dim), np.float32)
        self.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rc = hip.hipMemcpy(out.ctypes.data, p, nbytes, 2)                 # hipMemcpyDeviceToHost
        if rc != 0:
            raise RvcInferError(4, "hipMemcpy of the index failed (%d)" % rc)
        return out

    def save_index(self, path):
        """Write the loaded index as a Faiss file upstream reads: an IndexIVFFlat with the attached structure (trained or set) and the engine's nprobe (1 while
        the search is flat), or an IndexFlat when no structure is attached."""
        from . import faiss_index as F
        v = self.index_vectors()
        try:
            cent, assign = self.index_ivf()
        except RvcInferError:
            F.write_flat(os.fspath(path), v)
            return
        F.write_ivf_flat_assigned(os.fspath(path), v, cent, assign, nprobe=max(1, self.index_nprobe()))

    # -- index builder (rvc_index_build_*) ---------------------------------
    def index_build_begin(self, window: int = 0, capacity_hint: int = 0):
        """rvc_index_build_begin: open a build; window in 16 kHz samples (0 = 48 000), capacity_hint in rows (0 = 4096)."""
        self._chk(self._L.rvc_index_build_begin(self._h, int(window), int(capacity_hint)))

    def index_build_add(self, pcm16k) -> int:
        """rvc_index_build_add: the ContentVec frames of one 16 kHz recording as rows of the open build -> rows added"""
        x, xp = _f32(pcm16k)
        if x.ndim != 1:
            raise RvcInferError(5, "index build: a recording is a 1-D array")
        n = C.c_size_t()
        self._chk(self._L.rvc_index_build_add(self._h, xp, len(x), C.byref(n)))
        return int(n.value)

    def index_build_info(self) -> dict:
        """rvc_index_build_info of the open build -> {rows, capacity, windows, dropped_nonfinite, ms_contentvec, ms_append, ms_reduce}"""
        r, c, w, d = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        ms = (C.c_double * 3)()
        self._chk(self._L.rvc_index_build_info(self._h, C.byref(r), C.byref(c), C.byref(w), C.byref(d), ms))
        return {"rows": r.value, "capacity": c.value, "windows": w.value, "dropped_nonfinite": d.value,
                "ms_contentvec": ms[0], "ms_append": ms[1], "ms_reduce": ms[2]}

    def index_build_finish(self, max_rows: int = 0, reduce_to: int = 0, iters: int = 10, seed: int = 0) -> int:
        """rvc_index_build_finish: install the build as the engine's index (k-means reduction above max_rows; 0, 0 = upstream's 200 000 -> 10 000)
        -> rows of the installed index"""
        rows = self.index_build_info()["rows"]
        self._chk(self._L.rvc_index_build_finish(self._h, int(max_rows), int(reduce_to), int(iters), int(seed) & 0xffffffff))
        n = (int(reduce_to) or 10000) if rows > (int(max_rows) or 200000) else rows        # (the rule of the C entry point)
        _, nbytes = self.index_device_ptr()
        self._index_shape = (n, nbytes // (4 * n))
        return n

    def index_build_abort(self):
        self._L.rvc_index_build_abort(self._h)

    def build_index(self, recordings, window=None, max_rows=None, reduce_to=None, iters: int = 10, seed: int = 0, train: bool = True, nprobe: int = 1,
                    resampler: str = "blocks") -> dict:
        """Build this voice's index from its recordings on the device and install it.  `recordings`: an iterable of 1-D float arrays at 16 kHz, or of
        (array, rate) pairs; a pair whose rate is not 16 000 goes through the package's resampler (resample.FftFixedInOut, one call over the whole
        recording) first, or with resampler="device" through resample() (one launch).  window in 16 kHz samples (None = 48 000).  train=True: ends with train_index_ivf() (upstream's nlist rule, the same iters and
        seed) and sets nprobe.  -> the index_build_info fields as they stood before the build closed, "index_rows" = rows of the installed index, and
        "ivf" = train_index_ivf's report when trained."""
        if resampler not in ("blocks", "device"):
            raise ValueError("resampler: 'blocks' or 'device', not %r" % (resampler,))
        self.index_build_begin(window or 0, 0)
        try:
            for rec in recordings:
                rate = 16000
                if isinstance(rec, tuple):
                    rec, rate = rec
                x = np.ascontiguousarray(rec, np.float32)
                if x.ndim != 1:
                    raise RvcInferError(5, "index build: a recording is a 1-D array")
                if int(rate) != 16000 and len(x):
                    x = self._to_16k(x, int(rate)) if resampler == "blocks" else self.resample(x, int(rate), 16000)
                self.index_build_add(x)
            info = self.index_build_info()
            info["index_rows"] = self.index_build_finish(max_rows or 0, reduce_to or 0, iters, seed)
        except BaseException:
            self.index_build_abort()
            raise
        if train:
            info["ivf"] = self.train_index_ivf(iters=iters, seed=seed, nprobe=nprobe)
        return info

    def _to_16k(self, x: np.ndarray, rate: int) -> np.ndarray:
        """a whole recording through the package's converter (resample.FftFixedInOut, the plugin's rubato mirror) in blocks of about 20 ms, the last one
        zero-padded and one block of zeros behind it to flush the converter; its start-up delay (half a block) stays in as leading silence"""
        from .resample import FftFixedInOut
        r = FftFixedInOut(self, rate, 16000, max(rate // 50, 1))
        nin = r.input_frames_next()
        nblk = -(-len(x) // nin) + 1
        xp = np.zeros(nblk * nin, np.float32)
        xp[: len(x)] = x
        y = np.concatenate([np.array(r.process(xp[i * nin:(i + 1) * nin]), np.float32) for i in range(nblk)])
        return y[: -(-len(x) * 16000 // rate) + r.output_frames_max() // 2]

    # -- whole-recording conversion (rvc_convert*) ---------------------------
    @staticmethod
    def convert_geometry(n16k: int, sample_rate: int, k: int = 0, context: int = 0, crossfade: int = 0) -> dict:
        """rvc_convert_geometry (host only): the window geometry of a recording of n16k samples for a model at sample_rate; k / context / crossfade in
        10 ms frames, 0 = 14 / 48 / 5 -> {windows, n, sample_frame_16k_size, skip_head, return_length, hop, zc, output_samples}"""
        out = (C.c_size_t * 8)()
        rc = _native.lib().rvc_convert_geometry(int(n16k), int(sample_rate), int(k), int(context), int(crossfade), out)
        if rc != 0:
            raise RvcInferError(rc, "convert geometry out of range")
        return dict(zip(("windows", "n", "sample_frame_16k_size", "skip_head", "return_length", "hop", "zc", "output_samples"), (int(v) for v in out)))

    def convert(self, x, rate: int = 16000, k: int = 0, context: int = 0, crossfade: int = 0, pitch_shift: int = 0, highpass: bool = True):
        """rvc_convert: a whole recording -> (audio at the model's rate, that rate).  The windows run n_streams at a time (set_streams) and are SOLA-stitched on
        the device; the call starts from reset_state().  A rate other than 16 000 goes through the package's converter first, its start-up delay trimmed.
        pitch_shift is the integer, whole-octave shift of infer; set_pitch_semitones transposes by semitones."""
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 1:
            raise RvcInferError(5, "convert: a recording is a 1-D array")
        if int(rate) != 16000 and len(x):
            n16 = -(-len(x) * 16000 // int(rate))
            y = self._to_16k(x, int(rate))
            x = np.ascontiguousarray(y[len(y) - n16:])
        n = C.c_size_t()
        # (the first call sizes the output: a capacity of 0 is short for every recording, empty ones and unloaded models report their own status)
        rc = self._L.rvc_convert(self._h, x.ctypes.data_as(_FP), len(x), int(k), int(context), int(crossfade), int(pitch_shift or 0), 1 if highpass else 0, None, 0, C.byref(n))
        if rc != 5 or n.value == 0:
            self._chk(rc)
        out = np.empty(n.value, np.float32)
        self._chk(self._L.rvc_convert(self._h, x.ctypes.data_as(_FP), len(x), int(k), int(context), int(crossfade), int(pitch_shift or 0), 1 if highpass else 0,
                                      out.ctypes.data_as(_FP), len(out), C.byref(n)))
        # n_out = ceil(n / 160) zc samples and the model's rate is 100 zc
        return out[: n.value], 100 * (n.value // -(-len(x) // 160))

    def convert_info(self) -> dict:
        """rvc_convert_info of the last convert -> {windows, batches, offsets (int32 array), ms_highpass, ms_model, ms_stitch, ms_total} (device milliseconds)"""
        w, b = C.c_size_t(), C.c_size_t()
        ms = (C.c_double * 4)()
        self._chk(self._L.rvc_convert_info(self._h, C.byref(w), C.byref(b), None, 0, ms))
        off = np.empty(w.value, np.int32)
        self._chk(self._L.rvc_convert_info(self._h, None, None, off.ctypes.data_as(C.POINTER(C.c_int32)), len(off), None))
        return {"windows": w.value, "batches": b.value, "offsets": off, "ms_highpass": ms[0], "ms_model": ms[1], "ms_stitch": ms[2], "ms_total": ms[3]}

    # -- a file at any rate, with the volume envelope ------------------------
    @staticmethod
    def resample_geometry(rate_in: int, rate_out: int, n_in: int) -> dict:
        """rvc_resample_geometry (host only) -> {o, n, w, n_out} of the whole-signal converter rate_in -> rate_out over n_in samples"""
        out = (C.c_size_t * 4)()
        rc = _native.lib().rvc_resample_geometry(int(rate_in), int(rate_out), int(n_in), out)
        if rc != 0:
            raise RvcInferError(rc, "resample geometry out of range")
        return dict(zip(("o", "n", "w", "n_out"), (int(v) for v in out)))

    def resample(self, x, rate_in: int, rate_out: int):
        """rvc_resample: a whole signal rate_in -> rate_out in one launch (windowed sinc, width 6, rolloff 0.99); ceil(len(x) rate_out / rate_in) samples"""
        x, xp = _f32(x)
        if x.ndim != 1:
            raise RvcInferError(5, "resample: a signal is a 1-D array")
        n = C.c_size_t()
        rc = self._L.rvc_resample(self._h, xp, len(x), int(rate_in), int(rate_out), None, 0, C.byref(n))      # (sizes the output, as convert does)
        if rc != 5 or n.value == 0:
            self._chk(rc)
        out = np.empty(n.value, np.float32)
        self._chk(self._L.rvc_resample(self._h, xp, len(x), int(rate_in), int(rate_out), out.ctypes.data_as(_FP), len(out), C.byref(n)))
        return out

    def change_rms(self, src, rate_src: int, y, rate_y: int, rate: float):
        """rvc_change_rms (upstream's rms_mix_rate): the copy of `y` (at rate_y) that takes on the volume envelope of `src` (at rate_src); rate = 1 leaves it as it is,
        rate = 0 gives it the source's envelope"""
        s, sp = _f32(src)
        o = np.array(y, dtype=np.float32, copy=True)
        self._chk(self._L.rvc_change_rms(self._h, sp, len(s), int(rate_src), o.ctypes.data_as(_FP), len(o), int(rate_y), float(rate)))
        return o

    def convert_file(self, x, rate: int, k: int = 0, context: int = 0, crossfade: int = 0, pitch_shift: int = 0, highpass: bool = True, rms_mix_rate: float = 1.0,
                     out_rate: int = 0):
        """rvc_convert_file: a recording at `rate` -> (audio, its rate): resampled to 16 kHz, converted as convert() does, given the input's volume envelope
        (rms_mix_rate below 1), resampled to out_rate (0 = the model's) -- all on the device, one upload and one download.  convert_file_info() has the peak."""
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 1:
            raise RvcInferError(5, "convert_file: a recording is a 1-D array")
        n = C.c_size_t()
        a = (x.ctypes.data_as(_FP), len(x), int(rate), int(k), int(context), int(crossfade), int(pitch_shift or 0), 1 if highpass else 0, float(rms_mix_rate), int(out_rate))
        rc = self._L.rvc_convert_file(self._h, *a, None, 0, C.byref(n))
        if rc != 5 or n.value == 0:
            self._chk(rc)
        out = np.empty(n.value, np.float32)
        self._chk(self._L.rvc_convert_file(self._h, *a, out.ctypes.data_as(_FP), len(out), C.byref(n)))
        return out[: n.value], self.convert_file_info()["rate"]

    def convert_file_info(self) -> dict:
        """rvc_convert_file_info of the last convert_file -> {ms_resample_in, ms_highpass, ms_model, ms_stitch, ms_envelope, ms_resample_out, ms_total (device
        milliseconds), rate (of the output), peak (max |audio|, exact)}"""
        ms = (C.c_double * 7)()
        rate, peak = C.c_size_t(), C.c_float()
        self._chk(self._L.rvc_convert_file_info(self._h, ms, C.byref(rate), C.byref(peak)))
        d = dict(zip(("ms_resample_in", "ms_highpass", "ms_model", "ms_stitch", "ms_envelope", "ms_resample_out", "ms_total"), (float(v) for v in ms)))
        d["rate"], d["peak"] = int(rate.value), np.float32(peak.value)
        return d

    def sola_stitch(self, windows, sola_len: int, search: int, frame: int):
        """rvc_sola_stitch: the chained LINEAR sola_step over windows (n_windows, window_len), the tail starting as zeros -> (audio (n_windows * frame,),
        offsets (n_windows,) int32)"""
        y, yp = _f32(windows)
        if y.ndim != 2:
            raise RvcInferError(5, "sola_stitch: windows is an (n_windows, window_len) array")
        out = np.empty(y.shape[0] * int(frame), np.float32)
        off = np.empty(y.shape[0], np.int32)
        self._chk(self._L.rvc_sola_stitch(self._h, yp, y.shape[0], y.shape[1], int(sola_len), int(search), int(frame), out.ctypes.data_as(_FP),
                                          off.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, off

    # -- many recordings in one call (rvc_convert_many*) ----------------------
    @staticmethod
    def convert_many_geometry(lengths, sample_rate: int, k: int = 0, context: int = 0, crossfade: int = 0) -> dict:
        """rvc_convert_many_geometry (host only): the packing of recordings of `lengths` samples at 16 kHz for a model at sample_rate ->
        {windows (per file), output_samples (per file), windows_total, output_total}"""
        n = [int(v) for v in lengths]
        if any(v < 0 for v in n):
            raise RvcInferError(5, "convert_many geometry out of range")
        F = len(n)
        arr = (C.c_size_t * max(F, 1))(*n)
        w, o, tot = (C.c_size_t * max(F, 1))(), (C.c_size_t * max(F, 1))(), (C.c_size_t * 2)()
        rc = _native.lib().rvc_convert_many_geometry(arr, F, int(sample_rate), int(k), int(context), int(crossfade), w, o, tot)
        if rc != 0:
            raise RvcInferError(rc, "convert_many geometry out of range")
        return {"windows": [int(v) for v in w[:F]], "output_samples": [int(v) for v in o[:F]], "windows_total": int(tot[0]), "output_total": int(tot[1])}

    def convert_many(self, signals, k: int = 0, context: int = 0, crossfade: int = 0, pitch_shift: int = 0, highpass: bool = True):
        """rvc_convert_many: a list of 16 kHz recordings -> a list of arrays at the model's rate, one per recording in the order given.  One geometry and one set
        of settings for all; the windows of all recordings are laid end to end and run n_streams at a time, so short recordings share batches.  The call
        starts from reset_state().  Refused while auto-transpose is in force or an f0 curve is set; a pitch per recording: set_convert_many_pitch /
        set_convert_many_auto_transpose."""
        xs = [np.ascontiguousarray(x, np.float32) for x in signals]
        if any(x.ndim != 1 for x in xs):
            raise RvcInferError(5, "convert_many: a recording is a 1-D array")
        F = len(xs)
        pin = (_FP * max(F, 1))(*[x.ctypes.data_as(_FP) for x in xs])
        n = (C.c_size_t * max(F, 1))(*[len(x) for x in xs])
        lens = (C.c_size_t * max(F, 1))()
        a = (int(k), int(context), int(crossfade), int(pitch_shift or 0), 1 if highpass else 0)
        # (the first call sizes the outputs: no capacities is short for every recording; every other refusal reports its own status)
        rc = self._L.rvc_convert_many(self._h, pin, n, F, *a, None, None, lens)
        if rc != 5 or F == 0 or any(lens[f] == 0 for f in range(F)):
            self._chk(rc)
        outs = [np.empty(lens[f], np.float32) for f in range(F)]
        pout = (_FP * F)(*[o.ctypes.data_as(_FP) for o in outs])
        cap = (C.c_size_t * F)(*[len(o) for o in outs])
        self._chk(self._L.rvc_convert_many(self._h, pin, n, F, *a, pout, cap, lens))
        self._many_n = F      # (how many files convert_many_pitch_info reads by default)
        return outs

    def convert_many_info(self) -> dict:
        """rvc_convert_many_info of the last convert_many -> {windows, batches, offsets (int32 array, global window order), ms_highpass, ms_model, ms_stitch,
        ms_total} (device milliseconds)"""
        w, b = C.c_size_t(), C.c_size_t()
        ms = (C.c_double * 4)()
        self._chk(self._L.rvc_convert_many_info(self._h, C.byref(w), C.byref(b), None, 0, ms))
        off = np.empty(w.value, np.int32)
        self._chk(self._L.rvc_convert_many_info(self._h, None, None, off.ctypes.data_as(C.POINTER(C.c_int32)), len(off), None))
        return {"windows": w.value, "batches": b.value, "offsets": off, "ms_highpass": ms[0], "ms_model": ms[1], "ms_stitch": ms[2], "ms_total": ms[3]}

    # -- a pitch per recording for convert_many -----------------------------
    def analyze_f0_many(self, signals, window: int = 0, context: int = 0, crossfade: int = 0, highpass: bool = True) -> list:
        """rvc_analyze_f0_many: analyze_f0 of every recording of a list in one call -- the windows of all of them share batches, as convert_many's -> a list of
        float32 arrays, one per recording, each what analyze_f0 gives that recording alone"""
        xs = [np.ascontiguousarray(x, np.float32) for x in signals]
        if any(x.ndim != 1 for x in xs):
            raise RvcInferError(5, "analyze_f0_many: a recording is a 1-D array")
        F = len(xs)
        outs = [np.empty(-(-len(x) // 160), np.float32) for x in xs]
        pin = (_FP * max(F, 1))(*[x.ctypes.data_as(_FP) for x in xs])
        pout = (_FP * max(F, 1))(*[o.ctypes.data_as(_FP) for o in outs])
        n = (C.c_size_t * max(F, 1))(*[len(x) for x in xs])
        cap = (C.c_size_t * max(F, 1))(*[len(o) for o in outs])
        rows = (C.c_size_t * max(F, 1))()
        self._chk(self._L.rvc_analyze_f0_many(self._h, pin, n, F, int(window), int(context), int(crossfade), 1 if highpass else 0, pout, cap, rows))
        return [o[: rows[f]] for f, o in enumerate(outs)]

    def f0_stats_many(self, rows_list, quantiles=(0.5,)):
        """rvc_f0_stats_many: f0_stats of every array of a list in one launch -> (float32 array (files, quantiles), list of voiced counts)"""
        xs = [np.ascontiguousarray(x, np.float32) for x in rows_list]
        if any(x.ndim != 1 for x in xs):
            raise RvcInferError(5, "f0_stats_many: one-dimensional arrays of Hz")
        q = self._quantiles(quantiles)
        F = len(xs)
        hz = np.ascontiguousarray(np.concatenate(xs) if F else np.zeros(0, np.float32))
        rows = (C.c_size_t * max(F, 1))(*[len(x) for x in xs])
        out, v = np.zeros((F, len(q)), np.float32), (C.c_size_t * max(F, 1))()
        self._chk(self._L.rvc_f0_stats_many(self._h, hz.ctypes.data_as(_FP), rows, F, q.ctypes.data_as(C.POINTER(C.c_double)), len(q), out.ctypes.data_as(_FP), v))
        return out, [int(v[f]) for f in range(F)]

    def set_convert_many_pitch(self, semitones=None):
        """rvc_set_convert_many_pitch: one transpose in semitones (-24..24) per recording of the next convert_many calls; None or an empty list clears it"""
        st = [] if semitones is None else [float(v) for v in semitones]
        arr = (C.c_double * max(len(st), 1))(*st)
        self._chk(self._L.rvc_set_convert_many_pitch(self._h, arr if st else None, len(st)))

    def set_convert_many_auto_transpose(self, target_hz: float, step: int = 0, limit: float = 12.0):
        """rvc_set_convert_many_auto_transpose: convert_many measures the median f0 of EVERY recording and transposes each onto target_hz (0 = off); step and
        limit as set_auto_transpose's.  Composes with set_convert_many_pitch; set_auto_transpose keeps its meaning (one recording) and stays refused by
        convert_many"""
        self._chk(self._L.rvc_set_convert_many_auto_transpose(self._h, float(target_hz), int(step), float(limit)))

    def convert_many_auto_transpose(self) -> dict:
        t, s, l = C.c_double(), C.c_int(), C.c_double()
        self._chk(self._L.rvc_convert_many_auto_transpose(self._h, C.byref(t), C.byref(s), C.byref(l)))
        return {"target_hz": t.value, "step": s.value, "limit": l.value}

    def convert_many_pitch_info(self, files: int = None) -> dict:
        """rvc_convert_many_pitch_info of the last convert_many that ran the per-file pitch pass -> {median_hz (float32 array), voiced (list), auto_semitones,
        semitones (float64 arrays: a_f and t_f = list + a_f), ms_analysis, ms_select}; files: how many to read (default: those of the last convert_many)"""
        ms = (C.c_double * 2)()
        self._chk(self._L.rvc_convert_many_pitch_info(self._h, None, None, None, None, 0, ms))
        F = int(files) if files is not None else getattr(self, "_many_n", 0)
        m, v, a, t = np.zeros(F, np.float32), (C.c_size_t * max(F, 1))(), np.zeros(F, np.float64), np.zeros(F, np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self._L.rvc_convert_many_pitch_info(self._h, m.ctypes.data_as(_FP), v, a.ctypes.data_as(dp), t.ctypes.data_as(dp), F, None))
        return {"median_hz": m, "voiced": [int(v[f]) for f in range(F)], "auto_semitones": a, "semitones": t, "ms_analysis": ms[0], "ms_select": ms[1]}

    def sola_stitch_many(self, windows, windows_per_file, sola_len: int, search: int, frame: int):
        """rvc_sola_stitch_many: sola_stitch of several files at once.  windows (Wtot, window_len) holds the files' windows end to end, windows_per_file their
        counts; every file's tail starts as zeros -> (audio (Wtot * frame,), offsets (Wtot,) int32), equal to sola_stitch of each file's windows"""
        y, yp = _f32(windows)
        if y.ndim != 2:
            raise RvcInferError(5, "sola_stitch_many: windows is a (windows, window_len) array")
        wpf = [int(v) for v in windows_per_file]
        if any(v < 0 for v in wpf) or sum(wpf) != y.shape[0]:
            raise RvcInferError(5, "sola_stitch_many: windows_per_file does not add up to the number of windows")
        cnt = (C.c_size_t * max(len(wpf), 1))(*wpf)
        out = np.empty(y.shape[0] * int(frame), np.float32)
        off = np.empty(y.shape[0], np.int32)
        self._chk(self._L.rvc_sola_stitch_many(self._h, yp, cnt, len(wpf), y.shape[1], int(sola_len), int(search), int(frame), out.ctypes.data_as(_FP),
                                               off.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, off

    def highpass(self, pcm16k):
        """rvc_highpass: the converter's 48 Hz zero-phase high-pass (2049-tap FIR) of a 16 kHz signal"""
        x, xp = _f32(pcm16k)
        out = np.empty(len(x), np.float32)
        self._chk(self._L.rvc_highpass(self._h, xp, len(x), out.ctypes.data_as(_FP)))
        return out

    def rccl_unique_id(self) -> bytes:
        """rvc_rccl_unique_id: rank 0 creates the 128-byte ncclUniqueId the host then hands to the other ranks."""
        buf = C.create_string_buffer(128)
        self._chk(self._L.rvc_rccl_unique_id(buf))
        return buf.raw

    def index_broadcast(self, unique_id: bytes, rank: int, world: int, vectors=None, expect=None):
        """rvc_index_broadcast: ONE ncclBroadcast of the shared retrieval index from rank 0 into this rank's HBM (RCCL over xGMI).
        Rank 0 passes the (n, dim) matrix (or None to send the index it already holds); the other ranks pass None, optionally with the
        shape they expect (`expect=(n, dim)`: a mismatch with what rank 0 sends makes EVERY rank fail, together)."""
        assert len(unique_id) == 128
        if vectors is not None:
            v, vp = _f32(vectors)
            self._chk(self._L.rvc_index_broadcast(self._h, unique_id, int(rank), int(world), vp, v.shape[0], v.shape[1]))
            self._index_shape = (int(v.shape[0]), int(v.shape[1]))
        else:
            n, dim = expect if expect else (0, 0)
            self._chk(self._L.rvc_index_broadcast(self._h, unique_id, int(rank), int(world), None, int(n), int(dim)))
            self._index_shape = (int(n), int(dim)) if expect else None

    def rccl_available(self) -> bool:
        """rvc_rccl_available: can this process load librccl?  (no communicator is created)"""
        return int(self._L.rvc_rccl_available()) == 0

    def index_broadcast_info(self):
        """rvc_index_broadcast_info -> {ms_comm_init, ms_broadcast, ms_repack, ranks} of this engine's last broadcast"""
        ms = (C.c_double * 3)()
        ranks = C.c_int(0)
        self._chk(self._L.rvc_index_broadcast_info(self._h, ms, C.byref(ranks)))
        return {"ms_comm_init": round(ms[0], 3), "ms_broadcast": round(ms[1], 3), "ms_repack": round(ms[2], 3), "ranks": int(ranks.value)}

    def set_index_rate(self, rate: float):
        self._L.rvc_set_index_rate(self._h, float(rate))

    def knn(self, rows_cap: int = 4096):
        """hits of the last infer: (rows, k) indices and squared distances, k = index_k(); rows = return_length per stream, stream-major, for as many
        streams of a batched call as rows_cap holds whole"""
        k = self.index_k()       # (the last plan was built with it: the setting is part of a plan's identity)
        idx = np.empty((rows_cap, k), np.int32)
        dist = np.empty((rows_cap, k), np.float32)
        rows = C.c_size_t()
        self._chk(self._L.rvc_get_knn(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), dist.ctypes.data_as(_FP), rows_cap, C.byref(rows)))
        return idx[: rows.value].copy(), dist[: rows.value].copy()

    get_knn = knn

    def set_noise_seed(self, seed: int, stream_id: int = 0):
        self._L.rvc_set_noise_seed(self._h, int(seed), int(stream_id))

    def reset_state(self):
        self._L.rvc_reset_state(self._h)

    def set_formant_shift(self, semitones: float, stream: int = None):
        """Formant shift (the plugin's resonance shift, obs-rvc/src/lib.rs:80,103,176) in semitones, -5..5: every stream and the
        default of streams added later, or (stream given) one stream (rvc_set_formant_shift[_stream])."""
        if stream is None:
            self._chk(self._L.rvc_set_formant_shift(self._h, float(semitones)))
        else:
            self._chk(self._L.rvc_set_formant_shift_stream(self._h, int(stream), float(semitones)))

    def set_pitch_semitones(self, st: float, stream: int = None):
        """Transpose in semitones, -24..24, fractions allowed: every stream and the default of streams added later, or (stream given) one
        stream (rvc_set_pitch_semitones[_stream]).  The integer pitch_shift of pitch / infer keeps the reference's whole-octave meaning."""
        if stream is None:
            self._chk(self._L.rvc_set_pitch_semitones(self._h, float(st)))
        else:
            self._chk(self._L.rvc_set_pitch_semitones_stream(self._h, int(stream), float(st)))

    def set_f0_range(self, lo: float, hi: float, stream: int = None):
        """Voiced range in Hz: a voiced f0 row outside [lo, hi] becomes unvoiced; (0, inf) = off (rvc_set_f0_range[_stream])."""
        if stream is None:
            self._chk(self._L.rvc_set_f0_range(self._h, float(lo), float(hi)))
        else:
            self._chk(self._L.rvc_set_f0_range_stream(self._h, int(stream), float(lo), float(hi)))

    def set_f0_median(self, r: int, stream: int = None):
        """Median filter on the f0 rows of a chunk, radius 0..7 (upstream's filter_radius; rvc_set_f0_median[_stream])."""
        if stream is None:
            self._chk(self._L.rvc_set_f0_median(self._h, int(r)))
        else:
            self._chk(self._L.rvc_set_f0_median_stream(self._h, int(stream), int(r)))

    def set_f0_snap(self, mask_or_name, strength: float, stream: int = None):
        """Snap f0 to a scale with a strength in [0, 1]: a 12-bit pitch-class mask (SCALE_CHROMATIC, SCALE_C_MAJOR, scale_mask(root, kind);
        0 = off) or a name "<root> <kind>" such as "C major", "F# minor", "chromatic" (rvc_set_f0_snap[_stream])."""
        if isinstance(mask_or_name, str):
            words = mask_or_name.split()
            if len(words) not in (1, 2):
                raise ValueError("scale: '<root> <kind>' or 'chromatic', not %r" % mask_or_name)
            mask_or_name = scale_mask(0 if len(words) == 1 else words[0], words[-1].lower())
        mask = int(mask_or_name)
        if not 0 <= mask < 1 << 32:
            raise RvcInferError(5, "f0 snap: the pitch-class mask is a 12-bit value")
        if stream is None:
            self._chk(self._L.rvc_set_f0_snap(self._h, mask, float(strength)))
        else:
            self._chk(self._L.rvc_set_f0_snap_stream(self._h, int(stream), mask, float(strength)))

    def set_protect(self, value: float, stream: int = None):
        """Consonant protection (upstream RVC's `protect`), 0..0.5, 0.5 = off: on calls that use the index, unvoiced rows (pitchf < 1) become
        value * blended + (1 - value) * raw ContentVec features.  Every stream and the default of streams added later, or (stream given) one
        stream (rvc_set_protect[_stream])."""
        if stream is None:
            self._chk(self._L.rvc_set_protect(self._h, float(value)))
        else:
            self._chk(self._L.rvc_set_protect_stream(self._h, int(stream), float(value)))

    def set_f0_override(self, stream: int, hz):
        """f0 from outside (rvc_set_f0_override_stream): `hz` rows in Hz for the END of the next f0 window of `stream` -- NaN keeps the tracker's value, 0 is
        unvoiced, else a finite value in (0, 20000]; None or an empty array clears.  The rows replace the tracker's in front of every pitch setting, so they are
        transposed like any f0 (absolute values need pitch_shift 0 and set_pitch_semitones(0)).  Consumed by the stream's next infer call unless
        set_f0_override_hold(True)."""
        if hz is None or len(hz) == 0:
            self._chk(self._L.rvc_set_f0_override_stream(self._h, int(stream), None, 0))
            return
        hz = np.ascontiguousarray(hz, np.float32)
        if hz.ndim != 1:
            raise RvcInferError(5, "f0 override: a one-dimensional array of Hz")
        self._chk(self._L.rvc_set_f0_override_stream(self._h, int(stream), hz.ctypes.data_as(C.POINTER(C.c_float)), len(hz)))

    def set_f0_override_hold(self, hold: bool):
        """False (default): an override is consumed by the next infer call of its stream; True: it stays until cleared (rvc_set_f0_override_hold)"""
        self._chk(self._L.rvc_set_f0_override_hold(self._h, 1 if hold else 0))

    def set_f0_curve(self, t, hz):
        """The f0 curve of the recording convert() / convert_file() convert next (rvc_set_f0_curve; upstream's "f0 curve file"): breakpoints t (seconds, strictly
        increasing) and hz (0 = unvoiced, else up to 20000).  Frames between the first and the last time take the curve instead of the tracker's value; the curve
        is transposed like any f0.  Streaming calls never read it."""
        t, hz = np.ascontiguousarray(t, np.float64), np.ascontiguousarray(hz, np.float32)
        if t.ndim != 1 or t.shape != hz.shape or len(t) < 1:
            raise RvcInferError(5, "f0 curve: two one-dimensional arrays of one length, at least one breakpoint")
        self._chk(self._L.rvc_set_f0_curve(self._h, t.ctypes.data_as(C.POINTER(C.c_double)), hz.ctypes.data_as(C.POINTER(C.c_float)), len(t)))

    def clear_f0_curve(self):
        self._chk(self._L.rvc_set_f0_curve(self._h, None, None, 0))

    def f0_curve_grid(self, n_frames: int) -> np.ndarray:
        """the first n_frames rows of the curve's 10 ms grid as the device builds it, NaN = "keep the tracker's value" (rvc_f0_curve_grid)"""
        out = np.empty(int(n_frames), np.float32)
        self._chk(self._L.rvc_f0_curve_grid(self._h, len(out), out.ctypes.data_as(C.POINTER(C.c_float)), len(out)))
        return out

    def convert_f0(self) -> np.ndarray:
        """the conditioned f0 of the last completed conversion, one value per 10 ms frame of the recording (rvc_convert_f0)"""
        n = C.c_size_t(0)
        self._L.rvc_convert_f0(self._h, None, 0, C.byref(n))
        out = np.empty(max(int(n.value), 1), np.float32)
        self._chk(self._L.rvc_convert_f0(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), len(out), C.byref(n)))
        return out[: int(n.value)]

    # -- f0 analysis, order statistics, auto-transpose ------------------------
    def analyze_f0(self, pcm16k, window: int = 0, context: int = 0, crossfade: int = 0, highpass: bool = True) -> np.ndarray:
        """rvc_analyze_f0: the f0 of a whole 16 kHz recording, one value per 10 ms frame (0 = unvoiced), through convert()'s windows and the pitch-only plan --
        no synthesizer, no voice model needed.  The tracker's own rows: no transpose, no pitch control applies."""
        x = np.ascontiguousarray(pcm16k, np.float32)
        if x.ndim != 1:
            raise RvcInferError(5, "analyze_f0: a recording is a 1-D array")
        out = np.empty(-(-len(x) // 160), np.float32)
        n = C.c_size_t()
        self._chk(self._L.rvc_analyze_f0(self._h, x.ctypes.data_as(_FP), len(x), int(window), int(context), int(crossfade), 1 if highpass else 0,
                                         out.ctypes.data_as(_FP), len(out), C.byref(n)))
        return out[: n.value]

    @staticmethod
    def _quantiles(quantiles):
        q = np.atleast_1d(np.asarray(quantiles, np.float64))
        if q.ndim != 1 or not 1 <= len(q) <= 8 or not np.all((q >= 0.0) & (q <= 1.0)):
            raise RvcInferError(5, "f0_stats: 1 to 8 quantiles in [0, 1]")
        return np.ascontiguousarray(q)

    def f0_stats(self, hz, quantiles=(0.5,)):
        """rvc_f0_stats: exact order statistics of the voiced rows (finite and > 0) of `hz`: quantile p is sorted[floor(p (v - 1))], an element of the input
        (0.5 = the lower median) -> (float32 array per quantile, v); all zeros when nothing is voiced"""
        x = np.ascontiguousarray(hz, np.float32)
        if x.ndim != 1:
            raise RvcInferError(5, "f0_stats: a one-dimensional array of Hz")
        q = self._quantiles(quantiles)
        out, v = np.zeros(len(q), np.float32), C.c_size_t()
        self._chk(self._L.rvc_f0_stats(self._h, x.ctypes.data_as(_FP), len(x), q.ctypes.data_as(C.POINTER(C.c_double)), len(q), out.ctypes.data_as(_FP), C.byref(v)))
        return out, int(v.value)

    def f0_stats_stream(self, stream: int = 0, quantiles=(0.5,)):
        """rvc_f0_stats_stream: the same over the stream's 1024-row pitch cache on the device.  The cache holds conditioned f0 (transposed, filtered): read it
        while the transpose is 0 for the raw median"""
        q = self._quantiles(quantiles)
        out, v = np.zeros(len(q), np.float32), C.c_size_t()
        self._chk(self._L.rvc_f0_stats_stream(self._h, int(stream), q.ctypes.data_as(C.POINTER(C.c_double)), len(q), out.ctypes.data_as(_FP), C.byref(v)))
        return out, int(v.value)

    def set_auto_transpose(self, target_hz: float, step: int = 1, limit: float = 12.0):
        """rvc_set_auto_transpose: convert() / convert_file() measure the recording's median f0 first and transpose it onto target_hz (0 = off; Applio's defaults
        are 155 Hz for a male voice, 255 Hz for a female one).  step 0 = exact, 1 = whole semitones, 12 = whole octaves; limit = the largest transpose, 0..24"""
        self._chk(self._L.rvc_set_auto_transpose(self._h, float(target_hz), int(step), float(limit)))

    def auto_transpose(self) -> dict:
        t, s, l = C.c_double(), C.c_int(), C.c_double()
        self._chk(self._L.rvc_auto_transpose(self._h, C.byref(t), C.byref(s), C.byref(l)))
        return {"target_hz": t.value, "step": s.value, "limit": l.value}

    def auto_transpose_info(self) -> dict:
        """of the last conversion that ran the analysis -> {median_hz (float32), voiced, semitones, ms_analysis, ms_select}"""
        m, v, a, ms = C.c_float(), C.c_size_t(), C.c_double(), (C.c_double * 2)()
        self._chk(self._L.rvc_auto_transpose_info(self._h, C.byref(m), C.byref(v), C.byref(a), ms))
        return {"median_hz": np.float32(m.value), "voiced": int(v.value), "semitones": a.value, "ms_analysis": ms[0], "ms_select": ms[1]}

    # -- the file converter's silence gate (rvc_set_convert_silence, rvc_silence_map) --
    def set_convert_silence(self, threshold_db: float, hang_frames: int = 30):
        """rvc_set_convert_silence: convert(), convert_file(), convert_many(), analyze_f0() and the auto-transpose analysis skip the windows in which no 10 ms frame
        within hang_frames of their returned frames reaches threshold_db (the session gate's measure: 40 ms RMS in dB).  threshold_db <= -60 = off (the
        default).  A skipped window is exact zeros in the stitch and 0 in the f0 rows; the windows that run are compacted into full batches."""
        self._chk(self._L.rvc_set_convert_silence(self._h, float(threshold_db), int(hang_frames)))

    def convert_silence(self) -> dict:
        t, h = C.c_double(), C.c_int()
        self._chk(self._L.rvc_convert_silence(self._h, C.byref(t), C.byref(h)))
        return {"threshold_db": t.value, "hang_frames": h.value, "on": t.value > -60.0}

    def convert_silence_info(self) -> dict:
        """of the last completed call that ran with the gate -> {windows_run, windows_skipped, frames_loud, frames_kept, ms_analysis}"""
        v = [C.c_size_t() for _ in range(4)]
        ms = C.c_double()
        self._chk(self._L.rvc_convert_silence_info(self._h, *[C.byref(x) for x in v], C.byref(ms)))
        d = dict(zip(("windows_run", "windows_skipped", "frames_loud", "frames_kept"), (int(x.value) for x in v)))
        d["ms_analysis"] = ms.value
        return d

    def silence_map(self, x, threshold_db: float, hang_frames: int = 30, k: int = 0, context: int = 0, crossfade: int = 0, sample_rate: int = 16000) -> dict:
        """rvc_silence_map: the gate's analysis of a 16 kHz recording alone (no model needed) -> {loud, kept (bool per 10 ms frame), active (bool per window),
        place (int32 per window: its rank among the active windows, -1 = skipped)}"""
        s, sp = _f32(x)
        if s.ndim != 1:
            raise RvcInferError(5, "silence_map: a recording is a 1-D array")
        geo = self.convert_geometry(len(s), int(sample_rate), int(k), int(context), int(crossfade))
        nf, w = geo["output_samples"] // (int(sample_rate) // 100), geo["windows"]
        loud, kept, act = np.zeros(nf, np.uint8), np.zeros(nf, np.uint8), np.zeros(w, np.uint8)
        place = np.zeros(w, np.int32)
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        self._chk(self._L.rvc_silence_map(self._h, sp, len(s), float(threshold_db), int(hang_frames), int(k), int(context), int(crossfade), int(sample_rate),
                                          u8(loud), u8(kept), nf, u8(act), place.ctypes.data_as(C.POINTER(C.c_int32)), w))
        return {"loud": loud.astype(bool), "kept": kept.astype(bool), "active": act.astype(bool), "place": place}

    @staticmethod
    def formant_geometry(return_length: int, sample_rate: int, semitones: float):
        """-> (R2, upp_res): the decoder's frame count and the resampler's input samples per frame of a formant shift
        (rvc_formant_geometry; host only)."""
        out = (C.c_size_t * 2)()
        rc = _native.lib().rvc_formant_geometry(int(return_length), int(sample_rate), float(semitones), out)
        if rc != 0:
            raise RvcInferError(rc, "formant geometry out of range")
        return int(out[0]), int(out[1])

    def set_streams(self, n: int):
        self._chk(self._L.rvc_set_streams(self._h, int(n)))
        self.n_streams = int(n)

    def infer_batch(self, inputs, sample_frame_16k_size: int, pitch_shift, skip_head: int, return_length: int):
        """inputs (n_streams, n) -> (n_streams, N).  pitch_shift: one int for every stream, or a sequence of n_streams ints (every
        stream of a batch is a caller of its own: rvc_infer_batch_v)."""
        x, xp = _f32(inputs)
        assert x.ndim == 2 and x.shape[0] == self.n_streams
        n = C.c_size_t()
        cap = int(return_length) * 1024 + 16
        out = np.empty((self.n_streams, cap), np.float32)
        if pitch_shift is None:      # (a model without pitch guidance has no use for one)
            pitch_shift = 0
        if np.ndim(pitch_shift) == 0:
            self._chk(self._L.rvc_infer_batch(self._h, xp, x.shape[1], int(sample_frame_16k_size), int(pitch_shift), int(skip_head),
                                              int(return_length), out.ctypes.data_as(_FP), cap, C.byref(n)))
        else:
            sh = np.ascontiguousarray(pitch_shift, dtype=np.int32)
            assert sh.shape == (self.n_streams,)
            self._chk(self._L.rvc_infer_batch_v(self._h, xp, x.shape[1], int(sample_frame_16k_size), sh.ctypes.data_as(C.POINTER(C.c_int32)), int(skip_head),
                                                int(return_length), out.ctypes.data_as(_FP), cap, C.byref(n)))
        return out[:, : n.value].copy()

    def infer_batch_g(self, inputs, sample_frame_16k_size, pitch_shift, skip_head, return_length):
        """rvc_infer_batch_g: one call for n_streams callers that do NOT share a geometry (each argument is a sequence with one entry per
        stream; inputs[s] is that stream's 16 kHz buffer).  -> list of n_streams output arrays"""
        S = self.n_streams
        assert len(inputs) == len(sample_frame_16k_size) == len(skip_head) == len(return_length) == S
        xs = [np.ascontiguousarray(x, dtype=np.float32) for x in inputs]
        caps = [int(r) * 1024 + 16 for r in return_length]
        outs = [np.empty(c, np.float32) for c in caps]
        in_p = (_FP * S)(*[x.ctypes.data_as(_FP) for x in xs])
        out_p = (_FP * S)(*[o.ctypes.data_as(_FP) for o in outs])
        sz = C.c_size_t
        n_a = (sz * S)(*[x.shape[0] for x in xs]); f_a = (sz * S)(*[int(v) for v in sample_frame_16k_size]); cap_a = (sz * S)(*caps); len_a = (sz * S)()
        sh_a = (C.c_uint32 * S)(*[int(v) for v in skip_head]); rl_a = (C.c_uint32 * S)(*[int(v) for v in return_length])
        ps_a = None if pitch_shift is None else (C.c_int32 * S)(*[int(v) for v in pitch_shift])
        self._chk(self._L.rvc_infer_batch_g(self._h, in_p, n_a, f_a, ps_a, sh_a, rl_a, out_p, cap_a, len_a))
        return [o[: len_a[i]].copy() for i, o in enumerate(outs)]

    def infer_device(self, d_in_ptr: int, n: int, sample_frame_16k_size: int, pitch_shift: int, skip_head: int, return_length: int,
                     d_out_ptr: int, cap_per_stream: int, sync: bool = False) -> int:
        nn = C.c_size_t()
        self._chk(self._L.rvc_infer_device(self._h, C.c_void_p(d_in_ptr), int(n), int(sample_frame_16k_size), int(pitch_shift or 0), int(skip_head),
                                           int(return_length), C.c_void_p(d_out_ptr), int(cap_per_stream), C.byref(nn), 1 if sync else 0))
        return nn.value

    def set_pipeline(self, on: bool = True):
        """Offline throughput mode: unsynchronised infer_device calls overlap across chunks (rvc_set_pipeline)."""
        self._L.rvc_set_pipeline(self._h, 1 if on else 0)

    def set_gemm_precision(self, mode: int):
        """EXPLORATORY: 1 = the wide 1-D layers as three bf16 matrix-core products per fp32 product at many streams; 0 = fp32 (default)."""
        self._chk(self._L.rvc_set_gemm_precision(self._h, int(mode)))

    def set_plan_cache(self, n_plans: int):
        """Plans (one per call geometry) the engine keeps; least recently used evicted first (rvc_set_plan_cache)."""
        self._chk(self._L.rvc_set_plan_cache(self._h, int(n_plans)))

    def set_plan_autotune(self, on: bool = True):
        """plans of more than 4 streams pick among the eligible kernels / tiles of every layer by timing them at plan build (default on); False: the rules only"""
        self._chk(self._L.rvc_set_plan_autotune(self._h, 1 if on else 0))

    def plan_autotune_info(self) -> dict:
        """the last plan build: layers tuned by trials / changed against the rules / served from the process cache, ms in trials, ms in all"""
        t, c, h = C.c_int(), C.c_int(), C.c_int()
        tm, bm = C.c_double(), C.c_double()
        self._chk(self._L.rvc_plan_autotune_info(self._h, C.byref(t), C.byref(c), C.byref(h), C.byref(tm), C.byref(bm)))
        return {"tuned": t.value, "changed": c.value, "cache_hits": h.value, "tune_ms": tm.value, "build_ms": bm.value}

    def plan_cache_info(self) -> dict:
        cap, cached, builds = C.c_int(), C.c_int(), C.c_longlong()
        self._L.rvc_plan_cache_info(self._h, C.byref(cap), C.byref(cached), C.byref(builds))
        return {"capacity": cap.value, "cached": cached.value, "builds": builds.value}

    def retrieval_recoveries(self) -> int:
        """Chunks whose retrieval was recomputed through the exhaustive scan after a hand-off time-out (they returned normally)."""
        return int(self._L.rvc_retrieval_recoveries(self._h))

    def synchronize(self):
        self._chk(self._L.rvc_synchronize(self._h))

    def set_use_graph(self, on: bool = True):
        self._L.rvc_set_use_graph(self._h, 1 if on else 0)

    def set_profile(self, on: bool = True):
        self._L.rvc_set_profile(self._h, 1 if on else 0)

    def last_gpu_ms(self) -> float:
        return float(self._L.rvc_last_gpu_ms(self._h))

    def profile_last(self):
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        self._chk(self._L.rvc_profile_last(self._h, C.byref(n), C.byref(ms), C.byref(fl)))
        return n.value, ms.value, fl.value

    def profile_last_knn(self):
        n, ms, by = C.c_int(), C.c_double(), C.c_double()
        self._chk(self._L.rvc_profile_last_knn(self._h, C.byref(n), C.byref(ms), C.byref(by)))
        return n.value, ms.value, by.value

    def enable_taps(self, on=True):
        """True / 1: taps on the explicit plan; 2: taps on the production plan (folded LayerNorms, composed WaveNets); False: off"""
        self._L.rvc_enable_taps(self._h, 2 if on == 2 else (1 if on else 0))

    def plan_ops(self) -> int:
        """kernel launches / copies queued per chunk by the plan of the last call (test aid: which plan ran)"""
        n = C.c_int(0)
        self._L.rvc_debug_last_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        self._L.rvc_debug_last_plan.restype = C.c_int
        assert self._L.rvc_debug_last_plan(self._h, C.byref(n)) == 1
        return int(n.value)

    def tap(self, name: str, stream: int = 0):
        """the named tap of one stream of the last call (enable_taps): stream 0 through rvc_get_tap, any other through the test hook rvc_debug_tap"""
        n = C.c_size_t()
        cap = 1 << 24
        out = np.empty(cap, np.float32)
        if stream == 0:
            self._chk(self._L.rvc_get_tap(self._h, name.encode(), out.ctypes.data_as(_FP), cap, C.byref(n)))
        else:
            self._L.rvc_debug_tap.argtypes = [C.c_void_p, C.c_char_p, C.c_int, _FP, C.c_size_t, C.POINTER(C.c_size_t)]
            self._L.rvc_debug_tap.restype = C.c_int
            self._chk(self._L.rvc_debug_tap(self._h, name.encode(), int(stream), out.ctypes.data_as(_FP), cap, C.byref(n)))
        return out[: n.value].copy()

    def pitch_cache(self, stream: int = 0):
        out = np.zeros(1024, np.float32)
        self._L.rvc_get_pitch_cache(self._h, int(stream), out.ctypes.data_as(_FP))
        return out

    # -- caller-side post-processing (obs-rvc/src/rt_utils.rs) ---------------------------------
    def envelop_mixing(self, input, output, sample_rate: int, mix_rate: float):
        """rt_utils.rs:119-132; returns the mixed copy of `output`."""
        x, xp = _f32(input)
        o = np.array(output, dtype=np.float32, copy=True)
        self._chk(self._L.rvc_envelop_mixing(self._h, xp, o.ctypes.data_as(_FP), len(o), int(sample_rate), float(mix_rate)))
        return o

    def sola_step(self, output, sola_buffer, search: int, frame: int, crossfade: int = 0):
        """rt_utils.rs:60-90 + lib.rs:768-794; returns (offset, frame samples, new sola buffer).  crossfade: CROSSFADE_LINEAR (the
        plugin's sin^2 blend, rvc_sola_step) or CROSSFADE_PHASE_VOCODER (rvc_sola_step_x)."""
        return self.sola_step_full(output, sola_buffer, search, frame, crossfade)[:3]

    def sola_step_full(self, output, sola_buffer, search: int, frame: int, crossfade: int = 0):
        """sola_step that also returns the blended copy of `output`: (offset, frame samples, new sola buffer, output)."""
        o = np.array(output, dtype=np.float32, copy=True)
        sb = np.array(sola_buffer, dtype=np.float32, copy=True)
        fr = np.empty(frame, np.float32)
        off = C.c_size_t()
        if crossfade == CROSSFADE_LINEAR:
            rc = self._L.rvc_sola_step(self._h, o.ctypes.data_as(_FP), len(o), sb.ctypes.data_as(_FP), len(sb), int(search), int(frame),
                                       fr.ctypes.data_as(_FP), C.byref(off))
        else:
            rc = self._L.rvc_sola_step_x(self._h, o.ctypes.data_as(_FP), len(o), sb.ctypes.data_as(_FP), len(sb), int(search), int(frame),
                                         fr.ctypes.data_as(_FP), C.byref(off), int(crossfade))
        self._chk(rc)
        return off.value, fr, sb, o

    def input_gate(self, hist, chunk, sample_rate: int, threshold_db: float):
        """rvc_input_gate: hist = the 3 * (sample_rate // 100) ungated samples before `chunk` -> (gated chunk, next history)."""
        h, hp = _f32(hist)
        x, xp = _f32(chunk)
        if len(h) != 3 * (int(sample_rate) // 100):
            raise RvcInferError(5, "input_gate: the history holds 30 ms")
        out, hist_out = np.empty(len(x), np.float32), np.empty(len(h), np.float32)
        self._chk(self._L.rvc_input_gate(self._h, hp, xp, len(x), int(sample_rate), float(threshold_db), out.ctypes.data_as(_FP), hist_out.ctypes.data_as(_FP)))
        return out, hist_out

    def index_device_ptr(self):
        b = C.c_size_t()
        p = self._L.rvc_index_device_ptr(self._h, C.byref(b))
        return p, b.value
