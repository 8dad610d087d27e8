"""python -m obs_rvc_amd.build_index <wav-dir-or-files...> -o added.index [--version 2] [--window 3.0] [--max-rows N] [--reduce-to N] [--resampler blocks|device]

Upstream's "train feature index" with this engine: ContentVec over a voice's recordings on the GPU, the frames stacked in HBM
(RvcInfer.build_index), reduced by k-means when there are too many, an IVF structure trained, and the result written as a Faiss file upstream reads
(RvcInfer.save_index).  WAV files are read with the standard library: PCM, 16-bit or 32-bit integer, mono or stereo (mixed down).  Argument parsing and
WAV decoding are plain functions; only main() touches the GPU."""
from __future__ import annotations

import argparse
import os
import sys
import wave

import numpy as np


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m obs_rvc_amd.build_index", description="build a voice's retrieval index from WAV recordings on the GPU")
    p.add_argument("inputs", nargs="+", help="WAV files, or directories searched (not recursively) for *.wav")
    p.add_argument("-o", "--output", required=True, help="the Faiss index file to write (added_*.index)")
    p.add_argument("--data", default=None, help="the engine's data directory (contentvec/...); default: the model zoo of the package")
    p.add_argument("--version", type=int, choices=(1, 2), default=2, help="RVC model version: 1 = 256-dim layer-9 features, 2 = 768-dim layer-12 (default)")
    p.add_argument("--window", type=float, default=3.0, help="seconds of audio per ContentVec run (default 3.0)")
    p.add_argument("--max-rows", type=int, default=0, help="reduce by k-means above this many rows (default: upstream's 200000)")
    p.add_argument("--reduce-to", type=int, default=0, help="k-means centres kept when reducing (default: upstream's 10000)")
    p.add_argument("--resampler", choices=("blocks", "device"), default="blocks",
                   help="route of a recording to 16 kHz: blocks = the streaming converter block by block (default), device = the whole-signal converter")
    p.add_argument("--device", type=int, default=-1)
    a = p.parse_args(argv)
    if not a.window > 0:
        p.error("--window must be positive")
    if a.max_rows < 0 or a.reduce_to < 0:
        p.error("--max-rows and --reduce-to are row counts")
    return a


def wav_files(inputs) -> list:
    """the WAV files the arguments name: a file as it is, a directory's *.wav entries in name order"""
    out = []
    for path in inputs:
        if os.path.isdir(path):
            out += [os.path.join(path, f) for f in sorted(os.listdir(path)) if f.lower().endswith(".wav")]
        else:
            out.append(path)
    return out


def read_wav(path) -> tuple:
    """-> (samples float32 in [-1, 1), mono; sample rate).  16-bit samples are divided by 2^15, 32-bit by 2^31; the channels of a frame are averaged."""
    with wave.open(os.fspath(path), "rb") as w:
        ch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        if w.getcomptype() != "NONE":
            raise ValueError("%s: compressed WAV is not supported" % path)
        raw = w.readframes(n)
    if width == 2:
        x = np.frombuffer(raw, "<i2").astype(np.float32) / np.float32(32768.0)
    elif width == 4:
        x = (np.frombuffer(raw, "<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    else:
        raise ValueError("%s: %d-bit samples are not supported (16-bit or 32-bit integer PCM)" % (path, 8 * width))
    if ch < 1 or len(x) % ch:
        raise ValueError("%s: truncated frame" % path)
    if ch > 1:
        x = x.reshape(-1, ch).mean(axis=1, dtype=np.float64).astype(np.float32)
    return x, int(rate)


def main(argv=None) -> int:
    a = parse_args(argv)
    files = wav_files(a.inputs)
    if not files:
        print("no WAV files found", file=sys.stderr)
        return 2
    from . import weights as W
    from .rvc import RvcInfer
    eng = RvcInfer(a.data or W.default_zoo_root("full"), device=a.device)
    eng.load_contentvec(a.version)
    info = eng.build_index((read_wav(f) for f in files), window=int(round(a.window * 16000)), max_rows=a.max_rows, reduce_to=a.reduce_to,
                           resampler=a.resampler)
    eng.save_index(a.output)
    print("%s: %d rows from %d files (%d ContentVec runs, %d rows dropped as non-finite)" % (a.output, info["index_rows"], len(files), info["windows"], info["dropped_nonfinite"]))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
