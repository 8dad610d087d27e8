"""python -m obs_rvc_amd.convert in.wav -o out.wav --model M [--data D] [--version 2] [--f0 rmvpe|yin|crepe-full|crepe-tiny|fcpe|pm|"hybrid[a+b..]" --f0-hybrid-mode vote|median] [--index I --index-rate r --index-k 4|8 --nprobe p]
       [--pitch semitones] [--formant st] [--protect p] [--streams S] [--window k --context C --crossfade X] [--no-highpass] [--rate out_rate]
       [--rms-mix-rate r] [--resampler blocks|device] [--sid N | --sid-mix 0:0.3,2:0.7]
       [--auto-pitch HZ | --auto-pitch-from REF.wav] [--auto-pitch-step 0|1|12] [--auto-pitch-limit st] [--analyze-only --f0-out PATH]

Upstream's "model inference" tab with this engine: a WAV file through RvcInfer.convert -- windows of one geometry run `--streams` at a
time through the batched infer path and are SOLA-stitched on the GPU -- and the result written as 16-bit PCM.  The WAV file is read with
build_index.read_wav and written with the standard library; like upstream the output is divided by peak / 0.99 when its peak exceeds 1.  Argument parsing and
WAV writing are plain functions; only main() touches the GPU.  With --resampler device, or --rms-mix-rate below 1 (upstream's volume envelope), the file goes
through RvcInfer.convert_file instead: both rate conversions and the envelope run on the GPU too, and the peak comes back with the audio.
--auto-pitch / --auto-pitch-from: the recording's median f0 is measured first and transposed onto a target (the forks' "proposed
pitch"); --analyze-only writes the recording's f0 to --f0-out and converts nothing."""
from __future__ import annotations

import argparse
import os
import sys
import wave

import numpy as np

from .build_index import read_wav


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m obs_rvc_amd.convert", description="convert a WAV recording to a voice on the GPU")
    p.add_argument("input", help="the WAV file to convert (16-bit or 32-bit integer PCM, mono or stereo)")
    p.add_argument("-o", "--output", default=None, help="the WAV file to write (16-bit PCM, mono); required unless --analyze-only")
    p.add_argument("--model", default=None, help="the voice: <model>.rvcw (or its .onnx sibling's name); required unless --analyze-only")
    p.add_argument("--data", default=None, help="the engine's data directory (contentvec/, f0/); default: the model zoo of the package")
    p.add_argument("--version", type=int, choices=(1, 2), default=2, help="RVC model version: 1 = 256-dim features, 2 = 768-dim (default)")
    p.add_argument("--f0", type=f0_arg, default="rmvpe", metavar="{%s,hybrid[a+b..]}" % ",".join(F0_CHOICES),
                   help="f0 method (default rmvpe; not loaded for a model without pitch guidance); the CREPE presets are named by their weight files, <data>/f0/crepe-full.rvcw and crepe-tiny.rvcw; fcpe reads <data>/f0/fcpe.rvcw; yin and pm (Praat's autocorrelation tracker) need no file; "
                        "hybrid[rmvpe+fcpe] (quote it) runs 1 to 4 of them and combines their answers per frame, the first member breaking ties")
    p.add_argument("--f0-hybrid-mode", choices=("vote", "median"), default="vote",
                   help="how a hybrid combines: vote = majority voicing, median of the voiced values (default); median = plain median with unvoiced members as 0 (the forks')")
    p.add_argument("--index", default=None, help="retrieval index: a Faiss .index file or a .npy matrix")
    p.add_argument("--index-rate", type=float, default=0.75, help="share of the retrieved features (default 0.75, with --index only)")
    p.add_argument("--index-k", type=int, choices=(4, 8), default=8, help="neighbours blended per frame (default 8, upstream's)")
    p.add_argument("--nprobe", type=int, default=0, help="IVF lists probed per frame; 0 = search every row (default)")
    p.add_argument("--pitch", type=float, default=0.0, help="transpose in semitones, -24..24 (default 0)")
    p.add_argument("--formant", type=float, default=0.0, help="formant shift in semitones, -5..5 (default 0)")
    p.add_argument("--protect", type=float, default=0.5, help="consonant protection, 0..0.5; 0.5 = off (default)")
    p.add_argument("--streams", type=int, default=8, help="windows converted at a time (default 8)")
    p.add_argument("--window", type=int, default=0, help="window size k: a window is 32 k - 1 frames of 10 ms; 2..32 (default 14)")
    p.add_argument("--context", type=int, default=0, help="context frames on each side of a window, >= 3 (default 48)")
    p.add_argument("--crossfade", type=int, default=0, help="crossfade frames between windows, >= 1 (default 5)")
    p.add_argument("--no-highpass", dest="highpass", action="store_false", help="skip the 48 Hz high-pass in front of the model")
    p.add_argument("--rate", type=int, default=0, help="output sample rate (default: the model's)")
    p.add_argument("--rms-mix-rate", type=float, default=1.0, help="volume envelope, 0..1: 0 = the input's envelope, 1 = the model's own (default)")
    p.add_argument("--resampler", choices=("blocks", "device"), default="blocks",
                   help="sample-rate conversion: blocks = the streaming converter block by block (default), device = the whole-signal converter")
    p.add_argument("--sid", type=int, default=None, help="speaker id of a multi-speaker model (default: the speaker baked into the model file)")
    p.add_argument("--sid-mix", default=None, help="a blend of up to 8 speakers as id:weight pairs, e.g. 0:0.3,2:0.7 (weights are normalised)")
    p.add_argument("--f0-file", default=None, metavar="PATH",
                   help="an f0 curve for the recording, upstream's format: one `t,f0` pair per line (seconds, Hz; 0 = unvoiced), blank lines and # comments "
                        "ignored.  Frames between the first and the last time take the curve instead of the tracker's value.  Unlike upstream the curve is "
                        "transposed like any f0: it is absolute only with --pitch 0")
    p.add_argument("--f0-out", default=None, metavar="PATH", help="write the f0 the synthesizer got, one `t,f0` pair per 10 ms frame (the format --f0-file reads)")
    p.add_argument("--auto-pitch", type=float, default=0.0, metavar="HZ",
                   help="auto-transpose: move the recording's median f0 onto HZ (Applio's defaults: 155 for a male voice, 255 for a female one); 0 = off (default)")
    p.add_argument("--auto-pitch-from", default=None, metavar="REF.wav", help="auto-transpose onto the median f0 of a recording of the target voice")
    p.add_argument("--auto-pitch-step", type=int, choices=AUTO_PITCH_STEPS, default=1, help="round the transpose to 1 = whole semitones (default), 12 = whole octaves, 0 = not at all")
    p.add_argument("--auto-pitch-limit", type=float, default=12.0, help="the largest auto-transpose in semitones, 0..24 (default 12)")
    p.add_argument("--analyze-only", action="store_true", help="write the recording's f0 (no transpose, no pitch control) to --f0-out and convert nothing; needs no --model")
    p.add_argument("--skip-silence", type=float, default=None, metavar="DB",
                   help="do not run windows in which nothing reaches DB (40 ms RMS in dB, the live gate's measure; above -60, e.g. -50): they become exact silence")
    p.add_argument("--silence-hang", type=int, default=None, metavar="FRAMES", help="10 ms frames kept on each side of a loud frame, 0..1000 (default 30; with --skip-silence)")
    p.add_argument("--device", type=int, default=-1)
    a = p.parse_args(argv)
    if a.analyze_only:
        if a.f0_out is None:
            p.error("--analyze-only writes the f0 to --f0-out: name the file")
    elif a.model is None or a.output is None:
        p.error("the following arguments are required: -o/--output, --model")
    if not 0.0 <= a.auto_pitch <= 20000.0:
        p.error("--auto-pitch is a frequency in Hz, up to 20000 (0 = off)")
    if a.auto_pitch > 0.0 and a.auto_pitch_from is not None:
        p.error("--auto-pitch and --auto-pitch-from exclude each other")
    if not 0.0 <= a.auto_pitch_limit <= 24.0:
        p.error("--auto-pitch-limit is 0..24 semitones")
    if a.silence_hang is not None and a.skip_silence is None:
        p.error("--silence-hang goes with --skip-silence")
    if a.skip_silence is not None and not -60.0 < a.skip_silence <= 0.0:
        p.error("--skip-silence is a level in dB above -60 and at most 0")
    if a.silence_hang is None:
        a.silence_hang = SILENCE_HANG_DEFAULT
    if not 0 <= a.silence_hang <= 1000:
        p.error("--silence-hang is 0..1000 frames")
    if a.f0_file is not None:
        try:
            with open(a.f0_file) as fh:
                a.f0_curve = parse_f0_curve(fh.read())
        except (OSError, ValueError) as x:
            p.error("--f0-file %s: %s" % (a.f0_file, x))
    else:
        a.f0_curve = None
    if a.sid is not None and a.sid_mix is not None:
        p.error("--sid and --sid-mix exclude each other")
    if a.sid is not None and a.sid < 0:
        p.error("--sid is a speaker id, 0 or more")
    if a.sid_mix is not None:
        try:
            a.sid_mix = parse_sid_mix(a.sid_mix)
        except ValueError as x:
            p.error("--sid-mix: %s" % x)
    if not 0.0 <= a.rms_mix_rate <= 1.0:
        p.error("--rms-mix-rate is 0..1")
    if not -24.0 <= a.pitch <= 24.0:
        p.error("--pitch is -24..24 semitones")
    if not -5.0 <= a.formant <= 5.0:
        p.error("--formant is -5..5 semitones")
    if not 0.0 <= a.protect <= 0.5:
        p.error("--protect is 0..0.5")
    if not 0.0 <= a.index_rate <= 1.0:
        p.error("--index-rate is 0..1")
    if not 1 <= a.streams <= 4096:
        p.error("--streams is 1..4096")
    if not 0 <= a.nprobe <= 64:
        p.error("--nprobe is 0..64")
    if a.window and not 2 <= a.window <= 32:
        p.error("--window is 2..32")
    if a.context and a.context < 3:
        p.error("--context is at least 3")
    if a.crossfade < 0 or a.context < 0:
        p.error("--context and --crossfade are frame counts")
    if a.rate < 0 or a.rate % 100:
        p.error("--rate is a multiple of 100")
    return a


F0_CHOICES = ("rmvpe", "yin", "crepe-full", "crepe-tiny", "fcpe", "pm")
AUTO_PITCH_STEPS = (0, 1, 12)
SILENCE_HANG_DEFAULT = 30


def f0_arg(text: str) -> str:
    """--f0: one of F0_CHOICES, or the forks' hybrid[a+b+..] of 1 to 4 distinct ones (-> lower case, blanks removed); anything else is refused"""
    from .rvc_common import parse_f0_hybrid
    try:
        members = parse_f0_hybrid(text, F0_CHOICES)
    except ValueError as x:
        raise argparse.ArgumentTypeError(str(x))
    if members is not None:
        return "hybrid[%s]" % "+".join(members)
    if text not in F0_CHOICES:
        raise argparse.ArgumentTypeError("invalid choice: %r (choose from %s, or hybrid[a+b..])" % (text, ", ".join(F0_CHOICES)))
    return text


def parse_f0_curve(text: str):
    """upstream's f0 curve file: one `t,f0` pair per line, seconds and Hz; blank lines and # comments (whole lines or trailing) are ignored.  -> (t float64 [n],
    hz float32 [n]) with n >= 1, t strictly increasing, hz 0 or in (0, 20000]: what rvc_set_f0_curve takes.  ValueError names the line"""
    t, hz = [], []
    for no, line in enumerate(text.splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        parts = line.split(",")
        try:
            if len(parts) != 2:
                raise ValueError
            ti, hi = float(parts[0]), float(parts[1])
        except ValueError:
            raise ValueError("line %d: %r is no `t,f0` pair" % (no, line)) from None
        if not np.isfinite(ti) or (t and ti <= t[-1]):
            raise ValueError("line %d: the time %r is not finite or not after the line before" % (no, parts[0].strip()))
        if not 0.0 <= hi <= 20000.0:
            raise ValueError("line %d: the f0 %r is not 0 or in (0, 20000] Hz" % (no, parts[1].strip()))
        t.append(ti); hz.append(hi)
    if not t:
        raise ValueError("no `t,f0` pair")
    return np.asarray(t, np.float64), np.asarray(hz, np.float32)


def format_f0_curve(hz) -> str:
    """one `t,f0` line per 10 ms frame: what --f0-out writes and parse_f0_curve reads back to the same float32 values.  The file is always one --f0-file
    accepts: a frame that is not a number or negative is written as 0 (unvoiced), one above 20000 Hz (a transposed value can be) as 20000"""
    hz = np.asarray(hz, np.float32)
    hz = np.where(hz >= 0, np.minimum(hz, np.float32(20000.0)), np.float32(0.0))
    return "".join("%.2f,%.9g\n" % (j / 100.0, float(v)) for j, v in enumerate(hz))


def parse_sid_mix(text: str) -> dict:
    """"0:0.3,2:0.7" -> {0: 0.3, 2: 0.7}: 1 to 8 distinct ids, weights finite, >= 0 and not all zero (what rvc_set_speaker_mix takes)"""
    mix = {}
    for part in text.split(","):
        k, sep, v = part.partition(":")
        if not sep:
            raise ValueError("%r is no id:weight pair" % part)
        sid, w = int(k), float(v)
        if sid < 0 or sid in mix:
            raise ValueError("id %d is negative or repeated" % sid)
        if not (w >= 0.0 and np.isfinite(w)):
            raise ValueError("weight %r is negative or not finite" % v)
        mix[sid] = w
    if not 1 <= len(mix) <= 8 or not sum(mix.values()) > 0.0:
        raise ValueError("1 to 8 speakers with a positive weight sum")
    return mix


def normalise_peak(x: np.ndarray, peak=None) -> np.ndarray:
    """upstream's rule for a converted file: a peak above 1 is brought down to 0.99, anything else is left alone.  peak: max |x| where the caller has it already"""
    x = np.asarray(x, np.float32)
    if peak is None:
        peak = float(np.max(np.abs(x))) if len(x) else 0.0
    peak = float(peak)
    return x / np.float32(peak / 0.99) if peak > 1.0 else x


def write_wav(path, x, rate: int, peak=None) -> None:
    """mono 16-bit PCM: the peak rule, then round(x * 32767) clipped to the int16 range (build_index.read_wav divides by 32768)"""
    x = normalise_peak(x, peak)
    pcm = np.clip(np.rint(x.astype(np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(os.fspath(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(rate))
        w.writeframes(pcm.tobytes())


def _resample(eng, x: np.ndarray, rate_in: int, rate_out: int) -> np.ndarray:
    """a whole signal through the package's converter in blocks of about 20 ms (as RvcInfer._to_16k), its start-up delay of half a block trimmed"""
    from .resample import FftFixedInOut
    r = FftFixedInOut(eng, rate_in, rate_out, max(rate_in // 50, 1))
    nin = r.input_frames_next()
    nblk = -(-len(x) // nin) + 1
    xp = np.zeros(nblk * nin, np.float32)
    xp[: len(x)] = x
    y = np.concatenate([np.array(r.process(xp[i * nin:(i + 1) * nin]), np.float32) for i in range(nblk)])
    delay, n = r.output_frames_max() // 2, -(-len(x) * rate_out // rate_in)
    return y[delay: delay + n]


def main(argv=None) -> int:
    a = parse_args(argv)
    x, rate = read_wav(a.input)
    if not len(x):
        print("%s holds no samples" % a.input, file=sys.stderr)
        return 2
    from . import weights as W
    from .rvc import RvcInfer
    eng = RvcInfer(a.data or W.default_zoo_root("full"), device=a.device)

    def load_f0():
        if a.f0.startswith("hybrid["):
            eng.load_f0_hybrid(a.f0[len("hybrid["):-1].split("+"), mode=a.f0_hybrid_mode)
        else:
            eng.load_f0_method(a.f0)

    def to_16k(sig, r):
        return sig if r == 16000 else (eng.resample(sig, r, 16000) if a.resampler == "device" else _resample(eng, sig, r, 16000))
    if a.analyze_only:      # the recording's own f0 and nothing else: no ContentVec, no voice model
        load_f0()
        eng.set_streams(a.streams)
        if a.skip_silence is not None:
            eng.set_convert_silence(a.skip_silence, a.silence_hang)
        hz = eng.analyze_f0(to_16k(x, rate), window=a.window, context=a.context, crossfade=a.crossfade, highpass=a.highpass)
        with open(a.f0_out, "w") as fh:
            fh.write(format_f0_curve(hz))
        med, voiced = eng.f0_stats(hz)
        line = "%s: %d frames, %d voiced, median f0 %.2f Hz" % (a.f0_out, len(hz), voiced, float(med[0]))
        if a.skip_silence is not None:
            s = eng.convert_silence_info()
            line += "; %d windows run, %d skipped as silent" % (s["windows_run"], s["windows_skipped"])
        print(line)
        eng.close()
        return 0
    eng.load_contentvec(a.version)
    eng.load_model(a.model)
    if a.f0_out is not None and not eng.model_has_f0():      # (before anything is converted or written)
        print("--f0-out: %s was trained without pitch guidance and has no f0" % a.model, file=sys.stderr)
        eng.close()
        return 2
    if eng.model_has_f0():      # (a model trained without pitch guidance runs no tracker: --f0 names none for it)
        load_f0()
    eng.set_streams(a.streams)
    if a.sid is not None:
        eng.set_speaker(a.sid)
    elif a.sid_mix is not None:
        eng.set_speaker_mix(a.sid_mix)
    if a.index:
        eng.load_index(a.index, nprobe=a.nprobe or None, k=a.index_k)
        eng.set_index_rate(a.index_rate)
    eng.set_pitch_semitones(a.pitch)
    eng.set_formant_shift(a.formant)
    eng.set_protect(a.protect)
    if a.f0_curve is not None:
        eng.set_f0_curve(*a.f0_curve)
    if a.skip_silence is not None:
        eng.set_convert_silence(a.skip_silence, a.silence_hang)
    auto = eng.model_has_f0() and (a.auto_pitch > 0.0 or a.auto_pitch_from is not None)
    if auto:
        target = a.auto_pitch
        if a.auto_pitch_from is not None:      # the target voice's own median, measured as the input's will be
            ref, ref_rate = read_wav(a.auto_pitch_from)
            if not len(ref):
                print("%s holds no samples" % a.auto_pitch_from, file=sys.stderr)
                eng.close()
                return 2
            med, voiced = eng.f0_stats(eng.analyze_f0(to_16k(ref, ref_rate), window=a.window, context=a.context, crossfade=a.crossfade, highpass=a.highpass))
            if not voiced:
                print("--auto-pitch-from: %s has no voiced frame" % a.auto_pitch_from, file=sys.stderr)
                eng.close()
                return 2
            target = float(med[0])
        eng.set_auto_transpose(target, a.auto_pitch_step, a.auto_pitch_limit)
    if a.resampler == "device" or a.rms_mix_rate < 1.0:
        y, out_rate = eng.convert_file(x, rate, k=a.window, context=a.context, crossfade=a.crossfade, pitch_shift=0, highpass=a.highpass, rms_mix_rate=a.rms_mix_rate,
                                       out_rate=a.rate)
        info, f = eng.convert_info(), eng.convert_file_info()
        write_wav(a.output, y, out_rate, peak=f["peak"])
        print("device ms: resample in %.2f, envelope %.2f, resample out %.2f, file total %.2f" % (f["ms_resample_in"], f["ms_envelope"], f["ms_resample_out"], f["ms_total"]))
    else:
        y, model_rate = eng.convert(x, rate=rate, k=a.window, context=a.context, crossfade=a.crossfade, pitch_shift=0, highpass=a.highpass)
        info = eng.convert_info()
        out_rate = a.rate or model_rate
        if out_rate != model_rate:
            y = _resample(eng, y, model_rate, out_rate)
        write_wav(a.output, y, out_rate)
    if a.f0_out is not None:
        with open(a.f0_out, "w") as fh:
            fh.write(format_f0_curve(eng.convert_f0()))
    if auto:
        t = eng.auto_transpose_info()
        print("auto-pitch: median f0 %.2f Hz over %d voiced frames, target %.2f Hz -> %+.2f semitones (device ms: analysis %.2f, select %.2f)"
              % (float(t["median_hz"]), t["voiced"], eng.auto_transpose()["target_hz"], t["semitones"], t["ms_analysis"], t["ms_select"]))
    if a.skip_silence is not None:
        s = eng.convert_silence_info()
        n16 = -(-len(x) * 16000 // rate)      # the gate's frames are those of the 16 kHz signal the model saw
        print("skip-silence: %d windows run, %d skipped; %d of %d frames kept (device ms: analysis %.2f)"
              % (s["windows_run"], s["windows_skipped"], s["frames_kept"], -(-n16 // 160), s["ms_analysis"]))
    print("%s: %.2f s at %d Hz from %d windows in %d batches; device ms: high-pass %.2f, model %.2f, stitch %.2f, total %.2f"
          % (a.output, len(y) / out_rate, out_rate, info["windows"], info["batches"], info["ms_highpass"], info["ms_model"], info["ms_stitch"], info["ms_total"]))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
