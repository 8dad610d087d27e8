"""python -m obs_rvc_amd.convert_dir IN_DIR -o OUT_DIR --model M [--data D] [--version 2] [--f0 rmvpe|yin|crepe-full|crepe-tiny|fcpe|pm|"hybrid[a+b..]" --f0-hybrid-mode vote|median]
       [--index I --index-rate r --index-k 4|8 --nprobe p] [--pitch semitones] [--formant st] [--protect p] [--sid N | --sid-mix 0:0.3,2:0.7] [--streams S]
       [--window k --context C --crossfade X] [--no-highpass] [--rate out_rate] [--rms-mix-rate r]
       [--each-pitch FILE] [--each-auto-pitch HZ | --each-auto-pitch-from REF.wav] [--each-auto-pitch-step 0|1|12] [--each-auto-pitch-limit ST]
       [--each-f0-out DIR [--each-analyze-only]]

Upstream's "model inference" tab, second half (vc_multi): every WAV file of a folder converted with one set of settings.  The files are
read in sorted name order as convert.py reads one, brought to 16 kHz on the GPU (RvcInfer.resample) and converted by ONE RvcInfer.convert_many: the windows
of all files are laid end to end and run `--streams` at a time, so short files share batches instead of each padding one of its own.  Per file the result
then gets the input's volume envelope (--rms-mix-rate below 1), the output rate (--rate) and upstream's 0.99 peak rule, and is written as
OUT_DIR/<name>.wav.  Settings that belong to one recording -- an f0 curve (--f0-file), auto-transpose (--auto-pitch*) -- are convert.py's and refused here.
A pitch per file is this tool's own: --each-pitch FILE lists `name,semitones` lines, --each-auto-pitch HZ (or -from REF.wav, the
reference's median measured as convert.py measures it) moves every file's own median f0 onto the target; both compose, and one line per file on stderr says
what was measured and applied.  --each-f0-out DIR writes every file's own f0 (the analysis, not the transposed curve) as DIR/<name>.csv in the format of
convert's --f0-out; with --each-analyze-only nothing else happens and neither a model nor ContentVec is loaded.
Argument parsing is a plain function; only main() touches the GPU."""
from __future__ import annotations

import argparse
import os
import sys

from .build_index import read_wav
from .convert import AUTO_PITCH_STEPS, F0_CHOICES, SILENCE_HANG_DEFAULT, f0_arg, format_f0_curve, parse_sid_mix, write_wav

PER_RECORDING = ("--auto-pitch", "--f0-file", "--f0-out", "--analyze-only")


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m obs_rvc_amd.convert_dir", description="convert every WAV recording of a folder to a voice on the GPU", allow_abbrev=False)
    p.add_argument("input", help="the folder whose *.wav files are converted (16-bit or 32-bit integer PCM, mono or stereo), in sorted name order")
    p.add_argument("-o", "--output", default=None, help="the folder the converted files are written to under their own names (16-bit PCM, mono); created if missing")
    p.add_argument("--model", default=None, help="the voice: <model>.rvcw (or its .onnx sibling's name)")
    p.add_argument("--data", default=None, help="the engine's data directory (contentvec/, f0/); default: the model zoo of the package")
    p.add_argument("--version", type=int, choices=(1, 2), default=2, help="RVC model version: 1 = 256-dim features, 2 = 768-dim (default)")
    p.add_argument("--f0", type=f0_arg, default="rmvpe", metavar="{%s,hybrid[a+b..]}" % ",".join(F0_CHOICES), help="f0 method, as convert's (default rmvpe)")
    p.add_argument("--f0-hybrid-mode", choices=("vote", "median"), default="vote", help="how a hybrid combines, as convert's (default vote)")
    p.add_argument("--index", default=None, help="retrieval index: a Faiss .index file or a .npy matrix")
    p.add_argument("--index-rate", type=float, default=0.75, help="share of the retrieved features (default 0.75, with --index only)")
    p.add_argument("--index-k", type=int, choices=(4, 8), default=8, help="neighbours blended per frame (default 8, upstream's)")
    p.add_argument("--nprobe", type=int, default=0, help="IVF lists probed per frame; 0 = search every row (default)")
    p.add_argument("--pitch", type=float, default=0.0, help="transpose in semitones, -24..24 (default 0), the same for every file")
    p.add_argument("--formant", type=float, default=0.0, help="formant shift in semitones, -5..5 (default 0)")
    p.add_argument("--protect", type=float, default=0.5, help="consonant protection, 0..0.5; 0.5 = off (default)")
    p.add_argument("--sid", type=int, default=None, help="speaker id of a multi-speaker model (default: the speaker baked into the model file)")
    p.add_argument("--sid-mix", default=None, help="a blend of up to 8 speakers as id:weight pairs, e.g. 0:0.3,2:0.7 (weights are normalised)")
    p.add_argument("--streams", type=int, default=8, help="windows converted at a time, whichever files they belong to (default 8)")
    p.add_argument("--window", type=int, default=0, help="window size k: a window is 32 k - 1 frames of 10 ms; 2..32 (default 14)")
    p.add_argument("--context", type=int, default=0, help="context frames on each side of a window, >= 3 (default 48)")
    p.add_argument("--crossfade", type=int, default=0, help="crossfade frames between windows, >= 1 (default 5)")
    p.add_argument("--no-highpass", dest="highpass", action="store_false", help="skip the 48 Hz high-pass in front of the model")
    p.add_argument("--rate", type=int, default=0, help="output sample rate (default: the model's)")
    p.add_argument("--rms-mix-rate", type=float, default=1.0, help="volume envelope, 0..1: 0 = each input's envelope, 1 = the model's own (default)")
    p.add_argument("--skip-silence", type=float, default=None, metavar="DB",
                   help="do not run windows in which nothing reaches DB (40 ms RMS in dB, the live gate's measure; above -60, e.g. -50): they become exact silence")
    p.add_argument("--silence-hang", type=int, default=None, metavar="FRAMES", help="10 ms frames kept on each side of a loud frame, 0..1000 (default 30; with --skip-silence)")
    p.add_argument("--each-pitch", default=None, metavar="FILE", help="a transpose per file: lines `name,semitones` (-24..24); a file not named gets 0, an unknown name is an error")
    p.add_argument("--each-auto-pitch", type=float, default=0.0, metavar="HZ", help="move the median f0 of EVERY file onto HZ, each by its own transpose (0 = off, the default)")
    p.add_argument("--each-auto-pitch-from", default=None, metavar="REF.wav", help="... onto the median f0 of this recording of the target voice")
    p.add_argument("--each-auto-pitch-step", type=int, choices=AUTO_PITCH_STEPS, default=1, help="round each transpose to 0 = nothing, 1 = semitones (default), 12 = octaves")
    p.add_argument("--each-auto-pitch-limit", type=float, default=12.0, metavar="ST", help="the largest transpose, 0..24 semitones (default 12)")
    p.add_argument("--each-f0-out", default=None, metavar="DIR", help="write every file's own f0 as DIR/<name>.csv, one `t,f0` line per 10 ms frame")
    p.add_argument("--each-analyze-only", action="store_true", help="with --each-f0-out: analyse and stop; no model is loaded, nothing is converted")
    p.add_argument("--device", type=int, default=-1)
    for arg in (sys.argv[1:] if argv is None else argv):
        if str(arg).startswith(PER_RECORDING):
            p.error("%s belongs to one recording: use python -m obs_rvc_amd.convert for it" % str(arg).split("=", 1)[0])
    a = p.parse_args(argv)
    if a.each_analyze_only and a.each_f0_out is None:
        p.error("--each-analyze-only goes with --each-f0-out")
    if not a.each_analyze_only and (a.output is None or a.model is None):
        p.error("a conversion needs -o/--output and --model")
    if not 0.0 <= a.each_auto_pitch <= 20000.0:
        p.error("--each-auto-pitch is a frequency in Hz, up to 20000 (0 = off)")
    if a.each_auto_pitch > 0.0 and a.each_auto_pitch_from is not None:
        p.error("--each-auto-pitch and --each-auto-pitch-from exclude each other")
    if not 0.0 <= a.each_auto_pitch_limit <= 24.0:
        p.error("--each-auto-pitch-limit is 0..24 semitones")
    if a.silence_hang is not None and a.skip_silence is None:
        p.error("--silence-hang goes with --skip-silence")
    if a.skip_silence is not None and not -60.0 < a.skip_silence <= 0.0:
        p.error("--skip-silence is a level in dB above -60 and at most 0")
    if a.silence_hang is None:
        a.silence_hang = SILENCE_HANG_DEFAULT
    if not 0 <= a.silence_hang <= 1000:
        p.error("--silence-hang is 0..1000 frames")
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


def parse_each_pitch(text: str, names) -> list:
    """--each-pitch's file: one `name,semitones` pair per line, blank lines and # comments ignored; `name` is a file of the folder with or without its .wav.
    -> semitones per file of `names`, in their order, 0 for a file not named.  ValueError names the line: no pair, a value outside -24..24, an unknown or
    repeated name"""
    stems = {}
    for i, f in enumerate(names):
        stems[f] = i
        stems.setdefault(os.path.splitext(f)[0], i)
    out, seen = [0.0] * len(names), set()
    for no, line in enumerate(text.splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        name, sep, val = line.rpartition(",")
        try:
            if not sep:
                raise ValueError
            st = float(val)
        except ValueError:
            raise ValueError("line %d: %r is no `name,semitones` pair" % (no, line)) from None
        if not -24.0 <= st <= 24.0:
            raise ValueError("line %d: %r is outside -24..24 semitones" % (no, val.strip()))
        name = name.strip()
        if name not in stems:
            raise ValueError("line %d: the folder holds no file %r" % (no, name))
        if stems[name] in seen:
            raise ValueError("line %d: %r is named twice" % (no, name))
        seen.add(stems[name])
        out[stems[name]] = st
    return out


def list_wavs(folder) -> list:
    """the *.wav files (any letter case) directly inside `folder`, in sorted name order"""
    return sorted(f for f in os.listdir(folder) if f.lower().endswith(".wav") and os.path.isfile(os.path.join(folder, f)))


def main(argv=None) -> int:
    a = parse_args(argv)
    names = list_wavs(a.input)
    if not names:
        print("%s holds no WAV file" % a.input, file=sys.stderr)
        return 2
    if a.output is not None and os.path.realpath(a.input) == os.path.realpath(a.output):
        print("the output folder is the input folder: the converted files would replace the recordings", file=sys.stderr)
        return 2
    each_pitch = None
    if a.each_pitch is not None:
        try:
            with open(a.each_pitch) as fh:
                each_pitch = parse_each_pitch(fh.read(), names)
        except (OSError, ValueError) as x:
            print("--each-pitch %s: %s" % (a.each_pitch, x), file=sys.stderr)
            return 2
    recs = [read_wav(os.path.join(a.input, f)) for f in names]
    for f, (x, _) in zip(names, recs):
        if not len(x):
            print("%s holds no samples" % os.path.join(a.input, f), file=sys.stderr)
            return 2
    from . import weights as W
    from .rvc import RvcInfer
    eng = RvcInfer(a.data or W.default_zoo_root("full"), device=a.device)

    def load_f0():
        if a.f0.startswith("hybrid["):
            eng.load_f0_hybrid(a.f0[len("hybrid["):-1].split("+"), mode=a.f0_hybrid_mode)
        else:
            eng.load_f0_method(a.f0)

    def write_f0(rows):
        os.makedirs(a.each_f0_out, exist_ok=True)
        for f, hz in zip(names, rows):
            with open(os.path.join(a.each_f0_out, os.path.splitext(f)[0] + ".csv"), "w") as fh:
                fh.write(format_f0_curve(hz))

    def analyze(sigs):
        return eng.analyze_f0_many(sigs, window=a.window, context=a.context, crossfade=a.crossfade, highpass=a.highpass)
    if a.each_analyze_only:      # every recording's own f0 and nothing else: no ContentVec, no voice model
        load_f0()
        eng.set_streams(a.streams)
        if a.skip_silence is not None:
            eng.set_convert_silence(a.skip_silence, a.silence_hang)
        rows = analyze([x if rate == 16000 else eng.resample(x, rate, 16000) for x, rate in recs])
        write_f0(rows)
        med, voiced = eng.f0_stats_many(rows)
        for f, m, v in zip(names, med[:, 0], voiced):
            print("%s: median f0 %.2f Hz over %d voiced frames" % (f, float(m), v), file=sys.stderr)
        print("%s: the f0 of %d files" % (a.each_f0_out, len(names)))
        eng.close()
        return 0
    eng.load_contentvec(a.version)
    eng.load_model(a.model)
    if a.each_f0_out is not None and not eng.model_has_f0():      # (before anything is converted or written)
        print("--each-f0-out: %s was trained without pitch guidance and has no f0" % a.model, file=sys.stderr)
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
    if a.skip_silence is not None:
        eng.set_convert_silence(a.skip_silence, a.silence_hang)
    x16 = [x if rate == 16000 else eng.resample(x, rate, 16000) for x, rate in recs]
    per_file = eng.model_has_f0() and (each_pitch is not None or a.each_auto_pitch > 0.0 or a.each_auto_pitch_from is not None)
    if per_file:
        target = a.each_auto_pitch
        if a.each_auto_pitch_from is not None:      # the target voice's own median, measured as the inputs' will be (convert.py's --auto-pitch-from)
            ref, ref_rate = read_wav(a.each_auto_pitch_from)
            if not len(ref):
                print("%s holds no samples" % a.each_auto_pitch_from, file=sys.stderr)
                eng.close()
                return 2
            ref16 = ref if ref_rate == 16000 else eng.resample(ref, ref_rate, 16000)
            med, voiced = eng.f0_stats(eng.analyze_f0(ref16, window=a.window, context=a.context, crossfade=a.crossfade, highpass=a.highpass))
            if not voiced:
                print("--each-auto-pitch-from: %s has no voiced frame" % a.each_auto_pitch_from, file=sys.stderr)
                eng.close()
                return 2
            target = float(med[0])
        eng.set_convert_many_pitch(each_pitch)
        eng.set_convert_many_auto_transpose(target, a.each_auto_pitch_step, a.each_auto_pitch_limit)
    if a.each_f0_out is not None:
        write_f0(analyze(x16))
    ys = eng.convert_many(x16, k=a.window, context=a.context, crossfade=a.crossfade, pitch_shift=0, highpass=a.highpass)
    info = eng.convert_many_info()
    if per_file:
        t = eng.convert_many_pitch_info()
        for f, m, v, st in zip(names, t["median_hz"], t["voiced"], t["semitones"]):
            print("%s: median f0 %.2f Hz over %d voiced frames -> %+.2f semitones" % (f, float(m), v, st), file=sys.stderr)
        print("each-pitch: device ms: analysis %.2f, select %.2f" % (t["ms_analysis"], t["ms_select"]))
    # the model's rate: a file's output is ceil(n / 160) frames of rate / 100 samples
    model_rate = 100 * (len(ys[0]) // -(-len(x16[0]) // 160))
    out_rate = a.rate or model_rate
    os.makedirs(a.output, exist_ok=True)
    seconds = 0.0
    for f, x, y in zip(names, x16, ys):
        if a.rms_mix_rate != 1.0:      # against the signal the model saw, as convert_file does
            y = eng.change_rms(eng.highpass(x) if a.highpass else x, 16000, y, model_rate, a.rms_mix_rate)
        if out_rate != model_rate:
            y = eng.resample(y, model_rate, out_rate)
        write_wav(os.path.join(a.output, os.path.splitext(f)[0] + ".wav"), y, out_rate)
        seconds += len(y) / out_rate
    if a.skip_silence is not None:
        s = eng.convert_silence_info()
        print("skip-silence: %d windows run, %d skipped (device ms: analysis %.2f)" % (s["windows_run"], s["windows_skipped"], s["ms_analysis"]))
    print("%s: %d files, %.2f s at %d Hz from %d windows in %d batches; device ms: high-pass %.2f, model %.2f, stitch %.2f, total %.2f"
          % (a.output, len(names), seconds, out_rate, info["windows"], info["batches"], info["ms_highpass"], info["ms_model"], info["ms_stitch"], info["ms_total"]))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
