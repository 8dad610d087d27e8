"""python -m obs_rvc_amd.convert_dir IN_DIR -o OUT_DIR --model M [--data D] [--version 2] [--f0 rmvpe|yin|crepe-full|crepe-tiny|fcpe|pm|"hybrid[a+b..]" --f0-hybrid-mode vote|median]
       [--index I --index-rate r --index-k 4|8 --nprobe p] [--pitch semitones] [--formant st] [--protect p] [--sid N | --sid-mix 0:0.3,2:0.7] [--streams S]
       [--window k --context C --crossfade X] [--no-highpass] [--rate out_rate] [--rms-mix-rate r]

Upstream's "model inference" tab, second half (vc_multi): every WAV file of a folder converted with one set of settings.  The files are
read in sorted name order as convert.py reads one, brought to 16 kHz on the GPU (RvcInfer.resample) and converted by ONE RvcInfer.convert_many: the windows
of all files are laid end to end and run `--streams` at a time, so short files share batches instead of each padding one of its own.  Per file the result
then gets the input's volume envelope (--rms-mix-rate below 1), the output rate (--rate) and upstream's 0.99 peak rule, and is written as
OUT_DIR/<name>.wav.  Settings that belong to one recording -- an f0 curve (--f0-file), auto-transpose (--auto-pitch*) -- are convert.py's and refused here.
Argument parsing is a plain function; only main() touches the GPU."""
from __future__ import annotations

import argparse
import os
import sys

from .build_index import read_wav
from .convert import F0_CHOICES, SILENCE_HANG_DEFAULT, f0_arg, parse_sid_mix, write_wav

PER_RECORDING = ("--auto-pitch", "--f0-file", "--f0-out", "--analyze-only")


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m obs_rvc_amd.convert_dir", description="convert every WAV recording of a folder to a voice on the GPU", allow_abbrev=False)
    p.add_argument("input", help="the folder whose *.wav files are converted (16-bit or 32-bit integer PCM, mono or stereo), in sorted name order")
    p.add_argument("-o", "--output", required=True, help="the folder the converted files are written to under their own names (16-bit PCM, mono); created if missing")
    p.add_argument("--model", required=True, help="the voice: <model>.rvcw (or its .onnx sibling's name)")
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
    p.add_argument("--device", type=int, default=-1)
    for arg in (sys.argv[1:] if argv is None else argv):
        if str(arg).startswith(PER_RECORDING):
            p.error("%s belongs to one recording: use python -m obs_rvc_amd.convert for it" % str(arg).split("=", 1)[0])
    a = p.parse_args(argv)
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


def list_wavs(folder) -> list:
    """the *.wav files (any letter case) directly inside `folder`, in sorted name order"""
    return sorted(f for f in os.listdir(folder) if f.lower().endswith(".wav") and os.path.isfile(os.path.join(folder, f)))


def main(argv=None) -> int:
    a = parse_args(argv)
    names = list_wavs(a.input)
    if not names:
        print("%s holds no WAV file" % a.input, file=sys.stderr)
        return 2
    if os.path.realpath(a.input) == os.path.realpath(a.output):
        print("the output folder is the input folder: the converted files would replace the recordings", file=sys.stderr)
        return 2
    recs = [read_wav(os.path.join(a.input, f)) for f in names]
    for f, (x, _) in zip(names, recs):
        if not len(x):
            print("%s holds no samples" % os.path.join(a.input, f), file=sys.stderr)
            return 2
    from . import weights as W
    from .rvc import RvcInfer
    eng = RvcInfer(a.data or W.default_zoo_root("full"), device=a.device)
    eng.load_contentvec(a.version)
    eng.load_model(a.model)
    if eng.model_has_f0():      # (a model trained without pitch guidance runs no tracker: --f0 names none for it)
        if a.f0.startswith("hybrid["):
            eng.load_f0_hybrid(a.f0[len("hybrid["):-1].split("+"), mode=a.f0_hybrid_mode)
        else:
            eng.load_f0_method(a.f0)
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
    ys = eng.convert_many(x16, k=a.window, context=a.context, crossfade=a.crossfade, pitch_shift=0, highpass=a.highpass)
    info = eng.convert_many_info()
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
