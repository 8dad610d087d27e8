"""Mirror of the reference's `rvc-common` crate: enums and the error type.

Reference: /root/reference/rvc-common/src/enums.rs:4-146, rvc-common/src/errors.rs:2-20.
"""
from __future__ import annotations

import enum

# crossfade of the SOLA seam (include/rvc_mi355x.h RVC_CROSSFADE_*): the plugin's sin^2 blend, or the phase-vocoder blend
CROSSFADE_LINEAR, CROSSFADE_PHASE_VOCODER = 0, 1
# f0 methods of rvc_load_f0_method (include/rvc_mi355x.h RVC_F0_*): PitchAlgorithm below stays the reference's one-variant enum
F0_RMVPE, F0_YIN = 1, 2
F0_CREPE, F0_CREPE_TINY = 4, 5          # (3 is no method: it stays the unknown value it was)
F0_FCPE = 7                             # (nor is 6)
F0_PM = 9                               # Praat's autocorrelation tracker (upstream's "pm"), weight-free as YIN
F0_HYBRID = 8                           # rvc_load_f0_hybrid: several of the above combined per frame (RVC_HYBRID_VOTE / _MEDIAN)
HYBRID_VOTE, HYBRID_MEDIAN = 0, 1
HYBRID_MAX_MEMBERS = 4
# CREPE's decoders (rvc_set_crepe_decoder, RVC_CREPE_*)
CREPE_VITERBI, CREPE_ARGMAX = 0, 1
# input gate: a threshold at or below this many dB switches it off
INPUT_GATE_OFF_DB = -60.0
# sides of the session's spectral-gate noise reduction (include/rvc_mi355x.h RVC_DENOISE_*): in front of the host-rate ring, or on the finished frame
DENOISE_INPUT, DENOISE_OUTPUT = 0, 1
# scale snap (rvc_set_f0_snap): bit k of a mask allows pitch class k, C = 0, so MIDI note n is allowed iff bit n % 12 is set
SCALE_CHROMATIC = 0xFFF
_SCALE_STEPS = {"major": (0, 2, 4, 5, 7, 9, 11), "minor": (0, 2, 3, 5, 7, 8, 10), "chromatic": tuple(range(12))}
_NOTE_NAMES = {"c": 0, "d": 2, "e": 4, "f": 5, "g": 7, "a": 9, "b": 11}


def parse_f0_hybrid(text: str, names):
    """The forks' bracket form of a hybrid f0 method: "hybrid[rmvpe+fcpe+crepe-tiny]" -> ["rmvpe", "fcpe", "crepe-tiny"] (lower case, the order kept: the first
    member is the lead).  `names`: the member names accepted.  None when `text` is not of the form hybrid[...] at all; ValueError when it is but names no valid
    hybrid: an empty or unknown member, a member named twice, more than HYBRID_MAX_MEMBERS."""
    t = text.strip().lower()
    if not t.startswith("hybrid"):
        return None
    if not (t.startswith("hybrid[") and t.endswith("]")):
        raise ValueError("hybrid f0: write hybrid[a+b], e.g. hybrid[rmvpe+fcpe], not %r" % text)
    members = [m.strip() for m in t[len("hybrid["):-1].split("+")]
    for m in members:
        if m not in names:
            raise ValueError("hybrid f0: %r is no member (%s)" % (m, ", ".join(sorted(names))))
    if len(set(members)) != len(members):
        raise ValueError("hybrid f0: a member is named twice in %r" % text)
    if not 1 <= len(members) <= HYBRID_MAX_MEMBERS:
        raise ValueError("hybrid f0: 1 to %d members, not %d" % (HYBRID_MAX_MEMBERS, len(members)))
    return members


def scale_mask(root, kind: str = "major") -> int:
    """The pitch-class mask of a scale: root = a pitch class 0..11 or a note name ("C", "F#", "Bb"), kind = "major" | "minor" (natural
    minor) | "chromatic"."""
    if isinstance(root, str):
        name = root.strip().lower()
        if not name or name[0] not in _NOTE_NAMES or name[1:] not in ("", "#", "b"):
            raise ValueError("scale root: a note name such as 'C', 'F#', 'Bb', not %r" % root)
        root = _NOTE_NAMES[name[0]] + {"": 0, "#": 1, "b": -1}[name[1:]]
    if kind not in _SCALE_STEPS:
        raise ValueError("scale kind: 'major', 'minor' or 'chromatic', not %r" % kind)
    mask = 0
    for s in _SCALE_STEPS[kind]:
        mask |= 1 << ((int(root) + s) % 12)
    return mask


SCALE_C_MAJOR = scale_mask(0, "major")        # 0xAB5


class RvcModelVersion(enum.Enum):
    V1 = 1
    V2 = 2

    def text_encoder_in_channels(self) -> int:      # enums.rs:10-16
        return 256 if self is RvcModelVersion.V1 else 768

    def output_layers(self) -> int:                 # enums.rs:17-23
        return 9 if self is RvcModelVersion.V1 else 12

    @classmethod
    def from_value(cls, val) -> "RvcModelVersion":
        """enums.rs:42-74: 1/"v1" -> V1, 2/"v2" -> V2, anything else silently maps to V2."""
        if isinstance(val, cls):
            return val
        if val in (1, "v1"):
            return cls.V1
        return cls.V2

    def __int__(self) -> int:                        # enums.rs:32-40
        return self.value

    def __str__(self) -> str:                        # enums.rs:53-60, 76-83
        return "v1" if self is RvcModelVersion.V1 else "v2"

    @staticmethod
    def is_valid(val: int) -> bool:                  # enums.rs:85-92
        return val in (1, 2)


class PitchAlgorithm(enum.Enum):
    Rmvpe = 1

    @classmethod
    def from_value(cls, val) -> "PitchAlgorithm":
        """enums.rs:104-133: every value maps to Rmvpe."""
        return cls.Rmvpe

    def __int__(self) -> int:
        return 1

    def __str__(self) -> str:
        return "rmvpe"

    @staticmethod
    def is_valid(val: int) -> bool:
        return val == 1


class RvcInferError(Exception):
    """errors.rs:2-8.  `kind` is one of the variant names; Ort(..) is called Backend here."""

    KINDS = {1: "ModelNotLoaded", 2: "ContentvecNotLoaded", 3: "F0NotLoaded", 4: "Backend", 5: "NdarrayShapeError", 6: "Panic"}

    def __init__(self, code: int, message: str = ""):
        self.code = code
        self.kind = self.KINDS.get(code, "Unknown(%d)" % code)
        super().__init__("%s%s" % (self.kind, (": " + message) if message else ""))
