"""Audio-reactive frame feedback (no counterpart in the reference): ``ar.Feedback`` builds the per-frame rows that csrc/feedback.hip
applies to the generator's fp32 image — the previous OUTPUT frame fed back under the new one, slightly zoomed, turned or moved and a
little darker, so that highlights leave trails and a kick opens an echo tunnel —, in front of the lens, the grade and every quantiser
(render.feedback_frames / render.render_fed; a plugin hands it over as ``args.feedback``).

Per rendered frame t, in unit space (0 = black, so a trail decays towards black, not towards grey):
    out_t = min(combine(dry cur_t, gain tint warp(out_{t-1})), limit)
with ``warp`` a bilinear tap through the frame's affine map and ``combine`` one of add / max / screen (include/maua_hip.h states the
arithmetic).  Before the first frame of a render the previous output is black.  A row with gain 0 and dry 1 passes its frame through bit
for bit.  With --subframes N the recurrence runs per RENDERED sub-frame (the fold averages afterwards): ``gain`` then compounds N times
per written frame — ``Feedback.gain_for(half_life, fps * N)`` gives the gain of a wanted half-life.

A device row is 16 float32: the INVERSE matrix in pixels a, b, tx, c, d, ty, gain, tint[3], dry, limit, a "still" flag (the matrix is
exactly the identity: such frames run on the register path of the kernel), three reserved zeros.  Translations are fractions of the
frame's width and height, so the rows are built per frame size (``rows`` / ``operands``).
"""
import math

import numpy as np

from . import frame_table
from .frame_table import FrameTable, collect, host64

__all__ = ["Feedback", "FEEDBACK_ROW"]

FEEDBACK_ROW = 16
MODES = ("add", "max", "screen")
BORDERS = ("zero", "replicate", "mirror", "wrap")
_A, _TY, _GAIN, _TINT, _DRY, _LIMIT, _STILL = 0, 5, 6, 7, 10, 11, 12
# the columns of the parameter table (float64 [n, 10])
P_GAIN, P_DRY, P_ZOOM, P_ROTATE, P_TX, P_TY, P_TINT, P_LIMIT, P_COLS = 0, 1, 2, 3, 4, 5, 6, 9, 10


class Feedback(FrameTable):
    """Frame feedback: one parameter row per rendered frame, or one row for all of them.

    ``gain``, ``dry``, ``zoom``, ``rotate`` are scalars or per-frame sequences — [n_frames] or [n_frames, 1] —, ``translate`` a pair or
    [n_frames, 2], ``tint`` a triple (R, G, B) or [n_frames, 3]; torch or numpy, host or device.  ``n_frames`` None: the length of the
    sequences (they must agree), one row without any.

      gain       what of the previous output survives a frame (>= 0); 0 switches the feedback off.  ``Feedback.gain_for`` turns a
                 half-life in seconds into a gain
      dry        weight of the new frame (1: unchanged)
      zoom       > 1: each recirculation MAGNIFIES the old picture about the centre — the trail flies outward; < 1: it recedes
      rotate     degrees per frame, counter-clockwise as seen on the screen
      translate  (right, down) per frame, as fractions of the frame's width and height
      tint       colour the trail is multiplied by every frame: old echoes drift towards it
      limit      ceiling of the result in unit space (> 0; 1 = display white): caps a diverging ``add``
      mode       "add" | "max" | "screen": how the new frame and the trail combine (one per render)
      border     "zero" | "replicate" | "mirror" | "wrap": what a tap outside the frame sees (one per render)

    Refused: non-finite values, gain < 0, limit <= 0, zoom <= 0, sequences of different lengths, an unknown mode or border.  The device
    checks none of this."""

    MASK = "neutral"  # (a neutral row — gain 0, dry 1 — is this class's identity)

    def __init__(self, n_frames=None, *, gain=0, dry=1, zoom=1, rotate=0, translate=(0, 0), tint=(1, 1, 1), limit=4.0, mode="add",
                 border="zero"):
        n, cols = collect("Feedback", n_frames, [("gain", gain, 1, False), ("dry", dry, 1, False), ("zoom", zoom, 1, False), ("rotate", rotate, 1, False),
                                                 ("translate", translate, 2, False), ("tint", tint, 3, False), ("limit", limit, 1, False)])
        table = np.concatenate([np.broadcast_to(c, (n, c.shape[1])) for c in cols], axis=1)
        self._init(table, mode, border)

    def _init(self, table, mode, border):
        if mode not in MODES:
            raise ValueError(f"Feedback: unknown mode {mode!r} ({' | '.join(MODES)})")
        if border not in BORDERS:
            raise ValueError(f"Feedback: unknown border {border!r} ({' | '.join(BORDERS)})")
        table = np.array(table, np.float64)
        if table.ndim != 2 or table.shape[1] != P_COLS or table.shape[0] < 1:
            raise ValueError(f"Feedback: the parameter table must be [n, {P_COLS}], got {table.shape}")
        with np.errstate(over="ignore"):
            if not np.all(np.isfinite(table.astype(np.float32))):
                raise ValueError("Feedback: the parameters overflow float32 or are not finite")
        if np.any(table[:, P_GAIN] < 0):
            raise ValueError("Feedback: gain must not be negative")
        if np.any(table[:, P_LIMIT] <= 0):
            raise ValueError("Feedback: limit must be positive")
        if np.any(table[:, P_ZOOM] <= 0):
            raise ValueError("Feedback: zoom must be positive")
        self.table, self.mode, self.border = table, mode, border
        self.table.setflags(write=False)
        with np.errstate(over="ignore"):
            self.neutral = (table[:, P_GAIN].astype(np.float32) == 0) & (table[:, P_DRY].astype(np.float32) == 1)
        self._rows = {}

    @classmethod
    def from_tables(cls, table, mode="add", border="zero"):
        """A feedback from a finished parameter table, float64 [n, 10]: gain, dry, zoom, rotate, translate x, y, tint r, g, b, limit per row
        (validated as the constructor does)."""
        self = cls.__new__(cls)
        self._init(host64(table), mode, border)
        return self

    @staticmethod
    def gain_for(half_life_seconds, fps):
        """The gain at which a trail loses half its light in ``half_life_seconds`` at ``fps`` RENDERED frames a second:
        0.5 ** (1 / (half_life fps))."""
        frames = float(half_life_seconds) * float(fps)
        if not (math.isfinite(frames) and frames > 0):
            raise ValueError(f"Feedback.gain_for: a half-life of {half_life_seconds!r} s at {fps!r} fps")
        return 0.5 ** (1.0 / frames)

    def __repr__(self):
        return (f"Feedback({self._count()}, mode={self.mode}, border={self.border}, "
                f"neutral={int(self.neutral.sum())})")

    def rows(self, h, w):
        """The device rows, float32 [n, 16] on the host, for frames of h x w: each row's inverse matrix in pixels, composed in float64 —
        d_out = zoom R d_src + t with R = [[cos, sin], [-sin, cos]] (counter-clockwise on a screen whose y points down) and
        t = (translate_x w, translate_y h), so d_src = (1 / zoom) R^T (d_out - t) — and the still flag, set exactly when the float32 matrix
        is the identity.  Built once per size."""
        key = (int(h), int(w))
        if key not in self._rows:
            if h < 1 or w < 1:
                raise ValueError(f"Feedback.rows: a frame of {h} x {w}")
            t = self.table
            ang = np.radians(t[:, P_ROTATE])
            co, si, z = np.cos(ang), np.sin(ang), t[:, P_ZOOM]
            a, b, c, d = co / z, -si / z, si / z, co / z
            px, py = t[:, P_TX] * float(w), t[:, P_TY] * float(h)
            rows = np.zeros((self.n_rows, FEEDBACK_ROW), np.float64)
            rows[:, 0], rows[:, 1], rows[:, 2] = a, b, -(a * px + b * py)
            rows[:, 3], rows[:, 4], rows[:, 5] = c, d, -(c * px + d * py)
            rows[:, _GAIN], rows[:, _DRY], rows[:, _LIMIT] = t[:, P_GAIN], t[:, P_DRY], t[:, P_LIMIT]
            rows[:, _TINT:_TINT + 3] = t[:, P_TINT:P_TINT + 3]
            with np.errstate(over="ignore"):
                rows = rows.astype(np.float32)
            if not np.all(np.isfinite(rows)):
                raise ValueError(f"Feedback: the matrices overflow float32 on frames of {h} x {w}")
            rows[:, _STILL] = (rows[:, _A:_TY + 1] == np.asarray((1, 0, 0, 0, 1, 0), np.float32)).all(axis=1)
            rows.setflags(write=False)
            self._rows[key] = rows
        return self._rows[key]

    def operands(self, h, w):
        """(rows, mode index, border index) for frames of h x w.  The rows stay on the HOST (float32 [n, 16], contiguous): the entry reads
        them while it plans its launches and hands each launch its row by value."""
        return self.rows(h, w), MODES.index(self.mode), BORDERS.index(self.border)

    def tables(self):
        """(table, mode, border): ``Feedback.from_tables(*x.tables())`` is x."""
        return self.table, self.mode, self.border

    def _block(self, lo, hi):
        return Feedback.from_tables(self.table[lo:hi], self.mode, self.border)  # (the recurrence starts from black at ``lo``)


SPEC_KEYS = ("gain", "dry", "zoom", "rotate", "translate", "tint", "limit", "mode", "border")


def parse_spec(text):
    """A static feedback as text, ``"gain=0.92,zoom=1.015,rotate=0.3,mode=max,border=mirror"`` (the --feedback flag), -> the keyword
    arguments of Feedback.  Keys: SPEC_KEYS; a value is a number, translate two and tint three numbers joined by ``:``
    (``translate=0.01:0``), mode and border a name."""
    counts = {k: ({"translate": 2, "tint": 3}.get(k, 1),) for k in SPEC_KEYS[:-2]}
    return frame_table.parse_spec("--feedback", text, counts, {"mode": MODES, "border": BORDERS})
