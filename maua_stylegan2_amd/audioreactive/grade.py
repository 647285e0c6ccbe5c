"""Audio-reactive colour grading (no counterpart in the reference): ``ar.Grade`` builds the per-frame row table that csrc/grade.hip
applies to the generator's fp32 image, in front of every quantiser (render.grade_frames / render.render_graded; a plugin hands it over as
``args.grade``).  ``ar.load_cube`` / ``ar.save_cube`` / ``ar.lut_from_function`` make the 3-D LUT.

A row is 24 float32 (include/maua_hip.h, maua_grade_f32): slope[3] offset[3] power[3] matrix[9] bias[3] lut_mix reserved[2]; per pixel
the device computes  v = clamp01(x / 2 + 1 / 2);  t = clamp01(v * slope + offset) ** power;  m = clamp01(M t + bias);  m = lerp(m,
tetra(lut, m), lut_mix);  y = 2 m - 1.  A row that is the identity passes its frame through bit for bit.
"""
import math

import numpy as np
import torch as th

from . import frame_table
from .frame_table import FrameTable, collect, host64

__all__ = ["Grade", "load_cube", "save_cube", "lut_from_function", "hue_matrix", "saturation_matrix", "GRADE_ROW"]

GRADE_ROW = 24
_SLOPE, _OFFSET, _POWER, _MATRIX, _BIAS, _MIX = 0, 3, 6, 9, 18, 21
LUMA_REC709 = (0.2126, 0.7152, 0.0722)
LUT_MIN, LUT_MAX = 2, 65


def saturation_matrix(s):
    """The ASC CDL saturation as a matrix: out = luma + s (in - luma) with the Rec. 709 weights 0.2126 / 0.7152 / 0.0722.  ``s``: a scalar or
    [n]; returns [3, 3] or [n, 3, 3] float64."""
    s = np.asarray(s, np.float64)
    w = np.tile(np.asarray(LUMA_REC709, np.float64), (3, 1))
    return (1.0 - s)[..., None, None] * w + s[..., None, None] * np.eye(3)


def hue_matrix(degrees):
    """The luma-preserving hueRotate matrix of the SVG / CSS filter specification (weights 0.213 / 0.715 / 0.072).  ``degrees``: a scalar or
    [n]; returns [3, 3] or [n, 3, 3] float64; 0 degrees is the identity exactly."""
    d = np.asarray(degrees, np.float64)
    a = np.deg2rad(d)
    base = np.array([[0.213, 0.715, 0.072]] * 3)
    cos = np.array([[0.787, -0.715, -0.072], [-0.213, 0.285, -0.072], [-0.213, -0.715, 0.928]])
    sin = np.array([[-0.213, -0.715, 0.928], [0.143, 0.140, -0.283], [-0.787, 0.715, 0.072]])
    m = base + np.cos(a)[..., None, None] * cos + np.sin(a)[..., None, None] * sin
    return np.where((d == 0)[..., None, None], np.eye(3), m)


class Grade(FrameTable):
    """A colour grade: one parameter row per rendered frame, or one row for all of them, and an optional 3-D LUT.

    Every argument is a scalar, a per-channel triple (R, G, B) where it says so, or a per-frame sequence — [n_frames], [n_frames, 1] or
    (per-channel arguments) [n_frames, 3]; torch or numpy, host or device.  A [3] value of a per-channel argument is a triple.  ``n_frames``
    None: the length of the sequences (they must agree), one row without any.

      exposure       stops: gain 2 ** exposure                                         scalar / per frame
      white_balance  gain per channel                                                   per channel
      slope, offset  ASC CDL slope and offset                                           per channel
      contrast, pivot   c (t - pivot) + pivot, applied after the gains and the offset  scalar / per frame
      power, gamma   ASC CDL power (> 0); gamma g is power 1 / g; both multiply         per channel
      saturation     ASC CDL saturation (Rec. 709 luma), as a matrix                    scalar / per frame
      hue            degrees; the SVG hueRotate matrix                                  scalar / per frame
      matrix, bias   an explicit 3 x 3 matrix ([3, 3] or [n_frames, 3, 3]) and bias     bias per channel
      lut, lut_mix   a table [N, N, N, 3] (load_cube, lut_from_function) or a .cube path; its weight in [0, 1]

    The row holds slope = 2 ** exposure * white_balance * slope * contrast, offset = offset * contrast + pivot (1 - contrast), power =
    power / gamma, and the matrix  hue . saturation . matrix : the user matrix is applied FIRST, then the saturation, then the hue rotation.
    Refused: non-finite values, power or gamma <= 0, lut_mix outside [0, 1], sequences of different lengths, a table that is not
    [N, N, N, 3] with 2 <= N <= 65.  The device checks none of this."""

    def __init__(self, n_frames=None, *, exposure=0, contrast=1, pivot=0.5, slope=1, offset=0, power=1, gamma=None, white_balance=None,
                 saturation=1, hue=0, matrix=None, bias=0, lut=None, lut_mix=1):
        per_frame, per_channel = (1, False), (3, True)
        n, (exposure, contrast, pivot, slope, offset, power, gamma, wb, saturation, hue, bias, mix, user) = collect("Grade", n_frames, [
            ("exposure", exposure, *per_frame), ("contrast", contrast, *per_frame), ("pivot", pivot, *per_frame), ("slope", slope, *per_channel),
            ("offset", offset, *per_channel), ("power", power, *per_channel), ("gamma", gamma, *per_channel),
            ("white_balance", white_balance, *per_channel), ("saturation", saturation, *per_frame), ("hue", hue, *per_frame),
            ("bias", bias, *per_channel), ("lut_mix", lut_mix, *per_frame), ("matrix", matrix, (3, 3), False)])
        if np.any(power <= 0) or (gamma is not None and np.any(gamma <= 0)):
            raise ValueError("Grade: power and gamma must be greater than 0")
        if np.any(mix < 0) or np.any(mix > 1):
            raise ValueError("Grade: lut_mix must lie in [0, 1]")

        rows = np.zeros((n, GRADE_ROW), np.float64)
        gain = np.exp2(exposure) * slope * (1.0 if wb is None else wb)
        rows[:, _SLOPE:_SLOPE + 3] = gain * contrast
        rows[:, _OFFSET:_OFFSET + 3] = offset * contrast + pivot * (1.0 - contrast)
        rows[:, _POWER:_POWER + 3] = power * (1.0 if gamma is None else 1.0 / gamma)
        m = hue_matrix(hue[:, 0]) @ saturation_matrix(saturation[:, 0])
        if user is not None:
            m = m @ user
        rows[:, _MATRIX:_MATRIX + 9] = np.broadcast_to(m, (n, 3, 3)).reshape(n, 9)
        rows[:, _BIAS:_BIAS + 3] = bias
        rows[:, _MIX] = mix[:, 0]
        with np.errstate(over="ignore"):
            table = rows.astype(np.float32)
        if not np.all(np.isfinite(table)):
            raise ValueError("Grade: the parameters overflow float32")
        if np.any(table[:, _POWER:_POWER + 3] <= 0):
            raise ValueError("Grade: power / gamma underflows float32")
        self._init(table, _check_lut(lut))

    def _init(self, table, lut):
        self.table = table
        self.table.setflags(write=False)
        self.lut = lut
        ident = np.zeros(GRADE_ROW, np.float32)
        ident[[0, 1, 2, 6, 7, 8, 9, 13, 17]] = 1
        self.identity = (table[:, :_MIX] == ident[:_MIX]).all(axis=1) & ((table[:, _MIX] == 0) | (lut is None))
        self._device = {}

    @classmethod
    def from_table(cls, table, lut=None):
        """A grade from a finished row table [n, 24] (validated as the constructor validates) and an optional LUT."""
        table = np.array(host64(table), np.float32)
        if table.ndim != 2 or table.shape[1] != GRADE_ROW or table.shape[0] < 1:
            raise ValueError(f"Grade.from_table: the table must be [n, {GRADE_ROW}], got {table.shape}")
        if not np.all(np.isfinite(table)):
            raise ValueError("Grade.from_table: the table holds non-finite values")
        if np.any(table[:, _POWER:_POWER + 3] <= 0):
            raise ValueError("Grade.from_table: power must be greater than 0")
        if np.any(table[:, _MIX] < 0) or np.any(table[:, _MIX] > 1):
            raise ValueError("Grade.from_table: lut_mix must lie in [0, 1]")
        self = cls.__new__(cls)
        self._init(table, _check_lut(lut))
        return self

    from_tables = from_table  # (the name Lens and Feedback give theirs: ``from_tables(*x.tables())`` is x for the three)

    @property
    def lut_n(self):
        return 0 if self.lut is None else self.lut.shape[0]

    def __repr__(self):
        return f"Grade({self._count()}, lut={'none' if self.lut is None else self.lut_n}, identity={int(self.identity.sum())})"

    def rows(self, device):
        """The row table as a float32 tensor [n, 24] on ``device`` (uploaded once per device)."""
        device = th.device(device)
        key = ("rows", str(device))
        if key not in self._device:
            self._device[key] = th.from_numpy(np.array(self.table)).to(device)
        return self._device[key]

    def lut_table(self, device):
        """The LUT in the device layout of maua_grade_f32, float32 [N^3, 4] (entries padded to 16 bytes), or None."""
        if self.lut is None:
            return None
        device = th.device(device)
        key = ("lut", str(device))
        if key not in self._device:
            padded = np.zeros((self.lut_n ** 3, 4), np.float32)
            padded[:, :3] = self.lut.reshape(-1, 3)
            self._device[key] = th.from_numpy(padded).to(device)
        return self._device[key]

    def tables(self):
        """(table, lut): ``Grade.from_table(*g.tables())`` is g."""
        return self.table, self.lut

    def _block(self, lo, hi):
        return Grade.from_table(self.table[lo:hi], self.lut)

    def with_lut(self, lut, lut_mix=1.0):
        """This grade with ``lut`` attached at ``lut_mix`` on every row; refused when it has a LUT already."""
        if self.lut is not None:
            raise ValueError("Grade.with_lut: the grade has a LUT already")
        if not (isinstance(lut_mix, (int, float)) and 0 <= lut_mix <= 1):
            raise ValueError("Grade: lut_mix must lie in [0, 1]")
        table = np.array(self.table)
        table[:, _MIX] = lut_mix
        return Grade.from_table(table, lut)


SPEC_KEYS = ("exposure", "contrast", "pivot", "slope", "offset", "power", "gamma", "saturation", "hue", "bias")


def parse_spec(text):
    """A static grade as text, ``"exposure=0.3,saturation=1.2,gamma=0.9,hue=15"`` (the --grade flag), -> the keyword arguments of Grade.
    Keys: SPEC_KEYS; a value is a number, or three numbers joined by ``:`` for the per-channel ones (``slope=1.1:1:0.9``)."""
    return frame_table.parse_spec("--grade", text, {k: (1, 3) if k in ("slope", "offset", "power", "gamma", "bias") else (1,) for k in SPEC_KEYS})


def _check_lut(lut):
    if lut is None:
        return None
    if isinstance(lut, (str, bytes)) or hasattr(lut, "__fspath__"):
        lut = load_cube(lut)
    table = np.ascontiguousarray(host64(lut), np.float32)
    if table.ndim != 4 or table.shape[3] != 3 or not (table.shape[0] == table.shape[1] == table.shape[2]) or not LUT_MIN <= table.shape[0] <= LUT_MAX:
        raise ValueError(f"Grade: a LUT is [N, N, N, 3] with {LUT_MIN} <= N <= {LUT_MAX}, got {table.shape}")
    if not np.all(np.isfinite(table)):
        raise ValueError("Grade: the LUT holds non-finite values")
    table.setflags(write=False)
    return table


def lut_from_function(fn, n):
    """The table [n, n, n, 3] (float32, indexed [blue, green, red]) of ``fn``: an array [..., 3] of (r, g, b) in [0, 1] -> [..., 3]."""
    if isinstance(n, bool) or int(n) != n or not LUT_MIN <= int(n) <= LUT_MAX:
        raise ValueError(f"lut_from_function: n must be an integer in {LUT_MIN} .. {LUT_MAX}, got {n!r}")
    g = np.linspace(0.0, 1.0, int(n))
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    out = np.asarray(fn(np.stack([r, gg, b], axis=-1)), np.float64)
    if out.shape != (n, n, n, 3):
        raise ValueError(f"lut_from_function: fn returned shape {out.shape} for an input of shape {(n, n, n, 3)}")
    return _check_lut(out)


def save_cube(path, table, title=None):
    """Write ``table`` [N, N, N, 3] as a 3-D .cube file (red fastest, domain 0 .. 1)."""
    table = _check_lut(table)
    n = table.shape[0]
    with open(path, "w") as f:
        if title is not None:
            f.write('TITLE "%s"\n' % str(title).replace('"', "'"))
        f.write(f"LUT_3D_SIZE {n}\nDOMAIN_MIN 0.0 0.0 0.0\nDOMAIN_MAX 1.0 1.0 1.0\n")
        for r, g, b in table.reshape(-1, 3):
            f.write(f"{float(r):.9g} {float(g):.9g} {float(b):.9g}\n")  # (9 significant digits: a float32 round trip is exact)


def load_cube(path):
    """Read a 3-D .cube file -> float32 [N, N, N, 3] (indexed [blue, green, red]).  Understood: TITLE, LUT_3D_SIZE, DOMAIN_MIN / DOMAIN_MAX
    (0 0 0 / 1 1 1 only), comments (#) and blank lines.  Refused with the reason: 1-D LUTs, another domain, unknown keywords, a wrong number
    of entries, non-finite values."""
    n = None
    values = []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            word = line.split()[0]
            where = f"{path}:{number}"
            if word == "TITLE":
                continue
            if word == "LUT_1D_SIZE" or word == "LUT_1D_INPUT_RANGE":
                raise ValueError(f"{where}: 1-D .cube LUTs are not supported (only LUT_3D_SIZE tables)")
            if word == "LUT_3D_SIZE":
                parts = line.split()
                if len(parts) != 2 or not parts[1].isdigit() or not LUT_MIN <= int(parts[1]) <= LUT_MAX:
                    raise ValueError(f"{where}: LUT_3D_SIZE must be an integer in {LUT_MIN} .. {LUT_MAX}")
                n = int(parts[1])
                continue
            if word in ("DOMAIN_MIN", "DOMAIN_MAX", "LUT_3D_INPUT_RANGE"):
                try:
                    nums = [float(p) for p in line.split()[1:]]
                except ValueError:
                    raise ValueError(f"{where}: {word} wants numbers") from None
                want = {"DOMAIN_MIN": [0.0] * 3, "DOMAIN_MAX": [1.0] * 3, "LUT_3D_INPUT_RANGE": [0.0, 1.0]}[word]
                if nums != want:
                    raise ValueError(f"{where}: {line!r}: only the domain 0 .. 1 is supported")
                continue
            if word[0].isalpha() or word[0] == "_":
                raise ValueError(f"{where}: unknown keyword {word!r}")
            try:
                rgb = [float(p) for p in line.split()]
            except ValueError:
                raise ValueError(f"{where}: {line!r} is not three numbers") from None
            if len(rgb) != 3 or not all(math.isfinite(v) for v in rgb):
                raise ValueError(f"{where}: {line!r} is not three finite numbers")
            values.append(rgb)
    if n is None:
        raise ValueError(f"{path}: no LUT_3D_SIZE")
    if len(values) != n ** 3:
        raise ValueError(f"{path}: LUT_3D_SIZE {n} wants {n ** 3} entries, the file has {len(values)}")
    return _check_lut(np.asarray(values, np.float64).reshape(n, n, n, 3))
