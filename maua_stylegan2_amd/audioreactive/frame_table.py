"""What ar.Grade, ar.Lens and ar.Feedback share (host only: numpy and torch, no device call): an effect on the generator's fp32 image is a
table with one parameter row per rendered frame, or one row for all of them.  Here are the one rule of their constructors' arguments
(``collect``), the base class of the three (``FrameTable``: rows, identity, slice, tables) and the parser of their static flags
(``parse_spec``).  Each class keeps what is its own: the arithmetic of its rows, its validation, its device operands.
"""
import numpy as np
import torch as th


def host64(value):
    """``value`` (a number, a sequence, a numpy array, a torch tensor on any device) as a float64 numpy array on the host."""
    if isinstance(value, th.Tensor):
        return value.detach().to("cpu", th.float64).numpy()
    return np.asarray(value, np.float64)


def _forms(shape, narrow):
    dims = ", ".join(str(s) for s in shape)
    wide = [] if shape == (1,) else [{(2,): "a pair", (3,): "a triple"}.get(shape, f"[{dims}]"), f"[n_frames, {dims}]"]
    return " | ".join((["a scalar", "[n_frames]", "[n_frames, 1]"] if narrow else []) + wide)


def collect(cls, n_frames, specs):
    """The arguments of a constructor -> (n, arrays).  ``cls``: the class name, for the messages; ``specs``: (name, value, width,
    narrow_ok) in the order of the signature.  An argument of ``width`` w is one row — [w], or a scalar for w = 1 — or a per-frame
    sequence [n, w] ([n] for w = 1); ``narrow_ok`` also accepts a scalar, [n] and [n, 1] for w > 1 (one value for all channels).  ``width``
    may be a shape: (3, 3) takes [3, 3] or [n, 3, 3].  A value of None stays None.  The sequences must agree in length with each other
    and with ``n_frames`` where that is given; n is that length, 1 without a sequence (one row serves every frame, whatever n_frames
    says).  Returns the float64 arrays as [n or 1, w] ([n or 1, 1] for a narrow value).  Refused: a bad n_frames, non-finite values, an
    empty sequence, any other shape, lengths that differ."""
    if n_frames is not None and (isinstance(n_frames, bool) or int(n_frames) != n_frames or int(n_frames) < 1):
        raise ValueError(f"{cls}: n_frames must be a positive integer, got {n_frames!r}")
    lengths, arrays = {}, []
    for name, value, width, narrow_ok in specs:
        if value is None:
            arrays.append(None)
            continue
        a = host64(value)
        shape = (width,) if isinstance(width, int) else tuple(width)
        narrow = narrow_ok or shape == (1,)
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{cls}: {name} holds non-finite values")
        if a.size == 0:
            raise ValueError(f"{cls}: {name} is empty (shape {a.shape}): a sequence needs an entry per frame")
        if narrow and a.ndim == 0:
            a = a.reshape(1, 1)
        elif shape != (1,) and a.shape == shape:
            a = a[None]
        elif a.ndim == len(shape) + 1 and a.shape[1:] == shape:
            lengths[name] = a.shape[0]
        elif narrow and (a.ndim == 1 or (a.ndim == 2 and a.shape[1] == 1)):
            lengths[name] = a.shape[0]
            a = a.reshape(-1, 1)
        else:
            raise ValueError(f"{cls}: {name} of shape {a.shape} ({a.ndim} dimensions) is none of {_forms(shape, narrow)}")
        arrays.append(a)
    # (the length the others must say: n_frames where it is given, else that of the first sequence)
    other, want = next(iter(lengths.items()), (None, 1)) if n_frames is None else ("n_frames", int(n_frames))
    for name, n in lengths.items():
        if n != want:
            raise ValueError(f"{cls}: {name} has {n} entries, {other} says {want}")
    return (want if lengths else 1), arrays


class FrameTable:
    """The base of Grade, Lens and Feedback: ``table`` (read-only, a row per frame or one row), and what follows from its row count alone.
    A subclass sets ``table`` and its per-row identity mask (the attribute named by ``MASK``) in its ``_init``, and defines ``tables()`` —
    the arguments of its ``from_tables`` that give this object back — and ``_block(lo, hi)``."""

    MASK = "identity"

    @property
    def n_rows(self):
        return self.table.shape[0]

    def __len__(self):
        return self.n_rows

    @property
    def is_identity(self):
        """True when every row is the identity: the render then delivers the frames bit for bit as they were (and a lens or a feedback
        launches nothing)."""
        return bool(getattr(self, self.MASK).all())

    def _count(self):
        """"1 row" / "N rows", for the reprs."""
        return f"{self.n_rows} row{'s' if self.n_rows != 1 else ''}"

    def slice(self, lo, hi):
        """The effect of the frames [lo, hi), with what belongs to the whole table kept (a LUT, a lens's plan_max, a feedback's mode): a
        one-row table is its own slice."""
        name = type(self).__name__
        if self.n_rows == 1:
            return self
        if not 0 <= lo <= hi <= self.n_rows:
            raise ValueError(f"{name}.slice: [{lo}, {hi}) is not inside the {self.n_rows} rows")
        if hi == lo:
            raise ValueError(f"{name}.slice: an empty slice")
        return self._block(lo, hi)


_COUNT_WORDS = {1: "one number", 2: "two numbers", 3: "three numbers"}


def parse_spec(flag, text, counts, names=None):
    """A static effect as text, ``"key=value,key=value"`` (the flag ``flag``, e.g. "--lens"), -> the keyword arguments of its class.
    ``counts``: key -> the allowed numbers of ``:``-joined values, e.g. (1,), (1, 3), (3,); ``names``: key -> its allowed words.  A
    value comes back as a float (one number), a list (several) or a str (a word)."""
    names = names or {}
    keys = tuple(counts) + tuple(names)
    out = {}
    for part in str(text).split(","):
        part = part.strip()
        if not part:
            continue
        key, eq, value = part.partition("=")
        key, value = key.strip(), value.strip()
        if not eq or key not in keys:
            raise ValueError(f"{flag} {text!r}: {part!r} is not key=value with a key of {', '.join(keys)}")
        if key in out:
            raise ValueError(f"{flag} {text!r}: {key} is given twice")
        if key in names:
            if value not in names[key]:
                raise ValueError(f"{flag} {text!r}: {key} is one of {', '.join(names[key])}, not {value!r}")
            out[key] = value
            continue
        try:
            nums = [float(v) for v in value.split(":")]
        except ValueError:
            raise ValueError(f"{flag} {text!r}: {value!r} is not a number") from None
        if len(nums) not in counts[key]:
            takes = " or ".join(_COUNT_WORDS[c] for c in counts[key]) + (" joined by ':'" if max(counts[key]) > 1 else "")
            raise ValueError(f"{flag} {text!r}: {key} takes {takes}")
        out[key] = nums[0] if len(nums) == 1 else nums
    if not out:
        raise ValueError(f"{flag} {text!r} names no parameter")
    return out
