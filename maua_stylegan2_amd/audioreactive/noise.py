"""Synthesised noise slots: a noise input described by a recipe instead of a resident ``[n_frames, 1, h, w]`` sequence.

Almost everything an audio-reactive plugin does with noise — blending short loops by an envelope, gating a fast and a slow field by onsets
and a static mask, cross-fading two fields — is

    noise[frame, y, x] = gain * sum_k envelope_k[frame] * mask_k[y, x] * field_k[(frame + phase_k) mod P_k, y, x]

with at most four terms.  ``NoiseSynth`` holds such a recipe on the device; ``get_noise`` may return it in place of a tensor.  The generator
then produces the maps of each batch with one launch of ``maua_noise_synth_f32`` (include/maua_hip.h, csrc/noise_synth.hip) — inside the
captured forward on the graph lanes, or per batch on the eager path, the same kernel and the same bits either way — so a 1024^2 layer costs
the memory of its loops (a 110-frame loop: 0.45 GB) instead of 4 MB per frame of the track (36 GB for 9000 frames).

There is no helper for building a loop because none is needed: ``ar.gaussian_filter`` is circular in time, so
``ar.gaussian_filter(torch.randn(P, 1, h, w, device="cuda"), sigma)`` already is a seamless loop of period P, and ``ar.perlin_noise`` tiles
in time by default.
"""
import math

import torch as th

from .. import _lib

__all__ = ["NoiseSynth", "noise_term"]

MAX_TERMS = _lib.NOISE_SYNTH_MAX_TERMS
STD_SAMPLE_FRAMES = 16  # ``NoiseSynth.std`` looks at no more frames than this


class _Term:
    """One term of a recipe as the caller gave it (``noise_term``); validated against a map size by ``NoiseSynth``."""

    def __init__(self, bank, envelope, mask, phase):
        self.bank, self.envelope, self.mask, self.phase = bank, envelope, mask, phase


def noise_term(bank, envelope=None, mask=None, phase=0):
    """One term ``envelope[frame] * mask[y, x] * bank[(frame + phase) mod P, y, x]`` of a ``NoiseSynth``.

    ``bank``: a loop ``[P, 1, h, w]`` or ``[P, h, w]``, one static map ``[h, w]`` (P = 1), or the string ``"randn"`` = a fresh seeded
    N(0,1) map per frame (the counter-based noise of ``randomize_noise``: a pure function of the recipe's seed, the absolute frame and the
    slot).  ``envelope``: ``[n_frames]`` or None (= 1).  ``mask``: ``[h, w]`` or None (= 1).  ``phase``: integer frame offset into the loop."""
    return _Term(bank, envelope, mask, phase)


def _checked_terms(height, width, terms, gain, seed):
    """Host-side validation of a recipe: touches shapes only, never a device.  Returns [(bank or None, envelope, mask, period, phase)] with
    the tensors as given (reshaped, not moved) and the envelope length (None: no term has one)."""
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f"NoiseSynth: map size {height} x {width} must be positive")
    terms = list(terms)
    if not 1 <= len(terms) <= MAX_TERMS:
        raise ValueError(f"NoiseSynth takes 1 to {MAX_TERMS} terms, got {len(terms)}")
    if isinstance(gain, bool) or not isinstance(gain, (int, float)) or not math.isfinite(gain):
        raise ValueError(f"NoiseSynth: gain must be a finite number, got {gain!r}")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64):
        raise ValueError(f"NoiseSynth: seed must be an integer in [0, 2^64), got {seed!r}")
    out, n_env, n_randn = [], None, 0
    for k, t in enumerate(terms):
        if not isinstance(t, _Term):
            raise TypeError(f"NoiseSynth: term {k} is a {type(t).__name__}; build terms with ar.noise_term(...)")
        bank, period = None, 1
        if isinstance(t.bank, str):
            if t.bank != "randn":
                raise ValueError(f"NoiseSynth: term {k}: the only bank named by a string is \"randn\", got {t.bank!r}")
            n_randn += 1
        elif isinstance(t.bank, th.Tensor):
            shape = tuple(t.bank.shape)
            if len(shape) == 4 and shape[1:] == (1, height, width) or len(shape) == 3 and shape[1:] == (height, width):
                period = shape[0]
            elif shape != (height, width):
                raise ValueError(f"NoiseSynth: term {k}: bank {shape} is not [P, 1, {height}, {width}], [P, {height}, {width}] or "
                                 f"[{height}, {width}]")
            if period < 1:
                raise ValueError(f"NoiseSynth: term {k}: a loop needs at least one frame (P >= 1), got {shape}")
            if period * height * width >= 2 ** 40 or period >= 2 ** 31:
                raise ValueError(f"NoiseSynth: term {k}: bank {shape} is too large")
            bank = t.bank.reshape(period, height * width)
        else:
            raise TypeError(f"NoiseSynth: term {k}: bank must be a tensor or \"randn\", got {type(t.bank).__name__}")
        envelope = t.envelope
        if envelope is not None:
            if not isinstance(envelope, th.Tensor) or envelope.dim() != 1 or envelope.shape[0] < 1:
                raise ValueError(f"NoiseSynth: term {k}: envelope must be a [n_frames] tensor, got "
                                 f"{tuple(envelope.shape) if isinstance(envelope, th.Tensor) else type(envelope).__name__}")
            if n_env is not None and envelope.shape[0] != n_env:
                raise ValueError(f"NoiseSynth: term {k}: envelope has {envelope.shape[0]} frames, an earlier term's has {n_env}")
            n_env = int(envelope.shape[0])
        mask = t.mask
        if mask is not None:
            if not isinstance(mask, th.Tensor) or tuple(mask.shape) != (height, width):
                raise ValueError(f"NoiseSynth: term {k}: mask must be a [{height}, {width}] tensor, got "
                                 f"{tuple(mask.shape) if isinstance(mask, th.Tensor) else type(mask).__name__}")
            mask = mask.reshape(height * width)
        if isinstance(t.phase, bool) or not isinstance(t.phase, int):
            raise TypeError(f"NoiseSynth: term {k}: phase must be an integer, got {t.phase!r}")
        out.append((bank, envelope, mask, int(period), int(t.phase) % int(period)))
    if n_randn > 1:
        raise ValueError(f"NoiseSynth: at most one \"randn\" term per recipe, got {n_randn}")
    return out, n_env


class NoiseSynth:
    """``NoiseSynth(height, width, terms, gain=1.0, seed=None)`` — the recipe of one noise input (see the module docstring); ``terms`` is a
    list of 1 to 4 ``ar.noise_term(...)``.  ``seed`` feeds the ``"randn"`` term (None: one draw from torch's CPU generator at construction,
    so ``torch.manual_seed`` makes a job repeatable).  The tensors are moved to ``device`` once, as contiguous fp32, and kept there."""

    def __init__(self, height, width, terms, gain=1.0, seed=None, device="cuda"):
        checked, n_env = _checked_terms(height, width, terms, gain, seed)
        self.height, self.width, self.gain = int(height), int(width), float(gain)
        if seed is None:
            seed = int(th.randint(0, 2 ** 63 - 1, (1,), dtype=th.int64).item()) if any(t[0] is None for t in checked) else 0
        self.seed = int(seed)
        self.device = th.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = th.device("cuda", th.cuda.current_device())
        put = lambda t: None if t is None else t.detach().to(self.device, th.float32).contiguous()  # noqa: E731
        # per term: (bank [P, hw] or None = "randn", the FULL envelope or None, mask [hw] or None, period, phase)
        self._terms = [(put(b), put(e), put(m), period, phase) for b, e, m, period, phase in checked]
        self._env_len = n_env
        self.offset = 0          # absolute frame of local frame 0: advanced by ``window``
        self._lo, self._hi = 0, n_env  # the part of the envelopes this recipe covers

    # ------------------------------------------------------------------ description
    @property
    def n_frames(self):
        """Frames the recipe covers, or None when no term has an envelope (it then fits a render of any length)."""
        return None if self._env_len is None else self._hi - self._lo

    @property
    def shape(self):
        return (self.n_frames or 1, 1, self.height, self.width)

    @property
    def hw(self):
        return self.height * self.width

    def _copy(self):
        other = object.__new__(NoiseSynth)
        other.__dict__.update(self.__dict__)
        return other

    def window(self, lo, hi):
        """The recipe of frames [lo, hi) of this one: the envelopes are cut and the frame offset moves on by ``lo``, so loop phases and the
        counter-based maps continue where the full sequence has them.  Shares the banks; copies nothing."""
        lo, hi = int(lo), int(hi)
        n = self.n_frames
        if lo < 0 or hi < lo or (n is not None and hi > n):
            raise ValueError(f"NoiseSynth.window: [{lo}, {hi}) is outside the recipe's {n} frames")
        other = self._copy()
        other.offset = self.offset + lo
        if n is not None:
            other._lo, other._hi = self._lo + lo, self._lo + hi
        return other

    def with_gain(self, gain):
        """The same recipe (shared tensors) with another gain — a plugin's own normalisation: ``r.with_gain(1 / (2.5 * float(r.std())))``."""
        if isinstance(gain, bool) or not isinstance(gain, (int, float)) or not math.isfinite(gain):
            raise ValueError(f"NoiseSynth: gain must be a finite number, got {gain!r}")
        other = self._copy()
        other.gain = float(gain)
        return other

    def rows(self, frame):
        """Host arithmetic of local ``frame``: (per term the bank row, None for the ``"randn"`` term; the absolute = counter frame)."""
        absolute = self.offset + int(frame)
        return [None if bank is None else (absolute + phase) % period for bank, _, _, period, phase in self._terms], absolute

    def table_entry(self, dst, slot, first=0):
        """The maua_noise_synth_slot_t of this recipe with its envelopes starting at local frame ``first``, writing ``dst`` (a device
        pointer) for noise slot ``slot``.  Launch it with frame0 = ``offset + first``."""
        entry = _lib.NoiseSynthSlot()
        entry.dst, entry.hw, entry.slot, entry.n_terms = int(dst), self.hw, int(slot), len(self._terms)
        entry.gain, entry.seed = self.gain, self.seed
        for k, (bank, envelope, mask, period, phase) in enumerate(self._terms):
            t = entry.term[k]
            t.bank = None if bank is None else bank.data_ptr()
            t.envelope = None if envelope is None else envelope.data_ptr() + 4 * (self._lo + int(first))
            t.mask = None if mask is None else mask.data_ptr()
            t.period, t.phase = period, phase
        return entry

    # ------------------------------------------------------------------ evaluation
    def frames(self, frame0, batch, slot=0):
        """Maps of local frames [frame0, frame0 + batch): ``[batch, 1, h, w]``, one launch of maua_noise_synth_f32.  ``slot`` only names
        the counter word of a ``"randn"`` term (the noise slot the maps are for)."""
        frame0, batch = int(frame0), int(batch)
        n = self.n_frames
        if frame0 < 0 or batch < 1 or (n is not None and frame0 + batch > n) or self.offset + frame0 + batch > 2 ** 31:
            raise ValueError(f"NoiseSynth.frames: [{frame0}, {frame0 + batch}) is outside the recipe's {n} frames")
        if self.device.type != "cuda":
            raise RuntimeError("NoiseSynth.frames needs the recipe on a HIP device; there is no CPU fallback")
        out = th.empty((batch, 1, self.height, self.width), dtype=th.float32, device=self.device)
        host = self.table_entry(out.data_ptr(), slot, first=frame0)
        table = th.frombuffer(bytearray(bytes(host)), dtype=th.uint8).to(self.device)
        _lib.call("maua_noise_synth_f32", table, 1, batch, self.offset + frame0, None)
        table.record_stream(th.cuda.current_stream(self.device))
        return out

    def materialize(self, n_frames=None, slot=0, chunk=64):
        """The whole ``[n_frames, 1, h, w]`` sequence (StyleGAN1, inspection): what the recipe exists to avoid at high resolutions."""
        n = self.n_frames if n_frames is None else int(n_frames)
        if n is None:
            raise ValueError("NoiseSynth.materialize: a recipe without envelopes has no length of its own; pass n_frames")
        return th.cat([self.frames(f, min(chunk, n - f), slot) for f in range(0, n, chunk)])

    def std(self, n_frames=None):
        """Amplitude (standard deviation, a device scalar) over at most STD_SAMPLE_FRAMES frames spread evenly over the first ``n_frames``
        (default: the recipe's own length, or its longest loop)."""
        n = n_frames if n_frames is not None else self.n_frames
        if n is None:
            n = max(period for _, _, _, period, _ in self._terms)
        n = int(n)
        if n < 1 or (self.n_frames is not None and n > self.n_frames):
            raise ValueError(f"NoiseSynth.std: {n} frames are outside the recipe's {self.n_frames}")
        count = min(n, STD_SAMPLE_FRAMES)
        picks = sorted({(2 * j + 1) * n // (2 * count) for j in range(count)})
        return th.cat([self.frames(f, 1) for f in picks]).std()

    # ------------------------------------------------------------------ moving between processes (generate(): one process per GPU)
    def structure(self):
        """Everything but the tensors, picklable: with ``tensors()`` enough to rebuild the recipe on another rank."""
        return {"height": self.height, "width": self.width, "gain": self.gain, "seed": self.seed, "offset": self.offset,
                "env": (self._env_len, self._lo, self._hi),
                "terms": [(None if b is None else tuple(b.shape), e is not None, m is not None, period, phase)
                          for b, e, m, period, phase in self._terms]}

    def tensors(self):
        return [t for term in self._terms for t in term[:3] if t is not None]

    @classmethod
    def from_structure(cls, structure, device, tensors=None):
        """The recipe ``structure`` describes on ``device``, around ``tensors`` (in ``tensors()`` order) or freshly allocated ones to be
        filled by the caller."""
        self = object.__new__(cls)
        self.height, self.width, self.gain = structure["height"], structure["width"], structure["gain"]
        self.seed, self.offset = structure["seed"], structure["offset"]
        self._env_len, self._lo, self._hi = structure["env"]
        self.device = th.device(device)
        given = iter(tensors) if tensors is not None else None
        new = lambda shape: next(given) if given is not None else th.empty(shape, dtype=th.float32, device=self.device)  # noqa: E731
        self._terms = []
        for bank_shape, has_env, has_mask, period, phase in structure["terms"]:
            self._terms.append((None if bank_shape is None else new(bank_shape), new((self._env_len,)) if has_env else None,
                                new((self.height * self.width,)) if has_mask else None, period, phase))
        return self
