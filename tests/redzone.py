"""Red-zone (canary) windows for GPU tests that call the C ABI directly.

Every operand, output and workspace buffer of a call is a window of exactly the size the header promises inside a larger allocation whose
surroundings (RED dwords either side) hold a quiet NaN with a recognisable payload; outputs are pre-filled with the same pattern.  After the
launch `Guard.check` asserts that the red zones are bit-identical (no write outside any buffer), that no named output element is still the
canary (every element written) and that every named floating-point output is finite (an operand read outside its buffer multiplies a NaN
into the result)."""
import numpy as np
import torch

RED = 4096
CANARY_BITS = 0x7FC0BEEF  # a quiet NaN with a payload nothing computes
_WIDE = (torch.float64, torch.int64)
_DTYPES = (torch.float32, torch.uint8, torch.float64, torch.int32, torch.float16)


class Guard:
    """Windows of exact size between red zones, all in one registry so that one call checks every buffer of a launch."""

    def __init__(self, dev):
        self.dev = dev
        self.items = []
        self.dtypes = {}

    def _alloc(self, n, dtype):
        assert dtype in _DTYPES
        if dtype == torch.uint8:
            n_f = (n + 3) // 4
        elif dtype == torch.float16:
            n_f = (n + 1) // 2
        elif dtype in _WIDE:
            n_f = 2 * n
        else:
            n_f = n
        raw = torch.full((RED + n_f + RED,), CANARY_BITS, dtype=torch.int32, device=self.dev)
        return raw, n_f

    def inp(self, t, name, dtype=torch.float32):
        """A copy of ``t`` (any shape; a tensor or an array) as ``dtype`` in a guarded window."""
        t = torch.as_tensor(t).to(self.dev, dtype).contiguous()
        raw, n_f = self._alloc(t.numel(), dtype)
        view = raw[RED: RED + n_f].view(dtype)[:t.numel()]
        view.copy_(t.reshape(-1))
        self.items.append((name, raw, n_f, False))
        self.dtypes[name] = dtype
        return view.view(t.shape)

    def out(self, shape, name, dtype=torch.float32):
        """An output / workspace window, pre-filled with the canary."""
        n = int(np.prod(shape))
        raw, n_f = self._alloc(n, dtype)
        self.items.append((name, raw, n_f, True))
        self.dtypes[name] = dtype
        if dtype in (torch.uint8, torch.float16):  # (n need not fill the last dword)
            return raw[RED: RED + n_f].view(dtype)[:n].view(shape)
        return raw[RED: RED + n_f].view(dtype).view(shape)

    def untouched(self, name):
        """True when the window ``name`` still holds nothing but the canary (a refused call must not have launched)."""
        torch.cuda.synchronize(self.dev)
        return all(bool((raw[RED: RED + n_f] == CANARY_BITS).all()) for nm, raw, n_f, _ in self.items if nm == name)

    def check(self, written=(), nonfinite_ok=()):
        """Red zones intact everywhere; the outputs named in ``written`` hold no canary and only finite values (``nonfinite_ok``: outputs of
        a case that feeds non-finite input on purpose)."""
        torch.cuda.synchronize(self.dev)
        for name, raw, n_f, is_out in self.items:
            lo, hi = raw[:RED], raw[RED + n_f:]
            assert bool((lo == CANARY_BITS).all()), f"{name}: write BELOW the buffer ({int((lo != CANARY_BITS).sum())} dwords)"
            assert bool((hi == CANARY_BITS).all()), f"{name}: write BEYOND the buffer ({int((hi != CANARY_BITS).sum())} dwords)"
            if is_out and name in written:
                body = raw[RED: RED + n_f]
                dtype = self.dtypes[name]
                if dtype in _WIDE:  # an element is unwritten when BOTH of its dwords are still the canary
                    stale = (body.view(-1, 2) == CANARY_BITS).all(dim=1)
                else:
                    stale = body == CANARY_BITS
                assert not bool(stale.any()), f"{name}: {int(stale.sum())} elements never written"
                if name in nonfinite_ok or dtype == torch.int32:
                    continue
                if dtype == torch.float16:  # (half a dword of canary stays behind an odd count: a NaN by design)
                    halves = body.view(torch.float16)
                    fl = halves if bool((halves.view(torch.int16)[-1:] != (CANARY_BITS >> 16)).all()) else halves[:-1]
                else:
                    fl = body.view(torch.float64) if dtype == torch.float64 else body.view(torch.float32)
                assert bool(torch.isfinite(fl).all()), f"{name}: non-finite output (an operand was read outside its buffer?)"
