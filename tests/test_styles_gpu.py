"""GPU: maua_style_affine_f32 / maua_demod_f32 (csrc/styles.hip) through the C ABI against numpy float64, written from the formulas of
include/maua_hip.h:

    latent' = trunc_latent + trunc[b] * (latent - trunc_latent)                      (trunc != NULL; trunc_latent == NULL: a zero mean)
    s[b, s_off + i] = sum_j mod_w[i, j] latent'[b, lat_idx, j] / sqrt(style_dim) + mod_b[i]
    d[d_off + b cout + o] = rsqrt(wscale^2 sum_i wsq[o, i] s[b, s_off + i]^2 + 1e-8)

Tolerances (from the float64 reference, never from the device result):
  affine, per element:  (style_dim/64 + 14) 2^-24 (sum_j |w_ij| |l'_j| / sqrt(style_dim) + |b_i|) — a style_dim/64-long fma chain per lane,
      6 butterfly adds, the scale, the bias add and the 3 roundings of the lerp;
  demod, relative:  (ceil(cin/64) + 12) 2^-24 / 2 + 4 * 2^-24 — half the relative error of a sum of non-negative terms (wsq is drawn as
      squares, as real sums of squared taps are) + rsqrtf; the reference is fed the s that was uploaded, so this tests demod alone.
Every operand, table, output sits between red zones (tests/redzone.py); unused columns of s and the gaps between the blocks of d must
still hold the canary afterwards."""
import ctypes

import numpy as np
import pytest
import torch

from maua_stylegan2_amd import _lib
from maua_stylegan2_amd.models.stylegan2 import _style_table
from redzone import CANARY_BITS, Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

U = 2.0 ** -24
EINVAL = -22
ROWS = (1, 3, 15, 16, 17, 40, 1000, 1024)


class _Affine:
    """One affine table between red zones: entries (cin, lat_idx) laid out in a batch row of s from column ``s_off0`` on, ``gap`` unused
    columns behind every slice (so most offsets are no multiple of 4 and the row ends in unused columns)."""

    def __init__(self, gpu, style_dim, layers, seed, s_off0=3, gap=5):
        self.gpu, self.style_dim, self.g = gpu, style_dim, Guard(gpu)
        r = np.random.default_rng(seed)
        self.host, entries, off = [], [], s_off0
        for k, (cin, lat_idx) in enumerate(layers):
            w = r.standard_normal((cin, style_dim)).astype(np.float32)
            b = (1 + 0.1 * r.standard_normal(cin)).astype(np.float32)
            entries.append(dict(mod_w=self.g.inp(w, f"mod_w{k}"), mod_b=self.g.inp(b, f"mod_b{k}"), wsq=None, cin=cin, cout=0, lat_idx=lat_idx,
                                s_off=off, d_off=0, wscale=1.0))
            self.host.append((w.astype(np.float64), b.astype(np.float64), lat_idx, off))
            off += cin + gap
        self.s_stride, self.n, self.max_cin = off, len(layers), max(c for c, _ in layers)
        self.table = self.g.inp(_style_table(entries, "cpu"), "table", dtype=torch.uint8)

    def run(self, batch, n_latent, lat=None, trunc=None, tl=None, src=None, name="s"):
        s = self.g.out((batch, self.s_stride), name)
        rc = _lib.load().maua_style_affine_f32(_lib.ptr(lat), batch, n_latent, self.style_dim, _lib.ptr(trunc), _lib.ptr(tl), self.table.data_ptr(),
                                               self.n, self.max_cin, s.data_ptr(), self.s_stride, src, _lib.stream_ptr(self.gpu))
        assert rc == 0, rc
        return s

    def check(self, s, lat, trunc=None, tl=None, label=""):
        """``s`` against float64 at the derived bound; columns outside every slice still the canary.  ``lat`` [batch, n_latent, style_dim],
        ``trunc`` [batch] / ``tl`` [style_dim] as uploaded (float32 arrays).  Returns the largest error / bound."""
        self.g.check()
        got = s.cpu().numpy()
        unused = np.ones(self.s_stride, bool)
        worst = 0.0
        for w, b, lat_idx, off in self.host:
            l_ = lat[:, lat_idx].astype(np.float64)
            if trunc is not None:
                m = np.zeros(self.style_dim) if tl is None else tl.astype(np.float64)
                l_ = m + trunc.astype(np.float64)[:, None] * (l_ - m)
            want = l_ @ w.T / np.sqrt(self.style_dim) + b
            bound = (self.style_dim / 64 + 14) * U * (np.abs(l_) @ np.abs(w).T / np.sqrt(self.style_dim) + np.abs(b))
            err = np.abs(got[:, off: off + w.shape[0]].astype(np.float64) - want)
            assert np.all(err <= bound), (label, w.shape[0], float(np.nanmax(err / bound)))  # (an unwritten element is a NaN: fails here)
            worst = max(worst, float((err / bound).max()))
            unused[off: off + w.shape[0]] = False
        assert np.all(got.view(np.int32)[:, unused] == CANARY_BITS), f"{label}: a column outside every layer's slice was written"
        print(f"[style_affine] {label}: max error / bound {worst:.3f}")
        return worst


def _latents(batch, n_latent, style_dim, seed):
    return np.random.default_rng(seed).standard_normal((batch, n_latent, style_dim)).astype(np.float32)


@pytest.mark.parametrize("batch", [1, 16, 17, 33, 70])
@pytest.mark.parametrize("style_dim", [64, 192, 512, 1024])
def test_affine_table_of_eight_widths(gpu, style_dim, batch):
    """1, 3, 8 and 16 values per lane; one table whose eight entries have 1 .. 1024 rows (whole and ragged 16-row workgroups, rows beyond
    an entry's cin inside the grid of the widest) and read latent rows 0 and 2 of 3; 1 .. 70 frames (one chunk of 16, its tail, several
    chunks: the staging loop ends inside a 4096-element pass for every batch * style_dim that is no multiple of 4096)."""
    t = _Affine(gpu, style_dim, [(cin, 2 * (k % 2)) for k, cin in enumerate(ROWS)], 1000 + style_dim + batch)
    lat = _latents(batch, 3, style_dim, style_dim * batch)
    s = t.run(batch, 3, lat=t.g.inp(lat, "latents"))
    t.check(s, lat, label=f"style_dim {style_dim} batch {batch}")


@pytest.mark.parametrize("lat_idx", [0, 2])
@pytest.mark.parametrize("cin", ROWS)
def test_affine_single_entry(gpu, cin, lat_idx):
    """A one-entry table (the grid is sized by this entry alone), each row count, either latent row."""
    t = _Affine(gpu, 512, [(cin, lat_idx)], 50 + cin + lat_idx, s_off0=1 + lat_idx, gap=3)
    lat = _latents(17, 3, 512, cin)
    s = t.run(17, 3, lat=t.g.inp(lat, "latents"))
    t.check(s, lat, label=f"single entry cin {cin} lat_idx {lat_idx}")


def test_affine_truncation(gpu):
    """The lerp with trunc and trunc_latent; trunc alone (pinned: a zero mean latent, latent' = trunc * latent — include/maua_hip.h);
    per-frame values 1.0 (the un-truncated result, to the bound) and 0.0 (the affine of trunc_latent, exactly)."""
    batch, dim = 19, 512
    t = _Affine(gpu, dim, [(40, 0), (17, 2), (512, 1)], 77)
    r = np.random.default_rng(78)
    lat = _latents(batch, 3, dim, 79)
    tl = r.standard_normal(dim).astype(np.float32)
    trunc = (0.3 + 0.9 * r.random(batch)).astype(np.float32)
    trunc[[0, 5, 16, 18]] = 1.0
    trunc[[1, 6, 17]] = 0.0
    lat_d, tl_d, trunc_d = t.g.inp(lat, "latents"), t.g.inp(tl, "trunc_latent"), t.g.inp(trunc, "trunc")
    both = t.run(batch, 3, lat=lat_d, trunc=trunc_d, tl=tl_d, name="s_both")
    t.check(both, lat, trunc, tl, label="trunc + trunc_latent")
    alone = t.run(batch, 3, lat=lat_d, trunc=trunc_d, name="s_alone")
    t.check(alone, lat, trunc, None, label="trunc, trunc_latent NULL")
    plain = t.run(batch, 3, lat=lat_d, name="s_plain")
    t.check(plain, lat, label="no truncation")
    ones = trunc == 1.0
    t.check(both[torch.from_numpy(ones).to(gpu)], lat[ones], label="trunc == 1 against the un-truncated reference")
    mean_rows = np.broadcast_to(tl, (batch, 3, dim)).copy()
    of_mean = t.run(batch, 3, lat=t.g.inp(mean_rows, "mean_rows"), name="s_mean")
    t.check(of_mean, mean_rows, label="affine of trunc_latent")
    zeros = torch.from_numpy(trunc == 0.0).to(gpu)
    assert torch.equal(both[zeros].view(torch.int32), of_mean[zeros].view(torch.int32))  # (tl + 0 * (l - tl) is tl in any rounding; bits: the unused columns hold NaNs)


def _frame_source(g, frame0, latents=None, trunc=None, noise=()):
    src = _lib.FrameSource()
    src.frame0 = frame0
    src.latents, src.trunc = _lib.ptr(latents), _lib.ptr(trunc)
    for slot, (t, stride) in noise:
        src.noise[slot], src.noise_stride[slot] = _lib.ptr(t), stride
    return g.inp(torch.frombuffer(bytearray(bytes(src)), dtype=torch.uint8), "frame_source", dtype=torch.uint8)


@pytest.mark.parametrize("with_trunc", [False, True])
@pytest.mark.parametrize("frame0", [0, 5])
def test_affine_through_a_frame_source(gpu, frame0, with_trunc):
    """latents == NULL, the latents (and truncation) of a 9-frame sequence behind src, 4 frames from frame0: the bits of the direct call on
    that slice.  The launcher's own trunc argument (NaN here) is ignored with src."""
    frames, batch, dim = 9, 4, 512
    t = _Affine(gpu, dim, [(40, 0), (1000, 2), (17, 1)], 11)
    r = np.random.default_rng(12 + frame0)
    seq = _latents(frames, 3, dim, 13)
    tl = r.standard_normal(dim).astype(np.float32)
    tr = (0.3 + 0.9 * r.random(frames)).astype(np.float32)
    seq_d, tl_d, tr_d = t.g.inp(seq, "sequence"), t.g.inp(tl, "trunc_latent"), t.g.inp(tr, "trunc_sequence")
    nan_trunc = t.g.inp(np.full(batch, np.nan, np.float32), "ignored_trunc")
    src = _frame_source(t.g, frame0, seq_d, tr_d if with_trunc else None)
    via_src = t.run(batch, 3, lat=None, trunc=nan_trunc, tl=tl_d, src=src.data_ptr(), name="s_src")
    sl = slice(frame0, frame0 + batch)
    direct = t.run(batch, 3, lat=t.g.inp(seq[sl], "slice"), trunc=t.g.inp(tr[sl], "trunc_slice") if with_trunc else None, tl=tl_d, name="s_direct")
    t.check(direct, seq[sl], tr[sl] if with_trunc else None, tl, label=f"frame source frame0 {frame0} trunc {with_trunc}")
    assert torch.equal(via_src.view(torch.int32), direct.view(torch.int32))  # (bits: the unused columns hold the canary NaN)


# ---- demodulation

DEMOD_COUTS = (1, 3, 17, 32, 515)


def _demod_case(gpu, cin, batch, couts, seed, null_at=2):
    """A table of one entry per cout (+ one wsq == NULL entry at ``null_at``), all with ``cin`` input channels and a slice of their own in s;
    the blocks of d three floats apart.  Returns (guard, d, per-entry (d_off, cout, reference or None), largest error / bound)."""
    lib = _lib.load()
    g = Guard(gpu)
    r = np.random.default_rng(seed)
    dummy_w, dummy_b = g.inp(np.zeros(4, np.float32), "mod_w"), g.inp(np.zeros(4, np.float32), "mod_b")
    layout = list(couts)
    layout.insert(null_at, None)  # (the entry without demodulation: cout 8 and a block of d that nothing may write)
    n = len(layout)
    s_stride = n * (cin + 2) + 3
    s = (1 + 0.3 * r.standard_normal((batch, s_stride))).astype(np.float32)
    s_d = g.inp(s, "s")
    entries, blocks, d_off = [], [], 2
    for k, cout in enumerate(layout):
        s_off = 3 + k * (cin + 2)
        wscale = float(np.float32(1 / np.sqrt(cin * 9)))
        if cout is None:
            entries.append(dict(mod_w=dummy_w, mod_b=dummy_b, wsq=None, cin=cin, cout=8, lat_idx=0, s_off=s_off, d_off=d_off, wscale=wscale))
            blocks.append((d_off, 8, None))
            d_off += batch * 8 + 3
            continue
        wsq = (r.standard_normal((cout, cin)) ** 2).astype(np.float32)
        entries.append(dict(mod_w=dummy_w, mod_b=dummy_b, wsq=g.inp(wsq, f"wsq{k}"), cin=cin, cout=cout, lat_idx=0, s_off=s_off, d_off=d_off,
                            wscale=wscale))
        s2 = s[:, s_off: s_off + cin].astype(np.float64) ** 2
        blocks.append((d_off, cout, 1 / np.sqrt(wscale ** 2 * (s2 @ wsq.astype(np.float64).T) + 1e-8)))
        d_off += batch * cout + 3
    table = g.inp(_style_table(entries, "cpu"), "table", dtype=torch.uint8)
    d = g.out((d_off,), "d")
    rc = lib.maua_demod_f32(table.data_ptr(), n, max(couts), s_d.data_ptr(), s_stride, d.data_ptr(), batch, _lib.stream_ptr(gpu))
    assert rc == 0, rc
    g.check()
    got = d.cpu().numpy()
    rtol = (-(-cin // 64) + 12) * U / 2 + 4 * U
    unused = np.ones(d_off, bool)
    worst = 0.0
    for off, cout, want in blocks:
        if want is None:
            continue
        unused[off: off + batch * cout] = False
        rel = np.abs(got[off: off + batch * cout].astype(np.float64).reshape(batch, cout) - want) / want
        assert np.all(rel <= rtol), (cin, cout, batch, float(np.nanmax(rel)), rtol)
        worst = max(worst, float(rel.max() / rtol))
    assert np.all(got.view(np.int32)[unused] == CANARY_BITS), "d was written outside an entry's [batch, cout] block (or for a wsq == NULL entry)"
    print(f"[demod] cin {cin} batch {batch}: max relative error / bound {worst:.3f} (bound {rtol:.3e})")
    return worst


@pytest.mark.parametrize("batch", [1, 17, 33])
@pytest.mark.parametrize("cin", [1, 63, 64, 65, 1000, 1024])
def test_demod_against_float64(gpu, cin, batch):
    """cin around the 64 lanes of a wave and at the limit of the kernel; cout 1 .. 515 in one table (ragged 16-row workgroups, entries narrower
    than the grid) together with an entry that does not demodulate."""
    _demod_case(gpu, cin, batch, DEMOD_COUTS, 300 + cin + batch)


@pytest.mark.parametrize("cout", DEMOD_COUTS)
def test_demod_single_entry(gpu, cout):
    """A one-entry table per cout (the grid is sized by this entry alone); the entry without demodulation comes last."""
    _demod_case(gpu, 65, 17, (cout,), 400 + cout, null_at=1)


# ---- limits and refusals

def test_demodulated_entry_wider_than_1024_is_refused_where_the_table_is_built(monkeypatch):
    """demod_kernel keeps [16][cin] squared styles in 64 KB of LDS: cin > 1024 with wsq != NULL would write past it.  The launcher cannot see
    the table, so _style_table and the standalone layer path (_layer_styles) raise — before the library is even loaded (no launch)."""
    from maua_stylegan2_amd.models import stylegan2
    from maua_stylegan2_amd.models.stylegan2 import ModulatedConv2d

    w = torch.zeros(4)
    wide = dict(mod_w=w, mod_b=w, wsq=w, cin=1040, cout=8, lat_idx=0, s_off=0, d_off=0, wscale=1.0)
    with pytest.raises(NotImplementedError, match="1024 input channels"):
        _style_table([dict(wide, cin=1024), wide], "cpu")
    assert _style_table([dict(wide, cin=1024), dict(wide, wsq=None, cin=8192)], "cpu").numel() == 2 * ctypes.sizeof(_lib.StyleLayer)

    def no_launch():
        raise AssertionError("the library was reached before the refusal")

    monkeypatch.setattr(stylegan2._lib, "load", no_launch)
    layer = ModulatedConv2d(1040, 8, 3, 64)
    with pytest.raises(NotImplementedError, match="1024 input channels"):
        layer(torch.zeros(1, 1040, 4, 4), torch.zeros(1, 64))
    with pytest.raises(NotImplementedError, match="2048"):
        ModulatedConv2d(2048, 8, 3, 64)(torch.zeros(1, 2048, 4, 4), torch.zeros(1, 64))


def test_refused_arguments_leave_the_outputs_untouched(gpu):
    lib = _lib.load()
    t = _Affine(gpu, 512, [(40, 0)], 5)
    lat = t.g.inp(_latents(4, 1, 512, 6), "latents")
    wide = t.g.inp(np.zeros((4, 1, 1088), np.float32), "wide_latents")
    s = t.g.out((4, t.s_stride), "s")
    d = t.g.out((4 * 8,), "d")
    st = _lib.stream_ptr(gpu)
    tab = t.table.data_ptr()

    def affine(lat_=lat.data_ptr(), batch=4, dim=512, table=tab, n_layers=1, s_=s.data_ptr(), src=None):
        return lib.maua_style_affine_f32(lat_, batch, 1, dim, None, None, table, n_layers, 40, s_, t.s_stride, src, st)

    assert affine() == 0
    t.g.check()
    s.view(torch.int32).fill_(CANARY_BITS)
    for dim in (0, 96, 1088):  # not positive, no multiple of 64, more than 16 values per lane
        assert affine(lat_=wide.data_ptr(), dim=dim) == EINVAL
    assert affine(lat_=None) == EINVAL  # latents and src both NULL
    assert affine(batch=0) == EINVAL
    assert affine(n_layers=0) == EINVAL
    assert affine(table=None) == EINVAL
    assert affine(s_=None) == EINVAL

    def demod(table=tab, n_layers=1, s_=s.data_ptr(), d_=d.data_ptr(), batch=4):
        return lib.maua_demod_f32(table, n_layers, 8, s_, t.s_stride, d_, batch, st)

    assert demod(table=None) == EINVAL
    assert demod(s_=None) == EINVAL
    assert demod(d_=None) == EINVAL
    assert demod(batch=0) == EINVAL
    assert demod(n_layers=0) == EINVAL
    assert t.g.untouched("s") and t.g.untouched("d")
    t.g.check()
