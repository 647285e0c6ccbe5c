"""Shared references of the modulated 3x3 convolution for the GPU tests: a layer with seeded weights, the fp64 direct convolution of the
shared-weight formulation (tests/test_canary_gpu.py, tests/test_conv_instances_gpu.py, tests/test_weight_pack_gpu.py), the same
convolution over absolute values (the magnitude `M` that per-element rounding bounds are stated against) and float32 numpy emulations
of the one-axis Winograd forms of csrc/modconv.hip "exactly as written" (modes 2, 3 and 4) and of the two-axis forms of
csrc/modconv_w2d.hip (mode 5) and csrc/modconv_up2d.hip (mode 6), from which the amplification of rounding by each transform is MEASURED
on the CPU against the fp64 reference (tools/conv_instance_sweep.py --ratios / --dedicated) instead of being taken from the kernel under
test; and the fp64 reference of the whole up-sampling StyledConv for general 4 x 4 blur taps (tests/test_conv_dedicated_gpu.py)."""
import numpy as np
import torch

U32 = 2.0 ** -24  # unit round-off of float32


def _layer(cin, cout, up, seed, dev):
    from maua_stylegan2_amd.models.stylegan2 import ModulatedConv2d

    r = np.random.default_rng(seed)
    m = ModulatedConv2d(cin, cout, 3, 512, upsample=up)
    m.weight.copy_(torch.from_numpy(r.standard_normal((1, cout, cin, 3, 3)).astype(np.float32)))
    return m.to(dev), r


def _direct_conv64(x, s, d, w, up):
    import torch.nn.functional as F

    xs = (x.double().cpu() * s.double().cpu()[:, :, None, None])
    wd = w[0].double().cpu()
    if up:
        y = F.conv_transpose2d(xs, wd.transpose(0, 1), stride=2)
    else:
        y = F.conv2d(xs, wd, padding=1)
    scale = 1.0 / np.sqrt(w.shape[2] * 9)
    return y * scale * d[:, :, None, None].double().cpu()


def _direct_conv(x, s, d, w, up):
    """fp64 reference of the shared-weight formulation: conv(x * s, W) * wscale * d (transposed, stride 2, for up)."""
    import torch.nn.functional as F

    xs = (x * s[:, :, None, None]).double().cpu()
    wd = w[0].double().cpu()
    if up:
        y = F.conv_transpose2d(xs, wd.transpose(0, 1), stride=2)
    else:
        y = F.conv2d(xs, wd, padding=1)
    scale = 1.0 / np.sqrt(w.shape[2] * 9)
    return (y * scale * d[:, :, None, None].double().cpu()).float()


def conv_and_magnitude(x, s, d, w, up):
    """(want, M) in fp64: the convolution of the fp32 operands (the product x * s formed in fp64 as well) and the same convolution with
    every operand replaced by its absolute value, M = wscale * |d| * sum |x s| |w| — the quantity every rounding bound scales with."""
    want = _direct_conv64(x, s, d, w, up)
    mag = _direct_conv64(x.abs(), s.abs(), d.abs(), w.abs(), up)
    return want, mag


def upfirdn64(x, kernel, up=1, pad=(0, 0)):
    """fp64 upfirdn2d (zero-stuff by ``up``, pad, true convolution with ``kernel``; down = 1), as oracle/ops_oracle.py states it in fp32."""
    import torch.nn.functional as F

    n, c, h, w = x.shape
    planes = x.double().reshape(n * c, 1, h, w)
    stuffed = planes.new_zeros(n * c, 1, h * up, w * up)
    stuffed[:, :, ::up, ::up] = planes
    stuffed = F.pad(stuffed, [pad[0], pad[1], pad[0], pad[1]])
    taps = torch.flip(kernel.double().cpu(), [0, 1])[None, None]
    out = F.conv2d(stuffed, taps)
    return out.reshape(n, c, *out.shape[-2:])


def case_operands(mode, cin, cout, h, w, batch, seed=0):
    """The seeded fp32 operands of one test case — x, s [B, s_stride = cin + 5] (a slice of a wider styles table), d, weight
    [1, cout, cin, 3, 3] — and the generator they came from (for the case's further operands).  The GPU test and the CPU measurement of
    the rounding ratios draw the SAME operands: how much a Winograd transform amplifies rounding at an element depends on the data
    (a product such as (g0 + g2) d1 is rounded relative to terms that cancel out of the result), so the ratio is measured on what the
    test feeds."""
    rng = np.random.default_rng([seed, mode, cin, cout, h, w, batch])
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))  # noqa: E731
    x, s, wt = f(batch, cin, h, w), 1 + 0.3 * f(batch, cin + 5), f(1, cout, cin, 3, 3)
    d = torch.from_numpy((0.5 + rng.random((batch, cout))).astype(np.float32))
    return rng, x, s, d, wt


# ---- float32 emulations of the transforms as csrc/modconv.hip writes them ---------------------------------------------------------------
_F = np.float32


def _chain(u_rows, v_rows):
    """sum over k of u[k] * v[k] accumulated term after term in float32 (u[k]: [O, 1...], v[k]: [B, 1, ...] broadcast)."""
    acc = None
    for u, v in zip(u_rows, v_rows):
        t = (u * v).astype(_F)
        acc = t if acc is None else (acc + t).astype(_F)
    return acc


def w2d_matrices():
    """(BT2, G2, AT2, BT4, G4, AT4) of F(2x4, 3x3), the matrices tests/test_winograd_algebra.py proves the identity with."""
    import test_winograd_algebra as wa

    return wa._BT2, wa._G2, wa._AT2, wa._BT4, wa._G4, wa._AT4


def emulate_w2d_f32(xs, g, gain, mats=None):
    """Mode 5, F(2,3) along y on F(4,3) along x, all tiles at once: transformed kernel and windows in float32, the 24 products summed
    channel after channel in float32, the inverse transform in float32, then the gain.  xs [B, C, H, W] (scaled input), g [O, C, 3, 3],
    gain [B, O, 1, 1], all float32; H % 2 == 0, W % 4 == 0.  ``mats`` replaces the six matrices (the host tests perturb one constant)."""
    bt2, g2, at2, bt4, g4, at4 = (m.astype(_F) for m in (mats or w2d_matrices()))
    b, c, h, wd = xs.shape
    xp = np.pad(xs, ((0, 0), (0, 0), (1, 1), (1, 1)))
    u = np.einsum("ak,ockl,bl->ocab", g2, g, g4).astype(_F)                                       # [O, C, 4, 6]
    rows = np.stack([xp[:, :, k:k + h:2, :] for k in range(4)], 2)                                # [B, C, 4, H/2, W+2]
    win = np.stack([rows[..., k:k + wd:4] for k in range(6)], 3)                                  # [B, C, 4, 6, H/2, W/4]
    v = np.einsum("ak,zcklij,bl->zcabij", bt2, win, bt4).astype(_F)
    acc = _chain([u[None, :, ch, :, :, None, None] for ch in range(c)], [v[:, None, ch] for ch in range(c)])  # [B, O, 4, 6, H/2, W/4]
    t = np.einsum("pa,zoabij,qb->zoipjq", at2, acc, at4).astype(_F)                                # [B, O, H/2, 2, W/4, 4]
    return (t.reshape(b, g.shape[0], h, wd) * gain).astype(_F)


def _up2d_pack(g):
    """up2d_pack of tests/test_winograd_algebra.py on a whole weight: g [O, C, 3, 3] -> the 16 entries, each [O, C] (float32 sums)."""
    import test_winograd_algebra as wa

    return wa.up2d_pack(np.ascontiguousarray(g.transpose(2, 3, 0, 1)))


def emulate_up2d_f32(xs, g, gain, drop=None):
    """Mode 6, F(2,2) on both axes of the transposed convolution, all 2 x 2 blocks at once: the 16 kernel entries and the 16 window forms
    in float32, every one of the 25 products summed over the channels in float32 BEFORE the output sums (the kernel's accumulators), the
    sums in the kernel's order; the edge lines (row 2H, column 2W) as plain polyphase chains.  xs [B, C, H, W], g [O, C, 3, 3],
    gain [B, O, 1, 1] -> [B, O, 2H+1, 2W+1].  ``drop`` = (i, j) leaves the odd-odd product of that position out (host tests)."""
    u = _up2d_pack(g)
    b, c, h, wd = xs.shape
    o = g.shape[0]
    xp = np.pad(xs, ((0, 0), (0, 0), (1, 1), (1, 1)))
    win = [[xp[:, :, a:a + h:2, k:k + wd:2] for k in range(3)] for a in range(3)]                 # rows / columns p - 1, p, p + 1 of every block
    sub = lambda p, q: (p - q).astype(_F)  # noqa: E731
    r = [[sub(win[0][k], win[1][k]) for k in range(3)], win[1], [sub(win[2][k], win[1][k]) for k in range(3)], win[2]]
    bf = [[sub(rf[0], rf[1]), rf[1], sub(rf[2], rf[1]), rf[2]] for rf in r]

    def dot(uk, v):  # [O, C] x [B, C, i, j] -> [B, O, i, j], channel after channel in float32
        return _chain([uk[None, :, ch, None, None] for ch in range(c)], [v[:, None, ch] for ch in range(c)])

    ee = [[dot(u[3 * a + k], bf[a][k]) for k in range(3)] for a in range(3)]
    eo = [[dot(u[9 + a], bf[a][1 + 2 * j]) for j in range(2)] for a in range(3)]
    oe = [[dot(u[12 + k], bf[1 + 2 * i][k]) for k in range(3)] for i in range(2)]
    oo = [[dot(u[15], bf[1 + 2 * i][1 + 2 * j]) for j in range(2)] for i in range(2)]
    if drop is not None:
        oo[drop[0]][drop[1]] = np.zeros_like(oo[0][0])
    add = lambda p, q: (p + q).astype(_F)  # noqa: E731
    y = np.zeros((b, o, 2 * h + 1, 2 * wd + 1), _F)
    for i in range(2):
        for j in range(2):
            y[:, :, 2 * i:2 * h:4, 2 * j:2 * wd:4] = add(add(ee[i][j], ee[i][j + 1]), add(ee[i + 1][j], ee[i + 1][j + 1]))
            y[:, :, 2 * i:2 * h:4, 2 * j + 1:2 * wd:4] = add(eo[i][j], eo[i + 1][j])
            y[:, :, 2 * i + 1:2 * h:4, 2 * j:2 * wd:4] = add(oe[i][j], oe[i][j + 1])
            y[:, :, 2 * i + 1:2 * h:4, 2 * j + 1:2 * wd:4] = oo[i][j]
    # edge lines: y[2n] = t0 v[n] + t2 v[n - 1], y[2n + 1] = t1 v[n] with v the last input row / column, t the kernel's last row / column
    for line, n_in, v, taps in ((0, wd, xs[:, :, h - 1, :], g[:, :, 2, :]), (1, h, xs[:, :, :, wd - 1], g[:, :, :, 2])):
        vp = np.pad(v, ((0, 0), (0, 0), (1, 1)))  # vp[n + 1] = v[n]
        even = _chain([taps[None, :, ch, t, None] for ch in range(c) for t in (0, 2)],
                      [vp[:, None, ch, (1 if t == 0 else 0):(1 if t == 0 else 0) + n_in + 1] for ch in range(c) for t in (0, 2)])
        odd = _chain([taps[None, :, ch, 1, None] for ch in range(c)], [v[:, None, ch, :] for ch in range(c)])
        if line == 0:
            y[:, :, 2 * h, 0::2], y[:, :, 2 * h, 1::2] = even, odd
        else:
            y[:, :, 0:2 * h:2, 2 * wd], y[:, :, 1:2 * h:2, 2 * wd] = even[..., :n_in], odd
    return (y * gain).astype(_F)


def emulate_f32(mode, x, s, d, w):
    """Modes 2 / 3 / 4 (one-axis forms of csrc/modconv.hip), 5 (csrc/modconv_w2d.hip) and 6 (csrc/modconv_up2d.hip) in float32 numpy: the
    input scaled by the style, the window transforms, the packed-weight formulas of include/maua_hip.h, one float32 accumulator per
    frequency over (kernel row, channel), the inverse transform and the gain wscale * d, each operation rounded to float32 as the kernel's
    statements are.  x [B, C, H, W], s [B, C], d [B, O], w [1, O, C, 3, 3] (torch fp32) -> [B, O, OH, OW] float32."""
    x, s, d, g = (t.numpy().astype(_F) for t in (x, s, d, w[0]))
    if mode in (5, 6):
        xs = (x * s[:, :, None, None]).astype(_F)
        gain = (_F(1.0 / np.sqrt(x.shape[1] * 9)) * d).astype(_F)[:, :, None, None]
        return emulate_w2d_f32(xs, g, gain) if mode == 5 else emulate_up2d_f32(xs, g, gain)
    b, c, h, wd = x.shape
    o = g.shape[0]
    xs = (x * s[:, :, None, None]).astype(_F)
    gain = (_F(1.0 / np.sqrt(c * 9)) * d).astype(_F)[:, :, None, None]
    g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]  # [O, C, ky]
    if mode == 2:
        u = [g0, (_F(0.5) * ((g0 + g1).astype(_F) + g2).astype(_F)).astype(_F), (_F(0.5) * ((g0 - g1).astype(_F) + g2).astype(_F)).astype(_F), g2]
        xp = np.pad(xs, ((0, 0), (0, 0), (1, 1), (1, 1)))
        dd = [xp[:, :, :, k:k + wd:2] for k in range(4)]  # d0..d3 of every output pair: [B, C, H + 2, W / 2]
        t = [(dd[0] - dd[2]).astype(_F), (dd[1] + dd[2]).astype(_F), (dd[2] - dd[1]).astype(_F), (dd[1] - dd[3]).astype(_F)]
        m = [_chain([u[xi][None, :, ch, ky, None, None] for ky in range(3) for ch in range(c)],
                    [t[xi][:, None, ch, ky:ky + h, :] for ky in range(3) for ch in range(c)]) for xi in range(4)]
        y = np.empty((b, o, h, wd), _F)
        y[..., 0::2] = ((m[0] + m[1]).astype(_F) + m[2]).astype(_F)
        y[..., 1::2] = ((m[1] - m[2]).astype(_F) - m[3]).astype(_F)
        return (y * gain).astype(_F)
    if mode == 3:
        s012p, s012m = ((g0 + g1).astype(_F) + g2).astype(_F), ((g0 - g1).astype(_F) + g2).astype(_F)
        a24p = ((g0 + (_F(2) * g1).astype(_F)).astype(_F) + (_F(4) * g2).astype(_F)).astype(_F)
        a24m = ((g0 - (_F(2) * g1).astype(_F)).astype(_F) + (_F(4) * g2).astype(_F)).astype(_F)
        u = [(g0 * _F(0.25)).astype(_F), (-s012p * _F(1.0 / 6.0)).astype(_F), (-s012m * _F(1.0 / 6.0)).astype(_F),
             (a24p * _F(1.0 / 24.0)).astype(_F), (a24m * _F(1.0 / 24.0)).astype(_F), g2]
        xp = np.pad(xs, ((0, 0), (0, 0), (1, 1), (1, 1)))
        dd = [xp[:, :, :, k:k + wd:4] for k in range(6)]
        a_ = (dd[4] - (_F(4) * dd[2])).astype(_F)   # (the kernel's fmaf forms round once; numpy rounds the product first: exact for x 4, x 2)
        b_ = (dd[3] - (_F(4) * dd[1])).astype(_F)
        c_, e_ = (dd[4] - dd[2]).astype(_F), (dd[3] - dd[1]).astype(_F)
        # fmaf(4, d0, fmaf(-5, d2, d4)): the inner fma rounds once (formed in fp64 here), 4 d0 is exact
        t0 =((_F(4) * dd[0]) + ((dd[4].astype(np.float64) - 5.0 * dd[2].astype(np.float64)).astype(_F))).astype(_F)
        t5 = ((_F(4) * dd[1]) + ((dd[5].astype(np.float64) - 5.0 * dd[3].astype(np.float64)).astype(_F))).astype(_F)
        t = [t0, (a_ + b_).astype(_F), (a_ - b_).astype(_F), (c_ + _F(2) * e_).astype(_F), (c_ - _F(2) * e_).astype(_F), t5]
        m = [_chain([u[xi][None, :, ch, ky, None, None] for ky in range(3) for ch in range(c)],
                    [t[xi][:, None, ch, ky:ky + h, :] for ky in range(3) for ch in range(c)]) for xi in range(6)]
        s12, d12, s34, d34 = (m[1] + m[2]).astype(_F), (m[1] - m[2]).astype(_F), (m[3] + m[4]).astype(_F), (m[3] - m[4]).astype(_F)
        y = np.empty((b, o, h, wd), _F)
        y[..., 0::4] = ((m[0] + s12).astype(_F) + s34).astype(_F)
        y[..., 1::4] = (d12 + _F(2) * d34).astype(_F)
        y[..., 2::4] = (s12 + _F(4) * s34).astype(_F)
        y[..., 3::4] = ((d12 + _F(8) * d34).astype(_F) + m[5]).astype(_F)
        return (y * gain).astype(_F)
    assert mode == 4
    # transposed, F(2,2) on the even x-phase: position rows i = 0 .. H, position pairs p = 0, 2, .. W; kernel rows 0 / 1 read input row i,
    # kernel row 2 input row i - 1; weight rows g2, g0 + g2, g0, g1; slots [row parity][m0, m1, m2, o_p, o_p+1]
    u = [g2, (g0 + g2).astype(_F), g0, g1]
    npair = wd // 2 + 1
    xp = np.pad(xs, ((0, 0), (0, 0), (1, 1), (1, 3)))  # xp[r + 1, q + 1] = xs[r, q]; zeros outside
    d0, d1, d2 = (xp[:, :, :, k:k + 2 * npair:2] for k in range(3))  # [B, C, H + 2, npair]: x[r, p - 1], x[r, p], x[r, p + 1]
    t = [(d0 - d1).astype(_F), d1, (d2 - d1).astype(_F), d2]
    row = lambda a, ky, ch: a[:, None, ch, (0 if ky == 2 else 1):(0 if ky == 2 else 1) + h + 1, :]  # noqa: E731  input row i - 1 / i for i = 0 .. H
    y = np.zeros((b, o, 2 * h + 2, 4 * npair), _F)
    for parity, kys in ((0, (0, 2)), (1, (1,))):
        slot = []
        for j in range(5):
            wrow, bk = (j, j) if j < 3 else (3, 1 if j == 3 else 3)
            slot.append(_chain([u[wrow][None, :, ch, ky, None, None] for ch in range(c) for ky in kys],
                               [row(t[bk], ky, ch) for ch in range(c) for ky in kys]))
        y[:, :, parity::2, 0::4] = (slot[0] + slot[1]).astype(_F)
        y[:, :, parity::2, 1::4] = slot[3]
        y[:, :, parity::2, 2::4] = (slot[1] + slot[2]).astype(_F)
        y[:, :, parity::2, 3::4] = slot[4]
    return (y[:, :, :2 * h + 1, :2 * wd + 1] * gain).astype(_F)


def ratio_of(mode, x, s, d, wt, got=None):
    """max |emulation - fp64| / (u * M) of the given operands (``got``: an emulation computed by the caller)."""
    want, mag = conv_and_magnitude(x, s, d, wt, mode in (4, 6))
    got = emulate_f32(mode, x, s, d, wt) if got is None else got
    err = np.abs(got.astype(np.float64) - want.numpy())
    m = mag.numpy()
    ok = m > 0
    assert np.all(err[~ok] == 0)
    return float((err[ok] / (U32 * m[ok])).max())


def prescale(x, s):
    """The style fold on the host: (x * s) rounded to float32 and styles of one — what a kernel instance with s == NULL is fed."""
    return (x * s[:, :, None, None]).float(), torch.ones_like(s)


def rounding_ratio(mode, cin, cout, h, w, batch, seed=0, pre=False):
    """max |emulation - fp64| / (u * M) of one case's operands (case_operands; ``pre``: the pre-scaled input of the s == NULL instances)."""
    _, x, s, d, wt = case_operands(mode, cin, cout, h, w, batch, seed)
    s = s[:, :cin].contiguous()
    if pre:
        x, s = prescale(x, s)
    return ratio_of(mode, x, s, d, wt)


def asymmetric_taps():
    """4 x 4 blur taps from two different, non-palindromic factors, outer([1, 2, 4, 1], [2, 1, 3, 2]) scaled to sum 4: every entry is an
    integer / 16, so the matrix, its row sums, its column sums and 1 / total are exact in float32 and the matrix is EXACTLY separable."""
    return torch.outer(torch.tensor([1.0, 2.0, 4.0, 1.0]), torch.tensor([2.0, 1.0, 3.0, 2.0])) / 16.0


def upconv_styled64(x, s, d, w, k4, noise_term=None, bias=None, post=None, conv=None):
    """fp64 reference of the whole up-sampling StyledConv for general 4 x 4 taps: raw transposed convolution -> upfirdn64(pad = (1, 1)) ->
    + noise_term (noise_w * noise, fp64, broadcastable) -> + bias [O] -> leaky ReLU * sqrt(2) -> * post [B, O].  Returns (want, parts):
    parts holds the same chain over absolute values — "raw" / "mag" (the raw map and its magnitude M), "blur_raw" = blur_|k|(|raw|),
    "blur_mag" = blur_|k|(M), "tail" = |noise_term| + |bias| — from which the tests state their bounds.  ``conv``: (raw, mag) when the
    caller has them already."""
    raw, mag = conv if conv is not None else conv_and_magnitude(x, s, d, w, True)
    k4 = k4.double().cpu()
    t = upfirdn64(raw, k4, up=1, pad=(1, 1))
    tail = torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    if noise_term is not None:
        t, tail = t + noise_term, tail + noise_term.abs()
    if bias is not None:
        bt = bias.double()[None, :, None, None]
        t, tail = t + bt, tail + bt.abs()
    want = torch.where(t > 0, t, 0.2 * t) * 2.0 ** 0.5
    if post is not None:
        want = want * post.double()[:, :, None, None]
    parts = dict(raw=raw, mag=mag, blur_raw=upfirdn64(raw.abs(), k4.abs(), up=1, pad=(1, 1)), blur_mag=upfirdn64(mag, k4.abs(), up=1, pad=(1, 1)),
                 tail=tail)
    return want, parts
