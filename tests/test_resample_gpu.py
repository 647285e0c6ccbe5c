"""GPU: maua_resample_u8 / maua_resample_u16 (csrc/resample.hip) through the C ABI between red zones, bit for bit against the numpy twin
(tests/resample_ref.py = Pillow's 8-bit resize restated) and, for the 8-bit cases, against Pillow itself where it imports.

Every buffer of a launch is a byte window of exact size inside a canary-filled allocation (redzone.Guard); the output is compared WHOLE
with "the bytes it held before the launch, the window replaced by the twin's result", so a byte written outside the window fails the
comparison and a byte written outside the buffer fails the red zones.  The geometry list is one that maua_resample_plan proves to reach
every instance (test_case_list_reaches_every_instance runs without a GPU)."""
import numpy as np
import pytest
import torch

import resample_ref as rr
from maua_stylegan2_amd import _lib
from redzone import Guard
from test_delivery_gpu import RESIZE_CASES, X0, Y0, decoy_frame

EINVAL, ENOSYS = -22, -38
DTYPES = {"u8": np.uint8, "u16": np.uint16}
TOP = {"u8": 255, "u16": 65535}


def make_frames(kind, batch, h, w, seed, fill=None, binary=False):
    r = np.random.default_rng(seed)
    if fill is not None:
        return np.full((batch, h, w, 3), fill, DTYPES[kind])
    if binary:
        return (r.integers(0, 2, (batch, h, w, 3)) * TOP[kind]).astype(DTYPES[kind])
    return r.integers(0, TOP[kind] + 1, (batch, h, w, 3)).astype(DTYPES[kind])


def c_tables(n, in0, in1, m, filt):
    """The entry's tables of one axis from maua_resample_coeffs; None where the definition copies the axis."""
    if rr.axis_is_identity(n, in0, in1, m):
        return None
    rc, k, bounds = _lib.resample_coeffs(n, in0, in1, m, filt)
    assert rc > 0, (n, in0, in1, m, filt, rc)
    return k, bounds


def twin_from_tables(frames, tx, ty, top):
    out = frames.astype(np.int64)
    if tx is not None:
        out = rr.apply_axis(out, tx[0], tx[1], 2, top)
    if ty is not None:
        out = rr.apply_axis(out, ty[0], ty[1], 1, top)
    return out.astype(frames.dtype)


class Launch:
    """One guarded launch: operands in windows of exact size (plus the requested skew in bytes), the output pre-filled with the canary."""

    def __init__(self, gpu, kind, frames, out_shape, window, tx, ty, skew_in=0, skew_out=0):
        self.kind, self.frames, self.window, self.tx, self.ty = kind, frames, window, tx, ty
        self.sz = 1 if kind == "u8" else 2
        batch, in_h, in_w, _ = frames.shape
        self.g = g = Guard(gpu)
        raw = np.zeros(frames.size * self.sz + skew_in, np.uint8)
        raw[skew_in:] = frames.reshape(-1).view(np.uint8)
        self.fin = g.inp(raw, "in", torch.uint8)[skew_in:]
        self.out_bytes = int(np.prod(out_shape)) * self.sz
        self.out = g.out((self.out_bytes + skew_out,), "out", torch.uint8)[skew_out:]
        self.out_shape = tuple(out_shape)
        dev = {}
        for axis, t in (("x", tx), ("y", ty)):
            dev[axis] = (None, None, 0) if t is None else (g.inp(t[0], "k" + axis, torch.int32), g.inp(t[1], "b" + axis, torch.int32), t[0].shape[1])
        x, y, w, h = window
        self.geo = (batch, in_h, in_w, out_shape[1], out_shape[2], x, y, w, h)
        n_ws = int(_lib.load().maua_resample_ws_bytes(self.sz, batch, in_h, in_w, w, h, dev["x"][2], dev["y"][2]))
        self.ws = g.out((n_ws,), "ws", torch.uint8) if n_ws else None
        self.dev = dev
        self.before = self.out.clone()
        self.plan = _lib.planned_resample(self.sz, *self.geo, dev["x"][2], dev["y"][2], self.out.data_ptr() & 3)

    def run(self, gpu, **override):
        fn = getattr(_lib.load(), "maua_resample_" + self.kind)
        (kx, bx, ksx), (ky, by, ksy) = self.dev["x"], self.dev["y"]
        args = dict(inp=self.fin.data_ptr(), out=self.out.data_ptr(), geo=self.geo, kx=_lib.ptr(kx), bx=_lib.ptr(bx), ksx=ksx, ky=_lib.ptr(ky),
                    by=_lib.ptr(by), ksy=ksy, ws=_lib.ptr(self.ws))
        args.update(override)
        return fn(args["inp"], args["out"], *args["geo"], args["kx"], args["bx"], args["ksx"], args["ky"], args["by"], args["ksy"], args["ws"],
                  _lib.stream_ptr(gpu))

    def result(self):
        return self.out.cpu().numpy().view(DTYPES[self.kind]).reshape(self.out_shape)

    def expected(self, inside=None):
        """The output's earlier content with the window replaced by ``inside`` (default: the twin on the launch's own tables)."""
        x, y, w, h = self.window
        want = self.before.cpu().numpy().view(DTYPES[self.kind]).reshape(self.out_shape).copy()
        want[:, y:y + h, x:x + w] = twin_from_tables(self.frames, self.tx, self.ty, TOP[self.kind]) if inside is None else inside
        return want

    def check(self, inside=None, tag=None):
        got, want = self.result(), self.expected(inside)
        self.g.check()
        bad = int((got != want).sum())
        assert bad == 0, (tag, self.plan, bad, np.argwhere(got != want)[:4].tolist())
        return got


def geometry(gpu, kind, batch, src, size, filt, box=None, out=None, at=(0, 0), skew_in=0, skew_out=0, seed=0, fill=None, binary=False):
    """A launch of the definition: ``src = (W, H)`` frames resized to ``size = (w, h)`` with ``filt`` from the source ``box``, into the
    window at ``at`` of ``out = (OW, OH)`` frames (default: the window is the frame)."""
    W, H = src
    w, h = size
    x0, y0, x1, y1 = box or (0, 0, W, H)
    frames = make_frames(kind, batch, H, W, seed, fill, binary)
    tx, ty = c_tables(W, x0, x1, w, filt), c_tables(H, y0, y1, h, filt)
    ow, oh = out or size
    launch = Launch(gpu, kind, frames, (batch, oh, ow, 3), at + (w, h), tx, ty, skew_in, skew_out)
    launch.definition = lambda: rr.resize(frames, size, filt, box)
    return launch


# ---------------------------------------------------------------------------------------------------------------- the case list
# (name, batch, (W, H), (w, h), filter, box, (OW, OH) or None, (x, y)): small sources, every filter, up / down / mixed, crops, identity axes
SOURCES = [
    ("tiny-up", 1, (5, 3), (13, 9), "lanczos", None, None, (0, 0)),
    ("tiny-up-bicubic", 2, (5, 3), (64, 16), "bicubic", None, None, (0, 0)),
    ("one-column", 1, (9, 7), (1, 5), "hamming", None, None, (0, 0)),
    ("63-columns", 1, (20, 11), (63, 17), "bilinear", None, None, (0, 0)),
    ("64-columns", 3, (20, 11), (64, 33), "box", None, None, (0, 0)),
    ("65-columns", 1, (20, 11), (65, 16), "lanczos", None, None, (0, 0)),
    ("down", 2, (130, 70), (33, 21), "lanczos", None, None, (0, 0)),
    ("down-box", 1, (130, 70), (40, 35), "box", None, None, (0, 0)),
    ("down-box-ties", 1, (60, 45), (40, 30), "box", None, None, (0, 0)),  # scale 1.5: window ends at exact ties (n + 0.5)
    ("down-hamming", 1, (97, 66), (31, 20), "hamming", None, None, (0, 0)),
    ("mixed", 1, (37, 70), (90, 20), "bicubic", None, None, (0, 0)),
    ("crop", 2, (50, 40), (77, 31), "bilinear", (3, 2, 47, 39), None, (0, 0)),
    ("crop-down", 1, (130, 70), (30, 30), "bicubic", (10, 0, 120, 70), None, (0, 0)),
    ("identity-x", 1, (66, 30), (66, 47), "lanczos", None, None, (0, 0)),
    ("identity-y", 2, (30, 18), (71, 18), "hamming", None, None, (0, 0)),
    ("identity-both", 1, (70, 20), (70, 20), "box", None, None, (0, 0)),
    ("pad-window", 2, (40, 30), (52, 38), "lanczos", None, (70, 44), (8, 2)),
    ("pad-window-odd", 1, (40, 30), (51, 37), "bicubic", None, (67, 41), (5, 3)),
    ("pad-down", 1, (120, 64), (60, 32), "bilinear", None, (64, 48), (2, 8)),
]
# geometries chosen for the planner (tests below assert what the plan says of each)
TWOPASS_U8 = ("twopass-u8", 1, (9, 100), (31, 5), "bilinear", None, None, (0, 0))          # 20 : 1 down, 41 taps: the row span leaves LDS
TWOPASS_U16 = ("twopass-u16", 1, (9, 100), (31, 10), "bilinear", None, None, (0, 0))       # 10 : 1 down, 21 taps
TWOPASS_COPY_X = ("twopass-copy-x", 2, (33, 100), (33, 5), "bilinear", None, (40, 9), (4, 3))  # no horizontal launch, a window
TWOPASS_TRIPS = ("twopass-trips", 3, (5, 400), (2200, 40), "bilinear", None, None, (0, 0))  # both launches take a second grid-stride trip
FUSED_TRIPS = ("fused-trips", 1, (5, 3), (65, 64 * 1025), "bilinear", None, None, (0, 0))   # 2 x 1025 tiles of 64 rows > 2048 workgroups
TILES = ("64x64", "64x32", "64x16")
CASE = {case[0]: case for case in SOURCES}


def _ksize(n, in0, in1, m, filt):
    return 0 if rr.axis_is_identity(n, in0, in1, m) else rr.ksize_of(in0, in1, m, filt)


def plan_of(kind, case, misalign=0):
    _, batch, (W, H), (w, h), filt, box, out, at = case
    x0, y0, x1, y1 = box or (0, 0, W, H)
    ow, oh = out or (w, h)
    return _lib.planned_resample(1 if kind == "u8" else 2, batch, H, W, oh, ow, at[0], at[1], w, h, _ksize(W, x0, x1, w, filt),
                                 _ksize(H, y0, y1, h, filt), misalign)


def test_case_list_reaches_every_instance(built_lib):
    """maua_resample_plan on the list: every instance (fused / two-pass x sample type x store path), a partial last tile, exact 1 / 63 / 64 /
    65 column windows, a second trip of the fused tile loop and of both two-pass launches."""
    seen, tiles = set(), set()
    for kind in DTYPES:
        for case in SOURCES:
            for misalign in (0, 1 if kind == "u8" else 2):
                rc, name, fields = plan_of(kind, case, misalign)
                assert rc == 0 and name.startswith("fused." + kind), (case[0], rc, name)
                assert fields["tile"] in TILES and int(fields["lds"]) <= 65536 and int(fields["rows"]) >= 1
                tiles.add(fields["tile"])
                seen.add(name)
    assert seen == {f"fused.{k}.{p}" for k in DTYPES for p in ("vec", "scalar")}
    assert tiles == set(TILES), tiles  # every tile height: the tallest whose LDS stays within a workgroup's share
    widths = {case[3][0] for case in SOURCES}
    assert {1, 63, 64, 65} <= widths and any(case[3][1] % 16 for case in SOURCES)
    assert plan_of("u8", TWOPASS_U8)[1] == "twopass.u8" and plan_of("u16", TWOPASS_U16)[1] == "twopass.u16"
    assert plan_of("u8", TWOPASS_U16)[1].startswith("fused.u8")  # the same geometry fits at 8 bits: the switch-over is the LDS budget
    rc, name, fields = plan_of("u16", TWOPASS_COPY_X)
    assert name == "twopass.u16" and fields["ws"] == "0" and fields["trips"].split(",")[0] == "0"
    rc, name, fields = plan_of("u16", TWOPASS_TRIPS)
    assert name == "twopass.u16" and all(int(t) >= 2 for t in fields["trips"].split(",")), fields
    assert int(fields["ws"]) == 3 * 400 * 2200 * 3 * 2
    rc, name, fields = plan_of("u8", FUSED_TRIPS)
    assert name == "fused.u8.scalar" and fields["tile"] == "64x64" and int(fields["tiles"]) == 2 * 1025 and fields["trips"] == "2"  # (65 * 3 bytes a row: no 4-byte pitch)
    # an odd row pitch, an odd window column or a skewed pointer take the scalar store path
    assert _lib.planned_resample(1, 1, 8, 8, 8, 64, 0, 0, 64, 8, 3, 0)[1] == "fused.u8.vec"
    assert _lib.planned_resample(1, 1, 8, 8, 8, 66, 1, 0, 64, 8, 3, 0)[1] == "fused.u8.scalar"
    assert _lib.planned_resample(1, 1, 8, 8, 8, 67, 0, 0, 64, 8, 3, 0)[1] == "fused.u8.scalar"
    assert _lib.planned_resample(2, 1, 8, 8, 8, 67, 0, 0, 64, 8, 3, 0)[1] == "fused.u16.scalar"
    assert _lib.planned_resample(2, 1, 8, 8, 8, 66, 0, 0, 64, 8, 3, 0, 2)[1] == "fused.u16.scalar"


def _pil(frames, size, filt, box):
    try:
        import PIL.Image as Image
    except ImportError:
        return None
    flt = {"box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[filt]
    return np.stack([np.array(Image.fromarray(f).resize(size, flt, box=box)) for f in frames])


def _run_case(gpu, kind, case, seed, **kw):
    name, batch, src, size, filt, box, out, at = case
    launch = geometry(gpu, kind, batch, src, size, filt, box, out, at, seed=seed, **kw)
    assert launch.run(gpu) == 0, name
    want = launch.definition()  # the twin on its OWN tables: the C tables and the kernels against the definition at once
    launch.check(inside=want, tag=name)
    if kind == "u8":
        pil = _pil(launch.frames, size, filt, box)
        assert pil is None or np.array_equal(pil, want), ("the twin left Pillow", name)
    return launch


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(DTYPES))
def test_small_sources_against_the_twin(gpu, kind):
    """Every geometry of SOURCES, random and 0 / top-valued frames: bit-equal, nothing outside the window written."""
    for n, case in enumerate(SOURCES):
        launch = _run_case(gpu, kind, case, seed=100 + n, binary=bool(n % 2))
        assert launch.plan[1].startswith("fused." + kind), (case[0], launch.plan)
    print(f"[resample_{kind}] {len(SOURCES)} geometries, 0 samples differ from the twin" + (" and from Pillow" if kind == "u8" else ""))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("filt", list(rr.FILTERS))
def test_every_filter_up_and_down(gpu, kind, filt):
    for n, (src, size, box) in enumerate([((23, 17), (70, 40), None), ((129, 67), (40, 21), None), ((40, 30), (29, 66), (1, 2, 38, 29))]):
        _run_case(gpu, kind, (f"{filt}-{n}", 1 + n % 2, src, size, filt, box, None, (0, 0)), seed=200 + n)


@pytest.mark.gpu
def test_two_pass_geometries(gpu):
    """Row spans beyond the LDS budget: the two-launch path through the workspace gives the same bits; the workspace stays inside its window."""
    for kind, case in (("u8", TWOPASS_U8), ("u16", TWOPASS_U8), ("u16", TWOPASS_U16), ("u8", TWOPASS_COPY_X), ("u16", TWOPASS_COPY_X)):
        launch = _run_case(gpu, kind, case, seed=300)
        assert launch.plan[1] == "twopass." + kind, (case[0], launch.plan)
        assert (launch.ws is None) == (case is TWOPASS_COPY_X)


@pytest.mark.gpu
def test_second_grid_stride_trips(gpu):
    launch = _run_case(gpu, "u8", FUSED_TRIPS, seed=400)
    assert launch.plan[1] == "fused.u8.scalar" and launch.plan[2]["trips"] == "2"
    launch = _run_case(gpu, "u16", TWOPASS_TRIPS, seed=401)
    assert launch.plan[1] == "twopass.u16" and all(int(t) >= 2 for t in launch.plan[2]["trips"].split(","))


def _hand_tables(rng, n, m, taps, full_scale=True):
    """Tables no filter produces: ``taps`` weights per output summing to 2^22 (some negative), windows placed anywhere inside [0, n]."""
    k = np.zeros((m, taps), np.int32)
    bounds = np.zeros((m, 2), np.int32)
    for j in range(m):
        cnt = min(taps, n)
        lo = int(rng.integers(0, n - cnt + 1))
        w = rng.integers(-(1 << 13), 1 << 15, cnt).astype(np.int64)  # (255 * sum |k| stays inside the 32-bit sums of the 8-bit passes)
        w[0] += (1 << 22) - w.sum()
        k[j, :cnt] = w
        bounds[j] = lo, cnt
    return k, bounds


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(DTYPES))
def test_one_tap_and_sixty_four_taps(gpu, kind):
    """Hand-made tables at both ends of the accepted range (1 and MAUA_RESAMPLE_MAX_TAPS taps), windows in any order — not monotone, as
    no filter's are: the tile loop takes whatever row groups fit its LDS."""
    rng = np.random.default_rng(7)
    for taps_x, taps_y, (W, H), (w, h) in ((1, 1, (9, 7), (70, 19)), (64, 64, (90, 70), (66, 33)), (1, 64, (12, 70), (5, 33)), (64, 1, (70, 6), (65, 40))):
        frames = make_frames(kind, 2, H, W, taps_x + taps_y)
        tx, ty = _hand_tables(rng, W, w, taps_x), _hand_tables(rng, H, h, taps_y)
        launch = Launch(gpu, kind, frames, (2, h, w, 3), (0, 0, w, h), tx, ty)
        assert launch.plan[1].startswith("fused"), launch.plan
        assert launch.run(gpu) == 0
        launch.check(tag=(taps_x, taps_y))


@pytest.mark.gpu
def test_out_of_range_bounds_are_clamped_on_the_device(gpu):
    """Bounds that point outside the frame are clamped by the kernels (never a read outside `in`): the result is the twin's on the clamped
    tables, fused and two-pass."""
    for kind, (W, H), (w, h), taps_y in (("u8", (9, 12), (20, 15), 5), ("u16", (9, 100), (20, 5), 41)):
        frames = make_frames(kind, 1, H, W, 5)
        rng = np.random.default_rng(3)
        (kx, bx), (ky, by) = _hand_tables(rng, W, w, 3), _hand_tables(rng, H, h, taps_y)
        wild_x, wild_y = bx.copy(), by.copy()
        wild_x[0], wild_x[1], wild_x[2] = (-5, 3), (W - 1, 3), (2, 99)
        wild_y[0], wild_y[1] = (-1, taps_y), (H - 2, taps_y)

        def clamp(b, n, ks):
            lo = np.clip(b[:, 0], 0, n - 1)
            return np.stack([lo, np.minimum(np.clip(b[:, 1], 0, None), np.minimum(ks, n - lo))], 1).astype(np.int32)

        def zero_tail(k, b):
            k = k.copy()
            k[np.arange(k.shape[1])[None] >= b[:, 1:]] = 0
            return k

        cx, cy = clamp(wild_x, W, 3), clamp(wild_y, H, taps_y)
        launch = Launch(gpu, kind, frames, (1, h, w, 3), (0, 0, w, h), (kx, wild_x), (ky, wild_y))
        assert launch.run(gpu) == 0
        inside = twin_from_tables(frames, (zero_tail(kx, cx), cx), (zero_tail(ky, cy), cy), TOP[kind])
        launch.check(inside=inside, tag=kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(DTYPES))
def test_skewed_pointers(gpu, kind):
    """Input and output at every offset from a 4-byte boundary the sample type allows: the plan names the store path, the bits are the same."""
    step = 1 if kind == "u8" else 2
    for skew_in in range(0, 4, step):
        for skew_out in range(0, 4, step):
            name, batch, src, size, filt, box, out, at = SOURCES[2 + (skew_in + skew_out) % 5]
            size = (64, size[1])  # (64 columns: a 4-byte row pitch at both sample sizes, so that the pointer alone decides)
            launch = geometry(gpu, kind, batch, src, size, filt, box, None, at, skew_in, skew_out, seed=skew_in * 4 + skew_out)
            assert launch.plan[1] == f"fused.{kind}." + ("vec" if skew_out == 0 else "scalar"), (skew_out, launch.plan)
            assert launch.run(gpu) == 0
            launch.check(inside=launch.definition(), tag=(skew_in, skew_out))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(DTYPES))
def test_constant_frames_stay_constant(gpu, kind):
    """The weights of an output sum to 2^22 up to their rounding, far below half a code: 0, the top code and a mid grey come back exactly."""
    for fill in (0, TOP[kind], TOP[kind] // 3):
        for case in (CASE["tiny-up"], CASE["down"], CASE["mixed"], CASE["pad-window"], TWOPASS_U8):
            launch = geometry(gpu, kind, *case[1:5], case[5], case[6], case[7], fill=fill)
            assert launch.run(gpu) == 0
            x, y, w, h = launch.window
            got = launch.check(inside=launch.definition(), tag=(fill, case[0]))
            assert (got[:, y:y + h, x:x + w] == fill).all(), (fill, case[0])


@pytest.mark.gpu
def test_bilinear_upscales_equal_the_crop_resize_entries(gpu):
    """The 2-tap entries the resampler generalises: on a sample of their own case list maua_resample_u8 / _u16 with bilinear tables give the
    bits of maua_crop_resize_u8 / _u16.  The crop itself is the source of both (the older entries clamp their taps to the crop, Pillow's
    ``box`` — the definition here — lets them reach the pixels around it: the two agree where the crop is the whole frame)."""
    lib, st = _lib.load(), _lib.stream_ptr(gpu)
    for n, (cw, ch, ow, oh) in enumerate(RESIZE_CASES[::41]):
        crop8 = np.ascontiguousarray(decoy_frame(2, cw, ch, seed=n)[:, Y0:Y0 + ch, X0:X0 + cw])
        for kind, frames in (("u8", crop8), ("u16", crop8.astype(np.uint16) * 257 ^ (n * 77 & 255))):
            frames = np.ascontiguousarray(frames.astype(DTYPES[kind]))
            tx, ty = c_tables(cw, 0, cw, ow, "bilinear"), c_tables(ch, 0, ch, oh, "bilinear")
            launch = Launch(gpu, kind, frames, (2, oh, ow, 3), (0, 0, ow, oh), tx, ty)
            assert launch.run(gpu) == 0
            mine = launch.check(tag=(kind, cw, ch, ow, oh))
            older = torch.empty(launch.out_bytes, dtype=torch.uint8, device=gpu)
            rc = getattr(lib, "maua_crop_resize_" + kind)(launch.fin.data_ptr(), older.data_ptr(), 2, ch, cw, 0, 0, cw, ch, ow, oh, st)
            assert rc == 0
            assert np.array_equal(older.cpu().numpy().view(DTYPES[kind]).reshape(mine.shape), mine), (kind, cw, ch, ow, oh)


@pytest.mark.gpu
def test_two_runs_give_identical_bits(gpu):
    for kind, case in (("u8", CASE["down"]), ("u16", CASE["pad-window"]), ("u16", TWOPASS_U16)):
        first = _run_case(gpu, kind, case, seed=9).result()
        second = _run_case(gpu, kind, case, seed=9).result()
        assert np.array_equal(first, second)


@pytest.mark.gpu
def test_refusals_leave_the_output_untouched(gpu):
    base = dict(kind="u8", batch=2, src=(20, 11), size=(33, 17), filt="bicubic", out=(40, 20), at=(3, 2))
    launch = geometry(gpu, **base)
    batch, in_h, in_w, out_h, out_w, x, y, w, h = launch.geo

    def geo(**kw):
        d = dict(batch=batch, in_h=in_h, in_w=in_w, out_h=out_h, out_w=out_w, x=x, y=y, w=w, h=h)
        d.update(kw)
        return tuple(d.values())

    refused = [
        (dict(inp=None), EINVAL), (dict(out=None), EINVAL),
        (dict(kx=None), EINVAL), (dict(by=None), EINVAL),                                   # one table of an axis without the other
        (dict(ksx=0), EINVAL), (dict(ksy=65), EINVAL), (dict(ksx=-1), EINVAL),                # taps outside 1 .. 64
        (dict(geo=geo(x=8)), EINVAL), (dict(geo=geo(y=4)), EINVAL), (dict(geo=geo(x=-1)), EINVAL), (dict(geo=geo(y=-2)), EINVAL),
        (dict(geo=geo(w=0)), EINVAL), (dict(geo=geo(h=-1)), EINVAL), (dict(geo=geo(in_h=0)), EINVAL), (dict(geo=geo(out_w=0)), EINVAL),
        (dict(geo=geo(batch=-1)), EINVAL), (dict(geo=geo(batch=65536)), ENOSYS),
        (dict(kx=None, bx=None), EINVAL),                                                   # a copied axis of unequal lengths
        (dict(out=launch.fin.data_ptr() + 5), EINVAL),                                        # out overlaps in
    ]
    for override, code in refused:
        assert launch.run(gpu, **override) == code, override
        assert launch.g.untouched("out"), override
    assert launch.run(gpu, geo=geo(batch=0)) == 0 and launch.g.untouched("out")             # an empty batch: nothing is launched
    launch.g.check()
    two = geometry(gpu, "u16", *TWOPASS_U16[1:5])
    assert two.run(gpu, ws=None) == EINVAL and two.run(gpu, ws=two.fin.data_ptr()) == EINVAL  # a needed workspace: NULL, overlapping in
    assert two.run(gpu, inp=two.fin.data_ptr() + 1) == EINVAL                                # 16-bit samples at an odd address
    assert two.g.untouched("out") and two.g.untouched("ws")
    two.g.check()


@pytest.mark.gpu
def test_captured_launch_replays_on_changed_input(gpu):
    """One capture of the fused and of the two-launch form (no allocation, no synchronisation inside the entry), replayed on new input."""
    stream = torch.cuda.Stream(gpu)
    for kind, case in (("u8", CASE["pad-window"]), ("u16", TWOPASS_U16)):
        name, batch, src, size, filt, box, out, at = case
        launch = geometry(gpu, kind, batch, src, size, filt, box, out, at, seed=1)
        other = make_frames(kind, batch, src[1], src[0], seed=2)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc = launch.run(gpu)
            assert rc == 0
            launch.fin.copy_(torch.from_numpy(other.reshape(-1).view(np.uint8).copy()).to(gpu))
            graph.replay()
            stream.synchronize()
        launch.frames = other
        launch.check(inside=rr.resize(other, size, filt, box), tag=name)
