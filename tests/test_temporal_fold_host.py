"""CPU: temporal supersampling without a device — the shutters, the sRGB tables of the linear-light fold and their properties, the
accumulator bound and the exact division the kernel relies on, the CLI flags and the way a fold travels from generate() into the render
loop, the scatter in units of delivered frames on a 2-rank gloo group, the generated code's resource usage and the entry's refusals."""
import argparse
import inspect
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from temporal_fold_ref import accumulate_ref, fold_ref, shutter_ref, srgb_encode_all, srgb_tables_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------------------------------------------------------- shutters and settings
def test_shutter_weights_box_tent_and_lists(built_lib):
    from maua_stylegan2_amd import render

    tents = {1: (1,), 2: (1, 1), 5: (1, 2, 3, 2, 1), 8: (1, 2, 3, 4, 4, 3, 2, 1)}
    for n in (1, 2, 5, 8):
        assert render.shutter_weights("box", n) == (1,) * n
        assert render.shutter_weights("tent", n) == tents[n] == tuple(shutter_ref("tent", n))
    assert render.shutter_weights("1,1,0,0", 4) == (1, 1, 0, 0)      # a 180 degree shutter
    assert render.shutter_weights("255", 1) == (255,) and render.shutter_weights(" 1, 2 ,3", 3) == (1, 2, 3)
    fold = render.TemporalFold(4, "1,1,0,0", "linear")
    assert (fold.subframes, fold.weights, fold.light) == (4, (1, 1, 0, 0), "linear")
    fold = render.TemporalFold(8)
    assert (fold.shutter, fold.light, fold.weights) == ("box", "encoded", (1,) * 8)
    assert render.TemporalFold(16, "tent").weights == tuple(min(i + 1, 16 - i) for i in range(16))


@pytest.mark.parametrize("shutter,n", [("1,1,0", 4), ("1,2,3,4,5", 4), ("0,0,0,0", 4), ("0", 1), ("1,256", 2), ("1,-1", 2), ("1,x", 2),
                                       ("", 1), ("gauss", 3), ("1.5,2", 2), ("1,,2", 3)])
def test_shutter_refusals(built_lib, shutter, n):
    from maua_stylegan2_amd import render

    with pytest.raises(ValueError, match="shutter"):
        render.shutter_weights(shutter, n)
    with pytest.raises(ValueError, match="shutter"):
        render.TemporalFold(n, shutter)


def test_settings_refusals_and_the_environment(built_lib, monkeypatch):
    from maua_stylegan2_amd import render

    for bad in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError, match="subframes"):
            render.TemporalFold(bad)
    with pytest.raises(ValueError, match="light"):
        render.TemporalFold(2, "box", "gamma")
    for name in ("MAUA_SUBFRAMES", "MAUA_SHUTTER", "MAUA_SHUTTER_LIGHT"):
        monkeypatch.delenv(name, raising=False)
    assert render._fold_from_env() is None
    monkeypatch.setenv("MAUA_SHUTTER", "tent")  # without $MAUA_SUBFRAMES the other two mean nothing
    assert render._fold_from_env() is None
    monkeypatch.setenv("MAUA_SUBFRAMES", "4")
    monkeypatch.setenv("MAUA_SHUTTER_LIGHT", "linear")
    fold = render._fold_from_env()
    assert (fold.subframes, fold.weights, fold.light) == (4, (1, 2, 2, 1), "linear")
    monkeypatch.setenv("MAUA_SUBFRAMES", "1")   # one sub-frame is the plain render, whatever the other two say
    monkeypatch.setenv("MAUA_SHUTTER", "1,1,0,0")
    assert render._fold_from_env() is None
    monkeypatch.setenv("MAUA_SUBFRAMES", "four")
    with pytest.raises(ValueError, match="MAUA_SUBFRAMES"):
        render._fold_from_env()
    monkeypatch.setenv("MAUA_SUBFRAMES", "17")
    with pytest.raises(ValueError, match="subframes"):
        render._fold_from_env()


# ---------------------------------------------------------------------------------------------------------------------------- tables
def test_srgb_tables_and_their_properties(built_lib):
    from maua_stylegan2_amd import render

    decode, threshold = render.srgb_fold_tables()
    want_decode, want_threshold = srgb_tables_ref()
    assert decode.dtype == threshold.dtype == np.uint16 and decode.shape == threshold.shape == (256,)
    assert np.array_equal(decode, want_decode) and np.array_equal(threshold, want_threshold)
    assert decode[0] == 0 and decode[255] == 65535 and threshold[0] == 0
    encoded = srgb_encode_all()
    assert np.all(np.diff(encoded) >= 0) and encoded[0] == 0 and encoded[-1] == 255        # the code is monotone in L
    assert np.all(np.diff(threshold.astype(np.int64)) >= 0)
    assert np.array_equal(encoded[decode], np.arange(256))                                # encode(decode[v]) == v, all 256
    searched = np.searchsorted(threshold, np.arange(65536), side="right") - 1             # max{v : threshold[v] <= L}
    assert np.array_equal(searched, encoded)                                              # the search IS the formula, all 65536 L
    render.check_fold_tables(decode, threshold)
    for bad in (threshold[::-1].copy(), np.where(np.arange(256) == 0, 1, threshold).astype(np.uint16), threshold[:255], threshold.astype(np.int32)):
        with pytest.raises(ValueError):
            render.check_fold_tables(decode, bad)
    # N = 1 is the identity in linear light with these tables, whatever the single weight
    ramp = np.arange(256, dtype=np.uint8)[None, :]
    for w in (1, 7, 255):
        assert np.array_equal(fold_ref(ramp, [w], decode, threshold), ramp)


def test_accumulator_bound_and_the_exact_multiply_shift():
    """The largest numerator, sixteen weights of 255 on the largest table entry plus the rounding term, stays below 2^28; for numerators
    below 2^28 and every W in 1 .. 4080, (n * ceil(2^40 / W)) >> 40 == n // W (checked on the numerators next to every multiple of W the
    kernel can meet, where a wrong reciprocal would show first) and the product fits 64 bits."""
    worst = 16 * 255 * 65535
    assert worst == 267382800 and worst + (16 * 255) // 2 < 2 ** 28 < 2 ** 32
    frames = np.full((16, 3), 255, np.uint8)
    mean, total = accumulate_ref(frames, [255] * 16, np.full(256, 65535, np.uint16))
    assert total == 4080 and np.all(mean == 65535)
    for w in range(1, 4081):
        magic = -(-(1 << 40) // w)
        top = w * 65535 + w // 2  # the largest numerator with this W
        assert top < 2 ** 28 and top * magic < 2 ** 64
        q = np.unique(np.concatenate([np.arange(0, 65536, 257), np.array([1, 2, 65534, 65535])])).astype(object)
        for n in np.concatenate([q * w - 1, q * w, q * w + 1, q * w + w - 1]):
            if 0 <= n <= top:
                assert (int(n) * magic) >> 40 == int(n) // w, (w, n)


def test_reference_folds_known_answers():
    frames = np.array([[0, 10, 255, 1], [1, 20, 255, 2], [3, 30, 255, 4], [4, 40, 255, 9]], np.uint8)
    assert fold_ref(frames, [1, 1]).tolist() == [[1, 15, 255, 2], [4, 35, 255, 7]]      # halves round up
    assert fold_ref(frames, [1, 2, 3, 0]).tolist() == [[(0 + 2 + 9 + 3) // 6, (10 + 40 + 90 + 3) // 6, 255, (1 + 4 + 12 + 3) // 6]]
    assert fold_ref(frames, [1, 1, 0, 0]).tolist() == [[1, 15, 255, 2]]


# --------------------------------------------------------------------------------------------------------------- CLI and the way in
def test_cli_flags_defaults_and_position(built_lib):
    from maua_stylegan2_amd import generate_audiovisual as gav

    parser = gav.build_parser()
    args = parser.parse_args([])
    assert (args.subframes, args.shutter, args.shutter_light) == (1, "box", "encoded")
    args = parser.parse_args(["--subframes", "8", "--shutter", "1,1,1,1,0,0,0,0", "--shutter_light", "linear"])
    assert (args.subframes, args.shutter, args.shutter_light) == (8, "1,1,1,1,0,0,0,0", "linear")
    with pytest.raises(SystemExit):
        parser.parse_args(["--shutter_light", "gamma"])
    with pytest.raises(SystemExit):
        parser.parse_args(["--subframes", "two"])
    flags = [flag for flag, _ in gav.CLI_FLAGS]
    assert flags[flags.index("--pipe_pix_fmt") + 1] == "--mjpeg_quality"
    assert flags[flags.index("--mjpeg_quality") + 1:] == ["--subframes", "--shutter", "--shutter_light"]
    assert gav._fold_of(parser.parse_args([])) is None and gav._fold_of(argparse.Namespace()) is None
    assert gav._fold_of(parser.parse_args(["--shutter", "tent"])) is None  # one sub-frame: the plain render
    fold = gav._fold_of(parser.parse_args(["--subframes", "4", "--shutter", "tent"]))
    assert (fold.subframes, fold.weights, fold.light) == (4, (1, 2, 2, 1), "encoded")


def test_pinned_signatures_hold_and_render_folded_exists(built_lib):
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render

    shard = list(inspect.signature(render.render_shard).parameters)
    assert shard[-2:] == ["transport", "pipe_pix_fmt"] and len(shard) == 17
    folded = inspect.signature(render.render_folded).parameters
    assert list(folded) == shard + ["fold"] and folded["fold"].default is None
    assert list(inspect.signature(render.render).parameters)[-1] == "ffmpeg_preset"
    for fn in (render.render, gav.generate):
        assert not {"fold", "subframes", "shutter", "shutter_light"} & set(inspect.signature(fn).parameters)
    assert list(inspect.signature(render.fold_frames).parameters) == ["u8", "fold", "scratch"]


def test_frame_counts_are_checked_before_anything_runs(built_lib):
    from maua_stylegan2_amd import render

    fold = render.TemporalFold(4)
    args = (None, torch.zeros(28, 1, 1), [], 0, 1.0)
    tail = (512, None, None, 1.0, [], {}, False, "slow")
    with pytest.raises(ValueError, match=r"--batch 6 is not a multiple of --subframes 4.*--batch 8"):
        render.render_folded(*args, 6, *tail, None, fold=fold)
    with pytest.raises(ValueError, match="--batch 16"):
        render.render_folded(*args, 8, *tail, None, fold=render.TemporalFold(16))
    with pytest.raises(ValueError, match="whole groups of 4"):
        render.render_folded(None, torch.zeros(30, 1, 1), [], 0, 1.0, 8, *tail, None, fold=fold)
    with pytest.raises(ValueError, match="whole groups of 4"):
        render.render_folded(*args, 8, *tail, (0, 14, 28), fold=fold)
    assert render.fold_shard_bounds(28, 4, 0, 2) == (0, 16) and render.fold_shard_bounds(28, 4, 1, 2) == (16, 28)
    assert render.fold_shard_bounds(28, 1, 1, 2) == (14, 28)


def test_generate_renders_at_the_sub_frame_rate_and_delivers_at_fps(monkeypatch, tmp_path, built_lib):
    """--fps F --subframes N is --fps F * N up to and including synthesis: n_frames = N * round(duration * F), args.fps = F * N, the
    smoothing factor of F * N; args.video_fps = F.  Without --subframes nothing moves."""
    from maua_stylegan2_amd import audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (np.zeros(8, np.float32), 100, 2.1))
    monkeypatch.setattr(ar, "generate_latents", lambda *a, **kw: torch.zeros(3, 2, 4))
    monkeypatch.setattr(gav, "_cached_generator", lambda *a, **kw: ("G", True))
    smf, seen, rendered = [], {}, []
    monkeypatch.setattr(ar, "set_SMF", lambda v: smf.append(v))

    def get_latents(selection, args):
        seen.update(fps=args.fps, n_frames=args.n_frames, video_fps=args.video_fps, subframes=args.subframes)
        return torch.zeros(args.n_frames, 2, 4)

    for name in ("MAUA_PIPE_PIX_FMT", "MAUA_SUBFRAMES", "MAUA_DELIVER_SIZE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(gav.render, "render_frames", lambda *a, **kw: rendered.append((a, kw)) or len(a[1]))
    plain = dict(pipe_pix_fmt=None, fold=None, resize=None, grade=None, lens=None, feedback=None)
    common = dict(ckpt=None, audio_file="a.wav", get_latents=get_latents, get_noise=lambda **kw: None, fps=24, batch=8, out_size=512, G_res=512)

    def run(**extra):
        args = argparse.Namespace(**common, **extra, offset=0, duration=-1, latent_file=None, latent_count=3, noconst=False, latent_dim=4,
                                  n_mlp=2, channel_multiplier=2, shuffle_latents=False)
        gav.generate(**common, output_file="o.mp4", args=args)
        return args

    run()
    assert seen == dict(fps=24, n_frames=50, video_fps=24, subframes=1) and smf[-1] == 24 / 30
    assert len(rendered[-1][0]) == 15 and rendered[-1][0][3:6] == (0, 2.1, 8) and rendered[-1][1] == plain  # no fold reaches the body
    run(subframes=1, shutter="tent", shutter_light="linear")
    assert seen == dict(fps=24, n_frames=50, video_fps=24, subframes=1) and len(rendered[-1][0]) == 15 and rendered[-1][1] == plain
    args = run(subframes=4, shutter="tent", shutter_light="linear")
    assert seen == dict(fps=96, n_frames=200, video_fps=24, subframes=4) and smf[-1] == 96 / 30
    assert (args.fps, args.n_frames, args.video_fps, args.subframes) == (96, 200, 24, 4)
    fold = rendered[-1][1]["fold"]
    assert rendered[-1][1] == dict(plain, fold=fold) and (fold.subframes, fold.weights, fold.light) == (4, (1, 2, 2, 1), "linear")
    assert len(rendered[-1][0]) == 15 and len(rendered[-1][0][1]) == 200 and rendered[-1][0][4] == 2.1


# ------------------------------------------------------------------------------------------------- sharding in units of delivered frames
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


N_OUT, SUB = 7, 4


def _scatter_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from maua_stylegan2_amd import generate_audiovisual as gav
        from maua_stylegan2_amd import render

        n = N_OUT * SUB
        frames = torch.arange(n, dtype=torch.float32)
        latents = (frames[:, None, None] + torch.tensor([0.0, 0.25])[None, :, None] + torch.zeros(1, 1, 3)) if rank == 0 else None
        noise = [frames[:, None, None, None] * torch.ones(1, 1, 2, 2), None, 100 + frames[:, None, None, None] * torch.ones(1, 1, 4, 4)] if rank == 0 else []
        truncation = frames / 100 if rank == 0 else None
        bends = [{"layer": 0, "transform": None, "modulation": 7 * frames[:, None]}]
        rewrites = {"w": [None, 9 * frames[:, None]]}
        lat, nz, trunc = gav._scatter_from_rank0(latents, noise, truncation, bends, rewrites, n, SUB)
        lo, hi = render.fold_shard_bounds(n, SUB, rank, world)
        assert (lo, hi) == ((0, 16), (16, 28))[rank]  # 4 + 3 delivered frames: no group straddles the ranks
        mine = frames[lo:hi]
        assert lat.shape == (hi - lo, 2, 3) and torch.equal(lat[:, 0, 0].cpu(), mine) and torch.equal(lat[:, 1, 2].cpu(), mine + 0.25)
        assert len(nz) == 3 and nz[1] is None
        assert nz[0].shape == (hi - lo, 1, 2, 2) and torch.equal(nz[0][:, 0, 1, 1].cpu(), mine)
        assert nz[2].shape == (hi - lo, 1, 4, 4) and torch.equal(nz[2][:, 0, 3, 0].cpu(), mine + 100)
        assert trunc.shape == (hi - lo,) and torch.equal(trunc.cpu(), mine / 100)
        assert torch.equal(bends[0]["modulation"].cpu(), 7 * mine[:, None]) and torch.equal(rewrites["w"][1].cpu(), 9 * mine[:, None])
        # the plain scatter of the same job cuts at 14: the two differ, and the default argument is the plain one
        lat1, _, _ = gav._scatter_from_rank0(latents, [], 1.0, [], {}, n)
        assert lat1.shape[0] == 14 and float(lat1[0, 0, 0]) == 14.0 * rank
        torch.save({"lo": lo, "hi": hi}, os.path.join(out_dir, f"scatter{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_scatter_in_units_of_delivered_frames_on_two_ranks(tmp_path, built_lib):
    mp.spawn(_scatter_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(tmp_path / f"scatter{r}.pt", weights_only=False) for r in (0, 1)]
    assert [(g["lo"], g["hi"]) for g in got] == [(0, 16), (16, 28)]


# ------------------------------------------------------------------------------------------------------- generated code and the entry
@pytest.fixture(scope="module")
def fold_build(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("isa") / "temporal_fold.s")
    done = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                           f"-I{REPO}/include", f"{REPO}/maua_stylegan2_amd/csrc/temporal_fold.hip", "-o", dst], check=True, capture_output=True,
                          text=True)
    return open(dst).read(), done.stderr


def _metadata(asm, key):
    names = [n for n in re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M) if n.startswith("_Z")]
    values = [int(v) for v in re.findall(rf"^\s+\.{key}:\s+(\d+)", asm, flags=re.M)]
    assert names and len(names) == len(values), (names, values)
    return dict(zip(names, values))


def test_fold_kernels_use_no_scratch_and_vector_accesses(fold_build):
    asm, remarks = fold_build
    usage = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)",
                       remarks, flags=re.S)
    assert len(usage) == 4 and all("temporal_fold_kernel" in name for name, *_ in usage), usage  # {encoded, linear} x {vector, byte}
    for name, scratch, sgpr_spill, vgpr_spill, lds in usage:
        assert (int(scratch), int(sgpr_spill), int(vgpr_spill)) == (0, 0, 0), (name, scratch, sgpr_spill, vgpr_spill)
        assert int(lds) == (1024 if "ILb1E" in name else 0), (name, lds)  # linear light: the two 512-byte tables, nothing else
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert all(v == 0 for v in _metadata(asm, key).values())
    assert all(v <= 64 for v in _metadata(asm, "vgpr_count").values())  # full occupancy: the kernel hides its loads with waves
    assert asm.count("global_load_dwordx4") >= 2 and asm.count("global_store_dwordx4") == 2  # the aligned body of both vector kernels


def test_entry_refuses_bad_arguments_without_a_device(built_lib):
    import ctypes

    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    assert "maua_temporal_fold_u8" in _lib.exported_symbols() and len(_lib._SIGNATURES["maua_temporal_fold_u8"][1]) == 9
    assert lib.maua_abi_version() == _lib.ABI_VERSION == 8
    fake_in, fake_out, tables = 0x100000, 0x900000, 0x800000  # never dereferenced
    ones = (ctypes.c_uint8 * 16)(*([1] * 16))
    zeros = (ctypes.c_uint8 * 16)()

    def call(groups=1, n=4, fb=64, src=fake_in, dst=fake_out, w=ones, dec=None, thr=None):
        return lib.maua_temporal_fold_u8(src, dst, groups, n, fb, w, dec, thr, None)

    for n in (0, -1, 17, 1 << 20):
        assert call(n=n) == -22, n
    assert call(w=zeros) == -22 and call(n=16, w=zeros) == -22               # W == 0
    assert call(n=2, w=(ctypes.c_uint8 * 2)(0, 0)) == -22
    assert call(fb=0) == -22 and call(fb=-16) == -22
    assert call(dec=tables) == -22 and call(thr=tables) == -22               # exactly one table
    assert call(src=None) == -22 and call(dst=None) == -22 and call(w=None) == -22
    assert call(groups=-1) == -22
    # out overlapping in: inside, at its start, one byte into its end, and in starting inside out
    for dst in (fake_in, fake_in + 64, fake_in + 4 * 64 - 1, fake_in - 63):
        assert call(dst=dst) == -22, hex(dst)
    assert call(groups=0) == 0 and call(groups=0, src=None, dst=None) == 0   # an empty launch succeeds and touches nothing
    assert call(groups=0, w=zeros) == -22 and call(groups=0, n=17) == -22   # ... but its arguments are still checked
