"""Audio-reactive video synthesis on MI355X — the drop-in for /root/reference/generate_audiovisual.py.

What is kept from the reference: the keyword contract and defaults of ``generate(...)``
(generate_audiovisual.py:59-91), the ``args`` namespace it builds from its own arguments and extends with ``audio``,
``sr``, ``duration``, ``n_frames`` (:94-113), the callback protocol — ``initialize(args)``, ``get_latents(selection,
args)``, ``get_noise(height, width, scale, num_scales, args)``, ``get_bends(args)``, ``get_rewrites(args)``,
``get_truncation(args)`` (:115-186) — the CLI flags and the plugin file's ``OVERRIDE`` dict (:234-299), and the side
effects ``workspace/last-latents.npy`` / ``output/<track>_<ckpt>_<id>.mp4``.

What is different: features come from HIP STFT/mel/chroma kernels, latents and noise stay in HBM, the generator is
hipGraph-replayed, frames leave as uint8, and under ``torchrun`` every GPU renders a contiguous shard of the frames
(``--dataparallel`` is accepted and ignored).  Importing this module aliases ``audioreactive``, ``render``,
``models.stylegan2`` and ``op`` to this package's mirrors so unmodified reference plugin files run.

Temporal supersampling (not in the reference): ``--fps F --subframes N`` is ``--fps F * N`` up to and including synthesis; the frames are
then folded N:1 on the device (``--shutter``, ``--shutter_light``; render.TemporalFold) and written at F.  ``--batch`` must be a multiple
of N.

Colour grading (not in the reference): a plugin's ``initialize`` (or its ``OVERRIDE``, or the caller's ``args``) leaves an ``ar.Grade`` — or a
callable ``grade(args)`` — in ``args.grade``; ``--grade`` / ``--grade_lut`` / ``--grade_lut_mix`` build a static one.  Every rendered frame is
then graded on the device in front of the quantiser (render.grade_frames).

Lens effects (not in the reference): likewise an ``ar.Lens`` — or a callable ``lens(args)`` — in ``args.lens``, or a static ``--lens``: bloom,
sharpen and vignette on every rendered frame's fp32 image, in front of the grade (render.lens_frames).

Frame feedback (not in the reference): likewise an ``ar.Feedback`` — or a callable ``feedback(args)`` — in ``args.feedback``, or a static
``--feedback``: every rendered frame is combined with the warped, dimmed previous output, in front of the lens (render.feedback_frames).  A
recurrence over the frames: one rank only.  With --subframes N it runs per rendered sub-frame, so ``gain`` compounds N times per written frame.
"""
import argparse
import gc
import importlib
import importlib.util
import os
import random
import sys
import time
import traceback
import uuid

import numpy as np
import torch as th

from . import audioreactive as ar
from . import render, sharding
from .models.stylegan2 import Generator

CALLBACK_NAMES = ("initialize", "get_latents", "get_noise", "get_bends", "get_rewrites", "get_truncation")

# (flag, argparse keyword arguments) — the reference's 24 flags with their defaults (generate_audiovisual.py:236-259)
CLI_FLAGS = (
    ("--ckpt", dict(type=str)),
    ("--audio_file", dict(type=str)),
    ("--audioreactive_file", dict(type=str, default="audioreactive/examples/default.py")),
    ("--output_dir", dict(type=str, default="./output")),
    ("--offset", dict(type=float, default=0)),
    ("--duration", dict(type=float, default=-1, help="length of rendered video in seconds")),
    ("--latent_file", dict(type=str, default=None)),
    ("--shuffle_latents", dict(action="store_true")),
    ("--G_res", dict(type=int, default=1024)),
    ("--out_size", dict(type=int, default=1024, help="rendered video size. Options: 512, 1024, 1920")),
    ("--fps", dict(type=int, default=30)),
    ("--latent_count", dict(type=int, default=12)),
    ("--batch", dict(type=int, default=8)),
    ("--dataparallel", dict(action="store_true")),
    ("--truncation", dict(type=float, default=1.0)),
    ("--stylegan1", dict(action="store_true")),
    ("--noconst", dict(action="store_true")),
    ("--latent_dim", dict(type=int, default=512)),
    ("--n_mlp", dict(type=int, default=8)),
    ("--channel_multiplier", dict(type=int, default=2)),
    ("--randomize_noise", dict(action="store_true")),
    ("--base_res_factor", dict(type=float, default=1)),
    ("--ffmpeg_preset", dict(type=str, default="slow")),
    ("--output_file", dict(type=str, default=None)),
    # (not one of the reference's: what travels to the encoder — planar 4:2:0 is made on the device, render.frames_to_yuv420p)
    # ... or one baseline JPEG per frame, render.frames_to_mjpeg, at --mjpeg_quality 1 .. 95)
    # ... or a deep format, render.frames_to_deep: 16-bit RGB / 10-bit BT.709 YUV from the fp32 image, encoded as HEVC Main10)
    ("--pipe_pix_fmt", dict(type=str, default="rgb24", choices=render.PIPE_PIX_FMTS + render.DEEP_PIX_FMTS)),
    ("--mjpeg_quality", dict(type=int, default=render.MJPEG_DEFAULT_QUALITY)),
    # (temporal supersampling, render.TemporalFold: --fps F --subframes N is --fps F * N up to and including synthesis; the frames are then
    # folded N:1 on the device and written at F)
    ("--subframes", dict(type=int, default=1, help="sub-frames rendered and averaged per video frame (1 .. 16)")),
    ("--shutter", dict(type=str, default="box", help="box, tent or N comma-separated integer weights, e.g. 1,1,0,0")),
    ("--shutter_light", dict(type=str, default="encoded", choices=render.SHUTTER_LIGHTS)),
)
# (delivery at any size, render.FrameResize: every frame is resampled on the device before the colour conversion.
# A table of its own: tests hold the order of CLI_FLAGS)
DELIVERY_FLAGS = (
    ("--deliver_size", dict(type=str, default=None, help="WIDTHxHEIGHT of the written video, e.g. 1920x1080 (default: the generator's)")),
    ("--deliver_filter", dict(type=str, default="lanczos", choices=render.RESIZE_FILTERS)),
    ("--deliver_fit", dict(type=str, default="crop", choices=render.RESIZE_FITS)),
)
# (colour grading, audioreactive/grade.py + csrc/grade.hip: static flags that build a one-row ar.Grade; a modulated grade comes from the
# plugin as ``args.grade``.  A table of its own again)
GRADE_FLAGS = (
    ("--grade_lut", dict(type=str, default=None, help="a 3-D .cube file applied to every frame after the CDL and the matrix")),
    ("--grade_lut_mix", dict(type=float, default=1.0, help="weight of --grade_lut, 0 .. 1")),
    ("--grade", dict(type=str, default=None, dest="grade_spec",
                     help='a static grade, e.g. "exposure=0.3,saturation=1.2,gamma=0.9,hue=15" (keys: ' + ", ".join(ar.grade.SPEC_KEYS) + ")")),
)

# (lens effects, audioreactive/lens.py + csrc/lens.hip: one static flag that builds a one-row ar.Lens; a modulated lens comes from the plugin
# as ``args.lens``)
LENS_FLAGS = (
    ("--lens", dict(type=str, default=None, dest="lens_spec",
                    help='static lens effects, e.g. "bloom=0.8,bloom_size=0.03,bloom_threshold=0.6,sharpen=0.4,vignette=0.3" (keys: '
                         + ", ".join(ar.lens.SPEC_KEYS) + ")")),
)

# (frame feedback, audioreactive/feedback.py + csrc/feedback.hip: one static flag that builds a one-row ar.Feedback; a modulated one comes
# from the plugin as ``args.feedback``)
FEEDBACK_FLAGS = (
    ("--feedback", dict(type=str, default=None, dest="feedback_spec",
                        help='static frame feedback (trails), e.g. "gain=0.92,zoom=1.015,rotate=0.3,mode=max,border=mirror" (keys: '
                             + ", ".join(ar.feedback.SPEC_KEYS) + "); one rank only")),
)
# The frame effects (audioreactive/frame_table.py), in the order of their flags: (name, class, flags).  ``args.<name>`` and
# ``args.<name>_spec`` hold an effect (_effect_of), ``ar.<name>.parse_spec`` reads its static flag.  The parser, the keys main() keeps out
# of generate()'s settings and the per-job "is it set on rank 0" broadcasts are derived from this table: a new effect is a row here
EFFECTS = (("grade", ar.Grade, GRADE_FLAGS), ("lens", ar.Lens, LENS_FLAGS), ("feedback", ar.Feedback, FEEDBACK_FLAGS))


def _install_aliases():
    from . import models, op
    from .models import stylegan2

    for name, mod in (("audioreactive", ar), ("render", render), ("op", op), ("models", models),
                      ("models.stylegan2", stylegan2)):
        sys.modules.setdefault(name, mod)


_install_aliases()


def get_noise_range(out_size, generator_resolution, is_stylegan1):
    """(first scale, one-past-last scale, scale -> log2 side) for an output size / generator resolution.
    StyleGAN2 has two noise maps per resolution above 4 px and one at 4 px (reference :22-34)."""
    top = int(np.log2(out_size))
    bottom = 2 + (top - int(np.log2(generator_resolution)))
    if is_stylegan1:
        return bottom, top + 1, (lambda s: s)
    return 2 * bottom + 1, 2 * (top + 1), (lambda s: int(s / 2))


def load_generator(ckpt, is_stylegan1, G_res, out_size, noconst, latent_dim, n_mlp, channel_multiplier, dataparallel,
                   base_res_factor):
    """Reference :37-56.  Only rank 0 reads the checkpoint; the other ranks receive the weights over RCCL."""
    rank, _ = sharding.rank_world()
    if is_stylegan1:
        from .models.stylegan1 import G_style

        # only rank 0 probes the checkpoint for the network resolution (1024 -> 512 -> 256 -> 128); the other ranks build that
        # very network, so that blocks, the enlarged constant and the noise buffers have one shape everywhere before broadcast_module
        generator = G_style(output_size=out_size, checkpoint=ckpt) if rank == 0 else None
        resolution = int(sharding.broadcast_object(generator.network_resolution if rank == 0 else None))
        if generator is None:
            generator = G_style(output_size=out_size, checkpoint=None, network_resolution=resolution)
        generator = generator.cuda()
        generator.truncation_latent = sharding.broadcast_tensor(generator.truncation_latent.cuda().contiguous())
        return sharding.broadcast_module(generator).eval()
    # The module is built ON the device (torch's default-device context: every factory call of the constructors allocates there) and the
    # checkpoint's tensors are copied into it one by one: no CPU copy of the module first and no module-wide .cuda() (0.06 + 0.08 s of
    # a 1.1 s job in round 5's profile; the reference builds on the CPU, generate_audiovisual.py:43-53)
    with th.device(th.device("cuda", th.cuda.current_device())):
        generator = Generator(G_res, latent_dim, n_mlp, channel_multiplier=channel_multiplier, constant_input=not noconst,
                              checkpoint=ckpt if rank == 0 else None, output_size=out_size, base_res_factor=base_res_factor)
    generator = generator.cuda()  # (a no-op for what is there already; anything a constructor left on the CPU follows)
    return sharding.broadcast_module(generator).eval()


# One generator is kept across generate() calls of a process (a notebook / a server rendering track after track from one checkpoint):
# the packed weights and the captured graph lanes hang off the module, so a job on the same checkpoint file (path, mtime, size) and the
# same architecture flags starts rendering without reloading, re-packing or re-capturing anything.  What the reference re-draws per
# job is re-drawn here as well (the lazy random truncation centre, resized random noise buffers).  MAUA_GENERATOR_CACHE=0 turns it off;
# one process per GPU (a process group) always loads (rank 0 reads, the others receive the broadcast).
_GENERATOR_CACHE = {}


def _cached_generator(load, ckpt, flags, before_load=lambda: None):
    """(generator, came from the cache).  ``before_load`` runs in front of every real load (generate() passes its one full collection)."""
    if sharding.grouped() or os.environ.get("MAUA_GENERATOR_CACHE", "1") in ("0", "") or ckpt is None:
        before_load()
        return load(), False
    try:
        st = os.stat(ckpt)
    except OSError:
        before_load()
        return load(), False
    key = (os.path.realpath(ckpt), st.st_mtime_ns, st.st_size, th.cuda.current_device()) + tuple(flags)
    hit = _GENERATOR_CACHE.get("entry")
    if hit is not None and hit[0] == key:
        generator = hit[1]
        if hasattr(generator, "n_latent"):  # StyleGAN2: the truncation centre is a fresh draw per job (models/stylegan2.py:539-540)
            generator.truncation_latent = None
            if getattr(generator, "_random_noise_buffers", False):  # resized noise buffers are random per construction (:461-470)
                for i in range(generator.num_layers):
                    getattr(generator.noises, f"noise_{i}").normal_()
        return generator, True
    _GENERATOR_CACHE.pop("entry", None)  # (one entry: a generator owns GBs of static buffers)
    before_load()
    generator = load()
    _GENERATOR_CACHE["entry"] = (key, generator)
    return generator, False


def _seed_all(seed):
    """torch (CPU and device generators), numpy and python generators of this process."""
    th.manual_seed(seed)
    np.random.seed(seed % (2 ** 32))
    random.seed(seed)


def _noise_sides(out_size):
    """(height multiplier, width multiplier) of the noise maps for portrait / landscape HD output (reference :150-151)."""
    return (2 if out_size == 1080 else 1), (2 if out_size == 1920 else 1)


def _collect_noise(get_noise, args, out_size, G_res, stylegan1, header=None):
    first, stop, log_side = get_noise_range(out_size, G_res, stylegan1)
    mul_h, mul_w = _noise_sides(out_size)
    maps, shown = [], []
    for scale in range(first, stop):
        side = 2 ** log_side(scale)
        nz = get_noise(height=mul_h * side, width=mul_w * side, scale=scale - first, num_scales=stop - first, args=args)
        if isinstance(nz, ar.NoiseSynth) and (nz.height, nz.width) != (mul_h * side, mul_w * side):
            raise RuntimeError(f"get_noise returned a NoiseSynth of {nz.height} x {nz.width} maps for the {mul_h * side} x {mul_w * side} scale")
        if nz is not None:  # (a recipe's amplitude comes from a bounded sample of its frames: nothing is materialised)
            shown.append((list(nz.shape), nz.std()))  # (printed below: formatting a device scalar is a host sync per scale)
        maps.append(nz)
    if header is not None:
        header()
    if shown:  # one D2H for all scales instead of one synchronisation each (16 x 6 ms in round 5's profile); same lines, same order
        for shape, amp in zip([s for s, _ in shown], th.stack([a.detach().float().reshape(()) for _, a in shown]).tolist()):
            print(shape, f"amplitude={amp}")
    # (the reference collects + empties the cache after every scale, generate_audiovisual.py:157-158, to fit small GPUs: 17 full collections cost
    # 0.7 s here.  The filtered fields are freed by refcount; generate() runs ONE full collection, right before the generator is loaded.)
    return maps


def _scatter_from_rank0(latents, noise, truncation, bends, rewrites, n_frames, subframes=1):
    """One process per GPU: rank 0 ran the audio front end and the callbacks; every rank receives only its contiguous
    block of the per-frame inputs (sharding.scatter_frames).  Bend modulations are broadcast (they are [n_frames, k]
    vectors) and cut to the block here, because the transforms that consume them are closures every rank built itself.
    ``subframes`` N > 1 (a temporal fold): the job is sharded in units of delivered frames — every per-frame tensor travels as
    [n_frames / N, N, ...] — so that a rank's block, render.fold_shard_bounds, holds whole groups of sub-frames."""
    rank, world = sharding.rank_world()
    dev = th.device("cuda", th.cuda.current_device()) if th.cuda.is_available() else th.device("cpu")
    on_dev = lambda t: None if t is None else t.to(dev, th.float32).contiguous()  # noqa: E731
    if subframes == 1:
        scatter = lambda t: sharding.scatter_frames(t, n_frames, device=dev)  # noqa: E731
    else:
        if n_frames % subframes:
            raise RuntimeError(f"{n_frames} frames are not whole groups of {subframes} sub-frames")
        n_out = n_frames // subframes

        def scatter(t):
            if t is not None and t.shape[0] != n_frames:
                raise RuntimeError(f"per-frame tensor has {t.shape[0]} entries for {n_frames} frames")
            block = sharding.scatter_frames(None if t is None else t.reshape((n_out, subframes) + tuple(t.shape[1:])), n_out, device=dev)
            return None if block is None else block.flatten(0, 1)

    latents = scatter(on_dev(latents))
    # NoiseSynth recipes are broadcast, not scattered: their structure rides along with the slot count (a job without recipes sends the
    # plain count, as before), their tensors — loops, envelopes, masks: small next to a per-frame sequence — follow one by one, and every
    # rank cuts its frames out with ``window``, which copies nothing
    lo, hi = render.fold_shard_bounds(n_frames, subframes, rank, world)
    recipes = {i: nz for i, nz in enumerate(noise) if isinstance(nz, ar.NoiseSynth)} if rank == 0 else {}
    head = sharding.broadcast_object((len(noise) if not recipes else (len(noise), {i: nz.structure() for i, nz in recipes.items()}))
                                     if rank == 0 else None)
    n_noise, structures = head if isinstance(head, tuple) else (head, {})
    noise = list(noise) if rank == 0 else [None] * n_noise
    for i in range(n_noise):
        if i in structures:
            recipe = noise[i] if rank == 0 else ar.NoiseSynth.from_structure(structures[i], dev)
            if recipe.device != dev:
                raise RuntimeError(f"noise[{i}]: the recipe lives on {recipe.device}, this rank renders on {dev}")
            for t in recipe.tensors():
                sharding.broadcast_tensor(t)
            if recipe.n_frames is not None and recipe.n_frames != n_frames:
                raise RuntimeError(f"noise[{i}]: the recipe's envelopes cover {recipe.n_frames} frames, the job has {n_frames}")
            noise[i] = recipe.window(lo, hi)
        else:
            noise[i] = scatter(on_dev(noise[i]) if rank == 0 else None)
    is_float = sharding.broadcast_object(isinstance(truncation, float) if rank == 0 else None)
    if is_float:
        truncation = float(sharding.broadcast_object(truncation if rank == 0 else None))
    else:
        truncation = scatter(on_dev(truncation) if rank == 0 else None)
    for bend in bends:
        if "modulation" in bend:
            bend["modulation"] = sharding.broadcast_tensor(on_dev(bend["modulation"]))[lo:hi]
    for name in sorted(rewrites):
        rewrite, modulation = rewrites[name]
        rewrites[name] = [rewrite, sharding.broadcast_tensor(on_dev(modulation))[lo:hi]]
    return latents, noise, truncation


def generate(ckpt, audio_file, initialize=None, get_latents=None, get_noise=None, get_bends=None, get_rewrites=None,
             get_truncation=None, output_dir="./output", audioreactive_file="audioreactive/examples/default.py",
             offset=0, duration=-1, latent_file=None, shuffle_latents=False, G_res=1024, out_size=1024, fps=30,
             latent_count=12, batch=8, dataparallel=False, truncation=1.0, stylegan1=False, noconst=False,
             latent_dim=512, n_mlp=8, channel_multiplier=2, randomize_noise=False, ffmpeg_preset="slow",
             base_res_factor=1, output_file=None, args=None):
    if args is None:  # direct (notebook) call: the namespace is this call's own arguments, as in the reference (:94-98)
        args = argparse.Namespace(**{k: v for k, v in locals().items() if k != "args"})
        args.args = None

    # Temporal supersampling (generate() keeps the reference's parameter list: --subframes / --shutter / --shutter_light arrive in the
    # namespace, as the pipe format does).  ``--fps F --subframes N`` IS ``--fps F * N`` up to and including synthesis — args.fps, the
    # smoothing factor and args.n_frames are those of the rendered rate, so plugins that count frames or smooth in seconds stay right —;
    # the frames are then folded N:1 on the device and written at F (args.video_fps).
    fold = _fold_of(args)
    subframes = 1 if fold is None else fold.subframes
    args.video_fps, args.subframes = fps, subframes
    if subframes > 1:
        args.fps = fps * subframes

    started = time.time()
    th.set_grad_enabled(False)
    ar.set_SMF(args.fps / 30)  # temporal smoothing independent of the frame rate

    rank, world = sharding.rank_world()
    grouped = sharding.grouped()  # a process group of ANY size (one rank included) takes the collective order of operations
    # One process per GPU: the audio front end and the latent / noise / truncation callbacks run on rank 0 only and their
    # per-frame results are scattered.  Bends and rewrites are closures, so a plugin that defines them is run on every rank;
    # every rank re-seeds its torch / numpy / python generators from one broadcast seed IMMEDIATELY before get_bends and before
    # get_rewrites (rank 0 has consumed draws in the latent / noise callbacks by then, the others have not), so that random
    # draws inside them — e.g. AddNoise(0.025 * th.randn(...)) in examples/kelp.py, tauceti.py — agree across shards.
    everywhere = grouped and (get_bends is not None or get_rewrites is not None)
    front_end = rank == 0 or everywhere
    if grouped:
        seed = int(sharding.broadcast_object(random.randrange(2 ** 31) if rank == 0 else None))
        if everywhere:
            _seed_all(seed)

    from .audioreactive.examples import default as default_plugin

    get_latents = get_latents or default_plugin.get_latents
    get_noise = get_noise or default_plugin.get_noise
    latents, noise, bends, rewrites = None, [], [], {}

    def load():
        return load_generator(ckpt=ckpt, is_stylegan1=stylegan1, G_res=G_res, out_size=out_size, noconst=noconst,
                              latent_dim=latent_dim, n_mlp=n_mlp, channel_multiplier=channel_multiplier,
                              dataparallel=dataparallel, base_res_factor=base_res_factor)

    # One process per GPU: the weights travel FIRST (rank 0 reads the checkpoint, one flat broadcast), so that every other rank
    # packs its weights and captures its graph lanes while rank 0 runs the audio front end and the callbacks — a captured forward
    # reads its inputs through a frame source and needs none of them (render.prepare).  A single process keeps the reference's
    # order (generator after the preprocessing, :215-224), so the callbacks see the same random stream as there.
    generator = None
    will_bend = get_bends is not None or get_rewrites is not None
    if grouped:
        generator = load()
        if rank != 0:
            render.prepare(generator, batch, bends=will_bend)

    if front_end:
        args.audio, args.sr, duration = ar.load_audio(audio_file, offset, duration)
    duration = float(sharding.broadcast_object(duration if rank == 0 else None))
    args.duration = duration
    args.n_frames = n_frames = subframes * int(round(duration * fps))  # (delivered frames = round(duration * fps), N rendered for each)
    if front_end:
        if initialize is not None:
            args = initialize(args)
    # (generate() keeps the reference's parameter list: a colour grade arrives in the namespace — ``args.grade`` set by the plugin's
    # initialize, by its OVERRIDE or by the caller, and the --grade / --grade_lut flags —; resolved on rank 0, after initialize)
    # (``args.lens`` / --lens and ``args.feedback`` / --feedback the same way)
    effects = dict(grade=_grade_of(args), lens=_lens_of(args), feedback=_feedback_of(args)) if rank == 0 else dict.fromkeys(n for n, _, _ in EFFECTS)
    on_rank0 = lambda name: sharding.broadcast_object(effects[name] is not None if rank == 0 else None)  # noqa: E731
    if grouped and world > 1 and on_rank0("feedback"):
        # (every rank raises, before the scatter: a shard's first frame needs its predecessor's state — render.render_frames)
        raise ValueError(render.FEEDBACK_ONE_RANK.format(where=f"this is a {world}-rank job"))

    if rank == 0:
        print("\ngenerating latents...")
        if latent_file is not None:
            selection = ar.load_latents(latent_file)
        else:
            selection = ar.generate_latents(args.latent_count, ckpt, G_res, noconst, latent_dim, n_mlp, channel_multiplier)
        if shuffle_latents:
            selection = selection[random.sample(range(len(selection)), len(selection))]
        os.makedirs("workspace", exist_ok=True)
        np.save("workspace/last-latents.npy", selection.numpy())
        latents = get_latents(selection=selection, args=args)
        latent_amp = latents.std()  # (formatted after the noise callbacks have been issued: no host sync in between)

        noise = _collect_noise(get_noise, args, out_size, G_res, stylegan1, header=lambda: print(
            f"{list(latents.shape)} amplitude={float(latent_amp)}\n\ngenerating noise..."))
        print()

    if front_end and get_bends is not None:
        print("generating network bends...")
        if grouped:
            _seed_all(seed + 1)
        bends = get_bends(args=args)
    if front_end and get_rewrites is not None:
        print("generating model rewrites...")
        if grouped:
            _seed_all(seed + 2)
        rewrites = get_rewrites(args=args)
    if rank == 0:
        if get_truncation is not None:
            print("generating truncation...")
            truncation = get_truncation(args=args)
        else:
            truncation = float(truncation)

    shard = None
    if grouped:
        if subframes > 1:
            latents, noise, truncation = _scatter_from_rank0(latents, noise, truncation, bends, rewrites, n_frames, subframes)
        else:
            latents, noise, truncation = _scatter_from_rank0(latents, noise, truncation, bends, rewrites, n_frames)
        lo, hi = render.fold_shard_bounds(n_frames, subframes, rank, world)
        shard = (lo, hi, n_frames)
        for name in ("grade", "lens"):  # (a feedback is not sharded: refused above)
            if on_rank0(name):  # (a job without this effect adds this one object, nothing else)
                effects[name] = _broadcast_effect(name, effects[name], lo, hi)

    # (reference :191-192.)  The job's one collection — 45-70 ms on this heap.  Full on purpose where it runs: young-generation collections
    # (tried in round 5) leave the preprocessing's cyclic garbage, device tensors among it, alive, and a render that has to LOAD its generator
    # then pays more in fresh allocations (+60 ms).  A job whose generator is already there (kept from the previous job: the allocator's
    # pools are warm, nothing large is about to be allocated) skips it — measured 0.87-0.99 s against 0.90-1.01 s per warm 900-frame job
    # (tools/e2e_config3.py --gc none / full, alternating); the interpreter's own thresholds collect the garbage of a run of jobs.
    hit = False
    if generator is None:
        generator, hit = _cached_generator(load, ckpt, (bool(stylegan1), G_res, out_size, bool(noconst), latent_dim, n_mlp, channel_multiplier,
                                                        base_res_factor), before_load=gc.collect)
    if not hit and grouped:
        gc.collect()
    if grouped and not stylegan1 and not (isinstance(truncation, float) and truncation == 1.0):
        # the truncation centre is a random draw (mean_latent(2**14), reference models/stylegan2.py:539-540): one draw, on rank
        # 0, for every shard — otherwise neighbouring shards are truncated toward slightly different centres
        centre = generator.mean_latent(2 ** 14) if rank == 0 else th.empty(1, latent_dim, device=render.device_of(generator))
        generator.truncation_latent = sharding.broadcast_tensor(centre.contiguous())
    print(f"\npreprocessing took {time.time() - started:.2f}s\n")

    print(f"rendering {n_frames} frames...")
    if output_file is None:
        stem = lambda path: str(path).split("/")[-1].split(".")[0].lower()  # noqa: E731
        output_file = f"{output_dir}/{stem(audio_file)}_{stem(ckpt)}_{uuid.uuid4().hex[:8]}.mp4"
    t0 = time.time()
    if grouped and hasattr(generator, "random_noise"):
        # randomize_noise: every rank generates the maps of its frames from the job's one broadcast seed (Generator.random_noise)
        generator.noise_seed = seed + 3
    try:
        # generate() keeps the reference's parameter list: the pipe format, the fold and the delivery size arrive in the namespace
        # (the flags, a plugin's OVERRIDE, a caller's own ``args``) or, for some jobs, through the environment (_tail_options)
        pix_fmt, fold, resize = _tail_options(args, fold, **effects)
        written = render.render_frames(generator, latents, noise, offset, duration, batch, out_size, output_file, audio_file, truncation,
                                       bends, rewrites, randomize_noise, ffmpeg_preset, shard, pipe_pix_fmt=pix_fmt, fold=fold, resize=resize,
                                       **effects)
    finally:
        if grouped and hasattr(generator, "random_noise"):
            generator.noise_seed = None  # the generator is cached across jobs
    dt = max(time.time() - t0, 1e-9)
    print(f"\nrendered {written} frames in {dt:.2f}s ({written / dt:.1f} frames/s)")
    print(f"total time taken: {(time.time() - started) / 60:.2f} minutes")
    return output_file


def _fold_of(args):
    """The temporal fold a namespace asks for (``subframes``, ``shutter``, ``shutter_light``: the CLI flags, a plugin's OVERRIDE or a
    caller's own ``args``): a render.TemporalFold, or None for one sub-frame — the plain render, whatever the other two say."""
    subframes = getattr(args, "subframes", None)
    if subframes is None or subframes == 1:
        return None
    return render.TemporalFold(subframes, getattr(args, "shutter", None) or "box", getattr(args, "shutter_light", None) or "encoded")


def _resize_of(args):
    """The delivery size a namespace asks for (``deliver_size``, ``deliver_filter``, ``deliver_fit``: the CLI flags, a plugin's OVERRIDE or
    a caller's own ``args``): a render.FrameResize, or None without a ``deliver_size`` — whatever the other two say."""
    size = getattr(args, "deliver_size", None)
    if not size:
        return None
    return render.FrameResize(size, getattr(args, "deliver_filter", None) or "lanczos", getattr(args, "deliver_fit", None) or "crop")


def _effect_of(args, name, **flag_kwargs):
    """The frame effect ``name`` (EFFECTS) a namespace asks for, or None.  ``args.<name>``: an instance of the effect's class, a callable
    ``<name>(args)`` that returns one or None (evaluated here: after initialize, so it may use what initialize computed), or a string
    as the flag takes it; ``args.<name>_spec``: the CLI flag, which builds a one-row effect (with ``flag_kwargs``: what further flags add
    to it).  The flag next to an effect of the namespace's own is refused: two effects do not compose into one row."""
    cls = next(c for n, c, _ in EFFECTS if n == name)
    kind, parse = f"ar.{cls.__name__}", getattr(ar, name).parse_spec
    effect, spec = getattr(args, name, None), getattr(args, f"{name}_spec", None)
    if isinstance(effect, str):
        effect = cls(**parse(effect))
    elif effect is not None and not isinstance(effect, cls):
        if not callable(effect):
            raise TypeError(f"args.{name} must be an {kind} or a callable {name}(args) -> {kind}, got {type(effect).__name__}")
        effect = effect(args)
        if effect is not None and not isinstance(effect, cls):
            raise TypeError(f"args.{name}(args) must return an {kind}, got {type(effect).__name__}")
    if effect is None:
        return cls(**parse(spec), **flag_kwargs) if spec else None
    if spec:
        raise ValueError(f"--{name} cannot be combined with the plugin's {name} (two of them do not compose into one row): set it in the plugin")
    return effect


def _grade_of(args):
    """The colour grade a namespace asks for, or None (_effect_of), and on top of it ``grade_lut`` / ``grade_lut_mix``, the LUT flags: they
    alone build a one-row grade, and --grade_lut is attached to a grade that has no LUT of its own; two LUTs are refused."""
    lut, mix = getattr(args, "grade_lut", None), getattr(args, "grade_lut_mix", None)
    mix = 1.0 if mix is None else mix
    grade = _effect_of(args, "grade", lut_mix=mix)
    if lut:
        if grade is not None and grade.lut is not None:  # (the plugin's: a grade built from --grade has none yet)
            raise ValueError("--grade_lut cannot be combined with a plugin grade that has a LUT of its own")
        grade = (ar.Grade(lut_mix=mix) if grade is None else grade).with_lut(lut, mix)
    return grade


def _lens_of(args):
    """The lens a namespace asks for, or None: ``args.lens`` / --lens (_effect_of)."""
    return _effect_of(args, "lens")


def _feedback_of(args):
    """The frame feedback a namespace asks for, or None: ``args.feedback`` / --feedback (_effect_of)."""
    return _effect_of(args, "feedback")


def _broadcast_effect(name, effect, lo, hi):
    """One process per GPU: rank 0's grade or lens reaches every rank — its ``tables()`` are broadcast whole (with them what belongs to the
    whole table: the LUT, the lens's ``plan_max``, so that every rank derives the reduction, the radii and the taps of a frame that the
    one-rank job derives), the effect is rebuilt and cut to this rank's frames [lo, hi); a one-row table is kept as it is."""
    rank, _ = sharding.rank_world()
    cls = next(c for n, c, _ in EFFECTS if n == name)
    whole = cls.from_tables(*sharding.broadcast_object(effect.tables() if rank == 0 else None))
    if whole.n_rows == 1:
        return whole
    if hi > whole.n_rows:
        raise RuntimeError(f"the {name}'s table has {whole.n_rows} rows, this rank renders the frames {lo} .. {hi}")
    return whole.slice(lo, hi) if hi > lo else whole.slice(0, 1)  # (a rank without frames: one row, never applied)


def _broadcast_grade(grade, lo, hi):
    return _broadcast_effect("grade", grade, lo, hi)


def _broadcast_lens(lens, lo, hi):
    return _broadcast_effect("lens", lens, lo, hi)


def _pipe_format_of(args):
    """The pipe format a namespace asks for (``pipe_pix_fmt``, ``mjpeg_quality``) as render takes it: the quality of an mjpeg pipe
    travels in the format's name, ``mjpeg:<quality>``."""
    pix_fmt, quality = getattr(args, "pipe_pix_fmt", None), getattr(args, "mjpeg_quality", None)
    return f"mjpeg:{quality}" if pix_fmt == "mjpeg" and quality is not None else pix_fmt


def _tail_options(args, fold, grade, lens, feedback):
    """(pipe_pix_fmt, fold, resize) of a job's render: what the namespace says, and for some jobs what the environment says where the
    namespace is silent ("Render tail": kept as it grew, route by route).  A job with a grade, a lens, a feedback or a
    --deliver_size reads the namespace alone.  Any other job takes its delivery size from $MAUA_DELIVER_SIZE..., and — unless the
    namespace sets a fold — its fold from $MAUA_SUBFRAMES... and, where the namespace says rgb24 (the flag's default), its pipe format
    from $MAUA_PIPE_PIX_FMT.  (A namespace without a ``pipe_pix_fmt`` is $MAUA_PIPE_PIX_FMT for every job: render resolves None.)"""
    pix_fmt, resize = _pipe_format_of(args), _resize_of(args)
    if resize is None and grade is None and lens is None and feedback is None:
        resize = render._resize_from_env()
        if fold is None:
            fold = render._fold_from_env()
            pix_fmt = None if pix_fmt == "rgb24" else pix_fmt
    return pix_fmt, fold, resize


def load_plugin(audioreactive_file):
    """Import a plugin file (path or dotted module) and pick out the optional callbacks and its ``OVERRIDE`` dict
    (reference :262-292: a missing callback falls back to the default, any other import error is fatal)."""
    if os.path.exists(audioreactive_file):
        spec = importlib.util.spec_from_file_location("maua_audioreactive_plugin", audioreactive_file)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    else:
        module = importlib.import_module(audioreactive_file.replace(".py", "").replace("/", "."))
    callbacks = {}
    for name in CALLBACK_NAMES:
        callbacks[name] = getattr(module, name, None)
        if callbacks[name] is None:
            print(f"No '{name}' function found in --audioreactive_file, using default...")
    return callbacks, dict(getattr(module, "OVERRIDE", {}))


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for flag, kwargs in CLI_FLAGS + DELIVERY_FLAGS + sum((flags for _, _, flags in EFFECTS), ()):
        parser.add_argument(flag, **kwargs)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    os.makedirs(args.output_dir, exist_ok=True)

    own_group = int(os.environ.get("WORLD_SIZE", "1")) > 1 and not th.distributed.is_initialized()
    if own_group:
        th.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        th.distributed.init_process_group("nccl")

    plugin_path = args.audioreactive_file
    if not os.path.exists(plugin_path) and plugin_path == build_parser().get_default("audioreactive_file"):
        plugin_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "audioreactive", "examples", "default.py")
    try:
        callbacks, override = load_plugin(plugin_path)
    except Exception:
        print("Error while loading --audioreactive_file...")
        traceback.print_exc()
        sys.exit(1)

    settings = vars(args).copy()
    for key, value in override.items():  # the plugin's OVERRIDE dict beats the command line
        settings[key] = value
        setattr(args, key, value)
    ckpt, audio_file = settings.pop("ckpt", None), settings.pop("audio_file", None)
    # (what stays in ``args``, where generate() reads it, and is not one of its parameters: the pipe format, the fold, the delivery size
    # and, per effect, ``args.<name>`` and the destinations of its flags)
    for key in ("pipe_pix_fmt", "mjpeg_quality", "subframes", "shutter", "shutter_light") + tuple(f.lstrip("-") for f, _ in DELIVERY_FLAGS):
        settings.pop(key, None)
    for name, _, flags in EFFECTS:
        for key in (name,) + tuple(kwargs.get("dest", flag.lstrip("-")) for flag, kwargs in flags):
            settings.pop(key, None)
    try:
        generate(ckpt=ckpt, audio_file=audio_file, **callbacks, **settings, args=args)
    finally:
        if own_group:
            th.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
