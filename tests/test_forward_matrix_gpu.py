"""Whole forwards of the generator on every dispatch route (tests/forward_ref.py holds the cases, the fp64 reference, the bounds and the
expected routes; tests/test_forward_routes_host.py proves on the host that the cases cover every path and every reachable mode).

Every case: (1) the route the host dispatch of models/stylegan2.py took, recorded layer by layer by a test-side wrapper, equals
forward_ref.expected_route; (2) every map the forward stored (a posted one against the reference map times the consumer's fp64 styles),
every intermediate image and the final image lie inside the per-element bounds 4 G max |fp32 - fp64| of the CPU references, no element
exempt; (3) the captured form of the forward, bound to the
case's 2 x batch frames and replayed at offsets 0 and batch, equals the eager forward bit for bit and records the same route.  The uint8
cases compare the frames of a forward captured with ``frames_u8`` with floor((clamp(fp64) + 1) 127.5): exact wherever the reference decides
the level, one level elsewhere.

The non-square cases (``orient`` "wide" / "tall") run the same assertions on generators built for 1920 / 1080 output behind the replicate
``ar.Pad`` on layer id 0 that widens the constant to 4 x 8 / 8 x 4: every layer then works on a 2:1 / 1:2 map and takes a route no square
generator takes (tests/test_forward_routes_host.py lists them), and the last layer's epilogue writes 2:1 / 1:2 frames."""
import contextlib

import pytest
import torch

from maua_stylegan2_amd import _lib

import forward_ref as fr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


# ---- the route recorder (test side only) ---------------------------------------------------------------------------------------------------
class Recorder:
    """Wraps StyledConv.run, Generator._run_const_conv, ToRGB.run and the library's maua_frames_to_u8 while active.  ``forwards``: one list
    of layer records per forward seen (a forward starts at conv1); ``keep_maps``: clone what every layer returned (eager forwards only)."""

    def __init__(self, keep_maps=False):
        self.keep_maps = keep_maps
        self.forwards = []

    def _layer(self, layer, tag, x_hw, rgb, src, prescaled, post_off, call):
        mode = layer.conv.conv_mode(*x_hw)
        if tag == "conv1":
            self.forwards.append([])
        offered = rgb is not None
        out = call()
        name = _lib.last_modconv_instance()
        rec = dict(tag=tag, mode=mode, prescaled=bool(prescaled), post_off=post_off, offered=offered, path=layer.last_path, posted=bool(layer.posted),
                   done=bool(offered and rgb.get("done")), u8_done=bool(offered and rgb.get("u8") is not None and rgb.get("done") and rgb.get("u8_done", True)),
                   stored=not offered or bool(rgb.get("store", True)), instance=name, separate=False, u8_pass=False, up=layer.conv.upsample,
                   out=out.clone() if self.keep_maps and src is None else None)
        self.forwards[-1].append(rec)
        return out

    def __enter__(self):
        from maua_stylegan2_amd.models import stylegan2 as sg

        rec = self
        self._lib = _lib.load()
        self._saved = (sg.StyledConv.run, sg.Generator._run_const_conv, sg.ToRGB.run, self._lib.maua_frames_to_u8)
        run, const_run, rgb_run, to_u8 = self._saved

        def styled_run(self, x, s, s_off, d, noise, bufs, tag, rgb=None, src=None, slot=0, prescaled=False, post_off=None):
            return rec._layer(self, tag, tuple(x.shape[2:]), rgb, src, prescaled, post_off,
                              lambda: run(self, x, s, s_off, d, noise, bufs, tag, rgb=rgb, src=src, slot=slot, prescaled=prescaled, post_off=post_off))

        def const_conv(self, s, s_off, d, noise, bufs, rgb, src, batch):
            return rec._layer(self.conv1, "conv1", tuple(self.input.input.shape[2:]), rgb, src, False, None,
                              lambda: const_run(self, s, s_off, d, noise, bufs, rgb, src, batch))

        def torgb_run(self, x, s, s_off, skip, out):
            if s is not None and rec.forwards:  # (s None: the plane sum behind a layer that left partial sums — part of that layer's path)
                rec.forwards[-1][-1]["separate"] = True
            return rgb_run(self, x, s, s_off, skip, out)

        def frames_to_u8(*args):
            if rec.forwards:
                rec.forwards[-1][-1]["u8_pass"] = True
            return to_u8(*args)

        sg.StyledConv.run, sg.Generator._run_const_conv, sg.ToRGB.run = styled_run, const_conv, torgb_run
        self._lib.maua_frames_to_u8 = frames_to_u8
        return self

    def __exit__(self, *exc):
        from maua_stylegan2_amd.models import stylegan2 as sg

        sg.StyledConv.run, sg.Generator._run_const_conv, sg.ToRGB.run, self._lib.maua_frames_to_u8 = self._saved
        return False

    @staticmethod
    def route(records):
        """{tag: forward_ref.Route} of one forward's records, and the checks a Route does not carry: the instance name agrees with mode, path
        and the pre-scaled flag, a posting layer was given a post_off, nobody writes the uint8 frame twice."""
        out = {}
        for i, r in enumerate(records):
            name = r["instance"]
            if r["path"] == "const":
                family = "const"  # (no modconv launch: the name is the previous call's)
            else:
                family = {"modconv_mfma": "mfma", "modconv_w2d": "w2d", "modconv_up2d": "up2d"}[name.split("_kernel")[0].replace("w2dw", "w2d")]
                args = [a.strip() for a in name[name.index("<") + 1: name.index(">")].split(",")]
                if family == "mfma":
                    assert int(args[3]) == r["mode"], (r["tag"], name, r["mode"])
                else:
                    assert ("true" in args) == r["prescaled"], (r["tag"], name, r["prescaled"])
                if family == "up2d":
                    assert args[1] == ("2" if r["path"] == "fused" else "0"), (r["tag"], name, r["path"])
            assert not r["posted"] or r["post_off"] is not None, r["tag"]
            assert not (r["u8_done"] and r["u8_pass"]), f"{r['tag']}: the uint8 frame was written by the epilogue AND by maua_frames_to_u8"
            rgb = None if r["up"] else ("folded" if r["path"] == "torgb" else "partial") if r["done"] else "separate" if r["separate"] else None
            u8 = "layer" if r["u8_done"] else "pass" if r["u8_pass"] else None
            assert i == len(records) - 1 or u8 is None, r["tag"]
            out[r["tag"]] = fr.Route(r["mode"], r["path"], r["prescaled"], r["posted"], rgb, u8, family)
        return out


def _short(route):
    return " ".join(f"{tag.replace('convs.', 'c')}:{r.mode}/{r.path}{'<' if r.prescaled else ''}{'>' if r.posted else ''}"
                    f"{'' if r.rgb is None else '+' + r.rgb}{'' if r.u8 is None else '+u8:' + r.u8}" for tag, r in route.items())


def _build(case, gpu):
    from maua_stylegan2_amd.models.stylegan2 import Generator

    inp = fr.inputs(case)
    g = Generator(case.size, 512, 8, channel_multiplier=case.cm, constant_input=case.constant_input, min_rgb_size=case.min_rgb_size,
                  output_size=case.output_size)
    g.load_state_dict(inp["sd"], strict=True)  # (a non-square case: the 2:1 noise buffers are part of the state dict)
    assert [tuple(getattr(g.noises, f"noise_{i}").shape[-2:]) for i in range(g.num_layers)] == fr.noise_shapes(case)
    g = g.to(gpu).eval()
    for attr, value in case.gen:
        setattr(g, attr, value)
    if inp["tl"] is not None:
        g.truncation_latent = inp["tl"].to(gpu)
    dev = dict(latents=inp["latents"].to(gpu), noise=[None if nz is None else nz.to(gpu) for nz in inp["noise"]],
               trunc=None if inp["trunc"] is None else inp["trunc"].to(gpu))
    return g, dev


def _eager(g, dev, case, first, bends):
    b = case.batch
    return g(styles=dev["latents"][first: first + b], noise=fr.frames(dev["noise"], first, b),
             truncation=1.0 if dev["trunc"] is None else dev["trunc"][first: first + b], randomize_noise=False, input_is_latent=True,
             return_activation_maps=case.acts, transform_dict_list=bends)


@pytest.mark.parametrize("case", fr.CASES, ids=lambda c: c.name)
def test_forward_route_and_fp64_parity(gpu, case):
    ref, bnd = fr.reference(case), fr.bounds(case)
    g, dev = _build(case, gpu)
    bends = fr.device_bends(case)
    b = case.batch
    worst = []  # (fraction of the bound, message)
    with contextlib.ExitStack() as stack:
        stack.enter_context(fr.switched(case))
        flags = fr.route_flags(case)
        want_eager = fr.expected_route(g, b, dict(flags, frames_u8=False))
        with Recorder(keep_maps=True) as rec:
            image, acts = _eager(g, dev, case, 0, bends)
        assert len(rec.forwards) == 1
        records = rec.forwards[0]
        got = Recorder.route(records)
        print(f"\n[{case.name}] route: {_short(got)}")
        print(f"[{case.name}] instances: " + "; ".join(f"{r['tag']} {r['instance']}" for r in records if r["path"] != "const"))
        assert got == want_eager, {t: (got.get(t), want_eager[t]) for t in want_eager if got.get(t) != want_eager[t]}
        # (2) every stored map, every intermediate image, the image
        for i, r in enumerate(records):
            if r["posted"]:  # the stored map carries the consumer's styles
                worst.append(fr.check(f"{r['tag']} posted map (mode {r['mode']}, {r['path']})", r["out"], fr.posted_map(ref, i), bnd["posted"][i]))
            elif r["stored"]:
                worst.append(fr.check(f"{r['tag']} map (mode {r['mode']}, {r['path']})", r["out"], ref["raw"][i], bnd["raw"][i]))
        if case.acts:
            assert len(acts) == len(ref["acts"])
            assert not any(r["posted"] or r["prescaled"] for r in records) and records[-1]["stored"]
            for i, a in enumerate(acts):
                worst.append(fr.check(f"returned activation map {i}", a, ref["acts"][i], bnd["acts"][i]))
        for n, want in enumerate(ref["images"]):
            if want is not None and case.min_rgb_size <= 4 * 2 ** n:
                buf = g._bufs[(b, "rgb1" if n == 0 else f"rgbs.{n - 1}", 0)]
                side = f"{4 * 2 ** n}^2" if case.orient == "square" else f"{want.shape[2]} x {want.shape[3]}"
                worst.append(fr.check(f"image after {side}", buf, want, bnd["images"][n]))
        if ref["image"] is None:
            assert image is None
        else:
            worst.append(fr.check("image", image, ref["image"], bnd["image"]))
        del rec, records
        for frac, msg in worst:
            print(f"[{case.name}] {msg}")
        top = max(worst)
        print(f"[{case.name}] worst: {top[1]}; without G (4 x the fp32 CPU forward's own error) that is {top[0] * fr.winograd_gain(case.orient):.2f} of the bound")
        assert all(frac <= 1.0 for frac, _ in worst), [msg for frac, msg in worst if frac > 1.0]
        # (3) the captured form
        if not case.capturable:
            return
        second = _eager(g, dev, case, b, bends)[0]
        second = None if second is None else second.clone()
        want_graph = fr.expected_route(g, b, flags)
        g.tap_float_image = bool(case.u8)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            with Recorder() as rec:
                lane = g.capture_graph(b, bends=bends, frames_u8=case.u8 is not None)
            assert len(rec.forwards) == 2  # the warm-up and the captured forward
            for records in rec.forwards:
                got = Recorder.route(records)
                assert got == want_graph, {t: (got.get(t), want_graph[t]) for t in want_graph if got.get(t) != want_graph[t]}
            if case.u8 is not None:
                print(f"[{case.name}] captured route: {_short(got)}")
            lane.bind(dev["latents"], dev["noise"], dev["trunc"])
            for first, eager in ((0, image), (b, second)):
                lane.replay(first)
                stream.synchronize()
                if case.u8 is None:
                    assert (lane.image is None and eager is None) or torch.equal(lane.image, eager), f"replay at {first} != eager"
                    continue
                last = want_graph[f"convs.{g.num_layers - 2}"]
                frames = lane.u8.cpu()
                assert tuple(frames.shape) == (b,) + tuple(ref["image"].shape[2:]) + (3,)  # (rows x columns of the padded generator)
                cast = lambda img: ((img.clamp(-1, 1) + 1) * 127.5).permute(0, 2, 3, 1).to(torch.uint8).cpu()  # noqa: E731
                assert int((frames.int() - cast(eager).int()).abs().max()) <= 1  # (the eager forward has no uint8 form: another instance)
                if last.u8 == "layer" and not case.u8:
                    assert lane.image is None
                else:
                    assert torch.equal(frames, cast(lane.image)), "frame != cast of the float image of the same forward"
                    if last.u8 == "pass":  # the same kernels as the eager forward, + maua_frames_to_u8
                        assert torch.equal(lane.image, eager), f"replay at {first} != eager"
                    if first == 0:
                        frac, msg = fr.check("tapped image", lane.image, ref["image"], bnd["image"])
                        print(f"[{case.name}] {msg}")
                        assert frac <= 1.0, msg
                if first == 0:
                    levels, ambiguous = fr.frames_u8_reference(ref["image"], bnd["image"])
                    diff = (frames.int() - levels.int()).abs()
                    share = float(ambiguous.float().mean())
                    print(f"[{case.name}] frames: {int((diff > 0).sum())} of {diff.numel()} values off by one level, "
                          f"{int((diff[~ambiguous] > 0).sum())} of them where the reference decides; ambiguous share {100 * share:.2f} %")
                    assert int(diff[~ambiguous].max()) == 0 and int(diff.max()) <= 1
            lane.release()
