"""Retake without a GPU: the window arithmetic on cases worked by hand (restatement and TemporalRegionMask agree), apply_to against the
token ranges, the configuration record, the source-clip rules, the restatement's integer composite, generate_video's routing and the ABI
declarations."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import retake_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
NEW_ENTRIES = ("ltx2_retake_prepare", "ltx2_retake_composite")

# fps, latent frames, (start, end) in seconds, [f0, f1) worked by hand (None: the window touches nothing)
WINDOWS = [
    (24, 5, (0.0, 1.0), (0, 3)),        # sp = 0: (-1)//8 = -1, clamped to 0; ep = 24: 23//8 + 1 = 3
    (24, 5, (0.5, 1.0), (1, 3)),        # sp = 12: 11//8 = 1
    (24, 5, (1.0, 1.02), (2, 3)),       # sp = ep = 24: 23//8 = 2 and 2 + 1
    (24, 5, (5.0, 6.0), None),          # sp = 120: 14; ep = 144 -> min(5, 18) = 5: f0 >= f1
    (25, 4, (0.04, 10.0), (0, 4)),      # sp = 1: 0//8 = 0; ep = 250 -> min(4, 32)
]


@pytest.mark.parametrize("fps,frames,times,want", WINDOWS)
def test_frame_window_by_hand(fps, frames, times, want):
    from ltx_2_mlx_amd.pipelines import TemporalRegionMask
    ref = RR.frame_window(*times, fps, frames)
    got = TemporalRegionMask(*times, fps).frame_window(frames)
    assert got == ref
    if want is None:
        assert got[0] >= got[1]
    else:
        assert got == want


def test_pixel_window():
    from ltx_2_mlx_amd.pipelines import TemporalRegionMask
    # latent frame 0 is pixel frame 0, latent frame k >= 1 the pixel frames 8(k-1)+1 .. 8k
    assert RR.pixel_window((0, 1), 17) == (0, 1) and RR.pixel_window((1, 2), 17) == (1, 9) and RR.pixel_window((2, 3), 17) == (9, 17)
    assert RR.pixel_window((0, 3), 17) == (0, 17) and RR.pixel_window((1, 3), 17) == (1, 17) and RR.pixel_window((3, 3), 17) == (0, 0)
    for fps, frames, times, want in WINDOWS:
        pix = 8 * (frames - 1) + 1
        m = TemporalRegionMask(*times, fps)
        assert m.pixel_window(frames, pix) == RR.pixel_window(RR.frame_window(*times, fps, frames), pix), (fps, frames, times)
    assert TemporalRegionMask(0.4, 0.7, 24).frame_window(3) == (1, 2) and TemporalRegionMask(0.4, 0.7, 24).pixel_window(3, 17) == (1, 9)


def test_apply_to_sets_the_token_ranges():
    from ltx_2_mlx_amd.components import VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning.tools import VideoLatentTools
    from ltx_2_mlx_amd.pipelines import TemporalRegionMask
    from ltx_2_mlx_amd.types import VideoLatentShape
    tools = VideoLatentTools(patchifier=VideoLatentPatchifier(patch_size=1), target_shape=VideoLatentShape(1, 128, 5, 2, 3), fps=24.0)
    g = torch.Generator().manual_seed(1)
    enc = torch.randn(1, 128, 5, 2, 3, generator=g)
    state = tools.create_initial_state(dtype=torch.float32, initial_latent=enc)
    assert bool((state.denoise_mask == 1).all())
    for fps, frames, times, want in WINDOWS[:4]:
        out = TemporalRegionMask(*times, fps).apply_to(state, tools)
        m = out.denoise_mask
        assert m.shape == (1, 30, 1) and m.dtype == state.denoise_mask.dtype
        f0, f1 = want or (0, 0)
        assert bool((m[0, f0 * 6: f1 * 6] == 1).all()) and float(m.sum()) == (f1 - f0) * 6
        assert out.latent is state.latent and out.clean_latent is state.clean_latent and out.positions is state.positions
        # the restatement's prepare builds the same mask and the same clean tokens
        if want:
            clean, rm, _ = RR.prepare(enc, want, torch.zeros(1, 30, 128))
            assert torch.equal(rm, m) and torch.equal(clean, state.clean_latent)


def test_restatement_prepare_blend():
    g = torch.Generator().manual_seed(2)
    enc, noise = torch.randn(1, 128, 3, 2, 3, generator=g), torch.randn(1, 18, 128, generator=g)
    clean, mask, lat = RR.prepare(enc, (1, 2), noise, 1.0)
    assert torch.equal(lat[:, :6], clean[:, :6]) and torch.equal(lat[:, 12:], clean[:, 12:]) and torch.equal(lat[:, 6:12], noise[:, 6:12])
    assert torch.equal(clean[0, 7], enc[0, :, 1, 0, 1])
    _, _, half = RR.prepare(enc, (1, 2), noise, 0.5)
    assert torch.equal(half[:, 6:12], noise[:, 6:12] * 0.5 + clean[:, 6:12] * 0.5) and torch.equal(half[:, :6], clean[:, :6])


def test_config_defaults_and_validation():
    from ltx_2_mlx_amd.pipelines import RetakeConfig
    c = RetakeConfig(start_time=1.0, end_time=2.0)
    assert (c.regenerate_video, c.regenerate_audio, c.distilled, c.num_inference_steps, c.cfg_scale, c.seed, c.tiling_config) == \
        (True, True, False, 40, 3.0, 42, None)
    assert (c.fps, c.use_hip_graph, c.composite_source, c.composite_ramp) == (None, True, False, 4)
    for s, e in ((2.0, 2.0), (3.0, 1.0)):
        with pytest.raises(ValueError, match=r"start_time \(.*\) must be < end_time"):
            RetakeConfig(start_time=s, end_time=e)
    assert "no effect" in RetakeConfig.__doc__ and "regenerate_audio" in RetakeConfig.__doc__


class _NoEncoder:
    device = torch.device("cpu")

    def encode_patches(self, x):
        raise AssertionError("the encoder must not be reached")


def test_source_rules(tmp_path):
    """Arrays and directories need config.fps; the size must be divisible by 32 (named in the message); an empty window names the clip's
    duration -- all before the encoder runs."""
    from ltx_2_mlx_amd.pipelines import RetakeConfig, RetakePipeline, get_video_metadata, load_video_frames
    rng = np.random.default_rng(4)
    good = tmp_path / "clip.npy"
    np.save(good, rng.integers(0, 256, (20, 64, 96, 3), dtype=np.uint8))
    odd = tmp_path / "odd.npy"
    np.save(odd, np.zeros((9, 48, 100, 3), np.uint8))
    pipe = RetakePipeline.__new__(RetakePipeline)
    pipe.video_encoder = _NoEncoder()
    ctx = torch.zeros(1, 4, 128)
    with pytest.raises(ValueError, match="RetakeConfig.fps"):
        get_video_metadata(str(good))
    assert get_video_metadata(str(good), 24) == (24.0, 20, 96, 64)
    with pytest.raises(ValueError, match="RetakeConfig.fps"):
        pipe.denoise_latent(str(good), ctx, RetakeConfig(0.0, 1.0))
    with pytest.raises(ValueError, match="RetakeConfig.fps"):
        pipe.denoise_latent(None, ctx, RetakeConfig(0.0, 1.0), frames=np.zeros((9, 64, 96, 3), np.uint8))
    with pytest.raises(ValueError, match=r"100x48.*divisible by 32"):
        pipe.denoise_latent(str(odd), ctx, RetakeConfig(0.0, 1.0, fps=24))
    with pytest.raises(FileNotFoundError):
        pipe.denoise_latent(str(tmp_path / "missing.npy"), ctx, RetakeConfig(0.0, 1.0, fps=24))
    with pytest.raises(ValueError, match="uint8"):
        pipe.denoise_latent(None, ctx, RetakeConfig(0.0, 1.0, fps=24), frames=np.zeros((9, 64, 96, 3), np.float32))
    # 20 frames are snapped down to 17 and sent to the encoder's device as they are
    src, fps = pipe._load_source(str(good), None, RetakeConfig(0.0, 1.0, fps=24))
    assert src.dtype == torch.uint8 and src.shape == (17, 64, 96, 3) and fps == 24.0 and np.array_equal(src.numpy(), np.load(good)[:17])
    v = load_video_frames(str(good), 64, 96, 17)
    assert v.shape == (1, 3, 17, 64, 96) and float(v.min()) >= -1 and float(v.max()) <= 1
    # a directory of image frames
    from PIL import Image
    d = tmp_path / "frames"
    d.mkdir()
    for i in range(9):
        Image.fromarray(np.load(good)[i]).save(d / f"f{i:03d}.png")
    assert get_video_metadata(str(d), 25) == (25.0, 9, 96, 64)
    src, _ = pipe._load_source(str(d), None, RetakeConfig(0.0, 1.0, fps=25))
    assert np.array_equal(src.numpy(), np.load(good)[:9])


def test_empty_window_raises_with_the_duration(monkeypatch):
    """Checked after the encoder in the pipeline (the window needs the latent shape), so a stub encoder stands in for it here."""
    import ltx_2_mlx_amd.pipelines.retake as R
    from ltx_2_mlx_amd.pipelines import RetakeConfig, RetakePipeline

    class Enc:
        device = torch.device("cpu")

        def encode_patches(self, x):
            return torch.zeros(1, 128, 3, 2, 3)

    pipe = RetakePipeline.__new__(RetakePipeline)
    pipe.video_encoder = Enc()
    monkeypatch.setattr(R.K, "frames_to_patches", lambda x: x)
    with pytest.raises(ValueError, match=r"touches no frame.*17 frames at 24 fps, 0\.708 s"):
        pipe.denoise_latent(None, torch.zeros(1, 4, 128), RetakeConfig(5.0, 6.0, fps=24), frames=np.zeros((17, 64, 96, 3), np.uint8))


def test_restatement_composite():
    rng = np.random.default_rng(8)
    dec = rng.integers(0, 256, (17, 4, 5, 3), dtype=np.uint8)
    src = rng.integers(0, 256, (17, 4, 5, 3), dtype=np.uint8)
    # ramp 0: the source's bytes outside, decoded inside
    for p0, p1 in ((0, 9), (1, 9), (0, 1), (9, 17), (16, 17), (0, 17), (5, 5)):
        out = RR.composite(dec, src, p0, p1, 0)
        assert np.array_equal(out[p0:p1], dec[p0:p1]) and np.array_equal(out[:p0], src[:p0]) and np.array_equal(out[p1:], src[p1:])
    # ramp 3: weights fall by one per frame of distance, monotone on each side, 4/4 inside
    a = RR.composite_weights(17, 6, 9, 3)
    assert a.tolist() == [0, 0, 0, 1, 2, 3, 4, 4, 4, 3, 2, 1, 0, 0, 0, 0, 0]
    assert all(a[i] <= a[i + 1] for i in range(6)) and all(a[i] >= a[i + 1] for i in range(8, 16))
    # exact values on constant frames: decoded 255 over source 0 gives (255 a + 2) // 4, and the other way round
    hi, lo = np.full((17, 2, 2, 3), 255, np.uint8), np.zeros((17, 2, 2, 3), np.uint8)
    up = RR.composite(hi, lo, 6, 9, 3)[:, 0, 0, 0].tolist()
    assert up == [0, 0, 0, 64, 128, 191, 255, 255, 255, 191, 128, 64, 0, 0, 0, 0, 0]
    down = RR.composite(lo, hi, 6, 9, 3)[:, 0, 0, 0].tolist()
    assert down == [255, 255, 255, 191, 128, 64, 0, 0, 0, 64, 128, 191, 255, 255, 255, 255, 255]
    assert np.array_equal(RR.composite(hi, hi, 6, 9, 3), hi) and np.array_equal(RR.composite(lo, lo, 6, 9, 3), lo)
    # a ramp longer than the clip never reaches the source's own bytes
    assert RR.composite_weights(17, 16, 17, 40).min() == 41 - 16


def test_generate_video_routes_retake(monkeypatch, tmp_path):
    import generate as gen

    class Routed(Exception):
        pass

    def spy(name):
        def f(*a, **k):
            raise Routed(name, a, k)
        return f

    for name in ("load_transformer", "load_av_transformer", "create_vae_decoder", "create_dummy_text_encoding", "encode_with_gemma"):
        monkeypatch.setattr(gen, name, spy(name))
    clip = str(tmp_path / "c.npy")
    np.save(clip, np.zeros((20, 64, 96, 3), np.uint8))
    kw = dict(use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"), retake_video=clip, retake_start_time=0.4, retake_end_time=0.7)
    # refused by name, before any model loads and before the GPU is touched
    for extra in (dict(generate_audio=True), dict(audio_path="a.wav"), dict(keyframes=["k.png:0"]), dict(control_video="c.npy"),
                  dict(two_stage_distilled=True), dict(upscale_spatial=True), dict(upscale_temporal=True), dict(fp8_resident=True)):
        with pytest.raises(NotImplementedError, match=f"{list(extra)[0]} with retake_video"):
            gen.generate_video("p", **kw, **extra)
    with pytest.raises(ValueError, match="touches no frame"):
        gen.generate_video("p", **{**kw, "retake_start_time": 5.0, "retake_end_time": 6.0})
    with pytest.raises(ValueError, match="must be < end_time"):
        gen.generate_video("p", **{**kw, "retake_start_time": 0.7, "retake_end_time": 0.4})
    with pytest.raises(FileNotFoundError):
        gen.generate_video("p", **{**kw, "retake_video": str(tmp_path / "missing.npy")})
    odd = str(tmp_path / "odd.npy")
    np.save(odd, np.zeros((9, 48, 100, 3), np.uint8))
    with pytest.raises(ValueError, match=r"100x48.*divisible by 32"):
        gen.generate_video("p", **{**kw, "retake_video": odd})
    # two more the route cannot honour: an image conditioning and another pipeline
    img = str(tmp_path / "i.png")
    open(img, "wb").close()
    with pytest.raises(NotImplementedError, match="image_path with retake_video"):
        gen.generate_video("p", **kw, image_path=img)
    for pt in ("distilled", "one-stage", "ic-lora", "keyframe-interpolation", "ti2vid-hq"):
        with pytest.raises(NotImplementedError, match="pipeline_type with retake_video"):
            gen.generate_video("p", **kw, pipeline_type=pt)
    # everything in order: the first loader is reached, also with the end of the window left to the clip's
    for extra in ({}, dict(retake_end_time=None), dict(retake_composite=True, model_variant="dev", cfg_scale=3.0)):
        with pytest.raises(Routed) as e:
            gen.generate_video("p", **{**kw, **extra})
        assert e.value.args[0] == "create_dummy_text_encoding"
    # the command line reaches it
    a = gen.build_parser().parse_args(["a prompt", "--retake", clip, "--retake-start", "0.4", "--retake-end", "0.7", "--retake-keep-source"])
    k = gen.kwargs_from_args(a)
    assert (k["retake_video"], k["retake_start_time"], k["retake_end_time"], k["retake_composite"]) == (clip, 0.4, 0.7, True)
    k = gen.kwargs_from_args(gen.build_parser().parse_args(["p"]))
    assert (k["retake_video"], k["retake_start_time"], k["retake_end_time"], k["retake_composite"]) == (None, 0.0, None, False)
    sig = inspect.signature(gen.generate_video).parameters
    assert all(sig[n].kind == inspect.Parameter.KEYWORD_ONLY for n in ("retake_video", "retake_start_time", "retake_end_time", "retake_composite"))
    assert list(sig)[-4:] == ["retake_video", "retake_start_time", "retake_end_time", "retake_composite"]


# fps, pixel frames (8k + 1): lengths at which n / fps * fps truncates to n - 1 in floating point, and some at which it does not
CLIP_ENDS = [(25, 57), (25, 113), (25, 201), (50, 57), (50, 201), (29.97, 241), (23.976, 97), (23.976, 113), (23.976, 217), (23.976, 417),
             (24, 17), (24, 97), (30, 121), (12, 9), (60, 1)]


def test_default_end_reaches_the_last_latent_frame(monkeypatch, tmp_path):
    """retake_end_time=None means "to the end of the clip": the window's f1 must be F for every length and rate, which num_frames / fps as
    the end does not give (int(57 / 25 * 25) is 56); through generate_video too, for 57 frames at 25 fps."""
    import generate as gen
    import ltx_2_mlx_amd.pipelines as P
    assert int(57 / 25 * 25) == 56 and P.TemporalRegionMask(0.0, 57 / 25, 25).frame_window(8) == (0, 7)       # what the default must not be
    for fps, n in CLIP_ENDS:
        latent = (n - 1) // 8 + 1
        end = P.end_of_clip(n, fps)
        assert int(end * fps) == n, (fps, n)
        assert P.TemporalRegionMask(0.0, end, fps).frame_window(latent) == RR.frame_window(0.0, end, fps, latent) == (0, latent), (fps, n)
        assert P.TemporalRegionMask(0.0, end, fps).pixel_window(latent, n) == (0, n)
    seen = []

    class Spy(P.TemporalRegionMask):
        def frame_window(self, latent_frames):
            seen.append((self.start_time, self.fps, latent_frames, super().frame_window(latent_frames)))
            return seen[-1][-1]

    class Routed(Exception):
        pass

    def stop(*a, **k):
        raise Routed()

    monkeypatch.setattr(P, "TemporalRegionMask", Spy)
    monkeypatch.setattr(gen, "create_dummy_text_encoding", stop)
    for fps, n in ((25, 57), (25, 60), (24, 17)):                               # 60 frames are snapped to 57
        clip = str(tmp_path / f"c{fps}_{n}.npy")
        np.save(clip, np.zeros((n, 32, 32, 3), np.uint8))
        with pytest.raises(Routed):
            gen.generate_video("p", use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"), retake_video=clip, retake_start_time=0.5,
                               output_fps=fps)
        latent = (((n - 1) // 8) * 8) // 8 + 1
        assert seen[-1][1:3] == (float(fps), latent) and seen[-1][3][1] == latent, seen[-1]


def test_retake_output_is_written_at_the_source_rate():
    """The frames of a retake enter ffmpeg at the source's rate and none is interpolated, whatever that rate is; every other route keeps
    the native 24 fps input."""
    import generate as gen
    for rate, text in ((30.0, "30"), (12.0, "12"), (24.0, "24"), (29.97, "29.97")):
        cmd = gen.ffmpeg_command(96, 64, "o.mp4", fps=rate, input_fps=rate)
        assert cmd[cmd.index("-framerate") + 1] == text and "-vf" not in cmd, cmd
    assert gen.video_filters(30.0, 1.0, 30.0) == [] and gen.video_filters(30.0, 2.0, 30.0) == ["setpts=0.5*PTS"]
    cmd = gen.ffmpeg_command(96, 64, "o.mp4", fps=48)
    assert cmd[cmd.index("-framerate") + 1] == "24" and any("minterpolate=fps=48" in c for c in cmd)
    assert inspect.signature(gen.save_video).parameters["input_fps"].default == gen.NATIVE_FPS


def test_abi_declares_the_retake_entries():
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    for name in NEW_ENTRIES:
        assert name in nv.SIGNATURES and name in nv.exported_symbols() and nv.SIGNATURES[name][0] is nv.i32, name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == len(nv.SIGNATURES[name][1]), name
    assert nv.RETAKE_MAX_RAMP == int(re.search(r"#define\s+LTX2_RETAKE_MAX_RAMP\s+(\d+)", header).group(1))
    assert 255 * (nv.RETAKE_MAX_RAMP + 1) + (nv.RETAKE_MAX_RAMP + 1) // 2 < 2 ** 32          # the composite's 32-bit numerator
    assert callable(K.retake_prepare) and callable(K.retake_composite)
    import ltx_2_mlx_amd.pipelines as P
    for name in ("RetakeConfig", "TemporalRegionMask", "RetakePipeline", "get_video_metadata", "load_video_frames", "create_retake_pipeline",
                 "end_of_clip"):
        assert hasattr(P, name) and name in P.__all__, name
