"""IC-LoRA without a GPU: the Canny restatement's two hysteresis formulations, the configuration records, the control-video loader, the
conditioning against the vectors recorded from the reference, generate_video's routing and the ABI declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import canny_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
NEW_ENTRIES = ("ltx2_canny_u8", "ltx2_canny_hysteresis", "ltx2_frames_to_patches")


# ------------------------------------------------------------------ the restatement
def test_hysteresis_formulations_agree():
    """Flood fill from the strong pixels == connected components that hold a strong pixel, on random maps of several densities and on the
    serpentine; a map without a strong pixel gives nothing."""
    rng = np.random.default_rng(5)
    for h, w, p_weak, p_strong in ((1, 1, 0.5, 0.5), (7, 9, 0.5, 0.05), (40, 53, 0.45, 0.004), (40, 53, 0.3, 0.02), (64, 64, 0.6, 0.001)):
        for _ in range(4):
            u = rng.random((h, w))
            m = np.where(u < p_strong, 2, np.where(u < p_strong + p_weak, 1, 0)).astype(np.uint8)
            a, b = CR.hysteresis_flood(m), CR.hysteresis_label(m)
            assert np.array_equal(a, b) and set(np.unique(a)) <= {0, 255}
            assert np.array_equal(a[m == 2], np.full((m == 2).sum(), 255)) and not a[m == 0].any()
    m, start = CR.serpentine(13, 11)
    assert not CR.hysteresis_flood(m).any() and not CR.hysteresis_label(m).any()
    m[start] = 2
    want = (m != 0) * np.uint8(255)
    assert np.array_equal(CR.hysteresis_flood(m), want) and np.array_equal(CR.hysteresis_label(m), want)
    # a diagonal-only connection counts (8-connectivity)
    d = np.zeros((4, 4), np.uint8)
    d[1, 1], d[2, 2] = 2, 1
    assert CR.hysteresis_label(d)[2, 2] == 255 and CR.hysteresis_flood(d)[2, 2] == 255


def test_canny_restatement_properties():
    rng = np.random.default_rng(6)
    flat = np.full((1, 9, 12, 3), 77, np.uint8)
    assert not CR.canny(flat, 0, 0).any()                                    # no gradient, mag = 0 is not > 0
    img = rng.integers(0, 256, (2, 21, 30, 3), dtype=np.uint8)
    assert np.array_equal(CR.canny(img, 100, 200), CR.canny(img, 200, 100))     # swapped thresholds
    assert np.array_equal(CR.canny(img, 50.7, 120.2), CR.canny(img, 50, 120))   # floored thresholds
    assert CR.thresholds(200, 100) == (100, 200) and CR.thresholds(50.7, 120.2) == (50, 120)
    # a vertical step edge: gray 0 | 255 gives one column of strong pixels on the bright side of the step (mag > left && mag >= right)
    step = np.zeros((1, 8, 10, 3), np.uint8)
    step[:, :, 5:] = 255
    e = CR.canny(step, 100, 200)[0]
    assert (e[:, 4] == 255).all() and not e[:, :4].any() and not e[:, 5:].any()
    assert CR.gray(np.array([[[255, 255, 255]]], np.uint8))[0, 0] == 255 and CR.gray(np.array([[[255, 0, 0]]], np.uint8))[0, 0] == 76


# ------------------------------------------------------------------ config
def test_config_defaults_and_validation():
    from ltx_2_mlx_amd.pipelines import ControlType, ICLoraConfig, VideoCondition
    with pytest.raises(ValueError, match="must be divisible by 64"):
        ICLoraConfig()                                                       # the reference's own default 480x704 fails its check
    c = ICLoraConfig(height=512, width=768)
    assert (c.height, c.width, c.num_frames, c.stage_1_steps, c.stage_2_steps, c.seed, c.fps, c.tiling_config, c.dtype) == \
        (512, 768, 97, 7, 3, 42, 24.0, None, torch.float32)
    with pytest.raises(ValueError, match=r"num_frames must be 8\*k \+ 1, got 96"):
        ICLoraConfig(height=512, width=768, num_frames=96)
    with pytest.raises(ValueError, match="must be divisible by 64"):
        ICLoraConfig(height=512, width=736)
    v = VideoCondition("c.mp4")
    assert (v.video_path, v.strength, v.control_type, v.canny_low, v.canny_high, v.save_control) == ("c.mp4", 0.95, ControlType.RAW, 100, 200, False)
    assert [t.value for t in ControlType] == ["canny", "raw"] and ControlType("canny") is ControlType.CANNY
    with pytest.raises(ValueError):
        ControlType("depth")


def test_pipeline_requires_upscaler_and_one_adapter():
    from ltx_2_mlx_amd.loader.lora_loader import LoRAConfig
    from ltx_2_mlx_amd.pipelines import ICLoraConfig, ICLoraPipeline

    class M:
        model_type = None
        device = "cpu"

    class X0:
        velocity_model = M()

    conf = ICLoraConfig(height=64, width=128, num_frames=9)
    pipe = ICLoraPipeline.__new__(ICLoraPipeline)
    pipe.transformer, pipe._velocity_model, pipe.spatial_upscaler, pipe.lora_configs = X0(), M(), None, []
    with pytest.raises(ValueError, match="requires spatial_upscaler"):
        pipe.denoise_latent(torch.zeros(1, 4, 8), conf)
    # one adapter at a time: refused before anything is loaded or encoded (video_encoder is not even set here)
    pipe.spatial_upscaler = object()
    pipe.lora_configs = [LoRAConfig("a.safetensors", 1.0), LoRAConfig("b.safetensors", 0.5)]
    with pytest.raises(NotImplementedError, match="more than one IC-LoRA"):
        pipe.denoise_latent(torch.zeros(1, 4, 8), conf)
    with pytest.raises(NotImplementedError, match="more than one IC-LoRA"):
        pipe.stage1_latent(torch.zeros(1, 4, 8), conf)


# ------------------------------------------------------------------ the loader
def test_load_control_frames(tmp_path, monkeypatch):
    from PIL import Image
    from ltx_2_mlx_amd.pipelines import ic_lora as IC
    rng = np.random.default_rng(7)
    clip = rng.integers(0, 256, (5, 16, 24, 3), dtype=np.uint8)
    np.save(tmp_path / "c.npy", clip)
    np.savez(tmp_path / "c.npz", frames=clip)
    for name in ("c.npy", "c.npz"):
        got = IC.load_control_frames(str(tmp_path / name), 16, 24, 9)
        assert got.dtype == np.uint8 and got.shape == (9, 16, 24, 3) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got[:5], clip) and all(np.array_equal(got[i], clip[4]) for i in range(5, 9))      # padded with the last frame
    assert np.array_equal(IC.load_control_frames(str(tmp_path / "c.npy"), 16, 24, 3), clip[:3])                # a long clip is cut
    gray = clip[..., 0]
    np.save(tmp_path / "g.npy", gray)
    assert np.array_equal(IC.load_control_frames(str(tmp_path / "g.npy"), 16, 24, 5), np.repeat(gray[..., None], 3, -1))
    # another size: the plain PIL LANCZOS resize, frame by frame
    got = IC.load_control_frames(str(tmp_path / "c.npy"), 8, 16, 5)
    want = np.stack([np.array(Image.fromarray(f).resize((16, 8), Image.Resampling.LANCZOS)) for f in clip])
    assert got.shape == (5, 8, 16, 3) and np.array_equal(got, want)
    # a directory of PNG frames, sorted by name (written out of order)
    d = tmp_path / "frames"
    d.mkdir()
    for i in (2, 0, 1):
        Image.fromarray(clip[i]).save(d / f"f_{i:03d}.png")
    (d / "notes.txt").write_text("not a frame")
    got = IC.load_control_frames(str(d), 16, 24, 5)
    assert np.array_equal(got[:3], clip[:3]) and np.array_equal(got[3], clip[2]) and np.array_equal(got[4], clip[2])
    # errors
    with pytest.raises(FileNotFoundError, match="Control video not found"):
        IC.load_control_frames(str(tmp_path / "missing.npy"), 16, 24, 5)
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="Could not read any frames"):
        IC.load_control_frames(str(tmp_path / "empty"), 16, 24, 5)
    np.save(tmp_path / "f.npy", clip.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        IC.load_control_frames(str(tmp_path / "f.npy"), 16, 24, 5)
    (tmp_path / "v.mp4").write_bytes(b"\x00" * 16)
    monkeypatch.setattr(IC.shutil, "which", lambda name: None)
    with pytest.raises(RuntimeError, match=r"ffmpeg binary.*\.npy / \.npz.*directory of image frames"):
        IC.load_control_frames(str(tmp_path / "v.mp4"), 16, 24, 5)
    # a video file with an ffmpeg binary: one run, frames piped out as PPM images that carry their own decoded size
    ppm = lambda f: b"P6\n%d %d\n255\n" % (f.shape[1], f.shape[0]) + f.tobytes()
    assert np.array_equal(IC._ppm_frames(b"".join(ppm(f) for f in clip)), clip)
    assert np.array_equal(IC._ppm_frames(b"".join(ppm(f) for f in clip) + ppm(clip[0])[:-5]), clip)          # a cut-off last image is dropped
    for bad in (b"", b"P5\n2 2\n255\n0000", ppm(clip[0]) + ppm(clip[0][:8])):
        with pytest.raises(ValueError):
            IC._ppm_frames(bad)
    runs = []

    class Done:
        def __init__(self, rc, out, err=b""):
            self.returncode, self.stdout, self.stderr = rc, out, err

    def fake_run(cmd, **kw):
        runs.append(cmd)
        return Done(0, b"".join(ppm(f) for f in clip[:int(cmd[cmd.index("-frames:v") + 1])]))

    monkeypatch.setattr(IC.shutil, "which", lambda name: "/usr/bin/ffmpeg")
    monkeypatch.setattr(IC.subprocess, "run", fake_run)
    got = IC.load_control_frames(str(tmp_path / "v.mp4"), 16, 24, 3)
    assert np.array_equal(got, clip[:3]) and len(runs) == 1 and runs[0][0] == "ffmpeg" and str(tmp_path / "v.mp4") in runs[0]
    assert "scale" not in " ".join(runs[0])                                                                  # the resize stays PIL's
    assert np.array_equal(IC.load_control_frames(str(tmp_path / "v.mp4"), 8, 16, 5), want)
    monkeypatch.setattr(IC.subprocess, "run", lambda cmd, **kw: Done(1, b"", b"moov atom not found"))
    with pytest.raises(ValueError, match="Could not read any frames.*moov atom"):
        IC.load_control_frames(str(tmp_path / "v.mp4"), 16, 24, 3)
    # the host form of the control tensor: (1, 3, F, H, W) in [-1, 1]
    t = IC.load_control_signal_tensor(clip)
    assert t.shape == (1, 3, 5, 16, 24) and t.dtype == torch.float32
    assert np.array_equal(t[0].permute(1, 2, 3, 0).numpy(), clip.astype(np.float32) / 127.5 - 1.0)


def test_save_control_sidecar_location(tmp_path, monkeypatch):
    """The edges go to save_dir under the control video's base name; beside the control video without one.  kernels.canny and the encoder
    are stand-ins: this is about where the file lands."""
    from ltx_2_mlx_amd.pipelines import ControlType, VideoCondition, ic_lora as IC

    class Enc:
        device = "cpu"

        def encode_patches(self, x):
            return torch.zeros(1, 128, 2, 1, 1)

    monkeypatch.setattr(IC.K, "canny", lambda x, low, high: x[..., 0])
    monkeypatch.setattr(IC.K, "frames_to_patches", lambda x: x)
    (tmp_path / "in").mkdir()
    (tmp_path / "out").mkdir()
    src = tmp_path / "in" / "clip.v1.npy"
    np.save(src, np.zeros((9, 32, 32, 3), np.uint8))
    wrote = []
    writer = lambda frames, path, fps: wrote.append((frames.shape, frames.dtype, path, fps))
    vc = [VideoCondition(str(src), control_type=ControlType.CANNY, save_control=True)]
    IC.create_video_conditionings(vc, Enc(), 32, 32, 9, save_video=writer, save_dir=str(tmp_path / "out"))
    IC.create_video_conditionings(vc, Enc(), 32, 32, 9, save_video=writer)
    assert wrote == [((9, 32, 32, 3), np.uint8, str(tmp_path / "out" / "clip.v1_canny.mp4"), 24),
                     ((9, 32, 32, 3), np.uint8, str(tmp_path / "in" / "clip.v1_canny.mp4"), 24)]
    IC.create_video_conditionings(vc, Enc(), 32, 32, 9, save_dir=str(tmp_path / "out"))                       # no writer: the frames as an array
    assert np.load(tmp_path / "out" / "clip.v1_canny.npz")["frames"].shape == (9, 32, 32, 3)
    IC.create_video_conditionings([VideoCondition(str(src), control_type=ControlType.RAW, save_control=True)], Enc(), 32, 32, 9, save_video=writer)
    assert len(wrote) == 2                                                                                    # nothing to save for a raw control


# ------------------------------------------------------------------ the conditioning against the reference's
def test_conditioning_matches_reference():
    """tests/golden/ic_lora_conditioning.npz (tools/pin_ic_lora_against_reference.py): the reference's own VideoConditionByLatentIndex and
    VideoConditionByKeyframeIndex applied in the pipeline's order, image first and control after it, on a (1, 128, 2, 2, 3) state."""
    from ltx_2_mlx_amd.components import VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning.keyframe import VideoConditionByKeyframeIndex
    from ltx_2_mlx_amd.conditioning.latent import VideoConditionByLatentIndex
    from ltx_2_mlx_amd.conditioning.tools import VideoLatentTools
    from ltx_2_mlx_amd.pipelines import apply_conditionings
    from ltx_2_mlx_amd.types import VideoLatentShape
    z = np.load(os.path.join(ROOT, "tests", "golden", "ic_lora_conditioning.npz"))
    t = lambda k: torch.from_numpy(z[k])
    assert z["control"].shape == (1, 128, 2, 2, 3) and z["initial"].shape == (1, 128, 2, 2, 3)
    tools = VideoLatentTools(patchifier=VideoLatentPatchifier(patch_size=1), target_shape=VideoLatentShape.from_shape(z["initial"].shape), fps=float(z["fps"]))
    state = tools.create_initial_state(dtype=torch.float32, initial_latent=t("initial"))
    conds = [VideoConditionByLatentIndex(latent=t("image"), strength=float(z["image_strength"]), latent_idx=0),
             VideoConditionByKeyframeIndex(keyframes=t("control"), frame_idx=0, strength=float(z["control_strength"]))]
    state = apply_conditionings(state, conds, tools)
    assert state.latent.shape == (1, 24, 128)
    assert np.array_equal(state.latent.numpy(), z["latent"]) and np.array_equal(state.clean_latent.numpy(), z["clean_latent"])
    assert np.array_equal(state.denoise_mask.numpy().reshape(-1), z["denoise_mask"].reshape(-1))
    assert state.positions.shape == z["positions"].shape and np.abs(state.positions.numpy() - z["positions"]).max() <= 1e-6
    # the control tokens sit after the 12 video tokens with mask 1 - strength; the image occupies latent frame 0
    m = state.denoise_mask.reshape(-1)
    assert torch.allclose(m[12:], torch.full((12,), 1 - float(z["control_strength"]))) and torch.allclose(m[:6], torch.full((6,), 1 - float(z["image_strength"])))
    cleared = tools.clear_conditioning(state)
    assert cleared.latent.shape == (1, 12, 128)


# ------------------------------------------------------------------ generate_video
def test_generate_video_routes_ic_lora(monkeypatch, tmp_path):
    import generate as gen

    class Routed(Exception):
        pass

    def spy(name):
        def f(*a, **k):
            raise Routed(name, a, k)
        return f

    for name in ("load_transformer", "load_av_transformer", "create_vae_decoder", "create_dummy_text_encoding", "encode_with_gemma"):
        monkeypatch.setattr(gen, name, spy(name))
    ctrl, lora, img = str(tmp_path / "c.npy"), str(tmp_path / "l.safetensors"), str(tmp_path / "i.png")
    np.save(ctrl, np.zeros((9, 64, 96, 3), np.uint8))
    open(lora, "wb").close()
    open(img, "wb").close()
    kw = dict(use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"), height=128, width=192, num_frames=9, pipeline_type="ic-lora")
    up = dict(spatial_upscaler_weights="random")
    cv = dict(control_video=ctrl)
    # with neither input it is refused by name, and the message names the flag
    with pytest.raises(NotImplementedError, match=r"ic-lora.*--control-video"):
        gen.generate_video("p", **kw, **up)
    # refused with this pipeline, before any model loads
    for extra in (dict(generate_audio=True), dict(audio_path="a.wav"), dict(two_stage_distilled=True), dict(upscale_temporal=True),
                  dict(keyframes=["k.png:0"])):
        with pytest.raises(NotImplementedError, match="ic-lora"):
            gen.generate_video("p", **kw, **up, **cv, **extra)
    with pytest.raises(NotImplementedError, match="fp8_resident"):
        gen.generate_video("p", **kw, **up, **cv, ic_lora_weights=lora, fp8_resident=True)
    with pytest.raises(ValueError, match="--spatial-upscaler-weights"):
        gen.generate_video("p", **kw, **cv)
    with pytest.raises(ValueError, match="divisible by 64"):
        gen.generate_video("p", **{**kw, "height": 96}, **up, **cv)
    with pytest.raises(ValueError, match="8\\*k \\+ 1"):
        gen.generate_video("p", **{**kw, "num_frames": 8}, **up, **cv)
    with pytest.raises(ValueError, match="depth"):
        gen.generate_video("p", **kw, **up, **cv, control_type="depth")
    with pytest.raises(FileNotFoundError, match="control video"):
        gen.generate_video("p", **kw, **up, control_video=str(tmp_path / "missing.npy"))
    with pytest.raises(FileNotFoundError, match="IC-LoRA weights"):
        gen.generate_video("p", **kw, **up, **cv, ic_lora_weights=str(tmp_path / "missing.safetensors"))
    # honoured with this pipeline only: refused exactly as before everywhere else
    for pt in ("text-to-video", "distilled", "one-stage", "ti2vid-hq"):
        for extra, name in ((cv, "control_video"), (dict(save_control=True), "save_control"), (dict(ic_lora_weights=lora), "ic_lora_weights")):
            with pytest.raises(NotImplementedError, match=name + "=.*outside the MI355X hot path"):
                gen.generate_video("p", **{**kw, "pipeline_type": pt}, **up, **extra)
    with pytest.raises(NotImplementedError, match="control_video"):
        gen.generate_video("p", **{**kw, "pipeline_type": "keyframe-interpolation"}, **up, **cv, keyframes=[img + ":0"])
    # everything in order: the first loader is reached
    for extra in (cv, dict(image_path=img), dict(**cv, image_path=img, ic_lora_weights=lora, save_control=True, control_type="canny", canny_low=50,
                                                  canny_high=150, control_strength=0.8)):
        with pytest.raises(Routed) as e:
            gen.generate_video("p", **kw, **up, **extra)
        assert e.value.args[0] == "create_dummy_text_encoding"
    # the command line reaches it
    a = gen.build_parser().parse_args(["a prompt", "--pipeline", "ic-lora", "--control-video", ctrl, "--control-type", "canny", "--save-control",
                                       "--ic-lora-weights", lora, "--canny-low", "50", "--control-strength", "0.8"])
    k = gen.kwargs_from_args(a)
    assert (k["pipeline_type"], k["control_video"], k["control_type"], k["save_control"], k["ic_lora_weights"], k["canny_low"], k["canny_high"],
            k["control_strength"]) == ("ic-lora", ctrl, "canny", True, lora, 50, 200, 0.8)


# ------------------------------------------------------------------ ABI
def test_abi_declares_the_control_entries():
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    assert nv.ABI_VERSION == 3
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    assert re.search(r"#define\s+LTX2_ABI_VERSION\s+3\b", header)
    for name in NEW_ENTRIES:
        assert name in nv.SIGNATURES and name in nv.exported_symbols(), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    n_args = lambda name: len(nv.SIGNATURES[name][1])
    assert (n_args("ltx2_canny_u8"), n_args("ltx2_canny_hysteresis"), n_args("ltx2_frames_to_patches")) == (11, 9, 7)
    macro = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert K.CANNY_TILE == (macro("LTX2_CANNY_TILE_H"), macro("LTX2_CANNY_TILE_W")) == (nv.CANNY_TILE_H, nv.CANNY_TILE_W)
    assert nv.CANNY_FLAG_BYTES == macro("LTX2_CANNY_FLAG_BYTES")
    assert "control.hip" in open(os.path.join(ROOT, "ltx-2-mlx_amd", "csrc", "Makefile")).read()
