"""Keyframe interpolation, the parts that need no GPU: the appended-token conditioning against the vector recorded from the reference
(tests/golden/keyframe_conditioning.npz, tools/pin_keyframe_against_reference.py), clear_conditioning, the config, the --keyframe parser,
generate_video's routing and the three new ABI entries."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEW_ENTRIES = ("ltx2_guided_euler_step", "ltx2_dit_guided_step", "ltx2_dit_graph_capture_guided")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "keyframe_conditioning.npz"))
    return {k: z[k] for k in z.files}


def _apply(golden):
    from ltx_2_mlx_amd.components import VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning import VideoConditionByKeyframeIndex, VideoLatentTools
    from ltx_2_mlx_amd.types import VideoLatentShape
    initial = torch.from_numpy(golden["initial"])
    tools = VideoLatentTools(patchifier=VideoLatentPatchifier(patch_size=1), target_shape=VideoLatentShape.from_shape(initial.shape),
                             fps=float(golden["fps"]))
    state = tools.create_initial_state(initial_latent=initial)
    for kf, idx, st in zip(golden["keyframes"], golden["frame_idx"], golden["strength"]):
        state = VideoConditionByKeyframeIndex(torch.from_numpy(kf), int(idx), float(st)).apply_to(state, tools)
    return tools, state


def test_keyframe_conditioning_equals_the_reference_vector(golden):
    """Two keyframes appended to a (1, 128, 3, 2, 3) state: frame 0 at strength 1 (causal first-frame shift on) and frame 16 at 0.9 (off)."""
    _, state = _apply(golden)
    assert state.latent.shape == (1, 18 + 2 * 6, 128) and state.positions.shape == (1, 3, 30, 2)
    assert torch.equal(state.latent, torch.from_numpy(golden["latent"]))
    assert torch.equal(state.clean_latent, torch.from_numpy(golden["clean_latent"]))
    assert torch.equal(state.denoise_mask, torch.from_numpy(golden["denoise_mask"]))
    assert float((state.positions - torch.from_numpy(golden["positions"])).abs().max()) <= 1e-6
    # what the two causal_fix settings mean: frame 0 covers [0, 1) frames, frame 16 covers [16, 24) frames, in seconds at fps 24
    assert state.positions[0, 0, 18].tolist() == pytest.approx([0.0, 1 / 24]) and state.positions[0, 0, 24].tolist() == pytest.approx([16 / 24, 1.0])


def test_keyframe_restatement_equals_the_reference_vector(golden):
    """tests/keyframe_ref.append_keyframe (what the GPU pipeline test compares against) gives the same four arrays."""
    import keyframe_ref as R
    from oracle import loop
    initial = torch.from_numpy(golden["initial"])
    tok = loop.patchify(initial)
    state = (tok, tok.clone(), torch.ones(1, 18, 1), loop.video_positions(1, 3, 2, 3, float(golden["fps"])))
    for kf, idx, st in zip(golden["keyframes"], golden["frame_idx"], golden["strength"]):
        state = R.append_keyframe(*state, torch.from_numpy(kf), int(idx), float(st), float(golden["fps"]))
    lat, clean, mask, pos = state
    assert torch.equal(lat, torch.from_numpy(golden["latent"])) and torch.equal(clean, torch.from_numpy(golden["clean_latent"]))
    assert torch.equal(mask, torch.from_numpy(golden["denoise_mask"]))
    assert float((pos - torch.from_numpy(golden["positions"])).abs().max()) <= 1e-6


def test_clear_conditioning_cuts_the_appended_tokens(golden):
    tools, state = _apply(golden)
    cleared = tools.clear_conditioning(state)
    assert cleared.latent.shape == (1, 18, 128) and cleared.positions.shape == (1, 3, 18, 2) and cleared.clean_latent.shape == (1, 18, 128)
    assert torch.equal(cleared.latent, state.latent[:, :18]) and torch.equal(cleared.denoise_mask, torch.ones(1, 18, 1))


def test_config_defaults_and_validation():
    from ltx_2_mlx_amd.pipelines import Keyframe, KeyframeInterpolationConfig
    d = {f.name: f.default for f in dataclasses.fields(KeyframeInterpolationConfig)}
    ref = dict(height=480, width=704, num_frames=97, num_inference_steps=30, cfg_scale=7.5, seed=42, fps=24.0, use_two_stage=True,
               stage_2_steps=3, tiling_config=None, dtype=torch.float32)
    assert {k: d[k] for k in ref} == ref
    # the reference's own defaults do not pass its own check (480 is no multiple of 64): kept, it is the reference's behaviour
    with pytest.raises(ValueError, match="divisible by 64"):
        KeyframeInterpolationConfig()
    assert KeyframeInterpolationConfig(use_two_stage=False).height == 480
    assert KeyframeInterpolationConfig(height=512).stage_2_steps == 3
    with pytest.raises(ValueError, match=r"8\*k \+ 1"):
        KeyframeInterpolationConfig(height=512, num_frames=96)
    kf = Keyframe("a.png", 8)
    assert kf.strength == 0.95 and kf.image is None


def test_keyframe_string_parsing():
    import generate as gen
    kf = gen.parse_keyframe("img.png:0")
    assert (kf.image_path, kf.frame_index, kf.strength) == ("img.png", 0, 0.95)
    kf = gen.parse_keyframe("dir/img2.png:64:0.9")
    assert (kf.image_path, kf.frame_index, kf.strength) == ("dir/img2.png", 64, 0.9)
    assert gen.parse_keyframe(kf) is kf
    with pytest.raises(ValueError, match=re.escape("Invalid keyframe format: img.png. Use 'path:frame_index' or 'path:frame_index:strength'")):
        gen.parse_keyframe("img.png")


def test_generate_video_routes_keyframes(monkeypatch, tmp_path):
    import generate as gen
    import ltx_2_mlx_amd.pipelines as P
    from PIL import Image

    class Routed(Exception):
        pass

    def spy(name):
        def f(*a, **k):
            raise Routed(name, a, k)
        return f

    loaders = ("load_transformer", "load_av_transformer", "create_vae_decoder", "create_dummy_text_encoding", "encode_with_gemma")
    for name in loaders:
        monkeypatch.setattr(gen, name, spy(name))
    img = str(tmp_path / "k.png")
    Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(img)
    kw = dict(use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"), height=128, width=192, num_frames=9)
    kfs = [f"{img}:0", f"{img}:8:0.9"]
    # the pipeline without keyframes: refused by name, and told how to run it
    with pytest.raises(NotImplementedError, match="keyframe-interpolation") as e:
        gen.generate_video("p", pipeline_type="keyframe-interpolation", **kw)
    assert "--keyframe" in str(e.value)
    # keyframes with another pipeline: refused by name
    with pytest.raises(NotImplementedError, match="keyframes"):
        gen.generate_video("p", pipeline_type="text-to-video", keyframes=kfs, **kw)
    # every combination that is not built fails before any loader is called (a loader would raise Routed)
    for bad in (dict(generate_audio=True), dict(audio_path=str(tmp_path / "a.wav")), dict(two_stage_distilled=True), dict(upscale_temporal=True),
                dict(image_path=img)):
        with pytest.raises(NotImplementedError, match=next(iter(bad))):
            gen.generate_video("p", pipeline_type="keyframe-interpolation", keyframes=kfs, **dict(kw, **bad))
    with pytest.raises(ValueError, match="Invalid keyframe format"):
        gen.generate_video("p", pipeline_type="keyframe-interpolation", keyframes=["nocolon"], **kw)
    with pytest.raises(ValueError, match="outside"):
        gen.generate_video("p", pipeline_type="keyframe-interpolation", keyframes=[f"{img}:9"], **kw)
    with pytest.raises(ValueError, match="divisible by 64"):
        gen.generate_video("p", pipeline_type="keyframe-interpolation", keyframes=kfs, **dict(kw, height=96))
    with pytest.raises(FileNotFoundError):
        gen.generate_video("p", pipeline_type="keyframe-interpolation", keyframes=[str(tmp_path / "missing.png") + ":0"], **kw)
    # keyframes + the pipeline: past the refusals, through the loaders, into KeyframeInterpolationPipeline
    with pytest.raises(Routed) as e:
        gen.generate_video("p", pipeline_type="keyframe-interpolation", keyframes=kfs, model_variant="dev", cfg_scale=3.0, **kw)
    assert e.value.args[0] == "create_dummy_text_encoding"
    ctx = torch.zeros(1, 4, 16)
    monkeypatch.setattr(gen, "create_dummy_text_encoding", lambda *a, **k: (ctx, None))
    monkeypatch.setattr(gen, "load_transformer", lambda *a, **k: "the transformer")
    monkeypatch.setattr(gen, "X0Model", lambda m: m)
    monkeypatch.setattr(gen, "create_vae_decoder", lambda *a, **k: "the decoder")

    class Enc:
        def __init__(self, **k):
            pass

        def init_random_weights(self, seed=0):
            pass

    monkeypatch.setattr(gen, "SimpleVideoEncoder", Enc)
    import ltx_2_mlx_amd.model.upscaler as U
    monkeypatch.setattr(U, "SpatialUpscaler", lambda **k: Enc())

    class SpyPipeline:
        def __init__(self, transformer, video_encoder, video_decoder, spatial_upscaler=None):
            self.parts = (transformer, video_encoder, video_decoder, spatial_upscaler)

        def __call__(self, text_encoding, text_mask, keyframes, config, negative_text_encoding=None, **k):
            raise Routed("pipeline", self.parts, dict(keyframes=keyframes, config=config, negative=negative_text_encoding, ctx=text_encoding))

    monkeypatch.setattr(P, "KeyframeInterpolationPipeline", SpyPipeline)
    with pytest.raises(Routed) as e:
        gen.generate_video("p", pipeline_type="keyframe-interpolation", keyframes=kfs, model_variant="dev", cfg_scale=3.0, num_steps=5, **kw)
    name, parts, got = e.value.args
    assert name == "pipeline" and parts[0] == "the transformer" and parts[2] == "the decoder" and isinstance(parts[1], Enc) and isinstance(parts[3], Enc)
    assert [(k.image_path, k.frame_index, k.strength) for k in got["keyframes"]] == [(img, 0, 0.95), (img, 8, 0.9)]
    c = got["config"]
    assert (c.height, c.width, c.num_frames, c.num_inference_steps, c.cfg_scale, c.fps, c.use_two_stage) == (128, 192, 9, 5, 3.0, 24.0, True)
    assert got["negative"] is None and got["ctx"] is ctx
    with pytest.raises(Routed) as e:                        # the distilled variant forces guidance off, as everywhere in this script
        gen.generate_video("p", pipeline_type="keyframe-interpolation", keyframes=kfs, cfg_scale=3.0, **kw)
    assert e.value.args[2]["config"].cfg_scale == 1.0


def test_abi_declares_the_guided_entries():
    from ltx_2_mlx_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    assert re.search(r"#define LTX2_ABI_VERSION 3\b", header) and nv.ABI_VERSION == 3
    for name in NEW_ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in nv.SIGNATURES and nv.SIGNATURES[name][0] is nv.i32, name
    # argument counts of the binding against the header's declarations
    for name in NEW_ENTRIES:
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(nv.SIGNATURES[name][1]), name
    lib = nv.lib() if os.path.exists(nv.LIB_PATH) else None
    if lib is not None:
        assert all(hasattr(lib, n) for n in NEW_ENTRIES)
