"""Audio-to-video, the parts that need no GPU: A2VidConfig against the reference's fields, the fp32 restatement of the video-only loop
against the results recorded from the reference's own class (tests/golden/a2vid_loop.npz, tools/pin_a2vid_against_reference.py), the new
route's refusals before any model loads, the command line, and the new ABI entries and exports."""
import dataclasses
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEW_ENTRIES = ("ltx2_dit_guided_step_av", "ltx2_dit_graph_capture_guided_av")


# ------------------------------------------------------------------ config
def test_config_defaults_and_validation():
    from ltx_2_mlx_amd.pipelines import A2VidConfig
    from ltx_2_mlx_amd.model.video_vae import TilingConfig
    d = {f.name: f.default for f in dataclasses.fields(A2VidConfig)}
    ref = dict(height=512, width=768, num_frames=97, num_inference_steps=30, cfg_scale=3.0, seed=42, fps=25.0, distilled_lora_config=None,
               tiling_config=None, audio_vae_channels=8, audio_mel_bins=16, audio_sample_rate=16000, audio_hop_length=160,
               audio_downsample_factor=4, audio_output_sample_rate=24000, audio_start_time=0.0, audio_max_duration=None)
    assert {k: d[k] for k in ref} == ref
    assert list(d)[:len(ref) + 1] == list(ref)[:9] + ["dtype"] + list(ref)[9:]          # the reference's fields in the reference's order
    assert isinstance(d["dtype"], torch.dtype) and d["use_hip_graph"] is True and list(d)[-1] == "use_hip_graph"
    with pytest.raises(ValueError, match=r"num_frames must be 8\*k \+ 1, got 96"):
        A2VidConfig(num_frames=96)
    with pytest.raises(ValueError, match=r"Resolution \(480x768\) must be divisible by 64\."):
        A2VidConfig(height=480)
    with pytest.raises(ValueError, match="divisible by 64"):
        A2VidConfig(width=736)
    c = A2VidConfig()
    assert isinstance(c._get_tiling_config(), TilingConfig)                               # 13 * 16 * 24 = 4992 latent voxels > 4000
    assert A2VidConfig(height=256, width=384)._get_tiling_config() is None
    mine = TilingConfig.default()
    assert A2VidConfig(height=256, width=384, tiling_config=mine)._get_tiling_config() is mine


# ------------------------------------------------------------------ the restatement against the reference's class
@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "a2vid_loop.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _restated(g, scale, neg_v, neg_a, seen=None):
    import a2vid_ref as R
    return R.video_only_denoise_loop(g["latent"], g["denoise_mask"], g["clean_latent"], g["audio"], g["sigmas"].tolist(), R.toy_x0_video,
                                     g["video_context"], g["audio_context"], g["negative_video_context"] if neg_v else None,
                                     g["negative_audio_context"] if neg_a else None, scale,
                                     (lambda i, n: seen.append([i, n])) if seen is not None else None)


@pytest.mark.parametrize("run,scale,neg_v,neg_a", [("cfg3_no_negative_audio", 3.0, True, False), ("cfg1", 1.0, True, True),
                                                   ("cfg3_no_negative", 3.0, False, False)])
def test_restated_loop_equals_the_reference_recording(golden, run, scale, neg_v, neg_a):
    """tests/a2vid_ref.video_only_denoise_loop (what the GPU tests compare against) over the toy transformer, against what the reference's
    _video_only_denoise_loop gave for the same inputs.  Both are fp32 torch arithmetic; the bound allows for another order of the same ops."""
    seen = []
    v, a = _restated(golden, scale, neg_v, neg_a, seen)
    assert a is golden["audio"] and torch.equal(golden[run + "_audio"], golden["audio"])          # untouched, there and here
    assert seen == golden[run + "_callback"].tolist() == [[1, 3], [2, 3], [3, 3]]
    assert float((v - golden[run + "_video"]).abs().max()) <= 1e-5 * float(golden[run + "_video"].abs().max())
    assert float((v - golden["latent"]).abs().max()) > 0.1                                    # the video moved


def test_what_the_recording_says_about_guidance(golden):
    g = golden
    # cfg = 1 and a missing negative video context both skip the second evaluation: the same bits in the reference's own results
    assert torch.equal(g["cfg1_video"], g["cfg3_no_negative_video"])
    assert float((g["cfg3_no_negative_audio_video"] - g["cfg1_video"]).abs().max()) > 1e-2       # guidance acts on the video
    # the conditioned token (mask 0) ends at its clean latent under guidance too
    assert float((g["cfg3_no_negative_audio_video"][0, 0] - g["clean_latent"][0, 0]).abs().max()) < 1e-5
    # negative_audio_context None falls back to audio_context: the restatement gives the recorded result with either spelling ...
    fallback, _ = _restated(g, 3.0, True, False)
    g2 = dict(g, negative_audio_context=g["audio_context"])
    explicit, _ = _restated(g2, 3.0, True, True)
    assert torch.equal(fallback, explicit)
    # ... and another one with a negative audio context of its own (a run the reference cannot make: see the pin tool)
    own, _ = _restated(g, 3.0, True, True)
    assert float((own - fallback).abs().max()) > 1e-4


# ------------------------------------------------------------------ the loop's own checks
def test_loop_refuses_an_audio_state_that_is_not_frozen():
    from ltx_2_mlx_amd.pipelines import frozen_audio_guided_loop
    from ltx_2_mlx_amd.types import LatentState
    a = torch.zeros(1, 4, 128)
    audio = LatentState(latent=a, denoise_mask=torch.tensor([0.0, 0.0, 0.5, 0.0]).reshape(1, 4, 1), positions=torch.zeros(1, 1, 4, 2), clean_latent=a)
    with pytest.raises(ValueError, match="all zero"):
        frozen_audio_guided_loop(object(), None, audio, [1.0, 0.0], None, None, None, None, 3.0, None)
    sig = inspect.signature(frozen_audio_guided_loop).parameters
    assert list(sig) == ["transformer", "video_state", "audio_state", "sigmas", "video_context", "audio_context", "negative_video_context",
                         "negative_audio_context", "cfg_scale", "stepper", "callback", "use_hip_graph"]
    assert sig["callback"].default is None and sig["use_hip_graph"].default is True


# ------------------------------------------------------------------ generate_video / CLI
def test_route_refusals_come_before_any_model(monkeypatch, tmp_path):
    import generate as gen

    class Routed(Exception):
        pass

    def spy(name):
        def f(*a, **k):
            raise Routed(name)
        return f

    for name in ("load_transformer", "load_av_transformer", "create_vae_decoder", "create_dummy_text_encoding", "encode_with_gemma",
                 "encode_audio_for_video"):
        monkeypatch.setattr(gen, name, spy(name))
    wav, lora = str(tmp_path / "a.wav"), str(tmp_path / "l.safetensors")
    open(wav, "wb").close()
    open(lora, "wb").close()
    kw = dict(a2vid_two_stage=True, audio_path=wav, spatial_upscaler_weights="random", use_gemma=False, device="cpu",
              output_path=str(tmp_path / "o.mp4"), height=128, width=192, num_frames=9)
    with pytest.raises(ValueError, match="a2vid_two_stage needs audio_path"):
        gen.generate_video("p", **dict(kw, audio_path=None))
    with pytest.raises(ValueError, match="spatial-upscaler-weights"):
        gen.generate_video("p", **dict(kw, spatial_upscaler_weights=None))
    with pytest.raises(FileNotFoundError, match="audio file not found"):
        gen.generate_video("p", **dict(kw, audio_path=str(tmp_path / "missing.wav")))
    for bad in (dict(two_stage_distilled=True), dict(upscale_temporal=True), dict(retake_video=str(tmp_path / "clip.npy"))):
        with pytest.raises(NotImplementedError, match=next(iter(bad)) + " with a2vid_two_stage"):
            gen.generate_video("p", **dict(kw, **bad))
    for bad in (dict(keyframes=["k.png:0"]), dict(control_video="c.npy")):
        with pytest.raises(NotImplementedError, match=next(iter(bad))):
            gen.generate_video("p", **dict(kw, **bad))
    with pytest.raises(NotImplementedError, match="drop fp8_resident"):
        gen.generate_video("p", **dict(kw, distilled_lora=lora, fp8_resident=True))
    with pytest.raises(FileNotFoundError, match="distilled LoRA not found"):
        gen.generate_video("p", **dict(kw, distilled_lora=str(tmp_path / "missing.safetensors")))
    with pytest.raises(ValueError, match="divisible by 64"):
        gen.generate_video("p", **dict(kw, height=96))
    # what stays refused as it was: audio_path with two_stage_distilled, audio_path on the video-only branch
    with pytest.raises(NotImplementedError, match="audio_path .* with two_stage_distilled"):
        gen.generate_video("p", **dict(kw, a2vid_two_stage=False, two_stage_distilled=True, generate_audio=True))
    with pytest.raises(ValueError, match="needs the AudioVideo branch"):
        gen.generate_video("p", **dict(kw, a2vid_two_stage=False))
    # past the refusals: the route, the AudioVideo transformer, the forced cfg of the distilled variant
    r = gen._resolve_request(_request(gen, **dict(kw, distilled_lora=lora, distilled_lora_scale=0.5, model_variant="dev", cfg_scale=3.0)))
    assert r.route == "a2vid" and r.av and r.generate_audio and r.cfg_scale == 3.0 and not r.need_cfg
    assert (r.a2vid_lora.path, r.a2vid_lora.strength) == (lora, 0.5)
    assert gen._resolve_request(_request(gen, **dict(kw, cfg_scale=3.0))).cfg_scale == 1.0
    with pytest.raises(Routed) as e:
        gen.generate_video("p", **kw)
    assert e.value.args[0] == "create_dummy_text_encoding"


def _request(gen, **kw):
    sig = inspect.signature(gen.generate_video).parameters
    return dict({k: p.default for k, p in sig.items() if p.default is not inspect.Parameter.empty}, prompt="p", **kw)


def test_cli_flag_and_keyword():
    import generate as gen
    sig = inspect.signature(gen.generate_video).parameters
    assert sig["a2vid_two_stage"].kind == inspect.Parameter.KEYWORD_ONLY and sig["a2vid_two_stage"].default is False
    a = gen.build_parser().parse_args(["a prompt", "--a2vid-two-stage", "--audio", "in.wav", "--spatial-upscaler-weights", "random"])
    k = gen.kwargs_from_args(a)
    assert k["a2vid_two_stage"] is True and k["audio_path"] == "in.wav" and k["pipeline_type"] == "text-to-video"
    assert gen.kwargs_from_args(gen.build_parser().parse_args(["a prompt"]))["a2vid_two_stage"] is False
    # the reference's 57 flags are all still there, and --pipeline keeps the reference's choices
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "generate_cli_flags.json")))
    have = {s for act in gen.build_parser()._actions for s in (act.option_strings or [act.dest])}
    assert len(gold["flags"]) == 57 and all(s in have for f in gold["flags"] for s in f["flags"])
    assert "--a2vid-two-stage" not in {s for f in gold["flags"] for s in f["flags"]}
    assert set(gen._ROUTES) >= {"a2vid"} and "a2vid" in gen._ROUTE_EXCLUDES and gen._ROUTE_OWNS["a2vid"] == ("distilled_lora",)
    assert gen.fit_audio_latent.__module__ == "ltx_2_mlx_amd.pipelines.a2vid_two_stage"          # the loader lives in the package


# ------------------------------------------------------------------ exports
def test_abi_and_exports():
    from ltx_2_mlx_amd import _native as nv
    import ltx_2_mlx_amd.pipelines as P
    from ltx_2_mlx_amd.model.transformer import LTXModel
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    assert re.search(r"#define LTX2_ABI_VERSION 3\b", header) and nv.ABI_VERSION == 3          # additive entries: the version stays
    for name in NEW_ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in nv.SIGNATURES and nv.SIGNATURES[name][0] is nv.i32, name
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(nv.SIGNATURES[name][1]), name
    assert re.search(r"ltx2_dit_guided_step_av\([^)]*const float\* a_latent", header, re.S)      # the audio latent is read-only in the ABI
    lib = nv.lib() if os.path.exists(nv.LIB_PATH) else None
    if lib is not None:
        assert all(hasattr(lib, n) for n in NEW_ENTRIES)
    for name in ("A2VidConfig", "A2VidPipelineTwoStage", "create_a2vid_pipeline", "encode_audio_file", "frozen_audio_guided_loop"):
        assert hasattr(P, name) and name in P.__all__, name
    for name in ("guided_step_av_", "capture_guided_av_graph", "replay_guided_av_graph"):
        assert callable(getattr(LTXModel, name)), name
    sig = inspect.signature(P.A2VidPipelineTwoStage.__init__).parameters
    assert list(sig)[1:] == ["transformer", "video_encoder", "video_decoder", "spatial_upscaler", "audio_decoder", "vocoder", "audio_encoder",
                             "audio_processor"]
    call = inspect.signature(P.A2VidPipelineTwoStage.__call__).parameters
    assert list(call)[1:9] == ["audio_path", "positive_encoding", "negative_encoding", "config", "images", "callback", "positive_audio_encoding",
                               "negative_audio_encoding"]
    assert all(call[n].kind == inspect.Parameter.KEYWORD_ONLY for n in ("initial_noise", "stage_2_noise", "audio_latent"))
