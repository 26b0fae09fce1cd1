"""TI2VidHQ with sound, the parts that need no GPU: the fp32 restatement of the joint loop (tests/hq_audio_ref.py) against the results recorded
from the reference's own loop (tests/golden/res2s_av_loop.npz, tools/pin_res2s_av_against_reference.py), the three new ABI entries, the
exports, generate_video's hq_av route and its refusals, and the refusal that stays."""
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

import hq_audio_ref as H  # noqa: E402

LOOP_GATE = 5 * 1.431e-6      # the threshold of tests/test_res2s_cpu.py for its golden: 5 x the largest difference torch.tanh's vector path was seen to make
NEW_ENTRIES = {"ltx2_res2s_midpoint_pair": 29, "ltx2_res2s_combine_pair": 30, "ltx2_dit_res2s_step_av": 21}


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "res2s_av_loop.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype == np.float32 else z[k]) for k in z.files}


# ------------------------------------------------------------------ the joint loop against the reference's own
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "plain"])
@pytest.mark.parametrize("table", ["scheduler", "final"])
def test_restatement_equals_the_reference(gold, table, guided):
    """hq_audio_ref.res2s_av_loop with the stored stub against the reference's own _res2s_denoise_loop over a video and an audio state
    (float32, executed through the shim): the same elementary fp32 operations in the same order; on the machine that recorded the fixture the
    maximum absolute difference is 0 on both modalities, all four cases."""
    t = gold
    p = {k: t[k] for k in ("w_v", "w_a", "x_av", "x_va", "bias_v", "bias_a")}
    pos = H.stub_x0_av(p, t["video_context"], t["audio_context"])
    neg = H.stub_x0_av(p, t["negative_video_context"], t["negative_audio_context"]) if guided else None
    cfg, acfg = float(t["cfg_scale"]), float(t["audio_cfg_scale"])
    assert cfg != acfg and cfg > 1 and acfg > 1
    assert sorted(set(t["video_mask"].reshape(-1).tolist())) == [0.0, pytest.approx(0.1), 1.0] and bool((t["audio_mask"] == 1).all())
    sig = t[f"sigmas_{table}"].tolist()
    trace, calls = [], []
    v, a = H.res2s_av_loop((t["video_latent"], t["video_mask"], t["video_clean"]), (t["audio_latent"], t["audio_mask"], t["audio_latent"]), pos, neg,
                           sig, cfg, acfg, trace, calls)
    tag = f"{table}_{'guided' if guided else 'plain'}"
    dv, da = float((v - t["video_" + tag]).abs().max()), float((a - t["audio_" + tag]).abs().max())
    print(f"joint res_2s restatement vs reference, {tag}: max abs difference video {dv:.3e} audio {da:.3e}")
    assert dv <= LOOP_GATE and da <= LOOP_GATE
    if table == "scheduler":
        assert sig[-1] == 0.0 and len(trace) == 4 and not any(f for _, _, f in trace) and trace[-1][1] == 0.0011
    else:
        assert [f for _, _, f in trace] == [False, True] and sig[-1] == 0.0005
        assert torch.equal(v[:, :4], t["video_clean"][:, :4])                          # after a final step the tokens of mask 0 sit on their clean values
    assert [list(c) for c in calls] == t["callbacks_" + tag].tolist() == [[i + 1, len(sig) - 1] for i in range(sum(not f for _, _, f in trace))]
    # guidance matters, per modality
    other = f"{table}_{'plain' if guided else 'guided'}"
    assert not torch.equal(t["video_" + tag], t["video_" + other]) and not torch.equal(t["audio_" + tag], t["audio_" + other])


def test_each_scale_guides_its_own_modality(gold):
    """In one evaluation the audio scale touches the audio output alone; over the loop it reaches the video through the cross dependency."""
    t = gold
    p = {k: t[k] for k in ("w_v", "w_a", "x_av", "x_va", "bias_v", "bias_a")}
    pos = H.stub_x0_av(p, t["video_context"], t["audio_context"])
    neg = H.stub_x0_av(p, t["negative_video_context"], t["negative_audio_context"])
    run = lambda sig, c, ac: H.res2s_av_loop((t["video_latent"], t["video_mask"], t["video_clean"]), (t["audio_latent"], t["audio_mask"], t["audio_latent"]),  # noqa: E731
                                             pos, neg, sig, c, ac)
    one = [0.5, 0.0005]                         # a single final step: latent = d
    (v1, a1), (v2, a2) = run(one, 3.0, 7.0), run(one, 3.0, 2.0)
    assert torch.equal(v1, v2) and not torch.equal(a1, a2)
    (v1, a1), (v2, a2) = run(one, 3.0, 7.0), run(one, 2.0, 7.0)
    assert not torch.equal(v1, v2) and torch.equal(a1, a2)
    sig = t["sigmas_scheduler"].tolist()
    assert not torch.equal(run(sig, 3.0, 7.0)[0], run(sig, 3.0, 2.0)[0])


# ------------------------------------------------------------------ ABI and exports
def test_abi_declares_the_joint_entries():
    from ltx_2_mlx_amd import _native as nv
    import ltx_2_mlx_amd.kernels as K
    import ltx_2_mlx_amd.pipelines as P
    from ltx_2_mlx_amd.model.transformer import LTXModel
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    assert re.search(r"#define\s+LTX2_ABI_VERSION\s+3\b", header) and nv.ABI_VERSION == 3          # additive entries: the version stays
    for name, n_args in NEW_ENTRIES.items():
        assert name in nv.SIGNATURES and nv.SIGNATURES[name][0] is nv.i32, name
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", header, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(nv.SIGNATURES[name][1]) == n_args, name
    capi = open(os.path.join(ROOT, "ltx-2-mlx_amd", "csrc", "capi.hip")).read() + open(os.path.join(ROOT, "ltx-2-mlx_amd", "csrc", "dit_engine.hip")).read()
    assert all(re.search(r"\bint " + name + r"\(", capi) for name in NEW_ENTRIES)
    if os.path.exists(nv.LIB_PATH):
        assert all(hasattr(nv.lib(), n) for n in NEW_ENTRIES)
    assert callable(K.res2s_midpoint_pair) and callable(K.res2s_combine_pair)
    assert hasattr(P, "res2s_av_denoise_loop") and "res2s_av_denoise_loop" in P.__all__
    assert callable(LTXModel.res2s_step_av_)
    sig = inspect.signature(P.res2s_av_denoise_loop).parameters
    assert list(sig) == ["transformer", "video_state", "audio_state", "sigmas", "video_context", "audio_context", "negative_video_context",
                         "negative_audio_context", "cfg_scale", "audio_cfg_scale", "callback", "use_hip_graph"]
    assert sig["callback"].default is None and sig["use_hip_graph"].default is True
    for fn in (P.TI2VidHQPipeline.__call__, P.TI2VidHQPipeline.denoise_latent):
        params = inspect.signature(fn).parameters
        for name in ("initial_noise", "stage2_noise", "initial_audio_noise", "stage2_audio_noise"):
            assert params[name].kind == inspect.Parameter.KEYWORD_ONLY and params[name].default is None, name


# ------------------------------------------------------------------ the loop's host side
class _FakeModel:
    is_av = True

    def __init__(self):
        self.calls, self.prepared = [], []

    def clone_sharing_weights(self):
        self.neg = _FakeModel()
        return self.neg

    def prepare(self, context, positions, per_token=False, audio_context=None, audio_positions=None):
        self.prepared.append((context, per_token, audio_context))

    def res2s_step_av_(self, neg, lat, alat, video, audio, sub, asub, sigma, sigma_next, cfg, acfg, **cond):
        self.calls.append((neg is not None, sigma, sigma_next, None if sub is None else float(sub.sigma[0]), None if asub is None else float(asub.sigma[0]),
                           video.timesteps.numel(), audio.timesteps.numel(), cfg, acfg, cond))


def test_loop_sigma_handling_contexts_and_forms(capsys):
    from ltx_2_mlx_amd.components import LTX2Scheduler
    from ltx_2_mlx_amd.pipelines import common
    from ltx_2_mlx_amd.types import LatentState
    common._eager_noted.clear()

    class X0:
        def __init__(self):
            self.velocity_model = _FakeModel()

    vmask = torch.ones(1, 6, 1)
    vmask[:, :2] = 0.0
    st = LatentState(latent=torch.zeros(1, 6, 8), denoise_mask=vmask, positions=torch.zeros(1, 3, 6, 2), clean_latent=torch.zeros(1, 6, 8))
    ast = LatentState(latent=torch.zeros(1, 5, 8), denoise_mask=torch.ones(1, 5, 1), positions=torch.zeros(1, 1, 5, 2), clean_latent=torch.zeros(1, 5, 8))
    ctx, actx, wide = torch.zeros(1, 4, 8), torch.ones(1, 4, 8), torch.zeros(1, 4, 16)
    f32 = lambda v: float(np.float32(v))          # noqa: E731
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    x, seen = X0(), []
    v, a = common.res2s_av_denoise_loop(x, st, ast, sig, ctx, actx, ctx, actx, 3.0, 7.0, callback=lambda i, n: seen.append((i, n)))
    calls = x.velocity_model.calls
    assert v.latent.shape == (1, 6, 8) and a.latent.shape == (1, 5, 8) and len(calls) == 4 and seen == [(1, 4), (2, 4), (3, 4), (4, 4)]
    assert calls[-1][2] == f32(0.0011) and [c[1] for c in calls] == sig[:4] and all(c[0] for c in calls)
    assert all(c[3] == c[4] and c[3] is not None for c in calls)                              # one sub-sigma, both modalities
    assert all((c[5], c[6], c[7], c[8]) == (6, 1, 3.0, 7.0) for c in calls)                   # per-token video, uniform audio, each its own scale
    assert calls[0][9]["denoise_mask"].shape == (6,) and calls[0][9]["audio_denoise_mask"] is None
    assert x.velocity_model.prepared[0][1] is True and x.velocity_model.neg.prepared[0][2] is actx
    assert "hipGraph replay skipped" in capsys.readouterr().err                              # use_hip_graph defaults to True: said once, not ignored silently
    x = X0()
    common.res2s_av_denoise_loop(x, st, ast, sig, ctx, actx, ctx, None, 3.0, 7.0)             # no callback: the same steps; the negative video context stands in
    assert [c[:3] for c in x.velocity_model.calls] == [c[:3] for c in calls] and x.velocity_model.neg.prepared[0][2] is ctx
    with pytest.raises(ValueError, match="negative_audio_context"):
        common.res2s_av_denoise_loop(X0(), st, ast, sig, wide, actx, wide, None, 3.0, 7.0)
    with pytest.raises(ValueError, match="audio_encoding"):
        common.res2s_av_denoise_loop(X0(), st, ast, sig, ctx, None, ctx, None, 3.0, 7.0)
    x, seen = X0(), []
    common.res2s_av_denoise_loop(x, st, ast, [0.5, 0.1, 0.0005], ctx, actx, ctx, actx, 3.0, 7.0, callback=lambda i, n: seen.append((i, n)))
    assert [(c[1], c[2]) for c in x.velocity_model.calls] == [(0.5, f32(0.1)), (f32(0.1), f32(0.0005))] and seen == [(1, 2)]
    assert x.velocity_model.calls[-1][3] is None and x.velocity_model.calls[-1][4] is None
    for cfg, acfg, nctx, want in ((1.0, 1.0, ctx, False), (1.0, 7.0, ctx, True), (3.0, 1.0, ctx, True), (3.0, 7.0, None, False)):
        x = X0()
        common.res2s_av_denoise_loop(x, st, ast, sig, ctx, actx, nctx, actx, cfg, acfg, callback=lambda i, n: None)
        assert all(c[0] == want for c in x.velocity_model.calls), (cfg, acfg, want)
    x = X0()
    common.res2s_av_denoise_loop(x, st, ast, [1.0 - 0.01 * i for i in range(70)], ctx, actx, ctx, actx, 3.0, 7.0)
    assert len(x.velocity_model.calls) == 69


# ------------------------------------------------------------------ generate_video / CLI
def _request(gen, **kw):
    sig = inspect.signature(gen.generate_video).parameters
    return dict({k: p.default for k, p in sig.items() if p.default is not inspect.Parameter.empty}, prompt="p", **kw)


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
    lora = str(tmp_path / "l.safetensors")
    open(lora, "wb").close()
    kw = dict(ti2vid_hq_audio=True, spatial_upscaler_weights="random", use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"),
              height=128, width=192, num_frames=9)
    for bad in (dict(audio_path="a.wav"), dict(two_stage_distilled=True), dict(upscale_temporal=True), dict(retake_video=str(tmp_path / "clip.npy")),
                dict(a2vid_two_stage=True)):
        with pytest.raises(NotImplementedError, match=next(iter(bad)) + " with ti2vid_hq_audio"):
            gen.generate_video("p", **dict(kw, **bad))
    with pytest.raises(NotImplementedError, match="keyframes"):
        gen.generate_video("p", **dict(kw, keyframes=["k.png:0"]))
    with pytest.raises(ValueError, match="spatial-upscaler-weights"):
        gen.generate_video("p", **dict(kw, spatial_upscaler_weights=None))
    with pytest.raises(ValueError, match="divisible by 64"):
        gen.generate_video("p", **dict(kw, height=96))
    with pytest.raises(NotImplementedError, match="drop fp8_resident"):
        gen.generate_video("p", **dict(kw, distilled_lora=lora, fp8_resident=True))
    with pytest.raises(FileNotFoundError, match="distilled LoRA not found"):
        gen.generate_video("p", **dict(kw, distilled_lora=str(tmp_path / "missing.safetensors")))
    # the existing hq route keeps its refusal, verbatim
    with pytest.raises(NotImplementedError, match=r"generate_audio with pipeline_type='ti2vid-hq': TI2VidHQPipeline is video-only \(the joint audio branch"):
        gen.generate_video("p", **dict(kw, ti2vid_hq_audio=False, pipeline_type="ti2vid-hq", generate_audio=True))
    r = gen._resolve_request(_request(gen, **dict(kw, distilled_lora=lora, distilled_lora_scale=0.5, model_variant="dev", cfg_scale=3.0)))
    assert r.route == "hq_av" and r.av and r.generate_audio and r.cfg_scale == 3.0 and r.audio_cfg_scale == 7.0 and not r.need_cfg
    assert (r.hq_lora.path, r.hq_lora.strength) == (lora, 0.5)
    with pytest.raises(Routed) as e:
        gen.generate_video("p", **kw)
    assert e.value.args[0] == "create_dummy_text_encoding"


def test_cli_flag_and_keyword():
    import generate as gen
    sig = inspect.signature(gen.generate_video).parameters
    assert sig["ti2vid_hq_audio"].kind == inspect.Parameter.KEYWORD_ONLY and sig["ti2vid_hq_audio"].default is False
    k = gen.kwargs_from_args(gen.build_parser().parse_args(["a prompt", "--ti2vid-hq-audio", "--spatial-upscaler-weights", "random", "--decode-audio"]))
    assert k["ti2vid_hq_audio"] is True and k["decode_audio"] is True and k["pipeline_type"] == "text-to-video"
    assert gen.kwargs_from_args(gen.build_parser().parse_args(["a prompt"]))["ti2vid_hq_audio"] is False
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "generate_cli_flags.json")))
    have = {s for act in gen.build_parser()._actions for s in (act.option_strings or [act.dest])}
    assert len(gold["flags"]) == 57 and all(s in have for f in gold["flags"] for s in f["flags"])
    assert "--ti2vid-hq-audio" not in {s for f in gold["flags"] for s in f["flags"]}
    assert "hq_av" in gen._ROUTES and "hq_av" in gen._ROUTE_EXCLUDES and gen._ROUTE_OWNS["hq_av"] == ("distilled_lora",)
    assert set(gen._ROUTE_EXCLUDES["hq_av"][0]) == {"audio_path", "two_stage_distilled", "upscale_temporal", "keyframes", "retake_video", "a2vid_two_stage"}
    flag = next(act for act in gen.build_parser()._actions if "--ti2vid-hq-audio" in act.option_strings)
    assert "--ti2vid-hq /" in flag.help and "--generate-audio" in flag.help              # the help points at the video-only route


# ------------------------------------------------------------------ the refusal that stays
def test_audio_on_a_video_only_model_still_raises():
    from ltx_2_mlx_amd.pipelines import TI2VidHQConfig, TI2VidHQPipeline

    class M:
        model_type = None
        device = "cpu"

    pipe = TI2VidHQPipeline.__new__(TI2VidHQPipeline)
    pipe.transformer = pipe._velocity_model = M()
    pipe.spatial_upscaler = object()
    conf = TI2VidHQConfig(height=64, width=128, num_frames=9, audio_enabled=True)
    for call in (pipe.denoise_latent, pipe.stage1_latent, pipe.__call__):
        with pytest.raises(NotImplementedError, match="TI2VidHQPipeline.*AudioVideo"):
            call(torch.zeros(1, 4, 8), None, conf)
