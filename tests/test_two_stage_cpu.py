"""The two-stage pipeline, the parts that need no GPU: MultiModalGuider against hand-computed values, the configuration's errors, the new ABI
entries, the exports, generate_video's two_stage_cfg route with its refusals (and the refusal of pipeline_type="two-stage" that stays), and the
loop's host side on a recording model."""
import dataclasses
import inspect
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import two_stage_ref as R  # noqa: E402

NEW_ENTRIES = {"ltx2_mm_guided_euler_step": 18, "ltx2_mm_guided_euler_step_pair": 33, "ltx2_mm_guidance_sums": 15, "ltx2_mm_rescaled_euler_step": 21,
               "ltx2_dit_forward_isolated_av": 12, "ltx2_dit_mm_guided_step_av": 32}


# ------------------------------------------------------------------ the guider
def test_guider_hand_computed():
    from ltx_2_mlx_amd.components import MultiModalGuider, MultiModalGuiderParams
    cond, u, p, m = (torch.tensor([[v, -v]]) for v in (1.0, 0.5, 0.25, 2.0))
    g = MultiModalGuider(MultiModalGuiderParams(cfg_scale=3.0, stg_scale=0.5, modality_scale=4.0))
    # 1 + 2*(1 - 0.5) + 0.5*(1 - 0.25) + 3*(1 - 2) = 1 + 1 + 0.375 - 3
    assert g.calculate(cond, u, p, m).tolist() == [[-0.625, 0.625]]
    assert g.calculate(cond, u, 0.0, m).tolist() == [[-1.0, 1.0]]                  # a float: that pass did not run
    assert g.calculate(cond, 0.0, 0.0, m).tolist() == [[-2.0, 2.0]]
    assert g.calculate(cond, u, 0.0, 0.0).tolist() == [[2.0, -2.0]]
    assert g.calculate(cond, 0.0, 0.0, 0.0) is cond
    neutral = MultiModalGuider(MultiModalGuiderParams())                           # a pass that ran at a neutral scale adds an exact zero
    assert torch.equal(neutral.calculate(cond, u, p, m), cond)
    # rescale: pred = 3 * cond here, so var(pred) = 9 var(cond) and the factor is 0.7 / 3 + 0.3 (up to the 1e-8)
    r = MultiModalGuider(MultiModalGuiderParams(cfg_scale=3.0, rescale_scale=0.7))
    out = r.calculate(cond, torch.zeros_like(cond), 0.0, 0.0)
    assert torch.allclose(out, 3.0 * cond * (0.7 / 3 + 0.3), rtol=1e-6)
    # the restatement the GPU tests use agrees with the guider where the scale differences are exact
    assert torch.equal(R.calculate(cond, u, p, m, 3.0, 0.5, 4.0), g.calculate(cond, u, p, m))
    s = R.sums_f64(cond, 3.0 * cond)
    assert R.rescale_factor_f64(s, 2, 0.7) == pytest.approx(0.7 / 3 + 0.3, rel=1e-7)
    for params, want in ((dict(), (False, False, False)), (dict(cfg_scale=3.0), (True, False, False)), (dict(stg_scale=1.0), (False, True, False)),
                         (dict(modality_scale=3.0), (False, False, True)), (dict(cfg_scale=1.0 + 1e-12, modality_scale=1.0 - 1e-12, stg_scale=0.0), (False, False, False)), (dict(stg_scale=1e-12), (False, True, False))):
        # (math.isclose's relative tolerance: 1 + 1e-12 is close to 1, while nothing but 0 is close to 0 -- stg_scale 1e-12 runs the pass, as in the reference)
        g = MultiModalGuider(MultiModalGuiderParams(**params))
        assert (g.do_unconditional_generation(), g.do_perturbed_generation(), g.do_isolated_modality_generation()) == want, params
    assert not any(MultiModalGuider(MultiModalGuiderParams()).should_skip_step(i) for i in range(5))
    assert [MultiModalGuider(MultiModalGuiderParams(skip_step=2)).should_skip_step(i) for i in range(6)] == [False, True, True, False, True, True]
    d = MultiModalGuiderParams()
    assert (d.cfg_scale, d.stg_scale, d.stg_blocks, d.rescale_scale, d.modality_scale, d.skip_step) == (1.0, 0.0, [], 0.0, 1.0, 0)
    with pytest.raises(Exception):
        d.cfg_scale = 2.0                                                          # frozen


def test_config_errors_and_exports():
    import ltx_2_mlx_amd.components as C
    import ltx_2_mlx_amd.pipelines as P
    for name in ("MultiModalGuider", "MultiModalGuiderParams"):
        assert name in C.__all__ and hasattr(C, name)
    for name in ("TwoStageCFGConfig", "TwoStagePipeline", "create_two_stage_pipeline", "multimodal_denoise_loop"):
        assert name in P.__all__ and hasattr(P, name)
    d = {f.name: f.default for f in dataclasses.fields(P.TwoStageCFGConfig)}
    assert [d[k] for k in ("height", "width", "num_frames", "num_inference_steps", "cfg_scale", "audio_cfg_scale", "guidance_rescale", "modality_scale", "rescale_scale",
                           "audio_enabled", "use_internal_audio_branch")] == [480, 704, 97, 30, 3.0, 7.0, 0.0, 3.0, 0.0, False, True]
    with pytest.raises(ValueError, match=r"Resolution \(480x704\)"):
        P.TwoStageCFGConfig()                      # the reference's own defaults do not pass its own check: kept as it is
    with pytest.raises(ValueError, match=r"num_frames must be 8\*k \+ 1, got 10"):
        P.TwoStageCFGConfig(height=128, width=192, num_frames=10)
    with pytest.raises(ValueError, match=r"Resolution \(96x192\) must be divisible by 64 for two-stage pipeline"):
        P.TwoStageCFGConfig(height=96, width=192, num_frames=9)
    for fn in (P.TwoStagePipeline.__call__, P.TwoStagePipeline.denoise_latent):
        params = inspect.signature(fn).parameters
        for name in ("initial_noise", "stage_2_noise", "initial_audio_noise", "stage_2_audio_noise"):
            assert params[name].kind == inspect.Parameter.KEYWORD_ONLY and params[name].default is None, name
    sig = inspect.signature(P.multimodal_denoise_loop).parameters
    assert list(sig) == ["transformer", "video_state", "audio_state", "sigmas", "video_context", "audio_context", "negative_video_context",
                         "negative_audio_context", "video_guider", "audio_guider", "callback", "fused"] and sig["fused"].default is True
    vg, ag = P.TwoStagePipeline.guiders(None, P.TwoStageCFGConfig(height=128, width=192, rescale_scale=0.5))
    assert (vg.params.cfg_scale, ag.params.cfg_scale, vg.params.modality_scale, ag.params.modality_scale, vg.params.rescale_scale, ag.params.stg_scale) == (3.0, 7.0, 3.0, 3.0, 0.5, 0.0)


def test_video_only_model_is_refused():
    from ltx_2_mlx_amd.pipelines import TwoStageCFGConfig, TwoStagePipeline

    class M:
        model_type = None
        device = "cpu"

    pipe = TwoStagePipeline.__new__(TwoStagePipeline)
    pipe.transformer = pipe._velocity_model = M()
    pipe.is_av_model = False
    pipe.spatial_upscaler = object()
    pipe.audio_decoder = pipe.vocoder = None
    conf = TwoStageCFGConfig(height=64, width=128, num_frames=9)
    z = torch.zeros(1, 2, 4)
    for call in (pipe.denoise_latent, pipe.stage1_latent, pipe.__call__):
        with pytest.raises(NotImplementedError, match="_denoise_loop_cfg.*undefined `guider`"):
            call(z, z, conf, positive_audio_encoding=z, negative_audio_encoding=z)


# ------------------------------------------------------------------ the ABI
def test_new_entries_in_header_and_binding():
    from ltx_2_mlx_amd import _native as nv
    assert nv.ABI_VERSION == 3
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltx2hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+LTX2_ABI_VERSION\s+3\b", txt)
    for name, n in NEW_ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, name
        assert len(m.group(1).split(",")) == n == len(nv.SIGNATURES[name][1]), name
    assert "ltx2_mm_guidance_sums_blocks" not in nv.SIGNATURES                      # ltx2_guidance_sums_blocks is shared
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import LTXModel, X0Model
    for name in ("mm_guided_euler_step", "mm_guided_euler_step_pair", "mm_guidance_sums", "mm_rescaled_euler_step"):
        assert callable(getattr(K, name))
    assert callable(LTXModel.forward_isolated) and callable(LTXModel.mm_guided_step_av_) and callable(X0Model.forward_isolated)


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
    kw = dict(two_stage_cfg=True, spatial_upscaler_weights="random", use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"),
              height=128, width=192, num_frames=9)
    for bad in (dict(ti2vid_hq_audio=True), dict(a2vid_two_stage=True), dict(retake_video=str(tmp_path / "clip.npy")), dict(two_stage_distilled=True),
                dict(upscale_temporal=True), dict(audio_path="a.wav")):
        with pytest.raises(NotImplementedError, match=next(iter(bad)) + " with two_stage_cfg"):
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
    # pipeline_type="two-stage" keeps its refusal, verbatim
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "generate_routes.json")))
    pinned = [v for v in _strings(gold) if v.startswith("pipeline_type='two-stage' is outside the MI355X hot path")]
    assert len(pinned) >= 1
    with pytest.raises(NotImplementedError) as e:
        gen.generate_video("p", **dict(kw, two_stage_cfg=False, pipeline_type="two-stage"))
    assert str(e.value) == pinned[0]
    r = gen._resolve_request(_request(gen, **dict(kw, distilled_lora=lora, distilled_lora_scale=0.5, model_variant="dev", cfg_scale=3.0)))
    assert r.route == "two_stage_cfg" and r.av and r.generate_audio and r.cfg_scale == 3.0 and r.audio_cfg_scale == 7.0 and not r.need_cfg and r.encode_negative
    assert (r.two_stage_lora.path, r.two_stage_lora.strength) == (lora, 0.5) and r.modality_scale == 3.0 and r.two_stage_rescale == 0.0
    with pytest.raises(Routed) as e:
        gen.generate_video("p", **kw)
    assert e.value.args[0] == "create_dummy_text_encoding"


def _strings(o):
    if isinstance(o, str):
        yield o
    elif isinstance(o, dict):
        for v in o.values():
            yield from _strings(v)
    elif isinstance(o, (list, tuple)):
        for v in o:
            yield from _strings(v)


def test_cli_flag_and_keywords():
    import generate as gen
    sig = inspect.signature(gen.generate_video).parameters
    for name, default in (("two_stage_cfg", False), ("modality_scale", 3.0), ("two_stage_rescale", 0.0)):
        assert sig[name].kind == inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
    k = gen.kwargs_from_args(gen.build_parser().parse_args(["a prompt", "--two-stage-cfg", "--modality-scale", "2.5", "--spatial-upscaler-weights", "random"]))
    assert k["two_stage_cfg"] is True and k["modality_scale"] == 2.5 and k["pipeline_type"] == "text-to-video"
    d = gen.kwargs_from_args(gen.build_parser().parse_args(["a prompt"]))
    assert d["two_stage_cfg"] is False and d["modality_scale"] == 3.0
    assert list(gen._ROUTES)[0] == "two_stage_cfg" and gen._ROUTE_OWNS["two_stage_cfg"] == ("distilled_lora",)
    assert set(gen._ROUTE_EXCLUDES["two_stage_cfg"][0]) == {"ti2vid_hq_audio", "a2vid_two_stage", "retake_video", "keyframes", "two_stage_distilled",
                                                            "upscale_temporal", "audio_path"}
    assert all("stg_scale" not in v for k, v in gen._ROUTE_OWNS.items() if k != "av")


# ------------------------------------------------------------------ the loop's host side
class _FakeModel:
    is_av = True
    out_channels = AUDIO_OUT_CHANNELS = 8

    def __init__(self):
        self.calls, self.prepared, self.stg = [], [], {}

    def clone_sharing_weights(self):
        self.neg = _FakeModel()
        return self.neg

    def prepare(self, context, positions, per_token=False, audio_context=None, audio_positions=None):
        self.prepared.append((context, per_token, audio_context))

    def set_stg_blocks(self, blocks, modality=0):
        self.stg[modality] = blocks

    def mm_guided_step_av_(self, neg, lat, alat, video, audio, sigma, sigma_next, vparams, aparams, isolated=None, perturbed=None, **cond):
        self.calls.append((neg is not None, isolated is not None, perturbed is not None, sigma, sigma_next, video.timesteps.numel(), audio.timesteps.numel(),
                           vparams, aparams, None if isolated is None else tuple(t.shape for t in isolated), cond))


def test_loop_passes_and_call_order():
    from ltx_2_mlx_amd.components import LTX2Scheduler, MultiModalGuider, MultiModalGuiderParams
    from ltx_2_mlx_amd.pipelines import common
    from ltx_2_mlx_amd.types import LatentState

    class X0:
        def __init__(self):
            self.velocity_model = _FakeModel()

    vmask = torch.ones(1, 6, 1)
    vmask[:, :2] = 0.0
    st = LatentState(latent=torch.zeros(1, 6, 8), denoise_mask=vmask, positions=torch.zeros(1, 3, 6, 2), clean_latent=torch.zeros(1, 6, 8))
    ast = LatentState(latent=torch.zeros(1, 5, 8), denoise_mask=torch.ones(1, 5, 1), positions=torch.zeros(1, 1, 5, 2), clean_latent=torch.zeros(1, 5, 8))
    ctx, actx, nctx, nactx = (torch.full((1, 4, 8), float(i)) for i in range(4))
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    mk = lambda **p: MultiModalGuider(MultiModalGuiderParams(**p))      # noqa: E731
    # which passes run: every combination of cfg = 1, mod = 1, stg = 0 on the video guider, the audio guider neutral and then not
    for cfg in (1.0, 3.0):
        for mod in (1.0, 3.0):
            for stg in (0.0, 0.8):
                for audio_too in (False, True):
                    x, seen = X0(), []
                    vg = mk(cfg_scale=cfg, modality_scale=mod, stg_scale=stg, stg_blocks=[1])
                    ag = mk(cfg_scale=7.0, modality_scale=3.0, stg_scale=0.5, stg_blocks=None) if audio_too else mk()
                    common.multimodal_denoise_loop(x, st, ast, sig, ctx, actx, nctx, nactx, vg, ag, callback=lambda i, n: seen.append((i, n)))
                    m = x.velocity_model
                    want = (cfg != 1.0 or audio_too, mod != 1.0 or audio_too, stg != 0.0 or audio_too)
                    assert len(m.calls) == 4 and seen == [(1, 4), (2, 4), (3, 4), (4, 4)]
                    assert all(c[:3] == want for c in m.calls), (cfg, mod, stg, audio_too)
                    assert [c[3] for c in m.calls] == sig[:4] and [c[4] for c in m.calls] == sig[1:]
                    assert all((c[5], c[6]) == (6, 1) and c[7] is vg.params and c[8] is ag.params for c in m.calls)       # per-token video, uniform audio
                    assert m.prepared == [(ctx, True, actx)] and (m.neg.prepared == [(nctx, True, nactx)] if want[0] else not hasattr(m, "neg"))
                    assert m.stg == ({0: [1], 1: None} if audio_too else {0: [1], 1: []} if want[2] else {})
                    if want[1]:
                        assert m.calls[0][9] == ((6, 8), (5, 8))
                    assert m.calls[0][10]["denoise_mask"].shape == (6,) and m.calls[0][10]["audio_denoise_mask"] is None
    with pytest.raises(ValueError, match="negative prompt"):
        common.multimodal_denoise_loop(X0(), st, ast, sig, ctx, actx, None, nactx, mk(cfg_scale=3.0), mk())
    with pytest.raises(ValueError, match="audio_encoding"):
        common.multimodal_denoise_loop(X0(), st, ast, sig, ctx, None, nctx, nactx, mk(), mk())
    with pytest.raises(ValueError, match="stg_blocks"):
        common.multimodal_denoise_loop(X0(), st, ast, sig, ctx, actx, nctx, nactx, mk(stg_scale=1.0), mk())
    x = X0()
    x.velocity_model.is_av = False
    with pytest.raises(ValueError, match=r"requires an audio-video \(AV\) model"):
        common.multimodal_denoise_loop(x, st, ast, sig, ctx, actx, nctx, nactx, mk(), mk())
