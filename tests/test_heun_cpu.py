"""The Heun sampler and the GE velocity correction without a GPU: the restatement and HeunDiffusionStep against vectors recorded from the
reference, the order of accuracy, what GE does, how generate_video and OneStagePipeline route and refuse, and the ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import heun_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
NEW_ENTRIES = ["ltx2_heun_predict", "ltx2_heun_correct", "ltx2_ge_euler_step", "ltx2_heun_predict_pair", "ltx2_heun_correct_pair", "ltx2_ge_euler_step_pair",
               "ltx2_dit_heun_step", "ltx2_dit_heun_step_av", "ltx2_dit_ge_step", "ltx2_dit_graph_capture_heun"]
ULP4 = 4.8e-7          # the spacing of fp32 numbers in [4, 8): every value of the golden chains is below 8 in magnitude


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "heun_ge.npz")) as z:
        return {k: (torch.from_numpy(z[k]) if z[k].ndim else float(z[k])) for k in z.files}


# ------------------------------------------------------------------ the reference's own vectors
def test_heun_diffusion_step_reproduces_the_reference(gold):
    """HeunDiffusionStep.step on the recorded inputs.  The chain is (x - d)/s, *dt, +x and for the corrector (xp - d2)/s', +, *0.5, *dt, +x: at
    most 8 operations, each within half an ulp of its own result and none amplified (|dt| <= s, the velocities are added then halved), so the
    result is within 8 * 0.5 ulp = 4 ulp of the reference's; the bound is 4 ulp at the largest magnitude, 4 * 4.8e-7."""
    from ltx_2_mlx_amd.components import HeunDiffusionStep
    assert max(float(gold[k].abs().max()) for k in ("step_sample", "step_predicted", "step_result")) < 8.0
    step, sig = HeunDiffusionStep(), [float(s) for s in gold["step_sigmas"]]
    pred = step.step(gold["step_sample"], gold["step_denoised"], sig, 0)
    full = step.step(gold["step_sample"], gold["step_denoised"], sig, 0, denoised_at_predicted=gold["step_denoised_at_predicted"])
    last = step.step(gold["step_sample"], gold["step_denoised_last"], sig, 1)                      # sigma_next = 0: the predictor lands on the x0
    for got, want in ((pred, "step_predicted"), (full, "step_result"), (last, "step_result_to_zero")):
        assert float((got - gold[want]).abs().max()) <= 4 * ULP4, want
    assert float((last - gold["step_denoised_last"]).abs().max()) <= 4 * ULP4
    assert not torch.equal(pred, full)


def test_restatement_reproduces_the_reference_loops(gold):
    """tests/heun_ref.py over the closed-form denoiser against _denoise_loop_heun (without and with GE) and _denoise_loop_cfg with GE, 4 steps, a
    mask of 0, 0.1 and 1, CFG 3, ge_gamma 2.  Per evaluation about 25 fp32 operations (the denoiser's 5, x0 formation and guidance 6, GE 7,
    the blend 4, the step 4), two evaluations per Heun step, 4 steps: 200 operations at half an ulp each, none amplified beyond 1 (tanh' <= 1,
    |w * t| < 1, |dt| <= sigma) except GE's gamma = 2 on the velocity difference, which doubles what the three steps before it left: a bound of
    200 * 0.5 * 2 = 200 ulp at magnitude < 8, 200 * 4.8e-7 = 9.6e-5."""
    w, bias = gold["w"], gold["bias"]
    x0_pos, x0_neg = R.closed_form_x0(w, bias), R.closed_form_x0(w, bias * gold["neg_bias"])
    sig = [float(s) for s in gold["sigmas"]]
    assert sig[-1] == 0.0 and len(sig) == 5
    for name, heun, gamma in (("heun", True, 0.0), ("heun_ge", True, gold["ge_gamma"]), ("euler_ge", False, gold["ge_gamma"])):
        got = R.video_loop(heun, gold["latent"], gold["mask"], gold["clean"], x0_pos, x0_neg, sig, gold["cfg_scale"], gamma)
        want = gold["result_" + name]
        assert float(want.abs().max()) < 8.0
        assert float((got - want).abs().max()) <= 200 * ULP4, name
    assert torch.equal(gold["result_heun"][:, :4], gold["clean"][:, :4])                          # mask 0: the last step ends on the clean tokens
    assert not torch.allclose(gold["result_heun"], gold["result_heun_ge"], atol=1e-3)


# ------------------------------------------------------------------ order of accuracy
def _endpoint_error(heun, x0_of_x, n, exact):
    sig = torch.linspace(1.0, 0.25, n + 1, dtype=torch.float64).tolist()
    x = torch.ones(1, 1, 1, dtype=torch.float64)
    mask = torch.ones(1, 1, 1, dtype=torch.float64)
    out = R.video_loop(heun, x, mask, torch.zeros_like(x), lambda x, ts, s: x0_of_x(x), None, sig, 1.0)
    return abs(float(out) - exact)


def test_order_of_accuracy():
    """fp64, sigma from 1 to 0.25 in 8, 16 and 32 equal steps.  On x0 = 0 the ODE dx/dsigma = x/sigma has the solution x = sigma, a straight
    line, which the Euler step follows exactly: both loops land on 0.25 to round-off and their error ratios say nothing, so that problem checks
    exactness.  The order shows on x0 = x/2, dx/dsigma = x/(2 sigma), x = sqrt(sigma): halving the step cuts Heun's error by more than 3 (theory:
    4) and Euler's by less than 2.5 (theory: 2)."""
    for heun in (False, True):
        for n in (8, 16, 32):
            assert _endpoint_error(heun, lambda x: torch.zeros_like(x), n, 0.25) < 1e-14, (heun, n)
    err = {heun: [_endpoint_error(heun, lambda x: 0.5 * x, n, 0.5) for n in (8, 16, 32)] for heun in (False, True)}
    for a, b in ((0, 1), (1, 2)):
        assert err[True][a] / err[True][b] > 3.0, err
        assert 1.5 < err[False][a] / err[False][b] < 2.5, err
    assert all(h < e for h, e in zip(err[True], err[False]))


def test_order_of_accuracy_of_the_shipped_loop():
    """The same ratios through the code that ships, in fp32 (HeunDiffusionStep computes in fp32): heun_denoise_loop(fused=False) over a stub X0
    model x0 = x/2, and for the first-order side HeunDiffusionStep.step without its corrector, which is the Euler step.  At 32 steps Heun's error is
    1.3e-4, some 50 x the fp32 round-off 32 steps accumulate, so the ratios stand as in fp64."""
    from ltx_2_mlx_amd.components import HeunDiffusionStep
    from ltx_2_mlx_amd.pipelines.common import heun_denoise_loop
    from ltx_2_mlx_amd.types import LatentState

    class Half:          # stands where X0Model stands: Modality -> x0
        velocity_model = type("M", (), {"is_av": False})()

        def __call__(self, video):
            return 0.5 * video.latent

    def table(n):
        return torch.linspace(1.0, 0.25, n + 1, dtype=torch.float64).tolist()

    def heun_error(n):
        st = LatentState(latent=torch.ones(1, 1, 1), denoise_mask=torch.ones(1, 1, 1), positions=torch.zeros(1, 3, 1, 2), clean_latent=torch.zeros(1, 1, 1))
        out, _ = heun_denoise_loop(Half(), st, None, table(n), torch.zeros(1, 1, 1), None, None, None, None, fused=False)
        return abs(float(out.latent) - 0.5)

    def euler_error(n):
        x, sig, step = torch.ones(1, 1, 1), table(n), HeunDiffusionStep()
        for i in range(n):
            x = step.step(x, 0.5 * x, sig, i)
        return abs(float(x) - 0.5)

    heun, euler = [heun_error(n) for n in (8, 16, 32)], [euler_error(n) for n in (8, 16, 32)]
    for a, b in ((0, 1), (1, 2)):
        assert heun[a] / heun[b] > 3.0, heun
        assert 1.5 < euler[a] / euler[b] < 2.5, euler
    assert all(h < e for h, e in zip(heun, euler))


# ------------------------------------------------------------------ GE
def test_ge_properties(gold):
    w, bias = gold["w"], gold["bias"]
    x0_pos, x0_neg = R.closed_form_x0(w, bias), R.closed_form_x0(w, bias * gold["neg_bias"])
    sig = [float(s) for s in gold["sigmas"]]
    args = (gold["latent"], gold["mask"], gold["clean"], x0_pos, x0_neg)
    plain = [R.video_loop(False, *args, sig[:k + 1] if k < 4 else sig, 3.0) for k in (1, 2, 3, 4)]
    # the first step only stores the velocity: one step with GE is one step of plain Euler, bit for bit
    assert torch.equal(R.video_loop(False, *args, sig[:2], 3.0, 2.0), plain[0])
    assert not torch.allclose(R.video_loop(False, *args, sig[:3], 3.0, 2.0), plain[1], atol=1e-4)
    # gamma = 1: tot = (cur - prev) + prev = cur up to an ulp of the velocities, x - tot*sigma = the guided x0 up to a few ulp: plain Euler on every step
    for k in (2, 3, 4):
        got = R.video_loop(False, *args, sig[:k + 1] if k < 4 else sig, 3.0, 1.0)
        assert float((got - plain[k - 1]).abs().max()) <= 16 * k * ULP4, k
    # prev holds the UNcorrected velocity: (x - guided x0)/sigma of each step's own latent, whatever the step then did with it
    trace = []
    R.video_loop(False, *args, sig, 3.0, 2.0, trace)
    x = gold["latent"].float()
    for i in range(3):
        s = sig[i]
        ts = gold["mask"] * s
        a, b = x0_pos(x, ts, s), x0_neg(x, ts, s)
        assert torch.equal(trace[i][0], (x - (a + (3.0 - 1) * (a - b))) / s), i
        x = x + ((x - trace[i][1]) / s) * (sig[i + 1] - s)
    # on the Heun loop GE acts on the first evaluation alone: with one step to sigma_next > 0 it changes nothing
    assert torch.equal(R.video_loop(True, *args, sig[:2], 3.0, 2.0), R.video_loop(True, *args, sig[:2], 3.0))


# ------------------------------------------------------------------ OneStagePipeline's own routing
def _stub_pipe():
    from ltx_2_mlx_amd.pipelines import OneStagePipeline

    class Stub:
        num_layers = 4
        device = torch.device("cpu")
    pipe = OneStagePipeline.__new__(OneStagePipeline)
    pipe.transformer, pipe.is_av_model = type("X", (), {"velocity_model": Stub()})(), False
    return pipe


def test_one_stage_pipeline_routes_and_refuses(monkeypatch):
    import ltx_2_mlx_amd.pipelines.one_stage as one_stage
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider, LtxAPGGuider
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    gate = OneStagePipeline._require_no_guidance
    for bad, text in ((dict(ge_gamma=2.0), "GE velocity"), (dict(sampler="heun"), "sampler='heun'"), (dict(cross_attn_scale=2.0), "cross_attn_scale"),
                      (dict(stg_scale=1.0), "STG"), (dict(temporal_upscaler=object()), "temporal upscaler")):
        a = dict(stg_scale=0.0, guider_override=None, ge_gamma=0.0, sampler="euler", temporal_upscaler=None, cross_attn_scale=1.0)
        a.update(bad)
        with pytest.raises(NotImplementedError, match=text):                  # the gate itself is as it was
            gate(**a)
    pipe = _stub_pipe()
    conf = OneStageCFGConfig(height=64, width=96, num_frames=9)
    enc = torch.zeros(1, 4, 8)
    with pytest.raises(ValueError, match="sampler='dpm'"):
        pipe(enc, enc, conf, sampler="dpm")
    for kw, text in ((dict(stg_scale=1.0, ge_gamma=0.5), "GE velocity"), (dict(stg_scale=1.0, sampler="heun"), "sampler='heun'"),
                     (dict(sampler="heun", cross_attn_scale=2.0), "cross_attn_scale"), (dict(ge_gamma=2.0, temporal_upscaler=object()), "temporal upscaler")):
        with pytest.raises(NotImplementedError, match=text):
            pipe(enc, enc, conf, **kw)
    # which loop, and which form of it
    seen = []

    def recorder(name):
        def loop(transformer, video_state, audio_state, sigmas, vctx, actx, nvctx, nactx, video_guider, audio_guider, ge_gamma, callback, use_hip_graph, fused):
            seen.append((name, type(video_guider).__name__, ge_gamma, fused, nvctx is not None))
            return video_state, audio_state
        return loop

    monkeypatch.setattr(one_stage, "heun_denoise_loop", recorder("heun"))
    monkeypatch.setattr(one_stage, "ge_denoise_loop", recorder("ge"))
    monkeypatch.setattr(one_stage, "decode_video", lambda latent, decoder, tiling: latent)
    pipe.patchifier, pipe.video_encoder, pipe.video_decoder = one_stage.VideoLatentPatchifier(patch_size=1), None, None
    pipe.scheduler, pipe.diffusion_step = one_stage.LTX2Scheduler(), None
    plain = OneStageCFGConfig(height=64, width=96, num_frames=9, rescale_scale=0.0)
    pipe(enc, enc, plain, sampler="heun")
    pipe(enc, enc, plain, sampler="heun", ge_gamma=2.0)
    pipe(enc, enc, plain, ge_gamma=2.0)
    pipe(enc, enc, conf, sampler="heun")                                      # the config default: CFG*
    pipe(enc, enc, plain, sampler="heun", guider_override=LtxAPGGuider(3.0, 0.5, 5.0))
    pipe(enc, None, OneStageCFGConfig(height=64, width=96, num_frames=9, cfg_scale=1.0, rescale_scale=0.0), sampler="heun", ge_gamma=-1.0)
    assert seen == [("heun", "CFGGuider", 0.0, True, True), ("heun", "CFGGuider", 2.0, True, True), ("ge", "CFGGuider", 2.0, True, True),
                    ("heun", "CFGStarRescalingGuider", 0.0, False, True), ("heun", "LtxAPGGuider", 0.0, False, True),
                    ("heun", "CFGGuider", 0.0, True, False)]
    assert CFGGuider(1.0).enabled() is False and CFGStarRescalingGuider(3.0).enabled()


def test_device_form_is_for_plain_cfg():
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider, LegacyStatefulAPGGuider
    from ltx_2_mlx_amd.pipelines.common import heun_device_form
    assert heun_device_form(CFGGuider(3.0)) and heun_device_form(CFGGuider(3.0), CFGGuider(7.0)) and heun_device_form(None, None)
    assert heun_device_form(CFGStarRescalingGuider(1.0))                     # not enabled: no guidance at all
    assert not heun_device_form(CFGStarRescalingGuider(3.0)) and not heun_device_form(CFGGuider(3.0), CFGStarRescalingGuider(7.0))
    assert not heun_device_form(LegacyStatefulAPGGuider(2.0, 0.5, 4.0, 0.25))


def test_exports():
    import ltx_2_mlx_amd.components as C
    import ltx_2_mlx_amd.pipelines as P
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import LTXModel
    assert "HeunDiffusionStep" in C.__all__ and callable(C.HeunDiffusionStep().step)
    for name in ("heun_denoise_loop", "ge_denoise_loop"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    for name in ("heun_step_", "heun_step_av_", "ge_step_", "capture_heun_graph", "replay_heun_graph"):
        assert callable(getattr(LTXModel, name)), name
    for name in ("heun_predict", "heun_correct", "ge_euler_step", "heun_predict_pair", "heun_correct_pair", "ge_euler_step_pair"):
        assert callable(getattr(K, name)), name


def test_abi_declares_the_heun_entries():
    from ltx_2_mlx_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    assert re.search(r"#define LTX2_ABI_VERSION 3\b", header) and nv.ABI_VERSION == 3          # additive entries: no bump
    for name in NEW_ENTRIES:
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S)
        assert decl, name
        assert name in nv.SIGNATURES and nv.SIGNATURES[name][0] is nv.i32, name
        assert len(decl.group(1).split(",")) == len(nv.SIGNATURES[name][1]), name
    if os.path.exists(nv.LIB_PATH):
        assert all(hasattr(nv.lib(), n) for n in NEW_ENTRIES)


# ------------------------------------------------------------------ generate_video(sampler=..., ge_gamma=...)
def _call(tmp, route, **extra):
    from test_projected_guidance_cpu import _call as call
    return call(tmp, route, **extra)


def _negatives(tmp):
    emb = os.path.join(tmp, "emb.npz")
    np.savez(emb, **{k: np.ones((4, 16), np.float32) for k in ("embedding", "audio_embedding", "negative_embedding", "negative_audio_embedding")})
    return emb


def test_sampler_and_ge_gamma_reach_one_stage_pipeline(tmp_path):
    import generate as gen
    tmp = str(tmp_path)
    assert "ge_gamma" in gen._ROUTE_OWNS["av"] and all("ge_gamma" not in v for k, v in gen._ROUTE_OWNS.items() if k != "av")
    seen, lines = _call(tmp, "av", sampler="heun", ge_gamma=2.0, model_variant="distilled")
    assert "raised" not in seen, seen
    k = seen["kwargs"]
    assert seen["pipeline"] == "OneStagePipeline" and (k["sampler"], k["ge_gamma"]) == ("heun", 2.0)
    assert [l for l in lines if "Sampler" in l] == ["Sampler: heun (2x model evals per step), GE gamma=2.0"]
    seen, lines = _call(tmp, "av", ge_gamma=0.5, embedding_path=_negatives(tmp))                  # the dev variant: guided
    assert "raised" not in seen and (seen["kwargs"]["sampler"], seen["kwargs"]["ge_gamma"]) == ("euler", 0.5)
    assert [l for l in lines if "Sampler" in l] == ["Sampler: euler, GE gamma=0.5"]
    seen, lines = _call(tmp, "av", sampler="heun", model_variant="distilled")
    assert (seen["kwargs"]["sampler"], seen["kwargs"]["ge_gamma"]) == ("heun", 0.0)
    seen, lines = _call(tmp, "av", model_variant="distilled")                                     # without either: no keyword, no line
    assert "sampler" not in seen["kwargs"] and "ge_gamma" not in seen["kwargs"] and not [l for l in lines if "Sampler" in l]
    # beside STG both stay refused, GE with its out-of-path text
    seen, _ = _call(tmp, "av", stg_scale=1.0, ge_gamma=0.5, model_variant="distilled")
    assert isinstance(seen.get("raised"), NotImplementedError) and "ge_gamma=0.5 is outside the MI355X hot path" in str(seen["raised"])
    seen, _ = _call(tmp, "av", stg_scale=1.0, sampler="heun", model_variant="distilled")
    assert isinstance(seen.get("raised"), NotImplementedError) and "sampler='heun'" in str(seen["raised"])
    seen, _ = _call(tmp, "av", sampler="dpm", model_variant="distilled")
    assert isinstance(seen.get("raised"), ValueError) and "sampler='dpm'" in str(seen["raised"])
    seen, _ = _call(tmp, "av", sampler="heun", cross_attn_scale=2.0, model_variant="distilled")
    assert isinstance(seen.get("raised"), NotImplementedError) and "cross_attn_scale=2.0" in str(seen["raised"])


@pytest.mark.parametrize("route", ["standard", "keyframe", "retake", "hq", "ic_lora", "two_stage"])
def test_sampler_and_ge_gamma_stay_refused_off_the_av_route(route, tmp_path):
    seen, _ = _call(str(tmp_path), route, ge_gamma=0.5)
    assert isinstance(seen.get("raised"), NotImplementedError), seen
    assert str(seen["raised"]) == "ge_gamma=0.5 is outside the MI355X hot path (see DESIGN.md); leave it at its default 0.0"
    seen, _ = _call(str(tmp_path), route, sampler="heun")
    assert isinstance(seen.get("raised"), NotImplementedError) and "sampler='heun'" in str(seen["raised"]) and "pipeline" not in seen


def test_cli_passes_the_sampler_flag():
    import inspect
    import generate as gen
    p = gen.build_parser()
    a = p.parse_args(["p", "--generate-audio", "--sampler", "heun", "--ge-gamma", "2"])
    k = gen.kwargs_from_args(a)
    assert (k["sampler"], k["ge_gamma"]) == ("heun", 2.0)
    assert gen.kwargs_from_args(p.parse_args(["p"]))["sampler"] == "euler"
    with pytest.raises(SystemExit):
        p.parse_args(["p", "--sampler", "dpm"])
    sig = inspect.signature(gen.generate_video).parameters["sampler"]
    assert sig.kind is inspect.Parameter.KEYWORD_ONLY and sig.default == "euler"
