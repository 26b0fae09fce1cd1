"""The Euler-ancestral sampler without a GPU: the Philox restatement against the Random123 known-answer vectors, its statistics,
_get_ancestral_step against hand values, EulerAncestralDiffusionStep.step with a given noise against the formula, and the ABI."""
import os
import re

import numpy as np
import pytest
import torch

import ancestral_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["ltx2_philox_bits", "ltx2_philox_normal", "ltx2_ancestral_euler_step", "ltx2_ancestral_euler_step_pair", "ltx2_ancestral_euler_step_x0",
               "ltx2_dit_ancestral_step", "ltx2_dit_ancestral_step_joint_av", "ltx2_dit_graph_capture_ancestral",
               "ltx2_dit_graph_capture_ancestral_joint_av"]
SEEDS = [0, 42, 123456789012345]
N = 1 << 20


def test_philox_known_answer_vectors():
    for counter, key, want in R.KAT:
        assert tuple(int(v) for v in R.philox4x32_10(counter, key)[0]) == want, (counter, key)


def test_quad_bits_keys_the_counter_as_the_kernels_do():
    """quad q -> counter (lo32(q), hi32(q), step, stream), key (lo32(seed), hi32(seed)); a quad index past 2^32 reaches the second counter word.
    (ltx2_philox_bits takes no start offset, so that counter is checked here, on the restatement, and not on the device.)"""
    seed, q = 0x299F31D0A4093822, (0x85A308D3 << 32) | 0x243F6A88
    assert tuple(int(v) for v in R.quad_bits(q, 1, seed, 0x13198A2E, 0x03707344)[0]) == R.KAT[2][2]
    assert tuple(int(v) for v in R.quad_bits(0, 1, 0, 0, 0)[0]) == R.KAT[0][2]
    big = R.quad_bits((1 << 32) - 2, 4, 42, 7, 1)
    assert np.array_equal(big[2], R.philox4x32_10((0, 1, 7, 1), (42, 0))[0]) and len({tuple(r) for r in big.tolist()}) == 4


@pytest.fixture(scope="module")
def draws():
    """n = 2^20 float64 normals per (seed, step, stream), made once."""
    return {(s, st, sm): R.normals(N, s, st, sm) for s in SEEDS for st, sm in ((0, 0), (1, 0), (0, 1))}


@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_statistics(draws, seed):
    """Six standard errors over n = 2^20: |mean| < 6/sqrt(n), |var - 1| < 6 sqrt(2/n), |m4 - 3| < 6 sqrt(96/n), |corr| < 6/sqrt(n) between steps 0
    and 1 and between streams 0 and 1.  Deterministic for a fixed seed."""
    z = draws[(seed, 0, 0)]
    assert np.isfinite(z).all() and np.abs(z).max() < 5.8
    assert abs(z.mean()) < 5.9e-3 and abs(z.var() - 1) < 8.3e-3 and abs((z ** 4).mean() - 3) < 5.7e-2
    for other in ((seed, 1, 0), (seed, 0, 1)):
        assert abs(np.corrcoef(z, draws[other])[0, 1]) < 5.9e-3, other


def test_get_ancestral_step_hand_values():
    from ltx_2_mlx_amd.components import EulerAncestralDiffusionStep as S
    assert S._get_ancestral_step(1.0, 0.5, 0.0) == (0.0, 0.5)                       # eta = 0: the Euler step
    assert S._get_ancestral_step(0.7, 0.0, 1.0) == (0.0, 0.0)                       # the last step adds no noise
    up, down = S._get_ancestral_step(1.0, 0.6, 1.0)                                 # sqrt(0.36 * 0.64 / 1) = 0.48, sqrt(0.36 - 0.2304) = 0.36
    assert abs(up - 0.48) < 1e-15 and abs(down - 0.36) < 1e-15
    up, down = S._get_ancestral_step(1.0, 0.6, 2.0)                                 # 2 * 0.48 = 0.96 > sigma_to: clamped, nothing left to step down to
    assert up == 0.6 and down == 0.0
    for args in ((1.0, 0.6, 1.0), (0.909375, 0.725, 0.5), (1.0, 0.6, 2.0)):
        assert S._get_ancestral_step(*args) == pytest.approx(R.ancestral_sigmas(*args), abs=1e-15)
        up, down = S._get_ancestral_step(*args)
        assert abs(up ** 2 + down ** 2 - args[1] ** 2) < 1e-15                      # the variance of the target sigma is kept


def test_step_with_given_noise_is_the_formula():
    """torch CPU, fp32: x + ((x - x0)/sigma)*(sigma_down - sigma) + noise*sigma_up.  Four fp32 operations on values below 8 in magnitude against
    the float64 formula: within 4 * 0.5 ulp at 8, 4 * 4.8e-7 / 2 -- gated at 4 ulp of [4, 8), 1.9e-6."""
    from ltx_2_mlx_amd.components import EulerAncestralDiffusionStep
    g = torch.Generator().manual_seed(5)
    x, x0, noise = (torch.randn(1, 35, 128, generator=g) for _ in range(3))
    sig = [0.909375, 0.725, 0.0]
    for eta in (1.0, 0.5, 0.0):
        got = EulerAncestralDiffusionStep(eta=eta).step(x, x0, sig, 0, noise=noise)
        want = R.ancestral_step(x.double().numpy(), x0.double().numpy(), sig[0], sig[1], noise.double().numpy(), eta)
        assert got.dtype == torch.float32 and float(np.abs(got.double().numpy() - want).max()) <= 4 * 4.8e-7, eta
    last = EulerAncestralDiffusionStep().step(x, x0, sig, 1, noise=noise)           # sigma_next = 0: lands on x0, no noise
    assert float((last - x0).abs().max()) <= 4 * 4.8e-7
    euler = EulerAncestralDiffusionStep(eta=0.0).step(x, x0, sig, 0, noise=noise)
    assert float((euler - (x + (x - x0) / sig[0] * (sig[1] - sig[0]))).abs().max()) <= 4 * 4.8e-7


def test_abi_lists_the_new_entries():
    from ltx_2_mlx_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    for name in NEW_ENTRIES:
        assert name in nv.SIGNATURES and re.search(r"\bint %s\(" % name, header), name
    assert nv.ABI_VERSION == 3 and "#define LTX2_ABI_VERSION 3" in header
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.pipelines.common import ancestral_denoise_loop  # noqa: F401
    for fn in ("philox_bits", "philox_normal", "ancestral_euler_step", "ancestral_euler_step_pair", "ancestral_euler_step_x0"):
        assert callable(getattr(K, fn))


# ------------------------------------------------------------------ OneStagePipeline's own routing
def test_one_stage_pipeline_routes_and_refuses(monkeypatch):
    import ltx_2_mlx_amd.pipelines.one_stage as one_stage
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider, LtxAPGGuider
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig
    from test_heun_cpu import _stub_pipe
    pipe = _stub_pipe()
    enc = torch.zeros(1, 4, 8)
    plain = OneStageCFGConfig(height=64, width=96, num_frames=9, rescale_scale=0.0, seed=11)
    with pytest.raises(ValueError, match="sampler='dpm'"):
        pipe(enc, enc, plain, sampler="dpm")
    refusals = ((dict(stg_scale=1.0), "STG"), (dict(ge_gamma=2.0), "GE velocity"), (dict(cross_attn_scale=2.0), "cross_attn_scale"),
                (dict(temporal_upscaler=object()), "temporal upscaler"), (dict(guider_override=LtxAPGGuider(3.0, 0.5, 5.0)), "CFG\\* / APG"),
                (dict(guider_override=CFGStarRescalingGuider(3.0)), "CFG\\* / APG"))
    for kw, text in refusals:
        with pytest.raises(NotImplementedError, match=text):
            pipe(enc, enc, plain, sampler="euler_ancestral", **kw)
    with pytest.raises(NotImplementedError, match="CFG\\*"):                  # the config default: CFG*
        pipe(enc, enc, OneStageCFGConfig(height=64, width=96, num_frames=9), sampler="euler_ancestral")
    with pytest.raises(ValueError, match="ancestral_eta"):
        pipe(enc, enc, plain, sampler="euler_ancestral", ancestral_eta=-1.0)
    seen = []

    def loop(transformer, video_state, audio_state, sigmas, vctx, actx, nvctx, nactx, cfg_scale, audio_cfg_scale, eta, seed, callback, use_hip_graph):
        seen.append((cfg_scale, audio_cfg_scale, eta, seed, nvctx is not None, audio_state is None, len(sigmas)))
        return video_state, audio_state

    monkeypatch.setattr(one_stage, "ancestral_denoise_loop", loop)
    monkeypatch.setattr(one_stage, "decode_video", lambda latent, decoder, tiling: latent)
    pipe.patchifier, pipe.video_encoder, pipe.video_decoder = one_stage.VideoLatentPatchifier(patch_size=1), None, None
    pipe.scheduler, pipe.diffusion_step = one_stage.LTX2Scheduler(), None
    pipe(enc, enc, plain, sampler="euler_ancestral")
    pipe(enc, enc, plain, sampler="euler_ancestral", ancestral_eta=0.5, guider_override=CFGGuider(5.0))
    pipe(enc, None, OneStageCFGConfig(height=64, width=96, num_frames=9, cfg_scale=1.0, seed=3), sampler="euler_ancestral")      # no guidance: CFG* at scale 1 is off
    assert seen == [(3.0, 1.0, 1.0, 11, True, True, 31), (5.0, 1.0, 0.5, 11, True, True, 31), (1.0, 1.0, 1.0, 3, False, True, 31)]


# ------------------------------------------------------------------ generate_video(sampler="euler_ancestral", ancestral_eta=...)
def _call(tmp, route, **extra):
    """test_projected_guidance_cpu's _call with DistilledPipeline recorded too -> (pipeline, its kwargs, its config, or the exception; the printed lines)."""
    import contextlib
    import io
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import test_generate_routes_cpu as G
    import ltx_2_mlx_amd.pipelines as P
    paths = G._files(tmp)
    fill = lambda v: next((v.replace(k, p) for k, p in paths.items() if k in v), v) if isinstance(v, str) else v          # noqa: E731
    kw = dict(use_gemma=False, device="cpu", save_mp4=False, output_path=os.path.join(tmp, "out", "o.mp4"), seed=7)
    kw.update({k: fill(v) for k, v in dict(G.ROUTES[route], **extra).items()})
    seen = {}

    def recorder(name):
        class Pipe:
            def __init__(self, *a, **k):
                pass

            def __call__(self, *a, **k):
                conf = next(v for v in list(a) + list(k.values()) if type(v).__name__.endswith("Config"))
                seen.update(pipeline=name, kwargs=k, config=conf)
                frames = torch.zeros(conf.num_frames, conf.height, conf.width, 3, dtype=torch.uint8)
                return (frames, None) if name == "DistilledPipeline" else (frames, torch.zeros(1, 8, 3, 16))
        return Pipe

    out = io.StringIO()
    with pytest.MonkeyPatch.context() as mp:
        gen = G._stub_everything(mp, [], [], lambda s: s)
        for name in ("OneStagePipeline", "DistilledPipeline"):
            mp.setattr(P, name, recorder(name))
        with contextlib.redirect_stdout(out):
            try:
                gen.generate_video("a prompt", **kw)
            except Exception as e:  # noqa: BLE001
                seen["raised"] = e
    return seen, out.getvalue().splitlines()


def test_generate_video_reaches_the_two_pipelines(tmp_path):
    tmp = str(tmp_path)
    seen, lines = _call(tmp, "av", sampler="euler_ancestral", ancestral_eta=0.7, model_variant="distilled")
    assert "raised" not in seen, seen
    assert seen["pipeline"] == "OneStagePipeline" and (seen["kwargs"]["sampler"], seen["kwargs"]["ancestral_eta"]) == ("euler_ancestral", 0.7)
    assert seen["config"].seed == 7                                                       # the noise seed is `seed` itself
    assert [l for l in lines if l.startswith("Sampler")] == ["Sampler: euler_ancestral, eta=0.7 (noise seed 7, made in the step kernel)"]
    seen, _ = _call(tmp, "av", model_variant="distilled")                                 # the default changes nothing
    assert "sampler" not in seen["kwargs"] and "ancestral_eta" not in seen["kwargs"]
    seen, lines = _call(tmp, "two_stage", sampler="euler_ancestral", ancestral_eta=0.5)
    assert "raised" not in seen, seen
    assert seen["pipeline"] == "DistilledPipeline" and (seen["config"].sampler, seen["config"].ancestral_eta, seen["config"].seed) == ("euler_ancestral", 0.5, 7)
    assert [l for l in lines if l.startswith("Sampler")] == ["Sampler: euler_ancestral, eta=0.5 (noise seed 7, made in the step kernel)"]
    seen, _ = _call(tmp, "two_stage")
    assert (seen["config"].sampler, seen["config"].ancestral_eta) == ("euler", 1.0)


@pytest.mark.parametrize("route", ["standard", "keyframe", "retake", "hq", "ic_lora"])
def test_generate_video_refuses_it_on_the_other_routes(route, tmp_path):
    seen, _ = _call(str(tmp_path), route, sampler="euler_ancestral")
    assert isinstance(seen.get("raised"), NotImplementedError) and "sampler='euler_ancestral'" in str(seen["raised"]) and "pipeline" not in seen, seen


def test_generate_video_refuses_it_beside_each_excluded_option(tmp_path):
    tmp = str(tmp_path)
    for extra in (dict(stg_scale=1.0), dict(stg_audio_scale=1.0), dict(ge_gamma=0.5), dict(apg_scale=3.0), dict(cross_attn_scale=2.0)):
        seen, _ = _call(tmp, "av", sampler="euler_ancestral", model_variant="distilled", **extra)
        assert isinstance(seen.get("raised"), NotImplementedError) and "pipeline" not in seen, (extra, seen)
        assert list(extra)[0] in str(seen["raised"]), (extra, seen["raised"])
    emb = os.path.join(tmp, "emb.npz")
    np.savez(emb, **{k: np.ones((4, 16), np.float32) for k in ("embedding", "audio_embedding", "negative_embedding", "negative_audio_embedding")})
    seen, _ = _call(tmp, "av", sampler="euler_ancestral", embedding_path=emb, model_variant="dev", cfg_scale=3.0)              # the dev variant's default guidance is CFG*
    assert isinstance(seen.get("raised"), NotImplementedError) and "CFG*" in str(seen["raised"])
    seen, _ = _call(tmp, "av", sampler="euler_ancestral", embedding_path=emb, model_variant="dev", cfg_scale=3.0, rescale_scale=0.0)      # plain CFG: runs
    assert "raised" not in seen and seen["kwargs"]["sampler"] == "euler_ancestral", seen
    seen, _ = _call(tmp, "av", sampler="dpm", model_variant="distilled")
    assert isinstance(seen.get("raised"), ValueError) and "sampler='dpm'" in str(seen["raised"])
    seen, _ = _call(tmp, "av", ancestral_eta=0.5, model_variant="distilled")               # eta without its sampler
    assert isinstance(seen.get("raised"), ValueError) and "ancestral_eta" in str(seen["raised"])
    seen, _ = _call(tmp, "av", sampler="euler_ancestral", ancestral_eta=-1.0, model_variant="distilled")
    assert isinstance(seen.get("raised"), ValueError) and "ancestral_eta" in str(seen["raised"])


def test_cli_and_signature():
    import inspect
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate as gen
    p = gen.build_parser()
    k = gen.kwargs_from_args(p.parse_args(["p", "--generate-audio", "--sampler", "euler_ancestral", "--ancestral-eta", "0.5"]))
    assert (k["sampler"], k["ancestral_eta"]) == ("euler_ancestral", 0.5)
    k = gen.kwargs_from_args(p.parse_args(["p"]))
    assert (k["sampler"], k["ancestral_eta"]) == ("euler", 1.0)
    with pytest.raises(SystemExit):
        p.parse_args(["p", "--sampler", "dpm"])
    params = inspect.signature(gen.generate_video).parameters
    names = list(params)
    # keyword-only, beside `sampler` among the MI355X additions: tests/test_retake_cpu.py pins the four retake keywords as the signature's last
    assert names[names.index("sampler") + 1] == "ancestral_eta" and params["ancestral_eta"].kind is inspect.Parameter.KEYWORD_ONLY and params["ancestral_eta"].default == 1.0
    assert names[:4] == ["prompt", "height", "width", "num_frames"] and names.index("negative_prompt") < names.index("stg_blocks")        # the pinned prefix is intact
