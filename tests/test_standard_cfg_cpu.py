"""The guided standard one-stage loop without a GPU: the restatement on hand-checked numbers, the torch form that ships against it, how
generate_video(standard_cfg=True) routes and refuses, and the ABI."""
import contextlib
import inspect
import io
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import standard_cfg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
NEW_ENTRIES = {"ltx2_channel_guidance_stats_blocks": 2, "ltx2_channel_guidance_stats": 11, "ltx2_rescaled_guided_euler_step": 14,
               "ltx2_dit_rescaled_guided_step": 11, "ltx2_dit_graph_capture_rescaled_guided": 8, "ltx2_dit_set_cross_attn_scale": 3}


# ------------------------------------------------------------------ the restatement on numbers checked by hand
def test_rescale_gives_the_conditional_statistics_at_r_1():
    """Two channels, four rows, float64.  g has per-channel (mean, population std) (4, sqrt 5) and (10, sqrt 20), a has (1, sqrt 1.25) and
    (-2, sqrt 5): at r = 1 the output has a's mean and std per channel, up to the 1e-8 under the roots (relative 1e-8 / var <= 1e-8)."""
    g = torch.tensor([[1.0, 4.0], [3.0, 8.0], [5.0, 12.0], [7.0, 16.0]], dtype=torch.float64)
    a = torch.tensor([[-0.5, -5.0], [0.5, -3.0], [1.5, -1.0], [2.5, 1.0]], dtype=torch.float64)
    stats = torch.from_numpy(R.channel_stats64(g.numpy(), a.numpy()))
    assert np.allclose(stats[0], [4.0, 10.0]) and np.allclose(stats[2], [1.0, -2.0])
    assert np.allclose(stats[1] ** 2, [5.0 + 1e-8, 20.0 + 1e-8]) and np.allclose(stats[3] ** 2, [1.25 + 1e-8, 5.0 + 1e-8])
    out = R.rescale_noise_cfg(g, a, stats, 1.0)
    assert torch.allclose(out.mean(0), torch.tensor([1.0, -2.0], dtype=torch.float64), atol=1e-12)
    assert torch.allclose(out.var(0, unbiased=False), torch.tensor([1.25, 5.0], dtype=torch.float64), rtol=1e-7)
    # g is an affine image of a per channel here (g = 2a + 2 and 2a + 14), so the rescale lands on a itself
    assert torch.allclose(out, a, atol=1e-7)


def test_rescale_is_the_identity_at_r_0_and_blends_between():
    g = torch.tensor([[1.0, 4.0], [3.0, 8.0], [5.0, 12.0]])
    a = torch.tensor([[0.5, -5.0], [0.25, -3.0], [1.5, 1.0]])
    stats = torch.from_numpy(R.channel_stats64(g.numpy(), a.numpy())).float()
    assert torch.equal(R.rescale_noise_cfg(g, a, stats, 0.0), g)
    full, half = R.rescale_noise_cfg(g, a, stats, 1.0), R.rescale_noise_cfg(g, a, stats, 0.5)
    assert torch.allclose(half, 0.5 * full + 0.5 * g, atol=1e-6) and not torch.allclose(full, g, atol=1e-2)


def test_guidance_order_and_euler_step():
    """g = b + cfg*(a - b): 2 + 3*(5 - 2) = 11, not a + (cfg - 1)*(a - b) rounded otherwise; the step x + ((x - d)/sigma)*(sigma_next - sigma):
    x = 8, d = 4, sigma 0.5 -> 0.25: 8 + 8*(-0.25) = 6.  One step of the loop on a constant model reproduces both."""
    x, vc, vu = torch.tensor([[9.0]]), torch.tensor([[8.0]]), torch.tensor([[14.0]])
    a, g = R.guidance(x, vc, vu, torch.tensor([0.5]), 3.0)
    assert float(a) == 5.0 and float(g) == 11.0
    assert float(R.euler_x0(torch.tensor([[8.0]]), torch.tensor([[4.0]]), 0.5, 0.25)) == 6.0
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        R.euler_x0(x, x, 0.0, 0.0)
    out = R.standard_cfg_loop(torch.full((1, 3, 2), 8.0), lambda t, ts, s: torch.full_like(t, 5.0), lambda t, ts, s: torch.full_like(t, 2.0), [0.5, 0.25], 3.0, 0.0)
    assert torch.equal(out, torch.full((1, 3, 2), 8.0 + (8.0 - 11.0) / 0.5 * -0.25))
    assert torch.equal(R.rescaled_guided_euler_step(x, vc, vu, torch.tensor([0.5]), None, 3.0, 0.7, 0.5, 0.25), R.euler_x0(x, g, 0.5, 0.25))


def test_shipped_torch_form_equals_the_restatement():
    """pipelines.common.rescale_noise_cfg (the eager loop's statements, on (B, N, C)) against the restatement fed float64 statistics: fp32 means over
    37 rows differ from the float64 ones by a few ulp, and (g - mean)/std*std_a amplifies nothing here (std_a / std_g < 1): 1e-5 absolute on O(1) values."""
    from ltx_2_mlx_amd.pipelines import rescale_noise_cfg
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(1, 37, 6, generator=gen)
    g = 3.0 * a + torch.randn(1, 37, 6, generator=gen) + 0.5
    want = R.rescale_noise_cfg(g[0], a[0], torch.from_numpy(R.channel_stats64(g[0].numpy(), a[0].numpy())).float(), 0.7)
    assert float((rescale_noise_cfg(g, a, 0.7)[0] - want).abs().max()) < 1e-5
    assert torch.equal(rescale_noise_cfg(g, a, 0.0), g)


# ------------------------------------------------------------------ the loop's host side
class _FakeModel:
    is_av = False

    def __init__(self):
        self.calls, self.prepared = [], []

    def clone_sharing_weights(self):
        self.neg = _FakeModel()
        return self.neg

    def prepare(self, context, positions, per_token=False, audio_context=None, audio_positions=None):
        self.prepared.append((context, per_token))

    def rescaled_guided_step_(self, neg, lat, video, sigma, sigma_next, cfg_scale, guidance_rescale):
        self.calls.append(("step", neg is self.neg, sigma, sigma_next, cfg_scale, guidance_rescale, video.timesteps.numel()))

    def capture_rescaled_guided_graph(self, neg, lat, sigmas, cfg_scale, guidance_rescale):
        self.calls.append(("capture", neg is self.neg, list(sigmas), cfg_scale, guidance_rescale))

    def replay_rescaled_guided_graph(self):
        self.calls.append(("replay",))


def test_loop_call_order_and_refusals(monkeypatch):
    from ltx_2_mlx_amd.pipelines import common
    from ltx_2_mlx_amd.types import LatentState
    monkeypatch.setattr(common, "capture_and_replay", lambda capture, replay: (capture(), replay()))
    x = types.SimpleNamespace(velocity_model=_FakeModel())
    st = LatentState(latent=torch.zeros(1, 6, 8), denoise_mask=torch.ones(1, 6, 1), positions=torch.zeros(1, 3, 6, 2), clean_latent=torch.zeros(1, 6, 8))
    ctx, nctx, sig = torch.zeros(1, 4, 8), torch.ones(1, 4, 8), [1.0, 0.6, 0.3, 0.0]
    out = common.standard_cfg_denoise_loop(x, st, sig, ctx, nctx, 3.0, 0.7)
    m = x.velocity_model
    assert m.calls == [("capture", True, sig, 3.0, 0.7), ("replay",)] and out.latent.shape == (1, 6, 8)
    assert m.prepared == [(ctx, False)] and m.neg.prepared == [(nctx, False)]
    seen = []
    x = types.SimpleNamespace(velocity_model=_FakeModel())
    common.standard_cfg_denoise_loop(x, st, sig, ctx, nctx, 3.0, 0.0, callback=lambda i, n: seen.append((i, n)))
    assert [c[:6] for c in x.velocity_model.calls] == [("step", True, sig[i], sig[i + 1], 3.0, 0.0) for i in range(3)] and seen == [(1, 3), (2, 3), (3, 3)]
    assert all(c[6] == 1 for c in x.velocity_model.calls)                                          # uniform timesteps: the route has no conditioning
    with pytest.raises(ValueError, match="negative prompt"):
        common.standard_cfg_denoise_loop(x, st, sig, ctx, None, 3.0, 0.7)
    masked = st.replace(denoise_mask=torch.zeros(1, 6, 1))
    with pytest.raises(ValueError, match="no conditioning"):
        common.standard_cfg_denoise_loop(x, masked, sig, ctx, nctx, 3.0, 0.7)
    x.velocity_model.is_av = True
    with pytest.raises(ValueError, match="video-only"):
        common.standard_cfg_denoise_loop(x, st, sig, ctx, nctx, 3.0, 0.7)
    # cfg_scale <= 1: the existing unguided loop
    x.velocity_model.is_av = False
    hit = []
    monkeypatch.setattr(common, "joint_denoise_loop", lambda *a, **k: (hit.append(a[1:4] + a[7:]) or (st, None)))
    assert common.standard_cfg_denoise_loop(x, st, sig, ctx, nctx, 1.0, 0.7, None, False) is st and len(hit) == 1 and hit[0][0] is False


# ------------------------------------------------------------------ generate_video(standard_cfg=True)
def _call(tmp, **extra):
    """One generate_video call on test_generate_routes_cpu's stubs with the new loop replaced by a recorder -> (what it was given or the
    exception, the printed lines, the load calls that happened)."""
    import test_generate_routes_cpu as G
    from ltx_2_mlx_amd.pipelines import common
    kw = dict(use_gemma=False, device="cpu", save_mp4=False, output_path=os.path.join(tmp, "out", "o.mp4"), seed=7, height=64, width=64, num_frames=9,
              standard_cfg=True, model_variant="dev", cfg_scale=3.0, num_steps=4, vae_base_channels=16)
    kw.update(extra)
    seen, log = {}, []

    def loop(transformer, video_state, sigmas, context, negative_context, cfg_scale, guidance_rescale, callback=None, use_hip_graph=True, fused=True):
        seen.update(loop="standard_cfg", sigmas=list(sigmas), context=context, negative=negative_context, cfg_scale=cfg_scale, guidance_rescale=guidance_rescale,
                    use_hip_graph=use_hip_graph, fused=fused, mask_ones=bool((video_state.denoise_mask == 1).all()), tokens=tuple(video_state.latent.shape))
        return video_state

    out = io.StringIO()
    with pytest.MonkeyPatch.context() as mp:
        gen = G._stub_everything(mp, log, [], lambda s: s)
        stub_x0 = gen.X0Model

        def x0(transformer):
            m = stub_x0(transformer)
            m.velocity_model.set_cross_attn_scale = lambda scale, start_layer=40: seen.update(cross_attn=(scale, start_layer))
            return m

        mp.setattr(gen, "X0Model", x0)
        mp.setattr(common, "standard_cfg_denoise_loop", loop)
        with contextlib.redirect_stdout(out):
            try:
                seen["returned"] = gen.generate_video("a prompt", **kw)
            except Exception as e:  # noqa: BLE001
                seen["raised"] = e
    seen["loads"] = [c[0] for c in log if isinstance(c, list) and c[0] in ("load_transformer", "load_av_transformer", "create_vae_decoder", "create_dummy_text_encoding")]
    return seen, out.getvalue().splitlines()


def test_route_reaches_the_loop(tmp_path):
    import generate as gen
    tmp = str(tmp_path)
    seen, lines = _call(tmp)
    assert "raised" not in seen, seen.get("raised")
    assert seen["loop"] == "standard_cfg" and (seen["cfg_scale"], seen["guidance_rescale"]) == (3.0, 0.7) and seen["mask_ones"] and seen["fused"]
    assert seen["tokens"] == (1, 2 * 2 * 2, 128) and len(seen["sigmas"]) == 5 and seen["sigmas"][-1] == 0.0
    assert seen["negative"].shape == seen["context"].shape and not seen["negative"].any()             # no encoding given: zeros
    assert any("Negative prompt: no encoding given" in l for l in lines) and "  Standard CFG loop: cfg=3.0, guidance rescale=0.7" in lines
    assert "cross_attn" not in seen and os.path.exists(os.path.join(tmp, "out", "o_latent.npz")) and seen["returned"] is not None
    # the schedule is LTX2Scheduler's, not the distilled table
    from ltx_2_mlx_amd.components import LTX2Scheduler
    want = [float(s) for s in LTX2Scheduler().execute(steps=4, latent=torch.zeros(1, 128, 2, 2, 2))]
    assert seen["sigmas"] == pytest.approx(want)
    # the negative encoding of the embedding file, guidance_rescale, cross_attn_scale and the eager form
    emb = os.path.join(tmp, "emb.npz")
    np.savez(emb, embedding=np.ones((4, 16), np.float32), negative_embedding=np.full((4, 16), 2.0, np.float32))
    seen, lines = _call(tmp, embedding_path=emb, guidance_rescale=0.25, cross_attn_scale=1.5, use_hip_graph=False)
    assert "raised" not in seen, seen.get("raised")
    assert float(seen["negative"].mean()) == 2.0 and seen["guidance_rescale"] == 0.25 and seen["cross_attn"] == (1.5, 40) and seen["use_hip_graph"] is False
    assert any("cross-attention scale 1.5x" in l for l in lines)
    # registered as its own route
    assert gen._ROUTES["standard_cfg"] is gen._run_standard and gen._ROUTE_OWNS["standard_cfg"] == ("negative_prompt", "cross_attn_scale")
    assert "image_path" in gen._ROUTE_EXCLUDES["standard_cfg"][0] and list(gen._ROUTES)[0] == "two_stage_cfg"
    r = gen._resolve_request(dict({k: p.default for k, p in inspect.signature(gen.generate_video).parameters.items() if p.default is not inspect.Parameter.empty},
                                  prompt="p", standard_cfg=True, model_variant="dev", cfg_scale=3.0, use_gemma=False, device="cpu", height=64, width=64, num_frames=9,
                                  output_path=os.path.join(tmp, "o.mp4")))
    assert r.route == "standard_cfg" and not r.need_cfg and r.encode_negative and r.guidance_rescale == 0.7 and not r.av


def test_distilled_variant_is_forced_to_the_plain_loop(tmp_path):
    seen, lines = _call(str(tmp_path), model_variant="distilled", cfg_scale=3.0)
    assert "raised" not in seen, seen.get("raised")
    assert (seen["cfg_scale"], seen["guidance_rescale"]) == (1.0, 0.0)                                 # the loop takes its unguided branch at cfg <= 1
    assert any("the reference forces cfg = 1 and guidance_rescale = 0 for the distilled variant" in l for l in lines)
    assert "  Standard CFG loop: cfg=1.0" in lines and not any("Negative prompt" in l for l in lines)


REFUSED = [(dict(stg_scale=1.0), "stg_scale"), (dict(apg_scale=3.0), "apg_scale"), (dict(ge_gamma=0.5), "ge_gamma"), (dict(sampler="heun"), "sampler='heun'"),
           (dict(image_path="<img>"), "image_path with standard_cfg"), (dict(generate_audio=True), "generate_audio with standard_cfg"),
           (dict(audio_path="a.wav"), "audio_path with standard_cfg"), (dict(two_stage_distilled=True), "two_stage_distilled with standard_cfg"),
           (dict(keyframes=["<img>:0"]), "keyframes"), (dict(control_video="<ctl>"), "control_video"), (dict(retake_video="<clip>"), "retake_video with standard_cfg"),
           (dict(two_stage_cfg=True), "two_stage_cfg with standard_cfg"), (dict(model_version="2.3"), "LTX-2.3"), (dict(pipeline_type="two-stage"), "pipeline_type='two-stage'")]


@pytest.mark.parametrize("bad,text", REFUSED, ids=[next(iter(b)) for b, _ in REFUSED])
def test_stays_refused_before_any_model_loads(bad, text, tmp_path):
    import test_generate_routes_cpu as G
    paths = G._files(str(tmp_path))
    fill = lambda v: [fill(x) for x in v] if isinstance(v, list) else (next((v.replace(k, p) for k, p in paths.items() if k in v), v) if isinstance(v, str) else v)  # noqa: E731
    seen, _ = _call(str(tmp_path), **{k: fill(v) for k, v in bad.items()})
    assert isinstance(seen.get("raised"), NotImplementedError), seen
    assert text in str(seen["raised"]) and seen["loads"] == [] and "loop" not in seen


def test_without_the_keyword_the_pinned_refusal_is_unchanged(tmp_path):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "generate_routes.json")))
    want = gold["conflicts"]["standard-model_variant-cfg_scale"]["raised"]
    seen, _ = _call(str(tmp_path), standard_cfg=False)
    assert [type(seen["raised"]).__name__, str(seen["raised"])] == want and "classifier-free guidance is built in OneStagePipeline" in want[1]
    # elsewhere cross_attn_scale keeps its out-of-path text; the plain standard route honours it as the reference does
    seen, _ = _call(str(tmp_path), standard_cfg=False, generate_audio=True, decode_audio=False, model_variant="distilled", cross_attn_scale=2.0)
    assert str(seen["raised"]) == "cross_attn_scale=2.0 is outside the MI355X hot path (see DESIGN.md); leave it at its default 1.0"
    seen, lines = _call(str(tmp_path), standard_cfg=False, model_variant="distilled", cross_attn_scale=2.0)
    assert "raised" not in seen and seen["cross_attn"] == (2.0, 40) and "loop" not in seen


def test_cli_flag_and_keyword():
    import generate as gen
    sig = inspect.signature(gen.generate_video).parameters
    assert sig["standard_cfg"].kind is inspect.Parameter.KEYWORD_ONLY and sig["standard_cfg"].default is False and sig["guidance_rescale"].default == 0.7
    p = gen.build_parser()
    k = gen.kwargs_from_args(p.parse_args(["p", "--standard-cfg", "--model-variant", "dev", "--cfg", "3", "--cross-attn-scale", "1.5"]))
    assert k["standard_cfg"] is True and k["cross_attn_scale"] == 1.5 and k["guidance_rescale"] == 0.7 and k["model_variant"] == "dev"
    assert gen.kwargs_from_args(p.parse_args(["p"]))["standard_cfg"] is False


# ------------------------------------------------------------------ exports and the ABI
def test_exports_and_abi():
    import ltx_2_mlx_amd.pipelines as P
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import LTXModel
    for name in ("standard_cfg_denoise_loop", "rescale_noise_cfg"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    for name in ("set_cross_attn_scale", "rescaled_guided_step_", "capture_rescaled_guided_graph", "replay_rescaled_guided_graph"):
        assert callable(getattr(LTXModel, name)), name
    assert inspect.signature(LTXModel.set_cross_attn_scale).parameters["start_layer"].default == 40
    for name in ("channel_guidance_stats_blocks", "channel_guidance_stats", "rescaled_guided_euler_step"):
        assert callable(getattr(K, name)), name
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltx2hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+LTX2_ABI_VERSION\s+3\b", txt) and nv.ABI_VERSION == 3          # additive entries: no bump
    assert re.search(r"#define\s+LTX2_E_UNSUPPORTED\s+\(-4\)", txt) and nv.E_UNSUPPORTED == -4
    for name, n in NEW_ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, name
        assert len(m.group(1).split(",")) == n == len(nv.SIGNATURES[name][1]) and nv.SIGNATURES[name][0] is nv.i32, name
    if os.path.exists(nv.LIB_PATH):
        assert all(hasattr(nv.lib(), n) for n in NEW_ENTRIES)
