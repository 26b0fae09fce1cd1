"""The res_2s sampler and the HQ pipeline, the parts that need no GPU: the coefficients and the loop restatement against the vectors
recorded from the reference (tests/golden/res2s_coefficients.json, res2s_loop_tiny.npz, tools/pin_res2s_against_reference.py), the sigma
handling, the config, generate_video's routing, the LoRA fuse-and-restore and the four new ABI entries."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import res2s_ref as R  # noqa: E402

LOOP_GATE = 5 * 1.431e-6      # 5 x the largest maximum absolute difference measured (see test_restatement_loop_equals_the_reference)
NEW_ENTRIES = ("ltx2_res2s_midpoint", "ltx2_res2s_combine", "ltx2_dit_res2s_step", "ltx2_dit_graph_capture_res2s")


@pytest.fixture(scope="module")
def tiny():
    z = np.load(os.path.join(ROOT, "tests", "golden", "res2s_loop_tiny.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype == np.float32 else z[k]) for k in z.files}


# ------------------------------------------------------------------ coefficients
def test_coefficients_equal_the_reference():
    from ltx_2_mlx_amd.components import get_res2s_coefficients
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "res2s_coefficients.json")))
    hs = [r["h"] for r in gold["rows"]]
    assert len(hs) >= 12 and all(h in hs for h in (0.0, 1e-12, 0.05, 0.49, 0.5, 2.0))
    sig = gold["scheduler_sigmas_15"]
    assert len(sig) == 16 and all(math.log(sig[i] / sig[i + 1]) in hs for i in range(14))
    cache = {}
    for r in gold["rows"]:
        got = get_res2s_coefficients(r["h"], cache, r["c2"])
        for g, w in zip(got, r["coefficients"]):
            assert abs(g - w) <= 1e-12 * abs(w), (r, got)
    assert (1, -0.05 * 0.5) in cache and (2, -0.05) in cache             # the cache is keyed (j, z), as the reference's


def test_coefficients_closed_forms():
    from ltx_2_mlx_amd.components import get_res2s_coefficients, phi
    assert phi(1, 0.0) == 1.0 and phi(2, 0.0) == 0.5 and phi(3, 0.0) == 1.0 / 6
    assert phi(1, 5e-11) == 1.0 and phi(2, -5e-11) == 0.5                 # the |z| < 1e-10 branch
    for z in (-2.0, -0.3, 0.7):
        assert abs(phi(1, z) - math.expm1(z) / z) < 1e-14
        assert abs(phi(2, z) - (math.expm1(z) - z) / z**2) < 1e-13
    for h in (0.05, 0.49, 0.5, 2.0):
        for c2 in (0.5, 0.25):
            a21, b1, b2 = get_res2s_coefficients(h, {}, c2)
            assert abs(b1 + b2 - phi(1, -h)) < 1e-15 and a21 == c2 * phi(1, -h * c2) and b2 == phi(2, -h) / c2


# ------------------------------------------------------------------ the loop against the reference's own
@pytest.mark.parametrize("table", ["scheduler", "bong", "final"])
def test_restatement_loop_equals_the_reference(tiny, table):
    """tests/res2s_ref.res2s_loop with the stored stub against the reference's own _res2s_denoise_loop (float32, executed through the shim):
    the same elementary fp32 operations in the same order.  On the machine that recorded the fixture the two are bit-equal (maximum
    absolute difference 0, all three tables); on another CPU torch.tanh's vector path rounds the last bit differently and the measured
    maximum is 1.431e-06 (scheduler table; 2.384e-07 bong, 0 final) on values of order 1.  Gate: 5 x that."""
    t = tiny
    x0p, x0n = R.stub_x0(t["w"], t["bias"], t["context"]), R.stub_x0(t["w"], t["bias"], t["negative_context"])
    assert sorted(set(t["mask"].reshape(-1).tolist())) == [0.0, pytest.approx(0.1), 1.0] and t["latent"].shape == (1, 24, 8)
    trace = []
    sig = t[f"sigmas_{table}"].tolist()
    got = R.res2s_loop(t["latent"], t["mask"], t["clean"], x0p, x0n, sig, float(t["cfg_scale"]), trace=trace)
    want = t[f"result_{table}"]
    print(f"res2s restatement vs reference, table {table}: max abs difference {float((got - want).abs().max()):.3e}")
    assert float((got - want).abs().max()) <= LOOP_GATE
    # what the table is there for
    bong = [(-math.log(sn / s) < 0.5, s > 0.03) for s, sn, _ in trace if sn > 0]
    if table == "scheduler":
        assert sig[-1] == 0.0 and len(trace) == 4 and not any(f for _, _, f in trace) and trace[-1][1] == 0.0011
    elif table == "bong":
        assert {(True, True), (True, False), (False, True), (False, False)} <= set(bong)
    else:
        assert [f for _, _, f in trace] == [False, True] and sig[-1] == 0.0005
    # the reference calls back after every step but a final one
    assert t[f"callbacks_{table}"].tolist() == [[i + 1, len(sig) - 1] for i in range(sum(not f for _, _, f in trace))]
    # after a final step (latent = denoised) the tokens of mask 0 sit on their clean values
    assert torch.equal(got[:, :8], t["clean"][:, :8]) == (table == "final")


def test_kernel_restatement_matches_loop_restatement(tiny):
    """midpoint / combine written over velocities (what the kernels take) compose to the loop's step written over x0 predictions."""
    t = tiny
    g = torch.Generator().manual_seed(3)
    x, vc, vu, clean = (torch.randn(24, 8, generator=g) for _ in range(4))
    mask = t["mask"].reshape(-1)
    s, sn, cfg = 0.05, 0.035, 3.0
    from ltx_2_mlx_amd.components import get_res2s_coefficients
    h = -math.log(sn / s)
    a21, b1, b2 = get_res2s_coefficients(h, {})
    ts = mask * s
    xm, an, e = R.midpoint(x, vc, vu, ts, mask, clean, cfg, h * a21, 100)
    d = R.guide_blend(x - ts[:, None] * vc, x - ts[:, None] * vu, mask, clean, cfg)
    xm2, an2, e2 = R.midpoint_from_d(x, d, h * a21, 100)
    assert torch.equal(xm, xm2) and torch.equal(an, an2) and torch.equal(e, e2)
    assert torch.equal(R.midpoint(x, vc, vu, ts, mask, clean, cfg, 0.0, 0, final=True)[0], d)
    assert torch.equal(R.midpoint(x, vc, None, ts, None, None, cfg, 0.0, 0, final=True)[0], x - ts[:, None] * vc)
    out = R.combine(xm, vc, vu, ts, mask, clean, cfg, an, e, h, b1, b2)
    assert out.shape == x.shape and bool(torch.isfinite(out).all())


def test_sigma_injection_keeps_the_step_count():
    from ltx_2_mlx_amd.components import LTX2Scheduler
    for steps in (4, 15):
        sig = [float(s) for s in LTX2Scheduler().execute(steps=steps)]
        n, used = R.loop_sigmas(sig)
        assert sig[-1] == 0.0 and n == steps and len(used) == steps + 2 and used[n] == 0.0011 and used[:n] == sig[:n]
    n, used = R.loop_sigmas([0.5, 0.1, 0.0005])
    assert n == 2 and used == [0.5, 0.1, 0.0005]


class _FakeModel:
    """What res2s_denoise_loop asks of the engine, recorded on the CPU."""
    is_av = False

    def __init__(self):
        self.calls, self.captured = [], None

    def clone_sharing_weights(self):
        self.neg = _FakeModel()
        return self.neg

    def prepare(self, *a, **k):
        pass

    def res2s_step_(self, neg, lat, video, sub, sigma, sigma_next, cfg, denoise_mask=None, clean_latent=None):
        self.calls.append((neg is not None, sigma, sigma_next, None if sub is None else float(sub.sigma[0])))

    def capture_res2s_graph(self, neg, lat, sig, cfg, denoise_mask=None, clean_latent=None):
        self.captured = (neg is not None, list(sig))

    def replay_res2s_graph(self):
        pass


class _FakeStream:
    def wait_stream(self, s):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_denoise_loop_sigma_handling_and_negative_condition(monkeypatch):
    """res2s_denoise_loop hands the engine the reference's steps: len(sigmas) - 1 of them, the last landing on 0.0011; a table that ends
    above 0 stops on its final step without a callback; the negative context is used under the reference's condition."""
    from ltx_2_mlx_amd.components import LTX2Scheduler
    from ltx_2_mlx_amd.pipelines import common
    from ltx_2_mlx_amd.types import LatentState
    monkeypatch.setattr(torch.cuda, "Stream", _FakeStream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: _FakeStream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: s)

    class X0:
        def __init__(self):
            self.velocity_model = _FakeModel()

    st = LatentState(latent=torch.zeros(1, 6, 8), denoise_mask=torch.ones(1, 6, 1), positions=torch.zeros(1, 3, 6, 2), clean_latent=torch.zeros(1, 6, 8))
    ctx = torch.zeros(1, 4, 8)
    f32 = lambda v: float(np.float32(v))
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    x, seen = X0(), []
    out = common.res2s_denoise_loop(x, st, sig, ctx, ctx, 3.0, callback=lambda i, n: seen.append((i, n)))
    calls = x.velocity_model.calls
    assert out.latent.shape == (1, 6, 8) and len(calls) == 4 and seen == [(1, 4), (2, 4), (3, 4), (4, 4)]
    assert calls[-1][2] == f32(0.0011) and [c[1] for c in calls] == sig[:4] and all(c[0] for c in calls)
    assert calls[-1][3] == pytest.approx(math.sqrt(sig[3] * 0.0011), rel=1e-6)
    x = X0()
    common.res2s_denoise_loop(x, st, sig, ctx, ctx, 3.0)                                   # no callback: captured
    assert x.velocity_model.calls == [] and x.velocity_model.captured == (True, sig[:4] + [f32(0.0011)])
    x, seen = X0(), []
    common.res2s_denoise_loop(x, st, [0.5, 0.1, 0.0005], ctx, ctx, 3.0, callback=lambda i, n: seen.append((i, n)))
    assert [(c[1], c[2]) for c in x.velocity_model.calls] == [(0.5, f32(0.1)), (f32(0.1), f32(0.0005))] and seen == [(1, 2)]
    assert x.velocity_model.calls[-1][3] is None                                          # the final step has no sub-sigma evaluation
    for cfg, acfg, nctx, want in ((1.0, 1.0, ctx, False), (1.0, 7.0, ctx, True), (3.0, 1.0, ctx, True), (3.0, 7.0, None, False)):
        x = X0()
        common.res2s_denoise_loop(x, st, sig, ctx, nctx, cfg, acfg, callback=lambda i, n: None)
        assert all(c[0] == want for c in x.velocity_model.calls), (cfg, acfg, want)
    x = X0()
    common.res2s_denoise_loop(x, st, [1.0 - 0.01 * i for i in range(70)], ctx, ctx, 3.0)    # 69 steps: not captured
    assert x.velocity_model.captured is None and len(x.velocity_model.calls) == 69


# ------------------------------------------------------------------ config
def test_config_defaults_and_validation():
    from ltx_2_mlx_amd.pipelines import TI2VidHQConfig
    c = TI2VidHQConfig()
    assert (c.height, c.width, c.num_frames, c.num_inference_steps, c.cfg_scale, c.audio_cfg_scale, c.guidance_rescale, c.seed, c.fps) == \
        (1088, 1920, 97, 15, 3.0, 7.0, 0.45, 42, 25.0)
    assert c.distilled_lora_config is None and c.tiling_config is None and c.audio_enabled is False and c.use_internal_audio_branch is True
    assert (c.audio_vae_channels, c.audio_mel_bins, c.audio_sample_rate, c.audio_hop_length, c.audio_downsample_factor, c.audio_output_sample_rate) == \
        (8, 16, 16000, 160, 4, 24000)
    assert c._get_tiling_config() is not None and TI2VidHQConfig(height=64, width=128, num_frames=9)._get_tiling_config() is None
    with pytest.raises(ValueError, match=r"num_frames must be 8\*k \+ 1, got 96"):
        TI2VidHQConfig(num_frames=96)
    with pytest.raises(ValueError, match="must be divisible by 64"):
        TI2VidHQConfig(height=1080)
    with pytest.raises(ValueError, match="must be divisible by 64"):
        TI2VidHQConfig(width=1000)


def test_pipeline_refuses_audio():
    from ltx_2_mlx_amd.pipelines import TI2VidHQConfig, TI2VidHQPipeline

    class M:
        model_type = None
        device = "cpu"

    class X0(M):
        velocity_model = M()

    from ltx_2_mlx_amd.model import transformer as T
    pipe = TI2VidHQPipeline.__new__(TI2VidHQPipeline)
    pipe.transformer = pipe._velocity_model = M()
    pipe.spatial_upscaler = object()
    with pytest.raises(NotImplementedError, match="TI2VidHQPipeline"):
        pipe.denoise_latent(torch.zeros(1, 4, 8), None, TI2VidHQConfig(height=64, width=128, num_frames=9, audio_enabled=True))
    pipe.spatial_upscaler = None
    with pytest.raises(ValueError, match="requires spatial_upscaler"):
        pipe.denoise_latent(torch.zeros(1, 4, 8), None, TI2VidHQConfig(height=64, width=128, num_frames=9))
    assert T.LTXModel.res2s_step_ and T.LTXModel.capture_res2s_graph and T.LTXModel.replay_res2s_graph


# ------------------------------------------------------------------ generate_video
def test_generate_video_routes_ti2vid_hq(monkeypatch, tmp_path):
    import generate as gen

    class Routed(Exception):
        pass

    def spy(name):
        def f(*a, **k):
            raise Routed(name, a, k)
        return f

    for name in ("load_transformer", "load_av_transformer", "create_vae_decoder", "create_dummy_text_encoding", "encode_with_gemma"):
        monkeypatch.setattr(gen, name, spy(name))
    kw = dict(use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"), height=128, width=192, num_frames=9, pipeline_type="ti2vid-hq")
    up = dict(spatial_upscaler_weights="random")
    assert "ti2vid-hq" in gen._PIPELINES_KNOWN
    with pytest.raises(ValueError, match="unknown pipeline_type"):
        gen.generate_video("p", **{**kw, "pipeline_type": "bogus"})
    for pt in ("two-stage", "ic-lora"):
        with pytest.raises(NotImplementedError, match=pt):
            gen.generate_video("p", **{**kw, "pipeline_type": pt})
    # refused with this pipeline, before any model loads
    lora = str(tmp_path / "l.safetensors")
    open(lora, "wb").close()
    for extra in (dict(generate_audio=True), dict(audio_path="a.wav"), dict(two_stage_distilled=True), dict(upscale_temporal=True),
                  dict(keyframes=["k.png:0"])):
        with pytest.raises(NotImplementedError, match="ti2vid-hq"):
            gen.generate_video("p", **kw, **up, **extra)
    with pytest.raises(ValueError, match="--spatial-upscaler-weights"):
        gen.generate_video("p", **kw)
    with pytest.raises(ValueError, match="divisible by 64"):
        gen.generate_video("p", **{**kw, "height": 96}, **up)
    with pytest.raises(FileNotFoundError, match="distilled LoRA"):
        gen.generate_video("p", **kw, **up, distilled_lora=str(tmp_path / "missing.safetensors"))
    with pytest.raises(NotImplementedError, match="fp8_resident"):
        gen.generate_video("p", **kw, **up, distilled_lora=lora, fp8_resident=True)
    # distilled_lora is honoured here and refused as before everywhere else
    with pytest.raises(NotImplementedError, match="distilled_lora"):
        gen.generate_video("p", **{**kw, "pipeline_type": "text-to-video"}, distilled_lora=lora)
    # everything in order: the first loader is reached
    for extra in ({}, dict(distilled_lora=lora, distilled_lora_scale=0.5), dict(cfg_scale=3.0)):
        with pytest.raises(Routed) as e:
            gen.generate_video("p", **kw, **up, **extra)
        assert e.value.args[0] == "create_dummy_text_encoding"
    # the command line: --pipeline keeps the reference's choices, --ti2vid-hq selects the pipeline
    p = gen.build_parser()
    assert gen.kwargs_from_args(p.parse_args(["a prompt", "--ti2vid-hq"]))["pipeline_type"] == "ti2vid-hq"
    assert gen.kwargs_from_args(p.parse_args(["a prompt"]))["pipeline_type"] == "text-to-video"
    assert "never reaches" in p.format_help()


# ------------------------------------------------------------------ the LoRA of stage 2
def test_lora_fuse_and_restore_on_cpu_tensors():
    from ltx_2_mlx_amd.loader.lora_loader import LoRAConfig
    from ltx_2_mlx_amd.pipelines.ti2vid_hq import checkpoint_views, fused_lora, lora_touched

    class Model:
        def __init__(self):
            g = torch.Generator().manual_seed(9)
            r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)
            self.w = {"transformer_blocks.0.attn1.to_qkv.weight": r(24, 8), "transformer_blocks.0.attn1.to_qkv.bias": torch.randn(24, generator=g),
                      "transformer_blocks.0.attn2.to_kv.weight": r(16, 8), "transformer_blocks.0.attn2.to_q.weight": r(8, 8),
                      "transformer_blocks.0.ff.net.2.weight": r(8, 32), "proj_out.weight": r(8, 8)}
            self.replaced = []

        def weight_tensors(self):
            return self.w

        def replace_weights(self, tensors):
            self.replaced.append(sorted(tensors))
            self.w.update(tensors)

    m = Model()
    before = {k: v.clone() for k, v in m.w.items()}
    ids = {k: v.data_ptr() for k, v in m.w.items()}
    assert [k for k, _ in checkpoint_views("transformer_blocks.0.attn1.to_qkv.weight", m.w["transformer_blocks.0.attn1.to_qkv.weight"])] == \
        [f"transformer_blocks.0.attn1.{p}.weight" for p in ("to_q", "to_k", "to_v")]
    keys = ["diffusion_model.transformer_blocks.0.attn1.to_k.lora_A.weight", "diffusion_model.transformer_blocks.0.attn1.to_k.lora_B.weight",
            "transformer_blocks.0.ff.net.2.lora_down.weight", "transformer_blocks.0.ff.net.2.lora_up.weight"]
    touched = lora_touched(m.w, keys)
    assert sorted(touched) == ["transformer_blocks.0.attn1.to_qkv.weight", "transformer_blocks.0.ff.net.2.weight"]

    def fuse(weights, configs):              # stands for loader.fuse_lora_into_weights (its GEMM needs the GPU): adds strength where the file has a pair
        assert sorted(weights) == sorted(k for views in touched.values() for k, _ in views)
        hit = ("transformer_blocks.0.attn1.to_k.weight", "transformer_blocks.0.ff.net.2.weight")
        return {k: ((v.float() + configs[0].strength).to(v.dtype) if k in hit else v) for k, v in weights.items()}

    with pytest.raises(RuntimeError, match="inside"):
        with fused_lora(m, LoRAConfig("unused", 0.5), fuse=fuse, lora_keys=keys):
            qkv = m.w["transformer_blocks.0.attn1.to_qkv.weight"]
            b = before["transformer_blocks.0.attn1.to_qkv.weight"]
            assert torch.equal(qkv[:8], b[:8]) and torch.equal(qkv[16:], b[16:]) and torch.equal(qkv[8:16], (b[8:16].float() + 0.5).to(torch.bfloat16))
            assert not torch.equal(m.w["transformer_blocks.0.ff.net.2.weight"], before["transformer_blocks.0.ff.net.2.weight"])
            assert m.w["proj_out.weight"].data_ptr() == ids["proj_out.weight"]          # untouched tensors are not copied
            raise RuntimeError("inside")                                                # the originals come back in a finally
    assert m.replaced == [sorted(touched), sorted(touched)]
    assert set(m.w) == set(before) and all(torch.equal(m.w[k], before[k]) and m.w[k].data_ptr() == ids[k] for k in before)
    with fused_lora(m, None):
        pass
    assert len(m.replaced) == 2
    m.w["transformer_blocks.0.ff.net.0.proj.weight"] = torch.zeros(32, 8, dtype=torch.uint8)      # an fp8-resident model
    with pytest.raises(NotImplementedError, match="fp8_resident"):
        with fused_lora(m, LoRAConfig("unused", 0.5), fuse=fuse, lora_keys=keys):
            pass


# ------------------------------------------------------------------ ABI
def test_abi_declares_the_res2s_entries():
    from ltx_2_mlx_amd import _native as nv
    assert nv.ABI_VERSION == 3
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    assert re.search(r"#define\s+LTX2_ABI_VERSION\s+3\b", header)
    for name in NEW_ENTRIES:
        assert name in nv.SIGNATURES, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    n_args = lambda name: len(nv.SIGNATURES[name][1])
    assert (n_args("ltx2_res2s_midpoint"), n_args("ltx2_res2s_combine"), n_args("ltx2_dit_res2s_step"), n_args("ltx2_dit_graph_capture_res2s")) == (16, 17, 14, 11)
