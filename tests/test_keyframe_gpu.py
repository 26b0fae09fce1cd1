"""Keyframe interpolation on the GPU: the guided Euler kernel bit for bit, the one-call guided step and its captured graph against the
same kernels called one by one, the guided loop against the fp32 restatement (with the EXISTING eager guidance as the yardstick), the
pipeline and the CLI.  Tiny models as tests/test_parity.py builds them (2 heads x 128, 2 layers, caption 128)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import measure, rel_l2

import keyframe_ref as R
from test_parity import make_dit, make_vae, pearson

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("rows,C", [(37, 128), (5, 6), (33000, 128)])       # 16-byte form; element-wise form (C % 4 != 0); past one pass of the capped grid
@pytest.mark.parametrize("build", [torch.bfloat16, torch.float16])
def test_guided_euler_step_bit_for_bit(dev, build, rows, C):
    from ltx_2_mlx_amd import kernels as K
    g = torch.Generator().manual_seed(rows * 131 + C)
    x, vc, vu, clean = (torch.randn(rows, C, generator=g) for _ in range(4))
    ts_row = torch.rand(rows, generator=g)
    mask = torch.ones(rows)
    mask[::3] = 0.0
    mask[1::3] = 0.05
    n = rows * C
    sigma, sigma_next = 0.909375, 0.725
    for ts in (torch.tensor([0.909375]), ts_row):
        for mk in (None, mask):
            for scale in (1.0, 3.0, 7.5):
                ref = R.guided_euler_step(x, vc, vu, ts, mk, clean if mk is not None else None, scale, sigma, sigma_next)
                buf = torch.full((n + 64,), SENTINEL, device=dev)
                out = buf[:n].view(rows, C)
                args = (vc.to(dev), vu.to(dev), ts.to(dev), scale, sigma, sigma_next)
                kw = dict(mask=None if mk is None else mk.to(dev), clean=None if mk is None else clean.to(dev), dtype=build)
                K.guided_euler_step(x.to(dev), *args, out=out, **kw)
                tag = f"ts{ts.numel()} mask{mk is not None} cfg{scale}"
                assert torch.equal(out.cpu(), ref), f"{tag}: {int((out.cpu() != ref).sum())} of {n} elements differ"
                assert bool((buf[n:] == SENTINEL).all()), tag                   # nothing past rows * C
                # in place: the same bits
                xbuf = torch.full((n + 64,), SENTINEL, device=dev)
                xin = xbuf[:n].view(rows, C)
                xin.copy_(x)
                K.guided_euler_step(xin, *args, out=xin, **kw)
                assert torch.equal(xin.cpu(), ref) and bool((xbuf[n:] == SENTINEL).all()), tag
    if rows == 37:
        with pytest.raises(ValueError, match="Sigma can't be 0.0"):
            K.guided_euler_step(x.to(dev), vc.to(dev), vu.to(dev), torch.tensor([0.5], device=dev), 3.0, 0.0, 0.5, dtype=build)
        with pytest.raises(ValueError, match="Sigma can't be 0.0"):
            R.guided_euler_step(x, vc, vu, ts_row, None, None, 3.0, 0.0, 0.5)


_off_case = {}


@pytest.mark.parametrize("build", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("off", ["x", "vc", "vu", "clean", "out"])
def test_guided_euler_step_each_operand_off_alignment(dev, build, off):
    """9 x 8 with one [rows][C] operand 4 bytes off a 16-byte boundary: the element-wise form although C % 4 == 0, the same bits as the CPU
    restatement (computed once), nothing written outside `out`."""
    from ltx_2_mlx_amd import kernels as K
    rows, C, sigma, sigma_next = 9, 8, 0.909375, 0.725
    if not _off_case:
        g = torch.Generator().manual_seed(rows * 131 + C)
        for name in ("x", "vc", "vu", "clean"):
            _off_case[name] = torch.randn(rows, C, generator=g)
        _off_case["ts"] = torch.rand(rows, generator=g)
        _off_case["mask"] = torch.tensor([0.0, 0.05, 1.0] * 3)
        _off_case["ref"] = R.guided_euler_step(*(_off_case[k] for k in ("x", "vc", "vu", "ts", "mask", "clean")), 3.0, sigma, sigma_next)
    t, n, d, bufs = _off_case, rows * C, {}, {}
    for name in ("x", "vc", "vu", "clean", "out"):
        o = 1 if name == off else 0
        bufs[name] = torch.full((n + 64 + o,), SENTINEL, device=dev)
        d[name] = bufs[name][o:o + n].view(rows, C)
        assert d[name].data_ptr() % 16 == 4 * o
        if name != "out":
            d[name].copy_(t[name])
    K.guided_euler_step(d["x"], d["vc"], d["vu"], t["ts"].to(dev), 3.0, sigma, sigma_next, mask=t["mask"].to(dev), clean=d["clean"], out=d["out"], dtype=build)
    assert torch.equal(d["out"].cpu(), t["ref"]), f"{int((d['out'].cpu() != t['ref']).sum())} of {n} elements differ"
    o = 1 if off == "out" else 0
    assert bool((bufs["out"][:o] == SENTINEL).all()) and bool((bufs["out"][o + n:] == SENTINEL).all())


# ------------------------------------------------------------------ shared tiny model + keyframe state (N = 72 + 2 * 24 = 120, S = 64)
class Tiny:
    pass


@pytest.fixture(scope="module")
def tiny(dev):
    from ltx_2_mlx_amd.components import VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning import VideoConditionByKeyframeIndex, VideoLatentTools
    from ltx_2_mlx_amd.types import VideoLatentShape
    t = Tiny()
    t.cfg, t.wq, t.m = make_dit(dev, heads=2, layers=2, cap=128)
    g = torch.Generator().manual_seed(4321)
    tools = VideoLatentTools(patchifier=VideoLatentPatchifier(patch_size=1), target_shape=VideoLatentShape(1, 128, 3, 4, 6), fps=24.0)
    st = tools.create_initial_state()
    t.kf = [torch.randn(1, 128, 1, 4, 6, generator=g) for _ in range(2)]
    st = VideoConditionByKeyframeIndex(t.kf[0], 0, 1.0).apply_to(st, tools)          # keyframe A: mask 0
    st = VideoConditionByKeyframeIndex(t.kf[1], 16, 0.9).apply_to(st, tools)         # keyframe B: mask 0.1
    t.tools = tools
    t.mask, t.clean, t.pos = st.denoise_mask, st.clean_latent, st.positions
    assert t.mask.shape == (1, 120, 1) and float(t.mask[0, 72, 0]) == 0.0 and abs(float(t.mask[0, 96, 0]) - 0.1) < 1e-6
    t.lat = torch.randn(1, 120, 128, generator=g)
    t.ctx = 0.1 * torch.randn(1, 64, 128, generator=g)
    t.nctx = 0.1 * torch.randn(1, 64, 128, generator=g)
    return t


def _state(t, dev):
    from ltx_2_mlx_amd.types import LatentState
    return LatentState(latent=t.lat.clone().to(dev), denoise_mask=t.mask.to(dev), positions=t.pos.to(dev), clean_latent=t.clean.to(dev))


# ------------------------------------------------------------------ 2. the engine step
def test_guided_step_equals_its_three_parts(dev, tiny):
    """guided_step_ == ltx2_dit_forward(ctx), ltx2_dit_forward(neg), ltx2_guided_euler_step: the same kernels in the same order (the video
    path has no atomics), so the same bits.  Per-token timesteps (mask * sigma) and the uniform form."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import Modality
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    ctx, nctx, pos = t.ctx.to(dev), t.nctx.to(dev), t.pos.to(dev)
    sigma, sigma_next, scale = 0.909375, 0.725, 3.0
    mask1 = t.mask[0].reshape(-1).to(dev).contiguous()
    clean = t.clean[0].to(dev).contiguous()
    for per_token in (True, False):
        m.prepare(ctx, pos, per_token=per_token)
        neg.prepare(nctx, pos, per_token=per_token)
        ts = (t.mask.to(dev) * sigma) if per_token else torch.tensor([sigma], device=dev)
        lat = t.lat[0].to(dev).contiguous()
        mod = lambda c: Modality(latent=lat[None], context=c, context_mask=None, timesteps=ts, positions=pos)
        vc, vu = m(mod(ctx))[0].clone(), neg(mod(nctx))[0].clone()
        assert float((vc - vu).abs().max()) > 1e-3                                  # two prompts, two velocities
        mk, cl = (mask1, clean) if per_token else (None, None)
        want = K.guided_euler_step(lat, vc, vu, ts.reshape(-1), scale, sigma, sigma_next, mask=mk, clean=cl)
        got = lat.clone()
        m.guided_step_(neg, got, mod(ctx), sigma, sigma_next, scale, denoise_mask=mk, clean_latent=cl)
        assert torch.equal(got, want), f"per_token={per_token}: {int((got != want).sum())} elements differ"
        assert bool(torch.isfinite(got).all()) and not torch.equal(got, lat)


def test_guided_step_refusals(dev, tiny):
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd.model.transformer import LTXModel, LTXModelType, Modality
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    ctx, nctx, pos = t.ctx.to(dev), t.nctx.to(dev), t.pos.to(dev)
    m.prepare(ctx, pos, per_token=True)
    neg.prepare(nctx, pos, per_token=True)
    lat = t.lat[0].to(dev).contiguous()
    ts1 = torch.tensor([0.5], device=dev)
    tsn = (t.mask.to(dev) * 0.5).reshape(-1).contiguous()
    L = nv.lib()

    def step(a, b, ts=ts1, n_ts=1, sigma=0.5):
        nv.check(L.ltx2_dit_guided_step(a, b, nv.ptr(lat), nv.ptr(ts), n_ts, None, None, None, 3.0, sigma, 0.25, nv.stream()))

    with pytest.raises(ValueError, match="ctx == neg"):
        step(m._h, m._h)
    av = LTXModel(model_type=LTXModelType.AudioVideo, num_attention_heads=2, attention_head_dim=128, num_layers=2, caption_channels=128,
                  audio_attention_heads=2, device=dev)
    for a, b in ((m._h, av._h), (av._h, m._h)):
        with pytest.raises(ValueError, match="VideoOnly"):
            step(a, b)
    fresh = LTXModel(num_attention_heads=2, attention_head_dim=128, num_layers=2, caption_channels=128, device=dev)      # never prepared
    with pytest.raises(ValueError, match="prepare"):
        step(m._h, fresh._h)
    other = make_dit(dev, heads=2, layers=2, cap=128)[2]
    other.prepare(nctx, pos[:, :, :96].contiguous(), per_token=True)                # another N
    with pytest.raises(ValueError, match="contexts differ"):
        step(m._h, other._h)
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        step(m._h, neg._h, sigma=0.0)
    other.prepare(nctx, pos, per_token=False)                                       # a fresh binding at N = 120 without per-token buffers
    with pytest.raises(ValueError, match="per-token"):
        step(m._h, other._h, ts=tsn, n_ts=120)
    with torch.cuda.stream(torch.cuda.Stream()):
        with pytest.raises(ValueError, match="per-token"):
            m.capture_guided_graph(other, lat.clone(), [1.0, 0.5, 0.0], 3.0, denoise_mask=tsn, clean_latent=t.clean[0].to(dev).contiguous())
        with pytest.raises(ValueError, match="tokens x"):
            m.capture_guided_graph(neg, lat.clone(), [1.0, 0.5, 0.0], 3.0, denoise_mask=tsn[:100].contiguous(), clean_latent=t.clean[0].to(dev).contiguous())
        with pytest.raises(ValueError, match="bad argument"):
            m.capture_guided_graph(neg, lat.clone(), [1.0 - 0.01 * i for i in range(66)], 3.0)
    with pytest.raises(ValueError, match="second LTXModel"):
        m.guided_step_(None, lat, Modality(latent=lat[None], context=ctx, context_mask=None, timesteps=ts1, positions=pos), 0.5, 0.25, 3.0)


# ------------------------------------------------------------------ 3. the loop
@pytest.fixture(scope="module")
def loop_ref(tiny):
    """Four LTX2Scheduler steps at cfg 3 in fp32 (oracle.dit.x0_model inside keyframe_ref.guided_loop), computed once."""
    from oracle import dit
    from ltx_2_mlx_amd.components import LTX2Scheduler
    t = tiny
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    x0 = lambda c: (lambda x, ts, s: dit.x0_model(x, c, ts, t.pos, t.wq, t.cfg))
    return sig, R.guided_loop(t.lat, t.mask, t.clean, x0(t.ctx), x0(t.nctx), sig, 3.0)


def test_guided_loop_graph_eager_and_restatement(dev, tiny, loop_ref):
    """Graph replay == the eager guided_step_ loop, bit for bit.  Against the fp32 restatement the new loop may be at most 1.5 x as far
    as the EXISTING eager guidance (two X0Model calls + torch glue + ltx2_euler_step): the two differ only in fp32 rounding order inside
    the step, the 1.5 allows for 16-bit rounding flips of the DiT's input.  Measured on the MI355X: E0 = 5.749e-04, E1 = 5.750e-04."""
    from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import guided_denoise_loop, joint_denoise_loop
    t = tiny
    sig, ref = loop_ref
    x0m = X0Model(t.m)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    seen = []
    graph = guided_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFGGuider(3.0), EulerDiffusionStep(), use_hip_graph=True).latent.cpu()
    eager = guided_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFGGuider(3.0), EulerDiffusionStep(), use_hip_graph=False).latent.cpu()
    cb = guided_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFGGuider(3.0), EulerDiffusionStep(), callback=lambda i, n: seen.append((i, n)),
                             use_hip_graph=True).latent.cpu()
    assert torch.equal(graph, eager) and torch.equal(cb, eager) and seen == [(1, 4), (2, 4), (3, 4), (4, 4)]
    assert bool(torch.isfinite(graph).all())
    # keyframe A's appended tokens (mask 0) end at their clean values; the free tokens moved
    assert rel_l2(graph[:, 72:96], t.clean[:, 72:96]) < 1e-5 and rel_l2(graph[:, :72], t.lat[:, :72]) > 0.1
    old = joint_denoise_loop(x0m, False, _state(t, dev), None, sig, ctx, None, EulerDiffusionStep(), use_hip_graph=False,
                             negative_video_context=nctx, video_guider=CFGGuider(3.0))[0].latent.cpu()
    e0 = measure("E0 existing eager guidance vs fp32", rel_l2(old, ref))
    e1 = measure("E1 guided loop vs fp32", rel_l2(graph, ref))
    print(f"guided loop: E0 = {e0:.4e}  E1 = {e1:.4e}  pearson = {pearson(graph, ref):.6f}")
    assert e1 <= 1.5 * e0 and pearson(graph, ref) > 0.999


def test_other_guiders_go_through_joint_denoise_loop(dev, tiny):
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider, EulerDiffusionStep, LTX2Scheduler
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import guided_denoise_loop, joint_denoise_loop
    t = tiny
    sig = [float(s) for s in LTX2Scheduler().execute(steps=2)]
    x0m = X0Model(t.m)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    for guider in (CFGGuider(1.0), CFGStarRescalingGuider(3.0)):
        for graph in (False, True):
            a = guided_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, guider, EulerDiffusionStep(), use_hip_graph=graph).latent
            b = joint_denoise_loop(x0m, False, _state(t, dev), None, sig, ctx, None, EulerDiffusionStep(), None, graph,
                                   negative_video_context=nctx, video_guider=guider)[0].latent
            assert torch.equal(a, b), (guider, graph)


# ------------------------------------------------------------------ 4. the pipeline
@pytest.fixture(scope="module")
def parts(dev, tiny):
    from oracle import vae_encoder as oenc
    from ltx_2_mlx_amd.model.upscaler import SpatialUpscaler
    from ltx_2_mlx_amd.model.video_vae_encoder import SimpleVideoEncoder
    p = Tiny()
    w = oenc.make_encoder_weights(seed=51)
    p.enc_wq = {k: (v.to(torch.bfloat16).float() if v.dim() == 5 else v) for k, v in w.items()}
    p.enc = SimpleVideoEncoder(device=dev)
    p.enc.load_state_dict(w)
    _, _, p.dec = make_vae(dev, layers=1)
    p.up = SpatialUpscaler(in_channels=128, mid_channels=64, num_blocks_per_stage=1, device=dev)
    p.up.init_random_weights(seed=3)
    return p


PIPELINE_MEASURED = 7.283e-4    # rel-L2 of the stage-1 latent against the fp32 restatement, measured on the MI355X


def test_pipeline_single_stage_against_restatement(dev, tiny, parts):
    """use_two_stage=False at 64x96x9, keyframes at frames 0 and 8 given as tensors, 4 steps at cfg 3, the same noise on both sides: the
    denoised latent against tests/keyframe_ref.stage1 (oracle VAE encoder, oracle DiT, fp32 loop).  Gate: 5 x the value measured on the MI355X, 7.283e-04."""
    from oracle import dit, vae_encoder as oenc
    from ltx_2_mlx_amd.components import LTX2Scheduler
    from ltx_2_mlx_amd.pipelines import Keyframe, KeyframeInterpolationConfig, KeyframeInterpolationPipeline
    t = tiny
    g = torch.Generator().manual_seed(77)
    imgs = [torch.rand(1, 3, 1, 64, 96, generator=g) * 2 - 1 for _ in range(2)]
    noise = torch.randn(1, 12 + 2 * 6, 128, generator=g)
    kfs = [Keyframe(None, 0, 1.0, image=imgs[0]), Keyframe(None, 8, 0.9, image=imgs[1])]
    conf = KeyframeInterpolationConfig(height=64, width=96, num_frames=9, num_inference_steps=4, cfg_scale=3.0, use_two_stage=False)
    pipe = KeyframeInterpolationPipeline(t.m, parts.enc, None)
    out = pipe(t.ctx.to(dev), None, kfs, conf, negative_text_encoding=t.nctx.to(dev), initial_noise=noise.to(dev))
    assert out.shape == (1, 128, 2, 2, 3) and pipe.token_counts == [24]
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    x0 = lambda c: (lambda x, ts, s, pos: dit.x0_model(x, c, ts, pos, t.wq, t.cfg))
    ref = R.stage1([oenc.encoder_forward(i, parts.enc_wq) for i in imgs], [0, 8], [1.0, 0.9], (2, 2, 3), 24.0, noise, x0(t.ctx), x0(t.nctx), sig, 3.0)
    err = measure("keyframe stage 1 vs fp32 restatement", rel_l2(out.cpu(), ref))
    print(f"keyframe pipeline, single stage: rel-L2 = {err:.4e}  pearson = {pearson(out.cpu(), ref):.6f}")
    assert err <= 5 * PIPELINE_MEASURED
    # the default negative encoding is zeros of the context's shape
    a = pipe(t.ctx.to(dev), None, kfs, conf, initial_noise=noise.to(dev))
    b = pipe(t.ctx.to(dev), None, kfs, conf, negative_text_encoding=torch.zeros_like(t.ctx).to(dev), initial_noise=noise.to(dev))
    assert torch.equal(a, b) and not torch.equal(a, out)
    with pytest.raises(ValueError, match="outside"):
        pipe(t.ctx.to(dev), None, [Keyframe(None, 9, 1.0, image=imgs[0])], conf)


def test_pipeline_two_stage(dev, tiny, parts):
    from ltx_2_mlx_amd.pipelines import Keyframe, KeyframeInterpolationConfig, KeyframeInterpolationPipeline, create_keyframe_pipeline
    t = tiny
    g = torch.Generator().manual_seed(78)
    kfs = [Keyframe(None, 0, 1.0, image=torch.rand(1, 3, 1, 128, 192, generator=g) * 2 - 1),
           Keyframe(None, 8, 0.9, image=torch.rand(1, 3, 1, 128, 192, generator=g) * 2 - 1)]
    conf = KeyframeInterpolationConfig(height=128, width=192, num_frames=9, num_inference_steps=3, cfg_scale=3.0)
    pipe = create_keyframe_pipeline(t.m, parts.enc, parts.dec, parts.up)
    video = pipe(t.ctx.to(dev), None, kfs, conf)
    assert video.dtype == torch.uint8 and video.shape == (9, 128, 192, 3)
    assert pipe.token_counts == [12 + 2 * 6, 48 + 2 * 24]
    lat = pipe.denoise_latent(t.ctx.to(dev), kfs, conf)
    assert lat.shape == (1, 128, 2, 4, 6) and bool(torch.isfinite(lat).all())
    with pytest.raises(ValueError, match="requires spatial_upscaler"):
        KeyframeInterpolationPipeline(t.m, parts.enc, parts.dec)(t.ctx.to(dev), None, kfs, conf)


# ------------------------------------------------------------------ 5. the CLI
def test_generate_video_keyframe_interpolation(dev, tmp_path, capsys):
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    rs = np.random.RandomState(5)
    for name in ("a", "b"):
        Image.fromarray((rs.rand(100, 140, 3) * 255).astype(np.uint8)).save(tmp_path / f"{name}.png")
    frames = generate.generate_video("a test prompt", pipeline_type="keyframe-interpolation",
                                     keyframes=[f"{tmp_path / 'a.png'}:0", f"{tmp_path / 'b.png'}:8:0.9"], use_gemma=False, model_variant="dev",
                                     cfg_scale=3, num_steps=3, height=128, width=192, num_frames=9, seed=3, num_layers=2, num_heads=2,
                                     vae_base_channels=64, output_path=str(tmp_path / "k.mp4"))
    assert frames.dtype == torch.uint8 and frames.shape == (9, 128, 192, 3)
    saved = np.load(tmp_path / "k.npz")["frames"]
    assert saved.shape == (9, 128, 192, 3) and np.array_equal(saved, frames.cpu().numpy())
    assert os.path.exists(tmp_path / "k.mp4") or len(os.listdir(tmp_path / "k_frames")) == 9
    out = capsys.readouterr().out
    assert out.count("using zeros of the context's shape") == 1 and "DiT tokens per stage [24, 96]" in out
