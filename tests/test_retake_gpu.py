"""Retake on the GPU: retake_prepare against the torch path (every bit), retake_composite against the integer restatement (every byte),
the pipeline in both modes against a hand composition of the pieces that existed before it (every bit) and against the fp32 restatement,
the decoded and composited output, and the CLI.  Tiny models as tests/test_ic_lora_gpu.py builds them (2 heads x 128, 2 layers, caption 128)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import measure, rel_l2

import ic_lora_ref as IR
import retake_ref as RR
from test_parity import make_dit, make_vae, pearson

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = 1.5
GUARD = 0x5A


def _guarded_f32(shape, dev):
    """An fp32 buffer filled with PATTERN and its leading window of `shape`: nothing behind the window may change."""
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), PATTERN, dtype=torch.float32, device=dev)
    return buf, buf[:n].view(shape)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. retake_prepare
@pytest.mark.parametrize("grid", [(3, 2, 3), (3, 11, 1), (5, 9, 3)])        # P = 18 (below one tile), 33 (one over), 135 (tiles + a remainder)
def test_retake_prepare_equals_torch_path(dev, grid):
    """clean, mask and latent equal, as int32 views, what VideoLatentTools.create_initial_state (the patchify), the mask assignment of
    TemporalRegionMask.apply_to and GaussianNoiser give in torch, for four windows and two noise scales; nothing written behind the outputs."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.components import GaussianNoiser, VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning.tools import VideoLatentTools
    from ltx_2_mlx_amd.pipelines import TemporalRegionMask
    from ltx_2_mlx_amd.types import VideoLatentShape
    f, h, w = grid
    n = f * h * w
    g = torch.Generator().manual_seed(n)
    enc = torch.randn(1, 128, f, h, w, generator=g)
    flat = enc.view(-1)
    flat[:8] = torch.tensor([3.0e38, -3.0e38, 1.0e-40, -1.0e-42, 0.0, -0.0, 6.5e4, -1.17549435e-38])       # large, denormal, signed zeros
    flat[-3:] = torch.tensor([2.5e38, 1.0e-45, -7.0e-41])
    noise = torch.randn(n, 128, generator=g)
    enc, noise = enc.to(dev), noise.to(dev)
    tools = VideoLatentTools(patchifier=VideoLatentPatchifier(patch_size=1), target_shape=VideoLatentShape(1, 128, f, h, w), fps=24.0)
    base = tools.create_initial_state(dtype=torch.float32, initial_latent=enc)
    for f0, f1 in ((0, f), (0, 1), (f - 1, f), (1, 2)):
        mask = torch.zeros_like(base.denoise_mask)
        mask[:, f0 * h * w: f1 * h * w] = 1
        for scale in (1.0, 0.7):
            want = GaussianNoiser()(base.replace(denoise_mask=mask), noise_scale=scale, noise=noise[None])
            bufs, outs = zip(*[_guarded_f32(s, dev) for s in ((n, 128), (n,), (n, 128))])
            clean, m, lat = K.retake_prepare(enc, noise, f0, f1, noise_scale=scale, out=outs)
            assert clean.data_ptr() == outs[0].data_ptr() and lat.shape == (n, 128) and m.shape == (n,)
            for name, got, ref in (("clean", clean, want.clean_latent[0]), ("mask", m, want.denoise_mask[0, :, 0]), ("latent", lat, want.latent[0])):
                bad = int((_bits(got) != _bits(ref)).sum())
                assert bad == 0, f"{name} window [{f0}, {f1}) scale {scale}: {bad} of {ref.numel()} elements differ"
            for buf, s in zip(bufs, ((n, 128), (n,), (n, 128))):
                assert bool((buf[int(np.prod(s)):] == PATTERN).all())
            assert float(m.sum()) == (f1 - f0) * h * w
    # the mask is TemporalRegionMask's: 0.4 s - 0.7 s at 24 fps is latent frame 1
    region = TemporalRegionMask(0.4, 0.7, 24.0)
    assert region.frame_window(f) == (1, 2)
    _, m, _ = K.retake_prepare(enc, noise, 1, 2)
    assert torch.equal(m, region.apply_to(base, tools).denoise_mask[0, :, 0])
    # operands are taken as they lie or refused
    ok = lambda: [torch.empty(n, 128, device=dev), torch.empty(n, device=dev), torch.empty(n, 128, device=dev)]
    with pytest.raises(ValueError, match="encoded"):
        K.retake_prepare(enc.double(), noise, 0, 1)
    with pytest.raises(ValueError, match="encoded"):
        K.retake_prepare(enc[0], noise, 0, 1)
    with pytest.raises(ValueError, match="encoded"):
        K.retake_prepare(enc.cpu(), noise, 0, 1)
    with pytest.raises(ValueError, match="noise"):
        K.retake_prepare(enc, noise[:-1], 0, 1)
    with pytest.raises(ValueError, match="noise"):
        K.retake_prepare(enc, noise.half(), 0, 1)
    with pytest.raises(ValueError, match="noise"):
        K.retake_prepare(enc, torch.empty(n, 256, device=dev)[:, ::2], 0, 1)
    for f0, f1 in ((2, 1), (-1, 1), (0, f + 1)):
        with pytest.raises(ValueError, match="window"):
            K.retake_prepare(enc, noise, f0, f1)
    for i, bad in ((0, torch.empty(n, 256, device=dev)[:, ::2]), (1, torch.empty(n, 1, device=dev)), (2, torch.empty(n, 128, device=dev, dtype=torch.float16)),
                   (2, torch.empty(n + 1, 128, device=dev)), (1, torch.empty(n))):
        outs = ok()
        outs[i] = bad
        with pytest.raises(ValueError, match="out must be"):
            K.retake_prepare(enc, noise, 0, 1, out=outs)
    outs = ok()
    with pytest.raises(ValueError, match="overlap"):
        K.retake_prepare(enc, noise, 0, 1, out=(outs[0], outs[1], noise))
    with pytest.raises(ValueError, match="overlap"):
        K.retake_prepare(enc, noise, 0, 1, out=(outs[0], outs[1], outs[0]))


# ------------------------------------------------------------------ 2. retake_composite
WINDOWS = [(0, 9), (1, 9), (0, 1), (9, 17), (16, 17)]
RAMPS = [0, 1, 4, 40]


@pytest.mark.parametrize("shape", [(9, 4, 5), (17, 32, 48)])               # 60-byte frames: vectors across frame boundaries and a 12-byte tail
def test_retake_composite_equals_restatement(dev, shape):
    from ltx_2_mlx_amd import kernels as K
    t, h, w = shape
    rng = np.random.default_rng(t * 31 + w)
    dec = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    src = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    dec[2], src[2], dec[3], src[3] = 0, 255, 255, 0                        # constant frames, both ways round
    dec[t - 1], src[t - 1], dec[0, 0], src[0, 0] = 255, 255, 0, 0
    d, s = torch.from_numpy(dec).to(dev), torch.from_numpy(src).to(dev)
    n = dec.size
    for p0, p1 in WINDOWS:
        if p1 > t:
            with pytest.raises(ValueError, match="window"):
                K.retake_composite(d, s, p0, p1, 0)
            continue
        for ramp in RAMPS:
            buf = torch.full((n + 256,), GUARD, dtype=torch.uint8, device=dev)
            got = K.retake_composite(d, s, p0, p1, ramp, out=buf[:n].view(dec.shape))
            want = RR.composite(dec, src, p0, p1, ramp)
            bad = int((got.cpu().numpy() != want).sum())
            assert bad == 0, f"window [{p0}, {p1}) ramp {ramp}: {bad} of {n} bytes differ"
            assert bool((buf[n:] == GUARD).all())
            if ramp == 0:
                assert np.array_equal(want[:p0], src[:p0]) and np.array_equal(want[p1:], src[p1:]) and np.array_equal(want[p0:p1], dec[p0:p1])
    # clips that do not start on a 16-byte boundary go one byte per lane
    pad = lambda a: torch.cat([torch.zeros(1, dtype=torch.uint8, device=dev), a.reshape(-1)])[1:].view(a.shape)
    d1, s1 = pad(d), pad(s)
    assert d1.data_ptr() % 16 == 1
    assert np.array_equal(K.retake_composite(d1, s1, 1, 2, 4).cpu().numpy(), RR.composite(dec, src, 1, 2, 4))
    # out may not alias an input; operands are taken as they lie or refused
    for alias in (d, s):
        with pytest.raises(ValueError, match="overlap"):
            K.retake_composite(d, s, 0, 1, 1, out=alias)
    with pytest.raises(ValueError, match="out must be"):
        K.retake_composite(d, s, 0, 1, 1, out=torch.empty(t, h, w, 3, device=dev))
    with pytest.raises(ValueError, match="source"):
        K.retake_composite(d, s[:-1], 0, 1, 1)
    with pytest.raises(ValueError, match="decoded"):
        K.retake_composite(d.float(), s, 0, 1, 1)
    with pytest.raises(ValueError, match="source"):
        K.retake_composite(d, s.cpu(), 0, 1, 1)
    with pytest.raises(ValueError, match="decoded"):
        K.retake_composite(torch.zeros(t, h, w, 6, dtype=torch.uint8, device=dev)[..., ::2], s, 0, 1, 1)
    for ramp in (-1, 65536):
        with pytest.raises(ValueError, match="ramp"):
            K.retake_composite(d, s, 0, 1, ramp)
    with pytest.raises(ValueError, match="window"):
        K.retake_composite(d, s, 2, 1, 0)


# ------------------------------------------------------------------ shared models
class Parts:
    pass


@pytest.fixture(scope="module")
def parts(dev):
    from oracle import vae_encoder as oenc
    from ltx_2_mlx_amd.model.video_vae_encoder import SimpleVideoEncoder
    p = Parts()
    p.cfg, p.wq, p.m = make_dit(dev, heads=2, layers=2, cap=128)
    w = oenc.make_encoder_weights(seed=51)
    p.enc_wq = {k: (v.to(torch.bfloat16).float() if v.dim() == 5 else v) for k, v in w.items()}
    p.enc = SimpleVideoEncoder(device=dev)
    p.enc.load_state_dict(w)
    _, _, p.dec = make_vae(dev, layers=1)
    g = torch.Generator().manual_seed(93)
    p.ctx = 0.1 * torch.randn(1, 64, 128, generator=g)
    p.nctx = 0.1 * torch.randn(1, 64, 128, generator=g)
    p.source = torch.randint(0, 256, (17, 64, 96, 3), generator=g, dtype=torch.uint8).numpy()       # latent 3 x 2 x 3: 18 tokens
    p.noise = torch.randn(1, 18, 128, generator=g)
    p.encoded_ref = oenc.encoder_forward(IR.control_tensor(p.source), p.enc_wq)                     # the oracle's encoding, once
    return p


WINDOW = (0.4, 0.7)             # at 24 fps: pixel frames 9 .. 16 -> (9-1)//8 = 1, (16-1)//8 + 1 = 2: latent frame 1 alone


def _conf(window=WINDOW, **kw):
    from ltx_2_mlx_amd.pipelines import RetakeConfig
    return RetakeConfig(start_time=window[0], end_time=window[1], fps=24.0, **kw)


def _hand_state(parts, dev):
    """The state from the pieces that existed before the pipeline: the encoder's own entry on the host-normalised clip,
    create_initial_state, the torch TemporalRegionMask.apply_to, GaussianNoiser with the given noise."""
    from ltx_2_mlx_amd.components import GaussianNoiser, VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning.tools import VideoLatentTools
    from ltx_2_mlx_amd.pipelines import TemporalRegionMask, load_control_signal_tensor
    from ltx_2_mlx_amd.types import VideoLatentShape
    tools = VideoLatentTools(patchifier=VideoLatentPatchifier(patch_size=1), target_shape=VideoLatentShape(1, 128, 3, 2, 3), fps=24.0)
    encoded = parts.enc(load_control_signal_tensor(parts.source).to(dev))
    state = tools.create_initial_state(dtype=torch.float32, initial_latent=encoded)
    state = TemporalRegionMask(*WINDOW, 24.0).apply_to(state, tools)
    return tools, encoded, GaussianNoiser()(state, noise_scale=1.0, noise=parts.noise.to(dev))


def _preserved(out, encoded):
    """Latent frames 0 and 2 are the encoder's output bit for bit, frame 1 is not."""
    return torch.equal(_bits(out[:, :, 0]), _bits(encoded[:, :, 0])) and torch.equal(_bits(out[:, :, 2]), _bits(encoded[:, :, 2])) and \
        not torch.equal(out[:, :, 1], encoded[:, :, 1])


# ------------------------------------------------------------------ 3. distilled mode
DISTILLED_MEASURED = 5.568e-3    # rel-L2 of the retake latent against the fp32 restatement, measured on the MI355X (Pearson 0.999984)


def test_pipeline_distilled(dev, parts):
    """17 x 64 x 96 at 24 fps, the window 0.4 s - 0.7 s (latent frame 1 of 3), the 8 distilled steps, supplied noise.  Latent frames 0 and 2
    come back as the encoder gave them, bit for bit; the whole latent equals, bit for bit, the loop composed by hand from the existing
    pieces, captured, and the eager run with a callback.  Against tests/retake_ref.retake_latent (oracle VAE encoder, oracle DiT, fp32 loop)
    the gate is 5 x the rel-L2 measured on the MI355X, 5.568e-03, and Pearson > 0.999 (measured 0.999984).  Two of the three latent frames
    are the encoder's own output, so the figure is mostly the bf16 encoder's distance from the fp32 oracle encoder."""
    from oracle import dit
    from ltx_2_mlx_amd.components import DISTILLED_SIGMA_VALUES, EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import RetakePipeline, joint_denoise_loop
    pipe = RetakePipeline(parts.m, parts.enc, None)
    ctx, noise = parts.ctx.to(dev), parts.noise.to(dev)
    out = pipe(None, ctx, None, _conf(distilled=True), frames=parts.source, initial_noise=noise)
    assert out.shape == (1, 128, 3, 2, 3) and bool(torch.isfinite(out).all())
    assert (pipe.frame_window, pipe.pixel_window, pipe.token_count, pipe.fps) == ((1, 2), (1, 9), 18, 24.0)
    tools, encoded, state = _hand_state(parts, dev)
    assert _preserved(out, encoded)                                                                          # (a)
    sig = [float(s) for s in DISTILLED_SIGMA_VALUES]
    hand = joint_denoise_loop(X0Model(parts.m), False, state, None, sig, ctx, None, EulerDiffusionStep(), None, True)[0]
    assert torch.equal(_bits(out), _bits(tools.unpatchify(tools.clear_conditioning(hand)).latent))           # (b)
    seen = []
    eager = pipe(None, ctx, None, _conf(distilled=True), callback=lambda *a: seen.append(a), frames=parts.source, initial_noise=noise)
    assert torch.equal(_bits(eager), _bits(out)) and seen == [("retake", i + 1, 8) for i in range(8)]        # (c)
    x0 = lambda x, ts, s, pos: dit.x0_model(x, parts.ctx, ts, pos, parts.wq, parts.cfg)
    ref = RR.retake_latent(parts.encoded_ref, (1, 2), parts.noise, x0, sig)                                  # (d)
    err = measure("retake distilled vs fp32 restatement", rel_l2(out.cpu(), ref))
    r = pearson(out.cpu(), ref)
    print(f"retake pipeline, distilled: rel-L2 = {err:.4e}  pearson = {r:.6f}")
    assert err <= 5 * DISTILLED_MEASURED and r > 0.999
    # a seed instead of supplied noise: the same seed gives the same bits, the preserved frames stay preserved
    a = pipe(None, ctx, None, _conf(distilled=True, seed=5), frames=parts.source)
    b = pipe(None, ctx, None, _conf(distilled=True, seed=5), frames=torch.from_numpy(parts.source).to(dev))
    assert torch.equal(a, b) and _preserved(a, encoded) and not torch.equal(a, out)
    # regenerate_video=False: the mask stays all ones, every frame is regenerated
    full = pipe(None, ctx, None, _conf(distilled=True, regenerate_video=False), frames=parts.source, initial_noise=noise)
    assert pipe.frame_window == (0, 3) and not torch.equal(full[:, :, 0], encoded[:, :, 0]) and not torch.equal(full[:, :, 2], encoded[:, :, 2])
    with pytest.raises(ValueError, match=r"touches no frame.*17 frames at 24 fps"):
        pipe(None, ctx, None, _conf((5.0, 6.0), distilled=True), frames=parts.source)


# ------------------------------------------------------------------ 4. guided mode
GUIDED_MEASURED = 5.586e-3       # rel-L2 of the guided retake latent (4 steps, cfg 3) against the fp32 restatement, measured on the MI355X (Pearson 0.999984)


def test_pipeline_guided(dev, parts):
    """The same clip and window, LTX2Scheduler over 4 steps, cfg 3 with a random negative context: preserved frames bit-equal, the whole
    latent bit-equal to guided_denoise_loop called by hand on the hand-built state, different from the cfg 1 run; against the restatement
    with CFG the gate is 5 x the rel-L2 measured on the MI355X, 5.586e-03, and Pearson > 0.999 (measured 0.999984)."""
    from oracle import dit
    from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep, LTX2Scheduler
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import RetakePipeline, guided_denoise_loop
    pipe = RetakePipeline(parts.m, parts.enc, None)
    ctx, nctx, noise = parts.ctx.to(dev), parts.nctx.to(dev), parts.noise.to(dev)
    conf = _conf(num_inference_steps=4, cfg_scale=3.0)
    out = pipe(None, ctx, None, conf, negative_text_encoding=nctx, frames=parts.source, initial_noise=noise)
    tools, encoded, state = _hand_state(parts, dev)
    assert out.shape == (1, 128, 3, 2, 3) and bool(torch.isfinite(out).all()) and _preserved(out, encoded)
    sig = LTX2Scheduler().execute(steps=4)
    hand = guided_denoise_loop(X0Model(parts.m), state, sig, ctx, nctx, CFGGuider(3.0), EulerDiffusionStep(), None, True)
    assert torch.equal(_bits(out), _bits(tools.unpatchify(tools.clear_conditioning(hand)).latent))
    seen = []
    eager = pipe(None, ctx, None, conf, negative_text_encoding=nctx, callback=lambda *a: seen.append(a), frames=parts.source, initial_noise=noise)
    assert torch.equal(_bits(eager), _bits(out)) and seen == [("retake", i + 1, 4) for i in range(4)]
    plain = pipe(None, ctx, None, _conf(num_inference_steps=4, cfg_scale=1.0), negative_text_encoding=nctx, frames=parts.source, initial_noise=noise)
    assert _preserved(plain, encoded) and not torch.equal(plain, out)
    x0 = lambda c: (lambda x, ts, s, pos: dit.x0_model(x, c, ts, pos, parts.wq, parts.cfg))
    ref = RR.retake_latent(parts.encoded_ref, (1, 2), parts.noise, x0(parts.ctx), [float(s) for s in sig], cfg=(3.0, x0(parts.nctx)))
    err = measure("retake guided vs fp32 restatement", rel_l2(out.cpu(), ref))
    r = pearson(out.cpu(), ref)
    print(f"retake pipeline, guided: rel-L2 = {err:.4e}  pearson = {r:.6f}")
    assert err <= 5 * GUIDED_MEASURED and r > 0.999


# ------------------------------------------------------------------ 5. decoded output and composite
def test_decoded_output_and_composite(dev, parts):
    """The decoder mixes N(0, 1) noise into the latent (timestep conditioning), so every run decodes under the same generator state: the
    frames inside the window are then the uncomposited run's, byte for byte."""
    from ltx_2_mlx_amd.pipelines import create_retake_pipeline
    pipe = create_retake_pipeline(parts.m, parts.enc, parts.dec)
    ctx, noise = parts.ctx.to(dev), parts.noise.to(dev)

    def run(**kw):
        parts.dec.generator = torch.Generator(device=dev).manual_seed(7)
        try:
            return pipe(None, ctx, None, _conf(distilled=True, **kw), frames=parts.source, initial_noise=noise)
        finally:
            parts.dec.generator = None

    video = run()
    assert video.dtype == torch.uint8 and video.shape == (17, 64, 96, 3)
    kept = run(composite_source=True, composite_ramp=0)
    assert kept.dtype == torch.uint8 and kept.shape == (17, 64, 96, 3) and pipe.pixel_window == (1, 9)
    src = torch.from_numpy(parts.source).to(dev)
    assert torch.equal(kept[0], src[0]) and torch.equal(kept[9:], src[9:]) and torch.equal(kept[1:9], video[1:9])
    assert not torch.equal(video[0], src[0])                                 # the uncomposited run is a VAE round trip there
    faded = run(composite_source=True)                                       # the default ramp, 4 frames
    assert np.array_equal(faded.cpu().numpy(), RR.composite(video.cpu().numpy(), parts.source, 1, 9, 4))
    assert torch.equal(faded[13:], src[13:]) and not torch.equal(faded[9], src[9])


def test_tiled_decode_and_composite(dev, parts):
    """tiling_config: decode_tiled gives a float video, which the pipeline turns into uint8 frames before the composite.  Tiles of 64 pixels
    overlapping by 32 and of 16 frames overlapping by 8, so the 3 x 2 x 3 latent is cut along time and width.  The result is the tiled
    decode of the pipeline's own latent done by hand; with composite_source the frames outside the window are the source's bytes and
    those inside the uncomposited run's."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.video_vae import SpatialTilingConfig, TemporalTilingConfig, TilingConfig, decode_tiled
    from ltx_2_mlx_amd.pipelines import RetakePipeline
    tc = TilingConfig(SpatialTilingConfig(64, 32), TemporalTilingConfig(16, 8))
    pipe = RetakePipeline(parts.m, parts.enc, parts.dec)
    ctx, noise = parts.ctx.to(dev), parts.noise.to(dev)

    def seeded(fn):
        parts.dec.generator = torch.Generator(device=dev).manual_seed(11)
        try:
            return fn()
        finally:
            parts.dec.generator = None

    run = lambda **kw: seeded(lambda: pipe(None, ctx, None, _conf(distilled=True, tiling_config=tc, **kw), frames=parts.source, initial_noise=noise))
    video = run()
    assert video.dtype == torch.uint8 and video.shape == (17, 64, 96, 3)
    latent = pipe.denoise_latent(None, ctx, _conf(distilled=True), frames=parts.source, initial_noise=noise)
    hand = seeded(lambda: next(decode_tiled(latent, parts.dec, tc)))
    assert hand.dtype == torch.float32 and hand.shape == (1, 3, 17, 64, 96) and torch.equal(video, K.video_to_uint8(hand[0]))
    kept = run(composite_source=True, composite_ramp=0)
    src = torch.from_numpy(parts.source).to(dev)
    assert kept.dtype == torch.uint8 and torch.equal(kept[0], src[0]) and torch.equal(kept[9:], src[9:]) and torch.equal(kept[1:9], video[1:9])
    faded = run(composite_source=True, composite_ramp=2)
    assert np.array_equal(faded.cpu().numpy(), RR.composite(video.cpu().numpy(), parts.source, 1, 9, 2))


# ------------------------------------------------------------------ 6. the CLI
def test_generate_video_retake(dev, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    rng = np.random.default_rng(6)
    clip = rng.integers(0, 256, (20, 64, 96, 3), dtype=np.uint8)             # 20 frames are snapped down to 17
    path = tmp_path / "clip.npy"
    np.save(path, clip)
    frames = generate.generate_video("p", retake_video=str(path), retake_start_time=0.4, retake_end_time=0.7, output_fps=24, use_gemma=False,
                                     num_layers=2, num_heads=2, vae_base_channels=64, retake_composite=True, seed=3, save_mp4=False,
                                     output_path=str(tmp_path / "v.mp4"))
    assert frames.dtype == torch.uint8 and frames.shape == (17, 64, 96, 3)
    saved = np.load(tmp_path / "v.npz")["frames"]
    assert saved.shape == (17, 64, 96, 3) and np.array_equal(saved, frames.cpu().numpy())
    assert np.array_equal(saved[13:], clip[13:17]) and not np.array_equal(saved[1:9], clip[1:9])          # beyond the 4-frame fade: the source
    out = capsys.readouterr().out
    assert "Using Retake Pipeline" in out and "latent frames [1, 2) of 3, 18 DiT tokens" in out and "0.4s - 0.7s" in out
