"""IC-LoRA on the GPU: Canny and its hysteresis against the numpy restatement (every pixel), frames_to_patches against the torch glue (every
bit), encode_patches against the encoder's own entry, stage 1 of the pipeline against a hand composition of the existing pieces and against
the fp32 restatement, the adapter's fuse / restore, and the CLI.  Tiny models as tests/test_parity.py builds them (2 heads x 128, 2 layers,
caption 128)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import measure, rel_l2

import canny_ref as CR
import ic_lora_ref as IR
from test_parity import make_dit, make_vae, pearson

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = [torch.bfloat16, torch.float16]
GUARD = 0x5A


def _tile():
    from ltx_2_mlx_amd import kernels as K
    return K.CANNY_TILE


def _guarded(shape, dev):
    """A uint8 buffer filled with GUARD and its leading window of `shape`: nothing behind the window may change."""
    n = int(np.prod(shape))
    buf = torch.full((n + 256,), GUARD, dtype=torch.uint8, device=dev)
    return buf, buf[:n].view(shape)


def _intact(buf, shape):
    return bool((buf[int(np.prod(shape)):] == GUARD).all())


# ------------------------------------------------------------------ 1. Canny
THRESHOLDS = [(100, 200), (200, 100), (0, 0), (50.7, 120.2)]
_canny_cases = {}


def _images(shape):
    """uniform noise; noise blurred to about 4 px at a contrast of 80 grey levels per standard deviation (long connected edges, strong and
    weak pixels mixed, at every threshold pair); a constant image"""
    from scipy import ndimage
    rng = np.random.default_rng(sum(shape))
    noise = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    b = ndimage.gaussian_filter(rng.random(shape + (3,)), sigma=(0, 4, 4, 0), mode="nearest")
    blurred = np.clip(np.round((b - b.mean()) / b.std() * 80 + 128), 0, 255).astype(np.uint8)
    return {"noise": noise, "blurred": blurred, "constant": np.full(shape + (3,), 131, np.uint8)}


def _canny_case(shape):
    if shape not in _canny_cases:
        imgs = _images(shape)
        _canny_cases[shape] = (imgs, {(k, t): CR.canny(v, *t) for k, v in imgs.items() for t in THRESHOLDS})
    return _canny_cases[shape]


@pytest.mark.parametrize("which", ["below_one_tile", "remainders", "several_tiles"])
def test_canny_equals_restatement(dev, which):
    """Every pixel equal, for every image and threshold pair; nothing written behind `edges`."""
    from ltx_2_mlx_amd import kernels as K
    th, tw = _tile()
    shape = {"below_one_tile": (1, 5, 7), "remainders": (3, 33, 70), "several_tiles": (2, 2 * th + 3, 3 * tw + 5)}[which]
    imgs, refs = _canny_case(shape)
    for name, img in imgs.items():
        x = torch.from_numpy(img).to(dev)
        for t in THRESHOLDS:
            buf, out = _guarded(shape, dev)
            got, passes = K.canny(x, *t, out=out, return_passes=True)
            want = refs[(name, t)]
            bad = int((got.cpu().numpy() != want).sum())
            assert bad == 0, f"{name} {t}: {bad} of {want.size} pixels differ"
            assert _intact(buf, shape) and 1 <= passes <= shape[1] * shape[2] + 1, (name, t, passes)
            if name == "constant":
                assert not want.any()
            elif t == (100, 200) and min(shape[1:]) > 8:
                assert want.any() and not want.all()                 # the case says something
    assert np.array_equal(refs[("noise", (100, 200))], refs[("noise", (200, 100))])
    with pytest.raises(ValueError, match="canny"):
        K.canny(torch.zeros(1, 4, 4, 1, dtype=torch.uint8, device=dev))
    # a caller's `out` must be exactly what the kernel writes: too small, another dtype, not contiguous, on the host
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=dev)
    for bad in (torch.zeros(1, 8, 7, dtype=torch.uint8, device=dev), torch.zeros(1, 8, 8, dtype=torch.int32, device=dev),
                torch.zeros(1, 8, 16, dtype=torch.uint8, device=dev)[:, :, ::2], torch.zeros(1, 8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out must be"):
            K.canny(x, out=bad)
        with pytest.raises(ValueError, match="out must be"):
            K.canny_hysteresis(x[..., 0], out=bad)
    with pytest.raises(ValueError, match="uint8"):
        K.canny(torch.zeros(1, 4, 4, 3, device=dev))


def test_hysteresis_on_crafted_maps(dev):
    """The second stage on maps no image produces reliably: a one-pixel serpentine of weak pixels over 3 x 3 tiles with one strong pixel at
    its end (the path crosses tile borders in all four directions, so it takes many passes), the same without the strong pixel, two frames
    of which only the first holds it, diagonal-only connections across a tile corner, and random maps."""
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    th, tw = _tile()
    h, w = 3 * th + 1, 3 * tw + 2
    weak, start = CR.serpentine(h, w)
    strong = weak.copy()
    strong[start] = 2
    corner = np.zeros((2, h, w), np.uint8)
    corner[0, th - 1, tw - 1], corner[0, th, tw] = 2, 1                       # down-right across the corner of four tiles
    corner[0, 2 * th, tw - 1], corner[0, 2 * th - 1, tw] = 2, 1               # up-right across another
    corner[1, th - 1, 2 * tw], corner[1, th, 2 * tw - 1] = 1, 2               # the weak pixel up-right of the strong one
    corner[1, 5, 5], corner[1, 5, 7] = 2, 1                                   # two apart: not connected
    rng = np.random.default_rng(11)
    u = rng.random((3, h, w))
    random = np.where(u < 0.003, 2, np.where(u < 0.45, 1, 0)).astype(np.uint8)
    cases = {"serpentine": strong[None], "no strong pixel": weak[None], "second frame empty": np.stack([strong, weak]), "corners": corner,
             "random": random}
    passes = {}
    for name, m in cases.items():
        want = CR.hysteresis(m)
        buf, out = _guarded(m.shape, dev)
        got, passes[name] = K.canny_hysteresis(torch.from_numpy(m).to(dev), out=out, return_passes=True)
        bad = int((got.cpu().numpy() != want).sum())
        assert bad == 0 and _intact(buf, m.shape), f"{name}: {bad} of {want.size} pixels differ"
        assert np.array_equal(want, np.stack([CR.hysteresis_flood(f) for f in m])), name
    assert CR.hysteresis(cases["serpentine"]).sum() == 255 * int((weak != 0).sum())
    assert not CR.hysteresis(cases["no strong pixel"]).any() and not CR.hysteresis(cases["second frame empty"])[1].any()
    c = CR.hysteresis(corner)
    assert c[0, th, tw] == 255 and c[0, 2 * th - 1, tw] == 255 and c[1, th - 1, 2 * tw] == 255 and c[1, 5, 7] == 0
    print(f"hysteresis passes: {passes}")
    assert passes["no strong pixel"] == 1 and 3 < passes["serpentine"] <= h * w + 1
    dmap = torch.from_numpy(strong[None]).to(dev)
    with pytest.raises(ValueError, match="in place"):
        ws = torch.zeros(nv.CANNY_FLAG_BYTES, dtype=torch.uint8, device=dev)
        nv.check(nv.lib().ltx2_canny_hysteresis(nv.ptr(dmap), 1, h, w, nv.ptr(dmap), nv.ptr(ws), ws.numel(), None, nv.stream()))
    with pytest.raises(ValueError, match="workspace"):
        nv.check(nv.lib().ltx2_canny_hysteresis(nv.ptr(dmap), 1, h, w, nv.ptr(torch.empty_like(dmap)), nv.ptr(ws), 4, None, nv.stream()))


# ------------------------------------------------------------------ 2. frames_to_patches
def _glue(frames, dev, build):
    """patchify_video on frames / 127.5 - 1 formed on the host, as the reference's load_control_signal_tensor forms it (an IEEE division);
    the float16 build's yardstick is the same layout glue with the one rounding to float16."""
    from ltx_2_mlx_amd.model.video_vae_encoder import patchify_video
    from ltx_2_mlx_amd.pipelines import load_control_signal_tensor
    rgb = frames if frames.shape[-1] == 3 else np.repeat(frames, 3, axis=-1)
    v = load_control_signal_tensor(rgb)[0].to(dev)
    if build == torch.bfloat16:
        return patchify_video(v)
    c, f, h, w = v.shape
    out = torch.zeros(f, h // 4, w // 4, 64, device=dev, dtype=build)
    out[..., :48] = v.reshape(c, f, h // 4, 4, w // 4, 4).permute(1, 2, 4, 0, 5, 3).reshape(f, h // 4, w // 4, 48).to(build)
    return out


@pytest.mark.parametrize("shape", [(1, 32, 32), (9, 64, 96)])
@pytest.mark.parametrize("cin", [3, 1])
@pytest.mark.parametrize("build", BUILDS)
def test_frames_to_patches_equals_glue(dev, build, cin, shape):
    from ltx_2_mlx_amd import kernels as K
    rng = np.random.default_rng(shape[0] * 7 + cin)
    frames = rng.integers(0, 256, shape + (cin,), dtype=np.uint8)
    frames.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)                 # every value once, 0, 127, 128 and 255 among them
    frames.reshape(-1)[-4:] = (0, 127, 128, 255)
    want = _glue(frames, dev, build)
    f, h, w = shape
    n = f * (h // 4) * (w // 4) * 64
    buf = torch.full((n + 64,), 1.5, dtype=build, device=dev)                 # a non-zero pattern under the output and behind it
    out = buf[:n].view(f, h // 4, w // 4, 64)
    got = K.frames_to_patches(torch.from_numpy(frames).to(dev), dtype=build, out=out)
    assert got.dtype == build and got.shape == want.shape
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{int((got.view(torch.int16) != want.view(torch.int16)).sum())} of {n} elements differ"
    assert bool((got[..., 48:].view(torch.int16) == 0).all()) and bool((buf[n:] == 1.5).all())
    if cin == 1:                                                              # (F, H, W) is the same clip
        assert torch.equal(K.frames_to_patches(torch.from_numpy(frames[..., 0]).to(dev), dtype=build).view(torch.int16), want.view(torch.int16))
    for bad in (torch.zeros(f, h // 4, w // 4, 48, dtype=build, device=dev), torch.zeros(f, h // 4, w // 4, 64, device=dev),
                torch.zeros(f, h // 4, w // 4, 64, dtype=torch.float16 if build == torch.bfloat16 else torch.bfloat16, device=dev)):
        with pytest.raises(ValueError, match="out must be"):                  # `out` of another build's type must not select that build
            K.frames_to_patches(torch.from_numpy(frames).to(dev), dtype=build, out=bad)
    with pytest.raises(ValueError, match="dtype"):
        K.frames_to_patches(torch.from_numpy(frames).to(dev), dtype=torch.float32)
    with pytest.raises(ValueError, match="Cin"):
        K.frames_to_patches(torch.zeros(1, 8, 8, 2, dtype=torch.uint8, device=dev), dtype=build)
    with pytest.raises(ValueError, match="multiples of 4"):
        K.frames_to_patches(torch.zeros(1, 8, 6, 3, dtype=torch.uint8, device=dev), dtype=build)


# ------------------------------------------------------------------ shared models
class Parts:
    pass


@pytest.fixture(scope="module")
def parts(dev):
    from oracle import vae_encoder as oenc
    from ltx_2_mlx_amd.model.upscaler import SpatialUpscaler
    from ltx_2_mlx_amd.model.video_vae_encoder import SimpleVideoEncoder
    p = Parts()
    p.cfg, p.wq, p.m = make_dit(dev, heads=2, layers=2, cap=128)
    w = oenc.make_encoder_weights(seed=51)
    p.enc_wq = {k: (v.to(torch.bfloat16).float() if v.dim() == 5 else v) for k, v in w.items()}
    p.enc = SimpleVideoEncoder(device=dev)
    p.enc.load_state_dict(w)
    _, _, p.dec = make_vae(dev, layers=1)
    p.up = SpatialUpscaler(in_channels=128, mid_channels=64, num_blocks_per_stage=1, device=dev)
    p.up.init_random_weights(seed=3)
    g = torch.Generator().manual_seed(91)
    p.ctx = 0.1 * torch.randn(1, 64, 128, generator=g)
    p.control = torch.randint(0, 256, (9, 64, 96, 3), generator=g, dtype=torch.uint8).numpy()          # at stage 1's resolution
    p.noise1 = torch.randn(1, 24, 128, generator=g)                                                     # 12 free + 12 control tokens
    p.noise2 = torch.randn(1, 48, 128, generator=g)
    return p


@pytest.mark.parametrize("frames", [9, 17])
def test_encode_patches_equals_encoder(dev, parts, frames):
    """encode_patches(patchify_video(v)) == encoder(v) bit for bit; 17 frames pass both temporal downsamples with more than one frame."""
    from ltx_2_mlx_amd.model.video_vae_encoder import patchify_video
    g = torch.Generator().manual_seed(frames)
    v = (torch.rand(1, 3, frames, 64, 96, generator=g) * 2 - 1).to(dev)
    want = parts.enc(v)
    got = parts.enc.encode_patches(patchify_video(v[0]))
    assert want.shape == (1, 128, 1 + (frames - 1) // 8, 2, 3) and torch.equal(got, want) and bool(torch.isfinite(got).all())
    with pytest.raises(ValueError, match="patches"):
        parts.enc.encode_patches(patchify_video(v[0, :, :8]))
    with pytest.raises(ValueError, match="bfloat16"):
        parts.enc.encode_patches(patchify_video(v[0]).float())


# ------------------------------------------------------------------ 3. stage 1
STAGE1_MEASURED = 2.702e-4    # rel-L2 of the stage-1 latent against the fp32 restatement, measured on the MI355X (Pearson 1.000000)


def _conf(**kw):
    from ltx_2_mlx_amd.pipelines import ICLoraConfig
    return ICLoraConfig(height=128, width=192, num_frames=9, **kw)


def _video(parts, **kw):
    from ltx_2_mlx_amd.pipelines import VideoCondition
    return [VideoCondition(video_path=None, strength=0.95, frames=parts.control, **kw)]


def _hand_stage1(parts, dev, model):
    """Stage 1 from the pieces that existed before the pipeline: the encoder's own entry on the host-normalised clip,
    VideoConditionByKeyframeIndex, GaussianNoiser with the given noise, the conditioned loop (captured)."""
    from ltx_2_mlx_amd.components import DISTILLED_SIGMA_VALUES, EulerDiffusionStep, GaussianNoiser, VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning.keyframe import VideoConditionByKeyframeIndex
    from ltx_2_mlx_amd.conditioning.tools import VideoLatentTools
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import joint_denoise_loop, load_control_signal_tensor
    from ltx_2_mlx_amd.types import VideoLatentShape
    tools = VideoLatentTools(patchifier=VideoLatentPatchifier(patch_size=1), target_shape=VideoLatentShape(1, 128, 2, 2, 3), fps=24.0)
    latent = parts.enc(load_control_signal_tensor(parts.control).to(dev))
    state = VideoConditionByKeyframeIndex(latent, frame_idx=0, strength=0.95).apply_to(tools.create_initial_state(dtype=torch.float32, device=dev), tools)
    state = GaussianNoiser()(state, noise_scale=1.0, noise=parts.noise1.to(dev))
    sig = [float(s) for s in DISTILLED_SIGMA_VALUES[:8]]
    state = joint_denoise_loop(X0Model(model), False, state, None, sig, parts.ctx.to(dev), None, EulerDiffusionStep(), None, True)[0]
    return tools.unpatchify(tools.clear_conditioning(state)).latent


def test_stage1_equals_hand_composition_and_restatement(dev, parts):
    """Stage 1 of a 128x192x9 request (64x96: 2x2x3 latent frames, 12 free and 12 control tokens), control strength 0.95, the 7 default steps,
    the same noise everywhere.  Bit for bit the loop composed by hand from the existing pieces; against tests/ic_lora_ref.stage1 (oracle VAE
    encoder, oracle DiT, fp32 loop) the gate is 5 x the rel-L2 measured on the MI355X, 2.702e-04, and Pearson > 0.999 (measured 1.000000).
    The appended control tokens are cut off before the comparison, so the figure is the 12 free tokens' alone."""
    from oracle import dit, vae_encoder as oenc
    from ltx_2_mlx_amd.components import DISTILLED_SIGMA_VALUES
    from ltx_2_mlx_amd.pipelines import ICLoraPipeline
    pipe = ICLoraPipeline(parts.m, parts.enc, None, parts.up)
    seen = []
    out = pipe.stage1_latent(parts.ctx.to(dev), _conf(), None, _video(parts), initial_noise=parts.noise1.to(dev))
    assert out.shape == (1, 128, 2, 2, 3) and pipe.token_counts == [24] and bool(torch.isfinite(out).all())
    assert torch.equal(out, _hand_stage1(parts, dev, parts.m))
    eager = pipe.stage1_latent(parts.ctx.to(dev), _conf(), None, _video(parts), callback=lambda *a: seen.append(a), initial_noise=parts.noise1.to(dev))
    assert torch.equal(eager, out) and seen == [("stage1_iclora", i + 1, 7) for i in range(7)]
    sig = [float(s) for s in DISTILLED_SIGMA_VALUES[:8]]
    x0 = lambda x, ts, s, pos: dit.x0_model(x, parts.ctx, ts, pos, parts.wq, parts.cfg)
    ref = IR.stage1([oenc.encoder_forward(IR.control_tensor(parts.control), parts.enc_wq)], [0.95], (2, 2, 3), 24.0, parts.noise1, x0, sig)
    err = measure("ic-lora stage 1 vs fp32 restatement", rel_l2(out.cpu(), ref))
    r = pearson(out.cpu(), ref)
    print(f"ic-lora pipeline, stage 1: rel-L2 = {err:.4e}  pearson = {r:.6f}")
    assert err <= 5 * STAGE1_MEASURED and r > 0.999


def test_adapter_fuse_and_restore(dev, parts, tmp_path):
    """A random rank-4 LoRA on attn1 and ff: stage 1 runs under it, stage 2 on the base weights, and the model is left as it was."""
    from oracle import dit
    from safetensors.torch import save_file
    from ltx_2_mlx_amd.components import STAGE_2_DISTILLED_SIGMA_VALUES, EulerDiffusionStep, GaussianNoiser, VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning.tools import VideoLatentTools
    from ltx_2_mlx_amd.loader.lora_loader import LoRAConfig, fuse_lora_into_weights
    from ltx_2_mlx_amd.model.transformer import LTXModel, X0Model
    from ltx_2_mlx_amd.model.upscaler import upscale_latent
    from ltx_2_mlx_amd.pipelines import ICLoraPipeline, create_ic_lora_pipeline, joint_denoise_loop
    from ltx_2_mlx_amd.types import VideoLatentShape
    g = torch.Generator().manual_seed(92)
    lora = {}
    for name, (o, i) in (("transformer_blocks.0.attn1.to_k", (256, 256)), ("transformer_blocks.1.attn1.to_out.0", (256, 256)),
                         ("transformer_blocks.1.ff.net.0.proj", (1024, 256))):
        lora[f"diffusion_model.{name}.lora_A.weight"] = 0.3 * torch.randn(4, i, generator=g)
        lora[f"diffusion_model.{name}.lora_B.weight"] = 0.3 * torch.randn(o, 4, generator=g)
    path = str(tmp_path / "ic_lora.safetensors")
    save_file(lora, path)
    ctx = parts.ctx.to(dev)
    kw = dict(initial_noise=parts.noise1.to(dev), stage2_noise=parts.noise2.to(dev))
    plain = ICLoraPipeline(parts.m, parts.enc, None, parts.up)
    pipe = create_ic_lora_pipeline(parts.m, parts.enc, None, parts.up, base_transformer_weights=None, lora_configs=[LoRAConfig(path, 1.0)])
    before = {k: v.clone() for k, v in parts.m.weight_tensors().items()}
    s1_plain = plain.stage1_latent(ctx, _conf(), None, _video(parts), initial_noise=kw["initial_noise"])
    s1 = pipe.stage1_latent(ctx, _conf(), None, _video(parts), initial_noise=kw["initial_noise"])
    final = pipe.denoise_latent(ctx, _conf(), None, _video(parts), **kw)
    after = parts.m.weight_tensors()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)      # the originals are back, bit for bit
    assert bool(torch.isfinite(s1).all()) and not torch.equal(s1, s1_plain)
    assert torch.equal(plain.stage1_latent(ctx, _conf(), None, _video(parts), initial_noise=kw["initial_noise"]), s1_plain)
    # a model LOADED with the fused weights gives the same stage-1 bits
    sd = {k: (v.to(dev, torch.bfloat16) if (k.endswith(".weight") and v.dim() == 2) else v.to(dev)) for k, v in dit.make_dit_weights(parts.cfg, 0).items()}
    fused = LTXModel(num_attention_heads=2, attention_head_dim=128, num_layers=2, caption_channels=128, device=dev)
    fused.load_state_dict(fuse_lora_into_weights(sd, [LoRAConfig(path, 1.0)], verbose=False))
    assert torch.equal(_hand_stage1(parts, dev, fused), s1)
    # stage 2 by hand on the BASE model from that stage-1 latent: the bracketed x2 upscale, the noise at sigma_0, three steps
    assert final.shape == (1, 128, 2, 4, 6) and pipe.token_counts == [24, 48]
    stats = parts.enc.per_channel_statistics
    tools = VideoLatentTools(patchifier=VideoLatentPatchifier(patch_size=1), target_shape=VideoLatentShape(1, 128, 2, 4, 6), fps=24.0)
    state = tools.create_initial_state(dtype=torch.float32, initial_latent=upscale_latent(s1, parts.up, stats.mean_of_means, stats.std_of_means))
    sig2 = [float(s) for s in STAGE_2_DISTILLED_SIGMA_VALUES]
    state = GaussianNoiser()(state, noise_scale=sig2[0], noise=kw["stage2_noise"])
    state = joint_denoise_loop(X0Model(parts.m), False, state, None, sig2, ctx, None, EulerDiffusionStep(), None, True)[0]
    assert torch.equal(final, tools.unpatchify(state).latent)
    with pytest.raises(ValueError, match="requires spatial_upscaler"):
        ICLoraPipeline(parts.m, parts.enc, None, None).denoise_latent(ctx, _conf())
    # decoded: uint8 frames of the request's size
    video = ICLoraPipeline(parts.m, parts.enc, parts.dec, parts.up)(ctx, None, _conf(), None, _video(parts), **kw)
    assert video.dtype == torch.uint8 and video.shape == (9, 128, 192, 3)


# ------------------------------------------------------------------ 4. the CLI
def test_generate_video_ic_lora(dev, tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    from ltx_2_mlx_amd import kernels as K
    rng = np.random.default_rng(3)
    ctrl = tmp_path / "ctrl.npy"
    np.save(ctrl, rng.integers(0, 256, (5, 64, 96, 3), dtype=np.uint8))       # short: padded with its last frame
    calls = []
    real = K.canny

    def spy(frames, low, high, **kw):
        calls.append((frames.device.type, frames.dtype, tuple(frames.shape), low, high))
        return real(frames, low, high, **kw)

    monkeypatch.setattr(K, "canny", spy)
    frames = generate.generate_video("a test prompt", pipeline_type="ic-lora", control_video=str(ctrl), control_type="canny", save_control=True,
                                     canny_low=60, canny_high=160, spatial_upscaler_weights="random", use_gemma=False, num_steps=3, height=128,
                                     width=192, num_frames=9, seed=3, num_layers=2, num_heads=2, vae_base_channels=64,
                                     output_path=str(tmp_path / "v.mp4"))
    assert frames.dtype == torch.uint8 and frames.shape == (9, 128, 192, 3)
    saved = np.load(tmp_path / "v.npz")["frames"]
    assert saved.shape == (9, 128, 192, 3) and np.array_equal(saved, frames.cpu().numpy())
    assert calls == [("cuda", torch.uint8, (9, 64, 96, 3), 60, 160)]                      # the device path, at stage 1's resolution
    side = tmp_path / "ctrl_canny.mp4"
    assert side.exists() or len(os.listdir(tmp_path / "ctrl_canny_frames")) == 9          # PNG frames where there is no ffmpeg binary
    out = capsys.readouterr().out
    assert "Using IC-LoRA Pipeline" in out and "DiT tokens per stage [24, 48]" in out and "no --ic-lora-weights" in out
