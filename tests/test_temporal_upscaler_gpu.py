"""Temporal x2 latent upscaler on the MI355X: the per-frame GroupNorm kernel against a float64 restatement, the conv's temporal
depth-to-space epilogue against torch, TemporalUpscaler (both semantics) against the fp32 restatement and the reference's recorded
vector, and generate_video(upscale_temporal=True)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import measure, rel_l2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_upscaler_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, H16 = torch.bfloat16, torch.float16
EPS = float(np.float32(1e-5))            # the value the C ABI receives


def pearson(a, b):
    a = a.double().flatten() - a.double().mean()
    b = b.double().flatten() - b.double().mean()
    return float((a * b).sum() / (a.norm() * b.norm()))


def _ulp16(exact: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of the 16-bit format at |exact| (float64): 2^(floor(log2 |exact|) - mantissa bits), the subnormal spacing below the
    smallest normal."""
    mant, emin = (7, -126) if dtype == BF else (10, -14)
    e = torch.floor(torch.log2(exact.abs().clamp_min(2.0 ** -140))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def _gn_f64(x, res, gamma, beta, groups, interleaved, act, per_frame=True):
    """float64 restatement on the SAME 16-bit inputs: x [F][P][C]; group of channel c = c % G (interleaved) or c // (C/G)."""
    x = x.double()
    Fr, P, C = x.shape
    g = x.reshape(Fr, P, C // groups, groups) if interleaved else x.reshape(Fr, P, groups, C // groups)
    dims = ((1, 2) if interleaved else (1, 3)) if per_frame else ((0, 1, 2) if interleaved else (0, 1, 3))
    mean = g.mean(dim=dims, keepdim=True)
    var = g.var(dim=dims, keepdim=True, unbiased=False)
    v = ((g - mean) / torch.sqrt(var + EPS)).reshape(Fr, P, C) * gamma.double() + beta.double()
    if res is not None:
        v = v + res.double()
    return v * torch.sigmoid(v) if act else v


def _inputs(frames, P, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.arange(frames, dtype=torch.float32)
    offset = ((-1.0) ** f * 0.75 * (1 + f))[:, None, None]        # another offset and scale per frame: whole-clip statistics are wrong
    scale = (0.5 * (1 + f))[:, None, None]
    x = (offset + scale * torch.randn(frames, P, C, generator=g)).to(dtype)
    res = torch.randn(frames, P, C, generator=g).to(dtype)
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    return x, res, gamma, beta


# [frames][P_frame][C], groups.  With C = 512 and 32 groups a thread of the register form holds the positions r, r + R, ... of one vector
# column (R = 32 contiguous, 16 interleaved) in at most 24 register vectors: 768 / 384 positions per frame are the last that fit, 769 / 385
# and 1536 take the two-read form.  C = 36 is no multiple of 8: 8-byte vectors ([2][5][36] with 4 groups in both modes, with 6 groups
# contiguous, [1][700][36] two-read); 6 interleaved groups have no aligned tiling at all: the element-wise form.
SHAPES = [(3, 30, 64, 32), (1, 1, 128, 32), (2, 384, 512, 32), (2, 7, 96, 32), (1, 385, 512, 32), (1, 769, 512, 32), (1, 1536, 512, 32),
          (2, 5, 36, 6), (2, 5, 36, 4), (1, 700, 36, 6)]


@pytest.mark.parametrize("dtype", [BF, H16], ids=["bf16", "f16"])
@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "contiguous"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_frames_kernel_within_one_ulp(dev, shape, interleaved, dtype):
    """ltx2_groupnorm_frames_silu against the float64 value of the same 16-bit inputs: every element within one unit in the last place of
    the 16-bit output format AT the exact value.  The kernel takes its statistics and the affine in fp64 (sums of 16-bit values and of
    their squares are exact there), converts once to fp32 for the SiLU (v_exp_f32 / v_rcp_f32, ~1e-6 relative, multiplicative) and rounds
    once on store: |got - exact| <= ulp/2 + ~1e-6 |exact|.  With / without residual, with / without SiLU; two launches agree bit for bit."""
    from ltx_2_mlx_amd import kernels as K
    frames, P, C, G = shape
    x, res, gamma, beta = _inputs(frames, P, C, dtype, seed=P + C)
    xg, rg, gg, bg = x.to(dev), res.to(dev), gamma.to(dev), beta.to(dev)
    worst = 0.0
    for with_res in (False, True):
        for act in (True, False):
            got = K.groupnorm_frames_silu(xg, gg, bg, G, EPS, res=rg if with_res else None, act=act, interleaved=interleaved)
            again = K.groupnorm_frames_silu(xg, gg, bg, G, EPS, res=rg if with_res else None, act=act, interleaved=interleaved)
            torch.cuda.synchronize()
            assert got.shape == x.shape and got.dtype == dtype
            assert torch.equal(got.view(torch.int16), again.view(torch.int16))
            exact = _gn_f64(x, res if with_res else None, gamma, beta, G, interleaved, act)
            err = (got.cpu().double() - exact).abs() / _ulp16(exact, dtype)
            worst = max(worst, measure(f"groupnorm_frames |err| / ulp res={int(with_res)} act={int(act)}", err.max()))
            assert float(err.max()) <= 1.0, (with_res, act, float(err.max()))
            if frames > 1:      # the inputs do tell per-frame from whole-clip statistics
                clip = _gn_f64(x, res if with_res else None, gamma, beta, G, interleaved, act, per_frame=False)
                assert float((got.cpu().double() - clip).norm() / clip.norm()) > 0.1
    # the other grouping is another function (except where a group is the same set of channels either way)
    other = _gn_f64(x, None, gamma, beta, G, not interleaved, True)
    mine = _gn_f64(x, None, gamma, beta, G, interleaved, True)
    assert P * (C // G) == 1 or float((other - mine).norm() / mine.norm()) > 1e-2


@pytest.mark.parametrize("dtype", [BF, H16], ids=["bf16", "f16"])
def test_groupnorm_frames_zero_variance_and_bad_arguments(dev, dtype):
    """A single position of constant channels: variance 0, the output is [silu](beta + res).  A null operand and C % groups != 0 come
    back as an error code with a message (ValueError through the binding)."""
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    g = torch.Generator().manual_seed(9)
    x = torch.full((1, 1, 128), 1.5).to(dtype)
    res, gamma, beta = torch.randn(1, 1, 128, generator=g).to(dtype), torch.randn(128, generator=g), torch.randn(128, generator=g)
    for interleaved in (True, False):
        got = K.groupnorm_frames_silu(x.to(dev), gamma.to(dev), beta.to(dev), 32, EPS, res=res.to(dev), act=False, interleaved=interleaved)
        exact = beta.double() + res.double()
        assert float(((got.cpu().double() - exact).abs() / _ulp16(exact, dtype)).max()) <= 1.0
    xg = x.to(dev)
    with pytest.raises(ValueError, match="C % groups == 0"):
        K.groupnorm_frames_silu(xg, gamma.to(dev), beta.to(dev), 24, EPS)
    lib = nv.lib(dtype)
    y = torch.empty_like(xg)
    f32 = gamma.to(dev)
    rc = lib.ltx2_groupnorm_frames_silu(None, None, nv.ptr(y), 1, 1, 128, 32, 1, EPS, nv.ptr(f32), nv.ptr(f32), None, 1, nv.stream())
    assert rc == nv.E_INVALID and "null operand" in nv.last_error()
    rc = lib.ltx2_groupnorm_frames_silu(nv.ptr(xg), None, nv.ptr(y), 1, 1, 128, 32, 1, EPS, None, nv.ptr(f32), None, 1, nv.stream())
    assert rc == nv.E_INVALID and "null operand" in nv.last_error()


@pytest.mark.parametrize("upstream", [False, True], ids=["reference_packing", "upstream_packing"])
@pytest.mark.parametrize("T,H,W,Cin,Cout", [(3, 5, 6, 64, 128), (2, 4, 4, 512, 1024)])
def test_conv3d_temporal_depth_to_space(dev, T, H, W, Cin, Cout, upstream):
    """ltx2_conv3d_fused(mode=2, stride=(2, 1, 1), pad_zero=1) against conv3d + temporal shuffle + dropped first frame in float64 on the
    same bf16 operands.  Bound: the one rounding of the bf16 output is at most 2^-9 relative per element, so at most 2^-9 = 1.95e-3 in
    rel-L2; the fp32 accumulation over 27 * Cin terms adds < 1e-4."""
    from ltx_2_mlx_amd import kernels as K
    g = torch.Generator().manual_seed(T * 1000 + Cin)
    x = torch.randn(T, H, W, Cin, generator=g).to(BF)
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5).to(BF)
    b = 0.1 * torch.randn(Cout, generator=g)
    d2s = (2, 1, 1) if upstream else None
    out = K.conv3d(x.to(dev), K.conv_weight_to_engine(w.to(dev), d2s_stride=d2s), K.conv_bias_to_engine(b.to(dev), d2s), mode=2,
                   stride=(2, 1, 1), pad_zero=True)
    assert out.shape == (2 * T - 1, H, W, Cout // 2)
    full = F.conv3d(x.double().permute(3, 0, 1, 2)[None], w.double(), b.double(), padding=1)
    ref = R.temporal_pixel_shuffle(full, upstream)[:, :, 1:][0].permute(1, 2, 3, 0)
    assert measure("conv3d temporal d2s rel-L2", rel_l2(out.cpu().float(), ref)) < 2.0 ** -9 + 1e-4


# ---- model level: gates at <= 5x the rel-L2 measured on the MI355X against the fp32 restatement ----
def _tiny(dev, cs):
    from ltx_2_mlx_amd.model import TemporalUpscaler
    w = R.make_weights(R.TINY, R.TINY_SEED)
    up = TemporalUpscaler(latent_channels=64, hidden_channels=64, num_res_blocks=1, num_groups=32, device=dev, checkpoint_semantics=cs)
    up.load_state_dict(w)
    wq = {k: (v.to(BF).float() if v.dim() == 5 else v) for k, v in w.items()}
    return up, wq


# measured on the MI355X (bf16 activations through 5 / 19 convolutions): tiny 6.5e-3 (reference semantics; 7.7e-3 against the recorded
# reference vector) and 6.2e-3 (checkpoint semantics), bracket 3.7e-3, full width 9.5e-3
TINY_GATE = {False: 2e-2, True: 2e-2}
BRACKET_GATE = 1.2e-2
FULL_GATE = 3e-2


@pytest.mark.parametrize("cs", [False, True], ids=["reference_semantics", "checkpoint_semantics"])
def test_tiny_temporal_upscaler(dev, cs):
    """Tiny TemporalUpscaler (64 -> 64, 1 + 1 blocks, two channels per group) against the fp32 restatement on bf16-rounded conv weights,
    in both semantics; the reference semantics also against the vector recorded from the reference's own TemporalUpscaler."""
    up, wq = _tiny(dev, cs)
    x = R.tiny_input()
    out = up(x.to(dev))
    assert out.shape == (1, 64, 5, 5, 6) and out.dtype == torch.float32
    ref = R.forward(x, wq, R.TINY, checkpoint_semantics=cs)
    assert rel_l2(out.cpu(), ref) < TINY_GATE[cs] and pearson(out.cpu(), ref) > 0.999
    gold = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "temporal_upscaler_tiny.npz"))["y"])
    if cs:
        assert rel_l2(out.cpu(), gold) > 0.5            # the other semantics is another function
    else:
        assert rel_l2(out.cpu(), gold) < TINY_GATE[cs] and pearson(out.cpu(), gold) > 0.999


def test_upscale_latent_temporal_bracket(dev):
    from ltx_2_mlx_amd.model import upscale_latent_temporal
    up, wq = _tiny(dev, False)
    x = R.tiny_input()
    g = torch.Generator().manual_seed(5)
    mean, std = torch.randn(64, generator=g), 0.5 + torch.rand(64, generator=g)
    out = upscale_latent_temporal(x.to(dev), up, mean, std)
    ref = R.upscale_latent_temporal(x, wq, R.TINY, mean, std)
    assert out.shape == ref.shape == (1, 64, 5, 5, 6)
    assert rel_l2(out.cpu(), ref) < BRACKET_GATE and pearson(out.cpu(), ref) > 0.999


def test_full_width_temporal_upscaler(dev):
    """The released geometry (128 -> 512, 4 + 4 blocks, 32 groups of 16) on (1, 128, 3, 8, 8); the fp32 restatement runs on the GPU as
    the checker."""
    from ltx_2_mlx_amd.model import TemporalUpscaler
    cfg = R.TemporalUpscalerConfig()
    w = R.make_weights(cfg, 21)
    up = TemporalUpscaler(device=dev)
    up.load_state_dict(w)
    wq = {k: (v.to(BF).float() if v.dim() == 5 else v).to(dev) for k, v in w.items()}
    x = torch.randn(1, 128, 3, 8, 8, generator=torch.Generator().manual_seed(22))
    out = up(x.to(dev))
    ref = R.forward(x.to(dev), wq, cfg)
    assert out.shape == ref.shape == (1, 128, 5, 8, 8)
    assert rel_l2(out.cpu(), ref.cpu()) < FULL_GATE and pearson(out.cpu(), ref.cpu()) > 0.999


def test_generate_video_upscale_temporal(dev, tmp_path):
    """generate_video(upscale_temporal=True, temporal_upscaler_weights="random") at the smallest CLI geometry: 2 latent frames become 3,
    the decoder returns 16 * (F_latent - 1) + 1 = 17 frames instead of 9, and the file that save_video writes holds as many."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    kw = dict(height=64, width=96, num_frames=9, num_steps=2, seed=3, num_layers=2, num_heads=2, vae_base_channels=64, use_gemma=False,
              weights_path=None)
    base = generate.generate_video("p", output_path=str(tmp_path / "a.mp4"), **kw)
    frames = generate.generate_video("p", output_path=str(tmp_path / "b.mp4"), upscale_temporal=True, temporal_upscaler_weights="random", **kw)
    f_latent = np.load(tmp_path / "a_latent.npz")["latent"].shape[2]
    assert f_latent == 2 and base.shape == (9, 64, 96, 3)
    assert np.load(tmp_path / "b_latent.npz")["latent"].shape == (1, 128, 2 * f_latent - 1, 2, 3)
    assert frames.shape == (16 * (f_latent - 1) + 1, 64, 96, 3) and frames.dtype == torch.uint8
    if shutil.which("ffmpeg"):          # save_video wrote an mp4: decode it once to the null muxer and read ffmpeg's own frame count
        assert os.path.exists(tmp_path / "b.mp4")
        r = subprocess.run(["ffmpeg", "-i", str(tmp_path / "b.mp4"), "-map", "0:v:0", "-f", "null", "-"], capture_output=True, text=True)
        counts = re.findall(r"frame=\s*(\d+)", r.stderr)
        assert r.returncode == 0 and counts and int(counts[-1]) == 17, r.stderr[-400:]
    else:                               # no ffmpeg binary: save_video falls back to one PNG per frame
        assert len(os.listdir(tmp_path / "b_frames")) == 17
