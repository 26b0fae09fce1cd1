"""Temporal x2 latent upscaler, host side: the fp32 restatement (tests/temporal_upscaler_ref.py) against the vector recorded from the
reference's own TemporalUpscaler, the MLX GroupNorm definition, the two shuffle packings, the C ABI entry and the generate_video
routing.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import temporal_upscaler_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "temporal_upscaler_tiny.npz")


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_restatement_matches_the_reference_vector():
    """Reference mode of the restatement against tests/golden/temporal_upscaler_tiny.npz (the reference's own TemporalUpscaler over the
    shim) at the tolerance test_upscaler_matches_reference uses; the checkpoint semantics give something else on the same input."""
    z = np.load(GOLDEN)
    assert list(z["config"]) == [R.TINY.latent_channels, R.TINY.hidden_channels, R.TINY.num_res_blocks, R.TINY.num_groups]
    assert int(z["weight_seed"]) == R.TINY_SEED and int(z["input_seed"]) == R.TINY_INPUT_SEED
    x = R.tiny_input()
    assert np.array_equal(x.numpy(), z["x"])
    w = R.make_weights(R.TINY, R.TINY_SEED)
    y = R.forward(x, w, R.TINY, checkpoint_semantics=False)
    assert y.shape == (1, 64, 5, 5, 6)
    np.testing.assert_allclose(y.numpy(), z["y"], rtol=2e-4, atol=2e-5)
    other = R.forward(x, w, R.TINY, checkpoint_semantics=True)
    assert other.shape == y.shape
    assert _rel_l2(other, torch.from_numpy(z["y"])) > 1e-2          # the test can tell the two semantics apart


def _mlx_group_norm_f64(x, weight, bias, groups, eps, pytorch_compatible):
    """mlx.nn.GroupNorm from its definition, float64 numpy: default x.reshape(batch, -1, groups), mean / biased variance over axis 1;
    pytorch_compatible x.reshape(batch, -1, groups, group_size) normalised over (positions, group_size)."""
    x = x.astype(np.float64)
    batch, dims = x.shape[0], x.shape[-1]
    if pytorch_compatible:
        g = x.reshape(batch, -1, groups, dims // groups)
        mean, var = g.mean(axis=(1, 3), keepdims=True), g.var(axis=(1, 3), keepdims=True)
    else:
        g = x.reshape(batch, -1, groups)
        mean, var = g.mean(axis=1, keepdims=True), g.var(axis=1, keepdims=True)
    return ((g - mean) / np.sqrt(var + eps)).reshape(x.shape) * weight.astype(np.float64) + bias.astype(np.float64)


@pytest.mark.parametrize("compatible", [False, True])
def test_shim_group_norm_follows_the_mlx_definition(compatible):
    from tools import mlx_shim as shim
    rs = np.random.RandomState(3)
    x = (rs.randn(3, 5, 6, 64) * (1 + np.arange(3))[:, None, None, None] + np.arange(3)[:, None, None, None]).astype(np.float32)
    gn = shim.GroupNorm(32, 64, pytorch_compatible=compatible)
    gn.weight, gn.bias = shim.Arr(torch.from_numpy(rs.randn(64).astype(np.float32))), shim.Arr(torch.from_numpy(rs.randn(64).astype(np.float32)))
    got = gn(shim.Arr(torch.from_numpy(x))).t.numpy()
    ref = _mlx_group_norm_f64(x, gn.weight.t.numpy(), gn.bias.t.numpy(), 32, 1e-5, compatible)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5)
    # the restatement's per-frame norm is the same function on (B, C, T, H, W)
    mine = R.group_norm_frames(torch.from_numpy(x).permute(3, 0, 1, 2)[None], gn.weight.t, gn.bias.t, 32, 1e-5, interleaved=not compatible)
    np.testing.assert_allclose(mine[0].permute(1, 2, 3, 0).numpy(), ref, rtol=2e-5, atol=2e-5)
    # and the other grouping is a different function
    other = _mlx_group_norm_f64(x, gn.weight.t.numpy(), gn.bias.t.numpy(), 32, 1e-5, not compatible)
    assert np.linalg.norm(other - ref) / np.linalg.norm(ref) > 1e-2


def test_shuffle_packing_on_an_index_ramp():
    """Reference: out[c, 2t + p] = in[p * C + c, t]; upstream: in[2c + p, t]; the forward pass then drops frame 0."""
    C, T = 4, 3
    x = (torch.arange(2 * C)[:, None] * 100 + torch.arange(T)[None, :]).float().reshape(1, 2 * C, T, 1, 1)
    ref, ups = R.temporal_pixel_shuffle(x, False), R.temporal_pixel_shuffle(x, True)
    assert ref.shape == ups.shape == (1, C, 2 * T, 1, 1)
    for c in range(C):
        for t in range(T):
            for p in range(2):
                assert float(ref[0, c, 2 * t + p, 0, 0]) == (p * C + c) * 100 + t
                assert float(ups[0, c, 2 * t + p, 0, 0]) == (2 * c + p) * 100 + t
    assert float(ref[:, :, 1:][0, 1, 0, 0, 0]) == (1 * C + 1) * 100 + 0      # first kept frame is (t = 0, p = 1)
    # the engine's depth-to-space row order n' = s * Cf + c IS the reference packing; the upstream packing needs the d2s permutation
    from ltx_2_mlx_amd import kernels as K
    w = torch.arange(2 * C).float().reshape(2 * C, 1, 1, 1, 1).expand(2 * C, 1, 3, 3, 3)
    assert K.conv_weight_to_engine(w, dtype=torch.float32)[:, 0, 0].tolist() == list(range(2 * C))
    assert K.conv_weight_to_engine(w, d2s_stride=(2, 1, 1), dtype=torch.float32)[:, 0, 0].tolist() == [2 * c + p for p in range(2) for c in range(C)]
    assert K.conv_bias_to_engine(torch.arange(2 * C).float(), (2, 1, 1)).tolist() == [2 * c + p for p in range(2) for c in range(C)]


def test_entry_is_declared_bound_and_documented():
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    name = "ltx2_groupnorm_frames_silu"
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", header)
    assert m, "not declared in include/ltx2hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 14 and params[3] == "int frames" and params[4] == "int64_t P_frame" and params[7] == "int interleaved"
    res, args = nv.SIGNATURES[name]
    assert res is nv.i32 and len(args) == 14 and args[3] is nv.i32 and args[4] is nv.i64 and args[8] is nv.f32
    assert nv.ABI_VERSION == 3 and "#define LTX2_ABI_VERSION 3" in header
    assert "temporal.py:128-147" in header
    assert callable(K.groupnorm_frames_silu)
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert name in open(os.path.join(ROOT, "ltx-2-mlx_amd", "csrc", "capi.hip")).read()


def test_load_state_dict_refuses_a_wrong_shape_and_a_missing_key():
    from ltx_2_mlx_amd.model import TemporalUpscaler, load_temporal_upscaler_weights, upscale_latent_temporal  # noqa: F401
    with pytest.raises(RuntimeError):
        TemporalUpscaler(device="cpu")
    up = TemporalUpscaler(latent_channels=64, hidden_channels=64, num_res_blocks=1, num_groups=32, device="cuda")   # no GPU touched yet
    assert up.expected_weight_shapes() == R.weight_shapes(R.TINY)
    assert set(TemporalUpscaler(device="cuda").expected_weight_shapes()) == set(R.weight_shapes(R.TemporalUpscalerConfig()))
    w = R.make_weights(R.TINY, 1)
    missing = {k: v for k, v in w.items() if k != "post_upsample_res_blocks.0.norm2.bias"}
    with pytest.raises(KeyError, match="post_upsample_res_blocks.0.norm2.bias"):
        up.load_state_dict(missing)
    bad = dict(w)
    bad["upsampler.0.weight"] = torch.zeros(64, 64, 3, 3, 3)
    with pytest.raises(ValueError, match="upsampler.0.weight"):
        up.load_state_dict(bad)
    with pytest.raises(RuntimeError, match="weights not loaded"):
        up.forward_nhwc(torch.zeros(1))


def test_generate_video_routes_upscale_temporal(tmp_path, monkeypatch):
    """The AudioVideo branch refuses upscale_temporal before any model is loaded; the video-only branch reaches TemporalUpscaler with the
    debug-size widths, the semantics keyword and the spatial upscaler's "random" convention (constructor spied on, no GPU)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate as gen
    from ltx_2_mlx_amd.model import upscaler as U
    kw = dict(use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"), height=64, width=96, num_frames=9, num_steps=2,
              weights_path=None, upscale_temporal=True, temporal_upscaler_weights="random")
    with pytest.raises(NotImplementedError, match="upscale_temporal with the AudioVideo pipeline"):
        gen.generate_video("p", generate_audio=True, **kw)
    with pytest.raises(NotImplementedError, match="upscale_temporal"):
        gen.generate_video("p", two_stage_distilled=True, spatial_upscaler_weights="random", **kw)

    class Routed(Exception):
        pass

    def spy(*a, **k):
        raise Routed(a, k)
    monkeypatch.setattr(U, "TemporalUpscaler", spy)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)           # the placeholder loop ran on the CPU: nothing to wait for
    with pytest.raises(Routed) as e:
        gen.generate_video("p", use_placeholder=True, skip_vae=True, **kw)
    assert e.value.args[1] == dict(hidden_channels=512, num_res_blocks=4, checkpoint_semantics=False, device="cpu")
    with pytest.raises(Routed) as e:
        gen.generate_video("p", use_placeholder=True, skip_vae=True, vae_base_channels=64, temporal_upscaler_checkpoint_semantics=True, **kw)
    assert e.value.args[1] == dict(hidden_channels=64, num_res_blocks=1, checkpoint_semantics=True, device="cpu")
    # without weights the flag does nothing, as in the reference (`if upscale_temporal and temporal_upscaler_weights`)
    assert gen.generate_video("p", use_placeholder=True, skip_vae=True, **dict(kw, temporal_upscaler_weights=None)) is None
    lat = np.load(tmp_path / "o_latent.npz")["latent"]
    assert lat.shape == (1, 128, 2, 2, 3)
