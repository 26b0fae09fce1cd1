"""The guided standard one-stage loop on the GPU: the per-channel statistics against the float64 two-pass formula within the derived bound, the
step kernel bit for bit against the separate fp32 torch ops, the engine entries against their parts, the captured loop against the per-step
loop, cross_attn_scale against scaled weights, the loops against the fp32 restatement, and generate_video end to end.  Tiny models as
tests/test_parity.py builds them."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import measure, rel_l2

import keyframe_ref as KR
import standard_cfg_ref as R
from test_parity import make_av, make_dit, pearson

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0
SIGMA, SIGMA_NEXT, CFG = 0.909375, 0.725, 3.0
SHAPES = [(37, 128), (5, 6), (33000, 128), (1, 128)]     # 16-byte form; element-wise form (C % 4 != 0); 256 blocks of rows, ragged chunks; n = 1
U64 = 2.0 ** -53


# ------------------------------------------------------------------ inputs, made once per shape
_cases = {}


def _case(rows, C, dev):
    """x, vc, vu and per-row timesteps of one shape.  Channel 0: mean = 100 x std (x = 100 + N(0, 1), velocities 1e-2 N(0, 1)); channel 1: the
    constant 3 (zero velocities: a = g = 3 exactly); channel 2: zero; the rest N(0, 1)."""
    if (rows, C) not in _cases:
        g = torch.Generator().manual_seed(rows * 131 + C)
        t = {k: torch.randn(rows, C, generator=g) for k in ("x", "vc", "vu")}
        t["x"][:, 0] += 100.0
        t["vc"][:, 0] *= 1e-2
        t["vu"][:, 0] *= 1e-2
        t["x"][:, 1] = 3.0
        t["x"][:, 2] = 0.0
        for k in ("vc", "vu"):
            t[k][:, 1:3] = 0.0
        t["ts_row"] = torch.rand(rows, generator=g) * SIGMA
        _cases[(rows, C)] = {k: v.to(dev) for k, v in t.items()}
    return _cases[(rows, C)]


def _buf(n, dev, offset=0, dtype=torch.float32):
    """A sentinel-filled buffer and its [offset : offset + n] window (offset 1: a base pointer 4 bytes off a 16-byte boundary)."""
    buf = torch.full((n + 64 + offset,), SENTINEL, device=dev, dtype=dtype)
    return buf, buf[offset:offset + n]


def _intact(buf, n, offset=0):
    return bool((buf[offset + n:] == SENTINEL).all()) and bool((buf[:offset] == SENTINEL).all())


def _placed(t, names, off, dev):
    """The named operands of a case copied into sentinel buffers, those in `off` 4 bytes off alignment -> (views, [(buffer, n, offset)])."""
    v, bufs = {}, []
    for name in names:
        o = 1 if name in off else 0
        n = t[name].numel()
        buf, w = _buf(n, dev, o)
        v[name] = w.view(t[name].shape)
        v[name].copy_(t[name])
        assert v[name].data_ptr() % 16 == 4 * o
        bufs.append((buf, n, o))
    return v, bufs


# ------------------------------------------------------------------ 1. the statistics
def _stats_bound(rows, blocks, v64, ref_mean, ref_std):
    """The bound of DESIGN.md (section 1, "Guided standard loop") against the float64 two-pass formula, per channel, as absolute errors of the
    fp32 results.  A term passes through at most d = ceil(rows / nb) + 257 + nb fp64 additions (its thread's rows, the block's row lanes, the nb
    partial rows), and its own formation (v - v0, the square) adds 3 roundings: with k = 3*(d + 3) + 4 and u = 2^-53,
    |var - var_ref| <= k*u*M2 where M2 = mean((v - v0)^2), so |std - std_ref| <= k*u*M2 / (2*std_ref) + 2*u*std_ref, and
    |mean - mean_ref| <= (d + 3)*u*mean|v - v0| + 2*u*|mean_ref|; the rounding to fp32 adds half an fp32 ulp to each."""
    nb = blocks - 1
    d = math.ceil(rows / nb) + 257 + nb
    k = 3 * (d + 3) + 4
    dv = v64 - v64[0]
    m2, m1 = (dv ** 2).mean(axis=0), np.abs(dv).mean(axis=0)
    err_std = k * U64 * m2 / (2 * ref_std) + 2 * U64 * ref_std
    err_mean = (d + 3) * U64 * m1 + 2 * U64 * np.abs(ref_mean)
    half = lambda ref: 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)      # noqa: E731
    return err_mean, err_std, half(ref_mean), half(ref_std)


@pytest.mark.parametrize("rows,C", SHAPES)
def test_channel_stats_within_the_derived_bound(dev, rows, C):
    from ltx_2_mlx_amd import kernels as K
    t = _case(rows, C, dev)
    blocks = K.channel_guidance_stats_blocks(rows, C)
    assert blocks == min(256, (rows + 63) // 64) + 1
    worst = 0.0
    for per_row in (False, True):
        ts = t["ts_row"] if per_row else torch.tensor([SIGMA], device=dev)
        a, g = R.guidance(t["x"], t["vc"], t["vu"], ts, CFG)                      # the fp32 values the kernel forms, by the same separate ops
        g64, a64 = g.cpu().numpy().astype(np.float64), a.cpu().numpy().astype(np.float64)
        ref = R.channel_stats64(g64, a64)
        if rows > 1:
            assert abs(ref[2, 0] / np.sqrt(ref[3, 0] ** 2 - R.EPS)) > 50.0         # channel 0: the mean far from zero in units of its deviation
        assert np.all(ref[0, 1:3] == [3.0, 0.0]) and np.all(ref[1, 1:3] == np.sqrt(R.EPS))
        for off in ((), ("x",), ("vc",), ("vu",), ("x", "vc", "vu")):
            v, bufs = _placed(t, ("x", "vc", "vu"), off, dev)
            runs = []
            for _ in range(2):
                pb, pw = _buf(blocks * 4 * C, dev, dtype=torch.float64)
                sb, sw = _buf(4 * C, dev)
                K.channel_guidance_stats(v["x"], v["vc"], v["vu"], ts, CFG, partials=pw, stats=sw.view(4, C))
                assert _intact(pb, blocks * 4 * C) and _intact(sb, 4 * C)
                runs.append(sw.view(4, C).clone())
            assert torch.equal(runs[0], runs[1]), f"two runs differ, off={off}"       # no atomics: the same bits
            assert all(_intact(b, n, o) for b, n, o in bufs)
            got = runs[0].cpu().numpy().astype(np.float64)
            for kk, v64 in ((0, g64), (2, a64)):
                err_mean, err_std, half_mean, half_std = _stats_bound(rows, blocks, v64, ref[kk], ref[kk + 1])
                assert np.all(err_std <= half_std), "the bound closes: at most one fp32 ulp in all"
                assert err_mean[0] <= half_mean[0]
                dm, ds = np.abs(got[kk] - ref[kk]), np.abs(got[kk + 1] - ref[kk + 1])
                assert np.all(dm <= half_mean + err_mean), (off, per_row, kk, float((dm / (2 * half_mean + 1e-300)).max()))
                assert np.all(ds <= half_std + err_std), (off, per_row, kk, float((ds / (2 * half_std)).max()))
                worst = max(worst, float((ds / (2 * half_std)).max()), float((dm[half_mean > 0] / (2 * half_mean[half_mean > 0])).max()))
            if rows == 1:                                                            # n = 1: the mean is the value, std exactly sqrt(1e-8) rounded
                assert np.all(got[1] == np.float32(np.sqrt(R.EPS))) and np.all(got[0] == g64[0]) and np.all(got[2] == a64[0])
            assert np.all(got[1, 1:3] == np.float32(np.sqrt(R.EPS))) and np.all(got[0, 1:3] == [3.0, 0.0])
    measure(f"channel stats {rows}x{C}: worst error in fp32 ulps", worst)


def test_channel_stats_refusals(dev):
    from ltx_2_mlx_amd import kernels as K
    t = _case(5, 6, dev)
    with pytest.raises(ValueError, match="timesteps"):
        K.channel_guidance_stats(t["x"], t["vc"], t["vu"], torch.zeros(3, device=dev), CFG)
    assert K.channel_guidance_stats_blocks(0, 128) == 0


# ------------------------------------------------------------------ 2. the step kernel
@pytest.mark.parametrize("rows,C", SHAPES)
def test_step_bit_for_bit(dev, rows, C):
    from ltx_2_mlx_amd import kernels as K
    t = _case(rows, C, dev)
    n = rows * C
    offs = [(), ("x",), ("vc",), ("vu",), ("out",), ("x", "vc", "vu", "out")]
    for per_row in (False, True):
        ts = t["ts_row"] if per_row else torch.tensor([SIGMA], device=dev)
        stats = K.channel_guidance_stats(t["x"], t["vc"], t["vu"], ts, CFG)
        for with_stats, r in ((True, 0.7), (True, 1.0), (False, 0.7)):
            st = stats if with_stats else None
            want = R.rescaled_guided_euler_step(t["x"], t["vc"], t["vu"], ts, st, CFG, r, SIGMA, SIGMA_NEXT)
            assert bool(torch.isfinite(want).all())
            for off in offs:
                tag = f"per_row={per_row} stats={with_stats} r={r} off={off}"
                v, bufs = _placed(t, ("x", "vc", "vu"), off, dev)
                ob, ow = _buf(n, dev, 1 if "out" in off else 0)
                out = ow.view(rows, C)
                K.rescaled_guided_euler_step(v["x"], v["vc"], v["vu"], ts, CFG, r, SIGMA, SIGMA_NEXT, stats=st, out=out)
                assert torch.equal(out, want), f"{tag}: {int((out != want).sum())} of {n} elements differ"
                assert _intact(ob, n, 1 if "out" in off else 0) and all(_intact(b, m, o) for b, m, o in bufs), tag
                # in place: out over x
                K.rescaled_guided_euler_step(v["x"], v["vc"], v["vu"], ts, CFG, r, SIGMA, SIGMA_NEXT, stats=st, out=v["x"])
                assert torch.equal(v["x"], want) and all(_intact(b, m, o) for b, m, o in bufs), tag + " in place"
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        K.rescaled_guided_euler_step(t["x"], t["vc"], t["vu"], ts, CFG, 0.7, 0.0, 0.0)


# ------------------------------------------------------------------ shared tiny model
class Tiny:
    pass


@pytest.fixture(scope="module")
def tiny(dev):
    """The smallest video model of tests/test_parity.py: 12 tokens (2 x 2 x 3), no conditioning."""
    from oracle import loop
    t = Tiny()
    t.cfg, t.wq, t.m = make_dit(dev, heads=2, layers=2, cap=64, seed=11)
    g = torch.Generator().manual_seed(4321)
    t.pos = loop.video_positions(1, 2, 2, 3, 25.0)
    t.lat = torch.randn(1, 12, 128, generator=g)
    t.mask, t.clean = torch.ones(1, 12, 1), torch.zeros(1, 12, 128)
    t.ctx, t.nctx = 0.1 * torch.randn(1, 24, 64, generator=g), 2.0 * torch.randn(1, 24, 64, generator=g)
    return t


def _state(t, dev):
    from ltx_2_mlx_amd.types import LatentState
    return LatentState(latent=t.lat.clone().to(dev), denoise_mask=t.mask.to(dev), positions=t.pos.to(dev), clean_latent=t.clean.to(dev))


def _sigmas(steps=4):
    from ltx_2_mlx_amd.components import LTX2Scheduler
    return [float(s) for s in LTX2Scheduler().execute(steps=steps)]


# ------------------------------------------------------------------ 3. the engine entries
def test_step_entry_equals_its_parts(dev, tiny):
    """rescaled_guided_step_ == ltx2_dit_forward(ctx), ltx2_dit_forward(neg), the statistics, the step kernel: the same kernels in the same order,
    the same bits.  With and without rescale, two steps in a row."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import Modality
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    ctx, nctx, pos = t.ctx.to(dev), t.nctx.to(dev), t.pos.to(dev)
    m.prepare(ctx, pos)
    neg.prepare(nctx, pos)
    for r in (0.7, 0.0):
        lat, want = t.lat[0].to(dev).contiguous(), t.lat[0].to(dev).contiguous()
        for s, sn in ((0.9, 0.6), (0.6, 0.0)):
            ts = torch.tensor([s], device=dev)
            mod = lambda x, c: Modality(latent=x[None], context=c, context_mask=None, timesteps=ts, positions=pos)      # noqa: E731
            vc, vu = m(mod(want, ctx))[0].clone(), neg(mod(want, nctx))[0].clone()
            assert float((vc - vu).abs().max()) > 1e-3
            stats = K.channel_guidance_stats(want, vc, vu, ts, CFG) if r > 0 else None
            want = K.rescaled_guided_euler_step(want, vc, vu, ts, CFG, r, s, sn, stats=stats)
            m.rescaled_guided_step_(neg, lat, mod(lat, ctx), s, sn, CFG, r)
            assert torch.equal(lat, want), f"r={r} sigma={s}: {int((lat != want).sum())} elements differ"
        assert bool(torch.isfinite(lat).all())
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        m.rescaled_guided_step_(neg, lat, mod(lat, ctx), 0.0, 0.0, CFG, 0.7)
    with pytest.raises(ValueError, match="second LTXModel"):
        m.rescaled_guided_step_(None, lat, mod(lat, ctx), 0.5, 0.25, CFG, 0.7)


@pytest.mark.parametrize("r", [0.7, 0.0])
def test_captured_loop_equals_per_step_loop(dev, tiny, r):
    """The captured graph == one rescaled_guided_step_ per step, bit for bit, over 4 scheduler steps; a second replay on a fresh latent equals a
    fresh per-step run: a replay leaves nothing behind that the next one reads."""
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import standard_cfg_denoise_loop
    t, x0m, sig = tiny, X0Model(tiny.m), _sigmas(4)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    run = lambda **k: standard_cfg_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFG, r, **k).latent      # noqa: E731
    graph, eager = run(use_hip_graph=True), run(use_hip_graph=False)
    assert torch.equal(graph, eager), int((graph != eager).sum())
    seen = []
    assert torch.equal(run(callback=lambda i, n: seen.append((i, n))), eager) and seen == [(i + 1, 4) for i in range(4)]
    assert bool(torch.isfinite(graph).all()) and rel_l2(graph.cpu(), t.lat) > 0.1
    model, neg = t.m, t.m.clone_sharing_weights()
    model.prepare(ctx, t.pos.to(dev))
    neg.prepare(nctx, t.pos.to(dev))
    lat = t.lat[0].to(dev).float().contiguous()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        model.capture_rescaled_guided_graph(neg, lat, sig, CFG, r)
        outs = []
        for _ in range(2):
            lat.copy_(t.lat[0].to(dev))
            model.replay_rescaled_guided_graph()
            outs.append(lat.clone())
    side.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0][None], eager)
    with pytest.raises(RuntimeError, match="no guided graph"):
        model.replay_guided_graph()


# ------------------------------------------------------------------ 4. cross_attn_scale
def _scaled_weights(cfg, seed, scale, start_layer):
    """make_dit's weights with attn2.to_out (weight and bias) of the layers >= start_layer multiplied by `scale`."""
    from oracle import dit
    w = dit.make_dit_weights(cfg, seed)
    for i in range(start_layer, cfg.num_layers):
        for n in ("weight", "bias"):
            w[f"transformer_blocks.{i}.attn2.to_out.0.{n}"] = w[f"transformer_blocks.{i}.attn2.to_out.0.{n}"] * scale
    return w


def _forward(m, lat, ctx, pos, sigma, dev):
    from ltx_2_mlx_amd.model.transformer import Modality
    return m(Modality(latent=lat.to(dev), context=ctx.to(dev), context_mask=None, timesteps=torch.tensor([sigma], device=dev), positions=pos.to(dev)))[0].clone()


def test_cross_attn_scale(dev):
    from oracle import dit, loop
    from ltx_2_mlx_amd.model.transformer import LTXModel, Modality, X0Model
    cfg, wq, m = make_dit(dev, heads=2, layers=2, cap=64, seed=11)
    g = torch.Generator().manual_seed(77)
    lat, ctx, pos = torch.randn(1, 40, 128, generator=g), 0.5 * torch.randn(1, 24, 64, generator=g), loop.video_positions(1, 2, 4, 5, 25.0)
    plain = _forward(m, lat, ctx, pos, SIGMA, dev)
    # exact: x2 on layer 1 alone == a model whose attn2.to_out weight and bias are doubled there (doubling is exact in the 16-bit types)
    doubled = LTXModel(num_attention_heads=2, attention_head_dim=128, num_layers=2, caption_channels=64, device=dev)
    doubled.load_state_dict(_scaled_weights(cfg, 11, 2.0, 1))
    want = _forward(doubled, lat, ctx, pos, SIGMA, dev)
    m.set_cross_attn_scale(2.0, start_layer=1)
    got = _forward(m, lat, ctx, pos, SIGMA, dev)
    assert torch.equal(got, want) and not torch.equal(got, plain), int((got != want).sum())
    # a clone made afterwards, and one that exists already, carry the setting
    neg = m.clone_sharing_weights()
    assert torch.equal(_forward(neg, lat, ctx, pos, SIGMA, dev), want)
    m.set_cross_attn_scale(2.0, start_layer=2)                                             # no layer at or past 2: the plain forward
    assert torch.equal(_forward(m, lat, ctx, pos, SIGMA, dev), plain) and torch.equal(_forward(neg, lat, ctx, pos, SIGMA, dev), plain)
    # layer 0 as well: another result than layer 1 alone
    m.set_cross_attn_scale(2.0, start_layer=0)
    both = LTXModel(num_attention_heads=2, attention_head_dim=128, num_layers=2, caption_channels=64, device=dev)
    both.load_state_dict(_scaled_weights(cfg, 11, 2.0, 0))
    got0 = _forward(m, lat, ctx, pos, SIGMA, dev)
    assert torch.equal(got0, _forward(both, lat, ctx, pos, SIGMA, dev)) and not torch.equal(got0, want)
    # 1.0 is bit-identical to never setting it
    m.set_cross_attn_scale(1.0)
    assert torch.equal(_forward(m, lat, ctx, pos, SIGMA, dev), plain) and torch.equal(_forward(neg, lat, ctx, pos, SIGMA, dev), plain)
    # 1.5 against the fp32 oracle on correspondingly scaled weights, under the plain forward's own gate (tests/test_parity.py::test_dit_x0_tiny)
    m.set_cross_attn_scale(1.5, start_layer=1)
    w15 = _scaled_weights(cfg, 11, 1.0, 0)
    w15 = {k: (v.to(torch.bfloat16).float() if (k.endswith(".weight") and v.dim() == 2) else v) for k, v in w15.items()}
    for n in ("weight", "bias"):
        w15[f"transformer_blocks.1.attn2.to_out.0.{n}"] = w15[f"transformer_blocks.1.attn2.to_out.0.{n}"] * 1.5
    sigma = torch.tensor([SIGMA])
    ref = dit.x0_model(lat, ctx, sigma, pos, w15, cfg)
    x0 = X0Model(m)(Modality(latent=lat.to(dev), context=ctx.to(dev), context_mask=None, timesteps=sigma.to(dev), positions=pos.to(dev))).cpu()
    assert rel_l2(x0, ref) < 0.0025 and pearson(x0, ref) > 0.999
    assert rel_l2(x0, dit.x0_model(lat, ctx, sigma, pos, wq, cfg)) > rel_l2(x0, ref)       # and nearer to it than to the unscaled oracle
    m.set_cross_attn_scale(1.0)


@pytest.mark.parametrize("v23", [False, True], ids=["ltx20_av", "ltx23_av"])
def test_cross_attn_scale_is_refused_on_audio_video_models(dev, v23):
    m = make_av(dev, v23, seed=23)[3]
    with pytest.raises(NotImplementedError, match="VideoOnly LTX-2.0"):
        m.set_cross_attn_scale(2.0)


def test_cross_attn_scale_is_refused_on_a_gated_text_cross_attention(dev):
    from ltx_2_mlx_amd.model.transformer import LTXModel
    m = LTXModel(num_attention_heads=2, attention_head_dim=128, num_layers=2, caption_channels=None, cross_attention_adaln=True, apply_gated_attention=True,
                 device=dev)
    with pytest.raises(NotImplementedError, match="VideoOnly LTX-2.0"):
        m.set_cross_attn_scale(2.0, start_layer=0)


# ------------------------------------------------------------------ 5. the loop against its restatement
LOOP_MULTIPLE = 1.5       # of the yardstick measured in the same run; fixed after the first measurement on the MI355X: Y = 1.175e-3, the new loop
#                           1.175e-3 (rescale 0) and 1.062e-3 / 1.074e-3 (rescale 0.7, fused / eager), ratios 1.00 and 0.90; the keyframe loop's test uses the same 1.5


def test_loop_parity(dev, tiny):
    """4 LTX2Scheduler steps, cfg 3, guidance_rescale 0 and 0.7: fused, eager (fused=False) and the fp32 restatement over oracle.dit.  The
    yardstick Y is the rel-L2 of the existing guided_denoise_loop against its own restatement (keyframe_ref.guided_loop) on the same model,
    prompts, cfg and sigmas, measured in this run.  Both loops run the same two forwards per step, whose 16-bit operands carry nearly all of
    the distance to fp32; the element-wise tails differ in a handful of fp32 operations.  The gate on the new loop is LOOP_MULTIPLE x Y."""
    from oracle import dit
    from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import guided_denoise_loop, standard_cfg_denoise_loop
    t, sig = tiny, _sigmas(4)
    x0m = X0Model(t.m)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    x0 = lambda c: (lambda x, ts, s: dit.x0_model(x, c, ts, t.pos, t.wq, t.cfg))      # noqa: E731
    old = guided_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFGGuider(CFG), EulerDiffusionStep()).latent.cpu()
    old_ref = KR.guided_loop(t.lat, t.mask, t.clean, lambda x, ts, s: x0(t.ctx)(x, ts.reshape(-1)[:1], s), lambda x, ts, s: x0(t.nctx)(x, ts.reshape(-1)[:1], s),
                             sig, CFG)
    y = measure("Y existing guided loop vs its restatement", rel_l2(old, old_ref))
    for r in (0.0, 0.7):
        ref = R.standard_cfg_loop(t.lat, x0(t.ctx), x0(t.nctx), sig, CFG, r)
        fused = standard_cfg_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFG, r).latent.cpu()
        eager = standard_cfg_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFG, r, fused=False).latent.cpu()
        e_f = measure(f"fused loop vs restatement, rescale {r}", rel_l2(fused, ref))
        e_e = measure(f"eager loop vs restatement, rescale {r}", rel_l2(eager, ref))
        fe = measure(f"fused vs eager, rescale {r}", rel_l2(fused, eager))
        print(f"standard cfg loop, rescale {r}: Y = {y:.4e}  fused = {e_f:.4e}  eager = {e_e:.4e}  fused vs eager = {fe:.4e}")
        assert e_f <= LOOP_MULTIPLE * y and e_e <= LOOP_MULTIPLE * y and pearson(fused, ref) > 0.999
    # the rescale acts, and cfg <= 1 is the unguided loop
    a = standard_cfg_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFG, 0.0).latent
    b = standard_cfg_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFG, 0.7).latent
    assert rel_l2(a.cpu(), b.cpu()) > 1e-3
    from ltx_2_mlx_amd.pipelines.common import joint_denoise_loop
    plain = joint_denoise_loop(x0m, False, _state(t, dev), None, sig, ctx, None, EulerDiffusionStep(), None, True)[0].latent
    assert torch.equal(standard_cfg_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, 1.0, 0.7).latent, plain)


# ------------------------------------------------------------------ 6. end to end
def test_generate_video_standard_cfg(dev, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate as gen
    out = str(tmp_path / "o.mp4")
    gen.generate_video("a prompt", height=128, width=192, num_frames=9, num_steps=3, standard_cfg=True, model_variant="dev", cfg_scale=3.0, cross_attn_scale=1.5,
                       num_layers=2, num_heads=2, use_gemma=False, skip_vae=True, save_mp4=False, output_path=out, compute_dtype="bfloat16")
    with np.load(str(tmp_path / "o_latent.npz")) as z:
        latent = z["latent"]
    assert latent.shape == (1, 128, 2, 4, 6) and np.isfinite(latent).all() and latent.std() > 0
    with pytest.raises(NotImplementedError, match="classifier-free guidance is built in OneStagePipeline"):
        gen.generate_video("a prompt", height=128, width=192, num_frames=9, num_steps=3, model_variant="dev", cfg_scale=3.0, num_layers=2, num_heads=2,
                           use_gemma=False, skip_vae=True, save_mp4=False, output_path=out, compute_dtype="bfloat16")
