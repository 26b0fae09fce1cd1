"""The res_2s sampler and the HQ pipeline on the GPU: the two kernels bit for bit, the one-call step and its captured graph against the same
kernels called one by one, the loop against the fp32 restatement (with the EXISTING X0Model calls + torch glue as the yardstick), the
pipeline with and without its stage-2 LoRA, and the CLI.  Tiny models as tests/test_parity.py builds them (2 heads x 128, 2 layers,
caption 128)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import measure, rel_l2

import res2s_ref as R
from test_parity import make_dit, make_vae, pearson

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0
BUILDS = [torch.bfloat16, torch.float16]


# ------------------------------------------------------------------ 1. the kernels
_cases = {}


def _case(rows, C):
    """Inputs and CPU references of one shape, computed once and shared by both builds."""
    if (rows, C) not in _cases:
        g = torch.Generator().manual_seed(rows * 131 + C)
        t = dict(ref={})
        t["x"], t["vc"], t["vu"], t["clean"] = (torch.randn(rows, C, generator=g) for _ in range(4))
        t["ts_row"] = torch.rand(rows, generator=g)
        t["mask"] = torch.ones(rows)
        t["mask"][::3] = 0.0
        t["mask"][1::3] = 0.05
        _cases[(rows, C)] = t
    return _cases[(rows, C)]


H, B1, B2 = 0.3566749439387324, -0.05187, 0.91233           # h of 0.05 -> 0.035 and coefficients of that size (any fp32 values serve)
CC = 0.1635


def _combos(rows):
    if rows > 1000:      # the large shape is there for the grid-stride loop: the richest and the plainest form
        return [(True, True, True, 3.0, 100), (False, False, False, 1.0, 0)]
    return [(pt, mk, vu, cfg, nb) for pt in (False, True) for mk in (False, True) for vu in (False, True) for cfg in (1.0, 3.0, 7.5) for nb in (0, 1, 100)]


def _buf(n, dev, offset=0):
    """A sentinel-filled buffer and its [offset : offset + n] window (offset 1: a base pointer 4 bytes off a 16-byte boundary)."""
    buf = torch.full((n + 64 + offset,), SENTINEL, device=dev)
    return buf, buf[offset:offset + n]


def _intact(buf, n, offset=0):
    return bool((buf[offset + n:] == SENTINEL).all()) and bool((buf[:offset] == SENTINEL).all())


@pytest.mark.parametrize("rows,C", [(37, 128), (5, 6), (33000, 128)])       # 16-byte form; element-wise form (C % 4 != 0); past one pass of the capped grid
@pytest.mark.parametrize("build", BUILDS)
def test_res2s_kernels_bit_for_bit(dev, build, rows, C):
    from ltx_2_mlx_amd import kernels as K
    t = _case(rows, C)
    n = rows * C
    d = {k: v.to(dev) for k, v in t.items() if isinstance(v, torch.Tensor)}
    for pt, mk, vu, cfg, nb in _combos(rows):
        key = (pt, mk, vu, cfg, nb)
        ts = t["ts_row"] if pt else torch.tensor([0.909375])
        if key not in t["ref"]:
            args = (t["vc"], t["vu"] if vu else None, ts, t["mask"] if mk else None, t["clean"] if mk else None, cfg)
            xm, an, e = R.midpoint(t["x"], *args, CC, nb)
            t["ref"][key] = (xm, an, e, R.combine(xm, *args, an, e, H, B1, B2), R.midpoint(t["x"], *args, CC, nb, final=True)[0])
        xm_r, an_r, e_r, out_r, d_r = t["ref"][key]
        kw = dict(mask=d["mask"] if mk else None, clean=d["clean"] if mk else None, dtype=build)
        a = (d["vc"], d["vu"] if vu else None, ts.to(dev), cfg)
        tag = f"ts{ts.numel()} mask{mk} vu{vu} cfg{cfg} bong{nb}"
        bufs = [_buf(n, dev) for _ in range(4)]
        xm, an, e, out = (w.view(rows, C) for _, w in bufs)
        K.res2s_midpoint(d["x"], *a, CC, nb, x_mid=xm, anchor=an, eps1=e, **kw)
        K.res2s_combine(xm, *a, an, e, H, B1, B2, out=out, **kw)
        for got, want, name in ((xm, xm_r, "x_mid"), (an, an_r, "anchor"), (e, e_r, "eps1"), (out, out_r, "out")):
            assert torch.equal(got.cpu(), want), f"{tag} {name}: {int((got.cpu() != want).sum())} of {n} elements differ"
        assert all(_intact(b, n) for b, _ in bufs), tag                      # nothing past rows * C
        # aliasing: x_mid over x, then out over x_mid
        xb, xw = _buf(n, dev)
        xin = xw.view(rows, C)
        xin.copy_(d["x"])
        K.res2s_midpoint(xin, *a, CC, nb, x_mid=xin, anchor=an, eps1=e, **kw)
        assert torch.equal(xin.cpu(), xm_r) and torch.equal(an.cpu(), an_r) and torch.equal(e.cpu(), e_r), tag
        K.res2s_combine(xin, *a, an, e, H, B1, B2, out=xin, **kw)
        assert torch.equal(xin.cpu(), out_r) and _intact(xb, n), tag
        # the final-step form writes d to x_mid and nothing else
        fb, fw = _buf(n, dev)
        K.res2s_midpoint(d["x"], *a, CC, nb, x_mid=fw.view(rows, C), final=True, **kw)
        assert torch.equal(fw.view(rows, C).cpu(), d_r) and _intact(fb, n), tag
    if rows == 37:
        # a base pointer 4 bytes off: the element-wise form at C % 4 == 0, the same bits (one operand at a time, and all of them)
        pt, mk, vu, cfg, nb = True, True, True, 3.0, 100
        xm_r, an_r, e_r, out_r, _ = t["ref"][(pt, mk, vu, cfg, nb)]
        for which in ("x", "vc", "vu", "clean", "x_mid", "anchor", "eps1", "out", "all"):
            off = lambda name: 1 if which in (name, "all") else 0
            ins = {}
            for name in ("x", "vc", "vu", "clean"):
                _, w = _buf(n, dev, off(name))
                ins[name] = w.view(rows, C)
                ins[name].copy_(d[name])
            outs = {name: _buf(n, dev, off(name)) for name in ("x_mid", "anchor", "eps1", "out")}
            o = {name: w.view(rows, C) for name, (_, w) in outs.items()}
            assert which not in ins or ins[which].data_ptr() % 16 == 4
            K.res2s_midpoint(ins["x"], ins["vc"], ins["vu"], d["ts_row"], cfg, CC, nb, mask=d["mask"], clean=ins["clean"], x_mid=o["x_mid"],
                             anchor=o["anchor"], eps1=o["eps1"], dtype=build)
            K.res2s_combine(o["x_mid"], ins["vc"], ins["vu"], d["ts_row"], cfg, o["anchor"], o["eps1"], H, B1, B2, mask=d["mask"], clean=ins["clean"],
                            out=o["out"], dtype=build)
            for name, want in (("x_mid", xm_r), ("anchor", an_r), ("eps1", e_r), ("out", out_r)):
                assert torch.equal(o[name].cpu(), want), (which, name)
                assert _intact(outs[name][0], n, off(name)), (which, name)
        from ltx_2_mlx_amd import _native as nv
        L = nv.lib(build)
        p = nv.ptr
        with pytest.raises(ValueError, match="mask and clean go together"):
            nv.check(L.ltx2_res2s_midpoint(p(d["x"]), p(d["vc"]), None, p(d["ts_row"]), 1, p(d["mask"]), None, 3.0, CC, 0, p(xm), p(an), p(e), rows, C, nv.stream()))
        with pytest.raises(ValueError, match="anchor and eps1 go together"):
            nv.check(L.ltx2_res2s_midpoint(p(d["x"]), p(d["vc"]), None, p(d["ts_row"]), 1, None, None, 3.0, CC, 0, p(xm), p(an), None, rows, C, nv.stream()))
        with pytest.raises(ValueError, match="n_bong"):
            nv.check(L.ltx2_res2s_midpoint(p(d["x"]), p(d["vc"]), None, p(d["ts_row"]), 1, None, None, 3.0, CC, -1, p(xm), p(an), p(e), rows, C, nv.stream()))
        with pytest.raises(ValueError, match="ts_stride"):
            nv.check(L.ltx2_res2s_combine(p(xm), p(d["vc"]), None, p(d["ts_row"]), 2, None, None, 3.0, p(an), p(e), H, B1, B2, p(out), rows, C, nv.stream()))


def _off_case():
    """9 x 8 inputs and the CPU restatement of both passes (guided, blended, 100 bong iterations), computed once."""
    t = _case(9, 8)
    if "off" not in t["ref"]:
        args = (t["vc"], t["vu"], t["ts_row"], t["mask"], t["clean"], 3.0)
        xm, an, e = R.midpoint(t["x"], *args, CC, 100)
        t["ref"]["off"] = dict(x_mid=xm, anchor=an, eps1=e, out=R.combine(xm, *args, an, e, H, B1, B2))
    return t, t["ref"]["off"]


def _placed(names, off, src, dev, rows, C):
    """Sentinel-framed device buffers of the named [rows][C] operands, the one called `off` 4 bytes off a 16-byte boundary, filled from `src`
    where it has the name -> ({name: view}, {name: (whole buffer, offset)})."""
    views, bufs = {}, {}
    for name in names:
        o = 1 if name == off else 0
        buf, w = _buf(rows * C, dev, o)
        views[name], bufs[name] = w.view(rows, C), (buf, o)
        assert views[name].data_ptr() % 16 == 4 * o
        if name in src:
            views[name].copy_(src[name])
    return views, bufs


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("off", ["x", "vc", "vu", "clean", "x_mid", "anchor", "eps1"])
def test_res2s_midpoint_each_operand_off_alignment(dev, build, off):
    """One [rows][C] operand of the midpoint pass 4 bytes off a 16-byte boundary: the element-wise form although C % 4 == 0, the same bits."""
    from ltx_2_mlx_amd import kernels as K
    t, ref = _off_case()
    v, bufs = _placed(("x", "vc", "vu", "clean", "x_mid", "anchor", "eps1"), off, t, dev, 9, 8)
    K.res2s_midpoint(v["x"], v["vc"], v["vu"], t["ts_row"].to(dev), 3.0, CC, 100, mask=t["mask"].to(dev), clean=v["clean"], x_mid=v["x_mid"],
                     anchor=v["anchor"], eps1=v["eps1"], dtype=build)
    for name in ("x_mid", "anchor", "eps1"):
        assert torch.equal(v[name].cpu(), ref[name]), name
        assert _intact(bufs[name][0], 72, bufs[name][1]), name


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("off", ["x_mid", "vc", "vu", "clean", "anchor", "eps1", "out"])
def test_res2s_combine_each_operand_off_alignment(dev, build, off):
    """The same for the combine pass, from the restatement's x_mid, anchor and eps1."""
    from ltx_2_mlx_amd import kernels as K
    t, ref = _off_case()
    src = dict(vc=t["vc"], vu=t["vu"], clean=t["clean"], x_mid=ref["x_mid"], anchor=ref["anchor"], eps1=ref["eps1"])
    v, bufs = _placed(("x_mid", "vc", "vu", "clean", "anchor", "eps1", "out"), off, src, dev, 9, 8)
    K.res2s_combine(v["x_mid"], v["vc"], v["vu"], t["ts_row"].to(dev), 3.0, v["anchor"], v["eps1"], H, B1, B2, mask=t["mask"].to(dev), clean=v["clean"],
                    out=v["out"], dtype=build)
    assert torch.equal(v["out"].cpu(), ref["out"])
    assert _intact(bufs["out"][0], 72, bufs["out"][1])


# ------------------------------------------------------------------ shared tiny model + a conditioned state (N = 72 + one conditioned frame of 24, S = 64)
class Tiny:
    pass


def _fill(t, dev):
    from oracle import loop
    g = torch.Generator().manual_seed(4321)
    t.pos = loop.video_positions(1, 4, 4, 6, 24.0)
    n = 96
    t.lat = torch.randn(1, n, 128, generator=g)
    t.clean = torch.randn(1, n, 128, generator=g)
    t.mask = torch.ones(1, n, 1)
    t.mask[:, :12] = 0.0                 # the conditioned frame: half kept clean, half at strength 0.9
    t.mask[:, 12:24] = 0.1
    t.ctx = 0.1 * torch.randn(1, 64, 128, generator=g)
    t.nctx = 0.1 * torch.randn(1, 64, 128, generator=g)
    return t


@pytest.fixture(scope="module")
def tiny(dev):
    t = Tiny()
    t.cfg, t.wq, t.m = make_dit(dev, heads=2, layers=2, cap=128)
    return _fill(t, dev)


@pytest.fixture(scope="module")
def tiny16(dev):
    """The same model on the float16 build of the library."""
    from oracle import dit
    from ltx_2_mlx_amd.model.transformer import LTXModel
    t = Tiny()
    t.cfg = dit.DiTConfig(num_attention_heads=2, attention_head_dim=128, num_layers=2, caption_channels=128)
    t.m = LTXModel(num_attention_heads=2, attention_head_dim=128, num_layers=2, caption_channels=128, device=dev, compute_dtype=torch.float16)
    t.m.load_state_dict(dit.make_dit_weights(t.cfg, 0))
    return _fill(t, dev)


def _state(t, dev, masked=True):
    from ltx_2_mlx_amd.types import LatentState
    mask = t.mask if masked else torch.ones_like(t.mask)
    return LatentState(latent=t.lat.clone().to(dev), denoise_mask=mask.to(dev), positions=t.pos.to(dev), clean_latent=t.clean.to(dev))


def _plan(sigma, sigma_next):
    """(c, n_bong, h, b1, b2, sub_sigma) of a step as the engine plans it: doubles from fp32 sigmas."""
    from ltx_2_mlx_amd.components import get_res2s_coefficients
    s, sn = float(np.float32(sigma)), float(np.float32(sigma_next))
    h = -math.log(sn / s)
    a21, b1, b2 = get_res2s_coefficients(h, {})
    return h * a21, (100 if (h < 0.5 and s > 0.03) else 0), h, b1, b2, float(np.float32(math.sqrt(s * sn)))


# ------------------------------------------------------------------ 2. the engine step
@pytest.mark.parametrize("which", ["bf16", "f16"])
def test_res2s_step_equals_its_parts(dev, tiny, tiny16, which):
    """res2s_step_ == four ltx2_dit_forward calls and the two kernels: the same kernels in the same order (the video path has no atomics), so
    the same bits.  Per-token timesteps (mask * sigma) and the uniform form; with and without the negative context; a bong step, a plain
    step and the final step."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import Modality
    t = tiny if which == "bf16" else tiny16
    m, build = t.m, (torch.bfloat16 if which == "bf16" else torch.float16)
    neg = m.clone_sharing_weights()
    ctx, nctx, pos = t.ctx.to(dev), t.nctx.to(dev), t.pos.to(dev)
    mask1 = t.mask[0].reshape(-1).to(dev).contiguous()
    clean = t.clean[0].to(dev).contiguous()
    cfg = 3.0
    for per_token in (True, False):
        m.prepare(ctx, pos, per_token=per_token)
        neg.prepare(nctx, pos, per_token=per_token)
        mk, cl = (mask1, clean) if per_token else (None, None)
        for sigma, sigma_next, guided in ((0.9, 0.7, True), (0.7, 0.2, True), (0.7, 0.2, False), (0.05, 0.0005, True)):
            final = sigma_next <= 0.001
            lat = t.lat[0].to(dev).contiguous()

            def mod(x, s, c):
                ts = (t.mask.to(dev) * s) if per_token else torch.tensor([s], device=dev)
                return Modality(latent=x[None], context=c, context_mask=None, timesteps=ts, positions=pos, sigma=torch.tensor([s], device=dev))

            def velocities(x, s):
                return m(mod(x, s, ctx))[0].clone(), (neg(mod(x, s, nctx))[0].clone() if guided else None)

            vc, vu = velocities(lat, sigma)
            ts = mod(lat, sigma, ctx).timesteps.reshape(-1)
            if final:
                want = K.res2s_midpoint(lat, vc, vu, ts, cfg, 0.0, 0, mask=mk, clean=cl, final=True, dtype=build)[0]
                sub = None
            else:
                c, nb, h, b1, b2, sub_sigma = _plan(sigma, sigma_next)
                assert nb == (100 if sigma == 0.9 else 0)
                xm, an, e = K.res2s_midpoint(lat, vc, vu, ts, cfg, c, nb, mask=mk, clean=cl, dtype=build)
                vc2, vu2 = velocities(xm, sub_sigma)
                sub = mod(xm, sub_sigma, ctx)
                want = K.res2s_combine(xm, vc2, vu2, sub.timesteps.reshape(-1), cfg, an, e, h, b1, b2, mask=mk, clean=cl, dtype=build)
            got = lat.clone()
            m.res2s_step_(neg if guided else None, got, mod(lat, sigma, ctx), sub, sigma, sigma_next, cfg, denoise_mask=mk, clean_latent=cl)
            tag = f"per_token={per_token} {sigma}->{sigma_next} guided={guided}"
            assert torch.equal(got, want), f"{tag}: {int((got != want).sum())} elements differ"
            assert bool(torch.isfinite(got).all()) and not torch.equal(got, lat), tag
            if guided and not final:
                assert not torch.equal(vc, vu)                                     # two prompts, two velocities


@pytest.mark.parametrize("masked", [True, False])
def test_res2s_graph_equals_eager(dev, tiny, masked):
    """Graph replay == one res2s_step_ call per step, bit for bit: a scheduler table (its last step lands on 0.0011), a table with bong steps
    and one that ends in the final step; the callback form too."""
    from ltx_2_mlx_amd.components import LTX2Scheduler
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import res2s_denoise_loop
    t = tiny
    x0m = X0Model(t.m)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    for sig in ([float(s) for s in LTX2Scheduler().execute(steps=3)], [0.9, 0.7, 0.2, 0.05, 0.035], [0.5, 0.1, 0.0005]):
        for neg in (nctx, None):
            seen = []
            graph = res2s_denoise_loop(x0m, _state(t, dev, masked), sig, ctx, neg, 3.0, use_hip_graph=True).latent.cpu()
            eager = res2s_denoise_loop(x0m, _state(t, dev, masked), sig, ctx, neg, 3.0, use_hip_graph=False).latent.cpu()
            cb = res2s_denoise_loop(x0m, _state(t, dev, masked), sig, ctx, neg, 3.0, callback=lambda i, n: seen.append((i, n))).latent.cpu()
            assert torch.equal(graph, eager) and torch.equal(cb, eager), (sig, neg is None)
            assert bool(torch.isfinite(graph).all()) and rel_l2(graph, t.lat) > 0.1
            n = len(sig) - 1
            assert seen == [(i + 1, n) for i in range(n - (sig[-1] == 0.0005))]
            if masked and sig[-1] == 0.0005:          # after the final step the tokens of mask 0 sit on their clean values
                assert torch.equal(graph[:, :12], t.clean[:, :12])


def test_res2s_refusals(dev, tiny):
    """Each returns an error and launches nothing: the latent is untouched."""
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd.model.transformer import LTXModel, LTXModelType
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    ctx, nctx, pos = t.ctx.to(dev), t.nctx.to(dev), t.pos.to(dev)
    m.prepare(ctx, pos, per_token=True)
    neg.prepare(nctx, pos, per_token=True)
    lat = t.lat[0].to(dev).contiguous()
    keep = lat.clone()
    ts1 = torch.tensor([0.5], device=dev)
    tsn = (t.mask.to(dev) * 0.5).reshape(-1).contiguous()
    clean = t.clean[0].to(dev).contiguous()
    L = nv.lib()

    def step(a, b, ts=ts1, n_ts=1, sigma=0.5, sigma_next=0.25):
        nv.check(L.ltx2_dit_res2s_step(a, b, nv.ptr(lat), nv.ptr(ts), n_ts, None, nv.ptr(ts), None, None, None, 3.0, sigma, sigma_next, nv.stream()))

    def capture(a, b, sig, mask=None, cl=None):
        arr = (nv.C.c_float * len(sig))(*sig)
        n_el = lambda x: 0 if x is None else x.numel()
        nv.check(L.ltx2_dit_graph_capture_res2s(a, b, nv.ptr(lat), arr, len(sig) - 1, nv.ptr(mask), n_el(mask), nv.ptr(cl), n_el(cl), 3.0,
                                                torch.cuda.current_stream().cuda_stream))

    with pytest.raises(ValueError, match="ctx == neg"):
        step(m._h, m._h)
    av = LTXModel(model_type=LTXModelType.AudioVideo, num_attention_heads=2, attention_head_dim=128, num_layers=2, caption_channels=128,
                  audio_attention_heads=2, device=dev)
    for a, b in ((m._h, av._h), (av._h, m._h), (av._h, None)):
        with pytest.raises(ValueError, match="VideoOnly"):
            step(a, b)
    other = make_dit(dev, heads=2, layers=2, cap=128)[2]
    other.prepare(nctx, pos[:, :, :72].contiguous(), per_token=True)                # another N
    with pytest.raises(ValueError, match="contexts differ"):
        step(m._h, other._h)
    for s, sn in ((0.0, 0.0), (-0.5, 0.25), (0.5, -0.1)):
        with pytest.raises(ValueError, match="sigma"):
            step(m._h, neg._h, sigma=s, sigma_next=sn)
    other.prepare(nctx, pos, per_token=False)                                       # a binding at N = 96 without per-token buffers
    with pytest.raises(ValueError, match="per-token"):
        step(m._h, other._h, ts=tsn, n_ts=96)
    with pytest.raises(ValueError, match="per-token"):
        step(other._h, None, ts=tsn, n_ts=96)
    with torch.cuda.stream(torch.cuda.Stream()):
        with pytest.raises(ValueError, match="per-token"):
            capture(m._h, other._h, [1.0, 0.5, 0.0011], tsn, clean)
        with pytest.raises(ValueError, match="tokens x"):
            capture(m._h, neg._h, [1.0, 0.5, 0.0011], tsn[:90].contiguous(), clean)
        with pytest.raises(ValueError, match="bad argument"):
            capture(m._h, neg._h, [1.0 - 0.01 * i for i in range(65)])                  # 64 steps
        with pytest.raises(ValueError, match="sigma"):
            capture(m._h, neg._h, [1.0, 0.0, 0.0])
        with pytest.raises(ValueError, match="ctx == neg"):
            capture(m._h, m._h, [1.0, 0.5, 0.0011])
    torch.cuda.synchronize()
    assert torch.equal(lat, keep)


# ------------------------------------------------------------------ 3. the loop
def _eager_composition(x0m, st, sig_in, ctx, nctx, cfg):
    """The same loop composed from the EXISTING entry points: X0Model calls and torch fp32 glue (what a Python restatement of the reference
    would run on this engine)."""
    from ltx_2_mlx_amd.components import get_res2s_coefficients
    from ltx_2_mlx_amd.pipelines.common import modality_from_state, post_process_latent
    n, sig = R.loop_sigmas(sig_in)
    cache = {}

    def denoised(state, s):
        c, u = x0m(modality_from_state(state, ctx, s)), x0m(modality_from_state(state, nctx, s))
        return post_process_latent(u + cfg * (c - u), state.denoise_mask, state.clean_latent)

    for i in range(n):
        s, sn = sig[i], sig[i + 1]
        h = -math.log(sn / s)
        d = denoised(st, s)
        a21, b1, b2 = get_res2s_coefficients(h, cache)
        an = st.latent.float()
        e = d.float() - an
        xm = an + h * a21 * e
        if h < 0.5 and s > 0.03:
            for _ in range(100):
                an = xm - h * a21 * e
                e = d.float() - an
        d2 = denoised(st.replace(latent=xm), math.sqrt(s * sn))
        st = st.replace(latent=an + h * (b1 * e + b2 * (d2.float() - an)))
    return st.latent


def test_res2s_loop_against_restatement(dev, tiny):
    """Four LTX2Scheduler steps at cfg 3 on 72 free tokens plus one conditioned frame, against tests/res2s_ref.res2s_loop with
    oracle.dit.x0_model inside.  The yardstick E0 is the same loop composed from the existing X0Model calls and torch fp32 glue; the new
    loop may be at most 1.5 x as far from the restatement: the two differ only in where fp32 roundings fall (and in the fp32 rounding of
    0.0011), the 1.5 allows for 16-bit rounding flips of the DiT's input.  Measured on the MI355X: E0 = 4.594e-04, E1 = 4.596e-04."""
    from oracle import dit
    from ltx_2_mlx_amd.components import LTX2Scheduler
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import res2s_denoise_loop
    t = tiny
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    x0 = lambda c: (lambda x, ts, s: dit.x0_model(x, c, ts, t.pos, t.wq, t.cfg))
    ref = R.res2s_loop(t.lat, t.mask, t.clean, x0(t.ctx), x0(t.nctx), sig, 3.0)
    x0m = X0Model(t.m)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    new = res2s_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, 3.0).latent.cpu()
    old = _eager_composition(x0m, _state(t, dev), sig, ctx, nctx, 3.0).cpu()
    e0 = measure("E0 res_2s composed from existing entry points vs fp32", rel_l2(old, ref))
    e1 = measure("E1 res2s_denoise_loop vs fp32", rel_l2(new, ref))
    print(f"res_2s loop: E0 = {e0:.4e}  E1 = {e1:.4e}  pearson = {pearson(new, ref):.6f}")
    assert rel_l2(new[:, 24:], t.lat[:, 24:]) > 0.1
    assert e1 <= 1.5 * e0 and pearson(new, ref) > 0.999


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


PIPELINE_MEASURED = 4.270e-3    # rel-L2 of the stage-1 latent against the fp32 restatement, measured on the MI355X


def test_pipeline_stage1_against_restatement(dev, tiny, parts):
    """Stage 1 of a 128x192x9 request (64x96: 2x2x3 latent frames), one image at frame 0 with strength 0.9, 4 res_2s steps at cfg 3, the
    same noise on both sides: the half-resolution latent against tests/res2s_ref.stage1 (oracle VAE encoder, oracle DiT, fp32 loop).
    Gate: 5 x the value measured on the MI355X, 4.270e-03 (Pearson 0.999991).  Half of the 12 tokens are the conditioned frame, which stays
    in the output at mask 0.1, so the VAE encoder's 16-bit rounding is most of the figure; the loop alone is at 4.6e-04."""
    from oracle import dit, vae_encoder as oenc
    from ltx_2_mlx_amd.components import LTX2Scheduler
    from ltx_2_mlx_amd.pipelines import ImageCondition, TI2VidHQConfig, TI2VidHQPipeline
    t = tiny
    g = torch.Generator().manual_seed(77)
    img = torch.rand(1, 3, 1, 64, 96, generator=g) * 2 - 1
    noise = torch.randn(1, 12, 128, generator=g)
    conf = TI2VidHQConfig(height=128, width=192, num_frames=9, num_inference_steps=4, cfg_scale=3.0, fps=24.0)
    pipe = TI2VidHQPipeline(t.m, parts.enc, None, parts.up)
    out = pipe.stage1_latent(t.ctx.to(dev), t.nctx.to(dev), conf, [ImageCondition(None, 0, 0.9, image=img.to(dev))], initial_noise=noise.to(dev))
    assert out.shape == (1, 128, 2, 2, 3)
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    x0 = lambda c: (lambda x, ts, s, pos: dit.x0_model(x, c, ts, pos, t.wq, t.cfg))
    ref = R.stage1([oenc.encoder_forward(img, parts.enc_wq)], [0], [0.9], (2, 2, 3), 24.0, noise, x0(t.ctx), x0(t.nctx), sig, 3.0)
    err = measure("ti2vid-hq stage 1 vs fp32 restatement", rel_l2(out.cpu(), ref))
    print(f"ti2vid-hq pipeline, stage 1: rel-L2 = {err:.4e}  pearson = {pearson(out.cpu(), ref):.6f}")
    assert err <= 5 * PIPELINE_MEASURED
    with pytest.raises(NotImplementedError, match="TI2VidHQPipeline"):
        pipe.stage1_latent(t.ctx.to(dev), None, TI2VidHQConfig(height=128, width=192, num_frames=9, audio_enabled=True))


def test_pipeline_two_stage_and_lora(dev, tiny, parts, tmp_path):
    from oracle import dit
    from safetensors.torch import save_file
    from ltx_2_mlx_amd.loader.lora_loader import LoRAConfig, fuse_lora_into_weights
    from ltx_2_mlx_amd.model.transformer import LTXModel
    from ltx_2_mlx_amd.pipelines import TI2VidHQConfig, TI2VidHQPipeline, create_ti2vid_hq_pipeline
    t = tiny
    g = torch.Generator().manual_seed(78)
    kw = dict(initial_noise=torch.randn(1, 12, 128, generator=g).to(dev), stage2_noise=torch.randn(1, 48, 128, generator=g).to(dev))
    conf = TI2VidHQConfig(height=128, width=192, num_frames=9, num_inference_steps=3, cfg_scale=3.0)
    pipe = create_ti2vid_hq_pipeline(t.m, parts.enc, parts.dec, parts.up)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    video = pipe(ctx, nctx, conf, **kw)
    assert video.dtype == torch.uint8 and video.shape == (9, 128, 192, 3)
    base = pipe.denoise_latent(ctx, nctx, conf, **kw)
    assert base.shape == (1, 128, 2, 4, 6) and bool(torch.isfinite(base).all())
    assert torch.equal(base, pipe.denoise_latent(ctx, nctx, conf, **kw))
    with pytest.raises(ValueError, match="requires spatial_upscaler"):
        TI2VidHQPipeline(t.m, parts.enc, parts.dec, None)(ctx, nctx, conf)
    # a random rank-4 LoRA on a packed projection (to_k of attn1), a cross-attention query and a feed-forward layer
    lora = {}
    for name, (o, i) in (("transformer_blocks.0.attn1.to_k", (256, 256)), ("transformer_blocks.1.attn2.to_q", (256, 256)),
                         ("transformer_blocks.1.ff.net.0.proj", (1024, 256))):
        lora[f"diffusion_model.{name}.lora_A.weight"] = 0.3 * torch.randn(4, i, generator=g)
        lora[f"diffusion_model.{name}.lora_B.weight"] = 0.3 * torch.randn(o, 4, generator=g)
    path = str(tmp_path / "distilled_lora.safetensors")
    save_file(lora, path)
    lconf = TI2VidHQConfig(height=128, width=192, num_frames=9, num_inference_steps=3, cfg_scale=3.0, distilled_lora_config=LoRAConfig(path, 0.8))
    before = {k: v.clone() for k, v in t.m.weight_tensors().items()}
    with_lora = pipe.denoise_latent(ctx, nctx, lconf, **kw)
    after = t.m.weight_tensors()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)      # the originals are back, bit for bit
    assert bool(torch.isfinite(with_lora).all()) and not torch.equal(with_lora, base)
    assert torch.equal(pipe.denoise_latent(ctx, nctx, conf, **kw), base)                           # and the model computes what it did
    # a model LOADED with the fused weights, run without a LoRA from the same stage-1 latent, gives the same bits
    sd = {k: (v.to(dev, torch.bfloat16) if (k.endswith(".weight") and v.dim() == 2) else v.to(dev)) for k, v in dit.make_dit_weights(t.cfg, 0).items()}
    fused = LTXModel(num_attention_heads=2, attention_head_dim=128, num_layers=2, caption_channels=128, device=dev)
    fused.load_state_dict(fuse_lora_into_weights(sd, [LoRAConfig(path, 0.8)], verbose=False))
    stage1 = pipe.stage1_latent(ctx, nctx, conf, initial_noise=kw["initial_noise"])

    class Stage1Given(TI2VidHQPipeline):
        def stage1_latent(self, *a, **k):
            return stage1

    want = Stage1Given(fused, parts.enc, parts.dec, parts.up).denoise_latent(ctx, nctx, conf, **kw)
    assert torch.equal(with_lora, want)


# ------------------------------------------------------------------ 5. the CLI
def test_generate_video_ti2vid_hq(dev, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    frames = generate.generate_video("a test prompt", pipeline_type="ti2vid-hq", spatial_upscaler_weights="random", use_gemma=False, model_variant="dev",
                                     cfg_scale=3, num_steps=3, height=128, width=192, num_frames=9, seed=3, num_layers=2, num_heads=2,
                                     vae_base_channels=64, output_path=str(tmp_path / "h.mp4"))
    assert frames.dtype == torch.uint8 and frames.shape == (9, 128, 192, 3)
    saved = np.load(tmp_path / "h.npz")["frames"]
    assert saved.shape == (9, 128, 192, 3) and np.array_equal(saved, frames.cpu().numpy())
    assert os.path.exists(tmp_path / "h.mp4") or len(os.listdir(tmp_path / "h_frames")) == 9
    out = capsys.readouterr().out
    assert out.count("using zeros of the context's shape") == 1 and "TI2Vid HQ Pipeline (res_2s)" in out
