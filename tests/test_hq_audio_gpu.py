"""TI2VidHQ with sound on the GPU: the two-segment midpoint / combine launches against the single launches and the torch fp32 op sequence, the
joint res_2s step of the AudioVideo engine against its parts, the loop with and without a callback, the loop against the fp32
restatement (tests/hq_audio_ref.py over oracle.dit_av), the pipeline, the argument checks and generate_video.  The pipeline and generate_video
run with their defaults: with sound both stages step one C call at a time, whatever use_hip_graph says.  The smallest AudioVideo models
of tests/test_parity.py (4 heads, 2 layers), LTX-2.0 and LTX-2.3 form, at 64x96x9: 12 video tokens, 9 audio tokens, S = 24."""
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

from conftest import measure, rel_l2

import hq_audio_ref as HR
import res2s_ref as R
from test_parity import make_av, make_vae, pearson

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = [torch.bfloat16, torch.float16]
SENTINEL = -777.25
F, H, W, NA, S = 2, 2, 3, 9, 24
N = F * H * W
CFG, ACFG = 3.0, 7.0
HH, B1, B2, CC = 0.3566749439387324, -0.05187, 0.91233, 0.1635          # coefficients of a real step's size (any fp32 values serve)


# ------------------------------------------------------------------ 1. the pair kernels
def _buf(n, dev, offset=0):
    buf = torch.full((n + 64 + offset,), SENTINEL, device=dev)
    return buf, buf[offset:offset + n]


def _intact(buf, n, offset=0):
    return bool((buf[offset + n:] == SENTINEL).all()) and bool((buf[:offset] == SENTINEL).all())


def _segment(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    t = {k: torch.randn(rows, C, generator=g) for k in ("x", "vc", "vu", "clean")}
    t["mask"] = (torch.rand(rows, generator=g) > 0.5).float() * 0.9 + 0.1 * (torch.rand(rows, generator=g) > 0.5).float()
    t["ts_row"] = t["mask"] * 0.909375
    return t


_SEGMENTS = {}


def _seg(rows, C, seed):
    if (rows, C, seed) not in _SEGMENTS:
        _SEGMENTS[(rows, C, seed)] = _segment(rows, C, seed)
    return _SEGMENTS[(rows, C, seed)]


# (per-token timesteps, mask, vu) per segment, the two scales, n_bong
FORMS = [((True, True, True), (False, False, True), 3.0, 7.0, 100), ((False, False, False), (True, True, False), 1.0, 2.5, 0),
         ((True, False, True), (True, True, True), 7.5, 3.0, 1), ((False, True, True), (False, False, False), 3.0, 3.0, 0)]


@pytest.mark.parametrize("shape", [((12, 128), (9, 128), None), ((1, 4), (1, 4), None), ((3, 6), (5, 6), None), ((300, 128), (9, 128), None),
                                   ((12, 128), (9, 128), "vc"), ((12, 128), (9, 128), "out")],
                         ids=["12x128+9x128", "1x4+1x4", "3x6+5x6-scalar", "300x128+9x128-blocks", "audio-vc-off-alignment", "audio-out-off-alignment"])
@pytest.mark.parametrize("build", BUILDS, ids=["bf16", "f16"])
def test_pair_kernels_bit_for_bit(dev, build, shape):
    """ltx2_res2s_midpoint_pair / _combine_pair == the single launches on each segment == the separate fp32 torch ops (tests/res2s_ref.py), bit
    for bit, with sentinels behind every output: per-token and single timesteps, with and without a mask and vu per segment, another
    cfg_scale per segment, the final-step form, and in place (x_mid over x, out over x_mid)."""
    from ltx_2_mlx_amd import kernels as K
    (vr, vc_), (ar, ac_), off = shape
    segs = (_seg(vr, vc_, 11), _seg(ar, ac_, 12))
    dv = [{k: v.to(dev) for k, v in s.items()} for s in segs]
    if off == "vc":                                     # one audio input 4 bytes off a 16-byte boundary: V = 1 for BOTH segments
        _, w = _buf(ar * ac_, dev, 1)
        dv[1]["vc"] = w.view(ar, ac_).copy_(dv[1]["vc"])
        assert dv[1]["vc"].data_ptr() % 16 == 4
    for forms in FORMS:
        scales, nb = forms[2:4], forms[4]
        ref, single, ins = [], [], []
        for k, (s, d, (pt, mk, vu), cfg) in enumerate(zip(segs, dv, forms[:2], scales)):
            ts = s["ts_row"] if pt else torch.tensor([0.909375])
            args = (s["vc"], s["vu"] if vu else None, ts, s["mask"] if mk else None, s["clean"] if mk else None, cfg)
            xm, an, e = R.midpoint(s["x"], *args, CC, nb)
            ref.append(dict(x_mid=xm, anchor=an, eps1=e, out=R.combine(xm, *args, an, e, HH, B1, B2), d=R.midpoint(s["x"], *args, CC, nb, final=True)[0]))
            kw = dict(mask=d["mask"] if mk else None, clean=d["clean"] if mk else None)
            a = (d["vc"], d["vu"] if vu else None, ts.to(dev), cfg)
            sxm, san, se = K.res2s_midpoint(d["x"], *a, CC, nb, dtype=build, **kw)
            single.append(dict(x_mid=sxm, anchor=san, eps1=se, out=K.res2s_combine(sxm, *a, san, se, HH, B1, B2, dtype=build, **kw)))
            ins.append(dict(vel_cond=d["vc"], vel_uncond=d["vu"] if vu else None, timesteps=ts.to(dev), cfg_scale=cfg, **kw))
        sizes = (vr * vc_, ar * ac_)
        shapes = ((vr, vc_), (ar, ac_))
        o = lambda k, name: 1 if (k == 1 and off == "out" and name == "out") else 0          # noqa: E731
        bufs = [{name: _buf(sizes[k], dev, o(k, name)) for name in ("x_mid", "anchor", "eps1", "out")} for k in range(2)]
        view = lambda k, name: bufs[k][name][1].view(*shapes[k])          # noqa: E731
        tag = f"{forms}"
        K.res2s_midpoint_pair(*[dict(ins[k], x=dv[k]["x"], x_mid=view(k, "x_mid"), anchor=view(k, "anchor"), eps1=view(k, "eps1")) for k in range(2)],
                              CC, nb, dtype=build)
        K.res2s_combine_pair(*[dict(ins[k], x_mid=view(k, "x_mid"), anchor=view(k, "anchor"), eps1=view(k, "eps1"), out=view(k, "out")) for k in range(2)],
                             HH, B1, B2, dtype=build)
        for k in range(2):
            for name in ("x_mid", "anchor", "eps1", "out"):
                got = view(k, name)
                assert torch.equal(got, single[k][name]), f"{tag} segment {k} {name}: differs from the single launch"
                assert torch.equal(got.cpu(), ref[k][name]), f"{tag} segment {k} {name}: {int((got.cpu() != ref[k][name]).sum())} elements differ"
                assert _intact(bufs[k][name][0], sizes[k], o(k, name)), f"{tag} segment {k} {name}: wrote past rows * C"
        # in place: x_mid over x, then out over x_mid
        xb = [_buf(sizes[k], dev) for k in range(2)]
        xin = [xb[k][1].view(*shapes[k]).copy_(dv[k]["x"]) for k in range(2)]
        K.res2s_midpoint_pair(*[dict(ins[k], x=xin[k], x_mid=xin[k], anchor=view(k, "anchor"), eps1=view(k, "eps1")) for k in range(2)], CC, nb, dtype=build)
        assert all(torch.equal(xin[k].cpu(), ref[k]["x_mid"]) and torch.equal(view(k, "anchor").cpu(), ref[k]["anchor"]) for k in range(2)), tag
        K.res2s_combine_pair(*[dict(ins[k], x_mid=xin[k], anchor=view(k, "anchor"), eps1=view(k, "eps1"), out=xin[k]) for k in range(2)], HH, B1, B2,
                             dtype=build)
        assert all(torch.equal(xin[k].cpu(), ref[k]["out"]) and _intact(xb[k][0], sizes[k]) for k in range(2)), tag
        # the final-step form writes d to x_mid and nothing else
        fb = [_buf(sizes[k], dev) for k in range(2)]
        K.res2s_midpoint_pair(*[dict(ins[k], x=dv[k]["x"], x_mid=fb[k][1].view(*shapes[k])) for k in range(2)], CC, nb, final=True, dtype=build)
        assert all(torch.equal(fb[k][1].view(*shapes[k]).cpu(), ref[k]["d"]) and _intact(fb[k][0], sizes[k]) for k in range(2)), tag


def test_pair_kernel_refusals(dev):
    from ltx_2_mlx_amd import _native as nv
    d = [{k: v.to(dev) for k, v in _seg(r, 8, 13).items()} for r in (5, 3)]
    o = [torch.empty(3, r, 8, device=dev) for r in (5, 3)]
    L, p = nv.lib(), nv.ptr

    def seg(k, mask=None, clean=None, anchor=True, eps1=True, stride=1, rows=None):
        return [p(d[k]["x"]), p(d[k]["vc"]), None, p(d[k]["ts_row"]), stride, mask, clean, 3.0, p(o[k][0]), p(o[k][1]) if anchor else None,
                p(o[k][2]) if eps1 else None, d[k]["x"].shape[0] if rows is None else rows, 8]

    for bad, what in (((seg(0, mask=p(d[0]["mask"])), seg(1)), "mask and clean go together"), ((seg(0), seg(1, mask=p(d[1]["mask"]))), "mask and clean go together"),
                      ((seg(0, eps1=False), seg(1)), "anchor and eps1 go together"), ((seg(0, anchor=False, eps1=False), seg(1)), "both segments together"),
                      ((seg(0), seg(1, stride=2)), "ts_stride"), ((seg(0), seg(1, rows=0)), "empty shape")):
        with pytest.raises(ValueError, match=what):
            nv.check(L.ltx2_res2s_midpoint_pair(*bad[0], *bad[1], CC, 0, nv.stream()))
    with pytest.raises(ValueError, match="n_bong"):
        nv.check(L.ltx2_res2s_midpoint_pair(*seg(0), *seg(1), CC, -1, nv.stream()))


# ------------------------------------------------------------------ the tiny AudioVideo models
class Tiny:
    pass


@pytest.fixture(scope="module", params=[False, True], ids=["v20", "v23"])
def tiny(dev, request):
    from oracle import dit_av, loop
    from ltx_2_mlx_amd.components import LTX2Scheduler
    t = Tiny()
    t.v23 = request.param
    t.cfg, _, t.wq, t.m = make_av(dev, t.v23, seed=41 + t.v23)
    g = torch.Generator().manual_seed(978)
    cv, ca = t.cfg.caption_channels or t.cfg.inner_dim, t.cfg.caption_channels or t.cfg.audio_inner_dim
    t.vctx, t.nvctx = (0.1 * torch.randn(1, S, cv, generator=g) for _ in range(2))
    t.actx, t.nactx = (0.1 * torch.randn(1, S, ca, generator=g) for _ in range(2))
    t.lat = torch.randn(1, N, 128, generator=g)
    t.audio = torch.randn(1, NA, 128, generator=g)
    t.vpos, t.apos = loop.video_positions(1, F, H, W, 25.0), dit_av.audio_positions(1, NA)
    t.mask = torch.ones(1, N, 1)                 # frame 0 conditioned: half at strength 1, half at 0.9
    t.mask[:, :3] = 0.0
    t.mask[:, 3:6] = 0.1
    t.clean = torch.zeros(1, N, 128)
    t.clean[:, :6] = torch.randn(1, 6, 128, generator=g)
    t.sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    t.sig_final = [0.9, 0.5, 0.1, 0.02, 0.0005]      # four steps, the last the final-step branch
    return t


def _states(t, dev, cond):
    from ltx_2_mlx_amd.types import LatentState
    mask = t.mask if cond else torch.ones(1, N, 1)
    lat = torch.where(mask == 0, t.clean, t.lat) if cond else t.lat
    video = LatentState(latent=lat.clone().to(dev), denoise_mask=mask.to(dev), positions=t.vpos.to(dev), clean_latent=(t.clean if cond else lat).clone().to(dev))
    a = t.audio.to(dev)
    return video, LatentState(latent=a.clone(), denoise_mask=torch.ones(1, NA, 1, device=dev), positions=t.apos.to(dev), clean_latent=a.clone())


def _ctx(t, dev):
    if not hasattr(t, "dev_ctx"):
        t.dev_ctx = tuple(c.to(dev) for c in (t.vctx, t.actx, t.nvctx, t.nactx))
    return t.dev_ctx


def _plan(sigma, sigma_next):
    """(c, n_bong, h, b1, b2, sub_sigma) of a step as the engine plans it: doubles from fp32 sigmas."""
    from ltx_2_mlx_amd.components import get_res2s_coefficients
    s, sn = float(np.float32(sigma)), float(np.float32(sigma_next))
    h = -math.log(sn / s)
    a21, b1, b2 = get_res2s_coefficients(h, {})
    return h * a21, (100 if (h < 0.5 and s > 0.03) else 0), h, b1, b2, float(np.float32(math.sqrt(s * sn)))


# ------------------------------------------------------------------ 2. the engine step
@pytest.mark.parametrize("cond", [False, True], ids=["uniform", "frame0"])
def test_res2s_step_av_equals_its_parts(dev, tiny, cond):
    """res2s_step_av_ == four ltx2_dit_forward_av calls and the two pair kernels called one by one: the same kernels in the same order on the
    same streams, so the same bits on BOTH latents.  A bong step, a plain step, a step without the negative context and the final step."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.pipelines.common import audio_modality_from_state, modality_from_state
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    vs, as_ = _states(t, dev, cond)
    mk, cl = (vs.denoise_mask[0].reshape(-1).contiguous(), vs.clean_latent[0].contiguous()) if cond else (None, None)
    for sigma, sigma_next, guided in ((0.9, 0.7, True), (0.7, 0.2, True), (0.7, 0.2, False), (0.05, 0.0005, True)):
        final = sigma_next <= 0.001
        lat, alat = vs.latent[0].float().contiguous(), as_.latent[0].float().contiguous()

        def mods(x, xa, s, vc, ac):
            return (modality_from_state(vs.replace(latent=x[None]), vc, s, uniform=not cond), audio_modality_from_state(as_.replace(latent=xa[None]), ac, s, uniform=True))

        def velocities(x, xa, s):
            pv, pa = m(*mods(x, xa, s, vctx, actx))
            pv, pa = pv[0].clone(), pa[0].clone()
            if not guided:
                return pv, pa, None, None
            uv, ua = neg(*mods(x, xa, s, nvctx, nactx))
            return pv, pa, uv[0].clone(), ua[0].clone()

        def segs(x, xa, s, vel):
            vm, am = mods(x, xa, s, vctx, actx)
            return (dict(vel_cond=vel[0], vel_uncond=vel[2], timesteps=vm.timesteps.reshape(-1), cfg_scale=CFG, mask=mk, clean=cl),
                    dict(vel_cond=vel[1], vel_uncond=vel[3], timesteps=am.timesteps.reshape(-1), cfg_scale=ACFG))

        vel = velocities(lat, alat, sigma)
        sv, sa = segs(lat, alat, sigma, vel)
        if final:
            (want_v, _, _), (want_a, _, _) = K.res2s_midpoint_pair(dict(sv, x=lat), dict(sa, x=alat), 0.0, 0, final=True)
            sub = asub = None
        else:
            c, nb, h, b1, b2, sub_sigma = _plan(sigma, sigma_next)
            assert nb == (100 if sigma == 0.9 else 0)
            (xm, an, e), (xma, ana, ea) = K.res2s_midpoint_pair(dict(sv, x=lat), dict(sa, x=alat), c, nb)
            vel2 = velocities(xm, xma, sub_sigma)
            sv2, sa2 = segs(xm, xma, sub_sigma, vel2)
            sub, asub = mods(xm, xma, sub_sigma, vctx, actx)
            want_v, want_a = K.res2s_combine_pair(dict(sv2, x_mid=xm, anchor=an, eps1=e), dict(sa2, x_mid=xma, anchor=ana, eps1=ea), h, b1, b2)
        got_v, got_a = lat.clone(), alat.clone()
        m.res2s_step_av_(neg if guided else None, got_v, got_a, *mods(lat, alat, sigma, vctx, actx), sub, asub, sigma, sigma_next, CFG, ACFG,
                         denoise_mask=mk, clean_latent=cl)
        torch.cuda.synchronize()
        tag = f"{sigma}->{sigma_next} guided={guided}"
        assert torch.equal(got_v, want_v), f"{tag}: {int((got_v != want_v).sum())} video elements differ"
        assert torch.equal(got_a, want_a), f"{tag}: {int((got_a != want_a).sum())} audio elements differ"
        assert bool(torch.isfinite(got_v).all()) and bool(torch.isfinite(got_a).all()) and not torch.equal(got_v, lat) and not torch.equal(got_a, alat), tag
        if guided:
            assert not torch.equal(vel[0], vel[2]) and not torch.equal(vel[1], vel[3])               # two prompts, two velocities, per modality
        if cond and final:
            assert torch.equal(got_v[:3].cpu(), t.clean[0, :3])                                      # latent = d: mask 0 sits on the clean values


# ------------------------------------------------------------------ 3. the loop: plain and with a callback
@pytest.mark.parametrize("cond", [False, True], ids=["uniform", "frame0"])
@pytest.mark.parametrize("table", ["scheduler", "final"])
def test_loop_with_and_without_callback(dev, tiny, cond, table):
    """The loop is one C call per step (it has no captured form): a callback run equals the plain run bit for bit, the callback sequence is the
    reference's (none on a final step), each scale guides its own modality, and with guidance off neither scale matters."""
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import res2s_av_denoise_loop
    t = tiny
    x0m = X0Model(t.m)
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    sig = t.sig if table == "scheduler" else t.sig_final

    def run(cfg=CFG, acfg=ACFG, callback=None, neg=True, graph=True):
        v, a = res2s_av_denoise_loop(x0m, *_states(t, dev, cond), sig, vctx, actx, nvctx if neg else None, nactx if neg else None, cfg, acfg, callback, graph)
        torch.cuda.synchronize()
        return v.latent.cpu(), a.latent.cpu()

    seen = []
    plain, again = run(), run(graph=False)
    cb = run(callback=lambda i, n: seen.append((i, n)))
    for k, name in enumerate(("video", "audio")):
        assert torch.equal(plain[k], again[k]) and torch.equal(cb[k], plain[k]), name
        assert bool(torch.isfinite(plain[k]).all())
    assert seen == ([(1, 4), (2, 4), (3, 4), (4, 4)] if table == "scheduler" else [(1, 4), (2, 4), (3, 4)])
    assert rel_l2(plain[0], t.lat) > 0.1 and rel_l2(plain[1], t.audio) > 0.1
    if table == "scheduler":
        other = run(acfg=2.0)                                            # only audio_cfg_scale changes: the audio output changes
        assert not torch.equal(other[1], plain[1])
        off = run(neg=False)                                             # guidance off: neither scale matters
        assert all(torch.equal(a, b) for a, b in zip(off, run(cfg=5.0, acfg=1.5, neg=False)))
        assert not torch.equal(off[0], plain[0]) and not torch.equal(off[1], plain[1])
        tiny.loop_out = getattr(tiny, "loop_out", {})
        tiny.loop_out[cond] = plain


# ------------------------------------------------------------------ 4. against the fp32 restatement
# rel-L2 of res2s_av_denoise_loop against tests/hq_audio_ref.res2s_av_loop over oracle.dit_av, measured on the MI355X: (video, audio) per case
# (the existing video-only res_2s loop on the same models' video twins, printed beside them in the same run: 1.008e-03 v20, 1.229e-03 v23)
LOOP_MEASURED = {("v20", False): (1.034e-3, 1.253e-3), ("v20", True): (7.397e-4, 1.232e-3), ("v23", False): (1.214e-3, 1.697e-3), ("v23", True): (9.038e-4, 1.816e-3)}


@pytest.mark.parametrize("cond", [False, True], ids=["uniform", "frame0"])
def test_loop_against_restatement(dev, tiny, cond):
    """Four LTX2Scheduler steps, cfg 3 on the video and 7 on the audio, against the fp32 restatement of the reference's joint loop with
    oracle.dit_av inside (pinned to the reference by tests/golden/res2s_av_loop.npz).  Gate: 5 x the value measured on the MI355X, per
    modality."""
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import res2s_av_denoise_loop
    t = tiny
    mask = t.mask if cond else torch.ones(1, N, 1)
    lat = torch.where(mask == 0, t.clean, t.lat) if cond else t.lat
    clean = t.clean if cond else lat
    pos = HR.av_x0(t.wq, t.cfg, t.vpos, t.apos, t.vctx, t.actx)
    neg = HR.av_x0(t.wq, t.cfg, t.vpos, t.apos, t.nvctx, t.nactx)
    rv, ra = HR.res2s_av_loop((lat, mask, clean), (t.audio, torch.ones(1, NA, 1), t.audio), pos, neg, t.sig, CFG, ACFG)
    got = getattr(tiny, "loop_out", {}).get(cond)
    if got is None:
        v, a = res2s_av_denoise_loop(X0Model(t.m), *_states(t, dev, cond), t.sig, *_ctx(t, dev), CFG, ACFG)
        got = (v.latent.cpu(), a.latent.cpu())
    tag = f"{'v23' if t.v23 else 'v20'} {'frame0' if cond else 'uniform'}"
    ev = measure(f"hq-audio joint res_2s loop, video vs fp32 ({tag})", rel_l2(got[0], rv))
    ea = measure(f"hq-audio joint res_2s loop, audio vs fp32 ({tag})", rel_l2(got[1], ra))
    print(f"hq-audio joint loop {tag}: video rel-L2 = {ev:.4e} (pearson {pearson(got[0], rv):.6f})  audio rel-L2 = {ea:.4e} (pearson {pearson(got[1], ra):.6f})")
    mv, ma = LOOP_MEASURED[("v23" if t.v23 else "v20", cond)]
    assert mv is not None and ma is not None, "LOOP_MEASURED holds no figure for this case"
    assert ev <= 5 * mv and ea <= 5 * ma


def test_video_only_loop_figure_for_scale(dev, tiny):
    """The existing video-only res_2s loop on the same model's video twin against its restatement, printed beside the joint figures."""
    from oracle import dit_av
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import res2s_denoise_loop
    t = tiny
    vctx, _, nvctx, _ = _ctx(t, dev)
    x0 = lambda c: (lambda x, ts, s: dit_av.video_only_x0_model(dict(latent=x, context=c, timesteps=ts, sigma=torch.tensor([s]), positions=t.vpos), t.wq, t.cfg))  # noqa: E731
    ref = R.res2s_loop(t.lat, torch.ones(1, N, 1), t.lat, x0(t.vctx), x0(t.nvctx), t.sig, CFG)
    new = res2s_denoise_loop(X0Model(t.m), _states(t, dev, False)[0], t.sig, vctx, nvctx, CFG).latent.cpu()
    e = measure(f"video-only res_2s loop on the video twin vs fp32 ({'v23' if t.v23 else 'v20'})", rel_l2(new, ref))
    print(f"video-only res_2s loop for scale: rel-L2 = {e:.4e}")
    assert bool(torch.isfinite(new).all()) and pearson(new, ref) > 0.999


# ------------------------------------------------------------------ 5. the pipeline
@pytest.fixture(scope="module")
def parts(dev):
    from ltx_2_mlx_amd.model.audio_vae import AudioDecoder, Vocoder
    from ltx_2_mlx_amd.model.upscaler import SpatialUpscaler
    p = Tiny()
    _, _, p.dec = make_vae(dev, layers=1)
    p.up = SpatialUpscaler(in_channels=128, mid_channels=64, num_blocks_per_stage=1, device=dev)
    p.up.init_random_weights(seed=3)
    p.adec = AudioDecoder(device=dev)
    p.adec.init_random_weights(1)
    p.voc = Vocoder(upsample_initial_channel=128, device=dev)
    p.voc.init_random_weights(2)
    return p


PIPELINE_MEASURED = {"v20": (1.187e-3, 1.471e-3), "v23": (1.410e-3, 2.005e-3)}     # rel-L2 of the stage-1 (video, audio) latents against the fp32 restatement, measured on the MI355X


def test_pipeline_with_sound(dev, tiny, parts, tmp_path, monkeypatch):
    """TI2VidHQPipeline at 128x192x9 (stage 1 at 64x96), 3 joint res_2s steps and the 3 joint refinement steps, audio_enabled, fixed noises."""
    from safetensors.torch import save_file
    import ltx_2_mlx_amd.pipelines.ti2vid_hq as T
    from ltx_2_mlx_amd.components import LTX2Scheduler
    from ltx_2_mlx_amd.loader.lora_loader import LoRAConfig
    from ltx_2_mlx_amd.pipelines import TI2VidHQConfig, TI2VidHQPipeline
    t = tiny
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    g = torch.Generator().manual_seed(80)
    n1, n2 = torch.randn(1, N, 128, generator=g), torch.randn(1, 4 * N, 128, generator=g)
    a1, a2 = torch.randn(1, NA, 128, generator=g), torch.randn(1, NA, 128, generator=g)
    kw = dict(initial_noise=n1.to(dev), stage2_noise=n2.to(dev), initial_audio_noise=a1.to(dev), stage2_audio_noise=a2.to(dev))
    conf = TI2VidHQConfig(height=128, width=192, num_frames=9, num_inference_steps=3, cfg_scale=CFG, audio_cfg_scale=ACFG, audio_enabled=True)
    pipe = TI2VidHQPipeline(t.m, None, parts.dec, parts.up, parts.adec, parts.voc)
    frames, wav = pipe(vctx, nvctx, conf, None, None, actx, nactx, **kw)
    assert frames.dtype == torch.uint8 and frames.shape == (9, 128, 192, 3)
    assert wav.shape == (1, 2, (4 * NA - 3) * 240) and bool(torch.isfinite(wav).all())
    latent, alatent = pipe.denoise_latent(vctx, nvctx, conf, None, None, actx, nactx, **kw)
    assert latent.shape == (1, 128, 2, 4, 6) and alatent.shape == (1, 8, NA, 16) and bool(torch.isfinite(latent).all()) and bool(torch.isfinite(alatent).all())
    assert torch.equal(alatent, pipe.audio_latent) and torch.equal(wav, parts.voc(parts.adec(alatent)))
    assert TI2VidHQPipeline(t.m, None, parts.dec, parts.up)(vctx, nvctx, conf, None, None, actx, nactx, **kw)[1] is None        # no decoders: no waveform
    # stage 1 against the restatement, per modality
    s1v, s1a = pipe.stage1_latent(vctx, nvctx, conf, positive_audio_encoding=actx, negative_audio_encoding=nactx, initial_noise=kw["initial_noise"],
                                  initial_audio_noise=kw["initial_audio_noise"])
    assert s1v.shape == (1, 128, 2, 2, 3) and s1a.shape == (1, 8, NA, 16)
    sig = [float(s) for s in LTX2Scheduler().execute(steps=3)]
    pos = HR.av_x0(t.wq, t.cfg, t.vpos, t.apos, t.vctx, t.actx)
    neg = HR.av_x0(t.wq, t.cfg, t.vpos, t.apos, t.nvctx, t.nactx)
    rv, ra = HR.res2s_av_loop((n1, torch.ones(1, N, 1), n1), (a1, torch.ones(1, NA, 1), a1), pos, neg, sig, CFG, ACFG)
    from oracle import loop
    gv = loop.patchify(s1v.cpu().float())
    ga = s1a.cpu().float().permute(0, 2, 1, 3).reshape(1, NA, 128)                     # AudioPatchifier: (B, C, T, F) -> (B, T, C * F)
    tag = "v23" if t.v23 else "v20"
    ev = measure(f"hq-audio pipeline stage 1, video vs fp32 ({tag})", rel_l2(gv, rv))
    ea = measure(f"hq-audio pipeline stage 1, audio vs fp32 ({tag})", rel_l2(ga, ra))
    print(f"hq-audio pipeline stage 1 {tag}: video rel-L2 = {ev:.4e}  audio rel-L2 = {ea:.4e}")
    mv, ma = PIPELINE_MEASURED[tag]
    assert mv is not None and ma is not None, "PIPELINE_MEASURED holds no figure for this case"
    assert ev <= 5 * mv and ea <= 5 * ma
    # the stage-2 audio starts from the stage-1 audio: sigma_0 * noise + (1 - sigma_0) * stage 1, handed to the joint loop
    seen = {}
    real = T.joint_denoise_loop

    def spy(transformer, is_av, vstate, astate, *a, **k):
        seen["audio"] = None if astate is None else astate.latent.clone()
        seen["use_hip_graph"] = a[5]
        return real(transformer, is_av, vstate, astate, *a, **k)

    with monkeypatch.context() as mp:
        mp.setattr(T, "joint_denoise_loop", spy)
        again = pipe.denoise_latent(vctx, nvctx, conf, None, None, actx, nactx, **kw)
    assert torch.equal(again[0], latent) and torch.equal(again[1], alatent)
    s0 = float(T.STAGE_2_DISTILLED_SIGMA_VALUES[0])
    want = a2.to(dev) * s0 + s1a.permute(0, 2, 1, 3).reshape(1, NA, 128) * (1 - s0)
    assert rel_l2(seen["audio"].cpu(), want.cpu()) < 1e-6
    assert conf.use_hip_graph is True and seen["use_hip_graph"] is False          # with sound, stage 2 steps one C call at a time whatever the config says
    # a distilled LoRA is fused for stage 2 only and taken out again, bit for bit
    lora = {}
    for name, (o, i) in (("transformer_blocks.0.attn1.to_k", (512, 512)), ("transformer_blocks.1.ff.net.0.proj", (2048, 512))):
        lora[f"diffusion_model.{name}.lora_A.weight"] = 0.3 * torch.randn(4, i, generator=g)
        lora[f"diffusion_model.{name}.lora_B.weight"] = 0.3 * torch.randn(o, 4, generator=g)
    path = str(tmp_path / "distilled_lora.safetensors")
    save_file(lora, path)
    lconf = TI2VidHQConfig(height=128, width=192, num_frames=9, num_inference_steps=3, cfg_scale=CFG, audio_cfg_scale=ACFG, audio_enabled=True,
                           distilled_lora_config=LoRAConfig(path, 0.8))
    before = {k: v.clone() for k, v in t.m.weight_tensors().items()}
    with_lora = pipe.denoise_latent(vctx, nvctx, lconf, None, None, actx, nactx, **kw)
    after = t.m.weight_tensors()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not torch.equal(with_lora[0], latent) and bool(torch.isfinite(with_lora[0]).all()) and bool(torch.isfinite(with_lora[1]).all())
    # audio_enabled=False on the same AudioVideo model: the parent's path (the video twin through both loops), bit for bit
    from ltx_2_mlx_amd.components import STAGE_2_DISTILLED_SIGMA_VALUES, EulerDiffusionStep, VideoLatentPatchifier
    from ltx_2_mlx_amd.pipelines.common import (conditioned_initial_state, final_latent, joint_denoise_loop, res2s_denoise_loop, seeded_noiser, upscale_latent_x2,
                                                video_tools_for)
    silent = TI2VidHQConfig(height=128, width=192, num_frames=9, num_inference_steps=3, cfg_scale=CFG, audio_cfg_scale=ACFG)
    out = pipe.denoise_latent(vctx, nvctx, silent, initial_noise=kw["initial_noise"], stage2_noise=kw["stage2_noise"])
    assert isinstance(out, torch.Tensor) and out.shape == (1, 128, 2, 4, 6)
    noiser = seeded_noiser(dev, silent.seed)
    pat = VideoLatentPatchifier(patch_size=1)
    tools = video_tools_for(pat, 9, 64, 96, silent.fps)
    st = noiser(conditioned_initial_state(tools, [], silent.dtype, dev), noise_scale=1.0, noise=kw["initial_noise"])
    st = res2s_denoise_loop(pipe.transformer, st, LTX2Scheduler().execute(steps=3), vctx, nvctx, CFG, ACFG, None, True)
    tools2 = video_tools_for(pat, 9, 128, 192, silent.fps)
    st2 = conditioned_initial_state(tools2, [], silent.dtype, dev, initial_latent=upscale_latent_x2(final_latent(tools, st), parts.up, None, parts.dec))
    sig2 = [float(s) for s in STAGE_2_DISTILLED_SIGMA_VALUES]
    st2 = noiser(st2, noise_scale=sig2[0], noise=kw["stage2_noise"])
    st2 = joint_denoise_loop(pipe.transformer, True, st2, None, sig2, vctx, None, EulerDiffusionStep(), None, True)[0]
    assert torch.equal(out, final_latent(tools2, st2))
    with pytest.raises(NotImplementedError, match="TI2VidHQPipeline.*AudioVideo"):
        TI2VidHQPipeline(t.m._video_twin(), None, parts.dec, parts.up).denoise_latent(vctx, nvctx, conf)


# ------------------------------------------------------------------ 6. argument checks (host side, nothing is launched)
def test_res2s_step_av_refusals(dev, tiny):
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import res2s_av_denoise_loop
    from oracle import dit_av, loop
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    vs, as_ = _states(t, dev, True)
    m.prepare(vctx, vs.positions, per_token=True, audio_context=actx, audio_positions=as_.positions)
    neg.prepare(nvctx, vs.positions, per_token=True, audio_context=nactx, audio_positions=as_.positions)
    lat, alat = vs.latent[0].float().contiguous(), as_.latent[0].float().contiguous()
    before, abefore = lat.clone(), alat.clone()
    ts1, sg = torch.tensor([0.5], device=dev), torch.tensor([0.5], device=dev)
    tsn, atsn = torch.full((N,), 0.5, device=dev), torch.full((NA,), 0.5, device=dev)
    mk, cl = vs.denoise_mask[0].reshape(-1).contiguous(), vs.clean_latent[0].contiguous()
    L, p = nv.lib(), nv.ptr

    def step(a, b, ts=ts1, n_ts=1, ats=ts1, n_ats=1, sigma=0.5, sigma_next=0.25, vmask=None, vclean=None, amask=None, aclean=None, sub=True):
        nv.check(L.ltx2_dit_res2s_step_av(a, b, p(lat), p(alat), p(ts), n_ts, p(ats), n_ats, p(sg), p(ts) if sub else None, p(ats) if sub else None, p(sg), vmask,
                                          vclean, amask, aclean, CFG, ACFG, sigma, sigma_next, nv.stream()))

    with pytest.raises(ValueError, match="ctx == neg"):
        step(m._h, m._h)
    twin = m._video_twin()
    for a, b in ((m._h, twin._h), (twin._h, m._h), (twin._h, None)):
        with pytest.raises(ValueError, match="must be AudioVideo"):
            step(a, b)
    fresh = make_av(dev, t.v23, seed=3)[3]                                        # never prepared
    for a, b in ((m._h, fresh._h), (fresh._h, None)):
        with pytest.raises(ValueError, match="prepare"):
            step(a, b)
    for f, na in ((3, NA), (F, NA + 1)):                                          # another N, another Na
        fresh.prepare(nvctx, loop.video_positions(1, f, H, W, 25.0).to(dev), per_token=True, audio_context=nactx, audio_positions=dit_av.audio_positions(1, na).to(dev))
        with pytest.raises(ValueError, match="contexts differ"):
            step(m._h, fresh._h)
    for b in (neg._h, None):
        with pytest.raises(ValueError, match="must be 1 or N"):
            step(m._h, b, ts=tsn, n_ts=N - 1)
        with pytest.raises(ValueError, match="must be 1 or Na"):
            step(m._h, b, ats=atsn, n_ats=NA - 1)
        for kw in (dict(sigma=0.0), dict(sigma=-0.5), dict(sigma_next=-0.1)):
            with pytest.raises(ValueError, match="sigma"):
                step(m._h, b, **kw)
        for kw in (dict(vmask=p(mk)), dict(vclean=p(cl)), dict(amask=p(atsn)), dict(aclean=p(alat))):
            with pytest.raises(ValueError, match="mask and clean go together"):
                step(m._h, b, ts=tsn, n_ts=N, **kw)
        with pytest.raises(ValueError, match="ts_sub"):
            step(m._h, b, sub=False)
    fresh.prepare(nvctx, vs.positions, per_token=False, audio_context=nactx, audio_positions=as_.positions)       # N and Na fit, no per-token buffers
    for kw in (dict(ts=tsn, n_ts=N), dict(ats=atsn, n_ats=NA)):
        with pytest.raises(ValueError, match="per-token"):
            step(m._h, fresh._h, **kw)
        with pytest.raises(ValueError, match="per-token"):
            step(fresh._h, None, **kw)
    with pytest.raises(ValueError, match="AudioVideo contexts"):
        m.res2s_step_av_(twin, lat, alat, None, None, None, None, 0.5, 0.25, CFG, ACFG)
    with pytest.raises(ValueError, match="second LTXModel"):
        m.res2s_step_av_(object(), lat, alat, None, None, None, None, 0.5, 0.25, CFG, ACFG)
    torch.cuda.synchronize()
    assert torch.equal(lat, before) and torch.equal(alat, abefore)                # nothing was launched
    with pytest.raises(ValueError, match=r"requires an audio-video \(AV\) model"):
        res2s_av_denoise_loop(X0Model(twin), vs, as_, t.sig, vctx, actx, nvctx, nactx, CFG, ACFG)
    with pytest.raises(ValueError, match="audio_encoding"):
        res2s_av_denoise_loop(X0Model(m), vs, as_, t.sig, vctx, None, nvctx, nactx, CFG, ACFG)
    if vctx.shape[-1] != actx.shape[-1]:
        with pytest.raises(ValueError, match="negative_audio_context"):
            res2s_av_denoise_loop(X0Model(m), vs, as_, t.sig, vctx, actx, nvctx, None, CFG, ACFG)


# ------------------------------------------------------------------ 7. generate_video
def test_generate_video_ti2vid_hq_audio(dev, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    frames = generate.generate_video("a test prompt", ti2vid_hq_audio=True, decode_audio=True, spatial_upscaler_weights="random", use_gemma=False,
                                     model_variant="dev", cfg_scale=3, num_steps=2, num_layers=2, num_heads=2, vae_base_channels=64, height=128,
                                     width=192, num_frames=9, seed=3, output_path=str(tmp_path / "s.mp4"), save_mp4=False)
    assert frames.dtype == torch.uint8 and frames.shape == (9, 128, 192, 3)
    saved = np.load(tmp_path / "s.npz")["frames"]
    assert np.array_equal(saved, frames.cpu().numpy())
    lat = np.load(tmp_path / "s_audio_latent.npz")["latent"]
    assert lat.shape == (1, 8, NA, 16) and np.isfinite(lat).all()
    with wave.open(str(tmp_path / "s.wav"), "rb") as f:
        assert f.getnchannels() == 2 and f.getsampwidth() == 2 and f.getframerate() == 24000 and f.getnframes() == (4 * NA - 3) * 240
    cap = capsys.readouterr()
    assert "TI2Vid HQ Pipeline (res_2s, audio + video)" in cap.out
