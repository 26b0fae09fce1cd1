"""The Heun sampler and the GE velocity correction on the GPU: the kernels bit for bit against the separate fp32 torch ops on the device, each
pair launch against two single launches, the step entries against their parts, the captured loop against the per-step loop, the loops against
the fp32 oracle, and OneStagePipeline end to end.  Tiny models as tests/test_parity.py builds them."""
import os

import pytest
import torch

from conftest import measure, rel_l2

import heun_ref as R
from test_parity import make_av, make_dit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0
SIGMA, SIGMA_NEXT, GAMMA = 0.909375, 0.725, 2.0


# ------------------------------------------------------------------ 1. the kernels
_cases = {}


def _case(rows, C, dev):
    """Device inputs of one shape, made once."""
    if (rows, C) not in _cases:
        g = torch.Generator().manual_seed(rows * 131 + C)
        t = {k: torch.randn(rows, C, generator=g).to(dev) for k in ("x", "vc", "vu", "clean", "prev", "vc2", "vu2")}
        t["ts_row"], t["ts2_row"] = (torch.rand(rows, generator=g) * SIGMA).to(dev), (torch.rand(rows, generator=g) * SIGMA_NEXT).to(dev)
        mask = torch.ones(rows)
        mask[::3] = 0.0
        mask[1::3] = 0.05
        t["mask"] = mask.to(dev)
        _cases[(rows, C)] = t
    return _cases[(rows, C)]


def _buf(n, dev, offset=0):
    """A sentinel-filled buffer and its [offset : offset + n] window (offset 1: a base pointer 4 bytes off a 16-byte boundary)."""
    buf = torch.full((n + 64 + offset,), SENTINEL, device=dev)
    return buf, buf[offset:offset + n]


def _intact(buf, n, offset=0):
    return bool((buf[offset + n:] == SENTINEL).all()) and bool((buf[:offset] == SENTINEL).all())


def _combos(rows):
    if rows > 1000:      # the large shape is there for the grid-stride loop and the ragged tail: the richest and the plainest form
        return [(True, True, True, "next"), (False, False, False, "off")]
    return [(pt, mk, vu, ge) for pt in (False, True) for mk in (False, True) for vu in (False, True) for ge in ("off", "first", "next")]


@pytest.mark.parametrize("rows,C", [(37, 128), (5, 6), (33000, 128)])       # 16-byte form; element-wise form (C % 4 != 0); many blocks, ragged tail
def test_heun_kernels_bit_for_bit(dev, rows, C):
    from ltx_2_mlx_amd import kernels as K
    t = _case(rows, C, dev)
    n = rows * C
    cfg = 3.0
    for pt, mk, vu, ge in _combos(rows):
        tag = f"per_row={pt} mask={mk} vu={vu} ge={ge}"
        ts, ts2 = (t["ts_row"], t["ts2_row"]) if pt else (torch.tensor([SIGMA], device=dev), torch.tensor([SIGMA_NEXT], device=dev))
        mask, clean = (t["mask"], t["clean"]) if mk else (None, None)
        vu1, vu2 = (t["vu"], t["vu2"]) if vu else (None, None)
        gamma, first = (0.0 if ge == "off" else GAMMA), ge != "next"
        d_r, xp_r, prev_r = R.heun_predict(t["x"], t["vc"], vu1, ts, mask, clean, cfg, SIGMA, SIGMA_NEXT, gamma, t["prev"], first)
        out_r = R.heun_correct(t["x"], d_r, xp_r, t["vc2"], vu2, ts2, mask, clean, cfg, SIGMA, SIGMA_NEXT)
        bufs = [_buf(n, dev) for _ in range(4)]
        d, xp, out, prev = (w.view(rows, C) for _, w in bufs)
        prev.copy_(t["prev"])
        pv = None if ge == "off" else prev
        kw = dict(mask=mask, clean=clean)
        K.heun_predict(t["x"], t["vc"], vu1, ts, cfg, SIGMA, SIGMA_NEXT, gamma, pv, first, d=d, xp=xp, **kw)
        K.heun_correct(t["x"], d, xp, t["vc2"], vu2, ts2, cfg, SIGMA, SIGMA_NEXT, out=out, **kw)
        for got, want, name in ((d, d_r, "d"), (xp, xp_r, "xp"), (out, out_r, "out"), (prev, t["prev"] if ge == "off" else prev_r, "prev")):
            assert torch.equal(got, want), f"{tag} {name}: {int((got != want).sum())} of {n} elements differ"
        assert all(_intact(b, n) for b, _ in bufs), tag                      # nothing past rows * C
        # the Euler step with GE is the predictor alone
        if ge != "off":
            prev.copy_(t["prev"])
            gb, gw = _buf(n, dev)
            K.ge_euler_step(t["x"], t["vc"], vu1, ts, cfg, gamma, prev, first, SIGMA, SIGMA_NEXT, out=gw.view(rows, C), **kw)
            assert torch.equal(gw.view(rows, C), xp_r) and torch.equal(prev, prev_r) and _intact(gb, n), tag
        # the final-step form writes d and nothing else; here over x itself
        xb, xw = _buf(n, dev)
        xin = xw.view(rows, C)
        xin.copy_(t["x"])
        prev.copy_(t["prev"])
        K.heun_predict(xin, t["vc"], vu1, ts, cfg, SIGMA, 0.0, gamma, pv, first, d=xin, final=True, **kw)
        assert torch.equal(xin, d_r) and _intact(xb, n), tag
        # aliasing: the corrector's out over x
        xin.copy_(t["x"])
        K.heun_correct(xin, d, xp, t["vc2"], vu2, ts2, cfg, SIGMA, SIGMA_NEXT, out=xin, **kw)
        assert torch.equal(xin, out_r) and _intact(xb, n), tag


@pytest.mark.parametrize("off", ["x", "vc", "vu", "clean", "prev", "d", "xp", "vc2", "vu2", "out", "all"])
def test_each_operand_off_alignment(dev, off):
    """One [rows][C] operand 4 bytes off a 16-byte boundary: the element-wise form although C % 4 == 0, the same bits, nothing written outside."""
    from ltx_2_mlx_amd import kernels as K
    rows, C = 9, 8
    t = _case(rows, C, dev)
    n = rows * C
    d_r, xp_r, prev_r = R.heun_predict(t["x"], t["vc"], t["vu"], t["ts_row"], t["mask"], t["clean"], 3.0, SIGMA, SIGMA_NEXT, GAMMA, t["prev"], False)
    out_r = R.heun_correct(t["x"], d_r, xp_r, t["vc2"], t["vu2"], t["ts2_row"], t["mask"], t["clean"], 3.0, SIGMA, SIGMA_NEXT)
    v, bufs = {}, {}
    for name in ("x", "vc", "vu", "clean", "prev", "d", "xp", "vc2", "vu2", "out"):
        o = 1 if off in (name, "all") else 0
        buf, w = _buf(n, dev, o)
        v[name], bufs[name] = w.view(rows, C), (buf, o)
        assert v[name].data_ptr() % 16 == 4 * o
        if name in t:
            v[name].copy_(t[name])
    kw = dict(mask=t["mask"], clean=v["clean"])
    K.heun_predict(v["x"], v["vc"], v["vu"], t["ts_row"], 3.0, SIGMA, SIGMA_NEXT, GAMMA, v["prev"], False, d=v["d"], xp=v["xp"], **kw)
    K.heun_correct(v["x"], v["d"], v["xp"], v["vc2"], v["vu2"], t["ts2_row"], 3.0, SIGMA, SIGMA_NEXT, out=v["out"], **kw)
    for name, want in (("d", d_r), ("xp", xp_r), ("prev", prev_r), ("out", out_r)):
        assert torch.equal(v[name], want), name
    assert all(_intact(b, n, o) for b, o in bufs.values())


def test_pair_launches_equal_two_single_launches(dev):
    from ltx_2_mlx_amd import kernels as K
    v, a = _case(37, 128, dev), _case(11, 128, dev)
    for masked, final in ((True, False), (False, False), (True, True)):
        seg, single = {}, {}
        for key, t, cfg, pt in (("v", v, 3.0, True), ("a", a, 7.0, masked)):
            ts, ts2 = (t["ts_row"], t["ts2_row"]) if pt else (torch.tensor([SIGMA], device=dev), torch.tensor([SIGMA_NEXT], device=dev))
            mk = dict(mask=t["mask"], clean=t["clean"]) if masked else {}
            prev = t["prev"].clone() if key == "v" else None
            seg[key] = dict(x=t["x"], vel_cond=t["vc"], vel_uncond=t["vu"], timesteps=ts, cfg_scale=cfg, **mk)
            d, xp = K.heun_predict(t["x"], t["vc"], t["vu"], ts, cfg, SIGMA, 0.0 if final else SIGMA_NEXT, GAMMA if prev is not None else 0.0, prev, False,
                                   final=final, **mk)
            out = None if final else K.heun_correct(t["x"], d, xp, t["vc2"], t["vu2"], ts2, cfg, SIGMA, SIGMA_NEXT, **mk)
            ge = K.ge_euler_step(t["x"], t["vc"], t["vu"], ts, cfg, GAMMA, prev.clone(), True, SIGMA, SIGMA_NEXT, **mk) if prev is not None else \
                K.guided_euler_step(t["x"], t["vc"], t["vu"], ts, cfg, SIGMA, SIGMA_NEXT, **mk)
            single[key] = dict(d=d, xp=xp, out=out, prev=prev, ge=ge, ts2=ts2, mk=mk)
        pprev = v["prev"].clone()
        (vd, vxp), (ad, axp) = K.heun_predict_pair(dict(seg["v"], prev=pprev), seg["a"], SIGMA, 0.0 if final else SIGMA_NEXT, GAMMA, False, final=final)
        assert torch.equal(vd, single["v"]["d"]) and torch.equal(ad, single["a"]["d"]) and torch.equal(pprev, single["v"]["prev"])
        if final:
            assert vxp is None and axp is None
            continue
        assert torch.equal(vxp, single["v"]["xp"]) and torch.equal(axp, single["a"]["xp"])
        cseg = {k: dict(x=t["x"], d=single[k]["d"], xp=single[k]["xp"], vel_cond=t["vc2"], vel_uncond=t["vu2"], timesteps=single[k]["ts2"],
                        cfg_scale=seg[k]["cfg_scale"], **single[k]["mk"]) for k, t in (("v", v), ("a", a))}
        vout, aout = K.heun_correct_pair(cseg["v"], cseg["a"], SIGMA, SIGMA_NEXT)
        assert torch.equal(vout, single["v"]["out"]) and torch.equal(aout, single["a"]["out"])
        gprev = v["prev"].clone()
        vge, age = K.ge_euler_step_pair(dict(seg["v"], prev=gprev), seg["a"], GAMMA, True, SIGMA, SIGMA_NEXT)
        assert torch.equal(vge, single["v"]["ge"]) and torch.equal(age, single["a"]["ge"])


def test_kernel_refusals(dev):
    from ltx_2_mlx_amd import kernels as K
    t = _case(9, 8, dev)
    ts = torch.tensor([SIGMA], device=dev)
    with pytest.raises(ValueError, match="GE state"):
        K.heun_predict(t["x"], t["vc"], None, ts, 3.0, SIGMA, SIGMA_NEXT, 0.0, t["prev"].clone(), True)
    with pytest.raises(ValueError, match="GE state"):
        K.heun_predict(t["x"], t["vc"], None, ts, 3.0, SIGMA, SIGMA_NEXT, 2.0, None, True)
    with pytest.raises(ValueError, match="sigma"):
        K.heun_predict(t["x"], t["vc"], None, ts, 3.0, 0.0, SIGMA_NEXT)
    with pytest.raises(ValueError, match="sigma_next"):
        K.heun_correct(t["x"], t["x"], t["x"], t["vc"], None, ts, 3.0, SIGMA, 0.0)


# ------------------------------------------------------------------ shared tiny models
class Tiny:
    pass


@pytest.fixture(scope="module")
def tiny(dev):
    """The smallest video model of tests/test_parity.py: 12 tokens (2 x 2 x 3), frame 0 conditioned in the masked form."""
    from oracle import loop
    t = Tiny()
    t.cfg, t.wq, t.m = make_dit(dev, heads=2, layers=2, cap=64, seed=11)
    g = torch.Generator().manual_seed(4321)
    t.grid = (2, 2, 3)
    t.pos = loop.video_positions(1, 2, 2, 3, 25.0)
    t.lat, t.clean = torch.randn(1, 12, 128, generator=g), torch.randn(1, 12, 128, generator=g)
    t.mask = torch.ones(1, 12, 1)
    t.mask[:, :3] = 0.0
    t.mask[:, 3:6] = 0.1
    t.ctx, t.nctx = 0.1 * torch.randn(1, 24, 64, generator=g), 2.0 * torch.randn(1, 24, 64, generator=g)
    return t


@pytest.fixture(scope="module", params=[False, True], ids=["ltx20", "ltx23"])
def tiny_av(dev, request):
    """The smallest AudioVideo models of tests/test_parity.py: 12 video + 9 audio tokens."""
    from oracle import dit_av, loop
    t = Tiny()
    t.v23 = request.param
    t.cfg, _, t.wq, t.m = make_av(dev, t.v23, seed=23)
    g = torch.Generator().manual_seed(99)
    t.pos, t.apos = loop.video_positions(1, 2, 2, 3, 25.0), dit_av.audio_positions(1, 9)
    t.lat, t.clean = torch.randn(1, 12, 128, generator=g), torch.randn(1, 12, 128, generator=g)
    t.alat, t.aclean = torch.randn(1, 9, 128, generator=g), torch.randn(1, 9, 128, generator=g)
    t.mask, t.amask = torch.ones(1, 12, 1), torch.ones(1, 9, 1)
    t.mask[:, :3] = 0.0
    t.mask[:, 3:6] = 0.1
    wv, wa = t.cfg.caption_channels or t.cfg.inner_dim, t.cfg.caption_channels or t.cfg.audio_inner_dim
    t.ctx, t.actx = 0.1 * torch.randn(1, 24, wv, generator=g), 0.1 * torch.randn(1, 24, wa, generator=g)
    t.nctx, t.nactx = 2.0 * torch.randn(1, 24, wv, generator=g), 2.0 * torch.randn(1, 24, wa, generator=g)
    return t


def _state(lat, mask, pos, clean, dev, masked):
    from ltx_2_mlx_amd.types import LatentState
    return LatentState(latent=lat.clone().to(dev), denoise_mask=(mask if masked else torch.ones_like(mask)).to(dev), positions=pos.to(dev),
                       clean_latent=clean.to(dev))


def _sigmas(steps=4):
    from ltx_2_mlx_amd.components import LTX2Scheduler
    return [float(s) for s in LTX2Scheduler().execute(steps=steps)]


# ------------------------------------------------------------------ 2. the step entries
def test_step_entries_equal_their_parts(dev, tiny):
    """heun_step_ / ge_step_ == ltx2_dit_forward into the velocity buffers, then the Op launches: the same kernels in the same order, the same
    bits.  Per-token and uniform timesteps; with and without the negative context; GE off, first and continued; the sigma_next == 0 form."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import Modality
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    ctx, nctx, pos = t.ctx.to(dev), t.nctx.to(dev), t.pos.to(dev)
    mask1, clean = t.mask[0].reshape(-1).to(dev).contiguous(), t.clean[0].to(dev).contiguous()
    cfg = 3.0
    for per_token in (True, False):
        m.prepare(ctx, pos, per_token=per_token)
        neg.prepare(nctx, pos, per_token=per_token)
        kw = dict(denoise_mask=mask1, clean_latent=clean) if per_token else {}
        mk = dict(mask=mask1, clean=clean) if per_token else {}
        for guided in (True, False):
            def mod(x, s, c):
                ts = (t.mask.to(dev) * s) if per_token else torch.tensor([s], device=dev)
                return Modality(latent=x[None], context=c, context_mask=None, timesteps=ts, positions=pos, sigma=torch.tensor([s], device=dev))

            def velocities(x, s):
                return m(mod(x, s, ctx))[0].clone(), (neg(mod(x, s, nctx))[0].clone() if guided else None)

            # two GE steps in a row, then a step to sigma 0: the engine's kept velocity against one carried here
            lat, want, prev = t.lat[0].to(dev).contiguous(), t.lat[0].to(dev).contiguous(), torch.zeros(12, 128, device=dev)
            for i, (s, sn) in enumerate(((0.9, 0.6), (0.6, 0.3), (0.3, 0.0))):
                vc, vu = velocities(want, s)
                ts = mod(want, s, ctx).timesteps.reshape(-1)
                d, xp = K.heun_predict(want, vc, vu, ts, cfg, s, sn, GAMMA, prev, i == 0, final=sn == 0, **mk)
                if sn != 0:
                    vc2, vu2 = velocities(xp, sn)
                    d = K.heun_correct(want, d, xp, vc2, vu2, mod(xp, sn, ctx).timesteps.reshape(-1), cfg, s, sn, **mk)
                want = d
                m.heun_step_(neg if guided else None, lat, mod(lat, s, ctx), None if sn == 0 else mod(lat, sn, ctx), s, sn, cfg, GAMMA, i == 0, **kw)
                assert torch.equal(lat, want), f"heun per_token={per_token} guided={guided} step {i}: {int((lat != want).sum())} elements differ"
            assert bool(torch.isfinite(lat).all())
            if per_token:
                assert torch.equal(lat[:3], clean[:3])                                     # mask 0 tokens end on their clean values
            lat, want = t.lat[0].to(dev).contiguous(), t.lat[0].to(dev).contiguous()
            for i, (s, sn) in enumerate(((0.9, 0.6), (0.6, 0.3))):
                vc, vu = velocities(want, s)
                want = K.ge_euler_step(want, vc, vu, mod(want, s, ctx).timesteps.reshape(-1), cfg, GAMMA, prev, i == 0, s, sn, **mk)
                m.ge_step_(neg if guided else None, lat, mod(lat, s, ctx), s, sn, cfg, GAMMA, i == 0, **kw)
                assert torch.equal(lat, want), f"ge per_token={per_token} guided={guided} step {i}"
            # without GE the Heun step keeps no state
            lat = t.lat[0].to(dev).contiguous()
            vc, vu = velocities(lat, 0.9)
            d, xp = K.heun_predict(lat, vc, vu, mod(lat, 0.9, ctx).timesteps.reshape(-1), cfg, 0.9, 0.6, **mk)
            vc2, vu2 = velocities(xp, 0.6)
            want = K.heun_correct(lat, d, xp, vc2, vu2, mod(xp, 0.6, ctx).timesteps.reshape(-1), cfg, 0.9, 0.6, **mk)
            m.heun_step_(neg if guided else None, lat, mod(lat, 0.9, ctx), mod(lat, 0.6, ctx), 0.9, 0.6, cfg, **kw)
            assert torch.equal(lat, want)


def test_step_entry_av_equals_its_parts(dev, tiny_av):
    """heun_step_av_ == two ltx2_dit_forward_av per context and the pair launches; GE on the video alone."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import Modality
    t, m = tiny_av, tiny_av.m
    neg = m.clone_sharing_weights()
    dv = lambda x: x.to(dev)          # noqa: E731
    m.prepare(dv(t.ctx), dv(t.pos), per_token=True, audio_context=dv(t.actx), audio_positions=dv(t.apos))
    neg.prepare(dv(t.nctx), dv(t.pos), per_token=True, audio_context=dv(t.nactx), audio_positions=dv(t.apos))
    mask1, clean = dv(t.mask[0].reshape(-1)).contiguous(), dv(t.clean[0]).contiguous()

    def mods(x, ax, s, c, ac):
        sg = torch.tensor([s], device=dev)
        return (Modality(latent=x[None], context=c, context_mask=None, timesteps=dv(t.mask) * s, positions=dv(t.pos), sigma=sg),
                Modality(latent=ax[None], context=ac, context_mask=None, timesteps=sg, positions=dv(t.apos), sigma=sg))

    def velocities(x, ax, s):
        p, n = m(*mods(x, ax, s, dv(t.ctx), dv(t.actx))), neg(*mods(x, ax, s, dv(t.nctx), dv(t.nactx)))
        return [y[0].clone() for y in (*p, *n)]

    lat, alat = dv(t.lat[0]).contiguous(), dv(t.alat[0]).contiguous()
    wv, wa, prev = lat.clone(), alat.clone(), torch.zeros_like(lat)
    for i, (s, sn) in enumerate(((0.9, 0.5), (0.5, 0.0))):
        vc, ac, vu, au = velocities(wv, wa, s)
        ts, ats = dv(t.mask).reshape(-1) * s, torch.tensor([s], device=dev)
        vseg = dict(x=wv, vel_cond=vc, vel_uncond=vu, timesteps=ts, cfg_scale=3.0, mask=mask1, clean=clean, prev=prev)
        aseg = dict(x=wa, vel_cond=ac, vel_uncond=au, timesteps=ats, cfg_scale=7.0)
        (vd, vxp), (ad, axp) = K.heun_predict_pair(vseg, aseg, s, sn, GAMMA, i == 0, final=sn == 0)
        if sn != 0:
            vc2, ac2, vu2, au2 = velocities(vxp, axp, sn)
            vd, ad = K.heun_correct_pair(dict(x=wv, d=vd, xp=vxp, vel_cond=vc2, vel_uncond=vu2, timesteps=dv(t.mask).reshape(-1) * sn, cfg_scale=3.0,
                                              mask=mask1, clean=clean),
                                         dict(x=wa, d=ad, xp=axp, vel_cond=ac2, vel_uncond=au2, timesteps=torch.tensor([sn], device=dev), cfg_scale=7.0), s, sn)
        wv, wa = vd, ad
        nxt = (None, None) if sn == 0 else mods(lat, alat, sn, dv(t.ctx), dv(t.actx))
        m.heun_step_av_(neg, lat, alat, *mods(lat, alat, s, dv(t.ctx), dv(t.actx)), *nxt, s, sn, 3.0, 7.0, GAMMA, i == 0, denoise_mask=mask1, clean_latent=clean)
        assert torch.equal(lat, wv) and torch.equal(alat, wa), f"step {i}: {int((lat != wv).sum())} video, {int((alat != wa).sum())} audio elements differ"
    assert bool(torch.isfinite(lat).all()) and bool(torch.isfinite(alat).all())


# ------------------------------------------------------------------ 3. the loops
@pytest.mark.parametrize("masked", [True, False])
def test_captured_loop_equals_per_step_loop(dev, tiny, masked):
    """The captured graph == one heun_step_ call per step, bit for bit, over 4 scheduler steps, and a second replay on a fresh latent equals the
    first: a replay leaves nothing behind that the next one reads.  (That does not show the memset node at the head of the chain: step 0 runs
    with first = 1 and never reads the kept velocity, so the node has no effect a test could see.)"""
    from ltx_2_mlx_amd.components import CFGGuider
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import heun_denoise_loop
    t, x0m, sig = tiny, X0Model(tiny.m), _sigmas(4)
    st = lambda: _state(t.lat, t.mask, t.pos, t.clean, dev, masked)          # noqa: E731
    for guider, gamma in ((CFGGuider(3.0), GAMMA), (CFGGuider(3.0), 0.0), (CFGGuider(1.0), GAMMA)):
        run = lambda **k: heun_denoise_loop(x0m, st(), None, sig, t.ctx.to(dev), None, t.nctx.to(dev), None, guider, None, gamma, **k)[0].latent      # noqa: E731
        graph, eager = run(use_hip_graph=True), run(use_hip_graph=False)
        assert torch.equal(graph, eager), (guider.scale, gamma, int((graph != eager).sum()))
        seen = []
        assert torch.equal(run(callback=lambda i, n: seen.append((i, n))), eager) and seen == [(i + 1, 4) for i in range(4)]
        # the graph of the last capture is still there: replay it on a fresh latent twice
        model = t.m
        lat = st().latent[0].float().contiguous()
        neg = model.clone_sharing_weights()
        model.prepare(t.ctx.to(dev), t.pos.to(dev), per_token=masked)
        neg.prepare(t.nctx.to(dev), t.pos.to(dev), per_token=masked)
        cond = dict(denoise_mask=t.mask[0].reshape(-1).to(dev).contiguous(), clean_latent=t.clean[0].to(dev).contiguous()) if masked else {}
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            model.capture_heun_graph(neg if guider.enabled() else None, lat, sig, guider.scale, gamma, **cond)
            outs = []
            for _ in range(2):
                lat.copy_(t.lat[0].to(dev))
                model.replay_heun_graph()
                outs.append(lat.clone())
        side.synchronize()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0][None], eager), (guider.scale, gamma)


FUSED_VS_EAGER = 5 * 2.7e-7        # 5 x the largest figure measured on the MI355X, see test_fused_equals_eager_within_roundoff


def test_fused_equals_eager_within_roundoff(dev, tiny):
    """heun_denoise_loop / ge_denoise_loop: fused=True against fused=False, the same forwards with the x0 formed by other kernels (X0Model's
    contracted x - t*v and the plain Euler kernel against the individually rounded passes; (x - d)/sigma against (x - d)*(1/sigma)).  The two
    latents differ by about an fp32 ulp per operation, 1e-7 relative.  Fed to a forward, whose input is rounded to 16 bits (spacing 2^-8 relative),
    such a difference flips the rounding of a fraction 1e-7 / 2^-8 = 2.6e-5 of the elements by 2^-8 each: sqrt(2.6e-5) * 2^-8 = 2e-5 rel-L2 per
    forward where one flips; on these 12-token latents (1536 elements) none does.  Measured on the MI355X, rel-L2 of the final latents: video-only
    9.1e-8 .. 1.5e-7 over the six cases, joint 9.4e-8 .. 1.1e-7 (video) and 2.5e-7 .. 2.6e-7 (audio).  Gate: 5 x the largest, 1.35e-6."""
    from ltx_2_mlx_amd.components import CFGGuider
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import ge_denoise_loop, heun_denoise_loop
    t, sig = tiny, _sigmas(4)
    x0m = X0Model(t.m)
    for loop_fn, gamma in ((heun_denoise_loop, 0.0), (heun_denoise_loop, GAMMA), (ge_denoise_loop, GAMMA)):
        for masked in (True, False):
            run = lambda fused: loop_fn(x0m, _state(t.lat, t.mask, t.pos, t.clean, dev, masked), None, sig, t.ctx.to(dev), None, t.nctx.to(dev), None,      # noqa: E731
                                        CFGGuider(3.0), None, gamma, use_hip_graph=False, fused=fused)[0].latent
            e = measure(f"{loop_fn.__name__} gamma={gamma} masked={masked}: fused vs eager", rel_l2(run(True).cpu(), run(False).cpu()))
            assert e <= FUSED_VS_EAGER


def test_joint_fused_equals_eager_within_roundoff(dev, tiny_av):
    """The same for the joint audio+video Heun + GE loop; figures and gate in test_fused_equals_eager_within_roundoff."""
    from ltx_2_mlx_amd.components import CFGGuider
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import heun_denoise_loop
    a, sig = tiny_av, _sigmas(4)
    x0a = X0Model(a.m)
    dv = lambda x: x.to(dev)          # noqa: E731
    run = lambda fused: heun_denoise_loop(x0a, _state(a.lat, a.mask, a.pos, a.clean, dev, True), _state(a.alat, a.amask, a.apos, a.aclean, dev, False), sig,      # noqa: E731
                                          dv(a.ctx), dv(a.actx), dv(a.nctx), dv(a.nactx), CFGGuider(3.0), CFGGuider(7.0), GAMMA, use_hip_graph=False, fused=fused)
    (fv, fa), (ev, ea) = run(True), run(False)
    assert measure("joint heun: fused vs eager, video", rel_l2(fv.latent.cpu(), ev.latent.cpu())) <= FUSED_VS_EAGER
    assert measure("joint heun: fused vs eager, audio", rel_l2(fa.latent.cpu(), ea.latent.cpu())) <= FUSED_VS_EAGER


# rel-L2 of the final latent against the fp32 oracle, measured on the MI355X: (cfg_scale, frame 0 conditioned) -> loop -> figure
PARITY_MEASURED = {(3.0, True): {"heun": 6.306e-4, "heun+ge": 8.210e-4, "euler+ge": 1.337e-3},
                   (3.0, False): {"heun": 8.583e-4, "heun+ge": 1.183e-3, "euler+ge": 1.934e-3},
                   (7.0, True): {"heun": 1.431e-3, "heun+ge": 1.874e-3, "euler+ge": 3.411e-3},
                   (7.0, False): {"heun": 2.232e-3, "heun+ge": 2.886e-3, "euler+ge": 4.918e-3}}
# the joint Heun + GE loop: LTX-2.3 form -> (video, audio)
JOINT_MEASURED = {False: (1.128e-3, 2.197e-3), True: (1.205e-3, 2.146e-3)}


@pytest.mark.parametrize("masked", [True, False], ids=["frame0", "uniform"])
@pytest.mark.parametrize("cfg_scale", [3.0, 7.0])
def test_loops_against_the_fp32_oracle(dev, tiny, masked, cfg_scale):
    """4 scheduler steps on the 12-token model against tests/heun_ref.py over oracle.dit: Heun, Heun + GE and Euler + GE.  The yardstick is the
    existing guided Euler loop on the same model in the same run: Heun is the same forwards twice.  Each loop is gated at the smaller of 5 x its
    own measured figure (PARITY_MEASURED) and 5 x what guided Euler measures here.  Measured on the MI355X, guided Euler: 8.24e-4 / 1.17e-3 at
    cfg 3 (frame 0 conditioned / uniform), 2.04e-3 / 2.75e-3 at cfg 7."""
    from oracle import dit
    from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import ge_denoise_loop, guided_denoise_loop, heun_denoise_loop
    import keyframe_ref
    t, sig = tiny, _sigmas(4)
    mask = t.mask if masked else torch.ones_like(t.mask)
    x0 = lambda c: (lambda x, ts, s: dit.x0_model(x, c, ts, t.pos, t.wq, t.cfg))          # noqa: E731
    x0m, guider = X0Model(t.m), CFGGuider(cfg_scale)
    st = lambda: _state(t.lat, t.mask, t.pos, t.clean, dev, masked)          # noqa: E731
    args = (t.ctx.to(dev), None, t.nctx.to(dev), None, guider, None)
    yard = guided_denoise_loop(x0m, st(), sig, t.ctx.to(dev), t.nctx.to(dev), guider, EulerDiffusionStep(), use_hip_graph=False).latent.cpu()
    e0 = measure(f"guided Euler loop vs fp32 (cfg {cfg_scale}, masked={masked})", rel_l2(yard, keyframe_ref.guided_loop(t.lat, mask, t.clean, x0(t.ctx), x0(t.nctx), sig, cfg_scale)))
    for name, fn, heun, gamma in (("heun", heun_denoise_loop, True, 0.0), ("heun+ge", heun_denoise_loop, True, GAMMA), ("euler+ge", ge_denoise_loop, False, GAMMA)):
        got = fn(x0m, st(), None, sig, *args, gamma, use_hip_graph=False)[0].latent.cpu()
        ref = R.video_loop(heun, t.lat, mask, t.clean, x0(t.ctx), x0(t.nctx), sig, cfg_scale, gamma)
        e = measure(f"{name} loop vs fp32 (cfg {cfg_scale}, masked={masked})", rel_l2(got, ref))
        print(f"{name}: rel-L2 = {e:.4e}   guided Euler: {e0:.4e}")
        assert bool(torch.isfinite(got).all()) and rel_l2(got, yard) > 1e-3, name          # another trajectory than Euler's
        assert e <= min(5 * PARITY_MEASURED[(cfg_scale, masked)][name], 5 * e0), name


def test_joint_loop_against_the_fp32_oracle(dev, tiny_av):
    """The joint Heun + GE loop on the 12 + 9 token AudioVideo models (LTX-2.0 and LTX-2.3 forms) against tests/heun_ref.py over oracle.dit_av;
    each modality is gated at the smaller of 5 x its own measured figure (JOINT_MEASURED) and 5 x what the existing joint guided Euler loop
    measures for the SAME modality on the same model in this run (on the MI355X: video 1.16e-3 / 1.28e-3, audio 2.86e-3 / 2.90e-3)."""
    from oracle import dit_av
    from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import heun_denoise_loop, joint_guided_denoise_loop
    t, sig = tiny_av, _sigmas(4)
    dv = lambda x: x.to(dev)          # noqa: E731

    def x0(c, ac):
        def fn(xs, ts, s):
            sg = torch.tensor([s])
            return dit_av.av_x0_model(dict(latent=xs[0], context=c, timesteps=ts[0], sigma=sg, positions=t.pos),
                                      dict(latent=xs[1], context=ac, timesteps=ts[1], sigma=sg, positions=t.apos), t.wq, t.cfg)
        return fn

    mods = lambda: [dict(tokens=t.lat, mask=t.mask, clean=t.clean, cfg_scale=3.0), dict(tokens=t.alat, mask=t.amask, clean=t.aclean, cfg_scale=7.0)]      # noqa: E731
    states = lambda: (_state(t.lat, t.mask, t.pos, t.clean, dev, True), _state(t.alat, t.amask, t.apos, t.aclean, dev, False))          # noqa: E731
    x0m = X0Model(t.m)
    yv, ya = joint_guided_denoise_loop(x0m, *states(), sig, dv(t.ctx), dv(t.actx), dv(t.nctx), dv(t.nactx), 3.0, 7.0, EulerDiffusionStep(), use_hip_graph=False)
    rv, ra = R.sample_loop(False, mods(), x0(t.ctx, t.actx), x0(t.nctx, t.nactx), sig)
    e0v, e0a = measure("joint guided Euler vs fp32, video", rel_l2(yv.latent.cpu(), rv)), measure("joint guided Euler vs fp32, audio", rel_l2(ya.latent.cpu(), ra))
    gv, ga = heun_denoise_loop(x0m, *states(), sig, dv(t.ctx), dv(t.actx), dv(t.nctx), dv(t.nactx), CFGGuider(3.0), CFGGuider(7.0), GAMMA, use_hip_graph=False)
    rv, ra = R.sample_loop(True, mods(), x0(t.ctx, t.actx), x0(t.nctx, t.nactx), sig, GAMMA)
    ev, ea = measure("joint heun+ge vs fp32, video", rel_l2(gv.latent.cpu(), rv)), measure("joint heun+ge vs fp32, audio", rel_l2(ga.latent.cpu(), ra))
    print(f"joint heun+ge: video {ev:.4e} audio {ea:.4e}   joint guided Euler: video {e0v:.4e} audio {e0a:.4e}")
    mv, ma = JOINT_MEASURED[t.v23]
    assert ev <= min(5 * mv, 5 * e0v) and ea <= min(5 * ma, 5 * e0a)


# ------------------------------------------------------------------ 4. the pipeline
def _pipeline_states(pipe, conf, noise, anoise, dev):
    """The states OneStagePipeline.__call__ hands its loop for `conf` and the supplied noise, made with the pipeline's own tools
    -> (video tools, video state, audio tools, audio state; the audio pair None without anoise)."""
    from ltx_2_mlx_amd.pipelines.common import conditioned_initial_state, seeded_noiser, video_tools_for
    from ltx_2_mlx_amd.types import AudioLatentShape, VideoPixelShape
    noiser = seeded_noiser(dev, conf.seed)
    vt = video_tools_for(pipe.patchifier, conf.num_frames, conf.height, conf.width, conf.fps)
    vs = noiser(conditioned_initial_state(vt, [], conf.dtype, dev), noise_scale=1.0, noise=noise)
    if anoise is None:
        return vt, vs, None, None
    shape = AudioLatentShape.from_video_pixel_shape(VideoPixelShape(batch=1, frames=conf.num_frames, height=conf.height, width=conf.width, fps=conf.fps),
                                                    channels=conf.audio_vae_channels, mel_bins=conf.audio_mel_bins, sample_rate=conf.audio_sample_rate,
                                                    hop_length=conf.audio_hop_length, audio_latent_downsample_factor=conf.audio_downsample_factor)
    at = pipe._create_audio_tools(shape)
    return vt, vs, at, noiser(at.create_initial_state(dtype=conf.dtype, device=dev), noise_scale=1.0, noise=anoise)


def test_one_stage_pipeline_heun_video(dev, tiny):
    """OneStagePipeline(sampler="heun", ge_gamma=2) at 64x96x9 == heun_denoise_loop(fused=True) on the same state and sigmas, bit for bit; under the
    config's default CFG* it takes the eager form; Euler + GE likewise."""
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    from ltx_2_mlx_amd.pipelines.common import final_latent, ge_denoise_loop, heun_denoise_loop
    t = tiny
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(1, 12, 128, generator=g)
    kw = dict(height=64, width=96, num_frames=9, seed=1, fps=25.0, num_inference_steps=4, cfg_scale=3.0, rescale_scale=0.0)
    pipe = OneStagePipeline(t.m, None, None)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    vt = _pipeline_states(pipe, OneStageCFGConfig(**kw), noise.to(dev), None, dev)[0]
    state = lambda: _pipeline_states(pipe, OneStageCFGConfig(**kw), noise.to(dev), None, dev)[1]          # noqa: E731
    unpatch = lambda tokens: final_latent(vt, state().replace(latent=tokens))          # noqa: E731
    sig = pipe.scheduler.execute(steps=4)
    for graph in (False, True):
        lat, _ = pipe(ctx, nctx, OneStageCFGConfig(use_hip_graph=graph, **kw), sampler="heun", ge_gamma=GAMMA, initial_noise=noise.to(dev))
        want = heun_denoise_loop(X0Model(t.m), state(), None, sig, ctx, None, nctx, None, CFGGuider(3.0), None, GAMMA, use_hip_graph=graph)[0].latent
        assert torch.equal(lat, unpatch(want)), graph
    lat_ge, _ = pipe(ctx, nctx, OneStageCFGConfig(**kw), ge_gamma=GAMMA, initial_noise=noise.to(dev))
    want = ge_denoise_loop(X0Model(t.m), state(), None, sig, ctx, None, nctx, None, CFGGuider(3.0), None, GAMMA)[0].latent
    assert torch.equal(lat_ge, unpatch(want)) and not torch.equal(lat_ge, lat)
    plain, _ = pipe(ctx, nctx, OneStageCFGConfig(**kw), initial_noise=noise.to(dev))
    assert rel_l2(lat.cpu(), plain.cpu()) > 1e-3 and rel_l2(lat_ge.cpu(), plain.cpu()) > 1e-3
    # CFG* (rescale_scale 0.7, the default): the eager form
    star, _ = pipe(ctx, nctx, OneStageCFGConfig(**dict(kw, rescale_scale=0.7)), sampler="heun", ge_gamma=GAMMA, initial_noise=noise.to(dev))
    want = heun_denoise_loop(X0Model(t.m), state(), None, sig, ctx, None, nctx, None, CFGStarRescalingGuider(3.0), None, GAMMA, fused=False)[0].latent
    assert torch.equal(star, unpatch(want)) and bool(torch.isfinite(star).all())
    with pytest.raises(ValueError, match="device form"):
        heun_denoise_loop(X0Model(t.m), state(), None, sig, ctx, None, nctx, None, CFGStarRescalingGuider(3.0), None, GAMMA, fused=True)
    # the refusals that stay
    with pytest.raises(ValueError, match="sampler='dpm'"):
        pipe(ctx, nctx, OneStageCFGConfig(**kw), sampler="dpm")
    with pytest.raises(NotImplementedError, match="sampler='heun'"):
        pipe(ctx, nctx, OneStageCFGConfig(**kw), sampler="heun", stg_scale=1.0)
    with pytest.raises(NotImplementedError, match="GE velocity"):
        pipe(ctx, nctx, OneStageCFGConfig(**kw), ge_gamma=GAMMA, stg_scale=1.0)
    with pytest.raises(NotImplementedError, match="cross_attn_scale"):
        pipe(ctx, nctx, OneStageCFGConfig(**kw), sampler="heun", cross_attn_scale=2.0)
    with pytest.raises(NotImplementedError, match="temporal upscaler"):
        pipe(ctx, nctx, OneStageCFGConfig(**kw), sampler="heun", temporal_upscaler=object())


def test_one_stage_pipeline_heun_audio_video(dev, tiny_av):
    """The same on an AudioVideo transformer: both final latents equal heun_denoise_loop(fused=True)'s bit for bit."""
    from ltx_2_mlx_amd.components import CFGGuider
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    from ltx_2_mlx_amd.pipelines.common import final_latent, heun_denoise_loop
    t = tiny_av
    dv = lambda x: x.to(dev)          # noqa: E731
    g = torch.Generator().manual_seed(6)
    noise, anoise = torch.randn(1, 12, 128, generator=g), torch.randn(1, 9, 128, generator=g)
    conf = OneStageCFGConfig(height=64, width=96, num_frames=9, seed=1, fps=25.0, num_inference_steps=4, cfg_scale=3.0, audio_cfg_scale=7.0, rescale_scale=0.0,
                             audio_enabled=True)
    pipe = OneStagePipeline(t.m, None, None)
    lat, aud = pipe(dv(t.ctx), dv(t.nctx), conf, positive_audio_encoding=dv(t.actx), negative_audio_encoding=dv(t.nactx), sampler="heun", ge_gamma=GAMMA,
                    initial_noise=dv(noise), initial_audio_noise=dv(anoise))
    vt, vs, at, as_ = _pipeline_states(pipe, conf, dv(noise), dv(anoise), dev)
    assert as_.latent.shape == (1, 9, 128)
    wv, wa = heun_denoise_loop(X0Model(t.m), vs, as_, pipe.scheduler.execute(steps=4), dv(t.ctx), dv(t.actx), dv(t.nctx), dv(t.nactx), CFGGuider(3.0), CFGGuider(7.0), GAMMA)
    assert torch.equal(lat, final_latent(vt, wv)) and torch.equal(aud, final_latent(at, wa))
    assert bool(torch.isfinite(lat).all()) and bool(torch.isfinite(aud).all())


def test_engine_refusals(dev, tiny):
    """Each returns an error and launches nothing: the latent is untouched."""
    from ltx_2_mlx_amd import _native as nv
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    m.prepare(t.ctx.to(dev), t.pos.to(dev), per_token=False)
    neg.prepare(t.nctx.to(dev), t.pos.to(dev), per_token=False)
    lat = t.lat[0].to(dev).contiguous()
    keep = lat.clone()
    ts = torch.tensor([0.5], device=dev)
    L, p = nv.lib(), nv.ptr

    def heun(a, b, sigma=0.5, sigma_next=0.25, gamma=0.0, first=1, ts_next=ts):
        nv.check(L.ltx2_dit_heun_step(a, b, p(lat), p(ts), 1, None, p(ts_next), None, None, None, 3.0, gamma, first, sigma, sigma_next, nv.stream()))

    with pytest.raises(ValueError, match="ctx == neg"):
        heun(m._h, m._h)
    for s, sn in ((0.0, 0.0), (-0.5, 0.25), (0.5, -0.1)):
        with pytest.raises(ValueError, match="sigma"):
            heun(m._h, neg._h, sigma=s, sigma_next=sn)
    with pytest.raises(ValueError, match="ge_gamma"):
        heun(m._h, neg._h, gamma=-1.0)
    with pytest.raises(ValueError, match="ts_next"):
        heun(m._h, neg._h, ts_next=None)
    with pytest.raises(ValueError, match="ge_gamma"):
        nv.check(L.ltx2_dit_ge_step(m._h, neg._h, p(lat), p(ts), 1, None, None, None, 3.0, 0.0, 1, 0.5, 0.25, nv.stream()))
    with pytest.raises(ValueError, match="mask and clean"):
        nv.check(L.ltx2_dit_ge_step(m._h, neg._h, p(lat), p(ts), 1, None, p(ts), None, 3.0, 2.0, 1, 0.5, 0.25, nv.stream()))
    # first == 0 continues a GE loop: refused until a GE step with first != 0 has run on this workspace -- a step without GE allocates it and
    # leaves the velocity unfilled
    fresh = neg.clone_sharing_weights()          # a third context over the same weights, its workspace never touched
    fresh.prepare(t.ctx.to(dev), t.pos.to(dev), per_token=False)
    with pytest.raises(RuntimeError, match="first == 0"):
        heun(fresh._h, neg._h, gamma=2.0, first=0)
    torch.cuda.synchronize()
    assert torch.equal(lat, keep)
    scratch = lat.clone()

    def on_scratch(fn, *a):
        nv.check(fn(fresh._h, neg._h, p(scratch), p(ts), 1, None, *a, nv.stream()))

    on_scratch(L.ltx2_dit_heun_step, p(ts), None, None, None, 3.0, 0.0, 1, 0.5, 0.25)                  # no GE: the workspace exists now
    for fn, a in ((L.ltx2_dit_heun_step, (p(ts), None, None, None, 3.0, 2.0, 0, 0.5, 0.25)), (L.ltx2_dit_ge_step, (None, None, 3.0, 2.0, 0, 0.5, 0.25))):
        with pytest.raises(RuntimeError, match="first == 0"):
            on_scratch(fn, *a)
    on_scratch(L.ltx2_dit_ge_step, None, None, 3.0, 2.0, 1, 0.5, 0.25)                                  # a first step fills it
    on_scratch(L.ltx2_dit_heun_step, p(ts), None, None, None, 3.0, 2.0, 0, 0.25, 0.125)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(scratch).all())
