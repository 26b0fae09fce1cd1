"""Projected guidance (CFG*, APG, legacy APG with momentum) on the GPU: the two kernels' element-wise part bit for bit against a CPU fp32
restatement given the scalars the kernel reports, those scalars within one fp32 ulp of the float64 formula, determinism, the one-call step and
its captured graph against the same kernels called one by one, the loop against the fp32 restatement (with the EXISTING eager guidance as
the yardstick) and the three pipelines.  Tiny models as tests/test_parity.py builds them."""
import numpy as np
import pytest
import torch

from conftest import measure, rel_l2

import projected_guidance_ref as R
from test_keyframe_gpu import _state, tiny  # noqa: F401  (the keyframe tests' tiny DiT and 72 + 48-token state)
from test_parity import make_av, pearson
from test_retake_gpu import _bits, _conf, _hand_state, parts  # noqa: F401  (the retake tests' models and source clip)

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
SHAPES = [(37, 128), (5, 6), (33000, 128)]       # 16-byte form; element-wise form (C % 4 != 0); past one pass of the capped grid
BUILDS = [torch.bfloat16, torch.float16]
SIGMA, SIGMA_NEXT = 0.909375, 0.725


def _inputs(rows, C, seed=0):
    """x, vel_cond standard normal, vel_uncond = 0.7*vel_cond + 0.5*noise, t in [0.2, 1], a mask of 0 / 0.05 / 1."""
    g = torch.Generator().manual_seed(rows * 131 + C + seed)
    x, vc, noise, clean = (torch.randn(rows, C, generator=g) for _ in range(4))
    vu = 0.7 * vc + 0.5 * noise
    ts_row = 0.2 + 0.8 * torch.rand(rows, generator=g)
    mask = torch.ones(rows)
    mask[::3] = 0.0
    mask[1::3] = 0.05
    return x, vc, vu, clean, ts_row, mask


def _padded(t, dev, off=0, fill=None):
    """A device copy of `t` (or a `fill`ed buffer of its shape) that starts `off` floats past an aligned allocation, with 64 sentinels behind
    it -> (view, the whole buffer)."""
    n = t.numel()
    buf = torch.full((n + 64 + off,), SENTINEL, device=dev, dtype=t.dtype)
    view = buf[off:off + n].view(t.shape)
    view.copy_(t) if fill is None else view.fill_(fill)
    return view, buf


def _tail_intact(buf, n, off=0):
    return bool((buf[off + n:] == SENTINEL).all()) and bool((buf[:off] == SENTINEL).all())


def _run(dev, build, x, vc, vu, ts, mk, clean, mode, scale, eta, thr, running=None, first=True, momentum=0.0, in_place=False, off=None):
    """One sums + step pair on the device with a sentinel behind every output -> (out, scalars, running after, partials), all on the CPU.
    off: the name of one operand to place 4 bytes off a 16-byte boundary."""
    from ltx_2_mlx_amd import kernels as K
    rows, C = x.shape
    n = rows * C
    o = lambda name: 1 if off == name else 0
    xd, xbuf = _padded(x, dev, o("x"))
    vcd, _ = _padded(vc, dev, o("vc"))
    vud, _ = _padded(vu, dev, o("vu"))
    cld = None if mk is None else _padded(clean, dev, o("clean"))[0]
    mkd = None if mk is None else mk.to(dev)
    rund = runbuf = None
    if running is not None:
        rund, runbuf = _padded(running, dev, o("running"))
    nb = K.guidance_sums_blocks(rows, C, build)
    part, partbuf = _padded(torch.zeros(nb, 5, dtype=torch.float64), dev, fill=float("nan"))
    sc, scbuf = _padded(torch.zeros(2), dev, fill=SENTINEL)
    outd, outbuf = (xd, xbuf) if in_place else _padded(x, dev, o("out"), fill=SENTINEL)
    tsd = ts.to(dev)
    K.guidance_sums(xd, vcd, vud, tsd, partials=part, running=rund, first=first, momentum=momentum, dtype=build)
    K.projected_euler_step(xd, vcd, vud, tsd, part, mode, scale, eta, thr, SIGMA, SIGMA_NEXT, mask=mkd, clean=cld, running=rund, out=outd, scalars_out=sc,
                           dtype=build)
    assert _tail_intact(outbuf, n, o("x") if in_place else o("out")) and _tail_intact(partbuf, nb * 5) and _tail_intact(scbuf, 2)
    assert runbuf is None or _tail_intact(runbuf, n, o("running"))
    assert bool(torch.isfinite(part).all())                                  # every block wrote its row
    if mode == 0:
        assert float(sc[1]) == SENTINEL                                      # one scalar reported, one stored
    return outd.cpu(), sc.cpu(), None if rund is None else rund.cpu(), part.cpu()


def _check(tag, x, vc, vu, ts, mk, clean, mode, scale, eta, thr, got, g=None):
    """got = _run(...)'s result against the restatement: the element-wise part bit for bit given the reported scalars, the scalars within one
    fp32 ulp of the float64 formula (the bound is derived in DESIGN.md: relative error of each sum below 20 * n * 2^-53 < 1e-8 for inputs
    whose sums satisfy |sum t| >= 0.05 sum |t|, asserted here)."""
    out, sc, _, _ = got
    a, b = R.x0_pair(x, vc, vu, ts)
    g = a - b if g is None else g
    s, sabs = R.sums_f64(a, b, g)
    for k in ((1, 2) if mode == 0 else (0, 3, 4)):
        assert abs(s[k]) >= 0.05 * sabs[k], f"{tag}: the input is ill-conditioned for sum {k}"
    want = R.scalars_f64(s, mode, thr)
    for k, w in enumerate(want):
        u = R.ulps(float(sc[k]), w)
        assert u <= 1.0, f"{tag}: scalar {k} = {float(sc[k])!r} is {u} ulp from {w!r}"
    ref = R.projected_step(x, a, b, g, mk, clean if mk is not None else None, mode, scale, eta, float(sc[0]), float(sc[1]) if mode else 0.0, SIGMA, SIGMA_NEXT)
    assert torch.equal(out, ref), f"{tag}: {int((out != ref).sum())} of {out.numel()} elements differ"
    return s


def _thresholds(x, vc, vu, ts):
    """(0, one that binds, one that does not) from the input's own |g|."""
    a, b = R.x0_pair(x, vc, vu, ts)
    norm = float((a - b).double().norm())
    return 0.0, 0.5 * norm, 2.0 * norm


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("rows,C", SHAPES)
@pytest.mark.parametrize("build", BUILDS)
def test_projected_step_bit_for_bit_and_scalars(dev, build, rows, C):
    """Modes x scalar / per-row timesteps x mask absent / mixed x scale 1, 3, 7.5, with eta over 0, 0.5, 1 and the threshold over 0, binding,
    not binding; out over x.  On 33000 x 128 (4.2 M elements: the shape is there for the grid-stride wrap) one case per mode."""
    x, vc, vu, clean, ts_row, mask = _inputs(rows, C)
    big = rows > 1000
    i = 0
    for mode in (0, 1, 2):
        for ts in ((ts_row,) if big else (torch.tensor([SIGMA]), ts_row)):
            thrs = _thresholds(x, vc, vu, ts)
            for mk in ((mask,) if big else (None, mask)):
                for scale in ((3.0,) if big else (1.0, 3.0, 7.5)):
                    eta, thr = (0.0, 0.5, 1.0)[i % 3], thrs[(i // 3 + i) % 3] if not big else thrs[1]
                    i += 1
                    tag = f"mode{mode} ts{ts.numel()} mask{mk is not None} scale{scale} eta{eta} thr{thr:.3g}"
                    got = _run(dev, build, x, vc, vu, ts, mk, clean, mode, scale, eta, thr)
                    _check(tag, x, vc, vu, ts, mk, clean, mode, scale, eta, thr, got)
                    if mode and thr > 0:
                        assert (float(got[1][0]) < 1.0) == (thr == thrs[1]), tag          # the binding threshold binds, the other does not
                    if scale == 3.0:
                        again = _run(dev, build, x, vc, vu, ts, mk, clean, mode, scale, eta, thr, in_place=True)
                        assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and torch.equal(again[3], got[3]), tag   # in place, and twice the same bits


@pytest.mark.parametrize("rows,C", SHAPES)
@pytest.mark.parametrize("build", BUILDS)
def test_momentum_steps(dev, build, rows, C):
    """Legacy APG with momentum 0.5 over three steps with changing velocities: `running` after each sums pass bit for bit, and the step that
    reads it."""
    x, vc, vu, clean, ts_row, mask = _inputs(rows, C, seed=7)
    running = torch.full_like(x, 7.0)                     # the first step must not read it
    for step in range(3):
        vu_k = vu * (1.0 - 0.1 * step)
        a, b = R.x0_pair(x, vc, vu_k, ts_row)
        want_run = R.guidance(a, b, running, 0.5, first=(step == 0))
        thr = 0.5 * float(want_run.double().norm())
        got = _run(dev, build, x, vc, vu_k, ts_row, mask, clean, 2, 3.0, 0.5, thr, running=running, first=(step == 0), momentum=0.5)
        assert torch.equal(got[2], want_run), f"step {step}: running differs in {int((got[2] != want_run).sum())} elements"
        _check(f"momentum step {step}", x, vc, vu_k, ts_row, mask, clean, 2, 3.0, 0.5, thr, got, g=want_run)
        assert float(got[1][0]) < 1.0
        running = want_run


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("off", ["x", "vc", "vu", "clean", "running", "out"])
def test_each_operand_off_alignment(dev, build, off):
    """37 x 128 with one [rows][C] operand 4 bytes off a 16-byte boundary: the element-wise form, the same properties."""
    x, vc, vu, clean, ts_row, mask = _inputs(37, 128, seed=3)
    prev = torch.randn(37, 128, generator=torch.Generator().manual_seed(9))
    a, b = R.x0_pair(x, vc, vu, ts_row)
    want_run = R.guidance(a, b, prev, 0.5, first=False)
    thr = 0.5 * float(want_run.double().norm())
    got = _run(dev, build, x, vc, vu, ts_row, mask, clean, 2, 3.0, 0.5, thr, running=prev, first=False, momentum=0.5, off=off)
    assert torch.equal(got[2], want_run)
    _check(f"off {off}", x, vc, vu, ts_row, mask, clean, 2, 3.0, 0.5, thr, got, g=want_run)


def test_refusals(dev):
    from ltx_2_mlx_amd import kernels as K
    x, vc, vu, clean, ts_row, mask = (t.to(dev) for t in _inputs(37, 128))
    part = K.guidance_sums(x, vc, vu, ts_row)
    assert part.shape == (K.guidance_sums_blocks(37, 128), 5) and K.guidance_sums_blocks(33000, 128) == 1024
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        K.projected_euler_step(x, vc, vu, ts_row, part, 0, 3.0, 1.0, 0.0, 0.0, 0.5)
    with pytest.raises(ValueError, match="mode=3"):
        K.projected_euler_step(x, vc, vu, ts_row, part, 3, 3.0, 1.0, 0.0, 0.5, 0.25)
    with pytest.raises(ValueError, match="running"):
        K.projected_euler_step(x, vc, vu, ts_row, part, 1, 3.0, 1.0, 0.0, 0.5, 0.25, running=torch.zeros_like(x))
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        R.projected_step(x.cpu(), x.cpu(), x.cpu(), x.cpu(), None, None, 0, 3.0, 1.0, 1.0, 0.0, 0.0, 0.5)


# ------------------------------------------------------------------ 2. the engine step and its graph
GUIDERS = {0: dict(mode=0, scale=3.0, eta=1.0, norm_threshold=0.0, momentum=0.0), 1: dict(mode=1, scale=3.0, eta=0.5, norm_threshold=0.05, momentum=0.0),
           2: dict(mode=2, scale=2.0, eta=0.5, norm_threshold=0.05, momentum=0.5)}


def test_projected_step_equals_its_four_parts(dev, tiny):
    """projected_step_ == ltx2_dit_forward(ctx), ltx2_dit_forward(neg), ltx2_guidance_sums, ltx2_projected_euler_step: the same kernels in
    the same order, so the same bits; two steps in mode 2 so that the engine's running buffer is read.  Per-token and uniform timesteps."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import Modality
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    ctx, nctx, pos = t.ctx.to(dev), t.nctx.to(dev), t.pos.to(dev)
    mask1 = t.mask[0].reshape(-1).to(dev).contiguous()
    clean = t.clean[0].to(dev).contiguous()
    for per_token in (True, False):
        m.prepare(ctx, pos, per_token=per_token)
        neg.prepare(nctx, pos, per_token=per_token)
        mk, cl = (mask1, clean) if per_token else (None, None)
        for mode, ga in GUIDERS.items():
            want, got = t.lat[0].to(dev).contiguous(), t.lat[0].to(dev).contiguous()
            running = torch.zeros_like(want) if ga["momentum"] else None
            for step, (s, sn) in enumerate(((0.909375, 0.725), (0.725, 0.4))):
                ts = (t.mask.to(dev) * s) if per_token else torch.tensor([s], device=dev)
                mod = lambda lat, c: Modality(latent=lat[None], context=c, context_mask=None, timesteps=ts, positions=pos)
                vc, vu = m(mod(want, ctx))[0].clone(), neg(mod(want, nctx))[0].clone()
                part = K.guidance_sums(want, vc, vu, ts.reshape(-1), running=running, first=(step == 0), momentum=ga["momentum"])
                want = K.projected_euler_step(want, vc, vu, ts.reshape(-1), part, mode, ga["scale"], ga["eta"], ga["norm_threshold"], s, sn, mask=mk, clean=cl,
                                              running=running)
                m.projected_step_(neg, got, mod(got, ctx), s, sn, first=(step == 0), denoise_mask=mk, clean_latent=cl, **ga)
                assert torch.equal(got, want), f"per_token={per_token} mode={mode} step={step}: {int((got != want).sum())} elements differ"
            assert bool(torch.isfinite(got).all())
    fresh = neg.clone_sharing_weights()              # a third context, whose running guidance was never started
    fresh.prepare(ctx, pos, per_token=False)
    lat = t.lat[0].to(dev).contiguous()
    ts = torch.tensor([0.5], device=dev)
    with pytest.raises(RuntimeError, match="first"):
        fresh.projected_step_(neg, lat, Modality(latent=lat[None], context=ctx, context_mask=None, timesteps=ts, positions=pos), 0.5, 0.25, first=False, **GUIDERS[2])
    with pytest.raises(ValueError, match="momentum"):
        m.projected_step_(neg, lat, Modality(latent=lat[None], context=ctx, context_mask=None, timesteps=ts, positions=pos), 0.5, 0.25, **dict(GUIDERS[1], momentum=0.5))


def _guider(mode):
    from ltx_2_mlx_amd.components import CFGStarRescalingGuider, LegacyStatefulAPGGuider, LtxAPGGuider
    ga = GUIDERS[mode]
    return (CFGStarRescalingGuider(ga["scale"]), LtxAPGGuider(ga["scale"], ga["eta"], ga["norm_threshold"]),
            LegacyStatefulAPGGuider(ga["scale"], ga["eta"], ga["norm_threshold"], ga["momentum"]))[mode]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_graph_replay_equals_eager_steps(dev, tiny, mode):
    """Graph replay == the eager projected_step_ loop bit for bit, with the keyframe mask and without one; with momentum a second replay of
    the same graph from the same latent equals the first (the memset node at the head of the chain)."""
    from ltx_2_mlx_amd.components import EulerDiffusionStep, LTX2Scheduler
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import projected_denoise_loop
    t = tiny
    sig = [float(s) for s in LTX2Scheduler().execute(steps=3)]
    x0m = X0Model(t.m)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    for masked in (True, False):
        st = _state(t, dev)
        if not masked:
            st = st.replace(denoise_mask=torch.ones_like(st.denoise_mask))
        run = lambda **kw: projected_denoise_loop(x0m, st, sig, ctx, nctx, _guider(mode), EulerDiffusionStep(), **kw).latent
        seen = []
        graph, eager, cb = run(use_hip_graph=True), run(use_hip_graph=False), run(use_hip_graph=True, callback=lambda i, n: seen.append((i, n)))
        assert torch.equal(graph, eager) and torch.equal(cb, eager) and seen == [(1, 3), (2, 3), (3, 3)], (mode, masked)
        assert bool(torch.isfinite(graph).all()) and not torch.equal(graph, st.latent)
    if mode == 2:
        m, neg = t.m, t.m.clone_sharing_weights()
        pos = t.pos.to(dev)
        m.prepare(ctx, pos, per_token=False)
        neg.prepare(nctx, pos, per_token=False)
        lat0 = t.lat[0].to(dev).contiguous()
        lat = lat0.clone()
        outs = []
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.capture_projected_graph(neg, lat, sig, **GUIDERS[2])
            for _ in range(2):
                lat.copy_(lat0)
                m.replay_projected_graph()
                outs.append(lat.clone())
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], eager[0])


# ------------------------------------------------------------------ 3. parity of the loop
@pytest.fixture(scope="module")
def loop_refs(tiny):
    """Four LTX2Scheduler steps at scale 3 in fp32 (oracle.dit.x0_model inside projected_guidance_ref.guided_loop) for CFG* and for APG with a
    threshold at half of the first step's |cond - uncond|, so that it binds; computed once."""
    from oracle import dit
    from ltx_2_mlx_amd.components import CFGStarRescalingGuider, LTX2Scheduler, LtxAPGGuider
    t = tiny
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    x0 = lambda c: (lambda x, ts, s: dit.x0_model(x, c, ts, t.pos, t.wq, t.cfg))
    ts0 = t.mask * sig[0]
    thr = 0.5 * float((x0(t.ctx)(t.lat, ts0, sig[0]) - x0(t.nctx)(t.lat, ts0, sig[0])).norm())
    guiders = dict(cfg_star=CFGStarRescalingGuider(3.0), apg=LtxAPGGuider(3.0, 0.5, thr))
    return sig, {k: (g, R.guided_loop(t.lat, t.mask, t.clean, x0(t.ctx), x0(t.nctx), sig, g)) for k, g in guiders.items()}


@pytest.mark.parametrize("which", ["cfg_star", "apg"])
def test_loop_against_restatement(dev, tiny, loop_refs, which):
    """Against the fp32 restatement the new loop may be at most 1.5 x as far as the EXISTING eager guidance (two X0Model calls + the torch
    guider + ltx2_euler_step): the two differ only in rounding order, the project's rule for such a path.  Pearson > 0.999.  Measured on the MI355X: CFG* E0 = 5.6571e-04,
    E1 = 5.6571e-04; APG E0 = 3.9811e-04, E1 = 3.9811e-04."""
    from ltx_2_mlx_amd.components import EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import joint_denoise_loop, projected_denoise_loop
    t = tiny
    sig, refs = loop_refs
    guider, ref = refs[which]
    x0m = X0Model(t.m)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    new = projected_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, guider, EulerDiffusionStep(), use_hip_graph=True).latent.cpu()
    old = joint_denoise_loop(x0m, False, _state(t, dev), None, sig, ctx, None, EulerDiffusionStep(), use_hip_graph=False,
                             negative_video_context=nctx, video_guider=guider)[0].latent.cpu()
    e0 = measure(f"E0 existing eager {which} guidance vs fp32", rel_l2(old, ref))
    e1 = measure(f"E1 projected {which} loop vs fp32", rel_l2(new, ref))
    print(f"projected loop {which}: E0 = {e0:.4e}  E1 = {e1:.4e}  pearson = {pearson(new, ref):.6f}")
    assert rel_l2(new[:, 72:96], t.clean[:, 72:96]) < 1e-5 and rel_l2(new[:, :72], t.lat[:, :72]) > 0.1
    assert e1 <= 1.5 * e0 and pearson(new, ref) > 0.999


def test_other_guiders_are_handed_on(dev, tiny):
    """A plain CFGGuider goes to guided_denoise_loop, a guider that is not enabled or of another class to joint_denoise_loop."""
    from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep, LTX2Scheduler, LtxAPGGuider
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import guided_denoise_loop, joint_denoise_loop, projected_denoise_loop
    t = tiny
    sig = [float(s) for s in LTX2Scheduler().execute(steps=2)]
    x0m = X0Model(t.m)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    a = projected_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFGGuider(3.0), EulerDiffusionStep()).latent
    assert torch.equal(a, guided_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, CFGGuider(3.0), EulerDiffusionStep()).latent)
    a = projected_denoise_loop(x0m, _state(t, dev), sig, ctx, nctx, LtxAPGGuider(1.0), EulerDiffusionStep()).latent
    b = joint_denoise_loop(x0m, False, _state(t, dev), None, sig, ctx, None, EulerDiffusionStep(), None, True, negative_video_context=nctx,
                           video_guider=LtxAPGGuider(1.0))[0].latent
    assert torch.equal(a, b)


# ------------------------------------------------------------------ 4. the pipelines
def test_one_stage_pipeline_with_a_guider_override(dev, tiny):
    """OneStagePipeline(guider_override=LtxAPGGuider(3, 0.5, 5)) at 64 x 96 x 9 with injected noise: not the CFG run; projected_denoise_loop
    called by hand on the hand-built state, bit for bit; captured == eager with a callback."""
    from ltx_2_mlx_amd.components import EulerDiffusionStep, LTX2Scheduler, LtxAPGGuider, VideoLatentPatchifier
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline, projected_denoise_loop
    from ltx_2_mlx_amd.pipelines.common import conditioned_initial_state, final_latent, seeded_noiser, video_tools_for
    t = tiny
    ctx, nctx = t.ctx.to(dev), 20.0 * t.nctx.to(dev)          # a loud negative prompt: the tiny DiT hardly listens to a quiet one
    noise = torch.randn(1, 12, 128, generator=torch.Generator().manual_seed(5)).to(dev)
    kw = dict(height=64, width=96, num_frames=9, num_inference_steps=4, cfg_scale=3.0, rescale_scale=0.0, fps=24.0)
    pipe = OneStagePipeline(t.m, None, None)
    guider = LtxAPGGuider(3.0, 0.5, 5.0)
    out, _ = pipe(ctx, nctx, OneStageCFGConfig(use_hip_graph=True, **kw), guider_override=guider, initial_noise=noise)
    cfg, _ = pipe(ctx, nctx, OneStageCFGConfig(use_hip_graph=True, **kw), initial_noise=noise)
    assert out.shape == (1, 128, 2, 2, 3) and bool(torch.isfinite(out).all()) and not torch.equal(out, cfg)
    tools = video_tools_for(VideoLatentPatchifier(patch_size=1), 9, 64, 96, 24.0)
    state = seeded_noiser(dev, 42)(conditioned_initial_state(tools, [], torch.float32, dev), noise_scale=1.0, noise=noise)
    sig = LTX2Scheduler().execute(steps=4)
    hand = projected_denoise_loop(X0Model(t.m), state, sig, ctx, nctx, guider, EulerDiffusionStep(), None, True)
    assert torch.equal(out, final_latent(tools, hand))
    seen = []
    eager, _ = pipe(ctx, nctx, OneStageCFGConfig(use_hip_graph=True, **kw), guider_override=guider, initial_noise=noise, callback=lambda i, n: seen.append(i))
    assert torch.equal(eager, out) and seen == [1, 2, 3, 4]
    with pytest.raises(NotImplementedError, match="guider_override"):
        pipe(ctx, nctx, OneStageCFGConfig(**kw), guider_override=object(), initial_noise=noise)


def test_retake_pipeline_with_a_guider(dev, parts):
    """RetakePipeline(..., guider=LtxAPGGuider) == projected_denoise_loop by hand on the hand-built state, bit for bit; not the CFG run."""
    from ltx_2_mlx_amd.components import EulerDiffusionStep, LTX2Scheduler, LtxAPGGuider
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import RetakePipeline, projected_denoise_loop
    pipe = RetakePipeline(parts.m, parts.enc, None)
    ctx, nctx, noise = parts.ctx.to(dev), 20.0 * parts.nctx.to(dev), parts.noise.to(dev)
    conf = _conf(num_inference_steps=4, cfg_scale=3.0)
    guider = LtxAPGGuider(3.0, 0.5, 5.0)
    out = pipe(None, ctx, None, conf, negative_text_encoding=nctx, frames=parts.source, initial_noise=noise, guider=guider)
    plain = pipe(None, ctx, None, conf, negative_text_encoding=nctx, frames=parts.source, initial_noise=noise)
    assert out.shape == (1, 128, 3, 2, 3) and bool(torch.isfinite(out).all()) and not torch.equal(out, plain)
    tools, _, state = _hand_state(parts, dev)
    hand = projected_denoise_loop(X0Model(parts.m), state, LTX2Scheduler().execute(steps=4), ctx, nctx, guider, EulerDiffusionStep(), None, conf.use_hip_graph)
    assert torch.equal(_bits(out), _bits(tools.unpatchify(tools.clear_conditioning(hand)).latent))


def test_joint_audio_video_call_with_a_guider_override(dev):
    """The joint AudioVideo call with an override == the eager joint_denoise_loop given the same two guiders, bit for bit (the override is
    the video guider, audio keeps CFG*)."""
    from ltx_2_mlx_amd.components import AudioPatchifier, CFGStarRescalingGuider, EulerDiffusionStep, LTX2Scheduler, LegacyStatefulAPGGuider, VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning.tools import AudioLatentTools
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline, joint_denoise_loop
    from ltx_2_mlx_amd.pipelines.common import conditioned_initial_state, final_latent, seeded_noiser, video_tools_for
    from ltx_2_mlx_amd.types import AudioLatentShape, VideoPixelShape
    cfg, _, _, m = make_av(dev, False, seed=23)
    g = torch.Generator().manual_seed(31)
    S = 24
    ashape = AudioLatentShape.from_video_pixel_shape(VideoPixelShape(batch=1, frames=9, height=64, width=96, fps=25.0), channels=8, mel_bins=16, sample_rate=16000,
                                                     hop_length=160, audio_latent_downsample_factor=4)
    noise, anoise = torch.randn(1, 12, 128, generator=g).to(dev), torch.randn(1, ashape.frames, 128, generator=g).to(dev)
    vctx, actx, nvctx, nactx = (0.1 * torch.randn(1, S, cfg.caption_channels, generator=g).to(dev) for _ in range(4))
    kw = dict(height=64, width=96, num_frames=9, num_inference_steps=3, cfg_scale=3.0, audio_cfg_scale=7.0, rescale_scale=0.7, fps=25.0, audio_enabled=True)
    guider = LegacyStatefulAPGGuider(2.0, 0.5, 5.0, 0.5)
    pipe = OneStagePipeline(m, None, None)
    call = lambda: pipe(vctx, nvctx, OneStageCFGConfig(**kw), positive_audio_encoding=actx, negative_audio_encoding=nactx, guider_override=guider,
                        initial_noise=noise, initial_audio_noise=anoise)
    lat, aud = call()
    lat2, aud2 = call()                                       # the running state does not leak from one call into the next
    assert torch.equal(lat, lat2) and torch.equal(aud, aud2)
    tools = video_tools_for(VideoLatentPatchifier(patch_size=1), 9, 64, 96, 25.0)
    noiser = seeded_noiser(dev, 42)
    vstate = noiser(conditioned_initial_state(tools, [], torch.float32, dev), noise_scale=1.0, noise=noise)
    atools = AudioLatentTools(patchifier=AudioPatchifier(patch_size=1), target_shape=ashape)
    astate = noiser(atools.create_initial_state(dtype=torch.float32, device=dev), noise_scale=1.0, noise=anoise)
    guider.reset()
    hv, ha = joint_denoise_loop(X0Model(m), True, vstate, astate, LTX2Scheduler().execute(steps=3), vctx, actx, EulerDiffusionStep(), None, False,
                                negative_video_context=nvctx, negative_audio_context=nactx, video_guider=guider, audio_guider=CFGStarRescalingGuider(7.0))
    assert torch.equal(lat, final_latent(tools, hv)) and torch.equal(aud, final_latent(atools, ha))
    std, _ = pipe(vctx, nvctx, OneStageCFGConfig(**kw), positive_audio_encoding=actx, negative_audio_encoding=nactx, initial_noise=noise, initial_audio_noise=anoise)
    assert not torch.equal(std, lat)
