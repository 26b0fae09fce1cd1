"""The joint audio+video guided step with a guider per modality on the GPU: both pair kernels against the single-launch kernels bit for bit,
the one-call step against its parts and its captured graph against the per-step calls bit for bit, and OneStagePipeline's loop against the
eager loop and the fp32 restatement (OneStagePipeline keeps the eager loop: the device form measured no faster).  The tiny AudioVideo model of tests/test_projected_guidance_gpu.py (make_av seed 23; 64 x 96, 9 frames:
12 video and 9 audio tokens)."""
import pytest
import torch

from conftest import measure, rel_l2

import joint_projected_ref as JR
from test_parity import make_av, pearson

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
SIGMA, SIGMA_NEXT = 0.909375, 0.725


# ------------------------------------------------------------------ 1. the pair kernels
def _single(K, d, mode, first, masked, per_row):
    """One segment through the single-launch kernels -> (out, scalars, running after, partials); a field the mode does not have is None."""
    ts = d["ts_row"] if per_row else d["ts_one"]
    a, b = d["x"] - ts.reshape(-1, 1) * d["vc"], d["x"] - ts.reshape(-1, 1) * d["vu"]
    g, _ = JR.segment_guider(mode, float((a - b).double().norm()))
    mk, cl = (d["mask"], d["clean"]) if masked else (None, None)
    sc = torch.full((2,), SENTINEL, device=d["x"].device)
    if g["mode"] >= 3:       # no sums: CFGGuider's step; not guided: the same step at scale 1, a + 0*(a - b) = a
        out = K.guided_euler_step(d["x"], d["vc"], d["vu"], ts, g["scale"], SIGMA, SIGMA_NEXT, mask=mk, clean=cl)
        return g, out, sc, None, None
    run = None
    if g.get("momentum"):
        run = torch.full_like(d["x"], 7.0) if first else d["running"].clone()          # the first step must not read it
    part = K.guidance_sums(d["x"], d["vc"], d["vu"], ts, running=run, first=first, momentum=g.get("momentum", 0.0))
    out = K.projected_euler_step(d["x"], d["vc"], d["vu"], ts, part, g["mode"], g["scale"], g["eta"], g["norm_threshold"], SIGMA, SIGMA_NEXT, mask=mk,
                                 clean=cl, running=run, scalars_out=sc)
    return g, out, sc, run, part


@pytest.mark.parametrize("v_rows,a_rows,C", JR.SHAPES)
def test_pair_equals_single_launches_bit_for_bit(dev, v_rows, a_rows, C):
    """Every pairing of segment modes {off, CFG, CFG*, APG, APG + momentum} x first / continuing x mask on either side x scalar / per-row
    timesteps: out, scalars_out, running and partials of each segment of ONE pair launch equal the single-launch kernels' bit for bit."""
    from ltx_2_mlx_amd import kernels as K
    blocks = (K.guidance_sums_blocks(v_rows, C), K.guidance_sums_blocks(a_rows, C))
    if (v_rows, a_rows, C) == (37, 5, 128):
        assert blocks[0] > 1 and blocks[1] == 1                  # one segment with several partial rows, the other with exactly one
    if v_rows == 96:
        assert blocks[0] > 1 and blocks[1] > 1
    segs = []
    for rows, seed in ((v_rows, 0), (a_rows, 1)):
        d = {k: v.to(dev) for k, v in JR.inputs(rows, C, seed).items()}
        d["ts_one"] = torch.tensor([SIGMA], device=dev)
        segs.append(d)
    singles = {}

    def single(k, *key):
        if (k, *key) not in singles:
            singles[(k, *key)] = _single(K, segs[k], *key)
        return singles[(k, *key)]

    n = 0
    for first in (True, False):
        for v_masked, a_masked in ((False, False), (True, False), (False, True), (True, True)):
            for v_row, a_row in ((False, False), (True, True), (True, False), (False, True)):
                for v_mode in JR.SEGMENT_MODES:
                    for a_mode in JR.SEGMENT_MODES:
                        want = (single(0, v_mode, first, v_masked, v_row), single(1, a_mode, first, a_masked, a_row))
                        sums, step, got = [], [], []
                        for d, (g, _, _, run, part), masked, per_row in ((segs[0], want[0], v_masked, v_row), (segs[1], want[1], a_masked, a_row)):
                            ts = d["ts_row"] if per_row else d["ts_one"]
                            r = None if run is None else (torch.full_like(d["x"], 7.0) if first else d["running"].clone())
                            p = None if part is None else torch.full_like(part, float("nan"))
                            sc = torch.full((2,), SENTINEL, device=dev)
                            sums.append(None if part is None else dict(x=d["x"], vel_cond=d["vc"], vel_uncond=d["vu"], timesteps=ts, partials=p, running=r,
                                                                       first=first, momentum=g.get("momentum", 0.0)))
                            step.append(dict(x=d["x"], vel_cond=d["vc"], vel_uncond=d["vu"], timesteps=ts, partials=p, running=r, scalars_out=sc,
                                             mask=d["mask"] if masked else None, clean=d["clean"] if masked else None, **{k: v for k, v in g.items() if k != "momentum"}))
                            got.append((r, p, sc))
                        if sums[0] is not None or sums[1] is not None:
                            K.guidance_sums_pair(sums[0], sums[1])
                        outs = K.projected_euler_step_pair(step[0], step[1], SIGMA, SIGMA_NEXT)
                        for k in range(2):
                            tag = f"segment {k}: {v_mode} | {a_mode} first={first} masks={v_masked, a_masked} per_row={v_row, a_row}"
                            _, w_out, w_sc, w_run, w_part = want[k]
                            r, p, sc = got[k]
                            assert torch.equal(outs[k], w_out), f"{tag}: out differs in {int((outs[k] != w_out).sum())} elements"
                            assert torch.equal(sc, w_sc), f"{tag}: scalars {sc.tolist()} != {w_sc.tolist()}"
                            assert (r is None) == (w_run is None) and (r is None or torch.equal(r, w_run)), f"{tag}: running"
                            assert (p is None) == (w_part is None) and (p is None or torch.equal(p, w_part)), f"{tag}: partials"
                        n += 1
    assert n == 2 * 4 * 4 * 25
    for k in range(2):       # the references are what they claim: every mode another result, all finite (no mask: a row at mask 0 is its clean latent under every guider)
        outs = [single(k, mode, True, False, True)[1] for mode in JR.SEGMENT_MODES]
        assert all(bool(torch.isfinite(o).all()) for o in outs)
        assert all(not torch.equal(outs[i], outs[j]) for i in range(5) for j in range(i))


def test_pair_refusals(dev):
    from ltx_2_mlx_amd import kernels as K
    d = {k: v.to(dev) for k, v in JR.inputs(5, 128).items()}
    part = K.guidance_sums(d["x"], d["vc"], d["vu"], d["ts_row"])
    seg = lambda **kw: dict(dict(x=d["x"], vel_cond=d["vc"], vel_uncond=d["vu"], timesteps=d["ts_row"], partials=part, mode=0, scale=3.0), **kw)      # noqa: E731
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        K.projected_euler_step_pair(seg(), seg(), 0.0, 0.5)
    with pytest.raises(ValueError, match="audio mode=5"):
        K.projected_euler_step_pair(seg(), seg(mode=5), SIGMA, SIGMA_NEXT)
    with pytest.raises(ValueError, match="running"):
        K.projected_euler_step_pair(seg(mode=3, running=torch.zeros_like(d["x"])), seg(), SIGMA, SIGMA_NEXT)
    with pytest.raises(ValueError, match="reads partials"):
        K.projected_euler_step_pair(seg(partials=None), seg(), SIGMA, SIGMA_NEXT)
    with pytest.raises(ValueError, match="both partials are NULL"):
        K.guidance_sums_pair(None, None)
    with pytest.raises(ValueError, match="mode=3"):              # the single entry keeps its three modes
        K.projected_euler_step(d["x"], d["vc"], d["vu"], d["ts_row"], part, 3, 3.0, 1.0, 0.0, SIGMA, SIGMA_NEXT)


# ------------------------------------------------------------------ the tiny AudioVideo model
F, H, W, S = 2, 2, 3, 24
N = F * H * W
KW = dict(height=64, width=96, num_frames=9, num_inference_steps=3, cfg_scale=3.0, audio_cfg_scale=7.0, rescale_scale=0.7, fps=25.0, audio_enabled=True)


class Tiny:
    pass


@pytest.fixture(scope="module")
def tiny(dev):
    from oracle import dit_av, loop
    from ltx_2_mlx_amd.components import LTX2Scheduler
    from ltx_2_mlx_amd.types import AudioLatentShape, VideoPixelShape
    t = Tiny()
    t.cfg, _, t.wq, t.m = make_av(dev, False, seed=23)
    t.ashape = AudioLatentShape.from_video_pixel_shape(VideoPixelShape(batch=1, frames=9, height=64, width=96, fps=25.0), channels=8, mel_bins=16,
                                                       sample_rate=16000, hop_length=160, audio_latent_downsample_factor=4)
    t.na = t.ashape.frames
    g = torch.Generator().manual_seed(31)
    t.vnoise, t.anoise = torch.randn(1, N, 128, generator=g), torch.randn(1, t.na, 128, generator=g)
    t.vctx, t.actx = (0.1 * torch.randn(1, S, t.cfg.caption_channels, generator=g) for _ in range(2))
    t.nvctx, t.nactx = (2.0 * torch.randn(1, S, t.cfg.caption_channels, generator=g) for _ in range(2))       # a loud negative prompt: the tiny DiT hardly listens to a quiet one
    t.vclean = torch.randn(1, N, 128, generator=g)
    t.vpos, t.apos = loop.video_positions(1, F, H, W, 25.0), dit_av.audio_positions(1, t.na)
    t.vmask = torch.ones(1, N, 1)
    t.vmask[:, :H * W] = 0.05                                # the first latent frame conditioned on an image at strength 0.95
    t.sig = [float(s) for s in LTX2Scheduler().execute(steps=3)]
    t.ctx = tuple(c.to(dev) for c in (t.vctx, t.actx, t.nvctx, t.nactx))
    return t


def _states(t, dev, masked):
    """(video state, audio state): pure noise, or with masked the first video frame at its image-conditioning mask over the clean latent."""
    from ltx_2_mlx_amd.types import LatentState
    vm = t.vmask if masked else torch.ones_like(t.vmask)
    vlat = t.vnoise * vm + t.vclean * (1 - vm)
    video = LatentState(latent=vlat.to(dev), denoise_mask=vm.to(dev), positions=t.vpos.to(dev), clean_latent=t.vclean.clone().to(dev))
    audio = LatentState(latent=t.anoise.to(dev), denoise_mask=torch.ones(1, t.na, 1, device=dev), positions=t.apos.to(dev), clean_latent=t.anoise.clone().to(dev))
    return video, audio


PAIRS = [("cfg_star", "cfg_star"), ("apg_momentum", "cfg_star"), ("cfg", "off"), ("apg", "cfg")]


# ------------------------------------------------------------------ 2. the engine step and its graph
@pytest.mark.parametrize("masked", [False, True], ids=["uniform", "image-mask"])
@pytest.mark.parametrize("modes", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_projected_step_joint_av_equals_its_parts(dev, tiny, modes, masked):
    """projected_step_joint_av_ == forward_av(ctx), forward_av(neg), ltx2_guidance_sums_pair, ltx2_projected_euler_step_pair called one by
    one: the same kernels in the same order, so the same bits on both latents; two steps, so that a running buffer is read."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.pipelines.common import audio_modality_from_state, modality_from_state
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    vctx, actx, nvctx, nactx = t.ctx
    vs, as_ = _states(t, dev, masked)
    gs = [JR.segment_guider(mode)[0] for mode in modes]
    want = [vs.latent[0].float().contiguous(), as_.latent[0].float().contiguous()]
    got = [w.clone() for w in want]
    run = [torch.zeros_like(w) if g.get("momentum") else None for g, w in zip(gs, want)]
    run_got = [None if r is None else torch.full_like(r, 7.0) for r in run]
    mk = vs.denoise_mask[0].reshape(-1).contiguous() if masked else None
    cl = vs.clean_latent[0].contiguous() if masked else None
    for step, (s, sn) in enumerate(((t.sig[0], t.sig[1]), (t.sig[1], t.sig[2]))):
        mods = lambda lats, vc, ac: (modality_from_state(vs.replace(latent=lats[0][None]), vc, s, uniform=not masked),      # noqa: E731
                                     audio_modality_from_state(as_.replace(latent=lats[1][None]), ac, s, uniform=True))
        cond, unc = m(*mods(want, vctx, actx)), neg(*mods(want, nvctx, nactx))
        segs = []
        for k in range(2):
            ts = (mk * s) if (masked and k == 0) else torch.tensor([s], device=dev)
            part = torch.empty(K.guidance_sums_blocks(*want[k].shape), 5, device=dev, dtype=torch.float64) if gs[k]["mode"] < 3 else None
            segs.append(dict(x=want[k], vel_cond=cond[k][0].clone(), vel_uncond=unc[k][0].clone(), timesteps=ts, partials=part, running=run[k],
                             mask=mk if k == 0 else None, clean=cl if k == 0 else None, first=(step == 0), **gs[k]))
        sums = [None if sg["partials"] is None else {k: v for k, v in sg.items() if k in ("x", "vel_cond", "vel_uncond", "timesteps", "partials", "running", "first", "momentum")}
                for sg in segs]
        if sums[0] is not None or sums[1] is not None:
            K.guidance_sums_pair(*sums)
        want = list(K.projected_euler_step_pair(*({k: v for k, v in sg.items() if k not in ("first", "momentum")} for sg in segs), s, sn))
        m.projected_step_joint_av_(neg, got[0], got[1], *mods(got, vctx, actx), s, sn, gs[0], gs[1], first=(step == 0), running=run_got[0],
                                   audio_running=run_got[1], denoise_mask=mk, clean_latent=cl)
        torch.cuda.synchronize()
        for k in range(2):
            assert torch.equal(got[k], want[k]), f"{modes} masked={masked} step {step} modality {k}: {int((got[k] != want[k]).sum())} elements differ"
            assert run[k] is None or torch.equal(run_got[k], run[k])
    assert all(bool(torch.isfinite(g).all()) for g in got) and not torch.equal(got[0], vs.latent[0]) and not torch.equal(got[1], as_.latent[0])
    if masked:
        with pytest.raises(ValueError, match="mask and clean go together"):
            m.projected_step_joint_av_(neg, got[0], got[1], *mods(got, vctx, actx), 0.5, 0.25, gs[0], gs[1], running=run_got[0], denoise_mask=mk)
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        m.projected_step_joint_av_(neg, got[0], got[1], *mods(got, vctx, actx), 0.0, 0.5, gs[0], gs[1], running=run_got[0], denoise_mask=mk, clean_latent=cl)
    with pytest.raises(ValueError, match="running buffer"):
        m.projected_step_joint_av_(neg, got[0], got[1], *mods(got, vctx, actx), 0.5, 0.25, gs[0], gs[1], running=None if run_got[0] is not None else torch.zeros_like(got[0]),
                                   denoise_mask=mk, clean_latent=cl)


def _guider(mode):
    return JR.segment_guider(mode)[1]


@pytest.mark.parametrize("masked", [False, True], ids=["uniform", "image-mask"])
@pytest.mark.parametrize("modes", PAIRS[:2], ids=["+".join(p) for p in PAIRS[:2]])
def test_joint_projected_graph_equals_per_step_calls(dev, tiny, modes, masked):
    """3 steps: the captured graph, the per-step C calls and the per-step calls with a callback give the same bits on both latents; a second
    run of the loop (a fresh capture; with momentum the running guidance starts cleared) repeats them."""
    from ltx_2_mlx_amd.components import EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import joint_projected_denoise_loop
    t = tiny
    x0m = X0Model(t.m)

    def run(graph, callback=None):
        v, a = joint_projected_denoise_loop(x0m, *_states(t, dev, masked), t.sig, *t.ctx, _guider(modes[0]), _guider(modes[1]), EulerDiffusionStep(), callback, graph)
        torch.cuda.synchronize()
        return v.latent, a.latent

    seen = []
    graph, eager, again = run(True), run(False), run(True)
    cb = run(True, callback=lambda i, n: seen.append((i, n)))
    for k in range(2):
        assert torch.equal(graph[k], eager[k]), f"modality {k}: {int((graph[k] != eager[k]).sum())} elements differ"
        assert torch.equal(cb[k], eager[k]) and torch.equal(again[k], graph[k]) and bool(torch.isfinite(graph[k]).all())
    assert seen == [(1, 3), (2, 3), (3, 3)]
    vs, as_ = _states(t, dev, masked)
    assert not torch.equal(graph[0], vs.latent) and not torch.equal(graph[1], as_.latent)


def test_joint_projected_loop_hands_over(dev, tiny):
    """Neither guider enabled, or a negative context missing: joint_denoise_loop's run, bit for bit."""
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider, EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import joint_denoise_loop, joint_projected_denoise_loop
    t = tiny
    x0m, st = X0Model(t.m), EulerDiffusionStep()
    plain = joint_denoise_loop(x0m, True, *_states(t, dev, False), t.sig, t.ctx[0], t.ctx[1], st, None, True)
    for guiders, ctx in (((CFGStarRescalingGuider(1.0), CFGGuider(1.0)), t.ctx), ((None, None), t.ctx)):
        v, a = joint_projected_denoise_loop(x0m, *_states(t, dev, False), t.sig, *ctx, *guiders, st, None, True)
        assert torch.equal(v.latent, plain[0].latent) and torch.equal(a.latent, plain[1].latent)
    with pytest.raises(ValueError, match="negative prompt"):      # guiders enabled, no negative context: joint_denoise_loop's own refusal
        joint_projected_denoise_loop(x0m, *_states(t, dev, False), t.sig, t.ctx[0], t.ctx[1], None, t.ctx[3], CFGStarRescalingGuider(3.0), CFGStarRescalingGuider(7.0), st)


# ------------------------------------------------------------------ 3. the pipeline's loop
# rel-L2 of the device loop against the eager loop (two X0Model calls, the guiders in torch with fp32 reductions), measured on the MI355X; the
# gate sits at 5 x these
MEASURED = {"default": {"video": 1.1472e-7, "audio": 6.8598e-7}, "apg_override": {"video": 1.3137e-4, "audio": 1.8751e-4}}


@pytest.fixture(scope="module")
def loop_refs(tiny):
    """The fp32 restatement of both runs (oracle.dit_av.av_x0_model inside joint_projected_ref.guided_loop_av), computed once."""
    from oracle import dit_av
    from ltx_2_mlx_amd.components import CFGStarRescalingGuider, LtxAPGGuider
    t = tiny

    def x0(vc, ac):
        def f(v, vts, a, ats, s):
            sg = torch.tensor([s])
            return dit_av.av_x0_model(dict(latent=v, context=vc, timesteps=sg, sigma=sg, positions=t.vpos),
                                      dict(latent=a, context=ac, timesteps=sg, sigma=sg, positions=t.apos), t.wq, t.cfg)
        return f
    ones = (torch.ones(1, N, 1), torch.ones(1, t.na, 1))
    video, audio = (t.vnoise, ones[0], t.vnoise), (t.anoise, ones[1], t.anoise)
    guiders = dict(default=(CFGStarRescalingGuider(3.0), CFGStarRescalingGuider(7.0)), apg_override=(LtxAPGGuider(3.0, 0.5, 5.0), CFGStarRescalingGuider(7.0)))
    return {k: JR.guided_loop_av(video, audio, x0(t.vctx, t.actx), x0(t.nvctx, t.nactx), t.sig, *g) for k, g in guiders.items()}


@pytest.mark.parametrize("which", ["default", "apg_override"])
def test_joint_projected_loop_against_eager_and_restatement(dev, tiny, loop_refs, which, capfd, monkeypatch):
    """OneStagePipeline's states at cfg 3 / audio cfg 7 / rescale 0.7, 3 steps (which = apg_override: LtxAPGGuider(3, 0.5, 5) on the video, the
    audio on CFG*) through joint_projected_denoise_loop with use_hip_graph=True: against the eager joint_denoise_loop with the same guiders
    within 5 x the measured rel-L2 (the device sums are fp64, the torch guiders' fp32); against the fp32 restatement at most 1.5 x as far as
    that eager loop, Pearson > 0.999 (the gate of test_projected_guidance_gpu's loop); nothing says that the graph was skipped.  The pipeline
    itself keeps the eager loop (the device form measured no faster, profiles/joint_projected_step.md): its result is the eager loop's, bit for
    bit, with use_hip_graph or without.  Measured on the MI355X, video / audio: default vs eager 1.1472e-07 / 6.8598e-07, E0 = E1 = 1.8970e-03 /
    3.1036e-03; apg_override vs eager 1.3137e-04 / 1.8751e-04, E0 1.9057e-03 / 3.1263e-03, E1 1.9085e-03 / 3.1164e-03; Pearson 0.999995 or better."""
    from ltx_2_mlx_amd.components import AudioPatchifier, CFGStarRescalingGuider, EulerDiffusionStep, LtxAPGGuider, VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning.tools import AudioLatentTools
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline, common, joint_denoise_loop, joint_projected_denoise_loop
    from ltx_2_mlx_amd.pipelines.common import conditioned_initial_state, final_latent, seeded_noiser, video_tools_for
    t = tiny
    vctx, actx, nvctx, nactx = t.ctx
    monkeypatch.setattr(common, "_eager_noted", set())         # the note is printed once per process: let this run print it if it were due
    override = LtxAPGGuider(3.0, 0.5, 5.0) if which == "apg_override" else None
    pipe = OneStagePipeline(t.m, None, None)
    tools = video_tools_for(VideoLatentPatchifier(patch_size=1), 9, 64, 96, 25.0)
    atools = AudioLatentTools(patchifier=AudioPatchifier(patch_size=1), target_shape=t.ashape)

    def states():
        noiser = seeded_noiser(dev, 42)
        return (noiser(conditioned_initial_state(tools, [], torch.float32, dev), noise_scale=1.0, noise=t.vnoise.to(dev)),
                noiser(atools.create_initial_state(dtype=torch.float32, device=dev), noise_scale=1.0, noise=t.anoise.to(dev)))

    guiders = lambda: (LtxAPGGuider(3.0, 0.5, 5.0) if override else CFGStarRescalingGuider(3.0), CFGStarRescalingGuider(7.0))      # noqa: E731
    capfd.readouterr()
    hv, ha = joint_projected_denoise_loop(X0Model(t.m), *states(), t.sig, vctx, actx, nvctx, nactx, *guiders(), EulerDiffusionStep(), None, True)
    torch.cuda.synchronize()
    assert "hipGraph replay skipped" not in capfd.readouterr().err
    gv, ga = guiders()
    ev, ea = joint_denoise_loop(X0Model(t.m), True, *states(), t.sig, vctx, actx, EulerDiffusionStep(), None, False, negative_video_context=nvctx,
                                negative_audio_context=nactx, video_guider=gv, audio_guider=ga)
    new = (hv.latent.cpu(), ha.latent.cpu())
    old = (ev.latent.cpu(), ea.latent.cpu())
    for k, name in enumerate(("video", "audio")):
        d = measure(f"joint projected loop vs eager loop, {which} {name}", rel_l2(new[k], old[k]))
        e0 = measure(f"E0 eager joint loop vs fp32, {which} {name}", rel_l2(old[k], loop_refs[which][k]))
        e1 = measure(f"E1 joint projected loop vs fp32, {which} {name}", rel_l2(new[k], loop_refs[which][k]))
        print(f"joint projected loop, {which} {name}: vs eager = {d:.4e}  E0 = {e0:.4e}  E1 = {e1:.4e}  pearson = {pearson(new[k], loop_refs[which][k]):.6f}")
    for k, name in enumerate(("video", "audio")):
        assert rel_l2(new[k], old[k]) <= 5 * MEASURED[which][name], name
        assert rel_l2(new[k], loop_refs[which][k]) <= 1.5 * rel_l2(old[k], loop_refs[which][k]) and pearson(new[k], loop_refs[which][k]) > 0.999, name
    assert rel_l2(new[0], t.vnoise) > 0.1 and rel_l2(new[1], t.anoise) > 0.1
    for graph in (True, False):                                   # the pipeline: the eager loop's result
        lat_e, aud_e = pipe(vctx, nvctx, OneStageCFGConfig(use_hip_graph=graph, **KW), positive_audio_encoding=actx, negative_audio_encoding=nactx,
                            initial_noise=t.vnoise.to(dev), initial_audio_noise=t.anoise.to(dev), **(dict(guider_override=override) if override else {}))
        assert torch.equal(lat_e, final_latent(tools, ev)) and torch.equal(aud_e, final_latent(atools, ea))
