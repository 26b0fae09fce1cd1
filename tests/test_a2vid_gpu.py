"""Audio-to-video on the GPU: the one-call guided step of the AudioVideo engine against its parts called one by one, its captured graph against
the per-step loop, the loop against the fp32 restatement (with the EXISTING eager guidance as the yardstick), the argument checks, the
two-stage pipeline and generate_video.  The smallest AudioVideo models of tests/test_parity.py (4 heads, 2 layers), LTX-2.0 and LTX-2.3
form, at 64x96x9: 12 video tokens, 9 audio tokens, S = 24, 4 steps."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

from conftest import measure, rel_l2

import a2vid_ref as R
from test_parity import make_av, make_vae, pearson

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, H, W, NA, S = 2, 2, 3, 9, 24
N = F * H * W
SCALE = 3.0


class Tiny:
    pass


@pytest.fixture(scope="module", params=[False, True], ids=["v20", "v23"])
def tiny(dev, request):
    from oracle import dit_av, loop
    from ltx_2_mlx_amd.components import LTX2Scheduler
    t = Tiny()
    t.v23 = request.param
    t.cfg, _, t.wq, t.m = make_av(dev, t.v23, seed=41 + t.v23)
    g = torch.Generator().manual_seed(977)
    cv, ca = t.cfg.caption_channels or t.cfg.inner_dim, t.cfg.caption_channels or t.cfg.audio_inner_dim
    t.vctx, t.nvctx = (0.1 * torch.randn(1, S, cv, generator=g) for _ in range(2))
    t.actx, t.nactx = (0.1 * torch.randn(1, S, ca, generator=g) for _ in range(2))
    t.lat = torch.randn(1, N, 128, generator=g)
    t.audio, t.audio2 = (torch.randn(1, NA, 128, generator=g) for _ in range(2))
    t.vpos, t.apos = loop.video_positions(1, F, H, W, 25.0), dit_av.audio_positions(1, NA)
    # frame 0 conditioned at strength 1: its 6 tokens carry mask 0 and a clean latent
    t.mask = torch.ones(1, N, 1)
    t.mask[:, :6] = 0.0
    t.clean = torch.zeros(1, N, 128)
    t.clean[:, :6] = torch.randn(1, 6, 128, generator=g)
    t.sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    return t


def _states(t, dev, cond, audio=None):
    from ltx_2_mlx_amd.types import LatentState
    mask = t.mask if cond else torch.ones(1, N, 1)
    lat = torch.where(mask == 0, t.clean, t.lat) if cond else t.lat
    video = LatentState(latent=lat.clone().to(dev), denoise_mask=mask.to(dev), positions=t.vpos.to(dev), clean_latent=(t.clean if cond else lat).clone().to(dev))
    a = (t.audio if audio is None else audio).to(dev)
    return video, LatentState(latent=a.clone(), denoise_mask=torch.zeros(1, NA, 1, device=dev), positions=t.apos.to(dev), clean_latent=a.clone())


def _ctx(t, dev):
    if not hasattr(t, "dev_ctx"):
        t.dev_ctx = tuple(c.to(dev) for c in (t.vctx, t.actx, t.nvctx, t.nactx))
    return t.dev_ctx


# ------------------------------------------------------------------ 1. the engine step
@pytest.mark.parametrize("cond", [False, True], ids=["uniform", "frame0"])
def test_guided_step_av_equals_its_parts(dev, tiny, cond):
    """guided_step_av_ == ltx2_dit_forward_av(ctx), ltx2_dit_forward_av(neg), ltx2_guided_euler_step called separately: the same kernels in the
    same order on the same streams, so the same bits on the video latent; the audio latent tensor keeps its bits."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.pipelines.common import audio_modality_from_state, modality_from_state
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    sigma, sigma_next = t.sig[1], t.sig[2]
    vs, as_ = _states(t, dev, cond)
    mods = lambda vc, ac: (modality_from_state(vs, vc, sigma, uniform=not cond), audio_modality_from_state(as_, ac, sigma))          # noqa: E731
    vc = m(*mods(vctx, actx))[0][0].clone()
    vu = neg(*mods(nvctx, nactx))[0][0].clone()
    assert float((vc - vu).abs().max()) > 1e-3                                  # two prompts, two velocities
    lat = vs.latent[0].float().contiguous()
    mk, cl = (vs.denoise_mask[0].reshape(-1).contiguous(), vs.clean_latent[0].contiguous()) if cond else (None, None)
    ts = (vs.denoise_mask * sigma).reshape(-1) if cond else torch.tensor([sigma], device=dev)
    want = K.guided_euler_step(lat, vc, vu, ts, SCALE, sigma, sigma_next, mask=mk, clean=cl)
    got, alat = lat.clone(), as_.latent[0].float().contiguous()
    m.guided_step_av_(neg, got, alat, *mods(vctx, actx), sigma, sigma_next, SCALE, denoise_mask=mk, clean_latent=cl)
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"{int((got != want).sum())} elements differ"
    assert torch.equal(alat.cpu(), t.audio[0]) and bool(torch.isfinite(got).all()) and not torch.equal(got, lat)
    if cond:
        assert rel_l2(got[:6].cpu(), t.clean[0, :6]) < 1e-5                    # the conditioned tokens stay at their clean values


# ------------------------------------------------------------------ 2. graph, eager, callback
@pytest.mark.parametrize("cond", [False, True], ids=["uniform", "frame0"])
def test_guided_loop_graph_equals_eager(dev, tiny, cond):
    from ltx_2_mlx_amd.components import EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import frozen_audio_guided_loop
    t = tiny
    x0m = X0Model(t.m)
    ctx = _ctx(t, dev)

    def run(graph, audio=None, callback=None):
        vs, as_ = _states(t, dev, cond, audio)
        v, a = frozen_audio_guided_loop(x0m, vs, as_, t.sig, *ctx, SCALE, EulerDiffusionStep(), callback, graph)
        torch.cuda.synchronize()
        assert a is as_ and torch.equal(a.latent.cpu(), t.audio if audio is None else audio)     # the same object, the same bits
        return v.latent.cpu()

    seen = []
    graph, eager = run(True), run(False)
    cb = run(True, callback=lambda i, n: seen.append((i, n)))
    assert torch.equal(graph, eager), f"{int((graph != eager).sum())} elements differ"
    assert torch.equal(cb, eager) and seen == [(1, 4), (2, 4), (3, 4), (4, 4)]
    assert bool(torch.isfinite(graph).all()) and rel_l2(graph, t.lat) > 0.1
    other = run(True, audio=t.audio2)
    assert torch.equal(other, run(False, audio=t.audio2)) and not torch.equal(other, graph)      # the video listens to the audio
    tiny.loop_out = getattr(tiny, "loop_out", {})
    tiny.loop_out[cond] = graph


def test_one_graph_replayed_over_another_audio_latent(dev, tiny):
    """The captured graph reads the audio latent on every replay: new bytes in the same buffer, a restored video latent, a second launch."""
    from ltx_2_mlx_amd.components import EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import capture_and_replay, frozen_audio_guided_loop
    t, m = tiny, tiny.m
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    vs, as_ = _states(t, dev, False)
    neg = m.clone_sharing_weights()
    m.prepare(vctx, vs.positions, per_token=True, audio_context=actx, audio_positions=as_.positions)
    neg.prepare(nvctx, vs.positions, per_token=True, audio_context=nactx, audio_positions=as_.positions)
    lat, alat = vs.latent[0].clone(), as_.latent[0].clone()                      # stepped in place: not the state's own tensors
    amask = torch.zeros(NA, device=dev)
    capture_and_replay(lambda: m.capture_guided_av_graph(neg, lat, alat, t.sig, SCALE, audio_denoise_mask=amask), m.replay_guided_av_graph)
    torch.cuda.synchronize()
    first = lat.clone()
    lat.copy_(vs.latent[0])
    alat.copy_(t.audio2[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.replay_guided_av_graph()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(alat.cpu(), t.audio2[0]) and not torch.equal(lat, first)
    vs2, as2 = _states(t, dev, False, t.audio2)
    want = frozen_audio_guided_loop(X0Model(m), vs2, as2, t.sig, vctx, actx, nvctx, nactx, SCALE, EulerDiffusionStep(), None, False)[0].latent[0]
    assert torch.equal(lat, want)
    with pytest.raises(RuntimeError, match="no guided graph"):
        m.replay_guided_graph()                                                 # the capture is recorded under its own kind


def test_unguided_and_fallback_paths(dev, tiny):
    """cfg 1 or no negative context: joint_denoise_loop's frozen-audio path, unchanged.  negative_audio_context None: the positive one."""
    from ltx_2_mlx_amd.components import EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import frozen_audio_guided_loop, joint_denoise_loop
    t = tiny
    x0m = X0Model(t.m)
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    st = EulerDiffusionStep()
    for graph in (False, True):
        want = joint_denoise_loop(x0m, True, *_states(t, dev, True), t.sig, vctx, actx, st, None, graph)[0].latent
        for scale, nv in ((1.0, nvctx), (SCALE, None)):
            vs, as_ = _states(t, dev, True)
            v, a = frozen_audio_guided_loop(x0m, vs, as_, t.sig, vctx, actx, nv, nactx, scale, st, None, graph)
            assert torch.equal(v.latent, want) and a is as_
    a = frozen_audio_guided_loop(x0m, *_states(t, dev, False), t.sig, vctx, actx, nvctx, None, SCALE, st)[0].latent
    b = frozen_audio_guided_loop(x0m, *_states(t, dev, False), t.sig, vctx, actx, nvctx, actx, SCALE, st)[0].latent
    c = frozen_audio_guided_loop(x0m, *_states(t, dev, False), t.sig, vctx, actx, nvctx, nactx, SCALE, st)[0].latent
    assert torch.equal(a, b) and not torch.equal(a, c)


# ------------------------------------------------------------------ 3. against the fp32 restatement
@pytest.mark.parametrize("cond", [False, True], ids=["uniform", "frame0"])
def test_guided_loop_against_restatement(dev, tiny, cond):
    """Against the fp32 restatement of _video_only_denoise_loop (tests/a2vid_ref.py over oracle.dit_av) the new loop may be at most 1.5 x as far
    as the EXISTING eager path (joint_denoise_loop with CFGGuider(3) on the video, CFGGuider(1) on the audio and the frozen audio state): the
    two differ only in fp32 rounding order inside the step, the 1.5 allows for 16-bit rounding flips of the DiT's input.  Measured on the
    MI355X, E0 = E1 to four digits: 1.319e-03 / 9.278e-04 (LTX-2.0 form, uniform / frame 0), 1.519e-03 / 1.150e-03 (LTX-2.3 form)."""
    from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import frozen_audio_guided_loop, joint_denoise_loop
    t = tiny
    mask = t.mask if cond else torch.ones(1, N, 1)
    lat = torch.where(mask == 0, t.clean, t.lat) if cond else t.lat
    ref, raud = R.video_only_denoise_loop(lat, mask, t.clean if cond else lat, t.audio, t.sig, R.av_x0_video(t.wq, t.cfg, t.vpos, t.apos),
                                          t.vctx, t.actx, t.nvctx, t.nactx, SCALE)
    assert raud is t.audio
    x0m = X0Model(t.m)
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    new = frozen_audio_guided_loop(x0m, *_states(t, dev, cond), t.sig, vctx, actx, nvctx, nactx, SCALE, EulerDiffusionStep())[0].latent.cpu()
    vs, as_ = _states(t, dev, cond)
    old_v, old_a = joint_denoise_loop(x0m, True, vs, as_, t.sig, vctx, actx, EulerDiffusionStep(), use_hip_graph=False, negative_video_context=nvctx,
                                      negative_audio_context=nactx, video_guider=CFGGuider(SCALE), audio_guider=CFGGuider(1.0))
    assert rel_l2(old_a.latent.cpu(), t.audio) < 1e-6
    tag = f"{'v23' if t.v23 else 'v20'} {'frame0' if cond else 'uniform'}"
    e0 = measure(f"a2vid E0 existing eager guidance vs fp32 ({tag})", rel_l2(old_v.latent.cpu(), ref))
    e1 = measure(f"a2vid E1 frozen-audio guided loop vs fp32 ({tag})", rel_l2(new, ref))
    p = pearson(new, ref)
    print(f"a2vid guided loop {tag}: E0 = {e0:.4e}  E1 = {e1:.4e}  pearson = {p:.6f}")
    assert e1 <= 1.5 * e0 and p > 0.999


# ------------------------------------------------------------------ 4. argument checks (host side, nothing is launched)
def test_guided_step_av_refusals(dev, tiny):
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd.components import EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import LTXModel, X0Model
    from ltx_2_mlx_amd.pipelines.common import frozen_audio_guided_loop
    from oracle import dit_av, loop
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    vs, as_ = _states(t, dev, True)
    m.prepare(vctx, vs.positions, per_token=True, audio_context=actx, audio_positions=as_.positions)
    neg.prepare(nvctx, vs.positions, per_token=True, audio_context=nactx, audio_positions=as_.positions)
    lat, alat = vs.latent[0].float().contiguous(), as_.latent[0].float().contiguous()
    before = lat.clone()
    ts1, sg = torch.tensor([0.5], device=dev), torch.tensor([0.5], device=dev)
    tsn, atsn = torch.full((N,), 0.5, device=dev), torch.zeros(NA, device=dev)
    L = nv.lib()

    def step(a, b, ts=ts1, n_ts=1, ats=ts1, n_ats=1, sigma=0.5):
        nv.check(L.ltx2_dit_guided_step_av(a, b, nv.ptr(lat), nv.ptr(alat), nv.ptr(ts), n_ts, nv.ptr(ats), n_ats, nv.ptr(sg), None, None, SCALE,
                                           sigma, 0.25, nv.stream()))

    with pytest.raises(ValueError, match="ctx == neg"):
        step(m._h, m._h)
    twin = m._video_twin()
    for a, b in ((m._h, twin._h), (twin._h, m._h)):
        with pytest.raises(ValueError, match="must be AudioVideo"):
            step(a, b)
    fresh = make_av(dev, t.v23, seed=3)[3]                                        # never prepared
    with pytest.raises(ValueError, match="prepare"):
        step(m._h, fresh._h)
    for f, na, what in ((3, NA, "another N"), (F, NA + 1, "another Na")):
        fresh.prepare(nvctx, loop.video_positions(1, f, H, W, 25.0).to(dev), per_token=True, audio_context=nactx,
                      audio_positions=dit_av.audio_positions(1, na).to(dev))
        with pytest.raises(ValueError, match="contexts differ"):
            step(m._h, fresh._h)
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        step(m._h, neg._h, sigma=0.0)
    with pytest.raises(ValueError, match="must be 1 or N"):
        step(m._h, neg._h, ts=tsn, n_ts=N - 1)
    fresh.prepare(nvctx, vs.positions, per_token=False, audio_context=nactx, audio_positions=as_.positions)       # N and Na fit, no per-token buffers
    for kw in (dict(ts=tsn, n_ts=N), dict(ats=atsn, n_ats=NA)):
        with pytest.raises(ValueError, match="per-token"):
            step(m._h, fresh._h, **kw)
    mk, cl = vs.denoise_mask[0].reshape(-1).contiguous(), vs.clean_latent[0].contiguous()
    with torch.cuda.stream(torch.cuda.Stream()):
        with pytest.raises(ValueError, match="per-token"):
            m.capture_guided_av_graph(fresh, lat, alat, [1.0, 0.5, 0.0], SCALE, audio_denoise_mask=atsn)
        with pytest.raises(ValueError, match="tokens x"):
            m.capture_guided_av_graph(neg, lat, alat, [1.0, 0.5, 0.0], SCALE, denoise_mask=mk[:N - 2].contiguous(), clean_latent=cl, audio_denoise_mask=atsn)
        with pytest.raises(ValueError, match="tokens x"):
            m.capture_guided_av_graph(neg, lat, alat, [1.0, 0.5, 0.0], SCALE, audio_denoise_mask=torch.zeros(NA + 3, device=dev))
        with pytest.raises(ValueError, match="bad argument"):
            m.capture_guided_av_graph(neg, lat, alat, [1.0 - 0.01 * i for i in range(66)], SCALE)
    with pytest.raises(ValueError, match="AudioVideo contexts"):
        m.guided_step_av_(twin, lat, alat, None, None, 0.5, 0.25, SCALE)
    with pytest.raises(ValueError, match="second LTXModel"):
        m.guided_step_av_(None, lat, alat, None, None, 0.5, 0.25, SCALE)
    torch.cuda.synchronize()
    assert torch.equal(lat, before) and torch.equal(alat.cpu(), t.audio[0])          # nothing was launched
    as_bad = as_.replace(denoise_mask=torch.ones_like(as_.denoise_mask))
    with pytest.raises(ValueError, match="all zero"):
        frozen_audio_guided_loop(X0Model(m), vs, as_bad, t.sig, vctx, actx, nvctx, nactx, SCALE, EulerDiffusionStep())
    with pytest.raises(ValueError, match=r"requires an audio-video \(AV\) model"):
        frozen_audio_guided_loop(X0Model(twin), vs, as_, t.sig, vctx, actx, nvctx, nactx, SCALE, EulerDiffusionStep())


# ------------------------------------------------------------------ 5. the pipeline
@pytest.fixture(scope="module")
def parts(dev):
    from ltx_2_mlx_amd.model.upscaler import SpatialUpscaler
    p = Tiny()
    _, _, p.dec = make_vae(dev, layers=1)
    p.up = SpatialUpscaler(in_channels=128, mid_channels=64, num_blocks_per_stage=1, device=dev)
    p.up.init_random_weights(seed=3)
    return p


def _eager_parent_loop(transformer, video_state, audio_state, sigmas, vctx, actx, nvctx, nactx, cfg_scale, stepper, callback=None, use_hip_graph=True):
    """The parent's path to the same result: joint_denoise_loop's eager guidance (stage 1) and its eager frozen-audio loop (stage 2)."""
    from ltx_2_mlx_amd.components import CFGGuider
    from ltx_2_mlx_amd.pipelines.common import joint_denoise_loop
    guided = cfg_scale > 1.0 and nvctx is not None
    kw = dict(negative_video_context=nvctx, negative_audio_context=nactx, video_guider=CFGGuider(cfg_scale), audio_guider=CFGGuider(1.0)) if guided else {}
    v, _ = joint_denoise_loop(transformer, True, video_state, audio_state, sigmas, vctx, actx, stepper, None, False, **kw)
    return v, audio_state


def test_pipeline_two_stage(dev, tiny, parts, tmp_path, monkeypatch):
    """A2VidPipelineTwoStage at 128x192x9 (stage 1 at 64x96), 4 guided steps and the 3 refinement steps, audio_latent= supplied, fixed noises.
    The restatement's x2 upscale is the pipeline's own upscale_latent_x2 applied to the restatement's stage-1 latent (the upscaler is not
    what this feature adds)."""
    from safetensors.torch import save_file
    import ltx_2_mlx_amd.pipelines.a2vid_two_stage as A
    from ltx_2_mlx_amd.components import STAGE_2_DISTILLED_SIGMA_VALUES, EulerDiffusionStep, VideoLatentPatchifier
    from ltx_2_mlx_amd.loader.lora_loader import LoRAConfig
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import A2VidConfig, A2VidPipelineTwoStage, frozen_audio_guided_loop
    from ltx_2_mlx_amd.pipelines.common import upscale_latent_x2, video_tools_for
    from ltx_2_mlx_amd.types import LatentState
    t = tiny
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    g = torch.Generator().manual_seed(79)
    n1, n2 = torch.randn(1, N, 128, generator=g), torch.randn(1, 4 * N, 128, generator=g)
    alat = torch.randn(1, 8, NA, 16, generator=g)
    conf = A2VidConfig(height=128, width=192, num_frames=9, num_inference_steps=4, cfg_scale=SCALE)
    pipe = A2VidPipelineTwoStage(t.m, None, parts.dec, parts.up)
    kw = dict(positive_audio_encoding=actx, negative_audio_encoding=nactx, initial_noise=n1.to(dev), stage_2_noise=n2.to(dev))
    video, wav, rate = pipe(None, vctx, nvctx, conf, audio_latent=alat.to(dev), **kw)
    assert video.dtype == torch.uint8 and video.shape == (9, 128, 192, 3) and wav is None and rate is None
    assert pipe.token_counts == [N, 4 * N] and torch.equal(pipe.audio_latent.cpu(), alat)
    # stage 1 == the loop run by hand
    _, astate = pipe._frozen_audio_state(alat.to(dev), conf, dev)
    assert astate.latent.shape == (1, NA, 128) and not bool(astate.denoise_mask.any())
    stage1 = pipe.stage1_latent(astate, vctx, nvctx, conf, positive_audio_encoding=actx, negative_audio_encoding=nactx, initial_noise=n1.to(dev))
    tools = video_tools_for(VideoLatentPatchifier(patch_size=1), 9, 64, 96, 25.0)
    st = tools.create_initial_state(device=dev)
    st = st.replace(latent=n1.to(dev))                                          # noise at scale 1 over a zero latent with mask 1: the noise itself
    byhand = frozen_audio_guided_loop(X0Model(t.m), st, astate, t.sig, vctx, actx, nvctx, nactx, SCALE, EulerDiffusionStep())[0]
    assert torch.equal(stage1, tools.unpatchify(byhand).latent)
    # the final latent against the restatement's two-stage composition, E1 over E0 as in the loop test
    final = pipe.denoise_latent(alat.to(dev), vctx, nvctx, conf, **kw).cpu()
    assert final.shape == (1, 128, 2, 4, 6) and bool(torch.isfinite(final).all())
    atok = astate.latent.float().cpu()
    up = lambda lat: upscale_latent_x2(lat.to(dev), parts.up, None, parts.dec).cpu()          # noqa: E731
    _, ref = R.two_stage(n1, n2, atok, (F, H, W), 25.0, t.wq, t.cfg, up, t.sig, [float(s) for s in STAGE_2_DISTILLED_SIGMA_VALUES],
                         t.vctx, t.actx, t.nvctx, t.nactx, SCALE)
    with monkeypatch.context() as mp:
        mp.setattr(A, "frozen_audio_guided_loop", _eager_parent_loop)
        old = pipe.denoise_latent(alat.to(dev), vctx, nvctx, conf, **kw).cpu()
    tag = "v23" if t.v23 else "v20"
    e0 = measure(f"a2vid two-stage E0 parent's eager loops vs fp32 ({tag})", rel_l2(old, ref))
    e1 = measure(f"a2vid two-stage E1 pipeline vs fp32 ({tag})", rel_l2(final, ref))
    p = pearson(final, ref)
    print(f"a2vid two-stage {tag}: E0 = {e0:.4e}  E1 = {e1:.4e}  pearson = {p:.6f}")
    assert e1 <= 1.5 * e0 and p > 0.999
    # a distilled LoRA is fused for stage 2 only and taken out again, bit for bit
    lora = {}
    for name, (o, i) in (("transformer_blocks.0.attn1.to_k", (512, 512)), ("transformer_blocks.1.attn2.to_q", (512, 512)),
                         ("transformer_blocks.1.ff.net.0.proj", (2048, 512))):
        lora[f"diffusion_model.{name}.lora_A.weight"] = 0.3 * torch.randn(4, i, generator=g)
        lora[f"diffusion_model.{name}.lora_B.weight"] = 0.3 * torch.randn(o, 4, generator=g)
    path = str(tmp_path / "distilled_lora.safetensors")
    save_file(lora, path)
    lconf = A2VidConfig(height=128, width=192, num_frames=9, num_inference_steps=4, cfg_scale=SCALE, distilled_lora_config=LoRAConfig(path, 0.8))
    before = {k: v.clone() for k, v in t.m.weight_tensors().items()}
    with_lora = pipe.denoise_latent(alat.to(dev), vctx, nvctx, lconf, **kw).cpu()
    after = t.m.weight_tensors()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert bool(torch.isfinite(with_lora).all()) and not torch.equal(with_lora, final)
    assert torch.equal(pipe.denoise_latent(alat.to(dev), vctx, nvctx, conf, **kw).cpu(), final)
    with pytest.raises(ValueError, match=r"requires an audio-video \(AV\) model"):
        A2VidPipelineTwoStage(t.m._video_twin(), None, parts.dec, parts.up)
    with pytest.raises(ValueError, match="audio_latent is"):
        pipe(None, vctx, nvctx, conf, audio_latent=alat[:, :, :-1].to(dev), **kw)
    with pytest.raises(ValueError, match="audio_encoder"):
        pipe("in.wav", vctx, nvctx, conf, **kw)


# ------------------------------------------------------------------ 6. generate_video
def test_generate_video_a2vid_two_stage(dev, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    pcm = (8000 * np.sin(2 * np.pi * 330.0 * np.arange(3200) / 8000.0)).astype("<i2")          # 0.4 s, mono, 8 kHz
    with wave.open(str(tmp_path / "in.wav"), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(8000)
        f.writeframes(pcm.tobytes())
    rs = np.random.RandomState(11)
    emb = {k: (0.1 * rs.randn(1, 16, 3840)).astype(np.float32) for k in ("embedding", "audio_embedding", "negative_embedding", "negative_audio_embedding")}
    np.savez(tmp_path / "emb.npz", **emb)
    frames = generate.generate_video("a test prompt", a2vid_two_stage=True, audio_path=str(tmp_path / "in.wav"), spatial_upscaler_weights="random",
                                     model_variant="dev", cfg_scale=3, num_steps=2, num_layers=2, num_heads=2, vae_base_channels=64, height=128,
                                     width=192, num_frames=9, seed=3, embedding_path=str(tmp_path / "emb.npz"), output_path=str(tmp_path / "v.mp4"),
                                     save_mp4=False)
    assert frames.dtype == torch.uint8 and frames.shape == (9, 128, 192, 3)
    saved = np.load(tmp_path / "v.npz")["frames"]
    assert np.array_equal(saved, frames.cpu().numpy())
    lat = np.load(tmp_path / "v_audio_latent.npz")["latent"]
    want, wav, sr = generate.encode_audio_for_video(str(tmp_path / "in.wav"), 9, 25.0, None, seed=3 + 5)
    assert lat.shape == (1, 8, 9, 16) and np.isfinite(lat).all() and np.array_equal(lat, want.cpu().numpy())
    assert sr == 16000 and wav.shape == (1, 5760)
    cap = capsys.readouterr()
    assert "hipGraph replay skipped" not in cap.err and "DiT tokens per stage [12, 48]" in cap.out
