"""Retake with sound on the GPU: the sound track's glue kernels against their torch restatements (every bit), the pair step against two
launches of the single step (every bit), the joint guided engine step against its parts and its captured loop against the per-step loop (every
bit), and RetakePipeline with a sound track: what is kept is the encoded source bit for bit, what is regenerated is compared with the fp32
restatement of the reference's loop.  The tiny AudioVideo models of tests/test_parity.py (4 heads, 2 layers)."""
import numpy as np
import pytest
import torch

from conftest import measure, rel_l2

import ic_lora_ref as IR
import retake_av_ref as AR
from test_parity import make_av, pearson

pytestmark = pytest.mark.gpu
PATTERN = 1.5
V_SCALE, A_SCALE = 2.6, 7.0


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want):
    return int((_bits(got) != _bits(want)).sum())


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), PATTERN, dtype=torch.float32, device=dev)
    return buf, buf[:n].view(shape)


SPECIAL = [3.0e38, -3.0e38, 1.0e-40, -1.0e-42, 0.0, -0.0, 6.5e4, -1.17549435e-38]      # large, denormal, signed zeros


# ------------------------------------------------------------------ 1. retake_prepare_audio
@pytest.mark.parametrize("shape", [(8, 1, 16), (8, 37, 16), (3, 5, 7)])
def test_retake_prepare_audio_equals_torch(dev, shape):
    """clean, mask and latent equal, as int32 views, the separate fp32 torch statements, for the empty and the full window, [0, 1) and
    [T - 1, T), at two noise scales; nothing is written behind the outputs."""
    from ltx_2_mlx_amd import kernels as K
    c, t, m = shape
    g = torch.Generator().manual_seed(c * 100 + t)
    enc = torch.randn(1, c, t, m, generator=g)
    k = min(len(SPECIAL), enc.numel())
    enc.view(-1)[:k] = torch.tensor(SPECIAL[:k])
    noise = torch.randn(1, t, c * m, generator=g)
    enc, noise = enc.to(dev), noise.to(dev)
    for a0, a1 in ((0, 0), (t, t), (0, t), (0, 1), (t - 1, t)):
        for scale in (1.0, 0.7):
            want = AR.prepare_audio(enc, (a0, a1), noise, scale)
            bufs, outs = zip(*[_guarded(s, dev) for s in ((t, c * m), (t,), (t, c * m))])
            got = K.retake_prepare_audio(enc, noise[0], a0, a1, noise_scale=scale, out=outs)
            assert got[0].data_ptr() == outs[0].data_ptr()
            for name, x, ref in (("clean", got[0], want[0][0]), ("mask", got[1], want[1][0, :, 0]), ("latent", got[2], want[2][0])):
                assert _same_bits(x, ref) == 0, f"{name} window [{a0}, {a1}) scale {scale}: {_same_bits(x, ref)} of {ref.numel()} elements differ"
            for buf, s in zip(bufs, ((t, c * m), (t,), (t, c * m))):
                assert bool((buf[int(np.prod(s)):] == PATTERN).all())
            assert float(got[1].sum()) == a1 - a0
    for a0, a1 in ((1, 0), (-1, 1), (0, t + 1)):
        with pytest.raises(ValueError, match="window"):
            K.retake_prepare_audio(enc, noise[0], a0, a1)
    with pytest.raises(ValueError, match="noise"):
        K.retake_prepare_audio(enc, noise, 0, 1)
    with pytest.raises(ValueError, match="encoded"):
        K.retake_prepare_audio(enc[0], noise[0], 0, 1)
    o = [torch.empty(t, c * m, device=dev), torch.empty(t, device=dev), torch.empty(t, c * m, device=dev)]
    with pytest.raises(ValueError, match="overlap"):
        K.retake_prepare_audio(enc, noise[0], 0, 1, out=(o[0], o[1], o[0]))


# ------------------------------------------------------------------ 2. retake_composite_audio
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("samples", [1, 17, 4099])
def test_retake_composite_audio_equals_torch(dev, samples, channels):
    """Every bit of the separate fp32 torch statements, for windows at either end, in the middle and empty, ramps 0, 1 and longer than the
    clip; with ramp 0 every sample outside the window is the source's own bits, signed zeros, denormals and a decoded inf included."""
    from ltx_2_mlx_amd import kernels as K
    g = torch.Generator().manual_seed(samples * 3 + channels)
    dec, src = (torch.rand(channels, samples, generator=g) * 2 - 1 for _ in range(2))
    k = min(len(SPECIAL), samples)
    src[0, :k] = torch.tensor(SPECIAL[:k])
    dec[0, samples - 1] = float("inf")
    dec, src = dec.to(dev), src.to(dev)
    s = samples
    windows = {(0, 0), (s, s), (0, s), (0, 1), (s - 1, s), (0, (s + 1) // 2), (s // 2, s), (s // 3, s // 3 + max(1, s // 4))}
    for s0, s1 in sorted(w for w in windows if w[1] <= s):
        for ramp in (0, 1, s + 5):
            buf, out = _guarded((channels, s), dev)
            got = K.retake_composite_audio(dec, src, s0, s1, ramp, out=out)
            want = AR.composite_audio(dec, src, s0, s1, ramp)
            assert _same_bits(got, want) == 0, f"window [{s0}, {s1}) ramp {ramp}: {_same_bits(got, want)} of {want.numel()} samples differ"
            assert bool((buf[channels * s:] == PATTERN).all())
            assert _same_bits(got[:, s0:s1], dec[:, s0:s1]) == 0
            if ramp == 0:
                assert _same_bits(got[:, :s0], src[:, :s0]) == 0 and _same_bits(got[:, s1:], src[:, s1:]) == 0
    for alias in (dec, src):
        with pytest.raises(ValueError, match="overlap"):
            K.retake_composite_audio(dec, src, 0, 1, 1, out=alias)
    with pytest.raises(ValueError, match="window"):
        K.retake_composite_audio(dec, src, 1, 0, 0)
    with pytest.raises(ValueError, match="window"):
        K.retake_composite_audio(dec, src, 0, s + 1, 0)
    for ramp in (-1, 1 << 24):
        with pytest.raises(ValueError, match="ramp"):
            K.retake_composite_audio(dec, src, 0, 1, ramp)
    with pytest.raises(ValueError, match="source"):
        K.retake_composite_audio(dec, src.double(), 0, 1, 0)


# ------------------------------------------------------------------ 3. the pair step
@pytest.mark.parametrize("rows", [(5, 3), (2050, 67)], ids=["5x3", "2050x67"])
@pytest.mark.parametrize("v_mask", [False, True], ids=["v-plain", "v-mask"])
@pytest.mark.parametrize("a_mask", [False, True], ids=["a-plain", "a-mask"])
def test_guided_euler_step_pair_equals_two_single_launches(dev, rows, v_mask, a_mask):
    """Both segments of one ltx2_guided_euler_step_pair launch equal a ltx2_guided_euler_step launch of their own, bit for bit; the video
    under 2.6 and the audio under 7.0, so swapped scales or swapped operands fail; in place on x as the engine calls it."""
    from ltx_2_mlx_amd import kernels as K
    g = torch.Generator().manual_seed(rows[0] + 2 * v_mask + a_mask)
    sigma, sigma_next = 0.725, 0.421875
    segs, want, orig = [], [], []
    for n, masked, scale in ((rows[0], v_mask, V_SCALE), (rows[1], a_mask, A_SCALE)):
        x, vc, vu, clean = (torch.randn(n, 128, generator=g).to(dev) for _ in range(4))
        mask = (torch.arange(n) % 3 != 1).float().to(dev) if masked else None          # rows 0 and 2 regenerated, row 1 kept, and so on
        ts = (mask * sigma) if masked else torch.tensor([sigma], device=dev)
        want.append(K.guided_euler_step(x, vc, vu, ts, scale, sigma, sigma_next, mask=mask, clean=clean if masked else None))
        orig.append(x)
        segs.append(dict(x=x.clone(), vel_cond=vc, vel_uncond=vu, timesteps=ts, cfg_scale=scale, mask=mask, clean=clean if masked else None))
    for seg in segs:
        seg["out"] = seg["x"]
    got = K.guided_euler_step_pair(segs[0], segs[1], sigma, sigma_next)
    torch.cuda.synchronize()
    for name, a, b in (("video", got[0], want[0]), ("audio", got[1], want[1])):
        assert _same_bits(a, b) == 0, f"{name}: {_same_bits(a, b)} of {b.numel()} elements differ"
    assert got[0].data_ptr() == segs[0]["x"].data_ptr()
    a = segs[1]
    swapped = K.guided_euler_step(orig[1], a["vel_cond"], a["vel_uncond"], a["timesteps"], V_SCALE, sigma, sigma_next, mask=a["mask"], clean=a["clean"])
    assert not torch.equal(swapped, want[1])                 # the audio segment under the video's scale is another result
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        K.guided_euler_step_pair(segs[0], segs[1], 0.0, 0.5)


# ------------------------------------------------------------------ the tiny AudioVideo model
F, H, W, NA, S = 3, 2, 3, 18, 24
N = F * H * W


class Tiny:
    pass


@pytest.fixture(scope="module", params=[False, True], ids=["v20", "v23"])
def tiny(dev, request):
    from oracle import dit_av, loop
    from ltx_2_mlx_amd.components import LTX2Scheduler
    t = Tiny()
    t.v23 = request.param
    t.cfg, _, t.wq, t.m = make_av(dev, t.v23, seed=61 + t.v23)
    g = torch.Generator().manual_seed(311)
    cv, ca = t.cfg.caption_channels or t.cfg.inner_dim, t.cfg.caption_channels or t.cfg.audio_inner_dim
    t.vctx, t.nvctx = (0.1 * torch.randn(1, S, cv, generator=g) for _ in range(2))
    t.actx, t.nactx = (0.1 * torch.randn(1, S, ca, generator=g) for _ in range(2))
    t.vnoise, t.vclean = (torch.randn(1, N, 128, generator=g) for _ in range(2))
    t.anoise, t.aclean = (torch.randn(1, NA, 128, generator=g) for _ in range(2))
    t.vpos, t.apos = loop.video_positions(1, F, H, W, 24.0), dit_av.audio_positions(1, NA)
    t.vmask = torch.zeros(1, N, 1)
    t.vmask[:, 6:12] = 1.0                                   # latent frame 1
    t.amask = torch.zeros(1, NA, 1)
    t.amask[:, 1:11] = 1.0                                   # the audio tokens of the same seconds
    t.sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    return t


def _states(t, dev, masked=True):
    """(video state, audio state): noise on the masked tokens, the clean latent elsewhere; masked=False: all ones, pure noise."""
    from ltx_2_mlx_amd.types import LatentState
    out = []
    for noise, clean, mask, pos in ((t.vnoise, t.vclean, t.vmask, t.vpos), (t.anoise, t.aclean, t.amask, t.apos)):
        mk = mask if masked else torch.ones_like(mask)
        lat = noise * mk + clean * (1 - mk)
        out.append(LatentState(latent=lat.to(dev), denoise_mask=mk.to(dev), positions=pos.to(dev), clean_latent=clean.clone().to(dev)))
    return out


def _ctx(t, dev):
    if not hasattr(t, "dev_ctx"):
        t.dev_ctx = tuple(c.to(dev) for c in (t.vctx, t.actx, t.nvctx, t.nactx))
    return t.dev_ctx


# ------------------------------------------------------------------ 4. the engine step
@pytest.mark.parametrize("masked", [False, True], ids=["uniform", "window"])
def test_guided_step_joint_av_equals_its_parts(dev, tiny, masked):
    """guided_step_joint_av_ == forward_av(ctx), forward_av(neg), ltx2_guided_euler_step_pair called separately: the same kernels in the same
    order, so the same bits on both latents."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.pipelines.common import audio_modality_from_state, modality_from_state
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    vctx, actx, nvctx, nactx = _ctx(t, dev)
    sigma, sigma_next = t.sig[1], t.sig[2]
    vs, as_ = _states(t, dev, masked)
    mods = lambda vc, ac: (modality_from_state(vs, vc, sigma, uniform=not masked), audio_modality_from_state(as_, ac, sigma, uniform=not masked))      # noqa: E731
    cond, unc = m(*mods(vctx, actx)), neg(*mods(nvctx, nactx))
    segs = []
    for k, (st, scale) in enumerate(((vs, V_SCALE), (as_, A_SCALE))):
        mk = st.denoise_mask[0].reshape(-1).contiguous() if masked else None
        segs.append(dict(x=st.latent[0].float().contiguous(), vel_cond=cond[k][0].clone(), vel_uncond=unc[k][0].clone(), cfg_scale=scale, mask=mk,
                         clean=st.clean_latent[0].contiguous() if masked else None,
                         timesteps=(mk * sigma) if masked else torch.tensor([sigma], device=dev)))
        assert float((segs[k]["vel_cond"] - segs[k]["vel_uncond"]).abs().max()) > 1e-3
    want = K.guided_euler_step_pair(segs[0], segs[1], sigma, sigma_next)
    lat, alat = segs[0]["x"].clone(), segs[1]["x"].clone()
    m.guided_step_joint_av_(neg, lat, alat, *mods(vctx, actx), sigma, sigma_next, V_SCALE, A_SCALE, denoise_mask=segs[0]["mask"],
                            clean_latent=segs[0]["clean"], audio_denoise_mask=segs[1]["mask"], audio_clean_latent=segs[1]["clean"])
    torch.cuda.synchronize()
    assert _same_bits(lat, want[0]) == 0 and _same_bits(alat, want[1]) == 0
    assert not torch.equal(lat, segs[0]["x"]) and not torch.equal(alat, segs[1]["x"]) and bool(torch.isfinite(lat).all() and torch.isfinite(alat).all())
    if masked:                                                # the tokens outside the windows keep their clean bits
        keep_v, keep_a = (t.vmask[0, :, 0] == 0).to(dev), (t.amask[0, :, 0] == 0).to(dev)
        assert _same_bits(lat[keep_v], vs.clean_latent[0][keep_v]) == 0 and _same_bits(alat[keep_a], as_.clean_latent[0][keep_a]) == 0
        with pytest.raises(ValueError, match="mask and clean go together"):
            m.guided_step_joint_av_(neg, lat, alat, *mods(vctx, actx), sigma, sigma_next, V_SCALE, A_SCALE, denoise_mask=segs[0]["mask"],
                                    clean_latent=segs[0]["clean"], audio_denoise_mask=segs[1]["mask"])
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        m.guided_step_joint_av_(neg, lat, alat, *mods(vctx, actx), 0.0, 0.5, V_SCALE, A_SCALE)
    with pytest.raises(ValueError, match="AudioVideo contexts"):
        m.guided_step_joint_av_(m._video_twin(), lat, alat, *mods(vctx, actx), sigma, sigma_next, V_SCALE, A_SCALE)


# ------------------------------------------------------------------ 5. the captured loop
def test_joint_guided_loop_graph_equals_eager(dev, tiny):
    """4 steps, masks on both modalities: the captured graph, the per-step C calls (a callback forces them) and the loop written out by hand
    over guided_step_joint_av_ give the same bits on both latents; scales of at most 1 are joint_denoise_loop's run."""
    from ltx_2_mlx_amd.components import EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import joint_denoise_loop, joint_guided_denoise_loop
    t = tiny
    x0m, st = X0Model(t.m), EulerDiffusionStep()
    ctx = _ctx(t, dev)

    def run(graph, callback=None, masked=True, scales=(V_SCALE, A_SCALE)):
        v, a = joint_guided_denoise_loop(x0m, *_states(t, dev, masked), t.sig, *ctx, *scales, st, callback, graph)
        torch.cuda.synchronize()
        return v.latent, a.latent

    seen = []
    graph, eager = run(True), run(False)
    cb = run(True, callback=lambda i, n: seen.append((i, n)))
    for k in range(2):
        assert _same_bits(graph[k], eager[k]) == 0, f"modality {k}: {_same_bits(graph[k], eager[k])} elements differ"
        assert _same_bits(cb[k], eager[k]) == 0
    assert seen == [(1, 4), (2, 4), (3, 4), (4, 4)]
    vs, as_ = _states(t, dev)
    keep_v, keep_a = (t.vmask[0, :, 0] == 0).to(dev), (t.amask[0, :, 0] == 0).to(dev)
    assert _same_bits(graph[0][0][keep_v], vs.clean_latent[0][keep_v]) == 0 and _same_bits(graph[1][0][keep_a], as_.clean_latent[0][keep_a]) == 0
    assert rel_l2(graph[0][0][~keep_v].cpu(), vs.latent[0][~keep_v].cpu()) > 0.1 and rel_l2(graph[1][0][~keep_a].cpu(), as_.latent[0][~keep_a].cpu()) > 0.1
    u_graph, u_eager = run(True, masked=False), run(False, masked=False)                      # the uniform form: one timestep per modality
    assert _same_bits(u_graph[0], u_eager[0]) == 0 and _same_bits(u_graph[1], u_eager[1]) == 0
    other = run(True, scales=(A_SCALE, V_SCALE))
    assert not torch.equal(other[0], graph[0]) and not torch.equal(other[1], graph[1])          # each modality listens to its own scale
    plain = joint_denoise_loop(x0m, True, *_states(t, dev), t.sig, ctx[0], ctx[1], st, None, True)
    for scales, c in (((1.0, 1.0), ctx), ((V_SCALE, A_SCALE), (ctx[0], ctx[1], None, ctx[3])), ((V_SCALE, A_SCALE), (ctx[0], ctx[1], ctx[2], None))):
        v, a = joint_guided_denoise_loop(x0m, *_states(t, dev), t.sig, *c, *scales, st, None, True)
        assert torch.equal(v.latent, plain[0].latent) and torch.equal(a.latent, plain[1].latent)
    with pytest.raises(RuntimeError, match="no guided AudioVideo graph"):
        t.m.replay_guided_av_graph()                                                             # the capture is recorded under its own kind
    with torch.cuda.stream(torch.cuda.Stream()):
        neg = t.m.clone_sharing_weights()
        t.m.prepare(ctx[0], vs.positions, per_token=True, audio_context=ctx[1], audio_positions=as_.positions)
        neg.prepare(ctx[2], vs.positions, per_token=True, audio_context=ctx[3], audio_positions=as_.positions)
        lat, alat = vs.latent[0].clone(), as_.latent[0].clone()
        amk, acl = as_.denoise_mask[0].reshape(-1).contiguous(), as_.clean_latent[0].contiguous()
        with pytest.raises(ValueError, match="tokens x"):
            t.m.capture_guided_joint_graph(neg, lat, alat, t.sig, V_SCALE, A_SCALE, audio_denoise_mask=amk[:NA - 1].contiguous(), audio_clean_latent=acl)
        with pytest.raises(ValueError, match="bad argument"):
            t.m.capture_guided_joint_graph(neg, lat, alat, [1.0 - 0.01 * i for i in range(66)], V_SCALE, A_SCALE)


# ------------------------------------------------------------------ 6. the pipeline
WINDOW = (0.4, 0.7)             # at 24 fps: latent frame 1 of 3, pixel frames [1, 9), 1/24 s .. 9/24 s: audio tokens [1, 11) of 18
# rel-L2 of the regenerated window against the fp32 restatement of the reference's loop, measured on the MI355X (Pearson 0.999997 or better)
GUIDED_MEASURED = {"video": 1.2746e-3, "audio": 2.4889e-3}
DISTILLED_MEASURED = {"video": 5.8078e-4, "audio": 4.1734e-4}


@pytest.fixture(scope="module")
def parts(dev):
    from oracle import vae_encoder as oenc
    from ltx_2_mlx_amd.model.video_vae_encoder import SimpleVideoEncoder
    p = Tiny()
    p.cfg, _, p.wq, p.m = make_av(dev, True, seed=67)
    w = oenc.make_encoder_weights(seed=53)
    p.enc_wq = {k: (v.to(torch.bfloat16).float() if v.dim() == 5 else v) for k, v in w.items()}
    p.enc = SimpleVideoEncoder(device=dev)
    p.enc.load_state_dict(w)
    g = torch.Generator().manual_seed(97)
    p.vctx, p.nvctx = (0.1 * torch.randn(1, S, p.cfg.inner_dim, generator=g) for _ in range(2))
    p.actx, p.nactx = (0.1 * torch.randn(1, S, p.cfg.audio_inner_dim, generator=g) for _ in range(2))
    p.source = torch.randint(0, 256, (17, 64, 96, 3), generator=g, dtype=torch.uint8).numpy()       # latent 3 x 2 x 3: 18 tokens; 17 / 24 s: 18 audio tokens
    p.vnoise, p.anoise = torch.randn(1, N, 128, generator=g), torch.randn(1, NA, 128, generator=g)
    p.track = torch.randn(1, 8, NA, 16, generator=g)                                                  # the encoded sound track
    p.encoded_ref = oenc.encoder_forward(IR.control_tensor(p.source), p.enc_wq)                       # the oracle's encoding, once
    return p


def _conf(window=WINDOW, **kw):
    from ltx_2_mlx_amd.pipelines import RetakeConfig
    return RetakeConfig(start_time=window[0], end_time=window[1], fps=24.0, **kw)


def _run(pipe, p, dev, conf, callback=None, **kw):
    args = dict(negative_text_encoding=p.nvctx.to(dev), audio_encoding=p.actx.to(dev), negative_audio_encoding=p.nactx.to(dev), callback=callback,
                frames=p.source, initial_noise=p.vnoise.to(dev), audio_latent=p.track.to(dev), initial_audio_noise=p.anoise.to(dev))
    args.update(kw)
    return pipe(None, p.vctx.to(dev), None, conf, **args)


def _encoded(p, dev):
    from ltx_2_mlx_amd.pipelines import load_control_signal_tensor
    if not hasattr(p, "encoded"):
        p.encoded = p.enc(load_control_signal_tensor(p.source).to(dev))
    return p.encoded


def _gate(mode, pairs, measured):
    """pairs: modality -> (the regenerated window, the restatement's).  Every figure is printed before the first one is asserted."""
    figures = {}
    for name, (got, ref) in pairs.items():
        err = measure(f"retake with sound, {mode}, {name} window vs fp32 restatement", rel_l2(got, ref))
        figures[name] = (err, pearson(got, ref))
        print(f"retake with sound, {mode}, {name} window: rel-L2 = {err:.4e}  pearson = {figures[name][1]:.6f}")
    for name, (err, r) in figures.items():
        assert err <= 5 * measured[name] and r > 0.999, f"{mode}, {name}: rel-L2 {err:.4e} against 5 x {measured[name]:.4e}, pearson {r:.6f}"


def test_pipeline_guided(dev, parts):
    """17 x 64 x 96 at 24 fps with an 18-token track, the window 0.4 s - 0.7 s, LTX2Scheduler over 4 steps, cfg 2.6 on the video and 7.0 on
    the audio.  Latent frames 0 and 2 and the audio tokens outside [1, 11) come back as encoded, bit for bit; the captured run equals the run
    with a callback; the window is compared with tests/retake_av_ref.retake_av_latents (oracle VAE encoder, oracle AudioVideo DiT, the
    reference's loop in fp32): the gate is 5 x the rel-L2 measured on the MI355X, 1.2746e-03 (video) and 2.4889e-03 (audio), and Pearson > 0.999
    (measured 0.999999 / 0.999997)."""
    from ltx_2_mlx_amd.pipelines import RetakePipeline
    p = parts
    pipe = RetakePipeline(p.m, p.enc, None)
    conf = _conf(num_inference_steps=4, cfg_scale=V_SCALE, audio_cfg_scale=A_SCALE)
    video, audio = _run(pipe, p, dev, conf)
    assert video.shape == (1, 128, 3, 2, 3) and audio.shape == (1, 8, NA, 16) and bool(torch.isfinite(video).all() and torch.isfinite(audio).all())
    assert (pipe.frame_window, pipe.pixel_window, pipe.audio_window, pipe.audio_sample_window) == ((1, 2), (1, 9), (1, 11), None)
    assert torch.equal(pipe.audio_latent, audio)
    enc, track = _encoded(p, dev), p.track.to(dev)
    for k in (0, 2):
        assert _same_bits(video[:, :, k], enc[:, :, k]) == 0
    assert _same_bits(audio[:, :, :1], track[:, :, :1]) == 0 and _same_bits(audio[:, :, 11:], track[:, :, 11:]) == 0
    assert not torch.equal(video[:, :, 1], enc[:, :, 1]) and not bool((audio[:, :, 1:11] == track[:, :, 1:11]).all(dim=1).all(dim=-1).any())
    seen = []
    ev, ea = _run(pipe, p, dev, conf, callback=lambda *a: seen.append(a))
    assert _same_bits(ev, video) == 0 and _same_bits(ea, audio) == 0 and seen == [("retake", i + 1, 4) for i in range(4)]
    single = _run(pipe, p, dev, _conf(num_inference_steps=4, cfg_scale=V_SCALE))                  # audio_cfg_scale None: cfg_scale on both
    assert torch.equal(single[0][:, :, 0], video[:, :, 0]) and not torch.equal(single[1], audio)
    from ltx_2_mlx_amd.components import LTX2Scheduler
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    rv, ra = AR.retake_av_latents(p.encoded_ref, (1, 2), p.vnoise, p.track, (1, 11), p.anoise, p.wq, p.cfg, sig, p.vctx, p.actx, p.nvctx, p.nactx,
                                  V_SCALE, A_SCALE)
    _gate("guided", {"video": (video[:, :, 1].cpu(), rv[:, :, 1]), "audio": (audio[:, :, 1:11].cpu(), ra[:, :, 1:11])}, GUIDED_MEASURED)


def test_pipeline_distilled_and_flags(dev, parts):
    """The 8 distilled steps through joint_denoise_loop with both states, against the restatement without guidance (gate: 5 x the rel-L2
    measured on the MI355X, 5.8078e-04 video / 4.1734e-04 audio); regenerate_video=False
    returns the encoded clip everywhere and retakes the track over (start_time, end_time); regenerate_audio=False returns the encoded
    track; both False, a guider override, a missing audio context and a window that meets no audio token are refused."""
    from ltx_2_mlx_amd.components import DISTILLED_SIGMA_VALUES, CFGGuider
    from ltx_2_mlx_amd.pipelines import RetakePipeline
    p = parts
    pipe = RetakePipeline(p.m, p.enc, None)
    enc, track = _encoded(p, dev), p.track.to(dev)
    video, audio = _run(pipe, p, dev, _conf(distilled=True))
    for k in (0, 2):
        assert _same_bits(video[:, :, k], enc[:, :, k]) == 0
    assert _same_bits(audio[:, :, :1], track[:, :, :1]) == 0 and _same_bits(audio[:, :, 11:], track[:, :, 11:]) == 0
    sig = [float(s) for s in DISTILLED_SIGMA_VALUES]
    rv, ra = AR.retake_av_latents(p.encoded_ref, (1, 2), p.vnoise, p.track, (1, 11), p.anoise, p.wq, p.cfg, sig, p.vctx, p.actx)
    # the flags
    guided = dict(num_inference_steps=4, cfg_scale=V_SCALE, audio_cfg_scale=A_SCALE)
    v, a = _run(pipe, p, dev, _conf(regenerate_video=False, **guided))
    assert _same_bits(v, enc) == 0 and pipe.frame_window == (0, 0) and pipe.pixel_window == (0, 0)
    assert pipe.audio_window == AR.audio_window(0.4, 0.7, NA) == (10, 18)                        # (start_time, end_time) itself
    assert _same_bits(a[:, :, :10], track[:, :, :10]) == 0 and not torch.equal(a[:, :, 10:], track[:, :, 10:])
    v, a = _run(pipe, p, dev, _conf(regenerate_audio=False, **guided))
    assert _same_bits(a, track) == 0 and pipe.audio_window == (0, 0) and not torch.equal(v[:, :, 1], enc[:, :, 1])
    assert _same_bits(v[:, :, 0], enc[:, :, 0]) == 0
    with pytest.raises(ValueError, match="both False"):
        _run(pipe, p, dev, _conf(regenerate_video=False, regenerate_audio=False, **guided))
    with pytest.raises(NotImplementedError, match="guider override"):
        _run(pipe, p, dev, _conf(**guided), guider=CFGGuider(2.0))
    with pytest.raises(ValueError, match="audio_encoding"):
        _run(pipe, p, dev, _conf(**guided), audio_encoding=None)
    with pytest.raises(ValueError, match="touches no audio token"):
        _run(pipe, p, dev, _conf((5.0, 6.0), regenerate_video=False, **guided))
    with pytest.raises(ValueError, match="audio_latent is"):
        _run(pipe, p, dev, _conf(**guided), audio_latent=p.track[:, :, :-1].to(dev))
    with pytest.raises(ValueError, match="audio_encoder"):
        _run(pipe, p, dev, _conf(**guided), audio_latent=None, audio_path="track.wav")
    # a seed instead of supplied noises: the same seed, the same bits; the video noise is the silent path's draw
    a1 = _run(pipe, p, dev, _conf(distilled=True, seed=5), initial_noise=None, initial_audio_noise=None)
    a2 = _run(pipe, p, dev, _conf(distilled=True, seed=5), initial_noise=None, initial_audio_noise=None)
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[1], a2[1]) and not torch.equal(a1[1], audio)
    _gate("distilled", {"video": (video[:, :, 1].cpu(), rv[:, :, 1]), "audio": (audio[:, :, 1:11].cpu(), ra[:, :, 1:11])}, DISTILLED_MEASURED)


def test_silent_path_unchanged(dev, parts):
    """Without an audio argument the AudioVideo model's retake is what it was: one tensor, the video twin's loop, regenerate_video=False
    regenerating every frame."""
    from ltx_2_mlx_amd.pipelines import RetakePipeline
    p = parts
    pipe = RetakePipeline(p.m, p.enc, None)
    out = pipe(None, p.vctx.to(dev), None, _conf(distilled=True), frames=p.source, initial_noise=p.vnoise.to(dev))
    assert isinstance(out, torch.Tensor) and out.shape == (1, 128, 3, 2, 3) and pipe.audio_window is None and pipe.audio_latent is None
    full = pipe(None, p.vctx.to(dev), None, _conf(distilled=True, regenerate_video=False), frames=p.source, initial_noise=p.vnoise.to(dev))
    assert pipe.frame_window == (0, 3) and not torch.equal(full[:, :, 0], _encoded(p, dev)[:, :, 0])


def test_decoded_waveform_composite(dev, tmp_path):
    """_decode_audio with composite_source_audio on stand-in decoders: the source file, loaded at the vocoder's rate, one channel put on both
    and padded with silence to the waveform's length, comes back outside the audio window's samples -- bit for bit at ramp 0, the
    restatement's fade at 20 ms (480 samples at 24 kHz)."""
    import wave
    from ltx_2_mlx_amd.model.audio_vae import load_audio_file
    from ltx_2_mlx_amd.model.transformer import LTXModelType, X0Model
    from ltx_2_mlx_amd.pipelines import RetakeConfig, RetakePipeline
    pcm = (8000 * np.sin(2 * np.pi * 330.0 * np.arange(12000) / 24000.0)).astype("<i2")           # 0.5 s, mono, 24 kHz
    path = str(tmp_path / "track.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(24000)
        f.writeframes(pcm.tobytes())
    samples = 16560                                            # (4 * 18 - 3) mel frames of 240 samples
    decoded = torch.rand(1, 2, samples, generator=torch.Generator().manual_seed(4)).to(dev) * 2 - 1

    class Vocoder:
        output_sample_rate = 24000

        def __call__(self, mel):
            return decoded

    class AV:
        model_type = LTXModelType.AudioVideo

    pipe = RetakePipeline(X0Model(AV()), object(), None, audio_decoder=lambda latent: latent, vocoder=Vocoder())
    loaded, rate = load_audio_file(path, 24000)
    assert rate == 24000 and loaded.shape == (1, 12000)
    source = torch.zeros(2, samples)
    source[:, :12000] = torch.from_numpy(np.asarray(loaded, dtype=np.float32))
    source = source.to(dev)
    pipe.audio_window = (1, 11)
    for ramp_ms, ramp in ((0.0, 0), (20.0, 480)):
        conf = RetakeConfig(start_time=0.4, end_time=0.7, fps=24.0, composite_source_audio=True, audio_composite_ramp_ms=ramp_ms)
        got = pipe._decode_audio(torch.zeros(1, 8, NA, 16, device=dev), path, conf)
        assert pipe.audio_sample_window == (240, 9840) and got.shape == (2, samples)
        assert _same_bits(got, AR.composite_audio(decoded[0], source, 240, 9840, ramp)) == 0
        assert _same_bits(got[:, 240:9840], decoded[0][:, 240:9840]) == 0
        if ramp == 0:
            assert _same_bits(got[:, :240], source[:, :240]) == 0 and _same_bits(got[:, 9840:], source[:, 9840:]) == 0
        else:
            assert _same_bits(got[:, 9840 + 480:], source[:, 9840 + 480:]) == 0 and not torch.equal(got[:, 9840:9840 + 480], source[:, 9840:9840 + 480])


@pytest.mark.parametrize("how", ["odd-C", "audio-offset"])
def test_guided_euler_step_pair_scalar_path(dev, how):
    """Where either segment rules out 16-byte accesses the pair launch goes one element per lane on BOTH: an odd C on the audio, or an audio
    latent that starts 4 bytes off a 16-byte boundary.  Each segment still equals the single launch, which for the video is the vector form."""
    from ltx_2_mlx_amd import kernels as K
    g = torch.Generator().manual_seed(17)
    sigma, sigma_next = 0.725, 0.421875
    ca = 127 if how == "odd-C" else 128

    def operands(n, c, shift):
        out = []
        for _ in range(4):
            buf = torch.randn(n * c + 4, generator=g).to(dev)
            out.append(buf[shift: shift + n * c].view(n, c))
        return out

    segs, want = [], []
    for n, c, shift, scale in ((261, 128, 0, V_SCALE), (67, ca, 1 if how == "audio-offset" else 0, A_SCALE)):
        x, vc, vu, clean = operands(n, c, shift)
        assert x.data_ptr() % 16 == 4 * shift
        mask = (torch.arange(n) % 3 != 1).float().to(dev)
        want.append(K.guided_euler_step(x, vc, vu, mask * sigma, scale, sigma, sigma_next, mask=mask, clean=clean))
        segs.append(dict(x=x, vel_cond=vc, vel_uncond=vu, timesteps=mask * sigma, cfg_scale=scale, mask=mask, clean=clean))
    got = K.guided_euler_step_pair(segs[0], segs[1], sigma, sigma_next)
    torch.cuda.synchronize()
    assert _same_bits(got[0], want[0]) == 0 and _same_bits(got[1], want[1]) == 0


# ------------------------------------------------------------------ 7. generate_video
def test_generate_video_retake_av(dev, tmp_path, capsys):
    """--retake clip --retake-audio track --retake-keep-source with decoded audio: the frames beyond the 4-frame fade are the clip's, the
    written track beyond the window and its 20 ms fade is the source track as write_wav writes it, inside the window it is not."""
    import os
    import sys
    import wave
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import generate
    from ltx_2_mlx_amd.model.audio_vae import load_audio_file
    rng = np.random.default_rng(6)
    clip = rng.integers(0, 256, (20, 64, 96, 3), dtype=np.uint8)             # 20 frames are snapped down to 17
    np.save(tmp_path / "clip.npy", clip)
    pcm = (8000 * np.sin(2 * np.pi * 330.0 * np.arange(16000) / 24000.0)).astype("<i2")           # 0.667 s, mono, 24 kHz
    track = str(tmp_path / "track.wav")
    with wave.open(track, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(24000)
        f.writeframes(pcm.tobytes())
    frames = generate.generate_video("p", retake_video=str(tmp_path / "clip.npy"), retake_audio=track, retake_start_time=0.4, retake_end_time=0.7,
                                     output_fps=24, use_gemma=False, model_variant="dev", cfg_scale=3.0, retake_audio_cfg=7.0, num_steps=2, num_layers=2,
                                     num_heads=2, vae_base_channels=64, retake_composite=True, decode_audio=True, seed=3, save_mp4=False,
                                     output_path=str(tmp_path / "v.mp4"))
    assert frames.dtype == torch.uint8 and frames.shape == (17, 64, 96, 3)
    saved = np.load(tmp_path / "v.npz")["frames"]
    assert np.array_equal(saved, frames.cpu().numpy()) and np.array_equal(saved[13:], clip[13:17]) and not np.array_equal(saved[1:9], clip[1:9])
    lat = np.load(tmp_path / "v_audio_latent.npz")["latent"]
    assert lat.shape == (1, 8, 18, 16) and np.isfinite(lat).all()
    with wave.open(str(tmp_path / "v.wav"), "rb") as f:
        assert (f.getnchannels(), f.getframerate(), f.getnframes()) == (2, 24000, 16560)
        got = np.frombuffer(f.readframes(16560), "<i2").reshape(-1, 2).T
    src, _ = load_audio_file(track, 24000)
    want = np.zeros((2, 16560), np.float32)
    want[:, :16000] = src
    want = (want * 32767).clip(-32768, 32767).astype(np.int16)
    assert np.array_equal(got[:, 9840 + 480:], want[:, 9840 + 480:])          # (before the window the 480-sample fade reaches sample 0)
    assert not np.array_equal(got[:, 240:9840], want[:, 240:9840])
    out = capsys.readouterr().out
    assert "Using Retake Pipeline (picture and sound)" in out and "audio tokens [1, 11) retaken, samples [240, 9840]" in out
    assert "latent frames [1, 2) of 3, 18 DiT tokens, source frames and samples kept outside it" in out
