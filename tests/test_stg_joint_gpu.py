"""STG with sound on the GPU: ltx2_stg_euler_step_pair against single launches bit for bit, ltx2_dit_stg_step_joint_av against its parts bit
for bit, joint_stg_denoise_loop's device form against its eager form, the audio STG term against the zeroed-weights identity, the refusals
of the step entry, and OneStagePipeline(stg_audio_scale=...) against tests/stg_joint_ref.  The tiny AudioVideo model of
tests/test_joint_projected_gpu.py with 3 layers (make_av seed 23; 64 x 96, 9 frames: 12 video and 9 audio tokens), STG set = block 1."""
import itertools

import pytest
import torch

from conftest import measure, rel_l2

import stg_joint_ref as JR
import stg_ref as R
from test_parity import make_av

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
SIGMA, SIGMA_NEXT = 0.909375, 0.725

# rel-L2 measured on the MI355X; every gate is 5 x its figure, (video latent, audio latent)
LOOP_MEASURED = (1.035e-7, 2.364e-7)          # joint_stg_denoise_loop: the device form against the eager form (X0Model's contracted x0 and Euler kernels)
PIPE_MEASURED = (3.414e-3, 5.659e-3)          # OneStagePipeline, plain CFG 3 / 7, STG 1 / 1, 4 steps, against tests/stg_joint_ref.stg_joint_loop


# ------------------------------------------------------------------ 1. the kernel
def _segment(dev, rows, C, seed, per_row, masked, with_vu, with_vp, cfg, stg):
    """One segment's operands on the device, every [rows][C] buffer followed by 64 sentinel floats -> (the dict of kernels.stg_euler_step_pair
    with `out` set, the buffer `out` lives in)."""
    d = JR.inputs(rows, C, seed)
    n = rows * C
    obuf = torch.full((n + 64,), SENTINEL, device=dev)
    seg = dict(x=d["x"].to(dev), vel_cond=d["vc"].to(dev), vel_uncond=d["vu"].to(dev) if with_vu else None, vel_perturbed=d["vp"].to(dev) if with_vp else None,
               timesteps=(d["ts_row"] if per_row else torch.tensor([SIGMA])).to(dev), mask=d["mask"].to(dev) if masked else None,
               clean=d["clean"].to(dev) if masked else None, cfg_scale=cfg, stg_scale=stg, out=obuf[:n].view(rows, C))
    return seg, obuf


def _single(K, seg):
    """The segment through the single-launch entry that has its arithmetic: ltx2_stg_euler_step, without a perturbed velocity
    ltx2_guided_euler_step, with neither velocity the restatement (ltx2_euler_step's formula, individually rounded)."""
    kw = dict(mask=seg["mask"], clean=seg["clean"])
    if seg["vel_perturbed"] is not None:
        return K.stg_euler_step(seg["x"], seg["vel_cond"], seg["vel_uncond"], seg["vel_perturbed"], seg["timesteps"], seg["cfg_scale"], seg["stg_scale"], SIGMA,
                                SIGMA_NEXT, **kw)
    if seg["vel_uncond"] is not None:
        return K.guided_euler_step(seg["x"], seg["vel_cond"], seg["vel_uncond"], seg["timesteps"], seg["cfg_scale"], SIGMA, SIGMA_NEXT, **kw)
    return torch.from_numpy(JR.pair_segment(seg["x"], seg["vel_cond"], None, None, seg["timesteps"], seg["mask"], seg["clean"], seg["cfg_scale"], seg["stg_scale"],
                                            SIGMA, SIGMA_NEXT)).to(seg["x"].device)


SHAPES = [(37, 128, 5, 6), (5, 6, 9, 128), (33000, 128, 9, 128)]


@pytest.mark.parametrize("v_rows,v_C,a_rows,a_C", SHAPES, ids=["37x128+5x6", "5x6+9x128", "33000x128+9x128"])
def test_pair_equals_single_launches_bit_for_bit(dev, v_rows, v_C, a_rows, a_C):
    """Both segments of one ltx2_stg_euler_step_pair launch equal a single launch of their own, bit for bit: scalar and per-row timesteps, the
    mask absent / present / mixed, vel_uncond and vel_perturbed NULL per segment, in place, and nothing written behind an output.  The
    large shape (more than grid_for's cap of blocks) runs a diagonal of those combinations."""
    from ltx_2_mlx_amd import kernels as K
    big = v_rows > 1000
    flags = list(itertools.product((False, True), repeat=2))
    combos = list(itertools.product((False, True), flags, flags, flags))          # per_row, mask (v, a), vu (v, a), vp (v, a)
    if big:
        combos = [(i % 2 == 0, flags[i % 4], flags[(i + 1) % 4], flags[(i + 2) % 4]) for i in range(4)]
    singles = {}
    for per_row, masked, with_vu, with_vp in combos:
        segs, bufs = zip(*(_segment(dev, r, c, 11 * k + r, per_row, masked[k], with_vu[k], with_vp[k], (3.0, 7.0)[k], (1.5, 0.75)[k])
                           for k, (r, c) in enumerate(((v_rows, v_C), (a_rows, a_C)))))
        got = K.stg_euler_step_pair(*segs, SIGMA, SIGMA_NEXT)
        tag = f"per_row={per_row} mask={masked} vu={with_vu} vp={with_vp}"
        for k in range(2):
            key = (k, per_row, masked[k], with_vu[k], with_vp[k])
            if key not in singles:
                singles[key] = _single(K, segs[k])
            n = segs[k]["x"].numel()
            assert got[k].data_ptr() == segs[k]["out"].data_ptr()
            assert torch.equal(got[k], singles[key]), f"{tag} segment {k}: {int((got[k] != singles[key]).sum())} of {n} elements differ"
            assert bool((bufs[k][n:] == SENTINEL).all()), f"{tag} segment {k}: written behind the output"
        # in place: out == x on both segments, the same bits
        inplace = []
        for k in range(2):
            n = segs[k]["x"].numel()
            xbuf = torch.full((n + 64,), SENTINEL, device=dev)
            xin = xbuf[:n].view_as(segs[k]["x"])
            xin.copy_(segs[k]["x"])
            inplace.append((dict(segs[k], x=xin, out=xin), xbuf))
        K.stg_euler_step_pair(inplace[0][0], inplace[1][0], SIGMA, SIGMA_NEXT)
        for k in range(2):
            n = segs[k]["x"].numel()
            assert torch.equal(inplace[k][0]["x"], got[k]) and bool((inplace[k][1][n:] == SENTINEL).all()), f"{tag} segment {k} in place"
    if not big:
        # against the float64 restatement itself, every operand present
        segs = [_segment(dev, r, c, 5 + k, True, True, True, True, (3.0, 7.0)[k], (1.5, 0.75)[k])[0] for k, (r, c) in enumerate(((v_rows, v_C), (a_rows, a_C)))]
        got = K.stg_euler_step_pair(*segs, SIGMA, SIGMA_NEXT)
        want = JR.pair(*segs, SIGMA, SIGMA_NEXT)
        assert all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want))


def test_pair_off_alignment_and_refusals(dev):
    """Each [rows][C] operand of either segment 4 bytes off a 16-byte boundary: the element-wise form of BOTH segments, the same bits.
    sigma == 0 and a missing required operand are refused."""
    from ltx_2_mlx_amd import kernels as K
    mk = lambda: [_segment(dev, r, 128, 3 + k, True, True, True, True, (3.0, 7.0)[k], (1.5, 0.75)[k]) for k, r in enumerate((37, 9))]      # noqa: E731
    want = [w.clone() for w in K.stg_euler_step_pair(*(s for s, _ in mk()), SIGMA, SIGMA_NEXT)]
    for k in range(2):
        for name in ("x", "vel_cond", "vel_uncond", "vel_perturbed", "clean", "out"):
            segs = [s for s, _ in mk()]
            n = segs[k]["x"].numel()
            off = torch.full((n + 65,), SENTINEL, device=dev)
            moved = off[1:1 + n].view_as(segs[k]["x"])
            if name != "out":
                moved.copy_(segs[k][name])
            assert moved.data_ptr() % 16 == 4
            segs[k][name] = moved
            got = K.stg_euler_step_pair(*segs, SIGMA, SIGMA_NEXT)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"segment {k}, {name} off alignment"
            assert float(off[0]) == SENTINEL and bool((off[1 + n:] == SENTINEL).all())
    segs = [s for s, _ in mk()]
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        K.stg_euler_step_pair(*segs, 0.0, 0.5)
    with pytest.raises(ValueError, match="mask and clean go together"):
        from ltx_2_mlx_amd import _native as nv
        s = segs[0]
        args = [x for sg in (dict(s, clean=None), segs[1]) for x in (nv.ptr(sg["x"]), nv.ptr(sg["vel_cond"]), None, None, nv.ptr(sg["timesteps"]), 1, nv.ptr(sg["mask"]),
                                                                    nv.ptr(sg["clean"]), 3.0, 1.0, nv.ptr(sg["out"]), *sg["x"].shape)]
        nv.check(nv.lib().ltx2_stg_euler_step_pair(*args, SIGMA, SIGMA_NEXT, nv.stream()))


# ------------------------------------------------------------------ the tiny AudioVideo model
F, H, W, S, LAYERS, BLOCKS = 2, 2, 3, 24, 3, [1]
N = F * H * W


class Tiny:
    pass


@pytest.fixture(scope="module")
def tiny(dev):
    from oracle import dit_av, loop
    from ltx_2_mlx_amd.components import LTX2Scheduler
    from ltx_2_mlx_amd.types import AudioLatentShape, VideoPixelShape
    t = Tiny()
    t.cfg, t.w, t.wq, t.m = make_av(dev, False, layers=LAYERS, seed=23)
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
    t.sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
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


# ------------------------------------------------------------------ 2. the step entry
@pytest.mark.parametrize("masked", [False, True], ids=["uniform", "image-mask"])
@pytest.mark.parametrize("with_neg", [True, False], ids=["cfg", "no-cfg"])
def test_stg_step_joint_av_equals_its_parts(dev, tiny, with_neg, masked):
    """stg_step_joint_av_ == forward_av(ctx), forward_av(neg), forward_perturbed_av(ctx), ltx2_stg_euler_step_pair called one by one: the same
    kernels in the same order, so the same bits on both latents.  Two chained steps; both modalities STG-guided, then each one alone."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.pipelines.common import audio_modality_from_state, joint_stg_perturbations, modality_from_state
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights() if with_neg else None
    vctx, actx, nvctx, nactx = t.ctx
    vs, as_ = _states(t, dev, masked)
    mk = vs.denoise_mask[0].reshape(-1).contiguous() if masked else None
    cl = vs.clean_latent[0].contiguous() if masked else None
    cfg = (3.0, 7.0)
    for stg in ((1.5, 0.75), (0.0, 1.0), (1.0, 0.0)):
        want = [vs.latent[0].float().contiguous(), as_.latent[0].float().contiguous()]
        got = [w.clone() for w in want]
        scratch = [torch.full_like(w, SENTINEL) for w in want]
        for s, sn in ((t.sig[0], t.sig[1]), (t.sig[1], t.sig[2])):
            mods = lambda lats, vc, ac: (modality_from_state(vs.replace(latent=lats[0][None]), vc, s, uniform=not masked),      # noqa: E731
                                         audio_modality_from_state(as_.replace(latent=lats[1][None]), ac, s, uniform=True))
            cond = [c[0].clone() for c in m(*mods(want, vctx, actx))]
            unc = [u[0].clone() for u in neg(*mods(want, nvctx, nactx))] if with_neg else [None, None]
            pert = [p[0].clone() for p in m(*mods(want, vctx, actx), perturbations=joint_stg_perturbations(BLOCKS, stg[0] != 0, stg[1] != 0))]
            assert not torch.equal(pert[0], cond[0]) and not torch.equal(pert[1], cond[1])       # each modality sees the other's skip through the cross-modal attention
            segs = [dict(x=want[k], vel_cond=cond[k], vel_uncond=unc[k], vel_perturbed=pert[k] if stg[k] != 0 else None,
                         timesteps=(mk * s) if (masked and k == 0) else torch.tensor([s], device=dev), mask=mk if k == 0 else None,
                         clean=cl if k == 0 else None, cfg_scale=cfg[k], stg_scale=stg[k]) for k in range(2)]
            want = list(K.stg_euler_step_pair(*segs, s, sn))
            for k in range(2):
                m.set_stg_blocks(BLOCKS if stg[k] != 0 else [], k)
            m.stg_step_joint_av_(neg, got[0], got[1], *mods(got, vctx, actx), s, sn, cfg[0], cfg[1], stg[0], stg[1], scratch[0], scratch[1], denoise_mask=mk,
                                 clean_latent=cl)
            torch.cuda.synchronize()
            for k in range(2):
                assert torch.equal(got[k], want[k]), f"stg={stg} modality {k}: {int((got[k] != want[k]).sum())} elements differ"
                assert torch.equal(scratch[k], pert[k])                                          # the caller's scratch holds the perturbed velocity
        assert all(bool(torch.isfinite(g).all()) for g in got) and not torch.equal(got[0], vs.latent[0]) and not torch.equal(got[1], as_.latent[0])
    for k in range(2):
        m.set_stg_blocks([], k)


# ------------------------------------------------------------------ 3. the loops
def _loop(t, dev, masked, model=None, cfg=(3.0, 7.0), stg=(1.0, 1.0), cutoff=0.5, **kw):
    from ltx_2_mlx_amd.components import CFGGuider, STGGuider
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import joint_stg_denoise_loop
    vs, as_ = _states(t, dev, masked)
    sg = [STGGuider(s) if s else None for s in stg]
    v, a = joint_stg_denoise_loop(X0Model(t.m if model is None else model), vs, as_, t.sig, t.ctx[0], t.ctx[1], t.ctx[2], t.ctx[3], CFGGuider(cfg[0]), CFGGuider(cfg[1]), sg[0], sg[1],
                                  BLOCKS, cutoff, **kw)
    return v.latent, a.latent


@pytest.mark.parametrize("masked", [False, True], ids=["uniform", "image-mask"])
def test_joint_stg_loop_device_form_against_eager_form(dev, tiny, masked):
    """joint_stg_denoise_loop(fused=True) against fused=False: 4 steps, cfg 3 / 7, stg 1 / 1, cutoff 0.5 -- two STG steps, then two guided
    ones.  The eager form runs the same forward entries but takes x0 and the Euler update from X0Model's and EulerDiffusionStep's kernels,
    whose arithmetic is contracted, so the two agree to rounding, not bit for bit: each modality inside 5 x the measured rel-L2.  Measured
    on the MI355X: see LOOP_MEASURED.  The callback form is the same device loop; cutoff 0 is the joint guided loop bit for bit, and
    cutoff 0.5 is neither that nor cutoff 1."""
    from ltx_2_mlx_amd.components import EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import joint_guided_denoise_loop
    t = tiny
    fused, eager = _loop(t, dev, masked), _loop(t, dev, masked, fused=False)
    ev = measure("joint STG loop, device vs eager form, video", rel_l2(fused[0], eager[0]))
    ea = measure("joint STG loop, device vs eager form, audio", rel_l2(fused[1], eager[1]))
    print(f"joint STG loop, fused vs eager ({'masked' if masked else 'uniform'}): video rel-L2 = {ev:.4e}  audio rel-L2 = {ea:.4e}")
    assert all(bool(torch.isfinite(x).all()) for x in fused + eager)
    assert ev <= 5 * LOOP_MEASURED[0] and ea <= 5 * LOOP_MEASURED[1]
    seen = []
    cb = _loop(t, dev, masked, callback=lambda i, n: seen.append((i, n)))
    assert torch.equal(cb[0], fused[0]) and torch.equal(cb[1], fused[1]) and seen == [(1, 4), (2, 4), (3, 4), (4, 4)]
    full, none = _loop(t, dev, masked, cutoff=1.0), _loop(t, dev, masked, cutoff=0.0)
    assert not torch.equal(fused[0], full[0]) and not torch.equal(fused[0], none[0]) and not torch.equal(fused[1], full[1]) and not torch.equal(fused[1], none[1])
    vs, as_ = _states(t, dev, masked)
    gv, ga = joint_guided_denoise_loop(X0Model(t.m), vs, as_, t.sig, *t.ctx, 3.0, 7.0, EulerDiffusionStep(), use_hip_graph=False)
    assert torch.equal(none[0], gv.latent) and torch.equal(none[1], ga.latent)                   # past the cutoff: guided_step_joint_av_ itself


# ------------------------------------------------------------------ 4. the audio STG term
def test_the_audio_stg_term_acts(dev, tiny):
    """stg_audio_scale 1 against 0 (cfg 3 / 7, video stg 1): the audio latent differs.
    The zeroed-weights identity of tests/test_stg_gpu.py, for the audio: on a model whose block-1 audio_attn1.to_out is zero, a perturbed
    pass that skips that audio self-attention alone IS the plain pass (x + gate * 0 = x), bit for bit.  The STG term is stg * (g - p) with
    g the CFG-guided prediction, so it vanishes exactly where g is the conditional prediction: the audio guider not enabled (scale 1: g =
    a + 0 * (a - b)) and no video skip (a video skip reaches the audio through the cross-modal attention).  There audio STG 1 equals audio
    STG 0 -- the joint guided loop -- bit for bit on both latents; on the unmodified weights the same two runs differ."""
    from ltx_2_mlx_amd.components import EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import LTXModel, LTXModelType, X0Model
    from ltx_2_mlx_amd.pipelines.common import joint_guided_denoise_loop
    t = tiny
    with_a, without_a = _loop(t, dev, False, stg=(1.0, 1.0)), _loop(t, dev, False, stg=(1.0, 0.0))
    assert not torch.equal(with_a[1], without_a[1]) and bool(torch.isfinite(with_a[1]).all())
    measure("audio latent, stg_audio_scale 1 vs 0", rel_l2(with_a[1], without_a[1]))
    mz = LTXModel(model_type=LTXModelType.AudioVideo, num_attention_heads=4, attention_head_dim=128, num_layers=LAYERS, caption_channels=t.cfg.caption_channels,
                  audio_attention_heads=4, device=dev)
    mz.load_state_dict(R.zero_self_attn_out(t.w, BLOCKS, LAYERS, prefix="audio_attn1"))
    for model, same in ((mz, True), (t.m, False)):
        a1 = _loop(t, dev, False, model=model, cfg=(3.0, 1.0), stg=(0.0, 1.0), cutoff=1.0)
        vs, as_ = _states(t, dev, False)
        gv, ga = joint_guided_denoise_loop(X0Model(model), vs, as_, t.sig, *t.ctx, 3.0, 1.0, EulerDiffusionStep(), use_hip_graph=False)
        assert (torch.equal(a1[0], gv.latent) and torch.equal(a1[1], ga.latent)) == same, f"zeroed={same}: {int((a1[1] != ga.latent).sum())} audio elements differ"
        assert same or not torch.equal(a1[1], ga.latent)


# ------------------------------------------------------------------ 5. refusals
def test_stg_step_joint_av_refusals(dev, tiny):
    """Every refusal stands before anything is launched: the latents keep their bits."""
    from ltx_2_mlx_amd import _native as nv
    t, m = tiny, tiny.m
    neg = m.clone_sharing_weights()
    vctx, actx, nvctx, nactx = t.ctx
    for c, (vc, ac) in ((m, (vctx, actx)), (neg, (nvctx, nactx))):
        c.prepare(vc, t.vpos.to(dev), audio_context=ac, audio_positions=t.apos.to(dev))
    for k in range(2):
        m.set_stg_blocks(BLOCKS, k)
    lat, alat = t.vnoise[0].to(dev).contiguous(), t.anoise[0].to(dev).contiguous()
    keep = lat.clone(), alat.clone()
    ts = torch.tensor([0.5], device=dev)
    vp, ap = torch.empty_like(lat), torch.empty_like(alat)
    L = nv.lib()

    def call(ctx=m._h, ng=neg._h, vp=vp, n_vp=None, ap=ap, n_ap=None, stg=(1.0, 1.0), sigma=0.5, mask=None, clean=None):
        nv.check(L.ltx2_dit_stg_step_joint_av(ctx, ng, nv.ptr(lat), nv.ptr(alat), nv.ptr(ts), 1, nv.ptr(ts), 1, nv.ptr(ts), nv.ptr(mask), nv.ptr(clean), None, None,
                                              nv.ptr(vp), (0 if vp is None else vp.numel()) if n_vp is None else n_vp, nv.ptr(ap),
                                              (0 if ap is None else ap.numel()) if n_ap is None else n_ap, 3.0, 7.0, stg[0], stg[1], sigma, 0.25, nv.stream()))

    with pytest.raises(ValueError, match="perturbed scratch of 1408 elements"):
        call(n_vp=lat.numel() - 128)                                               # a scratch of another length would be written out of bounds
    with pytest.raises(ValueError, match="modality 1 has 9 tokens"):
        call(ap=vp, n_ap=vp.numel())
    with pytest.raises(ValueError, match="both required"):
        call(ap=None)
    m.set_stg_blocks([], 1)
    with pytest.raises(ValueError, match="no audio self-attention is marked"):
        call()
    call(stg=(1.0, 0.0))                                                           # ... and is no refusal while the audio is not STG-guided
    assert not torch.equal(lat, keep[0])
    lat.copy_(keep[0])
    alat.copy_(keep[1])
    m._put_stg_flags(1, bytes(LAYERS))                                             # an all-zero flag array is an empty set too
    with pytest.raises(ValueError, match="no audio self-attention is marked"):
        call()
    m.set_stg_blocks(BLOCKS, 1)
    with pytest.raises(ValueError, match="ltx2_dit_guided_step_joint_av"):
        call(stg=(0.0, 0.0))
    with pytest.raises(ValueError, match="ctx == neg"):
        call(ng=m._h)
    twin = m._video_twin()
    with pytest.raises(ValueError, match="AudioVideo"):
        call(ctx=twin._h, ng=None)
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        call(sigma=0.0)
    with pytest.raises(ValueError, match="mask and clean go together"):
        call(mask=torch.ones(N, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(lat, keep[0]) and torch.equal(alat, keep[1])
    for k in range(2):
        m.set_stg_blocks([], k)


# ------------------------------------------------------------------ 6. the pipeline
def test_one_stage_pipeline_with_audio_stg(dev, tiny):
    """OneStagePipeline on the AudioVideo model with plain CFG 3 / 7, stg_scale 1 and stg_audio_scale 1, 4 steps: the device loop, both latents
    against tests/stg_joint_ref.stg_joint_loop on the fp32 oracle (the perturbed pass on weights with block 1's attn1 and audio_attn1
    out-projections zeroed).  Each modality inside 5 x the measured rel-L2: see PIPE_MEASURED.  CFG* beside stg_audio_scale is refused by
    name, and so is stg_audio_scale without an audio state."""
    from oracle import dit_av, loop
    from ltx_2_mlx_amd.components import AudioPatchifier, CFGGuider
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    from ltx_2_mlx_amd.types import AudioLatentShape
    t = tiny
    sig = [float(s) for s in loop.ltx2_scheduler(4)]

    def x0(vc, ac, ww):
        def f(v, a, s):
            ts = torch.tensor([s])
            return dit_av.av_x0_model(dict(latent=v, context=vc, timesteps=ts, sigma=ts, positions=t.vpos),
                                      dict(latent=a, context=ac, timesteps=ts, sigma=ts, positions=t.apos), ww, t.cfg)
        return f
    wz = R.zero_self_attn_out(R.zero_self_attn_out(t.wq, BLOCKS, LAYERS, prefix="attn1"), BLOCKS, LAYERS, prefix="audio_attn1")
    rv, ra = JR.stg_joint_loop(t.vnoise, t.anoise, x0(t.vctx, t.actx, t.wq), x0(t.nvctx, t.nactx, t.wq), x0(t.vctx, t.actx, wz), sig, CFGGuider(3.0).guide,
                               CFGGuider(7.0).guide, 1.0, 1.0, 1.0)
    pipe = OneStagePipeline(t.m, None, None)
    base = dict(height=64, width=96, num_frames=9, seed=1, fps=25.0, num_inference_steps=4, cfg_scale=3.0, audio_cfg_scale=7.0, audio_enabled=True)
    conf = OneStageCFGConfig(rescale_scale=0.0, **base)
    vctx, actx, nvctx, nactx = t.ctx
    kw = dict(positive_audio_encoding=actx, negative_audio_encoding=nactx, initial_noise=t.vnoise.to(dev), initial_audio_noise=t.anoise.to(dev))
    lat, aud = pipe(vctx, nvctx, conf, stg_scale=1.0, stg_audio_scale=1.0, stg_blocks=BLOCKS, **kw)
    ev = measure("one-stage joint, STG 1 / 1, video latent vs stg_joint_ref", rel_l2(lat.cpu(), loop.unpatchify(rv, F, H, W)))
    ea = measure("one-stage joint, STG 1 / 1, audio latent vs stg_joint_ref", rel_l2(aud.cpu(), AudioPatchifier(patch_size=1).unpatchify(ra, AudioLatentShape(1, 8, t.na, 16))))
    print(f"pipeline, joint STG 1 / 1: video rel-L2 = {ev:.4e}  audio rel-L2 = {ea:.4e}")
    assert ev <= 5 * PIPE_MEASURED[0] and ea <= 5 * PIPE_MEASURED[1]
    # the audio scale reaches the loop: scale 0 is another audio latent, and the audio scale alone runs too
    lat0, aud0 = pipe(vctx, nvctx, conf, stg_scale=1.0, stg_blocks=BLOCKS, **kw)
    assert not torch.equal(aud0, aud) and not torch.equal(lat0, lat)
    lat1, aud1 = pipe(vctx, nvctx, conf, stg_audio_scale=1.0, stg_blocks=BLOCKS, **kw)
    assert bool(torch.isfinite(aud1).all()) and not torch.equal(aud1, aud) and not torch.equal(aud1, aud0)
    with pytest.raises(NotImplementedError, match="stg_audio_scale"):
        pipe(vctx, nvctx, OneStageCFGConfig(rescale_scale=0.7, **base), stg_scale=1.0, stg_audio_scale=1.0, stg_blocks=BLOCKS, **kw)
    with pytest.raises(ValueError, match="stg_audio_scale > 0 needs an audio state"):
        OneStagePipeline(t.m._video_twin(), None, None)(vctx, nvctx, OneStageCFGConfig(**dict(base, audio_enabled=False, rescale_scale=0.0)), stg_audio_scale=1.0,
                                                        initial_noise=t.vnoise.to(dev))
