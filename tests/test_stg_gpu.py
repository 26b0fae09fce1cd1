"""Spatio-temporal guidance on the GPU: the STG Euler kernel bit for bit, the engine's self-attention skip against a model whose attn1.to_out
is zero (bit for bit) and against the fp32 oracle, the one-call step and the captured loop against the same kernels called one by one, and
OneStagePipeline / generate_video against tests/stg_ref.  Tiny models: 3 layers, 2 heads x 128, caption 128, N = 70 (stg_ref.tiny_video);
the AudioVideo engine as tests/test_parity.make_av builds it (2 layers, 4 + 4 heads, N = 70, Na = 37)."""
import os
import sys

import pytest
import torch

from conftest import measure, rel_l2

import stg_ref as R
from test_parity import make_av

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0

# rel-L2 against the fp32 restatement, measured on the MI355X; every gate is 5 x its figure.  R.ENGINE_MEASURED: the
# perturbed velocity (shared with the non-vacuity check of test_stg_cpu)
FOLD_MEASURED = 3.323e-3            # perturbed velocity at D = 4096, N = 2023, default options (the norm fold on the layer that keeps its self-attention)
PIPE_CFG_MEASURED = 3.928e-3         # OneStagePipeline, video-only, plain CFG: the fused loop
PIPE_STAR_MEASURED = 3.680e-3        # the same under the default CFG*: the eager loop
PIPE_AV_MEASURED = (5.817e-3, 1.667e-3)  # joint audio+video: video latent, audio latent


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("rows,C", [(1, 128), (37, 128), (64, 8)])
def test_stg_euler_step_bit_for_bit(dev, rows, C):
    from ltx_2_mlx_amd import kernels as K
    g = torch.Generator().manual_seed(rows * 131 + C)
    x, vc, vu, vp, clean = (torch.randn(rows, C, generator=g) for _ in range(5))
    ts_row = torch.rand(rows, generator=g)
    mask = torch.ones(rows)
    mask[::3] = 0.0
    mask[1::3] = 0.05
    n = rows * C
    sigma, sigma_next, cfg, stg = 0.909375, 0.725, 3.0, 1.5
    d = lambda t: None if t is None else t.to(dev)
    for ts in (torch.tensor([0.909375]), ts_row):                                     # ts_stride 0 / 1
        for mk in (None, mask):
            for u in (None, vu):
                cl = clean if mk is not None else None
                ref = R.stg_euler_step(x, vc, u, vp, ts, mk, cl, cfg, stg, sigma, sigma_next)
                buf = torch.full((n + 64,), SENTINEL, device=dev)
                out = buf[:n].view(rows, C)
                K.stg_euler_step(d(x), d(vc), d(u), d(vp), d(ts), cfg, stg, sigma, sigma_next, mask=d(mk), clean=d(cl), out=out)
                tag = f"ts{ts.numel()} mask{mk is not None} vu{u is not None}"
                assert torch.equal(out.cpu(), ref), f"{tag}: {int((out.cpu() != ref).sum())} of {n} elements differ"
                assert bool((buf[n:] == SENTINEL).all()), tag                         # nothing past rows * C
                xbuf = torch.full((n + 64,), SENTINEL, device=dev)                    # out aliasing x: the same bits
                xin = xbuf[:n].view(rows, C)
                xin.copy_(x)
                K.stg_euler_step(xin, d(vc), d(u), d(vp), d(ts), cfg, stg, sigma, sigma_next, mask=d(mk), clean=d(cl), out=xin)
                assert torch.equal(xin.cpu(), ref) and bool((xbuf[n:] == SENTINEL).all()), tag
            # stg = 0: the guided step's bits
            a = K.stg_euler_step(d(x), d(vc), d(vu), d(vp), d(ts), cfg, 0.0, sigma, sigma_next, mask=d(mk), clean=d(clean if mk is not None else None))
            b = K.guided_euler_step(d(x), d(vc), d(vu), d(ts), cfg, sigma, sigma_next, mask=d(mk), clean=d(clean if mk is not None else None))
            assert torch.equal(a, b)
    if rows == 37:
        with pytest.raises(ValueError, match="Sigma can't be 0.0"):
            K.stg_euler_step(d(x), d(vc), d(vu), d(vp), torch.tensor([0.5], device=dev), cfg, stg, 0.0, 0.5)
        # one operand 4 bytes off a 16-byte boundary: the element-wise form, the same bits
        off = torch.full((n + 65,), SENTINEL, device=dev)
        vpo = off[1:1 + n].view(rows, C)
        vpo.copy_(vp)
        assert vpo.data_ptr() % 16 == 4
        got = K.stg_euler_step(d(x), d(vc), d(vu), vpo, d(ts_row), cfg, stg, sigma, sigma_next, mask=d(mask), clean=d(clean))
        assert torch.equal(got.cpu(), R.stg_euler_step(x, vc, vu, vp, ts_row, mask, clean, cfg, stg, sigma, sigma_next))


# ------------------------------------------------------------------ 2. the engine's skip
class Tiny:
    pass


def _model(dev, w):
    from ltx_2_mlx_amd.model.transformer import LTXModel
    m = LTXModel(num_attention_heads=R.HEADS, attention_head_dim=128, num_layers=R.LAYERS, caption_channels=R.CAP, device=dev)
    m.load_state_dict(w)
    return m


@pytest.fixture(scope="module")
def tiny(dev):
    t = Tiny()
    t.cfg, t.w, t.wq, t.lat, t.ctx, t.nctx, t.pos = R.tiny_video()
    t.m = _model(dev, t.w)
    return t


def _mod(dev, lat, ctx, pos, ts):
    from ltx_2_mlx_amd.model.transformer import Modality
    return Modality(latent=lat.to(dev), context=ctx.to(dev), context_mask=None, timesteps=ts.to(dev), positions=pos.to(dev))


def _stg_config(blocks, kind="video"):
    from ltx_2_mlx_amd.components import BatchedPerturbationConfig, Perturbation, PerturbationConfig, PerturbationType as PT
    kinds = {"video": [PT.SKIP_VIDEO_SELF_ATTN], "audio": [PT.SKIP_AUDIO_SELF_ATTN], "both": [PT.SKIP_VIDEO_SELF_ATTN, PT.SKIP_AUDIO_SELF_ATTN]}[kind]
    return BatchedPerturbationConfig([PerturbationConfig([Perturbation(k, blocks) for k in kinds])])


@pytest.mark.parametrize("name", list(R.SKIP_SETS))
def test_engine_skip_video_only(dev, tiny, name):
    """fold_norms = 0: the perturbed forward == an ordinary forward of a model whose attn1.to_out of the skipped blocks is zero, bit for bit
    (x + gate * 0 = x).  Default options: against the fp32 oracle on such weights.  The empty set == ltx2_dit_forward, bit for bit."""
    from oracle import dit
    t, blocks = tiny, R.SKIP_SETS[name]
    ts = torch.tensor([R.SIGMA])
    mod = _mod(dev, t.lat, t.ctx, t.pos, ts)
    plain = t.m(mod).clone()
    got = t.m(mod, perturbations=_stg_config(blocks)).clone()
    ref = dit.velocity_model(t.lat, t.ctx, ts, t.pos, R.zero_self_attn_out(t.wq, blocks, R.LAYERS), t.cfg)
    err = measure(f"perturbed velocity vs fp32 oracle [{name}]", rel_l2(got.cpu(), ref))
    print(f"engine skip {name}: rel-L2 = {err:.4e}")
    assert err <= R.ENGINE_GATE
    if name == "none":
        from ltx_2_mlx_amd import _native as nv
        from ltx_2_mlx_amd.components import BatchedPerturbationConfig
        assert torch.equal(got, plain)                                                # an empty config is the plain forward
        assert torch.equal(t.m(mod, perturbations=BatchedPerturbationConfig.empty(1)), plain)
        # the perturbed ENTRY itself with an empty set: cleared (NULL), then an all-zero flag array -- ltx2_dit_forward's bits
        lat, tsd = t.lat[0].to(dev).contiguous(), ts.to(dev)

        def perturbed():
            out = torch.full_like(plain[0], SENTINEL)
            nv.check(t.m._L.ltx2_dit_forward_perturbed(t.m._h, nv.ptr(lat), nv.ptr(tsd), 1, None, nv.ptr(out), nv.stream()))
            return out[None]
        t.m.set_stg_blocks([])
        assert t.m._stg[0] is None and torch.equal(perturbed(), plain)
        t.m._put_stg_flags(0, bytes(R.LAYERS))
        assert torch.equal(perturbed(), plain)
        t.m.set_stg_blocks([1])                                                       # (the entry does read the set)
        assert not torch.equal(perturbed(), plain)
        t.m.set_stg_blocks([])
        return
    assert rel_l2(got.cpu(), plain.cpu()) >= 10 * R.ENGINE_GATE                       # the skip is seen
    zeroed = _model(dev, R.zero_self_attn_out(t.w, blocks, R.LAYERS))
    for m in (t.m, zeroed):
        m.set_option("fold_norms", 0)
    try:
        a = t.m(mod, perturbations=_stg_config(blocks))
        b = zeroed(mod)
        assert torch.equal(a, b), f"{int((a != b).sum())} elements differ"
    finally:
        t.m.set_option("fold_norms", 1)
    assert torch.equal(t.m(mod), plain)                                               # the plain forward ignores the stored set
    # set_stg_blocks + the C entry directly: the same as the config; a config holds for its own call and leaves the stored set alone
    from ltx_2_mlx_amd import _native as nv
    t.m.set_stg_blocks(blocks)
    kept = t.m._stg[0]
    other = [2] if blocks != [2] else [0]
    assert not torch.equal(t.m(mod, perturbations=_stg_config(other)), got) and t.m._stg[0] == kept
    out = torch.empty_like(got[0])
    lat = t.lat[0].to(dev).contiguous()
    nv.check(t.m._L.ltx2_dit_forward_perturbed(t.m._h, nv.ptr(lat), nv.ptr(ts.to(dev)), 1, None, nv.ptr(out), nv.stream()))
    assert torch.equal(out[None], got)
    with pytest.raises(ValueError, match="out of range"):
        t.m.set_stg_blocks([R.LAYERS])


def test_engine_skip_with_the_norm_fold(dev):
    """Full width (D = 4096, 2 layers), N = 7 x 17 x 17 = 2023 rows (no multiple of a tile): here the GEMMs run on the kernels that fold the
    text cross-attention's pre-norm.  Block 0 is skipped, so it has no producer and runs its norm as a pass of its own, while block 1 keeps
    the fold.  Against the fp32 oracle (run on the GPU) on weights with block 0's attn1.to_out zeroed; the fold really ran (not the bits of
    fold_norms = 0) and agrees with the unfolded engine inside the same gate."""
    from oracle import dit, loop
    from test_parity import make_dit
    cfg, wq, m = make_dit(dev, heads=32, layers=2, cap=128, seed=61)
    g = torch.Generator().manual_seed(99)
    lat = torch.randn(1, 2023, 128, generator=g)
    ctx = 0.1 * torch.randn(1, 64, 128, generator=g)
    pos = loop.video_positions(1, 7, 17, 17, 24.0)
    ts = torch.tensor([R.SIGMA])
    mod = _mod(dev, lat, ctx, pos, ts)
    plain = m(mod).clone()
    got = m(mod, perturbations=_stg_config([0])).clone()
    with torch.device(dev), torch.no_grad():
        wz = {k: v.to(dev) for k, v in R.zero_self_attn_out(wq, [0], 2).items()}
        ref = dit.velocity_model(lat.to(dev), ctx.to(dev), ts.to(dev), pos.to(dev), wz, cfg).cpu()
    err = measure("perturbed velocity vs fp32 oracle, D = 4096, N = 2023, the fold on block 1", rel_l2(got.cpu(), ref))
    print(f"engine skip with the fold: rel-L2 = {err:.4e}")
    assert err <= 5 * FOLD_MEASURED
    m.set_option("fold_norms", 0)
    unfolded = m(mod, perturbations=_stg_config([0])).clone()
    plain0 = m(mod).clone()
    m.set_option("fold_norms", 1)
    assert not torch.equal(plain, plain0)                                             # this geometry folds
    assert not torch.equal(got, unfolded) and rel_l2(got.cpu(), unfolded.cpu()) <= 5 * FOLD_MEASURED
    assert measure("perturbed vs plain velocity, D = 4096", rel_l2(got.cpu(), plain.cpu())) > 5 * err          # the skip is seen


@pytest.mark.parametrize("kind", ["video", "audio", "both"])
def test_engine_skip_audio_video(dev, kind):
    """The AudioVideo engine (two streams, event joins): the perturbed forward == the ordinary forward of a model with the skipped blocks'
    attn1 / audio_attn1 to_out zeroed, bit for bit on both outputs -- no join was lost."""
    from oracle import dit_av, loop
    from ltx_2_mlx_amd.model.transformer import LTXModel, LTXModelType, Modality
    cfg, w, wq, m = make_av(dev, False, seed=5)
    blocks = {"video": [0], "audio": [1], "both": None}[kind]
    wz = dict(w)
    for pre in {"video": ["attn1"], "audio": ["audio_attn1"], "both": ["attn1", "audio_attn1"]}[kind]:
        wz = R.zero_self_attn_out(wz, blocks, cfg.num_layers, prefix=pre)
    mz = LTXModel(model_type=LTXModelType.AudioVideo, num_attention_heads=4, attention_head_dim=128, num_layers=cfg.num_layers,
                  caption_channels=cfg.caption_channels, audio_attention_heads=4, device=dev)
    mz.load_state_dict(wz)
    g = torch.Generator().manual_seed(3)
    f, h, wd, Ta, S = 2, 5, 7, 37, 50
    vlat, alat = torch.randn(1, f * h * wd, 128, generator=g), torch.randn(1, Ta, 128, generator=g)
    vctx, actx = 0.1 * torch.randn(1, S, cfg.caption_channels, generator=g), 0.1 * torch.randn(1, S, cfg.caption_channels, generator=g)
    vpos, apos = loop.video_positions(1, f, h, wd, 24.0), dit_av.audio_positions(1, Ta)
    s = torch.tensor([R.SIGMA], device=dev)
    mv = Modality(latent=vlat.to(dev), context=vctx.to(dev), context_mask=None, timesteps=s, positions=vpos.to(dev), sigma=s)
    ma = Modality(latent=alat.to(dev), context=actx.to(dev), context_mask=None, timesteps=s, positions=apos.to(dev), sigma=s)
    pv, pa = m(mv, ma)
    pv, pa = pv.clone(), pa.clone()
    gv, ga = m(mv, ma, perturbations=_stg_config(blocks, kind))
    zv, za = mz(mv, ma)
    assert torch.equal(gv, zv) and torch.equal(ga, za), f"{int((gv != zv).sum())} video, {int((ga != za).sum())} audio elements differ"
    assert not torch.equal(gv, pv) and not torch.equal(ga, pa)                       # each modality sees the other through the cross-modal attention
    v2, a2 = m(mv, ma)
    assert torch.equal(v2, pv) and torch.equal(a2, pa)                               # the plain forward ignores the stored sets
    # the perturbed ENTRY with both sets empty -- cleared (NULL), then all-zero flag arrays: ltx2_dit_forward_av's bits on both outputs
    from ltx_2_mlx_amd import _native as nv
    vl, al = vlat[0].to(dev).contiguous(), alat[0].to(dev).contiguous()

    def perturbed():
        ov, oa = torch.full_like(pv[0], SENTINEL), torch.full_like(pa[0], SENTINEL)
        nv.check(m._L.ltx2_dit_forward_perturbed_av(m._h, nv.ptr(vl), nv.ptr(s), 1, nv.ptr(s), nv.ptr(al), nv.ptr(s), 1, nv.ptr(s), nv.ptr(ov), nv.ptr(oa),
                                                    nv.stream()))
        return ov[None], oa[None]
    assert m._stg == {0: None, 1: None}                                              # the config above held for its own call
    for flags in (None, bytes(cfg.num_layers)):
        m._put_stg_flags(0, flags)
        m._put_stg_flags(1, flags)
        ev, ea = perturbed()
        assert torch.equal(ev, pv) and torch.equal(ea, pa), flags
    m.set_stg_blocks(blocks, 0 if kind != "audio" else 1)                            # (the entry does read the sets)
    ev, ea = perturbed()
    assert not torch.equal(ev, pv)
    m.set_stg_blocks([], 0)
    m.set_stg_blocks([], 1)
    from ltx_2_mlx_amd.components import BatchedPerturbationConfig, Perturbation, PerturbationConfig, PerturbationType as PT
    if kind == "both":
        for bad in (PT.SKIP_A2V_CROSS_ATTN, PT.SKIP_V2A_CROSS_ATTN):
            with pytest.raises(NotImplementedError, match=bad.name):
                m(mv, ma, perturbations=BatchedPerturbationConfig([PerturbationConfig([Perturbation(bad, [0])])]))
        with pytest.raises(ValueError, match="batch must be 1"):
            m(mv, ma, perturbations=BatchedPerturbationConfig.empty(2))


# ------------------------------------------------------------------ 3. fused = eager = captured
def _state(t, dev, masked):
    from ltx_2_mlx_amd.types import LatentState
    mask = torch.ones(1, t.lat.shape[1], 1)
    if masked:                                                                        # an image-conditioned state: the first frame's tokens are given
        mask[0, :35] = 0.0
    clean = torch.zeros_like(t.lat) if not masked else torch.where(mask == 0, t.lat * 0.5, torch.zeros_like(t.lat))
    return LatentState(latent=t.lat.clone().to(dev), denoise_mask=mask.to(dev), positions=t.pos.to(dev), clean_latent=clean.to(dev))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("with_neg", [True, False])
def test_stg_step_and_captured_loop(dev, tiny, masked, with_neg):
    """stg_step_ == forward x 3 + ltx2_stg_euler_step, bit for bit; the captured loop (4 steps, cutoff 0.5: two STG steps, then two guided or
    plain ones, in one graph) == the per-step loop, bit for bit."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep, LTX2Scheduler, STGGuider
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import guided_denoise_loop, modality_from_state, stg_denoise_loop
    t, m = tiny, tiny.m
    st = _state(t, dev, masked)
    ctx, nctx = t.ctx.to(dev), t.nctx.to(dev)
    sigma, sigma_next, cfg, stg = 0.909375, 0.725, 3.0, 1.5
    neg = m.clone_sharing_weights() if with_neg else None
    mod = lambda c: modality_from_state(st, c, sigma, uniform=not masked)
    vc = m(mod(ctx))[0].clone()
    vu = neg(mod(nctx))[0].clone() if with_neg else None
    vp = m(mod(ctx), perturbations=_stg_config([1]))[0].clone()
    assert float((vc - vp).abs().max()) > 1e-3
    lat = st.latent[0].float().contiguous()
    mk = st.denoise_mask[0].reshape(-1).float().contiguous() if masked else None
    cl = st.clean_latent[0].float().contiguous() if masked else None
    ts = mod(ctx).timesteps.reshape(-1)
    want = K.stg_euler_step(lat, vc, vu, vp, ts, cfg, stg, sigma, sigma_next, mask=mk, clean=cl)
    got = lat.clone()
    m.set_stg_blocks([1])
    if with_neg:
        neg.prepare(nctx, st.positions, per_token=masked)
    m.stg_step_(neg, got, mod(ctx), sigma, sigma_next, cfg, stg, torch.empty_like(got), denoise_mask=mk, clean_latent=cl)
    assert torch.equal(got, want), f"{int((got != want).sum())} elements differ"
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, lat)
    # the loop
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    x0m = X0Model(m)
    guider = CFGGuider(cfg if with_neg else 1.0)
    run = lambda **kw: stg_denoise_loop(x0m, _state(t, dev, masked), sig, ctx, nctx if with_neg else None, guider, STGGuider(stg), [1], 0.5,
                                        EulerDiffusionStep(), **kw).latent
    seen = []
    graph, eager = run(use_hip_graph=True), run(use_hip_graph=False)
    cb = run(use_hip_graph=True, callback=lambda i, n: seen.append((i, n)))
    assert torch.equal(graph, eager) and torch.equal(cb, eager) and seen == [(1, 4), (2, 4), (3, 4), (4, 4)]
    assert bool(torch.isfinite(graph).all())
    # cutoff 0.5 is neither all STG steps nor none; cutoff 0 is the guided loop
    full = stg_denoise_loop(x0m, _state(t, dev, masked), sig, ctx, nctx if with_neg else None, guider, STGGuider(stg), [1], 1.0, EulerDiffusionStep()).latent
    none = stg_denoise_loop(x0m, _state(t, dev, masked), sig, ctx, nctx if with_neg else None, guider, STGGuider(stg), [1], 0.0, EulerDiffusionStep()).latent
    plain = guided_denoise_loop(x0m, _state(t, dev, masked), sig, ctx, nctx if with_neg else None, guider, EulerDiffusionStep()).latent
    assert not torch.equal(graph, full) and not torch.equal(graph, none)
    if with_neg:
        assert torch.equal(none, plain)                                               # the same captured guided steps
    else:
        assert rel_l2(none, plain) < 1e-5                                             # the plain step's contracted arithmetic, graph or eager


def test_stg_step_refusals(dev, tiny):
    from ltx_2_mlx_amd import _native as nv
    t, m = tiny, tiny.m
    m.prepare(t.ctx.to(dev), t.pos.to(dev))
    lat = t.lat[0].to(dev).contiguous()
    ts = torch.tensor([0.5], device=dev)
    L = nv.lib()
    with pytest.raises(ValueError, match="vel_perturbed"):
        nv.check(L.ltx2_dit_stg_step(m._h, None, nv.ptr(lat), nv.ptr(ts), 1, None, None, None, None, 3.0, 1.0, 0.5, 0.25, nv.stream()))
    with pytest.raises(ValueError, match="ctx == neg"):
        nv.check(L.ltx2_dit_stg_step(m._h, m._h, nv.ptr(lat), nv.ptr(ts), 1, None, None, None, nv.ptr(lat.clone()), 3.0, 1.0, 0.5, 0.25, nv.stream()))
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        nv.check(L.ltx2_dit_stg_step(m._h, None, nv.ptr(lat), nv.ptr(ts), 1, None, None, None, nv.ptr(lat.clone()), 3.0, 1.0, 0.0, 0.25, nv.stream()))
    with pytest.raises(ValueError, match="n_layers"):
        nv.check(L.ltx2_dit_set_stg_blocks(m._h, 0, bytes(2), 2))
    with pytest.raises(ValueError, match="modality"):
        nv.check(L.ltx2_dit_set_stg_blocks(m._h, 1, bytes(R.LAYERS), R.LAYERS))          # a VideoOnly context has no audio modality
    with torch.cuda.stream(torch.cuda.Stream()):
        with pytest.raises(ValueError, match="vel_perturbed has"):
            m.capture_stg_graph(None, lat.clone(), [1.0, 0.5, 0.0], 3.0, 1.0, torch.empty(10, 128, device=dev))
    with pytest.raises(RuntimeError, match="no STG graph"):
        tiny.m.clone_sharing_weights().replay_stg_graph()


# ------------------------------------------------------------------ 4. the pipeline
H, W, F, STEPS, S = 64, 96, 17, 4, 24
GRID = (3, 2, 3)


@pytest.fixture(scope="module")
def pipe_case(tiny):
    from oracle import loop
    p = Tiny()
    g = torch.Generator().manual_seed(21)
    f, h, w = GRID
    p.noise = torch.randn(1, f * h * w, 128, generator=g)
    p.ctx = 0.1 * torch.randn(1, S, R.CAP, generator=g)
    p.nctx = 2.0 * torch.randn(1, S, R.CAP, generator=g)          # a tiny random DiT hardly listens to its prompt: a loud negative prompt
    p.pos = loop.video_positions(1, f, h, w, 25.0)
    p.sig = [float(s) for s in loop.ltx2_scheduler(STEPS)]
    p.kw = dict(height=H, width=W, num_frames=F, seed=1, fps=25.0, num_inference_steps=STEPS, audio_cfg_scale=1.0)
    return p


def _video_ref(t, p, guide, blocks, stg, cutoff):
    from oracle import dit, loop
    x0 = lambda c, ww: (lambda x, ts, s: dit.x0_model(x, c, torch.tensor([s]), p.pos, ww, t.cfg))
    mask, clean = torch.ones(1, p.noise.shape[1], 1), torch.zeros_like(p.noise)
    out = R.stg_loop(p.noise, mask, clean, x0(p.ctx, t.wq), x0(p.nctx, t.wq), x0(p.ctx, R.zero_self_attn_out(t.wq, blocks, R.LAYERS)), p.sig, guide, stg,
                     cutoff)
    return loop.unpatchify(out, *GRID)


def test_pipeline_video_only(dev, tiny, pipe_case):
    """OneStagePipeline on the video-only model, 4 steps, stg_scale 1.5, cutoff 0.5.  Plain CFG: the fused loop (graph and per-step agree bit
    for bit); the default CFG*: the eager loop.  Both against tests/stg_ref; stg_blocks=[1] differs from None."""
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    t, p = tiny, pipe_case
    pipe = OneStagePipeline(t.m, None, None)
    SC, stg = 3.0, 1.5
    run = lambda conf, **kw: pipe(p.ctx.to(dev), p.nctx.to(dev), conf, initial_noise=p.noise.to(dev), stg_scale=stg, stg_cutoff=0.5, **kw)[0]
    conf = dict(p.kw, cfg_scale=SC, rescale_scale=0.0)
    lat = run(OneStageCFGConfig(**conf), stg_blocks=[1])
    lat_g = run(OneStageCFGConfig(use_hip_graph=True, **conf), stg_blocks=[1])
    assert torch.equal(lat, lat_g)
    ref_one, ref_every = (_video_ref(t, p, CFGGuider(SC).guide, b, stg, 0.5) for b in ([1], None))
    err = measure("one-stage, plain CFG + STG (fused) vs stg_ref", rel_l2(lat.cpu(), ref_one))
    print(f"pipeline, plain CFG: rel-L2 = {err:.4e}")
    assert err <= 5 * PIPE_CFG_MEASURED
    every = run(OneStageCFGConfig(**conf), stg_blocks=None)
    err = measure("one-stage, plain CFG + STG in all blocks vs stg_ref", rel_l2(every.cpu(), ref_every))
    assert err <= 5 * PIPE_CFG_MEASURED
    # each run follows its own block set, and neither is the loop without STG
    assert rel_l2(every.cpu(), ref_one) > 10 * err and rel_l2(lat.cpu(), ref_every) > 10 * err
    plain = pipe(p.ctx.to(dev), p.nctx.to(dev), OneStageCFGConfig(**conf), initial_noise=p.noise.to(dev))[0]
    assert rel_l2(plain.cpu(), ref_one) > 10 * err
    # the config default: CFG* -- three evaluations and both guiders in torch
    conf = dict(p.kw, cfg_scale=SC, rescale_scale=0.7)
    star = run(OneStageCFGConfig(**conf), stg_blocks=[1])
    err = measure("one-stage, CFG* + STG (eager) vs stg_ref", rel_l2(star.cpu(), _video_ref(t, p, CFGStarRescalingGuider(SC).guide, [1], stg, 0.5)))
    print(f"pipeline, CFG*: rel-L2 = {err:.4e}")
    assert err <= 5 * PIPE_STAR_MEASURED
    # no guider enabled: two evaluations per STG step, no negative encoding needed
    solo = pipe(p.ctx.to(dev), None, OneStageCFGConfig(**dict(p.kw, cfg_scale=1.0, rescale_scale=0.0)), initial_noise=p.noise.to(dev), stg_scale=stg,
                stg_blocks=[1])[0]
    assert bool(torch.isfinite(solo).all()) and not torch.equal(solo, lat)


def test_pipeline_joint_audio_video(dev, pipe_case):
    """audio_enabled on the AudioVideo model: the eager joint loop, the perturbed evaluation on the positive contexts, only the video
    STG-guided.  Both latents against tests/stg_ref.stg_loop_av."""
    from oracle import dit_av, loop
    from ltx_2_mlx_amd.components import AudioPatchifier, CFGStarRescalingGuider
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    from ltx_2_mlx_amd.types import AudioLatentShape
    p = pipe_case
    cfg, w, wq, m = make_av(dev, False, seed=23)
    g = torch.Generator().manual_seed(22)
    Ta = AudioLatentShape.from_duration(1, F / 25.0).frames
    anoise = torch.randn(1, Ta, 128, generator=g)
    vctx, actx, nvctx, nactx = (0.1 * torch.randn(1, S, cfg.caption_channels, generator=g) for _ in range(4))
    apos = dit_av.audio_positions(1, Ta)
    stg, blocks = 8.0, [1]          # these weights (std 0.02) hardly feel one skipped self-attention: a large scale makes STG measurable

    def x0(vc, ac, ww):
        def f(v, a, s):
            ts = torch.tensor([s])
            return dit_av.av_x0_model(dict(latent=v, context=vc, timesteps=ts, sigma=ts, positions=p.pos),
                                      dict(latent=a, context=ac, timesteps=ts, sigma=ts, positions=apos), ww, cfg)
        return f
    gv, ga = CFGStarRescalingGuider(3.0), CFGStarRescalingGuider(7.0)
    rv, ra = R.stg_loop_av(p.noise, anoise, x0(vctx, actx, wq), x0(nvctx, nactx, wq), x0(vctx, actx, R.zero_self_attn_out(wq, blocks, cfg.num_layers)),
                           p.sig, gv.guide, ga.guide, stg, 0.5)
    pipe = OneStagePipeline(m, None, None)
    conf = OneStageCFGConfig(audio_enabled=True, **dict(p.kw, cfg_scale=3.0, audio_cfg_scale=7.0, rescale_scale=0.7))
    kw = dict(positive_audio_encoding=actx.to(dev), negative_audio_encoding=nactx.to(dev), initial_noise=p.noise.to(dev), initial_audio_noise=anoise.to(dev))
    lat, aud = pipe(vctx.to(dev), nvctx.to(dev), conf, stg_scale=stg, stg_blocks=blocks, stg_cutoff=0.5, **kw)
    ev = measure("one-stage joint, video latent vs stg_ref", rel_l2(lat.cpu(), loop.unpatchify(rv, *GRID)))
    ea = measure("one-stage joint, audio latent vs stg_ref", rel_l2(aud.cpu(), AudioPatchifier(patch_size=1).unpatchify(ra, AudioLatentShape(1, 8, Ta, 16))))
    print(f"pipeline, joint: video rel-L2 = {ev:.4e}  audio rel-L2 = {ea:.4e}")
    assert ev <= 5 * PIPE_AV_MEASURED[0] and ea <= 5 * PIPE_AV_MEASURED[1]
    plain, _ = pipe(vctx.to(dev), nvctx.to(dev), conf, **kw)
    assert rel_l2(plain.cpu(), loop.unpatchify(rv, *GRID)) > 5 * ev                   # STG moved the video


def test_generate_video_with_stg(dev, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    frames = generate.generate_video("a test prompt", generate_audio=True, stg_scale=1.0, stg_blocks=[0], use_gemma=False, num_steps=2, height=64,
                                     width=96, num_frames=9, seed=3, num_layers=2, num_heads=2, vae_base_channels=64, save_mp4=False,
                                     output_path=str(tmp_path / "s.mp4"))
    assert frames.dtype == torch.uint8 and frames.shape == (9, 64, 96, 3)
    assert "  STG guidance enabled (scale=1.0)" in capsys.readouterr().out.splitlines()
