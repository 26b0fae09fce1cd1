"""The Euler-ancestral sampler on the GPU: the Philox words against the numpy restatement, the normals against float64 Box-Muller on the same
bits and their statistics, the step kernels bit for bit against philox_normal + separate ops, and the loops (eager == fused == captured,
eta = 0 == the Euler loops, one captured graph for any seed).  Tiny models as tests/test_heun_gpu.py builds them."""
import numpy as np
import pytest
import torch

from conftest import measure

import ancestral_ref as R
from test_heun_gpu import _pipeline_states, _sigmas, _state, tiny, tiny_av  # noqa: F401  (the fixtures of the 64x96x9 models)

pytestmark = pytest.mark.gpu
SEEDS = [0, 42, 123456789012345]
SIGMA, SIGMA_NEXT = 0.909375, 0.725
NORMAL_MEASURED = 7.1e-7        # max |z_device - z_float64| over 2^20 values x 3 seeds, measured on the MI355X (see test_normals_...)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ 1. the noise
def test_bits_equal_the_restatement(dev):
    """ltx2_philox_bits == numpy Philox4x32-10, every word, over 1024 quads per (seed, step, stream); quad 0 of (seed 0, step 0, stream 0) is the
    first Random123 vector.  The entry takes no start offset, so the other two vectors and a quad index past 2^32 are checked on the
    restatement alone (tests/test_ancestral_cpu.py)."""
    from ltx_2_mlx_amd import kernels as K
    for seed in SEEDS:
        word = K.seed_word(seed, dev)
        for step in (0, 7):
            for stream in (0, 1):
                got = _u32(K.philox_bits(1024, word, step, stream))
                assert np.array_equal(got, R.quad_bits(0, 1024, seed, step, stream)), (seed, step, stream)
    assert tuple(int(v) for v in _u32(K.philox_bits(1, K.seed_word(0, dev), 0, 0))[0]) == R.KAT[0][2]
    neg = K.seed_word(0xFFFFFFFFFFFFFFFF, dev)          # the top bit of the seed reaches the key
    assert np.array_equal(_u32(K.philox_bits(4, neg, 1, 0)), R.quad_bits(0, 4, 0xFFFFFFFFFFFFFFFF, 1, 0))


@pytest.fixture(scope="module")
def device_normals(dev):
    from ltx_2_mlx_amd import kernels as K
    n = 1 << 20
    return {(s, st, sm): K.philox_normal(n, K.seed_word(s, dev), st, sm).cpu().numpy() for s in SEEDS for st, sm in ((0, 0), (1, 0), (0, 1))}


def test_normals_against_float64_on_the_same_bits(device_normals):
    """fp32 logf / sqrtf / sincospif and two products against float64 Box-Muller: a few fp32 ulp of |z| <= 5.8 (ulp 4.8e-7 in [4, 8)).  Measured
    on the MI355X: max abs error 7.1e-7 (seed 0; 6.0e-7 for the other two) over 2^20 values of each seed.  Gate: 5 x that."""
    worst = 0.0
    for seed in SEEDS:
        z = device_normals[(seed, 0, 0)]
        assert np.isfinite(z).all()
        worst = max(worst, measure(f"philox_normal seed={seed}: max abs error vs float64", float(np.abs(z.astype(np.float64) - R.normals(z.size, seed, 0, 0)).max())))
    assert worst <= 5 * NORMAL_MEASURED


@pytest.mark.parametrize("seed", SEEDS)
def test_normal_statistics(device_normals, seed):
    """Six standard errors over n = 2^20 (deterministic for a fixed seed): |mean| < 6/sqrt(n) = 5.9e-3, |var - 1| < 6 sqrt(2/n) = 8.3e-3,
    |m4 - 3| < 6 sqrt(96/n) = 5.7e-2, |corr| < 5.9e-3 between steps 0 and 1 and between streams 0 and 1."""
    z = device_normals[(seed, 0, 0)].astype(np.float64)
    assert abs(z.mean()) < 5.9e-3 and abs(z.var() - 1) < 8.3e-3 and abs((z ** 4).mean() - 3) < 5.7e-2
    for other in ((seed, 1, 0), (seed, 0, 1)):
        assert abs(np.corrcoef(z, device_normals[other].astype(np.float64))[0, 1]) < 5.9e-3, other


def test_normal_fill_does_not_depend_on_its_length(dev):
    from ltx_2_mlx_amd import kernels as K
    word = K.seed_word(42, dev)
    full = K.philox_normal(4099, word, 3, 1)
    for n in (1, 42, 4096):                             # a partial last quad; many blocks against one
        assert torch.equal(K.philox_normal(n, word, 3, 1), full[:n]), n


# ------------------------------------------------------------------ 2. the step kernels
_cases = {}


def _case(rows, C, dev):
    if (rows, C) not in _cases:
        g = torch.Generator().manual_seed(rows * 977 + C)
        t = {k: torch.randn(rows, C, generator=g).to(dev) for k in ("x", "vc", "vu", "clean")}
        t["ts_row"] = (torch.rand(rows, generator=g) * SIGMA).to(dev)
        mask = torch.ones(rows)
        mask[::3] = 0.0
        mask[1::3] = 0.05
        t["mask"] = mask.to(dev)
        _cases[(rows, C)] = t
    return _cases[(rows, C)]


def _f32(v):
    return float(np.float32(v))


def _blend(d, mask, clean):
    return d if mask is None else d * mask[:, None] + clean * (1 - mask[:, None])


def _parts(K, t, ts, vu, mask, cfg, up, down, z):
    """philox_normal's values and the separate ops: under guidance every fp32 torch op on its own; without, the plain step's kernels."""
    x, clean = t["x"], (t["clean"] if mask is not None else None)
    if vu is None:
        r = K.euler_step(x, _blend(K.x0_from_velocity(x, t["vc"], ts), mask, clean), SIGMA, down)
    else:
        tt = ts[:, None] if ts.numel() > 1 else ts
        a, b = x - tt * t["vc"], x - tt * vu
        d = _blend(a + _f32(np.float32(cfg) - np.float32(1)) * (a - b), mask, clean)
        r = x + ((x - d) * _f32(np.float32(1) / np.float32(SIGMA))) * _f32(np.float32(down) - np.float32(SIGMA))
    if up == 0:
        return r, None
    noise = z.reshape(x.shape) * _f32(up)
    return r + (noise if mask is None else noise * mask[:, None]), r


@pytest.mark.parametrize("rows,C", [(35, 128), (7, 6), (5, 128)])       # 16-byte form, 5 blocks; element-wise form, quads straddle rows, a partial last quad; one block
def test_step_kernel_bit_for_bit(dev, rows, C):
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.components import EulerAncestralDiffusionStep as S
    t, cfg, step = _case(rows, C, dev), 3.0, 5
    word = K.seed_word(42, dev)
    up, down = S._get_ancestral_step(SIGMA, SIGMA_NEXT, 1.0)
    z = K.philox_normal(rows * C, word, step, 0)
    for per_token in (False, True):
        ts = t["ts_row"] if per_token else torch.tensor([SIGMA], device=dev)
        for masked in (False, True):
            mask = t["mask"] if masked else None
            kw = dict(mask=mask, clean=t["clean"]) if masked else {}
            for vu in (t["vu"], None):
                tag = f"per_token={per_token} masked={masked} guided={vu is not None}"
                want, r = _parts(K, t, ts, vu, mask, cfg, up, down, z)
                got = K.ancestral_euler_step(t["x"], t["vc"], vu, ts, cfg, SIGMA, up, down, word, step, **kw)
                assert torch.equal(got, want), f"{tag}: {int((got != want).sum())} of {rows * C} elements differ"
                assert not torch.equal(got, r)
                if masked:                                      # m = 0: the Euler step towards clean and no noise on top
                    rows0 = t["mask"] == 0
                    assert torch.equal(got[rows0], r[rows0]) and not torch.equal(got[~rows0], r[~rows0])
                xin = t["x"].clone()                            # in place
                K.ancestral_euler_step(xin, t["vc"], vu, ts, cfg, SIGMA, up, down, word, step, out=xin, **kw)
                assert torch.equal(xin, want), tag
                # sigma_up == 0: the Euler step to sigma_down, no noise
                plain = K.ancestral_euler_step(t["x"], t["vc"], vu, ts, cfg, SIGMA, 0.0, down, word, step, **kw)
                if vu is not None:
                    assert torch.equal(plain, K.guided_euler_step(t["x"], t["vc"], vu, ts, cfg, SIGMA, down, **kw)), tag
                else:
                    d = _blend(K.x0_from_velocity(t["x"], t["vc"], ts), mask, t["clean"])
                    assert torch.equal(plain, K.euler_step(t["x"], d, SIGMA, down)), tag
            # the x0 form: the blended d as x0, the mask without clean -> the noise is masked, d is not blended again
            tt = ts[:, None] if per_token else ts
            a, b = t["x"] - tt * t["vc"], t["x"] - tt * t["vu"]
            d = _blend(a + _f32(np.float32(cfg) - np.float32(1)) * (a - b), mask, t["clean"])
            vel_form = K.ancestral_euler_step(t["x"], t["vc"], t["vu"], ts, cfg, SIGMA, up, down, word, step, **kw)
            assert torch.equal(K.ancestral_euler_step_x0(t["x"], d, SIGMA, up, down, word, step, 0, mask=mask), vel_form)
            if masked:                                          # with clean the entry blends itself
                g = a + _f32(np.float32(cfg) - np.float32(1)) * (a - b)
                assert torch.equal(K.ancestral_euler_step_x0(t["x"], g, SIGMA, up, down, word, step, 0, mask=mask, clean=t["clean"]), vel_form)
    # conditioned tokens (m = 0) sit on their clean values, as a loop holds them, and come out equal to clean: x - d = 0 and the noise is masked
    rows0 = t["mask"] == 0
    xc = t["x"].clone()
    xc[rows0] = t["clean"][rows0]
    for vu in (t["vu"], None):
        out = K.ancestral_euler_step(xc, t["vc"], vu, t["mask"] * SIGMA, cfg, SIGMA, up, down, word, step, mask=t["mask"], clean=t["clean"])
        assert torch.equal(out[rows0], t["clean"][rows0]) and not torch.equal(out[~rows0], xc[~rows0])


def test_pair_equals_two_single_launches(dev):
    """[35][128] + [9][128] in one launch: the video segment is the single launch's bits (stream 0), the audio segment those of philox_normal on
    stream 1 and the separate ops."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.components import EulerAncestralDiffusionStep as S
    v, a = _case(35, 128, dev), _case(9, 128, dev)
    word, step = K.seed_word(123456789012345, dev), 2
    up, down = S._get_ancestral_step(SIGMA, SIGMA_NEXT, 1.0)
    ts = torch.tensor([SIGMA], device=dev)
    for guided in (True, False):
        seg = lambda t, cfg, masked: dict(x=t["x"], vel_cond=t["vc"], vel_uncond=t["vu"] if guided else None, timesteps=t["ts_row"] if masked else ts,      # noqa: E731
                                          cfg_scale=cfg, **(dict(mask=t["mask"], clean=t["clean"]) if masked else {}))
        vout, aout = K.ancestral_euler_step_pair(seg(v, 3.0, True), seg(a, 7.0, False), SIGMA, up, down, word, step)
        single = K.ancestral_euler_step(v["x"], v["vc"], v["vu"] if guided else None, v["ts_row"], 3.0, SIGMA, up, down, word, step, mask=v["mask"], clean=v["clean"])
        assert torch.equal(vout, single), guided
        want_a, _ = _parts(K, a, ts, a["vu"] if guided else None, None, 7.0, up, down, K.philox_normal(9 * 128, word, step, 1))
        assert torch.equal(aout, want_a), guided
        assert not torch.equal(aout, K.ancestral_euler_step(a["x"], a["vc"], a["vu"] if guided else None, ts, 7.0, SIGMA, up, down, word, step))      # stream 0


def test_kernel_refusals(dev):
    from ltx_2_mlx_amd import _native as nv, kernels as K
    t = _case(5, 128, dev)
    word, ts = K.seed_word(1, dev), torch.tensor([SIGMA], device=dev)
    for bad in (dict(sigma=0.0), dict(sigma_up=-0.1), dict(sigma_down=-0.1)):
        kw = dict(sigma=SIGMA, sigma_up=0.1, sigma_down=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            K.ancestral_euler_step(t["x"], t["vc"], t["vu"], ts, 3.0, kw["sigma"], kw["sigma_up"], kw["sigma_down"], word, 0)
    with pytest.raises(ValueError):                 # a clean latent without its mask
        nv.check(nv.lib().ltx2_ancestral_euler_step_x0(nv.ptr(t["x"]), nv.ptr(t["vc"]), None, nv.ptr(t["clean"]), SIGMA, 0.1, 0.5, nv.ptr(word), 0, 0,
                                                       nv.ptr(torch.empty_like(t["x"])), 5, 128, nv.stream()))
    with pytest.raises(ValueError):                 # no seed
        nv.check(nv.lib().ltx2_philox_normal(nv.ptr(torch.empty(8, device=dev)), 8, None, 0, 0, nv.stream()))


# ------------------------------------------------------------------ 3. the loops
def _run(t, dev, joint, masked, start_clean=False, **kw):
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import ancestral_denoise_loop
    dv = lambda x: x.to(dev)          # noqa: E731
    lat = t.lat
    if start_clean:                   # the mask-0 tokens on their clean values
        lat = torch.where(t.mask == 0, t.clean, t.lat)
    vs = _state(lat, t.mask, t.pos, t.clean, dev, masked)
    if joint:
        out = ancestral_denoise_loop(X0Model(t.m), vs, _state(t.alat, t.amask, t.apos, t.aclean, dev, False), _sigmas(4), dv(t.ctx), dv(t.actx), dv(t.nctx),
                                     dv(t.nactx), **kw)
        return out[0].latent, out[1].latent
    return (ancestral_denoise_loop(X0Model(t.m), vs, None, _sigmas(4), dv(t.ctx), None, dv(t.nctx), None, **kw)[0].latent,)


def _loop_checks(t, dev, joint):
    from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import common as P
    same = lambda p, q: all(torch.equal(x, y) for x, y in zip(p, q))          # noqa: E731
    dv = lambda x: x.to(dev)          # noqa: E731
    for cfg in (dict(), dict(cfg_scale=3.0, audio_cfg_scale=7.0)):
        for masked in (True, False):
            eager = _run(t, dev, joint, masked, seed=42, use_hip_graph=False, fused=False, **cfg)
            fused = _run(t, dev, joint, masked, seed=42, use_hip_graph=False, **cfg)
            graph = _run(t, dev, joint, masked, seed=42, use_hip_graph=True, **cfg)
            assert same(eager, fused) and same(fused, graph), (cfg, masked, [int((x != y).sum()) for x, y in zip(eager, fused)])
            assert all(bool(torch.isfinite(x).all()) for x in fused)
            other = _run(t, dev, joint, masked, seed=43, use_hip_graph=False, **cfg)
            assert not any(torch.equal(x, y) for x, y in zip(fused, other))
            if masked:                                          # the image-conditioned tokens (mask 0) come back clean
                # the image-conditioned tokens (mask 0) started on noise here: they land on clean with the last step, to its rounding
                assert float((fused[0][0, :3] - t.clean[0, :3].to(dev)).abs().max()) <= 4 * 4.8e-7
                # started ON their clean values, as a pipeline's conditioning puts them, they are fixed points: x - d = 0 and the noise is masked
                rows0 = (t.mask[0].reshape(-1) == 0).to(dev)
                held = _run(t, dev, joint, True, seed=42, use_hip_graph=True, start_clean=True, **cfg)
                assert int(rows0.sum()) == 3 and torch.equal(held[0][0][rows0], t.clean[0].to(dev)[rows0]) and not torch.equal(held[0][0][~rows0], t.clean[0].to(dev)[~rows0])
        # eta = 0: the Euler loops' bits
        vs = lambda: _state(t.lat, t.mask, t.pos, t.clean, dev, False)          # noqa: E731
        zero = _run(t, dev, joint, False, eta=0.0, seed=42, use_hip_graph=False, **cfg)
        if joint and cfg:
            want = P.joint_guided_denoise_loop(X0Model(t.m), vs(), _state(t.alat, t.amask, t.apos, t.aclean, dev, False), _sigmas(4), dv(t.ctx), dv(t.actx),
                                               dv(t.nctx), dv(t.nactx), 3.0, 7.0, EulerDiffusionStep(), use_hip_graph=False)
        elif joint:
            want = P.joint_denoise_loop(X0Model(t.m), True, vs(), _state(t.alat, t.amask, t.apos, t.aclean, dev, False), _sigmas(4), dv(t.ctx), dv(t.actx),
                                        EulerDiffusionStep(), use_hip_graph=False)
        elif cfg:
            want = (P.guided_denoise_loop(X0Model(t.m), vs(), _sigmas(4), dv(t.ctx), dv(t.nctx), CFGGuider(3.0), EulerDiffusionStep(), use_hip_graph=False), None)
        else:
            want = P.joint_denoise_loop(X0Model(t.m), False, vs(), None, _sigmas(4), dv(t.ctx), None, EulerDiffusionStep(), use_hip_graph=False)
        assert same(zero, [w.latent for w in want if w is not None]), (cfg, [int((x != w.latent).sum()) for x, w in zip(zero, want)])


def test_video_loops(dev, tiny):
    """Eager (fused=False) == one C call per step == the captured graph, bit for bit, with and without guidance and an image-conditioned mask;
    two seeds differ; conditioned tokens come back clean; eta = 0 is joint_denoise_loop's / guided_denoise_loop's output bit for bit."""
    _loop_checks(tiny, dev, False)


def test_joint_loops(dev, tiny_av):
    """The same over both latents of the AudioVideo models, against joint_denoise_loop / joint_guided_denoise_loop at eta = 0."""
    _loop_checks(tiny_av, dev, True)


def test_one_captured_graph_serves_any_seed(dev, tiny):
    """The captured chain reads the seed from device memory: replayed after another seed is written into the word, it gives that seed's eager result."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.components import EulerAncestralDiffusionStep as S
    t, model, sig = tiny, tiny.m, _sigmas(4)
    steps = [S._get_ancestral_step(sig[i], sig[i + 1], 1.0) for i in range(4)]
    lat, word = t.lat[0].to(dev).float().contiguous(), K.seed_word(42, dev)
    neg = model.clone_sharing_weights()
    model.prepare(t.ctx.to(dev), t.pos.to(dev), per_token=False)
    neg.prepare(t.nctx.to(dev), t.pos.to(dev), per_token=False)
    side, outs = torch.cuda.Stream(), {}
    with torch.cuda.stream(side):
        model.capture_ancestral_graph(neg, lat, sig, [s[0] for s in steps], [s[1] for s in steps], word, 3.0)
        for seed in (42, 7, 42):
            lat.copy_(t.lat[0].to(dev))
            word.copy_(K.seed_word(seed, dev))
            model.replay_ancestral_graph()
            outs.setdefault(seed, []).append(lat.clone())
    side.synchronize()
    assert torch.equal(outs[42][0], outs[42][1]) and not torch.equal(outs[42][0], outs[7][0])
    for seed in (42, 7):
        assert torch.equal(outs[seed][0][None], _run(t, dev, False, False, seed=seed, cfg_scale=3.0, use_hip_graph=False)[0]), seed


def test_diffusion_step_class_runs_the_x0_kernel(dev):
    """EulerAncestralDiffusionStep.step without `noise` == its torch path fed philox_normal's values, to the rounding of (x - d)/sigma against
    (x - d)*(1/sigma): within 4 ulp of [4, 8)."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.components import EulerAncestralDiffusionStep
    t, sig = _case(35, 128, dev), [SIGMA, SIGMA_NEXT, 0.0]
    st = EulerAncestralDiffusionStep(eta=1.0, seed=42)
    got = st.step(t["x"][None], t["vc"][None], sig, 0, stream_id=1)
    z = K.philox_normal(35 * 128, K.seed_word(42, dev), 0, 1).reshape(1, 35, 128)
    assert got.shape == (1, 35, 128) and float((got - st.step(t["x"][None], t["vc"][None], sig, 0, noise=z)).abs().max()) <= 4 * 4.8e-7
    last = st.step(t["x"][None], t["vc"][None], sig, 1)                     # sigma_next = 0: lands on x0, no noise
    assert float((last - t["vc"][None]).abs().max()) <= 4 * 4.8e-7


# ------------------------------------------------------------------ 4. the pipeline
def test_distilled_pipeline_runs_stage_one_through_the_ancestral_loop(dev, tiny):
    """DistilledPipeline(sampler="euler_ancestral") == ancestral_denoise_loop on the same state (the noise seed is config.seed); another eta and the
    default sampler differ; an unknown sampler name is refused."""
    from oracle import loop
    from ltx_2_mlx_amd.components import DISTILLED_SIGMA_VALUES
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import DistilledConfig, DistilledPipeline
    from ltx_2_mlx_amd.pipelines.common import ancestral_denoise_loop, final_latent, video_tools_for
    t = tiny
    f, h, w = loop.latent_shape_from_pixels(9, 64, 96)
    assert (f, h, w) == (2, 2, 3)
    noise = t.lat.to(dev)
    pipe = DistilledPipeline(t.m, None, None)
    conf = lambda **k: DistilledConfig(height=128, width=192, num_frames=9, seed=7, **k)          # noqa: E731  (stage 1 at 64x96x9)
    got = pipe(t.ctx.to(dev), None, conf(sampler="euler_ancestral", ancestral_eta=0.8), initial_noise=noise)
    tools = video_tools_for(pipe.patchifier, 9, 64, 96, 25.0)
    state = tools.create_initial_state(dtype=torch.float32, device=dev)
    state = state.replace(latent=noise)
    want, _ = ancestral_denoise_loop(X0Model(t.m), state, None, DISTILLED_SIGMA_VALUES, t.ctx.to(dev), eta=0.8, seed=7, use_hip_graph=False)
    assert torch.equal(got, final_latent(tools, want))
    assert not torch.equal(got, pipe(t.ctx.to(dev), None, conf(sampler="euler_ancestral"), initial_noise=noise))
    assert not torch.equal(got, pipe(t.ctx.to(dev), None, conf(), initial_noise=noise))
    with pytest.raises(ValueError):
        conf(sampler="dpm")


def test_one_stage_pipeline_runs_the_ancestral_loop(dev, tiny, tiny_av):
    """OneStagePipeline(sampler="euler_ancestral") == ancestral_denoise_loop on the same states: video-only under plain CFG and unguided, and the
    AudioVideo model with both latents under a CFGGuider each; the noise seed is config.seed.  The listed refusals raise before anything runs."""
    from ltx_2_mlx_amd.components import CFGStarRescalingGuider, LTX2Scheduler, LtxAPGGuider
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    from ltx_2_mlx_amd.pipelines.common import ancestral_denoise_loop, final_latent, video_tools_for
    dv = lambda x: x.to(dev)          # noqa: E731
    t = tiny
    pipe = OneStagePipeline(t.m, None, None)
    conf = lambda **k: OneStageCFGConfig(height=64, width=96, num_frames=9, num_inference_steps=4, seed=5, fps=25.0, **k)          # noqa: E731
    sig = LTX2Scheduler().execute(steps=4)
    tools = video_tools_for(pipe.patchifier, 9, 64, 96, 25.0)
    start = tools.create_initial_state(dtype=torch.float32, device=dev).replace(latent=dv(t.lat))
    for cfg in (3.0, 1.0):
        got, _ = pipe(dv(t.ctx), dv(t.nctx), conf(cfg_scale=cfg, rescale_scale=0.0), sampler="euler_ancestral", ancestral_eta=0.8, initial_noise=dv(t.lat))
        want, _ = ancestral_denoise_loop(X0Model(t.m), start, None, sig, dv(t.ctx), None, dv(t.nctx), None, cfg_scale=cfg, eta=0.8, seed=5, use_hip_graph=False)
        assert torch.equal(got, final_latent(tools, want)), cfg
    assert not torch.equal(got, pipe(dv(t.ctx), None, conf(cfg_scale=1.0, rescale_scale=0.0), initial_noise=dv(t.lat))[0])          # the Euler sampler
    plain = conf(rescale_scale=0.0)
    for kw in (dict(stg_scale=1.0), dict(ge_gamma=2.0), dict(cross_attn_scale=2.0), dict(temporal_upscaler=object()), dict(guider_override=LtxAPGGuider(3.0, 0.5, 5.0)),
               dict(guider_override=CFGStarRescalingGuider(3.0))):
        with pytest.raises(NotImplementedError):
            pipe(dv(t.ctx), dv(t.nctx), plain, sampler="euler_ancestral", **kw)
    with pytest.raises(NotImplementedError):
        pipe(dv(t.ctx), dv(t.nctx), conf(), sampler="euler_ancestral")                      # the config default: CFG*
    with pytest.raises(ValueError):
        pipe(dv(t.ctx), dv(t.nctx), plain, sampler="dpm")
    # both latents
    a = tiny_av
    apipe = OneStagePipeline(a.m, None, None)
    aconf = conf(cfg_scale=3.0, audio_cfg_scale=7.0, rescale_scale=0.0, audio_enabled=True)
    got_v, got_a = apipe(dv(a.ctx), dv(a.nctx), aconf, positive_audio_encoding=dv(a.actx), negative_audio_encoding=dv(a.nactx), sampler="euler_ancestral",
                         initial_noise=dv(a.lat), initial_audio_noise=dv(a.alat))
    vt, vs, at, as_ = _pipeline_states(apipe, aconf, dv(a.lat), dv(a.alat), dev)
    assert as_.latent.shape == (1, 9, 128)
    wv, wa = ancestral_denoise_loop(X0Model(a.m), vs, as_, sig, dv(a.ctx), dv(a.actx), dv(a.nctx), dv(a.nactx), cfg_scale=3.0, audio_cfg_scale=7.0, seed=5,
                                    use_hip_graph=False)
    assert torch.equal(got_v, final_latent(vt, wv)) and torch.equal(got_a, final_latent(at, wa))
    assert bool(torch.isfinite(got_v).all()) and bool(torch.isfinite(got_a).all())
