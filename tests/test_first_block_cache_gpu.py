"""The first-block cache on the GPU: the metric kernel element-wise and against float64 within the bound of its reduction depth, t = 0 and
t = +inf loops, a controlled decision pattern against the fp32 restatement (tests/first_block_cache_ref.py), slot independence, and
generate_video end to end.  Tiny 3-layer models as tests/test_parity.py builds them."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import measure, rel_l2

import first_block_cache_ref as FR
from test_parity import make_dit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0
U64 = 2.0 ** -53
CFG, RESCALE = 3.0, 0.7
INF = float("inf")
# measured on the MI355X (the figures are in each test's docstring); every gate is at most 5x its figure
REUSE_GATE = 0.0
PATTERN_GATE = 1.0e-2


def _buf(n, dev, offset=0):
    buf = torch.full((n + 64 + offset,), SENTINEL, device=dev, dtype=torch.float32)
    return buf, buf[offset:offset + n]


def _intact(buf, n, offset=0):
    return bool((buf[offset + n:] == SENTINEL).all()) and bool((buf[:offset] == SENTINEL).all())


def _depth(n, blocks):
    """The fp64 additions one element's value passes through at the most: its thread's chain (4 per quad), the block's tree (8), the finishing
    block's chain over the partials and its tree (8) -- plus 1 for the rounding of the term |r - head_prev| itself."""
    quads = (n + 3) // 4
    return 4 * math.ceil(quads / (blocks * 256)) + 8 + math.ceil(blocks / 256) + 8 + 1


# ------------------------------------------------------------------ 1. the metric kernel
@pytest.mark.parametrize("rows,C,off", [(1, 128, 0), (5, 6, 0), (37, 128, 0), (37, 128, 1), (33000, 128, 0)])
def test_metric_kernel(dev, rows, C, off):
    """r bit for bit; num and den against exact sums (math.fsum of the float64 terms, so the reference carries no summation error of its own)
    within depth * 2^-53 * sum: the standard bound |fl(sum) - sum| <= gamma_k * sum|terms| for any order in which no value passes through more
    than k additions (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), gamma_k = k u / (1 - k u) <= 1.01 k u here, u = 2^-53,
    all terms being non-negative.  Two launches agree bit for bit, the aligned and the misaligned form agree bit for bit, an all-zero head_prev
    decides 0, and nothing is written outside the operands.  off = 1: every base pointer 4 bytes off a 16-byte boundary."""
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    n = rows * C
    g = torch.Generator().manual_seed(rows * 977 + C)
    src = {k: torch.randn(n, generator=g) for k in ("h0", "h1", "hp")}
    src["h1"] = src["h0"] + 0.3 * src["h1"]
    src["hp"] = 0.3 * src["hp"]
    bufs, v = {}, {}
    for k in ("h0", "h1", "hp", "r", "save"):
        bufs[k], v[k] = _buf(n, dev, off)
        if k in src:
            v[k].copy_(src[k])
    assert all(x.data_ptr() % 16 == 4 * off for x in v.values())
    blocks = nv.lib().ltx2_fbc_metric_blocks(n)
    assert blocks == min(1024, math.ceil(math.ceil(n / 4) / 2048))
    r64 = (src["h1"] - src["h0"]).double().numpy()           # the fp32 difference, widened
    terms = np.abs(r64 - src["hp"].double().numpy())
    num64, den64 = math.fsum(terms.tolist()), math.fsum(np.abs(src["hp"].double().numpy()).tolist())
    bound = 1.01 * _depth(n, blocks) * U64
    t = float(np.float32(1.02 * num64 / den64))               # just above the ratio: a skip
    r, num, den, skip = K.fbc_head_metric(v["h0"], v["h1"], v["hp"], t, r=v["r"], h1_save=v["save"])
    assert torch.equal(r.cpu(), src["h1"] - src["h0"]) and torch.equal(v["save"].cpu(), src["h1"])
    e_num, e_den = measure(f"num rel err {rows}x{C}", abs(num - num64) / num64), measure(f"den rel err {rows}x{C}", abs(den - den64) / den64)
    print(f"metric {rows}x{C} off {off}: blocks {blocks} depth {_depth(n, blocks)} bound {bound:.3e} num err {e_num:.3e} den err {e_den:.3e}")
    assert e_num <= bound and e_den <= bound
    assert skip == 1 and FR.decide(num, den, t)
    _, num2, den2, skip2 = K.fbc_head_metric(v["h0"], v["h1"], v["hp"], float(np.float32(0.98 * num64 / den64)), r=v["r"])
    assert (num2, den2) == (num, den) and skip2 == 0           # bit-identical sums from a second launch; just below the ratio computes
    assert K.fbc_head_metric(v["h0"], v["h1"], v["hp"], 0.0, r=v["r"])[3] == 0 and K.fbc_head_metric(v["h0"], v["h1"], v["hp"], INF, r=v["r"])[3] == 1
    # the other access form adds in the same order
    if off:
        al = {k: src[k].to(dev) for k in src}
        assert K.fbc_head_metric(al["h0"], al["h1"], al["hp"], t)[1:3] == (num, den)
    # an all-zero head_prev, and none at all: den = 0 decides 0 at any threshold; num is then sum |r|
    v["hp"].zero_()
    for hp in (v["hp"], None):
        _, nz, dz, sz = K.fbc_head_metric(v["h0"], v["h1"], hp, INF, r=v["r"])
        assert dz == 0.0 and sz == 0 and abs(nz - math.fsum(np.abs(r64).tolist())) <= bound * nz
    # in place over h0, as the engine saves h1
    K.fbc_head_metric(v["h0"], v["h1"], None, 0.0, r=v["r"], h1_save=v["h0"])
    assert torch.equal(v["h0"].cpu(), src["h1"]) and torch.equal(v["r"].cpu(), src["h1"] - src["h0"])
    # the two element-wise kernels, bit for bit
    tail = K.fbc_store_tail(v["h1"], v["save"], tail=v["r"])
    assert bool((tail == 0).all())
    v["save"].copy_(src["h0"])
    assert torch.equal(K.fbc_store_tail(v["h1"], v["save"], tail=v["r"]).cpu(), src["h1"] - src["h0"])
    assert torch.equal(K.fbc_apply_tail(v["save"], v["r"]).cpu(), src["h0"] + (src["h1"] - src["h0"]))
    torch.cuda.synchronize()
    assert all(_intact(bufs[k], n, off) for k in bufs), [k for k in bufs if not _intact(bufs[k], n, off)]


# ------------------------------------------------------------------ the tiny model
class Tiny:
    pass


@pytest.fixture(scope="module")
def tiny(dev):
    """3 layers (block 0 and a tail of two), 12 tokens, two prompts."""
    from oracle import loop
    t = Tiny()
    t.cfg, t.wq, t.m = make_dit(dev, heads=2, layers=3, cap=64, seed=11)
    g = torch.Generator().manual_seed(4321)
    t.pos = loop.video_positions(1, 2, 2, 3, 25.0)
    t.lat = torch.randn(1, 12, 128, generator=g)
    t.pert = torch.randn(1, 12, 128, generator=g)
    t.ctx, t.nctx = 0.1 * torch.randn(1, 24, 64, generator=g), 2.0 * torch.randn(1, 24, 64, generator=g)
    t.ctx_d, t.nctx_d, t.pos_d = t.ctx.to(dev), t.nctx.to(dev), t.pos.to(dev)       # one device copy each: a context is prepared once per prompt
    t.neg = t.m.clone_sharing_weights()
    t.m.prepare(t.ctx_d, t.pos_d)
    t.neg.prepare(t.nctx_d, t.pos_d)
    return t


def _state(t, dev):
    from ltx_2_mlx_amd.types import LatentState
    return LatentState(latent=t.lat.clone().to(dev), denoise_mask=torch.ones(1, 12, 1, device=dev), positions=t.pos_d,
                       clean_latent=torch.zeros(1, 12, 128, device=dev))


def _sigmas(steps):
    from ltx_2_mlx_amd.components import LTX2Scheduler
    return [float(s) for s in LTX2Scheduler().execute(steps=steps)]


def _loop(t, dev, sig, cfg_scale, **kw):
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines.common import first_block_cache_last_stats, standard_cfg_denoise_loop
    out = standard_cfg_denoise_loop(X0Model(t.m), _state(t, dev), sig, t.ctx_d, t.nctx_d, cfg_scale, RESCALE, **kw).latent
    return out, ([(d["evaluations"], d["skips"]) for d in first_block_cache_last_stats()] if kw.get("first_block_cache", 0) > 0 else None)


def _mod(t, dev, lat, ctx, sigma):
    from ltx_2_mlx_amd.model.transformer import Modality
    return Modality(latent=lat, context=ctx, context_mask=None, timesteps=torch.tensor([sigma], device=dev), positions=t.pos_d)


# ------------------------------------------------------------------ 2. t = 0
def test_zero_threshold_is_the_uncached_loop(dev, tiny):
    """The engine cannot be asked for a cache at t = 0 through the loop (0 is off), so the loop is driven by hand: 4 steps of the cached guided
    step at t = 0 against rescaled_guided_step_, and of the cached plain step against denoise_step_, bit for bit, with 0 skips in the stats."""
    t, m, sig = tiny, tiny.m, _sigmas(4)
    ctx = t.ctx_d
    m.enable_first_block_cache(0.0, slots=2)
    try:
        for guided in (True, False):
            m.reset_first_block_cache()
            a, b = t.lat[0].to(dev).contiguous(), t.lat[0].to(dev).contiguous()
            for i in range(4):
                if i == 3:
                    m.force_first_block_cache()
                if guided:
                    m.rescaled_guided_step_(t.neg, a, _mod(t, dev, a[None], ctx, sig[i]), sig[i], sig[i + 1], CFG, RESCALE)
                    m.rescaled_guided_step_cached_(t.neg, b, _mod(t, dev, b[None], ctx, sig[i]), sig[i], sig[i + 1], CFG, RESCALE)
                else:
                    m.denoise_step_(a, _mod(t, dev, a[None], ctx, sig[i]), sig[i], sig[i + 1])
                    m.denoise_step_cached_(b, _mod(t, dev, b[None], ctx, sig[i]), sig[i], sig[i + 1])
                assert torch.equal(a, b), (guided, i, int((a != b).sum()))
            st = m.first_block_cache_stats()
            assert [(d["evaluations"], d["skips"]) for d in st] == ([(4, 0), (4, 0)] if guided else [(4, 0), (0, 0)])
            assert st[0]["last_den"] > 0 and st[0]["last_num"] > 0         # steps 1 and 2 compared (and computed)
    finally:
        m.enable_first_block_cache(0.0, slots=0)
    assert m.first_block_cache_stats() == []


# ------------------------------------------------------------------ 3. t = +inf
def test_infinite_threshold(dev, tiny):
    """Every evaluation that is neither first nor last reuses the tail, in both loops; and the same input twice: the second evaluation reuses the
    tail of the first and differs from the plain forward by the fp32 rounding of h1 + (hL - h1) alone.  Measured on the MI355X: rel-L2 0.0 (on
    these 12 tokens the last-bit differences of the fp32 stream do not survive the rounding of the output head's 16-bit GEMM operand), so by
    the 5x rule the gate REUSE_GATE is 0: the two outputs are equal.  The kernels are deterministic, so the figure does not move."""
    t, m = tiny, tiny.m
    for steps in (4, 6):
        out, st = _loop(t, dev, _sigmas(steps), CFG, first_block_cache=INF)
        assert st == [(steps, steps - 2)] * 2 and bool(torch.isfinite(out).all())
        out, st = _loop(t, dev, _sigmas(steps), 1.0, first_block_cache=INF)
        assert st == [(steps, steps - 2)] and bool(torch.isfinite(out).all())
    mod = _mod(t, dev, t.lat.to(dev), t.ctx_d, 0.8)
    plain = m(mod).clone()
    m.enable_first_block_cache(INF, slots=1)
    try:
        first, second = m.forward_cached(mod).clone(), m.forward_cached(mod).clone()
        st = m.first_block_cache_stats()[0]
        assert (st["evaluations"], st["skips"], st["last_num"]) == (2, 1, 0.0) and st["last_den"] > 0
        assert torch.equal(first, plain)
        e = measure("tail reused on the same input vs plain forward", rel_l2(second.cpu(), plain.cpu()))
        print(f"t = inf, same input twice: rel-L2 {e:.3e}")
        assert e <= REUSE_GATE
        with pytest.raises(ValueError, match="slot"):
            m.forward_cached(mod, slot=1)
        from ltx_2_mlx_amd.components.perturbations import create_batched_stg_config
        with pytest.raises(NotImplementedError, match="perturbed"):
            m.forward_cached(mod, perturbations=create_batched_stg_config(1, True, [0]))
    finally:
        m.enable_first_block_cache(0.0, slots=0)
    with pytest.raises(ValueError, match="cache is off"):
        m.forward_cached(mod)


# ------------------------------------------------------------------ 4. a decision pattern
EPS = [0.0, 0.002, 0.5, 0.502, 0.504, 1.0]
T_MID = 0.05


def _pattern_inputs(t):
    return [t.lat + e * t.pert for e in EPS]


def _pattern_reference(t):
    cache = FR.FirstBlockCache(T_MID, 1)
    model = FR.BlockwiseDiT(t.cfg, t.wq, t.ctx, t.pos)
    ts = torch.tensor([0.8])
    outs = []
    for i, lat in enumerate(_pattern_inputs(t)):
        if i == len(EPS) - 1:
            cache.force_next()
        outs.append(model.velocity(lat, ts, cache, 0))
    return cache, outs


def test_decision_pattern(dev, tiny):
    """Six evaluations of base + eps_i * perturbation at one sigma, the last forced.  The restatement's float64 metric of every evaluation lies 25 %
    or more from T_MID (asserted), so the device's bf16 block 0 cannot flip a decision; the device pattern must be the restatement's, compute,
    skip, compute, skip, skip, compute, and every output within PATTERN_GATE of the restatement's (measured on the MI355X: 2.21e-3 to 2.34e-3,
    the skipped evaluations no further off than the computed ones; the gate is 4.3x the largest)."""
    t, m = tiny, tiny.m
    cache, ref = _pattern_reference(t)
    ratios = [e[1] / e[2] for e in cache.slots[0].log if e[1] is not None]
    print("reference metric per compared evaluation:", ["%.4f" % r for r in ratios])
    assert len(ratios) == 5 and all(abs(r - T_MID) >= 0.25 * T_MID for r in ratios)
    assert cache.pattern() == [False, True, False, True, True, False]
    m.enable_first_block_cache(T_MID, slots=1)
    try:
        got, skips = [], []
        for i, lat in enumerate(_pattern_inputs(t)):
            if i == len(EPS) - 1:
                m.force_first_block_cache()
            got.append(m.forward_cached(_mod(t, dev, lat.to(dev), t.ctx_d, 0.8)).cpu())
            skips.append(m.first_block_cache_stats()[0]["skips"])
        pattern = [b > a for a, b in zip([0] + skips, skips)]
    finally:
        m.enable_first_block_cache(0.0, slots=0)
    assert pattern == cache.pattern()
    errs = [measure(f"evaluation {i} vs restatement", rel_l2(g, r)) for i, (g, r) in enumerate(zip(got, ref))]
    print("decision pattern, rel-L2 per evaluation:", ["%.3e" % e for e in errs])
    assert max(errs) <= PATTERN_GATE


def test_pattern_inputs_on_the_restatement():
    """The CPU half of the condition above (no device needed, kept beside the test it serves)."""
    from oracle import dit, loop
    t = Tiny()
    t.cfg = dit.DiTConfig(num_attention_heads=2, attention_head_dim=128, num_layers=3, caption_channels=64)
    w = dit.make_dit_weights(t.cfg, 11)
    t.wq = {k: (v.to(torch.bfloat16).float() if (k.endswith(".weight") and v.dim() == 2) else v) for k, v in w.items()}
    g = torch.Generator().manual_seed(4321)
    t.pos = loop.video_positions(1, 2, 2, 3, 25.0)
    t.lat = torch.randn(1, 12, 128, generator=g)
    t.pert = torch.randn(1, 12, 128, generator=g)
    t.ctx = 0.1 * torch.randn(1, 24, 64, generator=g)
    cache, _ = _pattern_reference(t)
    ratios = [e[1] / e[2] for e in cache.slots[0].log if e[1] is not None]
    assert all(abs(r - T_MID) >= 0.25 * T_MID for r in ratios) and cache.pattern() == [False, True, False, True, True, False]


# ------------------------------------------------------------------ 5. slots
def test_slots(dev, tiny):
    """A CFG loop over slots 0 and 1 against two single-slot runs of the same passes: the latents the guided loop steps through are recorded, then
    each prompt's passes are replayed alone through a one-slot cache on its own context -- the same velocities bit for bit, hence the same
    decisions and counts.  And the same loop twice gives the same latents and stats: the reset at loop start leaves nothing behind."""
    from ltx_2_mlx_amd import kernels as K
    t, m, sig = tiny, tiny.m, _sigmas(5)
    ctx, nctx = t.ctx_d, t.nctx_d
    thr = 0.2
    a, st_a = _loop(t, dev, sig, CFG, first_block_cache=thr)
    b, st_b = _loop(t, dev, sig, CFG, first_block_cache=thr)
    assert torch.equal(a, b) and st_a == st_b and [s[0] for s in st_a] == [5, 5]
    # by hand: both slots on the positive context, the velocities visible
    m.enable_first_block_cache(thr, slots=2)
    try:
        m.reset_first_block_cache()
        lat, seen = t.lat[0].to(dev).contiguous(), []
        for i in range(5):
            if i == 4:
                m.force_first_block_cache()
            seen.append(lat.clone())
            m.rescaled_guided_step_cached_(t.neg, lat, _mod(t, dev, lat[None], ctx, sig[i]), sig[i], sig[i + 1], CFG, RESCALE)
        two = [(d["evaluations"], d["skips"]) for d in m.first_block_cache_stats()]
        assert torch.equal(lat[None], a) and two == st_a
    finally:
        m.enable_first_block_cache(0.0, slots=0)
    vels, one = {}, {}
    for name, model, c in (("pos", m, ctx), ("neg", t.neg, nctx)):
        model.enable_first_block_cache(thr, slots=1)
        try:
            model.reset_first_block_cache()
            vels[name] = []
            for i in range(5):
                if i == 4:
                    model.force_first_block_cache()
                vels[name].append(model.forward_cached(_mod(t, dev, seen[i][None], c, sig[i]))[0].clone())
            d = model.first_block_cache_stats()[0]
            one[name] = (d["evaluations"], d["skips"])
        finally:
            model.enable_first_block_cache(0.0, slots=0)
    assert [one["pos"], one["neg"]] == two
    lat = t.lat[0].to(dev).contiguous()
    for i in range(5):
        assert torch.equal(lat, seen[i]), i
        ts = torch.tensor([sig[i]], device=dev)
        stats = K.channel_guidance_stats(lat, vels["pos"][i], vels["neg"][i], ts, CFG)
        lat = K.rescaled_guided_euler_step(lat, vels["pos"][i], vels["neg"][i], ts, CFG, RESCALE, sig[i], sig[i + 1], stats=stats)
    assert torch.equal(lat[None], a)
    print(f"slots: (evaluations, skips) per slot at t = {thr}: {two}")


# ------------------------------------------------------------------ 6. end to end
def test_generate_video(dev, tmp_path, capsys, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate as gen
    from ltx_2_mlx_amd.model.transformer import LTXModel
    calls = {"capture": 0, "enable": 0}
    cap, en = LTXModel.capture_denoise_graph, LTXModel.enable_first_block_cache
    monkeypatch.setattr(LTXModel, "capture_denoise_graph", lambda self, *a, **k: (calls.__setitem__("capture", calls["capture"] + 1), cap(self, *a, **k))[1])
    monkeypatch.setattr(LTXModel, "enable_first_block_cache", lambda self, *a, **k: (calls.__setitem__("enable", calls["enable"] + 1), en(self, *a, **k))[1])
    kw = dict(height=128, width=192, num_frames=9, num_steps=4, num_layers=3, num_heads=2, vae_base_channels=64, use_gemma=False, save_mp4=False,
              compute_dtype="bfloat16")
    frames = gen.generate_video("a prompt", output_path=str(tmp_path / "on.mp4"), first_block_cache=0.1, **kw)
    out = capsys.readouterr().out
    line = [l.strip() for l in out.splitlines() if "first-block cache:" in l]
    assert len(line) == 1 and line[0].startswith("first-block cache: ") and line[0].endswith(" of 4 evaluations reused the tail (threshold 0.1)"), out
    assert frames is not None and frames.shape[1:] == (128, 192, 3) and calls == {"capture": 0, "enable": 2}
    # off: the captured graph, as before, and no word of the cache
    frames0 = gen.generate_video("a prompt", output_path=str(tmp_path / "off.mp4"), first_block_cache=0.0, **kw)
    out = capsys.readouterr().out
    assert "first-block cache" not in out and calls == {"capture": 1, "enable": 2} and frames0.shape == frames.shape
    # the guided route takes it too: two slots, 2 x 4 evaluations
    gen.generate_video("a prompt", output_path=str(tmp_path / "cfg.mp4"), first_block_cache=0.1, standard_cfg=True, model_variant="dev", cfg_scale=3.0,
                       **dict(kw, skip_vae=True))
    assert " of 8 evaluations reused the tail (threshold 0.1)" in capsys.readouterr().out
