"""First-block cache, host side: the restatement (tests/first_block_cache_ref.py) against hand-computed cases, the C ABI's new entries, and every
refusal of generate_video / the loop.  No GPU."""
import inspect
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import first_block_cache_ref as FR  # noqa: E402


# ------------------------------------------------------------------ the restatement, by hand
def _run(cache, inputs, slot=0, force_at=()):
    """Evaluate 1-element-per-entry streams: block 0 adds head[i] to the stream, blocks 1..L-1 add tail[i]; -> outputs."""
    out = []
    for i, (h0, head, tail) in enumerate(inputs):
        if i in force_at:
            cache.force_next(slot)
        t = lambda v: torch.tensor(v, dtype=torch.float32)      # noqa: E731
        out.append(cache.evaluate(slot, t(h0), lambda h, d=head: h + t(d), lambda h, d=tail: h + t(d)).tolist())
    return out


def test_metric_and_decision_by_hand():
    assert FR.metric64([1.0, -2.0, 4.0], [1.5, -2.0, 2.0]) == (2.5, 5.5)
    assert FR.decide(2.5, 5.5, 0.5) and not FR.decide(2.5, 5.5, 0.25)           # 2.5 < 2.75, 2.5 >= 1.375
    assert not FR.decide(2.75, 5.5, 0.5)                                        # strict: equality computes
    assert not FR.decide(0.0, 5.5, 0.0)                                         # t = 0 never skips, even at num = 0
    assert not FR.decide(0.0, 0.0, 1.0) and not FR.decide(0.0, 0.0, float("inf"))      # den = 0 never skips (inf * 0 is not a number)
    assert FR.decide(1e300, 1e-300, float("inf"))
    assert FR.decide(1.0, 10.0, 0.1) and not 1.0 < 0.1 * 10.0                   # the threshold is taken in float32: 0.1f = 0.100000001490116 > 0.1
    with pytest.raises(ValueError):
        FR.FirstBlockCache(-1.0, 1)


def test_skip_reuses_the_tail_and_keeps_the_state():
    # block 0 residuals 1.0, 1.04, 1.3, 1.34; tails 10, 20, 30, 40; t = 0.05
    c = FR.FirstBlockCache(0.05, 1)
    out = _run(c, [([0.0], [1.0], [10.0]), ([5.0], [1.04], [20.0]), ([5.0], [1.3], [30.0]), ([1.0], [1.34], [40.0])])
    # 1: |1.04 - 1| = 0.04 < 0.05*1: skip, h = h1 + 10.  2: 0.3 against head_prev = 1.0 (NOT 1.04): compute.  3: |1.34 - 1.3| = 0.04 < 0.065: skip with tail 30
    assert c.pattern() == [False, True, False, True]
    assert [o[0] for o in out] == pytest.approx([11.0, 16.04, 36.3, 32.34])
    assert c.stats() == [dict(evaluations=4, skips=2)]
    assert c.slots[0].head_prev.tolist() == pytest.approx([1.3]) and c.slots[0].tail.tolist() == pytest.approx([30.0])
    # head_prev is not updated on a skip: a slow drift 1.0 -> 1.04 -> 1.08 is measured against 1.0 both times, so the second one computes
    c = FR.FirstBlockCache(0.05, 1)
    _run(c, [([0.0], [1.0], [10.0]), ([0.0], [1.04], [10.0]), ([0.0], [1.08], [10.0])])
    assert c.pattern() == [False, True, False]
    assert [round(e[1], 6) if e[1] is not None else None for e in c.slots[0].log] == [None, 0.04, 0.08]


def test_zero_threshold_zero_denominator_and_forcing():
    same = [([0.0], [1.0], [10.0])] * 4
    c = FR.FirstBlockCache(0.0, 1)
    _run(c, same)
    assert c.pattern() == [False] * 4 and c.stats()[0]["skips"] == 0           # t = 0: num = 0 < 0 is false
    c = FR.FirstBlockCache(float("inf"), 1)
    _run(c, [([0.0], [0.0], [10.0])] * 3)
    assert c.pattern() == [False] * 3                                           # head_prev all zero: den = 0 never skips
    c = FR.FirstBlockCache(float("inf"), 1)
    out = _run(c, same, force_at=(2,))
    assert c.pattern() == [False, True, False, True] and out == [[11.0]] * 4    # a forced step computes, and the force is consumed by it
    c.reset()
    assert c.stats() == [dict(evaluations=0, skips=0)] and not c.slots[0].valid


def test_slots_are_independent():
    c = FR.FirstBlockCache(0.05, 2)
    _run(c, [([0.0], [1.0], [10.0]), ([0.0], [1.0], [10.0])], slot=0)
    _run(c, [([0.0], [2.0], [20.0])], slot=1)
    assert c.stats() == [dict(evaluations=2, skips=1), dict(evaluations=1, skips=0)]
    assert c.slots[1].head_prev.tolist() == [2.0] and c.slots[0].head_prev.tolist() == [1.0]


def test_loop_driver_forces_the_first_and_the_last_step():
    """At t = +inf every evaluation that is neither first nor last skips, in both slots; at t = 0 the cached loop is the plain one bit for bit."""
    from oracle import dit, loop
    cfg = dit.DiTConfig(num_attention_heads=1, attention_head_dim=128, num_layers=3, caption_channels=128)
    w = dit.make_dit_weights(cfg, 3)
    g = torch.Generator().manual_seed(5)
    lat, ctx, nctx = torch.randn(1, 8, 128, generator=g), 0.1 * torch.randn(1, 16, 128, generator=g), 0.1 * torch.randn(1, 16, 128, generator=g)
    pos = loop.video_positions(1, 2, 2, 2, 24.0)
    P, N = FR.BlockwiseDiT(cfg, w, ctx, pos), FR.BlockwiseDiT(cfg, w, nctx, pos)
    ts = torch.tensor([0.7])
    assert torch.equal(P.velocity(lat, ts), dit.velocity_model(lat, ctx, ts, pos, w, cfg))          # the block-by-block cut is the oracle's model
    sig = [1.0, 0.8, 0.6, 0.4, 0.2]
    c = FR.FirstBlockCache(float("inf"), 2)
    FR.cached_loop(lat, sig, c, P, N, 3.0, 0.7)
    assert c.pattern(0) == c.pattern(1) == [False, True, True, False] and c.stats() == [dict(evaluations=4, skips=2)] * 2
    c0 = FR.FirstBlockCache(0.0, 2)
    import standard_cfg_ref as R
    plain = R.standard_cfg_loop(lat, lambda x, t, s: x - s * P.velocity(x, t), lambda x, t, s: x - s * N.velocity(x, t), sig, 3.0, 0.7)
    assert torch.equal(FR.cached_loop(lat, sig, c0, P, N, 3.0, 0.7), plain) and c0.stats() == [dict(evaluations=4, skips=0)] * 2


# ------------------------------------------------------------------ the C ABI
NEW = {"ltx2_fbc_metric_blocks": 1, "ltx2_fbc_head_metric": 10, "ltx2_fbc_store_tail": 5, "ltx2_fbc_apply_tail": 4, "ltx2_dit_fbc_configure": 3,
       "ltx2_dit_fbc_reset": 1, "ltx2_dit_fbc_force_next": 2, "ltx2_dit_fbc_stats": 6, "ltx2_dit_forward_fbc": 9, "ltx2_dit_denoise_step_fbc": 9,
       "ltx2_dit_rescaled_guided_step_fbc": 13}


def test_abi_symbols():
    from ltx_2_mlx_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    docs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, n in NEW.items():
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == n == len(nv.SIGNATURES[name][1]) and nv.SIGNATURES[name][0] is nv.i32, name
        assert name in nv.exported_symbols() and name in docs, name
        for build in (None, torch.float16):
            assert hasattr(nv.lib(build), name), name
    assert nv.lib().ltx2_fbc_metric_blocks(0) == 0 and nv.lib().ltx2_fbc_metric_blocks(1) == 1
    assert nv.lib().ltx2_fbc_metric_blocks(8192) == 1 and nv.lib().ltx2_fbc_metric_blocks(8193) == 2 and nv.lib().ltx2_fbc_metric_blocks(1 << 40) == 1024
    # host-side refusals of the raw entries need no device
    assert nv.lib().ltx2_fbc_head_metric(None, None, None, None, None, None, None, 0.0, 4, None) == nv.E_INVALID
    assert "null operand" in nv.last_error()
    assert nv.lib().ltx2_fbc_apply_tail(None, None, 4, None) == nv.E_INVALID
    nv.last_error()


def test_python_surface():
    import ltx_2_mlx_amd.pipelines.common as PC
    from ltx_2_mlx_amd.model.transformer import LTXModel
    for name in ("enable_first_block_cache", "reset_first_block_cache", "first_block_cache_stats", "force_first_block_cache", "forward_cached",
                 "denoise_step_cached_", "rescaled_guided_step_cached_"):
        assert callable(getattr(LTXModel, name)), name
    p = inspect.signature(PC.standard_cfg_denoise_loop).parameters["first_block_cache"]
    assert p.default == 0.0
    line = PC.first_block_cache_summary([dict(evaluations=40, skips=11), dict(evaluations=40, skips=9)], 0.1)
    assert line == "first-block cache: 20 of 80 evaluations reused the tail (threshold 0.1)"


def test_loop_refusals():
    import ltx_2_mlx_amd.pipelines.common as PC
    fake = lambda av: SimpleNamespace(velocity_model=SimpleNamespace(is_av=av))      # noqa: E731
    st = SimpleNamespace(denoise_mask=torch.ones(1, 4, 1))
    with pytest.raises(ValueError, match="first_block_cache"):
        PC.standard_cfg_denoise_loop(fake(False), st, [1.0, 0.0], None, None, 3.0, 0.7, first_block_cache=-0.5)
    with pytest.raises(ValueError, match="first_block_cache"):
        PC.standard_cfg_denoise_loop(fake(False), st, [1.0, 0.0], None, None, 3.0, 0.7, first_block_cache=float("nan"))
    with pytest.raises(NotImplementedError, match="video-only model alone"):
        PC.standard_cfg_denoise_loop(fake(True), st, [1.0, 0.0], None, None, 3.0, 0.7, first_block_cache=0.1)
    with pytest.raises(NotImplementedError, match="fused"):
        PC.standard_cfg_denoise_loop(fake(False), st, [1.0, 0.0], None, None, 3.0, 0.7, fused=False, first_block_cache=0.1)
    with pytest.raises(ValueError, match="negative prompt"):
        PC.standard_cfg_denoise_loop(fake(False), st, [1.0, 0.0], None, None, 3.0, 0.7, first_block_cache=0.1)
    with pytest.raises(ValueError, match="denoise mask"):
        PC.standard_cfg_denoise_loop(fake(False), SimpleNamespace(denoise_mask=torch.zeros(1, 4, 1)), [1.0, 0.0], None, None, 1.0, 0.0, first_block_cache=0.1)


# ------------------------------------------------------------------ generate_video
def _request(tmp, **kw):
    import generate as gen
    base = {k: p.default for k, p in inspect.signature(gen.generate_video).parameters.items() if p.default is not inspect.Parameter.empty}
    base.update(prompt="p", use_gemma=False, device="cpu", height=64, width=64, num_frames=9, output_path=os.path.join(str(tmp), "o.mp4"))
    base.update(kw)
    return gen._resolve_request(base)


REFUSED = {
    "audiovideo": dict(generate_audio=True),
    "ltx23": dict(model_version="2.3"),
    "two_stage_distilled": dict(two_stage_distilled=True),
    "two_stage_cfg": dict(two_stage_cfg=True),
    "a2vid": dict(a2vid_two_stage=True, audio_path="a.wav"),
    "hq_audio": dict(ti2vid_hq_audio=True),
    "retake": dict(retake_video="clip.mp4"),
    "retake_audio": dict(retake_video="clip.mp4", retake_audio="replace"),
    "keyframe": dict(pipeline_type="keyframe-interpolation", keyframes=["a.png:0"]),
    "ic_lora": dict(pipeline_type="ic-lora", image_path="a.png"),
    "hq": dict(pipeline_type="ti2vid-hq"),
    "stg": dict(stg_scale=1.0, generate_audio=True),
    "stg_audio": dict(stg_audio_scale=1.0, generate_audio=True),
    "heun": dict(sampler="heun", generate_audio=True),
    "ancestral": dict(sampler="euler_ancestral", generate_audio=True),
    "ge": dict(ge_gamma=2.0, generate_audio=True),
    "apg": dict(apg_scale=2.0, generate_audio=True),
    "image": dict(image_path="a.png"),
    "placeholder": dict(use_placeholder=True),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_generate_video_refuses_every_other_route(tmp_path, case):
    with pytest.raises(NotImplementedError, match=r"first_block_cache=0\.1.*video-only standard loops alone"):
        _request(tmp_path, first_block_cache=0.1, **REFUSED[case])


def test_generate_video_threshold_and_defaults(tmp_path):
    import generate as gen
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="first_block_cache"):
            _request(tmp_path, first_block_cache=bad)
    p = inspect.signature(gen.generate_video).parameters["first_block_cache"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0.0
    # the default request resolves as before: the plain standard route, the captured graph, nothing of the cache handed on
    r = _request(tmp_path)
    assert r.route == "standard" and r.first_block_cache == 0.0 and r.use_hip_graph is True and not r.need_cfg and gen._first_block_cache_kw(r) == {}
    off = {k: v for k, v in vars(r).items() if k != "first_block_cache"}
    on = {k: v for k, v in vars(_request(tmp_path, first_block_cache=0.1)).items() if k != "first_block_cache"}
    assert off.keys() == on.keys() and all(off[k] is on[k] or off[k] == on[k] for k in off if k != "apg_guider")      # the option changes nothing else of the request
    # both routes that take it
    assert _request(tmp_path, first_block_cache=0.1).route == "standard"
    r = _request(tmp_path, first_block_cache=0.1, standard_cfg=True, model_variant="dev", cfg_scale=3.0)
    assert r.route == "standard_cfg" and gen._first_block_cache_kw(r) == dict(first_block_cache=0.1)
    # the CLI
    ps = gen.build_parser()
    assert gen.kwargs_from_args(ps.parse_args(["p", "--first-block-cache", "0.08"]))["first_block_cache"] == 0.08
    assert gen.kwargs_from_args(ps.parse_args(["p"]))["first_block_cache"] == 0.0
    assert "--first-block-cache" in open(os.path.join(ROOT, "README.md")).read()
