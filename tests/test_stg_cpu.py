"""Spatio-temporal guidance, the parts that need no GPU: the perturbation classes and STGGuider against hand-computed values, the exports and
the new ABI entries, generate_video's routing of stg_scale on stubs, tests/stg_ref against the plain guided loop, and the check that the
tiny case the GPU tests use is not vacuous."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stg_ref as R  # noqa: E402

NEW_ENTRIES = ("ltx2_stg_euler_step", "ltx2_dit_set_stg_blocks", "ltx2_dit_forward_perturbed", "ltx2_dit_forward_perturbed_av", "ltx2_dit_stg_step",
               "ltx2_dit_graph_capture_stg")


# ------------------------------------------------------------------ components
def test_perturbation_classes():
    from ltx_2_mlx_amd.components import (BatchedPerturbationConfig, Perturbation, PerturbationConfig, PerturbationType as PT,
                                          create_batched_stg_config, create_stg_perturbation)
    assert [t.value for t in PT] == ["skip_a2v_cross_attn", "skip_v2a_cross_attn", "skip_video_self_attn", "skip_audio_self_attn"]
    p = Perturbation(PT.SKIP_VIDEO_SELF_ATTN, [1, 3])
    assert p.is_perturbed(PT.SKIP_VIDEO_SELF_ATTN, 1) and p.is_perturbed(PT.SKIP_VIDEO_SELF_ATTN, 3)
    assert not p.is_perturbed(PT.SKIP_VIDEO_SELF_ATTN, 2) and not p.is_perturbed(PT.SKIP_AUDIO_SELF_ATTN, 1)
    every = Perturbation(PT.SKIP_AUDIO_SELF_ATTN)                         # blocks None: all of them
    assert every.blocks is None and all(every.is_perturbed(PT.SKIP_AUDIO_SELF_ATTN, b) for b in (0, 7, 47))
    with pytest.raises(Exception):
        p.blocks = None                                                   # frozen
    c = PerturbationConfig([p, every])
    assert c.is_perturbed(PT.SKIP_VIDEO_SELF_ATTN, 3) and c.is_perturbed(PT.SKIP_AUDIO_SELF_ATTN, 2) and not c.is_perturbed(PT.SKIP_VIDEO_SELF_ATTN, 0)
    assert not PerturbationConfig().is_perturbed(PT.SKIP_VIDEO_SELF_ATTN, 0) and PerturbationConfig().perturbations is None
    assert PerturbationConfig.empty().perturbations == [] and not PerturbationConfig.empty().is_perturbed(PT.SKIP_VIDEO_SELF_ATTN, 0)
    # a batch of three: perturbed in block 1, everywhere, nowhere
    b = BatchedPerturbationConfig([create_stg_perturbation(blocks=[1]), create_stg_perturbation(), PerturbationConfig.empty()])
    m = b.mask(PT.SKIP_VIDEO_SELF_ATTN, 1)
    assert isinstance(m, torch.Tensor) and m.dtype == torch.float32 and m.tolist() == [0.0, 0.0, 1.0]
    assert b.mask(PT.SKIP_VIDEO_SELF_ATTN, 0).tolist() == [1.0, 0.0, 1.0] and b.mask(PT.SKIP_AUDIO_SELF_ATTN, 1).tolist() == [1.0, 1.0, 1.0]
    assert b.mask(PT.SKIP_VIDEO_SELF_ATTN, 1, torch.float64).dtype == torch.float64
    like = b.mask_like(PT.SKIP_VIDEO_SELF_ATTN, 0, torch.zeros(3, 5, 7, dtype=torch.float64))
    assert like.shape == (3, 1, 1) and like.dtype == torch.float64 and like.flatten().tolist() == [1.0, 0.0, 1.0]
    assert b.any_in_batch(PT.SKIP_VIDEO_SELF_ATTN, 0) and not b.all_in_batch(PT.SKIP_VIDEO_SELF_ATTN, 0)
    assert not b.any_in_batch(PT.SKIP_AUDIO_SELF_ATTN, 0)
    e = BatchedPerturbationConfig.empty(2)
    assert len(e.perturbations) == 2 and e.mask(PT.SKIP_VIDEO_SELF_ATTN, 0).tolist() == [1.0, 1.0] and not e.any_in_batch(PT.SKIP_VIDEO_SELF_ATTN, 0)
    assert create_stg_perturbation(skip_video_self_attn=False).perturbations == []
    s = create_batched_stg_config(2, blocks=[29])
    assert len(s.perturbations) == 2 and s.all_in_batch(PT.SKIP_VIDEO_SELF_ATTN, 29) and not s.any_in_batch(PT.SKIP_VIDEO_SELF_ATTN, 28)
    assert create_batched_stg_config(1).all_in_batch(PT.SKIP_VIDEO_SELF_ATTN, 47)
    assert s.perturbations[0].perturbations[0] == Perturbation(PT.SKIP_VIDEO_SELF_ATTN, [29])


def test_stg_guider():
    from ltx_2_mlx_amd.components import STGGuider
    pos, pert = torch.tensor([1.0, 2.0, -3.0]), torch.tensor([0.5, 4.0, -3.0])
    g = STGGuider(2.0)
    assert g.delta(pos, pert).tolist() == [1.0, -4.0, 0.0] and g.guide(pos, pert).tolist() == [2.0, -2.0, -3.0]
    assert g.enabled() and not STGGuider(0.0).enabled() and STGGuider(-1.0).enabled()
    assert torch.equal(STGGuider(0.0).guide(pos, pert), pos)
    with pytest.raises(Exception):
        g.scale = 1.0                                                     # frozen


def test_exports():
    import ltx_2_mlx_amd.components as C
    import ltx_2_mlx_amd.pipelines as P
    for name in ("STGGuider", "PerturbationType", "Perturbation", "PerturbationConfig", "BatchedPerturbationConfig", "create_stg_perturbation",
                 "create_batched_stg_config"):
        assert name in C.__all__ and hasattr(C, name), name
    assert "stg_denoise_loop" in P.__all__ and callable(P.stg_denoise_loop)
    from ltx_2_mlx_amd.model.transformer import LTXModel
    for name in ("set_stg_blocks", "stg_step_", "capture_stg_graph", "replay_stg_graph"):
        assert callable(getattr(LTXModel, name)), name


def test_abi_declares_the_stg_entries():
    from ltx_2_mlx_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    assert re.search(r"#define LTX2_ABI_VERSION 3\b", header) and nv.ABI_VERSION == 3          # additive entries: no bump
    for name in NEW_ENTRIES:
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S)
        assert decl, name
        assert name in nv.SIGNATURES and nv.SIGNATURES[name][0] is nv.i32, name
        assert len(decl.group(1).split(",")) == len(nv.SIGNATURES[name][1]), name
    # the perturbed forwards take exactly the plain ones' arguments
    assert nv.SIGNATURES["ltx2_dit_forward_perturbed"] == nv.SIGNATURES["ltx2_dit_forward"]
    assert nv.SIGNATURES["ltx2_dit_forward_perturbed_av"] == nv.SIGNATURES["ltx2_dit_forward_av"]
    if os.path.exists(nv.LIB_PATH):
        assert all(hasattr(nv.lib(), n) for n in NEW_ENTRIES)


# ------------------------------------------------------------------ OneStagePipeline's own validation
def test_one_stage_validates_stg_itself():
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    gate = OneStagePipeline._require_no_guidance
    with pytest.raises(NotImplementedError, match="STG"):                 # the gate itself is as it was
        gate(1.0, None, 0.0, "euler", None, 1.0)

    class Stub:
        num_layers = 4
        device = torch.device("cpu")
    pipe = OneStagePipeline.__new__(OneStagePipeline)
    pipe.transformer, pipe.is_av_model = type("X", (), {"velocity_model": Stub()})(), False
    conf = OneStageCFGConfig(height=64, width=96, num_frames=9)
    enc = torch.zeros(1, 4, 8)
    with pytest.raises(ValueError, match=r"stg_blocks \[4\] out of range"):
        pipe(enc, enc, conf, stg_scale=1.0, stg_blocks=[0, 4])
    with pytest.raises(ValueError, match=r"stg_blocks \[-1\]"):
        pipe(enc, enc, conf, stg_scale=1.0, stg_blocks=[-1])
    for cutoff in (-0.1, 1.5):
        with pytest.raises(ValueError, match="stg_cutoff"):
            pipe(enc, enc, conf, stg_scale=1.0, stg_cutoff=cutoff)
    # the options that stay refused are still refused beside a valid STG request
    with pytest.raises(NotImplementedError, match="GE velocity"):
        pipe(enc, enc, conf, stg_scale=1.0, ge_gamma=0.5)
    with pytest.raises(NotImplementedError, match="sampler='heun'"):
        pipe(enc, enc, conf, stg_scale=1.0, sampler="heun")
    with pytest.raises(NotImplementedError, match="cross_attn_scale"):
        pipe(enc, enc, conf, stg_scale=1.0, cross_attn_scale=2.0)


# ------------------------------------------------------------------ generate_video(stg_scale=...)
def _call(tmp, route, **extra):
    from test_projected_guidance_cpu import _call as call
    return call(tmp, route, **extra)


REFUSED = "stg_scale=1.0 is outside the MI355X hot path (see DESIGN.md); leave it at its default 0.0"


@pytest.mark.parametrize("route", ["standard", "keyframe", "retake", "hq", "ic_lora", "two_stage"])
def test_stg_scale_stays_refused_off_the_av_route(route, tmp_path):
    seen, _ = _call(str(tmp_path), route, stg_scale=1.0)
    assert isinstance(seen.get("raised"), NotImplementedError), seen
    assert str(seen["raised"]) == REFUSED


def test_stg_scale_reaches_one_stage_pipeline(tmp_path):
    import generate as gen
    tmp = str(tmp_path)
    assert "stg_scale" in gen._ROUTE_OWNS["av"] and all("stg_scale" not in v for k, v in gen._ROUTE_OWNS.items() if k != "av")
    assert gen._OUT_OF_PATH_DEFAULTS["stg_scale"] == 0.0
    seen, lines = _call(tmp, "av", stg_scale=1.5, stg_blocks=[0, 1], stg_cutoff=0.8, model_variant="distilled")
    assert "raised" not in seen, seen
    k = seen["kwargs"]
    assert seen["pipeline"] == "OneStagePipeline" and (k["stg_scale"], k["stg_blocks"], k["stg_cutoff"]) == (1.5, [0, 1], 0.8)
    assert [l for l in lines if "STG" in l] == ["STG guidance: scale=1.5, mode=video", "  STG guidance enabled (scale=1.5)"]          # the reference's two lines
    seen, lines = _call(tmp, "av", stg_scale=1.0, model_variant="distilled")                      # the defaults: all blocks, every step
    assert (seen["kwargs"]["stg_blocks"], seen["kwargs"]["stg_cutoff"]) == (None, 1.0)
    seen, lines = _call(tmp, "av", model_variant="distilled")                                     # without the flag: no keyword, no line
    assert "stg_scale" not in seen["kwargs"] and not [l for l in lines if "STG" in l]
    # refused before any model loads
    seen, _ = _call(tmp, "av", stg_scale=1.0, stg_mode="both", model_variant="distilled")
    assert isinstance(seen.get("raised"), NotImplementedError) and "stg_mode='both'" in str(seen["raised"])
    seen, _ = _call(tmp, "av", stg_scale=0.0, stg_mode="both", model_variant="distilled")         # the mode alone is what the reference prints
    assert "raised" not in seen, seen
    seen, _ = _call(tmp, "av", stg_scale=1.0, stg_blocks=[48], model_variant="distilled")
    assert isinstance(seen.get("raised"), ValueError) and "stg_blocks [48] out of range" in str(seen["raised"])
    seen, _ = _call(tmp, "av", stg_scale=1.0, stg_blocks=[2], num_layers=2, model_variant="distilled")
    assert isinstance(seen.get("raised"), ValueError) and "the model has 2 layers" in str(seen["raised"])
    for cutoff in (-0.01, 1.01):
        seen, _ = _call(tmp, "av", stg_scale=1.0, stg_cutoff=cutoff, model_variant="distilled")
        assert isinstance(seen.get("raised"), ValueError) and "stg_cutoff" in str(seen["raised"])
    # the other refusals of the route table are as they were
    seen, _ = _call(tmp, "av", stg_scale=1.0, ge_gamma=0.5, model_variant="distilled")
    assert isinstance(seen.get("raised"), NotImplementedError) and "ge_gamma=0.5" in str(seen["raised"])
    seen, _ = _call(tmp, "standard", stg_scale=1.0, pipeline_type="two-stage")
    assert isinstance(seen.get("raised"), NotImplementedError) and str(seen["raised"]) == REFUSED


def test_cli_passes_the_stg_flags():
    import inspect
    import generate as gen
    a = gen.build_parser().parse_args(["p", "--generate-audio", "--stg-scale", "1.5", "--stg-blocks", "29", "30", "--stg-cutoff", "0.8"])
    k = gen.kwargs_from_args(a)
    assert (k["stg_scale"], k["stg_blocks"], k["stg_cutoff"], k["stg_mode"]) == (1.5, [29, 30], 0.8, "video")
    k = gen.kwargs_from_args(gen.build_parser().parse_args(["p"]))
    assert (k["stg_scale"], k["stg_blocks"], k["stg_cutoff"]) == (0.0, None, 1.0)
    sig = inspect.signature(gen.generate_video).parameters
    assert all(sig[n].kind == inspect.Parameter.KEYWORD_ONLY for n in ("stg_blocks", "stg_cutoff"))
    assert (sig["stg_blocks"].default, sig["stg_cutoff"].default) == (None, 1.0)
    assert sig["stg_scale"].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD


# ------------------------------------------------------------------ the restatement itself
@pytest.fixture(scope="module")
def case():
    return R.tiny_video()


def test_stg_ref_without_stg_is_the_guided_loop(case):
    import keyframe_ref as KR
    from oracle import dit
    from ltx_2_mlx_amd.components import LTX2Scheduler
    cfg, w, wq, lat, ctx, nctx, pos = case
    sig = [float(s) for s in LTX2Scheduler().execute(steps=2)]
    mask = torch.ones(1, lat.shape[1], 1)
    mask[0, :7] = 0.0
    clean = torch.zeros_like(lat)
    x0 = lambda c, ww: (lambda x, ts, s: dit.x0_model(x, c, ts, pos, ww, cfg))
    pert = x0(ctx, R.zero_self_attn_out(wq, None, cfg.num_layers))
    guide = lambda p, n: p + (3.0 - 1) * (p - n)
    plain = KR.guided_loop(lat, mask, clean, x0(ctx, wq), x0(nctx, wq), sig, 3.0)
    assert torch.equal(R.stg_loop(lat, mask, clean, x0(ctx, wq), x0(nctx, wq), pert, sig, guide, 0.0, 1.0), plain)
    assert torch.equal(R.stg_loop(lat, mask, clean, x0(ctx, wq), x0(nctx, wq), pert, sig, guide, 1.0, 0.0), plain)
    on = R.stg_loop(lat, mask, clean, x0(ctx, wq), x0(nctx, wq), pert, sig, guide, 1.0, 1.0)
    half = R.stg_loop(lat, mask, clean, x0(ctx, wq), x0(nctx, wq), pert, sig, guide, 1.0, 0.5)
    assert not torch.equal(on, plain) and not torch.equal(half, plain) and not torch.equal(half, on)          # step 1 of 2 alone is guided at 0.5
    # the element-wise step against the guided one at stg 0, and against STGGuider on the three x0
    g = torch.Generator().manual_seed(5)
    x, vc, vu, vp, cl = (torch.randn(9, 8, generator=g) for _ in range(5))
    ts, mk = torch.rand(9, generator=g), torch.tensor([0.0, 0.05, 1.0] * 3)
    assert torch.equal(R.stg_euler_step(x, vc, vu, vp, ts, mk, cl, 3.0, 0.0, 0.9, 0.7), KR.guided_euler_step(x, vc, vu, ts, mk, cl, 3.0, 0.9, 0.7))
    assert not torch.equal(R.stg_euler_step(x, vc, vu, vp, ts, mk, cl, 3.0, 1.0, 0.9, 0.7), KR.guided_euler_step(x, vc, vu, ts, mk, cl, 3.0, 0.9, 0.7))


def test_the_tiny_case_is_not_vacuous(case):
    """The GPU test accepts the engine's perturbed velocity within R.ENGINE_GATE (rel-L2) of the oracle's.  That says something only if the
    oracle's perturbed velocity is far from its unperturbed one on these weights: at least 10 x the gate, for every non-empty skip set."""
    from oracle import dit
    cfg, w, wq, lat, ctx, nctx, pos = case
    ts = torch.tensor([R.SIGMA])
    v = dit.velocity_model(lat, ctx, ts, pos, wq, cfg)
    for name, blocks in R.SKIP_SETS.items():
        vp = dit.velocity_model(lat, ctx, ts, pos, R.zero_self_attn_out(wq, blocks, cfg.num_layers), cfg)
        d = float((vp - v).norm() / v.norm())
        if name == "none":
            assert d == 0.0
        else:
            assert d >= 10 * R.ENGINE_GATE, (name, d)
