"""Projected guidance, the parts that need no GPU: the two APG guiders against the vectors recorded from the reference's own classes
(tests/golden/apg_guiders.npz, tools/pin_apg_against_reference.py), reset() and enabled(), generate_video's routing of apg_scale on stubs,
OneStagePipeline's gate and the new ABI entries."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEW_ENTRIES = ("ltx2_guidance_sums_blocks", "ltx2_guidance_sums", "ltx2_projected_euler_step", "ltx2_dit_projected_step", "ltx2_dit_graph_capture_projected")
TOL = dict(rtol=1e-5, atol=1e-5)          # test_guiders_match_reference's


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "apg_guiders.npz"))
    return {k: z[k] for k in z.files}


def test_apg_guiders_match_reference(golden):
    from ltx_2_mlx_amd.components import LegacyStatefulAPGGuider, LtxAPGGuider
    cond, uncond = torch.from_numpy(golden["cond"]), torch.from_numpy(golden["uncond"])
    assert len(golden["settings"]) >= 5
    norm = float((cond - uncond).norm())
    assert any(0 < t < norm for _, _, t in golden["settings"]) and any(t > norm for _, _, t in golden["settings"])      # one binds, one does not
    for i, (scale, eta, thr) in enumerate(golden["settings"]):
        got = LtxAPGGuider(float(scale), float(eta), float(thr)).guide(cond, uncond)
        assert np.allclose(got.numpy(), golden[f"apg_{i}"], **TOL), (scale, eta, thr)
    assert torch.equal(LtxAPGGuider(1.0).guide(cond, uncond), cond)
    scale, eta, thr, mom = (float(v) for v in golden["legacy"])
    g = LegacyStatefulAPGGuider(scale, eta, thr, mom)
    for k, f in enumerate(golden["uncond_factors"]):
        got = g.guide(cond, uncond * float(f))
        assert np.allclose(got.numpy(), golden[f"legacy_{k}"], **TOL), k
        assert np.allclose(g.running_avg.numpy(), golden[f"legacy_running_{k}"], **TOL), k
    assert not np.allclose(golden["legacy_1"], golden["legacy_0"], **TOL)
    stateless = LegacyStatefulAPGGuider(3.0, 0.5)
    assert np.allclose(stateless.guide(cond, uncond).numpy(), golden["legacy_stateless"], **TOL) and stateless.running_avg is None


def test_defaults_reset_and_enabled(golden):
    import dataclasses
    from ltx_2_mlx_amd.components import LegacyStatefulAPGGuider, LtxAPGGuider
    d = lambda cls: {f.name: f.default for f in dataclasses.fields(cls)}
    assert {k: d(LtxAPGGuider)[k] for k in ("eta", "norm_threshold")} == dict(eta=1.0, norm_threshold=0.0)
    assert {k: d(LegacyStatefulAPGGuider)[k] for k in ("norm_threshold", "momentum", "running_avg")} == dict(norm_threshold=5.0, momentum=0.0, running_avg=None)
    with pytest.raises(TypeError):
        LegacyStatefulAPGGuider(3.0)                    # eta has no default there
    assert not LtxAPGGuider(1.0).enabled() and LtxAPGGuider(3.0).enabled() and LtxAPGGuider(0.0).enabled()
    assert not LegacyStatefulAPGGuider(0.0, 1.0).enabled() and LegacyStatefulAPGGuider(1.0, 1.0).enabled()
    cond, uncond = torch.from_numpy(golden["cond"]), torch.from_numpy(golden["uncond"])
    g = LegacyStatefulAPGGuider(3.0, 0.5, 5.0, 0.5)
    first = g.guide(cond, uncond)
    second = g.guide(cond, uncond)
    assert g.running_avg is not None and not torch.equal(first, second)
    g.reset()
    assert g.running_avg is None and torch.equal(g.guide(cond, uncond), first)
    assert torch.equal(g.running_avg, cond - uncond)                      # the first call after reset() keeps the guidance itself


def test_require_no_guidance_accepts_the_four_guider_classes():
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider, LegacyStatefulAPGGuider, LtxAPGGuider
    from ltx_2_mlx_amd.pipelines import OneStagePipeline
    gate = OneStagePipeline._require_no_guidance
    base = dict(stg_scale=0.0, ge_gamma=0.0, sampler="euler", temporal_upscaler=None, cross_attn_scale=1.0)
    for guider in (CFGGuider(3.0), CFGStarRescalingGuider(3.0), LtxAPGGuider(3.0, 0.5, 5.0), LegacyStatefulAPGGuider(3.0, 0.5, 5.0, 0.5), None):
        gate(guider_override=guider, **base)

    class Mine(CFGGuider):
        pass

    for other in (object(), Mine(3.0), "apg"):
        with pytest.raises(NotImplementedError, match="guider_override"):
            gate(guider_override=other, **base)


def test_projected_guider_args():
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider, LegacyStatefulAPGGuider, LtxAPGGuider
    from ltx_2_mlx_amd.pipelines.common import projected_guider_args
    assert projected_guider_args(CFGStarRescalingGuider(3.0)) == dict(mode=0, scale=3.0, eta=1.0, norm_threshold=0.0, momentum=0.0)
    assert projected_guider_args(LtxAPGGuider(3.0, 0.5, 5.0)) == dict(mode=1, scale=3.0, eta=0.5, norm_threshold=5.0, momentum=0.0)
    assert projected_guider_args(LegacyStatefulAPGGuider(2.0, 0.5, 4.0, 0.25)) == dict(mode=2, scale=2.0, eta=0.5, norm_threshold=4.0, momentum=0.25)
    assert projected_guider_args(CFGGuider(3.0)) is None and projected_guider_args(object()) is None


# ------------------------------------------------------------------ generate_video(apg_scale=...)
def _call(tmp, route, **extra):
    """One generate_video call on test_generate_routes_cpu's stubs, with the three pipelines that take a guider replaced by recorders
    -> (what the pipeline's __call__ was given, or the exception; the printed lines)."""
    import test_generate_routes_cpu as G
    import ltx_2_mlx_amd.pipelines as P
    paths = G._files(tmp)
    fill = lambda v: [fill(x) for x in v] if isinstance(v, list) else (next((v.replace(k, p) for k, p in paths.items() if k in v), v) if isinstance(v, str) else v)
    kw = dict(use_gemma=False, device="cpu", save_mp4=False, output_path=os.path.join(tmp, "out", "o.mp4"), seed=7)
    kw.update({k: fill(v) for k, v in dict(G.ROUTES[route], **extra).items()})
    seen = {}

    def recorder(name):
        class Pipe:
            token_counts = [16, 64]

            def __init__(self, *a, **k):
                pass

            def __call__(self, *a, **k):
                seen.update(pipeline=name, kwargs=k)
                conf = next(v for v in list(a) + list(k.values()) if type(v).__name__.endswith("Config"))
                size = (17, 64, 96) if name == "RetakePipeline" else (conf.num_frames, conf.height, conf.width)
                frames = torch.zeros(*size, 3, dtype=torch.uint8)
                return (frames, torch.zeros(1, 8, 3, 16)) if name == "OneStagePipeline" else frames
        return Pipe

    out = io.StringIO()
    with pytest.MonkeyPatch.context() as mp:
        gen = G._stub_everything(mp, [], [], lambda s: s)
        for name in ("KeyframeInterpolationPipeline", "RetakePipeline", "OneStagePipeline"):
            mp.setattr(P, name, recorder(name))
        with contextlib.redirect_stdout(out):
            try:
                gen.generate_video("a prompt", **kw)
            except Exception as e:  # noqa: BLE001
                seen["raised"] = e
    return seen, out.getvalue().splitlines()


@pytest.mark.parametrize("route", ["standard", "hq", "ic_lora", "two_stage"])
def test_apg_scale_is_refused_where_no_guided_loop_takes_it(route, tmp_path):
    seen, _ = _call(str(tmp_path), route, apg_scale=3.0)
    assert isinstance(seen.get("raised"), NotImplementedError), seen
    assert str(seen["raised"]) == "apg_scale=3.0 is outside the MI355X hot path (see DESIGN.md); leave it at its default 1.0"


def test_apg_scale_is_refused_on_the_distilled_routes(tmp_path):
    for kw in (dict(pipeline_type="distilled"), dict(pipeline_type="one-stage")):
        seen, _ = _call(str(tmp_path), "standard", apg_scale=3.0, **kw)
        assert isinstance(seen.get("raised"), NotImplementedError) and "apg_scale=3.0" in str(seen["raised"])
    seen, _ = _call(str(tmp_path), "retake", apg_scale=3.0, model_variant="distilled")          # the distilled retake runs without guidance
    assert isinstance(seen.get("raised"), NotImplementedError) and "apg_scale=3.0" in str(seen["raised"])


def test_apg_scale_reaches_the_pipelines(tmp_path):
    from ltx_2_mlx_amd.components import LegacyStatefulAPGGuider, LtxAPGGuider
    tmp = str(tmp_path)
    banner = ["APG guidance: scale=3.0, eta=0.5, norm_threshold=5.0", "  APG guidance enabled (replaces standard CFG)"]
    for route, pipeline, key in (("keyframe", "KeyframeInterpolationPipeline", "guider"), ("retake", "RetakePipeline", "guider")):
        seen, lines = _call(tmp, route, apg_scale=3.0, apg_eta=0.5, apg_norm_threshold=5.0)
        assert "raised" not in seen, seen
        g = seen["kwargs"][key]
        assert seen["pipeline"] == pipeline and type(g) is LtxAPGGuider and (g.scale, g.eta, g.norm_threshold) == (3.0, 0.5, 5.0)
        assert [l for l in lines if "APG" in l] == banner
        seen, lines = _call(tmp, route)                                   # without the flag: no guider keyword, no line
        assert key not in seen["kwargs"] and not [l for l in lines if "APG" in l]
    # momentum > 0: the stateful guider, and the reference's extra line
    seen, lines = _call(tmp, "keyframe", apg_scale=3.0, apg_eta=0.5, apg_norm_threshold=5.0, apg_momentum=0.5)
    g = seen["kwargs"]["guider"]
    assert type(g) is LegacyStatefulAPGGuider and (g.scale, g.eta, g.norm_threshold, g.momentum) == (3.0, 0.5, 5.0, 0.5)
    assert [l for l in lines if "APG" in l] == [banner[0], "  Using stateful APG with momentum=0.5", banner[1]]
    # the AudioVideo route: guidance needs the negative encodings, here from the embedding file
    emb = os.path.join(tmp, "emb.npz")
    np.savez(emb, **{k: np.ones((4, 16), np.float32) for k in ("embedding", "audio_embedding", "negative_embedding", "negative_audio_embedding")})
    seen, lines = _call(tmp, "av", apg_scale=3.0, apg_eta=0.5, apg_norm_threshold=5.0, embedding_path=emb)
    assert "raised" not in seen, seen
    g = seen["kwargs"]["guider_override"]
    assert seen["pipeline"] == "OneStagePipeline" and type(g) is LtxAPGGuider and (g.scale, g.eta, g.norm_threshold) == (3.0, 0.5, 5.0)
    assert seen["kwargs"]["negative_encoding"] is not None and seen["kwargs"]["negative_audio_encoding"] is not None
    assert [l for l in lines if "APG" in l] == banner
    seen, _ = _call(tmp, "av", apg_scale=3.0)                             # guided, and no negative encodings anywhere
    assert isinstance(seen.get("raised"), NotImplementedError) and "NEGATIVE" in str(seen["raised"])
    seen, _ = _call(tmp, "av")
    assert "guider_override" not in seen["kwargs"]


def test_cli_passes_the_apg_flags():
    import generate as gen
    a = gen.build_parser().parse_args(["p", "--apg-scale", "3", "--apg-eta", "0.5", "--apg-norm-threshold", "5", "--apg-momentum", "0.5"])
    assert (a.apg_scale, a.apg_eta, a.apg_norm_threshold, a.apg_momentum) == (3.0, 0.5, 5.0, 0.5)


def test_abi_declares_the_projected_entries():
    from ltx_2_mlx_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    assert re.search(r"#define LTX2_ABI_VERSION 3\b", header) and nv.ABI_VERSION == 3
    for name in NEW_ENTRIES:
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S)
        assert decl, name
        assert name in nv.SIGNATURES and nv.SIGNATURES[name][0] is nv.i32, name
        assert len(decl.group(1).split(",")) == len(nv.SIGNATURES[name][1]), name
    lib = nv.lib() if os.path.exists(nv.LIB_PATH) else None
    if lib is not None:
        assert all(hasattr(lib, n) for n in NEW_ENTRIES)
        assert lib.ltx2_guidance_sums_blocks(37, 128) == 5 and lib.ltx2_guidance_sums_blocks(33000, 128) == 1024 and lib.ltx2_guidance_sums_blocks(0, 128) == 0
