"""The joint audio+video guided step with a guider per modality, without a GPU: the C ABI's new entries, OneStagePipeline's choice of loop on
stubbed loops (it keeps the eager one: the device form measured no faster), the guider -> kernel-argument mapping, and the torch guiders on the GPU file's kernel inputs (finite references)."""
import os
import re

import pytest
import torch

import joint_projected_ref as JR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_symbols_and_exports():
    """The four new entries are exported, declared in the header with the binding's argument counts and named in INTEGRATION.md; the ABI
    version is still 3.  The Python layers above them exist."""
    import ltx_2_mlx_amd.pipelines as P
    from ltx_2_mlx_amd import _native as nv, kernels as K
    from ltx_2_mlx_amd.model.transformer import LTXModel
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    docs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define\s+LTX2_ABI_VERSION\s+3\b", header) and nv.ABI_VERSION == 3
    for name, n_args in (("ltx2_guidance_sums_pair", 23), ("ltx2_projected_euler_step_pair", 37), ("ltx2_dit_projected_step_joint_av", 31),
                         ("ltx2_dit_graph_capture_projected_joint_av", 29)):
        assert name in nv.SIGNATURES and name in nv.exported_symbols() and nv.SIGNATURES[name][0] is nv.i32, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == len(nv.SIGNATURES[name][1]) == n_args, name
        assert name in docs, name
    for name in ("guidance_sums_pair", "projected_euler_step_pair"):
        assert callable(getattr(K, name)), name
    assert K.PAIR_GUIDANCE_MODES == dict(cfg_star=0, apg=1, legacy_apg=2, cfg=3, off=4) and K.GUIDANCE_MODES == dict(cfg_star=0, apg=1, legacy_apg=2)
    for name in ("projected_step_joint_av_", "capture_projected_joint_graph", "replay_projected_joint_graph"):
        assert callable(getattr(LTXModel, name)), name
    assert hasattr(P, "joint_projected_denoise_loop") and "joint_projected_denoise_loop" in P.__all__


def test_guider_to_kernel_arguments():
    """joint_guider_args: the projected guiders as projected_guider_args gives them, mode 3 for a plain CFGGuider, mode 4 for None or a guider
    that is not enabled (whatever its class), None for an enabled object of another class."""
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider, LegacyStatefulAPGGuider, LtxAPGGuider
    from ltx_2_mlx_amd.pipelines.common import joint_guider_args, projected_guider_args
    assert joint_guider_args(CFGGuider(7.0)) == dict(mode=3, scale=7.0)
    for g in (CFGStarRescalingGuider(3.0), LtxAPGGuider(3.0, 0.5, 5.0), LegacyStatefulAPGGuider(2.0, 0.5, 5.0, 0.5)):
        assert joint_guider_args(g) == projected_guider_args(g) and joint_guider_args(g)["mode"] in (0, 1, 2)
    for g in (None, CFGGuider(1.0), CFGStarRescalingGuider(1.0), LtxAPGGuider(1.0)):
        assert joint_guider_args(g) == dict(mode=4, scale=1.0)

    class Other:
        def enabled(self):
            return True
    assert joint_guider_args(Other()) is None
    for mode in JR.SEGMENT_MODES:                    # the GPU file's segment modes are these guiders
        args, guider = JR.segment_guider(mode)
        assert joint_guider_args(guider) == args, mode


class _Model:
    """Enough of an AudioVideo LTXModel for OneStagePipeline up to its loop."""
    num_layers = 4
    device = torch.device("cpu")

    def __init__(self):
        from ltx_2_mlx_amd.model.transformer import LTXModelType
        self.model_type = LTXModelType.AudioVideo


@pytest.fixture
def routed(monkeypatch):
    """OneStagePipeline over the stub model with every loop it may call replaced by a recorder -> (pipe, calls)."""
    from ltx_2_mlx_amd.model.transformer import X0Model
    from ltx_2_mlx_amd.pipelines import OneStagePipeline, one_stage
    calls = []

    def stub(name, video_at, joint):
        def f(*a, **k):
            calls.append((name, a, k))
            return (a[video_at], a[video_at + 1]) if joint else a[video_at]
        return f
    monkeypatch.setattr(one_stage, "joint_denoise_loop", stub("joint", 2, True))
    monkeypatch.setattr(one_stage, "projected_denoise_loop", stub("projected", 1, False))
    monkeypatch.setattr(one_stage, "stg_denoise_loop", stub("stg", 1, False))
    return OneStagePipeline(X0Model(_Model()), None, None), calls


def test_one_stage_keeps_the_eager_joint_branch(routed):
    """The device form of the joint guided loop measured no faster than the eager one (profiles/joint_projected_step.md), so OneStagePipeline
    does not take it: cfg 3 / audio cfg 7 / rescale 0.7 with sound -- what the CLI passes for an LTX-2.3 dev checkpoint -- goes to
    joint_denoise_loop with both guiders and both negative contexts, with and without use_hip_graph, as do STG, a frozen audio latent, an
    override and an unguided run; a video-only override keeps projected_denoise_loop and an override of another class is refused as before."""
    from ltx_2_mlx_amd.components import CFGStarRescalingGuider, LtxAPGGuider
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, one_stage
    pipe, calls = routed
    assert not hasattr(one_stage, "joint_projected_denoise_loop")
    enc = torch.zeros(1, 4, 8)
    base = dict(height=64, width=96, num_frames=9, num_inference_steps=3)
    kw = dict(positive_audio_encoding=enc, negative_audio_encoding=enc)
    dev_conf = OneStageCFGConfig(use_hip_graph=True, audio_enabled=True, **base)
    assert (dev_conf.cfg_scale, dev_conf.audio_cfg_scale, dev_conf.rescale_scale) == (3.0, 7.0, 0.7)

    def route(conf=dev_conf, neg=enc, **extra):
        del calls[:]
        pipe(enc, neg, conf, **{**kw, **extra})
        assert len(calls) == 1
        return calls[0]

    name, a, k = route()
    assert name == "joint" and a[3].latent.shape == (1, 9, 128) and a[9] is True
    assert type(k["video_guider"]) is CFGStarRescalingGuider and type(k["audio_guider"]) is CFGStarRescalingGuider
    assert (k["video_guider"].scale, k["audio_guider"].scale) == (3.0, 7.0) and k["negative_video_context"] is not None and k["negative_audio_context"] is not None
    override = LtxAPGGuider(3.0, 0.5, 5.0)
    name, _, k = route(guider_override=override)
    assert name == "joint" and k["video_guider"] is override and type(k["audio_guider"]) is CFGStarRescalingGuider
    assert route(OneStageCFGConfig(use_hip_graph=False, audio_enabled=True, **base))[0] == "joint"
    assert route(stg_scale=1.0)[0] == "joint"
    assert route(initial_audio_latent=torch.zeros(1, 8, 9, 16))[0] == "joint"
    assert route(OneStageCFGConfig(use_hip_graph=True, audio_enabled=True, cfg_scale=1.0, audio_cfg_scale=1.0, **base), neg=None,
                 negative_audio_encoding=None)[0] == "joint"
    assert route(OneStageCFGConfig(use_hip_graph=True, use_internal_audio_branch=False, **base), guider_override=override)[0] == "projected"
    assert route(OneStageCFGConfig(use_hip_graph=True, use_internal_audio_branch=False, **base))[0] == "joint"
    with pytest.raises(NotImplementedError, match="guider_override"):
        route(guider_override=object())


def test_joint_projected_loop_refusals_before_the_device():
    from ltx_2_mlx_amd.components import CFGStarRescalingGuider, EulerDiffusionStep
    from ltx_2_mlx_amd.model.transformer import LTXModelType, X0Model
    from ltx_2_mlx_amd.pipelines import joint_projected_denoise_loop

    class M:
        is_av = False
        model_type = LTXModelType.VideoOnly
    g = CFGStarRescalingGuider(3.0)
    with pytest.raises(ValueError, match=r"requires an audio-video \(AV\) model"):
        joint_projected_denoise_loop(X0Model(M()), None, None, [1.0, 0.0], None, None, None, None, g, g, EulerDiffusionStep())
    av = M()
    av.is_av = True
    with pytest.raises(ValueError, match="audio state"):
        joint_projected_denoise_loop(X0Model(av), None, None, [1.0, 0.0], None, None, None, None, g, g, EulerDiffusionStep())
    with pytest.raises(ValueError, match="audio_encoding"):
        joint_projected_denoise_loop(X0Model(av), object(), object(), [1.0, 0.0], None, None, None, None, g, g, EulerDiffusionStep())

    class Other:
        def enabled(self):
            return True
    with pytest.raises(ValueError, match="a guider is a CFGGuider"):
        joint_projected_denoise_loop(X0Model(av), object(), object(), [1.0, 0.0], object(), object(), None, None, g, Other(), EulerDiffusionStep())


@pytest.mark.parametrize("v_rows,a_rows,C", JR.SHAPES)
def test_reference_inputs_are_finite(v_rows, a_rows, C):
    """The torch guiders on the GPU file's kernel inputs: every guided x0 is finite, the negative prediction is never all zero (CFG*'s
    projection divides by |uncond|^2 + 1e-8: the guider's own epsilon is not what keeps these inputs finite), and a guider moves its input."""
    import projected_guidance_ref as R
    for rows, seed in ((v_rows, 0), (a_rows, 1)):
        t = JR.inputs(rows, C, seed)
        assert all(bool(torch.isfinite(v).all()) for v in t.values())
        for per_row in (True, False):
            a, b = R.x0_pair(t["x"], t["vc"], t["vu"], t["ts_row"] if per_row else torch.tensor([0.909375]))
            assert float(b.double().pow(2).sum()) > 1e-3
            for mode in JR.SEGMENT_MODES:
                d = JR.guided_x0(t, mode, per_row)
                assert d.shape == a.shape and bool(torch.isfinite(d).all()), (rows, C, mode)
                assert torch.equal(d, a) == (mode == "off"), (rows, C, mode)
