"""The host side of the six device-resident sampling loops of pipelines/common.py, on the CPU with a recording fake LTXModel: what each loop
asks of the engine -- one capture or n steps, with which sigmas, with or without a negative context -- and when it calls back."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMAS = [1.0, 0.75, 0.5, 0.25, 0.0]                      # 4 steps, every value exact in fp32
LONG = [1.0 - i / 128 for i in range(65)]                 # 64 steps, ends on 0.5: no final res_2s step
F32 = lambda v: float(np.float32(v))                      # noqa: E731


class _Recorder:
    """Every public step / capture / replay method of LTXModel that the loops call, recorded."""

    def __init__(self, is_av=False):
        self.is_av, self.steps, self.captures, self.replays, self.prepared, self.neg = is_av, [], [], [], [], None

    def clone_sharing_weights(self):
        self.neg = _Recorder(self.is_av)
        return self.neg

    def prepare(self, context, positions, per_token=False, audio_context=None, audio_positions=None):
        self.prepared.append((context, per_token, audio_context))

    def set_stg_blocks(self, blocks):
        self.stg_blocks = blocks

    def _step(self, name, neg, sigma, sigma_next, **extra):
        self.steps.append(dict(name=name, neg=neg is not None, pair=(sigma, sigma_next), **extra))

    def denoise_step_(self, lat, video, sigma, sigma_next, denoise_mask=None, clean_latent=None):
        self._step("denoise_step_", None, sigma, sigma_next)

    def guided_step_(self, neg, lat, video, sigma, sigma_next, cfg_scale, denoise_mask=None, clean_latent=None):
        self._step("guided_step_", neg, sigma, sigma_next)

    def stg_step_(self, neg, lat, video, sigma, sigma_next, cfg_scale, stg_scale, vel_perturbed, denoise_mask=None, clean_latent=None):
        self._step("stg_step_", neg, sigma, sigma_next)

    def guided_step_av_(self, neg, lat, alat, video, audio, sigma, sigma_next, cfg_scale, denoise_mask=None, clean_latent=None):
        self._step("guided_step_av_", neg, sigma, sigma_next)

    def projected_step_(self, neg, lat, video, sigma, sigma_next, mode, scale, eta=1.0, norm_threshold=0.0, momentum=0.0, first=True,
                        denoise_mask=None, clean_latent=None):
        self._step("projected_step_", neg, sigma, sigma_next, first=first)

    def res2s_step_(self, neg, lat, video, video_sub, sigma, sigma_next, cfg_scale, denoise_mask=None, clean_latent=None):
        self._step("res2s_step_", neg, sigma, sigma_next)

    def res2s_step_av_(self, neg, lat, alat, video, audio, video_sub, audio_sub, sigma, sigma_next, cfg_scale, audio_cfg_scale, denoise_mask=None,
                       clean_latent=None, audio_denoise_mask=None, audio_clean_latent=None):
        self._step("res2s_step_av_", neg, sigma, sigma_next)

    def _capture(self, name, neg, sigmas):
        self.captures.append((name, neg is not None, list(sigmas)))

    def capture_guided_graph(self, neg, lat, sigmas, cfg_scale, denoise_mask=None, clean_latent=None):
        self._capture("guided", neg, sigmas)

    def capture_stg_graph(self, neg, lat, sigmas, cfg_scale, stg_scale, vel_perturbed, stg_cutoff=1.0, denoise_mask=None, clean_latent=None):
        self._capture("stg", neg, sigmas)

    def capture_guided_av_graph(self, neg, lat, alat, sigmas, cfg_scale, denoise_mask=None, clean_latent=None, audio_denoise_mask=None):
        self._capture("guided_av", neg, sigmas)

    def capture_projected_graph(self, neg, lat, sigmas, mode, scale, eta=1.0, norm_threshold=0.0, momentum=0.0, denoise_mask=None, clean_latent=None):
        self._capture("projected", neg, sigmas)

    def capture_res2s_graph(self, neg, lat, sigmas, cfg_scale, denoise_mask=None, clean_latent=None):
        self._capture("res2s", neg, sigmas)

    def replay_guided_graph(self):
        self.replays.append("guided")

    def replay_stg_graph(self):
        self.replays.append("stg")

    def replay_guided_av_graph(self):
        self.replays.append("guided_av")

    def replay_projected_graph(self):
        self.replays.append("projected")

    def replay_res2s_graph(self):
        self.replays.append("res2s")


class _FakeStream:
    def wait_stream(self, s):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


@pytest.fixture(autouse=True)
def _no_gpu_streams(monkeypatch):
    monkeypatch.setattr(torch.cuda, "Stream", _FakeStream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: _FakeStream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: s)


def _states():
    from ltx_2_mlx_amd.types import LatentState
    video = LatentState(latent=torch.zeros(1, 6, 8), denoise_mask=torch.ones(1, 6, 1), positions=torch.zeros(1, 3, 6, 2), clean_latent=torch.zeros(1, 6, 8))
    audio = LatentState(latent=torch.zeros(1, 5, 8), denoise_mask=torch.ones(1, 5, 1), positions=torch.zeros(1, 1, 5, 2), clean_latent=torch.zeros(1, 5, 8))
    return video, audio


class _X0:
    def __init__(self, is_av):
        self.velocity_model = _Recorder(is_av)


def _run(loop, sigmas, callback=None, use_hip_graph=True, cfg_scale=3.0, stg_cutoff=1.0):
    """One call of the loop named `loop` -> the recording model."""
    from ltx_2_mlx_amd.components.guiders import CFGGuider, CFGStarRescalingGuider, STGGuider
    from ltx_2_mlx_amd.pipelines import common
    st, ast = _states()
    ctx, nctx, actx = torch.zeros(1, 4, 8), torch.ones(1, 4, 8), torch.full((1, 4, 8), 2.0)
    x = _X0(loop in ("frozen_audio", "res2s_av"))
    if loop == "guided":
        common.guided_denoise_loop(x, st, sigmas, ctx, nctx, CFGGuider(cfg_scale), None, callback, use_hip_graph)
    elif loop == "stg":
        common.stg_denoise_loop(x, st, sigmas, ctx, nctx, CFGGuider(cfg_scale), STGGuider(1.0), None, stg_cutoff, None, callback, use_hip_graph)
    elif loop == "frozen_audio":
        frozen = ast.replace(denoise_mask=torch.zeros(1, 5, 1))
        common.frozen_audio_guided_loop(x, st, frozen, sigmas, ctx, actx, nctx, None, cfg_scale, None, callback, use_hip_graph)
    elif loop == "projected":
        common.projected_denoise_loop(x, st, sigmas, ctx, nctx, CFGStarRescalingGuider(cfg_scale), None, callback, use_hip_graph)
    elif loop == "res2s":
        common.res2s_denoise_loop(x, st, sigmas, ctx, nctx, cfg_scale, 1.0, callback, use_hip_graph)
    else:
        common.res2s_av_denoise_loop(x, st, ast, sigmas, ctx, actx, nctx, actx, cfg_scale, 1.0, callback, use_hip_graph)
    return x.velocity_model


# loop -> (the kind of its capture, None: the loop has no captured form; its step method; whether it injects the res_2s sigma)
LOOPS = {
    "guided": ("guided", "guided_step_", False),
    "stg": ("stg", "stg_step_", False),
    "frozen_audio": ("guided_av", "guided_step_av_", False),
    "projected": ("projected", "projected_step_", False),
    "res2s": ("res2s", "res2s_step_", True),
    "res2s_av": (None, "res2s_step_av_", True),
}


def _used(sigmas, res2s):
    """The sigma list the engine sees: a res_2s loop replaces a trailing 0.0 by 0.0011 and rounds to fp32."""
    if res2s and sigmas[-1] == 0.0:
        sigmas = sigmas[:-1] + [0.0011]
    return [F32(s) for s in sigmas] if res2s else list(sigmas)


def _pairs(used):
    return [(used[i], used[i + 1]) for i in range(len(used) - 1)]


@pytest.mark.parametrize("loop", list(LOOPS))
def test_no_callback_is_one_capture(loop):
    kind, step, res2s = LOOPS[loop]
    m = _run(loop, SIGMAS)
    if kind is None:                    # the joint res_2s loop never captures
        assert m.captures == [] and m.replays == [] and [s["pair"] for s in m.steps] == _pairs(_used(SIGMAS, res2s))
        return
    assert m.captures == [(kind, True, _used(SIGMAS, res2s))] and m.replays == [kind] and m.steps == []
    assert m.neg is not None and m.neg.captures == [] and m.neg.steps == []


@pytest.mark.parametrize("loop", list(LOOPS))
def test_callback_is_n_steps_in_order(loop):
    kind, step, res2s = LOOPS[loop]
    seen = []
    m = _run(loop, SIGMAS, callback=lambda i, n: seen.append((i, n)))
    assert m.captures == [] and m.replays == []
    assert [s["name"] for s in m.steps] == [step] * 4 and all(s["neg"] for s in m.steps)
    assert [s["pair"] for s in m.steps] == _pairs(_used(SIGMAS, res2s))
    assert seen == [(1, 4), (2, 4), (3, 4), (4, 4)]


@pytest.mark.parametrize("loop", list(LOOPS))
def test_64_steps_are_not_captured(loop):
    kind, step, res2s = LOOPS[loop]
    m = _run(loop, LONG)
    assert m.captures == [] and m.replays == [] and [s["name"] for s in m.steps] == [step] * 64
    assert [s["pair"] for s in m.steps] == _pairs(_used(LONG, res2s))


@pytest.mark.parametrize("loop", list(LOOPS))
def test_use_hip_graph_false_is_not_captured(loop):
    kind, step, res2s = LOOPS[loop]
    m = _run(loop, SIGMAS, use_hip_graph=False)
    assert m.captures == [] and m.replays == [] and [s["pair"] for s in m.steps] == _pairs(_used(SIGMAS, res2s))


@pytest.mark.parametrize("cutoff", [0.0, 0.25, 0.3, 0.5, 0.75, 1.0])
@pytest.mark.parametrize("cfg_scale", [3.0, 1.0])
def test_stg_loop_switches_at_the_cutoff(cutoff, cfg_scale):
    """An STG step while (i + 1) / n <= cutoff; from the first i past it the guided step, or the plain one when the CFG guider is not enabled."""
    m = _run("stg", SIGMAS, callback=lambda i, n: None, cfg_scale=cfg_scale, stg_cutoff=cutoff)
    guided = cfg_scale != 1.0
    first_past = next((i for i in range(4) if (i + 1) / 4 > cutoff), 4)
    after = "guided_step_" if guided else "denoise_step_"
    assert [s["name"] for s in m.steps] == ["stg_step_"] * first_past + [after] * (4 - first_past)
    assert all(s["neg"] == (guided and s["name"] != "denoise_step_") for s in m.steps) and (m.neg is not None) == guided
    assert [s["pair"] for s in m.steps] == _pairs(SIGMAS)
    m = _run("stg", SIGMAS, cfg_scale=cfg_scale, stg_cutoff=cutoff)
    assert m.captures == [("stg", guided, SIGMAS)] and m.steps == []


def test_projected_loop_starts_the_running_guidance_once():
    m = _run("projected", SIGMAS, callback=lambda i, n: None)
    assert [s["first"] for s in m.steps] == [True, False, False, False]


@pytest.mark.parametrize("callback", [None, lambda i, n: None])
def test_frozen_audio_loop_prepares_both_contexts_per_token(callback):
    m = _run("frozen_audio", SIGMAS, callback=callback)
    assert len(m.prepared) == 1 and len(m.neg.prepared) == 1
    assert m.prepared[0][1] is True and m.neg.prepared[0][1] is True
    assert m.prepared[0][2] is not None and m.neg.prepared[0][2] is m.prepared[0][2]      # no negative audio context: the positive one stands in
