"""generate_video's seven routes on stubs, without a GPU: for one toy call per route, the ordered list of loader / model / pipeline calls, the
keywords every pipeline *Config was built with, the printed lines (timings masked) and the files written; and for conflicting arguments, which
error wins.  The expected values in tests/golden/generate_routes.json are a recording of the code, not a derivation: run this file as a script
to record them again after a deliberate change of behaviour."""
import contextlib
import dataclasses
import io
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
if ROOT not in sys.path:          # run as a script, without the suite's conftest
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "generate_routes.json")

PIPELINES = ("KeyframeInterpolationPipeline", "TI2VidHQPipeline", "ICLoraPipeline", "RetakePipeline", "DistilledPipeline", "OneStagePipeline")
CONFIGS = ("KeyframeInterpolationConfig", "TI2VidHQConfig", "ICLoraConfig", "RetakeConfig", "DistilledConfig", "OneStageCFGConfig")
SMALL, MID = dict(height=64, width=64, num_frames=9), dict(height=128, width=128, num_frames=9)       # MID: the configs that want multiples of 64

# route -> keywords of its one successful call; a "<name>" value stands for a file made in the run's directory (_files)
ROUTES = {
    "keyframe": dict(MID, pipeline_type="keyframe-interpolation", keyframes=["<img>:0", "<img>:8:0.9"], model_variant="dev", cfg_scale=3.0, num_steps=5),
    "hq": dict(MID, pipeline_type="ti2vid-hq", spatial_upscaler_weights="random", image_path="<img>", model_variant="dev", cfg_scale=3.0, num_steps=4,
               distilled_lora="<lora>", distilled_lora_scale=0.5),
    "ic_lora": dict(MID, pipeline_type="ic-lora", control_video="<ctl>", control_type="canny", save_control=True, image_path="<img>",
                    spatial_upscaler_weights="<missing>", ic_lora_weights="<lora>", vae_base_channels=16),
    "retake": dict(retake_video="<clip>", retake_start_time=0.4, retake_composite=True, model_variant="dev", cfg_scale=3.0, output_fps=30, tiled_vae=True),
    "two_stage": dict(MID, two_stage_distilled=True, spatial_upscaler_weights="random", image_path="<img>"),
    "av": dict(SMALL, generate_audio=True, decode_audio=False, image_path="<img>", num_steps=6),
    "standard": dict(SMALL, upscale_spatial=True, spatial_upscaler_weights="random", upscale_temporal=True, temporal_upscaler_weights="<missing>",
                     vae_base_channels=16, low_memory=True),
    "standard_placeholder": dict(SMALL, use_placeholder=True, skip_vae=True, upscale_spatial=True, spatial_upscaler_weights="random",
                                 upscale_temporal=True, temporal_upscaler_weights="random", temporal_upscaler_checkpoint_semantics=True),
}
# (route whose keywords are the base, the conflicting keywords): the first error, or the early return, of each is pinned
CONFLICTS = [
    ("keyframe", dict(generate_audio=True)), ("keyframe", dict(stg_scale=1.0, image_path="<img>")), ("keyframe", dict(height=96)),
    ("keyframe", dict(keyframes=["<img>:9"])), ("keyframe", dict(use_placeholder=True)), ("keyframe", dict(skip_vae=True)),
    ("hq", dict(upscale_temporal=True)), ("hq", dict(spatial_upscaler_weights=None, num_frames=10)), ("hq", dict(fp8_resident=True)),
    ("hq", dict(distilled_lora="<missing>")), ("hq", dict(use_placeholder=True)),
    ("ic_lora", dict(keyframes=["<img>:0"])), ("ic_lora", dict(control_type="bogus", control_video="<missing>")), ("ic_lora", dict(control_video="<missing>")),
    ("ic_lora", dict(fp8_resident=True)), ("ic_lora", dict(skip_vae=True)),
    ("retake", dict(pipeline_type="distilled", stg_scale=1.0)), ("retake", dict(retake_start_time=5.0, retake_end_time=6.0)),
    ("retake", dict(retake_end_time=0.2)), ("retake", dict(compute_dtype="float32")), ("retake", dict(use_placeholder=True)),
    ("two_stage", dict(audio_path="<img>", upscale_temporal=True)), ("two_stage", dict(upscale_temporal=True)),
    ("two_stage", dict(spatial_upscaler_weights=None, skip_vae=True)), ("two_stage", dict(skip_vae=True, use_placeholder=True)),
    ("two_stage", dict(use_placeholder=True)),
    ("av", dict(audio_path="<missing>", upscale_temporal=True)), ("av", dict(upscale_temporal=True)), ("av", dict(model_variant="dev", cfg_scale=1.0)),
    ("av", dict(upscale_spatial=True)), ("av", dict(use_placeholder=True)), ("av", dict(skip_vae=True)),
    ("standard", dict(model_variant="dev", cfg_scale=3.0)), ("standard", dict(num_frames=10, height=48)), ("standard", dict(use_fp16=False)),
    ("standard", dict(pipeline_type="two-stage")), ("standard", dict(pipeline_type="bogus", stg_scale=1.0)), ("standard", dict(audio_path="<img>")),
    ("standard", dict(negative_prompt="no")), ("standard", dict(use_gemma=True, gemma_path="<missing>")), ("standard", dict(lora_path="<lora>")),
]


def _files(tmp):
    """The input files the calls name; returns placeholder -> path."""
    from PIL import Image
    paths = {k: os.path.join(tmp, v) for k, v in (("<img>", "i.png"), ("<lora>", "lora.safetensors"), ("<ctl>", "ctl.npy"), ("<clip>", "clip.npy"),
                                                   ("<missing>", "missing.safetensors"))}
    Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(paths["<img>"])
    open(paths["<lora>"], "wb").close()
    np.save(paths["<ctl>"], np.zeros((9, 128, 128, 3), np.uint8))
    np.save(paths["<clip>"], np.zeros((20, 64, 96, 3), np.uint8))          # 20 frames are snapped to 17
    return paths


class _Named:
    """A stand-in whose every use is logged under its name."""

    def __init__(self, name, log):
        self.name, self.log = name, log

    def init_random_weights(self, seed=0):
        self.log.append(f"{self.name}.init_random_weights(seed={seed})")


def _plain(x, mask):
    """A call's arguments as JSON: stand-ins by name, tensors by shape, records by type name, the rest by repr with the run's directory masked."""
    if isinstance(x, _Named):
        return f"<{x.name}>"
    if isinstance(x, torch.Tensor):
        return f"tensor{tuple(x.shape)}" + ("=0" if not x.any() else "")
    if isinstance(x, (list, tuple)):
        return [_plain(v, mask) for v in x]
    if isinstance(x, dict):
        return {k: _plain(v, mask) for k, v in x.items()}
    if dataclasses.is_dataclass(x) and type(x).__name__ in CONFIGS:
        return f"<{type(x).__name__}>"
    if callable(x) and hasattr(x, "__name__"):
        return f"<function {x.__name__}>"
    return mask(repr(x))


def _stub_everything(mp, log, configs, mask):
    import generate as gen
    import ltx_2_mlx_amd.model.upscaler as U
    import ltx_2_mlx_amd.pipelines as P
    from ltx_2_mlx_amd.pipelines import common

    def called(name, result):
        def f(*a, **k):
            log.append([name, _plain(a, mask), _plain(k, mask)])
            return result(*a, **k) if callable(result) else result
        return f

    def module(name):
        def make(*a, **k):
            log.append([name, _plain(a, mask), _plain(k, mask)])
            return _Named(name, log)
        return make

    class Velocity(_Named):
        def prepare(self, context, positions):
            self.log.append(["velocity_model.prepare", _plain([context, positions], mask)])

        def capture_denoise_graph(self, lat, sigmas):
            self.log.append(["velocity_model.capture_denoise_graph", _plain(lat, mask), [round(float(s), 6) for s in sigmas]])

        def replay_denoise_graph(self):
            self.log.append("velocity_model.replay_denoise_graph")

    def x0(transformer):
        m = _Named("X0Model", log)
        m.velocity_model = Velocity("velocity_model", log)
        return m

    class Stream:
        def __init__(self, name="side"):
            self.name = name

        def wait_stream(self, other):
            log.append(f"{self.name} stream waits for {other.name}")

        def __enter__(self):
            log.append("enter side stream")

        def __exit__(self, *a):
            log.append("exit side stream")
            return False

    mp.setattr(torch.cuda, "synchronize", lambda *a: None)
    mp.setattr(torch.cuda, "Stream", Stream)
    mp.setattr(torch.cuda, "current_stream", lambda *a: Stream("current"))
    mp.setattr(torch.cuda, "stream", lambda s: s)
    mp.setattr(gen, "create_dummy_text_encoding", called("create_dummy_text_encoding", lambda prompt, embed_dim=3840, **k: (torch.ones(1, 4, 16), None)))
    mp.setattr(gen, "load_transformer", called("load_transformer", lambda *a, **k: _Named("transformer", log)))
    mp.setattr(gen, "load_av_transformer", called("load_av_transformer", lambda *a, **k: _Named("av_transformer", log)))
    mp.setattr(gen, "X0Model", x0)

    def vae_decoder(*a, **k):
        d = _Named("vae_decoder", log)
        d.per_channel_statistics = types.SimpleNamespace(mean_of_means="<mean_of_means>", std_of_means="<std_of_means>")
        return d

    mp.setattr(gen, "create_vae_decoder", called("create_vae_decoder", vae_decoder))
    mp.setattr(gen, "SimpleVideoEncoder", module("SimpleVideoEncoder"))
    mp.setattr(U, "SpatialUpscaler", module("SpatialUpscaler"))
    mp.setattr(U, "TemporalUpscaler", module("TemporalUpscaler"))
    mp.setattr(U, "upscale_latent", called("upscale_latent", lambda lat, *a: lat.repeat_interleave(2, 3).repeat_interleave(2, 4)))
    mp.setattr(U, "upscale_latent_temporal", called("upscale_latent_temporal", lambda lat, *a: torch.cat([lat, lat[:, :, 1:]], dim=2)))
    decode = called("decode_latent", lambda lat, dec: torch.zeros(8 * (lat.shape[2] - 1) + 1, 32 * lat.shape[3], 32 * lat.shape[4], 3, dtype=torch.uint8))
    mp.setattr(common, "decode_latent", decode)
    mp.setattr(gen, "decode_latent", decode, raising=False)          # whichever of the two namespaces the standard route decodes through

    def config(name):
        real = getattr(P, name)

        def make(*a, **k):
            configs.append([name, _plain(a, mask), _plain(k, mask)])
            return real(*a, **k)
        return make

    for name in CONFIGS:
        mp.setattr(P, name, config(name))

    def pipeline(name):
        class Pipe:
            token_counts = [16, 64]

            def __init__(self, *a, **k):
                log.append([name, _plain(a, mask), _plain(k, mask)])

            def __call__(self, *a, **k):
                log.append([name + ".__call__", _plain(a, mask), _plain(k, mask)])
                conf = next(v for v in list(a) + list(k.values()) if dataclasses.is_dataclass(v) and type(v).__name__ in CONFIGS)
                size = (17, 64, 96) if name == "RetakePipeline" else (conf.num_frames, conf.height, conf.width)
                frames = torch.zeros(*size, 3, dtype=torch.uint8)
                audio = getattr(conf, "audio_enabled", False) or name == "OneStagePipeline"
                return (frames, torch.zeros(1, 8, 3, 16)) if audio else frames
        return Pipe

    for name in PIPELINES:
        mp.setattr(P, name, pipeline(name))
    return gen


def _observe(tmp, route, conflict=None):
    """One generate_video call on the stubs -> what it did, as JSON."""
    paths = _files(tmp)

    def mask(s):
        return re.sub(r"\d+\.\d+ s\b", "<t> s", s.replace(tmp, "<tmp>"))

    def fill(v):
        if isinstance(v, list):
            return [fill(x) for x in v]
        if isinstance(v, str):
            for k, p in paths.items():
                v = v.replace(k, p)
        return v

    kw = dict(use_gemma=False, device="cpu", save_mp4=False, output_path=os.path.join(tmp, "out", "o.mp4"), seed=7)
    kw.update({k: fill(v) for k, v in dict(ROUTES[route], **(conflict or {})).items()})
    log, configs, seen = [], [], {}
    before = set(os.listdir(tmp))
    with pytest.MonkeyPatch.context() as mp:
        gen = _stub_everything(mp, log, configs, mask)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            try:
                result = gen.generate_video("a prompt", **kw)
                seen["returned"] = _plain(result, mask)
            except Exception as e:
                seen["raised"] = [type(e).__name__, mask(str(e))]
    written = sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs if d != tmp or f not in before)
    seen.update(calls=log, configs=configs, stdout=mask(out.getvalue()).splitlines(), files=written)
    return json.loads(json.dumps(seen))


def _conflict_id(case):
    return case[0] + "-" + "-".join(case[1])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_calls_configs_and_prints(route, golden, tmp_path):
    got, want = _observe(str(tmp_path), route), golden["routes"][route]
    assert "returned" in got, got.get("raised")
    for key in ("calls", "configs", "stdout", "files", "returned"):
        assert got[key] == want[key], key


@pytest.mark.parametrize("case", CONFLICTS, ids=_conflict_id)
def test_conflicting_arguments_first_error(case, golden, tmp_path):
    got, want = _observe(str(tmp_path), *case), golden["conflicts"][_conflict_id(case)]
    assert got == want


def test_the_recording_covers_every_route_once():
    """The seven routes each ran their own pipeline class (the standard route: none), so a recording of a wrong route cannot pass as golden."""
    with open(GOLDEN) as f:
        routes = json.load(f)["routes"]
    ran = {r: [c[0] for c in v["calls"] if isinstance(c, list) and c[0] in PIPELINES] for r, v in routes.items()}
    assert ran == {"keyframe": ["KeyframeInterpolationPipeline"], "hq": ["TI2VidHQPipeline"], "ic_lora": ["ICLoraPipeline"], "retake": ["RetakePipeline"],
                   "two_stage": ["DistilledPipeline"], "av": ["OneStagePipeline"], "standard": [], "standard_placeholder": []}


if __name__ == "__main__":
    import tempfile
    recorded = {"routes": {}, "conflicts": {}}
    assert len({_conflict_id(c) for c in CONFLICTS}) == len(CONFLICTS)
    for r in ROUTES:
        with tempfile.TemporaryDirectory() as d:
            recorded["routes"][r] = _observe(d, r)
    for c in CONFLICTS:
        with tempfile.TemporaryDirectory() as d:
            recorded["conflicts"][_conflict_id(c)] = _observe(d, *c)
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(ROUTES)} routes and {len(CONFLICTS)} conflicts to {GOLDEN}")
