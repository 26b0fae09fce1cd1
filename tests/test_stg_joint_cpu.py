"""STG with sound, the parts that need no GPU: generate_video's routing of stg_audio_scale on stubs (every refusal before a model loads), the
ABI entries, OneStagePipeline's own validation, and tests/stg_joint_ref's float64 restatement of the pair arithmetic against the package's
guiders, post_process_latent and EulerDiffusionStep composed in torch fp32."""
import contextlib
import inspect
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

import stg_joint_ref as JR  # noqa: E402

NEW_ENTRIES = {"ltx2_stg_euler_step_pair": 29, "ltx2_dit_stg_step_joint_av": 24}


# ------------------------------------------------------------------ generate_video(stg_audio_scale=...)
def _route(tmp, route, **extra):
    """One generate_video call on test_generate_routes_cpu's stubs with OneStagePipeline replaced by a recorder -> (what its __call__ was given,
    or the exception under "raised"; the printed lines).  Nothing is loaded: a refusal seen here stands before any model."""
    import test_generate_routes_cpu as G
    import ltx_2_mlx_amd.pipelines as P
    paths = G._files(tmp)

    def fill(v):
        if isinstance(v, list):
            return [fill(x) for x in v]
        return next((v.replace(k, p) for k, p in paths.items() if k in v), v) if isinstance(v, str) else v

    kw = dict(use_gemma=False, device="cpu", save_mp4=False, output_path=os.path.join(tmp, "out", "o.mp4"), seed=7)
    kw.update({k: fill(v) for k, v in dict(G.ROUTES[route], **extra).items()})
    seen = {}

    class Recorder:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            seen.update(pipeline="OneStagePipeline", kwargs=k)
            conf = k["config"]
            return torch.zeros(conf.num_frames, conf.height, conf.width, 3, dtype=torch.uint8), torch.zeros(1, 8, 3, 16)

    out = io.StringIO()
    with pytest.MonkeyPatch.context() as mp:
        gen = G._stub_everything(mp, [], [], lambda s: s)
        mp.setattr(P, "OneStagePipeline", Recorder)
        with contextlib.redirect_stdout(out):
            try:
                gen.generate_video("a prompt", **kw)
            except Exception as e:  # noqa: BLE001
                seen["raised"] = e
    return seen, out.getvalue().splitlines()


def test_stg_audio_scale_is_refused_off_the_av_route(tmp_path):
    seen, _ = _route(str(tmp_path), "standard", stg_audio_scale=1.0)
    assert isinstance(seen.get("raised"), NotImplementedError), seen
    assert str(seen["raised"]) == "stg_audio_scale=1.0 is outside the MI355X hot path (see DESIGN.md); leave it at its default 0.0"
    seen, _ = _route(str(tmp_path), "two_stage", stg_audio_scale=1.0)
    assert isinstance(seen.get("raised"), NotImplementedError) and "stg_audio_scale=1.0" in str(seen["raised"])


def test_stg_audio_scale_reaches_one_stage_pipeline(tmp_path):
    import generate as gen
    tmp = str(tmp_path)
    assert "stg_audio_scale" in gen._ROUTE_OWNS["av"] and all("stg_audio_scale" not in v for k, v in gen._ROUTE_OWNS.items() if k != "av")
    assert gen._OUT_OF_PATH_DEFAULTS["stg_audio_scale"] == 0.0
    seen, lines = _route(tmp, "av", stg_scale=1.5, stg_audio_scale=0.75, stg_blocks=[1], stg_cutoff=0.5, model_variant="distilled")
    assert "raised" not in seen, seen
    k = seen["kwargs"]
    assert seen["pipeline"] == "OneStagePipeline" and (k["stg_scale"], k["stg_audio_scale"], k["stg_blocks"], k["stg_cutoff"]) == (1.5, 0.75, [1], 0.5)
    assert "Audio STG guidance: scale=0.75 (the audio self-attention of the STG blocks is skipped too)" in lines
    # the audio alone: no stg_scale keyword, the block set and the cutoff travel with the audio scale
    seen, lines = _route(tmp, "av", stg_audio_scale=1.0, stg_blocks=[0], model_variant="distilled")
    k = seen["kwargs"]
    assert "raised" not in seen and "stg_scale" not in k and (k["stg_audio_scale"], k["stg_blocks"], k["stg_cutoff"]) == (1.0, [0], 1.0)
    assert not [l for l in lines if l.startswith("STG guidance")]
    # without the flag: no keyword, no line
    seen, lines = _route(tmp, "av", stg_scale=1.0, model_variant="distilled")
    assert "stg_audio_scale" not in seen["kwargs"] and not [l for l in lines if "Audio STG" in l]
    # Heun and GE beside it stay refused; stg_mode is as it was; the shared checks hold for the audio scale alone
    seen, _ = _route(tmp, "av", stg_audio_scale=1.0, sampler="heun", model_variant="distilled")
    assert isinstance(seen.get("raised"), NotImplementedError) and "sampler='heun' beside stg_audio_scale=1.0" in str(seen["raised"])
    seen, _ = _route(tmp, "av", stg_scale=1.0, stg_audio_scale=1.0, sampler="heun", model_variant="distilled")
    assert isinstance(seen.get("raised"), NotImplementedError) and "sampler='heun'" in str(seen["raised"])
    seen, _ = _route(tmp, "av", stg_audio_scale=1.0, ge_gamma=0.5, model_variant="distilled")
    assert isinstance(seen.get("raised"), NotImplementedError) and "ge_gamma=0.5" in str(seen["raised"])
    seen, _ = _route(tmp, "av", stg_scale=1.0, stg_audio_scale=1.0, stg_mode="both", model_variant="distilled")
    assert isinstance(seen.get("raised"), NotImplementedError) and "stg_mode='both'" in str(seen["raised"])
    seen, _ = _route(tmp, "av", stg_audio_scale=1.0, stg_blocks=[48], model_variant="distilled")
    assert isinstance(seen.get("raised"), ValueError) and "stg_blocks [48] out of range" in str(seen["raised"])
    seen, _ = _route(tmp, "av", stg_audio_scale=-1.0, model_variant="distilled")
    assert isinstance(seen.get("raised"), ValueError) and "stg_audio_scale" in str(seen["raised"])
    # CFG* (the dev variant's default rescale) and APG keep the eager loop, which STG-guides the video alone
    seen, _ = _route(tmp, "av", stg_audio_scale=1.0, rescale_scale=0.7, cfg_scale=3.0, model_variant="dev")
    assert isinstance(seen.get("raised"), NotImplementedError) and "stg_audio_scale=1.0 runs under plain CFG" in str(seen["raised"])


def test_cli_passes_stg_audio_scale():
    import generate as gen
    k = gen.kwargs_from_args(gen.build_parser().parse_args(["p", "--generate-audio", "--stg-audio-scale", "0.5"]))
    assert k["stg_audio_scale"] == 0.5 and k["stg_mode"] == "video"
    assert gen.kwargs_from_args(gen.build_parser().parse_args(["p"]))["stg_audio_scale"] == 0.0
    p = inspect.signature(gen.generate_video).parameters["stg_audio_scale"]
    assert p.kind == inspect.Parameter.KEYWORD_ONLY and p.default == 0.0
    assert "--stg-audio-scale" in open(os.path.join(ROOT, "README.md")).read()


# ------------------------------------------------------------------ the ABI and the exports
def test_abi_declares_the_joint_stg_entries():
    from ltx_2_mlx_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    assert re.search(r"#define LTX2_ABI_VERSION 3\b", header) and nv.ABI_VERSION == 3          # additive entries: no bump
    for name, n_args in NEW_ENTRIES.items():
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S)
        assert decl, name
        assert name in nv.SIGNATURES and nv.SIGNATURES[name][0] is nv.i32, name
        assert len(decl.group(1).split(",")) == len(nv.SIGNATURES[name][1]) == n_args, name
    # header, binding and library name the same entries
    declared = set(re.findall(r"^[A-Za-z_][\w \*]*?\b(ltx2_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.M))
    assert declared == set(nv.SIGNATURES), (sorted(declared - set(nv.SIGNATURES)), sorted(set(nv.SIGNATURES) - declared))
    if os.path.exists(nv.LIB_PATH):
        import shutil
        import subprocess
        assert all(hasattr(nv.lib(), n) for n in NEW_ENTRIES)
        if shutil.which("nm"):
            out = subprocess.run(["nm", "-D", "--defined-only", nv.LIB_PATH], capture_output=True, text=True, check=True).stdout
            exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("ltx2_") and " T " in ln}
            assert exported == declared, (sorted(exported - declared), sorted(declared - exported))


def test_exports():
    import ltx_2_mlx_amd.pipelines as P
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import LTXModel
    assert "joint_stg_denoise_loop" in P.__all__ and callable(P.joint_stg_denoise_loop)
    assert callable(K.stg_euler_step_pair) and callable(LTXModel.stg_step_joint_av_)
    sig = inspect.signature(P.OneStagePipeline.__call__).parameters["stg_audio_scale"]
    assert sig.kind == inspect.Parameter.KEYWORD_ONLY and sig.default == 0.0
    assert inspect.signature(P.joint_stg_denoise_loop).parameters["fused"].default is True


def test_joint_stg_perturbations():
    from ltx_2_mlx_amd.components import PerturbationType as PT
    from ltx_2_mlx_amd.pipelines.common import joint_stg_perturbations
    both, audio, video = joint_stg_perturbations([1], True, True), joint_stg_perturbations(None, False, True), joint_stg_perturbations([2], True, False)
    assert both.all_in_batch(PT.SKIP_VIDEO_SELF_ATTN, 1) and both.all_in_batch(PT.SKIP_AUDIO_SELF_ATTN, 1) and not both.any_in_batch(PT.SKIP_AUDIO_SELF_ATTN, 0)
    assert audio.all_in_batch(PT.SKIP_AUDIO_SELF_ATTN, 47) and not audio.any_in_batch(PT.SKIP_VIDEO_SELF_ATTN, 0)
    assert video.all_in_batch(PT.SKIP_VIDEO_SELF_ATTN, 2) and not video.any_in_batch(PT.SKIP_AUDIO_SELF_ATTN, 2)


# ------------------------------------------------------------------ OneStagePipeline's own validation
def test_one_stage_validates_stg_audio_scale_itself():
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline

    class Stub:
        num_layers = 4
        device = torch.device("cpu")
    pipe = OneStagePipeline.__new__(OneStagePipeline)
    pipe.transformer, pipe.is_av_model = type("X", (), {"velocity_model": Stub()})(), False
    conf = OneStageCFGConfig(height=64, width=96, num_frames=9)
    enc = torch.zeros(1, 4, 8)
    with pytest.raises(ValueError, match="stg_audio_scale > 0 needs an audio state"):
        pipe(enc, enc, conf, stg_audio_scale=1.0)
    pipe.is_av_model = True                                               # the audio branch is active: the checks STG shares
    kw = dict(positive_audio_encoding=enc, negative_audio_encoding=enc)
    with pytest.raises(ValueError, match=r"stg_blocks \[4\] out of range"):
        pipe(enc, enc, conf, stg_audio_scale=1.0, stg_blocks=[4], **kw)
    with pytest.raises(ValueError, match="stg_cutoff"):
        pipe(enc, enc, conf, stg_audio_scale=1.0, stg_cutoff=1.5, **kw)
    with pytest.raises(NotImplementedError, match="sampler='heun'"):
        pipe(enc, enc, conf, stg_audio_scale=1.0, sampler="heun", **kw)
    with pytest.raises(NotImplementedError, match="GE velocity"):
        pipe(enc, enc, conf, stg_audio_scale=1.0, ge_gamma=0.5, **kw)


# ------------------------------------------------------------------ the restatement of the pair arithmetic
def _torch_segment(mp, x, vc, vu, vp, ts, mask, clean, cfg, stg, sigma, sigma_next):
    """The package's own parts in torch fp32 on the CPU: x0 = x - t * v per velocity, CFGGuider, STGGuider, post_process_latent and
    EulerDiffusionStep.  EulerDiffusionStep hands its arithmetic to the ltx2_euler_step kernel, which needs a GPU; here that one call is
    replaced by the statement include/ltx2hip.h documents for the individually rounded steps, x + ((x - d) * (1/sigma)) * (sigma_next -
    sigma) with fp32 scalars, so the class itself (its reshapes and casts) still runs."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep, STGGuider
    from ltx_2_mlx_amd.pipelines.common import post_process_latent
    f = np.float32
    mp.setattr(K, "euler_step", lambda s, d, sg, sn, mask=None, clean=None: s + ((s - d) * torch.tensor(f(1.0) / f(sg))) * torch.tensor(f(sn) - f(sg)))
    t = ts.reshape(-1, 1)
    g = x - t * vc
    if vu is not None:
        g = CFGGuider(cfg).guide(g, x - t * vu)
    if vp is not None:
        g = STGGuider(stg).guide(g, x - t * vp)
    if mask is not None:
        g = post_process_latent(g[None], mask.reshape(1, -1, 1), clean[None])[0]
    return EulerDiffusionStep().step(x[None], g[None], [sigma, sigma_next], 0)[0]


@pytest.mark.parametrize("rows,C", [(37, 128), (5, 6)])
def test_pair_restatement_is_the_torch_composition_bit_for_bit(rows, C, monkeypatch):
    """Scales whose (cfg - 1) is exact in fp32 (3, 7; stg 1, 1.5), as CFGGuider forms cfg - 1 in double and the kernel in fp32."""
    d = JR.inputs(rows, C, seed=rows * 7 + C)
    sigma, sigma_next = 0.909375, 0.725
    n = 0
    for ts in (torch.tensor([sigma]), d["ts_row"]):
        for masked in (False, True):
            for vu in (None, d["vu"]):
                for vp in (None, d["vp"]):
                    for cfg, stg in ((3.0, 1.0), (7.0, 1.5)):
                        mk, cl = (d["mask"], d["clean"]) if masked else (None, None)
                        want = _torch_segment(monkeypatch, d["x"], d["vc"], vu, vp, ts, mk, cl, cfg, stg, sigma, sigma_next)
                        got = torch.from_numpy(JR.pair_segment(d["x"], d["vc"], vu, vp, ts, mk, cl, cfg, stg, sigma, sigma_next))
                        assert got.dtype == torch.float32 and torch.equal(got, want), (ts.numel(), masked, vu is not None, vp is not None, cfg)
                        n += 1
    assert n == 32
    # the restatement sees each term: STG, CFG and the mask all move the result
    base = JR.pair_segment(d["x"], d["vc"], d["vu"], d["vp"], d["ts_row"], d["mask"], d["clean"], 3.0, 1.0, sigma, sigma_next)
    assert not np.array_equal(base, JR.pair_segment(d["x"], d["vc"], d["vu"], None, d["ts_row"], d["mask"], d["clean"], 3.0, 1.0, sigma, sigma_next))
    assert not np.array_equal(base, JR.pair_segment(d["x"], d["vc"], None, d["vp"], d["ts_row"], d["mask"], d["clean"], 3.0, 1.0, sigma, sigma_next))
    assert not np.array_equal(base, JR.pair_segment(d["x"], d["vc"], d["vu"], d["vp"], d["ts_row"], None, None, 3.0, 1.0, sigma, sigma_next))
    # stg 0 with a perturbed velocity == no perturbed velocity (g + 0 * (g - p) = g), and both segments of pair() are pair_segment's
    zero = JR.pair_segment(d["x"], d["vc"], d["vu"], d["vp"], d["ts_row"], d["mask"], d["clean"], 3.0, 0.0, sigma, sigma_next)
    assert np.array_equal(zero, JR.pair_segment(d["x"], d["vc"], d["vu"], None, d["ts_row"], d["mask"], d["clean"], 3.0, 0.0, sigma, sigma_next))
    seg = dict(x=d["x"], vel_cond=d["vc"], vel_uncond=d["vu"], vel_perturbed=d["vp"], timesteps=d["ts_row"], mask=d["mask"], clean=d["clean"], cfg_scale=3.0,
               stg_scale=1.0)
    v, a = JR.pair(seg, dict(seg, vel_perturbed=None), sigma, sigma_next)
    assert np.array_equal(v, base) and not np.array_equal(a, base)
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        JR.pair_segment(d["x"], d["vc"], None, None, d["ts_row"], None, None, 3.0, 1.0, 0.0, 0.5)


def test_joint_loop_restatement_reduces_to_stg_loop_av():
    """stg_joint_loop with no audio STG term is tests/stg_ref.stg_loop_av, and its audio term acts on the audio alone (toy x0 functions)."""
    import stg_ref as R
    g = torch.Generator().manual_seed(3)
    v, a = torch.randn(1, 12, 8, generator=g), torch.randn(1, 9, 8, generator=g)
    pos = lambda v_, a_, s: (0.5 * v_ + s, 0.25 * a_ - s)           # noqa: E731
    neg = lambda v_, a_, s: (0.4 * v_, 0.3 * a_)                    # noqa: E731
    pert = lambda v_, a_, s: (0.45 * v_ + s, 0.2 * a_)              # noqa: E731
    gv, ga = (lambda p, n: p + 2.0 * (p - n)), (lambda p, n: p + 6.0 * (p - n))
    sig = [1.0, 0.75, 0.5, 0.25, 0.0]
    want = R.stg_loop_av(v, a, pos, neg, pert, sig, gv, ga, 1.5, 0.5)
    got = JR.stg_joint_loop(v, a, pos, neg, pert, sig, gv, ga, 1.5, 0.0, 0.5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    both = JR.stg_joint_loop(v, a, pos, neg, pert, sig, gv, ga, 1.5, 1.0, 0.5)
    assert torch.equal(both[0], want[0]) and not torch.equal(both[1], want[1])          # these toy modalities do not see each other
    none = JR.stg_joint_loop(v, a, pos, neg, pert, sig, gv, ga, 0.0, 0.0, 1.0)
    assert torch.equal(none[0], R.stg_loop_av(v, a, pos, neg, pert, sig, gv, ga, 0.0, 1.0)[0])
