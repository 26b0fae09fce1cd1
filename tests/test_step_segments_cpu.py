"""Where the library is built: every `ltx2_*_pair` sampler-step entry and its single twin refuse sigma == 0, a mask without its clean latent
and a bad ts_stride with E_INVALID and a fixed text -- what a later change of the launchers behind them has to keep.  The ctypes calls pass
dummy addresses and ONLY arguments that a check in front of the launch turns down, so nothing is ever launched and no GPU is needed."""
import os
import re

import pytest

from ltx_2_mlx_amd import _native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _code(text):
    """C++ without its comments."""
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


# ---- refusals through the C ABI: the texts below were recorded from the library as it is built today ----
PAIRS = ("ltx2_guided_euler_step_pair", "ltx2_ancestral_euler_step_pair", "ltx2_stg_euler_step_pair", "ltx2_res2s_midpoint_pair",
         "ltx2_res2s_combine_pair", "ltx2_heun_predict_pair", "ltx2_heun_correct_pair", "ltx2_ge_euler_step_pair", "ltx2_guidance_sums_pair",
         "ltx2_projected_euler_step_pair", "ltx2_mm_guided_euler_step_pair")
ENTRIES = PAIRS + tuple(e[:-len("_pair")] for e in PAIRS)

ADDR = 0x7F0000001000           # a 16-byte aligned address that is never read: every call below is refused in front of the launch


def _parameters(entry):
    """[(name, is a pointer)] of an exported entry, from the header."""
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    m = re.search(r"\b%s\(([^)]*)\)" % entry, _code(header))
    assert m, entry
    return [(re.search(r"(\w+)$", p.strip()).group(1), "*" in p) for p in m.group(1).split(",")]


def _arguments(entry, **override):
    """Arguments that pass every check of `entry` -- so that `override` alone is what it refuses.  NEVER call an entry with these as they
    are: each case below overrides one of them with a value the entry turns down before it launches."""
    assert override
    args = []
    for name, pointer in _parameters(entry):
        base = re.sub(r"^[va]_", "", name)
        if name in override:
            args.append(override[name])
        elif name == "stream":
            args.append(None)
        elif base == "running" and "projected" in entry:
            args.append(None)               # read under mode 2 alone
        elif pointer:
            args.append(ADDR)
        elif base in ("ts_stride", "first"):
            args.append(1)
        elif base in ("rows", "C"):
            args.append(8)
        elif base in ("mode", "n_bong", "step"):
            args.append(0)
        else:
            args.append(1.0)                # sigmas, scales, gammas, c, h, b1, b2, eta, norm_threshold, momentum
    return args


def _cases():
    for entry in ENTRIES:
        names = [n for n, _ in _parameters(entry)]
        segs = ("v_", "a_") if entry.endswith("_pair") else ("",)
        if "sigma" in names:
            yield entry, {"sigma": 0.0}
        for s in segs:
            yield entry, {s + "ts_stride": 2}
            if s + "mask" in names:
                yield entry, {s + "clean": None}


WHO = {e: e[len("ltx2_"):] for e in ENTRIES}
WHO.update(ltx2_ge_euler_step="heun_predict", ltx2_ge_euler_step_pair="heun_predict_pair")      # the GE step is the predictor's pass
SIGMA = {e: "Sigma can't be 0.0" for e in ENTRIES}
for _e in ("ltx2_heun_predict", "ltx2_ge_euler_step"):
    SIGMA[_e] = "heun_predict: sigma=0 must be > 0"
    SIGMA[_e + "_pair"] = "heun_predict_pair: sigma=0 must be > 0"
SIGMA["ltx2_heun_correct"] = "heun_correct: sigma=0 and sigma_next=1 must be > 0 (sigma_next == 0: the step ends with d)"
SIGMA["ltx2_heun_correct_pair"] = "heun_correct_pair: sigma=0 and sigma_next=1 must be > 0 (sigma_next == 0: the step ends with d)"


def _expected(entry, override):
    (name, _), = override.items()
    if name == "sigma":
        return SIGMA[entry]
    if name.endswith("ts_stride"):
        return WHO[entry] + ": ts_stride is 0 (one timestep) or 1 (one per row)"
    return WHO[entry] + ": mask and clean go together"


@pytest.mark.parametrize("entry,override", list(_cases()), ids=lambda v: v if isinstance(v, str) else "-".join("%s=%s" % kv for kv in v.items()))
def test_refusals_keep_their_code_and_their_words(entry, override):
    if not (os.path.exists(nv.LIB_PATH) and os.path.exists(nv.LIB_PATH_F16)):
        pytest.skip("the library is not built")
    import torch
    for build in (None, torch.float16):
        lib = nv.lib(build)
        lib.ltx2_clear_error()
        assert getattr(lib, entry)(*_arguments(entry, **override)) == nv.E_INVALID
        assert lib.ltx2_last_error().decode() == _expected(entry, override)
        lib.ltx2_clear_error()
