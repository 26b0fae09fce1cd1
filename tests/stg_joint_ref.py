"""Restatements for the joint audio+video STG step.  Checker side only: nothing here is imported by the package.

pair_segment / pair: ltx2_stg_euler_step_pair's arithmetic of one segment in numpy.  Every operation is carried out in float64 on fp32 values
and rounded to fp32 at once.  For +, - and * that is the fp32 operation itself: a product of two fp32 numbers is exact in float64, and a sum
rounded to 53 bits and then to 24 equals the sum rounded to 24 (53 >= 2 * 24 + 2).  So the result is what individually rounded fp32 ops
give, bit for bit, without relying on how a library contracts them.  The scalars are formed in fp32 as the host code forms them.

stg_joint_loop: tests/stg_ref.stg_loop_av with an STG term on the audio prediction too, from the oracle's own pieces."""
import numpy as np
import torch

from oracle import loop

from stg_ref import stg_active

F32, F64 = np.float32, np.float64


def _op(v):
    """One fp32 rounding of a float64 result, carried on in float64."""
    return np.asarray(v, F64).astype(F32).astype(F64)


def _a(t):
    return None if t is None else np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, F32).astype(F64)


def pair_segment(x, vel_cond, vel_uncond, vel_perturbed, timesteps, mask, clean, cfg_scale, stg_scale, sigma, sigma_next):
    """One segment of ltx2_stg_euler_step_pair -> np.float32 (rows, C).  vel_uncond None: no CFG; vel_perturbed None: no STG term (the
    guided step's arithmetic); timesteps: 1 or rows elements; mask (rows,) with clean (rows, C), or both None."""
    if sigma == 0:
        raise ValueError("Sigma can't be 0.0")
    s1, stg = F64(F32(cfg_scale) - F32(1.0)), F64(F32(stg_scale))
    inv, dt = F64(F32(1.0) / F32(sigma)), F64(F32(sigma_next) - F32(sigma))
    x, vc, vu, vp, cl = _a(x), _a(vel_cond), _a(vel_uncond), _a(vel_perturbed), _a(clean)
    t = _a(timesteps).reshape(-1, 1)
    g = _op(x - _op(t * vc))
    if vu is not None:
        b = _op(x - _op(t * vu))
        g = _op(g + _op(s1 * _op(g - b)))
    if vp is not None:
        p = _op(x - _op(t * vp))
        g = _op(g + _op(stg * _op(g - p)))
    if mask is not None:
        m = _a(mask).reshape(-1, 1)
        g = _op(_op(g * m) + _op(cl * _op(1.0 - m)))
    return _op(x + _op(_op(_op(x - g) * inv) * dt)).astype(F32)


def pair(video: dict, audio: dict, sigma, sigma_next):
    """Both segments, each a dict of pair_segment's arguments by name (as kernels.stg_euler_step_pair takes them)."""
    seg = lambda s: pair_segment(s["x"], s["vel_cond"], s.get("vel_uncond"), s.get("vel_perturbed"), s["timesteps"], s.get("mask"), s.get("clean"),      # noqa: E731
                                 s["cfg_scale"], s["stg_scale"], sigma, sigma_next)
    return seg(video), seg(audio)


def inputs(rows, C, seed):
    """fp32 operands of one segment: x, vc, vu, vp, clean (rows, C), per-row timesteps, and a mask with zeros, small values and ones."""
    g = torch.Generator().manual_seed(seed)
    d = {k: torch.randn(rows, C, generator=g) for k in ("x", "vc", "vu", "vp", "clean")}
    d["ts_row"] = torch.rand(rows, generator=g)
    d["mask"] = torch.ones(rows)
    d["mask"][::3] = 0.0
    d["mask"][1::3] = 0.05
    return d


def stg_joint_loop(vtok, atok, x0_pos, x0_neg, x0_pert, sigmas, guide_v, guide_a, stg_v, stg_a, cutoff):
    """The joint loop of pipelines/one_stage.py:495-563 in fp32 without conditioning tokens, an STG term per modality.  x0_*(video tokens,
    audio tokens, sigma) -> (video x0, audio x0); x0_neg None: no guider is enabled; x0_pert: the pass on the weights whose skipped
    self-attentions' out-projections are zero (video for stg_v != 0, audio for stg_a != 0)."""
    v, a = vtok.float(), atok.float()
    n = len(sigmas) - 1
    for i in range(n):
        s = float(sigmas[i])
        dv, da = x0_pos(v, a, s)
        if x0_neg is not None:
            nv, na = x0_neg(v, a, s)
            dv, da = guide_v(dv, nv), guide_a(da, na)
        if stg_active(i, n, 1.0, cutoff) and (stg_v != 0.0 or stg_a != 0.0):
            pv, pa = x0_pert(v, a, s)
            if stg_v != 0.0:
                dv = dv + stg_v * (dv - pv)
            if stg_a != 0.0:
                da = da + stg_a * (da - pa)
        v, a = loop.euler_step(v, dv, s, float(sigmas[i + 1])), loop.euler_step(a, da, s, float(sigmas[i + 1]))
    return v, a
