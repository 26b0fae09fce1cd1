"""Restatement (torch, CPU) of the joint audio+video guided step with a guider per modality: the kernel inputs of
tests/test_joint_projected_gpu.py, the torch guiders on them, and the reference's joint loop (pipelines/one_stage.py:466-568) in fp32 with
the torch guiders.  Checker side only: nothing here is imported by the package."""
import torch

import projected_guidance_ref as R
from oracle import loop

SEGMENT_MODES = ("off", "cfg", "cfg_star", "apg", "apg_momentum")
SHAPES = [(1, 1, 128), (37, 5, 128), (96, 9, 128), (37, 5, 12)]          # (video rows, audio rows, C)


def inputs(rows, C, seed=0):
    """One segment's kernel inputs, as tests/test_projected_guidance_gpu.py::_inputs draws them: x, vel_cond standard normal,
    vel_uncond = 0.7*vel_cond + 0.5*noise (never all zero: CFG*'s projection divides by |uncond|^2 + 1e-8), t in [0.2, 1], a mask of 0 / 0.05 / 1,
    and a previous running guidance for the continuing steps."""
    g = torch.Generator().manual_seed(rows * 131 + C + seed)
    x, vc, noise, clean = (torch.randn(rows, C, generator=g) for _ in range(4))
    vu = 0.7 * vc + 0.5 * noise
    ts_row = 0.2 + 0.8 * torch.rand(rows, generator=g)
    mask = torch.ones(rows)
    mask[::3] = 0.0
    mask[1::3] = 0.05
    running = torch.randn(rows, C, generator=g)
    return dict(x=x, vc=vc, vu=vu, clean=clean, ts_row=ts_row, mask=mask, running=running)


def segment_guider(mode, x0_norm=None):
    """(kernel arguments, the torch guider) of one segment mode.  The APG threshold is half of the input's own |cond - uncond| when it is given
    (so that it binds), else 5."""
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider, LegacyStatefulAPGGuider, LtxAPGGuider
    thr = 5.0 if x0_norm is None else 0.5 * x0_norm
    if mode == "off":
        return dict(mode=4, scale=1.0), None
    if mode == "cfg":
        return dict(mode=3, scale=2.5), CFGGuider(2.5)
    if mode == "cfg_star":
        return dict(mode=0, scale=3.0, eta=1.0, norm_threshold=0.0, momentum=0.0), CFGStarRescalingGuider(3.0)
    if mode == "apg":
        return dict(mode=1, scale=3.0, eta=0.5, norm_threshold=thr, momentum=0.0), LtxAPGGuider(3.0, 0.5, thr)
    if mode == "apg_momentum":
        return dict(mode=2, scale=2.5, eta=0.5, norm_threshold=thr, momentum=0.5), LegacyStatefulAPGGuider(2.5, 0.5, thr, 0.5)      # (scale 2 would be APG at scale 3 on a first step)
    raise ValueError(mode)


def guided_x0(t, mode, per_row=True):
    """The torch guider of `mode` on one segment's inputs -> the guided x0 (the conditional x0 for "off")."""
    ts = t["ts_row"] if per_row else torch.tensor([0.909375])
    a, b = R.x0_pair(t["x"], t["vc"], t["vu"], ts)
    guider = segment_guider(mode, float((a - b).double().norm()))[1]
    return a if guider is None else guider.guide(a[None], b[None])[0]


def guided_loop_av(video, audio, x0_pos, x0_neg, sigmas, video_guider, audio_guider):
    """The reference's joint guided loop in fp32: video / audio = (tokens, mask, clean); x0_pos / x0_neg(v, v_ts, a, a_ts, sigma) -> (video x0,
    audio x0); each modality's torch guider on its pair of predictions over ALL its tokens (None: the conditional prediction),
    post_process_latent, Euler.  -> (video tokens, audio tokens)."""
    for g in (video_guider, audio_guider):
        if hasattr(g, "reset"):
            g.reset()
    (v, vmask, vclean), (a, amask, aclean) = video, audio
    v, a = v.float(), a.float()
    for i in range(len(sigmas) - 1):
        s, sn = float(sigmas[i]), float(sigmas[i + 1])
        vts, ats = loop.timesteps_from_mask(vmask, s), loop.timesteps_from_mask(amask, s)
        pv, pa = x0_pos(v, vts, a, ats, s)
        nv, na = x0_neg(v, vts, a, ats, s)
        gv = pv if video_guider is None else video_guider.guide(pv, nv)
        ga = pa if audio_guider is None else audio_guider.guide(pa, na)
        v = loop.euler_step(v, loop.post_process_latent(gv, vmask, vclean), s, sn)
        a = loop.euler_step(a, loop.post_process_latent(ga, amask, aclean), s, sn)
    return v, a
