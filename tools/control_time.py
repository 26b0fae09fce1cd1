"""The control-video path of the IC-LoRA pipeline at 97x256x384 and 97x512x768 (stage-1 sizes of 512x768 and 1024x1536 requests):
  canny             whole (ltx2_canny_u8) and its hysteresis share (ltx2_canny_hysteresis on the same map), with the pass counts;
  frames_to_patches against the torch glue it replaces (patchify_video on the fp32 clip, the host-to-device copy of that clip left out)
                    and against a device copy of the same output bytes.
The clip is noise blurred to about 4 px at 80 grey levels per standard deviation (long connected edges).  Warm-up, device events, the median of repeated runs.

    python tools/control_time.py [--reps 20] [out.md]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import _native as nv  # noqa: E402
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.model.video_vae_encoder import patchify_video  # noqa: E402


def timed(fn, reps, warm=3):
    """median microseconds of `reps` single runs between device events, after `warm` runs"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def clip(f, h, w, dev):
    from scipy import ndimage
    rng = np.random.default_rng(1)
    b = ndimage.gaussian_filter(rng.random((f, h, w, 3), dtype=np.float32), sigma=(0, 4, 4, 0), mode="nearest")
    return torch.from_numpy(np.clip(np.round((b - b.mean()) / b.std() * 80 + 128), 0, 255).astype(np.uint8)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# IC-LoRA: the control-video path (`tools/control_time.py`)", "",
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; median of {a.reps} runs after 3 warm-up runs, device events.  The clip is",
             "noise blurred to about 4 px.  The canny figures include one host synchronisation per hysteresis pass (the flag read that decides",
             "whether another pass is launched): that is the call's real cost.", ""]
    for f, h, w in ((97, 256, 384), (97, 512, 768)):
        x = clip(f, h, w, dev)
        edges = torch.empty(f, h, w, dtype=torch.uint8, device=dev)
        ws = torch.empty(nv.CANNY_FLAG_BYTES + f * h * w, dtype=torch.uint8, device=dev)
        cmap = ws[nv.CANNY_FLAG_BYTES:].view(f, h, w)                        # the map ltx2_canny_u8 leaves in its workspace
        n_pass = nv.i32(0)

        def run_canny():
            nv.check(nv.lib().ltx2_canny_u8(nv.ptr(x), f, h, w, 100.0, 200.0, nv.ptr(edges), nv.ptr(ws), ws.numel(), nv.C.byref(n_pass), nv.stream()))

        t_canny = timed(run_canny, a.reps)
        cmap = cmap.clone()
        t_hyst = timed(lambda: K.canny_hysteresis(cmap, out=edges), a.reps)
        frac = float((edges != 0).float().mean())
        v = (x.permute(3, 0, 1, 2).float() / 127.5 - 1.0).contiguous()        # the fp32 clip the glue starts from, already on the device
        out = torch.empty(f, h // 4, w // 4, 64, dtype=torch.bfloat16, device=dev)
        t_new = timed(lambda: K.frames_to_patches(x, out=out), a.reps)
        t_glue = timed(lambda: patchify_video(v), a.reps)
        t_glue_u8 = timed(lambda: patchify_video(x.permute(3, 0, 1, 2).float() / 127.5 - 1.0), a.reps)
        src = torch.empty_like(out)
        t_copy = timed(lambda: out.copy_(src), a.reps)
        mb_out, mb_in = out.numel() * 2 / 1e6, x.numel() / 1e6
        lines += [f"### {f} x {h} x {w}", "",
                  f"canny (100, 200): {t_canny:.0f} us whole, {n_pass.value} hysteresis passes; the hysteresis alone {t_hyst:.0f} us "
                  f"({100 * t_hyst / t_canny:.0f} %); {100 * frac:.1f} % of the pixels are edges", "",
                  "| uint8 frames -> patchified bf16 operand | us |", "|---|---|",
                  f"| frames_to_patches ({mb_in:.1f} MB in, {mb_out:.1f} MB out) | {t_new:.0f} |",
                  f"| torch glue: patchify_video on the fp32 clip | {t_glue:.0f} |",
                  f"| torch glue from the uint8 frames (cast, divide, subtract, patchify_video) | {t_glue_u8:.0f} |",
                  f"| device copy of the {mb_out:.1f} MB of output | {t_copy:.0f} |", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
