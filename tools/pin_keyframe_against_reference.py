"""Generate tests/golden/keyframe_conditioning.npz by executing the REFERENCE'S OWN VideoConditionByKeyframeIndex.apply_to
(LTX_2_MLX/conditioning/keyframe.py, with its VideoLatentTools and patchifier) through the mlx->torch shim (tools/mlx_shim.py):

    python tools/pin_keyframe_against_reference.py REFERENCE_DIR      (the directory that holds LTX_2_MLX/)

State (1, 128, 3, 2, 3) at fps 24; two keyframes (1, 128, 1, 2, 3): frame_idx 0 at strength 1.0 (the causal first-frame shift applies)
and frame_idx 16 at strength 0.9 (it does not).  Stored: the seeded inputs and the four arrays of the resulting state (latent, clean
latent, denoise mask, positions).  Data only; no reference source travels.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "LTX_2_MLX")):
    sys.exit("usage: python tools/pin_keyframe_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
sys.path.insert(0, sys.argv[1])

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()

SHAPE = (1, 128, 3, 2, 3)
FPS = 24.0
KEYFRAMES = ((0, 1.0), (16, 0.9))
SEED = 20


def main():
    from LTX_2_MLX.components.patchifiers import VideoLatentPatchifier
    from LTX_2_MLX.conditioning.keyframe import VideoConditionByKeyframeIndex
    from LTX_2_MLX.conditioning.tools import VideoLatentTools
    from LTX_2_MLX.types import VideoLatentShape
    g = torch.Generator().manual_seed(SEED)
    initial = torch.randn(SHAPE, generator=g)
    kfs = [torch.randn(SHAPE[0], SHAPE[1], 1, SHAPE[3], SHAPE[4], generator=g) for _ in KEYFRAMES]
    tools = VideoLatentTools(patchifier=VideoLatentPatchifier(patch_size=1), target_shape=VideoLatentShape.from_shape(SHAPE), fps=FPS)
    state = tools.create_initial_state(dtype=mx.float32, initial_latent=shim.Arr(initial))
    for (idx, strength), kf in zip(KEYFRAMES, kfs):
        state = VideoConditionByKeyframeIndex(keyframes=shim.Arr(kf), frame_idx=idx, strength=strength).apply_to(state, tools)
    arr = lambda a: a.t.detach().float().numpy()
    out = os.path.join(ROOT, "tests", "golden", "keyframe_conditioning.npz")
    np.savez(out, initial=initial.numpy(), keyframes=torch.stack(kfs).numpy(), frame_idx=np.array([k[0] for k in KEYFRAMES], dtype=np.int64),
             strength=np.array([k[1] for k in KEYFRAMES], dtype=np.float64), fps=np.float64(FPS), latent=arr(state.latent),
             clean_latent=arr(state.clean_latent), denoise_mask=arr(state.denoise_mask), positions=arr(state.positions))
    n = SHAPE[2] * SHAPE[3] * SHAPE[4]
    print(f"wrote {out}: latent {arr(state.latent).shape}, mask tail {arr(state.denoise_mask)[0, n - 1:, 0].tolist()}, "
          f"temporal bounds of the two keyframes {arr(state.positions)[0, 0, n].tolist()} {arr(state.positions)[0, 0, n + 6].tolist()}")


if __name__ == "__main__":
    main()
