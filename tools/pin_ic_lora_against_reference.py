"""Generate tests/golden/ic_lora_conditioning.npz by executing the REFERENCE'S OWN conditioning classes in the order its IC-LoRA pipeline
applies them (LTX_2_MLX/pipelines/ic_lora.py: image conditionings first, control conditionings after them) through the mlx->torch shim
(tools/mlx_shim.py):

    python tools/pin_ic_lora_against_reference.py REFERENCE_DIR      (the directory that holds LTX_2_MLX/)

State (1, 128, 2, 2, 3) at fps 24 that already holds one image conditioning (VideoConditionByLatentIndex, latent frame 0, strength 0.9); then
a control latent of the whole clip, (1, 128, 2, 2, 3), appended by VideoConditionByKeyframeIndex at frame_idx 0 with strength 0.95.
Stored: the seeded inputs and the four arrays of the resulting state (latent, clean latent, denoise mask, positions).  Data only; no
reference source travels.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "LTX_2_MLX")):
    sys.exit("usage: python tools/pin_ic_lora_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
sys.path.insert(0, sys.argv[1])

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()

SHAPE = (1, 128, 2, 2, 3)
FPS = 24.0
IMAGE_STRENGTH, CONTROL_STRENGTH = 0.9, 0.95
SEED = 21


def main():
    from LTX_2_MLX.components.patchifiers import VideoLatentPatchifier
    from LTX_2_MLX.conditioning.keyframe import VideoConditionByKeyframeIndex
    from LTX_2_MLX.conditioning.latent import VideoConditionByLatentIndex
    from LTX_2_MLX.conditioning.tools import VideoLatentTools
    from LTX_2_MLX.pipelines.common import apply_conditionings
    from LTX_2_MLX.types import VideoLatentShape
    g = torch.Generator().manual_seed(SEED)
    initial = torch.randn(SHAPE, generator=g)
    image = torch.randn(SHAPE[0], SHAPE[1], 1, SHAPE[3], SHAPE[4], generator=g)
    control = torch.randn(SHAPE, generator=g)
    tools = VideoLatentTools(patchifier=VideoLatentPatchifier(patch_size=1), target_shape=VideoLatentShape.from_shape(SHAPE), fps=FPS)
    state = tools.create_initial_state(dtype=mx.float32, initial_latent=shim.Arr(initial))
    conds = [VideoConditionByLatentIndex(latent=shim.Arr(image), strength=IMAGE_STRENGTH, latent_idx=0),
             VideoConditionByKeyframeIndex(keyframes=shim.Arr(control), frame_idx=0, strength=CONTROL_STRENGTH)]
    state = apply_conditionings(state, conds, tools)
    arr = lambda a: a.t.detach().float().numpy()
    out = os.path.join(ROOT, "tests", "golden", "ic_lora_conditioning.npz")
    np.savez(out, initial=initial.numpy(), image=image.numpy(), control=control.numpy(), image_strength=np.float64(IMAGE_STRENGTH),
             control_strength=np.float64(CONTROL_STRENGTH), fps=np.float64(FPS), latent=arr(state.latent), clean_latent=arr(state.clean_latent),
             denoise_mask=arr(state.denoise_mask), positions=arr(state.positions))
    n = SHAPE[2] * SHAPE[3] * SHAPE[4]
    print(f"wrote {out}: latent {arr(state.latent).shape}, mask {arr(state.denoise_mask).reshape(-1)[[0, n - 1, n, 2 * n - 1]].tolist()}, "
          f"temporal bounds of the first and last control token {arr(state.positions)[0, 0, n].tolist()} {arr(state.positions)[0, 0, 2 * n - 1].tolist()}")


if __name__ == "__main__":
    main()
