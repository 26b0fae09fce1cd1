"""Generate tests/golden/apg_guiders.npz by executing the REFERENCE'S OWN LtxAPGGuider and LegacyStatefulAPGGuider
(LTX_2_MLX/components/guiders.py:105-205) through the mlx->torch shim (tools/mlx_shim.py), on the CPU in float32:

    python tools/pin_apg_against_reference.py REFERENCE_DIR      (the directory that holds LTX_2_MLX/)

Inputs from a fixed seed (stored in the file): cond (1, 48, 128) and uncond = 0.7 * cond + 0.5 * noise.  |cond - uncond| is about 46, so of the
thresholds below 5 and 20 bind and 1000 does not.
(a) LtxAPGGuider.guide for every (scale, eta, norm_threshold) of SETTINGS -> apg_<i>, the settings themselves in `settings`.
(b) LegacyStatefulAPGGuider(3, 0.5, 5, momentum 0.5).guide three times in a row with the uncond scaled by 1, 0.9, 0.8 -> legacy_<k>, and
    its running_avg after each call -> legacy_running_<k>; one stateless call (momentum 0, the class's default threshold) -> legacy_stateless.
Data only; no reference source travels.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "LTX_2_MLX")):
    sys.exit("usage: python tools/pin_apg_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
sys.path.insert(0, sys.argv[1])

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()

SEED = 4343
SETTINGS = [(3.0, 1.0, 0.0), (3.0, 0.5, 0.0), (7.5, 0.0, 5.0), (3.0, 0.5, 20.0), (3.0, 0.5, 1000.0), (1.0, 1.0, 0.0)]
LEGACY = (3.0, 0.5, 5.0, 0.5)
UNCOND_FACTORS = (1.0, 0.9, 0.8)


def main():
    from LTX_2_MLX.components.guiders import LegacyStatefulAPGGuider, LtxAPGGuider
    g = torch.Generator().manual_seed(SEED)
    cond = torch.randn(1, 48, 128, generator=g)
    uncond = 0.7 * cond + 0.5 * torch.randn(1, 48, 128, generator=g)
    num = lambda a: shim._unwrap(a).float().numpy()
    out = dict(cond=cond.numpy(), uncond=uncond.numpy(), settings=np.array(SETTINGS, dtype=np.float64), legacy=np.array(LEGACY, dtype=np.float64),
               uncond_factors=np.array(UNCOND_FACTORS, dtype=np.float64))
    for i, (scale, eta, thr) in enumerate(SETTINGS):
        out[f"apg_{i}"] = num(LtxAPGGuider(scale=scale, eta=eta, norm_threshold=thr).guide(shim._wrap(cond), shim._wrap(uncond)))
    assert not LtxAPGGuider(scale=1.0).enabled() and LtxAPGGuider(scale=3.0).enabled()
    assert not LegacyStatefulAPGGuider(scale=0.0, eta=1.0).enabled() and LegacyStatefulAPGGuider(scale=1.0, eta=1.0).enabled()
    st = LegacyStatefulAPGGuider(scale=LEGACY[0], eta=LEGACY[1], norm_threshold=LEGACY[2], momentum=LEGACY[3])
    for k, f in enumerate(UNCOND_FACTORS):
        out[f"legacy_{k}"] = num(st.guide(shim._wrap(cond), shim._wrap(uncond * f)))
        out[f"legacy_running_{k}"] = num(st.running_avg)
    out["legacy_stateless"] = num(LegacyStatefulAPGGuider(scale=3.0, eta=0.5).guide(shim._wrap(cond), shim._wrap(uncond)))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "apg_guiders.npz"), **out)
    print("apg_guiders.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    with torch.no_grad():
        main()
