"""Generate tests/golden/temporal_upscaler_tiny.npz by executing the REFERENCE'S OWN TemporalUpscaler and
load_temporal_upscaler_weights (LTX_2_MLX/model/upscaler/temporal.py) through the mlx->torch shim (tools/mlx_shim.py, whose
nn.GroupNorm follows MLX's definition):

    python tools/pin_temporal_upscaler_against_reference.py REFERENCE_DIR      (the directory that holds LTX_2_MLX/)

Tiny configuration (latent 64, hidden 64, one block per stage, 32 groups: two channels per group, so the interleaved grouping
c % 32 differs from the contiguous c // 2) on input (1, 64, 3, 5, 6).  Only the input, the seeds that regenerate the weights
(tests/temporal_upscaler_ref.make_weights) and the output (1, 64, 5, 5, 6) are stored; no reference source travels.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "LTX_2_MLX")):
    sys.exit("usage: python tools/pin_temporal_upscaler_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
sys.path.insert(0, sys.argv[1])

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()

import temporal_upscaler_ref as R  # noqa: E402


def main():
    from safetensors.torch import save_file
    from LTX_2_MLX.model.upscaler.temporal import TemporalUpscaler, load_temporal_upscaler_weights
    cfg = R.TINY
    w = R.make_weights(cfg, R.TINY_SEED)
    up = TemporalUpscaler(latent_channels=cfg.latent_channels, hidden_channels=cfg.hidden_channels, num_res_blocks=cfg.num_res_blocks,
                          num_groups=cfg.num_groups)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "tiny.safetensors")
        save_file({k: v.contiguous() for k, v in w.items()}, path)
        load_temporal_upscaler_weights(up, path)
    x = R.tiny_input()
    y = up(shim.Arr(x)).t.detach().float()
    assert tuple(y.shape) == (1, 64, 5, 5, 6), y.shape
    out = os.path.join(ROOT, "tests", "golden", "temporal_upscaler_tiny.npz")
    np.savez(out, x=x.numpy(), y=y.numpy(), weight_seed=np.int64(R.TINY_SEED), input_seed=np.int64(R.TINY_INPUT_SEED),
             config=np.array([cfg.latent_channels, cfg.hidden_channels, cfg.num_res_blocks, cfg.num_groups], dtype=np.int64))
    print(f"wrote {out}: x {tuple(x.shape)} -> y {tuple(y.shape)}, |y| rms {float(y.pow(2).mean().sqrt()):.4f}")
    ours = R.forward(x, w, cfg, checkpoint_semantics=False)
    print(f"restatement vs reference: max abs {float((ours - y).abs().max()):.3e}")
    other = R.forward(x, w, cfg, checkpoint_semantics=True)
    print(f"checkpoint semantics vs reference: rel-L2 {float((other - y).norm() / y.norm()):.3e}")


if __name__ == "__main__":
    main()
