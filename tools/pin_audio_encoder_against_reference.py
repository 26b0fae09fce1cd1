"""Generate tests/golden/audio_encoder_tiny.npz by executing the REFERENCE'S OWN audio VAE encoder (LTX_2_MLX/model/audio_vae/encoder.py)
through the throw-away mlx->torch shim (tools/mlx_shim.py), on the seeded tiny weights of tests/audio_encoder_ref.py.  The weights travel
as a safetensors file and enter the reference model through the reference's own loader (load_audio_encoder_weights), so its checkpoint
key spelling and the PyTorch -> MLX layouts are pinned too.  Needs a checkout of the reference (the directory that holds LTX_2_MLX/); the
GPU is not used:

    python tools/pin_audio_encoder_against_reference.py REFERENCE_DIR

One run: AudioEncoder(ch=8, ch_mult=(1, 2, 4), num_res_blocks=1, z_channels=2, mel_bins=4) on a (1, 2, 13, 16) mel: two strided
Downsample2d over an odd then an odd extent along time (13 -> 7 -> 4) and an even one along mel (16 -> 8 -> 4), nin_shortcuts, the
norm-less SiLU tail, and patchify -> normalize -> unpatchify with non-trivial statistics of z_channels * mel_bins = 8 entries.
Only the input, the output and the seed are stored.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "LTX_2_MLX")):
    sys.exit("usage: python tools/pin_audio_encoder_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
REFERENCE = os.path.abspath(sys.argv[1])
sys.path.insert(0, REFERENCE)

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()

import audio_encoder_ref as R  # noqa: E402
from LTX_2_MLX.model.audio_vae.encoder import AudioEncoder, encode_audio, load_audio_encoder_weights  # noqa: E402


def main():
    from safetensors.torch import save_file
    sd = R.tiny_weights()
    mel = R.tiny_input()
    c = R.TINY_ENCODER
    enc = AudioEncoder(ch=c["ch"], ch_mult=c["ch_mult"], num_res_blocks=c["num_res_blocks"], z_channels=c["z_channels"], mel_bins=R.TINY_MEL_BINS)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "enc.safetensors")
        save_file({k: v.contiguous() for k, v in sd.items()}, path)
        load_audio_encoder_weights(enc, path)
    # every conv of the reference model came from the file (none left at its zero initialisation), and so did the statistics
    convs = [enc.conv_in, enc.mid_block_1.conv1, enc.mid_block_1.conv2, enc.mid_block_2.conv1, enc.mid_block_2.conv2, enc.conv_out]
    for level in enc.down_blocks:
        for rb in level["res_blocks"]:
            convs += [rb.conv1, rb.conv2] + ([rb.skip] if rb.skip is not None else [])
        if level["downsample"] is not None:
            convs.append(level["downsample"].conv)
    assert len(convs) == sum(k.endswith(".weight") for k in sd)
    for cv in convs:
        assert float(shim._t(cv.weight).abs().sum()) > 0 and float(shim._t(cv.bias).abs().sum()) > 0, "a conv was not loaded"
    assert np.array_equal(np.asarray(shim._t(enc.per_channel_statistics.std_of_means)), sd[R.STD].numpy())
    y = np.asarray(shim._t(encode_audio(mx.array(mel.numpy()), enc)), dtype=np.float32)
    assert y.shape == (1, 2, 4, 4), y.shape
    out = {"mel": mel.numpy(), "latent": y, "seed": np.int64(R.TINY_SEED)}
    path = os.path.join(ROOT, "tests", "golden", "audio_encoder_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: " + ", ".join(f"{k} {v.shape}" for k, v in out.items()) + f"; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
