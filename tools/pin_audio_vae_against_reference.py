"""Generate tests/golden/audio_vae_tiny.npz by executing the REFERENCE'S OWN audio VAE decoder and vocoders
(LTX_2_MLX/model/audio_vae/decoder.py, vocoder.py) through the throw-away mlx->torch shim (tools/mlx_shim.py), on the seeded tiny
weights of tests/audio_vae_ref.py.  The weights travel as a safetensors file and enter the reference models through the reference's
own loaders (load_audio_decoder_weights, load_vocoder_weights, load_vocoder_with_bwe_weights), so the checkpoint key names and the
PyTorch -> MLX layouts are pinned too.  Needs a checkout of the reference (the directory that holds LTX_2_MLX/); the GPU is not used:

    python tools/pin_audio_vae_against_reference.py REFERENCE_DIR

Four runs: AudioDecoder (3 levels: two x2 upsamples, nin_shortcuts, the 4T - 3 trim), an LTX-2.0 Vocoder (resblock "1"), an AMP1
Vocoder and a VocoderWithBWE (a real Hann-windowed DFT basis and a mel basis, base waveform length not a multiple of the hop).
Only inputs, outputs and the seed are stored.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "LTX_2_MLX")):
    sys.exit("usage: python tools/pin_audio_vae_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
REFERENCE = os.path.abspath(sys.argv[1])
sys.path.insert(0, REFERENCE)

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()

import audio_vae_ref as R  # noqa: E402
from LTX_2_MLX.model.audio_vae.decoder import AudioDecoder, load_audio_decoder_weights  # noqa: E402
from LTX_2_MLX.model.audio_vae.vocoder import (MelSTFT, Vocoder, VocoderWithBWE, load_vocoder_weights,  # noqa: E402
                                               load_vocoder_with_bwe_weights)


def _arrays(obj, path="", seen=None):
    """(dotted path, shim array) of every array attribute reachable from a reference module"""
    seen = set() if seen is None else seen
    if id(obj) in seen:
        return
    seen.add(id(obj))
    items = obj.items() if isinstance(obj, dict) else enumerate(obj) if isinstance(obj, (list, tuple)) else vars(obj).items() \
        if hasattr(obj, "__dict__") else []
    for k, v in items:
        if isinstance(v, shim.Arr):
            yield f"{path}{k}", v
        elif isinstance(v, (dict, list, tuple)) or isinstance(v, shim.Module):
            yield from _arrays(v, f"{path}{k}.", seen)


def _all_loaded(model, skip=()):
    """every weight / bias / alpha / beta / filter / basis the reference model holds came from the checkpoint (none left at its zero
    initialisation): a key the loader misses would otherwise pass silently"""
    for name, a in _arrays(model):
        if name.split(".")[-1] in ("weight", "bias", "alpha", "beta", "filter", "forward_basis", "mel_basis") and not any(s in name for s in skip):
            assert float(shim._t(a).abs().sum()) > 0, f"{name} was not loaded"


def _t(a):
    return np.asarray(shim._t(a), dtype=np.float32)


def main():
    from safetensors.torch import save_file
    dec_w, voc_w, amp_w, bwe_w = R.tiny_weights()
    z, mel = R.tiny_inputs()
    out = {"z": z.numpy(), "mel": mel.numpy(), "seed": np.int64(R.TINY_SEED)}
    with tempfile.TemporaryDirectory() as tmp:
        def ckpt(sd, name):
            path = os.path.join(tmp, name)
            save_file({k: v.contiguous() for k, v in sd.items()}, path)
            return path

        d = R.TINY_DECODER
        dec = AudioDecoder(ch=d["ch"], out_ch=d["out_ch"], ch_mult=d["ch_mult"], num_res_blocks=d["num_res_blocks"], z_channels=d["z_channels"],
                           mel_bins=z.shape[3])
        load_audio_decoder_weights(dec, ckpt(dec_w, "dec.safetensors"))
        _all_loaded(dec)
        out["decoder"] = _t(dec(mx.array(z.numpy())))

        def vocoder(cfg, **kw):
            return Vocoder(resblock_kernel_sizes=cfg["resblock_kernel_sizes"], upsample_rates=cfg["upsample_rates"],
                           upsample_kernel_sizes=cfg["upsample_kernel_sizes"], resblock_dilation_sizes=cfg["resblock_dilation_sizes"],
                           upsample_initial_channel=cfg["upsample_initial_channel"], resblock=cfg.get("resblock", "1"), **kw)

        voc = vocoder(R.TINY_VOCODER)
        load_vocoder_weights(voc, ckpt(voc_w, "voc.safetensors"))
        _all_loaded(voc)
        out["vocoder"] = _t(voc(mx.array(mel.numpy())))

        amp = vocoder(R.TINY_AMP, activation="snakebeta")
        load_vocoder_weights(amp, ckpt(amp_w, "amp.safetensors"))
        _all_loaded(amp)
        out["vocoder_amp"] = _t(amp(mx.array(mel.numpy())))

        s = R.TINY_STFT
        vb = VocoderWithBWE(vocoder=vocoder(R.TINY_AMP, activation="snakebeta"),
                            bwe_generator=vocoder(R.TINY_BWE, activation="snakebeta", apply_final_activation=False),
                            mel_stft=MelSTFT(s["n_fft"], s["hop"], s["n_fft"], s["n_mels"]), input_sampling_rate=s["in_rate"],
                            output_sampling_rate=s["out_rate"], hop_length=s["hop"])
        load_vocoder_with_bwe_weights(vb, ckpt(bwe_w, "bwe.safetensors"))
        _all_loaded(vb, skip=("resampler",))           # the resampler's Hann filter is computed, not loaded (vocoder.py:578-581)
        out["vocoder_bwe"] = _t(vb(mx.array(mel.numpy())))
    path = os.path.join(ROOT, "tests", "golden", "audio_vae_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: " + ", ".join(f"{k} {v.shape}" for k, v in out.items()) + f"; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
