"""Time the audio VAE decoder and both vocoder forms on the 121-frame clip (127 audio latent frames -> 505 mel frames, ~5 s) with
random weights, fp32 end to end.  Prints one JSON line per component: median / min / max wall ms over the timed repetitions (after
warm-up), the algorithmic convolution FLOPs counted from the launched shapes, and the fraction of the 157.3 TF fp32 matrix peak.

    python tools/audio_decode_time.py [--frames 127] [--reps 10] [--warmup 3] [--only decoder,vocoder,bwe]

The BWE form uses the reference's inner-vocoder defaults (AMP1, 1024 channels) and a BWE generator consistent with hop 240 at x2
(upsample rates 6-5-2-2-2-2 = 480 = 2 x 240, n_fft 2048, 64 mel bins per channel)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ltx_2_mlx_amd import kernels as K  # noqa: E402

PEAK_TF = 157.3
FLOPS = [0]


def _counting(fn, flops):
    def wrapped(*a, **kw):
        FLOPS[0] += flops(*a, **kw)
        return fn(*a, **kw)
    return wrapped


def _install_counters():
    def conv1d(x, w, bias, c_out, k, *, stride=1, dilation=1, padding=0, t_out=None, c_in=None, **_):
        c_in = x.shape[1] if c_in is None else c_in
        t_out = (x.shape[0] + 2 * padding - dilation * (k - 1) - 1) // stride + 1 if t_out is None else t_out
        return 2 * t_out * c_out * k * c_in

    def conv2d(x, w, bias, c_out, kh, kw, pad_h, pad_w, *, upsample=False, **_):
        h, wd, c_in = x.shape
        return 2 * ((2 * h - 1) * 2 * wd if upsample else h * wd) * c_out * kh * kw * c_in

    def convt(x, w, bias, c_out, k, rate, padding, **_):
        return 2 * ((x.shape[0] - 1) * rate + k - 2 * padding) * c_out * ((k + rate - 1) // rate) * x.shape[1]

    K.audio_conv1d = _counting(K.audio_conv1d, conv1d)
    K.audio_conv2d = _counting(K.audio_conv2d, conv2d)
    K.audio_conv_transpose1d = _counting(K.audio_conv_transpose1d, convt)


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    FLOPS[0] = 0
    fn()
    torch.cuda.synchronize()
    flops = FLOPS[0]
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms, flops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=127)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="decoder,vocoder,bwe")
    a = ap.parse_args()
    _install_counters()
    from ltx_2_mlx_amd.model.audio_vae import AudioDecoder, MelSTFT, Vocoder, VocoderWithBWE
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    z = torch.randn(1, 8, a.frames, 16, generator=g).to(dev)
    mel = torch.randn(1, 2, 4 * a.frames - 3, 64, generator=g).to(dev)
    todo = a.only.split(",")
    runs = {}
    if "decoder" in todo:
        dec = AudioDecoder(device=dev)
        dec.init_random_weights(1)
        runs["decoder"] = lambda: dec(z)
    if "vocoder" in todo:
        voc = Vocoder(device=dev)
        voc.init_random_weights(2)
        runs["vocoder_ltx20"] = lambda: voc(mel)
    if "bwe" in todo:
        inner = Vocoder(resblock="AMP1", activation="snakebeta", device=dev)
        bwe = Vocoder(upsample_rates=[6, 5, 2, 2, 2, 2], upsample_kernel_sizes=[12, 11, 4, 4, 4, 4], upsample_initial_channel=256, resblock="AMP1",
                      activation="snakebeta", apply_final_activation=False, output_sample_rate=48000, device=dev)
        inner.init_random_weights(3)
        bwe.init_random_weights(4)
        ms = MelSTFT(2048, 240, 2048, 64, device=dev)
        ms.set_buffers(0.01 * torch.randn(2 * 1025, 1, 2048, generator=g), None, torch.rand(64, 1025, generator=g))
        vb = VocoderWithBWE(inner, bwe, ms, 24000, 48000, 240)
        runs["vocoder_bwe_ltx23"] = lambda: vb(mel)
    for name, fn in runs.items():
        times, flops = _time(fn, a.reps, a.warmup)
        med = statistics.median(times)
        print(json.dumps({"component": name, "latent_frames": a.frames, "mel_frames": 4 * a.frames - 3, "median_ms": round(med, 3),
                          "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "reps": a.reps, "warmup": a.warmup,
                          "conv_tflop": round(flops / 1e12, 4), "frac_fp32_peak": round(flops / (med * 1e-3) / (PEAK_TF * 1e12), 4)}), flush=True)


if __name__ == "__main__":
    main()
