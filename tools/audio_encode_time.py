"""Time the audio path INTO the model on the MI355X, fp32 end to end, random weights: AudioProcessor.waveform_to_mel and AudioEncoder on a
5 s and a 20 s clip (T_mel = 501 / 2001), and the two Downsample2d convolutions as the strided kernel against what it replaces (the
stride-1 kernel followed by a [::2, ::2] subsample) on the same tensors, alternated in one process.  One JSON line per measurement:
median / min / max ms of device events over the timed repetitions after warm-up, the convolution FLOPs counted from the launched shapes.

    python tools/audio_encode_time.py [--reps 20] [--warmup 5] [--only encode,downsample] [--seconds 5,20]

The per-kernel share comes from a run of its own under the profiler (`rocprofv3 --kernel-trace --stats -- python
tools/audio_encode_time.py --only encode --seconds 5 --reps 3 --warmup 1`); see profiles/audio_encode.md."""
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


def _install_counters():
    def wrap(fn, flops):
        def wrapped(*a, **kw):
            FLOPS[0] += flops(*a, **kw)
            return fn(*a, **kw)
        return wrapped

    def conv2d(x, w, bias, c_out, kh, kw, pad_h, pad_w, *, stride=(1, 1), **_):
        h, wd, c_in = x.shape
        return 2 * ((h + pad_h - kh) // stride[0] + 1) * ((wd + 2 * pad_w - kw) // stride[1] + 1) * c_out * kh * kw * c_in

    K.audio_conv2d = wrap(K.audio_conv2d, conv2d)
    K.audio_conv2d_strided = wrap(K.audio_conv2d_strided, conv2d)


def _events(fns, reps, warmup):
    """fns: name -> callable, alternated inside every repetition; -> name -> [ms]"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b))
    return ms


def _line(**kw):
    print(json.dumps(kw), flush=True)


def _stats(times):
    return dict(median_ms=round(statistics.median(times), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="encode,downsample")
    ap.add_argument("--seconds", default="5,20")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("audio_encode_time.py measures on the GPU only")
    _install_counters()
    from ltx_2_mlx_amd.model.audio_vae import AudioEncoder, AudioProcessor
    dev = torch.device("cuda:0")
    _line(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip, reps=a.reps, warmup=a.warmup)
    g = torch.Generator().manual_seed(0)
    enc = AudioEncoder(device=dev)
    enc.init_random_weights(1)
    proc = AudioProcessor(device=dev)
    todo = a.only.split(",")
    for sec in [int(s) for s in a.seconds.split(",")]:
        wave = (0.1 * torch.randn(2, sec * 16000, generator=g)).to(dev)
        t_mel = proc.mel_frames(wave.shape[1])
        if "encode" in todo:
            mel = proc.waveform_to_mel(wave, 16000)
            FLOPS[0] = 0
            z = enc(mel)
            torch.cuda.synchronize()
            flops = FLOPS[0]
            ms = _events({"waveform_to_mel": lambda: proc.waveform_to_mel(wave, 16000), "encoder": lambda: enc(mel)}, a.reps, a.warmup)
            _line(what="waveform_to_mel", seconds=sec, t_mel=t_mel, **_stats(ms["waveform_to_mel"]))
            med = statistics.median(ms["encoder"])
            _line(what="AudioEncoder", seconds=sec, t_mel=t_mel, latent=list(z.shape), **_stats(ms["encoder"]), conv_tflop=round(flops / 1e12, 4),
                  frac_fp32_peak=round(flops / (med * 1e-3) / (PEAK_TF * 1e12), 4))
        if "downsample" in todo:
            h, wd = t_mel, 64
            for lvl, c in ((0, enc.ch * enc.ch_mult[0]), (1, enc.ch * enc.ch_mult[1])):
                name = f"down.{lvl}.downsample.conv"
                w, b = enc._packed[f"audio_vae.encoder.{name}.weight"], enc._w[f"audio_vae.encoder.{name}.bias"]
                x = torch.randn(h, wd, c, generator=g).to(dev)
                strided = lambda: K.audio_conv2d_strided(x, w, b, c, 3, 3, 2, 1, stride=(2, 2))          # noqa: E731
                full = lambda: K.audio_conv2d(x, w, b, c, 3, 3, 2, 1)[::2, ::2].contiguous()              # noqa: E731
                same = bool(torch.equal(strided(), full()))
                ms = _events({"strided": strided, "stride1_subsample": full}, a.reps, a.warmup)
                ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
                fl = 2 * ho * wo * c * 9 * c
                s, f = statistics.median(ms["strided"]), statistics.median(ms["stride1_subsample"])
                _line(what=name, seconds=sec, input=[h, wd, c], output=[ho, wo, c], bit_identical=same, strided=_stats(ms["strided"]),
                      stride1_subsample=_stats(ms["stride1_subsample"]), ratio=round(f / s, 3), strided_gflop=round(fl / 1e9, 3),
                      strided_frac_fp32_peak=round(fl / (s * 1e-3) / (PEAK_TF * 1e12), 4))
                h, wd = ho, wo


if __name__ == "__main__":
    main()
