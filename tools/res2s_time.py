"""One res_2s step at the bench geometry's half-resolution stage (N = 3456 tokens, full width, 48 layers, bf16, random weights, cfg 3):
ms per step three ways, alternated --
  eager composition   the loop written over the EXISTING X0Model calls and torch fp32 glue (runs at the parent commit too: the
                      comparison for what the fusion returns)
  one call            LTXModel.res2s_step_ per step (ltx2_dit_res2s_step)
  graph               one captured graph of all the steps (ltx2_dit_graph_capture_res2s)
and the two kernels alone against a device copy of the same bytes, with and without the 100 bong iterations.

    python tools/res2s_time.py [--steps 4] [--reps 3] [--layers 48] [out.md]
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd.components import VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning import VideoLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, X0Model  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import modality_from_state, post_process_latent  # noqa: E402
from ltx_2_mlx_amd.types import VideoLatentShape  # noqa: E402


def phi(j, z):
    if abs(z) < 1e-10:
        return 1.0 / math.factorial(j)
    return (math.exp(z) - sum(z**k / math.factorial(k) for k in range(j))) / z**j


def eager_composition(x0m, st, sig, ctx, nctx, cfg):
    """Nothing newer than the parent commit: two X0Model calls per evaluation, torch glue, the bong loop as 200 torch passes."""
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        h = -math.log(sn / s)
        a21, b2 = 0.5 * phi(1, -h * 0.5), phi(2, -h) / 0.5
        b1 = phi(1, -h) - b2

        def denoised(state, sigma):
            c, u = x0m(modality_from_state(state, ctx, sigma, uniform=True)), x0m(modality_from_state(state, nctx, sigma, uniform=True))
            return post_process_latent(u + cfg * (c - u), state.denoise_mask, state.clean_latent)

        d = denoised(st, s)
        an = st.latent.float()
        e = d - an
        xm = an + h * a21 * e
        if h < 0.5 and s > 0.03:
            for _ in range(100):
                an = xm - h * a21 * e
                e = d - an
        d2 = denoised(st.replace(latent=xm), math.sqrt(s * sn))
        st = st.replace(latent=an + h * (b1 * e + b2 * (d2 - an)))
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = LTXModel(num_layers=a.layers, device=dev)
    m.init_random_weights(seed=0)
    g = torch.Generator(device=dev).manual_seed(3)
    tools = VideoLatentTools(VideoLatentPatchifier(1), VideoLatentShape(1, 128, 9, 16, 24), fps=25.0)
    st = tools.create_initial_state(device=dev)
    n = st.latent.shape[1]
    st = st.replace(latent=torch.randn(1, n, 128, generator=g, device=dev))
    ctx = 0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev)
    nctx = 0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev)
    # a table above 0.001 whose first step takes the bong iteration and whose others do not
    sig = [1.0, 0.7] + [0.7 * 0.25 ** (i + 1) for i in range(a.steps - 1)]
    x0m = X0Model(m)
    ways = {"eager composition over X0Model (runs at the parent commit)": lambda: eager_composition(x0m, st, sig, ctx, nctx, 3.0)}
    K = None
    try:
        from ltx_2_mlx_amd.pipelines.common import res2s_denoise_loop
        from ltx_2_mlx_amd import kernels as K
        ways["one res2s_step_ call per step"] = lambda: res2s_denoise_loop(x0m, st, sig, ctx, nctx, 3.0, use_hip_graph=False)
        ways["graph replay (capture included)"] = lambda: res2s_denoise_loop(x0m, st, sig, ctx, nctx, 3.0, use_hip_graph=True)
    except ImportError:              # the parent commit: the yardstick alone
        pass
    best = {k: float("inf") for k in ways}
    for rep in range(a.reps + 1):                   # the first round warms up (allocation, the per-prompt setup); alternated afterwards
        for name, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                best[name] = min(best[name], (time.perf_counter() - t0) / a.steps * 1e3)
    lines = [f"N = {n} tokens, {a.layers} layers, full width, bf16, cfg 3, {a.steps} steps (the first takes the bong iteration), best of {a.reps}", "",
             "| res_2s step (4 DiT evaluations) | ms / step |", "|---|---|"]
    lines += [f"| {k} | {v:.2f} |" for k, v in best.items()]
    if K is not None:
        neg = m.clone_sharing_weights()
        lat = st.latent[0].clone()
        m.prepare(ctx, st.positions)
        neg.prepare(nctx, st.positions)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.capture_res2s_graph(neg, lat, sig, 3.0)
            m.replay_res2s_graph()
            side.synchronize()
            replay = float("inf")
            for _ in range(a.reps):
                t0 = time.perf_counter()
                m.replay_res2s_graph()
                side.synchronize()
                replay = min(replay, (time.perf_counter() - t0) / a.steps * 1e3)
        lines += [f"| graph replay alone | {replay:.2f} |", ""]
        # the kernels alone beside a device copy of the bytes they move
        x, vc, vu, xm, an, e = (torch.randn(n, 128, generator=g, device=dev) for _ in range(6))
        ts = torch.full((1,), 0.5, device=dev)

        def timed(fn, iters=200):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters * 1e3

        mb = 6 * n * 128 * 4 / 1e6          # midpoint: 3 in, 3 out; combine: 5 in, 1 out
        src, dst = torch.empty(3 * n * 128, device=dev), torch.empty(3 * n * 128, device=dev)
        t_c = min(timed(lambda: dst.copy_(src)) for _ in range(3))
        for name, fn in (("midpoint, n_bong 0", lambda: K.res2s_midpoint(x, vc, vu, ts, 3.0, 0.16, 0, x_mid=xm, anchor=an, eps1=e)),
                         ("midpoint, n_bong 100", lambda: K.res2s_midpoint(x, vc, vu, ts, 3.0, 0.16, 100, x_mid=xm, anchor=an, eps1=e)),
                         ("combine", lambda: K.res2s_combine(xm, vc, vu, ts, 3.0, an, e, 0.36, -0.05, 0.91, out=x))):
            t_k = min(timed(fn) for _ in range(3))
            lines.append(f"{name}: {t_k:.1f} us for {mb:.1f} MB ({mb / t_k * 1e-3:.2f} TB/s)")
        lines.append(f"device copy of the same bytes: {t_c:.1f} us ({mb / t_c * 1e-3:.2f} TB/s)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
