"""The projected guidance step (CFG*, APG) at the bench geometry (N = 3456 tokens, full width, 48 layers, bf16, random weights): ms per guided
step three ways, each a median of --reps runs after a warm-up, timed with device events --
  eager glue   the existing joint_denoise_loop(video_guider=...): two X0Model calls, the torch guider, ltx2_euler_step
  one call     LTXModel.projected_step_ per step (ltx2_dit_projected_step)
  graph        replay of one captured graph of all the steps (ltx2_dit_graph_capture_projected), capture not included
and the kernel pair alone (ltx2_guidance_sums + ltx2_projected_euler_step) against a device copy of the bytes they move.

    python tools/projected_guidance_time.py [--steps 2] [--reps 20] [--layers 48] [out.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.components import CFGStarRescalingGuider, EulerDiffusionStep, LTX2Scheduler, LtxAPGGuider, VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning import VideoLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, X0Model  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import joint_denoise_loop, projected_denoise_loop, projected_guider_args  # noqa: E402
from ltx_2_mlx_amd.types import VideoLatentShape  # noqa: E402


def event_ms(fn, stream=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = LTXModel(num_layers=a.layers, device=dev)
    m.init_random_weights(seed=0)
    g = torch.Generator(device=dev).manual_seed(3)
    tools = VideoLatentTools(VideoLatentPatchifier(1), VideoLatentShape(1, 128, 9, 16, 24), fps=24.0)
    st = tools.create_initial_state(device=dev)
    n = st.latent.shape[1]
    st = st.replace(latent=torch.randn(1, n, 128, generator=g, device=dev))
    ctx = 0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev)
    nctx = 0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev)
    sig = [float(s) for s in LTX2Scheduler().execute(steps=a.steps)]
    x0m, stepper = X0Model(m), EulerDiffusionStep()
    lines = [f"N = {n} tokens, {a.layers} layers, full width, bf16, scale 3, {a.steps} steps per run, median of {a.reps} runs after one warm-up, device events", ""]
    for name, guider in (("CFG*", CFGStarRescalingGuider(3.0)), ("APG (eta 0.5, norm_threshold 5)", LtxAPGGuider(3.0, 0.5, 5.0))):
        ways = {
            "eager glue (existing)": lambda: joint_denoise_loop(x0m, False, st, None, sig, ctx, None, stepper, use_hip_graph=False,
                                                                negative_video_context=nctx, video_guider=guider),
            "one projected_step_ call per step": lambda: projected_denoise_loop(x0m, st, sig, ctx, nctx, guider, stepper, use_hip_graph=False),
        }
        times = {k: [] for k in ways}
        for rep in range(a.reps + 1):                   # the first round warms up (allocation, the per-prompt setup); alternated afterwards
            for k, fn in ways.items():
                torch.cuda.synchronize()
                t = event_ms(fn)
                if rep:
                    times[k].append(t / a.steps)
        neg = m.clone_sharing_weights()
        lat = st.latent[0].clone()
        m.prepare(ctx, st.positions, per_token=False)
        neg.prepare(nctx, st.positions, per_token=False)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        replay = []
        with torch.cuda.stream(side):
            m.capture_projected_graph(neg, lat, sig, **projected_guider_args(guider))
            m.replay_projected_graph()
            side.synchronize()
            for _ in range(a.reps):
                replay.append(event_ms(m.replay_projected_graph, side) / a.steps)
        lines += [f"| {name} | ms / step |", "|---|---|"] + [f"| {k} | {statistics.median(v):.2f} |" for k, v in times.items()]
        lines += [f"| graph replay | {statistics.median(replay):.2f} |", ""]

    # the kernel pair alone beside a device copy of the bytes it moves: sums reads x and two velocities, the step reads them again and writes x
    x, vc, vu = (torch.randn(n, 128, generator=g, device=dev) for _ in range(3))
    ts = torch.tensor([0.5], device=dev)
    part = K.guidance_sums(x, vc, vu, ts)
    src, dst = torch.empty(7 * n * 128 // 2, device=dev), torch.empty(7 * n * 128 // 2, device=dev)     # a copy reads and writes: half the elements

    def pair():
        K.guidance_sums(x, vc, vu, ts, partials=part)
        K.projected_euler_step(x, vc, vu, ts, part, 1, 3.0, 0.5, 5.0, 0.5, 0.25, out=x)

    def per_call_us(fn, iters=200):
        fn()
        return event_ms(lambda: [fn() for _ in range(iters)]) / iters * 1e3

    t_pair = statistics.median(per_call_us(pair) for _ in range(5))
    t_sums = statistics.median(per_call_us(lambda: K.guidance_sums(x, vc, vu, ts, partials=part)) for _ in range(5))
    t_copy = statistics.median(per_call_us(lambda: dst.copy_(src)) for _ in range(5))
    mb = 7 * n * 128 * 4 / 1e6
    lines += [f"kernel pair alone (APG, no mask): {t_pair:.1f} us for {mb:.1f} MB ({mb / t_pair:.2f} TB/s), of which the sums kernel {t_sums:.1f} us; "
              f"device copy of the same bytes: {t_copy:.1f} us ({mb / t_copy:.2f} TB/s); {K.guidance_sums_blocks(n, 128)} partial rows"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
