"""The captured STG loop against the captured guided loop at the bench geometry (768x512x65 -> N = 9 * 16 * 24 = 3456 tokens, video-only model,
full width, 48 layers, bf16, random weights): ms per step of the replay alone, timed with device events, the loops alternated --
  guided        ltx2_dit_graph_capture_guided: forward(ctx), forward(neg), the guided Euler kernel
  STG [29]      ltx2_dit_graph_capture_stg, block 29's video self-attention skipped in the third pass
  STG all       the same with every block's skipped
A step of the STG loop is three forwards minus the skipped self-attentions against two.

    python tools/stg_step_time.py [--steps 8] [--reps 5] [--layers 48] [out.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd.components import LTX2Scheduler, VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import video_tools_for  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = LTXModel(num_layers=a.layers, device=dev)
    m.init_random_weights(seed=0)
    neg = m.clone_sharing_weights()
    g = torch.Generator(device=dev).manual_seed(3)
    st = video_tools_for(VideoLatentPatchifier(1), 65, 512, 768, 24.0).create_initial_state(device=dev)
    n = st.latent.shape[1]
    noise = torch.randn(n, 128, generator=g, device=dev)
    ctx, nctx = (0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev) for _ in range(2))
    sig = [float(s) for s in LTX2Scheduler().execute(steps=a.steps)]
    m.prepare(ctx, st.positions)
    neg.prepare(nctx, st.positions)
    lat, vel_p = noise.clone(), torch.empty_like(noise)
    one = [b for b in (29,) if b < a.layers] or [a.layers - 1]
    ways = {"guided (two forwards)": (lambda: m.capture_guided_graph(neg, lat, sig, 3.0), m.replay_guided_graph, None),
            f"STG, block {one[0]} skipped": (lambda: m.capture_stg_graph(neg, lat, sig, 3.0, 1.0, vel_p), m.replay_stg_graph, one),
            "STG, all blocks skipped": (lambda: m.capture_stg_graph(neg, lat, sig, 3.0, 1.0, vel_p), m.replay_stg_graph, None)}
    times = {k: [] for k in ways}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for rep in range(a.reps + 1):               # the first round warms up; alternated afterwards.  One context holds one graph: capture, then time the replay alone
            for name, (capture, replay, blocks) in ways.items():
                if name != "guided (two forwards)":
                    m.set_stg_blocks(blocks)
                lat.copy_(noise)
                capture()
                replay()                            # the first launch of a fresh graph uploads it
                lat.copy_(noise)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                replay()
                e1.record()
                e1.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1) / a.steps)
    base = statistics.median(times["guided (two forwards)"])
    lines = [f"N = {n} tokens, {a.layers} layers, full width, bf16, cfg 3, stg 1, cutoff 1, {a.steps} steps per replay, {a.reps} alternated replays, device events", "",
             "| captured loop | ms / step, median | min | max | x guided |", "|---|---|---|---|---|"]
    for k, v in times.items():
        lines.append(f"| {k} | {statistics.median(v):.2f} | {min(v):.2f} | {max(v):.2f} | {statistics.median(v) / base:.3f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
