"""What the Euler-ancestral step costs.  Two tables, medians over device events, the ways alternated:
  kernels  at the headline geometry, the video latent [6144][128] and the pair with an audio latent [126][128], uniform timesteps, no mask:
           ltx2_guided_euler_step (the yardstick: the same kernel as before this sampler), ltx2_ancestral_euler_step (guided and not), the noise
           fill ltx2_philox_normal alone, the fill + the Euler step + a torch add as separate launches, the pair launches, and the element-wise
           form (operands 4 bytes off a 16-byte boundary: every thread evaluates a whole Philox quad for one element).  Each figure is the
           device's time per launch inside ONE captured graph of `--launches` launches that rotate over `--sets` operand sets (24 x 5 operands x
           3.1 MB = 377 MB, past the 256 MB last-level cache), so the bytes come from HBM.
  loops    the video-only DiT at the bench geometry (N = 3456 tokens, S = 1024, 48 layers, bf16, random weights), the 8 distilled sigmas: one
           C call per step and one captured graph, the Euler loop (ltx2_dit_denoise_step / ltx2_dit_graph_capture, as before this sampler)
           against the ancestral loop (ltx2_dit_ancestral_step / ltx2_dit_graph_capture_ancestral), unguided as the distilled route runs.

    python tools/bench_ancestral.py [--reps 20] [--layers 48] [--skip-loops] [out.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.components import DISTILLED_SIGMA_VALUES, EulerAncestralDiffusionStep, VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning import VideoLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import modality_from_state  # noqa: E402
from ltx_2_mlx_amd.types import VideoLatentShape  # noqa: E402

ROWS, AROWS, C = 6144, 126, 128
SIGMA, SIGMA_NEXT = 0.909375, 0.725


def span(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_table(a, dev):
    g = torch.Generator(device=dev).manual_seed(3)
    word = K.seed_word(42, dev)
    up, down = EulerAncestralDiffusionStep._get_ancestral_step(SIGMA, SIGMA_NEXT, 1.0)
    ts = torch.full((1,), SIGMA, device=dev)
    names = ("x", "vc", "vu", "out", "z")

    def operand_sets(rows, offset=0):
        """a.sets sets of five [rows][C] operands; offset 1: every base pointer 4 bytes off a 16-byte boundary (the element-wise form)"""
        return [{k: torch.randn(rows * C + 4, generator=g, device=dev)[offset:offset + rows * C].view(rows, C) for k in names} for _ in range(a.sets)]

    v, vo, au = operand_sets(ROWS), operand_sets(ROWS, 1), operand_sets(AROWS)
    seg = lambda t, guided: dict(x=t["x"], vel_cond=t["vc"], vel_uncond=t["vu"] if guided else None, timesteps=ts, cfg_scale=3.0, out=t["out"])      # noqa: E731

    def separate(t):
        K.philox_normal(ROWS * C, word, 3, 0)
        K.guided_euler_step(t["x"], t["vc"], t["vu"], ts, 3.0, SIGMA, down, out=t["out"])
        t["out"].add_(t["z"], alpha=up)

    mb, amb = ROWS * C * 4 / 1e6, AROWS * C * 4 / 1e6
    ways = [("guided_euler_step (yardstick)", 4 * mb, lambda i: K.guided_euler_step(v[i]["x"], v[i]["vc"], v[i]["vu"], ts, 3.0, SIGMA, SIGMA_NEXT, out=v[i]["out"])),
            ("ancestral_euler_step, guided", 4 * mb, lambda i: K.ancestral_euler_step(v[i]["x"], v[i]["vc"], v[i]["vu"], ts, 3.0, SIGMA, up, down, word, 3, out=v[i]["out"])),
            ("ancestral_euler_step, guided, sigma_up = 0 (no Philox)", 4 * mb,
             lambda i: K.ancestral_euler_step(v[i]["x"], v[i]["vc"], v[i]["vu"], ts, 3.0, SIGMA, 0.0, down, word, 3, out=v[i]["out"])),
            ("ancestral_euler_step, unguided", 3 * mb, lambda i: K.ancestral_euler_step(v[i]["x"], v[i]["vc"], None, ts, 1.0, SIGMA, up, down, word, 3, out=v[i]["out"])),
            ("philox_normal fill alone (into a fresh tensor)", mb, lambda i: K.philox_normal(ROWS * C, word, 3, 0)),
            ("fill + guided_euler_step + torch add: three launches", 8 * mb, lambda i: separate(v[i])),
            ("guided_euler_step_pair (yardstick)", 4 * (mb + amb), lambda i: K.guided_euler_step_pair(seg(v[i], True), seg(au[i], True), SIGMA, SIGMA_NEXT)),
            ("ancestral_euler_step_pair, guided", 4 * (mb + amb), lambda i: K.ancestral_euler_step_pair(seg(v[i], True), seg(au[i], True), SIGMA, up, down, word, 3)),
            ("guided_euler_step, element-wise form", 4 * mb, lambda i: K.guided_euler_step(vo[i]["x"], vo[i]["vc"], vo[i]["vu"], ts, 3.0, SIGMA, SIGMA_NEXT, out=vo[i]["out"])),
            ("ancestral_euler_step, guided, element-wise form", 4 * mb,
             lambda i: K.ancestral_euler_step(vo[i]["x"], vo[i]["vc"], vo[i]["vu"], ts, 3.0, SIGMA, up, down, word, 3, out=vo[i]["out"]))]
    graphs = []
    for _, _, fn in ways:
        fn(0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i in range(a.launches):
                fn(i % a.sets)
        graph.replay()
        graphs.append(graph)
    torch.cuda.synchronize()
    times = [[] for _ in ways]
    for rep in range(a.reps + 2):                    # two warm-up rounds, alternated afterwards
        for k, graph in enumerate(graphs):
            t = span(graph.replay) / a.launches * 1e3
            if rep >= 2:
                times[k].append(t)
    lines = [f"kernels: video latent [{ROWS}][{C}] fp32 (audio [{AROWS}][{C}] in the pair), per launch inside one captured graph of {a.launches} launches rotating over "
             f"{a.sets} operand sets, medians of {a.reps} (min - max)", "",
             "| launch | us | MB read + written | GB/s |", "|---|---|---|---|"]
    for (name, mbytes, _), t in zip(ways, times):
        med = statistics.median(t)
        lines.append(f"| {name} | {med:.2f} ({min(t):.2f} - {max(t):.2f}) | {mbytes:.2f} | {mbytes / med * 1e3:.0f} |")
    med = [statistics.median(t) for t in times]
    lines += ["", f"ancestral (guided) / guided_euler_step: {med[1] / med[0]:.3f};  ancestral / (fill + Euler + add as three launches): {med[1] / med[5]:.3f};  "
              f"pair: {med[7] / med[6]:.3f};  element-wise form: {med[9] / med[8]:.3f}", ""]
    return lines


def loop_table(a, dev):
    m = LTXModel(num_layers=a.layers, device=dev)
    m.init_random_weights(seed=0)
    g = torch.Generator(device=dev).manual_seed(3)
    vs = VideoLatentTools(VideoLatentPatchifier(1), VideoLatentShape(1, 128, 9, 16, 24), fps=25.0).create_initial_state(device=dev)
    n = vs.latent.shape[1]
    ctx = 0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev)
    m.prepare(ctx, vs.positions)
    sig = [float(s) for s in DISTILLED_SIGMA_VALUES]
    steps = len(sig) - 1
    st = [EulerAncestralDiffusionStep._get_ancestral_step(sig[i], sig[i + 1], 1.0) for i in range(steps)]
    up, down = [s[0] for s in st], [s[1] for s in st]
    word = K.seed_word(42, dev)
    start = torch.randn(n, 128, generator=g, device=dev)
    lat = {k: start.clone() for k in ("euler", "ancestral", "euler graph", "ancestral graph")}
    vm = lambda s: modality_from_state(vs, ctx, s, uniform=True)      # noqa: E731

    def euler():
        for i in range(steps):
            m.denoise_step_(lat["euler"], vm(sig[i]), sig[i], sig[i + 1])

    def ancestral():
        for i in range(steps):
            m.ancestral_step_(None, lat["ancestral"], vm(sig[i]), sig[i], up[i], down[i], word, i)

    twin = m.clone_sharing_weights()                 # a context holds one graph: the second loop is captured on a second context over the same weights
    twin.prepare(ctx, vs.positions)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        m.capture_denoise_graph(lat["euler graph"], sig)
        twin.capture_ancestral_graph(None, lat["ancestral graph"], sig, up, down, word)
    side.synchronize()
    ways = {"Euler loop, one C call per step (denoise_step_)": euler, "ancestral loop, one C call per step (ancestral_step_)": ancestral,
            "Euler loop, one graph replay": m.replay_denoise_graph, "ancestral loop, one graph replay": twin.replay_ancestral_graph}
    times = {k: [] for k in ways}
    for rep in range(a.reps + 2):
        for name, fn in ways.items():
            for t in lat.values():
                t.copy_(start)
            ms = span(fn) / steps
            if rep >= 2:
                times[name].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    k = list(ways)
    lines = [f"loops: video-only DiT, N = {n} tokens, S = 1024, {a.layers} layers, bf16, unguided, the {steps} distilled steps, eta = 1; ms per step, medians of {a.reps} (min - max)",
             "", "| loop | ms / step |", "|---|---|"]
    lines += [f"| {name} | {med[name]:.3f} ({min(times[name]):.3f} - {max(times[name]):.3f}) |" for name in ways]
    lines += ["", f"ancestral / Euler, per-call: {med[k[1]] / med[k[0]]:.4f};  captured: {med[k[3]] / med[k[2]]:.4f}", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--launches", type=int, default=192)
    ap.add_argument("--sets", type=int, default=24)
    ap.add_argument("--skip-loops", action="store_true")
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = kernel_table(a, dev) + ([] if a.skip_loops else loop_table(a, dev))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
