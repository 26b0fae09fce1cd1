"""The LTX-2.3 (V2) text path on one MI355X, Gemma resident: (1) `ltx2_gemma_features_rms` against the operand build it replaces
(49 `ltx2_adaln_rmsnorm` launches + 49 strided slice copies + where / zeros_like) at T = 128 and T = 1024, alternated in one process;
(2) the whole per-prompt path -- features, two projections at K = 188 160, two 8-block connectors -- as wall time around a
synchronise.  Random weights at the LTX-2.3 sizes.

    python tools/text_encoder_v2_time.py [--kernels-only] [--json OUT]

`--kernels-only` runs just the two operand builds (a short run to put under `rocprofv3 --kernel-trace --stats -- python ...`)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ltx_2_mlx_amd.kernels as K  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
D, L = 3840, 49
HBM_COPY_TBS = 6.29           # float4 copy rate measured on the MI355X (79 % of the 8 TB/s spec)


def median_us(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return statistics.median(ts)


def old_operand(states, valid):
    """The operand build before ltx2_gemma_features_rms (GemmaFeaturesExtractorV2.extract_from_hidden_states of the parent commit)."""
    t, d = states[0].shape
    a = torch.empty(t, L * d, device=DEV, dtype=BF16)
    for l, hs in enumerate(states):
        a[:, l * d:(l + 1) * d] = K.adaln_rmsnorm(hs, 1e-6)
    return torch.where(valid, a, torch.zeros_like(a))


def kernels(res):
    for t in (128, 1024):
        hidden = torch.randn(L, t, D, device=DEV)
        states = list(hidden.unbind(0))
        mask = torch.ones(t, device=DEV, dtype=torch.int32)
        valid = mask.bool().reshape(t, 1)
        out = torch.empty(t, L * D, device=DEV, dtype=BF16)
        differ = int((K.gemma_features_rms(states, mask, out=out).view(torch.int16) != old_operand(states, valid).view(torch.int16)).sum())
        print(f"T = {t:4d}: {differ} of {out.numel()} elements differ from the old build (another summation order: last-bit only)")
        new, old = [], []
        for _ in range(3):                   # alternate the two builds
            new.append(median_us(lambda: K.gemma_features_rms(states, mask, out=out)))
            old.append(median_us(lambda: old_operand(states, valid)))
        new_us, old_us = statistics.median(new), statistics.median(old)
        nbytes = t * L * D * (4 + 2)         # every fp32 element read once, every 16-bit element written once
        tbs = nbytes / (new_us * 1e-6) / 1e12
        res[f"features_rms_T{t}"] = dict(new_us=new_us, old_us=old_us, new_runs=new, old_runs=old, bytes=nbytes, tb_per_s=tbs,
                                         share_of_copy_rate=tbs / HBM_COPY_TBS)
        print(f"T = {t:4d}: ltx2_gemma_features_rms {new_us:8.1f} us ({nbytes / 1e6:6.1f} MB, {tbs:.2f} TB/s = {tbs / HBM_COPY_TBS:.0%} of the "
              f"{HBM_COPY_TBS} TB/s copy rate) | 49 norms + copies + where {old_us:8.1f} us | x{old_us / new_us:.1f}")


def whole_path(res):
    from ltx_2_mlx_amd.model.text_encoder import create_av_text_encoder_v2
    enc = create_av_text_encoder_v2(double_precision_rope=True, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    k = D * L
    enc.feature_extractor.load_state_dict({
        "video_aggregate_embed.weight": torch.randn(4096, k, generator=g, device=DEV) / math.sqrt(k),
        "video_aggregate_embed.bias": torch.zeros(4096, device=DEV),
        "audio_aggregate_embed.weight": torch.randn(2048, k, generator=g, device=DEV) / math.sqrt(k),
        "audio_aggregate_embed.bias": torch.zeros(2048, device=DEV)})
    enc.embeddings_connector.init_random_weights(1)
    enc.audio_embeddings_connector.init_random_weights(2)
    for t in (128, 1024):
        hidden = torch.randn(1, L, t, D, device=DEV)
        states = [hidden[:, l] for l in range(L)]
        mask = torch.ones(1, t, device=DEV)
        parts = {}
        fe = enc.feature_extractor
        parts["features + 2 projections"] = median_us(lambda: fe.extract_from_hidden_states(states, mask), n=10, warm=2)
        v, a = fe.extract_from_hidden_states(states, mask)
        parts["video connector (8 blocks, 32 x 128)"] = median_us(lambda: enc.embeddings_connector(v), n=10, warm=2)
        parts["audio connector (8 blocks, 32 x 64)"] = median_us(lambda: enc.audio_embeddings_connector(a), n=10, warm=2)
        walls = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc.encode_from_hidden_states(states, mask)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        wall = statistics.median(walls[2:])
        res[f"whole_path_T{t}"] = dict(wall_ms=wall, walls_ms=walls, parts_us=parts)
        print(f"T = {t:4d}: whole V2 text path (encode_from_hidden_states, host included) {wall:.2f} ms; "
              + "; ".join(f"{n} {u / 1e3:.2f} ms" for n, u in parts.items()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    res = {}
    kernels(res)
    if not args.kernels_only:
        whole_path(res)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
