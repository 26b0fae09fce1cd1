#!/usr/bin/env python
"""LTX-2 generation CLI on MI355X for the distilled denoise + VAE-decode hot path.

Keeps the flag names and `generate_video(...)` keyword names of the reference's
scripts/generate.py (argparse block :2364-2641, `generate_video` :933-997) for this path:
standard single-stage distilled loop (reference :1764-1984) followed by `decode_latent` (:2080-2091).
Gemma-3 encodes the prompt on the GPU when `--gemma-path` holds its weights (model/text_encoder/gemma3.py; reference
encode_with_gemma :340-486, encode_av_gemma_batch :511-640; an LTX-2.3 checkpoint gets the V2 text encoder, create_av_text_encoder_v2_from_checkpoint
:548-551).  `--stg-scale S [--stg-blocks ... --stg-cutoff F]` adds spatio-temporal guidance on the av route (OneStagePipeline), `--stg-audio-scale S` an STG term on the audio latent too (plain CFG or none);
`--sampler heun` and `--ge-gamma G` run its Heun loop and its GE velocity correction there.  Out of this path (and rejected
with a clear message): STG guidance, Heun and GE on every other route and Heun / GE beside STG, CFG in the video-only loop, the dev model's `--pipeline two-stage`.
`generate_video` resolves its arguments once (`_resolve_request`: every refusal, before a model is loaded), loads the text encoding, the transformer and the VAE decoder, and
runs ONE route, each a function of its own: two_stage_cfg (`--two-stage-cfg --spatial-upscaler-weights W`: TwoStagePipeline, CFG + modality-isolated guidance on the AudioVideo model), hq_av (`--ti2vid-hq-audio --spatial-upscaler-weights W`: TI2VidHQPipeline with sound, the joint res_2s loop on the AudioVideo model), a2vid (`--a2vid-two-stage --audio FILE --spatial-upscaler-weights W`: the two-stage audio-to-video pipeline), retake (`--retake CLIP`), keyframe (`--pipeline keyframe-interpolation --keyframe path:frame[:strength]`), hq (`--ti2vid-hq`), ic_lora
(`--pipeline ic-lora --control-video V` and / or `--image`), two_stage (`--two-stage-distilled --spatial-upscaler-weights W`; with `--generate-audio` on the AudioVideo transformer), av
(`--generate-audio` or an LTX-2.3 checkpoint: the audio LATENT is saved beside the frames; `--decode-audio`, the default when the checkpoint holds the audio VAE decoder and vocoder, also
decodes it to `<output>.wav` and muxes it into the mp4, reference save_video_with_audio; `--audio FILE` generates the video TO that audio: the audio VAE encoder's latent stays frozen in
the joint loop, and the original audio is muxed into the mp4) and standard (everything else: the video-only loop, then `--upscale-spatial` / `--upscale-temporal`).
`save_video` keeps the reference's ffmpeg settings (frames piped as raw RGB; PNG frames when no ffmpeg binary exists).  `--lora` fuses an adapter into the checkpoint weights at load.  `--image` conditions latent frame 0 on an image through the VAE encoder (the reference
routes that through its pipelines, scripts/generate.py:1711-1731).  Without Gemma weights, text embeddings come from `--embedding file.npz` (keys
`embedding`, `attention_mask`, as the reference's `load_text_embedding` :730-750) or the reference's
dummy encoder (`--no-gemma`, :642-661).  Frames are written as `<output>.npz` (uint8 T,H,W,3) and
the final latent as `<output>_latent.npz` like the reference (:1994-1996).
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ltx_2_mlx_amd.components import DISTILLED_SIGMA_VALUES, VideoLatentPatchifier, get_pixel_coords, get_sigma_schedule  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, Modality, X0Model  # noqa: E402
from ltx_2_mlx_amd.model.video_vae import SimpleVideoDecoder, TilingConfig, load_vae_decoder_weights  # noqa: E402
from ltx_2_mlx_amd.model.video_vae_encoder import SimpleVideoEncoder, load_vae_encoder_weights  # noqa: E402
from ltx_2_mlx_amd.pipelines.a2vid_two_stage import encode_audio_file, fit_audio_latent  # noqa: E402,F401
from ltx_2_mlx_amd.types import SpatioTemporalScaleFactors, VideoLatentShape  # noqa: E402


def write_wav(path: str, waveform, sample_rate: int) -> str:
    """waveform (B, 2, samples) or (2, samples) float in [-1, 1] -> 16-bit stereo PCM WAV of the first batch item, with the reference's
    scaling (x 32767, clipped) and interleave (save_video_with_audio, :2270-2288)."""
    import wave
    a = waveform.float().cpu().numpy() if isinstance(waveform, torch.Tensor) else np.asarray(waveform, dtype=np.float32)
    a = a[0] if a.ndim == 3 else a
    pcm = (a * 32767).clip(-32768, 32767).astype(np.int16).T.flatten()
    with wave.open(path, "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(pcm.tobytes())
    return path


def audio_filters(speed: float = 1.0):
    """The reference's atempo chain for a speed change (each stage within [0.5, 2.0], :2309-2320)."""
    out, rem = [], speed
    if speed != 1.0:
        while rem > 2.0:
            out.append("atempo=2.0")
            rem /= 2.0
        while rem < 0.5:
            out.append("atempo=0.5")
            rem /= 0.5
        if rem != 1.0:
            out.append(f"atempo={rem}")
    return out


def ffmpeg_av_command(width: int, height: int, wav_path: str, sample_rate: int, output_path: str, fps: int = 24, speed: float = 1.0, input_fps=None):
    """The reference's audio mux settings (:2323-2355: libx264 crf 18, aac 320k at the vocoder's rate, -shortest); the frames arrive as
    raw RGB on stdin.  input_fps: the rate the frames are played at (a retake source's own; None: the native 24 fps)."""
    input_fps = NATIVE_FPS if input_fps is None else input_fps
    cmd = ["ffmpeg", "-y", "-f", "rawvideo", "-pix_fmt", "rgb24", "-s", f"{width}x{height}", "-framerate", f"{input_fps:g}", "-i", "-",
           "-i", wav_path]
    if video_filters(fps, speed, input_fps):
        cmd += ["-vf", ",".join(video_filters(fps, speed, input_fps))]
    if audio_filters(speed):
        cmd += ["-af", ",".join(audio_filters(speed))]
    return cmd + ["-c:v", "libx264", "-c:a", "aac", "-b:a", "320k", "-ar", str(sample_rate), "-pix_fmt", "yuv420p", "-crf", "18", "-shortest",
                  "-loglevel", "error", output_path]


def save_video_with_audio(frames, audio_waveform, output_path: str, audio_sample_rate: int, fps: int = 24, speed: float = 1.0, input_fps=None):
    """Writes `<output stem>.wav` (the reference's sidecar) and muxes it into output_path with ffmpeg; without an ffmpeg binary the
    frames go to PNGs as in save_video and the .wav stays beside them.  Returns (video path or frames dir, wav path)."""
    import shutil
    import subprocess
    wav_path = write_wav(os.path.splitext(output_path)[0] + ".wav", audio_waveform, audio_sample_rate)
    n = (audio_waveform.shape[-1])
    print(f"    Sidecar WAV: {wav_path} ({n} samples, {n / audio_sample_rate:.2f} s at {audio_sample_rate} Hz)")
    if shutil.which("ffmpeg") is None:
        return save_video(frames, output_path, fps=fps, speed=speed, **({} if input_fps is None else dict(input_fps=input_fps))), wav_path
    frames = np.ascontiguousarray(np.asarray(frames))
    t, h, w, _ = frames.shape
    result = subprocess.run(ffmpeg_av_command(w, h, wav_path, audio_sample_rate, output_path, fps, speed, input_fps), input=frames.tobytes(), capture_output=True)
    if result.returncode != 0:
        raise RuntimeError(f"FFmpeg failed: {result.stderr.decode(errors='replace')}")
    return output_path, wav_path


def create_dummy_text_encoding(prompt: str, batch_size: int = 1, max_tokens: int = 256, embed_dim: int = 3840, device="cuda"):
    """0.1 * N(0,1) embedding seeded by the prompt (reference :642-661; torch RNG instead of MLX's)."""
    g = torch.Generator().manual_seed(hash(prompt) % (2 ** 31))
    return (0.1 * torch.randn(batch_size, max_tokens, embed_dim, generator=g)).to(device), torch.ones(batch_size, max_tokens, device=device)


NATIVE_FPS = 24     # the model generates motion at 24 fps


def video_filters(fps=24, speed: float = 1.0, input_fps=NATIVE_FPS):
    """ffmpeg -vf chain of the reference's save_video (scripts/generate.py:2178-2194): speed first (setpts), then
    motion-compensated interpolation when the target frame rate exceeds the rate the frames arrive at (the native 24 fps, or a retake
    source's own rate)."""
    filters = []
    if speed != 1.0:
        filters.append(f"setpts={1.0 / speed}*PTS")
    if fps > input_fps:
        filters.append(f"minterpolate=fps={fps}:mi_mode=mci:mc_mode=aobmc:me_mode=bidir:vsbmc=1")
    return filters


def ffmpeg_command(width: int, height: int, output_path: str, fps=24, speed: float = 1.0, input_fps=NATIVE_FPS):
    """Same encoder settings as the reference (:2201-2222: libx264, yuv420p, crf 18, input at the native 24 fps); the
    frames arrive as raw RGB on stdin instead of a directory of PNGs.  input_fps: the rate the frames are played at (a retake source's own)."""
    cmd = ["ffmpeg", "-y", "-f", "rawvideo", "-pix_fmt", "rgb24", "-s", f"{width}x{height}", "-framerate", f"{input_fps:g}", "-i", "-"]
    filters = video_filters(fps, speed, input_fps)
    if filters:
        cmd += ["-vf", ",".join(filters)]
    return cmd + ["-c:v", "libx264", "-pix_fmt", "yuv420p", "-crf", "18", "-loglevel", "error", output_path]


def save_video(frames, output_path: str, fps=24, speed: float = 1.0, input_fps=NATIVE_FPS):
    """frames: uint8 (T, H, W, 3) array or list of (H, W, 3) arrays -> output_path via ffmpeg (reference :2153-2226).
    Without an ffmpeg binary the frames are written as PNGs into `<output stem>_frames/` and that directory is returned
    (the reference raises there; on a GPU box without ffmpeg the frames are still wanted)."""
    import shutil
    import subprocess
    frames = np.ascontiguousarray(np.stack([np.asarray(f) for f in frames]) if isinstance(frames, (list, tuple)) else np.asarray(frames))
    if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype != np.uint8:
        raise ValueError(f"save_video expects uint8 frames (T, H, W, 3), got {frames.dtype} {frames.shape}")
    t, h, w, _ = frames.shape
    if shutil.which("ffmpeg") is None:
        from PIL import Image
        out_dir = os.path.splitext(output_path)[0] + "_frames"
        os.makedirs(out_dir, exist_ok=True)
        for i in range(t):
            Image.fromarray(frames[i]).save(os.path.join(out_dir, f"frame_{i:04d}.png"))
        print(f"  ffmpeg not found: wrote {t} PNG frames to {out_dir}/")
        return out_dir
    result = subprocess.run(ffmpeg_command(w, h, output_path, fps, speed, input_fps), input=frames.tobytes(), capture_output=True)
    if result.returncode != 0:
        raise RuntimeError(f"FFmpeg failed: {result.stderr.decode(errors='replace')}")
    return output_path


def encode_text_features(path: str, weights_path=None, device="cuda", seed: int = 0):
    """`--text-features file.npz`: key `features` = the Gemma feature extractor's output [T, 3840] or [1, T, 3840]
    (or `hidden_states` [L, T, 3840] = all Gemma layers, run through the extractor first) and `attention_mask` [T].
    The Embeddings1DConnector (registers, 2 blocks, final RMSNorm) runs on the GPU (reference `encode_projected` /
    `encode_from_hidden_states`, model/text_encoder/encoder.py:136-215); its weights come from `--weights`
    (`model.diffusion_model.video_embeddings_connector.*`, `text_embedding_projection.*`) or are random without one."""
    from ltx_2_mlx_amd.model.text_encoder import create_text_encoder, load_text_encoder_weights
    z = np.load(path)
    enc = create_text_encoder(device=device)
    if weights_path:
        load_text_encoder_weights(enc, weights_path)
    else:
        enc.embeddings_connector.init_random_weights(seed)
    mask = torch.from_numpy(z["attention_mask"]).float().reshape(1, -1) if "attention_mask" in z else None
    if "hidden_states" in z:
        hs = [torch.from_numpy(h).float()[None] for h in z["hidden_states"]]
        mask = torch.ones(1, hs[0].shape[1]) if mask is None else mask
        out = enc.encode_from_hidden_states(hs, mask.to(device))
    else:
        feats = torch.from_numpy(z["features"]).float()
        feats = feats[None] if feats.dim() == 2 else feats
        mask = torch.ones(feats.shape[:2]) if mask is None else mask
        out = enc.encode_projected(feats.to(device), mask.to(device))
    return out.video_encoding, out.attention_mask.float()


def _gemma_text_encoder(gemma_cfg, ltx_weights_path, device, seed: int = 0, audio_video: bool = False, model_version=None, num_heads: int = 32):
    """Feature extractor + connector(s) for a Gemma of `gemma_cfg`: from the LTX checkpoint when given (its text_embedding_projection must
    take (hidden, layers + 1) hidden states: raises naming both shapes otherwise), else randomly initialised at that size.  An LTX-2.3
    checkpoint (`is_v2_model`; `model_version` overrides the metadata, as in generate_video), or `model_version` 2.3 without a checkpoint,
    gets the V2 encoder (create_av_text_encoder_v2: per-token RMS
    extractor to the transformer's widths num_heads * 128 / num_heads * 64, 8-block gated connectors)."""
    import math
    from ltx_2_mlx_amd.model.text_encoder import (AudioVideoGemmaTextEncoderModel, Embeddings1DConnector, GemmaFeaturesExtractorProjLinear,
                                                  VideoGemmaTextEncoderModel, create_av_text_encoder_v2,
                                                  create_av_text_encoder_v2_from_checkpoint, load_av_text_encoder_v2_weights,
                                                  load_text_encoder_weights)
    hidden, nl = gemma_cfg.hidden_size, gemma_cfg.num_hidden_layers + 1
    if model_version is None:
        model_version = detect_model_version(ltx_weights_path) if ltx_weights_path else ""
    if str(model_version).startswith("2.3"):
        if not ltx_weights_path:
            video_dim, audio_dim = num_heads * 128, num_heads * 64
            enc = create_av_text_encoder_v2(hidden_dim=hidden, num_gemma_layers=nl, video_inner_dim=video_dim, audio_inner_dim=audio_dim,
                                            video_connector_heads=num_heads, audio_connector_heads=num_heads, device=device)
            g = torch.Generator().manual_seed(seed)
            enc.feature_extractor.load_state_dict({
                "video_aggregate_embed.weight": torch.randn(video_dim, hidden * nl, generator=g) / math.sqrt(hidden * nl),
                "video_aggregate_embed.bias": 0.02 * torch.randn(video_dim, generator=g),
                "audio_aggregate_embed.weight": torch.randn(audio_dim, hidden * nl, generator=g) / math.sqrt(hidden * nl),
                "audio_aggregate_embed.bias": 0.02 * torch.randn(audio_dim, generator=g)})
            enc.embeddings_connector.init_random_weights(seed + 1)
            enc.audio_embeddings_connector.init_random_weights(seed + 2)
            return enc
        from safetensors import safe_open
        dims = {}
        with safe_open(ltx_weights_path, framework="pt") as f:
            for name in ("video_aggregate_embed", "audio_aggregate_embed"):
                key = f"text_embedding_projection.{name}.weight"
                if key not in f.keys():
                    raise KeyError(f"{key} is not in the LTX-2.3 checkpoint {ltx_weights_path}")
                have = tuple(f.get_slice(key).get_shape())
                if have[1] != hidden * nl:
                    raise ValueError(f"the Gemma at hand gives (hidden, layers + 1) = {(hidden, nl)}, i.e. a {key} of "
                                     f"{(have[0], hidden * nl)}, but the LTX checkpoint's is {have}")
                dims[name] = have[0]
        enc = create_av_text_encoder_v2_from_checkpoint(ltx_weights_path, hidden_dim=hidden, num_gemma_layers=nl,
                                                        video_inner_dim=dims["video_aggregate_embed"],
                                                        audio_inner_dim=dims["audio_aggregate_embed"], device=device)
        load_av_text_encoder_v2_weights(enc, ltx_weights_path)
        return enc
    fe = GemmaFeaturesExtractorProjLinear(hidden_dim=hidden, num_layers=nl, device=device)
    conns = [Embeddings1DConnector(device=device) for _ in range(2 if audio_video else 1)]
    enc = AudioVideoGemmaTextEncoderModel(fe, conns[0], conns[1]) if audio_video else VideoGemmaTextEncoderModel(fe, conns[0])
    if ltx_weights_path:
        from safetensors import safe_open
        with safe_open(ltx_weights_path, framework="pt") as f:
            key = "text_embedding_projection.aggregate_embed.weight"
            have = tuple(f.get_slice(key).get_shape()) if key in f.keys() else None
        if have is not None and have != (hidden, hidden * nl):
            raise ValueError(f"the Gemma at hand gives (hidden, layers + 1) = {(hidden, nl)}, i.e. a text_embedding_projection of "
                             f"{(hidden, hidden * nl)}, but the LTX checkpoint's is {have}")
        load_text_encoder_weights(enc, ltx_weights_path)
    else:
        g = torch.Generator().manual_seed(seed)
        fe.load_state_dict({"aggregate_embed.weight": torch.randn(hidden, hidden * nl, generator=g) / math.sqrt(hidden * nl)})
        for i, c in enumerate(conns):
            c.init_random_weights(seed + 1 + i)
    return enc


def _load_gemma(gemma_path: str, device):
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import create_gemma3_model, load_gemma_tokenizer
    print(f"  Loading tokenizer from {gemma_path}...")
    tokenizer = load_gemma_tokenizer(gemma_path)
    print("  Loading Gemma 3 model (bfloat16 operands, fp32 residual stream)...")
    t0 = time.time()
    gemma = create_gemma3_model(gemma_path, device=device)
    torch.cuda.synchronize()
    print(f"  Gemma 3: {gemma.config.num_hidden_layers} layers x {gemma.config.hidden_size} loaded in {time.time() - t0:.1f} s")
    return tokenizer, gemma


def _gemma_hidden_states(gemma, tokenizer, prompt: str, max_length: int, device):
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import tokenize_prompt
    ids, mask = tokenize_prompt(tokenizer, prompt, max_length)       # raw prompt, left padding, truncation (reference :384-393)
    num_tokens = int(mask.sum())
    if num_tokens == 0:
        raise ValueError(f"prompt {prompt!r} gives no tokens")
    print(f"  Token count: {num_tokens}/{max_length}")
    _, states = gemma(torch.from_numpy(ids), attention_mask=torch.from_numpy(mask))
    return states, torch.from_numpy(mask).to(device)


def _free_gemma(gemma):
    """Free Gemma before the DiT loads (reference :631-640)."""
    gemma.free()
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def encode_with_gemma(prompt: str, gemma_path: str, ltx_weights_path, max_length: int = 1024, use_early_layers_only: bool = False, *,
                      device="cuda", seed: int = 0):
    """Gemma 3 + the LTX-2 text encoder (feature extractor + connector) for one prompt (reference scripts/generate.py:340-486).
    Returns (embedding [1, T', 3840], attention_mask [1, T']).  Without `ltx_weights_path` (keyword-compatible None) the text encoder is
    randomly initialised at the Gemma's size."""
    tokenizer, gemma = _load_gemma(gemma_path, device)
    try:
        print("  Running Gemma 3 forward pass...")
        states, mask = _gemma_hidden_states(gemma, tokenizer, prompt, max_length, device)
        if use_early_layers_only:                   # reference :437-451: layer 0 (the scaled embeddings), padding zeroed
            return states[0] * mask[:, :, None].float(), mask.to(torch.int32)
        enc = _gemma_text_encoder(gemma.config, ltx_weights_path, device, seed)
        out = enc.encode_from_hidden_states(states, mask, padding_side="left")
        return out.video_encoding, out.attention_mask
    finally:
        _free_gemma(gemma)


def encode_av_gemma_batch(prompts: list, gemma_path: str, ltx_weights_path, max_length: int = 1024, *, device="cuda", seed: int = 0,
                          model_version=None, num_heads: int = 32) -> list:
    """Several prompts under ONE Gemma load with the AudioVideo text encoder (reference scripts/generate.py:511-640): the hidden states are
    trimmed to the real tokens, later prompts are tokenised with max_length = the first encoding's length.  An LTX-2.3 checkpoint (or
    model_version 2.3 without a checkpoint, at num_heads) gets the V2 encoder (reference :548-551).  Returns
    [(video_encoding, audio_encoding, attention_mask), ...]."""
    tokenizer, gemma = _load_gemma(gemma_path, device)
    try:
        enc = _gemma_text_encoder(gemma.config, ltx_weights_path, device, seed, audio_video=True, model_version=model_version,
                                  num_heads=num_heads)
        results = []
        for i, prompt in enumerate(prompts):
            print(f"  Running Gemma 3 forward pass (prompt {i + 1}/{len(prompts)})...")
            states, mask = _gemma_hidden_states(gemma, tokenizer, prompt, max_length, device)
            n, t = int(mask.sum()), mask.shape[1]
            if n < t:                               # left padding: the real tokens are the last n (reference :587-595)
                states = [h[:, -n:] for h in states]
                mask = mask[:, -n:]
            out = enc.encode_from_hidden_states(states, mask, padding_side="left")
            results.append((out.video_encoding, out.audio_encoding, out.attention_mask))
            del states
            if i == 0:
                max_length = out.video_encoding.shape[1]
        return results
    finally:
        _free_gemma(gemma)


def _read_checkpoint_config(checkpoint_path: str) -> dict:
    """The JSON `config` entry of the safetensors metadata (reference scripts/generate.py:142-152); {} when absent / unreadable."""
    import json
    try:
        from safetensors import safe_open
        with safe_open(checkpoint_path, framework="pt") as f:
            metadata = f.metadata() or {}
        return json.loads(metadata.get("config", "{}"))
    except Exception:
        return {}


def create_vocoder_for_checkpoint(checkpoint_path, compute_dtype=torch.float32, device="cuda") -> tuple:
    """The plain HiFi-GAN Vocoder (LTX-2.0: no `bwe` in the metadata's vocoder config) or VocoderWithBWE (LTX-2.3), configured from
    the checkpoint metadata as the reference's create_vocoder_for_checkpoint (:155-221).  Returns (vocoder, is_bwe)."""
    from ltx_2_mlx_amd.model.audio_vae import MelSTFT, Vocoder, VocoderWithBWE
    config = _read_checkpoint_config(checkpoint_path) if checkpoint_path and os.path.exists(checkpoint_path) else {}
    vocoder_cfg = config.get("vocoder", {})
    if "bwe" not in vocoder_cfg:
        return Vocoder(compute_dtype=compute_dtype, device=device), False
    inner_cfg = vocoder_cfg.get("vocoder", {})
    bwe_cfg = vocoder_cfg["bwe"]
    inner = Vocoder(
        resblock_kernel_sizes=inner_cfg.get("resblock_kernel_sizes", [3, 7, 11]),
        upsample_rates=inner_cfg.get("upsample_rates", [6, 5, 2, 2, 2]),
        upsample_kernel_sizes=inner_cfg.get("upsample_kernel_sizes", [16, 15, 8, 4, 4]),
        resblock_dilation_sizes=inner_cfg.get("resblock_dilation_sizes", [[1, 3, 5], [1, 3, 5], [1, 3, 5]]),
        upsample_initial_channel=inner_cfg.get("upsample_initial_channel", 1024),
        resblock=inner_cfg.get("resblock", "AMP1"),
        output_sample_rate=bwe_cfg.get("input_sampling_rate", 24000),
        activation=inner_cfg.get("activation", "snakebeta"),
        use_tanh_at_final=inner_cfg.get("use_tanh_at_final", True),
        compute_dtype=compute_dtype, device=device)
    bwe = Vocoder(
        resblock_kernel_sizes=bwe_cfg.get("resblock_kernel_sizes", [3, 7, 11]),
        upsample_rates=bwe_cfg.get("upsample_rates", [2]),
        upsample_kernel_sizes=bwe_cfg.get("upsample_kernel_sizes", [4]),
        resblock_dilation_sizes=bwe_cfg.get("resblock_dilation_sizes", [[1, 3, 5], [1, 3, 5], [1, 3, 5]]),
        upsample_initial_channel=bwe_cfg.get("upsample_initial_channel", 256),
        resblock=bwe_cfg.get("resblock", "AMP1"),
        output_sample_rate=bwe_cfg.get("output_sampling_rate", 48000),
        activation=bwe_cfg.get("activation", "snakebeta"),
        apply_final_activation=False,
        use_tanh_at_final=bwe_cfg.get("use_tanh_at_final", True),
        compute_dtype=compute_dtype, device=device)
    mel_stft = MelSTFT(filter_length=bwe_cfg.get("n_fft", 2048), hop_length=bwe_cfg.get("hop_length", 240), win_length=bwe_cfg.get("n_fft", 2048),
                       n_mel_channels=bwe_cfg.get("num_mels", 128), device=device)
    return VocoderWithBWE(vocoder=inner, bwe_generator=bwe, mel_stft=mel_stft, input_sampling_rate=bwe_cfg.get("input_sampling_rate", 24000),
                          output_sampling_rate=bwe_cfg.get("output_sampling_rate", 48000), hop_length=bwe_cfg.get("hop_length", 240)), True


def checkpoint_has_audio_decoders(checkpoint_path) -> bool:
    """True when the checkpoint carries `audio_vae.decoder.*` and `vocoder.*` tensors."""
    if not checkpoint_path or not os.path.exists(checkpoint_path):
        return False
    from ltx_2_mlx_amd.loader.weight_converter import SafetensorsStream
    keys = SafetensorsStream(checkpoint_path, "cpu").keys()
    return any(k.startswith("audio_vae.decoder.") for k in keys) and any(k.startswith("vocoder.") for k in keys)


def create_audio_decoders(decode_audio, weights_path, device="cuda", seed=0):
    """(AudioDecoder, vocoder) for decode_audio: None decodes when the checkpoint holds the audio decoder and vocoder tensors (else None
    with a note), True always decodes (random-initialised decoders without those tensors), False never.  The vocoder form follows the
    checkpoint's metadata (create_vocoder_for_checkpoint); without a checkpoint that is the LTX-2.0 HiFi-GAN Vocoder (24 kHz) even when
    model_version selects the LTX-2.3 transformer: no metadata says what BWE configuration a random LTX-2.3 vocoder would have."""
    from ltx_2_mlx_amd.model.audio_vae import AudioDecoder, load_audio_decoder_weights, load_vocoder_weights, load_vocoder_with_bwe_weights
    if decode_audio is False:
        return None
    if checkpoint_has_audio_decoders(weights_path):
        dec = AudioDecoder(device=device)
        load_audio_decoder_weights(dec, weights_path)
        voc, is_bwe = create_vocoder_for_checkpoint(weights_path, device=device)
        (load_vocoder_with_bwe_weights if is_bwe else load_vocoder_weights)(voc, weights_path)
        return dec, voc
    if decode_audio is None:
        print("  note: no audio_vae.decoder.* / vocoder.* tensors in the checkpoint: the audio latent is kept (decode_audio=True / --decode-audio "
              "decodes with random-initialised decoders)")
        return None
    print("  Audio decoder + vocoder: random init (no checkpoint tensors; the vocoder form follows the checkpoint metadata, "
          "the LTX-2.0 HiFi-GAN Vocoder without one)")
    dec = AudioDecoder(device=device)
    dec.init_random_weights(seed)
    voc, is_bwe = create_vocoder_for_checkpoint(weights_path, device=device)
    for v in ((voc.vocoder, voc.bwe_generator) if is_bwe else (voc,)):
        v.init_random_weights(seed + 1)
    return dec, voc


def checkpoint_has_audio_encoder(checkpoint_path) -> bool:
    if not checkpoint_path or not os.path.exists(checkpoint_path):
        return False
    from ltx_2_mlx_amd.loader.weight_converter import SafetensorsStream
    with SafetensorsStream(checkpoint_path, "cpu") as st:
        return any(k.startswith("audio_vae.encoder.") for k in st.keys())


def create_audio_encoder(weights_path=None, device="cuda", seed=0):
    """The audio VAE encoder: weights from the checkpoint when it has `audio_vae.encoder.*`, random init otherwise."""
    from ltx_2_mlx_amd.model.audio_vae import AudioEncoder, load_audio_encoder_weights
    enc = AudioEncoder(device=device)
    if checkpoint_has_audio_encoder(weights_path):
        load_audio_encoder_weights(enc, weights_path)
    else:
        print("  note: no audio_vae.encoder.* tensors in the checkpoint: RANDOM audio encoder (test mode)")
        enc.init_random_weights(seed=seed)
    return enc


def encode_audio_for_video(audio_path, num_frames: int, fps: float, weights_path=None, device="cuda", seed=0, start_time: float = 0.0,
                           max_duration=None):
    """Audio file -> (frozen audio latent (1, 8, T_a, 16) for a num_frames / fps video, the fitted waveform [C, samples], its rate):
    create_audio_encoder, then pipelines.a2vid_two_stage.encode_audio_file (load_audio_file with the start / duration trim and the resample to
    16 kHz, cut or right-padded with silence to the video's length, AudioProcessor.waveform_to_mel, AudioEncoder)."""
    enc = create_audio_encoder(weights_path, device, seed)
    t0 = time.time()
    latent, waveform, sr = encode_audio_file(audio_path, num_frames, fps, enc, start_time=start_time, max_duration=max_duration)
    torch.cuda.synchronize()
    print(f"  audio encode: {(time.time() - t0):.3f} s -> {tuple(latent.shape)}")
    return latent, waveform, sr


def detect_model_version(checkpoint_path: str) -> str:
    """`model_version` of the safetensors metadata, e.g. "2.3.0"; "" if unknown (reference :224-236)."""
    try:
        from safetensors import safe_open
        with safe_open(checkpoint_path, framework="pt") as f:
            metadata = f.metadata() or {}
        return metadata.get("model_version", "")
    except Exception:
        return ""


def is_v2_model(checkpoint_path: str) -> bool:
    """LTX-2.3 ("V2") checkpoint? (reference :239-242)"""
    return detect_model_version(checkpoint_path).startswith("2.3")


def get_vae_config(checkpoint_path: str) -> dict:
    """`config.vae` of the checkpoint metadata: decoder_blocks / decoder_base_channels / timestep_conditioning (reference :245-254)."""
    return _read_checkpoint_config(checkpoint_path).get("vae", {})


def create_vae_decoder(weights_path, device="cuda", seed=0, use_placeholder=False, base_channels_override=None, compute_dtype=None):
    """SimpleVideoDecoder built from the checkpoint's own architecture record (reference :1255-1273): decoder_blocks,
    decoder_base_channels (128 when absent), timestep_conditioning (True when absent).  Without a readable checkpoint the
    default 19B decoder is built and random-initialised (no checkpoints exist on a bare box; the reference would run the
    uninitialised module)."""
    have = bool(weights_path) and os.path.exists(weights_path)
    vae_config = get_vae_config(weights_path) if have else {}
    decoder_blocks = vae_config.get("decoder_blocks", None)
    base_channels = vae_config.get("decoder_base_channels", 128) if base_channels_override is None else base_channels_override
    timestep_cond = vae_config.get("timestep_conditioning", True)
    if decoder_blocks:
        print(f"  VAE config: {len(decoder_blocks)} blocks, base_ch={base_channels}, timestep={timestep_cond}")
    dec = SimpleVideoDecoder(decoder_blocks=decoder_blocks, base_channels=base_channels, timestep_conditioning=timestep_cond, device=device,
                             **({} if compute_dtype is None else {"compute_dtype": compute_dtype}))
    if have and not use_placeholder:
        load_vae_decoder_weights(dec, weights_path)
    else:
        if weights_path and not have:
            print(f"  Warning: Weights not found at {weights_path}, using random init")
        dec.init_random_weights(seed=seed)
    return dec


def _dtype_of(compute_dtype):
    return torch.bfloat16 if compute_dtype is None else compute_dtype


def load_transformer(weights_path, num_layers: int = 48, compute_dtype=None, use_fp8: bool = False, low_memory: bool = False,
                     fast_mode: bool = False, *, num_heads: int = 32, caption_channels: int = 3840, seed: int = 0, device="cuda",
                     lora_path=None, lora_strength: float = 1.0, fp8_resident: bool = False, fp8_compute: bool = False):
    """LTXModel(VideoOnly, 32x128, caption 3840) with checkpoint weights (reference load_transformer :788-835; same leading
    parameters).  A missing checkpoint file means random init with the reference's warning.  low_memory / fast_mode have
    no effect here; keyword-only extras are MI355X additions.  fp8_compute (BASELINE config 3, "fp8 weights (CDNA4 fp8 MFMA)"):
    the video stream's projections run fp8 x fp8 on the fp8 MFMA -- an fp8 checkpoint's codes stay resident (as fp8_resident),
    a bf16 / fp16 checkpoint is quantised per output channel at load; activations are quantised per token inside the step.  Not
    bit-identical to the reference's dequantise-at-load (`use_fp8`), which stays the default (reference :2424-2436,
    loader/fp8_loader.py:54-130)."""
    model = LTXModel(num_attention_heads=num_heads, attention_head_dim=128, num_layers=num_layers, caption_channels=caption_channels,
                     compute_dtype=_dtype_of(compute_dtype), device=device, fp8_compute=fp8_compute)
    if weights_path and os.path.exists(weights_path):
        from ltx_2_mlx_amd.loader import LoRAConfig, is_fp8_checkpoint, load_transformer_weights
        fp8 = use_fp8 or is_fp8_checkpoint(weights_path)
        # LoRA fusion needs dequantised weights; with fp8_compute they are re-quantised per channel after the fuse (load_state_dict)
        load_transformer_weights(model, weights_path, strict=True, use_fp8=fp8, fp8_resident=(fp8_resident or fp8_compute) and fp8 and not lora_path,
                                 lora_configs=[LoRAConfig(lora_path, lora_strength)] if lora_path else None)
    elif lora_path:
        raise ValueError("--lora needs --weights (an adapter is fused into checkpoint weights)")
    else:
        if weights_path:
            print(f"  Warning: Weights not found at {weights_path}, using random init")
        model.init_random_weights(seed=seed)
    return model


def load_av_transformer(weights_path, num_layers: int = 48, compute_dtype=None, use_fp8: bool = False, low_memory: bool = False,
                        caption_channels=3840, cross_attention_adaln: bool = False, apply_gated_attention: bool = False, *,
                        num_heads: int = 32, seed: int = 0, device="cuda", lora_path=None, lora_strength: float = 1.0,
                        fp8_compute: bool = False):
    """AudioVideo LTXModel (video 32x128 + audio 32x64 heads) with checkpoint weights (reference load_av_transformer :838-902,
    same parameters): caption_channels = 3840 for LTX-2.0, None for LTX-2.3 (the feature extractor already projects to the
    transformer widths); cross_attention_adaln / apply_gated_attention = the LTX-2.3 block variant;
    av_ca_timestep_scale_multiplier = 1000 as the reference passes it.  lora_path / lora_strength (keyword-only): the adapter is fused
    into whichever transformer is loaded, as the reference does (:1186-1202, loader/lora_loader.py:129-195); fp8_compute: as load_transformer
    (the VIDEO stream's projections; the audio stream and the cross-modal attention stay on the 16-bit path)."""
    from ltx_2_mlx_amd.model.transformer import LTXModelType
    model = LTXModel(model_type=LTXModelType.AudioVideo, num_attention_heads=num_heads, attention_head_dim=128, num_layers=num_layers,
                     caption_channels=caption_channels, audio_attention_heads=num_heads, cross_attention_adaln=cross_attention_adaln,
                     apply_gated_attention=apply_gated_attention, av_ca_timestep_scale_multiplier=1000,
                     compute_dtype=_dtype_of(compute_dtype), device=device, fp8_compute=fp8_compute)
    if weights_path and os.path.exists(weights_path):
        from ltx_2_mlx_amd.loader import LoRAConfig, is_fp8_checkpoint, load_av_transformer_weights
        fp8 = use_fp8 or is_fp8_checkpoint(weights_path)
        load_av_transformer_weights(model, weights_path, strict=True, use_fp8=fp8, fp8_resident=fp8_compute and fp8 and not lora_path,
                                    lora_configs=[LoRAConfig(lora_path, lora_strength)] if lora_path else None)
    elif lora_path:
        raise ValueError("--lora needs --weights (an adapter is fused into checkpoint weights)")
    else:
        if weights_path:
            print(f"  Warning: Weights not found at {weights_path}, using random init")
        model.init_random_weights(seed=seed)
    return model


def euler_step_x0(sample, denoised, sigma, sigma_next):
    from ltx_2_mlx_amd import kernels as K
    c = sample.shape[-1]
    return K.euler_step(sample.reshape(-1, c).float(), denoised.reshape(-1, c).float(), sigma, sigma_next).reshape(sample.shape)


# Keyword surface of the reference's generate_video (scripts/generate.py:933-997), names and defaults verbatim, so a caller of
# the reference can switch without touching its call site.  Options outside the MI355X hot path are accepted at their
# reference defaults and raise NotImplementedError only when set to something else.
_OUT_OF_PATH_DEFAULTS = dict(
    early_layers_only=False, enhance_prompt_flag=False,
    cross_attn_scale=1.0, distilled_lora=None, stg_scale=0.0, apg_scale=1.0, control_video=None, save_control=False,
    ge_gamma=0.0, keyframes=None, ic_lora_weights=None, negative_prompt=None, stg_audio_scale=0.0)
# pipelines whose algorithm is not built: "two-stage" is the dev model's CFG stage 1 + distilled-LoRA stage 2 (TwoStageCFGConfig,
# reference :1276-1431).  "keyframe-interpolation" (:1552-1637) is built, but only WITH keyframes, and "ic-lora" (:1434-1549) only WITH a
# control video and / or an image: without them they are refused like "two-stage" (the reference raises ValueError there)
_PIPELINES_BUILT = ("text-to-video", "distilled", "one-stage")
_PIPELINES_CLI = _PIPELINES_BUILT + ("two-stage", "ic-lora", "keyframe-interpolation")      # the reference parser's --pipeline choices, verbatim
# "ti2vid-hq" is an addition: the reference has pipelines/ti2vid_hq.py (res_2s second-order sampler, 15 steps) but its own generate.py never
# reaches it.  Here pipeline_type="ti2vid-hq" (--ti2vid-hq on the command line) runs TI2VidHQPipeline.
_PIPELINES_KNOWN = _PIPELINES_CLI + ("ti2vid-hq",)


def parse_keyframe(spec):
    """'path:frame_index[:strength]' (one --keyframe argument) -> Keyframe; a Keyframe passes through (reference :1558-1568)."""
    from ltx_2_mlx_amd.pipelines import Keyframe
    if isinstance(spec, Keyframe):
        return spec
    parts = str(spec).split(":")
    if len(parts) < 2:
        raise ValueError(f"Invalid keyframe format: {spec}. Use 'path:frame_index' or 'path:frame_index:strength'")
    return Keyframe(image_path=parts[0], frame_index=int(parts[1]), strength=float(parts[2]) if len(parts) > 2 else 0.95)


def _frames_from_video(video):
    """Pipeline output -> uint8 (T, H, W, 3): decode_latent already returns that; decode_tiled returns float (1, 3, T, H, W) in
    [-1, 1] (reference :1744-1755 converts it the same way)."""
    if video.dtype == torch.uint8:
        return video
    from ltx_2_mlx_amd import kernels as K
    return K.video_to_uint8(video[0] if video.dim() == 5 else video)


def _batched(t):
    """An encoding stored without its batch axis gets one."""
    return t[None] if t.dim() == 2 else t


# ---- request resolution: everything generate_video decides before a model is loaded ----

# route -> (the arguments it is not combined with, in the order they are refused; the tail of the refusal)
_ROUTE_EXCLUDES = {
    "retake": (("generate_audio", "audio_path", "keyframes", "control_video", "image_path", "two_stage_distilled", "upscale_spatial",
                "upscale_temporal", "fp8_resident", "pipeline_type"),
               "with retake_video: RetakePipeline is video-only, conditions on its source clip alone and runs one stage at the source's own "
               "size on dequantised weights"),
    "retake_av": (("audio_path", "keyframes", "control_video", "image_path", "two_stage_distilled", "upscale_spatial", "upscale_temporal", "fp8_resident",
                   "pipeline_type"),
                  "with retake_video and retake_audio: RetakePipeline conditions on its source clip and sound track alone and runs one stage at the "
                  "source's own size on dequantised weights"),
    "keyframe": (("generate_audio", "audio_path", "two_stage_distilled", "upscale_temporal", "image_path"),
                 "with keyframes: the keyframe interpolation pipeline is video-only, conditions on its keyframes alone and ends with its own "
                 "x2 spatial stage"),
    "hq": (("generate_audio", "audio_path", "two_stage_distilled", "upscale_temporal", "keyframes"),
           "with pipeline_type='ti2vid-hq': TI2VidHQPipeline is video-only (the joint audio branch of the res_2s loop is not built), "
           "conditions on image_path alone and ends with its own x2 spatial stage"),
    "ic_lora": (("generate_audio", "audio_path", "two_stage_distilled", "upscale_temporal", "keyframes"),
                "with pipeline_type='ic-lora': ICLoraPipeline is video-only, conditions on its control video and image_path alone and ends "
                "with its own x2 spatial stage"),
    "a2vid": (("two_stage_distilled", "upscale_temporal", "retake_video"),          # keyframes / control_video: not owned, refused with the out-of-path defaults
              "with a2vid_two_stage: A2VidPipelineTwoStage generates the video to audio_path on the AudioVideo model, conditions on image_path "
              "alone and ends with its own x2 spatial stage"),
    "hq_av": (("audio_path", "two_stage_distilled", "upscale_temporal", "keyframes", "retake_video", "a2vid_two_stage"),
              "with ti2vid_hq_audio: TI2VidHQPipeline samples its own audio latent beside the video on the AudioVideo model, conditions on image_path "
              "alone and ends with its own x2 spatial stage"),
    "two_stage_cfg": (("ti2vid_hq_audio", "a2vid_two_stage", "retake_video", "keyframes", "two_stage_distilled", "upscale_temporal", "audio_path"),
                      "with two_stage_cfg: TwoStagePipeline samples its own audio latent beside the video on the AudioVideo model, conditions on image_path "
                      "alone and ends with its own x2 spatial stage"),
    "standard_cfg": (("generate_audio", "audio_path", "two_stage_distilled", "two_stage_cfg", "ti2vid_hq_audio", "a2vid_two_stage", "retake_video", "image_path"),
                     "with standard_cfg: the guided standard loop is video-only and has no conditioning code (the reference's standard loop has none); it runs one stage "
                     "on the video-only dev model"),
}
# route -> the _OUT_OF_PATH_DEFAULTS arguments that route takes itself.  apg_scale: the routes whose guided loop takes a guider (the AudioVideo route as
# OneStagePipeline's guider_override, keyframe stage 1, retake's guided mode).  stg_scale, stg_audio_scale and ge_gamma: OneStagePipeline alone (the AudioVideo
# route), and GE not beside STG (_check_sampler)
_ROUTE_OWNS = {"keyframe": ("keyframes", "apg_scale"), "hq": ("distilled_lora", "keyframes"),
               "ic_lora": ("control_video", "save_control", "keyframes", "ic_lora_weights"), "retake": ("apg_scale",), "av": ("apg_scale", "stg_scale", "stg_audio_scale", "ge_gamma"), "a2vid": ("distilled_lora",),
               "hq_av": ("distilled_lora",), "two_stage_cfg": ("distilled_lora",), "standard_cfg": ("negative_prompt", "cross_attn_scale"),
               "retake_av": ()}          # no guider override on the joint audio+video loop: apg_scale keeps its out-of-path refusal


def _owning_route(r):
    """The route whose _ROUTE_OWNS entry decides about apg_scale and stg_scale, before the checkpoint has been looked at: the named one (a distilled retake runs
    without guidance and owns no guider), else "av" when OneStagePipeline will run (generate_audio or an LTX-2.3 checkpoint, without two_stage_distilled)."""
    if r.route == "retake":
        return None if r.model_variant == "distilled" else "retake"
    if r.route is not None or r.two_stage_distilled:
        return r.route
    have_ckpt = bool(r.weights_path) and os.path.exists(r.weights_path)
    version = r.model_version if r.model_version is not None else (detect_model_version(r.weights_path) if have_ckpt else "")
    return "av" if (r.generate_audio or str(version).startswith("2.3")) else None


def _apg_guider(r):
    """The guider of apg_scale / apg_eta / apg_norm_threshold / apg_momentum (reference :1226-1242, with its lines :1033-1036 and :1242); None at apg_scale 1."""
    if r.apg_scale == 1.0:
        return None
    from ltx_2_mlx_amd.components import LegacyStatefulAPGGuider, LtxAPGGuider
    print(f"APG guidance: scale={r.apg_scale}, eta={r.apg_eta}, norm_threshold={r.apg_norm_threshold}")
    if r.apg_momentum > 0:
        print(f"  Using stateful APG with momentum={r.apg_momentum}")
        guider = LegacyStatefulAPGGuider(scale=r.apg_scale, eta=r.apg_eta, norm_threshold=r.apg_norm_threshold, momentum=r.apg_momentum)
    else:
        guider = LtxAPGGuider(scale=r.apg_scale, eta=r.apg_eta, norm_threshold=r.apg_norm_threshold)
    print("  APG guidance enabled (replaces standard CFG)")
    return guider


def _check_stg(r):
    """stg_scale > 0 (the reference enables STG for nothing else, :1246) or stg_audio_scale > 0: the mode that is built, block indices of this model, a cutoff that is a
    fraction of the steps.  stg_audio_scale is a number, not a negative one; it needs no stg_scale beside it (the audio alone may be STG-guided)."""
    if r.stg_audio_scale < 0:
        raise ValueError(f"stg_audio_scale={r.stg_audio_scale} must not be negative (0: the audio latent is not STG-guided)")
    if not (r.stg_scale > 0 or r.stg_audio_scale > 0):
        return
    if r.stg_mode != "video":
        raise NotImplementedError(f"stg_mode={r.stg_mode!r}: STG skips the video self-attention (the reference prints the mode and does the same); leave it at 'video'")
    bad = [b for b in (r.stg_blocks or []) if not 0 <= int(b) < r.num_layers]
    if bad:
        raise ValueError(f"stg_blocks {bad} out of range: the model has {r.num_layers} layers")
    if not 0.0 <= r.stg_cutoff <= 1.0:
        raise ValueError(f"stg_cutoff={r.stg_cutoff} must lie in [0, 1]: the fraction of the steps that STG guides")


def _check_first_block_cache(r, final: bool):
    """first_block_cache = t > 0 (--first-block-cache T): the first-block cache of the video-only standard loops (_run_standard: the plain loop and the standard_cfg one).  A negative
    threshold is a ValueError.  final=False, before the checkpoint is looked at: the named routes, STG, Heun / ancestral, GE and APG refuse it; final=True, once the route is known: the
    AudioVideo / LTX-2.3 route, the two-stage route and a conditioned (image_path) or placeholder standard run do."""
    t = r.first_block_cache
    if not float(t) >= 0.0:
        raise ValueError(f"first_block_cache={t!r} must be >= 0 (0: off)")
    if t == 0:
        return
    tail = "the first-block cache is built for the video-only standard loops alone (the plain loop and standard_cfg; see DESIGN.md)"
    if not final:
        if r.route not in (None, "standard_cfg"):
            raise NotImplementedError(f"first_block_cache={t!r} on the {r.route} route: {tail}")
        for k, off in (("stg_scale", 0.0), ("stg_audio_scale", 0.0), ("ge_gamma", 0.0), ("apg_scale", 1.0), ("sampler", "euler")):
            if getattr(r, k) != off:
                raise NotImplementedError(f"first_block_cache={t!r} beside {k}={getattr(r, k)!r}: {tail}")
        if r.two_stage_distilled:
            raise NotImplementedError(f"first_block_cache={t!r} with two_stage_distilled: {tail}")
        return
    if r.route not in ("standard", "standard_cfg"):
        raise NotImplementedError(f"first_block_cache={t!r} on the {'AudioVideo / LTX-2.3' if r.route == 'av' else r.route} route: {tail}")
    if r.image_path or r.use_placeholder:
        raise NotImplementedError(f"first_block_cache={t!r} with {'image_path' if r.image_path else 'use_placeholder'}: {tail}; the loop it caches has no conditioning")


def _check_sampler(r, owner):
    """sampler='heun' runs in OneStagePipeline alone (the AudioVideo route), and not beside STG.  sampler='euler_ancestral' runs there too -- under plain
    CFG or without guidance, not beside STG, GE, APG or cross_attn_scale -- and in stage 1 of two_stage_distilled (DistilledPipeline)."""
    if r.ancestral_eta < 0:
        raise ValueError(f"ancestral_eta={r.ancestral_eta} must not be negative (0: the Euler step)")
    if r.sampler == "euler":
        if r.ancestral_eta != 1.0:
            raise ValueError(f"ancestral_eta={r.ancestral_eta!r} goes with sampler='euler_ancestral'")
        return
    if r.sampler == "euler_ancestral" and r.two_stage_distilled and r.route is None:
        return
    if r.sampler == "euler_ancestral":
        if owner != "av":
            raise NotImplementedError(f"sampler={r.sampler!r} is built on the AudioVideo route (OneStagePipeline: generate_audio or an LTX-2.3 checkpoint) and "
                                      "for two_stage_distilled (DistilledPipeline's stage 1); leave it at its default 'euler'")
        for k, off in (("stg_scale", 0.0), ("stg_audio_scale", 0.0), ("ge_gamma", 0.0), ("apg_scale", 1.0), ("cross_attn_scale", 1.0)):
            if (getattr(r, k) > 0) if off == 0.0 else (getattr(r, k) != off):
                raise NotImplementedError(f"sampler={r.sampler!r} beside {k}={getattr(r, k)!r} is outside the MI355X hot path (see DESIGN.md)")
        if r.upscale_temporal:
            raise NotImplementedError(f"sampler={r.sampler!r} beside upscale_temporal is outside the MI355X hot path (see DESIGN.md)")
        return
    if owner != "av":
        raise NotImplementedError(f"sampler={r.sampler!r} is built on the AudioVideo route alone (OneStagePipeline: generate_audio or an LTX-2.3 checkpoint); "
                                  "leave it at its default 'euler'")
    if r.stg_scale > 0:
        raise NotImplementedError(f"sampler={r.sampler!r} beside stg_scale={r.stg_scale!r} is outside the MI355X hot path (see DESIGN.md)")
    if r.stg_audio_scale > 0:
        raise NotImplementedError(f"sampler={r.sampler!r} beside stg_audio_scale={r.stg_audio_scale!r} is outside the MI355X hot path (see DESIGN.md)")


def _refuse_combinations(r):
    names, tail = _ROUTE_EXCLUDES[r.route]
    for k in names:
        if getattr(r, k) and (k, getattr(r, k)) != ("pipeline_type", "text-to-video"):
            raise NotImplementedError(f"{k} {tail}")


def _lora_config(r, path, strength, what):
    """The LoRAConfig of a route's own adapter (None without one); fusion needs dequantised weights and the file."""
    if not path:
        return None
    if r.fp8_resident:
        raise NotImplementedError("LoRA fusion needs dequantised weights: drop fp8_resident")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{what} not found: {path}")
    from ltx_2_mlx_amd.loader.lora_loader import LoRAConfig
    return LoRAConfig(path, strength)


def _need_spatial_upscaler(r):
    if not r.spatial_upscaler_weights:
        raise ValueError(f"pipeline_type={r.pipeline_type!r} needs --spatial-upscaler-weights (its second stage runs at twice the resolution)")


def _resolve_retake(r):
    """The source clip decides height, width, num_frames and the rate; the window is checked against it."""
    from ltx_2_mlx_amd.pipelines import RetakeConfig, TemporalRegionMask, end_of_clip, get_video_metadata
    r.retake_video = str(r.retake_video)
    # an array or a directory carries no frame rate: it plays at output_fps; a video file at its own
    plays_at_output_fps = os.path.isdir(r.retake_video) or r.retake_video.lower().endswith((".npy", ".npz"))
    r.retake_fps, src_frames, r.width, r.height = get_video_metadata(r.retake_video, float(r.output_fps) if plays_at_output_fps else None)
    if src_frames < 1:
        raise ValueError(f"Could not read any frames from {r.retake_video}")
    r.num_frames = ((src_frames - 1) // 8) * 8 + 1
    if r.height % 32 != 0 or r.width % 32 != 0:
        raise ValueError(f"Source resolution ({r.width}x{r.height}) must be divisible by 32 (the source is not resized)")
    r.retake_to_end = r.retake_end_time is None
    if r.retake_to_end:
        r.retake_end_time = end_of_clip(r.num_frames, r.retake_fps)        # not num_frames / fps: int(end * fps) must reach the last frame
    RetakeConfig(start_time=r.retake_start_time, end_time=r.retake_end_time)          # its ValueError (start_time >= end_time)
    latent_frames = (r.num_frames - 1) // 8 + 1
    r.retake_window = TemporalRegionMask(r.retake_start_time, r.retake_end_time, r.retake_fps).frame_window(latent_frames)
    if r.retake_window[0] >= r.retake_window[1]:
        raise ValueError(f"the retake window {r.retake_start_time}s - {r.retake_end_time}s touches no frame of the source: it has "
                         f"{r.num_frames} frames at {r.retake_fps:g} fps, {r.num_frames / r.retake_fps:.3f} s")


def _resolve_keyframe(r):
    from ltx_2_mlx_amd.pipelines import KeyframeInterpolationConfig
    KeyframeInterpolationConfig(height=r.height, width=r.width, num_frames=r.num_frames)          # its ValueErrors (8k + 1 frames, multiples of 64)
    r.parsed_keyframes = [parse_keyframe(k) for k in r.keyframes]
    for kf in r.parsed_keyframes:
        if not 0 <= kf.frame_index < r.num_frames:
            raise ValueError(f"keyframe frame_index {kf.frame_index} is outside [0, {r.num_frames})")
        if kf.image is None and not os.path.exists(kf.image_path):
            raise FileNotFoundError(f"keyframe image not found: {kf.image_path}")


def _resolve_hq(r):
    _need_spatial_upscaler(r)
    from ltx_2_mlx_amd.pipelines import TI2VidHQConfig
    TI2VidHQConfig(height=r.height, width=r.width, num_frames=r.num_frames)          # its ValueErrors (8k + 1 frames, multiples of 64)
    r.hq_lora = _lora_config(r, r.distilled_lora, r.distilled_lora_scale, "distilled LoRA")


def _resolve_ic_lora(r):
    _need_spatial_upscaler(r)
    from ltx_2_mlx_amd.pipelines import ControlType, ICLoraConfig
    ICLoraConfig(height=r.height, width=r.width, num_frames=r.num_frames)          # its ValueErrors (8k + 1 frames, multiples of 64)
    ControlType(r.control_type)                                                      # ValueError for anything but "canny" / "raw"
    if r.control_video and not os.path.exists(r.control_video):
        raise FileNotFoundError(f"control video not found: {r.control_video}")
    lora = _lora_config(r, r.ic_lora_weights, 1.0, "IC-LoRA weights")
    r.ic_loras = [lora] if lora else []


def _resolve_a2vid(r):
    if not r.audio_path:
        raise ValueError("a2vid_two_stage needs audio_path (--audio): the video is generated to that audio track")
    _need_spatial_upscaler(r)
    from ltx_2_mlx_amd.pipelines import A2VidConfig
    A2VidConfig(height=r.height, width=r.width, num_frames=r.num_frames)          # its ValueErrors (8k + 1 frames, multiples of 64)
    r.a2vid_lora = _lora_config(r, r.distilled_lora, r.distilled_lora_scale, "distilled LoRA")
    r.generate_audio = True          # the AudioVideo transformer and both text encodings, as generate_audio asks for them


def _resolve_hq_av(r):
    _need_spatial_upscaler(r)
    from ltx_2_mlx_amd.pipelines import TI2VidHQConfig
    TI2VidHQConfig(height=r.height, width=r.width, num_frames=r.num_frames)          # its ValueErrors (8k + 1 frames, multiples of 64)
    r.hq_lora = _lora_config(r, r.distilled_lora, r.distilled_lora_scale, "distilled LoRA")
    r.generate_audio = True          # the AudioVideo transformer and both text encodings, as generate_audio asks for them


def _resolve_two_stage_cfg(r):
    _need_spatial_upscaler(r)
    from ltx_2_mlx_amd.pipelines import TwoStageCFGConfig
    TwoStageCFGConfig(height=r.height, width=r.width, num_frames=r.num_frames)          # its ValueErrors (8k + 1 frames, multiples of 64)
    r.two_stage_lora = _lora_config(r, r.distilled_lora, r.distilled_lora_scale, "distilled LoRA")
    r.generate_audio = True          # the AudioVideo transformer and both text encodings, as generate_audio asks for them


def _resolve_retake_av(r):
    """The silent route's checks on the clip and the window, then the sound track: it must exist; the AudioVideo transformer and both text encodings, as generate_audio asks for them."""
    _resolve_retake(r)
    r.retake_audio = str(r.retake_audio)
    if not os.path.exists(r.retake_audio):
        raise FileNotFoundError(f"retake audio track not found: {r.retake_audio}")
    if r.retake_audio_cfg is not None and not r.retake_audio_cfg >= 0.0:
        raise ValueError(f"retake_audio_cfg={r.retake_audio_cfg} must be >= 0")
    r.generate_audio = True


def _resolve_standard_cfg(r):
    if r.pipeline_type not in _PIPELINES_BUILT:
        raise NotImplementedError(f"pipeline_type={r.pipeline_type!r} with standard_cfg: the guided standard loop is the reference's one-stage text-to-video route; "
                                  "leave pipeline_type at 'text-to-video'")


_RESOLVE_ROUTE = {"standard_cfg": _resolve_standard_cfg, "two_stage_cfg": _resolve_two_stage_cfg, "keyframe": _resolve_keyframe, "hq": _resolve_hq, "ic_lora": _resolve_ic_lora, "a2vid": _resolve_a2vid, "hq_av": _resolve_hq_av}


def _resolve_request(kw: dict):
    """generate_video's keywords -> the request: those keywords as attributes, overwritten where validation decides otherwise (a retake's height / width / num_frames / retake_end_time, the forced
    and defaulted guidance scales, compute_dtype), plus `route` (the ONE of keyframe, hq, ic_lora, retake, two_stage, av, standard that runs) and what validation derives: retake_fps /
    retake_to_end / retake_window, parsed_keyframes, hq_lora / ic_loras, cdt, need_cfg, gemma_encodes, encode_negative, have_ckpt / version / v2 / av, toy, output_dir, and negative_encoding /
    negative_audio_encoding of the embedding file.  Loads no model and touches no GPU; every refusal is raised here, in a fixed order.  Returns None (after saying so) when Gemma is asked for and
    its weights are missing."""
    r = SimpleNamespace(**kw, retake_fps=None, retake_to_end=False, retake_window=None, parsed_keyframes=[], hq_lora=None, ic_loras=[], a2vid_lora=None, two_stage_lora=None)
    if r.retake_audio is not None and r.retake_video is None:
        raise ValueError("retake_audio (--retake-audio) is the sound track of retake_video (--retake): pass the clip as well")
    if r.standard_cfg:
        r.route = "standard_cfg"
    elif r.two_stage_cfg:
        r.route = "two_stage_cfg"
    elif r.ti2vid_hq_audio:
        r.route = "hq_av"
    elif r.a2vid_two_stage:
        r.route = "a2vid"
    elif r.retake_video is not None and r.retake_audio is not None:
        r.route = "retake_av"
    elif r.retake_video is not None:
        r.route = "retake"
    elif r.pipeline_type == "keyframe-interpolation" and bool(r.keyframes):
        r.route = "keyframe"
    elif r.pipeline_type == "ti2vid-hq":
        r.route = "hq"
    elif r.pipeline_type == "ic-lora" and bool(r.control_video or r.image_path):
        r.route = "ic_lora"
    else:
        r.route = None                                                   # two_stage, av or standard: decided below, once the checkpoint is looked at
    _check_first_block_cache(r, final=False)                             # an MI355X extra of two routes: refused by name before a named route looks at its files
    if r.route == "retake":                                              # its refusals win over every other one
        _refuse_combinations(r)
        _resolve_retake(r)
    elif r.route == "retake_av":
        _refuse_combinations(r)
        _resolve_retake_av(r)
    # Gemma encodes the prompt (and the negative prompt) when its weights are there and no pre-computed encoding is given
    r.gemma_encodes = bool(r.use_gemma and not (r.embedding_path or r.text_features_path) and r.gemma_path and os.path.exists(r.gemma_path))
    if r.sampler not in ("euler", "heun", "euler_ancestral"):
        raise ValueError(f"sampler={r.sampler!r}: 'euler', 'heun' or 'euler_ancestral'")
    asks_av = r.apg_scale != 1.0 or r.stg_scale != 0.0 or r.stg_audio_scale != 0.0 or r.ge_gamma != 0.0 or r.sampler != "euler"
    owner = _owning_route(r) if asks_av else r.route
    owns = _ROUTE_OWNS.get(owner, ())
    if r.stg_scale > 0 or r.stg_audio_scale > 0:
        owns = tuple(k for k in owns if k != "ge_gamma")          # GE beside STG is not built: its out-of-path refusal
    for k, default in _OUT_OF_PATH_DEFAULTS.items():
        if k in owns or (k == "negative_prompt" and r.gemma_encodes):
            continue
        if k == "cross_attn_scale" and r.route is None and not r.two_stage_distilled and _owning_route(r) is None:
            continue                                  # the plain standard route applies it too, as the reference does (:1174)
        v = (r.enhance_prompt_flag and r.use_gemma) if k == "enhance_prompt_flag" else getattr(r, k)
        if v != default:
            raise NotImplementedError(f"{k}={v!r} is outside the MI355X hot path (see DESIGN.md); leave it at its default {default!r}")
    if r.pipeline_type not in _PIPELINES_KNOWN:
        raise ValueError(f"unknown pipeline_type {r.pipeline_type!r}; the reference knows {_PIPELINES_KNOWN}")
    _check_stg(r)
    _check_sampler(r, owner)
    if r.pipeline_type not in _PIPELINES_BUILT and r.route not in _RESOLVE_ROUTE:
        raise NotImplementedError(f"pipeline_type={r.pipeline_type!r} is outside the MI355X hot path (see DESIGN.md): 'two-stage' is the dev "
                                  "model's CFG stage 1 + distilled-LoRA stage 2; for the distilled two-stage DistilledPipeline pass "
                                  "two_stage_distilled=True (--two-stage-distilled); 'keyframe-interpolation' is built and needs its "
                                  "images: pass keyframes / --keyframe path:frame_index[:strength]; 'ic-lora' is built and needs its control "
                                  "video and / or an image: pass control_video / --control-video (--image)")
    if r.route in _RESOLVE_ROUTE:
        _refuse_combinations(r)
        _RESOLVE_ROUTE[r.route](r)
    r.output_dir = os.path.dirname(r.output_path)
    if r.output_dir:
        os.makedirs(r.output_dir, exist_ok=True)          # reference :1000-1003
    if r.num_frames % 8 != 1:
        raise ValueError(f"num_frames must be 8*k + 1, got {r.num_frames}")
    if r.height % 32 != 0 or r.width % 32 != 0:
        raise ValueError(f"Resolution ({r.height}x{r.width}) must be divisible by 32")
    # use_fp16=True (the reference's default, :1006): float16 operands on libltx2hip_f16.so; compute_dtype="bfloat16" (MI355X extra,
    # --bf16) selects the bfloat16 build the headline benchmark runs.  Accumulation and the residual stream are fp32 in both.
    if r.compute_dtype is None:
        if not r.use_fp16:
            raise NotImplementedError("use_fp16=False (fp32 compute): the MI355X path computes with float16 or bfloat16 operands, fp32 accumulation and an "
                                      "fp32 residual stream")
        r.compute_dtype = "float16"
    if r.compute_dtype not in ("float16", "bfloat16"):
        raise ValueError(f"compute_dtype={r.compute_dtype!r}: float16 or bfloat16")
    r.cdt = torch.float16 if r.compute_dtype == "float16" else torch.bfloat16
    # printed here, not by generate_video: it has always come before the notes and the refusals below
    print(f"Compute dtype: {r.compute_dtype} operands / fp32 accumulate / fp32 residual stream")
    if r.use_gemma and not (r.embedding_path or r.text_features_path):
        if not os.path.exists(r.gemma_path):              # the reference prints this and returns (:1085-1092)
            print(f"\n  ERROR: Gemma weights not found at {r.gemma_path}\n  Use use_gemma=False (--no-gemma) for dummy embeddings, or pass "
                  f"embedding_path / text_features_path")
            return None
    if r.route == "standard_cfg" and r.model_variant == "distilled":
        print("  standard_cfg with model_variant='distilled': the reference forces cfg = 1 and guidance_rescale = 0 for the distilled variant; running the plain loop")
        r.cfg_scale, r.guidance_rescale = 1.0, 0.0
    if r.model_variant == "distilled" and r.cfg_scale > 1.2:
        print(f"  WARNING: Distilled model requires CFG=1.0 (no guidance). You requested {r.cfg_scale}.\n  Forcing CFG=1.0 (reference :1207-1216).")
        r.cfg_scale, r.guidance_rescale, r.audio_cfg_scale, r.rescale_scale = 1.0, 0.0, 1.0, 0.0
    # Guidance scales are resolved BEFORE any model is loaded: the AudioVideo branch's defaults for a non-distilled variant are
    # audio_cfg_scale 7.0 / rescale 0.7 (reference :1713-1716), i.e. guidance even at --cfg 1.0, and guidance needs negative encodings.
    if r.audio_cfg_scale is None:
        r.audio_cfg_scale = 1.0 if r.model_variant == "distilled" else 7.0
    if r.rescale_scale is None:
        r.rescale_scale = 0.0 if r.model_variant == "distilled" else 0.7
    if r.stg_scale > 0:
        print(f"STG guidance: scale={r.stg_scale}, mode={r.stg_mode}")           # the settings banner's line (reference :1031-1032); the second one: _run_av
    if r.stg_audio_scale > 0:
        print(f"Audio STG guidance: scale={r.stg_audio_scale} (the audio self-attention of the STG blocks is skipped too)")
    if r.sampler == "euler_ancestral" and r.rescale_scale > 0 and not r.two_stage_distilled and (r.cfg_scale != 1.0 or r.audio_cfg_scale != 1.0):
        raise NotImplementedError(f"sampler={r.sampler!r} runs under plain CFG (rescale_scale=0.0) or without guidance: beside CFG* it is outside the MI355X hot path")
    if r.sampler == "euler_ancestral":
        print(f"Sampler: {r.sampler}, eta={r.ancestral_eta} (noise seed {r.seed}, made in the step kernel)")
    if r.sampler == "heun" or r.ge_gamma > 0:
        print(f"Sampler: {r.sampler}" + (" (2x model evals per step)" if r.sampler == "heun" else "") + (f", GE gamma={r.ge_gamma}" if r.ge_gamma > 0 else ""))
    r.apg_guider = _apg_guider(r)
    if r.stg_audio_scale > 0 and (r.apg_guider is not None or (r.rescale_scale > 0 and (r.cfg_scale != 1.0 or r.audio_cfg_scale != 1.0))):
        raise NotImplementedError(f"stg_audio_scale={r.stg_audio_scale!r} runs under plain CFG (rescale_scale=0.0, apg_scale=1.0) or without guidance: beside "
                                  "CFG* / APG the eager loop STG-guides the video alone")
    r.negative_encoding = r.negative_audio_encoding = None
    if r.embedding_path and os.path.exists(r.embedding_path):
        with np.load(r.embedding_path) as z:                # optional entries of the pre-computed embedding file: the negative prompt's encodings
            if "negative_embedding" in z:
                r.negative_encoding = _batched(torch.from_numpy(z["negative_embedding"]).float())
            if "negative_audio_embedding" in z:
                r.negative_audio_encoding = _batched(torch.from_numpy(z["negative_audio_embedding"]).float())
    # reference :1073: V2.3 always uses the AV transformer and the dual text encodings; generate_audio asks for them
    r.have_ckpt = bool(r.weights_path) and os.path.exists(r.weights_path)
    r.version = r.model_version if r.model_version is not None else (detect_model_version(r.weights_path) if r.have_ckpt else "")
    r.v2 = str(r.version).startswith("2.3")
    r.av = bool(r.generate_audio or r.v2)
    if r.route == "standard_cfg" and r.v2:
        raise NotImplementedError(f"standard_cfg with an LTX-{r.version} / AudioVideo checkpoint: the guided standard loop runs the video-only dev model; "
                                  "LTX-2.3 and AudioVideo checkpoints are guided by OneStagePipeline (drop standard_cfg)")
    # the video-only loop of the reference guides only for cfg_scale > 1 (:1935); OneStagePipeline's guiders are enabled for any scale != 1
    r.need_cfg = (r.cfg_scale != 1.0 or r.audio_cfg_scale != 1.0 or r.apg_guider is not None) if r.av else r.cfg_scale > 1.0
    if r.audio_path and r.route == "a2vid":
        if not os.path.exists(r.audio_path):
            raise FileNotFoundError(f"audio file not found: {r.audio_path}")
    elif r.audio_path:
        if r.two_stage_distilled:
            raise NotImplementedError("audio_path (--audio) with two_stage_distilled: DistilledPipeline with a given audio latent is not built")
        if not r.av:
            raise ValueError("audio_path (--audio) needs the AudioVideo branch: pass generate_audio=True (--generate-audio) or an LTX-2.3 checkpoint; "
                             "the video-only transformer has no audio stream to condition on")
        if not os.path.exists(r.audio_path):
            raise FileNotFoundError(f"audio file not found: {r.audio_path}")
    if r.upscale_temporal and (r.av or r.two_stage_distilled):
        raise NotImplementedError("upscale_temporal with the " + ("AudioVideo pipeline (the reference's AV branch returns before its upscalers)" if r.av
                                  else "two-stage DistilledPipeline (it returns before the post-denoise upscalers)"))
    if r.route is not None:
        r.need_cfg = False                  # guided by the pipeline itself (ic-lora: not at all); a missing negative encoding becomes zeros
    if r.need_cfg and not r.av:
        raise NotImplementedError(f"cfg_scale={r.cfg_scale}: classifier-free guidance is built in OneStagePipeline (the AudioVideo / LTX-2.3 branch); the "
                                  "standard video-only loop of this script runs the distilled model's cfg = 1")
    if r.need_cfg and not r.gemma_encodes and (r.negative_encoding is None or r.negative_audio_encoding is None):
        raise NotImplementedError(f"cfg_scale={r.cfg_scale} / audio_cfg_scale={r.audio_cfg_scale}: classifier-free guidance needs the NEGATIVE prompt's encodings: "
                                  "let Gemma encode the prompts (gemma_path), add `negative_embedding` and `negative_audio_embedding` arrays to the --embedding "
                                  "file, or pass cfg_scale=1.0, audio_cfg_scale=1.0 (what --model-variant distilled does)")
    if r.low_memory or r.fast_mode:
        print("  low_memory / fast_mode: no effect here (weights and caches stay resident in HBM, the loop is one hipGraph)")
    # the routes that guide themselves take Gemma's encoding of the negative prompt when they will guide (retake: the dev variant only)
    r.encode_negative = (r.cfg_scale != 1.0 or r.apg_guider is not None) and (r.route in ("keyframe", "hq", "a2vid", "hq_av", "two_stage_cfg") or (r.route == "retake" and r.model_variant != "distilled")
                                                                                  or (r.route == "standard_cfg" and r.cfg_scale > 1.0))
    r.toy = r.vae_base_channels is not None and r.vae_base_channels != 128        # debug-size VAE: matching debug-size upscaler / encoder
    if r.route is None:
        r.route = "two_stage" if r.two_stage_distilled else "av" if r.av else "standard"
    _check_first_block_cache(r, final=True)
    return r


# ---- the session: what the three load stages leave behind, and the pieces the routes share ----

def _encode_text(r):
    """[1/5] -> (text_encoding, text_audio_encoding or None, negative_encoding, negative_audio_encoding): the negatives are the embedding file's unless Gemma encodes the negative prompt."""
    print("[1/5] text encoding")
    weights = r.weights_path if r.have_ckpt else None
    audio, negative, negative_audio = None, r.negative_encoding, r.negative_audio_encoding
    if r.text_features_path:
        text, _ = encode_text_features(r.text_features_path, weights, r.device, r.seed)
    elif r.gemma_encodes and r.av:
        # prompt AND negative prompt under one Gemma load (reference :1096-1116); Gemma is freed before the transformer loads.  LTX-2.3
        # gets the V2 encoder: encodings at the transformer's own widths (num_heads * 128 video, num_heads * 64 audio)
        results = encode_av_gemma_batch([r.prompt, r.negative_prompt or ""], r.gemma_path, weights, device=r.device, seed=r.seed,
                                        model_version=r.version, num_heads=r.num_heads)
        text, audio, _ = results[0]
        negative, negative_audio, _ = results[1]
        print("  Encoded both prompts with Gemma 3 (AudioVideo, single load)")
    elif r.gemma_encodes:
        text, _ = encode_with_gemma(r.prompt, r.gemma_path, weights, use_early_layers_only=r.early_layers_only, device=r.device, seed=r.seed)
        print("  Encoded with Gemma 3")
        if r.encode_negative:
            negative, _ = encode_with_gemma(r.negative_prompt or "", r.gemma_path, weights, device=r.device, seed=r.seed)
            print("  Encoded the negative prompt with Gemma 3")
    elif r.embedding_path:
        with np.load(r.embedding_path) as z:              # keys as the reference's load_text_embedding (:730-750), plus the audio encoding
            text = _batched(torch.from_numpy(z["embedding"]).float()).to(r.device)
            if r.av and "audio_embedding" in z:
                audio = _batched(torch.from_numpy(z["audio_embedding"]).float().to(r.device))
            elif r.av:
                print("  WARNING: Pre-computed embeddings don't include audio encoding. Audio quality may be degraded.")
    else:
        # dummy encodings (reference :1129-1138).  LTX-2.3 has no caption projection: its contexts arrive at the transformer
        # widths (4096 video / 2048 audio) -- the reference's 3840-wide dummy would not fit that model at all
        text, _ = create_dummy_text_encoding(r.prompt, embed_dim=r.num_heads * 128 if r.v2 else 3840, device=r.device)
        if r.v2:
            audio, _ = create_dummy_text_encoding(r.prompt + " (audio)", embed_dim=r.num_heads * 64, device=r.device)
        print("  Using DUMMY encoding (test mode - output will be random)")
    if r.av and audio is None:
        audio = text                                    # reference :1080-1081, :1131-1132
    return text, audio, negative, negative_audio


def _load_model(r, text_encoding):
    """[2/5] -> the X0Model of the video-only or the AudioVideo transformer; None in placeholder mode."""
    print("[2/5] transformer")
    if r.use_placeholder:
        print("  Skipping model load (placeholder mode)")
        return None
    if r.av:
        return X0Model(load_av_transformer(r.weights_path, num_layers=r.num_layers, compute_dtype=r.cdt, use_fp8=r.use_fp8, low_memory=r.low_memory,
                                           caption_channels=None if r.v2 else text_encoding.shape[-1], cross_attention_adaln=r.v2,
                                           apply_gated_attention=r.v2, num_heads=r.num_heads, seed=r.seed, device=r.device,
                                           lora_path=r.lora_path, lora_strength=r.lora_strength, fp8_compute=r.fp8_compute))
    return X0Model(load_transformer(r.weights_path, num_layers=r.num_layers, compute_dtype=r.cdt, use_fp8=r.use_fp8, low_memory=r.low_memory,
                                    fast_mode=r.fast_mode, num_heads=r.num_heads, caption_channels=text_encoding.shape[-1], seed=r.seed,
                                    device=r.device, lora_path=r.lora_path, lora_strength=r.lora_strength, fp8_resident=r.fp8_resident,
                                    fp8_compute=r.fp8_compute))


def _load_vae_decoder(r):
    """[3/5] -> the decoder; None with skip_vae."""
    print("[3/5] VAE decoder")
    if r.skip_vae:
        print("  VAE decoder skipped by user")
        return None
    return create_vae_decoder(r.weights_path, r.device, r.seed + 1, r.use_placeholder, r.vae_base_channels, compute_dtype=r.cdt)


def make_encoder(r):
    enc = SimpleVideoEncoder(device=r.device)
    if r.have_ckpt:
        load_vae_encoder_weights(enc, r.weights_path)
    else:
        enc.init_random_weights(seed=r.seed + 2)
    return enc


def _load_or_random(r, kind, weights=None):
    """The "spatial" or "temporal" x2 latent upscaler: from `weights` (the request's by default), or random-initialised for "random" and (with a warning) for a missing file, then with one block
    per stage at the debug width a toy VAE asks for."""
    import ltx_2_mlx_amd.model.upscaler as U
    cls, load, width_name, width, blocks_name, seed, kw = {
        "spatial": (U.SpatialUpscaler, U.load_spatial_upscaler_weights, "mid_channels", 1024, "num_blocks_per_stage", r.seed + 2, {}),
        "temporal": (U.TemporalUpscaler, U.load_temporal_upscaler_weights, "hidden_channels", 512, "num_res_blocks", r.seed + 4,
                     dict(checkpoint_semantics=r.temporal_upscaler_checkpoint_semantics))}[kind]
    weights = weights or getattr(r, kind + "_upscaler_weights")
    kw = dict(kw, device=r.device, **{width_name: 64 if r.toy else width})
    if weights == "random" or not os.path.exists(str(weights)):
        if weights != "random":
            print(f"  Warning: Weights not found at {weights}, using random init")
        up = cls(**kw, **{blocks_name: 4 if kw[width_name] == width else 1})
        up.init_random_weights(seed=seed)
    else:
        up = cls(**kw)
        load(up, weights)
    return up


# route -> (without a model, without a VAE decoder, what placeholder mode is told instead of the first, whether the decoder is asked for first)
_REQUIRES = {
    "keyframe": ("Keyframe interpolation pipeline requires a loaded model", "Keyframe interpolation pipeline requires VAE decoder",
                 "  Keyframe interpolation requires model - cannot use placeholder mode", False),
    "hq": ("TI2Vid HQ pipeline requires a loaded model", "TI2Vid HQ pipeline requires VAE decoder", None, False),
    "ic_lora": ("IC-LoRA pipeline requires a loaded model", "IC-LoRA pipeline requires VAE decoder", None, False),
    "retake": ("Retake pipeline requires a loaded model", "Retake pipeline requires VAE decoder", None, False),
    "retake_av": ("Retake pipeline requires a loaded model", "Retake pipeline requires VAE decoder", None, False),
    "two_stage": ("Two-stage pipeline requires a loaded model (cannot use placeholder mode)",
                  "the two-stage pipeline needs the VAE weights (per-channel statistics): drop --skip-vae", None, True),
    "av": (None, "AV pipeline requires VAE decoder", "  AV pipeline requires model - cannot use placeholder mode", False),
    "a2vid": ("A2Vid pipeline requires a loaded model", "A2Vid pipeline requires VAE decoder", None, False),
    "hq_av": ("TI2Vid HQ pipeline requires a loaded model", "TI2Vid HQ pipeline requires VAE decoder", None, False),
    "two_stage_cfg": ("Two-stage pipeline requires a loaded model", "Two-stage pipeline requires VAE decoder", None, False),
}


def _require(r, s) -> bool:
    """The route's pipeline needs the model and the decoder: ValueError without one.  False where placeholder mode is told so instead and
    generate_video returns None."""
    no_model, no_decoder, placeholder_note, decoder_first = _REQUIRES[r.route]
    if decoder_first and s.vae_decoder is None:
        raise ValueError(no_decoder)
    if s.model is None:
        if placeholder_note and (r.use_placeholder or no_model is None):
            print(placeholder_note)
            return False
        raise ValueError(no_model)
    if s.vae_decoder is None:
        raise ValueError(no_decoder)
    return True


def _banners(r, upscaler: bool):
    """The load stages a conditioned route adds: the VAE encoder (random-initialised without a checkpoint), the spatial upscaler."""
    print("[3.5/5] VAE encoder")
    if not r.have_ckpt:
        print("  Warning: no checkpoint, the VAE encoder is random-initialised")
    if upscaler:
        print("[3.6/5] spatial upscaler")


def _negative_or_zeros_note(guided: bool, negative) -> bool:
    """Says that a guided run without a negative encoding gets zeros; True when it does."""
    if guided and negative is None:
        print("  Negative prompt: no encoding given, using zeros of the context's shape (the reference's null text encoding)")
        return True
    return False


def _image_conditions(r):
    """image_path as the frame-0 condition of the routes that take one through their pipeline."""
    if not r.image_path:
        return []
    from ltx_2_mlx_amd.pipelines import ImageCondition
    print(f"  Image conditioning: {r.image_path} (strength={r.image_strength})")
    return [ImageCondition(image_path=r.image_path, frame_index=0, strength=r.image_strength)]


def _tiling(r):
    return TilingConfig.default() if r.tiled_vae else None


def _timed_run(label, run, tokens_of=None):
    """Runs a pipeline and reports its time -> (uint8 frames, audio latent or None).  tokens_of: the pipeline whose per-stage token counts close the line."""
    t0 = time.time()
    out = run()
    video, audio_latent = out if isinstance(out, tuple) else (out, None)
    frames = _frames_from_video(video)
    torch.cuda.synchronize()
    print(f"  {label}: {(time.time() - t0):.3f} s -> {tuple(frames.shape)}" + (f", DiT tokens per stage {tokens_of.token_counts}" if tokens_of else ""))
    return frames, audio_latent


def decode_audio_latent(r, s, audio_latent):
    """the latent is always kept as <stem>_audio_latent.npz; with decoders it also becomes the waveform (a sidecar .wav)"""
    np.savez(s.base + "_audio_latent.npz", latent=audio_latent.float().cpu().numpy())
    decoders = create_audio_decoders(r.decode_audio, r.weights_path if r.have_ckpt else None, device=r.device, seed=r.seed + 3)
    if decoders is None:
        return None
    t0 = time.time()
    waveform = decoders[1](decoders[0](audio_latent))
    torch.cuda.synchronize()
    print(f"  audio decode: {(time.time() - t0):.3f} s -> {tuple(waveform.shape)} at {decoders[1].output_sample_rate} Hz")
    return waveform, decoders[1].output_sample_rate


def finish(r, s, frames, audio=None, source_fps=None):
    """Writes <stem>.npz and the video file -> frames.  audio: (waveform, rate) to mux in.  source_fps: a retake is written at its source's rate: the frames enter ffmpeg at it and none is
    interpolated."""
    fps, input_fps = (r.output_fps, NATIVE_FPS) if source_fps is None else (source_fps, source_fps)
    frames_np = frames.cpu().numpy()
    np.savez_compressed(s.base + ".npz", frames=frames_np)
    if audio is not None and r.save_mp4:
        at_source_rate = {} if source_fps is None else dict(input_fps=input_fps)          # the retake route with sound
        video_out, wav = save_video_with_audio(frames_np, audio[0], r.output_path, audio[1], fps=fps, speed=r.output_speed, **at_source_rate)
        print(f"  video: {video_out}, audio: {wav}")
    elif audio is not None:
        print(f"  audio: {write_wav(s.base + '.wav', audio[0], audio[1])}")
    elif r.save_mp4:
        print(f"  video: {save_video(frames_np, r.output_path, fps=fps, speed=r.output_speed, input_fps=input_fps)}")
    print(f"Done in {time.time() - s.t_all:.1f} s: {s.base}.npz")
    return frames


# ---- one function per route: (request, session) -> what finish returns ----

def _run_keyframe(r, s):
    """pipeline_type="keyframe-interpolation" with keyframes (a list of 'path:frame_index[:strength]' strings, one per --keyframe) runs KeyframeInterpolationPipeline (reference :1552-1637): stage
    1 at half resolution over num_steps with classifier-free guidance at cfg_scale (model_variant="distilled" forces 1), x2 spatial upscale, 3 refinement steps; the VAE encoder and the spatial
    upscaler are loaded (random-initialised with a warning when the file is missing).  The negative encoding is Gemma's of `negative_prompt or ""` when Gemma encodes, else `negative_embedding` of
    the --embedding file, else zeros.  Not combined with generate_audio, audio_path, two_stage_distilled, upscale_temporal or image_path.  Without keyframes the pipeline_type raises
    NotImplementedError."""
    print("\n=== Using Keyframe Interpolation Pipeline ===")
    for kf in r.parsed_keyframes:
        print(f"  Keyframe: {kf.image_path} at frame {kf.frame_index} (strength={kf.strength})")
    if not _require(r, s):
        return None
    from ltx_2_mlx_amd.pipelines import KeyframeInterpolationConfig, KeyframeInterpolationPipeline
    conf = KeyframeInterpolationConfig(height=r.height, width=r.width, num_frames=r.num_frames, seed=r.seed, fps=24.0, num_inference_steps=r.num_steps,
                                       cfg_scale=r.cfg_scale, use_hip_graph=r.use_hip_graph, tiling_config=_tiling(r))
    _banners(r, upscaler=True)
    pipe = KeyframeInterpolationPipeline(s.model, make_encoder(r), s.vae_decoder, spatial_upscaler=_load_or_random(
        r, "spatial", r.spatial_upscaler_weights or "weights/ltx-2/ltx-2-spatial-upscaler-x2-1.0.safetensors"))
    _negative_or_zeros_note(conf.cfg_scale != 1.0 or r.apg_guider is not None, s.negative_encoding)
    print(f"[5/5] Running keyframe interpolation ({r.num_steps} steps)...")
    guider = dict(guider=r.apg_guider) if r.apg_guider is not None else {}
    frames, _ = _timed_run("keyframe interpolation",
                           lambda: pipe(s.text_encoding, None, r.parsed_keyframes, conf, negative_text_encoding=s.negative_encoding, **guider), tokens_of=pipe)
    return finish(r, s, frames)


def _run_hq(r, s):
    """pipeline_type="ti2vid-hq" (--ti2vid-hq) runs TI2VidHQPipeline (reference pipelines/ti2vid_hq.py; its own CLI never reaches it): num_steps res_2s second-order steps at half resolution with
    classifier-free guidance at cfg_scale, the x2 spatial upscale (spatial_upscaler_weights is required, "random" for a random-initialised one) and 3 distilled steps, under distilled_lora when
    given. image_path sits at frame 0.  The negative encoding as for keyframes.  Not combined with generate_audio, audio_path, two_stage_distilled, upscale_temporal or keyframes, nor
    distilled_lora with fp8_resident."""
    images = _image_conditions(r)
    print("\n=== Using TI2Vid HQ Pipeline (res_2s) ===")
    _require(r, s)
    from ltx_2_mlx_amd.pipelines import TI2VidHQConfig, TI2VidHQPipeline
    conf = TI2VidHQConfig(height=r.height, width=r.width, num_frames=r.num_frames, seed=r.seed, num_inference_steps=r.num_steps,
                          cfg_scale=r.cfg_scale, audio_cfg_scale=r.audio_cfg_scale, distilled_lora_config=r.hq_lora, use_hip_graph=r.use_hip_graph,
                          tiling_config=_tiling(r))
    _banners(r, upscaler=True)
    pipe = TI2VidHQPipeline(s.model, make_encoder(r), s.vae_decoder, _load_or_random(r, "spatial"))
    negative = s.negative_encoding
    if _negative_or_zeros_note(r.cfg_scale > 1.0 or r.audio_cfg_scale > 1.0, negative):
        negative = torch.zeros_like(s.text_encoding)
    print(f"[5/5] Running TI2Vid HQ ({r.num_steps} res_2s steps at {r.width // 2}x{r.height // 2}, then 3 at {r.width}x{r.height})...")
    frames, _ = _timed_run("ti2vid-hq", lambda: pipe(s.text_encoding, negative, conf, images=images))
    return finish(r, s, frames)


def _run_hq_av(r, s):
    """ti2vid_hq_audio=True (--ti2vid-hq-audio; keyword-only) runs TI2VidHQPipeline with sound on the AudioVideo transformer: num_steps joint res_2s steps at half resolution, the video guided
    at cfg_scale and the audio at audio_cfg_scale, the x2 spatial upscale of the video (spatial_upscaler_weights is required, "random" for a random-initialised one), stage 1's audio latent
    re-noised, and 3 joint distilled steps, under distilled_lora when given; both stages run one C call per step (use_hip_graph has no effect on this route).  image_path sits at frame 0.  The negative encodings are Gemma's of `negative_prompt or ""` when Gemma encodes, else
    `negative_embedding` / `negative_audio_embedding` of the --embedding file, else zeros.  The audio latent is written to `<stem>_audio_latent.npz`; decode_audio turns it into `<stem>.wav`,
    muxed into the mp4, as in the av route.  Not combined with audio_path, two_stage_distilled, upscale_temporal, keyframes, retake_video or a2vid_two_stage, nor distilled_lora with
    fp8_resident.  pipeline_type="ti2vid-hq" without this flag stays the video-only run."""
    images = _image_conditions(r)
    print("\n=== Using TI2Vid HQ Pipeline (res_2s, audio + video) ===")
    _require(r, s)
    from ltx_2_mlx_amd.pipelines import TI2VidHQConfig, TI2VidHQPipeline
    conf = TI2VidHQConfig(height=r.height, width=r.width, num_frames=r.num_frames, seed=r.seed, num_inference_steps=r.num_steps,
                          cfg_scale=r.cfg_scale, audio_cfg_scale=r.audio_cfg_scale, distilled_lora_config=r.hq_lora, use_hip_graph=r.use_hip_graph,
                          tiling_config=_tiling(r), audio_enabled=True)
    _banners(r, upscaler=True)
    pipe = TI2VidHQPipeline(s.model, make_encoder(r), s.vae_decoder, _load_or_random(r, "spatial"))
    guided = r.cfg_scale > 1.0 or r.audio_cfg_scale > 1.0
    negative, negative_audio = s.negative_encoding, s.negative_audio_encoding
    if _negative_or_zeros_note(guided, negative):
        negative = torch.zeros_like(s.text_encoding)
    if _negative_or_zeros_note(guided, negative_audio):
        negative_audio = torch.zeros_like(s.text_audio_encoding)
    print(f"[5/5] Running TI2Vid HQ with audio ({r.num_steps} joint res_2s steps at {r.width // 2}x{r.height // 2}, then 3 at {r.width}x{r.height})...")
    frames, _ = _timed_run("ti2vid-hq audio+video", lambda: pipe(s.text_encoding, negative, conf, images=images, positive_audio_encoding=s.text_audio_encoding,
                                                                 negative_audio_encoding=negative_audio))
    return finish(r, s, frames, audio=decode_audio_latent(r, s, pipe.audio_latent))


def _run_two_stage_cfg(r, s):
    """two_stage_cfg=True (--two-stage-cfg; keyword-only) runs TwoStagePipeline, the reference's `--pipeline two-stage` on an AudioVideo checkpoint (reference :1276-1431): steps_stage1 joint
    steps at half resolution, each the positive prompt, the negative prompt and the modality-isolated pass, the video guided at `cfg_stage1 or cfg_scale`, the audio at audio_cfg_scale (default
    7), both at modality_scale (--modality-scale, default 3) and, with two_stage_rescale != 0, rescaled; the x2 spatial upscale of the video (spatial_upscaler_weights is required, "random"
    for a random-initialised one), stage 1's audio latent re-noised, and 3 joint distilled steps, under distilled_lora when given; both stages run one C call per step.  image_path sits at
    frame 0.  The negative encodings as in the hq_av route.  The audio latent is written to `<stem>_audio_latent.npz`; decode_audio turns it into `<stem>.wav`, muxed into the mp4, as in the av
    route.  Not combined with ti2vid_hq_audio, a2vid_two_stage, retake_video, keyframes, two_stage_distilled, upscale_temporal or audio_path, nor distilled_lora with fp8_resident.
    pipeline_type="two-stage" without this flag keeps its refusal."""
    images = _image_conditions(r)
    cfg = r.cfg_stage1 or r.cfg_scale
    print("\n=== Using Two-Stage Pipeline ===")
    print(f"  Stage 1: {r.steps_stage1} steps at {r.height // 2}x{r.width // 2} with CFG {cfg}")
    if r.guidance_rescale > 0:
        print(f"  Guidance rescale: {r.guidance_rescale}")
    print(f"  Stage 2: 3 steps at {r.height}x{r.width} (distilled refinement)")
    print("  Audio generation: ENABLED")
    _require(r, s)
    from ltx_2_mlx_amd.pipelines import TwoStageCFGConfig, TwoStagePipeline
    conf = TwoStageCFGConfig(height=r.height, width=r.width, num_frames=r.num_frames, seed=r.seed, num_inference_steps=r.steps_stage1, cfg_scale=cfg,
                             audio_cfg_scale=r.audio_cfg_scale, guidance_rescale=r.guidance_rescale, modality_scale=r.modality_scale,
                             rescale_scale=r.two_stage_rescale, distilled_lora_config=r.two_stage_lora, tiling_config=_tiling(r))
    _banners(r, upscaler=True)
    pipe = TwoStagePipeline(s.model, make_encoder(r), s.vae_decoder, _load_or_random(r, "spatial"))
    negative, negative_audio = s.negative_encoding, s.negative_audio_encoding
    if _negative_or_zeros_note(True, negative):
        negative = torch.zeros_like(s.text_encoding)
    if _negative_or_zeros_note(True, negative_audio):
        negative_audio = torch.zeros_like(s.text_audio_encoding)
    print(f"[5/5] Running the two-stage pipeline ({r.steps_stage1} guided joint steps at {r.width // 2}x{r.height // 2}, then 3 at {r.width}x{r.height})...")
    frames, _ = _timed_run("two-stage audio+video", lambda: pipe(s.text_encoding, negative, conf, images=images, positive_audio_encoding=s.text_audio_encoding,
                                                                 negative_audio_encoding=negative_audio))
    return finish(r, s, frames, audio=decode_audio_latent(r, s, pipe.audio_latent))


def _run_ic_lora(r, s):
    """pipeline_type="ic-lora" with control_video and / or image_path runs ICLoraPipeline (reference :1434-1549): the control video (a .npy / .npz array of uint8 frames, a directory of image
    frames, or a video file when an ffmpeg binary exists) is preprocessed on the device (control_type "canny": Canny edges between canny_low and canny_high, written with save_control to `<control
    video's base name>_canny.mp4` in output_path's directory; "raw": as it is), encoded and appended to the sequence at control_strength; stage 1 runs num_steps distilled steps at half resolution
    under ic_lora_weights (a LoRA file fused for that stage only), then the x2 spatial upscale and 3 refinement steps on the base weights; the image sits at frame 0 with image_strength.
    spatial_upscaler_weights is required ("random" for a random-initialised one).  Not combined with generate_audio, audio_path, two_stage_distilled, upscale_temporal or keyframes, nor
    ic_lora_weights with fp8_resident.  Without a control video and an image the pipeline_type raises NotImplementedError."""
    images = _image_conditions(r)
    print("\n=== Using IC-LoRA Pipeline ===")
    _require(r, s)
    from ltx_2_mlx_amd.pipelines import ControlType, ICLoraConfig, ICLoraPipeline, VideoCondition
    conf = ICLoraConfig(height=r.height, width=r.width, num_frames=r.num_frames, seed=r.seed, fps=24.0, stage_1_steps=r.num_steps,
                        use_hip_graph=r.use_hip_graph, tiling_config=_tiling(r))
    videos = []
    if r.control_video:
        print(f"  Control video: {r.control_video} (type={r.control_type}, strength={r.control_strength})")
        videos = [VideoCondition(video_path=r.control_video, strength=r.control_strength, control_type=ControlType(r.control_type),
                                 canny_low=r.canny_low, canny_high=r.canny_high, save_control=r.save_control)]
    if not r.ic_loras:
        print("  Warning: no --ic-lora-weights, stage 1 runs on the base weights")
    _banners(r, upscaler=True)
    pipe = ICLoraPipeline(s.model, make_encoder(r), s.vae_decoder, _load_or_random(r, "spatial"), lora_configs=r.ic_loras, save_video=save_video,
                          save_dir=r.output_dir or ".")
    print(f"[5/5] Running IC-LoRA ({r.num_steps} steps at {r.width // 2}x{r.height // 2}, then {conf.stage_2_steps} at {r.width}x{r.height})...")
    frames, _ = _timed_run("ic-lora", lambda: pipe(s.text_encoding, None, conf, images=images, video_conditioning=videos), tokens_of=pipe)
    return finish(r, s, frames)


def _run_retake(r, s):
    """retake_video (keyword-only; RetakePipeline, reference pipelines/retake.py, which the reference's own CLI never reaches): the source clip (a .npy / .npz array of uint8 frames or a directory
    of image frames, played at output_fps; a video file when ffmpeg and ffprobe exist, at its own frame rate) is kept and the seconds [retake_start_time, retake_end_time) of it are regenerated
    from the prompt (retake_end_time None: to the end of the clip, taken as half a frame past its last one, since int(num_frames / fps * fps) can fall one frame short).  The output is written at
    the source's rate: its frames enter ffmpeg at that rate and none is interpolated.  height, width and num_frames come from the source (frames snapped down to 8k + 1; the size must be divisible
    by 32, nothing is resized).  model_variant="distilled" runs the 8 distilled steps without guidance, any other variant LTX2Scheduler over num_steps with classifier-free guidance at cfg_scale
    (the negative encoding as for keyframes).  The window is widened to whole latent frames (8 pixel frames each; TemporalRegionMask); retake_composite puts the source's own frames back outside
    it, with a 4-frame fade.  Not combined with generate_audio, audio_path, keyframes, control_video, image_path, two_stage_distilled, upscale_spatial, upscale_temporal, fp8_resident or another
    pipeline_type."""
    print("\n=== Using Retake Pipeline ===")
    _require(r, s)
    from ltx_2_mlx_amd.pipelines import RetakeConfig, RetakePipeline
    distilled = r.model_variant == "distilled"
    conf = RetakeConfig(start_time=r.retake_start_time, end_time=r.retake_end_time, distilled=distilled, num_inference_steps=r.num_steps,
                        cfg_scale=r.cfg_scale, seed=r.seed, fps=r.retake_fps, use_hip_graph=r.use_hip_graph, composite_source=r.retake_composite,
                        tiling_config=_tiling(r))
    latent_frames = (r.num_frames - 1) // 8 + 1
    print(f"  Source: {r.retake_video}, {r.width}x{r.height}, {r.num_frames} frames @ {r.retake_fps:g} FPS")
    print(f"  Retake region: {r.retake_start_time:g}s - {'the end of the clip' if r.retake_to_end else f'{r.retake_end_time:g}s'} -> latent frames "
          f"[{r.retake_window[0]}, {r.retake_window[1]}) of {latent_frames}, {latent_frames * (r.height // 32) * (r.width // 32)} DiT tokens"
          + (", source frames kept outside it" if r.retake_composite else ""))
    _banners(r, upscaler=False)
    pipe = RetakePipeline(s.model, make_encoder(r), s.vae_decoder)
    _negative_or_zeros_note(not distilled and (r.cfg_scale > 1.0 or r.apg_guider is not None), s.negative_encoding)
    print(f"[5/5] Running retake ({'8 distilled steps' if distilled else f'{r.num_steps} steps, cfg {r.cfg_scale}'})...")
    guider = dict(guider=r.apg_guider) if r.apg_guider is not None else {}
    frames, _ = _timed_run("retake", lambda: pipe(r.retake_video, s.text_encoding, None, conf, negative_text_encoding=s.negative_encoding, **guider))
    return finish(r, s, frames, source_fps=r.retake_fps)


def _run_retake_av(r, s):
    """retake_video with retake_audio (both keyword-only): the silent route's retake (_run_retake: the clip, the window, the variants, the output at the source's rate) on the AudioVideo
    transformer, with the clip's sound track -- any file load_audio_file reads -- encoded by the audio VAE encoder and retaken over the same seconds as the picture: the audio tokens whose
    seconds meet the widened pixel window.  model_variant="distilled" runs the 8 joint distilled steps; any other variant LTX2Scheduler over num_steps with classifier-free guidance on both
    latents, the video at cfg_scale and the audio at retake_audio_cfg (None: cfg_scale), one HIP step per step in one captured graph.  The negative encodings as in the hq_av route.  The audio
    latent is written to `<stem>_audio_latent.npz`; decode_audio turns it into `<stem>.wav`, muxed into the mp4.  retake_composite puts the source's own frames back outside the window AND
    the source track's own samples (20 ms fade outside it).  Not combined with audio_path, keyframes, control_video, image_path, two_stage_distilled, upscale_spatial, upscale_temporal,
    fp8_resident, apg_scale or another pipeline_type."""
    print("\n=== Using Retake Pipeline (picture and sound) ===")
    _require(r, s)
    from ltx_2_mlx_amd.pipelines import RetakeConfig, RetakePipeline
    distilled = r.model_variant == "distilled"
    conf = RetakeConfig(start_time=r.retake_start_time, end_time=r.retake_end_time, distilled=distilled, num_inference_steps=r.num_steps,
                        cfg_scale=r.cfg_scale, seed=r.seed, fps=r.retake_fps, use_hip_graph=r.use_hip_graph, composite_source=r.retake_composite,
                        tiling_config=_tiling(r), audio_cfg_scale=r.retake_audio_cfg, composite_source_audio=r.retake_composite)
    latent_frames = (r.num_frames - 1) // 8 + 1
    print(f"  Source: {r.retake_video}, {r.width}x{r.height}, {r.num_frames} frames @ {r.retake_fps:g} FPS; sound track: {r.retake_audio}")
    print(f"  Retake region: {r.retake_start_time:g}s - {'the end of the clip' if r.retake_to_end else f'{r.retake_end_time:g}s'} -> latent frames "
          f"[{r.retake_window[0]}, {r.retake_window[1]}) of {latent_frames}, {latent_frames * (r.height // 32) * (r.width // 32)} DiT tokens"
          + (", source frames and samples kept outside it" if r.retake_composite else ""))
    _banners(r, upscaler=False)
    weights = r.weights_path if r.have_ckpt else None
    decoders = create_audio_decoders(r.decode_audio, weights, device=r.device, seed=r.seed + 3) or (None, None)
    pipe = RetakePipeline(s.model, make_encoder(r), s.vae_decoder, decoders[0], decoders[1], audio_encoder=create_audio_encoder(weights, r.device, seed=r.seed + 5))
    audio_cfg = r.cfg_scale if r.retake_audio_cfg is None else r.retake_audio_cfg
    guided = not distilled and (r.cfg_scale > 1.0 or audio_cfg > 1.0)
    negative, negative_audio = s.negative_encoding, s.negative_audio_encoding
    if _negative_or_zeros_note(guided, negative):
        negative = torch.zeros_like(s.text_encoding)
    if _negative_or_zeros_note(guided, negative_audio):
        negative_audio = torch.zeros_like(s.text_audio_encoding)
    print(f"[5/5] Running retake with sound ({'8 joint distilled steps' if distilled else f'{r.num_steps} joint steps, cfg {r.cfg_scale} / {audio_cfg}'})...")
    frames, audio = _timed_run("retake audio+video", lambda: pipe(r.retake_video, s.text_encoding, None, conf, negative_text_encoding=negative,
                                                                  audio_encoding=s.text_audio_encoding, negative_audio_encoding=negative_audio,
                                                                  audio_path=r.retake_audio))
    np.savez(s.base + "_audio_latent.npz", latent=pipe.audio_latent.float().cpu().numpy())
    print(f"  audio tokens [{pipe.audio_window[0]}, {pipe.audio_window[1]}) retaken" + (f", samples {list(pipe.audio_sample_window)} of the waveform" if decoders[0] else ""))
    return finish(r, s, frames, audio=(audio, decoders[1].output_sample_rate) if decoders[0] is not None else None, source_fps=r.retake_fps)


def _run_a2vid(r, s):
    """a2vid_two_stage=True (--a2vid-two-stage; keyword-only, the reference's own CLI never reaches pipelines/a2vid_two_stage.py) runs A2VidPipelineTwoStage on the AudioVideo transformer:
    audio_path (required; audio_start_time / audio_max_duration trim) is cut or right-padded with silence to num_frames / 25 seconds and encoded by the audio VAE encoder; the latent stays frozen
    through num_steps steps at half resolution with classifier-free guidance at cfg_scale on the video alone (model_variant="distilled" forces 1: the unguided captured loop), the x2 spatial
    upscale (spatial_upscaler_weights is required, "random" for a random-initialised one) and 3 distilled steps, under distilled_lora when given.  image_path sits at frame 0.  The negative
    encodings are Gemma's of `negative_prompt or ""` when Gemma encodes, else `negative_embedding` / `negative_audio_embedding` of the --embedding file, else zeros (video) and the positive
    audio encoding (audio, as the reference's loop falls back).  Written: the video, `<stem>_audio_latent.npz` (the frozen latent), and the ORIGINAL audio muxed into the mp4 when an ffmpeg
    binary exists.  Not combined with two_stage_distilled, upscale_temporal, keyframes, retake_video or control_video, nor distilled_lora with fp8_resident."""
    images = _image_conditions(r)
    print("\n=== Using A2Vid Two-Stage Pipeline ===")
    _require(r, s)
    from ltx_2_mlx_amd.pipelines import A2VidConfig, A2VidPipelineTwoStage
    conf = A2VidConfig(height=r.height, width=r.width, num_frames=r.num_frames, seed=r.seed, num_inference_steps=r.num_steps, cfg_scale=r.cfg_scale,
                       distilled_lora_config=r.a2vid_lora, use_hip_graph=r.use_hip_graph, tiling_config=_tiling(r), audio_start_time=r.audio_start_time,
                       audio_max_duration=r.audio_max_duration)
    _banners(r, upscaler=True)
    print(f"  Encoding audio: {r.audio_path}")
    latent, waveform, rate = encode_audio_for_video(r.audio_path, r.num_frames, conf.fps, r.weights_path if r.have_ckpt else None, device=r.device,
                                                    seed=r.seed + 5, start_time=r.audio_start_time, max_duration=r.audio_max_duration)
    pipe = A2VidPipelineTwoStage(s.model, make_encoder(r) if images else None, s.vae_decoder, _load_or_random(r, "spatial"))
    negative = s.negative_encoding
    if _negative_or_zeros_note(r.cfg_scale > 1.0, negative):
        negative = torch.zeros_like(s.text_encoding)
    print(f"[5/5] Running A2Vid ({r.num_steps} steps at {r.width // 2}x{r.height // 2}, cfg {r.cfg_scale}, then 3 at {r.width}x{r.height})...")
    frames, _ = _timed_run("a2vid two-stage", lambda: pipe(None, s.text_encoding, negative, conf, images=images, positive_audio_encoding=s.text_audio_encoding,
                                                           negative_audio_encoding=s.negative_audio_encoding, audio_latent=latent)[0], tokens_of=pipe)
    import shutil
    np.savez(s.base + "_audio_latent.npz", latent=pipe.audio_latent.float().cpu().numpy())
    wav = np.repeat(waveform, 2, axis=0) if waveform.shape[0] == 1 else waveform
    return finish(r, s, frames, audio=(wav, rate) if (r.save_mp4 and shutil.which("ffmpeg")) else None)


def _run_two_stage(r, s):
    """MI355X extra: two_stage_distilled=True runs the reference's DistilledPipeline class (pipelines/distilled.py:274-505), which the reference's own CLI never wires: 8 steps at half resolution,
    x2 latent upscale, 3 steps at full resolution, image conditioning at both resolutions, auto-tiled decode; with generate_audio on the AudioVideo transformer, the audio latent saved and decoded
    as in the av route."""
    images = _image_conditions(r)
    if not r.spatial_upscaler_weights:
        raise ValueError("two_stage_distilled needs --spatial-upscaler-weights (two-stage pipeline)")
    _require(r, s)
    from ltx_2_mlx_amd.pipelines import DistilledConfig, DistilledPipeline
    pipe = DistilledPipeline(s.model, make_encoder(r) if images else s.vae_decoder, s.vae_decoder, spatial_upscaler=_load_or_random(r, "spatial"))
    conf = DistilledConfig(height=r.height, width=r.width, num_frames=r.num_frames, seed=r.seed, fps=24.0, use_hip_graph=r.use_hip_graph,
                           audio_enabled=r.generate_audio, tiling_config=_tiling(r),
                           **(dict(sampler=r.sampler, ancestral_eta=r.ancestral_eta) if r.sampler == "euler_ancestral" else {}))
    print("[4/5] two-stage distilled pipeline (8 steps at half resolution, x2 upscale, 3 steps)" + (" with the audio branch" if r.av else ""))
    frames, audio_latent = _timed_run("two-stage", lambda: pipe(s.text_encoding, None, conf, images=images, audio_encoding=s.text_audio_encoding))
    return finish(r, s, frames, audio=decode_audio_latent(r, s, audio_latent) if audio_latent is not None else None)


def _run_av(r, s):
    """The AudioVideo route (reference :1638-1776): generate_audio=True or an LTX-2.3 checkpoint (always) runs the AudioVideo transformer through OneStagePipeline (fps 25, LTX2Scheduler over
    num_steps), guided for any cfg_scale / audio_cfg_scale != 1. The audio latent is always written to `<stem>_audio_latent.npz`; decode_audio (keyword-only) turns it into a waveform through
    AudioDecoder + the checkpoint's vocoder (create_vocoder_for_checkpoint) and writes `<stem>.wav`, muxed into the mp4 when an ffmpeg binary exists.  None decodes when the checkpoint holds
    `audio_vae.decoder.*` and `vocoder.*` tensors, True always (random-initialised decoders without them), False never. audio_path (keyword-only): the video is generated TO this audio file.  It is
    loaded (audio_start_time / audio_max_duration trim), cut or right-padded with silence to num_frames / fps seconds, turned into a log-mel and encoded by AudioEncoder; the latent stays frozen
    through the denoise loop (denoise_mask = 0, reference pipelines/a2vid_two_stage.py:338-357) and is written to `<stem>_audio_latent.npz`; the original audio, not a decode of the latent, is
    muxed into the mp4 when an ffmpeg binary exists."""
    images = _image_conditions(r)
    print("\n=== Using Audio-Video Pipeline ===")
    if not _require(r, s):
        return None
    if r.upscale_spatial:
        raise NotImplementedError("upscale_spatial with the AudioVideo pipeline (the reference's AV branch returns before its upscalers)")
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    av_pipeline = OneStagePipeline(transformer=s.model, video_encoder=make_encoder(r) if images else None, video_decoder=s.vae_decoder)
    av_config = OneStageCFGConfig(
        height=r.height, width=r.width, num_frames=r.num_frames, seed=r.seed,
        fps=25.0,  # matches the upstream frame_rate for the audio latent shape (reference :1704-1712)
        num_inference_steps=r.num_steps, cfg_scale=r.cfg_scale,
        audio_cfg_scale=r.audio_cfg_scale, rescale_scale=r.rescale_scale,
        audio_enabled=r.generate_audio, use_hip_graph=r.use_hip_graph, tiling_config=_tiling(r))
    given_audio = None
    if r.audio_path:
        print(f"  Encoding audio: {r.audio_path}")
        given_audio = encode_audio_for_video(r.audio_path, r.num_frames, av_config.fps, r.weights_path if r.have_ckpt else None, device=r.device,
                                             seed=r.seed + 5, start_time=r.audio_start_time, max_duration=r.audio_max_duration)
    stg = {}
    if r.stg_scale > 0:
        print(f"  STG guidance enabled (scale={r.stg_scale})")
        stg = dict(stg_scale=r.stg_scale, stg_blocks=r.stg_blocks, stg_cutoff=r.stg_cutoff)
    if r.stg_audio_scale > 0:
        stg.update(stg_audio_scale=r.stg_audio_scale, stg_blocks=r.stg_blocks, stg_cutoff=r.stg_cutoff)
    if r.sampler == "heun" or r.ge_gamma > 0:
        stg.update(sampler=r.sampler, ge_gamma=r.ge_gamma)
    if r.sampler == "euler_ancestral":
        stg.update(sampler=r.sampler, ancestral_eta=r.ancestral_eta)
    print(f"[5/5] Running audio-video generation ({r.num_steps} steps)...")
    frames, audio_latent = _timed_run("audio-video pipeline", lambda: av_pipeline(
        positive_encoding=s.text_encoding, negative_encoding=s.negative_encoding if r.need_cfg else None, config=av_config, images=images,
        positive_audio_encoding=s.text_audio_encoding, negative_audio_encoding=s.negative_audio_encoding if r.need_cfg else None,
        initial_audio_latent=given_audio[0] if given_audio else None, **(dict(guider_override=r.apg_guider) if r.apg_guider is not None else {}), **stg))
    if given_audio:
        # the frozen latent is kept; the ORIGINAL audio goes into the mp4 (the reference returns the original waveform, not a decode)
        import shutil
        np.savez(s.base + "_audio_latent.npz", latent=audio_latent.float().cpu().numpy())
        wav = np.repeat(given_audio[1], 2, axis=0) if given_audio[1].shape[0] == 1 else given_audio[1]
        return finish(r, s, frames, audio=(wav, given_audio[2]) if (r.save_mp4 and shutil.which("ffmpeg")) else None)
    return finish(r, s, frames, audio=decode_audio_latent(r, s, audio_latent) if audio_latent is not None else None)


def _first_block_cache_kw(r):
    """The keyword only when the cache is on: with it off the loop is called exactly as before."""
    return dict(first_block_cache=r.first_block_cache) if r.first_block_cache > 0 else {}


def _first_block_cache_report(r):
    if r.first_block_cache > 0:
        from ltx_2_mlx_amd.pipelines.common import first_block_cache_last_stats, first_block_cache_summary
        print("  " + first_block_cache_summary(first_block_cache_last_stats(), r.first_block_cache))


def _run_standard(r, s):
    """The standard route (one-stage, video-only; reference :1778-2095): the distilled sigma table (LTX2Scheduler for another variant) in one captured hipGraph, or eagerly with
    use_hip_graph=False, with image_path as an encoded frame 0, or as noise arithmetic in placeholder mode. upscale_spatial doubles the denoised latent before decoding (2W x 2H output);
    upscale_temporal doubles it in time (F -> 2F - 1 latent frames, after the spatial upscale when both are set; same output fps).  temporal_upscaler_checkpoint_semantics (keyword-only): False
    computes what the reference's TemporalUpscaler computes, True what the upstream PyTorch model does (see model/upscaler.py; which one the released weights want is not verified).
    `<stem>_latent.npz` holds the latent that is decoded; without a VAE decoder it is all there is.  cross_attn_scale != 1 scales the text cross-attention output of layers 40 and up
    (reference :1174-1176).  standard_cfg=True (--standard-cfg) runs the loop's guided branch instead (:1895-1976): see the branch below; everything after the loop is shared."""
    from ltx_2_mlx_amd.pipelines.common import capture_and_replay, decode_video
    device, model, vae_decoder = r.device, s.model, s.vae_decoder
    print("[4/5] latent noise")
    lf, lh, lw = (r.num_frames - 1) // 8 + 1, r.height // 32, r.width // 32
    g = torch.Generator(device=device).manual_seed(r.seed)
    latent = torch.randn(1, 128, lf, lh, lw, generator=g, device=device)
    sigmas = DISTILLED_SIGMA_VALUES[:r.num_steps + 1] if r.model_variant == "distilled" else \
        [float(x) for x in get_sigma_schedule(r.num_steps, distilled=False, latent=latent)]
    patchifier = VideoLatentPatchifier(patch_size=1)
    shape = VideoLatentShape(1, 128, lf, lh, lw)
    coords = patchifier.get_patch_grid_bounds(shape, device=device)
    positions = get_pixel_coords(coords, SpatioTemporalScaleFactors.default(), causal_fix=True).float()
    positions = torch.cat([positions[:, 0:1] / 24.0, positions[:, 1:]], dim=1)          # fps = 24 on the CLI path (:1823)
    print(f"[5/5] denoising ({len(sigmas) - 1} steps)")
    t0 = time.time()
    tok = patchifier.patchify(latent).contiguous()
    if r.cross_attn_scale != 1.0 and not r.use_placeholder:          # reference :1174-1176
        model.velocity_model.set_cross_attn_scale(r.cross_attn_scale, start_layer=40)
        print(f"  Applied cross-attention scale {r.cross_attn_scale}x for layers 40-{r.num_layers - 1}" if r.num_layers > 40 else
              f"  cross-attention scale {r.cross_attn_scale}x applies from layer 40 on: this model has {r.num_layers} layers, none is scaled")
    if r.use_placeholder:
        for i in range(len(sigmas) - 1):
            tok = tok + 0.1 * torch.randn_like(tok) * (sigmas[i + 1] - sigmas[i])
    elif r.route == "standard_cfg":
        # standard_cfg=True (--standard-cfg; keyword-only): the guided branch of the reference's standard loop (:1895-1976) for the dev video-only model: the positive and the negative prompt every
        # step, uncond + cfg_scale*(cond - uncond) on the x0 predictions and, with guidance_rescale > 0 (default 0.7), rescale_noise_cfg, each step one C call and the loop one captured graph.
        # The negative encoding is Gemma's of `negative_prompt or ""`, else `negative_embedding` of the --embedding file, else zeros.  model_variant="distilled" arrives here at cfg = 1: the plain loop
        from ltx_2_mlx_amd.pipelines.common import standard_cfg_denoise_loop
        from ltx_2_mlx_amd.types import LatentState
        negative = s.negative_encoding
        if _negative_or_zeros_note(r.cfg_scale > 1.0, negative):
            negative = torch.zeros_like(s.text_encoding)
        print(f"  Standard CFG loop: cfg={r.cfg_scale}" + (f", guidance rescale={r.guidance_rescale}" if r.cfg_scale > 1.0 and r.guidance_rescale > 0 else ""))
        st = LatentState(latent=tok, denoise_mask=torch.ones(1, tok.shape[1], 1, device=device), positions=positions, clean_latent=torch.zeros_like(tok))
        tok = standard_cfg_denoise_loop(model, st, sigmas, s.text_encoding, negative.to(device) if negative is not None else None, r.cfg_scale, r.guidance_rescale,
                                        use_hip_graph=r.use_hip_graph, **_first_block_cache_kw(r)).latent
        _first_block_cache_report(r)
    elif r.first_block_cache > 0:
        # first_block_cache > 0 on the plain route: the same loop at cfg = 1 (no negative prompt), every forward through cache slot 0, eager
        from ltx_2_mlx_amd.pipelines.common import standard_cfg_denoise_loop
        from ltx_2_mlx_amd.types import LatentState
        st = LatentState(latent=tok, denoise_mask=torch.ones(1, tok.shape[1], 1, device=device), positions=positions, clean_latent=torch.zeros_like(tok))
        tok = standard_cfg_denoise_loop(model, st, sigmas, s.text_encoding, None, 1.0, 0.0, use_hip_graph=r.use_hip_graph, **_first_block_cache_kw(r)).latent
        _first_block_cache_report(r)
    elif r.image_path:
        # image-to-video: encoded image replaces latent frame 0, its tokens keep (1 - strength) of the noise level
        from ltx_2_mlx_amd.conditioning import VideoLatentTools
        from ltx_2_mlx_amd.components import EulerDiffusionStep, GaussianNoiser
        from ltx_2_mlx_amd.pipelines import ImageCondition, apply_conditionings, create_image_conditionings, joint_denoise_loop
        tools = VideoLatentTools(patchifier, shape, fps=24.0)
        st = tools.create_initial_state(device=device)
        st = apply_conditionings(st, create_image_conditionings([ImageCondition(r.image_path, 0, r.image_strength)], make_encoder(r), r.height, r.width), tools)
        st = GaussianNoiser()(st, noise_scale=1.0, noise=tok)
        st, _ = joint_denoise_loop(model, False, st, None, sigmas, s.text_encoding, None, EulerDiffusionStep(), None, r.use_hip_graph)
        tok = st.latent
    elif r.use_hip_graph:
        vm = model.velocity_model
        vm.prepare(s.text_encoding, positions)
        lat2d = tok[0].float().contiguous()
        capture_and_replay(lambda: vm.capture_denoise_graph(lat2d, sigmas), vm.replay_denoise_graph)
        tok = lat2d[None]
    else:
        for i in range(len(sigmas) - 1):
            m = Modality(latent=tok, context=s.text_encoding, context_mask=None,
                         timesteps=torch.tensor([sigmas[i]], device=device), positions=positions, enabled=True)
            tok = euler_step_x0(tok, model(m), sigmas[i], sigmas[i + 1])
    torch.cuda.synchronize()
    print(f"  denoise: {(time.time() - t0):.3f} s")
    latent = patchifier.unpatchify(tok, shape)
    np.savez(s.base + "_latent.npz", latent=latent.float().cpu().numpy())

    def upscaled(latent, kind, upscale):
        """Post-denoise x2 latent upscale (reference :2000-2077): un-normalise with the VAE statistics, upscale, re-normalise.  Without a
        decoder there are no statistics: zeros / ones, with a warning.  The saved latent follows."""
        print(f"\nApplying 2x {kind} upscaling...\n  Input latent: {tuple(latent.shape)}")
        up = _load_or_random(r, kind)
        if vae_decoder is not None:
            stats = vae_decoder.per_channel_statistics
            latent = upscale(latent, up, stats.mean_of_means, stats.std_of_means)
        else:
            print("  WARNING: No VAE decoder for normalization - output may have wrong range")
            latent = upscale(latent, up, torch.zeros(128, device=device), torch.ones(128, device=device))
        print(f"  Upscaled latent: {tuple(latent.shape)}")
        np.savez(s.base + "_latent.npz", latent=latent.float().cpu().numpy())
        return latent

    import ltx_2_mlx_amd.model.upscaler as U
    if r.upscale_spatial and r.spatial_upscaler_weights:          # the decoded video is 2W x 2H
        latent = upscaled(latent, "spatial", U.upscale_latent)
    if r.upscale_temporal and r.temporal_upscaler_weights:        # F latent frames become 2F - 1, decoded to 8 * (2F - 2) + 1 video frames saved at the unchanged output fps (:2140)
        latent = upscaled(latent, "temporal", U.upscale_latent_temporal)
    if vae_decoder is None:
        print(f"Done in {time.time() - s.t_all:.1f} s: {s.base}_latent.npz")
        return None
    t0 = time.time()
    frames = _frames_from_video(decode_video(latent, vae_decoder, _tiling(r)))
    torch.cuda.synchronize()
    print(f"  decode: {(time.time() - t0):.3f} s -> {tuple(frames.shape)}")
    return finish(r, s, frames)


# today's precedence, top to bottom; _resolve_request names the one that runs
_ROUTES = {"two_stage_cfg": _run_two_stage_cfg, "hq_av": _run_hq_av, "a2vid": _run_a2vid, "keyframe": _run_keyframe, "hq": _run_hq, "ic_lora": _run_ic_lora, "retake_av": _run_retake_av,
           "retake": _run_retake, "two_stage": _run_two_stage,
           "av": _run_av, "standard": _run_standard, "standard_cfg": _run_standard}


def generate_video(
    prompt: str,
    height: int = 480,
    width: int = 704,
    num_frames: int = 97,
    num_steps: int = 7,
    cfg_scale: float = 5.0,
    guidance_rescale: float = 0.7,
    steps_stage1: int = 15,
    steps_stage2: int = 3,
    cfg_stage1=None,
    seed: int = 42,
    weights_path=None,
    output_path: str = "gens/output.mp4",
    use_placeholder: bool = False,
    skip_vae: bool = False,
    embedding_path=None,
    gemma_path: str = "weights/gemma-3-12b",
    use_gemma: bool = True,
    use_fp16: bool = True,
    use_fp8: bool = False,
    model_variant: str = "distilled",
    upscale_spatial: bool = False,
    spatial_upscaler_weights=None,
    upscale_temporal: bool = False,
    temporal_upscaler_weights=None,
    generate_audio: bool = False,
    low_memory: bool = False,
    fast_mode: bool = False,
    image_path=None,
    image_strength: float = 0.95,
    lora_path=None,
    lora_strength: float = 1.0,
    tiled_vae: bool = False,
    pipeline_type: str = "text-to-video",
    early_layers_only: bool = False,
    enhance_prompt_flag: bool = False,
    cross_attn_scale: float = 1.0,
    distilled_lora=None,
    distilled_lora_scale: float = 1.0,
    stg_scale: float = 0.0,
    stg_mode: str = "video",
    apg_scale: float = 1.0,
    apg_eta: float = 1.0,
    apg_norm_threshold: float = 0.0,
    apg_momentum: float = 0.0,
    control_video=None,
    control_type: str = "raw",
    canny_low: int = 100,
    canny_high: int = 200,
    control_strength: float = 0.95,
    save_control: bool = False,
    ge_gamma: float = 0.0,
    output_fps: int = 24,
    output_speed: float = 1.0,
    keyframes=None,
    ic_lora_weights=None,
    audio_cfg_scale=None,
    rescale_scale=None,
    negative_prompt=None,
    *,
    # MI355X additions (keyword-only; the reference has no counterpart)
    stg_blocks: Optional[List[int]] = None,        # with stg_scale: what OneStagePipeline takes beside it (the reference's CLI leaves them at these defaults)
    stg_cutoff: float = 1.0,
    stg_audio_scale: float = 0.0,                  # > 0: the AudioVideo route STG-guides the audio latent too (OneStagePipeline's stg_audio_scale; plain CFG or none)
    sampler: str = "euler",                       # "heun": OneStagePipeline's predictor-corrector loop (the reference's own CLI never reaches it); "euler_ancestral"
    ancestral_eta: float = 1.0,                    # with sampler="euler_ancestral": the noise scale of EulerAncestralDiffusionStep (0: the Euler step); the noise seed is `seed`
    use_hip_graph: bool = True,
    num_layers: int = 48,
    num_heads: int = 32,
    vae_base_channels=None,
    device: str = "cuda",
    text_features_path=None,
    save_mp4: bool = True,
    two_stage_distilled: bool = False,
    fp8_resident: bool = False,
    model_version=None,
    compute_dtype=None,
    fp8_compute: bool = False,
    decode_audio=None,
    temporal_upscaler_checkpoint_semantics: bool = False,
    audio_path=None,
    audio_start_time: float = 0.0,
    audio_max_duration=None,
    a2vid_two_stage: bool = False,
    ti2vid_hq_audio: bool = False,
    two_stage_cfg: bool = False,
    standard_cfg: bool = False,                    # the dev video-only model under CFG with the per-channel rescale: the guided branch of the reference's standard loop
    first_block_cache: float = 0.0,                # > 0: the video-only standard loops reuse the residual of blocks 1..L-1 where block 0's residual moved less than this threshold (eager loop)
    modality_scale: float = 3.0,
    two_stage_rescale: float = 0.0,
    retake_audio: Optional[str] = None,
    retake_audio_cfg: Optional[float] = None,
    retake_video=None,
    retake_start_time: float = 0.0,
    retake_end_time=None,
    retake_composite: bool = False,
):
    """Generate video from a text prompt: denoise loop + VAE decode on MI355X behind the reference's signature.  _resolve_request validates the arguments and names the one route that runs, before
    any model is loaded; then the text encoding, the transformer and the VAE decoder (built from the checkpoint's `config.vae` record) are loaded and the route's function runs.  Precedence, each
    documented on its function: standard_cfg (the guided branch of _run_standard; keyword-only, the dev video-only model under cfg_scale, guidance_rescale and cross_attn_scale, without conditioning), two_stage_cfg (_run_two_stage_cfg; keyword-only, with modality_scale and two_stage_rescale), ti2vid_hq_audio (_run_hq_av; keyword-only), a2vid_two_stage (_run_a2vid; keyword-only, it refuses retake_video), retake_video with retake_audio (_run_retake_av; keyword-only, the clip's sound track is retaken with the picture), retake_video (_run_retake; it refuses every other route), pipeline_type "keyframe-interpolation" with keyframes (_run_keyframe), "ti2vid-hq" (_run_hq), "ic-lora"
    with a control video or an image (_run_ic_lora), two_stage_distilled (_run_two_stage), generate_audio or an LTX-2.3 checkpoint (_run_av), else the standard video-only loop (_run_standard).
    pipeline_type "two-stage" raises NotImplementedError. MI355X extras for every route: model_version="2.3" builds the LTX-2.3 architecture without a checkpoint (random init, for tests and
    benchmarks); fp8_resident keeps fp8 checkpoint weights as codes in HBM; fp8_compute runs the video stream's projections fp8 x fp8 on the fp8 MFMA (BASELINE config 3; per-token / per-channel
    e4m3fn scales, not bit-identical to dequantise-at-load); vae_base_channels overrides the checkpoint's decoder_base_channels; compute_dtype="bfloat16" runs the bfloat16 build instead of the
    reference's float16 default (use_fp16=True).  Returns the uint8 frames (T, H, W, 3); None where the reference returns early."""
    r = _resolve_request(dict(locals()))
    if r is None:
        return None
    torch.manual_seed(r.seed)
    s = SimpleNamespace(t_all=time.time(), base=os.path.splitext(r.output_path)[0])
    s.text_encoding, s.text_audio_encoding, s.negative_encoding, s.negative_audio_encoding = _encode_text(r)
    s.model = _load_model(r, s.text_encoding)
    s.vae_decoder = _load_vae_decoder(r)
    return _ROUTES[r.route](r, s)


def build_parser() -> argparse.ArgumentParser:
    """Every flag of the reference's parser (scripts/generate.py:2364-2641: names, types, defaults, choices;
    tests/golden/generate_cli_flags.json), plus the MI355X extras at the end."""
    p = argparse.ArgumentParser(description="Generate video with LTX-2 on MI355X (denoise + VAE-decode hot path)")
    p.add_argument("prompt", type=str, help="Text prompt for generation")
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--width", type=int, default=704)
    p.add_argument("--frames", type=int, default=97)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--cfg", type=float, default=5.0, help="CFG scale (forced to 1.0 for the distilled model, as the reference does)")
    p.add_argument("--guidance-rescale", type=float, default=0.7)
    p.add_argument("--steps-stage1", type=int, default=15)
    p.add_argument("--steps-stage2", type=int, default=3)
    p.add_argument("--cfg-stage1", type=float, default=None)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--fps", type=int, default=24, help="output frame rate; > 24 interpolates")
    p.add_argument("--speed", type=float, default=1.0, help="playback speed multiplier")
    p.add_argument("--output", "-o", type=str, default="outputs/output.mp4")
    p.add_argument("--weights", type=str, default="weights/ltx-2/ltx-2-19b-distilled.safetensors")
    p.add_argument("--placeholder", action="store_true")
    p.add_argument("--skip-vae", action="store_true")
    p.add_argument("--embedding", type=str, default=None)
    p.add_argument("--gemma-path", type=str, default="weights/gemma-3-12b")
    p.add_argument("--no-gemma", action="store_true", help="dummy text embeddings")
    p.add_argument("--fp16", action="store_true", default=True, help="reference default: float16 operands (libltx2hip_f16.so), fp32 accumulate / residual stream; --bf16 selects the bfloat16 build")
    p.add_argument("--fp32", "--no-fp16", action="store_true", dest="fp32")
    p.add_argument("--fp8", action="store_true")
    p.add_argument("--model-variant", type=str, choices=["distilled", "dev"], default="distilled")
    p.add_argument("--distilled-lora", type=str, default=None)
    p.add_argument("--distilled-lora-scale", type=float, default=1.0)
    p.add_argument("--upscale-spatial", action="store_true")
    p.add_argument("--spatial-upscaler-weights", type=str, default="weights/ltx-2/ltx-2-spatial-upscaler-x2-1.0.safetensors")
    p.add_argument("--upscale-temporal", action="store_true")
    p.add_argument("--temporal-upscaler-weights", type=str, default="weights/ltx-2/ltx-2-temporal-upscaler-x2-1.0.safetensors")
    p.add_argument("--generate-audio", action="store_true")
    p.add_argument("--decode-audio", dest="decode_audio", action="store_true", default=None,
                   help="decode the audio latent to a .wav (muxed into the mp4 with ffmpeg); default: when the checkpoint holds the audio decoder "
                        "and vocoder, random-initialised decoders without a checkpoint")
    p.add_argument("--no-decode-audio", dest="decode_audio", action="store_false", help="keep only the audio latent (.npz)")
    p.add_argument("--low-memory", action="store_true")
    p.add_argument("--fast-mode", action="store_true")
    p.add_argument("--image", type=str, default=None)
    p.add_argument("--image-strength", type=float, default=0.95)
    p.add_argument("--lora", type=str, default=None)
    p.add_argument("--lora-strength", type=float, default=1.0)
    p.add_argument("--stg-scale", type=float, default=0.0)
    p.add_argument("--stg-mode", type=str, choices=["video", "audio", "both"], default="video")
    p.add_argument("--apg-scale", type=float, default=1.0)
    p.add_argument("--apg-eta", type=float, default=1.0)
    p.add_argument("--apg-norm-threshold", type=float, default=0.0)
    p.add_argument("--apg-momentum", type=float, default=0.0)
    p.add_argument("--ge-gamma", type=float, default=0.0)
    p.add_argument("--control-video", type=str, default=None)
    p.add_argument("--control-type", type=str, choices=["canny", "raw"], default="raw")
    p.add_argument("--canny-low", type=int, default=100)
    p.add_argument("--canny-high", type=int, default=200)
    p.add_argument("--control-strength", type=float, default=0.95)
    p.add_argument("--save-control", action="store_true")
    p.add_argument("--tiled-vae", action="store_true")
    p.add_argument("--pipeline", type=str, choices=list(_PIPELINES_CLI), default="text-to-video")
    p.add_argument("--keyframe", type=str, action="append", default=None)
    p.add_argument("--ic-lora-weights", type=str, default=None)
    p.add_argument("--early-layers-only", action="store_true")
    p.add_argument("--enhance-prompt", action="store_true")
    p.add_argument("--cross-attn-scale", type=float, default=1.0)
    # --- MI355X extras (no counterpart in the reference) ---
    p.add_argument("--text-features", type=str, default=None, help="npz with Gemma `features` [T,3840] (or `hidden_states` [L,T,3840]) + `attention_mask`: run the text connector on the GPU")
    p.add_argument("--no-hip-graph", action="store_true", help="run the step loop eagerly instead of replaying the captured hipGraph")
    p.add_argument("--ti2vid-hq", action="store_true", help="TI2VidHQPipeline (pipeline_type='ti2vid-hq'): --steps res_2s second-order steps at half resolution with "
                   "classifier-free guidance, x2 latent upscale (--spatial-upscaler-weights), 3 distilled steps, optionally under --distilled-lora.  An addition: "
                   "the reference ships this pipeline but its own command line never reaches it, so --pipeline keeps the reference's choices")
    p.add_argument("--two-stage-distilled", action="store_true", help="DistilledPipeline: 8 steps at half resolution, x2 latent upscale (--spatial-upscaler-weights), 3 steps")
    p.add_argument("--fp8-resident", action="store_true", help="keep fp8 checkpoint weights as codes in HBM (bit-identical to dequantising at load)")
    p.add_argument("--fp8-compute", action="store_true", help="BASELINE config 3: the video stream's projections fp8 x fp8 on the CDNA4 fp8 MFMA (per-token / per-channel e4m3fn scales; "
                   "an fp8 checkpoint's codes stay resident, a 16-bit checkpoint is quantised at load); --fp8 alone keeps the reference's dequantise-at-load arithmetic")
    p.add_argument("--bf16", action="store_true", help="bfloat16 operands instead of the reference's float16 default (both: fp32 accumulate / residual stream)")
    p.add_argument("--model-version", type=str, default=None, help="force the architecture family (e.g. 2.3) instead of reading the checkpoint metadata")
    p.add_argument("--layers", type=int, default=48, help="debug: number of DiT layers for random-weight runs")
    p.add_argument("--heads", type=int, default=32, help="debug: attention heads (x128) for random-weight runs")
    p.add_argument("--vae-base-channels", type=int, default=None, help="debug: override the checkpoint's decoder_base_channels")
    p.add_argument("--no-video-file", action="store_true", help="keep only the .npz outputs (skip ffmpeg / PNG frames)")
    p.add_argument("--audio", type=str, default=None, help="generate the video TO this audio file (with --generate-audio or an LTX-2.3 checkpoint): it is "
                   "encoded by the audio VAE encoder and stays frozen while the video is denoised; the original audio is muxed into the mp4")
    p.add_argument("--audio-start", type=float, default=0.0, help="seconds into --audio to start from")
    p.add_argument("--audio-duration", type=float, default=None, help="at most this many seconds of --audio (the rest of the video's length is silence)")
    p.add_argument("--ti2vid-hq-audio", action="store_true", help="TI2VidHQPipeline WITH sound on the AudioVideo model: --steps joint res_2s steps at half resolution (video guided "
                   "at --cfg, audio at audio_cfg_scale), x2 spatial upscale, 3 joint distilled steps; needs --spatial-upscaler-weights; --decode-audio writes the .wav. "
                   "(--ti2vid-hq / pipeline_type='ti2vid-hq' stays the video-only run and keeps refusing --generate-audio)")
    p.add_argument("--two-stage-cfg", action="store_true", help="TwoStagePipeline (the reference's --pipeline two-stage on an AudioVideo checkpoint): --steps-stage1 joint steps at half "
                   "resolution under CFG (video --cfg-stage1 or --cfg, audio 7) and modality-isolated guidance (--modality-scale), x2 spatial upscale, 3 joint distilled steps; needs "
                   "--spatial-upscaler-weights; --decode-audio writes the .wav.  (--pipeline two-stage itself keeps its refusal)")
    p.add_argument("--first-block-cache", type=float, default=0.0, metavar="T",
                   help="first-block cache of the video-only standard loops (plain and --standard-cfg): reuse the residual of blocks 1..L-1 on steps whose block-0 residual moved "
                        "less than T (relative L1); 0 is off.  The loop then runs eagerly.  Not verified with real weights")
    p.add_argument("--standard-cfg", action="store_true", help="the reference's standard one-stage loop for the dev video-only model (--model-variant dev): positive and negative prompt "
                   "every step, CFG at --cfg on the x0 predictions, the per-channel --guidance-rescale (default 0.7), --cross-attn-scale on layers 40-47; no conditioning "
                   "(--image is refused).  (--model-variant dev --cfg 3 without this flag keeps its refusal)")
    p.add_argument("--modality-scale", type=float, default=3.0, help="modality_scale of --two-stage-cfg: guidance away from the pass without audio<->video cross-attention")
    p.add_argument("--a2vid-two-stage", action="store_true", help="A2VidPipelineTwoStage: generate the video TO --audio at production quality on the AudioVideo model: --steps "
                   "steps at half resolution with classifier-free guidance on the video alone and the encoded audio frozen, x2 latent upscale "
                   "(--spatial-upscaler-weights), 3 distilled steps over the same frozen audio, optionally under --distilled-lora.  A flag of its own: "
                   "the reference ships this pipeline but its command line never reaches it, so --pipeline keeps the reference's choices")
    p.add_argument("--retake", type=str, default=None, help="RetakePipeline: keep this clip (.npy / .npz frames or an image directory at --fps; a video file with ffmpeg) "
                   "and regenerate the seconds --retake-start .. --retake-end of it from the prompt; size and length come from the clip.  --model-variant distilled: "
                   "8 steps, no guidance; dev: --steps steps at --cfg")
    p.add_argument("--retake-start", type=float, default=0.0, help="start of the regenerated window in seconds (inclusive)")
    p.add_argument("--retake-end", type=float, default=None, help="end of the regenerated window in seconds (exclusive); default: the end of the clip")
    p.add_argument("--retake-keep-source", action="store_true", help="put the source's own frames back outside the window (4-frame fade outside it)")
    p.add_argument("--retake-audio", type=str, default=None, help="with --retake: the clip's sound track (a .wav, or any file ffmpeg / soundfile reads); picture AND sound "
                   "are regenerated over the same seconds on the AudioVideo model; --decode-audio writes the .wav and muxes it; --retake-keep-source also puts the track's own "
                   "samples back outside the window")
    p.add_argument("--retake-audio-cfg", type=float, default=None, help="with --retake-audio: guidance scale of the audio latent (default: --cfg)")
    p.add_argument("--stg-blocks", type=int, nargs="+", default=None, help="with --stg-scale: the blocks whose video self-attention the perturbed pass skips (default: all)")
    p.add_argument("--stg-cutoff", type=float, default=1.0, help="with --stg-scale: STG guides the first fraction of the steps, (step + 1) / steps <= cutoff")
    p.add_argument("--stg-audio-scale", type=float, default=0.0,
                   help="AudioVideo route, plain CFG (rescale_scale=0) or no guidance (--model-variant distilled): STG-guide the audio latent too, at this scale (the perturbed pass then skips the audio "
                        "self-attention of --stg-blocks as well); with or without --stg-scale")
    p.add_argument("--sampler", type=str, choices=["euler", "heun", "euler_ancestral"], default="euler", help="on the AudioVideo route (OneStagePipeline): heun runs "
                   "the second-order predictor-corrector loop, two guided evaluations per step; --ge-gamma adds the GE velocity correction to either sampler; "
                   "euler_ancestral (also with --two-stage-distilled, stage 1) adds fresh noise per step, made in the step kernel from --seed")
    p.add_argument("--ancestral-eta", type=float, default=1.0, help="with --sampler euler_ancestral: the noise scale eta (1.0: the reference's step, 0: the Euler step)")
    return p


def kwargs_from_args(a) -> dict:
    """argparse namespace -> generate_video keywords, as the reference's main() maps them (:2644-2725), incl. its weight-file
    auto-selection for --model-variant dev / --fp8."""
    if a.model_variant == "dev":
        a.weights = a.weights.replace("distilled", "dev")
        if a.steps == 7:
            a.steps = 30
    if a.fp8 and ".safetensors" in a.weights and "-fp8" not in a.weights:
        a.weights = a.weights.replace(".safetensors", "-fp8.safetensors")
    return dict(
        distilled_lora=a.distilled_lora, distilled_lora_scale=a.distilled_lora_scale, prompt=a.prompt, height=a.height, width=a.width,
        num_frames=a.frames, num_steps=a.steps, cfg_scale=a.cfg, guidance_rescale=a.guidance_rescale, seed=a.seed, weights_path=a.weights,
        output_path=a.output, use_placeholder=a.placeholder, skip_vae=a.skip_vae, embedding_path=a.embedding, gemma_path=a.gemma_path,
        use_gemma=not a.no_gemma, use_fp16=not a.fp32, use_fp8=a.fp8, model_variant=a.model_variant, upscale_spatial=a.upscale_spatial,
        spatial_upscaler_weights=a.spatial_upscaler_weights, upscale_temporal=a.upscale_temporal,
        temporal_upscaler_weights=a.temporal_upscaler_weights, generate_audio=a.generate_audio, low_memory=a.low_memory, fast_mode=a.fast_mode,
        image_path=a.image, image_strength=a.image_strength, lora_path=a.lora, lora_strength=a.lora_strength, tiled_vae=a.tiled_vae,
        pipeline_type="ti2vid-hq" if a.ti2vid_hq else a.pipeline, early_layers_only=a.early_layers_only, enhance_prompt_flag=a.enhance_prompt, cross_attn_scale=a.cross_attn_scale,
        steps_stage1=a.steps_stage1, steps_stage2=a.steps_stage2, cfg_stage1=a.cfg_stage1, stg_scale=a.stg_scale, stg_mode=a.stg_mode,
        apg_scale=a.apg_scale, apg_eta=a.apg_eta, apg_norm_threshold=a.apg_norm_threshold, apg_momentum=a.apg_momentum,
        control_video=a.control_video, control_type=a.control_type, canny_low=a.canny_low, canny_high=a.canny_high,
        control_strength=a.control_strength, save_control=a.save_control, ge_gamma=a.ge_gamma, output_fps=a.fps, output_speed=a.speed,
        keyframes=a.keyframe, ic_lora_weights=a.ic_lora_weights,
        # MI355X extras
        text_features_path=a.text_features, use_hip_graph=not a.no_hip_graph, two_stage_distilled=a.two_stage_distilled,
        fp8_resident=a.fp8_resident, fp8_compute=a.fp8_compute, model_version=a.model_version, compute_dtype="bfloat16" if a.bf16 else None, num_layers=a.layers, num_heads=a.heads,
        vae_base_channels=a.vae_base_channels, save_mp4=not a.no_video_file, decode_audio=a.decode_audio,
        audio_path=a.audio, audio_start_time=a.audio_start, audio_max_duration=a.audio_duration, a2vid_two_stage=a.a2vid_two_stage, ti2vid_hq_audio=a.ti2vid_hq_audio,
        two_stage_cfg=a.two_stage_cfg, modality_scale=a.modality_scale, standard_cfg=a.standard_cfg, first_block_cache=a.first_block_cache,
        retake_audio=a.retake_audio, retake_audio_cfg=a.retake_audio_cfg,
        retake_video=a.retake, retake_start_time=a.retake_start, retake_end_time=a.retake_end, retake_composite=a.retake_keep_source,
        stg_blocks=a.stg_blocks, stg_cutoff=a.stg_cutoff, stg_audio_scale=a.stg_audio_scale, sampler=a.sampler, ancestral_eta=a.ancestral_eta)


def main(argv=None):
    generate_video(**kwargs_from_args(build_parser().parse_args(argv)))


if __name__ == "__main__":
    main()
