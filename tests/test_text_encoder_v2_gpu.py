"""The LTX-2.3 ("V2") text encoder on the MI355X: the `ltx2_gemma_features_rms` kernel, the feature extractor at the full K = 188 160,
the connectors at the LTX-2.3 widths, SPLIT RoPE and the assembled encoder against the reference's own vectors
(tests/golden/text_encoder_v2.npz, pinned by tools/pin_oracle_against_reference.py text_encoder_v2), and generate_video from a
prompt alone on a synthetic LTX-2.3 checkpoint.  Everything goes through the C ABI; torch on the GPU only runs the checker."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import measure, rel_l2  # noqa: E402
from test_parity import pearson  # noqa: E402

import gemma3_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# rel-L2 gates at no more than 5x the value measured on the MI355X:
FE_GATE = 1e-2              # feature extractor at K = 188 160: measured 2.38e-3 (M = 64 and M = 1024); 5x would be 1.19e-2, the toy-size
#                             test's 1e-2 is the cap
CONN8_GATE = 0.019          # 8 connector blocks: measured 4.21e-3 (video 32 x 128) and 3.97e-3 (audio 32 x 64); 5 x 3.97e-3 = 0.0198
GOLD = os.path.join(ROOT, "tests", "golden", "text_encoder_v2.npz")


def _ordered(x16: torch.Tensor) -> torch.Tensor:
    """16-bit floats as integers that count representable values in order (sign-magnitude -> a monotone scale), so that
    |a - b| is the distance in units in the last place."""
    i = x16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _hidden(layers, t, d, seed):
    """[L, T, D] fp32 hidden states: unit-scale rows with per-layer offsets, layer 3 scaled by 1e4 and layer 1 by 1e-4 (mean square
    1e-8, well under the 1e-6 in the rsqrt, so the epsilon decides that layer's scale)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(layers, t, d, generator=g) * (1 + 0.1 * torch.arange(layers, dtype=torch.float32)[:, None, None])
    x[3 % layers] *= 1e4
    x[1 % layers] *= 1e-4
    return x


def _mask(kind, t):
    m = torch.ones(t, dtype=torch.int32)
    pad = t // 3
    if kind == "left":
        m[:pad] = 0
    elif kind == "right":
        m[t - pad:] = 0
    return m


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("d,layers,t", [(3840, 49, 1), (3840, 49, 37), (3840, 49, 256), (64, 5, 37)])
def test_features_rms_kernel_within_one_ulp(d, layers, t, dtype):
    """ltx2_gemma_features_rms against oracle.text_connector.norm_and_concat_per_token_rms computed in fp32 and rounded once to the
    16-bit type.  Bound: one unit in the last place.  The kernel and the oracle both form x * rsqrt(mean(x^2) + 1e-6) in fp32; they
    differ by the summation order (a few fp32 ulps of the mean) and the rsqrt (1 fp32 ulp), i.e. by ~1e-6 relative before the one
    rounding to 8 or 11 significant bits, which can move the result across at most one rounding boundary.  Pad rows are exact zeros
    and two runs are bit-identical."""
    from oracle import text_connector as tc
    from ltx_2_mlx_amd import kernels as K
    x = _hidden(layers, t, d, seed=100 + t)
    xg = x.to(DEV)
    worst = 0
    for kind in ("left", "right", "all"):
        m = _mask(kind, t)
        ref = tc.norm_and_concat_per_token_rms(x.permute(1, 2, 0)[None], m[None])[0]         # [T, D * L], index d * L + l
        ref = ref.reshape(t, d, layers).permute(0, 2, 1).reshape(t, layers * d).to(dtype)      # layer-major, rounded once
        got = K.gemma_features_rms(xg, m.to(DEV), 1e-6, dtype=dtype)
        again = K.gemma_features_rms(list(xg.unbind(0)), m.to(DEV), 1e-6, dtype=dtype)
        torch.cuda.synchronize()
        assert got.shape == (t, layers * d) and got.dtype == dtype
        assert torch.equal(got.view(torch.int16), again.view(torch.int16))                     # deterministic, list of views == tensor
        got = got.cpu()
        assert torch.isfinite(got.float()).all()
        ulps = int((_ordered(got) - _ordered(ref)).abs().max())
        worst = max(worst, ulps)
        assert ulps <= 1, (kind, ulps)
        pad = m == 0
        if pad.any():
            assert torch.equal(got[pad].view(torch.int16), torch.zeros_like(got[pad]).view(torch.int16))     # +0, bit for bit
        # the epsilon matters on the near-zero layer: without it that layer would come out at unit RMS
        l0 = 1 % layers
        rms = got[~pad][:, l0 * d:(l0 + 1) * d].float().pow(2).mean().sqrt() if (~pad).any() else torch.tensor(0.0)
        assert (~pad).sum() == 0 or float(rms) < 0.2
    measure("features_rms max ulp distance", worst)


def test_features_rms_reads_sliced_views_and_stacks_loose_tensors():
    """The hidden states as Gemma3Model returns them -- views of one [L, T, D] buffer, trimmed to the real tokens -- are read in place;
    tensors that are not such views are stacked once.  Both give the same bits; bad arguments are ValueErrors."""
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    x = _hidden(7, 48, 256, seed=5).to(DEV)
    views = [x[l][-20:] for l in range(7)]
    assert K._layer_strides(views) == (48 * 256, 256)
    loose = [v.clone() for v in views]
    a, b = K.gemma_features_rms(views), K.gemma_features_rms(loose)
    assert torch.equal(a, b) and torch.equal(a, K.gemma_features_rms(x[:, -20:]))
    out = torch.empty(20, 7 * 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError):         # D not a multiple of 8
        nv.check(nv.lib().ltx2_gemma_features_rms(nv.ptr(x), 48 * 256, 256, None, nv.ptr(out), 7 * 252, 20, 7, 252, 1e-6, nv.stream()))
    with pytest.raises(ValueError):         # output rows narrower than L * D
        nv.check(nv.lib().ltx2_gemma_features_rms(nv.ptr(x), 48 * 256, 256, None, nv.ptr(out), 6 * 256, 20, 7, 256, 1e-6, nv.stream()))


@pytest.mark.parametrize("m", [64, 1024])
def test_feature_extractor_v2_full_k(m):
    """GemmaFeaturesExtractorV2 at D = 3840, L = 49 (K = 188 160), N = 4096 / 2048 against oracle.text_connector.feature_extractor_v2
    (fp32, run through torch on the GPU) on the same bf16-rounded weights.  Measured on the MI355X: rel-L2 2.38e-3 at M = 64 and
    2.38e-3 at M = 1024, video and audio alike (the bf16 rounding of the operand and of the sqrt(N / D)-scaled weights); gate FE_GATE.
    M = 64 takes the skinny GEMM route, M = 1024 the 128 x 128 tile route.  Pad rows equal the bias, bit for bit."""
    from oracle import text_connector as tc
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd.model.text_encoder import GemmaFeaturesExtractorV2
    d, layers, k = 3840, 49, 3840 * 49
    g = torch.Generator(device=DEV).manual_seed(7)
    sd = {}
    for name, n in (("video_aggregate_embed", 4096), ("audio_aggregate_embed", 2048)):
        sd[name + ".weight"] = (torch.randn(n, k, generator=g, device=DEV) / math.sqrt(k)).to(torch.bfloat16).float()
        sd[name + ".bias"] = 0.1 * torch.randn(n, generator=g, device=DEV)
    fe = GemmaFeaturesExtractorV2(device=DEV)
    fe.load_state_dict(sd)
    hidden = torch.randn(1, layers, m, d, generator=g, device=DEV) * (1 + 0.2 * torch.arange(layers, device=DEV)[None, :, None, None])
    states = [hidden[:, l] for l in range(layers)]
    mask = torch.ones(1, m, device=DEV)
    mask[:, :m // 4] = 0                       # left padding
    assert nv.lib().ltx2_gemm_route(m, 4096, k, nv.EPI_F32, 0, 0) == (nv.ROUTE_SKINNY if m <= 128 else nv.ROUTE_SMALL)
    video, audio = fe.extract_from_hidden_states(states, mask)
    rv, ra = tc.feature_extractor_v2(states, mask, sd)
    torch.cuda.synchronize()
    assert video.shape == (1, m, 4096) and audio.shape == (1, m, 2048)
    ev, ea = rel_l2(video.cpu(), rv.cpu()), rel_l2(audio.cpu(), ra.cpu())
    print(f"feature extractor V2, M = {m}: rel-L2 video {ev:.3e} audio {ea:.3e}")
    assert ev < FE_GATE and ea < FE_GATE, (ev, ea)
    assert torch.equal(video[0, :m // 4], sd["video_aggregate_embed.bias"].expand(m // 4, -1))
    assert torch.equal(audio[0, :m // 4], sd["audio_aggregate_embed.bias"].expand(m // 4, -1))


def _qw(w):
    return {k: (v.to(torch.bfloat16).float() if v.dim() == 2 and k != "learnable_registers" else v) for k, v in w.items()}


@pytest.mark.parametrize("blocks", [1, 8])
@pytest.mark.parametrize("heads,head_dim", [(32, 128), (32, 64)])
def test_connectors_at_ltx23_width(heads, head_dim, blocks):
    """Embeddings1DConnector at the LTX-2.3 widths (video 32 x 128 = 4096, audio 32 x 64 = 2048), gated attention, float64 frequency
    grid, INTERLEAVED RoPE, a 100-token prompt extended to 1024 rows, against oracle.text_connector.embeddings_connector on bf16-rounded
    matrices.  One block: the existing production-width gate (rel-L2 0.012, Pearson 0.999); measured 3.06e-3 (video) and 2.69e-3
    (audio).  Eight blocks: measured 4.21e-3 (video) and 3.97e-3 (audio), gate CONN8_GATE."""
    from oracle import text_connector as tc
    from ltx_2_mlx_amd.model.text_encoder import Embeddings1DConnector
    cfg = tc.ConnectorConfig(num_attention_heads=heads, attention_head_dim=head_dim, num_layers=blocks, apply_gated_attention=True,
                             double_precision_rope=True)
    w = tc.make_connector_weights(cfg, seed=81)
    conn = Embeddings1DConnector(attention_head_dim=head_dim, num_attention_heads=heads, num_layers=blocks, apply_gated_attention=True,
                                 double_precision_rope=True, device=DEV)
    conn.load_state_dict(w)
    x = torch.randn(1, 100, cfg.inner_dim, generator=torch.Generator().manual_seed(82))
    y, mk = conn(x.to(DEV))
    ref = tc.embeddings_connector(x, _qw(w), cfg)
    assert y.shape == (1, 1024, cfg.inner_dim) and float(mk.abs().max()) == 0.0 and torch.isfinite(y).all()
    e, r = rel_l2(y.cpu(), ref), pearson(y.cpu(), ref)
    print(f"connector {heads} x {head_dim}, {blocks} block(s): rel-L2 {e:.3e} Pearson {r:.6f}")
    assert e < (0.012 if blocks == 1 else CONN8_GATE) and r > 0.999, (e, r)


def _pin_inputs(z):
    """The seeded weights and hidden states of tests/golden/text_encoder_v2.npz, rebuilt from the seeds it stores (the recipe of
    tools/pin_oracle_against_reference.py v2_pin_inputs)."""
    from oracle import text_connector as tc
    c = dict(zip([str(k) for k in z["config_keys"]], [int(v) for v in z["config"]]))
    k = c["hidden"] * c["layers"]
    g = torch.Generator().manual_seed(c["seed_fe"])
    fe = {}
    for name, n in (("video_aggregate_embed", c["heads"] * c["video_head_dim"]), ("audio_aggregate_embed", c["heads"] * c["audio_head_dim"])):
        fe[name + ".weight"] = torch.randn(n, k, generator=g) / k ** 0.5
        fe[name + ".bias"] = 0.1 * torch.randn(n, generator=g)
    conn = {}
    for tag, hd, seed in (("video", c["video_head_dim"], c["seed_video"]), ("audio", c["audio_head_dim"], c["seed_audio"])):
        cfg = tc.ConnectorConfig(num_attention_heads=c["heads"], attention_head_dim=hd, num_layers=c["blocks"],
                                 num_learnable_registers=c["registers"], apply_gated_attention=True)
        conn[tag] = tc.make_connector_weights(cfg, seed=seed)
    g = torch.Generator().manual_seed(c["seed_hidden"])
    hs = [torch.randn(1, c["tokens"], c["hidden"], generator=g) * (1 + 0.5 * i) + 0.05 * i for i in range(c["layers"])]
    mask = torch.ones(1, c["tokens"])
    mask[:, :c["pad"]] = 0
    return c, fe, conn["video"], conn["audio"], hs, mask


@pytest.mark.parametrize("rope_type", ["interleaved", "split"])
def test_assembled_encoder_matches_the_reference(rope_type):
    """create_av_text_encoder_v2 (hidden 64, 5 layers, video 2 x 128, audio 2 x 64, 2 gated blocks, 16 registers) with INTERLEAVED and
    with SPLIT RoPE against the vectors the reference's own create_av_text_encoder_v2 gave on the same seeded weights and hidden states;
    gated like the connector_*_head / _tail vectors (rel-L2 0.008; measured 2.8e-3 head, 1.9e-3 tail for both types).  The two rotations differ by 2e-2 .. 3e-2 on the head rows of
    these inputs, so the wrong one fails."""
    from ltx_2_mlx_amd.model.text_encoder import create_av_text_encoder_v2
    z = np.load(GOLD)
    c, fe, wv, wa, hs, mask = _pin_inputs(z)
    enc = create_av_text_encoder_v2(hidden_dim=c["hidden"], num_gemma_layers=c["layers"], video_inner_dim=c["heads"] * c["video_head_dim"],
                                    audio_inner_dim=c["heads"] * c["audio_head_dim"], video_connector_heads=c["heads"],
                                    video_connector_head_dim=c["video_head_dim"], audio_connector_heads=c["heads"],
                                    audio_connector_head_dim=c["audio_head_dim"], connector_layers=c["blocks"], num_registers=c["registers"],
                                    rope_type=rope_type, connector_apply_gated_attention=True, double_precision_rope=True, device=DEV)
    enc.feature_extractor.load_state_dict(fe)
    enc.embeddings_connector.load_state_dict(wv)
    enc.audio_embeddings_connector.load_state_dict(wa)
    out = enc.encode_from_hidden_states([h.to(DEV) for h in hs], mask.to(DEV), padding_side="left")
    assert torch.equal(out.attention_mask.cpu(), torch.from_numpy(z[f"{rope_type}_mask"]))
    for mod, y in (("video", out.video_encoding.cpu()), ("audio", out.audio_encoding.cpu())):
        eh = rel_l2(y[:, :56], torch.from_numpy(z[f"{rope_type}_{mod}_head"]))
        et = rel_l2(y[:, 992:], torch.from_numpy(z[f"{rope_type}_{mod}_tail"]))
        print(f"assembled encoder, {rope_type} {mod}: rel-L2 head {eh:.3e} tail {et:.3e}")
        assert eh < 0.008 and et < 0.008, (rope_type, mod, eh, et)


WORDS = ["a", "red", "fox", "runs", "through", "the", "snow", "blurry", "low", "quality", "cat"]
HEADS = 2


@pytest.fixture(scope="module")
def gemma_dir(tmp_path_factory):
    """A 2-layer Gemma (hidden 256, 4 / 2 heads of 256) with a word-level tokenizer: (hidden, layers + 1) = (256, 3)."""
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Config
    d = tmp_path_factory.mktemp("gemma_v2")
    vocab = gemma3_ref.write_wordlevel_tokenizer(d, WORDS)
    cfg = Gemma3Config(vocab_size=len(vocab), num_hidden_layers=2, hidden_size=256, intermediate_size=512, num_attention_heads=4,
                       num_key_value_heads=2, head_dim=256, sliding_window=24)
    gemma3_ref.write_gemma_checkpoint(str(d), cfg, gemma3_ref.make_gemma3_weights(cfg, 11, device=DEV))
    return str(d)


@pytest.fixture(scope="module")
def ltx23_checkpoint(tmp_path_factory):
    """A synthetic LTX-2.3 checkpoint: metadata (model_version 2.3.0, the transformer record's connector settings, a small VAE), the
    V2 AudioVideo transformer blocks (2 heads, 2 layers), both aggregate embeds for a (256, 3) Gemma, two 8-block gated connectors."""
    from safetensors.torch import save_file
    from oracle import dit_av, vae
    from oracle import text_connector as tc
    blocks = [["res_x", {"num_layers": 1}], ["compress_all", {"multiplier": 2, "residual": True}], ["res_x", {"num_layers": 1}]]
    tensors = {k: v.contiguous() for k, v in vae.make_vae_weights(vae.VAEConfig(decoder_blocks=blocks, base_channels=32,
                                                                                 timestep_conditioning=False), 5).items()}
    cfg = dit_av.AVConfig(num_attention_heads=HEADS, attention_head_dim=128, audio_heads=HEADS, audio_head_dim=64, num_layers=2,
                          caption_channels=None, cross_attention_adaln=True, apply_gated_attention=True)
    tensors.update({"model.diffusion_model." + k: v.contiguous() for k, v in dit_av.make_av_weights(cfg, seed=6).items()})
    g = torch.Generator().manual_seed(9)
    k = 256 * 3
    for name, n in (("video_aggregate_embed", HEADS * 128), ("audio_aggregate_embed", HEADS * 64)):
        tensors[f"text_embedding_projection.{name}.weight"] = torch.randn(n, k, generator=g) / math.sqrt(k)
        tensors[f"text_embedding_projection.{name}.bias"] = 0.05 * torch.randn(n, generator=g)
    for tag, hd, seed in (("video", 128, 31), ("audio", 64, 32)):
        ccfg = tc.ConnectorConfig(num_attention_heads=HEADS, attention_head_dim=hd, num_layers=8, apply_gated_attention=True)
        tensors.update({f"model.diffusion_model.{tag}_embeddings_connector.{kk}": v.contiguous()
                        for kk, v in tc.make_connector_weights(ccfg, seed=seed).items()})
    meta = {"vae": {"decoder_blocks": blocks, "decoder_base_channels": 32, "timestep_conditioning": False},
            "transformer": {"connector_num_attention_heads": HEADS, "connector_attention_head_dim": 128, "connector_num_layers": 8,
                            "audio_connector_num_attention_heads": HEADS, "audio_connector_attention_head_dim": 64,
                            "connector_positional_embedding_max_pos": [4096], "rope_type": "interleaved",
                            "connector_apply_gated_attention": True, "frequencies_precision": "float64"}}
    ck = str(tmp_path_factory.mktemp("ltx23") / "ltx-2.3-synthetic.safetensors")
    save_file(tensors, ck, metadata={"model_version": "2.3.0", "config": json.dumps(meta)})
    return ck


def _spies(monkeypatch, generate):
    import ltx_2_mlx_amd.pipelines.common as common          # the pipelines' one final decode (decode_video) lives there
    seen = {"loads": 0, "latents": [], "batches": []}
    real_load, real_batch, real_decode = generate._load_gemma, generate.encode_av_gemma_batch, common.decode_latent

    def spy_load(*a, **k):
        seen["loads"] += 1
        return real_load(*a, **k)

    def spy_batch(prompts, *a, **k):
        out = real_batch(prompts, *a, **k)
        seen["batches"].append((list(prompts), out))
        return out

    def spy_decode(latent, *a, **k):
        seen["latents"].append(latent.detach().float().cpu().clone())
        return real_decode(latent, *a, **k)
    monkeypatch.setattr(generate, "_load_gemma", spy_load)
    monkeypatch.setattr(generate, "encode_av_gemma_batch", spy_batch)
    monkeypatch.setattr(common, "decode_latent", spy_decode)
    return seen


def test_generate_video_ltx23_from_a_prompt_alone(gemma_dir, ltx23_checkpoint, tmp_path, monkeypatch):
    """The README's LTX-2.3 line on a synthetic checkpoint: generate_video(prompt, weights_path=<2.3 file>, gemma_path=...) encodes the
    prompt with Gemma and the V2 encoder at the transformer's widths and writes the frames and the audio latent.  The same run from an
    --embedding file holding those encodings gives bit-identical video and audio latents.  (The AudioVideo branch needs a VAE decoder,
    as in the reference, so the checkpoint carries a small one; the video latent is taken where the pipeline hands it to the decoder.)"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    seen = _spies(monkeypatch, generate)
    kw = dict(height=64, width=96, num_frames=9, num_steps=2, seed=3, weights_path=ltx23_checkpoint, num_layers=2, num_heads=HEADS,
              save_mp4=False, generate_audio=True, decode_audio=False)
    frames = generate.generate_video("a red fox runs through the snow", gemma_path=gemma_dir, output_path=str(tmp_path / "p.mp4"), **kw)
    assert frames.shape == (3, 16, 24, 3) and frames.dtype == torch.uint8         # the checkpoint's small decoder: one x2 stage
    assert seen["loads"] == 1 and len(seen["batches"]) == 1 and len(seen["latents"]) == 1
    (pv, pa, pm), _ = seen["batches"][0][1]
    assert pv.shape == (1, 1024, HEADS * 128) and pa.shape == (1, 1024, HEADS * 64) and int(pm.sum()) == 1024
    assert torch.isfinite(pv).all() and torch.isfinite(pa).all()
    audio_a = np.load(tmp_path / "p_audio_latent.npz")["latent"]
    assert (tmp_path / "p.npz").exists() and np.isfinite(audio_a).all() and np.isfinite(seen["latents"][0].numpy()).all()
    # the same encodings through --embedding: bit-identical latents
    np.savez(tmp_path / "enc.npz", embedding=pv.cpu().numpy(), audio_embedding=pa.cpu().numpy())
    frames_b = generate.generate_video("a red fox runs through the snow", embedding_path=str(tmp_path / "enc.npz"),
                                       output_path=str(tmp_path / "q.mp4"), **kw)
    assert seen["loads"] == 1 and len(seen["latents"]) == 2
    assert torch.equal(seen["latents"][0], seen["latents"][1])
    assert np.array_equal(audio_a, np.load(tmp_path / "q_audio_latent.npz")["latent"])
    assert torch.equal(frames, frames_b)
    # a Gemma of another size than the checkpoint's aggregate embeds is refused with both shapes named
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Config
    with pytest.raises(ValueError, match=r"\(256, 4\).*\(256, 768\)"):
        generate._gemma_text_encoder(Gemma3Config(vocab_size=16, num_hidden_layers=3, hidden_size=256), ltx23_checkpoint, DEV)


def test_generate_video_ltx23_cfg_encodes_the_negative_prompt_under_one_load(gemma_dir, ltx23_checkpoint, tmp_path, monkeypatch):
    """model_variant="dev" with cfg_scale / audio_cfg_scale != 1 on the 2.3 checkpoint: prompt and negative prompt are encoded by the
    V2 encoder under ONE Gemma load."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    seen = _spies(monkeypatch, generate)
    frames = generate.generate_video("a red fox runs through the snow", gemma_path=gemma_dir, weights_path=ltx23_checkpoint,
                                     model_variant="dev", cfg_scale=3.0, audio_cfg_scale=5.0, negative_prompt="blurry low quality",
                                     output_path=str(tmp_path / "cfg.mp4"), height=64, width=96, num_frames=9, num_steps=2, seed=5,
                                     num_layers=2, num_heads=HEADS, save_mp4=False, generate_audio=True, decode_audio=False)
    assert frames.shape == (3, 16, 24, 3) and len(seen["latents"]) == 1 and torch.isfinite(seen["latents"][0]).all()
    assert (tmp_path / "cfg_audio_latent.npz").exists()
    assert seen["loads"] == 1 and seen["batches"][0][0] == ["a red fox runs through the snow", "blurry low quality"]
    (pv, pa, _), (nv_, na, _) = seen["batches"][0][1]
    assert nv_.shape == pv.shape == (1, 1024, HEADS * 128) and na.shape == pa.shape == (1, 1024, HEADS * 64)
    assert torch.isfinite(nv_).all() and torch.isfinite(na).all() and float((pv - nv_).abs().mean()) > 0


def test_generate_video_ltx23_random_init_without_a_checkpoint(gemma_dir, tmp_path, monkeypatch):
    """model_version="2.3" without a checkpoint: the V2 encoder is randomly initialised at the Gemma's (hidden, layers + 1) and the
    transformer's widths."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    seen = _spies(monkeypatch, generate)
    frames = generate.generate_video("a red fox", gemma_path=gemma_dir, weights_path=None, model_version="2.3", height=64, width=96,
                                     num_frames=9, num_steps=2, seed=5, num_layers=2, num_heads=HEADS, vae_base_channels=64, save_mp4=False,
                                     output_path=str(tmp_path / "r.mp4"))
    assert frames.shape == (9, 64, 96, 3)
    (pv, pa, _), _ = seen["batches"][0][1]
    assert pv.shape[-1] == HEADS * 128 and pa.shape[-1] == HEADS * 64
