"""Gemma-3 text encoder on the MI355X: the gemma.hip kernels against fp32 torch, the model against the reference's own output
(tests/golden/gemma3_tiny.npz, pinned by tools/pin_gemma_against_reference.py) and against the fp32 restatement (tests/gemma3_ref.py)
at production width, and the prompt-only generate_video path end to end.  Parity gates sit at <= 5x the value measured on the GPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import rel_l2  # noqa: E402

import gemma3_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
GOLD = os.path.join(ROOT, "tests", "golden", "gemma3_tiny.npz")


def _attn_ref(q, k, v, heads, kv_heads, causal, window):
    """fp32 torch: q [T, H*256], k / v [Tkv, Hkv*256] -> [T, H*256]; a row without visible keys -> 0."""
    tq, tkv = q.shape[0], k.shape[0]
    qh = q.float().reshape(tq, heads, 256).transpose(0, 1)
    kh = torch.repeat_interleave(k.float().reshape(tkv, kv_heads, 256).transpose(0, 1), heads // kv_heads, dim=0)
    vh = torch.repeat_interleave(v.float().reshape(tkv, kv_heads, 256).transpose(0, 1), heads // kv_heads, dim=0)
    s = (qh @ kh.transpose(-1, -2)) / 16.0
    if causal:
        i = torch.arange(tq, device=q.device)[:, None]
        j = torch.arange(tkv, device=q.device)[None, :]
        ok = j <= i
        if window:
            ok = ok & ((i - j) < window)
        s = s.masked_fill(~ok, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    return (p @ vh).transpose(0, 1).reshape(tq, heads * 256)


@pytest.mark.parametrize("t,heads,kv,causal,window", [
    (100, 4, 2, True, 0),          # T not a multiple of the 64-row tile
    (300, 4, 2, True, 48),         # window < T: tiles outside the window skipped, edge tiles masked
    (150, 16, 8, True, 1024),      # window >= T
    (1, 4, 2, True, 24),           # one valid row
    (130, 4, 2, False, 0),         # the attention_mask=None form: no mask
    (257, 2, 1, True, 64),         # ratio 2 with one kv head, window a tile multiple
])
def test_gemma_attn_matches_torch(t, heads, kv, causal, window):
    from ltx_2_mlx_amd import kernels as K
    g = torch.Generator(device=DEV).manual_seed(t + heads)
    qkv = torch.randn(t, (heads + 2 * kv) * 256, device=DEV, generator=g).to(BF)
    q, k, v = qkv[:, :heads * 256], qkv[:, heads * 256:(heads + kv) * 256], qkv[:, (heads + kv) * 256:]
    out = K.gemma_attn(q, k, v, heads, kv, causal=causal, window=window)
    out2 = K.gemma_attn(q, k, v, heads, kv, causal=causal, window=window)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, out2), "two launches differ"
    ref = _attn_ref(q, k, v, heads, kv, causal, window)
    err = rel_l2(out.float(), ref)
    assert err < 1e-2, err           # measured 1.9e-3 - 2.1e-3


def test_gemma_attn_fully_masked_rows_write_zeros():
    """The causal mask leaves no row of a prompt empty; a problem without keys does: every row is fully masked -> zeros, not NaN."""
    from ltx_2_mlx_amd import _native as nv
    q = torch.randn(70, 2 * 256, device=DEV).to(BF)
    kv = torch.randn(4, 256, device=DEV).to(BF)
    out = torch.full((70, 512), float("nan"), device=DEV, dtype=BF)
    nv.check(nv.lib().ltx2_gemma_attn(nv.ptr(q), 512, nv.ptr(kv), 256, nv.ptr(kv), 256, nv.ptr(out), 512, 70, 0, 2, 1, 1, 0, 1 / 16.0,
                                      nv.stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.float(), torch.zeros(70, 512, device=DEV))


def test_gemma_row_kernels_match_torch():
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import rope_cos_sin
    g = torch.Generator(device=DEV).manual_seed(7)
    t, h, kv, d, inter = 37, 4, 2, 768, 1024
    # per-head q / k norm + rotate-half RoPE, V columns untouched
    qkv = torch.randn(t, (h + 2 * kv) * 256, device=DEV, generator=g).to(BF)
    qw, kw = 0.3 * torch.randn(256, device=DEV, generator=g), 0.3 * torch.randn(256, device=DEV, generator=g)
    pos = torch.arange(100, 100 + t)
    cos, sin = rope_cos_sin(pos, 256, 1e6, 8.0)
    x = qkv.float()
    ref = x.clone()
    for lo, n, w in ((0, h, qw), (h * 256, kv, kw)):
        y = x[:, lo:lo + n * 256].reshape(t, n, 256)
        y = gemma3_ref.rms_norm(y, w, 1e-6).transpose(0, 1)
        ref[:, lo:lo + n * 256] = gemma3_ref.rope(y, pos.to(DEV), 1e6, 8.0).transpose(0, 1).reshape(t, n * 256)
    K.gemma_qknorm_rope_(qkv, h, kv, qw, kw, cos.to(DEV), sin.to(DEV))
    assert rel_l2(qkv.float(), ref) < 5e-3                           # bf16 rounding: measured 1.4e-3
    assert torch.equal(qkv[:, (h + kv) * 256:].float(), x[:, (h + kv) * 256:])
    # residual + post-norm + next pre-norm
    xin = torch.randn(t, d, device=DEV, generator=g)
    y = torch.randn(t, d, device=DEV, generator=g).to(BF)
    wp, wn = 0.5 * torch.randn(d, device=DEV, generator=g), 0.5 * torch.randn(d, device=DEV, generator=g)
    xo, hb, hf = torch.empty(t, d, device=DEV), torch.empty(t, d, device=DEV, dtype=BF), torch.empty(t, d, device=DEV)
    K.gemma_resid_norm(xin, y, wp, wn, x_out=xo, h_out=hb, hf_out=hf)
    xr = xin + gemma3_ref.rms_norm(y.float(), wp, 1e-6)
    nr = gemma3_ref.rms_norm(xr, wn, 1e-6)
    assert rel_l2(xo, xr) < 3e-7                                     # measured 5.5e-8
    assert rel_l2(hf, nr) < 4e-7                                     # measured 8.1e-8
    assert rel_l2(hb.float(), nr) < 5e-3                             # bf16 rounding: measured 1.7e-3
    K.gemma_resid_norm(xin, None, None, wn, hf_out=hf)
    assert rel_l2(hf, gemma3_ref.rms_norm(xin, wn, 1e-6)) < 3e-7     # measured 5.7e-8
    # gated activations, both
    gu = torch.randn(t, 2 * inter, device=DEV, generator=g).to(BF)
    for act, kind in ((0, "silu"), (1, "gelu_pytorch_tanh")):
        out = K.gemma_gated_act(gu, inter, act)
        ref = gemma3_ref.act(gu[:, :inter].float(), kind) * gu[:, inter:].float()
        assert rel_l2(out.float(), ref) < 5e-3, kind                 # measured 1.7e-3
    # embedding gather * sqrt(hidden)
    table = torch.randn(50, d, device=DEV, generator=g).to(BF)
    ids = torch.tensor([3, 0, 49, 7], device=DEV, dtype=torch.int32)
    e = K.gemma_embed(ids, table, d ** 0.5)
    assert torch.equal(e, table[ids.long()].float() * torch.tensor(d ** 0.5, dtype=torch.float32))


def _tiny_config(**kw):
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Config
    z = np.load(GOLD)
    d = dict(zip([str(k) for k in z["config_keys"]], [int(v) for v in z["config"]]))
    d.update(kw)
    return Gemma3Config(**d)


def _model(cfg, w):
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Model
    m = Gemma3Model(cfg, device=DEV)
    m.load_state_dict(w)
    return m


def test_gemma3_tiny_model_matches_golden_and_restatement():
    z = np.load(GOLD)
    cfg = _tiny_config()
    w = gemma3_ref.make_gemma3_weights(cfg, int(z["seed"]))
    m = _model(cfg, w)
    ids, mask = torch.from_numpy(z["input_ids"]).long(), torch.from_numpy(z["attention_mask"]).long()
    last, states = m(ids, attention_mask=mask)
    torch.cuda.synchronize()
    assert len(states) == 7 and last.shape == (1, 64, 256)
    valid = mask[0].bool()
    gold = torch.from_numpy(z["hidden_states"])
    got = torch.stack([s[0, valid.to(DEV)].cpu() for s in states])
    assert all(torch.equal(s[0, ~valid.to(DEV)].cpu(), torch.zeros(int((~valid).sum()), 256)) for s in states)   # padded rows zero
    err_gold = rel_l2(got, gold)
    assert err_gold < 5e-2, err_gold      # measured 1.0e-2 (bf16 weights against the reference's fp32)
    ref = gemma3_ref.forward(ids, gemma3_ref.bf16_weights(w), cfg, attention_mask=mask)
    err_ref = rel_l2(got, torch.stack([s[0, valid] for s in ref]))
    assert err_ref < 3.5e-2, err_ref      # measured 7.6e-3


def _production(layers, vocab=1024, seed=0):
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Config
    cfg = Gemma3Config(vocab_size=vocab, num_hidden_layers=layers)
    w = gemma3_ref.round_bf16_(gemma3_ref.make_gemma3_weights(cfg, seed, device=DEV))
    return cfg, w


@pytest.mark.parametrize("t,valid", [(1024, 1024), (1024, 300), (1280, 1280)])
def test_gemma3_production_width_six_layers(t, valid):
    cfg, w = _production(6)
    m = _model(cfg, w)
    g = torch.Generator().manual_seed(t + valid)
    ids = torch.randint(0, cfg.vocab_size, (1, t), generator=g)
    mask = torch.zeros(1, t, dtype=torch.long)
    mask[:, t - valid:] = 1
    _, states = m(ids, attention_mask=mask)
    with torch.no_grad():
        ref = gemma3_ref.forward(ids[:, t - valid:], w, cfg, attention_mask=torch.ones(1, valid, dtype=torch.long),
                                 positions=torch.arange(t - valid, t))
    got = torch.stack([s[0, t - valid:] for s in states])
    assert torch.isfinite(got).all()
    err = rel_l2(got, torch.stack([s[0] for s in ref]))
    assert err < 3.5e-2, err              # measured 6.9e-3 - 7.3e-3
    if valid < t:
        assert float(torch.stack([s[0, :t - valid] for s in states]).abs().max()) == 0.0


def test_gemma3_48_layers_finite_and_matches_restatement():
    cfg, w = _production(48)
    m = _model(cfg, w)
    t = 128
    ids = torch.randint(0, cfg.vocab_size, (1, t), generator=torch.Generator().manual_seed(48))
    mask = torch.ones(1, t, dtype=torch.long)
    _, states = m(ids, attention_mask=mask)
    del m
    with torch.no_grad():
        ref = gemma3_ref.forward(ids, w, cfg, attention_mask=mask)
    got = torch.stack([s[0] for s in states])
    assert len(states) == 49 and torch.isfinite(got).all()
    err = rel_l2(got, torch.stack([s[0] for s in ref]))
    assert err < 6e-2, err                # measured 1.2e-2


WORDS = ["a", "red", "fox", "runs", "through", "the", "snow", "blurry", "low", "quality", "cat"]


@pytest.fixture(scope="module")
def gemma_dir(tmp_path_factory):
    """Production-width (3840 hidden, 16 / 8 x 256 heads, 15360 intermediate), 6-layer, small-vocabulary Gemma checkpoint + tokenizer."""
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Config
    d = tmp_path_factory.mktemp("gemma")
    vocab = gemma3_ref.write_wordlevel_tokenizer(d, WORDS)
    cfg = Gemma3Config(vocab_size=len(vocab), num_hidden_layers=6)
    w = gemma3_ref.make_gemma3_weights(cfg, 11, device=DEV)
    gemma3_ref.write_gemma_checkpoint(str(d), cfg, w)
    del w
    torch.cuda.empty_cache()
    return str(d)


def test_generate_video_from_a_prompt_alone(gemma_dir, tmp_path, monkeypatch):
    """generate_video(prompt, gemma_path=...) with no embedding file: Gemma encodes on the GPU and the frames come out; the context
    the DiT received is encode_with_gemma's."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    used = {}
    real_encode = generate.encode_with_gemma

    def spy_encode(*a, **k):
        used["ctx"] = real_encode(*a, **k)
        return used["ctx"]
    real_load = generate.load_transformer

    def spy_load(*a, **k):
        used["caption_channels"] = k.get("caption_channels")
        return real_load(*a, **k)
    monkeypatch.setattr(generate, "encode_with_gemma", spy_encode)
    monkeypatch.setattr(generate, "load_transformer", spy_load)
    kw = dict(height=256, width=384, num_frames=17, num_steps=2, seed=3, num_layers=2, num_heads=2, vae_base_channels=64, save_mp4=False)
    frames = generate.generate_video("a red fox runs through the snow", gemma_path=gemma_dir, weights_path=None,
                                     output_path=str(tmp_path / "fox.mp4"), **kw)
    assert frames.shape == (17, 256, 384, 3) and frames.dtype == torch.uint8
    assert used["caption_channels"] == 3840
    direct, mask = real_encode("a red fox runs through the snow", gemma_dir, None, seed=3)
    assert torch.equal(used["ctx"][0], direct) and torch.equal(used["ctx"][1], mask)
    assert torch.isfinite(direct).all() and direct.shape[-1] == 3840
    # a nonexistent gemma_path keeps the reference's message and return
    assert generate.generate_video("x", gemma_path=str(tmp_path / "nowhere"), weights_path=None, **kw) is None
    # negative_prompt stays refused with a pre-computed encoding
    np.savez(tmp_path / "e.npz", embedding=np.zeros((8, 3840), np.float32))
    with pytest.raises(NotImplementedError, match="negative_prompt"):
        generate.generate_video("x", embedding_path=str(tmp_path / "e.npz"), negative_prompt="blurry", weights_path=None, **kw)


def test_generate_video_audio_video_cfg_encodes_the_negative_prompt(gemma_dir, tmp_path, monkeypatch):
    """The AudioVideo branch with cfg_scale != 1 takes its negative encodings from Gemma: prompt and negative prompt under ONE load."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    loads, batches = [], []
    real_load, real_batch = generate._load_gemma, generate.encode_av_gemma_batch

    def spy_load(*a, **k):
        loads.append(a[0])
        return real_load(*a, **k)

    def spy_batch(prompts, *a, **k):
        batches.append(list(prompts))
        out = real_batch(prompts, *a, **k)
        batches.append(out)
        return out
    monkeypatch.setattr(generate, "_load_gemma", spy_load)
    monkeypatch.setattr(generate, "encode_av_gemma_batch", spy_batch)
    frames = generate.generate_video("a red fox runs through the snow", gemma_path=gemma_dir, weights_path=None, generate_audio=True,
                                     model_variant="dev", cfg_scale=3.0, negative_prompt="blurry low quality",
                                     output_path=str(tmp_path / "av.mp4"), height=256, width=384, num_frames=17, num_steps=2, seed=5,
                                     num_layers=2, num_heads=2, vae_base_channels=64, save_mp4=False)
    assert frames.shape == (17, 256, 384, 3)
    assert len(loads) == 1 and batches[0] == ["a red fox runs through the snow", "blurry low quality"]
    (pv, pa, pm), (nv_, na, nm) = batches[1]
    assert pv.shape[-1] == nv_.shape[-1] == 3840 and torch.isfinite(nv_).all() and torch.isfinite(na).all()
    assert float((pv - nv_).abs().mean()) > 0          # the negative prompt was encoded, not copied
