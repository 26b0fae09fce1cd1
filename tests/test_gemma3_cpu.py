"""Gemma-3 text encoder, host side (no GPU): the fp32 restatement (tests/gemma3_ref.py) against the reference's own output
(tests/golden/gemma3_tiny.npz) and against HF's Gemma3TextModel, the valid-run compaction, the loader's key mapping and config.json
parsing, the tokenizer path, and the GEMM routes of the Gemma shapes."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemma3_ref  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "gemma3_tiny.npz")


def _tiny():
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Config
    z = np.load(GOLD)
    return Gemma3Config(**dict(zip([str(k) for k in z["config_keys"]], [int(v) for v in z["config"]]))), z


def test_restatement_matches_reference_golden():
    cfg, z = _tiny()
    assert cfg.head_dim == 256 and cfg.layer_types[5] == "full_attention" and cfg.sliding_window < int(z["attention_mask"].sum())
    w = gemma3_ref.make_gemma3_weights(cfg, int(z["seed"]))
    ids, mask = torch.from_numpy(z["input_ids"]).long(), torch.from_numpy(z["attention_mask"]).long()
    states = gemma3_ref.forward(ids, w, cfg, attention_mask=mask)
    valid = mask[0].bool()
    got = torch.stack([s[0, valid] for s in states])
    gold = torch.from_numpy(z["hidden_states"])
    assert got.shape == gold.shape == (7, 40, 256)
    assert float((got - gold).norm() / gold.norm()) < 1e-5


def test_padded_and_compacted_valid_rows_agree():
    """Left padding: the valid rows computed inside the padded sequence equal the valid rows computed alone at their absolute positions
    (what Gemma3Model runs)."""
    cfg, z = _tiny()
    w = gemma3_ref.make_gemma3_weights(cfg, 5)
    ids, mask = torch.from_numpy(z["input_ids"]).long(), torch.from_numpy(z["attention_mask"]).long()
    t, n = ids.shape[1], int(mask.sum())
    full = gemma3_ref.forward(ids, w, cfg, attention_mask=mask)
    comp = gemma3_ref.forward(ids[:, t - n:], w, cfg, attention_mask=torch.ones(1, n, dtype=torch.long), positions=torch.arange(t - n, t))
    for a, b in zip(full, comp):
        assert float((a[0, t - n:] - b[0]).norm() / b[0].norm()) < 1e-5


def test_restatement_gelu_mode_matches_hf_gemma3():
    transformers = pytest.importorskip("transformers")
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Config
    hc = transformers.Gemma3TextConfig(
        vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=6, num_attention_heads=4, num_key_value_heads=2,
        head_dim=256, sliding_window=24, query_pre_attn_scalar=256, hidden_activation="gelu_pytorch_tanh", attn_implementation="eager",
        rope_parameters={"full_attention": {"rope_type": "linear", "factor": 8.0, "rope_theta": 1e6},
                         "sliding_attention": {"rope_type": "default", "rope_theta": 1e4}})
    cfg = Gemma3Config.from_dict(hc.to_dict(), hidden_activation="gelu_pytorch_tanh")
    assert cfg.full_rope_scaling_factor == 8.0 and cfg.sliding_rope_theta == 1e4 and cfg.layer_types == hc.layer_types
    m = transformers.Gemma3TextModel(hc).eval()
    w = gemma3_ref.make_gemma3_weights(cfg, 3)
    m.load_state_dict(w, strict=True)
    ids = torch.randint(0, 512, (1, 40), generator=torch.Generator().manual_seed(0))       # 40 > window 24
    mask = torch.ones(1, 40, dtype=torch.long)
    with torch.no_grad():
        hs = m(input_ids=ids, attention_mask=mask, output_hidden_states=True).hidden_states
    ref = gemma3_ref.forward(ids, w, cfg, attention_mask=mask)
    assert len(hs) == len(ref) == 7
    for a, b in zip(hs, ref):
        assert float((a - b).norm() / b.norm()) < 1e-5


def test_noncontiguous_mask_is_refused_and_runs_are_found():
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import valid_run
    assert valid_run(torch.tensor([0, 0, 1, 1, 1])) == (2, 3)          # left padding
    assert valid_run(torch.tensor([1, 1, 0])) == (0, 2)                # right padding
    assert valid_run(torch.ones(4)) == (0, 4)                          # none
    with pytest.raises(ValueError, match="contiguous"):
        valid_run(torch.tensor([1, 0, 1, 1]))


def test_model_refuses_cpu():
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Model
    with pytest.raises(RuntimeError):
        Gemma3Model(device="cpu")


def _write_checkpoint(path, cfg, prefix, drop=None, extra=None):
    from safetensors.torch import save_file
    w = gemma3_ref.make_gemma3_weights(cfg, 0)
    sd = {prefix + k: v.to(torch.bfloat16) for k, v in w.items() if k != drop}
    if extra:
        sd.update(extra)
    keys = sorted(sd)
    half = len(keys) // 2
    os.makedirs(path, exist_ok=True)
    save_file({k: sd[k].contiguous() for k in keys[:half]}, os.path.join(path, "model-00001-of-00002.safetensors"))
    save_file({k: sd[k].contiguous() for k in keys[half:]}, os.path.join(path, "model-00002-of-00002.safetensors"))


def test_loader_key_mapping_config_json_and_errors(tmp_path):
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Config, checkpoint_key_to_name, scan_gemma3_checkpoint
    assert checkpoint_key_to_name("language_model.model.layers.3.mlp.up_proj.weight") == "layers.3.mlp.up_proj.weight"
    assert checkpoint_key_to_name("model.layers.0.self_attn.q_norm.weight") == "layers.0.self_attn.q_norm.weight"
    assert checkpoint_key_to_name("model.language_model.norm.weight") == "norm.weight"
    assert checkpoint_key_to_name("vision_tower.vision_model.embeddings.patch_embedding.weight") is None
    with pytest.raises(KeyError, match="something.weight"):
        checkpoint_key_to_name("something.weight")
    # config.json: the multimodal form (text_config) with the older rope fields, and the text-only form with per-type rope_parameters
    cfg = Gemma3Config.from_dict({"text_config": {"hidden_size": 256, "intermediate_size": 512, "num_hidden_layers": 6, "num_attention_heads": 4,
                                                  "num_key_value_heads": 2, "head_dim": 256, "vocab_size": 64, "sliding_window": 24,
                                                  "rope_theta": 1e6, "rope_local_base_freq": 1e4, "sliding_window_pattern": 6,
                                                  "rope_scaling": {"rope_type": "linear", "factor": 8.0}, "hidden_activation": "gelu_pytorch_tanh"}})
    assert (cfg.hidden_size, cfg.num_hidden_layers, cfg.vocab_size, cfg.sliding_window) == (256, 6, 64, 24)
    assert cfg.layer_types == ["sliding_attention"] * 5 + ["full_attention"] and cfg.full_rope_scaling_factor == 8.0
    assert cfg.hidden_activation == "silu"           # the activation is the caller's choice, never the file's
    d = tmp_path / "gemma"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"hidden_size": 256, "intermediate_size": 512, "num_hidden_layers": 6, "num_attention_heads": 4,
                                               "num_key_value_heads": 2, "head_dim": 256, "vocab_size": 64, "sliding_window": 24,
                                               "layer_types": cfg.layer_types,
                                               "rope_parameters": {"full_attention": {"rope_type": "linear", "factor": 8.0, "rope_theta": 1e6},
                                                                   "sliding_attention": {"rope_type": "default", "rope_theta": 1e4}}}))
    cfg2 = Gemma3Config.from_pretrained(str(d))
    assert cfg2 == cfg
    assert Gemma3Config.from_pretrained(str(tmp_path / "none")) == Gemma3Config()
    for prefix in ("language_model.model.", "model."):
        p = tmp_path / prefix.strip(".").replace(".", "_")
        _write_checkpoint(str(p), cfg, prefix, extra={"vision_tower.x.weight": torch.zeros(2)})
        plan = scan_gemma3_checkpoint(str(p), cfg)
        assert len(plan) == 2 + 13 * 6 and plan["layers.5.self_attn.k_proj.weight"][1] == prefix + "layers.5.self_attn.k_proj.weight"
    _write_checkpoint(str(tmp_path / "missing"), cfg, "model.", drop="layers.2.mlp.down_proj.weight")
    with pytest.raises(KeyError, match="layers.2.mlp.down_proj.weight"):
        scan_gemma3_checkpoint(str(tmp_path / "missing"), cfg)
    _write_checkpoint(str(tmp_path / "unknown"), cfg, "model.", extra={"model.layers.0.self_attn.extra.weight": torch.zeros(2)})
    with pytest.raises(KeyError, match="model.layers.0.self_attn.extra.weight"):
        scan_gemma3_checkpoint(str(tmp_path / "unknown"), cfg)
    with pytest.raises(FileNotFoundError):
        scan_gemma3_checkpoint(str(tmp_path), cfg)


def test_tokenizer_left_pads_with_eos_and_truncates(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    from ltx_2_mlx_amd.model.text_encoder.gemma3 import load_gemma_tokenizer, tokenize_prompt
    vocab = gemma3_ref.write_wordlevel_tokenizer(tmp_path, ["a", "red", "fox", "runs", "through", "the", "snow"])
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")
    tok = load_gemma_tokenizer(str(tmp_path))
    assert tok.padding_side == "left" and tok.pad_token == "<eos>"
    ids, mask = tokenize_prompt(tok, "a red fox runs through the snow", max_length=12)
    assert ids.shape == mask.shape == (1, 12)
    assert mask[0].tolist() == [0] * 4 + [1] * 8 and ids[0, :4].tolist() == [vocab["<eos>"]] * 4
    assert ids[0, 4:].tolist() == [vocab[w] for w in "<bos> a red fox runs through the snow".split()]
    ids, mask = tokenize_prompt(tok, "a red fox runs through the snow", max_length=4)          # truncation
    assert mask.tolist() == [[1, 1, 1, 1]] and ids[0].tolist() == [vocab[w] for w in ("<bos>", "a", "red", "fox")]
    with pytest.raises(OSError):                     # local files only: a name that is not a directory is never looked up online
        load_gemma_tokenizer(str(tmp_path / "no-such-tokenizer"))


def test_gemm_routes_of_the_gemma_shapes():
    """The four Gemma GEMMs on ltx2_gemm_bf16 (bf16 epilogue), pinned at 64, 300 and 1024 rows the way
    test_gemm_dispatch_routes_of_every_model_gemm pins the DiT's.  Host logic only."""
    from ltx_2_mlx_amd import _native as nv
    if not os.path.exists(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = nv.lib()
    name = {getattr(nv, k): k for k in dir(nv) if k.startswith("ROUTE_")}
    shapes = {"qkv": (8192, 3840), "o_proj": (3840, 4096), "gate_up": (30720, 3840), "down": (3840, 15360)}
    assert all(k % 128 == 0 for _, k in shapes.values())
    want = {64: dict(qkv="ROUTE_SKINNY", o_proj="ROUTE_SKINNY", gate_up="ROUTE_SKINNY", down="ROUTE_SKINNY"),
            300: dict(qkv="ROUTE_SMALL", o_proj="ROUTE_SMALL", gate_up="ROUTE_SMALL", down="ROUTE_SMALL"),
            1024: dict(qkv="ROUTE_V4_224", o_proj="ROUTE_SMALL", gate_up="ROUTE_V4_256", down="ROUTE_SMALL")}
    for m, routes in want.items():
        for nm, (n, k) in shapes.items():
            assert name.get(L.ltx2_gemm_route(m, n, k, nv.EPI_BF16, 0, 0)) == routes[nm], (m, nm)
