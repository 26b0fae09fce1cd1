"""The LTX-2.3 ("V2") text encoder's host side, without a GPU: the checkpoint-metadata rules of create_av_text_encoder_v2_from_checkpoint
(reference LTX_2_MLX/model/text_encoder/encoder.py:717-871), the key scheme of load_av_text_encoder_v2_weights (:874-913), the new C-ABI
symbol in the header / library / binding, the routing of generate_video to the V2 encoder, and the stored reference vectors."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_ckpt(path, tensors, config=None, version="2.3.0"):
    from safetensors.torch import save_file
    md = {"model_version": version}
    if config is not None:
        md["config"] = config if isinstance(config, str) else json.dumps(config)
    save_file(tensors, str(path), metadata=md)
    return str(path)


class _Spy:
    made = []

    def __init__(self, **kw):
        self.kw = kw
        self.loaded = None
        _Spy.made.append(self)

    def load_state_dict(self, sd, strict=True):
        self.loaded = dict(sd)


class _SpyConnector(_Spy):
    pass


class _SpyExtractor(_Spy):
    pass


@pytest.fixture
def spied(monkeypatch):
    from ltx_2_mlx_amd.model.text_encoder import encoder
    _Spy.made = []
    monkeypatch.setattr(encoder, "Embeddings1DConnector", _SpyConnector)
    monkeypatch.setattr(encoder, "GemmaFeaturesExtractorV2", _SpyExtractor)
    return encoder


FULL = {"connector_num_attention_heads": 32, "connector_attention_head_dim": 128, "connector_num_layers": 8,
        "audio_connector_num_attention_heads": 32, "audio_connector_attention_head_dim": 64,
        "connector_positional_embedding_max_pos": [4096], "rope_type": "interleaved", "connector_apply_gated_attention": True,
        "frequencies_precision": "float64", "num_attention_heads": 32}


def _connectors(enc):
    return enc.embeddings_connector.kw, enc.audio_embeddings_connector.kw


def test_metadata_rules_of_the_v2_encoder(tmp_path, spied, capsys):
    """Four forms of the `transformer` record give the connector configurations the reference's rules give."""
    t = {"x": torch.zeros(2)}
    # 1. a full LTX-2.3 record
    enc = spied.create_av_text_encoder_v2_from_checkpoint(_write_ckpt(tmp_path / "full.safetensors", t, {"transformer": FULL}), device="cpu")
    v, a = _connectors(enc)
    common = dict(num_layers=8, num_learnable_registers=128, positional_embedding_max_pos=[4096], rope_type="interleaved",
                  apply_gated_attention=True, double_precision_rope=True, device="cpu")
    assert v == dict(attention_head_dim=128, num_attention_heads=32, **common)
    assert a == dict(attention_head_dim=64, num_attention_heads=32, **common)
    assert enc.feature_extractor.kw == dict(hidden_dim=3840, num_layers=49, video_inner_dim=4096, audio_inner_dim=2048, device="cpu")
    assert ("AV text encoder config: video_heads=32x128, audio_heads=32x64, layers=8, rope=interleaved, max_pos=[4096], gated=on, "
            "double_precision_rope=on") in capsys.readouterr().out
    # 2. the keys missing (an empty record, no config at all, a config that is not JSON): the fall-back values
    fallback = dict(num_layers=8, num_learnable_registers=128, positional_embedding_max_pos=[1], rope_type="interleaved",
                    apply_gated_attention=True, double_precision_rope=False, device="cpu")
    for i, cfg in enumerate(({"transformer": {}}, None, "not json", {"transformer": "nonsense"})):
        enc = spied.create_av_text_encoder_v2_from_checkpoint(_write_ckpt(tmp_path / f"miss{i}.safetensors", t, cfg), device="cpu")
        v, a = _connectors(enc)
        assert v == dict(attention_head_dim=128, num_attention_heads=32, **fallback), cfg
        assert a == dict(attention_head_dim=64, num_attention_heads=32, **fallback), cfg
    # the audio connector follows the video connector's head count when it has none of its own
    enc = spied.create_av_text_encoder_v2_from_checkpoint(
        _write_ckpt(tmp_path / "heads.safetensors", t, {"transformer": {"connector_num_attention_heads": 16, "connector_num_layers": 4}}), device="cpu")
    v, a = _connectors(enc)
    assert (v["num_attention_heads"], a["num_attention_heads"], a["attention_head_dim"], v["num_layers"], a["num_layers"]) == (16, 16, 64, 4, 4)
    # 3. rope_type: "split" in any case, the `split_rope` spelling, garbage -> interleaved
    for j, (rec, want) in enumerate((({"rope_type": "split"}, "split"), ({"rope_type": " SPLIT "}, "split"), ({"split_rope": "split"}, "split"),
                                     ({"rope_type": "spiral"}, "interleaved"), ({"rope_type": 7}, "interleaved"),
                                     ({"split_rope": True}, "interleaved"), ({"rope_type": "interleaved", "split_rope": "split"}, "interleaved"))):
        enc = spied.create_av_text_encoder_v2_from_checkpoint(_write_ckpt(tmp_path / f"rope{j}.safetensors", t, {"transformer": rec}), device="cpu")
        assert [c["rope_type"] for c in _connectors(enc)] == [want, want], rec
    # 4. max_pos: int / float / list / empty list / missing
    for j, (val, want) in enumerate(((4096, [4096]), (2048.0, [2048]), ([4096], [4096]), ([20, 2048], [20, 2048]), ([], [1]), ("4096", [1]))):
        enc = spied.create_av_text_encoder_v2_from_checkpoint(
            _write_ckpt(tmp_path / f"pos{j}.safetensors", t, {"transformer": {"connector_positional_embedding_max_pos": val}}), device="cpu")
        assert [c["positional_embedding_max_pos"] for c in _connectors(enc)] == [want, want], val
    # gated off, another frequency precision
    enc = spied.create_av_text_encoder_v2_from_checkpoint(
        _write_ckpt(tmp_path / "g.safetensors", t, {"transformer": {"connector_apply_gated_attention": False, "frequencies_precision": "float32"}}),
        device="cpu")
    assert [(c["apply_gated_attention"], c["double_precision_rope"]) for c in _connectors(enc)] == [(False, False)] * 2


def test_create_av_text_encoder_v2_defaults_are_the_reference_ones(spied):
    import inspect
    sig = inspect.signature(spied.create_av_text_encoder_v2)
    got = {k: p.default for k, p in sig.parameters.items()}
    assert got == dict(hidden_dim=3840, num_gemma_layers=49, video_inner_dim=4096, audio_inner_dim=2048, video_connector_heads=32,
                       video_connector_head_dim=128, audio_connector_heads=32, audio_connector_head_dim=64, connector_layers=8,
                       num_registers=128, positional_embedding_max_pos=None, rope_type="interleaved", connector_apply_gated_attention=True,
                       double_precision_rope=False, device="cuda")
    from ltx_2_mlx_amd.model import text_encoder as te
    for name in ("create_av_text_encoder_v2", "create_av_text_encoder_v2_from_checkpoint", "load_av_text_encoder_v2_weights"):
        assert name in te.__all__ and getattr(te, name) is getattr(spied, name)


def test_connector_rope_type_is_validated_before_the_device():
    from ltx_2_mlx_amd.model.text_encoder import Embeddings1DConnector
    with pytest.raises(ValueError, match="rope_type"):
        Embeddings1DConnector(rope_type="spiral", device="cpu")
    with pytest.raises(RuntimeError, match="MI355X"):              # a valid type gets as far as the device check (no CPU fallback)
        Embeddings1DConnector(rope_type="split", device="cpu")


def test_v2_loader_key_scheme(tmp_path, spied):
    """load_av_text_encoder_v2_weights consumes exactly the four aggregate-embed tensors and the tensors under the two connector
    prefixes; `caption_projection.*`, a V1 `aggregate_embed`, and the DiT's own keys are left alone."""
    def fresh(keys):            # safetensors refuses tensors that share storage: a new one per key
        return {k: torch.zeros(2) for k in keys}
    z = None
    mine = {"text_embedding_projection.video_aggregate_embed.weight": z, "text_embedding_projection.video_aggregate_embed.bias": z,
            "text_embedding_projection.audio_aggregate_embed.weight": z, "text_embedding_projection.audio_aggregate_embed.bias": z,
            "model.diffusion_model.video_embeddings_connector.learnable_registers": z,
            "model.diffusion_model.video_embeddings_connector.transformer_1d_blocks.0.attn1.to_q.weight": z,
            "model.diffusion_model.video_embeddings_connector.transformer_1d_blocks.7.attn1.to_gate_logits.bias": z,
            "model.diffusion_model.audio_embeddings_connector.learnable_registers": z,
            "model.diffusion_model.audio_embeddings_connector.transformer_1d_blocks.3.ff.net.2.weight": z}
    others = {"model.diffusion_model.caption_projection.linear_1.weight": z, "model.diffusion_model.audio_caption_projection.linear_1.weight": z,
              "model.diffusion_model.transformer_blocks.0.attn1.to_q.weight": z, "text_embedding_projection.aggregate_embed.weight": z,
              "model.diffusion_model.video_embeddings_connector_extra.weight": z, "vae.decoder.conv_in.conv.weight": z}
    mine, others = fresh(mine), fresh(others)
    path = _write_ckpt(tmp_path / "k.safetensors", {**mine, **others})
    enc = spied.create_av_text_encoder_v2(device="cpu")
    assert spied.load_av_text_encoder_v2_weights(enc, path) == len(mine) == 9
    assert sorted(enc.feature_extractor.loaded) == ["audio_aggregate_embed.bias", "audio_aggregate_embed.weight", "video_aggregate_embed.bias",
                                                    "video_aggregate_embed.weight"]
    assert sorted(enc.embeddings_connector.loaded) == ["learnable_registers", "transformer_1d_blocks.0.attn1.to_q.weight",
                                                       "transformer_1d_blocks.7.attn1.to_gate_logits.bias"]
    assert sorted(enc.audio_embeddings_connector.loaded) == ["learnable_registers", "transformer_1d_blocks.3.ff.net.2.weight"]
    with pytest.raises(KeyError, match="text_embedding_projection.*video_embeddings_connector.*audio_embeddings_connector"):
        spied.load_av_text_encoder_v2_weights(enc, _write_ckpt(tmp_path / "none.safetensors", others))


def test_features_rms_symbol_in_header_library_and_binding():
    from ltx_2_mlx_amd import _native as nv
    name = "ltx2_gemma_features_rms"
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltx2hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ltx2_[a-z0-9_]+)\s*\(", txt)))
    assert name in declared and name in nv.SIGNATURES and len(nv.SIGNATURES[name][1]) == 11
    assert sorted(nv.exported_symbols()) == declared                       # the header and the binding agree in number
    if not os.path.exists(nv.LIB_PATH) or not os.path.exists(nv.LIB_PATH_F16):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    for path in (nv.LIB_PATH, nv.LIB_PATH_F16):
        lib = ctypes.CDLL(path)
        assert all(hasattr(lib, s) for s in declared), path
    from ltx_2_mlx_amd import kernels as K
    assert callable(K.gemma_features_rms)
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_generate_video_routes_a_23_checkpoint_to_the_v2_encoder(tmp_path, monkeypatch):
    """generate_video(weights_path=<2.3 file>, gemma_path=<existing dir>) reaches create_av_text_encoder_v2_from_checkpoint with the
    Gemma's (hidden, layers + 1) and the checkpoint's widths (the Gemma loader is stubbed, the constructor spied on); a checkpoint whose
    aggregate embeds do not fit the Gemma at hand is a ValueError naming both shapes; without a checkpoint model_version="2.3" reaches
    create_av_text_encoder_v2 at the transformer's widths."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate as gen
    from ltx_2_mlx_amd.model import text_encoder as te

    class Cfg:
        hidden_size, num_hidden_layers = 8, 2

    class FakeGemma:
        config = Cfg()
        freed = 0

        def free(self):
            FakeGemma.freed += 1

    class Routed(Exception):
        pass

    def spy(name):
        def f(*a, **k):
            raise Routed(name, a, k)
        return f
    loads = []
    monkeypatch.setattr(gen, "_load_gemma", lambda path, device: (loads.append(path), (object(), FakeGemma()))[1])
    monkeypatch.setattr(te, "create_av_text_encoder_v2_from_checkpoint", spy("from_checkpoint"))
    monkeypatch.setattr(te, "create_av_text_encoder_v2", spy("random"))
    gemma_dir = tmp_path / "gemma"
    gemma_dir.mkdir()
    t = {"text_embedding_projection.video_aggregate_embed.weight": torch.zeros(16, 24),
         "text_embedding_projection.audio_aggregate_embed.weight": torch.zeros(8, 24)}
    ck = _write_ckpt(tmp_path / "v23.safetensors", t, {"transformer": FULL})
    kw = dict(gemma_path=str(gemma_dir), device="cpu", output_path=str(tmp_path / "o.mp4"))
    with pytest.raises(Routed) as e:
        gen.generate_video("a prompt", weights_path=ck, **kw)
    assert e.value.args[0] == "from_checkpoint" and e.value.args[1] == (ck,)
    assert e.value.args[2] == dict(hidden_dim=8, num_gemma_layers=3, video_inner_dim=16, audio_inner_dim=8, device="cpu")
    assert loads == [str(gemma_dir)] and FakeGemma.freed == 1            # one load, freed although the encoder failed
    bad = _write_ckpt(tmp_path / "bad.safetensors", {k: torch.zeros(v.shape[0], 40) for k, v in t.items()}, {"transformer": FULL})
    with pytest.raises(ValueError, match=r"\(8, 3\).*\(16, 24\).*\(16, 40\)"):
        gen.generate_video("a prompt", weights_path=bad, **kw)
    with pytest.raises(Routed) as e:
        gen.generate_video("a prompt", weights_path=None, model_version="2.3", num_heads=4, **kw)
    assert e.value.args[0] == "random"
    assert e.value.args[2] == dict(hidden_dim=8, num_gemma_layers=3, video_inner_dim=512, audio_inner_dim=256, video_connector_heads=4,
                                   audio_connector_heads=4, device="cpu")
    src = open(os.path.join(ROOT, "scripts", "generate.py")).read()
    assert "Gemma encoding for LTX-2.3" not in src


def test_text_encoder_v2_fixture_keys_and_shapes():
    """tests/golden/text_encoder_v2.npz (tools/pin_oracle_against_reference.py text_encoder_v2): data only -- seeds, the head and tail
    rows of both encodings under both RoPE types, the mask."""
    path = os.path.join(ROOT, "tests", "golden", "text_encoder_v2.npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    c = dict(zip([str(k) for k in z["config_keys"]], [int(v) for v in z["config"]]))
    assert c == dict(hidden=64, layers=5, heads=2, video_head_dim=128, audio_head_dim=64, blocks=2, registers=16, tokens=40, pad=10,
                     seed_fe=71, seed_video=72, seed_audio=73, seed_hidden=74)
    want = {"config_keys", "config"}
    for tag in ("interleaved", "split"):
        for mod, width in (("video", 256), ("audio", 128)):
            assert z[f"{tag}_{mod}_head"].shape == (1, 56, width) and z[f"{tag}_{mod}_tail"].shape == (1, 32, width)
            assert z[f"{tag}_{mod}_head"].dtype == np.float32 and np.isfinite(z[f"{tag}_{mod}_head"]).all()
            assert z[f"{tag}_{mod}_stats"].shape == (3,)
            want |= {f"{tag}_{mod}_head", f"{tag}_{mod}_tail", f"{tag}_{mod}_stats"}
        assert z[f"{tag}_mask"].shape == (1, 1024) and int(z[f"{tag}_mask"].sum()) == 1024
        want.add(f"{tag}_mask")
    assert set(z.files) == want
    # the two rotations are told apart by the 0.008 gate of the GPU test
    for mod in ("video", "audio"):
        a, b = z[f"split_{mod}_head"].astype(np.float64), z[f"interleaved_{mod}_head"].astype(np.float64)
        assert np.linalg.norm(a - b) / np.linalg.norm(b) > 2 * 0.008


def test_gemm_routes_of_the_v2_projections():
    """The two aggregate-embed projections (K = 49 * 3840 = 188 160, a multiple of 256; N = 4096 / 2048) on the existing GEMM entry:
    the skinny kernel up to 128 prompt tokens, the 128 x 128 tiles above.  (Neither route splits K or needs a workspace, and both
    address with 64-bit offsets, so this K needed no change to them; tests/test_text_encoder_v2_gpu.py runs both at full size.)"""
    from ltx_2_mlx_amd import _native as nv
    route = nv.lib().ltx2_gemm_route
    for n in (4096, 2048):
        assert [route(m, n, 188160, nv.EPI_F32, 0, 0) for m in (1, 64, 128, 256, 1024)] == \
            [nv.ROUTE_SKINNY, nv.ROUTE_SKINNY, nv.ROUTE_SKINNY, nv.ROUTE_SMALL, nv.ROUTE_SMALL]
