"""CPU-only tests (run with -m "not gpu"): the oracle against the reference's own closed-form
known answers, the host-side logic of the product against the oracle, the C-ABI symbol table,
and the world_size-2 gloo path of the prompt sharding / weight broadcast."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- oracle vs reference known answers
def test_sigma_tables_match_reference_constants():
    # reference components/schedulers.py:236-253, asserted by its tests/test_scheduler.py:103-144
    from oracle import loop
    from ltx_2_mlx_amd.components import DISTILLED_SIGMA_VALUES, STAGE_2_DISTILLED_SIGMA_VALUES
    assert loop.DISTILLED_SIGMA_VALUES == [1.0, 0.99375, 0.9875, 0.98125, 0.975, 0.909375, 0.725, 0.421875, 0.0]
    assert loop.STAGE_2_DISTILLED_SIGMA_VALUES == [0.909375, 0.725, 0.421875, 0.0]
    assert DISTILLED_SIGMA_VALUES == loop.DISTILLED_SIGMA_VALUES
    assert STAGE_2_DISTILLED_SIGMA_VALUES == loop.STAGE_2_DISTILLED_SIGMA_VALUES
    assert len(DISTILLED_SIGMA_VALUES) == 9 and len(STAGE_2_DISTILLED_SIGMA_VALUES) == 4
    assert DISTILLED_SIGMA_VALUES[-1] == 0.0 and all(a >= b for a, b in zip(DISTILLED_SIGMA_VALUES, DISTILLED_SIGMA_VALUES[1:]))


def test_post_process_and_timesteps_known_answers():
    # reference tests/test_pipelines.py:193-266
    from oracle import loop
    from ltx_2_mlx_amd.pipelines import post_process_latent, timesteps_from_mask
    den = torch.tensor([[[1.0, 2.0], [3.0, 4.0]]])
    clean = torch.tensor([[[5.0, 6.0], [7.0, 8.0]]])
    for fn in (loop.post_process_latent, post_process_latent):
        assert torch.allclose(fn(den, torch.ones_like(den), clean), den)
        assert torch.allclose(fn(den, torch.zeros_like(den), clean), clean)
        assert torch.allclose(fn(torch.tensor([[[1.0, 2.0]]]), torch.tensor([[[1.0, 0.0]]]), torch.tensor([[[5.0, 6.0]]])),
                              torch.tensor([[[1.0, 6.0]]]))
    for fn in (loop.timesteps_from_mask, timesteps_from_mask):
        assert torch.allclose(fn(torch.ones(1, 10), 0.5), torch.full((1, 10), 0.5))
        assert torch.allclose(fn(torch.tensor([[1.0, 0.5, 0.0]]), 2.0), torch.tensor([[2.0, 1.0, 0.0]]))


def test_latent_shape_known_answer():
    # reference tests/test_pipelines.py:269-297: 97 x 480 x 704 -> 13 x 15 x 22
    from oracle import loop
    from ltx_2_mlx_amd.types import VideoLatentShape, VideoPixelShape
    assert loop.latent_shape_from_pixels(97, 480, 704) == (13, 15, 22)
    s = VideoLatentShape.from_pixel_shape(VideoPixelShape(1, 97, 480, 704, 24.0))
    assert (s.batch, s.channels, s.frames, s.height, s.width) == (1, 128, 13, 15, 22)
    assert loop.latent_shape_from_pixels(65, 512, 768) == (9, 16, 24)        # BASELINE main config: N = 3456


def test_patchify_roundtrip_and_positions():
    from oracle import loop
    from ltx_2_mlx_amd.components import VideoLatentPatchifier
    from ltx_2_mlx_amd.conditioning import VideoLatentTools
    from ltx_2_mlx_amd.types import VideoLatentShape
    x = torch.randn(1, 128, 3, 4, 5)
    p = VideoLatentPatchifier(1)
    shp = VideoLatentShape.from_shape(x.shape)
    tok = p.patchify(x)
    assert tok.shape == (1, 60, 128) and torch.equal(tok, loop.patchify(x))
    assert torch.equal(p.unpatchify(tok, shp), x) and torch.equal(loop.unpatchify(tok, 3, 4, 5), x)
    st = VideoLatentTools(p, shp, fps=24.0).create_initial_state()
    assert st.latent.shape == (1, 60, 128) and st.denoise_mask.shape == (1, 60, 1) and st.positions.shape == (1, 3, 60, 2)
    assert torch.allclose(st.positions, loop.video_positions(1, 3, 4, 5, 24.0))
    # causal fix: first latent frame covers [0, 1/24) s; second [1/24, 9/24)
    assert torch.allclose(st.positions[0, 0, 0], torch.tensor([0.0, 1 / 24]))
    assert torch.allclose(st.positions[0, 0, 20], torch.tensor([1 / 24, 9 / 24]))
    with pytest.raises(ValueError):
        VideoLatentTools(p, shp, fps=24.0).create_initial_state(initial_latent=torch.zeros(1, 128, 3, 4, 6))


def test_ltx2_scheduler_properties():
    from oracle import loop
    from ltx_2_mlx_amd.components import LTX2Scheduler
    for steps in (2, 8, 30):
        s = LTX2Scheduler().execute(steps)
        assert torch.allclose(s, loop.ltx2_scheduler(steps))
        assert s.shape == (steps + 1,) and abs(float(s[0]) - 1.0) < 1e-6 and s[-1] == 0.0
        assert bool((s[:-1] >= s[1:]).all())
        assert abs(float(s[-2]) - 0.1) < 1e-6                         # stretched to terminal 0.1
    lat = torch.zeros(1, 128, 9, 16, 24)
    assert torch.allclose(LTX2Scheduler().execute(8, latent=lat), loop.ltx2_scheduler(8, tokens=3456))


def test_rope_tables_layout():
    """SPLIT RoPE: 2 identity slots at the FRONT, slot = f*3 + d, head h gets slots [64h, 64h+64)."""
    from oracle import dit, loop
    from ltx_2_mlx_amd.model.transformer import rope_tables_token_major
    heads, D = 32, 4096
    pos = loop.video_positions(1, 2, 3, 4, 24.0)
    cos, sin = dit.rope_split_tables(pos, D, heads, 10000.0, [20, 2048, 2048])
    assert cos.shape == (1, 32, 24, 64)
    assert torch.all(cos[0, 0, :, :2] == 1) and torch.all(sin[0, 0, :, :2] == 0)     # 4096/2 - 3*682 = 2 pad
    grid = dit.rope_freq_grid(10000.0, 3, D)
    assert grid.shape == (682,) and abs(float(grid[0]) - torch.pi / 2) < 1e-6
    tok = 13
    mid = (pos[0, :, tok, 0] + pos[0, :, tok, 1]) / 2
    frac = mid / torch.tensor([20.0, 2048.0, 2048.0])
    # slot 2 + (f*3 + d) -> head 0, index 2 + 3f + d
    for f_idx, d_idx in [(0, 0), (0, 2), (5, 1)]:
        expect = torch.cos(grid[f_idx] * (frac[d_idx] * 2 - 1))
        assert abs(float(cos[0, 0, tok, 2 + 3 * f_idx + d_idx]) - float(expect)) < 1e-6
    ct, st = rope_tables_token_major(pos, D, heads, 10000.0, [20, 2048, 2048])
    assert torch.equal(ct, cos[0].permute(1, 0, 2).reshape(24, D // 2))
    assert torch.equal(st, sin[0].permute(1, 0, 2).reshape(24, D // 2))
    with pytest.raises(ValueError):
        rope_tables_token_major(pos, D, heads, 10000.0, [20, 2048])


def test_split_rope_is_a_rotation():
    from oracle import dit, loop
    pos = loop.video_positions(1, 2, 2, 2, 24.0)
    cos, sin = dit.rope_split_tables(pos, 256, 2, 10000.0, [20, 2048, 2048])
    x = torch.randn(1, 8, 256)
    y = dit.apply_split_rope(x, cos, sin)
    assert torch.allclose(y.norm(dim=-1), x.norm(dim=-1), rtol=1e-5)                   # norm preserving
    assert torch.allclose(dit.apply_split_rope(y, cos, -sin), x, atol=1e-5)            # inverse rotation


def test_oracle_conv3d_matches_tap_loop():
    """conv3d_simple == the reference's 3-tap conv2d accumulation with explicit padding."""
    import torch.nn.functional as F
    from oracle import vae
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 4, 3, 5, 6, generator=g)
    w = torch.randn(7, 4, 3, 3, 3, generator=g)
    b = torch.randn(7, generator=g)
    for causal in (False, True):
        xp = torch.cat([x[:, :, :, 1:2].flip(3), x, x[:, :, :, -2:-1].flip(3)], 3)
        xp = torch.cat([xp[..., 1:2].flip(4), xp, xp[..., -2:-1].flip(4)], 4)
        xp = torch.cat([xp[:, :, :1]] * (2 if causal else 1) + [xp] + ([] if causal else [xp[:, :, -1:]]), 2)
        out = None
        for kt in range(3):
            xs = xp[:, :, kt:kt + 3].permute(0, 2, 1, 3, 4).reshape(3, 4, 7, 8)
            o = F.conv2d(xs, w[:, :, kt]).reshape(1, 3, 7, 5, 6).permute(0, 2, 1, 3, 4)
            out = o if out is None else out + o
        out = out + b[None, :, None, None, None]
        assert torch.allclose(vae.conv3d_simple(x, w, b, causal), out, atol=1e-4)


def test_oracle_unpatchify_and_d2s_orders():
    from oracle import vae
    # unpatchify: packing (c, p, r_w, r_h): channel c*16 + rw*4 + rh -> pixel (h*4+rh, w*4+rw)
    x = torch.zeros(1, 48, 1, 2, 2)
    x[0, 1 * 16 + 2 * 4 + 3, 0, 1, 0] = 5.0
    y = vae.unpatchify(x, 4, 1)
    assert y.shape == (1, 3, 1, 8, 8) and y[0, 1, 0, 1 * 4 + 3, 0 * 4 + 2] == 5.0 and y.abs().sum() == 5.0
    # depth to space: channel ((c*ft + a)*fh + b)*fw + d -> (t*ft+a, h*fh+b, w*fw+d)
    z = torch.zeros(1, 16, 2, 2, 2)
    z[0, ((1 * 2 + 1) * 2 + 0) * 2 + 1, 1, 0, 1] = 3.0
    d = vae.depth_to_space(z, 2, (2, 2, 2))
    assert d[0, 1, 1 * 2 + 1, 0 * 2 + 0, 1 * 2 + 1] == 3.0 and d.abs().sum() == 3.0


def test_decode_chunk_walk_and_blend():
    from oracle import vae
    assert vae.temporal_chunks(9) == [(0, 7), (5, 9)]
    assert vae.temporal_chunks(7) == [(0, 7)]
    assert vae.temporal_chunks(13) == [(0, 7), (5, 12), (10, 13)]
    assert vae.latent_t_to_pixel_t(9) == 65 and vae.latent_t_to_pixel_t(2) == 9
    a = torch.zeros(1, 3, 49, 2, 2)
    b = torch.ones(1, 3, 25, 2, 2)
    v = vae.blend_chunks([a, b], 9)
    assert v.shape[2] == 65
    assert torch.all(v[:, :, :40] == 0) and torch.all(v[:, :, 49:] == 1)
    assert torch.allclose(v[0, 0, 40:49, 0, 0], torch.linspace(0, 1, 9))


def test_tile_specs_and_masks_match_oracle():
    from oracle import vae
    from ltx_2_mlx_amd.model.video_vae import TilingConfig, compute_trapezoidal_mask_1d, generate_tile_specs
    specs = generate_tile_specs((1, 128, 9, 32, 48), TilingConfig.default())
    ref = vae.tile_specs((1, 128, 9, 32, 48))
    assert len(specs) == len(ref) == 24                                   # 2 x 3 x 4 tiles
    for s, r in zip(specs, ref):
        assert (s.in_t_start, s.in_t_end) == r["in_t"] and (s.in_h_start, s.in_h_end) == r["in_h"] and (s.in_w_start, s.in_w_end) == r["in_w"]
        assert (s.out_t_start, s.out_t_end) == r["out_t"] and (s.ramp_h_left, s.ramp_h_right) == r["ramp_h"]
    for args in [(10, 3, 2, False), (10, 3, 0, True), (5, 9, 9, False), (64, 0, 24, True)]:
        assert torch.allclose(compute_trapezoidal_mask_1d(*args), vae.trapezoid_mask_1d(*args))
    m = compute_trapezoidal_mask_1d(6, 2, 0, False)
    assert torch.allclose(m, torch.tensor([1 / 3, 2 / 3, 1, 1, 1, 1]))
    with pytest.raises(ValueError):
        compute_trapezoidal_mask_1d(0, 0, 0)


def test_config_validation_matches_reference_errors():
    from ltx_2_mlx_amd.model.video_vae import SpatialTilingConfig, TemporalTilingConfig
    from ltx_2_mlx_amd.pipelines import DistilledConfig
    with pytest.raises(ValueError, match="8\\*k \\+ 1"):
        DistilledConfig(num_frames=64)
    with pytest.raises(ValueError, match="divisible by 64"):
        DistilledConfig(height=500, width=704)
    assert DistilledConfig(height=512, width=768, num_frames=65)._get_tiling_config() is None      # 3456 voxels
    assert DistilledConfig(height=1024, width=1536, num_frames=65)._get_tiling_config() is not None  # 13824 > 4000
    with pytest.raises(ValueError):
        SpatialTilingConfig(32)
    with pytest.raises(ValueError):
        TemporalTilingConfig(16, 16)


def test_euler_oracle_known_answer():
    from oracle import loop
    x = torch.tensor([[2.0, -1.0]])
    x0 = torch.tensor([[1.0, 1.0]])
    # v = (x - x0)/sigma = [2, -4]; x + v*(0.25-0.5) = [1.5, 0]
    assert torch.allclose(loop.euler_step(x, x0, 0.5, 0.25), torch.tensor([[1.5, 0.0]]))
    assert torch.allclose(loop.euler_step(x, x0, 0.5, 0.0), x0)            # stepping to sigma 0 lands on x0
    with pytest.raises(ValueError, match="Sigma can't be 0.0"):
        loop.euler_step(x, x0, 0.0, 0.0)


def test_oracle_dit_invariances():
    """Size-independent properties: per-token uniform timesteps == scalar timestep; zero gates make a
    block the identity on the residual stream."""
    from oracle import dit, loop
    cfg = dit.DiTConfig(num_attention_heads=2, num_layers=1, caption_channels=64)
    w = dit.make_dit_weights(cfg, 0)
    lat = torch.randn(1, 12, 128)
    ctx = torch.randn(1, 5, 64) * 0.1
    pos = loop.video_positions(1, 1, 3, 4, 24.0)
    a = dit.x0_model(lat, ctx, torch.tensor([0.7]), pos, w, cfg)
    b = dit.x0_model(lat, ctx, torch.full((1, 12, 1), 0.7), pos, w, cfg)
    assert torch.allclose(a, b, atol=1e-5)


# ---------------------------------------------------------------- C ABI
def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ltx2_[a-z0-9_]+)\s*\(", txt)))


def test_capi_exports_every_declared_symbol():
    from ltx_2_mlx_amd import _native as nv
    if not os.path.exists(nv.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(nv.LIB_PATH)
    declared = _header_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f"libltx2hip.so does not export {name}"
    assert sorted(nv.exported_symbols()) == declared          # python binding table == header
    # the header's version macro, the library and the binding agree; a library of another version is refused at load
    hdr = int(re.search(r"#define LTX2_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "ltx2hip.h")).read()).group(1))
    assert nv.lib().ltx2_abi_version() == nv.ABI_VERSION == hdr == 3


def test_library_of_another_abi_version_is_refused(tmp_path):
    """ltx2_dit_forward / ltx2_dit_denoise_step gained an argument mid-list; a stale .so (or a caller built against the old
    header) must fail at load, not shift pointers.  A stub library that reports version 1 is refused by the binding."""
    import subprocess
    src = tmp_path / "stub.c"
    src.write_text("int ltx2_abi_version(void) { return 1; }\nconst char* ltx2_last_error(void) { return \"\"; }\n")
    so = tmp_path / "libstub.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    code = ("import sys; sys.path.insert(0, %r)\nfrom ltx_2_mlx_amd import _native as nv\n"
            "try:\n    nv.lib()\nexcept nv.NativeLibraryMissing as e:\n    print('REFUSED', e)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, LTX2HIP_LIB=str(so)))
    assert "REFUSED" in r.stdout and "ABI version 1" in r.stdout, r.stdout + r.stderr


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "ltx-2-mlx_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{f} imports the oracle"
                assert "reference" not in dp


def test_no_cpu_fallback():
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import LTXModel
    with pytest.raises(RuntimeError):
        K.gemm(torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(128, 64, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        LTXModel(num_attention_heads=2, num_layers=1, device="cpu")
    # every other model class on the path refuses a CPU device the same way
    from ltx_2_mlx_amd.model.text_encoder import Embeddings1DConnector, GemmaFeaturesExtractorProjLinear, GemmaFeaturesExtractorV2
    from ltx_2_mlx_amd.model.upscaler import SpatialUpscaler
    from ltx_2_mlx_amd.model.video_vae import SimpleVideoDecoder
    from ltx_2_mlx_amd.model.video_vae_encoder import SimpleVideoEncoder
    for ctor in (Embeddings1DConnector, GemmaFeaturesExtractorProjLinear, GemmaFeaturesExtractorV2, SpatialUpscaler, SimpleVideoDecoder,
                 SimpleVideoEncoder):
        with pytest.raises(RuntimeError):
            ctor(device="cpu")


# ---------------------------------------------------------------- multi-process (gloo, world_size 2)
def test_shard_units():
    from ltx_2_mlx_amd.distributed import shard_units
    assert shard_units(8, 0, 8) == [0] and shard_units(8, 7, 8) == [7]
    assert shard_units(8, 1, 2) == [1, 3, 5, 7]
    got = sorted(sum((shard_units(11, r, 4) for r in range(4)), []))
    assert got == list(range(11))
    with pytest.raises(ValueError):
        shard_units(4, 4, 4)


_WORKER = r"""
import os, sys, torch
sys.path.insert(0, {root!r})
from ltx_2_mlx_amd.distributed import (init_distributed, broadcast_tensors, shard_units, max_over_ranks, barrier, count_ranks, gather_floats,
                                       replicas_identical, tensors_checksum)
rank, world, _ = init_distributed("gloo")
def draw(seed):
    g = torch.Generator().manual_seed(seed)
    return {{"a.weight": torch.randn(300, 7, generator=g).to(torch.bfloat16), "b.bias": torch.randn(11, generator=g),
            "c.weight": torch.randn(5000, generator=g).to(torch.bfloat16), "d.table": torch.randn(6, 16, generator=g),
            "e.codes": torch.randint(0, 255, (37, 5), generator=g).to(torch.uint8)}}
ref = draw(100)
for mode in ("ring", "scatter"):                       # the ring broadcast and the scatter + all-gather form (LTX2_BCAST=scatter)
    t = draw(100 + rank)                               # different content per rank before the broadcast
    assert not replicas_identical(t, torch.device("cpu"))
    n = broadcast_tensors(t, src=0, bucket_bytes=4096, mode=mode)
    assert all(torch.equal(t[k], ref[k]) for k in t), "broadcast mismatch (%s)" % mode
    assert n >= 3
    assert replicas_identical(t, torch.device("cpu")) and tensors_checksum(t) == tensors_checksum(ref)
    if rank == world - 1:                              # one flipped bit on one rank is seen by every rank
        t["c.weight"].view(torch.int16)[1234] ^= 1
    assert not replicas_identical(t, torch.device("cpu"))
units = shard_units(world * 2 + 1, rank, world)
assert units == list(range(rank, world * 2 + 1, world))
m = max_over_ranks(float(rank + 1), device=torch.device("cpu"))
assert m == float(world)
assert count_ranks(torch.device("cpu")) == world      # counted through the process group, not read from WORLD_SIZE
assert gather_floats([10.0 + rank, -1.0]) == [[10.0 + r, -1.0] for r in range(world)]
barrier()
open(os.path.join({out!r}, "ok_%d" % rank), "w").write("OK")
"""


@pytest.mark.parametrize("world", [2, 4])
def test_gloo_world2_broadcast_and_sharding(tmp_path, world):
    """The N > 1 host logic over gloo: both broadcast forms (ring, scatter + all-gather), the replica checksum (and that it sees one flipped
    bit), sharding, the reductions bench.py uses -- at world sizes 2 and 4."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, out=str(tmp_path)))
    port = 29500 + (os.getpid() % 2000) + world
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert all((tmp_path / f"ok_{i}").exists() for i in range(world))


def test_save_video_command_and_png_fallback(tmp_path, monkeypatch):
    """CLI file output (reference scripts/generate.py:2153-2226): the ffmpeg filter chain / encoder settings, and
    the PNG-frame fallback used on boxes without an ffmpeg binary."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("ltx2_generate_cli", os.path.join(ROOT, "scripts", "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.video_filters(24, 1.0) == []
    assert gen.video_filters(24, 2.0) == ["setpts=0.5*PTS"]
    assert gen.video_filters(48, 0.5) == ["setpts=2.0*PTS", "minterpolate=fps=48:mi_mode=mci:mc_mode=aobmc:me_mode=bidir:vsbmc=1"]
    cmd = gen.ffmpeg_command(768, 512, "out.mp4", fps=48)
    assert cmd[:2] == ["ffmpeg", "-y"] and "768x512" in cmd and cmd[cmd.index("-framerate") + 1] == "24"
    assert cmd[-9:] == ["-c:v", "libx264", "-pix_fmt", "yuv420p", "-crf", "18", "-loglevel", "error", "out.mp4"]
    frames = (np.arange(3 * 8 * 16 * 3) % 251).astype(np.uint8).reshape(3, 8, 16, 3)
    monkeypatch.setattr("shutil.which", lambda name: None)
    out = gen.save_video(frames, str(tmp_path / "clip.mp4"))
    from PIL import Image
    files = sorted(os.listdir(out))
    assert files == ["frame_0000.png", "frame_0001.png", "frame_0002.png"]
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, files[1]))), frames[1])
    with pytest.raises(ValueError):
        gen.save_video(frames.astype(np.float32), str(tmp_path / "bad.mp4"))


def test_generate_video_keeps_the_reference_keyword_surface(tmp_path, capsys):
    """Drop-in boundary: `generate_video` takes the reference's parameters, in order, with the reference's
    defaults (tests/golden/generate_video_signature.json, written from /root/reference/scripts/generate.py:933-997 by
    tools/pin_generate_signature.py); MI355X extras are keyword-only and come after them.  Out-of-path options raise only
    when they are moved off their reference default."""
    import inspect
    import json
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "generate_video_signature.json")))["params"]
    ours = list(inspect.signature(generate.generate_video).parameters.values())
    assert [p.name for p in ours[:len(ref)]] == [r["name"] for r in ref]
    for p, r in zip(ours, ref):
        assert p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert (p.default is inspect.Parameter.empty) == r["required"], p.name
        if not r["required"]:
            assert p.default == r["default"] and type(p.default) is type(r["default"]), (p.name, p.default, r["default"])
    assert all(p.kind == inspect.Parameter.KEYWORD_ONLY for p in ours[len(ref):])
    # every reference default is accepted as given: with use_gemma=True (the default) and no Gemma weights on disk the
    # reference prints an error and returns None (:1085-1092) -- so does this one, before touching the GPU
    kw = {r["name"]: r["default"] for r in ref if not r["required"]}
    kw["output_path"] = str(tmp_path / "gens" / "o.mp4")
    assert generate.generate_video("a prompt", **kw) is None
    assert "Gemma weights not found" in capsys.readouterr().out and os.path.isdir(tmp_path / "gens")
    # an out-of-path option off its default is refused by name; frames / resolution errors keep the reference's wording
    with pytest.raises(NotImplementedError, match="stg_scale"):
        generate.generate_video("a prompt", **dict(kw, stg_scale=1.0))
    with pytest.raises(NotImplementedError, match="use_fp16=False"):
        generate.generate_video("a prompt", **dict(kw, use_fp16=False))
    with pytest.raises(ValueError, match="8\\*k \\+ 1"):
        generate.generate_video("a prompt", **dict(kw, num_frames=96))
    with pytest.raises(ValueError, match="divisible by 32"):
        generate.generate_video("a prompt", **dict(kw, height=250))


def test_gemm_k_loop_generator_checks_its_own_pipeline():
    """ltx-2-mlx_amd/csrc/gen_gemm_v4.py emits the hand-scheduled K loops AND replays each schedule against the LDS-stage / fragment
    protocol (read only after the DMA landed + a barrier, DMA only after the last read retired + a barrier, no MFMA on an unretired
    fragment).  The shipped variants must pass; schedules that break the protocol must be caught -- that is the point of the checker."""
    import importlib.util, os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ltx-2-mlx_amd", "csrc", "gen_gemm_v4.py")
    spec = importlib.util.spec_from_file_location("gen_gemm_v4", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d14 = list(range(0, 56, 4)) + [55]
    ok = gen.Gen(14, 4, mb=16, npa=7, dma_last=d14, dma_ks0=[], m0_early=True)
    ok.build()
    assert gen.check(ok) == []
    short = gen.Gen(6, 4, mb=16, npa=3, dma_last=list(range(1, 23, 2)), dma_ks0=[], m0_early=True)       # the ragged-last-row-tile loop
    short.build()
    assert gen.check(short) == []
    # the checker must notice a broken protocol: replay the SAME schedule with its barriers, its DMA waits or its fragment waits removed
    for drop in ("barrier", "vm", "lgkm0"):
        bad = gen.Gen(14, 4, mb=16, npa=7, dma_last=d14, dma_ks0=[], m0_early=True)
        bad.build()
        bad.trace = [e for e in bad.trace if e[0] != drop]
        assert gen.check(bad), drop
    # the rolling fp8 loop (layout 6: one k-step per K-tile, single-set activation fragments read behind their last use)
    roll = dict(mb=16, npa=7, dma_last=list(range(2, 54, 3))[:15], dma_ks0=[], f8=True)
    ok = gen.Gen(14, 4, **roll)
    ok.build()
    assert ok.roll and ok.vgpr_top <= gen.VGPR_TOP_MAX and gen.check(ok) == []
    for drop in ("barrier", "vm", "lgkm0"):
        bad = gen.Gen(14, 4, **roll)
        bad.build()
        bad.trace = [e for e in bad.trace if e[0] != drop]
        assert gen.check(bad), drop
    bad = gen.Gen(14, 4, **roll)            # a fragment read moved IN FRONT of the MFMAs that still use its registers
    bad.build()
    tr = bad.trace
    i = next(k for k, e in enumerate(tr) if e[0] == "read" and e[1][0] == "A" and e[1][4] == "T+1")
    j = max(k for k in range(i) if tr[k][0] == "mfma" and tr[k][1][1] == tr[i][1][1])          # last MFMA on that row block before the read
    tr.insert(j - 2, tr.pop(i))
    assert gen.check(bad)


def test_generated_k_loops_are_in_sync_with_their_generator(tmp_path):
    """gemm_v4_loop.inc is generated code kept in the tree (hipcc needs it): regenerating it must reproduce the committed file byte for byte."""
    import subprocess
    csrc = os.path.join(ROOT, "ltx-2-mlx_amd", "csrc")
    out = tmp_path / "loop.inc"
    subprocess.check_call([sys.executable, os.path.join(csrc, "gen_gemm_v4.py"), str(out)], stdout=subprocess.DEVNULL)
    assert out.read_bytes() == open(os.path.join(csrc, "gemm_v4_loop.inc"), "rb").read()


def _load_generate():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    return generate


def test_cli_accepts_every_reference_flag():
    """Drop-in boundary: every argument of the reference's parser (scripts/generate.py:2364-2641, pinned in
    tests/golden/generate_cli_flags.json by tools/pin_generate_cli.py) exists here with the same flag strings, type, default,
    choices and action, and main()'s mapping onto generate_video keywords is the reference's (:2658-2725): the reference's own
    expressions are evaluated over a namespace parsed by THIS parser and compared keyword by keyword."""
    import json
    gen = _load_generate()
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "generate_cli_flags.json")))
    assert len(gold["flags"]) == 57
    parser = gen.build_parser()
    acts = {}
    for a in parser._actions:
        for s in (a.option_strings or [a.dest]):
            acts[s] = a
    types = {"int": int, "float": float, "str": str}
    sample = {int: "3", float: "0.25", str: "x"}
    argv = ["a prompt"]
    for f in gold["flags"]:
        a = acts[f["flags"][0]]
        for s in f["flags"]:
            assert acts[s] is a, s
        if f["flags"] == ["prompt"]:
            continue
        action = f.get("action", "store")
        assert type(a).__name__ == {"store": "_StoreAction", "store_true": "_StoreTrueAction", "append": "_AppendAction"}[action], f
        if "type" in f:
            assert a.type is types[f["type"]], f
        assert a.default == f.get("default", False if action == "store_true" else None), f
        assert (list(a.choices) if a.choices else None) == f.get("choices"), f
        if "dest" in f:
            assert a.dest == f["dest"]
        # a non-default legal value for every flag
        if action == "store_true":
            argv.append(f["flags"][-1])
        else:
            val = f["choices"][-1] if "choices" in f else sample[types[f["type"]]]
            argv += [f["flags"][0], val]
    args = parser.parse_args(argv)
    import copy
    ours = gen.kwargs_from_args(copy.copy(args))
    # the reference's main() edits args.weights / args.steps first (:2644-2656); replay that on a copy, then its expressions
    ref_args = copy.copy(args)
    if ref_args.model_variant == "dev":
        ref_args.weights = ref_args.weights.replace("distilled", "dev")
        if ref_args.steps == 7:
            ref_args.steps = 30
    if ref_args.fp8 and ".safetensors" in ref_args.weights and "-fp8" not in ref_args.weights:
        ref_args.weights = ref_args.weights.replace(".safetensors", "-fp8.safetensors")
    assert len(gold["generate_video_kwargs"]) == 56
    for k, expr in gold["generate_video_kwargs"].items():
        assert ours[k] == eval(expr, {"args": ref_args, "getattr": getattr}), (k, expr)
    # and with no flags at all: the reference's defaults reach generate_video unchanged
    d = gen.kwargs_from_args(parser.parse_args(["p"]))
    dref = parser.parse_args(["p"])
    for k, expr in gold["generate_video_kwargs"].items():
        assert d[k] == eval(expr, {"args": dref, "getattr": getattr}), k
    import inspect
    sig = inspect.signature(gen.generate_video).parameters
    assert set(ours) <= set(sig), set(ours) - set(sig)


def _write_ckpt(path, tensors, config=None, version=None):
    import json
    from safetensors.torch import save_file
    md = {}
    if config is not None:
        md["config"] = json.dumps(config)
    if version is not None:
        md["model_version"] = version
    save_file(tensors, str(path), metadata=md or None)


def test_checkpoint_metadata_drives_model_construction(tmp_path, monkeypatch):
    """The reference reads the architecture from the safetensors metadata (scripts/generate.py:142-152, 224-254) and builds the
    VAE decoder (:1255-1266) and the AudioVideo / LTX-2.3 transformer (:1073-1074, 1158-1164) from it.  Tiny safetensors files WITH
    metadata (an LTX-2.0-style record and a "2.3.0" one) go through the same helpers here; the constructors are spied on, so this
    runs without a GPU."""
    import torch
    gen = _load_generate()
    blocks = [["res_x", {"num_layers": 2}], ["compress_all", {"multiplier": 2, "residual": True}], ["res_x", {"num_layers": 1}],
              ["compress_time", {"multiplier": 1}], ["res_x", {"num_layers": 1}]]
    v1, v23, bare = tmp_path / "v1.safetensors", tmp_path / "v23.safetensors", tmp_path / "bare.safetensors"
    t = {"x": torch.zeros(2)}
    _write_ckpt(v1, t, {"vae": {"decoder_blocks": blocks, "decoder_base_channels": 64, "timestep_conditioning": False}, "vocoder": {}}, "2.0.1")
    _write_ckpt(v23, t, {"vae": {"decoder_base_channels": 32}}, "2.3.0")
    _write_ckpt(bare, t)
    assert gen.detect_model_version(str(v1)) == "2.0.1" and not gen.is_v2_model(str(v1))
    assert gen.detect_model_version(str(v23)) == "2.3.0" and gen.is_v2_model(str(v23))
    assert gen.detect_model_version(str(bare)) == "" and not gen.is_v2_model(str(bare))
    assert gen.detect_model_version(str(tmp_path / "missing.safetensors")) == "" and gen.get_vae_config(str(tmp_path / "missing.safetensors")) == {}
    assert gen.get_vae_config(str(v1)) == {"decoder_blocks": blocks, "decoder_base_channels": 64, "timestep_conditioning": False}
    assert gen.get_vae_config(str(bare)) == {} and gen._read_checkpoint_config(str(v23)) == {"vae": {"decoder_base_channels": 32}}

    made = []

    class SpyDecoder:
        def __init__(self, **kw):
            made.append(kw)

        def init_random_weights(self, seed=0):
            made[-1]["random"] = seed

    monkeypatch.setattr(gen, "SimpleVideoDecoder", SpyDecoder)
    monkeypatch.setattr(gen, "load_vae_decoder_weights", lambda dec, path: made[-1].update(loaded=path))
    gen.create_vae_decoder(str(v1), device="cpu")
    assert made[-1] == dict(decoder_blocks=blocks, base_channels=64, timestep_conditioning=False, device="cpu", loaded=str(v1))
    gen.create_vae_decoder(str(v23), device="cpu")          # absent keys take the reference's defaults (:1258-1260)
    assert made[-1] == dict(decoder_blocks=None, base_channels=32, timestep_conditioning=True, device="cpu", loaded=str(v23))
    gen.create_vae_decoder(None, device="cpu", seed=7)
    assert made[-1] == dict(decoder_blocks=None, base_channels=128, timestep_conditioning=True, device="cpu", random=7)
    gen.create_vae_decoder(str(v1), device="cpu", base_channels_override=16)
    assert made[-1]["base_channels"] == 16

    # routing of generate_video: which transformer loader gets which architecture arguments
    class Routed(Exception):
        pass

    def spy(name):
        def f(*a, **k):
            raise Routed(name, a, k)
        return f

    monkeypatch.setattr(gen, "load_transformer", spy("video"))
    monkeypatch.setattr(gen, "load_av_transformer", spy("av"))
    kw = dict(use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"))
    with pytest.raises(Routed) as e:
        gen.generate_video("p", weights_path=str(v1), **kw)
    assert e.value.args[0] == "video" and e.value.args[2]["caption_channels"] == 3840
    with pytest.raises(Routed) as e:
        gen.generate_video("p", weights_path=str(v1), generate_audio=True, **kw)
    assert e.value.args[0] == "av" and e.value.args[1] == (str(v1),)
    assert {k: e.value.args[2][k] for k in ("caption_channels", "cross_attention_adaln", "apply_gated_attention")} == \
        dict(caption_channels=3840, cross_attention_adaln=False, apply_gated_attention=False)
    with pytest.raises(Routed) as e:                        # LTX-2.3: always the AV transformer, V2 blocks, no caption projection
        gen.generate_video("p", weights_path=str(v23), **kw)
    assert e.value.args[0] == "av"
    assert {k: e.value.args[2][k] for k in ("caption_channels", "cross_attention_adaln", "apply_gated_attention", "num_layers")} == \
        dict(caption_channels=None, cross_attention_adaln=True, apply_gated_attention=True, num_layers=48)
    with pytest.raises(Routed) as e:                        # no checkpoint on disk + model_version: the same architecture, random init
        gen.generate_video("p", weights_path=None, model_version="2.3", **kw)
    assert e.value.args[0] == "av" and e.value.args[2]["cross_attention_adaln"] is True
    # pipelines the reference knows but this path does not build are refused by name; unknown names are a ValueError
    for pt in ("two-stage", "ic-lora", "keyframe-interpolation"):
        with pytest.raises(NotImplementedError, match=pt):
            gen.generate_video("p", pipeline_type=pt, **kw)
    with pytest.raises(ValueError, match="unknown pipeline_type"):
        gen.generate_video("p", pipeline_type="bogus", **kw)
    with pytest.raises(NotImplementedError, match="cfg_scale"):
        gen.generate_video("p", model_variant="dev", **kw)      # dev model: cfg 5.0 stays on -> classifier-free guidance


def test_one_stage_config_and_guidance_gate():
    """OneStageCFGConfig keeps the reference's fields / defaults / validation (pipelines/one_stage.py:52-110); the pipeline runs
    only its guidance-free branches and says so for everything else."""
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    c = OneStageCFGConfig()
    assert (c.height, c.width, c.num_frames, c.seed, c.fps, c.num_inference_steps) == (480, 704, 97, 42, 24.0, 30)
    assert (c.cfg_scale, c.audio_cfg_scale, c.rescale_scale, c.audio_enabled, c.use_internal_audio_branch) == (3.0, 7.0, 0.7, False, True)
    assert (c.audio_vae_channels, c.audio_mel_bins, c.audio_sample_rate, c.audio_hop_length, c.audio_downsample_factor, c.audio_output_sample_rate) == \
        (8, 16, 16000, 160, 4, 24000)
    assert c._get_tiling_config() is not None                       # 13 x 15 x 22 = 4290 latent voxels > 4000
    assert OneStageCFGConfig(height=512, width=768, num_frames=65)._get_tiling_config() is None     # 9 x 16 x 24 = 3456
    with pytest.raises(ValueError, match="8\\*k \\+ 1"):
        OneStageCFGConfig(num_frames=96)
    with pytest.raises(ValueError, match="divisible by 32"):
        OneStageCFGConfig(height=500)
    gate = OneStagePipeline._require_no_guidance
    gate(0.0, None, 0.0, "euler", None, 1.0)
    gate(-1.0, None, -0.5, "euler", None, 1.0)          # the reference enables STG / GE only for values > 0 (one_stage.py:867, :301)
    for bad in (dict(stg_scale=1.0), dict(ge_gamma=2.0),
                dict(sampler="heun"), dict(temporal_upscaler=object()), dict(cross_attn_scale=5.0), dict(guider_override=object())):
        a = dict(stg_scale=0.0, guider_override=None, ge_gamma=0.0, sampler="euler", temporal_upscaler=None, cross_attn_scale=1.0)
        a.update(bad)
        with pytest.raises(NotImplementedError):
            gate(**a)


def test_guiders_match_reference():
    """CFGGuider / CFGStarRescalingGuider / projection_coef against the vectors recorded from the reference's own components/guiders.py
    (tests/golden/guiders.npz, tools/pin_oracle_against_reference.py guiders)."""
    import numpy as np
    from ltx_2_mlx_amd.components import CFGGuider, CFGStarRescalingGuider, projection_coef
    z = np.load(os.path.join(ROOT, "tests", "golden", "guiders.npz"))
    g = torch.Generator().manual_seed(4242)
    cond = torch.randn(1, 48, 128, generator=g)
    uncond = 0.7 * cond + 0.5 * torch.randn(1, 48, 128, generator=g)
    assert np.allclose(projection_coef(cond, uncond).numpy(), z["projection_coef"], rtol=1e-5, atol=1e-6)
    for sc in (1.0, 3.0, 7.0):
        assert np.allclose(CFGGuider(scale=sc).guide(cond, uncond).numpy(), z[f"cfg_{sc}"], rtol=1e-5, atol=1e-5)
        assert np.allclose(CFGStarRescalingGuider(scale=sc).guide(cond, uncond).numpy(), z[f"cfgstar_{sc}"], rtol=1e-5, atol=1e-5)
    assert not CFGGuider(scale=1.0).enabled() and not CFGStarRescalingGuider(scale=1.0).enabled() and CFGGuider(scale=3.0).enabled()
    assert torch.equal(CFGGuider(scale=1.0).guide(cond, uncond), cond)


def test_gemm_dispatch_routes_of_every_model_gemm():
    """every dispatch branch is a parity surface.  The route of EVERY dense GEMM the three models issue at the BASELINE
    geometry (19B VideoOnly at 768x512x65 and at the two-stage 1536x1024x65 size, AudioVideo 19B-style and LTX-2.3) is pinned, for bf16
    weights, fp8-resident weights and the fp8 compute mode -- so kernel work cannot silently strand a shape on a slow path.  Host logic
    only (ltx2_gemm_route launches nothing)."""
    from ltx_2_mlx_amd import _native as nv
    L = nv.lib()
    R = {k: getattr(nv, k) for k in dir(nv) if k.startswith("ROUTE_")}
    name = {v: k for k, v in R.items()}
    BF, GELU, F32, RES = nv.EPI_BF16, nv.EPI_GELU_BF16, nv.EPI_F32, nv.EPI_RESID_GATE_F32

    def route(M, N, K, epi, weights=0, vt=0):
        r = L.ltx2_gemm_route(M, N, K, epi, weights, vt)
        return (name.get(r & 0xff, r), bool(r & 0x100)) if r >= 0 else ("INVALID", False)

    D, Da, S, cap = 4096, 2048, 1024, 3840
    for N in (3456, 13824):                          # 768x512x65 and the stage-2 grid of 1536x1024x65
        layer = [("attn1.to_qkv", N, 3 * D, D, BF, 1), ("attn1.to_out", N, D, D, RES, 0), ("attn2.to_q", N, D, D, BF, 0),
                 ("attn2.to_out", N, D, D, RES, 0), ("ff.net.0", N, 4 * D, D, GELU, 0), ("ff.net.2", N, D, 4 * D, RES, 0)]
        for nm, M, Nn, K, epi, vt in layer:
            # 224-row tiles wherever they need fewer CU-rounds than 256-row tiles: everywhere but the 13824 x 16384 grid (a tie -> 256)
            t = "256" if (N == 13824 and Nn == 4 * D) else "224"
            assert route(M, Nn, K, epi, 0, vt) == ("ROUTE_V4_" + t, bool(vt)), (nm, N)
            assert route(M, Nn, K, epi, 1, vt) == ("ROUTE_V4_W8_" + t, bool(vt)), (nm, N)       # fp8-resident weights
            # fp8 compute: 224-row tiles run the 16x16x128 block (layout 6) and also win ties and near-ties (gemm.h: gemm_v4_prefer_224)
            assert route(M, Nn, K, epi, 2, vt) == ("ROUTE_V4_F8_224", bool(vt)), (nm, N)
        assert route(N, D, 128, F32)[0] == "ROUTE_PP"                    # patchify_proj: K = 128 is below the asm loop's minimum
        assert route(N, 128, D, F32)[0] == "ROUTE_SMALL"                 # proj_out: 128 output channels
        assert route(N, D, 256, nv.EPI_SILU_BF16)[0] == "ROUTE_V4_224"   # per-token AdaLN MLP (image conditioning)
        assert route(N, 6 * D, D, F32)[0] == ("ROUTE_V4_224" if N == 3456 else "ROUTE_V4_256")
    # per-prompt setup (S = 1024 text tokens): caption projection on the 128x128 tile, the fused text K/V projection on the asm-loop kernel
    assert route(S, D, cap, GELU)[0] == "ROUTE_SMALL" and route(S, D, D, BF)[0] == "ROUTE_SMALL"
    assert route(S, 2 * D, D, BF)[0] == "ROUTE_V4_224" and route(S, 2 * D, D, BF, 1)[0] == "ROUTE_V4_W8_224"
    # AudioVideo: the 68-token audio stream streams its weights (skinny kernel); cross-modal projections of the video tokens
    Na = 68
    for nm, M, Nn, K, epi in [("audio qkv", Na, 3 * Da, Da, BF), ("audio to_out", Na, Da, Da, RES), ("audio ff1", Na, 4 * Da, Da, GELU),
                              ("audio ff2", Na, Da, 4 * Da, RES), ("a2v kv", Na, 2 * Da, Da, BF), ("v2a q", Na, Da, Da, BF), ("v2a to_out", Na, Da, Da, RES)]:
        assert route(M, Nn, K, epi)[0] == "ROUTE_SKINNY", nm
    assert route(3456, Da, D, BF)[0] == "ROUTE_SMALL"                    # a2v query projection: 128 big tiles lose to the small tile (68 vs ~89 us)
    assert route(3456, 2 * Da, D, BF)[0] == "ROUTE_V4_224"               # v2a K/V from the video tokens
    assert route(3456, D, Da, RES)[0] == "ROUTE_V4_224"                  # a2v to_out
    assert route(S, 2 * Da, Da, BF)[0] == "ROUTE_SMALL"                  # audio text K/V (LTX-2.3: per step)
    # unsupported fp8 problems are refused, not rerouted
    assert route(3456, 4096, 384, BF, 2)[0] == "INVALID" and route(3456, 200, 4096, BF, 1)[0] == "INVALID"
    import re
    src = "".join(open(os.path.join(ROOT, "ltx-2-mlx_amd", "csrc", f)).read() for f in os.listdir(os.path.join(ROOT, "ltx-2-mlx_amd", "csrc")) if f.endswith((".hip", ".h")))
    assert set(re.findall(r'getenv\("(\w+)"\)', src)) == set(), "tuning switches belong in A/B builds (tools/ab_build.py + LTX2HIP_LIB), not in the product"


_ROUTE_GRID = ((1, 16, 64, 128, 129, 512, 1023, 1024, 1100, 3456, 4096, 13824),                 # M
               (48, 64, 128, 200, 256, 2048, 4096, 8192, 10240, 12288, 16384),                  # N
               (64, 128, 192, 256, 384, 512, 3840, 4096, 16384, 188160),                        # K
               range(6), range(3), range(2))                                                    # epilogue, weights, has_vt
_ROUTE_GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_routes.txt")


def _gemm_route_table(L):
    """One character per cell of the full cross product of _ROUTE_GRID, has_vt fastest: 'A' + (route + 1) + 11 * fused (ROUTE_INVALID = -1)."""
    import itertools
    out = []
    for cell in itertools.product(*_ROUTE_GRID):
        r = L.ltx2_gemm_route(*cell)
        out.append(chr(65 + (r & 0xff) + 1 + (11 if r & 0x100 else 0)) if r >= 0 else "A")
    return "".join(out)


def test_gemm_route_table_matches_the_recorded_dispatch():
    """The whole dispatch surface against a table recorded BEFORE gemm_route() became the launcher's only decider: every (M, N, K,
    epilogue, weights, has_vt) of _ROUTE_GRID (47 520 cells, none skipped), route byte and fused-V^T bit.  tests/golden/gemm_routes.txt was
    written from a library built at the parent commit of that change (never from the code under test), by
        LTX2HIP_LIB=<parent build>/libltx2hip.so python -c "from tests import test_host_cpu as t; from ltx_2_mlx_amd import _native as nv;
        open(t._ROUTE_GOLDEN, 'w').write(t._gemm_route_table(nv.lib()))"
    A deliberate re-plan of a route re-records the table the same way, from the build that carries the new plan."""
    import itertools
    import torch
    from ltx_2_mlx_amd import _native as nv
    want = open(_ROUTE_GOLDEN).read()
    cells = list(itertools.product(*_ROUTE_GRID))
    assert len(want) == len(cells) == 47520
    dec = lambda ch: ((ord(ch) - 65) % 11 - 1, (ord(ch) - 65) // 11)      # (route, fused)
    for dt in (torch.bfloat16, torch.float16):          # both builds carry the same host logic
        got = _gemm_route_table(nv.lib(dt))
        if got != want:
            i = next(j for j in range(len(cells)) if got[j] != want[j])
            raise AssertionError(f"{dt}: (M, N, K, epilogue, weights, vt) = {cells[i]}: (route, fused) = {dec(got[i])}, recorded {dec(want[i])}")


def _binding_kinds(fn_node):
    """name -> set of kinds it is bound to inside one function body (nested functions are their own scope).  kind: "ctor:<dotted call>" when the
    value is a call whose last attribute is Capitalised (torch.Generator(...), torch.cuda.Stream(), LTXModel(...)), else a coarse tag."""
    import ast

    def dotted(f):
        parts = []
        while isinstance(f, ast.Attribute):
            parts.append(f.attr)
            f = f.value
        if isinstance(f, ast.Name):
            parts.append(f.id)
        return ".".join(reversed(parts))

    def kind_of(v, idx=None):
        if idx is not None:
            return f"unpack[{idx}]:{dotted(v.func) if isinstance(v, ast.Call) else type(v).__name__}"
        if isinstance(v, ast.Call):
            d = dotted(v.func)
            return ("ctor:" if d.split(".")[-1][:1].isupper() else "call:") + d
        if isinstance(v, ast.Constant):
            return "const:" + type(v.value).__name__
        return "expr:" + type(v).__name__

    kinds = {}

    def bind(target, value, idx=None):
        if isinstance(target, ast.Name):
            kinds.setdefault(target.id, set()).add(kind_of(value, idx))
        elif isinstance(target, (ast.Tuple, ast.List)):
            for i, t in enumerate(target.elts):
                bind(t, value, i)

    def walk(node):
        for ch in ast.iter_child_nodes(node):
            if isinstance(ch, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda, ast.ClassDef)):
                continue
            if isinstance(ch, ast.Assign):
                for t in ch.targets:
                    bind(t, ch.value)
            elif isinstance(ch, (ast.For, ast.comprehension)):
                bind(ch.target, ch.iter, 0)
            elif isinstance(ch, ast.With):
                for it in ch.items:
                    if it.optional_vars is not None:
                        bind(it.optional_vars, it.context_expr)
            walk(ch)
    walk(fn_node)
    return kinds


def test_bench_never_rebinds_an_object_name():
    """Round 4's bench line was lost to `_, g = timed(...)` rebinding the torch.Generator `g` to a float, in a branch only the driver's K = 20
    takes.  In every function of bench.py a name bound to a constructed object (torch.Generator, torch.cuda.Stream, a model ...) is never bound to
    anything of another kind, and one-letter generator names are gone from main()."""
    import ast
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    bad = []
    for fn in ast.walk(tree):
        if not isinstance(fn, ast.FunctionDef):
            continue
        for name, ks in _binding_kinds(fn).items():
            ctors = {k for k in ks if k.startswith("ctor:")}
            others = ks - ctors - {"const:NoneType"}
            if ctors and (others or len(ctors) > 1):
                bad.append((fn.name, name, sorted(ks)))
    assert not bad, bad
    # the checker itself: the round-4 shape is caught
    probe = ast.parse("def f():\n    g = torch.Generator()\n    if x:\n        _, g = timed(run, 8)\n    return g\n").body[0]
    ks = _binding_kinds(probe)["g"]
    assert any(k.startswith("ctor:") for k in ks) and any(k.startswith("unpack") for k in ks)
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    assert "g" not in _binding_kinds(main)
    # the defaults are the driver's argv (`--steps 20 --warmup 5`): a bare `python bench.py` takes the driver's branch
    assert 'add_argument("--steps", type=int, default=20' in src and 'add_argument("--warmup", type=int, default=5' in src
