"""The stage helpers every pipeline shares (pipelines/common.py), on stub objects: the statistics rule of the x2 upscale, the final decode,
the automatic tiling threshold, the side-stream capture and the per-stage callback.  No GPU."""
import pytest
import torch


class _Stats:
    """un_normalize adds `shift`, normalize subtracts it again and tags the result with `tag`, so a test sees whose statistics ran."""

    def __init__(self, shift, tag):
        self.shift, self.tag = shift, tag

    def un_normalize(self, x):
        return x + self.shift

    def normalize(self, x):
        return x - self.shift + self.tag


class _Vae:
    def __init__(self, stats=None, loaded=None):
        self.per_channel_statistics = stats
        if loaded is not None:
            self._loaded = loaded


def _double(x):
    return 2 * x


def test_upscale_takes_the_encoder_statistics_only_when_it_is_loaded():
    from ltx_2_mlx_amd.pipelines.common import upscale_latent_x2
    lat = torch.arange(6.0).reshape(1, 1, 1, 2, 3)
    enc, dec = _Stats(1.0, 100.0), _Stats(3.0, 200.0)
    want_enc, want_dec = 2 * (lat + 1.0) - 1.0 + 100.0, 2 * (lat + 3.0) - 3.0 + 200.0
    assert torch.equal(upscale_latent_x2(lat, _double, _Vae(enc, loaded=True), _Vae(dec)), want_enc)
    assert torch.equal(upscale_latent_x2(lat, _double, _Vae(enc), _Vae(dec)), want_enc)              # no _loaded attribute: trusted
    assert torch.equal(upscale_latent_x2(lat, _double, _Vae(enc, loaded=False), _Vae(dec)), want_dec)
    assert torch.equal(upscale_latent_x2(lat, _double, None, _Vae(dec)), want_dec)
    for encoder, decoder in ((None, None), (_Vae(None), _Vae(None)), (_Vae(enc, loaded=False), None)):
        with pytest.raises(ValueError, match="per_channel_statistics"):
            upscale_latent_x2(lat, _double, encoder, decoder)


def test_decode_video_paths(monkeypatch):
    from ltx_2_mlx_amd.pipelines import common
    lat, dec, tiling = torch.zeros(1, 2, 3, 1, 1), object(), object()
    a, b = torch.ones(1, 3, 4, 2, 2), torch.full((1, 3, 5, 2, 2), 2.0)
    seen = []

    def tiled(chunks):
        def f(latent, decoder, cfg):
            seen.append(("tiled", latent is lat, decoder is dec, cfg is tiling))
            return iter(chunks)
        return f

    def plain(latent, decoder):
        seen.append(("plain", latent is lat, decoder is dec))
        return a

    monkeypatch.setattr(common, "decode_latent", plain)
    monkeypatch.setattr(common, "decode_tiled", tiled([a]))
    assert common.decode_video(lat, None, tiling) is lat and common.decode_video(lat, None, None) is lat and seen == []
    assert common.decode_video(lat, dec, tiling) is a and seen == [("tiled", True, True, True)]
    monkeypatch.setattr(common, "decode_tiled", tiled([a, b]))
    out = common.decode_video(lat, dec, tiling)
    assert out.shape == (1, 3, 9, 2, 2) and torch.equal(out, torch.cat([a, b], dim=2))
    seen.clear()
    assert common.decode_video(lat, dec, None) is a and seen == [("plain", True, True)]


def test_auto_tiling_config_threshold():
    from ltx_2_mlx_amd.model.video_vae import TilingConfig
    from ltx_2_mlx_amd.pipelines.common import auto_tiling_config
    given = TilingConfig.default()
    assert auto_tiling_config(given, 9, 64, 64) is given and auto_tiling_config(given, 65, 1024, 1536) is given
    assert auto_tiling_config(None, 65, 512, 768) is None                                # 9 x 16 x 24 = 3456 voxels
    assert auto_tiling_config(None, 65, 1024, 1536) == TilingConfig.default()            # 9 x 32 x 48 = 13824 > 4000


def test_capture_and_replay_runs_both_once_on_the_side_stream(monkeypatch):
    from ltx_2_mlx_amd.pipelines import common
    log = []

    class Stream:
        def __init__(self, name="side"):
            self.name = name

        def wait_stream(self, other):
            log.append((self.name, "waits for", other.name))

        def __enter__(self):
            log.append("enter")

        def __exit__(self, *a):
            log.append("exit")
            return False

    monkeypatch.setattr(torch.cuda, "Stream", Stream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: Stream("current"))
    monkeypatch.setattr(torch.cuda, "stream", lambda s: s)
    common.capture_and_replay(lambda: log.append("capture"), lambda: log.append("replay"))
    assert log == [("side", "waits for", "current"), "enter", "capture", "replay", "exit", ("current", "waits for", "side")]


def test_stage_callback_forwards_the_stage_name_first():
    from ltx_2_mlx_amd.pipelines.common import stage_callback
    assert stage_callback(None, "stage1") is None
    seen = []
    cb = stage_callback(lambda *a: seen.append(a), "stage2")
    cb(1, 3)
    cb(3, 3)
    assert seen == [("stage2", 1, 3), ("stage2", 3, 3)]
