"""Leaf tests of the VAE glue kernels of csrc/vae_glue.hip, the cast of csrc/rowops.hip and the plain sampler step of csrc/sampler.hip: tile blend, chunk cross-fade, uint8
conversion, unpatchify, latent (un)normalise, space-to-depth downsample, fp32 -> 16-bit cast, x0 / Euler step.

These kernels are index arithmetic (LDS transposes, space-to-depth channel orders, tile offsets, grid-stride loops, ragged tails), and most
are written as bit-exact replacements of separate torch ops (`__fmul_rn` / `__fadd_rn`, no contraction -- or no arithmetic at all).  So the
reference is the plain CPU op sequence (fp32 op by op where the kernel claims bit-exactness, fp64 otherwise) and nearly every assertion is
equality.  Where the compiler may legally fuse a multiply-add the bound is DERIVED (u = 2^-24 is the fp32 unit roundoff, ulp16 the spacing
of the 16-bit output type at the exact result), never measured:

  prepare_latent   |got - exact| <= ulp16(exact)/2 + 4u (|l s| + |m| + |n ns|)
  s2d_downsample   |got - exact| <= ulp16(exact)/2 + (gs + 2) u (|y| + sum|x_q| / gs)
  x0_from_velocity |got - exact| <= 4u (|latent| + |ts v|)                       two roundings: the product, the difference
  euler_step       |got - exact| <= 4u (|x| + 2 k |x - d| + k |x0 m| + k |clean (1 - m)|),   k = |(s' - s) / s|
                   exact = x + (x - d) / s * (s' - s) with d = x0 m + clean (1 - m) and the fp32 values of s, s'.  Rigorous count: u |out|
                   for the last add; (x - d) k carries five roundings (the difference, 1/s, s' - s, two products) -> with |out| <= |x| +
                   k |x - d| that is 6u k |x - d| + u |x|; d itself carries <= 2u |x0 m| + 3u |clean (1 - m)| (1 - m, two products, the
                   sum), scaled by k.  Every coefficient is <= the 4u (or 8u) the bound grants; the mask terms vanish without a mask.

Every ratio |got - exact| / bound is recorded with conftest.measure() and must be <= 1.

Each kernel with a grid-stride loop gets one case past its grid cap (16384 blocks x 256 threads, cast: 4096 x 256 x 4 elements: 4 194 304
work items either way), so the stride loop and its tail run.  Kernels compiled per activation type run on the bfloat16 and float16 builds.
Only freshly allocated contiguous tensors are passed."""
import numpy as np
import pytest
import torch

from conftest import measure

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(F16, id="f16")]
U = 2.0 ** -24
CAP = 4 * 1024 * 1024          # work items one launch covers before the grid-stride loop takes its second trip


@pytest.fixture(scope="module")
def K(dev):
    import ltx_2_mlx_amd.kernels as k
    return k


@pytest.fixture(scope="module")
def nv(dev):
    from ltx_2_mlx_amd import _native
    return _native


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ulp16(x, dtype):
    """Spacing of `dtype` (bfloat16: 8 significand bits, emin -126; float16: 11, -14) at |x|, as fp64."""
    p, emin = (8, -126) if dtype == BF else (11, -14)
    x = x.double().abs()
    _, e = torch.frexp(x)                                   # |x| = m 2^e, m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return torch.ldexp(torch.ones_like(x), e - (p - 1))


def bits16(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------ 1. tile_blend_accumulate / tile_blend_finish
def blend_ref(out, wsum, tile, nt, nh, nw, mt, mh, mw, t0, h0, w0):
    """The three fp32 statements of oracle.vae.decode_tiled on out [3,OT,OH,OW] / wsum [OT,OH,OW] (in place)."""
    mask = (mt[:, None, None] * mh[None, :, None]) * mw[None, None, :]
    out[:, t0:t0 + nt, h0:h0 + nh, w0:w0 + nw] += tile[:, :nt, :nh, :nw] * mask
    wsum[t0:t0 + nt, h0:h0 + nh, w0:w0 + nw] += mask


def finish_ref(out, wsum):
    return out / torch.clamp(wsum, min=1e-8)


def test_tile_blend_cropped_tile(K, dev):
    """(a) one tile cropped on every axis at a non-zero offset of a non-square volume; everything outside the window keeps its sentinel."""
    g = gen(11)
    OT, OH, OW = 5, 7, 11
    dt, dh, dw, nt, nh, nw, t0, h0, w0 = 4, 5, 6, 3, 4, 5, 1, 2, 3
    out0 = torch.randn(3, OT, OH, OW, generator=g) + 40.0          # sentinel: no accumulated value lands near 40
    w0s = torch.rand(OT, OH, OW, generator=g) + 40.0
    tile = torch.randn(3, dt, dh, dw, generator=g)
    mt, mh, mw = torch.rand(nt, generator=g), torch.rand(nh, generator=g), torch.rand(nw, generator=g)
    out, wsum = out0.to(dev), w0s.to(dev)
    K.tile_blend_accumulate(tile.to(dev), nt, nh, nw, mt.to(dev), mh.to(dev), mw.to(dev), out, wsum, t0, h0, w0)
    ro, rw = out0.clone(), w0s.clone()
    blend_ref(ro, rw, tile, nt, nh, nw, mt, mh, mw, t0, h0, w0)
    assert torch.equal(out.cpu(), ro) and torch.equal(wsum.cpu(), rw)
    outside = torch.ones(OT, OH, OW, dtype=torch.bool)
    outside[t0:t0 + nt, h0:h0 + nh, w0:w0 + nw] = False
    assert torch.equal(out.cpu()[:, outside], out0[:, outside]) and torch.equal(wsum.cpu()[outside], w0s[outside])
    assert not torch.equal(out.cpu()[:, ~outside], out0[:, ~outside])


def test_tile_blend_eight_overlapping_tiles(K, dev):
    """(b) eight tiles meeting at a 3-D corner, trapezoid masks built on the CPU, accumulated in sequence, then the finish.  (With (d), the
    test that caught the FMA hipcc made of __fadd_rn(out, __fmul_rn(tile, m)): out starts at 0, so the product's own rounding shows.)"""
    from ltx_2_mlx_amd.model.video_vae import compute_trapezoidal_mask_1d as trap
    g = gen(12)
    OT, OH, OW = 9, 12, 14
    spans = {"t": [(0, 6, 0, 3), (3, 9, 3, 0)], "h": [(0, 8, 0, 4), (4, 12, 4, 0)], "w": [(0, 9, 0, 4), (5, 14, 4, 0)]}   # start, end, ramps
    out, wsum = torch.zeros(3, OT, OH, OW, device=dev), torch.zeros(OT, OH, OW, device=dev)
    ro, rw, cover = torch.zeros(3, OT, OH, OW), torch.zeros(OT, OH, OW), torch.zeros(OT, OH, OW)
    for (t0, t1, tl, tr) in spans["t"]:
        for (h0, h1, hl, hr) in spans["h"]:
            for (w0, w1, wl, wr) in spans["w"]:
                nt, nh, nw = t1 - t0, h1 - h0, w1 - w0
                tile = torch.randn(3, nt + 1, nh + 2, nw + 3, generator=g)           # every tile is cropped to its window
                mt, mh, mw = trap(nt, tl, tr, left_starts_from_0=(t0 == 0)), trap(nh, hl, hr), trap(nw, wl, wr)
                K.tile_blend_accumulate(tile.to(dev), nt, nh, nw, mt.to(dev), mh.to(dev), mw.to(dev), out, wsum, t0, h0, w0)
                blend_ref(ro, rw, tile, nt, nh, nw, mt, mh, mw, t0, h0, w0)
                cover[t0:t1, h0:h1, w0:w1] += 1
    assert torch.equal(out.cpu(), ro) and torch.equal(wsum.cpu(), rw)
    assert float(rw.min()) > 0 and cover.min() == 1 and cover[4, 6, 7] == 8           # all eight tiles meet at the corner
    K.tile_blend_finish(out, wsum)
    assert torch.equal(out.cpu(), finish_ref(ro, rw))


def test_tile_blend_finish_zero_weight(K, dev):
    """(c) wsum == 0 (nothing accumulated there) gives exactly 0.0; weights under the 1e-8 clamp divide by the clamp; all finite."""
    g = gen(13)
    OT, OH, OW = 5, 7, 11
    wsum = torch.rand(OT, OH, OW, generator=g) * 3
    sel = torch.rand(OT, OH, OW, generator=g)
    wsum[sel < 0.3] = 0.0
    wsum[(sel >= 0.3) & (sel < 0.4)] = 3e-9                # below the clamp, with a non-zero numerator
    wsum[(sel >= 0.4) & (sel < 0.5)] = 1e-8
    out0 = torch.randn(3, OT, OH, OW, generator=g)
    out0[:, wsum == 0] = 0.0
    out = out0.to(dev)
    K.tile_blend_finish(out, wsum.to(dev))
    got = out.cpu()
    assert torch.equal(got, finish_ref(out0, wsum))
    assert bool(torch.isfinite(got).all()) and bool((got[:, wsum == 0] == 0).all())


def test_tile_blend_grid_stride(K, dev):
    """(d) 17 x 512 x 512 positions: past the 16384 x 256 cap of both kernels."""
    g = gen(14)
    nt, nh, nw = 17, 512, 512
    assert nt * nh * nw > CAP
    tile = torch.randn(3, nt, nh, nw, generator=g)
    mt, mh, mw = torch.rand(nt, generator=g), torch.rand(nh, generator=g), torch.rand(nw, generator=g)
    ro, rw = torch.randn(3, nt, nh, nw, generator=g), torch.rand(nt, nh, nw, generator=g)
    out, wsum = ro.to(dev), rw.to(dev)
    K.tile_blend_accumulate(tile.to(dev), nt, nh, nw, mt.to(dev), mh.to(dev), mw.to(dev), out, wsum, 0, 0, 0)
    blend_ref(ro, rw, tile, nt, nh, nw, mt, mh, mw, 0, 0, 0)
    assert torch.equal(out.cpu(), ro) and torch.equal(wsum.cpu(), rw)
    K.tile_blend_finish(out, wsum)
    assert torch.equal(out.cpu(), finish_ref(ro, rw))


def test_tile_blend_rejects_tile_outside_volume(K, dev):
    """(e) t0 + nt > OT (and the like) is an argument error; out and wsum are not touched."""
    g = gen(15)
    OT, OH, OW = 5, 7, 11
    out0, w0s = torch.randn(3, OT, OH, OW, generator=g), torch.rand(OT, OH, OW, generator=g)
    tile = torch.randn(3, 4, 5, 6, generator=g).to(dev)
    one = torch.ones(8, device=dev)
    out, wsum = out0.to(dev), w0s.to(dev)
    for (nt, nh, nw, t0, h0, w0) in [(3, 4, 5, 3, 0, 0), (3, 4, 5, 0, 4, 0), (3, 4, 5, 0, 0, 7), (5, 4, 5, 0, 0, 0)]:   # last: nt > dt
        with pytest.raises(ValueError, match="tile outside the volume"):
            K.tile_blend_accumulate(tile, nt, nh, nw, one, one, one, out, wsum, t0, h0, w0)
    assert torch.equal(out.cpu(), out0) and torch.equal(wsum.cpu(), w0s)


# ------------------------------------------------------------------------------------------ 2. video_to_uint8 / video_chunk_to_uint8
def boundary_values(with_inf):
    """For every k in 0..255 the fp32 value 2k/255 - 1 and its two fp32 neighbours (every truncation boundary of the uint8 conversion),
    then +-1, +-1.5, -0.0 and, optionally, +-inf.  No NaN: torch's NaN -> uint8 is undefined."""
    b = (2.0 * torch.arange(256, dtype=torch.float64) / 255.0 - 1.0).float()
    inf = torch.tensor(float("inf"))
    vals = [b, torch.nextafter(b, inf.expand_as(b)), torch.nextafter(b, -inf.expand_as(b)), torch.tensor([1.0, -1.0, 1.5, -1.5, -0.0])]
    if with_inf:
        vals.append(torch.tensor([float("inf"), -float("inf")]))
    return torch.cat(vals)


def video_values(shape, seed, with_inf):
    """fp32 tensor of `shape`: the boundary values scattered at random places among random values x 0.8."""
    g = gen(seed)
    n = int(np.prod(shape))
    v = torch.randn(n, generator=g) * 0.8
    b = boundary_values(with_inf)
    assert n >= 2 * b.numel()
    v[torch.randperm(n, generator=g)[:b.numel()]] = b
    return v.reshape(shape)


@pytest.fixture(scope="module")
def big_video():
    """prev [3,10,704,672] and cur [3,9,704,672]: 9 x 704 x 672 positions pass the grid cap (shared by both large uint8 cases)."""
    g = gen(21)
    assert 9 * 704 * 672 > CAP
    return torch.randn(3, 10, 704, 672, generator=g) * 0.8, torch.randn(3, 9, 704, 672, generator=g) * 0.8


def test_video_to_uint8_exact(K, dev):
    from oracle import vae
    v = video_values((3, 3, 13, 37), 22, with_inf=True)
    assert torch.equal(K.video_to_uint8(v.to(dev)).cpu(), vae.to_uint8_frames(v[None]))


def test_video_to_uint8_grid_stride(K, dev, big_video):
    from oracle import vae
    v = big_video[0]
    assert torch.equal(K.video_to_uint8(v.to(dev)).cpu(), vae.to_uint8_frames(v[None]))


def run_chunk(K, dev, cur, prev, T, overlap=2):
    """One video_chunk_to_uint8 call against to_uint8_frames(blend_chunks([prev, cur], T)): `cur` lands on frame prev_T - ov, frames past
    the trim are dropped, the frames before t_dst0 (which an earlier call owns) keep their sentinel."""
    from oracle import vae
    total = vae.latent_t_to_pixel_t(T)
    if prev is None:
        ref = vae.to_uint8_frames(vae.blend_chunks([cur[None]], T, overlap))
        t_dst0, ramp = 0, None
    else:
        ref = vae.to_uint8_frames(vae.blend_chunks([prev[None], cur[None]], T, overlap))
        ov = min(vae.latent_t_to_pixel_t(overlap), cur.shape[1], prev.shape[1])
        t_dst0, ramp = prev.shape[1] - ov, torch.linspace(0.0, 1.0, ov)
    T_out = min(total, ref.shape[0])
    assert ref.shape[0] == T_out
    frames = torch.full((T_out,) + tuple(cur.shape[2:]) + (3,), 77, dtype=torch.uint8, device=dev)
    K.video_chunk_to_uint8(cur.to(dev), frames, t_dst0, prev=None if prev is None else prev.to(dev), ramp=None if ramp is None else ramp.to(dev))
    got = frames.cpu()
    assert torch.equal(got[t_dst0:], ref[t_dst0:])
    assert bool((got[:t_dst0] == 77).all())
    return t_dst0, T_out


def test_video_chunk_no_prev(K, dev):
    cur = video_values((3, 9, 13, 37), 23, with_inf=True)
    assert run_chunk(K, dev, cur, None, T=2) == (0, 9)


def test_video_chunk_overlap_is_whole_chunk(K, dev):
    """ov == Tc: every frame of `cur` is blended (ov = min(9, Tc = 4, prev_T = 6))."""
    prev, cur = video_values((3, 6, 13, 37), 24, False), video_values((3, 4, 13, 37), 25, False)
    assert run_chunk(K, dev, cur, prev, T=3) == (2, 6)


def test_video_chunk_overlap_shorter_than_chunk(K, dev):
    """ov = 9 < Tc = 12 and prev_T = 11 > ov: the blend reads the LAST ov frames of prev, the rest of cur passes through."""
    prev, cur = video_values((3, 11, 13, 37), 26, False), video_values((3, 12, 13, 37), 27, False)
    assert run_chunk(K, dev, cur, prev, T=3) == (2, 14)


def test_video_chunk_trim(K, dev):
    """t_dst0 + Tc > T_out: 2 + 12 frames against a 9-frame output, the last five frames of cur are dropped."""
    prev, cur = video_values((3, 11, 13, 37), 28, False), video_values((3, 12, 13, 37), 29, False)
    assert run_chunk(K, dev, cur, prev, T=2) == (2, 9)


def test_video_chunk_grid_stride(K, dev, big_video):
    prev, cur = big_video
    assert run_chunk(K, dev, cur, prev, T=3) == (1, 10)


def test_video_chunk_rejects_bad_overlap(dev, nv):
    g = gen(30)
    Tc, pT, H, W = 4, 3, 5, 7
    cur, prev = torch.randn(3, Tc, H, W, generator=g).to(dev), torch.randn(3, pT, H, W, generator=g).to(dev)
    ramp = torch.linspace(0.0, 1.0, 8).to(dev)
    frames = torch.full((12, H, W, 3), 77, dtype=torch.uint8, device=dev)
    f = nv.lib().ltx2_video_chunk_to_uint8
    bad = [(nv.ptr(prev), nv.ptr(ramp), pT, 5),     # ov > Tc
           (nv.ptr(prev), nv.ptr(ramp), pT, 4),     # ov > prev_T
           (nv.ptr(prev), None, pT, 2)]             # prev without ramp
    for p, r, prev_T, ov in bad:
        assert f(nv.ptr(cur), p, r, nv.ptr(frames), Tc, prev_T, ov, H, W, 0, 12, nv.stream()) == nv.E_INVALID
        assert "bad overlap" in nv.last_error()
    assert bool((frames.cpu() == 77).all())


# ------------------------------------------------------------------------------------------ 3. vae_unpatchify
def run_unpatchify(nv, dev, dtype, T, H, W):
    from oracle import vae
    span = 256 if dtype == BF else 2048                    # integers up to 2^8 / 2^11 are exact in the type
    n = T * H * W * 48
    x = ((torch.arange(n) % (2 * span + 1)) - span).float().reshape(T, H, W, 48).to(dtype)
    assert torch.equal(x.float().flatten(), ((torch.arange(n) % (2 * span + 1)) - span).float())
    video = torch.full((3, T, 4 * H, 4 * W), float("nan"), device=dev)
    xd = x.to(dev)                                         # named: the raw pointer does not keep a temporary alive
    nv.check(nv.lib(dtype).ltx2_vae_unpatchify(nv.ptr(xd), nv.ptr(video), T, H, W, nv.stream()))
    ref = vae.unpatchify(x.float().permute(3, 0, 1, 2)[None].contiguous(), 4, 1)[0]
    assert torch.equal(video.cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_vae_unpatchify_exact(dev, nv, dtype):
    run_unpatchify(nv, dev, dtype, 2, 3, 5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_vae_unpatchify_grid_stride(dev, nv, dtype):
    assert 3 * 9 * 384 * 512 > CAP
    run_unpatchify(nv, dev, dtype, 9, 96, 128)


# ------------------------------------------------------------------------------------------ 4. vae_prepare_latent
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,P", [(128, 1), (128, 31), (128, 32), (128, 33), (128, 3 * 4 * 5), (48, 33), (130, 3 * 4 * 5)])
def test_vae_prepare_latent(dev, nv, dtype, C, P):
    g = gen(40 + C + P)
    lat, noise = torch.randn(C, P, generator=g), torch.randn(C, P, generator=g)
    std, mean = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    f = nv.lib(dtype).ltx2_vae_prepare_latent
    lat_d, noise_d, std_d, mean_d = lat.to(dev), noise.to(dev), std.to(dev), mean.to(dev)      # raw pointers keep nothing alive
    outs = {}
    for with_noise in (False, True):
        for ns in (0.0, 0.025):
            out = torch.full((P, C), float("nan"), device=dev, dtype=dtype)         # sentinel: every element must be written
            nv.check(f(nv.ptr(lat_d), nv.ptr(std_d), nv.ptr(mean_d), nv.ptr(noise_d) if with_noise else None, ns, nv.ptr(out), C, P,
                       nv.stream()))
            got = out.cpu()
            assert not bool(torch.isnan(got).any())
            ns32 = float(np.float32(ns))                                             # what the C ABI's float argument holds
            ls, m = lat.double() * std.double()[:, None], mean.double()[:, None]
            nn = noise.double() * ns32 if with_noise else torch.zeros(C, P, dtype=torch.float64)
            exact = ls + m
            if ns > 0:
                exact = nn + (1.0 - ns32) * exact
            else:
                nn = torch.zeros_like(nn)
            bound = 0.5 * ulp16(exact, dtype) + 4 * U * (ls.abs() + m.abs() + nn.abs())
            ratio = ((got.double().t() - exact).abs() / bound).max()
            measure(f"prepare_latent err/bound noise={int(with_noise)} ns={ns}", ratio)
            assert float(ratio) <= 1.0
            outs[(with_noise, ns)] = got
    assert torch.equal(bits16(outs[(False, 0.0)]), bits16(outs[(True, 0.0)]))         # noise_scale 0: the noise pointer is not read


# ------------------------------------------------------------------------------------------ 5. latent_normalize_nchw
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [128, 64, 48, 130])
def test_latent_normalize_nchw_exact(K, dev, dtype, C):
    """A subtraction, then a division: both correctly rounded, nothing to fuse -> the fp32 torch ops bit for bit."""
    for shape in [(1, 1, 1), (1, 1, 63), (1, 1, 64), (1, 1, 65), (2, 3, 7)]:
        g = gen(50 + C + shape[2])
        x = torch.randn(*shape, C, generator=g).to(dtype)
        mean, std = 0.3 * torch.randn(C, generator=g), 0.5 + 1.5 * torch.rand(C, generator=g)
        got = K.latent_normalize_nchw(x.to(dev), mean.to(dev), std.to(dev)).cpu()
        ref = ((x.float() - mean) / std).permute(3, 0, 1, 2).contiguous()
        ulps = (got.view(torch.int32).long() - ref.view(torch.int32).long()).abs().max()    # same sign wherever they differ by an ulp
        measure("latent_normalize fp32 ulps", ulps)
        assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------ 6. s2d_downsample
STRIDES = [(2, 2, 2), (1, 2, 2), (2, 1, 1), (1, 1, 1)]


def s2d_exact(y, x, Cc, stride):
    """oracle space_to_depth(y) + group mean of space_to_depth(x) on channels-last [T,H,W,C] inputs -> channels-last, in the inputs' type."""
    from oracle import vae_encoder as ve
    y5, x5 = y.permute(3, 0, 1, 2)[None], x.permute(3, 0, 1, 2)[None]
    sp = stride[0] * stride[1] * stride[2]
    ys, xs = ve.space_to_depth(y5, stride), ve.space_to_depth(x5, stride)
    cout = Cc * sp
    gs = xs.shape[1] // cout
    xg = xs.reshape(1, cout, gs, *xs.shape[2:])
    return (ys + xg.mean(2))[0].permute(1, 2, 3, 0), (ys.abs() + xg.abs().sum(2) / gs)[0].permute(1, 2, 3, 0), gs


def s2d_integer_input(T, H, W, C, stride, salt):
    """Integers in [-8, 8] (exact in both 16-bit types): (5 c + 3 s + 7 cell + salt) mod 17 - 8 with s the sub-position inside the stride
    cell.  5 and 3 are units mod 17, so exchanging two channels, or two sub-positions, that differ by less than 17 changes the value: a
    wrong channel order fails at nearly every element, not in the noise.  (17 integers cannot tell 128 x 8 pairs apart outright.)"""
    st, sh, sw = stride
    i32 = lambda n: torch.arange(n, dtype=torch.int32)
    t, h, w, c = i32(T)[:, None, None, None], i32(H)[None, :, None, None], i32(W)[None, None, :, None], i32(C)[None, None, None, :]
    s = ((t % st) * sh + (h % sh)) * sw + (w % sw)
    cell = ((t // st) * (H // sh) + (h // sh)) * (W // sw) + (w // sw)
    return ((5 * c + (3 * s + 7 * cell + salt) % 17) % 17 - 8).float()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", STRIDES, ids=lambda s: "s%d%d%d" % s)
@pytest.mark.parametrize("Cc,Cin", [(32, 128), (64, 64)])
def test_s2d_downsample_integer_exact(K, dev, dtype, stride, Cc, Cin):
    """(a) gs = 4 and 1: every fp32 step (the sum of gs integers, / gs, + y) is exact, and so is the single rounding to the type."""
    T, H, W = 4, 6, 10
    y, x = s2d_integer_input(T, H, W, Cc, stride, 0).to(dtype), s2d_integer_input(T, H, W, Cin, stride, 5).to(dtype)
    exact, _, gs = s2d_exact(y.double(), x.double(), Cc, stride)
    assert gs == Cin // Cc
    got = K.s2d_downsample(y.to(dev), x.to(dev), stride).cpu()
    assert got.shape == exact.shape
    assert torch.equal(bits16(got), bits16(exact.to(dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", STRIDES, ids=lambda s: "s%d%d%d" % s)
@pytest.mark.parametrize("Cc,Cin", [(32, 128), (64, 64), (16, 48)])
def test_s2d_downsample_random_bound(K, dev, dtype, stride, Cc, Cin):
    """(b) random inputs, gs = 4, 1 and 3 (1/3 is not exact): gs - 1 additions, the division, the final addition in fp32, one rounding."""
    T, H, W = 4, 6, 10
    g = gen(60 + Cc + stride[0] * 4 + stride[1])
    y, x = torch.randn(T, H, W, Cc, generator=g).to(dtype), torch.randn(T, H, W, Cin, generator=g).to(dtype)
    exact, mag, gs = s2d_exact(y.double(), x.double(), Cc, stride)
    got = K.s2d_downsample(y.to(dev), x.to(dev), stride).cpu()
    bound = 0.5 * ulp16(exact, dtype) + (gs + 2) * U * mag
    ratio = ((got.double() - exact).abs() / bound).max()
    measure(f"s2d err/bound gs={gs}", ratio)
    assert float(ratio) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_s2d_downsample_grid_stride(K, dev, dtype):
    T, H, W, Cc, Cin, stride = 4, 192, 192, 32, 128, (2, 2, 2)
    assert (T // 2) * (H // 2) * (W // 2) * Cc * 8 > CAP
    y, x = s2d_integer_input(T, H, W, Cc, stride, 0).to(dtype), s2d_integer_input(T, H, W, Cin, stride, 5).to(dtype)
    exact, _, _ = s2d_exact(y.float(), x.float(), Cc, stride)          # integers: fp32 is as exact as fp64 here, at half the memory
    got = K.s2d_downsample(y.to(dev), x.to(dev), stride).cpu()
    assert torch.equal(bits16(got), bits16(exact.to(dtype)))


def test_s2d_downsample_rejects_bad_shapes(K, dev):
    z = lambda *s: torch.zeros(*s, device=dev, dtype=BF)
    with pytest.raises(ValueError, match="dims must divide by the stride"):
        K.s2d_downsample(z(3, 6, 10, 32), z(3, 6, 10, 128), (2, 2, 2))
    with pytest.raises(ValueError, match="dims must divide by the stride"):
        K.s2d_downsample(z(4, 6, 9, 32), z(4, 6, 9, 128), (1, 2, 2))
    with pytest.raises(ValueError, match="must be a multiple of the conv width"):
        K.s2d_downsample(z(4, 6, 10, 32), z(4, 6, 10, 48), (2, 2, 2))


# ------------------------------------------------------------------------------------------ 7. cast_f32_bf16 (both builds)
def cast_specials():
    """fp32 bit patterns: +-0, +-inf, NaNs, fp32 subnormals, then for bfloat16 (16 dropped bits) and float16 (13 dropped bits, narrower
    exponent) exact ties with an even and an odd kept significand, their neighbours, the largest finite value, the first value that
    rounds to inf, and the ties of the types' own subnormal range."""
    bits = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001,
            0x00000001, 0x80000001, 0x00400000, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF,
            # bfloat16
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F817FFF, 0x3F807FFF, 0x3F818001,
            0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0xFF7F7FFF, 0xFF7F8000, 0x00008000, 0x00018000, 0x00008001,
            # float16: ties at 1 + 2^-11 (even -> down) and 1 + 3 2^-11 (odd -> up); 65504 is the largest finite, 65520 the tie to inf
            0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000, 0x3F801001, 0x3F802FFF, 0x3F800FFF, 0x3F803001,
            0x477FE000, 0x477FEFFF, 0x477FF000, 0xC77FEFFF, 0xC77FF000, 0x47800000,
            # float16 subnormals: 2^-24, the ties 2^-25 (-> 0) and 3 2^-25 (-> 2^-23), just above 2^-25, 2^-14 and its predecessor
            0x33800000, 0x33000000, 0x33C00000, 0x33000001, 0xB3000000, 0x38800000, 0x387FFFFF]
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, CAP + 5])
def test_cast_f32_exact(K, dev, dtype, n):
    """x.to(dtype) bit for bit (NaN-ness compared separately: the payload is not part of the contract)."""
    g = gen(70 + n % 1000)
    sp = cast_specials()
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 18, (n,), generator=g).float())
    if n >= 2 * sp.numel():
        x[:sp.numel()] = sp
        x[-5 - sp.numel():-5] = sp.flip(0)                 # and again next to the ragged tail
    else:
        x[:] = sp[torch.arange(n) + 15]                    # n <= 5: bfloat16 ties
    check_cast(K, dev, dtype, x)


def check_cast(K, dev, dtype, x):
    got, ref = K.cast_bf16(x.to(dev), dtype).cpu(), x.to(dtype)
    assert got.dtype == dtype and got.shape == ref.shape
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(bits16(got)[~nan], bits16(ref)[~nan])


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast_f32_specials_short(K, dev, dtype):
    """Every special value at lengths that end in the scalar tail (n = 4 q + 1, 2, 3) and in the vector body (4 q), from either end of
    the list so each value meets both the vector and the scalar path."""
    sp = cast_specials()
    for n in range(sp.numel() - 3, sp.numel() + 1):
        check_cast(K, dev, dtype, sp[:n].clone())
        check_cast(K, dev, dtype, sp[-n:].clone())


# ------------------------------------------------------------------------------------------ 8. x0_from_velocity / euler_step
SAMPLER_SHAPES = [(1031, 1), (77, 128), (32769, 128)]       # C = 1, C = 128, rows x C past the grid cap


@pytest.mark.parametrize("rows,C", SAMPLER_SHAPES)
@pytest.mark.parametrize("per_row", [False, True], ids=["scalar_ts", "row_ts"])
def test_x0_from_velocity_bound(K, dev, rows, C, per_row):
    g = gen(80 + C + rows % 7)
    lat, vel = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    ts = torch.rand(rows if per_row else 1, generator=g)
    got = K.x0_from_velocity(lat.to(dev), vel.to(dev), ts.to(dev)).cpu()
    tv = ts.double()[:, None] * vel.double()
    exact = lat.double() - tv
    ratio = ((got.double() - exact).abs() / (4 * U * (lat.double().abs() + tv.abs()))).max()
    measure("x0_from_velocity err/bound", ratio)
    assert float(ratio) <= 1.0


@pytest.mark.parametrize("rows,C", SAMPLER_SHAPES)
@pytest.mark.parametrize("mask_kind", ["none", "zeros", "ones", "mixed"])
def test_euler_step_bound(K, dev, rows, C, mask_kind):
    g = gen(90 + C + rows % 7)
    x, x0, clean = (torch.randn(rows, C, generator=g) for _ in range(3))
    sigma, sigma_next = 0.9, 0.7
    if mask_kind == "none":
        mask = None
    elif mask_kind == "mixed":
        mask = torch.rand(rows, generator=g)                # fractional weights, with hard 0 / 1 rows among them
        sel = torch.rand(rows, generator=g)
        mask[sel < 0.25], mask[sel > 0.75] = 0.0, 1.0
    else:
        mask = torch.full((rows,), 0.0 if mask_kind == "zeros" else 1.0)
    got = K.euler_step(x.to(dev), x0.to(dev), sigma, sigma_next, None if mask is None else mask.to(dev),
                       None if mask is None else clean.to(dev)).cpu()
    s, sn = float(np.float32(sigma)), float(np.float32(sigma_next))      # the C ABI takes fp32 sigmas
    xd = x.double()
    if mask is None:
        d, dmag = x0.double(), torch.zeros_like(xd)
    else:
        m = mask.double()[:, None]
        a, b = x0.double() * m, clean.double() * (1.0 - m)
        d, dmag = a + b, a.abs() + b.abs()
    k = abs((sn - s) / s)
    exact = xd + (xd - d) / s * (sn - s)
    bound = 4 * U * (xd.abs() + 2 * k * (xd - d).abs() + k * dmag)
    ratio = ((got.double() - exact).abs() / bound).max()
    measure(f"euler_step err/bound mask={mask_kind}", ratio)
    assert float(ratio) <= 1.0
    if mask_kind == "zeros":                                # the step then moves x towards `clean`, and x0 must not leak in
        other = K.euler_step(x.to(dev), (x0 + 3.0).to(dev), sigma, sigma_next, mask.to(dev), clean.to(dev)).cpu()
        assert torch.equal(other, got)


# ------------------------------------------------------------------------------------------ 9. the two host paths with a fake decoder
def fake_decoder(z, timestep=None, noise=None):
    """[1,128,t,h,w] -> fp32 [1,3,(t-1)*8+1,32h,32w] by gathers alone (no arithmetic on values: the CPU and the GPU give the same bits).
    Frame F reads latent frame (F+7)//8 -- frame 0 alone, then eight frames per latent frame, as the causal decoder lays them out, so a
    temporal tile that starts at latent frame t0 produces the frames from 8 t0 on -- and pixel (Y, X) reads cell (Y//32, X//32); the
    channel it reads depends on the output channel and on the offset inside the cell."""
    _, C, t, h, w = z.shape
    dev = z.device
    F, Y, X, c = (torch.arange(n, device=dev) for n in ((t - 1) * 8 + 1, 32 * h, 32 * w, 3))
    ch = (c[:, None, None, None] * 41 + ((F + 7) % 8)[None, :, None, None] * 17 + (Y % 32)[None, None, :, None] * 5
          + (X % 32)[None, None, None, :] * 3) % C
    return z[0].float()[ch, ((F + 7) // 8)[None, :, None, None], (Y // 32)[None, None, :, None], (X // 32)[None, None, None, :]][None]


def test_decode_tiled_with_fake_decoder(dev):
    from oracle import vae
    from ltx_2_mlx_amd.model.video_vae import SpatialTilingConfig, TemporalTilingConfig, TilingConfig, decode_tiled
    z = torch.randn(1, 128, 4, 4, 6, generator=gen(100))
    got = next(decode_tiled(z.to(dev), fake_decoder, TilingConfig(SpatialTilingConfig(96, 32), TemporalTilingConfig(16, 8)))).cpu()
    assert len(vae.tile_specs(z.shape, (96, 32), (16, 8))) == 3 * 2 * 3
    ref = vae.decode_tiled(z, fake_decoder, spatial=(96, 32), temporal=(16, 8))
    assert got.shape == ref.shape == (1, 3, 25, 128, 192)
    assert torch.equal(got, ref)
    # every tile decodes the same value at a pixel, so the blend returns it up to the roundings of <= 8 weighted terms and one division
    whole = fake_decoder(z)
    ratio = ((got.double() - whole.double()).abs() / (16 * U * whole.double().abs()).clamp_min(1e-300)).max()
    measure("decode_tiled vs untiled err/bound", ratio)
    assert float(ratio) <= 1.0


@pytest.mark.parametrize("T,chunk,overlap", [(8, 7, 2), (9, 7, 2), (12, 7, 2), (13, 7, 2), (5, 3, 1), (6, 3, 1)])
def test_decode_latent_with_fake_decoder(dev, T, chunk, overlap):
    """Default chunking (two chunks at T' = 8, 9, 12, three at 13) and chunk 3 / overlap 1, whose one-frame overlap takes the concatenate
    path and whose chunks add up to more frames than the video has (the final trim)."""
    from oracle import vae
    from ltx_2_mlx_amd.model.video_vae import decode_latent
    z = torch.randn(1, 128, T, 1, 2, generator=gen(110 + T)) * 0.8
    spans = vae.temporal_chunks(T, chunk, overlap)
    assert len(spans) == {8: 2, 9: 2, 12: 2, 13: 3, 5: 2, 6: 3}[T]
    chunks = [fake_decoder(z[:, :, s:e]) for s, e in spans]
    if overlap == 1:
        assert sum(c.shape[2] for c in chunks) > vae.latent_t_to_pixel_t(T)
    ref = vae.to_uint8_frames(vae.blend_chunks(chunks, T, overlap))
    got = decode_latent(z.to(dev), fake_decoder, temporal_chunk_size=chunk, temporal_overlap=overlap).cpu()
    assert got.shape == ref.shape == (vae.latent_t_to_pixel_t(T), 32, 64, 3)
    assert torch.equal(got, ref)
