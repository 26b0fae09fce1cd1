"""CPU checks of tests/attention_exact_ref.py: every condition the exact-arithmetic attention tests rest on, for every parametrisation
test_attention_exact_gpu.py runs, on the references alone (no kernel, no GPU)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import attention_exact_ref as R
from attention_exact_ref import BF, F16

DTYPES = [pytest.param(BF, id="bf16"), pytest.param(F16, id="f16")]
TIE_CAP = 0.01          # share of elements assert_exact may hold to 1 ulp only: a condition on the inputs, not a measurement


# ------------------------------------------------------------------------------------------------------------------ the scale
def test_ln2_scale_gives_a_unit_exp2_factor():
    assert R.ln2_scale() == math.log(2.0)
    assert R.scale_log2e_f32().dtype == np.float32
    assert R.unit_scale_error() <= 4.0
    for dtype in (BF, F16):
        assert R.q_survives_scale(dtype)


def test_scale_is_passed_as_a_c_float():
    from ltx_2_mlx_amd import _native as nv
    for name in ("ltx2_flash_attn", "ltx2_flash_attn_keymask", "ltx2_flash_attn_gated", "ltx2_flash_attn_gated_parts", "ltx2_flash_attn_rowscale"):
        res, args = nv.SIGNATURES[name]
        assert res is ctypes.c_int and args[12] is ctypes.c_float, name        # Q ldq K ldk VT Npad out ldo Nq Nkv H head_dim | scale
        assert args[:12] == [nv.vp, nv.i64, nv.vp, nv.i64, nv.vp, nv.i32, nv.vp, nv.i64, nv.i32, nv.i32, nv.i32, nv.i32], name


@pytest.mark.parametrize("dim", sorted({h * 128 for h in R.HEADS}))
def test_rowscale_partials_give_a_unit_factor(dim):
    """sum / q_norm_dim + eps is exactly 1 in the kernel's fp32 expression; a factor one ulp32 off 1 (the rsqrt) still returns every Q value."""
    t, r = R.rowscale_partials(dim)
    assert r == 1.0
    f = np.float32
    assert f(f(R.QSS_LD) * f(t)) / f(dim) < f(1.0)             # the eps matters: without it the argument is 1 - 1e-6
    for dtype in (BF, F16):
        assert R.q_survives_scale(dtype, R.scale_log2e_f32())
        assert R.q_survives_scale(dtype, np.nextafter(R.scale_log2e_f32(), f(0)))
        assert R.q_survives_scale(dtype, np.nextafter(R.scale_log2e_f32(), f(2)))


# ------------------------------------------------------------------------------------------------------------------ rounding helpers
@pytest.mark.parametrize("dtype", DTYPES)
def test_round16_ulp_and_ties_against_every_code(dtype):
    """Every finite positive 16-bit value: round16 returns it, ulp is the distance to its successor, the midpoint is a tie and rounds to even."""
    codes = torch.arange(0, 0x7C00 if dtype == F16 else 0x7F80, dtype=torch.int32).to(torch.int16)
    x = codes.view(dtype).double()
    assert torch.equal(R.round16(x, dtype).view(torch.int16), codes)
    nxt = x[1:]
    assert torch.equal(R.ulp(dtype, x[:-1]), nxt - x[:-1])
    mid = (x[:-1] + nxt) / 2
    assert R.near_tie(mid[1:], dtype).all()
    even = torch.where(codes[:-1] % 2 == 0, codes[:-1], codes[1:])
    assert torch.equal(R.round16(mid, dtype).view(torch.int16), even)
    assert torch.equal(R.round16(mid * (1 + 2.0 ** -30), dtype).view(torch.int16), codes[1:])
    assert not R.near_tie(x[1:], dtype).any()
    off = mid[1:] * (1 + 2.0 ** -18)
    assert not R.near_tie(off, dtype).any()
    assert torch.equal(R.round16(-x, dtype).double(), -x)


def test_comparators_reject_one_ulp():
    ref = torch.tensor([[1.2345, -3.25, 0.0, 100.7]], dtype=torch.float64)
    for dtype in (BF, F16):
        good = R.round16(ref, dtype)
        R.assert_exact(good, ref, dtype)
        R.assert_close(good, ref, ref.abs(), dtype)
        for e in range(ref.numel()):
            bad = good.clone()
            bad.view(torch.int16)[0, e] += 1
            with pytest.raises(AssertionError):
                R.assert_exact(bad, ref, dtype)
            worse = good.clone()
            worse.view(torch.int16)[0, e] += 3
            with pytest.raises(AssertionError):
                R.assert_close(worse, ref, ref.abs(), dtype)
        tie = torch.tensor([[1.0 + 2.0 ** -(R.MANT[dtype] + 1)]], dtype=torch.float64)          # an exact tie: either neighbour passes, the next one does not
        for code_off, ok in ((0, True), (1, True), (2, False)):
            t = torch.ones(1, 1, dtype=dtype)
            t.view(torch.int16)[0, 0] += code_off
            if ok:
                R.assert_exact(t, tie, dtype)
            else:
                with pytest.raises(AssertionError):
                    R.assert_exact(t, tie, dtype)


# ------------------------------------------------------------------------------------------------------------------ V^T layout
@pytest.mark.parametrize("nkv", [1, 65])
@pytest.mark.parametrize("hd", R.HD)
def test_vt_layout_against_brute_force(nkv, hd):
    heads = 3
    v = torch.arange(nkv * (heads * hd + 8), dtype=torch.float32).reshape(nkv, heads * hd + 8) % 251 + 1       # a strided source: 8 spare columns
    vt = R.vt_layout(v, heads, hd)
    npad = (nkv + 63) // 64 * 64
    assert vt.shape == (heads, hd, npad)
    want = torch.zeros(heads, hd, npad)
    for h in range(heads):
        for d in range(hd):
            for kv in range(nkv):
                blk, in_blk = divmod(kv, 32)
                half, in_half = divmod(in_blk, 16)
                g, r = divmod(in_half, 4)
                want[h, d, 32 * blk + 8 * g + 4 * half + r] = v[kv, h * hd + d]
    assert torch.equal(vt, want)
    assert int((vt != 0).sum()) == heads * hd * nkv            # every key once, the pad zero


# ------------------------------------------------------------------------------------------------------------------ selection inputs
@pytest.mark.parametrize("dtype", DTYPES)
def test_selection_values_are_distinct(dtype):
    v = R.v_codes(261, 8, 128, dtype).double()
    assert v.min() >= 1.0 and v.max() < 4.0
    vh = v.reshape(261, 8, 128)
    for h in range(8):
        assert all(len(set(vh[j, h].tolist())) == 128 for j in (0, 100, 260))                   # over the columns of a key
        for j0 in (0, 5):
            assert all(len(set(vh[j0:j0 + 256, h, d].tolist())) == 256 for d in (0, 63, 127))   # over any 256 consecutive keys of a column


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", R.GAPS)
def test_selection_conditions(dtype, g):
    limit = 2.0 ** -10 if dtype == BF else 2.0 ** -13
    covered = {}
    for nq, nkv, heads, hd in R.ALL_SHAPES:
        inp = R.selection_inputs(dtype, nq, nkv, heads, hd, g)
        c = inp["cond"]
        assert c["sel_score"]
        assert c["other_weight"] < limit, (nq, nkv, heads, hd, c)
        assert c["gap_max"] <= (29 if g == 24 else 2 * g)
        assert c["gap_late_min"] > (15 if g == 24 else 30)             # f16 must re-reference at 24, both builds at 40
        if nkv > 64 and nq * heads >= 64:
            assert c["gap_late_min"] < math.inf                        # and some row does select a key past the first tile
        covered.setdefault((nkv, hd), set()).update(inp["sel"].reshape(-1).tolist())
        if nq == 130 and heads == 8:
            assert c["covered"], (nq, nkv, heads, hd)                  # every key index is selected by some (i, h): 1040 queries over at most 261 keys
        ref = R.ref64(inp["q"], inp["k"], inp["v"], heads, hd)[0]
        assert torch.equal(R.round16(ref, dtype).view(torch.int16), inp["expect"].view(torch.int16))
        assert not R.near_tie(ref, dtype).any()
    assert all(s == set(range(nkv)) for (nkv, _), s in covered.items())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", R.GAPS)
def test_selection_conditions_under_the_key_mask(dtype, g):
    limit = 2.0 ** -10 if dtype == BF else 2.0 ** -13
    for nq, nkv, heads, hd in R.FORM_SHAPES:
        inp = R.selection_inputs(dtype, nq, nkv, heads, hd, g, masked=True)
        keep, c = inp["keep"], inp["cond"]
        assert keep.any() and keep[inp["sel"].reshape(-1)].all()
        assert c["covered"], (nq, nkv, heads, hd)                      # the mask removes exactly the keys no query selects (plus tile 0)
        assert nkv <= 64 or not keep[:64].any()
        assert c["sel_score"] and c["other_weight"] < limit
        ref = R.ref64(inp["q"], inp["k"], inp["v"], heads, hd, keep)[0]
        assert torch.equal(R.round16(ref, dtype).view(torch.int16), inp["expect"].view(torch.int16))
    assert any(not R.selection_inputs(dtype, *s, g, masked=True)["keep"][64:].all() for s in R.FORM_SHAPES if s[1] > 64)     # a non-trivial mask exists


# ------------------------------------------------------------------------------------------------------------------ weighted inputs
def test_weighted_reference_against_softmax():
    for dtype in (BF, F16):
        for nq, nkv, heads, hd in ((37, 197, 3, 64), (130, 261, 8, 128)):
            inp = R.weighted_inputs(dtype, nq, nkv, heads, hd)
            s = R.scores(inp["q"], inp["k"], heads, hd)
            assert s.min() >= -4 and s.max() <= 0 and torch.equal(s, s.round())
            assert len(set(s.reshape(-1).tolist())) >= 4
            assert set(inp["k"].float().unique().tolist()) == {-1.0, 0.0} and set(inp["q"].float().unique().tolist()) == {0.0, 1.0}
            assert (inp["k"].float().reshape(nkv, heads, hd) != 0).sum(dim=2).max() <= 4
            hit = (inp["k"].float().reshape(nkv, heads, hd) != 0).any(dim=0)
            assert hit.reshape(heads, hd // 8, 8).any(dim=2).all() and hit.double().mean() > 0.75      # D_j spread over the head's columns: every 8-column MFMA k-group
            ref, absref, _ = R.ref64(inp["q"], inp["k"], inp["v"], heads, hd)
            p = torch.softmax(s * math.log(2.0), dim=2)
            want = torch.einsum("hij,jhd->ihd", p, inp["v"].double().reshape(nkv, heads, hd)).reshape(nq, heads * hd)
            assert (ref - want).abs().max() < 1e-12
            assert (absref >= ref.abs() - 1e-12).all()
            keep = R.weighted_mask(nkv, "tile0")
            ref_m = R.ref64(inp["q"], inp["k"], inp["v"], heads, hd, keep)[0]
            p = torch.softmax((s * math.log(2.0))[:, :, keep], dim=2)
            want = torch.einsum("hij,jhd->ihd", p, inp["v"].double().reshape(nkv, heads, hd)[keep]).reshape(nq, heads * hd)
            assert (ref_m - want).abs().max() < 1e-12
            none = torch.zeros(nkv, dtype=torch.bool)
            ref_u = R.ref64(inp["q"], inp["k"], inp["v"], heads, hd, none)[0]
            assert (ref_u - inp["v"].double().mean(dim=0)[None, :]).abs().max() < 1e-12


@pytest.mark.parametrize("dtype", DTYPES)
def test_tie_share_of_every_exact_reference(dtype):
    """assert_exact holds at most 1 % of any shipped reference to 1 ulp only."""
    def share(q, k, v, heads, hd, keep=None):
        ref, _, exact_div = R.ref64(q, k, v, heads, hd, keep)
        return R.tie_share(ref, dtype, exact_div)

    worst = 0.0
    for nq, nkv, heads, hd in R.ALL_SHAPES:                             # weighted, plain form
        inp = R.weighted_inputs(dtype, nq, nkv, heads, hd)
        worst = max(worst, share(inp["q"], inp["k"], inp["v"], heads, hd))
    for nq, nkv, heads, hd in R.FORM_SHAPES:                            # weighted, key-mask form
        inp = R.weighted_inputs(dtype, nq, nkv, heads, hd)
        for kind in R.MASK_KINDS:
            keep = R.weighted_mask(nkv, kind)
            assert keep.any() and not keep.all()
            worst = max(worst, share(inp["q"], inp["k"], inp["v"], heads, hd, keep))
    for nq, nkv, heads, hd in R.MEAN_SHAPES:                            # Q = 0; all keys masked: the same reference
        inp = R.weighted_inputs(dtype, nq, nkv, heads, hd)
        mean = inp["v"].double().mean(dim=0)[None, :].expand(nq, -1)
        ref, _, exact_div = R.ref64(torch.zeros_like(inp["q"]), inp["k"], inp["v"], heads, hd)
        assert (ref - mean).abs().max() < 1e-12 and bool(exact_div.all()) == (nkv in (64, 128))
        assert torch.equal(ref, R.ref64(inp["q"], inp["k"], inp["v"], heads, hd, torch.zeros(nkv, dtype=torch.bool))[0])
        worst = max(worst, R.tie_share(ref, dtype, exact_div))
    assert worst <= TIE_CAP, worst


def test_exact_sums_fit_fp32():
    """Nkv <= 512, |V| <= 7, P in [2^-4, 2^4] in units of 2^-4: l < 2^17 and |O| < 2^20 units."""
    assert max(R.NKV) <= 512
    assert max(R.NKV) * 7 * 2 ** 8 < 2 ** 24
    for dtype in (BF, F16):
        v = R.weighted_inputs(dtype, 1, max(R.NKV), 3, 64)["v"].double()
        assert torch.equal(v, v.round()) and v.abs().max() == 7


# ------------------------------------------------------------------------------------------------------------------ boost, gates
@pytest.mark.parametrize("dtype", DTYPES)
def test_boost_conditions(dtype):
    for nq, nkv, heads, hd in R.BOOST_SHAPES:
        inp = R.boost_inputs(dtype, nq, nkv, heads, hd)
        c = inp["cond"]
        assert c["first_max_zero"]
        assert len(c["waves"]) == (nq + 31) // 32
        for w in c["waves"]:
            assert w == {"below": True, "inside": True, "above": True, "half_inf": True}, (nq, nkv, heads, hd, w)
        s = R.scores(inp["q"], inp["k"], heads, hd)
        assert s.max() == 16 and torch.equal(s, s.round())
        assert (s[:, 3::4].max() <= 0) and (s[:, 0::4].amax(dim=2) >= 14).all()       # rows 3 mod 4 see no boost, the others their head's


def test_gate_inputs():
    lg = R.gate_logits(130, 8)
    assert lg.dtype == torch.float32 and set(lg.unique().tolist()) == set(R.GATE_LOGITS)
    assert all(set(lg[:, h].tolist()) == set(R.GATE_LOGITS) for h in range(8))
    for dtype in (BF, F16):
        x, w, b, logits = R.gate_parts_inputs(dtype, 130, 8)
        assert x.shape == (130, R.GATE_DQ) and w.shape == (8, R.GATE_DQ) and R.GATE_DQ % 256 == 0
        parts = torch.stack([(x.double()[:, c:c + 32] @ w.double()[:, c:c + 32].t()) for c in range(0, R.GATE_DQ, 32)])     # the eight K slices
        assert torch.equal(parts, parts.round()) and parts.abs().max() <= 2
        acc = torch.zeros(130, 8, dtype=torch.float32)
        for pt in parts:
            acc = acc + pt.float()
        assert torch.equal(acc + b[None, :], logits) and torch.equal(logits.double(), parts.sum(dim=0) + b.double()[None, :])
        assert len(logits.unique()) >= 8 and logits.abs().max() <= 16.5        # 16 products of -1 / 0 / 1 and the bias
    f = R.gate_factor(torch.zeros(2, 3))
    assert torch.equal(f, torch.ones(2, 3, dtype=torch.float64))
