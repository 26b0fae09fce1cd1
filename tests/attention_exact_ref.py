"""Exact-arithmetic inputs, float64 references and comparators for the flash-attention kernel of csrc/attention.hip (plain torch / numpy, CPU only).

Why the kernel can be driven exactly through its public entries.  The C entries form  scale_log2e = float(scale) * 1.4426950408889634f  (capi.hip); with
scale = ln 2 that product is 1 within a few ulp32 (unit_scale_error()).  The kernel multiplies Q by it in fp32 and rounds back to 16 bits, which returns
any 16-bit q unchanged (q_survives_scale()).  Small-integer Q and K then give integer scores, accumulated in fp32 by the MFMA from the integer start -M,
so the exponent's argument is an integer and P = exp2(integer) is a power of two: v_exp_f32 is specified to 1 ulp and the rounding of P to 16 bits removes
that ulp (the UNROUNDED P enters the denominator l: that ulp is part of assert_exact's margin).  Small-integer V makes every partial sum of O and l an
integer multiple of a fixed power of two below 2^24, so both are exact in fp32 whatever the order of summation.  What is left is  O * (1 / l)  and one
rounding to 16 bits; the expected value is the rational  sum 2^s v / sum 2^s,  evaluated in float64.

Three families of inputs:
  selection   a two-digit one-hot address: key j = 16 b + a has K[j, 1 + a] = K[j, 17 + b] = 1; the query of (row i, head h) holds g at the two columns
              of key sel(i, h) = (7 i + 13 h + 5) % Nkv.  Scores: 2 g (selected), g (one digit matches), 0.  With g = 24 / 40 every other key weighs
              2^-24 or less and the only correctly rounded answer is V[sel] itself -- checked with torch.equal.  V carries 256 consecutive 16-bit codes
              from 1.0 up, indexed by (31 j + 7 d + 3 h) % 256: distinct over the columns of a key and over any 256 consecutive keys of a column, so a
              wrong key, head, row or column mapping cannot cancel.
  weighted    K = -1 on at most four pseudo-random columns per key, Q pseudo-random in {0, 1}: integer scores in [-4, 0], V integer in [-7, 7].
  boost       weighted plus one reserved column through which a few keys of tiles 1 and 2 score +12 .. +16: tile sums below 2^12, inside (2^12, 2^15]
              and above 2^15, and one P of 2^16 (infinite in IEEE half) -- the f16 build's bound AT_P_BIG from both sides.  Sums are no longer exact.

Two comparators: assert_exact (bit-equal to the rounded float64 value except within 2^-19 of a rounding tie; where the denominator is a power of two
the division is exact too and equality holds on ties as well) and assert_close (1 ulp16 plus 2^-15 of the magnitude actually summed).  The parametrisations of tests/test_attention_exact_gpu.py live here, so test_attention_exact_cpu.py checks the conditions
each derivation needs for exactly the cases the GPU file runs."""
import functools
import itertools
import math

import numpy as np
import torch

BF, F16 = torch.bfloat16, torch.float16
DTYPES = (BF, F16)
MANT = {BF: 7, F16: 10}                 # explicit mantissa bits
EMIN = {BF: -126, F16: -14}             # exponent of the smallest normal number
ONE_CODE = {BF: 0x3F80, F16: 0x3C00}    # bit pattern of 1.0
KVB = 64                                # keys per tile (attention.hip)
LOG2E_F32 = np.float32(1.4426950408889634)

# ---- the cases of the GPU file -------------------------------------------------------------------------------------------------------------
NKV = (37, 64, 128, 197, 261)           # one ragged tile / one full / two full / 3 full + ragged (LDS parity 1) / 4 full + ragged (parity 0)
NQ = (1, 37, 130)                       # one row / less than a wave pair / one full workgroup plus one holding two rows
HEADS = (3, 8)                          # only a multiple of 8 takes the XCD head remap
HD = (64, 128)
GAPS = (24, 40)                         # 24: bf16 stays on the stale-maximum path, f16 re-references; 40: both re-reference
ALL_SHAPES = tuple(itertools.product(NQ, NKV, HEADS, HD))                                                          # (nq, nkv, heads, hd)
FORM_SHAPES = tuple((nq, nkv, h, hd) for nkv in (37, 197, 261) for nq, h in ((37, 3), (130, 8)) for hd in HD)     # the other kernel forms
BOOST_SHAPES = tuple((nq, nkv, h, hd) for nkv in (197, 261) for nq, h in ((37, 3), (130, 8)) for hd in HD)        # need three full tiles
MEAN_SHAPES = tuple((nq, nkv, h, hd) for nkv in NKV for nq, h in ((37, 3), (130, 8)) for hd in HD)                # uniform and all-masked
MASK_KINDS = ("sparse", "tile0", "tail")
GATE_LOGITS = (-3.0, -0.5, 0.75, 4.0)
GATE_DQ = 256                           # width of the gate projection's input in the K-slice form (the smallest: 8 slices of 32)
QSS_LD = 32                             # partial sums of squares per row in the row-scale form: two 16-byte pieces per lane
Q_EPS = 1e-6


# ---- the scale ------------------------------------------------------------------------------------------------------------------------------
def ln2_scale():
    """The `scale` argument (a Python float; ctypes passes it as a C float) for which the kernel's exp2-domain factor is 1."""
    return math.log(2.0)


def scale_log2e_f32():
    """What the C entries compute from it: float(scale) * 1.4426950408889634f, in float32 arithmetic."""
    return np.float32(np.float32(ln2_scale()) * LOG2E_F32)


def unit_scale_error():
    """|scale_log2e - 1| in units of 2^-23 (the ulp of fp32 at 1.0)."""
    return abs(float(scale_log2e_f32()) - 1.0) * 2.0 ** 23


Q_VALUES = (0.0, 1.0) + tuple(float(g) for g in GAPS)       # every value the constructions put into Q


def q_survives_scale(dtype, c=None):
    """round16(q * c) == q for every Q value, with the fp32 product the kernel forms (also for c one ulp32 to either side: the row-scale form's rsqrt)."""
    cs = [scale_log2e_f32()] if c is None else [np.float32(c)]
    cs = cs + [np.nextafter(cs[0], np.float32(0)), np.nextafter(cs[0], np.float32(2))]
    qv = torch.tensor(Q_VALUES, dtype=torch.float32)
    return all(torch.equal((qv * torch.tensor(float(x), dtype=torch.float32)).to(dtype).float(), qv) for x in cs)


def rowscale_partials(q_norm_dim, eps=Q_EPS):
    """The value t that fills q_ss [Nq, QSS_LD] so that the row-scale factor is 1: the kernel adds the QSS_LD equal partials pairwise (every sum a power
    of two times t: exact), divides by q_norm_dim and adds eps, all in fp32.  Returns (t, sum / q_norm_dim + eps as the fp32 expression gives it)."""
    f = np.float32
    t = f(f(q_norm_dim) * f(1.0 - eps) / f(QSS_LD))
    for cand in (t, np.nextafter(t, f(0)), np.nextafter(t, f(1e30))):
        r = f(f(f(QSS_LD) * cand) / f(q_norm_dim)) + f(eps)
        if r == f(1.0):
            return float(cand), float(r)
    return float(t), float(f(f(f(QSS_LD) * t) / f(q_norm_dim)) + f(eps))


# ---- 16-bit rounding in float64 ------------------------------------------------------------------------------------------------------------
def ulp(dtype, x):
    """Spacing of `dtype` at |x| (float64 tensor), subnormal range included."""
    x = x.double().abs()
    e = (torch.frexp(x)[1] - 1).double()                    # x = m 2^e, m in [1, 2)
    e = torch.where(x == 0, torch.full_like(e, EMIN[dtype]), e).clamp_min(EMIN[dtype])
    return torch.exp2(e - MANT[dtype])


def round16(x, dtype):
    """float64 -> dtype, one correct rounding to nearest even (torch's own cast goes through float32: two roundings)."""
    x = x.double()
    u = ulp(dtype, x)
    return (torch.round(x / u) * u).to(dtype)               # x / u and the product are exact: u is a power of two


def near_tie(x, dtype, rel=2.0 ** -19):
    """True where x lies within rel * |x| of the midpoint between two neighbours of `dtype`."""
    x = x.double()
    u = ulp(dtype, x)
    t = x.abs() / u
    return ((t - torch.floor(t)) - 0.5).abs() * u <= rel * x.abs()


def tie_share(ref64, dtype, exact_div=None):
    """Share of elements in assert_exact's 1-ulp class: a condition on the inputs (at most 1 %), checked on the reference alone."""
    near = near_tie(ref64, dtype)
    if exact_div is not None:
        near = near & ~exact_div
    return float(near.double().mean())


def _report(bad, out, exp, ref64, what):
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: got {float(out[idx])!r}, expected {float(exp[idx])!r} "
            f"(float64 {float(ref64[idx])!r})")


def assert_exact(out, ref64, dtype, what="attention", exact_div=None):
    """out (CPU, dtype) equals ref64 rounded to dtype wherever ref64 is further than 2^-19 (relative) from a rounding tie, and is within 1 ulp elsewhere.
    The margin: with O and l exact, the kernel's value is O * (1 / l): the reciprocal carries at most 1 ulp32, the product 0.5 ulp32; the UNROUNDED P in
    l at most 1 ulp32 (v_exp_f32's stated accuracy) and one rescale factor exp2(M - M') 1 ulp32: 3.5 ulp32 < 2^-21 relative; 2^-19 leaves two bits.
    exact_div (bool, out's shape): elements whose denominator l is a power of two.  There 1 / l and the product are exact as well, the kernel rounds the
    true value once, and equality is required ON a tie too (round to nearest even) -- small integers over 64 or 128 keys land on exact ties often.
    Equality is by value: the sign of a zero is not compared."""
    assert out.dtype == dtype and out.shape == ref64.shape, (out.dtype, out.shape, ref64.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    exp = round16(ref64, dtype)
    o, e = out.double(), exp.double()
    near = near_tie(ref64, dtype)
    if exact_div is not None:
        near = near & ~exact_div
    bad = torch.where(near, (o - e).abs() > ulp(dtype, ref64), o != e)
    assert not bad.any(), _report(bad, o, e, ref64, what)


def assert_close(out, ref64, absref, dtype, what="attention"):
    """|out - ref64| <= ulp(dtype, ref64) + 2^-15 absref, absref = sum w |v| / sum w: the second term bounds the accumulation error of at most 512 fp32
    additions of at most 2^-24 each (relative to the magnitude actually summed, which matters where V's signs cancel); it also covers the few ulp32 of
    1 / l, exp2 and the gate's __expf."""
    assert out.dtype == dtype and out.shape == ref64.shape, (out.dtype, out.shape, ref64.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    o = out.double()
    bad = (o - ref64).abs() > ulp(dtype, ref64) + 2.0 ** -15 * absref
    assert not bad.any(), _report(bad, o, ref64, ref64, what)


# ---- layouts and the float64 reference -----------------------------------------------------------------------------------------------------
def vt_layout(v, heads, hd):
    """V [Nkv, >= heads*hd] -> V^T [H][hd][Npad] as attention.h documents it: inside every 32-key block key 16 h + 4 g + r (h < 2, g < 4, r < 4) sits at
    position 8 g + 4 h + r; Npad = Nkv rounded up to 64, keys >= Nkv are zero."""
    nkv = v.shape[0]
    npad = (nkv + KVB - 1) // KVB * KVB
    kv = torch.arange(nkv)
    pos = 32 * (kv // 32) + 8 * ((kv // 4) % 4) + 4 * ((kv // 16) % 2) + kv % 4
    vt = torch.zeros(heads, hd, npad, dtype=v.dtype)
    vt[:, :, pos] = v[:, :heads * hd].reshape(nkv, heads, hd).permute(1, 2, 0)
    return vt


def scores(q, k, heads, hd):
    """Q K^T per head in float64 (exp2 units at scale = ln 2): [H, Nq, Nkv]."""
    qh = q.double().reshape(q.shape[0], heads, hd)
    kh = k.double().reshape(k.shape[0], heads, hd)
    return torch.einsum("ihd,jhd->hij", qh, kh)


def ref64(q, k, v, heads, hd, keep=None):
    """sum 2^s v / sum 2^s over the kept keys in float64 -> (ref [Nq, H*hd], absref = sum 2^s |v| / sum 2^s, exact_div = the denominator is a power of
    two [Nq, H*hd] bool).  keep: bool [Nkv] or None; no key kept = the uniform result over all Nkv keys (attention.h: a row whose keys are all masked)."""
    s = scores(q, k, heads, hd)
    if keep is not None:
        if keep.any():
            s = s.masked_fill(~keep[None, None, :], -math.inf)
        else:
            s = torch.zeros_like(s)
    w = torch.exp2(s - s.max(dim=2, keepdim=True).values)              # integer arguments: exact powers of two
    vh = v.double().reshape(v.shape[0], heads, hd)
    den = w.sum(dim=2)
    ref = torch.einsum("hij,jhd->ihd", w, vh) / den.t()[:, :, None]
    absref = torch.einsum("hij,jhd->ihd", w, vh.abs()) / den.t()[:, :, None]
    n = q.shape[0]
    pow2 = (torch.frexp(den)[0] == 0.5).t()[:, :, None].expand(n, heads, hd)
    return ref.reshape(n, heads * hd), absref.reshape(n, heads * hd), pow2.reshape(n, heads * hd)


# ---- selection inputs ----------------------------------------------------------------------------------------------------------------------
def v_codes(nkv, heads, hd, dtype):
    """V[j, h*hd + d] = the 16-bit value with bit pattern code(1.0) + (31 j + 7 d + 3 h) % 256: bf16 values in [1, 4), f16 values in [1, 1.25)."""
    j = torch.arange(nkv)[:, None, None]
    h = torch.arange(heads)[None, :, None]
    d = torch.arange(hd)[None, None, :]
    code = ONE_CODE[dtype] + (31 * j + 7 * d + 3 * h) % 256
    return code.to(torch.int16).reshape(nkv, heads * hd).view(dtype)


def sel_index(nq, heads, nkv, allowed=None):
    """sel(i, h) = (7 i + 13 h + 5) % Nkv.  With a sorted list `allowed` of n unmasked keys: allowed[(s (heads i + h) + 5) % n], s the first of 7, 11, 13, 17
    coprime to n -- the queries number at least n there (the list is a subset of what sel() selects), so every allowed key is selected."""
    i, h = torch.arange(nq)[:, None], torch.arange(heads)[None, :]
    if allowed is None:
        return (7 * i + 13 * h + 5) % nkv
    n = allowed.numel()
    s = next(c for c in (7, 11, 13, 17) if math.gcd(c, n) == 1)
    return allowed[(s * (heads * i + h) + 5) % n]


def selection_mask(nq, nkv, heads):
    """The key mask of the masked selection case: only keys that sel() selects in this case stay, minus one whole 64-key tile (tile 0, whose keys then
    leave the first tile's maximum at the masked score; only where another tile exists) -> (keep bool [Nkv], allowed sorted indices)."""
    keep = torch.zeros(nkv, dtype=torch.bool)
    keep[sel_index(nq, heads, nkv).reshape(-1)] = True
    if nkv > KVB:
        keep[:KVB] = False
    return keep, keep.nonzero().reshape(-1)


@functools.lru_cache(maxsize=None)
def selection_inputs(dtype, nq, nkv, heads, hd, g, masked=False):
    """-> dict(q, k, v, sel, expect, keep, cond).  expect = V[sel]; cond holds the conditions under which that is the only correctly rounded answer:
      selected      number of distinct keys selected in this case, `covered`: all keys (all unmasked keys) are
      other_weight  max over rows of (sum of 2^(s_j - s_sel) over the other attended keys) * max|V| / min|V|   (must be < 2^-10 bf16, 2^-13 f16: half an
                    ulp16 relative is at least 2^-9 / 2^-12)
      gap_max       max over rows of s_sel - (maximum of the row's first tile): at most 29 for g = 24 keeps every bf16 tile sum under 2^30
      gap_late_min  min of that gap over rows whose selected key lies past the first tile (g = 24: > 15, the f16 build must re-reference; g = 40: > 30,
                    both builds must)"""
    D = heads * hd
    assert nkv <= 16 * 17 and hd >= 17 + 17
    keep, allowed = selection_mask(nq, nkv, heads) if masked else (None, None)
    sel = sel_index(nq, heads, nkv, allowed)
    j = torch.arange(nkv)
    k = torch.zeros(nkv, D)
    q = torch.zeros(nq, D)
    rows = torch.arange(nq)
    for h in range(heads):
        k[j, h * hd + 1 + j % 16] = 1.0
        k[j, h * hd + 17 + j // 16] = 1.0
        q[rows, h * hd + 1 + sel[:, h] % 16] = float(g)
        q[rows, h * hd + 17 + sel[:, h] // 16] = float(g)
    v = v_codes(nkv, heads, hd, dtype)
    expect = torch.gather(v.view(torch.int16).reshape(nkv, heads, hd), 0, sel[:, :, None].expand(nq, heads, hd)).reshape(nq, D).view(dtype)
    s = scores(q, k, heads, hd)                                         # [H, Nq, Nkv]
    ssel = torch.gather(s, 2, sel.t()[:, :, None])                      # [H, Nq, 1]
    w = torch.exp2(s - ssel)
    if keep is not None:
        w = w * keep[None, None, :]
    other = w.sum(dim=2) - 1.0
    vd = v.double().abs()
    first = s[:, :, :min(KVB, nkv)].max(dim=2, keepdim=True).values
    gap = (ssel - first).reshape(heads, nq)
    late = (sel.t() >= KVB)
    want = set(range(nkv)) if allowed is None else set(allowed.tolist())
    cond = {
        "selected": len(set(sel.reshape(-1).tolist())),
        "covered": set(sel.reshape(-1).tolist()) == want,
        "sel_score": bool((ssel == 2 * g).all()),
        "other_weight": float(other.max() * vd.max() / vd.min()),
        "gap_max": float(gap.max()),
        "gap_late_min": float(gap[late].min()) if late.any() else math.inf,
    }
    return {"q": q.to(dtype), "k": k.to(dtype), "v": v, "sel": sel, "expect": expect, "keep": keep, "cond": cond}


# ---- weighted inputs -----------------------------------------------------------------------------------------------------------------------
def _mix(x):
    """A fixed 32-bit integer hash (int64 tensors; wrap-around keeps the low 32 bits).  The offset is the first of 0, 7919, 2 * 7919, ... for which
    every weighted reference of the cases above keeps its share of near-ties under assert_exact's 1 % (float16's natural rate at 2^-19 is ~0.6 %)."""
    x = ((x + 79190) * 2654435761) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 2246822519) & 0xFFFFFFFF
    return x ^ (x >> 13)


@functools.lru_cache(maxsize=None)
def weighted_inputs(dtype, nq, nkv, heads, hd):
    """K[j, d] = -1 on D_j (four draws from the head's hd columns: at most four distinct), Q in {0, 1}: scores are integers in [-4, 0];
    V[j, h*hd + d] = (5 j + 3 d + h) % 15 - 7.  Every partial sum of l and O stays an integer multiple of one power of two below 2^24 for Nkv <= 512:
    P spans [2^-4, 2^4] around the first tile's maximum (9 bits), |V| <= 7 (3 bits), 512 keys (9 bits)."""
    assert nkv <= 512
    D = heads * hd
    j = torch.arange(nkv)[:, None, None]
    i = torch.arange(nq)[:, None, None]
    h = torch.arange(heads)[None, :, None]
    d = torch.arange(hd)[None, None, :]
    m = torch.arange(4)[None, None, :]
    col = _mix(j * 131 + h * 17 + m * 7 + 1) % hd                       # [Nkv, H, 4]
    k = torch.zeros(nkv, heads, hd)
    k.scatter_(2, col, -1.0)
    q = ((_mix(i * 257 + h * 19 + d * 3 + 2) >> 4) & 1).float()         # [Nq, H, hd]
    v = (((5 * j + 3 * d + h) % 15) - 7).float().reshape(nkv, D).to(dtype)
    return {"q": q.reshape(nq, D).to(dtype), "k": k.reshape(nkv, D).to(dtype), "v": v}


def weighted_mask(nkv, kind):
    """Key masks of the weighted tests (True = attend).  sparse: every fourth key off; tile0: also the whole first tile (its maximum is the masked score,
    the next tile rescales by exp2(-1e30 - m) = 0); tail: also the whole last tile (ragged where Nkv is).  The two tile kinds need a second tile."""
    j = torch.arange(nkv)
    keep = (3 * j + 1) % 4 != 0
    if kind == "tile0" and nkv > KVB:
        keep &= j >= KVB
    if kind == "tail" and nkv > KVB:
        keep &= j < (nkv - 1) // KVB * KVB
    return keep


# ---- the boost variant ---------------------------------------------------------------------------------------------------------------------
BOOST_KEYS = {0: ((KVB + 5, 12), (KVB + 22, 13), (KVB + 43, 14)),       # head % 3 == 0: tile 1 sums inside (2^12, 2^15]: the f16 build stays on the fast path
              1: ((KVB + 9, 15), (2 * KVB + 30, 16)),                   # == 1: tile 1 above 2^15 (re-reference); tile 2 is then 2^1 above the new reference
              2: ((2 * KVB + 50, 16),)}                                 # == 2: tile 1 plain; tile 2 holds the row's only heavy key, P = 2^16 = inf in half


@functools.lru_cache(maxsize=None)
def boost_inputs(dtype, nq, nkv, heads, hd):
    """Weighted inputs with column 0 of every head reserved: K[:, 0] = 0 except the keys of BOOST_KEYS (whose other columns are 0, so they score exactly
    their boost), Q[i, 0] = 1 except rows i % 4 == 3 (which ride through the re-referenced tiles without a large score of their own).  Key 0 is all zero,
    so every row's first-tile maximum, the stale reference, is 0.  cond: per wave of 32 rows, over the heads, the classes of (tile >= 1, lane) sums of
    2^score over the lane's 16 keys {16 kb + 4 g + r} -- `below` (a whole wave-tile under 2^12), `inside` (a wave-tile whose largest lane sum is in
    (2^12, 2^15]), `above` (a lane sum past 2^15), `half_inf` (a single P >= 2^16 > 65504)."""
    assert nkv >= 3 * KVB
    base = weighted_inputs(dtype, nq, nkv, heads, hd)
    q = base["q"].float().reshape(nq, heads, hd).clone()
    k = base["k"].float().reshape(nkv, heads, hd).clone()
    k[:, :, 0] = 0.0
    k[0] = 0.0
    q[:, :, 0] = 1.0
    q[3::4, :, 0] = 0.0
    for h in range(heads):
        for key, boost in BOOST_KEYS[h % 3]:
            k[key, h] = 0.0
            k[key, h, 0] = float(boost)
    D = heads * hd
    q, k = q.reshape(nq, D).to(dtype), k.reshape(nkv, D).to(dtype)
    s = scores(q, k, heads, hd)
    first_max = s[:, :, :KVB].max(dim=2).values
    nfull = nkv // KVB
    p = torch.exp2(s[:, :, KVB:nfull * KVB]).reshape(heads, nq, nfull - 1, 4, 4, 4)      # [h, i, tile, kb, g, r]
    lane = p.sum(dim=(3, 5))                                                             # [h, i, tile, g]
    waves = []
    for w0 in range(0, nq, 32):
        big = lane[:, w0:w0 + 32].amax(dim=(1, 3))                                       # [h, tile]: what the wave's __any sees
        waves.append({"below": bool((big < 2.0 ** 12).any()), "inside": bool(((big > 2.0 ** 12) & (big <= 2.0 ** 15)).any()),
                      "above": bool((big > 2.0 ** 15).any()), "half_inf": bool((p[:, w0:w0 + 32] >= 2.0 ** 16).any())})
    cond = {"first_max_zero": bool((first_max == 0).all()), "waves": waves}
    return {"q": q, "k": k, "v": base["v"], "cond": cond}


# ---- gates ---------------------------------------------------------------------------------------------------------------------------------
def gate_logits(nq, heads):
    """logits[i, h] = GATE_LOGITS[(i + h) % 4] (fp32)."""
    idx = (torch.arange(nq)[:, None] + torch.arange(heads)[None, :]) % 4
    return torch.tensor(GATE_LOGITS, dtype=torch.float32)[idx]


def gate_parts_inputs(dtype, nq, heads, dq=GATE_DQ):
    """x [Nq, dq], gate_w [H, dq] with entries in {-1, 0, 1} on every 16th column and gate_b [H] in quarters: every K-slice partial sum is a small integer
    (exact in fp32 in any order), their sum and the bias add exactly -> (x, gate_w, gate_b, logits fp32 [Nq, H])."""
    c = torch.arange(dq)[None, :]
    on = (c % 16 == 0)
    x = torch.where(on, (_mix(torch.arange(nq)[:, None] * 97 + c) % 3) - 1, torch.zeros(1, dtype=torch.int64))
    w = torch.where(on, (_mix(torch.arange(heads)[:, None] * 53 + c * 5 + 7) % 3) - 1, torch.zeros(1, dtype=torch.int64))
    b = (torch.arange(heads) % 4).float() * 0.25 - 0.5
    logits = (x @ w.t()).float() + b[None, :]
    return x.to(dtype), w.to(dtype), b, logits


def gate_factor(logits):
    """2 sigmoid(logit) in float64, [Nq, H]."""
    return 2.0 / (1.0 + torch.exp(-logits.double()))


def apply_gate(t, factor, heads, hd):
    n = t.shape[0]
    return (t.reshape(n, heads, hd) * factor[:, :, None]).reshape(n, heads * hd)
