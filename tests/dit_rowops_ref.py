"""fp64 references, derived error bounds, fp32 emulations and the shared case lists for the DiT row kernels of csrc/rowops.hip
(norm_mod / norm_mod_shared / norm_mod_shared2, qknorm_rope, gate_logits, head_gate).  CPU only: test_dit_rowops_ref_cpu.py checks
this file against the oracle and checks that every bound is sound and not vacuous; test_dit_rowops_gpu.py holds the kernels to it.

The exact value is computed in fp64 from the inputs the kernel reads (16-bit tensors converted to fp64; fp32 tables, weights and eps at
their fp32 values).  Every bound is  ulp16(exact)/2 + E  with E = u * (counted fp32 roundings x the magnitudes they act on), u = 2^-24.
The counts follow the kernels' expressions as written; a multiply-add counts its unfused form (two roundings), which covers the fused
one; rsqrtf, exp2 and the reciprocal of the hardware count 2u each.  SECOND_ORDER (1.01) multiplies E for the products of the counted
roundings (the largest, the offset-16 LayerNorm rows' 3/8 dvar^2, is below 1e-3 of the first-order term).

norm_mod (all three kernels), per row of D elements, NV = 4 (D <= 4096) or 8 vector trips per thread:
  n = 4 NV + 9          additions in the chain of a block sum: 4 per trip in the thread, 6 shuffle steps, 3 LDS adds
  ms = s2 / D           all-positive sum: (n + 1) u relative (n additions, the rounding of each square), + u for the division
  RMS:       dvar = (n + 2) u                                  relative error of var = ms
  LayerNorm: mean = s1 / D carries (n + 1) u mean|x| absolute; var = ms - mean^2 carries
             (n + 2) u ms + 2 |mean| (n + 1) u mean|x| + u mean^2 + u var <= (2 n + 5) u (ms + mean^2)      [mean|x| <= sqrt(ms)]
             dvar = (2 n + 5) u kappa,  kappa = (ms + mean^2) / var       the amplification of the one-pass variance, explicit
  rstd = rsqrtf(var + eps):   c_r u = (dvar / 2 + 1/2 + 2) u            half the relative error of var, the addition of eps, the rsqrt
  out = (x - mean) rstd (1 + sc) + sh,  sc = tab + emb, sh = tab + emb;   T = |x - mean| rstd, S = 1 + |sc_tab| + |sc_emb|, Hm = |sh_tab| + |sh_emb|
     x - mean             u T S            (LayerNorm; exact for RMS, granted to both)
     error of mean        (n + 1) u mean|x| rstd S        (LayerNorm only)
     rstd                 c_r u T S
     (x - mean) * rstd    u T S
     sc = tab + emb, 1 + sc    2 u T S
     * (1 + sc)           u T S
     sh = tab + emb       u Hm
     + sh                 u (T S + Hm)
  E = u [ (c_r + 6) T S + (n + 1) mean|x| rstd S [LayerNorm] + 2 Hm ]

qknorm_rope, per segment row of D elements:
  n = 25                16 additions per thread (8 pairs: a a + b b, then + ss), 6 shuffle steps, 3 LDS adds
  rstd = rsqrtf(ss / D + eps):   c_r = ((n + 1) + 1) / 2 + 1/2 + 2 = 16
  a, b = x rstd w       c_r + 2
  a c - b s             one rounding per product, one for the difference
  E = (c_r + 4) u (|a c| + |b s|) = 20 u (|a c| + |b s|)                (without cos / sin: c = 1, s = 0)

gate logits (x @ Wg^T + b over Dq, MFMA accumulation, 4-wave LDS reduction), as the issue states it, for any accumulation order, rounding
or truncating:   E = 2 (Dq + 8) u sum|x w| + 2 u |b|          (fp32 output: no ulp16 term)

head gate   out = att * g,  g = 2 / (1 + __expf(-l)),  __expf(y) = exp2(y log2e):
  argument y log2e      the fp32 constant (u) and the product (u): 2 u |l| log2e absolute -> 2 |l| u relative after exp2 (ln2 log2e = 1)
  exp2                  2 u;   1 + e: u;   the division: 2 u;   every error of e reaches g scaled by e / (1 + e) <= 1
  att * g               u
  E = c(l) u |exact|,   c(l) = 2 |l| + 6
"""
import math

import numpy as np
import torch

BF, F16 = torch.bfloat16, torch.float16
U = 2.0 ** -24
SECOND_ORDER = 1.01
EPS = 1e-6


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(v):
    """The value a C `float` argument holds."""
    return float(np.float32(v))


def ulp16(x, dtype):
    """Spacing of `dtype` (bfloat16: 8 significand bits, emin -126; float16: 11, -14) at |x|, as fp64."""
    p, emin = (8, -126) if dtype == BF else (11, -14)
    x = x.double().abs()
    _, e = torch.frexp(x)                                   # |x| = m 2^e, m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return torch.ldexp(torch.ones_like(x), e - (p - 1))


def bound16(exact, E, dtype):
    return 0.5 * ulp16(exact, dtype) + E


def ratio16(got, exact, E, dtype):
    """max |got - exact| / bound; NaN / inf in `got` give inf."""
    r = (got.double() - exact).abs() / bound16(exact, E, dtype)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max())


# ================================================================================================ norm_mod
def norm_nv(D):
    return 4 if D <= 4096 else 8


def norm_chain(D):
    return 4 * norm_nv(D) + 9


def _d(t):
    return None if t is None else t.double()


def _zero_or(t, like):
    return torch.zeros_like(like) if t is None else t.double().expand_as(like)


def norm_exact(x, eps, layer_norm, sct=None, sht=None, sce=None, she=None):
    """x fp32 [rows, D]; tables [D]; embeddings [D] (row-invariant) or [rows, D] (per token); any of the four may be None.
    Returns (exact, E) in fp64."""
    xd = x.double()
    D = x.shape[1]
    n = norm_chain(D)
    e = f32(eps)
    ms = (xd * xd).mean(-1, keepdim=True)
    a1 = xd.abs().mean(-1, keepdim=True)
    if layer_norm:
        mean = xd.mean(-1, keepdim=True)
        var = ((xd - mean) ** 2).mean(-1, keepdim=True)
        kappa = torch.where(var > 0, (ms + mean * mean) / var.clamp_min(1e-300), torch.ones_like(var))
        dvar = (2 * n + 5) * kappa
    else:
        mean = torch.zeros_like(ms)
        var = ms
        dvar = torch.full_like(ms, float(n + 2))
    r = 1.0 / torch.sqrt(var + e)
    c_r = 0.5 * dvar + 2.5
    t = xd - mean
    a, b = _zero_or(sct, xd), _zero_or(sce, xd)
    c, d = _zero_or(sht, xd), _zero_or(she, xd)
    exact = t * r * (1.0 + (a + b)) + (c + d)
    T, S, Hm = t.abs() * r, 1.0 + a.abs() + b.abs(), c.abs() + d.abs()
    E = (c_r + 6) * T * S + 2 * Hm
    if layer_norm:
        E = E + (n + 1) * a1 * r * S
    return exact, SECOND_ORDER * U * E


def fma32(a, b, c):
    """fp32 fused multiply-add: the product is exact in fp64, the sum rounds once to fp64 and once more to fp32."""
    return (a.double() * b.double() + c.double()).float()


def block_sum_kernel_order(q4, fused_sq):
    """The kernels' own order over [rows, D] fp32 values whose squares (fused_sq is not None) or values are summed: thread t owns elements
    4t .. 4t+3 of every 1024-wide trip; xor-butterfly over 64 lanes; the four wave sums added left to right."""
    rows, D = q4.shape
    nv = norm_nv(D)
    p = torch.zeros(rows, nv * 1024, dtype=torch.float32)
    p[:, :D] = q4
    p = p.reshape(rows, nv, 256, 4)
    s = torch.zeros(rows, 256, dtype=torch.float32)
    for i in range(nv):
        v = p[:, i]
        if fused_sq is None:
            s = s + (((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3])
        elif fused_sq:
            s = s + fma32(v[..., 3], v[..., 3], fma32(v[..., 2], v[..., 2], fma32(v[..., 1], v[..., 1], v[..., 0] * v[..., 0])))
        else:
            s = s + (((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]) + v[..., 3] * v[..., 3])
    s = s.reshape(rows, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lane ^ o]
    w = s[:, :, 0]
    return (((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])[:, None]


def norm_emulate(x, eps, layer_norm, sct=None, sht=None, sce=None, she=None, order="kernel", fused=False, wrong=None):
    """fp32 emulation of norm_mod's arithmetic before the 16-bit rounding.  order: "kernel" (block_sum_kernel_order) or "torch" (torch's own
    vectorised / pairwise sum); fused: the multiply-adds the compiler may contract are fused.  wrong: None, "no_eps", "d_minus_4"."""
    rows, D = x.shape
    if order == "kernel":
        s1 = block_sum_kernel_order(x, None)
        s2 = block_sum_kernel_order(x, fused)
    else:
        s1 = x.sum(-1, keepdim=True)
        s2 = (x * x).sum(-1, keepdim=True)
    Df = torch.tensor(float(D - 4 if wrong == "d_minus_4" else D), dtype=torch.float32)
    mean = s1 / Df if layer_norm else torch.zeros_like(s1)
    ms = s2 / Df
    if layer_norm:
        var = fma32(-mean, mean, ms) if fused else ms - mean * mean
        var = var.clamp_min(0.0)
    else:
        var = ms
    e = torch.tensor(0.0 if wrong == "no_eps" else eps, dtype=torch.float32)
    rstd = torch.rsqrt(var + e)
    z = torch.zeros(rows, D, dtype=torch.float32)
    sc, sh = z.clone(), z.clone()
    for tt in (sct, sce):
        if tt is not None:
            sc = sc + tt
    for tt in (sht, she):
        if tt is not None:
            sh = sh + tt
    sc1 = 1.0 + sc
    t = (x - mean) * rstd
    return fma32(t, sc1, sh) if fused else t * sc1 + sh


NORM_ROW_SHAPES = [(3, 8), (5, 36), (7, 1028), (4, 4096), (3, 4100), (2, 8192)]            # per-row kernel: <4> up to 4096, <8> beyond
NORM_SHARED_SHAPES = [(1025, 36), (2049, 1028), (1027, 4100), (1024, 36)]                  # row-invariant kernel; 1024 rows stay per-row
NORM_POINTER_SETS = ["none", "tables", "embeddings", "all", "scale_only", "shift_only"]
NORM2_SHAPES = [(5, 36), (1025, 1028), (3, 4100)]
NORM_FP8_SHAPES = [(5, 36), (3, 4100), (1025, 1028)]


def norm_rows(rows, D, seed):
    """fp32 [rows, D]: randn * 3; rows 1 (mod 4) carry an offset of one standard deviation, rows 2 (mod 4) of sixteen (the variance
    cancellation, std >= |mean| / 16 up to the sample's own spread); with >= 4 rows the last is all zeros (exact output: shift) and the one
    before it is scaled by 1e-3 (var of the order of eps)."""
    g = gen(seed)
    x = torch.randn(rows, D, generator=g) * 3
    r = torch.arange(rows)
    x[r % 4 == 1] += 3.0
    x[r % 4 == 2] += 48.0
    if rows >= 4:
        x[rows - 2] = torch.randn(D, generator=g) * 1e-3
        x[rows - 1] = 0.0
    return x


def norm_tables(rows, D, seed, pointer_set, per_token):
    """dict(sct, sht, sce, she): tables [D]; embeddings [D], or, per token, [rows, D] views of one [rows, 6, D] tensor (emb_stride 6 D)."""
    g = gen(seed + 1000)
    tab = 0.3 * torch.randn(2, D, generator=g)
    emb = 0.3 * torch.randn(rows, 6, D, generator=g) if per_token else 0.3 * torch.randn(6, D, generator=g)
    sce, she = (emb[:, 4], emb[:, 1]) if per_token else (emb[4], emb[1])
    full = dict(sct=tab[1], sht=tab[0], sce=sce, she=she)
    keep = {"none": (), "tables": ("sct", "sht"), "embeddings": ("sce", "she"), "all": ("sct", "sht", "sce", "she"),
            "scale_only": ("sct",), "shift_only": ("sht",)}[pointer_set]
    return {k: (v if k in keep else None) for k, v in full.items()}, emb


def norm_cases():
    """Every (rows, D, layer_norm, pointer_set, per_token) the GPU test runs, smallest first."""
    out = []
    for rows, D in NORM_ROW_SHAPES:
        for ln in (0, 1):
            for ps in NORM_POINTER_SETS:
                out.append((rows, D, ln, ps, False))
            out.append((rows, D, ln, "embeddings", True))
            out.append((rows, D, ln, "all", True))
    for rows, D in NORM_SHARED_SHAPES:
        for ln in (0, 1):
            for ps in ("tables", "all", "scale_only", "shift_only", "embeddings"):
                out.append((rows, D, ln, ps, False))
    return out


# ================================================================================================ qknorm_rope
QK_CHAIN = 25
QK_C = 20.0
QK_CASES = ([(16, 16, 1), (16, 16, 37), (128, 64, 1)]
            + [(D, hd, 37) for D in (128, 2048, 4096) for hd in (16, 64, 128)]
            + [(128, hd, rows) for rows in (2049, 4097) for hd in (16, 64, 128)])             # (D, head_dim, rows)


def qk_layout(D):
    """(ld, q_off, k_off): two segments inside one [rows, ld] buffer."""
    return 3 * D + 72, 0, D + 64


def qk_inputs(D, hd, rows, dtype, seed):
    """buf [rows, ld] 16-bit (every column random: the columns outside the segments are the sentinels), per-channel norm weights, and
    cos / sin [rows, D/2] from oracle.dit.rope_split_tables on a 3-axis grid.  Row 0 of q is all zeros (rows > 1: row 1 of k holds a single
    non-zero element)."""
    from oracle import dit, loop
    g = gen(seed)
    ld, qo, ko = qk_layout(D)
    buf = (torch.randn(rows, ld, generator=g) * 2).to(dtype)
    buf[0, qo:qo + D] = 0
    if rows > 1:
        buf[1, ko:ko + D] = 0
        buf[1, ko + (D // 3)] = 3.0
    wq = 1 + 0.25 * torch.randn(D, generator=g)
    wk = 1 + 0.25 * torch.randn(D, generator=g)
    f = max(1, math.ceil(rows / (5 * 7)))
    pos = loop.video_positions(1, f, 5, 7, 24.0)[:, :, :rows].contiguous()
    c, s = dit.rope_split_tables(pos, D, D // hd, 10000.0, [20, 2048, 2048])              # [1, H, rows, hd/2]
    cos = c[0].permute(1, 0, 2).reshape(rows, D // 2).contiguous()
    sin = s[0].permute(1, 0, 2).reshape(rows, D // 2).contiguous()
    return buf, wq, wk, cos, sin


def _split_heads(v, hd):
    rows, D = v.shape
    v = v.reshape(rows, D // hd, 2, hd // 2)
    return v[:, :, 0], v[:, :, 1]


def _join_heads(a, b):
    rows = a.shape[0]
    return torch.stack([a, b], dim=2).reshape(rows, -1)


def qk_exact(x16, w, hd, eps, cos=None, sin=None):
    """x16 [rows, D] 16-bit segment, w fp32 [D], cos / sin fp32 [rows, D/2] or None.  Returns (exact, E) fp64 [rows, D]."""
    xd, wd = x16.double(), w.double()
    rows, D = xd.shape
    r = 1.0 / torch.sqrt((xd * xd).mean(-1, keepdim=True) + f32(eps))
    y = xd * r * wd
    a, b = _split_heads(y, hd)
    if cos is None:
        return y, SECOND_ORDER * QK_C * U * y.abs()
    c, s = cos.double().reshape(rows, D // hd, hd // 2), sin.double().reshape(rows, D // hd, hd // 2)
    exact = _join_heads(a * c - b * s, b * c + a * s)
    mag = _join_heads((a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs())
    return exact, SECOND_ORDER * QK_C * U * mag


def qk_emulate(x16, w, hd, eps, cos=None, sin=None, order="kernel", fused=False, wrong=None):
    """fp32 emulation before the 16-bit rounding.  order "kernel": thread t owns rotation pairs 8t .. 8t+7; "torch": torch's own sum."""
    x = x16.float()
    rows, D = x.shape
    a, b = _split_heads(x, hd)                                     # [rows, H, hd/2]: pair p = h * hd/2 + j
    if order == "kernel":
        pa, pb = torch.zeros(rows, 2048), torch.zeros(rows, 2048)
        pa[:, :D // 2], pb[:, :D // 2] = a.reshape(rows, -1), b.reshape(rows, -1)
        pa, pb = pa.reshape(rows, 256, 8), pb.reshape(rows, 256, 8)
        s = torch.zeros(rows, 256)
        for e in range(8):
            s = s + (fma32(pb[..., e], pb[..., e], pa[..., e] * pa[..., e]) if fused else (pa[..., e] * pa[..., e] + pb[..., e] * pb[..., e]))
        s = s.reshape(rows, 4, 64)
        lane = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, :, lane ^ o]
        wv = s[:, :, 0]
        ss = (((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3])[:, None]
    else:
        ss = (x * x).sum(-1, keepdim=True)
    Df = torch.tensor(float(D - 4 if wrong == "d_minus_4" else D))
    e = torch.tensor(0.0 if wrong == "no_eps" else eps, dtype=torch.float32)
    rstd = torch.rsqrt(ss / Df + e)
    y = x * rstd * w
    if cos is None:
        return y
    ya, yb = _split_heads(y, hd)
    c, s = cos.reshape(rows, D // hd, hd // 2), sin.reshape(rows, D // hd, hd // 2)
    if fused:
        return _join_heads(fma32(ya, c, -(yb * s)), fma32(yb, c, ya * s))
    return _join_heads(ya * c - yb * s, yb * c + ya * s)


# ================================================================================================ gate logits / head gate
def int_tensor(shape, seed, lim=8):
    """Integers in [-lim, lim] as fp32 (exact in both 16-bit types for lim <= 256)."""
    return torch.randint(-lim, lim + 1, shape, generator=gen(seed)).float()


def gate_logits_int(x, w, b):
    """int64 product of integer-valued tensors: x [M, K], w [H, K], b [H] -> [M, H]."""
    return x.long() @ w.long().t() + b.long()


def gate_logits_exact(x16, w16, b):
    """fp64 logits and the bound 2 (Dq + 8) u sum|x w| + 2 u |b|."""
    xd, wd, bd = x16.double(), w16.double(), b.double()
    Dq = xd.shape[1]
    return xd @ wd.t() + bd, 2 * (Dq + 8) * U * (xd.abs() @ wd.abs().t()) + 2 * U * bd.abs()


def head_gate_exact(att16, logits, hd):
    """att16 [rows, H*hd] 16-bit, logits fp32 [rows, H] (the values the kernel reads).  Returns (exact, E) fp64."""
    rows = att16.shape[0]
    l = logits.double()
    g = 2.0 * torch.sigmoid(l)
    exact = (att16.double().reshape(rows, -1, hd) * g[..., None]).reshape(rows, -1)
    c = (2 * l.abs() + 6)[..., None].expand(rows, l.shape[1], hd).reshape(rows, -1)
    return exact, SECOND_ORDER * c * U * exact.abs()


def head_gate_emulate(att16, logits, hd):
    rows = att16.shape[0]
    g = 2.0 / (1.0 + torch.exp(-logits.float()))
    return (att16.float().reshape(rows, -1, hd) * g[..., None]).reshape(rows, -1)


def shift_one_ulp(rounded, exact, E, dtype, index):
    """`rounded` (fp64 values of a 16-bit result) with element `index` moved one 16-bit ulp plus the slack E further from `exact`."""
    out = rounded.clone().reshape(-1)
    ex, Ef = exact.reshape(-1), E.reshape(-1)
    sgn = 1.0 if float(out[index] - ex[index]) >= 0 else -1.0
    out[index] = out[index] + sgn * (float(ulp16(ex[index:index + 1], dtype)) + float(Ef[index]))
    return out.reshape(rounded.shape)


# ================================================================================================ key-mask words
def keymask_words(mask, nwords):
    """fp32 mask [S] (non-zero = attend; -0.0 is zero) -> int64 words, bit i of word t = key 64 t + i; keys >= S are masked."""
    S = mask.numel()
    bits = np.zeros(nwords * 64, dtype=np.uint64)
    bits[:S] = (mask.numpy() != 0).astype(np.uint64)
    words = (bits.reshape(nwords, 64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return torch.from_numpy(words.view(np.int64).copy())
