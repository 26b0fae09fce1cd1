"""Element-wise tests of the DiT row kernels of csrc/rowops.hip through their C entries: AdaLN RMS / LayerNorm (norm_mod, the row-invariant
norm_mod_shared, the two-output norm_mod_shared2, the fused fp8 quantiser), the fp8 row quantiser, QK-norm + split RoPE, the gate-logit
product (one launch and K-slice parts), the head gate and the key-mask words.

The exact value is computed in fp64 from the inputs the kernel reads; every 16-bit output is held to  ulp16(exact)/2 + E  with E counted
from the kernel's fp32 expression (u = 2^-24; tests/dit_rowops_ref.py derives each count, test_dit_rowops_ref_cpu.py checks the bounds
against fp32 emulations before any GPU run):

  norm_mod     E = u [ (c_r + 6) T S + (n + 1) mean|x| rstd S [LayerNorm] + 2 Hm ],   T = |x - mean| rstd, S = 1 + |sc_tab| + |sc_emb|,
               Hm = |sh_tab| + |sh_emb|, n = 4 NV + 9 (NV = 4 up to D = 4096, else 8), c_r = dvar / 2 + 2.5 with dvar = n + 2 (RMS: the
               all-positive sum of squares) or (2 n + 5) (ms + mean^2) / var (LayerNorm: the one-pass variance's amplification, explicit)
  qknorm_rope  E = 20 u (|a c| + |b s|),  a, b = x rstd w        (n = 25, c_r = 16, two products, one product each by c / s, the difference)
  gate logits  integer inputs: equal to the int64 product; random inputs: |got - exact| <= 2 (Dq + 8) u sum|x w| + 2 u |b|
  head gate    E = (2 |l| + 6) u |exact|                          (the exponent's argument rounding grows with |l|)
  quantisers, parts, key-mask words: bit for bit (quant_rows_emulated; int64 products per K slice; CPU bit packing)

Each E carries the factor 1.01 for second-order terms.  Every ratio |got - exact| / bound is recorded with conftest.measure() and must
be <= 1.  Strides other than the row width go through the C entries directly (the wrappers of kernels.py always pass the width); every
padding column and guard region is pre-filled and must come back bit-identical.  The shapes are the smallest that reach each path: both
template widths and both sides of every switch (D 4096 / 4100, rows 1024 / 1025, K 4096 / 4104 / 16384 / 16392), a last vector trip with
one active thread (D = 1028, 4100), two and three rows per block with a ragged last block, H in 17..31 (the second weight fragment's
clamp), no / one / one-plus-tail / two deep trips per wave in the logit product, the second outer trip of the parts kernel (Dq = 4352),
the head gate past its 4096-block cap, key counts that are no multiple of 64."""
import pytest
import torch

import dit_rowops_ref as R
from conftest import measure, rel_l2
from dit_rowops_ref import BF, F16, U

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(BF, id="bf16"), pytest.param(F16, id="f16")]
ulp16 = R.ulp16
EPS = R.EPS
SENT = 77.0                     # exact in both 16-bit types; no output of these tests lands on it by design of the inputs


@pytest.fixture(scope="module")
def K(dev):
    import ltx_2_mlx_amd.kernels as k
    return k


@pytest.fixture(scope="module")
def nv(dev):
    from ltx_2_mlx_amd import _native
    return _native


def bits16(t):
    return t.contiguous().view(torch.int16)


def padded(t, ld, fill):
    """[rows, W] -> [rows, ld] with the columns from W on set to `fill`."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def assert_padding(buf, width, ref):
    """Columns >= width of the [rows, ld] device buffer are bit-identical to those of `ref` (CPU)."""
    got = buf.cpu()
    view = {2: torch.int16, 1: torch.uint8, 4: torch.int32}[got.element_size()]
    assert torch.equal(got[:, width:].contiguous().view(view), ref[:, width:].contiguous().view(view))


# ------------------------------------------------------------------------------------------ 1. norm_mod (ltx2_adaln_rmsnorm)
def run_norm(nv, dev, dtype, x, ln, tabs, emb, emb_mode, ldx, ldo):
    """One ltx2_adaln_rmsnorm call; returns the [rows, D] result (CPU).  emb_mode: 0 (row-invariant [D] vectors), "D" (per token,
    contiguous [rows, D]) or "6D" (per token, rows of the [rows, 6, D] tensor `emb`)."""
    rows, D = x.shape
    xb = padded(x, ldx, SENT).to(dev)
    out0 = torch.full((rows, ldo), SENT, dtype=dtype)
    out = out0.to(dev)
    dv = {k: (None if v is None else v.contiguous().to(dev)) for k, v in tabs.items()}
    stride = 0
    emb_d = None
    if emb_mode == "D":
        stride = D
    elif emb_mode == "6D":
        emb_d = emb.to(dev)                                     # [rows, 6, D]: rows 4 (scale) and 1 (shift) of every token
        stride = 6 * D
        dv["sce"] = None if tabs["sce"] is None else emb_d[:, 4]
        dv["she"] = None if tabs["she"] is None else emb_d[:, 1]
    nv.check(nv.lib(dtype).ltx2_adaln_rmsnorm(nv.ptr(xb), ldx, nv.ptr(out), ldo, rows, D, EPS, ln, nv.ptr(dv["sct"]), nv.ptr(dv["sht"]),
                                              nv.ptr(dv["sce"]), nv.ptr(dv["she"]), stride, nv.stream()))
    assert_padding(out, D, out0)
    return out.cpu()[:, :D]


def check_norm(nv, dev, dtype, rows, D, ln, ps, per_token):
    x = R.norm_rows(rows, D, 7 * rows + D + ln)
    tabs, emb = R.norm_tables(rows, D, rows + D, ps, per_token)
    exact, E = R.norm_exact(x, EPS, ln, **tabs)
    modes = ("D", "6D") if per_token else (0,)
    worst = 0.0
    for mode in modes:
        for ldx, ldo in ((D + 4, D + 8),) + (((D, D),) if ps == "all" else ()):
            got = run_norm(nv, dev, dtype, x, ln, tabs, emb, mode, ldx, ldo)
            worst = max(worst, R.ratio16(got, exact, E, dtype))
    kind = "layernorm" if ln else "rmsnorm"
    measure(f"norm_mod {kind} err/bound", worst)
    assert worst <= 1.0, (rows, D, ln, ps, per_token, worst)
    if rows >= 4:                                              # the all-zero row: the exact output is the shift, and E its two roundings
        Hm = sum(v.double().abs().expand_as(exact)[rows - 1] for v in (tabs["sht"], tabs["she"]) if v is not None) + torch.zeros(D, dtype=torch.float64)
        assert torch.equal(E[rows - 1], R.SECOND_ORDER * U * 2 * Hm)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,D", R.NORM_ROW_SHAPES)
def test_norm_mod_per_row(dev, nv, dtype, rows, D):
    """norm_mod_kernel<4> / <8>: every pointer set, per-token embeddings at emb_stride D and 6 D, ldx = D + 4 and ldo = D + 8."""
    for case in R.norm_cases():
        if case[:2] == (rows, D):
            check_norm(nv, dev, dtype, *case)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,D", R.NORM_SHARED_SHAPES)
def test_norm_mod_row_invariant(dev, nv, dtype, rows, D):
    """norm_mod_shared_kernel (emb_stride 0, a table set, rows > 1024): a last block of one row, three rows per block, the <8> width; and
    1024 rows with the same tables, which stay on the per-row kernel."""
    for case in R.norm_cases():
        if case[:2] == (rows, D):
            check_norm(nv, dev, dtype, *case)


# ------------------------------------------------------------------------------------------ 2. norm_mod2 (ltx2_adaln_rmsnorm2)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,D", R.NORM2_SHAPES)
def test_norm_mod2(dev, nv, dtype, rows, D):
    x = R.norm_rows(rows, D, 3 * rows + D)
    g = R.gen(rows + D + 5)
    t = [0.3 * torch.randn(D, generator=g) for _ in range(4)]              # scale0, shift0, scale1, shift1
    ldx, ldo = D + 4, D + 8
    xb = padded(x, ldx, SENT).to(dev)
    td = [v.to(dev) for v in t]
    for null in (None, 0, 1, 2, 3):
        use = [None if i == null else td[i] for i in range(4)]
        cpu = [None if i == null else t[i] for i in range(4)]
        o0_0 = torch.full((rows, ldo), SENT, dtype=dtype)
        o0, o1 = o0_0.to(dev), o0_0.to(dev)
        nv.check(nv.lib(dtype).ltx2_adaln_rmsnorm2(nv.ptr(xb), ldx, nv.ptr(o0), nv.ptr(o1), ldo, rows, D, EPS, nv.ptr(use[0]), nv.ptr(use[1]),
                                                   nv.ptr(use[2]), nv.ptr(use[3]), nv.stream()))
        for out, (sc, sh) in ((o0, cpu[0:2]), (o1, cpu[2:4])):
            assert_padding(out, D, o0_0)
            exact, E = R.norm_exact(x, EPS, 0, sct=sc, sht=sh)
            r = measure("norm_mod2 err/bound", R.ratio16(out.cpu()[:, :D], exact, E, dtype))
            assert r <= 1.0, (null, r)


# ------------------------------------------------------------------------------------------ 3. norm -> fp8 (ltx2_adaln_rmsnorm_fp8)
def quantise_rows(nv, dev, x16, ld_in=None, ld_out=None):
    """ltx2_quantize_rows_fp8 on a CPU [rows, K] 16-bit tensor with row strides ld_in / ld_out (padding pre-filled and checked)."""
    rows, K = x16.shape
    ld_in, ld_out = ld_in or K, ld_out or K
    xb = padded(x16, ld_in, 30000.0).to(dev)                  # a padding column read by mistake would win the row maximum
    c0 = torch.full((rows, ld_out), 0xAB, dtype=torch.uint8)
    codes, scale = c0.to(dev), torch.full((rows,), -1.0, device=dev)
    nv.check(nv.lib(x16.dtype).ltx2_quantize_rows_fp8(nv.ptr(xb), ld_in, rows, K, nv.ptr(codes), ld_out, nv.ptr(scale), nv.stream()))
    assert_padding(codes, K, c0)
    return codes.cpu()[:, :K], scale.cpu()


@pytest.mark.parametrize("rows,D", R.NORM_FP8_SHAPES)
def test_norm_fp8_equals_norm_then_quantise(dev, nv, rows, D):
    """Codes and scales of the fused call == ltx2_quantize_rows_fp8 of the unfused call's bf16 output, bit for bit.  The quantiser takes
    K % 8 == 0 and these D are 4 mod 8, so the bf16 rows are extended by four zeros, which change neither the row maximum nor a code."""
    x = R.norm_rows(rows, D, 11 * rows + D)
    ldq = D + 4
    for ln in (0, 1):
        for ps in ("all", "none") if rows <= 1024 else ("all", "tables"):
            tabs, emb = R.norm_tables(rows, D, rows + D, ps, False)
            ref16 = run_norm(nv, dev, BF, x, ln, tabs, emb, 0, D, D)
            rc, rs = quantise_rows(nv, dev, padded(ref16, (D + 7) // 8 * 8, 0.0))
            xd = x.to(dev)
            dv = {k: (None if v is None else v.contiguous().to(dev)) for k, v in tabs.items()}
            for want16 in (True, False):
                c0 = torch.full((rows, ldq), 0xAB, dtype=torch.uint8)
                codes, scale = c0.to(dev), torch.full((rows,), -1.0, device=dev)
                out = torch.full((rows, D), SENT, dtype=BF, device=dev) if want16 else None
                nv.check(nv.lib(BF).ltx2_adaln_rmsnorm_fp8(nv.ptr(xd), D, nv.ptr(out), D, nv.ptr(codes), ldq, nv.ptr(scale), rows, D, EPS, ln,
                                                           nv.ptr(dv["sct"]), nv.ptr(dv["sht"]), nv.ptr(dv["sce"]), nv.ptr(dv["she"]), 0, nv.stream()))
                assert_padding(codes, D, c0)
                assert torch.equal(codes.cpu()[:, :D], rc[:, :D]) and torch.equal(scale.cpu(), rs), (ln, ps, want16)
                if want16:
                    assert torch.equal(bits16(out.cpu()), bits16(ref16))


# ------------------------------------------------------------------------------------------ 4. quantize_rows_fp8
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Kdim", [8, 4096, 4104, 16384, 16392, 32768])
def test_quantize_rows_fp8_exact(dev, nv, dtype, Kdim):
    """quant_rows_fp8_kernel<2> / <8> / <16> on both sides of each switch, ldx = ldo = K + 8: a random, an all-zero, an outlier, a tiny and a
    large row against the existing fp32 / float8_e4m3fn emulation, bit for bit."""
    from test_kernels_gpu import quant_rows_emulated
    x = torch.randn(5, Kdim, generator=R.gen(Kdim))
    x[1] = 0.0
    x[2, Kdim - 1] = 300.0
    x[3] *= 1e-3
    x[4] *= 1e3
    x = x.to(dtype)
    codes, scale = quantise_rows(nv, dev, x, Kdim + 8, Kdim + 8)
    rc, rs = quant_rows_emulated(x)
    assert torch.equal(scale, rs)
    assert torch.equal(codes, rc), int((codes != rc).sum())
    assert float(scale[1]) == 1.0 and int(codes[1].max()) == 0


# ------------------------------------------------------------------------------------------ 5. qknorm_rope
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,hd,rows", R.QK_CASES)
def test_qknorm_rope(dev, nv, dtype, D, hd, rows):
    """Two segments (q at 0, k at D + 64) of one [rows, 3 D + 72] buffer with cos / sin, the one-segment form, and two segments without
    cos / sin.  Per-channel norm weights, a (row, slot)-dependent table, a zero row and a row with one non-zero element."""
    buf, wq, wk, cos, sin = R.qk_inputs(D, hd, rows, dtype, D + hd + rows)
    ld, qo, ko = R.qk_layout(D)
    wqd, wkd, cd, sd = wq.to(dev), wk.to(dev), cos.to(dev), sin.to(dev)
    f = nv.lib(dtype).ltx2_qknorm_rope
    for two, rope in ((True, True), (False, True), (True, False)):
        b = buf.to(dev)
        nv.check(f(nv.ptr(b), ld, rows, D, hd, qo, nv.ptr(wqd), ko, nv.ptr(wkd) if two else None, EPS, nv.ptr(cd) if rope else None,
                   nv.ptr(sd) if rope else None, nv.stream()))
        got = b.cpu()
        touched = torch.zeros(ld, dtype=torch.bool)
        for off, w in ((qo, wq), (ko, wk))[:2 if two else 1]:
            touched[off:off + D] = True
            exact, E = R.qk_exact(buf[:, off:off + D], w, hd, EPS, cos if rope else None, sin if rope else None)
            r = measure(f"qknorm_rope rope={int(rope)} err/bound", R.ratio16(got[:, off:off + D], exact, E, dtype))
            assert r <= 1.0, (two, rope, off, r)
        assert torch.equal(bits16(got[:, ~touched]), bits16(buf[:, ~touched]))
        assert not bool(got[0, qo:qo + D].any())                # the all-zero row stays zero


# ------------------------------------------------------------------------------------------ 6. gate logits (ltx2_attn_head_gate)
def run_head_gate(nv, dev, dtype, att, ld, x, w, b, hd):
    """att [rows, H*hd] (CPU, 16-bit) gated in a [rows, ld] buffer; x [rows, Dq] passed as a column view of a wider buffer.  Returns
    (gated att, logits) on the CPU; the padding of att and a guard region behind the logits must be untouched."""
    rows, Dq = x.shape
    H = w.shape[0]
    ldx = Dq + 64
    xb = torch.full((rows, ldx), 3.0, dtype=dtype)
    xb[:, 32:32 + Dq] = x
    xb = xb.to(dev)
    a0 = padded(att, ld, SENT)
    ab, wd, bd = a0.to(dev), w.contiguous().to(dev), b.float().to(dev)
    lg = torch.full((rows * H + 64,), -12345.0, device=dev)
    nv.check(nv.lib(dtype).ltx2_attn_head_gate(nv.ptr(ab), ld, nv.ptr(xb[:, 32:]), ldx, nv.ptr(wd), nv.ptr(bd), nv.ptr(lg), rows, Dq, H, hd, nv.stream()))
    assert_padding(ab, H * hd, a0)
    lg = lg.cpu()
    assert bool((lg[rows * H:] == -12345.0).all())
    return ab.cpu()[:, :H * hd], lg[:rows * H].reshape(rows, H)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Dq", [128, 2048, 2176, 4096])
def test_gate_logits_integer_exact(dev, nv, dtype, Dq):
    """Integers |v| <= 8: every partial sum is an integer below 2^24, so the logits equal the int64 product whatever the order.  Per wave
    Dq / 4 columns: no deep trip (128), exactly one (2048), one and one tail step (2176), two (4096)."""
    for rows in (1, 16, 17, 37):
        for H in (1, 16, 17, 31, 32):
            seed = Dq + 100 * rows + H
            x, w, b = R.int_tensor((rows, Dq), seed), R.int_tensor((H, Dq), seed + 1), R.int_tensor((H,), seed + 2)
            att = torch.ones(rows, H * 8, dtype=dtype)
            _, lg = run_head_gate(nv, dev, dtype, att, H * 8, x.to(dtype), w.to(dtype), b, 8)
            ref = R.gate_logits_int(x, w, b)
            assert torch.equal(lg.long(), ref) and torch.equal(lg, ref.float()), (rows, H, int((lg.long() != ref).sum()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Dq", [128, 2048, 2176, 4096])
def test_gate_logits_random_bound(dev, nv, dtype, Dq):
    for rows, H in ((37, 31), (17, 5)):
        g = R.gen(Dq + rows)
        x = torch.randn(rows, Dq, generator=g).to(dtype)
        w = (torch.randn(H, Dq, generator=g) / Dq ** 0.5).to(dtype)
        b = 0.5 * torch.randn(H, generator=g)
        _, lg = run_head_gate(nv, dev, dtype, torch.ones(rows, H * 8, dtype=dtype), H * 8, x, w, b, 8)
        exact, E = R.gate_logits_exact(x, w, b)
        r = measure("gate_logits err/bound", ((lg.double() - exact).abs() / E).max())
        assert r <= 1.0


# ------------------------------------------------------------------------------------------ 7. head gate
def gate_through_identity(nv, dev, dtype, att, ld, logits16, bias, hd):
    """Logits of any value per (row, head): x[row, h] = logits16[row, h], Wg = the first H rows of the identity, so the product is
    logits16 exactly and the kernel's logits are fp32(logits16 + bias)."""
    rows, H = logits16.shape
    x = torch.zeros(rows, 128, dtype=dtype)
    x[:, :H] = logits16
    w = torch.eye(H, 128).to(dtype)
    got, lg = run_head_gate(nv, dev, dtype, att, ld, x, w, bias, hd)
    assert torch.equal(lg, logits16.float() + bias.float())
    return got, lg


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [8, 64, 128])
def test_head_gate(dev, nv, dtype, hd):
    g = R.gen(hd)
    rows, H = 37, 5
    att = torch.randn(rows, H * hd, generator=g).to(dtype)
    ints = torch.randint(-30, 31, (rows, H), generator=g).float()
    ints[0] = torch.tensor([-30.0, 30.0, 0.0, -1.0, 1.0])
    for tag, l16, bias in (("int", ints.to(dtype), torch.zeros(H)), ("randn", (2 * torch.randn(rows, H, generator=g)).to(dtype), torch.randn(H, generator=g))):
        got, lg = gate_through_identity(nv, dev, dtype, att, H * hd + 8, l16, bias, hd)
        exact, E = R.head_gate_exact(att, lg, hd)
        r = measure(f"head_gate {tag} err/bound", R.ratio16(got, exact, E, dtype))
        assert r <= 1.0, (tag, r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_head_gate_grid_stride(dev, nv, dtype):
    """2049 x 32 x 128: 1 049 088 eight-element groups, past the 4096 blocks x 256 threads one launch covers."""
    rows, H, hd = 2049, 32, 128
    assert rows * H * hd // 8 > 4096 * 256
    g = R.gen(99)
    att = torch.randn(rows, H * hd, generator=g).to(dtype)
    l16 = (2 * torch.randn(rows, H, generator=g)).to(dtype)
    got, lg = gate_through_identity(nv, dev, dtype, att, H * hd + 8, l16, torch.randn(H, generator=g), hd)
    exact, E = R.head_gate_exact(att, lg, hd)
    r = measure("head_gate grid-stride err/bound", R.ratio16(got, exact, E, dtype))
    assert r <= 1.0


# ------------------------------------------------------------------------------------------ 8. gate-logit parts (ltx2_flash_attn_gated_parts)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Dq", [256, 4096, 4352])
def test_gate_logit_parts_integer_exact(K, dev, nv, dtype, Dq):
    """parts[ks] == the int64 product over K slice ks for all 8 slices (Dq = 4352: Kc = 544, the second outer trip); the guard region
    behind [8][Nq][H] is untouched; the attention output equals flash_attn_gated fed the summed logits."""
    hd, Nkv, KS = 64, 70, 8
    Kc = Dq // KS
    for Nq in (1, 63, 65, 130):
        for H in (1, 17, 32):
            seed = Dq + 100 * Nq + H
            g = R.gen(seed)
            x, w, b = R.int_tensor((Nq, Dq), seed), R.int_tensor((H, Dq), seed + 1), R.int_tensor((H,), seed + 2)
            q, k, v = (torch.randn(n, H * hd, generator=g).to(dtype).to(dev) for n in (Nq, Nkv, Nkv))
            vt = K.vt_transpose(v, H, head_dim=hd)
            ldx = Dq + 64
            xb = torch.full((Nq, ldx), 3.0, dtype=dtype)
            xb[:, 32:32 + Dq] = x.to(dtype)
            xb, wd, bd = xb.to(dev), w.to(dtype).to(dev), b.to(dev)
            n = KS * Nq * H
            parts = torch.full((n + 256,), -12345.0, device=dev)
            out = torch.empty(Nq, H * hd, device=dev, dtype=dtype)
            nv.check(nv.lib(dtype).ltx2_flash_attn_gated_parts(nv.ptr(q), H * hd, nv.ptr(k), H * hd, nv.ptr(vt), vt.shape[2], nv.ptr(out), H * hd, Nq, Nkv,
                                                               H, hd, hd ** -0.5, nv.ptr(xb[:, 32:]), ldx, nv.ptr(wd), nv.ptr(bd), Dq, nv.ptr(parts),
                                                               nv.stream()))
            p = parts.cpu()
            assert bool((p[n:] == -12345.0).all()), (Nq, H)
            ref = torch.stack([x[:, s * Kc:(s + 1) * Kc].long() @ w[:, s * Kc:(s + 1) * Kc].long().t() for s in range(KS)])
            got = p[:n].reshape(KS, Nq, H)
            assert torch.equal(got.long(), ref) and torch.equal(got, ref.float()), (Nq, H, int((got.long() != ref).sum()))
            logits = (got.sum(0) + b).to(dev)                   # integers: exact in any order
            assert torch.equal(logits.cpu().long(), R.gate_logits_int(x, w, b))
            gated = K.flash_attn_gated(q, k, vt, H, Nkv, logits)
            assert rel_l2(out.float().cpu(), gated.float().cpu()) < 7e-5, (Nq, H)


# ------------------------------------------------------------------------------------------ 9. key-mask words (ltx2_flash_attn_keymask)
@pytest.mark.parametrize("S", [1, 63, 64, 65, 200])
def test_keymask_words_exact(K, dev, nv, S):
    H, hd, Nq = 2, 64, 5
    g = R.gen(S)
    q, k, v = (torch.randn(n, H * hd, generator=g).to(BF).to(dev) for n in (Nq, S, S))
    vt = K.vt_transpose(v, H, head_dim=hd)
    nwords = vt.shape[2] // 64
    rnd = (torch.rand(S, generator=g) > 0.5).float()
    rnd[S // 2] = 1.0
    last = torch.zeros(S)
    last[S - 1] = 1.0
    negz = torch.where(rnd != 0, rnd, torch.full((S,), -0.0))
    assert S == 1 or bool(torch.signbit(negz).any())
    for mask in (rnd, last, negz):
        assert float(mask.abs().sum()) >= 1
        md = torch.cat([mask, torch.ones(8)]).to(dev)          # what lies behind key S - 1 reads as "attend": it must not reach a word
        words = torch.full((nwords + 4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
        out = torch.empty(Nq, H * hd, device=dev, dtype=BF)
        nv.check(nv.lib(BF).ltx2_flash_attn_keymask(nv.ptr(q), H * hd, nv.ptr(k), H * hd, nv.ptr(vt), vt.shape[2], nv.ptr(out), H * hd, Nq, S, H, hd,
                                                    hd ** -0.5, nv.ptr(md), nv.ptr(words), nv.stream()))
        wc = words.cpu()
        assert bool((wc[nwords:] == 0x5A5A5A5A5A5A5A5A).all())
        assert torch.equal(wc[:nwords], R.keymask_words(mask, nwords))
        assert bool(torch.isfinite(out.float()).all())
