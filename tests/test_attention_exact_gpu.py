"""Element-wise tests of csrc/attention.hip (attn_fwd_kernel in every shipped form, vt_transpose_kernel) on exact-arithmetic inputs, both library builds.

tests/attention_exact_ref.py builds the inputs, the float64 references and the two comparators and says why the kernel's arithmetic is exact on them;
tests/test_attention_exact_cpu.py checks every condition that argument needs for the cases below.  Here the kernel is called through the C ABI exactly
as kernels.py does, but with operands the wrappers cannot express: Q and K are column slices of one fused buffer (row stride 2 D + 8), V^T is the
documented layout built on the CPU (so attention is checked against the contract, vt_transpose against the same contract in a test of its own), and the
output lands in a sentinel-filled [Nq + 3, D + 8] buffer whose spare rows and columns must come back untouched.

  selection  out == V[sel] bit for bit: a wrong key, row, head or column anywhere in the load, V^T, MFMA or epilogue mapping shows as another 16-bit code
  weighted   assert_exact against sum 2^s v / sum 2^s: one key too many or too few in the ragged tile moves the denominator by one weight
  uniform    Q = 0 / every key masked: the mean over exactly Nkv keys
  boost      tile sums on both sides of the f16 build's 2^15 bound and a P of 2^16: finite, assert_close
  gates      2 sigmoid(logit) in the epilogue, logits given and from K-slice partial sums: assert_close

Sensitivity, measured once on an MI355X with the ragged tile's bound  kv0 + kl >= Nkv  written  >  (one zero key too many, no out-of-range read): the
uniform, every-key-masked, weighted-plain, boost and gate tests fail at every ragged Nkv (37, 197, 261) on both builds, 184 cases; of the 43 earlier
test_flash_attn* / float16 attention cases only the four with Nkv = 37 or 68 notice.  The key-mask form hides that mutant unless every key is masked (the
mask word's bit for key Nkv is 0), and the selection tests do by design (the extra key weighs 2^-48).  Every exact case passes on the unmodified
kernel, so v_exp_f32 did return exact powers of two at the integer arguments used here (-80 .. 40)."""
import pytest
import torch

import attention_exact_ref as R
from attention_exact_ref import BF, F16

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(BF, id="bf16"), pytest.param(F16, id="f16")]
SENT = 77.0                     # exact in both 16-bit types; no output of these tests equals it
SCALE = R.ln2_scale()


def shape_id(s):
    return "q%d-kv%d-h%d-d%d" % s


@pytest.fixture(scope="module")
def nv(dev):
    from ltx_2_mlx_amd import _native
    return _native


def run_attn(nv, dev, dtype, form, q, k, v, heads, hd, **kw):
    """One attention call of the given form through the C ABI -> out [Nq, H*hd] (CPU).  Asserts the output buffer's guard rows and columns."""
    nq, nkv, D = q.shape[0], k.shape[0], heads * hd
    ld = 2 * D + 8
    fused = torch.full((max(nq, nkv), ld), SENT, dtype=dtype)
    fused[:nq, :D] = q
    fused[:nkv, D:2 * D] = k
    fused = fused.to(dev)
    qd, kd = fused[:, :D], fused[:, D:2 * D]
    vt = R.vt_layout(v, heads, hd).to(dev)
    npad = vt.shape[2]
    ldo = D + 8
    out0 = torch.full((nq + 3, ldo), SENT, dtype=dtype)
    out = out0.to(dev)
    L = nv.lib(dtype)
    common = (nv.ptr(qd), ld, nv.ptr(kd), ld, nv.ptr(vt), npad, nv.ptr(out), ldo, nq, nkv, heads, hd, SCALE)
    if form == "plain":
        nv.check(L.ltx2_flash_attn(*common, nv.stream()))
    elif form == "rowscale":
        t, _ = R.rowscale_partials(D)
        q_ss = torch.full((nq, R.QSS_LD), t, dtype=torch.float32, device=dev)
        nv.check(L.ltx2_flash_attn_rowscale(*common, nv.ptr(q_ss), R.QSS_LD, D, R.Q_EPS, nv.stream()))
    elif form == "gated":
        gate_ld = heads + 3
        logits = torch.full((nq, gate_ld), 1e4, dtype=torch.float32)       # the spare columns would saturate a gate that read them
        logits[:, :heads] = kw["logits"]
        logits = logits.to(dev)
        nv.check(L.ltx2_flash_attn_gated(*common, nv.ptr(logits), gate_ld, nv.stream()))
    elif form == "gated_parts":
        x, gw, gb = kw["x"], kw["gate_w"], kw["gate_b"]
        ldx = x.shape[1] + 8
        xd = torch.full((nq, ldx), SENT, dtype=dtype)
        xd[:, :x.shape[1]] = x
        xd, gw, gb = xd.to(dev), gw.contiguous().to(dev), gb.float().contiguous().to(dev)
        parts = torch.empty(8, nq, heads, dtype=torch.float32, device=dev)
        nv.check(L.ltx2_flash_attn_gated_parts(*common, nv.ptr(xd), ldx, nv.ptr(gw), nv.ptr(gb), x.shape[1], nv.ptr(parts), nv.stream()))
    elif form == "keymask":
        mask = kw["keep"].to(torch.float32).to(dev)
        words = torch.empty(npad // 64, dtype=torch.int64, device=dev)
        nv.check(L.ltx2_flash_attn_keymask(*common, nv.ptr(mask), nv.ptr(words), nv.stream()))
    else:
        raise ValueError(form)
    got = out.cpu()
    bits, bits0 = got.view(torch.int16), out0.view(torch.int16)
    assert torch.equal(bits[nq:], bits0[nq:]), f"{form}: rows >= Nq written"
    assert torch.equal(bits[:, D:], bits0[:, D:]), f"{form}: columns >= H*hd written"
    return got[:nq, :D].contiguous()


def assert_selected(got, inp, what):
    exp = inp["expect"]
    if not torch.equal(got.view(torch.int16), exp.view(torch.int16)):
        bad = got.view(torch.int16) != exp.view(torch.int16)
        i, c = (int(t) for t in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from V[sel]; first at row {i}, column {c}: "
                             f"got {float(got[i, c])!r}, expected {float(exp[i, c])!r}; rows affected: {bad.any(dim=1).nonzero().reshape(-1).tolist()[:16]}")


# ------------------------------------------------------------------------------------------ 1. vt_transpose == the documented layout
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", R.HD)
@pytest.mark.parametrize("nkv", [1, 37, 64, 65, 197])
def test_vt_transpose_is_the_documented_layout(nv, dev, dtype, hd, nkv):
    heads = 3
    D = heads * hd
    v = R.v_codes(nkv, heads, hd, dtype)
    want = R.vt_layout(v, heads, hd)
    npad = want.shape[2]
    assert npad % 64 == 0 and npad - nkv < 64
    wide = torch.full((nkv, 3 * D + 8), SENT, dtype=dtype)            # the V columns of a fused QKV buffer, row stride 3 D + 8
    wide[:, 2 * D:3 * D] = v
    wide = wide.to(dev)
    for src, ld in ((v.to(dev), D), (wide[:, 2 * D:3 * D], 3 * D + 8)):
        assert src.stride(0) == ld
        vt = torch.full((heads + 1, hd, npad), SENT, dtype=dtype, device=dev)       # one spare head as a guard
        nv.check(nv.lib(dtype).ltx2_vt_transpose(nv.ptr(src), ld, nv.ptr(vt), nkv, npad, heads, hd, nv.stream()))
        got = vt.cpu()
        assert torch.equal(got[:heads].view(torch.int16), want.view(torch.int16)), f"ld={ld}"
        assert int((got[:heads] != 0).sum()) == heads * hd * nkv                   # every pad position is zero: V itself has no zero
        assert (got[heads] == SENT).all()


# ------------------------------------------------------------------------------------------ 2. selection, plain form
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", R.GAPS)
@pytest.mark.parametrize("shape", R.ALL_SHAPES, ids=shape_id)
def test_selection_plain(nv, dev, dtype, g, shape):
    nq, nkv, heads, hd = shape
    inp = R.selection_inputs(dtype, nq, nkv, heads, hd, g)
    got = run_attn(nv, dev, dtype, "plain", inp["q"], inp["k"], inp["v"], heads, hd)
    assert_selected(got, inp, "plain")


# ------------------------------------------------------------------------------------------ 3. selection through every other form, factor exactly 1
# (the row-scale form exists for head_dim 128 only: capi.hip refuses 64)
FORM_CASES = [(form, s) for form in ("rowscale", "gated", "gated_parts", "keymask_all", "keymask_sel") for s in R.FORM_SHAPES
              if form != "rowscale" or s[3] == 128]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", R.GAPS)
@pytest.mark.parametrize("form,shape", FORM_CASES, ids=lambda v: v if isinstance(v, str) else shape_id(v))
def test_selection_other_forms(nv, dev, dtype, g, form, shape):
    nq, nkv, heads, hd = shape
    inp = R.selection_inputs(dtype, nq, nkv, heads, hd, g, masked=(form == "keymask_sel"))
    kw = {}
    if form == "gated":
        kw["logits"] = torch.zeros(nq, heads)                           # 2 / (1 + exp(0)) = 1
    elif form == "gated_parts":
        kw = {"x": torch.zeros(nq, R.GATE_DQ, dtype=dtype), "gate_w": R.gate_parts_inputs(dtype, nq, heads)[1], "gate_b": torch.zeros(heads)}
    elif form == "keymask_all":
        kw["keep"] = torch.ones(nkv, dtype=torch.bool)
    elif form == "keymask_sel":
        kw["keep"] = inp["keep"]
    got = run_attn(nv, dev, dtype, form.split("_")[0] if form.startswith("keymask") else form, inp["q"], inp["k"], inp["v"], heads, hd, **kw)
    assert_selected(got, inp, form)


def test_rowscale_refuses_head_dim_64(nv, dev):
    inp = R.selection_inputs(BF, 37, 37, 3, 64, 24)
    with pytest.raises(ValueError):
        run_attn(nv, dev, BF, "rowscale", inp["q"], inp["k"], inp["v"], 3, 64)


# ------------------------------------------------------------------------------------------ 4. weighted, plain and key-mask forms
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.ALL_SHAPES, ids=shape_id)
def test_weighted_plain(nv, dev, dtype, shape):
    nq, nkv, heads, hd = shape
    inp = R.weighted_inputs(dtype, nq, nkv, heads, hd)
    ref, _, exact_div = R.ref64(inp["q"], inp["k"], inp["v"], heads, hd)
    got = run_attn(nv, dev, dtype, "plain", inp["q"], inp["k"], inp["v"], heads, hd)
    R.assert_exact(got, ref, dtype, "weighted", exact_div)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", R.MASK_KINDS)
@pytest.mark.parametrize("shape", R.FORM_SHAPES, ids=shape_id)
def test_weighted_keymask(nv, dev, dtype, kind, shape):
    nq, nkv, heads, hd = shape
    inp = R.weighted_inputs(dtype, nq, nkv, heads, hd)
    keep = R.weighted_mask(nkv, kind)
    ref, _, exact_div = R.ref64(inp["q"], inp["k"], inp["v"], heads, hd, keep)          # the masked keys are dropped from the reference
    got = run_attn(nv, dev, dtype, "keymask", inp["q"], inp["k"], inp["v"], heads, hd, keep=keep)
    R.assert_exact(got, ref, dtype, f"weighted, mask {kind}", exact_div)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.MEAN_SHAPES, ids=shape_id)
def test_every_key_masked_is_the_mean_over_the_real_keys(nv, dev, dtype, shape):
    """attention.h: a row whose keys are all masked gets the uniform result over them -- the Nkv real keys, not the pad of the ragged tile."""
    nq, nkv, heads, hd = shape
    inp = R.weighted_inputs(dtype, nq, nkv, heads, hd)
    keep = torch.zeros(nkv, dtype=torch.bool)
    ref, _, exact_div = R.ref64(inp["q"], inp["k"], inp["v"], heads, hd, keep)
    assert torch.equal(ref, inp["v"].double().sum(dim=0)[None, :].expand(nq, -1) / nkv)
    got = run_attn(nv, dev, dtype, "keymask", inp["q"], inp["k"], inp["v"], heads, hd, keep=keep)
    R.assert_exact(got, ref, dtype, "all keys masked", exact_div)


# ------------------------------------------------------------------------------------------ 5. uniform
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.MEAN_SHAPES, ids=shape_id)
def test_uniform_is_the_mean_over_exactly_nkv_keys(nv, dev, dtype, shape):
    """Q = 0: every real key weighs 1, every pad key of the ragged tile 0."""
    nq, nkv, heads, hd = shape
    inp = R.weighted_inputs(dtype, nq, nkv, heads, hd)
    q0 = torch.zeros_like(inp["q"])
    ref, _, exact_div = R.ref64(q0, inp["k"], inp["v"], heads, hd)
    assert torch.equal(ref, inp["v"].double().sum(dim=0)[None, :].expand(nq, -1) / nkv)
    got = run_attn(nv, dev, dtype, "plain", q0, inp["k"], inp["v"], heads, hd)
    R.assert_exact(got, ref, dtype, "uniform", exact_div)


# ------------------------------------------------------------------------------------------ 6. the boost variant
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.BOOST_SHAPES, ids=shape_id)
def test_boost_across_the_half_precision_bound(nv, dev, dtype, shape):
    """Tile sums below 2^12, inside (2^12, 2^15] and above 2^15, a single P of 2^16: the f16 build must leave the stale-maximum path exactly where IEEE
    half would overflow (AT_P_BIG); the bf16 build keeps all of it on that path."""
    nq, nkv, heads, hd = shape
    inp = R.boost_inputs(dtype, nq, nkv, heads, hd)
    ref, absref, _ = R.ref64(inp["q"], inp["k"], inp["v"], heads, hd)
    got = run_attn(nv, dev, dtype, "plain", inp["q"], inp["k"], inp["v"], heads, hd)
    assert torch.isfinite(got).all()
    R.assert_close(got, ref, absref, dtype, "boost")


# ------------------------------------------------------------------------------------------ 7. gates with non-unit factors
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["gated", "gated_parts"])
@pytest.mark.parametrize("shape", R.FORM_SHAPES, ids=shape_id)
def test_gates_scale_the_fp32_result(nv, dev, dtype, form, shape):
    nq, nkv, heads, hd = shape
    inp = R.weighted_inputs(dtype, nq, nkv, heads, hd)
    ref, absref, _ = R.ref64(inp["q"], inp["k"], inp["v"], heads, hd)
    if form == "gated":
        logits = R.gate_logits(nq, heads)
        kw = {"logits": logits}
    else:
        x, gw, gb, logits = R.gate_parts_inputs(dtype, nq, heads)
        kw = {"x": x, "gate_w": gw, "gate_b": gb}
    f = R.gate_factor(logits)
    got = run_attn(nv, dev, dtype, form, inp["q"], inp["k"], inp["v"], heads, hd, **kw)
    R.assert_close(got, R.apply_gate(ref, f, heads, hd), R.apply_gate(absref, f, heads, hd), dtype, form)
