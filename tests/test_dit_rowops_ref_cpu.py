"""CPU checks of tests/dit_rowops_ref.py, the references and bounds test_dit_rowops_gpu.py holds the DiT row kernels to:

  * each fp64 reference agrees with the oracle (oracle.dit.rms_norm / adaln_forward / apply_split_rope on rope_split_tables) on the GPU
    cases' inputs, to fp32's accuracy -- the oracle works in fp32;
  * each bound is sound: an fp32 emulation of the kernel's arithmetic, in the kernel's summation order and in torch's, with and without
    fused multiply-adds, stays inside it on every GPU case's inputs;
  * each bound is not vacuous: one element moved by a 16-bit ulp plus the slack, eps omitted, and the sum divided by D - 4 all exceed it."""
import pytest
import torch

import dit_rowops_ref as R
from dit_rowops_ref import BF, F16

DTYPES = [pytest.param(BF, id="bf16"), pytest.param(F16, id="f16")]
VARIANTS = [("kernel", False), ("kernel", True), ("torch", False), ("torch", True)]


def norm_case_inputs(rows, D, ln, ps, per_token):
    x = R.norm_rows(rows, D, 7 * rows + D + ln)
    tabs, _ = R.norm_tables(rows, D, rows + D, ps, per_token)
    return x, tabs


# ------------------------------------------------------------------------------------------ the references against the oracle
def test_norm_reference_matches_oracle():
    from oracle import dit
    worst = 0.0
    for rows, D, ln, ps, per_token in R.norm_cases():
        if ln:
            continue                                           # the oracle's AdaLN is the RMS form; LayerNorm is checked against torch below
        x, t = norm_case_inputs(rows, D, ln, ps, per_token)
        exact, _ = R.norm_exact(x, R.EPS, ln, **t)
        z = torch.zeros(D)
        sc = sum((v for v in (t["sct"], t["sce"]) if v is not None), z)
        sh = sum((v for v in (t["sht"], t["she"]) if v is not None), z)
        ref = dit.adaln_forward(x, sc, sh, R.EPS)
        err = (exact - ref.double()).abs() / (ref.double().abs() + 1.0)
        worst = max(worst, float(err.max()))
        if ps == "none":
            assert float(((exact - dit.rms_norm(x, None, R.EPS).double()).abs()).max()) < 2e-5
    assert worst < 2e-5                                        # a few fp32 roundings of values of a few units


def test_layernorm_reference_matches_torch():
    for rows, D in R.NORM_ROW_SHAPES:
        x = R.norm_rows(rows, D, 7 * rows + D + 1)
        tabs, _ = R.norm_tables(rows, D, rows + D, "all", False)
        exact, _ = R.norm_exact(x, R.EPS, 1, **tabs)
        ln = torch.nn.functional.layer_norm(x.double(), (D,), eps=R.f32(R.EPS))
        ref = ln * (1 + tabs["sct"].double() + tabs["sce"].double()) + tabs["sht"].double() + tabs["she"].double()
        assert float((exact - ref).abs().max()) < 1e-9


@pytest.mark.parametrize("D,hd,rows", R.QK_CASES)
def test_qk_reference_matches_oracle(D, hd, rows):
    from oracle import dit
    buf, wq, wk, cos, sin = R.qk_inputs(D, hd, rows, BF, D + hd + rows)
    _, qo, ko = R.qk_layout(D)
    H = D // hd
    c4, s4 = cos.reshape(rows, H, hd // 2).permute(1, 0, 2)[None], sin.reshape(rows, H, hd // 2).permute(1, 0, 2)[None]
    for off, w in ((qo, wq), (ko, wk)):
        x = buf[:, off:off + D]
        exact, _ = R.qk_exact(x, w, hd, R.EPS, cos, sin)
        ref = dit.apply_split_rope(dit.rms_norm(x.float(), w, R.EPS)[None], c4, s4)[0]
        assert float(((exact - ref.double()).abs() / (ref.double().abs() + 1.0)).max()) < 2e-5
        plain, _ = R.qk_exact(x, w, hd, R.EPS)
        assert float(((plain - dit.rms_norm(x.float(), w, R.EPS).double()).abs() / (plain.abs() + 1.0)).max()) < 2e-5


# ------------------------------------------------------------------------------------------ the bounds: sound ...
@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_bound_holds_for_fp32_emulations(dtype):
    worst = 0.0
    for rows, D, ln, ps, per_token in R.norm_cases():
        x, t = norm_case_inputs(rows, D, ln, ps, per_token)
        exact, E = R.norm_exact(x, R.EPS, ln, **t)
        for order, fused in VARIANTS:
            got = R.norm_emulate(x, R.EPS, ln, order=order, fused=fused, **t).to(dtype)
            r = R.ratio16(got, exact, E, dtype)
            assert r <= 1.0, (rows, D, ln, ps, per_token, order, fused, r)
            worst = max(worst, r)
    assert worst > 0.5                                         # the half-ulp term is attained: the bound is a 16-bit rounding, not more


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,hd,rows", R.QK_CASES)
def test_qk_bound_holds_for_fp32_emulations(dtype, D, hd, rows):
    buf, wq, wk, cos, sin = R.qk_inputs(D, hd, rows, dtype, D + hd + rows)
    _, qo, ko = R.qk_layout(D)
    for off, w in ((qo, wq), (ko, wk)):
        x = buf[:, off:off + D]
        for cs in ((cos, sin), (None, None)):
            exact, E = R.qk_exact(x, w, hd, R.EPS, *cs)
            for order, fused in VARIANTS:
                got = R.qk_emulate(x, w, hd, R.EPS, *cs, order=order, fused=fused).to(dtype)
                r = R.ratio16(got, exact, E, dtype)
                assert r <= 1.0, (off, cs[0] is None, order, fused, r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_head_gate_bound_holds_for_fp32_emulation(dtype):
    g = R.gen(5)
    rows, H, hd = 37, 5, 8
    att = torch.randn(rows, H * hd, generator=g).to(dtype)
    for logits in (torch.randint(-30, 31, (rows, H), generator=g).float(), 3 * torch.randn(rows, H, generator=g)):
        exact, E = R.head_gate_exact(att, logits, hd)
        got = R.head_gate_emulate(att, logits, hd).to(dtype)
        assert R.ratio16(got, exact, E, dtype) <= 1.0
        bad = R.shift_one_ulp(got.double(), exact, E, dtype, 17)
        assert R.ratio16(bad, exact, E, dtype) > 1.0
        wrong_head = R.head_gate_emulate(att, logits.roll(1, 1), hd).to(dtype)           # the gate of the neighbouring head
        assert R.ratio16(wrong_head, exact, E, dtype) > 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_gate_logit_bound_holds_for_fp32_products(dtype):
    g = R.gen(6)
    M, H, Dq = 37, 17, 2176
    x = torch.randn(M, Dq, generator=g).to(dtype)
    w = (torch.randn(H, Dq, generator=g) / Dq ** 0.5).to(dtype)
    b = 0.5 * torch.randn(H, generator=g)
    exact, E = R.gate_logits_exact(x, w, b)
    one = x.float() @ w.float().t() + b                                                    # torch's blocked order
    parts = sum((x[:, k:k + 32].float() @ w[:, k:k + 32].float().t() for k in range(0, Dq, 32)), torch.zeros(M, H)) + b   # 32-wide steps
    for got in (one, parts):
        assert float(((got.double() - exact).abs() / E).max()) <= 1.0
    dropped = one - x[:, 512:520].float() @ w[:, 512:520].float().t()                     # one 8-element K chunk missing
    assert float(((dropped.double() - exact).abs() / E).max()) > 1.0


# ------------------------------------------------------------------------------------------ ... and not vacuous
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wrong", ["no_eps", "d_minus_4"])
def test_norm_bound_rejects_wrong_statistics(dtype, wrong):
    for rows, D, ln, ps, per_token in R.norm_cases():
        if rows < 4 or ps != "all" or per_token:
            continue                                           # the tiny row (var ~ eps) exists from four rows on; one pointer set is enough
        x, t = norm_case_inputs(rows, D, ln, ps, per_token)
        exact, E = R.norm_exact(x, R.EPS, ln, **t)
        for order, fused in VARIANTS:
            got = R.norm_emulate(x, R.EPS, ln, order=order, fused=fused, wrong=wrong, **t).to(dtype)
            assert R.ratio16(got, exact, E, dtype) > 1.0, (rows, D, ln, order, fused)


@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_bound_rejects_one_ulp(dtype):
    for rows, D, ln, ps, per_token in R.norm_cases():
        if ps != "all" or per_token:
            continue
        x, t = norm_case_inputs(rows, D, ln, ps, per_token)
        exact, E = R.norm_exact(x, R.EPS, ln, **t)
        got = R.norm_emulate(x, R.EPS, ln, **t).to(dtype).double()
        for index in (0, D - 1, rows * D - 1):
            assert R.ratio16(R.shift_one_ulp(got, exact, E, dtype, index), exact, E, dtype) > 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,hd,rows", [c for c in R.QK_CASES if c[2] == 37])
def test_qk_bound_rejects_wrong_variants(dtype, D, hd, rows):
    buf, wq, wk, cos, sin = R.qk_inputs(D, hd, rows, dtype, D + hd + rows)
    _, qo, _ = R.qk_layout(D)
    x = buf[:, qo:qo + D]
    exact, E = R.qk_exact(x, wq, hd, R.EPS, cos, sin)
    got = R.qk_emulate(x, wq, hd, R.EPS, cos, sin).to(dtype).double()
    assert R.ratio16(R.shift_one_ulp(got, exact, E, dtype, D + 3), exact, E, dtype) > 1.0
    tiny = (x.float() * 1e-3).to(dtype)                        # ms of the order of eps: the rows where eps matters
    ex_t, E_t = R.qk_exact(tiny, wq, hd, R.EPS, cos, sin)
    assert R.ratio16(R.qk_emulate(tiny, wq, hd, R.EPS, cos, sin).to(dtype), ex_t, E_t, dtype) <= 1.0
    assert R.ratio16(R.qk_emulate(tiny, wq, hd, R.EPS, cos, sin, wrong="no_eps").to(dtype), ex_t, E_t, dtype) > 1.0
    if D >= 128:                                               # at D = 16, D - 4 is off by a quarter: trivially caught, nothing to learn
        assert R.ratio16(R.qk_emulate(x, wq, hd, R.EPS, cos, sin, wrong="d_minus_4").to(dtype), exact, E, dtype) > 1.0
    swapped = R.qk_emulate(x, wq, hd, R.EPS, cos, -sin).to(dtype)                           # the sign of sin
    assert R.ratio16(swapped, exact, E, dtype) > 1.0


def test_keymask_words_reference():
    m = torch.zeros(200)
    m[[0, 63, 64, 130, 199]] = 1.0
    m[5] = -0.0
    w = R.keymask_words(m, 4)
    assert w.tolist() == [1 - 2 ** 63, 1, 4, 128]             # bit 63 set reads as the sign of the int64 word
    assert R.keymask_words(torch.ones(1), 1).tolist() == [1]


def test_ulp16_and_integer_product():
    assert float(R.ulp16(torch.tensor([1.0]), BF)) == 2.0 ** -7 and float(R.ulp16(torch.tensor([1.0]), F16)) == 2.0 ** -10
    assert float(R.ulp16(torch.tensor([0.0]), BF)) == 2.0 ** -133 and float(R.ulp16(torch.tensor([0.0]), F16)) == 2.0 ** -24
    assert float(R.ulp16(torch.tensor([1.99]), BF)) == 2.0 ** -7 and float(R.ulp16(torch.tensor([2.0]), BF)) == 2.0 ** -6
    x, w, b = R.int_tensor((37, 4096), 1), R.int_tensor((32, 4096), 2), R.int_tensor((32,), 3)
    ref = R.gate_logits_int(x, w, b)
    assert int(ref.abs().max()) < 2 ** 24 and torch.equal((x @ w.t() + b).long(), ref)      # fp32 holds every partial sum exactly
    assert torch.equal(x.to(BF).float(), x) and torch.equal(x.to(F16).float(), x)
