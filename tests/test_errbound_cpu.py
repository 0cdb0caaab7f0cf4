"""The element-wise metric of tests/errbound.py, proven on the CPU.

1. The float64 references equal torch's own convolutions (1e-12) for every tap form tests/test_elementwise_gpu.py uses, and the
   oracle's attention.
2. A faithful emulation of what the kernels are allowed to do - an fp32 matmul in torch's own order, one round-to-nearest store;
   for attention an fp32 softmax, P rounded to bf16 in front of the PV product, the row sum from the unrounded exponentials -
   has ZERO violating elements on every shape of the GPU file.
3. Seven defects seeded into that emulation are each flagged by `check`; for the ones confined enough the whole-tensor rel-L2
   stays below the 1e-2 of tests/test_ops_gpu.py, which is the gap the element-wise files close.
"""
import pytest
import torch
import torch.nn.functional as F_

import errbound as E
from helpers import rel_l2
from oracle import unet_ref as uref

BF, F32 = torch.bfloat16, torch.float32
DT = {"f32": F32, "bf16": BF}


def _ops():
    from mm_diffusion import ops
    return ops


def _operands(M, Cin, Cout, ntaps, dt, seed, bias=True, res=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, Cin, generator=g).to(dt)
    w = (torch.randn(Cout, ntaps * Cin, generator=g) * (ntaps * Cin) ** -0.5).to(dt)
    b = torch.randn(Cout, generator=g) if bias else None
    r = torch.randn(M, Cout, generator=g).to(dt) if res else None
    return x, w, b, r


def _trunc_bf16(t):
    return (t.float().view(torch.int32) & -65536).view(F32).to(BF)


def emulate_conv(x, w, bias, res, taps, dims, out_dtype, defect=None):
    """fp32 accumulation in torch's order, bias and residual added in fp32, one round-to-nearest store; `defect` seeds one error."""
    M, Cin = x.shape
    D0, D1, D2 = dims
    gath = [g for g, _ in E.conv_gather(x.float(), taps, dims)]
    m = torch.arange(M)
    if defect == "corner_tap":                       # tap (+1, +1) - the one corner tap that lands - dropped at pixel (0, 0) of every frame
        gath[taps.index((0, 1, 1))][m % (D1 * D2) == 0] = 0
    if defect == "clip_boundary":                    # tap (+1, 0, 0) of the last frame of sample 0 reads sample 1's first frame
        t = taps.index((1, 0, 0))
        rows = m[(m < D0 * D1 * D2) & ((m // (D1 * D2)) % D0 == D0 - 1)]
        gath[t][rows] = x.float()[rows + D1 * D2]
    wf = w.float()
    if defect == "bf16_accumulator":                 # the accumulator rounded to bf16 after every K step of 64 channels
        acc = torch.zeros(M, w.shape[0])
        for t, g in enumerate(gath):
            for c0 in range(0, Cin, 64):
                acc = (acc + g[:, c0:c0 + 64] @ wf[:, t * Cin + c0:t * Cin + c0 + 64].t()).to(BF).float()
    else:
        acc = torch.cat(gath, dim=1) @ wf.t()
    if bias is not None:
        b = bias.clone()
        if defect == "bias_shift":                   # bias column c used for column c + 1 in the last 8 columns
            b[-8:] = bias[-9:-1]
        acc = acc + b
    if res is not None:
        r = res.float().clone()
        if defect == "residual_row":                 # the last (ragged) row takes the previous row's residual
            r[-1] = r[-2]
        acc = acc + r
    return _trunc_bf16(acc) if defect == "truncate" else acc.to(out_dtype)


def emulate_attn(q, k, v, heads, out_dtype, p_round=True, drop_key=None):
    """fp32 softmax; P rounded to bf16 in front of the PV product (p_round), the row sum from the unrounded exponentials."""
    Tq, C = q.shape
    ch = C // heads
    qh, kh, vh = (t.float().reshape(-1, heads, ch).permute(1, 0, 2) for t in (q, k, v))
    a = (qh * ch ** -0.5) @ kh.transpose(1, 2)
    if drop_key is not None:
        a[:, :, drop_key] = -1e30
    e = torch.exp(a - a.amax(-1, keepdim=True))
    l = e.sum(-1, keepdim=True)
    o = (e.to(BF).float() if p_round else e) @ vh
    return (o / l).permute(1, 0, 2).reshape(Tq, C).to(out_dtype)


# --------------------------------------------------------------------------- 1. the references
def test_tap_tables_are_the_package_s():
    ops = _ops()
    assert E.TAPS_1 == ops.TAPS_1 and E.TAPS_SPATIAL == ops.TAPS_SPATIAL and E.TAPS_TEMPORAL == ops.TAPS_TEMPORAL
    assert E.TAPS_TEMPORAL_D1 == ops.TAPS_TEMPORAL_D1 and all(E.taps_audio(d) == ops.taps_audio(d) for d in (1, 4, 16, 128))


def _close12(a, b):
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def _rows(x):            # [N, C, *spatial] -> [(n spatial), C]
    return x.movedim(1, -1).reshape(-1, x.shape[1])


def test_conv_rows_ref_equals_torch_convs():
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    # 1x1
    x, w, b = rn(3, 24, 5, 7), rn(40, 24, 1, 1), rn(40)
    r = rn(3 * 5 * 7, 40)
    ref, S = E.conv_rows_ref(_rows(x), ops.pack_conv_weight(w, torch.float64), b, r, E.TAPS_1, (1, 1, 1))
    _close12(ref, _rows(F_.conv2d(x, w, b)) + r)
    _close12(S, _rows(F_.conv2d(x.abs(), w.abs(), b.abs())) + r.abs())
    # spatial 3x3 over N * F frames (frame sides that divide nothing, and the 8 x 16 of the halo tile)
    for NF, H, W in ((2, 5, 7), (3, 8, 16)):
        x, w, b = rn(NF, 16, H, W), rn(24, 16, 3, 3), rn(24)
        ref, S = E.conv_rows_ref(_rows(x), ops.pack_conv_weight(w, torch.float64), b, None, E.TAPS_SPATIAL, (NF, H, W))
        _close12(ref, _rows(F_.conv2d(x, w, b, padding=1)))
        _close12(S, _rows(F_.conv2d(x.abs(), w.abs(), b.abs(), padding=1)))
        x3 = x.reshape(1, NF, 16, H, W).permute(0, 2, 1, 3, 4)                               # the same frames as one conv3d clip
        _close12(ref, _rows(F_.conv3d(x3, w[:, :, None], b, padding=(0, 1, 1))))
    # temporal k = 3 in both forms: D = (F, HW, 1) repeating over the samples, and D = (N, F, HW) with the taps on D1
    for N, F, HW in ((2, 1, 5), (2, 3, 5), (2, 16, 6), (2, 8, 16)):
        x, w, b = rn(N, 16, F, HW), rn(24, 16, 3), rn(24)
        want = _rows(F_.conv2d(x, w[..., None], b, padding=(1, 0)))
        wp = ops.pack_conv_weight(w, torch.float64)
        _close12(E.conv_rows_ref(_rows(x), wp, b, None, E.TAPS_TEMPORAL, (F, HW, 1))[0], want)
        _close12(E.conv_rows_ref(_rows(x), wp, b, None, E.TAPS_TEMPORAL_D1, (N, F, HW))[0], want)
    # audio, dilated, two samples (d = 128 > L: the side taps never land)
    for L, d in ((100, 1), (100, 4), (100, 16), (100, 128), (257, 16)):
        x, w, b = rn(2, 16, L), rn(24, 16, 3), rn(24)
        ref, S = E.conv_rows_ref(_rows(x), ops.pack_conv_weight(w, torch.float64), b, None, E.taps_audio(d), (L, 1, 1))
        _close12(ref, _rows(F_.conv1d(x, w, b, padding=d, dilation=d)))
        _close12(S, _rows(F_.conv1d(x.abs(), w.abs(), b.abs(), padding=d, dilation=d)))


@pytest.mark.parametrize("Tq,Tk,heads,ch", [(4, 4, 4, 16), (70, 70, 1, 96), (37, 130, 2, 48)])
def test_attn_ref_equals_the_oracle(Tq, Tk, heads, ch):
    """oracle.unet_ref._attend runs in fp32: agreement to fp32 rounding (its own error is a few 1e-7 on O(1) values)."""
    g = torch.Generator().manual_seed(2)
    q, k, v = torch.randn(Tq, heads * ch, generator=g), torch.randn(Tk, heads * ch, generator=g), torch.randn(Tk, heads * ch, generator=g)
    ref, Sv, e32 = E.attn_ref(q, k, v, heads)
    got = uref._attend(q.t()[None], k.t()[None], v.t()[None], heads)[0].t()
    assert float((got.double() - ref).abs().max()) < 1e-5
    assert bool((Sv >= ref.abs() - 1e-15).all()) and bool((e32 > 0).all())
    E.check(got, ref, e32, what="fp32 oracle")            # the oracle itself is an fp32 attention: inside the fp32-level term


# --------------------------------------------------------------------------- 2. the faithful emulation: zero violations
CONV = [(c, dt) for c in E.conv_cases() for dt in c["dtypes"]]


@pytest.mark.parametrize("case,dt", CONV, ids=[f"{c['name']}-{dt}" for c, dt in CONV])
def test_emulated_conv_has_no_violation(case, dt):
    dt = DT[dt]
    K = len(case["taps"]) * case["Cin"]
    for res in (False, True):
        x, w, b, r = _operands(case["M"], case["Cin"], case["Cout"], len(case["taps"]), dt, 3, res=res)
        ref, S = E.conv_rows_ref(x, w, b, r, case["taps"], case["dims"])
        E.check(emulate_conv(x, w, b, r, case["taps"], case["dims"], dt), ref, E.gemm_bound(ref, S, K, dt), case["pixels"], case["name"])


@pytest.mark.parametrize("name,M,Cin,Cout,taps,dims", E.strip_cases() + [("gn-loader", 1200, 256, 256, E.TAPS_1, (1, 1, 1)),
                                                                        ("strided", 200, 128, 64, E.TAPS_1, (1, 1, 1))],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_emulated_strip_shapes_have_no_violation(name, M, Cin, Cout, taps, dims):
    x, w, b, r = _operands(M, Cin, Cout, len(taps), BF, 4)
    ref, S = E.conv_rows_ref(x, w, b, r, taps, dims)
    E.check(emulate_conv(x, w, b, r, taps, dims, BF), ref, E.gemm_bound(ref, S, len(taps) * Cin, BF), what=name)


def _qkv(T, C, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(T, C, generator=g) * scale).to(dt) for _ in range(3))


ATTN = ([(T, T, h, ch) for T, h, ch in E.SELF_ATTN] + [(F, F, h, ch) for F, _, h, ch in E.TEMPORAL_ATTN]
        + [(HW, win * (L // F), h, ch) for F, HW, L, win, _, h, ch in E.CROSS_ATTN]
        + [(L - (F - 1) * (L // F), win * HW, h, ch) for F, HW, L, win, _, h, ch in E.CROSS_ATTN])


@pytest.mark.parametrize("Tq,Tk,heads,ch", sorted(set(ATTN)))
def test_emulated_attention_has_no_violation(Tq, Tk, heads, ch):
    for dt in (F32, BF):
        q, _, _ = _qkv(Tq, heads * ch, dt, 5)
        _, k, v = _qkv(Tk, heads * ch, dt, 6)
        ref, Sv, e32 = E.attn_ref(q, k, v, heads)
        E.check(emulate_attn(q, k, v, heads, dt, p_round=dt == BF), ref, E.attn_bound(ref, Sv, dt, e32), what=f"attn {dt}")
    E.check(emulate_attn(q, k, v, heads, BF, p_round=False), ref, E.attn_bound(ref, Sv, BF, e32, p_round=0.0), what="attn, P in fp32")


def spike_qkv(spike_key=250, scale=40.0):
    """The input of tests/test_ops_gpu.py::test_attention_softmax_spike: one key aligned with query 7."""
    g = torch.Generator().manual_seed(28)
    qkv = (torch.randn(300, 192, generator=g).to(BF).float()) * 0.3
    qkv[spike_key, 64:128] = qkv[7, :64] * scale
    return qkv.to(BF)


def test_emulated_softmax_spike_has_no_violation():
    qkv = spike_qkv()
    q, k, v = qkv[:, :64], qkv[:, 64:128], qkv[:, 128:]
    ref, Sv, e32 = E.attn_ref(q, k, v, 1)
    E.check(emulate_attn(q, k, v, 1, BF), ref, E.attn_bound(ref, Sv, BF, e32), what="spike")


# --------------------------------------------------------------------------- 3. the seeded defects
# name -> (M, Cin, Cout, taps, dims, pixels, whether the whole-tensor rel-L2 of tests/test_ops_gpu.py (1e-2) lets it pass)
DEFECTS = {
    "corner_tap":       (4 * 16 * 32, 64, 136, E.TAPS_SPATIAL, (4, 16, 32), 512, True),
    "bf16_accumulator": (4 * 16 * 32, 64, 136, E.TAPS_SPATIAL, (4, 16, 32), 512, True),
    "truncate":         (293, 256, 264, E.TAPS_1, (1, 1, 1), None, True),
    "residual_row":     (128 * 100 + 37, 64, 264, E.TAPS_1, (1, 1, 1), None, True),      # one row in 12837: rel-L2 ~ 12837 ** -0.5
    "bias_shift":       (293, 256, 264, E.TAPS_1, (1, 1, 1), None, False),
    "clip_boundary":    (2 * 16 * 6, 64, 72, E.TAPS_TEMPORAL, (16, 6, 1), None, False),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_seeded_conv_defect_is_flagged(defect):
    M, Cin, Cout, taps, dims, pixels, l2_blind = DEFECTS[defect]
    x, w, b, r = _operands(M, Cin, Cout, len(taps), BF, 7)
    ref, S = E.conv_rows_ref(x, w, b, r, taps, dims)
    bound = E.gemm_bound(ref, S, len(taps) * Cin, BF)
    good = emulate_conv(x, w, b, r, taps, dims, BF)
    assert E.check(good, ref, bound, pixels, "unmodified") <= 1.0
    bad = emulate_conv(x, w, b, r, taps, dims, BF, defect=defect)
    assert not torch.equal(good, bad)
    nbad, worst, _ = E.violations(bad, ref, bound)
    l2 = rel_l2(bad.float(), ref)
    print(f"{defect}: {nbad} of {bad.numel()} elements outside the bound, worst ratio {worst:.2f}, whole-tensor rel-L2 {l2:.2e}")
    with pytest.raises(AssertionError, match="outside the bound"):
        E.check(bad, ref, bound, pixels, defect)
    assert nbad > 0 and worst > 1.0
    if l2_blind:
        assert l2 < 1e-2            # the metric of tests/test_ops_gpu.py passes this defect


def test_seeded_attention_defect_is_flagged():
    """One key of a ragged last key tile (T = 70 = 64 + 6) left out of the softmax."""
    T, heads, ch = 70, 1, 96
    q, k, v = _qkv(T, heads * ch, BF, 8)
    ref, Sv, e32 = E.attn_ref(q, k, v, heads)
    bound = E.attn_bound(ref, Sv, BF, e32)
    assert E.check(emulate_attn(q, k, v, heads, BF), ref, bound, what="unmodified") <= 1.0
    bad = emulate_attn(q, k, v, heads, BF, drop_key=T - 1)
    nbad, worst, _ = E.violations(bad, ref, bound)
    print(f"dropped key: {nbad} of {bad.numel()} elements outside the bound, worst ratio {worst:.2f}, rel-L2 {rel_l2(bad.float(), ref):.2e}")
    with pytest.raises(AssertionError, match="outside the bound"):
        E.check(bad, ref, bound, what="dropped key")
    # the same miss in ONE query row (one wave's key mask): invisible to the whole-tensor metric, still flagged
    one = emulate_attn(q, k, v, heads, BF)
    one[3] = bad[3]
    assert rel_l2(one.float(), ref) < 1e-2 and E.violations(one, ref, bound)[0] > 0


def test_check_reports_nonfinite_and_location():
    ref = torch.zeros(300, 140, dtype=torch.float64)
    bound = torch.full_like(ref, 1e-3)
    y = torch.zeros(300, 140)
    assert E.check(y, ref, bound) == 0.0
    y[129, 5], y[257, 133] = float("nan"), 1.0
    with pytest.raises(AssertionError) as ei:
        E.check(y, ref, bound, pixels=100, what="probe")
    s = str(ei.value)
    assert "2 of 42000" in s and "non-finite: 1" in s and "(129,5)" in s and "(257,133)" in s
    assert "by row % 128: 1:2" in s and "by column % 128: 5:2" in s and "by pixel (row % 100)" in s
