"""mmd_resample / mmd_resample_stats, the producers' statistics records, mmd_bilinear_concat(_rows) and the chain producer -> records ->
mmd_gn_finalize_stats against float64, ELEMENT BY ELEMENT and RECORD BY RECORD (tests/errbound_fwd.py: the references, the bounds and
their derivation, the case lists; tests/test_errbound_fwd_cpu.py: the metric proven on seeded defects).

Every case calls the kernel through mm_diffusion.ops with NaN-prefilled outputs, builds the reference with torch double ops on the
STORED operands - never with a libmmd kernel - and admits ZERO elements outside the per-element bound.  Every (64-row record, channel
quad) pair (sum, sum of squares) meets the float64 sums of its own 256 stored values within its own bound (`check_records`): no
global max-scale.  The nearest upsample at scale 1 stays torch.equal, the output of the stats= variant stays bitwise the plain one,
the x half of bilinear_concat is an exact copy and the pad columns of bilinear_concat_rows are exactly zero.

Worst error / bound ratio, as printed by the tests (`-s`) on an MI355X (a record of headroom, not a tolerance):

    kernel                                    dtype  cases  worst ratio
    resample pool                             bf16       5        0.996
    resample pool                             f32        5        0.691
    resample nearest upsample                 both       6        0 (exact at scale 1; 0.25 is a power of two)
    resample_stats records                    f32        4        0.018
    conv_gemm records, tile 64                bf16/f32   4/4      0.011 / 0.009
    conv_gemm records, tiles 128, 129         bf16/f32   4/4      0.008 / 0.007
    conv_gemm records, tile 131               bf16       2        0.007
    bilinear_concat, bilinear_concat_rows f32 f32        6        0.238
    bilinear_concat_rows bf16                 bf16       6        0.984
    chain: records (all six producers)        f32       12        0.010
    chain: a / b / mean / rstd                f32       12        0.011

Every case: zero violating elements, zero non-finite outputs.  The records sit at 0.01: the any-order bound grants each of 255
additions a full u.  Run time on an MI355X: 1.7 s for the 41 cases.
"""
import pytest
import torch

import errbound as E
import errbound_fwd as W

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
DT = W.DT
SENTINEL = 1e4


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mm_diffusion import ops as o
    return o


def _cu(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def _slice(rows, C, dtype, extra, pad, fill):
    buf = torch.full((rows, C + extra), SENTINEL, dtype=dtype, device="cuda")
    view = buf[:, pad:pad + C]
    view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
    return buf, view


def _untouched(buf, pad, C, what):
    assert bool((buf[:, :pad] == SENTINEL).all()) and bool((buf[:, pad + C:] == SENTINEL).all()), f"{what}: wrote outside the output view"


def _nan(*s):
    return torch.full(s, float("nan"), dtype=F32, device="cuda")


# --------------------------------------------------------------------------- resample, resample_stats
@pytest.mark.parametrize("case", W.resample_cases(), ids=lambda c: c[0])
def test_resample_elementwise(ops, case):
    name, dt, NF, Hh, Ww, C, fh, fw, mode, scale, strided, stats = case
    x, = _cu(W.resample_inputs(NF, Hh, Ww, C, dt))
    ref, bound = W.resample_ref(x, NF, Hh, Ww, fh, fw, mode, scale, DT[dt])
    Mo = ref.shape[0]
    xin = _slice(x.shape[0], C, x.dtype, 40, 16, x)[1] if strided else x
    buf, out = _slice(Mo, C, x.dtype, 48 if strided else 0, 8 if strided else 0, float("nan"))
    ops.resample(xin, out, NF, Hh, Ww, fh, fw, mode, scale)
    worst = E.check(out, ref, bound, what=f"resample {name}")
    if strided:
        _untouched(buf, 8, C, name)
    if mode == 1 and scale == 1.0:
        assert torch.equal(out.double(), ref), f"resample {name}: the nearest upsample at scale 1 is a copy"
    wrec = 0.0
    if stats:
        wide = torch.full((Mo // 64, C // 4 + 10, 2), SENTINEL, dtype=F32, device="cuda")
        rec = wide[:, 6:6 + C // 4]
        rec.fill_(float("nan"))
        buf2, out2 = _slice(Mo, C, x.dtype, 48 if strided else 0, 8 if strided else 0, float("nan"))
        ops.resample(xin, out2, NF, Hh, Ww, fh, fw, mode, scale, stats=rec)
        assert torch.equal(out2.view(torch.int16), out.view(torch.int16)), f"resample {name}: stats= changed the output"
        wrec = W.check_records(rec, W.record_values(out2), f"resample_stats {name}: records")
        assert bool((wide[:, :6] == SENTINEL).all()) and bool((wide[:, 6 + C // 4:] == SENTINEL).all())
    print(f"\nRATIO resample {dt} {name}: {worst:.3f} records {wrec:.3f}")


# --------------------------------------------------------------------------- conv_gemm records
@pytest.mark.parametrize("dt,tile", [(dt, t) for dt in ("bf16", "f32") for t in (64, 128, 129, 131) if (dt, t) != ("f32", 131)])     # tile 131 is bf16 only
def test_conv_gemm_records_per_record(ops, dt, tile):
    worst, n = 0.0, 0
    for M, Cin, Cout in W.GEMM_RECORD_CASES:
        if tile == 131 and not W.strip_ok(dt, Cin, Cout):
            continue
        g = torch.Generator().manual_seed(M + Cin + Cout)
        x = (torch.randn(M, Cin, generator=g) + 0.4).to(DT[dt]).cuda()
        w = (torch.randn(Cout, Cin, generator=g) * Cin ** -0.5).to(DT[dt]).cuda()
        bias = torch.randn(Cout, generator=g).cuda()
        res = torch.randn(M, Cout, generator=g).to(DT[dt]).cuda() if M != 192 else None
        rec = _nan(M // 64, Cout // 4, 2)
        y = ops.conv_gemm(x, w, bias, residual=res, tile=tile, stats=rec)
        assert torch.equal(y, ops.conv_gemm(x, w, bias, residual=res, tile=tile)), "stats= changed the output"
        worst = max(worst, W.check_records(rec, W.record_values(y), f"conv_gemm tile {tile} {dt} {(M, Cin, Cout)}: records"))
        n += 1
    assert n >= 2
    print(f"\nRATIO records conv_gemm {dt} tile{tile}: {worst:.3f} ({n} shapes)")


# --------------------------------------------------------------------------- bilinear_concat, bilinear_concat_rows
@pytest.mark.parametrize("case", W.BILINEAR_CASES, ids=str)
def test_bilinear_concat_elementwise(ops, case):
    N, C, Hh, Ww, h, w = case
    x, low = _cu(*W.bilinear_inputs(*case))
    ref, bound = W.bilinear_ref(low, Hh, Ww)
    flat = lambda t: t.reshape(-1, Ww)
    out = _nan(N, 2 * C, Hh, Ww)
    ops.bilinear_concat(x, low, out)
    assert torch.equal(out[:, :C], x), "bilinear_concat: the x half is a copy"
    worst = E.check(flat(out[:, C:]), flat(ref), flat(bound), what=f"bilinear_concat {case}")
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(N * Hh * Ww, -1)
    wr = {}
    for dt, Cpad in (("f32", 2 * C + 2), ("bf16", 8)):
        o = torch.full((N * Hh * Ww, Cpad), float("nan"), dtype=DT[dt], device="cuda")
        ops.bilinear_concat_rows(x, low, o)
        assert torch.equal(o[:, :C], rows(x).to(DT[dt])), f"bilinear_concat_rows {dt}: the x half is x rounded once"
        assert bool((o[:, 2 * C:] == 0).all()), f"bilinear_concat_rows {dt}: the pad columns are zero"
        r, e = rows(ref), rows(bound)
        wr[dt] = E.check(o[:, C:2 * C], r, W._store(r, e, DT[dt]), what=f"bilinear_concat_rows {dt} {case}")
    print(f"\nRATIO bilinear f32 {case}: api {worst:.3f} rows-f32 {wr['f32']:.3f} rows-bf16 {wr['bf16']:.3f}")


# --------------------------------------------------------------------------- chain: producer -> records -> gn_finalize_stats
@pytest.mark.parametrize("case", W.CHAIN_CASES, ids=lambda c: f"{c[0]}-mean{c[5]}")
def test_chain_producer_records_finalize(ops, case):
    prod, M, Cin, C, S, m = case
    x, w, bias, res, gamma, beta, film = _cu(*W.chain_inputs(M, Cin, C, S, m))
    rec = _nan(M // 64, C // 4, 2)
    if prod.startswith("tile"):
        y = ops.conv_gemm(x, w, bias, residual=res, tile=int(prod[4:]), stats=rec)
    elif prod == "gn_conv1x1":
        geom = ops.Geom.per_sample(S, M // S)
        gg = torch.Generator().manual_seed(5)
        ga, gb = (1 + 0.1 * torch.randn(S, Cin, generator=gg)).cuda(), (0.1 * torch.randn(S, Cin, generator=gg)).cuda()
        y = ops.gn_conv1x1(x, ga, gb, geom, True, w, bias, residual=res, tile=128, stats=rec)
    else:                                                    # resample with stats=: a 2 x 2 pool of rows that carry the mean
        xin = (x.float() * 2 + m).to(BF)                     # x [M, C] here: NF = 2 S frames of 8 x 16 rows -> M / 4 output rows of unit variance
        rec = _nan(M // 4 // 64, C // 4, 2)
        y = torch.full((M // 4, C), float("nan"), dtype=BF, device="cuda")
        ops.resample(xin, y, 2 * S, 8, M // (16 * S), 2, 2, 0, 1.0, stats=rec)
    assert torch.isfinite(y.float()).all()
    wrec = W.check_records(rec, W.record_values(y), f"chain {prod}: records")
    r = W.chain_ref(y, gamma, beta, film, S)
    ratio = float((r["mean"] * r["rstd"]).abs().median())
    assert 0.6 * m < ratio < 1.6 * m, (ratio, m)             # the stored output has the stated mean / std
    a, b, mr = _nan(S, C), _nan(S, C), _nan(S, 32, 2)
    ops.gn_finalize_stats(rec, gamma, beta, ops.Geom.per_sample(S, y.shape[0] // S), film=film, a=a, b=b, mr=mr)
    what = f"chain {prod} mean {m}"
    worst = max(E.check(a, r["a"], r["e_a"], what=what + ": a"), E.check(b, r["b"], r["e_b"], what=what + ": b"),
                E.check(mr[..., 0], r["mean"], r["e_mean"], what=what + ": mean"), E.check(mr[..., 1], r["rstd"], r["e_rstd"], what=what + ": rstd"))
    print(f"\nRATIO chain f32 {prod} mean {m}: records {wrec:.3f} affine {worst:.3f}")
