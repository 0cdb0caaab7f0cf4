"""The streamed ResBlock tail (mmd_res_tail, mmd_rtail.hip) against the launches it replaces, through the C-ABI: conv_gemm(x, W2, b2)
-> sk, then the out conv of the normalised h with sk as residual - the norm fused into the row-strip GEMM where that kernel takes the
slices, gn_apply + the strip GEMM otherwise (what the engine does; the two are bitwise equal paths).

The fused launch keeps the skip product in its own accumulator, rounds it to bf16 with its bias where sk would have been stored and
adds it where the residual is added; its records are folded in the order of the strip instance the out conv runs (two row fragments
per wave at K1 <= 256 with these short samples - reproduced across a wave pair -, one at K1 >= 384).  So every comparison is an EQUALITY on the int16 / int32 views of
Y and of the records, in both norm modes (affine in the launch / null affine behind gn_apply).  One case also meets a float64
reference element by element (tests/errbound.py), so that the chain of equalities hangs on something that is not a libmmd GEMM.

The shapes are the smallest at which the kernel can still go wrong: 192-row samples make a 128-row block straddle two samples, K2 = 640 is no multiple of 128, Cout = 384 gives three column ranges, M = 400 leaves 16 rows in the last block."""
import os
import re
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest
import torch

import errbound as E
from mm_diffusion import _hip as H
from mm_diffusion import ops as _ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (samples, rows per sample, K1, K2, Cout, records)
CASES = [(2, 192, 256, 128, 256, True),       # a block straddles two samples; two-fragment record order; the shortest skip operand
         (2, 192, 384, 640, 384, True),       # one-fragment record order; K2 no multiple of 128; three column ranges
         (2, 192, 512, 1024, 512, True),      # longest K; deepest column split
         (2, 200, 512, 896, 512, False),      # ragged last block: M = 400, 16 rows in it
         (2, 192, 128, 512, 128, True),       # the audio ds1 block the strip refuses (K1 + K2 = 640)
         # the launch picks its instance by size: the rows above run 64-column workgroups with 128-channel K steps wherever K1 and K2
         # allow (one row fragment) - these two reach the other instances
         (2, 192, 384, 192, 384, True),       # K2 no multiple of 128: 64-channel K steps
         (4, 2112, 512, 64, 512, True),       # 66 row blocks x 4 column ranges >= 192 workgroups: 128-column workgroups; shortest K2
         (4, 3136, 256, 64, 256, True)]       # 98 x 2: 128-column workgroups with the two-fragment record order


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _ops


def _operands(S, L, K1, K2, Cout, seed, ldx=None):
    """h, x (the right-hand columns of a buffer of ldx columns), both weights and biases, the fused affine of h's norm (with FiLM)."""
    M = S * L
    g = torch.Generator(device="cuda").manual_seed(seed)
    h = (torch.randn(M, K1, device="cuda", generator=g) * 1.4 + 0.3).to(BF)      # SiLU sees both signs
    xw = (torch.randn(M, ldx or K2, device="cuda", generator=g) * 1.2 - 0.2).to(BF)
    x = xw[:, xw.shape[1] - K2:]
    w = (torch.randn(Cout, K1, device="cuda", generator=g) * K1 ** -0.5).to(BF)
    ws = (torch.randn(Cout, K2, device="cuda", generator=g) * K2 ** -0.5).to(BF)
    b, bs = torch.randn(Cout, device="cuda", generator=g), torch.randn(Cout, device="cuda", generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(K1, device="cuda", generator=g), torch.randn(K1, device="cuda", generator=g)
    film = torch.randn(S, 2 * K1, device="cuda", generator=g) * 0.3
    geom = _ops.Geom.per_sample(S, L)
    ga, gb = _ops.gn_stats(h, gamma, beta, geom, film=film)
    return h, x, w, ws, b, bs, ga, gb, geom


def _two_launches(ops, h, x, w, ws, b, bs, ga, gb, geom, stats=None, out=None):
    """Today's path: the skip conv, then the out conv with the skip tensor as residual - norm fused where the strip kernel takes the
    slices, applied first otherwise."""
    sk = ops.conv_gemm(x, ws, bs)
    if ops.strip_tile_ok(h, w.shape[0], stats=stats, geom=geom):
        return ops.gn_conv1x1(h, ga, gb, geom, True, w, b, residual=sk, tile=131, stats=stats, out=out)
    return ops.conv_gemm(ops.gn_apply(h, ga, gb, geom, act=True), w, b, residual=sk, tile=131, stats=stats, out=out)


_REF = {}


def _case(ops, case):
    """Operands and the two-launch reference (Y, records) of a table row: computed once, shared, never written again."""
    if case not in _REF:
        S, L, K1, K2, Cout, records = case
        opnd = _operands(S, L, K1, K2, Cout, 7 * K1 + K2 + L)
        rec = torch.full((S * L // 64, Cout // 4, 2), float("nan"), device="cuda") if records else None
        y = _two_launches(ops, *opnd, stats=rec)
        torch.cuda.synchronize()
        _REF[case] = (opnd, y, rec)
    return _REF[case]


def _same_bits(a, b):
    view = torch.int16 if a.dtype == BF else torch.int32
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%dx%d-K%d+%d-N%d" % c[:5])
@pytest.mark.parametrize("mode", ["affine", "prenormalised"])
def test_streamed_tail_is_bitwise_the_two_launches(ops, case, mode):
    S, L, K1, K2, Cout, records = case
    (h, x, w, ws, b, bs, ga, gb, geom), y_ref, rec_ref = _case(ops, case)
    M = S * L
    hin, a_, b_ = (h, ga, gb) if mode == "affine" else (ops.gn_apply(h, ga, gb, geom, act=True), None, None)
    ybuf = torch.full((M + 128, Cout), float("nan"), device="cuda", dtype=BF)      # 128 guard rows behind the last block
    rec = torch.full((M // 64, Cout // 4, 2), float("nan"), device="cuda") if records else None
    assert ops.res_tail_ok(hin, x, Cout, geom, rec, ybuf[:M])
    ops.res_tail(hin, a_, b_, geom, True, w, b, x, ws, bs, out=ybuf[:M], stats=rec)
    assert _same_bits(ybuf[:M], y_ref), "Y"
    assert bool(torch.isnan(ybuf[M:]).all()), "rows past M written"
    if records:
        assert _same_bits(rec, rec_ref), "records"
        # without records: the same Y
        y2 = torch.full((M, Cout), float("nan"), device="cuda", dtype=BF)
        ops.res_tail(hin, a_, b_, geom, True, w, b, x, ws, bs, out=y2)
        assert _same_bits(y2, y_ref), "Y without records"


def test_streamed_tail_follows_the_fold_of_long_samples(ops):
    """K1 = 128 with samples of >= 16384 rows is where the out conv's record fold depends on the norm mode: with the norm fused the
    strip GEMM holds one row fragment per wave (half records through LDS), behind gn_apply two (one running sum over rows r, r + 32).
    The streamed launch follows each: with the affine given it meets the norm-fused strip GEMM, with a null affine the plain one behind
    gn_apply - Y and records bit for bit.  The smallest such launch: one sample, K2 = Cout = 64 (64-column workgroups, 64-channel K steps)."""
    S, L, K1, K2, Cout = 1, 16384, 128, 64, 64
    h, x, w, ws, b, bs, ga, gb, geom = _operands(S, L, K1, K2, Cout, 11)
    M = S * L
    rec_ref = torch.full((M // 64, Cout // 4, 2), float("nan"), device="cuda")
    assert ops.strip_tile_ok(h, Cout, stats=rec_ref, geom=geom)
    y_ref = _two_launches(ops, h, x, w, ws, b, bs, ga, gb, geom, stats=rec_ref)      # the norm inside the strip GEMM
    rec = torch.full_like(rec_ref, float("nan"))
    assert ops.res_tail_ok(h, x, Cout, geom, rec)
    y = ops.res_tail(h, ga, gb, geom, True, w, b, x, ws, bs, stats=rec)
    assert _same_bits(y, y_ref), "Y, affine"
    assert _same_bits(rec, rec_ref), "records, affine"
    hn = ops.gn_apply(h, ga, gb, geom, act=True)
    rec_ref2 = torch.full_like(rec_ref, float("nan"))
    y_ref2 = ops.conv_gemm(hn, w, b, residual=ops.conv_gemm(x, ws, bs), tile=131, stats=rec_ref2)
    rec2 = torch.full_like(rec_ref, float("nan"))
    y2 = ops.res_tail(hn, None, None, geom, True, w, b, x, ws, bs, stats=rec2)
    assert _same_bits(y2, y_ref2), "Y, prenormalised"
    assert _same_bits(rec2, rec_ref2), "records, prenormalised"
    assert _same_bits(y2, y_ref), "the two norm modes store the same Y"


def test_streamed_tail_without_biases_and_without_silu(ops):
    """Null biases and act = 0 take their own paths in the prologue and the norm."""
    S, L, K1, K2, Cout = 2, 192, 384, 640, 384
    h, x, w, ws, b, bs, ga, gb, geom = _operands(S, L, K1, K2, Cout, 5)
    sk = ops.conv_gemm(x, ws, None)
    rec_ref = torch.full((S * L // 64, Cout // 4, 2), float("nan"), device="cuda")
    y_ref = ops.conv_gemm(ops.gn_apply(h, ga, gb, geom, act=False), w, None, residual=sk, tile=131, stats=rec_ref)
    rec = torch.full_like(rec_ref, float("nan"))
    y = ops.res_tail(h, ga, gb, geom, False, w, None, x, ws, None, stats=rec)
    assert _same_bits(y, y_ref) and _same_bits(rec, rec_ref)


def test_streamed_tail_on_strided_views(ops):
    """x the right-hand column view of a wider concat buffer, Y a column slice of a wider buffer, the records at a quad offset; the
    columns on both sides stay untouched."""
    S, L, K1, K2, Cout = 2, 192, 384, 640, 384
    h, x, w, ws, b, bs, ga, gb, geom = _operands(S, L, K1, K2, Cout, 23, ldx=K2 + 256)
    M = S * L
    assert x.stride(0) == K2 + 256 and x.data_ptr() != x.untyped_storage().data_ptr()
    rec_ref = torch.full((M // 64, Cout // 4, 2), float("nan"), device="cuda")
    y_ref = _two_launches(ops, h, x, w, ws, b, bs, ga, gb, geom, stats=rec_ref)
    yw = torch.full((M, Cout + 48), 3.0, device="cuda", dtype=BF)
    recw = torch.full((M // 64, Cout // 4 + 10, 2), 7.0, device="cuda")
    ysl, rsl = yw[:, 16:16 + Cout], recw[:, 6:6 + Cout // 4, :]
    assert ops.res_tail_ok(h, x, Cout, geom, rsl, ysl)
    ops.res_tail(h, ga, gb, geom, True, w, b, x, ws, bs, out=ysl, stats=rsl)
    assert _same_bits(ysl, y_ref) and _same_bits(rsl, rec_ref)
    assert float((yw[:, :16].float() - 3).abs().max()) == 0 and float((yw[:, 16 + Cout:].float() - 3).abs().max()) == 0
    assert float((recw[:, :6] - 7).abs().max()) == 0 and float((recw[:, 6 + Cout // 4:] - 7).abs().max()) == 0


def test_streamed_tail_meets_float64_element_by_element(ops):
    """Not a self-comparison: the first table row against torch double ops on the stored bf16 operands.

    y = rn16(acc1 + r) with r = rn16(acc2) the bf16-rounded skip product.  acc2 is a GEMM of depth K2 with a bias: r lies within
    b_sk = gemm_bound(sk64, S2, K2, bf16) of sk64 = W2 x + b2 in float64.  acc1 + r is a GEMM of depth K1 with a bias and a residual
    (errbound.py), so against ref = W g(h) + b + sk64 (g(h): gn_apply's stored output, the operand the kernel feeds bit for bit)
        |y - ref| <= gemm_bound(ref, S1, K1, bf16) + (1 + v) b_sk,   S1 = sum |g(h)| |W| + |b| + |sk64| + b_sk
    - the residual the kernel adds is r, not sk64: its distance b_sk enters once directly, once through the output rounding, and
    its magnitude |r| <= |sk64| + b_sk enters the fp32 accumulation term."""
    case = CASES[0]
    S, L, K1, K2, Cout, _ = case
    (h, x, w, ws, b, bs, ga, gb, geom), _, _ = _case(ops, case)
    y = torch.full((S * L, Cout), float("nan"), device="cuda", dtype=BF)
    ops.res_tail(h, ga, gb, geom, True, w, b, x, ws, bs, out=y)
    sk64, S2 = E.conv_rows_ref(x, ws, bs, None, E.TAPS_1, (1, 1, 1))
    b_sk = E.gemm_bound(sk64, S2, K2, BF)
    hn = ops.gn_apply(h, ga, gb, geom, act=True)
    ref, S1 = E.conv_rows_ref(hn, w, b, sk64, E.TAPS_1, (1, 1, 1))
    bound = E.gemm_bound(ref, S1 + b_sk, K1, BF) + (1 + E.U16) * b_sk
    ratio = E.check(y, ref, bound, what="res_tail 2x192 K=256+128 N=256")
    print(f"\nRATIO res_tail 2x192x(256+128)x256 bf16: {ratio:.3f}")


@pytest.mark.parametrize("K1,K2,Cout", [(384, 1088, 384), (320, 640, 320), (384, 640, 416)])
def test_unsupported_shapes_are_refused_without_a_launch(ops, K1, K2, Cout):
    """K2 beyond 1024, a K1 without an instance, Cout % 64 != 0: the library's error, nothing written."""
    M = 256
    g = torch.Generator(device="cuda").manual_seed(3)
    h, x = torch.randn(M, K1, device="cuda", generator=g).to(BF), torch.randn(M, K2, device="cuda", generator=g).to(BF)
    w, ws = torch.zeros(Cout, K1, device="cuda", dtype=BF), torch.zeros(Cout, K2, device="cuda", dtype=BF)
    ga, gb = torch.ones(1, K1, device="cuda"), torch.zeros(1, K1, device="cuda")
    y = torch.full((M, Cout), float("nan"), device="cuda", dtype=BF)
    assert not ops.res_tail_ok(h, x, Cout, ops.Geom.per_sample(1, M), None, y)
    with pytest.raises(H.MMDError, match="res_tail"):
        ops.res_tail(h, ga, gb, ops.Geom.per_sample(1, M), True, w, None, x, ws, None, out=y)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


def test_overlapping_output_is_refused(ops):
    """Y inside the buffer x lives in: the column ranges of a row block would read rows the others write."""
    M, K1, K2, Cout = 256, 384, 640, 384
    buf = torch.full((M, 1024), float("nan"), device="cuda", dtype=BF)
    h = torch.zeros(M, K1, device="cuda", dtype=BF)
    w, ws = torch.zeros(Cout, K1, device="cuda", dtype=BF), torch.zeros(Cout, K2, device="cuda", dtype=BF)
    geom = ops.Geom.per_sample(1, M)
    assert not ops.res_tail_ok(h, buf[:, 384:], Cout, geom, None, buf[:, :384])
    with pytest.raises(H.MMDError, match="overlap"):
        ops.res_tail(h, None, None, geom, True, w, None, buf[:, 384:], ws, None, out=buf[:, :384])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# --------------------------------------------------------------------------- engine: same model, streamed tails on / off
# (the switch is read at import, so each arm is its own interpreter)
_ENGINE_SCRIPT = r"""
import os, sys
for p in ({root!r}, os.path.join({root!r}, "mm-diffusion_amd"), os.path.join({root!r}, "tests")):
    sys.path.insert(0, p)
import numpy as np, torch
from helpers import flags, inputs
from mm_diffusion import multimodal_script_util as msu, logger
from mm_diffusion.synth import synth_init_
logger.set_quiet(True)
# (channel_mult spelled out: the script utility's table of defaults knows frame sides from 64 up; "1,2,3,4" is the base model's entry)
f = flags("full", use_fp16=True, video_size=[16, 3, 32, 32], audio_size=[1, 6400], num_res_blocks=1, channel_mult="1,2,3,4")
model, _ = msu.create_model_and_diffusion(**f)
synth_init_(model)
model.cuda().eval()
video, audio = inputs(f, 1, 17)
import random
random.seed(17)                # the window shifts come from the global generator: both arms must draw the same ones
shifts = model.draw_shifts()
it = iter(shifts)
model.shift_source = lambda lo, hi: next(it)
with torch.no_grad():
    vo, ao = model(video.cuda(), audio.cuda(), torch.tensor([417]).cuda())
eng = next(iter(model._engines.values()))
launches = [e for e in eng.plan if e[0] is not None]
np.savez({out!r}, vo=vo.float().cpu().numpy(), ao=ao.float().cpu().numpy(), names=np.array([e[2] for e in launches]),
         labels=np.array([e[3][0] for e in launches]))
"""


def _engine_arm(tmp_path, stream):
    out = str(tmp_path / f"stream{stream}.npz")
    r = subprocess.run([sys.executable, "-c", _ENGINE_SCRIPT.format(root=ROOT, out=out)], env=dict(os.environ, MMD_TAIL_STREAM=stream),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


def test_engine_streams_the_deep_tails_and_computes_the_same_bits(tmp_path):
    """The base model on 32 x 32 frames and 6400 audio positions with one ResBlock per level (the smallest shipped-shape model whose
    deep levels still route to the new launch), one sample, bf16: with the streamed tails the plan is shorter by one launch per fused
    block - its skip conv is gone - plus the gn_apply launches the in-kernel norm replaced, and the outputs are bitwise those of the
    two-launch plan (MMD_TAIL_STREAM=0)."""
    on, off = _engine_arm(tmp_path, "1"), _engine_arm(tmp_path, "0")
    assert np.array_equal(on["vo"], off["vo"]) and np.array_equal(on["ao"], off["ao"])
    n_on, n_off = Counter(on["names"].tolist()), Counter(off["names"].tolist())
    l_on, l_off = Counter(on["labels"].tolist()), Counter(off["labels"].tolist())
    fused = n_on["mmd_res_tail"]
    applies = n_off["mmd_gn_apply"] - n_on["mmd_gn_apply"]
    print("streamed tails:", {k: v for k, v in l_on.items() if k.startswith("res_tail")}, "gn_apply removed:", applies,
          "launches", len(on["names"]), "was", len(off["names"]))
    assert fused > 0 and n_off["mmd_res_tail"] == 0 and applies >= 0
    assert len(on["names"]) == len(off["names"]) - fused - applies
    assert n_on["mmd_gn_conv1x1_skip"] == n_off["mmd_gn_conv1x1_skip"] > 0        # the ds1 strip fusion is untouched
    seen = 0
    for label, n in l_on.items():
        m = re.fullmatch(r"res_tail<bf16,stream>\[M=(\d+),K=(\d+)\+(\d+),N=(\d+)\]", label)
        if m:         # the block's skip conv left the plan (whatever tile it ran on)
            skip = re.compile(r"conv_gemm<bf16,[^>]*>\[M=%s,K=%s,N=%s\]" % (m.group(1), m.group(3), m.group(4)))
            was = sum(c for k, c in l_off.items() if skip.fullmatch(k))
            now = sum(c for k, c in l_on.items() if skip.fullmatch(k))
            assert was - now == n, (label, was, now)
            seen += n
    assert seen == fused
