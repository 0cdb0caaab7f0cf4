"""ResBlock out conv with its 1x1 skip conv in ONE launch (mmd_gn_conv1x1_skip, mmd_gemm.hip: conv1x1_strip_skip_kernel) against the
launches it replaces, through the C-ABI: conv_gemm(x, W_skip, b_skip) -> sk, then the out conv of the normalised h with sk as residual.

The fused launch keeps the skip product in its own accumulator, rounds it to bf16 with its bias where sk would have been stored and
adds it where the residual is added, so every comparison here is an EQUALITY (torch.equal on Y and on the statistics records).  No
new fp64 bound is needed: both constituents are already bounded element by element (tests/test_elementwise_fwd_*), and equality
carries those bounds over to the fused launch.

Records: the fused launch folds a record the way the one-fragment K = 128 strip instance does, which is what the out conv of a
layer with slices of >= 16384 rows runs today - the only layers the engine fuses (ops.skip_fusable).  With shorter slices today's
out conv runs the two-fragment instance, whose fold differs in the last bit, so for the small geometries the record reference is
the same rows run through the two launches as the head of one 16384-row slice (a record depends on its own 64 rows and the slice's
affine only); Y is compared against the two launches at the geometry itself as well."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mm_diffusion import _hip as H
from mm_diffusion import ops as _ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(_ops._STRIP_MODE != "pin", reason="the row-strip kernel is switched off (MMD_GEMM_STRIP)")]
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RF1_ROWS = 16384      # slices of at least this many rows run the one-fragment instance (mmd_gemm.hip: dispatch_conv1x1_strip)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _ops


def _operands(M, S, K1, K2, Cout, seed, ldh=None, ldx=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    hw = (torch.randn(M, ldh or K1, device="cuda", generator=g) * 1.4 + 0.3).to(BF)      # SiLU sees both signs
    xw = (torch.randn(M, ldx or K2, device="cuda", generator=g) * 1.2 - 0.2).to(BF)
    h = hw[:, (hw.shape[1] - K1) // 16 * 8:][:, :K1]
    x = xw[:, (xw.shape[1] - K2) // 16 * 8:][:, :K2]
    w = (torch.randn(Cout, K1, device="cuda", generator=g) * K1 ** -0.5).to(BF)
    ws = (torch.randn(Cout, K2, device="cuda", generator=g) * K2 ** -0.5).to(BF)
    b, bs = torch.randn(Cout, device="cuda", generator=g), torch.randn(Cout, device="cuda", generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(K1, device="cuda", generator=g), torch.randn(K1, device="cuda", generator=g)
    film = torch.randn(S, 2 * K1, device="cuda", generator=g) * 0.3
    geom = _ops.Geom.per_sample(S, M // S)
    ga, gb = _ops.gn_stats(h, gamma, beta, geom, film=film)
    return h, x, w, ws, b, bs, ga, gb, geom


def _two_launches(ops, h, x, w, ws, b, bs, ga, gb, geom, act, stats=None, out=None):
    """Today's path: the skip conv, then the out conv with the skip tensor as residual - norm fused where the strip kernel takes the
    slices, applied first otherwise (what the engine does)."""
    sk = ops.conv_gemm(x, ws, bs)
    if ops.strip_tile_ok(h, w.shape[0], stats=stats, geom=geom):
        return ops.gn_conv1x1(h, ga, gb, geom, act, w, b, residual=sk, tile=131, stats=stats, out=out)
    return ops.conv_gemm(ops.gn_apply(h, ga, gb, geom, act=act), w, b, residual=sk, stats=stats, out=out)


def _rf1_records(ops, h, x, w, ws, b, bs, ga, gb, geom, act, y):
    """The records of the two-launch path in the one-fragment fold: every slice as the head of one RF1_ROWS-row slice with the slice's
    affine.  Also checks that those launches store the same Y rows."""
    M, Cout = h.shape[0], w.shape[0]
    if geom.Tn >= RF1_ROWS:
        rec = torch.full((M // 64, Cout // 4, 2), float("nan"), device="cuda")
        assert torch.equal(_two_launches(ops, h, x, w, ws, b, bs, ga, gb, geom, act, stats=rec), y)
        return rec
    assert geom.Tn % 64 == 0
    recs, g1 = [], ops.Geom.per_sample(1, RF1_ROWS)
    for s in range(geom.S):
        hp, xp = torch.zeros(RF1_ROWS, h.shape[1], device="cuda", dtype=BF), torch.zeros(RF1_ROWS, x.shape[1], device="cuda", dtype=BF)
        hp[:geom.Tn], xp[:geom.Tn] = h[s * geom.Tn:(s + 1) * geom.Tn], x[s * geom.Tn:(s + 1) * geom.Tn]
        rec = torch.full((RF1_ROWS // 64, Cout // 4, 2), float("nan"), device="cuda")
        yp = _two_launches(ops, hp, xp, w, ws, b, bs, ga[s:s + 1].contiguous(), gb[s:s + 1].contiguous(), g1, act, stats=rec)
        assert torch.equal(yp[:geom.Tn], y[s * geom.Tn:(s + 1) * geom.Tn])
        recs.append(rec[:geom.Tn // 64])
    return torch.cat(recs)


GEOMS = [(128, 1),        # one block, deepest column split
         (384, 3),        # three slices of 128 rows, one per strip
         (640, 2),        # slices of 320 rows: the middle strip spans two slices
         (330, 1),        # rows past M in the last block
         (40000, 1)]      # more than 256 row blocks: no column split; a slice the engine's rule accepts


@pytest.mark.parametrize("K2", [256, 384])
@pytest.mark.parametrize("Cout", [128, 256])
@pytest.mark.parametrize("M,S", GEOMS)
def test_fused_launch_is_bitwise_the_two_launches(ops, M, S, K2, Cout):
    """act on / off x statistics on / off x biases present / absent at every row geometry, K2 and Cout: Y and the records."""
    K1 = 128
    h, x, w, ws, b, bs, ga, gb, geom = _operands(M, S, K1, K2, Cout, M + K2 + Cout)
    for act, with_bias in itertools.product((True, False), (True, False)):
        bo, bk = (b, bs) if with_bias else (None, None)
        y_ref = _two_launches(ops, h, x, w, ws, bo, bk, ga, gb, geom, act)
        y = torch.full((M, Cout), float("nan"), device="cuda", dtype=BF)
        ops.gn_conv1x1_skip(h, ga, gb, geom, act, w, bo, x, ws, bk, out=y)
        assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16)), (act, with_bias)
        if M % 64:
            continue                                   # (records are whole 64-row groups)
        rec = torch.full((M // 64, Cout // 4, 2), float("nan"), device="cuda")
        y2 = torch.full((M, Cout), float("nan"), device="cuda", dtype=BF)
        ops.gn_conv1x1_skip(h, ga, gb, geom, act, w, bo, x, ws, bk, out=y2, stats=rec)
        assert torch.equal(y2.view(torch.int16), y_ref.view(torch.int16)), (act, with_bias, "with records")
        rec_ref = _rf1_records(ops, h, x, w, ws, bo, bk, ga, gb, geom, act, y_ref)
        assert torch.equal(rec.view(torch.int32), rec_ref.view(torch.int32)), (act, with_bias, "records")


@pytest.mark.parametrize("K2", [256, 384])
def test_fused_launch_on_strided_views(ops, K2):
    """x as a column view of a wider buffer (the concat buffers), h with a row stride above K1, Y and its records as column views with
    guard columns on both sides, which stay untouched."""
    M, S, K1, Cout = 640, 2, 128, 128
    h, x, w, ws, b, bs, ga, gb, geom = _operands(M, S, K1, K2, Cout, 11 + K2, ldh=K1 + 64, ldx=K2 + 128)
    assert h.stride(0) > K1 and x.stride(0) > K2 and x.data_ptr() != x.untyped_storage().data_ptr()
    y_ref = _two_launches(ops, h, x, w, ws, b, bs, ga, gb, geom, True)
    yw = torch.full((M, Cout + 48), 3.0, device="cuda", dtype=BF)
    recw = torch.full((M // 64, Cout // 4 + 10, 2), 7.0, device="cuda")
    ops.gn_conv1x1_skip(h, ga, gb, geom, True, w, b, x, ws, bs, out=yw[:, 16:16 + Cout], stats=recw[:, 6:6 + Cout // 4, :])
    assert torch.equal(yw[:, 16:16 + Cout], y_ref)
    assert float((yw[:, :16].float() - 3).abs().max()) == 0 and float((yw[:, 16 + Cout:].float() - 3).abs().max()) == 0
    rec_ref = _rf1_records(ops, h.contiguous(), x.contiguous(), w, ws, b, bs, ga, gb, geom, True, y_ref)
    assert torch.equal(recw[:, 6:6 + Cout // 4, :], rec_ref)
    assert float((recw[:, :6] - 7).abs().max()) == 0 and float((recw[:, 6 + Cout // 4:] - 7).abs().max()) == 0


@pytest.mark.parametrize("K2,Cout", [(512, 128), (256, 144)])
def test_unsupported_shapes_are_refused_without_a_launch(ops, K2, Cout):
    """K1 + K2 = 640 (beyond the operand registers of a strip) and Cout % 32 != 0: the library's error, nothing written."""
    M, K1 = 256, 128
    g = torch.Generator(device="cuda").manual_seed(3)
    h, x = torch.randn(M, K1, device="cuda", generator=g).to(BF), torch.randn(M, K2, device="cuda", generator=g).to(BF)
    w, ws = torch.zeros(Cout, K1, device="cuda", dtype=BF), torch.zeros(Cout, K2, device="cuda", dtype=BF)
    ga, gb = torch.ones(1, K1, device="cuda"), torch.zeros(1, K1, device="cuda")
    y = torch.full((M, Cout), float("nan"), device="cuda", dtype=BF)
    with pytest.raises(H.MMDError, match="gn_conv1x1_skip"):
        ops.gn_conv1x1_skip(h, ga, gb, ops.Geom.per_sample(1, M), True, w, None, x, ws, None, out=y)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


def test_skip_fusable_follows_the_layer_geometry(ops):
    """The rule on the model's layer shapes (device tensors: alignment is part of it)."""
    def t(rows, C, ld=None, off=0):
        return torch.empty(rows, ld or C, device="cuda", dtype=BF)[:, off:off + C]
    N = 2
    gv, ga = ops.Geom.per_sample(N, 65536), ops.Geom.per_sample(N, 25600)
    assert ops.skip_fusable(t(N * 65536, 128), t(N * 65536, 384, 384 + 128, 128), 128, gv, stats=True)     # ds1 video, x a concat view
    assert ops.skip_fusable(t(N * 25600, 128), t(N * 25600, 256), 128, ga)                                   # ds1 audio
    assert not ops.skip_fusable(t(N * 25600, 128), t(N * 25600, 512), 128, ga)                               # K1 + K2 = 640
    assert not ops.skip_fusable(t(N * 16384, 256), t(N * 16384, 128), 256, ops.Geom.per_sample(N, 16384))    # ds2: K1 = 256
    assert not ops.skip_fusable(t(N * 4096, 128), t(N * 4096, 256), 128, ops.Geom.per_sample(N, 4096))       # short slices: the two-fragment fold
    assert not ops.skip_fusable(t(N * 25600, 128), t(N * 25600, 256, 256 + 8, 4), 128, ga)                   # x not 16-byte aligned
    assert not ops.skip_fusable(t(N * 25600, 128).float(), t(N * 25600, 256).float(), 128, ga)               # fp32 mode


# --------------------------------------------------------------------------- engine: same model, fused tail on / off
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
f = flags("full", use_fp16=True)
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


def _engine_arm(tmp_path, fuse):
    out = str(tmp_path / f"fuse{fuse}.npz")
    r = subprocess.run([sys.executable, "-c", _ENGINE_SCRIPT.format(root=ROOT, out=out)], env=dict(os.environ, MMD_SKIP_FUSE=fuse),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


def test_engine_fuses_the_ds1_tails_and_computes_the_same_bits(tmp_path):
    """The base model (the smallest shipped configuration with a channel-changing block at >= 16384 rows per sample: its ds1 level), one
    sample, bf16: with the fused tails the plan has one launch fewer per fused block - its skip conv is gone, its out conv carries the
    fused label - and the outputs are bitwise those of the two-launch plan (MMD_SKIP_FUSE=0)."""
    import re
    from collections import Counter
    on, off = _engine_arm(tmp_path, "1"), _engine_arm(tmp_path, "0")
    assert np.array_equal(on["vo"], off["vo"]) and np.array_equal(on["ao"], off["ao"])
    n_on, n_off = Counter(on["names"].tolist()), Counter(off["names"].tolist())
    l_on, l_off = Counter(on["labels"].tolist()), Counter(off["labels"].tolist())
    fused = n_on["mmd_gn_conv1x1_skip"]
    print("fused tails:", {k: v for k, v in l_on.items() if k.startswith("gn_conv1x1_skip")}, "launches", len(on["names"]), "was", len(off["names"]))
    assert fused > 0 and n_off["mmd_gn_conv1x1_skip"] == 0
    assert len(on["names"]) == len(off["names"]) - fused
    assert n_on["mmd_conv_gemm"] + n_on["mmd_conv_gemm_stats"] == n_off["mmd_conv_gemm"] + n_off["mmd_conv_gemm_stats"] - fused
    assert n_on["mmd_gn_conv1x1"] + n_on["mmd_gn_conv1x1_stats"] == n_off["mmd_gn_conv1x1"] + n_off["mmd_gn_conv1x1_stats"] - fused
    for label, n in l_on.items():
        m = re.fullmatch(r"gn_conv1x1_skip<bf16,strip>\[M=(\d+),K=128\+(\d+),N=(\d+)\]", label)
        if m:         # the block's skip conv and its out conv with a residual left the plan
            skip = f"conv_gemm<bf16,strip>[M={m.group(1)},K={m.group(2)},N={m.group(3)}]"
            assert l_off[skip] - l_on[skip] == n, (label, l_off[skip], l_on[skip])
            assert int(m.group(1)) >= 16384
