"""The fused VideoConv (mmd_vconv2d1d) and the fused temporal-attention block (mmd_tattn_block) against staged float64 references,
ELEMENT BY ELEMENT (tests/errbound_fused.py: the references, the propagated bounds and their derivation;
tests/test_errbound_fused_cpu.py: the metric proven on seeded defects, on exactly these cases).

Every case builds its reference with torch double ops on the stored operands - never with a libmmd kernel -, prefills the output with
NaN and admits ZERO elements outside the per-element bound.  The cases are the smallest at which each mechanism of the kernels is
exercised (errbound_fused.VCONV_CASES / TATTN_CASES say which); the strided cases also hold the guard columns of the output buffer
bitwise untouched.

Worst error / bound ratio per group, as printed by the tests (`-s`) on an MI355X (`cases` = launches in the group):

    kernel        group                                   cases  worst ratio
    vconv2d1d     plain conv (no input norm)                  6        0.807
    vconv2d1d     input affine                                6        0.790
    vconv2d1d     input affine + SiLU                         6        0.803
    tattn_block   1x8, 3x8, 1x40, 2x24                        4        0.147
    tattn_block   spike (q, k x 3)                            1        0.018
    tattn_block   offset (residual 32 x the branch)           1        0.627
    tattn_block   strided views                               1        0.146

Every case: zero violating elements, 2 s for the module.  The VideoConv maxima (0.79 - 0.81) are the single-chunk case 1x4x4-c32, where
the output-rounding term 2**-8 |ref| is half of the bound and some accumulator value lands next to a rounding midpoint; with more
chunks the propagated deviation of T takes a larger share and the worst ratio falls (2x8x12-c160: 0.27 - 0.36).  The attention block sits
at 0.13 - 0.15 because its bound is dominated by the propagated, worst-case deviation of O (errbound_fused.py, HOW SHARP), which the
kernel's actual rounding flips fill to a seventh; on the offset case the store term leads and the ratio is 0.63.  The ratios equal those
of the fp32 CPU emulations of tests/test_errbound_fused_cpu.py to three digits on every case: the element with the worst ratio is one
whose stored value the emulation reproduces bit for bit.  Nothing asserts against these figures; the assertions are the derived bounds.
"""
import functools

import pytest
import torch

import errbound as E
import errbound_fused as Z

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mm_diffusion import ops as o
    return o


def _cuda(t):
    return t.cuda() if isinstance(t, torch.Tensor) else t


def _guarded(t, width, off, fill):
    """t as a column slice [:, off : off + C] of a fresh buffer `width` wide, the rest = fill; returns (buffer, view)."""
    buf = torch.full((t.shape[0], width), fill, dtype=t.dtype, device="cuda")
    view = buf[:, off:off + t.shape[1]]
    view.copy_(t)
    return buf, view


def _untouched(buf, off, C):
    """The guard columns of a NaN-prefilled buffer still hold the prefill's bits."""
    want = torch.full_like(buf, float("nan")).view(torch.int16)
    got = buf.view(torch.int16)
    return torch.equal(got[:, :off], want[:, :off]) and torch.equal(got[:, off + C:], want[:, off + C:])


# --------------------------------------------------------------------------- fused VideoConv
@functools.lru_cache(maxsize=None)
def _vconv_operands(N, Hh, Ww, Cin, S, gn):
    """Operands on the GPU with their reference and bound: the strided case shares them with the plain launch of its geometry."""
    name = next(c[0] for c in Z.VCONV_CASES if c[1:6] == (N, Hh, Ww, Cin, S))
    o = tuple(_cuda(t) for t in Z.vconv_case(name, gn))
    return o, Z.vconv_ref(*o)


VC = [(c, gn) for c in Z.VCONV_CASES for gn in Z.VCONV_GN]


@pytest.mark.parametrize("case,gn", VC, ids=[f"{c[0]}-{gn}" for c, gn in VC])
def test_vconv2d1d_elementwise(ops, case, gn):
    name, N, Hh, Ww, Cin, S, strided = case
    (x, ws, wt, bs, bt, a, b, act, _, _, _), (ref, bound) = _vconv_operands(N, Hh, Ww, Cin, S, gn)
    M = x.shape[0]
    wf = ops.vconv_pack(ws, wt)
    if strided:                                           # ldx = Cin + 40 with the view 16 bytes in; the output 64 bytes into a buffer of 192 columns
        _, x = _guarded(x, Cin + 40, 8, 1e4)
        ybuf = torch.full((M, 192), float("nan"), dtype=BF, device="cuda")
        y = ybuf[:, 32:32 + Z.COUT]
    else:
        y = torch.full((M, Z.COUT), float("nan"), dtype=BF, device="cuda")
    kw = {} if a is None else dict(a=a, b=b, geom=ops.Geom.per_sample(S, M // S), act=act)
    ops.vconv2d1d(x, wf, bs, bt, N, Z.F, Hh, Ww, out=y, **kw)
    ratio = E.check(y, ref, bound, pixels=Hh * Ww, what=f"vconv2d1d {name} gn={gn}")
    if strided:
        assert _untouched(ybuf, 32, Z.COUT), "guard columns of the output buffer written"
    print(f"\nRATIO vconv2d1d {name} gn={gn}: {ratio:.3f}")


# --------------------------------------------------------------------------- fused temporal-attention block
@functools.lru_cache(maxsize=None)
def _tattn_operands(N, HW, qk, off):
    name = next(c[0] for c in Z.TATTN_CASES if c[1:5] == (N, HW, qk, off))
    o = tuple(_cuda(t) for t in Z.tattn_case(name))
    return o, Z.tattn_ref(*o)


@pytest.mark.parametrize("case", Z.TATTN_CASES, ids=[c[0] for c in Z.TATTN_CASES])
def test_tattn_block_elementwise(ops, case):
    name, N, HW, qk, off, strided = case
    (x, wqkv, wproj, bqkv, bproj, gamma, beta, _, _), (ref, bound, validity) = _tattn_operands(N, HW, qk, off)
    assert validity < 0.5                                 # the validity condition of the propagation (tattn_ref asserts it as well)
    M, C = x.shape
    wf = ops.tattn_pack(wqkv, wproj)
    if strided:                                           # the engine's skip-concat buffers: x at columns 64 .. 320 of 384, y at 128 .. 384 of 512
        _, x = _guarded(x, 384, 64, 1e4)
        ybuf = torch.full((M, 512), float("nan"), dtype=BF, device="cuda")
        y = ybuf[:, 128:128 + C]
    else:
        y = torch.full((M, C), float("nan"), dtype=BF, device="cuda")
    ops.tattn_block(x, wf, bqkv, bproj, gamma, beta, Z.HEADS, N, Z.F, HW, out=y)
    ratio = E.check(y, ref, bound, what=f"tattn_block {name}")
    if strided:
        assert _untouched(ybuf, 128, C), "guard columns of the output buffer written"
    print(f"\nRATIO tattn_block {name}: {ratio:.3f}  (max sum p eta {validity:.3g})")
