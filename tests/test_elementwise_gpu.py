"""The conv-GEMM and attention forward kernels against float64, ELEMENT BY ELEMENT (tests/errbound.py: the bounds and their
derivation; tests/test_errbound_cpu.py: the metric proven on seeded defects).

Every case builds its reference with torch double ops on the stored operands - never with a libmmd kernel -, prefills the output
with NaN, and admits ZERO elements outside the per-element bound.  These are the roots of the suite's "bitwise equal to ..."
chains: the strip kernel, the ring tile, the halo tiles, mmd_tconv (bitwise conv_gemm), mmd_aconv (bitwise gn_apply + conv_gemm),
mmd_gn_conv1x1_skip, the halo loader of mmd_gn_conv_gemm and the FRONT stage of mmd_tattn_block (bitwise the strip GEMM) are compared
with tiles 64 / 128 / 129 of mmd_conv_gemm elsewhere, and here those tiles (and the others directly) meet an independent reference
on ragged M, ragged Cout, deep K, strided views, every tap form and every frame border.  The fused VideoConv (mmd_vconv2d1d) and
mmd_tattn_block itself hang on NO bitwise chain - their own tests compare whole tensors by rel-L2 (and, for the VideoConv, a 97 %
bitwise share) with the unfused paths -; they meet their float64 references element by element in
tests/test_elementwise_fused_gpu.py (staged references with propagated bounds: tests/errbound_fused.py).

Worst error / bound ratio per kernel / variant / dtype, as printed by the tests (`-s`) on an MI355X (`cases` = launches in the group):

    kernel                      variant     dtype  cases  worst ratio
    conv_gemm 1x1               tile 64     f32        7        0.045
    conv_gemm 1x1               tile 64     bf16       7        0.987
    conv_gemm 1x1               tile 128    f32        7        0.045
    conv_gemm 1x1               tile 128    bf16       7        0.987
    conv_gemm 1x1               tile 129    f32        7        0.045
    conv_gemm 1x1               tile 129    bf16       7        0.987
    conv_gemm 1x1               tile 132    f32        5        0.018
    conv_gemm 1x1               tile 132    bf16       5        0.980
    conv_gemm 3x3               tile 64     f32        6        0.010
    conv_gemm 3x3               tile 64     bf16       6        0.976
    conv_gemm 3x3               tile 128    f32        6        0.010
    conv_gemm 3x3               tile 128    bf16       6        0.976
    conv_gemm 3x3               tile 129    f32        6        0.010
    conv_gemm 3x3               tile 129    bf16       6        0.976
    conv_gemm halo              tile 130    f32       17        0.009
    conv_gemm halo              tile 130    bf16      17        0.961
    conv_gemm halo16            tile 133    bf16       5        0.801
    conv_gemm temporal          tile 64     f32        6        0.016
    conv_gemm temporal          tile 64     bf16       6        0.981
    conv_gemm temporal          tile 128    f32        6        0.016
    conv_gemm temporal          tile 128    bf16       6        0.981
    conv_gemm temporal          tile 129    f32        6        0.016
    conv_gemm temporal          tile 129    bf16       6        0.981
    conv_gemm temporal_d1       tile 130    f32        2        0.020
    conv_gemm temporal_d1       tile 130    bf16       2        0.982
    conv_gemm audio             tile 64     f32        8        0.035
    conv_gemm audio             tile 64     bf16       8        0.984
    conv_gemm audio             tile 128    f32        8        0.035
    conv_gemm audio             tile 128    bf16       8        0.984
    conv_gemm audio             tile 129    f32        8        0.035
    conv_gemm audio             tile 129    bf16       8        0.984
    conv_gemm strip             tile 131    bf16      53        0.991
    conv_gemm strided           tile 129    f32        1        0.027
    conv_gemm strided           tile 129    bf16       1        0.981
    conv_gemm strided           tile 131    bf16       1        0.981
    gn_conv1x1 (fused loader)   tile 128    bf16       2        0.985
    attn self                   impl 0      f32        5        0.037
    attn self                   impl 0      bf16       5        0.605
    attn self                   impl 1      bf16       5        0.964
    attn self                   impl 2      bf16       5        0.605
    attn self                   impl 3      bf16       2        0.312
    attn self                   impl 4      bf16       2        0.312
    attn cross                  impl 0      f32        5        0.044
    attn cross                  impl 0      bf16       5        0.641
    attn cross                  impl 1      bf16       5        0.989
    attn cross                  impl 2      bf16       5        0.641
    attn spike                  impl 0      f32        1        0.004
    attn spike                  impl 0      bf16       1        0.423
    attn spike                  impl 1      bf16       1        0.946
    attn spike                  impl 2      bf16       1        0.423
    attn spike                  impl 3      bf16       1        0.423
    attn spike                  impl 4      bf16       1        0.423
    attn temporal               attn_small  f32        3        0.017
    attn temporal               attn_small  bf16       3        0.976

Every case: zero violating elements.  The bf16 ratios of 0.96 - 0.99 (all conv tiles, the fused GroupNorm loader, the VALU attention
kernel impl 1 and attn_small) come from the output-rounding term 2**-8 |ref|: among the 1e4 - 1e6 stored elements of a group some
accumulator values land within 1 - 2 % of a bf16 rounding midpoint, and round-to-nearest then uses its whole half-ulp.  The
maxima occur at the shallow depths (K <= 512), where the fp32 accumulation term e32 is a few percent of the bound; a truncating
store reads 1.95 and a bf16 accumulator 27 on the same metric (tests/test_errbound_cpu.py).  Tile 133 (0.80) runs at K = 2304 only,
where e32 = 1.4e-4 S with S around 30 is as large as the rounding term and, being a worst-case term, is not filled.  The MFMA flash
kernels (impl 0 / 2 / 3 / 4 in bf16) sit at 0.3 - 0.65 because their bound carries the worst-case P term 2**-8 Sv, while the
roundings of the individual P_j average out over the keys.  No fp32 ratio exceeds 0.05: fp32 accumulation errors add like sqrt(K),
the bound grows like K.
"""
import pytest
import torch

import errbound as E

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DT = {"f32": F32, "bf16": BF}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mm_diffusion import ops as o
    return o


def _operands(M, Cin, Cout, ntaps, dt, seed, bias=True, res=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, Cin, device="cuda", generator=g).to(dt)
    w = (torch.randn(Cout, ntaps * Cin, device="cuda", generator=g) * (ntaps * Cin) ** -0.5).to(dt)
    b = torch.randn(Cout, device="cuda", generator=g) if bias else None
    r = torch.randn(M, Cout, device="cuda", generator=g).to(dt) if res else None
    return x, w, b, r


def _tile_takes(ops, tile, x, Cout, taps, dims):
    """(whether the forced main loop takes this launch, the reason when it does not) - from the package's own ops.*_ok rules."""
    if tile == 130:
        return ops.halo_tile_ok(x, taps, dims), "ops.halo_tile_ok: tile 130 does not take this launch"
    if tile == 133:
        return (ops.halo_tile_ok(x, taps, dims) and ops.halo_tile_code(x, taps, dims) == 133), "ops.halo_tile_code: tile 133 is not chosen for this launch (MMD_HALO16)"
    if tile == 131:
        return ops.strip_tile_pinned(x, Cout, taps), "ops.strip_tile_pinned: tile 131 does not take this launch (MMD_GEMM_STRIP)"
    if tile == 132:
        return ops.ring_tile_candidate(x, Cout, len(taps)), "ops.ring_tile_candidate: tile 132 does not take this launch (MMD_GEMM_RING)"
    return True, ""


def _run_conv(ops, name, tile, x, w, b, r, taps, dims, pixels=None):
    ok, why = _tile_takes(ops, tile, x, w.shape[0], taps, dims)
    if not ok:
        pytest.skip(why)
    y = torch.full((x.shape[0], w.shape[0]), float("nan"), dtype=x.dtype, device="cuda")
    ops.conv_gemm(x, w, b, taps=taps, dims=dims, residual=r, out=y, tile=tile)
    ref, S = E.conv_rows_ref(x, w, b, r, taps, dims)
    ratio = E.check(y, ref, E.gemm_bound(ref, S, len(taps) * x.shape[1], x.dtype), pixels, f"{name} tile {tile}")
    print(f"\nRATIO conv {name} tile={tile} {str(x.dtype)[6:]} res={int(r is not None)} bias={int(b is not None)}: {ratio:.3f}")
    return ratio


# --------------------------------------------------------------------------- conv_gemm, plain path
CONV = [(c, t, dt, res) for c in E.conv_cases() for t in c["tiles"] for dt in c["dtypes"] for res in (False, True)]


@pytest.mark.parametrize("case,tile,dt,res", CONV, ids=[f"{c['name']}-t{t}-{dt}-{'res' if res else 'nores'}" for c, t, dt, res in CONV])
def test_conv_gemm_elementwise(ops, case, tile, dt, res):
    nt = len(case["taps"])
    x, w, b, r = _operands(case["M"], case["Cin"], case["Cout"], nt, DT[dt], 100 + case["M"] + case["Cin"], res=res)
    _run_conv(ops, case["name"], tile, x, w, b, r, case["taps"], case["dims"], case["pixels"])


NOBIAS = ([("1x1-293x256x264", t, dt) for t in (64, 128, 129, 132) for dt in ("f32", "bf16")]
          + [("halo-2x24x48-192-264", 130, "f32"), ("halo-2x24x48-192-264", 130, "bf16"), ("halo16-2x16x32", 133, "bf16")])


@pytest.mark.parametrize("name,tile,dt", NOBIAS)
def test_conv_gemm_without_bias(ops, name, tile, dt):
    """bias = None once per tile: the zero page / the skipped bias load, with a residual."""
    case = next(c for c in E.conv_cases() if c["name"] == name)
    x, w, _, r = _operands(case["M"], case["Cin"], case["Cout"], len(case["taps"]), DT[dt], 7 + tile)
    _run_conv(ops, name, tile, x, w, None, r, case["taps"], case["dims"], case["pixels"])


# --------------------------------------------------------------------------- tile 131 (row strip, bf16)
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("name,M,Cin,Cout,taps,dims", E.strip_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_strip_elementwise(ops, name, M, Cin, Cout, taps, dims, res):
    x, w, b, r = _operands(M, Cin, Cout, len(taps), BF, 200 + M + Cout, res=res)
    _run_conv(ops, name, 131, x, w, b, r, taps, dims)


def test_strip_without_bias(ops):
    x, w, _, r = _operands(288, 256, 192, 1, BF, 11)
    _run_conv(ops, "strip-1x1-288x256x192", 131, x, w, None, r, E.TAPS_1, (1, 1, 1))


# --------------------------------------------------------------------------- strided views
@pytest.mark.parametrize("tile,dt", [(129, "f32"), (129, "bf16"), (131, "bf16")])
def test_strided_views_elementwise(ops, tile, dt):
    """Input, residual and output as column slices of wider buffers; the guard columns of the output stay NaN."""
    dt = DT[dt]
    M, Cin, Cout = 200, 128, 64
    g = torch.Generator(device="cuda").manual_seed(12)
    xb = torch.randn(M, 288, device="cuda", generator=g).to(dt)
    rb = torch.randn(M, 160, device="cuda", generator=g).to(dt)
    w = (torch.randn(Cout, Cin, device="cuda", generator=g) * Cin ** -0.5).to(dt)
    b = torch.randn(Cout, device="cuda", generator=g)
    ob = torch.full((M, 192), float("nan"), dtype=dt, device="cuda")
    x, r, y = xb[:, 96:96 + Cin], rb[:, 64:64 + Cout], ob[:, 64:64 + Cout]
    ok, why = _tile_takes(ops, tile, x, Cout, E.TAPS_1, (1, 1, 1))
    if not ok:
        pytest.skip(why)
    ops.conv_gemm(x, w, b, residual=r, out=y, tile=tile)
    ref, S = E.conv_rows_ref(x, w, b, r, E.TAPS_1, (1, 1, 1))
    ratio = E.check(y, ref, E.gemm_bound(ref, S, Cin, dt), what=f"strided views tile {tile}")
    assert bool(torch.isnan(ob[:, :64]).all()) and bool(torch.isnan(ob[:, 64 + Cout:]).all()), "guard columns written"
    print(f"\nRATIO conv strided-200x128x64 tile={tile} {str(dt)[6:]} res=1 bias=1: {ratio:.3f}")


# --------------------------------------------------------------------------- GroupNorm fused into the tile-128 loader
def test_gn_fused_loader_tile128_elementwise(ops):
    """gn_conv1x1(tile=128): the GEMM half in isolation.  The reference is conv_rows_ref on gn_apply's STORED bf16 output (gn_apply
    has its own fp64-level tests); the loader's operand is bit for bit that output (errbound.py: same expressions), so the
    plain GEMM bound holds with no extra term.  400 rows per sample: the 128-row blocks straddle the samples."""
    S, Tn, Cin, Cout = E.GN_LOADER_CASE
    g = torch.Generator(device="cuda").manual_seed(13)
    x = (torch.randn(S * Tn, Cin, device="cuda", generator=g) * 1.3 + 0.2).to(BF)
    w = (torch.randn(Cout, Cin, device="cuda", generator=g) * Cin ** -0.5).to(BF)
    b = torch.randn(Cout, device="cuda", generator=g)
    r = torch.randn(S * Tn, Cout, device="cuda", generator=g).to(BF)
    gamma, beta = 1 + 0.1 * torch.randn(Cin, device="cuda", generator=g), torch.randn(Cin, device="cuda", generator=g)
    film = torch.randn(S, 2 * Cin, device="cuda", generator=g) * 0.3
    geom = ops.Geom.per_sample(S, Tn)
    a_, b_ = ops.gn_stats(x, gamma, beta, geom, film=film)
    for act in (True, False):
        xn = ops.gn_apply(x, a_, b_, geom, act=act)
        y = torch.full((S * Tn, Cout), float("nan"), dtype=BF, device="cuda")
        ops.gn_conv1x1(x, a_, b_, geom, act, w, b, residual=r, out=y, tile=128)
        ref, Sa = E.conv_rows_ref(xn, w, b, r, E.TAPS_1, (1, 1, 1))
        ratio = E.check(y, ref, E.gemm_bound(ref, Sa, Cin, BF), what=f"gn_conv1x1 tile 128 act={act}")
        print(f"\nRATIO gn_conv1x1 3x400x256x256 tile=128 bf16 act={int(act)}: {ratio:.3f}")


# --------------------------------------------------------------------------- attention forward
def _impls(ch):
    """(dtype, impl, rounding of P) for every impl tests/test_ops_gpu.py exercises: 0 = auto, 1 = VALU kernel (P in fp32), 2 = per-128-query
    MFMA kernel, 3 = staged-window kernel and 4 = DMA-staged kernel (head width 64 only)."""
    out = [("f32", 0, 0.0), ("bf16", 0, None), ("bf16", 1, 0.0), ("bf16", 2, None)]
    return out + ([("bf16", 3, None), ("bf16", 4, None)] if ch == 64 else [])


def _qkv(rows, C, dt, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(rows, 3 * C, device="cuda", generator=g) * scale).to(dt)


def _check_attn(out, qrows, kvrows, pairs, heads, dt, p_round, what):
    """pairs: (query row indices, key row indices) of every (batch, group); every output row is covered exactly once."""
    C = out.shape[1]
    ref, bound = torch.empty(out.shape, dtype=torch.float64, device="cuda"), torch.empty(out.shape, dtype=torch.float64, device="cuda")
    seen = torch.zeros(out.shape[0], dtype=torch.int32, device="cuda")
    for qi, ki in pairs:
        r, Sv, e32 = E.attn_ref(qrows[qi, :C], kvrows[ki, C:2 * C], kvrows[ki, 2 * C:], heads)
        ref[qi], bound[qi] = r, E.attn_bound(r, Sv, dt, e32, p_round)
        seen[qi] += 1
    assert bool((seen == 1).all())
    return E.check(out, ref, bound, what=what)


SELF = [(T, h, ch, *i) for T, h, ch in E.SELF_ATTN for i in _impls(ch)]


@pytest.mark.parametrize("T,heads,ch,dt,impl,p_round", SELF, ids=[f"T{c[0]}-h{c[1]}-ch{c[2]}-{c[3]}-impl{c[4]}" for c in SELF])
def test_self_attention_elementwise(ops, T, heads, ch, dt, impl, p_round):
    N, G, C = 2, 2, heads * ch
    qkv = _qkv(N * G * T, C, DT[dt], 25)
    out = torch.full((N * G * T, C), float("nan"), dtype=DT[dt], device="cuda")
    ops.attn(qkv, qkv, out, heads, ch, N, G, G * T, T, G * T, T, 1, impl=impl)
    idx = [torch.arange(s * T, (s + 1) * T, device="cuda") for s in range(N * G)]
    ratio = _check_attn(out, qkv, qkv, [(i, i) for i in idx], heads, DT[dt], p_round, f"self-attention impl {impl}")
    print(f"\nRATIO attn self T={T} h={heads} ch={ch} {dt} impl={impl}: {ratio:.3f}")


CROSS = [(*c, *i) for c in E.CROSS_ATTN for i in _impls(c[6])]


@pytest.mark.parametrize("F,HW,L,win,shift,heads,ch,dt,impl,p_round", CROSS,
                         ids=[f"F{c[0]}-HW{c[1]}-L{c[2]}-w{c[3]}-s{c[4]}-h{c[5]}-ch{c[6]}-{c[7]}-impl{c[8]}" for c in CROSS])
def test_cross_attention_windows_elementwise(ops, F, HW, L, win, shift, heads, ch, dt, impl, p_round):
    """RS-MMA in both directions: wrap-around windows, one audio token per frame, L % F != 0 (the last group owns the remainder)."""
    N, C = 2, heads * ch
    apf = L // F
    vq, aq = _qkv(N * F * HW, C, DT[dt], 26), _qkv(N * L, C, DT[dt], 27)
    sh = torch.tensor([shift], dtype=torch.int32, device="cuda")
    vo = torch.full((N * F * HW, C), float("nan"), dtype=DT[dt], device="cuda")
    ao = torch.full((N * L, C), float("nan"), dtype=DT[dt], device="cuda")
    ops.attn(vq, aq, vo, heads, ch, N, F, F * HW, HW, L, apf, win, shift_dev=sh, impl=impl)
    ops.attn(aq, vq, ao, heads, ch, N, F, L, apf, F * HW, HW, win, shift_dev=sh, impl=impl)
    ar = lambda *a: torch.arange(*a, device="cuda")
    vpairs, apairs = [], []
    for n in range(N):
        for i in range(F):
            vpairs.append((n * F * HW + ar(i * HW, (i + 1) * HW), n * L + (ar(win * apf) + (i + shift) * apf) % L))
            apairs.append((n * L + ar(i * apf, L if i == F - 1 else (i + 1) * apf), n * F * HW + (ar(win * HW) + (i + shift) * HW) % (F * HW)))
    rv = _check_attn(vo, vq, aq, vpairs, heads, DT[dt], p_round, f"video <- audio impl {impl}")
    ra = _check_attn(ao, aq, vq, apairs, heads, DT[dt], p_round, f"audio <- video impl {impl}")
    print(f"\nRATIO attn cross F={F} HW={HW} L={L} win={win} shift={shift} {dt} impl={impl}: {max(rv, ra):.3f}")


@pytest.mark.parametrize("dt,impl,p_round", _impls(64), ids=lambda v: str(v))
def test_attention_softmax_spike_elementwise(ops, dt, impl, p_round):
    """The input of test_ops_gpu.py::test_attention_softmax_spike at key 250: one key dominates query 7 late in the sequence."""
    T = 300
    g = torch.Generator().manual_seed(28)
    qkv = torch.randn(T, 192, generator=g).to(BF).float() * 0.3
    qkv[250, 64:128] = qkv[7, :64] * 40.0
    qkv = qkv.to(BF).to(DT[dt]).cuda()
    out = torch.full((T, 64), float("nan"), dtype=DT[dt], device="cuda")
    ops.attn(qkv, qkv, out, 1, 64, 1, 1, T, T, T, T, 1, impl=impl)
    i = torch.arange(T, device="cuda")
    ratio = _check_attn(out, qkv, qkv, [(i, i)], 1, DT[dt], p_round, f"softmax spike impl {impl}")
    print(f"\nRATIO attn spike T=300 {dt} impl={impl}: {ratio:.3f}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("F,HW,heads,ch", E.TEMPORAL_ATTN)
def test_temporal_attention_elementwise(ops, dt, F, HW, heads, ch):
    """attn_small over (pixel, head) slices of F frames.  bf16 at these head widths and F <= 16 runs attn_small_mfma_kernel: P as a
    bf16 hi + lo pair (p_round = 2**-16); fp32 mode runs the VALU kernel."""
    N, C = 2, heads * ch
    qkv = _qkv(N * F * HW, C, DT[dt], 29)
    out = torch.full((N * F * HW, C), float("nan"), dtype=DT[dt], device="cuda")
    ops.attn_small(qkv, out, C, heads, ops.Geom.temporal(N, F, HW))
    idx = [n * F * HW + torch.arange(F, device="cuda") * HW + p for n in range(N) for p in range(HW)]
    assert ch in (32, 64, 96, 128) and F <= 16                       # (else bf16 runs the VALU kernel: p_round 0)
    ratio = _check_attn(out, qkv, qkv, [(i, i) for i in idx], heads, DT[dt], 2.0 ** -16 if dt == "bf16" else 0.0, "temporal attention")
    print(f"\nRATIO attn temporal F={F} HW={HW} h={heads} ch={ch} {dt}: {ratio:.3f}")
