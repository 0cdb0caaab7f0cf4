"""The element-wise metric of tests/errbound_bwd.py, proven on the CPU (the backward twin of tests/test_errbound_cpu.py).

1. The float64 references equal torch autograd of float64 primitives (conv1d, conv2d - the frames of a 3 x 3 and the (F, HW) planes of
   a temporal conv are conv3d with a unit axis -, group_norm with FiLM and SiLU, explicit softmax attention) to 1e-12 on every shape of
   tests/test_elementwise_bwd_gpu.py: all case lists live in tests/errbound_bwd.py and both files iterate over them.
2. A faithful emulation of each kernel's arithmetic - fp32 accumulation in a scrambled order, bf16 roundings exactly where the kernel
   has them, stored O and stored lse2 from an emulated forward - has ZERO violating elements on every GPU shape, and the exact-sum
   inputs give bitwise the float64 reference under three accumulation orders.
3. Fifteen seeded defects are each flagged by `check`; `DEFECT_LOG` records for each whether the whole-tensor rel-L2 tolerance of
   tests/test_bwd_gpu.py (2e-2 bf16, 5e-5 fp32) would have passed it, and the last test asserts that four do:

       defect                                              rel-L2    old tolerance
       wgrad: last 64-row chunk dropped (one wave's tile)  1.7e-02   PASSES (2e-2)
       wgrad: one split added twice (one wave's tile)      3.4e-02   fails
       wgrad: border mask of a tap wraps                   6.1e-02   fails
       dgrad: taps not negated                             1.3e+00   fails
       wgrad: ci * ntaps + tap swapped with tap * Cin + ci 1.4e+00   fails
       db: ragged tail missing                             1.7e-01   fails
       attention: D from the neighbouring head             3.2e-01   fails
       attention: scale missing from dK                    5.9e+00   fails
       attention: window start off by one group            5.8e-01   fails
       attention: dS rounded to bf16 twice                 2.9e-03   PASSES
       attention: keys outside every window not zero       9.4e-03   PASSES
       GroupNorm: v (1 - sg) of SiLU' dropped              2.5e-01   fails
       GroupNorm: last Tn % RPP rows skipped (dx)          6.8e-03   PASSES
       GroupNorm: m2 divided by the wrong count            1.0e-01   fails
       GroupNorm: FiLM 1 + scale missing from dgamma       2.7e-01   fails (5e-5)
   (the numbers of one run; the test prints them with -s)
"""
import math

import pytest
import torch
import torch.nn.functional as F_

import errbound as E
import errbound_bwd as B
from helpers import rel_l2

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DT = {"f32": F32, "bf16": BF}
OLD_TOL = {BF: 2e-2, F32: 5e-5}
DEFECT_LOG = {}


def _log(name, got, ref, dt):
    r = rel_l2(got.double(), ref)
    DEFECT_LOG[name] = (r, r < OLD_TOL[dt])
    print(f"\nDEFECT {name}: rel-L2 {r:.2e} -> the old tolerance {OLD_TOL[dt]:g} {'PASSES' if r < OLD_TOL[dt] else 'fails'} it")


def _close12(a, b):
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# --------------------------------------------------------------------------- conv
def _conv_torch(xr, w, taps, dims, M):
    """The conv of the row tensor xr [M, Cin] with the torch-layout weight w [Cout, Cin, ntaps] through torch's own convolutions."""
    Cin, nt = xr.shape[1], len(taps)
    D0, D1, D2 = dims
    if nt == 1:
        return F_.conv1d(xr.t()[None], w).squeeze(0).t()
    if nt == 9:
        x = xr.reshape(-1, D1, D2, Cin).permute(0, 3, 1, 2)
        return F_.conv2d(x, w.reshape(w.shape[0], Cin, 3, 3), padding=1).permute(0, 2, 3, 1).reshape(M, -1)
    if taps == E.TAPS_TEMPORAL:
        x = xr.reshape(-1, D0, D1, Cin).permute(0, 3, 1, 2)
        return F_.conv2d(x, w[..., None], padding=(1, 0)).permute(0, 2, 3, 1).reshape(M, -1)
    d = taps[2][0]
    x = xr.reshape(-1, D0, Cin).permute(0, 2, 1)
    return F_.conv1d(x, w, padding=d, dilation=d).permute(0, 2, 1).reshape(M, -1)


WG = [(c, ch) for c in B.wgrad_cases() for ch in c["chans"]]
WG_IDS = [f"{c['name']}-{ci}-{co}" for c, (ci, co) in WG]
WG_ALL = WG + B.wgrad64_bf16_cases()                         # + wgrad_kernel<__bf16>: Cin < 64 or Cout < 64, Cout = 2056
WG_ALL_IDS = [f"{c['name']}-{ci}-{co}" for c, (ci, co) in WG_ALL]


def _plan(case, chans):
    """(splits, rows per split, xcd order) of the bf16 launch: the 128-tile plan of the case, or the 64-tile's for the narrow widths."""
    return B.wgrad_plan(case["M"], chans[0], chans[1], len(case["taps"]), True)[1:]


def test_wgrad_plans_are_the_derived_ones():
    for c, (ci, co) in WG:
        assert B.wgrad_plan(c["M"], ci, co, len(c["taps"]), True) == ("tr",) + c["plan"], c["name"]
        assert B.exact_sum_ok(c["M"]) and B.exact_sum_ok(len(c["taps"]) * co)


@pytest.mark.parametrize("case,chans", WG_ALL + [(B.wgrad_case(g), (ci, co)) for g, ci, co in B.DGRAD if (ci, co) == (128, 72)],
                         ids=WG_ALL_IDS + ["dgrad-3x3-2x21x25-128-72"])
def test_conv_backward_refs_equal_autograd(case, chans):
    Cin, Cout = chans
    M, taps, dims, nt = case["M"], case["taps"], case["dims"], len(case["taps"])
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, Cin, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(Cout, Cin, nt, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(M, Cout, generator=g, dtype=F64)
    _conv_torch(x, w, taps, dims, M).backward(dy)
    dW, _, db, _ = B.wgrad_ref(dy, x, taps, dims)
    _close12(B.to_torch_layout(dW, Cin, nt), w.grad.reshape(Cout, Cin * nt))
    _close12(db, dy.sum(0))
    wt, ntaps = B.dgrad_operands(w.detach(), taps)
    _close12(E.conv_rows_ref(dy, wt, None, None, ntaps, dims)[0], x.grad)


def emulate_wgrad(dy, x, taps, dims, plan, seed, defect=None, blk=None):
    """What the 128-tile kernels do: per row split the 64-row chunks accumulated in fp32 (a matmul per chunk, chunks in a scrambled
    order), the splits added in a scrambled order onto zeros.  Returns dW [Cout, ntaps * Cin] fp32 (packed) and db.
    blk = (co slice, tap, ci slice): the one block a block-level defect hits."""
    splits, rps, _ = plan
    M, Cin = x.shape
    Cout, nt = dy.shape[1], len(taps)
    gen = torch.Generator().manual_seed(seed)
    xf, dyf = x.float(), dy.float()
    gath = [gx for gx, _ in E.conv_gather(xf, taps, dims)]
    if defect == "border_wrap":                      # tap (0, 0, +1): the p2 + 1 < D2 test dropped - reads the next frame row's first pixel
        t = taps.index((0, 0, 1))
        m = torch.arange(M)
        gath[t] = xf[(m + 1).clamp(max=M - 1)] * (m + 1 < M)[:, None]
    G = torch.cat(gath, dim=1)                       # [M, nt * Cin]
    dW = torch.zeros(Cout, nt * Cin)
    db = torch.zeros(Cout)
    order = torch.randperm(splits, generator=gen).tolist()
    if defect == "split_twice":
        order.append(order[0])
    for si, s in enumerate(order):
        lo, hi = s * rps, min((s + 1) * rps, M)
        chunks = list(range(lo, hi, 64))
        chunks = [chunks[i] for i in torch.randperm(len(chunks), generator=gen).tolist()]
        acc, accb = torch.zeros(Cout, nt * Cin), torch.zeros(Cout)
        for c0 in chunks:
            c1 = min(c0 + 64, hi)
            part = dyf[c0:c1].t() @ G[c0:c1]
            if defect == "drop_chunk" and s == splits - 2 and c0 == max(chunks):       # the split's last 64 rows, wherever the order put them
                co, t, ci = blk
                part[co, t * Cin + ci.start:t * Cin + ci.stop] = 0
            if not (defect == "db_tail" and c1 - c0 < 64):
                accb = accb + dyf[c0:c1].sum(0)
            acc = acc + part
        if defect == "split_twice" and si == len(order) - 1:            # the doubled split: one block only
            co, t, ci = blk
            keep = torch.zeros_like(acc)
            keep[co, t * Cin + ci.start:t * Cin + ci.stop] = acc[co, t * Cin + ci.start:t * Cin + ci.stop]
            acc, accb = keep, torch.zeros(Cout)
        dW = dW + acc
        db = db + accb
    return dW, db


def _wg_inputs(case, chans, dt, seed, exact=False):
    Cin, Cout = chans
    g = torch.Generator().manual_seed(seed)
    if exact:
        return B.grid_randn((case["M"], Cout), g).to(dt), B.grid_randn((case["M"], Cin), g).to(dt)
    return torch.randn(case["M"], Cout, generator=g).to(dt), torch.randn(case["M"], Cin, generator=g).to(dt)


@pytest.mark.parametrize("case,chans", WG_ALL, ids=WG_ALL_IDS)
def test_wgrad_emulation_has_no_violation_and_exact_sums_are_bitwise(case, chans):
    M, taps, dims = case["M"], case["taps"], case["dims"]
    plan = _plan(case, chans)
    assert (case, chans) not in WG or plan == case["plan"]
    for dt in (BF, F32):
        dy, x = _wg_inputs(case, chans, dt, 5)
        dW, S, db, Sb = B.wgrad_ref(dy, x, taps, dims)
        got, gdb = emulate_wgrad(dy, x, taps, dims, plan, 1)
        B.check_groups(got, dW, B.wgrad_bound(S, M, dt), chans[0], "tap", f"{case['name']} emulation")
        E.check(gdb[None], db[None], B.colsum_bound(Sb, M)[None], what="db emulation")
    dy, x = _wg_inputs(case, chans, BF, 6, exact=True)
    dW, _, db, _ = B.wgrad_ref(dy, x, taps, dims)
    for seed in (1, 2, 3):
        got, gdb = emulate_wgrad(dy, x, taps, dims, plan, seed)
        assert torch.equal(got, dW.float()) and torch.equal(gdb, db.float())
    assert torch.equal(dW.float().double(), dW)                           # (the reference itself is exact in fp32)


_case = B.wgrad_case


@pytest.mark.parametrize("defect", ["drop_chunk", "split_twice", "border_wrap", "layout_swap", "db_tail"])
def test_wgrad_seeded_defects_are_flagged(defect):
    case, chans = _case("3x3-2x33x31"), (192, 264)
    M, taps, dims, Cin = case["M"], case["taps"], case["dims"], chans[0]
    blk = (slice(128, 192), 4, slice(0, 64))                              # one wave's 64 x 64 quadrant of one 128 x 128 block
    for exact in (False, True):
        dy, x = _wg_inputs(case, chans, BF, 7, exact=exact)
        dW, S, db, Sb = B.wgrad_ref(dy, x, taps, dims)
        got, gdb = emulate_wgrad(dy, x, taps, dims, case["plan"], 1, defect=defect, blk=blk)
        if defect == "layout_swap":                                          # written as [co][ci][tap], read back as [co][tap][ci]
            got = B.to_torch_layout(got, Cin, len(taps))
        if defect == "db_tail":
            nbad = E.violations(gdb[None], db[None], B.colsum_bound(Sb, M)[None])[0]
            assert nbad > 0 and (not exact or not torch.equal(gdb, db.float()))
            if not exact:
                _log("db: ragged tail missing", gdb, db, BF)
            continue
        with pytest.raises(AssertionError, match="outside the bound"):
            B.check_groups(got, dW, B.wgrad_bound(S, M, BF), Cin, "tap", defect)
        assert not exact or not torch.equal(got, dW.float())
        if not exact:
            _log({"drop_chunk": "wgrad: last 64-row chunk of one split dropped (one wave's tile)", "split_twice": "wgrad: one split added twice (one wave's tile)",
                  "border_wrap": "wgrad: border mask of a tap wraps", "layout_swap": "wgrad: ci * ntaps + tap swapped with tap * Cin"}[defect],
                 got, dW, BF)


def emulate_dgrad(dy, wt, taps, dims, out_dtype, seed):
    """conv_gemm on dY with the transposed weight: the K = ntaps * Cout products accumulated in fp32 in 64-wide steps over a scrambled
    K order, one round-to-nearest store."""
    G = torch.cat([gx for gx, _ in E.conv_gather(dy.float(), taps, dims)], 1)
    perm = torch.randperm(G.shape[1], generator=torch.Generator().manual_seed(seed))
    acc = torch.zeros(G.shape[0], wt.shape[0])
    for k0 in range(0, len(perm), 64):
        idx = perm[k0:k0 + 64]
        acc = acc + G[:, idx] @ wt.float()[:, idx].t()
    return acc.to(out_dtype)


def _dgrad_inputs(geom, Cin, Cout, dt, exact):
    case = B.wgrad_case(geom)
    M, taps, nt = case["M"], case["taps"], len(case["taps"])
    g = torch.Generator().manual_seed(8)
    if exact:
        dy, w = B.grid_randn((M, Cout), g).to(dt), B.grid_randn((Cout, Cin, nt), g).to(dt)
    else:
        dy, w = torch.randn(M, Cout, generator=g).to(dt), (torch.randn(Cout, Cin, nt, generator=g) * (nt * Cout) ** -0.5).to(dt)
    return case, dy, w


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("geom,Cin,Cout", B.DGRAD)
def test_dgrad_emulation_has_no_violation_and_exact_sums_are_bitwise(geom, Cin, Cout, dt):
    for exact in (False, True):
        case, dy, w = _dgrad_inputs(geom, Cin, Cout, DT[dt], exact)
        taps, dims, K = case["taps"], case["dims"], len(case["taps"]) * Cout
        wt, ntaps = B.dgrad_operands(w, taps)
        ref, S = E.conv_rows_ref(dy, wt, None, None, ntaps, dims)
        for seed in (1, 2, 3):
            got = emulate_dgrad(dy, wt, ntaps, dims, DT[dt], seed)
            if exact:
                assert B.exact_sum_ok(K) and torch.equal(got, ref.float().to(DT[dt]))
            else:
                E.check(got, ref, E.gemm_bound(ref, S, K, DT[dt]), what=f"dgrad emulation {geom}")


def test_dgrad_unnegated_taps_are_flagged():
    for exact in (False, True):
        case, dy, w = _dgrad_inputs("3x3-2x5x7", 64, 96, BF, exact)
        taps, dims = case["taps"], case["dims"]
        wt, ntaps = B.dgrad_operands(w, taps)
        ref, S = E.conv_rows_ref(dy, wt, None, None, ntaps, dims)
        bad = emulate_dgrad(dy, wt, taps, dims, BF, 1)
        assert E.violations(bad, ref, E.gemm_bound(ref, S, 9 * 96, BF))[0] > 0
        if exact:
            assert not torch.equal(bad, ref.float().to(BF))
        else:
            _log("dgrad: taps not negated", bad, ref, BF)


@pytest.mark.parametrize("S,Tn,C,dt", B.COLSUM_SLICES)
def test_colsum_slices_emulation_has_no_violation_and_exact_sums_are_bitwise(S, Tn, C, dt):
    """fp32 row-by-row accumulation in a scrambled order: random inputs within (Tn + 1) u Sb, exact-sum inputs bitwise, three orders."""
    g = torch.Generator().manual_seed(9)
    assert B.exact_sum_ok(Tn)
    for exact in (False, True):
        dy = (B.grid_randn((S * Tn, C), g) if exact else torch.randn(S * Tn, C, generator=g)).to(DT[dt])
        d3 = dy.double().reshape(S, Tn, C)
        ref, Sb = d3.sum(1), d3.abs().sum(1)
        for seed in (1, 2, 3):
            perm = torch.randperm(Tn, generator=torch.Generator().manual_seed(seed))
            acc = torch.zeros(S, C)
            for j in perm.tolist():
                acc = acc + dy.float().reshape(S, Tn, C)[:, j]
            if exact:
                assert torch.equal(acc, ref.float())
            else:
                E.check(acc, ref, B.colsum_bound(Sb, Tn), what="colsum_slices emulation")


# --------------------------------------------------------------------------- GroupNorm
def _gn_inputs(dt, C, kind, Tn, big, device="cpu", seed=11):
    N, HW = 2, 3
    g = torch.Generator(device=device).manual_seed(seed + C + Tn)
    slices, geom = B.gn_slices(kind, N, Tn, HW)
    rows = slices.numel()
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    x = ((rn(rows, C) * (1.0 if big else 1.5) + (20.0 if big else 0.3))).to(DT[dt])
    dy = rn(rows, C).to(DT[dt])
    gamma, beta = 1 + 0.1 * rn(C), rn(C)
    film = rn(geom[0], 2 * C) * 0.3 if kind == "per_sample_film" else None
    return x, dy, gamma, beta, film, kind.startswith("per_sample"), slices, geom


@pytest.mark.parametrize("dt,C,kind,Tn,big", B.gn_cases() + [(*c, False) for c in B.GN_AUTOGRAD], ids=str)
def test_gn_bwd_ref_equals_autograd(dt, C, kind, Tn, big):
    x, dy, gamma, beta, film, act, slices, _ = _gn_inputs(dt, C, kind, Tn, big)
    S = slices.shape[0]
    xl, gl, bl = (t.double().clone().requires_grad_(True) for t in (x, gamma, beta))
    fl = None if film is None else film.double().clone().requires_grad_(True)
    y = F_.group_norm(xl[slices].permute(0, 2, 1), 32, gl, bl, B.GN_EPS)                # [S, C, Tn]
    if fl is not None:
        y = y * (1 + fl[:, :C, None]) + fl[:, C:, None]
    if act:
        y = F_.silu(y)
    y.backward(dy.double()[slices].permute(0, 2, 1))
    r = B.gn_bwd_ref(x, dy, gamma, beta, film, act, slices)
    _close12(r["dx"], xl.grad)
    _close12(r["dgamma"], gl.grad)
    _close12(r["dbeta"], bl.grad)
    if fl is not None:
        _close12(r["dfilm"], fl.grad)


def emulate_gn(x, dy, gamma, beta, film, act, slices, seed, defect=None, rpp=1):
    """The three stages in fp32 as the kernels order them (rows in a scrambled order), from an emulated fp32 forward."""
    S, Tn = slices.shape
    C = x.shape[1]
    cpg = C // 32
    gen = torch.Generator().manual_seed(seed)
    perm = torch.randperm(Tn, generator=gen)
    xs, ds = x.float()[slices][:, perm], dy.float()[slices][:, perm]                # [S, Tn, C]
    rep = lambda t: t.repeat_interleave(cpg, dim=-1)
    # forward: shifted sums in fp32, the rest in double, rounded once
    piv = x.float()[slices][:, :1].reshape(S, 1, 32, cpg)[..., :1]
    d = xs.reshape(S, Tn, 32, cpg) - piv
    sd, sq = torch.zeros(S, 32, cpg), torch.zeros(S, 32, cpg)
    for j in range(Tn):
        sd, sq = sd + d[:, j], sq + d[:, j] * d[:, j]
    cnt = Tn * cpg
    dm = sd.double().sum(-1) / cnt
    var = (sq.double().sum(-1) / cnt - dm * dm).clamp_min(0)
    mean, rstd = (piv[:, 0, :, 0].double() + dm).float(), (1.0 / torch.sqrt(var + B.GN_EPS)).float()
    a = rep(rstd) * gamma
    b = beta - rep(mean) * a
    sc1 = 1 + film[:, :C] if film is not None else torch.ones(S, C)
    if film is not None:
        a, b = a * sc1, b * sc1 + film[:, C:]
    # backward
    if act:
        v = xs * a[:, None] + b[:, None]
        sg = 1.0 / (1.0 + torch.exp(-v))
        dv = ds * (sg * (1.0 + (0 if defect == "silu_term" else 1) * v * (1.0 - sg)))
    else:
        dv = ds
    z = (xs - rep(mean)[:, None]) * rep(rstd)[:, None]
    P, Q = torch.zeros(S, C), torch.zeros(S, C)
    nrows = Tn - Tn % rpp if defect == "skip_rows" else Tn
    for j in range(nrows):
        P, Q = P + dv[:, j], Q + dv[:, j] * z[:, j]
    g = sc1 * gamma
    cntf = float(Tn if defect == "m2_count" else cnt)
    m1 = (g * P).reshape(S, 32, cpg).sum(-1) / float(cnt)
    m2 = (g * Q).reshape(S, 32, cpg).sum(-1) / cntf
    rs, mu = rep(rstd)[:, None], rep(mean)[:, None]
    k1, k2, k3 = rs * g[:, None], -rs * rs * rep(m2)[:, None], rs * (mu * rs * rep(m2)[:, None] - rep(m1)[:, None])
    dxs = (k1 * dv + k2 * xs + k3).to(x.dtype)
    dx = torch.full(x.shape, float("nan"), dtype=x.dtype)
    dx[slices[:, perm]] = dxs
    dgamma = ((Q if defect == "film_dgamma" else sc1 * Q)).sum(0)
    out = dict(dx=dx, dgamma=dgamma, dbeta=(sc1 * P).sum(0), a=a, b=b, mean=mean, rstd=rstd)
    out["dfilm"] = None if film is None else torch.cat([gamma * Q + beta * P, P], 1)
    return out


@pytest.mark.parametrize("dt,C,kind,Tn,big", B.gn_cases() + [(*c, False) for c in B.GN_AUTOGRAD], ids=str)
def test_gn_emulation_has_no_violation(dt, C, kind, Tn, big):
    x, dy, gamma, beta, film, act, slices, _ = _gn_inputs(dt, C, kind, Tn, big)
    got = emulate_gn(x, dy, gamma, beta, film, act, slices, 1)
    r = B.gn_bwd_ref(x, dy, gamma, beta, film, act, slices, stored=(got["a"], got["b"], got["mean"], got["rstd"]), out_dtype=DT[dt])
    B.check_gn(got, r, f"GroupNorm emulation {dt} C={C} {kind} Tn={Tn}")


@pytest.mark.parametrize("defect,key", [("silu_term", "dx"), ("skip_rows", "dx"), ("m2_count", "dx"), ("film_dgamma", "dgamma")])
def test_gn_seeded_defects_are_flagged(defect, key):
    dt, C, kind, Tn = "bf16", 160, "per_sample_film", 257
    x, dy, gamma, beta, film, act, slices, _ = _gn_inputs(dt, C, kind, Tn, False)
    got = emulate_gn(x, dy, gamma, beta, film, act, slices, 1, defect=defect, rpp=12)        # 256 / (160 / 8) = 12 row lanes: 257 % 12 = 5
    r = B.gn_bwd_ref(x, dy, gamma, beta, film, act, slices, stored=(got["a"], got["b"], got["mean"], got["rstd"]), out_dtype=BF)
    ok = ~torch.isnan(r["dx"][:, 0])
    g_, r_, e_ = (got["dx"][ok], r["dx"][ok], r["e_dx"][ok]) if key == "dx" else (got[key][None], r[key][None], r["e_" + key][None])
    assert E.violations(g_, r_, e_)[0] > 0
    _log({"silu_term": "GroupNorm: v (1 - sg) of SiLU' dropped", "skip_rows": "GroupNorm: last Tn % RPP rows skipped (dx)",
          "m2_count": "GroupNorm: m2 divided by the wrong count", "film_dgamma": "GroupNorm: FiLM 1 + scale missing from dgamma"}[defect],
         g_, r_, BF if key == "dx" else F32)
    if defect == "skip_rows":                                               # the skipped rows also show in the parameter gradients
        assert E.violations(got["dgamma"][None], r["dgamma"][None], r["e_dgamma"][None])[0] > 0


# --------------------------------------------------------------------------- attention
def _attn_inputs(Nq, Nk, C, dt, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device).to(dt)
    return rn(Nq, 3 * C), (rn(Nk, 3 * C) if Nk else None), rn(Nq, C)


def _autograd_attn(qbuf, kvbuf, do, pairs, heads):
    C = do.shape[1]
    ch = C // heads
    ql, kl = qbuf.double().clone().requires_grad_(True), kvbuf.double().clone().requires_grad_(True)
    loss = 0
    for qi, ki in pairs:
        hd = lambda t: t.reshape(-1, heads, ch).permute(1, 0, 2)
        p = torch.softmax(hd(ql[qi, :C]) @ hd(kl[ki, C:2 * C]).transpose(1, 2) / math.sqrt(ch), -1)
        loss = loss + ((p @ hd(kl[ki, 2 * C:])).permute(1, 0, 2).reshape(-1, C) * do.double()[qi]).sum()
    loss.backward()
    return ql.grad, kl.grad


def emulate_attn_bwd(qbuf, kvbuf, do, pairs, heads, mode, out_dtype, seed=1, defect=None):
    """Forward and backward of one attention call as the kernels compute them.  mode 'mfma': stored bf16 O and fp32 lse2 from the
    forward, P = exp2(s * scale * log2e - lse2), P and dS rounded to bf16 in front of the second product; 'valu': the same with the
    kernel's own fp32 log-sum-exp and fp32 P / dS; 'small': P = e / sum e, D = sum_j P_j dP_j.  Keys in a scrambled order.
    Returns dq [Nq, C], dk, dv [Nk, C] in out_dtype, and the stored o, lse2."""
    C = do.shape[1]
    ch = C // heads
    sc = torch.tensor(1.0 / math.sqrt(ch), dtype=F32)
    gen = torch.Generator().manual_seed(seed)
    Nq, Nk = qbuf.shape[0], kvbuf.shape[0]
    hd = lambda t: t.float().reshape(-1, heads, ch).permute(1, 0, 2)
    back = lambda t: t.permute(1, 0, 2).reshape(-1, C)
    dq, o = torch.zeros(Nq, C), torch.zeros(Nq, C, dtype=out_dtype)
    lse2 = torch.zeros(Nq, heads)
    dk, dv = torch.zeros(Nk, C), torch.zeros(Nk, C)
    rb = (lambda t: t.to(BF).float()) if mode == "mfma" else (lambda t: t)
    for pi, (qi, ki) in enumerate(pairs):
        if defect == "window_off" and pi == 0:
            ki = pairs[1][1]
        ki = ki[torch.randperm(len(ki), generator=gen)]
        qh, kh, vh, gh = hd(qbuf[qi, :C]), hd(kvbuf[ki, C:2 * C]), hd(kvbuf[ki, 2 * C:]), hd(do[qi])
        s = qh @ kh.transpose(1, 2)
        a = s * sc
        m = a.amax(-1, keepdim=True)
        e = torch.exp(a - m)
        l = e.sum(-1, keepdim=True)
        oh = ((rb(e) @ vh) / l)
        o[qi] = back(oh).to(out_dtype)
        L2 = (m * 1.4426950408889634 + torch.log2(l))
        lse2[qi] = L2[..., 0].t()
        if mode == "small":
            p = e / l
        else:
            p = torch.exp2(s * (sc * 1.4426950408889634) - L2)
        dP = gh @ vh.transpose(1, 2)
        if mode == "small":
            D = (p * dP).sum(-1, keepdim=True)
        else:
            oh_st = hd(o[qi])
            if defect == "D_head":
                oh_st = oh_st.roll(1, 0)
            D = (gh * oh_st).sum(-1, keepdim=True)
        dS = (rb(p) if defect == "dS_twice" else p) * (dP - D)
        dq[qi] = back((rb(dS) @ kh) * sc)
        dk.index_add_(0, ki, back(rb(dS).transpose(1, 2) @ qh))
        dv.index_add_(0, ki, back(rb(p).transpose(1, 2) @ gh))
    dk = dk * (1.0 if defect == "dk_scale" else sc)
    return dq.to(out_dtype), dk.to(out_dtype), dv.to(out_dtype), o, lse2


def _self_pairs(T, nb, device="cpu"):
    return [(torch.arange(s * T, (s + 1) * T, device=device),) * 2 for s in range(nb)]


def _temporal_pairs(N, F, HW, device="cpu"):
    return [(n * F * HW + torch.arange(F, device=device) * HW + p,) * 2 for n in range(N) for p in range(HW)]


ATTN_ALL = ([("self", c, "mfma", "bf16") for c in B.SELF_ATTN_BWD + [B.ATTN_AUTOGRAD["spatial"]]] + [("cross", c, "mfma", "bf16") for c in B.CROSS_ATTN_BWD]
            + [("self", (*c, 2), "valu", dt) for c in B.VALU_ATTN_BWD for dt in ("f32", "bf16")]
            + [("temporal", c, "small", dt) for c in B.TEMPORAL_ATTN_BWD for dt in ("f32", "bf16")])


def _attn_setup(kind, c, dt, device="cpu"):
    """(list of (qbuf, kvbuf, do, pairs) calls, heads, C): one call for self / temporal attention, the two directions for cross."""
    if kind == "self":
        T, heads, ch, nb = c
        q, _, do = _attn_inputs(nb * T, 0, heads * ch, DT[dt], 21, device)
        return [(q, q, do, _self_pairs(T, nb, device))], heads, heads * ch
    if kind == "temporal":
        F, HW, heads, ch = c
        q, _, do = _attn_inputs(2 * F * HW, 0, heads * ch, DT[dt], 22, device)
        return [(q, q, do, _temporal_pairs(2, F, HW, device))], heads, heads * ch
    F, HW, L, win, shift, heads, ch = c
    N, C = 2, heads * ch
    vq, aq, dvo = _attn_inputs(N * F * HW, N * L, C, DT[dt], 23, device)
    dao = torch.randn(N * L, C, generator=torch.Generator(device=device).manual_seed(24), device=device).to(DT[dt])
    vp, ap = B.cross_pairs(N, F, HW, L, win, shift, device)
    return [(vq, aq, dvo, vp), (aq, vq, dao, ap)], heads, C


@pytest.mark.parametrize("kind,c,mode,dt", ATTN_ALL, ids=str)
def test_attn_bwd_ref_equals_autograd_and_emulation_has_no_violation(kind, c, mode, dt):
    calls, heads, C = _attn_setup(kind, c, dt)
    for qbuf, kvbuf, do, pairs in calls:
        r = B.attn_bwd_assemble(qbuf, kvbuf, None, do, pairs, heads, mode, F64)
        gq, gk = _autograd_attn(qbuf, kvbuf, do, pairs, heads)
        _close12(r["dq"], gq[:, :C])
        _close12(r["dk"], gk[:, C:2 * C])
        _close12(r["dv"], gk[:, 2 * C:])
        dq, dk, dv, o, lse2 = emulate_attn_bwd(qbuf, kvbuf, do, pairs, heads, mode, DT[dt])
        r = B.attn_bwd_assemble(qbuf, kvbuf, o, do, pairs, heads, mode, DT[dt])
        E.check(lse2, r["lse2"], r["e_lse2"], what="stored lse2")
        B.check_attn_bwd((dq, dk, dv), r, C, f"attention emulation {kind} {c} {mode} {dt}", heads)


def test_cross_case_with_keys_in_no_window():
    """(4, 8, 43, 1, 0): audio positions 40 ... 42 are in no video query's window; with win = 3, shift = 2 the wrap covers them."""
    vp, _ = B.cross_pairs(1, 4, 8, 43, 1, 0)
    assert sorted(set(range(43)) - set(torch.cat([k for _, k in vp]).tolist())) == [40, 41, 42]
    vp, ap = B.cross_pairs(1, 4, 8, 43, 3, 2)
    assert set(torch.cat([k for _, k in vp]).tolist()) == set(range(43)) and [len(q) for q, _ in ap] == [10, 10, 10, 13]


@pytest.mark.parametrize("defect,which", [("D_head", 0), ("dk_scale", 1), ("window_off", 0), ("dS_twice", 0), ("dead_keys", 1)])
def test_attention_seeded_defects_are_flagged(defect, which):
    name = {"D_head": "attention: D from the neighbouring head", "dk_scale": "attention: scale missing from dK",
            "window_off": "attention: window start off by one group", "dS_twice": "attention: dS rounded to bf16 twice",
            "dead_keys": "attention: keys outside every window not zero"}[defect]
    if defect == "dS_twice":
        # two keys, one of them carrying all of K: dQ = scale dS_ij k_j is ONE product, so its bound is the two roundings the kernel is
        # allowed (dS, the store) and a third rounding shows where all three fall the same way; among 2 * 4096 * 64 elements some do
        T, heads, ch, nb = 2, 1, 64, 4096
        q, _, do = _attn_inputs(nb * T, 0, heads * ch, BF, 31)
        q[0::2, ch:2 * ch] = 0
        calls, C = [(q, q, do, _self_pairs(T, nb))], heads * ch
    else:
        kind, c = ("cross", (4, 8, 43, 1, 0, 2, 32)) if defect in ("dead_keys", "window_off") else ("self", (130, 2, 48, 2))
        calls, heads, C = _attn_setup(kind, c, "bf16")
    qbuf, kvbuf, do, pairs = calls[0]
    dq, dk, dv, o, _ = emulate_attn_bwd(qbuf, kvbuf, do, pairs, heads, "mfma", BF, defect=defect)
    r = B.attn_bwd_assemble(qbuf, kvbuf, o, do, pairs, heads, "mfma", BF)
    if defect == "dead_keys":
        dk[r["nq"] == 0] = 0.01                                               # a stale row, small against the live ones
    got, key = (dq, "dq") if which == 0 else (dk, "dk")
    if defect == "dead_keys":
        with pytest.raises(AssertionError):
            B.check_attn_bwd((dq, dk, dv), r, C, defect, heads)
    assert E.violations(got, r[key], r["e_" + key])[0] > 0
    _log(name, got, r[key], BF)


def test_zz_several_defects_pass_the_old_tolerance():
    """Runs last in this file: of the fifteen seeded defects, each flagged element-wise above, at least four stay below the rel-L2
    tolerance of tests/test_bwd_gpu.py."""
    if len(DEFECT_LOG) < 15:                                                  # run on its own: seed the defects here
        for d in ("drop_chunk", "split_twice", "border_wrap", "layout_swap", "db_tail"):
            test_wgrad_seeded_defects_are_flagged(d)
        test_dgrad_unnegated_taps_are_flagged()
        for d, k in (("silu_term", "dx"), ("skip_rows", "dx"), ("m2_count", "dx"), ("film_dgamma", "dgamma")):
            test_gn_seeded_defects_are_flagged(d, k)
        for d, w in (("D_head", 0), ("dk_scale", 1), ("window_off", 0), ("dS_twice", 0), ("dead_keys", 1)):
            test_attention_seeded_defects_are_flagged(d, w)
    assert len(DEFECT_LOG) == 15
    assert sum(1 for _, ok in DEFECT_LOG.values() if ok) >= 4, DEFECT_LOG
