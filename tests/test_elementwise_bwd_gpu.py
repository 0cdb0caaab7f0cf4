"""The backward kernels of the training step against float64, ELEMENT BY ELEMENT (tests/errbound_bwd.py: the references, the bounds and
their derivation, the case lists; tests/test_errbound_bwd_cpu.py: the metric proven on seeded defects).

Every case calls the kernel through mm_diffusion.ops with buffers, strides and layouts of its own, builds the reference with torch
double ops on the STORED operands - never with a libmmd kernel -, and admits ZERO elements outside the per-element bound.  Where the
operation is a plain sum (weight gradient, bias gradient, input gradient, colsum_slices) a second input family on a coarse grid makes
every partial sum exact in fp32, and the assertion is torch.equal: a dropped or doubled row, tap, split or tile, a wrong border
mask or layout index fails with no tolerance at all.  One pass per family goes through the train_ops autograd wrappers.

Worst error / bound ratio per kernel family, as printed by the tests (`-s`) on an MI355X (`cases` = test cases in the group; a record of
headroom, not a tolerance):

    kernel family                                        dtype  cases  worst ratio
    conv_wgrad, DMA 128-tile (wgrad_tr_bf16_kernel)      bf16      22        0.025
    conv_wgrad, wgrad_kernel<float> + colsum             f32       22        0.069
    conv_wgrad, wgrad_kernel<__bf16> + colsum            bf16      16        0.010
    conv_wgrad, wgrad128_bf16_kernel (MMD_WGRAD_TR=0)    bf16      10        0.026
    conv_wgrad, forced 64-tile (MMD_WGRAD_TILE64=1)      bf16      10        0.026
    colsum_slices                                        bf16       2        0.001
    colsum_slices                                        f32        2        0.008
    ConvFn.backward (dX, dW, db)                         bf16       5        0.974
    ConvFn.backward (dX, dW, db)                         f32        5        0.055
    gn_stats a / b / mean / rstd                         bf16      60        0.912
    gn_stats a / b / mean / rstd                         f32       36        0.410
    gn_bwd dx                                            bf16      60        0.995
    gn_bwd dx                                            f32       36        0.195
    gn_bwd dgamma / dbeta / dfilm                        bf16      60        0.319
    gn_bwd dgamma / dbeta / dfilm                        f32       36        0.317
    GroupNormFn.backward                                 bf16       2        0.991
    GroupNormFn.backward                                 f32        1        0.174
    attn_lse stored lse2                                 bf16       7        0.036
    attn_bwd_mfma self                                   bf16       7        0.753
    attn_bwd_mfma cross (both directions)                bf16       7        0.822
    attn_bwd (VALU)                                      f32        2        0.022
    attn_bwd (VALU)                                      bf16       2        0.964
    attn_small_bwd                                       f32        3        0.012
    attn_small_bwd                                       bf16       3        0.979
    SelfAttnFn spatial / temporal, CrossAttnFn           bf16       3        0.978

Every case: zero violating elements; every exact-sum case: bitwise equal.  The weight-gradient ratios are small because the output is
fp32 with no store rounding and the bound grows like M while random rounding errors add like sqrt(M).  The bf16 ratios of 0.96 - 0.995
(dX, GroupNorm dx, the VALU and short attention kernels) are the output-rounding term 2**-8 |ref| used up by elements that land next to a
rounding midpoint; the same happens to the forward's a / b in bf16 mode at Tn = 1, where the whole budget is the fp32 store of the
result (a few u).  The MFMA attention kernels sit at 0.75 - 0.82: their bound carries the worst-case 2**-8 sum |dS| |K| of the bf16 dS /
P operands, which the individual roundings do not fill.  Run time on an MI355X: 4.2 s for the 199 in-process cases, 4.6 s for the
test with the two child processes.

Defect found by this file: ops.gn_bwd cached the kept GroupNorm-backward workspace by its length alone
(test_group_norm_backward_kept_workspaces_of_equal_size); fixed in mm_diffusion/ops.py.
"""
import os
import subprocess
import sys

import pytest
import torch

import errbound as E
import errbound_bwd as B

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DT = {"f32": F32, "bf16": BF}
PAD = 16                  # strided views: the operand sits at column PAD of a buffer 40 columns wider
SENTINEL = 777.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mm_diffusion import ops as o
    return o


@pytest.fixture(scope="module")
def tr():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mm_diffusion import train_ops
    return train_ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _view(t, strided):
    """t itself, or t as a column slice of a wider buffer (ld = C + 40; the neighbours hold 1e4: read by mistake they break every bound)."""
    if not strided:
        return t
    buf = torch.full((t.shape[0], t.shape[1] + 40), 1e4, dtype=t.dtype, device=t.device)
    buf[:, PAD:PAD + t.shape[1]] = t
    return buf[:, PAD:PAD + t.shape[1]]


# --------------------------------------------------------------------------- conv weight / bias gradient
def _wg_inputs(M, Cin, Cout, dt, seed, exact):
    g = _gen(seed)
    if exact:
        return B.grid_randn((M, Cout), g, "cuda").to(dt), B.grid_randn((M, Cin), g, "cuda").to(dt)
    return torch.randn(M, Cout, device="cuda", generator=g).to(dt), torch.randn(M, Cin, device="cuda", generator=g).to(dt)


def _launch_wgrad(ops, dy, x, taps, dims, with_db, torch_layout, strided):
    Cout, Cin, nt = dy.shape[1], x.shape[1], len(taps)
    dW = torch.zeros(Cout, nt * Cin, dtype=F32, device="cuda")
    db = torch.zeros(Cout, dtype=F32, device="cuda") if with_db else None
    ops.conv_wgrad(_view(dy, strided), _view(x, strided), dW, db, taps, dims, torch_layout=torch_layout)
    return dW, db


def _wgrad_all_variants(ops, name, M, Cin, Cout, taps, dims, dt):
    """Random inputs against the bound: (db, packed, contiguous) and (no db, torch layout, column slices); exact-sum inputs bitwise:
    (db, torch layout, column slices) and (no db, packed, contiguous).  Returns the worst error / bound ratio."""
    nt = len(taps)
    assert B.exact_sum_ok(M)
    dy, x = _wg_inputs(M, Cin, Cout, dt, 300 + M + Cin, False)
    dW, S, db, Sb = B.wgrad_ref(dy, x, taps, dims)
    bound = B.wgrad_bound(S, M, dt)
    got, gdb = _launch_wgrad(ops, dy, x, taps, dims, True, False, False)
    worst = B.check_groups(got, dW, bound, Cin, "tap", f"{name} dW packed")
    worst = max(worst, E.check(gdb[None], db[None], B.colsum_bound(Sb, M)[None], what=f"{name} db"))
    got, _ = _launch_wgrad(ops, dy, x, taps, dims, False, True, True)
    worst = max(worst, E.check(got, B.to_torch_layout(dW, Cin, nt), B.to_torch_layout(bound, Cin, nt), what=f"{name} dW torch layout, strided"))
    dy, x = _wg_inputs(M, Cin, Cout, dt, 400 + M + Cin, True)
    dW, _, db, _ = B.wgrad_ref(dy, x, taps, dims)
    got, gdb = _launch_wgrad(ops, dy, x, taps, dims, True, True, True)
    assert torch.equal(got, B.to_torch_layout(dW, Cin, nt).float()), f"{name}: exact-sum dW (torch layout, strided) differs in {int((got != B.to_torch_layout(dW, Cin, nt).float()).sum())} elements"
    assert torch.equal(gdb, db.float()), f"{name}: exact-sum db differs"
    got, _ = _launch_wgrad(ops, dy, x, taps, dims, False, False, False)
    bad = got != dW.float()
    assert not bool(bad.any()), f"{name}: exact-sum dW (packed) differs in {int(bad.sum())} elements, by tap: {E._hist(torch.nonzero(bad)[:, 1].cpu() // Cin, nt)}"
    return worst


WG = [(c, ch, dt) for c in B.wgrad_cases() for ch in c["chans"] for dt in ("bf16", "f32")]


@pytest.mark.parametrize("case,chans,dt", WG, ids=[f"{c['name']}-{ci}-{co}-{dt}" for c, (ci, co), dt in WG])
def test_conv_wgrad_elementwise(ops, case, chans, dt):
    """bf16: the DMA-staged 128-tile (wgrad_tr_bf16_kernel) on the split plan the case was built for; fp32: wgrad_kernel<float> + colsum."""
    Cin, Cout = chans
    plan = B.wgrad_plan(case["M"], Cin, Cout, len(case["taps"]), dt == "bf16")
    if dt == "bf16":
        assert plan == ("tr",) + case["plan"], f"the launcher's cost model moved {case['name']} off its path: {plan}"
    else:
        assert plan[0] == "64"
    r = _wgrad_all_variants(ops, case["name"], case["M"], Cin, Cout, case["taps"], case["dims"], DT[dt])
    print(f"\nRATIO wgrad {'tr128' if dt == 'bf16' else 'tile64'} {case['name']} {Cin}->{Cout} {dt} splits={plan[1]} xcd={plan[3]}: {r:.3f}")


WG64 = [(c["name"], ch) for c, ch in B.wgrad64_bf16_cases()]


@pytest.mark.parametrize("geom,chans", WG64, ids=[f"{g}-{ci}-{co}" for g, (ci, co) in WG64])
def test_conv_wgrad_tile64_bf16_elementwise(ops, geom, chans):
    """wgrad_kernel<__bf16> (Cin < 64 or Cout < 64: the input and output convs) with the colsum launch; Cout = 2056: two colsum slabs."""
    case = next(c for c in B.wgrad_cases() if c["name"] == geom)
    Cin, Cout = chans
    assert B.wgrad_plan(case["M"], Cin, Cout, len(case["taps"]), True)[0] == "64"
    r = _wgrad_all_variants(ops, geom, case["M"], Cin, Cout, case["taps"], case["dims"], BF)
    print(f"\nRATIO wgrad tile64 {geom} {Cin}->{Cout} bf16: {r:.3f}")


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import errbound as E, errbound_bwd as B
from mm_diffusion import ops
worst = 0.0
for name in B.WGRAD_CHILD_GEOMS:
    c = next(k for k in B.wgrad_cases() if k["name"] == name)
    M, taps, dims, nt = c["M"], c["taps"], c["dims"], len(c["taps"])
    for Cin, Cout in c["chans"][:2]:
        for exact in (False, True):
            g = torch.Generator(device="cuda").manual_seed(500 + M + Cin)
            mk = (lambda s: B.grid_randn(s, g, "cuda")) if exact else (lambda s: torch.randn(*s, device="cuda", generator=g))
            dy, x = mk((M, Cout)).to(torch.bfloat16), mk((M, Cin)).to(torch.bfloat16)
            dW, S, db, Sb = B.wgrad_ref(dy, x, taps, dims)
            got, gdb = torch.zeros(Cout, nt * Cin, device="cuda"), torch.zeros(Cout, device="cuda")
            ops.conv_wgrad(dy, x, got, gdb, taps, dims, torch_layout=exact)
            if exact:
                assert torch.equal(got, B.to_torch_layout(dW, Cin, nt).float()) and torch.equal(gdb, db.float()), (name, Cin, Cout, "exact sums differ")
            else:
                worst = max(worst, B.check_groups(got, dW, B.wgrad_bound(S, M, torch.bfloat16), Cin, "tap", f"{name} {Cin}->{Cout}"),
                            E.check(gdb[None], db[None], B.colsum_bound(Sb, M)[None], what=f"{name} db"))
print(f"CHILD-OK worst ratio {worst:.3f}")
"""


def test_conv_wgrad_switched_kernels_in_child_processes(tmp_path):
    """wgrad128_bf16_kernel (MMD_WGRAD_TR=0) and the forced 64-tile (MMD_WGRAD_TILE64=1) on the same small case list: the switches
    are read once per process, so each arm runs in a fresh interpreter, one after the other, each under its own time limit.  An arm
    that ends on a signal or runs into the limit fails the test before the next one starts."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "wgrad_arm.py"
    script.write_text(_CHILD)
    for var in ("MMD_WGRAD_TR=0", "MMD_WGRAD_TILE64=1"):
        k, v = var.split("=")
        env = {e: val for e, val in os.environ.items() if e not in ("MMD_WGRAD_TR", "MMD_WGRAD_TILE64", "MMD_WGRAD_BLOCKS")}
        env[k] = v
        p = subprocess.run([sys.executable, str(script), here, os.path.join(os.path.dirname(here), "mm-diffusion_amd")], env=env, timeout=240,
                           capture_output=True, text=True)
        assert p.returncode == 0 and "CHILD-OK" in p.stdout, f"{var}: exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        print(f"\nRATIO wgrad child {var}: {p.stdout.strip().splitlines()[-1]}")


@pytest.mark.parametrize("S,Tn,C,dt", B.COLSUM_SLICES)
def test_colsum_slices_elementwise(ops, S, Tn, C, dt):
    g = _gen(31)
    for exact in (False, True):
        dy = (B.grid_randn((S * Tn, C), g, "cuda") if exact else torch.randn(S * Tn, C, device="cuda", generator=g)).to(DT[dt])
        view = _view(dy, True)
        out = torch.zeros(S, C + 8, dtype=F32, device="cuda")
        ops.colsum_slices(view, out[:, :C], Tn)
        d3 = dy.double().reshape(S, Tn, C)
        ref, Sb = d3.sum(1), d3.abs().sum(1)
        assert bool((out[:, C:] == 0).all()), "columns past C written"
        if exact:
            assert B.exact_sum_ok(Tn) and torch.equal(out[:, :C], ref.float())
        else:
            r = E.check(out[:, :C], ref, B.colsum_bound(Sb, Tn), what="colsum_slices")
            print(f"\nRATIO colsum_slices S={S} Tn={Tn} C={C} {dt}: {r:.3f}")


# --------------------------------------------------------------------------- conv input gradient and the autograd wrapper
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("geom,Cin,Cout", B.DGRAD)
def test_conv_backward_through_autograd(ops, tr, geom, Cin, Cout, dt):
    """ConvFn.backward: dX = conv_gemm(dY, W^T, mirrored taps) against conv_rows_ref on operands the TEST transposes and mirrors; the
    residual gradient is dY itself; dW / db through both wrapper paths (returned tensors; accumulated straight into preallocated .grad
    in the parameter's layout); a frozen-weight call returns dX and the residual gradient only."""
    case = next(c for c in B.wgrad_cases() if c["name"] == geom)
    M, taps, dims, nt = case["M"], case["taps"], case["dims"], len(case["taps"])
    kshape = {1: (1,), 3: (3,), 9: (3, 3)}[nt]
    assert B.exact_sum_ok(nt * Cout) and B.exact_sum_ok(M)
    for exact in (False, True):
        g = _gen(40 + M)
        mk = (lambda *s: B.grid_randn(s, g, "cuda")) if exact else (lambda *s: torch.randn(*s, device="cuda", generator=g))
        x, dy, res = mk(M, Cin).to(DT[dt]), mk(M, Cout).to(DT[dt]), mk(M, Cout).to(DT[dt])
        w = (mk(Cout, Cin, nt) * (1.0 if exact else (nt * Cout) ** -0.5)).to(DT[dt]).float()        # fp32 parameter holding values of the compute type
        bias = mk(Cout).float()
        wt, ntaps = B.dgrad_operands(w.to(DT[dt]), taps)
        ref_dx, S_dx = E.conv_rows_ref(dy, wt, None, None, ntaps, dims)
        dW, S, db, Sb = B.wgrad_ref(dy, x, taps, dims)
        dW_t, bound_t = B.to_torch_layout(dW, Cin, nt), B.to_torch_layout(B.wgrad_bound(S, M, DT[dt]), Cin, nt)

        def run(frozen, slot):
            xd, rd = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
            wd, bd = w.reshape(Cout, Cin, *kshape).clone().requires_grad_(not frozen), bias.clone().requires_grad_(not frozen)
            if slot:
                wd.grad, bd.grad = torch.zeros_like(wd), torch.zeros_like(bd)
            tr.conv(xd, wd, bd, taps=taps, dims=dims, residual=rd).backward(dy)
            return xd.grad, rd.grad, wd.grad, bd.grad

        worst = 0.0
        for frozen, slot in ((False, False), (False, True), (True, False)):
            gx, gr, gw, gb = run(frozen, slot)
            what = f"{geom} {dt} frozen={frozen} slot={slot} exact={exact}"
            assert torch.equal(gr, dy), what + ": the residual gradient is dY"
            if frozen:
                assert gw is None and gb is None
            if exact:
                assert torch.equal(gx, ref_dx.float().to(DT[dt])), what + ": dX"
                if not frozen:
                    assert torch.equal(gw.reshape(Cout, -1), dW_t.float()) and torch.equal(gb, db.float()), what + ": dW / db"
            else:
                worst = max(worst, E.check(gx, ref_dx, E.gemm_bound(ref_dx, S_dx, nt * Cout, DT[dt]), what=what + ": dX"))
                if not frozen:
                    worst = max(worst, E.check(gw.reshape(Cout, -1), dW_t, bound_t, what=what + ": dW"),
                                E.check(gb[None], db[None], B.colsum_bound(Sb, M)[None], what=what + ": db"))
        if not exact:
            print(f"\nRATIO conv autograd {geom} {Cin}->{Cout} {dt}: {worst:.3f}")


# --------------------------------------------------------------------------- GroupNorm
def _gn_inputs(dt, C, kind, Tn, big, seed=11):
    N, HW = 2, 3
    g = _gen(seed + C + Tn)
    slices, geom = B.gn_slices(kind, N, Tn, HW)
    rows = slices.numel()
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    x = (rn(rows, C) * (1.0 if big else 1.5) + (20.0 if big else 0.3)).to(DT[dt])
    dy = rn(rows, C).to(DT[dt])
    gamma, beta = 1 + 0.1 * rn(C), rn(C)
    film = rn(geom[0], 2 * C) * 0.3 if kind == "per_sample_film" else None
    return x, dy, gamma, beta, film, kind.startswith("per_sample"), slices, geom


@pytest.mark.parametrize("dt,C,kind,Tn,big", B.gn_cases(), ids=str)
def test_group_norm_backward_elementwise(ops, monkeypatch, dt, C, kind, Tn, big):
    """gn_stats's a, b, mean, rstd against float64 first; then gn_bwd through the per-call workspace entry and twice through the
    kept-workspace entry (one workspace: the second call proves the parameter stage left it zero)."""
    x, dy, gamma, beta, film, act, slices, geom = _gn_inputs(dt, C, kind, Tn, big)
    geom = ops.Geom(*geom)
    S = geom.S
    mr = torch.empty(S, 32, 2, dtype=F32, device="cuda")
    a, b = ops.gn_stats(x, gamma, beta, geom, film=film, mr=mr)
    stored = (a, b, mr[..., 0], mr[..., 1])
    r = B.gn_bwd_ref(x, dy, gamma, beta, film, act, slices, stored=stored, out_dtype=DT[dt])
    worst = {}
    for ws0 in (False, True, True):
        monkeypatch.setattr(ops, "_GN_BWD_WS0", ws0)
        dx = torch.full_like(x, float("nan"))
        dgamma, dbeta = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        dfilm = None if film is None else torch.full((S, 2 * C), float("nan"), device="cuda")
        ops.gn_bwd(x, dy, dx, geom, a, b, mr, gamma, beta, film, act, dgamma, dbeta, dfilm)
        got = dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dfilm=dfilm, a=a, b=b, mean=stored[2], rstd=stored[3])
        w = B.check_gn(got, r, f"GroupNorm {dt} C={C} {kind} Tn={Tn} big={big} ws0={ws0}")
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    print(f"\nRATIO gn {dt} C={C} {kind} Tn={Tn} big={int(big)}: fwd {max(worst[k] for k in ('a', 'b', 'mean', 'rstd')):.3f} dx {worst['dx']:.3f} "
          f"params {max(v for k, v in worst.items() if k in ('dgamma', 'dbeta', 'dfilm')):.3f}")


def test_group_norm_backward_kept_workspaces_of_equal_size(ops, monkeypatch):
    """Two norms whose workspaces have the same length but another split: S = 6, C = 32 and S = 2, C = 160 are both S (2 C + 64) = 768
    floats, accumulators in the first 384 / 640 of them.  The first call leaves its group means at [384, 768); a cache keyed by the
    length alone handed that buffer to the second call as 'zero on entry' (found by this file: slice 1, channels >= 32 of dx wrong by
    1e-2 ... 1e-1).  In this order, in one test, whatever ran before."""
    monkeypatch.setattr(ops, "_GN_BWD_WS0", True)
    for dt, C, kind, Tn in (("bf16", 32, "temporal", 7), ("bf16", 160, "per_sample", 7)):
        x, dy, gamma, beta, film, act, slices, geom = _gn_inputs(dt, C, kind, Tn, False, seed=13)
        geom = ops.Geom(*geom)
        assert geom.S * (2 * C + 64) == 768
        mr = torch.empty(geom.S, 32, 2, dtype=F32, device="cuda")
        a, b = ops.gn_stats(x, gamma, beta, geom, film=film, mr=mr)
        r = B.gn_bwd_ref(x, dy, gamma, beta, film, act, slices, stored=(a, b, mr[..., 0], mr[..., 1]), out_dtype=DT[dt])
        dx = torch.full_like(x, float("nan"))
        dgamma, dbeta = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        ops.gn_bwd(x, dy, dx, geom, a, b, mr, gamma, beta, film, act, dgamma, dbeta, None)
        B.check_gn(dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dfilm=None, a=a, b=b, mean=mr[..., 0], rstd=mr[..., 1]), r, f"kept workspace S={geom.S} C={C}")


@pytest.mark.parametrize("dt,C,kind,Tn", B.GN_AUTOGRAD)
def test_group_norm_backward_through_autograd(ops, tr, dt, C, kind, Tn):
    x, dy, gamma, beta, film, act, slices, geom = _gn_inputs(dt, C, kind, Tn, False, seed=12)
    geom = ops.Geom(*geom)
    mr = torch.empty(geom.S, 32, 2, dtype=F32, device="cuda")
    a, b = ops.gn_stats(x, gamma, beta, geom, film=film, mr=mr)
    r = B.gn_bwd_ref(x, dy, gamma, beta, film, act, slices, stored=(a, b, mr[..., 0], mr[..., 1]), out_dtype=DT[dt])
    xd, gd, bd = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    fd = None if film is None else film.clone().requires_grad_(True)
    tr.group_norm(xd, gd, bd, geom, act, film=fd).backward(dy)
    got = dict(dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad, dfilm=None if fd is None else fd.grad, a=a, b=b, mean=mr[..., 0], rstd=mr[..., 1])
    w = B.check_gn(got, r, f"GroupNorm autograd {dt} C={C} {kind} Tn={Tn}")
    print(f"\nRATIO gn autograd {dt} C={C} {kind} Tn={Tn}: {max(w.values()):.3f}")


# --------------------------------------------------------------------------- attention
def _rand(rows, cols, dt, seed):
    return torch.randn(rows, cols, device="cuda", generator=_gen(seed)).to(dt)


def _grad_buffer(rows, C3, dt):
    """A [rows, 3C] gradient view at column 8 of a sentinel-filled buffer 16 columns wider."""
    buf = torch.full((rows, C3 + 16), SENTINEL, dtype=dt, device="cuda")
    return buf, buf[:, 8:8 + C3]


def _guards_intact(buf, C3, what):
    assert bool((buf[:, :8] == SENTINEL).all()) and bool((buf[:, 8 + C3:] == SENTINEL).all()), what + ": columns outside the gradient ranges written"


def _written(t, what):
    assert not bool((t == SENTINEL).any()), what + ": rows or columns left unwritten"


def _self_pairs(T, nb):
    return [(torch.arange(s * T, (s + 1) * T, device="cuda"),) * 2 for s in range(nb)]


@pytest.mark.parametrize("T,heads,ch,nb", B.SELF_ATTN_BWD)
def test_self_attention_backward_mfma_elementwise(ops, T, heads, ch, nb):
    """attn_bwd_mfma after attn_lse.  ch = 16 / 48: the zero-padded transposed tile; 192: the two-half dK / dV kernel; T = 257: three
    query tiles; heads * nb = 8 with two tiles: the remapped block order."""
    C = heads * ch
    rows = nb * T
    qkv, do = _rand(rows, 3 * C, BF, 51), _rand(rows, C, BF, 52)
    out = torch.full((rows, C), float("nan"), dtype=BF, device="cuda")
    lse = torch.full((rows * heads,), float("nan"), dtype=F32, device="cuda")
    ops.attn_lse(qkv, qkv, out, lse, heads, ch, nb, 1, T, T, T, T, 1)
    buf, dqkv = _grad_buffer(rows, 3 * C, BF)
    ops.attn_bwd_mfma(qkv, qkv, out, do, dqkv, 0, dqkv, C, 2 * C, lse, heads, ch, nb, 1, T, T, T, T, 1)
    what = f"self-attention backward MFMA T={T} h={heads} ch={ch} nb={nb}"
    _guards_intact(buf, 3 * C, what)
    _written(dqkv, what)
    r = B.attn_bwd_assemble(qkv, qkv, out, do, _self_pairs(T, nb), heads, "mfma", BF)
    rl = E.check(lse.reshape(rows, heads), r["lse2"], r["e_lse2"], what=what + ": stored lse2")
    w = B.check_attn_bwd((dqkv[:, :C], dqkv[:, C:2 * C], dqkv[:, 2 * C:]), r, C, what, heads)
    print(f"\nRATIO attn bwd mfma self T={T} h={heads} ch={ch} nb={nb}: {w:.3f} (lse2 {rl:.3f})")


@pytest.mark.parametrize("F,HW,L,win,shift,heads,ch", B.CROSS_ATTN_BWD)
def test_cross_attention_backward_mfma_elementwise(ops, F, HW, L, win, shift, heads, ch):
    """Both directions, each into its own column ranges of the two gradient buffers: after the first call the ranges of the second are
    still untouched.  (4, 8, 43, ...): the last audio group has 13 queries; with win = 1, shift = 0 the audio positions 40 ... 42 are
    in no window and their dK / dV are exactly zero."""
    N, C = 2, heads * ch
    apf = L // F
    vq, aq = _rand(N * F * HW, 3 * C, BF, 53), _rand(N * L, 3 * C, BF, 54)
    dvo, dao = _rand(N * F * HW, C, BF, 55), _rand(N * L, C, BF, 56)
    sh = torch.tensor([shift], dtype=torch.int32, device="cuda")
    vo = torch.full((N * F * HW, C), float("nan"), dtype=BF, device="cuda")
    ao = torch.full((N * L, C), float("nan"), dtype=BF, device="cuda")
    vl = torch.full((N * F * HW * heads,), float("nan"), dtype=F32, device="cuda")
    al = torch.full((N * L * heads,), float("nan"), dtype=F32, device="cuda")
    ops.attn_lse(vq, aq, vo, vl, heads, ch, N, F, F * HW, HW, L, apf, win, shift_dev=sh)
    ops.attn_lse(aq, vq, ao, al, heads, ch, N, F, L, apf, F * HW, HW, win, shift_dev=sh)
    vbuf, dv = _grad_buffer(N * F * HW, 3 * C, BF)
    abuf, da = _grad_buffer(N * L, 3 * C, BF)
    what = f"cross-attention backward MFMA F={F} HW={HW} L={L} win={win} shift={shift} h={heads} ch={ch}"
    ops.attn_bwd_mfma(vq, aq, vo, dvo, dv, 0, da, C, 2 * C, vl, heads, ch, N, F, F * HW, HW, L, apf, win, shift_dev=sh)
    assert bool((dv[:, C:] == SENTINEL).all()) and bool((da[:, :C] == SENTINEL).all()), what + ": the other direction's columns written"
    ops.attn_bwd_mfma(aq, vq, ao, dao, da, 0, dv, C, 2 * C, al, heads, ch, N, F, L, apf, F * HW, HW, win, shift_dev=sh)
    for buf, t in ((vbuf, dv), (abuf, da)):
        _guards_intact(buf, 3 * C, what)
        _written(t, what)
    vp, ap = B.cross_pairs(N, F, HW, L, win, shift, "cuda")
    rv = B.attn_bwd_assemble(vq, aq, vo, dvo, vp, heads, "mfma", BF)
    ra = B.attn_bwd_assemble(aq, vq, ao, dao, ap, heads, "mfma", BF)
    E.check(vl.reshape(-1, heads), rv["lse2"], rv["e_lse2"], what=what + ": stored lse2 (video)")
    E.check(al.reshape(-1, heads), ra["lse2"], ra["e_lse2"], what=what + ": stored lse2 (audio)")
    if (win, shift) == (1, 0) and L == 43:
        assert int((rv["nq"] == 0).sum()) == 3 * N
    w = max(B.check_attn_bwd((dv[:, :C], da[:, C:2 * C], da[:, 2 * C:]), rv, C, what + " video <- audio", heads),
            B.check_attn_bwd((da[:, :C], dv[:, C:2 * C], dv[:, 2 * C:]), ra, C, what + " audio <- video", heads))
    print(f"\nRATIO attn bwd mfma cross F={F} HW={HW} L={L} win={win} shift={shift} h={heads} ch={ch}: {w:.3f}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("T,heads,ch", B.VALU_ATTN_BWD)
def test_attention_backward_valu_elementwise(ops, T, heads, ch, dt):
    """mmd_attn_bwd (fp32 math on LDS tiles): P and dS stay in fp32, D from the stored forward output.  ch = 24 is no MFMA head width."""
    nb, C = 2, heads * ch
    rows = nb * T
    qkv, do = _rand(rows, 3 * C, DT[dt], 57), _rand(rows, C, DT[dt], 58)
    out = torch.full((rows, C), float("nan"), dtype=DT[dt], device="cuda")
    ops.attn(qkv, qkv, out, heads, ch, nb, 1, T, T, T, T, 1)
    buf, dqkv = _grad_buffer(rows, 3 * C, DT[dt])
    geo = (1, T, 1, 1)
    ops.attn_bwd(qkv, 0, qkv, C, 2 * C, out, do, dqkv, 0, dqkv, C, 2 * C, heads, ch, nb, 1, geo, T, T, geo, T, T, 1, None)
    what = f"attention backward VALU T={T} h={heads} ch={ch} {dt}"
    _guards_intact(buf, 3 * C, what)
    _written(dqkv, what)
    r = B.attn_bwd_assemble(qkv, qkv, out, do, _self_pairs(T, nb), heads, "valu", DT[dt])
    w = B.check_attn_bwd((dqkv[:, :C], dqkv[:, C:2 * C], dqkv[:, 2 * C:]), r, C, what, heads)
    print(f"\nRATIO attn bwd valu T={T} h={heads} ch={ch} {dt}: {w:.3f}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("F,HW,heads,ch", B.TEMPORAL_ATTN_BWD)
def test_temporal_attention_backward_elementwise(ops, F, HW, heads, ch, dt):
    """attn_small_bwd: one wave per (pixel, head), rows strided by HW; softmax and D = sum_j P_j dP_j in the kernel, all in fp32."""
    N, C = 2, heads * ch
    rows = N * F * HW
    qkv, do = _rand(rows, 3 * C, DT[dt], 59), _rand(rows, C, DT[dt], 60)
    buf, dqkv = _grad_buffer(rows, 3 * C, DT[dt])
    ops.attn_small_bwd(qkv, do, dqkv, C, heads, ops.Geom.temporal(N, F, HW))
    what = f"temporal attention backward F={F} HW={HW} h={heads} ch={ch} {dt}"
    _guards_intact(buf, 3 * C, what)
    _written(dqkv, what)
    pairs = [(n * F * HW + torch.arange(F, device="cuda") * HW + p,) * 2 for n in range(N) for p in range(HW)]
    r = B.attn_bwd_assemble(qkv, qkv, None, do, pairs, heads, "small", DT[dt])
    w = B.check_attn_bwd((dqkv[:, :C], dqkv[:, C:2 * C], dqkv[:, 2 * C:]), r, C, what, heads)
    print(f"\nRATIO attn bwd small F={F} HW={HW} h={heads} ch={ch} {dt}: {w:.3f}")


def test_attention_backward_through_autograd(ops, tr):
    """SelfAttnFn (spatial: MFMA; temporal: attn_small_bwd) and CrossAttnFn in bf16: the wrappers' column offsets and geometries."""
    HW, heads, ch, NF = B.ATTN_AUTOGRAD["spatial"]
    C = heads * ch
    N, F = 2, NF // 2
    qkv, do = _rand(N * F * HW, 3 * C, BF, 61), _rand(N * F * HW, C, BF, 62)
    qd = qkv.clone().requires_grad_(True)
    od = tr.SelfAttnFn.apply(qd, heads, "spatial", N, F, HW)
    od.backward(do)
    r = B.attn_bwd_assemble(qkv, qkv, od.detach(), do, _self_pairs(HW, N * F), heads, "mfma", BF)
    w1 = B.check_attn_bwd((qd.grad[:, :C], qd.grad[:, C:2 * C], qd.grad[:, 2 * C:]), r, C, "SelfAttnFn spatial", heads)
    F, HW = B.ATTN_AUTOGRAD["temporal"][:2]
    assert B.ATTN_AUTOGRAD["temporal"][2:] == (heads, ch)
    qkv, do = _rand(N * F * HW, 3 * C, BF, 63), _rand(N * F * HW, C, BF, 64)
    qd = qkv.clone().requires_grad_(True)
    tr.SelfAttnFn.apply(qd, heads, "temporal", N, F, HW).backward(do)
    pairs = [(n * F * HW + torch.arange(F, device="cuda") * HW + p,) * 2 for n in range(N) for p in range(HW)]
    r = B.attn_bwd_assemble(qkv, qkv, None, do, pairs, heads, "small", BF)
    w2 = B.check_attn_bwd((qd.grad[:, :C], qd.grad[:, C:2 * C], qd.grad[:, 2 * C:]), r, C, "SelfAttnFn temporal", heads)
    F, HW, L, win, shift = B.ATTN_AUTOGRAD["cross"][:5]
    assert B.ATTN_AUTOGRAD["cross"][5:] == (heads, ch)
    vq, aq = _rand(N * F * HW, 3 * C, BF, 65), _rand(N * L, 3 * C, BF, 66)
    dvo, dao = _rand(N * F * HW, C, BF, 67), _rand(N * L, C, BF, 68)
    vd, ad = vq.clone().requires_grad_(True), aq.clone().requires_grad_(True)
    vo, ao = tr.CrossAttnFn.apply(vd, ad, heads, N, F, HW, L, win, shift)
    torch.autograd.backward([vo, ao], [dvo, dao])
    vp, ap = B.cross_pairs(N, F, HW, L, win, shift, "cuda")
    rv = B.attn_bwd_assemble(vq, aq, vo.detach(), dvo, vp, heads, "mfma", BF)
    ra = B.attn_bwd_assemble(aq, vq, ao.detach(), dao, ap, heads, "mfma", BF)
    w3 = max(B.check_attn_bwd((vd.grad[:, :C], ad.grad[:, C:2 * C], ad.grad[:, 2 * C:]), rv, C, "CrossAttnFn video <- audio", heads),
             B.check_attn_bwd((ad.grad[:, :C], vd.grad[:, C:2 * C], vd.grad[:, 2 * C:]), ra, C, "CrossAttnFn audio <- video", heads))
    print(f"\nRATIO attn autograd spatial {w1:.3f} temporal {w2:.3f} cross {w3:.3f}")
