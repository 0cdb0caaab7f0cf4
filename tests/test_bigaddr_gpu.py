"""The strided kernels at address ranges past 2 GiB and 4 GiB (tests/bigaddr.py: the limits table, the placement model, the arena).

Every case is an EXISTING small case of the element-wise suites; only the row stride of its operands grows, so that the operand's
byte extent passes 2**31 (placement B) or 2**32 (placement C) - A is the control below 2**31.  All operands are views of one arena
filled with a non-finite pattern; after the launch the outputs are copied out, the inputs are compared with what was copied in, the
pattern is written back over both, and the WHOLE arena must be the pattern again (exact stray-write check).  Judged per placement:
the element-wise float64 bound of the case's own suite (unchanged), bitwise equality with the compact contiguous run wherever the
launch label is the same (it always is: bigaddr.LABEL_MAY_DIFFER is empty), records and lse like Y.  Where the limits table says the
entry refuses, the C call must return its error by name with nothing written, the Python predicate must be False, and the path the
engine takes instead must compute the case within its bound.

Worst error / bound ratio per family over all placements, as printed (`-s`, lines `RATIO bigaddr ...`) on an MI355X:

    family                                        placed runs   worst ratio
    GEMM tiles, Y                                         393         0.990
    GEMM tiles, statistics records                          -         0.010
    GroupNorm, row bias, resample, copies,                225         0.999
      short attention (wide ld)
    the same kernels, wide outer_stride / tstride          78         0.994
    fused convs, stem, head                                63         0.994
    backward                                              171         0.984
    attention forward (O and lse2)                        117         0.944

(0.99 on Y: the bf16 output rounding uses its whole half ulp, as in tests/test_elementwise_gpu.py; add_rowbias in fp32 is one rounded
add against a bound of one ulp.)  Every placed output of a launch that was not refused is bitwise the compact output, except the
sums of fp32 atomics (bigaddr.atomic_sums), which meet the bound and, on exact-sum inputs, the exact sums.

Peak arena: 11 GiB (bf16 cases), 16 GiB + 1 MiB (fp32 cases), never both at once.
"""
from unittest import mock

import pytest
import torch

import bigaddr as B
import errbound as E
import errbound_fwd as EF

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f32": torch.float32}
TAPS = {"1": E.TAPS_1, "9": E.TAPS_SPATIAL, "t3": E.TAPS_TEMPORAL}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mm_diffusion import ops as o
    return o


@pytest.fixture(scope="module")
def arena_of():
    """get(es): the arena of that element size.  One is alive at a time; it is deleted (and the cache emptied) when another size is
    asked for and when the module ends."""
    held = {}

    def drop():
        held.clear()
        torch.cuda.empty_cache()

    def get(es):
        if es not in held:
            drop()
            free, _ = torch.cuda.mem_get_info()
            if free < B.ARENA_BYTES[es] + 2 * B.GIB:
                pytest.skip(f"{free / B.GIB:.1f} GiB free: the {B.ARENA_BYTES[es] / B.GIB:.1f} GiB arena plus 2 GiB does not fit")
            held[es] = B.Arena(es)
        return held[es]

    yield get
    drop()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _as_rec(t):
    """[rows, 2 Q] fp32 view -> the [rows, Q, 2] record view ops takes."""
    return torch.as_strided(t, (t.shape[0], t.shape[1] // 2, 2), (t.stride(0), 2, 1), t.storage_offset())


class Placed:
    """The operands of one run as views of the arena: inputs copied in, outputs left as the pattern.  finish() copies the outputs out,
    proves the inputs untouched, restores the pattern and checks the whole arena."""

    def __init__(self, arena, operands, wide, placement, inputs, dtypes, inout=(), views=None):
        self.arena, self.inputs, self.inout = arena, inputs, set(inout)
        self.views = B.layout(operands, wide, placement, arena.es) if views is None else views
        assert B.arena_need(self.views, arena.es) <= arena.nbytes
        self.t = {n: arena.tensor(v, dtypes[n]) for n, v in self.views.items()}
        for n, src in inputs.items():
            self.t[n].copy_(src)

    def finish(self, what):
        torch.cuda.synchronize()
        outs = {n: t.clone() for n, t in self.t.items() if n not in self.inputs or n in self.inout}
        try:
            for n, src in self.inputs.items():
                assert n in self.inout or _same_bits(self.t[n], src), f"{what}: input {n} was written"
            for v in self.views.values():
                self.arena.repattern(v)
            n, where = self.arena.dirty()
            assert n == 0, f"{what}: {n} words of the arena outside the operands were written, first at byte offsets {where}"
        except AssertionError:
            self.arena.fill()
            raise
        return outs

    def untouched(self, what):
        """After a refused call: the inputs are what was copied in and nothing else differs from the pattern (the inputs are put back
        for the run that follows)."""
        torch.cuda.synchronize()
        try:
            for n, src in self.inputs.items():
                assert _same_bits(self.t[n], src), f"{what}: a refused call wrote input {n}"
                self.arena.repattern(self.views[n])
            n, where = self.arena.dirty()
            assert n == 0, f"{what}: a refused call wrote {n} words, first at byte offsets {where}"
        except AssertionError:
            self.arena.fill()
            raise
        for n, src in self.inputs.items():
            self.t[n].copy_(src)


def _record(ops, fn):
    """Record fn()'s launches instead of running them: (plan, labels)."""
    plan = []
    with ops.recording(plan):
        fn()
    return plan, [e[3][0] for e in plan]


def _rc(ops, plan):
    """Run a recorded plan entry by entry on the current stream: the first non-zero return code (0: every call enqueued)."""
    from mm_diffusion import _hip as H
    for fn, args, *_ in plan:
        rc = fn(*args, H.stream_handle())
        if rc != 0:
            return rc, H.lib().mmd_last_error().decode()
    return 0, ""


def test_arena_check_sees_one_stray_word(arena_of):
    """The stray-write check is exact: one 16-bit cell anywhere - the first word, the last, a cell next to an operand's row - is seen."""
    arena = arena_of(2)
    assert arena.dirty() == (0, [])
    cells = arena.buf.view(torch.int16)
    for off in (0, B.BASE[2] - 2, B.BASE[2] + 3 * B.GIB + 4098, arena.nbytes - 2):
        cells[off // 2] = 0
        n, where = arena.dirty()
        assert n == 1 and where == [off // 4 * 4], (off, n, where)
        cells[off // 2] = B.PATTERN16
    assert arena.dirty() == (0, [])


# ------------------------------------------------------------------------------------------------- GEMM tiles
def _gemm_inputs(ops, c):
    """Compact operands of a case (seeded), the weights / biases / fused affine, and the float64 reference with its bound."""
    dt, M, Cin, Cout = DT[c["dt"]], c["M"], c["Cin"], c["Cout"]
    taps = TAPS[c["taps"]]
    g = torch.Generator(device="cuda").manual_seed(1000 + M + Cin + Cout)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x = (rnd(M, Cin) * (1.4 if c["gn"] else 1.0) + (0.3 if c["gn"] else 0.0)).to(dt)
    w = (rnd(Cout, len(taps) * Cin) * (len(taps) * Cin) ** -0.5).to(dt)
    b = rnd(Cout)
    ins, ex = {"A": x}, {"w": w, "b": b, "taps": taps}
    if c["res"]:
        ins["R"] = rnd(M, Cout).to(dt)
    if "K2" in c:
        ins["X2"] = (rnd(M, c["K2"]) * 1.2 - 0.2).to(dt)
        ex["w2"], ex["b2"] = (rnd(Cout, c["K2"]) * c["K2"] ** -0.5).to(dt), rnd(Cout)
    xn = x
    if c["gn"]:
        S, Tn = c["gn"]
        ex["geom"] = ops.Geom.per_sample(S, Tn)
        gamma, beta, film = 1 + 0.1 * rnd(Cin), rnd(Cin), rnd(S, 2 * Cin) * 0.3
        ex["ga"], ex["gb"] = ops.gn_stats(x, gamma, beta, ex["geom"], film=film)
        xn = ops.gn_apply(x, ex["ga"], ex["gb"], ex["geom"], act=c["act"])      # the operand the fused loaders feed, bit for bit
    K = len(taps) * Cin
    if "K2" in c:          # tests/test_restail_gpu.py::test_streamed_tail_meets_float64_element_by_element: the derivation
        sk64, S2 = E.conv_rows_ref(ins["X2"], ex["w2"], ex["b2"], None, E.TAPS_1, (1, 1, 1))
        b_sk = E.gemm_bound(sk64, S2, c["K2"], dt)
        ref, S1 = E.conv_rows_ref(xn, w, b, sk64, E.TAPS_1, (1, 1, 1))
        bound = E.gemm_bound(ref, S1 + b_sk, K, dt) + (1 + E.U16) * b_sk
    else:
        ref, S1 = E.conv_rows_ref(xn, w, b, ins.get("R"), taps, c["dims"])
        bound = E.gemm_bound(ref, S1, K, dt)
    ex["xn"] = xn
    return ins, ex, ref, bound


def _gemm_launch(ops, c, t, ex, tile=None):
    """The ops call of the case on the operand tensors t (compact or placed)."""
    tile = c["tile"] if tile is None else tile
    rec = _as_rec(t["rec"]) if "rec" in t else None
    e = c["entry"]
    if e in ("mmd_conv_gemm", "mmd_conv_gemm_stats"):
        ops.conv_gemm(t["A"], ex["w"], ex["b"], taps=ex["taps"], dims=c["dims"], residual=t.get("R"), out=t["Y"], tile=tile, stats=rec)
    elif e in ("mmd_gn_conv1x1", "mmd_gn_conv1x1_stats"):
        ops.gn_conv1x1(t["A"], ex["ga"], ex["gb"], ex["geom"], c["act"], ex["w"], ex["b"], residual=t.get("R"), out=t["Y"], tile=tile, stats=rec)
    elif e == "mmd_gn_conv_gemm":
        ops.gn_conv_gemm(t["A"], ex["ga"], ex["gb"], ex["geom"], c["act"], ex["w"], ex["b"], ex["taps"], c["dims"], residual=t.get("R"),
                         out=t["Y"], tile=tile)
    elif e == "mmd_gn_conv1x1_skip":
        ops.gn_conv1x1_skip(t["A"], ex["ga"], ex["gb"], ex["geom"], c["act"], ex["w"], ex["b"], t["X2"], ex["w2"], ex["b2"], out=t["Y"], stats=rec)
    else:
        assert e == "mmd_res_tail"
        ops.res_tail(t["A"], ex["ga"], ex["gb"], ex["geom"], c["act"], ex["w"], ex["b"], t["X2"], ex["w2"], ex["b2"], out=t["Y"], stats=rec)


def _gemm_predicate(ops, c, t, ex):
    """The Python rule that routes a launch to this entry / tile, on the placed tensors."""
    rec = _as_rec(t["rec"]) if "rec" in t else None
    if c["entry"] == "mmd_gn_conv1x1_skip":      # (a rule on the layer: slices of >= 16384 rows; its size term is proven on the model's
        return None                              # geometry in tests/test_bigaddr_cpu.py - at this small case it is False everywhere)
    if c["entry"] == "mmd_res_tail":
        return ops.res_tail_ok(t["A"], t["X2"], c["Cout"], ex["geom"], stats=rec, out=t["Y"])
    if c["tile"] == 133:
        return ops.halo_tile_code(t["A"], ex["taps"], c["dims"]) == 133
    if c["tile"] == 131:
        geom = ex.get("geom")
        return (ops.strip_tile_ok(t["A"], c["Cout"], ex["taps"], rec, geom, dims=c["dims"], out=t["Y"], residual=t.get("R"))
                and ops.strip_tile_pinned(t["A"], c["Cout"], ex["taps"], rec, geom, dims=c["dims"], out=t["Y"], residual=t.get("R")))
    return True


def _gemm_engine_path(ops, c, t, ex):
    """What the engine runs when the predicate is False (eager, through ops): tile 133 -> tile 130 (ops.halo_tile_code); tile 131 ->
    gn_apply (for a fused norm) + conv_gemm on the tile the launch rule picks; the fused skip launch -> the two launches."""
    rec = _as_rec(t["rec"]) if "rec" in t else None
    if c["tile"] == 133:
        return _gemm_launch(ops, c, t, ex, tile=ops.halo_tile_code(t["A"], ex["taps"], c["dims"]))
    if c["entry"] == "mmd_gn_conv1x1_skip":
        sk = ops.conv_gemm(t["X2"], ex["w2"], ex["b2"])
        if ops.strip_tile_ok(t["A"], c["Cout"], stats=rec, geom=ex["geom"], out=t["Y"], residual=sk):
            return ops.gn_conv1x1(t["A"], ex["ga"], ex["gb"], ex["geom"], c["act"], ex["w"], ex["b"], residual=sk, tile=131, stats=rec, out=t["Y"])
        hn = ops.gn_apply(t["A"], ex["ga"], ex["gb"], ex["geom"], act=c["act"])
        return ops.conv_gemm(hn, ex["w"], ex["b"], residual=sk, stats=rec, out=t["Y"])
    assert c["tile"] == 131
    xin = ops.gn_apply(t["A"], ex["ga"], ex["gb"], ex["geom"], act=c["act"]) if c["gn"] else t["A"]
    ops.conv_gemm(xin, ex["w"], ex["b"], taps=ex["taps"], dims=c["dims"], residual=t.get("R"), out=t["Y"], tile=0, stats=rec)


def _gemm_check(c, outs, ref, bound, what):
    ratio = E.check(outs["Y"], ref, bound, what=what)
    rrec = EF.check_records(_as_rec(outs["rec"]), EF.record_values(outs["Y"]), what + ": records") if "rec" in outs else 0.0
    return ratio, rrec


_GEMM_ORDER = sorted(B.GEMM_CASES, key=lambda c: c["dt"])          # bf16 first: one arena switch


@pytest.mark.parametrize("c", _GEMM_ORDER, ids=lambda c: c["id"])
def test_gemm_tiles_at_wide_address_ranges(ops, arena_of, c):
    es = B.ES[c["dt"]]
    arena = arena_of(es)
    operands = B.gemm_operands(c)
    dtypes = {n: (torch.float32 if n == "rec" else DT[c["dt"]]) for n, *_ in operands}
    ins, ex, ref, bound = _gemm_inputs(ops, c)
    # the compact, contiguous run
    t0 = dict(ins)
    t0["Y"] = torch.full((c["M"], c["Cout"]), float("nan"), dtype=DT[c["dt"]], device="cuda")
    if c["stats"]:
        t0["rec"] = torch.full((c["M"] // 64, c["Cout"] // 4 * 2), float("nan"), device="cuda")
    plan, labels0 = _record(ops, lambda: _gemm_launch(ops, c, t0, ex))
    assert _rc(ops, plan)[0] == 0
    torch.cuda.synchronize()
    r0, rr0 = _gemm_check(c, t0, ref, bound, f"{c['id']} compact")
    worst, worst_rec, seen = r0, rr0, set()
    for wide in B.gemm_variants(c):
        for pl in B.PLACEMENTS:
            what = f"{c['id']} wide={'+'.join(wide)} placement {pl}"
            P = Placed(arena, operands, wide, pl, ins, dtypes)
            expect, limit = B.gemm_expect(c, P.views)
            seen.add(expect)
            assert pl != "A" or expect == "computes"
            if expect == "refuses":
                with mock.patch.object(ops, "strip_tile_ok", lambda *a, **k: True):       # reach the LIBRARY's answer, not the wrapper's
                    plan, _ = _record(ops, lambda: _gemm_launch(ops, c, P.t, ex))
                rc, msg = _rc(ops, plan)
                name = {133: "tile 133", 131: "tile 131"}.get(c["tile"], c["entry"][4:])
                assert rc < 0 and name in msg and limit in msg, (what, rc, msg)
                P.untouched(what)
                assert not _gemm_predicate(ops, c, P.t, ex), f"{what}: the library refuses, the Python rule does not"
                _gemm_engine_path(ops, c, P.t, ex)
                outs = P.finish(what + " (engine path)")
                r, rr = _gemm_check(c, outs, ref, bound, what + " (engine path)")
            else:
                assert _gemm_predicate(ops, c, P.t, ex) is not False, f"{what}: the Python rule refuses a launch the library runs"
                plan, labels = _record(ops, lambda: _gemm_launch(ops, c, P.t, ex))
                rc, msg = _rc(ops, plan)
                assert rc == 0, (what, rc, msg)
                outs = P.finish(what)
                r, rr = _gemm_check(c, outs, ref, bound, what)
                if labels == labels0:
                    assert _same_bits(outs["Y"], t0["Y"]), f"{what}: Y differs from the compact run"
                    assert "rec" not in outs or _same_bits(outs["rec"], t0["rec"]), f"{what}: records differ from the compact run"
                else:
                    assert c["id"] in B.LABEL_MAY_DIFFER, (what, labels, labels0)
            print(f"\nRATIO bigaddr {c['entry']} {c['id']} {'+'.join(wide)} {pl} [{expect}]: {r:.3f}" + (f" records {rr:.3f}" if c["stats"] else ""))
            worst, worst_rec = max(worst, r), max(worst_rec, rr)
    print(f"\nRATIO bigaddr family=gemm {c['id']}: worst {worst:.3f} records {worst_rec:.3f} behaviours {sorted(seen)}")


# ------------------------------------------------------------------------------------------------- GroupNorm, row bias, resample, copies
def _extras(r):
    """What a launch closure returns: its compact extra outputs as a dict (anything else - the op's own return value - is none)."""
    return r if isinstance(r, dict) else {}


def _nan32(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _norm_setup(ops, c, box=None):
    """(strided inputs, in-place names, launch(t, mode) -> compact extra outputs, check(outs, mode, what) -> ratio, modes) of a
    NORM_CASES row; the float64 references are built once per case."""
    import errbound_bwd as EB
    dt, e = DT[c["dt"]], c["entry"]
    cu = lambda *ts: tuple(None if t is None else t.cuda() for t in ts)
    box = {} if box is None else box
    G = lambda default: ops.Geom(*box.get("geom", default))          # the case's own geometry unless a test substitutes a wide one
    if e == "mmd_gn_apply":
        x, a, b, slices, geom = EF.apply_inputs(c["dt"], c["C"], c["kind"], c["N"], c["Tn"], c["HW"], False)
        x, a, b, slices = cu(x, a, b, slices)
        refs = {act: EF.apply_ref(x[slices], a, b, act, dt) for act in (False, True)}

        def launch(t, act):
            ops.gn_apply(t["X"], a, b, G(geom), act=act, out=t["Y"])

        def check(outs, act, what):
            ref, bound = refs[act]
            return E.check(outs["Y"][slices].flatten(0, 1), ref.flatten(0, 1), bound.flatten(0, 1), what=what)
        return {"X": x}, (), launch, check, (False, True)
    if e in ("mmd_gn_stats", "mmd_gn_small", "mmd_gn_group"):
        x, gamma, beta, fl, slices, geom = EF.gn_inputs(c["dt"], c["C"], c["kind"], c["N"], c["Tn"], c["HW"], 0.0, 51, film=None if e == "mmd_gn_stats" else False)
        x, gamma, beta, fl, slices = cu(x, gamma, beta, fl, slices)
        S = geom[0]
        if e == "mmd_gn_stats":
            f = EB.gn_fwd_ref(x, gamma, beta, fl, slices)

            def launch(t, _):
                a, b, mr = _nan32(S, c["C"]), _nan32(S, c["C"]), _nan32(S, 32, 2)
                ops.gn_stats(t["X"], gamma, beta, G(geom), film=fl, a=a, b=b, mr=mr)
                return {"a": a, "b": b, "mr": mr}

            def check(outs, _, what):
                return max(E.check(outs["a"], f["a"], f["e_a"], what=what + ": a"), E.check(outs["b"], f["b"], f["e_b"], what=what + ": b"),
                           E.check(outs["mr"][..., 0], f["mean"], f["e_mean"], what=what + ": mean"),
                           E.check(outs["mr"][..., 1], f["rstd"], f["e_rstd"], what=what + ": rstd"))
            return {"X": x}, (), launch, check, (None,)
        kern = "small" if e == "mmd_gn_small" else "group"
        refs = {act: EF.two_pass_ref(x, gamma, beta, None, slices, act, dt, kern) for act in (False, True)}

        def launch(t, act):
            if kern == "small":
                ops.gn_small(t["X"], gamma, beta, G(geom), act=act, out=t["Y"])
                return None
            a, b, mr = _nan32(S, c["C"]), _nan32(S, c["C"]), _nan32(S, 32, 2)
            ops.gn_group(t["X"], gamma, beta, ops.Geom(*geom), a=a, b=b, out=t["Y"], act=act, mr=mr)
            return {"a": a, "b": b, "mr": mr}

        def check(outs, act, what):
            r = refs[act]
            w = E.check(outs["Y"], r["y"], r["e_y"], what=what + ": y")
            if kern == "group":
                w = max(w, E.check(outs["a"], r["a"], r["e_a"], what=what + ": a"), E.check(outs["b"], r["b"], r["e_b"], what=what + ": b"),
                        E.check(outs["mr"][..., 0], r["mean"], r["e_mean"], what=what + ": mean"),
                        E.check(outs["mr"][..., 1], r["rstd"], r["e_rstd"], what=what + ": rstd"))
            return w
        return {"X": x}, (), launch, check, (False, True)
    if e == "mmd_gn_finalize_stats":
        rec, gamma, beta, fl = cu(*EF.finalize_inputs(c["C"], c["S"], c["nrec"], 0.6, True))
        r = EF.finalize_ref(rec, c["C"], c["S"], c["nrec"] * 64, gamma, beta, fl)

        def launch(t, _):
            a, b, mr = _nan32(c["S"], c["C"]), _nan32(c["S"], c["C"]), _nan32(c["S"], 32, 2)
            ops.gn_finalize_stats(_as_rec(t["rec"]), gamma, beta, ops.Geom.per_sample(c["S"], c["nrec"] * 64), film=fl, a=a, b=b, mr=mr)
            return {"a": a, "b": b, "mr": mr}

        def check(outs, _, what):
            return max(E.check(outs["a"], r["a"], r["e_a"], what=what + ": a"), E.check(outs["b"], r["b"], r["e_b"], what=what + ": b"),
                       E.check(outs["mr"][..., 0], r["mean"], r["e_mean"], what=what + ": mean"),
                       E.check(outs["mr"][..., 1], r["rstd"], r["e_rstd"], what=what + ": rstd"))
        return {"rec": rec.reshape(rec.shape[0], -1)}, (), launch, check, (None,)
    if e in ("mmd_resample", "mmd_resample_stats"):
        x = EF.resample_inputs(c["NF"], c["H"], c["W"], c["C"], c["dt"]).cuda()
        ref, bound = EF.resample_ref(x, c["NF"], c["H"], c["W"], c["fh"], c["fw"], c["mode"], 1.0, dt)
        orows = ref.shape[0]

        def launch(t, _):
            rec = _nan32(orows // 64, c["C"] // 4, 2) if e == "mmd_resample_stats" else None
            ops.resample(t["X"], t["Y"], c["NF"], c["H"], c["W"], c["fh"], c["fw"], c["mode"], 1.0, stats=rec)
            return {"records": rec} if rec is not None else None

        def check(outs, _, what):
            w = E.check(outs["Y"], ref, bound, what=what)
            if "records" in outs:
                w = max(w, EF.check_records(outs["records"], EF.record_values(outs["Y"]), what + ": records"))
            return w
        return {"X": x}, (), launch, check, (None,)
    if e == "mmd_attn_small_fwd":
        N, F, HW, heads, C = c["N"], c["F"], c["HW"], c["heads"], c["C"]
        g = torch.Generator(device="cuda").manual_seed(29)
        qkv = torch.randn(N * F * HW, 3 * C, device="cuda", generator=g).to(dt)
        ref, bound = (torch.empty(N * F * HW, C, dtype=torch.float64, device="cuda") for _ in range(2))
        for n in range(N):
            for p in range(HW):
                i = n * F * HW + torch.arange(F, device="cuda") * HW + p
                r, Sv, e32 = E.attn_ref(qkv[i, :C], qkv[i, C:2 * C], qkv[i, 2 * C:], heads)
                ref[i], bound[i] = r, E.attn_bound(r, Sv, dt, e32, 2.0 ** -16 if c["dt"] == "bf16" else 0.0)   # (tests/test_elementwise_gpu.py: P as a hi + lo pair)
        return ({"X": qkv}, (), (lambda t, _: ops.attn_small(t["X"], t["Y"], C, heads, G(ops.Geom.temporal(N, F, HW).args()))),
                (lambda outs, _, what: E.check(outs["Y"], ref, bound, what=what)), (None,))
    if e == "mmd_add_rowbias":
        x, eb = cu(*EF.rowbias_inputs(c["dt"], c["N"], c["rps"], c["C"]))
        ref, bound = EF.rowbias_ref(x, eb, c["rps"], dt)
        return {"X": x}, ("X",), (lambda t, _: ops.add_rowbias(t["X"], eb, c["rps"])), (lambda outs, _, what: E.check(outs["X"], ref, bound, what=what)), (None,)
    assert e == "mmd_copy2d"
    x = EF.rowbias_inputs(c["dt"], 3, 37, c["C"])[0].cuda()

    def same(outs, _, what):
        assert _same_bits(outs["Y"], x), f"{what}: not a copy"
        return 0.0
    return {"X": x}, (), (lambda t, _: ops.copy2d(t["X"], t["Y"])), same, (None,)


def _run_placed_family(ops, arena_of, c, family, setup, expect=None, refusal=None):
    """One case of a table whose rows name their strided operands (bigaddr.norm_operands): the compact run, then every wide set at
    placements A / B / C.  setup(ops, c) -> (strided inputs, in-place names, launch(t, mode) -> compact extra outputs, check(outs,
    mode, what) -> ratio, modes[, box]).  A mode starting with "eager" is launched directly instead of through a recorded plan (the
    entry the wrapper picks outside a recording).  expect(c, views) -> (behaviour, limit); refusal(P, mode, what): the checks of a
    refused launch."""
    arena = arena_of(B.ES[c["dt"]])
    operands = B.norm_operands(c)
    dtypes = {n: (torch.float32 if n == "rec" else DT[c["dt"]]) for n, *_ in operands}
    ins, inout, launch, check, modes = setup(ops, c)[:5]
    worst, seen = 0.0, set()

    def go(t, mode):
        extra = {}
        if str(mode).startswith("eager"):
            extra.update(_extras(launch(t, mode)))
            return 0, "", None, extra
        plan, labels = _record(ops, lambda: extra.update(_extras(launch(t, mode))))
        rc, msg = _rc(ops, plan)
        return rc, msg, labels, extra

    all_ins = ins
    for mode in modes:
        ins = all_ins.of(mode) if hasattr(all_ins, "of") else all_ins
        bitwise = not B.atomic_sums(c, mode)
        t0 = {n: (ins[n].clone() if n in ins else torch.full((rows, cols), float("nan"), dtype=dtypes[n], device="cuda")) for n, rows, cols, _ in operands}
        rc, msg, labels0, extra0 = go(t0, mode)
        assert rc == 0, msg
        torch.cuda.synchronize()
        t0.update(extra0)
        worst = max(worst, check(t0, mode, f"{c['id']} compact"))
        for wide in B.variants(operands, c):
            for pl in B.PLACEMENTS:
                what = f"{c['id']} mode={mode} wide={'+'.join(wide)} placement {pl}"
                P = Placed(arena, operands, wide, pl, ins, dtypes, inout)
                behaviour, limit = expect(c, P.views) if expect else ("computes", None)
                seen.add(behaviour)
                if behaviour == "refuses":
                    refusal(ops, c, P, mode, limit, what, go)
                    P.finish(what + " (after the refusal)")
                    print(f"\nRATIO bigaddr {c['entry']} {c['id']} mode={mode} {'+'.join(wide)} {pl} [refuses]: -")
                    continue
                rc, msg, labels, extra = go(P.t, mode)
                assert rc == 0, (what, rc, msg)
                outs = {**P.finish(what), **extra}
                r = check(outs, mode, what)
                assert labels == labels0
                for n in outs:
                    assert not bitwise or _same_bits(outs[n], t0[n]), f"{what}: {n} differs from the compact run"
                print(f"\nRATIO bigaddr {c['entry']} {c['id']} mode={mode} {'+'.join(wide)} {pl} [computes]: {r:.3f}")
                worst = max(worst, r)
    print(f"\nRATIO bigaddr family={family} {c['id']}: worst {worst:.3f} behaviours {sorted(seen)}")


_NORM_ORDER = sorted(B.NORM_CASES, key=lambda c: c["dt"])


@pytest.mark.parametrize("c", _NORM_ORDER, ids=lambda c: c["id"])
def test_norm_and_copies_at_wide_address_ranges(ops, arena_of, c):
    _run_placed_family(ops, arena_of, c, "norm", _norm_setup)


# ------------------------------------------------------------------------------------------------- fused convs, stem, head
def _fused_setup(ops, c):
    import errbound_fused as Z
    e = c["entry"]
    cu = lambda *ts: tuple(t.cuda() if torch.is_tensor(t) else t for t in ts)
    if e == "mmd_tconv":
        N, HW, Cin, Cout = c["N"], c["HW"], c["Cin"], c["Cout"]
        g = torch.Generator(device="cuda").manual_seed(N + HW + Cin + Cout)
        x = torch.randn(N * 16 * HW, Cin, device="cuda", generator=g).to(torch.bfloat16)
        w = (torch.randn(Cout, 3 * Cin, device="cuda", generator=g) * (3 * Cin) ** -0.5).to(torch.bfloat16)
        b = torch.randn(Cout, device="cuda", generator=g)
        wf = ops.tconv_pack(w)
        ref, S = E.conv_rows_ref(x, w, b, None, E.TAPS_TEMPORAL, (16, HW, 1))      # mmd_tconv is bitwise conv_gemm with the temporal taps
        bound = E.gemm_bound(ref, S, 3 * Cin, torch.bfloat16)

        def launch(t, _):
            rec = _nan32(N * 16 * HW // 64, Cout // 4, 2)
            ops.tconv(t["X"], wf, b, Cout, N, 16, HW, out=t["Y"], stats=rec)
            return {"records": rec}

        def check(outs, _, what):
            vals = outs["Y"].view(N, 16, HW // 4, 4, Cout // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(N * HW // 4, Cout // 4, 256)   # the kernel's record order
            return max(E.check(outs["Y"], ref, bound, what=what), EF.check_records(outs["records"], vals, what + ": records"))
        return {"X": x}, (), launch, check, (None,)
    if e == "mmd_aconv":
        N, L, Cin, Cout, dil = c["N"], c["L"], c["Cin"], c["Cout"], c["dil"]
        g = torch.Generator().manual_seed(N * L + Cin + dil)
        x = (torch.randn(N * L, Cin, generator=g) * 1.5 + 0.3).to(torch.bfloat16).cuda()
        w = torch.randn(Cout, Cin, 3, generator=g) * (1.0 / (3 * Cin) ** 0.5)
        bias = torch.randn(Cout, generator=g).cuda()
        gamma, beta = (1 + 0.2 * torch.randn(Cin, generator=g)).cuda(), (0.2 * torch.randn(Cin, generator=g)).cuda()
        wp = ops.pack_conv_weight(w, torch.bfloat16).cuda()
        geom = ops.Geom.per_sample(N, L)
        a, b = ops.gn_stats(x, gamma, beta, geom)
        xn = ops.gn_apply(x, a, b, geom, act=True)           # the operand the kernel feeds, bit for bit (bitwise gn_apply + conv_gemm)
        ref, S = E.conv_rows_ref(xn, wp, bias, None, E.taps_audio(dil), (L, 1, 1))
        bound = E.gemm_bound(ref, S, 3 * Cin, torch.bfloat16)

        def launch(t, _):
            rec = _nan32(N * L // 64, Cout // 4, 2)
            ops.aconv(t["X"], a, b, wp, bias, N, L, dil, act=True, out=t["Y"], stats=rec)
            return {"records": rec}

        def check(outs, _, what):
            return max(E.check(outs["Y"], ref, bound, what=what), EF.check_records(outs["records"], EF.record_values(outs["Y"]), what + ": records"))
        return {"X": x}, (), launch, check, (None,)
    if e == "mmd_tattn_block":
        o = cu(*Z.tattn_case(c["name"]))
        x, wqkv, wproj, bqkv, bproj, gamma, beta, N, HW = o
        ref, bound, validity = Z.tattn_ref(*o)
        assert validity < 0.5
        wf = ops.tattn_pack(wqkv, wproj)
        return ({"X": x}, (), (lambda t, _: ops.tattn_block(t["X"], wf, bqkv, bproj, gamma, beta, Z.HEADS, N, Z.F, HW, out=t["Y"])),
                (lambda outs, _, what: E.check(outs["Y"], ref, bound, what=what)), (None,))
    if e == "mmd_vconv2d1d":
        o = cu(*Z.vconv_case(c["name"], c["gn"]))
        x, ws, wt, bs, bt, a, b, act, N, Hh, Ww = o
        ref, bound = Z.vconv_ref(*o)
        wf = ops.vconv_pack(ws, wt)
        M = x.shape[0]
        S = 2

        def launch(t, _):
            kw = {} if a is None else dict(a=a, b=b, geom=ops.Geom.per_sample(S, M // S), act=act)
            with mock.patch.object(ops, "vconv_shape_ok", _vconv_shape_only):      # the LIBRARY's answer to a sample of 2 GiB, not the wrapper's
                ops.vconv2d1d(t["X"], wf, bs, bt, N, Z.F, Hh, Ww, out=t["Y"], **kw)
        return {"X": x}, (), launch, (lambda outs, _, what: E.check(outs["Y"], ref, bound, pixels=Hh * Ww, what=what)), (None,)
    if e == "mmd_stem_conv":
        k = next(k for k in EF.stem_cases() if k["name"] == c["name"])
        x, w, bias = (None if t is None else t.cuda() for t in EF.edge_inputs(k))
        taps, dims = EF.TAPS[k["taps"]], (k["F"], k["H"], k["W"])
        ref, bound = EF.edge_ref(EF.api_to_rows(x), w, bias, taps, dims, DT[c["dt"]])
        return ({}, (), (lambda t, _: ops.stem_conv(x, w, bias, t["Y"], k["N"], k["F"], k["Cin"], k["H"], k["W"], taps)),
                (lambda outs, _, what: E.check(outs["Y"], ref, bound, pixels=k["H"] * k["W"], what=what)), (None,))
    if e == "mmd_head_conv":
        k = next(k for k in EF.head_cases() if k["name"] == c["name"])
        x, w, bias = (None if t is None else t.cuda() for t in EF.edge_inputs(k))
        taps, dims = EF.TAPS[k["taps"]], (k["F"], k["H"], k["W"])
        ref, bound = EF.edge_ref(x, w, bias, taps, dims, torch.float32)

        def launch(t, _):
            y = _nan32(k["N"], k["F"], k["Co"], k["H"], k["W"])
            ops.head_conv(t["X"], w, bias, y, k["N"], k["F"], k["H"], k["W"], taps)
            return {"y": y}
        return {"X": x}, (), launch, (lambda outs, _, what: E.check(EF.api_to_rows(outs["y"]), ref, bound, pixels=k["H"] * k["W"], what=what)), (None,)
    assert e == "mmd_head_gemm"
    name, Co, tk, N, Fr, Hh, Ww, S = next(k for k in EF.HEAD_GEMM_CASES if k[0] == c["name"])
    taps = EF.TAPS[tk]
    x, a, b, w, bias = (t.cuda() for t in EF.head_gemm_inputs(Co, tk, N, Fr, Hh, Ww, S))
    M, NO = x.shape[0], len(taps) * Co
    geom = ops.Geom.per_sample(S, M // S)
    wimg = ops.head_gemm_pack(w)
    Pref, eP = EF.head_gemm_ref(x.view(S, M // S, 128), a, b, True, w, EF.head_gemm_unpack(wimg))

    def launch(t, _):
        P = _nan32(NO, M)
        ops.head_gemm(t["X"], a, b, geom, True, wimg, P, NO)
        return {"P": P}
    return {"X": x}, (), launch, (lambda outs, _, what: E.check(outs["P"], Pref, eP, what=what)), (None,)


def _vconv_shape_only(x, Cout, N, F, Hh, Ww):
    """ops.vconv_shape_ok without its size term."""
    return x.dtype == torch.bfloat16 and F == 16 and Cout == 128 and x.shape[1] % 32 == 0 and Hh % 4 == 0 and Ww % 4 == 0 and x.shape[0] == N * F * Hh * Ww


def _fused_refusal(ops, c, P, mode, limit, what, go):
    """mmd_vconv2d1d with one sample's rows of X spanning 2 GiB: refused by name, nothing written, the Python rule False."""
    rc, msg, _, _ = go(P.t, mode)
    assert rc < 0 and "vconv2d1d" in msg and limit in msg, (what, rc, msg)
    P.untouched(what)
    assert not ops.vconv_shape_ok(P.t["X"], 128, 2, 16, 4, 8) and not ops.vconv_fused_ok(P.t["X"], 128, 2, 16, 4, 8, out=P.t["Y"]), what


_FUSED_ORDER = sorted(B.FUSED_CASES, key=lambda c: c["dt"])


@pytest.mark.parametrize("c", _FUSED_ORDER, ids=lambda c: c["id"])
def test_fused_convs_stem_and_head_at_wide_address_ranges(ops, arena_of, c):
    _run_placed_family(ops, arena_of, c, "fused", _fused_setup, B.fused_expect, _fused_refusal)


# ------------------------------------------------------------------------------------------------- backward
def _bwd_setup(ops, c):
    import errbound_bwd as EB
    e, dt = c["entry"], DT[c["dt"]]
    gen = lambda seed: torch.Generator(device="cuda").manual_seed(seed)
    if e == "mmd_colsum_slices":
        S, Tn, C = c["S"], c["Tn"], c["C"]
        g = gen(31)
        data = {False: torch.randn(S * Tn, C, device="cuda", generator=g).to(dt), True: EB.grid_randn((S * Tn, C), g, "cuda").to(dt)}
        assert EB.exact_sum_ok(Tn)
        box = {}

        def launch(t, exact):
            out = torch.zeros(S, C, dtype=torch.float32, device="cuda")
            ops.colsum_slices(t["X"], out, Tn)
            return {"out": out}

        def check(outs, exact, what):
            d3 = data[exact].double().reshape(S, Tn, C)
            ref, Sb = d3.sum(1), d3.abs().sum(1)
            if exact:
                assert torch.equal(outs["out"], ref.float()), what + ": exact sums differ"
                return 0.0
            return E.check(outs["out"], ref, EB.colsum_bound(Sb, Tn), what=what)
        return _Modal({"X": data}), (), launch, check, (False, True)
    if e in ("mmd_gn_bwd", "mmd_gn_bwd_ws0"):
        N, HW, C, kind, Tn = 2, 3, c["C"], c["kind"], c["Tn"]
        g = gen(11 + C + Tn)
        slices, geom = EB.gn_slices(kind, N, Tn, HW)
        rows = slices.numel()
        rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
        x, dy = (rn(rows, C) * 1.5 + 0.3).to(dt), rn(rows, C).to(dt)
        gamma, beta = 1 + 0.1 * rn(C), rn(C)
        film = rn(geom[0], 2 * C) * 0.3 if kind == "per_sample_film" else None
        act = kind.startswith("per_sample")
        G = ops.Geom(*geom)
        S = G.S
        mr = torch.empty(S, 32, 2, dtype=torch.float32, device="cuda")
        a, b = ops.gn_stats(x, gamma, beta, G, film=film, mr=mr)
        r = EB.gn_bwd_ref(x, dy, gamma, beta, film, act, slices, stored=(a, b, mr[..., 0], mr[..., 1]), out_dtype=dt)

        def launch(t, _):
            dgamma, dbeta = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
            dfilm = None if film is None else _nan32(S, 2 * C)
            ops.gn_bwd(t["X"], t["DY"], t["DX"], G, a, b, mr, gamma, beta, film, act, dgamma, dbeta, dfilm)
            return {k: v for k, v in (("dgamma", dgamma), ("dbeta", dbeta), ("dfilm", dfilm)) if v is not None}

        def check(outs, _, what):
            got = dict(dx=outs["DX"], dgamma=outs["dgamma"], dbeta=outs["dbeta"], dfilm=outs.get("dfilm"), a=a, b=b, mean=mr[..., 0], rstd=mr[..., 1])
            return max(EB.check_gn(got, r, what).values())
        # outside a recording the wrapper takes the kept-workspace entry (mmd_gn_bwd_ws0), inside one mmd_gn_bwd
        return {"X": x, "DY": dy}, (), launch, check, (("eager-ws0", "eager-ws0-again") if e == "mmd_gn_bwd_ws0" else (None,))
    if e in ("mmd_attn_bwd_mfma", "mmd_attn_bwd", "mmd_attn_small_bwd"):
        heads, ch = c["heads"], c["ch"]
        C = heads * ch
        if e == "mmd_attn_small_bwd":
            N, F, HW = c["N"], c["F"], c["HW"]
            rows = N * F * HW
            pairs = [(n * F * HW + torch.arange(F, device="cuda") * HW + p,) * 2 for n in range(N) for p in range(HW)]
        else:
            T, nb = c["T"], c["nb"]
            rows = nb * T
            pairs = [(torch.arange(s * T, (s + 1) * T, device="cuda"),) * 2 for s in range(nb)]
        qkv = torch.randn(rows, 3 * C, device="cuda", generator=gen(51)).to(dt)
        do = torch.randn(rows, C, device="cuda", generator=gen(52)).to(dt)
        ins = {"X": qkv, "DO": do}
        lse = None
        if e != "mmd_attn_small_bwd":                        # the forward output (and lse2) the backward reads: computed once, compact
            out = torch.full((rows, C), float("nan"), dtype=dt, device="cuda")
            if e == "mmd_attn_bwd_mfma":
                lse = _nan32(rows * heads)
                ops.attn_lse(qkv, qkv, out, lse, heads, ch, nb, 1, T, T, T, T, 1)
            else:
                ops.attn(qkv, qkv, out, heads, ch, nb, 1, T, T, T, T, 1)
            ins["O"] = out
        mode = {"mmd_attn_bwd_mfma": "mfma", "mmd_attn_bwd": "valu", "mmd_attn_small_bwd": "small"}[e]
        r = EB.attn_bwd_assemble(qkv, qkv, ins.get("O"), do, pairs, heads, mode, dt)

        def launch(t, _):
            d = t["DX"]
            if e == "mmd_attn_bwd_mfma":
                ops.attn_bwd_mfma(t["X"], t["X"], t["O"], t["DO"], d, 0, d, C, 2 * C, lse, heads, ch, nb, 1, T, T, T, T, 1)
            elif e == "mmd_attn_bwd":
                geo = (1, T, 1, 1)
                ops.attn_bwd(t["X"], 0, t["X"], C, 2 * C, t["O"], t["DO"], d, 0, d, C, 2 * C, heads, ch, nb, 1, geo, T, T, geo, T, T, 1, None)
            else:
                ops.attn_small_bwd(t["X"], t["DO"], d, C, heads, ops.Geom.temporal(N, F, HW))

        def check(outs, _, what):
            d = outs["DX"]
            return EB.check_attn_bwd((d[:, :C], d[:, C:2 * C], d[:, 2 * C:]), r, C, what, heads)
        return ins, (), launch, check, (None,)
    assert e == "mmd_conv_wgrad"
    k = next(k for k in EB.wgrad_cases() if k["name"] == c["name"])
    M, Cin, Cout, taps, dims = k["M"], c["Cin"], c["Cout"], k["taps"], k["dims"]
    nt = len(taps)
    assert EB.exact_sum_ok(M)
    g = gen(300 + M + Cin)
    data_dy = {False: torch.randn(M, Cout, device="cuda", generator=g).to(dt), True: EB.grid_randn((M, Cout), g, "cuda").to(dt)}
    data_x = {False: torch.randn(M, Cin, device="cuda", generator=g).to(dt), True: EB.grid_randn((M, Cin), g, "cuda").to(dt)}
    refs = {ex: EB.wgrad_ref(data_dy[ex], data_x[ex], taps, dims) for ex in (False, True)}

    def launch(t, exact):
        dW, db = torch.zeros(Cout, nt * Cin, dtype=torch.float32, device="cuda"), torch.zeros(Cout, dtype=torch.float32, device="cuda")
        ops.conv_wgrad(t["DY"], t["X"], dW, db, taps, dims)
        return {"dW": dW, "db": db}

    def check(outs, exact, what):
        dW, S, db, Sb = refs[exact]
        if exact:
            assert torch.equal(outs["dW"], dW.float()) and torch.equal(outs["db"], db.float()), what + ": exact sums differ"
            return 0.0
        return max(EB.check_groups(outs["dW"], dW, EB.wgrad_bound(S, M, dt), Cin, "tap", what + ": dW"),
                   E.check(outs["db"][None], db[None], EB.colsum_bound(Sb, M)[None], what=what + ": db"))
    # random inputs meet the bound; the atomic kernels' sums depend on the order, so only the exact-sum inputs are compared bitwise
    return _Modal({"DY": data_dy, "X": data_x}), (), launch, check, (False, True)


class _Modal(dict):
    """Strided inputs that depend on the mode (random / exact-sum operands): {name: {mode: tensor}}; the runner asks for one mode's."""

    def of(self, mode):
        return {n: v[mode] for n, v in self.items()}


_BWD_ORDER = sorted(B.BWD_CASES, key=lambda c: c["dt"])


@pytest.mark.parametrize("c", _BWD_ORDER, ids=lambda c: c["id"])
def test_backward_at_wide_address_ranges(ops, arena_of, c):
    """The backward kernels.  mmd_conv_wgrad: placement A runs the transposing 9-tap kernel below its 2 GiB gate, B and C the 128-tile
    kernel above it (bigaddr.wgrad_kernel); both accumulate with atomics, so random inputs are held to the bound and the exact-sum
    inputs to exact equality - with the float64 sums and therefore with the compact run."""
    _run_placed_family(ops, arena_of, c, "backward", _bwd_setup)


# ------------------------------------------------------------------------------------------------- wide Geom fields (outer_stride, tstride)
_GEOM_ORDER = sorted(B.GEOM_CASES, key=lambda c: c["dt"])


@pytest.mark.parametrize("c", _GEOM_ORDER, ids=lambda c: c["id"])
def test_wide_geom_fields(ops, arena_of, c):
    """The row stride stays compact; the extent comes from the Geom's outer_stride or tstride alone (bigaddr.geom_layout): the slices'
    rows lie gigabytes apart in rows of ld elements, everything between them stays the arena's pattern."""
    es, dt = B.ES[c["dt"]], DT[c["dt"]]
    arena = arena_of(es)
    case = dict(c, F=c["Tn"], heads=2, ch=32) if c["entry"] == "mmd_attn_small_fwd" else c
    box = {}
    ins, _, launch, check, modes = _norm_setup(ops, case, box)
    x = ins["X"]
    import errbound_bwd as EB
    slices = EB.gn_slices(c["kind"], c["N"], c["Tn"], c["HW"])[0].cuda()          # the compact rows of every (slice, j), the same order as geom_layout's
    names = B.geom_operands(c)
    worst = 0.0
    for mode in modes:
        t0 = {"X": x}
        if len(names) > 1:
            t0["Y"] = torch.full((x.shape[0], names[1][1]), float("nan"), dtype=dt, device="cuda")
        extra0 = {}
        plan, labels0 = _record(ops, lambda: extra0.update(_extras(launch(t0, mode))))
        assert _rc(ops, plan)[0] == 0
        torch.cuda.synchronize()
        t0.update(extra0)
        worst = max(worst, check(t0, mode, f"{c['id']} compact"))
        for pl in B.PLACEMENTS:
            what = f"{c['id']} mode={mode} placement {pl}"
            ld, geom, rows, R, cols = B.geom_layout(c, pl)
            idx = torch.tensor(rows, device="cuda").flatten()
            nrows = int(idx.max()) + 1
            assert B.BASE[es] + nrows * ld * es + B.GUARD <= arena.nbytes
            full = {n: torch.as_strided(arena.buf.view(dt), (nrows, C), (ld, 1), (B.BASE[es] // es) + cols[n]) for n, C in names}
            cells = {n: torch.as_strided(arena.buf.view(torch.int16), (nrows, C * es // 2), (ld * es // 2, 1), (B.BASE[es] + cols[n] * es) // 2) for n, C in names}
            head = {n: torch.as_strided(arena.buf.view(dt), (x.shape[0], C), (ld, 1), (B.BASE[es] // es) + cols[n]) for n, C in names}   # what ops sees: S * Tn rows
            full["X"][idx] = x[slices.flatten()]
            box["geom"] = geom
            extra = {}
            try:
                plan, labels = _record(ops, lambda: extra.update(_extras(launch(head, mode))))
                rc, msg = _rc(ops, plan)
                assert rc == 0 and labels == labels0, (what, rc, msg)
                torch.cuda.synchronize()
            finally:
                box.pop("geom", None)
            outs = dict(extra)
            if "Y" in full:
                y = torch.full_like(t0["Y"], float("nan"))
                y[slices.flatten()] = full["Y"][idx]
                outs["Y"] = y
            try:
                assert _same_bits(full["X"][idx], x[slices.flatten()]), f"{what}: the input was written"
                for n in cells:
                    cells[n][idx] = B.PATTERN16
                n, where = arena.dirty()
                assert n == 0, f"{what}: {n} words outside the slices' rows were written, first at byte offsets {where}"
            except AssertionError:
                arena.fill()
                raise
            r = check(outs, mode, what)
            for n in outs:
                assert _same_bits(outs[n], t0[n]), f"{what}: {n} differs from the compact run"
            print(f"\nRATIO bigaddr {c['entry']} {c['id']} mode={mode} {c['field']} {pl} [computes]: {r:.3f}")
            worst = max(worst, r)
    print(f"\nRATIO bigaddr family=geom {c['id']}: worst {worst:.3f}")


# ------------------------------------------------------------------------------------------------- attention forward
_ATTN_REF = {}


def _attn_case(c, nb=2, G=2):
    """QKV rows of nb batches of G groups of T rows (seeded), and per group the float64 reference pieces - built once per shape."""
    import errbound_bwd as EB
    key = (c["T"], c["heads"], c["ch"], c["dt"], nb, G)
    if key not in _ATTN_REF:
        T, heads, ch = c["T"], c["heads"], c["ch"]
        C = heads * ch
        g = torch.Generator(device="cuda").manual_seed(25)
        qkv = torch.randn(nb * G * T, 3 * C, device="cuda", generator=g).to(DT[c["dt"]])
        ref, Sv, e32 = (torch.empty(nb * G * T, C, dtype=torch.float64, device="cuda") for _ in range(3))
        lse, e_lse = (torch.empty(nb * G * T, heads, dtype=torch.float64, device="cuda") for _ in range(2))
        for s in range(nb * G):
            i = slice(s * T, (s + 1) * T)
            ref[i], Sv[i], e32[i] = E.attn_ref(qkv[i, :C], qkv[i, C:2 * C], qkv[i, 2 * C:], heads)
            if c["dt"] == "bf16":
                r = EB.attn_bwd_ref(qkv[i, :C], qkv[i, C:2 * C], qkv[i, 2 * C:], None, torch.zeros(T, C, device="cuda", dtype=DT[c["dt"]]), heads, "mfma")
                lse[i], e_lse[i] = r["lse2"], r["e_lse2"]
        _ATTN_REF[key] = (qkv, ref, Sv, e32, lse, e_lse)
    return _ATTN_REF[key]


def _attn_check(c, outs, refs, what):
    _, ref, Sv, e32, lse, e_lse = refs
    r = E.check(outs["O"], ref, E.attn_bound(ref, Sv, DT[c["dt"]], e32, c["p_round"]), what=what)
    if "lse" in outs:
        r = max(r, E.check(outs["lse"], lse, e_lse, what=what + ": lse2"))
    return r


_ATTN_ORDER = sorted(B.ATTN_CASES, key=lambda c: c["dt"])


@pytest.mark.parametrize("c", _ATTN_ORDER, ids=lambda c: c["id"])
def test_attention_forward_at_wide_address_ranges(ops, arena_of, c):
    arena = arena_of(B.ES[c["dt"]])
    T, heads, ch = c["T"], c["heads"], c["ch"]
    C, rows = heads * ch, 4 * T
    refs = _attn_case(c)
    qkv = refs[0]
    operands = B.attn_operands(c)
    dtypes = {n: DT[c["dt"]] for n, *_ in operands}
    with_lse = c["entry"] == "mmd_attn_fwd_lse"

    def launch(t, impl):
        if with_lse:
            ops.attn_lse(t["QKV"], t["QKV"], t["O"], t["lse"], heads, ch, 2, 2, 2 * T, T, 2 * T, T, 1)
        else:
            ops.attn(t["QKV"], t["QKV"], t["O"], heads, ch, 2, 2, 2 * T, T, 2 * T, T, 1, impl=impl)

    def fresh_lse():
        return {"lse": torch.full((rows, heads), float("nan"), device="cuda")} if with_lse else {}

    t0 = {"QKV": qkv, "O": torch.full((rows, C), float("nan"), dtype=DT[c["dt"]], device="cuda"), **fresh_lse()}
    plan, labels0 = _record(ops, lambda: launch(t0, c["impl"]))
    assert _rc(ops, plan)[0] == 0
    torch.cuda.synchronize()
    worst, seen = _attn_check(c, t0, refs, f"{c['id']} compact"), set()
    for wide in B.variants(operands):
        for pl in B.PLACEMENTS:
            what = f"{c['id']} wide={'+'.join(wide)} placement {pl}"
            P = Placed(arena, operands, wide, pl, {"QKV": qkv}, dtypes)
            extra = fresh_lse()                                    # lse2_out has no row stride: a compact [rows, heads] table
            tt = {**P.t, **extra}
            expect, limit = B.attn_expect(c, P.views)
            seen.add(expect)
            impl = c["impl"]
            if expect == "refuses":
                plan, _ = _record(ops, lambda: launch(tt, impl))
                rc, msg = _rc(ops, plan)
                assert rc < 0 and f"impl {impl}" in msg and limit in msg, (what, rc, msg)
                P.untouched(what)
                impl = 0                                           # what the engine asks for: the library picks the kernel
            plan, labels = _record(ops, lambda: launch(tt, impl))
            rc, msg = _rc(ops, plan)
            assert rc == 0, (what, rc, msg)
            outs = {**P.finish(what), **extra}
            r = _attn_check(c, outs, refs, what)
            assert labels == labels0
            for n in outs:          # (impl 4 / 5 are bitwise impl 2, which impl 0 runs beyond the DMA path's reach: include/mmd.h)
                assert _same_bits(outs[n], t0[n]), f"{what}: {n} differs from the compact run"
            print(f"\nRATIO bigaddr {c['entry']} {c['id']} {'+'.join(wide)} {pl} [{expect}]: {r:.3f}")
            worst = max(worst, r)
    print(f"\nRATIO bigaddr family=attn {c['id']}: worst {worst:.3f} behaviours {sorted(seen)}")


@pytest.mark.parametrize("nb", [3, 5])
@pytest.mark.parametrize("impl", [0, 4, 5])
def test_attention_dma_batch_split(ops, arena_of, impl, nb):
    """nb = 3 batches whose K/V are just under 1 GiB each: the DMA-staged path runs launches of 2 + 1 batches.  Then the same with the
    Q rows, and separately the O rows, of one such launch spanning more than 2**31 and 2**32 bytes."""
    c = dict(B.ATTN_SPLIT if nb == 3 else B.ATTN_SPLIT5, impl=impl, p_round=None)
    arena = arena_of(2)
    T, heads, ch, nb = c["T"], c["heads"], c["ch"], c["nb"]
    C, rows = heads * ch, nb * T
    refs = _attn_case(c, nb=nb, G=1)
    qkv = refs[0]
    q = qkv[:, :C].contiguous()

    def launch(t):
        ops.attn(t["Q"], t["KV"], t["O"], heads, ch, nb, 1, T, T, T, T, 1, impl=impl)

    t0 = {"Q": q, "KV": qkv, "O": torch.full((rows, C), float("nan"), dtype=torch.bfloat16, device="cuda")}
    plan, labels0 = _record(ops, lambda: launch(t0))
    assert _rc(ops, plan)[0] == 0
    torch.cuda.synchronize()
    worst = _attn_check(c, t0, refs, "split compact")
    for tag, views in B.attn_split_layouts(c).items():
        what = f"{c['id']} impl {impl} layout {tag}"
        P = Placed(arena, None, None, None, {"Q": q, "KV": qkv}, {n: torch.bfloat16 for n in views}, views=views)
        plan, labels = _record(ops, lambda: launch(P.t))
        rc, msg = _rc(ops, plan)
        assert rc == 0 and labels == labels0, (what, rc, msg)
        outs = P.finish(what)
        r = _attn_check(c, outs, refs, what)
        assert _same_bits(outs["O"], t0["O"]), f"{what}: O differs from the compact run"
        print(f"\nRATIO bigaddr mmd_attn_fwd {c['id']} impl={impl} {tag} [splits]: {r:.3f}")
        worst = max(worst, r)
    print(f"\nRATIO bigaddr family=attn {c['id']} impl={impl}: worst {worst:.3f}")
