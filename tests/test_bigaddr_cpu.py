"""Host side of the wide-address tests (tests/bigaddr.py): the placement arithmetic on plain integers, the limits table against the
Python predicates on fake tensors of every placement, the LD list of include/mmd.h against the covered + excluded entries, the
library's refusals by name (argument checks run before anything touches a device), and the seeded defects: the address sets of a
kernel that truncates a byte offset to 32 bits, sign-extends a 32-bit element index or clamps a descriptor's record count differ
from the true ones exactly at the placements that are meant to show them."""
import ctypes

import pytest
import torch

import bigaddr as B

BF, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF, "f32": F32}


class Fake:
    """What the predicates of mm_diffusion.ops read of a tensor: shape, dtype, row stride, first byte."""

    def __init__(self, rows, cols, dtype, ld=None, ptr=1 << 20):
        self.shape, self.dtype, self._ld, self._ptr = (rows, cols), dtype, ld or cols, ptr

    def dim(self):
        return 2

    def stride(self, i):
        return (self._ld, 1)[i]

    def data_ptr(self):
        return self._ptr

    def element_size(self):
        return self.dtype.itemsize


def _fake(v, dtype):
    return Fake(v.rows, v.cols, dtype, v.ld // v.es, (1 << 32) + v.off)


def _all_layouts():
    """(case id, element size, wide names, placement, views) of every GEMM / norm / attention case."""
    for c in B.GEMM_CASES:
        for wide in B.gemm_variants(c):
            for pl in B.PLACEMENTS:
                yield c, B.ES[c["dt"]], wide, pl, B.layout(B.gemm_operands(c), wide, pl, B.ES[c["dt"]])
    for c in B.NORM_CASES + B.FUSED_CASES + B.BWD_CASES:
        es = B.ES[c["dt"]]
        for wide in B.variants(B.norm_operands(c), c):
            for pl in B.PLACEMENTS:
                yield c, es, wide, pl, B.layout(B.norm_operands(c), wide, pl, es)
    for c in B.ATTN_CASES:
        es = B.ES[c["dt"]]
        for wide in B.variants(B.attn_operands(c)):
            for pl in B.PLACEMENTS:
                yield c, es, wide, pl, B.layout(B.attn_operands(c), wide, pl, es)


LAYOUTS = list(_all_layouts())


def test_arena_sizes():
    for es in (2, 4):
        assert B.ARENA_BYTES[es] <= 17 * B.GIB
        assert B.BASE[es] >= B.B31 * es
        assert B.ARENA_BYTES[es] >= B.BASE[es] + (B.B32 + B.GUARD if es == 2 else 1 << 33)
        assert B.ARENA_BYTES[es] % 4 == 0 and B.CHUNK % 4 == 0
    # the pattern is not a finite number in either format
    assert torch.tensor([B.PATTERN16], dtype=torch.int16).view(BF).isnan().all()
    assert torch.tensor([B.PATTERN32], dtype=torch.int32).view(F32).isnan().all()
    assert torch.tensor([B.PATTERN32], dtype=torch.int32).view(torch.int16).tolist() == [B.PATTERN16, B.PATTERN16]


def test_placements_straddle_where_they_claim_and_stay_inside_the_arena():
    n = 0
    for c, es, wide, pl, views in LAYOUTS:
        what = (c["id"], wide, pl)
        assert B.arena_need(views, es) <= B.ARENA_BYTES[es], what
        taken = []
        for v in views.values():
            assert v.off % 16 == 0 or v.name == "rec", what
            assert v.ld % (8 if v.name == "rec" else 16) == 0 and v.ld >= v.row_bytes, what
            iv = v.intervals()
            assert not B._overlaps(iv, taken), what          # no two operands share a byte
            taken += iv
            if not v.wide:
                assert v.ld == v.row_bytes and B.GUARD <= v.off and v.off + v.extent <= B.B31, what
                continue
            offs = v.row_offsets()
            assert offs == [r * v.ld for r in range(v.rows)] and v.off >= B.BASE[es], what
            if v.name != "rec":      # (records: float2 units addressed by an int64 record index, slid behind the activations)
                assert v.off + max(v.extent, B.B32 if es == 2 else 1 << 33) + (B.GUARD if es == 2 else 0) <= B.ARENA_BYTES[es], what
            if pl == "A":
                assert v.extent < B.B31 - B.GUARD, what
            else:
                bd, k = B.BOUNDARY[pl], v.k
                assert 0 < k < v.rows - 1, what
                assert offs[k] < bd < offs[k] + v.row_bytes, what                  # row k starts below the boundary and ends above it
                assert offs[k + 1] >= bd and offs[k - 1] + v.row_bytes <= bd, what   # a whole row above, a whole row below
                if pl == "B" and v.name != "rec":
                    assert v.rows * v.ld + v.row_bytes <= B.B32 - B.GUARD, what      # B stays clear of every 4 GiB limit
            # wherever a 32-bit mistake in the offset or the element index would land, it lands in memory the test owns
            for d in B.DEFECTS:
                for a in B.touched(v, d):
                    assert 0 <= a and a + v.es <= B.ARENA_BYTES[es], (what, v.name, d, a)
            n += 1
    assert n > 500


# defect -> the placements at which it must show, per element size: a zero-extended 32-bit quantity wraps at 2**32, a sign-extended one
# at 2**31 - bytes for a byte offset, elements (times ES bytes) for an element index
DIFFERS_AT = {"uint32_byte_offset": {2: {"C"}, 4: {"C"}}, "int32_byte_offset": {2: {"B", "C"}, 4: {"B", "C"}},
              "int32_element_index": {2: {"C"}, 4: set()}, "uint32_element_index": {2: set(), 4: set()}}


@pytest.mark.parametrize("defect", sorted(DIFFERS_AT))
def test_seeded_offset_defects_change_the_address_set_exactly_where_the_placement_says(defect):
    """A truncated byte offset shows once offsets reach 2**32 (placement C), a sign-extended one once they reach 2**31 (B and C), a
    sign-extended bf16 element index at 2**31 elements = 2**32 bytes (C); none at A: without that difference the placements would
    prove nothing.  An fp32 element index reaches 2**31 only at 8 GiB and a zero-extended index later still: no placement asked for
    goes there, and the table says so instead of pretending (the arena still holds wherever such an index would land).
    Activation operands only (bf16 / fp32 elements)."""
    seen = {"A": 0, "B": 0, "C": 0}
    for c, es, wide, pl, views in LAYOUTS:
        for v in views.values():
            if not v.wide or v.name == "rec":
                continue
            same = B.touched(v, defect) == B.touched(v)
            assert same == (pl not in DIFFERS_AT[defect][v.es]), (c["id"], wide, pl, v.name)
            seen[pl] += 1
    assert min(seen.values()) > 100


def test_seeded_descriptor_clamp_loses_rows_at_b_and_c_only():
    """A buffer descriptor whose record count is clamped to 2**31 - 1 without a guard in the launcher silently drops the rows above."""
    for c, es, wide, pl, views in LAYOUTS:
        for v in views.values():
            if v.wide:
                lost = v.rows - len(B.clamped_records(v))
                assert (lost == 0) == (pl == "A"), (c["id"], wide, pl, v.name, lost)
                if pl != "A":
                    assert lost >= v.rows - 1 - v.k          # the straddling row and everything above it


def test_wide_geom_placements():
    """outer_stride / tstride carry the extent, the row stride stays compact: a used row of every operand straddles the boundary, a
    whole used row lies above, and every address a 32-bit mistake would form stays inside the arena."""
    for c in B.GEOM_CASES:
        es = B.ES[c["dt"]]
        for pl in B.PLACEMENTS:
            ld, geom, rows, R, cols = B.geom_layout(c, pl)
            S, Tn, inner, outer, istride, tstride = geom
            assert ld % 8 == 0 and ld < 8192 and len(rows) == S and all(len(r) == Tn for r in rows)
            # the rows are what mmd_gn_stats' slice formula gives: base(s) + j * tstride
            assert rows == [[(s // inner) * outer + (s % inner) * istride + j * tstride for j in range(Tn)] for s in range(S)]
            wide_field = outer if c["field"] == "outer_stride" else tstride
            assert wide_field * ld * es > (B.GIB if pl != "A" else 64 * B.MIB) // 16
            used = sorted(r for sl in rows for r in sl)
            top = (used[-1] + 1) * ld * es
            assert B.BASE[es] + top + B.GUARD <= B.ARENA_BYTES[es]
            for name, C in B.geom_operands(c):
                off = B.BASE[es] + cols[name] * es
                if pl == "A":
                    assert top < B.B31 - B.GUARD
                else:
                    bd = B.BOUNDARY[pl]
                    assert R * ld * es < bd < R * ld * es + C * es - cols[name] * es or R * ld * es < bd < R * ld * es + C * es
                    assert any(r > R for r in used)
                for r in used:
                    for o in (r * ld * es, r * ld * es + C * es - es):
                        for d in B.DEFECTS.values():
                            a = off + d(o, es)
                            assert 0 <= a and a + es <= B.ARENA_BYTES[es], (c["id"], pl, name, r)


def test_attention_split_layouts():
    """The hand-made strides of the DMA split case: inside the arena, no shared byte, the chunk extents they claim."""
    views5 = B.attn_split_layouts(B.ATTN_SPLIT5)["kv"]
    kv5 = B.ATTN_SPLIT5["T"] * views5["KV"].ld
    assert B.attn_batch_split(5, kv5) == [(0, 2), (2, 4), (4, 5)] and 5 * kv5 > B.B32 and B.arena_need(views5, 2) <= B.ARENA_BYTES[2]
    assert views5["KV"].off + views5["KV"].extent + B.GUARD <= B.ARENA_BYTES[2]
    c = B.ATTN_SPLIT
    T = c["T"]
    for tag, views in B.attn_split_layouts(c).items():
        assert B.arena_need(views, 2) <= B.ARENA_BYTES[2], tag
        taken = []
        for v in views.values():
            assert not B._overlaps(v.intervals(), taken) and v.off + v.extent + B.GUARD <= B.ARENA_BYTES[2], (tag, v.name)
            taken += v.intervals()
            for d in B.DEFECTS:
                assert all(0 <= a and a + v.es <= B.ARENA_BYTES[2] for a in B.touched(v, d)), (tag, v.name, d)
        kv = T * views["KV"].ld
        assert B.attn_batch_split(c["nb"], kv) == [(0, 2), (2, 3)] and B.GIB - 64 * B.KB < kv < B.GIB
        for n, bd in (("q31", B.B31), ("q32", B.B32), ("o31", B.B31), ("o32", B.B32)):
            if tag.endswith(n):
                v = views[n[0].upper()]
                assert (2 * T - 1) * v.ld + v.row_bytes > bd and (2 * T - 2) * v.ld < bd + 64 * B.MIB      # the 2-batch launch passes the boundary


def test_seeded_dropped_attention_split():
    """nb = 3 batches of just under 1 GiB of K/V: the launcher runs 2 + 1 batches, every launch's descriptor below 2**31; with the
    split dropped the one descriptor's (int) byte count is not the true one.  Whether the hardware then misreads is not emulable
    here (an unsigned record count of 3 GiB still covers the rows): the model shows the cast going wrong, the GPU test shows the split
    computing the case."""
    kv = B.GIB - 4096
    as_int = lambda n: ((n & 0xFFFFFFFF) ^ B.B31) - B.B31
    split = B.attn_batch_split(3, kv)
    assert split == [(0, 2), (2, 3)]
    assert all(as_int((b - a) * kv) == (b - a) * kv for a, b in split)
    (a, b), = B.attn_batch_split(3, kv, defect=True)
    assert as_int((b - a) * kv) != (b - a) * kv
    assert B.attn_batch_split(3, 1 << 20) == [(0, 3)] == B.attn_batch_split(3, 1 << 20, defect=True)     # small: no difference


# ------------------------------------------------------------------------------------------------- the table against the predicates
def _gemm_fakes(c, views):
    dt = DT[c["dt"]]
    t = {n: _fake(v, F32 if n == "rec" else dt) for n, v in views.items()}
    return t


def test_limits_table_fields():
    for r in B.LIMITS:
        assert r["kind"] in ("launch", "sample", "frame", "none") and r["beyond"] in ("computes", "splits", "refuses")
        assert (r["limit"] is None) == (r["kind"] == "none")
        assert r["entry"] in B.ld_entries()
    # every refusal names the Python rule that mirrors it (the DMA attention impls are forced by tests only: impl 0 never refuses)
    assert all(r["predicate"] for r in B.LIMITS if r["beyond"] == "refuses" and r["entry"] != "mmd_attn_fwd")


def test_predicates_are_false_wherever_the_table_refuses():
    from mm_diffusion import ops
    from mm_diffusion.ops import Geom
    import errbound as E
    taps_of = {"1": E.TAPS_1, "9": E.TAPS_SPATIAL, "t3": E.TAPS_TEMPORAL}
    seen = {}
    for c in B.GEMM_CASES:
        es = B.ES[c["dt"]]
        taps = taps_of[c["taps"]]
        geom = Geom.per_sample(*c["gn"]) if c["gn"] else None
        for wide in B.gemm_variants(c):
            for pl in B.PLACEMENTS:
                views = B.layout(B.gemm_operands(c), wide, pl, es)
                t = _gemm_fakes(c, views)
                expect, _ = B.gemm_expect(c, views)
                refuses = expect == "refuses"
                what = (c["id"], wide, pl, expect)
                stats = True if c["stats"] else None
                if c["tile"] == 131:
                    fused = geom if c["entry"].startswith("mmd_gn_conv1x1") else None
                    kw = dict(dims=c["dims"], out=t["Y"], residual=t.get("R"))
                    assert ops.strip_tile_ok(t["A"], c["Cout"], taps, stats, fused, **kw) == (not refuses), what
                    assert ops.strip_tile_pinned(t["A"], c["Cout"], taps, stats, fused, **kw) == (not refuses), what
                    if fused is not None and refuses:
                        assert not ops.gn_fusable(fused, c["Cin"], c["Cout"], t["A"], stats, act=c["act"], out=t["Y"], residual=t.get("R")), what
                elif c["tile"] == 133:
                    assert (ops.halo_tile_code(t["A"], taps, c["dims"]) == 133) == (not refuses), what
                    assert ops.halo_tile_ok(t["A"], taps, c["dims"]), what             # tile 130 takes the frame either way
                elif c["entry"] == "mmd_res_tail":
                    assert not refuses and ops.res_tail_ok(t["A"], t["X2"], c["Cout"], geom, stats, t["Y"]), what
                elif c["tile"] == 132:
                    assert not refuses and ops.ring_tile_candidate(t["A"], c["Cout"], len(taps)), what
                else:
                    assert not refuses or c["entry"] == "mmd_gn_conv1x1_skip", what
                seen[(c["tile"] or c["entry"], expect)] = seen.get((c["tile"] or c["entry"], expect), 0) + 1
    # both sides of every limit were met
    for key in ((131, "computes"), (131, "splits"), (131, "refuses"), (133, "computes"), (133, "refuses"),
                ("mmd_gn_conv1x1_skip", "refuses"), ("mmd_gn_conv1x1_skip", "computes"), ("mmd_res_tail", "computes")):
        assert seen.get(key, 0) > 0, key


def test_skip_fusable_and_strip_rules_on_the_model_geometry_at_large_batch():
    """The ds1 level of the base model in bf16: 65536 rows per sample, the ResBlock output a 128-channel slice of the 384-channel concat
    buffer - M * ldy * 2 passes 4 GiB at batch 86.  The fused skip launch is refused there by the library, so skip_fusable is False; the
    row strip is cut into several launches, so strip_tile_ok / strip_tile_pinned / gn_fusable / res_tail_ok stay True: the layer keeps
    its kernel family at every batch size."""
    from mm_diffusion import ops
    from mm_diffusion.ops import Geom
    rows = 65536
    for N, big in ((4, False), (85, False), (86, True), (200, True)):
        M = N * rows
        assert (M * 384 * 2 >= 0xffffffff) == big
        h, x, y = Fake(M, 128, BF), Fake(M, 256, BF, 384, (1 << 30)), Fake(M, 128, BF, 384, (1 << 40))
        geom = Geom.per_sample(N, rows)
        assert ops.skip_fusable(h, x, 128, geom, stats=True, out=y) == (not big)
        assert ops.strip_tile_ok(h, 128, stats=True, geom=geom, out=y) and ops.strip_tile_pinned(h, 128, stats=True, geom=geom, out=y)
        assert ops.gn_fusable(geom, 128, 128, h, True, act=True, out=y)
        assert ops.strip_cut_rows(geom=geom) == rows and 0xfffffffe // (384 * 2) >= rows
    # the deep levels (mmd_res_tail: 64-bit addresses, no limit)
    M = 200 * 16384
    assert ops.res_tail_ok(Fake(M, 256, BF), Fake(M, 640, BF, ptr=1 << 36), 256, Geom.per_sample(200, 16384), True, Fake(M, 256, BF, 1024, 1 << 42))


def test_rules_with_and_without_a_size_term_match_the_table():
    """vconv: a sample of 2 GiB or more is refused on both sides.  tconv / aconv / tattn: no launcher guard, no term in the rule."""
    from mm_diffusion import ops
    N, F, Hh, Ww, Cin = 1, 16, 8, 8, 64
    M = N * F * Hh * Ww
    for ld, ok in ((Cin, True), ((B.B31 // 2 - 2 * Cin) // (16 * Hh * Ww), True), (B.B31 // 2 // (16 * Hh * Ww) + 8, False)):
        x = Fake(M, Cin, BF, ld)
        assert ((16 * Hh * Ww * ld + Cin) * 2 < B.B31) == ok
        assert ops.vconv_shape_ok(x, 128, N, F, Hh, Ww) == ok, ld
    wide = (B.B32 // M) // 16 * 8
    assert ops.tconv_shape_ok(Fake(M, 256, BF, wide), 256, N, F, Hh * Ww)
    assert ops.tattn_shape_ok(Fake(M, 256, BF, wide), 4, N, F, Hh * Ww)
    assert ops.aconv_shape_ok(Fake(M, 256, BF, wide, 1 << 20), 256, 2, M // 2)


def test_ld_list_is_covered_or_excluded():
    ld = B.ld_entries()
    assert len(ld) >= 36 and "mmd_conv_gemm" in ld and ld["mmd_copy2d"] == ["ldx_bytes", "ldy_bytes"]
    assert not set(B.COVERED) & set(B.EXCLUDED)
    assert set(B.COVERED) | set(B.EXCLUDED) == set(ld), (set(ld) - set(B.COVERED) - set(B.EXCLUDED), (set(B.COVERED) | set(B.EXCLUDED)) - set(ld))
    cased = {c["entry"] for cs in (B.GEMM_CASES, B.NORM_CASES, B.FUSED_CASES, B.BWD_CASES, B.ATTN_CASES) for c in cs}
    assert {c["entry"] for c in B.GEOM_CASES} == {"mmd_gn_stats", "mmd_gn_apply", "mmd_gn_small", "mmd_attn_small_fwd"}
    assert set(B.EXCLUDED) == {"mmd_vlb_terms", "mmd_cond_replace", "mmd_cond_replace_ctr"}      # only entries with no strided activation
    assert cased == set(B.COVERED)
    assert all(len(why) > 10 for why in B.EXCLUDED.values())
    assert {r["entry"] for r in B.LIMITS} >= set(ld) - {"mmd_vlb_terms", "mmd_cond_replace", "mmd_cond_replace_ctr"}
    assert B.LABEL_MAY_DIFFER == {}


# ------------------------------------------------------------------------------------------------- the library's refusals by name
def _lib():
    from mm_diffusion import _hip
    return _hip.lib()


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: only where no launch can follow a missing refusal (the GPU module "
                    "runs the same refusals on memory it owns)")
def test_library_refuses_by_name_before_any_launch():
    """Argument checks run before anything touches a device: fake (aligned) pointers, no GPU."""
    lib = _lib()
    p = 1 << 30
    taps1 = (ctypes.c_int * 3)(0, 0, 0)
    # tile 131: 100 rows cannot be cut (the unit is 256 rows), Y past 4 GiB
    ld = B.B32 // 100 // 16 * 8 + 8
    assert 100 * ld * 2 >= 0xffffffff and 0xfffffffe // (ld * 2) < 256      # (never a call that would launch: there is no device here)
    rc = lib.mmd_conv_gemm(1, p, 128, p, None, None, 0, p, ld, 100, 64, 128, 1, taps1, 1, 1, 1, 131, None)
    msg = lib.mmd_last_error()
    assert rc < 0 and b"tile 131" in msg and b"4 GB" in msg, msg
    # ... and the residual alone
    rc = lib.mmd_conv_gemm(1, p, 128, p, None, p, ld, p, 64, 100, 64, 128, 1, taps1, 1, 1, 1, 131, None)
    assert rc < 0 and b"tile 131" in lib.mmd_last_error() and b"4 GB" in lib.mmd_last_error()
    # the fused skip launch: M * ldy * 2 >= 4 GiB
    ldy = B.B32 // 384 // 16 * 8 + 8
    assert 384 * ldy * 2 >= 0xffffffff
    rc = lib.mmd_gn_conv1x1_skip(1, p, 128, p, p, 1, 1, 384, p, None, p, 256, 256, p, None, p, ldy, 384, 128, 128, None, 0, None)
    assert rc < 0 and b"gn_conv1x1_skip" in lib.mmd_last_error() and b"4 GB" in lib.mmd_last_error()
    # tile 133: one frame of 2 GiB
    taps9 = (ctypes.c_int * 27)(*[v for dh in (-1, 0, 1) for dw in (-1, 0, 1) for v in (0, dh, dw)])
    lda = B.B31 // 511 // 16 * 8 + 16
    assert (511 * lda + 256) * 2 >= 0x7fffffff          # (never a call that would launch: there is no device here)
    rc = lib.mmd_conv_gemm(1, p, lda, p, None, None, 0, p, 128, 1024, 128, 256, 9, taps9, 2, 16, 32, 133, None)
    assert rc < 0 and b"tile 133" in lib.mmd_last_error() and b"2 GB" in lib.mmd_last_error()
