"""Address ranges past 2 GiB and 4 GiB: the size-limit table of libmmd's strided kernels, the placement model and the arena.

The kernel-level suite runs small shapes, so every byte offset in it fits in 31 bits.  The library also has code that only runs when
an operand's address range - (rows - 1) * ld * ES + C * ES of a row-strided view, not the amount of work - passes 2**31 or 2**32
bytes: other instantiations, launches cut into several, refusals.  This module reaches those ranges with the EXISTING small cases
by widening the row stride only (a few hundred rows, megabytes apart), inside one allocation the test owns:

  LIMITS       the reading pass over every kernel reached from a C-ABI entry with a row stride (the LD list of include/mmd.h): how it
               forms global addresses, the extent at which that stops being valid, what the launcher does beyond, what the Python
               predicates know.  include/mmd.h ("Size limits") and INTEGRATION.md say the same in words.
  ld_entries   the LD list derived from the header; COVERED + EXCLUDED must equal it (tests/test_bigaddr_cpu.py).
  stride_for / layout   the placement model, plain integers: placements A (control, below 2**31), B (crosses 2**31: one row straddles
               the boundary, a whole row lies above) and C (the same for 2**32), the operands' offsets inside the arena, and the
               address sets a defective kernel would touch (DEFECTS) - all of which stay inside the arena.
  Arena        the one torch.uint8 allocation per element size (GPU only) with its exact stray-write check.

Remaining gap: a 32-bit ELEMENT index (as opposed to a byte offset) wraps at 2**31 elements, i.e. at 4 GiB in bf16 (placement C shows it)
but only at 8 GiB in fp32, and a zero-extended one at 8 / 16 GiB; no placement goes there (an fp32 arena of 8 GiB extent behind a base of
8 GiB does not fit the 17 GiB cap), so for fp32 operands the placements prove byte-offset mistakes only (tests/test_bigaddr_cpu.py:
DIFFERS_AT).  Tile 133 and the DMA attention have a limit per frame / per batch: tile 133's existing cases have at most two frames, so
"every frame below the limit, the tensor past 2**32" cannot be built from them (its C placement is the refusal); attention has it (nb = 5).

Arena layout for element size ES (2: bf16, 4: fp32), offsets from the arena start:
  [64 kB, 2**31)                         compact (contiguous) operands of the case
  [2**31 * ES, ...)                      the wide operands; a sign-extended 32-bit byte offset or element index scaled by ES still
                                         lands at or behind the arena start
  ... base + max(extent, 2**32) + 64 kB  (ES = 4: base + 2**33) a zero-extended or wrapped one still lands in front of the arena end
"""
import math
import os
import re

KB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30
B31, B32 = 1 << 31, 1 << 32
GUARD = 64 * KB
PATTERN32 = 0x7FA57FA5          # as two bf16: 0x7FA5, 0x7FA5 (NaN); as one fp32: NaN - one int32 compare checks either arena
PATTERN16 = 0x7FA5
CHUNK = 256 * MIB
ES = {"bf16": 2, "f32": 4}
BASE = {2: B31 * 2, 4: B31 * 4}                                   # first wide-operand byte, from the arena start
ARENA_BYTES = {2: 11 * GIB, 4: 16 * GIB + MIB}                    # at most 17 GiB; one alive at a time
EXTENT_CAP = {"A": B31 - GUARD, "B": B32 - GUARD, "C": {2: ARENA_BYTES[2] - BASE[2] - 2 * GUARD, 4: (1 << 33) - 2 * GUARD}}
BOUNDARY = {"B": B31, "C": B32}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the LD list of include/mmd.h
_STRIDE_PARAM = re.compile(r"ld[a-z0-9_]*|[a-z0-9_]*_ld|[a-z0-9_]*stride[a-z0-9_]*|rows_per_[a-z0-9_]*")


def ld_entries(header_text=None):
    """{entry: [stride parameters]} for every prototype of include/mmd.h with an ld*, *_ld, *stride* or rows_per_* parameter."""
    if header_text is None:
        header_text = open(os.path.join(ROOT, "include", "mmd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|int64_t)\s+(mmd_[a-z0-9_]+)\s*\(([^;]*)\);", text):
        names = [p.strip().split()[-1].lstrip("*") for p in m.group(2).split(",") if p.strip() != "void"]
        hit = [n for n in names if _STRIDE_PARAM.fullmatch(n)]
        if hit:
            out[m.group(1)] = hit
    return out


# ------------------------------------------------------------------------------------------------- the reading pass
# entry, variant (tile / impl / kernel; "" = every variant), operand, how the kernel addresses it, limit kind (launch | sample | frame |
# none), limit in bytes, behaviour beyond (computes | splits | refuses), the Python predicate that knows (or None), source.
# "launch": M * ld * ES of the whole launch; "sample": one batch / sample; "frame": one frame of D1 * D2 rows.
def _row(entry, variant, operand, addressing, kind, limit, beyond, predicate, source):
    return dict(entry=entry, variant=variant, operand=operand, addressing=addressing, kind=kind, limit=limit, beyond=beyond,
                predicate=predicate, source=source)


_GEMM = ("mmd_conv_gemm", "mmd_conv_gemm_stats", "mmd_gn_conv1x1", "mmd_gn_conv1x1_stats", "mmd_gn_conv_gemm")
LIMITS = []
for _e in _GEMM:
    LIMITS += [
        _row(_e, "64,128,130", "A,R,Y,stats", "64-bit", "none", None, "computes", None, "mmd_gemm.hip: load_a_tile / tile epilogue, int64 row * ld"),
        _row(_e, "129,132", "A", "descriptor + 32-bit offsets below the limit, 64-bit pointers beyond", "launch", B31 - 1, "computes", None,
             "mmd_gemm.hip: glds_desc_ok; conv_gemm_glds_kernel<.., DESC>"),
        _row(_e, "129,132", "R,Y,stats", "64-bit", "none", None, "computes", None, "mmd_gemm.hip: tile epilogue"),
        _row(_e, "133", "A", "per-frame descriptor, 32-bit offsets inside the frame", "frame", B31 - 1, "refuses", "halo_tile_code",
             "mmd_gemm.hip: launch_conv_gemm_halo16 / conv_gemm_halo16_kernel rsrcA"),
        _row(_e, "133", "R,Y", "64-bit", "none", None, "computes", None, "mmd_gemm.hip: halo16 epilogue, int64 row_of"),
        _row(_e, "131", "A,stats", "64-bit", "none", None, "computes", None, "mmd_gemm.hip: conv1x1_strip_body ap / rec"),
        _row(_e, "131", "R,Y", "32-bit byte offset from a 64-bit base", "launch", B32 - 1, "splits", None,
             "mmd_gemm.hip: conv1x1_strip_body yoff / roff; dispatch_conv1x1_strip cuts the rows"),
        _row(_e, "131", "R,Y", "one cut unit of the launch: 256 rows, the GroupNorm slice, the sample of a conv with taps", "sample", B32 - 1, "refuses",
             "strip_tile_ok", "mmd_gemm.hip: dispatch_conv1x1_strip"),
    ]
LIMITS += [
    _row("mmd_gn_conv1x1_skip", "", "h,x,stats", "64-bit", "none", None, "computes", None, "mmd_gemm.hip: conv1x1_strip_body ap / q.A2"),
    _row("mmd_gn_conv1x1_skip", "", "Y", "32-bit byte offset from a 64-bit base", "launch", B32 - 1, "refuses", "skip_fusable",
         "mmd_gemm.hip: mmd_gn_conv1x1_skip MMD_REQUIRE"),
    _row("mmd_res_tail", "", "h,x,Y,stats", "64-bit", "none", None, "computes", None, "mmd_rtail.hip: load_act / epilogue, int64 rowc * ld"),
    _row("mmd_attn_fwd", "impl 4,5 (and 0 at head width 64)", "KV", "descriptor over the batches of one launch, 32-bit row offsets", "sample",
         B31 - 1, "splits", None, "mmd_attn.hip: attn_fwd_impl batch loop; mmd_attn_common.h: kv_rsrc"),
    _row("mmd_attn_fwd", "impl 4,5", "KV", "one batch of K/V", "sample", B31 - 1, "refuses", None, "mmd_attn.hip: dma_ok (impl 0 runs the per-128-query kernel, bitwise equal)"),
    _row("mmd_attn_fwd", "", "Q,O", "64-bit", "none", None, "computes", None, "mmd_attn.hip: q_frag / store_o, int64 q_row0"),
    _row("mmd_attn_fwd_lse", "", "Q,KV,O", "as mmd_attn_fwd impl 0", "none", None, "computes", None, "mmd_attn.hip: attn_fwd_impl"),
    _row("mmd_attn_small_fwd", "", "QKV,O", "64-bit", "none", None, "computes", None, "mmd_attn.hip: attn_small kernels, int64 row * ld"),
    _row("mmd_vconv2d1d", "", "X", "per-sample descriptor re-based per sample", "sample", B31 - 1, "refuses", "vconv_shape_ok",
         "mmd_vconv.hip:559 / :100; ops.vconv_shape_ok"),
    _row("mmd_conv_wgrad", "transposing kernel", "dY,X", "descriptors cast to int", "launch", B31 - 1, "computes", None,
         "mmd_wgrad.hip:539 gate M * ld * 2 < 2 GiB (the 128-tile kernel runs beyond), :306-307 (int) record counts, :324-338 32-bit row offsets"),
]
for _e in ("mmd_gn_stats", "mmd_gn_apply", "mmd_gn_small", "mmd_gn_group", "mmd_gn_finalize_stats", "mmd_add_rowbias", "mmd_copy2d"):
    LIMITS.append(_row(_e, "", "all", "64-bit", "none", None, "computes", None, "mmd_norm.hip / mmd_misc.hip: int64 base * ld, int64 row strides"))
_I64 = "64-bit: int64 row index times an int64_t ld field"
LIMITS += [
    _row("mmd_tconv", "", "X,Y,stats", _I64, "none", None, "computes", None,
         "mmd_tconv.hip:78 rowi int64, :81 / :153 rowi * p.ldx / p.ldy; the descriptor at :69 covers the packed WEIGHT image (wf_bytes), no activation"),
    _row("mmd_aconv", "", "X,Y,stats", _I64, "none", None, "computes", None, "mmd_aconv.hip:74-75 src int64 * p.ldx, :142 (int64_t)rowc * p.ldy"),
    _row("mmd_tattn_block", "", "X,A,MID,Y,stats", _I64, "none", None, "computes", None,
         "mmd_tattn.hip:136 rowi int64, :139 / :234 / :263 rowi * ld; the descriptor at :126 covers the packed WEIGHT image only"),
    _row("mmd_resample", "", "x,y", _I64, "none", None, "computes", None, "mmd_misc.hip:95-112 irow / orow * ldx / ldy (int64_t parameters)"),
    _row("mmd_resample_stats", "", "x,y,stats", _I64, "none", None, "computes", None, "mmd_misc.hip:147-158"),
    _row("mmd_stem_conv", "", "y", _I64, "none", None, "computes", None, "mmd_edge.hip:28 / :120 / :234 m int64, :44 / :122 / :243 m * p.ldy"),
    _row("mmd_head_conv", "", "x", _I64, "none", None, "computes", None, "mmd_edge.hip:157 / :337 / :417 src int64, :158 / :338 / :421 src * p.ldx"),
    _row("mmd_head_gemm", "", "x", _I64, "none", None, "computes", None, "mmd_edge.hip:569-573 mc int64 * p.ldx"),
    _row("mmd_colsum_slices", "", "dY", _I64, "none", None, "computes", None, "mmd_wgrad.hip:437 / :448 (int64_t)m * ld, :560 (int64_t)s * Tn * lddy"),
    _row("mmd_conv_wgrad", "128-tile and 64-tile kernels", "dY,X", _I64, "none", None, "computes", None, "mmd_wgrad.hip:101-103, :182-186 (int64_t)m * p.lddy / p.ldx"),
    _row("mmd_gn_bwd", "", "x,dy,dx", _I64, "none", None, "computes", None, "mmd_gn_bwd.hip:40-50 (the row walk of reduce and apply), :178 r0 int64 * ldx / lddy / lddx"),
    _row("mmd_gn_bwd_ws0", "", "x,dy,dx", _I64, "none", None, "computes", None, "as mmd_gn_bwd (one implementation: gn_bwd_impl, mmd_gn_bwd.hip:190)"),
    _row("mmd_attn_bwd", "", "Q,KV,O,dO,dQ,dKV", _I64, "none", None, "computes", None, "mmd_attn_bwd_body.inc:32-295 row * p.ld* with int64_t ld fields (mmd_attn_bwd.hip:15-20)"),
    _row("mmd_attn_bwd_mfma", "", "Q,KV,O,dO,dQ,dKV", _I64, "none", None, "computes", None, "mmd_attn_bwd_mfma.hip:84-299 row * p.ld* with int64_t ld fields (:13-18)"),
    _row("mmd_attn_small_bwd", "", "QKV,dO,dQKV", _I64, "none", None, "computes", None, "mmd_attn_bwd.hip:176-213 row * p.ld / lddo / ldd (int64_t, :141-143)"),
]

# Entries whose wide placements tests/test_bigaddr_gpu.py runs ...
COVERED = {
    "mmd_conv_gemm": "GEMM tiles 64 / 128 / 129 / 132 / 130 / 133 / 131",
    "mmd_conv_gemm_stats": "GEMM tiles 64 / 128 / 129 / 131 with records",
    "mmd_gn_conv1x1": "tiles 128 / 131",
    "mmd_gn_conv1x1_stats": "tiles 128 / 131",
    "mmd_gn_conv_gemm": "tiles 130 / 133",
    "mmd_gn_conv1x1_skip": "Y past 4 GiB is refused; the two launches run instead",
    "mmd_res_tail": "streamed tail",
    "mmd_gn_apply": "per-sample and temporal geometry, wide ldx / ldy",
    "mmd_gn_stats": "per-sample and temporal geometry, wide ld",
    "mmd_gn_small": "temporal geometry",
    "mmd_gn_group": "per-sample geometry",
    "mmd_gn_finalize_stats": "wide rec_ld",
    "mmd_resample": "pool and upsample",
    "mmd_resample_stats": "pool with records",
    "mmd_attn_small_fwd": "temporal geometry",
    "mmd_tconv": "fused temporal conv",
    "mmd_aconv": "fused audio conv",
    "mmd_tattn_block": "fused temporal attention block",
    "mmd_vconv2d1d": "fused VideoConv: a sample below 2 GiB (re-based descriptor) and the refusal above",
    "mmd_stem_conv": "pixel / strip / mfma kernels, wide ldy",
    "mmd_head_conv": "strip / coop / plain kernels, wide ldx",
    "mmd_head_gemm": "wide ldx",
    "mmd_colsum_slices": "wide lddy",
    "mmd_conv_wgrad": "transposing kernel below its gate, 128-tile above, 64-tile",
    "mmd_gn_bwd": "per-sample and temporal geometry",
    "mmd_gn_bwd_ws0": "temporal geometry",
    "mmd_attn_bwd": "VALU kernel, bf16 and fp32",
    "mmd_attn_bwd_mfma": "head width 96",
    "mmd_attn_small_bwd": "temporal geometry",
    "mmd_add_rowbias": "wide ld",
    "mmd_copy2d": "wide ldx_bytes / ldy_bytes",
    "mmd_attn_fwd": "impl 0 - 5 at head width 64, impl 0 - 2 at 96; the DMA batch split",
    "mmd_attn_fwd_lse": "head width 64",
}
# ... and the strided entries it does not run, each with the reason.  A new strided entry of include/mmd.h lands in neither set and fails
# tests/test_bigaddr_cpu.py::test_ld_list_is_covered_or_excluded.
EXCLUDED = {
    # small fp32 tables, not activations: out_ld strides a [N, T] table of per-step results, mask_stride a uint8 mask of F * HW cells
    "mmd_vlb_terms": "out_ld: row stride of an fp32 [N, steps] result table, indexed by int64; no activation operand is strided",
    "mmd_cond_replace": "mask_stride: 0 or F * HW cells of a uint8 mask; the fp32 operands are contiguous API tensors",
    "mmd_cond_replace_ctr": "as mmd_cond_replace",
}


# ------------------------------------------------------------------------------------------------- placement model (plain integers)
def stride_for(rows, row_bytes, placement, es, align=16, limited=True):
    """(row stride in bytes, straddling row k) of placement A / B / C for an operand of `rows` rows of `row_bytes` bytes.

    A: rows * ld <= 2**31 - 64 kB (about 1 GiB).  B / C: row k starts below the boundary 2**31 / 2**32 and ends above it
    (k * ld = boundary - d, 0 < d < row_bytes), row k + 1 lies wholly above it, and rows * ld + row_bytes stays below the placement's
    cap (B: 2**32 - 64 kB, so that B never touches the 4 GiB limits).  limited = False - the record buffers: a few dozen rows of
    float2 records addressed by int64 record index, with no limit in any launcher - only keeps the extent inside the arena.  The stride is a multiple of `align` bytes (the kernels' 16-byte
    rows).  The row count is never changed."""
    assert rows >= 3 or placement == "A", "a straddling row and a whole row above it need three rows"
    if placement == "A":
        ld = max(-(-row_bytes // align) * align, (GIB // rows) // align * align)
        assert rows * ld + row_bytes <= EXTENT_CAP["A"]
        return ld, None
    bd = BOUNDARY[placement]
    cap = EXTENT_CAP["B"] if placement == "B" and limited else EXTENT_CAP["C"][es]
    best = None
    for j in range(1, max(2, row_bytes // align)):           # d = j * align < row_bytes
        if j * align >= row_bytes:
            break
        t = bd // align - j                                  # k * (ld / align) == t
        for k in range(rows - 2, 0, -1):
            if t % k == 0:
                ld = t // k * align
                span = rows * ld if limited else (rows - 1) * ld
                if ld >= row_bytes and span + row_bytes <= cap and (best is None or ld < best[0]):
                    best = (ld, k)
                break                                        # the largest k for this d gives its smallest stride
    assert best is not None, f"no stride: rows={rows} row_bytes={row_bytes} placement={placement}"
    return best


class View:
    """A row-strided operand inside the arena: byte offset of its first byte from the arena start, row stride in bytes."""
    __slots__ = ("name", "rows", "cols", "es", "off", "ld", "k", "wide")

    def __init__(self, name, rows, cols, es, off, ld, k=None, wide=False):
        self.name, self.rows, self.cols, self.es, self.off, self.ld, self.k, self.wide = name, rows, cols, es, off, ld, k, wide

    @property
    def row_bytes(self):
        return self.cols * self.es

    @property
    def extent(self):
        return (self.rows - 1) * self.ld + self.row_bytes

    def row_offsets(self):                                   # true byte offset of every row from the operand's own pointer
        return [r * self.ld for r in range(self.rows)]

    def intervals(self):
        return [(self.off + r * self.ld, self.off + r * self.ld + self.row_bytes) for r in range(self.rows)]


def _overlaps(iv, taken):
    return any(a < d and c < b for a, b in iv for c, d in taken)


def layout(operands, wide, placement, es):
    """Place the operands of one case.  operands: [(name, rows, cols, element size)]; wide: the names that take the placement's wide
    stride (the others stay contiguous in the low zone).  Wide operands with the same row count are column slices of one wide matrix;
    one with another row count (the record buffer) gets a stride of its own and is slid until none of its rows meets another's.
    Returns {name: View}."""
    views, low = {}, GUARD
    taken = []
    groups = {}
    for name, rows, cols, oes in operands:
        if name in wide:
            groups.setdefault(rows, []).append((name, cols, oes))
        else:
            views[name] = View(name, rows, cols, oes, low, cols * oes)
            low += -(-rows * cols * oes // 4096) * 4096 + GUARD
    assert low <= B31, "compact operands must stay in the low zone"
    start = BASE[es]
    for rows, ops in groups.items():
        width = sum(-(-c * e // 256) * 256 + 256 for _, c, e in ops)     # column slices 256 bytes apart
        rec = all(n == "rec" for n, _, _ in ops)                          # float2 records: 8-byte rows
        ld, k = stride_for(rows, min(c * e for _, c, e in ops), placement, es, 8 if rec else 16, not rec)
        assert ld >= width, (ld, width)
        off = start
        while True:
            col, ivs = 0, []
            for name, c, e in ops:
                ivs += View(name, rows, c, e, off + col, ld).intervals()
                col += -(-c * e // 256) * 256 + 256
            if not _overlaps(ivs, taken):
                break
            off += 4096
            assert off < start + 64 * MIB
        col = 0
        for name, c, e in ops:
            views[name] = View(name, rows, c, e, off + col, ld, k, True)
            col += -(-c * e // 256) * 256 + 256
        taken += ivs
        start = off + width + 4096                           # (the next group's rows interleave with this one's anyway)
    return views


def arena_need(views, es):
    """Bytes the arena must have for this layout: base + max(extent, 2**32) + 64 kB (ES = 4: base + max(extent, 2**33))."""
    need = BASE[es] + (B32 + GUARD if es == 2 else 1 << 33)
    for v in views.values():
        if v.wide:
            need = max(need, v.off + v.extent + GUARD)
    return need


def place(specs, es):
    """Hand-made strides: specs [(name, rows, cols, element size, row stride in bytes or None = contiguous in the low zone)].  Wide
    operands start at the arena's base and are slid (4 kB steps) until no two rows meet."""
    views, low, taken, start = {}, GUARD, [], BASE[es]
    for name, rows, cols, oes, ld in specs:
        if ld is None:
            views[name] = View(name, rows, cols, oes, low, cols * oes)
            low += -(-rows * cols * oes // 4096) * 4096 + GUARD
            continue
        off = start
        while _overlaps(View(name, rows, cols, oes, off, ld).intervals(), taken):
            off += 4096
            assert off < start + 64 * MIB
        views[name] = View(name, rows, cols, oes, off, ld, None, True)
        taken += views[name].intervals()
        start = off + -(-cols * oes // 256) * 256 + GUARD
    assert low <= B31
    return views


# address arithmetic a kernel could get wrong, applied to a TRUE byte offset (from the operand's pointer) of an operand of element
# size es: the byte offset the defective kernel would use instead
DEFECTS = {
    "uint32_byte_offset": lambda off, es: off & 0xFFFFFFFF,
    "int32_byte_offset": lambda off, es: ((off & 0xFFFFFFFF) ^ B31) - B31,
    "uint32_element_index": lambda off, es: ((off // es) & 0xFFFFFFFF) * es,
    "int32_element_index": lambda off, es: ((((off // es) & 0xFFFFFFFF) ^ B31) - B31) * es,
}


def touched(view, defect=None):
    """Arena offsets of the first and last byte of every row as a kernel with `defect` (None: a correct one) addresses them."""
    f = (lambda o, e: o) if defect is None else DEFECTS[defect]
    out = []
    for r in range(view.rows):
        for o in (r * view.ld, r * view.ld + view.row_bytes - view.es):
            out.append(view.off + f(o, view.es))
    return out


def clamped_records(view):
    """Rows a buffer descriptor whose record count was clamped to 2**31 - 1 (with no guard in the launcher) can still reach: the
    hardware returns zero / drops the store beyond.  A correct launch reaches every row."""
    return [r for r in range(view.rows) if r * view.ld + view.row_bytes <= B31 - 1]


def attn_batch_split(nb, kv_batch_bytes, defect=False):
    """The batch ranges mmd_attn_fwd's DMA-staged path launches (mmd_attn.hip: attn_fwd_impl): `per` batches whose K/V stay below 2 GiB.
    defect: the split dropped - one launch whose descriptor holds (int)(nb * kv_batch_bytes)."""
    if defect:
        return [(0, nb)]
    per = min(nb, (B31 - 1) // kv_batch_bytes)
    return [(n0, min(nb, n0 + per)) for n0 in range(0, nb, per)]


# ------------------------------------------------------------------------------------------------- case tables (existing small cases)
def _c(id, entry, **kw):
    d = dict(id=id, entry=entry, dt="bf16", tile=0, taps="1", dims=(1, 1, 1), res=True, stats=False, gn=None, act=True)
    d.update(kw)
    return d


# conv_gemm family.  Shapes: errbound.conv_cases() / strip_cases() / GN_LOADER_CASE, errbound_fwd.GEMM_RECORD_CASES / CHAIN_CASES,
# tests/test_strip_gpu.py::test_strip_fused_groupnorm (the two with whole 64-row records), the smallest geometry with records of
# tests/test_skipfuse_gpu.py (GEOMS[1]) and tests/test_restail_gpu.py (CASES[0]).  gn = (S, Tn).
GEMM_CASES = [
    _c("t64-bf16-1x1-77x96x72", "mmd_conv_gemm", tile=64, M=77, Cin=96, Cout=72),
    _c("t128-bf16-1x1-77x96x72", "mmd_conv_gemm", tile=128, M=77, Cin=96, Cout=72),
    _c("t64-f32-1x1-77x96x72", "mmd_conv_gemm", tile=64, dt="f32", M=77, Cin=96, Cout=72),
    _c("t128-f32-1x1-77x96x72", "mmd_conv_gemm", tile=128, dt="f32", M=77, Cin=96, Cout=72),
    _c("t129-bf16-1x1-293x256x264", "mmd_conv_gemm", tile=129, M=293, Cin=256, Cout=264),
    _c("t132-bf16-1x1-293x256x264", "mmd_conv_gemm", tile=132, M=293, Cin=256, Cout=264),
    _c("t129-f32-1x1-293x256x264", "mmd_conv_gemm", tile=129, dt="f32", M=293, Cin=256, Cout=264),
    _c("t132-f32-1x1-293x256x264", "mmd_conv_gemm", tile=132, dt="f32", M=293, Cin=256, Cout=264),
    _c("t129-bf16-temporal-2x16x6", "mmd_conv_gemm", tile=129, M=192, Cin=64, Cout=72, taps="t3", dims=(16, 6, 1)),
    _c("t130-bf16-halo-3x8x16-64-96", "mmd_conv_gemm", tile=130, M=384, Cin=64, Cout=96, taps="9", dims=(3, 8, 16)),
    _c("t130-f32-halo-3x8x16-64-96", "mmd_conv_gemm", tile=130, dt="f32", M=384, Cin=64, Cout=96, taps="9", dims=(3, 8, 16)),
    _c("t133-bf16-halo16-2x16x32", "mmd_conv_gemm", tile=133, M=1024, Cin=256, Cout=128, taps="9", dims=(2, 16, 32)),
    _c("t131-strip-1x1-288x128x64", "mmd_conv_gemm", tile=131, M=288, Cin=128, Cout=64),
    _c("t131-strip-1x1-288x256x192", "mmd_conv_gemm", tile=131, M=288, Cin=256, Cout=192),
    _c("t131-strip-1x1-288x384x96", "mmd_conv_gemm", tile=131, M=288, Cin=384, Cout=96),
    _c("t131-strip-1x1-608x512x96-nores", "mmd_conv_gemm", tile=131, M=608, Cin=512, Cout=96, res=False),
    _c("t131-strip-temporal-2x5x24", "mmd_conv_gemm", tile=131, M=240, Cin=128, Cout=96, taps="t3", dims=(5, 24, 1)),
    _c("t64-bf16-records-256x64x96", "mmd_conv_gemm_stats", tile=64, M=256, Cin=64, Cout=96, stats=True),
    _c("t128-f32-records-256x64x96", "mmd_conv_gemm_stats", tile=128, dt="f32", M=256, Cin=64, Cout=96, stats=True),
    _c("t129-bf16-records-256x256x192", "mmd_conv_gemm_stats", tile=129, M=256, Cin=256, Cout=192, stats=True),
    _c("t131-records-6x256x384x1152", "mmd_conv_gemm_stats", tile=131, M=1536, Cin=384, Cout=1152, stats=True),
    _c("t131-records-5x320x128x64", "mmd_conv_gemm_stats", tile=131, M=1600, Cin=128, Cout=64, stats=True),
    _c("gn-t128-3x400x256x256", "mmd_gn_conv1x1", tile=128, M=1200, Cin=256, Cout=256, gn=(3, 400)),
    _c("gn-t131-3x400x256x256", "mmd_gn_conv1x1", tile=131, M=1200, Cin=256, Cout=256, gn=(3, 400)),
    _c("gn-t128-records-2x128x128x128", "mmd_gn_conv1x1_stats", tile=128, M=256, Cin=128, Cout=128, gn=(2, 128), stats=True),
    _c("gn-t131-records-6x256x384x1152", "mmd_gn_conv1x1_stats", tile=131, M=1536, Cin=384, Cout=1152, gn=(6, 256), stats=True, act=False, res=False),
    _c("gn-t131-records-5x320x128x64", "mmd_gn_conv1x1_stats", tile=131, M=1600, Cin=128, Cout=64, gn=(5, 320), stats=True, res=False),
    _c("gnhalo-t130-3x8x16-64-96", "mmd_gn_conv_gemm", tile=130, M=384, Cin=64, Cout=96, taps="9", dims=(3, 8, 16), gn=(3, 128)),
    _c("gnhalo-t133-2x16x32", "mmd_gn_conv_gemm", tile=133, M=1024, Cin=256, Cout=128, taps="9", dims=(2, 16, 32), gn=(2, 512)),
    _c("skip-384x3-K128+256-N128", "mmd_gn_conv1x1_skip", M=384, Cin=128, K2=256, Cout=128, gn=(3, 128), stats=True, res=False),
    _c("rtail-2x192-K256+128-N256", "mmd_res_tail", M=384, Cin=256, K2=128, Cout=256, gn=(2, 192), stats=True, res=False),
]


def gemm_operands(c):
    """[(name, rows, cols, element size)] of the strided operands of a GEMM-family case."""
    es = ES[c["dt"]]
    ops = [("A", c["M"], c["Cin"], es)]
    if "K2" in c:
        ops.append(("X2", c["M"], c["K2"], es))
    if c["res"]:
        ops.append(("R", c["M"], c["Cout"], es))
    ops.append(("Y", c["M"], c["Cout"], es))
    if c["stats"]:
        ops.append(("rec", c["M"] // 64, c["Cout"] // 4 * 2, 4))
    return ops


def gemm_variants(c):
    """The wide-operand sets of a case: each strided operand in turn, then all together.  mmd_res_tail compares the WHOLE address ranges
    of h / x with Y's (interleaved rows of one wide matrix count as overlapping and are refused), so its last set leaves Y compact."""
    names = [o[0] for o in gemm_operands(c)]
    together = tuple(n for n in names if not (c["entry"] == "mmd_res_tail" and n == "Y"))
    return [(n,) for n in names] + [together]


PLACEMENTS = ("A", "B", "C")


def gemm_cut_unit(c):
    """The test's own model of the row unit at which the library cuts a tile-131 launch (independent of ops.strip_cut_rows)."""
    unit = 256
    if c["gn"]:
        unit = math.lcm(unit, c["gn"][1])
    if c["taps"] != "1":
        unit = math.lcm(unit, c["dims"][0] * c["dims"][1] * c["dims"][2])
    return unit


def gemm_expect(c, views):
    """What the LIMITS table says this launch does at this layout: (behaviour, the limit's name for the refusal message)."""
    entry, tile = c["entry"], c["tile"]
    if entry == "mmd_gn_conv1x1_skip":
        return ("refuses", "4 GB") if c["M"] * views["Y"].ld >= B32 - 1 else ("computes", None)
    if entry == "mmd_res_tail":
        return "computes", None
    if tile == 133:
        frame = (c["dims"][1] * c["dims"][2] - 1) * views["A"].ld + views["A"].row_bytes
        return ("refuses", "2 GB") if frame >= B31 - 1 else ("computes", None)
    if tile == 131:
        rb = max(views[n].ld for n in ("Y", "R") if n in views)
        if c["M"] * rb < B32 - 1:
            return "computes", None
        return ("splits", None) if (B32 - 2) // rb >= gemm_cut_unit(c) else ("refuses", "4 GB")
    return "computes", None


# GroupNorm apply, row bias, copies.  Shapes: errbound_fwd.apply_cases() at 96 channels and Tn = 7 (N = 2, HW = 3: per-sample slices of
# 14 rows in all, temporal slices - every third row - of 42), errbound_fwd.ROWBIAS_CASES[0 / 1] (3 samples of 37 rows, 136 channels).
NORM_CASES = [
    dict(id="gn_apply-bf16-96-per_sample-7", entry="mmd_gn_apply", dt="bf16", C=96, kind="per_sample", N=2, Tn=7, HW=3, rows=14),
    dict(id="gn_apply-bf16-96-temporal-7", entry="mmd_gn_apply", dt="bf16", C=96, kind="temporal", N=2, Tn=7, HW=3, rows=42),
    dict(id="gn_apply-f32-96-per_sample-7", entry="mmd_gn_apply", dt="f32", C=96, kind="per_sample", N=2, Tn=7, HW=3, rows=14),
    dict(id="gn_apply-f32-96-temporal-7", entry="mmd_gn_apply", dt="f32", C=96, kind="temporal", N=2, Tn=7, HW=3, rows=42),
    dict(id="add_rowbias-bf16-3x37x136", entry="mmd_add_rowbias", dt="bf16", C=136, N=3, rps=37, rows=111),
    dict(id="add_rowbias-f32-3x37x136", entry="mmd_add_rowbias", dt="f32", C=136, N=3, rps=37, rows=111),
    dict(id="copy2d-bf16-111x136", entry="mmd_copy2d", dt="bf16", C=136, rows=111),
    dict(id="copy2d-f32-111x136", entry="mmd_copy2d", dt="f32", C=136, rows=111),
    # errbound_bwd.gn_cases() at 96 channels, Tn = 7 (the statistics pass; its outputs are contiguous [S, C] tables: only x is strided)
    dict(id="gn_stats-bf16-96-per_sample_film-7", entry="mmd_gn_stats", dt="bf16", C=96, kind="per_sample_film", N=2, Tn=7, HW=3, rows=14, ops=[("X", 14, 96, 2)]),
    dict(id="gn_stats-bf16-96-temporal-7", entry="mmd_gn_stats", dt="bf16", C=96, kind="temporal", N=2, Tn=7, HW=3, rows=42, ops=[("X", 42, 96, 2)]),
    dict(id="gn_stats-f32-96-temporal-7", entry="mmd_gn_stats", dt="f32", C=96, kind="temporal", N=2, Tn=7, HW=3, rows=42, ops=[("X", 42, 96, 4)]),
    # errbound_fwd.small_cases(): 128 channels, temporal slices of 5 rows (N = 3, HW = 7)
    dict(id="gn_small-bf16-128-temporal-5", entry="mmd_gn_small", dt="bf16", C=128, kind="temporal", N=3, Tn=5, HW=7, rows=105),
    dict(id="gn_small-f32-128-temporal-5", entry="mmd_gn_small", dt="f32", C=128, kind="temporal", N=3, Tn=5, HW=7, rows=105),
    # errbound_fwd.group_cases(): 128 channels, two samples of 37 rows
    dict(id="gn_group-bf16-128-37", entry="mmd_gn_group", dt="bf16", C=128, kind="per_sample", N=2, Tn=37, HW=1, rows=74),
    dict(id="gn_group-f32-128-37", entry="mmd_gn_group", dt="f32", C=128, kind="per_sample", N=2, Tn=37, HW=1, rows=74),
    # errbound_fwd.finalize_cases() 'strided': 256 channels, 3 slices of 7 records - rec_ld takes the wide stride
    dict(id="gn_finalize_stats-256-3x7", entry="mmd_gn_finalize_stats", dt="f32", C=256, S=3, nrec=7, rows=21, ops=[("rec", 21, 128, 4)]),
    # errbound_fwd.resample_cases(): pool2x2 (with records in bf16: mmd_resample_stats) and up2x2
    dict(id="resample-pool2x2-bf16", entry="mmd_resample_stats", dt="bf16", C=64, NF=4, H=8, W=16, fh=2, fw=2, mode=0, rows=512,
         ops=[("X", 512, 64, 2), ("Y", 128, 64, 2)]),
    dict(id="resample-pool2x2-f32", entry="mmd_resample", dt="f32", C=64, NF=4, H=8, W=16, fh=2, fw=2, mode=0, rows=512,
         ops=[("X", 512, 64, 4), ("Y", 128, 64, 4)]),
    dict(id="resample-up2x2-bf16", entry="mmd_resample", dt="bf16", C=72, NF=2, H=4, W=4, fh=2, fw=2, mode=1, rows=32,
         ops=[("X", 32, 72, 2), ("Y", 128, 72, 2)]),
    # errbound.TEMPORAL_ATTN (13, 4, 2, 32): attention over the 13 frames of each of 4 pixels, N = 2
    dict(id="attn_small-bf16-F13-HW4-h2-ch32", entry="mmd_attn_small_fwd", dt="bf16", C=64, F=13, HW=4, heads=2, ch=32, N=2, rows=104,
         ops=[("X", 104, 192, 2), ("Y", 104, 64, 2)]),
    dict(id="attn_small-f32-F13-HW4-h2-ch32", entry="mmd_attn_small_fwd", dt="f32", C=64, F=13, HW=4, heads=2, ch=32, N=2, rows=104,
         ops=[("X", 104, 192, 4), ("Y", 104, 64, 4)]),
]


# Fused convs (errbound_fused.VCONV_CASES / TATTN_CASES, tests/test_tconv_gpu.py, tests/test_round6_gpu.py ACONV_CASES: the smallest of
# each), stem / head (errbound_fwd.stem_cases() / head_cases() / HEAD_GEMM_CASES: the first case of every kernel variant).  They run
# through the same runner as NORM_CASES.
FUSED_CASES = [
    dict(id="tconv-1x8-256-128", entry="mmd_tconv", dt="bf16", N=1, HW=8, Cin=256, Cout=128, ops=[("X", 128, 256, 2), ("Y", 128, 128, 2)]),
    dict(id="aconv-1x256-128-128-d8", entry="mmd_aconv", dt="bf16", N=1, L=256, Cin=128, Cout=128, dil=8, ops=[("X", 256, 128, 2), ("Y", 256, 128, 2)]),
    dict(id="tattn-1x8", entry="mmd_tattn_block", dt="bf16", name="1x8", ops=[("X", 128, 256, 2), ("Y", 128, 256, 2)]),
    dict(id="vconv-2x4x8-c96-silu", entry="mmd_vconv2d1d", dt="bf16", name="2x4x8-c96", gn="silu", sample_rows=512,
         ops=[("X", 1024, 96, 2), ("Y", 1024, 128, 2)]),
    dict(id="vconv-2x4x8-c96-none", entry="mmd_vconv2d1d", dt="bf16", name="2x4x8-c96", gn="none", sample_rows=512,
         ops=[("X", 1024, 96, 2), ("Y", 1024, 128, 2)]),
    dict(id="stem-pixel-2x4x8-c2-bf16", entry="mmd_stem_conv", dt="bf16", name="pixel-2x4x8-c2-bf16", ops=[("Y", 128, 32, 2)]),
    dict(id="stem-strip-2x3x12-bf16", entry="mmd_stem_conv", dt="bf16", name="strip-2x3x12-bf16", ops=[("Y", 144, 64, 2)]),
    dict(id="stem-mfma-3x5x32-o32-bf16", entry="mmd_stem_conv", dt="bf16", name="mfma-3x5x32-o32-bf16", ops=[("Y", 960, 32, 2)]),
    dict(id="stem-strip-3x5x8-f32", entry="mmd_stem_conv", dt="f32", name="strip-3x5x8-f32", ops=[("Y", 240, 64, 4)]),
    dict(id="head-strip-l4-bf16", entry="mmd_head_conv", dt="bf16", name="strip-l4-3x5x8-o3-27-bf16", ops=[("X", 240, 32, 2)]),
    dict(id="head-coop-o4-bf16", entry="mmd_head_conv", dt="bf16", name="coop-o4-27-bf16", ops=[("X", 240, 64, 2)]),
    dict(id="head-plain-c96-bf16", entry="mmd_head_conv", dt="bf16", name="plain-c96-o3-27-bf16", ops=[("X", 240, 96, 2)]),
    dict(id="head-strip-l4-f32", entry="mmd_head_conv", dt="f32", name="strip-l4-3x5x8-o3-27-f32", ops=[("X", 240, 16, 4)]),
    dict(id="head_gemm-o1-27", entry="mmd_head_gemm", dt="bf16", name="o1-27", ops=[("X", 384, 128, 2)]),
]

# Backward (errbound_bwd: COLSUM_SLICES[0] / [2], gn_cases() at 96 channels and Tn = 7, SELF_ATTN_BWD (70, 1, 96, 2), VALU_ATTN_BWD
# (70, 2, 32), TEMPORAL_ATTN_BWD (13, 4, 2, 32), wgrad_cases() '3x3-3x8x16' 128 -> 128 - the transposing 9-tap kernel below its 2 GiB gate
# (placement A), the 128-tile kernel above it (B, C) -, '3x3-2x21x25' 32 -> 40 (errbound_bwd.WGRAD64_BF16_*) and '3x3-2x5x7' 64 -> 96 in fp32 on the 64-tile kernel).  Atomic weight gradients run the
# exact-sum inputs (errbound_bwd.grid_randn), so that bitwise comparison means something.
BWD_CASES = [
    dict(id="colsum-bf16-2x100x96", entry="mmd_colsum_slices", dt="bf16", S=2, Tn=100, C=96, ops=[("X", 200, 96, 2)]),
    dict(id="colsum-f32-2x130x264", entry="mmd_colsum_slices", dt="f32", S=2, Tn=130, C=264, ops=[("X", 260, 264, 4)]),
    dict(id="gn_bwd-bf16-96-per_sample_film-7", entry="mmd_gn_bwd", dt="bf16", C=96, kind="per_sample_film", Tn=7,
         ops=[("X", 14, 96, 2), ("DY", 14, 96, 2), ("DX", 14, 96, 2)]),
    dict(id="gn_bwd-bf16-96-temporal-7", entry="mmd_gn_bwd", dt="bf16", C=96, kind="temporal", Tn=7,
         ops=[("X", 42, 96, 2), ("DY", 42, 96, 2), ("DX", 42, 96, 2)]),
    dict(id="gn_bwd_ws0-f32-96-temporal-7", entry="mmd_gn_bwd_ws0", dt="f32", C=96, kind="temporal", Tn=7,
         ops=[("X", 42, 96, 4), ("DY", 42, 96, 4), ("DX", 42, 96, 4)]),
    dict(id="attn_bwd_mfma-T70-h1-ch96", entry="mmd_attn_bwd_mfma", dt="bf16", T=70, heads=1, ch=96, nb=2,
         ops=[("X", 140, 288, 2), ("O", 140, 96, 2), ("DO", 140, 96, 2), ("DX", 140, 288, 2)]),
    dict(id="attn_bwd-valu-T70-h2-ch32-bf16", entry="mmd_attn_bwd", dt="bf16", T=70, heads=2, ch=32, nb=2,
         ops=[("X", 140, 192, 2), ("O", 140, 64, 2), ("DO", 140, 64, 2), ("DX", 140, 192, 2)]),
    dict(id="attn_bwd-valu-T70-h2-ch32-f32", entry="mmd_attn_bwd", dt="f32", T=70, heads=2, ch=32, nb=2,
         ops=[("X", 140, 192, 4), ("O", 140, 64, 4), ("DO", 140, 64, 4), ("DX", 140, 192, 4)]),
    dict(id="attn_small_bwd-bf16-F13-HW4-h2-ch32", entry="mmd_attn_small_bwd", dt="bf16", F=13, HW=4, heads=2, ch=32, N=2,
         ops=[("X", 104, 192, 2), ("DO", 104, 64, 2), ("DX", 104, 192, 2)]),
    dict(id="wgrad-tr-3x3-3x8x16-128-128", entry="mmd_conv_wgrad", dt="bf16", name="3x3-3x8x16", Cin=128, Cout=128,
         ops=[("DY", 384, 128, 2), ("X", 384, 128, 2)]),
    dict(id="wgrad-64-3x3-2x21x25-32-40-bf16", entry="mmd_conv_wgrad", dt="bf16", name="3x3-2x21x25", Cin=32, Cout=40,
         ops=[("DY", 1050, 40, 2), ("X", 1050, 32, 2)]),
    dict(id="wgrad-64-3x3-2x5x7-64-96-f32", entry="mmd_conv_wgrad", dt="f32", name="3x3-2x5x7", Cin=64, Cout=96,
         ops=[("DY", 70, 96, 4), ("X", 70, 64, 4)]),
]


# Launches whose outputs are sums of fp32 atomics (mmd_wgrad.hip:67 / :259 dW, :246 / :414 db, :459 colsum, mmd_gn_bwd.hip:97-98 and :124-125 the
# GroupNorm backward's partial sums): their last bit depends on the order of the run, so these are held to the bound - and, on the
# exact-sum inputs (mode True), to exact equality - but not compared bitwise with the compact run.
def atomic_sums(c, mode):
    return (c["entry"] in ("mmd_conv_wgrad", "mmd_colsum_slices") and mode is False) or c["entry"] in ("mmd_gn_bwd", "mmd_gn_bwd_ws0")


def fused_expect(c, views):
    """mmd_vconv2d1d: one sample's rows of X below 2 GiB (mmd_vconv.hip:559); everything else in these lists computes."""
    if c["entry"] == "mmd_vconv2d1d" and (c["sample_rows"] - 1) * views["X"].ld + views["X"].row_bytes >= B31 - 1:
        return "refuses", "2 GB"
    return "computes", None


def wgrad_kernel(c, views):
    """Which weight-gradient kernel the launcher takes (mmd_wgrad.hip:539): the transposing 9-tap kernel only while M * ld * 2 < 2 GiB on both
    operands; the kernels are bitwise equal on exact-sum inputs only, so the comparison with the compact run uses those."""
    if c["dt"] != "bf16" or c["Cin"] < 64 or c["Cout"] < 64:
        return "64"
    M = views["DY"].rows
    return "tr" if max(M * views["DY"].ld, M * views["X"].ld) < B31 - 1 else "128"


# Geometry-only placements: the row stride stays the compact one (ld = C plus the few columns of padding that let a used row cross the
# boundary) and the extent comes from the Geom's own 64-bit fields - outer_stride alone (per-sample / spatial form: slice s at
# row s * outer_stride; temporal form: sample n at row n * outer_stride) or tstride alone (temporal form: frame j of a pixel at row
# j * tstride).  (entry, dt, C, kind, N, Tn, HW, which field is wide)
GEOM_CASES = [dict(id=f"{e[4:]}-{dt}-{C}-{kind}-{Tn}-wide-{fld}", entry=e, dt=dt, C=C, kind=kind, N=N, Tn=Tn, HW=HW, field=fld)
              for e, dt, C, N, Tn, HW in (("mmd_gn_stats", "bf16", 96, 2, 7, 3), ("mmd_gn_stats", "f32", 96, 2, 7, 3),
                                          ("mmd_gn_apply", "bf16", 96, 2, 7, 3), ("mmd_gn_apply", "f32", 96, 2, 7, 3),
                                          ("mmd_gn_small", "bf16", 128, 3, 5, 7), ("mmd_attn_small_fwd", "bf16", 64, 2, 13, 4))
              for kind, fld in (("per_sample", "outer_stride"), ("temporal", "outer_stride"), ("temporal", "tstride"))
              if not (e == "mmd_attn_small_fwd" and kind == "per_sample")]


def geom_operands(c):
    """[(name, columns)] of the operands that follow the Geom of a GEOM_CASES row."""
    if c["entry"] == "mmd_gn_stats":
        return [("X", c["C"])]
    if c["entry"] == "mmd_attn_small_fwd":
        return [("X", 3 * c["C"]), ("Y", c["C"])]
    return [("X", c["C"]), ("Y", c["C"])]


def geom_layout(c, placement):
    """(ld in elements, Geom arguments (S, Tn, inner, outer_stride, inner_stride, tstride), row index of every (slice, j) as a list of
    lists, straddling row, {operand: column offset in elements}) for a GEOM_CASES row.  The operands are column slices of rows of ld
    elements (the kernels take one Geom for x and y).  Placement A keeps the extent near 1 GiB; B / C put one used row of every
    operand across 2**31 / 2**32 with a whole used row above it."""
    es = ES[c["dt"]]
    ops_ = geom_operands(c)
    N, Tn, HW, kind, fld = c["N"], c["Tn"], c["HW"], c["kind"], c["field"]
    bd = GIB if placement == "A" else BOUNDARY[placement]
    cols, col = {}, 0
    for name, C in ops_:
        cols[name] = col
        col += C + 8
    narrow = min(C for _, C in ops_)
    for ld in range(col, col + 4096, 8):
        ldb = ld * es
        R = bd // ldb                                        # the row that holds byte bd
        if not 0 < bd - R * ldb < narrow * es:
            continue                                         # (the boundary must fall inside the columns of every operand's row)
        if kind == "per_sample":                             # slice s: rows s * outer + j; the last slice's row Tn - 2 straddles
            outer = (R - (Tn - 2)) // (N - 1)
            if outer * (N - 1) + Tn - 2 != R:
                continue
            geom = (N, Tn, 1, outer, 1, 1)
            rows = [[s * outer + j for j in range(Tn)] for s in range(N)]
        elif fld == "outer_stride":                          # temporal, sample n at n * outer: the last sample's last-but-one row straddles
            outer = (R - (Tn * HW - 2)) // (N - 1)
            if outer * (N - 1) + Tn * HW - 2 != R:
                continue
            geom = (N * HW, Tn, HW, outer, 1, HW)
            rows = [[n * outer + p + j * HW for j in range(Tn)] for n in range(N) for p in range(HW)]
        else:                                                # temporal, frame j at j * t (samples Tn * t apart): row (N - 1, j = Tn - 2, p) straddles
            k = (N - 1) * Tn + Tn - 2
            t, p0 = R // k, R % k
            if p0 >= HW or t < HW:
                continue
            geom = (N * HW, Tn, HW, Tn * t, 1, t)
            rows = [[n * Tn * t + p + j * t for j in range(Tn)] for n in range(N) for p in range(HW)]
        used = sorted(r for sl in rows for r in sl)
        assert R in used and used[-1] > R and len(set(used)) == len(used)
        return ld, geom, rows, R, cols
    raise AssertionError(f"no geometry placement for {c['id']} {placement}")


def norm_operands(c):
    es = ES[c["dt"]]
    if "ops" in c:
        return list(c["ops"])
    if c["entry"] == "mmd_add_rowbias":                      # in place
        return [("X", c["rows"], c["C"], es)]
    return [("X", c["rows"], c["C"], es), ("Y", c["rows"], c["C"], es)]


# entries that compare the WHOLE address ranges of input and output and refuse an overlap (mmd_vconv.hip, mmd_aconv.hip:188, as mmd_res_tail):
# interleaved rows of one wide matrix count as overlapping, so their operands take the wide stride one at a time only
RANGES_APART = ("mmd_vconv2d1d", "mmd_aconv")


def variants(operands, c=None):
    """The wide-operand sets: each strided operand in turn, then all together."""
    names = [o[0] for o in operands]
    together = len(names) > 1 and not (c is not None and c["entry"] in RANGES_APART)
    return [(n,) for n in names] + ([tuple(names)] if together else [])


# Attention forward: errbound.SELF_ATTN (257, 2, 64) - the smallest at head width 64 - and (70, 1, 96); N = 2 batches of G = 2 groups as
# tests/test_elementwise_gpu.py runs them.  (id, entry, T, heads, ch, dt, impl, P rounding: None = 2**-8, 0.0 = none)
ATTN_CASES = [dict(id=f"attn-T257-h2-ch64-bf16-impl{i}", entry="mmd_attn_fwd", T=257, heads=2, ch=64, dt="bf16", impl=i, p_round=0.0 if i == 1 else None)
              for i in (0, 1, 2, 3, 4, 5)]
ATTN_CASES += [dict(id=f"attn-T70-h1-ch96-bf16-impl{i}", entry="mmd_attn_fwd", T=70, heads=1, ch=96, dt="bf16", impl=i, p_round=0.0 if i == 1 else None)
               for i in (0, 1, 2)]
ATTN_CASES += [dict(id="attn-T70-h1-ch96-f32-impl0", entry="mmd_attn_fwd", T=70, heads=1, ch=96, dt="f32", impl=0, p_round=0.0),
               dict(id="attn_lse-T257-h2-ch64-bf16", entry="mmd_attn_fwd_lse", T=257, heads=2, ch=64, dt="bf16", impl=0, p_round=None)]
# the DMA batch split: nb = 3 batches of one group of 257 keys, one batch's K/V just under 1 GiB (per = 2: launches of 2 + 1 batches)
ATTN_SPLIT = dict(id="attn-split-nb3-T257-h2-ch64", entry="mmd_attn_fwd", T=257, heads=2, ch=64, dt="bf16", nb=3)
# ... and nb = 5: every batch below 2 GiB, 5 GiB of K/V in all (past 2**32 with the split still in force)
ATTN_SPLIT5 = dict(ATTN_SPLIT, id="attn-split-nb5-T257-h2-ch64", nb=5)

def attn_operands(c):
    es = ES[c["dt"]]
    rows, C = 2 * 2 * c["T"], c["heads"] * c["ch"]           # N = 2 batches of G = 2 groups of T rows
    return [("QKV", rows, 3 * C, es), ("O", rows, C, es)]


def attn_expect(c, views):
    """(behaviour, limit) of mmd_attn_fwd on this layout (self-attention: K/V rows = the 2 T rows of a batch of the QKV tensor)."""
    kv_batch = 2 * c["T"] * views["QKV"].ld
    dma = c["dt"] == "bf16" and c["ch"] == 64 and c["entry"] == "mmd_attn_fwd" and c["impl"] in (0, 4, 5)
    if not dma:
        return "computes", None
    if kv_batch >= B31 - 1:
        return ("refuses", "2 GB") if c["impl"] in (4, 5) else ("computes", None)      # impl 0: the per-128-query kernel, bitwise equal
    return ("splits", None) if 2 * kv_batch >= B31 - 1 else ("computes", None)


def attn_split_layouts(c):
    """The DMA batch split (ATTN_SPLIT): K/V of one batch just under 1 GiB, so that a launch takes 2 of the 3 batches; Q and O compact,
    then the Q (and, separately, the O) rows of one 2-batch launch spanning more than 2**31 and more than 2**32 bytes."""
    es, T, C = ES[c["dt"]], c["T"], c["heads"] * c["ch"]
    rows = c["nb"] * T
    ld_kv = (GIB - 4096) // T // 16 * 16
    assert (B31 - 1) // (T * ld_kv) == 2
    out = {}
    if c["nb"] > 3:          # every batch below 2 GiB, more than 4 GiB of K/V in all (launches of 2 + 2 + 1 batches); Q and O compact
        return {"kv": place([("KV", rows, 3 * C, es, ld_kv), ("Q", rows, C, es, None), ("O", rows, C, es, None)], es)}
    for tag, ld_q, ld_o in (("kv", None, None), ("kv+q31", -(-B31 // (2 * T - 2)) // 16 * 16 + 16, None), ("kv+q32", -(-B32 // (2 * T - 2)) // 16 * 16 + 16, None),
                            ("kv+o31", None, -(-B31 // (2 * T - 2)) // 16 * 16 + 16), ("kv+o32", None, -(-B32 // (2 * T - 2)) // 16 * 16 + 16)):
        out[tag] = place([("KV", rows, 3 * C, es, ld_kv), ("Q", rows, C, es, ld_q), ("O", rows, C, es, ld_o)], es)
    return out


# Cases whose launch label may differ between the compact run and a wide placement (the bound alone judges there).  The reading pass
# found no kernel that changes family with the size of its address range under a forced tile / impl: the pointer instantiation of
# tiles 129 / 132 and the cut launches of tile 131 carry the same label, and are the same arithmetic.  The list is empty on purpose.
LABEL_MAY_DIFFER = {}


# ------------------------------------------------------------------------------------------------- the arena (GPU)
class Arena:
    """One torch.uint8 allocation filled with PATTERN32; views into it; the exact stray-write check."""

    def __init__(self, es):
        import torch
        self.es, self.nbytes = es, ARENA_BYTES[es]
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.fill()

    def fill(self):
        import torch
        self.buf.view(torch.int32).fill_(PATTERN32)

    def tensor(self, v, dtype):
        """The torch view of a View (dtype's element size must be v.es)."""
        import torch
        assert dtype.itemsize == v.es and v.off % v.es == 0 and v.ld % v.es == 0 and v.off + v.extent <= self.nbytes
        return torch.as_strided(self.buf.view(dtype), (v.rows, v.cols), (v.ld // v.es, 1), v.off // v.es)

    def repattern(self, v):
        import torch
        torch.as_strided(self.buf.view(torch.int16), (v.rows, v.row_bytes // 2), (v.ld // 2, 1), v.off // 2).fill_(PATTERN16)

    def dirty(self):
        """Number of 32-bit words that are not the pattern (0: the arena is untouched), in 256 MiB chunks; on a hit also the byte
        offsets of the first few."""
        import torch
        a = self.buf.view(torch.int32)
        bad = torch.zeros((), dtype=torch.int64, device="cuda")
        step = CHUNK // 4
        for i in range(0, a.numel(), step):
            bad += (a[i:i + step] != PATTERN32).sum()
        n = int(bad)
        where = []
        if n:
            for i in range(0, a.numel(), step):
                idx = torch.nonzero(a[i:i + step] != PATTERN32)[:8].flatten()
                if idx.numel():
                    where = [(i + int(j)) * 4 for j in idx]
                    break
        return n, where
