"""Host side of the streamed ResBlock tail (mmd_res_tail): the selection rule on the model's layer shapes, the engine's order of the
two fused tails, and the new symbol in the header, the binding table and the library."""
import os
import re
from types import SimpleNamespace
from unittest import mock

import torch

from conftest import ROOT

BF = torch.bfloat16
N = 2
# rows per sample: video 16 frames of 32 x 32 / 16 x 16 / 8 x 8 pixels, audio 6400 / 1600 / 400 positions
VIDEO = {"ds2": 16384, "ds4": 4096, "ds8": 1024}
AUDIO = {"ds1": 25600, "ds2": 6400, "ds4": 1600, "ds8": 400}
# (K1 = out-conv input = Cout, K2 = skip input) of the twelve channel-changing blocks per chain below ds1
DEEP = {"ds2": (256, (128, 384, 512, 640)), "ds4": (384, (256, 640, 768, 896)), "ds8": (512, (384, 896, 1024, 1024))}


def _t(rows, C, ld=None, off=0, dtype=BF):
    return torch.empty(rows, ld or C, dtype=dtype)[:, off:off + C]


def _per(rows):
    from mm_diffusion.ops import Geom
    return Geom.per_sample(N, rows)


def test_res_tail_ok_truth_table_on_the_model_layer_shapes():
    """ops.res_tail_ok looks at layer geometry and alignment only; records are asked for wherever the rows are whole 64-row groups
    (the audio ds8 samples have 400 rows: those buffers carry no records)."""
    from mm_diffusion import ops
    from mm_diffusion.ops import Geom
    n = 0
    for rows_of in (VIDEO, AUDIO):
        for lvl, (K1, K2s) in DEEP.items():
            rows = rows_of[lvl]
            for K2 in K2s:
                stats = True if (N * rows) % 64 == 0 else None
                assert ops.res_tail_ok(_t(N * rows, K1), _t(N * rows, K2), K1, _per(rows), stats=stats), (lvl, rows, K1, K2)
                assert not ops.skip_fusable(_t(N * rows, K1), _t(N * rows, K2), K1, _per(rows), stats=stats)
                n += 1
    assert n == 24
    M = N * 25600
    assert ops.res_tail_ok(_t(M, 128), _t(M, 512), 128, _per(25600), stats=True)        # audio ds1, K1 + K2 = 640: the strip refuses it
    assert not ops.skip_fusable(_t(M, 128), _t(M, 512), 128, _per(25600), stats=True)
    # column views: x the right-hand part of a concat buffer, Y a slice of a wider one
    M = N * 4096
    h = _t(M, 384)
    assert ops.res_tail_ok(h, _t(M, 640, 640 + 256, 256), 384, _per(4096), out=_t(M, 384, 768, 384))
    assert not ops.res_tail_ok(_t(M, 384, dtype=torch.float32), _t(M, 640, dtype=torch.float32), 384, _per(4096))      # fp32 mode
    assert not ops.res_tail_ok(_t(N * 1024, 512), _t(N * 1024, 896), 512, Geom.spatial(N, 16, 64))  # per-frame slices (ds8: 64 rows each)
    assert not ops.res_tail_ok(h, _t(M, 640), 384, Geom.temporal(N, 16, 256))                       # per-pixel slices along the frames
    assert not ops.res_tail_ok(h, _t(M // 2, 640), 384, _per(4096))                                 # row counts differ
    assert not ops.res_tail_ok(h, _t(M, 640, 640 + 8, 4), 384, _per(4096))                          # x 8 bytes off a 16-byte boundary
    assert not ops.res_tail_ok(h, _t(M, 640), 384, _per(4096), out=_t(M, 384, 384 + 4))             # Y row stride not a 16-byte multiple
    assert not ops.res_tail_ok(_t(N * 400, 512), _t(N * 400, 896), 512, _per(400), stats=True)      # records need whole 64-row groups
    assert not ops.res_tail_ok(_t(N * 100, 512), _t(N * 100, 896), 512, _per(100))                  # samples below one row block
    assert not ops.res_tail_ok(h, _t(M, 1088), 384, _per(4096))                                     # K2 beyond 1024
    assert not ops.res_tail_ok(h, _t(M, 96), 384, _per(4096))                                       # K2 % 64
    assert not ops.res_tail_ok(_t(M, 320), _t(M, 640), 320, _per(4096))                             # K1 has no instance
    assert not ops.res_tail_ok(h, _t(M, 640), 416, _per(4096))                                      # Cout % 64
    buf = torch.empty(M, 1024, dtype=BF)
    assert not ops.res_tail_ok(buf[:, :384], buf[:, 384:], 384, _per(4096), out=buf[:, 512:896])    # Y inside the buffer x lives in


def test_norm_mode_at_128_channels_follows_the_two_launch_path():
    """At K1 = 128 the record fold of today's out conv depends on whether ITS norm is fused, so the streamed tail's mode must be the
    same decision (ops.gn_fusable); elsewhere the mode is a speed rule between two bitwise-equal paths."""
    from mm_diffusion import ops
    for rows in (25600, 4096, 192):
        h = _t(N * rows, 128)
        assert ops.res_tail_norm_fused(h, 128, _per(rows), True) == ops.gn_fusable(_per(rows), 128, 128, h, True, act=True)
    assert not ops.res_tail_norm_fused(_t(N * 192, 128), 128, _per(192), True)        # slices below the two-fragment block: gn_apply first


def test_speed_rule_keeps_the_measured_losers_on_two_launches():
    """ops.res_tail_pays: among the accepted launches, the shapes the kernel-level A/B did not show as wins stay on two launches."""
    from mm_diffusion import ops
    assert ops.res_tail_pays(_t(2 * 16384, 256), _t(2 * 16384, 640)) and ops.res_tail_pays(_t(4 * 16384, 256), _t(4 * 16384, 640))
    assert ops.res_tail_pays(_t(4 * 6400, 256), _t(4 * 6400, 128))
    assert ops.res_tail_pays(_t(4 * 4096, 384), _t(4 * 4096, 256)) and ops.res_tail_pays(_t(4 * 25600, 128), _t(4 * 25600, 512))
    assert ops.res_tail_pays(_t(2048, 512), _t(2048, 896)) and not ops.res_tail_pays(_t(2048, 512), _t(2048, 384))
    assert _route(_t(N * 1024, 512), _t(N * 1024, 384), 512) is None and _route(_t(N * 1024, 512), _t(N * 1024, 1024), 512) == "stream"


def _route(h, xs, cout, skip_fuse=True, tail_stream=True):
    """Which fused launch UNetEngine._res_tail records for a channel-changing block (None: the two launches)."""
    from mm_diffusion import engine, ops
    eng = mock.MagicMock()
    eng._rec_slice.return_value = (None, 0)
    eng._stats_for.return_value = None
    eng._gn_affine.return_value = (None, None)
    eng._wb = engine.UNetEngine._wb
    s = SimpleNamespace(cin=xs.shape[1], cout=cout, out_norm="n", out_conv="o", skip="k")
    rows = h.shape[0] // N
    called = []
    with mock.patch.object(ops, "gn_conv1x1_skip", lambda *a, **k: called.append("strip")), \
            mock.patch.object(ops, "res_tail", lambda *a, **k: called.append("stream")), \
            mock.patch.object(engine, "_SKIP_FUSE", skip_fuse), mock.patch.object(engine, "_TAIL_STREAM", tail_stream):
        engine.UNetEngine._res_tail(eng, s, h, xs, _per(rows), None, lambda: _t(h.shape[0], cout))
    assert len(called) <= 1
    return called[0] if called else None


def test_engine_tries_the_strip_fusion_first_and_the_switches_are_independent():
    M = N * 65536
    ds1 = (_t(M, 128), _t(M, 256), 128)                  # a shape ops.skip_fusable takes
    assert _route(*ds1) == "strip"
    assert _route(*ds1, skip_fuse=False) is None         # MMD_SKIP_FUSE=0 keeps its two launches: never the streamed launch instead
    assert _route(*ds1, tail_stream=False) == "strip"
    deep = (_t(N * 4096, 384), _t(N * 4096, 640), 384)
    assert _route(*deep) == "stream"
    assert _route(*deep, skip_fuse=False) == "stream"
    assert _route(*deep, tail_stream=False) is None
    a512 = (_t(N * 25600, 128), _t(N * 25600, 512), 128)
    assert _route(*a512) == "stream" and _route(*a512, tail_stream=False) is None


def test_new_symbol_is_declared_bound_and_exported():
    from mm_diffusion import _hip
    hdr = open(os.path.join(ROOT, "include", "mmd.h")).read()
    declared = set(re.findall(r"\b(mmd_[a-z0-9_]+)\s*\(", hdr))
    assert "mmd_res_tail" in declared and "mmd_res_tail" in _hip.EXPORTS
    proto = re.search(r"int mmd_res_tail\(([^;]*)\);", hdr).group(1)
    assert len(proto.split(",")) == len(_hip._PROTOS["mmd_res_tail"][1]) == 21 and proto.split(",")[-1].strip() == "void* stream"
    assert "`mmd_res_tail`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _hip.lib()
    assert hasattr(lib, "mmd_res_tail")
    # argument errors are reported before anything touches a device: a null operand ...
    assert lib.mmd_res_tail(None, 384, None, None, 1, None, None, None, 640, None, None, None, 384, 256, 128, 384, 640, 384, None, 0, None) < 0
    assert b"res_tail: null pointer" in lib.mmd_last_error()
    # ... and K2 = 1088 (the pointers are only compared and checked for alignment before the shape is refused)
    p = 1 << 20
    assert lib.mmd_res_tail(p, 384, None, None, 1, p, None, p, 1088, p, None, p, 384, 256, 128, 384, 1088, 384, None, 0, None) < 0
    assert b"res_tail: K2 = 1088" in lib.mmd_last_error()
