"""Host side of the fused ResBlock tail (mmd_gn_conv1x1_skip): the selection rule on the model's layer shapes and the new symbol in
the header, the binding table and the library."""
import os
import re

import torch

from conftest import ROOT

BF = torch.bfloat16


def _t(rows, C, ld=None, off=0, dtype=BF):
    return torch.empty(rows, ld or C, dtype=dtype)[:, off:off + C]


def test_skip_fusable_truth_table_on_the_model_layer_shapes():
    """ops.skip_fusable looks at layer geometry and alignment only.  Rows are per sample x batch 2: video 16 frames of 64 x 64 / 32 x 32
    / 16 x 16 pixels, audio 25600 / 6400 samples; the channel-changing blocks of the base model around them."""
    from mm_diffusion import ops
    from mm_diffusion.ops import Geom
    N = 2
    per = lambda rows: Geom.per_sample(N, rows)
    table = [
        # (rows per sample, K1 = out-conv input, K2 = skip input, Cout, expected)
        (65536, 128, 256, 128, True),       # ds1 video, up path: concat of two 128-channel tensors
        (65536, 128, 384, 128, True),       # ds1 video: concat 256 + 128
        (25600, 128, 256, 128, True),       # ds1 audio
        (25600, 128, 384, 128, True),
        (25600, 128, 512, 128, False),      # K1 + K2 = 640: beyond the operand registers of a strip
        (16384, 256, 128, 256, False),      # ds2 video, down path 128 -> 256: the out conv runs a two-fragment instance
        (16384, 256, 512, 256, False),      # ds2 video, up path
        (6400, 256, 384, 256, False),       # ds2 audio
        (4096, 384, 256, 384, False),       # ds4 video
        (4096, 128, 256, 128, False),       # right channels, slices below 16384 rows: today's records are folded in the two-fragment order
        (65536, 128, 256, 144, False),      # Cout % 32 != 0
        (65536, 128, 128, 128, False),      # K2 = 128 has no instance
    ]
    for rows, K1, K2, Cout, want in table:
        got = ops.skip_fusable(_t(N * rows, K1), _t(N * rows, K2), Cout, per(rows), stats=True)
        assert got == want, (rows, K1, K2, Cout, got)
    M = N * 65536
    h = _t(M, 128)
    assert ops.skip_fusable(h, _t(M, 384, 384 + 128, 128), 128, per(65536), out=_t(M, 128, 256, 128))        # column views: x in a concat buffer, Y too
    assert not ops.skip_fusable(h, _t(M, 256, 256 + 8, 4), 128, per(65536))                                   # x 8 bytes off a 16-byte boundary
    assert not ops.skip_fusable(h, _t(M, 256), 128, per(65536), out=_t(M, 128, 128 + 4))                      # Y row stride not a 16-byte multiple
    assert not ops.skip_fusable(_t(M, 128, dtype=torch.float32), _t(M, 256, dtype=torch.float32), 128, per(65536))      # fp32 mode
    assert not ops.skip_fusable(h, _t(M, 256), 128, Geom.spatial(N, 16, 4096))                                # per-frame slices
    assert not ops.skip_fusable(h, _t(M // 2, 256), 128, per(65536))                                          # row counts differ
    assert not ops.skip_fusable(_t(N * 16400, 128), _t(N * 16400, 256), 128, per(16400), stats=True)          # records need whole 64-row groups


def test_new_symbol_is_declared_bound_and_exported():
    from mm_diffusion import _hip
    hdr = open(os.path.join(ROOT, "include", "mmd.h")).read()
    declared = set(re.findall(r"\b(mmd_[a-z0-9_]+)\s*\(", hdr))
    assert "mmd_gn_conv1x1_skip" in declared and "mmd_gn_conv1x1_skip" in _hip.EXPORTS
    # 23 arguments in the header's order; the stream comes last as for every entry point
    proto = re.search(r"int mmd_gn_conv1x1_skip\(([^;]*)\);", hdr).group(1)
    assert len(proto.split(",")) == len(_hip._PROTOS["mmd_gn_conv1x1_skip"][1]) == 23 and proto.split(",")[-1].strip() == "void* stream"
    lib = _hip.lib()
    assert hasattr(lib, "mmd_gn_conv1x1_skip")
    # argument errors are reported before anything touches a device: a null operand, and K1 + K2 = 640
    assert lib.mmd_gn_conv1x1_skip(1, None, 0, None, None, 1, 1, 128, None, None, None, 0, 256, None, None, None, 0, 128, 128, 128, None, 0, None) < 0
    assert b"gn_conv1x1_skip" in lib.mmd_last_error()
