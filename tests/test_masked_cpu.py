"""Masked conditional sampling, the parts that need no GPU: the C ABI of mmd_cond_replace, masking.normalize / prefix_masks, the
refusal of CPU tensors, and the float64 restatement (masked_ref.py) checked against an fp32 emulation and three seeded defects."""
import os
import re

import numpy as np
import pytest
import torch

import masked_ref as R
from conftest import ROOT

SYMBOLS = ("mmd_cond_replace", "mmd_cond_replace_ctr")


# ----------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_bound_and_exported():
    from mm_diffusion import _hip
    hdr = open(os.path.join(ROOT, "include", "mmd.h")).read()
    lib = _hip.lib()
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert name in _hip.EXPORTS and hasattr(lib, name)
        res, args = _hip._PROTOS[name]
        assert len(args) == len(params), (name, params)
        # the two host scalars travel as C floats, the mask stride as a 64-bit integer, the stream last
        for p, a in zip(params, args):
            if p.startswith("float ") and "*" not in p:
                assert a is _hip.f32, (name, p)
            if p.startswith("int64_t ") and "*" not in p:
                assert a is _hip.i64, (name, p)
            if "*" in p:
                assert a is _hip.vp, (name, p)
        assert params[-1] == "void* stream"
    assert hdr.index("int mmd_cond_replace(") < hdr.index("int mmd_cond_replace_ctr(")
    assert "gd:642-720" in hdr[hdr.index("int mmd_cond_replace(") - 1500:hdr.index("int mmd_cond_replace(")]


def test_null_arguments_are_refused_before_any_launch():
    from mm_diffusion import _hip
    lib = _hip.lib()
    rc = lib.mmd_cond_replace(None, None, None, None, 0, None, None, 1.0, 0.0, 4, 1, 1, 1, 8, None)
    assert rc < 0 and b"cond_replace" in lib.mmd_last_error()
    rc = lib.mmd_cond_replace_ctr(None, None, None, None, 0, None, 0, None, None, 1.0, 0.0, 4, 1, 1, 1, 8, None)
    assert rc < 0 and b"cond_replace_ctr" in lib.mmd_last_error()


# ----------------------------------------------------------------------------- masking.normalize
SHAPE = {"video": (2, 4, 3, 5, 6), "audio": (2, 1, 40)}


def _known(**over):
    d = {"video": torch.randn(*SHAPE["video"]), "audio": torch.randn(*SHAPE["audio"])}
    d.update(over)
    return d


def test_normalize_accepts_every_documented_mask_shape():
    from mm_diffusion import masking
    B, F, C, Hh, Ww = SHAPE["video"]
    L = SHAPE["audio"][2]
    for dt in (torch.bool, torch.uint8):
        for vm, vs in ((torch.ones(F, Hh, Ww, dtype=dt), 0), (torch.ones(B, F, Hh, Ww, dtype=dt), F * Hh * Ww)):
            for am, as_ in ((torch.ones(L, dtype=dt), 0), (torch.ones(B, L, dtype=dt), L)):
                out = masking.normalize(_known(), {"video": vm, "audio": am}, SHAPE)
                assert set(out) == {"video", "audio"}
                assert (out["video"].stride, out["audio"].stride) == (vs, as_)
                for k in out:
                    assert out[k].mask.dtype == torch.uint8 and out[k].mask.is_contiguous()
                    assert out[k].known.dtype == torch.float32 and out[k].known.is_contiguous()
    # a missing key, or no mask at all: the whole stream; a stream that is not in `known` is not conditioned
    out = masking.normalize(_known(), {"audio": torch.zeros(L, dtype=torch.bool)}, SHAPE)
    assert out["video"].mask is None and out["video"].stride == 0 and out["audio"].mask is not None
    out = masking.normalize({"video": torch.randn(*SHAPE["video"]).double()}, None, SHAPE)
    assert set(out) == {"video"} and out["video"].mask is None and out["video"].known.dtype == torch.float32
    # values survive: a non-contiguous known tensor and a uint8 mask with values other than 1
    v = torch.randn(2, 4, 3, 6, 5).transpose(3, 4)
    m = (torch.arange(4 * 5 * 6) % 3).to(torch.uint8).reshape(4, 5, 6)
    out = masking.normalize({"video": v}, {"video": m}, SHAPE)
    assert torch.equal(out["video"].known, v) and torch.equal(out["video"].mask, m)


@pytest.mark.parametrize("known,mask,name", [
    (lambda: _known(), lambda: {"video": torch.ones(4, 5, dtype=torch.bool)}, "mask['video']"),                 # wrong rank
    (lambda: _known(), lambda: {"audio": torch.ones(2, 1, 40, dtype=torch.bool)}, "mask['audio']"),             # wrong rank
    (lambda: _known(), lambda: {"video": torch.ones(4, 5, 7, dtype=torch.bool)}, "mask['video']"),              # wrong size
    (lambda: _known(), lambda: {"audio": torch.ones(3, 40, dtype=torch.bool)}, "mask['audio']"),                # wrong batch
    (lambda: _known(), lambda: {"video": torch.ones(4, 5, 6)}, "mask['video']"),                                # float mask
    (lambda: _known(), lambda: {"audio": torch.ones(40, dtype=torch.int64)}, "mask['audio']"),                  # neither bool nor uint8
    (lambda: _known(), lambda: {"image": torch.ones(4, 5, 6, dtype=torch.bool)}, "mask['image']"),              # unknown key
    (lambda: _known(image=torch.randn(2, 3, 5, 6)), lambda: None, "known['image']"),                            # unknown key
    (lambda: {"video": torch.randn(2, 4, 3, 5, 6)}, lambda: {"audio": torch.ones(40, dtype=torch.bool)}, "mask['audio']"),      # no such known
    (lambda: _known(video=torch.randn(3, 4, 3, 5, 6)), lambda: None, "known['video']"),                         # batch differs from shape
    (lambda: _known(audio=torch.randn(2, 1, 41)), lambda: None, "known['audio']"),                              # size differs
    (lambda: _known(audio=torch.zeros(2, 1, 40, dtype=torch.int64)), lambda: None, "known['audio']"),           # not floating point
])
def test_normalize_refuses_and_names_the_entry(known, mask, name):
    from mm_diffusion import masking
    from mm_diffusion._hip import MMDError
    with pytest.raises(MMDError) as e:
        masking.normalize(known(), mask(), SHAPE)
    assert name in str(e.value), str(e.value)


def test_normalize_refuses_an_empty_condition():
    from mm_diffusion import masking
    from mm_diffusion._hip import MMDError
    for known in ({}, None, [torch.zeros(1)]):
        with pytest.raises(MMDError):
            masking.normalize(known, None, SHAPE)


def test_to_device_keeps_a_missing_mask_and_every_shape_and_dtype():
    from mm_diffusion import masking
    B, F, _, Hh, Ww = SHAPE["video"]
    cond = masking.normalize(_known(), {"video": torch.ones(B, F, Hh, Ww, dtype=torch.bool)}, SHAPE)
    out = masking.to_device(cond, "cpu")
    assert set(out) == {"video", "audio"} and out["audio"].mask is None
    for k, c in cond.items():
        assert out[k].stride == c.stride and torch.equal(out[k].known, c.known)
        assert out[k].known.dtype == torch.float32 and out[k].known.shape == c.known.shape and out[k].known.device.type == "cpu"
    m = out["video"].mask
    assert m.dtype == torch.uint8 and m.shape == cond["video"].mask.shape and torch.equal(m, cond["video"].mask)
    assert masking.to_device({}, "cpu") == {}


@pytest.mark.parametrize("vs,as_", [((8, 3, 16, 16), (1, 512)), ((16, 3, 64, 64), (1, 25600))])
def test_prefix_masks(vs, as_):
    from mm_diffusion import masking
    from mm_diffusion._hip import MMDError
    F, L = vs[0], as_[1]
    for frames in (0, 1, 3, 4, F - 1, F):
        m = masking.prefix_masks(vs, as_, frames)
        assert m["video"].dtype == torch.bool and tuple(m["video"].shape) == (F, vs[2], vs[3])
        assert m["audio"].dtype == torch.bool and tuple(m["audio"].shape) == (L,)
        assert m["video"][:frames].all() and not m["video"][frames:].any()
        n = frames * L // F
        assert m["audio"][:n].all() and not m["audio"][n:].any() and int(m["audio"].sum()) == n
        out = masking.normalize({"video": torch.zeros(2, *vs), "audio": torch.zeros(2, *as_)}, m, {"video": (2, *vs), "audio": (2, *as_)})
        assert out["video"].stride == 0 and out["audio"].stride == 0
    assert int(masking.prefix_masks(vs, as_, 0)["audio"].sum()) == 0 and bool(masking.prefix_masks(vs, as_, F)["audio"].all())
    assert int(masking.prefix_masks((8, 3, 16, 16), (1, 512), 3)["audio"].sum()) == 192
    for frames in (-1, F + 1):
        with pytest.raises(MMDError):
            masking.prefix_masks(vs, as_, frames)


def test_masked_sample_loop_has_no_cpu_fallback():
    from mm_diffusion import multimodal_script_util as msu
    from mm_diffusion._hip import MMDError
    diff = msu.create_gaussian_diffusion(steps=1000, timestep_respacing="4")
    shape = {"video": (1, 8, 3, 16, 16), "audio": (1, 1, 512)}
    known = {"video": torch.zeros(*shape["video"])}
    model = lambda v, a, t, **kw: (v, a)      # noqa: E731
    with pytest.raises(MMDError):             # a CPU device
        diff.masked_sample_loop(model, shape, known, device=torch.device("cpu"))
    with pytest.raises(MMDError):             # CPU tensors for a GPU run: refused before anything is drawn or launched
        diff.masked_sample_loop(model, shape, known, device=torch.device("cuda"))
    with pytest.raises(MMDError):
        diff.masked_sample_loop(model, shape, known, device=torch.device("cuda"), sampler="dpm")


# ----------------------------------------------------------------------------- the float64 restatement
def _cases():
    for shape in R.SMALL + [R.BIG_MEMORY, R.BIG_COUNTER]:
        kinds = R.MASKS if shape in R.SMALL else [("random", True)]
        for kind, per_sample in kinds:
            yield shape, kind, per_sample


def test_fp32_emulation_keeps_the_bound_on_every_gpu_shape():
    tab = R.qtab()
    T = tab.shape[1]
    worst = 0.0
    for shape, kind, per_sample in _cases():
        x, known, eps = R.make_case(shape, seed=1)
        mask, stride = R.make_mask(kind, per_sample, shape)
        t = R.timesteps(shape[0], T)
        A, B = tab[0][t], tab[1][t]
        y, on, bound = R.replace64(x, known, eps, shape, mask, stride, A, B)
        for fused in (False, True):
            got = R.emulate32(x, known, eps, shape, mask, stride, A, B, fused=fused)
            assert R.violations(got, y, bound) == 0, (shape, kind, per_sample, fused)
            assert np.array_equal(got[~on], x[~on])
            if on.any():
                worst = max(worst, float((np.abs(got.astype(np.float64) - y)[on] / np.maximum(bound[on], 1e-300)).max()))
        # the number of known elements is what the mask says: C elements per set cell
        cells = shape[0] * shape[1] * shape[3] if mask is None else int((mask != 0).sum()) * (1 if per_sample else shape[0])
        assert int(on.sum()) == cells * shape[2], (shape, kind, per_sample)
    print("largest |err| / bound of the fp32 emulation:", worst)
    assert 0.0 < worst <= 1.0
    # the paste and the host-scalar form: A = 1, B = 0 gives `known` exactly
    x, known, eps = R.make_case(R.VIDEO, seed=2)
    mask, stride = R.make_mask("random", True, R.VIDEO)
    got = R.emulate32(x, known, eps, R.VIDEO, mask, stride, np.ones(3), np.zeros(3))
    on = R.known_cells(R.VIDEO, mask, stride)
    assert np.array_equal(got[on], known[on]) and np.array_equal(got[~on], x[~on])


@pytest.mark.parametrize("defect", ["channel_in_cell", "batch_stride_ignored", "t_of_sample_0"])
def test_seeded_defects_are_flagged(defect):
    tab = R.qtab()
    shape = R.VIDEO
    x, known, eps = R.make_case(shape, seed=3)
    mask, stride = R.make_mask("random", True, shape)
    t = R.timesteps(shape[0], tab.shape[1])
    A, B = tab[0][t], tab[1][t]
    y, on, bound = R.replace64(x, known, eps, shape, mask, stride, A, B)
    good = R.emulate32(x, known, eps, shape, mask, stride, A, B)
    bad = R.emulate32(x, known, eps, shape, mask, stride, A, B, defect=defect)
    assert R.violations(good, y, bound) == 0
    n = R.violations(bad, y, bound)
    print(defect, "violations:", n, "of", y.size)
    assert n > 0
    # and the restatement with the defect disagrees with the sound one as well
    y_bad, on_bad, _ = R.replace64(x, known, eps, shape, mask, stride, A, B, defect=defect)
    assert not np.array_equal(y_bad, y)
