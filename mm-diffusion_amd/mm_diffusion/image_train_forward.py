"""Differentiable (training-mode) forward of the image super-resolution U-Net: the block walk of ImageUnet._run, eager and built
from the autograd Functions of train_ops.py so that loss.backward() runs the libmmd backward kernels (train_forward.py is the same
for the coupled U-Net).

Mirrors reference image_unet.py:672-698 (forward), 217-252 (ResBlock._forward, both use_scale_shift_norm settings, resblock
up / down), 290-305 (AttentionBlock) and 327-393 (the two qkv channel orders).  Parameters are read in the reference's layouts, so
every .grad lands on the nn.Parameter in the reference's order: the legacy qkv order [head][q|k|v][ch] is turned into the kernels'
[q|k|v][head][ch] by a view permutation of the qkv WEIGHT rows (3C x C elements, not the activations) that autograd undoes on
the way back.
"""
import torch
import torch.nn.functional as F_

from . import ops
from . import train_ops as T
from .ops import Geom


def _pad_cols(x, mult=8):
    c = x.shape[1]
    return x if c % mult == 0 else F_.pad(x, (0, mult - c % mult))


def image_train_forward(model, rows, shape, timesteps):
    """rows: channels-last input rows [N*H*W, Cpad] in the activation dtype (zero-padded to 8 channels; no gradient flows to them),
    shape = (N, in_channels, H, W).  Returns the fp32 output [N, out_channels, H, W] with a grad_fn."""
    P = dict(model.named_parameters())
    N, Cin, Hh, Ww = shape
    assert Hh == Ww, "square images only"
    mc = model.model_channels
    ss = model.use_scale_shift_norm
    plan_in, plan_mid, plan_out = model._plan

    e0 = torch.empty(N, mc, dtype=torch.float32, device=rows.device)
    ops.timestep_embedding(timesteps.contiguous(), mc, e0)
    emb = T.LinearFn.apply(T.SiluFn.apply(T.LinearFn.apply(e0, P["time_embed.0.weight"], P["time_embed.0.bias"])),
                           P["time_embed.2.weight"], P["time_embed.2.bias"])
    semb = T.SiluFn.apply(emb)         # every emb_layers Sequential starts with SiLU (image_unet.py:176-182)

    def gn(x, prefix, rows_per_sample, act, film=None):
        return T.group_norm(x, P[prefix + ".weight"], P[prefix + ".bias"], Geom.per_sample(N, rows_per_sample), act, film=film)

    def conv3(x, prefix, Hc, residual=None):
        return T.conv(x, P[prefix + ".weight"], P[prefix + ".bias"], taps=ops.TAPS_SPATIAL, dims=(N, Hc, Hc), residual=residual)

    def res_block(x, L, Hc):
        _, p, cin, cout, updown = L
        film = T.LinearFn.apply(semb, P[p + ".emb_layers.1.weight"], P[p + ".emb_layers.1.bias"])
        h = gn(x, p + ".in_layers.0", Hc * Hc, True)
        if updown is not None:           # in_rest -> h_upd / x_upd -> in_conv (image_unet.py:223-228)
            mode = 0 if updown == "down" else 1
            h = T.ResampleFn.apply(h, N, Hc, Hc, 2, 2, mode)
            x = T.ResampleFn.apply(x, N, Hc, Hc, 2, 2, mode)
            Hc = Hc // 2 if updown == "down" else Hc * 2
        h = conv3(h, p + ".in_layers.2", Hc)
        if not ss:                       # h + emb_out, then the plain norm (image_unet.py:241-243)
            h = T.RowBiasFn.apply(h, film, Hc * Hc)
        h = gn(h, p + ".out_layers.0", Hc * Hc, True, film=film if ss else None)
        if model.dropout > 0 and model.training:
            h = T.DropoutFn.apply(h, float(model.dropout))
        sk = x if cin == cout else T.conv(x, P[p + ".skip_connection.weight"], P[p + ".skip_connection.bias"])
        return conv3(h, p + ".out_layers.3", Hc, residual=sk), Hc

    def attn_block(x, L, Hc):
        _, p, C, heads = L
        Tn = Hc * Hc
        wq, bq = P[p + ".qkv.weight"], P[p + ".qkv.bias"]
        if not model.use_new_attention_order:      # legacy output rows [head][q|k|v][ch] -> [q|k|v][head][ch]
            ch = C // heads
            wq = wq.reshape(heads, 3, ch, C).permute(1, 0, 2, 3).reshape(3 * C, C, 1)
            bq = bq.reshape(heads, 3, ch).permute(1, 0, 2).reshape(3 * C)
        qkv = T.conv(gn(x, p + ".norm", Tn, False), wq, bq)
        att = T.SelfAttnFn.apply(qkv, heads, "spatial", N, 1, Tn)
        return T.conv(att, P[p + ".proj_out.weight"], P[p + ".proj_out.bias"], residual=x)

    def run_layers(layers, h, Hc):
        for L in layers:
            if L[0] == "stem":
                w = P[L[1] + ".weight"]
                w = F_.pad(w, (0, 0, 0, 0, 0, rows.shape[1] - w.shape[1]))       # input channels padded like the rows (SR model: 6 -> 8)
                h = T.conv(rows, w, P[L[1] + ".bias"], taps=ops.TAPS_SPATIAL, dims=(N, Hc, Hc))
            elif L[0] == "res":
                h, Hc = res_block(h, L, Hc)
            else:
                h = attn_block(h, L, Hc)
        return h, Hc

    h, hs = None, []
    for layers in plan_in:
        h, Hh = run_layers(layers, h, Hh)
        hs.append(h)
    h, Hh = run_layers(plan_mid, h, Hh)
    for layers in plan_out:
        h = T.CatFn.apply(h, hs.pop())
        h, Hh = run_layers(layers, h, Hh)

    # head: GN -> SiLU -> 3x3 conv, output channels padded to a multiple of 8 for the GEMM and sliced back
    Co = model.out_channels
    pad = (-Co) % 8
    h = gn(h, "out.0", Hh * Hh, True)
    w8 = F_.pad(P["out.2.weight"], (0, 0, 0, 0, 0, 0, 0, pad))
    b8 = F_.pad(P["out.2.bias"], (0, pad))
    y = T.conv(h, w8, b8, taps=ops.TAPS_SPATIAL, dims=(N, Hh, Hh))[:, :Co]
    return y.float().reshape(N, Hh, Hh, Co).permute(0, 3, 1, 2).contiguous()


def input_rows(x, dtype):
    """[N, C, H, W] API-layout input -> channels-last rows [N*H*W, C padded to 8] in the activation dtype (plain ImageUnet; the SR model's
    rows come from mmd_bilinear_concat_rows)."""
    N, C, Hh, Ww = x.shape
    return _pad_cols(x.float().permute(0, 2, 3, 1).reshape(-1, C)).to(dtype).contiguous()
