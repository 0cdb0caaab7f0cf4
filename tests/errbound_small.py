"""Float64 references, element-wise bounds, fp32 emulations and case lists for the small kernels that were held only by whole-tensor
rel-L2 (test infrastructure; plain torch / numpy, no import of the package under test).  tests/test_errbound_small_cpu.py proves the
references and the bounds on the CPU, tests/test_errbound_small_gpu.py holds the kernels to them; both iterate over the lists here.

Notation: U = 2^-24, U16 = 2^-8 (tests/errbound.py); `V` = value + magnitude + rounding count (tests/errbound_expr.py), whose
bound() is n U m for an fp32 evaluation of the expression in any association, with or without fused multiply-adds.

Conditioning path (mmd_misc.hip)
    timestep_embedding: f_k = expf(-logf(10000) k / half), a = t f_k, out = (cos a | sin a | 0).  In V: logf's value 3 ulp
    (K_LOG), the product with k and the quotient by half one rounding each, expf K_EXP with the argument's error carried relatively,
    the product with t one rounding; a's error (up to ~999 * 20 U) enters the sine and the cosine ABSOLUTELY (V.sin / V.cos) beside
    the K_SIN = K_COS roundings of the result.  At t = 0 the argument is exactly 0 and the output exactly (1.., 0..).
    temb_fwd: layer by layer.  With e the embedding and E_e its bound,
        a1 = b0 + W0 e        E_1   = |W0| E_e + (dim + 1) U (|W0| |e| + |b0|)      any-order sum of dim products and the bias
        h  = silu(a1)         E_h   = L E_1 + e_silu(a1)                           L = 1.1 >= sup |silu'| = 1.0998; e_silu = V.silu_f
        raw = b2 + W2 h       E_raw = |W2| E_h + (dim + 1) U (|W2| |h| + |b2|)
        out = silu(raw)       E_out = L E_raw + e_silu(raw)
    linear_fwd: y = b + x W^T, K products and the bias in any order (64 strided chains and a butterfly): (K + 1) U (|x| |W|^T + |b|).

Element-wise training kernels (mmd_misc.hip, mmd_optim.hip)
    silu, forward x sg and `dy` form dy sg (1 + x (1 - sg)) with sg = rcp(1 + __expf(-x)): V.sigmoid_f / V.silu_f.  bf16: the inputs
    are the stored bf16 values, the output one round-to-nearest: U16 (|ref| + e) + e.
    dropout (x mask scale) and cast ((T)(x scale)): one fp32 product and one round-to-nearest-even store - the C expression fixes
    every bit, so the tests assert BIT equality with the same expression in torch; a NaN must stay a NaN (its payload is free).
    mse_grad: 2 (out - target) w[n] / per in V.

AdamW (mmd_adamw_step, mmd_adamw_step_guarded): the kernel's expression in V, ONE step from the state the kernel stored before it.
    The betas, lr, eps, weight decay and EMA rates are the fp32 values the kernel receives.  mmd_adamw_step takes 1 - powf(beta, step)
    on the host in fp32: powf within 1 ulp (K_POWF = 2, what the C library documents), then `1 - pw` in V, whose magnitude 1 + pw
    carries the cancellation at small step counts.  The guarded kernel reads bc1, bc2 and the clip coefficient from the control
    block: the tests read the same three floats back and use them as exact inputs, and hold them to float64 on their own.

Weight pack / gradient unpack: pure data movement, `torch.equal` with permute + .to(dtype); the emulation walks the kernel's tiles
and lanes (pack_ci_tile, the lane split tstep = 64 / nci, pack_find's count over the table) so that a defect lands where the kernel's
would.

Solver helpers (mmd_diffusion.hip: lincomb, lincomb_t; mmd_dpm.hip: clamp_scale, dpm_err): lincomb (ca a, then one fma per present term: product and sum counted apart), lincomb_t
(ca[t] a + cb[t] b) cs[t], clamp_scale clamp(x, -sn, sn) / (sn / max_val) with sn = max(s, 1) (the comparisons are on exact inputs),
dpm_err: e = (hi - lo) / max(atol, rtol max(|lo|, |prev|)) in V (max is 1-Lipschitz: V.max needs no branch), e^2 is exact in double,
the double sum of `per` terms costs per 2^-53 of it: bound = sum (2 |e| b_e + b_e^2) + per 2^-53 sum e^2.
"""
import math

import numpy as np
import torch

import errbound as eb
from errbound_expr import K_LOG, U, V, cat, where          # noqa: F401

U16 = eb.U16
F32, BF16 = torch.float32, torch.bfloat16
K_POWF = 2
SILU_LIP = 1.1
LN1E4 = math.log(10000.0)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def store_bound(ref, e, dtype):
    """bound of a value computed to within e in fp32 and stored in dtype"""
    return e if dtype == F32 else U16 * (ref.abs() + e) + e


def trunc_bf16(x):
    """fp32 -> bf16 by dropping the low 16 bits (the defect; the kernels round to nearest even)"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


# ============================================================================= timestep embedding, temb MLP, linear
EMB_DIMS = (64, 128, 130, 300, 7)          # 64 / 128: the model_channels of the shipped configurations (asserted on the CPU)
EMB_NS = (1, 5, 17)
T_INT, T_FLOAT = (0, 1, 17, 999), (0.25, 131.5, 999.999)


def emb_t(kind, N):
    """timesteps of one kind ('i64', 'i32', 'f32'), N of them cycling through the list from an offset that depends on N"""
    vals = T_FLOAT + (0.0,) if kind == "f32" else T_INT
    v = [vals[(i + N) % len(vals)] for i in range(N)]
    return torch.tensor(v, dtype={"i64": torch.int64, "i32": torch.int32, "f32": F32}[kind])


def emb_cases():
    return [(dim, N, kind) for dim in EMB_DIMS for N in EMB_NS for kind in ("i64", "i32", "f32")]


def emb_ref(t, dim):
    """nn.py:192-210 in float64 on the given timesteps: cat(cos, sin) of t * exp(-ln(10000) k / half), zero-padded to dim"""
    half = dim // 2
    freqs = torch.exp(-LN1E4 * torch.arange(half, dtype=torch.float64) / half)
    args = t.double()[:, None] * freqs[None]
    e = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        e = torch.cat([e, torch.zeros_like(e[:, :1])], dim=-1)
    return e


def emb_V(t, dim, ksin=None):
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64)
    f = (-(V(LN1E4, n=K_LOG) * V(k)) / V(float(half))).exp()
    a = V(t.double()[:, None]) * V(f.v[None], f.m[None], f.n)
    e = cat(a.cos(ksin), a.sin(ksin), 1)
    if dim % 2:
        z = torch.zeros(t.shape[0], 1, dtype=torch.float64)
        e = cat(e, V(z), 1)
    return e


def emu_emb(t, dim, defect=None):
    half = dim // 2
    tv = t.float()
    if defect == "trunc_t":
        tv = tv.trunc()
    k = torch.arange(half, dtype=F32)
    den = float(half - 1) if defect == "half_minus_1" else float(half)
    f = torch.exp(-torch.tensor(LN1E4, dtype=F32) * k / den)
    a = tv[:, None] * f[None]
    parts = [torch.sin(a), torch.cos(a)] if defect == "swap" else [torch.cos(a), torch.sin(a)]
    if dim % 2:
        parts.append(torch.zeros(t.shape[0], 1))
    return torch.cat(parts, dim=-1)


def temb_weights(dim):
    g = gen(3200 + dim)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale          # noqa: E731
    return r(dim, dim, scale=dim ** -0.5), r(dim), r(dim, dim, scale=dim ** -0.5), r(dim)


def silu64(x):
    return x * torch.sigmoid(x)


def temb_ref(t, dim, W0, b0, W2, b2, ksin=None):
    """-> (raw, E_raw, out, E_out) float64 [N, dim] (module docstring)"""
    e = emb_V(t, dim, ksin)
    W0, b0, W2, b2 = (w.double() for w in (W0, b0, W2, b2))
    a1 = e.v @ W0.t() + b0
    E1 = e.bound() @ W0.abs().t() + (dim + 1) * U * (e.v.abs() @ W0.abs().t() + b0.abs())
    h = silu64(a1)
    Eh = SILU_LIP * E1 + V(a1).silu_f().bound()
    raw = h @ W2.t() + b2
    Eraw = Eh @ W2.abs().t() + (dim + 1) * U * (h.abs() @ W2.abs().t() + b2.abs())
    return raw, Eraw, silu64(raw), SILU_LIP * Eraw + V(raw).silu_f().bound()


def silu32(x):
    return x * (1.0 / (1.0 + torch.exp(-x)))


def _chain(W, b, e):
    """b + sum_k W[:, k] e[:, k] as ONE sequential fp32 chain per output (temb_kernel's loops)"""
    a = b[None].expand(e.shape[0], -1).clone()
    for k in range(W.shape[1]):
        a = a + W[:, k][None] * e[:, k:k + 1]
    return a


def emu_temb(t, dim, W0, b0, W2, b2, emb_defect=None):
    e = emu_emb(t, dim, emb_defect)
    raw = _chain(W2, b2, silu32(_chain(W0, b0, e)))
    return raw, silu32(raw)


LIN_NS, LIN_KS, LIN_JS = (1, 8, 9, 17), (100, 128, 2304), (6, 1234)


def linear_cases():
    """(name, N, K, J, bias, backward use)"""
    cases = [(f"N{N}-K{K}-J{J}-{'bias' if b else 'nobias'}", N, K, J, b, False) for K in LIN_KS for J in LIN_JS for N in LIN_NS for b in (True, False)]
    cases.append(("bwd-N9-K1234-J100", 9, 1234, 100, False, True))          # dx = dy W: x = dy [N, 1234], the operand is W.t().contiguous() of a [1234, 100] weight
    return cases


def linear_inputs(N, K, J, bias, bwd):
    g = gen(7 * N + 3 * K + J)
    x = torch.randn(N, K, generator=g)
    if bwd:
        W = torch.randn(K, J, generator=g).t().contiguous()          # the weight of the forward layer is [K, J]; the kernel reads its transpose
    else:
        W = torch.randn(J, K, generator=g)
    return x, W, (torch.randn(J, generator=g) if bias else None)


def linear_ref(x, W, b):
    x, W = x.double(), W.double()
    ref, S = x @ W.t(), x.abs() @ W.abs().t()
    if b is not None:
        ref, S = ref + b.double(), S + b.double().abs()
    return ref, (x.shape[1] + 1) * U * S


def emu_linear(x, W, b, defect=None):
    """linear_kernel: lane l of a wave sums k = l, l + 64, ... in order, then the xor butterfly 32 .. 1, then the bias"""
    N, K = x.shape
    J = W.shape[0]
    steps = -(-K // 64)
    Wp = torch.zeros(J, steps * 64)
    Wp[:, :K] = W
    xp = torch.zeros(N, steps * 64)
    xp[:, :K] = x
    lane = torch.arange(64)
    y = torch.empty(N, J)
    for n in range(N):
        acc = torch.zeros(J, 64)
        for s in range(steps):
            acc = acc + Wp[:, s * 64:(s + 1) * 64] * xp[n, s * 64:(s + 1) * 64][None]
        if defect == "bias_per_lane" and b is not None:
            acc = acc + b[:, None]
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lane ^ o]
        y[n] = acc[:, 0] + (b if b is not None and defect != "bias_per_lane" else 0.0)
    if defect == "drop_sample_8" and N > 8:
        y[8] = y[0]
    return y


# ============================================================================= silu, dropout, cast, mse_grad
SECOND_TRIP_VECS = 4096 * 256 + 37          # more 16-byte vectors (or elements) than the 4096 x 256 threads of an element-wise grid
EDGE = (0.0, -0.0, 88.0, -88.0, 100.0, -100.0, 1e-30, -1e-30)


def ew_sizes(dtype):
    epv = 4 if dtype == F32 else 8
    return (8, 8 * 37, SECOND_TRIP_VECS * epv)


def silu_inputs(n, dtype):
    """x with the edge values at both ends (the far end lies in the second trip of the large case), dy; as stored in dtype"""
    g = gen(n % 1000 + (0 if dtype == F32 else 1))
    x = torch.randn(n, generator=g) * 3
    x[:8] = torch.tensor(EDGE)
    x[-8:] = torch.tensor(EDGE)
    dy = torch.randn(n, generator=g)
    return x.to(dtype), dy.to(dtype)


def silu_ref(x, dy, dtype):
    """-> (ref, bound): forward if dy is None, else dy * silu'(x)"""
    xv = V(x.double())
    if dy is None:
        y = xv.silu_f()
        ref = silu64(xv.v)
    else:
        sg = xv.sigmoid_f()
        y = V(dy.double()) * sg * (1.0 + xv * (1.0 - sg))
        s = torch.sigmoid(xv.v)
        ref = dy.double() * (s * (1 + xv.v * (1 - s)))
    return ref, store_bound(ref, y.bound(), dtype)


def emu_silu(x, dy, dtype, defect=None):
    f = x.float()
    sg = 1.0 / (1.0 + torch.exp(-f))
    if dy is None:
        y = f * sg
    else:
        y = dy.float() * sg * (1.0 + f * (1.0 - sg))
        if defect == "no_x_term_lane3":
            epv = 4 if dtype == F32 else 8
            lane3 = torch.arange(f.numel()) % epv == 3
            y = torch.where(lane3, dy.float() * sg, y)
    if defect == "trunc_store" and dtype == BF16:
        return trunc_bf16(y)
    return y.to(dtype)


def dropout_inputs(n, dtype, mask_kind):
    g = gen(n % 1000 + 11)
    x = (torch.randn(n, generator=g) * 2).to(dtype)
    mask = {"zeros": torch.zeros(n, dtype=torch.uint8), "ones": torch.ones(n, dtype=torch.uint8),
            "random": (torch.rand(n, generator=g) < 0.7).to(torch.uint8)}[mask_kind]
    return x, mask


def dropout_expr(x, mask, scale, defect=None):
    """the kernel's C expression: mask ? x * scale : 0 in fp32, one round-to-nearest-even store"""
    y = torch.where(mask.bool(), x.float() * torch.tensor(scale, dtype=F32), torch.zeros(()))
    return trunc_bf16(y) if defect == "trunc_store" and x.dtype == BF16 else y.to(x.dtype)


def _bits32(*words):
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32).view(torch.float32)


def cast_inputs(src, n):
    """random values behind a head of special ones: exact bf16 ties of both parities, the largest finite fp32 (rounds to inf in
    bf16), +-inf, NaNs whose payload lies in the low 16 bits only (a truncating conversion makes them inf) and with the sign bit set"""
    g = gen(n % 1000 + 21)
    x = torch.randn(n, generator=g) * 5
    if src == F32:
        head = _bits32(0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
                       0x7F800001, 0xFF800001, 0xFFC00000, 0x7FC00000, 0x00000001, 0x80000000, 0x3F807FFF, 0x3F808001)
    else:
        head = _bits32(0x7F7F0000, 0xFF7F0000, 0x7F800000, 0xFF800000, 0x7F810000, 0xFF810000, 0xFFC00000, 0x00010000)
    x[:head.numel()] = head
    return x.to(src) if src == BF16 else x


def cast_expr(x, dst, scale, defect=None):
    y = x.float() * torch.tensor(scale, dtype=F32)
    if dst == F32:
        return y
    if defect == "trunc_store":
        return trunc_bf16(y)
    out = y.to(BF16)
    if defect == "signed_nan_to_zero":
        out = torch.where(torch.isnan(y) & torch.signbit(y), torch.zeros((), dtype=BF16), out)
    return out


def same_bits(got, want):
    """bit equality where `want` is a number; NaN exactly where `want` is NaN (a NaN's payload is not fixed by the C expression)"""
    got, want = got.detach().cpu(), want.cpu()
    nan = torch.isnan(want)
    it = torch.int32 if got.dtype == F32 else torch.int16
    return bool((torch.isnan(got) == nan).all()) and torch.equal(got.view(it)[~nan], want.view(it)[~nan])


def mse_inputs(per, N=3):
    g = gen(per)
    return torch.randn(N, per, generator=g), torch.randn(N, per, generator=g), torch.tensor([0.75, 0.0, 1.5])[:N]


def mse_grad_ref(out, target, w):
    per = out.shape[1]
    y = ((V(out.double()) - V(target.double())).exact(2.0) * V(w.double()[:, None])) / V(float(per))
    ref = 2 * (out.double() - target.double()) * w.double()[:, None] / per
    return ref, y.bound(), y.v


def emu_mse_grad(out, target, w):
    return 2.0 * (out - target) * w[:, None] / float(out.shape[1])


# ============================================================================= AdamW
def f32(x):
    return float(np.float32(x))


HYPER = dict(lr=f32(1e-2), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8))
ADAM_STEPS = (1, 2, 3, 100000)


def adamw_cases():
    """(name, n, gradient scale, weight decay, EMA copies) for mmd_adamw_step; the second-trip size once"""
    cases = [(f"g{gs:g}-wd{wd:g}-ema{ne}", 1000, gs, f32(wd), ne) for gs in (1.0, 1e-9, 0.0) for wd in (0.0, 0.05) for ne in (1, 0)]
    cases.append(("second-trip", SECOND_TRIP_VECS, 1.0, f32(0.05), 1))
    return cases


def adamw_state(n, gs, seed=0):
    g = gen(seed + 5)
    p = torch.randn(n, generator=g)
    return dict(p=p, g=torch.randn(n, generator=g) * gs, m=torch.zeros(n), v=torch.zeros(n))


def bias_corrections(beta1, beta2, step, host=True):
    """1 - beta^step as V: the host's fp32 powf within 1 ulp, then one fp32 subtraction (module docstring)"""
    out = []
    for b in (beta1, beta2):
        pw = torch.tensor(float(b), dtype=torch.float64) ** step
        out.append(1.0 - V(pw, n=K_POWF))
    return out


def adamw_V(p, g, m, v, emas, rates, lr, beta1, beta2, eps, wd, bc1, bc2, clip=None):
    """one step of adamw_kernel / adamw_guarded_kernel on the stored fp32 state -> dict of V: p, m, v, ema0 .."""
    P, G, M, Vv = (V(a.double()) for a in (p, g, m, v))
    lr, beta1, beta2, eps, wd = (V(torch.tensor(float(a), dtype=torch.float64)) for a in (lr, beta1, beta2, eps, wd))
    w = P * (1.0 - lr * wd)
    gi = G if clip is None else G * V(torch.tensor(float(clip), dtype=torch.float64))
    mi = beta1 * M + (1.0 - beta1) * gi
    vi = beta2 * Vv + (1.0 - beta2) * gi * gi
    w = w - lr * (mi / V.of(bc1)) / ((vi / V.of(bc2)).sqrt() + eps)
    out = dict(p=w, m=mi, v=vi)
    for k, (e, r) in enumerate(zip(emas, rates)):
        r = V(torch.tensor(float(r), dtype=torch.float64))
        out[f"ema{k}"] = V(e.double()) * r + w * (1.0 - r)
    return out


def adamw_plain64(p, g, m, v, emas, rates, lr, beta1, beta2, eps, wd, step, clip=1.0):
    """the same step as torch.optim.AdamW states it, plain float64 -> (p, m, v, emas)"""
    p, g, m, v = (a.double() for a in (p, g, m, v))
    g = g * clip
    p = p * (1 - lr * wd)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    p = p - lr * (m / (1 - beta1 ** step)) / ((v / (1 - beta2 ** step)).sqrt() + eps)
    return p, m, v, [e.double() * r + p * (1 - r) for e, r in zip(emas, rates)]


def emu_adamw(p, g, m, v, emas, rates, lr, beta1, beta2, eps, wd, step, clip=None, defect=None):
    """fp32, the kernel's statement order -> dict p, m, v, ema0 .. (new tensors)"""
    t = lambda a: torch.tensor(a, dtype=F32)          # noqa: E731
    lr, beta1, beta2, eps, wd = t(lr), t(beta1), t(beta2), t(eps), t(wd)
    bc1 = t(1.0) - torch.pow(beta1, t(float(step)))
    bc2 = t(1.0) - torch.pow(beta2, t(float(step)))
    if defect == "no_bc2":
        bc2 = t(1.0)
    w = p * (t(1.0) - lr * wd)
    gi = g if clip is None else g * t(clip)
    mi = beta1 * m + (t(1.0) - beta1) * gi
    vi = beta2 * v + (t(1.0) - beta2) * gi * gi
    den = torch.sqrt(vi / bc2 + eps) if defect == "eps_in_sqrt" else torch.sqrt(vi / bc2) + eps
    w = w - lr * (mi / bc1) / den
    out = dict(p=w, m=mi, v=v.clone() if defect == "v_not_stored" else vi)
    src = p if defect == "ema_old_p" else w
    for k, (e, r) in enumerate(zip(emas, rates)):
        out[f"ema{k}"] = e * t(r) + src * (t(1.0) - t(r))
    return out


# ============================================================================= weight pack / gradient unpack
PK_CO, PK_ROW, PK_NT_MAX = 32, 216, 27
PACK_GAP = 221                                   # sentinel elements in front of, between and behind the weights (odd: nothing stays aligned)
PACK_SHAPES = [(128, 3, 9), (128, 1, 3),         # the stems: one tile narrower than a vector
               (6, 128, 27),                     # a head: the 8-channel tile
               (40, 200, 9),                     # Cout tail of 8 rows; Cin tail of 8 behind twelve 16-wide tiles
               (33, 70, 3),                      # a 64-wide tile, then a 6-wide one: tstep = 10 does not divide 64
               (32, 24, 5),                      # 24 of the 32 lanes of a tap in use
               (64, 213, 1)]                     # the 208-wide tile and a tail of 5
PACK_MANY = [(1 + i % 7, 1 + i % 5, (1, 3, 9)[i % 3]) for i in range(300)]          # 300 one-block weights: pack_find's second trip
# the list tests/test_round6_gpu.py::test_weight_pack_and_grad_unpack_tiles holds the kernels to today
PACK_TODAY = [(128, 3, 27), (3, 128, 27), (128, 1, 3), (2, 128, 3), (256, 384, 9), (40, 24, 3), (512, 512, 1), (33, 17, 9), (384, 640, 3)]


def pack_ci_tile(nt):
    c = PK_ROW // nt
    return c & ~15 if c >= 16 else c


def pack_blocks(Cout, Cin, nt):
    if Cout <= 0 or Cin <= 0 or nt <= 0 or nt > PK_NT_MAX:
        return -1
    ct = pack_ci_tile(nt)
    return -(-Cout // PK_CO) * -(-Cin // ct)


def pack_layout(shapes, gap=PACK_GAP):
    """offsets of the weights in one flat buffer with `gap` sentinel elements in front of, between and behind them -> (offsets, total)"""
    offs, off = [], gap
    for Cout, Cin, nt in shapes:
        offs.append(off)
        off += Cout * Cin * nt + gap
    return offs, off


def pack_weights(shapes, seed=0):
    g = gen(seed + 31)
    return [torch.randn(*s, generator=g) for s in shapes]


def pack_expected(ws, shapes, dtype):
    """(fwd, bwd) flat buffers: NaN sentinels, permute + .to(dtype) at each weight's offset"""
    offs, total = pack_layout(shapes)
    fwd, bwd = (torch.full((total,), float("nan"), dtype=dtype) for _ in range(2))
    for w, (Cout, Cin, nt), off in zip(ws, shapes, offs):
        fwd[off:off + w.numel()] = w.permute(0, 2, 1).reshape(-1).to(dtype)
        bwd[off:off + w.numel()] = w.permute(1, 2, 0).reshape(-1).to(dtype)
    return fwd, bwd


_lane_maps = {}


def _lane_map(nci, nt, ct, defect):
    """the (tap, ci) pairs the 64 lanes of a wave visit in the forward-operand loop of pack_weights_kernel / the load loop of
    unpack_grads_kernel, as two index arrays"""
    key = (nci, nt, ct, defect)
    if key not in _lane_maps:
        w = 8 if defect == "tstep8" and nci == 6 else nci
        lim = ct if defect == "tail_full" and nci < ct else w
        tstep = 1 if w >= 64 else 64 // w
        cstep = w if tstep > 1 else 64
        taps, cis = [], []
        for lane in range(64):
            lt, lci = divmod(lane, w)
            if lt >= tstep:
                continue
            for tap in range(lt, nt, tstep):
                for ci in range(lci, lim, cstep):
                    taps.append(tap)
                    cis.append(ci)
        _lane_maps[key] = (torch.tensor(taps), torch.tensor(cis))
    return _lane_maps[key]


def _tiles(shapes, select=None, defect=None):
    """every block of one launch -> (weight index, co0, ci0, nco, nci, ct): pack_find + pack_tile.  select: the weights of a
    per-bucket table.  defect 'one_trip': pack_find counts only the first 256 descriptors"""
    idx = list(range(len(shapes))) if select is None else list(select)
    starts, b = [], 0
    for i in idx:
        starts.append(b)
        b += pack_blocks(*shapes[i])
    starts = np.array(starts)
    for block in range(b):
        seen = starts[:256] if defect == "one_trip" else starts
        j = int((seen <= block).sum()) - 1
        Cout, Cin, nt = shapes[idx[j]]
        ct = pack_ci_tile(nt)
        tiles_ci = -(-Cin // ct)
        tb = block - int(starts[j])
        co0, ci0 = (tb // tiles_ci) * PK_CO, (tb % tiles_ci) * ct
        nco, nci = min(PK_CO, Cout - co0), min(ct, Cin - ci0)
        if nco <= 0:
            continue                          # every loop of the kernel is empty
        yield idx[j], co0, ci0, nco, nci, ct


def emu_pack(ws, shapes, dtype, defect=None):
    offs, total = pack_layout(shapes)
    fwd, bwd = (torch.full((total,), float("nan"), dtype=dtype) for _ in range(2))
    for i, co0, ci0, nco, nci, ct in _tiles(shapes, defect=defect):
        Cout, Cin, nt = shapes[i]
        sT = torch.zeros(PK_CO, PK_ROW + 1)
        sT[:nco, :nci * nt] = ws[i][co0:co0 + nco, ci0:ci0 + nci, :].reshape(nco, nci * nt)
        tap, ci = _lane_map(nci, nt, ct, defect)
        c = torch.arange(nco)[:, None]
        fwd[offs[i] + (co0 + c) * nt * Cin + tap[None] * Cin + ci0 + ci[None]] = sT[c, (ci * nt + tap)[None]].to(dtype)
        cc, ii, tt = torch.meshgrid(torch.arange(nco), torch.arange(nci), torch.arange(nt), indexing="ij")
        bwd[offs[i] + (ci0 + ii) * nt * Cout + tt * Cout + co0 + cc] = sT[cc, ii * nt + tt].to(dtype)
    return fwd, bwd


def unpack_inputs(shapes, seed=0):
    """(.grad flat, packed flat): fp32 buffers in the layout of pack_layout, random at the weights, NaN in the gaps"""
    offs, total = pack_layout(shapes)
    g = gen(seed + 41)
    grad, packed = (torch.full((total,), float("nan")) for _ in range(2))
    for (Cout, Cin, nt), off in zip(shapes, offs):
        n = Cout * Cin * nt
        grad[off:off + n] = torch.randn(n, generator=g)
        packed[off:off + n] = torch.randn(n, generator=g)
    return grad, packed


def unpack_expected(grad, packed, shapes, select=None):
    """.grad += permuted(packed) (one fp32 addition), packed = 0, for the selected weights; everything else as it was"""
    offs, _ = pack_layout(shapes)
    grad, packed = grad.clone(), packed.clone()
    for i in (range(len(shapes)) if select is None else select):
        Cout, Cin, nt = shapes[i]
        s = slice(offs[i], offs[i] + Cout * Cin * nt)
        grad[s] = grad[s] + packed[s].view(Cout, nt, Cin).permute(0, 2, 1).reshape(-1)
        packed[s] = 0.0
    return grad, packed


def emu_unpack(grad, packed, shapes, select=None, defect=None):
    offs, _ = pack_layout(shapes)
    grad, packed = grad.clone(), packed.clone()
    for i, co0, ci0, nco, nci, ct in _tiles(shapes, select, defect):
        Cout, Cin, nt = shapes[i]
        sT = torch.zeros(PK_CO, PK_ROW + 1)
        tap, ci = _lane_map(nci, nt, ct, defect)
        c = torch.arange(nco)[:, None]
        src = offs[i] + (co0 + c) * nt * Cin + tap[None] * Cin + ci0 + ci[None]
        sT[c, (ci * nt + tap)[None]] = packed[src]
        if defect != "no_clear":
            packed[src] = 0.0
        run = nci * nt
        dst = offs[i] + ((co0 + c) * Cin + ci0) * nt + torch.arange(run)[None]
        grad[dst] = grad[dst] + sT[:nco, :run]
    return grad, packed


# ============================================================================= lincomb, lincomb_t, clamp_scale, dpm_err
# (ca, cb) rows of tests/test_dpmpp_gpu.py::_x0_case - the +-157.4 pair cancels - and a third coefficient each
LINCOMB_COEFS = [(1.7, -1.3, 0.25), (157.41, -157.40, -0.011), (1.0002, -0.017, 3.5), (3.0, 0.5, -157.40)]
LINCOMB_N = 3 * 3 * 3 * 683


def lincomb_cases():
    """(name, ca, cb or None, cc or None): one, two, three terms, and the first with the third (b absent)"""
    cases = []
    for r, (ca, cb, cc) in enumerate(LINCOMB_COEFS):
        ca, cb, cc = f32(ca), f32(cb), f32(cc)
        cases += [(f"row{r}-a", ca, None, None), (f"row{r}-ab", ca, cb, None), (f"row{r}-abc", ca, cb, cc), (f"row{r}-ac", ca, None, cc)]
    return cases


def lincomb_inputs():
    g = gen(61)
    return tuple(torch.randn(LINCOMB_N, generator=g) * s for s in (1.0, 1.5, 0.7))


def lincomb_ref(a, ca, b, cb, c, cc):
    y = V(ca) * V(a.double())
    ref = ca * a.double()
    if b is not None:
        y, ref = y + V(cb) * V(b.double()), ref + cb * b.double()
    if c is not None:
        y, ref = y + V(cc) * V(c.double()), ref + cc * c.double()
    return ref, y.bound(), y.v


def emu_lincomb(a, ca, b, cb, c, cc, defect=None):
    t = lambda s: torch.tensor(s, dtype=F32)          # noqa: E731
    v = t(ca) * a
    if b is not None:
        v = v + t(cb) * b
    if c is not None and not (defect == "drop_c_without_b" and b is None):
        v = v + t(cc) * c
    return v


LT_T = 10


def lincomb_t_cases():
    """(name, per, t kind, has ca / cb / cs / b): the three forms multimodal_gaussian_diffusion.py calls (_lin)"""
    forms = [("a", (True, False, False, False)), ("ab", (True, True, False, True)), ("abs", (True, True, True, True))]
    return [(f"{f}-per{per}-t{tk}", per, tk, has) for f, has in forms for per in (30, 4099) for tk in ("zero", "last", "mixed")]


def lincomb_t_inputs(per, tk, N=3):
    g = gen(per + 71)
    a, b = torch.randn(N, per, generator=g), torch.randn(N, per, generator=g)
    tabs = [torch.randn(LT_T, generator=g) * s for s in (2.0, 1.0, 0.5)]
    t = {"zero": torch.zeros(N, dtype=torch.int64), "last": torch.full((N,), LT_T - 1), "mixed": torch.tensor([4, 0, LT_T - 1])[:N]}[tk]
    return a, b, tabs, t


def lincomb_t_ref(a, b, tabs, t, has):
    ca, cb, cs = (tab.double()[t][:, None] if h else None for tab, h in zip(tabs, has[:3]))
    y = V(ca) * V(a.double()) if ca is not None else V(a.double())
    ref = a.double() * (ca if ca is not None else 1.0)
    if has[3]:
        y = y + (V(cb) * V(b.double()) if cb is not None else V(b.double()))
        ref = ref + b.double() * (cb if cb is not None else 1.0)
    if cs is not None:
        y, ref = y * V(cs), ref * cs
    return ref, y.bound(), y.v


def emu_lincomb_t(a, b, tabs, t, has):
    ca, cb, cs = (tab[t][:, None] if h else None for tab, h in zip(tabs, has[:3]))
    v = a * ca if ca is not None else a.clone()
    if has[3]:
        v = v + (b * cb if cb is not None else b)
    return v * cs if cs is not None else v


CLAMP_S = (0.5, 1.0, 37.5)          # below 1 (the floor), 1, large


def clamp_cases():
    return [(f"per{per}-max{mv:g}", per, mv) for per in (30, 4099) for mv in (1.0, 0.5)]


def clamp_inputs(per):
    g = gen(per + 81)
    s = torch.tensor(CLAMP_S)
    sn = s.clamp_min(1.0)[:, None]
    x = torch.randn(len(CLAMP_S), per, generator=g) * sn * 1.2          # inside and outside
    x[:, 0], x[:, 1] = sn[:, 0], -sn[:, 0]                             # on the threshold
    x[:, 2], x[:, 3] = s, -s                                           # on the raw s: inside for s < 1
    return x, s


def clamp_ref(x, s, max_val, floor=True):
    sn = s.double().clamp_min(1.0) if floor else s.double()
    sn = sn[:, None]
    c = torch.minimum(torch.maximum(x.double(), -sn), sn)
    y = V(c) / (V(sn) / V(torch.tensor(float(max_val), dtype=torch.float64)))
    return c / (sn / max_val), y.bound().expand_as(c), y.v


def emu_clamp(x, s, max_val, defect=None):
    sn = (s if defect == "no_floor" else s.clamp_min(1.0))[:, None]
    return torch.minimum(torch.maximum(x, -sn), sn) / (sn / torch.tensor(max_val, dtype=F32))


DPM_ATOL, DPM_RTOL = f32(0.0078), f32(0.05)
DPM_PERS = (30, 4096, 3 * 4096 + 5)


def dpm_err_inputs(per, N=3):
    """lo ~ N(0, 1): rtol |lo| passes atol at |lo| = 0.156, so both regimes occur; prev unlike hi"""
    g = gen(per + 91)
    lo = torch.randn(N, per, generator=g)
    lo[:, ::7] *= 0.05                                    # atol-dominated elements
    hi = lo + 0.02 * torch.randn(N, per, generator=g)
    prev = torch.randn(N, per, generator=g) * 3
    prev[:, ::7] *= 0.01
    return hi, lo, prev


def dpm_err_ref(hi, lo, prev, atol=DPM_ATOL, rtol=DPM_RTOL):
    """-> (sum [N] float64, bound [N]) of one call on a zeroed `out`"""
    h, l, p = (V(a.double()) for a in (hi, lo, prev))
    delta = (V(torch.tensor(rtol, dtype=torch.float64)) * l.abs().max(p.abs())).max(V(torch.tensor(atol, dtype=torch.float64)))
    e = (h - l) / delta
    plain = ((hi.double() - lo.double()) / torch.clamp_min(rtol * torch.maximum(lo.double().abs(), prev.double().abs()), atol)) ** 2
    assert float((e.v ** 2 - plain).abs().max()) <= 1e-12 * float(plain.max())
    b = e.bound()
    ref = plain.sum(1)
    return ref, (2 * e.v.abs() * b + b * b).sum(1) + hi.shape[1] * 2.0 ** -53 * ref


def emu_dpm_err(hi, lo, prev, atol=DPM_ATOL, rtol=DPM_RTOL, defect=None):
    other = hi if defect == "hi_for_prev" else prev
    delta = torch.clamp_min(torch.tensor(rtol, dtype=F32) * torch.maximum(lo.abs(), other.abs()), atol)
    e = (hi - lo) / delta
    return (e.double() ** 2).sum(1)


def dpm_order_inputs(small_at):
    """The input that pins dpm_err's order (atol = 1, rtol = 0, so e = hi): one sample of 3 * 4096 + 5 elements, e = 2^26 at the
    elements 0 and 256 (thread 0 of the block: its sum is 2^53) and e = 1 at the two elements `small_at`.  The tree adds
    s[t] += s[t + o] for o = 128 .. 1: small ones at 128 and 64 meet the large sum one by one, 2^53 + 1 rounds back to 2^53 both
    times -> 2^53; small ones at 64 and 192 meet each other first (o = 128) -> 2^53 + 2."""
    per = 3 * 4096 + 5
    hi = torch.zeros(1, per)
    hi[0, 0] = hi[0, 256] = 2.0 ** 26
    for i in small_at:
        hi[0, i] = 1.0
    return hi, torch.zeros(1, per), torch.zeros(1, per)
