"""Value + magnitude + rounding count: the class `V` with which the element-wise tests restate a kernel's fp32 expression in float64
and obtain, beside the value, a bound on what an fp32 evaluation of the same expression may differ by (test infrastructure; plain
torch, no import of the package under test).  Moved here from tests/test_diffusion_core_gpu.py, whose docstring explains the three
fields; used by that file and by tests/errbound_small.py.

    v       the float64 value,
    m >= |v| the summed magnitudes of the terms of the expression (a difference keeps both sides, a quotient and a root keep the
            amplification of their operand),
    n       the number of fp32 roundings so far,
so that an fp32 evaluation in any association, with or without fused multiply-adds, is within n U m of v (U = 2^-24, first order).

Library functions enter as K roundings of their result, K from what the device library promises - the single-precision accuracy of the
OpenCL C specification, in units of U = half an ulp:
    expf   3 ulp  K_EXP  = 6      tanhf  5 ulp  K_TANH = 10      (tests/test_diffusion_core_gpu.py)
    sinf   4 ulp  K_SIN  = 8      cosf   4 ulp  K_COS  = 8       logf  3 ulp  K_LOG = 6
sin / cos: the argument's error passes through with derivative <= 1 and the result carries K roundings of itself:
    |fl(sin(a')) - sin(a)| <= n_a U m_a + K U |sin a| <= (n_a + K) U max(m_a, |sin a|).
Measured on an MI355X with tests/test_errbound_small_gpu.py (timestep_embedding and temb_fwd, every case): the smallest K_SIN = K_COS
at which no element leaves its bound is
    measured count = 0    (with sinf and cosf counted as exact the worst error / bound is 0.177: the rounding of the argument t f, up to
                           999 U, hides the library's own error at every element whose argument is not zero, and at t = 0 the
                           library returns 1 and 0 exactly)
so, as for expf / tanhf, the allowance is the specification's and not what was seen.

silu_f (mmd_common.h: `x * rcp(1 + __expf(-x))`), stated once from the terms tests/errbound_fwd.py and tests/errbound_bwd.py grant:
__expf multiplies the argument by log2(e) (one rounding, U |x| absolute in the exponent), v_exp_f32 is accurate to 1 ulp = 2 U, the
add of 1 rounds once, v_rcp_f32 is accurate to 1 ulp = 2 U:
    e_sg = sg ((1 - sg) (e_x + U |x| + 2 U) + 3 U) + TINY
and the product x sg rounds once more (V's product rule).  TINY = 2^-126: v_exp_f32 and v_rcp_f32 flush results below the normal
range, and __expf(-x) overflows for x < -88.7, where the kernel's sigmoid is 0 and float64's is below TINY.
max: |max(a', b') - max(a, b)| <= max(e_a, e_b).
"""
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
K_EXP, K_TANH = 6, 10          # 3 ulp and 5 ulp, in units of U = half an ulp
K_SIN = K_COS = 8              # 4 ulp
K_LOG = 6                      # 3 ulp


# ------------------------------------------------------------------ value + magnitude + rounding count
class V:
    def __init__(self, v, m=None, n=0):
        self.v = torch.as_tensor(v, dtype=torch.float64)
        self.m = self.v.abs() if m is None else m
        self.n = n

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def bound(self):
        return self.n * U * self.m

    def _sum(self, o, v):
        exact = self.n == 0 and o.n == 0          # one rounding of the result of two exact operands: U |v|, not U (|a| + |b|)
        return V(v, v.abs() if exact else self.m + o.m, self.n + o.n + 1)

    def __add__(self, o):
        o = V.of(o)
        return self._sum(o, self.v + o.v)

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return self._sum(o, self.v - o.v)

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, self.m, self.n)

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, self.m * o.m, self.n + o.n + 1)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        amp = torch.where(o.v == 0, torch.ones_like(o.m), o.m / o.v.abs())
        return V(self.v / o.v, self.m / o.v.abs() * amp, self.n + o.n + 1)

    def exact(self, c):
        """times a power of two"""
        return V(self.v * c, self.m * abs(c), self.n)

    def sqrt(self):
        r = self.v.sqrt()
        return V(r, torch.where(self.v == 0, self.m, r * self.m / self.v.abs().clamp_min(1e-300)), self.n + 1)

    def exp(self):
        r = self.v.exp()
        return V(r, r * self.m.clamp_min(1.0), self.n + K_EXP)

    def tanh(self):
        r = self.v.tanh()
        return V(r, (1 - r * r) * self.m + r.abs(), self.n + K_TANH)

    def sin(self, k=None):
        r = self.v.sin()
        return V(r, torch.maximum(self.m, r.abs()), self.n + (K_SIN if k is None else k))

    def cos(self, k=None):
        r = self.v.cos()
        return V(r, torch.maximum(self.m, r.abs()), self.n + (K_COS if k is None else k))

    def sigmoid_f(self):
        """rcp(1 + __expf(-x)): e_sg of the module docstring as (n + 6) roundings of max(sg, e_sg / ((n + 6) U))"""
        sg = torch.sigmoid(self.v)
        e = sg * ((1 - sg) * (self.bound() + U * self.v.abs() + 2 * U) + 3 * U) + TINY
        n = self.n + 6
        return V(sg, torch.maximum(sg, e / (n * U)), n)

    def silu_f(self):
        return self * self.sigmoid_f()

    def max(self, o):
        o = V.of(o)
        return V(torch.maximum(self.v, o.v), torch.maximum(self.m, o.m), max(self.n, o.n))

    def abs(self):
        return V(self.v.abs(), self.m, self.n)

    def clamp(self, lo, hi):
        return V(self.v.clamp(lo, hi), self.m, self.n)

    def expand_as(self, t):
        return V(self.v.expand_as(t), self.m.expand_as(t), self.n)


def C32(c):
    """a constant the kernel holds in fp32: within one rounding of the double the oracle uses"""
    return V(c, n=1)


def where(mask, a, b):
    a, b = V.of(a), V.of(b)
    return V(torch.where(mask, a.v, b.v), torch.where(mask, a.m, b.m), max(a.n, b.n))


def cat(a, b, dim):
    return V(torch.cat([a.v, b.v], dim), torch.cat([a.m, b.m], dim), max(a.n, b.n))
