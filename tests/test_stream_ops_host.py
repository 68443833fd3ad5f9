"""CPU: the kernels that carry data between the large ones on every refinement iteration -- norm.hip (InstanceNorm,
GroupNorm+ReLU), resample.hip (bilinear resize, 2x2 average pool, mask product, strided copy, convex up-sampling) and
pose.hip (pose update, re-projection, un-projection, filter_flow_by_mask) -- restated in float64, with a per-element
error bound for any fp32 evaluation in the kernel's operation order, the inputs tests/test_gpu_stream_ops.py feeds the
HIP kernels, and the proof that the bounds are neither vacuous (planted defects fall outside) nor unreachable (fp32
references stay inside).

Every bound is built from U = 2**-24 (the unit round-off of one fp32 operation) and magnitude shadows (the same
computation on absolute values); multipliers count operations in the kernel source.  Two forms:

* sums (norms, resize, pool, convex blend): an analytic bound, `chain depth x U x shadow`;
* short straight-line arithmetic (pose update, re- / un-projection, the filter's sample coordinate): `EV`, a value
  with a running error bound -- every fp32 operation of the kernel source is replayed once on float64 values and adds
  U |result| to the errors it propagates.  A fused multiply-add rounds less often than the replay assumes, so the
  contraction the compiler is free to choose stays inside.

expf: the ROCm device-library documents shipped with the toolchain state no error for it; EXP_ULPS = 2 is ASSUMED.
fp32 underflow is outside the model except where a bound says otherwise (convex weights below 2**-126).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle

U = 2.0 ** -24
EXP_ULPS = 2.0                      # assumed (see above); one ulp is at most 2 U relative
F32_MAX = 3.4028234663852886e38
LABEL_PER_SAMPLE, DEPTH_LINEAR = 1, 2


def f64(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; an element with bound 0 must be exact; NaN in got where ref is finite
    counts as inf."""
    got, ref, bound = f64(got), f64(ref), np.broadcast_to(f64(bound), f64(ref).shape)
    with np.errstate(all='ignore'):
        err = np.abs(got - ref)
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def measured(name, value):
    print(f'[measured] {name}: {value:.3g}')


# ---------------------------------------------------------------------------------------------- running error bounds
class EV:
    """float64 value(s) `v` of an fp32 computation and a bound `e` on |computed - v|.  Each operation returns the exact
    result of the values, the propagated error, and one rounding U (|v| + e)."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) + e

    @staticmethod
    def _lift(x):
        return x if isinstance(x, EV) else EV(x)

    @staticmethod
    def _rnd(v, e, exact=False):
        with np.errstate(all='ignore'):
            return EV(v, e if exact else e + U * (np.abs(v) + e))

    def __add__(self, o):
        o = EV._lift(o)
        return EV._rnd(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = EV._lift(o)
        return EV._rnd(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = EV._lift(o)
        with np.errstate(all='ignore'):
            return EV._rnd(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = EV._lift(o)
        with np.errstate(all='ignore'):
            v = self.v / o.v
            den = np.abs(o.v) - o.e
            e = np.where(den > 0, (self.e + np.abs(v) * o.e) / np.where(den > 0, den, 1.0), np.inf)
            e = np.where((self.e == 0) & (o.e == 0), 0.0, e)
        return EV._rnd(v, e)

    def sqrt(self):
        with np.errstate(all='ignore'):
            v = np.sqrt(self.v)                                     # |sqrt a' - sqrt a| <= min(e / sqrt a, sqrt e)
            e = np.minimum(np.where(v > 0, self.e / np.where(v > 0, v, 1.0), np.inf), np.sqrt(self.e))
        return EV._rnd(v, e)

    def exp(self):
        with np.errstate(all='ignore'):
            v = np.exp(self.v)
            return EV(v, v * np.expm1(self.e) + 2 * EXP_ULPS * U * v * np.exp(self.e))

    def maxc(self, c):
        return EV(np.maximum(self.v, c), self.e)


def ev_matvec(m, vec, add=None, sub=None, m_err=0.0):
    """rows of a 3x3 `m` (..., 3, 3; entries carry a relative error m_err) times a list of three EV, in the kernel's
    order m0 v0 + m1 v1 + m2 v2 (+ add | - sub)."""
    out = []
    for r in range(3):
        acc = None
        for c in range(3):
            t = EV(m[..., r, c], m_err * np.abs(m[..., r, c])) * vec[c]
            acc = t if acc is None else acc + t
        if add is not None:
            acc = acc + EV(add[..., r])
        if sub is not None:
            acc = acc - EV(sub[..., r])
        out.append(acc)
    return out


# ======================================================================================================= InstanceNorm
IN_EPS = 1e-5
IN_REGIMES = ['nominal', 'offset', 'strong_offset', 'tiny_var', 'constant', 'wide']
# (H, W): HW / 4 and the launch route of scf_instance_norm (norm.hip: n4 <= 256 -> <1>, <= 1024 -> <4>, <= 4096 -> <16>,
# <= 8192 -> <8,1024>, <= 20480 -> <20,1024>, else / HW % 4 != 0 / misaligned -> generic).  Each is the smallest or the
# largest plane of its route, so a moved threshold puts one of them on another kernel (with another chain depth D).
IN_SHAPES = [
    (2, 2),        # n4 = 1: smallest vector plane, 255 idle lanes of <1>
    (32, 32),      # n4 = 256: last <1>
    (4, 257),      # n4 = 257: first <4>
    (64, 64),      # n4 = 1024: last <4>
    (4, 1025),     # n4 = 1025: first <16>
    (128, 128),    # n4 = 4096: last <16>
    (4, 4097),     # n4 = 4097: first <8,1024>
    (128, 256),    # n4 = 8192: last <8,1024>
    (4, 8193),     # n4 = 8193: first <20,1024>
    (256, 320),    # n4 = 20480: last <20,1024>, the largest register-resident plane
    (4, 20481),    # n4 = 20481: generic by size
    (5, 7),        # HW % 4 != 0: generic
    (1, 1),        # HW = 1: generic, variance exactly 0
]
IN_REGIME_SHAPES = [(64, 64), (256, 320), (5, 7), (4, 20481)]     # a register route, the largest one, generic (small, by size)


def in_depth(hw, aligned=True):
    """D: the longest chain of fp32 additions an element's value passes through on its way into a plane sum.
    register path: VEC4 accumulations of a 2-deep pair tree per thread, 6 shuffle levels, then the cross-wave sum (256
    threads: (r0 + r1) + (r2 + r3) added to 0 -> 3; 1024 threads: four such pairs accumulated -> 6);
    generic path: ceil(HW / 256) accumulations, 6 shuffle levels, 2 for the four waves."""
    n4 = hw // 4
    if hw % 4 == 0 and aligned and n4 <= 20480:
        vec4, nt = ((1, 256) if n4 <= 256 else (4, 256) if n4 <= 1024 else (16, 256) if n4 <= 4096 else
                    (8, 1024) if n4 <= 8192 else (20, 1024))
        return vec4 + 2 + 6 + (3 if nt == 256 else 6)
    return -(-hw // 256) + 8


def norm_core(x, depth, eps=IN_EPS):
    """x (..., M) float64 -> (y, bound) of (x - mean) / sqrt(var + eps) over the last axis for a two-pass fp32 evaluation
    whose sums have chain depth `depth`.
      mean:   |dm| <= (D + 1) U mean|x|                         (the sum, then the division)
      d_i = fl(x_i - m^): the shift by dm moves sum d^2 / M by exactly dm^2 (sum (x - m) = 0); squares, the sum and the
              division round (D + 4) U relative; + eps, sqrt and the reciprocal 3 U:
      rstd:   relative error rho <= ((D + 4) U + (dm rstd)^2) / 2 + 3 U     (|1 / sqrt(1 + t) - 1| <= t / 2 for t >= 0)
      y_i:    rstd |dm| + |y_i| (rho + 2 U)   (the subtraction and the product), second order kept by (1 + rho_lin).
    With em = rstd |dm| this is the issue's  rstd (D + 2) U max|x| + c U |y|  with mean|x| for max|x| (sharper, and equal
    on a constant plane) and c = (D + 4) / 2 + 5.  A constant plane has y = 0, so |y^| <= ~ rstd (D + 1) U |x|; a plane
    with mean 1e4 and std 1e-2 has em ~ 1: conditioning-limited, and the em^2 term keeps the bound honest there."""
    eps = float(np.float32(eps))
    with np.errstate(all='ignore'):                                 # a poisoned plane is NaN here too; its caller masks it
        mean = x.mean(-1, keepdims=True)
        var = ((x - mean) ** 2).mean(-1, keepdims=True)
        rstd = 1.0 / np.sqrt(var + eps)
        y = (x - mean) * rstd
    em = (depth + 1) * U * np.abs(x).mean(-1, keepdims=True) * rstd
    rho_lin = 0.5 * (depth + 4) * U + 3 * U + 2 * U
    rho = rho_lin + 0.5 * em * em                 # the em^2 part only ever LOWERS rstd^: it scales |y|, not the em term
    return y, (em + np.abs(y) * rho) * (1 + rho_lin)


def instance_norm_ref(x, res=None, relu=False, aligned=True):
    """x (N, C, H, W) fp32 -> (float64 reference, per-element bound)."""
    n, c, h, w = x.shape
    y, b = norm_core(f64(x).reshape(n, c, h * w), in_depth(h * w, aligned))
    if res is not None:
        r = f64(res).reshape(n, c, h * w)
        b = b + U * (np.abs(y) + np.abs(r) + b)                     # one addition
        y = y + r
    if relu:
        y = np.maximum(y, 0.0)                                      # exact and 1-Lipschitz
    return y.reshape(n, c, h, w), b.reshape(n, c, h, w)


def in_case(regime, shape, seed=0):
    """x (2, 3, H, W) and a residual.  `wide`: the largest magnitudes whose sum of squared deviations stays finite in
    fp32 -- ~1e18 on the smallest planes, sqrt(2e37 / HW) in general: a plane of 1e18 values with more than ~300
    elements overflows the variance sum in ANY fp32 evaluation (torch's own on a GPU included)."""
    g = torch.Generator().manual_seed(7000 + 100 * IN_REGIMES.index(regime) + seed)
    h, w = shape
    z = torch.randn((2, 3, h, w), generator=g)
    if regime == 'nominal':
        x = 0.5 + 2.0 * z
    elif regime == 'offset':
        x = 1e3 + z
    elif regime == 'strong_offset':
        x = 1e4 + 1e-2 * z
    elif regime == 'tiny_var':
        x = 1e-4 * z
    elif regime == 'constant':
        x = torch.tensor([3.7, -1e3, 0.0, 1e-3, 123456.0, -0.1]).view(2, 3, 1, 1).expand(2, 3, h, w).contiguous()
    else:
        x = z * min(1e18, math.sqrt(2e37 / (h * w)))
        assert float((x.double() ** 2).sum((2, 3)).max()) < 1e38
    res = torch.randn((2, 3, h, w), generator=g)
    return x.float().contiguous(), res


def instance_norm_fp32(x, res=None, relu=False, defect=None):
    """fp32 two-pass InstanceNorm in torch, with one planted defect."""
    n, c, h, w = x.shape
    hw = h * w
    v = x.reshape(n, c, hw)
    mean = v.sum(-1, keepdim=True) / hw
    if defect == 'single_pass':
        var = (v * v).sum(-1, keepdim=True) / hw - mean * mean
    elif defect == 'bessel':
        var = ((v - mean) ** 2).sum(-1, keepdim=True) / max(hw - 1, 1)
    else:
        var = ((v - mean) ** 2).sum(-1, keepdim=True) / hw
    eps = torch.tensor(IN_EPS, dtype=torch.float32)
    rstd = 1.0 / (torch.sqrt(var.clamp_min(0)) + eps) if defect == 'eps_outside' else 1.0 / torch.sqrt(var + eps)
    y = ((v - mean) * rstd).reshape(x.shape)
    if defect == 'relu_first':
        y = torch.relu(y)
        return y + res if res is not None else y
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


def torch_instance_norm(x, res=None, relu=False):
    if x.shape[2] * x.shape[3] == 1:        # F.instance_norm refuses a single spatial element: the fp32 restatement (0)
        return instance_norm_fp32(x, res, relu)
    y = F.instance_norm(x, eps=IN_EPS)
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


# ========================================================================================================== GroupNorm
GN_C, GN_G = 8, 2
GN_HW = [1,      # one element per channel, 4 per group
         16,     # 64 per group: one partial wave
         512,    # 2048 per group: the last register-resident size (KEEP * 256)
         513,    # 2052 per group: the first size that re-reads its input in every pass
         529]    # 23 x 23: odd, re-reading
GN_PARTS = [1, 3, 4, 5, 8]          # 4: the last part of the up-front loads; 5, 8: the loop for further parts
GN_REGIMES = ['nominal', 'offset', 'constant_group', 'cancelling']


def gn_depth(cnt):
    return (8 if cnt <= 2048 else -(-cnt // 256)) + 8


def gn_sum_parts(parts):
    """(S, N, C, HW) fp32 -> the element values the kernel normalises: the IN-ORDER fp32 sum part0 + part1 + ...  Each
    partial sum is rounded to fp32 (IEEE addition: the same bits as the kernel's), so cancelling parts have one right
    answer and a reference that summed in float64, or in another order, would be a different function."""
    v = parts[0].clone()
    for s in range(1, parts.shape[0]):
        v = (v + parts[s]).float()
    return v


def group_norm_relu_ref(parts, gamma, beta, groups):
    """parts (S, N, C, HW) fp32 -> (reference, bound) of relu(GroupNorm(sum of parts) * gamma[c] + beta[c])."""
    v = f64(gn_sum_parts(parts))
    n, c, hw = v.shape
    cpg = c // groups
    y, b = norm_core(v.reshape(n, groups, cpg * hw), gn_depth(cpg * hw))
    y, b = y.reshape(n, c, hw), b.reshape(n, c, hw)
    ga, be = f64(gamma).reshape(1, c, 1), f64(beta).reshape(1, c, 1)
    t = y * ga
    bt = np.abs(ga) * b
    bt = bt + U * (np.abs(t) + bt)                                  # the product with gamma
    bt = bt + U * (np.abs(t) + np.abs(be) + bt)                     # the addition of beta
    return np.maximum(t + be, 0.0), bt


def gn_case(regime, hw, parts, c=GN_C, groups=GN_G, n=2, seed=0):
    g = torch.Generator().manual_seed(9000 + 100 * GN_REGIMES.index(regime) + 10 * parts + seed + hw)
    p = torch.randn((parts, n, c, hw), generator=g)
    if regime == 'offset':
        p[0] += 300.0
    if regime == 'constant_group':                                  # group 0 of every sample: one value; group 1: nominal
        p[:, :, :c // groups] = 0.0
        p[0, :, :c // groups] = 2.5
    if regime == 'cancelling' and parts > 1:                        # part0 = -part1 + small
        p[0] = -p[1] * 1e3 + 1e-3 * p[0]
        p[1] = p[1] * 1e3
    gamma = 1.0 + 0.5 * torch.randn((c,), generator=g)
    beta = 0.3 * torch.randn((c,), generator=g)
    return p.float().contiguous(), gamma, beta


def group_norm_relu_fp32(parts, gamma, beta, groups, defect=None):
    v = gn_sum_parts(parts)
    n, c, hw = v.shape
    cpg = c // groups
    if defect == 'affine_by_group':
        y = F.group_norm(v, groups, eps=IN_EPS).reshape(n, groups, cpg * hw)
        y = y * gamma[:groups].view(1, groups, 1) + beta[:groups].view(1, groups, 1)
        return torch.relu(y).reshape(n, c, hw)
    return torch.relu(F.group_norm(v, groups, gamma, beta, eps=IN_EPS))


# ============================================================================================================= resize
# (planes, in, out): what each reaches in resize_bilinear_kernel (one thread = 4 output columns, block = 4 rows x 256
# columns, grid z = planes capped at ~4 blocks per CU)
RESIZE_SIZES = [
    (4, (1, 1), (1, 1)),           # scale 0 both ways
    (4, (1, 1), (3, 5)),           # one source pixel: every +1 tap clamped
    (4, (2, 3), (1, 1)),           # Hout = Wout = 1: scale defined as 0
    (4, (8, 8), (8, 8)),           # identity: every coordinate an integer
    (4, (5, 9), (9, 17)),          # (out - 1) a multiple of (in - 1): every second coordinate an integer
    (4, (17, 25), (3, 4)),         # down-sampling, Wout % 4 == 0 (VEC)
    (4, (4, 33), (6, 260)),        # second 256-column segment, Wout % 4 == 0
    (4, (9, 7), (30, 301)),        # ragged last quadruple (scalar stores), two segments
    (4, (3, 3), (5, 8)),           # the GPU file also runs it with `out` one float off alignment: scalar stores, Wout % 4 == 0
    (1030, (2, 2), (4, 4)),        # 103 x 10 planes > 4 x 256 CUs: the plane grid-stride loop
    (4, (4, 8), (10, 50)),         # fl(7 / 49) * 49 > 7: the last coordinate lands past in - 1, on the clamped +1 tap
    (4, (3, 8), (42, 24)),         # fl(scale) * index on the other side of an integer than the exact coordinate, both axes
]
RESIZE_C = 8    # a + b; 1 - lx, its product, the row sum; 1 - ly, its product, the column sum; mul


def resize_coords(n_in, n_out, mode):
    """source coordinate of every output index: 'exact' = index (in - 1) / (out - 1) in float64; 'fp32' = what ATen and
    the kernel define it as, fl(fl((in - 1) / (out - 1)) * index) in fp32 -- an input of the operation, not an error."""
    idx = np.arange(n_out)
    if n_out <= 1:
        return np.zeros(n_out)
    if mode == 'exact':
        return idx * (float(n_in - 1) / float(n_out - 1))
    s = np.float32(n_in - 1) / np.float32(n_out - 1)
    return (s * idx.astype(np.float32)).astype(np.float64)


def _taps(f, n_in):
    i0 = np.minimum(np.floor(f).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), f - i0


def _nbr_delta(v, axis):
    """per element: the largest |difference| over the three intervals next to it along `axis` ([i-1, i], [i, i+1],
    [i+1, i+2], clamped): the slope bound for a coordinate that may sit on either side of an integer."""
    d = np.abs(np.diff(v, axis=axis))
    pad = [(0, 0)] * v.ndim
    pad[axis] = (2, 2)
    d = np.pad(d, pad)                                              # d[j + 2] = |v[j + 1] - v[j]|
    n = v.shape[axis]
    sl = lambda o: tuple(slice(o, o + n) if a == axis else slice(None) for a in range(v.ndim))  # noqa: E731
    return np.maximum(np.maximum(d[sl(1)], d[sl(2)]), d[sl(3)]) if n > 1 else np.zeros_like(v)


def resize_ref(a, out_hw, mul=1.0, b=None, coords='exact'):
    """a (P, Hin, Win) fp32 -> (reference, bound) of mul * bilinear(a + b), align_corners=True.
    bound = |mul| U (C S + coord), S = sum w' |v| with every `1 - l` weight widened by its own rounding U.
    coords='exact': the kernel's coordinate fl(fl(scale) * index) is off by <= 2 U f (the scale, the product); the
      interpolant is continuous and piecewise linear, so the result moves by <= 2 U (fx Gx + fy Gy) with G the largest
      tap difference over the intervals next to the coordinate -- also where the rounded coordinate falls on the other
      side of an integer (identity sizes, (out - 1) a multiple of (in - 1)).
    coords='fp32': the coordinate is the operation's (torch rounds it the same way); fx - x0 is exact, no coord term.
      This is the sharp form: a fused scale * index - x0 moves the weights by half an ulp of the coordinate and fails it."""
    v = f64(a) + (f64(b) if b is not None else 0.0)
    p, hin, win = v.shape
    ho, wo = out_hw
    fy, fx = resize_coords(hin, ho, coords), resize_coords(win, wo, coords)
    y0, y1, ly = _taps(fy, hin)
    x0, x1, lx = _taps(fx, win)
    ly, lx = ly[None, :, None], lx[None, None, :]
    hy, hx = 1.0 - ly, 1.0 - lx
    g = lambda t, yy, xx: t[:, yy][:, :, xx]                        # noqa: E731
    ref = mul * (hy * (hx * g(v, y0, x0) + lx * g(v, y0, x1)) + ly * (hx * g(v, y1, x0) + lx * g(v, y1, x1)))
    av = np.abs(v)
    s = (hy + U) * ((hx + U) * g(av, y0, x0) + lx * g(av, y0, x1)) + ly * ((hx + U) * g(av, y1, x0) + lx * g(av, y1, x1))
    bound = RESIZE_C * s
    if coords == 'exact':
        gx, gy = _nbr_delta(v, 2), _nbr_delta(v, 1)
        gxm = np.maximum(np.maximum(g(gx, y0, x0), g(gx, y0, x1)), np.maximum(g(gx, y1, x0), g(gx, y1, x1)))
        gym = np.maximum(np.maximum(g(gy, y0, x0), g(gy, y0, x1)), np.maximum(g(gy, y1, x0), g(gy, y1, x1)))
        bound = bound + 2.0 * (fx[None, None, :] * gxm + fy[None, :, None] * gym)
    return ref, abs(mul) * U * bound


def resize_case(kind, planes, in_hw, seed=0):
    g = torch.Generator().manual_seed(11000 + seed + 7 * in_hw[0] + in_hw[1])
    if kind == 'checker':                                           # +-1e3 checkerboard: the worst tap differences
        yy, xx = torch.meshgrid(torch.arange(in_hw[0]), torch.arange(in_hw[1]), indexing='ij')
        a = (1e3 * (1 - 2 * ((yy + xx) % 2)).float())[None].repeat(planes, 1, 1)
        a = a * (1.0 + 0.01 * torch.rand((planes, 1, 1), generator=g))
    else:
        a = torch.randn((planes, *in_hw), generator=g)
    b = torch.randn((planes, *in_hw), generator=g)
    return a.contiguous(), b


def resize_fp32(a, out_hw, mul=1.0, b=None, defect=None):
    """the kernel's operation order in numpy fp32, with one planted defect."""
    f = np.float32
    v = a.numpy() + (b.numpy() if b is not None else f(0))
    p, hin, win = v.shape
    ho, wo = out_hw

    def axis(n_in, n_out):
        s = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
        idx = np.arange(n_out).astype(f)
        fc = (s * idx).astype(f)
        i0 = np.minimum(fc.astype(np.int64), n_in - 1)
        if defect == 'fused':                                       # one rounding: fl(scale * index - i0)
            lo = (np.float64(s) * idx.astype(np.float64) - i0).astype(f)
        else:
            lo = (fc - i0.astype(f)).astype(f)
        return i0, i0 + 1, lo

    y0, y1, ly = axis(hin, ho)
    x0, x1, lx = axis(win, wo)
    vp = np.zeros((p, hin + 1, win + 1), dtype=f)                   # the +1 taps past the edge
    vp[:, :hin, :win] = v
    if defect != 'unclamped':                                       # clamped: the edge pixel again; defect: read as zero
        vp[:, hin, :win], vp[:, :hin, win], vp[:, hin, win] = v[:, -1], v[:, :, -1], v[:, -1, -1]
    ly, lx = ly[None, :, None], lx[None, None, :]
    hy, hx = f(1) - ly, f(1) - lx
    g = lambda yy, xx: vp[:, yy][:, :, xx]                          # noqa: E731
    return f(mul) * (hy * (hx * g(y0, x0) + lx * g(y0, x1)) + ly * (hx * g(y1, x0) + lx * g(y1, x1)))


# ============================================================================================================ avgpool
POOL_SIZES = [(2, 2), (3, 2), (5, 7), (12, 20)]     # one window; odd height; both odd (last row / column dropped); even


def avgpool_ref(x):
    """x (P, H, W) -> (reference, 3 U sum|s| / 4): three additions, the scale by 0.25 is exact."""
    v = f64(x)
    h2, w2 = v.shape[1] // 2, v.shape[2] // 2
    q = [v[:, dy:2 * h2:2, dx:2 * w2:2] for dy in (0, 1) for dx in (0, 1)]
    return sum(q) / 4.0, 3 * U * sum(np.abs(t) for t in q) / 4.0


# ==================================================================================================== convex upsample
CONVEX_SIZES = [(1, 1, 1, 1),      # all eight neighbours are padding
                (2, 2, 3, 33),     # two 32-pixel segments, the second with one live lane; interior and every border
                (1, 8, 2, 5)]      # C = 8: exactly the 64 KiB of LDS the entry point allows
CONVEX_REGIMES = ['nominal', 'sharp', 'tied', 'equal_zero', 'equal_nonzero']
CONVEX_NONFINITE = ['nan', 'pinf', 'one_ninf', 'all_ninf']


def convex_case(regime, size, seed=0):
    n, c, h, w = size
    g = torch.Generator().manual_seed(13000 + seed + 31 * (CONVEX_REGIMES + CONVEX_NONFINITE).index(regime) + h * w)
    x = torch.randn((n, c, h, w), generator=g) * 3.0
    m = torch.randn((n, 9, 64, h, w), generator=g) * 4.0
    mask_mul = 0.25
    if regime == 'sharp':                                           # mask_mul * mask ~ +-200: one-hot weights
        m = m * 200.0
    if regime == 'tied':                                            # two exactly tied maxima
        m[:, 2] = 9.0
        m[:, 6] = 9.0
    if regime == 'equal_zero':
        m[:] = 0.0
    if regime == 'equal_nonzero':
        m[:] = -37.3
        mask_mul = 0.3                                              # not a power of two: the product rounds
    k = torch.randint(0, 9, (n, 64, h, w), generator=g)
    sel = F.one_hot(k, 9).permute(0, 4, 1, 2, 3).bool()             # one logit per sub-pixel
    if regime == 'nan':
        m[sel] = float('nan')
    if regime == 'pinf':
        m[sel] = float('inf')
    if regime == 'one_ninf':
        m[sel] = float('-inf')
    if regime == 'all_ninf':
        m[:, :, ::2] = float('-inf')                                # every second sub-pixel: all nine -inf
    return x.contiguous(), m.reshape(n, 576, h, w).contiguous(), 1.5, mask_mul


def convex_ref(x, mask, x_mul, mask_mul, order='ky_kx'):
    """(reference, bound).  a_k = mask_mul mask_k - max (softmax is invariant to the shift, so only the product's
    rounding -- none for a power-of-two mask_mul -- and the subtraction's enter the exponent: e_k = U (|l_k| + |a_k|));
    a weight's numerator is off by r_k = expm1(e_k) + expf's error, the denominator by the weighted mean of the r_j plus
    its 8 additions, then the reciprocal and w inv (2), x_mul x and the product (2), 9 accumulations:
        bound = sum_k w_k |x_mul x_k| (r_k + sum_j w_j r_j + 21 U)  (+ weights lost below 2**-126)."""
    n, c, h, w = x.shape
    xm, mm = float(np.float32(x_mul)), float(np.float32(mask_mul))
    l = mm * f64(mask).reshape(n, 9, 8, 8, h, w)
    with np.errstate(all='ignore'):
        wt = torch.softmax(torch.from_numpy(l), dim=1).numpy()
        a = l - l.max(1, keepdims=True)
        pow2 = math.frexp(mm)[0] == 0.5
        e = U * ((0.0 if pow2 else 1.0) * np.abs(l) + np.abs(a))
        r = np.where(np.isneginf(a), 0.0, np.expm1(e) + 2 * EXP_ULPS * U)
        rbar = (wt * r).sum(1, keepdims=True)
    xp = np.pad(xm * f64(x), ((0, 0), (0, 0), (1, 1), (1, 1)))
    ref = np.zeros((n, c, 8, 8, h, w))
    bound = np.zeros_like(ref)
    for k in range(9):
        ky, kx = (k // 3, k % 3) if order == 'ky_kx' else (k % 3, k // 3)
        tap = xp[:, :, ky:ky + h, kx:kx + w][:, :, None, None]
        wk = wt[:, k][:, None]
        with np.errstate(all='ignore'):
            ref += wk * tap
            bound += wk * np.abs(tap) * (r[:, k][:, None] + rbar[:, 0][:, None] + 21 * U) + 2.0 ** -120 * np.abs(tap)
    shuffle = lambda t: t.transpose(0, 1, 4, 2, 5, 3).reshape(n, c, 8 * h, 8 * w)   # noqa: E731
    return shuffle(ref), shuffle(bound * (1 + 1e-6))


def convex_fp32(x, mask, x_mul, mask_mul, defect=None):
    n, c, h, w = x.shape
    l = (mask_mul * mask).view(n, 9, 8, 8, h, w)
    if defect == 'no_max':
        ex = torch.exp(l)
        wt = ex / ex.sum(1, keepdim=True)
    else:
        wt = torch.softmax(l, dim=1)
    xp = F.pad(x_mul * x, (1, 1, 1, 1))
    out = torch.zeros((n, c, 8, 8, h, w))
    for k in range(9):
        ky, kx = (k % 3, k // 3) if defect == 'transposed' else (k // 3, k % 3)
        out += wt[:, k][:, None] * xp[:, :, ky:ky + h, kx:kx + w][:, :, None, None]
    return out.permute(0, 1, 4, 2, 5, 3).reshape(n, c, 8 * h, 8 * w)


def same_nan_pattern(got, ref):
    return bool(np.array_equal(np.isnan(f64(got)), np.isnan(f64(ref))))


# ======================================================================================================== pose update
POSE_N = [1, 3, 70]                 # 70: a second 64-thread block, 6 live threads in it
POSE_REGIMES = ['nominal', 'tiny_a', 'huge_a', 'zero_a', 'parallel', 'near_parallel', 'dz_neg', 'dz_zero', 'dz_pos',
                'steep']
NUM_CLASS = 21


def rand_rot(n, g, angle=None):
    """orthonormal fp32-rounded rotations from random axis-angle (Rodrigues, float64)."""
    ax = torch.randn((n, 3), generator=g, dtype=torch.float64)
    ax = ax / ax.norm(dim=1, keepdim=True)
    th = (torch.rand((n, 1, 1), generator=g, dtype=torch.float64) * 2 - 1) * (math.pi if angle is None else angle)
    kx = torch.zeros((n, 3, 3), dtype=torch.float64)
    kx[:, 0, 1], kx[:, 0, 2], kx[:, 1, 0] = -ax[:, 2], ax[:, 1], ax[:, 2]
    kx[:, 1, 2], kx[:, 2, 0], kx[:, 2, 1] = -ax[:, 0], -ax[:, 1], ax[:, 0]
    r = torch.eye(3, dtype=torch.float64) + torch.sin(th) * kx + (1 - torch.cos(th)) * (kx @ kx)
    return r.float()


def pose_case(regime, n, seed=0):
    g = torch.Generator().manual_seed(15000 + 100 * POSE_REGIMES.index(regime) + n + seed)
    rot_all = torch.randn((n, NUM_CLASS, 6), generator=g)
    trans_all = torch.randn((n, NUM_CLASS, 3), generator=g) * 0.3
    label = torch.randint(0, NUM_CLASS, (n,), generator=g)
    label[0] = 20 if n == 1 else 0
    label[-1] = 20
    rot = rand_rot(n, g)
    trans = torch.randn((n, 3), generator=g) * 0.2
    trans[:, 2] = 0.5 + torch.rand((n,), generator=g)
    a, b = rot_all[..., 0:3], rot_all[..., 3:6]
    if regime == 'tiny_a':
        a *= 1e-6
    if regime == 'huge_a':
        a *= 1e6
    if regime == 'zero_a':
        a[:] = 0.0
    if regime == 'parallel':
        b[:] = 2.0 * a
    if regime == 'near_parallel':                                   # sin(a, b) ~ 1e-3
        b[:] = 1.5 * a + 1e-3 * a.norm(dim=-1, keepdim=True) * torch.randn(a.shape, generator=g)
    if regime in ('dz_neg', 'dz_zero', 'dz_pos'):
        trans_all[..., 2] = {'dz_neg': -20.0, 'dz_zero': 0.0, 'dz_pos': 20.0}[regime]
    if regime == 'steep':                                           # |tx / tz| ~ 10
        trans[:, 0] = 10.0 * trans[:, 2] * (1 - 2 * (torch.arange(n) % 2)).float()
    return rot_all.contiguous(), trans_all.contiguous(), label, rot.contiguous(), trans.contiguous()


def pose_select(rot_all, trans_all, label, mode):
    n = rot_all.shape[0]
    cls = label if mode & LABEL_PER_SAMPLE else label[0].expand(n)
    idx = torch.arange(n)
    return rot_all[idx, cls], trans_all[idx, cls]


def pose_update_ref(rot_all, trans_all, label, rot, trans, mode):
    """-> d_rot, d_trans (bit-exact selects), (R', bound), (t', bound): pose_update_one (pose.hip) replayed through EV."""
    d_rot, d_trans = pose_select(rot_all, trans_all, label, mode)
    o6, dt, rs, ts = f64(d_rot), f64(d_trans), f64(rot), f64(trans)
    a = [EV(o6[:, i]) for i in range(3)]
    b = [EV(o6[:, 3 + i]) for i in range(3)]
    nx = ((a[0] * a[0] + a[1] * a[1] + a[2] * a[2]).sqrt()).maxc(1e-12)
    x = [a[i] / nx for i in range(3)]
    z = [x[1] * b[2] - x[2] * b[1], x[2] * b[0] - x[0] * b[2], x[0] * b[1] - x[1] * b[0]]
    nz = ((z[0] * z[0] + z[1] * z[1] + z[2] * z[2]).sqrt()).maxc(1e-12)
    z = [z[i] / nz for i in range(3)]
    y = [z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]]
    rd = [[x[r], y[r], z[r]] for r in range(3)]                     # columns [x y z]
    rv, re = np.zeros((len(o6), 3, 3)), np.zeros((len(o6), 3, 3))
    for r in range(3):
        for c in range(3):
            acc = rd[r][0] * EV(rs[:, 0, c]) + rd[r][1] * EV(rs[:, 1, c]) + rd[r][2] * EV(rs[:, 2, c])
            rv[:, r, c], re[:, r, c] = acc.v, acc.e
    tz = EV(ts[:, 2])
    vz = tz * (EV(dt[:, 2]) + 1.0) if mode & DEPTH_LINEAR else tz / EV(dt[:, 2]).exp()
    vx = vz * (EV(dt[:, 0]) / 10.0 + EV(ts[:, 0]) / tz)
    vy = vz * (EV(dt[:, 1]) / 10.0 + EV(ts[:, 1]) / tz)
    tv = np.stack([vx.v, vy.v, vz.v], -1)
    te = np.stack([vx.e, vy.e, vz.e], -1)
    with np.errstate(all='ignore'):                                 # a || b: z = 0 / 0 in the reference, any R' in the kernel
        re = np.where(np.isnan(rv) | np.isnan(re), np.inf, re)
        rv = np.nan_to_num(rv, nan=0.0)
    return d_rot, d_trans, (rv, re), (tv, te)


def pose_update_fp32(rot_all, trans_all, label, rot, trans, mode, defect=None):
    """the oracle's fp32 pose update on the selected rows, with one planted defect."""
    if defect == 'label0':
        mode = mode & ~LABEL_PER_SAMPLE
    d_rot, d_trans = pose_select(rot_all, trans_all, label, mode)
    if defect == 'xzy':
        a, b = d_rot[:, 0:3], d_rot[:, 3:6]
        x = F.normalize(a, dim=1)
        z = F.normalize(torch.cross(x, b, dim=1), dim=1)
        rd = torch.stack([x, z, torch.cross(z, x, dim=1)], dim=2)
        r_new = torch.bmm(rd, rot)
        _, t_new = oracle.pose_from_delta_pose(d_rot, d_trans, rot, trans,
                                               depth_transform='linear' if mode & DEPTH_LINEAR else 'exp')
    else:
        r_new, t_new = oracle.pose_from_delta_pose(d_rot, d_trans, rot, trans,
                                                   depth_transform='linear' if mode & DEPTH_LINEAR else 'exp')
    return d_rot, d_trans, r_new, t_new


# ==================================================================================== re-projection and un-projection
GEOM_SIZES = [(1, 1, 1), (2, 5, 7), (3, 12, 20),
              (1, 129, 130)]        # 16770 pixels > 64 blocks x 256 threads: the grid-stride loop runs a second time
GEOM_POSES = ['identity', 'large_rotation', 'through_camera']
QZ_RULE = 64.0                      # pixels with |qz| < 64 U S_qz have no meaningful bound (issue, section 1)
LEFT_OUT_CAP = 0.01


def geom_case(pose, size, skew=True, seed=0):
    """depth map with background zeros, negative depths, a NaN and depths 0.05 .. 50; intrinsics with / without skew
    and an off-centre principal point; R0 / t0 and the new pose."""
    n, h, w = size
    g = torch.Generator().manual_seed(17000 + 100 * GEOM_POSES.index(pose) + h * w + seed + (1 if skew else 0))
    depth = torch.exp(torch.rand((n, h, w), generator=g) * math.log(1000.0)) * 0.05
    kind = torch.rand((n, h, w), generator=g)
    depth[kind < 0.25] = 0.0
    depth[(kind >= 0.25) & (kind < 0.32)] *= -1.0
    if h * w > 4:
        depth[0, h // 2, w // 3] = float('nan')
    k = torch.zeros((n, 3, 3))
    k[:, 0, 0] = 1.1 * max(h, w) * (1 + 0.1 * torch.rand((n,), generator=g))
    k[:, 1, 1] = 1.3 * max(h, w) * (1 + 0.1 * torch.rand((n,), generator=g))
    k[:, 0, 1] = 0.7 if skew else 0.0
    k[:, 0, 2], k[:, 1, 2], k[:, 2, 2] = 0.37 * w + 0.5, 0.61 * h - 0.25, 1.0
    rot0 = rand_rot(n, g)
    trans0 = torch.randn((n, 3), generator=g) * 0.1
    trans0[:, 2] = 1.0 + torch.rand((n,), generator=g)
    if pose == 'identity':                                          # the flow is a pure cancellation
        rot, trans = rot0.clone(), trans0.clone()
    elif pose == 'large_rotation':
        rot = torch.bmm(rand_rot(n, g, angle=2.5), rot0)
        trans = trans0 + torch.randn((n, 3), generator=g) * 0.05
    else:
        # the object is pulled through the camera plane: p_z = d - 5, and one run of pixels of sample 0 gets
        # d = 5 (1 + j 4e-6), i.e. qz = 0, 2e-5, 4e-5, ...: the first few are the pixels the |qz| rule is for
        rot = rot0.clone()
        trans = trans0.clone()
        trans[:, 2] -= 5.0
        if w >= 20:
            depth[0, 1, :8] = 5.0 * (1.0 + 4e-6 * torch.arange(8))
    return depth.contiguous(), k.contiguous(), rot0.contiguous(), trans0.contiguous(), rot.contiguous(), trans.contiguous()


def _inv64(m):
    return np.linalg.inv(f64(m))


def _unproject_ev(depth, k, rot0, trans0):
    n, h, w = depth.shape
    d = f64(depth)
    fg = d > 0                                                      # NaN > 0 is false: background
    d = np.where(fg, d, 1.0)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    kinv, r0inv = _inv64(k)[:, None, None], _inv64(rot0)[:, None, None]
    hom = [EV(xs[None]) * EV(d), EV(ys[None]) * EV(d), EV(d)]
    # the fp64 adjugate rounded to fp32: each entry of the inverse carries U relative
    cam = ev_matvec(kinv, hom, sub=f64(trans0)[:, None, None], m_err=U)
    return fg, xs, ys, ev_matvec(r0inv, cam, m_err=U)


def unproject_ref(depth, k, rot0, trans0):
    """-> (pts (N, 3, H, W), bound); background (depth <= 0 or NaN) is exactly 0."""
    fg, _, _, obj = _unproject_ev(depth, k, rot0, trans0)
    ref = np.stack([np.where(fg, o.v, 0.0) for o in obj], 1)
    return ref, np.stack([np.where(fg, o.e, 0.0) for o in obj], 1)


def reproject_ref(depth, k, rot0, trans0, rot, trans, invalid):
    """-> (flow (N, 2, H, W), bound, left_out (N, H, W)): u = qx / qz - x with the shadows carried through Kinv, R0inv,
    R, K; with e_q the running bound of q, |q^x / q^z - qx / qz| <= (e_qx + |qx / qz| e_qz) / (|qz| - e_qz), i.e. the
    issue's c U (S_qx / |qz| + |qx| S_qz / qz^2 + |x|).  left_out: foreground pixels with |qz| < 64 U S_qz."""
    fg, xs, ys, obj = _unproject_ev(depth, k, rot0, trans0)
    cam = ev_matvec(f64(rot)[:, None, None], obj, add=f64(trans)[:, None, None])
    q = ev_matvec(f64(k)[:, None, None], cam)
    # S_qz: the magnitude shadow of qz -- the same chain on absolute values
    ab = lambda m: np.abs(f64(m))[:, None, None]                    # noqa: E731
    mv = lambda m, v: [m[..., r, 0] * v[0] + m[..., r, 1] * v[1] + m[..., r, 2] * v[2] for r in range(3)]   # noqa: E731
    dd = np.where(fg, f64(depth), 1.0)
    sh = mv(np.abs(_inv64(k))[:, None, None], [xs[None] * dd, ys[None] * dd, dd])
    sh = mv(np.abs(_inv64(rot0))[:, None, None], [sh[i] + ab(trans0)[..., i] for i in range(3)])
    sh = mv(ab(rot), sh)
    s_qz = mv(ab(k), [sh[i] + ab(trans)[..., i] for i in range(3)])[2]
    with np.errstate(all='ignore'):
        left = fg & (np.abs(q[2].v) < QZ_RULE * U * s_qz)
    fu, fv = q[0] / q[2] - EV(xs[None]), q[1] / q[2] - EV(ys[None])
    ref = np.stack([np.where(fg, fu.v, invalid), np.where(fg, fv.v, invalid)], 1)
    bound = np.stack([np.where(fg, fu.e, 0.0), np.where(fg, fv.e, 0.0)], 1)
    return ref, bound, left


def geom_fp32(depth, k, rot0, trans0, rot, trans, invalid, defect=None):
    """the kernels' operation order in numpy fp32 (inverses: float64, rounded, like inv3x3) -> (flow, pts).  The
    oracle's own fp32 path inverts K and R0 by fp32 LU and may exceed the bound; its ratio is printed, this one asserted."""
    f = np.float32
    n, h, w = depth.shape
    d = depth.numpy()
    with np.errstate(all='ignore'):
        fg = d > 0
    dd = np.where(fg, d, f(1))
    ys, xs = np.meshgrid(np.arange(h, dtype=f), np.arange(w, dtype=f), indexing='ij')
    kinv = _inv64(k).astype(f)[:, None, None]
    r0inv = (f64(rot0) if defect == 'r0_not_inverted' else _inv64(rot0)).astype(f)[:, None, None]
    kk, rr = k.numpy()[:, None, None], rot.numpy()[:, None, None]
    t0, tt = trans0.numpy()[:, None, None], trans.numpy()[:, None, None]
    mv = lambda m, v: [m[..., r, 0] * v[0] + m[..., r, 1] * v[1] + m[..., r, 2] * v[2] for r in range(3)]   # noqa: E731
    cam = mv(kinv, [xs[None] * dd, ys[None] * dd, dd])
    cam = [cam[i] - t0[..., i] for i in range(3)]
    obj = mv(r0inv, cam)
    p = mv(rr, obj)
    p = [p[i] + tt[..., i] for i in range(3)]
    q = mv(kk, p)
    with np.errstate(all='ignore'):
        flow = np.stack([np.where(fg, q[0] / q[2] - xs[None], f(invalid)), np.where(fg, q[1] / q[2] - ys[None], f(invalid))], 1)
    return flow, np.stack([np.where(fg, o, f(0)) for o in obj], 1)


def oracle_reproject(depth, k, rot0, trans0, rot, trans, invalid):
    """oracle.flow_from_delta_pose_and_depth; a NaN depth is background there too (NaN > 0 is false)."""
    return oracle.flow_from_delta_pose_and_depth(rot0, trans0, rot, trans, depth, k, invalid_num=invalid)


def check_left_out(left, compared):
    """the cap of section 4: at most 1 % of the compared elements of a case may be left out."""
    share = float(left.sum()) / max(int(compared.sum()), 1)
    assert share <= LEFT_OUT_CAP, f'{share:.3%} of the compared elements left out (cap 1 %)'
    return share


# ================================================================================================ filter_flow_by_mask
FILTER_SIZES = [(1, 1, 1), (2, 5, 7), (2, 32, 40)]
FILTER_INVALID = 400.0


def filter_case(mask_kind, size, seed=0):
    """flow (N, 2, H, W) with, in its first pixels in row-major order, end points exactly on the border and one pixel
    outside each side, invalid_num in one / both components, +-1e9, and NaN / +inf / -inf / 3e38 in one component;
    elsewhere small random flow.  mask (N, H, W): binary, or smooth and crossing 0.9."""
    n, h, w = size
    g = torch.Generator().manual_seed(19000 + h * w + seed + (0 if mask_kind == 'binary' else 50))
    flow = torch.randn((n, 2, h, w), generator=g) * 1.5
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing='ij')
    if mask_kind == 'binary':
        mask = (torch.rand((n, h, w), generator=g) < 0.8).float()
    else:
        mask = (0.9 + 0.12 * torch.sin(0.9 * xx + 0.3) * torch.cos(0.7 * yy + 0.1))[None].repeat(n, 1, 1).clamp(0, 1)
        mask = (mask + 0.003 * torch.rand((n, h, w), generator=g)).clamp(0, 1)
    inf, nan = float('inf'), float('nan')
    special = [(-1.0, 0.0), (0.0, -1.0), (1.0, 0.0), (0.0, 1.0),                    # filled in per pixel below: border +-1
               (FILTER_INVALID, 0.25), (0.25, FILTER_INVALID), (FILTER_INVALID, FILTER_INVALID), (500.0, 401.0),
               (1e9, 0.0), (0.0, -1e9), (-1e9, 1e9),
               (nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, inf), (-inf, 0.0), (0.0, -inf), (3e38, 0.0), (0.0, -3e38),
               (inf, 500.0), (nan, nan), (inf, inf)]
    fx, fy = flow[:, 0].reshape(n, -1), flow[:, 1].reshape(n, -1)
    px, py = xx.reshape(-1), yy.reshape(-1)
    for i, (sx, sy) in enumerate(special):
        for rep in range(2):                                        # twice: once from the first pixels, once from the last
            q = i if rep == 0 else h * w - 1 - i
            if not 0 <= q < h * w:
                continue
            if i < 4:       # end point on the border (first copy) / one pixel outside that side (second copy)
                out = float(rep)
                tx = {-1.0: -out, 1.0: (w - 1) + out}.get(sx, px[q].item())
                ty = {-1.0: -out, 1.0: (h - 1) + out}.get(sy, py[q].item())
                fx[:, q], fy[:, q] = tx - px[q], ty - py[q]
            else:
                fx[:, q], fy[:, q] = sx, sy
    return flow.contiguous(), mask.contiguous()


def filter_ref(flow, mask, invalid, align_corners):
    """-> (expected flow, compared (N, H, W)).  The decision  invalid <- sampled < 0.9 || both >= invalid_num  is compared
    where it is certain:
      * a non-finite sample coordinate in fp32 (NaN / inf flow, or a finite one that overflows (x + f) * 2): grid_sample
        returns NaN and `NaN < 0.9` is false -- the vector is KEPT unless both components are >= invalid_num;
      * the end point is outside the image by more than its coordinate error: the sample is exactly 0;
      * |sampled - 0.9| > margin, margin = (e_x + e_y) max|mask| + 10 U max|mask|: e = the running error of the fp32
        coordinate (a few U max(W, H)); the bilinear sample of a mask in [0, max] with zero padding is continuous with
        slope <= max per pixel, and its four products and three sums round <= 10 U.
    Compared outputs must be bit-equal to the input flow or to invalid_num."""
    n, _, h, w = flow.shape
    fl, m = f64(flow), f64(mask)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')

    def coord(pix, f, size):
        gn = (EV(pix[None]) + EV(f)) * 2.0 / float(max(size - 1, 1)) - 1.0
        return (gn + 1.0) / 2.0 * float(size - 1) if align_corners else ((gn + 1.0) * float(size) - 1.0) / 2.0

    def coord32(pix, f, size):                                      # coords_grid + ATen's unnormalize, in fp32
        t = np.float32
        with np.errstate(all='ignore'):
            gn = (pix[None].astype(t) + f) * t(2) / t(max(size - 1, 1)) - t(1)
            return (gn + t(1)) / t(2) * t(size - 1) if align_corners else ((gn + t(1)) * t(size) - t(1)) / t(2)

    with np.errstate(all='ignore'):
        ix, iy = coord(xs, fl[:, 0], w), coord(ys, fl[:, 1], h)
        nonfinite = ~(np.isfinite(coord32(xs, flow[:, 0].numpy(), w)) & np.isfinite(coord32(ys, flow[:, 1].numpy(), h)))
        both = (fl[:, 0] >= invalid) & (fl[:, 1] >= invalid)
        outside = ((ix.v + ix.e < -1) | (ix.v - ix.e > w) | (iy.v + iy.e < -1) | (iy.v - iy.e > h)) & ~nonfinite
        cx, cy = np.clip(np.nan_to_num(ix.v), -2, w + 1), np.clip(np.nan_to_num(iy.v), -2, h + 1)
    x0, y0 = np.floor(cx), np.floor(cy)
    mp = np.pad(m, ((0, 0), (3, 3), (3, 3)))
    bi = np.arange(n)[:, None, None]
    at = lambda yy, xx: mp[bi, yy.astype(np.int64) + 3, xx.astype(np.int64) + 3]    # noqa: E731
    lx, ly = cx - x0, cy - y0
    smp = (1 - ly) * ((1 - lx) * at(y0, x0) + lx * at(y0, x0 + 1)) + ly * ((1 - lx) * at(y0 + 1, x0) + lx * at(y0 + 1, x0 + 1))
    smp = np.where(outside, 0.0, smp)
    mmax = float(np.abs(m).max())
    with np.errstate(all='ignore'):
        margin = np.where(nonfinite | outside, 0.0, (ix.e + iy.e) * mmax + 10 * U * mmax)
        certain = nonfinite | outside | both | (np.abs(smp - 0.9) > margin)
        inval = both | (~nonfinite & (smp < 0.9))
    expect = flow.clone()
    expect[torch.from_numpy(inval)[:, None].expand_as(flow)] = invalid
    return expect, certain


def filter_fp32(flow, mask, invalid, align_corners, defect=None):
    """oracle.filter_flow_by_mask; defect: the align_corners=False branch de-normalised with W - 1 (= sampled with
    align_corners=True)."""
    if defect == 'denorm_wm1' and not align_corners:
        return oracle.filter_flow_by_mask(flow, mask, invalid, align_corners=True)
    return oracle.filter_flow_by_mask(flow, mask, invalid, align_corners=align_corners)


def same_bits(a, b):
    a = a.detach().cpu().contiguous().view(torch.int32)
    b = b.detach().cpu().contiguous().view(torch.int32)
    return bool(torch.equal(a, b))


def filter_agrees(got, expect, certain):
    sel = torch.from_numpy(certain)[:, None].expand_as(expect)
    return same_bits(got.cpu()[sel], expect[sel])


# ===================================================================================================== the self-checks
def _in_inputs():
    for shape in IN_SHAPES:
        yield 'nominal', shape
    for shape in IN_REGIME_SHAPES:
        for regime in IN_REGIMES[1:]:
            yield regime, shape


def test_ev_counts_roundings():
    """the running bound is what counting gives: a 3-term dot product of exact inputs = 3 products, 2 sums."""
    a = [EV(np.array(1.0)), EV(np.array(2.0)), EV(np.array(3.0))]
    d = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
    assert d.v == 14.0 and 3 * U * 14 * 0.3 < d.e < 3 * U * 14 * 1.01
    assert (EV(np.array(4.0), 0.0).sqrt()).e == pytest.approx(2 * U)
    assert np.isinf((EV(np.array(1.0)) / EV(np.array(1e-9), 1e-8)).e)


def test_instance_norm_reference_inside():
    """torch's fp32 F.instance_norm (+res, +ReLU) inside the bound on every shape and regime of the GPU file."""
    worst = {}
    for regime, shape in _in_inputs():
        x, res = in_case(regime, shape)
        for r in (None, res):
            for relu in (False, True):
                ref, bound = instance_norm_ref(x, r, relu)
                worst[regime] = max(worst.get(regime, 0.0), worst_ratio(torch_instance_norm(x, r, relu), ref, bound))
    for regime, v in worst.items():
        measured(f'instance_norm torch fp32 / bound, {regime}', v)
        assert v <= 1.0, regime


def test_instance_norm_bound_properties():
    """what must FOLLOW from the bound: a constant plane may come out as rstd D U |x| (not 0), and mean 1e4 / std 1e-2 is
    conditioning-limited (~3e-2 is legitimate) -- while the nominal regime stays at a few 1e-6."""
    x, _ = in_case('constant', (64, 64))
    ref, bound = instance_norm_ref(x)
    d = in_depth(64 * 64)
    rstd = 1.0 / math.sqrt(float(np.float32(IN_EPS)))
    assert np.all(ref == 0)
    assert np.all(bound <= rstd * (d + 2) * U * np.abs(f64(x)) * 1.001)
    x, _ = in_case('strong_offset', (64, 64))
    _, bound = instance_norm_ref(x)
    assert 3e-2 < bound.max() < 10.0
    x, _ = in_case('nominal', (64, 64))
    _, bound = instance_norm_ref(x)
    assert bound.max() < 1e-5


@pytest.mark.parametrize('defect, regime', [('single_pass', 'offset'), ('bessel', 'nominal'), ('eps_outside', 'nominal'),
                                            ('eps_outside', 'tiny_var'), ('relu_first', 'nominal')])
def test_instance_norm_planted_defects_outside(defect, regime):
    worst = 0.0
    for shape in [s for r, s in _in_inputs() if r == regime]:
        if shape == (1, 1) or in_depth(shape[0] * shape[1]) > 40:
            continue        # HW = 1: every variant gives 0; (4, 20481): the generic kernel's chain of 329 additions makes a
                            # bound (1e-5 relative) that a defect of a few 1e-6 stays inside -- honest, and said here
        x, res = in_case(regime, shape)
        ref, bound = instance_norm_ref(x, res, True)
        good = worst_ratio(instance_norm_fp32(x, res, True), ref, bound)
        bad = worst_ratio(instance_norm_fp32(x, res, True, defect=defect), ref, bound)
        assert good <= 1.0 < bad, (defect, shape, good, bad)
        worst = max(worst, bad)
    measured(f'instance_norm defect {defect} / bound, {regime}', worst)


def test_instance_norm_nonfinite_reference():
    """one NaN or one +inf poisons exactly its plane in torch (every element NaN), with and without the ReLU; the HIP
    kernel's ReLU is v_max, which returns 0 for NaN (its comment) -- the GPU file pins that difference."""
    x, _ = in_case('nominal', (5, 7))
    x[0, 1, 2, 3] = float('nan')
    x[1, 0, 0, 0] = float('inf')
    for relu in (False, True):
        y = torch_instance_norm(x, None, relu)
        bad = torch.isnan(y).flatten(2).all(2)
        assert bad.tolist() == [[False, True, False], [True, False, False]]
        assert not torch.isnan(y).flatten(2).any(2)[~bad].any()


def _gn_inputs():
    for hw in GN_HW:
        for parts in GN_PARTS:
            yield 'nominal', hw, parts
    for regime in GN_REGIMES[1:]:
        for hw, parts in ((16, 1), (512, 3), (513, 5)):
            yield regime, hw, parts


def test_group_norm_reference_inside_and_defect_outside():
    worst, worst_bad = {}, float('inf')
    for regime, hw, parts in _gn_inputs():
        p, gamma, beta = gn_case(regime, hw, parts)
        ref, bound = group_norm_relu_ref(p, gamma, beta, GN_G)
        worst[regime] = max(worst.get(regime, 0.0), worst_ratio(group_norm_relu_fp32(p, gamma, beta, GN_G), ref, bound))
        worst_bad = min(worst_bad, worst_ratio(group_norm_relu_fp32(p, gamma, beta, GN_G, 'affine_by_group'), ref, bound))
    for c, g, hw in ((128, 32, 16), (128, 32, 256)):                # the pose head's own group shape
        p, gamma, beta = gn_case('nominal', hw, 1, c=c, groups=g)
        ref, bound = group_norm_relu_ref(p, gamma, beta, g)
        worst['pose_head'] = max(worst.get('pose_head', 0.0), worst_ratio(group_norm_relu_fp32(p, gamma, beta, g), ref, bound))
    for regime, v in worst.items():
        measured(f'group_norm_relu torch fp32 / bound, {regime}', v)
        assert v <= 1.0, regime
    measured('group_norm_relu defect affine_by_group / bound (least)', worst_bad)
    assert worst_bad > 1.0


def test_group_norm_cancelling_parts_need_the_in_order_sum():
    """with part0 = -part1 + small, (part0 + part1) is exact and the third part is added to a small number; a kernel
    that added the parts in another order ((part2 + part1) + part0) rounds at the magnitude of the large parts and is
    far outside the bound: the in-order sum is the only right answer."""
    p, gamma, beta = gn_case('cancelling', 512, 3)
    ref, bound = group_norm_relu_ref(p, gamma, beta, GN_G)
    other = group_norm_relu_fp32(p.flip(0), gamma, beta, GN_G)
    assert worst_ratio(group_norm_relu_fp32(p, gamma, beta, GN_G), ref, bound) <= 1.0 < worst_ratio(other, ref, bound)


def _resize_inputs():
    for planes, in_hw, out_hw in RESIZE_SIZES:
        for kind in ('nominal', 'checker'):
            yield kind, planes, in_hw, out_hw


def test_resize_reference_inside():
    """F.interpolate(a + b) * mul and the fp32 restatement inside BOTH bounds (exact and fp32 coordinates)."""
    worst = {}
    for kind, planes, in_hw, out_hw in _resize_inputs():
        a, b = resize_case(kind, planes, in_hw)
        for mul in (1.0, 0.125):
            for bb in (None, b):
                t = mul * F.interpolate((a if bb is None else a + bb)[None], size=out_hw, mode='bilinear', align_corners=True)[0]
                for coords in ('exact', 'fp32'):
                    ref, bound = resize_ref(a, out_hw, mul, bb, coords)
                    key = f'{kind}, {coords} coordinates'
                    worst[key] = max(worst.get(key, 0.0), worst_ratio(t, ref, bound),
                                     worst_ratio(resize_fp32(a, out_hw, mul, bb), ref, bound))
    for key, v in worst.items():
        measured(f'resize_bilinear torch fp32 / bound, {key}', v)
        assert v <= 1.0, key


def test_resize_sizes_put_coordinates_on_the_other_side_of_integers():
    """the size list holds coordinates whose fp32 value and exact value have different integer parts (the continuity
    argument is exercised), and a last coordinate past in - 1 (the +1 tap's clamp is exercised)."""
    crossed = past = 0
    for _, in_hw, out_hw in RESIZE_SIZES:
        for n_in, n_out in zip(in_hw, out_hw):
            e, f = resize_coords(n_in, n_out, 'exact'), resize_coords(n_in, n_out, 'fp32')
            crossed += int((np.floor(e + 1e-9) != np.floor(f)).sum())
            past += int((f > n_in - 1).sum())
    measured('resize coordinates on the other side of an integer', crossed)
    measured('resize last coordinates past in - 1', past)
    assert crossed > 0 and past > 0


@pytest.mark.parametrize('defect, coords', [('fused', 'fp32'), ('unclamped', 'fp32')])
def test_resize_planted_defects_outside(defect, coords):
    """both defects are caught by the sharp form (the coordinate as fp32 defines it).  Against exact coordinates neither
    can be: a fused scale * index - x0 is CLOSER to the exact coordinate, and the unclamped tap only shows where the
    rounded coordinate overshoots in - 1 by an ulp, which the coordinate term allows for."""
    worst = 0.0
    for kind, planes, in_hw, out_hw in _resize_inputs():
        a, b = resize_case(kind, planes, in_hw)
        ref, bound = resize_ref(a, out_hw, 1.0, b, coords)
        assert worst_ratio(resize_fp32(a, out_hw, 1.0, b), ref, bound) <= 1.0
        worst = max(worst, worst_ratio(resize_fp32(a, out_hw, 1.0, b, defect=defect), ref, bound))
    measured(f'resize_bilinear defect {defect} / bound ({coords} coordinates)', worst)
    assert worst > 1.0


def test_avgpool_reference_inside():
    worst = 0.0
    for h, w in POOL_SIZES:
        x = torch.randn((6, h, w), generator=torch.Generator().manual_seed(h * 100 + w)) * 3 + 1
        ref, bound = avgpool_ref(x)
        assert ref.shape == (6, h // 2, w // 2)
        worst = max(worst, worst_ratio(F.avg_pool2d(x[None], 2, 2)[0], ref, bound))
    measured('avgpool2x2 torch fp32 / bound', worst)
    assert worst <= 1.0


def _convex_inputs():
    for size in CONVEX_SIZES:
        for regime in CONVEX_REGIMES:
            yield regime, size


def test_convex_reference_inside():
    worst = {}
    for regime, size in _convex_inputs():
        x, m, x_mul, mask_mul = convex_case(regime, size)
        ref, bound = convex_ref(x, m, x_mul, mask_mul)
        got = oracle.convex_upsample(x, mask_mul * m, x_mul=x_mul)
        worst[regime] = max(worst.get(regime, 0.0), worst_ratio(got, ref, bound), worst_ratio(convex_fp32(x, m, x_mul, mask_mul), ref, bound))
    for regime, v in worst.items():
        measured(f'convex_upsample oracle fp32 / bound, {regime}', v)
        assert v <= 1.0, regime


@pytest.mark.parametrize('defect', ['no_max', 'transposed'])
def test_convex_planted_defects_outside(defect):
    worst = 0.0
    for regime, size in _convex_inputs():
        x, m, x_mul, mask_mul = convex_case(regime, size)
        ref, bound = convex_ref(x, m, x_mul, mask_mul)
        worst = max(worst, worst_ratio(convex_fp32(x, m, x_mul, mask_mul, defect), ref, bound))
    measured(f'convex_upsample defect {defect} / bound', worst)
    assert worst > 1.0


def test_convex_nonfinite_reference():
    """what torch's softmax does with non-finite logits, per sub-pixel: a NaN or a +inf among the nine -> every output of
    that sub-pixel NaN; one -inf -> that weight is exactly 0, the rest finite; all nine -inf -> NaN.  convex_ref (float64
    softmax) and the fp32 oracle agree on the pattern."""
    size = (2, 2, 3, 33)
    for regime, all_nan in (('nan', True), ('pinf', True), ('one_ninf', False), ('all_ninf', None)):
        x, m, x_mul, mask_mul = convex_case(regime, size)
        ref, bound = convex_ref(x, m, x_mul, mask_mul)
        got = oracle.convex_upsample(x, mask_mul * m, x_mul=x_mul)
        assert same_nan_pattern(got, ref), regime
        nan = np.isnan(ref)
        if all_nan is True:
            assert nan.all()
        elif all_nan is False:
            assert not nan.any() and worst_ratio(got, ref, bound) <= 1.0
        else:                                                       # sub-pixel index sy * 8 + sx even <=> sx even
            assert nan[..., 0::2].all() and not nan[..., 1::2].any()
            assert worst_ratio(got.numpy()[..., 1::2], ref[..., 1::2], bound[..., 1::2]) <= 1.0


def _pose_inputs():
    for n in POSE_N:
        for mode in range(4):
            yield 'nominal', n, mode
    for regime in POSE_REGIMES[1:]:
        for mode in (1, 3):
            yield regime, 3, mode


def _pose_ratios(got, ref):
    d_rot, d_trans, (rv, re), (tv, te) = ref
    assert same_bits(got[0], d_rot) and same_bits(got[1], d_trans)
    return worst_ratio(got[2], rv, re), worst_ratio(got[3], tv, te)


def test_pose_update_reference_inside():
    worst = {}
    for regime, n, mode in _pose_inputs():
        case = pose_case(regime, n)
        ref = pose_update_ref(*case, mode)
        rr, rt = _pose_ratios(pose_update_fp32(*case, mode), ref)
        worst[regime] = max(worst.get(regime, 0.0), rr, rt)
        if regime not in ('zero_a', 'parallel'):
            assert np.isfinite(ref[2][1]).all() and ref[2][1].max() < 1e-2, regime      # a meaningful bound on R'
    for regime, v in worst.items():
        measured(f'pose_update oracle fp32 / bound, {regime}', v)
        assert v <= 1.0, regime


def test_pose_update_orthonormality_follows_from_the_bound():
    """R' R'^T - I of the float64 reference is 0 to float64 precision whenever R is orthonormal (to fp32 rounding) and
    a is not parallel to b, so |R^' R^'^T - I| <= 2 sum_k |R'_ik| e_jk + 3 U for any evaluation inside the bound."""
    case = pose_case('nominal', 70)
    _, _, (rv, re), _ = pose_update_ref(*case, 1)
    dev = np.abs(rv @ rv.transpose(0, 2, 1) - np.eye(3))
    assert dev.max() < 4 * U                                        # the input R is orthonormal only to fp32 rounding
    assert orthonormality_bound(rv, re).max() < 1e-4


def orthonormality_bound(rv, re):
    return np.abs(rv) @ re.transpose(0, 2, 1) + re @ np.abs(rv).transpose(0, 2, 1) + re @ re.transpose(0, 2, 1) + 4 * U


@pytest.mark.parametrize('defect', ['xzy', 'label0'])
def test_pose_update_planted_defects_outside(defect):
    worst = 0.0
    for regime, n, mode in _pose_inputs():
        if not (mode & LABEL_PER_SAMPLE) or n == 1 or regime in ('zero_a', 'parallel'):
            continue
        case = pose_case(regime, n)
        d_rot, d_trans, (rv, re), (tv, te) = pose_update_ref(*case, mode)
        got = pose_update_fp32(*case, mode, defect=defect)
        bad = max(worst_ratio(got[2], rv, re), worst_ratio(got[3], tv, te))
        bad = max(bad, 0.0 if same_bits(got[0], d_rot) and same_bits(got[1], d_trans) else float('inf'))
        assert bad > 1.0, (defect, regime, n, mode)
        worst = max(worst, min(bad, 1e30))
    measured(f'pose_update defect {defect} / bound', worst)


def _geom_inputs():
    for size in GEOM_SIZES:
        for pose in GEOM_POSES:
            yield pose, size, size[1] % 2 == 1


def test_geometry_reference_inside():
    """the fp32 restatement in the kernels' order inside the bounds of re- and un-projection on every case; the |qz|
    rule leaves out <= 1 % of the compared elements; the oracle's own fp32 path (LU inverses) is printed."""
    worst, worst_oracle = {}, 0.0
    for pose, size, skew in _geom_inputs():
        for invalid in (0.0, 400.0):
            case = geom_case(pose, size, skew)
            ref, bound, left = reproject_ref(*case, invalid)
            flow, pts = geom_fp32(*case, invalid)
            fg = f64(case[0]) > 0
            check_left_out(left, fg)
            keep = ~left[:, None].repeat(2, 1)
            worst['reproject ' + pose] = max(worst.get('reproject ' + pose, 0.0), worst_ratio(flow[keep], ref[keep], bound[keep]))
            assert same_bits(torch.from_numpy(flow[~fg[:, None].repeat(2, 1)]), torch.full((int((~fg).sum()) * 2,), invalid))
            pref, pbound = unproject_ref(*case[:4])
            worst['unproject'] = max(worst.get('unproject', 0.0), worst_ratio(pts, pref, pbound))
            o = oracle_reproject(*case, invalid).numpy()
            worst_oracle = max(worst_oracle, worst_ratio(o[keep], ref[keep], bound[keep]))
            assert np.array_equal(o[:, 0] == invalid, flow[:, 0] == invalid) or invalid == 0.0
    for key, v in worst.items():
        measured(f'{key} fp32 restatement / bound', v)
        assert v <= 1.0, key
    measured('reproject oracle fp32 (LU inverses) / bound -- not asserted', worst_oracle)


def test_geometry_identity_pose_is_a_cancellation_inside_the_bound():
    case = geom_case('identity', (3, 12, 20))
    ref, bound, left = reproject_ref(*case, 0.0)
    assert not left.any()
    assert np.abs(ref).max() < 1e-3 and bound.max() < 1e-2          # |flow| <= a few 1e-5 px: the bound is the test


def test_geometry_through_camera_leaves_out_exactly_the_qz_pixels():
    """the planted run d = 5 (1 + j 4e-6) puts pixels at and next to qz = 0: the rule names some of them (not all, not
    none), every other pixel keeps a finite bound, and there is no z > 0 guard: pixels behind the camera are compared."""
    case = geom_case('through_camera', (3, 12, 20))
    ref, bound, left = reproject_ref(*case, 400.0)
    fg = f64(case[0]) > 0
    assert 0 < left.sum() < 8 and left[0, 1, :8].sum() == left.sum()
    assert np.isfinite(bound[~left[:, None].repeat(2, 1)]).all()
    check_left_out(left, fg)
    assert (f64(case[0])[fg] < 5.0).any() and (f64(case[0])[fg] > 5.0).any()


def test_geometry_planted_defect_outside():
    worst = float('inf')
    for pose, size, skew in _geom_inputs():
        if size == (1, 1, 1):
            continue
        case = geom_case(pose, size, skew)
        ref, bound, left = reproject_ref(*case, 400.0)
        keep = ~left[:, None].repeat(2, 1)
        flow, pts = geom_fp32(*case, 400.0, defect='r0_not_inverted')
        pref, pbound = unproject_ref(*case[:4])
        worst = min(worst, worst_ratio(flow[keep], ref[keep], bound[keep]), worst_ratio(pts, pref, pbound))
    measured('re-/un-projection defect R0 for R0^-1 / bound (least)', worst)
    assert worst > 1.0


def test_geometry_nan_depth_is_background_in_the_reference():
    case = geom_case('large_rotation', (2, 5, 7))
    assert torch.isnan(case[0]).sum() == 1
    o = oracle_reproject(*case, 400.0)
    nan_at = torch.isnan(case[0])
    assert (o[:, 0][nan_at] == 400.0).all() and (o[:, 1][nan_at] == 400.0).all() and not torch.isnan(o).any()
    ref, _, _ = reproject_ref(*case, 400.0)
    assert (ref[:, 0][nan_at.numpy()] == 400.0).all()
    pref, _ = unproject_ref(*case[:4])
    assert (pref[:, :, nan_at[0].numpy()][0] == 0).all() and not np.isnan(pref).any()


def _filter_inputs():
    for size in FILTER_SIZES:
        for kind in ('binary', 'smooth'):
            for ac in (False, True):
                yield kind, size, ac


def test_filter_reference_inside():
    """oracle.filter_flow_by_mask (grid_sample) makes the restatement's decision wherever it is certain, bit for bit; at
    most 1 % of the vectors are uncertain."""
    worst = 0.0
    for kind, size, ac in _filter_inputs():
        flow, mask = filter_case(kind, size)
        expect, certain = filter_ref(flow, mask, FILTER_INVALID, ac)
        worst = max(worst, check_left_out(~certain, np.ones_like(certain)))
        assert filter_agrees(filter_fp32(flow, mask, FILTER_INVALID, ac), expect, certain), (kind, size, ac)
    measured('filter_flow_by_mask share of vectors inside 0.9 +- margin (worst case)', worst)


def test_filter_nonfinite_reference():
    """the recorded behaviour of the reference: a NaN, +inf, -inf or overflowing (3e38) component keeps the vector
    (grid_sample returns NaN, NaN < 0.9 is false) unless both components are >= invalid_num; +-1e9 samples padding and
    is invalid -- except on a 1 x 1 image with align_corners=True, where every coordinate is multiplied by size - 1 = 0."""
    inf, nan = float('inf'), float('nan')
    for h, w in ((5, 7), (1, 1)):
        for ac in (False, True):
            mask = torch.ones((1, h, w))
            for vec, kept in (((nan, 0.0), True), ((0.0, nan), True), ((inf, 0.0), True), ((0.0, -inf), True),
                              ((3e38, 0.0), True), ((0.0, -3e38), True), ((inf, 500.0), False), ((inf, inf), False),
                              ((nan, nan), True), ((1e9, 0.0), (h, w, ac) == (1, 1, True)), ((0.0, -1e9), (h, w, ac) == (1, 1, True))):
                flow = torch.zeros((1, 2, h, w))
                flow[0, 0], flow[0, 1] = vec
                got = oracle.filter_flow_by_mask(flow, mask, FILTER_INVALID, align_corners=ac)
                want = flow if kept else torch.full_like(flow, FILTER_INVALID)
                assert same_bits(got, want), (vec, h, w, ac)
                expect, certain = filter_ref(flow, mask, FILTER_INVALID, ac)
                assert certain.all() and same_bits(expect, want), (vec, h, w, ac)


def test_filter_planted_defect_outside():
    bad = 0
    for kind, size, ac in _filter_inputs():
        if ac or size == (1, 1, 1):
            continue
        flow, mask = filter_case(kind, size)
        expect, certain = filter_ref(flow, mask, FILTER_INVALID, ac)
        bad += not filter_agrees(filter_fp32(flow, mask, FILTER_INVALID, ac, 'denorm_wm1'), expect, certain)
    assert bad == 4                                                 # every align_corners=False case above 1 x 1
