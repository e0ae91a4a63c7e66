"""The per-ray kernels of a training step (csrc/eonerf_rays.hip, csrc/eonerf_rays_bwd.hip, csrc/eonerf_ambient_dev.h) restated in plain torch
(device-agnostic), and the decoding of the per-ray buffers a render call leaves in the caller's workspace.

WHERE the buffers lie is asked of the library (eonerf_ray_layout / eonerf_workspace_layout, include/eonerf_layout.h).  RAY_REC and the RR_*
columns of a ray record are read from csrc/eonerf_rays.h (K()), not restated.

Every operation is written ONCE, in the operation order of its kernel, over an arithmetic `A`:

  * Ref  -- the float64 reference.  A number is an EV: the float64 value `v` of the exact operation on the inputs' bits, and `e`, a bound
            on |what the fp32 kernel computes - v| accumulated operation by operation (running error analysis, Higham, Accuracy and
            Stability of Numerical Algorithms, 3.3):  every fp32 operation returns the rounded exact result of its (perturbed) operands,
            |fl(x) - x| <= u |x| with u = 2^-24, plus 2^-126 where a result in the denormal range may be flushed to zero;
            the device expf / logf / sinf are allowed LIBM = 8 u relative (the project's allowance, tests/slab_checks.py: "8 fp32 ulp for the
            device expf / log1pf"); a k-term sum in the kernel's tree or scan order is within gamma(k) of the sum of the magnitudes.
            Nothing in `e` is fitted: it scales with the magnitudes of the terms that enter an element, never with |v| of a cancelling
            difference and never with a tensor norm.  A contracted multiply-add rounds once where the model rounds twice: covered.
  * F32  -- plain fp32 torch, the same operations in the kernel's own order (Hillis-Steele scans, butterfly sums): an emulation of the
            kernel, used by tests/test_ray_checks_cpu.py to build clean and defective workspaces.  `defect` names one seeded fault.
"""
import functools
import os
import re

import torch

import workspace_guard as wg

F64, F32T = torch.float64, torch.float32
U = 2.0 ** -24
TINY = 2.0 ** -126
LIBM = 8 * U
BETA_MIN = 0.05


def gamma(k):
    return k * U / (1.0 - k * U)


@functools.lru_cache(maxsize=None)
def K():
    """RAY_REC and the RR_* columns, from the one `constexpr int RR_DEPTH = 0, ..., RAY_REC = 12;` of csrc/eonerf_rays.h."""
    text = open(os.path.join(wg.CSRC, "eonerf_rays.h")).read()
    m = re.search(r"constexpr\s+int\s+(RR_DEPTH\s*=[^;]*);", text)
    if not m:
        raise RuntimeError("ray_restated: the ray record's columns not found in eonerf_rays.h")
    c = {k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)", m.group(1))}
    for name in ("RR_DEPTH", "RR_ALB", "RR_TS", "RR_TB", "RR_WSUM", "RR_AMB", "RR_GEO", "RAY_REC"):
        if name not in c:
            raise RuntimeError(f"ray_restated: {name} not found in eonerf_rays.h")
    return c


def f32c(c):
    """The fp32 constant the kernel holds for the literal c (0.2f, 0.05f), as a Python float."""
    return float(torch.tensor(c, dtype=F32T))


# ------------------------------------------------------------------------------------------------------------ eonerf_ray_layout
RAY_LAYOUT = ["cnt_first", "cnt_retry", "flags", "ray_rec", "g_ray", "amb_save", "rad_rays", "emb_rays"]      # order of include/eonerf_layout.h
RAY_ENTRIES = len(RAY_LAYOUT)
LAYOUT_NONE = (1 << 64) - 1


def ray_layout_dict(table):
    table = [int(v) for v in table]
    assert len(table) == RAY_ENTRIES
    return {k: v for k, v in zip(RAY_LAYOUT, table) if v != LAYOUT_NONE}


class RayView:
    """The per-ray buffers of a render call: ws uint8 [bytes], off = ray_layout_dict(...), R rays."""

    def __init__(self, ws, off, R):
        self.ws, self.off, self.R = ws, off, R

    def has(self, name):
        return name in self.off

    def _v(self, name, dtype, n):
        o = self.off[name]
        return self.ws[o:o + 4 * n].view(dtype)

    def i32(self, name, n=None):
        return self._v(name, torch.int32, self.R if n is None else n)

    def rec(self, name="ray_rec"):
        return self._v(name, F32T, self.R * K()["RAY_REC"]).view(self.R, K()["RAY_REC"])

    def f32(self, name, cols):
        return self._v(name, F32T, self.R * cols).view(self.R, cols)


class PassView:
    """The per-sample arrays of one pass: off = a pass dict of slab_restated.layout_dict, W = 64 * slots per lane of the kernels' instance."""

    def __init__(self, ws, off, p_cap, R, n_samples):
        self.ws, self.off, self.p_cap, self.R = ws, off, p_cap, R
        self.W = 64 if n_samples <= 64 else (256 if n_samples > 128 else 128)
        self.counts = ws[off["counts"]:off["counts"] + 4 * R].view(torch.int32).long()
        self.offsets = ws[off["offsets"]:off["offsets"] + 4 * (R + 1)].view(torch.int32).long()
        self.n = int(ws[off["n_pts"]:off["n_pts"] + 4].view(torch.int32)[0])
        slot = torch.arange(self.W, device=ws.device)[None]
        self.mask = slot < self.counts[:, None]
        self.idx = torch.where(self.mask, self.offsets[:R, None] + slot, torch.zeros_like(slot))

    def has(self, name):
        return name in self.off

    def flat(self, name, rows=1):
        o = self.off[name]
        return self.ws[o:o + 4 * rows * self.p_cap].view(F32T).view(rows, self.p_cap)

    def dense(self, name, row=0, rows=1):
        """[R, W] fp32: slot i of ray r = element offsets[r] + i; zeros beyond the ray's count."""
        v = self.flat(name, rows)[row][self.idx]
        return torch.where(self.mask, v, torch.zeros_like(v))


def build_image(ray, cam, sun, p_cap):
    """Inverse of the two views: a synthetic workspace (uint8, prefilled with 0xFF) at made-up 256-byte aligned offsets.
    ray: name -> tensor; cam / sun: member -> tensor (int32 or fp32; per-sample arrays [rows, p_cap]); -> (ws, ray off, cam off, sun off)."""
    parts, pos = [], 0

    def put(t):
        nonlocal pos
        pos = (pos + 255) // 256 * 256
        b = t.contiguous().reshape(-1).view(torch.uint8)
        parts.append((pos, b))
        o = pos
        pos += b.numel()
        return o
    offs = [{k: put(v) for k, v in d.items()} if d is not None else None for d in (ray, cam, sun)]
    ws = torch.full((pos + 256,), 0xFF, dtype=torch.uint8)
    for o, b in parts:
        ws[o:o + b.numel()] = b
    return ws, offs[0], offs[1], offs[2]


# ------------------------------------------------------------------------------------------------------------ arithmetics
class EV:
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v.to(F64)
        self.e = torch.zeros_like(self.v) if e is None else e

    def __getitem__(self, i):
        return EV(self.v[i], self.e[i])

    @property
    def shape(self):
        return self.v.shape

    def mag(self):
        return self.v.abs() + self.e


def _lane():
    return torch.arange(64)


class F32:
    """fp32 torch, one rounding per operation, the kernels' own summation orders."""
    ref = False

    @staticmethod
    def inp(x):
        return x.to(F32T)

    @staticmethod
    def full(like, c):
        return torch.full_like(like, c)

    mul = staticmethod(lambda a, b: a * b)
    add = staticmethod(lambda a, b: a + b)
    sub = staticmethod(lambda a, b: a - b)
    div = staticmethod(lambda a, b: a / b)
    neg = staticmethod(lambda a: -a)
    scale2 = staticmethod(lambda a, p: a * p)
    expneg = staticmethod(lambda a: torch.exp(-a))
    log = staticmethod(torch.log)
    sin = staticmethod(torch.sin)
    relu = staticmethod(lambda a: a.clamp_min(0))
    clamp01 = staticmethod(lambda a: a.clamp(0, 1))
    where = staticmethod(lambda m, a, b: torch.where(m, a, b))
    val = staticmethod(lambda a: a)
    take = staticmethod(lambda a, idx: a.gather(-1, idx))
    stack = staticmethod(lambda xs, dim=-1: torch.stack(xs, dim))

    @staticmethod
    def mulc(a, c):
        return a * torch.tensor(c, dtype=F32T, device=a.device)

    @staticmethod
    def wave_sum(x):
        """v += shfl_xor(v, o), o = 32 .. 1, over the last dimension of 64."""
        ln = _lane().to(x.device)
        for o in (32, 16, 8, 4, 2, 1):
            x = x + x[..., ln ^ o]
        return x[..., 0]

    @staticmethod
    def _incl(x, down):
        ln = _lane().to(x.device)
        for o in (1, 2, 4, 8, 16, 32):
            src = ln + o if down else ln - o
            ok = (src >= 0) & (src < 64)
            x = torch.where(ok, x + x[..., src.clamp(0, 63)], x)
        return x

    @classmethod
    def excl_prefix(cls, x):
        """ray_weights: x [R, SPL, 64] -> exclusive prefix over i = lane + 64 k (carry of the groups in front)."""
        out, carry = [], torch.zeros_like(x[:, 0, 0])
        for k in range(x.shape[1]):
            inc = cls._incl(x[:, k], False)
            prev = torch.cat([torch.zeros_like(inc[:, :1]), inc[:, :-1]], 1)
            ex = carry[:, None] + prev
            ex[:, 0] = carry
            out.append(ex)
            carry = carry + inc[:, 63]
        return torch.stack(out, 1)

    @classmethod
    def excl_suffix(cls, x, no_carry=False):
        """k_cam_composite_bwd: exclusive suffix sums (carry of the groups behind)."""
        spl = x.shape[1]
        out, carry = [None] * spl, torch.zeros_like(x[:, 0, 0])
        for k in range(spl - 1, -1, -1):
            suf = cls._incl(x[:, k], True)
            nxt = torch.cat([suf[:, 1:], torch.zeros_like(suf[:, :1])], 1)
            out[k] = nxt if (k == spl - 1 or no_carry) else nxt + carry[:, None]
            carry = carry + suf[:, 0]
        return torch.stack(out, 1)

    @classmethod
    def ray_sum(cls, x):
        """acc += term over the lane's slots k, then wave_sum: x [R, SPL, 64] -> [R]."""
        acc = x[:, 0]
        for k in range(1, x.shape[1]):
            acc = acc + x[:, k]
        return cls.wave_sum(acc)

    @staticmethod
    def seq_sum(xs, first=None):
        acc = first
        for x in xs:
            acc = x if acc is None else acc + x
        return acc

    @staticmethod
    def affine(b, W, X):
        """acc = b; acc = acc + W[j][i] X[i], i ascending: b [J], W [J, I], X [R, I] -> [R, J]."""
        acc = b[None].expand(X.shape[0], -1).clone()
        for i in range(W.shape[1]):
            acc = acc + W[None, :, i] * X[:, i:i + 1]
        return acc

    @staticmethod
    def sum_any(x, dim=0):
        return x.sum(dim)

    @staticmethod
    def index_sum(x, idx, n):
        return torch.zeros((n,) + x.shape[1:], dtype=x.dtype).index_add_(0, idx, x)

    @classmethod
    def block_sum(cls, part, first):
        """k_shade_bwd / k_loss: per-ray terms [R] -> waves of 64 rays (wave_sum), (s0 + s1) + (s2 + s3) per block of 256, then the blocks
        in order on top of `first`."""
        R = part.shape[0]
        nb = (R + 255) // 256
        p = torch.zeros(nb * 256, dtype=part.dtype)
        p[:R] = part
        s = cls.wave_sum(p.view(nb, 4, 64))
        blk = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
        total = torch.tensor(first, dtype=F32T)
        for b in range(nb):
            total = total + blk[b]
        return total


class Ref:
    """float64 values with a running bound on the fp32 kernel's error (module docstring)."""
    ref = True

    @staticmethod
    def inp(x):
        return EV(x)

    @staticmethod
    def full(like, c):
        return EV(torch.full_like(like.v, f32c(c)))

    @staticmethod
    def _r(v, e):
        return EV(v, e + U * (v.abs() + e) + TINY)

    @classmethod
    def mul(cls, a, b):
        return cls._r(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)

    @classmethod
    def mulc(cls, a, c):
        c = f32c(c)
        return cls._r(a.v * c, a.e * abs(c))

    @classmethod
    def add(cls, a, b):
        return cls._r(a.v + b.v, a.e + b.e)

    @classmethod
    def sub(cls, a, b):
        return cls._r(a.v - b.v, a.e + b.e)

    @classmethod
    def div(cls, a, b):
        den = b.v.abs() - b.e
        assert bool((den > 0).all()), "a divisor that may vanish"
        v = a.v / b.v
        return cls._r(v, a.mag() / den - v.abs())

    @staticmethod
    def neg(a):
        return EV(-a.v, a.e)

    @staticmethod
    def scale2(a, p):
        return EV(a.v * p, a.e * p)       # a power of two: exact

    @staticmethod
    def expneg(a):
        """expf(-a): exp(-(a +- e)) is within exp(-a) expm1(e) of exp(-a); then LIBM relative, and the flush floor."""
        v = torch.exp(-a.v)
        e = torch.where(v > 0, v * torch.expm1(a.e.clamp_max(700.0)), torch.exp(a.e - a.v))      # (v == 0: exp(-(a - e)) itself)
        return EV(v, e + LIBM * (v + e) + TINY)

    @staticmethod
    def log(a):
        assert bool((a.v > a.e).all())
        v = torch.log(a.v)
        e = -torch.log1p(-a.e / a.v)
        return EV(v, e + LIBM * (v.abs() + e) + TINY)

    @staticmethod
    def sin(a):
        v = torch.sin(a.v)
        return EV(v, a.e + LIBM * (v.abs() + a.e) + TINY)

    @staticmethod
    def relu(a):
        return EV(a.v.clamp_min(0), a.e)      # |max(x', 0) - max(x, 0)| <= |x' - x|

    @staticmethod
    def clamp01(a):
        return EV(a.v.clamp(0, 1), a.e)

    @staticmethod
    def where(m, a, b):
        return EV(torch.where(m, a.v, b.v), torch.where(m, a.e, b.e))

    @staticmethod
    def val(a):
        return a.v

    @staticmethod
    def take(a, idx):
        return EV(a.v.gather(-1, idx), a.e.gather(-1, idx))

    @staticmethod
    def stack(xs, dim=-1):
        return EV(torch.stack([x.v for x in xs], dim), torch.stack([x.e for x in xs], dim))

    @staticmethod
    def _tree(v, e, m, depth):
        """A sum whose every term passes through at most `depth` fp32 additions: within gamma(depth) of the summed magnitudes m."""
        return EV(v, e + gamma(depth) * m + TINY)

    @classmethod
    def wave_sum(cls, x):
        return cls._tree(x.v.sum(-1), x.e.sum(-1), x.mag().sum(-1), 6)

    @classmethod
    def excl_prefix(cls, x):
        """Hillis-Steele inclusive scan (6 levels), + carry (1), the carry's own chain (SPL - 1): depth <= 6 + SPL."""
        R, spl, _ = x.shape
        # (shifted, never inclusive - self: the camera pass' last interval has sigma delta ~ 1e10 and would cancel the whole prefix)
        ex = lambda t: torch.cat([torch.zeros(R, 1, dtype=F64, device=t.device), t.reshape(R, -1).cumsum(1)[:, :-1]], 1).reshape(R, spl, 64)      # noqa: E731
        return cls._tree(ex(x.v), ex(x.e), ex(x.mag()), 6 + spl)

    @classmethod
    def excl_suffix(cls, x, no_carry=False):
        R, spl, _ = x.shape
        assert not no_carry
        sx = lambda t: torch.cat([t.reshape(R, -1).flip(1).cumsum(1).flip(1)[:, 1:], torch.zeros(R, 1, dtype=F64, device=t.device)], 1).reshape(R, spl, 64)      # noqa: E731
        return cls._tree(sx(x.v), sx(x.e), sx(x.mag()), 6 + spl)

    @classmethod
    def ray_sum(cls, x):
        return cls._tree(x.v.sum((1, 2)), x.e.sum((1, 2)), x.mag().sum((1, 2)), 6 + x.shape[1] - 1)

    @classmethod
    def seq_sum(cls, xs, first=None):
        xs = list(xs) if first is None else [first] + list(xs)
        return cls._tree(sum(x.v for x in xs), sum(x.e for x in xs), sum(x.mag() for x in xs), len(xs) - 1)

    @classmethod
    def affine(cls, b, W, X):
        """I products and I additions per element: gamma(I + 1) of |b| + sum |w x| (Higham 3.1, a dot product with a bias)."""
        v = b.v[None] + X.v @ W.v.t()
        m = b.v.abs()[None] + X.v.abs() @ W.v.abs().t()
        return EV(v, gamma(W.shape[1] + 1) * m + TINY)

    @classmethod
    def sum_any(cls, x, dim=0):
        n = x.shape[dim]
        return cls._tree(x.v.sum(dim), x.e.sum(dim), x.mag().sum(dim), max(n - 1, 1))

    @classmethod
    def index_sum(cls, x, idx, n):
        """Per table row, the sum over its rays in ANY order (atomics): gamma(rays of the row)."""
        z = lambda t: torch.zeros((n,) + t.shape[1:], dtype=F64, device=t.device).index_add_(0, idx, t)      # noqa: E731
        cnt = torch.bincount(idx, minlength=n).to(F64).clamp_min(1.0)
        g = (cnt * U / (1 - cnt * U)).view(-1, *([1] * (x.v.dim() - 1)))
        return EV(z(x.v), z(x.e) + g * z(x.mag()) + TINY)

    @classmethod
    def block_sum(cls, part, first):
        nb = (part.shape[0] + 255) // 256
        return cls._tree(part.v.sum() + first, part.e.sum(), part.mag().sum() + abs(first), 6 + 2 + nb)


# ------------------------------------------------------------------------------------------------------------ the operations
def _g(x, spl):
    """[R, W] -> [R, SPL, 64] (slot i = lane + 64 k)."""
    if isinstance(x, EV):
        return EV(x.v.view(x.v.shape[0], spl, 64), x.e.view(x.v.shape[0], spl, 64))
    return x.view(x.shape[0], spl, 64)


def _u(x):
    if isinstance(x, EV):
        return EV(x.v.reshape(x.v.shape[0], -1), x.e.reshape(x.v.shape[0], -1))
    return x.reshape(x.shape[0], -1)


def ray_weights(A, sigma, delta, mask, defect=None):
    """ray_weights<SPL>: sd = sigma delta (0 beyond the ray's count), ex = exclusive prefix, T = expf(-ex), e = expf(-sd),
    w = T (1 - e).  All [R, W]."""
    spl = mask.shape[1] // 64
    zero = A.full(sigma, 0.0)
    sd = A.where(mask, A.mul(sigma, delta), zero)
    ex = _u(A.excl_prefix(_g(sd, spl)))
    if defect == "inclusive_T":        # ray 3: the transmittance takes the sample's own interval in
        row = torch.zeros_like(mask)
        row[3] = True
        ex = A.where(row, A.add(ex, sd), ex)
    T = A.expneg(ex)
    e = A.expneg(sd)
    w = A.where(mask, A.mul(T, A.sub(A.full(e, 1.0), e)), zero)
    return dict(sd=sd, ex=ex, T=T, e=e, w=w)


def composite_record(A, rw, tmid, albedo, ts, tb, depth_only=False, defect=None):
    """k_composite_fwd: [depth, alb0, alb1, alb2, ts, tb + 0.05f, wsum] per ray; the head sums are 0 for depth_only."""
    spl = rw["w"].shape[1] // 64
    s = lambda x: A.ray_sum(_g(A.mul(rw["w"], x), spl))      # noqa: E731
    depth = s(tmid)
    zero = A.full(depth, 0.0)
    heads = [zero] * 5 if depth_only else [s(albedo[0]), s(albedo[1]), s(albedo[2]), s(ts), s(tb)]
    wsum = A.ray_sum(_g(rw["w"], spl))
    tbv = A.add(heads[4], A.full(depth, BETA_MIN))
    if defect == "no_beta_min":         # ray 4: beta without beta_min
        tbv = tbv.clone()
        tbv[4] = heads[4][4]
    return [depth] + heads[:4] + [tbv, wsum]


def geo_shadow(A, rw, counts, defect=None):
    """k_composite_fwd (shadow_only): T at the last valid sample, exactly 1 for an empty ray."""
    last = (counts - 1).clamp_min(0)[:, None]
    if defect == "geo_late":            # T one sample further: inclusive of the last sample
        tl = A.take(A.expneg(A.add(rw["ex"], rw["sd"])), last)
    else:
        tl = A.take(rw["T"], last)
    tl = tl[:, 0]
    return A.where(counts > 0, tl, A.full(tl, 1.0))


def shade(A, rec, tabA, tabb, use_shadow):
    """shade_ray: rec = the record's columns (list of RAY_REC), tabA / tabb = the ray's radiometric gains / offsets (3 each).
    -> {column: value} of the computed columns 0..2, 7..9, 18..20, and pre / lin per channel."""
    k = K()
    one = A.full(rec[0], 1.0)
    wsum, ts = rec[k["RR_WSUM"]], rec[k["RR_TS"]]
    s = A.mul(rec[k["RR_GEO"]], ts) if use_shadow else one
    out, pre_l, lin_l, amb_l = {}, [], [], []
    for c in range(3):
        alb = rec[k["RR_ALB"] + c]
        amb = A.mulc(A.mul(wsum, rec[k["RR_AMB"] + c]), 0.2)
        pre = A.add(A.mul(alb, s), A.mul(A.sub(one, s), A.mul(amb, alb)))
        lin = A.add(A.mul(tabA[c], pre), tabb[c])
        out[c] = A.clamp01(lin)
        out[7 + c] = amb
        out[18 + c] = A.add(A.mul(tabA[c], alb), tabb[c])
        pre_l.append(pre), lin_l.append(lin), amb_l.append(amb)
    return out, dict(s=s, pre=pre_l, lin=lin_l, amb=amb_l)


def loss_terms(A, rgb, beta, gt, n, kind):
    """k_loss / the loss inside k_shade_bwd: per ray the term of the mean and the gradient columns {0, 1, 2[, 12]}."""
    one = A.full(rgb[0], 1.0)
    nf = A.full(rgb[0], float(n))
    inv = A.div(one, A.mulc(nf, 3.0))
    df = [A.sub(rgb[c], gt[c]) for c in range(3)]
    go = {}
    if kind == 0:
        part = A.seq_sum([A.mul(A.mul(d, d), inv) for d in df], first=A.full(rgb[0], 0.0))
        for c in range(3):
            go[c] = A.mul(A.mulc(df[c], 2.0), inv)
        return part, go
    ib2 = A.div(one, A.mul(beta, beta))
    sq = A.seq_sum([A.mul(d, d) for d in df], first=A.full(rgb[0], 0.0))
    for c in range(3):
        go[c] = A.mul(A.mul(df[c], ib2), inv)
    part = A.add(A.mul(A.mul(A.mulc(sq, 0.5), ib2), inv), A.div(A.mulc(A.log(beta), 0.5), nf))
    go[12] = A.add(A.mul(A.div(A.mul(A.neg(sq), ib2), beta), inv), A.div(A.full(beta, 0.5), A.mul(nf, beta)))
    return part, go


def loss_total(A, part, kind, defect=None):
    return A.block_sum(part, 1.5 if (kind == 1 and defect != "no_three_halves") else 0.0)


def shade_bwd(A, rec, go, tabA, tabb, use_shadow, defect=None, force_pass=None):
    """k_shade_bwd: go = {column: gradient of out} (absent = 0).  -> g = {record column: value}, rad = the ray's six table terms
    (dA3, db3), lin per channel.  The clip gradient passes for 0 <= lin <= 1 (lin recomputed as in the forward).
    force_pass [3][R] bool: take the clip decision from there (the kernel's own, for the rays where float64 cannot decide)."""
    k = K()
    zero, one = A.full(rec[0], 0.0), A.full(rec[0], 1.0)
    gz = lambda c: go.get(c, zero)      # noqa: E731
    _, f = shade(A, rec, tabA, tabb, use_shadow)
    s, wsum, ts, geo = f["s"], rec[k["RR_WSUM"]], rec[k["RR_TS"]], rec[k["RR_GEO"]]
    oms = A.sub(one, s)
    g, rad_a, rad_b, g_s_terms, g_w_terms = {}, [], [], [], []
    for c in range(3):
        alb, head, amb, pre, lin = rec[k["RR_ALB"] + c], rec[k["RR_AMB"] + c], f["amb"][c], f["pre"][c], f["lin"][c]
        lv = A.val(lin)
        passes = (lv >= 0) & (lv <= 1) if force_pass is None else force_pass[c]
        if defect == "clip_open":
            passes = torch.ones_like(passes)
        g_lin = A.where(passes, gz(c), zero)
        g_shl = gz(18 + c)
        rad_a.append(A.add(A.mul(g_lin, pre), A.mul(g_shl, alb)))
        rad_b.append(A.add(g_lin, g_shl))
        g_pre = A.mul(g_lin, tabA[c])
        g[k["RR_ALB"] + c] = A.add(A.add(A.mul(g_pre, A.add(s, A.mul(oms, amb))), gz(4 + c)), A.mul(g_shl, tabA[c]))
        g_amb = A.add(A.mul(A.mul(g_pre, oms), alb), gz(7 + c))
        g_s_terms.append(A.mul(g_pre, A.sub(alb, A.mul(amb, alb))))
        g02 = g_amb if defect == "no_02_in_g_wsum" else A.mulc(g_amb, 0.2)
        g_w_terms.append(A.mul(g02, head))
        g[k["RR_AMB"] + c] = A.mul(A.mulc(g_amb, 0.2), wsum)
    g_s = A.seq_sum(g_s_terms, first=zero)
    g[k["RR_WSUM"]] = A.seq_sum(g_w_terms, first=zero)
    g[k["RR_DEPTH"]] = gz(3)
    g[k["RR_TB"]] = gz(12)
    if use_shadow:
        g[k["RR_TS"]] = A.add(A.mul(g_s, geo), gz(11))
        g[k["RR_GEO"]] = A.add(A.mul(g_s, ts), gz(10))
    else:
        g[k["RR_TS"]] = A.add(zero, gz(11))
        g[k["RR_GEO"]] = zero
    return g, rad_a + rad_b, f["lin"]


def rendering_out(A, rec):
    """k_rendering_out: ambient = wsum * head per channel (the other outputs are copies)."""
    k = K()
    return [A.mul(rec[k["RR_WSUM"]], rec[k["RR_AMB"] + c]) for c in range(3)]


def rendering_out_bwd(A, rec, g_ambient):
    """k_rendering_out_bwd: g[AMB + c] = ga_c wsum, g[WSUM] = sum_c ga_c head_c (from 0, c ascending); the rest are copies."""
    k = K()
    g = {k["RR_AMB"] + c: A.mul(g_ambient[c], rec[k["RR_WSUM"]]) for c in range(3)}
    g[k["RR_WSUM"]] = A.seq_sum([A.mul(g_ambient[c], rec[k["RR_AMB"] + c]) for c in range(3)], first=A.full(rec[0], 0.0))
    return g


def cam_composite_bwd(A, rw, mask, delta, tmid, albedo, ts, tb, g, view_d=None, sun_gpos=None, depth_only=False, defect=None):
    """k_cam_composite_bwd.  g = the record's gradient columns (list of RAY_REC, [R]); sun_gpos = the three [R, W] gathers of the sun pass'
    g_pos over the ray's shadow samples (zeros beyond their count) and view_d the ray's direction (3 x [R]), or None.
    -> g_sigma, [g_alb0, g_alb1, g_alb2], g_ts, g_tb (all [R, W])."""
    k = K()
    spl = mask.shape[1] // 64
    zero = A.full(delta, 0.0)
    bc = lambda x: _bcast(A, x, mask.shape[1])      # noqa: E731
    g_depth = g[k["RR_DEPTH"]]
    if sun_gpos is not None and defect != "no_sun_depth_term":
        t = A.add(A.add(A.mul(sun_gpos[0], bc(view_d[0])), A.mul(sun_gpos[1], bc(view_d[1]))), A.mul(sun_gpos[2], bc(view_d[2])))
        g_depth = A.add(g_depth, A.ray_sum(_g(t, spl)))
    w = rw["w"]
    gw = A.mul(bc(g_depth), tmid)
    outs = None
    if not depth_only:
        galb = [bc(g[k["RR_ALB"] + c]) for c in range(3)]
        gts, gtb = bc(g[k["RR_TS"]]), bc(g[k["RR_TB"]])
        for c in range(3):
            gw = A.add(gw, A.mul(galb[c], albedo[c]))
        gw = A.add(A.add(A.add(gw, A.mul(gts, ts)), A.mul(gtb, tb)), bc(g[k["RR_WSUM"]]))
        outs = [A.where(mask, A.mul(w, x), zero) for x in galb + [gts, gtb]]
        if defect == "g_albedo_ulp":      # one element a few fp32 ulp off
            v = outs[1].clone()
            v[6, 0] = v[6, 0] * (1 + 2.0 ** -19)
            outs[1] = v
    gw = A.where(mask, gw, zero)
    gw_w = A.mul(gw, w)
    after = _u(A.excl_suffix(_g(gw_w, spl), no_carry=(defect == "suffix_no_carry")))
    g_sigma = A.where(mask, A.mul(delta, A.sub(A.mul(A.mul(gw, rw["T"]), rw["e"]), after)), zero)
    return (g_sigma,) + ((None, None, None) if outs is None else (outs[:3], outs[3], outs[4]))


def _bcast(A, x, W):
    if isinstance(x, EV):
        return EV(x.v[:, None].expand(-1, W), x.e[:, None].expand(-1, W))
    return x[:, None].expand(-1, W)


def sun_composite_bwd(A, g_geo, geo, delta, mask, counts, defect=None):
    """k_sun_composite_bwd: g_sigma_i = (-g_geo geo) delta_i for i < n - 1, exactly 0 at i = n - 1."""
    W = mask.shape[1]
    zero = A.full(delta, 0.0)
    v = A.mul(_bcast(A, A.mul(A.neg(g_geo), geo), W), delta)
    slot = torch.arange(W, device=mask.device)[None]
    inner = slot < (counts[:, None] - 1)
    if defect == "sun_last_nonzero":
        inner = mask
    return A.where(inner, v, zero)


PI_2_F = 1.57079637050628662109375


def ambient_encoding(A, sun):
    """sun_encoding_wave: [x, y, z, sin(2^k c_d) (k, d), sin(2^k c_d + fp32(pi / 2)) (k, d)], k = 0..3: 27 values; sun = 3 x [R]."""
    enc = list(sun)
    for half in (0, 1):
        for kk in range(4):
            for d in range(3):
                xb = A.scale2(sun[d], float(1 << kk))
                enc.append(A.sin(xb if half == 0 else A.add(xb, A.full(xb, PI_2_F))))
    return enc


def ambient_hidden(A, enc27, w1, b1):
    """hid = max(b1 + sum_i w1[j][i] enc[i], 0): enc27 [R, 27] -> [R, 128]."""
    return A.relu(A.affine(b1, w1, enc27))


def ambient_out(A, hid, w2, b2):
    """out_o = sigmoid_f(wave_sum(w2[o][lane] hid[lane] + w2[o][lane + 64] hid[lane + 64]) + b2[o]); hid [R, 128] -> 3 x [R]."""
    out = []
    for o in range(3):
        if A.ref:
            prod = A.mul(EV(w2.v[o][None].expand_as(hid.v)), hid)
            lo, hi = EV(prod.v[:, :64], prod.e[:, :64]), EV(prod.v[:, 64:], prod.e[:, 64:])
            b = EV(b2.v[o].expand(hid.v.shape[0]))
        else:
            prod = w2[o][None] * hid
            lo, hi = prod[:, :64], prod[:, 64:]
            b = b2[o].expand(hid.shape[0])
        pre = A.add(A.wave_sum(A.add(lo, hi)), b)
        one = A.full(pre, 1.0)
        out.append(A.div(one, A.add(one, A.expneg(pre))))
    return out


def ambient_bwd(A, g_amb, out, enc27, hid, w2, defect=None):
    """ambient_bwd_body: per ray gpre_o = (g_o out_o) (1 - out_o), ghid_j = sum_o w2[o][j] gpre_o (0 where the saved hid_j <= 0);
    d_w2[o][j] = sum_r gpre_o hid_j, d_b2 = sum_r gpre, d_b1 = sum_r ghid, d_w1[j][i] = sum_r ghid_j enc_i -- the rays in any order
    (streams, blocks, atomics).  g_amb, out: 3 x [R]; enc27 [R, 27]; hid [R, 128]; w2 [3, 128]."""
    R = A.val(hid).shape[0]
    one = A.full(out[0], 1.0)
    gpre = [A.mul(A.mul(g_amb[o], out[o]), A.sub(one, out[o])) for o in range(3)]
    hv = A.val(hid)
    alive = hv > 0
    if defect == "relu_leak":
        alive = alive.clone()
        r = int(A.val(gpre[0]).abs().argmax())      # (a ray whose gradient is not zero)
        alive[r, int(torch.nonzero(~alive[r])[0])] = True
    col = lambda x: _bcast(A, x, 128)      # noqa: E731
    row = (lambda o: EV(w2.v[o][None].expand(R, -1))) if A.ref else (lambda o: w2[o][None].expand(R, -1))
    d_w2 = [A.sum_any(A.mul(col(gpre[o]), hid)) for o in range(3)]
    d_b2 = [A.sum_any(gpre[o]) for o in range(3)]
    ghid = A.seq_sum([A.mul(row(o), col(gpre[o])) for o in range(3)], first=A.full(hid, 0.0))
    ghid = A.where(alive, ghid, A.full(hid, 0.0))
    d_b1 = A.sum_any(ghid)
    if A.ref:
        t = EV(ghid.v[:, :, None] * enc27.v[:, None, :], ghid.e[:, :, None] * enc27.v.abs()[:, None, :])
        t = Ref._r(t.v, t.e)
    else:
        t = ghid[:, :, None] * enc27[:, None, :]
    d_w1 = A.sum_any(t)
    return dict(w1=d_w1, b1=d_b1, w2=A.stack(d_w2, 0), b2=A.stack(d_b2, 0))
