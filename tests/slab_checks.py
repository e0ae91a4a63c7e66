"""Per-kernel references for what a training call leaves in its workspace: every chain / GEMM kernel is held to an fp64 evaluation of ITS
OWN operation on the exact bits it read (the saved operands decoded by tests/slab_restated.py), not to an end-to-end model.

Plain torch in float64 on whatever device the tensors are on.  Every check returns a list of `Worst`: per tensor the element with the
largest |got - ref| / bound, with its row and sample; ratio <= 1 passes.  No element is skipped or masked out; a non-finite value has
ratio inf.

Notation of the bounds (all derived from the formats, none measured):
  u32 = 2^-24 (fp32 unit roundoff), gamma(n) = n u32 / (1 - n u32): a sum of n fp32-rounded operations in ANY order is within
  gamma(n) x S of the exact sum, S = sum of the absolute values of the terms (products of two bf16 numbers are exact in fp32);
  2^-8 |v| = one round-to-nearest bf16 rounding (8 significant bits);
  Wb = the operand the kernel multiplies by: the bf16 rounding of the fp32 master weight in bf16 mode, the master weight in fp32 mode.
"""
import math

import torch

import slab_restated as sr

U32 = 2.0 ** -24
BF = 2.0 ** -8
F64 = torch.float64


def gamma(n):
    return n * U32 / (1.0 - n * U32)


class Worst:
    def __init__(self, name, row, sample, ratio, got, ref, bound):
        self.name, self.row, self.sample, self.ratio, self.got, self.ref, self.bound = name, row, sample, ratio, got, ref, bound

    @property
    def ok(self):
        return self.ratio <= 1.0

    def __repr__(self):
        return (f"{self.name}[row {self.row}, sample {self.sample}]: got {self.got!r} ref {self.ref!r} |diff| {abs(self.got - self.ref):.3e} "
                f"bound {self.bound:.3e} ratio {self.ratio:.3g}")


def compare(name, got, ref, bound, row0=0, cols=None):
    """Worst |got - ref| / bound over a [rows, samples] tensor.  bound == 0 demands equality; a non-finite `got` is ratio inf.
    cols: the sample index of every column (default: the column index)."""
    got, ref, bound = got.to(F64), ref.to(F64), bound.to(F64)
    if got.dim() == 1:
        got, ref, bound = got[None], ref[None], bound[None]
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    if got.numel() == 0:
        return Worst(name, row0, -1, 0.0, 0.0, 0.0, 0.0)
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, math.inf))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    k = int(torch.argmax(ratio))
    r, c = divmod(k, got.shape[1])
    return Worst(name, row0 + r, c if cols is None else int(cols[c]), float(ratio[r, c]), float(got[r, c]), float(ref[r, c]), float(bound[r, c]))


# ------------------------------------------------------------------------------------------------------------ parameters
TRUNK = "base_mlp.hidden_layers.%d"
SIG, BOT = "sigma_layer.output_layer", "bottleneck_layer.output_layer"
A1, A2 = "albedo_mlp.hidden_layers.0", "albedo_mlp.output_layer"
TR = "transient_mlp.hidden_layers.%d"
TSC, TBE, EMB = "transient_scalar.output_layer", "transient_beta.output_layer", "transient_encoder.weight"


class Params:
    """The fp32 master weights (views of the flat buffer the kernels were packed from) and the operands made of them."""

    def __init__(self, tensors, precision):
        self.t, self.precision, self.bf16 = tensors, precision, precision == "bf16"
        self._fold = None

    @classmethod
    def from_flat(cls, flat, layout, precision):
        """layout: [(name, offset, rows, cols)] (eonerf_param_info)."""
        return cls({name: flat[off:off + r * c].view(r, c) for name, off, r, c in layout}, precision)

    @classmethod
    def from_state_dict(cls, sd, precision):
        return cls({k: (v.float().view(1, -1) if v.dim() == 1 else v.float()) for k, v in sd.items() if v.is_floating_point()}, precision)

    def w(self, name):
        """fp32 master weight as float64 (biases: 1-D)."""
        v = self.t[name].to(F64)
        return v.reshape(-1) if name.endswith(".bias") else v

    def op(self, name):
        """Wb as float64."""
        v = self.t[name]
        return (v.to(torch.bfloat16) if self.bf16 else v).to(F64)

    def fold(self):
        """The heads' first layers folded with the identity-activation bottleneck layer (csrc/eonerf_pack.h), as k_fold forms them
        (csrc/eonerf_ctx.hip): W_f[o][i] = sum_k [W_A1; W_T1[:, :256]][o][k] W_bott[k][i] in fp32 through FOUR interleaved fmaf chains
        (k & 3), combined as (a0 + a1) + (a2 + a3); the bias likewise, plus [b_A1; b_T1].  The chains are written with explicit fmaf in
        a fixed order, so the reference follows them step by step: a x b is exact in float64 (48 bits), each step is rounded to fp32.

        Correction of the derivation the test was specified with.  It proposed an fp64 product and called an entry AMBIGUOUS when it
        lies within gamma(257) S_fold of a bf16 rounding boundary, with fewer than 1 % of the matrix allowed to be.  Measured on the
        CPU for seeds 7, 1, 2, 3, that criterion marks 20.3 / 20.3 / 20.1 / 20.2 % of the entries: gamma(257) S_fold is 1.5e-5 x 13 |w|
        against a rounding interval of 2^-8 |w| -- no seed can stay under the cap.  Following k_fold's own operation order removes the
        summation error from the comparison; what is left is the double rounding of the emulation itself (the float64 sum a b + c,
        then fp32: a slip of one fp32 ulp of an accumulator, |acc| <= S_fold, when the float64 sum falls within 2^-53 of an fp32
        boundary: 2 u32 |acc| <= 2 u32 S_fold per slip).  An entry is ambiguous when its emulated value lies within 4 u32 S_fold of a bf16
        boundary (room for two slips in one entry; about 0.03 slips are expected in the whole matrix); the cap of 1 % is asserted on that
        set (measured: 0.61 / 0.63 / 0.68 % for seeds 7 / 1 / 2).  Returns a dict: W, b (float64 values of the fp32 fold), op (Wb), S,
        amb_ulp (bf16 ulp at the ambiguous entries, 0 elsewhere), amb_frac, b_slack."""
        if self._fold is not None:
            return self._fold
        L = torch.cat([self.t[A1 + ".weight"], self.t[TR % 0 + ".weight"][:, :256]]).to(F64)      # [o 256][k 256]
        R = self.t[BOT + ".weight"].to(F64)                                                           # [k 256][i 256]
        bb = self.t[BOT + ".bias"].to(F64).reshape(-1)
        r32 = lambda x: x.float().to(F64)      # noqa: E731
        acc = [torch.zeros(256, 256, dtype=F64, device=L.device) for _ in range(4)]
        b4 = [torch.zeros(256, dtype=F64, device=L.device) for _ in range(4)]
        for k in range(256):
            acc[k & 3] = r32(L[:, k:k + 1] * R[k:k + 1, :] + acc[k & 3])
            b4[k & 3] = r32(L[:, k] * bb[k] + b4[k & 3])
        W = r32(r32(acc[0] + acc[1]) + r32(acc[2] + acc[3]))
        b1 = torch.cat([self.t[A1 + ".bias"].reshape(-1), self.t[TR % 0 + ".bias"].reshape(-1)]).to(F64)
        b = r32(r32(r32(b4[0] + b4[1]) + r32(b4[2] + b4[3])) + b1)
        S = L.abs() @ R.abs()
        slack = 4 * U32 * S
        amb_ulp = torch.zeros_like(W)
        if self.bf16:
            q = W.float().to(torch.bfloat16).to(F64)
            ulp = torch.exp2(torch.floor(torch.log2(W.abs().clamp_min(1e-300))) - 7)
            amb = (ulp / 2 - (W - q).abs()) <= slack
            amb_ulp = torch.where(amb, ulp, amb_ulp)
            op = q
        else:
            amb = torch.zeros_like(W, dtype=torch.bool)
            op = W
        self._fold = dict(W=W, b=b, op=op, S=S, amb_ulp=amb_ulp, amb_frac=float(amb.double().mean()),
                          w_slack=torch.zeros_like(S) if self.bf16 else slack, b_slack=4 * U32 * (L.abs() @ bb.abs() + b1.abs()))
        return self._fold


# ------------------------------------------------------------------------------------------------------------ one pass' buffers
class Pass:
    """What one MLP pass left in the workspace, decoded on demand as float64 [rows, n] (the live samples only: rows beyond n_pts are
    not asserted on).  off: member name -> byte offset (eonerf_workspace_layout); unit_blocks: first rows of the 256-row blocks of
    the gradient slab that lie in unit order (dY_0 / dY_5 behind the pipelined backward)."""

    def __init__(self, ws, off, p_cap, n, precision, full, unit_blocks=()):
        self.ws, self.off, self.p_cap, self.n, self.precision, self.full = ws, off, int(p_cap), int(n), precision, full
        self.bf16 = precision == "bf16"
        self.nt = self.p_cap // sr.seg_samples(precision)
        self.unit_blocks = set(unit_blocks)
        self._cache = {}

    def _block(self, which, blk):
        key = (which, blk[0])
        if key not in self._cache:
            if which == "grd" and blk[0] in self.unit_blocks:
                d = sr.decode_unit_block(self.ws, self.off["grd"], blk[0], self.nt)
            else:
                d = sr.decode_block(self.ws, self.off[which], blk[0], blk[1], self.nt, self.precision)
            self._cache[key] = d[:, :self.n].to(F64)
        return self._cache[key]

    def act(self, row, rows):
        blk = sr.act_block(row)
        assert row + rows <= blk[0] + blk[1]
        return self._block("act", blk)[row - blk[0]:row - blk[0] + rows]

    def grd(self, row, rows):
        blk = sr.grd_block(row)
        assert row + rows <= blk[0] + blk[1]
        return self._block("grd", blk)[row - blk[0]:row - blk[0] + rows]

    def f32(self, name, rows=1):
        return sr.soa(self.ws, self.off[name], rows, self.p_cap)[:, :self.n].to(F64)

    def simg(self):
        return sr.soa(self.ws, self.off["simg"], 1, self.p_cap, torch.int32)[0, :self.n].long()

    def g_emb(self):
        return self.ws[self.off["g_emb"]:self.off["g_emb"] + 16 * self.p_cap].view(torch.float32).view(self.p_cap, 4)[:self.n].to(F64).t()

    def xyz(self):
        return torch.cat([self.f32("px"), self.f32("py"), self.f32("pz")])

    def drop(self):
        self._cache.clear()


def _C():
    return sr.K()


def enc_ref(ps):
    """[63, n]: the saved encoding rows in the reference's column order (the operand of layer 0 and of the skip columns of layer 5)."""
    e = ps.act(_C()["ACT_ROW_ENC"], 64)
    cols = sr.enc_col_of_row(ps.precision)
    out = torch.empty(63, ps.n, dtype=F64, device=e.device)
    for r, c in enumerate(cols):
        if c >= 0:
            out[c] = e[r]
    return out


def _enc_dim_scale():
    """Per reference column: (dimension, k or -1 for the raw coordinates, phase flag)."""
    out = [(d, -1, 0) for d in range(3)]
    for half in range(2):
        for j in range(30):
            out.append((j % 3, j // 3, half))
    return out


PI_2_F = 1.57079637050628662109375      # fp32(0.5 * pi): radiance_fields/mlp.py:203, EO_PI_2_F


# ------------------------------------------------------------------------------------------------------------ encoding
def check_encoding(ps):
    """Encoding rows (encode_position, csrc/eonerf_mlp_fwd.hip): the saved value of a sine slot is the stored rounding of
    sin(fl(2^k x + phase)).  |got - sin(2^k x + phase)| <= 2^-8 |v| + 2^-14: one bf16 rounding (dropped in fp32 mode), half an fp32 ulp of
    an argument of up to 512 + pi/2 (2^-15; |sin'| <= 1) and as much again for the sine itself.  The raw coordinates and the pad row are
    held to the same bound (their argument term is slack; the pad row's reference is 0 with bound 0)."""
    xyz = ps.xyz()
    e = ps.act(_C()["ACT_ROW_ENC"], 64)
    ref = torch.zeros_like(e)
    bound = torch.zeros_like(e)
    for r, c in enumerate(sr.enc_col_of_row(ps.precision)):
        if c < 0:
            continue
        d, k, half = _enc_dim_scale()[c]
        ref[r] = xyz[d] if k < 0 else torch.sin(xyz[d] * float(1 << k) + (PI_2_F if half else 0.0))
        bound[r] = (BF * ref[r].abs() if ps.bf16 else 0.0) + 2.0 ** -14
    return [compare("encoding", e, ref, bound)]


# ------------------------------------------------------------------------------------------------------------ forward
def _lin(W, X, b=None):
    v, S = W @ X, W.abs() @ X.abs()
    if b is not None:
        v, S = v + b[:, None], S + b.abs()[:, None]
    return v, S


def _acc_bound(S, K, bf16):
    """fp32 accumulation of K products (+ the bias the accumulator starts from): gamma(K + 1) S; fp32 mode: the products themselves are
    rounded as well: gamma(K + 2) S."""
    return gamma(K + 1 if bf16 else K + 2) * S


def _relu_layer(name, ps, W, X, b, out_row, extra=None):
    v, S = _lin(W, X, b)
    ref = v.clamp_min(0)
    bound = (BF * ref if ps.bf16 else 0.0) + _acc_bound(S, W.shape[1], ps.bf16)
    if extra is not None:
        bound = bound + extra
    return compare(name, ps.act(out_row, W.shape[0]), ref, bound, out_row)


def _head_out(name, ps, W, X, b, got, kind):
    """Scalar head outputs: the pre-activation bound through the activation's Lipschitz constant (softplus 1, sigmoid 1/4) plus 8 u32
    relative for the device's expf / log1pf and the arithmetic around them (the ROCm documentation on this machine does not state ulp
    bounds for the OCML single-precision functions; 8 ulp is kept as specified)."""
    v, S = _lin(W, X, b)
    pre = _acc_bound(S, W.shape[1], ps.bf16)
    if kind == "softplus":
        ref, lip = torch.where(v > 20, v, torch.log1p(torch.exp(v.clamp_max(20)))), 1.0
    else:
        ref, lip = torch.sigmoid(v), 0.25
    return compare(name, got, ref, lip * pre + 8 * U32 * ref.abs())


def check_forward(ps, pr):
    """Forward chain (k_mlp_fwd), layer by layer, each from the SAVED input of that layer and Wb:  v = b + sum_k Wb X,
    |got - relu(v)| <= 2^-8 |relu(v)| + gamma(K + 1) S  (fp32 mode: gamma(K + 2) S only).  ReLU is 1-Lipschitz, so the accumulation
    bound passes through it.  The folded layers [A1-fold; T1-fold + embedding] add, per row, ulp x |X| of the entries whose bf16
    rounding is ambiguous (Params.fold), 4 u32 S_fold |X| in fp32 mode and the slack of the folded bias."""
    c = _C()
    out = []
    E = enc_ref(ps)
    x1 = c["ACT_ROW_X1"]
    X = lambda l: ps.act(x1 + 256 * (l - 1), 256)      # noqa: E731  X_l = output of trunk layer l - 1
    for l in range(8):
        W, b = pr.op(TRUNK % l + ".weight"), pr.w(TRUNK % l + ".bias")
        inp = E if l == 0 else (torch.cat([X(5), E]) if l == 5 else X(l))
        out.append(_relu_layer(f"X_{l + 1}", ps, W, inp, b, x1 + 256 * l))
    X8 = X(8)
    out.append(_head_out("sigma", ps, pr.op(SIG + ".weight"), X8, pr.w(SIG + ".bias"), ps.f32("sigma"), "softplus"))
    if not ps.full:
        return out
    f = pr.fold()
    aX8 = X8.abs()
    extra = (f["amb_ulp"] + f["w_slack"]) @ aX8 + f["b_slack"][:, None]
    out.append(_relu_layer("A1", ps, f["op"][:128], X8, f["b"][:128], c["ACT_ROW_A1"], extra[:128]))
    A1h = ps.act(c["ACT_ROW_A1"], 128)
    out.append(_head_out("albedo", ps, pr.op(A2 + ".weight"), A1h, pr.w(A2 + ".bias"), ps.f32("albedo", 3), "sigmoid"))
    # embedding rows: the operand of the transient head's first layer (rows 0..3 of its block; rows 4..7 belong to the other lane half: 0)
    emb = pr.t[EMB].to(F64)[ps.simg()].t()
    emb_got = ps.act(c["ACT_ROW_EMB"], 8)
    emb_ref = torch.cat([emb, torch.zeros_like(emb)])
    out.append(compare("embedding rows", emb_got, emb_ref, BF * emb_ref.abs() if ps.bf16 else torch.zeros_like(emb_ref)))
    t1 = c["ACT_ROW_T1"]
    W = torch.cat([f["op"][128:], pr.op(TR % 0 + ".weight")[:, 256:260]], 1)
    out.append(_relu_layer("T1", ps, W, torch.cat([X8, emb_got[:4]]), f["b"][128:], t1, extra[128:]))
    for l in range(1, 4):
        out.append(_relu_layer(f"T{l + 1}", ps, pr.op(TR % l + ".weight"), ps.act(t1 + 128 * (l - 1), 128), pr.w(TR % l + ".bias"), t1 + 128 * l))
    T4 = ps.act(t1 + 384, 128)
    out.append(_head_out("ts", ps, pr.op(TSC + ".weight"), T4, pr.w(TSC + ".bias"), ps.f32("ts"), "sigmoid"))
    out.append(_head_out("tb", ps, pr.op(TBE + ".weight"), T4, pr.w(TBE + ".bias"), ps.f32("tb"), "softplus"))
    return out


# ------------------------------------------------------------------------------------------------------------ backward chain
def _head_rows(ps):
    """Reference and bound of the heads' pre-activation gradients (k_mlp_bwd "output heads"), from the upstream gradients and the SAVED
    forward outputs, all fp32 on the device:
      softplus: g (1 - expf(-s)): t = expf(-s) within 8 u32 t, the difference and the product one rounding each:
                |err| <= |g| u32 (8 t + 3 |1 - t|);
      sigmoid : g a (1 - a): three roundings: 4 u32 |ref|;
    plus the bf16 rounding of the stored row, 2^-8 |ref| (not in fp32 mode)."""
    def softplus(g, s):
        t = torch.exp(-s)
        ref = g * (1 - t)
        return ref, g.abs() * U32 * (8 * t + 3 * (1 - t).abs()) + (BF * ref.abs() if ps.bf16 else 0.0)

    def sigmoid(g, a):
        ref = g * a * (1 - a)
        return ref, (4 * U32 + (BF if ps.bf16 else 0.0)) * ref.abs()
    rows = {"sig": softplus(ps.f32("g_sigma"), ps.f32("sigma"))}
    if ps.full:
        rows["alb"] = sigmoid(ps.f32("g_albedo", 3), ps.f32("albedo", 3))
        ts, tb = sigmoid(ps.f32("g_ts"), ps.f32("ts")), softplus(ps.f32("g_tb"), ps.f32("tb"))
        rows["t5"] = (torch.cat([ts[0], tb[0]]), torch.cat([ts[1], tb[1]]))
    return rows


def _bwd_layer(name, ps, W, dY, X_mask, got, row0=0, extra=None, rounded=True):
    """dX = sum_f Wb[f, .] dY[f], masked by ReLU' = [saved activation > 0] (the 1-bit masks the chain reads hold exactly that bit; the
    pipeline's stages derive it from the saved activations themselves):  |got - ref| <= 2^-8 |ref| + gamma(K + 1) S where the mask is
    set (fp32 mode gamma(K + 2) S), and got == 0 exactly where it is not -- a wrong mask bit shows as a full-size error."""
    v, S = W.t() @ dY, W.t().abs() @ dY.abs()
    bound = _acc_bound(S, W.shape[0], ps.bf16)
    if extra is not None:
        bound = bound + extra
    if X_mask is not None:
        m = (X_mask > 0).to(F64)
        v, bound = v * m, bound * m
    if rounded and ps.bf16:
        bound = bound + BF * v.abs()
    return compare(name, got, v, bound, row0)


def check_backward(ps, pr, transient=True, dy7=None, stop_at_dy7=False):
    """Backward chain (k_mlp_bwd), layer by layer, each from the SAVED dY of the layer above (the kernel's own operand: it hands on the
    rounded values it stores).  dy7: dY_7 decoded from the pipeline's input buffer (unit order) instead of the gradient slab;
    stop_at_dy7: the heads chain of the pipelined path ends there."""
    c = _C()
    out = []
    hr = _head_rows(ps)
    dsig = ps.grd(c["GRD_ROW_SIG"], 1)
    out.append(compare("d sigma_pre", dsig, *hr["sig"], row0=c["GRD_ROW_SIG"]))
    x1 = c["ACT_ROW_X1"]
    X = lambda l: ps.act(x1 + 256 * (l - 1), 256)      # noqa: E731
    y0 = c["GRD_ROW_Y0"]
    dY7 = ps.grd(y0 + 7 * 256, 256) if dy7 is None else dy7
    wsig = pr.op(SIG + ".weight")
    if ps.full:
        dalb = ps.grd(c["GRD_ROW_A2"], 3)
        out.append(compare("d albedo_pre", dalb, *hr["alb"], row0=c["GRD_ROW_A2"]))
        t1a, t1g = c["ACT_ROW_T1"], c["GRD_ROW_T1"]
        dA1 = ps.grd(c["GRD_ROW_A1"], 128)
        out.append(_bwd_layer("dY_A1", ps, pr.op(A2 + ".weight"), dalb, ps.act(c["ACT_ROW_A1"], 128), dA1, c["GRD_ROW_A1"]))
        srcs, Ws = [dA1], [pr.fold()["op"][:128]]
        amb = [pr.fold()["amb_ulp"][:128] + pr.fold()["w_slack"][:128]]
        if transient:
            dt5 = ps.grd(c["GRD_ROW_T5"], 2)
            out.append(compare("d {ts, tb}_pre", dt5, *hr["t5"], row0=c["GRD_ROW_T5"]))
            W = torch.cat([pr.op(TSC + ".weight"), pr.op(TBE + ".weight")])
            dT = ps.grd(t1g + 384, 128)
            out.append(_bwd_layer("dY_T4", ps, W, dt5, ps.act(t1a + 384, 128), dT, t1g + 384))
            for l in (3, 2, 1):
                nxt = ps.grd(t1g + 128 * (l - 1), 128)
                out.append(_bwd_layer(f"dY_T{l}", ps, pr.op(TR % l + ".weight"), dT, ps.act(t1a + 128 * (l - 1), 128), nxt, t1g + 128 * (l - 1)))
                dT = nxt
            out.append(_bwd_layer("g_emb", ps, pr.op(TR % 0 + ".weight")[:, 256:260], dT, None, ps.g_emb(), rounded=False))
            srcs.append(dT); Ws.append(pr.fold()["op"][128:]); amb.append(pr.fold()["amb_ulp"][128:] + pr.fold()["w_slack"][128:])
        srcs.append(dsig); Ws.append(wsig); amb.append(torch.zeros_like(wsig))
        src, W, A = torch.cat(srcs), torch.cat(Ws), torch.cat(amb)
        out.append(_bwd_layer("dY_7", ps, W, src, X(8), dY7, y0 + 7 * 256, extra=A.t() @ src.abs()))
    else:
        out.append(_bwd_layer("dY_7", ps, wsig, dsig, X(8), dY7, y0 + 7 * 256))
    if stop_at_dy7:
        return out
    dY = dY7
    for l in range(6, -1, -1):      # dY_l from dY_{l+1} through W_{l+1} (its 256 trunk columns)
        nxt = ps.grd(y0 + 256 * l, 256)
        out.append(_bwd_layer(f"dY_{l}", ps, pr.op(TRUNK % (l + 1) + ".weight")[:, :256], dY, X(l + 1), nxt, y0 + 256 * l))
        dY = nxt
    return out


def check_input_grad(ps, pr, name="g_pos"):
    """g_pos (the chain's input-gradient tail; eonerf_ig_tail.hip / eonerf_enc_pair.hip on the pipelined path):
      d enc[c] = sum_o Wb_5[o, 256 + c] dY_5[o] + Wb_0[o, c] dY_0[o]      (512 products, fp32),
      g_pos[d] = sum over the columns of dimension d of d enc[c] x dv[c],  dv = 1 (raw coordinate) or 2^k cos(2^k x + phase).
    Bound: gamma(512 + 34) S for the two accumulations, the 21-term sum and its products, plus per sine slot the effect of the fp32
    argument rounding on dv: |d enc[c]| x 2^-15 x 2^k (half an ulp of an argument up to 512 + pi/2, |cos'| <= 1, scaled by 2^k)."""
    c = _C()
    xyz = ps.xyz()
    dY5, dY0 = ps.grd(c["GRD_ROW_Y0"] + 5 * 256, 256), ps.grd(c["GRD_ROW_Y0"], 256)
    W5, W0 = pr.op(TRUNK % 5 + ".weight")[:, 256:], pr.op(TRUNK % 0 + ".weight")
    denc = W5.t() @ dY5 + W0.t() @ dY0
    Sd = W5.t().abs() @ dY5.abs() + W0.t().abs() @ dY0.abs()
    ref = torch.zeros(3, ps.n, dtype=F64, device=xyz.device)
    bound = torch.zeros_like(ref)
    for col, (d, k, half) in enumerate(_enc_dim_scale()):
        if k < 0:
            dv, arg_err = torch.ones_like(xyz[d]), 0.0
        else:
            dv, arg_err = float(1 << k) * torch.cos(xyz[d] * float(1 << k) + (PI_2_F if half else 0.0)), 2.0 ** -15 * float(1 << k)
        ref[d] += denc[col] * dv
        bound[d] += gamma(512 + 34) * Sd[col] * dv.abs() + denc[col].abs() * arg_err
    return [compare(name, ps.f32("g_pos", 3), ref, bound)]


# ------------------------------------------------------------------------------------------------------------ weight gradients
def _nz(dY):
    return torch.nonzero((dY != 0).any(0)).flatten()


def check_weight_gradients(passes, pr, grads, m_bott=None, transient=True, trunk=range(1, 8), enc=True, heads=True, tag=""):
    """Every job of wgrad_plan (csrc/eonerf_wgrad_plan.h) whose destination received the contributions of `passes` (one pass, or the
    camera and the shadow pass of a render step: the products of both are summed, the bounds add).
    One job of the weight-gradient GEMM (k_wgrad): dW = sum_{p < n_pts} dY[:, p] X[:, p]^T in float64 from the decoded operands.
    Elementwise |got - ref| <= gamma(n_nz + 257) S_ij: n_nz = samples with a non-zero dY row (the others add exact zeros), 257 for the
    combination of up to 256 slice partials (atomic adds in any order); fp32 mode one more for the rounded product.  The bias gradient
    (the ones column of the same product) is held to the same bound.  Samples with an all-zero dY row are left out of the float64
    product: they contribute exactly nothing to either side.  grads: name -> [rows, cols] view of
    d_flat, zeroed before the call.  m_bott: the read-back bottleneck factors [256][256] M | [256] db (full pass only).
    trunk (the layers among 1..7) / enc / heads select the job groups: behind the pipelined backward only dY_5 and dY_0 exist."""
    c = _C()
    out = []
    y0, x1 = c["GRD_ROW_Y0"], c["ACT_ROW_X1"]

    def both(name, rows_of, got_w, got_b=None, only_full=False):
        ps_list = [p for p in passes if p.full] if only_full else passes
        res = None
        for p in ps_list:
            dY, X = rows_of(p)
            idx = _nz(dY)
            d, x = dY[:, idx], X[:, idx]
            g = gamma(idx.numel() + 257 + (0 if p.bf16 else 1))
            part = [d @ x.t(), g * (d.abs() @ x.abs().t()), d.sum(1), g * d.abs().sum(1)]
            res = part if res is None else [a + b for a, b in zip(res, part)]
        out.append(compare("dW " + name + tag, got_w, res[0], res[1]))
        if got_b is not None:
            out.append(compare("db " + name + tag, got_b.reshape(1, -1), res[2][None], res[3][None]))

    cols = sr.enc_col_of_row(passes[0].precision)
    keep = [r for r, k in enumerate(cols) if k >= 0]
    order = torch.tensor([cols[r] for r in keep])

    def enc_rows(p):      # the 64 encoding rows, permuted to the reference's 63 columns (the GEMM's col_map drops the pad slot)
        e = p.act(c["ACT_ROW_ENC"], 64)
        o = torch.empty(63, p.n, dtype=F64, device=e.device)
        o[order.to(e.device)] = e[torch.tensor(keep, device=e.device)]
        return o
    if enc:
        both("0", lambda p: (p.grd(y0, 256), enc_rows(p)), grads[TRUNK % 0 + ".weight"], grads[TRUNK % 0 + ".bias"])
        both("5[:, 256:]", lambda p: (p.grd(y0 + 5 * 256, 256), enc_rows(p)), grads[TRUNK % 5 + ".weight"][:, 256:])
    if trunk:
        for l in trunk:
            both(f"{l}", lambda p, l=l: (p.grd(y0 + 256 * l, 256), p.act(x1 + 256 * (l - 1), 256)), grads[TRUNK % l + ".weight"][:, :256], grads[TRUNK % l + ".bias"])
    if not heads:
        return out
    X8 = lambda p: p.act(x1 + 256 * 7, 256)      # noqa: E731
    both("sigma", lambda p: (p.grd(c["GRD_ROW_SIG"], 1), X8(p)), grads[SIG + ".weight"], grads[SIG + ".bias"])
    full = [p for p in passes if p.full]
    if not full:
        return out
    ps = full[0]
    both("A2", lambda p: (p.grd(c["GRD_ROW_A2"], 3), p.act(c["ACT_ROW_A1"], 128)), grads[A2 + ".weight"], grads[A2 + ".bias"], only_full=True)
    t1a, t1g = c["ACT_ROW_T1"], c["GRD_ROW_T1"]
    if transient:
        both("T1[:, 256:260]", lambda p: (p.grd(t1g, 128), p.act(c["ACT_ROW_EMB"], 4)), grads[TR % 0 + ".weight"][:, 256:260], only_full=True)
        for l in range(1, 4):
            both(f"T{l + 1}", lambda p, l=l: (p.grd(t1g + 128 * l, 128), p.act(t1a + 128 * (l - 1), 128)), grads[TR % l + ".weight"], grads[TR % l + ".bias"], only_full=True)
        both("ts", lambda p: (p.grd(c["GRD_ROW_T5"], 1), p.act(t1a + 384, 128)), grads[TSC + ".weight"], grads[TSC + ".bias"], only_full=True)
        both("tb", lambda p: (p.grd(c["GRD_ROW_T5"] + 1, 1), p.act(t1a + 384, 128)), grads[TBE + ".weight"], grads[TBE + ".bias"], only_full=True)
        # embedding table: the scatter of g_emb by the samples' image index (fp32 atomic / per-image sums of count terms in any order)
        ge, im = ps.g_emb(), ps.simg()
        n_img = grads[EMB].shape[0]
        ref = torch.zeros(n_img, 4, dtype=F64, device=ge.device).index_add_(0, im, ge.t())
        S = torch.zeros_like(ref).index_add_(0, im, ge.t().abs())
        cnt = torch.bincount(im, minlength=n_img).to(F64)
        out.append(compare("d embedding table" + tag, grads[EMB], ref, (cnt + 1)[:, None] * U32 / (1 - (cnt + 1)[:, None] * U32) * S))
    # ---- bottleneck factors and the three weight gradients that follow from them (BottWgradArgs, csrc/eonerf_rays.h) ----
    rows = 256 if transient else 128
    dAT = ps.grd(c["GRD_ROW_A1"], rows)
    idx = _nz(dAT)
    d, x = dAT[:, idx], X8(ps)[:, idx]
    g = gamma(idx.numel() + 257 + (0 if ps.bf16 else 1))
    M, EM, db, Edb = d @ x.t(), g * (d.abs() @ x.abs().t()), d.sum(1), g * d.abs().sum(1)
    if m_bott is not None:
        got = m_bott.to(F64)
        out.append(compare("bottleneck factors" + tag, got[:rows * 256].view(rows, 256), M, EM))
        out.append(compare("bottleneck factor biases" + tag, got[65536:65536 + rows][None], db[None], Edb[None]))
    # dW_bott = W_A1^T M_a + W_T1'^T M_t, db_bott = W_A1^T db_A1 + W_T1'^T db_T1; dW_A1 = M_a W_bott^T + db_A1 (x) b_bott, dW_T1[:, :256]
    # likewise; db_A1 / db_T1 are the factor biases themselves.  fp32 products of the fp32 master weights (bott_wgrad_body): the factor
    # bound propagated through the product in absolute value, plus gamma(257) of the product's own absolute sum.
    WAT = torch.cat([pr.w(A1 + ".weight"), pr.w(TR % 0 + ".weight")[:, :256]])[:rows]
    Wb_, bb = pr.w(BOT + ".weight"), pr.w(BOT + ".bias")
    g257 = gamma(257)
    out.append(compare("dW bottleneck" + tag, grads[BOT + ".weight"], WAT.t() @ M, WAT.t().abs() @ EM + g257 * (WAT.t().abs() @ M.abs())))
    out.append(compare("db bottleneck" + tag, grads[BOT + ".bias"].reshape(1, -1), (WAT.t() @ db)[None], (WAT.t().abs() @ Edb + g257 * (WAT.t().abs() @ db.abs()))[None]))
    ref = M @ Wb_.t() + db[:, None] * bb[None]
    bnd = EM @ Wb_.t().abs() + Edb[:, None] * bb.abs()[None] + g257 * (M.abs() @ Wb_.t().abs() + db.abs()[:, None] * bb.abs()[None])
    out.append(compare("dW A1" + tag, grads[A1 + ".weight"], ref[:128], bnd[:128]))
    out.append(compare("db A1" + tag, grads[A1 + ".bias"].reshape(1, -1), db[None, :128], Edb[None, :128]))
    if transient:
        out.append(compare("dW T1[:, :256]" + tag, grads[TR % 0 + ".weight"][:, :256], ref[128:], bnd[128:]))
        out.append(compare("db T1" + tag, grads[TR % 0 + ".bias"].reshape(1, -1), db[None, 128:], Edb[None, 128:]))
    return out


def check_field_pair(ps, pr, grads, m_bott):
    """Everything eonerf_field_forward_train + eonerf_field_backward leave behind (chain + GEMM path)."""
    out = check_encoding(ps) + check_forward(ps, pr) + check_backward(ps, pr) + check_input_grad(ps, pr)
    return out + check_weight_gradients([ps], pr, grads, m_bott if ps.full else None)


def failures(results):
    return [w for w in results if not w.ok]
