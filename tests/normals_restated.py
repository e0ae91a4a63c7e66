"""The rules of include/eonerf_normals.h restated in numpy fp64: the density chain carried as four planes per point (value, d/dx, d/dy,
d/dz) and the per-ray compositing of the unit gradients.  Nothing here re-implements a kernel: no lanes, no tiles, no packed weights.

    sd       a state dict of the field as {name: array} (the trunk base_mlp.hidden_layers.0..7 and sigma_layer.output_layer are read)
    x        [n, 3] points
The encoding is the reference's: [x, sin(2^k x) frequency-major, sin(2^k x + pi/2)], L = 10; layer 5 reads [h, encoding].
"""
import numpy as np

POS_L = 10
N_TRUNK = 8
SKIP_AFTER = 4
HALF_PI32 = float(np.float32(0.5 * np.pi))      # the fp32 constant both the reference's fp32 run and the device add


def encode_planes(x, half_pi=0.5 * np.pi):
    """[n, 3] -> [n, 4, 63]: plane 0 the encoding, plane 1 + j its derivative along coordinate j.  The raw slot of a coordinate holds
    1 in its own plane; slot sin(2^k c + off) holds 2^k sin(2^k c + off + pi/2) in the plane of coordinate c; 0 elsewhere."""
    x = np.asarray(x, dtype=np.float64)
    E = np.zeros((x.shape[0], 4, 3 + 6 * POS_L))
    E[:, 0, 0:3] = x
    for j in range(3):
        E[:, 1 + j, j] = 1.0
    for k in range(POS_L):
        for d in range(3):
            col = 3 + 3 * k + d
            arg = x[:, d] * 2.0 ** k
            for off, c in ((0.0, col), (half_pi, col + 3 * POS_L)):
                E[:, 0, c] = np.sin(arg + off)
                E[:, 1 + d, c] = 2.0 ** k * np.sin(arg + off + 0.5 * np.pi)
    return E


def _f64(sd, name):
    a = sd[name]
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)


def density_planes(sd, x, half_pi=0.5 * np.pi):
    """-> (sigma [n], grad [n, 3], min_pre [n]): the four-plane chain.  Every trunk layer: the bias goes to plane 0 only; planes 1..3
    keep their value where plane 0's pre-activation is > 0 and get 0 elsewhere.  Head: sigma = softplus(raw) (threshold 20),
    d sigma = raw' / (1 + exp(-raw)).  min_pre: the smallest |pre-activation| of plane 0 over the eight trunk layers -- the distance
    of the point from the nearest ReLU kink, where the gradient is discontinuous."""
    E = encode_planes(x, half_pi)
    H = E
    min_pre = np.full(E.shape[0], np.inf)
    for l in range(N_TRUNK):
        W, b = _f64(sd, f"base_mlp.hidden_layers.{l}.weight"), _f64(sd, f"base_mlp.hidden_layers.{l}.bias")
        Z = H @ W.T
        Z[:, 0, :] += b
        min_pre = np.minimum(min_pre, np.abs(Z[:, 0, :]).min(axis=1))
        H = np.where(Z[:, 0:1, :] > 0, Z, 0.0)
        if l == SKIP_AFTER:
            H = np.concatenate([H, E], axis=2)
    W, b = _f64(sd, "sigma_layer.output_layer.weight"), _f64(sd, "sigma_layer.output_layer.bias")
    raw = (H @ W.T)[:, :, 0]
    raw[:, 0] += b[0]
    r0 = raw[:, 0]
    with np.errstate(over="ignore"):
        sigma = np.where(r0 > 20.0, r0, np.log1p(np.exp(np.minimum(r0, 20.0))))
        grad = raw[:, 1:4] / (1.0 + np.exp(-r0))[:, None]
    return sigma, grad, min_pre


def kept(min_pre, margin=1e-5):
    """Points a gradient comparison may use: further than `margin` (in pre-activation units) from every ReLU kink."""
    return np.asarray(min_pre) > margin


def rel_stats(got, want):
    """(max over points of |got - want| / |want|, relative L2 over all points) of [n, 3] gradients."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.linalg.norm(got - want, axis=1)
    return float((err / np.linalg.norm(want, axis=1)).max()), float(np.sqrt((err ** 2).sum() / (want ** 2).sum()))


# ---- compositing -----------------------------------------------------------------------------------------------------------------
def ray_weights(sigma, delta):
    """w_k = exp(-E_k) (1 - exp(-sigma_k delta_k)), E the exclusive prefix sum of sigma * delta."""
    sd = np.asarray(sigma, dtype=np.float64) * np.asarray(delta, dtype=np.float64)
    E = np.concatenate([[0.0], np.cumsum(sd)[:-1]]) if sd.size else sd
    return np.exp(-E) * (1.0 - np.exp(-sd))


def unit_gradients(grad, axis_scale=(1.0, 1.0, 1.0)):
    """u_k = g_k / |g_k| with g_k = grad_k * axis_scale; 0 where |g_k| is 0 or not finite."""
    g = np.asarray(grad, dtype=np.float64).reshape(-1, 3) * np.asarray(axis_scale, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((g * g).sum(axis=1))
        ok = (length > 0) & np.isfinite(length)
        return np.where(ok[:, None], g / np.where(ok, length, 1.0)[:, None], 0.0)


def composite(sigma, delta, mid, grad, axis_scale=(1.0, 1.0, 1.0)):
    """One ray -> (depth, N [3], A): sum w mid, -sum w u, sum w.  A ray without samples gives zeros."""
    w = ray_weights(sigma, delta)
    if w.size == 0:
        return 0.0, np.zeros(3), 0.0
    u = unit_gradients(grad, axis_scale)
    return float((w * np.asarray(mid, dtype=np.float64)).sum()), -(w[:, None] * u).sum(axis=0), float(w.sum())


def last_delta(ts, te):
    """The forward's delta of one ray's samples (fp32): te - ts, the last one 1e10 - ts."""
    ts, te = np.asarray(ts, dtype=np.float32), np.asarray(te, dtype=np.float32)
    d = te - ts
    if d.size:
        d[-1] = np.float32(1e10) - ts[-1]
    return d
