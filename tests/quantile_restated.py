"""The quantile-depth rule of include/eonerf_quantile.h restated in numpy fp64 scalar loops over ONE ray's composited samples, and the
acceptance test a device value is held to.  Nothing here re-implements a kernel: no lanes, no scans, no rounds.

    ts, te   [n]   the sampler's interval ends (te of the last sample: the sampler's own value, not 1e10)
    sigma    [n]   the density per sample
    delta    [n]   the forward's delta: te - ts, the ray's last sample ends at 1e10
    L              -log1p(-q)
"""
import numpy as np

D_REL = 32 * 2.0 ** -24      # the roundings on any path of the prefix sums plus the rounds' carries (at most 24 at 255 samples, block 16) and sigma * delta
A_ABS = 16 * 2.0 ** -23      # the final subtract, divide and add; times max(1, |t|)


def L_of(q):
    """L_q = (float)(-log1p(-(double)q)) of the fp32 quantile q."""
    return np.float32(-np.log1p(-np.float64(np.float32(q))))


def last_delta(ts, te):
    """The forward's delta of one ray's samples (fp32): te - ts, the last one 1e10 - ts."""
    ts, te = np.asarray(ts, dtype=np.float32), np.asarray(te, dtype=np.float32)
    d = te - ts
    if d.size:
        d[-1] = np.float32(1e10) - ts[-1]
    return d


def t_q(ts, te, sigma, delta, L):
    n = len(ts)
    if n == 0:
        return 0.0
    L, E = float(L), 0.0
    for k in range(n):
        I = E + float(sigma[k]) * float(delta[k])
        if I >= L:                                   # the bracket: the first k with I_k >= L (then sigma_k > 0)
            return float(ts[k]) + min(max((L - E) / float(sigma[k]), 0.0), float(te[k]) - float(ts[k]))
        E = I
    return float(te[n - 1])                          # all density zero to the end


def od_front(sigma, delta):
    """E_{n-1}: the optical depth in front of the ray's last sample; 0 without samples."""
    E = 0.0
    for k in range(len(sigma) - 1):
        E += float(sigma[k]) * float(delta[k])
    return E


def expected_depth(ts, te, sigma, delta):
    """sum of exp(-E_k) (1 - exp(-sd_k)) mid_k."""
    E, d = 0.0, 0.0
    for k in range(len(ts)):
        sd = float(sigma[k]) * float(delta[k])
        d += np.exp(-E) * (1.0 - np.exp(-sd)) * 0.5 * (float(ts[k]) + float(te[k]))
        E += sd
    return float(d)


def bounds(ts, te, sigma, delta, L, d=D_REL):
    """(lo, hi) of the rule at L (1 - d) and L (1 + d): t_q is monotone in L."""
    return t_q(ts, te, sigma, delta, float(L) * (1.0 - d)), t_q(ts, te, sigma, delta, float(L) * (1.0 + d))


def accepts(t, ts, te, sigma, delta, L, d=D_REL, a=A_ABS):
    """A device value t passes iff ref(L (1 - d)) - a' <= t <= ref(L (1 + d)) + a', a' = a max(1, |t|).  No ray is left out: a bracket
    that flips across a gap lies between the two references."""
    t = float(t)
    if not np.isfinite(t):
        return False
    lo, hi = bounds(ts, te, sigma, delta, L, d)
    tol = a * max(1.0, abs(t))
    return lo - tol <= t <= hi + tol


def accepts_od(od, sigma, delta, d=D_REL):
    """od_front passes iff it is E_{n-1} up to the relative width of the prefix sums."""
    E = od_front(sigma, delta)
    od = float(od)
    return np.isfinite(od) and E * (1.0 - d) <= od <= E * (1.0 + d)
