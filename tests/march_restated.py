"""The march rule of include/eonerf_march.h restated in numpy fp64 over a dense [R, n] slot layout (n = n_samples - 1 slots per ray).
Nothing here re-implements a kernel: no lanes, no windows, no carried state -- prefix sums over the whole ray and the rule's sentences.

    valid [R, n] bool      the pass' validity (cube filter, grid rule) per slot
    sd    [R, n] float     sigma_i * delta_i (ignored where not valid); the camera pass' 1e10 interval already in delta
    eps, block             early_stop_eps and the slots per round
    values                 {name: [R, n] or [R, n, c]} per-sample values to accumulate with the weights

march() returns a dict:
    kept    [R, n] bool    valid slots of alive rounds
    alive   [R, rounds]    the ray is alive in round j
    rounds  [R] int        rounds the ray took part in: up to the round of its last valid slot, or up to the boundary it died at
    weights [R, n]         exp(-(sum of sd over kept slots in front)) * (1 - exp(-sd)) on kept slots, 0 elsewhere
    sums    {name: [R, c]} sum of weights * values;  wsum [R]
    geo     [R]            exclusive transmittance at the last valid slot if kept, else exp(-OD) at the boundary the ray died at, 1 without samples
    margin  [R]            min over the boundaries the ray was decided at of |exp(-OD_j) / eps - 1| (inf: no decision, or eps = 0)
"""
import numpy as np


def march(valid, sd, eps, block, values=None):
    valid = np.asarray(valid, dtype=bool)
    R, n = valid.shape
    sdv = np.where(valid, np.asarray(sd, dtype=np.float64), 0.0)
    n_rounds = max(1, -(-n // block))
    incl = np.cumsum(sdv, axis=1)
    # exclusive prefix = the inclusive one shifted (never "inclusive - self": the 1e10 interval would cancel the prefix)
    excl = np.concatenate([np.zeros((R, 1)), incl[:, :-1]], axis=1)
    od = np.zeros((R, n_rounds))                       # OD_j: sum of sd over valid i < j * block
    for j in range(1, n_rounds):
        od[:, j] = incl[:, j * block - 1]
    with np.errstate(over="ignore"):
        trans_at = np.exp(-od)
    ok = trans_at >= eps
    ok[:, 0] = True
    alive = np.logical_and.accumulate(ok, axis=1)
    slot_round = np.arange(n) // block
    kept = valid & alive[:, slot_round]
    # dead rounds are a suffix, so "kept slots in front of i" are all valid slots in front of a kept i
    with np.errstate(over="ignore"):
        weights = np.where(kept, np.exp(-excl) * (1.0 - np.exp(-sdv)), 0.0)
    has = valid.any(axis=1)
    last = np.where(has, n - 1 - np.argmax(valid[:, ::-1], axis=1), -1)
    last_round = np.where(has, last // block, -1)
    died = ~alive
    first_dead = np.where(died.any(axis=1), np.argmax(died, axis=1), n_rounds)      # j*: the boundary the ray died at
    rounds = np.where(has, np.minimum(last_round + 1, first_dead), 0)
    geo = np.ones(R)
    margin = np.full(R, np.inf)
    for r in range(R):
        if not has[r]:
            continue
        if kept[r, last[r]]:
            geo[r] = np.exp(-excl[r, last[r]])
        else:
            geo[r] = trans_at[r, first_dead[r]]
        if eps > 0:
            # decided at boundaries 1 .. min(j*, round of the last valid slot): those with samples still behind them, while alive
            for j in range(1, min(first_dead[r], last_round[r]) + 1):
                margin[r] = min(margin[r], abs(trans_at[r, j] / eps - 1.0))
    out = {"kept": kept, "alive": alive, "rounds": rounds, "weights": weights, "wsum": weights.sum(axis=1), "geo": geo, "margin": margin, "sums": {}}
    for name, v in (values or {}).items():
        v = np.asarray(v, dtype=np.float64)
        v3 = v[:, :, None] if v.ndim == 2 else v
        out["sums"][name] = (weights[:, :, None] * np.where(kept[:, :, None], v3, 0.0)).sum(axis=1)
    return out


def dense_layout(ray_indices, slots, n_rays, n, **columns):
    """Scatter a flattened sample list (ray index, slot index per sample) into the dense layout: valid [R, n] and one [R, n(, c)] array
    per keyword column."""
    ray_indices, slots = np.asarray(ray_indices), np.asarray(slots)
    valid = np.zeros((n_rays, n), dtype=bool)
    valid[ray_indices, slots] = True
    out = {}
    for name, col in columns.items():
        col = np.asarray(col, dtype=np.float64)
        d = np.zeros((n_rays, n) + col.shape[1:])
        d[ray_indices, slots] = col
        out[name] = d
    return valid, out
