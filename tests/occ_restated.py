"""The occupancy grid of include/eonerf_occ.h restated: numpy for the definitions (cell index, culling rule, update, dilation, bit
packing, the Philox draw of the per-cell points), torch for what the GPU tests filter on the device.  Written from the header, not
from the kernels; tests/test_occ_restated_cpu.py holds it to brute-force loops."""
import numpy as np
import torch

F = np.float32


# ---------------------------------------------------------------------------------------------------------------- cells
def cell_axis(x, r):
    """i = min(r - 1, (int)(((x + 1) * 0.5f) * (float)r)): three fp32 operations, each rounded."""
    x = np.asarray(x, dtype=F)
    v = ((x + F(1.0)) * F(0.5)) * F(r)
    assert v.dtype == F
    return np.minimum(r - 1, v.astype(np.int64))


def cell_index(xyz, r):
    """flat cell (ix * r + iy) * r + iz of points [..., 3]."""
    xyz = np.asarray(xyz, dtype=F)
    return (cell_axis(xyz[..., 0], r) * r + cell_axis(xyz[..., 1], r)) * r + cell_axis(xyz[..., 2], r)


def pack_bits(flags):
    """bool [n] -> uint32 [ceil(n / 32)]: cell c is bit c & 31 of word c >> 5; the unused bits of the last word are zero."""
    flags = np.asarray(flags, dtype=bool).reshape(-1)
    n = flags.size
    padded = np.zeros((n + 31) // 32 * 32, dtype=np.uint64)
    padded[:n] = flags
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def unpack_bits(words, n):
    words = np.asarray(words).astype(np.uint32).astype(np.uint64)
    return (((words[:, None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)).reshape(-1)[:n]).astype(bool)


# ---------------------------------------------------------------------------------------------------------------- culling
def keep_mask(ray_indices, occupied):
    """The culling rule on a cube-valid sample list in ray order: a sample is kept iff its cell's bit is set (`occupied`) or it is the
    last sample of its ray in the list."""
    ray_indices = np.asarray(ray_indices).reshape(-1)
    occupied = np.asarray(occupied, dtype=bool).reshape(-1)
    if ray_indices.size == 0:
        return occupied.copy()
    last = np.ones(ray_indices.size, dtype=bool)
    last[:-1] = ray_indices[1:] != ray_indices[:-1]
    return occupied | last


def cull(ray_indices, xyz, flags, r):
    """keep_mask of samples at mid points xyz [n, 3] against the grid `flags` (bool [r^3])."""
    return keep_mask(ray_indices, np.asarray(flags, dtype=bool).reshape(-1)[cell_index(xyz, r)])


# ---------------------------------------------------------------------------------------------------------------- update
def philox_u4(seed, c0, c1, c2, c3):
    """Philox4x32-10 at counters (c0, c1, c2, c3) (arrays or scalars), key = the 64-bit seed -> fp32 [n, 4] in [0, 1), 24 bits each."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) for v in (c0, c1, c2, c3)]
    n = max(v.size for v in c)
    c = [np.broadcast_to(v, (n,)).copy() for v in c]
    m32 = np.uint64(0xFFFFFFFF)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        n0, n2 = (p1 >> np.uint64(32)) ^ c[1] ^ k0, (p0 >> np.uint64(32)) ^ c[3] ^ k1
        c = [n0 & m32, p1 & m32, n2 & m32, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([(v >> np.uint64(8)).astype(F) * F(2.0 ** -24) for v in c], axis=1)


def cell_points(r, seed=0, call=0, jitter=True):
    """One point per cell, [r^3, 3] fp32: per axis ((i + u) / r) * 2 - 1, every operation rounded in fp32; u = words 0..2 of the
    Philox draw at counter (cell, 0, 3, call), or 0.5 without jitter."""
    cells = np.arange(r ** 3, dtype=np.int64)
    idx = np.stack([cells // (r * r), (cells // r) % r, cells % r], axis=1).astype(F)
    u = philox_u4(seed, cells, 0, 3, call)[:, :3] if jitter else np.full((r ** 3, 3), 0.5, dtype=F)
    p = ((idx + u) / F(r)) * F(2.0) - F(1.0)
    assert p.dtype == F
    return p


def update(occs, sigma, step_size, decay, occ_thre):
    """-> (occs', mean fp64, thr fp32, flags bool [r^3]): occs' = max(occs * decay, sigma * step) in fp32, mean in fp64,
    thr = min((float)mean, occ_thre), flags = occs' > thr."""
    occs, sigma = np.asarray(occs, dtype=F), np.asarray(sigma, dtype=F)
    new = np.maximum(occs * F(decay), sigma * F(step_size))
    assert new.dtype == F
    mean = new.astype(np.float64).sum() / new.size
    thr = min(F(mean), F(occ_thre))
    return new, mean, F(thr), new > thr


def dilate(flags, r):
    """A cell is set if any of its 27 neighbours (itself included) is set; neighbours outside the cube do not exist."""
    g = np.asarray(flags, dtype=bool).reshape(r, r, r)
    p = np.zeros((r + 2, r + 2, r + 2), dtype=bool)
    p[1:-1, 1:-1, 1:-1] = g
    out = np.zeros_like(g)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                out |= p[dx:dx + r, dy:dy + r, dz:dz + r]
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- torch (device)
def cell_index_torch(x, y, z, r):
    """The cell formula in torch fp32 (one rounded op per step): flat int64 index of points given as three fp32 tensors."""
    def axis(v):
        return torch.clamp((((v + 1.0) * 0.5) * float(r)).to(torch.int64), max=r - 1)
    assert x.dtype == torch.float32
    return (axis(x) * r + axis(y)) * r + axis(z)


def keep_mask_torch(ray_indices, occupied):
    last = torch.ones_like(occupied)
    if ray_indices.numel() > 1:
        last[:-1] = ray_indices[1:] != ray_indices[:-1]
    return occupied | last


def mid_points_torch(table, ray_indices, t_starts, t_ends):
    """The sampler's mid points (sat_rendering.py:79-80) of the flattened samples of the [R, 11] ray table, unfused fp32."""
    mid = (t_starts + t_ends) / 2.0
    o, d = table[ray_indices, 0:3], table[ray_indices, 3:6]
    return o[:, 0] + d[:, 0] * mid, o[:, 1] + d[:, 1] * mid, o[:, 2] + d[:, 2] * mid
