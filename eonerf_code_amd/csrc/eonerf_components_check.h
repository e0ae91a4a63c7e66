// Host side of include/eonerf_components.h: the refusals of the entry points in their documented order, the 64-bit sizes and the
// rule's predicates -- which side a value is on, the seven forward directions, the boundary of the volume, which component the filter
// drops -- in functions with no HIP call, shared by the kernels of eonerf_components.hip and by a stand-alone program
// (tests/host/components_checks.cpp).  Each check returns 0 or the EONERF_E_* the entry point returns before it launches anything.
// The point count and the directions are those of the mesh group (eonerf_mesh_check.h): one statement of each.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_components.h"
#include "eonerf_mesh_check.h"

constexpr int kCcBlock = 256;                                                     // threads of every kernel of the group
constexpr int kCcTx = EONERF_CC_TILE_X, kCcTy = EONERF_CC_TILE_Y, kCcTz = EONERF_CC_TILE_Z;
constexpr int kCcTile = kCcTx * kCcTy * kCcTz;                                    // points of one tile
constexpr int kCcRounds = kCcTile / kCcBlock;                                     // points per thread of the LOCAL launch
static_assert(kCcTile % kCcBlock == 0 && kCcTile <= 32768, "a tile is a whole number of rounds and its local indices fit an int16");
static_assert((kCcTx & (kCcTx - 1)) == 0 && (kCcTy & (kCcTy - 1)) == 0 && (kCcTz & (kCcTz - 1)) == 0, "tile sizes are powers of two");
constexpr size_t kCcWorkspaceBytes = 256;                                         // one 64-bit word: the packed largest component

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
struct CcTiles { uint64_t tx, ty, tz, tiles; };
inline CcTiles cc_tiles(int nx, int ny, int nz) {
    CcTiles t;
    t.tx = ((uint64_t)nx + kCcTx - 1) / kCcTx; t.ty = ((uint64_t)ny + kCcTy - 1) / kCcTy; t.tz = ((uint64_t)nz + kCcTz - 1) / kCcTz;
    t.tiles = t.tx * t.ty * t.tz;             // at most 2^28 * 4 * 2 (each dimension >= 2 rounds up to at most tile / 2 times itself): 64 bits hold it
    return t;
}
inline size_t cc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) { return mesh_points(nx, ny, nz) ? kCcWorkspaceBytes : 0; }

// ---- refusals ---------------------------------------------------------------------------------------------------------------------
inline int cc_check_label(const void* f, int nx, int ny, int nz, float level, int side, const void* labels, const void* info,
                          const void* counts_dev, const void* workspace, size_t workspace_bytes) {
    if (!f || !labels || !info || !counts_dev || !workspace) return EONERF_E_ARG;
    if (nx < 2 || ny < 2 || nz < 2) return EONERF_E_ARG;
    if (!mesh_points(nx, ny, nz)) return EONERF_E_UNSUPPORTED;
    if (!isfinite(level)) return EONERF_E_ARG;
    if (side != 0 && side != 1) return EONERF_E_ARG;
    if (workspace_bytes < cc_workspace_bytes(nx, ny, nz)) return EONERF_E_WORKSPACE;
    return EONERF_OK;
}

inline int cc_check_filter(const void* f, const void* labels, const void* info, int nx, int ny, int nz, int side, int64_t min_points,
                           int protect_boundary, const void* f_out, const void* dropped_dev) {
    if (!f || !labels || !info || !f_out || !dropped_dev) return EONERF_E_ARG;
    if (nx < 2 || ny < 2 || nz < 2) return EONERF_E_ARG;
    if (!mesh_points(nx, ny, nz)) return EONERF_E_UNSUPPORTED;
    if ((side != 0 && side != 1) || (protect_boundary != 0 && protect_boundary != 1)) return EONERF_E_ARG;
    if (min_points < 0) return EONERF_E_ARG;
    if (side == 1 && !protect_boundary) return EONERF_E_ARG;
    return EONERF_OK;
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
// side 0: f >= level (false for a NaN); side 1: everything else
MESH_HD inline bool cc_on_side(float v, float level, int side) { return (v >= level) != (side != 0); }
// the forward direction of slot 0 .. 6 as three bits, x = 1, y = 2, z = 4: the owned edges of the mesh rule
MESH_HD inline int cc_dir(int slot) { return mesh_slot_dir(slot); }
// a point with an index equal to 0 or n - 1 on its axis
MESH_HD inline bool cc_on_boundary(int i, int j, int k, int nx, int ny, int nz) {
    return i == 0 || j == 0 || k == 0 || i == nx - 1 || j == ny - 1 || k == nz - 1;
}
// the filter: is the component with this info word dropped?
MESH_HD inline bool cc_dropped(uint32_t info, int64_t min_points, int protect_boundary) {
    return (int64_t)(info & ~EONERF_CC_BOUNDARY) < min_points && !(protect_boundary && (info & EONERF_CC_BOUNDARY));
}
// the value the filter writes into a dropped point
MESH_HD inline float cc_fill(int side) { return side ? INFINITY : -INFINITY; }
// the 64-bit word whose maximum names the largest component, the smallest root among ties, and its two halves
MESH_HD inline uint64_t cc_pack_largest(uint32_t size, uint32_t root) { return ((uint64_t)size << 32) | (uint64_t)(0xFFFFFFFFu - root); }
MESH_HD inline int64_t cc_largest_size(uint64_t packed) { return (int64_t)(packed >> 32); }
MESH_HD inline int64_t cc_largest_root(uint64_t packed) { return packed ? (int64_t)(0xFFFFFFFFu - (uint32_t)packed) : -1; }
