// Host-only checks of include/eonerf_components.h (eonerf_components_check.h), built for the CPU under the address +
// undefined-behaviour sanitizers (tests/host/test_components_host.py): every refusal in its documented order, the size arithmetic at
// EONERF_MESH_MAX_POINTS and one beyond, the rule's predicates, and a plain sequential union-find over those predicates.
// No HIP runtime call is made and no device pointer is dereferenced.
//   components_checks                 the checks
//   components_checks IN OUT          also labels the volume in IN (int32 nx ny nz side, float level, float f[nz*ny*nx]), filters it
//                                     (int64 min_points, int32 protect_boundary follow the volume) and writes OUT
//                                     (int64 counts[4] dropped[2], int32 labels[n], uint32 info[n], float f_out[n])
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../eonerf_code_amd/csrc/eonerf_components_check.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const void* const dev = reinterpret_cast<const void*>((uintptr_t)1 << 40);      // never dereferenced: stands for device pointers

struct Labelled { std::vector<int32_t> labels; std::vector<uint32_t> info; int64_t counts[4]; };

static int32_t find(std::vector<int32_t>& parent, int32_t x) {
    while (parent.at(x) != x) x = parent[x] = parent.at(parent[x]);
    return x;
}

// the rule, one point and one forward edge after the other; a union always hangs the larger root below the smaller one
static Labelled label(const std::vector<float>& f, int nx, int ny, int nz, float level, int side) {
    const int64_t n = (int64_t)mesh_points(nx, ny, nz);
    Labelled out;
    std::vector<int32_t>& parent = out.labels;
    parent.assign(n, -1);
    out.info.assign(n, 0u);
    for (int64_t p = 0; p < n; ++p)
        if (cc_on_side(f.at(p), level, side)) parent[p] = (int32_t)p;
    for (int64_t p = 0; p < n; ++p) {
        if (parent[p] < 0) continue;
        const int i = (int)(p % nx), j = (int)(p / nx % ny), k = (int)(p / nx / ny);
        for (int s = 0; s < 7; ++s) {
            const int d = cc_dir(s);
            if (((d & 1) && i + 1 >= nx) || ((d & 2) && j + 1 >= ny) || ((d & 4) && k + 1 >= nz)) continue;
            const int64_t q = p + mesh_corner_offset(d, (unsigned)nx, (unsigned)nx * (unsigned)ny);
            if (parent.at(q) < 0) continue;
            const int32_t a = find(parent, (int32_t)p), b = find(parent, (int32_t)q);
            if (a != b) parent[a > b ? a : b] = a > b ? b : a;
        }
    }
    uint64_t packed = 0;
    out.counts[0] = out.counts[1] = 0;
    for (int64_t p = 0; p < n; ++p) {
        if (parent[p] < 0) continue;
        const int32_t r = find(parent, (int32_t)p);
        const int i = (int)(p % nx), j = (int)(p / nx % ny), k = (int)(p / nx / ny);
        out.info.at(r) += 1u;
        if (cc_on_boundary(i, j, k, nx, ny, nz)) out.info[r] |= EONERF_CC_BOUNDARY;
        ++out.counts[1];
    }
    for (int64_t p = 0; p < n; ++p) {
        if (parent[p] < 0) continue;
        parent[p] = find(parent, (int32_t)p);
        if (parent[p] == p) {
            ++out.counts[0];
            const uint64_t mine = cc_pack_largest(out.info[p] & ~EONERF_CC_BOUNDARY, (uint32_t)p);
            if (mine > packed) packed = mine;
        }
    }
    out.counts[2] = cc_largest_size(packed);
    out.counts[3] = cc_largest_root(packed);
    return out;
}

int main(int argc, char** argv) {
    const float nanf_ = nanf(""), inff_ = INFINITY;

    // ---------------------------------------------------------------- sizes
    const int64_t MAXP = EONERF_MESH_MAX_POINTS;
    CHECK(cc_workspace_bytes(2, 2, 2) == kCcWorkspaceBytes && cc_workspace_bytes(33, 17, 9) == kCcWorkspaceBytes, "plain shapes");
    CHECK(cc_workspace_bytes(1, 2, 2) == 0 && cc_workspace_bytes(2, 1, 2) == 0 && cc_workspace_bytes(2, 2, 1) == 0 && cc_workspace_bytes(-5, 9, 9) == 0, "a dimension below 2");
    CHECK(cc_workspace_bytes(1 << 14, 1 << 13, 2) == kCcWorkspaceBytes && cc_workspace_bytes(2, 2, MAXP / 4) == kCcWorkspaceBytes, "the last point count that fits");
    CHECK(cc_workspace_bytes((1 << 14) + 1, 1 << 13, 2) == 0 && cc_workspace_bytes(2, 2, MAXP / 4 + 1) == 0 && cc_workspace_bytes(1 << 16, 1 << 16, 1 << 16) == 0 &&
          cc_workspace_bytes(INT_MAX, INT_MAX, INT_MAX) == 0 && cc_workspace_bytes((int64_t)1 << 32, (int64_t)1 << 32, 2) == 0, "beyond it, with no wrap in 64 bits");
    CHECK(kCcWorkspaceBytes >= sizeof(uint64_t), "the workspace holds the packed word");
    {
        const CcTiles a = cc_tiles(2, 2, 2), b = cc_tiles(kCcTx, kCcTy, kCcTz), c = cc_tiles(kCcTx + 1, kCcTy + 1, kCcTz + 1);
        CHECK(a.tiles == 1 && b.tiles == 1 && c.tx == 2 && c.ty == 2 && c.tz == 2 && c.tiles == 8, "tiles round up");
        // the shapes with the most tiles per point: the launch grid of one workgroup per tile stays far below 2^31
        const CcTiles z = cc_tiles(2, 2, (int)(MAXP / 4)), y = cc_tiles(2, (int)(MAXP / 4), 2), x = cc_tiles((int)(MAXP / 4), 2, 2);
        CHECK(z.tiles == (uint64_t)MAXP / 4 / kCcTz && y.tiles == (uint64_t)MAXP / 4 / kCcTy && x.tiles == (uint64_t)MAXP / 4 / kCcTx, "thin volumes at the limit");
        CHECK(z.tiles < ((uint64_t)1 << 31) && (uint64_t)MAXP <= (uint64_t)INT_MAX, "grid sizes and labels stay int32");
        CHECK((uint64_t)MAXP < (uint64_t)EONERF_CC_BOUNDARY, "a count stays below bit 31");
    }

    // ---------------------------------------------------------------- label
    const size_t need = kCcWorkspaceBytes;
    CHECK(cc_check_label(dev, 33, 17, 9, 0.5f, 0, dev, dev, dev, dev, need) == EONERF_OK && cc_check_label(dev, 33, 17, 9, 0.5f, 1, dev, dev, dev, dev, need) == EONERF_OK, "plain calls");
    CHECK(cc_check_label(nullptr, 33, 17, 9, 0.5f, 0, dev, dev, dev, dev, need) == EONERF_E_ARG && cc_check_label(dev, 33, 17, 9, 0.5f, 0, nullptr, dev, dev, dev, need) == EONERF_E_ARG &&
          cc_check_label(dev, 33, 17, 9, 0.5f, 0, dev, nullptr, dev, dev, need) == EONERF_E_ARG && cc_check_label(dev, 33, 17, 9, 0.5f, 0, dev, dev, nullptr, dev, need) == EONERF_E_ARG &&
          cc_check_label(dev, 33, 17, 9, 0.5f, 0, dev, dev, dev, nullptr, need) == EONERF_E_ARG, "null pointers");
    CHECK(cc_check_label(dev, 1, 17, 9, 0.5f, 0, dev, dev, dev, dev, need) == EONERF_E_ARG && cc_check_label(dev, 33, 1, 9, 0.5f, 0, dev, dev, dev, dev, need) == EONERF_E_ARG &&
          cc_check_label(dev, 33, 17, 0, 0.5f, 0, dev, dev, dev, dev, need) == EONERF_E_ARG, "a dimension below 2");
    CHECK(cc_check_label(dev, (1 << 14) + 1, 1 << 13, 2, 0.5f, 0, dev, dev, dev, dev, SIZE_MAX) == EONERF_E_UNSUPPORTED, "one row beyond the limit");
    CHECK(cc_check_label(dev, 1 << 14, 1 << 13, 2, 0.5f, 0, dev, dev, dev, dev, need) == EONERF_OK, "the limit itself");
    CHECK(cc_check_label(dev, 33, 17, 9, nanf_, 0, dev, dev, dev, dev, need) == EONERF_E_ARG && cc_check_label(dev, 33, 17, 9, -inff_, 0, dev, dev, dev, dev, need) == EONERF_E_ARG, "a level that is not finite");
    CHECK(cc_check_label(dev, 33, 17, 9, 0.5f, 2, dev, dev, dev, dev, need) == EONERF_E_ARG && cc_check_label(dev, 33, 17, 9, 0.5f, -1, dev, dev, dev, dev, need) == EONERF_E_ARG, "a side that is none");
    CHECK(cc_check_label(dev, 33, 17, 9, 0.5f, 0, dev, dev, dev, dev, need - 1) == EONERF_E_WORKSPACE && cc_check_label(dev, 33, 17, 9, 0.5f, 0, dev, dev, dev, dev, 0) == EONERF_E_WORKSPACE, "a workspace too small");
    // the order: each refusal with every later one also present
    CHECK(cc_check_label(nullptr, 1, 17, 9, nanf_, 2, dev, dev, dev, dev, 0) == EONERF_E_ARG, "null first");
    CHECK(cc_check_label(dev, 1, INT_MAX, INT_MAX, nanf_, 2, dev, dev, dev, dev, 0) == EONERF_E_ARG, "dimension before the point count");
    CHECK(cc_check_label(dev, INT_MAX, INT_MAX, INT_MAX, nanf_, 2, dev, dev, dev, dev, 0) == EONERF_E_UNSUPPORTED, "point count before the level");
    CHECK(cc_check_label(dev, 33, 17, 9, nanf_, 2, dev, dev, dev, dev, 0) == EONERF_E_ARG && cc_check_label(dev, 33, 17, 9, 0.5f, 2, dev, dev, dev, dev, 0) == EONERF_E_ARG,
          "level and side before the workspace");

    // ---------------------------------------------------------------- filter
    CHECK(cc_check_filter(dev, dev, dev, 33, 17, 9, 0, 5, 0, dev, dev) == EONERF_OK && cc_check_filter(dev, dev, dev, 33, 17, 9, 0, 0, 1, dev, dev) == EONERF_OK &&
          cc_check_filter(dev, dev, dev, 33, 17, 9, 1, INT64_MAX, 1, dev, dev) == EONERF_OK, "plain calls");
    CHECK(cc_check_filter(nullptr, dev, dev, 33, 17, 9, 0, 5, 0, dev, dev) == EONERF_E_ARG && cc_check_filter(dev, nullptr, dev, 33, 17, 9, 0, 5, 0, dev, dev) == EONERF_E_ARG &&
          cc_check_filter(dev, dev, nullptr, 33, 17, 9, 0, 5, 0, dev, dev) == EONERF_E_ARG && cc_check_filter(dev, dev, dev, 33, 17, 9, 0, 5, 0, nullptr, dev) == EONERF_E_ARG &&
          cc_check_filter(dev, dev, dev, 33, 17, 9, 0, 5, 0, dev, nullptr) == EONERF_E_ARG, "null pointers");
    CHECK(cc_check_filter(dev, dev, dev, 1, 17, 9, 0, 5, 0, dev, dev) == EONERF_E_ARG && cc_check_filter(dev, dev, dev, 33, 17, 1, 0, 5, 0, dev, dev) == EONERF_E_ARG, "a dimension below 2");
    CHECK(cc_check_filter(dev, dev, dev, (1 << 14) + 1, 1 << 13, 2, 0, 5, 0, dev, dev) == EONERF_E_UNSUPPORTED, "beyond the limit");
    CHECK(cc_check_filter(dev, dev, dev, 33, 17, 9, 2, 5, 1, dev, dev) == EONERF_E_ARG && cc_check_filter(dev, dev, dev, 33, 17, 9, 0, 5, 2, dev, dev) == EONERF_E_ARG &&
          cc_check_filter(dev, dev, dev, 33, 17, 9, 0, 5, -1, dev, dev) == EONERF_E_ARG, "side and protect_boundary are 0 or 1");
    CHECK(cc_check_filter(dev, dev, dev, 33, 17, 9, 0, -1, 0, dev, dev) == EONERF_E_ARG && cc_check_filter(dev, dev, dev, 33, 17, 9, 0, INT64_MIN, 1, dev, dev) == EONERF_E_ARG, "a negative min_points");
    CHECK(cc_check_filter(dev, dev, dev, 33, 17, 9, 1, 5, 0, dev, dev) == EONERF_E_ARG, "the outside world is not a cavity");
    CHECK(cc_check_filter(nullptr, dev, dev, 1, 17, 9, 1, -1, 0, dev, dev) == EONERF_E_ARG, "null first");
    CHECK(cc_check_filter(dev, dev, dev, 1, INT_MAX, INT_MAX, 1, -1, 0, dev, dev) == EONERF_E_ARG, "dimension before the point count");
    CHECK(cc_check_filter(dev, dev, dev, INT_MAX, INT_MAX, INT_MAX, 1, -1, 0, dev, dev) == EONERF_E_UNSUPPORTED, "point count before the values");

    // ---------------------------------------------------------------- predicates
    CHECK(cc_on_side(1.f, 1.f, 0) && !cc_on_side(1.f, 1.f, 1) && !cc_on_side(0.5f, 1.f, 0) && cc_on_side(0.5f, 1.f, 1), "a value on the level is inside");
    CHECK(!cc_on_side(nanf_, 0.f, 0) && cc_on_side(nanf_, 0.f, 1) && cc_on_side(inff_, 0.f, 0) && cc_on_side(-inff_, 0.f, 1), "a NaN is outside");
    { int seen = 0; for (int s = 0; s < 7; ++s) seen |= 1 << cc_dir(s); CHECK(seen == 0xfe, "the seven directions are the seven non-zero corners"); }
    CHECK(cc_on_boundary(0, 1, 1, 3, 3, 3) && cc_on_boundary(1, 2, 1, 3, 3, 3) && cc_on_boundary(1, 1, 2, 3, 3, 3) && !cc_on_boundary(1, 1, 1, 3, 3, 3), "the boundary");
    CHECK(cc_dropped(3u, 4, 0) && !cc_dropped(4u, 4, 0) && !cc_dropped(3u, 0, 0) && cc_dropped(3u | EONERF_CC_BOUNDARY, 4, 0) && !cc_dropped(3u | EONERF_CC_BOUNDARY, 4, 1) &&
          cc_dropped((uint32_t)MAXP, INT64_MAX, 1), "which component is dropped");
    CHECK(cc_fill(0) == -inff_ && cc_fill(1) == inff_, "the fill values");
    CHECK(cc_pack_largest(5, 9) > cc_pack_largest(4, 0) && cc_pack_largest(5, 3) > cc_pack_largest(5, 9) && cc_largest_size(cc_pack_largest(5, 9)) == 5 &&
          cc_largest_root(cc_pack_largest(5, 9)) == 9 && cc_largest_root(cc_pack_largest(1, 0)) == 0 && cc_largest_root(0) == -1 && cc_largest_size(0) == 0, "the packed word");

    // ---------------------------------------------------------------- one cell: 000-110 is an edge, 100-010 is none
    {
        std::vector<float> f(8, -1.f);
        f[0] = f[3] = 1.f;
        Labelled a = label(f, 2, 2, 2, 0.f, 0);
        CHECK(a.counts[0] == 1 && a.counts[1] == 2 && a.counts[2] == 2 && a.counts[3] == 0 && a.labels[3] == 0 && a.info[0] == (2u | EONERF_CC_BOUNDARY), "000-110 joined");
        f.assign(8, -1.f);
        f[1] = f[2] = 1.f;
        Labelled b = label(f, 2, 2, 2, 0.f, 0);
        CHECK(b.counts[0] == 2 && b.counts[2] == 1 && b.counts[3] == 1 && b.labels[1] == 1 && b.labels[2] == 2, "100-010 apart");
        Labelled c = label(f, 2, 2, 2, 0.f, 1);
        CHECK(c.counts[0] == 1 && c.counts[1] == 6 && c.labels[1] == -1 && c.labels[7] == 0, "the complement of the pair is one piece");
    }

    if (argc == 3) {
        FILE* in = fopen(argv[1], "rb");
        if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        int32_t head[4]; float level = 0.f; int64_t min_points = 0; int32_t protect = 0;
        bool good = fread(head, 4, 4, in) == 4 && fread(&level, 4, 1, in) == 1 && mesh_points(head[0], head[1], head[2]) != 0;
        std::vector<float> f(good ? (size_t)mesh_points(head[0], head[1], head[2]) : 0);
        good = good && fread(f.data(), 4, f.size(), in) == f.size() && fread(&min_points, 8, 1, in) == 1 && fread(&protect, 4, 1, in) == 1;
        fclose(in);
        good = good && cc_check_label(dev, head[0], head[1], head[2], level, head[3], dev, dev, dev, dev, kCcWorkspaceBytes) == EONERF_OK &&
               cc_check_filter(dev, dev, dev, head[0], head[1], head[2], head[3], min_points, protect, dev, dev) == EONERF_OK;
        if (!good) { fprintf(stderr, "malformed volume file\n"); return 2; }
        const Labelled m = label(f, head[0], head[1], head[2], level, head[3]);
        int64_t dropped[2] = {0, 0};
        std::vector<float> out(f);
        for (size_t p = 0; p < f.size(); ++p) {
            const int32_t l = m.labels[p];
            if (l >= 0 && cc_dropped(m.info.at(l), min_points, protect)) { out[p] = cc_fill(head[3]); ++dropped[1]; dropped[0] += l == (int32_t)p; }
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        fwrite(m.counts, 8, 4, o);
        fwrite(dropped, 8, 2, o);
        fwrite(m.labels.data(), 4, m.labels.size(), o);
        fwrite(m.info.data(), 4, m.info.size(), o);
        fwrite(out.data(), 4, out.size(), o);
        fclose(o);
    }

    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("components checks ok\n");
    return 0;
}
