// Host-only checks of include/eonerf_mesh.h (eonerf_mesh_check.h), built for the CPU under the address + undefined-behaviour
// sanitizers (tests/host/test_mesh_host.py): every refusal in its documented order, the size arithmetic at EONERF_MESH_MAX_POINTS and
// one beyond, the workspace carve, and the rule itself -- the functions the kernels of eonerf_mesh.hip call per thread, run here in a
// loop over the points with the workspace's own layout (scans inside tiles of EONERF_MESH_TILE points plus tile offsets).
// No HIP runtime call is made and no device pointer is dereferenced.
//   mesh_checks                 the checks
//   mesh_checks IN OUT          also meshes the volume in IN (int32 nx ny nz, float level origin[3] spacing[3], float f[nz*ny*nx]) and
//                               writes OUT (int64 V T nonfinite, float vertices[V][3], int64 keys[V], int32 triangles[T][3])
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <utility>
#include <vector>

#include "../../eonerf_code_amd/csrc/eonerf_mesh_check.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const void* const dev = reinterpret_cast<const void*>((uintptr_t)1 << 40);      // never dereferenced: stands for device pointers
static constexpr MeshTable kTable = mesh_make_table();

struct Mesh { std::vector<float> vertices; std::vector<int64_t> keys; std::vector<int32_t> triangles; int64_t nonfinite = 0; };

// count + emit as the kernels do them, one point after the other
static Mesh run(const std::vector<float>& f, int nx, int ny, int nz, float level, const float* origin, const float* spacing) {
    const uint64_t n = mesh_points(nx, ny, nz);
    const MeshCarve c = mesh_carve(n);
    std::vector<uint16_t> lv(n), lt(n);
    std::vector<uint8_t> mask(n);
    std::vector<uint32_t> l1v(c.n1), l1t(c.n1);
    std::vector<uint8_t> in8(n);
    Mesh m;
    uint32_t tile_v = 0, tile_t = 0, all_v = 0, all_t = 0;
    for (uint64_t p = 0; p < n; ++p) {
        if (p % kMeshTile == 0) { l1v[p / kMeshTile] = all_v; l1t[p / kMeshTile] = all_t; tile_v = tile_t = 0; }
        const int i = (int)(p % nx), j = (int)(p / nx % ny), k = (int)(p / nx / ny);
        const MeshPoint pt = mesh_classify(kTable, f.data(), nx, ny, nz, i, j, k, (unsigned)p, level);
        lv[p] = (uint16_t)tile_v; lt[p] = (uint16_t)tile_t; mask[p] = (uint8_t)pt.mask; in8[p] = (uint8_t)pt.in8;
        const uint32_t nv = (uint32_t)__builtin_popcount(pt.mask);
        tile_v += nv; tile_t += pt.triangles; all_v += nv; all_t += pt.triangles;
        m.nonfinite += pt.nonfinite;
    }
    m.vertices.resize((size_t)all_v * 3); m.keys.resize(all_v); m.triangles.resize((size_t)all_t * 3);
    const unsigned nxy = (unsigned)nx * (unsigned)ny;
    for (uint64_t p = 0; p < n; ++p) {
        const int i = (int)(p % nx), j = (int)(p / nx % ny), k = (int)(p / nx / ny);
        for (int s = 0; s < 7; ++s) {
            if (!((mask[p] >> s) & 1)) continue;
            const uint32_t id = l1v[p / kMeshTile] + lv[p] + (uint32_t)__builtin_popcount(mask[p] & ((1u << s) - 1u));
            mesh_vertex(f.data(), nx, ny, i, j, k, (unsigned)p, s, level, origin, spacing, &m.vertices.at((size_t)id * 3));
            m.keys.at(id) = (int64_t)p * 8 + s;
        }
        if (i + 1 < nx && j + 1 < ny && k + 1 < nz && in8[p] != 0 && in8[p] != 0xff) {
            auto id_of = [&](int corner, int slot) {
                const unsigned q = (unsigned)p + mesh_corner_offset(corner, (unsigned)nx, nxy);
                return (int32_t)(l1v[q / kMeshTile] + lv[q] + (uint32_t)__builtin_popcount(mask[q] & ((1u << slot) - 1u)));
            };
            auto put = [&](uint64_t at, int32_t a, int32_t b, int32_t c3) {
                m.triangles.at(at * 3) = a; m.triangles.at(at * 3 + 1) = b; m.triangles.at(at * 3 + 2) = c3;
            };
            mesh_cell_triangles(kTable, in8[p], (uint64_t)l1t[p / kMeshTile] + lt[p], id_of, put);
        }
    }
    return m;
}

int main(int argc, char** argv) {
    const float nanf_ = nanf(""), inff_ = INFINITY;
    float org[3] = {-1.f, -1.f, -1.f}, sp[3] = {0.125f, 0.125f, 0.25f};

    // ---------------------------------------------------------------- sizes
    const int64_t MAXP = EONERF_MESH_MAX_POINTS;
    CHECK(mesh_points(2, 2, 2) == 8 && mesh_points(33, 17, 9) == 5049, "plain shapes");
    CHECK(mesh_points(1, 2, 2) == 0 && mesh_points(2, 1, 2) == 0 && mesh_points(2, 2, 1) == 0 && mesh_points(0, 0, 0) == 0 && mesh_points(-5, 9, 9) == 0,
          "a dimension below 2");
    CHECK(mesh_points(1 << 14, 1 << 13, 2) == (uint64_t)MAXP && mesh_points(MAXP / 4, 2, 2) == (uint64_t)MAXP, "the last point count that fits");
    CHECK(mesh_points((1 << 14) + 1, 1 << 13, 2) == 0 && mesh_points(MAXP / 4 + 1, 2, 2) == 0 && mesh_points(2, 2, MAXP / 4 + 1) == 0, "beyond it");
    CHECK(mesh_points(INT_MAX, INT_MAX, INT_MAX) == 0 && mesh_points(INT64_MAX, 2, 2) == 0 && mesh_points(1 << 16, 1 << 16, 1 << 16) == 0 &&
          mesh_points((int64_t)1 << 32, (int64_t)1 << 32, 2) == 0, "no wrap in 64 bits");
    CHECK(7 * (uint64_t)MAXP <= (uint64_t)INT_MAX, "seven vertices per point stay an int32 index");
    CHECK(12 * (uint64_t)MAXP <= (uint64_t)UINT_MAX, "twelve triangles per cell stay a uint32 offset");
    CHECK(mesh_slab_points(1, 1, 0, 1) == 1 && mesh_slab_points(17, 17, 16, 1) == 289 && mesh_slab_points(0, 1, 0, 1) == 0 && mesh_slab_points(1, 1, -1, 1) == 0,
          "slabs take any dimension from 1");
    CHECK(mesh_slab_points(1 << 14, 1 << 14, 0, 1) == (uint64_t)MAXP && mesh_slab_points(1 << 14, 1 << 14, 0, 2) == 0 && mesh_slab_points(2, 2, MAXP, 1) == 0 &&
          mesh_slab_points(2, 2, INT_MAX, INT_MAX) == 0, "slab limits");
    {
        const MeshCarve c = mesh_carve(8);
        CHECK(c.n1 == 1 && c.n2 == 1 && c.lv_off == 0 && c.lt_off == 256 && c.mask_off == 512 && c.l1_off == 768 && c.l2_off == 1024 && c.l3_off == 1280 &&
              c.bytes == 1536, "the smallest carve: %zu", c.bytes);
        const MeshCarve t1 = mesh_carve(kMeshTile), t2 = mesh_carve(kMeshTile + 1);
        CHECK(t1.n1 == 1 && t2.n1 == 2 && t2.n2 == 1, "one point beyond a tile");
        const MeshCarve s1 = mesh_carve((uint64_t)kMeshTile * kMeshTile), s2 = mesh_carve((uint64_t)kMeshTile * kMeshTile + 1);
        CHECK(s1.n1 == (uint64_t)kMeshTile && s1.n2 == 1 && s2.n1 == (uint64_t)kMeshTile + 1 && s2.n2 == 2, "one point beyond a tile of tiles");
        const MeshCarve m = mesh_carve((uint64_t)MAXP);
        CHECK(m.n1 == (uint64_t)MAXP / kMeshTile && m.n2 == (uint64_t)MAXP / kMeshTile / kMeshTile && m.n2 <= (uint64_t)kMeshTile, "the largest call: one third-level sum");
        CHECK(m.lt_off == 2 * (size_t)MAXP && m.mask_off == 4 * (size_t)MAXP && m.l1_off == 5 * (size_t)MAXP && m.bytes == 5 * (size_t)MAXP + 8 * m.n1 + 8 * m.n2 + 256,
              "%zu bytes at the limit (beyond 2^30: computed in 64 bits)", m.bytes);
        for (uint64_t n : {(uint64_t)8, (uint64_t)1000, (uint64_t)1025, (uint64_t)5049, (uint64_t)MAXP}) {
            const MeshCarve c2 = mesh_carve(n);
            CHECK(c2.lv_off % 256 == 0 && c2.lt_off % 256 == 0 && c2.mask_off % 256 == 0 && c2.l1_off % 256 == 0 && c2.l2_off % 256 == 0 && c2.l3_off % 256 == 0 &&
                  c2.lt_off >= c2.lv_off + 2 * n && c2.mask_off >= c2.lt_off + 2 * n && c2.l1_off >= c2.mask_off + n && c2.l2_off >= c2.l1_off + 8 * c2.n1 &&
                  c2.l3_off >= c2.l2_off + 8 * c2.n2 && c2.bytes >= c2.l3_off + 8, "parts aligned and disjoint at %llu points", (unsigned long long)n);
        }
    }
    const size_t need = mesh_carve(5049).bytes;

    // ---------------------------------------------------------------- lattice points
    CHECK(mesh_check_lattice(org, sp, 33, 17, 0, 9, dev) == EONERF_OK && mesh_check_lattice(org, sp, 1, 1, 5, 1, dev) == EONERF_OK, "plain calls");
    CHECK(mesh_check_lattice(nullptr, sp, 33, 17, 0, 9, dev) == EONERF_E_ARG && mesh_check_lattice(org, nullptr, 33, 17, 0, 9, dev) == EONERF_E_ARG &&
          mesh_check_lattice(org, sp, 33, 17, 0, 9, nullptr) == EONERF_E_ARG, "null pointers");
    CHECK(mesh_check_lattice(org, sp, 0, 17, 0, 9, dev) == EONERF_E_ARG && mesh_check_lattice(org, sp, 33, 0, 0, 9, dev) == EONERF_E_ARG &&
          mesh_check_lattice(org, sp, 33, 17, 0, 0, dev) == EONERF_E_ARG && mesh_check_lattice(org, sp, 33, 17, -1, 9, dev) == EONERF_E_ARG, "empty or negative");
    CHECK(mesh_check_lattice(nullptr, sp, 0, 17, 0, 9, dev) == EONERF_E_ARG, "a null pointer comes first");
    CHECK(mesh_check_lattice(org, sp, 1 << 15, 1 << 14, 0, 1, dev) == EONERF_E_UNSUPPORTED && mesh_check_lattice(org, sp, 2, 2, INT_MAX, 2, dev) == EONERF_E_UNSUPPORTED,
          "too many points");
    for (int k = 0; k < 3; ++k) {
        float bad[3] = {sp[0], sp[1], sp[2]};
        bad[k] = nanf_;
        CHECK(mesh_check_lattice(bad, sp, 33, 17, 0, 9, dev) == EONERF_E_ARG && mesh_check_lattice(org, bad, 33, 17, 0, 9, dev) == EONERF_E_ARG, "NaN %d", k);
        CHECK(mesh_check_lattice(bad, sp, 1 << 15, 1 << 14, 0, 1, dev) == EONERF_E_UNSUPPORTED, "the point count comes before the values");
        bad[k] = 0.f;
        CHECK(mesh_check_lattice(bad, sp, 33, 17, 0, 9, dev) == EONERF_OK && mesh_check_lattice(org, bad, 33, 17, 0, 9, dev) == EONERF_E_ARG, "zero origin is fine, zero spacing is not %d", k);
        bad[k] = -0.25f;
        CHECK(mesh_check_lattice(org, bad, 33, 17, 0, 9, dev) == EONERF_OK, "a negative spacing is a spacing");
    }

    // ---------------------------------------------------------------- count
    CHECK(mesh_check_count(dev, 33, 17, 9, 0.5f, dev, dev, need) == EONERF_OK, "a plain call");
    CHECK(mesh_check_count(nullptr, 33, 17, 9, 0.5f, dev, dev, need) == EONERF_E_ARG && mesh_check_count(dev, 33, 17, 9, 0.5f, nullptr, dev, need) == EONERF_E_ARG &&
          mesh_check_count(dev, 33, 17, 9, 0.5f, dev, nullptr, need) == EONERF_E_ARG, "null pointers");
    CHECK(mesh_check_count(dev, 1, 17, 9, 0.5f, dev, dev, need) == EONERF_E_ARG && mesh_check_count(dev, 33, 1, 9, 0.5f, dev, dev, need) == EONERF_E_ARG &&
          mesh_check_count(dev, 33, 17, 1, 0.5f, dev, dev, need) == EONERF_E_ARG && mesh_check_count(dev, -3, 17, 9, 0.5f, dev, dev, need) == EONERF_E_ARG, "a dimension below 2");
    CHECK(mesh_check_count(dev, (1 << 14) + 1, 1 << 13, 2, 0.5f, dev, dev, SIZE_MAX) == EONERF_E_UNSUPPORTED, "one row beyond the limit");
    CHECK(mesh_check_count(dev, 1 << 14, 1 << 13, 2, 0.5f, dev, dev, mesh_carve(MAXP).bytes) == EONERF_OK, "the limit itself");
    CHECK(mesh_check_count(dev, 33, 17, 9, nanf_, dev, dev, need) == EONERF_E_ARG && mesh_check_count(dev, 33, 17, 9, -inff_, dev, dev, need) == EONERF_E_ARG, "a level that is not finite");
    CHECK(mesh_check_count(dev, 33, 17, 9, 0.5f, dev, dev, need - 1) == EONERF_E_WORKSPACE && mesh_check_count(dev, 33, 17, 9, 0.5f, dev, dev, 0) == EONERF_E_WORKSPACE, "a workspace too small");
    // the order: each refusal with every later one also present
    CHECK(mesh_check_count(nullptr, 1, 17, 9, nanf_, dev, dev, 0) == EONERF_E_ARG, "null first");
    CHECK(mesh_check_count(dev, 1, INT_MAX, INT_MAX, nanf_, dev, dev, 0) == EONERF_E_ARG, "dimension before the point count");
    CHECK(mesh_check_count(dev, INT_MAX, INT_MAX, INT_MAX, nanf_, dev, dev, 0) == EONERF_E_UNSUPPORTED, "point count before the level");
    CHECK(mesh_check_count(dev, 33, 17, 9, nanf_, dev, dev, 0) == EONERF_E_ARG, "level before the workspace");

    // ---------------------------------------------------------------- emit
    struct Emit {
        const void *f = dev, *ws = dev, *v = dev, *t = dev, *st = dev;
        int nx = 33, ny = 17, nz = 9; float level = 0.5f; const float *o, *s; size_t bytes; int64_t cap_v = 100, cap_t = 200;
        int run() const { return mesh_check_emit(f, nx, ny, nz, level, o, s, ws, bytes, v, cap_v, t, cap_t, st); }
    };
    Emit ok; ok.o = org; ok.s = sp; ok.bytes = need;
    CHECK(ok.run() == EONERF_OK, "a plain call");
    { Emit e = ok; e.cap_v = e.cap_t = 0; CHECK(e.run() == EONERF_OK, "zero capacities"); }
    { Emit e = ok; e.f = nullptr; CHECK(e.run() == EONERF_E_ARG, "null f"); }
    { Emit e = ok; e.o = nullptr; CHECK(e.run() == EONERF_E_ARG, "null origin"); }
    { Emit e = ok; e.s = nullptr; CHECK(e.run() == EONERF_E_ARG, "null spacing"); }
    { Emit e = ok; e.ws = nullptr; CHECK(e.run() == EONERF_E_ARG, "null workspace"); }
    { Emit e = ok; e.v = nullptr; CHECK(e.run() == EONERF_E_ARG, "null vertices"); }
    { Emit e = ok; e.t = nullptr; CHECK(e.run() == EONERF_E_ARG, "null triangles"); }
    { Emit e = ok; e.st = nullptr; CHECK(e.run() == EONERF_E_ARG, "null status"); }
    { Emit e = ok; e.nx = 1; CHECK(e.run() == EONERF_E_ARG, "nx 1"); e = ok; e.ny = 1; CHECK(e.run() == EONERF_E_ARG, "ny 1"); e = ok; e.nz = 0; CHECK(e.run() == EONERF_E_ARG, "nz 0"); }
    { Emit e = ok; e.nx = (1 << 14) + 1; e.ny = 1 << 13; e.nz = 2; e.bytes = SIZE_MAX; CHECK(e.run() == EONERF_E_UNSUPPORTED, "beyond the limit"); }
    { Emit e = ok; e.level = inff_; CHECK(e.run() == EONERF_E_ARG, "infinite level"); }
    for (int k = 0; k < 3; ++k) {
        float bad[3] = {sp[0], sp[1], sp[2]};
        Emit e = ok;
        bad[k] = inff_; e.o = bad; CHECK(e.run() == EONERF_E_ARG, "infinite origin %d", k);
        e = ok; bad[k] = nanf_; e.s = bad; CHECK(e.run() == EONERF_E_ARG, "NaN spacing %d", k);
        bad[k] = 0.f; CHECK(e.run() == EONERF_E_ARG, "zero spacing %d", k);
        bad[k] = -0.f; CHECK(e.run() == EONERF_E_ARG, "minus zero spacing %d", k);
    }
    { Emit e = ok; e.cap_v = -1; CHECK(e.run() == EONERF_E_ARG, "negative cap_v"); e = ok; e.cap_t = INT64_MIN; CHECK(e.run() == EONERF_E_ARG, "negative cap_t"); }
    { Emit e = ok; e.bytes = need - 1; CHECK(e.run() == EONERF_E_WORKSPACE, "a workspace too small"); }
    // the order
    float zero_sp[3] = {0.f, 1.f, 1.f};
    { Emit e = ok; e.st = nullptr; e.nx = 1; e.level = nanf_; e.s = zero_sp; e.cap_v = -1; e.bytes = 0; CHECK(e.run() == EONERF_E_ARG, "null first");
      e.st = dev; e.ny = e.nz = INT_MAX; CHECK(e.run() == EONERF_E_ARG, "dimension before the point count");
      e.nx = INT_MAX; CHECK(e.run() == EONERF_E_UNSUPPORTED, "point count before the values");
      e.nx = 33; e.ny = 17; e.nz = 9; e.level = 0.5f; e.cap_v = 1; CHECK(e.run() == EONERF_E_ARG, "zero spacing before the workspace");
      e.s = sp; e.cap_t = -1; CHECK(e.run() == EONERF_E_ARG, "capacity before the workspace");
      e.cap_t = 0; CHECK(e.run() == EONERF_E_WORKSPACE, "the workspace last"); }

    // ---------------------------------------------------------------- the table
    for (int t = 0; t < 6; ++t) {
        CHECK(kTable.corner[t][0] == 0 && kTable.corner[t][3] == 7 && __builtin_popcount(kTable.corner[t][1]) == 1 && __builtin_popcount(kTable.corner[t][2]) == 2 &&
              (kTable.corner[t][1] & kTable.corner[t][2]) == kTable.corner[t][1], "tetrahedron %d is a path along the body diagonal", t);
        for (int m = 1; m < 15; ++m)
            for (unsigned q = 0; q < 3 * mesh_case_triangles(__builtin_popcount(m)); ++q) {
                const int owner = kTable.ref[t][m][q] & 7, slot = kTable.ref[t][m][q] >> 3, far = owner | mesh_slot_dir(slot);
                bool on_path_o = false, on_path_f = false, differ = false;
                int co = 0, cf = 0;
                for (int c = 0; c < 4; ++c) { if (kTable.corner[t][c] == owner) { on_path_o = true; co = c; } if (kTable.corner[t][c] == far) { on_path_f = true; cf = c; } }
                differ = (((m >> co) ^ (m >> cf)) & 1) != 0;
                CHECK(slot < 7 && !(owner & mesh_slot_dir(slot)) && on_path_o && on_path_f && differ, "tet %d case %d ref %u names a crossing edge of the tetrahedron", t, m, q);
            }
    }
    for (int s = 0; s < 7; ++s) CHECK(mesh_dir_slot(mesh_slot_dir(s)) == s, "slot %d", s);
    CHECK(mesh_slot_dir(0) == 1 && mesh_slot_dir(1) == 2 && mesh_slot_dir(2) == 4 && mesh_slot_dir(3) == 3 && mesh_slot_dir(4) == 5 && mesh_slot_dir(5) == 6 && mesh_slot_dir(6) == 7, "slot directions");

    // ---------------------------------------------------------------- a sphere on 9^3 points: 472 vertices, 940 triangles, closed and oriented
    {
        const int n = 9;
        const double R = 0.37 * (n - 1), cx = (n - 1) / 2.0 + 0.137, cy = (n - 1) / 2.0 + 0.187, cz = (n - 1) / 2.0 - 0.073;
        std::vector<float> f((size_t)n * n * n);
        for (int k = 0; k < n; ++k) for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i)
            f[((size_t)k * n + j) * n + i] = (float)(R * R - ((i - cx) * (i - cx) + (j - cy) * (j - cy) + (k - cz) * (k - cz)));
        const float o0[3] = {0.f, 0.f, 0.f}, s1[3] = {1.f, 1.f, 1.f};
        const Mesh m = run(f, n, n, n, 0.f, o0, s1);
        CHECK(m.keys.size() == 472 && m.triangles.size() == 3 * 940 && m.nonfinite == 0, "%zu vertices, %zu triangles", m.keys.size(), m.triangles.size() / 3);
        std::map<std::pair<int, int>, int> edges;
        double vol = 0.0;
        for (size_t t = 0; t + 2 < m.triangles.size(); t += 3) {
            const int32_t* v = &m.triangles[t];
            for (int e = 0; e < 3; ++e) ++edges[{v[e], v[(e + 1) % 3]}];
            const float *a = &m.vertices[(size_t)v[0] * 3], *b = &m.vertices[(size_t)v[1] * 3], *c = &m.vertices[(size_t)v[2] * 3];
            vol += ((double)a[0] * ((double)b[1] * c[2] - (double)b[2] * c[1]) - (double)a[1] * ((double)b[0] * c[2] - (double)b[2] * c[0]) +
                    (double)a[2] * ((double)b[0] * c[1] - (double)b[1] * c[0])) / 6.0;
        }
        bool closed = true;
        for (const auto& e : edges) closed = closed && e.second == 1 && edges.count({e.first.second, e.first.first}) == 1;
        const double exact = 4.0 / 3.0 * 3.14159265358979323846 * R * R * R;
        CHECK(closed, "every edge once in each direction");
        CHECK(vol > 0.0 && vol < exact && vol > 0.9 * exact, "volume %.4f of %.4f", vol, exact);
        for (size_t v = 1; v < m.keys.size(); ++v) CHECK(m.keys[v] > m.keys[v - 1], "keys increase at %zu", v);
    }

    if (argc == 3) {
        FILE* in = fopen(argv[1], "rb");
        if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        int32_t dims[3]; float par[7];
        bool good = fread(dims, 4, 3, in) == 3 && fread(par, 4, 7, in) == 7 && mesh_points(dims[0], dims[1], dims[2]) != 0;
        std::vector<float> f(good ? (size_t)mesh_points(dims[0], dims[1], dims[2]) : 0);
        good = good && fread(f.data(), 4, f.size(), in) == f.size();
        fclose(in);
        if (!good) { fprintf(stderr, "malformed volume file\n"); return 2; }
        const Mesh m = run(f, dims[0], dims[1], dims[2], par[0], par + 1, par + 4);
        FILE* out = fopen(argv[2], "wb");
        if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        const int64_t head[3] = {(int64_t)m.keys.size(), (int64_t)m.triangles.size() / 3, m.nonfinite};
        fwrite(head, 8, 3, out);
        fwrite(m.vertices.data(), 4, m.vertices.size(), out);
        fwrite(m.keys.data(), 8, m.keys.size(), out);
        fwrite(m.triangles.data(), 4, m.triangles.size(), out);
        fclose(out);
    }

    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("mesh checks ok\n");
    return 0;
}
