// Host-only checks of csrc/eonerf_dual.h (eonerf_dual_check.h), built for the CPU under the address + undefined-behaviour sanitizers
// (tests/host/test_dual_host.py): every refusal in its documented order, the size arithmetic at EONERF_MESH_MAX_POINTS and one beyond,
// the workspace carve, and the rule itself -- the functions the kernels of eonerf_dual.hip call per thread, run here in a loop over the
// points with the workspace's own layout (scans inside tiles of EONERF_MESH_TILE points plus tile offsets).
// No HIP runtime call is made and no device pointer is dereferenced.
//   dual_checks                 the checks
//   dual_checks IN OUT          also contours the volume in IN (int32 nx ny nz, float level origin[3] spacing[3] lambda, int64 G,
//                               float f[nz*ny*nx], float g[G][3]) and writes OUT (int64 H V T nonfinite clamped fallback dropped beyond,
//                               float points[H][3], int64 keys[H], float vertices[V][3], int64 cell_keys[V], int32 triangles[T][3])
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../eonerf_code_amd/csrc/eonerf_dual_check.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const void* const dev = reinterpret_cast<const void*>((uintptr_t)1 << 40);      // never dereferenced: stands for device pointers

struct Dual {
    std::vector<float> points, vertices; std::vector<int64_t> keys, cell_keys; std::vector<int32_t> triangles;
    int64_t nonfinite = 0, clamped = 0, fallback = 0, dropped = 0, beyond = 0;
};

// count + hermite + emit as the kernels do them, one point after the other
static Dual run(const std::vector<float>& f, int nx, int ny, int nz, float level, const float* origin, const float* spacing, float lambda,
                const std::vector<float>& g) {
    const uint64_t n = mesh_points(nx, ny, nz);
    const DualCarve c = dual_carve(n);
    std::vector<uint16_t> lh(n), lc(n), lq(n);
    std::vector<uint8_t> info(n);
    std::vector<uint32_t> l1h(c.n1), l1c(c.n1), l1q(c.n1);
    Dual m;
    uint32_t tile[3] = {0, 0, 0}, all[3] = {0, 0, 0};
    for (uint64_t p = 0; p < n; ++p) {
        if (p % kMeshTile == 0) { l1h[p / kMeshTile] = all[0]; l1c[p / kMeshTile] = all[1]; l1q[p / kMeshTile] = all[2]; tile[0] = tile[1] = tile[2] = 0; }
        const int i = (int)(p % nx), j = (int)(p / nx % ny), k = (int)(p / nx / ny);
        const DualPoint pt = dual_classify(f.data(), nx, ny, nz, i, j, k, (unsigned)p, level);
        lh[p] = (uint16_t)tile[0]; lc[p] = (uint16_t)tile[1]; lq[p] = (uint16_t)tile[2]; info[p] = (uint8_t)dual_info(pt);
        const uint32_t add[3] = {(uint32_t)__builtin_popcount(pt.mask), pt.active, pt.quads};
        for (int s = 0; s < 3; ++s) { tile[s] += add[s]; all[s] += add[s]; }
        m.nonfinite += pt.nonfinite;
    }
    m.points.resize((size_t)all[0] * 3); m.keys.resize(all[0]); m.vertices.resize((size_t)all[1] * 3); m.cell_keys.resize(all[1]);
    m.triangles.resize((size_t)all[2] * 6);
    auto hermite_of = [&](unsigned q, int slot) {
        return (int64_t)(l1h[q / kMeshTile] + lh[q] + (uint32_t)__builtin_popcount(info[q] & ((1u << slot) - 1u)));
    };
    auto vertex_of = [&](unsigned q) { return (int32_t)(l1c[q / kMeshTile] + lc[q]); };
    auto put = [&](uint64_t at, int32_t a, int32_t b, int32_t c3) {
        m.triangles.at(at * 3) = a; m.triangles.at(at * 3 + 1) = b; m.triangles.at(at * 3 + 2) = c3;
    };
    for (uint64_t p = 0; p < n; ++p) {
        const int i = (int)(p % nx), j = (int)(p / nx % ny), k = (int)(p / nx / ny);
        const unsigned mask = info[p] & kDualMask;
        for (int s = 0; s < 3; ++s) {
            if (!((mask >> s) & 1)) continue;
            const int64_t id = hermite_of((unsigned)p, s);
            dual_hermite_point(f.data(), nx, ny, i, j, k, (unsigned)p, s, level, origin, spacing, &m.points.at((size_t)id * 3));
            m.keys.at(id) = (int64_t)p * 8 + s;
        }
        if (info[p] >> kDualQuadShift)
            dual_point_quads(mask, f[p] >= level, nx, ny, nz, i, j, k, (unsigned)p, 2 * ((uint64_t)l1q[p / kMeshTile] + lq[p]), vertex_of, put);
        if (info[p] & kDualActive) {
            const DualVertex v = dual_cell_vertex(f.data(), nx, ny, (unsigned)p, level, spacing, (double)lambda, g.data(), (int64_t)(g.size() / 3), hermite_of);
            m.clamped += v.clamped; m.fallback += v.fallback; m.dropped += v.dropped; m.beyond += v.beyond;
            const int32_t id = vertex_of((unsigned)p);
            dual_vertex_position(v, i, j, k, origin, spacing, &m.vertices.at((size_t)id * 3));
            m.cell_keys.at(id) = (int64_t)p;
        }
    }
    return m;
}

int main(int argc, char** argv) {
    const float nanf_ = nanf(""), inff_ = INFINITY;
    float org[3] = {-1.f, -1.f, -1.f}, sp[3] = {0.125f, 0.125f, 0.25f};

    // ---------------------------------------------------------------- sizes
    const int64_t MAXP = EONERF_MESH_MAX_POINTS;
    {
        const DualCarve c = dual_carve(8);
        CHECK(c.n1 == 1 && c.n2 == 1 && c.lh_off == 0 && c.lc_off == 256 && c.lq_off == 512 && c.info_off == 768 && c.l1_off == 1024 && c.l2_off == 1280 &&
              c.l3_off == 1536 && c.bytes == 1792, "the smallest carve: %zu", c.bytes);
        const DualCarve t1 = dual_carve(kMeshTile), t2 = dual_carve(kMeshTile + 1);
        CHECK(t1.n1 == 1 && t2.n1 == 2 && t2.n2 == 1, "one point beyond a tile");
        const DualCarve s1 = dual_carve((uint64_t)kMeshTile * kMeshTile), s2 = dual_carve((uint64_t)kMeshTile * kMeshTile + 1);
        CHECK(s1.n1 == (uint64_t)kMeshTile && s1.n2 == 1 && s2.n1 == (uint64_t)kMeshTile + 1 && s2.n2 == 2, "one point beyond a tile of tiles");
        const DualCarve m = dual_carve((uint64_t)MAXP);
        CHECK(m.n1 == (uint64_t)MAXP / kMeshTile && m.n2 == (uint64_t)MAXP / kMeshTile / kMeshTile && m.n2 <= (uint64_t)kMeshTile, "the largest call: one third-level sum");
        CHECK(m.lc_off == 2 * (size_t)MAXP && m.lq_off == 4 * (size_t)MAXP && m.info_off == 6 * (size_t)MAXP && m.l1_off == 7 * (size_t)MAXP &&
              m.bytes == 7 * (size_t)MAXP + 16 * m.n1 + 16 * m.n2 + 256, "%zu bytes at the limit (beyond 2^30: computed in 64 bits)", m.bytes);
        CHECK(m.bytes > ((size_t)1 << 30) && 3 * (uint64_t)MAXP <= (uint64_t)INT_MAX && 6 * (uint64_t)MAXP <= (uint64_t)UINT_MAX, "ids and offsets at the limit");
        for (uint64_t n : {(uint64_t)8, (uint64_t)1000, (uint64_t)1025, (uint64_t)5049, (uint64_t)MAXP}) {
            const DualCarve c2 = dual_carve(n);
            CHECK(c2.lh_off % 256 == 0 && c2.lc_off % 256 == 0 && c2.lq_off % 256 == 0 && c2.info_off % 256 == 0 && c2.l1_off % 256 == 0 && c2.l2_off % 256 == 0 &&
                  c2.l3_off % 256 == 0 && c2.lc_off >= c2.lh_off + 2 * n && c2.lq_off >= c2.lc_off + 2 * n && c2.info_off >= c2.lq_off + 2 * n &&
                  c2.l1_off >= c2.info_off + n && c2.l2_off >= c2.l1_off + 16 * c2.n1 && c2.l3_off >= c2.l2_off + 16 * c2.n2 && c2.bytes >= c2.l3_off + 16,
                  "parts aligned and disjoint at %llu points", (unsigned long long)n);
        }
    }
    const size_t need = dual_carve(5049).bytes;

    // ---------------------------------------------------------------- count
    CHECK(dual_check_count(dev, 33, 17, 9, 0.5f, dev, dev, need) == EONERF_OK, "a plain call");
    CHECK(dual_check_count(nullptr, 33, 17, 9, 0.5f, dev, dev, need) == EONERF_E_ARG && dual_check_count(dev, 33, 17, 9, 0.5f, nullptr, dev, need) == EONERF_E_ARG &&
          dual_check_count(dev, 33, 17, 9, 0.5f, dev, nullptr, need) == EONERF_E_ARG, "null pointers");
    CHECK(dual_check_count(dev, 1, 17, 9, 0.5f, dev, dev, need) == EONERF_E_ARG && dual_check_count(dev, 33, 1, 9, 0.5f, dev, dev, need) == EONERF_E_ARG &&
          dual_check_count(dev, 33, 17, 1, 0.5f, dev, dev, need) == EONERF_E_ARG && dual_check_count(dev, -3, 17, 9, 0.5f, dev, dev, need) == EONERF_E_ARG, "a dimension below 2");
    CHECK(dual_check_count(dev, (1 << 14) + 1, 1 << 13, 2, 0.5f, dev, dev, SIZE_MAX) == EONERF_E_UNSUPPORTED, "one row beyond the limit");
    CHECK(dual_check_count(dev, 1 << 14, 1 << 13, 2, 0.5f, dev, dev, dual_carve(MAXP).bytes) == EONERF_OK &&
          dual_check_count(dev, 1 << 14, 1 << 13, 2, 0.5f, dev, dev, dual_carve(MAXP).bytes - 1) == EONERF_E_WORKSPACE, "the limit itself");
    CHECK(dual_check_count(dev, 33, 17, 9, nanf_, dev, dev, need) == EONERF_E_ARG && dual_check_count(dev, 33, 17, 9, -inff_, dev, dev, need) == EONERF_E_ARG, "a level that is not finite");
    CHECK(dual_check_count(dev, 33, 17, 9, 0.5f, dev, dev, need - 1) == EONERF_E_WORKSPACE && dual_check_count(dev, 33, 17, 9, 0.5f, dev, dev, 0) == EONERF_E_WORKSPACE, "a workspace too small");
    CHECK(dual_check_count(nullptr, 1, 17, 9, nanf_, dev, dev, 0) == EONERF_E_ARG, "null first");
    CHECK(dual_check_count(dev, 1, INT_MAX, INT_MAX, nanf_, dev, dev, 0) == EONERF_E_ARG, "dimension before the point count");
    CHECK(dual_check_count(dev, INT_MAX, INT_MAX, INT_MAX, nanf_, dev, dev, 0) == EONERF_E_UNSUPPORTED, "point count before the level");
    CHECK(dual_check_count(dev, 33, 17, 9, nanf_, dev, dev, 0) == EONERF_E_ARG, "level before the workspace");

    // ---------------------------------------------------------------- hermite
    struct Hermite {
        const void *f = dev, *ws = dev, *pts = dev, *st = dev;
        int nx = 33, ny = 17, nz = 9; float level = 0.5f; const float *o, *s; size_t bytes; int64_t cap = 100;
        int run() const { return dual_check_hermite(f, nx, ny, nz, level, o, s, ws, bytes, pts, cap, st); }
    };
    Hermite hok; hok.o = org; hok.s = sp; hok.bytes = need;
    CHECK(hok.run() == EONERF_OK, "a plain call");
    { Hermite e = hok; e.cap = 0; CHECK(e.run() == EONERF_OK, "zero capacity"); }
    { Hermite e = hok; e.f = nullptr; CHECK(e.run() == EONERF_E_ARG, "null f"); e = hok; e.o = nullptr; CHECK(e.run() == EONERF_E_ARG, "null origin");
      e = hok; e.s = nullptr; CHECK(e.run() == EONERF_E_ARG, "null spacing"); e = hok; e.ws = nullptr; CHECK(e.run() == EONERF_E_ARG, "null workspace");
      e = hok; e.pts = nullptr; CHECK(e.run() == EONERF_E_ARG, "null points"); e = hok; e.st = nullptr; CHECK(e.run() == EONERF_E_ARG, "null status"); }
    { Hermite e = hok; e.nx = 1; CHECK(e.run() == EONERF_E_ARG, "nx 1"); e = hok; e.nz = 0; CHECK(e.run() == EONERF_E_ARG, "nz 0"); }
    { Hermite e = hok; e.nx = (1 << 14) + 1; e.ny = 1 << 13; e.nz = 2; e.bytes = SIZE_MAX; CHECK(e.run() == EONERF_E_UNSUPPORTED, "beyond the limit"); }
    { Hermite e = hok; e.level = inff_; CHECK(e.run() == EONERF_E_ARG, "infinite level"); }
    { Hermite e = hok; e.cap = -1; CHECK(e.run() == EONERF_E_ARG, "negative capacity"); }
    { Hermite e = hok; e.bytes = need - 1; CHECK(e.run() == EONERF_E_WORKSPACE, "a workspace too small"); }

    // ---------------------------------------------------------------- emit
    struct Emit {
        const void *f = dev, *g = dev, *ws = dev, *v = dev, *t = dev, *rep = dev, *st = dev;
        int nx = 33, ny = 17, nz = 9; float level = 0.5f, lambda = 0.1f; const float *o, *s; size_t bytes; int64_t n_g = 50, cap_v = 100, cap_t = 200;
        int run() const { return dual_check_emit(f, nx, ny, nz, level, o, s, g, n_g, lambda, ws, bytes, v, cap_v, t, cap_t, rep, st); }
    };
    Emit ok; ok.o = org; ok.s = sp; ok.bytes = need;
    CHECK(ok.run() == EONERF_OK, "a plain call");
    { Emit e = ok; e.cap_v = e.cap_t = e.n_g = 0; CHECK(e.run() == EONERF_OK, "zero capacities"); }
    { Emit e = ok; e.f = nullptr; CHECK(e.run() == EONERF_E_ARG, "null f"); }
    { Emit e = ok; e.o = nullptr; CHECK(e.run() == EONERF_E_ARG, "null origin"); }
    { Emit e = ok; e.s = nullptr; CHECK(e.run() == EONERF_E_ARG, "null spacing"); }
    { Emit e = ok; e.g = nullptr; CHECK(e.run() == EONERF_E_ARG, "null gradient"); }
    { Emit e = ok; e.ws = nullptr; CHECK(e.run() == EONERF_E_ARG, "null workspace"); }
    { Emit e = ok; e.v = nullptr; CHECK(e.run() == EONERF_E_ARG, "null vertices"); }
    { Emit e = ok; e.t = nullptr; CHECK(e.run() == EONERF_E_ARG, "null triangles"); }
    { Emit e = ok; e.rep = nullptr; CHECK(e.run() == EONERF_E_ARG, "null report"); }
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
        bad[k] = -0.25f; CHECK(e.run() == EONERF_OK, "a negative spacing is a spacing %d", k);
    }
    for (float lam : {nanf_, inff_, -0.1f, 0.f, ldexpf(1.f, -10) * 0.999f, 16.001f}) { Emit e = ok; e.lambda = lam; CHECK(e.run() == EONERF_E_ARG, "lambda %g", (double)lam); }
    for (float lam : {ldexpf(1.f, -10), 16.f, 1.f}) { Emit e = ok; e.lambda = lam; CHECK(e.run() == EONERF_OK, "lambda %g", (double)lam); }
    { Emit e = ok; e.cap_v = -1; CHECK(e.run() == EONERF_E_ARG, "negative cap_v"); e = ok; e.cap_t = INT64_MIN; CHECK(e.run() == EONERF_E_ARG, "negative cap_t");
      e = ok; e.n_g = -1; CHECK(e.run() == EONERF_E_ARG, "negative n_gradient"); }
    { Emit e = ok; e.bytes = need - 1; CHECK(e.run() == EONERF_E_WORKSPACE, "a workspace too small"); }
    // the order: each refusal with every later one also present
    float zero_sp[3] = {0.f, 1.f, 1.f};
    { Emit e = ok; e.st = nullptr; e.nx = 1; e.level = nanf_; e.s = zero_sp; e.lambda = 0.f; e.cap_v = -1; e.bytes = 0; CHECK(e.run() == EONERF_E_ARG, "null first");
      e.st = dev; e.ny = e.nz = INT_MAX; CHECK(e.run() == EONERF_E_ARG, "dimension before the point count");
      e.nx = INT_MAX; CHECK(e.run() == EONERF_E_UNSUPPORTED, "point count before the values");
      e.nx = 33; e.ny = 17; e.nz = 9; e.level = 0.5f; e.lambda = 0.1f; e.cap_v = 1; CHECK(e.run() == EONERF_E_ARG, "zero spacing before the workspace");
      e.s = sp; e.lambda = 17.f; CHECK(e.run() == EONERF_E_ARG, "lambda before the workspace");
      e.lambda = 0.1f; e.cap_t = -1; CHECK(e.run() == EONERF_E_ARG, "capacity before the workspace");
      e.cap_t = 0; CHECK(e.run() == EONERF_E_WORKSPACE, "the workspace last"); }

    // ---------------------------------------------------------------- the cell's edges
    for (int e = 0; e < 12; ++e) {
        const int a = e >> 2, corner = dual_edge_corner(e);
        CHECK(!(corner & (1 << a)) && corner < 8, "edge %d starts on the low side of its axis", e);
        for (int e2 = 0; e2 < e; ++e2) CHECK((e2 >> 2) != a || dual_edge_corner(e2) != corner, "edges %d and %d differ", e, e2);
    }
    CHECK(dual_edge_corner(0) == 0 && dual_edge_corner(1) == 2 && dual_edge_corner(2) == 4 && dual_edge_corner(3) == 6 && dual_edge_corner(5) == 1 &&
          dual_edge_corner(6) == 4 && dual_edge_corner(9) == 1 && dual_edge_corner(10) == 2 && dual_edge_corner(11) == 3, "u is the offset on the lower axis");
    CHECK(dual_edge_quad(0, 0, 1, 1, 3, 3, 3) && !dual_edge_quad(0, 1, 0, 1, 3, 3, 3) && !dual_edge_quad(0, 1, 2, 1, 3, 3, 3) && dual_edge_quad(2, 1, 1, 0, 3, 3, 3) &&
          !dual_edge_quad(1, 1, 1, 1, 2, 3, 3), "a quad needs four cells around the edge");

    // ---------------------------------------------------------------- a sphere on 9^3 points: closed, oriented, positive volume
    {
        const int n = 9;
        const double R = 0.37 * (n - 1), cx = (n - 1) / 2.0 + 0.137, cy = (n - 1) / 2.0 + 0.187, cz = (n - 1) / 2.0 - 0.073;
        std::vector<float> f((size_t)n * n * n);
        for (int k = 0; k < n; ++k) for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i)
            f[((size_t)k * n + j) * n + i] = (float)(R - sqrt((i - cx) * (i - cx) + (j - cy) * (j - cy) + (k - cz) * (k - cz)));
        const float o0[3] = {0.f, 0.f, 0.f}, s1[3] = {1.f, 1.f, 1.f};
        const Dual h = run(f, n, n, n, 0.f, o0, s1, 0.1f, std::vector<float>());
        CHECK(h.beyond > 0 && h.dropped == 0, "an empty gradient table: every plane is beyond it");
        std::vector<float> g(h.points.size());
        for (size_t v = 0; v < h.keys.size(); ++v) { g[3 * v] = (float)(cx - h.points[3 * v]); g[3 * v + 1] = (float)(cy - h.points[3 * v + 1]); g[3 * v + 2] = (float)(cz - h.points[3 * v + 2]); }
        const Dual m = run(f, n, n, n, 0.f, o0, s1, 0.1f, g);
        CHECK(m.beyond == 0 && m.dropped == 0 && m.fallback == 0 && m.nonfinite == 0, "every plane used");
        CHECK(m.triangles.size() == 6 * m.keys.size() && m.cell_keys.size() == m.keys.size() + 2, "%zu Hermite points, %zu vertices, %zu triangles: one quad per edge, Euler 2",
              m.keys.size(), m.cell_keys.size(), m.triangles.size() / 3);
        double vol = 0.0, worst = 0.0;
        for (size_t t = 0; t + 2 < m.triangles.size(); t += 3) {
            const int32_t* v = &m.triangles[t];
            const float *a = &m.vertices.at((size_t)v[0] * 3), *b = &m.vertices.at((size_t)v[1] * 3), *c = &m.vertices.at((size_t)v[2] * 3);
            vol += ((double)a[0] * ((double)b[1] * c[2] - (double)b[2] * c[1]) - (double)a[1] * ((double)b[0] * c[2] - (double)b[2] * c[0]) +
                    (double)a[2] * ((double)b[0] * c[1] - (double)b[1] * c[0])) / 6.0;
        }
        for (size_t v = 0; v < m.cell_keys.size(); ++v) {
            const double r = sqrt((m.vertices[3 * v] - cx) * (m.vertices[3 * v] - cx) + (m.vertices[3 * v + 1] - cy) * (m.vertices[3 * v + 1] - cy) +
                                  (m.vertices[3 * v + 2] - cz) * (m.vertices[3 * v + 2] - cz));
            worst = fabs(r - R) > worst ? fabs(r - R) : worst;
        }
        const double exact = 4.0 / 3.0 * 3.14159265358979323846 * R * R * R;
        CHECK(vol > 0.97 * exact && vol < 1.03 * exact && worst < 0.25, "volume %.4f of %.4f, worst radius error %.4f", vol, exact, worst);
        for (size_t v = 1; v < m.keys.size(); ++v) CHECK(m.keys[v] > m.keys[v - 1], "keys increase at %zu", v);
        for (size_t v = 1; v < m.cell_keys.size(); ++v) CHECK(m.cell_keys[v] > m.cell_keys[v - 1], "cell keys increase at %zu", v);
    }

    if (argc == 3) {
        FILE* in = fopen(argv[1], "rb");
        if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        int32_t dims[3]; float par[8]; int64_t rows = 0;
        bool good = fread(dims, 4, 3, in) == 3 && fread(par, 4, 8, in) == 8 && fread(&rows, 8, 1, in) == 1 && mesh_points(dims[0], dims[1], dims[2]) != 0 && rows >= 0 &&
                    rows <= 3 * (int64_t)mesh_points(dims[0], dims[1], dims[2]);
        std::vector<float> f(good ? (size_t)mesh_points(dims[0], dims[1], dims[2]) : 0), g(good ? (size_t)rows * 3 : 0);
        good = good && fread(f.data(), 4, f.size(), in) == f.size() && fread(g.data(), 4, g.size(), in) == g.size();
        fclose(in);
        if (!good) { fprintf(stderr, "malformed volume file\n"); return 2; }
        const Dual m = run(f, dims[0], dims[1], dims[2], par[0], par + 1, par + 4, par[7], g);
        FILE* out = fopen(argv[2], "wb");
        if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        const int64_t head[8] = {(int64_t)m.keys.size(), (int64_t)m.cell_keys.size(), (int64_t)m.triangles.size() / 3, m.nonfinite, m.clamped, m.fallback, m.dropped, m.beyond};
        fwrite(head, 8, 8, out);
        fwrite(m.points.data(), 4, m.points.size(), out);
        fwrite(m.keys.data(), 8, m.keys.size(), out);
        fwrite(m.vertices.data(), 4, m.vertices.size(), out);
        fwrite(m.cell_keys.data(), 8, m.cell_keys.size(), out);
        fwrite(m.triangles.data(), 4, m.triangles.size(), out);
        fclose(out);
    }

    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("dual checks ok\n");
    return 0;
}
