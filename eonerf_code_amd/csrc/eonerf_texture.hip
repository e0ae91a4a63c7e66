// Texture baking on the device (eonerf_texture.h): the per-face atlas of a mesh, the ground point of every texel, and the fused
// gather -- the chain of eonerf_ortho.hip (inverse UTM series -> each image's RPC -> bilinear gather -> mean / median) with the loop
// over the K images INSIDE the kernel, so that no K x n x C layer table exists: per sample only the fused colour is written.
// Everything is fp64 (one thread per texel / sample) until the one cast to fp32 of each output.
// Built with -ffp-contract=off: the arithmetic is that of eonerf_ortho.hip, unfused.
// Cost: per sample and image four cubics and two divides in fp64, as k_ortho_gather; k is uniform across the wave, so the RPC, the
// shape, the gain / bias and the view vector of image k are read through uniform addresses (scalar loads), and the per-lane traffic is
// the point, the normal, one occlusion byte per image and the four taps.  The median keeps one sample's values in private memory,
// 64 floats a channel, inserted in ascending k exactly as k_ortho_fuse does.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/eonerf_hip.h"
#include "eonerf_texture.h"
#include "eonerf_texture_check.h"
#include "eonerf_rpc_dev.h"

namespace {

constexpr int kBlock = kTextureBlock;

struct UvArgs {
    int64_t n_faces, cells_per_row, atlas_w, atlas_h; int texels;
    float* uv;
};

__global__ __launch_bounds__(kBlock) void k_texture_uv(UvArgs a) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= a.n_faces) return;
    float* o = a.uv + (size_t)f * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double u, v;
        texture_corner(f, c, a.cells_per_row, a.texels, &u, &v);
        o[2 * c] = (float)(u / (double)a.atlas_w);
        o[2 * c + 1] = (float)(1.0 - v / (double)a.atlas_h);
    }
}

struct SampleArgs {
    const float* vertices; int64_t n_vertices; const int32_t* triangles; int64_t n_faces;
    int64_t cells_per_row, cells, atlas_w; int texels;
    int64_t first, n;
    double scale[3], offset[3];
    UtmParams utm; double beta[6];
    int32_t* face; float* bary; float* xyz; double* lla; float* normal;
};

__global__ __launch_bounds__(kBlock) void k_texture_samples(SampleArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const int64_t t = a.first + i;                                          // < atlas_w * atlas_h (host check)
    double b[3];
    const int64_t face = texture_texel(t % a.atlas_w, t / a.atlas_w, a.cells_per_row, a.cells, a.n_faces, a.texels, b);
    const double nan = __builtin_nan("");
    double p[3] = {nan, nan, nan}, nrm[3] = {nan, nan, nan};
    if (face >= 0) {                                                        // face < n_faces: the index triple is inside the table
        const int32_t* tri = a.triangles + (size_t)face * 3;
        const int64_t ia = tri[0], ib = tri[1], ic = tri[2];
        if (ia >= 0 && ia < a.n_vertices && ib >= 0 && ib < a.n_vertices && ic >= 0 && ic < a.n_vertices) {
            double A[3], B[3], Cc[3];
            bool finite = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                A[k] = (double)a.vertices[(size_t)ia * 3 + k];
                B[k] = (double)a.vertices[(size_t)ib * 3 + k];
                Cc[k] = (double)a.vertices[(size_t)ic * 3 + k];
                finite = finite && isfinite(A[k]) && isfinite(B[k]) && isfinite(Cc[k]);
            }
            if (finite) {
                double e1[3], e2[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    p[k] = (b[0] * A[k] + b[1] * B[k]) + b[2] * Cc[k];
                    e1[k] = (B[k] - A[k]) * a.scale[k];
                    e2[k] = (Cc[k] - A[k]) * a.scale[k];
                }
                const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
                const double len = sqrt((nx * nx + ny * ny) + nz * nz);
                if (len > 0.0 && isfinite(len)) { nrm[0] = nx / len; nrm[1] = ny / len; nrm[2] = nz / len; }
            }
        }
    }
    if (a.face) a.face[i] = (int32_t)face;
    if (a.bary)
        for (int k = 0; k < 3; ++k) a.bary[(size_t)i * 3 + k] = (float)b[k];
    if (a.xyz)
        for (int k = 0; k < 3; ++k) a.xyz[(size_t)i * 3 + k] = (float)p[k];
    if (a.normal)
        for (int k = 0; k < 3; ++k) a.normal[(size_t)i * 3 + k] = (float)nrm[k];
    if (a.lla) {
        double* o = a.lla + (size_t)i * 3;
        if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
            double m[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] = p[k] * a.scale[k] + a.offset[k];
            double lon, lat;
            utm_inverse(a.utm, a.beta, m[0], m[1], lon, lat);
            o[0] = lon; o[1] = lat; o[2] = m[2];
        } else {
            o[0] = o[1] = o[2] = nan;
        }
    }
}

struct BakeArgs {
    const double* __restrict__ lla; const float* __restrict__ normal; int64_t n;
    const RpcModel* __restrict__ rpcs; const uint64_t* __restrict__ pixels; const int32_t* __restrict__ shapes;
    int K, channels;
    const float* __restrict__ gain; const float* __restrict__ bias; const double* __restrict__ sat; const uint8_t* __restrict__ blocked;
    double min_cos; int angle_weight;
    float* colour; float* wsum; int32_t* count; int32_t* best;
};

// Image k at one point: the weight (0: the image does not count) and, where it counts, the C values -- k_ortho_gather's expressions.
template <int C>
__device__ __forceinline__ float bake_image(const BakeArgs& a, int k, int64_t p, double lon, double lat, double alt, bool point_ok, bool has_normal,
                                            double n0, double n1, double n2, float* val) {
    const int h = a.shapes[2 * k], w = a.shapes[2 * k + 1];
    bool ok = point_ok && h >= 1 && w >= 1;
    double gain[C], bias[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        gain[c] = (double)a.gain[(size_t)k * C + c];
        bias[c] = (double)a.bias[(size_t)k * C + c];
        ok = ok && gain[c] != 0.0 && isfinite(gain[c]) && isfinite(bias[c]);
    }
    if (a.blocked) ok = ok && a.blocked[(size_t)k * (size_t)a.n + (size_t)p] == 0;
    float wgt = 1.0f;
    if (has_normal) {
        const double* s = a.sat + (size_t)k * 3;
        const double cosv = (n0 * s[0] + n1 * s[1]) + n2 * s[2];
        ok = ok && cosv >= a.min_cos;                                                                 // NaN fails
        if (a.angle_weight) wgt = (float)cosv;
    }
    if (!ok) return 0.0f;                                                                             // before the cubics: most rejections are cheap
    const RpcModel& r = a.rpcs[k];
    double x, y;
    project_n(r, (lat - r.lat_offset) / r.lat_scale, (lon - r.lon_offset) / r.lon_scale, (alt - r.alt_offset) / r.alt_scale, x, y);
    const double col = x * r.col_scale + r.col_offset, row = y * r.row_scale + r.row_offset;
    ok = col >= 0.0 && col <= (double)(w - 1) && row >= 0.0 && row <= (double)(h - 1);                // NaN fails
    if (!ok) return 0.0f;
    const double fc = floor(col), fr = floor(row);                                                   // only now are the four taps inside the image
    const int c0 = (int)fc, r0 = (int)fr;
    const int c1 = min(c0 + 1, w - 1), r1 = min(r0 + 1, h - 1);
    const double fx = col - fc, fy = row - fr;
    const float* px = (const float*)a.pixels[k];
    const float* p00 = px + ((size_t)r0 * w + c0) * C;
    const float* p01 = px + ((size_t)r0 * w + c1) * C;
    const float* p10 = px + ((size_t)r1 * w + c0) * C;
    const float* p11 = px + ((size_t)r1 * w + c1) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double t00 = (double)p00[c], t01 = (double)p01[c], t10 = (double)p10[c], t11 = (double)p11[c];
        ok = ok && isfinite(t00) && isfinite(t01) && isfinite(t10) && isfinite(t11);
        const double s = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t01) + fy * ((1.0 - fx) * t10 + fx * t11);
        val[c] = (float)((s - bias[c]) / gain[c]);
    }
    return (ok && wgt > 0.0f) ? wgt : 0.0f;
}

template <int C, int MODE>
__global__ __launch_bounds__(kBlock) void k_texture_bake(BakeArgs a) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    const double lon = a.lla[(size_t)p * 3], lat = a.lla[(size_t)p * 3 + 1], alt = a.lla[(size_t)p * 3 + 2];
    const bool point_ok = isfinite(lon) && isfinite(lat) && isfinite(alt);
    const bool has_normal = a.normal != nullptr;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (has_normal) { n0 = (double)a.normal[(size_t)p * 3]; n1 = (double)a.normal[(size_t)p * 3 + 1]; n2 = (double)a.normal[(size_t)p * 3 + 2]; }

    int m = 0, best = -1;
    float best_w = 0.0f;
    double ws = 0.0;
    double acc[C];
    float best_v[C];
    float s[MODE == EONERF_TEXTURE_MEDIAN ? C * EONERF_TEXTURE_MAX_MEDIAN : 1];     // kept sorted per channel; K <= 64 (host check)
#pragma unroll
    for (int c = 0; c < C; ++c) { acc[c] = 0.0; best_v[c] = 0.0f; }
    for (int k = 0; k < a.K; ++k) {                                                // ascending k: the sums' order is fixed
        float val[C];
        const float w = bake_image<C>(a, k, p, lon, lat, alt, point_ok, has_normal, n0, n1, n2, val);
        if (!(w > 0.0f)) continue;
        ws += (double)w;
        if (w > best_w) {                                                          // strictly: ties stay with the smaller k
            best_w = w; best = k;
#pragma unroll
            for (int c = 0; c < C; ++c) best_v[c] = val[c];
        }
        if (MODE == EONERF_TEXTURE_MEAN) {
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (double)w * (double)val[c];
        } else if (MODE == EONERF_TEXTURE_MEDIAN) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float* sc = s + c * EONERF_TEXTURE_MAX_MEDIAN;
                int j = m;                                                         // m < K <= 64: sc[j] stays inside the channel's 64
                while (j > 0 && sc[j - 1] > val[c]) { sc[j] = sc[j - 1]; --j; }
                sc[j] = val[c];
            }
        }
        ++m;
    }
    if (a.count) a.count[p] = m;
    if (a.wsum) a.wsum[p] = (float)ws;
    if (a.best) a.best[p] = best;
    if (!a.colour) return;
    float* out = a.colour + (size_t)p * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float v = __builtin_nanf("");
        if (m > 0) {
            if (MODE == EONERF_TEXTURE_MEAN) v = (float)(acc[c] / ws);
            else if (MODE == EONERF_TEXTURE_MEDIAN) {
                const float* sc = s + c * EONERF_TEXTURE_MAX_MEDIAN;
                v = (float)(0.5 * ((double)sc[(m - 1) / 2] + (double)sc[m / 2]));  // numpy's median
            } else v = best_v[c];
        }
        out[c] = v;
    }
}

template <int C>
void launch_bake(const BakeArgs& a, int mode, hipStream_t st) {
    const dim3 grid(texture_blocks(a.n)), block(kBlock);
    if (mode == EONERF_TEXTURE_MEAN) hipLaunchKernelGGL((k_texture_bake<C, EONERF_TEXTURE_MEAN>), grid, block, 0, st, a);
    else if (mode == EONERF_TEXTURE_MEDIAN) hipLaunchKernelGGL((k_texture_bake<C, EONERF_TEXTURE_MEDIAN>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_texture_bake<C, EONERF_TEXTURE_BEST>), grid, block, 0, st, a);
}

}  // namespace

extern "C" {

int eonerf_texture_version(void) { return EONERF_TEXTURE_VERSION; }

int eonerf_texture_layout(int64_t n_faces, int texels, int64_t out[3]) {
    if (!out) return EONERF_E_ARG;
    TextureLayout l;
    const int rc = texture_layout(n_faces, texels, &l);
    if (rc != EONERF_OK) return rc;
    out[0] = l.atlas_w; out[1] = l.atlas_h; out[2] = l.cells_per_row;
    return EONERF_OK;
}

int eonerf_texture_uv(int64_t n_faces, int texels, void* uv_out, void* stream) {
    TextureLayout l;
    const int rc = texture_check_uv(n_faces, texels, uv_out, &l);
    if (rc != EONERF_OK || n_faces == 0) return rc;
    UvArgs a;
    a.n_faces = n_faces; a.cells_per_row = l.cells_per_row; a.atlas_w = l.atlas_w; a.atlas_h = l.atlas_h; a.texels = texels;
    a.uv = (float*)uv_out;
    hipLaunchKernelGGL(k_texture_uv, dim3(texture_blocks(n_faces)), dim3(kBlock), 0, (hipStream_t)stream, a);      // n_faces <= 2^31: one grid
    return (int)hipGetLastError();
}

int eonerf_texture_samples(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_faces, int texels, int64_t first, int64_t n,
                           const float scene_scale[3], const float scene_offset[3], int utm_zone, int south, void* face_out, void* bary_out,
                           void* xyz_out, void* lonlatalt_out, void* normal_out, void* stream) {
    TextureLayout l;
    const int rc = texture_check_samples(vertices, n_vertices, triangles, n_faces, texels, first, n, scene_scale, scene_offset, utm_zone, face_out,
                                         bary_out, xyz_out, lonlatalt_out, normal_out, &l);
    if (rc != EONERF_OK || n == 0) return rc;
    SampleArgs a;
    a.vertices = (const float*)vertices; a.n_vertices = n_vertices; a.triangles = (const int32_t*)triangles; a.n_faces = n_faces;
    a.cells_per_row = l.cells_per_row; a.cells = l.cells; a.atlas_w = l.atlas_w; a.texels = texels;
    a.first = first; a.n = n;
    for (int k = 0; k < 3; ++k) { a.scale[k] = (double)scene_scale[k]; a.offset[k] = (double)scene_offset[k]; }
    a.utm = eo_utm_params(utm_zone, south);
    eo_krueger_beta(a.beta);
    a.face = (int32_t*)face_out; a.bary = (float*)bary_out; a.xyz = (float*)xyz_out; a.lla = (double*)lonlatalt_out; a.normal = (float*)normal_out;
    hipLaunchKernelGGL(k_texture_samples, dim3(texture_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int eonerf_texture_bake(const void* lonlatalt, const void* normal, int64_t n, const void* rpcs, const void* pixel_addresses, const void* shapes,
                        int K, int channels, const void* gain, const void* bias, const void* to_satellite, const void* blocked, float min_cos,
                        int angle_weight, int mode, void* colour_out, void* weight_sum_out, void* count_out, void* best_out, void* stream) {
    const int rc = texture_check_bake(lonlatalt, normal, n, rpcs, pixel_addresses, shapes, K, channels, gain, bias, to_satellite, min_cos,
                                      angle_weight, mode, colour_out, weight_sum_out, count_out, best_out);
    if (rc != EONERF_OK || n == 0) return rc;
    static_assert(sizeof(eonerf_rpc) == sizeof(RpcModel), "RPC struct mismatch");
    BakeArgs a;
    a.lla = (const double*)lonlatalt; a.normal = (const float*)normal; a.n = n;
    a.rpcs = (const RpcModel*)rpcs; a.pixels = (const uint64_t*)pixel_addresses; a.shapes = (const int32_t*)shapes;
    a.K = K; a.channels = channels;
    a.gain = (const float*)gain; a.bias = (const float*)bias; a.sat = (const double*)to_satellite; a.blocked = (const uint8_t*)blocked;
    a.min_cos = (double)min_cos; a.angle_weight = angle_weight;
    a.colour = (float*)colour_out; a.wsum = (float*)weight_sum_out; a.count = (int32_t*)count_out; a.best = (int32_t*)best_out;
    const hipStream_t st = (hipStream_t)stream;
    switch (channels) {
        case 1: launch_bake<1>(a, mode, st); break;
        case 2: launch_bake<2>(a, mode, st); break;
        case 3: launch_bake<3>(a, mode, st); break;
        default: launch_bake<4>(a, mode, st); break;
    }
    return (int)hipGetLastError();
}

}  // extern "C"
