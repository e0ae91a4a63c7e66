// RPC / UTM code shared by eonerf_raygen.hip (image -> ground), eonerf_prior.hip and eonerf_ortho.hip (ground -> image): the rational
// cubic of the rpcm dict format and the inverse Krueger series on the device, and the WGS84 Krueger-series constants on the host.
#pragma once
#include <math.h>
#include "eonerf_raygen.h"

__device__ __forceinline__ double poly20(const double* p, double x, double y, double z) {   // sat_utils.py:437-450
    double out = 0;
    out += p[0];
    out += p[1] * y + p[2] * x + p[3] * z;
    out += p[4] * y * x + p[5] * y * z + p[6] * x * z;
    out += p[7] * y * y + p[8] * x * x + p[9] * z * z;
    out += p[10] * x * y * z;
    out += p[11] * y * y * y;
    out += p[12] * y * x * x + p[13] * y * z * z + p[14] * y * y * x;
    out += p[15] * x * x * x;
    out += p[16] * x * z * z + p[17] * y * y * z + p[18] * x * x * z;
    out += p[19] * z * z * z;
    return out;
}
__device__ __forceinline__ void project_n(const RpcModel& r, double nlat, double nlon, double nalt, double& x, double& y) {
    x = poly20(r.col_num, nlat, nlon, nalt) / poly20(r.col_den, nlat, nlon, nalt);
    y = poly20(r.row_num, nlat, nlon, nalt) / poly20(r.row_den, nlat, nlon, nalt);
}

// "+proj=utm +zone=<zone> [+south]" on WGS84: Krueger series coefficients (Karney 2011, eq. 35) -- what PROJ's etmerc evaluates
inline UtmParams eo_utm_params(int utm_zone, int south) {
    UtmParams u;
    const double f = 1.0 / 298.257223563, nn = f / (2.0 - f);
    const double n2 = nn * nn, n3 = n2 * nn, n4 = n3 * nn, n5 = n4 * nn, n6 = n5 * nn;
    u.lon0_deg = utm_zone * 6.0 - 183.0;
    u.e = sqrt(f * (2.0 - f));
    u.k0A = 0.9996 * 6378137.0 / (1.0 + nn) * (1.0 + n2 / 4 + n4 / 64 + n6 / 256);
    u.false_north = south ? 10000000.0 : 0.0;
    u.alpha[0] = nn / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800;
    u.alpha[1] = 13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360;
    u.alpha[2] = 61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440;
    u.alpha[3] = 49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600;
    u.alpha[4] = 34729 * n5 / 80640 - 3418889 * n6 / 1995840;
    u.alpha[5] = 212378941 * n6 / 319334400;
    return u;
}

// Krueger series, inverse direction (Karney 2011, eq. 36)
inline void eo_krueger_beta(double beta[6]) {
    const double f = 1.0 / 298.257223563, nn = f / (2.0 - f);
    const double n2 = nn * nn, n3 = n2 * nn, n4 = n3 * nn, n5 = n4 * nn, n6 = n5 * nn;
    beta[0] = nn / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800;
    beta[1] = n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720;
    beta[2] = 17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720;
    beta[3] = 4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600;
    beta[4] = 4583 * n5 / 161280 - 108847 * n6 / 3991680;
    beta[5] = 20648693 * n6 / 638668800;
}

constexpr int kNewton = 5;          // iterations on tan(lat): quadratic convergence from a 0.7 % start, round-off after three

// WGS84 transverse Mercator, inverse 6th-order Krueger series (PROJ etmerc; Karney 2011 eqs. 11, 36 and 19-21).  The including file is
// built with -ffp-contract=off.
__device__ inline void utm_inverse(const UtmParams& u, const double* beta, double east, double north, double& lon_deg, double& lat_deg) {
    const double r2d = 57.29577951308232;
    const double xi = (north - u.false_north) / u.k0A, eta = (east - 500000.0) / u.k0A;
    double xi_p = xi, eta_p = eta;
#pragma unroll
    for (int j = 1; j <= 6; ++j) {
        xi_p -= beta[j - 1] * sin(2 * j * xi) * cosh(2 * j * eta);
        eta_p -= beta[j - 1] * cos(2 * j * xi) * sinh(2 * j * eta);
    }
    const double sh = sinh(eta_p), c = cos(xi_p);
    const double lam = atan2(sh, c);
    const double taup = sin(xi_p) / sqrt(sh * sh + c * c);          // tan of the conformal latitude
    const double e2m = 1.0 - u.e * u.e;
    double tau = taup / e2m;
    for (int k = 0; k < kNewton; ++k) {
        const double tau1 = sqrt(1.0 + tau * tau);
        const double sig = sinh(u.e * atanh(u.e * tau / tau1));
        const double taupa = sqrt(1.0 + sig * sig) * tau - sig * tau1;
        tau += (taup - taupa) * (1.0 + e2m * tau * tau) / (e2m * tau1 * sqrt(1.0 + taupa * taupa));
    }
    lat_deg = atan(tau) * r2d;
    lon_deg = u.lon0_deg + lam * r2d;
}
