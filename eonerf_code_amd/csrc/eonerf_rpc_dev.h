// RPC / UTM code shared by eonerf_raygen.hip (image -> ground) and eonerf_prior.hip (ground -> image): the rational cubic of the
// rpcm dict format on the device, and the WGS84 Krueger-series constants on the host.
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
