/* osmt_project.h — Point::from_node on the device, shared by k_project (osmt_kernels.hip) and the node labels of
 * osmt_tilelabels.hip: one function, so a label anchor and a display-list point of the same node never differ.
 * Compiled with -ffp-contract=off like everything that includes it. */
#ifndef OSMT_PROJECT_H
#define OSMT_PROJECT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/osmtile.h"

namespace {

constexpr double PI = 3.14159265358979323846264338327950288;

/* Rust `f64 as i32` (saturating, NaN -> 0) */
__device__ __forceinline__ int32_t f64_as_i32(double v) {
    if (v != v) return 0;
    if (v >= 2147483647.0) return INT32_MAX;
    if (v <= -2147483648.0) return INT32_MIN;
    return (int32_t)v;
}

/* tile.rs:88-106 + point.rs:11-19 */
__device__ __forceinline__ void project_point(double lat, double lon, uint32_t zoom, uint32_t tx, uint32_t ty,
                                              double scale, int32_t* ox, int32_t* oy) {
    const double lat_rad = lat * (PI / 180.0);
    const double lon_rad = lon * (PI / 180.0);
    const double x = lon_rad + PI;
    const double y = PI - log(tan((PI / 4.0) + (lat_rad / 2.0)));
    const double dim = (double)(OSMT_TILE_SIZE * (1u << zoom));
    const double px = (x / (2.0 * PI)) * dim;
    const double py = (y / (2.0 * PI)) * dim;
    const double rx = px - (double)(uint32_t)(tx * OSMT_TILE_SIZE);
    const double ry = py - (double)(uint32_t)(ty * OSMT_TILE_SIZE);
    *ox = f64_as_i32(round(rx * scale));
    *oy = f64_as_i32(round(ry * scale));
}

}  // namespace

#endif
