// f3dg_mesh_project.h -- the one projection of a mesh vertex under a world_view that the mesh rasteriser (f3dg_mesh_raster.hip) and the
// vertex colour baking (f3dg_mesh_bake.hip) share: the baking tests a vertex against the z-buffer the rasteriser wrote, so both must
// form x, y, z, u, v to the bit. float64 on float32 inputs, the operation order of include/f3dg.h, no contraction (build.py).
#pragma once
#include "f3dg_common.h"

__device__ __forceinline__ bool f3dg_mesh_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }       // (false for a NaN)

// (X, Y, Z) under the row-major 4 x 4 matrix m (row-vector convention; M is float in global memory or double in a widened table):
// camera space x, y, z and the pixel coordinates u, v (pixel centres at integers; half_w = (double)W / 2). Returns true when the point
// is NEAR / NON-FINITE: a non-finite x, y, z, u or v, or not (z > z_near).
template <typename M>
__device__ __forceinline__ bool f3dg_mesh_project(double X, double Y, double Z, const M* m, double fx, double fy, double half_w,
                                                  double half_h, double z_near, double& x, double& y, double& z, double& u, double& v)
{
    x = ((X * (double)m[0] + Y * (double)m[4]) + Z * (double)m[8]) + (double)m[12];
    y = ((X * (double)m[1] + Y * (double)m[5]) + Z * (double)m[9]) + (double)m[13];
    z = ((X * (double)m[2] + Y * (double)m[6]) + Z * (double)m[10]) + (double)m[14];
    u = ((fx * x) / z + half_w) - 0.5;
    v = ((fy * y) / z + half_h) - 0.5;
    return !f3dg_mesh_finite(x) || !f3dg_mesh_finite(y) || !f3dg_mesh_finite(z) || !(z > z_near) || !f3dg_mesh_finite(u) || !f3dg_mesh_finite(v);
}
