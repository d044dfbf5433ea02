// f3dg_epilogue.h -- the per-pixel arithmetic of the render epilogue (src/gaussian_renderer/__init__.py:881-909 depth_to_normal,
// :1043-1053 world normals) and of its adjoint, shared by the epilogue kernels (f3dg_splat_head.hip) and the fused geometry losses
// (f3dg_geometry_loss.hip): both evaluate normal_world and depth_normal with these very float32 expressions. Compiled with
// -ffp-contract=off like the rest of the library.
#pragma once

namespace {

// inverse of a 4x4 (row-major) by cofactors in float64, rounded to float32 (the camera-to-world matrix of the epilogue: one thread)
__device__ void invert4x4(const float* m_, float* out)
{
    double m[16], inv[16];
    for (int i = 0; i < 16; i++) m[i] = m_[i];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    const double r = 1.0 / det;
    for (int i = 0; i < 16; i++) out[i] = (float)(inv[i] * r);
}

// ---- per-pixel arithmetic shared by epilogue_kernel and epilogue_backward_kernel
// ray(yy, xx) = [xx,yy,1] @ Kinv^T @ R^T with Kinv = [[ax,0,bx],[0,ay,by],[0,0,1]], R = Cw[:3,:3] (Cw row-major 4x4)
__device__ __forceinline__ void epilogue_ray(const float* Cw, float ax, float bx, float ay, float by, int yy, int xx,
                                             float& dx, float& dy, float& dz)
{
    const float cx = xx * ax + bx, cy = yy * ay + by;
    dx = cx * Cw[0] + cy * Cw[1] + Cw[2];
    dy = cx * Cw[4] + cy * Cw[5] + Cw[6];
    dz = cx * Cw[8] + cy * Cw[9] + Cw[10];
}
// point(yy, xx) = depth * ray(yy, xx) + origin
__device__ __forceinline__ void epilogue_point(const float* __restrict__ dep, const float* Cw, int W, float ax, float bx, float ay, float by,
                                               int yy, int xx, float& px, float& py, float& pz)
{
    float dx, dy, dz;
    epilogue_ray(Cw, ax, bx, ay, by, yy, xx, dx, dy, dz);
    const float dd = dep[yy * W + xx];
    px = dd * dx + Cw[3]; py = dd * dy + Cw[7]; pz = dd * dz + Cw[11];
}
// the two difference vectors of the interior pixel (y, x): e = point(y+1, x) - point(y-1, x) ("dx": along rows),
// g = point(y, x+1) - point(y, x-1) ("dy": along columns), and their cross product c = e x g
struct EpilogueCross { float ex, ey, ez, gx, gy, gz, cx, cy, cz; };
__device__ __forceinline__ EpilogueCross epilogue_cross(const float* __restrict__ dep, const float* Cw, int W, float ax, float bx, float ay,
                                                        float by, int y, int x)
{
    float ux, uy, uz, lx, ly, lz, rx, ry, rz, dx_, dy_, dz_;
    epilogue_point(dep, Cw, W, ax, bx, ay, by, y + 1, x, ux, uy, uz);
    epilogue_point(dep, Cw, W, ax, bx, ay, by, y - 1, x, lx, ly, lz);
    epilogue_point(dep, Cw, W, ax, bx, ay, by, y, x + 1, rx, ry, rz);
    epilogue_point(dep, Cw, W, ax, bx, ay, by, y, x - 1, dx_, dy_, dz_);
    EpilogueCross r;
    r.ex = ux - lx; r.ey = uy - ly; r.ez = uz - lz;
    r.gx = rx - dx_; r.gy = ry - dy_; r.gz = rz - dz_;
    r.cx = r.ey * r.gz - r.ez * r.gy; r.cy = r.ez * r.gx - r.ex * r.gz; r.cz = r.ex * r.gy - r.ey * r.gx;
    return r;
}

// Backward of F.normalize(v, eps = 1e-12) for one 3-vector: (g - n^ (n^ . g)) / |v|, or g / 1e-12 where the clamp is active (what
// torch.autograd gives for v / clamp_min(|v|, 1e-12): the clamped norm gets no gradient)
__device__ __forceinline__ void normalize3_backward(float a, float b, float c, float& g0, float& g1, float& g2)
{
    const float raw = sqrtf(a * a + b * b + c * c);
    if (raw >= 1e-12f) {
        const float ha = a / raw, hb = b / raw, hc = c / raw;
        const float dot = ha * g0 + hb * g1 + hc * g2;
        g0 = (g0 - ha * dot) / raw; g1 = (g1 - hb * dot) / raw; g2 = (g2 - hc * dot) / raw;
    } else {
        g0 = g0 / 1e-12f; g1 = g1 / 1e-12f; g2 = g2 / 1e-12f;
    }
}

} // namespace
