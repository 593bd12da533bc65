// dirt_texture_cube.h -- the per-look-up arithmetic of a cube map (specification: the head of dirt_texture_cube.hip, spec 2-6), for
// the units that look a cube up by a direction: dirt_texture_cube.hip (the look-up itself and its gradient), dirt_shade_ibl.hip
// (image-based lighting, which gathers from two cubes per pixel) and dirt_background.hip (the environment behind the mesh).  One
// copy of the face rule, the index, the taps, the three-channel sample and the direction gradient; and the launch of the backward
// kernels, which the last two use for the scatter alone.
#pragma once
#include "dirt_texture_common.h"

namespace dirt {

int mip_level_count(int Ht, int Wt, int max_level);   // dirt_texture_mip.hip

struct CubeParams {
    const float* pyr;        // [6, face_floats]: a packed pyramid per face (one level: the cube itself)
    const float* dirs;       // n directions (x, y, z), `dir_stride` floats apart
    const float* lod;        // n levels of detail, or nullptr (level 0 only)
    long long n, face_floats;
    int N, Ct, L, dir_stride, gdir_stride;
    float lod_bias;
    unsigned flags;
    float* out;              // [n, Ct]
    const float* grad_out;   // [n, Ct]
    float* grad_pyr;         // [6, face_floats], accumulated into (cleared by the caller of the kernel)
    float* grad_dirs;        // n triples `gdir_stride` apart, or nullptr
    float* grad_lod;         // n, or nullptr
};

// The float offset of the level of size nk in a face's packed pyramid [N x N, ...] x Ct: the levels before it hold
// N^2 (1 + 1/4 + ...) = 4 (N^2 - nk^2) / 3 texels (a level exists only while the one below is even: N = nk 2^k, and 4^k - 1 is a multiple of 3)
__host__ __device__ __forceinline__ long long cube_level_offset(int N, int nk, int Ct)
{
    return ((long long)N * N - (long long)nk * nk) / 3 * 4 * Ct;
}

// the floats of a face's packed pyramid of L levels
__host__ __device__ __forceinline__ long long cube_face_floats(int N, int L, int Ct)
{
    const int top = mip_dim(N, L - 1);
    return cube_level_offset(N, top, Ct) + (long long)top * top * Ct;
}

// spec 2, 3: the face of a direction, (sc, tc) over a, and what the gradient needs to go back
struct CubeLook {
    bool valid, pos;   // pos: the major component is > 0
    int major;         // 0, 1, 2 = x, y, z
    float s, t, a;     // sc / a, tc / a, the magnitude of the major component
    __device__ __forceinline__ int face() const { return 2 * major + (pos ? 0 : 1); }
};
__device__ __forceinline__ CubeLook cube_look(float x, float y, float z)
{
    CubeLook q;
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const bool mx = ax >= ay && ax >= az, my = !mx && ay >= az;
    q.major = mx ? 0 : (my ? 1 : 2);
    q.a = mx ? ax : (my ? ay : az);
    q.pos = (mx ? x : (my ? y : z)) > 0.f;
    q.valid = ax < INFINITY && ay < INFINITY && az < INFINITY && q.a > 0.f;   // (a NaN fails its comparison)
    const float sc = mx ? (q.pos ? -z : z) : (my ? x : (q.pos ? x : -x));
    const float tc = my ? (q.pos ? z : -z) : -y;
    q.s = q.valid ? sc / q.a : 0.f;
    q.t = q.valid ? tc / q.a : 0.f;
    return q;
}

// spec 4: sc / a or tc / a -> the index at a level of size n, and d index / d (sc / a)
__device__ __forceinline__ float cube_index(float s, int n, float& d)
{
    const float x = ((s + 1.f) * 0.5f) * (float)n - 0.5f, top = (float)(n - 1);
    d = x >= 0.f && x <= top ? 0.5f * (float)n : 0.f;
    return x < 0.f ? 0.f : (x > top ? top : x);
}

// the taps of a look-up at a level of size n; 'nearest': one tap of weight 1
__device__ __forceinline__ Taps cube_taps(const CubeLook& q, int n, bool nearest, float& drow, float& dcol)
{
    const float row = cube_index(q.t, n, drow), col = cube_index(q.s, n, dcol);
    Taps k = bilinear_taps(row, col, n, n);
    if (nearest) {
        k.r0 = k.r1 = texel_index(row + 0.5f, n); k.c0 = k.c1 = texel_index(col + 0.5f, n);
        k.fr = 0.f; k.fc = 0.f; k.wr0 = 1.f; k.wc0 = 1.f;
    }
    return k;
}

// dL/d(sc / a), dL/d(tc / a) -> dL/d(x, y, z) (spec 6): sc and tc over a, and a = |major component|
__device__ __forceinline__ void cube_direction_gradient(const CubeLook& q, float gs, float gt, float (&g)[3])
{
    const float g_sc = gs / q.a, g_tc = gt / q.a;
    const float g_a = -((gs * q.s + gt * q.t) / q.a);
    const float g_m = q.pos ? g_a : -g_a;
    if (q.major == 0) { g[0] = g_m; g[1] = -g_tc; g[2] = q.pos ? -g_sc : g_sc; }
    else if (q.major == 1) { g[0] = g_sc; g[1] = g_m; g[2] = q.pos ? g_tc : -g_tc; }
    else { g[0] = q.pos ? g_sc : -g_sc; g[1] = -g_tc; g[2] = g_m; }
}

// a bilinear look-up of three channels and, per channel, its derivative by sc / a and tc / a (0 where the index is clamped):
// what the shaders that look an environment up per pixel gather with (dirt_shade_ibl.hip, dirt_background.hip)
struct CubeSample { float v[3], ds[3], dt[3]; };

// one level [n, n, 3] of a face at the look-up q
template <bool GRAD>
__device__ __forceinline__ void cube_sample(const float* __restrict__ lv, int n, const CubeLook& q, CubeSample& s)
{
    float drow, dcol;
    const Taps k = cube_taps(q, n, false, drow, dcol);
    const Four<size_t> o = tap_offsets(k, n, 3, 0);
    float tl[3], tr[3], bl[3], br[3];
    load3(lv + o.tl, tl); load3(lv + o.tr, tr); load3(lv + o.bl, bl); load3(lv + o.br, br);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        s.v[j] = bilinear_blend(tl[j], tr[j], bl[j], br[j], k);
        if constexpr (GRAD) {
            float e_fr, e_fc;
            tap_gradients(1.f, {tl[j], tr[j], bl[j], br[j]}, k, e_fr, e_fc);
            s.ds[j] = e_fc * dcol; s.dt[j] = e_fr * drow;
        }
    }
}

__device__ __forceinline__ void cube_sample_clear(CubeSample& s)
{
#pragma unroll
    for (int j = 0; j < 3; ++j) { s.v[j] = 0.f; s.ds[j] = 0.f; s.dt[j] = 0.f; }
}

// dirt_texture_cube.hip: clears p.grad_pyr, then launches the backward kernel (the trilinear one where p.lod is there) on the
// tiles of the rows x cols grid of p.n = rows * cols look-ups.  The caller has checked the sizes (check_pixel_grid, the tile
// count) and filled every field of p but `out`; p.grad_dirs / p.grad_lod may be null: the scatter alone.
hipError_t cube_backward_launch(const CubeParams& p, long long rows, long long cols, hipStream_t stream);

}  // namespace dirt
