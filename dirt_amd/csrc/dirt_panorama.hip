// dirt_panorama.hip -- lat-long (equirectangular) environment maps, fused: a panorama resampled into a cube and a cube into a
// panorama, both supersampled, differentiable, and under an optional rotation that is differentiable too.
//
// The head of the environment chain: every other stage takes the environment as a cube [6, N, N, C]; captured environments come
// as panoramas [Hp, Wp, C].  The specification (DESIGN.md §7k restates it; dirt_amd/texture.py::panorama_to_cube_dense and
// cube_to_panorama_dense are its readable forms, which tests/panorama_reference.py restates in float64), one float32 operation
// per step, with K2 = float(1 / (2 pi)), K1 = float(1 / pi), PI = float(pi), PI2 = float(2 pi):
//
//  1. The panorama's row 0 is +Y (up), its middle column looks along -Z, its columns grow towards +X.  The look-up L(d) of a
//     direction d, valid as a cube look-up's (all finite, not all zero; otherwise 0 and no gradient), is that of
//     (x, y, z) = d 2^-e, e = frexp(max |d_i|)'s exponent: the largest component in [0.5, 1), exactly, a subnormal one included,
//     so that rho2 neither overflows nor underflows whatever the length of d.  The gradient of d is that of (x, y, z) times 2^-e.
//       rho2 = x x + z z    rho = sqrt(rho2)    theta = atan2(rho, y)    phi = atan2(x, -z), 0 where rho == 0
//       u = phi K2 + 0.5    v = theta K1        col = u Wp - 0.5         row = clamp(v Hp - 0.5, 0, Hp - 1)
//       columns wrap: taps at floor(col) mod Wp and that + 1 mod Wp, weight fc = col - floor(col);
//       rows clamp:   taps at r0 = floor(row) and min(r0 + 1, Hp - 1), weight fr = row - r0;   L = bilinear_blend of the four.
//     d phi / d d = (-z, 0, x) / rho2,  d theta / d d = (x y / rho, -rho, z y / rho) / (rho2 + y y), both 0 where rho == 0;
//     d row = 0 where v Hp - 0.5 lies outside [0, Hp - 1].
//  2. The inverse map, sub-sample (a, b) of S x S of pixel (i, j) of an H x W panorama:
//       v = (i + (a + 0.5) / S) / H     u = (j + (b + 0.5) / S) / W     theta = PI v     phi = PI2 (u - 0.5)
//       d = (sin theta sin phi, cos theta, -(sin theta cos phi))
//  3. Sub-sample (a, b) of cube texel (f, r, c): tc = (2 (r + (a + 0.5) / S)) / N - 1, sc likewise from c and b; its direction e
//     (not normalised) by the table of cube_texel_directions.
//  4. The rotation R [3, 3], row vectors: its rows are the images of the panorama's axes in the cube's frame.
//     panorama_to_cube looks up L(p), p_k = (e_0 R[k][0] + e_1 R[k][1]) + e_2 R[k][2];
//     cube_to_panorama looks the cube up (bilinear, dirt_texture_cube.h) at q, q_k = (d_0 R[0][k] + d_1 R[1][k]) + d_2 R[2][k].
//  5. Both outputs: the S^2 samples added in (a, b) row-major order from 0, then times float(1 / S^2).
//
// Kernels.  panorama_to_cube_forward_kernel<S, CT>: one lane per cube texel on the 16 x 16 tiles of a face, the face in
// blockIdx.y, R wave-uniform.  panorama_to_cube_backward_kernel<S, CT>: one workgroup per tile, the forward again with the
// derivative of each sample by its index; d rotation's nine sums by wave_sum -> fold_waves_to_row -> a row per workgroup in
// caller-owned scratch -> shade_launch_reduce, in a fixed order (no float atomics); d panorama a scatter with float atomics,
// through the LDS patch of dirt_texture_common.h where the bounding box of the tile's taps fits it, straight to memory where it
// does not (a tile on the wrap seam, around a pole, heavy minification).  cube_to_panorama_forward_kernel<S, CT>: one lane per
// panorama pixel, the samples' directions made in registers.  cube_to_panorama_backward_kernel<S, CT>: d rotation likewise
// (cube_direction_gradient), and per sample the looked-up direction and grad_out / S^2 left in scratch, which the entry point
// hands to cube_backward_launch on the (H S) x (W S) grid of samples for the scatter into the cube.
// CT: the channels as registers (1, 3, 4), or 0 = any count, one channel per pass.  What is not asked for is a NULL pointer and
// a workgroup-uniform branch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_shade_common.h"
#include "dirt_texture_cube.h"

namespace dirt {

constexpr int PANO_BLOCK = 256;        // lanes of a workgroup, texels / pixels of a tile
constexpr int PANO_ROT = 9;            // the sums of a workgroup: d rotation
constexpr float PANO_K2 = 0.15915494309189535f, PANO_K1 = 0.3183098861837907f;   // 1 / (2 pi), 1 / pi
constexpr float PANO_PI = 3.14159265358979f, PANO_PI2 = 6.28318530717959f;

struct PanoParams {
    const float* src;        // panorama_to_cube: the panorama [Hp, Wp, Ct]; cube_to_panorama: the cube [6, N, N, Ct]
    const float* rot;        // [3, 3]
    float* out;              // the cube / the panorama
    const float* gout;       // like out
    float* gsrc;             // panorama_to_cube: d panorama (cleared by the entry point), or nullptr
    float* part;             // [workgroups, 9], or nullptr
    float* s_dir;            // cube_to_panorama: [H S, W S, 3] the samples' looked-up directions; these two or nullptr
    float* s_g;              // ... and [H S, W S, Ct] what arrives at each sample
    int Hp, Wp, N, Ct;
};

// one pixel / texel of NV channels (4: 16 bytes at 4-byte alignment, 3: 12, 1: 4)
template <int NV> __device__ __forceinline__ void pano_load(const float* __restrict__ p, float (&v)[NV])
{
    if constexpr (NV == 4) { const Float4 q = *reinterpret_cast<const Float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else if constexpr (NV == 3) load3(p, v);
    else v[0] = p[0];
}
template <int NV> __device__ __forceinline__ void pano_store(float* __restrict__ p, const float (&v)[NV])
{
    if constexpr (NV == 4) *reinterpret_cast<Float4*>(p) = Float4{v[0], v[1], v[2], v[3]};
    else if constexpr (NV == 3) store3(p, v);
    else p[0] = v[0];
}

// spec 3: the face coordinate of sub-sample a of texel r
template <int S> __device__ __forceinline__ float pano_face_coordinate(int r, int a, int N)
{
    return (2.f * ((float)r + ((float)a + 0.5f) / (float)S)) / (float)N - 1.f;
}

// ... and the direction of (sc, tc) on face f (wave-uniform)
__device__ __forceinline__ void pano_face_direction(int f, float sc, float tc, float (&e)[3])
{
    if (f == 0) { e[0] = 1.f; e[1] = -tc; e[2] = -sc; }
    else if (f == 1) { e[0] = -1.f; e[1] = -tc; e[2] = sc; }
    else if (f == 2) { e[0] = sc; e[1] = 1.f; e[2] = tc; }
    else if (f == 3) { e[0] = sc; e[1] = -1.f; e[2] = -tc; }
    else if (f == 4) { e[0] = sc; e[1] = -tc; e[2] = 1.f; }
    else { e[0] = -sc; e[1] = -tc; e[2] = -1.f; }
}

// spec 2: the direction of sub-sample (a, b) of pixel (r, c)
template <int S> __device__ __forceinline__ void pano_pixel_direction(int r, int c, int a, int b, int H, int W, float (&d)[3])
{
    const float v = ((float)r + ((float)a + 0.5f) / (float)S) / (float)H, u = ((float)c + ((float)b + 0.5f) / (float)S) / (float)W;
    const float theta = PANO_PI * v, phi = PANO_PI2 * (u - 0.5f);
    const float st = sinf(theta);
    d[0] = st * sinf(phi); d[1] = cosf(theta); d[2] = -(st * cosf(phi));
}

// spec 1: the taps of a direction, and what the gradient needs to go back
struct PanoLook {
    bool valid, inside;   // inside: the row is not clamped
    Taps k;
    float x, y, z, rho, rho2;   // of the direction times 2^-e
    int e;
};
__device__ __forceinline__ PanoLook pano_look(float x, float y, float z, int Hp, int Wp)
{
    PanoLook q;
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const float big = fmaxf(ax, fmaxf(ay, az));
    q.valid = ax < INFINITY && ay < INFINITY && az < INFINITY && big > 0.f;   // (a NaN fails its comparison)
    q.e = 0;
    if (q.valid) (void)frexpf(big, &q.e);   // big 2^-e lies in [0.5, 1); ldexpf is exact here, for a subnormal `big` too
    q.x = q.valid ? ldexpf(x, -q.e) : 0.f; q.y = q.valid ? ldexpf(y, -q.e) : 1.f; q.z = q.valid ? ldexpf(z, -q.e) : 0.f;
    q.rho2 = q.x * q.x + q.z * q.z;
    q.rho = sqrtf(q.rho2);
    const float theta = atan2f(q.rho, q.y), phi = q.rho == 0.f ? 0.f : atan2f(q.x, -q.z);
    const float u = phi * PANO_K2 + 0.5f, v = theta * PANO_K1;
    const float col = u * (float)Wp - 0.5f, rowu = v * (float)Hp - 0.5f, top = (float)(Hp - 1);
    q.inside = rowu >= 0.f && rowu <= top;
    const float row = rowu < 0.f ? 0.f : (rowu > top ? top : rowu);
    const float fr0 = floorf(row), fc0 = floorf(col);
    q.k.fr = row - fr0; q.k.fc = col - fc0;
    q.k.wr0 = 1.f - q.k.fr; q.k.wc0 = 1.f - q.k.fc;
    q.k.r0 = min(max((int)fr0, 0), Hp - 1); q.k.r1 = min(q.k.r0 + 1, Hp - 1);
    int c0 = (int)fc0;                      // -1 .. Wp - 1 (u lies in [0, 1]); one wrap either way, then held inside whatever rounding did
    c0 = c0 < 0 ? c0 + Wp : (c0 >= Wp ? c0 - Wp : c0);
    q.k.c0 = min(max(c0, 0), Wp - 1);
    q.k.c1 = q.k.c0 + 1 >= Wp ? 0 : q.k.c0 + 1;
    return q;
}

// (g_row, g_col) = dL / d (row, col) of a look-up -> dL / d d: that of the scaled direction, times 2^-e
__device__ __forceinline__ void pano_direction_gradient(const PanoLook& q, float g_row, float g_col, int Hp, int Wp, float (&g)[3])
{
    const float gphi = g_col * ((float)Wp * PANO_K2), gth = q.inside ? g_row * ((float)Hp * PANO_K1) : 0.f;
    const bool pole = !q.valid || q.rho == 0.f;
    const float rho2 = pole ? 1.f : q.rho2, rho = pole ? 1.f : q.rho;
    const float a = gphi / rho2, b = gth / (rho2 + q.y * q.y);
    g[0] = pole ? 0.f : ldexpf(a * -q.z + b * ((q.x * q.y) / rho), -q.e);
    g[1] = pole ? 0.f : ldexpf(b * -rho, -q.e);
    g[2] = pole ? 0.f : ldexpf(a * q.x + b * ((q.z * q.y) / rho), -q.e);
}

// the bounding box of tap sets whose columns wrap (c1 may be 0 beside c0 = Wp - 1)
__device__ __forceinline__ void pano_box_add(int* box, const Taps& k)
{
    atomicMin(&box[0], k.r0); atomicMax(&box[1], k.r1);
    atomicMin(&box[2], min(k.c0, k.c1)); atomicMax(&box[3], max(k.c0, k.c1));
}

// ---- panorama -> cube, forward: one lane per cube texel; R is wave-uniform (scalar loads)
template <int S, int CT>
__global__ __launch_bounds__(PANO_BLOCK) void panorama_to_cube_forward_kernel(PanoParams P, int tw, int th, int tiles_x)
{
    constexpr int NV = CT ? CT : 1;
    long long i;
    if (!tile_pixel<int>(threadIdx.x, tw, th, tiles_x, P.N, P.N, i)) return;
    const int r = (int)(i / P.N), c = (int)(i - (long long)r * P.N), f = blockIdx.y;
    const int Ct = CT ? CT : P.Ct;
    const float* __restrict__ R = P.rot;
    float* __restrict__ out = P.out + ((size_t)f * P.N * P.N + (size_t)i) * Ct;
    constexpr float inv = 1.f / (float)(S * S);
    for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) {
        float acc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = 0.f;
#pragma unroll
        for (int a = 0; a < S; ++a) {
            const float tc = pano_face_coordinate<S>(r, a, P.N);
#pragma unroll
            for (int b = 0; b < S; ++b) {
                float e[3], p[3];
                pano_face_direction(f, pano_face_coordinate<S>(c, b, P.N), tc, e);
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = (e[0] * R[3 * k] + e[1] * R[3 * k + 1]) + e[2] * R[3 * k + 2];
                const PanoLook q = pano_look(p[0], p[1], p[2], P.Hp, P.Wp);
                const Four<size_t> o = tap_offsets(q.k, P.Wp, Ct, ch);
                float tl[NV], tr[NV], bl[NV], br[NV];
                pano_load<NV>(P.src + o.tl, tl); pano_load<NV>(P.src + o.tr, tr); pano_load<NV>(P.src + o.bl, bl); pano_load<NV>(P.src + o.br, br);
#pragma unroll
                for (int j = 0; j < NV; ++j) acc[j] += q.valid ? bilinear_blend(tl[j], tr[j], bl[j], br[j], q.k) : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] *= inv;
        pano_store<NV>(out + ch, acc);
    }
}

// ---- panorama -> cube, backward: one workgroup per tile of a face
template <int S, int CT>
__global__ __launch_bounds__(PANO_BLOCK) void panorama_to_cube_backward_kernel(PanoParams P, int tw, int th, int tiles_x)
{
    constexpr int NV = CT ? CT : 1;
    __shared__ float s_acc[TEX_PATCH * NV];
    __shared__ int s_box[4];
    __shared__ float s_part[4 * PANO_ROT];
    const int tid = threadIdx.x;
    long long i;
    const bool active = tile_pixel<int>(tid, tw, th, tiles_x, P.N, P.N, i);
    const int r = (int)(i / P.N), c = (int)(i - (long long)r * P.N), f = blockIdx.y;
    const int Ct = CT ? CT : P.Ct;
    const float* __restrict__ R = P.rot;
    const float* __restrict__ gout = P.gout + ((size_t)f * P.N * P.N + (size_t)i) * Ct;
    constexpr float inv = 1.f / (float)(S * S);

    // the look-up of sub-sample (a, b) of this lane's texel, and its direction before the rotation
    auto look = [&](int a, int b, float (&e)[3]) {
        float p[3];
        pano_face_direction(f, pano_face_coordinate<S>(c, b, P.N), pano_face_coordinate<S>(r, a, P.N), e);
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = (e[0] * R[3 * k] + e[1] * R[3 * k + 1]) + e[2] * R[3 * k + 2];
        return pano_look(p[0], p[1], p[2], P.Hp, P.Wp);
    };

    bool patch = false;
    int rmin = 0, cmin = 0, bh = 0, bw = 0;
    if (P.gsrc) {   // (uniform) the bounding box of every tap of the tile
        if (tid == 0) box_clear(s_box);
        __syncthreads();
        if (active) {
#pragma unroll
            for (int a = 0; a < S; ++a)
#pragma unroll
                for (int b = 0; b < S; ++b) {
                    float e[3];
                    const PanoLook q = look(a, b, e);
                    if (q.valid) pano_box_add(s_box, q.k);
                }
        }
        __syncthreads();
        rmin = s_box[0]; cmin = s_box[2];
        bh = s_box[1] - rmin + 1; bw = s_box[3] - cmin + 1;
        patch = bh > 0 && bw > 0 && (long long)bh * bw <= TEX_PATCH;   // (workgroup-uniform; no valid look-up: no patch)
    }
    float dR[PANO_ROT];
#pragma unroll
    for (int k = 0; k < PANO_ROT; ++k) dR[k] = 0.f;
    for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) {
        if (patch) {
            clear_patch(s_acc, bh * bw * NV, tid);
            __syncthreads();
        }
        if (active) {
            float g[NV];
            pano_load<NV>(gout + ch, g);
#pragma unroll
            for (int j = 0; j < NV; ++j) g[j] *= inv;
#pragma unroll
            for (int a = 0; a < S; ++a)
#pragma unroll
                for (int b = 0; b < S; ++b) {
                    float e[3];
                    const PanoLook q = look(a, b, e);
                    if (!q.valid) continue;
                    const Four<size_t> o = tap_offsets(q.k, P.Wp, Ct, ch);
                    if (P.part) {   // (uniform)
                        float tl[NV], tr[NV], bl[NV], br[NV];
                        pano_load<NV>(P.src + o.tl, tl); pano_load<NV>(P.src + o.tr, tr); pano_load<NV>(P.src + o.bl, bl); pano_load<NV>(P.src + o.br, br);
                        float g_row = 0.f, g_col = 0.f;
#pragma unroll
                        for (int j = 0; j < NV; ++j) {
                            float e_fr, e_fc;
                            tap_gradients(g[j], {tl[j], tr[j], bl[j], br[j]}, q.k, e_fr, e_fc);
                            g_row += e_fr; g_col += e_fc;
                        }
                        float gp[3];
                        pano_direction_gradient(q, g_row, g_col, P.Hp, P.Wp, gp);
#pragma unroll
                        for (int k = 0; k < 3; ++k)
#pragma unroll
                            for (int j = 0; j < 3; ++j) dR[3 * k + j] += gp[k] * e[j];
                    }
                    if (P.gsrc) {   // (uniform)
                        const Four<float> w = {q.k.wc0 * q.k.wr0, q.k.fc * q.k.wr0, q.k.wc0 * q.k.fr, q.k.fc * q.k.fr};
                        if (patch) {
                            const Four<int> l = patch_offsets(q.k, rmin, cmin, bw, NV);
#pragma unroll
                            for (int j = 0; j < NV; ++j) add_taps(s_acc, l, j, g[j], w);
                        } else {
#pragma unroll
                            for (int j = 0; j < NV; ++j) add_taps(P.gsrc, o, j, g[j], w);
                        }
                    }
                }
        }
        if (patch) {
            __syncthreads();
            for (int t = tid; t < bh * bw * NV; t += PANO_BLOCK) {   // (as texture_backward_kernel's)
                const float val = s_acc[t];
                const int j = t % NV, texel = t / NV;
                if (val != 0.f) atomicAdd(&P.gsrc[box_texel(texel, rmin, cmin, bw, P.Wp, Ct) + ch + j], val);
            }
            __syncthreads();
        }
    }
    if (P.part) {   // (uniform)
        const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int k = 0; k < PANO_ROT; ++k) {
            const float s = wave_sum(dR[k]);
            if (lane == 0) s_part[wave * PANO_ROT + k] = s;
        }
        __syncthreads();
        if (tid < PANO_ROT) fold_waves_to_row<PANO_ROT>(s_part, P.part, tid);
    }
}

// the look-up of sub-sample (a, b) of panorama pixel (r, c): its direction, that direction in the cube's frame, the face
template <int S>
__device__ __forceinline__ CubeLook cube_to_panorama_look(const PanoParams& P, const float* __restrict__ R, int r, int c, int a, int b,
                                                          float (&d)[3], float (&q)[3])
{
    pano_pixel_direction<S>(r, c, a, b, P.Hp, P.Wp, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = (d[0] * R[k] + d[1] * R[3 + k]) + d[2] * R[6 + k];
    return cube_look(q[0], q[1], q[2]);
}

// ---- cube -> panorama, forward: one lane per panorama pixel
template <int S, int CT>
__global__ __launch_bounds__(PANO_BLOCK) void cube_to_panorama_forward_kernel(PanoParams P, int tw, int th, int tiles_x)
{
    constexpr int NV = CT ? CT : 1;
    long long i;
    if (!tile_pixel<int>(threadIdx.x, tw, th, tiles_x, P.Hp, P.Wp, i)) return;
    const int r = (int)(i / P.Wp), c = (int)(i - (long long)r * P.Wp);
    const int Ct = CT ? CT : P.Ct;
    const float* __restrict__ R = P.rot;
    const size_t face_floats = (size_t)P.N * P.N * Ct;
    float* __restrict__ out = P.out + (size_t)i * Ct;
    constexpr float inv = 1.f / (float)(S * S);
    for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) {
        float acc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = 0.f;
#pragma unroll
        for (int a = 0; a < S; ++a)
#pragma unroll
            for (int b = 0; b < S; ++b) {
                float d[3], q3[3];
                const CubeLook q = cube_to_panorama_look<S>(P, R, r, c, a, b, d, q3);
                float drow, dcol;
                const Taps k = cube_taps(q, P.N, false, drow, dcol);
                const float* __restrict__ face = P.src + (size_t)q.face() * face_floats;
                const Four<size_t> o = tap_offsets(k, P.N, Ct, ch);
                float tl[NV], tr[NV], bl[NV], br[NV];
                pano_load<NV>(face + o.tl, tl); pano_load<NV>(face + o.tr, tr); pano_load<NV>(face + o.bl, bl); pano_load<NV>(face + o.br, br);
#pragma unroll
                for (int j = 0; j < NV; ++j) acc[j] += q.valid ? bilinear_blend(tl[j], tr[j], bl[j], br[j], k) : 0.f;
            }
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] *= inv;
        pano_store<NV>(out + ch, acc);
    }
}

// ---- cube -> panorama, backward: one workgroup per tile of the panorama
template <int S, int CT>
__global__ __launch_bounds__(PANO_BLOCK) void cube_to_panorama_backward_kernel(PanoParams P, int tw, int th, int tiles_x)
{
    constexpr int NV = CT ? CT : 1;
    __shared__ float s_part[4 * PANO_ROT];
    const int tid = threadIdx.x;
    long long i;
    const bool active = tile_pixel<int>(tid, tw, th, tiles_x, P.Hp, P.Wp, i);
    const int r = (int)(i / P.Wp), c = (int)(i - (long long)r * P.Wp);
    const int Ct = CT ? CT : P.Ct;
    const float* __restrict__ R = P.rot;
    const size_t face_floats = (size_t)P.N * P.N * Ct;
    const float* __restrict__ gout = P.gout + (size_t)i * Ct;
    constexpr float inv = 1.f / (float)(S * S);
    float dR[PANO_ROT];
#pragma unroll
    for (int k = 0; k < PANO_ROT; ++k) dR[k] = 0.f;
    for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) {
        if (!active) break;
        float g[NV];
        pano_load<NV>(gout + ch, g);
#pragma unroll
        for (int j = 0; j < NV; ++j) g[j] *= inv;
#pragma unroll
        for (int a = 0; a < S; ++a)
#pragma unroll
            for (int b = 0; b < S; ++b) {
                float d[3], q3[3];
                const CubeLook q = cube_to_panorama_look<S>(P, R, r, c, a, b, d, q3);
                if (P.s_dir) {   // (uniform) what the scatter reads: an all-zero direction adds nothing
                    const size_t smp = ((size_t)r * S + a) * ((size_t)P.Wp * S) + ((size_t)c * S + b);
                    if (ch == 0) {
                        float z[3];
#pragma unroll
                        for (int j = 0; j < 3; ++j) z[j] = q.valid ? q3[j] : 0.f;
                        store3(P.s_dir + smp * 3, z);
                    }
                    pano_store<NV>(P.s_g + smp * Ct + ch, g);
                }
                if (P.part && q.valid) {   // (the pointer: uniform)
                    float drow, dcol;
                    const Taps k = cube_taps(q, P.N, false, drow, dcol);
                    const float* __restrict__ face = P.src + (size_t)q.face() * face_floats;
                    const Four<size_t> o = tap_offsets(k, P.N, Ct, ch);
                    float tl[NV], tr[NV], bl[NV], br[NV];
                    pano_load<NV>(face + o.tl, tl); pano_load<NV>(face + o.tr, tr); pano_load<NV>(face + o.bl, bl); pano_load<NV>(face + o.br, br);
                    float d_fr = 0.f, d_fc = 0.f;
#pragma unroll
                    for (int j = 0; j < NV; ++j) {
                        float e_fr, e_fc;
                        tap_gradients(g[j], {tl[j], tr[j], bl[j], br[j]}, k, e_fr, e_fc);
                        d_fr += e_fr; d_fc += e_fc;
                    }
                    float gq[3];
                    cube_direction_gradient(q, d_fc * dcol, d_fr * drow, gq);
#pragma unroll
                    for (int j = 0; j < 3; ++j)
#pragma unroll
                        for (int k2 = 0; k2 < 3; ++k2) dR[3 * j + k2] += d[j] * gq[k2];
                }
            }
    }
    if (P.part) {   // (uniform)
        const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int k = 0; k < PANO_ROT; ++k) {
            const float s = wave_sum(dR[k]);
            if (lane == 0) s_part[wave * PANO_ROT + k] = s;
        }
        __syncthreads();
        if (tid < PANO_ROT) fold_waves_to_row<PANO_ROT>(s_part, P.part, tid);
    }
}

// f(S, CT as integral constants) for the instantiation of `samples` and `channels`
template <class F> inline void pano_dispatch(int samples, int channels, F&& f)
{
    dispatch_channels(channels, true, [&](auto ct) {
        if (samples == 1) f(std::integral_constant<int, 1>{}, ct);
        else if (samples == 2) f(std::integral_constant<int, 2>{}, ct);
        else if (samples == 3) f(std::integral_constant<int, 3>{}, ct);
        else f(std::integral_constant<int, 4>{}, ct);
    });
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_texture_error;   // the error channel of this file's entry points

constexpr long long PANO_MAX_SIDE = 1ll << 20;   // rows and columns of a panorama

// the tiles of a rows x cols grid of lanes; 0 for a grid a launch cannot address
static long long pano_tiles(long long rows, long long cols)
{
    const dirt::TileGrid t = dirt::tile_grid(rows, cols);
    return t.tiles > 0x7fffffffll ? 0 : t.tiles;
}

// what every entry point refuses, before any device work; fills what they share of P
static int panorama_check(const char* who, long long rows, long long cols, int size, int channels, int samples, bool to_cube, dirt::PanoParams& P)
{
    if (rows < 1 || cols < 1 || size < 1 || channels < 1)
        TEX_FAIL("%s: bad sizes (rows=%lld cols=%lld size=%d channels=%d), each at least 1", who, rows, cols, size, channels);
    if (samples < 1 || samples > DIRT_PANORAMA_MAX_SAMPLES) TEX_FAIL("%s: samples=%d, 1..%d", who, samples, DIRT_PANORAMA_MAX_SAMPLES);
    if (size > 32768) TEX_FAIL("%s: cube size %d, at most 32768", who, size);
    if (rows > PANO_MAX_SIDE || cols > PANO_MAX_SIDE) TEX_FAIL("%s: panorama of %lld x %lld, at most %lld each way", who, rows, cols, PANO_MAX_SIDE);
    if (channels > 65536) TEX_FAIL("%s: %d channels, at most 65536", who, channels);
    if (!to_cube && (pano_tiles(rows, cols) == 0 || pano_tiles(rows * samples, cols * samples) == 0))
        TEX_FAIL("%s: grid too large (rows=%lld cols=%lld samples=%d): more than 2^31 - 1 tiles", who, rows, cols, samples);
    P.Hp = (int)rows; P.Wp = (int)cols; P.N = size; P.Ct = channels;
    return DIRT_OK;
}

// the floats of the partial rows at the head of the scratch
static long long pano_partial_floats(long long rows, long long cols, int size, int to_cube)
{
    return (to_cube ? 6 * pano_tiles(size, size) : pano_tiles(rows, cols)) * dirt::PANO_ROT;
}

size_t dirt_panorama_scratch_bytes(long long rows, long long cols, int size, int channels, int samples, int to_cube)
{
    if (rows < 1 || cols < 1 || size < 1 || channels < 1 || samples < 1 || samples > DIRT_PANORAMA_MAX_SAMPLES || size > 32768 || rows > PANO_MAX_SIDE ||
        cols > PANO_MAX_SIDE || channels > 65536)
        return 0;
    if (!to_cube && (pano_tiles(rows, cols) == 0 || pano_tiles(rows * samples, cols * samples) == 0)) return 0;
    long long floats = pano_partial_floats(rows, cols, size, to_cube);
    if (!to_cube) floats += rows * samples * cols * samples * (3 + (long long)channels);
    return sizeof(float) * (size_t)floats;
}

int dirt_panorama_to_cube_forward(const float* panorama, const float* rotation, float* cube, long long rows, long long cols, int size, int channels,
                                  int samples, void* stream)
{
    const char* who = "dirt_panorama_to_cube_forward";
    dirt::PanoParams P{};
    if (int rc = panorama_check(who, rows, cols, size, channels, samples, true, P)) return rc;
    if (!panorama || !rotation || !cube) TEX_FAIL("%s: panorama / rotation / cube is NULL", who);
    P.src = panorama; P.rot = rotation; P.out = cube;
    const dirt::TileGrid t = dirt::tile_grid(size, size);
    dirt::pano_dispatch(samples, channels, [&](auto s, auto ct) {
        hipLaunchKernelGGL((dirt::panorama_to_cube_forward_kernel<decltype(s)::value, decltype(ct)::value>), dim3((unsigned)t.tiles, 6u),
                           dim3(dirt::PANO_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), P, t.tw, t.th, (int)t.tiles_x);
    });
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_panorama_to_cube_backward(const float* panorama, const float* rotation, const float* grad_cube, float* grad_panorama, float* grad_rotation,
                                   void* scratch, size_t scratch_bytes, long long rows, long long cols, int size, int channels, int samples,
                                   void* stream)
{
    const char* who = "dirt_panorama_to_cube_backward";
    dirt::PanoParams P{};
    if (int rc = panorama_check(who, rows, cols, size, channels, samples, true, P)) return rc;
    if (!grad_panorama && !grad_rotation) return dirt::stage_ok(report);
    if (!panorama || !rotation || !grad_cube) TEX_FAIL("%s: panorama / rotation / grad_cube is NULL", who);
    if (grad_rotation)
        if (int rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_panorama_scratch_bytes(rows, cols, size, channels, samples, 1),
                                         "dirt_panorama_scratch_bytes"))
            return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    P.src = panorama; P.rot = rotation; P.gout = grad_cube; P.gsrc = grad_panorama;
    P.part = grad_rotation ? static_cast<float*>(scratch) : nullptr;
    hipError_t e = grad_panorama ? dirt::clear_floats(grad_panorama, rows * cols * channels, s) : hipSuccess;
    const dirt::TileGrid t = dirt::tile_grid(size, size);
    if (e == hipSuccess) {
        dirt::pano_dispatch(samples, channels, [&](auto sm, auto ct) {
            hipLaunchKernelGGL((dirt::panorama_to_cube_backward_kernel<decltype(sm)::value, decltype(ct)::value>), dim3((unsigned)t.tiles, 6u),
                               dim3(dirt::PANO_BLOCK), 0, s, P, t.tw, t.th, (int)t.tiles_x);
        });
        e = hipGetLastError();
    }
    if (e == hipSuccess && grad_rotation) {
        dirt::shade_launch_reduce(P.part, grad_rotation, 6 * t.tiles, dirt::PANO_ROT, 1, s);
        e = hipGetLastError();
    }
    return dirt::stage_hip(report, who, e);
}

int dirt_cube_to_panorama_forward(const float* cube, const float* rotation, float* panorama, long long rows, long long cols, int size, int channels,
                                  int samples, void* stream)
{
    const char* who = "dirt_cube_to_panorama_forward";
    dirt::PanoParams P{};
    if (int rc = panorama_check(who, rows, cols, size, channels, samples, false, P)) return rc;
    if (!cube || !rotation || !panorama) TEX_FAIL("%s: cube / rotation / panorama is NULL", who);
    P.src = cube; P.rot = rotation; P.out = panorama;
    const dirt::TileGrid t = dirt::tile_grid(rows, cols);
    dirt::pano_dispatch(samples, channels, [&](auto s, auto ct) {
        hipLaunchKernelGGL((dirt::cube_to_panorama_forward_kernel<decltype(s)::value, decltype(ct)::value>), dim3((unsigned)t.tiles),
                           dim3(dirt::PANO_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), P, t.tw, t.th, (int)t.tiles_x);
    });
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_cube_to_panorama_backward(const float* cube, const float* rotation, const float* grad_panorama, float* grad_cube, float* grad_rotation,
                                   void* scratch, size_t scratch_bytes, long long rows, long long cols, int size, int channels, int samples,
                                   void* stream)
{
    const char* who = "dirt_cube_to_panorama_backward";
    dirt::PanoParams P{};
    if (int rc = panorama_check(who, rows, cols, size, channels, samples, false, P)) return rc;
    if (!grad_cube && !grad_rotation) return dirt::stage_ok(report);
    if (!cube || !rotation || !grad_panorama) TEX_FAIL("%s: cube / rotation / grad_panorama is NULL", who);
    if (int rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_panorama_scratch_bytes(rows, cols, size, channels, samples, 0),
                                     "dirt_panorama_scratch_bytes"))
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long grid_rows = rows * samples, grid_cols = cols * samples, n = grid_rows * grid_cols;
    float* const base = static_cast<float*>(scratch);
    P.src = cube; P.rot = rotation; P.gout = grad_panorama;
    P.part = grad_rotation ? base : nullptr;
    if (grad_cube) {
        P.s_dir = base + pano_partial_floats(rows, cols, size, 0);
        P.s_g = P.s_dir + 3 * n;
    }
    const dirt::TileGrid t = dirt::tile_grid(rows, cols);
    dirt::pano_dispatch(samples, channels, [&](auto sm, auto ct) {
        hipLaunchKernelGGL((dirt::cube_to_panorama_backward_kernel<decltype(sm)::value, decltype(ct)::value>), dim3((unsigned)t.tiles),
                           dim3(dirt::PANO_BLOCK), 0, s, P, t.tw, t.th, (int)t.tiles_x);
    });
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && grad_rotation) {
        dirt::shade_launch_reduce(P.part, grad_rotation, t.tiles, dirt::PANO_ROT, 1, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess && grad_cube) {   // the scatter, by the cube look-up's backward kernel (no gradient to a direction)
        dirt::CubeParams c{};
        c.n = n; c.Ct = channels; c.gdir_stride = 3; c.lod_bias = 0.f; c.flags = 0;
        c.pyr = cube; c.dirs = P.s_dir; c.dir_stride = 3; c.lod = nullptr;
        c.N = size; c.L = 1; c.face_floats = (long long)size * size * channels; c.grad_out = P.s_g; c.grad_pyr = grad_cube;
        e = dirt::cube_backward_launch(c, grid_rows, grid_cols, s);
    }
    return dirt::stage_hip(report, who, e);
}

}  // extern "C"
