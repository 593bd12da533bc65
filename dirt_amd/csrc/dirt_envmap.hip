// dirt_envmap.hip -- the convolution of one level of a cube map with a lobe on the sphere (a GGX lobe of a given roughness, or the
// clamped cosine), and its transpose: what turns the box pyramid of an environment cube into the prefiltered pyramid of split-sum
// image-based lighting, and a cube into its irradiance.
//
// Replaces no reference interface (the reference has no environment maps).  The specification (DESIGN.md §7 restates it;
// tests/envmap_reference.py implements it in numpy float64):
//
//  1. Texel direction.  Face f, row r, column c of an n x n face: sc = 2 (c + 0.5) / n - 1, tc = 2 (r + 0.5) / n - 1; the
//     unnormalised direction is the inverse of the (sc, tc) table of dirt_texture_cube.hip (spec 3 there):
//     +X (1, -tc, -sc), -X (-1, -tc, sc), +Y (sc, 1, tc), -Y (sc, -1, -tc), +Z (sc, -tc, 1), -Z (-sc, -tc, -1); d is that vector
//     normalised, and the texel's solid angle, up to a constant, W = (1 + sc^2 + tc^2)^(-3/2).
//  2. Weight of a pair, t = d_o . d_s, t+ = max(t, 0).  Lambert: k = t+.  GGX, alpha = roughness^2: q(t) = 1 / (1 + t+^2 (alpha^2 - 1))^2,
//     q_c = q(1) / 256 if 16 alpha^2 < 1 (reached at t_c^2 = (1 - 16 alpha^2) / (1 - alpha^2)), else q_c = 0 (t_c = 0);
//     k = t+ max(q(t) - q_c, 0): continuous, and exactly 0 for t <= t_c.
//  3. Forward, source and output on the same grid: Z_o = sum_s k(t_os) W_s, out[o, c] = sum_s k(t_os) W_s S[s, c] / Z_o.
//  4. Transposed: grad_S[s, c] = W_s sum_o k(t_os) grad_out[o, c] / Z_o.
//
// One kernel for both: a workgroup of 256 lanes owns a 16 x 16 tile of one face, each lane one texel with its direction and its
// running sums in registers, and walks the 16 x 16 tiles of all six faces in a fixed order.  A tile whose every texel is at
// least the cut-off angle acos(t_c) from every texel of the workgroup's is dropped by a test on the two tiles' bounding cones,
// taken by 64 lanes for 64 tiles at a time (a ballot: wave-uniform, and the same in all four waves).  A live tile is staged in
// LDS -- direction, W, channels; transposed: grad_out / Z -- and every lane reads the same staged texel (a broadcast read).
// What the kernel computes is q alpha^4 (q(1) = 1, q_c = 1 / 256: the factor cancels in 3), from 1 - t^2 = e (1 - e / 4) with
// e = |d_o - d_s|^2: taken from t, 1 + t^2 (alpha^2 - 1) would cancel to nothing at alpha = 1 / 1024.  A tile's terms are summed
// on their own, then added to the running sums: partial sums of at most 256 + (tiles) terms.  Every output is written once, by its
// own lane, and nothing is added to memory: a fixed order, the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "dirt_stage.h"

namespace dirt {

constexpr int ENV_TILE = 16;                 // a tile is ENV_TILE x ENV_TILE texels, one per lane
constexpr float ENV_CULL_MARGIN = 1e-4f;     // radians the cone test stays on the safe side by (its float32 error is ~1e-6)

struct EnvmapParams {
    const float* src;     // the level inside face 0; transposed: grad_dst
    const float* norm;    // transposed: [6, n, n] as the forward wrote it
    float* dst;           // the level inside face 0; transposed: grad_src
    float* norm_out;      // forward: [6, n, n]
    long long face_stride;
    int n, Ct, tiles_x;   // tiles along a face's side
    float alpha2;         // GGX: alpha^2
    float q_cut;          // GGX: q_c alpha^4 (1 / 256 or 0)
    float cut_angle;      // acos(t_c)
};

// spec 1: the unnormalised direction of the point (sc, tc) of face f
__device__ __forceinline__ void envmap_face_point(int f, float sc, float tc, float (&v)[3])
{
    switch (f) {
    case 0: v[0] = 1.f; v[1] = -tc; v[2] = -sc; break;
    case 1: v[0] = -1.f; v[1] = -tc; v[2] = sc; break;
    case 2: v[0] = sc; v[1] = 1.f; v[2] = tc; break;
    case 3: v[0] = sc; v[1] = -1.f; v[2] = -tc; break;
    case 4: v[0] = sc; v[1] = -tc; v[2] = 1.f; break;
    default: v[0] = -sc; v[1] = -tc; v[2] = -1.f; break;
    }
}

// spec 1: the direction of the centre of texel (r, c) of face f, and its solid-angle weight
__device__ __forceinline__ void envmap_texel(int f, float r, float c, int n, float (&d)[3], float& w)
{
    const float sc = 2.f * (c + 0.5f) / (float)n - 1.f, tc = 2.f * (r + 0.5f) / (float)n - 1.f;
    float v[3];
    envmap_face_point(f, sc, tc, v);
    const float inv = 1.f / sqrtf((1.f + sc * sc) + tc * tc);
    d[0] = v[0] * inv; d[1] = v[1] * inv; d[2] = v[2] * inv;
    w = (inv * inv) * inv;
}

// the angle between two unit vectors, accurate near 0 (acos of the dot product is not)
__device__ __forceinline__ float envmap_angle(const float (&a)[3], const float (&b)[3])
{
    float x[3];
    cross3(a, b, x);
    return atan2f(sqrtf(dot3(x, x)), dot3(a, b));
}

// the bounding cone of the texel centres of tile (ty, tx) of face f: the axis through the middle of their rectangle and the
// largest angle from it to a corner (a cone of less than a right angle cuts the face's plane in a convex region, so a rectangle
// whose corners are inside is inside)
__device__ __forceinline__ float envmap_tile_cone(int f, int ty, int tx, int n, float (&axis)[3])
{
    const float r0 = (float)(ty * ENV_TILE), c0 = (float)(tx * ENV_TILE);
    const float r1 = (float)(min(ty * ENV_TILE + ENV_TILE, n) - 1), c1 = (float)(min(tx * ENV_TILE + ENV_TILE, n) - 1);
    float w;
    envmap_texel(f, 0.5f * (r0 + r1), 0.5f * (c0 + c1), n, axis, w);
    float half = 0.f, d[3];
    envmap_texel(f, r0, c0, n, d, w); half = fmaxf(half, envmap_angle(axis, d));
    envmap_texel(f, r0, c1, n, d, w); half = fmaxf(half, envmap_angle(axis, d));
    envmap_texel(f, r1, c0, n, d, w); half = fmaxf(half, envmap_angle(axis, d));
    envmap_texel(f, r1, c1, n, d, w); half = fmaxf(half, envmap_angle(axis, d));
    return half;
}

// spec 2, scaled by alpha^4 for GGX, of a pair of unit vectors
template <unsigned KIND>
__device__ __forceinline__ float envmap_weight(const float (&a)[3], float bx, float by, float bz, float alpha2, float q_cut)
{
    const float x = a[0] - bx, y = a[1] - by, z = a[2] - bz;
    const float e = fmaf(z, z, fmaf(y, y, x * x));      // |a - b|^2 = 2 - 2 t
    const float t = fmaxf(fmaf(-0.5f, e, 1.f), 0.f);
    if (KIND == DIRT_ENVMAP_LAMBERT) return t;
    const float rest = t > 0.f ? e * fmaf(-0.25f, e, 1.f) : 1.f;       // 1 - t+^2 (an antipodal pair, e = 4: 1, not 0)
    const float den = fmaf(alpha2, t * t, rest);                       // 1 + t+^2 (alpha^2 - 1) >= alpha^2 > 0
    const float r = alpha2 * __builtin_amdgcn_rcpf(den);
    return t * fmaxf(fmaf(r, r, -q_cut), 0.f);
}

// CT channels per pass: 1, 3, 4, or 0 = any count in passes of four
template <int CT, unsigned KIND, bool TRANSPOSED>
__global__ __launch_bounds__(256) void envmap_filter_kernel(EnvmapParams p)
{
    constexpr int NV = CT ? CT : 4;
    constexpr int LS = CT == 1 ? 1 : 4;                // floats of LDS per staged texel's channels (three: padded to a 16-byte read)
    __shared__ __attribute__((aligned(16))) Float4 s_dir[ENV_TILE * ENV_TILE];      // direction, W
    __shared__ __attribute__((aligned(16))) float s_val[ENV_TILE * ENV_TILE * LS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = p.n, Ct = CT ? CT : p.Ct, tiles_x = p.tiles_x, per_face = tiles_x * tiles_x;
    const int face = blockIdx.y, ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x % tiles_x;
    const int lr = tid / ENV_TILE, lc = tid % ENV_TILE;
    const int row = ty * ENV_TILE + lr, col = tx * ENV_TILE + lc;
    const bool active = row < n && col < n;
    float d[3], w_own;
    envmap_texel(face, (float)row, (float)col, n, d, w_own);
    float own_axis[3];
    const float own_half = envmap_tile_cone(face, ty, tx, n, own_axis);
    const size_t own = (size_t)face * p.face_stride + ((size_t)row * n + col) * Ct;

    for (int c0 = 0; c0 < Ct; c0 += NV) {
        const int nc = CT ? CT : min(NV, Ct - c0);
        float total[NV + 1];                            // the channels' sums, then Z
#pragma unroll
        for (int j = 0; j <= NV; ++j) total[j] = 0.f;
        for (int base = 0; base < 6 * per_face; base += 64) {
            // lane l: is tile base + l within the cut-off angle of this workgroup's?
            const int cand = base + lane;
            bool live = false;
            if (cand < 6 * per_face) {
                const int f = cand / per_face, t = cand % per_face;
                float axis[3];
                const float half = envmap_tile_cone(f, t / tiles_x, t % tiles_x, n, axis);
                live = envmap_angle(own_axis, axis) - own_half - half - ENV_CULL_MARGIN < p.cut_angle;
            }
            unsigned long long todo = __ballot(live);
            while (todo) {
                const int tile = base + __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int sf = tile / per_face, st = tile % per_face;
                const int sr0 = (st / tiles_x) * ENV_TILE, sc0 = (st % tiles_x) * ENV_TILE;
                const int rh = min(ENV_TILE, n - sr0), cw = min(ENV_TILE, n - sc0);
                __syncthreads();                        // the previous tile has been read
                if (lr < rh && lc < cw) {
                    float sd[3], sw;
                    envmap_texel(sf, (float)(sr0 + lr), (float)(sc0 + lc), n, sd, sw);
                    const size_t texel = (size_t)(sr0 + lr) * n + (sc0 + lc);
                    const float* __restrict__ v = p.src + (size_t)sf * p.face_stride + texel * Ct + c0;
                    float scale = 1.f;
                    if (TRANSPOSED) scale = 1.f / p.norm[(size_t)sf * n * n + texel];
                    s_dir[tid] = Float4{sd[0], sd[1], sd[2], sw};
#pragma unroll
                    for (int j = 0; j < NV; ++j) s_val[tid * LS + j] = j < nc ? (TRANSPOSED ? v[j] * scale : v[j]) : 0.f;
                }
                __syncthreads();
                float part[NV + 1];
#pragma unroll
                for (int j = 0; j <= NV; ++j) part[j] = 0.f;
                for (int r = 0; r < rh; ++r) {
                    for (int c = 0; c < cw; ++c) {
                        const int s = r * ENV_TILE + c;
                        const Float4 g = s_dir[s];
                        float k = envmap_weight<KIND>(d, g.x, g.y, g.z, p.alpha2, p.q_cut);
                        if (!TRANSPOSED) { k *= g.w; part[NV] += k; }
#pragma unroll
                        for (int j = 0; j < NV; ++j) part[j] = fmaf(k, s_val[s * LS + j], part[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j <= NV; ++j) total[j] += part[j];
            }
        }
        if (active) {
            const float scale = TRANSPOSED ? w_own : 1.f / total[NV];   // (a texel sees itself: Z > 0)
            for (int j = 0; j < nc; ++j) p.dst[own + c0 + j] = total[j] * scale;
            if (!TRANSPOSED && c0 == 0) p.norm_out[(size_t)face * n * n + (size_t)row * n + col] = total[NV];
        }
    }
}

}  // namespace dirt

static constexpr dirt::ErrorSetter report = dirt::set_texture_error;   // the error channel of this file's entry points

// what both entry points refuse, before any device work; fills `p` but its pointers
static int envmap_check(const char* who, int size, int channels, long long face_stride, float alpha, unsigned kind, dirt::EnvmapParams& p)
{
    if (size < 1 || channels < 1) TEX_FAIL("%s: bad sizes (size=%d channels=%d)", who, size, channels);
    if (size > 16384) TEX_FAIL("%s: size %d, at most 16384", who, size);
    if (face_stride < (long long)size * size * channels)
        TEX_FAIL("%s: face_stride %lld is less than a level (%d x %d x %d)", who, face_stride, size, size, channels);
    if (kind != DIRT_ENVMAP_GGX && kind != DIRT_ENVMAP_LAMBERT) TEX_FAIL("%s: kind %u is neither DIRT_ENVMAP_GGX nor DIRT_ENVMAP_LAMBERT", who, kind);
    if (kind == DIRT_ENVMAP_GGX && !(alpha > 0.f && alpha <= 1.f)) TEX_FAIL("%s: alpha %g is outside (0, 1]", who, (double)alpha);
    p.n = size; p.Ct = channels; p.face_stride = face_stride; p.tiles_x = (size + dirt::ENV_TILE - 1) / dirt::ENV_TILE;
    const double a2 = (double)alpha * (double)alpha;
    const bool cut = kind == DIRT_ENVMAP_GGX && 16.0 * a2 < 1.0;
    p.alpha2 = (float)a2;
    p.q_cut = cut ? 1.f / 256.f : 0.f;
    p.cut_angle = cut ? (float)acos(sqrt((1.0 - 16.0 * a2) / (1.0 - a2))) : 1.57079637f;
    return DIRT_OK;
}

template <bool TRANSPOSED>
static int envmap_launch(const char* who, const dirt::EnvmapParams& p, unsigned kind, void* stream)
{
    const dim3 grid((unsigned)(p.tiles_x * p.tiles_x), 6);
    dirt::dispatch_channels(p.Ct, true, [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        if (kind == DIRT_ENVMAP_GGX)
            hipLaunchKernelGGL((dirt::envmap_filter_kernel<CT, DIRT_ENVMAP_GGX, TRANSPOSED>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
        else
            hipLaunchKernelGGL((dirt::envmap_filter_kernel<CT, DIRT_ENVMAP_LAMBERT, TRANSPOSED>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
    });
    return dirt::stage_hip(report, who, hipGetLastError());
}

extern "C" {

int dirt_envmap_filter_forward(const float* src, float* dst, float* norm, int size, int channels, long long face_stride, float alpha,
                               unsigned kind, void* stream)
{
    const char* who = "dirt_envmap_filter_forward";
    dirt::EnvmapParams p{};
    const int rc = envmap_check(who, size, channels, face_stride, alpha, kind, p);
    if (rc) return rc;
    if (!src || !dst || !norm) TEX_FAIL("%s: src / dst / norm is NULL", who);
    if (src == dst) TEX_FAIL("%s: dst is src (every output reads the whole level)", who);
    p.src = src; p.dst = dst; p.norm_out = norm;
    return envmap_launch<false>(who, p, kind, stream);
}

int dirt_envmap_filter_backward(const float* grad_dst, const float* norm, float* grad_src, int size, int channels, long long face_stride,
                                float alpha, unsigned kind, void* stream)
{
    const char* who = "dirt_envmap_filter_backward";
    dirt::EnvmapParams p{};
    const int rc = envmap_check(who, size, channels, face_stride, alpha, kind, p);
    if (rc) return rc;
    if (!grad_dst || !norm || !grad_src) TEX_FAIL("%s: grad_dst / norm / grad_src is NULL", who);
    if (grad_dst == grad_src) TEX_FAIL("%s: grad_src is grad_dst (every output reads the whole level)", who);
    p.src = grad_dst; p.norm = norm; p.dst = grad_src;
    return envmap_launch<true>(who, p, kind, stream);
}

}  // extern "C"
