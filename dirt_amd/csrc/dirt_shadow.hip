// dirt_shadow.hip -- the per-pixel look-up of shadow maps from a G-buffer, fused: one kernel forward, one backward.
//
// A light's depth image (clip-space z of the nearest surface, drawn by the rasteriser from the light: shading.py::
// render_shadow_map) is compared with the depth of each pixel's world position as that light sees it, through a percentage-
// closer filter and a smooth comparison, so that the visibility is differentiable in the position, the map and the matrix.
// The specification (DESIGN.md §7h restates it; dirt_amd/lighting.py::shadow_visibility is its readable form, which
// tests/shadow_reference.py restates in float64), per pixel with position p, normal n, mask m, and per light with map Z
// [Hs, Ws] and matrix M (row vectors: clip = [q, 1] @ M), K = kernel in {1, 3, 5}, h = (K - 1) / 2:
//
//     q = p + normal_offset unit3(n)               (x, y, z, w) = [q, 1] @ M           d = z
//     col = (x / w + 1) Ws / 2 - 0.5               row = (1 - y / w) Hs / 2 - 0.5
//     r0 = floor(row) - h, fr = row - floor(row)   c0 = floor(col) - h, fc = col - floor(col)
//     wr[0] = 1 - fr, wr[K] = fr, wr[a] = 1 between; wc likewise
//     S(r, c) = s(((Z[r, c] - d) + bias) (1 / softness) + 1/2) inside the map, 1 outside;  s(t) = u u (3 - 2 u), u = clamp(t, 0, 1)
//     v = (1 / K^2) sum_{a, b = 0..K} (wr[a] wc[b]) S(r0 + a, c0 + b)                   out = 1 - m (1 - v)
//
//  A pixel that is not (w > 0) or whose whole window lies off the map has v = 1 and gives no gradient (a NaN fails every
//  comparison the conditions are written with and so falls into this case).  Gradients, with g = d loss / d out, cw = m g / K^2,
//  e(r, c) = cw wr wc 6 u (1 - u) / softness for the texels inside:
//
//     d m = -(1 - v) g           d Z[r, c] += e(r, c)          d z = -sum e
//     d row = cw sum_b wc[b] (S[K][b] - S[0][b])               d col = cw sum_a wr[a] (S[a][K] - S[a][0])
//     d (x / w) = d col Ws / 2      d (y / w) = -d row Hs / 2
//     d x = d (x / w) / w     d y = d (y / w) / w     d w = -(d (x / w) x / w + d (y / w) y / w) / w
//     d q = M d clip          d M[i][j] = [q, 1]_i d clip_j        d p = d q        d n = unit3_backward(normal_offset d q)
//
// Kernels: shadow_forward_kernel<K>, one lane per pixel, a loop over the lights; shadow_backward_kernel<K>, one workgroup of
// SHADOW_BLOCK lanes per tile of the pixel grid (16 x 16 of an image, 256 x 1 of a flat list: dirt_texture_common.h), SHADOW_ITER
// tile per workgroup.  A lane recomputes its pixel's forward and, per light, (c) scatters d Z by the texture backward's scheme --
// a tile whose window box in the light's map fits TEX_PATCH texels sums in LDS and sends one atomic per touched texel, a larger
// box and every flat list send theirs straight to memory: d maps is not the same bits on every run -- and (b) leaves the
// workgroup's 16 sums of d M in LDS: wave_sum, lane 0, then one row of 16 L partial sums per workgroup in caller-owned
// scratch, which shade_launch_reduce adds in a fixed order (a matrix set shared by the scenes: over the scenes in scene
// order).  No float atomics there, the same bits on every run.  (a) The lanes' rows d p, d n, d m wait in LDS and leave through
// the tile walk of dirt_shade_common.h, one image row of the tile after the other: every row of d gbuffer is written whole,
// whatever Cg, exact zeros in the channels no attribute uses.  What `needs_input_grad` does not ask for is a NULL pointer
// and a workgroup-uniform branch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_shade_common.h"
#include "dirt_texture_common.h"

namespace dirt {

constexpr int SHADOW_BLOCK = 256;   // lanes of a workgroup, pixels of a tile
constexpr int SHADOW_ITER = 1;      // tiles of a backward workgroup
static_assert(SHADOW_ITER == 1, "the backward kernel holds one tile's rows and one row of partial sums in LDS");
constexpr int SHADOW_MAT = 16;     // floats of a light's matrix, sums of its gradient
constexpr int SHADOW_ROW = 9, SHADOW_ZERO = 7;   // floats of a pixel's row in the LDS tile: dp[3], dn[3], dm, 0 (odd: no bank conflicts)

struct ShadowParams {
    const float* g;         // [scenes, pixels, Cg]
    const float* maps;      // [map_scenes, L, Hs, Ws]
    const float* mats;      // [matrix_scenes, L, 4, 4]
    float* out;             // [scenes, pixels, L]
    const float* gout;      // [scenes, pixels, L]
    float* gg;              // [scenes, pixels, Cg] or nullptr
    float* gmaps;           // like maps, accumulated into (cleared by the entry point), or nullptr
    float* partial;         // [scenes, tiles, 16 L] or nullptr
    long long pixels;       // of a scene
    long long map_stride;   // floats between two scenes' maps, 0: one set for every scene
    int mat_stride;         // likewise of the matrices
    int Cg, op, on, om;     // on = -1: normal_offset is 0; om = -1: every pixel is covered
    int L, Hs, Ws;
    float bias, inv_softness, offset;
};

// where a pixel falls in a light's map
struct ShadowTap {
    bool on;               // in front of the light and with a texel of its window on the map
    int r0, c0;
    float fr, fc, d, ws, ndx, ndy;
};

template <int K>
__device__ __forceinline__ void shadow_project(const float (&q)[3], const float* __restrict__ M, int Hs, int Ws, ShadowTap& t)
{
    constexpr int H = (K - 1) / 2;
    const float x = ((q[0] * M[0] + q[1] * M[4]) + q[2] * M[8]) + M[12], y = ((q[0] * M[1] + q[1] * M[5]) + q[2] * M[9]) + M[13];
    const float z = ((q[0] * M[2] + q[1] * M[6]) + q[2] * M[10]) + M[14], w = ((q[0] * M[3] + q[1] * M[7]) + q[2] * M[11]) + M[15];
    const bool front = w > 0.f;                 // (false for a NaN)
    t.ws = front ? w : 1.f;
    t.ndx = x / t.ws; t.ndy = y / t.ws; t.d = z;
    const float col = (t.ndx + 1.f) * (0.5f * (float)Ws) - 0.5f, row = (1.f - t.ndy) * (0.5f * (float)Hs) - 0.5f;
    const float fr0 = floorf(row), fc0 = floorf(col);
    // rows r0 .. r0 + K of the window against rows 0 .. Hs - 1 of the map, in float: false for a NaN and for what no int holds
    t.on = front && fr0 + (float)(H + 1) >= 0.f && fr0 - (float)H <= (float)(Hs - 1) && fc0 + (float)(H + 1) >= 0.f && fc0 - (float)H <= (float)(Ws - 1);
    t.r0 = t.on ? (int)fr0 - H : 0; t.c0 = t.on ? (int)fc0 - H : 0;
    t.fr = t.on ? row - fr0 : 0.f; t.fc = t.on ? col - fc0 : 0.f;
}

// the weight of tap a = 0 .. K along an axis with fraction f
template <int K> __device__ __forceinline__ float shadow_weight(int a, float f) { return a == 0 ? 1.f - f : (a == K ? f : 1.f); }

__device__ __forceinline__ float shadow_compare(float Z, float d, const ShadowParams& P)
{
    return clip01(((Z - d) + P.bias) * P.inv_softness + 0.5f);   // u: S = u u (3 - 2 u)
}

// q = p + normal_offset unit3(n) of pixel `row`
__device__ __forceinline__ void shadow_point(const ShadowParams& P, const float* __restrict__ row, float (&p)[3], float (&n)[3], float (&q)[3],
                                             float& len, float& inv)
{
    load3(row + P.op, p);
    q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    n[0] = n[1] = n[2] = 0.f; len = 0.f; inv = 0.f;
    if (P.on >= 0) {   // (uniform)
        float N[3];
        load3(row + P.on, n);
        unit3(n, N, len, inv);
#pragma unroll
        for (int j = 0; j < 3; ++j) q[j] = p[j] + P.offset * N[j];
    }
}

// ---- forward: one lane per pixel
template <int K>
__global__ __launch_bounds__(SHADOW_BLOCK) void shadow_forward_kernel(ShadowParams P)
{
    const long long i = (long long)blockIdx.x * SHADOW_BLOCK + threadIdx.x;
    if (i >= P.pixels) return;
    const long long pix = (long long)blockIdx.y * P.pixels + i;
    const float* __restrict__ row = P.g + pix * P.Cg;
    float p[3], n[3], q[3], len, inv;
    shadow_point(P, row, p, n, q, len, inv);
    const float m = P.om >= 0 ? row[P.om] : 1.f;
    for (int l = 0; l < P.L; ++l) {
        const float* __restrict__ M = P.mats + (size_t)blockIdx.y * P.mat_stride + l * SHADOW_MAT;
        const float* __restrict__ Z = P.maps + (size_t)blockIdx.y * P.map_stride + (size_t)l * P.Hs * P.Ws;
        ShadowTap t;
        shadow_project<K>(q, M, P.Hs, P.Ws, t);
        float v = 1.f;
        if (t.on) {
            float acc = 0.f;
            for (int a = 0; a <= K; ++a) {
                const int r = t.r0 + a;
                const float wr = shadow_weight<K>(a, t.fr);
#pragma unroll
                for (int b = 0; b <= K; ++b) {
                    const int c = t.c0 + b;
                    float S = 1.f;
                    if ((unsigned)r < (unsigned)P.Hs && (unsigned)c < (unsigned)P.Ws) {
                        const float u = shadow_compare(Z[(size_t)r * P.Ws + c], t.d, P);
                        S = (u * u) * (3.f - 2.f * u);
                    }
                    acc += (wr * shadow_weight<K>(b, t.fc)) * S;
                }
            }
            v = acc * (1.f / (float)(K * K));
        }
        P.out[pix * P.L + l] = 1.f - m * (1.f - v);
    }
}

// ---- backward: one workgroup per tile of the pixel grid
template <int K>
__global__ __launch_bounds__(SHADOW_BLOCK) void shadow_backward_kernel(ShadowParams P, int rows, int cols, int tw, int th, int tiles_x)
{
    __shared__ float s_acc[TEX_PATCH];
    __shared__ int s_box[4];                                   // rmin, rmax, cmin, cmax of the tile's windows in a light's map
    __shared__ float s_g[SHADOW_BLOCK * SHADOW_ROW];
    __shared__ float s_part[4 * DIRT_SHADOW_MAX_LIGHTS * SHADOW_MAT];
    __shared__ unsigned char s_src[DIRT_SHADE_MAX_CHANNELS];
    const int tid = threadIdx.x, Cg = P.Cg, NP = P.L * SHADOW_MAT;
    if (P.gg)   // (uniform)
        for (int ch = tid; ch < Cg; ch += SHADOW_BLOCK)
            s_src[ch] = (unsigned char)((unsigned)(ch - P.op) < 3u ? ch - P.op
                                        : (P.on >= 0 && (unsigned)(ch - P.on) < 3u ? 3 + ch - P.on : (ch == P.om ? 6 : SHADOW_ZERO)));
    long long i;
    const bool active = tile_pixel<long long>(tid, tw, th, tiles_x, (long long)rows, (long long)cols, i);
    const long long pix = (long long)blockIdx.y * P.pixels + i;
    const float* __restrict__ row = P.g + pix * Cg;
    float p[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f}, len = 0.f, inv = 0.f, m = 0.f;
    if (active) {
        shadow_point(P, row, p, n, q, len, inv);
        m = P.om >= 0 ? row[P.om] : 1.f;
    }
    float dq[3] = {0.f, 0.f, 0.f}, dm = 0.f;
    const bool patches = P.gmaps && rows > 1;                  // (uniform) a flat list sends its atomics straight to memory
    for (int l = 0; l < P.L; ++l) {
        const float* __restrict__ M = P.mats + (size_t)blockIdx.y * P.mat_stride + l * SHADOW_MAT;
        const size_t map0 = (size_t)blockIdx.y * P.map_stride + (size_t)l * P.Hs * P.Ws;
        const float* __restrict__ Z = P.maps + map0;
        ShadowTap t;
        shadow_project<K>(q, M, P.Hs, P.Ws, t);
        t.on = t.on && active;
        bool patch = false;
        int rmin = 0, cmin = 0, bh = 0, bw = 0;
        if (patches) {
            __syncthreads();   // every lane has read the light before's box
            if (tid == 0) box_clear(s_box);
            __syncthreads();
            if (t.on) {   // the window's texels inside the map
                Taps k;
                k.r0 = max(t.r0, 0); k.r1 = min(t.r0 + K, P.Hs - 1); k.c0 = max(t.c0, 0); k.c1 = min(t.c0 + K, P.Ws - 1);
                box_add(s_box, k);
            }
            __syncthreads();
            rmin = s_box[0]; cmin = s_box[2];
            bh = s_box[1] - rmin + 1; bw = s_box[3] - cmin + 1;
            patch = bh > 0 && bw > 0 && (long long)bh * bw <= TEX_PATCH;   // (uniform)
            if (patch) {
                clear_patch(s_acc, bh * bw, tid);
                __syncthreads();
            }
        }
        float dclip[4] = {0.f, 0.f, 0.f, 0.f};
        if (t.on) {
            const float g = P.gout[pix * P.L + l];
            const float cw = (m * g) * (1.f / (float)(K * K));
            float acc = 0.f, r_first = 0.f, r_last = 0.f, c_first = 0.f, c_last = 0.f, dd = 0.f;
            float* __restrict__ gz = P.gmaps ? P.gmaps + map0 : nullptr;
            for (int a = 0; a <= K; ++a) {
                const int r = t.r0 + a;
                const float wr = shadow_weight<K>(a, t.fr);
#pragma unroll
                for (int b = 0; b <= K; ++b) {
                    const int c = t.c0 + b;
                    const float wc = shadow_weight<K>(b, t.fc);
                    float S = 1.f;
                    if ((unsigned)r < (unsigned)P.Hs && (unsigned)c < (unsigned)P.Ws) {
                        const float u = shadow_compare(Z[(size_t)r * P.Ws + c], t.d, P);
                        S = (u * u) * (3.f - 2.f * u);
                        const float e = ((cw * (wr * wc)) * ((6.f * u) * (1.f - u))) * P.inv_softness;
                        dd -= e;
                        if (gz && e != 0.f) {
                            if (patch) atomicAdd(&s_acc[(r - rmin) * bw + (c - cmin)], e);
                            else atomicAdd(&gz[(size_t)r * P.Ws + c], e);
                        }
                    }
                    acc += (wr * wc) * S;
                    // the window's first and last row and column, each summed by itself in the same order: where they hold
                    // the same comparisons (a lit or a shadowed region) their difference is an exact zero
                    if (a == 0) r_first += wc * S;
                    if (a == K) r_last += wc * S;
                    if (b == 0) c_first += wr * S;
                    if (b == K) c_last += wr * S;
                }
            }
            const float a_fr = r_last - r_first, a_fc = c_last - c_first;
            const float v = acc * (1.f / (float)(K * K));
            dm -= (1.f - v) * g;
            const float dndx = (cw * a_fc) * (0.5f * (float)P.Ws), dndy = -((cw * a_fr) * (0.5f * (float)P.Hs));
            dclip[0] = dndx / t.ws; dclip[1] = dndy / t.ws; dclip[2] = dd;
            dclip[3] = -(dndx * t.ndx + dndy * t.ndy) / t.ws;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                dq[j] += (M[j * 4] * dclip[0] + M[j * 4 + 1] * dclip[1]) + (M[j * 4 + 2] * dclip[2] + M[j * 4 + 3] * dclip[3]);
        }
        if (patch) {
            __syncthreads();
            // the patch to memory: consecutive lanes -> consecutive floats of a map row
            float* __restrict__ gz = P.gmaps + map0;
            for (int e = tid; e < bh * bw; e += SHADOW_BLOCK) {
                const float val = s_acc[e];
                if (val != 0.f) atomicAdd(&gz[box_texel(e, rmin, cmin, bw, P.Ws, 1)], val);
            }
            __syncthreads();
        }
        if (P.partial) {   // (uniform) d M[i][j] = [q, 1]_i d clip_j: the wave's sums to lane 0's row of s_part
            const float q4[4] = {q[0], q[1], q[2], 1.f};
#pragma unroll
            for (int k = 0; k < SHADOW_MAT; ++k) {
                const float s = wave_sum(t.on ? q4[k >> 2] * dclip[k & 3] : 0.f);   // (a select: a NaN point adds nothing)
                if ((tid & 63) == 0) s_part[(tid >> 6) * NP + l * SHADOW_MAT + k] = s;
            }
        }
    }
    if (P.gg && active) {   // the lane's row of the LDS tile
        float dn[3] = {0.f, 0.f, 0.f};
        if (P.on >= 0) {
            const float gN[3] = {P.offset * dq[0], P.offset * dq[1], P.offset * dq[2]};
            unit3_backward(gN, n, len, inv, dn);
        }
        float* __restrict__ r = s_g + tid * SHADOW_ROW;
#pragma unroll
        for (int j = 0; j < 3; ++j) { r[j] = dq[j]; r[3 + j] = dn[j]; }
        r[6] = dm; r[SHADOW_ZERO] = 0.f;
    }
    __syncthreads();
    // (fold_waves_to_row with the row's length known at run time: L is no template argument here)
    if (P.partial && tid < NP)
        P.partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NP + tid] = (s_part[tid] + s_part[NP + tid]) + (s_part[2 * NP + tid] + s_part[3 * NP + tid]);
    if (P.gg) {   // (uniform) the tile's image rows leave one after the other, each whole
        const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
        const long long x0 = (long long)tile_x * tw, y0 = (long long)tile_y * th;
        const int wv = (int)(cols - x0 < tw ? cols - x0 : tw), hv = (int)(rows - y0 < th ? rows - y0 : th);
        const TileWalk wk = tile_walk<SHADOW_BLOCK>(Cg, tid);
        for (int rr = 0; rr < hv; ++rr) {
            float* __restrict__ dst = P.gg + ((long long)blockIdx.y * P.pixels + (y0 + rr) * cols + x0) * Cg;
            const float* s_row = s_g + rr * tw * SHADOW_ROW;
            tile_for_each<SHADOW_BLOCK>(wv, Cg, tid, wk, [&](int e, int pxi, int ch) { dst[e] = s_row[pxi * SHADOW_ROW + s_src[ch]]; });
        }
    }
}

template <template <int> class F, class... A>
inline void shadow_dispatch(int kernel, A&&... a)
{
    if (kernel == 1) F<1>::go(a...);
    else if (kernel == 3) F<3>::go(a...);
    else F<5>::go(a...);
}
template <int K> struct ShadowForward {
    static void go(const ShadowParams& P, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((shadow_forward_kernel<K>), grid, dim3(SHADOW_BLOCK), 0, s, P); }
};
template <int K> struct ShadowBackward {
    static void go(const ShadowParams& P, dim3 grid, hipStream_t s, long long rows, long long cols, const TileGrid& t)
    {
        hipLaunchKernelGGL((shadow_backward_kernel<K>), grid, dim3(SHADOW_BLOCK), 0, s, P, (int)rows, (int)cols, t.tw, t.th, (int)t.tiles_x);
    }
};

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

// the arguments both entry points take, under the names they take them by
struct ShadowArgs {
    long long scenes, pixels;
    int Cg, off_positions, off_normals, off_mask, lights, Hs, Ws, map_scenes, matrix_scenes, kernel;
    float bias, softness, normal_offset;
};

static int shadow_check(const char* who, const ShadowArgs& a, dirt::ShadowParams& P)
{
    if (int rc = dirt::shade_check_sizes(who, a.scenes, a.pixels, a.Cg)) return rc;
    if (a.scenes * a.pixels > (1ll << 40)) STAGE_FAIL("%s: %lld x %lld pixels, at most 2^40", who, a.scenes, a.pixels);
    if (a.lights < 1 || a.lights > DIRT_SHADOW_MAX_LIGHTS) STAGE_FAIL("%s: %d lights, 1..%d", who, a.lights, DIRT_SHADOW_MAX_LIGHTS);
    if (a.Hs < 1 || a.Ws < 1 || (long long)a.Hs * a.Ws > 0x7fffffffll) STAGE_FAIL("%s: a map of %d x %d texels, 1 x 1 to 2^31 - 1 texels", who, a.Hs, a.Ws);
    if (a.map_scenes != 1 && a.map_scenes != a.scenes) STAGE_FAIL("%s: map_scenes=%d is neither 1 nor scenes=%lld", who, a.map_scenes, a.scenes);
    if (a.matrix_scenes != 1 && a.matrix_scenes != a.scenes) STAGE_FAIL("%s: matrix_scenes=%d is neither 1 nor scenes=%lld", who, a.matrix_scenes, a.scenes);
    if (a.kernel != 1 && a.kernel != 3 && a.kernel != 5) STAGE_FAIL("%s: kernel=%d is none of 1, 3, 5", who, a.kernel);
    if (!(a.softness > 0.f) || !(a.softness <= 3.4e38f)) STAGE_FAIL("%s: softness=%g is not a finite number > 0", who, a.softness);
    // inv_softness below: past FLT_MAX it would be Inf, and 0 * Inf where (Z - d) + bias is 0 a NaN in the value and every gradient
    if (1.0 / (double)a.softness > 3.4028234663852886e38) STAGE_FAIL("%s: softness=%g has no finite float32 reciprocal", who, a.softness);
    if (!(a.bias >= -3.4e38f && a.bias <= 3.4e38f)) STAGE_FAIL("%s: bias=%g is not finite", who, a.bias);
    if (!(a.normal_offset >= -3.4e38f && a.normal_offset <= 3.4e38f)) STAGE_FAIL("%s: normal_offset=%g is not finite", who, a.normal_offset);
    if (a.normal_offset != 0.f && a.off_normals == -1) STAGE_FAIL("%s: normal_offset=%g needs the normals' channels", who, a.normal_offset);
    const int off[3] = {a.off_positions, a.off_normals, a.off_mask}, width[3] = {3, 3, 1};
    const bool absent[3] = {false, a.off_normals == -1, a.off_mask == -1};
    const char* const names[3] = {"positions", "normals", "mask"};
    if (int rc = dirt::shade_check_attributes(who, a.Cg, 3, off, width, absent, names)) return rc;
    P.pixels = a.pixels; P.Cg = a.Cg; P.op = a.off_positions; P.on = a.normal_offset != 0.f ? a.off_normals : -1; P.om = a.off_mask;
    P.L = a.lights; P.Hs = a.Hs; P.Ws = a.Ws;
    P.map_stride = a.map_scenes == 1 ? 0 : (long long)a.lights * a.Hs * a.Ws;
    P.mat_stride = a.matrix_scenes == 1 ? 0 : a.lights * dirt::SHADOW_MAT;
    P.bias = a.bias; P.inv_softness = (float)(1.0 / (double)a.softness); P.offset = a.normal_offset;
    return DIRT_OK;
}

// the pixel grid of a backward: rows x cols, whose tiles and sides the kernel holds in ints; 0 tiles for a grid it refuses
static long long shadow_tiles(long long rows, long long cols)
{
    if (rows < 0 || cols < 0 || rows > 0x7fffffffll || cols > 0x7fffffffll) return 0;
    const dirt::TileGrid t = dirt::tile_grid(rows, cols);
    return t.tiles > 0x7fffffffll ? 0 : t.tiles;
}

size_t dirt_shadow_scratch_bytes(long long scenes, long long rows, long long cols, int lights)
{
    if (scenes < 0 || scenes > 65535 || lights < 1 || lights > DIRT_SHADOW_MAX_LIGHTS) return 0;
    return sizeof(float) * (size_t)scenes * (size_t)shadow_tiles(rows, cols) * (size_t)(lights * dirt::SHADOW_MAT);
}

int dirt_shadow_forward(const float* gbuffer, const float* maps, const float* matrices, float* out, long long scenes, long long pixels, int Cg,
                        int off_positions, int off_normals, int off_mask, int lights, int Hs, int Ws, int map_scenes, int matrix_scenes, int kernel,
                        float bias, float softness, float normal_offset, void* stream)
{
    const char* who = "dirt_shadow_forward";
    dirt::ShadowParams P{};
    const ShadowArgs a{scenes, pixels, Cg, off_positions, off_normals, off_mask, lights, Hs, Ws, map_scenes, matrix_scenes, kernel, bias, softness, normal_offset};
    if (int rc = shadow_check(who, a, P)) return rc;
    if (scenes * pixels == 0) return dirt::stage_ok(report);
    if (!gbuffer || !maps || !matrices || !out) STAGE_FAIL("%s: gbuffer / maps / matrices / out is NULL", who);
    if (pixels > 0x7fffffffll * dirt::SHADOW_BLOCK) STAGE_FAIL("%s: too many pixels per scene", who);
    P.g = gbuffer; P.maps = maps; P.mats = matrices; P.out = out;
    const dim3 grid((unsigned)((pixels + dirt::SHADOW_BLOCK - 1) / dirt::SHADOW_BLOCK), (unsigned)scenes);
    dirt::shadow_dispatch<dirt::ShadowForward>(kernel, P, grid, reinterpret_cast<hipStream_t>(stream));
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_shadow_backward(const float* gbuffer, const float* maps, const float* matrices, const float* grad_out, float* grad_gbuffer, float* grad_maps,
                         float* grad_matrices, void* scratch, size_t scratch_bytes, long long scenes, long long rows, long long cols, int Cg,
                         int off_positions, int off_normals, int off_mask, int lights, int Hs, int Ws, int map_scenes, int matrix_scenes, int kernel,
                         float bias, float softness, float normal_offset, void* stream)
{
    const char* who = "dirt_shadow_backward";
    dirt::ShadowParams P{};
    if (rows < 0 || cols < 0 || (rows > 0 && cols > (1ll << 40) / rows)) STAGE_FAIL("%s: bad pixel grid (rows=%lld cols=%lld)", who, rows, cols);
    const ShadowArgs a{scenes, rows * cols, Cg, off_positions, off_normals, off_mask, lights, Hs, Ws, map_scenes, matrix_scenes, kernel, bias, softness, normal_offset};
    if (int rc = shadow_check(who, a, P)) return rc;
    if (!grad_gbuffer && !grad_maps && !grad_matrices) return dirt::stage_ok(report);
    const long long tiles = shadow_tiles(rows, cols);
    if (scenes * P.pixels > 0) {
        if (tiles == 0) STAGE_FAIL("%s: pixel grid too large (rows=%lld cols=%lld)", who, rows, cols);
        if (!gbuffer || !maps || !matrices || !grad_out) STAGE_FAIL("%s: gbuffer / maps / matrices / grad_out is NULL", who);
        if (grad_matrices)
            if (int rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_shadow_scratch_bytes(scenes, rows, cols, lights), "dirt_shadow_scratch_bytes"))
                return rc;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int NP = lights * dirt::SHADOW_MAT;
    hipError_t e = hipSuccess;
    if (grad_maps) e = dirt::clear_floats(grad_maps, (long long)map_scenes * lights * Hs * Ws, s);
    if (e != hipSuccess) return dirt::stage_hip(report, who, e);
    if (scenes * P.pixels == 0) {   // nothing to launch: the sums are zeros
        if (grad_matrices) e = dirt::clear_floats(grad_matrices, (long long)matrix_scenes * NP, s);
        return dirt::stage_hip(report, who, e);
    }
    P.g = gbuffer; P.maps = maps; P.mats = matrices; P.gout = grad_out; P.gg = grad_gbuffer; P.gmaps = grad_maps;
    P.partial = grad_matrices ? static_cast<float*>(scratch) : nullptr;
    const dirt::TileGrid t = dirt::tile_grid(rows, cols);
    dirt::shadow_dispatch<dirt::ShadowBackward>(kernel, P, dim3((unsigned)tiles, (unsigned)scenes), s, rows, cols, t);
    return dirt::shade_backward_finish(who, scratch, grad_matrices, scenes, tiles, NP, matrix_scenes, s);
}

}  // extern "C"
