// dirt_background.hip -- the environment seen behind the mesh (a skybox), fused: one kernel forward; backward one per-pixel
// pass and the cube look-up's own backward kernels for the scatter into the environment.
//
// The pixels a mesh does not cover show the environment cube itself, looked up along the ray through the pixel.  The ray needs
// nothing from memory but the 16 floats of the camera's clip-to-world matrix, and the mask says which pixels need no look-up
// at all.  The specification (DESIGN.md §7i restates it; dirt_amd/lighting.py::environment_background is its readable form,
// which tests/background_reference.py restates in float64), per pixel (r, c) of an H x W image with mask m (0 without one),
// matrix M (row vectors) and intensity I, one float32 operation per step:
//
//     nx = (2 (c + 0.5)) / W - 1           ny = 1 - (2 (r + 0.5)) / H
//     a_j = nx M[0][j] + ny M[1][j]        h0_j = a_j + M[3][j]             hm_j = (a_j - M[2][j]) + M[3][j]
//     end = h0.xyz / h0.w                  start = hm.xyz / hm.w             d = end - start
//     E = the look-up of d: spec 2 - 5 of dirt_texture_cube.hip (nearest: the texel; bilinear; trilinear at lambda)
//     out_j = ((1 - m) I_j) E_j            (0 where d is not valid or 1 - m == 0: no look-up is made there)
//
//  lambda = lod + lod_bias, or from the analytic footprint, for axis x with row M[0] and scale 2 / W, y with M[1] and 2 / H:
//     dd = scale ((row.xyz - end row.w) / h0.w - (row.xyz - start row.w) / hm.w)
//     ds = (sc(dd) - s ma(dd)) / a         dt = (tc(dd) - t ma(dd)) / a     (the picks of d's own face; s, t, a of cube_look)
//     rho = (N / 2) sqrt(max(ds_x^2 + dt_x^2, ds_y^2 + dt_y^2))             lambda = log2 rho + lod_bias
//  and is a constant: no gradient flows through it.
//
//  Gradients, with g = d loss / d out and w = 1 - m:  d I_j = sum w E_j g_j;  d m = -sum_j I_j E_j g_j;  what arrives at E is
//  (w I_j) g_j;  gd = the cube look-up's direction gradient of that (spec 6);  then
//     g0.xyz = gd / h0.w    g0.w = -(gd . end) / h0.w        gm.xyz = -gd / hm.w     gm.w = (gd . start) / hm.w
//     d M[0][j] = sum nx (g0_j + gm_j)     d M[1][j] = sum ny (g0_j + gm_j)     d M[2][j] = sum -gm_j     d M[3][j] = sum (g0_j + gm_j)
//
// Kernels: background_forward_kernel<FILTER>, one lane per pixel on the 16 x 16 tiles of the pixel grid (256 x 1 of a one-row
// image), the scene in blockIdx.y; the matrix and the intensity are wave-uniform (scalar loads), the mask one 4-byte load at its
// own stride, 12 bytes written per lane.  background_backward_kernel<FILTER>, one workgroup per tile: the forward again with
// the derivative of each look-up by its own index (cube_sample), d mask by one dense store per lane, the 16 + 3 sums of d M and
// d I by wave_sum -> fold_waves_to_row -> one row each per workgroup in caller-owned scratch -> shade_launch_reduce, in a
// fixed order (an operand shared by the scenes: over the scenes in scene order): no float atomics.  What the environment's
// gradient needs it leaves per pixel in the same scratch -- d (zeros where nothing is to be added), lambda, and the gradient
// arriving at E -- and the entry point hands those to cube_backward_launch for the scatter alone, as dirt_shade_ibl.hip does.
// What `needs_input_grad` does not ask for is a NULL pointer and a workgroup-uniform branch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_shade_common.h"
#include "dirt_texture_cube.h"

namespace dirt {

constexpr int BG_BLOCK = 256;          // lanes of a workgroup, pixels of a tile
constexpr int BG_MAT = 16, BG_INT = 3;   // the sums of a workgroup: d matrix, d intensity
constexpr int BG_PIXEL_FLOATS = 7;     // per-pixel floats of the scratch: d[3], lambda, d E[3]

struct BackgroundParams {
    const float* pyr;        // [6, face_floats]: the environment, a packed pyramid per face (one level: the cube itself), 3 channels
    const float* mats;       // [matrix_scenes, 4, 4]
    const float* inten;      // [intensity_scenes, 3]
    const float* mask;       // a scene's pixels `mask_stride` floats apart, or nullptr (every pixel is background)
    float* out;              // [scenes, pixels, 3]
    const float* gout;       // [scenes, pixels, 3]
    float* gmask;            // [scenes, pixels] or nullptr
    float* part_m;           // [scenes, tiles, 16] or nullptr
    float* part_i;           // [scenes, tiles, 3] or nullptr
    float* s_dir;            // [scenes, pixels, 3]: d; these three or nullptr (the environment wants no gradient)
    float* s_lod;            // [scenes, pixels]
    float* s_genv;           // [scenes, pixels, 3]: what arrives at E
    long long pixels, face_floats, mask_scene;   // pixels of a scene; floats of a face; floats between two scenes' masks (0: one mask)
    int rows, cols, N, L, mat_stride, int_stride, mask_stride;
    int footprint;           // lambda from the footprint, not from `lod`
    float lod, lod_bias;
};

// everything the forward computes at a pixel; the derivatives only where GRAD
struct BackgroundEval {
    float nx, ny, h0w, hmw, start[3], end[3], lam, f;
    CubeLook q;
    CubeSample s0, s1;       // the two levels at d (nearest: s0.v is the texel)
    float E[3];
};

// log2 of the footprint of a pixel in texels of level 0 (the head of this file)
__device__ __forceinline__ float background_footprint(const BackgroundParams& P, const float* __restrict__ M, const BackgroundEval& e)
{
    float n2[2];
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {
        const float* __restrict__ row = M + 4 * axis;
        const float scale = 2.f / (float)(axis == 0 ? P.cols : P.rows);
        float dd[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) dd[j] = scale * ((row[j] - e.end[j] * row[3]) / e.h0w - (row[j] - e.start[j] * row[3]) / e.hmw);
        const bool mx = e.q.major == 0, my = e.q.major == 1, pos = e.q.pos;
        const float sc = mx ? (pos ? -dd[2] : dd[2]) : (my ? dd[0] : (pos ? dd[0] : -dd[0]));
        const float tc = my ? (pos ? dd[2] : -dd[2]) : -dd[1];
        const float mc = mx ? dd[0] : (my ? dd[1] : dd[2]);
        const float ma = pos ? mc : -mc;
        const float ds = (sc - e.q.s * ma) / e.q.a, dt = (tc - e.q.t * ma) / e.q.a;
        n2[axis] = ds * ds + dt * dt;
    }
    const float big = n2[0] > n2[1] ? n2[0] : n2[1];   // (a NaN in n2[0] leaves n2[1]; lambda NaN: level 0, mip_split)
    return log2f((0.5f * (float)P.N) * sqrtf(big));
}

// FILTER: DIRT_BACKGROUND_NEAREST / _BILINEAR / _TRILINEAR.  `look`: the pixel is inside the grid and 1 - m != 0
template <int FILTER, bool GRAD>
__device__ __forceinline__ void background_eval(const BackgroundParams& P, const float* __restrict__ M, int r, int c, bool look, BackgroundEval& e)
{
    e.nx = (2.f * ((float)c + 0.5f)) / (float)P.cols - 1.f;
    e.ny = 1.f - (2.f * ((float)r + 0.5f)) / (float)P.rows;
    float h0[4], hm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = e.nx * M[j] + e.ny * M[4 + j];
        h0[j] = a + M[12 + j];
        hm[j] = (a - M[8 + j]) + M[12 + j];
    }
    e.h0w = h0[3]; e.hmw = hm[3];
    float d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        e.end[j] = h0[j] / h0[3]; e.start[j] = hm[j] / hm[3];
        d[j] = look ? e.end[j] - e.start[j] : 0.f;
    }
    e.q = cube_look(d[0], d[1], d[2]);       // (all zero: not valid)
    cube_sample_clear(e.s0); cube_sample_clear(e.s1);
    e.E[0] = e.E[1] = e.E[2] = 0.f; e.lam = 0.f; e.f = 0.f;
    if (!e.q.valid) return;
    const float* __restrict__ face = P.pyr + (size_t)e.q.face() * P.face_floats;
    if constexpr (FILTER == DIRT_BACKGROUND_NEAREST) {   // the texel itself, not a blend of weight 1
        float drow, dcol;
        const Taps k = cube_taps(e.q, P.N, true, drow, dcol);
        load3(face + ((size_t)k.r0 * P.N + k.c0) * 3, e.s0.v);
#pragma unroll
        for (int j = 0; j < 3; ++j) e.E[j] = e.s0.v[j];
        return;
    }
    int l = 0;
    if constexpr (FILTER == DIRT_BACKGROUND_TRILINEAR) {
        e.lam = (P.footprint ? background_footprint(P, M, e) : P.lod) + P.lod_bias;   // (uniform)
        mip_split(e.lam, P.L, l, e.f);
    }
    const int n0 = mip_dim(P.N, l);
    cube_sample<GRAD>(face + cube_level_offset(P.N, n0, 3), n0, e.q, e.s0);
    if (e.f != 0.f) {
        const int n1 = mip_dim(P.N, l + 1);
        cube_sample<GRAD>(face + cube_level_offset(P.N, n1, 3), n1, e.q, e.s1);
    }
    const float w0 = 1.f - e.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) e.E[j] = e.f != 0.f ? w0 * e.s0.v[j] + e.f * e.s1.v[j] : e.s0.v[j];
}

// lane `tid`'s pixel: its index in the scene, row and column, and 1 - m; false outside the grid
__device__ __forceinline__ bool background_pixel(const BackgroundParams& P, int tid, int tw, int th, int tiles_x, long long& i, int& r, int& c, float& m)
{
    const bool active = tile_pixel<int>(tid, tw, th, tiles_x, P.rows, P.cols, i);
    r = (int)(i / P.cols); c = (int)(i - (long long)r * P.cols);
    m = active && P.mask ? P.mask[(long long)blockIdx.y * P.mask_scene + i * P.mask_stride] : 0.f;
    return active;
}

// ---- forward: one lane per pixel; the matrix and the intensity are wave-uniform (scalar loads)
template <int FILTER>
__global__ __launch_bounds__(BG_BLOCK) void background_forward_kernel(BackgroundParams P, int tw, int th, int tiles_x)
{
    long long i; int r, c; float m;
    if (!background_pixel(P, threadIdx.x, tw, th, tiles_x, i, r, c, m)) return;
    const float* __restrict__ M = P.mats + (size_t)blockIdx.y * P.mat_stride;
    const float* __restrict__ I = P.inten + (size_t)blockIdx.y * P.int_stride;
    const float w = 1.f - m;
    BackgroundEval e;
    background_eval<FILTER, false>(P, M, r, c, w != 0.f, e);
    float o[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = e.q.valid ? (w * I[j]) * e.E[j] : 0.f;
    store3(P.out + ((long long)blockIdx.y * P.pixels + i) * 3, o);
}

// ---- backward: one workgroup per tile of the pixel grid
template <int FILTER>
__global__ __launch_bounds__(BG_BLOCK) void background_backward_kernel(BackgroundParams P, int tw, int th, int tiles_x)
{
    __shared__ float s_part_m[4 * BG_MAT];
    __shared__ float s_part_i[4 * BG_INT];
    const int tid = threadIdx.x;
    long long i; int r, c; float m;
    const bool active = background_pixel(P, tid, tw, th, tiles_x, i, r, c, m);
    const long long pix = (long long)blockIdx.y * P.pixels + i;
    const float* __restrict__ M = P.mats + (size_t)blockIdx.y * P.mat_stride;
    const float* __restrict__ I = P.inten + (size_t)blockIdx.y * P.int_stride;
    const float w = 1.f - m;
    BackgroundEval e;
    background_eval<FILTER, true>(P, M, r, c, active && w != 0.f, e);
    const bool valid = e.q.valid;            // (false outside the grid and where 1 - m == 0)
    float g[3] = {0.f, 0.f, 0.f};
    if (active) load3(P.gout + pix * 3, g);
    float genv[3], gI[3], gm = 0.f, gs = 0.f, gt = 0.f;
    const float w0 = 1.f - e.f;
    const bool two = e.f != 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float eg = e.E[j] * g[j];
        gI[j] = valid ? w * eg : 0.f;
        gm -= valid ? I[j] * eg : 0.f;
        genv[j] = valid ? (w * I[j]) * g[j] : 0.f;
        gs += genv[j] * (two ? w0 * e.s0.ds[j] + e.f * e.s1.ds[j] : e.s0.ds[j]);
        gt += genv[j] * (two ? w0 * e.s0.dt[j] + e.f * e.s1.dt[j] : e.s0.dt[j]);
    }
    if (active && P.gmask) P.gmask[pix] = gm;
    if (active && P.s_dir) {   // (uniform pointer) what the scatter reads: an all-zero direction adds nothing
        float d[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) d[j] = valid ? e.end[j] - e.start[j] : 0.f;
        store3(P.s_dir + pix * 3, d);
        P.s_lod[pix] = e.lam;
        store3(P.s_genv + pix * 3, genv);
    }
    if (P.part_m) {   // (uniform) d M through d = end - start, end = h0.xyz / h0.w, start = hm.xyz / hm.w
        float gd[3] = {0.f, 0.f, 0.f};
        if (valid && FILTER != DIRT_BACKGROUND_NEAREST) cube_direction_gradient(e.q, gs, gt, gd);
        float g0[4], gmn[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) { g0[j] = gd[j] / e.h0w; gmn[j] = -(gd[j] / e.hmw); }
        g0[3] = -(dot3(gd, e.end) / e.h0w);
        gmn[3] = dot3(gd, e.start) / e.hmw;
        const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int k = 0; k < BG_MAT; ++k) {
            const int j = k & 3, row = k >> 2;
            const float sum = g0[j] + gmn[j];
            const float v = row == 0 ? e.nx * sum : (row == 1 ? e.ny * sum : (row == 2 ? -gmn[j] : sum));
            const float s = wave_sum(valid ? v : 0.f);   // (a select: a pixel with h.w = 0 adds nothing)
            if (lane == 0) s_part_m[wave * BG_MAT + k] = s;
        }
    }
    if (P.part_i) {   // (uniform)
        const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int k = 0; k < BG_INT; ++k) {
            const float s = wave_sum(gI[k]);
            if (lane == 0) s_part_i[wave * BG_INT + k] = s;
        }
    }
    __syncthreads();
    if (P.part_m && tid < BG_MAT) fold_waves_to_row<BG_MAT>(s_part_m, P.part_m, tid);
    if (P.part_i && tid < BG_INT) fold_waves_to_row<BG_INT>(s_part_i, P.part_i, tid);
}

template <template <int> class F, class... A>
inline void background_dispatch(int filter, A&&... a)
{
    if (filter == DIRT_BACKGROUND_NEAREST) F<DIRT_BACKGROUND_NEAREST>::go(a...);
    else if (filter == DIRT_BACKGROUND_BILINEAR) F<DIRT_BACKGROUND_BILINEAR>::go(a...);
    else F<DIRT_BACKGROUND_TRILINEAR>::go(a...);
}
template <int FILTER> struct BackgroundForward {
    static void go(const BackgroundParams& P, dim3 grid, hipStream_t s, const TileGrid& t)
    {
        hipLaunchKernelGGL((background_forward_kernel<FILTER>), grid, dim3(BG_BLOCK), 0, s, P, t.tw, t.th, (int)t.tiles_x);
    }
};
template <int FILTER> struct BackgroundBackward {
    static void go(const BackgroundParams& P, dim3 grid, hipStream_t s, const TileGrid& t)
    {
        hipLaunchKernelGGL((background_backward_kernel<FILTER>), grid, dim3(BG_BLOCK), 0, s, P, t.tw, t.th, (int)t.tiles_x);
    }
};

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

// the arguments both entry points take, under the names they take them by
struct BackgroundArgs {
    long long scenes, rows, cols;
    int size, levels, matrix_scenes, intensity_scenes, mask_scenes, mask_stride, filter;
    float lod, lod_bias; unsigned flags;
};

// the tiles of a scene's pixel grid; 0 for a grid the entry points refuse
static long long background_tiles(long long rows, long long cols)
{
    if (rows < 0 || cols < 0 || rows > 0x7fffffffll || cols > 0x7fffffffll || (rows > 0 && cols > (1ll << 40) / rows)) return 0;
    const dirt::TileGrid t = dirt::tile_grid(rows, cols);
    return t.tiles > 0x7fffffffll ? 0 : t.tiles;
}

// what both entry points refuse, before any device work; fills what they share of P
static int background_check(const char* who, const BackgroundArgs& a, bool has_mask, dirt::BackgroundParams& P)
{
    if (a.scenes < 0 || a.scenes > 65535) STAGE_FAIL("%s: %lld scenes, 0..65535", who, a.scenes);
    if (a.rows < 0 || a.cols < 0 || a.rows > 0x7fffffffll || a.cols > 0x7fffffffll || (a.rows > 0 && a.cols > (1ll << 40) / a.rows))
        STAGE_FAIL("%s: bad pixel grid (rows=%lld cols=%lld), at most 2^31 - 1 each way and 2^40 pixels", who, a.rows, a.cols);
    if (a.filter != DIRT_BACKGROUND_NEAREST && a.filter != DIRT_BACKGROUND_BILINEAR && a.filter != DIRT_BACKGROUND_TRILINEAR)
        STAGE_FAIL("%s: filter=%d is none of DIRT_BACKGROUND_NEAREST, _BILINEAR, _TRILINEAR", who, a.filter);
    if (a.flags & ~DIRT_BACKGROUND_FOOTPRINT) STAGE_FAIL("%s: unknown flags 0x%x", who, a.flags);
    if (a.filter != DIRT_BACKGROUND_TRILINEAR && (a.flags & DIRT_BACKGROUND_FOOTPRINT))
        STAGE_FAIL("%s: DIRT_BACKGROUND_FOOTPRINT applies to DIRT_BACKGROUND_TRILINEAR only (filter=%d)", who, a.filter);
    if (a.size < 1 || a.size > 32768) STAGE_FAIL("%s: environment size %d, 1..32768", who, a.size);
    const int most = dirt::mip_level_count(a.size, a.size, -1);
    if (a.levels < 1 || a.levels > most) STAGE_FAIL("%s: %d levels, a %d x %d face has 1..%d", who, a.levels, a.size, a.size, most);
    if (a.filter != DIRT_BACKGROUND_TRILINEAR && a.levels != 1)
        STAGE_FAIL("%s: %d levels, a look-up that is not trilinear reads a cube of one level", who, a.levels);
    if (a.matrix_scenes != 1 && a.matrix_scenes != a.scenes) STAGE_FAIL("%s: matrix_scenes=%d is neither 1 nor scenes=%lld", who, a.matrix_scenes, a.scenes);
    if (a.intensity_scenes != 1 && a.intensity_scenes != a.scenes)
        STAGE_FAIL("%s: intensity_scenes=%d is neither 1 nor scenes=%lld", who, a.intensity_scenes, a.scenes);
    if (has_mask && a.mask_scenes != 1 && a.mask_scenes != a.scenes) STAGE_FAIL("%s: mask_scenes=%d is neither 1 nor scenes=%lld", who, a.mask_scenes, a.scenes);
    if (has_mask && a.mask_stride < 1) STAGE_FAIL("%s: mask_stride=%d, a pixel's mask is 1 float", who, a.mask_stride);
    if (!(a.lod >= -3.4e38f && a.lod <= 3.4e38f) || !(a.lod_bias >= -3.4e38f && a.lod_bias <= 3.4e38f))
        STAGE_FAIL("%s: lod=%g, lod_bias=%g: not finite", who, a.lod, a.lod_bias);
    if (a.scenes * a.rows * a.cols > 0 && background_tiles(a.rows, a.cols) == 0) STAGE_FAIL("%s: pixel grid too large (rows=%lld cols=%lld)", who, a.rows, a.cols);
    P.pixels = a.rows * a.cols; P.rows = (int)a.rows; P.cols = (int)a.cols; P.N = a.size; P.L = a.levels;
    P.face_floats = dirt::cube_face_floats(a.size, a.levels, 3);
    P.mat_stride = a.matrix_scenes == 1 ? 0 : dirt::BG_MAT; P.int_stride = a.intensity_scenes == 1 ? 0 : dirt::BG_INT;
    P.mask_stride = has_mask ? a.mask_stride : 0;
    P.mask_scene = has_mask && a.mask_scenes != 1 ? P.pixels * a.mask_stride : 0;
    P.footprint = (a.flags & DIRT_BACKGROUND_FOOTPRINT) ? 1 : 0; P.lod = a.lod; P.lod_bias = a.lod_bias;
    return DIRT_OK;
}

// the floats of the partial rows in front of the per-pixel scratch
static long long background_partial_floats(long long scenes, long long rows, long long cols)
{
    return scenes * background_tiles(rows, cols) * (dirt::BG_MAT + dirt::BG_INT);
}

size_t dirt_background_scratch_bytes(long long scenes, long long rows, long long cols)
{
    if (scenes < 0 || scenes > 65535 || (rows * cols != 0 && background_tiles(rows, cols) == 0)) return 0;
    return sizeof(float) * (size_t)(background_partial_floats(scenes, rows, cols) + scenes * rows * cols * dirt::BG_PIXEL_FLOATS);
}

int dirt_background_forward(const float* environment, const float* matrices, const float* intensity, const float* mask, float* out,
                            long long scenes, long long rows, long long cols, int size, int levels, int matrix_scenes, int intensity_scenes,
                            int mask_scenes, int mask_stride, int filter, float lod, float lod_bias, unsigned flags, void* stream)
{
    const char* who = "dirt_background_forward";
    dirt::BackgroundParams P{};
    const BackgroundArgs a{scenes, rows, cols, size, levels, matrix_scenes, intensity_scenes, mask_scenes, mask_stride, filter, lod, lod_bias, flags};
    if (int rc = background_check(who, a, mask != nullptr, P)) return rc;
    if (scenes * P.pixels == 0) return dirt::stage_ok(report);
    if (!environment || !matrices || !intensity || !out) STAGE_FAIL("%s: environment / matrices / intensity / out is NULL", who);
    P.pyr = environment; P.mats = matrices; P.inten = intensity; P.mask = mask; P.out = out;
    const dirt::TileGrid t = dirt::tile_grid(rows, cols);
    dirt::background_dispatch<dirt::BackgroundForward>(filter, P, dim3((unsigned)t.tiles, (unsigned)scenes), reinterpret_cast<hipStream_t>(stream), t);
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_background_backward(const float* environment, const float* matrices, const float* intensity, const float* mask, const float* grad_out,
                             float* grad_environment, float* grad_matrices, float* grad_intensity, float* grad_mask, void* scratch,
                             size_t scratch_bytes, long long scenes, long long rows, long long cols, int size, int levels, int matrix_scenes,
                             int intensity_scenes, int mask_scenes, int mask_stride, int filter, float lod, float lod_bias, unsigned flags,
                             void* stream)
{
    const char* who = "dirt_background_backward";
    dirt::BackgroundParams P{};
    const BackgroundArgs a{scenes, rows, cols, size, levels, matrix_scenes, intensity_scenes, mask_scenes, mask_stride, filter, lod, lod_bias, flags};
    if (int rc = background_check(who, a, mask != nullptr, P)) return rc;
    if (grad_mask && !mask) STAGE_FAIL("%s: grad_mask without mask", who);
    if (!grad_environment && !grad_matrices && !grad_intensity && !grad_mask) return dirt::stage_ok(report);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long n = scenes * P.pixels;
    if (n == 0) {   // nothing to launch: the sums are zeros
        hipError_t e = grad_environment ? dirt::clear_floats(grad_environment, 6 * P.face_floats, s) : hipSuccess;
        if (e == hipSuccess && grad_matrices) e = dirt::clear_floats(grad_matrices, (long long)matrix_scenes * dirt::BG_MAT, s);
        if (e == hipSuccess && grad_intensity) e = dirt::clear_floats(grad_intensity, (long long)intensity_scenes * dirt::BG_INT, s);
        return dirt::stage_hip(report, who, e);
    }
    if (!environment || !matrices || !intensity || !grad_out) STAGE_FAIL("%s: environment / matrices / intensity / grad_out is NULL", who);
    if (grad_environment || grad_matrices || grad_intensity)
        if (int rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_background_scratch_bytes(scenes, rows, cols), "dirt_background_scratch_bytes"))
            return rc;
    const dirt::TileGrid t = dirt::tile_grid(rows, cols);
    // the grid of the environment's scatter: the scenes' images one below the other (a one-row image: one row)
    const long long grid_rows = rows == 1 ? 1 : scenes * rows, grid_cols = rows == 1 ? n : cols;
    if (grad_environment && (dirt::tile_grid(grid_rows, grid_cols).tiles > 0x7fffffffll || grid_cols > 0x7fffffffll || grid_rows > 0x7fffffffll))
        STAGE_FAIL("%s: pixel grid too large (scenes=%lld rows=%lld cols=%lld)", who, scenes, rows, cols);
    P.pyr = environment; P.mats = matrices; P.inten = intensity; P.mask = mask; P.gout = grad_out; P.gmask = grad_mask;
    float* const base = static_cast<float*>(scratch);
    if (grad_matrices) P.part_m = base;
    if (grad_intensity) P.part_i = base + scenes * t.tiles * dirt::BG_MAT;
    if (grad_environment) {
        P.s_dir = base + background_partial_floats(scenes, rows, cols);
        P.s_lod = P.s_dir + 3 * n; P.s_genv = P.s_lod + n;
    }
    dirt::background_dispatch<dirt::BackgroundBackward>(filter, P, dim3((unsigned)t.tiles, (unsigned)scenes), s, t);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && grad_matrices) {
        dirt::shade_launch_reduce(P.part_m, grad_matrices, matrix_scenes == 1 ? scenes * t.tiles : t.tiles, dirt::BG_MAT, matrix_scenes, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess && grad_intensity) {
        dirt::shade_launch_reduce(P.part_i, grad_intensity, intensity_scenes == 1 ? scenes * t.tiles : t.tiles, dirt::BG_INT, intensity_scenes, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess && grad_environment) {   // the scatter, by the cube look-up's backward kernels (no gradient to a direction or to lod)
        dirt::CubeParams c{};
        c.n = n; c.Ct = 3; c.gdir_stride = 3; c.lod_bias = 0.f; c.flags = filter == DIRT_BACKGROUND_NEAREST ? DIRT_TEX_NEAREST : 0;
        c.pyr = environment; c.dirs = P.s_dir; c.dir_stride = 3; c.lod = filter == DIRT_BACKGROUND_TRILINEAR ? P.s_lod : nullptr;
        c.N = size; c.L = levels; c.face_floats = P.face_floats; c.grad_out = P.s_genv; c.grad_pyr = grad_environment;
        e = dirt::cube_backward_launch(c, grid_rows, grid_cols, s);
    }
    return dirt::stage_hip(report, who, e);
}

}  // extern "C"
