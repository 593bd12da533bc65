// dirt_texture_mip.hip -- trilinear (mipmapped) texture look-up of a deferred shader, and its gradient.
//
// Extends the fused look-up of dirt_texture.hip (the reference's samples/textured.py:16-61: `uvs_to_pixel_indices` then a
// bilinear `sample_texture`) with a mip pyramid and a level of detail taken from the screen-space footprint of (u, v).
// The specification (DESIGN.md §7 restates it; tests/mip_reference.py implements it in numpy):
//
//  1. Pyramid.  Level 0 is the texture [Ht, Wt, Ct].  Level k+1 exists while level k is not 1 x 1, each dimension of level
//     k is even or 1, and k+1 <= max_level (when given).  Each dimension halves; a dimension of size 1 stays 1.  A texel of
//     level k+1 is the mean of its 2 x 2 block, ((t00 + t01) + (t10 + t11)) * 0.25, or of its 2 x 1 block, (a + b) * 0.5,
//     in float32.  All levels live in one packed buffer, level after level, each [H_k, W_k, Ct]; H_k = max(Ht >> k, 1).
//  2. Index at level k.  The level-0 fractional index (row, col) is uv_to_index's (repeat / clamp, scaled by Ht, Wt).  Per
//     axis, with s = size_0 / size_k: index_k = max((index_0 - (s - 1) * 0.5) / s, 0) (texel footprints stay aligned across
//     levels under the reference's convention of no half-texel shift; the max keeps bilinear_taps inside its domain), and
//     index_0 itself at k = 0.  Then the bilinear taps at level k's size.  (max is written x < 0 ? 0 : x: a NaN stays NaN.)
//  3. LOD.  Either given per look-up (lambda = lod + lod_bias), or from an image of look-ups [..., H, W, 2] (stacked images
//     never share neighbours): x-difference = uv(r, c+1) - uv(r, c) if that pixel exists and is valid, else
//     uv(r, c) - uv(r, c-1) if that one is, else 0; the y-difference likewise along rows; `valid` = mask != 0 (every pixel
//     without a mask); repeat mode wraps each difference to d - rint(d).  rho = max(|(du_x Wt, dv_x Ht)|, |(du_y Wt, dv_y Ht)|)
//     and lambda = log2(rho) + lod_bias; a pixel whose own mask is 0 takes lambda = 0.
//  4. Blend.  lambda clamped to [0, L - 1] (NaN -> 0); l = floor(lambda), f = lambda - l;
//     out = (1 - f) * S_l + f * S_{l+1} with S_l the bilinear sample of level l; where f == 0 only S_l is read and written
//     (so lambda <= 0 gives the bilinear look-up of dirt_texture.hip bit for bit).
//  5. Gradients.  To the texture: every level's share is summed into a pyramid-shaped scratch buffer, which one launch
//     collapses to level 0 (each base texel sums its ancestors top down: acc = g_{L-1}; acc = g_k + acc * factor_{k+1},
//     factor 1/4 for a 2 x 2 block, 1/2 for a 2 x 1 one).  To (u, v): through both levels' bilinear weights, the 1/s of
//     index_k included, clamp mode's zero outside [0, 1] as before; lambda is held constant (no gradient flows through the
//     finite-difference footprint).  To lod: S_{l+1} - S_l where lambda lies strictly inside (0, L - 1) before the clamp,
//     else 0.  To the mask: none.
//
// Kernels: the pyramid in one launch of 32 x 32-texel blocks reduced through levels 1-5 in LDS, plus one single-workgroup
// launch for the levels above; the forward one look-up per lane (its (u, v) neighbours read through L1 / L2); the backward
// on 16 x 16-pixel tiles that sum into an LDS patch per touched level (at most two adjacent levels) and fall back to float
// atomics into the scratch pyramid where the footprint does not fit; then the collapse.  A texture per scene
// (dirt_texture_*_batch*): every kernel's BATCH instantiation, the scene in gridDim.y, pyramids and scratch [scenes, floats]
// (dirt_texture_common.h: batched launches); the top build launch becomes one workgroup per scene.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_texture_common.h"

namespace dirt {

constexpr int MIP_MAX = 32;        // levels of a pyramid (a dimension of 2^31 halves 31 times)
constexpr int MIP_TILE_LEVELS = 5; // levels reduced in LDS by the block kernel (a 32 x 32 block -> 1 x 1)

struct MipArgs {
    const float* pyr;        // packed pyramid (level 0 = the texture)
    const float* uvs;        // rows x cols pairs (u, v), `uv_stride` floats apart
    const float* lod;        // rows x cols levels of detail, or nullptr (footprint)
    const float* mask;       // rows x cols, `mask_stride` floats apart, or nullptr (every pixel valid)
    long long rows, cols;    // the look-ups as an image grid (stacked images: `image_rows` rows each)
    int image_rows, Ht, Wt, Ct, L, uv_stride, guv_stride, mask_stride;
    float lod_bias;
    unsigned flags;
    float* out;              // [n, Ct]
    const float* grad_out;   // [n, Ct]
    float* grad_pyr;         // packed pyramid-shaped scratch (cleared by the caller of the kernel)
    float* grad_uvs;         // pairs `guv_stride` apart, or nullptr
    float* grad_lod;         // n, or nullptr
};
struct MipParams : MipArgs {
    long long off[MIP_MAX];  // float offset of each level in the packed buffers
};

// the floats of the packed pyramid
template <class P> __host__ __device__ __forceinline__ long long mip_floats(const P& p)
{
    return p.off[p.L - 1] + (long long)mip_dim(p.Ht, p.L - 1) * mip_dim(p.Wt, p.L - 1) * p.Ct;
}

// BATCH: the kernel's argument describes scene 0 of a batch and blockIdx.y is the scene (dirt_texture_common.h).  What that scene's look-ups
// see: MipParams member for member, the pointers at the scene's pyramid, look-ups, outputs and gradients, the level offsets still the
// argument's own table (a modified copy of the whole argument left the table, indexed by level, in scratch memory in the backward kernel).
// The per-look-up functions below take either as `P`.
struct MipScene : MipArgs {
    const long long (&off)[MIP_MAX];
    __device__ __forceinline__ MipScene(const MipParams& q) : MipArgs(q), off(q.off)
    {
        const size_t b = blockIdx.y, floats = (size_t)mip_floats(q), n = (size_t)(rows * cols);
        scene_shift(pyr, b * floats); scene_shift(uvs, b * n * uv_stride); scene_shift(lod, b * n); scene_shift(mask, b * n * mask_stride);
        scene_shift(out, b * n * Ct); scene_shift(grad_out, b * n * Ct); scene_shift(grad_pyr, b * floats);
        scene_shift(grad_uvs, b * n * guv_stride); scene_shift(grad_lod, b * n);
    }
};
template <bool BATCH> __device__ __forceinline__ std::conditional_t<BATCH, MipScene, const MipParams&> mip_scene(const MipParams& q)
{
    if constexpr (BATCH) return MipScene(q); else return q;
}

// the index of a level-0 fractional index at level k, per axis (spec 2), and its derivative with respect to the level-0 index
__device__ __forceinline__ float mip_index(float idx0, int n0, int nk, float& d)
{
    const float s = (float)n0 / (float)nk;             // a power of two: the division and 1 / s are exact
    const float x = (idx0 - (s - 1.f) * 0.5f) * (1.f / s);
    d = x < 0.f ? 0.f : 1.f / s;
    return x < 0.f ? 0.f : x;
}

template <class P> __device__ __forceinline__ bool mip_valid(const P& p, long long j) { return !p.mask || p.mask[j * p.mask_stride] != 0.f; }

template <class P> __device__ __forceinline__ void mip_uv(const P& p, long long j, float& u, float& v)
{
    u = p.uvs[j * p.uv_stride]; v = p.uvs[j * p.uv_stride + 1];
}

// lambda of look-up i, before the clamp (spec 3)
template <class P> __device__ __forceinline__ float mip_lambda(const P& p, long long i, float u, float v, bool clamp_mode)
{
    if (p.lod) return p.lod[i] + p.lod_bias;
    if (!mip_valid(p, i)) return 0.f;
    long long py, px, r;   // grid row and column, row inside the image (32-bit divisions where the grid allows)
    if (i <= 0x7fffffffll && p.cols <= 0x7fffffffll) {
        const unsigned q = (unsigned)i / (unsigned)p.cols;
        py = q; px = (long long)((unsigned)i - q * (unsigned)p.cols); r = q % (unsigned)p.image_rows;
    } else {
        py = i / p.cols; px = i - py * p.cols; r = py % p.image_rows;
    }
    float dux = 0.f, dvx = 0.f, duy = 0.f, dvy = 0.f, un, vn;
    if (px + 1 < p.cols && mip_valid(p, i + 1)) { mip_uv(p, i + 1, un, vn); dux = un - u; dvx = vn - v; }
    else if (px >= 1 && mip_valid(p, i - 1)) { mip_uv(p, i - 1, un, vn); dux = u - un; dvx = v - vn; }
    if (r + 1 < p.image_rows && mip_valid(p, i + p.cols)) { mip_uv(p, i + p.cols, un, vn); duy = un - u; dvy = vn - v; }
    else if (r >= 1 && mip_valid(p, i - p.cols)) { mip_uv(p, i - p.cols, un, vn); duy = u - un; dvy = v - vn; }
    if (!clamp_mode) { dux -= rintf(dux); dvx -= rintf(dvx); duy -= rintf(duy); dvy -= rintf(dvy); }
    const float ax = dux * (float)p.Wt, bx = dvx * (float)p.Ht, ay = duy * (float)p.Wt, by = dvy * (float)p.Ht;
    const float rx = sqrtf(ax * ax + bx * bx), ry = sqrtf(ay * ay + by * by);
    return log2f(fmaxf(rx, ry)) + p.lod_bias;
}

// ---- pyramid build: a workgroup takes a block of th x tw base texels (32 x 32 where the pyramid goes that far) and reduces it
// through levels 1..kt in LDS, writing level 0 (the copy) and every level it makes; channels in passes of four.
__device__ __forceinline__ float mip_reduce(const float* __restrict__ src, int sw, int r, int c, bool hr, bool hc, int j)
{
    const int r0 = hr ? 2 * r : r, c0 = hc ? 2 * c : c;
    const float t00 = src[(r0 * sw + c0) * 4 + j];
    if (hr && hc) {
        const float t01 = src[(r0 * sw + c0 + 1) * 4 + j], t10 = src[((r0 + 1) * sw + c0) * 4 + j], t11 = src[((r0 + 1) * sw + c0 + 1) * 4 + j];
        return ((t00 + t01) + (t10 + t11)) * 0.25f;
    }
    const float t1 = hr ? src[((r0 + 1) * sw + c0) * 4 + j] : src[(r0 * sw + c0 + 1) * 4 + j];
    return (t00 + t1) * 0.5f;
}

template <bool BATCH = false>
__global__ __launch_bounds__(256) void mip_build_blocks_kernel(const float* __restrict__ tex, float* __restrict__ pyr, MipParams p, int kt,
                                                               int tiles_x)
{
    if constexpr (BATCH) { tex += (size_t)blockIdx.y * p.Ht * p.Wt * p.Ct; pyr += (size_t)blockIdx.y * mip_floats(p); }
    __shared__ float s_a[32 * 32 * 4];
    __shared__ float s_b[16 * 16 * 4];
    const int tid = threadIdx.x, Ct = p.Ct;
    const int Hk_t = mip_dim(p.Ht, kt), Wk_t = mip_dim(p.Wt, kt);
    const int th = p.Ht / Hk_t, tw = p.Wt / Wk_t;   // the block of base texels (<= 32 x 32)
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    for (int c0 = 0; c0 < Ct; c0 += 4) {
        const int nc = min(4, Ct - c0);
        for (int e = tid; e < th * tw * nc; e += 256) {   // consecutive lanes on consecutive floats of a texture row
            const int rr = e / (tw * nc), rest = e - rr * tw * nc, cc = rest / nc, j = rest - cc * nc;
            const size_t g = ((size_t)(ty * th + rr) * p.Wt + (tx * tw + cc)) * Ct + c0 + j;
            const float x = tex[g];
            pyr[g] = x;
            s_a[(rr * tw + cc) * 4 + j] = x;
        }
        __syncthreads();
        int sh = th, sw = tw;
        for (int k = 1; k <= kt; ++k) {
            const bool hr = mip_dim(p.Ht, k - 1) > 1, hc = mip_dim(p.Wt, k - 1) > 1;
            const int dh = hr ? sh / 2 : sh, dw = hc ? sw / 2 : sw;
            const float* src = (k & 1) ? s_a : s_b;
            float* dst = (k & 1) ? s_b : s_a;
            const int Wk = mip_dim(p.Wt, k);
            for (int e = tid; e < dh * dw * nc; e += 256) {
                const int rr = e / (dw * nc), rest = e - rr * dw * nc, cc = rest / nc, j = rest - cc * nc;
                const float x = mip_reduce(src, sw, rr, cc, hr, hc, j);
                dst[(rr * dw + cc) * 4 + j] = x;
                pyr[p.off[k] + ((size_t)(ty * dh + rr) * Wk + (tx * dw + cc)) * Ct + c0 + j] = x;
            }
            __syncthreads();
            sh = dh; sw = dw;
        }
    }
}

// the levels above kt: one workgroup, level after level from the packed buffer (a level kt of up to 64 x 64 texels for a
// 2048 x 2048 texture); BATCH: one workgroup per scene
template <bool BATCH = false>
__global__ __launch_bounds__(1024) void mip_build_top_kernel(float* __restrict__ pyr, MipParams p, int kt)
{
    if constexpr (BATCH) pyr += (size_t)blockIdx.y * mip_floats(p);
    const int Ct = p.Ct;
    for (int k = kt + 1; k < p.L; ++k) {
        const bool hr = mip_dim(p.Ht, k - 1) > 1, hc = mip_dim(p.Wt, k - 1) > 1;
        const int Hk = mip_dim(p.Ht, k), Wk = mip_dim(p.Wt, k), Ws = mip_dim(p.Wt, k - 1);
        const float* __restrict__ src = pyr + p.off[k - 1];
        float* __restrict__ dst = pyr + p.off[k];
        for (int e = threadIdx.x; e < Hk * Wk * Ct; e += blockDim.x) {
            const int t = e / Ct, j = e - t * Ct, r = t / Wk, c = t - r * Wk;
            const int r0 = hr ? 2 * r : r, c0 = hc ? 2 * c : c;
            const float t00 = src[((size_t)r0 * Ws + c0) * Ct + j];
            float x;
            if (hr && hc) {
                const float t01 = src[((size_t)r0 * Ws + c0 + 1) * Ct + j], t10 = src[((size_t)(r0 + 1) * Ws + c0) * Ct + j];
                const float t11 = src[((size_t)(r0 + 1) * Ws + c0 + 1) * Ct + j];
                x = ((t00 + t01) + (t10 + t11)) * 0.25f;
            } else {
                const float t1 = hr ? src[((size_t)(r0 + 1) * Ws + c0) * Ct + j] : src[((size_t)r0 * Ws + c0 + 1) * Ct + j];
                x = (t00 + t1) * 0.5f;
            }
            dst[e] = x;
        }
        __threadfence();
        __syncthreads();
    }
}

// ---- collapse: dL/dtexture[r, c] = sum over levels k of dL/dlevel_k[ancestor] * (the product of the factors below k), top down
template <bool BATCH = false>
__global__ __launch_bounds__(256) void mip_collapse_kernel(const float* __restrict__ gp, float* __restrict__ gt, MipParams p)
{
    if constexpr (BATCH) { gp += (size_t)blockIdx.y * mip_floats(p); gt += (size_t)blockIdx.y * p.Ht * p.Wt * p.Ct; }
    const int Ct = p.Ct;
    const long long n = (long long)p.Ht * p.Wt * Ct;
    const int lgh = 31 - __clz(p.Ht), lgw = 31 - __clz(p.Wt);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const long long t = e / Ct;
        const int j = (int)(e - t * Ct);
        const int r = (int)(t / p.Wt), c = (int)(t - (long long)r * p.Wt);
        float acc = 0.f;
        for (int k = p.L - 1; k >= 0; --k) {
            const int rk = r >> min(k, lgh), ck = c >> min(k, lgw);
            const float g = gp[p.off[k] + ((size_t)rk * mip_dim(p.Wt, k) + ck) * Ct + j];
            if (k == p.L - 1) { acc = g; continue; }
            const float factor = (mip_dim(p.Ht, k) > 1 && mip_dim(p.Wt, k) > 1) ? 0.25f : 0.5f;   // level k+1's block
            acc = g + acc * factor;
        }
        gt[e] = acc;
    }
}

// the taps of level l for a level-0 index (and the derivatives of the level's index)
template <class P> __device__ __forceinline__ Taps mip_taps(const P& p, int l, float row, float col, float& drow, float& dcol)
{
    if (l == 0) { drow = 1.f; dcol = 1.f; return bilinear_taps(row, col, p.Ht, p.Wt); }
    const int Hk = mip_dim(p.Ht, l), Wk = mip_dim(p.Wt, l);
    const float rk = mip_index(row, p.Ht, Hk, drow), ck = mip_index(col, p.Wt, Wk, dcol);
    return bilinear_taps(rk, ck, Hk, Wk);
}

// ---- forward: one look-up per lane
template <int CT, bool BATCH = false>
__global__ __launch_bounds__(256) void mip_forward_kernel(MipParams args)
{
    const auto& p = mip_scene<BATCH>(args);
    const bool clamp_mode = (p.flags & DIRT_TEX_CLAMP) != 0;
    const int Ct = CT ? CT : p.Ct;
    constexpr int NV = CT ? CT : 1;
    const long long n = p.rows * p.cols;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float u, v;
        mip_uv(p, i, u, v);
        float row, col, drow_dv, dcol_du;
        uv_to_index(u, v, p.Ht, p.Wt, clamp_mode, row, col, drow_dv, dcol_du);
        int l; float f;
        mip_split(mip_lambda(p, i, u, v, clamp_mode), p.L, l, f);
        float dr, dc;
        const Taps k0 = mip_taps(p, l, row, col, dr, dc);
        const float* __restrict__ lv0 = p.pyr + p.off[l];
        const int W0 = mip_dim(p.Wt, l);
        float* __restrict__ out = p.out + i * Ct;
        if (f == 0.f) {
            for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) { float o[NV]; mip_sample<CT>(lv0, W0, k0, Ct, ch, o); store_ch<CT>(out, o, ch); }
            continue;
        }
        const Taps k1 = mip_taps(p, l + 1, row, col, dr, dc);
        const float* __restrict__ lv1 = p.pyr + p.off[l + 1];
        const int W1 = mip_dim(p.Wt, l + 1);
        const float g = 1.f - f;
        for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) {
            float a[NV], b[NV], o[NV];
            mip_sample<CT>(lv0, W0, k0, Ct, ch, a); mip_sample<CT>(lv1, W1, k1, Ct, ch, b);
#pragma unroll
            for (int j = 0; j < NV; ++j) o[j] = g * a[j] + f * b[j];
            store_ch<CT>(out, o, ch);
        }
    }
}

// ---- backward: the tile scheme of dirt_texture_common.h with one LDS patch per touched level.  A lane's look-up has up to two tap
// sets: level l with weight 1 - f and level l + 1 with weight f (when f != 0).  Where the tile's sets span at most two adjacent levels
// and both bounding boxes fit TEX_PATCH texels together, each set sums into its level's patch; otherwise they scatter into memory.
template <int CT, bool BATCH = false>
__global__ __launch_bounds__(256) void mip_backward_kernel(MipParams args, int tw, int th, int tiles_x)
{
    const auto& p = mip_scene<BATCH>(args);
    constexpr int LCT = CT ? CT : 4;
    __shared__ float s_acc[TEX_PATCH * LCT];
    __shared__ int s_box[10];   // lmin, lmax, then rmin, rmax, cmin, cmax of the two levels' taps
    const bool clamp_mode = (p.flags & DIRT_TEX_CLAMP) != 0;
    const int Ct = CT ? CT : p.Ct;
    const int tid = threadIdx.x;
    long long i;
    const bool active = tile_pixel(tid, tw, th, tiles_x, p.rows, p.cols, i);
    if (tid == 0) {
        s_box[0] = 0x7fffffff; s_box[1] = -1;
        for (int s = 0; s < 2; ++s) box_clear(&s_box[2 + 4 * s]);
    }
    float u = 0.f, v = 0.f;
    if (active) mip_uv(p, i, u, v);
    float row, col, drow_dv, dcol_du;
    uv_to_index(u, v, p.Ht, p.Wt, clamp_mode, row, col, drow_dv, dcol_du);
    float lam = 0.f;
    if (active) lam = mip_lambda(p, i, u, v, clamp_mode);
    int l; float f;
    mip_split(lam, p.L, l, f);
    const bool inside = lam > 0.f && lam < (float)(p.L - 1);        // d out / d lambda is S_{l+1} - S_l here, 0 where clamped
    const bool want_lod = p.grad_lod && inside;
    const bool two = f != 0.f;                                       // the second set carries weight
    const bool read1 = two || want_lod;                              // ... or is read for the lod gradient only
    float dr0, dc0, dr1 = 0.f, dc1 = 0.f;
    const Taps k0 = mip_taps(p, l, row, col, dr0, dc0);
    Taps k1 = k0;
    if (read1) k1 = mip_taps(p, l + 1, row, col, dr1, dc1);
    __syncthreads();
    if (active) { atomicMin(&s_box[0], l); atomicMax(&s_box[1], two ? l + 1 : l); }
    __syncthreads();
    const int lmin = s_box[0];
    const bool span = s_box[1] - lmin <= 1;
    if (active && span) {
        box_add(&s_box[2 + 4 * (l - lmin)], k0);
        if (two) box_add(&s_box[2 + 4 * (l + 1 - lmin)], k1);
    }
    __syncthreads();
    int pr0[2], pc0[2], pw[2], pbase[2];
    int used = 0;
    for (int s = 0; s < 2; ++s) {
        const int bh = s_box[3 + 4 * s] - s_box[2 + 4 * s] + 1, bw = s_box[5 + 4 * s] - s_box[4 + 4 * s] + 1;
        pr0[s] = s_box[2 + 4 * s]; pc0[s] = s_box[4 + 4 * s];
        pw[s] = bh > 0 && bw > 0 ? bw : 0;
        pbase[s] = used;
        if (bh > 0 && bw > 0) used += (long long)bh * bw > TEX_PATCH ? TEX_PATCH + 1 : bh * bw;
    }
    const bool patch = span && used > 0 && used <= TEX_PATCH;   // (workgroup-uniform)
    const float w0 = 1.f - f;
    const float* __restrict__ lv0 = p.pyr + p.off[l];
    const float* __restrict__ lv1 = p.pyr + p.off[read1 ? l + 1 : l];
    float* __restrict__ gv0 = p.grad_pyr + p.off[l];
    float* __restrict__ gv1 = p.grad_pyr + p.off[two ? l + 1 : l];
    const int W0 = mip_dim(p.Wt, l), W1 = mip_dim(p.Wt, read1 ? l + 1 : l);
    float d_fr0 = 0.f, d_fc0 = 0.f, d_fr1 = 0.f, d_fc1 = 0.f, d_lod = 0.f;
    const float* __restrict__ gout = p.grad_out + i * Ct;
    for (int c0 = 0; c0 < Ct; c0 += LCT) {
        const int nc = CT ? CT : min(LCT, Ct - c0);
        if (patch) {
            clear_patch(s_acc, used * LCT, tid);
            __syncthreads();
        }
        if (active) {
            float g[LCT];
            load_grad_out<CT>(gout, Ct, c0, nc, g);
            for (int set = 0; set < 2; ++set) {
                if (set == 1 && !read1) break;   // the second set: read for the lod gradient, added only where it carries weight
                const Taps& k = set ? k1 : k0;
                const float* __restrict__ lv = set ? lv1 : lv0;
                float* __restrict__ gv = set ? gv1 : gv0;
                const float w = set ? f : w0;
                const bool scatter = set == 0 || two;
                const int ps = l + set - lmin;
                const Four<float> wt = {(k.wc0 * k.wr0) * w, (k.fc * k.wr0) * w, (k.wc0 * k.fr) * w, (k.fc * k.fr) * w};
                const Four<size_t> o = tap_offsets(k, set ? W1 : W0, Ct, c0);
                Four<int> lo = {0, 0, 0, 0};
                if (patch && scatter) lo = patch_offsets(k, pr0[ps], pc0[ps], pw[ps], LCT);
#pragma unroll
                for (int j = 0; j < LCT; ++j) {
                    if (j >= nc) break;
                    const Four<float> t = {lv[o.tl + j], lv[o.tr + j], lv[o.bl + j], lv[o.br + j]};
                    float e_fr, e_fc;
                    tap_gradients(g[j], t, k, e_fr, e_fc);
                    const float smp = ((t.tl * k.wc0) * k.wr0 + (t.tr * k.fc) * k.wr0) + ((t.bl * k.wc0) * k.fr + (t.br * k.fc) * k.fr);
                    if (set) { d_fr1 += e_fr; d_fc1 += e_fc; d_lod += g[j] * smp; }
                    else { d_fr0 += e_fr; d_fc0 += e_fc; d_lod -= g[j] * smp; }
                    if (!scatter) continue;
                    if (patch) add_taps(s_acc + pbase[ps] * LCT, lo, j, g[j], wt);
                    else add_taps(gv, o, j, g[j], wt);
                }
            }
        }
        if (patch) {
            __syncthreads();
            for (int e = tid; e < used * LCT; e += 256) {   // (as texture_backward_kernel's; a texel lies in the first level's box or the second's)
                const float val = s_acc[e];
                const int j = e % LCT, t = e / LCT;
                if (val != 0.f && j < nc) {
                    const int s = t >= pbase[1] && pw[1] > 0 ? 1 : 0;
                    const int lev = lmin + s, W = mip_dim(p.Wt, lev);
                    atomicAdd(&p.grad_pyr[p.off[lev] + box_texel(t - pbase[s], pr0[s], pc0[s], pw[s], W, Ct) + c0 + j], val);
                }
            }
            __syncthreads();
        }
    }
    if (!active) return;
    if (p.grad_uvs) {   // floor() has zero gradient: d frac / d index_k = 1, d index_k / d index_0 = 1 / s (0 where the max clamps)
        const float gu = (d_fc0 * dc0) * w0 + (two ? (d_fc1 * dc1) * f : 0.f);
        const float gvv = (d_fr0 * dr0) * w0 + (two ? (d_fr1 * dr1) * f : 0.f);
        p.grad_uvs[i * p.guv_stride] = gu * dcol_du;
        p.grad_uvs[i * p.guv_stride + 1] = gvv * drow_dv;
    }
    if (p.grad_lod) p.grad_lod[i] = want_lod ? d_lod : 0.f;
}

int mip_level_count(int Ht, int Wt, int max_level)
{
    int L = 1;
    int h = Ht, w = Wt;
    while (L < MIP_MAX && !(h == 1 && w == 1) && (h == 1 || h % 2 == 0) && (w == 1 || w % 2 == 0) && (max_level < 0 || L <= max_level)) {
        h = h > 1 ? h / 2 : 1; w = w > 1 ? w / 2 : 1; ++L;
    }
    return L;
}

void mip_offsets(MipParams& p)
{
    long long o = 0;
    for (int k = 0; k < MIP_MAX; ++k) {
        p.off[k] = o;
        if (k < p.L) o += (long long)mip_dim(p.Ht, k) * mip_dim(p.Wt, k) * p.Ct;
    }
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_texture_error;   // the error channel of this file's entry points

int dirt_texture_mip_levels(int Ht, int Wt, int Ct, int max_level, long long* pyramid_floats)
{
    if (Ht <= 0 || Wt <= 0 || Ct <= 0) TEX_FAIL("dirt_texture_mip_levels: bad sizes (Ht=%d Wt=%d Ct=%d)", Ht, Wt, Ct);
    dirt::MipParams p{};
    p.Ht = Ht; p.Wt = Wt; p.Ct = Ct; p.L = dirt::mip_level_count(Ht, Wt, max_level);
    dirt::mip_offsets(p);
    if (pyramid_floats) *pyramid_floats = dirt::mip_floats(p);
    dirt::stage_ok(report);
    return p.L;
}

static int mip_check(const char* who, int Ht, int Wt, int Ct, int levels, dirt::MipParams& p)
{
    if (Ht <= 0 || Wt <= 0 || Ct <= 0) TEX_FAIL("%s: bad sizes (Ht=%d Wt=%d Ct=%d)", who, Ht, Wt, Ct);
    if (levels < 1 || levels > dirt::mip_level_count(Ht, Wt, -1))
        TEX_FAIL("%s: %d levels, a %d x %d texture has 1..%d", who, levels, Ht, Wt, dirt::mip_level_count(Ht, Wt, -1));
    p.Ht = Ht; p.Wt = Wt; p.Ct = Ct; p.L = levels;
    dirt::mip_offsets(p);
    return DIRT_OK;
}

// (every entry point below and its batched form are one function that takes a dirt::Scenes: a single texture launches the kernels'
// single-texture instantiations; a batch of `sc.count` textures, checked by check_scenes, their BATCH ones with the scene in gridDim.y)

static int mip_build(const char* who, dirt::Scenes sc, const float* texture, float* pyramid, int Ht, int Wt, int Ct, int levels, void* stream)
{
    dirt::MipParams p{};
    int rc = mip_check(who, Ht, Wt, Ct, levels, p);
    if (rc) return rc;
    if (!texture || !pyramid) TEX_FAIL("%s: texture / pyramid is NULL", who);
    if (sc.batch && (rc = dirt::check_scenes(who, sc.count, {{dirt::mip_floats(p), 1}}))) return rc;
    if (sc.none()) return dirt::stage_ok(report);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (levels == 1)   // (a batch of one-level pyramids is the batch of textures)
        return dirt::stage_hip(report, who, hipMemcpyAsync(pyramid, texture, sizeof(float) * (size_t)Ht * Wt * Ct * sc.count, hipMemcpyDeviceToDevice, s));
    const int kt = min(levels - 1, dirt::MIP_TILE_LEVELS);
    const int tiles_y = dirt::mip_dim(Ht, kt), tiles_x = dirt::mip_dim(Wt, kt);
    if ((long long)tiles_x * tiles_y > 0x7fffffffll) TEX_FAIL("%s: texture too large", who);
    dirt::dispatch_scenes(sc, [&](auto b) {
        hipLaunchKernelGGL(dirt::mip_build_blocks_kernel<decltype(b)::value>, dirt::scene_grid(tiles_x * tiles_y, sc), dim3(256), 0, s, texture, pyramid, p, kt, tiles_x);
        if (levels - 1 > kt) hipLaunchKernelGGL(dirt::mip_build_top_kernel<decltype(b)::value>, dirt::scene_grid(1, sc), dim3(1024), 0, s, pyramid, p, kt);
    });
    return dirt::stage_hip(report, who, hipGetLastError());
}

static int mip_collapse(const char* who, dirt::Scenes sc, const float* grad_pyramid, float* grad_texture, int Ht, int Wt, int Ct, int levels, void* stream)
{
    dirt::MipParams p{};
    int rc = mip_check(who, Ht, Wt, Ct, levels, p);
    if (rc) return rc;
    if (!grad_pyramid || !grad_texture) TEX_FAIL("%s: grad_pyramid / grad_texture is NULL", who);
    if (sc.batch && (rc = dirt::check_scenes(who, sc.count, {{dirt::mip_floats(p), 1}}))) return rc;
    if (sc.none()) return dirt::stage_ok(report);
    const long long n = (long long)Ht * Wt * Ct;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dirt::dispatch_scenes(sc, [&](auto b) {
        hipLaunchKernelGGL(dirt::mip_collapse_kernel<decltype(b)::value>, dirt::scene_grid(dirt::capped_blocks(n), sc), dim3(256), 0, s, grad_pyramid, grad_texture, p);
    });
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_texture_mip_build(const float* texture, float* pyramid, int Ht, int Wt, int Ct, int levels, void* stream)
{
    return mip_build("dirt_texture_mip_build", dirt::ONE_TEXTURE, texture, pyramid, Ht, Wt, Ct, levels, stream);
}

int dirt_texture_mip_build_batch(const float* textures, float* pyramids, long long scenes, int Ht, int Wt, int Ct, int levels, void* stream)
{
    return mip_build("dirt_texture_mip_build_batch", {true, scenes}, textures, pyramids, Ht, Wt, Ct, levels, stream);
}

int dirt_texture_mip_collapse(const float* grad_pyramid, float* grad_texture, int Ht, int Wt, int Ct, int levels, void* stream)
{
    return mip_collapse("dirt_texture_mip_collapse", dirt::ONE_TEXTURE, grad_pyramid, grad_texture, Ht, Wt, Ct, levels, stream);
}

int dirt_texture_mip_collapse_batch(const float* grad_pyramids, float* grad_textures, long long scenes, int Ht, int Wt, int Ct, int levels,
                                    void* stream)
{
    return mip_collapse("dirt_texture_mip_collapse_batch", {true, scenes}, grad_pyramids, grad_textures, Ht, Wt, Ct, levels, stream);
}

static int mip_sample_check(const char* who, const float* pyramid, const float* uvs, const float* lod, long long rows, long long cols,
                            int image_rows, int Ht, int Wt, int Ct, int levels, int uv_stride, int mask_stride, const float* mask,
                            float lod_bias, unsigned flags, dirt::MipParams& p)
{
    int rc = mip_check(who, Ht, Wt, Ct, levels, p);
    if (!rc) rc = dirt::check_pixel_grid(who, rows, cols);
    if (rc) return rc;
    if (image_rows < 1 || (rows > 0 && rows % image_rows)) TEX_FAIL("%s: image_rows=%d does not divide rows=%lld", who, image_rows, rows);
    if (uv_stride < 2) TEX_FAIL("%s: uv_stride < 2", who);
    if (mask && mask_stride < 1) TEX_FAIL("%s: mask_stride < 1", who);
    if (rows * cols > 0 && (!pyramid || !uvs)) TEX_FAIL("%s: pyramid / uvs is NULL", who);
    if (flags & DIRT_TEX_NEAREST) TEX_FAIL("%s: DIRT_TEX_NEAREST does not apply to a trilinear look-up", who);
    p.pyr = pyramid; p.uvs = uvs; p.lod = lod; p.mask = lod ? nullptr : mask; p.rows = rows; p.cols = cols; p.image_rows = image_rows;
    p.uv_stride = uv_stride; p.mask_stride = mask_stride; p.lod_bias = lod_bias; p.flags = flags;
    return DIRT_OK;
}

// the per-scene extents of a batched look-up (p as mip_sample_check and the entry point filled it)
static int mip_sample_scenes(const char* who, long long scenes, const dirt::MipParams& p)
{
    const long long n = p.rows * p.cols;
    return dirt::check_scenes(who, scenes, {{dirt::mip_floats(p), 1}, {n, p.uv_stride}, {n, p.Ct}, {n, p.mask ? p.mask_stride : 0}, {n, p.grad_uvs ? p.guv_stride : 0}});
}

static int mip_sample_forward(const char* who, dirt::Scenes sc, const float* pyramid, const float* uvs, const float* lod, const float* mask, float* out,
                              long long rows, long long cols, int image_rows, int Ht, int Wt, int Ct, int levels, int uv_stride,
                              int mask_stride, float lod_bias, unsigned flags, void* stream)
{
    dirt::MipParams p{};
    int rc = mip_sample_check(who, pyramid, uvs, lod, rows, cols, image_rows, Ht, Wt, Ct, levels, uv_stride, mask_stride, mask, lod_bias, flags, p);
    if (rc) return rc;
    const long long n = rows * cols;
    if (n > 0 && !out) TEX_FAIL("%s: out is NULL", who);
    if (sc.batch && (rc = mip_sample_scenes(who, sc.count, p))) return rc;
    if (n == 0 || sc.none()) return dirt::stage_ok(report);
    p.out = out;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool a16 = (reinterpret_cast<uintptr_t>(pyramid) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;   // (four channels: every scene's, as scene 0's)
    dirt::dispatch_channels(Ct, a16, [&](auto ct) { dirt::dispatch_scenes(sc, [&](auto b) {
        hipLaunchKernelGGL((dirt::mip_forward_kernel<decltype(ct)::value, decltype(b)::value>), dirt::scene_grid(dirt::capped_blocks(n), sc), dim3(256), 0, s, p);
    }); });
    return dirt::stage_hip(report, who, hipGetLastError());
}

static int mip_sample_backward(const char* who, dirt::Scenes sc, const float* pyramid, const float* uvs, const float* lod, const float* mask,
                               const float* grad_out, float* grad_pyramid, float* grad_texture, float* grad_uvs, float* grad_lod, long long rows, long long cols,
                               int image_rows, int Ht, int Wt, int Ct, int levels, int uv_stride, int grad_uv_stride, int mask_stride, float lod_bias,
                               unsigned flags, void* stream)
{
    dirt::MipParams p{};
    int rc = mip_sample_check(who, pyramid, uvs, lod, rows, cols, image_rows, Ht, Wt, Ct, levels, uv_stride, mask_stride, mask, lod_bias, flags, p);
    if (rc) return rc;
    if (!grad_pyramid || !grad_texture) TEX_FAIL("%s: grad_pyramid / grad_texture is NULL", who);
    const long long n = rows * cols;
    if (n > 0 && !grad_out) TEX_FAIL("%s: grad_out is NULL", who);
    if (grad_uvs && grad_uv_stride < 2) TEX_FAIL("%s: grad_uv_stride < 2", who);
    if (grad_lod && !lod) TEX_FAIL("%s: grad_lod needs lod", who);
    p.grad_out = grad_out; p.grad_pyr = grad_pyramid; p.grad_uvs = grad_uvs; p.grad_lod = grad_lod; p.guv_stride = grad_uv_stride;
    if (sc.batch && (rc = mip_sample_scenes(who, sc.count, p))) return rc;
    const dirt::TileGrid t = dirt::tile_grid(rows, cols);
    if (t.tiles > 0x7fffffffll) TEX_FAIL("%s: pixel grid too large", who);
    if (sc.none()) return dirt::stage_ok(report);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = dirt::clear_floats(grad_pyramid, dirt::mip_floats(p) * sc.count, s);
    if (e != hipSuccess) return dirt::stage_hip(report, who, e);
    if (n > 0) {
        const bool a16 = (reinterpret_cast<uintptr_t>(grad_out) & 15u) == 0;
        dirt::dispatch_channels(Ct, a16, [&](auto ct) { dirt::dispatch_scenes(sc, [&](auto b) {
            hipLaunchKernelGGL((dirt::mip_backward_kernel<decltype(ct)::value, decltype(b)::value>), dirt::scene_grid((unsigned)t.tiles, sc), dim3(256), 0, s, p, t.tw,
                               t.th, (int)t.tiles_x);
        }); });
        e = hipGetLastError();
        if (e != hipSuccess) return dirt::stage_hip(report, who, e);
    }
    // (the collapse reports under its own entry point's name)
    return mip_collapse(sc.batch ? "dirt_texture_mip_collapse_batch" : "dirt_texture_mip_collapse", sc, grad_pyramid, grad_texture, Ht, Wt, Ct, levels, stream);
}

int dirt_texture_sample_mip_forward(const float* pyramid, const float* uvs, const float* lod, const float* mask, float* out, long long rows,
                                    long long cols, int image_rows, int Ht, int Wt, int Ct, int levels, int uv_stride, int mask_stride,
                                    float lod_bias, unsigned flags, void* stream)
{
    return mip_sample_forward("dirt_texture_sample_mip_forward", dirt::ONE_TEXTURE, pyramid, uvs, lod, mask, out, rows, cols, image_rows, Ht, Wt, Ct, levels,
                              uv_stride, mask_stride, lod_bias, flags, stream);
}

int dirt_texture_sample_mip_batch_forward(const float* pyramids, const float* uvs, const float* lod, const float* mask, float* out, long long scenes,
                                          long long rows, long long cols, int image_rows, int Ht, int Wt, int Ct, int levels, int uv_stride,
                                          int mask_stride, float lod_bias, unsigned flags, void* stream)
{
    return mip_sample_forward("dirt_texture_sample_mip_batch_forward", {true, scenes}, pyramids, uvs, lod, mask, out, rows, cols, image_rows, Ht, Wt, Ct,
                              levels, uv_stride, mask_stride, lod_bias, flags, stream);
}

int dirt_texture_sample_mip_backward(const float* pyramid, const float* uvs, const float* lod, const float* mask, const float* grad_out,
                                     float* grad_pyramid, float* grad_texture, float* grad_uvs, float* grad_lod, long long rows, long long cols,
                                     int image_rows, int Ht, int Wt, int Ct, int levels, int uv_stride, int grad_uv_stride, int mask_stride,
                                     float lod_bias, unsigned flags, void* stream)
{
    return mip_sample_backward("dirt_texture_sample_mip_backward", dirt::ONE_TEXTURE, pyramid, uvs, lod, mask, grad_out, grad_pyramid, grad_texture, grad_uvs, grad_lod,
                               rows, cols, image_rows, Ht, Wt, Ct, levels, uv_stride, grad_uv_stride, mask_stride, lod_bias, flags, stream);
}

int dirt_texture_sample_mip_batch_backward(const float* pyramids, const float* uvs, const float* lod, const float* mask, const float* grad_out,
                                           float* grad_pyramids, float* grad_textures, float* grad_uvs, float* grad_lod, long long scenes,
                                           long long rows, long long cols, int image_rows, int Ht, int Wt, int Ct, int levels, int uv_stride,
                                           int grad_uv_stride, int mask_stride, float lod_bias, unsigned flags, void* stream)
{
    return mip_sample_backward("dirt_texture_sample_mip_batch_backward", {true, scenes}, pyramids, uvs, lod, mask, grad_out, grad_pyramids, grad_textures, grad_uvs,
                               grad_lod, rows, cols, image_rows, Ht, Wt, Ct, levels, uv_stride, grad_uv_stride, mask_stride, lod_bias,
                               flags, stream);
}

}  // extern "C"
