// dirt_texture_cube.hip -- cube-map look-up of a deferred shader (an environment map indexed by a direction), and its gradient.
//
// Replaces no reference interface: the reference's samples/textured.py:16-61 indexes one flat texture by (u, v).  A cube map is six
// flat textures, so the per-look-up arithmetic and the backward tile scheme are those of dirt_texture.hip / dirt_texture_mip.hip
// (dirt_texture_common.h).  The specification (DESIGN.md §7 restates it; tests/cube_reference.py implements it in numpy):
//
//  1. Operands.  cube [6, N, N, Ct], faces in OpenGL order +X, -X, +Y, -Y, +Z, -Z; directions (x, y, z), not normalised.
//  2. Validity.  A direction is valid iff x, y, z are finite and a = max(|x|, |y|, |z|) > 0.  An invalid look-up returns 0 in every
//     channel and adds to no gradient (its grad_directions row and its grad_lod are 0): a G-buffer's background needs no mask.
//  3. Face.  X if |x| >= |y| and |x| >= |z|, otherwise Y if |y| >= |z|, otherwise Z; the positive face if the major component is > 0.
//     (sc, tc) = +X (-z, -y), -X (+z, -y), +Y (+x, +z), -Y (+x, -z), +Z (+x, -y), -Z (-x, -y).
//  4. Index at a level of size n (n = N at level 0), one float32 operation per step: col = ((sc / a + 1) * 0.5) * n - 0.5, clamped to
//     [0, n - 1]; row the same from tc.  Texel centres as in GL, clamp-to-edge per face: taps never cross to a neighbouring face.  Then
//     bilinear_taps / bilinear_blend; 'nearest' takes texel (texel_index(row + 0.5), texel_index(col + 0.5)).  d col / d (sc / a) is
//     n / 2 where the unclamped value lies in [0, n - 1] (bounds included), else 0.
//  5. Trilinear.  A pyramid per face, as dirt_texture_mip_build_batch makes it of the six faces; lambda = lod + lod_bias; the level
//     split, the blend and the lod gradient are those of dirt_texture_mip.hip (spec 4, 5 there).  Each level takes its own index from
//     (sc, tc, a) with its own n.
//  6. Gradients to the cube, the directions (that of (sc / a, tc / a): orthogonal to the direction) and lod.
//
// The per-look-up arithmetic of spec 2-4 and 6 is dirt_texture_cube.h, which dirt_shade_ibl.hip shares; that unit also launches
// this one's backward kernels (cube_backward_launch, at the end of this file) for the scatter into its two cubes.
// Kernels: the forward one look-up per lane.  The backward on 16 x 16-pixel tiles (256 x 1 of a flat list): a bilinear / nearest tile
// whose valid look-ups lie on ONE face and whose taps' bounding box fits TEX_PATCH texels sums in an LDS patch and sends each touched
// texel to memory once; a tile that straddles a face edge, or whose box is larger, adds straight to memory.  The trilinear backward
// does the same with a patch per touched level (at most two adjacent ones) of the pyramid-shaped scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_texture_cube.h"

namespace dirt {

// ---- forward: one look-up per lane, CT channels per access ----
template <int CT>
__global__ __launch_bounds__(256) void texture_cube_forward_kernel(CubeParams p)
{
    const bool nearest = (p.flags & DIRT_TEX_NEAREST) != 0;
    const int Ct = CT ? CT : p.Ct;
    constexpr int NV = CT ? CT : 1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += (long long)gridDim.x * blockDim.x) {
        float d[3];
        load3(p.dirs + i * p.dir_stride, d);
        const CubeLook q = cube_look(d[0], d[1], d[2]);
        float* __restrict__ out = p.out + i * Ct;
        if (!q.valid) {
            for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) { float o[NV]; for (int j = 0; j < NV; ++j) o[j] = 0.f; store_ch<CT>(out, o, ch); }
            continue;
        }
        const float* __restrict__ face = p.pyr + (size_t)q.face() * p.face_floats;
        int l = 0; float f = 0.f;
        if (p.lod) mip_split(p.lod[i] + p.lod_bias, p.L, l, f);
        float dr, dc;
        const int n0 = mip_dim(p.N, l);
        const Taps k0 = cube_taps(q, n0, nearest, dr, dc);
        const float* __restrict__ lv0 = face + cube_level_offset(p.N, n0, Ct);
        if (nearest) {   // the texel itself, not a blend of weight 1
            const float* __restrict__ t = lv0 + ((size_t)k0.r0 * n0 + k0.c0) * Ct;
            for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) { float o[NV]; load_ch<CT>(t, Ct, o, ch); store_ch<CT>(out, o, ch); }
            continue;
        }
        if (f == 0.f) {
            for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) { float o[NV]; mip_sample<CT>(lv0, n0, k0, Ct, ch, o); store_ch<CT>(out, o, ch); }
            continue;
        }
        const int n1 = mip_dim(p.N, l + 1);
        const Taps k1 = cube_taps(q, n1, false, dr, dc);
        const float* __restrict__ lv1 = face + cube_level_offset(p.N, n1, Ct);
        const float g = 1.f - f;
        for (int ch = 0; ch < (CT ? 1 : Ct); ++ch) {
            float a[NV], b[NV], o[NV];
            mip_sample<CT>(lv0, n0, k0, Ct, ch, a); mip_sample<CT>(lv1, n1, k1, Ct, ch, b);
#pragma unroll
            for (int j = 0; j < NV; ++j) o[j] = g * a[j] + f * b[j];
            store_ch<CT>(out, o, ch);
        }
    }
}

// lane `tid`'s look-up of the backward kernels: false outside the pixel grid and for an invalid direction
__device__ __forceinline__ bool cube_tile_look(const CubeParams& p, int tid, int rows, int cols, int tw, int th, int tiles_x, long long& i, bool& active, CubeLook& q)
{
    active = tile_pixel(tid, tw, th, tiles_x, rows, cols, i);
    float d[3] = {0.f, 0.f, 0.f};
    if (active) load3(p.dirs + i * p.dir_stride, d);
    q = cube_look(d[0], d[1], d[2]);
    return active && q.valid;
}

// ---- backward, bilinear / nearest: the tile scheme of dirt_texture_common.h with one patch, on the face the tile's look-ups share
template <int CT>
__global__ __launch_bounds__(256) void texture_cube_backward_kernel(CubeParams p, int rows, int cols, int tw, int th, int tiles_x)
{
    constexpr int LCT = CT ? CT : 4;                 // channels per LDS patch pass (any count: passes of 4)
    __shared__ float s_acc[TEX_PATCH * LCT];
    __shared__ int s_box[6];                         // rmin, rmax, cmin, cmax of the tile's taps; the lowest and highest face
    const bool nearest = (p.flags & DIRT_TEX_NEAREST) != 0;
    const int Ct = CT ? CT : p.Ct;
    const int tid = threadIdx.x;
    long long i;
    bool active;
    CubeLook q;
    const bool valid = cube_tile_look(p, tid, rows, cols, tw, th, tiles_x, i, active, q);
    if (tid == 0) { box_clear(s_box); s_box[4] = 6; s_box[5] = -1; }
    float drow, dcol;
    const Taps k = cube_taps(q, p.N, nearest, drow, dcol);
    const int face = q.face();
    __syncthreads();
    if (valid) { box_add(s_box, k); atomicMin(&s_box[4], face); atomicMax(&s_box[5], face); }
    __syncthreads();
    const int rmin = s_box[0], cmin = s_box[2];
    const int bh = s_box[1] - rmin + 1, bw = s_box[3] - cmin + 1;
    const bool patch = s_box[4] == s_box[5] && bh > 0 && bw > 0 && (long long)bh * bw <= TEX_PATCH;   // (workgroup-uniform; no valid look-up: no patch)
    const Four<float> w = {k.wc0 * k.wr0, k.fc * k.wr0, k.wc0 * k.fr, k.fc * k.fr};
    float d_fr = 0.f, d_fc = 0.f;
    const float* __restrict__ gout = p.grad_out + i * Ct;
    const float* __restrict__ tex = p.pyr + (size_t)face * p.face_floats;        // level 0 of the lane's face
    float* __restrict__ gtex = p.grad_pyr + (size_t)face * p.face_floats;
    float* __restrict__ gbox = p.grad_pyr + (size_t)(patch ? s_box[4] : 0) * p.face_floats;   // ... of the tile's face
    for (int c0 = 0; c0 < Ct; c0 += LCT) {          // (CT = 1, 3, 4: one pass; any other count: passes of four channels)
        const int nc = CT ? CT : min(LCT, Ct - c0);
        if (patch) {
            clear_patch(s_acc, bh * bw * LCT, tid);
            __syncthreads();
        }
        if (valid) {
            float g[LCT];
            load_grad_out<CT>(gout, Ct, c0, nc, g);
            const Four<size_t> o = tap_offsets(k, p.N, Ct, c0);
            const Four<int> l = patch_offsets(k, rmin, cmin, bw, LCT);
#pragma unroll
            for (int j = 0; j < LCT; ++j) {
                if (j >= nc) break;
                if (!nearest) {
                    float e_fr, e_fc;
                    tap_gradients(g[j], {tex[o.tl + j], tex[o.tr + j], tex[o.bl + j], tex[o.br + j]}, k, e_fr, e_fc);
                    d_fr += e_fr; d_fc += e_fc;
                }
                if (patch) {
                    if (nearest) { atomicAdd(&s_acc[l.tl + j], g[j]); continue; }
                    add_taps(s_acc, l, j, g[j], w);
                } else {
                    if (nearest) { atomicAdd(&gtex[o.tl + j], g[j]); continue; }
                    add_taps(gtex, o, j, g[j], w);
                }
            }
        }
        if (patch) {
            __syncthreads();
            for (int e = tid; e < bh * bw * LCT; e += 256) {   // (as texture_backward_kernel's)
                const float val = s_acc[e];
                const int j = e % LCT, t = e / LCT;
                if (val != 0.f && j < nc) atomicAdd(&gbox[box_texel(t, rmin, cmin, bw, p.N, Ct) + c0 + j], val);
            }
            __syncthreads();
        }
    }
    if (active && p.grad_dirs) {   // floor() has zero gradient: d frac / d index = 1 (nearest, invalid: zero)
        float g[3] = {0.f, 0.f, 0.f};
        if (valid && !nearest) cube_direction_gradient(q, d_fc * dcol, d_fr * drow, g);
        store3(p.grad_dirs + i * p.gdir_stride, g);
    }
}

// ---- backward, trilinear: the tile scheme with one LDS patch per touched level, as mip_backward_kernel of dirt_texture_mip.hip.  A
// lane's look-up has up to two tap sets: level l with weight 1 - f and level l + 1 with weight f (when f != 0).  Where the tile's valid
// look-ups lie on ONE face, their sets span at most two adjacent levels and both bounding boxes fit TEX_PATCH texels together, each set
// sums into its level's patch; otherwise they add straight into the scratch pyramid.
template <int CT>
__global__ __launch_bounds__(256) void texture_cube_backward_mip_kernel(CubeParams p, int rows, int cols, int tw, int th, int tiles_x)
{
    constexpr int LCT = CT ? CT : 4;
    __shared__ float s_acc[TEX_PATCH * LCT];
    __shared__ int s_box[12];   // lmin, lmax, the lowest and highest face, then rmin, rmax, cmin, cmax of the two levels' taps
    const int Ct = CT ? CT : p.Ct;
    const int tid = threadIdx.x;
    long long i;
    bool active;
    CubeLook q;
    const bool valid = cube_tile_look(p, tid, rows, cols, tw, th, tiles_x, i, active, q);
    if (tid == 0) {
        s_box[0] = 0x7fffffff; s_box[1] = -1; s_box[2] = 6; s_box[3] = -1;
        for (int s = 0; s < 2; ++s) box_clear(&s_box[4 + 4 * s]);
    }
    float lam = 0.f;
    if (valid) lam = p.lod[i] + p.lod_bias;
    int l; float f;
    mip_split(lam, p.L, l, f);
    const bool inside = lam > 0.f && lam < (float)(p.L - 1);        // d out / d lambda is S_{l+1} - S_l here, 0 where clamped
    const bool want_lod = p.grad_lod && inside && valid;
    const bool two = f != 0.f;                                       // the second set carries weight
    const bool read1 = two || want_lod;                              // ... or is read for the lod gradient only
    const int n0 = mip_dim(p.N, l), n1 = mip_dim(p.N, read1 ? l + 1 : l);
    float dr0, dc0, dr1, dc1;
    const Taps k0 = cube_taps(q, n0, false, dr0, dc0), k1 = cube_taps(q, n1, false, dr1, dc1);
    const int face = q.face();
    __syncthreads();
    if (valid) { atomicMin(&s_box[0], l); atomicMax(&s_box[1], two ? l + 1 : l); atomicMin(&s_box[2], face); atomicMax(&s_box[3], face); }
    __syncthreads();
    const int lmin = s_box[0];
    const bool span = s_box[2] == s_box[3] && s_box[1] - lmin <= 1;   // (no valid look-up: the faces are 6 and -1)
    if (valid && span) {
        box_add(&s_box[4 + 4 * (l - lmin)], k0);
        if (two) box_add(&s_box[4 + 4 * (l + 1 - lmin)], k1);
    }
    __syncthreads();
    int pr0[2], pc0[2], pw[2], pbase[2];
    int used = 0;
    for (int s = 0; s < 2; ++s) {
        const int bh = s_box[5 + 4 * s] - s_box[4 + 4 * s] + 1, bw = s_box[7 + 4 * s] - s_box[6 + 4 * s] + 1;
        pr0[s] = s_box[4 + 4 * s]; pc0[s] = s_box[6 + 4 * s];
        pw[s] = bh > 0 && bw > 0 ? bw : 0;
        pbase[s] = used;
        if (bh > 0 && bw > 0) used += (long long)bh * bw > TEX_PATCH ? TEX_PATCH + 1 : bh * bw;
    }
    const bool patch = span && used > 0 && used <= TEX_PATCH;   // (workgroup-uniform)
    const size_t base = (size_t)face * p.face_floats;                               // the lane's face
    float* __restrict__ gbox = p.grad_pyr + (size_t)(patch ? s_box[2] : 0) * p.face_floats;   // the tile's
    const long long off0 = cube_level_offset(p.N, n0, Ct), off1 = cube_level_offset(p.N, n1, Ct);
    const float w0 = 1.f - f;
    float d_fr0 = 0.f, d_fc0 = 0.f, d_fr1 = 0.f, d_fc1 = 0.f, d_lod = 0.f;
    const float* __restrict__ gout = p.grad_out + i * Ct;
    for (int c0 = 0; c0 < Ct; c0 += LCT) {
        const int nc = CT ? CT : min(LCT, Ct - c0);
        if (patch) {
            clear_patch(s_acc, used * LCT, tid);
            __syncthreads();
        }
        if (valid) {
            float g[LCT];
            load_grad_out<CT>(gout, Ct, c0, nc, g);
            for (int set = 0; set < 2; ++set) {
                if (set == 1 && !read1) break;   // the second set: read for the lod gradient, added only where it carries weight
                const Taps& k = set ? k1 : k0;
                const float* __restrict__ lv = p.pyr + base + (set ? off1 : off0);
                float* __restrict__ gv = p.grad_pyr + base + (set ? off1 : off0);
                const float w = set ? f : w0;
                const bool scatter = set == 0 || two;
                const int ps = l + set - lmin;
                const Four<float> wt = {(k.wc0 * k.wr0) * w, (k.fc * k.wr0) * w, (k.wc0 * k.fr) * w, (k.fc * k.fr) * w};
                const Four<size_t> o = tap_offsets(k, set ? n1 : n0, Ct, c0);
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
            for (int e = tid; e < used * LCT; e += 256) {   // (as mip_backward_kernel's; a texel lies in the first level's box or the second's)
                const float val = s_acc[e];
                const int j = e % LCT, t = e / LCT;
                if (val != 0.f && j < nc) {
                    const int s = t >= pbase[1] && pw[1] > 0 ? 1 : 0;
                    const int nk = mip_dim(p.N, lmin + s);
                    atomicAdd(&gbox[cube_level_offset(p.N, nk, Ct) + box_texel(t - pbase[s], pr0[s], pc0[s], pw[s], nk, Ct) + c0 + j], val);
                }
            }
            __syncthreads();
        }
    }
    if (!active) return;
    if (p.grad_dirs) {   // (an invalid look-up: zero)
        float g[3] = {0.f, 0.f, 0.f};
        const float gs = (d_fc0 * dc0) * w0 + (two ? (d_fc1 * dc1) * f : 0.f);
        const float gt = (d_fr0 * dr0) * w0 + (two ? (d_fr1 * dr1) * f : 0.f);
        if (valid) cube_direction_gradient(q, gs, gt, g);
        store3(p.grad_dirs + i * p.gdir_stride, g);
    }
    if (p.grad_lod) p.grad_lod[i] = want_lod ? d_lod : 0.f;
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_texture_error;   // the error channel of this file's entry points

// what both entry points refuse, before any device work; fills what they share of `p`
static int cube_check(const char* who, const float* pyramid, const float* directions, const float* lod, long long n, int size, int channels,
                      int levels, int dir_stride, float lod_bias, unsigned flags, dirt::CubeParams& p)
{
    if (flags & ~DIRT_TEX_NEAREST) TEX_FAIL("%s: flags 0x%x: a cube look-up takes DIRT_TEX_NEAREST only (its faces clamp to their edges)", who, flags);
    if ((flags & DIRT_TEX_NEAREST) && lod) TEX_FAIL("%s: DIRT_TEX_NEAREST does not apply to a trilinear look-up (lod given)", who);
    if (n < 0 || size < 1 || channels < 1 || dir_stride < 3)
        TEX_FAIL("%s: bad sizes (n=%lld size=%d channels=%d dir_stride=%d)", who, n, size, channels, dir_stride);
    const int most = dirt::mip_level_count(size, size, -1);
    if (levels < 1 || levels > most) TEX_FAIL("%s: %d levels, a %d x %d face has 1..%d", who, levels, size, size, most);
    if (n > 0 && (!pyramid || !directions)) TEX_FAIL("%s: pyramid / directions is NULL", who);
    p.pyr = pyramid; p.dirs = directions; p.lod = lod; p.n = n; p.N = size; p.Ct = channels; p.L = levels; p.dir_stride = dir_stride;
    p.lod_bias = lod_bias; p.flags = flags;
    p.face_floats = dirt::cube_level_offset(size, dirt::mip_dim(size, levels - 1), channels) + (long long)dirt::mip_dim(size, levels - 1) * dirt::mip_dim(size, levels - 1) * channels;
    return DIRT_OK;
}

int dirt_texture_cube_forward(const float* pyramid, const float* directions, const float* lod, float* out, long long n, int size, int channels,
                              int levels, int dir_stride, float lod_bias, unsigned flags, void* stream)
{
    const char* who = "dirt_texture_cube_forward";
    dirt::CubeParams p{};
    int rc = cube_check(who, pyramid, directions, lod, n, size, channels, levels, dir_stride, lod_bias, flags, p);
    if (rc) return rc;
    if (n > 0 && !out) TEX_FAIL("%s: out is NULL", who);
    if (n == 0) return dirt::stage_ok(report);
    p.out = out;
    const bool a16 = (reinterpret_cast<uintptr_t>(pyramid) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;   // (four channels: every face and level starts a multiple of 16 bytes in)
    dirt::dispatch_channels(channels, a16, [&](auto ct) {
        hipLaunchKernelGGL(dirt::texture_cube_forward_kernel<decltype(ct)::value>, dim3(dirt::capped_blocks(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
    });
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_texture_cube_backward(const float* pyramid, const float* directions, const float* lod, const float* grad_out, float* grad_pyramid,
                               float* grad_directions, float* grad_lod, long long rows, long long cols, int size, int channels, int levels,
                               int dir_stride, int grad_dir_stride, float lod_bias, unsigned flags, void* stream)
{
    const char* who = "dirt_texture_cube_backward";
    dirt::CubeParams p{};
    int rc = dirt::check_pixel_grid(who, rows, cols);
    if (!rc) rc = cube_check(who, pyramid, directions, lod, rows * cols, size, channels, levels, dir_stride, lod_bias, flags, p);
    if (rc) return rc;
    const long long n = rows * cols;
    if (n > 0 && (!grad_out || !grad_pyramid)) TEX_FAIL("%s: grad_out / grad_pyramid is NULL", who);
    if (grad_directions && grad_dir_stride < 3) TEX_FAIL("%s: grad_dir_stride < 3", who);
    if (grad_lod && !lod) TEX_FAIL("%s: grad_lod needs lod", who);
    const dirt::TileGrid t = dirt::tile_grid(rows, cols);
    if (t.tiles > 0x7fffffffll || cols > 0x7fffffffll || rows > 0x7fffffffll) TEX_FAIL("%s: pixel grid too large (rows=%lld cols=%lld)", who, rows, cols);
    if (!grad_pyramid) return dirt::stage_ok(report);   // (n == 0 without a gradient buffer: nothing to clear)
    p.grad_out = grad_out; p.grad_pyr = grad_pyramid; p.grad_dirs = grad_directions; p.grad_lod = grad_lod; p.gdir_stride = grad_dir_stride;
    return dirt::stage_hip(report, who, dirt::cube_backward_launch(p, rows, cols, reinterpret_cast<hipStream_t>(stream)));
}

}  // extern "C"

namespace dirt {

// (dirt_texture_cube.h)
hipError_t cube_backward_launch(const CubeParams& p, long long rows, long long cols, hipStream_t s)
{
    hipError_t e = clear_floats(p.grad_pyr, 6 * p.face_floats, s);
    if (e != hipSuccess || p.n <= 0) return e;
    const TileGrid t = tile_grid(rows, cols);
    const bool a16 = (reinterpret_cast<uintptr_t>(p.grad_out) & 15u) == 0;
    dispatch_channels(p.Ct, a16, [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        if (p.lod) hipLaunchKernelGGL(texture_cube_backward_mip_kernel<CT>, dim3((unsigned)t.tiles), dim3(256), 0, s, p, (int)rows, (int)cols, t.tw, t.th, (int)t.tiles_x);
        else hipLaunchKernelGGL(texture_cube_backward_kernel<CT>, dim3((unsigned)t.tiles), dim3(256), 0, s, p, (int)rows, (int)cols, t.tw, t.th, (int)t.tiles_x);
    });
    return hipGetLastError();
}

}  // namespace dirt
