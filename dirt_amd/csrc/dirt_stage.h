// dirt_stage.h -- what the fused stages around the rasteriser share, each piece written and explained once here:
//   texture look-up   (dirt_texture.hip, dirt_texture_mip.hip, dirt_texture_cube.hip; what only those three share -- the per-look-up arithmetic, the backward tile scheme, the pixel grid -- is dirt_texture_common.h; a cube look-up's own arithmetic, which dirt_shade_ibl.hip uses too, is dirt_texture_cube.h);
//   G-buffer lighting (dirt_shade.hip, dirt_shade_sh.hip, dirt_shade_pbr.hip, dirt_shade_ibl.hip; what only these and dirt_normal_map.hip share -- the tile walk, the clamp, the host checks, the backward's epilogue -- is dirt_shade_common.h);
//   vertex stage      (dirt_geometry.hip);
//   skinning          (dirt_skin.hip: Float3 / Float4 / load3 / store3, dot3, the wave sum, the four-wave fold, the error channel, the scratch check);
//   kinematics        (dirt_kinematics.hip: Float4 / load3 / store3, dot3, the error channel, the scratch check);
//   blend shapes      (dirt_blend.hip: Float4 / load3 / store3, load_quad / store_quad, the wave sum, the four-wave fold, the error channel, the scratch check);
//   normal mapping    (dirt_tangent.hip, dirt_normal_map.hip: Float4 / load3 / store3, dot3 / cross3, the error channel, the scratch check).
// Device side: the 12- and 16-byte accesses to rows that are only 4-byte aligned (Float3 of dirt_device.h, Float4, load3 /
// store3: all four; load_quad / store_quad, a quad of a row with its zero-padded tail: blend shapes), dot3 / cross3 (shade, geometry), the all-lanes wave sum, the fold of a workgroup's four waves into its
// row of partial sums and the fixed-order sum of a column of such rows (shade, geometry: their parameter and matrix gradients).
// Host side: the two error channels and the helpers that report into either (all four, and dirt_capi.hip for the first
// channel), the scratch check (shade, geometry), the channel-count dispatch and the capped grid of a grid-stride launch
// (texture, mip).  NOT shared: the two reduce kernels themselves -- geometry's early exit for a matrix shared by the scenes and
// its two outputs are real differences -- and what precedes the fold in a kernel: the lane-0 writes (geometry writes two
// columns per step), the barrier and the `tid < N`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>
#include "../../include/dirt_hip.h"
#include "dirt_device.h"

namespace dirt {

// ---- device ---------------------------------------------------------------------------------------------------------------

struct Float4 { float x, y, z, w; };   // four consecutive floats, 4-byte aligned (a float4 would promise 16): one 16-byte access

// three consecutive floats, 4-byte aligned: one 12-byte access
__device__ __forceinline__ void load3(const float* __restrict__ p, float (&v)[3])
{
    const Float3 t = *reinterpret_cast<const Float3*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z;
}
__device__ __forceinline__ void store3(float* p, const float (&v)[3]) { *reinterpret_cast<Float3*>(p) = Float3{v[0], v[1], v[2]}; }

// four consecutive elements e .. e + 3 of a 4-byte aligned row of E floats in one 16-byte access; at the end of the row the
// elements past it read as zero and are not written
__device__ __forceinline__ void load_quad(const float* __restrict__ row, int e, int E, float (&x)[4])
{
    if (e + 4 <= E) {
        const Float4 q = *reinterpret_cast<const Float4*>(row + e);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = e + i < E ? row[e + i] : 0.f;
    }
}

__device__ __forceinline__ void store_quad(float* row, int e, int E, const float (&x)[4])
{
    if (e + 4 <= E) {
        *reinterpret_cast<Float4*>(row + e) = Float4{x[0], x[1], x[2], x[3]};
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e + i < E) row[e + i] = x[i];
    }
}

__device__ __forceinline__ float dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], float (&c)[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- the sum of a value over the 64 lanes of a wave, in every lane, in a fixed tree: DPP adds inside the rows of 16, then the four rows
template <int CTRL>
__device__ __forceinline__ float wave_dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

__device__ __forceinline__ float wave_sum(float v)
{
    v += wave_dpp<0xB1>(v);    // quad_perm [1,0,3,2]
    v += wave_dpp<0x4E>(v);    // quad_perm [2,3,0,1]
    v += wave_dpp<0x141>(v);   // row_half_mirror: the other quad of the eight
    v += wave_dpp<0x140>(v);   // row_mirror: the other eight of the row
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}

// ---- a workgroup of four waves leaves ONE row of N partial sums in caller-owned scratch.  Lane 0 of wave w has written its
// wave's sum of value k to s_part[w * N + k] (4 N floats of LDS) and the workgroup has synchronised; lane tid < N adds the four
// rows' value tid in a fixed tree and stores it to row (blockIdx.y, blockIdx.x) of partial [gridDim.y, gridDim.x, N].
// (The barrier and the `tid < N` stay with the caller: with them in here the kernels' blocks were laid out differently.)
template <int N>
__device__ __forceinline__ void fold_waves_to_row(const float* s_part, float* partial, int tid)
{
    const float s = (s_part[tid] + s_part[N + tid]) + (s_part[2 * N + tid] + s_part[3 * N + tid]);
    partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * N + tid] = s;
}

// ---- the sum of base[0], base[stride], ..., `rows` values, by a workgroup of BLOCK lanes in a fixed order: lane t takes rows
// t, t + BLOCK, ..., then the lanes fold in s_sum (BLOCK floats of LDS).  No atomics, and the same bits on every run.  The
// total is for lane 0 to use.
template <int BLOCK>
__device__ __forceinline__ float block_column_sum(const float* base, long long rows, int stride, float* s_sum)
{
    const int tid = threadIdx.x;
    float s = 0.f;
    for (long long r = tid; r < rows; r += BLOCK) s += base[r * stride];
    s_sum[tid] = s;
    __syncthreads();
    for (int h = BLOCK / 2; h > 0; h >>= 1) {
        if (tid < h) s_sum[tid] += s_sum[tid + h];
        __syncthreads();
    }
    return s_sum[0];
}

// ---- host -----------------------------------------------------------------------------------------------------------------

// The library has TWO error channels, each a thread-local buffer that only the function defined next to it writes
// (printf-style; "" clears it; returns `code`):
//   set_last_error    -> dirt_last_error()         (dirt_capi.hip):    the rasteriser, shade, geometry;
//   set_texture_error -> dirt_texture_last_error() (dirt_texture.hip): the texture and mip entry points.
int set_last_error(int code, const char* fmt, ...);
int set_texture_error(int code, const char* fmt, ...);
using ErrorSetter = int (*)(int code, const char* fmt, ...);

// the formatting of both: at most size - 1 characters, always terminated
inline void format_error(char* buf, size_t size, const char* fmt, va_list ap) { vsnprintf(buf, size, fmt, ap); }

// a refused argument, one macro per channel; the helpers below take the channel as `set`
#define STAGE_FAIL(...) return dirt::set_last_error(DIRT_E_INVALID_ARGUMENT, __VA_ARGS__)
#define TEX_FAIL(...) return dirt::set_texture_error(DIRT_E_INVALID_ARGUMENT, __VA_ARGS__)

// success clears the channel
inline int stage_ok(ErrorSetter set) { return set(DIRT_OK, "%s", ""); }

inline int stage_hip(ErrorSetter set, const char* who, hipError_t e)
{
    if (e != hipSuccess) return set(DIRT_E_HIP, "%s: %s", who, hipGetErrorString(e));
    return stage_ok(set);
}

// caller-owned scratch: there, at least `need` bytes (what `sizer`, the entry point's ..._scratch_bytes, returns), 4-byte aligned
inline int check_scratch(ErrorSetter set, const char* who, const void* scratch, size_t bytes, size_t need, const char* sizer)
{
    if (!scratch || bytes < need)
        return set(DIRT_E_INVALID_ARGUMENT, "%s: scratch is NULL or smaller than %s (%zu < %zu)", who, sizer, bytes, need);
    if (reinterpret_cast<uintptr_t>(scratch) & 3u) return set(DIRT_E_INVALID_ARGUMENT, "%s: scratch is not 4-byte aligned", who);
    return DIRT_OK;
}

// f(std::integral_constant<int, CT>) for the kernel instantiation of a texture of Ct channels: 4 (when `a16`: every pointer the
// kernel reads or writes as float4 is 16-byte aligned -- which pointers those are differs per launch), 3, 1, or 0 = any count
template <class F>
inline void dispatch_channels(int Ct, bool a16, F&& f)
{
    if (Ct == 4 && a16) f(std::integral_constant<int, 4>{});
    else if (Ct == 3) f(std::integral_constant<int, 3>{});
    else if (Ct == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}

// workgroups of 256 lanes for a grid-stride loop over n elements, at most 256 * 64 of them
inline unsigned capped_blocks(long long n)
{
    const long long blocks = (n + 255) / 256;
    return (unsigned)(blocks > 256 * 64 ? 256 * 64 : blocks);
}

}  // namespace dirt
