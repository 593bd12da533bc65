// dirt_texture_common.h -- the per-look-up arithmetic shared by the texture kernels (dirt_texture.hip: nearest / bilinear;
// dirt_texture_mip.hip: trilinear over a mip pyramid): (u, v) -> fractional (row, column) index of the reference's
// samples/textured.py:16-26, the four bilinear taps of :36-60 and the channel-vector loads / stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_stage.h"

namespace dirt {

// tf.clip_by_value(x, 0, 1) = minimum(maximum(x, 0), 1), which keeps a NaN (fminf / fmaxf would return the bound instead)
__device__ __forceinline__ float clip01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// samples/textured.py:16-26: (u, v) -> fractional (row, column) index
__device__ __forceinline__ void uv_to_index(float u, float v, int Ht, int Wt, bool clamp_mode, float& row, float& col, float& drow_dv,
                                            float& dcol_du)
{
    if (clamp_mode) {
        row = clip01(v) * (float)Ht;
        col = clip01(u) * (float)Wt;
        drow_dv = (v >= 0.f && v <= 1.f) ? (float)Ht : 0.f;   // the gradient of clip_by_value
        dcol_du = (u >= 0.f && u <= 1.f) ? (float)Wt : 0.f;
    } else {
        row = (v - floorf(v)) * (float)Ht;                    // uvs % 1. (floor-mod)
        col = (u - floorf(u)) * (float)Wt;
        drow_dv = (float)Ht; dcol_du = (float)Wt;
    }
}

// One texel / output pixel of CT channels as a register array, with the widest access its size and alignment allow
// (CT = 4: 16 bytes; 3: 12; 1: 4; 0: any count `ct`, channel by channel).
template <int CT>
__device__ __forceinline__ void load_ch(const float* __restrict__ p, int ct, float (&v)[CT ? CT : 1], int ch0 = 0)
{
    if constexpr (CT == 4) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else if constexpr (CT == 3) load3(p, v);
    else v[0] = p[ch0];
}
template <int CT>
__device__ __forceinline__ void store_ch(float* __restrict__ p, const float (&v)[CT ? CT : 1], int ch0 = 0)
{
    if constexpr (CT == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else if constexpr (CT == 3) store3(p, v);
    else p[ch0] = v[0];
}

// A float index -> texel index in [0, n - 1] as min(max((int)x, 0), n - 1), with a NaN index (a NaN coordinate) taking 0:
// converting a NaN to int is undefined in C++, so the rule is written out here instead of being left to the compiler
__device__ __forceinline__ int texel_index(float x, int n) { return x >= 1.f ? min((int)fminf(x, (float)n), n - 1) : 0; }

// The four texels of a bilinear look-up (samples/textured.py:36-60) and their weights
struct Taps {
    int r0, r1, c0, c1;
    float fr, fc, wr0, wc0;
};
__device__ __forceinline__ Taps bilinear_taps(float row, float col, int Ht, int Wt)
{
    Taps t;
    const float fr0 = floorf(row), fc0 = floorf(col);
    t.fr = row - fr0; t.fc = col - fc0;   // frac_indices[..., :1] (row), [..., 1:] (column)
    t.r0 = texel_index(fr0, Ht); t.r1 = min(t.r0 + 1, Ht - 1);
    t.c0 = texel_index(fc0, Wt); t.c1 = min(t.c0 + 1, Wt - 1);
    t.wc0 = 1.f - t.fc; t.wr0 = 1.f - t.fr;
    return t;
}

// ---- p[0 .. n) = 0 on `stream`: how the backward entry points clear the buffer their kernels add into.  A kernel of the
// library's own, NOT hipMemsetAsync: captured in a graph (hipGraph, torch.cuda.graph), the runtime's memset node cleared the
// buffer on the first replay only -- from the second replay on, one float in four came back holding the float count
// (tests/test_texture_edges.py::test_a_captured_lookup_and_backward_replay_on_new_textures).  The floats before the first
// 16-byte boundary (`head`, < 4) and after the last one are stored one by one, the rest as float4.
static __global__ __launch_bounds__(256) void clear_floats_kernel(float* __restrict__ p, long long n, int head)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x, lanes = (long long)gridDim.x * 256;
    const long long quads = (n - head) / 4, tail = head + quads * 4;
    float4* __restrict__ q = reinterpret_cast<float4*>(p + head);
    for (long long i = lane; i < quads; i += lanes) q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < head) p[lane] = 0.f;
    if (lane < n - tail) p[tail + lane] = 0.f;
}

inline hipError_t clear_floats(float* p, long long n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const long long to_boundary = (4 - (long long)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3;
    const int head = (int)(to_boundary < n ? to_boundary : n);
    const long long quads = (n - head) / 4;
    hipLaunchKernelGGL(clear_floats_kernel, dim3(capped_blocks(quads > 0 ? quads : 1)), dim3(256), 0, stream, p, n, head);
    return hipGetLastError();
}

}  // namespace dirt
