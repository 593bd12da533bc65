// dirt_blend.hip -- blend shapes in front of the kinematics and skinning stages, fused: a template mesh, shape coefficients
// and a table of directions -> the rest-pose vertices and the rest-pose joint positions in one launch, and the gradients
// to the template and the coefficients without float atomics.
//
// Every body, hand and face model the later stages name (SMPL, MANO, SMPL-X, FLAME) makes its rest mesh as template +
// sum of coefficient x direction (identity shape, expression, pose correctives) and regresses its joints from the shaped
// mesh.  The specification (DESIGN.md §7f restates it; tests/blend_reference.py composes it in float64), per scene, E = 3 V
// elements, K directions of which the first Ks move the joints:
//
//     vertices[e] = template[e] + sum over k < K of c[k] * directions[k, e]
//     joints[j]   = sum over the non-zeros (j, v) of the regressor of w[j, v] * template[v]
//                 + sum over k < Ks of c[k] * joint_directions[k, j]           (joint_directions = regressor @ directions[k],
//                                                                               a constant the caller computes once in float64)
// The directions, the regressor and joint_directions are constants: no gradient goes to them.  Gradients are those of
// torch's autograd for this composition:
//     d template[v] = g_vertices[v] + sum over the non-zeros (j, v) of column v of w[j, v] * g_joints[j]
//     d c[k]        = sum over e of directions[k, e] * g_vertices[e] + [k < Ks] sum over j of joint_directions[k, j] . g_joints[j]
// and an operand shared by the scenes receives the sum over the scenes.
//
// The table is the caller's packed copy [K, stride]: stride = 3 V rounded up to a multiple of 4 floats, the padding zero, the
// base 16-byte aligned -- so a lane reads one aligned 16-byte quad of four elements per direction.  The template, the outputs
// and the gradients are plain [.., V, 3] rows that are only 4-byte aligned (Float4 of dirt_stage.h).
//
// The order of every sum (the same on every run; no atomics, global or LDS):
//   vertices      directions in blocks of BL_UNROLL = 8, ascending: p = 0; p = fmaf(c[k], d[k], p) for the block's k in order;
//                 acc = acc + p, acc starting as the template's element.  (Blocked, not one chain over K: at K of a few hundred
//                 the chain's rounding grows with K, the blocked sum's with K / 8 + 8.)
//   joints        lane l of a wave takes non-zeros l, l + 64, ... of the joint's row, a = fmaf(w, template, a) from 0; wave_sum;
//                 the same over k = l, l + 64, ... < Ks with h = fmaf(c[k], joint_directions, h); wave_sum; joints = a + h.
//   d template    a = g_vertices[v] (or 0), a = fmaf(w, g_joints[j], a) over column v's non-zeros by j; shared template: the
//                 scenes' a added in scene order.
//   d c           first launch: workgroup (slab of 1024 elements, range of BL_KR = 8 directions, tile of BL_S = 4 scenes); a lane
//                 forms (d.x g.x + d.y g.y) + (d.z g.z + d.w g.w) of its quad, slab 0 adds fmaf(joint_directions, g_joints, .)
//                 over elements tid, tid + 256, ... < 3 J; wave_sum; four-wave fold -> one row of 32 partials per workgroup.
//                 Second launch: per (range, output scene) lane (slot, k) adds rows slot, slot + 32, ... (row = slab, or
//                 scene * slabs + slab for shared coefficients), then the 32 slots in order.
//
// Kernels:
//   blend_forward_kernel<S, AHEAD>    blockIdx.x < slabs: a quad of four elements per lane for S scenes (blockIdx.y = scene
//                                     tile), each direction row read once for the tile, AHEAD rows loaded before the first is
//                                     used -- <4, 16> for B > 1, <1, 32> for a single scene; the blocks of the sum are the same
//                                     in both, so a scene has the same bits alone and in a batch; blockIdx.x >= slabs: four
//                                     joints per workgroup, one (scene, joint) per wave in turn.
//   blend_template_backward_kernel    one vertex per lane; blockIdx.y = scene, or a loop over the scenes for a shared template.
//   blend_coefficient_sum_kernel      as above; blend_coefficient_reduce_kernel   as above.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_stage.h"

namespace dirt {

constexpr int BL_BLOCK = 256;     // lanes of a workgroup
constexpr int BL_QUAD = 4;        // consecutive elements of a lane: one 16-byte read of a direction row
constexpr int BL_SLAB = BL_BLOCK * BL_QUAD;   // elements of a workgroup
constexpr int BL_S = 4;           // scenes of a tile: they share every direction row from registers (a single scene: a tile of one)
constexpr int BL_UNROLL = 8;      // directions of a block of the forward's sum
constexpr int BL_AHEAD = 16;      // rows loaded before the first is used = 16-byte loads in flight per lane, tiles of BL_S scenes
constexpr int BL_AHEAD_ONE = 32;  // the same for a single scene (B = 1), whose quad leaves the registers for it
constexpr int BL_KR = 8;          // directions of a workgroup of the coefficient gradient's first launch
constexpr int BL_ROW = BL_S * BL_KR;   // floats of a workgroup's row of partial sums
constexpr int BL_SLOTS = 32;      // the reduce kernel: 32 slots x 8 directions = its 256 lanes

struct BlendParams {
    const float* t;               // [1 or B, V, 3] template
    const float* c;               // [1 or B, K] coefficients
    const float* d;               // [K, stride] packed directions, 16-byte aligned, stride % 4 == 0
    const int32_t* offsets;       // forward: CSR [J + 1]; backward: CSC [V + 1]
    const int32_t* indices;       // forward: the vertex of every non-zero; backward: its joint
    const float* weights;         // the non-zeros in that order
    const float* jd;              // [Ks, J, 3] joint_directions
    const float* gv;              // [B, V, 3] d loss / d vertices, or nullptr
    const float* gj;              // [B, J, 3] d loss / d joints, or nullptr
    float* vertices;              // [B, V, 3]
    float* joints;                // [B, J, 3]
    float* gt;                    // [1 or B, V, 3]
    float* partial;               // [tiles, ranges, slabs, BL_ROW]
    long long t_stride, c_stride; // floats between two scenes; 0 for an operand shared by the scenes
    long long stride;             // floats of a packed row
    int V, E, K, Ks, J, B, slabs;
};

// BL_UNROLL-aligned rows k0 .. k0 + AHEAD of the table into the accumulators of S scenes: ALL the loads first, unconditionally
// (AHEAD 16-byte loads in flight per lane; FULL: every row exists; otherwise rows past K - 1 re-read row K - 1 and only the
// arithmetic is guarded), then the blocks of BL_UNROLL in order.
template <int S, int AHEAD, bool FULL>
__device__ __forceinline__ void blend_rows(const float4* __restrict__ drow, size_t stride4, const float* (&cs)[S], int k0, int K,
                                           float (&acc)[S][BL_QUAD])
{
    float4 d[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) d[u] = drow[(size_t)(FULL ? k0 + u : min(k0 + u, K - 1)) * stride4];
    __builtin_amdgcn_sched_barrier(0);   // the scheduler may not sink a load below the arithmetic (it did: seven in flight, to save registers)
#pragma unroll
    for (int u0 = 0; u0 < AHEAD; u0 += BL_UNROLL) {
        if (!FULL && k0 + u0 >= K) break;   // (uniform)
        float part[S][BL_QUAD];
#pragma unroll
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int i = 0; i < BL_QUAD; ++i) part[s][i] = 0.f;
        }
#pragma unroll
        for (int u = u0; u < u0 + BL_UNROLL; ++u) {
            if (FULL || k0 + u < K) {   // (uniform)
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const float ck = cs[s][k0 + u];   // (uniform address, read-only memory: scalar loads)
                    part[s][0] = fmaf(ck, d[u].x, part[s][0]);
                    part[s][1] = fmaf(ck, d[u].y, part[s][1]);
                    part[s][2] = fmaf(ck, d[u].z, part[s][2]);
                    part[s][3] = fmaf(ck, d[u].w, part[s][3]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int i = 0; i < BL_QUAD; ++i) acc[s][i] += part[s][i];
        }
    }
}

// ---- forward.  S: scenes of a tile; AHEAD: rows of the table loaded before the first is used.  `c` and `table` are P.c and
// P.d again, as restrict-qualified arguments of their own: what lets the compiler prove them unwritten and read c with
// scalar loads.
template <int S, int AHEAD>
__global__ __launch_bounds__(BL_BLOCK) void blend_forward_kernel(const float* __restrict__ c, const float* __restrict__ table, BlendParams P)
{
    const int tid = threadIdx.x, b0 = blockIdx.y * S;
    if ((int)blockIdx.x < P.slabs) {
        const int q = blockIdx.x * BL_BLOCK + tid, e = q * BL_QUAD;
        if (e >= P.E) return;
        // a scene past the last one of the tile repeats the last one and is not stored
        const float* cs[S];
        float acc[S][BL_QUAD];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int b = min(b0 + s, P.B - 1);
            cs[s] = c + (size_t)b * P.c_stride;
            load_quad(P.t + (size_t)b * P.t_stride, e, P.E, acc[s]);
        }
        const float4* __restrict__ drow = reinterpret_cast<const float4*>(table) + q;
        const size_t stride4 = (size_t)(P.stride / BL_QUAD);
        int k0 = 0;
        for (; k0 + AHEAD <= P.K; k0 += AHEAD) blend_rows<S, AHEAD, true>(drow, stride4, cs, k0, P.K, acc);   // (uniform)
        if (k0 < P.K) blend_rows<S, AHEAD, false>(drow, stride4, cs, k0, P.K, acc);
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (b0 + s < P.B) store_quad(P.vertices + (size_t)(b0 + s) * P.E, e, P.E, acc[s]);
        return;
    }
    // the joints: wave w of workgroup x takes joint 4 (x - slabs) + w, the scenes of the tile in turn
    const int wave = tid >> 6, lane = tid & 63;
    const int j = ((int)blockIdx.x - P.slabs) * (BL_BLOCK / 64) + wave;
    if (j >= P.J) return;   // (the whole wave)
    const int r0 = P.offsets[j], r1 = P.offsets[j + 1];
    for (int s = 0; s < S && b0 + s < P.B; ++s) {   // (uniform)
        const int b = b0 + s;
        const float* __restrict__ tb = P.t + (size_t)b * P.t_stride;
        const float* __restrict__ cb = c + (size_t)b * P.c_stride;
        float a[3] = {0.f, 0.f, 0.f}, h[3] = {0.f, 0.f, 0.f}, x[3];
        for (int i = r0 + lane; i < r1; i += 64) {
            const float w = P.weights[i];
            load3(tb + (size_t)P.indices[i] * 3, x);
#pragma unroll
            for (int n = 0; n < 3; ++n) a[n] = fmaf(w, x[n], a[n]);
        }
        for (int k = lane; k < P.Ks; k += 64) {
            const float ck = cb[k];
            load3(P.jd + ((size_t)k * P.J + j) * 3, x);
#pragma unroll
            for (int n = 0; n < 3; ++n) h[n] = fmaf(ck, x[n], h[n]);
        }
        float out[3];
#pragma unroll
        for (int n = 0; n < 3; ++n) out[n] = wave_sum(a[n]) + wave_sum(h[n]);
        if (lane == 0) store3(P.joints + ((size_t)b * P.J + j) * 3, out);
    }
}

// ---- backward to the template: one vertex per lane; scene blockIdx.y, or for a template shared by the scenes every scene
// in turn (the sum in scene order)
__global__ __launch_bounds__(BL_BLOCK) void blend_template_backward_kernel(BlendParams P)
{
    const int v = blockIdx.x * BL_BLOCK + threadIdx.x;
    if (v >= P.V) return;
    const bool shared = P.t_stride == 0;
    const int first = shared ? 0 : (int)blockIdx.y, last = shared ? P.B : first + 1;
    int c0 = 0, c1 = 0;
    if (P.gj) { c0 = P.offsets[v]; c1 = P.offsets[v + 1]; }
    float total[3] = {0.f, 0.f, 0.f};
    for (int b = first; b < last; ++b) {   // (uniform)
        float a[3] = {0.f, 0.f, 0.f}, x[3];
        if (P.gv) load3(P.gv + ((size_t)b * P.V + v) * 3, a);
        for (int i = c0; i < c1; ++i) {
            const float w = P.weights[i];
            load3(P.gj + ((size_t)b * P.J + P.indices[i]) * 3, x);
#pragma unroll
            for (int n = 0; n < 3; ++n) a[n] = fmaf(w, x[n], a[n]);
        }
#pragma unroll
        for (int n = 0; n < 3; ++n) total[n] = b == first ? a[n] : total[n] + a[n];
    }
    store3(P.gt + ((size_t)(shared ? 0 : first) * P.V + v) * 3, total);
}

// ---- backward to the coefficients, first launch: workgroup (slab x, range y, tile z) leaves the BL_S x BL_KR dot products
// of its slab in row (z, y, x) of P.partial; slab 0 carries the joint term
__global__ __launch_bounds__(BL_BLOCK) void blend_coefficient_sum_kernel(BlendParams P)
{
    __shared__ float s_part[4 * BL_ROW];
    const int tid = threadIdx.x, k0 = blockIdx.y * BL_KR, b0 = blockIdx.z * BL_S;
    float dot[BL_S][BL_KR];
#pragma unroll
    for (int s = 0; s < BL_S; ++s) {
#pragma unroll
        for (int u = 0; u < BL_KR; ++u) dot[s][u] = 0.f;
    }
    if (P.gv) {   // (uniform)
        const int q = blockIdx.x * BL_BLOCK + tid, e = q * BL_QUAD;
        const bool live = e < P.E;
        float g[BL_S][BL_QUAD];
#pragma unroll
        for (int s = 0; s < BL_S; ++s) {
            if (live && b0 + s < P.B) {
                load_quad(P.gv + (size_t)(b0 + s) * P.E, e, P.E, g[s]);
            } else {
#pragma unroll
                for (int i = 0; i < BL_QUAD; ++i) g[s][i] = 0.f;
            }
        }
        const float4* __restrict__ drow = reinterpret_cast<const float4*>(P.d) + (live ? q : 0);
        const size_t stride4 = (size_t)(P.stride / BL_QUAD);
        float4 d[BL_KR];   // all eight loads first, unconditionally: rows past K - 1 re-read row K - 1 and are not used
#pragma unroll
        for (int u = 0; u < BL_KR; ++u) d[u] = drow[(size_t)min(k0 + u, P.K - 1) * stride4];
        __builtin_amdgcn_sched_barrier(0);   // (the loads stay in front of the arithmetic)
#pragma unroll
        for (int u = 0; u < BL_KR; ++u) {
            if (k0 + u < P.K && live) {   // a lane past the row adds nothing (not 0 x a value that may not be finite)
#pragma unroll
                for (int s = 0; s < BL_S; ++s)
                    if (b0 + s < P.B) dot[s][u] = (d[u].x * g[s][0] + d[u].y * g[s][1]) + (d[u].z * g[s][2] + d[u].w * g[s][3]);
            }
        }
    }
    if (P.gj && blockIdx.x == 0) {   // (uniform)
        const int EJ = 3 * P.J;
        for (int e = tid; e < EJ; e += BL_BLOCK) {
            float g[BL_S];
#pragma unroll
            for (int s = 0; s < BL_S; ++s) g[s] = b0 + s < P.B ? P.gj[(size_t)(b0 + s) * EJ + e] : 0.f;
#pragma unroll
            for (int u = 0; u < BL_KR; ++u) {
                if (k0 + u < P.Ks) {
                    const float x = P.jd[(size_t)(k0 + u) * EJ + e];
#pragma unroll
                    for (int s = 0; s < BL_S; ++s)
                        if (b0 + s < P.B) dot[s][u] = fmaf(x, g[s], dot[s][u]);
                }
            }
        }
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int s = 0; s < BL_S; ++s) {
#pragma unroll
        for (int u = 0; u < BL_KR; ++u) {
            const float t = wave_sum(dot[s][u]);
            if (lane == 0) s_part[wave * BL_ROW + s * BL_KR + u] = t;
        }
    }
    __syncthreads();
    if (tid < BL_ROW) fold_waves_to_row<BL_ROW>(s_part, P.partial + (size_t)blockIdx.z * gridDim.y * gridDim.x * BL_ROW, tid);
}

// ---- backward to the coefficients, second launch: workgroup (range y = blockIdx.x, scene of the output blockIdx.y) adds
// the rows of its range in a fixed order -- for coefficients shared by the scenes (`shared`, gridDim.y = 1) those of all B
// scenes, scene by scene -- and writes d c[k] of its up to BL_KR directions.
__global__ __launch_bounds__(BL_BLOCK) void blend_coefficient_reduce_kernel(const float* __restrict__ partial, float* __restrict__ gc, int slabs,
                                                                            int B, int K, int shared)
{
    __shared__ float s_sum[BL_SLOTS * BL_KR];
    const int tid = threadIdx.x, y = blockIdx.x, ranges = gridDim.x;
    const int slot = tid / BL_KR, u = tid - BL_KR * slot;
    const long long rows = shared ? (long long)slabs * B : slabs;
    float s = 0.f;
    for (long long r = slot; r < rows; r += BL_SLOTS) {
        const long long scene = shared ? r / slabs : blockIdx.y, x = shared ? r % slabs : r;
        const long long z = scene / BL_S, sl = scene % BL_S;
        s += partial[(((size_t)z * ranges + y) * slabs + x) * BL_ROW + sl * BL_KR + u];
    }
    s_sum[tid] = s;
    __syncthreads();
    const int k = y * BL_KR + tid;
    if (tid < BL_KR && k < K) {
        float t = 0.f;
        for (int i = 0; i < BL_SLOTS; ++i) t += s_sum[i * BL_KR + tid];
        gc[(size_t)blockIdx.y * K + k] = t;
    }
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

static long long blend_slabs(long long V) { return (3 * V + dirt::BL_SLAB - 1) / dirt::BL_SLAB; }
static long long blend_tiles(long long B) { return (B + dirt::BL_S - 1) / dirt::BL_S; }
static long long blend_ranges(long long K) { return (K + dirt::BL_KR - 1) / dirt::BL_KR; }

static int blend_check(const char* who, int template_scenes, int coefficient_scenes, const float* directions, long long stride,
                       const float* joint_directions, long long B, long long V, int K, int Ks, int J, unsigned flags, dirt::BlendParams& P)
{
    if (B < 0 || V < 0 || K < 0 || Ks < 0 || J < 0) STAGE_FAIL("%s: negative sizes (B=%lld V=%lld K=%d Ks=%d J=%d)", who, B, V, K, Ks, J);
    if (B > 65535 || V > DIRT_BLEND_MAX_VERTICES || K > DIRT_BLEND_MAX_SHAPES || J > DIRT_BLEND_MAX_JOINTS)
        STAGE_FAIL("%s: B=%lld V=%lld K=%d J=%d, at most 65535 scenes, %d vertices, %d shapes, %d joints", who, B, V, K, J, DIRT_BLEND_MAX_VERTICES,
                   DIRT_BLEND_MAX_SHAPES, DIRT_BLEND_MAX_JOINTS);
    if (Ks > K) STAGE_FAIL("%s: Ks=%d of K=%d shapes move the joints", who, Ks, K);
    if (template_scenes != 1 && template_scenes != B) STAGE_FAIL("%s: template_scenes=%d is neither 1 nor B=%lld", who, template_scenes, B);
    if (coefficient_scenes != 1 && coefficient_scenes != B) STAGE_FAIL("%s: coefficient_scenes=%d is neither 1 nor B=%lld", who, coefficient_scenes, B);
    if (stride < 3 * V || stride % 4) STAGE_FAIL("%s: stride=%lld, a multiple of 4 floats that holds 3 V = %lld", who, stride, 3 * V);
    if (flags) STAGE_FAIL("%s: unknown flags 0x%x", who, flags);
    if (B == 0 || V == 0) return DIRT_OK;
    if (K && !directions) STAGE_FAIL("%s: directions is NULL", who);
    if (reinterpret_cast<uintptr_t>(directions) & 15u) STAGE_FAIL("%s: directions (the packed table) is not 16-byte aligned", who);
    if (Ks && J && !joint_directions) STAGE_FAIL("%s: joint_directions is NULL", who);
    P.d = directions; P.jd = joint_directions; P.stride = stride;
    P.V = (int)V; P.E = (int)(3 * V); P.K = K; P.Ks = Ks; P.J = J; P.B = (int)B;
    P.t_stride = template_scenes == 1 ? 0 : 3 * V;
    P.c_stride = coefficient_scenes == 1 ? 0 : K;
    P.slabs = (int)blend_slabs(V);
    return DIRT_OK;
}

size_t dirt_blend_scratch_bytes(long long B, long long V, long long K)
{
    if (B < 0 || B > 65535 || V < 0 || V > DIRT_BLEND_MAX_VERTICES || K < 0 || K > DIRT_BLEND_MAX_SHAPES) return 0;
    return sizeof(float) * dirt::BL_ROW * (size_t)blend_tiles(B) * (size_t)blend_ranges(K) * (size_t)blend_slabs(V);
}

int dirt_blend_forward(const float* template_vertices, int template_scenes, const float* coefficients, int coefficient_scenes,
                       const float* directions, long long stride, const int32_t* row_offsets, const int32_t* row_vertices,
                       const float* row_weights, const float* joint_directions, float* vertices, float* joints, long long B, long long V,
                       int K, int Ks, int J, unsigned flags, void* stream)
{
    const char* who = "dirt_blend_forward";
    dirt::BlendParams P{};
    int rc = blend_check(who, template_scenes, coefficient_scenes, directions, stride, joint_directions, B, V, K, Ks, J, flags, P);
    if (rc) return rc;
    if (J == 0) joints = nullptr;
    if (B == 0 || V == 0 || (!vertices && !joints)) return dirt::stage_ok(report);
    if (!template_vertices) STAGE_FAIL("%s: template_vertices is NULL", who);
    if (K && !coefficients) STAGE_FAIL("%s: coefficients is NULL", who);
    if (joints && !row_offsets) STAGE_FAIL("%s: joints need row_offsets (and row_vertices / row_weights of its non-zeros)", who);
    P.t = template_vertices; P.c = coefficients; P.offsets = row_offsets; P.indices = row_vertices; P.weights = row_weights;
    P.vertices = vertices; P.joints = joints;
    if (!vertices) P.slabs = 0;
    const unsigned joint_blocks = joints ? (unsigned)((J + 3) / 4) : 0u;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (B == 1) {   // one scene: nothing to share a row with, so twice the rows in flight
        const dim3 grid((unsigned)P.slabs + joint_blocks, 1u);
        hipLaunchKernelGGL((dirt::blend_forward_kernel<1, dirt::BL_AHEAD_ONE>), grid, dim3(dirt::BL_BLOCK), 0, s, P.c, P.d, P);
    } else {
        const dim3 grid((unsigned)P.slabs + joint_blocks, (unsigned)blend_tiles(B));
        hipLaunchKernelGGL((dirt::blend_forward_kernel<dirt::BL_S, dirt::BL_AHEAD>), grid, dim3(dirt::BL_BLOCK), 0, s, P.c, P.d, P);
    }
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_blend_backward(int template_scenes, int coefficient_scenes, const float* directions, long long stride, const int32_t* column_offsets,
                        const int32_t* column_joints, const float* column_weights, const float* joint_directions, const float* grad_vertices,
                        const float* grad_joints, float* grad_template, float* grad_coefficients, void* scratch, size_t scratch_bytes,
                        long long B, long long V, int K, int Ks, int J, unsigned flags, void* stream)
{
    const char* who = "dirt_blend_backward";
    dirt::BlendParams P{};
    int rc = blend_check(who, template_scenes, coefficient_scenes, directions, stride, joint_directions, B, V, K, Ks, J, flags, P);
    if (rc) return rc;
    if (J == 0) grad_joints = nullptr;
    if (K == 0) grad_coefficients = nullptr;
    if (B == 0 || V == 0 || (!grad_template && !grad_coefficients)) return dirt::stage_ok(report);
    if (grad_joints && grad_template && !column_offsets) STAGE_FAIL("%s: grad_template needs column_offsets (and column_joints / column_weights)", who);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    P.gv = grad_vertices; P.gj = grad_joints;
    hipError_t e = hipSuccess;
    if (grad_coefficients) {
        rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_blend_scratch_bytes(B, V, K), "dirt_blend_scratch_bytes");
        if (rc) return rc;
        P.partial = static_cast<float*>(scratch);
        // without a gradient from the vertices only slab 0 -- the joint term -- has anything to add
        const int slabs = grad_vertices ? P.slabs : 1;
        const dim3 grid((unsigned)slabs, (unsigned)blend_ranges(K), (unsigned)blend_tiles(B));
        hipLaunchKernelGGL(dirt::blend_coefficient_sum_kernel, grid, dim3(dirt::BL_BLOCK), 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return dirt::stage_hip(report, who, e);
        const int shared = coefficient_scenes == 1 ? 1 : 0;
        hipLaunchKernelGGL(dirt::blend_coefficient_reduce_kernel, dim3((unsigned)blend_ranges(K), shared ? 1u : (unsigned)B), dim3(dirt::BL_BLOCK), 0, s,
                           P.partial, grad_coefficients, slabs, (int)B, K, shared);
        if ((e = hipGetLastError()) != hipSuccess) return dirt::stage_hip(report, who, e);
    }
    if (grad_template) {
        P.gt = grad_template; P.offsets = column_offsets; P.indices = column_joints; P.weights = column_weights;
        const dim3 grid((unsigned)((V + dirt::BL_BLOCK - 1) / dirt::BL_BLOCK), P.t_stride == 0 ? 1u : (unsigned)B);
        hipLaunchKernelGGL(dirt::blend_template_backward_kernel, grid, dim3(dirt::BL_BLOCK), 0, s, P);
        e = hipGetLastError();
    }
    return dirt::stage_hip(report, who, e);
}

}  // extern "C"
