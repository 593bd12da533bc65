// dirt_skin.hip -- linear-blend skinning in front of the vertex stage, fused: rest-pose vertices and bone transforms ->
// posed vertices in one launch, and the gradients to the vertices, the bone transforms and the skinning weights without
// float atomics.
//
// Extends what the reference's samples do with ONE matrix for the whole mesh (samples/deferred.py:40-41) to a per-vertex
// blend of bone matrices.  The specification (DESIGN.md §7d restates it; tests/skin_reference.py composes it in float64),
// per scene, row-vector convention, K influences per vertex:
//
//     v4 = (x, y, z, w or 1)
//     M[v] = sum over k in slot order of w[v, k] * T[idx[v, k]]            (a zero weight is padding; nothing is renormalised)
//     posed[v] = (v4 @ M[v])[:3]
//
// Column 3 of the transforms is never read: its gradient is zero and is written as zero.  Gradients are those of torch's
// autograd for this composition:
//     d v4      = g @ M[:, :3]^T                                  (all three or four components)
//     d T[j]    = sum over the entries (v, k) with idx[v, k] = j of w[v, k] * outer(v4, g)
//     d w[v, k] = (v4 @ T[idx[v, k]])[:3] . g
// and an operand shared by the scenes receives the sum over the scenes.
//
// The scatter of d T (float atomics on a few dozen addresses in a torch composition) is a gather here, over an inverted
// index the caller builds once per mesh: `entries` [V K], the positions v * K + k ordered by bone, then position; a chunk
// table [chunks, 3] of (bone, begin, end) that cuts every bone's run of `entries` into pieces of a fixed number of entries,
// none spanning two bones (a root bone that every vertex names is spread over many workgroups); `chunk_offsets` [J + 1], the
// chunks of bone j being chunk_offsets[j] .. chunk_offsets[j + 1].
//
// Kernels (KT: K at compile time, 4, or 0 for any K in 1..8; STAGED: the scene's 4x3 bone blocks staged in LDS):
//   skin_forward_kernel<KT, STAGED>           one (scene, vertex) per lane, blockIdx.y = scene.
//   skin_vertex_backward_kernel<KT, STAGED>   the same shape: d vertices of per-scene vertices.
//   skin_shared_backward_kernel<KT, STAGED>   one vertex per lane, looping over the scenes: d weights, and d vertices of a
//                                             rest mesh shared by the scenes (the sums over the scenes in scene order).
//   skin_bone_sum_kernel<KT>                  one workgroup per (chunk, scene): each lane sums the 12 values of its entries in
//                                             registers, wave sum, the four waves folded into one row of caller-owned scratch.
//   skin_bone_reduce_kernel                   one workgroup per (bone, scene of the output): the bone's rows -- of every scene
//                                             for shared transforms -- added in a fixed order; writes all 16 values.
// LDS budget of the staging: DIRT_SKIN_LDS_BONES = 256 bones x 12 floats = 12 KB per workgroup of 256 lanes -- thirteen
// such workgroups fit the 160 KB of a compute unit, more than the eight its 2048 lanes allow, so the staging never lowers
// the occupancy.  With more bones the blocks are read through L1 / L2 as four 12-byte loads each.
// No atomics anywhere (global or LDS), and the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_stage.h"

namespace dirt {

constexpr int SK_BLOCK = 256;        // lanes of a workgroup
constexpr int SK_ROW = 12;           // floats of a bone's 4x3 block = of a workgroup's row of partial sums
constexpr int SK_SLOTS = 21;         // the reduce kernel: 21 x 12 = 252 of its 256 lanes each sum every 21st row of one column
constexpr int SK_KMAX = DIRT_SKIN_MAX_INFLUENCES;

struct SkinParams {
    const float* v;               // [1 or B, V, C]
    const int32_t* idx;           // [V, K]
    const float* w;               // [V, K]
    const float* T;               // [1 or B, J, 16]
    const int32_t* entries;       // [V K]
    const int32_t* chunk_table;   // [chunks, 3]
    const float* g;               // [B, V, 3] d loss / d posed
    float* posed;                 // [B, V, 3]
    float* gv;                    // [1 or B, V, C] or nullptr
    float* gw;                    // [V, K] or nullptr
    float* partial;               // [B, chunks, 12]
    long long v_stride, T_stride; // floats between two scenes; 0 for an operand shared by the scenes
    int V, C, K, J, B;
};

// a vertex as the composition sees it: (x, y, z, w or 1)
__device__ __forceinline__ void skin_vertex(const float* __restrict__ vb, int C, int u, float (&x)[4])
{
    const float* __restrict__ p = vb + (size_t)u * C;
    const Float3 t = *reinterpret_cast<const Float3*>(p);
    x[0] = t.x; x[1] = t.y; x[2] = t.z;
    x[3] = C == 4 ? p[3] : 1.f;
}

// the scene's bone blocks into LDS: rows 0-3, columns 0-2 of every transform (every lane of the workgroup; the caller synchronises)
__device__ __forceinline__ void stage_bones(const float* __restrict__ Tb, float* s_T, int J, int tid)
{
    for (int i = tid; i < J * SK_ROW; i += SK_BLOCK) {
        const int j = i / SK_ROW, r = i - SK_ROW * j;
        s_T[i] = Tb[j * 16 + (r / 3) * 4 + r % 3];
    }
}

// the 4x3 block of bone j: t[3 r + c] = T[j][r][c]
template <bool STAGED>
__device__ __forceinline__ void bone_block(const float* __restrict__ Tb, const float* s_T, int j, float (&t)[SK_ROW])
{
    if constexpr (STAGED) {
        const float4* p = reinterpret_cast<const float4*>(s_T + j * SK_ROW);   // 48-byte blocks of a 16-byte aligned array
        const float4 a = p[0], b = p[1], c = p[2];
        t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
        t[8] = c.x; t[9] = c.y; t[10] = c.z; t[11] = c.w;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float row[3];
            load3(Tb + (size_t)j * 16 + 4 * r, row);
            t[3 * r] = row[0]; t[3 * r + 1] = row[1]; t[3 * r + 2] = row[2];
        }
    }
}

struct Int4 { int32_t x, y, z, w; };   // four consecutive indices, 4-byte aligned: one 16-byte access

// slot k of vertex i: its bone and weight.  KT = 4: the four of a vertex in one 16-byte load each
template <int KT>
__device__ __forceinline__ void load_slots(const SkinParams& P, int i, int (&idx)[KT ? KT : SK_KMAX], float (&w)[KT ? KT : SK_KMAX])
{
    if constexpr (KT == 4) {
        const Float4 ww = *reinterpret_cast<const Float4*>(P.w + (size_t)i * 4);
        const Int4 ii = *reinterpret_cast<const Int4*>(P.idx + (size_t)i * 4);
        w[0] = ww.x; w[1] = ww.y; w[2] = ww.z; w[3] = ww.w;
        idx[0] = ii.x; idx[1] = ii.y; idx[2] = ii.z; idx[3] = ii.w;
    } else {
#pragma unroll
        for (int k = 0; k < SK_KMAX; ++k) {   // (unrolled and predicated: the slots stay in registers)
            const bool on = k < P.K;
            idx[k] = on ? P.idx[(size_t)i * P.K + k] : 0;
            w[k] = on ? P.w[(size_t)i * P.K + k] : 0.f;
        }
    }
}

// M = sum over the slots, in slot order, of w * T[idx]
template <int KT, bool STAGED>
__device__ __forceinline__ void blend(const SkinParams& P, const float* __restrict__ Tb, const float* s_T, int i, float (&M)[SK_ROW])
{
    constexpr int KN = KT ? KT : SK_KMAX;
    int idx[KN];
    float w[KN];
    load_slots<KT>(P, i, idx, w);
#pragma unroll
    for (int q = 0; q < SK_ROW; ++q) M[q] = 0.f;
#pragma unroll
    for (int k = 0; k < KN; ++k) {
        if (KT || k < P.K) {
            float t[SK_ROW];
            bone_block<STAGED>(Tb, s_T, idx[k], t);
#pragma unroll
            for (int q = 0; q < SK_ROW; ++q) M[q] += w[k] * t[q];
        }
    }
}

// row vector times a 4x3 block
__device__ __forceinline__ void transform43(const float (&x)[4], const float (&m)[SK_ROW], float (&y)[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) y[c] = ((x[0] * m[c] + x[1] * m[3 + c]) + x[2] * m[6 + c]) + x[3] * m[9 + c];
}

// ---- forward: one (scene, vertex) per lane
template <int KT, bool STAGED>
__global__ __launch_bounds__(SK_BLOCK) void skin_forward_kernel(SkinParams P)
{
    __shared__ __attribute__((aligned(16))) float s_T[STAGED ? DIRT_SKIN_LDS_BONES * SK_ROW : 4];
    const int tid = threadIdx.x, i = blockIdx.x * SK_BLOCK + tid, b = blockIdx.y;
    const float* __restrict__ Tb = P.T + (size_t)b * P.T_stride;
    if constexpr (STAGED) {
        stage_bones(Tb, s_T, P.J, tid);
        __syncthreads();
    }
    if (i >= P.V) return;
    float M[SK_ROW], x[4], y[3];
    blend<KT, STAGED>(P, Tb, s_T, i, M);
    skin_vertex(P.v + (size_t)b * P.v_stride, P.C, i, x);
    transform43(x, M, y);
    store3(P.posed + ((size_t)b * P.V + i) * 3, y);
}

// d v4[r] = g . M[r][:]
__device__ __forceinline__ void vertex_grad(const float (&g)[3], const float (&M)[SK_ROW], float (&d)[4])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = (g[0] * M[3 * r] + g[1] * M[3 * r + 1]) + g[2] * M[3 * r + 2];
}

// ---- backward to per-scene vertices: the forward's shape
template <int KT, bool STAGED>
__global__ __launch_bounds__(SK_BLOCK) void skin_vertex_backward_kernel(SkinParams P)
{
    __shared__ __attribute__((aligned(16))) float s_T[STAGED ? DIRT_SKIN_LDS_BONES * SK_ROW : 4];
    const int tid = threadIdx.x, i = blockIdx.x * SK_BLOCK + tid, b = blockIdx.y;
    const float* __restrict__ Tb = P.T + (size_t)b * P.T_stride;
    if constexpr (STAGED) {
        stage_bones(Tb, s_T, P.J, tid);
        __syncthreads();
    }
    if (i >= P.V) return;
    float M[SK_ROW], g[3], d[4];
    blend<KT, STAGED>(P, Tb, s_T, i, M);
    load3(P.g + ((size_t)b * P.V + i) * 3, g);
    vertex_grad(g, M, d);
    float* __restrict__ o = P.gv + ((size_t)b * P.V + i) * P.C;
    *reinterpret_cast<Float3*>(o) = Float3{d[0], d[1], d[2]};
    if (P.C == 4) o[3] = d[3];
}

// ---- backward to the operands the scenes share: one vertex per lane, the scenes in turn (sums in scene order).
// d weights (P.gw) and, for a rest mesh shared by the scenes (or a single scene), d vertices (P.gv)
template <int KT, bool STAGED>
__global__ __launch_bounds__(SK_BLOCK) void skin_shared_backward_kernel(SkinParams P)
{
    constexpr int KN = KT ? KT : SK_KMAX;
    __shared__ __attribute__((aligned(16))) float s_T[STAGED ? DIRT_SKIN_LDS_BONES * SK_ROW : 4];
    const int tid = threadIdx.x, i = blockIdx.x * SK_BLOCK + tid;
    const bool live = i < P.V;
    int idx[KN];
    float w[KN], gw[KN], gv[4] = {0.f, 0.f, 0.f, 0.f};
    load_slots<KT>(P, live ? i : 0, idx, w);
#pragma unroll
    for (int k = 0; k < KN; ++k) gw[k] = 0.f;
    for (int b = 0; b < P.B; ++b) {   // (uniform)
        const float* __restrict__ Tb = P.T + (size_t)b * P.T_stride;
        if constexpr (STAGED) {
            if (b == 0 || P.T_stride != 0) {   // (uniform) shared transforms are staged once
                if (b != 0) __syncthreads();   // every lane has read the scene before
                stage_bones(Tb, s_T, P.J, tid);
                __syncthreads();
            }
        }
        if (!live) continue;
        float x[4], g[3], M[SK_ROW];
        skin_vertex(P.v + (size_t)b * P.v_stride, P.C, i, x);
        load3(P.g + ((size_t)b * P.V + i) * 3, g);
#pragma unroll
        for (int q = 0; q < SK_ROW; ++q) M[q] = 0.f;
#pragma unroll
        for (int k = 0; k < KN; ++k) {
            if (KT || k < P.K) {
                float t[SK_ROW], y[3];
                bone_block<STAGED>(Tb, s_T, idx[k], t);
                transform43(x, t, y);
                gw[k] += dot3(y, g);
#pragma unroll
                for (int q = 0; q < SK_ROW; ++q) M[q] += w[k] * t[q];
            }
        }
        float d[4];
        vertex_grad(g, M, d);
#pragma unroll
        for (int r = 0; r < 4; ++r) gv[r] += d[r];
    }
    if (!live) return;
    if (P.gv) {
        float* __restrict__ o = P.gv + (size_t)i * P.C;
        *reinterpret_cast<Float3*>(o) = Float3{gv[0], gv[1], gv[2]};
        if (P.C == 4) o[3] = gv[3];
    }
    if (P.gw) {
        if constexpr (KT == 4) {
            *reinterpret_cast<Float4*>(P.gw + (size_t)i * 4) = Float4{gw[0], gw[1], gw[2], gw[3]};
        } else {
#pragma unroll
            for (int k = 0; k < SK_KMAX; ++k)
                if (k < P.K) P.gw[(size_t)i * P.K + k] = gw[k];
        }
    }
}

// ---- backward to the bones, first launch: workgroup (chunk, scene) sums w * outer(v4, g) over the entries of its chunk
// into row (scene, chunk) of P.partial.  Lane t takes entries begin + t, begin + t + 256, ...
template <int KT>
__global__ __launch_bounds__(SK_BLOCK) void skin_bone_sum_kernel(SkinParams P)
{
    __shared__ float s_part[4 * SK_ROW];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int32_t* __restrict__ ct = P.chunk_table + (size_t)blockIdx.x * 3;
    const int beg = ct[1], end = ct[2];
    const float* __restrict__ vb = P.v + (size_t)b * P.v_stride;
    const float* __restrict__ gb = P.g + (size_t)b * P.V * 3;
    float acc[SK_ROW];
#pragma unroll
    for (int q = 0; q < SK_ROW; ++q) acc[q] = 0.f;
    for (int e = beg + tid; e < end; e += SK_BLOCK) {
        const int entry = P.entries[e];
        const int u = KT ? entry / (KT ? KT : 1) : entry / P.K;
        const float w = P.w[entry];
        float x[4], g[3];
        skin_vertex(vb, P.C, u, x);
        load3(gb + (size_t)u * 3, g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[3 * r + c] += w * (x[r] * g[c]);
        }
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int q = 0; q < SK_ROW; ++q) {
        const float s = wave_sum(acc[q]);
        if (lane == 0) s_part[wave * SK_ROW + q] = s;
    }
    __syncthreads();
    if (tid < SK_ROW) fold_waves_to_row<SK_ROW>(s_part, P.partial, tid);
}

// ---- backward to the bones, second launch: workgroup (bone j, scene b of the output) adds the rows of the bone's chunks
// in a fixed order -- for transforms shared by the scenes (`shared`, gridDim.y = 1) those of all B scenes, scene by scene
// -- and writes the 16 values of d T[b][j], column 3 as zero.  (Twelve totals per workgroup from rows of twelve: lane
// 12 s + q sums rows s, s + 21, ... of column q, so a wave reads whole rows; block_column_sum gives one total per workgroup.)
__global__ __launch_bounds__(SK_BLOCK) void skin_bone_reduce_kernel(const float* __restrict__ partial, const int32_t* __restrict__ chunk_offsets,
                                                                    float* __restrict__ gT, long long chunks, int B, int shared)
{
    __shared__ float s_sum[SK_SLOTS * SK_ROW];
    const int tid = threadIdx.x, j = blockIdx.x, b = blockIdx.y;
    const int c0 = chunk_offsets[j], nc = chunk_offsets[j + 1] - c0;
    const long long rows = shared ? (long long)nc * B : nc;
    if (tid < SK_SLOTS * SK_ROW) {
        const int slot = tid / SK_ROW, q = tid - SK_ROW * slot;
        float s = 0.f;
        for (long long r = slot; r < rows; r += SK_SLOTS) {
            const long long scene = shared ? r / nc : b, c = c0 + (shared ? r % nc : r);
            s += partial[(scene * chunks + c) * SK_ROW + q];
        }
        s_sum[tid] = s;
    }
    __syncthreads();
    if (tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        float t = 0.f;
        if (c < 3) {
            for (int slot = 0; slot < SK_SLOTS; ++slot) t += s_sum[slot * SK_ROW + 3 * r + c];
        }
        gT[((size_t)b * gridDim.x + j) * 16 + tid] = t;
    }
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

static long long skin_blocks(long long V) { return (V + dirt::SK_BLOCK - 1) / dirt::SK_BLOCK; }

static int skin_check(const char* who, const float* vertices, int components, int vertex_scenes, const int32_t* bone_indices,
                      const float* bone_weights, const float* transforms, int transform_scenes, long long B, long long V, int K, int J,
                      unsigned flags, dirt::SkinParams& P)
{
    if (B < 0 || V < 0 || J < 0) STAGE_FAIL("%s: negative sizes (B=%lld V=%lld J=%d)", who, B, V, J);
    if (B > 65535 || V > DIRT_SKIN_MAX_VERTICES || J > DIRT_SKIN_MAX_BONES)
        STAGE_FAIL("%s: B=%lld V=%lld J=%d, at most 65535 scenes, %d vertices, %d bones", who, B, V, J, DIRT_SKIN_MAX_VERTICES, DIRT_SKIN_MAX_BONES);
    if (K < 1 || K > DIRT_SKIN_MAX_INFLUENCES) STAGE_FAIL("%s: K=%d influences, 1 to %d", who, K, DIRT_SKIN_MAX_INFLUENCES);
    if (V * K > DIRT_SKIN_MAX_ENTRIES) STAGE_FAIL("%s: V=%lld K=%d, at most %d entries (V K)", who, V, K, DIRT_SKIN_MAX_ENTRIES);
    if (components != 3 && components != 4) STAGE_FAIL("%s: vertices have %d components, 3 or 4", who, components);
    if (vertex_scenes != 1 && vertex_scenes != B) STAGE_FAIL("%s: vertex_scenes=%d is neither 1 nor B=%lld", who, vertex_scenes, B);
    if (transform_scenes != 1 && transform_scenes != B) STAGE_FAIL("%s: transform_scenes=%d is neither 1 nor B=%lld", who, transform_scenes, B);
    if (flags) STAGE_FAIL("%s: unknown flags 0x%x", who, flags);
    if (B == 0 || V == 0) return DIRT_OK;
    if (J == 0) STAGE_FAIL("%s: %lld vertices and no bone", who, V);
    if (!vertices || !bone_indices || !bone_weights || !transforms) STAGE_FAIL("%s: vertices / bone_indices / bone_weights / transforms is NULL", who);
    P.v = vertices; P.idx = bone_indices; P.w = bone_weights; P.T = transforms;
    P.V = (int)V; P.C = components; P.K = K; P.J = J; P.B = (int)B;
    P.v_stride = vertex_scenes == 1 ? 0 : V * components;
    P.T_stride = transform_scenes == 1 ? 0 : (long long)J * 16;
    return DIRT_OK;
}

// kernel<KT, STAGED> for these K and J
#define SKIN_LAUNCH(kernel, grid, s, P)                                                                                     \
    do {                                                                                                                    \
        const bool staged_ = (P).J <= DIRT_SKIN_LDS_BONES;                                                                  \
        if ((P).K == 4) {                                                                                                   \
            if (staged_) hipLaunchKernelGGL((dirt::kernel<4, true>), grid, dim3(dirt::SK_BLOCK), 0, s, P);                  \
            else hipLaunchKernelGGL((dirt::kernel<4, false>), grid, dim3(dirt::SK_BLOCK), 0, s, P);                         \
        } else {                                                                                                            \
            if (staged_) hipLaunchKernelGGL((dirt::kernel<0, true>), grid, dim3(dirt::SK_BLOCK), 0, s, P);                  \
            else hipLaunchKernelGGL((dirt::kernel<0, false>), grid, dim3(dirt::SK_BLOCK), 0, s, P);                         \
        }                                                                                                                   \
    } while (0)

size_t dirt_skin_scratch_bytes(long long B, long long chunks)
{
    if (B < 0 || B > 65535 || chunks < 0 || chunks > DIRT_SKIN_MAX_CHUNKS) return 0;
    return sizeof(float) * dirt::SK_ROW * (size_t)B * (size_t)chunks;
}

int dirt_skin_forward(const float* vertices, int components, int vertex_scenes, const int32_t* bone_indices, const float* bone_weights,
                      const float* transforms, int transform_scenes, float* posed, long long B, long long V, int K, int J, unsigned flags,
                      void* stream)
{
    const char* who = "dirt_skin_forward";
    dirt::SkinParams P{};
    int rc = skin_check(who, vertices, components, vertex_scenes, bone_indices, bone_weights, transforms, transform_scenes, B, V, K, J, flags, P);
    if (rc) return rc;
    if (B == 0 || V == 0 || !posed) return dirt::stage_ok(report);
    P.posed = posed;
    const dim3 grid((unsigned)skin_blocks(V), (unsigned)B);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SKIN_LAUNCH(skin_forward_kernel, grid, s, P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_skin_backward(const float* vertices, int components, int vertex_scenes, const int32_t* bone_indices, const float* bone_weights,
                       const float* transforms, int transform_scenes, const int32_t* entries, const int32_t* chunk_table,
                       const int32_t* chunk_offsets, const float* grad_posed, float* grad_vertices, float* grad_transforms, float* grad_weights,
                       void* scratch, size_t scratch_bytes, long long B, long long V, int K, int J, long long chunks, unsigned flags, void* stream)
{
    const char* who = "dirt_skin_backward";
    dirt::SkinParams P{};
    int rc = skin_check(who, vertices, components, vertex_scenes, bone_indices, bone_weights, transforms, transform_scenes, B, V, K, J, flags, P);
    if (rc) return rc;
    if (chunks < 0 || chunks > DIRT_SKIN_MAX_CHUNKS) STAGE_FAIL("%s: chunks=%lld, 0 to %d", who, chunks, DIRT_SKIN_MAX_CHUNKS);
    if (B == 0 || V == 0 || (!grad_vertices && !grad_transforms && !grad_weights)) return dirt::stage_ok(report);
    if (!grad_posed) STAGE_FAIL("%s: grad_posed is NULL", who);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    P.g = grad_posed;
    hipError_t e = hipSuccess;
    if (grad_transforms) {
        if (chunks == 0 || !entries || !chunk_table || !chunk_offsets) STAGE_FAIL("%s: grad_transforms needs entries / chunk_table / chunk_offsets", who);
        rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_skin_scratch_bytes(B, chunks), "dirt_skin_scratch_bytes");
        if (rc) return rc;
        P.entries = entries; P.chunk_table = chunk_table; P.partial = static_cast<float*>(scratch);
        const dim3 grid((unsigned)chunks, (unsigned)B);
        if (K == 4) hipLaunchKernelGGL(dirt::skin_bone_sum_kernel<4>, grid, dim3(dirt::SK_BLOCK), 0, s, P);
        else hipLaunchKernelGGL(dirt::skin_bone_sum_kernel<0>, grid, dim3(dirt::SK_BLOCK), 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return dirt::stage_hip(report, who, e);
        const int shared = transform_scenes == 1 ? 1 : 0;
        hipLaunchKernelGGL(dirt::skin_bone_reduce_kernel, dim3((unsigned)J, shared ? 1u : (unsigned)B), dim3(dirt::SK_BLOCK), 0, s, P.partial,
                           chunk_offsets, grad_transforms, chunks, (int)B, shared);
        if ((e = hipGetLastError()) != hipSuccess) return dirt::stage_hip(report, who, e);
    }
    const bool per_scene_vertices = grad_vertices && P.v_stride != 0;   // (B > 1)
    if (per_scene_vertices) {
        P.gv = grad_vertices;
        const dim3 grid((unsigned)skin_blocks(V), (unsigned)B);
        SKIN_LAUNCH(skin_vertex_backward_kernel, grid, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return dirt::stage_hip(report, who, e);
    }
    if (grad_weights || (grad_vertices && !per_scene_vertices)) {
        P.gv = per_scene_vertices ? nullptr : grad_vertices;
        P.gw = grad_weights;
        const dim3 grid((unsigned)skin_blocks(V));
        SKIN_LAUNCH(skin_shared_backward_kernel, grid, s, P);
        e = hipGetLastError();
    }
    return dirt::stage_hip(report, who, e);
}

}  // extern "C"
