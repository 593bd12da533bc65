// dirt_geometry.hip -- the vertex stage in front of the rasteriser, fused: object-space vertices -> clip-space vertices,
// world positions and world normals in one launch, and the gradients of all three without float atomics.
//
// Replaces the torch composition every sample of the reference starts from (samples/deferred.py:40-51, samples/simple.py:45-56,
// samples/textured.py:97-108): two matrix products and `vertex_normals` (dirt/lighting.py:21-28,31-89) or
// `vertex_normals_pre_split` (dirt/lighting.py:97-129).  The specification (DESIGN.md §7c restates it;
// tests/geometry_reference.py composes it from dirt_amd/lighting.py in float64), per scene, row-vector convention:
//
//     v4 = (x, y, z, w or 1)        world4 = v4 @ model (v4 without a model)        clip = world4 @ view_projection
//     per face (i0, i1, i2), from the first three components of world4:
//         n = (w1 - w0) x (w2 - w0)             fn = n / (|n| + 1e-12)
//     per vertex:  s = sum of fn over the (face, corner) pairs that name the vertex, ordered by face, then corner
//         normals = s / (|s| + 1e-12),   or s itself with DIRT_GEOM_PRE_SPLIT
//
// Gradients are those of torch's autograd for this composition: the norm of a zero vector has gradient 0, so a zero-area
// face hands d fn / 1e-12 to its cross product and nothing through the norm (not guarded), and a vertex whose s is zero
// likewise.
//
// The scatter of the composition (three index_adds forward, three gathers' gradients backward: float atomics on a GPU) is
// a gather here, over an inverted index the caller builds once per topology: offsets [V + 1] and entries [3 F], entry =
// 3 * face + corner, ordered by vertex, then face, then corner.  Every kernel gives one vertex to a lane, which walks its
// list and recomputes each incident face from its three vertices (the model matrix applied on the fly: the vertex array is
// L2-resident at the sizes that matter, 75 000 x 16 B = 1.2 MB).  A list longer than `long_list` entries (a fan's hub) is
// not walked by its lane: after the short lists the wave takes the long ones of its 64 vertices in turn, lane l summing
// entries l, l + 64, ..., and the 64 partial sums are added in a fixed tree.  No atomics, no intermediate per-face tensor,
// and the same bits on every run.
//
// Kernels: geometry_forward_kernel (1 launch).  Backward: geometry_sum_grad_kernel (d loss / d s per vertex, into
// scratch; skipped with DIRT_GEOM_PRE_SPLIT and when the normals carry no gradient), geometry_gather_kernel (per vertex
// the corner gradients of its incident faces, the transforms' terms, d vertices, and per workgroup one row of partial
// sums of d model and d view_projection), geometry_reduce_kernel (the rows added in a fixed order; only when a matrix
// gradient is wanted): 2 launches, + 1 for the matrices.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_stage.h"

namespace dirt {

constexpr int VS_BLOCK = 256;        // lanes of a workgroup = vertices of a workgroup
constexpr int VS_PARTIAL = 32;       // floats of a workgroup's row of partial sums: d model [16], d view_projection [16]

struct VertexStageParams {
    const float* v;            // [B, V, C]
    const int32_t* faces;      // [F, 3]
    const int32_t* offsets;    // [V + 1]
    const int32_t* entries;    // [3 F]
    const float* model;        // [1 or B, 16] or nullptr (identity)
    const float* vp;           // [1 or B, 16] or nullptr
    float* clip;               // forward outputs, each [B, V, 4 / 4 / 3] or nullptr
    float* world;
    float* normals;
    const float* g_clip;       // incoming gradients, each or nullptr
    const float* g_world;
    const float* g_normals;
    const float* g_sum;        // [B, V, 3] d loss / d s (the scratch geometry_sum_grad_kernel wrote, or g_normals itself when pre-split), or nullptr
    float* g_sum_out;          // [B, V, 3] where geometry_sum_grad_kernel writes
    float* gv;                 // [B, V, C] or nullptr
    float* partial;            // [B, blocks, 32] or nullptr
    int V, C;
    int model_stride, vp_stride;   // 16, or 0 for one matrix shared by the scenes
    int pre_split, long_list;
};

// a vertex as the composition sees it: (x, y, z, w or 1)
__device__ __forceinline__ void load_vertex(const VertexStageParams& P, const float* __restrict__ vb, int u, float (&x)[4])
{
    const float* __restrict__ p = vb + (size_t)u * P.C;
    const Float3 t = *reinterpret_cast<const Float3*>(p);
    x[0] = t.x; x[1] = t.y; x[2] = t.z;
    x[3] = P.C == 4 ? p[3] : 1.f;
}

// row vector times matrix, COLS columns of it
template <int COLS>
__device__ __forceinline__ void transform(const float (&x)[4], const float (&m)[16], float (&y)[COLS])
{
#pragma unroll
    for (int j = 0; j < COLS; ++j) y[j] = ((x[0] * m[j] + x[1] * m[4 + j]) + x[2] * m[8 + j]) + x[3] * m[12 + j];
}

// the world position (three components) of vertex u
__device__ __forceinline__ void world3(const VertexStageParams& P, const float* __restrict__ vb, const float (&m)[16], bool has_model, int u,
                                       float (&w)[3])
{
    float x[4];
    load_vertex(P, vb, u, x);
    if (has_model) transform<3>(x, m, w);
    else { w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; }
}

// one face: its two edges from corner 0, their cross product and its length
struct FaceGeo { int i[3]; float e1[3], e2[3], n[3], len; };

__device__ __forceinline__ void face_geometry(const VertexStageParams& P, const float* __restrict__ vb, const float (&m)[16], bool has_model, int f,
                                              FaceGeo& q)
{
    const int32_t* __restrict__ fi = P.faces + (size_t)f * 3;
    q.i[0] = fi[0]; q.i[1] = fi[1]; q.i[2] = fi[2];
    float w0[3], w1[3], w2[3];
    world3(P, vb, m, has_model, q.i[0], w0);
    world3(P, vb, m, has_model, q.i[1], w1);
    world3(P, vb, m, has_model, q.i[2], w2);
#pragma unroll
    for (int j = 0; j < 3; ++j) { q.e1[j] = w1[j] - w0[j]; q.e2[j] = w2[j] - w0[j]; }
    cross3(q.e1, q.e2, q.n);
    q.len = sqrtf(dot3(q.n, q.n));
}

// ---- s = the sum of term(entry) over entries [beg, end) of this lane's vertex.  Lists of up to `long_list` entries are walked
// by their lane, in list order; the longer ones by the whole wave, one after the other.  EVERY lane of the wave must call this
// (lanes without a vertex with beg == end): the wave's part has no divergent entry.
template <class Term>
__device__ __forceinline__ void sum_over_list(const int32_t* __restrict__ entries, int beg, int end, int long_list, Term&& term, float (&s)[3])
{
    s[0] = s[1] = s[2] = 0.f;
    const bool is_long = end - beg > long_list;
    if (!is_long) {
        for (int e = beg; e < end; ++e) {
            float c[3];
            term(entries[e], c);
            s[0] += c[0]; s[1] += c[1]; s[2] += c[2];
        }
    }
    unsigned long long pending = __ballot(is_long);
    if (pending == 0) return;
    const int lane = threadIdx.x & 63;
    while (pending) {   // (wave-uniform)
        const int src = __ffsll(pending) - 1;
        pending &= pending - 1;
        const int b2 = __builtin_amdgcn_readlane(beg, src), e2 = __builtin_amdgcn_readlane(end, src);
        float p[3] = {0.f, 0.f, 0.f};
        for (int e = b2 + lane; e < e2; e += 64) {
            float c[3];
            term(entries[e], c);
            p[0] += c[0]; p[1] += c[1]; p[2] += c[2];
        }
        p[0] = wave_sum(p[0]); p[1] = wave_sum(p[1]); p[2] = wave_sum(p[2]);
        if (lane == src) { s[0] = p[0]; s[1] = p[1]; s[2] = p[2]; }
    }
}

// the un-normalised normal sum s of a lane's vertex
__device__ __forceinline__ void normal_sum(const VertexStageParams& P, const float* __restrict__ vb, const float (&m)[16], bool has_model, int beg,
                                           int end, float (&s)[3])
{
    sum_over_list(P.entries, beg, end, P.long_list, [&](int entry, float (&c)[3]) {
        FaceGeo q;
        face_geometry(P, vb, m, has_model, entry / 3, q);
        const float inv = 1.f / (q.len + 1.e-12f);
        c[0] = q.n[0] * inv; c[1] = q.n[1] * inv; c[2] = q.n[2] * inv;
    }, s);
}

__device__ __forceinline__ void load_matrix(const float* __restrict__ p, float (&m)[16])
{
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = p[k];   // a wave-uniform address: scalar loads
}

// ---- forward: one vertex per lane
__global__ __launch_bounds__(VS_BLOCK) void geometry_forward_kernel(VertexStageParams P)
{
    const int i = blockIdx.x * VS_BLOCK + threadIdx.x;
    const bool live = i < P.V;
    const size_t row = (size_t)blockIdx.y * P.V + (live ? i : 0);
    const float* __restrict__ vb = P.v + (size_t)blockIdx.y * P.V * P.C;
    const bool has_model = P.model != nullptr;
    float m[16];
    if (has_model) load_matrix(P.model + (size_t)blockIdx.y * P.model_stride, m);
    if (live && (P.clip || P.world)) {
        float x[4], w[4];
        load_vertex(P, vb, i, x);
        if (has_model) transform<4>(x, m, w);
        else { w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; w[3] = x[3]; }
        if (P.world) *reinterpret_cast<Float4*>(P.world + row * 4) = Float4{w[0], w[1], w[2], w[3]};
        if (P.clip) {
            float q[16], c[4];
            load_matrix(P.vp + (size_t)blockIdx.y * P.vp_stride, q);
            transform<4>(w, q, c);
            *reinterpret_cast<Float4*>(P.clip + row * 4) = Float4{c[0], c[1], c[2], c[3]};
        }
    }
    if (!P.normals) return;   // (uniform)
    const int beg = live ? P.offsets[i] : 0, end = live ? P.offsets[i + 1] : 0;
    float s[3];
    normal_sum(P, vb, m, has_model, beg, end, s);
    if (!live) return;
    if (!P.pre_split) {
        const float inv = 1.f / (sqrtf(dot3(s, s)) + 1.e-12f);
        s[0] *= inv; s[1] *= inv; s[2] *= inv;
    }
    store3(P.normals + row * 3, s);
}

// ---- backward, first launch: d loss / d s from d loss / d normals, per vertex (s recomputed as the forward computes it)
__global__ __launch_bounds__(VS_BLOCK) void geometry_sum_grad_kernel(VertexStageParams P)
{
    const int i = blockIdx.x * VS_BLOCK + threadIdx.x;
    const bool live = i < P.V;
    const size_t row = (size_t)blockIdx.y * P.V + (live ? i : 0);
    const float* __restrict__ vb = P.v + (size_t)blockIdx.y * P.V * P.C;
    const bool has_model = P.model != nullptr;
    float m[16];
    if (has_model) load_matrix(P.model + (size_t)blockIdx.y * P.model_stride, m);
    const int beg = live ? P.offsets[i] : 0, end = live ? P.offsets[i + 1] : 0;
    float s[3];
    normal_sum(P, vb, m, has_model, beg, end, s);
    if (!live) return;
    float gn[3];
    load3(P.g_normals + row * 3, gn);
    // normals = s / (L + 1e-12):  d s = gn / (L + 1e-12) + (d L) s / L,  d L = -(gn . s) / (L + 1e-12)^2;  nothing through L at s = 0
    const float L = sqrtf(dot3(s, s)), inv = 1.f / (L + 1.e-12f);
    const float k = L == 0.f ? 0.f : -((dot3(gn, s) * inv) * inv) / L;
    const float gs[3] = {gn[0] * inv + s[0] * k, gn[1] * inv + s[1] * k, gn[2] * inv + s[2] * k};
    store3(P.g_sum_out + row * 3, gs);
}

// ---- backward, second launch: per vertex, the gradient its incident faces send to its world position (each face's gradient
// recomputed from the d s of its three vertices), the transforms' terms, d vertices; MATS: one row of partial sums of
// d model and d view_projection per workgroup
template <bool MATS>
__global__ __launch_bounds__(VS_BLOCK) void geometry_gather_kernel(VertexStageParams P)
{
    __shared__ float s_part[MATS ? 4 * VS_PARTIAL : 1];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * VS_BLOCK + tid;
    const bool live = i < P.V;
    const size_t row = (size_t)blockIdx.y * P.V + (live ? i : 0);
    const float* __restrict__ vb = P.v + (size_t)blockIdx.y * P.V * P.C;
    const bool has_model = P.model != nullptr;
    float m[16];
    if (has_model) load_matrix(P.model + (size_t)blockIdx.y * P.model_stride, m);
    float G[4] = {0.f, 0.f, 0.f, 0.f};   // d loss / d world4 of this vertex
    if (P.g_sum) {   // (uniform)
        const float* __restrict__ gs = P.g_sum + (size_t)blockIdx.y * P.V * 3;
        const int beg = live ? P.offsets[i] : 0, end = live ? P.offsets[i + 1] : 0;
        float s[3];
        sum_over_list(P.entries, beg, end, P.long_list, [&](int entry, float (&c)[3]) {
            const int f = entry / 3, corner = entry - 3 * f;
            FaceGeo q;
            face_geometry(P, vb, m, has_model, f, q);
            float gf[3];   // d loss / d fn: the face's unit normal went to its three vertices
            {
                const Float3 a = *reinterpret_cast<const Float3*>(gs + (size_t)q.i[0] * 3), b = *reinterpret_cast<const Float3*>(gs + (size_t)q.i[1] * 3),
                         d = *reinterpret_cast<const Float3*>(gs + (size_t)q.i[2] * 3);
                gf[0] = (a.x + b.x) + d.x; gf[1] = (a.y + b.y) + d.y; gf[2] = (a.z + b.z) + d.z;
            }
            // fn = n / (len + 1e-12): as for s above; a zero-area face passes gf / 1e-12 on
            const float inv = 1.f / (q.len + 1.e-12f);
            const float k = q.len == 0.f ? 0.f : -((dot3(gf, q.n) * inv) * inv) / q.len;
            const float gn[3] = {gf[0] * inv + q.n[0] * k, gf[1] * inv + q.n[1] * k, gf[2] * inv + q.n[2] * k};
            // n = e1 x e2:  d e1 = e2 x gn,  d e2 = gn x e1;  corner 1 receives d e1, corner 2 d e2, corner 0 minus both
            float ge1[3], ge2[3];
            cross3(q.e2, gn, ge1);
            cross3(gn, q.e1, ge2);
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] = corner == 1 ? ge1[j] : (corner == 2 ? ge2[j] : -(ge1[j] + ge2[j]));
        }, s);
        G[0] = s[0]; G[1] = s[1]; G[2] = s[2];
    }
    float x[4] = {0.f, 0.f, 0.f, 0.f}, w[4] = {0.f, 0.f, 0.f, 0.f}, gc[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        load_vertex(P, vb, i, x);
        if (has_model) transform<4>(x, m, w);
        else { w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; w[3] = x[3]; }
        if (P.g_world) {
            const Float4 t = *reinterpret_cast<const Float4*>(P.g_world + row * 4);
            G[0] += t.x; G[1] += t.y; G[2] += t.z; G[3] += t.w;
        }
        if (P.g_clip) {   // clip = world4 @ vp
            const Float4 t = *reinterpret_cast<const Float4*>(P.g_clip + row * 4);
            gc[0] = t.x; gc[1] = t.y; gc[2] = t.z; gc[3] = t.w;
            float q[16];
            load_matrix(P.vp + (size_t)blockIdx.y * P.vp_stride, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) G[j] += ((gc[0] * q[4 * j] + gc[1] * q[4 * j + 1]) + gc[2] * q[4 * j + 2]) + gc[3] * q[4 * j + 3];
        }
        if (P.gv) {   // world4 = v4 @ model
            float g[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                g[r] = has_model ? ((G[0] * m[4 * r] + G[1] * m[4 * r + 1]) + G[2] * m[4 * r + 2]) + G[3] * m[4 * r + 3] : G[r];
            float* __restrict__ o = P.gv + row * P.C;
            *reinterpret_cast<Float3*>(o) = Float3{g[0], g[1], g[2]};
            if (P.C == 4) o[3] = g[3];
        }
    }
    if constexpr (MATS) {
        const int wave = tid >> 6, lane = tid & 63;
        // d model[r][j] = sum over vertices of v4[r] G[j];  d view_projection[r][j] = sum of world4[r] gc[j]  (zeros from lanes without a vertex)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = wave_sum(live ? x[r] * G[j] : 0.f), b = wave_sum(live ? w[r] * gc[j] : 0.f);
                if (lane == 0) { s_part[wave * VS_PARTIAL + 4 * r + j] = a; s_part[wave * VS_PARTIAL + 16 + 4 * r + j] = b; }
            }
        }
        __syncthreads();
        if (tid < VS_PARTIAL) fold_waves_to_row<VS_PARTIAL>(s_part, P.partial, tid);
    }
}

// ---- backward, last launch: the rows of partial sums added in a fixed order (block_column_sum).  Workgroup (k, b) sums value k (0-15: d model,
// 16-31: d view_projection) of scene b -- or, for a matrix shared by the scenes, workgroup (k, 0) that of all of them
__global__ __launch_bounds__(VS_BLOCK) void geometry_reduce_kernel(const float* __restrict__ partial, float* __restrict__ g_model, float* __restrict__ g_vp,
                                                                   int model_shared, int vp_shared, long long blocks, int B)
{
    __shared__ float s_sum[VS_BLOCK];
    const int k = blockIdx.x, b = blockIdx.y;
    float* __restrict__ out = k < 16 ? g_model : g_vp;
    const bool shared = k < 16 ? model_shared : vp_shared;
    if (!out || (shared && b != 0)) return;   // (uniform)
    const long long rows = shared ? blocks * B : blocks;
    const float total = block_column_sum<VS_BLOCK>(partial + (size_t)b * blocks * VS_PARTIAL + k, rows, VS_PARTIAL, s_sum);
    if (threadIdx.x == 0) out[(size_t)b * 16 + (k & 15)] = total;
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

static long long geom_blocks(long long V) { return (V + dirt::VS_BLOCK - 1) / dirt::VS_BLOCK; }

static bool geom_sizes_ok(long long B, long long V, long long F)
{
    return B >= 0 && B <= 65535 && V >= 0 && V <= DIRT_GEOM_MAX_VERTICES && F >= 0 && F <= DIRT_GEOM_MAX_FACES;
}

static int geom_check(const char* who, const float* vertices, int components, const int32_t* faces, const int32_t* offsets, const int32_t* entries,
                      const float* model, int model_scenes, const float* view_projection, int vp_scenes, long long B, long long V, long long F,
                      unsigned flags, dirt::VertexStageParams& P)
{
    if (B < 0 || V < 0 || F < 0) STAGE_FAIL("%s: negative sizes (B=%lld V=%lld F=%lld)", who, B, V, F);
    if (!geom_sizes_ok(B, V, F)) STAGE_FAIL("%s: B=%lld V=%lld F=%lld, at most 65535 scenes, %d vertices, %d faces", who, B, V, F,
                                            DIRT_GEOM_MAX_VERTICES, DIRT_GEOM_MAX_FACES);
    if (components != 3 && components != 4) STAGE_FAIL("%s: vertices have %d components, 3 or 4", who, components);
    if (model_scenes != 0 && model_scenes != 1 && model_scenes != B) STAGE_FAIL("%s: model_scenes=%d is none of 0, 1, B=%lld", who, model_scenes, B);
    if (vp_scenes != 0 && vp_scenes != 1 && vp_scenes != B) STAGE_FAIL("%s: view_projection_scenes=%d is none of 0, 1, B=%lld", who, vp_scenes, B);
    if (flags & ~(DIRT_GEOM_PRE_SPLIT | DIRT_GEOM_LONG_LIST_MASK)) STAGE_FAIL("%s: unknown flags 0x%x", who, flags);
    if (B == 0 || V == 0) return DIRT_OK;
    if (!vertices || !offsets) STAGE_FAIL("%s: vertices / offsets is NULL", who);
    if (F > 0 && (!faces || !entries)) STAGE_FAIL("%s: faces / entries is NULL", who);
    if ((model_scenes != 0) != (model != nullptr)) STAGE_FAIL("%s: model and model_scenes=%d disagree", who, model_scenes);
    if ((vp_scenes != 0) != (view_projection != nullptr)) STAGE_FAIL("%s: view_projection and view_projection_scenes=%d disagree", who, vp_scenes);
    P.v = vertices; P.faces = faces; P.offsets = offsets; P.entries = entries; P.model = model; P.vp = view_projection;
    P.V = (int)V; P.C = components;
    P.model_stride = model_scenes == 1 ? 0 : 16; P.vp_stride = vp_scenes == 1 ? 0 : 16;
    P.pre_split = (flags & DIRT_GEOM_PRE_SPLIT) ? 1 : 0;
    const int asked = (int)((flags & DIRT_GEOM_LONG_LIST_MASK) >> DIRT_GEOM_LONG_LIST_SHIFT);
    P.long_list = asked ? asked : DIRT_GEOM_LONG_LIST_DEFAULT;
    return DIRT_OK;
}

size_t dirt_geometry_scratch_bytes(long long B, long long V, long long F)
{
    if (!geom_sizes_ok(B, V, F)) return 0;
    return sizeof(float) * ((size_t)B * (size_t)V * 3 + (size_t)B * (size_t)geom_blocks(V) * dirt::VS_PARTIAL);
}

int dirt_geometry_forward(const float* vertices, int components, const int32_t* faces, const int32_t* offsets, const int32_t* entries,
                          const float* model, int model_scenes, const float* view_projection, int view_projection_scenes, float* clip,
                          float* world, float* normals, long long B, long long V, long long F, unsigned flags, void* stream)
{
    const char* who = "dirt_geometry_forward";
    dirt::VertexStageParams P{};
    int rc = geom_check(who, vertices, components, faces, offsets, entries, model, model_scenes, view_projection, view_projection_scenes, B, V, F,
                        flags, P);
    if (rc) return rc;
    if (B == 0 || V == 0 || (!clip && !world && !normals)) return dirt::stage_ok(report);
    if (clip && !view_projection) STAGE_FAIL("%s: clip is wanted and there is no view_projection", who);
    P.clip = clip; P.world = world; P.normals = normals;
    const dim3 grid((unsigned)geom_blocks(V), (unsigned)B);
    hipLaunchKernelGGL(dirt::geometry_forward_kernel, grid, dim3(dirt::VS_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_geometry_backward(const float* vertices, int components, const int32_t* faces, const int32_t* offsets, const int32_t* entries,
                           const float* model, int model_scenes, const float* view_projection, int view_projection_scenes,
                           const float* grad_clip, const float* grad_world, const float* grad_normals, float* grad_vertices, float* grad_model,
                           float* grad_view_projection, void* scratch, size_t scratch_bytes, long long B, long long V, long long F,
                           unsigned flags, void* stream)
{
    const char* who = "dirt_geometry_backward";
    dirt::VertexStageParams P{};
    int rc = geom_check(who, vertices, components, faces, offsets, entries, model, model_scenes, view_projection, view_projection_scenes, B, V, F,
                        flags, P);
    if (rc) return rc;
    if (B == 0 || V == 0 || (!grad_vertices && !grad_model && !grad_view_projection)) return dirt::stage_ok(report);
    if (grad_clip && !view_projection) STAGE_FAIL("%s: grad_clip is given and there is no view_projection", who);
    if (grad_model && !model) STAGE_FAIL("%s: grad_model is wanted and there is no model", who);
    if (grad_view_projection && !view_projection) STAGE_FAIL("%s: grad_view_projection is wanted and there is no view_projection", who);
    const bool mats = grad_model || grad_view_projection, sum_pass = grad_normals && !P.pre_split;
    if (mats || sum_pass) {
        rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_geometry_scratch_bytes(B, V, F), "dirt_geometry_scratch_bytes");
        if (rc) return rc;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long blocks = geom_blocks(V);
    const dim3 grid((unsigned)blocks, (unsigned)B);
    float* sums = static_cast<float*>(scratch);
    P.g_clip = grad_clip; P.g_world = grad_world; P.g_normals = grad_normals; P.gv = grad_vertices;
    P.partial = mats ? sums + (size_t)B * (size_t)V * 3 : nullptr;
    P.g_sum = grad_normals;   // pre-split: the normals ARE the sums
    if (sum_pass) {
        P.g_sum_out = sums;
        P.g_sum = sums;
        hipLaunchKernelGGL(dirt::geometry_sum_grad_kernel, grid, dim3(dirt::VS_BLOCK), 0, s, P);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return dirt::stage_hip(report, who, e);
    }
    if (mats) hipLaunchKernelGGL(dirt::geometry_gather_kernel<true>, grid, dim3(dirt::VS_BLOCK), 0, s, P);
    else hipLaunchKernelGGL(dirt::geometry_gather_kernel<false>, grid, dim3(dirt::VS_BLOCK), 0, s, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dirt::stage_hip(report, who, e);
    if (mats) {
        hipLaunchKernelGGL(dirt::geometry_reduce_kernel, dim3(dirt::VS_PARTIAL, (unsigned)B), dim3(dirt::VS_BLOCK), 0, s, P.partial, grad_model,
                           grad_view_projection, model_scenes == 1 ? 1 : 0, view_projection_scenes == 1 ? 1 : 0, blocks, (int)B);
        e = hipGetLastError();
    }
    return dirt::stage_hip(report, who, e);
}

}  // extern "C"
