// dirt_tangent.hip -- per-vertex tangent frames from the uv parametrisation, fused: one launch forward, two backward, no float
// atomics and the same bits on every run.
//
// The geometry side of tangent-space normal mapping (the pixel side is dirt_normal_map.hip).  The specification (DESIGN.md §7g
// restates it; dirt_amd/lighting.py::vertex_tangents is its readable form, which tests/normal_map_reference.py restates in
// float64), per scene, with the uvs [V, 2] shared by the scenes:
//
//     per face (i0, i1, i2):  e1 = p1 - p0, e2 = p2 - p0     (du1, dv1) = uv1 - uv0, (du2, dv2) = uv2 - uv0
//         det = du1 dv2 - du2 dv1,  s = sign(det)
//         t_f = (s dv2) e1 - (s dv1) e2               b_f = (s du1) e2 - (s du2) e1
//         a face is LIVE iff det is finite and non-zero; a dead face (a degenerate uv triangle, a NaN or Inf uv) has the four
//         coefficients s dv2, s dv1, s du1, s du2 exactly 0, whatever its uvs hold: it adds nothing to T, Bt or any gradient
//     per vertex:  T, Bt = the sums of t_f, b_f over the (face, corner) pairs that name the vertex, in list order
//         x = T - n (n . T)       t = x / |x| where x . x > 0, else 0       w = -1 where cross(n, t) . Bt < 0, else +1
//         out = (t, w)
//
// Gradients go to the positions and to the normals; w is a sign and Bt feeds only it, so neither carries one, and the
// incoming gradient of w is not read.  With gt = d loss / d t:
//
//     gx = (gt - t (t . gt)) / |x|        G_T = d loss / d T = gx - n (n . gx)        d n = -((n . T) gx + T (n . gx))
//
// and nothing where x . x = 0.  Every t_f is linear in the positions with coefficients a = s dv2, b = s dv1 that depend on the
// uvs only, and it was added to T of each of the face's three corners: so the gradient of a position is a GATHER over the
// same inverted index the forward walks (MeshTopology: offsets [V + 1], entries [3 F], entry = 3 * face + corner),
//
//     d p_v = sum over the entries (f, corner) of v of  coefficient(f, corner) * (G_T[i0] + G_T[i1] + G_T[i2]),
//     coefficient = a at corner 1, -b at corner 2, b - a at corner 0.
//
// Kernels: tangent_forward_kernel.  Backward: tangent_frame_grad_kernel (T again per vertex; G_T into caller scratch, d n),
// tangent_gather_kernel (d vertices; only when they are wanted).  A lane has one vertex and walks its list itself, however
// long: a fan's hub of hundreds of entries is summed by its one lane, correct and in list order but serial (dirt_geometry.hip
// hands such lists to the wave; that path was not built here -- DESIGN.md §7g).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_stage.h"

namespace dirt {

constexpr int TG_BLOCK = 256;        // lanes of a workgroup = vertices of a workgroup

struct TangentParams {
    const float* v;            // [B, V, C]
    const float* n;            // [B, V, 3]
    const float* uv;           // [V, 2]
    const int32_t* faces;      // [F, 3]
    const int32_t* offsets;    // [V + 1]
    const int32_t* entries;    // [3 F]
    float* out;                // [B, V, 4]
    const float* g_out;        // [B, V, 4]
    float* g_sum;              // [B, V, 3] scratch: d loss / d T, written by the first backward launch and read by the second, or nullptr
    float* gv;                 // [B, V, C] or nullptr
    float* gn;                 // [B, V, 3] or nullptr
    int V, C;
};

// a face as the tangent sums see it: its vertices and the two uv-only coefficients of t_f = a e1 - b e2, and those of b_f = c e2 - d e1
struct FaceUv { int i[3]; float a, b, c, d; };
struct Float2 { float x, y; };   // a (u, v) pair, 4-byte aligned (a float2 would promise 8): one 8-byte access

__device__ __forceinline__ void face_uv(const TangentParams& P, int f, FaceUv& q)
{
    const int32_t* __restrict__ fi = P.faces + (size_t)f * 3;
    q.i[0] = fi[0]; q.i[1] = fi[1]; q.i[2] = fi[2];
    const Float2 u0 = *reinterpret_cast<const Float2*>(P.uv + (size_t)q.i[0] * 2), u1 = *reinterpret_cast<const Float2*>(P.uv + (size_t)q.i[1] * 2),
                 u2 = *reinterpret_cast<const Float2*>(P.uv + (size_t)q.i[2] * 2);
    const float du1 = u1.x - u0.x, dv1 = u1.y - u0.y, du2 = u2.x - u0.x, dv2 = u2.y - u0.y;
    const float det = du1 * dv2 - du2 * dv1;
    const bool live = fabsf(det) < INFINITY && det != 0.f;        // finite and non-zero (a NaN fails the first comparison)
    const float s = det > 0.f ? 1.f : -1.f;                       // sign(det) of a live face
    q.a = live ? s * dv2 : 0.f; q.b = live ? s * dv1 : 0.f;       // selects, not products: 0 * NaN is NaN
    q.c = live ? s * du1 : 0.f; q.d = live ? s * du2 : 0.f;
}

// T (and, BITANGENT, Bt) of the vertex whose list is entries [beg, end), summed in list order
template <bool BITANGENT>
__device__ __forceinline__ void tangent_sums(const TangentParams& P, const float* __restrict__ vb, int beg, int end, float (&T)[3], float (&Bt)[3])
{
    T[0] = T[1] = T[2] = 0.f;
    Bt[0] = Bt[1] = Bt[2] = 0.f;
    for (int e = beg; e < end; ++e) {
        FaceUv q;
        face_uv(P, P.entries[e] / 3, q);
        float p0[3], p1[3], p2[3];
        load3(vb + (size_t)q.i[0] * P.C, p0);
        load3(vb + (size_t)q.i[1] * P.C, p1);
        load3(vb + (size_t)q.i[2] * P.C, p2);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float e1 = p1[j] - p0[j], e2 = p2[j] - p0[j];
            T[j] += q.a * e1 - q.b * e2;
            if constexpr (BITANGENT) Bt[j] += q.c * e2 - q.d * e1;
        }
    }
}

// x = T - n (n . T) and its squared length
__device__ __forceinline__ float reject(const float (&T)[3], const float (&n)[3], float (&x)[3])
{
    const float nt = dot3(n, T);
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = T[j] - n[j] * nt;
    return dot3(x, x);
}

// ---- forward: one vertex per lane
__global__ __launch_bounds__(TG_BLOCK) void tangent_forward_kernel(TangentParams P)
{
    const int i = blockIdx.x * TG_BLOCK + threadIdx.x;
    if (i >= P.V) return;
    const size_t row = (size_t)blockIdx.y * P.V + i;
    const float* __restrict__ vb = P.v + (size_t)blockIdx.y * P.V * P.C;
    float T[3], Bt[3], n[3], x[3];
    tangent_sums<true>(P, vb, P.offsets[i], P.offsets[i + 1], T, Bt);
    load3(P.n + row * 3, n);
    const float xx = reject(T, n, x);
    float t[3] = {0.f, 0.f, 0.f};
    if (xx > 0.f) {
        const float len = sqrtf(xx);
        t[0] = x[0] / len; t[1] = x[1] / len; t[2] = x[2] / len;
    }
    float c[3];
    cross3(n, t, c);
    const float w = dot3(c, Bt) < 0.f ? -1.f : 1.f;
    *reinterpret_cast<Float4*>(P.out + row * 4) = Float4{t[0], t[1], t[2], w};
}

// ---- backward, first launch: d loss / d T per vertex (T recomputed as the forward computes it) into scratch, and d normals
__global__ __launch_bounds__(TG_BLOCK) void tangent_frame_grad_kernel(TangentParams P)
{
    const int i = blockIdx.x * TG_BLOCK + threadIdx.x;
    if (i >= P.V) return;
    const size_t row = (size_t)blockIdx.y * P.V + i;
    const float* __restrict__ vb = P.v + (size_t)blockIdx.y * P.V * P.C;
    float T[3], Bt[3], n[3], x[3];
    tangent_sums<false>(P, vb, P.offsets[i], P.offsets[i + 1], T, Bt);
    load3(P.n + row * 3, n);
    const float xx = reject(T, n, x);
    float gT[3] = {0.f, 0.f, 0.f}, gn[3] = {0.f, 0.f, 0.f};
    if (xx > 0.f) {
        const float len = sqrtf(xx);
        const Float4 go = *reinterpret_cast<const Float4*>(P.g_out + row * 4);   // (go.w, the sign's, is not used)
        const float gt[3] = {go.x, go.y, go.z};
        const float t[3] = {x[0] / len, x[1] / len, x[2] / len};
        const float tg = dot3(t, gt);
        float gx[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) gx[j] = (gt[j] - t[j] * tg) / len;
        const float ng = dot3(n, gx), nt = dot3(n, T);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            gT[j] = gx[j] - n[j] * ng;
            gn[j] = -(nt * gx[j] + T[j] * ng);
        }
    }
    if (P.g_sum) store3(P.g_sum + row * 3, gT);
    if (P.gn) store3(P.gn + row * 3, gn);
}

// ---- backward, second launch: d vertices, gathered over each vertex's list from the d loss / d T of its faces' corners
__global__ __launch_bounds__(TG_BLOCK) void tangent_gather_kernel(TangentParams P)
{
    const int i = blockIdx.x * TG_BLOCK + threadIdx.x;
    if (i >= P.V) return;
    const size_t row = (size_t)blockIdx.y * P.V + i;
    const float* __restrict__ gs = P.g_sum + (size_t)blockIdx.y * P.V * 3;
    float g[3] = {0.f, 0.f, 0.f};
    const int beg = P.offsets[i], end = P.offsets[i + 1];
    for (int e = beg; e < end; ++e) {
        const int entry = P.entries[e], f = entry / 3, corner = entry - 3 * f;
        FaceUv q;
        face_uv(P, f, q);
        float g0[3], g1[3], g2[3];
        load3(gs + (size_t)q.i[0] * 3, g0);
        load3(gs + (size_t)q.i[1] * 3, g1);
        load3(gs + (size_t)q.i[2] * 3, g2);
        const float k = corner == 1 ? q.a : (corner == 2 ? -q.b : q.b - q.a);
#pragma unroll
        for (int j = 0; j < 3; ++j) g[j] += k * ((g0[j] + g1[j]) + g2[j]);
    }
    float* __restrict__ o = P.gv + row * P.C;
    store3(o, g);
    if (P.C == 4) o[3] = 0.f;
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

static bool tangent_sizes_ok(long long B, long long V, long long F)
{
    return B >= 0 && B <= 65535 && V >= 0 && V <= DIRT_GEOM_MAX_VERTICES && F >= 0 && F <= DIRT_GEOM_MAX_FACES;
}

static int tangent_check(const char* who, const float* vertices, int components, const float* normals, const float* uvs, const int32_t* faces,
                         const int32_t* offsets, const int32_t* entries, long long B, long long V, long long F, dirt::TangentParams& P)
{
    if (B < 0 || V < 0 || F < 0) STAGE_FAIL("%s: negative sizes (B=%lld V=%lld F=%lld)", who, B, V, F);
    if (!tangent_sizes_ok(B, V, F)) STAGE_FAIL("%s: B=%lld V=%lld F=%lld, at most 65535 scenes, %d vertices, %d faces", who, B, V, F,
                                               DIRT_GEOM_MAX_VERTICES, DIRT_GEOM_MAX_FACES);
    if (components != 3 && components != 4) STAGE_FAIL("%s: vertices have %d components, 3 or 4", who, components);
    if (B == 0 || V == 0) return DIRT_OK;
    if (!vertices || !normals || !uvs || !offsets) STAGE_FAIL("%s: vertices / normals / uvs / offsets is NULL", who);
    if (F > 0 && (!faces || !entries)) STAGE_FAIL("%s: faces / entries is NULL", who);
    P.v = vertices; P.n = normals; P.uv = uvs; P.faces = faces; P.offsets = offsets; P.entries = entries;
    P.V = (int)V; P.C = components;
    return DIRT_OK;
}

size_t dirt_tangent_scratch_bytes(long long B, long long V, long long F)
{
    if (!tangent_sizes_ok(B, V, F)) return 0;
    return sizeof(float) * (size_t)B * (size_t)V * 3;
}

int dirt_tangent_forward(const float* vertices, int components, const float* normals, const float* uvs, const int32_t* faces,
                         const int32_t* offsets, const int32_t* entries, float* tangents, long long B, long long V, long long F, void* stream)
{
    const char* who = "dirt_tangent_forward";
    dirt::TangentParams P{};
    int rc = tangent_check(who, vertices, components, normals, uvs, faces, offsets, entries, B, V, F, P);
    if (rc) return rc;
    if (B == 0 || V == 0) return dirt::stage_ok(report);
    if (!tangents) STAGE_FAIL("%s: tangents is NULL", who);
    P.out = tangents;
    const dim3 grid((unsigned)((V + dirt::TG_BLOCK - 1) / dirt::TG_BLOCK), (unsigned)B);
    hipLaunchKernelGGL(dirt::tangent_forward_kernel, grid, dim3(dirt::TG_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_tangent_backward(const float* vertices, int components, const float* normals, const float* uvs, const int32_t* faces,
                          const int32_t* offsets, const int32_t* entries, const float* grad_tangents, float* grad_vertices,
                          float* grad_normals, void* scratch, size_t scratch_bytes, long long B, long long V, long long F, void* stream)
{
    const char* who = "dirt_tangent_backward";
    dirt::TangentParams P{};
    int rc = tangent_check(who, vertices, components, normals, uvs, faces, offsets, entries, B, V, F, P);
    if (rc) return rc;
    if (B == 0 || V == 0 || (!grad_vertices && !grad_normals)) return dirt::stage_ok(report);
    if (!grad_tangents) STAGE_FAIL("%s: grad_tangents is NULL", who);
    if (grad_vertices) {
        rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_tangent_scratch_bytes(B, V, F), "dirt_tangent_scratch_bytes");
        if (rc) return rc;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((V + dirt::TG_BLOCK - 1) / dirt::TG_BLOCK), (unsigned)B);
    P.g_out = grad_tangents; P.gv = grad_vertices; P.gn = grad_normals;
    P.g_sum = grad_vertices ? static_cast<float*>(scratch) : nullptr;
    hipLaunchKernelGGL(dirt::tangent_frame_grad_kernel, grid, dim3(dirt::TG_BLOCK), 0, s, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !grad_vertices) return dirt::stage_hip(report, who, e);
    hipLaunchKernelGGL(dirt::tangent_gather_kernel, grid, dim3(dirt::TG_BLOCK), 0, s, P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

}  // extern "C"
