// dirt_kinematics.hip -- forward kinematics in front of the skinning stage, fused: angle-axis rotations and rest-pose joint
// positions of a skeleton (a forest: parents come before their children) -> the bone transforms `skin_vertices` takes and
// the posed joint positions, in one launch; and the gradients to the rotations and the joints without float atomics.
//
// Extends what the reference's samples do with ONE matrices.rodrigues / compose per mesh (samples/deferred.py:40-41;
// dirt/matrices.py:15-61,183-207) to a tree of them.  The specification (DESIGN.md §7e restates it;
// tests/kinematics_reference.py composes it in float64), per scene, float32, row vectors:
//
//     R[j]  = matrices.rodrigues(r[j], three_by_three=True)     operation for operation: v = r + 1e-12, n = |v|, k = v / n,
//                                                               c I + (1 - c) k k^T + s K with c = cosf(n), s = sinf(n)
//     tl[j] = p[j] - p[j] @ R[j]                                L[j] = translation(-p[j]) @ R[j] @ translation(p[j])
//     root:   S3[j] = R[j],               t[j] = tl[j]
//     else:   S3[j] = R[j] @ S3[parent],  t[j] = tl[j] @ S3[parent] + t[parent]               S[j] = L[j] @ S[parent]
//     transforms[j] = [[S3[j], 0], [t[j], 1]]                   column 3 is written as exactly (0, 0, 0, 1)
//     posed_joints[j] = p[j] @ S3[j] + t[j]
//
// Gradients are those of torch's autograd for this composition (the one at a zero rotation vector included: it exists
// because of the 1e-12); the incoming gradient of column 3 is ignored; an output nobody used (a NULL gradient) contributes
// nothing.  With GS[j] / Gt[j] the gradient of S3[j] / t[j]:
//     seed:     GS[j] = gT[j][:3, :3] + outer(p[j], gq[j]),   Gt[j] = gT[j][3, :3] + gq[j],   d p[j] = S3[j] @ gq[j]
//     children: GS[j] += R[c]^T @ GS[c] + outer(tl[c], Gt[c]),  Gt[j] += Gt[c]       over the children c of j, in index order
//     own:      d R = GS[j] @ S3[parent]^T,  d tl = Gt[j] @ S3[parent]^T             (a root: d R = GS[j], d tl = Gt[j])
//               d p[j] += d tl - R[j] @ d tl,   d R -= outer(p[j], d tl),   d r[j] = (Rodrigues derivative)(d R)
// The scatter of a child's block into its parent is a gather here, over the inverted index of `parents` the caller builds
// once per rig (dirt_amd.kinematics.Skeleton): `child_entries`, the non-root joints ordered by parent, then index, and
// `child_offsets` [J + 1]; the joints of one depth form a level (`order` [J]: the joints by depth, then index;
// `level_offsets` [levels + 1]).
//
// Kernels (BLOCK = 64 lanes for J <= 64 -- one wave, whose barriers cost nothing -- and 256 otherwise):
//   kinematics_forward_kernel<BLOCK>    a workgroup per scene, lane i owns joint order[i] for the whole kernel: the
//                                       Rodrigues step of all joints first, in parallel and in registers; then the levels
//                                       in turn with a barrier between them, every joint's 12 values (S3, t) staying in LDS
//                                       for its children.
//   kinematics_backward_kernel<BLOCK>   the same shape: recomputes the forward into LDS, seeds every joint's 12-value
//                                       gradient, walks the levels in reverse -- a joint adds the blocks its children left
//                                       in LDS (in the slot of their own, by then dead, S3 / t), leaves its own block for
//                                       its parent -- and ends with the Rodrigues derivative of all joints in parallel.
//                                       Rows of an operand shared by B > 1 scenes go to caller-owned scratch.
//   kinematics_reduce_kernel            a workgroup per joint adds the joint's rows of all scenes in a fixed order (up to 42
//                                       scenes: scene order): the shape of the skinning stage's reduce kernel, six totals
//                                       per workgroup from rows of six.
// Static LDS of the forward and backward kernels: 256 joints x 12 floats = 12 288 bytes, + 257 level offsets (1 028) and,
// backward, 256 child entries (1 024): 14 340 bytes at most, of the 64 KB a workgroup may have.
// No atomics anywhere (global or LDS), and the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_stage.h"

#ifndef DIRT_KINEMATICS_SMALL_BLOCK
#define DIRT_KINEMATICS_SMALL_BLOCK 64   // lanes of the workgroup for J <= 64 (256: the A/B build of tools/bench_kinematics.py)
#endif

namespace dirt {

constexpr int KN_ROW = 12;           // floats of a joint's block: S3 row-major, then t
constexpr int KN_COLS = 6;           // floats of a scratch row: d r, d p of one (scene, joint)
constexpr int KN_SLOTS = 42;         // the reduce kernel: 42 x 6 = 252 of its 256 lanes each sum every 42nd row of one column
constexpr int KN_REDUCE_BLOCK = 256;

struct KinParams {
    const float* r;               // [1 or B, J, 3] angle-axis rotations
    const float* p;               // [1 or B, J, 3] rest-pose joint positions
    const int32_t* parents;       // [J]
    const int32_t* order;         // [J]
    const int32_t* level_offsets; // [levels + 1]
    const int32_t* child_entries; // [J - roots]
    const int32_t* child_offsets; // [J + 1]
    const float* gT;              // [B, J, 16] or nullptr
    const float* gq;              // [B, J, 3] or nullptr
    float* T;                     // [B, J, 16] or nullptr
    float* q;                     // [B, J, 3] or nullptr
    float* gr;                    // d r: rows of gr_row floats, or nullptr
    float* gp;                    // d p likewise
    long long r_stride, p_stride; // floats between two scenes; 0 for an operand shared by the scenes
    long long gr_scene, gp_scene; // floats between two scenes of the gradient rows (scratch: J * 6, an output: J * 3)
    int gr_row, gp_row;           // floats between two joints of the gradient rows (scratch: 6, an output: 3)
    int J, levels;
};

// what the Rodrigues step leaves in a lane's registers
struct Rodrigues {
    float v[3], k[3], n, c, s;
    float R[9];                   // R[3 a + b] = R[a][b], indexed [in, out]
};

// matrices.rodrigues, operation for operation
__device__ __forceinline__ void rodrigues(const float (&r)[3], Rodrigues& o)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) o.v[a] = r[a] + 1.e-12f;
    o.n = sqrtf((o.v[0] * o.v[0] + o.v[1] * o.v[1]) + o.v[2] * o.v[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) o.k[a] = o.v[a] / o.n;
    o.c = cosf(o.n);
    o.s = sinf(o.n);
    const float m = 1.f - o.c;
    const float K[9] = {0.f, -o.k[2], o.k[1], o.k[2], 0.f, -o.k[0], -o.k[1], o.k[0], 0.f};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float kk = (m * o.k[a]) * o.k[b];
            o.R[3 * a + b] = a == b ? o.c + kk : kk + o.s * K[3 * a + b];
        }
    }
}

// d loss / d r from d loss / d R: the chain of matrices.rodrigues backwards, as autograd walks it
__device__ __forceinline__ void rodrigues_backward(const Rodrigues& o, const float (&dR)[9], float (&dr)[3])
{
    const float m = 1.f - o.c;
    float dk[3], dm = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float u = 0.f;   // sum over b of (d R[a][b] + d R[b][a]) k[b]
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            u += (dR[3 * a + b] + dR[3 * b + a]) * o.k[b];
            dm += dR[3 * a + b] * (o.k[a] * o.k[b]);
        }
        dk[a] = m * u;
    }
    const float w[3] = {dR[7] - dR[5], dR[2] - dR[6], dR[3] - dR[1]};   // d (s K) / d k: K[1][2] = -k0, K[2][1] = k0, ...
    const float ds = dot3(w, o.k);
#pragma unroll
    for (int a = 0; a < 3; ++a) dk[a] += o.s * w[a];
    const float dc = ((dR[0] + dR[4]) + dR[8]) - dm;
    // k = v / n: d v = d k / n, d n = -sum (d k * (v / n) / n); c = cos n, s = sin n; n = |v|: d v += d n * v / n
    float dn = ds * o.c - dc * o.s;
    dn -= ((dk[0] * o.k[0] + dk[1] * o.k[1]) + dk[2] * o.k[2]) / o.n;
#pragma unroll
    for (int a = 0; a < 3; ++a) dr[a] = dk[a] / o.n + dn * (o.v[a] / o.n);
}

__device__ __forceinline__ void lds_block(const float* s, int j, float (&t)[KN_ROW])
{
    const float4* p = reinterpret_cast<const float4*>(s + j * KN_ROW);   // 48-byte blocks of a 16-byte aligned array
    const float4 a = p[0], b = p[1], c = p[2];
    t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
    t[8] = c.x; t[9] = c.y; t[10] = c.z; t[11] = c.w;
}

__device__ __forceinline__ void lds_store_block(float* s, int j, const float (&t)[KN_ROW])
{
    float4* p = reinterpret_cast<float4*>(s + j * KN_ROW);
    p[0] = make_float4(t[0], t[1], t[2], t[3]);
    p[1] = make_float4(t[4], t[5], t[6], t[7]);
    p[2] = make_float4(t[8], t[9], t[10], t[11]);
}

// what a lane keeps of its joint from the forward walk
struct Joint {
    int j, parent, level;
    float p[3], tl[3];
    float S[KN_ROW];              // S3 row-major, then t
    Rodrigues rod;
};

// The forward walk of one scene: lane i < J owns joint order[i]; on return s_S holds every joint's block, the workgroup has
// synchronised, and `me` holds the lane's own joint.  s_lo: the level offsets, staged here.
template <int BLOCK>
__device__ __forceinline__ void kinematics_walk(const KinParams& P, int b, float* s_S, int* s_lo, Joint& me)
{
    const int tid = threadIdx.x;
    const bool live = tid < P.J;
    for (int i = tid; i <= P.levels; i += BLOCK) s_lo[i] = P.level_offsets[i];
    me.j = live ? P.order[tid] : 0;
    me.parent = live ? P.parents[me.j] : -1;
    float r[3];
    load3(P.r + (size_t)b * P.r_stride + (size_t)me.j * 3, r);
    load3(P.p + (size_t)b * P.p_stride + (size_t)me.j * 3, me.p);
    rodrigues(r, me.rod);
    const float (&R)[9] = me.rod.R;
#pragma unroll
    for (int c = 0; c < 3; ++c) me.tl[c] = me.p[c] - ((me.p[0] * R[c] + me.p[1] * R[3 + c]) + me.p[2] * R[6 + c]);
    __syncthreads();
    // the lane's level: the number of level starts at or before its position
    me.level = 0;
    for (int d = 1; d < P.levels; ++d) me.level += tid >= s_lo[d] ? 1 : 0;
    if (!live) me.level = -1;
    for (int d = 0; d < P.levels; ++d) {   // (uniform)
        if (d == me.level) {
            if (me.parent < 0) {
#pragma unroll
                for (int q = 0; q < 9; ++q) me.S[q] = R[q];
#pragma unroll
                for (int c = 0; c < 3; ++c) me.S[9 + c] = me.tl[c];
            } else {
                float Sp[KN_ROW];
                lds_block(s_S, me.parent, Sp);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) me.S[3 * a + c] = (R[3 * a] * Sp[c] + R[3 * a + 1] * Sp[3 + c]) + R[3 * a + 2] * Sp[6 + c];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) me.S[9 + c] = ((me.tl[0] * Sp[c] + me.tl[1] * Sp[3 + c]) + me.tl[2] * Sp[6 + c]) + Sp[9 + c];
            }
            lds_store_block(s_S, me.j, me.S);
        }
        __syncthreads();
    }
}

// ---- forward: a workgroup per scene
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void kinematics_forward_kernel(KinParams P)
{
    __shared__ __attribute__((aligned(16))) float s_S[BLOCK * KN_ROW];
    __shared__ int s_lo[BLOCK + 1];
    const int b = blockIdx.x;
    Joint me;
    kinematics_walk<BLOCK>(P, b, s_S, s_lo, me);
    if ((int)threadIdx.x >= P.J) return;
    const size_t row = (size_t)b * P.J + me.j;
    if (P.T) {
        Float4* o = reinterpret_cast<Float4*>(P.T + row * 16);
        o[0] = Float4{me.S[0], me.S[1], me.S[2], 0.f};
        o[1] = Float4{me.S[3], me.S[4], me.S[5], 0.f};
        o[2] = Float4{me.S[6], me.S[7], me.S[8], 0.f};
        o[3] = Float4{me.S[9], me.S[10], me.S[11], 1.f};
    }
    if (P.q) {
        float y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) y[c] = ((me.p[0] * me.S[c] + me.p[1] * me.S[3 + c]) + me.p[2] * me.S[6 + c]) + me.S[9 + c];
        store3(P.q + row * 3, y);
    }
}

// ---- backward: a workgroup per scene
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void kinematics_backward_kernel(KinParams P)
{
    __shared__ __attribute__((aligned(16))) float s_S[BLOCK * KN_ROW];
    __shared__ int s_lo[BLOCK + 1];
    __shared__ int s_child[BLOCK];
    const int tid = threadIdx.x, b = blockIdx.x;
    const bool live = tid < P.J;
    const int children = P.child_offsets[P.J];
    for (int i = tid; i < children; i += BLOCK) s_child[i] = P.child_entries[i];
    Joint me;
    kinematics_walk<BLOCK>(P, b, s_S, s_lo, me);   // (its barriers order s_child too)
    const int c0 = live ? P.child_offsets[me.j] : 0, c1 = live ? P.child_offsets[me.j + 1] : 0;
    // the seed: G = (GS row-major, Gt), and d p = S3 @ gq
    const size_t row = (size_t)b * P.J + me.j;
    float G[KN_ROW], dp[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < KN_ROW; ++q) G[q] = 0.f;
    if (live && P.gT) {
        const Float4* g = reinterpret_cast<const Float4*>(P.gT + row * 16);
        const Float4 g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
        G[0] = g0.x; G[1] = g0.y; G[2] = g0.z; G[3] = g1.x; G[4] = g1.y; G[5] = g1.z;
        G[6] = g2.x; G[7] = g2.y; G[8] = g2.z; G[9] = g3.x; G[10] = g3.y; G[11] = g3.z;
    }
    if (live && P.gq) {
        float gq[3];
        load3(P.gq + row * 3, gq);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = 0; c < 3; ++c) G[3 * a + c] += me.p[a] * gq[c];
            G[9 + a] += gq[a];
            dp[a] = (me.S[3 * a] * gq[0] + me.S[3 * a + 1] * gq[1]) + me.S[3 * a + 2] * gq[2];
        }
    }
    const float (&R)[9] = me.rod.R;
    float dR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dtl[3] = {0.f, 0.f, 0.f};
    for (int d = P.levels - 1; d >= 0; --d) {   // (uniform)
        if (d == me.level) {
            for (int e = c0; e < c1; ++e) {   // the blocks the children left, in index order
                float C[KN_ROW];
                lds_block(s_S, s_child[e], C);
#pragma unroll
                for (int q = 0; q < KN_ROW; ++q) G[q] += C[q];
            }
            if (me.parent < 0) {
#pragma unroll
                for (int q = 0; q < 9; ++q) dR[q] = G[q];
#pragma unroll
                for (int c = 0; c < 3; ++c) dtl[c] = G[9 + c];
            } else {
                float Sp[KN_ROW], C[KN_ROW];
                lds_block(s_S, me.parent, Sp);   // (the parent, a level down, has not yet replaced its block)
#pragma unroll
                for (int x = 0; x < 4; ++x) {    // rows of GS, then Gt, times S3[parent]^T
#pragma unroll
                    for (int y = 0; y < 3; ++y) {
                        const float t = (G[3 * x] * Sp[3 * y] + G[3 * x + 1] * Sp[3 * y + 1]) + G[3 * x + 2] * Sp[3 * y + 2];
                        if (x < 3) dR[3 * x + y] = t;
                        else dtl[y] = t;
                    }
                }
#pragma unroll
                for (int y = 0; y < 3; ++y) {    // the block for the parent: R^T @ GS + outer(tl, Gt), and Gt
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        C[3 * y + c] = ((R[y] * G[c] + R[3 + y] * G[3 + c]) + R[6 + y] * G[6 + c]) + me.tl[y] * G[9 + c];
                    C[9 + y] = G[9 + y];
                }
                lds_store_block(s_S, me.j, C);   // (every child of this joint has read its S3 / t a level up)
            }
        }
        __syncthreads();
    }
    if (!live) return;
    if (P.gp) {
        float o[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = (dp[a] + dtl[a]) - ((R[3 * a] * dtl[0] + R[3 * a + 1] * dtl[1]) + R[3 * a + 2] * dtl[2]);
        store3(P.gp + (size_t)b * P.gp_scene + (size_t)me.j * P.gp_row, o);
    }
    if (P.gr) {
        float o[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = 0; c < 3; ++c) dR[3 * a + c] -= me.p[a] * dtl[c];
        }
        rodrigues_backward(me.rod, dR, o);
        store3(P.gr + (size_t)b * P.gr_scene + (size_t)me.j * P.gr_row, o);
    }
}

// ---- the gradient of an operand shared by the scenes: workgroup j adds the rows (scene, j) of `partial` [B, J, 6] in a
// fixed order -- lane 6 s + q sums rows s, s + 42, ... of column q, so a wave reads whole rows, then lane q folds the 42
// slots in slot order (up to 42 scenes that is scene order) -- and writes d r[j] (columns 0-2) and / or d p[j] (3-5).
// The shape of skin_bone_reduce_kernel: six totals per workgroup from rows of six; block_column_sum gives one total per
// workgroup and log2(256) barriers for each.
__global__ __launch_bounds__(KN_REDUCE_BLOCK) void kinematics_reduce_kernel(const float* __restrict__ partial, float* __restrict__ gr,
                                                                            float* __restrict__ gp, int B, int J)
{
    __shared__ float s_sum[KN_SLOTS * KN_COLS];
    const int tid = threadIdx.x, j = blockIdx.x;
    if (tid < KN_SLOTS * KN_COLS) {
        const int slot = tid / KN_COLS, q = tid - KN_COLS * slot;
        float s = 0.f;
        if (q < 3 ? gr != nullptr : gp != nullptr) {
            for (int b = slot; b < B; b += KN_SLOTS) s += partial[((size_t)b * J + j) * KN_COLS + q];
        }
        s_sum[tid] = s;
    }
    __syncthreads();
    if (tid < KN_COLS) {
        float* out = tid < 3 ? gr : gp;
        if (out) {
            float t = 0.f;
            for (int slot = 0; slot < KN_SLOTS; ++slot) t += s_sum[slot * KN_COLS + tid];
            out[(size_t)j * 3 + (tid < 3 ? tid : tid - 3)] = t;
        }
    }
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

static int kinematics_check(const char* who, const float* rotations, int rotation_scenes, const float* joints, int joint_scenes,
                            const int32_t* parents, const int32_t* order, const int32_t* level_offsets, int levels, long long B, int J,
                            unsigned flags, dirt::KinParams& P)
{
    if (B < 0 || J < 0) STAGE_FAIL("%s: negative sizes (B=%lld J=%d)", who, B, J);
    if (B > 65535 || J > DIRT_KINEMATICS_MAX_JOINTS) STAGE_FAIL("%s: B=%lld J=%d, at most 65535 scenes and %d joints", who, B, J, DIRT_KINEMATICS_MAX_JOINTS);
    if (rotation_scenes != 1 && rotation_scenes != B) STAGE_FAIL("%s: rotation_scenes=%d is neither 1 nor B=%lld", who, rotation_scenes, B);
    if (joint_scenes != 1 && joint_scenes != B) STAGE_FAIL("%s: joint_scenes=%d is neither 1 nor B=%lld", who, joint_scenes, B);
    if (flags) STAGE_FAIL("%s: unknown flags 0x%x", who, flags);
    if (B == 0 || J == 0) return DIRT_OK;
    if (levels < 1 || levels > J) STAGE_FAIL("%s: levels=%d, 1 to J=%d", who, levels, J);
    if (!rotations || !joints || !parents || !order || !level_offsets) STAGE_FAIL("%s: rotations / joints / parents / order / level_offsets is NULL", who);
    P.r = rotations; P.p = joints; P.parents = parents; P.order = order; P.level_offsets = level_offsets;
    P.J = J; P.levels = levels;
    P.r_stride = rotation_scenes == 1 ? 0 : (long long)J * 3;
    P.p_stride = joint_scenes == 1 ? 0 : (long long)J * 3;
    return DIRT_OK;
}

// kernel<BLOCK> for this J
#define KINEMATICS_LAUNCH(kernel, B, s, P)                                                                                         \
    do {                                                                                                                           \
        if ((P).J <= 64) hipLaunchKernelGGL((dirt::kernel<DIRT_KINEMATICS_SMALL_BLOCK>), dim3((unsigned)(B)), dim3(DIRT_KINEMATICS_SMALL_BLOCK), 0, s, P); \
        else hipLaunchKernelGGL((dirt::kernel<256>), dim3((unsigned)(B)), dim3(256), 0, s, P);                                     \
    } while (0)

size_t dirt_kinematics_scratch_bytes(long long B, long long J)
{
    if (B < 0 || B > 65535 || J < 0 || J > DIRT_KINEMATICS_MAX_JOINTS) return 0;
    return sizeof(float) * dirt::KN_COLS * (size_t)B * (size_t)J;
}

int dirt_kinematics_forward(const float* rotations, int rotation_scenes, const float* joints, int joint_scenes, const int32_t* parents,
                            const int32_t* order, const int32_t* level_offsets, int levels, float* transforms, float* posed_joints, long long B,
                            int J, unsigned flags, void* stream)
{
    const char* who = "dirt_kinematics_forward";
    dirt::KinParams P{};
    int rc = kinematics_check(who, rotations, rotation_scenes, joints, joint_scenes, parents, order, level_offsets, levels, B, J, flags, P);
    if (rc) return rc;
    if (B == 0 || J == 0 || (!transforms && !posed_joints)) return dirt::stage_ok(report);
    P.T = transforms; P.q = posed_joints;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KINEMATICS_LAUNCH(kinematics_forward_kernel, B, s, P);
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_kinematics_backward(const float* rotations, int rotation_scenes, const float* joints, int joint_scenes, const int32_t* parents,
                             const int32_t* order, const int32_t* level_offsets, int levels, const int32_t* child_entries,
                             const int32_t* child_offsets, const float* grad_transforms, const float* grad_posed_joints, float* grad_rotations,
                             float* grad_joints, void* scratch, size_t scratch_bytes, long long B, int J, unsigned flags, void* stream)
{
    const char* who = "dirt_kinematics_backward";
    dirt::KinParams P{};
    int rc = kinematics_check(who, rotations, rotation_scenes, joints, joint_scenes, parents, order, level_offsets, levels, B, J, flags, P);
    if (rc) return rc;
    if (B == 0 || J == 0 || (!grad_rotations && !grad_joints)) return dirt::stage_ok(report);
    if (!child_offsets || (levels > 1 && !child_entries)) STAGE_FAIL("%s: child_entries / child_offsets is NULL", who);
    // an operand shared by B > 1 scenes: its per-scene rows go to scratch and a second launch adds them
    const bool sum_r = grad_rotations && rotation_scenes == 1 && B > 1, sum_p = grad_joints && joint_scenes == 1 && B > 1;
    float* partial = nullptr;
    if (sum_r || sum_p) {
        rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_kinematics_scratch_bytes(B, J), "dirt_kinematics_scratch_bytes");
        if (rc) return rc;
        partial = static_cast<float*>(scratch);
    }
    P.child_entries = child_entries; P.child_offsets = child_offsets;
    P.gT = grad_transforms; P.gq = grad_posed_joints;
    const long long row = dirt::KN_COLS;
    P.gr = sum_r ? partial : grad_rotations;
    P.gr_row = sum_r ? (int)row : 3;
    P.gr_scene = (long long)J * P.gr_row;
    P.gp = sum_p ? partial + 3 : grad_joints;
    P.gp_row = sum_p ? (int)row : 3;
    P.gp_scene = (long long)J * P.gp_row;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KINEMATICS_LAUNCH(kinematics_backward_kernel, B, s, P);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && partial) {
        hipLaunchKernelGGL(dirt::kinematics_reduce_kernel, dim3((unsigned)J), dim3(dirt::KN_REDUCE_BLOCK), 0, s, partial,
                           sum_r ? grad_rotations : nullptr, sum_p ? grad_joints : nullptr, (int)B, J);
        e = hipGetLastError();
    }
    return dirt::stage_hip(report, who, e);
}

}  // extern "C"
