// dirt_grad_common.h -- steps of the gradient pass (assemble_grads, csrc/rasterise_grad_egl.cu:93-236) that its three kernels
// share, each written and explained once here:
//   grad_kernel      (dirt_grad.hip):       4 pixels per lane, 32 x 32 tiles;
//   grad_kernel_px2  (dirt_grad_px2.hip):   2 pixels per lane, 32 x 16 tiles;
//   grad_kernel_px1  (dirt_grad_small.hip): 1 pixel per lane, 16 x 16 tiles for small frames (the scalar steps only).
// Shared: the Scharr stencils (scalar: px1 and both Q1 border fix-ups; packed pair: grad_kernel, px2), the layout of a face's
// values, a pixel's non-finite test, the row minimum / maximum and the joins of a pair of rows, the atomic tail of a
// face-loop iteration, the trace macros, write_debug, ndc_of.  NOT shared yet -- written out in both grad_kernel and
// grad_kernel_px2, to be changed in both: the dilation and its attempt order, the ring-cell gather, the lane roles and
// the atomics of a non-finite pixel.
#pragma once
#include "dirt_device.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dirt {

// ---- per-wave phase timestamps (s_memtime) for tools/trace_grad.py and tools/trace_px2.py.  Only the tracing build of the
//      library defines DIRT_TRACE (tools/build_tools.sh); the product library (dirt_amd/build.py) never does.  A kernel names
//      its buffer once (GRAD_TRACE_BUFFER(_px2): g_trace_grad_px2 and its setter dirt_debug_set_trace_grad_px2), opens with
//      GRAD_TRACE_BEGIN(), marks its phases with GMARK(), counts with GCOUNT() and closes with GRAD_TRACE_END(_px2):
//      16 values per wave -- 12 timestamps, 2 counters, the wall clock at the start, duration << 20 | HW_ID. ----
#ifdef DIRT_TRACE
#define GRAD_TRACE_BUFFER(SUFFIX)                                                          \
    __device__ long long* g_trace_grad##SUFFIX = nullptr;                                  \
    extern "C" void dirt_debug_set_trace_grad##SUFFIX(void* p)                             \
    {                                                                                      \
        long long* q = reinterpret_cast<long long*>(p);                                    \
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_trace_grad##SUFFIX), &q, sizeof(q));          \
    }
#define GRAD_TRACE_BEGIN() long long tr_t[12]; int tr_n = 0; long long tr_c[4] = {0, 0, 0, 0}; const long long tr_wall0 = wall_clock64()
#define GMARK() do { if (tr_n < 12) { long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); tr_t[tr_n++] = t_; } } while (0)
#define GCOUNT(i, v) do { tr_c[i] += (v); } while (0)
#define GRAD_TRACE_END(SUFFIX) grad_trace_end(g_trace_grad##SUFFIX, tr_t, tr_n, tr_c, tr_wall0)
__device__ __forceinline__ void grad_trace_end(long long* buf, const long long (&tr_t)[12], int tr_n, const long long (&tr_c)[4], long long tr_wall0)
{
    if ((threadIdx.x & 63) == 0 && buf) {
        long long* o = buf + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6)) * 16;
        for (int i = 0; i < 12; ++i) o[i] = i < tr_n ? tr_t[i] : 0;
        o[12] = tr_c[0]; o[13] = tr_c[1];
        o[14] = tr_wall0; o[15] = (((long long)wall_clock64() - tr_wall0) << 20) | (long long)(__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4 /* HW_REG_HW_ID */) & 0xFFFFF);
    }
}
#else
#define GRAD_TRACE_BUFFER(SUFFIX)
#define GRAD_TRACE_BEGIN() do {} while (0)
#define GMARK() do {} while (0)
#define GCOUNT(i, v) do {} while (0)
#define GRAD_TRACE_END(SUFFIX) do {} while (0)
#endif

typedef unsigned long long lanemask;   // one bit per lane of the wave, wave-uniform (a scalar register pair)
typedef float float2v __attribute__((ext_vector_type(2)));   // a register pair for the packed fp32 instructions (v_pk_fma_f32)

// (s, s) * b [+ c] in one packed instruction.  op_sel_hi:[0,1,1] makes both halves take their first factor from the LOW
// register of the first operand's pair, so the scalar needs no copy into a second register (the compiler, given a
// splat, emits a v_mov per use); the pair's high register is never read.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wuninitialized"
__device__ __forceinline__ float2v pk_fma_scalar(float s, float2v b, float2v c)
{
    float2v a;
    a.x = s;
    float2v d;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ float2v pk_mul_scalar(float s, float2v b)
{
    float2v a;
    a.x = s;
    float2v d;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
#pragma clang diagnostic pop

// NDC coordinate of the centre of pixel i of n: (2 i + 1 - n) / n.  The numerator is an exact small integer, so the result carries
// two roundings RELATIVE to its own size -- where ((i + 0.5) * (2 / n)) - 1 has an absolute error of an ulp of 1 whatever the
// value, i.e. no correct digit at the centre of the frame: there the reference's clip_x = sum_k b_k * vertex_k.x (:210-217), which
// this stands for, is small and accurate, and the position gradient's w term differed by up to 27 ulps of that sum's scale
// (round 5 fuzz sweep: two elements in 1 727 cases beyond the tolerance's cancellation term; none since).
__device__ __forceinline__ float ndc_of(int i, int n, float inv_n)
{
    return (float)(2 * i + 1 - n) * inv_n;
}

// ---- Scharr (:126-127), operation for operation: negative-offset minus positive-offset, offset_y is up = the previous tensor
//      row.  The operation order decides, through the L1 norms of :185, the discrete dilation axis. ----
// One "channel" from its 3 x 3 taps w[r][i] = (row y - 1 + r, column x - 1 + i).
__device__ __forceinline__ void scharr(const float (&w)[3][3], float& sx, float& sy)
{
    const float mm = w[2][0], m0 = w[1][0], mp = w[0][0];
    const float zm = w[2][1], zp = w[0][1];
    const float pm = w[2][2], p0 = w[1][2], pp = w[0][2];
    float d1 = ((mm + mp) - pm) - pp;
    float d2 = m0 - p0;
    float m1 = d1 * (3.f / 32.f), m2 = d2 * (10.f / 32.f);
    sx = m1 + m2;
    d1 = ((mm + pm) - mp) - pp;
    d2 = zm - zp;
    m1 = d1 * (3.f / 32.f); m2 = d2 * (10.f / 32.f);
    sy = m1 + m2;
}
// Two adjacent pixels q = 2P, 2P + 1 of a lane with the packed fp32 instructions.  Taps of row r as pairs: T[r][i] = columns
// (xs - 1 + 2i, xs + 2i) of the lane's first pixel xs; at(ox, oy) of pixel q: row 1 - oy, column q + 1 + ox of the taps.
template <int NT>
__device__ __forceinline__ void scharr_pk(const float2v (&T)[3][NT], int P, float2v& sx, float2v& sy)
{
    const float2v mm = T[2][P], m0 = T[1][P], mp = T[0][P];
    const float2v pm = T[2][P + 1], p0 = T[1][P + 1], pp = T[0][P + 1];
    float2v d1 = ((mm + mp) - pm) - pp;
    float2v d2 = m0 - p0;
    float2v m1 = d1 * (3.f / 32.f), m2 = d2 * (10.f / 32.f);
    sx = m1 + m2;
    d1 = ((mm + pm) - mp) - pp;
    // the middle column of each pixel: the high half of one tap pair and the low half of the next
    d2.x = T[2][P].y - T[0][P].y;
    d2.y = T[2][P + 1].x - T[0][P + 1].x;
    m1 = d1 * (3.f / 32.f); m2 = d2 * (10.f / 32.f);
    sy = m1 + m2;
}

// Quirk Q1 at the right image border: for the pixels of a strip (first column xs, row y) flagged in `which`, the
// aliased "channels" 1, 2 of 1-channel group c -- elements (pixel + 1, + 2) of the flattened [B,H,W,1] slice -- lie in
// the NEXT image row (past the end of the tensor they are clamped to its last element; undefined in the reference).
// Their dilation axis (:185) is decided again from memory -- the 5 x 3 window of elements the three Scharr stencils
// cover, requested together -- and replaces bits 0 .. 3 of `bits`.  Rare (the last two interior columns of a
// frame): a rolled loop behind a wave-uniform branch.  (grad_kernel_px2 has a loop shape of its own over the same scharr(),
// alias_wrap_fixup_rolled, for its register count.)
__device__ __forceinline__ uint32_t alias_wrap_fixup(const float* __restrict__ pixels, int B, int H, int W, int C, int iib, int y,
                                                  int xs, int c, uint32_t which, uint32_t bits)
{
    const size_t last = (size_t)B * H * W - 1;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        if (!((which >> j) & 1u)) continue;
        // w5[r][i]: element (centre + i - 1) of row y - 1 + r in flat order; the taps of "channel" ch start at column ch
        float w5[3][5];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const size_t base = ((size_t)iib * H + (y - 1 + r)) * W + xs + j - 1;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                size_t m = base + i;
                if (m > last) m = last;
                w5[r][i] = pixels[m * C + c];
            }
        }
        float w[3][3], sx, sy, l1x = 0.f, l1y = 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int i = 0; i < 3; ++i) w[r][i] = w5[r][ch + i];
            scharr(w, sx, sy);
            l1x = ch == 0 ? fabsf(sx) : l1x + fabsf(sx);
            l1y = ch == 0 ? fabsf(sy) : l1y + fabsf(sy);
        }
        bits = (bits & ~(1u << j)) | ((l1x > l1y) ? (1u << j) : 0u);
    }
    return bits;
}

// The reference's diagnostic output (csrc/rasterise_grad_egl.cu:150-151,172) of one pixel, for the first channel group
// (G channels starting at channel 0): [0] = 1e-2 where dilation fired, [1], [2] = elements (pix * G + 1, + 2) of the
// contiguous [B,H,W,G] slice of grad_pixels, clamped to its end.  Optional: only in the DEBUG instantiations.
__device__ __forceinline__ void write_debug(float* __restrict__ debug_thingy, const float* __restrict__ grad_pixels, int B, int H, int W,
                                        int C, int iib, int y, int x, int G, bool dilated)
{
    const size_t total_pix = (size_t)B * H * W;
    const size_t pix = ((size_t)iib * H + y) * W + x;
    float* dbg = debug_thingy + pix * 3;
    dbg[0] = dilated ? 1.e-2f : 0.f;
    for (int ch = 1; ch <= 2; ++ch) {
        size_t mp = G == 3 ? pix : pix + ch;      // pixel of that element
        int mc = G == 3 ? ch : 0;                 // channel inside the group
        if (mp > total_pix - 1) { mp = total_pix - 1; mc = G - 1; }
        dbg[ch] = grad_pixels[mp * C + mc];
    }
}

// ---- the values of a face in the face loop of the packed kernels: per vertex k the S values b_k * (g_0 .. g_NCH-1, fx, fy, fw)
//      (S = 3 + NCH rounded up to even), as HP = S / 2 packed pairs -- one v_pk_fma_f32 per pair and pixel; the NV = 3 S sums are
//      padded to the NR values the row reduction takes (row_reduce_scatter, dirt_reduce.h).  Order of a vertex's values: the
//      colours first (they arrive as whole registers of the grad_pixels loads), then the position factors with (fx, fy) as one
//      aligned pair: NCH even: g.., fx, fy, fw, 0;  odd: g.., fw, fx, fy.
//      FWS (grad_kernel's {3,3} shape with the aliased inbox): an even channel count leaves the w factor alone in its pair, and
//      the padding costs a register per pixel and per vertex sum.  There fw travels as a SCALAR next to the pairs (one
//      v_fma_f32 instead of one v_pk_fma_f32 per pixel and vertex: the same instruction count) and its three sums follow the
//      vertices' blocks in the reduction's input -- g.., fx, fy per vertex, then fw of the three vertices; IW = S marks "not in
//      the pairs": 9 registers less in a loop that has to fit 128. ----
template <int NCH_, bool FWS_ = false>
struct FaceValues {
    static constexpr int NCH = NCH_;
    static constexpr bool FWS = FWS_;
    static constexpr int S = FWS ? NCH + 2 : (3 + NCH + 1) & ~1;   // values per vertex held in pairs
    static constexpr int HP = S / 2;                                // ... as pairs
    static constexpr int NV = FWS ? 3 * S + 3 : 3 * S;              // values per face
    static constexpr int NR = NV <= 16 ? 16 : (NV <= 24 ? 24 : 32); // ... padded to what the row reduction takes
    static constexpr int IW = FWS ? S : ((NCH & 1) ? NCH : NCH + 2), IX = (NCH & 1) ? NCH + 1 : NCH, IY = IX + 1;
    static_assert(NV <= NR && (IX & 1) == 0 && IY < S && (FWS || IW < S), "");
};
// ---- non-finite factors (a NaN / Inf in grad_pixels, in `pixels` through the Scharr filter, a degenerate clip_w).  The face
//      loop multiplies every pixel's factors by a barycentric that is ZEROED where the pixel is not of the face at hand:
//      0 * NaN would carry one pixel's NaN into every face of the pixels reduced with it, where the reference adds a pixel's
//      terms to the vertices of its own face only (:140,228-230).  Such a pixel (rare; a sum of finite factors that overflows
//      is treated alike) adds its 3 (NCH + 3) products itself -- the reference's own atomics, term for term -- and leaves the
//      loop: the kernel zeroes its factors and strikes its face off.  (grad_kernel_px1 selects products instead.) ----
// fp: the pixel's factors in pairs, fpw: its w factor under FWS, bk: its barycentrics.
template <class L>
__device__ __forceinline__ bool pixel_nonfinite(const float2v (&fp)[L::HP], float fpw, const float (&bk)[3])
{
    float2v t = fp[0];
#pragma unroll
    for (int h = 1; h < L::HP; ++h) t += fp[h];
    if (L::FWS) t.x += fpw;
    const float u = (t.x + t.y) + ((bk[0] + bk[1]) + bk[2]);   // non-finite iff a factor is, or the sum overflows
    return !__builtin_isfinite(u);
}
// ---- across a DPP row of 16 lanes: the all-lanes minimum / maximum by four rotations; row_pair_*: joined with the other row
//      of a pair (rows 0, 1 and rows 2, 3) through v_permlane16_swap -- both rows get the result. ----
#define DIRT_ROW_ALL(OP, K)                                                                                   \
    K = OP(K, (uint32_t)__builtin_amdgcn_mov_dpp((int)K, 0x128 /* row_ror:8 */, 0xF, 0xF, true));           \
    K = OP(K, (uint32_t)__builtin_amdgcn_mov_dpp((int)K, 0x124 /* row_ror:4 */, 0xF, 0xF, true));           \
    K = OP(K, (uint32_t)__builtin_amdgcn_mov_dpp((int)K, 0x122 /* row_ror:2 */, 0xF, 0xF, true));           \
    K = OP(K, (uint32_t)__builtin_amdgcn_mov_dpp((int)K, 0x121 /* row_ror:1 */, 0xF, 0xF, true))
__device__ __forceinline__ uint32_t row_min(uint32_t K) { DIRT_ROW_ALL(min, K); return K; }
__device__ __forceinline__ uint32_t row_max(uint32_t K) { DIRT_ROW_ALL(max, K); return K; }
#undef DIRT_ROW_ALL
__device__ __forceinline__ uint32_t row_pair_min(uint32_t K)
{
    const auto sw = __builtin_amdgcn_permlane16_swap(K, K, false, false);
    return min(sw[0], sw[1]);
}
__device__ __forceinline__ float row_pair_sum(float d)
{
    const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(d), __float_as_uint(d), false, false);
    return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}

// ---- the tail of a face-loop iteration: the lane adds its total to the vertex (index vsel, loaded at the head of the
//      iteration) of its role.  The address is formed BEFORE the branch on `total != 0` on purpose: the wait for the vertex
//      index then sits on every path.  Inside the branch it would leave the load pending on the path around it, and the
//      compiler answers that with s_waitcnt vmcnt(0) in the loop header -- where it also waits, every iteration, for the
//      previous iteration's atomic to be acknowledged by the memory system (+3 us at K3, +11 us at K3-256).  The add is
//      written as a GLOBAL atomic: behind the asm barrier that pins the address the compiler no longer knows the pointer's
//      address space and emits flat_atomic_add_f32, which is issued to the LDS and the memory pipeline alike and counts on
//      both wait counters. ----
__device__ __forceinline__ float* pinned_vertex_address(float* base, int vsel, uint32_t stride)
{
    float* dst = reinterpret_cast<float*>(reinterpret_cast<char*>(base) + (size_t)((uint32_t)vsel * stride));
    asm volatile("" : "+v"(dst));
    return dst;
}
__device__ __forceinline__ void global_add(float* dst, float v)
{
    asm volatile("global_atomic_add_f32 %0, %1, off" : : "v"(dst), "v"(v) : "memory");
}

}  // namespace dirt
