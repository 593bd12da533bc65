// dirt_resolve.hip -- the last stage of the renderer, fused: supersample resolve, exposure, tone curve, sRGB encode, clamp;
// one pass forward, one backward (plus the fixed-order sum of the exposure's and the white point's gradients).
//
// The specification (DESIGN.md §7j restates it; dirt_amd/lighting.py::resolve_image is its readable form, which
// tests/resolve_reference.py restates in float64), per output pixel (r, c) and channel ch of a rows x cols image resolved from
// S rows x S cols samples, in float32 and in this order:
//
//     acc = 0;  for i in 0..S-1, for j in 0..S-1:  acc += image[S r + i, S c + j, ch] (+ add[...])        L = acc * float(1 / S^2)
//     E = exposure[ch] * L
//     DIRT_RESOLVE_LINEAR:    t = E
//     otherwise x = max0(E), and
//     DIRT_RESOLVE_REINHARD:  t = x * (1 + x / (w * w)) / (1 + x)                       (w: the white point)
//     DIRT_RESOLVE_ACES:      t = x * (2.51 x + 0.03) / (x * (2.43 x + 0.59) + 0.14)
//     DIRT_RESOLVE_ENCODE_LINEAR: y = t
//     DIRT_RESOLVE_ENCODE_SRGB:   u = max0(t);  y = 12.92 u where u <= 0.0031308, else 1.055 powf(u, 1 / 2.4) - 0.055
//     out = clamp(y, lo, hi) with DIRT_RESOLVE_CLAMP
//
// max0 and the clamp are those of dirt_shade_common.h: a NaN stays NaN; their gradients pass at the edge (x >= 0; lo <= y <= hi).
//
// Kernels: resolve_forward_kernel<S>, resolve_backward_kernel<S>.  A workgroup of RS_BLOCK lanes owns one stretch of an output
// row: RS_SPAN output pixels (RS_SPAN_FINE with S >= 3, which keeps the LDS tile at 32 KB), that is S stretches of S * span
// samples, each contiguous in its input row.
//   forward:  the workgroup walks each of those stretches float after float, lane after lane (16, 8 or 4 bytes a lane: what
//             the pointers and the row lengths allow; 4 bytes also where a sample's channels are part of a wider pixel), adds
//             `add`, and leaves the S stretches in LDS; then a lane takes consecutive floats of the OUTPUT row, sums its S x S
//             samples from LDS in the written order, develops the value and stores it (and L, the resolved linear value, when
//             a backward pass will want it: the only tensor that pass reads beside grad_out).
//   backward: a lane takes consecutive floats of grad_out and L, evaluates d y / d L * g / S^2 into LDS and its terms of the
//             exposure's and the white point's sums; then the workgroup walks the S stretches of grad_image (and grad_add) as
//             the forward walked the inputs, each float taking its output pixel's value from LDS.  The sums leave through
//             wave_sum and fold_waves_to_row as one row per workgroup in caller-owned scratch, and shade_launch_reduce adds
//             the rows in a fixed order: no atomics, the same bits on every run.
// The curve, the encoding and the vector widths are wave-uniform branches, not template arguments: the kernels are bound by
// their memory traffic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dirt_shade_common.h"

namespace dirt {

constexpr int RS_BLOCK = 256;        // lanes of a workgroup
constexpr int RS_SPAN = 256;         // output pixels of a workgroup with S <= 2
constexpr int RS_SPAN_FINE = 128;    // ... with S >= 3
constexpr int RS_MAX_C = DIRT_RESOLVE_MAX_CHANNELS;

constexpr int resolve_span(int S) { return S <= 2 ? RS_SPAN : RS_SPAN_FINE; }

struct ResolveParams {
    const float *img, *add;          // forward: a sample's C floats, istride / astride apart
    const float *expo, *white;       // [1 or scenes, C], [1 or scenes]
    const float *lin_in, *gout;      // backward: L and grad_out, [scenes, rows, cols, C]
    float *out, *lin;                // forward: [scenes, rows, cols, C]; lin may be nullptr
    float *gimg, *gadd;              // backward: [scenes, S rows, S cols, C] or nullptr
    float *part_e, *part_w;          // backward: [scenes, blocks, C], [scenes, blocks, 1] or nullptr
    long long img_scene, add_scene;  // floats between two scenes' images (0: one for all)
    int rows, cols, C, chunks;       // the output image; workgroups of a row
    int istride, astride, estride, wstride;
    int vec, ovec;                   // floats of a lane's access to the sample rows / to the output rows: 4, 2 or 1
    unsigned div_c;                  // e / C = (e * div_c) >> 16 for e < 2^13
    int curve, encode, clamp;
    float lo, hi, inv;
};

template <int V> struct alignas(4 * V) FloatV { float v[V]; };   // V consecutive floats, 4 V-byte aligned: one access

// what a value goes through between L and the clamp
struct ResolveEval { float E, x, t, u, y; };

__device__ __forceinline__ void resolve_develop(const ResolveParams& P, float ex, float w, float L, ResolveEval& d)
{
    d.E = ex * L;
    d.x = d.E; d.t = d.E;
    if (P.curve != DIRT_RESOLVE_LINEAR) {   // (uniform)
        const float x = max0(d.E);
        d.x = x;
        if (P.curve == DIRT_RESOLVE_REINHARD) d.t = x * (1.f + x / (w * w)) / (1.f + x);
        else d.t = x * (2.51f * x + 0.03f) / (x * (2.43f * x + 0.59f) + 0.14f);
    }
    d.u = d.t; d.y = d.t;
    if (P.encode == DIRT_RESOLVE_ENCODE_SRGB) {   // (uniform)
        const float u = max0(d.t);
        d.u = u;
        d.y = u <= 0.0031308f ? 12.92f * u : 1.055f * powf(u, 1.f / 2.4f) - 0.055f;
    }
}

// g = d loss / d out  ->  d loss / d E and d loss / d w
__device__ __forceinline__ void resolve_develop_backward(const ResolveParams& P, float w, const ResolveEval& d, float g, float& gE, float& gw)
{
    float gt = clamp_gate(P, d.y, g);
    if (P.encode == DIRT_RESOLVE_ENCODE_SRGB) {   // (uniform)
        const float slope = d.u <= 0.0031308f ? 12.92f : (1.055f / 2.4f) * powf(d.u, 1.f / 2.4f - 1.f);
        gt = d.t >= 0.f ? gt * slope : 0.f;
    }
    gw = 0.f;
    float gx = gt;
    if (P.curve == DIRT_RESOLVE_REINHARD) {
        const float x = d.x, ww = w * w, b = 1.f + x, a = x * (1.f + x / ww);
        gx = gt * (((1.f + (x + x) / ww) * b - a) / (b * b));
        gw = gt * (-2.f * (x * x) / (ww * w * b));
    } else if (P.curve == DIRT_RESOLVE_ACES) {
        const float x = d.x, n = x * (2.51f * x + 0.03f), q = x * (2.43f * x + 0.59f) + 0.14f;
        gx = gt * (((5.02f * x + 0.03f) * q - n * (4.86f * x + 0.59f)) / (q * q));
    }
    gE = P.curve == DIRT_RESOLVE_LINEAR || d.E >= 0.f ? gx : 0.f;
}

// where a workgroup works: output row r, its pixels c0 .. c0 + npx - 1; sample (S r + i, S c0) of the scene is sample s0 + i SW
template <int S>
__device__ __forceinline__ void resolve_place(const ResolveParams& P, int& r, int& c0, int& npx, long long& s0, long long& SW, long long& obase)
{
    constexpr int SPAN = resolve_span(S);
    r = (int)(blockIdx.x / (unsigned)P.chunks);
    c0 = (int)(blockIdx.x - (unsigned)r * (unsigned)P.chunks) * SPAN;
    npx = P.cols - c0 < SPAN ? P.cols - c0 : SPAN;
    SW = (long long)S * P.cols;
    s0 = (long long)S * r * SW + (long long)S * c0;
    obase = (((long long)blockIdx.y * P.rows + r) * P.cols + c0) * P.C;
}

// ---- forward, first half: the S stretches of samples (image + add) into LDS, V floats a lane
template <int S, int V>
__device__ __forceinline__ void resolve_stage(const ResolveParams& P, const float* __restrict__ img, const float* __restrict__ add,
                                              long long s0, long long SW, int total, int pitch, int tid, float* s_in)
{
    const int C = P.C;
    for (int e = tid * V; e < total; e += RS_BLOCK * V) {
        FloatV<V> a[S];
        if constexpr (V > 1) {   // (the samples' channels are the whole pixel: a stretch is `total` consecutive floats)
#pragma unroll
            for (int i = 0; i < S; ++i) a[i] = *reinterpret_cast<const FloatV<V>*>(img + (s0 + i * SW) * C + e);
            if (add) {   // (uniform)
                FloatV<V> b[S];
#pragma unroll
                for (int i = 0; i < S; ++i) b[i] = *reinterpret_cast<const FloatV<V>*>(add + (s0 + i * SW) * C + e);
#pragma unroll
                for (int i = 0; i < S; ++i)
#pragma unroll
                    for (int k = 0; k < V; ++k) a[i].v[k] = a[i].v[k] + b[i].v[k];
            }
        } else {
            const int q = (int)(((unsigned)e * P.div_c) >> 16), ch = e - q * C;
#pragma unroll
            for (int i = 0; i < S; ++i) a[i].v[0] = img[(s0 + i * SW + q) * P.istride + ch];
            if (add) {   // (uniform)
                float b[S];
#pragma unroll
                for (int i = 0; i < S; ++i) b[i] = add[(s0 + i * SW + q) * P.astride + ch];
#pragma unroll
                for (int i = 0; i < S; ++i) a[i].v[0] = a[i].v[0] + b[i];
            }
        }
#pragma unroll
        for (int i = 0; i < S; ++i) *reinterpret_cast<FloatV<V>*>(s_in + i * pitch + e) = a[i];
    }
}

// ---- forward, second half: V consecutive floats of the output row a lane
template <int S, int V>
__device__ __forceinline__ void resolve_emit(const ResolveParams& P, const float* s_in, const float (&ex)[RS_MAX_C], float w, int ototal,
                                             int pitch, long long obase, int tid)
{
    const int C = P.C;
    for (int o = tid * V; o < ototal; o += RS_BLOCK * V) {
        FloatV<V> y, l;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int el = o + k, px = (int)(((unsigned)el * P.div_c) >> 16), ch = el - px * C;
            const float* __restrict__ s = s_in + (S * px) * C + ch;
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int j = 0; j < S; ++j) acc += s[i * pitch + j * C];
            const float L = acc * P.inv;
            const float e = ch == 0 ? ex[0] : (ch == 1 ? ex[1] : (ch == 2 ? ex[2] : ex[3]));
            ResolveEval d;
            resolve_develop(P, e, w, L, d);
            l.v[k] = L;
            y.v[k] = clamp_out(P, d.y);
        }
        *reinterpret_cast<FloatV<V>*>(P.out + obase + o) = y;
        if (P.lin) *reinterpret_cast<FloatV<V>*>(P.lin + obase + o) = l;   // (uniform)
    }
}

__device__ __forceinline__ void resolve_scalars(const ResolveParams& P, float (&ex)[RS_MAX_C], float& w)
{
    const float* __restrict__ e = P.expo + (size_t)blockIdx.y * P.estride;
#pragma unroll
    for (int c = 0; c < RS_MAX_C; ++c) ex[c] = c < P.C ? e[c] : 0.f;
    w = P.white ? P.white[(size_t)blockIdx.y * P.wstride] : 1.f;
}

template <int S>
__global__ __launch_bounds__(RS_BLOCK) void resolve_forward_kernel(ResolveParams P)
{
    extern __shared__ __attribute__((aligned(16))) float s_in[];   // [S][span * S * C]
    const int tid = threadIdx.x;
    int r, c0, npx; long long s0, SW, obase;
    resolve_place<S>(P, r, c0, npx, s0, SW, obase);
    const int pitch = resolve_span(S) * S * P.C, total = npx * S * P.C;
    const float* __restrict__ img = P.img + (long long)blockIdx.y * P.img_scene;
    const float* __restrict__ add = P.add ? P.add + (long long)blockIdx.y * P.add_scene : nullptr;
    if (P.vec == 4) resolve_stage<S, 4>(P, img, add, s0, SW, total, pitch, tid, s_in);
    else if (P.vec == 2) resolve_stage<S, 2>(P, img, add, s0, SW, total, pitch, tid, s_in);
    else resolve_stage<S, 1>(P, img, add, s0, SW, total, pitch, tid, s_in);
    float ex[RS_MAX_C], w;
    resolve_scalars(P, ex, w);
    __syncthreads();
    if (P.ovec == 4) resolve_emit<S, 4>(P, s_in, ex, w, npx * P.C, pitch, obase, tid);
    else if (P.ovec == 2) resolve_emit<S, 2>(P, s_in, ex, w, npx * P.C, pitch, obase, tid);
    else resolve_emit<S, 1>(P, s_in, ex, w, npx * P.C, pitch, obase, tid);
}

// ---- backward, first half: d y / d L * g / S^2 of V consecutive floats of the output row into LDS, the lane's terms of the sums
template <int V>
__device__ __forceinline__ void resolve_gather(const ResolveParams& P, float* s_g, const float (&ex)[RS_MAX_C], float w, int ototal,
                                               long long obase, int tid, float (&pe)[RS_MAX_C], float& pw)
{
    const int C = P.C;
    for (int o = tid * V; o < ototal; o += RS_BLOCK * V) {
        const FloatV<V> g = *reinterpret_cast<const FloatV<V>*>(P.gout + obase + o);
        const FloatV<V> l = *reinterpret_cast<const FloatV<V>*>(P.lin_in + obase + o);
        FloatV<V> gs;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int el = o + k, px = (int)(((unsigned)el * P.div_c) >> 16), ch = el - px * C;
            const float e = ch == 0 ? ex[0] : (ch == 1 ? ex[1] : (ch == 2 ? ex[2] : ex[3]));
            ResolveEval d;
            resolve_develop(P, e, w, l.v[k], d);
            float gE, gw;
            resolve_develop_backward(P, w, d, g.v[k], gE, gw);
            gs.v[k] = (gE * e) * P.inv;
            const float ge = gE * l.v[k];
#pragma unroll
            for (int c = 0; c < RS_MAX_C; ++c) pe[c] += ch == c ? ge : 0.f;
            pw += gw;
        }
        *reinterpret_cast<FloatV<V>*>(s_g + o) = gs;
    }
}

// ---- backward, second half: the S stretches of grad_image (and grad_add), V floats a lane
template <int S, int V>
__device__ __forceinline__ void resolve_spread(const ResolveParams& P, const float* s_g, long long s0, long long SW, int total, int tid)
{
    const int C = P.C;
    float* __restrict__ gi = P.gimg ? P.gimg + ((long long)blockIdx.y * P.rows * S * SW + s0) * C : nullptr;
    float* __restrict__ ga = P.gadd ? P.gadd + ((long long)blockIdx.y * P.rows * S * SW + s0) * C : nullptr;
    for (int e = tid * V; e < total; e += RS_BLOCK * V) {
        FloatV<V> v;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int el = e + k, q = (int)(((unsigned)el * P.div_c) >> 16), ch = el - q * C;
            v.v[k] = s_g[(q / S) * C + ch];
        }
#pragma unroll
        for (int i = 0; i < S; ++i) {
            if (gi) *reinterpret_cast<FloatV<V>*>(gi + i * SW * C + e) = v;   // (uniform)
            if (ga) *reinterpret_cast<FloatV<V>*>(ga + i * SW * C + e) = v;   // (uniform)
        }
    }
}

template <int N>
__device__ __forceinline__ void resolve_fold_exposure(const float* s_part, float* partial, int tid)
{
    if (tid < N) fold_waves_to_row<N>(s_part, partial, tid);
}

template <int S>
__global__ __launch_bounds__(RS_BLOCK) void resolve_backward_kernel(ResolveParams P)
{
    __shared__ __attribute__((aligned(16))) float s_g[RS_SPAN * RS_MAX_C];
    __shared__ float s_part_e[4 * RS_MAX_C];
    __shared__ float s_part_w[4];
    const int tid = threadIdx.x, C = P.C;
    int r, c0, npx; long long s0, SW, obase;
    resolve_place<S>(P, r, c0, npx, s0, SW, obase);
    float ex[RS_MAX_C], w;
    resolve_scalars(P, ex, w);
    float pe[RS_MAX_C] = {0.f, 0.f, 0.f, 0.f}, pw = 0.f;
    if (P.ovec == 4) resolve_gather<4>(P, s_g, ex, w, npx * C, obase, tid, pe, pw);
    else if (P.ovec == 2) resolve_gather<2>(P, s_g, ex, w, npx * C, obase, tid, pe, pw);
    else resolve_gather<1>(P, s_g, ex, w, npx * C, obase, tid, pe, pw);
    const int wave = tid >> 6, lane = tid & 63;
    if (P.part_e) {   // (uniform)
#pragma unroll
        for (int c = 0; c < RS_MAX_C; ++c) {
            if (c < C) {   // (uniform)
                const float s = wave_sum(pe[c]);
                if (lane == 0) s_part_e[wave * C + c] = s;
            }
        }
    }
    if (P.part_w) {   // (uniform)
        const float s = wave_sum(pw);
        if (lane == 0) s_part_w[wave] = s;
    }
    __syncthreads();
    if (P.gimg || P.gadd) {   // (uniform)
        const int total = npx * S * C;
        if (P.vec == 4) resolve_spread<S, 4>(P, s_g, s0, SW, total, tid);
        else if (P.vec == 2) resolve_spread<S, 2>(P, s_g, s0, SW, total, tid);
        else resolve_spread<S, 1>(P, s_g, s0, SW, total, tid);
    }
    if (P.part_e) {   // (uniform)
        if (C == 1) resolve_fold_exposure<1>(s_part_e, P.part_e, tid);
        else if (C == 2) resolve_fold_exposure<2>(s_part_e, P.part_e, tid);
        else if (C == 3) resolve_fold_exposure<3>(s_part_e, P.part_e, tid);
        else resolve_fold_exposure<4>(s_part_e, P.part_e, tid);
    }
    if (P.part_w && tid < 1) fold_waves_to_row<1>(s_part_w, P.part_w, tid);
}

template <class F>
inline void resolve_dispatch(int S, F&& f)
{
    if (S == 1) f(std::integral_constant<int, 1>{});
    else if (S == 2) f(std::integral_constant<int, 2>{});
    else if (S == 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 4>{});
}

}  // namespace dirt

extern "C" {

static constexpr dirt::ErrorSetter report = dirt::set_last_error;   // the error channel of this file's entry points

// the arguments both entry points take, under the names they take them by
struct ResolveArgs {
    long long scenes, rows, cols;
    int channels, factor, exposure_scenes, white_scenes, curve, encode;
    float lo, hi; unsigned flags;
};

// the workgroups of a scene; 0 for sizes the entry points refuse
static long long resolve_blocks(long long rows, long long cols, int channels, int factor)
{
    if (rows < 0 || cols < 0 || rows > 0x7fffffffll / DIRT_RESOLVE_MAX_FACTOR || cols > 0x7fffffffll / DIRT_RESOLVE_MAX_FACTOR) return 0;
    if (channels < 1 || channels > DIRT_RESOLVE_MAX_CHANNELS || factor < 1 || factor > DIRT_RESOLVE_MAX_FACTOR) return 0;
    if (rows > 0 && cols > (1ll << 36) / rows) return 0;
    const int span = dirt::resolve_span(factor);
    const long long blocks = rows * ((cols + span - 1) / span);
    return blocks > 0x7fffffffll ? 0 : blocks;
}

// the widest access, in floats, that a pointer and the floats of a row allow
static int resolve_width(const void* p, long long row_floats)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (!(a & 15u) && !(row_floats & 3)) return 4;
    if (!(a & 7u) && !(row_floats & 1)) return 2;
    return 1;
}

// what both entry points refuse, before any device work; fills what they share of P
static int resolve_check(const char* who, const ResolveArgs& a, bool has_white, dirt::ResolveParams& P)
{
    if (a.scenes < 0 || a.scenes > 65535) STAGE_FAIL("%s: %lld scenes, 0..65535", who, a.scenes);
    if (a.channels < 1 || a.channels > DIRT_RESOLVE_MAX_CHANNELS) STAGE_FAIL("%s: %d channels, 1..%d", who, a.channels, DIRT_RESOLVE_MAX_CHANNELS);
    if (a.factor < 1 || a.factor > DIRT_RESOLVE_MAX_FACTOR) STAGE_FAIL("%s: factor=%d, 1..%d", who, a.factor, DIRT_RESOLVE_MAX_FACTOR);
    if (a.rows < 0 || a.cols < 0 || (a.rows != 0 && a.cols != 0 && resolve_blocks(a.rows, a.cols, a.channels, a.factor) == 0))
        STAGE_FAIL("%s: bad image size (rows=%lld cols=%lld), at most (2^31 - 1) / %d each way and 2^36 pixels", who, a.rows, a.cols,
                   DIRT_RESOLVE_MAX_FACTOR);
    if (a.curve != DIRT_RESOLVE_LINEAR && a.curve != DIRT_RESOLVE_REINHARD && a.curve != DIRT_RESOLVE_ACES)
        STAGE_FAIL("%s: curve=%d is none of DIRT_RESOLVE_LINEAR, _REINHARD, _ACES", who, a.curve);
    if (a.encode != DIRT_RESOLVE_ENCODE_LINEAR && a.encode != DIRT_RESOLVE_ENCODE_SRGB)
        STAGE_FAIL("%s: encode=%d is neither DIRT_RESOLVE_ENCODE_LINEAR nor _SRGB", who, a.encode);
    if (a.flags & ~DIRT_RESOLVE_CLAMP) STAGE_FAIL("%s: unknown flags 0x%x", who, a.flags);
    if ((a.flags & DIRT_RESOLVE_CLAMP) && !(a.lo <= a.hi)) STAGE_FAIL("%s: clamp bounds lo=%g > hi=%g", who, a.lo, a.hi);
    if (a.exposure_scenes != 1 && a.exposure_scenes != a.scenes)
        STAGE_FAIL("%s: exposure_scenes=%d is neither 1 nor scenes=%lld", who, a.exposure_scenes, a.scenes);
    if ((a.curve == DIRT_RESOLVE_REINHARD) != has_white) STAGE_FAIL("%s: white goes with DIRT_RESOLVE_REINHARD and only with it (curve=%d)", who, a.curve);
    if (has_white && a.white_scenes != 1 && a.white_scenes != a.scenes)
        STAGE_FAIL("%s: white_scenes=%d is neither 1 nor scenes=%lld", who, a.white_scenes, a.scenes);
    P.rows = (int)a.rows; P.cols = (int)a.cols; P.C = a.channels;
    const int span = dirt::resolve_span(a.factor);
    P.chunks = (int)((a.cols + span - 1) / span);
    P.estride = a.exposure_scenes == 1 ? 0 : a.channels; P.wstride = has_white && a.white_scenes != 1 ? 1 : 0;
    P.div_c = 65536u / (unsigned)a.channels + 1u;
    P.curve = a.curve; P.encode = a.encode; P.clamp = (a.flags & DIRT_RESOLVE_CLAMP) ? 1 : 0;
    P.lo = a.lo; P.hi = a.hi; P.inv = (float)(1.0 / (double)(a.factor * a.factor));
    return DIRT_OK;
}

size_t dirt_resolve_scratch_bytes(long long scenes, long long rows, long long cols, int channels, int factor)
{
    if (scenes < 0 || scenes > 65535) return 0;
    return sizeof(float) * (size_t)scenes * (size_t)resolve_blocks(rows, cols, channels, factor) * (size_t)(channels + 1);
}

int dirt_resolve_forward(const float* image, const float* add, const float* exposure, const float* white, float* out, float* linear,
                         long long scenes, long long rows, long long cols, int channels, int factor, int image_stride, int add_stride,
                         int image_scenes, int add_scenes, int exposure_scenes, int white_scenes, int curve, int encode, float clamp_lo,
                         float clamp_hi, unsigned flags, void* stream)
{
    const char* who = "dirt_resolve_forward";
    dirt::ResolveParams P{};
    const ResolveArgs a{scenes, rows, cols, channels, factor, exposure_scenes, white_scenes, curve, encode, clamp_lo, clamp_hi, flags};
    if (int rc = resolve_check(who, a, white != nullptr, P)) return rc;
    if (image_stride < channels) STAGE_FAIL("%s: image_stride=%d, a sample is %d floats", who, image_stride, channels);
    if (add && add_stride < channels) STAGE_FAIL("%s: add_stride=%d, a sample is %d floats", who, add_stride, channels);
    if (image_scenes != 1 && image_scenes != scenes) STAGE_FAIL("%s: image_scenes=%d is neither 1 nor scenes=%lld", who, image_scenes, scenes);
    if (add && add_scenes != 1 && add_scenes != scenes) STAGE_FAIL("%s: add_scenes=%d is neither 1 nor scenes=%lld", who, add_scenes, scenes);
    if (scenes == 0 || rows == 0 || cols == 0) return dirt::stage_ok(report);
    if (!image || !exposure || !out) STAGE_FAIL("%s: image / exposure / out is NULL", who);
    const long long samples = rows * cols * factor * factor, row_floats = cols * factor * channels;
    P.img = image; P.add = add; P.expo = exposure; P.white = white; P.out = out; P.lin = linear;
    P.istride = image_stride; P.astride = add ? add_stride : channels;
    P.img_scene = image_scenes == 1 ? 0 : samples * image_stride; P.add_scene = add && add_scenes != 1 ? samples * add_stride : 0;
    P.vec = 1;
    if (image_stride == channels && P.astride == channels) {
        P.vec = resolve_width(image, row_floats);
        if (add) { const int v = resolve_width(add, row_floats); P.vec = v < P.vec ? v : P.vec; }
    }
    P.ovec = resolve_width(out, cols * channels);
    if (linear) { const int v = resolve_width(linear, cols * channels); P.ovec = v < P.ovec ? v : P.ovec; }
    const dim3 grid((unsigned)resolve_blocks(rows, cols, channels, factor), (unsigned)scenes);
    dirt::resolve_dispatch(factor, [&](auto s) {
        constexpr int S = decltype(s)::value;
        const size_t lds = sizeof(float) * (size_t)S * dirt::resolve_span(S) * S * channels;
        hipLaunchKernelGGL((dirt::resolve_forward_kernel<S>), grid, dim3(dirt::RS_BLOCK), lds, reinterpret_cast<hipStream_t>(stream), P);
    });
    return dirt::stage_hip(report, who, hipGetLastError());
}

int dirt_resolve_backward(const float* linear, const float* exposure, const float* white, const float* grad_out, float* grad_image,
                          float* grad_add, float* grad_exposure, float* grad_white, void* scratch, size_t scratch_bytes, long long scenes,
                          long long rows, long long cols, int channels, int factor, int exposure_scenes, int white_scenes, int curve,
                          int encode, float clamp_lo, float clamp_hi, unsigned flags, void* stream)
{
    const char* who = "dirt_resolve_backward";
    dirt::ResolveParams P{};
    const ResolveArgs a{scenes, rows, cols, channels, factor, exposure_scenes, white_scenes, curve, encode, clamp_lo, clamp_hi, flags};
    if (int rc = resolve_check(who, a, white != nullptr, P)) return rc;
    if (grad_white && !white) STAGE_FAIL("%s: grad_white without white", who);
    if (!grad_image && !grad_add && !grad_exposure && !grad_white) return dirt::stage_ok(report);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (scenes == 0 || rows == 0 || cols == 0) {   // nothing to launch: the sums are zeros
        hipError_t e = grad_exposure ? hipMemsetAsync(grad_exposure, 0, sizeof(float) * (size_t)exposure_scenes * channels, s) : hipSuccess;
        if (e == hipSuccess && grad_white) e = hipMemsetAsync(grad_white, 0, sizeof(float) * (size_t)white_scenes, s);
        return dirt::stage_hip(report, who, e);
    }
    if (!linear || !exposure || !grad_out) STAGE_FAIL("%s: linear / exposure / grad_out is NULL", who);
    const long long blocks = resolve_blocks(rows, cols, channels, factor);
    if (grad_exposure || grad_white)
        if (int rc = dirt::check_scratch(report, who, scratch, scratch_bytes, dirt_resolve_scratch_bytes(scenes, rows, cols, channels, factor),
                                         "dirt_resolve_scratch_bytes"))
            return rc;
    P.lin_in = linear; P.expo = exposure; P.white = white; P.gout = grad_out; P.gimg = grad_image; P.gadd = grad_add;
    float* const base = static_cast<float*>(scratch);
    if (grad_exposure) P.part_e = base;
    if (grad_white) P.part_w = base + scenes * blocks * channels;
    const long long row_floats = cols * factor * channels;
    P.vec = 4;
    if (grad_image) { const int v = resolve_width(grad_image, row_floats); P.vec = v < P.vec ? v : P.vec; }
    if (grad_add) { const int v = resolve_width(grad_add, row_floats); P.vec = v < P.vec ? v : P.vec; }
    P.ovec = resolve_width(grad_out, cols * channels);
    { const int v = resolve_width(linear, cols * channels); P.ovec = v < P.ovec ? v : P.ovec; }
    const dim3 grid((unsigned)blocks, (unsigned)scenes);
    dirt::resolve_dispatch(factor, [&](auto f) {
        hipLaunchKernelGGL((dirt::resolve_backward_kernel<decltype(f)::value>), grid, dim3(dirt::RS_BLOCK), 0, s, P);
    });
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && grad_exposure) {
        dirt::shade_launch_reduce(P.part_e, grad_exposure, exposure_scenes == 1 ? scenes * blocks : blocks, channels, exposure_scenes, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess && grad_white) {
        dirt::shade_launch_reduce(P.part_w, grad_white, white_scenes == 1 ? scenes * blocks : blocks, 1, white_scenes, s);
        e = hipGetLastError();
    }
    return dirt::stage_hip(report, who, e);
}

}  // extern "C"
