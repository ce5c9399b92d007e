// STOM on the device (gfx950): what the reference's Spatio-Temporal Overlay Module does between the point tracker and the preprocessors (model/STOM.py:72-207), for a
// whole clip, with every per-frame decision kept in device memory -- no host round trip.  The numpy path of rga3/model/STOM.py is the exact reference: all arithmetic
// here is integer or single-operation IEEE (this file builds with floating-point contraction off), so the frames are equal byte for byte.
//
//   stom_flow_kernel       one workgroup per frame: mean_flow (:102-131).  Flow magnitudes of the visible points, their median and median absolute deviation by two
//                          bitonic sorts of the fp32 bit patterns in LDS (non-negative floats order like unsigned integers; hidden points and padding sort last as
//                          +inf), the keep test, the mean of the kept flows summed in fp64 in a fixed order and rounded once to fp32 -> record {apply, dx, dy, kept}.
//   stom_shift_kernel      one thread per destination pixel: shift_overlay + composite (:145-160) as a gather.  The reference scatters in row-major order, the last
//                          writer wins, so the source is the lexicographically largest (y, x) with alpha > 0 that truncates onto the pixel (<= 3 candidates per axis).
//   mask-shaped prompts (warp_point, :163-207):
//   stom_first_kernel      the first alpha > 0 pixel of the overlay in row-major order (integer atomic max of ~index), once per clip;
//   stom_raster_kernel     visible points -> bit-packed mask [T, H, ceil(W / 64)] by integer atomic OR, and the visible count of the gate;
//   stom_morph_kernel      dilation / erosion with the elliptical kernel on 64-bit words: per kernel row one horizontal span OR over a window of the word and its two
//                          neighbours, ORed over the rows.  The erosion is the dilation of the complement inside the frame (outside pixels neither set nor clear
//                          anything), and its pass sums count, sum x, sum y of the closed mask by popcounts and 64-bit integer atomics instead of storing it;
//   stom_circle_kernel     one thread per pixel: the filled circle at the centroid from a half-width table, composited in the prompt's clamped colour.
// Compositing is Pillow's alpha_composite over an opaque base followed by convert("RGB") in Pillow's integer arithmetic (AlphaComposite.c, 7 precision bits).
#include "common.h"

namespace rga3 {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned char u8;

constexpr int kStomMaxPoints = 16384;   // the reference's grid_size = 100 gives at most 10^4
constexpr int kStomMaxKernel = 128;     // one neighbour word each side covers a span of the structuring element
constexpr int kStomMaxRadius = 128;
constexpr int kFlowThreads = 1024;
constexpr u32 kInfBits = 0x7f800000u;

struct StomSpans { u8 lo[kStomMaxKernel], hi[kStomMaxKernel]; };   // kernel row i is set on columns lo[i] .. hi[i]
struct StomCircle { u8 hw[kStomMaxRadius + 1]; };                  // row |dy| of the filled circle covers |dx| <= hw[|dy|]

// workspace: {~first alpha index, pad} u32, per frame {count, sum x, sum y, visible} u64, then two bit-packed masks
constexpr int kStatWords = 4;
static inline int64_t stom_head_words(int64_t frames) { return 1 + kStatWords * frames; }

// Pillow's alpha_composite(dst, src) for an opaque dst, one channel, then convert("RGB") (which drops the alpha): AlphaComposite.c with dst->a = 255
__device__ __forceinline__ u32 pil_over(u32 d, u32 s, u32 a) {
    if (a == 0) return d;
    const u32 blend = 255u * (255u - a);
    const u32 outa255 = a * 255u + blend;
    const u32 coef1 = a * 255u * 255u * 128u / outa255;
    const u32 coef2 = 255u * 128u - coef1;
    const u32 t = s * coef1 + d * coef2 + (0x80u << 7);
    return (((t >> 8) + t) >> 8) >> 7;
}

__device__ __forceinline__ void composite_px(const u8* __restrict__ f, u8* __restrict__ o, u32 r, u32 g, u32 b, u32 a) {
    o[0] = (u8)pil_over(f[0], r, a);
    o[1] = (u8)pil_over(f[1], g, a);
    o[2] = (u8)pil_over(f[2], b, a);
}

// ---------------------------------------------------------------------------------------------------------------- flow record
__device__ __forceinline__ float flow_mag(const float* __restrict__ vip, const float* __restrict__ tgt, int n, float& fx, float& fy) {
#pragma clang fp contract(off)
    fx = tgt[2 * n] - vip[2 * n];
    fy = tgt[2 * n + 1] - vip[2 * n + 1];
    const float xx = fx * fx, yy = fy * fy;
    return sqrtf(xx + yy);
}

// ascending bitonic sort of s[0 .. p), p a power of two
__device__ __forceinline__ void lds_sort(u32* s, int p) {
    for (int k = 2; k <= p; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < p; i += kFlowThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const u32 a = s[i], b = s[l];
                    if (((i & k) == 0) ? (a > b) : (a < b)) {
                        s[i] = b;
                        s[l] = a;
                    }
                }
            }
        }
    }
    __syncthreads();
}

// median of the first m (> 0) of the sorted values: numpy's mean of the two middle ones for an even count
__device__ __forceinline__ float lds_median(const u32* s, int m) {
#pragma clang fp contract(off)
    const float a = __uint_as_float(s[(m - 1) >> 1]), b = __uint_as_float(s[m >> 1]);
    return (m & 1) ? a : (a + b) * 0.5f;
}

__global__ __launch_bounds__(kFlowThreads) void stom_flow_kernel(const float* __restrict__ tracks, const u8* __restrict__ vis, int* __restrict__ rec, int n_pts, int p,
                                                                 int vip_idx) {
#pragma clang fp contract(off)
    extern __shared__ u32 s_keys[];
    __shared__ double s_sum[2][kFlowThreads];
    __shared__ int s_cnt[kFlowThreads];
    __shared__ int s_flag;
    const int t = blockIdx.x, tid = threadIdx.x;
    int* out = rec + 4 * t;
    if (t == vip_idx) {
        if (tid < 4) out[tid] = 0;
        return;
    }
    const float* vip = tracks + (size_t)vip_idx * n_pts * 2;
    const float* tgt = tracks + (size_t)t * n_pts * 2;
    const u8* v = vis + (size_t)t * n_pts;
    if (tid == 0) s_flag = 0;
    __syncthreads();
    int nvis = 0;
    bool bad = false;
    for (int n = tid; n < p; n += kFlowThreads) {
        u32 key = kInfBits;
        if (n < n_pts && v[n]) {
            float fx, fy;
            key = __float_as_uint(flow_mag(vip, tgt, n, fx, fy));
            ++nvis;
            bad |= key >= kInfBits;
        }
        s_keys[n] = key;
    }
    s_cnt[tid] = nvis;
    if (bad) s_flag = 1;
    __syncthreads();
    for (int o = kFlowThreads / 2; o > 0; o >>= 1) {
        if (tid < o) s_cnt[tid] += s_cnt[tid + o];
        __syncthreads();
    }
    nvis = s_cnt[0];
    const bool skip = nvis == 0 || s_flag != 0;   // uniform: no visible point, or a non-finite magnitude (finite tracks are a precondition)
    __syncthreads();
    if (skip) {
        if (tid < 4) out[tid] = 0;
        return;
    }
    lds_sort(s_keys, p);
    const float med = lds_median(s_keys, nvis);
    __syncthreads();
    for (int n = tid; n < p; n += kFlowThreads) {
        u32 key = kInfBits;
        if (n < n_pts && v[n]) {
            float fx, fy;
            key = __float_as_uint(fabsf(flow_mag(vip, tgt, n, fx, fy) - med));
        }
        s_keys[n] = key;
    }
    lds_sort(s_keys, p);
    const float mad = lds_median(s_keys, nvis);
    const float thr = 3.f * mad;
    const float lo = med - thr, hi = med + thr;
    double sx = 0.0, sy = 0.0;
    int kept = 0;
    for (int n = tid; n < n_pts; n += kFlowThreads) {
        if (v[n]) {
            float fx, fy;
            const float mag = flow_mag(vip, tgt, n, fx, fy);
            if (mag >= lo && mag <= hi) {
                sx += (double)fx;
                sy += (double)fy;
                ++kept;
            }
        }
    }
    s_sum[0][tid] = sx;
    s_sum[1][tid] = sy;
    s_cnt[tid] = kept;
    __syncthreads();
    for (int o = kFlowThreads / 2; o > 0; o >>= 1) {
        if (tid < o) {
            s_sum[0][tid] += s_sum[0][tid + o];
            s_sum[1][tid] += s_sum[1][tid + o];
            s_cnt[tid] += s_cnt[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        kept = s_cnt[0];
        const bool apply = kept > 0 && kept >= n_pts / 2;
        const float dx = apply ? (float)(s_sum[0][0] / (double)kept) : 0.f;
        const float dy = apply ? (float)(s_sum[1][0] / (double)kept) : 0.f;
        out[0] = apply ? 1 : 0;
        out[1] = __float_as_int(dx);
        out[2] = __float_as_int(dy);
        out[3] = kept;
    }
}

// ---------------------------------------------------------------------------------------------------------------- shifted overlay + composite
// the sources c with trunc((double)c + d) == dst are among dst - trunc(d) + {-1, 0, 1}: the rounded sum is monotone in c and within one of c + trunc(d)
__device__ __forceinline__ bool lands_on(int c, double d, int dst) { return trunc((double)c + d) == (double)dst; }

__global__ __launch_bounds__(256) void stom_shift_kernel(const u8* __restrict__ frames, const u8* __restrict__ ov, const int* __restrict__ rec, u8* __restrict__ out,
                                                         int h, int w, int vip_idx) {
    const int idx = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (idx >= h * w) return;
    const size_t px = ((size_t)t * h * w + idx) * 3;
    const u8* f = frames + px;
    u8* o = out + px;
    int src = -1;
    if (t == vip_idx) {
        src = idx;
    } else if (rec[4 * t]) {
        const double dx = (double)__int_as_float(rec[4 * t + 1]), dy = (double)__int_as_float(rec[4 * t + 2]);
        if (fabs(dx) < 1.0e9 && fabs(dy) < 1.0e9) {   // anything larger lands outside every frame (and keeps the integer conversions below in range)
            const int ny = idx / w, nx = idx % w;
            const int by = ny - (int)trunc(dy), bx = nx - (int)trunc(dx);
            for (int y = by + 1; y >= by - 1 && src < 0; --y) {
                if (y < 0 || y >= h || !lands_on(y, dy, ny)) continue;
                for (int x = bx + 1; x >= bx - 1; --x) {
                    if (x < 0 || x >= w || !lands_on(x, dx, nx)) continue;
                    if (ov[((size_t)y * w + x) * 4 + 3]) {
                        src = y * w + x;
                        break;
                    }
                }
            }
        }
    }
    if (src < 0) {
        o[0] = f[0];
        o[1] = f[1];
        o[2] = f[2];
    } else {
        const u8* s = ov + (size_t)src * 4;
        composite_px(f, o, s[0], s[1], s[2], s[3]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- mask-shaped prompts
__global__ __launch_bounds__(256) void stom_first_kernel(const u8* __restrict__ ov, u32* __restrict__ first, int pixels) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const bool on = idx < pixels && ov[(size_t)idx * 4 + 3] != 0;
    const u64 m = __ballot(on);
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicMax(first, 0xffffffffu - (u32)idx);   // 0 = no such pixel
}

__global__ __launch_bounds__(256) void stom_raster_kernel(const float* __restrict__ tracks, const u8* __restrict__ vis, u64* __restrict__ stats, u64* __restrict__ mask,
                                                          int n_pts, int h, int w, int w64, int vip_idx) {
    const int n = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (t == vip_idx) return;
    const bool on = n < n_pts && vis[(size_t)t * n_pts + n] != 0;
    if (on) {
        const float* pt = tracks + ((size_t)t * n_pts + n) * 2;
        const float c = pt[0], r = pt[1];
        // int() truncates toward zero: (-1, 0) is row / column 0
        if (r > -1.f && r < (float)h && c > -1.f && c < (float)w) {
            const int row = (int)r, col = (int)c;
            atomicOr(mask + ((size_t)t * h + row) * w64 + (col >> 6), 1ull << (col & 63));
        }
    }
    const u64 m = __ballot(on);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(stats + (size_t)t * kStatWords + 3, (u64)__popcll(m));
}

struct Win { u64 l, c, r; };   // a word and its two neighbours in the row: bit i of l / c / r is column i - 64 / i / i + 64 of the word

__device__ __forceinline__ void win_shr(Win& v, int s) {   // towards lower columns by 0 <= s <= 64, zeros enter from above
    if (s == 64) {
        v.l = v.c;
        v.c = v.r;
        v.r = 0;
    } else if (s) {
        v.l = (v.l >> s) | (v.c << (64 - s));
        v.c = (v.c >> s) | (v.r << (64 - s));
        v.r >>= s;
    }
}

// bit x of the result = OR of columns x + a .. x + b of the window row, -64 <= a <= 0 <= b <= 63: a running OR of width b - a + 1 by doubling, then moved by a
__device__ __forceinline__ u64 span_or(Win v, int a, int b) {
    const int n = b - a + 1;
    for (int cov = 1; cov < n;) {
        const int s = min(cov, n - cov);
        Win q = v;
        win_shr(q, s);
        v.l |= q.l;
        v.c |= q.c;
        v.r |= q.r;
        cov += s;
    }
    const int m = -a;
    return m == 0 ? v.c : m == 64 ? v.l : (v.c << m) | (v.l >> (64 - m));
}

__device__ __forceinline__ u64 valid_bits(int wx, int w, int w64) { return (wx == w64 - 1 && (w & 63)) ? (1ull << (w & 63)) - 1ull : ~0ull; }

// kErode = false: dst = dilate(src).  kErode = true: erode(src) is not stored; its count / sum x / sum y are added to the frame's stats.
template <bool kErode>
__global__ __launch_bounds__(256) void stom_morph_kernel(const u64* __restrict__ src, u64* __restrict__ dst, u64* __restrict__ stats, int h, int w, int w64, int rows,
                                                         int anchor, int vip_idx, StomSpans sp) {
    const int idx = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (t == vip_idx) return;
    u64 res = 0;
    int y = 0, wx = 0;
    const bool in = idx < h * w64;
    if (in) {
        y = idx / w64;
        wx = idx % w64;
        const u64* fs = src + (size_t)t * h * w64;
        for (int i = 0; i < rows; ++i) {
            const int sy = y + i - anchor;
            if (sy < 0 || sy >= h) continue;
            const u64* row = fs + (size_t)sy * w64;
            Win v;
            v.l = wx > 0 ? row[wx - 1] : 0;
            v.c = row[wx];
            v.r = wx + 1 < w64 ? row[wx + 1] : 0;
            if (kErode) {
                v.l = wx > 0 ? ~v.l : 0;
                v.c = ~v.c & valid_bits(wx, w, w64);
                v.r = wx + 1 < w64 ? ~v.r & valid_bits(wx + 1, w, w64) : 0;
            }
            res |= span_or(v, (int)sp.lo[i] - anchor, (int)sp.hi[i] - anchor);
        }
        if (kErode) res = ~res;
        res &= valid_bits(wx, w, w64);
    }
    if (!kErode) {
        if (in) dst[(size_t)t * h * w64 + idx] = res;
        return;
    }
    u64 cnt = __popcll(res);
    u64 sx = (u64)wx * 64 * cnt;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        constexpr u64 kBit[6] = {0xaaaaaaaaaaaaaaaaull, 0xccccccccccccccccull, 0xf0f0f0f0f0f0f0f0ull, 0xff00ff00ff00ff00ull, 0xffff0000ffff0000ull, 0xffffffff00000000ull};
        sx += (u64)__popcll(res & kBit[b]) << b;
    }
    u64 sy = (u64)y * cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        sx += __shfl_xor(sx, o, 64);
        sy += __shfl_xor(sy, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
        u64* s = stats + (size_t)t * kStatWords;
        atomicAdd(s + 0, cnt);
        atomicAdd(s + 1, sx);
        atomicAdd(s + 2, sy);
    }
}

__global__ __launch_bounds__(256) void stom_circle_kernel(const u8* __restrict__ frames, const u8* __restrict__ ov, const u32* __restrict__ first,
                                                          const u64* __restrict__ stats, u8* __restrict__ out, int h, int w, int n_pts, int radius, int vip_idx,
                                                          StomCircle circle) {
    __shared__ int s_c[3];    // draw, cx, cy
    __shared__ u32 s_rgba[4];
    const int idx = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (threadIdx.x == 0 && t != vip_idx) {
        const u64* s = stats + (size_t)t * kStatWords;
        const u64 cnt = s[0];
        const bool draw = s[3] >= (u64)(n_pts / 2) && cnt > 0;
        s_c[0] = draw;
        s_c[1] = draw ? (int)(s[1] / cnt) : 0;
        s_c[2] = draw ? (int)(s[2] / cnt) : 0;
        const u32 code = *first;
        u32 r = 0, g = 0, b = 0, a = 0;
        if (code) {
            const u8* p = ov + (size_t)(0xffffffffu - code) * 4;
            r = p[0], g = p[1], b = p[2], a = p[3];
        }
        s_rgba[0] = r;
        s_rgba[1] = g;
        s_rgba[2] = b;
        s_rgba[3] = min(max(a, 96u), 148u);
    }
    __syncthreads();
    if (idx >= h * w) return;
    const size_t px = ((size_t)t * h * w + idx) * 3;
    const u8* f = frames + px;
    u8* o = out + px;
    if (t == vip_idx) {
        const u8* s = ov + (size_t)idx * 4;
        composite_px(f, o, s[0], s[1], s[2], s[3]);
        return;
    }
    bool inside = false;
    if (s_c[0]) {
        const int ady = abs(idx / w - s_c[2]), adx = abs(idx % w - s_c[1]);
        inside = ady <= radius && adx <= (int)circle.hw[ady];
    }
    if (inside) {
        composite_px(f, o, s_rgba[0], s_rgba[1], s_rgba[2], s_rgba[3]);
    } else {
        o[0] = f[0];
        o[1] = f[1];
        o[2] = f[2];
    }
}

// frames / h / w the kernels' 32-bit indices and the launch grids hold
static bool stom_shape_ok(int64_t frames, int64_t h, int64_t w) {
    if (frames <= 0 || h <= 0 || w <= 0 || frames > 65535 || h > (1 << 24) || w > (1 << 24)) return false;
    return h * w < (1ll << 31) - 256;
}

}  // namespace rga3

using namespace rga3;

extern "C" int64_t rga3_stom_ws_bytes(int64_t frames, int64_t h, int64_t w) {
    if (!stom_shape_ok(frames, h, w)) return fail(RGA3_EINVAL, "stom_ws_bytes: bad shape [%ld, %ld, %ld]", (long)frames, (long)h, (long)w);
    return (stom_head_words(frames) + 2 * frames * h * cdiv(w, 64)) * (int64_t)sizeof(u64);
}

extern "C" int rga3_stom_flow(const float* tracks, const void* visibility, int* records, int64_t frames, int64_t n_points, int vip_frame_idx, void* stream) {
    RGA3_CHECK_ARG(tracks && visibility && records, "stom_flow: null pointer");
    RGA3_CHECK_ARG(frames > 0 && frames <= 65535, "stom_flow: %ld frames (1..65535)", (long)frames);
    RGA3_CHECK_ARG(n_points > 0 && n_points <= kStomMaxPoints, "stom_flow: %ld points (1..%d)", (long)n_points, kStomMaxPoints);
    RGA3_CHECK_ARG(vip_frame_idx >= 0 && vip_frame_idx < frames, "stom_flow: vip_frame_idx %d outside [0, %ld)", vip_frame_idx, (long)frames);
    int p = 2;
    while (p < n_points) p <<= 1;
    const int lds = p * (int)sizeof(u32);
    return launch_lds<stom_flow_kernel>(dim3((unsigned)frames), dim3(kFlowThreads), lds, (hipStream_t)stream, "stom_flow", tracks, (const u8*)visibility, records,
                                        (int)n_points, p, vip_frame_idx);
}

extern "C" int rga3_stom_shift_composite(const void* frames_u8, const void* overlay_rgba, const int* records, void* out, int64_t frames, int64_t h, int64_t w,
                                         int vip_frame_idx, void* stream) {
    RGA3_CHECK_ARG(frames_u8 && overlay_rgba && records && out && frames_u8 != out, "stom_shift_composite: null pointer or in-place call");
    RGA3_CHECK_ARG(stom_shape_ok(frames, h, w), "stom_shift_composite: bad shape [%ld, %ld, %ld] (non-empty, <= 65535 frames)", (long)frames, (long)h, (long)w);
    RGA3_CHECK_ARG(vip_frame_idx >= 0 && vip_frame_idx < frames, "stom_shift_composite: vip_frame_idx %d outside [0, %ld)", vip_frame_idx, (long)frames);
    hipLaunchKernelGGL(stom_shift_kernel, dim3((unsigned)cdiv(h * w, 256), (unsigned)frames), dim3(256), 0, (hipStream_t)stream, (const u8*)frames_u8,
                       (const u8*)overlay_rgba, records, (u8*)out, (int)h, (int)w, vip_frame_idx);
    RGA3_CHECK_LAUNCH("stom_shift_composite");
    return 0;
}

extern "C" int rga3_stom_mask_composite(const void* frames_u8, const void* overlay_rgba, const float* tracks, const void* visibility, void* out, void* ws,
                                        int64_t ws_bytes, int64_t frames, int64_t h, int64_t w, int64_t n_points, int vip_frame_idx, const void* spans, int ksize,
                                        const void* half_widths, int radius, void* stream) {
    RGA3_CHECK_ARG(frames_u8 && overlay_rgba && tracks && visibility && out && ws && spans && half_widths && frames_u8 != out,
                   "stom_mask_composite: null pointer or in-place call");
    RGA3_CHECK_ARG(stom_shape_ok(frames, h, w), "stom_mask_composite: bad shape [%ld, %ld, %ld] (non-empty, <= 65535 frames)", (long)frames, (long)h, (long)w);
    RGA3_CHECK_ARG(n_points > 0 && n_points <= kStomMaxPoints, "stom_mask_composite: %ld points (1..%d)", (long)n_points, kStomMaxPoints);
    RGA3_CHECK_ARG(vip_frame_idx >= 0 && vip_frame_idx < frames, "stom_mask_composite: vip_frame_idx %d outside [0, %ld)", vip_frame_idx, (long)frames);
    RGA3_CHECK_ARG(ksize >= 0 && ksize <= kStomMaxKernel, "stom_mask_composite: structuring element of %d (0..%d)", ksize, kStomMaxKernel);
    RGA3_CHECK_ARG(radius >= 0 && radius <= kStomMaxRadius, "stom_mask_composite: radius %d (0..%d)", radius, kStomMaxRadius);
    const int64_t w64 = cdiv(w, 64), words = frames * h * w64, head = stom_head_words(frames);
    RGA3_CHECK_ARG(ws_bytes >= (head + 2 * words) * (int64_t)sizeof(u64) && ((uintptr_t)ws & 7) == 0,
                   "stom_mask_composite: workspace of rga3_stom_ws_bytes() bytes needed (8-byte aligned)");
    const int rows = ksize > 1 ? ksize : 1, anchor = ksize > 1 ? ksize / 2 : 0;
    StomSpans sp = {};
    const u8* sb = (const u8*)spans;   // rows x {lo, hi}
    for (int i = 0; i < rows; ++i) {
        sp.lo[i] = sb[2 * i];
        sp.hi[i] = sb[2 * i + 1];
        RGA3_CHECK_ARG(sp.lo[i] <= anchor && sp.hi[i] >= anchor && sp.hi[i] < rows, "stom_mask_composite: span %d = [%d, %d] does not hold the anchor column %d", i,
                       (int)sp.lo[i], (int)sp.hi[i], anchor);
    }
    StomCircle circle = {};
    for (int i = 0; i <= radius; ++i) {
        circle.hw[i] = ((const u8*)half_widths)[i];
        RGA3_CHECK_ARG(circle.hw[i] <= radius, "stom_mask_composite: half width %d of row %d exceeds the radius %d", (int)circle.hw[i], i, radius);
    }
    hipStream_t st = (hipStream_t)stream;
    u64* head_p = (u64*)ws;
    u64* stats = head_p + 1;
    u64* mask = head_p + head;
    u64* dil = mask + words;
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)(head + words) * sizeof(u64), st);   // first, stats and the raster; the dilation is written whole
    if (e != hipSuccess) return fail(-(int)e, "stom_mask_composite: memset: %s", hipGetErrorString(e));
    const dim3 frames_y_words((unsigned)cdiv(h * w64, 256), (unsigned)frames), frames_y_px((unsigned)cdiv(h * w, 256), (unsigned)frames);
    hipLaunchKernelGGL(stom_first_kernel, dim3((unsigned)cdiv(h * w, 256)), dim3(256), 0, st, (const u8*)overlay_rgba, (u32*)head_p, (int)(h * w));
    RGA3_CHECK_LAUNCH("stom_mask_composite (first)");
    hipLaunchKernelGGL(stom_raster_kernel, dim3((unsigned)cdiv(n_points, 256), (unsigned)frames), dim3(256), 0, st, tracks, (const u8*)visibility, stats, mask,
                       (int)n_points, (int)h, (int)w, (int)w64, vip_frame_idx);
    RGA3_CHECK_LAUNCH("stom_mask_composite (raster)");
    hipLaunchKernelGGL(stom_morph_kernel<false>, frames_y_words, dim3(256), 0, st, (const u64*)mask, dil, stats, (int)h, (int)w, (int)w64, rows, anchor, vip_frame_idx, sp);
    RGA3_CHECK_LAUNCH("stom_mask_composite (dilate)");
    hipLaunchKernelGGL(stom_morph_kernel<true>, frames_y_words, dim3(256), 0, st, (const u64*)dil, (u64*)nullptr, stats, (int)h, (int)w, (int)w64, rows, anchor,
                       vip_frame_idx, sp);
    RGA3_CHECK_LAUNCH("stom_mask_composite (erode)");
    hipLaunchKernelGGL(stom_circle_kernel, frames_y_px, dim3(256), 0, st, (const u8*)frames_u8, (const u8*)overlay_rgba, (const u32*)head_p, (const u64*)stats, (u8*)out,
                       (int)h, (int)w, (int)n_points, radius, vip_frame_idx, circle);
    RGA3_CHECK_LAUNCH("stom_mask_composite (circle)");
    return 0;
}
