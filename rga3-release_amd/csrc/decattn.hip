// Decode-step attention of generate() on the KV cache where it lies (reference app.py:308-317; HF modeling_qwen2_5_vl.py:602-757 with one query token per sequence).
// One call stands in for rope_kernel + two move_rows_kernel scatters + attn_fwd_kernel<split> + attn_split_combine_kernel of a decode layer:
//
//   decattn_partials_kernel   workgroup = (key slice of kDecKS keys, kv head, sequence): rotates its G query heads, and -- in the slice that holds position lens[b] --
//                             the new key row; stores the rotated k row and the v row at cache position lens[b]; leaves an un-normalised partial (max, sum, o[G][D]
//                             in f32) of softmax(scale q K^T) V over its keys in the workspace
//   decattn_combine_kernel    workgroup = (query head, sequence): merges the lens[b] / kDecKS + 1 partials in slice order, divides, rounds to bf16
//
// The cache is [B, cap, Hkv, D] through (sequence, token, head) strides, the lengths are ON THE DEVICE: a captured launch serves every length up to cap, and B
// sequences are the same code as one.  How a sequence's keys fall into slices and waves depends on lens[b] alone (slice s = keys [s * kDecKS, (s + 1) * kDecKS), wave w
// of it the next 16), never on B, cap or the neighbours: the output bits of a sequence do not depend on who shares its batch.  No atomics, fixed summation order.
//
// Lanes: 16 lanes x 16 bytes hold one row of D <= 128 (lane c of a 16-lane group: elements 8 c .. 8 c + 7; c >= D / 8 idles).  The four 16-lane groups of a wave take
// HPG = ceil(G / 4) query heads each and read the SAME 16 key rows (one pass over the group's K / V from L2 / HBM; the repeat is served inside the CU), so a wave's
// softmax over its 16 keys needs no merge between lane groups; the four waves meet in LDS.  K / V go straight to VGPRs, all 32 row loads of a wave issued before the
// first use (the kernel waits on latency, not on bytes: 4.3 MB of K / V per layer at S = 2112).  Rows past lens[b] are loaded (clamped inside the view) and then
// replaced by zeros on both the score and the value side: whatever they hold, NaN included, never reaches the result.
#include "common.h"

namespace rga3 {

constexpr int kDecKS = 64;                       // keys per slice (compile-time: the partition of a sequence is a function of its length only)
constexpr int kDecWaves = 4;
constexpr int kDecKW = kDecKS / kDecWaves;       // keys per wave
constexpr int kDecLdsRow = 132;                  // floats per (wave, head) in LDS: o[128], max, sum, 2 pad (rows start on 16 bytes)

struct DecAttnArgs {
    const unsigned short* qkv;   // [B, Hq + 2 Hkv, D] bf16, un-rotated, read-only
    const float* cs;             // [B, D]
    const float* sn;
    unsigned short* kc;          // caches
    unsigned short* vc;
    const int* lens;             // [B] tokens already stored (device)
    unsigned short* out;         // [B, Hq, D] bf16
    float* ws;                   // [B, Hkv, nsl, G, D + 2]
    int Hq, Hkv, G, D, nsl, cap;
    long ld_qkv, k_sb, k_st, k_sh, v_sb, v_st, v_sh, ld_out;
    float scale;
};

// one 8-wide chunk of x cos + rotate_half(x) sin, rope_kernel's arithmetic (rowops.hip): first half a c - b s with b the partner in the second half, second half
// b c + a s with a the partner in the first; f32, one bf16 rounding
__device__ __forceinline__ void rot8(const u32x4& own, const u32x4& par, const float* c, const float* s, bool first, float* o) {
    float x[8], y[8];
    unpack8(own, x);
    unpack8(par, y);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = first ? x[e] * c[e] - y[e] * s[e] : x[e] * c[e] + y[e] * s[e];
}

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int HPG>
__global__ __launch_bounds__(256) void decattn_partials_kernel(DecAttnArgs p) {
    __shared__ __attribute__((aligned(16))) float part[kDecWaves][8][kDecLdsRow];
    const int sl = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int len = p.lens[b];
    if (len < 0 || len >= p.cap) return;          // a length the host could not see: nothing is written (the combine makes the rows NaN)
    const int k0 = sl * kDecKS;
    if (k0 > len) return;                         // slice beyond the visible keys 0 .. len
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = lane & 15, grp = lane >> 4;
    const int D = p.D, cpr = D >> 3, hc = cpr >> 1;
    const bool act = c < cpr;
    const int cc = act ? c : 0;                   // idle lanes read chunk 0 (inside the row) and drop it
    const bool first = cc < hc;
    const int pc = first ? cc + hc : cc - hc;     // rotate-half partner chunk
    float cs[8], sn[8];
    {
        const float* cp = p.cs + (long)b * D + cc * 8;
        const float* sp = p.sn + (long)b * D + cc * 8;
        *(f32x4*)&cs[0] = *(const f32x4*)cp;
        *(f32x4*)&cs[4] = *(const f32x4*)(cp + 4);
        *(f32x4*)&sn[0] = *(const f32x4*)sp;
        *(f32x4*)&sn[4] = *(const f32x4*)(sp + 4);
    }
    const unsigned short* xrow = p.qkv + (long)b * p.ld_qkv;
    // ---- K / V rows of this wave: all loads first
    const int kbase = k0 + wv * kDecKW;
    const unsigned short* kp = p.kc + (long)b * p.k_sb + (long)h * p.k_sh + cc * 8;
    const unsigned short* vp = p.vc + (long)b * p.v_sb + (long)h * p.v_sh + cc * 8;
    u32x4 kk[kDecKW], vv[kDecKW];
#pragma unroll
    for (int j = 0; j < kDecKW; ++j) {
        const long r = min(kbase + j, p.cap - 1);                 // inside the view whatever the slice's tail
        kk[j] = *(const u32x4*)(kp + r * p.k_st);
        vv[j] = *(const u32x4*)(vp + r * p.v_st);
    }
    // ---- this group's query heads, rotated, as the bf16 numbers rope_ would have stored
    float q[HPG][8];
#pragma unroll
    for (int i = 0; i < HPG; ++i) {
        const int g = grp * HPG + i;
        const unsigned short* qr = xrow + (long)(h * p.G + min(g, p.G - 1)) * D;
        float o[8];
        rot8(*(const u32x4*)(qr + cc * 8), *(const u32x4*)(qr + pc * 8), cs, sn, first, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) q[i][e] = (act && g < p.G) ? bf16_round(o[e]) : 0.f;
    }
    // ---- the new row: the slice that holds position len rotates k, stores k and v, and keeps both in registers (no workgroup reads what another one writes)
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    u32x4 newk = zero4, newv = zero4;
    if (len < k0 + kDecKS) {
        const unsigned short* kr = xrow + (long)(p.Hq + h) * D;
        float o[8];
        rot8(*(const u32x4*)(kr + cc * 8), *(const u32x4*)(kr + pc * 8), cs, sn, first, o);
        newk = pack8(o);
        newv = *(const u32x4*)(xrow + (long)(p.Hq + p.Hkv + h) * D + cc * 8);
        if (wv == (len - k0) / kDecKW && grp == 0 && act) {
            *(u32x4*)(p.kc + (long)b * p.k_sb + (long)len * p.k_st + (long)h * p.k_sh + c * 8) = newk;
            *(u32x4*)(p.vc + (long)b * p.v_sb + (long)len * p.v_st + (long)h * p.v_sh + c * 8) = newv;
        }
    }
    // ---- scores
    float s[kDecKW][HPG];
#pragma unroll
    for (int j = 0; j < kDecKW; ++j) {
        const int kidx = kbase + j;
        const bool stored = act && kidx < len, fresh = act && kidx == len;     // fresh: only in the owning slice, where newk / newv are set
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            kk[j][e] = stored ? kk[j][e] : (fresh ? newk[e] : 0u);
            vv[j][e] = stored ? vv[j][e] : (fresh ? newv[e] : 0u);
        }
        float kf[8];
        unpack8(kk[j], kf);
#pragma unroll
        for (int i = 0; i < HPG; ++i) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) d = fmaf(kf[e], q[i][e], d);
            d = group16_sum(d);
            s[j][i] = kidx <= len ? d * p.scale : -INFINITY;
        }
    }
    // ---- softmax over the wave's keys, values
    float m[HPG], l[HPG], o[HPG][8];
#pragma unroll
    for (int i = 0; i < HPG; ++i) {
        m[i] = -INFINITY;
#pragma unroll
        for (int j = 0; j < kDecKW; ++j) m[i] = fmaxf(m[i], s[j][i]);
        l[i] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[i][e] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < kDecKW; ++j) {
        const bool vis = kbase + j <= len;
        float vf[8];
        unpack8(vv[j], vf);
#pragma unroll
        for (int i = 0; i < HPG; ++i) {
            const float pj = vis ? __expf(s[j][i] - m[i]) : 0.f;
            l[i] += pj;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[i][e] = fmaf(pj, vf[e], o[i][e]);
        }
    }
#pragma unroll
    for (int i = 0; i < HPG; ++i) {
        const int g = grp * HPG + i;
        if (act && g < p.G) {
            float* pr = &part[wv][g][0];
            *(f32x4*)(pr + c * 8) = *(const f32x4*)&o[i][0];
            *(f32x4*)(pr + c * 8 + 4) = *(const f32x4*)&o[i][4];
            if (c == 0) {
                pr[128] = m[i];
                pr[129] = l[i];
            }
        }
    }
    __syncthreads();
    // ---- the four waves, in wave order (a wave without visible keys carries max -inf, sum 0, o 0: weight exp(-inf) = 0)
    float* wout = p.ws + (((long)b * p.Hkv + h) * p.nsl + sl) * (long)p.G * (D + 2);
    for (int idx = threadIdx.x; idx < p.G * D; idx += 256) {
        const int g = idx / D, d = idx - g * D;
        float mw[kDecWaves], M = -INFINITY;
#pragma unroll
        for (int w = 0; w < kDecWaves; ++w) {
            mw[w] = part[w][g][128];
            M = fmaxf(M, mw[w]);
        }
        float acc = 0.f, lsum = 0.f;
#pragma unroll
        for (int w = 0; w < kDecWaves; ++w) {
            const float e = __expf(mw[w] - M);
            acc = fmaf(part[w][g][d], e, acc);
            lsum = fmaf(part[w][g][129], e, lsum);
        }
        float* wr = wout + (long)g * (D + 2);
        wr[d] = acc;
        if (d == 0) {
            wr[D] = M;
            wr[D + 1] = lsum;
        }
    }
}

// One workgroup per (query head, sequence), thread = output column.  The slice maxima are read by one thread each (one round of latency instead of a serial walk),
// the weights exp(max_s - M) are computed once per slice into LDS, and the columns are summed in slice order with eight independent loads in flight.
__global__ __launch_bounds__(128) void decattn_combine_kernel(DecAttnArgs p) {
    __shared__ float e_s[128], l_s[128], red[2];
    const int hq = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int D = p.D;
    const int len = p.lens[b];
    unsigned short* o = p.out + (long)b * p.ld_out + (long)hq * D + t;
    if (len < 0 || len >= p.cap) {                // (uniform over the workgroup)
        if (t < D) *o = 0x7fc0;                   // NaN: the sequence has no room for this step's row
        return;
    }
    const int ns = len / kDecKS + 1;              // <= nsl: len < cap
    const int h = hq / p.G, g = hq - h * p.G;
    const long ss = (long)p.G * (D + 2);
    const float* __restrict__ base = p.ws + (((long)b * p.Hkv + h) * p.nsl) * ss + (long)g * (D + 2);
    float M = -INFINITY;
    for (int s = t; s < ns; s += 128) M = fmaxf(M, base[s * ss + D]);
    M = wave_max(M);
    if ((t & 63) == 0) red[t >> 6] = M;
    __syncthreads();
    M = fmaxf(red[0], red[1]);                    // finite: slice 0 always holds a visible key
    float acc = 0.f, l = 0.f;
    for (int c0 = 0; c0 < ns; c0 += 128) {
        const int n = min(128, ns - c0);
        __syncthreads();                          // the previous chunk's weights have been read
        if (t < n) {
            const float* r = base + (c0 + t) * ss;
            e_s[t] = __expf(r[D] - M);
            l_s[t] = r[D + 1];
        }
        __syncthreads();
        if (t < D) {
            const float* __restrict__ col = base + c0 * ss + t;
            int s = 0;
            for (; s + 8 <= n; s += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = col[(s + u) * ss];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = fmaf(v[u], e_s[s + u], acc);
            }
            for (; s < n; ++s) acc = fmaf(col[s * ss], e_s[s], acc);
        }
        for (int s = 0; s < n; ++s) l = fmaf(l_s[s], e_s[s], l);
    }
    if (t < D) *o = f2bf(acc / l);
}

}  // namespace rga3

using namespace rga3;

extern "C" int rga3_decode_attn_slice_keys(void) { return kDecKS; }

extern "C" int64_t rga3_decode_attn_ws_floats(int64_t B, int64_t cap, int Hq, int D) {
    if (B < 1 || B > 65535 || cap < 1 || cap > 0x7fffffff - kDecKS || Hq < 1 || Hq > (1 << 20) || D < 1 || D > (1 << 20)) return -1;   // shapes: the call's business
    return B * Hq * cdiv(cap, kDecKS) * (D + 2);
}

extern "C" int rga3_decode_attn(const void* qkv, const float* cos, const float* sin, void* k_cache, void* v_cache, const int32_t* lens, void* out, float* ws,
                                int64_t ws_floats, int64_t B, int Hq, int Hkv, int D, int64_t cap, int64_t ld_qkv, int64_t k_sb, int64_t k_st, int64_t k_sh,
                                int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t ld_out, float scale, void* stream) {
    RGA3_CHECK_ARG(qkv && cos && sin && k_cache && v_cache && lens && out && ws, "decode_attn: null pointer");
    RGA3_CHECK_ARG(B >= 1 && B <= 65535, "decode_attn: B=%ld (1 to 65535 sequences)", (long)B);
    RGA3_CHECK_ARG(Hq >= 1 && Hkv >= 1 && Hkv <= 65535 && Hq % Hkv == 0 && Hq / Hkv <= 8, "decode_attn: Hq=%d Hkv=%d (at most 8 query heads per kv head)", Hq, Hkv);
    RGA3_CHECK_ARG(D >= 16 && D <= 128 && D % 16 == 0, "decode_attn: D=%d (a multiple of 16, at most 128)", D);
    RGA3_CHECK_ARG(cap >= 1 && cap <= 0x7fffffff - kDecKS, "decode_attn: cap=%ld", (long)cap);
    RGA3_CHECK_ARG((((uintptr_t)cos | (uintptr_t)sin) & 15) == 0, "decode_attn: cos/sin tables must be 16-byte aligned");
    RGA3_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0 && (((uintptr_t)lens | (uintptr_t)ws) & 3) == 0,
                   "decode_attn: qkv and the caches must be 16-byte aligned");
    RGA3_CHECK_ARG(ld_qkv % 8 == 0 && k_sb % 8 == 0 && k_st % 8 == 0 && k_sh % 8 == 0 && v_sb % 8 == 0 && v_st % 8 == 0 && v_sh % 8 == 0,
                   "decode_attn: strides must be multiples of 8 elements (rows start on 16 bytes)");
    RGA3_CHECK_LD("decode_attn", "ld_qkv", ld_qkv, (int64_t)(Hq + 2 * Hkv) * D, B);
    RGA3_CHECK_LD("decode_attn", "ld_out", ld_out, (int64_t)Hq * D, B);
    RGA3_CHECK_HEADS("decode_attn", "k_cache", k_st, k_sh, cap, (int64_t)Hkv, (int64_t)D);
    RGA3_CHECK_HEADS("decode_attn", "v_cache", v_st, v_sh, cap, (int64_t)Hkv, (int64_t)D);
    RGA3_CHECK_ARG(k_st >= 0 && k_sh >= 0 && v_st >= 0 && v_sh >= 0, "decode_attn: negative stride");
    RGA3_CHECK_LD("decode_attn", "k_cache sequence stride", k_sb, (cap - 1) * k_st + (Hkv - 1) * k_sh + D, B);
    RGA3_CHECK_LD("decode_attn", "v_cache sequence stride", v_sb, (cap - 1) * v_st + (Hkv - 1) * v_sh + D, B);
    const int64_t need = rga3_decode_attn_ws_floats(B, cap, Hq, D);
    RGA3_CHECK_ARG(ws_floats >= need, "decode_attn: workspace of %ld floats, %ld needed", (long)ws_floats, (long)need);
    DecAttnArgs a;
    a.qkv = (cus)qkv; a.cs = cos; a.sn = sin; a.kc = (us)k_cache; a.vc = (us)v_cache; a.lens = lens; a.out = (us)out; a.ws = ws;
    a.Hq = Hq; a.Hkv = Hkv; a.G = Hq / Hkv; a.D = D; a.nsl = (int)cdiv(cap, kDecKS); a.cap = (int)cap;
    a.ld_qkv = ld_qkv; a.k_sb = k_sb; a.k_st = k_st; a.k_sh = k_sh; a.v_sb = v_sb; a.v_st = v_st; a.v_sh = v_sh; a.ld_out = ld_out;
    a.scale = scale;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)a.nsl, (unsigned)Hkv, (unsigned)B);
    if (a.G <= 4) hipLaunchKernelGGL(decattn_partials_kernel<1>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(decattn_partials_kernel<2>, grid, dim3(256), 0, st, a);
    RGA3_CHECK_LAUNCH("decattn_partials_kernel");
    hipLaunchKernelGGL(decattn_combine_kernel, dim3((unsigned)Hq, (unsigned)B), dim3(128), 0, st, a);
    RGA3_CHECK_LAUNCH("decattn_combine_kernel");
    return 0;
}
