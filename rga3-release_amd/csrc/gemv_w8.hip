// Weight-only e4m3 decode step of generate() (reference app.py:308-317): the decoder projections stored as OCP e4m3 codes with one power-of-two scale per output
// row, streamed against M <= 4 bf16 activation rows.  The bf16 stream (gemv_kernel, gemm_bf16.hip, tile 40) reads 2 bytes per weight and token; this one reads 1.
//
//   quant_e4m3_rows_pow2_kernel   bf16 [rows, K] -> codes [rows, K] + scales [rows], scale = 2^k with k the smallest integer such that amax <= 448 * 2^k
//   gemv_w8_kernel                C[M, N] = (A[M, K] . code[N, K]^T) * scale[n] (+ bias) (SwiGLU) (+ residual), the e4m3 twin of gemv_kernel
//
// A power-of-two scale makes every dequantised weight code * 2^k a bf16 number (4 significant bits, exponent in range), so the bf16 kernels can run on exactly the
// values this one sees, and x / scale is exact.  A bf16 x e4m3 product has 8 + 4 = 12 significant bits: every product of the FMA chain below is exact in fp32, only
// the running sum rounds.
#include "common.h"

namespace rga3 {

enum { W8_ACT_NONE = RGA3_ACT_NONE, W8_ACT_SWIGLU = RGA3_ACT_SWIGLU };

// x * sigmoid(x) exactly as gemv_kernel's epilogue computes it (silu_f of gemm_bf16.hip, restated here so that the bf16 kernels' source stays as it is): the two
// must round alike, which tests/test_gemv_w8_gpu.py pins (SwiGLU outputs bit-identical to tile 40's).
__device__ __forceinline__ float silu_w8(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// ---------------------------------------------------------------------------------------------- row quantiser
// One 256-thread block per row, as quant_fp8_rows_kernel (gemm_fp8.hip): amax, then the codes; a thread's first chunks stay in registers between the two passes.
// k comes from amax's exponent and mantissa fields with integer compares: amax = 1.f * 2^(E - 127) = m * 2^(E - 126) with m = 1.f / 2 in [0.5, 1), and
// 448 = 0.875 * 2^9, so k = E - 126 - 9 when 1.f <= 1.75 (mantissa field <= 0x600000) and one more otherwise; clamped to k >= -126 so that 2^k and 2^-k are both
// normal numbers (bf16 subnormal rows land there).  x * 2^-k is exact (|x| <= 448 * 2^k; what underflows is far below e4m3's smallest subnormal 2^-9).
__global__ __launch_bounds__(256) void quant_e4m3_rows_pow2_kernel(const unsigned short* __restrict__ x, unsigned char* __restrict__ q, float* __restrict__ scales,
                                                                   int K, long ldx, long ldq) {
    __shared__ float part[4];
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    const unsigned short* xr = x + row * ldx;
    const int nch = K / 8;
    constexpr int KEEP = 4;
    u32x4 kept[KEEP];
    float amax = 0.f;
    auto amax8 = [&](const u32x4& v) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            amax = fmaxf(amax, fabsf(__uint_as_float(v[e] << 16)));
            amax = fmaxf(amax, fabsf(__uint_as_float(v[e] & 0xffff0000u)));
        }
    };
#pragma unroll
    for (int i = 0; i < KEEP; ++i) {
        const int ch = tid + i * 256;
        kept[i] = u32x4{0u, 0u, 0u, 0u};
        if (ch < nch) {
            kept[i] = *(const u32x4*)(xr + ch * 8);
            amax8(kept[i]);
        }
    }
    for (int ch = tid + KEEP * 256; ch < nch; ch += 256) amax8(*(const u32x4*)(xr + ch * 8));
    amax = wave_max(amax);
    if ((tid & 63) == 0) part[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
    const unsigned ab = __float_as_uint(amax);
    int k = (int)(ab >> 23) - 135 + ((ab & 0x7fffffu) > 0x600000u ? 1 : 0);
    k = max(k, -126);
    if (ab == 0u) k = 0;                                                // a zero row: scale 1
    const float rs = __uint_as_float((unsigned)(127 - k) << 23);        // 2^-k
    if (tid == 0) scales[row] = __uint_as_float((unsigned)(127 + k) << 23);
    unsigned char* qr = q + row * ldq;
    auto put = [&](int ch, const u32x4& v) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[2 * e] = __uint_as_float(v[e] << 16) * rs;
            f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u) * rs;
        }
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
        u32x2 o;
        o[0] = (unsigned)lo;
        o[1] = (unsigned)hi;
        *(u32x2*)(qr + ch * 8) = o;
    };
#pragma unroll
    for (int i = 0; i < KEEP; ++i) {
        const int ch = tid + i * 256;
        if (ch < nch) put(ch, kept[i]);
    }
    for (int ch = tid + KEEP * 256; ch < nch; ch += 256) put(ch, *(const u32x4*)(xr + ch * 8));
}

// ---------------------------------------------------------------------------------------------- weight stream
struct GemvW8Args {
    const unsigned short* A;   // [M, K] bf16
    const unsigned char* W;    // [N, K] e4m3 codes
    const float* sw;           // [N] row scales (powers of two)
    void* C;
    const unsigned short* bias;
    const unsigned short* res;
    int M, N, K;               // N = weight rows (SwiGLU: 2 x outputs)
    long lda, ldw, ldc, ldr;   // ldw in bytes
};

// 16 codes (one 16-byte load) -> 16 floats, in K order: word j, byte b is element 4 j + b
__device__ __forceinline__ void decode16(const u32x4& w, float* f) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
        f[4 * j] = lo[0];
        f[4 * j + 1] = lo[1];
        f[4 * j + 2] = hi[0];
        f[4 * j + 3] = hi[1];
    }
}

// A workgroup (4 waves) owns CW output columns and splits K between its waves: wave w reads the 16-byte chunks w * 64 + l, + 256, ... of each of the workgroup's
// weight rows (lane l; 16 codes a chunk, coalesced 1 KiB per row, wave and step, RW independent rows in flight) against the 16 matching activations (two 16-byte
// loads, L1 / L2 resident).  The four partial sums of a column meet in LDS and are added in wave order (fixed order: reproducible).  gemv_kernel gives a wave whole
// rows; at one byte per weight a row is over in half the steps, and the o_proj / down_proj widths (N = 3584: 896 such waves, 3.5 per CU, 4 KiB each) leave a CU
// with too few loads in flight -- here it holds 3.5 workgroups of 16 KiB.  Measured against two chunks per row in flight on whole-row waves.
template <int MR, int ACT, bool OUT_F32>
__global__ __launch_bounds__(256) void gemv_w8_kernel(GemvW8Args p) {
    constexpr int CW = 4;                                      // output columns per workgroup
    constexpr int RW = (ACT == W8_ACT_SWIGLU) ? 2 * CW : CW;   // weight rows per workgroup
    constexpr int NWV = 4;                                     // waves splitting K
    __shared__ float part[NWV][MR][RW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int Nout = (ACT == W8_ACT_SWIGLU) ? p.N / 2 : p.N;
    const int o0 = (int)blockIdx.x * CW;                       // < Nout: the grid is cdiv(Nout, CW)
    // weight rows of this workgroup's outputs (SwiGLU packing: 32-row blocks = 16 gate rows, then the 16 up rows of the same outputs)
    const unsigned char* wrow[RW];
#pragma unroll
    for (int cidx = 0; cidx < CW; ++cidx) {
        const int o = min(o0 + cidx, Nout - 1);
        if constexpr (ACT == W8_ACT_SWIGLU) {
            wrow[2 * cidx] = p.W + (long)((o >> 4) * 32 + (o & 15)) * p.ldw;
            wrow[2 * cidx + 1] = p.W + (long)((o >> 4) * 32 + 16 + (o & 15)) * p.ldw;
        } else {
            wrow[cidx] = p.W + (long)o * p.ldw;
        }
    }
    float acc[MR][RW];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[m][r] = 0.f;
    const int nch = p.K >> 4;
    for (int ch = wv * 64 + lane; ch < nch; ch += 64 * NWV) {      // nothing past a row's end is read, weights or activations
        u32x4 w[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) w[r] = __builtin_nontemporal_load((const u32x4*)(wrow[r] + (long)ch * 16));   // read-once weight stream kept out of L2 / Infinity Cache
        float xf[MR][16];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const unsigned short* xr = p.A + (long)min(m, p.M - 1) * p.lda + (long)ch * 16;
            unpack8(*(const u32x4*)xr, xf[m]);
            unpack8(*(const u32x4*)(xr + 8), xf[m] + 8);
        }
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            float wf[16];
            decode16(w[r], wf);
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[m][r] = fmaf(wf[e], xf[m][e], acc[m][r]);
        }
    }
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const float s = wave_sum(acc[m][r]);
            if (lane == 0) part[wv][m][r] = s;
        }
    __syncthreads();
    if (threadIdx.x >= CW * MR) return;
    const int cidx = threadIdx.x % CW, m = threadIdx.x / CW;
    const int o = o0 + cidx;
    if (o >= Nout || m >= p.M) return;
    auto total = [&](int r) { return ((part[0][m][r] + part[1][m][r]) + part[2][m][r]) + part[3][m][r]; };
    float v;
    // from here on gemv_kernel's epilogue, operation for operation, after the row scale (a power of two: exact)
    if constexpr (ACT == W8_ACT_SWIGLU) {
        const int rg = (o >> 4) * 32 + (o & 15), ru = rg + 16;
        float gt = total(2 * cidx) * p.sw[rg], up = total(2 * cidx + 1) * p.sw[ru];
        if (p.bias) {
            gt += bf2f(p.bias[rg]);
            up += bf2f(p.bias[ru]);
        }
        gt = bf2f(f2bf(gt));
        up = bf2f(f2bf(up));
        v = bf2f(f2bf(silu_w8(gt))) * up;
    } else {
        v = total(cidx) * p.sw[o];
        if (p.bias) v += bf2f(p.bias[o]);
    }
    if constexpr (OUT_F32) {
        ((float*)p.C)[(long)m * p.ldc + o] = v;
    } else {
        if (p.res) v = bf2f(f2bf(v)) + bf2f(p.res[(long)m * p.ldr + o]);
        ((unsigned short*)p.C)[(long)m * p.ldc + o] = f2bf(v);
    }
}

template <int ACT, bool OUT_F32>
static int launch_gemv_w8(const GemvW8Args& g, hipStream_t st) {
    const int nout = (ACT == W8_ACT_SWIGLU) ? g.N / 2 : g.N;
    const unsigned grid = (unsigned)cdiv(nout, 4);
    if (g.M == 1) hipLaunchKernelGGL((gemv_w8_kernel<1, ACT, OUT_F32>), dim3(grid), dim3(256), 0, st, g);
    else if (g.M == 2) hipLaunchKernelGGL((gemv_w8_kernel<2, ACT, OUT_F32>), dim3(grid), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((gemv_w8_kernel<4, ACT, OUT_F32>), dim3(grid), dim3(256), 0, st, g);
    RGA3_CHECK_LAUNCH("gemv_w8_kernel");
    return 0;
}

}  // namespace rga3

using namespace rga3;

extern "C" int rga3_quant_e4m3_rows_pow2(const void* w, void* q, float* scales, int64_t rows, int64_t K, int64_t ldw, int64_t ldq, void* stream) {
    RGA3_CHECK_ARG(w && q && scales, "quant_e4m3_rows_pow2: null pointer");
    RGA3_CHECK_ARG(rows > 0 && rows <= 0x7fffffff && K > 0 && K <= 0x7fffffff && K % 16 == 0, "quant_e4m3_rows_pow2: rows=%ld K=%ld (K must be a multiple of 16)",
                   (long)rows, (long)K);
    RGA3_CHECK_ARG(ldw % 8 == 0 && ldq % 16 == 0, "quant_e4m3_rows_pow2: ldw=%ld ldq=%ld (rows must start on 16 bytes)", (long)ldw, (long)ldq);
    RGA3_CHECK_ARG((((uintptr_t)w | (uintptr_t)q) & 15) == 0, "quant_e4m3_rows_pow2: pointers must be 16-byte aligned");
    RGA3_CHECK_LD("quant_e4m3_rows_pow2", "ldw", ldw, K, rows);
    RGA3_CHECK_LD("quant_e4m3_rows_pow2", "ldq", ldq, K, rows);
    hipLaunchKernelGGL(quant_e4m3_rows_pow2_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)w, (unsigned char*)q, scales,
                       (int)K, (long)ldw, (long)ldq);
    RGA3_CHECK_LAUNCH("quant_e4m3_rows_pow2_kernel");
    return 0;
}

extern "C" int rga3_gemv_w8(const void* A, const void* Wq, const float* sw, const void* bias, const void* residual, void* C, int64_t M, int64_t N, int64_t K,
                            int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int act, int out_dtype, void* stream) {
    RGA3_CHECK_ARG(A && Wq && sw && C, "gemv_w8: null pointer");
    RGA3_CHECK_ARG(M >= 1 && M <= 4, "gemv_w8: M=%ld (1 to 4 activation rows)", (long)M);
    RGA3_CHECK_ARG(N > 0 && N <= 0x7fffffff && K > 0 && K <= 0x7fffffff && K % 16 == 0, "gemv_w8: N=%ld K=%ld (K must be a multiple of 16)", (long)N, (long)K);
    RGA3_CHECK_ARG(act == RGA3_ACT_NONE || act == RGA3_ACT_SWIGLU, "gemv_w8: act %d (none or swiglu)", act);
    RGA3_CHECK_ARG(act != RGA3_ACT_SWIGLU || N % 32 == 0, "gemv_w8: N=%ld must be a multiple of 32 for swiglu", (long)N);
    RGA3_CHECK_ARG(out_dtype == RGA3_BF16 || out_dtype == RGA3_F32, "gemv_w8: out_dtype %d", out_dtype);
    RGA3_CHECK_ARG(!(out_dtype == RGA3_F32 && residual), "gemv_w8: f32 output takes no residual");
    RGA3_CHECK_ARG(lda % 8 == 0 && ldw % 16 == 0, "gemv_w8: lda=%ld ldw=%ld (rows must start on 16 bytes)", (long)lda, (long)ldw);
    RGA3_CHECK_ARG((((uintptr_t)A | (uintptr_t)Wq | (uintptr_t)C) & 15) == 0, "gemv_w8: pointers must be 16-byte aligned");
    const int64_t nout = act == RGA3_ACT_SWIGLU ? N / 2 : N;
    RGA3_CHECK_LD("gemv_w8", "lda", lda, K, M);
    RGA3_CHECK_LD("gemv_w8", "ldw", ldw, K, N);
    RGA3_CHECK_LD("gemv_w8", "ldc", ldc, nout, M);
    if (residual) RGA3_CHECK_LD("gemv_w8", "ldr", ldr, nout, M);
    GemvW8Args g;
    g.A = (const unsigned short*)A; g.W = (const unsigned char*)Wq; g.sw = sw; g.C = C;
    g.bias = (const unsigned short*)bias; g.res = (const unsigned short*)residual;
    g.M = (int)M; g.N = (int)N; g.K = (int)K; g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.ldr = ldr;
    hipStream_t st = (hipStream_t)stream;
    if (act == RGA3_ACT_SWIGLU) return out_dtype == RGA3_F32 ? launch_gemv_w8<W8_ACT_SWIGLU, true>(g, st) : launch_gemv_w8<W8_ACT_SWIGLU, false>(g, st);
    return out_dtype == RGA3_F32 ? launch_gemv_w8<W8_ACT_NONE, true>(g, st) : launch_gemv_w8<W8_ACT_NONE, false>(g, st);
}
