// Next-token selection for generate() (gfx950, wave64): HF's RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper
// and the draw, restated per row in f32 with one IEEE operation per step (this file is built with -ffp-contract=off; see the Makefile).
//
//   mark_tokens_kernel      seen[b, ids[b, s]] = 1: every writer stores the same byte, no atomics
//   penalize_kernel         f32 logits with the repetition penalty applied (the full-vocabulary sampling route)
//   select_slice_kernel     grid (vocabulary slices, B): the best min(top_k, slice) candidates of one slice of kSlice logits, as 64-bit keys
//   select_merge_kernel     one block per row: the best min(top_k, V) of the slices' candidates, then top-p, the draw, tok_out and seen
//
// A candidate is one 64-bit key: the f32 score mapped to an unsigned integer of the same order (-0 stored as +0) in the high word, ~index in the low word.  The
// larger key is the better candidate (higher score, then lower index), keys of different tokens differ, and 0 is no token at all (a valid low word has bit 31 set),
// so both kernels are top_k rounds of a block-wide max over keys, the winner struck out after each round.  The order of the result depends on the keys alone: not
// on the slice a token fell into, not on the launch geometry.
#include "common.h"

#include <math.h>

namespace rga3 {

typedef unsigned long long u64;

constexpr int kSelThreads = 256;
constexpr int kSelPerThread = 16;
constexpr int kSlice = kSelThreads * kSelPerThread;   // logits per block of the first launch
constexpr int kMaxTopK = 64;

__device__ __forceinline__ float load_logit(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float load_logit(const unsigned short* p, int64_t i) { return bf2f(p[i]); }

// HF RepetitionPenaltyLogitsProcessor: torch.where(score < 0, score * penalty, score / penalty) on the tokens seen
__device__ __forceinline__ float penalized(float x, bool seen, float penalty) {
    const float m = x * penalty, q = x / penalty;              // both, then selects: no branches in the unrolled load loops
    return seen ? (x < 0.f ? m : q) : x;
}

__device__ __forceinline__ u64 make_key(float s, unsigned idx) {
    unsigned u = __float_as_uint(s);
    if (s == 0.f) u = 0u;                                    // -0.0 and +0.0 are one score
    const unsigned m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)m << 32) | (u64)(~idx);
}
__device__ __forceinline__ float key_score(u64 k) {
    const unsigned m = (unsigned)(k >> 32);
    return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
}
__device__ __forceinline__ unsigned key_index(u64 k) { return ~(unsigned)k; }

__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a > b ? a : b; }

// max of one key per thread over the block; red: kSelThreads / 64 keys of LDS that no thread is still reading (the callers alternate two of them, so one barrier
// per round is enough: a thread writes buffer p again only after the barrier of the round in between, which every reader of buffer p has reached)
__device__ __forceinline__ u64 block_max_key(u64 v, u64* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        v = umax64(v, ((u64)hi << 32) | lo);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = red[0];
#pragma unroll
    for (int w = 1; w < kSelThreads / 64; ++w) r = umax64(r, red[w]);
    return r;
}

__global__ __launch_bounds__(256) void mark_tokens_kernel(const int64_t* __restrict__ ids, unsigned char* __restrict__ seen, int64_t B, int64_t S, int64_t V,
                                                          int64_t ld_ids, int64_t ld_seen) {
    const int64_t total = B * S;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / S, s = i - b * S;
        const int64_t id = ids[b * ld_ids + s];
        if (id >= 0 && id < V) seen[b * ld_seen + id] = 1;
    }
}

template <class T>
__global__ __launch_bounds__(256) void penalize_kernel(const T* __restrict__ logits, const unsigned char* __restrict__ seen, float* __restrict__ out, int64_t V,
                                                       int64_t ld_logits, int64_t ld_seen, int64_t ld_out, float penalty) {
    const int64_t b = blockIdx.y;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x)
        out[b * ld_out + v] = penalized(load_logit(logits, b * ld_logits + v), seen[b * ld_seen + v] != 0, penalty);
}

// cand [B, nslices, top_k] keys, best first; a slice with fewer than top_k tokens ends in zeros
template <class T>
__global__ __launch_bounds__(kSelThreads) void select_slice_kernel(const T* __restrict__ logits, const unsigned char* __restrict__ seen, u64* __restrict__ cand,
                                                                   int64_t V, int64_t ld_logits, int64_t ld_seen, float penalty, float temperature, int top_k) {
    __shared__ u64 red[2][kSelThreads / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y, base = (int64_t)blockIdx.x * kSlice;
    u64 k[kSelPerThread];
    u64 lmax = 0;
#pragma unroll
    for (int i = 0; i < kSelPerThread; ++i) {                  // straight-line: a position past V reads the row's last token and drops the key
        const int64_t v = base + i * kSelThreads + tid;
        const int64_t vc = v < V ? v : V - 1;
        const bool was_seen = seen != nullptr && seen[b * ld_seen + vc] != 0;
        const float s = penalized(load_logit(logits, b * ld_logits + vc), was_seen, penalty) / temperature;
        k[i] = v < V ? make_key(s, (unsigned)vc) : 0;
        lmax = umax64(lmax, k[i]);
    }
    u64* out = cand + ((int64_t)b * gridDim.x + blockIdx.x) * top_k;
#pragma unroll 1
    for (int r = 0; r < top_k; ++r) {
        const u64 win = block_max_key(lmax, red[r & 1]);      // the same value in every thread: the branches below are uniform
        if (tid == 0) out[r] = win;
        if (win == 0) {                                        // the slice is exhausted
            for (int q = r + 1 + tid; q < top_k; q += kSelThreads) out[q] = 0;
            break;
        }
        if (lmax == win) {                                     // keys are unique: exactly one thread owns the winner
            lmax = 0;
#pragma unroll
            for (int i = 0; i < kSelPerThread; ++i) {
                k[i] = k[i] == win ? 0 : k[i];
                lmax = umax64(lmax, k[i]);
            }
        }
    }
}

// One block per row.  cand: the row's ncand = nslices * top_k keys (struck out in place as they are taken).
__global__ __launch_bounds__(kSelThreads) void select_merge_kernel(u64* __restrict__ cand_all, int64_t ncand, unsigned char* __restrict__ seen, int64_t ld_seen,
                                                                   int top_k, float top_p, const float* __restrict__ u, int64_t* __restrict__ tok_out) {
    __shared__ u64 red[2][kSelThreads / 64];
    __shared__ u64 best[kMaxTopK];
    __shared__ float wgt[kMaxTopK];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    u64* cand = cand_all + b * ncand;
    u64 lmax = 0;
    for (int64_t i = tid; i < ncand; i += kSelThreads) lmax = umax64(lmax, cand[i]);
    int K = 0;                                                 // candidates found: min(top_k, V), the same in every thread
#pragma unroll 1
    for (int r = 0; r < top_k; ++r) {
        const u64 win = block_max_key(lmax, red[r & 1]);
        if (win == 0) break;
        if (tid == 0) best[r] = win;
        K = r + 1;
        if (u == nullptr) break;                               // greedy: candidate 0 is the answer
        if (lmax == win) {
            lmax = 0;
            for (int64_t i = tid; i < ncand; i += kSelThreads) {
                u64 c = cand[i];
                if (c == win) cand[i] = c = 0;
                lmax = umax64(lmax, c);
            }
        }
    }
    __syncthreads();
    if (K == 0) {                                              // unreachable for V >= 1; keeps tok_out defined
        if (tid == 0) tok_out[b] = 0;
        return;
    }
    if (u != nullptr) {
        if (tid < K) wgt[tid] = expf(key_score(best[tid]) - key_score(best[0]));
        __syncthreads();
    }
    if (tid != 0) return;
    int pick = 0;
    if (u != nullptr) {
        float Z = 0.f;
        for (int j = 0; j < K; ++j) Z = Z + wgt[j];
        // HF TopPLogitsWarper in descending order: j stays iff the sum of it and everything below it exceeds (1 - top_p) of the mass; the tail sums are taken
        // from the smallest weight upwards, as HF's cumsum over the ascending sort is
        const float thr = (1.f - top_p) * Z;
        int n = 1;
        float tail = 0.f;
        for (int j = K - 1; j >= 1; --j) {
            tail = tail + wgt[j];
            if (tail > thr) ++n;
        }
        float Zn = 0.f;
        for (int j = 0; j < n; ++j) Zn = Zn + wgt[j];
        const float t = u[b] * Zn;
        pick = n - 1;
        float c = 0.f;
        for (int j = 0; j < n; ++j) {
            c = c + wgt[j];
            if (c > t) {
                pick = j;
                break;
            }
        }
    }
    const unsigned tok = key_index(best[pick]);
    tok_out[b] = (int64_t)tok;
    if (seen != nullptr) seen[b * ld_seen + tok] = 1;
}

static inline int64_t select_slices(int64_t V) { return cdiv(V, kSlice); }

}  // namespace rga3

using namespace rga3;

extern "C" int rga3_mark_tokens(const int64_t* ids, void* seen, int64_t B, int64_t S, int64_t V, int64_t ld_ids, int64_t ld_seen, void* stream) {
    RGA3_CHECK_ARG(ids && seen, "mark_tokens: null pointer");
    RGA3_CHECK_ARG(B >= 1 && S >= 0 && V >= 1, "mark_tokens: B=%ld S=%ld V=%ld", (long)B, (long)S, (long)V);
    RGA3_CHECK_LD("mark_tokens", "ld_ids", ld_ids, S, B);
    RGA3_CHECK_LD("mark_tokens", "ld_seen", ld_seen, V, B);
    if (S == 0) return 0;
    hipLaunchKernelGGL(mark_tokens_kernel, dim3(grid1d(B * S)), dim3(256), 0, (hipStream_t)stream, ids, (unsigned char*)seen, B, S, V, ld_ids, ld_seen);
    RGA3_CHECK_LAUNCH("mark_tokens_kernel");
    return 0;
}

extern "C" int rga3_penalize_logits(const void* logits, int dtype, const void* seen, float* out, int64_t B, int64_t V, int64_t ld_logits, int64_t ld_seen,
                                    int64_t ld_out, float penalty, void* stream) {
    RGA3_CHECK_ARG(logits && seen && out, "penalize_logits: null pointer");
    RGA3_CHECK_ARG(dtype == RGA3_BF16 || dtype == RGA3_F32, "penalize_logits: dtype %d", dtype);
    RGA3_CHECK_ARG(B >= 1 && B <= 65535 && V >= 1, "penalize_logits: B=%ld V=%ld", (long)B, (long)V);
    RGA3_CHECK_ARG(penalty > 0.f, "penalize_logits: penalty %g must be positive", (double)penalty);
    RGA3_CHECK_LD("penalize_logits", "ld_logits", ld_logits, V, B);
    RGA3_CHECK_LD("penalize_logits", "ld_seen", ld_seen, V, B);
    RGA3_CHECK_LD("penalize_logits", "ld_out", ld_out, V, B);
    const dim3 grid(grid1d(V, 256, 1024), (unsigned)B);
    if (dtype == RGA3_F32)
        hipLaunchKernelGGL(penalize_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)logits, (const unsigned char*)seen, out, V, ld_logits,
                           ld_seen, ld_out, penalty);
    else
        hipLaunchKernelGGL(penalize_kernel<unsigned short>, grid, dim3(256), 0, (hipStream_t)stream, (cus)logits, (const unsigned char*)seen, out, V, ld_logits,
                           ld_seen, ld_out, penalty);
    RGA3_CHECK_LAUNCH("penalize_kernel");
    return 0;
}

extern "C" int64_t rga3_select_ws_bytes(int64_t B, int64_t V) {
    if (B < 1 || B > 65535 || V < 1 || V > (int64_t)1 << 31) return -1;
    return B * select_slices(V) * kMaxTopK * (int64_t)sizeof(u64);
}

extern "C" int rga3_select_token(const void* logits, int dtype, void* seen, float penalty, float temperature, int top_k, float top_p, const float* u,
                                 int64_t* tok_out, void* ws, int64_t ws_bytes, int64_t B, int64_t V, int64_t ld_logits, int64_t ld_seen, void* stream) {
    RGA3_CHECK_ARG(logits && tok_out && ws, "select_token: null pointer");
    RGA3_CHECK_ARG(dtype == RGA3_BF16 || dtype == RGA3_F32, "select_token: dtype %d", dtype);
    RGA3_CHECK_ARG(B >= 1 && B <= 65535 && V >= 1 && V <= (int64_t)1 << 31, "select_token: B=%ld V=%ld", (long)B, (long)V);
    RGA3_CHECK_ARG(penalty > 0.f, "select_token: penalty %g must be positive", (double)penalty);
    RGA3_CHECK_ARG(temperature > 0.f, "select_token: temperature %g must be positive", (double)temperature);
    RGA3_CHECK_ARG(top_k >= 1 && top_k <= kMaxTopK, "select_token: top_k %d outside 1..%d", top_k, kMaxTopK);
    RGA3_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "select_token: top_p %g outside (0, 1]", (double)top_p);
    RGA3_CHECK_LD("select_token", "ld_logits", ld_logits, V, B);
    if (seen) RGA3_CHECK_LD("select_token", "ld_seen", ld_seen, V, B);
    RGA3_CHECK_ARG(((uintptr_t)ws & 7) == 0, "select_token: ws must be 8-byte aligned");
    const int64_t need = rga3_select_ws_bytes(B, V);
    RGA3_CHECK_ARG(ws_bytes >= need, "select_token: ws holds %ld bytes, %ld needed (rga3_select_ws_bytes)", (long)ws_bytes, (long)need);
    const int64_t nsl = select_slices(V);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nsl, (unsigned)B);
    if (dtype == RGA3_F32)
        hipLaunchKernelGGL(select_slice_kernel<float>, grid, dim3(kSelThreads), 0, st, (const float*)logits, (const unsigned char*)seen, (u64*)ws, V, ld_logits,
                           ld_seen, penalty, temperature, top_k);
    else
        hipLaunchKernelGGL(select_slice_kernel<unsigned short>, grid, dim3(kSelThreads), 0, st, (cus)logits, (const unsigned char*)seen, (u64*)ws, V, ld_logits,
                           ld_seen, penalty, temperature, top_k);
    RGA3_CHECK_LAUNCH("select_slice_kernel");
    hipLaunchKernelGGL(select_merge_kernel, dim3((unsigned)B), dim3(kSelThreads), 0, st, (u64*)ws, nsl * top_k, (unsigned char*)seen, ld_seen, top_k, top_p, u,
                       tok_out);
    RGA3_CHECK_LAUNCH("select_merge_kernel");
    return 0;
}
