// J&F scoring counts on the device (gfx950): the integer half of the reference's region similarity J (db_eval_iou, evaluation/revos/metrics.py:43-74) and boundary
// F-measure (db_eval_boundary / f_measure / _seg2bmap, :77-214; the same file under evaluation/mevis_val_u and evaluation/reason_vos).  The reference dilates two
// boundary maps with a disk of radius r through OpenCV, per frame, on the host; here the masks never leave the device and only six integers per frame come back.
//
// Two launches, no host round trip:
//   jf_pack_kernel   one wave per (frame, 8-row strip, 64-column word): a lane per pixel, __ballot packs the void-masked masks into 64-bit words (bit i = column
//                    64 * word + i), the _seg2bmap boundary word is formed from the words of rows y / y + 1 and the bit of the next column, and written to the
//                    workspace (padding bits of a row's last word are zero by construction); n_fg, n_gt, inter, union by popcount.
//   jf_match_kernel  one thread per boundary word.  dilate(b, disk(r)) at a word is the OR over dy of row y + dy widened by k(dy) = floor(sqrt(r^2 - dy^2)).  k falls as
//                    |dy| grows, so the rows are folded from the centre outwards: Z_0 = row y, Z_j = widen(Z_{j-1}, k(j-1) - k(j)) | row y-j | row y+j, and Z_r is the
//                    dilated row (widen(widen(X, a), b) = widen(X, a + b), and widening distributes over OR).  The total widening is r <= 64 bits, so a window of the
//                    word and its two neighbours is exact at the centre word: after a total shift of c the window is needed (and is exact) only within 64 - c bits of
//                    the centre word.  Words whose own boundary word is empty skip the dilation, which is most of them: boundaries are thin.
// Every sum is an integer atomicAdd: order independent, so the result is exact and reproducible.
#include "common.h"

namespace rga3 {

typedef unsigned long long u64;
typedef unsigned char u8;

constexpr int kJfStrip = 8;        // rows per wave in the pack pass (row y + 1's words are carried to the next row)
constexpr int kJfMaxRadius = 64;   // one neighbour word each side covers the widening

// step[j] = k(j-1) - k(j) for j = 1..r, k(j) = floor(sqrt(r^2 - j^2)): what the folded rows are widened by before rows y -+ j join them
struct JfDisk { u8 step[kJfMaxRadius + 1]; };

struct JfRow { u64 s, a, sn, an; };   // void-masked seg / ann word of one row, and the bit of the column after the word (0 or 1)

__device__ __forceinline__ JfRow jf_load_row(const u8* __restrict__ seg, const u8* __restrict__ ann, const u8* __restrict__ vd, size_t row_off, int x0, int w, int lane,
                                             bool in_frame) {
    bool ps = false, pa = false, qs = false, qa = false;
    const int x = x0 + lane;
    if (in_frame && x < w) {
        const size_t o = row_off + (size_t)x;
        const bool keep = !(vd && vd[o]);
        ps = keep && seg[o];
        pa = keep && ann[o];
    }
    if (in_frame && lane == 0 && x0 + 64 < w) {
        const size_t o = row_off + (size_t)(x0 + 64);
        const bool keep = !(vd && vd[o]);
        qs = keep && seg[o];
        qa = keep && ann[o];
    }
    JfRow r;
    r.s = __ballot(ps);
    r.a = __ballot(pa);
    r.sn = __ballot(qs) & 1ull;
    r.an = __ballot(qa) & 1ull;
    return r;
}

// _seg2bmap on words: b = (m^E) | (m^S) | (m^SE); the last row is m^E only, the last column m^S only, the bottom-right pixel 0
__device__ __forceinline__ u64 jf_boundary(u64 m0, u64 n0, u64 m1, u64 n1, bool last_row, u64 last_col) {
    const u64 e0 = (m0 >> 1) | (n0 << 63), e1 = (m1 >> 1) | (n1 << 63);
    const u64 b = last_row ? (m0 ^ e0) : ((m0 ^ e0) | (m0 ^ m1) | (m0 ^ e1));
    const u64 c = last_row ? 0ull : (m0 ^ m1);
    return (b & ~last_col) | (c & last_col);
}

__global__ __launch_bounds__(256) void jf_pack_kernel(const u8* __restrict__ seg, const u8* __restrict__ ann, const u8* __restrict__ vd, u64* __restrict__ bseg,
                                                      u64* __restrict__ bann, u64* __restrict__ counts, int h, int w, int w64, int items) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
    if (item >= items) return;
    const int t = blockIdx.y, wx = item % w64, y0 = (item / w64) * kJfStrip, x0 = wx * 64;
    const int y1 = min(y0 + kJfStrip, h);
    const u64 last_col = (wx == w64 - 1) ? (1ull << ((w - 1) & 63)) : 0ull;
    const size_t frame = (size_t)t * (size_t)h;
    u64 n_fg = 0, n_gt = 0, inter = 0, uni = 0;
    JfRow cur = jf_load_row(seg, ann, vd, (frame + y0) * (size_t)w, x0, w, lane, true);
    for (int y = y0; y < y1; ++y) {
        const bool last_row = y == h - 1;
        const JfRow nxt = jf_load_row(seg, ann, vd, (frame + y + 1) * (size_t)w, x0, w, lane, !last_row);
        const u64 bs = jf_boundary(cur.s, cur.sn, nxt.s, nxt.sn, last_row, last_col);
        const u64 ba = jf_boundary(cur.a, cur.an, nxt.a, nxt.an, last_row, last_col);
        if (lane == 0) {
            const size_t o = (frame + y) * (size_t)w64 + wx;
            bseg[o] = bs;
            bann[o] = ba;
        }
        n_fg += __popcll(bs);
        n_gt += __popcll(ba);
        inter += __popcll(cur.s & cur.a);
        uni += __popcll(cur.s | cur.a);
        cur = nxt;
    }
    if (lane == 0) {
        u64* c = counts + (size_t)t * 6;
        if (n_fg) atomicAdd(c + 0, n_fg);
        if (n_gt) atomicAdd(c + 1, n_gt);
        if (inter) atomicAdd(c + 4, inter);
        if (uni) atomicAdd(c + 5, uni);
    }
}

struct JfWin { u64 l, c, r; };   // a word and its two neighbours in the row (zero outside the row)

__device__ __forceinline__ void jf_or_row(JfWin& z, const u64* __restrict__ row, int wx, int w64) {
    if (wx > 0) z.l |= row[wx - 1];
    z.c |= row[wx];
    if (wx + 1 < w64) z.r |= row[wx + 1];
}

// z |= z shifted by every amount in [-d, d], d <= 64.  A window that covers shifts [-cov, cov] ORed with itself shifted by -+s covers [-(cov + s), cov + s] without
// a gap while s <= 2 cov + 1, so the cover triples per step: s = 1, 3, 9, 27, then the rest (always within 1..27: plain 64-bit shifts).
__device__ __forceinline__ void jf_widen(JfWin& z, int d) {
    int cov = 0;
    while (cov < d) {
        const int s = min(2 * cov + 1, d - cov), n = 64 - s;
        const u64 l = z.l, c = z.c, r = z.r;
        z.l = l | (l << s) | (l >> s) | (c << n);
        z.c = c | (c << s) | (l >> n) | (c >> s) | (r << n);
        z.r = r | (r << s) | (c >> n) | (r >> s);
        cov += s;
    }
}

__global__ __launch_bounds__(256) void jf_match_kernel(const u64* __restrict__ bseg, const u64* __restrict__ bann, u64* __restrict__ counts, int h, int w64, int radius,
                                                       JfDisk disk) {
    const int idx = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    int fg = 0, gt = 0;
    if (idx < h * w64) {
        const int y = idx / w64, wx = idx % w64;
        const size_t frame = (size_t)t * (size_t)h * (size_t)w64;
        const u64* fs = bseg + frame;
        const u64* fa = bann + frame;
        const u64 bs = fs[(size_t)y * w64 + wx], ba = fa[(size_t)y * w64 + wx];
        if (bs | ba) {
            // the dilated ground truth is needed only where the prediction has boundary pixels, and the other way round
            const bool need_a = bs != 0, need_s = ba != 0;
            JfWin za = {0, 0, 0}, zs = {0, 0, 0};
            if (need_a) jf_or_row(za, fa + (size_t)y * w64, wx, w64);
            if (need_s) jf_or_row(zs, fs + (size_t)y * w64, wx, w64);
            for (int j = 1; j <= radius; ++j) {
                const int d = disk.step[j];
                if (d) {
                    if (need_a) jf_widen(za, d);
                    if (need_s) jf_widen(zs, d);
                }
                if (y - j >= 0) {
                    if (need_a) jf_or_row(za, fa + (size_t)(y - j) * w64, wx, w64);
                    if (need_s) jf_or_row(zs, fs + (size_t)(y - j) * w64, wx, w64);
                }
                if (y + j < h) {
                    if (need_a) jf_or_row(za, fa + (size_t)(y + j) * w64, wx, w64);
                    if (need_s) jf_or_row(zs, fs + (size_t)(y + j) * w64, wx, w64);
                }
            }
            fg = __popcll(bs & za.c);
            gt = __popcll(ba & zs.c);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        fg += __shfl_xor(fg, o, 64);
        gt += __shfl_xor(gt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        u64* c = counts + (size_t)t * 6;
        if (fg) atomicAdd(c + 2, (u64)fg);
        if (gt) atomicAdd(c + 3, (u64)gt);
    }
}

// frames / h / w the kernels' 32-bit indices and the launch grid hold
static bool jf_shape_ok(int64_t frames, int64_t h, int64_t w) {
    if (frames <= 0 || h <= 0 || w <= 0 || frames > 65535 || h > (1 << 24) || w > (1 << 24)) return false;
    return h * cdiv(w, 64) < (1ll << 31) - 256;
}

}  // namespace rga3

using namespace rga3;

extern "C" int64_t rga3_mask_jf_ws_bytes(int64_t frames, int64_t h, int64_t w) {
    if (!jf_shape_ok(frames, h, w)) return fail(RGA3_EINVAL, "mask_jf_ws_bytes: bad shape [%ld, %ld, %ld]", (long)frames, (long)h, (long)w);
    return 2 * frames * h * cdiv(w, 64) * (int64_t)sizeof(u64);
}

extern "C" int rga3_mask_jf_counts(const void* seg, const void* ann, const void* void_pixels, int64_t* counts, void* ws, int64_t ws_bytes, int64_t frames, int64_t h,
                                   int64_t w, int radius, void* stream) {
    RGA3_CHECK_ARG(seg && ann && counts && ws, "mask_jf_counts: null pointer");
    RGA3_CHECK_ARG(jf_shape_ok(frames, h, w), "mask_jf_counts: bad shape [%ld, %ld, %ld] (non-empty, <= 65535 frames)", (long)frames, (long)h, (long)w);
    RGA3_CHECK_ARG(radius >= 1 && radius <= kJfMaxRadius, "mask_jf_counts: radius %d (1..%d)", radius, kJfMaxRadius);
    const int64_t w64 = cdiv(w, 64), words = frames * h * w64;
    RGA3_CHECK_ARG(ws_bytes >= 2 * words * (int64_t)sizeof(u64) && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)counts & 7) == 0,
                   "mask_jf_counts: workspace of rga3_mask_jf_ws_bytes() bytes needed (8-byte aligned)");
    JfDisk disk = {};
    int prev = radius;   // k(0)
    for (int j = 1; j <= radius; ++j) {
        int k = prev;
        while (k * k > radius * radius - j * j) --k;
        disk.step[j] = (u8)(prev - k);
        prev = k;
    }
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int64_t) * 6 * frames, (hipStream_t)stream);
    if (e != hipSuccess) return fail(-(int)e, "mask_jf_counts: memset: %s", hipGetErrorString(e));
    u64* bseg = (u64*)ws;
    u64* bann = bseg + words;
    const int64_t items = cdiv(h, kJfStrip) * w64;
    hipLaunchKernelGGL(jf_pack_kernel, dim3((unsigned)cdiv(items, 4), (unsigned)frames), dim3(256), 0, (hipStream_t)stream, (const u8*)seg, (const u8*)ann,
                       (const u8*)void_pixels, bseg, bann, (u64*)counts, (int)h, (int)w, (int)w64, (int)items);
    RGA3_CHECK_LAUNCH("mask_jf_counts (pack)");
    hipLaunchKernelGGL(jf_match_kernel, dim3((unsigned)cdiv(h * w64, 256), (unsigned)frames), dim3(256), 0, (hipStream_t)stream, (const u64*)bseg, (const u64*)bann,
                       (u64*)counts, (int)h, (int)w64, radius, disk);
    RGA3_CHECK_LAUNCH("mask_jf_counts (match)");
    return 0;
}
