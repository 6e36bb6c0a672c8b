// Head of an inference frame whose inputs are 8-bit images (label_nc == 0 recipes: pose2body, edge2face), ONE launch
// (v2v_image_prologue).  The input window is uint8 HWC, [N][T][H][W][Cin], oldest frame first; the loader's value transforms
// (ToTensor + Normalize, data/base_dataset.py:148-157; the DensePose part-index rescale, data/pose_dataset.py:44) are per-byte
// functions, so a table lut[Cin][256] of fp32 values reproduces them bit for bit.  The launch writes
//   x0        NHWC activation dtype [N][H][W][c_stride]: channel t * Cin + c = lut[c][win[n][t][y][x][c]], converted as
//             pack_nchw_to_nhwc_kernel converts, pad channels zero -- the generator's stem input;
//   real_last planar fp32 [N][Cin][H][W]: the newest frame as x0 holds it, i.e. v2v_unpack_nhwc_to_nchw of its channels -- the decoded
//             values, rounded to bf16 in a bf16 engine as the fp32-input path returns them (real_A[0][0, -1], vid2vid_model_G.py:209);
//   packed / last (with `window`): the previous-frame window pack of the label frame head (window_pack_item, layout_vec.h);
// and, on `advance`, moves the window on by one frame (win[n][t] <- win[n][t + 1], t < T - 1; slot T - 1 is left for the next
// newest frame), so that a caller stages only that frame per call.
//
// A workgroup owns a run of R consecutive pixels of one sample.  Their bytes are contiguous inside every frame: each frame's piece
// (R Cin bytes) is staged into LDS by 16-byte loads of the aligned granules that cover it (what a granule holds of neighbouring
// pixels is never used), at the same offset inside a granule as in global memory.  The table is in LDS too (Cin <= 32: 32 KB).
// From there: the NHWC row of the run is contiguous -- one 16-byte store per thread, consecutive threads on consecutive
// addresses; real_last is written per channel by consecutive threads on consecutive pixels; the window advance stores back,
// from LDS, only bytes of the workgroup's own pixels (16-byte stores for the granules that lie inside the piece where a frame is a
// multiple of 16 bytes, so that both frames' pieces share an alignment; single bytes at the piece's ends and otherwise), behind
// the barrier that ends the staging: no workgroup reads a byte another one writes and goes on to use it.
//
// Stream slots and the stream pool (v2v_image_prologue_slots): the frame plan's per-call words, int32 [N] in device
// memory, are loaded once per workgroup when the launch runs (blockIdx.y is the row: wave-uniform) and branched on, as
// frame_prologue_pool_kernel loads its row_slot.  slot_mode[n] == 2 (idle) skips the advance of row n: no byte of its input
// window is written, its dense outputs are still written from the unchanged window.  With S_win > 0 `win` is the pool
// [S_win][T][H][W][Cin] and row n works, in place, on win[row_slot[n]]; with S_window > 0 `window` is the pool
// [S_window][win_C][H][W] and row n packs window[row_slot[n]].  A row whose word is outside a pool returns before it reads or
// writes anything.  Distinct words keep the ownership rule above: a workgroup writes bytes of its own pixels of its own slot.
#include "v2v_internal.h"
#include "layout_vec.h"

namespace v2v {

struct ImagePrologueArgs {
    unsigned char* win; const float* lut; void* x0; float* real_last;
    const float* window; void* packed; float* last;
    int N, T, H, W, Cin, c_stride, win_C, win_c_stride, last_C;
    int advance, R, frame_lds;           // R: pixels per run; frame_lds: bytes of LDS per staged frame piece (multiple of 16)
    const int* slot_mode; const int* row_slot;     // the plan's words (null: every row advances / row n is slot n)
    int S_win, S_window;                 // > 0: win / window is a pool of that many slots, reached through row_slot
};

static constexpr int IMAGE_PROLOGUE_MAX_CIN = 32;
static constexpr int IMAGE_PROLOGUE_LDS = 64 * 1024;

template <typename T>
__global__ __launch_bounds__(256) void image_prologue_kernel(const ImagePrologueArgs a) {
    constexpr int VEC = ElemTraits<T>::VEC;
    extern __shared__ uint4 lds_raw[];
    float* const tab = reinterpret_cast<float*>(lds_raw);                              // [Cin][256]
    unsigned char* const stage = reinterpret_cast<unsigned char*>(lds_raw) + (size_t)a.Cin * 1024;   // [T][frame_lds]
    const int tid = threadIdx.x;
    const long long n = blockIdx.y;
    const long long slot = a.row_slot ? a.row_slot[n] : n;
    if ((a.S_win > 0 && (slot < 0 || slot >= a.S_win)) || (a.S_window > 0 && (slot < 0 || slot >= a.S_window))) return;
    const bool advance = a.advance && !(a.slot_mode && a.slot_mode[n] == 2);
    const long long wn = a.S_win > 0 ? slot : n;                                       // this row's input window
    const long long hw = (long long)a.H * a.W;
    const long long frame_bytes = hw * a.Cin;
    const long long total_bytes = (long long)(a.S_win > 0 ? a.S_win : a.N) * a.T * frame_bytes;
    const bool same_align = (frame_bytes & 15) == 0;
    const int vpr = a.c_stride / VEC;
    const int wvpr = a.window ? a.win_c_stride / VEC : 0;
    T* const x0 = reinterpret_cast<T*>(a.x0) + n * hw * a.c_stride;
    float* const real_last = a.real_last + n * a.Cin * hw;
    const float* const window = a.window ? a.window + (a.S_window > 0 ? slot : n) * a.win_C * hw : nullptr;
    T* const packed = a.packed ? reinterpret_cast<T*>(a.packed) + n * hw * a.win_c_stride : nullptr;
    float* const last = a.last ? a.last + n * a.last_C * hw : nullptr;

    for (int i = tid; i < a.Cin * 64; i += 256)
        reinterpret_cast<float4*>(tab)[i] = reinterpret_cast<const float4*>(a.lut)[i];

    const long long runs = (hw + a.R - 1) / a.R;
    for (long long run = blockIdx.x; run < runs; run += gridDim.x) {
        const long long p0 = run * a.R;
        const int npix = (int)((hw - p0) < a.R ? (hw - p0) : a.R);
        const int len = npix * a.Cin;                                   // bytes of one frame's piece
        const long long piece0 = wn * a.T * frame_bytes + p0 * a.Cin;    // byte offset of frame 0's piece; frame t's: + t frame_bytes
        // ---- stage: the aligned 16-byte granules that cover each frame's piece
        const int gmax = (len + 15 + 15) / 16;                          // granules of a piece at the worst alignment
        for (int i = tid; i < a.T * gmax; i += 256) {
            const int t = i / gmax, k = i - t * gmax;
            const long long start = piece0 + t * frame_bytes;
            const long long g = (start & ~15ll) + 16ll * k;
            if (g >= start + len) continue;
            unsigned char* dst = stage + t * a.frame_lds + 16 * k;
            if (g + 16 <= total_bytes) {
                *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(a.win + g);
            } else {                                                     // the buffer ends inside this granule
                for (int b = 0; b < 16 && g + b < total_bytes; ++b) dst[b] = a.win[g + b];
            }
        }
        __syncthreads();
        // ---- x0: one 16-byte channel vector per thread, consecutive threads on consecutive addresses of the run's NHWC row
        for (int v = tid; v < npix * vpr; v += 256) {
            const int pix = v / vpr, cv = v - pix * vpr;
            int ch = cv * VEC;
            int t = ch / a.Cin, c = ch - t * a.Cin;
            float vals[VEC];
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                float val = 0.f;
                if (t < a.T) {
                    const int off = (int)((piece0 + t * frame_bytes) & 15);
                    val = tab[c * 256 + stage[t * a.frame_lds + off + pix * a.Cin + c]];
                }
                vals[q] = val;
                if (++c == a.Cin) { c = 0; ++t; }
            }
            store_vec(x0, (p0 + pix) * a.c_stride + cv * VEC, vals);
        }
        // ---- real_last: the newest frame, planar: consecutive threads on consecutive pixels of one channel
        {
            const unsigned char* newest = stage + (a.T - 1) * a.frame_lds + (int)((piece0 + (a.T - 1) * frame_bytes) & 15);
            for (int i = tid; i < npix * a.Cin; i += 256) {
                const int c = i / npix, pix = i - c * npix;
                float v = tab[c * 256 + newest[pix * a.Cin + c]];
                if constexpr (ElemTraits<T>::DTYPE == V2V_BF16) v = bf16_bits_to_f32(f32_to_bf16_bits(v));     // the value x0 holds
                real_last[c * hw + p0 + pix] = v;
            }
        }
        // ---- the previous-frame window pack of the label frame head, on this run's pixels
        for (int i = tid; i < npix * wvpr; i += 256) {
            const int cv = i / npix, pix = i - cv * npix;
            window_pack_item<T>(window, packed, last, p0 + pix, cv, hw, a.win_C, a.win_c_stride, a.last_C);
        }
        // ---- advance: frame t's piece <- frame t + 1's, from LDS; only bytes of this run's pixels are written
        if (advance) {
            for (int t = 0; t + 1 < a.T; ++t) {
                const long long dst0 = piece0 + t * frame_bytes;
                const unsigned char* src = stage + (t + 1) * a.frame_lds;
                const int soff = (int)((dst0 + frame_bytes) & 15);
                if (same_align) {                                       // soff is the destination's offset inside a granule too
                    const long long g0 = dst0 & ~15ll;
                    const int ng = (soff + len + 15) / 16;
                    for (int k = tid; k < ng; k += 256) {
                        const long long g = g0 + 16ll * k;
                        if (g >= dst0 && g + 16 <= dst0 + len) {
                            *reinterpret_cast<uint4*>(a.win + g) = *reinterpret_cast<const uint4*>(src + 16 * k);
                        } else {
                            for (int b = 0; b < 16; ++b)
                                if (g + b >= dst0 && g + b < dst0 + len) a.win[g + b] = src[16 * k + b];
                        }
                    }
                } else {
                    for (int b = tid; b < len; b += 256) a.win[dst0 + b] = src[soff + b];
                }
            }
        }
        __syncthreads();                                                 // the next run's staging overwrites the pieces
    }
}

struct ImagePrologueOp : Op {
    ImagePrologueArgs a; int dtype; unsigned lds;
    int launch(hipStream_t s) override {
        const long long runs = ceil_div((long long)a.H * a.W, a.R);
        // every workgroup fills its own copy of the table: few workgroups per CU, the runs behind them by grid stride
        long long gx = 512 / a.N;
        if (gx < 1) gx = 1;
        if (gx > runs) gx = runs;
        const dim3 g((unsigned)gx, (unsigned)a.N), b(256);
        if (dtype == V2V_BF16) hipLaunchKernelGGL(image_prologue_kernel<bf16_t>, g, b, lds, s, a);
        else                   hipLaunchKernelGGL(image_prologue_kernel<float>, g, b, lds, s, a);
        return check_launch();
    }
    const char* name() const override { return "image_prologue"; }
};

static bool ranges_overlap(const void* p, long long pb, const void* q, long long qb) {
    const char* a = (const char*)p; const char* b = (const char*)q;
    return p && q && a < b + qb && b < a + pb;
}

}  // namespace v2v

using namespace v2v;

extern "C" int v2v_image_prologue_slots(uint8_t* win, const float* lut, int32_t advance, void* x0, int32_t c_stride, float* real_last,
                                        int32_t N, int32_t T, int32_t H, int32_t W, int32_t Cin, const float* window, int32_t win_C,
                                        void* packed, int32_t win_c_stride, float* last, int32_t last_C, int32_t dtype, void* stream,
                                        const int32_t* slot_mode, const int32_t* row_slot, int32_t S_win, int32_t S_window) {
    if (!win || !lut || !x0 || !real_last) { set_error("image_prologue: null pointer"); return V2V_EINVAL; }
    if (dtype != V2V_F32 && dtype != V2V_BF16) { set_error("image_prologue: bad dtype %d", dtype); return V2V_EINVAL; }
    const int vec = dtype == V2V_BF16 ? 8 : 4;
    const int esize = dtype == V2V_BF16 ? 2 : 4;
    if (Cin < 1 || Cin > IMAGE_PROLOGUE_MAX_CIN) {
        set_error("image_prologue: %d input channels (the table of 1..%d channels is held in LDS)", Cin, IMAGE_PROLOGUE_MAX_CIN);
        return V2V_EINVAL;
    }
    if (N < 1 || N > 65535 || T < 1 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffll / Cin || c_stride % vec != 0 ||
        (long long)T * Cin > c_stride || (((uintptr_t)win | (uintptr_t)lut | (uintptr_t)x0) & 15) != 0 || ((uintptr_t)real_last & 3) != 0) {
        set_error("image_prologue: bad argument (win, lut and x0 16-byte aligned, T Cin <= c_stride)"); return V2V_EINVAL;
    }
    if (window && (!packed || win_C < 1 || win_c_stride % vec != 0 || win_C > win_c_stride || ((uintptr_t)packed & 15) != 0 ||
                   ((uintptr_t)window & 3) != 0 || (last && (last_C < 1 || last_C > win_C)))) {
        set_error("image_prologue: bad window pack argument"); return V2V_EINVAL;
    }
    if (S_win < 0 || S_window < 0 || (S_win > 0 && S_win < N) || (S_window > 0 && (S_window < N || !window)) ||
        ((S_win > 0 || S_window > 0) != (row_slot != nullptr))) {
        set_error("image_prologue: bad pool argument (a pool of S >= N slots goes with row_slot, row_slot with a pool)"); return V2V_EINVAL;
    }
    const long long hw = (long long)H * W;
    const long long win_bytes = (long long)(S_win > 0 ? S_win : N) * T * hw * Cin;               // the whole pool
    const long long window_bytes = window ? (long long)(S_window > 0 ? S_window : N) * win_C * hw * 4 : 0;
    if (ranges_overlap(win, win_bytes, x0, N * hw * c_stride * esize) || ranges_overlap(win, win_bytes, real_last, N * hw * Cin * 4) ||
        ranges_overlap(win, win_bytes, lut, Cin * 1024ll) || ranges_overlap(win, win_bytes, window, window_bytes) ||
        ranges_overlap(win, win_bytes, slot_mode, N * 4ll) || ranges_overlap(win, win_bytes, row_slot, N * 4ll) ||
        ranges_overlap(x0, N * hw * c_stride * esize, real_last, N * hw * Cin * 4) ||
        (window && (ranges_overlap(win, win_bytes, packed, N * hw * win_c_stride * esize) ||
                    ranges_overlap(win, win_bytes, last, N * hw * (long long)last_C * 4)))) {
        set_error("image_prologue: buffers overlap"); return V2V_EINVAL;
    }
    // the longest run (256, 128 or 64 pixels) whose T staged pieces fit beside the table
    int R = 256;
    auto frame_lds = [&](int r) { return (int)round_up((long long)r * Cin + 32, 16); };
    while (R > 64 && Cin * 1024ll + (long long)T * frame_lds(R) > IMAGE_PROLOGUE_LDS) R /= 2;
    const long long lds = Cin * 1024ll + (long long)T * frame_lds(R);
    if (lds > IMAGE_PROLOGUE_LDS) { set_error("image_prologue: %d frames of %d channels do not fit in LDS", T, Cin); return V2V_EINVAL; }
    auto op = std::make_unique<ImagePrologueOp>();
    op->a = ImagePrologueArgs{win, lut, x0, real_last, window, window ? packed : nullptr, window ? last : nullptr,
                              N, T, H, W, Cin, c_stride, window ? win_C : 0, window ? win_c_stride : 0, window ? last_C : 0,
                              advance ? 1 : 0, R, frame_lds(R), slot_mode, row_slot, S_win, S_window};
    op->dtype = dtype; op->lds = (unsigned)lds;
    return submit(std::move(op), stream);
}

extern "C" int v2v_image_prologue(uint8_t* win, const float* lut, int32_t advance, void* x0, int32_t c_stride, float* real_last,
                                  int32_t N, int32_t T, int32_t H, int32_t W, int32_t Cin, const float* window, int32_t win_C,
                                  void* packed, int32_t win_c_stride, float* last, int32_t last_C, int32_t dtype, void* stream) {
    return v2v_image_prologue_slots(win, lut, advance, x0, c_stride, real_last, N, T, H, W, Cin, window, win_C, packed, win_c_stride,
                                    last, last_C, dtype, stream, nullptr, nullptr, 0, 0);
}
