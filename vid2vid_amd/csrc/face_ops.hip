// Face discriminator window (--add_face_disc, the pose2body recipes): the data-dependent crop of
// Vid2VidModelD.get_face_region (models/vid2vid_model_D.py:215-230) computed and consumed on the device.
//
//   v2v_face_window              mask -> bounding box over all frames -> clamped fixed-size window, written to a
//                                caller-owned int32[8] {found, ys, ye, xs, xe, -, -, -}; three small launches
//                                (reset, reduce, finalize), no host synchronisation, graph-capturable
//   v2v_pack_concat_window_nhwc  cat([x0, x1], 1)[:, :, ys:ye, xs:xe] of planar fp32 -> NHWC engine dtype
//                                (the windowed twin of v2v_pack_concat_nhwc), window origin read on the device
//   v2v_unpack_window_nchw       backward of the x1 operand: channel slice inside the window, zeros outside, one pass
//
// Every launch writes with ordinary vector stores / vector atomics only.
#include "v2v_internal.h"
#include <climits>

namespace v2v {

static inline unsigned face_grid(long long n, int threads = 256, long long cap = 4096) {
    long long b = ceil_div(n, threads);
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// win[] word layout (include/v2v_hip.h V2V_FACE_WIN_*): the reduce step accumulates the inclusive box in words 1..4
// (y min, y max, x min, x max); the finalize step turns them into the window in place and writes word 0 (found).
enum { W_FOUND = 0, W_YS = 1, W_YE = 2, W_XS = 3, W_XE = 4 };

// ---- step 1: reset the accumulators (one wave).  Part of every call: nothing of an earlier call or shape is read.
__global__ __launch_bounds__(64) void face_window_reset_kernel(int32_t* win) {
    const int t = threadIdx.x;
    if (t < 8) {
        int32_t v = 0;
        if (t == W_YS || t == W_XS) v = INT_MAX;      // min accumulators
        else if (t == W_YE || t == W_XE) v = -1;      // max accumulators (-1: nothing found)
        win[t] = v;
    }
}

__device__ __forceinline__ bool face_pixel(const float* a, long long plane, long long pix, int mode) {
    // thresholds are fp32 constants: torch compares an fp32 tensor with a Python scalar in fp32
    const float c2 = a[2 * plane + pix];
    if (mode == V2V_FACE_DENSEPOSE) return c2 > 0.9f;
    const float c0 = a[pix], c1 = a[plane + pix];
    return c0 > 0.19f && c0 < 0.21f && c1 < -0.99f && c2 > -0.61f && c2 < -0.59f;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

struct FaceReduceArgs { const float* a; int32_t* win; int N, C, H, W, mode; };

// ---- step 2: grid-stride pass over the N mask planes; min / max inside each wave, then inside the workgroup (LDS),
// then one global atomic per accumulator per workgroup (integer min / max: the result does not depend on the order)
__global__ __launch_bounds__(256) void face_window_reduce_kernel(const FaceReduceArgs a) {
    const long long hw = (long long)a.H * a.W;
    const long long total = (long long)a.N * hw;
    const long long stride = (long long)gridDim.x * blockDim.x;
    int ymin = INT_MAX, ymax = -1, xmin = INT_MAX, xmax = -1;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const long long n = p / hw, pix = p - n * hw;
        if (face_pixel(a.a + n * a.C * hw, hw, pix, a.mode)) {
            const int y = (int)(pix / a.W), x = (int)(pix - (long long)y * a.W);
            ymin = min(ymin, y); ymax = max(ymax, y);
            xmin = min(xmin, x); xmax = max(xmax, x);
        }
    }
    ymin = wave_min(ymin); ymax = wave_max(ymax); xmin = wave_min(xmin); xmax = wave_max(xmax);
    __shared__ int part[4][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { part[wave][0] = ymin; part[wave][1] = ymax; part[wave][2] = xmin; part[wave][3] = xmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int w = 1; w < nw; ++w) {
            ymin = min(ymin, part[w][0]); ymax = max(ymax, part[w][1]);
            xmin = min(xmin, part[w][2]); xmax = max(xmax, part[w][3]);
        }
        if (ymax >= 0) {                               // this workgroup saw face pixels
            atomicMin(a.win + W_YS, ymin); atomicMax(a.win + W_YE, ymax);
            atomicMin(a.win + W_XS, xmin); atomicMax(a.win + W_XE, xmax);
        }
    }
}

// ---- step 3: box -> window, the reference's integer arithmetic (:223-228).  All operands are >= 0 where Python's //
// is used on them (crop <= H, W is validated), so C division gives the same results.
__global__ __launch_bounds__(64) void face_window_finalize_kernel(int32_t* win, int H, int W, int crop_h, int crop_w) {
    if (threadIdx.x != 0) return;
    const int ys0 = win[W_YS], ye0 = win[W_YE], xs0 = win[W_XS], xe0 = win[W_XE];
    const int found = ye0 >= 0 ? 1 : 0;
    int yc = crop_h / 2, xc = crop_w / 2;              // no face: the top-left window (in bounds, never used for a loss)
    if (found) {
        yc = (ys0 + ye0) / 2;
        xc = (xs0 + xe0) / 2;
        yc = max(crop_h / 2, min(H - 1 - crop_h / 2, yc));
        xc = max(crop_w / 2, min(W - 1 - crop_w / 2, xc));
    }
    win[W_YS] = yc - crop_h / 2; win[W_YE] = yc + crop_h / 2;
    win[W_XS] = xc - crop_w / 2; win[W_XE] = xc + crop_w / 2;
    win[W_FOUND] = found;
}

struct FaceWindowOp : Op {
    FaceReduceArgs a; int crop_h, crop_w;
    int launch(hipStream_t s) override {
        hipLaunchKernelGGL(face_window_reset_kernel, dim3(1), dim3(64), 0, s, a.win);
        const long long total = (long long)a.N * a.H * a.W;
        hipLaunchKernelGGL(face_window_reduce_kernel, dim3(face_grid(total, 256, 1024)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(face_window_finalize_kernel, dim3(1), dim3(64), 0, s, a.win, a.H, a.W, crop_h, crop_w);
        return check_launch();
    }
    const char* name() const override { return "face_window"; }
};

// window origin as the consumers read it: clamped into the frame so that a window word that is not a window (a buffer
// never written by v2v_face_window) cannot send a load or store out of bounds.  Valid windows pass unchanged.
__device__ __forceinline__ void window_origin(const int32_t* win, int H, int W, int crop_h, int crop_w, int& ys, int& xs) {
    ys = min(max(win[W_YS], 0), H - crop_h);
    xs = min(max(win[W_XS], 0), W - crop_w);
}

__device__ __forceinline__ void store_vec_w(bf16_t* y, long long e, const float (&v)[8]) {
    uint4 pk;
    pk.x = pack_bf16x2(v[0], v[1]); pk.y = pack_bf16x2(v[2], v[3]); pk.z = pack_bf16x2(v[4], v[5]); pk.w = pack_bf16x2(v[6], v[7]);
    *reinterpret_cast<uint4*>(y + e) = pk;
}
__device__ __forceinline__ void store_vec_w(float* y, long long e, const float (&v)[4]) {
    *reinterpret_cast<float4*>(y + e) = make_float4(v[0], v[1], v[2], v[3]);
}

struct PackWinArgs { const float* x0; const float* x1; const int32_t* win; void* y; int N, C0, C1, H, W, crop_h, crop_w, c_stride; };

// cat([x0, x1], 1)[:, :, ys:ys+crop_h, xs:xs+crop_w] -> NHWC [N][crop_h][crop_w][c_stride], padding channels zero
template <typename T>
__global__ __launch_bounds__(256) void pack_concat_window_kernel(const PackWinArgs a) {
    constexpr int VEC = ElemTraits<T>::VEC;
    int ys, xs;
    window_origin(a.win, a.H, a.W, a.crop_h, a.crop_w, ys, xs);
    const int vpr = a.c_stride / VEC;
    const long long hw = (long long)a.H * a.W;
    const long long chw = (long long)a.crop_h * a.crop_w;
    const long long npix = (long long)a.N * chw;
    const long long nvec = npix * vpr;
    const long long stride = (long long)gridDim.x * blockDim.x;
    T* y = reinterpret_cast<T*>(a.y);
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
        const long long pixg = v % npix;
        const int cv = (int)(v / npix);
        const long long n = pixg / chw;
        const int r = (int)(pixg - n * chw);
        const int oy = r / a.crop_w, ox = r - oy * a.crop_w;
        const long long pix = (long long)(ys + oy) * a.W + (xs + ox);
        float vals[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            const int c = cv * VEC + q;
            float val = 0.f;
            if (c < a.C0) val = a.x0[(n * a.C0 + c) * hw + pix];
            else if (c < a.C0 + a.C1) val = a.x1[(n * a.C1 + (c - a.C0)) * hw + pix];
            vals[q] = val;
        }
        store_vec_w(y, pixg * a.c_stride + cv * VEC, vals);
    }
}

struct PackWinOp : Op {
    PackWinArgs a; int dtype;
    int launch(hipStream_t s) override {
        const int vec = dtype == V2V_BF16 ? 8 : 4;
        const long long n = (long long)a.N * a.crop_h * a.crop_w * (a.c_stride / vec);
        if (dtype == V2V_BF16) hipLaunchKernelGGL(pack_concat_window_kernel<bf16_t>, dim3(face_grid(n)), dim3(256), 0, s, a);
        else                   hipLaunchKernelGGL(pack_concat_window_kernel<float>, dim3(face_grid(n)), dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "pack_concat_window_nhwc"; }
};

struct UnpackWinArgs { const void* dy; const int32_t* win; float* dx; int N, C, H, W, crop_h, crop_w, c_stride, c_off; };

// dx[n][c][h][w] = dy[n][h-ys][w-xs][c_off + c] inside the window, 0 outside: the whole planar gradient in one pass
template <typename T>
__global__ __launch_bounds__(256) void unpack_window_kernel(const UnpackWinArgs a) {
    int ys, xs;
    window_origin(a.win, a.H, a.W, a.crop_h, a.crop_w, ys, xs);
    const long long hw = (long long)a.H * a.W;
    const long long total = (long long)a.N * a.C * hw;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const T* dy = reinterpret_cast<const T*>(a.dy);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const long long pix = e % hw;
        const long long nc = e / hw;
        const long long n = nc / a.C;
        const int c = (int)(nc - n * a.C);
        const int h = (int)(pix / a.W), w = (int)(pix - (long long)h * a.W);
        const int oy = h - ys, ox = w - xs;
        float v = 0.f;
        if (oy >= 0 && oy < a.crop_h && ox >= 0 && ox < a.crop_w)
            v = load_act(dy, ((n * a.crop_h + oy) * a.crop_w + ox) * a.c_stride + a.c_off + c);
        a.dx[e] = v;
    }
}

struct UnpackWinOp : Op {
    UnpackWinArgs a; int dtype;
    int launch(hipStream_t s) override {
        const long long n = (long long)a.N * a.C * a.H * a.W;
        if (dtype == V2V_BF16) hipLaunchKernelGGL(unpack_window_kernel<bf16_t>, dim3(face_grid(n)), dim3(256), 0, s, a);
        else                   hipLaunchKernelGGL(unpack_window_kernel<float>, dim3(face_grid(n)), dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "unpack_window_nchw"; }
};

static bool window_fits(int32_t H, int32_t W, int32_t crop_h, int32_t crop_w) {
    return H > 0 && W > 0 && crop_h > 0 && crop_w > 0 && crop_h % 2 == 0 && crop_w % 2 == 0 && crop_h <= H && crop_w <= W;
}

}  // namespace v2v

using namespace v2v;

extern "C" int v2v_face_window(const float* real_A, int32_t N, int32_t C, int32_t H, int32_t W, int32_t mode,
                               int32_t crop_h, int32_t crop_w, int32_t* win, void* stream) {
    if (!real_A || !win || N <= 0 || C < 3 || (mode != V2V_FACE_DENSEPOSE && mode != V2V_FACE_OPENPOSE) ||
        !window_fits(H, W, crop_h, crop_w)) {
        set_error("face_window: bad argument"); return V2V_EINVAL;
    }
    auto op = std::make_unique<FaceWindowOp>();
    op->a = FaceReduceArgs{real_A, win, N, C, H, W, mode}; op->crop_h = crop_h; op->crop_w = crop_w;
    return submit(std::move(op), stream);
}

extern "C" int v2v_pack_concat_window_nhwc(const float* x0, int32_t C0, const float* x1, int32_t C1, int32_t N, int32_t H,
                                           int32_t W, const int32_t* win, int32_t crop_h, int32_t crop_w, void* y,
                                           int32_t c_stride, int32_t dtype, void* stream) {
    const int vec = dtype == V2V_BF16 ? 8 : 4;
    if (!x0 || !y || !win || C0 <= 0 || C1 < 0 || (C1 > 0 && !x1) || N <= 0 || (dtype != V2V_F32 && dtype != V2V_BF16) ||
        c_stride % vec != 0 || C0 + C1 > c_stride || !window_fits(H, W, crop_h, crop_w)) {
        set_error("pack_concat_window: bad argument"); return V2V_EINVAL;
    }
    auto op = std::make_unique<PackWinOp>();
    op->a = PackWinArgs{x0, C1 > 0 ? x1 : nullptr, win, y, N, C0, C1, H, W, crop_h, crop_w, c_stride}; op->dtype = dtype;
    return submit(std::move(op), stream);
}

extern "C" int v2v_unpack_window_nchw(const void* dy, const int32_t* win, int32_t N, int32_t C, int32_t H, int32_t W,
                                      int32_t crop_h, int32_t crop_w, int32_t c_stride, int32_t c_offset, float* dx,
                                      int32_t dtype, void* stream) {
    if (!dy || !win || !dx || N <= 0 || C <= 0 || c_offset < 0 || c_offset + C > c_stride ||
        (dtype != V2V_F32 && dtype != V2V_BF16) || !window_fits(H, W, crop_h, crop_w)) {
        set_error("unpack_window: bad argument"); return V2V_EINVAL;
    }
    auto op = std::make_unique<UnpackWinOp>();
    op->a = UnpackWinArgs{dy, win, dx, N, C, H, W, crop_h, crop_w, c_stride, c_offset}; op->dtype = dtype;
    return submit(std::move(op), stream);
}
