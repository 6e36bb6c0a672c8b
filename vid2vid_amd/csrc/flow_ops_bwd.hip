// Backward passes of FlowNet2's three native ops (the forward passes are in flow_ops.hip).  Written from the maths of the
// reference kernels, wave64-native, planar fp32 NCHW like their forward siblings:
//   correlation   correlation_cuda_kernel.cu:150-241 (input1), :243-334 (input2); host side correlation_cuda.cc:89-167
//   resample2d    resample2d_kernel.cu:67-117 (input1 = image), :119-190 (input2 = flow); resample2d_cuda.cc:15-26
//   channelnorm   channelnorm_kernel.cu:63-96; channelnorm_cuda.cc:16-25
// The reference's correlation backward is a grid (H, W, C) of 32-thread blocks inside a host loop over the batch, each block
// reducing prod_sum[32] serially in thread 0, on zero-padded NHWC copies of the inputs; here padding is a bounds test, one lane
// owns whole output elements and sums them in a fixed order (gather form): no atomics, no scratch tensor, bit-identical runs.
#include "v2v_internal.h"

namespace v2v {

// ---- correlation backward ----
// Forward (flow_ops.hip), in the unpadded frame, with off = max_disp - pad, dj = (tj - drad) s2, di = (ti - drad) s2:
//   out[n][tj D + ti][oy][ox] = 1/(k^2 C) sum_{c, j, i in [-krad, krad]} in1[n][c][ya][xa] * in2[n][c][ya + dj][xa + di]
//   ya = oy s1 + off + j, xa = ox s1 + off + i; a product with an operand outside the image is zero.
// Let P[tc][y][x] = sum of grad_out[n][tc][oy][ox] over the (oy, j), (ox, i) with ya == y, xa == x (grad_out brought onto the grid of
// in1; for kernel 1 / stride1 1 / pad == max_disp it IS grad_out).  The adjoint is then
//   grad_in1[n][c][y][x] = 1/(k^2 C) sum_tc P[tc][y][x]           * in2[n][c][y + dj][x + di]
//   grad_in2[n][c][y][x] = 1/(k^2 C) sum_tc P[tc][y - dj][x - di] * in1[n][c][y - dj][x - di]
struct CorrBwdArgs {
    const float* in1; const float* in2; const float* gout; float* g1; float* g2;
    int N, C, H, W, OH, OW, D;
    int pad, ksize, krad, max_disp, s1, s2, drad;
};

// Generic parameter sets: thread = (gradient, n, chunk of CG_CH channels, y, x); P is summed once per displacement and used for the
// CG_CH channels.  Simple on purpose (no LDS): FlowNetC's class takes the tile kernel below.
constexpr int CG_CH = 8;

__device__ __forceinline__ float corr_bwd_P(const CorrBwdArgs& a, const float* g, int y, int x) {
    // g: grad_out plane [OH][OW] of one (n, tc)
    const int off = a.max_disp - a.pad;
    float p = 0.f;
    for (int j = -a.krad; j <= a.krad; ++j) {
        const int ty = y - j - off;
        if (ty < 0 || ty % a.s1 != 0) continue;
        const int oy = ty / a.s1;
        if (oy >= a.OH) continue;
        for (int i = -a.krad; i <= a.krad; ++i) {
            const int tx = x - i - off;
            if (tx < 0 || tx % a.s1 != 0) continue;
            const int ox = tx / a.s1;
            if (ox >= a.OW) continue;
            p += g[(long long)oy * a.OW + ox];
        }
    }
    return p;
}

// grid (ceil(W / 64), H, N * ceil(C / CG_CH) * 2), block 64; which = blockIdx.z & 1 (0: grad_in1, 1: grad_in2)
__global__ __launch_bounds__(64) void correlation_bwd_generic_kernel(const CorrBwdArgs a) {
    const int which = blockIdx.z & 1;
    float* const dst = which ? a.g2 : a.g1;
    if (!dst) return;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y;
    if (x >= a.W) return;
    const int chunks = (a.C + CG_CH - 1) / CG_CH;
    const int zz = blockIdx.z >> 1;
    const int n = zz / chunks, c0 = (zz - n * chunks) * CG_CH;
    const long long hw = (long long)a.H * a.W, ohw = (long long)a.OH * a.OW;
    const float* other = (which ? a.in1 : a.in2) + ((long long)n * a.C + c0) * hw;
    const float* gn = a.gout + (long long)n * a.D * a.D * ohw;
    float acc[CG_CH];
#pragma unroll
    for (int q = 0; q < CG_CH; ++q) acc[q] = 0.f;
    for (int tj = 0; tj < a.D; ++tj) {
        const int dj = (tj - a.drad) * a.s2;
        const int yo = which ? y - dj : y + dj;          // row of the other feature map
        if ((unsigned)yo >= (unsigned)a.H) continue;
        for (int ti = 0; ti < a.D; ++ti) {
            const int di = (ti - a.drad) * a.s2;
            const int xo = which ? x - di : x + di;
            if ((unsigned)xo >= (unsigned)a.W) continue;
            const float* g = gn + (long long)(tj * a.D + ti) * ohw;
            const float p = which ? corr_bwd_P(a, g, yo, xo) : corr_bwd_P(a, g, y, x);
            const float* o = other + (long long)yo * a.W + xo;
#pragma unroll
            for (int q = 0; q < CG_CH; ++q)
                if (c0 + q < a.C) acc[q] += p * o[q * hw];
        }
    }
    const float inv = 1.f / (float)(a.ksize * a.ksize * a.C);
#pragma unroll
    for (int q = 0; q < CG_CH; ++q)
        if (c0 + q < a.C) dst[((long long)n * a.C + c0 + q) * hw + (long long)y * a.W + x] = acc[q] * inv;
}

// FlowNetC's geometry class (kernel_size 1, stride1 1, stride2 2, pad == max_disp even, D <= 21: FlowNetC.py:31), where P == grad_out:
//   grad_in1[c][y][x] = (1/C) sum_{tj, ti} g[tj][ti][y][x]   * f2[c][y + 2(tj - drad)][x + 2(ti - drad)]
//   grad_in2[c][y][x] = (1/C) sum_{tj, ti} g[tj][ti][y'][x'] * f1[c][y'][x'],   y' = y - 2(tj - drad), x' = x - 2(ti - drad)
// One wave (= one workgroup) owns 32 pixels of a row x CB_CH = 64 channels of ONE gradient and keeps its 2048 outputs in registers:
// thread (strip, channel lane) holds 4 same-parity pixels (x, x+2, x+4, x+6) x 8 channels.  It walks the D displacement rows tj; per
// row it stages in LDS
//   * the row of the OTHER feature map that tj selects, 32 + 4 drad columns x 64 channels, columns split by parity so that the D taps
//     of a pixel are D consecutive floats (the layout of correlation_lds_kernel); padding is a zero written at staging time;
//   * the grad_out band of the row: [D][32 pixels] (grad_in1: the pixel's own column) or [D][32 + 4 drad columns] (grad_in2: grad_out
//     sits at the displaced position, like f1);
// then loads the 4 x D band values of its pixels into registers ONCE and reuses them for its 8 channels: per channel one aligned
// 24-float window (6 ds_read_b128) feeds 4 x D FMAs -- 3.5 FMAs per LDS float, the band reads amortised 8x.  grad_in2 is the same
// loop with the tap order reversed (x' = x + 2(ti' - drad), ti' = D - 1 - ti).  Vector ALU, not MFMA: as a matrix product the
// contraction index is the displacement, which sits in the densified band at 21 of 96 columns (v2v_correlation_nhwc pays that with
// bf16 rate; in fp32 it does not pay), and the operands here are planar.  Every output is written by exactly one lane, summed in a
// fixed order: bit-identical from run to run.
constexpr int CB_TX = 32, CB_CH = 64, CB_CPT = 8, CB_DMAX = 21, CB_HALF = 36, CB_THREADS = 64, CB_U = 8;

// grid (ceil(W / 32), H, N * ceil(C / 64) * 2), block 64
__global__ __launch_bounds__(CB_THREADS) void correlation_bwd_tile_kernel(const CorrBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float fs[CB_CH][2 * CB_HALF];          // 18 KB
    __shared__ __attribute__((aligned(16))) float gs[CB_DMAX][2 * CB_HALF];        //  6 KB (grad_in1 uses [ti][32])
    const int which = blockIdx.z & 1;
    float* const dst = which ? a.g2 : a.g1;
    if (!dst) return;
    const int tid = threadIdx.x;
    const int groups = (a.C + CB_CH - 1) / CB_CH;
    const int zz = blockIdx.z >> 1;
    const int n = zz / groups, c0 = (zz - n * groups) * CB_CH;
    const int y = blockIdx.y, x0 = blockIdx.x * CB_TX;
    const int D = a.D, drad = a.drad;
    const int ncols = CB_TX + 4 * drad;
    const long long hw = (long long)a.H * a.W;
    const float* other = (which ? a.in1 : a.in2) + (long long)n * a.C * hw;
    const float* gn = a.gout + (long long)n * D * D * hw;                           // OH == H, OW == W in this class
    const int strip = tid & 7, cl = tid >> 3;                                       // 8 strips x 8 channel lanes
    const int par = strip & 1, s4 = strip >> 1;                                     // pixels px_k = par + 8 s4 + 2k
    float acc[CB_CPT][4];
#pragma unroll
    for (int q = 0; q < CB_CPT; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[q][k] = 0.f;
    // D < 21: the windows reach past the staged columns; those entries meet a zero band value and must be finite
    for (int e = tid; e < CB_CH * 2 * CB_HALF; e += CB_THREADS) (&fs[0][0])[e] = 0.f;
    for (int e = tid; e < CB_DMAX * 2 * CB_HALF; e += CB_THREADS) (&gs[0][0])[e] = 0.f;

    for (int tj = 0; tj < D; ++tj) {
        const int yo = which ? y - 2 * (tj - drad) : y + 2 * (tj - drad);
        if ((unsigned)yo >= (unsigned)a.H) continue;                                // uniform: the whole row is padding
        __syncthreads();                                                            // previous row fully consumed
        // CB_U loads in flight per lane before the first LDS store (one wave per SIMD: nothing else hides the latency)
        for (int e0 = tid; e0 < CB_CH * ncols; e0 += CB_THREADS * CB_U) {
            float v[CB_U];
#pragma unroll
            for (int u = 0; u < CB_U; ++u) {
                const int e = e0 + u * CB_THREADS;
                const int c = e / ncols, xx = e - c * ncols;
                const int x = x0 - 2 * drad + xx;
                v[u] = 0.f;
                if (c < CB_CH && c0 + c < a.C && (unsigned)x < (unsigned)a.W) v[u] = other[(c0 + c) * hw + (long long)yo * a.W + x];
            }
#pragma unroll
            for (int u = 0; u < CB_U; ++u) {
                const int e = e0 + u * CB_THREADS;
                const int c = e / ncols, xx = e - c * ncols;
                if (c < CB_CH) fs[c][(xx & 1) * CB_HALF + (xx >> 1)] = v[u];
            }
        }
        if (which) {                                                                // band at the displaced position: row yo, all columns
            for (int e0 = tid; e0 < D * ncols; e0 += CB_THREADS * CB_U) {
                float v[CB_U];
#pragma unroll
                for (int u = 0; u < CB_U; ++u) {
                    const int e = e0 + u * CB_THREADS;
                    const int ti = e / ncols, xx = e - ti * ncols;
                    const int x = x0 - 2 * drad + xx;
                    v[u] = 0.f;
                    if (ti < D && (unsigned)x < (unsigned)a.W) v[u] = gn[(long long)(tj * D + ti) * hw + (long long)yo * a.W + x];
                }
#pragma unroll
                for (int u = 0; u < CB_U; ++u) {
                    const int e = e0 + u * CB_THREADS;
                    const int ti = e / ncols, xx = e - ti * ncols;
                    if (ti < D) gs[ti][(xx & 1) * CB_HALF + (xx >> 1)] = v[u];
                }
            }
        } else {                                                                    // band at the pixel itself: row y, 32 columns
            for (int e0 = tid; e0 < D * CB_TX; e0 += CB_THREADS * CB_U) {
                float v[CB_U];
#pragma unroll
                for (int u = 0; u < CB_U; ++u) {
                    const int e = e0 + u * CB_THREADS;
                    const int ti = e >> 5, x = x0 + (e & 31);
                    v[u] = 0.f;
                    if (ti < D && x < a.W) v[u] = gn[(long long)(tj * D + ti) * hw + (long long)y * a.W + x];
                }
#pragma unroll
                for (int u = 0; u < CB_U; ++u) {
                    const int e = e0 + u * CB_THREADS;
                    const int ti = e >> 5, px = e & 31;
                    if (ti < D) gs[ti][(px & 1) * 16 + (px >> 1)] = v[u];
                }
            }
        }
        __syncthreads();
        float g[CB_DMAX][4];                                                        // g[t][k]: band value that meets window entry k + t
        if (which) {
#pragma unroll
            for (int t = 0; t < CB_DMAX; ++t)
#pragma unroll
                for (int k = 0; k < 4; ++k) g[t][k] = t < D ? gs[D - 1 - t][par * CB_HALF + 4 * s4 + k + t] : 0.f;
        } else {
#pragma unroll
            for (int t = 0; t < CB_DMAX; ++t) {
                if (t < D) {
                    const float4 t4 = *reinterpret_cast<const float4*>(&gs[t][par * 16 + 4 * s4]);
                    g[t][0] = t4.x; g[t][1] = t4.y; g[t][2] = t4.z; g[t][3] = t4.w;
                } else {
                    g[t][0] = g[t][1] = g[t][2] = g[t][3] = 0.f;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < CB_CPT; ++q) {
            const float4* wv = reinterpret_cast<const float4*>(&fs[cl * CB_CPT + q][par * CB_HALF + 4 * s4]);
            float w[24];
#pragma unroll
            for (int v = 0; v < 6; ++v) { const float4 t4 = wv[v]; w[4 * v] = t4.x; w[4 * v + 1] = t4.y; w[4 * v + 2] = t4.z; w[4 * v + 3] = t4.w; }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int t = 0; t < CB_DMAX; ++t) acc[q][k] += g[t][k] * w[k + t];
        }
    }
    const float inv = 1.f / (float)a.C;                                             // kernel_size 1: k^2 C = C
#pragma unroll
    for (int q = 0; q < CB_CPT; ++q) {
        const int c = c0 + cl * CB_CPT + q;
        if (c >= a.C) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + par + 8 * s4 + 2 * k;
            if (x < a.W) dst[((long long)n * a.C + c) * hw + (long long)y * a.W + x] = acc[q][k] * inv;
        }
    }
}

struct CorrBwdOp : Op {
    CorrBwdArgs a; bool tile;
    int launch(hipStream_t s) override {
        if (tile) {
            dim3 grid((unsigned)ceil_div(a.W, CB_TX), (unsigned)a.H, (unsigned)(a.N * ceil_div(a.C, CB_CH) * 2));
            hipLaunchKernelGGL(correlation_bwd_tile_kernel, grid, dim3(CB_THREADS), 0, s, a);
        } else {
            dim3 grid((unsigned)ceil_div(a.W, 64), (unsigned)a.H, (unsigned)(a.N * ceil_div(a.C, CG_CH) * 2));
            hipLaunchKernelGGL(correlation_bwd_generic_kernel, grid, dim3(64), 0, s, a);
        }
        return check_launch();
    }
    const char* name() const override { return "correlation_backward"; }
};

// ---- resample2d backward ----
// forward (flow_ops.hip): out[b][c][y][x] = sum_{fy, fx < k} bilinear weights(alpha, beta) * img[b][c][yT|yB + fy][xL|xR + fx] with
// indices clamped to the OUTPUT extent and the weights from the unclamped fractional parts.
struct Resample2dBwdArgs { const float* img; const float* flow; const float* gout; float* gimg; float* gflow; int N, C, H, W, OH, OW, ksize; };

__global__ __launch_bounds__(256) void zero_f32_kernel(float* p, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) p[e] = 0.f;
}

// thread = output pixel (b, y, x), loop over channels.  grad_img: the scatter of resample2d_kernel.cu:67-117 (float atomicAdd on
// global memory, the four corner weights of the forward); grad_flow: the gather of :119-190,
//   d/dfx = sum_c g * ((1-beta) (I[yT][xR] - I[yT][xL]) + beta (I[yB][xR] - I[yB][xL])),  d/dfy likewise,
// in the reference's own order of operations, summed over the channels by the one lane that owns the pixel: deterministic.
// Two deliberate differences for kernel_size > 1 (FlowNet2 only uses 1, where there is none): the indices are clamped to the OUTPUT
// extent as in the forward pass (the reference's image gradient clamps to the image extent, which lets yB + fy leave the image), and
// the flow gradient sums the same kernel_size^2 taps as the forward (the reference sums (2 ((k-1)/2) + 1)^2, one tap for k = 2).
__global__ __launch_bounds__(256) void resample2d_bwd_kernel(const Resample2dBwdArgs a) {
    const long long ohw = (long long)a.OH * a.OW;
    const long long total = (long long)a.N * ohw;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const long long b = e / ohw, pix = e - b * ohw;
        const int y = (int)(pix / a.OW), x = (int)(pix - (long long)y * a.OW);
        const float dx = a.flow[(b * 2 + 0) * ohw + pix], dy = a.flow[(b * 2 + 1) * ohw + pix];
        const float xf = (float)x + dx, yf = (float)y + dy;
        const float alpha = xf - floorf(xf), beta = yf - floorf(yf);
        const int xL = max(min((int)floorf(xf), a.OW - 1), 0);
        const int xR = max(min((int)floorf(xf) + 1, a.OW - 1), 0);
        const int yT = max(min((int)floorf(yf), a.OH - 1), 0);
        const int yB = max(min((int)floorf(yf) + 1, a.OH - 1), 0);
        const float gam_x = 1.f - alpha, gam_y = 1.f - beta;
        float gx = 0.f, gy = 0.f;
        for (int c = 0; c < a.C; ++c) {
            const long long plane = (b * a.C + c) * (long long)a.H * a.W;
            const float g = a.gout[(b * a.C + c) * ohw + pix];
            for (int fy = 0; fy < a.ksize; ++fy)
                for (int fx = 0; fx < a.ksize; ++fx) {
                    const long long iTL = plane + (long long)(yT + fy) * a.W + xL + fx, iTR = plane + (long long)(yT + fy) * a.W + xR + fx;
                    const long long iBL = plane + (long long)(yB + fy) * a.W + xL + fx, iBR = plane + (long long)(yB + fy) * a.W + xR + fx;
                    if (a.gimg) {
                        atomicAdd(&a.gimg[iTL], (1.f - alpha) * (1.f - beta) * g);
                        atomicAdd(&a.gimg[iTR], alpha * (1.f - beta) * g);
                        atomicAdd(&a.gimg[iBL], (1.f - alpha) * beta * g);
                        atomicAdd(&a.gimg[iBR], alpha * beta * g);
                    }
                    if (a.gflow) {
                        const float vTL = a.img[iTL], vTR = a.img[iTR], vBL = a.img[iBL], vBR = a.img[iBR];
                        gx += gam_y * g * vTR; gx -= gam_y * g * vTL; gx += (1.f - gam_y) * g * vBR; gx -= (1.f - gam_y) * g * vBL;
                        gy += gam_x * g * vBL; gy -= gam_x * g * vTL; gy += (1.f - gam_x) * g * vBR; gy -= (1.f - gam_x) * g * vTR;
                    }
                }
        }
        if (a.gflow) { a.gflow[(b * 2 + 0) * ohw + pix] = gx; a.gflow[(b * 2 + 1) * ohw + pix] = gy; }
    }
}

static inline unsigned bgrid(long long n, long long cap = 4096) {
    long long b = ceil_div(n, 256);
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}

struct Resample2dBwdOp : Op {
    Resample2dBwdArgs a;
    int launch(hipStream_t s) override {
        if (a.gimg) {
            const long long n = (long long)a.N * a.C * a.H * a.W;
            hipLaunchKernelGGL(zero_f32_kernel, dim3(bgrid(n)), dim3(256), 0, s, a.gimg, n);
            int rc = check_launch(); if (rc) return rc;
        }
        hipLaunchKernelGGL(resample2d_bwd_kernel, dim3(bgrid((long long)a.N * a.OH * a.OW)), dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "resample2d_backward"; }
};

// ---- channelnorm backward: grad_in[b][c][p] = grad_out[b][p] * x[b][c][p] / (out[b][p] + 1e-9)  (channelnorm_kernel.cu:93; the
// reference's 1e-9 is a double literal, so its division runs in double: kept, the kernel is bound by its memory traffic) ----
struct ChannelNormBwdArgs { const float* x; const float* out; const float* gout; float* gin; int N, C; long long hw; };

__global__ __launch_bounds__(256) void channelnorm_bwd_kernel(const ChannelNormBwdArgs a) {
    const long long total = (long long)a.N * a.hw;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const long long b = e / a.hw, pix = e - b * a.hw;
        const float g = a.gout[e];
        const double den = (double)a.out[e] + 1e-9;
        for (int c = 0; c < a.C; ++c) {
            const long long i = (b * a.C + c) * a.hw + pix;
            a.gin[i] = (float)((double)(g * a.x[i]) / den);
        }
    }
}

struct ChannelNormBwdOp : Op {
    ChannelNormBwdArgs a;
    int launch(hipStream_t s) override {
        hipLaunchKernelGGL(channelnorm_bwd_kernel, dim3(bgrid((long long)a.N * a.hw)), dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "channelnorm_backward"; }
};

}  // namespace v2v

using namespace v2v;

extern "C" int v2v_correlation_backward(const float* in1, const float* in2, const float* grad_out, float* grad_in1, float* grad_in2,
                                        int32_t N, int32_t C, int32_t H, int32_t W, int32_t out_c, int32_t out_h, int32_t out_w,
                                        int32_t pad_size, int32_t kernel_size, int32_t max_displacement,
                                        int32_t stride1, int32_t stride2, int32_t corr_type_multiply, void* stream) {
    if (!in1 || !in2 || !grad_out || (!grad_in1 && !grad_in2) || stride1 < 1 || stride2 < 1 || kernel_size < 1 || (kernel_size & 1) == 0) {
        set_error("correlation_backward: bad argument"); return V2V_EINVAL;
    }
    if (corr_type_multiply != 1) { set_error("correlation_backward: only corr_type_multiply=1 exists in the reference"); return V2V_EINVAL; }
    if (N < 1 || C < 1 || H < 1 || W < 1 || pad_size < 0 || max_displacement < 0) {
        set_error("correlation_backward: non-positive size (N=%d C=%d H=%d W=%d pad=%d max_disp=%d)", N, C, H, W, pad_size, max_displacement);
        return V2V_EINVAL;
    }
    CorrBwdArgs a;
    a.in1 = in1; a.in2 = in2; a.gout = grad_out; a.g1 = grad_in1; a.g2 = grad_in2; a.N = N; a.C = C; a.H = H; a.W = W;
    a.pad = pad_size; a.ksize = kernel_size; a.krad = (kernel_size - 1) / 2; a.max_disp = max_displacement;
    a.s1 = stride1; a.s2 = stride2; a.drad = max_displacement / stride2; a.D = 2 * a.drad + 1;
    int oc;
    v2v_correlation_out_size(H, W, pad_size, kernel_size, max_displacement, stride1, stride2, &oc, &a.OH, &a.OW);
    if (a.D > 64 || a.OH <= 0 || a.OW <= 0) { set_error("correlation_backward: unsupported geometry"); return V2V_EINVAL; }
    if (out_c != oc || out_h != a.OH || out_w != a.OW) {
        set_error("correlation_backward: grad_out is [%d][%d][%d], the forward output of this geometry is [%d][%d][%d]", out_c, out_h, out_w, oc, a.OH, a.OW);
        return V2V_EINVAL;
    }
    if ((long long)N * ceil_div(C, CG_CH) * 2 > 65535 || H > 65535) { set_error("correlation_backward: batch x channels too large for one launch"); return V2V_EINVAL; }
    auto op = std::make_unique<CorrBwdOp>();
    op->a = a;
    op->tile = kernel_size == 1 && stride1 == 1 && stride2 == 2 && pad_size == max_displacement && (max_displacement & 1) == 0 &&
               a.drad >= 1 && a.D <= CB_DMAX && a.OH == H && a.OW == W;             // FlowNetC's geometry class (FlowNetC.py:31)
    return submit(std::move(op), stream);
}

extern "C" int v2v_resample2d_backward(const float* img, const float* flow, const float* grad_out, float* grad_img, float* grad_flow,
                                       int32_t N, int32_t C, int32_t H, int32_t W, int32_t OH, int32_t OW,
                                       int32_t kernel_size, void* stream) {
    if (!img || !flow || !grad_out || (!grad_img && !grad_flow) || kernel_size < 1) { set_error("resample2d_backward: bad argument"); return V2V_EINVAL; }
    if (N < 1 || C < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) { set_error("resample2d_backward: non-positive size"); return V2V_EINVAL; }
    if (OH + kernel_size - 1 > H || OW + kernel_size - 1 > W) { set_error("resample2d_backward: image smaller than flow"); return V2V_EINVAL; }
    auto op = std::make_unique<Resample2dBwdOp>();
    op->a = Resample2dBwdArgs{img, flow, grad_out, grad_img, grad_flow, N, C, H, W, OH, OW, kernel_size};
    return submit(std::move(op), stream);
}

extern "C" int v2v_channelnorm_backward(const float* x, const float* out, const float* grad_out, float* grad_in,
                                        int32_t N, int32_t C, int32_t H, int32_t W, int32_t norm_deg, void* stream) {
    if (!x || !out || !grad_out || !grad_in) { set_error("channelnorm_backward: null"); return V2V_EINVAL; }
    if (norm_deg != 2) { set_error("channelnorm_backward: the reference kernel implements norm_deg=2 only"); return V2V_EINVAL; }
    if (N < 1 || C < 1 || H < 1 || W < 1) { set_error("channelnorm_backward: non-positive size"); return V2V_EINVAL; }
    auto op = std::make_unique<ChannelNormBwdOp>();
    op->a = ChannelNormBwdArgs{x, out, grad_out, grad_in, N, C, (long long)H * W};
    return submit(std::move(op), stream);
}
