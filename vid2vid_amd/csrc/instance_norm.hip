// Training-mode InstanceNorm2d at any batch size (reference: get_norm_layer, models/networks.py:23-30 ->
// functools.partial(nn.InstanceNorm2d, affine=False); .eval() is never called, so the statistics are always those of the
// input: per SAMPLE and per channel, over the sample's OH*OW pixels, biased variance).
//
// The batch-1 path (csrc/norm_act.hip) reuses the BatchNorm machinery: the conv epilogue's per-M-tile (sum, sum^2) rows
// are reduced into ONE [4][C] block.  M tiles run over N*OH*OW and straddle samples, so at N > 1 the statistics are taken
// here instead, from the conv's raw NHWC output, with the sample as a grid dimension:
//     v2v_in_stats     raw -> scale_shift[N][4][C]                       (one read of raw)
//     v2v_in_apply     y = act(raw*scale[n] + shift[n]) [+add0] [+add1]  (one read of raw, one write of y)
//     v2v_in_backward  dRaw from dY with that sample's mean / invstd     (two reads of dY and raw, one write)
// All three are HBM-bound streaming kernels: wave64, 256-thread blocks, 16-byte vectors.  Reductions are two-stage in a
// fixed order with an fp64 combine and no floating-point atomics: two runs give the same bits.
#include "v2v_internal.h"

namespace v2v {

// Pixel groups per sample: enough workgroups to fill the chip (~2048 over slabs x groups x samples), at least 64 pixels
// per group, at most 256 groups (the last arriver of a (sample, slab) walks the group rows: 256 rows = 64 per row phase).
static int in_groups(long long HW, int C, int N) {
    const long long slabs = ceil_div(C, 64);
    long long g = ceil_div(2048, slabs * N);
    const long long cap = ceil_div(HW, 64);
    if (g > cap) g = cap;
    if (g > 256) g = 256;
    if (g < 1) g = 1;
    return (int)g;
}

// 16 bytes of raw: 4 fp32 or 8 bf16 channels
__device__ __forceinline__ void load_raw16(const float* p, float v[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void load_raw16(const bf16_t* p, float v[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
    v[4] = __uint_as_float(t.z << 16); v[5] = __uint_as_float(t.z & 0xffff0000u);
    v[6] = __uint_as_float(t.w << 16); v[7] = __uint_as_float(t.w & 0xffff0000u);
}
__device__ __forceinline__ void load4f(const float* p, float v[4]) { load_raw16(p, v); }
__device__ __forceinline__ void load4f(const bf16_t* p, float v[4]) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
}
__device__ __forceinline__ void store4f(float* p, const float v[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store4f(bf16_t* p, const float v[4]) {
    uint2 t;
    t.x = pack_bf16x2(v[0], v[1]);
    t.y = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<uint2*>(p) = t;
}

// The hand-off of bn_partial_reduce_kernel (csrc/norm_act.hip): the producers' rows were stored write-through at agent scope
// (the L2s of different XCDs are not coherent); every wave drains its stores, the workgroup meets, one lane takes the ticket of
// this (sample, slab) and the last arriver re-arms it.  Returns true in every thread of the last workgroup, which then holds an
// agent-scope acquire and may read the other groups' rows with plain loads.
__device__ __forceinline__ bool in_last_arriver(int* ticket, int groups, int* last_flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tk = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = tk == groups - 1 ? 1 : 0;
        if (last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm
        *last_flag = last;
    }
    __syncthreads();
    if (!*last_flag) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return true;
}

__device__ __forceinline__ void in_store_row(double* dst, double t1, double t2) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)__double_as_longlong(t1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(dst) + 1, (unsigned long long)__double_as_longlong(t2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Thread (cx, ph) of 64 x 4 adds the group rows ph, ph + 4, ... of its channel in that order; phases are combined
// ((p0 + p1) + p2) + p3 through `shd` ([4][64][2] doubles).  Valid in threads with ph == 0 after the call.
__device__ __forceinline__ void in_sum_rows(const double* rows, int groups, int C, int c, double* shd, double& d1, double& d2) {
    const int cx = threadIdx.x & 63, ph = threadIdx.x >> 6;
    d1 = 0.0; d2 = 0.0;
    if (c < C) {
#pragma unroll 8
        for (int r = ph; r < groups; r += 4) {
            d1 += rows[((long long)r * C + c) * 2 + 0];
            d2 += rows[((long long)r * C + c) * 2 + 1];
        }
    }
    shd[(ph * 64 + cx) * 2] = d1; shd[(ph * 64 + cx) * 2 + 1] = d2;
    __syncthreads();
    if (ph == 0) {
        d1 = ((shd[(0 * 64 + cx) * 2] + shd[(1 * 64 + cx) * 2]) + shd[(2 * 64 + cx) * 2]) + shd[(3 * 64 + cx) * 2];
        d2 = ((shd[(0 * 64 + cx) * 2 + 1] + shd[(1 * 64 + cx) * 2 + 1]) + shd[(2 * 64 + cx) * 2 + 1]) + shd[(3 * 64 + cx) * 2 + 1];
    }
}

// ---------------------------------------------------------------------------------------
// statistics: grid (64-channel slabs, pixel groups, samples)
// ---------------------------------------------------------------------------------------
struct InStatsArgs {
    const void* raw; int c_stride_raw; long long HW; int C; int groups;
    const float* gamma; const float* beta; float eps; double inv_count;
    float* scale_shift;     // [N][4][C]: scale, shift, mean, invstd
    double* ws;             // [N][groups][C][2]
    int* ticket;            // [N][slabs]
};

// R = float: thread (tx of 16, ty of 16) owns 4 channels; R = bf16: (tx of 8, ty of 32) owns 8 -- one 16-byte load per pixel,
// every TY-th pixel of the group.  x and x^2 are accumulated in fp64 from the first add (three fp64 operations per element stay
// far below the HBM rate), so E[x^2] - mean^2 keeps its digits for samples whose mean dwarfs their spread.
template <typename R>
__global__ __launch_bounds__(256) void in_stats_kernel(const InStatsArgs a) {
    constexpr int CPT = 16 / (int)sizeof(R);
    constexpr int TX = 64 / CPT, TY = 256 / TX;
    __shared__ double sh[TY][64][2];
    __shared__ int last_flag;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int n = blockIdx.z, g = blockIdx.y;
    const int c0 = blockIdx.x * 64 + tx * CPT;
    const long long p0 = (a.HW * g) / a.groups, p1 = (a.HW * (g + 1)) / a.groups;
    double s1[CPT], s2[CPT];
#pragma unroll
    for (int q = 0; q < CPT; ++q) { s1[q] = 0.0; s2[q] = 0.0; }
    if (c0 < a.C) {                          // c_stride_raw is a multiple of CPT and >= C: the 16-byte load stays inside the pixel's row
        const R* base = reinterpret_cast<const R*>(a.raw) + (long long)n * a.HW * a.c_stride_raw + c0;
#pragma unroll 4
        for (long long p = p0 + ty; p < p1; p += TY) {
            float v[CPT];
            load_raw16(base + p * a.c_stride_raw, v);
#pragma unroll
            for (int q = 0; q < CPT; ++q) {
                const double d = (double)v[q];
                s1[q] += d;
                s2[q] = fma(d, d, s2[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < CPT; ++q) { sh[ty][tx * CPT + q][0] = s1[q]; sh[ty][tx * CPT + q][1] = s2[q]; }
    __syncthreads();
    const int slabs = gridDim.x;
    double* rows = a.ws + (long long)n * a.groups * a.C * 2;
    if (threadIdx.x < 64) {
        const int c = blockIdx.x * 64 + threadIdx.x;
        if (c < a.C) {
            double t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int q = 0; q < TY; ++q) { t1 += sh[q][threadIdx.x][0]; t2 += sh[q][threadIdx.x][1]; }
            in_store_row(rows + ((long long)g * a.C + c) * 2, t1, t2);
        }
    }
    if (!in_last_arriver(a.ticket + n * slabs + blockIdx.x, a.groups, &last_flag)) return;
    // ---- bn_finalize_kernel's arithmetic on this sample's group rows ----
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    double d1, d2;
    in_sum_rows(rows, a.groups, a.C, c, &sh[0][0][0], d1, d2);
    if ((threadIdx.x >> 6) == 0 && c < a.C) {
        const double mean = d1 * a.inv_count;
        double var = d2 * a.inv_count - mean * mean;
        if (var < 0.0) var = 0.0;
        const double invstd = 1.0 / sqrt(var + (double)a.eps);
        const double gm = a.gamma ? (double)a.gamma[c] : 1.0;
        const double bt = a.beta ? (double)a.beta[c] : 0.0;
        const double sc = gm * invstd;
        float* ss = a.scale_shift + (long long)n * 4 * a.C;
        ss[c] = (float)sc;
        ss[a.C + c] = (float)(bt - mean * sc);
        ss[2 * a.C + c] = (float)mean;          // rows 2, 3: saved for the backward pass
        ss[3 * a.C + c] = (float)invstd;
    }
}

struct InStatsOp : Op {
    InStatsArgs a; int N; int raw_dtype;
    int launch(hipStream_t s) override {
        const dim3 grid((unsigned)ceil_div(a.C, 64), (unsigned)a.groups, (unsigned)N);
        if (raw_dtype == V2V_BF16) hipLaunchKernelGGL(in_stats_kernel<bf16_t>, grid, dim3(256), 0, s, a);
        else                       hipLaunchKernelGGL(in_stats_kernel<float>, grid, dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "in_stats"; }
};

// ---------------------------------------------------------------------------------------
// apply: bn_apply_kernel's streaming pass with the sample as gridDim.y, so the scale / shift rows are fixed per workgroup
// ---------------------------------------------------------------------------------------
struct InApplyArgs {
    const void* raw; int raw_bf16; int c_stride_raw; const float* scale_shift;
    const void* add0; const void* add1; void* y; unsigned short* x3;
    long long HW; int C; int c_stride; int act; float act_param;
};

template <int VEC>
__device__ __forceinline__ void in_load_ss(const float* ss, int C, int c0, float sc[VEC], float sh[VEC]) {
    if ((C & 3) == 0) {
#pragma unroll
        for (int q = 0; q < VEC; q += 4) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f), h = s;
            if (c0 + q < C) { s = *reinterpret_cast<const float4*>(ss + c0 + q); h = *reinterpret_cast<const float4*>(ss + C + c0 + q); }
            sc[q] = s.x; sc[q + 1] = s.y; sc[q + 2] = s.z; sc[q + 3] = s.w;
            sh[q] = h.x; sh[q + 1] = h.y; sh[q + 2] = h.z; sh[q + 3] = h.w;
        }
    } else {                                 // C % 4 != 0 (2-channel test towers, 1027-channel --label_feat trunks): the [4][C] rows are unaligned
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            const bool ok = c0 + q < C;
            sc[q] = ok ? ss[c0 + q] : 0.f;
            sh[q] = ok ? ss[C + c0 + q] : 0.f;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void in_apply_kernel(const InApplyArgs a) {
    constexpr int VEC = ElemTraits<T>::VEC;
    const int n = blockIdx.y;
    const float* ss = a.scale_shift + (long long)n * 4 * a.C;
    const long long pb = (long long)n * a.HW;                // first pixel of this sample
    const int vpr = a.c_stride / VEC;                        // vectors per pixel row
    const long long nvec = a.HW * vpr;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const T* add0 = reinterpret_cast<const T*>(a.add0);
    const T* add1 = reinterpret_cast<const T*>(a.add1);
    T* y = reinterpret_cast<T*>(a.y);
    const bool small = nvec < (1ll << 31);                   // 32-bit division (a 64-bit one is ~100 instructions per vector)
    const bool fixed = (stride % vpr) == 0;                  // the thread keeps its channel group: scale / shift stay in registers
    long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float sc[VEC], sh[VEC];
    if (fixed) in_load_ss<VEC>(ss, a.C, (int)(v % vpr) * VEC, sc, sh);
    for (; v < nvec; v += stride) {
        const long long pix = small ? (long long)((unsigned)v / (unsigned)vpr) : v / vpr;
        const int c0 = (int)(v - pix * vpr) * VEC;
        if (!fixed) in_load_ss<VEC>(ss, a.C, c0, sc, sh);
        float r[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) r[q] = 0.f;
        if (c0 < a.C) {                      // c_stride_raw is a multiple of the load width and >= C: the loads stay inside the pixel's row
            if (a.raw_bf16) {
                const bf16_t* rp = reinterpret_cast<const bf16_t*>(a.raw) + (pb + pix) * a.c_stride_raw + c0;
                if constexpr (VEC == 8) load_raw16(rp, r);
                else load4f(rp, r);
            } else {
                const float* rp = reinterpret_cast<const float*>(a.raw) + (pb + pix) * a.c_stride_raw + c0;
                load_raw16(rp, r);
                if constexpr (VEC == 8) { if (c0 + 4 < a.C) load_raw16(rp + 4, r + 4); }
            }
        }
        float o[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) o[q] = apply_act(r[q] * sc[q] + sh[q], a.act, a.act_param);
        const long long e = (pb + pix) * a.c_stride + c0;
        if (add0) {
            float t[VEC];
            if constexpr (VEC == 8) load_raw16(add0 + e, t); else load4f(add0 + e, t);
#pragma unroll
            for (int q = 0; q < VEC; ++q) o[q] += t[q];
        }
        if (add1) {
            float t[VEC];
            if constexpr (VEC == 8) load_raw16(add1 + e, t); else load4f(add1 + e, t);
#pragma unroll
            for (int q = 0; q < VEC; ++q) o[q] += t[q];
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            if (c0 + q >= a.C) o[q] = 0.f;   // padded channels read as zero downstream
        }
        if constexpr (VEC == 4) {
            store4f(y + e, o);
            if (a.x3) {                      // the arithmetic of split_x3_kernel (csrc/pointwise.hip), as v2v_bn_apply_x3: [hi | lo | hi]
                unsigned short hi[4], lo[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    hi[q] = f32_to_bf16_bits(o[q]);
                    lo[q] = f32_to_bf16_bits(o[q] - bf16_bits_to_f32(hi[q]));
                }
                const uint2 vh = make_uint2((unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16));
                const uint2 vl = make_uint2((unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16));
                unsigned short* o3 = a.x3 + (pb + pix) * 3ll * a.C + c0;
                *reinterpret_cast<uint2*>(o3) = vh;
                *reinterpret_cast<uint2*>(o3 + a.C) = vl;
                *reinterpret_cast<uint2*>(o3 + 2 * a.C) = vh;
            }
        } else {
            uint4 pk;
            pk.x = pack_bf16x2(o[0], o[1]);
            pk.y = pack_bf16x2(o[2], o[3]);
            pk.z = pack_bf16x2(o[4], o[5]);
            pk.w = pack_bf16x2(o[6], o[7]);
            *reinterpret_cast<uint4*>(y + e) = pk;
        }
    }
}

struct InApplyOp : Op {
    InApplyArgs a; int N; int dtype;
    int launch(hipStream_t s) override {
        const int vec = dtype == V2V_BF16 ? 8 : 4;
        const long long nvec = a.HW * (a.c_stride / vec);
        long long blocks = ceil_div(nvec, 256), cap = 4096 / N;
        if (cap < 64) cap = 64;
        if (blocks > cap) blocks = cap;
        if (blocks < 1) blocks = 1;
        const dim3 grid((unsigned)blocks, (unsigned)N);
        if (dtype == V2V_BF16) hipLaunchKernelGGL(in_apply_kernel<bf16_t>, grid, dim3(256), 0, s, a);
        else                   hipLaunchKernelGGL(in_apply_kernel<float>, grid, dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "in_apply"; }
};

// ---------------------------------------------------------------------------------------
// backward of  y = act(instance_norm(raw)) (+ residuals)  -- autograd of nn.InstanceNorm2d in training mode + ReLU / LeakyReLU:
//   g      = dY * act'(raw*scale[n] + shift[n])
//   xhat   = (raw - mean[n]) * invstd[n]
//   dRaw   = scale[n] * (g - sum_p g / HW - xhat * sum_p g*xhat / HW)          sums over the SAMPLE's pixels
//   dbeta  = sum_n sum_p g,   dgamma = sum_n sum_p g*xhat                      (affine=True only)
// ---------------------------------------------------------------------------------------
struct InBwdArgs {
    const void* dy; const float* raw; const float* stats;    // stats: [N][4][C]
    void* draw;
    long long HW; int C, c_stride, c_stride_raw, c_stride_out, act; float act_param;
    int vec;                // strides / base pointers allow the 4-channel vector loads
    int groups; int N;
    double* ws;             // [N][groups][C][2]
    double* sums;           // [N][C][2]: (sum g, sum g*xhat) of each sample
    float* coef;            // [N][2][C]: the same over HW
    int* ticket;            // [N][slabs]
    double inv_count;
    float* dgamma; float* dbeta; int accumulate;
};

__device__ __forceinline__ float in_act_grad(float pre, int act, float param) {
    switch (act) {
        case V2V_ACT_RELU:  return pre > 0.f ? 1.f : 0.f;
        case V2V_ACT_LEAKY: return pre > 0.f ? 1.f : param;
        default:            return 1.f;
    }
}

// grid (64-channel slabs, pixel groups, samples); thread (tx, ty) of 16 x 16: 4 channels, every 16th pixel of the group
template <typename T>
__global__ __launch_bounds__(256) void in_bwd_reduce_kernel(const InBwdArgs a) {
    __shared__ double sh[16][64][2];
    __shared__ int last_flag;
    const T* dy = reinterpret_cast<const T*>(a.dy);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int n = blockIdx.z, g = blockIdx.y;
    const int c0 = blockIdx.x * 64 + tx * 4;
    const long long pb = (long long)n * a.HW;
    const long long p0 = pb + (a.HW * g) / a.groups, p1 = pb + (a.HW * (g + 1)) / a.groups;
    const float* st = a.stats + (long long)n * 4 * a.C;
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    if (c0 < a.C) {
        float sc[4], sf[4], mean[4], inv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = c0 + q < a.C ? c0 + q : a.C - 1;
            sc[q] = st[c]; sf[q] = st[a.C + c]; mean[q] = st[2 * a.C + c]; inv[q] = st[3 * a.C + c];
        }
        for (long long p = p0 + ty; p < p1; p += 16) {
            float gq[4], r[4];
            if (a.vec) { load4f(dy + p * a.c_stride + c0, gq); load4f(a.raw + p * a.c_stride_raw + c0, r); }
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool ok = c0 + q < a.C;
                    gq[q] = ok ? load_act(dy, p * a.c_stride + c0 + q) : 0.f;
                    r[q] = ok ? a.raw[p * a.c_stride_raw + c0 + q] : 0.f;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                gq[q] *= in_act_grad(r[q] * sc[q] + sf[q], a.act, a.act_param);
                s1[q] += gq[q];
                s2[q] += gq[q] * ((r[q] - mean[q]) * inv[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { sh[ty][tx * 4 + q][0] = (double)s1[q]; sh[ty][tx * 4 + q][1] = (double)s2[q]; }
    __syncthreads();
    const int slabs = gridDim.x;
    double* rows = a.ws + (long long)n * a.groups * a.C * 2;
    if (threadIdx.x < 64) {
        const int c = blockIdx.x * 64 + threadIdx.x;
        if (c < a.C) {
            double t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) { t1 += sh[q][threadIdx.x][0]; t2 += sh[q][threadIdx.x][1]; }
            in_store_row(rows + ((long long)g * a.C + c) * 2, t1, t2);
        }
    }
    if (!in_last_arriver(a.ticket + n * slabs + blockIdx.x, a.groups, &last_flag)) return;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    double d1, d2;
    in_sum_rows(rows, a.groups, a.C, c, &sh[0][0][0], d1, d2);
    if ((threadIdx.x >> 6) == 0 && c < a.C) {
        a.sums[((long long)n * a.C + c) * 2 + 0] = d1;       // read by the NEXT launch (in_bwd_apply_kernel): plain stores
        a.sums[((long long)n * a.C + c) * 2 + 1] = d2;
        float* k = a.coef + (long long)n * 2 * a.C;
        k[c] = (float)(d1 * a.inv_count);
        k[a.C + c] = (float)(d2 * a.inv_count);
    }
}

// grid (64-pixel blocks of the sample, 64-channel slabs of the output stride, samples).  Writes dRaw in the activation dtype, pad
// channels zero.  Workgroup (0, slab, 0) also adds the per-sample sums over the samples, in sample order, into dgamma / dbeta.
template <typename T>
__global__ __launch_bounds__(256) void in_bwd_apply_kernel(const InBwdArgs a) {
    const T* dy = reinterpret_cast<const T*>(a.dy);
    T* out = reinterpret_cast<T*>(a.draw);
    const int n = blockIdx.z;
    if (blockIdx.x == 0 && n == 0 && threadIdx.x < 64 && (a.dgamma || a.dbeta)) {
        const int c = blockIdx.y * 64 + threadIdx.x;
        if (c < a.C) {
            double d1 = 0.0, d2 = 0.0;
            for (int k = 0; k < a.N; ++k) { d1 += a.sums[((long long)k * a.C + c) * 2]; d2 += a.sums[((long long)k * a.C + c) * 2 + 1]; }
            if (a.dbeta)  a.dbeta[c]  = (a.accumulate ? a.dbeta[c] : 0.f) + (float)d1;
            if (a.dgamma) a.dgamma[c] = (a.accumulate ? a.dgamma[c] : 0.f) + (float)d2;
        }
    }
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int c0 = blockIdx.y * 64 + tx * 4;
    if (c0 >= a.c_stride_out) return;
    const float* st = a.stats + (long long)n * 4 * a.C;
    const float* kf = a.coef + (long long)n * 2 * a.C;
    float sc[4], sf[4], mean[4], inv[4], k1[4], k2[4];
    bool okc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        okc[q] = c0 + q < a.C;
        const int c = okc[q] ? c0 + q : a.C - 1;
        sc[q] = st[c]; sf[q] = st[a.C + c]; mean[q] = st[2 * a.C + c]; inv[q] = st[3 * a.C + c];
        k1[q] = kf[c]; k2[q] = kf[a.C + c];
    }
    const long long pb = (long long)n * a.HW;
    const long long q0 = (long long)blockIdx.x * 64;
    long long q1 = q0 + 64; if (q1 > a.HW) q1 = a.HW;
    for (long long p = pb + q0 + ty; p < pb + q1; p += 16) {
        float g[4] = {0.f, 0.f, 0.f, 0.f}, r[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        if (c0 < a.C) {
            if (a.vec) { load4f(dy + p * a.c_stride + c0, g); load4f(a.raw + p * a.c_stride_raw + c0, r); }
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (okc[q]) { g[q] = load_act(dy, p * a.c_stride + c0 + q); r[q] = a.raw[p * a.c_stride_raw + c0 + q]; }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float gg = g[q] * in_act_grad(r[q] * sc[q] + sf[q], a.act, a.act_param);
            o[q] = okc[q] ? sc[q] * (gg - k1[q] - (r[q] - mean[q]) * inv[q] * k2[q]) : 0.f;
        }
        store4f(out + p * a.c_stride_out + c0, o);
    }
}

struct InBwdOp : Op {
    InBwdArgs a; int dtype;
    int launch(hipStream_t s) override {
        const dim3 rgrid((unsigned)ceil_div(a.C, 64), (unsigned)a.groups, (unsigned)a.N);
        if (dtype == V2V_BF16) hipLaunchKernelGGL(in_bwd_reduce_kernel<bf16_t>, rgrid, dim3(256), 0, s, a);
        else                   hipLaunchKernelGGL(in_bwd_reduce_kernel<float>, rgrid, dim3(256), 0, s, a);
        int rc = check_launch(); if (rc) return rc;
        const dim3 agrid((unsigned)ceil_div(a.HW, 64), (unsigned)ceil_div(a.c_stride_out, 64), (unsigned)a.N);
        if (dtype == V2V_BF16) hipLaunchKernelGGL(in_bwd_apply_kernel<bf16_t>, agrid, dim3(256), 0, s, a);
        else                   hipLaunchKernelGGL(in_bwd_apply_kernel<float>, agrid, dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "in_backward"; }
};

// ---------------------------------------------------------------------------------------
// v2v_in_finalize_rows: per-sample finalize of the conv epilogue's statistics rows.  When every M tile of the conv launch
// covers pixels of ONE sample (v2v_conv_stats_rows_per_sample), sample n owns rows [n * R, (n + 1) * R) and its statistics
// need no second read of the raw output.  The arithmetic is v2v_bn_finalize's on that slice (csrc/norm_act.hip), bit for
// bit: four row phases per channel in fp64, combined ((p0 + p1) + p2) + p3; more than 512 rows per sample go through the
// same row groups first (bn_partial_reduce_kernel's cut), as a launch of its own.  A workgroup owns a (64-channel slab,
// sample) or a (slab, row group, sample); it reads only what the previous launch wrote: no tickets, no waiting.
// ---------------------------------------------------------------------------------------
struct InRowsArgs {
    const void* rows; int R; int C; int groups; double* ws;      // R: rows per sample (of the stage: conv rows, or group rows)
    double inv_count; const float* gamma; const float* beta; float eps; float* scale_shift;
};

__global__ __launch_bounds__(256) void in_rows_partial_kernel(const InRowsArgs a) {
    __shared__ double sh[4][64][2];
    const int cx = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    const int g = blockIdx.y, n = blockIdx.z;
    const float* part = reinterpret_cast<const float*>(a.rows) + (long long)n * a.R * a.C * 2;
    const int r0 = (int)(((long long)a.R * g) / a.groups), r1 = (int)(((long long)a.R * (g + 1)) / a.groups);
    double s1 = 0.0, s2 = 0.0;
    if (c < a.C) {
#pragma unroll 8
        for (int r = r0 + ph; r < r1; r += 4) {
            const float2 v = *reinterpret_cast<const float2*>(part + ((long long)r * a.C + c) * 2);
            s1 += (double)v.x;
            s2 += (double)v.y;
        }
    }
    sh[ph][cx][0] = s1;
    sh[ph][cx][1] = s2;
    __syncthreads();
    if (ph == 0 && c < a.C) {
        double* dst = a.ws + (((long long)n * a.groups + g) * a.C + c) * 2;
        dst[0] = ((sh[0][cx][0] + sh[1][cx][0]) + sh[2][cx][0]) + sh[3][cx][0];
        dst[1] = ((sh[0][cx][1] + sh[1][cx][1]) + sh[2][cx][1]) + sh[3][cx][1];
    }
}

template <typename R>
__global__ __launch_bounds__(256) void in_rows_finalize_kernel(const InRowsArgs a) {
    __shared__ double sh[4][64][2];
    const int cx = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    const int n = blockIdx.y;
    const R* rows_ = reinterpret_cast<const R*>(a.rows) + (long long)n * a.R * a.C * 2;
    double s1 = 0.0, s2 = 0.0;
    if (c < a.C) {
#pragma unroll 8
        for (int r = ph; r < a.R; r += 4) {
            s1 += (double)rows_[((long long)r * a.C + c) * 2 + 0];
            s2 += (double)rows_[((long long)r * a.C + c) * 2 + 1];
        }
    }
    sh[ph][cx][0] = s1;
    sh[ph][cx][1] = s2;
    __syncthreads();
    if (ph == 0 && c < a.C) {
        s1 = ((sh[0][cx][0] + sh[1][cx][0]) + sh[2][cx][0]) + sh[3][cx][0];
        s2 = ((sh[0][cx][1] + sh[1][cx][1]) + sh[2][cx][1]) + sh[3][cx][1];
        const double mean = s1 * a.inv_count;
        double var = s2 * a.inv_count - mean * mean;
        if (var < 0.0) var = 0.0;
        const double invstd = 1.0 / sqrt(var + (double)a.eps);
        const double g = a.gamma ? (double)a.gamma[c] : 1.0;
        const double b = a.beta ? (double)a.beta[c] : 0.0;
        const double sc = g * invstd;
        float* ss = a.scale_shift + (long long)n * 4 * a.C;
        ss[c] = (float)sc;
        ss[a.C + c] = (float)(b - mean * sc);
        ss[2 * a.C + c] = (float)mean;
        ss[3 * a.C + c] = (float)invstd;
    }
}

struct InRowsOp : Op {
    InRowsArgs a; int N;
    int launch(hipStream_t s) override {
        const unsigned slabs = (unsigned)ceil_div(a.C, 64);
        if (a.groups > 0) {
            hipLaunchKernelGGL(in_rows_partial_kernel, dim3(slabs, (unsigned)a.groups, (unsigned)N), dim3(256), 0, s, a);
            int rc = check_launch(); if (rc) return rc;
            InRowsArgs f = a;
            f.rows = a.ws; f.R = a.groups;
            hipLaunchKernelGGL(in_rows_finalize_kernel<double>, dim3(slabs, (unsigned)N), dim3(256), 0, s, f);
        } else {
            hipLaunchKernelGGL(in_rows_finalize_kernel<float>, dim3(slabs, (unsigned)N), dim3(256), 0, s, a);
        }
        return check_launch();
    }
    const char* name() const override { return "in_finalize_rows"; }
};

static bool in_geometry_ok(const char* who, int N, long long HW, int C) {
    if (N <= 0 || N > 65535 || HW <= 0 || C <= 0 || HW > (1ll << 40) / N) {
        set_error("%s: bad geometry (N=%d HW=%lld C=%d)", who, N, HW, C);
        return false;
    }
    return true;
}

}  // namespace v2v

using namespace v2v;

extern "C" int v2v_in_groups(int64_t HW, int32_t C, int32_t N) {
    if (HW <= 0 || C <= 0 || N <= 0) return 0;
    return in_groups(HW, C, N);
}

extern "C" int64_t v2v_in_workspace_bytes(int64_t HW, int32_t C, int32_t N) {
    if (HW <= 0 || C <= 0 || N <= 0) return 0;
    const int64_t G = in_groups(HW, C, N);
    return (int64_t)N * G * C * 2 * 8 + (int64_t)N * C * 2 * 8 + (int64_t)N * C * 2 * 4;
}

extern "C" int v2v_in_ticket_words(int32_t C, int32_t N) {
    if (C <= 0 || N <= 0) return 0;
    return (int)(N * ceil_div(C, 64));
}

extern "C" int64_t v2v_in_finalize_rows_workspace(int32_t rows_per_sample, int32_t C, int32_t N) {
    if (rows_per_sample <= 0 || C <= 0 || N <= 0) return 0;
    return (int64_t)N * v2v_bn_finalize_groups(rows_per_sample) * C * 2 * 8;
}

extern "C" int v2v_in_finalize_rows(const float* rows, int32_t rows_per_sample, int32_t N, int32_t C, int64_t count,
                                    const float* gamma, const float* beta, float eps, float* scale_shift, void* workspace,
                                    void* stream) {
    if (!in_geometry_ok("in_finalize_rows", N, count, C)) return V2V_EINVAL;
    if (!rows || !scale_shift || rows_per_sample <= 0 || (long long)rows_per_sample * N > 0x7fffffffll) {
        set_error("in_finalize_rows: bad argument"); return V2V_EINVAL;
    }
    const int groups = v2v_bn_finalize_groups(rows_per_sample);
    if (groups > 0 && (!workspace || (((uintptr_t)workspace) & 7))) {
        set_error("in_finalize_rows: %d rows per sample need the fp64 workspace (v2v_in_finalize_rows_workspace)", rows_per_sample);
        return V2V_EINVAL;
    }
    auto op = std::make_unique<InRowsOp>();
    InRowsArgs& a = op->a;
    a.rows = rows; a.R = rows_per_sample; a.C = C; a.groups = groups; a.ws = reinterpret_cast<double*>(workspace);
    a.inv_count = 1.0 / (double)count; a.gamma = gamma; a.beta = beta; a.eps = eps; a.scale_shift = scale_shift;
    op->N = N;
    return submit(std::move(op), stream);
}

extern "C" int v2v_in_stats(const void* raw, int32_t raw_dtype, int32_t c_stride_raw, const float* gamma, const float* beta, float eps,
                            float* scale_shift, void* workspace, int32_t* tickets, int32_t N, int64_t HW, int32_t C, void* stream) {
    if (!in_geometry_ok("in_stats", N, HW, C)) return V2V_EINVAL;
    if (!raw || !scale_shift || !workspace || !tickets) { set_error("in_stats: null argument"); return V2V_EINVAL; }
    const int w = raw_dtype == V2V_BF16 ? 8 : 4;
    if ((raw_dtype != V2V_F32 && raw_dtype != V2V_BF16) || c_stride_raw < C || c_stride_raw % w != 0 || (((uintptr_t)raw) & 15) || (((uintptr_t)workspace) & 7)) {
        set_error("in_stats: raw needs a 16-byte aligned tensor and a channel stride >= C that is a multiple of %d (C=%d raw=%d)", w, C, c_stride_raw);
        return V2V_EINVAL;
    }
    auto op = std::make_unique<InStatsOp>();
    InStatsArgs& a = op->a;
    a.raw = raw; a.c_stride_raw = c_stride_raw; a.HW = HW; a.C = C; a.groups = in_groups(HW, C, N);
    a.gamma = gamma; a.beta = beta; a.eps = eps; a.inv_count = 1.0 / (double)HW;
    a.scale_shift = scale_shift; a.ws = reinterpret_cast<double*>(workspace); a.ticket = tickets;
    op->N = N; op->raw_dtype = raw_dtype;
    return submit(std::move(op), stream);
}

extern "C" int v2v_in_apply(const void* raw, int32_t raw_dtype, int32_t c_stride_raw, const float* scale_shift,
                            const void* add0, const void* add1, void* y, void* x3, int32_t N, int64_t HW, int32_t C, int32_t c_stride,
                            int32_t act, float act_param, int32_t dtype, void* stream) {
    if (!in_geometry_ok("in_apply", N, HW, C)) return V2V_EINVAL;
    if (!raw || !scale_shift || !y) { set_error("in_apply: null argument"); return V2V_EINVAL; }
    const int vec = dtype == V2V_BF16 ? 8 : 4;
    const int w = raw_dtype == V2V_BF16 ? 8 : 4;
    if ((dtype != V2V_F32 && dtype != V2V_BF16) || (raw_dtype != V2V_F32 && raw_dtype != V2V_BF16) || act < V2V_ACT_NONE || act > V2V_ACT_SIGMOID) {
        set_error("in_apply: dtype / activation code"); return V2V_EINVAL;
    }
    if (c_stride % vec != 0 || c_stride_raw % w != 0 || C > c_stride || c_stride_raw < C ||
        ((((uintptr_t)raw) | ((uintptr_t)y) | ((uintptr_t)add0) | ((uintptr_t)add1)) & 15)) {
        set_error("in_apply: 16-byte aligned tensors and channel strides that are multiples of the vector width (C=%d stride=%d raw=%d)", C, c_stride, c_stride_raw);
        return V2V_EINVAL;
    }
    if (x3 && (dtype != V2V_F32 || C % 4 != 0 || c_stride != C || (((uintptr_t)x3) & 7))) {
        set_error("in_apply: the bf16x3 output needs fp32 and a dense channel stride, C %% 4 == 0"); return V2V_EINVAL;
    }
    auto op = std::make_unique<InApplyOp>();
    InApplyArgs& a = op->a;
    a.raw = raw; a.raw_bf16 = raw_dtype == V2V_BF16; a.c_stride_raw = c_stride_raw; a.scale_shift = scale_shift;
    a.add0 = add0; a.add1 = add1; a.y = y; a.x3 = reinterpret_cast<unsigned short*>(x3);
    a.HW = HW; a.C = C; a.c_stride = c_stride; a.act = act; a.act_param = act_param;
    op->N = N; op->dtype = dtype;
    return submit(std::move(op), stream);
}

extern "C" int v2v_in_backward(const void* dy, const float* raw, int32_t c_stride_raw, const float* stats,
                               void* draw, int32_t c_stride_out, float* dgamma, float* dbeta, int32_t accumulate,
                               void* workspace, int32_t* tickets, int32_t N, int64_t HW, int32_t C, int32_t c_stride,
                               int32_t act, float act_param, int32_t dtype, void* stream) {
    if (!in_geometry_ok("in_backward", N, HW, C)) return V2V_EINVAL;
    if (!dy || !raw || !stats || !draw || !workspace || !tickets) { set_error("in_backward: null argument"); return V2V_EINVAL; }
    if (dtype != V2V_F32 && dtype != V2V_BF16) { set_error("in_backward: dtype"); return V2V_EINVAL; }
    if (c_stride_out % 4 != 0 || C > c_stride || c_stride_raw < C || C > c_stride_out) { set_error("in_backward: strides"); return V2V_EINVAL; }
    if (((uintptr_t)draw & 15) || ((uintptr_t)workspace & 7)) { set_error("in_backward: draw must be 16-byte aligned"); return V2V_EINVAL; }
    if (act != V2V_ACT_NONE && act != V2V_ACT_RELU && act != V2V_ACT_LEAKY) { set_error("in_backward: activation"); return V2V_EINVAL; }
    auto op = std::make_unique<InBwdOp>();
    InBwdArgs& a = op->a;
    const int G = in_groups(HW, C, N);
    a.dy = dy; a.raw = raw; a.stats = stats; a.draw = draw;
    a.HW = HW; a.C = C; a.c_stride = c_stride; a.c_stride_raw = c_stride_raw; a.c_stride_out = c_stride_out;
    a.act = act; a.act_param = act_param;
    a.vec = (c_stride % 4 == 0 && c_stride_raw % 4 == 0 && (((uintptr_t)dy | (uintptr_t)raw) & 15) == 0) ? 1 : 0;
    a.groups = G; a.N = N;
    a.ws = reinterpret_cast<double*>(workspace);
    a.sums = a.ws + (long long)N * G * C * 2;
    a.coef = reinterpret_cast<float*>(a.sums + (long long)N * C * 2);
    a.ticket = tickets; a.inv_count = 1.0 / (double)HW;
    a.dgamma = dgamma; a.dbeta = dbeta; a.accumulate = accumulate;
    op->dtype = dtype;
    return submit(std::move(op), stream);
}
