// Loss reductions and the fused optimizer step of the vid2vid training path (gfx950).
//
//   GANLoss (LSGAN = MSE against a constant, models/networks.py:731-774)
//   criterionFeat = nn.L1Loss between discriminator features (models/vid2vid_model_D.py:65,208-211)
//   MaskedL1Loss (models/networks.py:804-812): mean |a*m - b*m| with the mask broadcast over channels
//   torch.optim.Adam (models/vid2vid_model_G.py:84, vid2vid_model_D.py:86-91) as ONE launch over the
//   flat parameter / gradient / moment buffers of an optimizer.
//
// All are HBM-bound streaming kernels.  Reductions are deterministic: fixed per-block partials,
// then one block combines them in order (fp64) and writes the scaled scalar.
#include "v2v_internal.h"
#include <cstring>

namespace v2v {

enum { LOSS_MSE_CONST = 0, LOSS_L1 = 1 };

struct LossArgs {
    const void* a; const void* b; const float* mask;   // mask: planar [N][1][HW] (planar mode only) or NULL
    float target; int kind;
    long long P; int C, c_stride;                      // NHWC mode: P pixels, C real channels
    long long n, chw, hw;                              // planar mode: n elements, C*HW, HW
    int planar;
    float* partials; int nblk;
    float* out; double scale;                          // out[0] = scale * sum
    const float* gout; void* da;                       // backward: da = d(out)/d(a) * gout[0]
};

template <typename T>
__device__ __forceinline__ float loss_term(const LossArgs& a, long long idx, float& av, float& bv, float& mv, bool& valid) {
    valid = true; mv = 1.f; bv = a.target;
    if (a.planar) {
        av = reinterpret_cast<const float*>(a.a)[idx];
        if (a.kind == LOSS_L1) bv = reinterpret_cast<const float*>(a.b)[idx];
        if (a.mask) { const long long n = idx / a.chw; mv = a.mask[n * a.hw + (idx % a.hw)]; }
    } else {
        const int c = (int)(idx % a.c_stride);
        valid = c < a.C;
        av = load_act(reinterpret_cast<const T*>(a.a), idx);
        if (a.kind == LOSS_L1) bv = load_act(reinterpret_cast<const T*>(a.b), idx);
    }
    if (!valid) return 0.f;
    if (a.kind == LOSS_MSE_CONST) { const float d = av - bv; return d * d; }
    return fabsf(av * mv - bv * mv);
}

template <typename T>
__global__ __launch_bounds__(256) void loss_partial_kernel(const LossArgs a) {
    __shared__ float sh[256];
    const long long total = a.planar ? a.n : a.P * a.c_stride;
    const long long stride = (long long)gridDim.x * blockDim.x;
    float s = 0.f;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        float av, bv, mv; bool valid;
        s += loss_term<T>(a, e, av, bv, mv, valid);
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.partials[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256) void loss_final_kernel(const LossArgs a) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < a.nblk; i += 256) s += (double)a.partials[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.out[0] = (float)(sh[0] * a.scale);
}

template <typename T>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const LossArgs a) {
    const long long total = a.planar ? a.n : a.P * a.c_stride;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const float g = a.gout[0] * (float)a.scale;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        float av, bv, mv; bool valid;
        loss_term<T>(a, e, av, bv, mv, valid);
        float d = 0.f;
        if (valid) {
            if (a.kind == LOSS_MSE_CONST) d = 2.f * (av - bv) * g;
            else { const float df = av * mv - bv * mv; d = (df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f)) * mv * g; }
        }
        if (a.planar) reinterpret_cast<float*>(a.da)[e] = d;
        else store_act(reinterpret_cast<T*>(a.da), e, d);
    }
}

static unsigned loss_grid(long long total) {
    long long b = ceil_div(total, 256 * 8);
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return (unsigned)b;
}

struct LossOp : Op {
    LossArgs a; int dtype; bool backward;
    int launch(hipStream_t s) override {
        const long long total = a.planar ? a.n : a.P * a.c_stride;
        if (backward) {
            long long b = ceil_div(total, 256); if (b > 4096) b = 4096; if (b < 1) b = 1;
            if (dtype == V2V_BF16 && !a.planar) hipLaunchKernelGGL(loss_bwd_kernel<bf16_t>, dim3((unsigned)b), dim3(256), 0, s, a);
            else                                 hipLaunchKernelGGL(loss_bwd_kernel<float>, dim3((unsigned)b), dim3(256), 0, s, a);
            return check_launch();
        }
        if (dtype == V2V_BF16 && !a.planar) hipLaunchKernelGGL(loss_partial_kernel<bf16_t>, dim3((unsigned)a.nblk), dim3(256), 0, s, a);
        else                                 hipLaunchKernelGGL(loss_partial_kernel<float>, dim3((unsigned)a.nblk), dim3(256), 0, s, a);
        int rc = check_launch(); if (rc) return rc;
        hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return backward ? "loss_backward" : "loss_forward"; }
};

// ---- Adam ------------------------------------------------------------------------------
struct AdamArgs { float* p; const float* g; float* m; float* v; long long n; float lr, b1, b2, eps, bc1, bc2_sqrt, wd, gscale; };

// The plain element loop: the one place the arithmetic of adam_step_kernel, adam_step_dev_kernel and adam_step_dev_guard_kernel
// is written.  `gscale` is a by-value argument in the first two and the guard block's scale word in the third.
template <typename A>
__device__ __forceinline__ void adam_plain_elems(const A& a, float step_size, float bc2_sqrt, float gscale) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        float g = a.g[i] * gscale;
        const float p = a.p[i];
        if (a.wd != 0.f) g += a.wd * p;
        const float m = a.b1 * a.m[i] + (1.f - a.b1) * g;
        const float v = a.b2 * a.v[i] + (1.f - a.b2) * g * g;
        a.m[i] = m; a.v[i] = v;
        const float denom = sqrtf(v) / bc2_sqrt + a.eps;
        a.p[i] = p - step_size * (m / denom);
    }
}

__global__ __launch_bounds__(256) void adam_step_kernel(const AdamArgs a) {
    adam_plain_elems(a, a.lr / a.bc1, a.bc2_sqrt, a.gscale);
}

// Graph-replayable form (optim.FusedAdam(capturable)): the 1-based step count and the learning rate live in DEVICE memory, so a
// launch captured once into a hipGraph keeps advancing the bias corrections on every replay (a by-value `step` would be frozen
// at its capture-time value).  state = {int step; float lr}: one thread bumps `step` in a launch of its own just before.
struct AdamDevState { int step; float lr; };
struct AdamDevArgs { float* p; const float* g; float* m; float* v; long long n; float b1, b2, eps, wd, gscale; AdamDevState* st; };

__global__ void adam_tick_kernel(AdamDevState* st) { st->step += 1; }

__device__ __forceinline__ void adam_dev_body(const AdamDevArgs& a, float gscale) {
    const int step = a.st->step;
    const double bc1 = 1.0 - pow((double)a.b1, (double)step);        // the host form's arithmetic (v2v_adam_step), once per thread
    const double bc2 = 1.0 - pow((double)a.b2, (double)step);
    adam_plain_elems(a, a.st->lr / (float)bc1, (float)sqrt(bc2), gscale);
}

__global__ __launch_bounds__(256) void adam_step_dev_kernel(const AdamDevArgs a) {
    adam_dev_body(a, a.gscale);
}

struct AdamDevOp : Op {
    AdamDevArgs a;
    int launch(hipStream_t s) override {
        hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, s, a.st);
        long long b = ceil_div(a.n, 256 * 4); if (b > 8192) b = 8192; if (b < 1) b = 1;
        hipLaunchKernelGGL(adam_step_dev_kernel, dim3((unsigned)b), dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "adam_step_dev"; }
};

struct AdamOp : Op {
    AdamArgs a;
    int launch(hipStream_t s) override {
        long long b = ceil_div(a.n, 256 * 4); if (b > 8192) b = 8192; if (b < 1) b = 1;
        hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)b), dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "adam_step"; }
};

// ---- Adam + weight averaging -----------------------------------------------
// The same update, plus a shadow of the weights in the same pass: ema = decay * ema + (1 - decay) * p'.  One kernel serves both
// forms (DEV: step count / learning rate in device memory, behind the same tick launch).  [head, head + 4 * nvec) is the part
// of [0, n) where all five buffers are 16-byte aligned (nvec = 0 when their misalignments differ): it moves as float4, the
// head and the tail as scalars.
struct AdamEmaArgs {
    float* p; const float* g; float* m; float* v; float* e; AdamDevState* st;
    long long n, head, nvec;
    float lr, b1, b2, eps, bc1, bc2_sqrt, wd, gscale, decay, omd;
};
struct AdamEmaCoef { float step_size, bc2_sqrt, b1, b2, omb1, omb2, eps, wd, gscale, decay, omd; };

// adam_step_kernel / adam_step_dev_kernel compile to separately rounded multiplies and adds everywhere except the last line,
// p - step_size * (m / denom), which is one fused multiply-add.  Contraction is switched off here and that one fma is written
// out, so these bits do not depend on what the optimiser makes of a wider loop body.
__device__ __forceinline__ void adam_ema_elem(float& p, float g, float& m, float& v, float& e, const AdamEmaCoef& c) {
#pragma clang fp contract(off)
    g = g * c.gscale;
    if (c.wd != 0.f) { const float t = c.wd * p; g = g + t; }
    const float m0 = c.b1 * m, m1 = c.omb1 * g;
    const float v0 = c.b2 * v, v1 = c.omb2 * g * g;
    m = m0 + m1; v = v0 + v1;
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = fmaf(-c.step_size, m / denom, p);
    const float q = c.omd * p;
    e = fmaf(c.decay, e, q);
}

template <bool DEV>
__device__ __forceinline__ void adam_ema_body(const AdamEmaArgs& a, float gscale) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    AdamEmaCoef c;
    if (DEV) {
        const int step = a.st->step;
        const double bc1 = 1.0 - pow((double)a.b1, (double)step);    // adam_step_dev_kernel's prologue
        const double bc2 = 1.0 - pow((double)a.b2, (double)step);
        c.step_size = a.st->lr / (float)bc1;
        c.bc2_sqrt = (float)sqrt(bc2);
    } else {
        c.step_size = a.lr / a.bc1;
        c.bc2_sqrt = a.bc2_sqrt;
    }
    c.b1 = a.b1; c.b2 = a.b2; c.omb1 = 1.f - a.b1; c.omb2 = 1.f - a.b2;
    c.eps = a.eps; c.wd = a.wd; c.gscale = gscale; c.decay = a.decay; c.omd = a.omd;

    const long long vbase = a.head;
    for (long long k = t0; k < a.nvec; k += stride) {
        const long long i = vbase + 4 * k;
        float4 p = *reinterpret_cast<const float4*>(a.p + i);
        const float4 g = *reinterpret_cast<const float4*>(a.g + i);
        float4 m = *reinterpret_cast<const float4*>(a.m + i);
        float4 v = *reinterpret_cast<const float4*>(a.v + i);
        float4 e = *reinterpret_cast<const float4*>(a.e + i);
        adam_ema_elem(p.x, g.x, m.x, v.x, e.x, c);
        adam_ema_elem(p.y, g.y, m.y, v.y, e.y, c);
        adam_ema_elem(p.z, g.z, m.z, v.z, e.z, c);
        adam_ema_elem(p.w, g.w, m.w, v.w, e.w, c);
        *reinterpret_cast<float4*>(a.m + i) = m;
        *reinterpret_cast<float4*>(a.v + i) = v;
        *reinterpret_cast<float4*>(a.p + i) = p;
        *reinterpret_cast<float4*>(a.e + i) = e;
    }
    const long long nscalar = a.n - 4 * a.nvec;          // head, then the tail behind the vector part
    for (long long j = t0; j < nscalar; j += stride) {
        const long long i = j < a.head ? j : j + 4 * a.nvec;
        float p = a.p[i], m = a.m[i], v = a.v[i], e = a.e[i];
        adam_ema_elem(p, a.g[i], m, v, e, c);
        a.m[i] = m; a.v[i] = v; a.p[i] = p; a.e[i] = e;
    }
}

template <bool DEV>
__global__ __launch_bounds__(256) void adam_step_ema_kernel(const AdamEmaArgs a) {
    adam_ema_body<DEV>(a, a.gscale);
}

struct AdamEmaOp : Op {
    AdamEmaArgs a; bool dev;
    int launch(hipStream_t s) override {
        long long b = ceil_div(a.n, 256 * 4); if (b > 8192) b = 8192; if (b < 1) b = 1;
        if (dev) {
            hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, s, a.st);
            hipLaunchKernelGGL(adam_step_ema_kernel<true>, dim3((unsigned)b), dim3(256), 0, s, a);
        } else {
            hipLaunchKernelGGL(adam_step_ema_kernel<false>, dim3((unsigned)b), dim3(256), 0, s, a);
        }
        return check_launch();
    }
    const char* name() const override { return dev ? "adam_step_dev_ema" : "adam_step_ema"; }
};

// ---- Adam behind a gradient guard --------------------------------------------
// Three launches ordered by the stream, no hand-off between workgroups: grad_sumsq (per-workgroup partials of sum g^2 in fp64
// and of the count of non-finite elements) -> guard_finalize (one workgroup: fixed-order sum, the skip decision, the step word,
// the scale) -> the device-state Adam kernels reading `scale` and `skip` from the guard block.
struct AdamGuard {                                   // v2v_hip.h documents this layout: the host reads it back
    double norm_sq; float scale; int skip; int skipped; int nonfinite; int applied; float gscale;
};
struct GuardPartial { double s; int nf; int pad; };
enum { GUARD_MAX_BLOCKS = 1024, GUARD_HEADER_BYTES = 32 };
static_assert(sizeof(AdamGuard) == GUARD_HEADER_BYTES && sizeof(GuardPartial) == 16, "guard block layout");

__device__ __forceinline__ GuardPartial* guard_partials(AdamGuard* gd) {
    return reinterpret_cast<GuardPartial*>(reinterpret_cast<char*>(gd) + GUARD_HEADER_BYTES);
}

struct SumsqArgs { const float* g; long long n, head, nvec; AdamGuard* gd; };

__device__ __forceinline__ void sumsq_elem(float g, double& s, int& nf) {
    const double d = (double)g;
    s += d * d;
    nf += isfinite(g) ? 0 : 1;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const SumsqArgs a) {
    __shared__ double sh[256];
    __shared__ int shn[256];
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double s = 0.0; int nf = 0;
    const float* gv = a.g + a.head;
    long long k = t0;
    for (; k + 3 * stride < a.nvec; k += 4 * stride) {           // four independent 16-byte loads in flight per thread
        const float4 g0 = *reinterpret_cast<const float4*>(gv + 4 * k);
        const float4 g1 = *reinterpret_cast<const float4*>(gv + 4 * (k + stride));
        const float4 g2 = *reinterpret_cast<const float4*>(gv + 4 * (k + 2 * stride));
        const float4 g3 = *reinterpret_cast<const float4*>(gv + 4 * (k + 3 * stride));
        sumsq_elem(g0.x, s, nf); sumsq_elem(g0.y, s, nf); sumsq_elem(g0.z, s, nf); sumsq_elem(g0.w, s, nf);
        sumsq_elem(g1.x, s, nf); sumsq_elem(g1.y, s, nf); sumsq_elem(g1.z, s, nf); sumsq_elem(g1.w, s, nf);
        sumsq_elem(g2.x, s, nf); sumsq_elem(g2.y, s, nf); sumsq_elem(g2.z, s, nf); sumsq_elem(g2.w, s, nf);
        sumsq_elem(g3.x, s, nf); sumsq_elem(g3.y, s, nf); sumsq_elem(g3.z, s, nf); sumsq_elem(g3.w, s, nf);
    }
    for (; k < a.nvec; k += stride) {
        const float4 g = *reinterpret_cast<const float4*>(gv + 4 * k);
        sumsq_elem(g.x, s, nf); sumsq_elem(g.y, s, nf); sumsq_elem(g.z, s, nf); sumsq_elem(g.w, s, nf);
    }
    const long long nscalar = a.n - 4 * a.nvec;          // head, then the tail behind the vector part
    for (long long j = t0; j < nscalar; j += stride) {
        const long long i = j < a.head ? j : j + 4 * a.nvec;
        sumsq_elem(a.g[i], s, nf);
    }
    sh[threadIdx.x] = s; shn[threadIdx.x] = nf;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh[threadIdx.x] += sh[threadIdx.x + w];
            const long long c = (long long)shn[threadIdx.x] + shn[threadIdx.x + w];
            shn[threadIdx.x] = c > 0x7fffffffLL ? 0x7fffffff : (int)c;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        GuardPartial* part = guard_partials(a.gd);
        part[blockIdx.x].s = sh[0]; part[blockIdx.x].nf = shn[0];
    }
}

struct FinalizeArgs { AdamGuard* gd; AdamDevState* st; int nblk; float gscale, max_norm; int skip_nonfinite; };

__global__ __launch_bounds__(256) void guard_finalize_kernel(const FinalizeArgs a) {
    __shared__ double sh[256];
    __shared__ long long shn[256];
    const GuardPartial* part = guard_partials(a.gd);
    double s = 0.0; long long nf = 0;
    for (int i = threadIdx.x; i < a.nblk; i += 256) { s += part[i].s; nf += part[i].nf; }
    sh[threadIdx.x] = s; shn[threadIdx.x] = nf;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { sh[threadIdx.x] += sh[threadIdx.x + w]; shn[threadIdx.x] += shn[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double norm_sq = sh[0];
    const int bad = shn[0] > 0x7fffffffLL ? 0x7fffffff : (int)shn[0];
    const int skip = (bad > 0 && a.skip_nonfinite) ? 1 : 0;
    double scale = (double)a.gscale;
    if (a.max_norm > 0.f) {                              // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
        double coef = (double)a.max_norm / ((double)a.gscale * sqrt(norm_sq) + 1e-6);
        if (coef > 1.0) coef = 1.0;                      // (a NaN norm keeps its NaN, as torch's clamp does)
        scale = (double)a.gscale * coef;
    }
    a.gd->norm_sq = norm_sq;
    a.gd->scale = (float)scale;
    a.gd->skip = skip;
    a.gd->nonfinite = bad;
    a.gd->gscale = a.gscale;
    if (skip) a.gd->skipped += 1;
    else if (a.st) a.st->step += 1;                      // stands in for adam_tick_kernel: a skipped step consumes no step number
    if (a.st) a.gd->applied = a.st->step;
}

__global__ __launch_bounds__(256) void adam_step_dev_guard_kernel(const AdamDevArgs a, const AdamGuard* gd) {
    if (gd->skip) return;
    adam_dev_body(a, gd->scale);
}

__global__ __launch_bounds__(256) void adam_step_ema_guard_kernel(const AdamEmaArgs a, const AdamGuard* gd) {
    if (gd->skip) return;
    adam_ema_body<true>(a, gd->scale);
}

static unsigned sumsq_grid(long long n) {
    long long b = ceil_div(n, 256 * 4);
    if (b > GUARD_MAX_BLOCKS) b = GUARD_MAX_BLOCKS;
    if (b < 1) b = 1;
    return (unsigned)b;
}

struct GradSumsqOp : Op {
    SumsqArgs a;
    int launch(hipStream_t s) override {
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(sumsq_grid(a.n)), dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "grad_sumsq"; }
};

struct GuardFinalizeOp : Op {
    FinalizeArgs a;
    int launch(hipStream_t s) override {
        hipLaunchKernelGGL(guard_finalize_kernel, dim3(1), dim3(256), 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "guard_finalize"; }
};

struct AdamGuardOp : Op {
    AdamDevArgs a; AdamEmaArgs ae; const AdamGuard* gd; bool ema;
    int launch(hipStream_t s) override {
        long long b = ceil_div(a.n, 256 * 4); if (b > 8192) b = 8192; if (b < 1) b = 1;
        if (ema) hipLaunchKernelGGL(adam_step_ema_guard_kernel, dim3((unsigned)b), dim3(256), 0, s, ae, gd);
        else     hipLaunchKernelGGL(adam_step_dev_guard_kernel, dim3((unsigned)b), dim3(256), 0, s, a, gd);
        return check_launch();
    }
    const char* name() const override { return ema ? "adam_step_dev_guard_ema" : "adam_step_dev_guard"; }
};

struct MemsetOp : Op {
    void* p; size_t bytes;
    int launch(hipStream_t s) override {
        hipError_t e = hipMemsetAsync(p, 0, bytes, s);
        if (e != hipSuccess) { set_error("memset: %s", hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    const char* name() const override { return "memset_zero"; }
};

}  // namespace v2v

using namespace v2v;

static int loss_common(LossArgs& a, int kind, const void* x, const void* b, const float* mask, float target,
                       int64_t P, int32_t C, int32_t c_stride, int64_t N, int64_t CHW, int64_t HW, int planar) {
    memset(&a, 0, sizeof(a));
    if (!x || (kind == LOSS_L1 && !b) || (kind != LOSS_L1 && kind != LOSS_MSE_CONST)) { set_error("loss: bad argument"); return V2V_EINVAL; }
    a.a = x; a.b = b; a.mask = mask; a.target = target; a.kind = kind; a.planar = planar;
    if (planar) {
        if (N <= 0 || CHW <= 0 || HW <= 0 || CHW % HW != 0) { set_error("loss: planar shape"); return V2V_EINVAL; }
        a.n = N * CHW; a.chw = CHW; a.hw = HW;
        a.scale = 1.0 / (double)a.n;
    } else {
        if (P <= 0 || C <= 0 || C > c_stride || mask) { set_error("loss: nhwc shape"); return V2V_EINVAL; }
        a.P = P; a.C = C; a.c_stride = c_stride;
        a.scale = 1.0 / ((double)P * (double)C);
    }
    return 0;
}

extern "C" int v2v_loss_workspace_floats(void) { return 1024; }

// mean loss over the real elements, times `weight`.  NHWC mode (planar = 0): a, b activations
// [P][c_stride] of `dtype`; planar mode: fp32 [N][C][HW] with optional mask [N][1][HW].
extern "C" int v2v_loss_forward(int32_t kind, const void* a, const void* b, const float* mask, float target, float weight,
                                int64_t P, int32_t C, int32_t c_stride, int64_t N, int64_t CHW, int64_t HW, int32_t planar,
                                float* workspace, float* out, int32_t dtype, void* stream) {
    auto op = std::make_unique<LossOp>();
    int rc = loss_common(op->a, kind, a, b, mask, target, P, C, c_stride, N, CHW, HW, planar);
    if (rc) return rc;
    if (!workspace || !out) { set_error("loss: null output"); return V2V_EINVAL; }
    op->a.scale *= (double)weight;
    op->a.partials = workspace; op->a.out = out;
    op->a.nblk = (int)loss_grid(planar ? op->a.n : P * c_stride);
    op->dtype = dtype; op->backward = false;
    return submit(std::move(op), stream);
}

extern "C" int v2v_loss_backward(int32_t kind, const void* a, const void* b, const float* mask, float target, float weight,
                                 int64_t P, int32_t C, int32_t c_stride, int64_t N, int64_t CHW, int64_t HW, int32_t planar,
                                 const float* grad_out, void* da, int32_t dtype, void* stream) {
    auto op = std::make_unique<LossOp>();
    int rc = loss_common(op->a, kind, a, b, mask, target, P, C, c_stride, N, CHW, HW, planar);
    if (rc) return rc;
    if (!grad_out || !da) { set_error("loss: null gradient"); return V2V_EINVAL; }
    op->a.scale *= (double)weight;
    op->a.gout = grad_out; op->a.da = da;
    op->dtype = dtype; op->backward = true;
    return submit(std::move(op), stream);
}

// torch.optim.Adam semantics (no amsgrad): step = 1-based step count after this update
extern "C" int v2v_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                             float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                             int32_t step, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step < 1) { set_error("adam: bad argument"); return V2V_EINVAL; }
    auto op = std::make_unique<AdamOp>();
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    op->a = AdamArgs{param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, (float)bc1, (float)sqrt(bc2), weight_decay, grad_scale};
    return submit(std::move(op), stream);
}

extern "C" int v2v_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                 float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                 void* state, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || !state) { set_error("adam (device state): bad argument"); return V2V_EINVAL; }
    auto op = std::make_unique<AdamDevOp>();
    op->a = AdamDevArgs{param, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, weight_decay, grad_scale, reinterpret_cast<AdamDevState*>(state)};
    return submit(std::move(op), stream);
}

// Argument checks and the vector split shared by the two weight-averaging entry points.
static int adam_ema_common(AdamEmaArgs& a, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                           int64_t n, float ema_decay) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0) { set_error("adam (ema): bad argument"); return V2V_EINVAL; }
    if (!ema) { set_error("adam (ema): null ema buffer"); return V2V_EINVAL; }
    if (!(ema_decay >= 0.f && ema_decay <= 1.f)) { set_error("adam (ema): ema_decay %g outside [0, 1]", (double)ema_decay); return V2V_EINVAL; }
    const void* bufs[5] = {param, grad, exp_avg, exp_avg_sq, ema};
    const uintptr_t e0 = (uintptr_t)ema, bytes = (uintptr_t)n * 4;
    for (int k = 0; k < 4; ++k) {
        const uintptr_t x0 = (uintptr_t)bufs[k];
        if (e0 < x0 + bytes && x0 < e0 + bytes) { set_error("adam (ema): the ema buffer overlaps another buffer"); return V2V_EINVAL; }
    }
    memset(&a, 0, sizeof(a));
    a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.e = ema; a.n = n;
    const uintptr_t mis = e0 & 15;
    bool same = (mis & 3) == 0;
    for (int k = 0; k < 4; ++k) same = same && ((uintptr_t)bufs[k] & 15) == mis;
    if (same) {
        a.head = (long long)((16 - mis) & 15) / 4;
        if (a.head > n) a.head = n;
        a.nvec = (n - a.head) / 4;
    }
    a.decay = ema_decay;
    a.omd = (float)(1.0 - (double)ema_decay);
    return 0;
}

// v2v_adam_step plus ema = ema_decay * ema + (1 - ema_decay) * param' in the same pass
extern "C" int v2v_adam_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                 int32_t step, float ema_decay, void* stream) {
    auto op = std::make_unique<AdamEmaOp>();
    int rc = adam_ema_common(op->a, param, grad, exp_avg, exp_avg_sq, ema, n, ema_decay);
    if (rc) return rc;
    if (step < 1) { set_error("adam (ema): bad argument"); return V2V_EINVAL; }
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    op->a.lr = lr; op->a.b1 = beta1; op->a.b2 = beta2; op->a.eps = eps; op->a.bc1 = (float)bc1; op->a.bc2_sqrt = (float)sqrt(bc2);
    op->a.wd = weight_decay; op->a.gscale = grad_scale;
    op->dev = false;
    return submit(std::move(op), stream);
}

extern "C" int v2v_adam_step_dev_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                     float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                     void* state, float ema_decay, void* stream) {
    auto op = std::make_unique<AdamEmaOp>();
    int rc = adam_ema_common(op->a, param, grad, exp_avg, exp_avg_sq, ema, n, ema_decay);
    if (rc) return rc;
    if (!state) { set_error("adam (ema, device state): bad argument"); return V2V_EINVAL; }
    op->a.b1 = beta1; op->a.b2 = beta2; op->a.eps = eps; op->a.wd = weight_decay; op->a.gscale = grad_scale;
    op->a.st = reinterpret_cast<AdamDevState*>(state);
    op->dev = true;
    return submit(std::move(op), stream);
}

// ---- guarded forms: extensions, nothing in the reference stands behind them ----
extern "C" int64_t v2v_adam_guard_workspace_bytes(void) { return GUARD_HEADER_BYTES + (int64_t)GUARD_MAX_BLOCKS * sizeof(GuardPartial); }

// the guard block: non-null, 8-byte aligned, overlapping none of `bufs` (n floats each)
static int guard_check(const void* guard, const void* const* bufs, int nbufs, int64_t n, const void* state = nullptr) {
    if (!guard) { set_error("adam (guard): null guard buffer"); return V2V_EINVAL; }
    if ((uintptr_t)guard & 7) { set_error("adam (guard): the guard buffer is not 8-byte aligned"); return V2V_EINVAL; }
    const uintptr_t g0 = (uintptr_t)guard, gbytes = (uintptr_t)v2v_adam_guard_workspace_bytes(), bytes = (uintptr_t)n * 4;
    for (int k = 0; k < nbufs; ++k) {
        const uintptr_t x0 = (uintptr_t)bufs[k];
        if (g0 < x0 + bytes && x0 < g0 + gbytes) { set_error("adam (guard): the guard buffer overlaps another buffer"); return V2V_EINVAL; }
    }
    const uintptr_t s0 = (uintptr_t)state;
    if (state && g0 < s0 + sizeof(AdamDevState) && s0 < g0 + gbytes) { set_error("adam (guard): the guard buffer overlaps the state words"); return V2V_EINVAL; }
    return 0;
}

// launches 1 and 2; `state` may be null (v2v_grad_sumsq)
static int guard_reduce(const float* grad, int64_t n, void* guard, void* state, float grad_scale, float max_norm, int skip_nonfinite,
                        void* stream) {
    auto sq = std::make_unique<GradSumsqOp>();
    memset(&sq->a, 0, sizeof(sq->a));
    sq->a.g = grad; sq->a.n = n; sq->a.gd = reinterpret_cast<AdamGuard*>(guard);
    const uintptr_t mis = (uintptr_t)grad & 15;
    if ((mis & 3) == 0) {
        sq->a.head = (long long)((16 - mis) & 15) / 4;
        if (sq->a.head > n) sq->a.head = n;
        sq->a.nvec = (n - sq->a.head) / 4;
    }
    int rc = submit(std::move(sq), stream);
    if (rc) return rc;
    auto fin = std::make_unique<GuardFinalizeOp>();
    fin->a = FinalizeArgs{reinterpret_cast<AdamGuard*>(guard), reinterpret_cast<AdamDevState*>(state), (int)sumsq_grid(n),
                          grad_scale, max_norm, skip_nonfinite ? 1 : 0};
    return submit(std::move(fin), stream);
}

extern "C" int v2v_grad_sumsq(const float* grad, int64_t n, void* guard, void* stream) {
    if (!grad || n <= 0) { set_error("grad_sumsq: bad argument"); return V2V_EINVAL; }
    const void* bufs[1] = {grad};
    int rc = guard_check(guard, bufs, 1, n);
    if (rc) return rc;
    return guard_reduce(grad, n, guard, nullptr, 1.f, 0.f, 0, stream);
}

extern "C" int v2v_adam_step_dev_guard(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                       float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                       void* state, void* guard, float max_norm, int32_t skip_nonfinite, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || !state) { set_error("adam (guard): bad argument"); return V2V_EINVAL; }
    if (!(max_norm >= 0.f)) { set_error("adam (guard): max_norm %g is negative or NaN", (double)max_norm); return V2V_EINVAL; }
    const void* bufs[4] = {param, grad, exp_avg, exp_avg_sq};
    int rc = guard_check(guard, bufs, 4, n, state);
    if (rc) return rc;
    rc = guard_reduce(grad, n, guard, state, grad_scale, max_norm, skip_nonfinite, stream);
    if (rc) return rc;
    auto op = std::make_unique<AdamGuardOp>();
    op->a = AdamDevArgs{param, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, weight_decay, grad_scale, reinterpret_cast<AdamDevState*>(state)};
    memset(&op->ae, 0, sizeof(op->ae));
    op->gd = reinterpret_cast<const AdamGuard*>(guard); op->ema = false;
    return submit(std::move(op), stream);
}

extern "C" int v2v_adam_step_dev_guard_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                           float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                           void* state, float ema_decay, void* guard, float max_norm, int32_t skip_nonfinite,
                                           void* stream) {
    auto op = std::make_unique<AdamGuardOp>();
    int rc = adam_ema_common(op->ae, param, grad, exp_avg, exp_avg_sq, ema, n, ema_decay);
    if (rc) return rc;
    if (!state) { set_error("adam (guard, ema): bad argument"); return V2V_EINVAL; }
    if (!(max_norm >= 0.f)) { set_error("adam (guard, ema): max_norm %g is negative or NaN", (double)max_norm); return V2V_EINVAL; }
    const void* bufs[5] = {param, grad, exp_avg, exp_avg_sq, ema};
    rc = guard_check(guard, bufs, 5, n, state);
    if (rc) return rc;
    rc = guard_reduce(grad, n, guard, state, grad_scale, max_norm, skip_nonfinite, stream);
    if (rc) return rc;
    op->ae.b1 = beta1; op->ae.b2 = beta2; op->ae.eps = eps; op->ae.wd = weight_decay; op->ae.gscale = grad_scale;
    op->ae.st = reinterpret_cast<AdamDevState*>(state);
    memset(&op->a, 0, sizeof(op->a)); op->a.n = n;
    op->gd = reinterpret_cast<const AdamGuard*>(guard); op->ema = true;
    return submit(std::move(op), stream);
}

extern "C" int v2v_memset_zero(void* p, int64_t bytes, void* stream) {
    if (!p || bytes < 0) { set_error("memset: bad argument"); return V2V_EINVAL; }
    auto op = std::make_unique<MemsetOp>();
    op->p = p; op->bytes = (size_t)bytes;
    return submit(std::move(op), stream);
}
