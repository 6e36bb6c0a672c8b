// 16-byte channel-vector accesses of the NHWC layout kernels, and the one work item of the previous-frame window pack that the
// frame heads share (frame_prologue_row in pointwise.hip, image_prologue_kernel in image_prologue.hip).
#pragma once
#include "v2v_internal.h"

namespace v2v {

// one 16-byte store of VEC consecutive channels (8 bf16 / 4 fp32) -- the layout kernels used to leave through VEC separate
// 2- / 4-byte stores (pack_concat 0.93 ms, pack_nchw_to_nhwc 1.6 ms, unpack 1.1 ms per launch at 2048x1024: 8.5 % of a training
// chunk, profiles/r06_v14_train_kernel_stats.txt, for tensors that take a tenth of that at the HBM rate)
__device__ __forceinline__ void store_vec(bf16_t* y, long long e, const float (&v)[8]) {
    uint4 pk;
    pk.x = pack_bf16x2(v[0], v[1]); pk.y = pack_bf16x2(v[2], v[3]); pk.z = pack_bf16x2(v[4], v[5]); pk.w = pack_bf16x2(v[6], v[7]);
    *reinterpret_cast<uint4*>(y + e) = pk;
}
__device__ __forceinline__ void store_vec(float* y, long long e, const float (&v)[4]) {
    *reinterpret_cast<float4*>(y + e) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void load_vec(const bf16_t* y, long long e, float (&v)[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(y + e);
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u); v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
    v[4] = __uint_as_float(t.z << 16); v[5] = __uint_as_float(t.z & 0xffff0000u); v[6] = __uint_as_float(t.w << 16); v[7] = __uint_as_float(t.w & 0xffff0000u);
}
__device__ __forceinline__ void load_vec(const float* y, long long e, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(y + e);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

// Channel vector cv of pixel pix of one sample's window pack: window planar fp32 [win_C][hw] -> y NHWC [hw][c_stride], bit for
// bit pack_nchw_to_nhwc_kernel (pad channels zero); the fp32 values of the window's last `last_C` planes also go to `last`
// ([last_C][hw], may be null).  Callers walk pix fastest: consecutive threads read consecutive pixels of one plane.
template <typename T>
__device__ __forceinline__ void window_pack_item(const float* window, T* y, float* last, long long pix, int cv, long long hw,
                                                 int win_C, int c_stride, int last_C) {
    constexpr int VEC = ElemTraits<T>::VEC;
    float vals[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        const int c = cv * VEC + q;
        vals[q] = c < win_C ? window[c * hw + pix] : 0.f;
        if (last && c < win_C && c >= win_C - last_C) last[(c - (win_C - last_C)) * hw + pix] = vals[q];
    }
    store_vec(y, pix * c_stride + cv * VEC, vals);
}

}  // namespace v2v
