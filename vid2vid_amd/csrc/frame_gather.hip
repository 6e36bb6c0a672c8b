// uint8 frames at source size -> the uint8 input windows at model size, ONE launch (v2v_gather_frames_u8).
// The reference's loaders bring a decoded frame to the model's size with img.resize((new_w, new_h), Image.NEAREST), __crop and
// FLIP_LEFT_RIGHT (data/base_dataset.py:130-175 with the parameters of get_img_params :85-128).  All three only move bytes, so
// the composition is an integer index map from a destination pixel (y, x) of the H x W result to one source pixel:
//   x' = flip ? W - 1 - x : x;   xr = x' + x1;   src_x = ((2 xr + 1) Ws) / (2 new_w)      (Pillow's nearest filter: the centre of
//   yr = y + y1;                                 src_y = ((2 yr + 1) Hs) / (2 new_h)       the destination pixel, floored)
// with (x1, y1) the crop's corner (0, 0 without a crop stage).  x1 + W <= new_w and y1 + H <= new_h (checked per entry, see
// below) keep src_x in [0, Ws) and src_y in [0, Hs); new_w, Ws <= 16384 keep (2 xr + 1) Ws below 2^31.
//
// src is [F][Hs][Ws][C], dst [D][H][W][C].  Entry e = {src_frame, dst_frame, geom, 0} copies one frame under geoms[geom] =
// {new_w, new_h, x1, y1, flip, 0, 0, 0}; both tables are int32 in device memory and read when the launch runs (blockIdx.y is the
// entry: the words are uniform over a workgroup).  An entry that names a frame or a geometry outside its table, or a geometry
// under which a source index could leave the source frame, returns before it reads or writes anything.
//
// A destination row is W C contiguous bytes.  A workgroup owns 256 / tpr consecutive rows of one entry, tpr threads per row
// (tpr = 16..256, the power of two that covers the row's 16-byte vectors): src_y and both row bases are computed once per row and
// thread; the row leaves as 16-byte stores at aligned addresses, consecutive threads on consecutive vectors; the bytes in front
// of the first and behind the last aligned vector (none where a row is whole vectors, as at every model size: W is a multiple of
// 32 there) leave as single bytes.  A pixel's bytes are loaded as dwords where C is a multiple of 4 and both bases are 4-byte
// aligned (a dword of the row then lies inside one pixel, at a 4-byte aligned source address), else byte by byte; src_x is
// recomputed, in 32-bit integers, when the pixel changes.  Every destination byte of a named frame is written by exactly one
// thread, and no destination byte is read.
#include "v2v_internal.h"

namespace v2v {

struct GatherFramesArgs {
    const unsigned char* src; unsigned char* dst;
    const int* entries; const int* geoms;
    int F, Hs, Ws, D, H, W, C, G;
    int tpr_log2;                        // threads per destination row: 1 << tpr_log2, 16..256
};

static constexpr int GATHER_MAX_SIZE = 16384;
static constexpr int GATHER_MAX_C = 32;

struct GatherGeom { int new_w, W, x1, flip, Ws, C; };

__device__ __forceinline__ int gather_src_x(const GatherGeom& g, int x) {
    const int xr = (g.flip ? g.W - 1 - x : x) + g.x1;
    return (int)(((unsigned)(2 * xr + 1) * (unsigned)g.Ws) / (unsigned)(2 * g.new_w));
}

template <bool DWORD>
__global__ __launch_bounds__(256) void gather_frames_u8_kernel(const GatherFramesArgs a) {
    const int4 ent = reinterpret_cast<const int4*>(a.entries)[blockIdx.y];
    const int sf = ent.x, df = ent.y, gi = ent.z;
    if (sf < 0 || sf >= a.F || df < 0 || df >= a.D || gi < 0 || gi >= a.G) return;
    const int4 gw = reinterpret_cast<const int4*>(a.geoms)[2 * gi];
    const int new_w = gw.x, new_h = gw.y, x1 = gw.z, y1 = gw.w;
    const int flip = a.geoms[8 * gi + 4] != 0;
    if (new_w < 1 || new_w > GATHER_MAX_SIZE || new_h < 1 || new_h > GATHER_MAX_SIZE || x1 < 0 || y1 < 0 ||
        x1 > new_w - a.W || y1 > new_h - a.H) return;
    const int tpr = 1 << a.tpr_log2;
    const int y = (int)blockIdx.x * (256 >> a.tpr_log2) + ((int)threadIdx.x >> a.tpr_log2);
    if (y >= a.H) return;
    const int lane = threadIdx.x & (tpr - 1);
    const int sy = (int)(((unsigned)(2 * (y + y1) + 1) * (unsigned)a.Hs) / (unsigned)(2 * new_h));
    const GatherGeom g{new_w, a.W, x1, flip, a.Ws, a.C};
    const int len = a.W * a.C;                                           // bytes of a destination row
    const unsigned char* const srow = a.src + ((long long)sf * a.Hs + sy) * a.Ws * a.C;
    unsigned char* const drow = a.dst + ((long long)df * a.H + y) * len;
    int head = (int)((16 - (reinterpret_cast<uintptr_t>(drow) & 15)) & 15);      // bytes in front of the first aligned vector
    if (head > len) head = len;
    const int nvec = (len - head) >> 4;
    const int tail0 = head + 16 * nvec;                                  // the bytes behind the last whole vector start here
    for (int v = lane; v < nvec; v += tpr) {
        const int o = head + 16 * v;
        uint4 pk;
        if constexpr (DWORD) {                                          // o is a multiple of 4: a dword lies inside one pixel
            unsigned w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int b = o + 4 * q;
                const int x = b / a.C, c = b - x * a.C;
                w[q] = *reinterpret_cast<const unsigned*>(srow + gather_src_x(g, x) * a.C + c);
            }
            pk = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            int x = o / a.C, c = o - x * a.C;
            const unsigned char* p = srow + gather_src_x(g, x) * a.C;
            unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                w[i >> 2] |= (unsigned)p[c] << (8 * (i & 3));
                if (++c == a.C) {
                    c = 0;
                    if (++x < a.W) p = srow + gather_src_x(g, x) * a.C;
                }
            }
            pk = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(drow + o) = pk;
    }
    // the generic ends of a row that is not whole aligned vectors
    const int ends = head + (len - tail0);
    for (int i = lane; i < ends; i += tpr) {
        const int o = i < head ? i : tail0 + (i - head);
        const int x = o / a.C, c = o - x * a.C;
        drow[o] = srow[gather_src_x(g, x) * a.C + c];
    }
}

struct GatherFramesOp : Op {
    GatherFramesArgs a; int E; bool dword;
    int launch(hipStream_t s) override {
        const int rows = 256 >> a.tpr_log2;
        const dim3 g((unsigned)ceil_div(a.H, rows), (unsigned)E), b(256);
        if (dword) hipLaunchKernelGGL(gather_frames_u8_kernel<true>, g, b, 0, s, a);
        else       hipLaunchKernelGGL(gather_frames_u8_kernel<false>, g, b, 0, s, a);
        return check_launch();
    }
    const char* name() const override { return "gather_frames_u8"; }
};

static bool gather_overlap(const void* p, long long pb, const void* q, long long qb) {
    const char* a = (const char*)p; const char* b = (const char*)q;
    return a < b + qb && b < a + pb;
}

}  // namespace v2v

using namespace v2v;

extern "C" int v2v_gather_frames_u8(const uint8_t* src, int32_t F, int32_t Hs, int32_t Ws, uint8_t* dst, int32_t D, int32_t H,
                                    int32_t W, int32_t C, const int32_t* entries, int32_t E, const int32_t* geoms, int32_t G,
                                    void* stream) {
    if (!src || !dst || !entries || !geoms) { set_error("gather_frames_u8: null pointer"); return V2V_EINVAL; }
    if (C < 1 || C > GATHER_MAX_C) { set_error("gather_frames_u8: %d channels (1..%d)", C, GATHER_MAX_C); return V2V_EINVAL; }
    if (Hs < 1 || Hs > GATHER_MAX_SIZE || Ws < 1 || Ws > GATHER_MAX_SIZE || H < 1 || H > GATHER_MAX_SIZE || W < 1 ||
        W > GATHER_MAX_SIZE || F < 1 || D < 1 || G < 1) {
        set_error("gather_frames_u8: sizes within 1..%d, at least one frame on either side and one geometry", GATHER_MAX_SIZE);
        return V2V_EINVAL;
    }
    if (E < 0 || E > 65535) { set_error("gather_frames_u8: %d entries (0..65535)", E); return V2V_EINVAL; }
    if (((reinterpret_cast<uintptr_t>(entries) | reinterpret_cast<uintptr_t>(geoms)) & 15) != 0) {
        set_error("gather_frames_u8: the tables are 16-byte aligned"); return V2V_EINVAL;
    }
    const long long src_bytes = (long long)F * Hs * Ws * C, dst_bytes = (long long)D * H * W * C;
    if (gather_overlap(src, src_bytes, dst, dst_bytes) || gather_overlap(entries, 16ll * (E > 0 ? E : 1), dst, dst_bytes) ||
        gather_overlap(geoms, 32ll * G, dst, dst_bytes)) {
        set_error("gather_frames_u8: dst overlaps src or a table"); return V2V_EINVAL;
    }
    if (E == 0) return 0;
    const int vecs = (int)ceil_div((long long)W * C, 16);
    int tpr_log2 = 4;
    while (tpr_log2 < 8 && (1 << tpr_log2) < vecs) ++tpr_log2;
    auto op = std::make_unique<GatherFramesOp>();
    op->a = GatherFramesArgs{src, dst, entries, geoms, F, Hs, Ws, D, H, W, C, G, tpr_log2};
    op->E = E;
    op->dword = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) == 0;
    return submit(std::move(op), stream);
}
