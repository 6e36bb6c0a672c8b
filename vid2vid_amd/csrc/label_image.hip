// The input picture of a label-model inference frame, ONE launch (v2v_label_image): what the reference's test.py
// saves beside every generated frame, util.tensor2label(real_A_last, label_nc) (util/util.py:73-87, Colorize :197-212), made
// straight from the label map and the instance map of the newest frame instead of from the (label_nc + 1) fp32 one-hot planes.
// The planes hold  plane c = (label == c), c < label_nc  (onehot_planar_kernel: label = (int)stored value)  and, with an
// instance map, plane label_nc = get_edges' 4-neighbour rule (models/base_model.py:146-152); tensor2label_kernel takes the
// first maximum over them and colours it through cmap, black for an index >= label_nc.  So, per pixel,
//   0 <= label < label_nc            -> cmap[label]      (its plane is 1 and comes before the edge plane)
//   otherwise (all one-hot planes 0) -> black on an instance edge (the edge plane is the only 1), cmap[0] off one (all planes 0);
//   one plane in all (label_nc == 1, no instance map): tensor2label colours the stored VALUE: 1 (label 0) -> black, 0 -> cmap[0].
// The instance map is read only by runs that hold such a label: none in a well-formed label map.
//
// Purely bandwidth bound.  A thread owns a run of R consecutive pixels of one row (R = 16 where rows have 16 pixels, else 4): one
// vector load of their labels where the run is whole and aligned, the palette from an LDS copy (256 packed words, black
// behind label_nc) filled once per workgroup, the 3 R bytes of the run packed in registers and stored as 16-byte vectors
// where the run starts on one, else as whole dwords between at most 3 leading and 3 trailing single bytes.  Image s is
// blockIdx.y; its runs go to the workgroups of a capped grid by grid stride.
#include "v2v_internal.h"

namespace v2v {

struct LabelImageArgs {
    const void* labels; const void* inst; const unsigned char* cmap; unsigned char* out;
    const int* mode; const int* row_slot;
    int K, S, T, H, W, label_nc, planes;     // planes: label_nc + (inst ? 1 : 0), the planes real_A_last would have
};

static constexpr int LABEL_IMAGE_GRID_CAP = 256;        // workgroups per image

// the row of image s: the first k with row_slot[k] == s (k == s without row_slot) whose mode is 0 or 1; -1: zeros (v2v_frames_u8)
__device__ __forceinline__ int label_image_row(const LabelImageArgs& a, int s) {
    for (int k = 0; k < a.K; ++k) {
        if ((a.row_slot ? a.row_slot[k] : k) != s) continue;
        const int m = a.mode ? a.mode[k] : 0;
        if (m == 0 || m == 1) return k;
    }
    return -1;
}

// v[0..n) <- p[0..n): 16-byte (4-byte for 4 bytes in all) vector loads where the run is whole and starts on one
template <typename T, int R>
__device__ __forceinline__ void load_run(const T* p, int n, T (&v)[R]) {
    constexpr int BYTES = R * (int)sizeof(T);
    constexpr int VB = BYTES < 16 ? 4 : 16;
    static_assert(BYTES % VB == 0, "whole vectors");
    if (n == R && (reinterpret_cast<uintptr_t>(p) & (VB - 1)) == 0) {
        if constexpr (VB == 4) {
            const unsigned w = *reinterpret_cast<const unsigned*>(p);
            __builtin_memcpy(v, &w, 4);
        } else {
            uint4 w[BYTES / 16];
#pragma unroll
            for (int i = 0; i < BYTES / 16; ++i) w[i] = reinterpret_cast<const uint4*>(p)[i];
            __builtin_memcpy(v, w, BYTES);
        }
    } else {
#pragma unroll
        for (int i = 0; i < R; ++i) v[i] = i < n ? p[i] : T(0);
    }
}

template <typename LT, typename IT, int R>
__global__ __launch_bounds__(256) void label_image_kernel(const LabelImageArgs a) {
    constexpr int NW = 3 * R / 4;                    // dwords of a whole run
    constexpr unsigned BLACK = 255;                  // label_nc <= 255: the palette's last word is always black
    __shared__ unsigned pal[256];
    {
        const int c = threadIdx.x;
        unsigned w = 0;
        if (c < a.label_nc) w = a.cmap[3 * c] | ((unsigned)a.cmap[3 * c + 1] << 8) | ((unsigned)a.cmap[3 * c + 2] << 16);
        pal[c] = w;
    }
    __syncthreads();
    const int s = blockIdx.y;
    const int row = label_image_row(a, s);
    const long long hw = (long long)a.H * a.W;
    const int rpr = (a.W + R - 1) / R;               // runs per row
    const long long runs = (long long)a.H * rpr;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long frame = ((long long)(row < 0 ? 0 : row) * a.T + (a.T - 1)) * hw;       // the newest frame of the row's sample
    const LT* const labels = reinterpret_cast<const LT*>(a.labels) + frame;
    const IT* const inst = a.inst ? reinterpret_cast<const IT*>(a.inst) + frame : nullptr;
    unsigned char* const out = a.out + (long long)s * hw * 3;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < runs; r += stride) {
        const int y = (int)(r / rpr);
        const int x0 = (int)(r - (long long)y * rpr) * R;
        const int n = a.W - x0 < R ? a.W - x0 : R;
        const long long p0 = (long long)y * a.W + x0;
        unsigned w[NW + 1];
#pragma unroll
        for (int j = 0; j <= NW; ++j) w[j] = 0u;
        if (row >= 0) {
            LT lab[R];
            load_run<LT, R>(labels + p0, n, lab);
            int idx[R];
            bool outside = false;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                idx[i] = (int)lab[i];                // as onehot_planar_kernel reads a label
                outside |= i < n && (idx[i] < 0 || idx[i] >= a.label_nc);
            }
            bool edge[R];
#pragma unroll
            for (int i = 0; i < R; ++i) edge[i] = false;
            if (inst && outside) {
                IT c[R], up[R], dn[R];
                load_run<IT, R>(inst + p0, n, c);
                const bool has_up = y > 0, has_dn = y + 1 < a.H, has_l = x0 > 0, has_r = x0 + n < a.W;
                if (has_up) load_run<IT, R>(inst + p0 - a.W, n, up);
                if (has_dn) load_run<IT, R>(inst + p0 + a.W, n, dn);
                const IT lft = has_l ? inst[p0 - 1] : IT(0);
                const IT rgt = has_r ? inst[p0 + n] : IT(0);
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    bool e = false;
                    if (i > 0) e |= c[i - 1] != c[i];
                    else       e |= has_l && lft != c[0];
                    if (i + 1 < n)       e |= c[(i + 1) % R] != c[i];          // (n <= R: the index never wraps)
                    else if (i + 1 == n) e |= has_r && rgt != c[i];
                    if (has_up) e |= up[i] != c[i];
                    if (has_dn) e |= dn[i] != c[i];
                    edge[i] = e;
                }
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                unsigned k;
                if (a.planes == 1) k = idx[i] == 0 ? BLACK : 0u;
                else if (idx[i] >= 0 && idx[i] < a.label_nc) k = (unsigned)idx[i];
                else k = edge[i] ? BLACK : 0u;
                const unsigned col = i < n ? pal[k] : 0u;
                const int word = (3 * i) >> 2, sh = ((3 * i) & 3) * 8;
                w[word] |= col << sh;
                if (sh > 8) w[word + 1] |= col >> (32 - sh);
            }
        }
        // ---- store the 3 n bytes of the run
        unsigned char* const dst = out + p0 * 3;
        const int nbytes = 3 * n;
        const uintptr_t addr = reinterpret_cast<uintptr_t>(dst);
        if (R == 16 && n == R && (addr & 15) == 0) {
#pragma unroll
            for (int j = 0; j < NW / 4; ++j)
                reinterpret_cast<uint4*>(dst)[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
        } else {
            int head = (int)((4 - (addr & 3)) & 3);                  // single bytes up to the first whole dword
            if (head > nbytes) head = nbytes;
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b < head) dst[b] = (unsigned char)(w[0] >> (8 * b));
            const int nd = (nbytes - head) >> 2, tail = (nbytes - head) & 3;
            unsigned* const dw = reinterpret_cast<unsigned*>(dst + head);
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const unsigned v = __builtin_amdgcn_alignbyte(w[j + 1], w[j], (unsigned)head);     // bytes head + 4 j .. of the run
                if (j < nd) dw[j] = v;
                else if (j == nd) {
#pragma unroll
                    for (int b = 0; b < 3; ++b)
                        if (b < tail) dst[head + 4 * nd + b] = (unsigned char)(v >> (8 * b));
                }
            }
        }
    }
}

struct LabelImageOp : Op {
    LabelImageArgs a; int in_u8;
    template <typename LT, typename IT>
    void go(hipStream_t s) {
        const dim3 b(256);
        if (a.W >= 16) {
            long long gx = ceil_div((long long)a.H * ceil_div(a.W, 16), 256);
            if (gx > LABEL_IMAGE_GRID_CAP) gx = LABEL_IMAGE_GRID_CAP;
            hipLaunchKernelGGL((label_image_kernel<LT, IT, 16>), dim3((unsigned)gx, (unsigned)a.S), b, 0, s, a);
        } else {
            long long gx = ceil_div((long long)a.H * ceil_div(a.W, 4), 256);
            if (gx > LABEL_IMAGE_GRID_CAP) gx = LABEL_IMAGE_GRID_CAP;
            hipLaunchKernelGGL((label_image_kernel<LT, IT, 4>), dim3((unsigned)gx, (unsigned)a.S), b, 0, s, a);
        }
    }
    int launch(hipStream_t s) override {
        if (in_u8) go<unsigned char, int>(s);
        else       go<float, float>(s);
        return check_launch();
    }
    const char* name() const override { return "label_image"; }
};

static bool ranges_overlap(const void* p, long long pb, const void* q, long long qb) {
    const char* a = (const char*)p; const char* b = (const char*)q;
    return p && q && a < b + qb && b < a + pb;
}

}  // namespace v2v

using namespace v2v;

extern "C" int v2v_label_image(const void* labels, const void* inst, int32_t in_u8, const uint8_t* cmap, int32_t label_nc,
                               uint8_t* out, const int32_t* mode, const int32_t* row_slot, int32_t K, int32_t S, int32_t T,
                               int32_t H, int32_t W, void* stream) {
    if (!labels || !cmap || !out) { set_error("label_image: null pointer"); return V2V_EINVAL; }
    if (label_nc < 1 || label_nc > 255) {
        set_error("label_image: label_nc %d (1..255: the palette and its black entry are 256 words of LDS)", label_nc); return V2V_EINVAL;
    }
    if ((in_u8 != 0 && in_u8 != 1) || K < 1 || S < K || S > 65535 || T < 1 || H < 1 || W < 1 ||
        (long long)K * T * H * W > 0x7fffffffffffll) {
        set_error("label_image: bad argument (1 <= K <= S <= 65535 rows / images, T, H, W >= 1)"); return V2V_EINVAL;
    }
    if (!row_slot && K != S) { set_error("label_image: without row_slot row k is image k: K == S"); return V2V_EINVAL; }
    const int lsize = in_u8 ? 1 : 4;
    if ((((uintptr_t)labels & (lsize - 1)) | ((uintptr_t)inst & 3) | ((uintptr_t)mode & 3) | ((uintptr_t)row_slot & 3)) != 0) {
        set_error("label_image: misaligned buffer (fp32 labels, inst, mode and row_slot are 4-byte aligned)"); return V2V_EINVAL;
    }
    const long long hw = (long long)H * W;
    const long long out_bytes = (long long)S * hw * 3, in_elems = (long long)K * T * hw;
    if (ranges_overlap(out, out_bytes, labels, in_elems * lsize) || ranges_overlap(out, out_bytes, inst, in_elems * 4) ||
        ranges_overlap(out, out_bytes, cmap, 3ll * label_nc) || ranges_overlap(out, out_bytes, mode, 4ll * K) ||
        ranges_overlap(out, out_bytes, row_slot, 4ll * K)) {
        set_error("label_image: out must not overlap an input"); return V2V_EINVAL;
    }
    auto op = std::make_unique<LabelImageOp>();
    op->a = LabelImageArgs{labels, inst, cmap, out, mode, row_slot, K, S, T, H, W, label_nc, label_nc + (inst ? 1 : 0)};
    op->in_u8 = in_u8;
    return submit(std::move(op), stream);
}
